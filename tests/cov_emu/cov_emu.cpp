/*
 * cov_emu.cpp -- the coverage-summary bodies (cbc_amd/csrc/cbc_cov_body.h) on the CPU through the lock-step wave emulation.
 * TEST AID ONLY: the weights, apply and lookup passes are run behind the emulated span decoder and the mark / tile / compact
 * passes of one contig's compressed coordinate (the order of cbc_gpu_decode_coverage), or straight on change points the test
 * fabricates (depths and run lengths whose products pass 2^32), under ASan-able host code before anything runs on a GPU.  The
 * front of the call, the scans between the passes and the passes themselves are those of tests/emu/post_emu.h.  Every table the
 * passes touch is an allocation of its exact size, so an index past it is an ASan finding.
 */
#include "../emu/post_emu.h"

/* the span-reporting decoder over every block of the batch */
extern "C" __attribute__((visibility("default")))
int emu_cov_decode(const cbc_dec_device_batch *b, uint32_t smax) { return emu_decode_blocks<WP, true>(b, smax); }

/* fabricated change points straight into the four passes (cp_cap = ncp: the tables are exactly as long as the tiles assume) */
extern "C" __attribute__((visibility("default")))
int emu_cov_points(const uint32_t *cp_pos, const uint32_t *cp_dep, uint32_t ncp, uint32_t slots, uint32_t min_depth,
                   const uint32_t *q, uint32_t n_q, uint64_t *sum, uint32_t *covered)
{
    g_emu_errors = 0;
    if (min_depth < 1u) return CBC_E_ARG;
    for (uint32_t i = 0; i < n_q; i++) if (q[2 * i] > slots || q[2 * i + 1] > slots - q[2 * i]) return CBC_E_ARG;
    cov_passes(cp_pos, cp_dep, ncp, ncp, slots, min_depth, q, n_q, sum, covered);
    return g_emu_errors ? -100 : 0;
}

/* ONE contig's call (iv: its n_iv merged intervals; block_iv relative to them), every pass in the order of
 * cbc_gpu_decode_coverage.  out[0] = reads counted, out[1] = change points, out[2] = slots.  CBC_E_BLOCK when a block of the
 * call failed to decode (it marked nothing; the results are those of the other blocks). */
extern "C" __attribute__((visibility("default")))
int emu_cov(const cbc_read_rec *recs, uint64_t n_recs, const uint8_t *seq, uint64_t seq_bytes, const cbc_dec_block_desc *blocks,
            const uint64_t *window_start, const cbc_block_result *dec_results, uint32_t n_blocks, const uint32_t *iv, uint32_t n_iv,
            const uint32_t *block_iv, uint32_t exclude, uint32_t min_depth, const uint32_t *q, uint32_t n_q, uint64_t *sum,
            uint32_t *covered, uint64_t *out)
{
    g_emu_errors = 0;
    out[0] = out[1] = out[2] = 0;
    for (uint32_t i = 0; i < n_q; i++) { sum[i] = 0; covered[i] = 0; }
    if (n_recs > 0x3fffffffull || n_iv == 0 || min_depth < 1u) return CBC_E_ARG;
    emu_depth_front F;
    if (F.intervals(iv, n_iv, block_iv, n_blocks)) return CBC_E_ARG;
    const uint64_t d_words = F.d_words;
    for (uint32_t i = 0; i < n_q; i++) if (q[2 * i] > d_words || q[2 * i + 1] > d_words - q[2 * i]) return CBC_E_ARG;
    const uint32_t cp_cap = (uint32_t)(2u * n_recs + 2u * (uint64_t)n_iv);
    F.tables(recs, n_recs, seq, seq_bytes, blocks, window_start, dec_results, n_blocks, exclude, cp_cap);
    F.mark();
    if (F.points()) return -100;
    cov_passes(F.cp_pos.data(), F.cp_dep.data(), F.ncp, cp_cap, (uint32_t)d_words, min_depth, q, n_q, sum, covered);
    out[0] = F.ctr[0]; out[1] = F.ncp; out[2] = d_words;
    if (g_emu_errors) return -100;
    for (uint32_t b = 0; b < n_blocks; b++) if (dec_results[b].status != CBC_ST_OK) return CBC_E_BLOCK;
    return 0;
}
