/*
 * targets_emu.cpp -- the target-set bodies (cbc_amd/csrc/cbc_targets_body.h) on the CPU through the lock-step wave emulation.
 * TEST AID ONLY: the keep rule over the interval table, the count / write passes for reads and SAM, and the depth passes in
 * the compressed coordinate are checked against the Python models and the single-region emulations under ASan-able host
 * code before anything runs on a GPU.  The front of the depth call and the scans between the passes are those of
 * tests/emu/post_emu.h.  Every table is copied into an allocation of its exact size, so an index past it is an ASan finding.
 */
#include "../emu/post_emu.h"

/* the span-reporting decoder over every block of the batch */
extern "C" __attribute__((visibility("default")))
int emu_targets_decode(const cbc_dec_device_batch *b, uint32_t smax) { return emu_decode_blocks<WP, true>(b, smax); }

/* reads (sam = 0) or SAM lines (sam != 0): count pass, scan, write pass (n_waves wavefronts per block, one after the other).
 * out[0] = text bytes, out[1] = reads kept.  Returns -1 (CBC_E_ARG) with out[] set and nothing written when the text does not
 * fit text_cap, as cbc_gpu_decode_targets does. */
extern "C" __attribute__((visibility("default")))
int emu_targets(const cbc_read_rec *recs, uint64_t n_recs, const uint8_t *seq, uint64_t seq_bytes, const cbc_dec_block_desc *blocks,
                const uint64_t *window_start, const cbc_block_result *dec_results, uint32_t n_blocks, const uint32_t *block_name,
                const uint8_t *names, uint32_t names_bytes, const uint32_t *iv, uint32_t n_iv, const uint32_t *block_iv, int sam,
                uint8_t *text, uint64_t text_cap, uint32_t n_waves, uint64_t *out)
{
    std::vector<uint32_t> ivv(iv, iv + 2u * (size_t)n_iv), biv(block_iv, block_iv + 2u * (size_t)n_blocks);
    std::vector<cbc_block_result> counts(n_blocks);
    std::vector<uint64_t> offs(n_blocks + 1u);
    cbc_targets_args A;
    memset(&A, 0, sizeof A);
    A.S.R.recs = recs; A.S.R.seq = seq; A.S.R.blocks = blocks; A.S.R.window_start = window_start; A.S.R.dec_results = dec_results;
    A.S.R.counts = counts.data(); A.S.R.offsets = offs.data(); A.S.R.text = text; A.S.R.text_cap = text_cap; A.S.R.n_recs = n_recs;
    A.S.R.seq_bytes = seq_bytes; A.S.R.beg = 1u; A.S.R.end = UINT64_MAX; A.S.R.n_blocks = n_blocks;
    A.S.block_name = block_name; A.S.names = names; A.S.names_bytes = names_bytes; A.S.region = 0u;
    A.iv = ivv.data(); A.block_iv = biv.data(); A.n_iv = n_iv;
    g_emu_errors = 0;
    for (uint32_t b = 0; b < n_blocks; b++) { if (sam) cbc_targets_sam_count<WP>(A, b); else cbc_targets_count<WP>(A, b); }
    scan(counts.data(), offs.data(), n_blocks);
    out[0] = offs[n_blocks]; out[1] = 0;
    for (uint32_t b = 0; b < n_blocks; b++) out[1] += counts[b].n_symbols;
    if (out[0] > text_cap) return CBC_E_ARG;
    for (uint32_t b = 0; b < n_blocks; b++)
        for (uint32_t w = 0; w < n_waves; w++) {
            if (sam) cbc_targets_sam_write<WP>(A, b, w, n_waves); else cbc_targets_write<WP>(A, b, w, n_waves);
        }
    return g_emu_errors ? -100 : 0;
}

/* the depth of ONE contig's intervals (iv: its n_iv pairs; block_iv relative to them), every pass in the order of
 * cbc_gpu_decode_targets.  out[0] = text bytes, out[1] = lines, out[2] = reads counted, out[3] = change points, out[4] = words
 * of the difference array. */
extern "C" __attribute__((visibility("default")))
int emu_targets_depth(const cbc_read_rec *recs, uint64_t n_recs, const uint8_t *seq, uint64_t seq_bytes, const cbc_dec_block_desc *blocks,
                      const uint64_t *window_start, const cbc_block_result *dec_results, uint32_t n_blocks, const uint8_t *name,
                      uint32_t name_len, const uint32_t *iv, uint32_t n_iv, const uint32_t *block_iv, uint32_t exclude,
                      uint8_t *text, uint64_t text_cap, uint64_t *out)
{
    g_emu_errors = 0;
    out[0] = out[1] = out[2] = out[3] = out[4] = 0;
    if (n_recs > 0x3fffffffull || n_iv == 0) return CBC_E_ARG;
    emu_depth_front F;
    if (F.intervals(iv, n_iv, block_iv, n_blocks)) return CBC_E_ARG;
    const uint64_t d_words = F.d_words;
    const uint32_t cp_cap = (uint32_t)(2u * n_recs + 2u * (uint64_t)n_iv), n_ttiles = (cp_cap + CBC_DEPTH_LINES - 1u) / CBC_DEPTH_LINES;
    std::vector<cbc_block_result> counts(n_ttiles + 1u);
    std::vector<uint64_t> toff(n_ttiles + 1u);
    std::vector<uint8_t> nm(name, name + name_len);
    F.tables(recs, n_recs, seq, seq_bytes, blocks, window_start, dec_results, n_blocks, exclude, cp_cap);
    cbc_tdepth_args &A = F.A;
    A.D.R.counts = counts.data(); A.D.R.offsets = toff.data(); A.D.R.text = text; A.D.R.text_cap = text_cap;
    A.D.name = nm.data(); A.D.name_len = name_len;
    F.mark();
    F.points();                                                      /* a finding is counted; the text passes still run */
    for (uint32_t t = 0; t < n_ttiles; t++) cbc_targets_depth_count<WP>(A, t);
    scan(counts.data(), toff.data(), n_ttiles);
    out[0] = toff[n_ttiles]; out[1] = F.ctr[1]; out[2] = F.ctr[0]; out[3] = F.ncp; out[4] = d_words;
    if (out[0] > text_cap) return CBC_E_ARG;
    for (uint32_t t = 0; t < n_ttiles; t++) cbc_targets_depth_write<WP>(A, t);
    return g_emu_errors ? -100 : 0;
}
