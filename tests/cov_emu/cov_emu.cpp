/*
 * cov_emu.cpp -- the coverage-summary bodies (cbc_amd/csrc/cbc_cov_body.h) on the CPU through the lock-step wave emulation.
 * TEST AID ONLY: the weights, apply and lookup passes are run behind the emulated span decoder and the mark / tile / compact
 * passes of one contig's compressed coordinate (the order of cbc_gpu_decode_coverage), or straight on change points the test
 * fabricates (depths and run lengths whose products pass 2^32), under ASan-able host code before anything runs on a GPU.  The
 * scans between the passes are the host loop below (on the device: cbc_scan_sizes_kernel).  Every table the new passes touch is
 * an allocation of its exact size, so an index past it is an ASan finding.
 */
#include <vector>
#include "../depth_emu/wave_emu_depth.h"
#include "../../cbc_amd/csrc/cbc_encode_body.h"
#include "../../cbc_amd/csrc/cbc_decode_body.h"
#include "../../cbc_amd/csrc/cbc_plan.h"
#include "../../cbc_amd/csrc/cbc_cov_body.h"

static int g_emu_errors = 0;
extern "C" void emu_oob(const char *what) { fprintf(stderr, "[emu] invariant violated: %s\n", what); g_emu_errors++; }

/* the span-reporting decoder over every block of the batch */
extern "C" __attribute__((visibility("default")))
int emu_cov_decode(const cbc_dec_device_batch *b, uint32_t smax)
{
    cbc_dec_args A;
    memset(&A, 0, sizeof A);
    A.in = b->d_in; A.blocks = b->d_blocks; A.ref = b->d_ref; A.recs = b->d_recs; A.seq = b->d_seq; A.results = b->d_results;
    A.in_bytes = b->in_bytes; A.ref_bytes = b->ref_bytes; A.n_recs = b->n_recs; A.seq_bytes = b->seq_bytes;
    A.n_blocks = b->n_blocks; A.cap_pos = b->caps.cap_pos; A.cap_var = b->caps.cap_var;
    A.var_scratch = b->d_var_scratch; A.var_scratch_words = b->var_scratch_words;
    g_emu_errors = 0;
    uint32_t words = cbc_plan_dec_lds_bytes(&b->caps) / 4;
    for (uint32_t blk = 0; blk < b->n_blocks; blk++) {
        std::vector<uint32_t> lds(words, 0xdeadbeefu);
        cbc_decode_stream<WaveEmuDepth, true>(A, blk, lds.data(), smax);
    }
    return g_emu_errors ? -100 : 0;
}

static void scan(const cbc_block_result *r, uint64_t *off, uint32_t n)
{
    uint64_t run = 0;
    for (uint32_t i = 0; i < n; i++) { off[i] = run; run += r[i].status == CBC_ST_OK ? r[i].nbytes : 0u; }
    off[n] = run;
}

/* weights, scans, apply, lookup over the first ncp change points; cp_cap sizes the tiles as the device call does */
static void cov_passes(const uint32_t *cp_pos, const uint32_t *cp_dep, uint32_t ncp, uint32_t cp_cap, uint32_t slots, uint32_t min_depth,
                       const uint32_t *q, uint32_t n_q, uint64_t *sum, uint32_t *covered)
{
    const uint32_t n_ttiles = (cp_cap + CBC_DEPTH_LINES - 1u) / CBC_DEPTH_LINES;
    std::vector<uint32_t> pos(cp_pos, cp_pos + ncp), dep(cp_dep, cp_dep + ncp), qq(q, q + 2u * (size_t)n_q);
    std::vector<uint32_t> pre_lo(ncp, 0xEEEEEEEEu), pre_hi(ncp, 0xEEEEEEEEu), pre_cov(ncp, 0xEEEEEEEEu), s(2u * (size_t)n_q, 0xEEEEEEEEu), c(n_q, 0xEEEEEEEEu);
    std::vector<cbc_block_result> tl(n_ttiles), th(n_ttiles), tc(n_ttiles);
    std::vector<uint64_t> ol(n_ttiles + 1u), oh(n_ttiles + 1u), oc(n_ttiles + 1u);
    const uint64_t cnt_off[1] = { ncp };                            /* n_tiles = 0: cnt_off[n_tiles] is the count */
    cbc_cov_args A;
    memset(&A, 0, sizeof A);
    A.cp_pos = pos.data(); A.cp_dep = dep.data(); A.cnt_off = cnt_off; A.n_tiles = 0u;
    A.tile_wlo = tl.data(); A.tile_whi = th.data(); A.tile_cov = tc.data(); A.wlo_off = ol.data(); A.whi_off = oh.data(); A.cov_off = oc.data();
    A.pre_lo = pre_lo.data(); A.pre_hi = pre_hi.data(); A.pre_cov = pre_cov.data(); A.q = qq.data(); A.sum = s.data(); A.covered = c.data();
    A.cp_cap = cp_cap; A.n_ttiles = n_ttiles; A.n_q = n_q; A.min_depth = min_depth; A.slots = slots;
    for (uint32_t t = 0; t < n_ttiles; t++) cbc_cov_weights<WaveEmuDepth>(A, t);
    scan(tl.data(), ol.data(), n_ttiles); scan(th.data(), oh.data(), n_ttiles); scan(tc.data(), oc.data(), n_ttiles);
    for (uint32_t t = 0; t < n_ttiles; t++) cbc_cov_apply<WaveEmuDepth>(A, t);
    for (uint32_t i = 0; i < ncp; i++) if (pre_lo[i] == 0xEEEEEEEEu && pre_hi[i] == 0xEEEEEEEEu && pre_cov[i] == 0xEEEEEEEEu) { emu_oob("a prefix was not written"); break; }
    for (uint32_t w = 0; w < (n_q + 63u) / 64u; w++) cbc_cov_lookup<WaveEmuDepth>(A, w);
    for (uint32_t i = 0; i < n_q; i++) { sum[i] = (uint64_t)s[2u * i] | ((uint64_t)s[2u * i + 1u] << 32); covered[i] = c[i]; }
}

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
    std::vector<uint32_t> ivv(iv, iv + 2u * (size_t)n_iv), biv(block_iv, block_iv + 2u * (size_t)n_blocks), ioff(n_iv + 1u);
    uint64_t run = 0;
    for (uint32_t i = 0; i < n_iv; i++) {
        if (iv[2 * i] < 1 || iv[2 * i] > iv[2 * i + 1] || iv[2 * i + 1] > CBC_SAM_MAX_POS || (i && iv[2 * i] <= iv[2 * i - 1] + 1u)) return CBC_E_ARG;
        ioff[i] = (uint32_t)run; run += (uint64_t)(iv[2 * i + 1] - iv[2 * i]) + 2u;
    }
    ioff[n_iv] = (uint32_t)run;
    const uint64_t d_words = run;
    for (uint32_t i = 0; i < n_q; i++) if (q[2 * i] > d_words || q[2 * i + 1] > d_words - q[2 * i]) return CBC_E_ARG;
    const uint32_t n_tiles = (uint32_t)((d_words + CBC_DEPTH_TILE - 1u) / CBC_DEPTH_TILE);
    const uint32_t cp_cap = (uint32_t)(2u * n_recs + 2u * (uint64_t)n_iv), n_ttiles = (cp_cap + CBC_DEPTH_LINES - 1u) / CBC_DEPTH_LINES;
    std::vector<uint32_t> diff((size_t)n_tiles * CBC_DEPTH_TILE, 0u), cp_pos(cp_cap + 1u, 0xEEEEEEEEu), cp_dep(cp_cap + 1u, 0xEEEEEEEEu);
    std::vector<cbc_block_result> tsum(n_tiles), tcnt(n_tiles);
    std::vector<uint64_t> soff(n_tiles + 1u), coff(n_tiles + 1u);
    uint32_t ctr[4] = { 0, 0, 0, 0 };
    cbc_tdepth_args A;
    memset(&A, 0, sizeof A);
    A.D.R.recs = recs; A.D.R.seq = seq; A.D.R.blocks = blocks; A.D.R.window_start = window_start; A.D.R.dec_results = dec_results;
    A.D.R.n_recs = n_recs; A.D.R.seq_bytes = seq_bytes; A.D.R.beg = 1u; A.D.R.end = UINT64_MAX; A.D.R.n_blocks = n_blocks;
    A.D.diff = diff.data(); A.D.diff_words = diff.size(); A.D.tile_sum = tsum.data(); A.D.tile_cnt = tcnt.data();
    A.D.sum_off = soff.data(); A.D.cnt_off = coff.data(); A.D.cp_pos = cp_pos.data(); A.D.cp_dep = cp_dep.data(); A.D.cp_cap = cp_cap;
    A.D.ctr = ctr; A.D.exclude = exclude; A.D.n_tiles = n_tiles; A.D.n_ttiles = n_ttiles;
    A.iv = ivv.data(); A.iv_off = ioff.data(); A.block_iv = biv.data(); A.n_iv = n_iv;
    for (uint32_t b = 0; b < n_blocks; b++) cbc_targets_mark<WaveEmuDepth>(A, b);
    for (uint32_t t = 0; t < n_tiles; t++) cbc_depth_tile<WaveEmuDepth>(A.D, t);
    scan(tsum.data(), soff.data(), n_tiles);
    scan(tcnt.data(), coff.data(), n_tiles);
    for (uint32_t t = 0; t < n_tiles; t++) cbc_depth_compact<WaveEmuDepth>(A.D, t);
    if (cp_pos[cp_cap] != 0xEEEEEEEEu || cp_dep[cp_cap] != 0xEEEEEEEEu) emu_oob("change point written past the table");
    if (coff[n_tiles] > cp_cap) { emu_oob("more change points than 2K + 2n"); return -100; }
    const uint32_t ncp = (uint32_t)coff[n_tiles];
    cov_passes(cp_pos.data(), cp_dep.data(), ncp, cp_cap, (uint32_t)d_words, min_depth, q, n_q, sum, covered);
    out[0] = ctr[0]; out[1] = ncp; out[2] = d_words;
    if (g_emu_errors) return -100;
    for (uint32_t b = 0; b < n_blocks; b++) if (dec_results[b].status != CBC_ST_OK) return CBC_E_BLOCK;
    return 0;
}
