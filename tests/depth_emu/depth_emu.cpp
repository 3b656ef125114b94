/*
 * depth_emu.cpp -- the coverage bodies (cbc_amd/csrc/cbc_depth_body.h) on the CPU through the lock-step wave emulation.
 * TEST AID ONLY: mark, tile sums, change points, line count and text are checked against the Python model
 * (tests/depthmodel.py) under ASan-able host code before anything runs on a GPU.  The records come from the emulated span
 * decoder or from arrays the test builds.  The scans between the passes are the host loop of tests/emu/post_emu.h (on the
 * device: cbc_scan_sizes_kernel).
 */
#include "../emu/post_emu.h"

/* the span-reporting decoder over every block of the batch */
extern "C" __attribute__((visibility("default")))
int emu_depth_decode(const cbc_dec_device_batch *b, uint32_t smax) { return emu_decode_blocks<WP, true>(b, smax); }

/* every pass in the order of cbc_gpu_decode_depth.  out[0] = text bytes, out[1] = lines, out[2] = reads kept, out[3] = change
 * points.  Returns -1 (CBC_E_ARG) with out[] set and nothing written when the text does not fit text_cap.  Every array is
 * allocated to its exact size so that an index past it is an ASan finding. */
extern "C" __attribute__((visibility("default")))
int emu_depth(const cbc_read_rec *recs, uint64_t n_recs, const uint8_t *seq, uint64_t seq_bytes, const cbc_dec_block_desc *blocks,
              const uint64_t *window_start, const cbc_block_result *dec_results, uint32_t n_blocks, const uint8_t *name,
              uint32_t name_len, uint64_t beg, uint64_t end, uint32_t exclude, uint8_t *text, uint64_t text_cap, uint64_t *out)
{
    g_emu_errors = 0;
    out[0] = out[1] = out[2] = out[3] = 0;
    if (beg < 1 || beg > end || end > CBC_SAM_MAX_POS || n_recs > 0x3fffffffull) return CBC_E_ARG;
    const uint64_t d_words = end - beg + 2u;
    const uint32_t n_tiles = (uint32_t)((d_words + CBC_DEPTH_TILE - 1u) / CBC_DEPTH_TILE);
    const uint32_t cp_cap = (uint32_t)(2u * n_recs), n_ttiles = (cp_cap + CBC_DEPTH_LINES - 1u) / CBC_DEPTH_LINES;
    std::vector<uint32_t> diff((size_t)n_tiles * CBC_DEPTH_TILE, 0u), cp_pos(cp_cap + 1u, 0xEEEEEEEEu), cp_dep(cp_cap + 1u, 0xEEEEEEEEu);
    std::vector<cbc_block_result> tsum(n_tiles), tcnt(n_tiles), counts(n_ttiles + 1u);
    std::vector<uint64_t> soff(n_tiles + 1u), coff(n_tiles + 1u), toff(n_ttiles + 1u);
    std::vector<uint8_t> nm(name, name + name_len);
    uint32_t ctr[4] = { 0, 0, 0, 0 };
    cbc_depth_args A;
    memset(&A, 0, sizeof A);
    A.R.recs = recs; A.R.seq = seq; A.R.blocks = blocks; A.R.window_start = window_start; A.R.dec_results = dec_results;
    A.R.counts = counts.data(); A.R.offsets = toff.data(); A.R.text = text; A.R.text_cap = text_cap; A.R.n_recs = n_recs;
    A.R.seq_bytes = seq_bytes; A.R.beg = beg; A.R.end = end; A.R.n_blocks = n_blocks;
    A.diff = diff.data(); A.diff_words = diff.size(); A.tile_sum = tsum.data(); A.tile_cnt = tcnt.data();
    A.sum_off = soff.data(); A.cnt_off = coff.data(); A.cp_pos = cp_pos.data(); A.cp_dep = cp_dep.data(); A.cp_cap = cp_cap;
    A.ctr = ctr; A.name = nm.data(); A.name_len = name_len; A.exclude = exclude; A.n_tiles = n_tiles; A.n_ttiles = n_ttiles;
    for (uint32_t b = 0; b < n_blocks; b++) cbc_depth_mark<WP>(A, b);
    uint32_t ncp = 0;
    emu_depth_points<WP>(A, soff.data(), coff.data(), "change point", &ncp);
    for (uint32_t t = 0; t < n_ttiles; t++) cbc_depth_count<WP>(A, t);
    scan(counts.data(), toff.data(), n_ttiles);
    out[0] = toff[n_ttiles]; out[1] = ctr[1]; out[2] = ctr[0]; out[3] = coff[n_tiles];
    if (out[0] > text_cap) return CBC_E_ARG;
    for (uint32_t t = 0; t < n_ttiles; t++) cbc_depth_write<WP>(A, t);
    return g_emu_errors ? -100 : 0;
}
