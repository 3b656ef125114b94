/*
 * hist_emu.cpp -- the depth-histogram bodies (cbc_amd/csrc/cbc_hist_body.h) on the CPU through the lock-step wave emulation.
 * TEST AID ONLY: the accumulate, count and write passes are run behind the emulated span decoder and the mark / tile / compact
 * passes of one contig's compressed coordinate (the order of cbc_gpu_decode_depth_hist), or straight on change points the test
 * fabricates (depths on both sides of CBC_HIST_LDS, bins past 2^31, a folded depth near 4 * 10^9), under ASan-able host code
 * before anything runs on a GPU.  The front of the call and the scans between the passes are those of tests/emu/post_emu.h.
 * Every table the new passes touch is an allocation of exactly the size the device call gives it, so an index past it is an
 * ASan finding.  With -DHIST_EMU_MAIN the file is a stand-alone program that builds the fabricated cases itself, compares them
 * with 64-bit host arithmetic and exits non-zero on a mismatch (make asan_check).
 */
#include "../emu/post_emu.h"
#include "../../cbc_amd/csrc/cbc_hist_body.h"

/* the span-reporting decoder over every block of the batch */
extern "C" __attribute__((visibility("default")))
int emu_hist_decode(const cbc_dec_device_batch *b, uint32_t smax) { return emu_decode_blocks<WP, true>(b, smax); }

/* zero, accumulate, count, scan, write over the first ncp change points, with the sizes of the device call: cp_cap sizes the
 * run tiles, `reads` and max_depth the bin table; grid = 0: min(run tiles, CBC_HIST_GRID) as on the device.  CBC_E_ARG with
 * *n_bins set and nothing copied when bin_cap is too small. */
static int hist_passes(const uint32_t *cp_pos, const uint32_t *cp_dep, uint32_t ncp, uint32_t cp_cap, uint64_t reads, uint32_t max_depth,
                       uint32_t grid, uint32_t *bin_depth, uint32_t *bin_bases, uint32_t bin_cap, uint32_t *n_bins)
{
    const uint32_t fold = max_depth ? max_depth : 0xffffffffu;
    const uint64_t h_bins = (reads < fold ? reads : fold) + 1u;
    const uint32_t n_ttiles = (cp_cap + CBC_DEPTH_LINES - 1u) / CBC_DEPTH_LINES;
    const uint32_t n_btiles = (uint32_t)((h_bins + CBC_DEPTH_TILE - 1u) / CBC_DEPTH_TILE);
    const uint32_t out_cap = (uint32_t)(h_bins - 1u < cp_cap ? h_bins - 1u : cp_cap);
    std::vector<uint32_t> pos(cp_pos, cp_pos + ncp), dep(cp_dep, cp_dep + ncp);
    std::vector<uint32_t> bins((size_t)n_btiles * CBC_DEPTH_TILE, 0u), od(out_cap, 0xEEEEEEEEu), ob(out_cap, 0xEEEEEEEEu);
    std::vector<cbc_block_result> tnz(n_btiles);
    std::vector<uint64_t> off(n_btiles + 1u);
    const uint64_t cnt_off[1] = { ncp };                            /* n_tiles = 0: cnt_off[n_tiles] is the count */
    cbc_hist_args A;
    memset(&A, 0, sizeof A);
    A.cp_pos = pos.data(); A.cp_dep = dep.data(); A.cnt_off = cnt_off; A.n_tiles = 0u;
    A.bins = bins.data(); A.tile_nz = tnz.data(); A.nz_off = off.data(); A.out_depth = od.data(); A.out_bases = ob.data();
    A.cp_cap = cp_cap; A.n_ttiles = n_ttiles; A.fold = fold; A.n_bins = (uint32_t)h_bins; A.n_btiles = n_btiles; A.out_cap = out_cap;
    A.grid = grid ? grid : (n_ttiles < CBC_HIST_GRID ? n_ttiles : CBC_HIST_GRID);
    for (uint32_t wg = 0; wg < A.grid; wg++) {
        std::vector<uint32_t> lds(CBC_HIST_LDS, 0xdeadbeefu);       /* one table per workgroup, exactly CBC_HIST_LDS words */
        WP::wg_table(lds.data(), CBC_HIST_LDS);
        cbc_hist_accum<WP>(A, wg, lds.data());
        WP::wg_table(nullptr, 0u);
    }
    for (uint64_t i = h_bins; i < bins.size(); i++) if (bins[i]) { emu_oob("a bin past the table's used part was written"); break; }
    for (uint32_t t = 0; t < n_btiles; t++) cbc_hist_count<WP>(A, t);
    scan(tnz.data(), off.data(), n_btiles);
    for (uint32_t t = 0; t < n_btiles; t++) cbc_hist_write<WP>(A, t);
    const uint64_t n = off[n_btiles];
    if (n > out_cap) { emu_oob("more non-zero bins than the pairs table holds"); return -100; }
    for (uint64_t i = 0; i < n; i++) if (ob[i] == 0u || (od[i] == 0xEEEEEEEEu && ob[i] == 0xEEEEEEEEu)) { emu_oob("a pair was not written"); break; }
    for (uint64_t i = n; i < out_cap; i++) if (od[i] != 0xEEEEEEEEu || ob[i] != 0xEEEEEEEEu) { emu_oob("a pair written past the count"); break; }
    *n_bins = (uint32_t)n;
    if (n > bin_cap) return CBC_E_ARG;
    for (uint64_t i = 0; i < n; i++) { bin_depth[i] = od[i]; bin_bases[i] = ob[i]; }
    return 0;
}

/* fabricated change points straight into the passes (cp_cap = ncp: the run tiles are exactly as many as the points need) */
extern "C" __attribute__((visibility("default")))
int emu_hist_points(const uint32_t *cp_pos, const uint32_t *cp_dep, uint32_t ncp, uint64_t reads, uint32_t max_depth, uint32_t grid,
                    uint32_t *bin_depth, uint32_t *bin_bases, uint32_t bin_cap, uint32_t *n_bins)
{
    g_emu_errors = 0;
    *n_bins = 0;
    if (reads < 1u || reads > 0x3fffffffull) return CBC_E_ARG;
    const int rc = hist_passes(cp_pos, cp_dep, ncp, ncp, reads, max_depth, grid, bin_depth, bin_bases, bin_cap, n_bins);
    return g_emu_errors ? -100 : rc;
}

/* ONE contig's call (iv: its n_iv merged intervals; block_iv relative to them), every pass in the order of
 * cbc_gpu_decode_depth_hist.  out[0] = reads counted, out[1] = change points, out[2] = slots.  CBC_E_BLOCK with *n_bins = 0 when
 * a block of the call failed to decode. */
extern "C" __attribute__((visibility("default")))
int emu_hist(const cbc_read_rec *recs, uint64_t n_recs, const uint8_t *seq, uint64_t seq_bytes, const cbc_dec_block_desc *blocks,
             const uint64_t *window_start, const cbc_block_result *dec_results, uint32_t n_blocks, const uint32_t *iv, uint32_t n_iv,
             const uint32_t *block_iv, uint32_t exclude, uint32_t max_depth, uint32_t *bin_depth, uint32_t *bin_bases, uint32_t bin_cap,
             uint32_t *n_bins, uint64_t *out)
{
    g_emu_errors = 0;
    out[0] = out[1] = out[2] = 0;
    *n_bins = 0;
    uint64_t k_reads = 0;
    for (uint32_t b = 0; b < n_blocks; b++) k_reads += blocks[b].n_reads;
    if (n_recs > 0x3fffffffull || n_iv == 0 || k_reads == 0) return CBC_E_ARG;
    emu_depth_front F;
    if (F.intervals(iv, n_iv, block_iv, n_blocks)) return CBC_E_ARG;
    const uint64_t d_words = F.d_words;
    const uint32_t cp_cap = (uint32_t)(2u * k_reads + 2u * (uint64_t)n_iv);
    F.tables(recs, n_recs, seq, seq_bytes, blocks, window_start, dec_results, n_blocks, exclude, cp_cap);
    F.mark();
    if (F.points()) return -100;
    const uint32_t ncp = F.ncp;
    uint32_t n = 0;
    std::vector<uint32_t> bd(bin_cap ? bin_cap : 1u), bb(bin_cap ? bin_cap : 1u);
    const int rc = hist_passes(F.cp_pos.data(), F.cp_dep.data(), ncp, cp_cap, k_reads, max_depth, 0u, bd.data(), bb.data(), bin_cap, &n);
    out[0] = F.ctr[0]; out[1] = ncp; out[2] = d_words;
    if (g_emu_errors) return -100;
    for (uint32_t b = 0; b < n_blocks; b++) if (dec_results[b].status != CBC_ST_OK) return CBC_E_BLOCK;   /* no bins */
    *n_bins = n;
    if (rc) return rc;
    for (uint32_t i = 0; i < n; i++) { bin_depth[i] = bd[i]; bin_bases[i] = bb[i]; }
    return 0;
}

#ifdef HIST_EMU_MAIN
#include <map>
/* ---- the stand-alone check: fabricated change points against 64-bit host arithmetic -------------------------------------------- */
struct fab { std::vector<uint32_t> pos, dep; };

static void fab_run(fab &f, uint64_t &at, uint32_t depth, uint32_t len) { f.pos.push_back((uint32_t)at); f.dep.push_back(depth); at += len; }
static void fab_end(fab &f, uint64_t at) { f.pos.push_back((uint32_t)at); f.dep.push_back(0u); }

static int fab_check(const char *what, const fab &f, uint64_t reads, uint32_t max_depth, uint32_t grid, int short_cap)
{
    const uint32_t fold = max_depth ? max_depth : 0xffffffffu;
    std::map<uint32_t, uint64_t> want;
    for (size_t j = 0; j + 1 < f.pos.size(); j++)
        if (f.dep[j]) want[f.dep[j] < fold ? f.dep[j] : fold] += f.pos[j + 1] - f.pos[j];
    const uint32_t cap = (uint32_t)want.size() - (short_cap && !want.empty() ? 1u : 0u);
    std::vector<uint32_t> bd(cap), bb(cap);                          /* exactly bin_cap entries */
    uint32_t n = 0;
    const int rc = emu_hist_points(f.pos.data(), f.dep.data(), (uint32_t)f.pos.size(), reads, max_depth, grid, bd.data(), bb.data(), cap, &n);
    int bad = 0;
    if (n != want.size()) bad = 1;
    if (short_cap && !want.empty()) { if (rc != CBC_E_ARG) bad = 1; }
    else {
        if (rc != 0) bad = 1;
        size_t i = 0;
        for (std::map<uint32_t, uint64_t>::const_iterator it = want.begin(); it != want.end() && !bad; ++it, ++i)
            if (bd[i] != it->first || (uint64_t)bb[i] != it->second) bad = 1;
    }
    printf("%-44s %s (rc %d, %u bins)\n", what, bad ? "MISMATCH" : "ok", rc, n);
    return bad;
}

int main()
{
    int bad = 0;
    uint64_t at;
    {   /* both sides of CBC_HIST_LDS, the same bins from the LDS and from the global path (a fold at 1024), zero runs between */
        fab f; at = 5;
        const uint32_t d[] = { 1023, 1024, 1025, 0, 1, 1023, 0, 0, 1024, 2000, 1025, 7, 1023 };
        for (size_t i = 0; i < sizeof d / sizeof d[0]; i++) fab_run(f, at, d[i], 10u + (uint32_t)i);
        fab_end(f, at);
        bad |= fab_check("around CBC_HIST_LDS", f, 2000, 0, 0, 0);
        bad |= fab_check("around CBC_HIST_LDS, fold 1024", f, 2000, 1024, 0, 0);
        bad |= fab_check("around CBC_HIST_LDS, fold 1023", f, 2000, 1023, 0, 0);
        bad |= fab_check("around CBC_HIST_LDS, fold 1", f, 2000, 1, 0, 0);
        bad |= fab_check("around CBC_HIST_LDS, fold above", f, 2000, 1999, 0, 0);
        bad |= fab_check("bin_cap one too small", f, 2000, 0, 0, 1);
    }
    {   /* three runs of 10^9 slots at one depth: the bin passes 2^31; once in LDS, once in the global table */
        for (uint32_t depth = 3; depth <= 3000; depth *= 1000) {
            fab f; at = 0;
            for (int i = 0; i < 3; i++) { fab_run(f, at, depth, 1000000000u); fab_run(f, at, 0, 7); }
            fab_end(f, at);
            bad |= fab_check(depth == 3 ? "3 * 10^9 slots in an LDS bin" : "3 * 10^9 slots in a global bin", f, 5000, 0, 0, 0);
        }
    }
    {   /* a depth near 4 * 10^9 folded by M */
        fab f; at = 100;
        fab_run(f, at, 4000000000u, 12345); fab_run(f, at, 3999999999u, 1); fab_run(f, at, 5000, 9); fab_run(f, at, 4999, 4);
        fab_end(f, at);
        bad |= fab_check("depth 4 * 10^9 folded at 5000", f, 0x3fffffffull, 5000, 0, 0);
        bad |= fab_check("depth 4 * 10^9 folded at 900", f, 0x3fffffffull, 900, 0, 0);
    }
    for (uint32_t ncp = 0; ncp <= 2; ncp++) {   /* no run at all, a lone change point, one run */
        fab f; at = 9;
        if (ncp == 2) fab_run(f, at, 6, 40);
        if (ncp >= 1) fab_end(f, at);
        bad |= fab_check(ncp == 0 ? "ncp 0" : ncp == 1 ? "ncp 1" : "ncp 2", f, 10, 0, 0, 0);
    }
    {   /* more runs than grid * tile: the stride loop turns, and the last tile is partial */
        fab f; at = 1;
        for (uint32_t i = 0; i < 5u * CBC_DEPTH_LINES + 77u; i++) fab_run(f, at, i % 5u == 0u ? 0u : 1u + (i * 7u) % 1500u, 1u + i % 9u);
        fab_end(f, at);
        bad |= fab_check("5 tiles of runs on a grid of 2", f, 1500, 0, 2, 0);
        bad |= fab_check("5 tiles of runs on a grid of 1", f, 1500, 1100, 1, 0);
        bad |= fab_check("5 tiles of runs, the device's grid", f, 1500, 0, 0, 0);
    }
    if (g_emu_errors) bad = 1;
    printf(bad ? "HIST EMU CHECK FAILED\n" : "HIST EMU CHECK OK\n");
    return bad;
}
#endif
