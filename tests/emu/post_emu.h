/*
 * post_emu.h -- what the emulation drivers of the post-decode bodies (tests/<name>_emu/<name>_emu.cpp) share: the error counter,
 * the host scan between two passes, the decoder over every block of a batch, the depth front of a target set, the passes of the
 * coverage summary and the pileup call.  TEST AID ONLY, like wave_emu.h: the bodies are run here on the CPU, every table an
 * allocation of its exact size, under ASan-able host code before anything runs on a GPU.  Each driver is one translation unit and
 * one library (or one check program), and each keeps its own copy of everything in this file.
 */
#ifndef CBC_POST_EMU_H
#define CBC_POST_EMU_H

#include <string>
#include <vector>
#include "wave_emu_post.h"
#include "../../cbc_amd/csrc/cbc_encode_body.h"
#include "../../cbc_amd/csrc/cbc_decode_body.h"
#include "../../cbc_amd/csrc/cbc_plan.h"
#include "../../cbc_amd/csrc/cbc_targets_body.h"
#include "../../cbc_amd/csrc/cbc_cov_body.h"
#include "../../cbc_amd/csrc/cbc_pileup_body.h"

typedef WaveEmuPost WP;

/* internal linkage, and emu_oob hidden by -fvisibility=hidden: the libraries are loaded together into one process */
static int g_emu_errors = 0;
extern "C" void emu_oob(const char *what) { fprintf(stderr, "[emu] invariant violated: %s\n", what); g_emu_errors++; }

/* the exclusive scan between two passes (on the device: cbc_scan_sizes_kernel) */
static void scan(const cbc_block_result *r, uint64_t *off, uint32_t n)
{
    uint64_t run = 0;
    for (uint32_t i = 0; i < n; i++) { off[i] = run; run += r[i].status == CBC_ST_OK ? r[i].nbytes : 0u; }
    off[n] = run;
}

/* the decoder over every block of the batch, each block with LDS of its exact size: the plain one, the span-reporting one
 * (SPAN), or the edit-reporting one (EDITS: side = 2 * n_recs words, arena = n_recs * per_read entries exactly, named to W) */
template <class W, bool SPAN, bool EDITS = false>
static int emu_decode_blocks(const cbc_dec_device_batch *b, uint32_t smax, uint32_t per_read = 0u, uint32_t *side = nullptr,
                             uint16_t *arena = nullptr)
{
    cbc_dec_args A;
    memset(&A, 0, sizeof A);
    A.in = b->d_in; A.blocks = b->d_blocks; A.ref = b->d_ref; A.recs = b->d_recs; A.seq = b->d_seq; A.results = b->d_results;
    A.in_bytes = b->in_bytes; A.ref_bytes = b->ref_bytes; A.n_recs = b->n_recs; A.seq_bytes = b->seq_bytes;
    A.n_blocks = b->n_blocks; A.cap_pos = b->caps.cap_pos; A.cap_var = b->caps.cap_var;
    A.var_scratch = b->d_var_scratch; A.var_scratch_words = b->var_scratch_words;
    cbc_dec_edits E;
    memset(&E, 0, sizeof E);
    E.side = side; E.arena = arena; E.arena_entries = b->n_recs * per_read; E.per_read = per_read;
    g_emu_errors = 0;
    if constexpr (EDITS) W::edit_arena(arena, E.arena_entries);
    uint32_t words = cbc_plan_dec_lds_bytes(&b->caps) / 4;
    for (uint32_t blk = 0; blk < b->n_blocks; blk++) {
        std::vector<uint32_t> lds(words, 0xdeadbeefu);
        cbc_decode_stream<W, SPAN, EDITS>(A, blk, lds.data(), smax, EDITS ? &E : nullptr);
    }
    if constexpr (EDITS) W::edit_arena(nullptr, 0);
    return g_emu_errors ? -100 : 0;
}

/* tile sums, their scans and the compact pass over D's difference array, then the checks on the table of D.cp_cap points, which
 * the caller allocated one entry longer and filled with 0xEEEEEEEE: nothing written past it, no more points than it holds.
 * soff / coff: the arrays behind D.sum_off / D.cnt_off.  what: "change point" (or covx's "start point").  Returns -100 when the
 * points pass the bound, else 0 with *n = their count. */
template <class W>
static int emu_depth_points(const cbc_depth_args &D, uint64_t *soff, uint64_t *coff, const char *what, uint32_t *n)
{
    for (uint32_t t = 0; t < D.n_tiles; t++) cbc_depth_tile<W>(D, t);
    scan(D.tile_sum, soff, D.n_tiles);
    scan(D.tile_cnt, coff, D.n_tiles);
    for (uint32_t t = 0; t < D.n_tiles; t++) cbc_depth_compact<W>(D, t);
    if (D.cp_pos[D.cp_cap] != 0xEEEEEEEEu || D.cp_dep[D.cp_cap] != 0xEEEEEEEEu) emu_oob((std::string(what) + " written past the table").c_str());
    *n = (uint32_t)coff[D.n_tiles];
    if (coff[D.n_tiles] > D.cp_cap) { emu_oob(("more " + std::string(what) + "s than the bound").c_str()); return -100; }
    return 0;
}

/* The depth front of ONE contig's target set, in the compressed coordinate: interval offsets, mark, tile sums, scans, compact.
 * Every table is copied into or allocated at its exact size.  The order of a call: intervals(), the caller's own argument
 * checks against d_words, tables(), mark(), points(); what follows reads cp_pos / cp_dep[0 .. ncp), ctr and d_words. */
struct emu_depth_front {
    std::vector<uint32_t> ivv, biv, ioff, diff, cp_pos, cp_dep;
    std::vector<cbc_block_result> tsum, tcnt;
    std::vector<uint64_t> soff, coff;
    uint32_t ctr[4], n_tiles, ncp;
    uint64_t d_words;
    cbc_tdepth_args A;

    /* iv: n_iv > 0 pairs, ascending and apart; block_iv relative to them.  CBC_E_ARG when they are not; else 0 and d_words */
    int intervals(const uint32_t *iv, uint32_t n_iv, const uint32_t *block_iv, uint32_t n_blocks)
    {
        ivv.assign(iv, iv + 2u * (size_t)n_iv); biv.assign(block_iv, block_iv + 2u * (size_t)n_blocks); ioff.assign(n_iv + 1u, 0u);
        uint64_t run = 0;
        for (uint32_t i = 0; i < n_iv; i++) {
            if (iv[2 * i] < 1 || iv[2 * i] > iv[2 * i + 1] || iv[2 * i + 1] > CBC_SAM_MAX_POS || (i && iv[2 * i] <= iv[2 * i - 1] + 1u)) return CBC_E_ARG;
            ioff[i] = (uint32_t)run; run += (uint64_t)(iv[2 * i + 1] - iv[2 * i]) + 2u;
        }
        ioff[n_iv] = (uint32_t)run;
        d_words = run;
        return 0;
    }
    /* the tables of d_words slots and at most cp_cap change points (plus the guard entry), and the arguments of the passes;
     * without intervals() before it (skipdel's window form) the caller has set d_words and sets A.D.R.beg / end */
    void tables(const cbc_read_rec *recs, uint64_t n_recs, const uint8_t *seq, uint64_t seq_bytes, const cbc_dec_block_desc *blocks,
                const uint64_t *window_start, const cbc_block_result *dec_results, uint32_t n_blocks, uint32_t exclude, uint32_t cp_cap)
    {
        n_tiles = (uint32_t)((d_words + CBC_DEPTH_TILE - 1u) / CBC_DEPTH_TILE);
        diff.assign((size_t)n_tiles * CBC_DEPTH_TILE, 0u); cp_pos.assign(cp_cap + 1u, 0xEEEEEEEEu); cp_dep.assign(cp_cap + 1u, 0xEEEEEEEEu);
        tsum.resize(n_tiles); tcnt.resize(n_tiles); soff.resize(n_tiles + 1u); coff.resize(n_tiles + 1u);
        ctr[0] = ctr[1] = ctr[2] = ctr[3] = 0; ncp = 0;
        memset(&A, 0, sizeof A);
        A.D.R.recs = recs; A.D.R.seq = seq; A.D.R.blocks = blocks; A.D.R.window_start = window_start; A.D.R.dec_results = dec_results;
        A.D.R.n_recs = n_recs; A.D.R.seq_bytes = seq_bytes; A.D.R.beg = 1u; A.D.R.end = UINT64_MAX; A.D.R.n_blocks = n_blocks;
        A.D.diff = diff.data(); A.D.diff_words = diff.size(); A.D.tile_sum = tsum.data(); A.D.tile_cnt = tcnt.data();
        A.D.sum_off = soff.data(); A.D.cnt_off = coff.data(); A.D.cp_pos = cp_pos.data(); A.D.cp_dep = cp_dep.data(); A.D.cp_cap = cp_cap;
        A.D.ctr = ctr; A.D.exclude = exclude; A.D.n_tiles = n_tiles; A.D.n_ttiles = (cp_cap + CBC_DEPTH_LINES - 1u) / CBC_DEPTH_LINES;
        A.iv = ivv.data(); A.iv_off = ioff.data(); A.block_iv = biv.data(); A.n_iv = (uint32_t)(ivv.size() / 2u);
    }
    /* starts != NULL: the pass also notes the pieces' first slots there (cbc_targets_mark<W, true>) */
    void mark(uint32_t *starts = nullptr)
    {
        for (uint32_t b = 0; b < A.D.R.n_blocks; b++) {
            if (starts) cbc_targets_mark<WP, true>(A, b, starts);
            else cbc_targets_mark<WP>(A, b);
        }
    }
    int points() { return emu_depth_points<WP>(A.D, soff.data(), coff.data(), "change point", &ncp); }
};

/* the passes of cbc_gpu_decode_coverage behind the change points -- weights, scans, apply, lookup over the first ncp of them;
 * cp_cap sizes the tiles as the device call does */
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
    for (uint32_t t = 0; t < n_ttiles; t++) cbc_cov_weights<WP>(A, t);
    scan(tl.data(), ol.data(), n_ttiles); scan(th.data(), oh.data(), n_ttiles); scan(tc.data(), oc.data(), n_ttiles);
    for (uint32_t t = 0; t < n_ttiles; t++) cbc_cov_apply<WP>(A, t);
    for (uint32_t i = 0; i < ncp; i++) if (pre_lo[i] == 0xEEEEEEEEu && pre_hi[i] == 0xEEEEEEEEu && pre_cov[i] == 0xEEEEEEEEu) { emu_oob("a prefix was not written"); break; }
    for (uint32_t w = 0; w < (n_q + 63u) / 64u; w++) cbc_cov_lookup<WP>(A, w);
    for (uint32_t i = 0; i < n_q; i++) { sum[i] = (uint64_t)s[2u * i] | ((uint64_t)s[2u * i + 1u] << 32); covered[i] = c[i]; }
}

template <int M>
static void pileup_count_and_write(const cbc_pileup_args &A, const cbc_pileup_sx &X, uint32_t n_tiles, std::vector<uint64_t> &offsets,
                                   const std::vector<cbc_block_result> &counts, const std::vector<uint32_t> &ctr, uint64_t text_cap, uint64_t *out, int &rc)
{
    for (uint32_t t = 0; t < n_tiles; t++) cbc_pileup_count<WP, M>(A, t, &X);
    for (uint32_t t = 0; t < n_tiles; t++) offsets[t + 1u] = offsets[t] + counts[t].nbytes;
    out[0] = offsets[n_tiles]; out[1] = ctr[1]; out[2] = ctr[0];
    if (out[0] > text_cap) rc = CBC_E_ARG;
    else for (uint32_t t = 0; t < n_tiles; t++) cbc_pileup_write<WP, M>(A, t, &X);
}

/* ONE cbc_gpu_decode_pileup_ext behind the decode (cbc_gpu_decode_pileup is ppm = 0, by_strand = 0: the plain bodies), the
 * passes in the call's order -- zero, cbc_depth_mark, (cbc_depth_mark of the forward reads,) events, cbc_depth_tile and the scan
 * (twice with by_strand), count, the scan, write.  Every table is an allocation of exactly its size and named to the emulation.
 * out[0] = text bytes (also when text_cap is too small: CBC_E_ARG, nothing written), out[1] = lines, out[2] = reads kept.
 * CBC_E_BLOCK (after the text of the other blocks) when a block of the call failed.  n_waves wavefronts share a block in the
 * events pass.  seed_depth, seed_cnt (the stand-alone check's ten-digit numbers; 0 otherwise): added before the passes to word 0
 * of the difference arrays and of every plane, as if that many reads had started and been observed at the window's first
 * position. */
static int emu_pileup_call(const cbc_read_rec *recs, uint64_t n_recs, const uint8_t *seq, uint64_t seq_bytes, const cbc_dec_block_desc *blocks,
                           const uint64_t *window_start, const cbc_block_result *dec_results, uint32_t n_blocks, const uint32_t *side,
                           const uint16_t *arena, uint32_t per_read, const uint8_t *ref, uint64_t ref_bytes, uint64_t ref_c0, const char *name,
                           uint32_t name_len, uint64_t beg, uint64_t end, uint32_t exclude, uint32_t min_alt, uint32_t ppm, uint32_t by_strand,
                           uint32_t n_waves, uint32_t seed_depth, uint32_t seed_cnt, uint8_t *text, uint64_t text_cap, uint64_t *out)
{
    g_emu_errors = 0;
    out[0] = out[1] = out[2] = 0;
    if (beg < 1 || beg > end || end > CBC_SAM_MAX_POS || n_waves < 1u || n_waves > 16u || min_alt < 1u || ppm > 1000000u || by_strand > 1u)
        return CBC_E_ARG;
    const bool bs = by_strand != 0u;
    const uint32_t planes = bs ? 2u * CBC_PILEUP_PLANES : CBC_PILEUP_PLANES;
    const uint64_t d_words = end - beg + 2u;
    const uint32_t n_tiles = (uint32_t)((d_words + CBC_DEPTH_TILE - 1u) / CBC_DEPTH_TILE);
    const size_t plane = (size_t)n_tiles * CBC_DEPTH_TILE;
    std::vector<uint32_t> diff(plane, 0u), diff_f(bs ? plane : 0u, 0u), tab(plane * planes, 0u), ctr(4, 0u);
    std::vector<cbc_block_result> tile_sum(n_tiles), tile_cnt(n_tiles), tile_sum_f(n_tiles), tile_cnt_f(n_tiles), counts(n_tiles);
    std::vector<uint64_t> sum_off(n_tiles + 1u, 0u), sum_off_f(n_tiles + 1u, 0u), offsets(n_tiles + 1u, 0u);
    std::vector<uint8_t> dname(name, name + name_len);
    cbc_pileup_args A;
    memset(&A, 0, sizeof A);
    cbc_region_args &R = A.D.R;
    R.recs = recs; R.seq = seq; R.blocks = blocks; R.window_start = window_start; R.dec_results = dec_results;
    R.counts = counts.data(); R.offsets = offsets.data(); R.text = text; R.text_cap = text_cap;
    R.n_recs = n_recs; R.seq_bytes = seq_bytes; R.beg = beg; R.end = end; R.n_blocks = n_blocks;
    A.D.diff = diff.data(); A.D.diff_words = diff.size(); A.D.tile_sum = tile_sum.data(); A.D.tile_cnt = tile_cnt.data();
    A.D.sum_off = sum_off.data(); A.D.cnt_off = sum_off.data(); A.D.ctr = ctr.data(); A.D.name = dname.data();
    A.D.name_len = name_len; A.D.exclude = exclude; A.D.n_tiles = n_tiles; A.D.n_ttiles = n_tiles;
    A.side = side; A.arena = arena; A.arena_entries = n_recs * per_read; A.per_read = per_read;
    A.ref = ref; A.ref_bytes = ref_bytes; A.ref_c0 = ref_c0; A.tab = tab.data(); A.plane = plane; A.min_alt = min_alt;
    cbc_depth_args F = A.D;                                          /* the forward reads' mark and tile passes */
    cbc_pileup_sx X;
    memset(&X, 0, sizeof X);
    X.ppm = ppm;
    if (bs) {
        F.diff = diff_f.data(); F.exclude = exclude | 16u; F.ctr = ctr.data() + 2; F.tile_sum = tile_sum_f.data(); F.tile_cnt = tile_cnt_f.data();
        F.sum_off = sum_off_f.data(); F.cnt_off = sum_off_f.data();
        X.diff_f = diff_f.data(); X.sum_off_f = sum_off_f.data();
    }
    diff[0] += seed_depth;
    if (bs) diff_f[0] += seed_depth;
    for (uint32_t k = 0; k < planes; k++) tab[(size_t)k * plane] += seed_cnt;
    WP::clear_ranges();
    /* the window's own words only: W + 1 of each difference array, W of every plane */
    WP::add_range(diff.data(), d_words);
    if (bs) WP::add_range(diff_f.data(), d_words);
    for (uint32_t k = 0; k < planes; k++) WP::add_range(tab.data() + (size_t)k * plane, d_words - 1u);
    WP::add_range(ctr.data(), bs ? 3 : 2);
    WP::edit_arena(arena, A.arena_entries);
    for (uint32_t b = 0; b < n_blocks; b++) cbc_depth_mark<WP>(A.D, b);
    for (uint32_t b = 0; bs && b < n_blocks; b++) cbc_depth_mark<WP>(F, b);
    for (uint32_t b = 0; b < n_blocks; b++)
        for (uint32_t w = 0; w < n_waves; w++) {
            if (bs) cbc_pileup_events<WP, true>(A, b, w, n_waves);
            else cbc_pileup_events<WP>(A, b, w, n_waves);
        }
    for (uint32_t t = 0; t < n_tiles; t++) cbc_depth_tile<WP>(A.D, t);
    for (uint32_t t = 0; t < n_tiles; t++) sum_off[t + 1u] = sum_off[t] + tile_sum[t].nbytes;
    for (uint32_t t = 0; bs && t < n_tiles; t++) cbc_depth_tile<WP>(F, t);
    for (uint32_t t = 0; bs && t < n_tiles; t++) sum_off_f[t + 1u] = sum_off_f[t] + tile_sum_f[t].nbytes;
    int rc = 0;
    if (bs) pileup_count_and_write<CBC_PILEUP_STRAND>(A, X, n_tiles, offsets, counts, ctr, text_cap, out, rc);
    else if (ppm) pileup_count_and_write<CBC_PILEUP_FRAC>(A, X, n_tiles, offsets, counts, ctr, text_cap, out, rc);
    else pileup_count_and_write<0>(A, X, n_tiles, offsets, counts, ctr, text_cap, out, rc);
    WP::clear_ranges();
    WP::edit_arena(nullptr, 0);
    if (g_emu_errors) return -100;
    if (rc) return rc;
    for (uint32_t b = 0; b < n_blocks; b++) if (dec_results[b].status != CBC_ST_OK) return CBC_E_BLOCK;
    return 0;
}

#endif
