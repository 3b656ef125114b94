/*
 * skipdel_emu.cpp -- the edit-reporting decoder (cbc_amd/csrc/cbc_decode_body.h, EDITS = true) and the unmark bodies of the
 * deletion-aware coverage (cbc_amd/csrc/cbc_skipdel_body.h) on the CPU through the lock-step wave emulation.  TEST AID ONLY: the
 * passes of a depth call under cbc_gpu_set_depth_skip_deletions are run in its order -- zero, mark, unmark, cbc_depth_tile, the two
 * scans, compact, count, the scan, write -- over one window (n_iv == 0) or over one contig's intervals in the compressed
 * coordinate, behind the emulated decoder or on records and arena entries the stand-alone program fabricates, under ASan-able
 * host code before anything runs on a GPU.  Every table is an allocation of exactly its size -- the change points exactly the
 * library's bound -- and the difference array's own words and the two counters are named to the emulation, so a list_add outside
 * them is a finding.  With -DSKIPDEL_EMU_MAIN the file is a stand-alone program that builds the fabricated cases itself,
 * compares them with a base-by-base host loop and exits non-zero on a mismatch (make asan_check).
 */
#include "../emu/post_emu.h"
#include "../../cbc_amd/csrc/cbc_skipdel_body.h"

/* the edit-reporting decoder over every block of the batch: side = 2 * n_recs words, arena = n_recs * per_read entries exactly */
extern "C" __attribute__((visibility("default")))
int emu_skipdel_decode(const cbc_dec_device_batch *b, uint32_t smax, uint32_t per_read, uint32_t *side, uint16_t *arena)
{ return emu_decode_blocks<WP, true, true>(b, smax, per_read, side, arena); }

/* the library's bound on the change points (post_sizes_of in cbc_gpu_post.hip): per_read == 0 is the span depth's */
extern "C" __attribute__((visibility("default")))
uint64_t emu_skipdel_cp_cap(uint64_t d_words, uint64_t n_recs, uint32_t n_iv, uint32_t per_read)
{
    if (per_read == 0u) return 2u * n_recs + 2u * (uint64_t)n_iv;
    const uint64_t by_edits = 2u * n_recs * (1u + (uint64_t)per_read) + 2u * (uint64_t)n_iv;
    return by_edits < d_words ? by_edits : d_words;
}

/* ONE depth call behind the decode.  n_iv == 0: the window [beg, end] (cbc_gpu_decode_depth); n_iv > 0: the contig's intervals
 * iv (n_iv pairs, ascending and apart; block_iv relative to them) in the compressed coordinate (cbc_gpu_decode_targets with the
 * depth output).  per_read > 0: deleted bases do not count; 0: the span depth, no unmark pass.  out[0] = text bytes (also when
 * text_cap is too small: CBC_E_ARG, nothing written), out[1] = lines, out[2] = reads kept, out[3] = change points, out[4] =
 * words of the difference array, out[5] = the bound on the change points; cp (NULL: not wanted): out[3] pairs position, depth,
 * room for out[5].  CBC_E_BLOCK (after the text of the other blocks) when a block of the call failed. */
extern "C" __attribute__((visibility("default")))
int emu_skipdel(const cbc_read_rec *recs, uint64_t n_recs, const uint8_t *seq, uint64_t seq_bytes, const cbc_dec_block_desc *blocks,
                const uint64_t *window_start, const cbc_block_result *dec_results, uint32_t n_blocks, const uint32_t *side,
                const uint16_t *arena, uint32_t per_read, const char *name, uint32_t name_len, uint64_t beg, uint64_t end,
                const uint32_t *iv, uint32_t n_iv, const uint32_t *block_iv, uint32_t exclude, uint32_t n_waves, uint8_t *text,
                uint64_t text_cap, uint32_t *cp, uint64_t *out)
{
    g_emu_errors = 0;
    for (int i = 0; i < 6; i++) out[i] = 0;
    const bool tg = n_iv != 0u;
    if (n_recs > 0x3fffffffull || n_waves < 1u || n_waves > 16u || per_read > 510u) return CBC_E_ARG;
    if (!tg && (beg < 1 || beg > end || end > CBC_SAM_MAX_POS)) return CBC_E_ARG;
    emu_depth_front F;
    F.d_words = end - beg + 2u;
    if (tg && F.intervals(iv, n_iv, block_iv, n_blocks)) return CBC_E_ARG;
    const uint64_t d_words = F.d_words;
    const uint32_t cp_cap = (uint32_t)emu_skipdel_cp_cap(d_words, n_recs, n_iv, per_read);
    const uint32_t n_ttiles = (cp_cap + CBC_DEPTH_LINES - 1u) / CBC_DEPTH_LINES;
    std::vector<cbc_block_result> counts(n_ttiles + 1u);
    std::vector<uint64_t> toff(n_ttiles + 1u);
    std::vector<uint8_t> nm(name, name + name_len);
    F.tables(recs, n_recs, seq, seq_bytes, blocks, window_start, dec_results, n_blocks, exclude, cp_cap);
    const uint32_t n_tiles = F.n_tiles;
    uint32_t *const ctr = F.ctr;
    cbc_tskipdel_args X;
    memset(&X, 0, sizeof X);
    X.T = F.A;
    cbc_tdepth_args &A = X.T;
    A.D.R.counts = counts.data(); A.D.R.offsets = toff.data(); A.D.R.text = text; A.D.R.text_cap = text_cap;
    if (!tg) { A.D.R.beg = beg; A.D.R.end = end; }
    A.D.name = nm.data(); A.D.name_len = name_len;
    X.E.side = side; X.E.arena = arena; X.E.arena_entries = n_recs * per_read; X.E.per_read = per_read;
    cbc_skipdel_args Wd;
    Wd.D = A.D; Wd.E = X.E;
    WP::clear_ranges();
    WP::add_range(F.diff.data(), d_words);                              /* the array's own words only, not the tile's padding */
    WP::add_range(ctr, 2);
    WP::edit_arena(arena, X.E.arena_entries);
    for (uint32_t b = 0; b < n_blocks; b++) { if (tg) cbc_targets_mark<WP>(A, b); else cbc_depth_mark<WP>(A.D, b); }
    const uint32_t kept = ctr[0];
    for (uint32_t b = 0; b < n_blocks && per_read; b++)
        for (uint32_t w = 0; w < n_waves; w++) { if (tg) cbc_skipdel_targets_unmark<WP>(X, b, w, n_waves); else cbc_skipdel_unmark<WP>(Wd, b, w, n_waves); }
    if (ctr[0] != kept) emu_oob("the unmark pass changed the count of the kept reads");
    uint32_t ncp = 0;
    emu_depth_points<WP>(A.D, F.soff.data(), F.coff.data(), "change point", &ncp);   /* a finding is counted; the text passes still run */
    if ((uint32_t)F.soff[n_tiles] != 0u) emu_oob("the depth behind the last word is not 0");
    for (uint32_t t = 0; t < n_ttiles; t++) { if (tg) cbc_targets_depth_count<WP>(A, t); else cbc_depth_count<WP>(A.D, t); }
    scan(counts.data(), toff.data(), n_ttiles);
    out[0] = toff[n_ttiles]; out[1] = ctr[1]; out[2] = ctr[0]; out[3] = F.coff[n_tiles]; out[4] = d_words; out[5] = cp_cap;
    for (uint64_t i = 0; cp && i < out[3] && i < cp_cap; i++) { cp[2 * i] = F.cp_pos[i]; cp[2 * i + 1] = F.cp_dep[i]; }
    int rc = 0;
    if (out[0] > text_cap) rc = CBC_E_ARG;
    else for (uint32_t t = 0; t < n_ttiles; t++) { if (tg) cbc_targets_depth_write<WP>(A, t); else cbc_depth_write<WP>(A.D, t); }
    WP::clear_ranges();
    WP::edit_arena(nullptr, 0);
    if (g_emu_errors) return -100;
    if (rc) return rc;
    for (uint32_t b = 0; b < n_blocks; b++) if (dec_results[b].status != CBC_ST_OK) return CBC_E_BLOCK;
    return 0;
}

#ifdef SKIPDEL_EMU_MAIN
#include "../emu/fab_reads.h"
/* ---- the stand-alone check: fabricated records and arena entries against a base-by-base host loop ------------------------------ */
/* the definition of include/cbc_gpu.h, one base at a time: depth[p] of positions 1 .. top, and the reads kept by `keep` */
static void want_depth(const fab &f, uint32_t exclude, const std::vector<int> &failed, uint64_t top, std::vector<int64_t> &depth)
{
    depth.assign((size_t)top + 2u, 0);
    size_t at = 0;
    for (size_t b = 0; b < f.block_n.size(); b++)
        for (uint32_t k = 0; k < f.block_n[b]; k++, at++) {
            const fread_ &r = f.reads[at];
            if (failed[b] || r.span < 1u || (r.flag & exclude)) continue;
            for (uint64_t p = r.pos; p < (uint64_t)r.pos + r.span && p <= top; p++) depth[p]++;
            for (size_t d = 0; d < r.dc.size(); d++) {
                const uint64_t off = (uint64_t)r.dc[d] + d, p = r.pos + off;
                if (off < r.span && p <= top) depth[p]--;
            }
        }
}

/* bedGraph of the positions [b, e] (1-based): one line per maximal run of equal non-zero depth; the runs are appended to `out` */
static void want_runs(const std::string &name, const std::vector<int64_t> &depth, uint64_t b, uint64_t e, std::string &out, uint64_t &lines,
                      uint64_t &points)
{
    int64_t cur = 0;
    uint64_t start = 0;
    for (uint64_t p = b; p <= e + 1u; p++) {
        const int64_t d = p <= e ? depth[p] : 0;
        if (d == cur) continue;
        points++;
        if (cur != 0) {
            char buf[400];
            snprintf(buf, sizeof buf, "%s\t%llu\t%llu\t%lld\n", name.c_str(), (unsigned long long)(start - 1u), (unsigned long long)(p - 1u), (long long)cur);
            out += buf; lines++;
        }
        cur = d; start = p;
    }
}

static int fab_check(const char *what, const fab &f, uint64_t beg, uint64_t end, const std::vector<uint32_t> &iv, uint32_t exclude,
                     uint32_t n_waves, int fail_block = -1)
{
    const std::string name = "ctg";
    const uint32_t n_iv = (uint32_t)(iv.size() / 2u);
    fab_arrays a;
    if (!fab_build(f, a, fail_block)) { printf("%-70s BAD FIXTURE\n", what); return 1; }
    const std::vector<int> &failed = a.failed;
    vu biv;
    for (size_t b = 0; b < f.block_n.size(); b++) { biv.push_back(0u); biv.push_back(n_iv); }   /* every block may reach every interval */
    uint64_t top = end;
    for (uint32_t i = 0; i < n_iv; i++) if (iv[2 * i + 1] > top) top = iv[2 * i + 1];
    std::vector<int64_t> depth;
    want_depth(f, exclude, failed, top, depth);
    for (uint64_t p = 0; p < depth.size(); p++) if (depth[p] < 0) { printf("%-70s BAD FIXTURE: negative depth\n", what); return 1; }
    std::string want;
    uint64_t lines = 0, points = 0, kept = 0;
    if (n_iv) for (uint32_t i = 0; i < n_iv; i++) want_runs(name, depth, iv[2 * i], iv[2 * i + 1], want, lines, points);
    else want_runs(name, depth, beg, end, want, lines, points);
    size_t at = 0;
    for (size_t b = 0; b < f.block_n.size(); b++)
        for (uint32_t k = 0; k < f.block_n[b]; k++, at++) {
            const fread_ &r = f.reads[at];
            if (failed[b] || r.span < 1u || (r.flag & exclude)) continue;
            const uint64_t last = (uint64_t)r.pos + r.span - 1u;
            bool hit = !n_iv && r.pos <= end && last >= beg;
            for (uint32_t i = 0; i < n_iv; i++) hit |= r.pos <= iv[2 * i + 1] && last >= iv[2 * i];
            kept += hit;
        }
    std::vector<uint8_t> text(want.size() + 16u, 0xEEu);
    uint64_t out[6] = { 0, 0, 0, 0, 0, 0 };
    auto call = [&](uint8_t *t, uint64_t cap) {
        return emu_skipdel(a.recs.data(), f.reads.size(), a.rows.data(), a.rows.size(), a.blocks.data(), a.ws.data(), a.res.data(), (uint32_t)a.blocks.size(),
                           a.side.data(), a.arena.data(), f.per_read, name.c_str(), (uint32_t)name.size(), beg, end, iv.data(), n_iv, biv.data(), exclude,
                           n_waves, t, cap, NULL, out);
    };
    const int rc = call(text.data(), want.size());
    int bad = rc != (fail_block >= 0 ? CBC_E_BLOCK : 0) || out[0] != want.size() || out[1] != lines || out[2] != kept || out[3] != points ||
              memcmp(text.data(), want.data(), want.size()) != 0;
    for (size_t i = want.size(); i < text.size(); i++) bad |= text[i] != 0xEEu;
    printf("%-70s %s (rc %d, %llu lines, %llu reads, %llu of %llu change points)\n", what, bad ? "MISMATCH" : "ok", rc, (unsigned long long)out[1],
           (unsigned long long)out[2], (unsigned long long)out[3], (unsigned long long)out[5]);
    if (!bad && want.size() > 0) bad |= fab_short_probe(what, 70, call, want.size(), out);
    return bad;
}

int main()
{
    int bad = 0;
    const vu none;
    fab f; f.stride = 152u; f.per_read = 80u; f.bases = false;
    static const uint32_t lens[] = { 1, 3, 4, 5, 63, 64, 65, 100, 150 };
    uint32_t pos = 5;
    for (size_t i = 0; i < sizeof lens / sizeof lens[0]; i++) {
        const uint32_t L = lens[i];
        fab_read(f, pos += 7u, 0u, L, vu(), vu());                                /* no edits */
        fab_read(f, pos += 1u, 16u, L, vu{ 0u }, vu());                           /* a deletion before the first base */
        fab_read(f, pos += 1u, 0u, L, vu{ L }, vu());                             /* one after the last, at matched coordinate T */
        fab_read(f, pos += 1u, 16u, L, vu{ L / 2u, L / 2u }, vu());               /* two deletions at one coordinate: a run of 2 */
        fab_read(f, pos += 1u, 0u, L, vu(), vu{ 0u });                            /* insertions change nothing */
        if (L >= 5u) {
            fab_read(f, pos += 1u, 0u, L, vu{ 2u }, vu{ 2u, 3u });
            fab_read(f, pos += 1u, 16u, L, vu{ 1u, 3u, 3u }, vu{ 0u, 1u, L - 2u, L - 1u });   /* separate runs */
            fab_read(f, pos += 1u, 0u, L, vu{ 1u, 2u, 4u }, vu());                /* three separate runs: 8 change points */
        }
        fab_read(f, pos += 1u, 0u, L, vu{ 70000u % 65536u, 60000u }, vu(), (int)L);   /* hostile entries that map past the span: ignored */
        vu run70(70u, L / 2u);
        fab_read(f, pos += 1u, 0u, L, run70, vu());                               /* a run of 70: a second turn of lanes */
    }
    while (f.reads.size() < 0u + 1u + 63u + 64u + 65u + 60u)
        fab_read(f, pos += 3u, (rnd() & 1u) * 16u, 100u, rnd() % 3u ? vu() : vu{ 40u, 40u, 41u }, rnd() % 4u ? vu() : vu{ 10u, 11u, 50u });
    {
        const uint32_t sizes[] = { 0, 1, 63, 64, 65 };
        uint32_t at = 0;
        for (int i = 0; i < 5; i++) { f.block_n.push_back(sizes[i]); at += sizes[i]; }
        f.block_n.push_back((uint32_t)f.reads.size() - at);
    }
    const uint64_t last = pos + 400u;
    bad |= fab_check("every case, whole window, one wavefront per block", f, 1u, last, none, 0u, 1u);
    bad |= fab_check("every case, whole window, four wavefronts per block", f, 1u, last, none, 0u, 4u);
    bad |= fab_check("exclude 16, three wavefronts", f, 1u, last, none, 16u, 3u);
    bad |= fab_check("exclude 0xffff keeps the FLAG 0 reads", f, 1u, last, none, 0xffffu, 4u);
    bad |= fab_check("a failed block", f, 1u, last, none, 0u, 4u, 3);
    bad |= fab_check("a window of more than one tile", f, 1u, 9000u, none, 0u, 4u);
    /* windows that start and end inside a read and inside its deleted bases */
    for (size_t i = 0; i < f.reads.size(); i += 3u) {
        const fread_ &r = f.reads[i];
        char what[96];
        snprintf(what, sizeof what, "window inside read %zu", i);
        bad |= fab_check(what, f, r.pos + 1u, r.pos + (r.span > 2u ? r.span - 2u : 1u), none, 0u, 2u);
        if (r.dc.empty() || r.dc[0] >= r.span) continue;
        const uint32_t d0 = r.pos + r.dc[0];                           /* the first deleted base */
        snprintf(what, sizeof what, "window on / cut by the deleted bases of read %zu", i);
        bad |= fab_check(what, f, d0, d0, none, 0u, 4u);
        bad |= fab_check(what, f, 1u, d0, none, 0u, 4u);
        bad |= fab_check(what, f, d0 + 1u, last, none, 0u, 4u);
        /* the same cuts as intervals: the deleted base on an interval's last position, a gap across the run, two far apart */
        snprintf(what, sizeof what, "intervals on / cut by the deleted bases of read %zu", i);
        bad |= fab_check(what, f, 1u, 1u, vu{ r.pos > 3u ? r.pos - 3u : 1u, d0 }, 0u, 4u);
        bad |= fab_check(what, f, 1u, 1u, vu{ r.pos > 3u ? r.pos - 3u : 1u, d0, d0 + 2u, d0 + 60u }, 0u, 3u);
        bad |= fab_check(what, f, 1u, 1u, vu{ 1u, d0 > 2u ? d0 - 1u : 1u, d0 + 70u, (uint32_t)last }, 16u, 1u);
    }
    bad |= fab_check("one interval over everything", f, 1u, 1u, vu{ 1u, (uint32_t)last }, 0u, 4u);
    bad |= fab_check("intervals of one position each", f, 1u, 1u, vu{ 10u, 10u, 12u, 12u, 14u, 14u, 40u, 40u, 100u, 100u }, 0u, 4u);
    bad |= fab_check("intervals, a failed block", f, 1u, 1u, vu{ 20u, 300u, 500u, 4200u }, 0u, 4u, 2);
    {   /* 64 reads apart, three separate deletion runs each: 8 change points per read, at exactly two arena entries per read too few
         * to waste: the bound is met with per_read = 3 */
        fab g; g.stride = 104u; g.per_read = 3u; g.bases = false;
        for (uint32_t i = 0; i < 64u; i++) fab_read(g, 10u + 200u * i, 0u, 100u, vu{ 20u, 40u, 60u }, vu());
        g.block_n.push_back(64u);
        bad |= fab_check("64 reads apart with three deletion runs each", g, 1u, 13000u, none, 0u, 4u);
        bad |= fab_check("the same over two intervals", g, 1u, 1u, vu{ 1u, 6000u, 6002u, 13000u }, 0u, 4u);
    }
    {   /* 300 reads deleting the same two positions: the words cancel to two change points of weight 300 */
        fab g; g.stride = 8u; g.per_read = 2u; g.bases = false;
        for (uint32_t i = 0; i < 300u; i++) fab_read(g, 3u, 0u, 6u, vu{ 2u, 2u }, vu());
        g.block_n.push_back(300u);
        bad |= fab_check("300 reads deleting the same positions: an arena of exactly the needed size", g, 1u, 40u, none, 0u, 4u);
        bad |= fab_check("the same over an interval that ends on the deleted bases", g, 1u, 1u, vu{ 2u, 6u }, 0u, 4u);
    }
    if (g_emu_errors) bad = 1;
    printf(bad ? "SKIPDEL EMU CHECK FAILED\n" : "SKIPDEL EMU CHECK OK\n");
    return bad;
}
#endif
