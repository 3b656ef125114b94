/*
 * pileup_strand_emu.cpp -- the pileup bodies of cbc_gpu_decode_pileup_ext (cbc_amd/csrc/cbc_pileup_body.h: the events into the
 * planes of the read's strand, the line passes with the fraction rule and the per-strand columns) on the
 * CPU through the lock-step wave emulation.  TEST AID ONLY: the passes are run in the call's order -- zero, cbc_depth_mark,
 * (cbc_depth_mark of the forward reads,) events, cbc_depth_tile and the scan (twice with by_strand), count, the scan, write --
 * behind the emulated decoder of tests/pileup_emu, or on records, rows and arena entries the stand-alone program fabricates,
 * under ASan-able host code before anything runs on a GPU.  Every table is an allocation of exactly its size and named to the
 * emulation, so an index past one is a finding.  With -DPILEUP_STRAND_EMU_MAIN the file is a stand-alone program that builds the
 * fabricated cases itself (those of tests/pileup_emu with forward, reverse and mixed strands, and the fraction rule's edges),
 * compares them with a base-by-base host loop and exits non-zero on a mismatch (make asan_check).
 */
#include <vector>
#include <string>
#include "../pileup_emu/wave_emu_pileup.h"
#include "../../cbc_amd/csrc/cbc_pileup_body.h"

typedef WaveEmuPileup WP;

static int g_emu_errors = 0;
extern "C" void emu_oob(const char *what) { fprintf(stderr, "[emu] invariant violated: %s\n", what); g_emu_errors++; }

template <int M>
static void count_and_write(const cbc_pileup_args &A, const cbc_pileup_sx &X, uint32_t n_tiles, std::vector<uint64_t> &offsets,
                            const std::vector<cbc_block_result> &counts, const std::vector<uint32_t> &ctr, uint64_t text_cap, uint64_t *out, int &rc)
{
    for (uint32_t t = 0; t < n_tiles; t++) cbc_pileup_count<WP, M>(A, t, &X);
    for (uint32_t t = 0; t < n_tiles; t++) offsets[t + 1u] = offsets[t] + counts[t].nbytes;
    out[0] = offsets[n_tiles]; out[1] = ctr[1]; out[2] = ctr[0];
    if (out[0] > text_cap) rc = CBC_E_ARG;
    else for (uint32_t t = 0; t < n_tiles; t++) cbc_pileup_write<WP, M>(A, t, &X);
}

/* ONE cbc_gpu_decode_pileup_ext behind the decode.  out[0] = text bytes (also when text_cap is too small: CBC_E_ARG, nothing
 * written), out[1] = lines, out[2] = reads kept.  CBC_E_BLOCK (after the text of the other blocks) when a block of the call
 * failed.  n_waves wavefronts share a block in the events pass.  ppm = 0 and by_strand = 0 run the plain bodies.
 * seed_depth, seed_cnt (the stand-alone check's ten-digit numbers; 0 otherwise): added before the passes to word 0 of the
 * difference arrays and of every plane, as if that many reads had started and been observed at the window's first position. */
extern "C" __attribute__((visibility("default")))
int emu_pileup_ext(const cbc_read_rec *recs, uint64_t n_recs, const uint8_t *seq, uint64_t seq_bytes, const cbc_dec_block_desc *blocks,
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
    if (bs) count_and_write<CBC_PILEUP_STRAND>(A, X, n_tiles, offsets, counts, ctr, text_cap, out, rc);
    else if (ppm) count_and_write<CBC_PILEUP_FRAC>(A, X, n_tiles, offsets, counts, ctr, text_cap, out, rc);
    else count_and_write<0>(A, X, n_tiles, offsets, counts, ctr, text_cap, out, rc);
    WP::clear_ranges();
    WP::edit_arena(nullptr, 0);
    if (g_emu_errors) return -100;
    if (rc) return rc;
    for (uint32_t b = 0; b < n_blocks; b++) if (dec_results[b].status != CBC_ST_OK) return CBC_E_BLOCK;
    return 0;
}

#ifdef PILEUP_STRAND_EMU_MAIN
/* ---- the stand-alone check: fabricated records, rows and arena entries against a base-by-base host loop ---------------------- */
struct fread_ { uint32_t pos, flag, span; std::string seq; std::vector<uint32_t> dc, oi; };
struct fab {
    uint32_t stride, per_read;
    std::vector<fread_> reads;
    std::vector<uint32_t> block_n;                                    /* reads per block */
    std::vector<uint8_t> ref;                                         /* window start 0: position p is ref[p - 1] */
};

static uint32_t g_rng = 2463534242u;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5; return g_rng; }

static uint32_t klass(uint8_t b) { b &= 0xdfu; return b == 'A' ? 0u : b == 'C' ? 1u : b == 'G' ? 2u : b == 'T' ? 3u : 4u; }

/* a read of `len` bases at `pos` with the given edits; span < 0: the honest one */
static void fab_read(fab &f, uint32_t pos, uint32_t flag, uint32_t len, std::vector<uint32_t> dc, std::vector<uint32_t> oi, int span = -1)
{
    fread_ r;
    r.pos = pos; r.flag = flag; r.dc = dc; r.oi = oi;
    r.span = span >= 0 ? (uint32_t)span : len + (uint32_t)dc.size() - (uint32_t)oi.size();
    for (uint32_t i = 0; i < len; i++) r.seq.push_back("ACGTNacgtRn"[rnd() % 11u]);
    f.reads.push_back(r);
}

struct tables { std::vector<uint64_t> cnt[5], del, ins, depth; uint64_t kept; };

/* the definitions of include/cbc_gpu.h, one base at a time */
static void want_tables(const fab &f, uint64_t beg, uint64_t end, uint32_t exclude, const std::vector<int> &failed, tables &T)
{
    const size_t W = (size_t)(end - beg + 1u);
    for (int k = 0; k < 5; k++) T.cnt[k].assign(W, 0);
    T.del.assign(W, 0); T.ins.assign(W, 0); T.depth.assign(W, 0); T.kept = 0;
    size_t at = 0;
    for (size_t b = 0; b < f.block_n.size(); b++)
        for (uint32_t k = 0; k < f.block_n[b]; k++, at++) {
            const fread_ &r = f.reads[at];
            if (failed[b] || r.span < 1u || (r.flag & exclude) || r.pos > end || (uint64_t)r.pos + r.span - 1u < beg) continue;
            T.kept++;
            for (uint64_t p = r.pos; p < (uint64_t)r.pos + r.span; p++) if (p >= beg && p <= end) T.depth[p - beg]++;
            const uint32_t rl = (uint32_t)r.seq.size();
            bool prev_ins = false;
            int64_t last = -1;                                       /* offset of the nearest aligned base before q */
            for (uint32_t q = 0; q < rl; q++) {
                uint32_t nb = 0; bool isins = false;
                for (uint32_t o : r.oi) { nb += o < q; isins |= o == q; }
                const uint32_t m = q - nb;
                uint32_t sh = 0;
                for (uint32_t d : r.dc) sh += d <= m;
                if (!isins) {
                    last = (int64_t)m + sh;
                    const uint64_t p = (uint64_t)r.pos + m + sh;
                    if ((uint64_t)m + sh < r.span && p >= beg && p <= end) T.cnt[klass((uint8_t)r.seq[q])][p - beg]++;
                } else if (!prev_ins) {
                    /* `last` is the aligned base in front of the run whether or not it fell inside the span */
                    const uint64_t off = m == 0u ? 0u : (uint64_t)last, p = r.pos + off;
                    if (off < r.span && p >= beg && p <= end) T.ins[p - beg]++;
                }
                prev_ins = isins;
            }
            for (size_t d = 0; d < r.dc.size(); d++) {
                const uint64_t off = (uint64_t)r.dc[d] + d, p = r.pos + off;
                if (off < r.span && p >= beg && p <= end) T.del[p - beg]++;
            }
        }
}

/* the seven counts of position i as the device sees them: depth is the span depth, the reference's class takes what the others
 * leave, everything modulo 2^32; seeds: what emu_pileup_ext was told to add at the window's first position.  Returns nonref. */
static uint64_t want_counts(const tables &T, size_t i, uint8_t rb, uint32_t seed_depth, uint32_t seed_cnt, uint32_t &depth, uint32_t *c)
{
    uint32_t mis = 0;
    depth = (uint32_t)T.depth[i] + seed_depth;
    for (uint32_t k = 0; k < 5u; k++) { c[k] = (k != klass(rb) ? (uint32_t)T.cnt[k][i] : 0u) + (i == 0 ? seed_cnt : 0u); mis += c[k]; }
    c[5] = (uint32_t)T.del[i] + (i == 0 ? seed_cnt : 0u); c[6] = (uint32_t)T.ins[i] + (i == 0 ? seed_cnt : 0u);
    const uint32_t nonref = mis + c[5] + c[6];
    c[klass(rb)] = depth - c[5] - mis;
    return nonref;
}

static std::string want_text(const fab &f, const std::string &name, uint64_t beg, uint64_t end, uint32_t min_alt, uint32_t ppm, bool by_strand,
                             uint32_t seed_depth, uint32_t seed_cnt, const tables &T, const tables &TF, uint64_t &lines)
{
    std::string out;
    lines = 0;
    for (uint64_t p = beg; p <= end; p++) {
        const size_t i = (size_t)(p - beg);
        const uint8_t rb = p - 1u < f.ref.size() ? f.ref[p - 1u] : (uint8_t)'N';
        uint32_t depth, c[7], depthf, cf[7];
        const uint64_t nonref = want_counts(T, i, rb, seed_depth, by_strand ? 2u * seed_cnt : seed_cnt, depth, c);
        if (nonref < min_alt || nonref * 1000000ull < (uint64_t)ppm * depth) continue;
        char buf[1024];
        int n = snprintf(buf, sizeof buf, "%s\t%llu\t%c\t%u\t%u\t%u\t%u\t%u\t%u\t%u\t%u", name.c_str(), (unsigned long long)p, rb, depth, c[0], c[1], c[2], c[3], c[4], c[5], c[6]);
        if (by_strand) {
            want_counts(TF, i, rb, seed_depth, seed_cnt, depthf, cf);
            n += snprintf(buf + n, sizeof buf - n, "\t%u\t%u\t%u\t%u\t%u\t%u\t%u", cf[0], cf[1], cf[2], cf[3], cf[4], cf[5], cf[6]);
        }
        out += buf; out += "\n"; lines++;
    }
    return out;
}

struct opt { uint32_t exclude, min_alt, ppm, by_strand, n_waves; int fail_block; uint32_t seed_depth, seed_cnt; const char *name; };
static opt O(uint32_t exclude, uint32_t min_alt, uint32_t n_waves, uint32_t ppm = 0u, uint32_t by_strand = 1u, int fail_block = -1)
{
    const opt o = { exclude, min_alt, ppm, by_strand, n_waves, fail_block, 0u, 0u, "ctg" };
    return o;
}

static size_t g_longest = 0;                                          /* the longest line any case produced */

static int fab_check(const char *what, const fab &f, uint64_t beg, uint64_t end, const opt &o)
{
    const std::string name = o.name;
    const size_t n = f.reads.size();
    std::vector<cbc_read_rec> recs(n ? n : 1);
    std::vector<uint8_t> rows(n * f.stride + 8u, 0xEEu);            /* exactly the spare bytes cbc_region_block asks for */
    std::vector<uint32_t> side(2u * (n ? n : 1), 0u);
    std::vector<uint16_t> arena(n * f.per_read, 0xEEEEu);
    std::vector<cbc_dec_block_desc> blocks(f.block_n.size());
    std::vector<uint64_t> ws(f.block_n.size(), 0u);
    std::vector<cbc_block_result> res(f.block_n.size());
    std::vector<int> failed(f.block_n.size(), 0);
    size_t at = 0;
    for (size_t b = 0; b < f.block_n.size(); b++) {
        memset(&blocks[b], 0, sizeof blocks[b]); memset(&res[b], 0, sizeof res[b]);
        blocks[b].rec_base = at; blocks[b].seq_base = (uint64_t)at * f.stride; blocks[b].n_reads = f.block_n[b]; blocks[b].seq_stride = f.stride;
        uint32_t used = 0;
        for (uint32_t k = 0; k < f.block_n[b]; k++, at++) {
            const fread_ &r = f.reads[at];
            uint32_t *w = (uint32_t *)&recs[at];
            w[0] = r.pos; w[1] = r.flag | ((uint32_t)r.seq.size() << 16); w[2] = k * f.stride; w[3] = r.span;
            memcpy(rows.data() + at * f.stride, r.seq.data(), r.seq.size());
            side[2 * at] = (r.dc.size() + r.oi.size()) ? used : 0u;
            side[2 * at + 1] = (uint32_t)r.dc.size() | ((uint32_t)r.oi.size() << 16);
            for (uint32_t d : r.dc) arena[blocks[b].rec_base * f.per_read + used++] = (uint16_t)d;
            for (uint32_t oo : r.oi) arena[blocks[b].rec_base * f.per_read + used++] = (uint16_t)oo;
            if (used > f.block_n[b] * f.per_read) { printf("%-76s BAD FIXTURE\n", what); return 1; }
        }
        if ((int)b == o.fail_block) { res[b].status = CBC_ST_EDITS; failed[b] = 1; }
    }
    tables T, TF;
    want_tables(f, beg, end, o.exclude, failed, T);
    want_tables(f, beg, end, o.exclude | 16u, failed, TF);
    uint64_t lines = 0;
    const std::string want = want_text(f, name, beg, end, o.min_alt, o.ppm, o.by_strand != 0u, o.seed_depth, o.seed_cnt, T, TF, lines);
    for (size_t s = 0, e; (e = want.find('\n', s)) != std::string::npos; s = e + 1u) if (e + 1u - s > g_longest) g_longest = e + 1u - s;
    std::vector<uint8_t> text(want.size() + 16u, 0xEEu);
    uint64_t out[4] = { 0, 0, 0, 0 };
    const int rc = emu_pileup_ext(recs.data(), n, rows.data(), rows.size(), blocks.data(), ws.data(), res.data(), (uint32_t)blocks.size(), side.data(),
                                  arena.data(), f.per_read, f.ref.data(), f.ref.size(), 0u, name.c_str(), (uint32_t)name.size(), beg, end, o.exclude,
                                  o.min_alt, o.ppm, o.by_strand, o.n_waves, o.seed_depth, o.seed_cnt, text.data(), want.size(), out);
    int bad = rc != (o.fail_block >= 0 ? CBC_E_BLOCK : 0) || out[0] != want.size() || out[1] != lines || out[2] != T.kept ||
              memcmp(text.data(), want.data(), want.size()) != 0;
    for (size_t i = want.size(); i < text.size(); i++) bad |= text[i] != 0xEEu;
    printf("%-76s %s (rc %d, %llu lines, %llu reads)\n", what, bad ? "MISMATCH" : "ok", rc, (unsigned long long)out[1], (unsigned long long)out[2]);
    if (!bad && want.size() > 0) {                                   /* one byte short: the size, CBC_E_ARG, nothing written */
        std::vector<uint8_t> t2(want.size() + 16u, 0xEEu);
        const int rc2 = emu_pileup_ext(recs.data(), n, rows.data(), rows.size(), blocks.data(), ws.data(), res.data(), (uint32_t)blocks.size(),
                                       side.data(), arena.data(), f.per_read, f.ref.data(), f.ref.size(), 0u, name.c_str(), (uint32_t)name.size(),
                                       beg, end, o.exclude, o.min_alt, o.ppm, o.by_strand, o.n_waves, o.seed_depth, o.seed_cnt, t2.data(),
                                       want.size() - 1u, out);
        bad |= rc2 != CBC_E_ARG || out[0] != want.size();
        for (size_t i = 0; i < t2.size(); i++) bad |= t2[i] != 0xEEu;
        if (bad) printf("%-76s MISMATCH (text_cap one byte short: rc %d)\n", what, rc2);
    }
    return bad;
}

typedef std::vector<uint32_t> vu;

/* the cases of tests/pileup_emu's check with the strands as `strand` says: 0 every read forward, 1 every read reverse, 2 as the
 * fixture has them (FLAG 0, 16 and 1024 mixed) */
static int strand_cases(uint32_t strand, int &n_cases)
{
    static const char *const sname[] = { "fwd", "rev", "mix" };
    int bad = 0;
    g_rng = 2463534242u;
    fab f; f.stride = 152u; f.per_read = 16u;
    for (uint32_t i = 0; i < 6000u; i++) f.ref.push_back("ACGTNacgtnRYk"[rnd() % 13u]);    /* lower-case and IUPAC reference bytes */
    static const uint32_t lens[] = { 1, 3, 4, 5, 63, 64, 65, 100, 150 };
    uint32_t pos = 5;
    for (size_t i = 0; i < sizeof lens / sizeof lens[0]; i++) {
        const uint32_t L = lens[i];
        fab_read(f, pos += 7u, 0u, L, vu(), vu());                                /* no edits */
        fab_read(f, pos += 1u, 16u, L, vu{ 0u }, vu());                           /* a deletion before the first base */
        fab_read(f, pos += 1u, 0u, L, vu{ L }, vu());                             /* one after the last, at matched coordinate T */
        fab_read(f, pos += 1u, 16u, L, vu{ L / 2u, L / 2u }, vu());               /* two deletions at one coordinate */
        fab_read(f, pos += 1u, 0u, L, vu(), vu{ 0u });                            /* an insertion run at read index 0 */
        fab_read(f, pos += 1u, 1024u, L, vu(), vu{ L - 1u });                     /* and one at rl - 1 */
        if (L >= 5u) {
            fab_read(f, pos += 1u, 0u, L, vu{ 2u }, vu{ 2u, 3u });                /* an insertion run directly after a deletion */
            fab_read(f, pos += 1u, 16u, L, vu{ 1u, 3u, 3u }, vu{ 0u, 1u, L - 2u, L - 1u });
        }
        vu all; for (uint32_t q = 0; q < L; q++) all.push_back(q);
        if (L <= 65u) {
            fab_read(f, pos += 1u, 0u, L, vu{ 0u, 0u }, all);                     /* nothing but insertions over two deleted bases */
            fab_read(f, pos += 1u, 0u, L, vu(), all);                             /* span 0: not kept */
        }
        fab_read(f, pos += 1u, 0u, L, vu{ 70000u % 65536u, 60000u }, vu(), (int)L);   /* hostile entries that map past the span: ignored */
        fab_read(f, pos += 1u, 0u, L, vu(), vu{ 0u }, (int)(L > 1u ? L - 1u : 1u));
    }
    while (f.reads.size() < 0u + 1u + 63u + 64u + 65u + 40u) fab_read(f, pos += 3u, (rnd() & 1u) * 16u, 100u, rnd() % 3u ? vu() : vu{ 40u, 40u, 41u }, rnd() % 4u ? vu() : vu{ 10u, 11u, 50u });
    for (fread_ &r : f.reads) r.flag = strand == 0u ? r.flag & ~16u : strand == 1u ? r.flag | 16u : r.flag;
    {
        const uint32_t sizes[] = { 0, 1, 63, 64, 65 };
        uint32_t at = 0;
        for (int i = 0; i < 5; i++) { f.block_n.push_back(sizes[i]); at += sizes[i]; }
        f.block_n.push_back((uint32_t)f.reads.size() - at);
    }
    const uint64_t last = pos + 160u;
    if (last > f.ref.size()) { printf("BAD FIXTURE: the reference is too short\n"); return 1; }
    char what[128];
#define CASE(text, ...) do { snprintf(what, sizeof what, "%s: %s", sname[strand], text); bad |= fab_check(what, __VA_ARGS__); n_cases++; } while (0)
    CASE("every case, whole window, one wavefront per block", f, 1u, last, O(0u, 1u, 1u));
    CASE("every case, whole window, four wavefronts per block", f, 1u, last, O(0u, 1u, 4u));
    CASE("min_alt 2, exclude 16, three wavefronts", f, 1u, last, O(16u, 2u, 3u));
    CASE("min_alt above every depth: empty", f, 1u, last, O(0u, 100000u, 4u));
    CASE("exclude 0xffff keeps the FLAG 0 reads", f, 1u, last, O(0xffffu, 1u, 4u));
    CASE("a failed block", f, 1u, last, O(0u, 1u, 4u, 0u, 1u, 3));
    /* windows that start and end inside a read, inside its deleted bases, and on an insertion's anchor */
    const fread_ &r2 = f.reads[f.reads.size() - 9u];
    for (size_t i = 0; i < f.reads.size(); i += 5u) {
        const fread_ &r = f.reads[i];
        char w2[96];
        snprintf(w2, sizeof w2, "window inside read %zu", i);
        CASE(w2, f, r.pos + 1u, r.pos + (r.span > 2u ? r.span - 2u : 1u), O(0u, 1u, 2u));
        if (!r.dc.empty()) { snprintf(w2, sizeof w2, "window on the deleted bases of read %zu", i); CASE(w2, f, r.pos + r.dc[0], r.pos + r.dc[0], O(0u, 1u, 4u)); }
        if (!r.oi.empty() && r.oi[0] > 0u) {
            snprintf(w2, sizeof w2, "window ends on / starts behind the anchor of read %zu", i);
            CASE(w2, f, 1u, r.pos + r.oi[0] - 1u, O(0u, 1u, 4u));
            CASE(w2, f, r.pos + r.oi[0], last, O(0u, 1u, 4u));
        }
    }
    CASE("one position", f, r2.pos, r2.pos, O(0u, 1u, 4u));
    CASE("a window of more than one tile", f, 1u, 6000u, O(0u, 1u, 4u));
    {   /* counters: 300 reads at one place, all mismatching, one deletion and one insertion each */
        fab g; g.stride = 8u; g.per_read = 2u;
        g.ref.assign(64u, 'A');
        for (uint32_t i = 0; i < 300u; i++) { fab_read(g, 3u, strand == 2u ? (i & 1u) * 16u : strand * 16u, 6u, vu{ 2u }, vu{ 4u }); g.reads.back().seq = "CCGGTT"; }
        g.block_n.push_back(300u);
        CASE("300 reads on one position: an arena of exactly the needed size", g, 1u, 40u, O(0u, 1u, 4u));
    }
    /* the same fixture through the fraction rule, with and without the columns, and the plain bodies through this driver */
    CASE("fraction 0.02 with the columns", f, 1u, last, O(0u, 1u, 4u, 20000u, 1u));
    CASE("fraction 0.5 alone, more than one tile", f, 1u, 6000u, O(0u, 1u, 4u, 500000u, 0u));
    CASE("fraction 1 with min_alt 2 and the columns", f, 1u, last, O(0u, 2u, 3u, 1000000u, 1u));
    CASE("neither option: the plain bodies", f, 1u, last, O(0u, 1u, 4u, 0u, 0u));
#undef CASE
    return bad;
}

int main()
{
    int bad = 0, n_cases = 0;
    for (uint32_t strand = 0; strand < 3u; strand++) bad |= strand_cases(strand, n_cases);
    printf("%d cases over the three strand settings\n", n_cases);
    {   /* the rule at equality and one below: depth 20, one alternative base (a C over A), on both strands in turn */
        for (uint32_t rev = 0; rev < 2u; rev++) {
            fab g; g.stride = 8u; g.per_read = 2u;
            g.ref.assign(64u, 'A');
            for (uint32_t i = 0; i < 20u; i++) { fab_read(g, 3u, (i == 0u ? rev : i & 1u) * 16u, 6u, vu(), vu()); g.reads.back().seq = i == 0u ? "AACAAA" : "AAAAAA"; }
            g.block_n.push_back(20u);
            for (uint32_t bs = 0; bs < 2u; bs++) {
                uint64_t lines = 0;
                tables T, TF;
                want_tables(g, 1u, 40u, 0u, std::vector<int>(1, 0), T); want_tables(g, 1u, 40u, 16u, std::vector<int>(1, 0), TF);
                const bool kept = want_text(g, "ctg", 1u, 40u, 1u, 50000u, bs != 0u, 0u, 0u, T, TF, lines).size() > 0 && lines == 1;
                want_text(g, "ctg", 1u, 40u, 1u, 50001u, bs != 0u, 0u, 0u, T, TF, lines);
                if (!kept || lines != 0) { printf("BAD FIXTURE: 1 of 20 is not kept at 0.05 and dropped at 0.050001\n"); bad = 1; }
                bad |= fab_check("depth 20, 1 alternative, F = 0.05: kept", g, 1u, 40u, O(0u, 1u, 4u, 50000u, bs));
                bad |= fab_check("depth 20, 1 alternative, F = 0.050001: dropped", g, 1u, 40u, O(0u, 1u, 4u, 50001u, bs));
            }
        }
    }
    {   /* ins > depth: one read of one aligned base with two insertion runs anchored on it (index 0: anchor POS; index 2: the base) */
        fab g; g.stride = 8u; g.per_read = 4u;
        g.ref.assign(64u, 'A');
        fab_read(g, 5u, 16u, 3u, vu(), vu{ 0u, 2u }); g.reads.back().seq = "CAC";
        g.block_n.push_back(1u);
        tables T; want_tables(g, 1u, 40u, 0u, std::vector<int>(1, 0), T);
        if (!(T.ins[4] == 2 && T.depth[4] == 1)) { printf("BAD FIXTURE: ins is not above the depth\n"); bad = 1; }
        bad |= fab_check("ins 2 over depth 1 passes F = 1", g, 1u, 40u, O(0u, 1u, 4u, 1000000u, 1u));
        bad |= fab_check("ins 2 over depth 1 passes F = 1, without the columns", g, 1u, 40u, O(0u, 2u, 4u, 1000000u, 0u));
    }
    {   /* the longest line: a 255-byte name, pos1 and all fifteen counts with ten digits (seeded at the window's first position,
         * which lies past the reference: its byte reads as N) */
        fab g; g.stride = 8u; g.per_read = 2u;
        g.ref.assign(64u, 'A');
        g.block_n.push_back(0u);
        opt o = O(0u, 1u, 4u, 100000u, 1u);                          /* both products of the rule pass 2^32 */
        const std::string nm(255u, 'n');
        o.name = nm.c_str(); o.seed_depth = 3000000000u; o.seed_cnt = 1000000000u;
        g_longest = 0;
        bad |= fab_check("a 255-byte name and sixteen ten-digit numbers", g, 2147483000u, 2147483647u, o);
        if (g_longest != 255u + 102u + 77u) { printf("BAD FIXTURE: the longest line has %zu bytes, not %u\n", g_longest, 255u + 102u + 77u); bad = 1; }
        o.by_strand = 0u;
        g_longest = 0;
        bad |= fab_check("a 255-byte name and nine ten-digit numbers, the fraction rule alone", g, 2147483000u, 2147483647u, o);
        if (g_longest != 255u + 102u) { printf("BAD FIXTURE: the longest line has %zu bytes, not %u\n", g_longest, 255u + 102u); bad = 1; }
    }
    if (g_emu_errors) bad = 1;
    printf(bad ? "PILEUP STRAND EMU CHECK FAILED\n" : "PILEUP STRAND EMU CHECK OK\n");
    return bad;
}
#endif
