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
#include "../emu/post_emu.h"

/* ONE cbc_gpu_decode_pileup_ext behind the decode: the driver of tests/emu/post_emu.h, which says what the arguments and out[]
 * are.  ppm = 0 and by_strand = 0 run the plain bodies. */
extern "C" __attribute__((visibility("default")))
int emu_pileup_ext(const cbc_read_rec *recs, uint64_t n_recs, const uint8_t *seq, uint64_t seq_bytes, const cbc_dec_block_desc *blocks,
                   const uint64_t *window_start, const cbc_block_result *dec_results, uint32_t n_blocks, const uint32_t *side,
                   const uint16_t *arena, uint32_t per_read, const uint8_t *ref, uint64_t ref_bytes, uint64_t ref_c0, const char *name,
                   uint32_t name_len, uint64_t beg, uint64_t end, uint32_t exclude, uint32_t min_alt, uint32_t ppm, uint32_t by_strand,
                   uint32_t n_waves, uint32_t seed_depth, uint32_t seed_cnt, uint8_t *text, uint64_t text_cap, uint64_t *out)
{
    return emu_pileup_call(recs, n_recs, seq, seq_bytes, blocks, window_start, dec_results, n_blocks, side, arena, per_read, ref, ref_bytes, ref_c0,
                           name, name_len, beg, end, exclude, min_alt, ppm, by_strand, n_waves, seed_depth, seed_cnt, text, text_cap, out);
}

#ifdef PILEUP_STRAND_EMU_MAIN
#include "../emu/fab_reads.h"
/* ---- the stand-alone check: fabricated records, rows and arena entries against a base-by-base host loop ---------------------- */
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
    fab_arrays a;
    if (!fab_build(f, a, o.fail_block)) { printf("%-76s BAD FIXTURE\n", what); return 1; }
    tables T, TF;
    want_tables(f, beg, end, o.exclude, a.failed, T);
    want_tables(f, beg, end, o.exclude | 16u, a.failed, TF);
    uint64_t lines = 0;
    const std::string want = want_text(f, name, beg, end, o.min_alt, o.ppm, o.by_strand != 0u, o.seed_depth, o.seed_cnt, T, TF, lines);
    for (size_t s = 0, e; (e = want.find('\n', s)) != std::string::npos; s = e + 1u) if (e + 1u - s > g_longest) g_longest = e + 1u - s;
    std::vector<uint8_t> text(want.size() + 16u, 0xEEu);
    uint64_t out[4] = { 0, 0, 0, 0 };
    auto call = [&](uint8_t *t, uint64_t cap) {
        return emu_pileup_ext(a.recs.data(), f.reads.size(), a.rows.data(), a.rows.size(), a.blocks.data(), a.ws.data(), a.res.data(),
                              (uint32_t)a.blocks.size(), a.side.data(), a.arena.data(), f.per_read, f.ref.data(), f.ref.size(), 0u, name.c_str(),
                              (uint32_t)name.size(), beg, end, o.exclude, o.min_alt, o.ppm, o.by_strand, o.n_waves, o.seed_depth, o.seed_cnt, t, cap, out);
    };
    const int rc = call(text.data(), want.size());
    int bad = rc != (o.fail_block >= 0 ? CBC_E_BLOCK : 0) || out[0] != want.size() || out[1] != lines || out[2] != T.kept ||
              memcmp(text.data(), want.data(), want.size()) != 0;
    for (size_t i = want.size(); i < text.size(); i++) bad |= text[i] != 0xEEu;
    printf("%-76s %s (rc %d, %llu lines, %llu reads)\n", what, bad ? "MISMATCH" : "ok", rc, (unsigned long long)out[1], (unsigned long long)out[2]);
    if (!bad && want.size() > 0) bad |= fab_short_probe(what, 76, call, want.size(), out);
    return bad;
}

/* the cases of tests/pileup_emu's check with the strands as `strand` says: 0 every read forward, 1 every read reverse, 2 as the
 * fixture has them (FLAG 0, 16 and 1024 mixed) */
static int strand_cases(uint32_t strand, int &n_cases)
{
    static const char *const sname[] = { "fwd", "rev", "mix" };
    int bad = 0;
    g_rng = 2463534242u;
    fab f;
    uint32_t pos;
    fab_pileup_cases(f, pos);
    for (fread_ &r : f.reads) r.flag = strand == 0u ? r.flag & ~16u : strand == 1u ? r.flag | 16u : r.flag;
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
