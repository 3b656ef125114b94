/*
 * covx_emu.cpp -- the read-count and threshold bodies (cbc_amd/csrc/cbc_covx_body.h) on the CPU through the lock-step wave
 * emulation.  TEST AID ONLY: the passes are run behind the emulated span decoder, the mark pass that also notes the pieces'
 * first slots (cbc_targets_mark<W, true>) and the tile / compact passes over the difference array and over the starts (the
 * order of cbc_gpu_decode_coverage_ext), or straight on change points and start points the test fabricates.  The front of
 * the call, the scans between the passes and the passes of cbc_gpu_decode_coverage are those of tests/emu/post_emu.h.  Every
 * table the new passes touch is an allocation of its exact size, so an index past it is an ASan finding.  With -DCOVX_EMU_MAIN the file is a stand-alone program that builds
 * the fabricated cases itself, compares them with 64-bit host arithmetic and exits non-zero on a mismatch (make asan_check).
 */
#include "../emu/post_emu.h"
#include "../../cbc_amd/csrc/cbc_covx_body.h"

/* the span-reporting decoder over every block of the batch */
extern "C" __attribute__((visibility("default")))
int emu_covx_decode(const cbc_dec_device_batch *b, uint32_t smax) { return emu_decode_blocks<WP, true>(b, smax); }

/* the new passes over the first ncp change points and nsp start points: the thresholds' weights, scans and prefixes, the
 * lookup.  cp_cap sizes the run tiles and the prefix table as the device call does.  reads == NULL: no read counts, and no
 * start-point table is looked at. */
static void covx_passes(const uint32_t *cp_pos, const uint32_t *cp_dep, uint32_t ncp, uint32_t cp_cap, const uint32_t *sp_pos,
                        const uint32_t *sp_cnt, uint32_t nsp, uint32_t slots, const uint32_t *thr, uint32_t n_thr, const uint32_t *q,
                        uint32_t n_q, uint32_t *thr_covered, uint32_t *reads)
{
    const uint32_t n_ttiles = (cp_cap + CBC_DEPTH_LINES - 1u) / CBC_DEPTH_LINES;
    std::vector<uint32_t> pos(cp_pos, cp_pos + ncp), dep(cp_dep, cp_dep + ncp), qq(q, q + 2u * (size_t)n_q);
    std::vector<uint32_t> spos, scnt;
    if (reads) { spos.assign(sp_pos, sp_pos + nsp); scnt.assign(sp_cnt, sp_cnt + nsp); }
    std::vector<uint32_t> pre((size_t)n_thr * cp_cap, 0xEEEEEEEEu), tc((size_t)n_q * n_thr, 0xEEEEEEEEu), rd(reads ? n_q : 0u, 0xEEEEEEEEu);
    std::vector<cbc_block_result> tt((size_t)n_thr * n_ttiles);
    std::vector<uint64_t> toff((size_t)n_thr * (n_ttiles + 1u));
    const uint64_t cnt_off[1] = { ncp }, sp_off[1] = { nsp };      /* n_tiles = 0: [n_tiles] is the count */
    cbc_covx_args A;
    memset(&A, 0, sizeof A);
    A.cp_pos = pos.data(); A.cp_dep = dep.data(); A.cnt_off = cnt_off; A.n_tiles = 0u;
    if (reads) { A.sp_pos = spos.data(); A.sp_cnt = scnt.data(); A.sp_off = sp_off; A.reads = rd.data(); }
    A.tile_thr = tt.data(); A.thr_off = toff.data(); A.pre_thr = pre.data(); A.q = qq.data(); A.thr_covered = tc.data();
    for (uint32_t t = 0; t < n_thr; t++) A.thr[t] = thr[t];
    A.n_thr = n_thr; A.cp_cap = cp_cap; A.sp_cap = nsp; A.n_ttiles = n_ttiles; A.n_q = n_q; A.slots = slots;
    if (n_thr) {
        for (uint32_t t = 0; t < n_ttiles; t++) cbc_covx_weights<WP>(A, t);
        for (uint32_t t = 0; t < n_thr; t++) scan(tt.data() + (size_t)t * n_ttiles, toff.data() + (size_t)t * (n_ttiles + 1u), n_ttiles);
        for (uint32_t t = 0; t < n_ttiles; t++) cbc_covx_apply<WP>(A, t);
        for (uint32_t t = 0; t < n_thr; t++)
            for (uint32_t i = 0; i < ncp; i++) if (pre[(size_t)t * cp_cap + i] == 0xEEEEEEEEu) { emu_oob("a threshold prefix was not written"); t = n_thr; break; }
    }
    if (n_thr || reads) for (uint32_t w = 0; w < (n_q + 63u) / 64u; w++) cbc_covx_lookup<WP>(A, w);
    for (size_t i = 0; i < tc.size(); i++) thr_covered[i] = tc[i];
    for (size_t i = 0; i < rd.size(); i++) reads[i] = rd[i];
}

/* fabricated change points and start points straight into the passes (cp_cap = ncp: the tables are exactly as long as the
 * tiles assume) */
extern "C" __attribute__((visibility("default")))
int emu_covx_points(const uint32_t *cp_pos, const uint32_t *cp_dep, uint32_t ncp, const uint32_t *sp_pos, const uint32_t *sp_cnt,
                    uint32_t nsp, uint32_t slots, const uint32_t *thr, uint32_t n_thr, const uint32_t *q, uint32_t n_q,
                    uint32_t *thr_covered, uint32_t *reads)
{
    g_emu_errors = 0;
    if (n_thr > CBC_COVX_MAX_THR) return CBC_E_ARG;
    for (uint32_t i = 0; i < n_q; i++) if (q[2 * i] > slots || q[2 * i + 1] > slots - q[2 * i]) return CBC_E_ARG;
    covx_passes(cp_pos, cp_dep, ncp, ncp, sp_pos, sp_cnt, nsp, slots, thr, n_thr, q, n_q, thr_covered, reads);
    return g_emu_errors ? -100 : 0;
}

/* ONE contig's call (iv: its n_iv merged intervals; block_iv relative to them), every pass in the order of
 * cbc_gpu_decode_coverage_ext.  out[0] = reads kept, out[1] = change points, out[2] = slots, out[3] = start points.
 * CBC_E_BLOCK when a block of the call failed to decode (it marked nothing; the numbers are those of the other blocks -- the
 * device call zeroes them on the host). */
extern "C" __attribute__((visibility("default")))
int emu_covx(const cbc_read_rec *recs, uint64_t n_recs, const uint8_t *seq, uint64_t seq_bytes, const cbc_dec_block_desc *blocks,
             const uint64_t *window_start, const cbc_block_result *dec_results, uint32_t n_blocks, const uint32_t *iv, uint32_t n_iv,
             const uint32_t *block_iv, uint32_t exclude, uint32_t min_depth, const uint32_t *q, uint32_t n_q, uint64_t *sum,
             uint32_t *covered, const uint32_t *thr, uint32_t n_thr, uint32_t *thr_covered, uint32_t *reads, uint64_t *out)
{
    g_emu_errors = 0;
    out[0] = out[1] = out[2] = out[3] = 0;
    for (uint32_t i = 0; i < n_q; i++) { sum[i] = 0; covered[i] = 0; if (reads) reads[i] = 0; }
    if (n_thr > CBC_COVX_MAX_THR) return CBC_E_ARG;
    for (uint64_t i = 0; i < (uint64_t)n_q * n_thr; i++) thr_covered[i] = 0;
    for (uint32_t t = 0; t < n_thr; t++) if (thr[t] < 1u || (t && thr[t] <= thr[t - 1])) return CBC_E_ARG;
    if (n_recs > 0x3fffffffull || n_iv == 0 || min_depth < 1u) return CBC_E_ARG;
    emu_depth_front F;
    if (F.intervals(iv, n_iv, block_iv, n_blocks)) return CBC_E_ARG;
    const uint64_t d_words = F.d_words;
    for (uint32_t i = 0; i < n_q; i++) if (q[2 * i] > d_words || q[2 * i + 1] > d_words - q[2 * i]) return CBC_E_ARG;
    const uint32_t cp_cap = (uint32_t)(2u * n_recs + 2u * (uint64_t)n_iv), sp_cap = (uint32_t)(n_recs + n_iv);
    F.tables(recs, n_recs, seq, seq_bytes, blocks, window_start, dec_results, n_blocks, exclude, cp_cap);
    const uint32_t n_tiles = F.n_tiles;
    std::vector<uint32_t> starts(reads ? (size_t)n_tiles * CBC_DEPTH_TILE : 0u, 0u), sp_pos(sp_cap + 1u, 0xEEEEEEEEu), sp_cnt(sp_cap + 1u, 0xEEEEEEEEu);
    F.mark(reads ? starts.data() : nullptr);
    if (F.points()) return -100;
    uint32_t nsp = 0;
    if (reads) {                                                    /* the same two bodies over the starts */
        std::vector<cbc_block_result> ssum(n_tiles), scnt(n_tiles);
        std::vector<uint64_t> ssoff(n_tiles + 1u), scoff(n_tiles + 1u);
        cbc_depth_args S = F.A.D;
        S.diff = starts.data(); S.tile_sum = ssum.data(); S.tile_cnt = scnt.data(); S.sum_off = ssoff.data(); S.cnt_off = scoff.data();
        S.cp_pos = sp_pos.data(); S.cp_dep = sp_cnt.data(); S.cp_cap = sp_cap;
        if (emu_depth_points<WP>(S, ssoff.data(), scoff.data(), "start point", &nsp)) return -100;
    }
    const uint32_t ncp = F.ncp;
    cov_passes(F.cp_pos.data(), F.cp_dep.data(), ncp, cp_cap, (uint32_t)d_words, min_depth, q, n_q, sum, covered);
    covx_passes(F.cp_pos.data(), F.cp_dep.data(), ncp, cp_cap, sp_pos.data(), sp_cnt.data(), nsp, (uint32_t)d_words, thr, n_thr, q, n_q,
                thr_covered, reads);
    out[0] = F.ctr[0]; out[1] = ncp; out[2] = d_words; out[3] = nsp;
    if (g_emu_errors) return -100;
    for (uint32_t b = 0; b < n_blocks; b++) if (dec_results[b].status != CBC_ST_OK) return CBC_E_BLOCK;
    return 0;
}

#ifdef COVX_EMU_MAIN
/* ---- the stand-alone check: fabricated change points and start points against 64-bit host arithmetic ---------------------------- */
struct fab { std::vector<uint32_t> pos, dep, spos, scnt; uint64_t slots; };

static int fab_check(const char *what, const fab &f, const std::vector<uint32_t> &thr, const std::vector<uint32_t> &q, bool want_reads)
{
    const uint32_t n_q = (uint32_t)(q.size() / 2), T = (uint32_t)thr.size();
    std::vector<uint32_t> tc((size_t)n_q * T), rd(want_reads ? n_q : 0u);      /* exactly as long as the call writes */
    const int rc = emu_covx_points(f.pos.data(), f.dep.data(), (uint32_t)f.pos.size(), f.spos.data(), f.scnt.data(), (uint32_t)f.spos.size(),
                                   (uint32_t)f.slots, thr.data(), T, q.data(), n_q, tc.data(), want_reads ? rd.data() : NULL);
    int bad = rc != 0;
    for (uint32_t i = 0; i < n_q && !bad; i++) {
        const uint64_t a = q[2 * i], b = a + q[2 * i + 1];
        for (uint32_t t = 0; t < T; t++) {
            uint64_t c = 0;
            for (size_t j = 0; j + 1 < f.pos.size(); j++) {
                const uint64_t lo = f.pos[j] > a ? f.pos[j] : a, hi = f.pos[j + 1] < b ? f.pos[j + 1] : b;
                if (hi > lo && f.dep[j] >= thr[t]) c += hi - lo;
            }
            if (tc[(size_t)i * T + t] != (uint32_t)c) bad = 1;
        }
        if (want_reads) {
            uint32_t depth = 0, csa = 0, csb = 0;                    /* CS modulo 2^32, as the device keeps it */
            for (size_t j = 0; j + 1 < f.pos.size(); j++) if (f.pos[j] <= a && a < f.pos[j + 1]) depth = f.dep[j];
            for (size_t j = 0; j < f.spos.size(); j++) { if (f.spos[j] <= a) csa = f.scnt[j]; if (b && f.spos[j] <= b - 1u) csb = f.scnt[j]; }
            const uint32_t want = b > a ? depth + (csb - csa) : 0u;
            if (rd[i] != want) bad = 1;
        }
    }
    printf("%-52s %s (rc %d, %u queries, %u thresholds)\n", what, bad ? "MISMATCH" : "ok", rc, n_q, T);
    return bad;
}

static uint32_t rnd(uint64_t &s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }

int main()
{
    int bad = 0;
    uint64_t seed = 7;
    {   /* runs near 10^6 slots x 2500 (more than two tiles of runs), depths near 4 * 10^9, thresholds 1 and 2^32 - 1 and between */
        fab f; uint64_t at = 17;
        for (uint32_t i = 0; i < 2500u; i++) {
            f.pos.push_back((uint32_t)at);
            f.dep.push_back(i == 2499u ? 0u : i == 800u ? 1u : i == 1200u ? 0u : i == 1300u ? 0xffffffffu : 3900000000u + rnd(seed) % 300000000u);
            at += 900000u + rnd(seed) % 200000u;
        }
        f.slots = f.pos.back() + 5u;
        /* start points: one per change point and some between, the cumulative count passing 2^31 and wrapping 2^32 */
        uint32_t cs = 0;
        for (uint32_t i = 0; i < 2500u; i++) {
            cs += 1000000u + rnd(seed) % 1500000u; f.spos.push_back(f.pos[i]); f.scnt.push_back(cs);
            if (i % 3u == 0u) { cs += 1u + rnd(seed) % 5u; f.spos.push_back(f.pos[i] + 1u + rnd(seed) % 1000u); f.scnt.push_back(cs); }
        }
        std::vector<uint32_t> q;
        const uint32_t fixed[][2] = { { 0u, (uint32_t)f.slots }, { 0u, f.pos[0] }, { f.pos[0], 1u }, { f.pos[2499], 5u }, { f.pos[2499] - 1u, 6u },
                                      { (uint32_t)f.slots, 0u }, { f.pos[5], 0u }, { f.pos[1023], f.pos[1024] - f.pos[1023] },
                                      { f.pos[1024], f.pos[1025] - f.pos[1024] }, { f.pos[2047] + 3u, f.pos[2049] - f.pos[2047] },
                                      { f.pos[1300], 10u }, { f.pos[1300] - 4u, 9u }, { f.pos[800] - 1u, 3u } };
        for (size_t i = 0; i < sizeof fixed / sizeof fixed[0]; i++) { q.push_back(fixed[i][0]); q.push_back(fixed[i][1]); }
        for (int i = 0; i < 150; i++) { const uint32_t a = rnd(seed) % (uint32_t)f.slots; q.push_back(a); q.push_back(rnd(seed) % ((uint32_t)f.slots - a + 1u)); }
        bad |= fab_check("10^6-slot runs x 2500, thresholds 1 and 2^32 - 1", f, { 1u, 0xffffffffu }, q, true);
        bad |= fab_check("the same, 8 thresholds", f, { 1u, 2u, 3900000000u, 4000000000u, 4100000000u, 4199999999u, 4200000000u, 0xffffffffu }, q, true);
        bad |= fab_check("the same, one threshold, no read counts", f, { 4000000000u }, q, false);
        bad |= fab_check("the same, no threshold, read counts only", f, {}, q, true);
    }
    for (uint32_t ncp = 0; ncp <= 2; ncp++) {   /* no run at all, a lone change point, one run; no start point, then one */
        for (int sp = 0; sp < 2; sp++) {
            fab f; f.slots = 100;
            if (ncp == 2) { f.pos.push_back(9); f.dep.push_back(6); }
            if (ncp >= 1) { f.pos.push_back(49); f.dep.push_back(0); }
            if (sp && ncp == 2) { f.spos.push_back(9); f.scnt.push_back(6); }
            char what[64];
            snprintf(what, sizeof what, "ncp %u, %s", ncp, sp && ncp == 2 ? "one start point" : "no start point");
            bad |= fab_check(what, f, { 1u, 6u, 7u }, { 0u, 100u, 9u, 1u, 8u, 1u, 48u, 1u, 49u, 1u, 5u, 0u, 100u, 0u, 0u, 9u, 0u, 10u }, true);
        }
    }
    {   /* more than 64 queries on few points, every query start and end on, one before and one behind a point */
        fab f; f.slots = 5000;
        const uint32_t p[] = { 10, 11, 20, 64, 65, 4095, 4096, 4097, 4999 }, d[] = { 1, 3, 2, 0, 5, 1, 2, 1, 0 };
        for (size_t i = 0; i < 9; i++) { f.pos.push_back(p[i]); f.dep.push_back(d[i]); }
        const uint32_t s[] = { 10, 11, 65, 4095, 4096 }, c[] = { 1, 3, 8, 9, 10 };
        for (size_t i = 0; i < 5; i++) { f.spos.push_back(s[i]); f.scnt.push_back(c[i]); }
        std::vector<uint32_t> q;
        for (size_t i = 0; i < 9; i++)
            for (int da = -1; da <= 1; da++)
                for (uint32_t len = 0; len <= 3; len++) if (p[i] + da + len <= f.slots) { q.push_back(p[i] + da); q.push_back(len); }
        q.push_back(0); q.push_back(5000); q.push_back(4999); q.push_back(1);
        bad |= fab_check("queries on, before and behind every point", f, { 1u, 2u, 3u, 5u, 6u }, q, true);
    }
    if (g_emu_errors) bad = 1;
    printf(bad ? "COVX EMU CHECK FAILED\n" : "COVX EMU CHECK OK\n");
    return bad;
}
#endif
