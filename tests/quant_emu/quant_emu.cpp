/*
 * quant_emu.cpp -- the quantile selection body (cbc_amd/csrc/cbc_quant_body.h) on the CPU through the lock-step wave emulation.
 * TEST AID ONLY: the body is run behind the emulated span decoder, the mark pass and the tile / compact passes over the
 * difference array (the order of cbc_gpu_decode_coverage_quant), or straight on change points the test fabricates.  The front
 * of the call and the scans between the passes are those of tests/emu/post_emu.h.  The wavefront's LDS table is a plain array
 * of exactly CBC_QUANT_LDS words that the emulation checks every zero / add / read against (tests/emu/wave_emu_post.h), and
 * every other table the body touches is an allocation of its exact size, so an index past it is an ASan finding.  With
 * -DQUANT_EMU_MAIN the file is a stand-alone program that builds fabricated cases itself, compares them with a sort on the host
 * and exits non-zero on a mismatch (make asan_check).
 */
#include <algorithm>
#include <utility>
#include "../emu/post_emu.h"
#include "../../cbc_amd/csrc/cbc_quant_body.h"

/* the span-reporting decoder over every block of the batch */
extern "C" __attribute__((visibility("default")))
int emu_quant_decode(const cbc_dec_device_batch *b, uint32_t smax) { WP::wg_table(nullptr, 0u); return emu_decode_blocks<WP, true>(b, smax); }

/* the selection over the first ncp change points: one emulated wavefront per query, each with a fresh table of garbage */
static void quant_pass(const uint32_t *cp_pos, const uint32_t *cp_dep, uint32_t ncp, uint32_t cp_cap, uint32_t slots, const uint32_t *pct,
                       uint32_t n_quant, const uint32_t *q, uint32_t n_q, uint32_t *quant)
{
    std::vector<uint32_t> pos(cp_pos, cp_pos + ncp), dep(cp_dep, cp_dep + ncp), qq(q, q + 2u * (size_t)n_q);
    std::vector<uint32_t> out((size_t)n_q * n_quant, 0xEEEEEEEEu);
    const uint64_t cnt_off[1] = { ncp };                            /* n_tiles = 0: [n_tiles] is the count */
    cbc_quant_args A;
    memset(&A, 0, sizeof A);
    A.cp_pos = pos.data(); A.cp_dep = dep.data(); A.cnt_off = cnt_off; A.n_tiles = 0u;
    A.q = qq.data(); A.quant = out.data();
    for (uint32_t t = 0; t < n_quant; t++) A.pct[t] = pct[t];
    A.n_quant = n_quant; A.cp_cap = cp_cap; A.n_q = n_q; A.slots = slots;
    for (uint32_t i = 0; i < n_q; i++) {
        std::vector<uint32_t> lds(CBC_QUANT_LDS, 0xdeadbeefu);
        WP::wg_table(lds.data(), CBC_QUANT_LDS);
        cbc_quant_select<WP>(A, i, lds.data());
        WP::wg_table(nullptr, 0u);
    }
    for (size_t i = 0; i < out.size(); i++) { if (out[i] == 0xEEEEEEEEu) emu_oob("a quantile was not written"); quant[i] = out[i]; }
}

/* fabricated change points straight into the body (cp_cap = ncp) */
extern "C" __attribute__((visibility("default")))
int emu_quant_points(const uint32_t *cp_pos, const uint32_t *cp_dep, uint32_t ncp, uint32_t slots, const uint32_t *pct, uint32_t n_quant,
                     const uint32_t *q, uint32_t n_q, uint32_t *quant)
{
    g_emu_errors = 0;
    if (n_quant < 1u || n_quant > CBC_QUANT_MAX) return CBC_E_ARG;
    for (uint32_t t = 0; t < n_quant; t++) if (pct[t] > 100u || (t && pct[t] <= pct[t - 1])) return CBC_E_ARG;
    for (uint32_t i = 0; i < n_q; i++) if (q[2 * i] > slots || q[2 * i + 1] > slots - q[2 * i]) return CBC_E_ARG;
    quant_pass(cp_pos, cp_dep, ncp, ncp, slots, pct, n_quant, q, n_q, quant);
    return g_emu_errors ? -100 : 0;
}

/* ONE contig's call (iv: its n_iv merged intervals; block_iv relative to them), every pass in the order of
 * cbc_gpu_decode_coverage_quant up to the change points, then the selection.  out[0] = reads kept, out[1] = change points,
 * out[2] = slots.  CBC_E_BLOCK when a block of the call failed to decode (it marked nothing; the numbers are those of the other
 * blocks -- the device call zeroes them on the host). */
extern "C" __attribute__((visibility("default")))
int emu_quant(const cbc_read_rec *recs, uint64_t n_recs, const uint8_t *seq, uint64_t seq_bytes, const cbc_dec_block_desc *blocks,
              const uint64_t *window_start, const cbc_block_result *dec_results, uint32_t n_blocks, const uint32_t *iv, uint32_t n_iv,
              const uint32_t *block_iv, uint32_t exclude, const uint32_t *q, uint32_t n_q, const uint32_t *pct, uint32_t n_quant,
              uint32_t *quant, uint64_t *out)
{
    g_emu_errors = 0;
    out[0] = out[1] = out[2] = 0;
    if (n_quant < 1u || n_quant > CBC_QUANT_MAX) return CBC_E_ARG;
    for (uint64_t i = 0; i < (uint64_t)n_q * n_quant; i++) quant[i] = 0;
    for (uint32_t t = 0; t < n_quant; t++) if (pct[t] > 100u || (t && pct[t] <= pct[t - 1])) return CBC_E_ARG;
    if (n_recs > 0x3fffffffull || n_iv == 0) return CBC_E_ARG;
    emu_depth_front F;
    if (F.intervals(iv, n_iv, block_iv, n_blocks)) return CBC_E_ARG;
    const uint64_t d_words = F.d_words;
    for (uint32_t i = 0; i < n_q; i++) if (q[2 * i] > d_words || q[2 * i + 1] > d_words - q[2 * i]) return CBC_E_ARG;
    const uint32_t cp_cap = (uint32_t)(2u * n_recs + 2u * (uint64_t)n_iv);
    F.tables(recs, n_recs, seq, seq_bytes, blocks, window_start, dec_results, n_blocks, exclude, cp_cap);
    WP::wg_table(nullptr, 0u);
    F.mark();
    if (F.points()) return -100;
    const uint32_t ncp = F.ncp;
    quant_pass(F.cp_pos.data(), F.cp_dep.data(), ncp, cp_cap, (uint32_t)d_words, pct, n_quant, q, n_q, quant);
    out[0] = F.ctr[0]; out[1] = ncp; out[2] = d_words;
    if (g_emu_errors) return -100;
    for (uint32_t b = 0; b < n_blocks; b++) if (dec_results[b].status != CBC_ST_OK) return CBC_E_BLOCK;
    return 0;
}

#ifdef QUANT_EMU_MAIN
/* ---- the stand-alone check: fabricated change points against a sort of (depth, length) pairs on the host ------------------------ */
struct fab { std::vector<uint32_t> pos, dep; uint64_t slots; };

static int fab_check(const char *what, const fab &f, const std::vector<uint32_t> &pct, const std::vector<uint32_t> &q)
{
    const uint32_t n_q = (uint32_t)(q.size() / 2), T = (uint32_t)pct.size();
    std::vector<uint32_t> got((size_t)n_q * T);                     /* exactly as long as the call writes */
    const int rc = emu_quant_points(f.pos.data(), f.dep.data(), (uint32_t)f.pos.size(), (uint32_t)f.slots, pct.data(), T, q.data(), n_q, got.data());
    int bad = rc != 0;
    for (uint32_t i = 0; i < n_q && !bad; i++) {
        const uint64_t a = q[2 * i], b = a + q[2 * i + 1], len = b - a;
        std::vector<std::pair<uint32_t, uint64_t> > runs;
        uint64_t nz = 0;
        for (size_t j = 0; j + 1 < f.pos.size(); j++) {
            const uint64_t lo = f.pos[j] > a ? f.pos[j] : a, hi = f.pos[j + 1] < b ? f.pos[j + 1] : b;
            if (hi > lo && f.dep[j]) { runs.push_back(std::make_pair(f.dep[j], hi - lo)); nz += hi - lo; }
        }
        runs.push_back(std::make_pair(0u, len - nz));
        std::sort(runs.begin(), runs.end());
        for (uint32_t t = 0; t < T; t++) {
            uint64_t k = ((uint64_t)pct[t] * len + 99u) / 100u, cum = 0;
            uint32_t want = 0;
            if (k < 1) k = 1;
            for (size_t j = 0; len && j < runs.size(); j++) { cum += runs[j].second; if (cum >= k) { want = runs[j].first; break; } }
            if (got[(size_t)i * T + t] != want) { bad = 1; fprintf(stderr, "%s: query %u (%llu, %llu) p %u: %u, want %u\n", what, i, (unsigned long long)a, (unsigned long long)len, pct[t], got[(size_t)i * T + t], want); }
        }
    }
    printf("%-60s %s (rc %d, %u queries, %u quantiles)\n", what, bad ? "MISMATCH" : "ok", rc, n_q, T);
    return bad;
}

static uint32_t rnd(uint64_t &s) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }

int main()
{
    int bad = 0;
    uint64_t seed = 7;
    const std::vector<uint32_t> p8 = { 0u, 1u, 25u, 50u, 75u, 90u, 99u, 100u }, p5 = { 0u, 1u, 50u, 99u, 100u };
    {   /* runs near 10^6 slots x 2500 (more than two tiles of runs), depths near 4 * 10^9: p * len passes 2^32, sums pass 2^31 */
        fab f; uint64_t at = 17;
        for (uint32_t i = 0; i < 2500u; i++) {
            f.pos.push_back((uint32_t)at);
            f.dep.push_back(i == 2499u ? 0u : i == 800u ? 1u : i == 1200u ? 0u : i == 1300u ? 0xffffffffu : 3900000000u + rnd(seed) % 300000000u);
            at += 900000u + rnd(seed) % 200000u;
        }
        f.slots = f.pos.back() + 5u;
        std::vector<uint32_t> q;
        const uint32_t fixed[][2] = { { 0u, (uint32_t)f.slots }, { 0u, f.pos[0] }, { f.pos[0], 1u }, { f.pos[2499], 5u }, { f.pos[2499] - 1u, 6u },
                                      { (uint32_t)f.slots, 0u }, { f.pos[5], 0u }, { f.pos[1023], f.pos[1024] - f.pos[1023] },
                                      { f.pos[1024], f.pos[1025] - f.pos[1024] }, { f.pos[2047] + 3u, f.pos[2049] - f.pos[2047] },
                                      { f.pos[1300], 10u }, { f.pos[1300] - 4u, 9u }, { f.pos[800] - 1u, 3u },
                                      { f.pos[100], f.pos[163] - f.pos[100] }, { f.pos[100], f.pos[164] - f.pos[100] }, { f.pos[100], f.pos[165] - f.pos[100] },
                                      { f.pos[100] + 7u, f.pos[164] - f.pos[100] } };
        for (size_t i = 0; i < sizeof fixed / sizeof fixed[0]; i++) { q.push_back(fixed[i][0]); q.push_back(fixed[i][1]); }
        for (int i = 0; i < 60; i++) { const uint32_t a = rnd(seed) % (uint32_t)f.slots; q.push_back(a); q.push_back(rnd(seed) % ((uint32_t)f.slots - a + 1u)); }
        bad |= fab_check("10^6-slot runs x 2500, depths near 4 * 10^9, 8 quantiles", f, p8, q);
        bad |= fab_check("the same, the median alone", f, { 50u }, q);
    }
    for (uint32_t ncp = 0; ncp <= 2; ncp++) {   /* no run at all, a lone change point, one run */
        fab f; f.slots = 100;
        if (ncp == 2) { f.pos.push_back(9); f.dep.push_back(6); }
        if (ncp >= 1) { f.pos.push_back(49); f.dep.push_back(0); }
        char what[64];
        snprintf(what, sizeof what, "ncp %u", ncp);
        bad |= fab_check(what, f, p5, { 0u, 100u, 9u, 1u, 8u, 1u, 48u, 1u, 49u, 1u, 5u, 0u, 100u, 0u, 0u, 9u, 0u, 10u, 9u, 40u, 8u, 42u, 20u, 5u });
    }
    {   /* small depths around the table's edge: CBC_QUANT_LDS - 1, CBC_QUANT_LDS, CBC_QUANT_LDS + 1 in 63, 64, 65 and 300 runs */
        const uint32_t counts[] = { 63u, 64u, 65u, 300u, 1100u, 2100u };
        for (size_t c = 0; c < sizeof counts / sizeof counts[0]; c++) {
            fab f; uint32_t at = 10;
            for (uint32_t i = 0; i < counts[c]; i++) {
                f.pos.push_back(at);
                const uint32_t r = rnd(seed) % 8u;
                f.dep.push_back(r == 0u ? 0u : r == 1u ? CBC_QUANT_LDS - 1u : r == 2u ? CBC_QUANT_LDS : r == 3u ? CBC_QUANT_LDS + 1u : r == 4u ? 5u : 1u + rnd(seed) % 3000u);
                at += 1u + rnd(seed) % 9u;
            }
            f.pos.push_back(at); f.dep.push_back(0u);
            f.slots = at + 20u;
            std::vector<uint32_t> q = { 0u, (uint32_t)f.slots, 10u, at - 10u, 11u, at - 12u, 0u, 10u, at, 20u, at - 1u, 1u };
            for (int i = 0; i < 40; i++) { const uint32_t a = rnd(seed) % (uint32_t)f.slots; q.push_back(a); q.push_back(rnd(seed) % ((uint32_t)f.slots - a + 1u)); }
            char what[64];
            snprintf(what, sizeof what, "%u runs around the table's edge", counts[c]);
            bad |= fab_check(what, f, p8, q);
        }
    }
    if (g_emu_errors) bad = 1;
    printf(bad ? "QUANT EMU CHECK FAILED\n" : "QUANT EMU CHECK OK\n");
    return bad;
}
#endif
