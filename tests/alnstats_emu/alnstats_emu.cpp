/*
 * alnstats_emu.cpp -- the statistics call with alignment tables (cbc_gpu_decode_stats_aln) on the CPU through the lock-step wave
 * emulation: the edit-reporting decoder (cbc_decode_body.h, EDITS = true), then the three bodies of cbc_stats_body.h and the three
 * of cbc_stats_aln_body.h, a workgroup phase by phase -- every wavefront zeroes, then every wavefront accumulates, then every
 * wavefront flushes: the two barriers of the kernels.  TEST AID ONLY.  Every buffer is an allocation of exactly its size and named
 * to the emulation -- the workgroup's table (CBC_SALN_LDS words), the global table (CBC_SALN_WORDS), the side array, the arena --
 * so an index past one is a finding.  With -DALNSTATS_EMU_MAIN the file is a stand-alone program that builds fabricated cases
 * itself, compares them with an element-by-element host loop and exits non-zero on a mismatch (make asan_check).
 */
#include "../emu/post_emu.h"
#include "../../cbc_amd/csrc/cbc_stats_aln_body.h"

/* the edit-reporting decoder over every block of the batch: side = 2 * n_recs words, arena = n_recs * per_read entries exactly */
extern "C" __attribute__((visibility("default")))
int emu_aln_decode(const cbc_dec_device_batch *b, uint32_t smax, uint32_t per_read, uint32_t *side, uint16_t *arena)
{ return emu_decode_blocks<WP, true, true>(b, smax, per_read, side, arena); }

extern "C" __attribute__((visibility("default")))
uint32_t emu_aln_words(uint32_t what) { return what == 0u ? CBC_SALN_WORDS : what == 1u ? CBC_SALN_LDS : what == 2u ? CBC_SALN_T_LO : CBC_SALN_T_HI; }

/* ONE call: iv == NULL the whole-file form, else the target form.  grid = 0: the device's grid; n_waves wavefronts share a
 * workgroup's tables.  preload (CBC_SALN_WORDS words or NULL): what the global alignment table holds before the first workgroup
 * flushes, instead of zeros.  CBC_E_BLOCK with all-zero tables when a block of the call failed. */
extern "C" __attribute__((visibility("default")))
int emu_stats_aln(const cbc_read_rec *recs, uint64_t n_recs, const uint8_t *seq, uint64_t seq_bytes, const cbc_dec_block_desc *blocks,
                  const uint64_t *window_start, const cbc_block_result *dec_results, uint32_t n_blocks, const uint32_t *iv, uint32_t n_iv,
                  const uint32_t *block_iv, uint32_t exclude, const uint32_t *side, const uint16_t *arena, uint32_t per_read,
                  const uint8_t *ref, uint64_t ref_bytes, uint32_t grid, uint32_t n_waves, const uint32_t *preload,
                  cbc_gpu_stats *out, cbc_gpu_stats_aln *aln)
{
    g_emu_errors = 0;
    memset(out, 0, sizeof *out); memset(aln, 0, sizeof *aln);
    if (n_waves < 1u || n_waves > 16u || n_recs > 0xffffffffull) return CBC_E_ARG;
    uint32_t most = 0;
    for (uint32_t b = 0; b < n_blocks; b++) if (blocks[b].n_reads > most) most = blocks[b].n_reads;
    if ((uint64_t)n_blocks * ((most + 63u) / 64u) > CBC_SALN_MAX_UNITS) return CBC_E_ARG;
    std::vector<uint32_t> tab(CBC_STATS_WORDS, 0u), atab(CBC_SALN_WORDS, 0u);      /* exactly the device's tables */
    if (preload) memcpy(atab.data(), preload, (size_t)CBC_SALN_WORDS * 4u);
    cbc_stats_aln_args A;
    memset(&A, 0, sizeof A);
    cbc_stats_args &S = A.S;
    S.R.recs = recs; S.R.seq = seq; S.R.blocks = blocks; S.R.window_start = window_start; S.R.dec_results = dec_results;
    S.R.n_recs = n_recs; S.R.seq_bytes = seq_bytes; S.R.beg = 1u; S.R.end = UINT64_MAX; S.R.n_blocks = n_blocks;
    S.iv = iv; S.block_iv = block_iv; S.n_iv = n_iv; S.tab = tab.data(); S.exclude = exclude; S.gmax = (most + 63u) / 64u;
    const uint64_t units = (uint64_t)n_blocks * S.gmax, wgs = (units + n_waves - 1u) / n_waves;
    S.grid = grid ? grid : (wgs < CBC_STATS_GRID ? (uint32_t)wgs : CBC_STATS_GRID);
    A.side = side; A.arena = arena; A.ref = ref; A.tab = atab.data();
    A.arena_entries = n_recs * per_read; A.ref_bytes = ref_bytes; A.per_read = per_read;
    WP::clear_ranges();
    WP::add_range(tab.data(), CBC_STATS_WORDS); WP::add_uni_range(tab.data(), CBC_STATS_WORDS);
    WP::add_range(atab.data(), CBC_SALN_WORDS); WP::add_uni_range(atab.data(), CBC_SALN_WORDS);
    WP::edit_arena(arena, A.arena_entries);
    for (uint32_t wg = 0; wg < S.grid; wg++) {                       /* the statistics kernel */
        std::vector<uint32_t> lds(CBC_STATS_LDS, 0xdeadbeefu);
        WP::wg_table(lds.data(), CBC_STATS_LDS);
        for (uint32_t w = 0; w < n_waves; w++) cbc_stats_zero<WP>(lds.data(), w, n_waves);
        for (uint32_t w = 0; w < n_waves; w++) {
            if (iv) cbc_stats_accum<WP, true>(S, wg, w, n_waves, lds.data());
            else cbc_stats_accum<WP, false>(S, wg, w, n_waves, lds.data());
        }
        for (uint32_t w = 0; w < n_waves; w++) cbc_stats_flush<WP>(S, lds.data(), w, n_waves);
        WP::wg_table(nullptr, 0u);
    }
    for (uint32_t wg = 0; wg < S.grid; wg++) {                       /* the alignment kernel */
        std::vector<uint32_t> lds(CBC_SALN_LDS, 0xdeadbeefu);        /* one table per workgroup, exactly CBC_SALN_LDS words */
        WP::wg_table(lds.data(), CBC_SALN_LDS);
        for (uint32_t w = 0; w < n_waves; w++) cbc_stats_aln_zero<WP>(lds.data(), w, n_waves);
        for (uint32_t w = 0; w < n_waves; w++) {
            if (iv) cbc_stats_aln_accum<WP, true>(A, wg, w, n_waves, lds.data());
            else cbc_stats_aln_accum<WP, false>(A, wg, w, n_waves, lds.data());
        }
        for (uint32_t w = 0; w < n_waves; w++) cbc_stats_aln_flush<WP>(A, lds.data(), w, n_waves);
        WP::wg_table(nullptr, 0u);
    }
    WP::clear_ranges();
    WP::edit_arena(nullptr, 0);
    if (tab[CBC_STATS_T_CTR + 1u] || atab[CBC_SALN_T_CTR + 1u] != (preload ? preload[CBC_SALN_T_CTR + 1u] : 0u)) emu_oob("a spare counter was written");
    if (g_emu_errors) return -100;
    for (uint32_t b = 0; b < n_blocks; b++) if (dec_results[b].status != CBC_ST_OK) return CBC_E_BLOCK;   /* all zero */
    cbc_stats_finish(tab.data(), out);
    cbc_stats_aln_finish(atab.data(), aln);
    return 0;
}

#ifdef ALNSTATS_EMU_MAIN
#include "../emu/fab_reads.h"
/* ---- the stand-alone check: fabricated records, rows and arena entries against an element-by-element host loop --------------- */
/* the semantics of include/cbc_gpu.h, one element at a time, into *a; false: not a valid record */
static bool host_count(const fab &f, const fread_ &r, cbc_gpu_stats_aln *a)
{
    const uint32_t rl = (uint32_t)r.seq.size(), nd = (uint32_t)r.dc.size(), ni = (uint32_t)r.oi.size();
    if (r.raw_cnt >= 0 || r.raw_e0 >= 0) return false;
    if (rl == 0u || nd > 255u || ni > 255u || ni > rl) return false;
    const uint32_t T = rl - ni;
    for (uint32_t i = 0; i < nd; i++) if (r.dc[i] > T || (i && r.dc[i] < r.dc[i - 1u])) return false;
    for (uint32_t i = 0; i < ni; i++) if (r.oi[i] >= rl || (i && r.oi[i] <= r.oi[i - 1u])) return false;
    if (r.pos < 1u || (uint64_t)r.pos - 1u + T + nd > f.ref.size()) return false;
    std::vector<bool> isins(rl, false);
    for (uint32_t o : r.oi) isins[o] = true;
    struct el { char k; uint32_t q, x; };
    std::vector<el> E;
    uint32_t q = 0, di = 0, x = 0;
    for (uint32_t m = 0; m <= T; m++) {
        while (q < rl && isins[q]) { E.push_back(el{ 'I', q, 0u }); q++; }
        while (di < nd && r.dc[di] == m) { E.push_back(el{ 'D', 0u, x++ }); di++; }
        if (m < T) { E.push_back(el{ 'M', q, x++ }); q++; }
    }
    if (q != rl || di != nd) return false;
    const bool rev = (r.flag & 16u) != 0u;
    uint32_t nm = 0, seen = 0;
    a->len[rl]++; a->reads++;
    for (size_t i = 0; i < E.size();) {
        size_t j = i;
        while (j < E.size() && E[j].k == E[i].k) j++;
        const uint32_t L = (uint32_t)(j - i);
        if (E[i].k == 'I') {
            uint32_t after = 0;
            for (size_t k = j; k < E.size(); k++) after += E[k].k == 'M';
            for (size_t k = i; k < j; k++) a->unal[rev ? rl - E[k].q : E[k].q + 1u]++;
            if (seen != 0u && after != 0u) { a->ins_len[L]++; a->ins_cyc[rev ? rl - E[j - 1].q : E[i].q + 1u]++; nm += L; }
        } else if (E[i].k == 'D') {
            const uint32_t k = j < E.size() ? E[j].q : rl;          /* behind a deleted run: an aligned base, or the end */
            a->del_len[L]++; a->del_cyc[rev ? rl - k : k]++; nm += L;
        } else
            for (size_t k = i; k < j; k++) {
                seen++;
                if ((uint8_t)r.seq[E[k].q] != f.ref[r.pos - 1u + E[k].x]) { a->mm[rev ? rl - E[k].q : E[k].q + 1u]++; nm++; }
            }
        i = j;
    }
    a->nm[nm]++;
    return true;
}

static bool same_aln(const cbc_gpu_stats_aln &a, const cbc_gpu_stats_aln &b, const char **which)
{
#define CMP(m) if (memcmp(a.m, b.m, sizeof a.m) != 0) { *which = #m; return false; }
    CMP(len) CMP(mm) CMP(unal) CMP(ins_cyc) CMP(del_cyc) CMP(nm) CMP(ins_len) CMP(del_len)
#undef CMP
    if (a.reads != b.reads) { *which = "reads"; return false; }
    if (a.invalid != b.invalid) { *which = "invalid"; return false; }
    return true;
}

/* pre_lo / pre_hi: what the two planes of the global table hold for ins_len[1] before the first flush (0, 0: nothing preloaded) */
static int fab_check(const char *what, fab &f, uint32_t exclude, uint32_t grid, uint32_t n_waves, const vu *iv = NULL, int fail_block = -1,
                     uint32_t pre_lo = 0u, uint32_t pre_hi = 0u)
{
    const size_t nb = f.block_n.size();
    fab_arrays a;
    if (!fab_build(f, a, fail_block, 2u)) { printf("%-66s BAD FIXTURE\n", what); return 1; }
    vu biv;
    for (size_t b = 0; b < nb; b++) { biv.push_back(0u); biv.push_back(iv ? (uint32_t)(iv->size() / 2u) : 0u); }
    std::vector<cbc_gpu_stats_aln> want(1), got(1);
    std::vector<cbc_gpu_stats> out(1);
    memset(&want[0], 0, sizeof want[0]);
    uint64_t counted = 0, excluded = 0;
    for (size_t at = 0; at < f.reads.size(); at++) {
        const fread_ &r = f.reads[at];
        for (uint32_t i = r.len; i < f.stride; i++) a.rows[at * f.stride + i] = (uint8_t)"GCN"[i % 3u];   /* behind the bases: never zero */
        if (iv) {
            bool hit = false;
            for (size_t q = 0; q + 1u < iv->size() && !hit; q += 2u) hit = r.pos <= (*iv)[q + 1u] && r.pos + r.span - 1u >= (*iv)[q];
            if (!hit) continue;
        }
        if (r.flag & exclude) { excluded++; continue; }
        counted++;
        const bool ok = host_count(f, r, &want[0]);
        if (!ok) want[0].invalid++;
        if (r.want_valid >= 0 && (r.want_valid != 0) != ok) { printf("%-66s BAD FIXTURE: read %zu validity\n", what, at); return 1; }
    }
    std::vector<uint32_t> pre;
    if (pre_lo | pre_hi) {
        pre.assign(emu_aln_words(0u), 0u);
        pre[emu_aln_words(2u) + 1u] = pre_lo; pre[emu_aln_words(3u) + 1u] = pre_hi;
        want[0].ins_len[1] += (uint64_t)pre_lo + ((uint64_t)pre_hi << 16);
    }
    const int rc = emu_stats_aln(a.recs.data(), f.reads.size(), a.rows.data(), a.rows.size(), a.blocks.data(), a.ws.data(), a.res.data(), (uint32_t)nb,
                                 iv ? iv->data() : NULL, iv ? (uint32_t)(iv->size() / 2u) : 0u, biv.data(), exclude, a.side.data(), a.arena.data(),
                                 f.per_read, f.ref.data(), f.ref.size(), grid, n_waves, pre.empty() ? NULL : pre.data(), &out[0], &got[0]);
    const char *which = "";
    int bad;
    if (fail_block >= 0) {
        std::vector<cbc_gpu_stats_aln> zero(1);
        memset(&zero[0], 0, sizeof zero[0]);
        bad = rc != CBC_E_BLOCK || !same_aln(got[0], zero[0], &which) || out[0].reads != 0u;
    } else
        bad = rc != 0 || !same_aln(got[0], want[0], &which) || out[0].reads != counted || out[0].excluded != excluded ||
              got[0].reads + got[0].invalid != counted;
    printf("%-66s %s%s (rc %d, %llu reads, %llu without alignment, ins_len[1] %llu)\n", what, bad ? "MISMATCH " : "ok", bad ? which : "", rc,
           (unsigned long long)got[0].reads, (unsigned long long)got[0].invalid, (unsigned long long)got[0].ins_len[1]);
    return bad;
}

int main()
{
    int bad = 0;
    static const uint32_t lens[] = { 1, 2, 3, 4, 5, 6, 7, 8, 63, 64, 65, 150, 251, 252, 253, 254, 255, 256 };
    const size_t n_lens = sizeof lens / sizeof lens[0];
    std::vector<uint8_t> ref;
    for (uint32_t i = 0; i < 9000u; i++) ref.push_back("ACGTNacgtnRYk"[rnd() % 13u]);         /* lower-case and IUPAC reference bytes */
    for (uint32_t stride = 256u; stride >= 4u; stride = stride == 256u ? 152u : stride == 152u ? 8u : stride == 8u ? 4u : 0u) {
        /* reads without indels: every length the stride holds on both strands; perfect, a mismatch at the first base, at the last,
         * in the dword that straddles the read's end, at all three; at reference offset 0 and ending on the last uploaded byte
         * (valid), one byte further (not valid, and not read) */
        fab f; f.stride = stride; f.per_read = 1u; f.on_ref = true; f.ref = ref;
        uint32_t pos = 1u;
        for (size_t i = 0; i < n_lens; i++) {
            const uint32_t L = lens[i];
            if (L > stride) continue;
            const uint32_t st = (L - 1u) - (L - 1u) % 4u;
            for (uint32_t fl = 0; fl <= 16u; fl += 16u) {
                fab_read(f, pos, fl, L, vu(), vu()).want_valid = 1;
                fab_read(f, pos += 2u, fl, L, vu(), vu(), vu{ 0u });
                fab_read(f, pos += 1u, fl | 1024u, L, vu(), vu(), vu{ L - 1u });
                fab_read(f, pos += 3u, fl, L, vu(), vu(), vu{ st });
                fab_read(f, pos += 1u, fl, L, vu(), vu(), vu{ 0u, st, L - 1u, L / 2u });
                fab_read(f, (uint32_t)ref.size() - L + 1u, fl, L, vu(), vu(), vu{ L - 1u }).want_valid = 1;
                fab_read(f, (uint32_t)ref.size() - L + 2u, fl, L, vu(), vu()).want_valid = 0;
            }
        }
        fab_read(f, (uint32_t)ref.size() + 1u, 0u, 1u, vu(), vu()).want_valid = 0;       /* POS - 1 = the upload's size */
        fab_read(f, (uint32_t)ref.size() + 9u, 0u, 1u, vu(), vu()).want_valid = 0;
        fab_read(f, 7u, 0u, 0u, vu(), vu()).want_valid = 0;                              /* rl = 0 */
        while (f.reads.size() < 1u + 63u + 64u + 65u + 70u) fab_read(f, pos += 1u, (rnd() & 1u) * 16u, stride - rnd() % 3u, vu(), vu(), vu{ rnd() % stride });
        uint32_t at = 0;
        static const uint32_t sizes[] = { 0, 1, 63, 64, 65 };
        for (int i = 0; i < 5; i++) { f.block_n.push_back(sizes[i]); at += sizes[i]; }
        f.block_n.push_back((uint32_t)f.reads.size() - at);
        char what[96];
        snprintf(what, sizeof what, "stride %u, no indels, the device's grid", stride);
        bad |= fab_check(what, f, 0u, 0u, 4u);
        snprintf(what, sizeof what, "stride %u, no indels, grid 1, one wavefront", stride);
        bad |= fab_check(what, f, 0u, 1u, 1u);
        snprintf(what, sizeof what, "stride %u, no indels, grid 2 of 3 wavefronts, exclude 16", stride);
        bad |= fab_check(what, f, 16u, 2u, 3u);
        snprintf(what, sizeof what, "stride %u, no indels, grid 2 of 2 wavefronts, exclude 0x400", stride);
        bad |= fab_check(what, f, 0x400u, 2u, 2u);
        vu iv{ 1u, 40u, 100u, 100u, pos - 20u, pos + 500u };
        snprintf(what, sizeof what, "stride %u, no indels, three intervals", stride);
        bad |= fab_check(what, f, 0u, 0u, 4u, &iv);
    }
    {   /* reads with indels, stride 256 */
        fab f; f.stride = 256u; f.per_read = 24u; f.on_ref = true; f.ref = ref;
        static const uint32_t ilens[] = { 1, 63, 64, 65, 127, 128, 129, 150, 256 };
        uint32_t pos = 5;
        for (size_t i = 0; i < sizeof ilens / sizeof ilens[0]; i++) {
            const uint32_t L = ilens[i];
            for (uint32_t fl = 0; fl <= 16u; fl += 16u) {
                fab_read(f, pos += 7u, fl, L, vu{ 0u }, vu());                        /* a deletion before the first base: cycle 0 or rl */
                fab_read(f, pos += 1u, fl, L, vu{ L }, vu());                         /* one after the last, at matched coordinate T */
                fab_read(f, pos += 1u, fl, L, vu{ 0u, 0u, L, L, L }, vu(), vu{ 0u, L - 1u });
                fab_read(f, pos += 1u, fl, L, vu{ L / 2u, L / 2u }, vu());
                fab_read(f, pos += 1u, fl, L, vu(), vu{ 0u });                        /* an insertion run at read index 0: S */
                fab_read(f, pos += 1u, fl, L, vu(), vu{ L - 1u });                    /* and one at rl - 1: S */
                vu all; for (uint32_t q = 0; q < L; q++) all.push_back(q);
                if (L <= 129u) {
                    fab_read(f, pos += 1u, fl, L, vu{ 0u, 0u }, all);                 /* nothing but insertions over two deleted bases */
                    fab_read(f, pos += 1u, fl, L, vu(), all).want_valid = 1;
                }
                if (L < 65u) continue;
                fab_read(f, pos += 1u, fl, L, vu{ 64u }, vu());                       /* a deletion at coordinate 64 */
                fab_read(f, pos += 1u, fl, L, vu{ 2u, 2u }, vu(), vu{ 2u });          /* a mismatch directly behind a deletion */
                fab_read(f, pos += 1u, fl, L, vu{ 5u, 6u }, vu(), vu{ 5u });          /* two D runs around one aligned base */
                fab_read(f, pos += 1u, fl, L, vu(), vu{ 0u, 1u, L - 2u, L - 1u });    /* both clips in one read */
                fab_read(f, pos += 1u, fl, L, vu(), vu{ 30u, 31u, 32u }, vu{ 29u, 33u });
                fab_read(f, pos += 1u, fl, L, vu{ 40u, 40u }, vu{ 40u, 41u, 42u });   /* an I run touching a D run */
                fab_read(f, pos += 1u, fl, L, vu{ 1u, 3u, 3u }, vu{ 0u, 1u, 62u, 63u, 64u, L - 2u, L - 1u }, vu{ 5u, 70u });
                fab_read(f, pos += 1u, fl, L, vu(), vu{ 62u, 63u, 64u, 65u });        /* an I run across the turn */
            }
        }
        /* not valid: every kind of DESIGN.md section 4.21 */
        fab_read(f, pos += 1u, 0u, 50u, vu(), vu()).raw_cnt = 256;                     /* nDel above 255 */
        fab_read(f, pos += 1u, 0u, 50u, vu(), vu()).raw_cnt = 256 << 16;               /* nIns above 255 */
        { fread_ &r = fab_read(f, pos += 1u, 0u, 50u, vu(), vu()); r.raw_cnt = 2; r.raw_e0 = 1 << 20; }      /* entries outside the block's arena */
        { fread_ &r = fab_read(f, pos += 1u, 0u, 50u, vu(), vu()); r.raw_cnt = 0; r.raw_e0 = 1 << 20; }      /* the same with empty lists */
        fab_read(f, pos += 1u, 0u, 50u, vu{ 5u, 3u }, vu()).want_valid = 0;            /* dc descending */
        fab_read(f, pos += 1u, 0u, 50u, vu{ 51u }, vu()).want_valid = 0;               /* dc above T */
        fab_read(f, pos += 1u, 0u, 50u, vu(), vu{ 3u, 3u }).want_valid = 0;            /* oi not strictly ascending */
        fab_read(f, pos += 1u, 0u, 50u, vu(), vu{ 50u }).want_valid = 0;               /* oi >= rl */
        fab_read(f, pos += 1u, 0u, 0u, vu(), vu()).want_valid = 0;                     /* rl = 0 */
        fab_read(f, (uint32_t)ref.size() - 60u, 0u, 50u, vu(12u, 20u), vu()).want_valid = 0;      /* the deleted bases reach past the upload */
        fab_read(f, (uint32_t)ref.size() - 60u, 0u, 50u, vu(11u, 20u), vu()).want_valid = 1;      /* ... and end on its last byte */
        while (f.reads.size() % 64u != 1u || f.reads.size() < 400u)
            fab_read(f, pos += 3u, (rnd() & 1u) * 16u, 100u, rnd() % 3u ? vu() : vu{ 40u, 40u, 41u }, rnd() % 4u ? vu() : vu{ 10u, 11u, 50u }, rnd() % 2u ? vu() : vu{ rnd() % 100u, rnd() % 100u });
        {
            const uint32_t sizes[] = { 0, 1, 63, 64, 65 };
            uint32_t at = 0;
            for (int i = 0; i < 5; i++) { f.block_n.push_back(sizes[i]); at += sizes[i]; }
            f.block_n.push_back((uint32_t)f.reads.size() - at);
        }
        if (pos + 600u > f.ref.size()) { printf("BAD FIXTURE: the reference is too short\n"); return 1; }
        bad |= fab_check("indels, the device's grid", f, 0u, 0u, 4u);
        bad |= fab_check("indels, grid 1, one wavefront", f, 0u, 1u, 1u);
        bad |= fab_check("indels, grid 2 of 3 wavefronts, exclude 16", f, 16u, 2u, 3u);
        bad |= fab_check("indels, grid 1 of 2 wavefronts", f, 0u, 1u, 2u);
        bad |= fab_check("indels, a failed block", f, 0u, 0u, 4u, NULL, 3);
        for (size_t i = 0; i < f.reads.size(); i += 37u) {              /* windows cut through reads */
            const fread_ &r = f.reads[i];
            char what[96];
            snprintf(what, sizeof what, "indels, an interval inside read %zu", i);
            vu iv{ r.pos + 1u, r.pos + 2u };
            bad |= fab_check(what, f, 0u, 0u, 4u, &iv);
        }
    }
    {   /* long lists: nDel and nIns above 64, 127 one-base I runs, an arena of exactly the needed size */
        fab g; g.stride = 256u; g.per_read = 135u; g.on_ref = true; g.ref = ref;                   /* 70 + 70 + 245 + 88 + 127 + 210 = 6 * 135 entries */
        vu d70(70u, 100u), d200, i70, i40, i127, d210;
        for (uint32_t i = 0; i < 200u; i++) d200.push_back(10u + i / 2u);
        for (uint32_t i = 0; i < 70u; i++) i70.push_back(60u + i);
        for (uint32_t i = 0; i < 45u; i++) i40.push_back(3u * i + 5u);
        for (uint32_t i = 0; i < 127u; i++) i127.push_back(2u * i + 1u);
        for (uint32_t i = 0; i < 210u; i++) d210.push_back(i);                    /* 210 one-base D runs */
        fab_read(g, 10u, 0u, 200u, d70, vu(), vu{ 100u });
        fab_read(g, 20u, 16u, 250u, vu(), i70, vu{ 3u, 200u });
        fab_read(g, 30u, 0u, 256u, d200, i40, vu{ 0u, 255u });
        fab_read(g, 40u, 16u, 256u, vu(88u, 200u), vu(), vu());
        fab_read(g, 50u, 0u, 255u, vu(), i127, vu{ 0u, 254u }).want_valid = 1;
        fab_read(g, 60u, 16u, 256u, d210, vu(), vu()).want_valid = 1;
        g.block_n.push_back(6u);
        bad |= fab_check("long lists, an arena of exactly the needed size", g, 0u, 0u, 4u);
        bad |= fab_check("long lists, one wavefront", g, 0u, 1u, 1u);
        /* the global ins_len[1] at 0xFFFFFFF0 before the flush -- its halves as the flushes of earlier workgroups leave them --
         * and the 127 runs on top: exact in 64 bits */
        bad |= fab_check("long lists, ins_len[1] preloaded to 0xFFFFFFF0", g, 0u, 0u, 4u, NULL, -1, 0xFFF0u, 0xFFFFu);
        bad |= fab_check("long lists, ins_len[1] halves preloaded to 2^27 and 2^23", g, 0u, 2u, 2u, NULL, -1, 1u << 27, 1u << 23);
    }
    if (g_emu_errors) bad = 1;
    printf(bad ? "ALNSTATS EMU CHECK FAILED\n" : "ALNSTATS EMU CHECK OK\n");
    return bad;
}
#endif
