/*
 * stats_emu.cpp -- the read-statistics bodies (cbc_amd/csrc/cbc_stats_body.h) on the CPU through the lock-step wave emulation.
 * TEST AID ONLY: the zero, accumulate and flush bodies are run behind the emulated span decoder (the order of
 * cbc_gpu_decode_stats), or on records and rows the stand-alone program fabricates, under ASan-able host code before anything
 * runs on a GPU.  A workgroup is run phase by phase: every wavefront zeroes, then every wavefront accumulates, then every
 * wavefront flushes -- the two barriers of the kernel.  The workgroup's table is an allocation of exactly CBC_STATS_LDS words and
 * the global table one of exactly CBC_STATS_WORDS, both bounds-checked by the emulation as well, so an index past either is a
 * finding.  With -DSTATS_EMU_MAIN the file is a stand-alone program that builds the fabricated cases itself, compares them with
 * a byte-by-byte host loop and exits non-zero on a mismatch (make asan_check).
 */
#include "../emu/post_emu.h"
#include "../../cbc_amd/csrc/cbc_stats_body.h"

/* the span-reporting decoder over every block of the batch */
extern "C" __attribute__((visibility("default")))
int emu_stats_decode(const cbc_dec_device_batch *b, uint32_t smax) { return emu_decode_blocks<WP, true>(b, smax); }

extern "C" __attribute__((visibility("default")))
uint32_t emu_stats_lds_flags(void) { return CBC_STATS_FLAGS_LDS; }

/* ONE call: iv == NULL the whole-file form, else the target form (iv: n_iv pairs; block_iv per block).  grid = 0: the device's
 * grid; n_waves wavefronts share a workgroup's table.  CBC_E_BLOCK with all-zero tables when a block of the call failed. */
extern "C" __attribute__((visibility("default")))
int emu_stats(const cbc_read_rec *recs, uint64_t n_recs, const uint8_t *seq, uint64_t seq_bytes, const cbc_dec_block_desc *blocks,
              const uint64_t *window_start, const cbc_block_result *dec_results, uint32_t n_blocks, const uint32_t *iv, uint32_t n_iv,
              const uint32_t *block_iv, uint32_t exclude, uint32_t grid, uint32_t n_waves, cbc_gpu_stats *out)
{
    g_emu_errors = 0;
    memset(out, 0, sizeof *out);
    if (n_waves < 1u || n_waves > 16u || n_recs > 0xffffffffull) return CBC_E_ARG;
    uint32_t most = 0;
    for (uint32_t b = 0; b < n_blocks; b++) if (blocks[b].n_reads > most) most = blocks[b].n_reads;
    std::vector<uint32_t> tab(CBC_STATS_WORDS, 0u);                  /* exactly the device's table */
    cbc_stats_args A;
    memset(&A, 0, sizeof A);
    A.R.recs = recs; A.R.seq = seq; A.R.blocks = blocks; A.R.window_start = window_start; A.R.dec_results = dec_results;
    A.R.n_recs = n_recs; A.R.seq_bytes = seq_bytes; A.R.beg = 1u; A.R.end = UINT64_MAX; A.R.n_blocks = n_blocks;
    A.iv = iv; A.block_iv = block_iv; A.n_iv = n_iv; A.tab = tab.data(); A.exclude = exclude; A.gmax = (most + 63u) / 64u;
    const uint64_t units = (uint64_t)n_blocks * A.gmax, wgs = (units + n_waves - 1u) / n_waves;
    A.grid = grid ? grid : (wgs < CBC_STATS_GRID ? (uint32_t)wgs : CBC_STATS_GRID);
    WP::global_table(tab.data(), CBC_STATS_WORDS);
    for (uint32_t wg = 0; wg < A.grid; wg++) {
        std::vector<uint32_t> lds(CBC_STATS_LDS, 0xdeadbeefu);      /* one table per workgroup, exactly CBC_STATS_LDS words */
        WP::wg_table(lds.data(), CBC_STATS_LDS);
        for (uint32_t w = 0; w < n_waves; w++) cbc_stats_zero<WP>(lds.data(), w, n_waves);
        for (uint32_t w = 0; w < n_waves; w++) {
            if (iv) cbc_stats_accum<WP, true>(A, wg, w, n_waves, lds.data());
            else cbc_stats_accum<WP, false>(A, wg, w, n_waves, lds.data());
        }
        for (uint32_t w = 0; w < n_waves; w++) cbc_stats_flush<WP>(A, lds.data(), w, n_waves);
        WP::wg_table(nullptr, 0u);
    }
    WP::global_table(nullptr, 0u);
    if (tab[CBC_STATS_T_CTR + 1u]) emu_oob("the spare counter was written");
    if (g_emu_errors) return -100;
    for (uint32_t b = 0; b < n_blocks; b++) if (dec_results[b].status != CBC_ST_OK) return CBC_E_BLOCK;   /* all zero */
    cbc_stats_finish(tab.data(), out);
    return 0;
}

#ifdef STATS_EMU_MAIN
/* ---- the stand-alone check: fabricated records and rows against a byte-by-byte host loop ---------------------------------------- */
struct fab {
    uint32_t stride;
    std::vector<cbc_read_rec> recs;
    std::vector<uint8_t> rows;
    std::vector<cbc_dec_block_desc> blocks;
    std::vector<uint64_t> ws;
    std::vector<cbc_block_result> res;
    std::vector<uint32_t> pos, span;                                 /* absolute POS and span per read, for the target form */
};

static uint32_t g_rng = 12345u;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }

/* a read of `len` bases: the row's bytes past the length are 'G', 'C' and 'N' -- never zero */
static void fab_read(fab &f, uint32_t pos, uint32_t flag, uint32_t len, int kind)
{
    static const char sym[] = "ACGTNacgtRY";
    cbc_read_rec r;
    memset(&r, 0, sizeof r);
    uint32_t *w = (uint32_t *)&r;
    w[0] = pos; w[1] = flag | (len << 16); w[2] = 0u; w[3] = len;
    f.recs.push_back(r);
    f.pos.push_back(pos); f.span.push_back(len);
    for (uint32_t i = 0; i < f.stride; i++) {
        uint8_t c;
        if (i >= len) c = "GCN"[i % 3u];
        else if (kind == 1) c = 'G';
        else if (kind == 2) c = 'A';
        else if (kind == 3) c = (i == 0u || i + 1u == len || i == (len - 1u) - (len - 1u) % 4u) ? 'N' : sym[rnd() % 4u];
        else c = sym[rnd() % (kind == 4 ? 11u : 4u)];
        f.rows.push_back(c);
    }
}

static void fab_block(fab &f, uint32_t first, uint32_t n)
{
    cbc_dec_block_desc d;
    memset(&d, 0, sizeof d);
    d.rec_base = first; d.seq_base = (uint64_t)first * f.stride; d.n_reads = n; d.seq_stride = f.stride;
    f.blocks.push_back(d);
    f.ws.push_back(0u);
    cbc_block_result r;
    memset(&r, 0, sizeof r);
    r.status = CBC_ST_OK;
    f.res.push_back(r);
}

static void want_tables(const fab &f, uint32_t exclude, const uint32_t *iv, uint32_t n_iv, cbc_gpu_stats *st)
{
    memset(st, 0, sizeof *st);
    for (size_t i = 0; i < f.recs.size(); i++) {
        const uint32_t *w = (const uint32_t *)&f.recs[i];
        const uint32_t flag = w[1] & 0xffffu, len = w[1] >> 16;
        if (iv) {
            bool hit = false;
            for (uint32_t k = 0; k < n_iv && !hit; k++) hit = f.pos[i] <= iv[2 * k + 1] && f.pos[i] + f.span[i] - 1u >= iv[2 * k];
            if (!hit) continue;
        }
        if (flag & exclude) { st->excluded++; continue; }
        st->reads++; st->flag[flag]++; st->len[len]++;
        const uint8_t *row = f.rows.data() + i * f.stride;
        uint32_t gc = 0;
        for (uint32_t c = 0; c < len; c++) {
            uint8_t b = (flag & 16u) ? row[len - 1u - c] : row[c];
            if (row[c] == 'G' || row[c] == 'C') gc++;
            if (flag & 16u) b = b == 'A' ? 'T' : b == 'T' ? 'A' : b == 'C' ? 'G' : b == 'G' ? 'C' : b;
            const uint32_t s = b == 'A' ? 0u : b == 'C' ? 1u : b == 'G' ? 2u : b == 'T' ? 3u : 4u;
            st->cyc[s * CBC_STATS_CYCLES + c]++;
        }
        if (len) st->gc[100u * gc / len]++;
    }
}

static int fab_check(const char *what, fab &f, uint32_t exclude, uint32_t grid, uint32_t n_waves, const std::vector<uint32_t> *iv)
{
    std::vector<uint8_t> rows(f.rows);
    rows.resize(rows.size() + 8u, 0xEEu);                            /* exactly the spare bytes cbc_region_block asks for */
    std::vector<uint32_t> biv;
    for (size_t b = 0; b < f.blocks.size(); b++) { biv.push_back(0u); biv.push_back(iv ? (uint32_t)(iv->size() / 2u) : 0u); }
    std::vector<cbc_gpu_stats> got(1), want(1);
    const int rc = emu_stats(f.recs.data(), f.recs.size(), rows.data(), rows.size(), f.blocks.data(), f.ws.data(), f.res.data(),
                             (uint32_t)f.blocks.size(), iv ? iv->data() : NULL, iv ? (uint32_t)(iv->size() / 2u) : 0u, biv.data(), exclude,
                             grid, n_waves, &got[0]);
    want_tables(f, exclude, iv ? iv->data() : NULL, iv ? (uint32_t)(iv->size() / 2u) : 0u, &want[0]);
    const int bad = rc != 0 || memcmp(&got[0], &want[0], sizeof(cbc_gpu_stats)) != 0;
    printf("%-58s %s (rc %d, %llu reads, %llu excluded)\n", what, bad ? "MISMATCH" : "ok", rc, (unsigned long long)got[0].reads,
           (unsigned long long)got[0].excluded);
    return bad;
}

int main()
{
    int bad = 0;
    static const uint32_t lens[] = { 0, 1, 2, 3, 4, 5, 6, 7, 8, 63, 64, 65, 150, 251, 252, 253, 254, 255, 256 };
    static const uint32_t flags[] = { 0, 16, 99, 147, 1024, 2048 + 16, 256, 512 + 83, 4095 & ~4, 4096 + 16, 4095, 4096, 65535, 40000 };
    for (uint32_t stride = 256u; stride >= 4u; stride = stride == 256u ? 152u : stride == 152u ? 8u : stride == 8u ? 4u : 0u) {
        /* every length the stride holds, forward and reverse, every kind of row; blocks of 1, 63, 64 and 65 reads */
        fab f; f.stride = stride;
        uint32_t pos = 10;
        for (int kind = 0; kind < 5; kind++)
            for (size_t i = 0; i < sizeof lens / sizeof lens[0]; i++)
                if (lens[i] <= stride) for (uint32_t fl = 0; fl <= 16u; fl += 16u) fab_read(f, pos += 3u, fl | (kind == 4 ? 1024u : 0u), lens[i], kind);
        for (size_t i = 0; i < 3u * sizeof flags / sizeof flags[0]; i++) fab_read(f, pos += 2u, flags[i % (sizeof flags / sizeof flags[0])], stride - (uint32_t)(i % 3u), 0);
        while (f.recs.size() < 1u + 63u + 64u + 65u + 130u) fab_read(f, pos += 1u, 83u, stride, 0);
        uint32_t at = 0;
        static const uint32_t sizes[] = { 1, 63, 64, 65 };
        for (int i = 0; i < 4; i++) { fab_block(f, at, sizes[i]); at += sizes[i]; }
        fab_block(f, at, 0u);                                           /* an empty block */
        fab_block(f, at, (uint32_t)f.recs.size() - at);
        char what[96];
        snprintf(what, sizeof what, "stride %u, every length and kind, the device's grid", stride);
        bad |= fab_check(what, f, 0u, 0u, 4u, NULL);
        snprintf(what, sizeof what, "stride %u, one wavefront per workgroup, grid 1", stride);
        bad |= fab_check(what, f, 0u, 1u, 1u, NULL);
        snprintf(what, sizeof what, "stride %u, grid 2 of 3 wavefronts, exclude 16", stride);
        bad |= fab_check(what, f, 16u, 2u, 3u, NULL);
        snprintf(what, sizeof what, "stride %u, exclude 0x400", stride);
        bad |= fab_check(what, f, 0x400u, 0u, 4u, NULL);
        std::vector<uint32_t> iv;
        iv.push_back(1u); iv.push_back(40u); iv.push_back(100u); iv.push_back(100u); iv.push_back(pos - 20u); iv.push_back(pos + 500u);
        snprintf(what, sizeof what, "stride %u, three intervals", stride);
        bad |= fab_check(what, f, 0u, 0u, 4u, &iv);
        snprintf(what, sizeof what, "stride %u, three intervals, exclude 16, grid 1", stride);
        bad |= fab_check(what, f, 16u, 1u, 2u, &iv);
        iv.clear(); iv.push_back(0x7fffff00u); iv.push_back(0x7fffffffu);
        snprintf(what, sizeof what, "stride %u, an interval that selects nothing", stride);
        bad |= fab_check(what, f, 0u, 0u, 4u, &iv);
    }
    {   /* same-address adds: 64 reads of one FLAG and one length in one block; then a failed block next to it */
        fab f; f.stride = 100u;
        for (uint32_t i = 0; i < 64u; i++) fab_read(f, 5u + i, 83u, 100u, 0);
        for (uint32_t i = 0; i < 64u; i++) fab_read(f, 90u + i, 4096u + 83u, 99u, 0);
        fab_block(f, 0u, 64u); fab_block(f, 64u, 64u);
        bad |= fab_check("64 reads of one FLAG in LDS, 64 of one FLAG in global", f, 0u, 0u, 4u, NULL);
        f.res[1].status = 2u;
        std::vector<cbc_gpu_stats> got(1), zero(1);
        memset(&zero[0], 0, sizeof(cbc_gpu_stats));
        std::vector<uint8_t> rows(f.rows);
        rows.resize(rows.size() + 8u, 0xEEu);
        const int rc = emu_stats(f.recs.data(), f.recs.size(), rows.data(), rows.size(), f.blocks.data(), f.ws.data(), f.res.data(), 2u, NULL, 0u,
                                 NULL, 0u, 0u, 4u, &got[0]);
        const int b2 = rc != CBC_E_BLOCK || memcmp(&got[0], &zero[0], sizeof(cbc_gpu_stats)) != 0;
        printf("%-58s %s (rc %d)\n", "a failed block: CBC_E_BLOCK and all-zero tables", b2 ? "MISMATCH" : "ok", rc);
        bad |= b2;
    }
    if (g_emu_errors) bad = 1;
    printf(bad ? "STATS EMU CHECK FAILED\n" : "STATS EMU CHECK OK\n");
    return bad;
}
#endif
