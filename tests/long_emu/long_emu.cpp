/*
 * long_emu.cpp -- cbc_long_decode (cbc_amd/csrc/cbc_long_body.h) on the CPU wave emulation over CORRUPTED long-read containers.
 * TEST AID ONLY.  Built with -DLONG_EMU_MAIN as long_emu_check under AddressSanitizer / UBSan (make asan_check) and run by
 * tests/test_long_edges.py as a process of its own on a dump of a real container:
 *
 *   "CBLEDGE1"  u64 n_blocks  u64 cap_pos  u64 ref_bytes  u64 payload_bytes
 *   n_blocks x { cbc_dec_block_desc (64 bytes), u64 ref_need = reference bytes the block's reads reach }
 *   payload bytes, reference bytes
 *
 * Every trial decodes ONE block with every buffer allocated at exactly the size the call is told (payload rounded up to whole
 * words as the decoder asks, records n_reads, bases reserved[0] + 8, reference ref_bytes, tables CBC_LONG_TABLE_WORDS, LDS
 * cbc_long_dec_lds_bytes), so that a read or write outside them is a sanitizer finding.  The program exits 0 only if every trial
 * returned, every status is a documented CBC_ST_* value, nothing was written behind the block's declared bases, and a status of
 * 0 came with records that tile exactly those bases.
 */
#include <vector>
#include "../emu/wave_emu.h"
#include "../../cbc_amd/csrc/cbc_long_body.h"

static int g_invariant = 0;
extern "C" void emu_oob(const char *what) { fprintf(stderr, "[emu] invariant violated: %s\n", what); g_invariant++; }

#ifdef LONG_EMU_MAIN
struct Blk { cbc_dec_block_desc bd; uint64_t ref_need; };
static std::vector<Blk> g_blk;
static std::vector<uint8_t> g_pay, g_ref;
static uint32_t g_cap_pos;
static int g_fail = 0, g_trials = 0;
static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }

static void bad(const char *what, const char *trial, uint32_t b, uint64_t x)
{
    fprintf(stderr, "FAIL %s: %s (block %u, %llu)\n", trial, what, b, (unsigned long long)x);
    g_fail++;
}

/* one block, its payload given apart (in_bytes of it are the call's); returns the status */
static uint32_t decode_one(const char *trial, uint32_t b, const uint8_t *pay, uint32_t in_bytes, uint32_t blk_bases, uint64_t ref_bytes)
{
    g_trials++;
    cbc_dec_block_desc bd = g_blk[b].bd;
    bd.in_off = 0; bd.in_bytes = in_bytes; bd.rec_base = 0; bd.seq_base = 0; bd.reserved[0] = blk_bases;
    const size_t in_alloc = ((size_t)in_bytes + 3u) & ~(size_t)3u, seq_alloc = (size_t)blk_bases + 8u;
    uint8_t *in = (uint8_t *)malloc(in_alloc ? in_alloc : 1), *ref = (uint8_t *)malloc(ref_bytes ? ref_bytes : 1), *seq = (uint8_t *)malloc(seq_alloc);
    cbc_read_rec *recs = (cbc_read_rec *)malloc(sizeof(cbc_read_rec) * (bd.n_reads ? bd.n_reads : 1));
    cbc_block_result *res = (cbc_block_result *)malloc(sizeof(cbc_block_result));
    uint32_t *tables = (uint32_t *)malloc(4u * CBC_LONG_TABLE_WORDS), *lds = (uint32_t *)malloc(cbc_long_dec_lds_bytes(g_cap_pos));
    if (!in || !ref || !seq || !recs || !res || !tables || !lds) { fprintf(stderr, "out of memory\n"); exit(3); }
    memset(in, 0, in_alloc ? in_alloc : 1); memcpy(in, pay, in_bytes);
    memcpy(ref, g_ref.data(), ref_bytes);
    memset(seq, 0xEE, seq_alloc); memset(recs, 0xEE, sizeof(cbc_read_rec) * (bd.n_reads ? bd.n_reads : 1));
    memset(res, 0xEE, sizeof *res); memset(tables, 0xEE, 4u * CBC_LONG_TABLE_WORDS); memset(lds, 0xEE, cbc_long_dec_lds_bytes(g_cap_pos));
    cbc_dec_args A;
    memset(&A, 0, sizeof A);
    A.in = in; A.blocks = &bd; A.ref = ref; A.recs = recs; A.seq = seq; A.results = res; A.var_scratch = tables;
    A.in_bytes = in_alloc; A.ref_bytes = ref_bytes; A.n_recs = bd.n_reads; A.seq_bytes = seq_alloc; A.var_scratch_words = CBC_LONG_TABLE_WORDS;
    A.n_blocks = 1; A.cap_pos = g_cap_pos; A.cap_var = 0;
    cbc_long_decode<WaveEmu>(A, 0u, lds);
    const uint32_t st = res->status;
    if (st > CBC_ST_EDITS) bad("status is no CBC_ST_* value", trial, b, st);
    for (uint32_t k = 0; k < 8u; k++) if (seq[blk_bases + k] != 0xEE) { bad("wrote behind the block's declared bases", trial, b, k); break; }
    if (st == CBC_ST_OK) {
        uint64_t so = 0;
        if (res->nbytes != bd.n_reads) bad("status 0 without all records", trial, b, res->nbytes);
        for (uint32_t r = 0; r < bd.n_reads; r++) {
            if (recs[r].seq_off != so || recs[r].rlen == 0 || so + recs[r].rlen > blk_bases) { bad("status 0 with a record outside the declared bases", trial, b, r); break; }
            so += recs[r].rlen;
        }
        if (so != blk_bases) bad("status 0 but the records do not fill the declared bases", trial, b, so);
    }
    free(in); free(ref); free(seq); free(recs); free(res); free(tables); free(lds);
    return st;
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s container.dump\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    char magic[8]; uint64_t h[4];
    if (fread(magic, 1, 8, f) != 8 || memcmp(magic, "CBLEDGE1", 8) || fread(h, 8, 4, f) != 4) { fprintf(stderr, "not a dump\n"); return 2; }
    g_blk.resize(h[0]); g_cap_pos = (uint32_t)h[1]; g_ref.resize(h[2]); g_pay.resize(h[3]);
    for (auto &k : g_blk) if (fread(&k.bd, sizeof k.bd, 1, f) != 1 || fread(&k.ref_need, 8, 1, f) != 1) { fprintf(stderr, "short dump\n"); return 2; }
    if (fread(g_pay.data(), 1, g_pay.size(), f) != g_pay.size() || fread(g_ref.data(), 1, g_ref.size(), f) != g_ref.size()) { fprintf(stderr, "short dump\n"); return 2; }
    fclose(f);
    const uint32_t nb = (uint32_t)g_blk.size();
    if (!nb) { fprintf(stderr, "no blocks\n"); return 2; }
    for (uint32_t b = 0; b < nb; b++) {
        const Blk &k = g_blk[b];
        if (k.bd.in_off + k.bd.in_bytes > g_pay.size() || k.bd.in_bytes <= 16u || k.ref_need > g_ref.size() || k.ref_need <= k.bd.ref_off) { fprintf(stderr, "dump out of range\n"); return 2; }
    }

    /* the container as it is: the harness itself is right */
    for (uint32_t b = 0; b < nb; b++)
        if (decode_one("clean", b, g_pay.data() + g_blk[b].bd.in_off, g_blk[b].bd.in_bytes, g_blk[b].bd.reserved[0], g_ref.size()) != CBC_ST_OK)
            bad("the clean block does not decode", "clean", b, 0);
    /* 1 - 3 bit flips past the 8-byte header */
    for (uint32_t t = 0; t < 160u; t++) {
        const uint32_t b = t % nb, n = g_blk[b].bd.in_bytes;
        std::vector<uint8_t> p(g_pay.begin() + g_blk[b].bd.in_off, g_pay.begin() + g_blk[b].bd.in_off + n);
        /* early bytes more often: a flip there reaches every later symbol */
        for (uint32_t k = 0, nf = 1u + (uint32_t)(rnd() % 3u); k < nf; k++) {
            const uint64_t span = (t & 1u) ? (uint64_t)(n - 8u) * 8u : ((uint64_t)(n - 8u) * 8u < 2048u ? (uint64_t)(n - 8u) * 8u : 2048u);
            const uint64_t bit = 64u + rnd() % span;
            p[bit >> 3] ^= (uint8_t)(1u << (bit & 7u));
        }
        decode_one("bit flips", b, p.data(), n, g_blk[b].bd.reserved[0], g_ref.size());
    }
    /* truncation at every 64th byte */
    for (uint32_t b = 0; b < nb; b++)
        for (uint32_t cut = 0; cut < g_blk[b].bd.in_bytes; cut += 64u)
            decode_one("truncation", b, g_pay.data() + g_blk[b].bd.in_off, cut, g_blk[b].bd.reserved[0], g_ref.size());
    /* a block index whose base count is off by one: the stream and the index disagree, whatever else holds */
    for (uint32_t b = 0; b < nb; b++)
        for (int d = -1; d <= 1; d += 2)
            if (decode_one("base count off by one", b, g_pay.data() + g_blk[b].bd.in_off, g_blk[b].bd.in_bytes, g_blk[b].bd.reserved[0] + (uint32_t)d, g_ref.size()) == CBC_ST_OK)
                bad("decoded with a wrong base count", "base count off by one", b, (uint64_t)d);
    /* a reference cut short: a read of the block runs off its end */
    for (uint32_t b = 0; b < nb; b++) {
        const uint64_t need = g_blk[b].ref_need, cuts[] = { 1u, 2u, 3u, 4u, 17u, 64u, 255u, (need - g_blk[b].bd.ref_off) / 2u, need - g_blk[b].bd.ref_off };
        for (uint64_t c : cuts)
            if (c <= need && decode_one("short reference", b, g_pay.data() + g_blk[b].bd.in_off, g_blk[b].bd.in_bytes, g_blk[b].bd.reserved[0], need - c) == CBC_ST_OK)
                bad("decoded a read that runs off the reference", "short reference", b, c);
    }
    if (g_invariant) { fprintf(stderr, "FAIL: %d invariant violations of the emulation\n", g_invariant); g_fail++; }
    if (g_trials < 200) { fprintf(stderr, "FAIL: only %d trials\n", g_trials); g_fail++; }
    if (g_fail) { printf("LONG EMU CHECK FAILED: %d findings in %d trials\n", g_fail, g_trials); return 1; }
    printf("LONG EMU CHECK OK trials=%d\n", g_trials);
    return 0;
}
#endif
