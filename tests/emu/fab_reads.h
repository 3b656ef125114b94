/*
 * fab_reads.h -- the fabricated reads of the stand-alone checks (make asan_check) of tests/pileup_emu, pileup_strand_emu,
 * skipdel_emu, cigar_emu and alnstats_emu: reads with deletion coordinates (dc) and inserted read indices (oi), and the arrays
 * the edit-reporting decoder would have left for them -- records, rows, side words, arena entries, block descriptors, decode
 * results -- each an allocation of exactly its size.  TEST AID ONLY.  The checks take no input: the random numbers are a fixed
 * sequence, and the order in which a check consumes rnd() is part of its fixture.
 */
#ifndef CBC_FAB_READS_H
#define CBC_FAB_READS_H

#include <string>
#include <vector>
#include "post_emu.h"

typedef std::vector<uint32_t> vu;

static uint32_t g_rng = 2463534242u;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5; return g_rng; }

static uint32_t klass(uint8_t b) { b &= 0xdfu; return b == 'A' ? 0u : b == 'C' ? 1u : b == 'G' ? 2u : b == 'T' ? 3u : 4u; }

struct fread_ {
    uint32_t pos, flag, len, span; std::string seq; vu dc, oi;
    int raw_cnt, raw_e0;                                              /* >= 0: the side words as given, whatever the lists hold */
    std::string want;                                                 /* cigar: "" = the plain line; else CIGAR \t NM \t MD */
    int want_valid;                                                   /* alnstats: -1 = whatever the host loop says */
};
struct fab {
    uint32_t stride, per_read;
    bool bases = true;                                                /* false (skipdel): no bases -- the rows stay 0xEE, no rnd() */
    bool on_ref = false;                                              /* true (cigar, alnstats): aligned bases are the reference's */
    std::vector<fread_> reads;
    vu block_n;                                                       /* reads per block */
    std::vector<uint8_t> ref;                                         /* window start 0: position p is ref[p - 1] */
};

/* a read of `len` random bases at `pos` with the given edits; span < 0: the honest one.  f.on_ref: the reference's bytes at its
 * aligned indices instead */
static fread_ &fab_read(fab &f, uint32_t pos, uint32_t flag, uint32_t len, vu dc, vu oi, int span = -1)
{
    fread_ r;
    r.pos = pos; r.flag = flag; r.len = len; r.dc = dc; r.oi = oi; r.raw_cnt = r.raw_e0 = -1; r.want_valid = -1;
    r.span = span >= 0 ? (uint32_t)span : len + (uint32_t)dc.size() - (oi.size() < len ? (uint32_t)oi.size() : len);
    for (uint32_t i = 0; f.bases && i < len; i++) r.seq.push_back("ACGTNacgtRn"[rnd() % 11u]);
    uint32_t nb = 0;
    for (uint32_t q = 0; f.on_ref && q < len; q++) {
        bool ins = false;
        for (uint32_t o : oi) ins |= o == q;
        if (ins) { nb++; continue; }
        uint32_t m = q - nb, sh = 0;
        for (uint32_t d : dc) sh += d <= m;
        const uint64_t at = (uint64_t)pos - 1u + m + sh;
        if (at < f.ref.size()) r.seq[q] = (char)f.ref[at];
    }
    f.reads.push_back(r);
    return f.reads.back();
}

/* the same, but for mismatches at the read indices in `mis` */
static fread_ &fab_read(fab &f, uint32_t pos, uint32_t flag, uint32_t len, vu dc, vu oi, vu mis)
{
    fread_ &r = fab_read(f, pos, flag, len, dc, oi);
    for (uint32_t q : mis) if (q < len) r.seq[q] = (char)(r.seq[q] == 'A' ? 'C' : 'A');
    return r;
}

struct fab_arrays {
    std::vector<cbc_read_rec> recs;
    std::vector<uint8_t> rows;
    vu side;
    std::vector<uint16_t> arena;
    std::vector<cbc_dec_block_desc> blocks;
    std::vector<uint64_t> ws;
    std::vector<cbc_block_result> res;
    std::vector<int> failed;
};

/* the arrays behind f's reads, block by block; block fail_block's decode result is fail_status.  false: a block's edits do not
 * fit its part of the arena -- a bad fixture */
static bool fab_build(const fab &f, fab_arrays &a, int fail_block = -1, uint32_t fail_status = CBC_ST_EDITS)
{
    const size_t n = f.reads.size(), nb = f.block_n.size();
    a.recs.assign(n ? n : 1, cbc_read_rec());
    a.rows.assign(n * f.stride + 8u, 0xEEu);                        /* exactly the spare bytes cbc_region_block asks for */
    a.side.assign(2u * (n ? n : 1), 0u);
    a.arena.assign(n * f.per_read, 0xEEEEu);
    a.blocks.assign(nb, cbc_dec_block_desc()); a.ws.assign(nb, 0u); a.res.assign(nb, cbc_block_result()); a.failed.assign(nb, 0);
    size_t at = 0;
    for (size_t b = 0; b < nb; b++) {
        a.blocks[b].rec_base = at; a.blocks[b].seq_base = (uint64_t)at * f.stride; a.blocks[b].n_reads = f.block_n[b]; a.blocks[b].seq_stride = f.stride;
        if ((int)b == fail_block) { a.res[b].status = fail_status; a.failed[b] = 1; }
        uint32_t used = 0;
        for (uint32_t k = 0; k < f.block_n[b]; k++, at++) {
            const fread_ &r = f.reads[at];
            uint32_t *w = (uint32_t *)&a.recs[at];
            w[0] = r.pos; w[1] = r.flag | (r.len << 16); w[2] = k * f.stride; w[3] = r.span;
            memcpy(a.rows.data() + at * f.stride, r.seq.data(), r.seq.size());
            a.side[2 * at] = r.raw_e0 >= 0 ? (uint32_t)r.raw_e0 : (r.dc.size() + r.oi.size()) ? used : 0u;
            a.side[2 * at + 1] = r.raw_cnt >= 0 ? (uint32_t)r.raw_cnt : (uint32_t)r.dc.size() | ((uint32_t)r.oi.size() << 16);
            if (r.raw_cnt >= 0 || r.raw_e0 >= 0) continue;
            if (used + r.dc.size() + r.oi.size() > (size_t)f.block_n[b] * f.per_read) return false;
            for (uint32_t d : r.dc) a.arena[a.blocks[b].rec_base * f.per_read + used++] = (uint16_t)d;
            for (uint32_t o : r.oi) a.arena[a.blocks[b].rec_base * f.per_read + used++] = (uint16_t)o;
        }
    }
    return true;
}

/* a text call that just passed with `bytes` > 0 of text, once more with a text_cap one byte short: CBC_E_ARG, the size
 * reported in out[0], nothing written.  call(text, text_cap) -> rc; width: of the case's name in the check's output */
template <class Call>
static int fab_short_probe(const char *what, int width, Call call, size_t bytes, const uint64_t *out)
{
    std::vector<uint8_t> t2(bytes + 16u, 0xEEu);
    const int rc2 = call(t2.data(), bytes - 1u);
    int bad = rc2 != CBC_E_ARG || out[0] != bytes;
    for (size_t i = 0; i < t2.size(); i++) bad |= t2[i] != 0xEEu;
    if (bad) printf("%-*s MISMATCH (text_cap one byte short: rc %d)\n", width, what, rc2);
    return bad;
}

/* ---- the pileup checks (tests/pileup_emu, tests/pileup_strand_emu) ------------------------------------------------------------ */
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

/* the fixture of both checks: a reference of 6000 bytes, every kind of read at every length, blocks of 0, 1, 63, 64, 65 reads and
 * the rest; pos: the last read's POS */
static void fab_pileup_cases(fab &f, uint32_t &pos)
{
    f.stride = 152u; f.per_read = 16u;
    for (uint32_t i = 0; i < 6000u; i++) f.ref.push_back("ACGTNacgtnRYk"[rnd() % 13u]);    /* lower-case and IUPAC reference bytes */
    static const uint32_t lens[] = { 1, 3, 4, 5, 63, 64, 65, 100, 150 };
    pos = 5;
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
    {
        const uint32_t sizes[] = { 0, 1, 63, 64, 65 };
        uint32_t at = 0;
        for (int i = 0; i < 5; i++) { f.block_n.push_back(sizes[i]); at += sizes[i]; }
        f.block_n.push_back((uint32_t)f.reads.size() - at);
    }
}

#endif
