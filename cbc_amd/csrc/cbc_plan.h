/*
 * cbc_plan.h -- host-side sizing helpers shared by the C ABI implementation (cbc_gpu.hip) and the
 * test emulation driver: LDS bytes per wavefront, the worst-case payload area per block and the chunks of the
 * host-buffer pipeline.
 */
#ifndef CBC_PLAN_H
#define CBC_PLAN_H

#include <stdint.h>
#include <string.h>
#include "../../include/cbc_gpu.h"

/* LDS layout constants, in 32-bit words (the kernel bodies take them from here).
 * [0, CBC_PLAN_TABLE_WORDS): model tables shared by encoder and decoder bodies:
 *   256 rlength, 256 snps, 256 indels, 2 x CBC_CAP_NAME contig-name pairs, CBC_BLOOM_WORDS Bloom filter,
 *   2 x CBC_P0_WORDS var events of the "p = 0" contexts (one array per strand, two 16-bit events per word) */
#define CBC_BLOOM_WORDS 256u                        /* 8192 bits, two hash functions (power of two) */
#define CBC_P0_WORDS    512u                        /* per strand: 8 buckets (d & 7) of 64 words = 128 events of 16 bits each */
#define CBC_P0_BUCKET_WORDS 64u                     /* one LDS load per lane scans a whole bucket */
#define CBC_P0_CAP      128u                        /* events per bucket */
#define CBC_PLAN_TABLE_WORDS (768u + 2u * CBC_CAP_NAME + CBC_BLOOM_WORDS + 2u * CBC_P0_WORDS)
#ifndef CBC_BATCH_SLOTS
#define CBC_BATCH_SLOTS 2u                         /* encoder hand-off ring depth (power of two; 2 measured as good as 4) */
#endif
#define CBC_BATCH_WORDS 200u                       /* 64 lo + 64 cnt + 64 n + {len, flags, status, record, match mask x2} */
#define CBC_POS_IDX_WORDS 256u                     /* alphabet index of the small POS deltas (multiple of 64) */
#define CBC_RING_WORDS  256u                       /* output bit ring of the coder wave (power of two) */
#define CBC_RUN_WORDS   16u                        /* scratch of the encoder's SNP run pass: one byte per SNP lane, then the window's 8 words */
/* encoder: tables, hand-off ring, its two counters (8 words), output ring, run-pass scratch; then 3 x cap_pos */
#define CBC_PLAN_LDS_FIXED_WORDS (CBC_PLAN_TABLE_WORDS + CBC_BATCH_SLOTS * CBC_BATCH_WORDS + 8u + CBC_RING_WORDS + CBC_RUN_WORDS)

/* LDS per wavefront: fixed tables + the POS alphabet.  The var-event list is NOT in LDS: it lives in
 * global memory behind the block's payload area (encode) / in the decode scratch, so caps->cap_var
 * only sizes those areas. */
static inline uint32_t cbc_plan_lds_bytes(const cbc_lds_caps *caps)
{
    /* pos_val, pos_occ, pos_pre; + the alphabet index of every POS delta below CBC_POS_IDX_WORDS (one LDS load per lane
     * instead of a walk over the alphabet in fixed_group()) */
    return 4u * (CBC_PLAN_LDS_FIXED_WORDS + 3u * caps->cap_pos + CBC_POS_IDX_WORDS);
}

/* decoder: tables, 80 words scratch read + 256 deletion positions, 512 pos_alpha histograms, 256 insertions;
 * then 2 x cap_pos.  It does not carry the encoder's rings: its LDS footprint decides how many blocks
 * a CU holds, and with one wavefront per block that is the decoder's only latency hiding. */
#define CBC_PLAN_DLDS_SCRATCH_WORDS 336u
#define CBC_PLAN_DLDS_FIXED_WORDS (CBC_PLAN_TABLE_WORDS + CBC_PLAN_DLDS_SCRATCH_WORDS + 768u)
static inline uint32_t cbc_plan_dec_lds_bytes(const cbc_lds_caps *caps)
{
    return 4u * (CBC_PLAN_DLDS_FIXED_WORDS + 2u * caps->cap_pos);
}

/* Upper bound on the payload of a block.  Every model total stays below 2^20, so one coded symbol
 * costs < 20 bits; 3 bytes per symbol leaves slack for the 26-bit flush.  Symbols per record:
 * same_ref 1 + rlength 4 + pos <=5 + flag 1 + match 1 = 12, plus for an imperfect read <= 4 count
 * symbols and 2 per edit (var + chars); stream header 136, contig name + sentinel <= 2*CAP_NAME.
 * nev = the block's edit events (an upper bound).  [0, payload_cap): payload; [payload_cap, out_cap): the
 * block's var-event list (one word per var symbol), kept in HBM/L2 instead of LDS.  Returns the area's size. */
static inline uint64_t cbc_plan_block_area(cbc_block_desc *bd, uint64_t off, uint64_t nev)
{
    const uint64_t nsym = 136u + 2u * CBC_CAP_NAME + 16ull * bd->n_reads + 2 * nev;
    uint64_t payload_cap = (3 * nsym + 256 + 255) & ~255ull;
    uint64_t cap = payload_cap + ((4 * (nev + 64) + 255) & ~255ull);
    if (cap > 0xffffff00ull) { cap = 0xffffff00ull; payload_cap = cap / 2; payload_cap &= ~255ull; }
    bd->out_off = off; bd->out_cap = (uint32_t)cap; bd->reserved = (uint32_t)payload_cap;
    return cap;
}

/* the areas with every block's events counted from its records' tokens */
static inline uint64_t cbc_plan_output(cbc_block_desc *blocks, uint32_t n_blocks,
                                       const cbc_read_rec *recs, const uint32_t *tok)
{
    uint64_t off = 0;
    for (uint32_t b = 0; b < n_blocks; b++) {
        cbc_block_desc *bd = &blocks[b];
        uint64_t nev = 0;
        for (uint32_t r = 0; r < bd->n_reads; r++) {
            const cbc_read_rec *rr = &recs[bd->rec_base + r];
            const uint32_t *t = tok + bd->tok_base + rr->tok_off;
            uint32_t n_cig = t[0] & 0xffffu, n_md = t[0] >> 16;
            nev += n_md;
            for (uint32_t k = 0; k < n_cig; k++) if ((t[2 + k] & 15u) != CBC_OP_M) nev += t[2 + k] >> 4;
        }
        off += cbc_plan_block_area(bd, off, nev);
    }
    return off;
}

/* The same bound without reading a single record: the packer cuts blocks so that none holds more than caps->cap_var - 1
 * edit events, so cap_var bounds every block's event count.  O(blocks) instead of O(records + tokens) on the host -- the
 * per-record form cost more than the whole device pipeline of a cfg2-sized call (2 x 15 ms of 48, round 3). */
static inline uint64_t cbc_plan_output_caps(cbc_block_desc *blocks, uint32_t n_blocks, const cbc_lds_caps *caps)
{
    uint64_t off = 0;
    for (uint32_t b = 0; b < n_blocks; b++) off += cbc_plan_block_area(&blocks[b], off, caps->cap_var);
    return off;
}

/* cbc_plan_output() when the tokens are on the device (cbc_gpu_tokenise_sam): the per-record bound travels in the summaries */
static inline uint64_t cbc_plan_output_summaries(cbc_block_desc *blocks, uint32_t n_blocks, const cbc_tok_record_summary *sums)
{
    uint64_t off = 0;
    for (uint32_t b = 0; b < n_blocks; b++) {
        uint64_t nev = 0;
        for (uint32_t r = 0; r < blocks[b].n_reads; r++) nev += sums[blocks[b].rec_base + r].nt_ev >> 16;
        off += cbc_plan_block_area(&blocks[b], off, nev);
    }
    return off;
}

/* ---- chunks of the host-buffer pipeline (cbc_gpu.hip, encode_blocks_impl / decode_blocks_impl) ----------------------
 * A block is one serial chain (~5.6 ms for 4096 reads) however few blocks a launch holds, and the link moves ~57 GB/s:
 * a batch of >= 512 blocks is cut into runs of consecutive blocks of about equal record counts (~ equal H2D volume),
 * >= 64 MiB and >= 256 blocks each, at most CBC_MAX_CHUNKS, each launched on its own stream the moment it has arrived.
 * That needs a contiguous descriptor list (what the packers produce): rec ranges that follow one another, seq and tok
 * bases in ascending order and inside the arrays.  Any other list, or split == false, is one chunk covering the arrays
 * whole.  Chunk c's ranges: blocks [b0, b1), records [r0, r1), bases [s0, s1), tokens [t0, t1), and the 2-bit code
 * words [w0, w1) it expands -- chunks meet inside a word, which goes with the earlier chunk. */
#define CBC_MAX_CHUNKS 8
typedef struct cbc_chunk { uint32_t b0, b1; uint64_t r0, r1, s0, s1, t0, t1, w0, w1; } cbc_chunk;
typedef struct cbc_chunk_plan { uint32_t n_chunks, contiguous; cbc_chunk c[CBC_MAX_CHUNKS]; } cbc_chunk_plan;

static inline uint64_t cbc_desc_tok_base(const cbc_block_desc *d) { return d->tok_base; }
static inline uint64_t cbc_desc_tok_base(const cbc_dec_block_desc *) { return 0; }      /* decode carries no tokens */

/* vol: the bytes the call moves per record, base and token over the link (what decides the chunk count) */
template <class Desc>
static inline void cbc_plan_chunks(const Desc *B, uint32_t nb, uint64_t n_recs, uint64_t seq_bytes, uint64_t n_tok,
                                   uint64_t vol, bool split, cbc_chunk_plan *p)
{
    bool contiguous = nb > 0;
    for (uint32_t b = 0; b + 1 < nb && contiguous; b++)
        contiguous = B[b + 1].rec_base == B[b].rec_base + B[b].n_reads && B[b + 1].seq_base >= B[b].seq_base
                     && cbc_desc_tok_base(&B[b + 1]) >= cbc_desc_tok_base(&B[b]);
    contiguous = contiguous && B[0].rec_base <= n_recs && B[nb - 1].rec_base + B[nb - 1].n_reads <= n_recs && B[nb - 1].seq_base <= seq_bytes
                 && cbc_desc_tok_base(&B[nb - 1]) <= (n_tok ? n_tok : 1);
    uint32_t n_chunks = 1, cut[CBC_MAX_CHUNKS + 1];
    if (split && contiguous && nb >= 512) {
        uint64_t want = vol / (64ull << 20);
        if (want > CBC_MAX_CHUNKS) want = CBC_MAX_CHUNKS;
        if (want > nb / 256) want = nb / 256;
        if (want >= 2) n_chunks = (uint32_t)want;
    }
    cut[0] = 0; cut[n_chunks] = nb;
    for (uint32_t c = 1; c < n_chunks; c++) {                 /* equal record counts ~ equal bytes */
        const uint64_t target = B[0].rec_base + (B[nb - 1].rec_base + B[nb - 1].n_reads - B[0].rec_base) * c / n_chunks;
        uint32_t lo = cut[c - 1] + 1, hi = nb - (n_chunks - c);
        while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (B[mid].rec_base < target) lo = mid + 1; else hi = mid; }
        cut[c] = lo;
    }
    memset(p, 0, sizeof *p);
    p->n_chunks = n_chunks; p->contiguous = contiguous;
    const bool whole = n_chunks == 1;
    for (uint32_t c = 0; c < n_chunks; c++) {
        cbc_chunk *k = &p->c[c];
        const uint32_t c0 = cut[c], c1 = cut[c + 1];
        k->b0 = c0; k->b1 = c1;
        k->r0 = whole ? 0 : B[c0].rec_base;              k->r1 = whole ? n_recs : B[c1 - 1].rec_base + B[c1 - 1].n_reads;
        k->s0 = whole ? 0 : B[c0].seq_base;              k->s1 = whole || c1 == nb ? seq_bytes : B[c1].seq_base;
        k->t0 = whole ? 0 : cbc_desc_tok_base(&B[c0]);   k->t1 = whole || c1 == nb ? n_tok : cbc_desc_tok_base(&B[c1]);
        k->w0 = c ? p->c[c - 1].w1 : 0;                  k->w1 = (k->s1 + 15) / 16;
        if (k->w1 < k->w0) k->w1 = k->w0;
    }
}

#endif
