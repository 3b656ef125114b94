/*
 * cbc_region_body.h -- region decode on the device, after the span-reporting decode of the selected blocks
 * (cbc_gpu_decode_region, include/cbc_gpu.h).
 *
 * The decode kernel (cbc_decode_body.h, SPAN = true) has left every record of the selected blocks in the context's arenas:
 * pos (block-local), flag | rlen << 16, the row offset, and the read's span in the fourth word.  Two passes turn them into
 * the text `cbc -x` writes for the reads that overlap [beg, end]:
 *   count  one wavefront per block: keep flags by the overlap rule, the block's kept reads and text bytes (sum of rlen + 1)
 *          by wave reductions, into a cbc_block_result (nbytes = text bytes, n_symbols = reads kept) so that the payload
 *          size scan of the encode path (cbc_scan_sizes_kernel) places the blocks in the text;
 *   write  `n_waves` wavefronts per block share its kept reads; a read is written by the whole wavefront: the dwords of the
 *          OUTPUT that lie inside the read's text are one aligned 4-byte store per lane (source bytes funnel-shifted out of
 *          two row words), the at most 3 + 3 bytes it shares with its neighbours are byte stores.
 * Both passes are the reads-text skeleton below (cbc_text_count / cbc_text_write), which cbc_sam_body.h and cbc_targets_body.h
 * instantiate too; cbc_store_result, the one place a wavefront stores a cbc_block_result, lives here as well.
 * Overlap rule: POS <= end and POS + span - 1 >= beg with POS = window_start + local POS, evaluated in local coordinates
 * (32-bit lanes, no 64-bit sums): local POS <= end - window_start and local POS + span >= beg + 1 - window_start.
 * Written against the wave policy (W = WaveGPU in cbc_gpu.hip, the lock-step emulation in the tests).
 */
#ifndef CBC_REGION_BODY_H
#define CBC_REGION_BODY_H

#include <stdint.h>
#include "../../include/cbc_gpu.h"

struct cbc_region_args {
    const cbc_read_rec       *recs;          /* the decode's records (tok_off = span)              */
    const uint8_t            *seq;           /* the decode's rows                                  */
    const cbc_dec_block_desc *blocks;        /* the selected blocks as decoded                     */
    const uint64_t           *window_start;  /* per block                                          */
    const cbc_block_result   *dec_results;   /* decode status per block: a failed block keeps none */
    cbc_block_result         *counts;        /* count pass out: nbytes = text bytes, n_symbols = reads kept */
    const uint64_t           *offsets;       /* write pass in: exclusive scan of counts[].nbytes (n_blocks + 1) */
    uint8_t                  *text;
    uint64_t text_cap, n_recs, seq_bytes, beg, end;
    uint32_t n_blocks, reserved;
};

/* where a block's reads are and the overlap bounds in its local coordinates; ok = false: the block keeps nothing */
struct cbc_region_blk {
    const uint4 *recs4; const uint8_t *rows;
    uint32_t n, stride, hi, lo;
    bool ok;
};

CBC_FN cbc_region_blk cbc_region_block(const cbc_region_args &A, uint32_t blk)
{
    cbc_region_blk B;
    const cbc_dec_block_desc *bd = A.blocks + blk;
    const uint64_t rec_base = bd->rec_base, seq_base = bd->seq_base, ws = A.window_start[blk];
    B.n = bd->n_reads; B.stride = bd->seq_stride;
    B.recs4 = (const uint4 *)(A.recs + rec_base); B.rows = A.seq + seq_base;
    /* the decoder's own range tests (rows + 8 spare bytes: the write pass reads one word past a full row) */
    B.ok = A.dec_results[blk].status == CBC_ST_OK && B.stride >= 4u && B.stride <= 256u && (B.stride & 3u) == 0u &&
           rec_base <= A.n_recs && B.n <= A.n_recs - rec_base && seq_base <= A.seq_bytes &&
           (uint64_t)B.n * B.stride + 8u <= A.seq_bytes - seq_base;
    /* local POS <= end - ws; local POS >= 1, so end < ws + 1 keeps nothing */
    B.ok = B.ok && A.end > ws && A.beg >= 1u && A.beg <= A.end;
    const uint64_t hi = A.end - ws;
    B.hi = hi > 0xffffffffull ? 0xffffffffu : (uint32_t)hi;
    /* local POS + span >= beg + 1 - ws: a decoded record has local POS + span < 2^32 (the decoder keeps POS + rl + 259
     * inside the 32-bit reference window and span <= rl + 255), so a bound at or past 2^32 keeps nothing */
    const uint64_t need = A.beg + 1u;
    const uint64_t lo = need > ws ? need - ws : 0u;
    B.ok = B.ok && lo <= 0xffffffffull;
    B.lo = (uint32_t)lo;
    return B;
}

/* keep flags of records [r0, r0 + 64): lp + span >= lo without the sum (lp >= lo, or span >= lo - lp) */
template <class W>
CBC_FN typename W::Mask cbc_region_keep(const cbc_region_blk &B, uint32_t r0, typename W::V32 &rlv)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    const V32 ln = W::lane();
    const Mask m = (ln + r0) < B.n;
    V32 lp, fl, off, span;
    W::load_rec(B.recs4, ln + r0, m, lp, fl, off, span);
    rlv = fl >> 16;
    return m & (lp <= B.hi) & ((lp >= B.lo) | (span >= B.lo - lp)) & (rlv <= B.stride);
}

/* one read's text (rl bases + '\n') at dst[0 ..]: the whole wavefront, lane-parallel */
template <class W>
CBC_FN void cbc_region_emit(uint8_t *dst, uint64_t o, const uint8_t *row, uint32_t rl)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    const V32 ln = W::lane();
    const uint32_t n = rl + 1u;
    const uint32_t h = (4u - (uint32_t)(o & 3u)) & 3u;            /* bytes before the first aligned output dword */
    const uint32_t hb = h < n ? h : n, full = (n - hb) >> 2, tail = (n - hb) & 3u;
    /* aligned dwords: lane k writes read bytes hb + 4k .. hb + 4k + 3, taken from row words k and k + 1 (k + 1 <= 64: the
     * word past a full row is one of the 8 spare bytes behind the rows); byte rl is the '\n' */
    const Mask mf = ln < full;
    const uint32_t *row32 = (const uint32_t *)row;
    const V32 w0 = W::load32(row32, ln, mf, 0u), w1 = W::load32(row32, ln + 1u, mf, 0u);
    V32 v = W::funnel_shr(w1, w0, 8u * hb);
    const V32 pk = W::splat(rl - hb) - ln * 4u;                      /* position of '\n' in lane k's dword, if < 4 */
    const V32 sh = (pk & 3u) * 8u;
    v = W::select(pk < 4u, (v & (W::splat(0xffffffffu) ^ (W::splat(0xffu) << sh))) | (W::splat(10u) << sh), v);
    W::store32_bytes(dst + o + hb, ln * 4u, v, mf);
    /* head bytes (lanes 0 .. hb-1) and tail bytes (lanes 4 .. 4+tail-1) */
    const V32 idx = W::select(ln < 4u, ln, ln + (hb + 4u * full - 4u));
    const Mask mb = (ln < hb) | ((ln >= 4u) & (ln < 4u + tail));
    const V32 b = W::load8(row, idx, mb & (idx != rl));
    W::store8(dst + o, idx, W::select(idx == rl, W::splat(10u), b), mb);
}

/* a cbc_block_result from a wavefront, as cbc_scan_sizes_kernel reads it */
template <class W>
CBC_FN void cbc_store_result(cbc_block_result *r, uint32_t nbytes, uint32_t n_symbols)
{
    uint32_t *c = (uint32_t *)r;
    W::write_uni(c, 0u, nbytes); W::write_uni(c, 1u, CBC_ST_OK); W::write_uni(c, 2u, n_symbols); W::write_uni(c, 3u, 0u);
}

/* ---- the reads-text skeleton ---------------------------------------------------------------------------------------------
 * The count and the write pass of every output that is one line per kept read: region and SAM text, and the two of a target
 * set (cbc_sam_body.h, cbc_targets_body.h), and the SAM text with CIGAR and tags (cbc_cigar_body.h).  A member is its argument
 * struct A (R = the cbc_region_args inside: counts, offsets, text) and LINE, which picks the line.  It supplies, overloaded on A
 * and found when the skeleton is instantiated:
 *   cbc_text_block<LINE>(A, blk)      the block set-up X; X.B is its cbc_region_blk
 *   cbc_text_keep<W>(A, X, r0, G)     keep flags of records [r0, r0 + 64); fills G.rlv, and G.lp, G.fl for a SAM line, and
 *                                     G.xa, G.xb where its line wants two more words per record
 * The line is overloaded on cbc_line<LINE>: the bases here, the SAM line in cbc_sam_body.h (its X is a cbc_sam_blk), the SAM
 * line with CIGAR, NM and MD in cbc_cigar_body.h (its X is a cbc_cigar_blk). */
enum { CBC_LINE_BASES = 0, CBC_LINE_SAM = 1, CBC_LINE_SAM_CIGAR = 2 };
template <class W>
struct cbc_text_grp { typename W::V32 rlv, lp, fl, tl, incl, xa, xb; };   /* 64 records: length, local POS, FLAG, line length, its scan; the line's own */
template <int LINE>
struct cbc_line {};

template <class W, class X>
CBC_FN typename W::V32 cbc_line_len(cbc_line<CBC_LINE_BASES>, const X &, const cbc_text_grp<W> &G) { return G.rlv + 1u; }

/* the line of record r0 + j = lane j of the group whose text begins at o */
template <class W, class X>
CBC_FN void cbc_line_emit(cbc_line<CBC_LINE_BASES>, uint8_t *text, uint64_t o, const X &x, uint32_t r0, uint32_t j, const cbc_text_grp<W> &G)
{
    const uint32_t rl = W::readlane(G.rlv, j), at = W::readlane(G.incl, j) - (rl + 1u);
    cbc_region_emit<W>(text, o + at, x.B.rows + (uint64_t)(r0 + j) * x.B.stride, rl);
}

struct cbc_region_tblk { cbc_region_blk B; };
template <int LINE>
CBC_FN cbc_region_tblk cbc_text_block(const cbc_region_args &A, uint32_t blk) { return cbc_region_tblk{cbc_region_block(A, blk)}; }

template <class W>
CBC_FN typename W::Mask cbc_text_keep(const cbc_region_args &, const cbc_region_tblk &X, uint32_t r0, cbc_text_grp<W> &G)
{
    return cbc_region_keep<W>(X.B, r0, G.rlv);
}

/* one wavefront per block: its kept reads and text bytes into counts[blk] for the size scan */
template <class W, int LINE, class Args>
CBC_FN void cbc_text_count(const Args &A, const cbc_region_args &R, uint32_t blk)
{
    const auto X = cbc_text_block<LINE>(A, blk);
    uint32_t kept = 0, bytes = 0;
    if (X.B.ok) {
        for (uint32_t r0 = 0; r0 < X.B.n; r0 += 64u) {
            cbc_text_grp<W> G;
            const typename W::Mask k = cbc_text_keep<W>(A, X, r0, G);
            kept += W::reduce_add(W::select(k, W::splat(1u), W::splat(0u)));
            bytes += W::reduce_add(W::select(k, cbc_line_len<W>(cbc_line<LINE>(), X, G), W::splat(0u)));
        }
    }
    cbc_store_result<W>(R.counts + blk, bytes, kept);
}

/* wavefront `wave` of `n_waves` writes every n_waves-th kept read of block blk.  The line length is asked for behind the keep
 * flags (in the count pass: behind their reduction, so that the two DPP ladders do not interleave) and r0, j go to the line
 * apart (the row address is formed behind the readlanes): profiles/text_bodies_isa.md */
template <class W, int LINE, class Args>
CBC_FN void cbc_text_write(const Args &A, const cbc_region_args &R, uint32_t blk, uint32_t wave, uint32_t n_waves)
{
    const auto X = cbc_text_block<LINE>(A, blk);
    const uint32_t bytes = R.counts[blk].nbytes;
    const uint64_t o0 = R.offsets[blk];
    if (!X.B.ok || bytes == 0u || o0 > R.text_cap || bytes > R.text_cap - o0) return;
    uint64_t o = o0;
    uint32_t q = 0;                                                    /* kept reads of the block so far */
    for (uint32_t r0 = 0; r0 < X.B.n; r0 += 64u) {
        cbc_text_grp<W> G;
        const typename W::Mask k = cbc_text_keep<W>(A, X, r0, G);
        G.tl = W::select(k, cbc_line_len<W>(cbc_line<LINE>(), X, G), W::splat(0u));
        G.incl = W::scan_incl_add(G.tl);
        const uint32_t chunk = W::readlane(G.incl, 63u);
        if (chunk > (o0 + bytes) - o) return;                          /* the records changed under the count pass */
        uint64_t bits = W::ballot(k);
        while (bits) {
            const uint32_t j = W::ctz64(bits);
            bits &= bits - 1u;
            if ((q++ % n_waves) != wave) continue;
            cbc_line_emit<W>(cbc_line<LINE>(), R.text, o, X, r0, j, G);
        }
        o += chunk;
    }
}

template <class W>
CBC_FN void cbc_region_count(const cbc_region_args &A, uint32_t blk) { cbc_text_count<W, CBC_LINE_BASES>(A, A, blk); }
template <class W>
CBC_FN void cbc_region_write(const cbc_region_args &A, uint32_t blk, uint32_t wave, uint32_t n_waves)
{
    cbc_text_write<W, CBC_LINE_BASES>(A, A, blk, wave, n_waves);
}

#endif /* CBC_REGION_BODY_H */
