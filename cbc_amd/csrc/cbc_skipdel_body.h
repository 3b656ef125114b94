/*
 * cbc_skipdel_body.h -- deletion-aware coverage on the device: the "unmark" stage of the depth kinds under
 * cbc_gpu_set_depth_skip_deletions (include/cbc_gpu.h).
 *
 * Under the option the depth at position p is the kept reads that have an ALIGNED base at p: the span depth of
 * cbc_depth_body.h less the deleted bases of the kept reads at p.  The edit-reporting decoder (cbc_decode_body.h, EDITS = true)
 * has left, per read with indels, the matched coordinates dc[] of its deleted bases (cbc_dec_edits); deleted base d lies at
 * POS + dc[d] + d, the form cbc_pileup_events counts its `del` column with (cbc_edits_del_offset, cbc_pileup_body.h).
 *
 * The stage runs behind the mark kernel and in front of cbc_depth_tile, on the same stream.  The mark pass has added +1 at the
 * first word of a kept read's piece of the difference array and -1 behind its last one; per deleted base at word x of that
 * piece this pass adds -1 (mod 2^32) at x and +1 at x + 1, by the same relaxed agent-scope atomics.  Neighbouring deleted bases
 * cancel on the word they share, so a run of deletions leaves two non-zero words, and everything behind the front (tile sums,
 * scans, change points, text, sums, thresholds, quantiles, bins) reads the new depth without knowing of it.
 *
 * Neither form restates the keep rule or the clipping: each IS its mark body (cbc_depth_mark, cbc_targets_mark) instantiated with
 * a hook U that is handed every group's kept reads in place of the +1 / -1 and the count, so mark and unmark cannot drift apart.
 *   window     cbc_skipdel_unmark: `n_waves` wavefronts per block share its kept reads with nDel > 0; a read is taken by the
 *              whole wavefront, one lane per deleted base, 64 a turn.  A deleted base is counted iff its word lies in
 *              [i0, i1), the read's own piece as the mark pass clipped it: inside the span and inside the window.
 *   target set cbc_skipdel_targets_unmark: the same over the compressed coordinate (cbc_targets_body.h).  A deleted base finds
 *              its interval by cbc_targets_find over the block's interval range and is dropped when it falls into a gap.  On an
 *              interval's last position its +1 lands on the spare slot, where the read's own -1 sits too: the spare slot still
 *              ends at depth 0.
 * The depth cannot wrap below zero for what the decoder writes: dc[d] + d ascends strictly, so a read takes a position off at
 * most once, and only where the mark pass put it on.  The guards against a hostile arena are those of cbc_pileup_events
 * (cbc_edits_block, cbc_edits_read_ok); a failed block contributes nothing (cbc_region_block).  n_reads_kept, the start slots of
 * cbc_targets_mark_starts and so the `reads` column keep their span meaning: this pass touches the difference array alone.
 * No LDS.  Written against the wave policy (W = WaveGPU in cbc_gpu.hip, the lock-step emulation in tests/skipdel_emu).
 */
#ifndef CBC_SKIPDEL_BODY_H
#define CBC_SKIPDEL_BODY_H

#include <stdint.h>
#include "../../include/cbc_gpu.h"
#include "cbc_region_body.h"
#include "cbc_depth_body.h"
#include "cbc_targets_body.h"
#include "cbc_pileup_body.h"       /* cbc_edits_block, cbc_edits_read_ok, cbc_edits_del_offset */

#define CBC_SKIPDEL_WAVES 4u       /* wavefronts that share one block's reads with deletions */

/* the EDITS decoder's side array and arena, as cbc_pileup_args names them */
struct cbc_skipdel_edits {
    const uint32_t *side;
    const uint16_t *arena;
    uint64_t arena_entries;
    uint32_t per_read, reserved;
};

struct cbc_skipdel_args  { cbc_depth_args D;  cbc_skipdel_edits E; };
struct cbc_tskipdel_args { cbc_tdepth_args T; cbc_skipdel_edits E; };

/* what both forms do with the side words of a group's kept reads: the reads with nDel > 0 are dealt to the block's wavefronts in
 * turn (nq counts them over the whole block), and every read a wavefront takes is handed to `one(j, ar, nd)`: its lane, its
 * matched coordinates dc = ar[0 .. nd) */
struct cbc_skipdel_blk { cbc_edits_blk E; uint32_t wave, n_waves, nq; };

template <class W, class F>
CBC_FN void cbc_skipdel_group(cbc_skipdel_blk &X, uint32_t r0, typename W::Mask k, const F &one)
{
    typedef typename W::V32 V32;
    const V32 ln = W::lane();
    const V32 sd1 = W::load32(X.E.side, (ln + r0) * 2u + 1u, k, 0u);
    k = k & ((sd1 & 0xffffu) != 0u);
    uint64_t bits = W::ballot(k);
    if (bits == 0ull) return;
    const V32 sd0 = W::load32(X.E.side, (ln + r0) * 2u, k, 0u);
    while (bits) {
        const uint32_t j = W::ctz64(bits);
        bits &= bits - 1u;
        if ((X.nq++ % X.n_waves) != X.wave) continue;
        const uint32_t e0 = W::readlane(sd0, j), cnt = W::readlane(sd1, j), nd = cnt & 0xffffu, ni = cnt >> 16;
        if (!cbc_edits_read_ok(e0, nd, ni, X.E.cap)) continue;
        one(j, X.E.arena + e0, nd);
    }
}

/* ---- window ------------------------------------------------------------------------------------------------------------ */
/* the U of cbc_depth_mark (cbc_depth_body.h): the kept reads of a group, clipped as the mark pass clipped them */
struct cbc_skipdel_win : cbc_skipdel_blk {
    static const bool unmark = true;
    template <class W>
    CBC_MFN void reads(uint32_t *p, uint32_t sub, uint32_t r0, const typename W::Mask &k, const typename W::V32 &lp,
                      const typename W::V32 &span, const typename W::V32 &i0, const typename W::V32 &i1)
    {
        typedef typename W::V32 V32;
        typedef typename W::Mask Mask;
        cbc_skipdel_group<W>(*this, r0, k, [&](uint32_t j, const uint16_t *ar, uint32_t nd) {
            const V32 ln = W::lane();
            const uint32_t lpj = W::readlane(lp, j), sp = W::readlane(span, j), a = W::readlane(i0, j), b = W::readlane(i1, j);
            for (uint32_t t = 0; t < nd; t += 64u) {                 /* deleted base d: POS + dc[d] + d */
                const V32 d = ln + t;
                const Mask md = d < nd;
                const V32 xo = cbc_edits_del_offset<W>(ar, d, md);   /* below 65536 + 255 */
                const V32 x = xo + lpj;                              /* decoded record: local POS + span < 2^32 */
                const V32 idx = x - sub;
                /* inside the span, and inside the read's own piece [a, b) of the difference array; b <= the last index */
                const Mask in = md & (xo < sp) & (x >= sub) & (idx >= a) & (idx < b);
                W::list_add(p, idx, W::splat(0xffffffffu), in);
                W::list_add(p, idx + 1u, W::splat(1u), in);
            }
        });
    }
};

template <class W>
CBC_FN void cbc_skipdel_unmark(const cbc_skipdel_args &A, uint32_t blk, uint32_t wave, uint32_t n_waves)
{
    if (blk >= A.D.R.n_blocks || n_waves == 0u || wave >= n_waves) return;
    const cbc_dec_block_desc *bd = A.D.R.blocks + blk;
    cbc_skipdel_win U;
    U.E = cbc_edits_block(A.E.side, A.E.arena, A.E.arena_entries, A.E.per_read, bd->rec_base, bd->n_reads);
    U.wave = wave; U.n_waves = n_waves; U.nq = 0u;
    if (!U.E.ok) return;
    cbc_depth_mark<W, cbc_skipdel_win>(A.D, blk, &U);                /* B.ok inside: the side array runs beside the records */
}

/* ---- target set -------------------------------------------------------------------------------------------------------- */
/* the U of cbc_targets_mark (cbc_targets_body.h) */
struct cbc_skipdel_tg : cbc_skipdel_blk {
    static const bool unmark = true;
    uint32_t *diff;                  /* the compressed coordinate's difference array */
    template <class W>
    CBC_MFN void reads(const cbc_targets_blk &T, const uint32_t *off, uint32_t lim, uint32_t r0, const typename W::Mask &k,
                      const typename W::V32 &pos, const typename W::V32 &last)
    {
        typedef typename W::V32 V32;
        typedef typename W::Mask Mask;
        uint32_t *df = diff;
        cbc_skipdel_group<W>(*this, r0, k, [&](uint32_t j, const uint16_t *ar, uint32_t nd) {
            const V32 ln = W::lane();
            const uint32_t pj = W::readlane(pos, j), lj = W::readlane(last, j);      /* POS <= last <= 2^31 - 1 */
            for (uint32_t t = 0; t < nd; t += 64u) {
                const V32 d = ln + t;
                const Mask md = d < nd;
                const V32 xo = cbc_edits_del_offset<W>(ar, d, md);
                const Mask sp = md & (xo <= lj - pj);                /* inside the span: POS + xo <= last, no sum that wraps */
                const V32 p = xo + pj;
                /* the interval that holds p: the first of the block's range with end >= p, if its beg <= p; else p lies in a gap.
                 * end >= p >= POS and beg <= p <= last: one of the intervals the mark pass walked for this read */
                const V32 q = cbc_targets_find<W>(T.iv + 1, 2u, T.cnt, p, sp);
                const Mask ex = sp & (q < T.cnt);
                const V32 bq = W::load32(T.iv, q * 2u, ex, 0u), eq = W::load32(T.iv, q * 2u + 1u, ex, 0u), o = W::load32(off, q, ex, 0u);
                /* the read's piece inside that interval as the mark pass clipped and tested it: slots [c0, c1), c1 < lim; p's
                 * slot s lies in it, and s + 1 <= c1 */
                const V32 f = W::select(bq <= W::splat(pj), W::splat(pj), bq), l = W::select(eq >= W::splat(lj), W::splat(lj), eq);
                const V32 c0 = o + (f - bq), c1 = (o + (l - bq)) + 1u, s = o + (p - bq);
                const Mask in = ex & (bq <= p) & (bq <= eq) & (l >= f) & (c1 > c0) & (c1 < lim);
                W::list_add(df, s, W::splat(0xffffffffu), in);
                W::list_add(df, s + 1u, W::splat(1u), in);
            }
        });
    }
};

template <class W>
CBC_FN void cbc_skipdel_targets_unmark(const cbc_tskipdel_args &A, uint32_t blk, uint32_t wave, uint32_t n_waves)
{
    if (blk >= A.T.D.R.n_blocks || n_waves == 0u || wave >= n_waves) return;
    const cbc_dec_block_desc *bd = A.T.D.R.blocks + blk;
    cbc_skipdel_tg U;
    U.E = cbc_edits_block(A.E.side, A.E.arena, A.E.arena_entries, A.E.per_read, bd->rec_base, bd->n_reads);
    U.wave = wave; U.n_waves = n_waves; U.nq = 0u; U.diff = A.T.D.diff;
    if (!U.E.ok) return;
    cbc_targets_mark<W, false, cbc_skipdel_tg>(A.T, blk, NULL, &U);
}

#endif /* CBC_SKIPDEL_BODY_H */
