/*
 * cbc_targets_body.h -- decode of a SET of regions on the device, after the span-reporting decode of the selected blocks
 * (cbc_gpu_decode_targets, include/cbc_gpu.h).
 *
 * The set is a table of merged intervals {beg, end} (1-based, inclusive, absolute 32-bit contig coordinates), grouped per
 * contig, disjoint and sorted inside a contig -- so their ends are sorted too.  Every block carries the range [first, count)
 * of the intervals its reads can reach.  A read is kept iff the first interval with end >= POS exists and has
 * beg <= POS + span - 1; that interval is found by a per-lane binary search (gathers over the block's range, a wave-uniform
 * trip count).  The comparisons carry no sum that can wrap: POS = window start + local POS is formed only for records with
 * local POS <= 2^31 - 1 - window start, and beg <= POS + span - 1 is taken as beg < POS or span > beg - POS.
 *
 *   reads, SAM   two members of the reads-text skeleton of cbc_region_body.h: the keep rule above, the lines of the region and of
 *                the SAM member.
 *   depth        one contig per call.  The difference array lives in a COMPRESSED coordinate: the contig's intervals laid
 *                end to end with one spare slot behind each (sum of len + 1 words), `iv_off` the exclusive prefix of the
 *                slots.  mark: a lane walks the intervals its read overlaps (from the search result while beg <= the read's
 *                last base), clips the read to each and adds +1 at the piece's first slot, -1 at the slot behind its last
 *                one.  The spare slot therefore always has depth 0: no run crosses a gap, and intervals that were merged
 *                are one interval, so no run is cut inside them.  The tile, scan and compact passes of cbc_depth_body.h run
 *                on that array unchanged.  count / write: the run-text skeleton of cbc_depth_body.h with the line function of
 *                this file: a change point is mapped back to its reference position by a binary search in iv_off; a run of
 *                non-zero depth lies inside one interval (or ends on its spare slot = the interval's end), so its end is
 *                start + the distance of the two change points.
 * Written against the wave policy (W = WaveGPU in cbc_gpu.hip, the lock-step emulation in tests/targets_emu).
 */
#ifndef CBC_TARGETS_BODY_H
#define CBC_TARGETS_BODY_H

#include <stdint.h>
#include "../../include/cbc_gpu.h"
#include "cbc_region_body.h"
#include "cbc_sam_body.h"
#include "cbc_depth_body.h"

struct cbc_targets_args {
    cbc_sam_args S;               /* S.R: records, rows, blocks, window starts, decode results, counts, offsets, text as for the
                                   * region passes (beg = 1, end = UINT64_MAX); block_name / names: SAM output only          */
    const uint32_t *iv;           /* n_iv pairs beg, end                                                                      */
    const uint32_t *block_iv;     /* per block: first interval, count                                                         */
    uint32_t n_iv, reserved;
};

struct cbc_tdepth_args {
    cbc_depth_args D;             /* as for the depth passes; diff = the compressed coordinate, D.R.beg / end unused        */
    const uint32_t *iv;           /* the contig's n_iv intervals                                                              */
    const uint32_t *iv_off;       /* n_iv + 1: first slot of interval i, iv_off[n_iv] = slots in all                          */
    const uint32_t *block_iv;     /* per block: first interval (of the contig's), count                                       */
    uint32_t n_iv, reserved;
};

struct cbc_targets_blk {
    cbc_region_blk B;
    const uint32_t *iv;           /* the block's first interval */
    uint32_t ws, cnt, first;
};

CBC_FN cbc_targets_blk cbc_targets_block(const cbc_region_blk &B, uint64_t ws, const uint32_t *iv, const uint32_t *block_iv,
                                         uint32_t n_iv, uint32_t blk)
{
    cbc_targets_blk T;
    T.B = B;
    const uint32_t first = block_iv[2u * blk], cnt = block_iv[2u * blk + 1u];
    T.B.ok = T.B.ok && ws <= CBC_SAM_MAX_POS && first <= n_iv && cnt <= n_iv - first;
    T.ws = (uint32_t)ws;
    T.first = T.B.ok ? first : 0u;
    T.cnt = T.B.ok ? cnt : 0u;
    T.iv = iv + 2u * (uint64_t)T.first;
    return T;
}

/* per lane: the first i in [0, cnt) with a[i * step] >= key, cnt if none (a[] ascending); floor(log2(cnt)) + 1 rounds */
template <class W>
CBC_FN typename W::V32 cbc_targets_find(const uint32_t *a, uint32_t step, uint32_t cnt, const typename W::V32 &key,
                                        const typename W::Mask &m)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    V32 lo = W::splat(0u), len = W::splat(cnt);
    for (uint32_t s = cnt; s; s >>= 1) {
        const V32 half = len >> 1, mid = lo + half;
        const Mask act = m & (len != 0u);                            /* mid < cnt while len > 0 */
        const V32 e = W::load32(a, mid * step, act, 0xffffffffu);
        const Mask go = act & (e < key);
        lo = W::select(go, mid + 1u, lo);
        len = W::select(go, (len - half) - 1u, half);
    }
    return lo;
}

/* keep flags of records [r0, r0 + 64) with length, local POS, FLAG, span and the interval found (index in the block's range) */
template <class W>
CBC_FN typename W::Mask cbc_targets_keep(const cbc_targets_blk &T, uint32_t r0, typename W::V32 &rlv, typename W::V32 &lp,
                                         typename W::V32 &fl, typename W::V32 &span, typename W::V32 &j)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    const V32 ln = W::lane();
    const Mask m = (ln + r0) < T.B.n;
    V32 w1, off;
    W::load_rec(T.B.recs4, ln + r0, m, lp, w1, off, span);
    rlv = w1 >> 16;
    fl = w1 & 0xffffu;
    const Mask k = m & (rlv <= T.B.stride) & (lp <= CBC_SAM_MAX_POS - T.ws);
    const V32 pos = lp + T.ws;                                       /* <= 2^31 - 1 under k */
    j = cbc_targets_find<W>(T.iv + 1, 2u, T.cnt, pos, k);            /* the ends */
    const Mask ex = k & (j < T.cnt);
    const V32 bj = W::load32(T.iv, j * 2u, ex, 0u);
    return ex & ((bj < pos) | (span > bj - pos));                    /* beg <= POS + span - 1 */
}

/* ---- reads, SAM: the two target-set members of the reads-text skeleton (cbc_region_body.h) ------------------------------- */
struct cbc_targets_tblk : cbc_sam_blk { cbc_targets_blk T; };        /* B = T.B; name, ws, nl are set up for a SAM line alone */

template <int LINE>
CBC_FN cbc_targets_tblk cbc_text_block(const cbc_targets_args &A, uint32_t blk)
{
    cbc_targets_tblk X = {};
    if (LINE == CBC_LINE_SAM) static_cast<cbc_sam_blk &>(X) = cbc_sam_block(A.S, blk); else X.B = cbc_region_block(A.S.R, blk);
    X.T = cbc_targets_block(X.B, A.S.R.window_start[blk], A.iv, A.block_iv, A.n_iv, blk);
    X.B = X.T.B;
    return X;
}

template <class W>
CBC_FN typename W::Mask cbc_text_keep(const cbc_targets_args &, const cbc_targets_tblk &X, uint32_t r0, cbc_text_grp<W> &G)
{
    typename W::V32 span, j;
    return cbc_targets_keep<W>(X.T, r0, G.rlv, G.lp, G.fl, span, j);
}

template <class W>
CBC_FN void cbc_targets_count(const cbc_targets_args &A, uint32_t blk) { cbc_text_count<W, CBC_LINE_BASES>(A, A.S.R, blk); }
template <class W>
CBC_FN void cbc_targets_write(const cbc_targets_args &A, uint32_t blk, uint32_t wave, uint32_t n_waves)
{
    cbc_text_write<W, CBC_LINE_BASES>(A, A.S.R, blk, wave, n_waves);
}
template <class W>
CBC_FN void cbc_targets_sam_count(const cbc_targets_args &A, uint32_t blk) { cbc_text_count<W, CBC_LINE_SAM>(A, A.S.R, blk); }
template <class W>
CBC_FN void cbc_targets_sam_write(const cbc_targets_args &A, uint32_t blk, uint32_t wave, uint32_t n_waves)
{
    cbc_text_write<W, CBC_LINE_SAM>(A, A.S.R, blk, wave, n_waves);
}

/* ---- depth: mark ------------------------------------------------------------------------------------------------------- */
/* STARTS (cbc_gpu_decode_coverage_ext, cbc_covx_body.h): per piece also +1 at its first slot in `starts`, an array as long as
 * the difference array */
/* U as for cbc_depth_mark (cbc_depth_body.h): a U with unmark = true is handed the kept reads of every group instead --
 * U::reads<W>(T, off, lim, r0, k, pos, last): keep flags, POS and the read's last base -- and nothing is marked or counted */
template <class W, bool STARTS = false, class U = cbc_mark_only>
CBC_FN void cbc_targets_mark(const cbc_tdepth_args &A, uint32_t blk, uint32_t *starts = NULL, U *u = NULL)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    const cbc_targets_blk T = cbc_targets_block(cbc_region_block(A.D.R, blk), A.D.R.window_start[blk], A.iv, A.block_iv, A.n_iv, blk);
    if (!T.B.ok || A.D.diff_words == 0u) return;
    const uint32_t *off = A.iv_off + T.first;
    const uint32_t lim = A.D.diff_words > 0xffffffffull ? 0xffffffffu : (uint32_t)A.D.diff_words;   /* slots behind diff */
    const V32 ln = W::lane();
    uint32_t kept = 0;
    for (uint32_t r0 = 0; r0 < T.B.n; r0 += 64u) {
        V32 rlv, lp, fl, span, i;
        Mask k = cbc_targets_keep<W>(T, r0, rlv, lp, fl, span, i);
        k = k & ((fl & (A.D.exclude & 0xffffu)) == 0u) & (span >= 1u);
        kept += W::popc64(W::ballot(k));
        /* the read's last base, not as a sum that wraps (POS <= 2^31 - 1 under k; no interval ends past that) */
        const V32 pos = lp + T.ws;
        const V32 last = W::select((span - 1u) >= (W::splat(CBC_SAM_MAX_POS) - pos), W::splat(CBC_SAM_MAX_POS), pos + (span - 1u));
        if (U::unmark) { u->template reads<W>(T, off, lim, r0, k, pos, last); continue; }
        Mask act = k;                                                /* interval i: end >= POS, and beg <= last by the keep rule */
        while (W::ballot(act) != 0ull) {
            const V32 b = W::load32(T.iv, i * 2u, act, 0u), e = W::load32(T.iv, i * 2u + 1u, act, 0u), o = W::load32(off, i, act, 0u);
            act = act & (b <= last) & (b <= e);
            /* the piece inside interval i: s = max(POS, beg) .. t = min(last, end); slots o + (s - beg) and o + (t - beg) + 1 */
            const V32 s = W::select(pos >= b, pos, b), t = W::select(last <= e, last, e);
            const V32 i0 = o + (s - b), i1 = (o + (t - b)) + 1u;
            const Mask w = act & (t >= s) & (i1 > i0) & (i1 < lim);
            W::list_add(A.D.diff, i0, W::splat(1u), w);
            W::list_add(A.D.diff, i1, W::splat(0xffffffffu), w);
            if (STARTS) W::list_add(starts, i0, W::splat(1u), w);
            i = i + 1u;
            act = act & (i < T.cnt);
        }
    }
    if (U::unmark) return;
    W::list_add(A.D.ctr, W::splat(0u), W::splat(kept), ln == 0u);
}

/* ---- depth: text ------------------------------------------------------------------------------------------------------- */
/* the target-set member of the run-text skeleton (cbc_depth_body.h): runs [j0, j0 + 64) of the contig's `nr` runs: start0, end0,
 * depth and the line's length (0: no line); no guard of its own */
CBC_FN bool cbc_depth_line_ok(const cbc_tdepth_args &) { return true; }

template <class W>
CBC_FN typename W::Mask cbc_depth_line(const cbc_tdepth_args &A, uint32_t j0, uint32_t nr, typename W::V32 &st,
                                       typename W::V32 &en, typename W::V32 &dp, typename W::V32 &len)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    const V32 j = W::lane() + j0;
    const Mask m = j < nr;                                           /* j + 1 <= nr < the change points */
    const V32 p = W::load32(A.D.cp_pos, j, m, 0u), q = W::load32(A.D.cp_pos, j + 1u, m, 0u);
    dp = W::load32(A.D.cp_dep, j, m, 0u);
    /* the interval whose slots hold p: the first i with iv_off[i + 1] > p */
    const Mask k0 = m & (dp != 0u) & (p != 0xffffffffu);
    const V32 i = cbc_targets_find<W>(A.iv_off + 1, 1u, A.n_iv, p + 1u, k0);
    const Mask k = k0 & (i < A.n_iv);
    const V32 b = W::load32(A.iv, i * 2u, k, 1u), o = W::load32(A.iv_off, i, k, 0u);
    st = (b - 1u) + (p - o);                                         /* 0-based */
    en = st + (q - p);                                               /* inside the interval, or its spare slot: the interval's end */
    const V32 l = cbc_sam_ndig_v<W>(st, 1000000000u) + cbc_sam_ndig_v<W>(en, 1000000000u) + cbc_sam_ndig_v<W>(dp, 1000000000u) +
                  (A.D.name_len + 4u);
    len = W::select(k, l, W::splat(0u));
    return k;
}

template <class W>
CBC_FN void cbc_targets_depth_count(const cbc_tdepth_args &A, uint32_t tt) { cbc_runs_count<W>(A, A.D, tt); }
template <class W>
CBC_FN void cbc_targets_depth_write(const cbc_tdepth_args &A, uint32_t tt) { cbc_runs_write<W>(A, A.D, tt); }

#endif /* CBC_TARGETS_BODY_H */
