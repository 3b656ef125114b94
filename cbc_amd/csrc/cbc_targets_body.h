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
 *   reads, SAM   count and write passes in the shape of cbc_region_body.h / cbc_sam_body.h with the keep rule above; the
 *                bytes come from cbc_region_emit and cbc_sam_emit, which are called.
 *   depth        one contig per call.  The difference array lives in a COMPRESSED coordinate: the contig's intervals laid
 *                end to end with one spare slot behind each (sum of len + 1 words), `iv_off` the exclusive prefix of the
 *                slots.  mark: a lane walks the intervals its read overlaps (from the search result while beg <= the read's
 *                last base), clips the read to each and adds +1 at the piece's first slot, -1 at the slot behind its last
 *                one.  The spare slot therefore always has depth 0: no run crosses a gap, and intervals that were merged
 *                are one interval, so no run is cut inside them.  The tile, scan and compact passes of cbc_depth_body.h run
 *                on that array unchanged.  count / write: a change point is mapped back to its reference position by a
 *                binary search in iv_off; a run of non-zero depth lies inside one interval (or ends on its spare slot =
 *                the interval's end), so its end is start + the distance of the two change points.  Digit counts and
 *                digits are cbc_sam_ndig_v and cbc_depth_digit.
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

/* ---- reads ------------------------------------------------------------------------------------------------------------ */
template <class W>
CBC_FN void cbc_targets_count(const cbc_targets_args &A, uint32_t blk)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    const cbc_targets_blk T = cbc_targets_block(cbc_region_block(A.S.R, blk), A.S.R.window_start[blk], A.iv, A.block_iv, A.n_iv, blk);
    uint32_t kept = 0, bytes = 0;
    if (T.B.ok) {
        for (uint32_t r0 = 0; r0 < T.B.n; r0 += 64u) {
            V32 rlv, lp, fl, span, j;
            const Mask k = cbc_targets_keep<W>(T, r0, rlv, lp, fl, span, j);
            kept += W::reduce_add(W::select(k, W::splat(1u), W::splat(0u)));
            bytes += W::reduce_add(W::select(k, rlv + 1u, W::splat(0u)));
        }
    }
    uint32_t *c = (uint32_t *)(A.S.R.counts + blk);
    W::write_uni(c, 0u, bytes); W::write_uni(c, 1u, CBC_ST_OK); W::write_uni(c, 2u, kept); W::write_uni(c, 3u, 0u);
}

/* wavefront `wave` of `n_waves` writes every n_waves-th kept read of block blk (cbc_region_emit) */
template <class W>
CBC_FN void cbc_targets_write(const cbc_targets_args &A, uint32_t blk, uint32_t wave, uint32_t n_waves)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    const cbc_targets_blk T = cbc_targets_block(cbc_region_block(A.S.R, blk), A.S.R.window_start[blk], A.iv, A.block_iv, A.n_iv, blk);
    const uint32_t bytes = A.S.R.counts[blk].nbytes;
    const uint64_t o0 = A.S.R.offsets[blk];
    if (!T.B.ok || bytes == 0u || o0 > A.S.R.text_cap || bytes > A.S.R.text_cap - o0) return;
    uint64_t o = o0;
    uint32_t q = 0;                                                    /* kept reads of the block so far */
    for (uint32_t r0 = 0; r0 < T.B.n; r0 += 64u) {
        V32 rlv, lp, fl, span, j;
        const Mask k = cbc_targets_keep<W>(T, r0, rlv, lp, fl, span, j);
        const V32 tl = W::select(k, rlv + 1u, W::splat(0u));
        const V32 incl = W::scan_incl_add(tl);
        const uint32_t chunk = W::readlane(incl, 63u);
        if (chunk > (o0 + bytes) - o) return;                          /* the records changed under the count pass */
        uint64_t bits = W::ballot(k);
        while (bits) {
            const uint32_t i = W::ctz64(bits);
            bits &= bits - 1u;
            if ((q++ % n_waves) != wave) continue;
            const uint32_t rl = W::readlane(rlv, i), at = W::readlane(incl, i) - (rl + 1u);
            cbc_region_emit<W>(A.S.R.text, o + at, T.B.rows + (uint64_t)(r0 + i) * T.B.stride, rl);
        }
        o += chunk;
    }
}

/* ---- SAM --------------------------------------------------------------------------------------------------------------- */
template <class W>
CBC_FN void cbc_targets_sam_count(const cbc_targets_args &A, uint32_t blk)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    const cbc_sam_blk S = cbc_sam_block(A.S, blk);
    const cbc_targets_blk T = cbc_targets_block(S.B, A.S.R.window_start[blk], A.iv, A.block_iv, A.n_iv, blk);
    uint32_t kept = 0, bytes = 0;
    if (T.B.ok) {
        for (uint32_t r0 = 0; r0 < T.B.n; r0 += 64u) {
            V32 rlv, lp, fl, span, j;
            const Mask k = cbc_targets_keep<W>(T, r0, rlv, lp, fl, span, j);
            kept += W::reduce_add(W::select(k, W::splat(1u), W::splat(0u)));
            bytes += W::reduce_add(W::select(k, cbc_sam_line_len<W>(S, rlv, lp, fl), W::splat(0u)));
        }
    }
    uint32_t *c = (uint32_t *)(A.S.R.counts + blk);
    W::write_uni(c, 0u, bytes); W::write_uni(c, 1u, CBC_ST_OK); W::write_uni(c, 2u, kept); W::write_uni(c, 3u, 0u);
}

/* wavefront `wave` of `n_waves` writes every n_waves-th kept read of block blk (cbc_sam_emit) */
template <class W>
CBC_FN void cbc_targets_sam_write(const cbc_targets_args &A, uint32_t blk, uint32_t wave, uint32_t n_waves)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    const cbc_sam_blk S = cbc_sam_block(A.S, blk);
    const cbc_targets_blk T = cbc_targets_block(S.B, A.S.R.window_start[blk], A.iv, A.block_iv, A.n_iv, blk);
    const uint32_t bytes = A.S.R.counts[blk].nbytes;
    const uint64_t o0 = A.S.R.offsets[blk];
    if (!T.B.ok || bytes == 0u || o0 > A.S.R.text_cap || bytes > A.S.R.text_cap - o0) return;
    const V32 tabc = cbc_sam_const_tab<W>();
    uint64_t o = o0;
    uint32_t q = 0;                                                    /* kept reads of the block so far */
    for (uint32_t r0 = 0; r0 < T.B.n; r0 += 64u) {
        V32 rlv, lp, fl, span, j;
        const Mask k = cbc_targets_keep<W>(T, r0, rlv, lp, fl, span, j);
        const V32 tl = W::select(k, cbc_sam_line_len<W>(S, rlv, lp, fl), W::splat(0u));
        const V32 incl = W::scan_incl_add(tl);
        const uint32_t chunk = W::readlane(incl, 63u);
        if (chunk > (o0 + bytes) - o) return;                          /* the records changed under the count pass */
        uint64_t bits = W::ballot(k);
        while (bits) {
            const uint32_t i = W::ctz64(bits);
            bits &= bits - 1u;
            if ((q++ % n_waves) != wave) continue;
            const uint32_t len = W::readlane(tl, i), at = W::readlane(incl, i) - len;
            cbc_sam_emit<W>(A.S.R.text, o + at, T.B.rows + (uint64_t)(r0 + i) * T.B.stride, W::readlane(rlv, i),
                            S.ws + W::readlane(lp, i), W::readlane(fl, i), S.name, S.nl, len, tabc);
        }
        o += chunk;
    }
}

/* ---- depth: mark ------------------------------------------------------------------------------------------------------- */
/* STARTS (cbc_gpu_decode_coverage_ext, cbc_covx_body.h): per piece also +1 at its first slot in `starts`, an array as long as
 * the difference array */
template <class W, bool STARTS = false>
CBC_FN void cbc_targets_mark(const cbc_tdepth_args &A, uint32_t blk, uint32_t *starts = NULL)
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
    W::list_add(A.D.ctr, W::splat(0u), W::splat(kept), ln == 0u);
}

/* ---- depth: text ------------------------------------------------------------------------------------------------------- */
/* runs [j0, j0 + 64) of the contig's `nr` runs: start0, end0, depth and the line's length (0: no line) */
template <class W>
CBC_FN typename W::Mask cbc_targets_line(const cbc_tdepth_args &A, uint32_t j0, uint32_t nr, typename W::V32 &st,
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
CBC_FN void cbc_targets_depth_count(const cbc_tdepth_args &A, uint32_t tt)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    const uint32_t nr = cbc_depth_runs(A.D);
    uint32_t lines = 0, bytes = 0;
    if (A.D.name_len <= CBC_SAM_MAX_NAME && tt < A.D.n_ttiles)
        for (uint32_t r = 0; r < CBC_DEPTH_LINES / 64u; r++) {
            const uint32_t j0 = tt * CBC_DEPTH_LINES + r * 64u;
            if (j0 >= nr) break;
            V32 st, en, dp, len;
            const Mask k = cbc_targets_line<W>(A, j0, nr, st, en, dp, len);
            lines += W::popc64(W::ballot(k));
            bytes += W::reduce_add(len);
        }
    uint32_t *c = (uint32_t *)(A.D.R.counts + tt);
    W::write_uni(c, 0u, bytes); W::write_uni(c, 1u, CBC_ST_OK); W::write_uni(c, 2u, lines); W::write_uni(c, 3u, 0u);
    if (lines) W::list_add(A.D.ctr, W::splat(1u), W::splat(lines), W::lane() == 0u);
}

/* the lines of text tile tt, one lane per line, four bytes at a time: the scheme of cbc_depth_write */
template <class W>
CBC_FN void cbc_targets_depth_write(const cbc_tdepth_args &A, uint32_t tt)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    if (tt >= A.D.n_ttiles || A.D.name_len > CBC_SAM_MAX_NAME) return;
    const uint32_t nr = cbc_depth_runs(A.D);
    const uint32_t bytes = A.D.R.counts[tt].nbytes, nl = A.D.name_len;
    const uint64_t o0 = A.D.R.offsets[tt];
    if (bytes == 0u || o0 > A.D.R.text_cap || bytes > A.D.R.text_cap - o0) return;
    uint64_t o = o0;
    for (uint32_t r = 0; r < CBC_DEPTH_LINES / 64u; r++) {
        const uint32_t j0 = tt * CBC_DEPTH_LINES + r * 64u;
        if (j0 >= nr) break;
        V32 st, en, dp, len;
        const Mask k = cbc_targets_line<W>(A, j0, nr, st, en, dp, len);
        const V32 incl = W::scan_incl_add(len);
        const uint32_t chunk = W::readlane(incl, 63u);
        if (chunk > (o0 + bytes) - o) return;                        /* the change points moved under the count pass */
        if (chunk == 0u) continue;
        const V32 at = incl - len;
        /* the line: name, '\t' at nl, start0, '\t' at e1, end0, '\t' at e2, depth, '\n' at e3 = len - 1 */
        const V32 e1 = cbc_sam_ndig_v<W>(st, 1000000000u) + (nl + 1u);
        const V32 e2 = e1 + cbc_sam_ndig_v<W>(en, 1000000000u) + 1u;
        const V32 e3 = len - 1u;
        V32 sh, sl, eh, el, dh, dl;
        cbc_depth_split<W>(st, sh, sl); cbc_depth_split<W>(en, eh, el); cbc_depth_split<W>(dp, dh, dl);
        uint8_t *dst = A.D.R.text + o;
        const uint32_t maxlen = W::readlane(W::scan_incl_max(len), 63u);
        for (uint32_t q = 0; q < maxlen; q += 4u) {
            V32 out = W::splat(0u);
            for (uint32_t t = 0; t < 4u; t++) {
                const uint32_t i = q + t;
                V32 by;
                if (i < nl) by = W::splat(W::read_uni8(A.D.name, i));
                else {
                    const V32 iv = W::splat(i);
                    const Mask f1 = iv < e1, f2 = iv < e2;
                    const V32 hi = W::select(f1, sh, W::select(f2, eh, dh)), lo = W::select(f1, sl, W::select(f2, el, dl));
                    const V32 d = (W::select(f1, e1, W::select(f2, e2, e3)) - 1u) - iv;
                    by = cbc_depth_digit<W>(hi, lo, d);
                    by = W::select((iv == nl) | (iv == e1) | (iv == e2), W::splat(9u), by);
                    by = W::select(iv == e3, W::splat(10u), by);
                }
                out = out | (by << (8u * t));
            }
            const Mask full = k & (W::splat(q + 4u) <= len);
            W::store32_bytes(dst, at + q, out, full);
            const Mask part = k & !full & (W::splat(q) < len);
            if (W::ballot(part) != 0ull)
                for (uint32_t t = 0; t < 3u; t++)
                    W::store8(dst, at + (q + t), (out >> (8u * t)) & 0xffu, part & (W::splat(q + t) < len));
        }
        o += chunk;
    }
}

#endif /* CBC_TARGETS_BODY_H */
