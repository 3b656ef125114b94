/*
 * cbc_cov_body.h -- per-query coverage summary on the device, after the depth passes of a target set have left the change
 * points of ONE contig's compressed coordinate (cbc_gpu_decode_coverage, include/cbc_gpu.h).
 *
 * The change points (cp_pos[j], cp_dep[j]), j < ncp, are what cbc_depth_compact wrote for the difference array of
 * cbc_targets_mark: run j = slots [cp_pos[j], cp_pos[j + 1]) has depth cp_dep[j]; in front of the first change point and behind
 * the last one the depth is 0.  A query is a slot range [slot, slot + len) inside one merged interval.  With
 *     S(x) = sum of the depth over the slots below x          C(x) = slots below x with depth >= min_depth (min_depth >= 1)
 * a query's sum is S(slot + len) - S(slot) and its covered count C(slot + len) - C(slot).
 *
 *   weights  one wavefront per CBC_DEPTH_LINES runs, one lane per run: w = depth * length as 64 bits (v_mul_lo / v_mul_hi),
 *            c = length when depth >= min_depth; the tile's totals -- low word of w, high word of w, c -- each into a
 *            cbc_block_result, so that cbc_scan_sizes_kernel (32-bit items, 64-bit sums) scans them: the 64-bit prefix is
 *            scan(low words) + (scan(high words) << 32).  Reduce, scan, apply: no wavefront waits for another.
 *   apply    the same tile again: the prefix inside the tile + the carry, stored per change point as the exclusive prefixes
 *            pre_lo / pre_hi (S at cp_pos[j]) and pre_cov (C at cp_pos[j]); the last change point gets the totals.
 *   lookup   one lane per query: for x = slot and x = slot + len the last change point with cp_pos <= x by a per-lane binary
 *            search with a wave-uniform trip count (cbc_targets_find), S(x) = pre[j] + cp_dep[j] * (x - cp_pos[j]).
 * The policy's vectors are 32 bits wide: a 64-bit value is a pair of them, added with the carry taken from an unsigned compare;
 * a wave-wide sum or prefix of 64-bit lanes goes through three 32-bit ones (the low word's two 16-bit halves cannot overflow
 * over 64 lanes, the high word is exact modulo 2^32 because the true totals fit 64 bits: depth < 2^32, slots < 2^32).
 * Range tests are written without base + length sums.  Written against the wave policy (W = WaveGPU in cbc_gpu.hip, the
 * lock-step emulation in tests/cov_emu).
 */
#ifndef CBC_COV_BODY_H
#define CBC_COV_BODY_H

#include <stdint.h>
#include "../../include/cbc_gpu.h"
#include "cbc_depth_body.h"
#include "cbc_targets_body.h"      /* cbc_targets_find */

struct cbc_cov_args {
    const uint32_t *cp_pos, *cp_dep;                     /* the change points                                                   */
    const uint64_t *cnt_off;                             /* cnt_off[n_tiles] = how many there are (cbc_depth_args.cnt_off)      */
    cbc_block_result *tile_wlo, *tile_whi, *tile_cov;    /* per tile of CBC_DEPTH_LINES runs: the totals (nbytes)               */
    const uint64_t *wlo_off, *whi_off, *cov_off;         /* their exclusive scans (n_ttiles + 1)                                */
    uint32_t *pre_lo, *pre_hi, *pre_cov;                 /* per change point: S and C at its position                           */
    const uint32_t *q;                                   /* n_q pairs slot, len                                                 */
    uint32_t *sum;                                       /* n_q pairs low word, high word                                       */
    uint32_t *covered;                                   /* n_q                                                                 */
    uint32_t cp_cap, n_tiles, n_ttiles, n_q, min_depth;
    uint32_t slots;                                      /* slots of the compressed coordinate: no query reaches past them      */
};

/* runs [j0, j0 + 64): weight (two words) and covered slots; a lane whose run does not exist (j + 1 >= ncp) gets zeros */
template <class W>
CBC_FN void cbc_cov_runs(const cbc_cov_args &A, uint32_t j0, uint32_t ncp, typename W::V32 &wlo, typename W::V32 &whi,
                         typename W::V32 &cov)
{
    typename W::V32 d, len;
    const typename W::Mask m = cbc_depth_run_load<W>(A.cp_pos, A.cp_dep, j0, ncp, d, len);
    wlo = d * len;
    whi = W::mulhi(d, len);
    cov = W::select(m & (d >= A.min_depth), len, W::splat(0u));
}

template <class W>
CBC_FN typename W::V32 cbc_cov_carry(const typename W::V32 &sum, const typename W::V32 &addend)
{
    return W::select(sum < addend, W::splat(1u), W::splat(0u));
}

template <class W>
CBC_FN void cbc_cov_weights(const cbc_cov_args &A, uint32_t tt)
{
    typedef typename W::V32 V32;
    const uint32_t ncp = cbc_depth_points(A.cnt_off, A.n_tiles, A.cp_cap);
    V32 alo = W::splat(0u), ahi = W::splat(0u), ac = W::splat(0u);
    if (tt < A.n_ttiles)
        for (uint32_t r = 0; r < CBC_DEPTH_LINES / 64u; r++) {
            const uint32_t j0 = tt * CBC_DEPTH_LINES + r * 64u;
            if (j0 >= ncp || ncp - j0 < 2u) break;                   /* no run from j0 on */
            V32 wlo, whi, cov;
            cbc_cov_runs<W>(A, j0, ncp, wlo, whi, cov);
            alo = alo + wlo;
            ahi = ahi + whi + cbc_cov_carry<W>(alo, wlo);
            ac = ac + cov;
        }
    const uint64_t tot = (uint64_t)W::reduce_add(alo & 0xffffu) + ((uint64_t)W::reduce_add(alo >> 16) << 16) +
                         ((uint64_t)W::reduce_add(ahi) << 32);
    cbc_store_result<W>(A.tile_wlo + tt, (uint32_t)tot, 0u);
    cbc_store_result<W>(A.tile_whi + tt, (uint32_t)(tot >> 32), 0u);
    cbc_store_result<W>(A.tile_cov + tt, W::reduce_add(ac), 0u);
}

template <class W>
CBC_FN void cbc_cov_apply(const cbc_cov_args &A, uint32_t tt)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    if (tt >= A.n_ttiles) return;
    const uint32_t ncp = cbc_depth_points(A.cnt_off, A.n_tiles, A.cp_cap);
    uint64_t run = A.wlo_off[tt] + (A.whi_off[tt] << 32);           /* S in front of the tile */
    uint32_t crun = (uint32_t)A.cov_off[tt];
    for (uint32_t r = 0; r < CBC_DEPTH_LINES / 64u; r++) {
        const uint32_t j0 = tt * CBC_DEPTH_LINES + r * 64u;
        if (j0 >= ncp) break;
        V32 wlo, whi, cov;
        cbc_cov_runs<W>(A, j0, ncp, wlo, whi, cov);
        const V32 l0 = wlo & 0xffffu, l1 = wlo >> 16;
        const V32 i0 = W::scan_incl_add(l0), i1 = W::scan_incl_add(l1), ih = W::scan_incl_add(whi), ic = W::scan_incl_add(cov);
        /* the exclusive prefix inside the round: 16 bits at a time, e0 and e1 stay below 2^23 */
        const V32 e0 = i0 - l0, e1 = (i1 - l1) + (e0 >> 16), eh = (ih - whi) + (e1 >> 16);
        const V32 elo = (e0 & 0xffffu) | (e1 << 16);
        const uint32_t rl = (uint32_t)run, rh = (uint32_t)(run >> 32);
        const V32 lo = elo + rl, hi = eh + rh + cbc_cov_carry<W>(lo, W::splat(rl));
        const V32 j = W::lane() + j0;
        const Mask m = j < ncp;
        W::store32(A.pre_lo, j, lo, m); W::store32(A.pre_hi, j, hi, m); W::store32(A.pre_cov, j, (ic - cov) + crun, m);
        run += (uint64_t)W::readlane(i0, 63u) + ((uint64_t)W::readlane(i1, 63u) << 16) + ((uint64_t)W::readlane(ih, 63u) << 32);
        crun += W::readlane(ic, 63u);
    }
}

/* S(x) as two words and C(x), per lane under m (x <= A.slots); lanes outside m get zeros */
template <class W>
CBC_FN void cbc_cov_prefix(const cbc_cov_args &A, uint32_t ncp, const typename W::V32 &x, const typename W::Mask &m,
                           typename W::V32 &slo, typename W::V32 &shi, typename W::V32 &sc)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    /* k = change points at or below x: the first one with cp_pos >= x + 1 (x < 2^32 - 1) */
    const V32 k = cbc_targets_find<W>(A.cp_pos, 1u, ncp, x + 1u, m);
    const Mask h = m & (k != 0u);                                    /* in front of the first change point: 0 */
    const Mask hr = h & (k < ncp);                                   /* behind the last one the depth is 0   */
    const V32 j = k - 1u;
    const V32 p = W::load32(A.cp_pos, j, h, 0u), d = W::load32(A.cp_dep, j, hr, 0u);
    const V32 plo = W::load32(A.pre_lo, j, h, 0u), phi = W::load32(A.pre_hi, j, h, 0u), pc = W::load32(A.pre_cov, j, h, 0u);
    const V32 dx = x - p;
    const V32 mlo = d * dx, mhi = W::mulhi(d, dx);
    slo = plo + mlo;
    shi = phi + mhi + cbc_cov_carry<W>(slo, mlo);
    sc = pc + W::select(hr & (d >= A.min_depth), dx, W::splat(0u));
}

/* queries [64 w, 64 w + 64) */
template <class W>
CBC_FN void cbc_cov_lookup(const cbc_cov_args &A, uint32_t w)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    const V32 i = W::lane() + w * 64u;                               /* n_q <= 2^24 */
    const Mask m = i < A.n_q;
    const V32 slot = W::load32(A.q, i * 2u, m, 0u), len = W::load32(A.q, i * 2u + 1u, m, 0u);
    const Mask ok = m & (slot <= A.slots) & (len <= A.slots - slot);
    const uint32_t ncp = cbc_depth_points(A.cnt_off, A.n_tiles, A.cp_cap);
    V32 alo, ahi, ac, blo, bhi, bc;
    cbc_cov_prefix<W>(A, ncp, slot, ok, alo, ahi, ac);
    cbc_cov_prefix<W>(A, ncp, slot + len, ok, blo, bhi, bc);        /* <= A.slots under ok */
    const V32 borrow = W::select(blo < alo, W::splat(1u), W::splat(0u));
    W::store32(A.sum, i * 2u, blo - alo, m);
    W::store32(A.sum, i * 2u + 1u, (bhi - ahi) - borrow, m);
    W::store32(A.covered, i, bc - ac, m);
}

#endif /* CBC_COV_BODY_H */
