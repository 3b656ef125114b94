/*
 * cbc_covx_body.h -- per-query read counts and depth thresholds on the device, beside the coverage summary of cbc_cov_body.h
 * (cbc_gpu_decode_coverage_ext, include/cbc_gpu.h).  ONE contig's compressed coordinate per call.
 *
 * Read counts.  A query [x, x + len) lies inside one merged interval and a kept read has at most one piece per interval, so
 *     reads = depth(x) + CS(x + len - 1) - CS(x)            CS(y) = pieces whose clipped first slot is <= y
 * (the pieces that start at or below x and still reach x are depth(x); those that start inside (x, x + len - 1] overlap; pieces
 * of other intervals do neither).  The mark pass of the call (cbc_targets_mark<W, true>, cbc_targets_body.h) adds +1 per piece at
 * its first slot into a second array, `starts`; cbc_depth_tile, the size scans and cbc_depth_compact run over it unchanged and
 * leave the START POINTS (sp_pos[j], sp_cnt[j]) = (slot, CS(slot)), ascending, CS modulo 2^32 -- a difference of two of them is
 * exact while the true count fits 32 bits (a call holds fewer than 2^30 reads).
 *
 * Thresholds.  For T <= CBC_COVX_MAX_THR depths thr[0] < thr[1] < ..., C_t(x) = slots below x with depth >= thr[t]:
 *   weights  one wavefront per CBC_DEPTH_LINES runs, one lane per run, ONE pass for all T: c_t = length when depth >= thr[t];
 *            the tile's T totals each into a cbc_block_result (tile_thr[t * n_ttiles + tile]) for cbc_scan_sizes_kernel.
 *   apply    the same tile again: per change point the exclusive prefix pre_thr[t * cp_cap + j] = C_t at cp_pos[j].
 *   lookup   one lane per query: the last change point at or below x = slot and x = slot + len (two cbc_targets_find, shared by
 *            all T and by depth(x)), C_t(x) = pre_thr[t][j] + (x - cp_pos[j] when the run's depth >= thr[t]), the partial run
 *            as cbc_cov_prefix takes pre_cov; then the two finds on the start points for the read count.
 * The loops over t are unrolled over CBC_COVX_MAX_THR with a wave-uniform t < n_thr in front of every reduction, scan and
 * store, so that the accumulators stay in registers.  Range tests are written without base + length sums.  Written against the
 * wave policy (W = WaveGPU in cbc_gpu.hip, the lock-step emulation in tests/covx_emu).
 */
#ifndef CBC_COVX_BODY_H
#define CBC_COVX_BODY_H

#include <stdint.h>
#include "../../include/cbc_gpu.h"
#include "cbc_cov_body.h"

#define CBC_COVX_MAX_THR 8u
#ifdef __HIP_DEVICE_COMPILE__
#define CBC_COVX_UNROLL _Pragma("unroll")
#else
#define CBC_COVX_UNROLL
#endif

struct cbc_covx_args {
    const uint32_t *cp_pos, *cp_dep;                     /* the change points                                                   */
    const uint64_t *cnt_off;                             /* cnt_off[n_tiles] = how many there are                               */
    const uint32_t *sp_pos, *sp_cnt;                     /* the start points (reads != NULL)                                    */
    const uint64_t *sp_off;                              /* sp_off[n_tiles] = how many there are                                */
    cbc_block_result *tile_thr;                          /* n_thr * n_ttiles: per threshold and tile of runs, the total (nbytes) */
    const uint64_t *thr_off;                             /* n_thr * (n_ttiles + 1): their exclusive scans                       */
    uint32_t *pre_thr;                                   /* n_thr * cp_cap: C_t at every change point                           */
    const uint32_t *q;                                   /* n_q pairs slot, len                                                 */
    uint32_t *thr_covered;                               /* n_q * n_thr, query-major                                            */
    uint32_t *reads;                                     /* n_q, or NULL: no read counts                                        */
    uint32_t thr[CBC_COVX_MAX_THR];
    uint32_t n_thr, cp_cap, sp_cap, n_tiles, n_ttiles, n_q;
    uint32_t slots, reserved;
};

/* runs [j0, j0 + 64): depth and length; a lane whose run does not exist (j + 1 >= ncp) gets length 0 */
template <class W>
CBC_FN void cbc_covx_runs(const cbc_covx_args &A, uint32_t j0, uint32_t ncp, typename W::V32 &d, typename W::V32 &len)
{
    const typename W::Mask m = cbc_depth_run_load<W>(A.cp_pos, A.cp_dep, j0, ncp, d, len);
    len = W::select(m, len, W::splat(0u));
}

template <class W>
CBC_FN void cbc_covx_weights(const cbc_covx_args &A, uint32_t tt)
{
    typedef typename W::V32 V32;
    if (tt >= A.n_ttiles || A.n_thr > CBC_COVX_MAX_THR) return;
    const uint32_t ncp = cbc_depth_points(A.cnt_off, A.n_tiles, A.cp_cap);
    V32 ac[CBC_COVX_MAX_THR];
CBC_COVX_UNROLL
    for (uint32_t t = 0; t < CBC_COVX_MAX_THR; t++) ac[t] = W::splat(0u);
    for (uint32_t r = 0; r < CBC_DEPTH_LINES / 64u; r++) {
        const uint32_t j0 = tt * CBC_DEPTH_LINES + r * 64u;
        if (j0 >= ncp || ncp - j0 < 2u) break;                       /* no run from j0 on */
        V32 d, len;
        cbc_covx_runs<W>(A, j0, ncp, d, len);
CBC_COVX_UNROLL
        for (uint32_t t = 0; t < CBC_COVX_MAX_THR; t++)
            if (t < A.n_thr) ac[t] = ac[t] + W::select(d >= A.thr[t], len, W::splat(0u));
    }
CBC_COVX_UNROLL
    for (uint32_t t = 0; t < CBC_COVX_MAX_THR; t++)
        if (t < A.n_thr)
            cbc_store_result<W>(A.tile_thr + ((uint64_t)t * A.n_ttiles + tt), W::reduce_add(ac[t]), 0u);
}

template <class W>
CBC_FN void cbc_covx_apply(const cbc_covx_args &A, uint32_t tt)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    if (tt >= A.n_ttiles || A.n_thr > CBC_COVX_MAX_THR) return;
    const uint32_t ncp = cbc_depth_points(A.cnt_off, A.n_tiles, A.cp_cap);
    uint32_t crun[CBC_COVX_MAX_THR];
CBC_COVX_UNROLL
    for (uint32_t t = 0; t < CBC_COVX_MAX_THR; t++)
        crun[t] = t < A.n_thr ? (uint32_t)A.thr_off[(uint64_t)t * (A.n_ttiles + 1u) + tt] : 0u;     /* C_t in front of the tile */
    for (uint32_t r = 0; r < CBC_DEPTH_LINES / 64u; r++) {
        const uint32_t j0 = tt * CBC_DEPTH_LINES + r * 64u;
        if (j0 >= ncp) break;
        V32 d, len;
        cbc_covx_runs<W>(A, j0, ncp, d, len);
        const V32 j = W::lane() + j0;
        const Mask m = j < ncp;
CBC_COVX_UNROLL
        for (uint32_t t = 0; t < CBC_COVX_MAX_THR; t++)
            if (t < A.n_thr) {
                const V32 c = W::select(d >= A.thr[t], len, W::splat(0u));
                const V32 ic = W::scan_incl_add(c);
                W::store32(A.pre_thr + (uint64_t)t * A.cp_cap, j, (ic - c) + crun[t], m);
                crun[t] += W::readlane(ic, 63u);
            }
    }
}

/* queries [64 w, 64 w + 64) */
template <class W>
CBC_FN void cbc_covx_lookup(const cbc_covx_args &A, uint32_t w)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    if (A.n_thr > CBC_COVX_MAX_THR) return;
    const V32 i = W::lane() + w * 64u;                               /* n_q <= 2^24 */
    const Mask m = i < A.n_q;
    const V32 slot = W::load32(A.q, i * 2u, m, 0u), len = W::load32(A.q, i * 2u + 1u, m, 0u);
    const Mask ok = m & (slot <= A.slots) & (len <= A.slots - slot);
    const uint32_t ncp = cbc_depth_points(A.cnt_off, A.n_tiles, A.cp_cap);
    /* the last change point at or below x = slot (a) and x = slot + len (b): k = change points with cp_pos <= x */
    const V32 end = slot + len;                                      /* <= A.slots under ok */
    const V32 ka = cbc_targets_find<W>(A.cp_pos, 1u, ncp, slot + 1u, ok), kb = cbc_targets_find<W>(A.cp_pos, 1u, ncp, end + 1u, ok);
    const Mask ha = ok & (ka != 0u), hb = ok & (kb != 0u);          /* in front of the first change point: 0 */
    const Mask hra = ha & (ka < ncp), hrb = hb & (kb < ncp);         /* behind the last one the depth is 0   */
    const V32 ja = ka - 1u, jb = kb - 1u;
    const V32 da = W::load32(A.cp_dep, ja, hra, 0u), db = W::load32(A.cp_dep, jb, hrb, 0u);
    const V32 dxa = slot - W::load32(A.cp_pos, ja, ha, 0u), dxb = end - W::load32(A.cp_pos, jb, hb, 0u);
CBC_COVX_UNROLL
    for (uint32_t t = 0; t < CBC_COVX_MAX_THR; t++)
        if (t < A.n_thr) {
            const uint32_t *pre = A.pre_thr + (uint64_t)t * A.cp_cap;
            const V32 ca = W::load32(pre, ja, ha, 0u) + W::select(hra & (da >= A.thr[t]), dxa, W::splat(0u));
            const V32 cb = W::load32(pre, jb, hb, 0u) + W::select(hrb & (db >= A.thr[t]), dxb, W::splat(0u));
            W::store32(A.thr_covered, i * A.n_thr + t, cb - ca, m);
        }
    if (A.reads) {
        const uint32_t nsp = cbc_depth_points(A.sp_off, A.n_tiles, A.sp_cap);
        const Mask one = ok & (len != 0u);
        /* CS(y) = sp_cnt of the last start point with sp_pos <= y, 0 in front of the first one */
        const V32 sa = cbc_targets_find<W>(A.sp_pos, 1u, nsp, slot + 1u, one), sb = cbc_targets_find<W>(A.sp_pos, 1u, nsp, end, one);
        const V32 csa = W::load32(A.sp_cnt, sa - 1u, one & (sa != 0u), 0u), csb = W::load32(A.sp_cnt, sb - 1u, one & (sb != 0u), 0u);
        W::store32(A.reads, i, W::select(one, da + (csb - csa), W::splat(0u)), m);
    }
}

#endif /* CBC_COVX_BODY_H */
