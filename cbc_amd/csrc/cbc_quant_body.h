/*
 * cbc_quant_body.h -- per-query depth quantiles on the device, beside the coverage summary of cbc_cov_body.h and the thresholds of
 * cbc_covx_body.h (cbc_gpu_decode_coverage_quant, include/cbc_gpu.h).  ONE contig's compressed coordinate
 * per call.
 *
 * Definition.  The depths of the len >= 1 positions of a query, sorted ascending, are d(0) <= ... <= d(len - 1); for an integer
 * percentage p in 0..100 the result is d(k - 1) with k = max(1, ceil(p * len / 100)): the nearest-rank ("lower") quantile, p = 0
 * the minimum, p = 50 the lower median, p = 100 the maximum.  With len = 100 a + b, k = p a + ceil(p b / 100) stays in 32 bits.
 * A query of no position gives 0.
 *
 * A quantile is no difference of prefix sums: it is a selection over the runs of the query.  ONE WAVEFRONT PER QUERY, all
 * quantiles (up to CBC_QUANT_MAX) in one go:
 *   runs      two cbc_targets_find (every lane the same key) give the first run that reaches the query and the last one that
 *             starts inside it; each run is clipped to [slot, slot + len).  Change point ncp - 1 starts no run; in front of the
 *             first change point and behind the last one the depth is 0.  The zero-depth positions are len - sum of the clipped
 *             lengths of the runs of depth != 0: nobody walks them.
 *   register  at most 64 runs: one lane holds one run as (depth, clipped length).  The value of rank k is the smallest v with
 *             zeros + sum(length where 0 < depth <= v) >= k, found by bisection over [0, max depth of the query]; a step is one
 *             compare, one select and one reduce_add.  No memory traffic after the first load.
 *   table     more than 64 runs: the runs are streamed 64 at a time in one pass; lengths of depths below CBC_QUANT_LDS go into
 *             a table in LDS that the wavefront owns (bin 0 gets the zeros), the total length at or above CBC_QUANT_LDS into one
 *             tail counter, and the maximum depth is kept.  The table is then scanned 64 bins per round with scan_incl_add and a
 *             running carry until the cumulative count has reached every k below the tail.  Only a k that lands in the tail is
 *             bisected over [CBC_QUANT_LDS, max depth], one more streaming pass per step.
 * Every count is at most len <= slots < 2^32.  Control flow is wave-uniform (the queries' words and the results of the finds are
 * read back into scalars), lane 0 stores the n_quant words of the query, range tests are written without base + length sums.
 * Written against the wave policy (W = WaveGPU in cbc_gpu.hip, the lock-step emulation in tests/quant_emu).
 */
#ifndef CBC_QUANT_BODY_H
#define CBC_QUANT_BODY_H

#include <stdint.h>
#include "../../include/cbc_gpu.h"
#include "cbc_cov_body.h"
#include "cbc_hist_body.h"         /* CBC_HIST_LDS */

#define CBC_QUANT_LDS CBC_HIST_LDS /* bins of the wavefront's LDS table: 16 rounds of 64 lanes */
#ifdef __HIP_DEVICE_COMPILE__
#define CBC_QUANT_UNROLL _Pragma("unroll")
#else
#define CBC_QUANT_UNROLL
#endif

struct cbc_quant_args {
    const uint32_t *cp_pos, *cp_dep;                     /* the change points                                                   */
    const uint64_t *cnt_off;                             /* cnt_off[n_tiles] = how many there are                               */
    const uint32_t *q;                                   /* n_q pairs slot, len                                                 */
    uint32_t *quant;                                     /* n_q * n_quant, query-major                                          */
    uint32_t pct[CBC_QUANT_MAX];                         /* the percentages, 0..100                                             */
    uint32_t n_quant, cp_cap, n_tiles, n_q, slots, reserved;
};

/* the rank of percentage p among len >= 1 values: max(1, ceil(p len / 100)) without a 32-bit overflow (p <= 100) */
CBC_FN uint32_t cbc_quant_rank(uint32_t p, uint32_t len)
{
    const uint32_t a = len / 100u, b = len % 100u;
    const uint32_t k = p * a + (p * b + 99u) / 100u;
    return k ? k : 1u;
}

/* runs [j0, j0 + 64) of the query's runs [.., j1), clipped to [slot, end): depth and clipped length; a lane past j1, or whose
 * clipped run is empty, gets length 0.  j1 <= ncp - 1, so every run loaded exists. */
template <class W>
CBC_FN void cbc_quant_runs(const cbc_quant_args &A, uint32_t j0, uint32_t j1, uint32_t slot, uint32_t end, typename W::V32 &d,
                           typename W::V32 &cl)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    const V32 j = W::lane() + j0;                                    /* j1 <= cp_cap < 2^32 - 64: no wrap */
    const Mask m = j < j1;
    const V32 p = W::load32(A.cp_pos, j, m, 0u), q = W::load32(A.cp_pos, j + 1u, m, 0u);
    d = W::load32(A.cp_dep, j, m, 0u);
    const V32 lo = W::select(p < slot, W::splat(slot), p), hi = W::select(q > end, W::splat(end), q);
    cl = W::select(m & (hi > lo), hi - lo, W::splat(0u));
}

/* query i; lds: CBC_QUANT_LDS words of this wavefront */
template <class W>
CBC_FN void cbc_quant_select(const cbc_quant_args &A, uint32_t i, uint32_t *lds)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    if (i >= A.n_q || A.n_quant == 0u || A.n_quant > CBC_QUANT_MAX) return;
    const uint32_t slot = W::read_uni(A.q, 2u * i), len = W::read_uni(A.q, 2u * i + 1u);
    uint32_t *out = A.quant + (uint64_t)i * A.n_quant;
    uint32_t res[CBC_QUANT_MAX], k[CBC_QUANT_MAX];
CBC_QUANT_UNROLL
    for (uint32_t t = 0; t < CBC_QUANT_MAX; t++) { res[t] = 0u; k[t] = 1u; }
    const bool ok = slot <= A.slots && len <= A.slots - slot && len != 0u;
    const uint32_t ncp = cbc_depth_points(A.cnt_off, A.n_tiles, A.cp_cap);
    uint32_t j0 = 0u, j1 = 0u;
    const uint32_t end = slot + len;                                 /* <= A.slots under ok */
    if (ok && ncp >= 2u) {
        /* ka = change points at or below slot, kb = change points below end (>= ka: end > slot) */
        const uint32_t ka = W::readlane(cbc_targets_find<W>(A.cp_pos, 1u, ncp, W::splat(slot + 1u), W::all()), 0u);
        const uint32_t kb = W::readlane(cbc_targets_find<W>(A.cp_pos, 1u, ncp, W::splat(end), W::all()), 0u);
        j0 = ka ? ka - 1u : 0u;                                      /* the run that holds slot, or the first one of all */
        j1 = kb < ncp - 1u ? kb : ncp - 1u;                          /* behind the last run that starts inside; ncp - 1 starts none */
        if (j1 < j0) j1 = j0;
    }
    const uint32_t nruns = j1 - j0;
    if (ok && nruns != 0u) {
CBC_QUANT_UNROLL
        for (uint32_t t = 0; t < CBC_QUANT_MAX; t++) if (t < A.n_quant) k[t] = cbc_quant_rank(A.pct[t], len);
        if (nruns <= 64u) {
            /* ---- register form ---- */
            V32 d, cl;
            cbc_quant_runs<W>(A, j0, j1, slot, end, d, cl);
            const Mask nz = (d != 0u);
            cl = W::select(nz, cl, W::splat(0u));
            const uint32_t zeros = len - W::reduce_add(cl);
            const uint32_t dmax = W::readlane(W::scan_incl_max(W::select(cl != 0u, d, W::splat(0u))), 63u);
CBC_QUANT_UNROLL
            for (uint32_t t = 0; t < CBC_QUANT_MAX; t++)
                if (t < A.n_quant && k[t] > zeros) {
                    uint32_t lo = 1u, hi = dmax;                     /* the answer is a depth in [1, dmax]: count(dmax) = len >= k */
                    while (lo < hi) {
                        const uint32_t mid = lo + ((hi - lo) >> 1);
                        const uint32_t c = zeros + W::reduce_add(W::select(d <= mid, cl, W::splat(0u)));
                        if (c >= k[t]) hi = mid; else lo = mid + 1u;
                    }
                    res[t] = lo;
                }
        } else {
            /* ---- table form ---- */
            const V32 ln = W::lane();
            for (uint32_t r = 0; r < CBC_QUANT_LDS / 64u; r++) W::lds_zero(lds, ln + r * 64u, W::all());
            V32 vtail = W::splat(0u), vlow = W::splat(0u), vmax = W::splat(0u);
            for (uint32_t j = j0; j < j1; j += 64u) {                /* j1 + 64 < 2^32 */
                V32 d, cl;
                cbc_quant_runs<W>(A, j, j1, slot, end, d, cl);
                const Mask live = (d != 0u) & (cl != 0u), low = live & (d < CBC_QUANT_LDS);
                W::lds_add(lds, d, cl, low);
                vlow = vlow + W::select(low, cl, W::splat(0u));
                vtail = vtail + W::select(live & !low, cl, W::splat(0u));
                vmax = W::select(live & (d > vmax), d, vmax);
            }
            const uint32_t tail = W::reduce_add(vtail), zeros = (len - tail) - W::reduce_add(vlow);
            const uint32_t dmax = W::readlane(W::scan_incl_max(vmax), 63u);
            W::lds_add(lds, W::splat(0u), W::splat(zeros), ln == 0u);       /* bin 0: the positions no run of depth != 0 holds */
            const uint32_t below = len - tail;                       /* positions with a depth below CBC_QUANT_LDS */
            uint32_t carry = 0u, t0 = 0u, nb = 0u;                   /* the k ascend with the percentages: t0 = the next one to find, */
CBC_QUANT_UNROLL
            for (uint32_t t = 0; t < CBC_QUANT_MAX; t++) if (t < A.n_quant && k[t] <= below) nb++;     /* nb = those below the tail */
            for (uint32_t r = 0; r < CBC_QUANT_LDS / 64u; r++) {
                if (t0 >= nb) break;
                const V32 v = W::lds_read(lds, ln + r * 64u, W::all());
                const V32 inc = W::scan_incl_add(v) + carry;
                const uint32_t upto = W::readlane(inc, 63u);
CBC_QUANT_UNROLL
                for (uint32_t t = 0; t < CBC_QUANT_MAX; t++)
                    if (t < A.n_quant && t == t0 && k[t] <= upto) {
                        res[t] = r * 64u + W::ctz64(W::ballot(inc >= k[t]));
                        t0 = t + 1u;
                    }
                carry = upto;
            }
CBC_QUANT_UNROLL
            for (uint32_t t = 0; t < CBC_QUANT_MAX; t++)
                if (t < A.n_quant && k[t] > below) {                 /* in the tail: bisect, a streaming pass per step */
                    uint32_t lo = CBC_QUANT_LDS, hi = dmax;
                    while (lo < hi) {
                        const uint32_t mid = lo + ((hi - lo) >> 1);
                        V32 acc = W::splat(0u);
                        for (uint32_t j = j0; j < j1; j += 64u) {
                            V32 d, cl;
                            cbc_quant_runs<W>(A, j, j1, slot, end, d, cl);
                            acc = acc + W::select((d >= CBC_QUANT_LDS) & (d <= mid), cl, W::splat(0u));
                        }
                        const uint32_t c = below + W::reduce_add(acc);
                        if (c >= k[t]) hi = mid; else lo = mid + 1u;
                    }
                    res[t] = lo;
                }
        }
    }
CBC_QUANT_UNROLL
    for (uint32_t t = 0; t < CBC_QUANT_MAX; t++) if (t < A.n_quant) W::write_uni(out, t, res[t]);
}

#endif /* CBC_QUANT_BODY_H */
