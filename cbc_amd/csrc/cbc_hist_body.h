/*
 * cbc_hist_body.h -- depth histogram on the device, after the depth passes of a target set have left the change points of ONE
 * contig's compressed coordinate (cbc_gpu_decode_depth_hist, include/cbc_gpu.h).
 *
 * The change points (cp_pos[j], cp_dep[j]), j < ncp, are what cbc_depth_compact wrote for the difference array of
 * cbc_targets_mark: run j = slots [cp_pos[j], cp_pos[j + 1]) has depth cp_dep[j].  The histogram adds every run's length to the
 * bin of its depth; depths at or above `fold` (max_depth, 2^32 - 1 when there is none) share bin `fold`.  Runs of depth 0 are
 * left out: the depth-0 bin is the caller's size - sum of the others, which also keeps the spare slot behind every interval out
 * of the count (a run of non-zero depth never holds one: reads are clipped to their interval, so the -1 of the last read lands
 * on the spare slot at the latest).
 *
 * The bin table has n_bins = min(fold, K) + 1 words for the K reads of the call (a depth cannot pass K), rounded up to whole
 * tiles and zeroed before.  A bin is 32 bits: its value is at most the slots of one contig's compressed coordinate,
 * <= 2^31 + 2^24 < 2^32, so every add is exact -- in the global table and in a workgroup's LDS table alike.
 *
 *   accum    a bounded grid of one-wavefront workgroups strides over the tiles of CBC_DEPTH_LINES runs, one lane per run.
 *            Real data puts millions of runs into a few dozen bins, and one global atomic per run would queue on a handful of
 *            L2 lines; so bins below CBC_HIST_LDS are added in a table in LDS and flushed once per workgroup, one list_add per
 *            non-zero word, and only depths at or above CBC_HIST_LDS go straight to the global table.  -DCBC_HIST_NO_LDS sends
 *            every run to the global table (A/B).
 *   count    one wavefront per tile of CBC_DEPTH_TILE bins: its non-zero words into a cbc_block_result for
 *            cbc_scan_sizes_kernel.  Reduce, scan, apply: no wavefront waits for another.
 *   write    the same tile again: the non-zero bins as dense pairs (depth, bases), ascending in depth.
 * Written against the wave policy (W = WaveGPU in cbc_gpu.hip, the lock-step emulation in tests/hist_emu).
 */
#ifndef CBC_HIST_BODY_H
#define CBC_HIST_BODY_H

#include <stdint.h>
#include "../../include/cbc_gpu.h"
#include "cbc_depth_body.h"

#define CBC_HIST_LDS  1024u        /* bins kept in the workgroup's LDS table: 16 rounds of 64 lanes */
#define CBC_HIST_GRID 2048u        /* workgroups of the accumulate pass at most                     */

struct cbc_hist_args {
    const uint32_t *cp_pos, *cp_dep;         /* the change points                                                               */
    const uint64_t *cnt_off;                 /* cnt_off[n_tiles] = how many there are (cbc_depth_args.cnt_off)                  */
    uint32_t *bins;                          /* n_btiles * CBC_DEPTH_TILE words, the first n_bins used                          */
    cbc_block_result *tile_nz;               /* per tile of bins: its non-zero words (nbytes)                                   */
    const uint64_t *nz_off;                  /* their exclusive scan (n_btiles + 1)                                             */
    uint32_t *out_depth, *out_bases;         /* the pairs, out_cap of each                                                      */
    uint32_t cp_cap, n_tiles, n_ttiles, fold, n_bins, n_btiles, out_cap, grid;
};

/* workgroup wg of A.grid: run tiles wg, wg + grid, ...; lds: CBC_HIST_LDS words of this workgroup (unused with CBC_HIST_NO_LDS) */
template <class W>
CBC_FN void cbc_hist_accum(const cbc_hist_args &A, uint32_t wg, uint32_t *lds)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    const uint32_t ncp = cbc_depth_points(A.cnt_off, A.n_tiles, A.cp_cap);
    const V32 ln = W::lane();
    if (A.grid == 0u || wg >= A.grid) return;
#ifndef CBC_HIST_NO_LDS
    for (uint32_t r = 0; r < CBC_HIST_LDS / 64u; r++) W::lds_zero(lds, ln + r * 64u, W::all());
#endif
    for (uint32_t tt = wg; tt < A.n_ttiles; tt += A.grid) {         /* n_ttiles + grid < 2^32: cp_cap < 2^31 + 2^25 */
        if ((uint64_t)tt * CBC_DEPTH_LINES >= ncp) break;
        for (uint32_t r = 0; r < CBC_DEPTH_LINES / 64u; r++) {
            const uint32_t j0 = tt * CBC_DEPTH_LINES + r * 64u;
            if (j0 >= ncp || ncp - j0 < 2u) break;                   /* no run from j0 on */
            V32 d, len;
            const Mask m = cbc_depth_run_load<W>(A.cp_pos, A.cp_dep, j0, ncp, d, len);
            const V32 bin = W::select(d < A.fold, d, W::splat(A.fold));
            const Mask k = m & (d != 0u) & (bin < A.n_bins);         /* a depth past the reads of the call: not from these passes */
#ifndef CBC_HIST_NO_LDS
            const Mask lo = k & (bin < CBC_HIST_LDS);
            W::lds_add(lds, bin, len, lo);
            W::list_add(A.bins, bin, len, k & !lo);
#else
            W::list_add(A.bins, bin, len, k);
#endif
        }
    }
#ifndef CBC_HIST_NO_LDS
    for (uint32_t r = 0; r < CBC_HIST_LDS / 64u; r++) {
        const V32 i = ln + r * 64u;
        const V32 v = W::lds_read(lds, i, W::all());
        W::list_add(A.bins, i, v, (v != 0u) & (i < A.n_bins));
    }
#endif
}

template <class W>
CBC_FN void cbc_hist_count(const cbc_hist_args &A, uint32_t t)
{
    typedef typename W::V32 V32;
    if (t >= A.n_btiles) return;
    const uint4 *b4 = (const uint4 *)(A.bins + (uint64_t)t * CBC_DEPTH_TILE);
    const V32 ln = W::lane();
    V32 c = W::splat(0u);
    for (uint32_t r = 0; r < CBC_DEPTH_TILE / 256u; r++) {
        V32 a, b, cc, d;
        W::load_rec(b4, ln + r * 64u, W::all(), a, b, cc, d);
        c = c + cbc_depth_nz<W>(a) + cbc_depth_nz<W>(b) + cbc_depth_nz<W>(cc) + cbc_depth_nz<W>(d);
    }
    cbc_store_result<W>(A.tile_nz + t, W::reduce_add(c), 0u);
}

template <class W>
CBC_FN void cbc_hist_write(const cbc_hist_args &A, uint32_t t)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    if (t >= A.n_btiles) return;
    const uint32_t cnt = A.tile_nz[t].nbytes;
    const uint64_t c0 = A.nz_off[t];
    if (cnt == 0u || c0 > A.out_cap || cnt > A.out_cap - c0) return;
    const uint4 *b4 = (const uint4 *)(A.bins + (uint64_t)t * CBC_DEPTH_TILE);
    const V32 ln = W::lane();
    uint32_t at = (uint32_t)c0;
    const uint32_t last = (uint32_t)c0 + cnt;
    for (uint32_t r = 0; r < CBC_DEPTH_TILE / 256u; r++) {
        V32 a, b, c, d;
        W::load_rec(b4, ln + r * 64u, W::all(), a, b, c, d);
        const V32 na = cbc_depth_nz<W>(a), nb = cbc_depth_nz<W>(b), nc = cbc_depth_nz<W>(c), nd = cbc_depth_nz<W>(d);
        const V32 n = na + nb + nc + nd;
        if (W::ballot(n != 0u) == 0ull) continue;
        const V32 ninc = W::scan_incl_add(n);
        const uint32_t chunk = W::readlane(ninc, 63u);
        if (chunk > last - at) return;                               /* the bins changed under the count pass */
        const V32 dep = ln * 4u + (t * CBC_DEPTH_TILE + r * 256u);   /* n_btiles * CBC_DEPTH_TILE <= 2^30 + 4096 */
        V32 o = (ninc - n) + at;
        Mask m = a != 0u;
        W::store32(A.out_depth, o, dep, m); W::store32(A.out_bases, o, a, m); o = o + na;
        m = b != 0u;
        W::store32(A.out_depth, o, dep + 1u, m); W::store32(A.out_bases, o, b, m); o = o + nb;
        m = c != 0u;
        W::store32(A.out_depth, o, dep + 2u, m); W::store32(A.out_bases, o, c, m); o = o + nc;
        m = d != 0u;
        W::store32(A.out_depth, o, dep + 3u, m); W::store32(A.out_bases, o, d, m);
        at += chunk;
    }
}

#endif /* CBC_HIST_BODY_H */
