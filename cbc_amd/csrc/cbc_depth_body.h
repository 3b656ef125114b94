/*
 * cbc_depth_body.h -- coverage on the device, after the span-reporting decode of one contig window's blocks
 * (cbc_gpu_decode_depth, include/cbc_gpu.h).
 *
 * Depth at reference position p = the kept reads with POS <= p <= POS + span - 1 (a SPAN coverage: the bases a read
 * deletes count as covered: this pass reads the span alone, cbc_pileup_body.h reads where they lie).  POS = window_start + local POS, span as
 * the decoder reports it (cbc_region_body.h); kept = the reads cbc_region_keep keeps for the window [beg, end], minus
 * those with FLAG & exclude != 0 or span == 0.  The output is bedGraph, one line per maximal run of equal non-zero depth
 * inside the window, 0-based half-open:   <name>\t<start0>\t<end0>\t<depth>\n
 *
 *   mark     one wavefront per block, one lane per record: the read clipped to the window, +1 at diff[s - beg] and -1
 *            (mod 2^32) at diff[e + 1 - beg] by relaxed agent-scope atomics.  diff has W + 1 words (W = end - beg + 1),
 *            zeroed before.  Everything a lane computes is block-local and 32-bit; only the wave-uniform offset of the
 *            block's window start in the diff array is 64-bit.
 *   tile     depth = inclusive prefix sum of diff, and it changes exactly where diff != 0.  One wavefront per tile of
 *            CBC_DEPTH_TILE words: the tile's sum and its count of non-zero words, each into a cbc_block_result so that
 *            cbc_scan_sizes_kernel gives the depth in front of every tile (low word of the 64-bit sum = the sum mod 2^32)
 *            and where its change points go.  Reduce, scan, apply: no wavefront waits for another.
 *   compact  the same tile again: prefix inside the tile + carry, the change points (position - beg, depth after) written
 *            densely.  The last change point of a window has depth 0 (every +1 has its -1 at or below index W).
 *   count    run j = [cp[j].pos, cp[j + 1].pos) with depth cp[j].depth, a line when that depth is not 0.  One wavefront
 *            per CBC_DEPTH_LINES runs: line lengths (digit counts by compares), lines and bytes into a cbc_block_result
 *            for the size scan (64-bit text offsets).
 *   write    the same runs, one lane per line (digits by the multiply-shift scheme of cbc_sam_body.h), through the
 *            line-per-lane writer cbc_lines_store, which cbc_pileup_body.h uses too.
 * count and write are the run-text skeleton below (cbc_runs_count / cbc_runs_write); cbc_targets_body.h instantiates it with
 * its own line function.  cbc_depth_points and cbc_depth_run_load serve every pass that reads the change points.
 * Range tests are written without base + length sums.  Written against the wave policy (W = WaveGPU in cbc_gpu.hip, the
 * lock-step emulation in tests/depth_emu).
 */
#ifndef CBC_DEPTH_BODY_H
#define CBC_DEPTH_BODY_H

#include <stdint.h>
#include "../../include/cbc_gpu.h"
#include "cbc_region_body.h"
#include "cbc_sam_body.h"          /* cbc_sam_ndig_v */

#define CBC_DEPTH_TILE  4096u      /* diff words per tile: 16 rounds of 64 lanes x 4 words */
#define CBC_DEPTH_LINES 1024u      /* runs per text tile: 16 rounds of 64 lanes           */

struct cbc_depth_args {
    cbc_region_args R;                       /* records, blocks, window starts, decode results, beg / end as for the region
                                              * passes; counts / offsets / text: the TEXT TILES' sizes, offsets, the output */
    uint32_t *diff;                          /* n_tiles * CBC_DEPTH_TILE words, the first W + 1 used                        */
    cbc_block_result *tile_sum, *tile_cnt;   /* per tile: sum of diff, non-zero words (nbytes)                              */
    const uint64_t *sum_off, *cnt_off;       /* their exclusive scans (n_tiles + 1)                                         */
    uint32_t *cp_pos, *cp_dep;               /* change points: position - beg, depth from there on                         */
    uint32_t *ctr;                           /* [0] reads kept, [1] lines written                                           */
    const uint8_t *name;                     /* device copy of the contig's name                                            */
    uint64_t diff_words;
    uint32_t cp_cap, name_len, exclude, n_tiles, n_ttiles, reserved;
};

/* ---- mark ------------------------------------------------------------------------------------------------------------ */
/* U: what is done with the kept reads.  cbc_mark_only (the default, the mark pass): +1 / -1 at the ends of every kept read's
 * piece, and the count of the kept.  A U with unmark = true (the unmark pass of cbc_skipdel_body.h) is handed the same reads
 * instead -- U::reads<W>(p, sub, r0, k, lp, span, i0, i1): group r0's keep flags, local POS, span and pieces [i0, i1) behind p --
 * and neither marks nor counts: the keep rule and the clipping are this one text for both passes, so they cannot drift apart. */
struct cbc_mark_only { static const bool unmark = false; template <class W, class... T> CBC_MFN void reads(const T &...) {} };

template <class W, class U = cbc_mark_only>
CBC_FN void cbc_depth_mark(const cbc_depth_args &A, uint32_t blk, U *u = NULL)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    const cbc_region_blk B = cbc_region_block(A.R, blk);             /* ok: decoded, 1 <= beg <= end, end > window start */
    if (!B.ok) return;
    const uint64_t ws = A.R.window_start[blk], beg = A.R.beg;
    const uint64_t nw = A.R.end - beg;                               /* W - 1; index W is the last word used */
    if (nw >= A.diff_words - 1u || A.diff_words == 0u) return;
    /* local coordinate x sits at diff[x + ws - beg]: ws >= beg moves the base up (ws - beg < W since end > ws), otherwise
     * `sub` = beg - ws comes off the lane's index (B.ok: beg + 1 - ws < 2^32) */
    const uint64_t fwd = ws >= beg ? ws - beg : 0u;
    const uint32_t sub = ws >= beg ? 0u : (uint32_t)(beg - ws);
    uint32_t *p = A.diff + fwd;
    const uint64_t rem64 = (nw + 1u) - fwd;                          /* the largest index behind p */
    const uint32_t rem = rem64 > 0xffffffffull ? 0xffffffffu : (uint32_t)rem64;
    const V32 ln = W::lane();
    uint32_t kept = 0;
    for (uint32_t r0 = 0; r0 < B.n; r0 += 64u) {
        V32 rlv, lp, fl, off, span;
        Mask k = cbc_region_keep<W>(B, r0, rlv);                     /* lp <= hi, lp + span >= beg + 1 - ws */
        W::load_rec(B.recs4, ln + r0, k, lp, fl, off, span);
        k = k & ((fl & (A.exclude & 0xffffu)) == 0u) & (span >= 1u);
        /* the read clipped to the window, local: s = max(lp, sub), e = min(lp + span - 1, hi), neither as a sum that wraps */
        const V32 s = W::select(lp >= sub, lp, W::splat(sub));
        const V32 e = W::select((span - 1u) >= (W::splat(B.hi) - lp), W::splat(B.hi), lp + (span - 1u));
        const V32 i0 = s - sub, i1 = (e - sub) + 1u;
        k = k & (i1 > i0) & (i1 <= rem);
        if (U::unmark) { u->template reads<W>(p, sub, r0, k, lp, span, i0, i1); continue; }
        W::list_add(p, i0, W::splat(1u), k);
        W::list_add(p, i1, W::splat(0xffffffffu), k);
        kept += W::popc64(W::ballot(k));
    }
    if (U::unmark) return;
    W::list_add(A.ctr, W::splat(0u), W::splat(kept), ln == 0u);
}

/* ---- tile sums, change points ----------------------------------------------------------------------------------------- */
template <class W>
CBC_FN typename W::V32 cbc_depth_nz(const typename W::V32 &x) { return W::select(x != 0u, W::splat(1u), W::splat(0u)); }

template <class W>
CBC_FN void cbc_depth_tile(const cbc_depth_args &A, uint32_t t)
{
    typedef typename W::V32 V32;
    if (t >= A.n_tiles || A.diff_words / CBC_DEPTH_TILE < A.n_tiles) return;
    const uint4 *d4 = (const uint4 *)(A.diff + (uint64_t)t * CBC_DEPTH_TILE);
    const V32 ln = W::lane();
    V32 s = W::splat(0u), c = W::splat(0u);
    for (uint32_t r = 0; r < CBC_DEPTH_TILE / 256u; r++) {
        V32 a, b, cc, d;
        W::load_rec(d4, ln + r * 64u, W::all(), a, b, cc, d);
        s = s + a + b + cc + d;
        c = c + cbc_depth_nz<W>(a) + cbc_depth_nz<W>(b) + cbc_depth_nz<W>(cc) + cbc_depth_nz<W>(d);
    }
    cbc_store_result<W>(A.tile_sum + t, W::reduce_add(s), 0u);
    cbc_store_result<W>(A.tile_cnt + t, W::reduce_add(c), 0u);
}

template <class W>
CBC_FN void cbc_depth_compact(const cbc_depth_args &A, uint32_t t)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    if (t >= A.n_tiles || A.diff_words / CBC_DEPTH_TILE < A.n_tiles) return;
    const uint32_t cnt = A.tile_cnt[t].nbytes;
    const uint64_t c0 = A.cnt_off[t];
    if (cnt == 0u || c0 > A.cp_cap || cnt > A.cp_cap - c0) return;
    const uint4 *d4 = (const uint4 *)(A.diff + (uint64_t)t * CBC_DEPTH_TILE);
    const V32 ln = W::lane();
    uint32_t run = (uint32_t)A.sum_off[t];                           /* depth in front of the tile, mod 2^32 */
    uint32_t at = (uint32_t)c0;
    const uint32_t last = (uint32_t)c0 + cnt;
    for (uint32_t r = 0; r < CBC_DEPTH_TILE / 256u; r++) {
        V32 a, b, c, d;
        W::load_rec(d4, ln + r * 64u, W::all(), a, b, c, d);
        const V32 na = cbc_depth_nz<W>(a), nb = cbc_depth_nz<W>(b), nc = cbc_depth_nz<W>(c), nd = cbc_depth_nz<W>(d);
        const V32 n = na + nb + nc + nd;
        if (W::ballot(n != 0u) == 0ull) continue;                    /* 256 zero words: depth and count unchanged */
        const V32 s1 = a, s2 = s1 + b, s3 = s2 + c, s4 = s3 + d;
        const V32 incl = W::scan_incl_add(s4), ninc = W::scan_incl_add(n);
        const uint32_t chunk = W::readlane(ninc, 63u);
        if (chunk > last - at) return;                               /* diff changed under the tile pass */
        const V32 ex = (incl - s4) + run;
        const V32 pos = ln * 4u + (t * CBC_DEPTH_TILE + r * 256u);
        V32 o = (ninc - n) + at;
        Mask m = a != 0u;
        W::store32(A.cp_pos, o, pos, m); W::store32(A.cp_dep, o, ex + s1, m); o = o + na;
        m = b != 0u;
        W::store32(A.cp_pos, o, pos + 1u, m); W::store32(A.cp_dep, o, ex + s2, m); o = o + nb;
        m = c != 0u;
        W::store32(A.cp_pos, o, pos + 2u, m); W::store32(A.cp_dep, o, ex + s3, m); o = o + nc;
        m = d != 0u;
        W::store32(A.cp_pos, o, pos + 3u, m); W::store32(A.cp_dep, o, ex + s4, m);
        run += W::readlane(incl, 63u);
        at += chunk;
    }
}

/* ---- text -------------------------------------------------------------------------------------------------------------- */
/* runs [j0, j0 + 64) of the window's `nr` runs: start0, end0, depth and the line's length (0: no line) */
template <class W>
CBC_FN typename W::Mask cbc_depth_line(const cbc_depth_args &A, uint32_t j0, uint32_t nr, typename W::V32 &st,
                                       typename W::V32 &en, typename W::V32 &dp, typename W::V32 &len)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    const V32 j = W::lane() + j0;
    const Mask m = j < nr;                                           /* j + 1 <= nr < the change points */
    const uint32_t b0 = (uint32_t)(A.R.beg - 1u);                    /* position beg is 0-based beg - 1; end <= CBC_SAM_MAX_POS */
    st = W::load32(A.cp_pos, j, m, 0u) + b0;
    en = W::load32(A.cp_pos, j + 1u, m, 0u) + b0;
    dp = W::load32(A.cp_dep, j, m, 0u);
    const Mask k = m & (dp != 0u);
    const V32 l = cbc_sam_ndig_v<W>(st, 1000000000u) + cbc_sam_ndig_v<W>(en, 1000000000u) + cbc_sam_ndig_v<W>(dp, 1000000000u) +
                  (A.name_len + 4u);
    len = W::select(k, l, W::splat(0u));
    return k;
}

/* the run text of cbc_depth_line as it stands: the window's first position is a POS */
CBC_FN bool cbc_depth_line_ok(const cbc_depth_args &A) { return A.R.beg >= 1u && A.R.beg <= CBC_SAM_MAX_POS; }

/* change points of a call: what the compact pass counted (cnt_off[n_tiles]), never more than the tables hold */
CBC_FN uint32_t cbc_depth_points(const uint64_t *cnt_off, uint32_t n_tiles, uint32_t cp_cap)
{
    const uint64_t n = cnt_off[n_tiles];
    return n > cp_cap ? cp_cap : (uint32_t)n;
}

/* runs of the window: the change points less one (the last one ends the last run) */
CBC_FN uint32_t cbc_depth_runs(const cbc_depth_args &A)
{
    const uint32_t ncp = cbc_depth_points(A.cnt_off, A.n_tiles, A.cp_cap);
    return ncp ? ncp - 1u : 0u;
}

/* runs [j0, j0 + 64) of ncp change points: depth and length under the mask returned (the run exists: j + 1 < ncp), zeros
 * in the other lanes */
template <class W>
CBC_FN typename W::Mask cbc_depth_run_load(const uint32_t *cp_pos, const uint32_t *cp_dep, uint32_t j0, uint32_t ncp,
                                           typename W::V32 &d, typename W::V32 &len)
{
    const typename W::V32 j = W::lane() + j0;
    const typename W::Mask m = (j + 1u) < ncp;                       /* ncp <= cp_cap < 2^32 - 64: no wrap */
    const typename W::V32 p = W::load32(cp_pos, j, m, 0u), q = W::load32(cp_pos, j + 1u, m, 0u);
    d = W::load32(cp_dep, j, m, 0u);
    len = q - p;
    return m;
}

/* v = hi * 10^5 + lo for any 32-bit v: floor(v / 10^5) = floor((v >> 5) / 3125) = ((v >> 5) * M) >> 39 with
 * M = ceil(2^39 / 3125) = 175921861: exact while (v >> 5) * (M * 3125 - 2^39) < 2^39, and that error term is below 3125 < 2^12
 * against v >> 5 < 2^27 */
template <class W>
CBC_FN void cbc_depth_split(const typename W::V32 &v, typename W::V32 &hi, typename W::V32 &lo)
{
    hi = W::mulhi(v >> 5, W::splat(175921861u)) >> 7;
    lo = v - hi * 100000u;
}

/* ASCII digit j (0 = least significant, j <= 9) of hi * 10^5 + lo, per lane: digit j mod 5 of a value below 10^5 by the
 * multiply-shift division of cbc_sam_digits (cbc_sam_body.h has the error bounds); a j past 9 gives a byte nobody stores */
template <class W>
CBC_FN typename W::V32 cbc_depth_digit(const typename W::V32 &hi, const typename W::V32 &lo, const typename W::V32 &j)
{
    typedef typename W::V32 V32;
    const V32 v = W::select(j < 5u, lo, hi);
    const V32 jj = W::select(j < 5u, j, j - 5u);
    const V32 M = W::select(jj == 1u, W::splat(429496730u), W::select(jj == 2u, W::splat(42949673u),
                  W::select(jj == 3u, W::splat(4294968u), W::splat(429497u))));
    const V32 q = W::select(jj == 0u, v, W::mulhi(v, M));
    return (q - W::mulhi(q, W::splat(429496730u)) * 10u) + 48u;
}

/* ---- the line-per-lane writer ------------------------------------------------------------------------------------------
 * Lane l under k writes its line of len bytes at dst[at ..]: `name` (nl bytes) and then, for i >= nl, byte i as
 * cbc_line_byte(L, i) gives it per lane -- overloaded on the line state L (cbc_depth_ln here, cbc_pileup_ln in
 * cbc_pileup_body.h).  The line is made four bytes at a time and written as dwords at its own byte offset; a dword never
 * leaves its line, the last 1..3 bytes are byte stores. */
template <class W, class L>
CBC_FN void cbc_lines_store(uint8_t *dst, const typename W::V32 &at, const typename W::V32 &len, const typename W::Mask &k,
                            const uint8_t *name, uint32_t nl, const L &ls)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    const uint32_t maxlen = W::readlane(W::scan_incl_max(len), 63u);
    for (uint32_t q = 0; q < maxlen; q += 4u) {
        V32 out = W::splat(0u);
        for (uint32_t t = 0; t < 4u; t++) {
            const uint32_t i = q + t;
            out = out | ((i < nl ? W::splat(W::read_uni8(name, i)) : cbc_line_byte(ls, i)) << (8u * t));
        }
        const Mask full = k & (W::splat(q + 4u) <= len);
        W::store32_bytes(dst, at + q, out, full);
        const Mask part = k & !full & (W::splat(q) < len);
        if (W::ballot(part) != 0ull)
            for (uint32_t t = 0; t < 3u; t++)
                W::store8(dst, at + (q + t), (out >> (8u * t)) & 0xffu, part & (W::splat(q + t) < len));
    }
}

/* a run's line: name, '\t' at nl, start0, '\t' at e1, end0, '\t' at e2, depth, '\n' at e3 = len - 1; the numbers split */
template <class W>
struct cbc_depth_ln { typename W::V32 e1, e2, e3, sh, sl, eh, el, dh, dl; uint32_t nl; };

template <class W>
CBC_FN typename W::V32 cbc_line_byte(const cbc_depth_ln<W> &L, uint32_t i)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    const V32 iv = W::splat(i);
    const Mask f1 = iv < L.e1, f2 = iv < L.e2;
    const V32 hi = W::select(f1, L.sh, W::select(f2, L.eh, L.dh)), lo = W::select(f1, L.sl, W::select(f2, L.el, L.dl));
    const V32 j = (W::select(f1, L.e1, W::select(f2, L.e2, L.e3)) - 1u) - iv;
    V32 by = cbc_depth_digit<W>(hi, lo, j);
    by = W::select((iv == L.nl) | (iv == L.e1) | (iv == L.e2), W::splat(9u), by);
    return W::select(iv == L.e3, W::splat(10u), by);
}

/* ---- the run-text skeleton ---------------------------------------------------------------------------------------------
 * count and write for one line per run of non-zero depth, one wavefront per CBC_DEPTH_LINES runs.  A member is its argument
 * struct A (D = the cbc_depth_args inside) with two functions overloaded on it: cbc_depth_line<W>(A, j0, nr, st, en, dp, len)
 * and its guard cbc_depth_line_ok(A).  The members: the window (above), the target set (cbc_targets_body.h). */
template <class W, class Args>
CBC_FN void cbc_runs_count(const Args &A, const cbc_depth_args &D, uint32_t tt)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    const uint32_t nr = cbc_depth_runs(D);
    uint32_t lines = 0, bytes = 0;
    if (D.name_len <= CBC_SAM_MAX_NAME && cbc_depth_line_ok(A) && tt < D.n_ttiles)
        for (uint32_t r = 0; r < CBC_DEPTH_LINES / 64u; r++) {
            const uint32_t j0 = tt * CBC_DEPTH_LINES + r * 64u;
            if (j0 >= nr) break;
            V32 st, en, dp, len;
            const Mask k = cbc_depth_line<W>(A, j0, nr, st, en, dp, len);
            lines += W::popc64(W::ballot(k));
            bytes += W::reduce_add(len);
        }
    cbc_store_result<W>(D.R.counts + tt, bytes, lines);
    if (lines) W::list_add(D.ctr, W::splat(1u), W::splat(lines), W::lane() == 0u);
}

template <class W, class Args>
CBC_FN void cbc_runs_write(const Args &A, const cbc_depth_args &D, uint32_t tt)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    if (tt >= D.n_ttiles || D.name_len > CBC_SAM_MAX_NAME || !cbc_depth_line_ok(A)) return;
    const uint32_t nr = cbc_depth_runs(D);
    const uint32_t bytes = D.R.counts[tt].nbytes;
    const uint64_t o0 = D.R.offsets[tt];
    if (bytes == 0u || o0 > D.R.text_cap || bytes > D.R.text_cap - o0) return;
    uint64_t o = o0;
    for (uint32_t r = 0; r < CBC_DEPTH_LINES / 64u; r++) {
        const uint32_t j0 = tt * CBC_DEPTH_LINES + r * 64u;
        if (j0 >= nr) break;
        V32 st, en, dp, len;
        const Mask k = cbc_depth_line<W>(A, j0, nr, st, en, dp, len);
        const V32 incl = W::scan_incl_add(len);
        const uint32_t chunk = W::readlane(incl, 63u);
        if (chunk > (o0 + bytes) - o) return;                        /* the change points moved under the count pass */
        if (chunk == 0u) continue;
        cbc_depth_ln<W> L;
        L.nl = D.name_len;
        L.e1 = cbc_sam_ndig_v<W>(st, 1000000000u) + (L.nl + 1u);
        L.e2 = L.e1 + cbc_sam_ndig_v<W>(en, 1000000000u) + 1u;
        L.e3 = len - 1u;
        cbc_depth_split<W>(st, L.sh, L.sl); cbc_depth_split<W>(en, L.eh, L.el); cbc_depth_split<W>(dp, L.dh, L.dl);
        cbc_lines_store<W>(D.R.text + o, incl - len, len, k, D.name, L.nl, L);
        o += chunk;
    }
}

template <class W>
CBC_FN void cbc_depth_count(const cbc_depth_args &A, uint32_t tt) { cbc_runs_count<W>(A, A, tt); }
template <class W>
CBC_FN void cbc_depth_write(const cbc_depth_args &A, uint32_t tt) { cbc_runs_write<W>(A, A, tt); }

#endif /* CBC_DEPTH_BODY_H */
