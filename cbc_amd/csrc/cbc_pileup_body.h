/*
 * cbc_pileup_body.h -- per-position allele counts on the device, after the edit-reporting decode of one contig window's blocks
 * (cbc_gpu_decode_pileup, include/cbc_gpu.h).
 *
 * The decoder (cbc_decode_body.h, EDITS = true) has left, beside the records, rows and spans, the alignment of every read with
 * indels: nDel matched coordinates dc[] and nIns read indices oi[] (cbc_dec_edits).  With T = rl - nIns:
 *   read index q with q == oi[i] for some i is inserted;
 *   any other q has matched coordinate m = q - #{i : oi[i] < q} and is aligned to POS + m + #{d : dc[d] <= m};
 *   deleted base d is reference position POS + dc[d] + d
 * -- the counting form edits_indel() rebuilds the read with, not restated with other edge cases: `#{oi < q}` is its `nb`,
 * `#{dc <= m}` its `sh`.  A read without indels (coded as perfect, or SNPs only) has q aligned to POS + q.  Whatever this maps
 * outside the read's span [POS, POS + span - 1] is not counted (only a crafted file does that).
 *
 * Per position p of the window [beg, end], seven 32-bit counters in seven planes of `plane` words (28 bytes per position):
 *   0..4   aligned read bases whose class (A, C, G, T, other: byte & 0xDF) DIFFERS from the class of the reference byte
 *   5      deleted bases
 *   6      insertion events: maximal runs of inserted read indices, anchored at the reference position of the nearest aligned
 *          base before the run, or at POS when there is none
 * A matching base costs no atomic: the line pass has the span depth (the prefix sum of cbc_depth_mark's difference array), and
 * cnt[class(ref)] = depth - del - the five mismatch counters.
 *
 *   events   CBC_PILEUP_WAVES wavefronts per block share its kept reads (the keep rule of cbc_depth_mark); a read is taken by
 *            the whole wavefront, 64 read indices a turn, one lane per index; then its deleted bases, one lane per base.
 *   count    one wavefront per tile of CBC_DEPTH_TILE positions, one lane per position: depth from the tile's carry
 *            (cbc_depth_tile + cbc_scan_sizes_kernel), the line rule nonref = mismatches + del + ins >= min_alt, lines and bytes
 *            into a cbc_block_result for the size scan (64-bit text offsets).
 *   write    the same tile again, one lane per line:  <name> <pos1> <ref> <depth> <A> <C> <G> <T> <N> <del> <ins>  tab-separated,
 *            through the line-per-lane writer of cbc_depth_body.h (cbc_lines_store) with the line bytes of cbc_pileup_ln.
 * cbc_gpu_decode_pileup_ext runs the same passes with a template parameter each: the events into the
 * planes of the read's strand (14 planes), the line rule with the fraction, the line with seven per-strand columns; the plain
 * call's instantiations are the bodies as they were.
 * Range tests are written without base + length sums.  Written against the wave policy (W = WaveGPU in cbc_gpu.hip, the
 * lock-step emulation in tests/pileup_emu and tests/pileup_strand_emu).
 */
#ifndef CBC_PILEUP_BODY_H
#define CBC_PILEUP_BODY_H

#include <stdint.h>
#include <type_traits>
#include "../../include/cbc_gpu.h"
#include "cbc_region_body.h"
#include "cbc_depth_body.h"

#define CBC_PILEUP_WAVES  4u       /* wavefronts that share one block's reads in the events pass */
#define CBC_PILEUP_PLANES 7u
#define CBC_PILEUP_DEL    5u
#define CBC_PILEUP_INS    6u

struct cbc_pileup_args {
    cbc_depth_args D;             /* records, blocks, window, diff, tile sums and their scan, counters ([0] reads kept by the mark
                                   * pass, [1] lines), name; R.counts / R.offsets / R.text: the position tiles' sizes, offsets, text */
    const uint32_t *side;         /* the EDITS decoder's side array and arena (cbc_dec_edits)                                    */
    const uint16_t *arena;
    const uint8_t  *ref;          /* the device reference                                                                        */
    uint32_t *tab;                /* CBC_PILEUP_PLANES planes of `plane` words, zeroed before                                    */
    uint64_t arena_entries, ref_bytes, plane;
    uint64_t ref_c0;              /* reference byte of window position p (1-based) = ref[ref_c0 + p - 1]                         */
    uint32_t per_read, min_alt;
};

/* class of a base byte: 0..3 = A, C, G, T in either case, 4 = anything else */
template <class W>
CBC_FN typename W::V32 cbc_pileup_class(const typename W::V32 &b)
{
    const typename W::V32 c = b & 0xdfu;
    return W::select(c == 0x41u, W::splat(0u), W::select(c == 0x43u, W::splat(1u), W::select(c == 0x47u, W::splat(2u),
           W::select(c == 0x54u, W::splat(3u), W::splat(4u)))));
}

/* where the local coordinates of a block sit in the planes: local x is plane word fwd + (x - sub), inside the window when
 * x >= sub and x - sub <= rem (the arithmetic of cbc_depth_mark) */
struct cbc_pileup_win { uint64_t fwd; uint32_t sub, rem; bool ok; };

CBC_FN cbc_pileup_win cbc_pileup_window(const cbc_pileup_args &A, uint32_t blk)
{
    cbc_pileup_win w;
    const uint64_t ws = A.D.R.window_start[blk], beg = A.D.R.beg;
    const uint64_t nw = A.D.R.end - beg;                             /* the window's last index */
    w.ok = A.plane != 0u && nw < A.plane;
    w.fwd = ws >= beg ? ws - beg : 0u;
    w.sub = ws >= beg ? 0u : (uint32_t)(beg - ws);                   /* cbc_region_block: beg + 1 - ws < 2^32 */
    w.ok = w.ok && w.fwd <= nw;
    const uint64_t rem64 = w.ok ? nw - w.fwd : 0u;
    w.rem = rem64 > 0xffffffffull ? 0xffffffffu : (uint32_t)rem64;
    return w;
}

/* ---- what every reader of the kept alignment shares (the events pass here, the unmark pass of cbc_skipdel_body.h) ---------- */
/* a block's part of the side array and of the arena, by the decoder's own test; the side array runs beside the records
 * (cbc_region_block's ok: inside n_recs).  ok = false (a per_read outside 1..510, a range outside the arena): the block's
 * alignment is not read */
struct cbc_edits_blk { const uint32_t *side; const uint16_t *arena; uint32_t cap; bool ok; };

CBC_FN cbc_edits_blk cbc_edits_block(const uint32_t *side, const uint16_t *arena, uint64_t arena_entries, uint32_t per_read,
                                     uint64_t rec_base, uint32_t n)
{
    cbc_edits_blk E;
    const uint64_t cap64 = (uint64_t)n * per_read, base64 = rec_base * per_read;
    E.ok = !(per_read < 1u || per_read > 510u || base64 > arena_entries || cap64 > arena_entries - base64);
    E.cap = (uint32_t)cap64;
    E.arena = arena + (E.ok ? base64 : 0u);
    E.side = side + 2u * rec_base;
    return E;
}

/* a read's entries [e0, e0 + nd + ni) of its block's `cap`: false is not what the decoder writes, and the read is skipped */
CBC_FN bool cbc_edits_read_ok(uint32_t e0, uint32_t nd, uint32_t ni, uint32_t cap)
{
    return !(nd > 255u || ni > 255u || e0 > cap || nd + ni > cap - e0);
}

/* deleted base d of a read with the matched coordinates dc[] = ar[0 .. nd): its offset from POS, dc[d] + d */
template <class W>
CBC_FN typename W::V32 cbc_edits_del_offset(const uint16_t *ar, const typename W::V32 &d, const typename W::Mask &md)
{
    return W::load16(ar, d, md) + d;
}

/* ---- events ------------------------------------------------------------------------------------------------------------ */
/* STRAND (cbc_gpu_decode_pileup_ext with by_strand): tab holds 2 * CBC_PILEUP_PLANES planes, the seven of
 * the reads with FLAG & 16 == 0 and behind them the seven of the others; an observation still costs one list_add, into the
 * planes of its read's strand, which is uniform over the wavefront's turn.  Without it the body is the text it was. */
template <class W, bool STRAND = false>
CBC_FN void cbc_pileup_events(const cbc_pileup_args &A, uint32_t blk, uint32_t wave, uint32_t n_waves)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    const cbc_region_blk B = cbc_region_block(A.D.R, blk);           /* ok: decoded, 1 <= beg <= end, end > window start */
    if (!B.ok || n_waves == 0u || wave >= n_waves) return;
    const cbc_pileup_win Wn = cbc_pileup_window(A, blk);
    if (!Wn.ok) return;
    const cbc_dec_block_desc *bd = A.D.R.blocks + blk;
    const uint64_t rec_base = bd->rec_base, ref_off = bd->ref_off;
    const cbc_edits_blk E = cbc_edits_block(A.side, A.arena, A.arena_entries, A.per_read, rec_base, B.n);
    if (!E.ok) return;
    const uint16_t *arena = E.arena;
    const uint32_t *side = E.side;
    if (ref_off > A.ref_bytes) return;
    const uint64_t ref_avail = A.ref_bytes - ref_off;
    const uint32_t ref_lim = ref_avail > 0xffffffffull ? 0xffffffffu : (uint32_t)ref_avail;
    const uint8_t *refb = A.ref + ref_off;
    uint32_t *p = A.tab + Wn.fwd;
    const V32 ln = W::lane();
    uint32_t nq = 0;                                                 /* kept reads of the block so far */
    for (uint32_t r0 = 0; r0 < B.n; r0 += 64u) {
        V32 rlv, lp, fl, off, span;
        Mask k = cbc_region_keep<W>(B, r0, rlv);
        W::load_rec(B.recs4, ln + r0, k, lp, fl, off, span);
        k = k & ((fl & (A.D.exclude & 0xffffu)) == 0u) & (span >= 1u);
        const V32 sd0 = W::load32(side, (ln + r0) * 2u, k, 0u), sd1 = W::load32(side, (ln + r0) * 2u + 1u, k, 0u);
        uint64_t bits = W::ballot(k);
        while (bits) {
            const uint32_t j = W::ctz64(bits);
            bits &= bits - 1u;
            if ((nq++ % n_waves) != wave) continue;
            const uint32_t rl = W::readlane(rlv, j), lpj = W::readlane(lp, j), sp = W::readlane(span, j);
            const uint32_t e0 = W::readlane(sd0, j), cnt = W::readlane(sd1, j), nd = cnt & 0xffffu, ni = cnt >> 16;
            if (!cbc_edits_read_ok(e0, nd, ni, E.cap)) continue;
            const uint16_t *ar = arena + e0;                         /* dc = ar[0 .. nd), oi = ar[nd .. nd + ni) */
            const uint8_t *row = B.rows + (uint64_t)(r0 + j) * B.stride;
            uint32_t *ps = p;                                        /* the planes of the read's strand */
            if constexpr (STRAND) ps = p + (uint64_t)(((W::readlane(fl, j) >> 4) & 1u) * CBC_PILEUP_PLANES) * A.plane;
            /* the first 64 entries of each list in a register; later ones (rare) are read one by one */
            const V32 dcv = W::load16(ar, ln, ln < nd), oiv = W::load16(ar, ln + nd, ln < ni);
            for (uint32_t b = 0; b < rl; b += 64u) {
                const V32 q = ln + b;
                const Mask inr = q < rl;
                V32 nb = W::splat(0u), ii = W::splat(0u), pi = W::splat(0u);
                for (uint32_t i = 0; i < ni; i++) {
                    const uint32_t oi = i < 64u ? W::readlane(oiv, i) : W::read_uni16(ar, nd + i);
                    nb = nb + W::select(q > oi, W::splat(1u), W::splat(0u));
                    ii = W::select(q == oi, W::splat(1u), ii);
                    pi = W::select(q == oi + 1u, W::splat(1u), pi);
                }
                const Mask isins = ii != 0u;
                const Mask al = inr & !isins;                        /* an aligned base */
                const Mask st = inr & isins & (pi == 0u);            /* the first index of an insertion run */
                const V32 m = q - nb;                                /* matched coordinate; of an inserted q: that of the next aligned base */
                const Mask none = isins & (m == 0u);                 /* no aligned base before the run: the anchor is POS */
                const V32 mm = W::select(isins & !none, m - 1u, m);  /* the run's anchor is the aligned base before it */
                V32 sh = W::splat(0u);
                for (uint32_t d = 0; d < nd; d++) {
                    const uint32_t dc = d < 64u ? W::readlane(dcv, d) : W::read_uni16(ar, d);
                    sh = sh + W::select(mm >= dc, W::splat(1u), W::splat(0u));
                }
                const V32 xo = W::select(none, W::splat(0u), mm + sh);     /* offset from POS; below rl + 255 */
                const V32 x = xo + lpj;                              /* decoded record: local POS + span < 2^32 */
                const Mask in = (al | st) & (xo < sp) & (x >= Wn.sub) & ((x - Wn.sub) <= Wn.rem);
                const V32 idx = x - Wn.sub;
                const Mask ab = al & in & ((x - 1u) < ref_lim);      /* local POS >= 1 */
                const V32 cb = cbc_pileup_class<W>(W::load8(row, q, ab)), cr = cbc_pileup_class<W>(W::load8(refb, x - 1u, ab));
                const Mask mis = ab & (cb != cr);
                if (W::ballot(mis) != 0ull)
                    for (uint32_t c = 0; c < 5u; c++) W::list_add(ps + (uint64_t)c * A.plane, idx, W::splat(1u), mis & (cb == c));
                W::list_add(ps + (uint64_t)CBC_PILEUP_INS * A.plane, idx, W::splat(1u), st & in);
            }
            for (uint32_t b = 0; b < nd; b += 64u) {                 /* deleted base d: POS + dc[d] + d */
                const V32 d = ln + b;
                const Mask md = d < nd;
                const V32 xo = cbc_edits_del_offset<W>(ar, d, md);
                const V32 x = xo + lpj;
                const Mask in = md & (xo < sp) & (x >= Wn.sub) & ((x - Wn.sub) <= Wn.rem);
                W::list_add(ps + (uint64_t)CBC_PILEUP_DEL * A.plane, x - Wn.sub, W::splat(1u), in);
            }
        }
    }
}

/* ---- lines ------------------------------------------------------------------------------------------------------------- */
/* positions [i0, i0 + 64) of the window, `run` = the depth in front of them (advanced): the nine numbers of the line in
 * v[] = pos1, depth, A, C, G, T, N, del, ins, the reference byte, the line's length (0: no line) */
/* What cbc_gpu_decode_pileup_ext adds, as the mode M of the line, count and write bodies: 0 the plain
 * call, whose bodies are the text they were; CBC_PILEUP_FRAC the fraction rule; CBC_PILEUP_STRAND the fraction rule and the
 * seven per-strand columns.  X is read by the modes above 0 only.
 *   fraction   a line needs nonref * 10^6 >= ppm * depth beside nonref >= min_alt, both products in 64 bits as (mulhi, low word)
 *              pairs: nonref, depth < 2^32 and ppm <= 10^6 < 2^20 keep them below 2^52.  ppm = 0 passes everything.
 *   strand     tab holds the forward planes and behind them the reverse planes (cbc_pileup_events<W, true>), a total is their
 *              sum; diff_f is a second difference array, marked by cbc_depth_mark with the forward reads only, with its own
 *              tile sums and their scan sum_off_f: its carry `runf` runs beside `run`, and the forward bases of the reference's
 *              class are depth+ - del+ - mismatches+ as for the totals.  v[9 .. 15] = A+, C+, G+, T+, N+, del+, ins+; len2 = the
 *              bytes of these seven columns, the tail of the line's len. */
#define CBC_PILEUP_FRAC   1
#define CBC_PILEUP_STRAND 2

struct cbc_pileup_sx {
    const uint32_t *diff_f;       /* STRAND: the forward reads' difference array, whole tiles like diff                        */
    const uint64_t *sum_off_f;    /* STRAND: the exclusive scan of its tile sums (n_tiles + 1)                                  */
    uint32_t ppm, reserved;       /* the least alternative fraction in parts per million, 0: none                              */
};

template <class W, int M = 0>
CBC_FN typename W::Mask cbc_pileup_line(const cbc_pileup_args &A, uint32_t i0, uint32_t &run, typename W::V32 *v,
                                        typename W::V32 &rb, typename W::V32 &len, const cbc_pileup_sx *X = NULL,
                                        uint32_t *runf = NULL, typename W::V32 *len2 = NULL)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    const V32 idx = W::lane() + i0;
    const uint64_t nw = A.D.R.end - A.D.R.beg;
    const Mask m = idx <= (nw > 0xffffffffull ? 0xffffffffu : (uint32_t)nw);
    const V32 d = W::load32(A.D.diff, idx, W::all(), 0u);            /* whole tiles behind diff */
    const V32 incl = W::scan_incl_add(d);
    const V32 depth = incl + run;
    run += W::readlane(incl, 63u);
    V32 c[CBC_PILEUP_PLANES], nonref = W::splat(0u);
    V32 cf[M == CBC_PILEUP_STRAND ? CBC_PILEUP_PLANES : 1u], depthf = W::splat(0u);
    if constexpr (M == CBC_PILEUP_STRAND) {
        const V32 inclf = W::scan_incl_add(W::load32(X->diff_f, idx, W::all(), 0u));
        depthf = inclf + *runf;
        *runf += W::readlane(inclf, 63u);
    }
    for (uint32_t k = 0; k < CBC_PILEUP_PLANES; k++) {
        c[k] = W::load32(A.tab + (uint64_t)k * A.plane, idx, m, 0u);
        if constexpr (M == CBC_PILEUP_STRAND) {
            cf[k] = c[k];
            c[k] = c[k] + W::load32(A.tab + (uint64_t)(CBC_PILEUP_PLANES + k) * A.plane, idx, m, 0u);
        }
        nonref = nonref + c[k];
    }
    Mask k = m & (nonref >= A.min_alt) & (A.min_alt >= 1u);
    if constexpr (M != 0) {
        const V32 mil = W::splat(1000000u), ppm = W::splat(X->ppm);
        const V32 nh = W::mulhi(nonref, mil), nl = nonref * 1000000u, dh = W::mulhi(depth, ppm), dl = depth * X->ppm;
        k = k & ((nh > dh) | ((nh == dh) & (nl >= dl)));
    }
    len = W::splat(0u);
    if constexpr (M == CBC_PILEUP_STRAND) *len2 = W::splat(0u);
    if (W::ballot(k) == 0ull) return k;
    const uint64_t at = A.ref_c0 + (A.D.R.beg - 1u);                 /* the reference byte of index 0 */
    const uint64_t avail = at <= A.ref_bytes ? A.ref_bytes - at : 0u;
    const Mask rok = k & (idx < (avail > 0xffffffffull ? 0xffffffffu : (uint32_t)avail));
    rb = W::select(rok, W::load8(A.ref + (at <= A.ref_bytes ? at : 0u), idx, rok), W::splat((uint32_t)'N'));
    const V32 cr = cbc_pileup_class<W>(rb);
    const V32 mis = c[0] + c[1] + c[2] + c[3] + c[4];
    const V32 same = depth - c[CBC_PILEUP_DEL] - mis;                /* the bases of the reference's class */
    v[0] = idx + (uint32_t)A.D.R.beg;                                /* end <= CBC_SAM_MAX_POS */
    v[1] = depth;
    for (uint32_t s = 0; s < 5u; s++) v[2u + s] = W::select(cr == s, same, c[s]);
    v[7] = c[CBC_PILEUP_DEL]; v[8] = c[CBC_PILEUP_INS];
    V32 l = W::splat(A.D.name_len + 12u);                            /* name, ten '\t', the reference byte, '\n' */
    for (uint32_t s = 0; s < 9u; s++) l = l + cbc_sam_ndig_v<W>(v[s], 1000000000u);
    if constexpr (M == CBC_PILEUP_STRAND) {
        const V32 misf = cf[0] + cf[1] + cf[2] + cf[3] + cf[4];
        const V32 samef = depthf - cf[CBC_PILEUP_DEL] - misf;        /* the forward bases of the reference's class */
        for (uint32_t s = 0; s < 5u; s++) v[9u + s] = W::select(cr == s, samef, cf[s]);
        v[14] = cf[CBC_PILEUP_DEL]; v[15] = cf[CBC_PILEUP_INS];
        V32 l2 = W::splat(7u);                                       /* seven '\t'; the '\n' of the first part becomes one */
        for (uint32_t s = 9; s < 16u; s++) l2 = l2 + cbc_sam_ndig_v<W>(v[s], 1000000000u);
        *len2 = W::select(k, l2, W::splat(0u));
        l = l + l2;
    }
    len = W::select(k, l, W::splat(0u));
    return k;
}

CBC_FN bool cbc_pileup_text_ok(const cbc_pileup_args &A, uint32_t t)
{
    return t < A.D.n_tiles && A.D.diff_words / CBC_DEPTH_TILE >= A.D.n_tiles && A.plane >= A.D.diff_words &&
           A.D.name_len <= CBC_SAM_MAX_NAME && A.D.R.beg >= 1u && A.D.R.beg <= A.D.R.end && A.D.R.end <= CBC_SAM_MAX_POS;
}

template <class W, int M = 0>
CBC_FN void cbc_pileup_count(const cbc_pileup_args &A, uint32_t t, const cbc_pileup_sx *X = NULL)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    uint32_t lines = 0, bytes = 0;
    if (cbc_pileup_text_ok(A, t)) {
        uint32_t run = (uint32_t)A.D.sum_off[t];                     /* depth in front of the tile, mod 2^32 */
        uint32_t runf = 0;
        if constexpr (M == CBC_PILEUP_STRAND) runf = (uint32_t)X->sum_off_f[t];
        for (uint32_t r = 0; r < CBC_DEPTH_TILE / 64u; r++) {
            V32 v[M == CBC_PILEUP_STRAND ? 16 : 9], rb, len, len2;
            const Mask k = cbc_pileup_line<W, M>(A, t * CBC_DEPTH_TILE + r * 64u, run, v, rb, len, X, &runf, &len2);
            if (W::ballot(k) == 0ull) continue;
            lines += W::popc64(W::ballot(k));
            bytes += W::reduce_add(len);
        }
    }
    if (t >= A.D.n_tiles) return;
    cbc_store_result<W>(A.D.R.counts + t, bytes, lines);
    if (lines) W::list_add(A.D.ctr, W::splat(1u), W::splat(lines), W::lane() == 0u);
}

/* the line for cbc_lines_store (cbc_depth_body.h): name, '\t' at nl, pos1, '\t' at e[0], the reference byte, '\t' at e[0] + 2, then
 * the eight counts, number s ending at e[s] with a '\t' there; e[8] = len - 1 holds the '\n'; hi / lo: the numbers split */
template <class W>
struct cbc_pileup_ln { typename W::V32 e[9], hi[9], lo[9], rb; uint32_t nl; };

template <class W>
CBC_FN typename W::V32 cbc_line_byte(const cbc_pileup_ln<W> &L, uint32_t i)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    const V32 iv = W::splat(i);
    V32 h = L.hi[8], l = L.lo[8], ee = L.e[8];
    Mask tab = iv == L.nl;
    for (int s = 7; s >= 0; s--) {                                   /* the first number that ends behind byte i */
        const Mask lt = iv < L.e[s];
        h = W::select(lt, L.hi[s], h); l = W::select(lt, L.lo[s], l); ee = W::select(lt, L.e[s], ee);
        tab = tab | (iv == L.e[s]);
    }
    V32 by = cbc_depth_digit<W>(h, l, (ee - 1u) - iv);
    by = W::select(tab | (iv == L.e[0] + 2u), W::splat(9u), by);
    by = W::select(iv == L.e[0] + 1u, L.rb, by);
    return W::select(iv == L.e[8], W::splat(10u), by);
}

/* STRAND: the line goes out in two parts, so that no more numbers are held at once than the plain line holds.  The first is the
 * plain line with a '\t' where its '\n' stood; the second, written behind it, is the seven per-strand numbers: number s ends at
 * e[s] with a '\t' there, e[6] holds the '\n'.  The second part keeps its numbers whole and splits the one a byte belongs to. */
template <class W>
struct cbc_pileup_ln_tab : cbc_pileup_ln<W> {};

template <class W>
CBC_FN typename W::V32 cbc_line_byte(const cbc_pileup_ln_tab<W> &L, uint32_t i)
{
    return W::select(W::splat(i) == L.e[8], W::splat(9u), cbc_line_byte(static_cast<const cbc_pileup_ln<W> &>(L), i));
}

template <class W>
struct cbc_pileup_ln2 { typename W::V32 e[7], v[7]; };

template <class W>
CBC_FN typename W::V32 cbc_line_byte(const cbc_pileup_ln2<W> &L, uint32_t i)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    const V32 iv = W::splat(i);
    V32 x = L.v[6], ee = L.e[6], hi, lo;
    Mask tab = iv != iv;
    for (int s = 5; s >= 0; s--) {                                   /* the first number that ends behind byte i */
        const Mask lt = iv < L.e[s];
        x = W::select(lt, L.v[s], x); ee = W::select(lt, L.e[s], ee);
        tab = tab | (iv == L.e[s]);
    }
    cbc_depth_split<W>(x, hi, lo);
    const V32 by = W::select(tab, W::splat(9u), cbc_depth_digit<W>(hi, lo, (ee - 1u) - iv));
    return W::select(iv == L.e[6], W::splat(10u), by);
}

/* count and write iterate positions, carry `run` and skip empty rounds: they share the writer with the run-text skeleton of
 * cbc_depth_body.h, not its loops */
template <class W, int M = 0>
CBC_FN void cbc_pileup_write(const cbc_pileup_args &A, uint32_t t, const cbc_pileup_sx *X = NULL)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    if (!cbc_pileup_text_ok(A, t)) return;
    const uint32_t bytes = A.D.R.counts[t].nbytes, nl = A.D.name_len;
    const uint64_t o0 = A.D.R.offsets[t];
    if (bytes == 0u || o0 > A.D.R.text_cap || bytes > A.D.R.text_cap - o0) return;
    uint64_t o = o0;
    uint32_t run = (uint32_t)A.D.sum_off[t];
    uint32_t runf = 0;
    if constexpr (M == CBC_PILEUP_STRAND) runf = (uint32_t)X->sum_off_f[t];
    for (uint32_t r = 0; r < CBC_DEPTH_TILE / 64u; r++) {
        V32 v[M == CBC_PILEUP_STRAND ? 16 : 9], rb, len, len2;
        const Mask k = cbc_pileup_line<W, M>(A, t * CBC_DEPTH_TILE + r * 64u, run, v, rb, len, X, &runf, &len2);
        if (W::ballot(k) == 0ull) continue;
        const V32 incl = W::scan_incl_add(len);
        const uint32_t chunk = W::readlane(incl, 63u);
        if (chunk > (o0 + bytes) - o) return;                        /* the counters moved under the count pass */
        typename std::conditional<M == CBC_PILEUP_STRAND, cbc_pileup_ln_tab<W>, cbc_pileup_ln<W> >::type L;
        L.nl = nl; L.rb = rb;
        L.e[0] = cbc_sam_ndig_v<W>(v[0], 1000000000u) + (nl + 1u);
        L.e[1] = L.e[0] + cbc_sam_ndig_v<W>(v[1], 1000000000u) + 3u;
        for (uint32_t s = 2; s < 9u; s++) L.e[s] = L.e[s - 1u] + cbc_sam_ndig_v<W>(v[s], 1000000000u) + 1u;
        for (uint32_t s = 0; s < 9u; s++) cbc_depth_split<W>(v[s], L.hi[s], L.lo[s]);
        if constexpr (M == CBC_PILEUP_STRAND) {
            cbc_lines_store<W>(A.D.R.text + o, incl - len, len - len2, k, A.D.name, nl, L);
            cbc_pileup_ln2<W> L2;
            for (uint32_t s = 0; s < 7u; s++) {
                L2.v[s] = v[9u + s];
                L2.e[s] = (s ? L2.e[s - 1u] + 1u : W::splat(0u)) + cbc_sam_ndig_v<W>(v[9u + s], 1000000000u);
            }
            cbc_lines_store<W>(A.D.R.text + o, incl - len2, len2, k, A.D.name, 0u, L2);
        } else
        cbc_lines_store<W>(A.D.R.text + o, incl - len, len, k, A.D.name, nl, L);
        o += chunk;
    }
}

#endif /* CBC_PILEUP_BODY_H */
