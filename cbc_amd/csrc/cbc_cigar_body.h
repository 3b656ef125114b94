/*
 * cbc_cigar_body.h -- CIGAR, NM and MD in the SAM text, on the device, after the edit-reporting decode of the blocks
 * (cbc_gpu_decode_sam_cigar, include/cbc_gpu.h).
 *
 * The decoder (cbc_decode_body.h, EDITS = true) has left, beside the records, rows and spans, the alignment of every read with
 * indels: nDel matched coordinates dc[] and nIns read indices oi[] (cbc_dec_edits), the mapping cbc_pileup_body.h states.  With
 * T = rl - nIns the elements of a read are, for m = 0 .. T: the inserted read indices in front of aligned base m, then the deleted
 * bases with dc = m, then aligned base m (m < T).  In read-index terms: index q is inserted or aligned; an aligned q of matched
 * coordinate m = q - #{oi < q} has dq = #{dc = m} deleted bases directly in front of it and sits at POS + m + #{dc <= m}; the dT
 * deleted bases with dc = T end the read.
 *   CIGAR  maximal runs of one kind: M (aligned), D (deleted), I (inserted); an inserted run that starts at index 0 or reaches
 *          index rl - 1 is S.  A run of read indices begins at q when q = 0, when q - 1 is of the other kind, or when dq > 0.
 *   MD     over the aligned and deleted elements with the matched-run counter n: a mismatch (the read byte differs from the
 *          reference byte, a plain byte compare) emits n, the reference byte; a deleted run emits n, '^', its reference bytes; the
 *          end emits n.  n = m - ms where ms = the matched coordinate behind the last mismatch, or of the aligned base behind the
 *          last deleted run: inserted bases never show.
 *   NM     mismatches + bases of I runs + deleted bases.
 * rl <= seq_stride <= 256 (cbc_region_block, cbc_sam_keep), so every run length, n and NM has at most three digits.
 *
 *   measure  CBC_CIGAR_WAVES wavefronts per block share its kept reads (the keep rule of cbc_sam_keep); a read is taken by the
 *            whole wavefront, 64 read indices a turn, one lane per index -- the turn of cbc_pileup_events.  Run starts and
 *            mismatches are masks, the token lengths are per lane of a boundary, the sums are wave reductions, the open run
 *            and the MD counter's origin cross the turns as two scalars (cbc_cigar_carry).  A turn without a boundary or a
 *            mismatch -- every turn of a perfect read -- ends behind its ballot.  Out: two words per record,
 *            CIGAR bytes | valid << 31 and NM | MD bytes << 16.  A record whose side / arena entries are not what the decoder
 *            writes is not valid and gets the plain SAM line.
 *   count    the reads-text skeleton of cbc_region_body.h with the line kind CBC_LINE_SAM_CIGAR: the SAM line's length - 1 +
 *            CIGAR bytes + 12 + digits(NM) + MD bytes.
 *   write    the same skeleton; the fields in front of the CIGAR and from the '\t' behind it to the '*' of QUAL go out as
 *            aligned output dwords as in cbc_sam_emit (SEQ funnel-shifted from wherever the CIGAR leaves it); the tokens are
 *            computed again turn by turn, placed by a wave prefix sum of their lengths and stored by their own lane, bytes
 *            (a line has about 4 + 20 of them).  No token byte is stored past the measured field; the recomputed lengths
 *            are compared with the measured ones (W::expect_eq).
 * Range tests are written without base + length sums.  Written against the wave policy (W = WaveGPU in cbc_gpu.hip, the
 * lock-step emulation in tests/cigar_emu).
 */
#ifndef CBC_CIGAR_BODY_H
#define CBC_CIGAR_BODY_H

#include <stdint.h>
#include "../../include/cbc_gpu.h"
#include "cbc_region_body.h"
#include "cbc_sam_body.h"

#define CBC_CIGAR_WAVES 4u              /* wavefronts that share one block's reads in the measure pass */
#define CBC_CIGAR_VALID 0x80000000u

struct cbc_cigar_args {
    cbc_sam_args S;               /* as for the SAM passes                                                                        */
    const uint32_t *side;         /* the EDITS decoder's side array and arena (cbc_dec_edits)                                    */
    const uint16_t *arena;
    const uint8_t  *ref;          /* the device reference                                                                        */
    uint32_t *meas;               /* two words per record: the measure pass's out, the count and the write pass's in             */
    uint64_t arena_entries, ref_bytes;
    uint32_t per_read, reserved;
};

struct cbc_cigar_blk : cbc_sam_blk {
    const uint32_t *side; const uint16_t *arena; const uint8_t *refb; uint32_t *meas;
    uint32_t cap, ref_lim;        /* the block's arena entries; reference bytes from its window's first on */
};

/* one kept read, wave-uniform: its lengths, its lists (the first 64 entries of each in a register) and what ends it */
template <class W>
struct cbc_cigar_read {
    uint32_t rl, lp, nd, ni, T, dT, lastins;
    const uint16_t *ar; const uint8_t *row;
    typename W::V32 dcv, oiv;
};

struct cbc_cigar_carry { uint32_t rs, ms; };     /* first read index of the open run; the matched coordinate MD counts from */

template <class W>
struct cbc_cigar_turn {
    typename W::Mask bnd, ev, mis;               /* a run begins at q > 0; an MD token begins at q; q is a mismatch */
    typename W::V32 clen, cop, dq, n, rb, x, ctok, mtok;
    bool any;
};

template <int LINE>
CBC_FN cbc_cigar_blk cbc_text_block(const cbc_cigar_args &A, uint32_t blk)
{
    cbc_cigar_blk X = {};
    static_cast<cbc_sam_blk &>(X) = cbc_sam_block(A.S, blk);
    const cbc_dec_block_desc *bd = A.S.R.blocks + blk;
    /* the block's part of the arena, by the decoder's own test (B.ok: rec_base inside n_recs) */
    const uint64_t rec_base = X.B.ok ? bd->rec_base : 0u, ref_off = bd->ref_off;
    const uint64_t cap64 = (uint64_t)X.B.n * A.per_read, base64 = rec_base * A.per_read;
    X.B.ok = X.B.ok && A.per_read >= 1u && A.per_read <= CBC_EDITS_MAX && base64 <= A.arena_entries && cap64 <= A.arena_entries - base64 &&
             ref_off <= A.ref_bytes;
    const uint64_t ref_avail = X.B.ok ? A.ref_bytes - ref_off : 0u;
    X.cap = X.B.ok ? (uint32_t)cap64 : 0u;
    X.ref_lim = ref_avail > 0xffffffffull ? 0xffffffffu : (uint32_t)ref_avail;
    X.arena = A.arena + (X.B.ok ? base64 : 0u);
    X.side = A.side + 2u * rec_base;
    X.meas = A.meas + 2u * rec_base;
    X.refb = A.ref + (X.B.ok ? ref_off : 0u);
    return X;
}

/* the keep flags of the SAM line, and the measured words of the kept records */
template <class W>
CBC_FN typename W::Mask cbc_text_keep(const cbc_cigar_args &A, const cbc_cigar_blk &X, uint32_t r0, cbc_text_grp<W> &G)
{
    const typename W::Mask k = cbc_sam_keep<W>(A.S, X, r0, G.rlv, G.lp, G.fl);
    const typename W::V32 at = (W::lane() + r0) * 2u;
    G.xa = W::load32(X.meas, at, k, 0u);
    G.xb = W::load32(X.meas, at + 1u, k, 0u);
    return k;
}

/* The read's side words checked against everything the passes rely on; false: the plain SAM line.  Counts above 255, entries
 * outside the block's arena, dc not ascending or above T, oi not strictly ascending or >= rl, rl = 0, and a read whose
 * T + nDel reference bytes do not lie inside the uploaded reference. */
template <class W>
CBC_FN bool cbc_cigar_open(const cbc_cigar_blk &X, const uint8_t *row, uint32_t rl, uint32_t lp, uint32_t e0, uint32_t cnt,
                           cbc_cigar_read<W> &R)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    const V32 ln = W::lane();
    const uint32_t nd = cnt & 0xffffu, ni = cnt >> 16;
    if (rl == 0u || nd > 255u || ni > 255u || e0 > X.cap || nd + ni > X.cap - e0 || ni > rl) return false;
    const uint32_t T = rl - ni;
    if (lp < 1u || lp - 1u > X.ref_lim || T + nd > X.ref_lim - (lp - 1u)) return false;
    R.rl = rl; R.lp = lp; R.nd = nd; R.ni = ni; R.T = T; R.dT = 0u; R.lastins = 0u; R.row = row;
    R.ar = X.arena + e0;                                             /* dc = ar[0 .. nd), oi = ar[nd .. nd + ni) */
    R.dcv = W::load16(R.ar, ln, ln < nd); R.oiv = W::load16(R.ar, ln + nd, ln < ni);
    uint64_t bad = 0u;
    uint32_t prev = 0u;
    for (uint32_t c = 0; c < nd; c += 64u) {
        const Mask m = (ln + c) < nd;
        const V32 v = c ? W::load16(R.ar, ln + c, m) : R.dcv;
        const V32 p = W::shift_up1(v, prev);
        bad |= W::ballot(m & ((v < p) | (v > T)));
        R.dT += W::popc64(W::ballot(m & (v == T)));
        prev = W::readlane(v, 63u);
    }
    prev = 0u;                                                       /* oi + 1 against its predecessor's: strictly ascending */
    for (uint32_t c = 0; c < ni; c += 64u) {
        const Mask m = (ln + c) < ni;
        const V32 v = c ? W::load16(R.ar, ln + (nd + c), m) : R.oiv;
        const V32 w = v + 1u, p = W::shift_up1(w, prev);
        bad |= W::ballot(m & ((w <= p) | (v >= rl)));
        prev = W::readlane(w, 63u);
    }
    if (bad) return false;
    if (ni) R.lastins = W::read_uni16(R.ar, nd + ni - 1u) == rl - 1u ? 1u : 0u;
    return true;
}

/* digits of x < 1000 */
template <class W>
CBC_FN typename W::V32 cbc_cigar_ndig(const typename W::V32 &x) { return cbc_sam_ndig_v<W>(x, 100u); }

/* decimal digit j (0 = the last) of v < 1000 as ASCII: floor(v / 10^j) by multiply-shift, exact as in cbc_sam_digits */
template <class W>
CBC_FN typename W::V32 cbc_cigar_digit(const typename W::V32 &v, const typename W::V32 &j)
{
    typedef typename W::V32 V32;
    const V32 M = W::select(j == 1u, W::splat(429496730u), W::splat(42949673u));
    const V32 q = W::select(j == 0u, v, W::mulhi(v, M));
    return (q - W::mulhi(q, W::splat(429496730u)) * 10u) + 48u;
}

/* read indices [b, b + 64) of the read: what every lane's index begins.  C is advanced. */
template <class W>
CBC_FN void cbc_cigar_step(const cbc_cigar_blk &X, const cbc_cigar_read<W> &R, uint32_t b, cbc_cigar_carry &C, cbc_cigar_turn<W> &U)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    const V32 ln = W::lane(), q = ln + b, zero = W::splat(0u), one = W::splat(1u);
    const Mask inr = q < R.rl;
    V32 nb = zero, ii = zero, pi = zero;
    for (uint32_t i = 0; i < R.ni; i++) {
        const uint32_t oi = i < 64u ? W::readlane(R.oiv, i) : W::read_uni16(R.ar, R.nd + i);
        nb = nb + W::select(q > oi, one, zero);
        ii = W::select(q == oi, one, ii);
        pi = W::select(q == oi + 1u, one, pi);
    }
    const Mask isins = ii != 0u, pvins = pi != 0u;
    const Mask al = inr & !isins;
    const V32 m = q - nb;                                            /* matched coordinate of an aligned q */
    V32 sh = zero, dq = zero;
    for (uint32_t d = 0; d < R.nd; d++) {
        const uint32_t dc = d < 64u ? W::readlane(R.dcv, d) : W::read_uni16(R.ar, d);
        sh = sh + W::select(m >= dc, one, zero);
        dq = dq + W::select(m == dc, one, zero);
    }
    dq = W::select(al, dq, zero);
    U.dq = dq;
    U.x = m + sh;                                                    /* offset from POS; x - dq .. x - 1: the deleted bases in front */
    U.rb = W::load8(X.refb, U.x + (R.lp - 1u), al);                  /* cbc_cigar_open: lp - 1 + T + nd inside the reference */
    const V32 cb = W::load8(R.row, q, al);
    U.mis = al & (cb != U.rb);
    const Mask hasd = dq != 0u;
    const Mask nins = !isins, npv = !pvins;
    const Mask st = inr & ((isins & npv) | (nins & pvins) | hasd);    /* q - 1 is of the other kind, or deleted bases lie between */
    U.bnd = st & ((q != 0u) | hasd);                                 /* deleted bases in front of index 0: a token without a run */
    U.ev = U.mis | hasd;
    U.ctok = zero; U.mtok = zero; U.clen = zero; U.cop = zero; U.n = zero;
    U.any = W::ballot(U.bnd | U.ev) != 0ull;
    if (!U.any) return;                                              /* the short path: nothing begins in this turn */
    {   /* the run that ends at q - 1 began at the last start in front of q */
        const V32 incl = W::scan_incl_max(W::select(U.bnd, q, zero));
        const V32 run = W::select(incl > C.rs, incl, W::splat(C.rs));
        const V32 ps = W::shift_up1(run, C.rs);
        U.clen = q - ps;
        U.cop = W::select(pvins, W::select(ps == 0u, W::splat((uint32_t)'S'), W::splat((uint32_t)'I')), W::splat((uint32_t)'M'));
        U.ctok = W::select(U.bnd, W::select(U.clen != 0u, cbc_cigar_ndig<W>(U.clen) + 1u, zero) + W::select(hasd, cbc_cigar_ndig<W>(dq) + 1u, zero), zero);
        C.rs = W::readlane(run, 63u);
    }
    {   /* the matched bases in front of the token: from behind the last mismatch, or from the base behind the last deleted run */
        const V32 incl = W::scan_incl_max(W::select(U.ev, m + W::select(U.mis, one, zero), zero));
        const V32 org = W::select(incl > C.ms, incl, W::splat(C.ms));
        const V32 po = W::shift_up1(org, C.ms);
        U.n = m - po;
        U.mtok = W::select(U.ev, cbc_cigar_ndig<W>(U.n) + 1u + W::select(hasd, dq + W::select(U.mis, W::splat(2u), zero), zero), zero);
        C.ms = W::readlane(org, 63u);
    }
}

/* what ends the read: the open run, the deleted bases at T, the last count of MD */
struct cbc_cigar_end { uint32_t clen, cop, nf, ctok, mtok; };

template <class W>
CBC_FN cbc_cigar_end cbc_cigar_finish(const cbc_cigar_read<W> &R, const cbc_cigar_carry &C)
{
    cbc_cigar_end E;
    E.clen = R.rl - C.rs; E.cop = R.lastins ? (uint32_t)'S' : (uint32_t)'M';
    E.nf = R.T - C.ms;
    E.ctok = cbc_sam_ndig(E.clen, 100u) + 1u + (R.dT ? cbc_sam_ndig(R.dT, 100u) + 1u : 0u);
    E.mtok = cbc_sam_ndig(E.nf, 100u) + (R.dT ? R.dT + 2u : 0u);
    return E;
}

/* ---- measure ----------------------------------------------------------------------------------------------------------- */
template <class W>
CBC_FN void cbc_cigar_measure(const cbc_cigar_args &A, uint32_t blk, uint32_t wave, uint32_t n_waves)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    const cbc_cigar_blk X = cbc_text_block<CBC_LINE_SAM_CIGAR>(A, blk);
    if (!X.B.ok || n_waves == 0u || wave >= n_waves) return;
    const V32 ln = W::lane(), zero = W::splat(0u);
    uint32_t nq = 0;                                                 /* kept reads of the block so far */
    for (uint32_t r0 = 0; r0 < X.B.n; r0 += 64u) {
        V32 rlv, lp, fl;
        const Mask k = cbc_sam_keep<W>(A.S, X, r0, rlv, lp, fl);
        const V32 sd0 = W::load32(X.side, (ln + r0) * 2u, k, 0u), sd1 = W::load32(X.side, (ln + r0) * 2u + 1u, k, 0u);
        uint64_t bits = W::ballot(k);
        while (bits) {
            const uint32_t j = W::ctz64(bits);
            bits &= bits - 1u;
            if ((nq++ % n_waves) != wave) continue;
            cbc_cigar_read<W> R;
            uint32_t w0 = 0u, w1 = 0u;
            if (cbc_cigar_open<W>(X, X.B.rows + (uint64_t)(r0 + j) * X.B.stride, W::readlane(rlv, j), W::readlane(lp, j),
                                  W::readlane(sd0, j), W::readlane(sd1, j), R)) {
                cbc_cigar_carry C = { 0u, 0u };
                uint32_t cg = 0u, md = 0u, nm = R.nd;
                for (uint32_t b = 0; b < R.rl; b += 64u) {
                    cbc_cigar_turn<W> U;
                    cbc_cigar_step<W>(X, R, b, C, U);
                    if (!U.any) continue;
                    cg += W::reduce_add(U.ctok); md += W::reduce_add(U.mtok);
                    nm += W::popc64(W::ballot(U.mis)) + W::reduce_add(W::select(U.bnd & (U.cop == (uint32_t)'I'), U.clen, zero));
                }
                const cbc_cigar_end E = cbc_cigar_finish<W>(R, C);
                w0 = (cg + E.ctok) | CBC_CIGAR_VALID; w1 = nm | ((md + E.mtok) << 16);       /* below 2^12, 2^10, 2^12 */
            }
            W::write_uni(X.meas, 2u * (r0 + j), w0); W::write_uni(X.meas, 2u * (r0 + j) + 1u, w1);
        }
    }
}

/* ---- the line ---------------------------------------------------------------------------------------------------------- */
template <class W>
CBC_FN typename W::V32 cbc_line_len(cbc_line<CBC_LINE_SAM_CIGAR>, const cbc_cigar_blk &X, const cbc_text_grp<W> &G)
{
    typedef typename W::V32 V32;
    const V32 extra = (G.xa & 0x7fffffffu) + 11u + cbc_cigar_ndig<W>(G.xb & 0xffffu) + (G.xb >> 16);
    return cbc_sam_line_len<W>(X, G.rlv, G.lp, G.fl) + W::select((G.xa & CBC_CIGAR_VALID) != 0u, extra, W::splat(0u));
}

/* byte t of a CIGAR token: the run's length and letter (none for clen = 0), then the deleted run's length and 'D' */
template <class W>
CBC_FN typename W::V32 cbc_cigar_ctok_byte(const typename W::V32 &clen, const typename W::V32 &cop, const typename W::V32 &dq,
                                           const typename W::V32 &t)
{
    typedef typename W::V32 V32;
    const V32 h = W::select(clen != 0u, cbc_cigar_ndig<W>(clen) + 1u, W::splat(0u)), d2 = cbc_cigar_ndig<W>(dq);
    V32 by = W::splat((uint32_t)'D');
    by = W::select(t < h + d2, cbc_cigar_digit<W>(dq, (h + d2 - 1u) - t), by);
    by = W::select(t + 1u == h, cop, by);
    return W::select(t + 1u < h, cbc_cigar_digit<W>(clen, (h - 2u) - t), by);
}

/* byte t of an MD token: n; with deleted bases in front '^' and their reference bytes; for a mismatch ('0' behind a deleted run
 * and) the reference byte.  x = the offset from POS of the aligned base the token belongs to. */
template <class W>
CBC_FN typename W::V32 cbc_cigar_mtok_byte(const cbc_cigar_blk &X, uint32_t lp, const typename W::V32 &n, const typename W::V32 &dq,
                                           const typename W::V32 &rb, const typename W::V32 &x, const typename W::V32 &t,
                                           const typename W::Mask &m)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    const V32 dn = cbc_cigar_ndig<W>(n);
    const V32 u = t - (dn + 1u);                                     /* index among the deleted bases */
    const Mask isd = m & (t > dn) & (u < dq);
    const V32 db = W::load8(X.refb, ((x - dq) + u) + (lp - 1u), isd);
    V32 by = W::select((dq != 0u) & (u == dq), W::splat((uint32_t)'0'), rb);
    by = W::select(isd, db, by);
    by = W::select((dq != 0u) & (t == dn), W::splat((uint32_t)'^'), by);
    return W::select(t < dn, cbc_cigar_digit<W>(n, (dn - 1u) - t), by);
}

/* one read's line with CIGAR and tags at text[o ..]: the whole wavefront */
template <class W>
CBC_FN void cbc_cigar_emit(uint8_t *text, uint64_t o, const cbc_cigar_blk &X, const cbc_cigar_read<W> &R, uint32_t pos,
                           uint32_t flag, uint32_t len, uint32_t cl, uint32_t nm, uint32_t mdl, const typename W::V32 &tabc)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    const V32 ln = W::lane(), zero = W::splat(0u);
    const uint32_t rl = R.rl, nl = X.nl, dnm = cbc_sam_ndig(nm, 100u);
    cbc_sam_line L;                                                  /* the plain line's fields */
    L.nl = nl; L.rl = rl;
    L.b = 2u + cbc_sam_ndig(flag, 10000u); L.c = L.b + 1u; L.e = L.c + nl + 1u;
    L.f = L.e + cbc_sam_ndig(pos, 1000000000u); L.g = L.f + 13u; L.n = L.g + rl + 3u;
    /* the CIGAR takes the place of the '*' at cb; SEQ begins at g2; te: the '\t' in front of NM; all below 2^13 */
    const uint32_t cb = L.f + 5u, g2 = L.g + (cl - 1u), te = g2 + rl + 2u, md0 = te + 12u + dnm;
    W::expect_eq(md0 + mdl + 1u, len, "SAM line length with CIGAR differs between the count and the write pass");
    if (cl == 0u || md0 + mdl + 1u != len) return;
    const V32 tab = cbc_sam_digits<W>(tabc, pos, flag);
    const uint32_t s = (uint32_t)(o & 3u);                           /* line byte i sits at base[s + i] */
    uint8_t *base = text + (o - s);
    {   /* line bytes [0, cb) and [cb + cl, te) as in cbc_sam_emit: plain line byte i, or i - (cl - 1) behind the CIGAR */
        const uint32_t sg = s + g2, Q = (sg + 3u) >> 2, m8 = 8u * (4u * Q - sg);
        const uint32_t nwr = (rl + 3u) >> 2, nd = (s + te + 3u) >> 2;
        const uint32_t *row32 = (const uint32_t *)R.row;
        for (uint32_t k0 = 0; k0 < nd; k0 += 64u) {
            const V32 k = ln + k0;
            const Mask act = k < nd;
            const V32 jl = k - Q, jh = jl + 1u;
            const V32 w0 = W::load32(row32, jl, act & (jl < nwr), 0u), w1 = W::load32(row32, jh, act & (jh < nwr), 0u);
            const V32 v = W::funnel_shr(w1, w0, m8);
            const V32 i0 = k * 4u - s;
            V32 out = zero;
            Mask full = act;
            for (uint32_t t = 0; t < 4u; t++) {
                const V32 i = i0 + t;
                const V32 ip = W::select(i < cb, i, i - (cl - 1u));
                const V32 by = W::select((i - g2) < rl, (v >> (8u * t)) & 0xffu, cbc_sam_field_byte<W>(L, X.name, tab, ip));
                out = out | (by << (8u * t));
                full = full & ((i < cb) | ((i >= cb + cl) & (i < te)));
            }
            W::store32_bytes(base, k * 4u, out, full);
            const Mask part = act & !full;
            if (W::ballot(part) != 0ull)
                for (uint32_t t = 0; t < 4u; t++) {
                    const V32 i = i0 + t;
                    W::store8(base, k * 4u + t, (out >> (8u * t)) & 0xffu, part & ((i < cb) | ((i >= cb + cl) & (i < te))));
                }
        }
    }
    uint8_t *line = text + o;
    {   /* "\tNM:i:" n "\tMD:Z:" one byte per lane, and the '\n' */
        const V32 u = ln - (6u + dnm);
        const V32 c1 = (W::select(ln < 4u, W::splat(0x3a4d4e09u), W::splat(0x00003a69u)) >> ((ln & 3u) * 8u)) & 0xffu;
        const V32 c2 = (W::select(u < 4u, W::splat(0x3a444d09u), W::splat(0x00003a5au)) >> ((u & 3u) * 8u)) & 0xffu;
        V32 by = W::select(ln < 6u + dnm, cbc_cigar_digit<W>(W::splat(nm), (5u + dnm) - ln), c2);
        by = W::select(ln < 6u, c1, by);
        by = W::select(ln == 63u, W::splat(10u), by);
        W::store8(line, W::select(ln == 63u, W::splat(len - 1u), ln + te), by, (ln < 12u + dnm) | (ln == 63u));
    }
    /* the tokens, turn by turn as measured */
    cbc_cigar_carry C = { 0u, 0u };
    uint32_t co = 0u, mo = 0u, nmr = R.nd;
    for (uint32_t b = 0; b < rl; b += 64u) {
        cbc_cigar_turn<W> U;
        cbc_cigar_step<W>(X, R, b, C, U);
        if (!U.any) continue;
        nmr += W::popc64(W::ballot(U.mis)) + W::reduce_add(W::select(U.bnd & (U.cop == (uint32_t)'I'), U.clen, zero));
        if (W::ballot(U.bnd) != 0ull) {
            const V32 incl = W::scan_incl_add(U.ctok);
            const V32 at = (incl - U.ctok) + co;
            for (uint32_t t = 0; t < 8u; t++) {
                const Mask m = U.bnd & (U.ctok > t) & ((at + t) < cl);
                if (W::ballot(m) == 0ull) break;
                W::store8(line, at + (cb + t), cbc_cigar_ctok_byte<W>(U.clen, U.cop, U.dq, W::splat(t)), m);
            }
            co += W::readlane(incl, 63u);
        }
        if (W::ballot(U.ev) != 0ull) {
            const V32 incl = W::scan_incl_add(U.mtok);
            const V32 at = (incl - U.mtok) + mo;
            for (uint32_t t = 0; t < 261u; t++) {
                const Mask m = U.ev & (U.mtok > t) & ((at + t) < mdl);
                if (W::ballot(m) == 0ull) break;
                W::store8(line, at + (md0 + t), cbc_cigar_mtok_byte<W>(X, R.lp, U.n, U.dq, U.rb, U.x, W::splat(t), m), m);
            }
            mo += W::readlane(incl, 63u);
        }
    }
    const cbc_cigar_end E = cbc_cigar_finish<W>(R, C);
    {   /* the open run, and the deleted bases at T: a byte per lane */
        const Mask m = (ln < E.ctok) & ((ln + co) < cl);
        W::store8(line, ln + (cb + co), cbc_cigar_ctok_byte<W>(W::splat(E.clen), W::splat(E.cop), W::splat(R.dT), ln), m);
        for (uint32_t t0 = 0; t0 < E.mtok; t0 += 64u) {              /* n, then '^', the bases, '0' (the byte behind is cut off) */
            const V32 t = ln + t0;
            const Mask mm = (t < E.mtok) & ((t + mo) < mdl);
            W::store8(line, t + (md0 + mo), cbc_cigar_mtok_byte<W>(X, R.lp, W::splat(E.nf), W::splat(R.dT), zero, W::splat(R.T + R.nd), t, mm), mm);
        }
    }
    W::expect_eq(co + E.ctok, cl, "CIGAR bytes differ between the measure and the write pass");
    W::expect_eq(mo + E.mtok, mdl, "MD bytes differ between the measure and the write pass");
    W::expect_eq(nmr, nm, "NM differs between the measure and the write pass");
}

template <class W>
CBC_FN void cbc_line_emit(cbc_line<CBC_LINE_SAM_CIGAR>, uint8_t *text, uint64_t o, const cbc_cigar_blk &X, uint32_t r0, uint32_t j,
                          const cbc_text_grp<W> &G)
{
    const uint32_t len = W::readlane(G.tl, j), at = W::readlane(G.incl, j) - len;
    const uint32_t w0 = W::readlane(G.xa, j), w1 = W::readlane(G.xb, j), rl = W::readlane(G.rlv, j), lp = W::readlane(G.lp, j);
    const uint8_t *row = X.B.rows + (uint64_t)(r0 + j) * X.B.stride;
    cbc_cigar_read<W> R;
    if ((w0 & CBC_CIGAR_VALID) == 0u) {
        cbc_sam_emit<W>(text, o + at, row, rl, X.ws + lp, W::readlane(G.fl, j), X.name, X.nl, len, cbc_sam_const_tab<W>());
        return;
    }
    const bool ok = cbc_cigar_open<W>(X, row, rl, lp, W::read_uni(X.side, 2u * (r0 + j)), W::read_uni(X.side, 2u * (r0 + j) + 1u), R);
    W::expect_eq(ok ? 1u : 0u, 1u, "a measured record is not valid in the write pass");
    if (!ok) return;
    cbc_cigar_emit<W>(text, o + at, X, R, X.ws + lp, W::readlane(G.fl, j), len, w0 & 0x7fffffffu, w1 & 0xffffu, w1 >> 16,
                      cbc_sam_const_tab<W>());
}

template <class W>
CBC_FN void cbc_sam_cigar_count(const cbc_cigar_args &A, uint32_t blk) { cbc_text_count<W, CBC_LINE_SAM_CIGAR>(A, A.S.R, blk); }
template <class W>
CBC_FN void cbc_sam_cigar_write(const cbc_cigar_args &A, uint32_t blk, uint32_t wave, uint32_t n_waves)
{
    cbc_text_write<W, CBC_LINE_SAM_CIGAR>(A, A.S.R, blk, wave, n_waves);
}

#endif /* CBC_CIGAR_BODY_H */
