/*
 * cbc_sam_body.h -- SAM text on the device, after the decode of the blocks (cbc_gpu_decode_sam, include/cbc_gpu.h;
 * DESIGN.md section 4.12).
 *
 * The decode kernel has left every record of the blocks in the context's arenas (plain decoder for a full decode, the
 * span-reporting one for a region).  Two passes, the reads-text skeleton of cbc_region_body.h with the keep rule, the line length
 * and the line of this file, turn them into one line per read:
 *     *\t<FLAG>\t<RNAME>\t<POS>\t255\t*\t*\t0\t0\t<SEQ>\t*\n          20 + digits(FLAG) + len(RNAME) + digits(POS) + rlen bytes
 *   count  one wavefront per block, one lane per record: keep flag (every record; with a region the rule of
 *          cbc_region_keep), line length (digit counts by compares), kept reads and text bytes by wave reductions into a
 *          cbc_block_result so that cbc_scan_sizes_kernel places the blocks in the text (64-bit offsets);
 *   write  `n_waves` wavefronts per block share its kept reads; a line is written by the whole wavefront, one aligned
 *          OUTPUT dword per lane.  A byte of the dword that lies in SEQ comes from two row words through a funnel shift (any
 *          output alignment); a byte of the fields around SEQ comes from a 34-entry table held one entry per lane (the
 *          decimal digits of POS and FLAG, made lane-parallel by multiply-shift division, and the constant fields) or from
 *          the device copy of the name table.  Byte stores only for the at most 3 + 3 bytes a line shares with its
 *          neighbours.
 * POS = window_start + local POS.  SAM allows POS up to 2^31 - 1: a block whose window starts past that is not written and
 * a record whose POS would pass it is not kept (the host refuses such a container before anything is launched).
 * Written against the wave policy (W = WaveGPU in cbc_gpu.hip, the lock-step emulation in tests/sam_emu).
 */
#ifndef CBC_SAM_BODY_H
#define CBC_SAM_BODY_H

#include <stdint.h>
#include "../../include/cbc_gpu.h"
#include "cbc_region_body.h"

struct cbc_sam_args {
    cbc_region_args R;            /* records, rows, blocks, window starts, decode results, counts, offsets, text: as for the
                                   * region passes; beg / end are read only when `region` is set                            */
    const uint32_t *block_name;   /* per block: offset and length of its contig's name in names[] (two words)              */
    const uint8_t  *names;
    uint32_t names_bytes, region;
};

struct cbc_sam_blk {
    cbc_region_blk B;
    const uint8_t *name;
    uint32_t ws, nl;
};

CBC_FN cbc_sam_blk cbc_sam_block(const cbc_sam_args &A, uint32_t blk)
{
    cbc_sam_blk S;
    S.B = cbc_region_block(A.R, blk);
    const uint64_t ws = A.R.window_start[blk];
    const uint32_t noff = A.block_name[2u * blk];
    S.nl = A.block_name[2u * blk + 1u];
    /* the name inside the table (no offset + length sum), the window start a POS, rows on a word boundary */
    S.B.ok = S.B.ok && ws <= CBC_SAM_MAX_POS && S.nl <= CBC_SAM_MAX_NAME && noff <= A.names_bytes && S.nl <= A.names_bytes - noff &&
             (A.R.blocks[blk].seq_base & 3u) == 0u;
    S.ws = (uint32_t)ws;
    S.name = A.names + (S.B.ok ? noff : 0u);
    return S;
}

/* decimal digits of x by compares: `hi` = the largest power of ten tested (10^4 for FLAG, 10^9 for POS) */
template <class W>
CBC_FN typename W::V32 cbc_sam_ndig_v(const typename W::V32 &x, uint32_t hi)
{
    typename W::V32 d = W::splat(1u);
    const typename W::V32 one = W::splat(1u), zero = W::splat(0u);
    for (uint32_t p = 10u;; p *= 10u) {
        d = d + W::select(x >= p, one, zero);
        if (p == hi) break;
    }
    return d;
}
CBC_FN uint32_t cbc_sam_ndig(uint32_t x, uint32_t hi)
{
    uint32_t d = 1u;
    for (uint32_t p = 10u;; p *= 10u) {
        d += x >= p ? 1u : 0u;
        if (p == hi) break;
    }
    return d;
}

/* keep flags of records [r0, r0 + 64) with their length, local POS and FLAG */
template <class W>
CBC_FN typename W::Mask cbc_sam_keep(const cbc_sam_args &A, const cbc_sam_blk &S, uint32_t r0, typename W::V32 &rlv,
                                     typename W::V32 &lp, typename W::V32 &fl)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    const V32 ln = W::lane();
    const Mask m = (ln + r0) < S.B.n;
    V32 w1, off, span;
    W::load_rec(S.B.recs4, ln + r0, m, lp, w1, off, span);
    rlv = w1 >> 16;
    fl = w1 & 0xffffu;
    Mask k = m & (rlv <= S.B.stride) & (lp <= CBC_SAM_MAX_POS - S.ws);
    if (A.region) {
        V32 rl2;
        k = k & cbc_region_keep<W>(S.B, r0, rl2);
    }
    return k;
}

template <class W>
CBC_FN typename W::V32 cbc_sam_line_len(const cbc_sam_blk &S, const typename W::V32 &rlv, const typename W::V32 &lp,
                                        const typename W::V32 &fl)
{
    return rlv + (20u + S.nl) + cbc_sam_ndig_v<W>(fl, 10000u) + cbc_sam_ndig_v<W>(lp + S.ws, 1000000000u);
}

/* The table of the bytes around NAME and SEQ, one entry per lane:
 *   0..9 POS digits (least significant first)   10..14 FLAG digits   15..27 "\t255\t*\t*\t0\t0\t"   28..29 "*\t"
 *   30..32 "\t*\n"   33 '\t'
 * the constant part (lanes 15..33), made once per wavefront */
template <class W>
CBC_FN typename W::V32 cbc_sam_const_tab()
{
    typedef typename W::V32 V32;
    const V32 t = W::lane() - 15u;                                 /* lanes below 15 are overwritten with digits */
    const V32 q = t >> 2;
    const V32 w = W::select(q == 0u, W::splat(0x35353209u),        /* \t 2 5 5 */
                  W::select(q == 1u, W::splat(0x2a092a09u),        /* \t * \t * */
                  W::select(q == 2u, W::splat(0x30093009u),        /* \t 0 \t 0 */
                  W::select(q == 3u, W::splat(0x09092a09u),        /* \t | * \t | \t */
                                     W::splat(0x00090a2au)))));    /* * \n | \t */
    return (w >> ((t & 3u) * 8u)) & 0xffu;
}

/* lanes 0..14 of the table for one read: ASCII digits of POS (<= 2^31 - 1) and FLAG (< 2^16).
 * POS = hi * 10^5 + lo, so every lane extracts digit j (0..4) of a value v < 10^5:
 *   floor(v / 10^j) = (v * M_j) >> 32 with M_j = ceil(2^32 / 10^j): exact while v * (M_j * 10^j - 2^32) < 2^32, and the
 *   error terms are 4, 4, 704, 2704 for j = 1..4 (v * 2704 < 2^29);  q mod 10 = q - 10 * ((q * M_1) >> 32) likewise. */
template <class W>
CBC_FN typename W::V32 cbc_sam_digits(const typename W::V32 &tabc, uint32_t pos, uint32_t flag)
{
    typedef typename W::V32 V32;
    const V32 ln = W::lane();
    const uint32_t hi = pos / 100000u, lo = pos - hi * 100000u;
    const V32 v = W::select(ln < 5u, W::splat(lo), W::select(ln < 10u, W::splat(hi), W::splat(flag)));
    const V32 j = W::select(ln < 5u, ln, W::select(ln < 10u, ln - 5u, ln - 10u));
    const V32 M = W::select(j == 1u, W::splat(429496730u), W::select(j == 2u, W::splat(42949673u),
                  W::select(j == 3u, W::splat(4294968u), W::splat(429497u))));
    const V32 q = W::select(j == 0u, v, W::mulhi(v, M));
    const V32 dg = q - W::mulhi(q, W::splat(429496730u)) * 10u;
    return W::select(ln < 15u, dg + 48u, tabc);
}

/* where the fields of one line begin (byte indices in the line) */
struct cbc_sam_line {
    uint32_t b, c, e, f, g, n;     /* '\t' after FLAG, NAME, '\t' after NAME + 1, end of POS, SEQ, line length */
    uint32_t nl, rl;
};

/* byte i of the line for an i outside SEQ (an i past the line gives a byte nobody stores) */
template <class W>
CBC_FN typename W::V32 cbc_sam_field_byte(const cbc_sam_line &L, const uint8_t *name, const typename W::V32 &tab,
                                          const typename W::V32 &i)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    V32 idx = (i - (L.g + L.rl)) + 30u;                             /* "\t*\n" behind SEQ                 */
    idx = W::select(i < L.g, (i - L.f) + 15u, idx);                 /* the constant fields behind POS     */
    idx = W::select(i < L.f, (L.f - 1u) - i, idx);                  /* POS, most significant digit first  */
    idx = W::select(i < L.e, W::splat(33u), idx);                   /* '\t' behind NAME (NAME: below)     */
    idx = W::select(i < L.c, W::splat(33u), idx);                   /* '\t' behind FLAG                   */
    idx = W::select(i < L.b, (L.b + 9u) - i, idx);                  /* FLAG: digit b - 1 - i at lane 10 + */
    idx = W::select(i < 2u, i + 28u, idx);                          /* "*\t"                              */
    const V32 t = W::lane_gather(tab, idx & 63u);
    const V32 x = i - L.c;
    const Mask isname = x < L.nl;
    return W::select(isname, W::load8(name, x, isname), t);
}

/* one read's line at text[o ..]: the whole wavefront, one aligned output dword per lane and round */
template <class W>
CBC_FN void cbc_sam_emit(uint8_t *text, uint64_t o, const uint8_t *row, uint32_t rl, uint32_t pos, uint32_t flag,
                         const uint8_t *name, uint32_t nl, uint32_t len, const typename W::V32 &tabc)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    const V32 ln = W::lane();
    cbc_sam_line L;
    L.nl = nl; L.rl = rl;
    L.b = 2u + cbc_sam_ndig(flag, 10000u); L.c = L.b + 1u; L.e = L.c + nl + 1u;
    L.f = L.e + cbc_sam_ndig(pos, 1000000000u); L.g = L.f + 13u; L.n = L.g + rl + 3u;       /* all below 600: no wrap */
    W::expect_eq(L.n, len, "SAM line length differs between the count and the write pass");
    if (L.n != len) return;
    const V32 tab = cbc_sam_digits<W>(tabc, pos, flag);
    const uint32_t s = (uint32_t)(o & 3u);                         /* line byte i sits at base[s + i] */
    uint8_t *base = text + (o - s);
    /* SEQ byte r of the row is line byte g + r: dword k holds row bytes 4 (k - Q) + m .., m = 4 Q - (s + g) in 0..3 */
    const uint32_t sg = s + L.g, Q = (sg + 3u) >> 2, m8 = 8u * (4u * Q - sg);
    const uint32_t nwr = (rl + 3u) >> 2, nd = (s + L.n + 3u) >> 2;  /* row words that hold bases (<= stride / 4); dwords touched */
    const uint32_t *row32 = (const uint32_t *)row;
    for (uint32_t k0 = 0; k0 < nd; k0 += 64u) {
        const V32 k = ln + k0;
        const Mask act = k < nd;
        const V32 jl = k - Q, jh = jl + 1u;                         /* a wrapped index is out of range */
        const V32 w0 = W::load32(row32, jl, act & (jl < nwr), 0u), w1 = W::load32(row32, jh, act & (jh < nwr), 0u);
        const V32 v = W::funnel_shr(w1, w0, m8);
        const V32 i0 = k * 4u - s;                                  /* wraps for the bytes in front of the line: not ours */
        V32 out = W::splat(0u);
        Mask full = act;
        for (uint32_t t = 0; t < 4u; t++) {
            const V32 i = i0 + t;
            const V32 by = W::select((i - L.g) < rl, (v >> (8u * t)) & 0xffu, cbc_sam_field_byte<W>(L, name, tab, i));
            out = out | (by << (8u * t));
            full = full & (i < L.n);
        }
        W::store32_bytes(base, k * 4u, out, full);
        const Mask part = act & !full;                              /* the first and the last dword, shared with the neighbours */
        if (W::ballot(part) != 0ull)
            for (uint32_t t = 0; t < 4u; t++)
                W::store8(base, k * 4u + t, (out >> (8u * t)) & 0xffu, part & ((i0 + t) < L.n));
    }
}

/* ---- the SAM line and the SAM member of the reads-text skeleton (cbc_region_body.h) ------------------------------------- */
template <class W>
CBC_FN typename W::V32 cbc_line_len(cbc_line<CBC_LINE_SAM>, const cbc_sam_blk &S, const cbc_text_grp<W> &G)
{
    return cbc_sam_line_len<W>(S, G.rlv, G.lp, G.fl);
}

/* the constant table is the same for every line: the compiler makes it once, in front of the loops */
template <class W>
CBC_FN void cbc_line_emit(cbc_line<CBC_LINE_SAM>, uint8_t *text, uint64_t o, const cbc_sam_blk &S, uint32_t r0, uint32_t j, const cbc_text_grp<W> &G)
{
    const uint32_t len = W::readlane(G.tl, j), at = W::readlane(G.incl, j) - len;
    cbc_sam_emit<W>(text, o + at, S.B.rows + (uint64_t)(r0 + j) * S.B.stride, W::readlane(G.rlv, j), S.ws + W::readlane(G.lp, j),
                    W::readlane(G.fl, j), S.name, S.nl, len, cbc_sam_const_tab<W>());
}

template <int LINE>
CBC_FN cbc_sam_blk cbc_text_block(const cbc_sam_args &A, uint32_t blk) { return cbc_sam_block(A, blk); }

template <class W>
CBC_FN typename W::Mask cbc_text_keep(const cbc_sam_args &A, const cbc_sam_blk &S, uint32_t r0, cbc_text_grp<W> &G)
{
    return cbc_sam_keep<W>(A, S, r0, G.rlv, G.lp, G.fl);
}

template <class W>
CBC_FN void cbc_sam_count(const cbc_sam_args &A, uint32_t blk) { cbc_text_count<W, CBC_LINE_SAM>(A, A.R, blk); }
template <class W>
CBC_FN void cbc_sam_write(const cbc_sam_args &A, uint32_t blk, uint32_t wave, uint32_t n_waves)
{
    cbc_text_write<W, CBC_LINE_SAM>(A, A.R, blk, wave, n_waves);
}

#endif /* CBC_SAM_BODY_H */
