/*
 * cbc_consensus_body.h -- the sequence the reads spell, as one FASTA record, on the device, behind the passes of the per-position
 * allele counts (cbc_gpu_decode_consensus, include/cbc_gpu.h).
 *
 * The edits decode, the zeroing, cbc_depth_mark, cbc_pileup_events<W, false>, cbc_depth_tile and the scan of its sums are the
 * pileup's own (cbc_pileup_body.h), unchanged: they leave the span depth's difference array and seven counter planes per
 * position.  Behind them:
 *
 *   count    one wavefront per tile of CBC_DEPTH_TILE positions, one lane per position, the depth carry as in cbc_pileup_line:
 *            the call rule (cbc_consensus_call), the tile's emitted bytes into counts[t] for the size scan (64-bit offsets),
 *            and the call's seven counters.
 *   write    the same tile again; the rule is derived again, not stored.  Per round of 64 positions the emit mask's exclusive
 *            scan gives a lane its rank k in the record; its byte goes to header + k + k / line_width, and the lane with
 *            (k + 1) % line_width == 0, or with the record's last byte, writes the '\n' behind it.  The 64-bit part of the address
 *            is uniform -- the base pointer advances per round -- and W::store8 takes a lane offset below 128.  The wavefront of
 *            tile 0 writes the header.  A round that would pass the tile's offset + count (the counters moved under the count
 *            pass) ends the tile.
 *
 * The rule, in exact integers.  c[0..3] = aligned bases of class A, C, G, T; c[4] = of any other class; d = deleted bases; ins =
 * insertion events; depth = c[0] + ... + c[4] + d -- the numbers of the pileup's line.  reaches(x): x * 10^6 >= ppm * depth, both
 * products as (mulhi, low word) pairs (x, depth < 2^32 and ppm <= 10^6 < 2^20 keep them below 2^52).
 *   1  depth < min_depth:  'N'; FILL_REF: the reference byte in lower case (byte | 0x20 when byte & 0xDF is a letter).
 *   2  the highest of c[0..3] and d; among ties the reference's class if it is one of them, else the first of A, C, G, T, DEL.
 *      reaches(it): a base writes its letter, DEL writes nothing (SHOW_DEL: '*').
 *   3  IUPAC only: over the t = c[i] > 0, S(t) = the bases with c[j] >= t; the largest t with reaches(sum of S(t)) writes the
 *      code of S(t); none: 'N'.
 *   4  otherwise 'N'.
 * Insertions are not applied.  ins_skipped counts the positions with depth >= min_depth and reaches(ins); a trailing soft clip is
 * stored as insertions and shows as one such event at the read's last aligned base.
 * Range tests are written without base + length sums.  Written against the wave policy (W = WaveGPU in cbc_gpu_post.hip, the
 * lock-step emulation in tests/consensus_emu).
 */
#ifndef CBC_CONSENSUS_BODY_H
#define CBC_CONSENSUS_BODY_H

#include "cbc_pileup_body.h"

/* the call's counters, in the order of cbc_consensus_counts behind `emitted` */
#define CBC_CONS_REF   0u
#define CBC_CONS_ALT   1u
#define CBC_CONS_DEL   2u
#define CBC_CONS_AMB   3u
#define CBC_CONS_LOW   4u
#define CBC_CONS_NONE  5u
#define CBC_CONS_INS   6u
#define CBC_CONS_CTRS  7u

struct cbc_consensus_args {
    cbc_pileup_args P;            /* the pileup's arguments: P.D.R.counts / offsets / text: the tiles' emitted bytes, their scan
                                   * (n_tiles + 1), the record; P.min_alt is not read                                             */
    uint32_t *cctr;               /* CBC_CONS_CTRS words, zeroed before                                                          */
    uint32_t min_depth, ppm, line_width, flags, with_range, reserved;
};

/* the header's bytes: '>', the name, with_range: ':' BEG '-' END, '\n' */
CBC_FN uint32_t cbc_consensus_hdr_len(const cbc_consensus_args &A)
{
    const uint32_t range = A.with_range ? 2u + cbc_sam_ndig((uint32_t)A.P.D.R.beg, 1000000000u) + cbc_sam_ndig((uint32_t)A.P.D.R.end, 1000000000u) : 0u;
    return A.P.D.name_len + 2u + range;
}

CBC_FN bool cbc_consensus_ok(const cbc_consensus_args &A, uint32_t t)
{
    return cbc_pileup_text_ok(A.P, t) && A.min_depth >= 1u && A.ppm >= 1u && A.ppm <= 1000000u && A.line_width >= 1u &&
           A.line_width <= 65535u;
}

/* positions [i0, i0 + 64) of the window, `run` = the depth in front of them (advanced): the byte of every position, the lanes
 * that emit one (returned), and in cls the position's counter (CBC_CONS_REF ... CBC_CONS_NONE; lanes outside the window:
 * CBC_CONS_CTRS) with bit 8 set where an insertion reaches the fraction */
template <class W>
CBC_FN typename W::Mask cbc_consensus_call(const cbc_consensus_args &A, uint32_t i0, uint32_t &run, typename W::V32 &by,
                                           typename W::V32 &cls)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    const cbc_pileup_args &P = A.P;
    const V32 idx = W::lane() + i0;
    const uint64_t nw = P.D.R.end - P.D.R.beg;
    const Mask m = idx <= (nw > 0xffffffffull ? 0xffffffffu : (uint32_t)nw);
    const V32 incl = W::scan_incl_add(W::load32(P.D.diff, idx, W::all(), 0u));   /* whole tiles behind diff */
    const V32 depth = incl + run;
    run += W::readlane(incl, 63u);
    const V32 zero = W::splat(0u);
    V32 c[CBC_PILEUP_PLANES];
    for (uint32_t k = 0; k < CBC_PILEUP_PLANES; k++) c[k] = W::load32(P.tab + (uint64_t)k * P.plane, idx, m, 0u);
    const uint64_t at = P.ref_c0 + (P.D.R.beg - 1u);                 /* the reference byte of index 0 */
    const uint64_t avail = at <= P.ref_bytes ? P.ref_bytes - at : 0u;
    const Mask rok = m & (idx < (avail > 0xffffffffull ? 0xffffffffu : (uint32_t)avail));
    const V32 rb = W::select(rok, W::load8(P.ref + (at <= P.ref_bytes ? at : 0u), idx, rok), W::splat((uint32_t)'N'));
    const V32 cr = cbc_pileup_class<W>(rb);
    const V32 d = c[CBC_PILEUP_DEL], ins = c[CBC_PILEUP_INS];
    const V32 same = depth - d - (c[0] + c[1] + c[2] + c[3] + c[4]); /* the bases of the reference's class */
    for (uint32_t s = 0; s < 4u; s++) c[s] = W::select(cr == s, same, c[s]);
    /* reaches(x): (x * 10^6) >= (ppm * depth) */
    const V32 mil = W::splat(1000000u), ppm = W::splat(A.ppm);
    const V32 dh = W::mulhi(depth, ppm), dl = depth * A.ppm;
#define CBC_CONS_REACHES(x) ((W::mulhi(x, mil) > dh) | ((W::mulhi(x, mil) == dh) & (((x) * 1000000u) >= dl)))
    /* 1: low depth */
    const Mask low = depth < A.min_depth;
    const V32 up = rb & 0xdfu;
    const V32 lower = W::select((up >= 0x41u) & (up <= 0x5au), rb | 0x20u, rb);
    by = (A.flags & CBC_CONS_FILL_REF) ? lower : W::splat((uint32_t)'N');
    cls = W::splat(CBC_CONS_LOW);
    /* 2: the single call; w = 0..3 a base, 4 = DEL.  Descending, so that the first of the order stays among ties */
    V32 top = d, w = W::splat(4u);
    for (int s = 3; s >= 0; s--) { const Mask ge = c[s] >= top; top = W::select(ge, c[s], top); w = W::select(ge, W::splat((uint32_t)s), w); }
    for (uint32_t s = 0; s < 4u; s++) w = W::select((cr == s) & (c[s] == top), W::splat(s), w);
    const Mask called = (!low) & CBC_CONS_REACHES(top);
    const Mask cdel = called & (w == 4u), cbase = called & (w != 4u);
    const V32 letter = W::select(w == 0u, W::splat((uint32_t)'A'), W::select(w == 1u, W::splat((uint32_t)'C'),
                       W::select(w == 2u, W::splat((uint32_t)'G'), W::splat((uint32_t)'T'))));
    by = W::select(cbase, letter, W::select(cdel, W::splat((uint32_t)'*'), by));
    cls = W::select(cbase, W::select(w == cr, W::splat(CBC_CONS_REF), W::splat(CBC_CONS_ALT)), W::select(cdel, W::splat(CBC_CONS_DEL), cls));
    /* 3, 4: no call */
    const Mask open = (!low) & (!called);
    by = W::select(open, W::splat((uint32_t)'N'), by);
    cls = W::select(open, W::splat(CBC_CONS_NONE), cls);
    if ((A.flags & CBC_CONS_IUPAC) && W::ballot(m & open) != 0ull) {
        V32 bt = zero, bs = zero;                                     /* the largest reaching t and its set, bit s = base s */
        for (uint32_t i = 0; i < 4u; i++) {
            V32 sum = zero, set = zero;
            for (uint32_t j = 0; j < 4u; j++) {
                const Mask in = c[j] >= c[i];
                sum = sum + W::select(in, c[j], zero);
                set = set | W::select(in, W::splat(1u << j), zero);
            }
            const Mask r = (c[i] > bt) & CBC_CONS_REACHES(sum);       /* c[i] > bt >= 0: c[i] > 0 */
            bt = W::select(r, c[i], bt); bs = W::select(r, set, bs);
        }
        /* the code of the set: "NACMGRSVTWYHKDBN"[set], four letters a word */
        const V32 q = bs >> 2u;
        const V32 word = W::select(q == 0u, W::splat(0x4d43414eu), W::select(q == 1u, W::splat(0x56535247u),
                         W::select(q == 2u, W::splat(0x48595754u), W::splat(0x4e42444bu))));
        const Mask amb = open & (bt != 0u);
        by = W::select(amb, (word >> ((bs & 3u) * 8u)) & 0xffu, by);
        cls = W::select(amb, W::splat(CBC_CONS_AMB), cls);
    }
    const Mask skipped = m & (!low) & CBC_CONS_REACHES(ins);
#undef CBC_CONS_REACHES
    cls = W::select(m, cls | W::select(skipped, W::splat(256u), zero), W::splat(CBC_CONS_CTRS));
    return m & !(cdel & ((A.flags & CBC_CONS_SHOW_DEL) == 0u));
}

template <class W>
CBC_FN void cbc_consensus_count(const cbc_consensus_args &A, uint32_t t)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    if (t >= A.P.D.n_tiles) return;
    uint32_t emitted = 0, n[CBC_CONS_CTRS];
    for (uint32_t k = 0; k < CBC_CONS_CTRS; k++) n[k] = 0u;
    if (cbc_consensus_ok(A, t)) {
        uint32_t run = (uint32_t)A.P.D.sum_off[t];                   /* depth in front of the tile, mod 2^32 */
        for (uint32_t r = 0; r < CBC_DEPTH_TILE / 64u; r++) {
            V32 by, cls;
            const Mask em = cbc_consensus_call<W>(A, t * CBC_DEPTH_TILE + r * 64u, run, by, cls);
            emitted += W::popc64(W::ballot(em));
            const V32 kind = cls & 0xffu;
            for (uint32_t k = 0; k < CBC_CONS_INS; k++) n[k] += W::popc64(W::ballot(kind == k));
            n[CBC_CONS_INS] += W::popc64(W::ballot((cls & 256u) != 0u));
        }
    }
    cbc_store_result<W>(A.P.D.R.counts + t, emitted, 0u);
    V32 v = W::splat(0u);
    for (uint32_t k = 0; k < CBC_CONS_CTRS; k++) W::set_lane(v, k, n[k]);
    W::list_add(A.cctr, W::lane(), v, (W::lane() < CBC_CONS_CTRS) & (v != 0u));
}

/* the header, by one wavefront: '>', the name 64 bytes a turn, the range's bytes from one register, '\n' */
template <class W>
CBC_FN void cbc_consensus_header(const cbc_consensus_args &A, uint8_t *text)
{
    typedef typename W::V32 V32;
    const uint32_t nl = A.P.D.name_len;
    const V32 ln = W::lane();
    W::store8(text, ln, W::splat((uint32_t)'>'), ln == 0u);
    for (uint32_t b = 0; b < nl; b += 64u) {
        const typename W::Mask in = (ln + b) < nl;
        W::store8(text + 1u, ln + b, W::load8(A.P.D.name, ln + b, in), in);
    }
    V32 tail = W::splat(0u);
    uint32_t n = 0;
    if (A.with_range) {
        const uint32_t v[2] = { (uint32_t)A.P.D.R.beg, (uint32_t)A.P.D.R.end };
        for (uint32_t s = 0; s < 2u; s++) {
            W::set_lane(tail, n++, s ? (uint32_t)'-' : (uint32_t)':');
            const uint32_t nd = cbc_sam_ndig(v[s], 1000000000u);
            uint32_t x = v[s];
            for (uint32_t j = nd; j-- > 0u; x /= 10u) W::set_lane(tail, n + j, 48u + x % 10u);
            n += nd;
        }
    }
    W::set_lane(tail, n++, 10u);
    W::store8(text + 1u + nl, ln, tail, ln < n);
}

template <class W>
CBC_FN void cbc_consensus_write(const cbc_consensus_args &A, uint32_t t)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    if (!cbc_consensus_ok(A, t)) return;
    const cbc_region_args &R = A.P.D.R;
    const uint32_t hdr = cbc_consensus_hdr_len(A), lw = A.line_width;
    if (hdr > R.text_cap) return;
    if (t == 0u) cbc_consensus_header<W>(A, R.text);
    const uint32_t cnt = R.counts[t].nbytes;
    const uint64_t o0 = R.offsets[t], total = R.offsets[A.P.D.n_tiles], room = R.text_cap - hdr;
    /* the tile's ranks [o0, o0 + cnt) lie in the record, and the record's hdr + total + ceil(total / lw) bytes in the text */
    if (cnt == 0u || o0 > total || cnt > total - o0 || total > room || (total + (lw - 1u)) / lw > room - total) return;
    const uint32_t magic = lw > 1u ? 0xffffffffu / lw + 1u : 0u;     /* ceil(2^32 / lw): floor(x / lw) = mulhi(x, magic) for x < 128 */
    uint64_t k0 = o0;
    uint32_t run = (uint32_t)A.P.D.sum_off[t];
    for (uint32_t r = 0; r < CBC_DEPTH_TILE / 64u; r++) {
        V32 by, cls;
        const Mask em = cbc_consensus_call<W>(A, t * CBC_DEPTH_TILE + r * 64u, run, by, cls);
        const uint64_t bits = W::ballot(em);
        if (bits == 0ull) continue;
        const uint32_t n = W::popc64(bits);
        if (n > (o0 + cnt) - k0) return;                             /* the counters moved under the count pass */
        const uint64_t q0 = k0 / lw;
        const uint32_t r0 = (uint32_t)(k0 - q0 * lw);                /* rank k0 + j sits at hdr + k0 + q0 + j + floor((r0 + j) / lw) */
        uint8_t *p = R.text + hdr + k0 + q0;
        const V32 j = W::prefix_popc(bits), x = j + r0;
        V32 wr, wr1;                                                 /* floor(x / lw), floor((x + 1) / lw): x + 1 <= lw + 63 */
        if (lw >= 64u) { wr = W::select(x >= lw, W::splat(1u), W::splat(0u)); wr1 = W::select(x + 1u >= lw, W::splat(1u), W::splat(0u)); }
        else if (lw == 1u) { wr = x; wr1 = x + 1u; }
        else { wr = W::mulhi(x, W::splat(magic)); wr1 = W::mulhi(x + 1u, W::splat(magic)); }
        const V32 off = j + wr;
        W::store8(p, off, by, em);
        const uint64_t left = total - k0;                            /* >= n: the record's last byte is lane rank left - 1 */
        const Mask last = j == (left <= 64u ? (uint32_t)left - 1u : 0xffffffffu);
        W::store8(p, off + 1u, W::splat(10u), em & ((wr1 != wr) | last));
        k0 += n;
    }
}

#endif /* CBC_CONSENSUS_BODY_H */
