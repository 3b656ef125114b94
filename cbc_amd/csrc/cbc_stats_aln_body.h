/*
 * cbc_stats_aln_body.h -- the alignment tables of the read statistics on the device, after the edit-reporting decode of the
 * selected blocks (cbc_gpu_decode_stats_aln, include/cbc_gpu.h).
 *
 * The decoder (cbc_decode_body.h, EDITS = true) has left, beside the records and rows, the alignment of every read with indels
 * (cbc_dec_edits); the element order, the S rule, the mismatch rule and what makes a record valid are those of
 * cbc_gpu_decode_sam_cigar (cbc_cigar_body.h: cbc_cigar_open and cbc_cigar_step are called, not restated).  A counted read is one
 * cbc_stats_accum counts: the same keep rule and exclusion, taken the same way.  With cyc(q) = q + 1 for a forward read and rl - q
 * for FLAG & 16, one pass fills, per workgroup in LDS and then in the global table:
 *   len      valid counted reads by length                                  a read adds 1 to one word
 *   mm       mismatches by cycle: cyc(q) of the aligned read index          a read has one base per cycle: at most 1 per word
 *   unal     inserted read indices (I and S) by cycle                       the same
 *   ins_cyc  I runs by the cycle of their first-sequenced base              runs are disjoint, so are their first bases: at most 1
 *   del_cyc  D runs by the cycle of the base sequenced just before: k forward, rl - k reverse, k = the read index of the aligned
 *            base behind the run, rl for the run at T; one run per matched coordinate, so k is distinct per run: at most 1
 *   nm       reads by NM = mismatches + I bases + D bases <= 256 + 255 + 255  a read adds 1 to one word
 *   ins_len, del_len  runs by length 1 .. 255                               a read adds up to 255 to a word (see the flush)
 * and one counter: the counted reads that are not valid, which are in no table.
 *
 * Work: the split of cbc_stats_accum -- units of 64 records strided over a bounded grid, CBC_STATS_WAVES wavefronts sharing one
 * LDS table of CBC_SALN_LDS words.  Per unit one lane per record takes the keep rule, the exclusion, the side words and the part
 * of the validity test that needs no list; then read by read, the whole wavefront on one read:
 *   without indels (nearly all)  lane l takes the row's dword l and the four reference bytes at POS - 1 + 4 l as one unaligned
 *            dword; the lane that holds the read's last 1 .. 3 bytes takes the dword that ENDS at the read's last byte and shifts,
 *            so nothing is read outside [POS - 1, POS - 1 + rl) -- the bytes the validity test has placed inside the upload (a
 *            read shorter than 4: byte loads).  XOR, mask by the length; a read without a mismatch ends behind one ballot, a
 *            mismatching byte costs one lds_add.
 *   with indels  cbc_cigar_open, then cbc_cigar_step turn by turn: mismatches and run starts are its masks, the I run that ends
 *            in front of lane q has its length in clen, the D run in front of aligned q in dq; the inserted indices go to unal
 *            one lane per list entry.
 * NM lands in the read's lane; len and nm are one lds_add per unit.  Range tests are written without base + length sums.
 * Zero, accumulate and flush are three bodies, as in cbc_stats_body.h.  Written against the wave policy (W = WaveGPU in
 * cbc_gpu.hip, the lock-step emulation in tests/alnstats_emu).
 */
#ifndef CBC_STATS_ALN_BODY_H
#define CBC_STATS_ALN_BODY_H

#include <stdint.h>
#include <string.h>
#include "../../include/cbc_gpu.h"
#include "cbc_stats_body.h"
#include "cbc_cigar_body.h"

/* the workgroup's table, in words; the global table begins with the same words in the same order */
#define CBC_SALN_L_LEN   0u
#define CBC_SALN_L_MM    (CBC_SALN_L_LEN + CBC_STATS_ALN_CYC)
#define CBC_SALN_L_UNAL  (CBC_SALN_L_MM + CBC_STATS_ALN_CYC)
#define CBC_SALN_L_ICYC  (CBC_SALN_L_UNAL + CBC_STATS_ALN_CYC)
#define CBC_SALN_L_DCYC  (CBC_SALN_L_ICYC + CBC_STATS_ALN_CYC)
#define CBC_SALN_L_NM    (CBC_SALN_L_DCYC + CBC_STATS_ALN_CYC)
#define CBC_SALN_L_ILEN  (CBC_SALN_L_NM + CBC_STATS_ALN_NM)
#define CBC_SALN_L_DLEN  (CBC_SALN_L_ILEN + CBC_STATS_ALN_LEN)
#define CBC_SALN_L_USED  (CBC_SALN_L_DLEN + CBC_STATS_ALN_LEN)
#define CBC_SALN_LDS     ((CBC_SALN_L_USED + 63u) & ~63u)
/* the global table: words [0, L_ILEN) as above; the two run-length tables as two planes of 2 x 256 words -- the sums of the low
 * and of the high 16-bit halves of the workgroups' counts -- then [0] = counted reads that are not valid, [1] spare */
#define CBC_SALN_T_LO    CBC_SALN_L_ILEN
#define CBC_SALN_T_HI    (CBC_SALN_T_LO + 2u * CBC_STATS_ALN_LEN)
#define CBC_SALN_T_CTR   (CBC_SALN_T_HI + 2u * CBC_STATS_ALN_LEN)
#define CBC_SALN_WORDS   (CBC_SALN_T_CTR + 2u)
/* A workgroup's count of a run length is below 2^32: a read adds at most 255 to it (nDel, nIns <= 255), a unit has 64 reads and
 * a workgroup of n_waves wavefronts takes at most n_waves * ceil(units / (grid * n_waves)) <= units / grid + n_waves units;
 * the host keeps units <= CBC_SALN_MAX_UNITS with the grid at CBC_STATS_GRID from 4 * CBC_STATS_GRID units on:
 * (2^18 + 4) * 64 * 255 < 2^32.  The low plane then takes less than 2^16 per workgroup, 2^27 in all; the high plane takes
 * count >> 16, in all at most 255 * 2^32 >> 16 < 2^24.  The host puts them together in 64 bits (cbc_stats_aln_finish). */
#define CBC_SALN_MAX_UNITS (1ull << 29)

struct cbc_stats_aln_args {
    cbc_stats_args S;             /* records, rows, blocks, window starts, decode results, intervals, exclude, gmax, grid as for
                                   * the statistics pass (S.tab is not read)                                                      */
    const uint32_t *side;         /* the EDITS decoder's side array and arena (cbc_dec_edits)                                    */
    const uint16_t *arena;
    const uint8_t  *ref;          /* the device reference                                                                        */
    uint32_t *tab;                /* CBC_SALN_WORDS, zeroed before                                                               */
    uint64_t arena_entries, ref_bytes;
    uint32_t per_read, reserved;
};

/* the block as cbc_cigar_open wants it: the set-up of cbc_text_block<CBC_LINE_SAM_CIGAR> without the contig name */
CBC_FN cbc_cigar_blk cbc_stats_aln_block(const cbc_stats_aln_args &A, const cbc_region_blk &B, uint32_t blk)
{
    cbc_cigar_blk X = {};
    X.B = B;
    const cbc_dec_block_desc *bd = A.S.R.blocks + blk;
    const uint64_t rec_base = X.B.ok ? bd->rec_base : 0u, ref_off = bd->ref_off;
    const uint64_t cap64 = (uint64_t)X.B.n * A.per_read, base64 = rec_base * A.per_read;
    X.B.ok = X.B.ok && A.per_read >= 1u && A.per_read <= CBC_EDITS_MAX && base64 <= A.arena_entries && cap64 <= A.arena_entries - base64 &&
             ref_off <= A.ref_bytes;
    const uint64_t ref_avail = X.B.ok ? A.ref_bytes - ref_off : 0u;
    X.cap = X.B.ok ? (uint32_t)cap64 : 0u;
    X.ref_lim = ref_avail > 0xffffffffull ? 0xffffffffu : (uint32_t)ref_avail;
    X.arena = A.arena + (X.B.ok ? base64 : 0u);
    X.side = A.side + 2u * rec_base;
    X.refb = A.ref + (X.B.ok ? ref_off : 0u);
    return X;
}

template <class W>
CBC_FN void cbc_stats_aln_zero(uint32_t *lds, uint32_t wave, uint32_t n_waves)
{
    for (uint32_t r = wave; r < CBC_SALN_LDS / 64u; r += n_waves) W::lds_zero(lds, W::lane() + r * 64u, W::all());
}

/* the workgroup's table into the global one: the 32-bit tables word for word, a run-length count as its two halves */
template <class W>
CBC_FN void cbc_stats_aln_flush(const cbc_stats_aln_args &A, const uint32_t *lds, uint32_t wave, uint32_t n_waves)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    for (uint32_t r = wave; r < CBC_SALN_LDS / 64u; r += n_waves) {
        const V32 i = W::lane() + r * 64u;
        const V32 v = W::lds_read(lds, i, W::all());
        const Mask nz = (v != 0u) & (i < CBC_SALN_L_USED), wide = i >= CBC_SALN_L_ILEN;
        const V32 lo = W::select(wide, v & 0xffffu, v), hi = v >> 16;
        W::list_add(A.tab, i, lo, nz & (lo != 0u));
        W::list_add(A.tab, i + (CBC_SALN_T_HI - CBC_SALN_T_LO), hi, nz & wide & (hi != 0u));
    }
}

/* wavefront `wave` of the n_waves of workgroup wg (of A.S.grid); TG: keep by the interval table */
template <class W, bool TG>
CBC_FN void cbc_stats_aln_accum(const cbc_stats_aln_args &A, uint32_t wg, uint32_t wave, uint32_t n_waves, uint32_t *lds)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    const cbc_stats_args &S = A.S;
    if (S.grid == 0u || wg >= S.grid || S.gmax == 0u || wave >= n_waves) return;
    const V32 ln = W::lane(), zero = W::splat(0u), one = W::splat(1u);
    const uint64_t units = (uint64_t)S.R.n_blocks * S.gmax, step = (uint64_t)S.grid * n_waves;
    uint32_t n_inv = 0;
    for (uint64_t u = (uint64_t)wg * n_waves + wave; u < units; u += step) {
        const uint32_t blk = (uint32_t)(u / S.gmax), r0 = (uint32_t)(u % S.gmax) * 64u;
        cbc_region_blk B = cbc_region_block(S.R, blk);
        if (!B.ok || r0 >= B.n) continue;
        V32 rlv, fl, lp;
        Mask k;
        if (TG) {                                                    /* the unit's head is that of cbc_stats_accum */
            const cbc_targets_blk T = cbc_targets_block(B, S.R.window_start[blk], S.iv, S.block_iv, S.n_iv, blk);
            if (!T.B.ok) continue;
            V32 span, j;
            k = cbc_targets_keep<W>(T, r0, rlv, lp, fl, span, j);
        } else {
            V32 w1, off, span;
            const Mask m = (ln + r0) < B.n;
            W::load_rec(B.recs4, ln + r0, m, lp, w1, off, span);
            rlv = w1 >> 16;
            fl = w1 & 0xffffu;
            k = m & (rlv <= B.stride);
        }
        const Mask c = k & ((fl & S.exclude) == 0u);
        uint64_t bits = W::ballot(c);
        if (!bits) continue;
        const cbc_cigar_blk X = cbc_stats_aln_block(A, B, blk);
        if (!X.B.ok) continue;
        /* the side words, and the tests of cbc_cigar_open that need no list */
        const V32 e0v = W::load32(X.side, (ln + r0) * 2u, c, 0u), cntv = W::load32(X.side, (ln + r0) * 2u + 1u, c, 0u);
        const V32 ndv = cntv & 0xffffu, niv = cntv >> 16;
        Mask vb = c & (rlv != 0u) & (ndv <= 255u) & (niv <= 255u) & (e0v <= X.cap) & (niv <= rlv) & (lp >= 1u);
        vb = vb & ((ndv + niv) <= (X.cap - e0v)) & ((lp - 1u) <= X.ref_lim) & (((rlv - niv) + ndv) <= (X.ref_lim - (lp - 1u)));
        uint64_t vbits = W::ballot(vb);
        const uint64_t indel = W::ballot(c & (cntv != 0u));
        V32 nmv = zero;
        bits = vbits;
        while (bits) {
            const uint32_t j = W::ctz64(bits);
            bits &= bits - 1u;
            const uint32_t rl = W::readlane(rlv, j), lpj = W::readlane(lp, j);
            const bool rev = (W::readlane(fl, j) & 16u) != 0u;
            const uint8_t *row = B.rows + (uint64_t)(r0 + j) * B.stride;
            uint32_t nm = 0;
            if (!((indel >> j) & 1u)) {
                /* vb: 1 <= rl, and reference bytes [lpj - 1, lpj - 1 + rl) lie inside the block's part of the upload */
                const uint8_t *rp = X.refb + (lpj - 1u);
                const V32 q0 = ln * 4u, rem = W::splat(rl) - q0;
                const Mask mv = q0 < rl, tail = mv & (rem < 4u);
                const V32 w = W::load32((const uint32_t *)row, ln, mv, 0u);
                V32 rw;
                if (rl >= 4u) {
                    rw = W::load32_bytes(rp, W::select(tail, W::splat(rl - 4u), q0), mv);
                    rw = rw >> W::select(tail, (4u - rem) * 8u, zero);           /* the tail's bytes are the dword's last rem */
                } else {
                    rw = zero;
                    for (uint32_t b = 0; b < rl; b++) rw = rw | (W::load8(rp, W::splat(b), ln == 0u) << (8u * b));
                }
                const V32 bm = W::select(tail, (one << (rem * 8u)) - 1u, W::splat(0xffffffffu));
                const V32 x = W::select(mv, (w ^ rw) & bm, zero);
                if (W::ballot(x != 0u) != 0ull)
                    for (uint32_t b = 0; b < 4u; b++) {
                        const Mask mb = ((x >> (8u * b)) & 0xffu) != 0u;
                        const V32 q = q0 + b;
                        W::lds_add(lds, (rev ? W::splat(rl) - q : q + 1u) + CBC_SALN_L_MM, one, mb);
                        nm += W::popc64(W::ballot(mb));
                    }
            } else {
                cbc_cigar_read<W> R;
                if (!cbc_cigar_open<W>(X, row, rl, lpj, W::readlane(e0v, j), W::readlane(cntv, j), R)) {
                    vbits &= ~(1ull << j);
                    continue;
                }
                cbc_cigar_carry C = { 0u, 0u };
                nm = R.nd;
                for (uint32_t b = 0; b < rl; b += 64u) {
                    cbc_cigar_turn<W> U;
                    cbc_cigar_step<W>(X, R, b, C, U);
                    if (!U.any) continue;
                    const V32 q = ln + b;                                /* the masks below hold only for q < rl */
                    const V32 back = W::splat(rl) - q;                   /* cyc(q) of a reverse read; q of the base sequenced before it */
                    W::lds_add(lds, (rev ? back : q + 1u) + CBC_SALN_L_MM, one, U.mis);
                    /* the run that ends at q - 1 is [q - clen, q - 1]: first sequenced q - clen forward, q - 1 reverse */
                    const Mask irun = U.bnd & (U.clen != 0u) & (U.cop == (uint32_t)'I');
                    W::lds_add(lds, (rev ? back + 1u : (q - U.clen) + 1u) + CBC_SALN_L_ICYC, one, irun);
                    W::lds_add(lds, U.clen + CBC_SALN_L_ILEN, one, irun);             /* clen <= nIns <= 255 */
                    /* the deleted run in front of aligned q: k = q */
                    const Mask drun = U.dq != 0u;
                    W::lds_add(lds, (rev ? back : q) + CBC_SALN_L_DCYC, one, drun);
                    W::lds_add(lds, U.dq + CBC_SALN_L_DLEN, one, drun);               /* dq <= nDel <= 255 */
                    nm += W::popc64(W::ballot(U.mis)) + W::reduce_add(W::select(irun, U.clen, zero));
                }
                if (R.dT) {                                              /* the run at T: k = rl */
                    W::lds_add(lds, W::splat((rev ? 0u : rl) + CBC_SALN_L_DCYC), one, ln == 0u);
                    W::lds_add(lds, W::splat(R.dT + CBC_SALN_L_DLEN), one, ln == 0u);
                }
                for (uint32_t i0 = 0; i0 < R.ni; i0 += 64u) {            /* cbc_cigar_open: every oi < rl */
                    const Mask m = (ln + i0) < R.ni;
                    const V32 oi = i0 ? W::load16(R.ar, ln + (R.nd + i0), m) : R.oiv;
                    W::lds_add(lds, (rev ? W::splat(rl) - oi : oi + 1u) + CBC_SALN_L_UNAL, one, m);
                }
            }
            W::set_lane(nmv, j, nm);
        }
        /* the per-read tables, one lane per read */
        const Mask v = W::lane_bit(vbits);
        W::lds_add(lds, rlv + CBC_SALN_L_LEN, one, v);                   /* rlv <= stride <= 256 */
        W::lds_add(lds, nmv + CBC_SALN_L_NM, one, v & (nmv < CBC_STATS_ALN_NM));
        n_inv += W::popc64(W::ballot(c)) - W::popc64(vbits);
    }
    W::list_add(A.tab, W::splat(CBC_SALN_T_CTR), W::splat(n_inv), (ln == 0u) & (n_inv != 0u));
}

/* host side: the device's table `w` (CBC_SALN_WORDS) into the caller's struct */
static inline void cbc_stats_aln_finish(const uint32_t *w, cbc_gpu_stats_aln *st)
{
    memset(st, 0, sizeof *st);
    memcpy(st->len, w + CBC_SALN_L_LEN, sizeof st->len);
    memcpy(st->mm, w + CBC_SALN_L_MM, sizeof st->mm);
    memcpy(st->unal, w + CBC_SALN_L_UNAL, sizeof st->unal);
    memcpy(st->ins_cyc, w + CBC_SALN_L_ICYC, sizeof st->ins_cyc);
    memcpy(st->del_cyc, w + CBC_SALN_L_DCYC, sizeof st->del_cyc);
    memcpy(st->nm, w + CBC_SALN_L_NM, sizeof st->nm);
    for (uint32_t l = 0; l < CBC_STATS_ALN_LEN; l++) {
        st->ins_len[l] = (uint64_t)w[CBC_SALN_T_LO + l] + ((uint64_t)w[CBC_SALN_T_HI + l] << 16);
        st->del_len[l] = (uint64_t)w[CBC_SALN_T_LO + CBC_STATS_ALN_LEN + l] + ((uint64_t)w[CBC_SALN_T_HI + CBC_STATS_ALN_LEN + l] << 16);
    }
    st->invalid = w[CBC_SALN_T_CTR];
    for (uint32_t l = 0; l < CBC_STATS_ALN_CYC; l++) st->reads += st->len[l];
}

#endif /* CBC_STATS_ALN_BODY_H */
