/*
 * cbc_stats_body.h -- read statistics on the device, after the decode of the selected blocks has left the records and the rows
 * in the context's arenas (cbc_gpu_decode_stats, include/cbc_gpu.h).
 *
 * One streaming pass over the records and rows fills four count tables, every counter 32 bits (no counter passes the reads of
 * the call, which the host keeps below 2^32):
 *   FLAG    65536 bins, one per 16-bit FLAG value
 *   length  bins 0 .. 256
 *   GC      bins 0 .. 100: floor(100 * (bytes 'G' and 'C') / length) of the reads of length >= 1
 *   cycle   4 x 256: how often 'A', 'C', 'G', 'T' stand in sequencing cycle c.  A forward read's cycle c is SEQ[c]; a read with
 *           FLAG & 16 has cycle c = the complement of SEQ[len - 1 - c].  The fifth row ("other") is the host's: the reads that
 *           reach cycle c (from the length table) less the four.
 * and one counter: the reads with FLAG & exclude != 0, which are counted there and nowhere else.
 *
 * Work: unit u = (block u / gmax, record group u % gmax) of 64 records, gmax = the groups of the largest block; the
 * grid * n_waves wavefronts of a bounded grid stride over the units.  A unit: one lane per record for FLAG, length and the keep
 * rule (every record, or cbc_targets_keep unchanged); then read by read over the kept ones, the whole wavefront on one row:
 * lane l owns cycles 4 l .. 4 l + 3.  A forward read is one aligned dword per lane.  A reverse read is taken by index from its
 * end: lane l wants bytes [len - 4 l - 4, len - 4 l), two aligned words and a funnel shift (the form of cbc_region_emit; the shift
 * 8 * (len & 3) is wave-uniform), then a byte reversal, and the complement is a swap of the counters the matches go to.  Both
 * kinds go through one branch-free fetch of two words per lane, issued one read ahead of the counting (cbc_stats_fetch).  Bytes
 * at or past the length are masked by the length, never trusted to be zero.  Four SWAR compares leave 0 / 1 per byte; they are
 * summed in four registers of four 8-bit counters (a unit adds at most 64 to each) and go to the workgroup's cycle table in LDS
 * once per unit.  The read's G + C count is four ballots and lands in the read's lane, so the percent is one exact restoring
 * division per unit, lane-parallel.
 *
 * The workgroup's tables live in LDS (CBC_STATS_LDS words): FLAG values below CBC_STATS_FLAGS_LDS (every defined SAM bit), length,
 * GC, cycle, laid out in the order of the global table so that the flush is one index shift.  FLAG values at or above the bound
 * go straight to the global table.  The n_waves wavefronts of a workgroup share the tables: zero, barrier, accumulate, barrier,
 * flush (one list_add per non-zero word) -- three bodies, so that the lock-step emulation can run them phase by phase.
 * Written against the wave policy (W = WaveGPU in cbc_gpu.hip, the lock-step emulation in tests/stats_emu).
 */
#ifndef CBC_STATS_BODY_H
#define CBC_STATS_BODY_H

#include <stdint.h>
#include <string.h>
#include "../../include/cbc_gpu.h"
#include "cbc_region_body.h"
#include "cbc_targets_body.h"

#ifndef CBC_STATS_FLAGS_LDS
#define CBC_STATS_FLAGS_LDS 4096u  /* FLAG bins kept in the workgroup's LDS table (0: all of them in the global table, A/B) */
#endif
#define CBC_STATS_WAVES 4u         /* wavefronts that share one workgroup's tables             */
#define CBC_STATS_GRID  2048u      /* workgroups at most                                       */

/* the global table, in words */
#define CBC_STATS_T_FLAG 0u
#define CBC_STATS_T_LEN  65536u
#define CBC_STATS_T_GC   (CBC_STATS_T_LEN + CBC_STATS_LEN_BINS)
#define CBC_STATS_T_CYC  (CBC_STATS_T_GC + CBC_STATS_GC_BINS)
#define CBC_STATS_T_CTR  (CBC_STATS_T_CYC + 4u * CBC_STATS_CYCLES)     /* [0] = reads excluded, [1] spare */
#define CBC_STATS_WORDS  (CBC_STATS_T_CTR + 2u)
/* the workgroup's table: the FLAG bins it keeps, then length, GC and cycle in the global order; whole rows of 64 words */
#define CBC_STATS_L_LEN  CBC_STATS_FLAGS_LDS
#define CBC_STATS_L_GC   (CBC_STATS_L_LEN + CBC_STATS_LEN_BINS)
#define CBC_STATS_L_CYC  (CBC_STATS_L_GC + CBC_STATS_GC_BINS)
#define CBC_STATS_L_USED (CBC_STATS_L_CYC + 4u * CBC_STATS_CYCLES)
#define CBC_STATS_LDS    ((CBC_STATS_L_USED + 63u) & ~63u)

struct cbc_stats_args {
    cbc_region_args R;            /* records, rows, blocks, window starts and decode results as for the region passes (beg = 1,
                                   * end = UINT64_MAX; counts, offsets and text unused)                                        */
    const uint32_t *iv;           /* target form: n_iv pairs beg, end, and per block its first interval and count             */
    const uint32_t *block_iv;
    uint32_t *tab;                /* CBC_STATS_WORDS, zeroed before                                                            */
    uint32_t n_iv, exclude, gmax, grid;
};

/* 0x01 in every byte of x that is zero, 0 elsewhere (no carry leaves a byte: the sum of two 7-bit values) */
template <class W>
CBC_FN typename W::V32 cbc_stats_zero_bytes(const typename W::V32 &x)
{
    typedef typename W::V32 V32;
    const V32 t = (x & 0x7f7f7f7fu) + 0x7f7f7f7fu;
    return (((t | x) | 0x7f7f7f7fu) ^ 0xffffffffu) >> 7;
}

/* the two aligned words of record r's row that hold lane l's four cycles, asked for in every lane and without a branch: a
 * forward read wants word l (twice); a read with FLAG & 16 wants bytes [s, s + 4), s = len - 4 l - 4, i.e. words s / 4 and
 * s / 4 + 1 -- rl / 4 at most, which is inside the row when rl & 3 != 0 and otherwise the word behind it (the next row, or the
 * spare bytes behind the rows, as in cbc_region_emit; its bytes are shifted out).  The lane with s < 0 and the lanes past the
 * read ask for word 0; what they get is masked by the length. */
template <class W>
struct cbc_stats_row { typename W::V32 w0, w1; uint32_t rl; bool rev; };

template <class W>
CBC_FN cbc_stats_row<W> cbc_stats_fetch(const cbc_region_blk &B, uint32_t r, uint32_t rl, bool rev)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    cbc_stats_row<W> R;
    const V32 ln = W::lane();
    const uint32_t *row32 = (const uint32_t *)(B.rows + (uint64_t)r * B.stride);
    const V32 rem = W::splat(rl) - ln * 4u;
    const Mask in = ((ln * 4u) < rl) & !((rem < 4u) & rev);
    const V32 i0 = rev ? (rem - 4u) >> 2 : ln;
    R.w0 = W::load32(row32, W::select(in, i0, W::splat(0u)), W::all(), 0u);
    R.w1 = W::load32(row32, W::select(in, rev ? i0 + 1u : i0, W::splat(0u)), W::all(), 0u);
    R.rl = rl; R.rev = rev;
    return R;
}

template <class W>
CBC_FN void cbc_stats_zero(uint32_t *lds, uint32_t wave, uint32_t n_waves)
{
    for (uint32_t r = wave; r < CBC_STATS_LDS / 64u; r += n_waves) W::lds_zero(lds, W::lane() + r * 64u, W::all());
}

/* the workgroup's table into the global one: words [0, FLAGS_LDS) are FLAG bins, the rest sits CBC_STATS_T_LEN - CBC_STATS_L_LEN
 * further on */
template <class W>
CBC_FN void cbc_stats_flush(const cbc_stats_args &A, const uint32_t *lds, uint32_t wave, uint32_t n_waves)
{
    typedef typename W::V32 V32;
    for (uint32_t r = wave; r < CBC_STATS_LDS / 64u; r += n_waves) {
        const V32 i = W::lane() + r * 64u;
        const V32 v = W::lds_read(lds, i, W::all());
        const V32 g = W::select(i < CBC_STATS_L_LEN, i, i + (CBC_STATS_T_LEN - CBC_STATS_L_LEN));
        W::list_add(A.tab, g, v, (v != 0u) & (i < CBC_STATS_L_USED));
    }
}

/* wavefront `wave` of the n_waves of workgroup wg (of A.grid); TG: keep by the interval table */
template <class W, bool TG>
CBC_FN void cbc_stats_accum(const cbc_stats_args &A, uint32_t wg, uint32_t wave, uint32_t n_waves, uint32_t *lds)
{
    typedef typename W::V32 V32;
    typedef typename W::Mask Mask;
    if (A.grid == 0u || wg >= A.grid || A.gmax == 0u || wave >= n_waves) return;
    const V32 ln = W::lane();
    const uint64_t units = (uint64_t)A.R.n_blocks * A.gmax, step = (uint64_t)A.grid * n_waves;
    uint32_t n_excl = 0;
    for (uint64_t u = (uint64_t)wg * n_waves + wave; u < units; u += step) {
        const uint32_t blk = (uint32_t)(u / A.gmax), r0 = (uint32_t)(u % A.gmax) * 64u;
        cbc_region_blk B = cbc_region_block(A.R, blk);
        if (!B.ok || r0 >= B.n) continue;
        V32 rlv, fl;
        Mask k;
        if (TG) {
            const cbc_targets_blk T = cbc_targets_block(B, A.R.window_start[blk], A.iv, A.block_iv, A.n_iv, blk);
            if (!T.B.ok) continue;
            V32 lp, span, j;
            k = cbc_targets_keep<W>(T, r0, rlv, lp, fl, span, j);
        } else {
            V32 lp, w1, off, span;
            const Mask m = (ln + r0) < B.n;
            W::load_rec(B.recs4, ln + r0, m, lp, w1, off, span);
            rlv = w1 >> 16;
            fl = w1 & 0xffffu;
            k = m & (rlv <= B.stride);
        }
        const Mask ex = k & ((fl & A.exclude) != 0u);
        const Mask c = k & !ex;
        n_excl += W::popc64(W::ballot(ex));
        V32 gcv = W::splat(0u), acc_a = W::splat(0u), acc_c = W::splat(0u), acc_g = W::splat(0u), acc_t = W::splat(0u);
        /* one read ahead: the two words of the next read are asked for in the turn that counts this one; the last read of the
         * unit fetches itself once more, so that every turn issues the same two loads.  (The compiler still places them at the
         * end of the turn and waits for both pairs: DESIGN.md section 4.18.) */
        uint64_t bits = W::ballot(c);
        if (bits) {
            uint32_t j = W::ctz64(bits);
            bits &= bits - 1u;
            cbc_stats_row<W> cur = cbc_stats_fetch<W>(B, r0 + j, W::readlane(rlv, j), (W::readlane(fl, j) & 16u) != 0u);
            for (;;) {
                const bool more = bits != 0u;
                const uint32_t jn = more ? W::ctz64(bits) : j;
                bits &= bits - 1u;
                const cbc_stats_row<W> nxt = cbc_stats_fetch<W>(B, r0 + jn, W::readlane(rlv, jn), (W::readlane(fl, jn) & 16u) != 0u);
                const uint32_t rl = cur.rl;
                const bool rev = cur.rev;
                const V32 rem = W::splat(rl) - ln * 4u;              /* bytes from this lane's first cycle to the read's end */
                const Mask mv = (ln * 4u) < rl;
                const V32 nv = W::select(mv, W::select(rem < 4u, rem, W::splat(4u)), W::splat(0u));
                /* forward: the word itself.  Reverse: bytes [rem - 4, rem) out of the two words, reversed; the lane that holds
                 * the read's first rem < 4 bytes takes a zero low word, and the bytes in front of the read land past the length
                 * after the reversal and are masked with the rest */
                const V32 lo = W::select((rem < 4u) & rev, W::splat(0u), cur.w0);
                const V32 x = W::funnel_shr(cur.w1, lo, rev ? 8u * (rl & 3u) : 0u);
                V32 v = rev ? W::bswap_v(x) : x;
                v = v & W::select(nv >= 4u, W::splat(0xffffffffu), (W::splat(1u) << (nv * 8u)) - 1u);     /* the low nv bytes count */
                const V32 ea = cbc_stats_zero_bytes<W>(v ^ 0x41414141u), ec = cbc_stats_zero_bytes<W>(v ^ 0x43434343u);
                const V32 eg = cbc_stats_zero_bytes<W>(v ^ 0x47474747u), et = cbc_stats_zero_bytes<W>(v ^ 0x54545454u);
                acc_a = acc_a + (rev ? et : ea); acc_t = acc_t + (rev ? ea : et);
                acc_c = acc_c + (rev ? eg : ec); acc_g = acc_g + (rev ? ec : eg);
                const V32 cg = ec + eg;                              /* 0 / 1 per byte: a byte is not both */
                uint32_t gc = 0;
                for (uint32_t b = 0; b < 4u; b++) gc += W::popc64(W::ballot((cg & (1u << (8u * b))) != 0u));
                W::set_lane(gcv, j, gc);
                if (!more) break;
                cur = nxt; j = jn;
            }
        }
        /* the unit's cycle counts: lane l, byte b of a register = cycle 4 l + b */
        for (uint32_t b = 0; b < 4u; b++) {
            const V32 at = ln * 4u + (CBC_STATS_L_CYC + b);
            const V32 xa = (acc_a >> (8u * b)) & 0xffu, xc = (acc_c >> (8u * b)) & 0xffu;
            const V32 xg = (acc_g >> (8u * b)) & 0xffu, xt = (acc_t >> (8u * b)) & 0xffu;
            W::lds_add(lds, at, xa, xa != 0u);
            W::lds_add(lds, at + CBC_STATS_CYCLES, xc, xc != 0u);
            W::lds_add(lds, at + 2u * CBC_STATS_CYCLES, xg, xg != 0u);
            W::lds_add(lds, at + 3u * CBC_STATS_CYCLES, xt, xt != 0u);
        }
        /* the per-read tables, one lane per read */
        const Mask lo = c & (fl < CBC_STATS_FLAGS_LDS);
        W::lds_add(lds, fl, W::splat(1u), lo);
        W::list_add(A.tab, fl, W::splat(1u), c & !lo);               /* fl <= 65535 */
        W::lds_add(lds, rlv + CBC_STATS_L_LEN, W::splat(1u), c);     /* rlv <= stride <= 256 */
        /* floor(100 gc / len), gc <= len <= 256: restoring division, the quotient is below 128 */
        V32 n = gcv * 100u, q = W::splat(0u);
        for (int b = 6; b >= 0; b--) {
            const V32 t = rlv << (uint32_t)b;
            const Mask ge = n >= t;
            n = W::select(ge, n - t, n);
            q = W::select(ge, q + (1u << b), q);
        }
        W::lds_add(lds, q + CBC_STATS_L_GC, W::splat(1u), c & (rlv != 0u) & (q < CBC_STATS_GC_BINS));
    }
    W::list_add(A.tab, W::splat(CBC_STATS_T_CTR), W::splat(n_excl), (ln == 0u) & (n_excl != 0u));
}

/* host side: the device's table `w` (CBC_STATS_WORDS) into the caller's struct.  reads = the sum of the length table; the fifth
 * cycle row: the reads that reach cycle c (those longer than c) less the four letters */
static inline void cbc_stats_finish(const uint32_t *w, cbc_gpu_stats *st)
{
    memcpy(st->flag, w + CBC_STATS_T_FLAG, sizeof st->flag);
    memcpy(st->len, w + CBC_STATS_T_LEN, sizeof st->len);
    memcpy(st->gc, w + CBC_STATS_T_GC, sizeof st->gc);
    memcpy(st->cyc, w + CBC_STATS_T_CYC, (size_t)4u * CBC_STATS_CYCLES * 4u);
    st->excluded = w[CBC_STATS_T_CTR];
    st->reads = 0;
    for (uint32_t l = 0; l < CBC_STATS_LEN_BINS; l++) st->reads += st->len[l];
    uint64_t reach = st->reads - st->len[0];
    for (uint32_t c = 0; c < CBC_STATS_CYCLES; c++) {
        uint64_t four = 0;
        for (uint32_t s = 0; s < 4u; s++) four += st->cyc[s * CBC_STATS_CYCLES + c];
        st->cyc[4u * CBC_STATS_CYCLES + c] = (uint32_t)(reach - four);
        reach -= st->len[c + 1u];
    }
}

#endif /* CBC_STATS_BODY_H */
