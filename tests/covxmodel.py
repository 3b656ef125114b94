"""Per-query read counts and depth thresholds in plain Python: what `cbc -x --bedcov --thresholds ..
--count-reads` must write.  Brute force on top of depthmodel.depth_array and covmodel: a threshold column is a count over a numpy
slice of the per-base depth, a read count is a pass over the read list with the overlap rule POS <= end and POS + span - 1 >= beg.
The read list is either view of section 4.13 (the packed arrays: depthmodel.intervals_a; POS + CIGAR of the SAM text:
depthmodel.intervals_b); on clip-free input the two must agree before either is used.  Also the ctypes wrapper of the emulation
library (tests/covx_emu)."""
import ctypes

import numpy as np

import covmodel as cm
from cbc_amd import host


# ---- ground truth ------------------------------------------------------------------------------------------------------------
def thr_expected(depth, queries, thresholds):
    """queries: [(contig or -1, start0, end0)], clamped; depth: covmodel.Depth.  Returns [[positions with depth >= T] per query]."""
    out = []
    for c, s, e in queries:
        if c < 0 or e <= s:
            out.append([0] * len(thresholds))
            continue
        d = depth.contig(c)[s:e]
        assert len(d) == e - s
        out.append([int(np.count_nonzero(d >= t)) for t in thresholds])
    return out


class Reads:
    """The kept reads of a read list [(contig, POS, span, FLAG[, block])] as per-contig arrays, made once and counted per query."""

    def __init__(self, iv, exclude=0, skip_blocks=()):
        self.by = {}
        for x in iv:
            if x[2] >= 1 and not (x[3] & exclude) and (len(x) < 5 or x[4] not in skip_blocks):
                self.by.setdefault(x[0], []).append((x[1], x[1] + x[2] - 1))
        self.by = {c: np.array(v, dtype=np.int64) for c, v in self.by.items()}

    def kept(self, c):
        return len(self.by.get(c, ()))

    def count(self, c, start0, end0):
        """Reads with POS <= end and POS + span - 1 >= beg for beg = start0 + 1, end = end0 (1-based, inclusive)."""
        if c < 0 or end0 <= start0 or c not in self.by:
            return 0
        a = self.by[c]
        return int(np.count_nonzero((a[:, 0] <= end0) & (a[:, 1] >= start0 + 1)))


def reads_loop(iv, queries, exclude=0):
    """The same by the plainest loop there is (small inputs): one pass over the read list per query."""
    out = []
    for c, s, e in queries:
        n = 0
        for x in iv:
            if x[0] == c and e > s and x[2] >= 1 and not (x[3] & exclude) and x[1] <= e and x[1] + x[2] - 1 >= s + 1:
                n += 1
        out.append(n)
    return out


def reads_expected(reads, queries):
    return [reads.count(c, s, e) for c, s, e in queries]


def text(chroms, queries, sums, covs, thr=None, reads=None):
    """The lines of `cbc -x --bedcov [--thresholds ..] [--count-reads]`: the six columns, one per threshold, reads last."""
    out = []
    for i, (n, (_, s, e), t, k) in enumerate(zip(chroms, queries, sums, covs)):
        ln = b"%s\t%d\t%d\t%d\t%d\t%s" % (n, s, e, t, k, cm.mean_text(t, e - s))
        if thr is not None:
            ln += b"".join(b"\t%d" % x for x in thr[i])
        if reads is not None:
            ln += b"\t%d" % reads[i]
        out.append(ln + b"\n")
    return b"".join(out)


# ---- the emulation library -----------------------------------------------------------------------------------------------------
def emu_load(path):
    L = ctypes.CDLL(path)
    V, U32, U64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    L.emu_covx_decode.restype = ctypes.c_int
    L.emu_covx_decode.argtypes = [V, U32]
    L.emu_targets_decode = L.emu_covx_decode                 # targetsmodel.emu_decode_all drives the decoder under this name
    L.emu_covx.restype = ctypes.c_int
    L.emu_covx.argtypes = [V, U64, V, U64, V, V, V, U32, V, U32, V, U32, U32, V, U32, V, V, V, U32, V, V, V]
    L.emu_covx_points.restype = ctypes.c_int
    L.emu_covx_points.argtypes = [V, V, U32, V, V, U32, U32, V, U32, V, U32, V, V]
    return L


def emu_covx(L, plan, dec, qs, thresholds=(), count_reads=True, exclude=0, min_depth=1, fail_blocks=()):
    """The calls of Encoder.decode_coverage(thresholds=, count_reads=) on the emulation: one per contig that has queries,
    intervals and blocks.  dec: targetsmodel.emu_decode_all.  Returns a dict: sum, covered, thr ([n_q][T]), reads (or None),
    rcs (per call), kept (reads kept per call), nsp (start points per call)."""
    ts = qs.targets
    T = len(thresholds)
    thr = np.ascontiguousarray(thresholds, dtype=np.uint32)
    length = (qs.end0 - qs.start0).astype(np.uint64)
    total, covered = np.zeros(qs.n_q, dtype=np.uint64), np.zeros(qs.n_q, dtype=np.uint32)
    xthr, xrd = np.zeros((qs.n_q, T), dtype=np.uint32), np.zeros(qs.n_q, dtype=np.uint32)
    rcs, kept, nsp = [], [], []
    for c in range(ts.n_contigs):
        k0, nb, f, n = int(ts.contig_blk_first[c]), int(ts.contig_blk_count[c]), int(ts.contig_first[c]), int(ts.contig_count[c])
        idx = np.flatnonzero((qs.contig == c) & (length > 0))
        if not nb or not n or not len(idx):
            continue
        sel = ts.blocks[k0:k0 + nb].astype(np.int64)
        bl = np.ascontiguousarray(dec["bl"][sel])
        ws = np.ascontiguousarray(plan.window_start[sel], dtype=np.uint64)
        res = dec["res"][sel].copy()
        for b in fail_blocks:
            if k0 <= b < k0 + nb:
                res[b - k0]["status"] = 2
        iv = np.ascontiguousarray(ts.iv[f:f + n], dtype=np.uint32)
        biv = np.ascontiguousarray(ts.block_iv[k0:k0 + nb], dtype=np.uint32).copy()
        biv[:, 0] -= np.uint32(f)
        q = np.ascontiguousarray(np.stack([qs.q["slot"][idx], length[idx].astype(np.uint32)], axis=1), dtype=np.uint32)
        s, cv, out = np.zeros(len(idx), dtype=np.uint64), np.zeros(len(idx), dtype=np.uint32), np.zeros(4, dtype=np.uint64)
        tc, rd = np.full((len(idx), T), 0xEE, dtype=np.uint32), np.full(len(idx), 0xEE, dtype=np.uint32)
        rc = L.emu_covx(dec["recs"].ctypes.data, dec["nrec"], dec["seq"].ctypes.data, dec["seq"].size, bl.ctypes.data, ws.ctypes.data,
                        res.ctypes.data, nb, iv.ctypes.data, n, biv.ctypes.data, exclude, min_depth, q.ctypes.data, len(idx),
                        s.ctypes.data, cv.ctypes.data, thr.ctypes.data if T else None, T, tc.ctypes.data if T else None,
                        rd.ctypes.data if count_reads else None, out.ctypes.data)
        assert rc in (0, -4), rc
        total[idx], covered[idx], xthr[idx] = s, cv, tc
        if count_reads:
            xrd[idx] = rd
        rcs.append(rc); kept.append(int(out[0])); nsp.append(int(out[3]))
    return dict(sum=[int(x) for x in total], covered=[int(x) for x in covered], thr=[[int(x) for x in r] for r in xthr],
                reads=[int(x) for x in xrd] if count_reads else None, rcs=rcs, kept=kept, nsp=nsp)


def emu_points(L, cp_pos, cp_dep, sp_pos, sp_cnt, slots, thresholds, q, count_reads=True):
    """Fabricated change points and start points straight into the weights / scan / apply / lookup bodies.
    Returns ([[thr] per query], [reads] or None)."""
    pos, dep = np.ascontiguousarray(cp_pos, dtype=np.uint32), np.ascontiguousarray(cp_dep, dtype=np.uint32)
    sp, sc = np.ascontiguousarray(sp_pos, dtype=np.uint32), np.ascontiguousarray(sp_cnt, dtype=np.uint32)
    thr = np.ascontiguousarray(thresholds, dtype=np.uint32)
    qq = np.ascontiguousarray(q, dtype=np.uint32).reshape(-1, 2)
    T = len(thr)
    tc, rd = np.zeros((len(qq), T), dtype=np.uint32), np.zeros(len(qq), dtype=np.uint32)
    rc = L.emu_covx_points(pos.ctypes.data, dep.ctypes.data, len(pos), sp.ctypes.data, sc.ctypes.data, len(sp), slots,
                           thr.ctypes.data if T else None, T, qq.ctypes.data, len(qq), tc.ctypes.data if T else None,
                           rd.ctypes.data if count_reads else None)
    assert rc == 0, rc
    return [[int(x) for x in r] for r in tc], ([int(x) for x in rd] if count_reads else None)


def points_expected(cp_pos, cp_dep, sp_pos, sp_cnt, thresholds, q):
    """Python integers: the depth is cp_dep[j] on [cp_pos[j], cp_pos[j + 1]) and 0 outside the change points; CS(y) is the
    count of the last start point at or below y (0 in front of the first), and reads = depth(x) + CS(x + len - 1) - CS(x)
    modulo 2^32 for len >= 1."""
    thr, rds = [], []
    for slot, ln in q:
        row = []
        for t in thresholds:
            k = 0
            for j in range(len(cp_pos) - 1):
                a, b = max(int(cp_pos[j]), slot), min(int(cp_pos[j + 1]), slot + ln)
                if b > a and int(cp_dep[j]) >= t:
                    k += b - a
            row.append(k)
        thr.append(row)
        depth = 0
        for j in range(len(cp_pos) - 1):
            if int(cp_pos[j]) <= slot < int(cp_pos[j + 1]):
                depth = int(cp_dep[j])

        def cs(y):
            v = 0
            for p, c in zip(sp_pos, sp_cnt):
                if int(p) <= y:
                    v = int(c)
            return v
        rds.append((depth + cs(slot + ln - 1) - cs(slot)) % 2 ** 32 if ln else 0)
    return thr, rds
