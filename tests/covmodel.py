"""Per-target coverage summary in plain Python: what `cbc -x --bedcov` must write.  Brute force and
nothing new as ground truth: the per-base depth of a contig is depthmodel.depth_array (the two interval models of section 4.13
must agree before either is used: depthmodel.assert_models_agree), a query is a numpy slice of it, and sum, covered and the
two-decimal mean are restated in Python integers.  Also the ctypes wrapper of the emulation library (tests/cov_emu)."""
import ctypes

import numpy as np

import depthmodel as dm
import targetsmodel as tm
from cbc_amd import host


# ---- ground truth ------------------------------------------------------------------------------------------------------------
class Depth:
    """Per-base depth of whole contigs, made once per (exclude, skip_blocks) and sliced per query."""

    def __init__(self, iv, lens, exclude=0, skip_blocks=()):
        self.iv, self.lens, self.exclude, self.skip = iv, lens, exclude, tuple(skip_blocks)
        self._d = {}

    def contig(self, c):
        if c not in self._d:
            self._d[c] = dm.depth_array(self.iv, c, 1, self.lens[c], self.exclude, self.skip)[0]
        return self._d[c]


def expected(depth, queries, min_depth=1):
    """queries: [(contig or -1, start0, end0)], already clamped.  Returns ([sum], [covered]) as Python integers."""
    sums, covs = [], []
    for c, s, e in queries:
        if c < 0 or e <= s:
            sums.append(0); covs.append(0)
            continue
        d = depth.contig(c)[s:e]
        assert len(d) == e - s
        sums.append(sum(int(x) for x in d.tolist()))
        covs.append(int((d >= min_depth).sum()))
    return sums, covs


def mean_text(total, length):
    """The integer rule of the issue: q = sum / len, r = sum % len, m = q * 100 + (r * 100 + len / 2) / len."""
    if length == 0:
        return b"0.00"
    q, r = divmod(total, length)
    m = q * 100 + (r * 100 + length // 2) // length
    return b"%d.%02d" % (m // 100, m % 100)


def clamp(c, start0, end0, lens):
    """What a BED line of a known contig becomes: both ends clamped to the contig."""
    return (c, min(start0, lens[c]), min(end0, lens[c]))


def cut(queries, window):
    """Every query replaced by its windows of `window` bases from its own start on (a query without a position stays)."""
    out = []
    for c, s, e in queries:
        if not window or e <= s:
            out.append((c, s, e))
        else:
            out += [(c, a, min(a + window, e)) for a in range(s, e, window)]
    return out


def text(chroms, queries, sums, covs):
    """The lines `cbc -x --bedcov` writes: chrom, start0, end0, sum, covered, mean."""
    return b"".join(b"%s\t%d\t%d\t%d\t%d\t%s\n" % (n, s, e, t, k, mean_text(t, e - s)) for n, (_, s, e), t, k in zip(chroms, queries, sums, covs))


def of_intervals(ivs):
    """(contig, beg, end) 1-based inclusive -> (contig, start0, end0)."""
    return [(c, b - 1, e) for c, b, e in ivs]


def bed(queries, names):
    """BED text of (contig, start0, end0) queries; names[c] or, for c = -1, an unknown chrom."""
    return b"".join((names[c] if c >= 0 else b"chrUn_gl0") + b"\t%d\t%d\n" % (s, e) for c, s, e in queries)


def check_queryset(qs, want, names):
    """The QuerySet holds `want` = [(contig or -1, start0, end0)] in order, with the chrom texts."""
    got = list(zip(qs.contig.tolist(), qs.start0.tolist(), qs.end0.tolist()))
    assert got == [tuple(x) for x in want], (got[:5], want[:5])
    assert [qs.chrom(i) for i in range(qs.n_q)] == [names[c] if c >= 0 else b"chrUn_gl0" for c, _, _ in want]


# ---- the emulation library -----------------------------------------------------------------------------------------------------
def emu_load(path):
    L = ctypes.CDLL(path)
    V, U32, U64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    L.emu_cov_decode.restype = ctypes.c_int
    L.emu_cov_decode.argtypes = [V, U32]
    L.emu_targets_decode = L.emu_cov_decode                  # targetsmodel.emu_decode_all drives the decoder under this name
    L.emu_cov.restype = ctypes.c_int
    L.emu_cov.argtypes = [V, U64, V, U64, V, V, V, U32, V, U32, V, U32, U32, V, U32, V, V, V]
    L.emu_cov_points.restype = ctypes.c_int
    L.emu_cov_points.argtypes = [V, V, U32, U32, U32, V, U32, V, V]
    return L


def emu_cov(L, plan, dec, qs, exclude=0, min_depth=1, fail_blocks=()):
    """The calls of Encoder.decode_coverage on the emulation: one per contig that has queries, intervals and blocks.
    dec: targetsmodel.emu_decode_all.  Returns ([sum], [covered], [rc per call], slots of the calls)."""
    ts = qs.targets
    length = (qs.end0 - qs.start0).astype(np.uint64)
    total, covered = np.zeros(qs.n_q, dtype=np.uint64), np.zeros(qs.n_q, dtype=np.uint32)
    rcs, slots = [], 0
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
        s, cv, out = np.zeros(len(idx), dtype=np.uint64), np.zeros(len(idx), dtype=np.uint32), np.zeros(3, dtype=np.uint64)
        rc = L.emu_cov(dec["recs"].ctypes.data, dec["nrec"], dec["seq"].ctypes.data, dec["seq"].size, bl.ctypes.data, ws.ctypes.data,
                       res.ctypes.data, nb, iv.ctypes.data, n, biv.ctypes.data, exclude, min_depth, q.ctypes.data, len(idx),
                       s.ctypes.data, cv.ctypes.data, out.ctypes.data)
        assert rc in (0, -4), rc
        assert int(out[2]) == int((iv[:, 1].astype(np.int64) - iv[:, 0] + 2).sum())          # memory follows the set
        total[idx], covered[idx] = s, cv
        rcs.append(rc); slots += int(out[2])
    return [int(x) for x in total], [int(x) for x in covered], rcs, slots


def emu_points(L, cp_pos, cp_dep, slots, q, min_depth=1):
    """Fabricated change points straight into the weights / scan / apply / lookup bodies.  Returns ([sum], [covered])."""
    pos, dep = np.ascontiguousarray(cp_pos, dtype=np.uint32), np.ascontiguousarray(cp_dep, dtype=np.uint32)
    qq = np.ascontiguousarray(q, dtype=np.uint32).reshape(-1, 2)
    s, cv = np.zeros(len(qq), dtype=np.uint64), np.zeros(len(qq), dtype=np.uint32)
    rc = L.emu_cov_points(pos.ctypes.data, dep.ctypes.data, len(pos), slots, min_depth, qq.ctypes.data, len(qq), s.ctypes.data, cv.ctypes.data)
    assert rc == 0, rc
    return [int(x) for x in s], [int(x) for x in cv]


def points_expected(cp_pos, cp_dep, q, min_depth=1):
    """Python integers: the depth is cp_dep[j] on [cp_pos[j], cp_pos[j + 1]) and 0 outside the change points."""
    sums, covs = [], []
    for slot, ln in q:
        t = k = 0
        for j in range(len(cp_pos) - 1):
            a, b = max(int(cp_pos[j]), slot), min(int(cp_pos[j + 1]), slot + ln)
            if b > a:
                t += int(cp_dep[j]) * (b - a)
                k += (b - a) if int(cp_dep[j]) >= min_depth else 0
        sums.append(t); covs.append(k)
    return sums, covs


def carry_points(seed=1, n=2500):
    """Change points whose weights pass 2^32 everywhere: depths near 4 * 10^9, runs near 10^6 slots, more than two tiles of
    runs; the last change point has depth 0.  Returns (cp_pos, cp_dep, slots)."""
    rng = np.random.default_rng(seed)
    pos = np.cumsum(rng.integers(900_000, 1_100_000, n)).astype(np.int64) + 17
    dep = rng.integers(3_900_000_000, 4_200_000_000, n).astype(np.int64)
    dep[-1] = 0
    dep[n // 3] = 1; dep[n // 2] = 0                       # a shallow and an empty run between the deep ones
    assert pos[-1] < 2 ** 32 - 10
    return pos, dep, int(pos[-1]) + 5


def selfcheck(L):
    """The ramp and a small mixed dataset through every pass, and the 64-bit carries: what the AddressSanitizer child of
    tests/test_coverage.py runs."""
    for make, kw in ((dm.ramp, {}), (dm.mixed, dict(seed=3, block_reads=64, n=400))):
        fa, sam, pb, contigs = make(**kw)
        ivm = dm.assert_models_agree(pb, sam)
        names, lens = dm.names_lens(None, contigs)
        import regionmodel as rm
        plan = host.UnpackPlan(rm.container(pb), fa)
        rng = np.random.default_rng(9)
        qs_in = []
        for _ in range(150):
            c = int(rng.integers(0, len(lens)))
            s = int(rng.integers(0, lens[c]))
            qs_in.append((c, s, min(lens[c], s + int(rng.choice([0, 1, 40, 300, 5000])))))
        qs_in += [(-1, 5, 900), (0, 0, lens[0])]
        for window in (0, 97):
            qs = plan.queries((), bed(qs_in, names), window)
            want = cut(qs_in, window)
            check_queryset(qs, want, names)
            dec = tm.emu_decode_all(L, plan, qs.targets.smax)
            for ex, md in ((0, 1), (16, 2)):
                s, c, rcs, _ = emu_cov(L, plan, dec, qs, ex, md)
                assert (s, c) == expected(Depth(ivm, lens, ex), want, md), (make.__name__, window, ex, md)
                assert all(r == 0 for r in rcs)
        plan.close(); pb.close()
    pos, dep, slots = carry_points(n=1500)
    q = [(0, slots), (int(pos[3]), int(pos[1400] - pos[3])), (int(pos[700]) + 5, 10)]
    assert emu_points(L, pos, dep, slots, q) == points_expected(pos, dep, q)
    return True
