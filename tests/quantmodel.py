"""Per-query depth quantiles in plain Python: what `cbc -x --bedcov --quantiles ..` must write.  Brute
force on top of covmodel.Depth: a query is a numpy slice of the per-base depth, sorted, and the value of rank
k = max(1, ceil(p * len / 100)) is read off with k in Python integers.  For fabricated change points the runs are expanded to
(depth, length) pairs, sorted and walked.  Also the text of the lines and the ctypes wrapper of the emulation library
(tests/quant_emu)."""
import ctypes

import numpy as np

import covxmodel as cx


# ---- ground truth ------------------------------------------------------------------------------------------------------------
def rank(p, length):
    """k = max(1, ceil(p * len / 100)) in Python integers."""
    return max(1, -((-p * length) // 100))


def quant_expected(depth, queries, pcts):
    """queries: [(contig or -1, start0, end0)], clamped; depth: covmodel.Depth.  Returns [[quantile per p] per query]."""
    out = []
    for c, s, e in queries:
        if c < 0 or e <= s:
            out.append([0] * len(pcts))
            continue
        d = np.sort(depth.contig(c)[s:e])
        assert len(d) == e - s
        out.append([int(d[rank(p, e - s) - 1]) for p in pcts])
    return out


def hist_quantiles(depths, bases, size, pcts):
    """The same from a histogram: bins (depth, bases) with bases > 0, ascending; what they leave of `size` is depth 0 (the C
    call leaves the depth-0 bin out, Encoder.decode_depth_hist lists it)."""
    pairs = [(0, int(size) - sum(int(b) for b in bases))] + [(int(d), int(b)) for d, b in zip(depths, bases)]
    return _walk(pairs, int(size), pcts)


def _walk(pairs, length, pcts):
    if length == 0:
        return [0] * len(pcts)
    pairs = sorted(x for x in pairs if x[1] > 0)
    row = []
    for p in pcts:
        k, cum = rank(p, length), 0
        for d, n in pairs:
            cum += n
            if cum >= k:
                row.append(d)
                break
    assert len(row) == len(pcts)
    return row


def points_expected(cp_pos, cp_dep, pcts, q):
    """Python integers: the depth is cp_dep[j] on [cp_pos[j], cp_pos[j + 1]) and 0 outside the change points; the clipped runs of
    a query as (depth, length) pairs with the zeros as one more, sorted and walked."""
    pos, dep = [int(x) for x in cp_pos], [int(x) for x in cp_dep]
    out = []
    for slot, ln in q:
        pairs, nz = [], 0
        for j in range(len(pos) - 1):
            a, b = max(pos[j], slot), min(pos[j + 1], slot + ln)
            if b > a and dep[j]:
                pairs.append((dep[j], b - a)); nz += b - a
        out.append(_walk(pairs + [(0, ln - nz)], ln, pcts))
    return out


def text(chroms, queries, sums, covs, thr=None, quant=None, reads=None):
    """The lines of `cbc -x --bedcov [--thresholds ..] [--quantiles ..] [--count-reads]`: covxmodel.text with one column per
    percentage behind the thresholds' and in front of the read count."""
    base = cx.text(chroms, queries, sums, covs, thr).split(b"\n")[:-1]
    out = []
    for i, ln in enumerate(base):
        if quant is not None:
            ln += b"".join(b"\t%d" % x for x in quant[i])
        if reads is not None:
            ln += b"\t%d" % reads[i]
        out.append(ln + b"\n")
    return b"".join(out)


# ---- the emulation library -----------------------------------------------------------------------------------------------------
def emu_load(path):
    L = ctypes.CDLL(path)
    V, U32, U64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    L.emu_quant_decode.restype = ctypes.c_int
    L.emu_quant_decode.argtypes = [V, U32]
    L.emu_targets_decode = L.emu_quant_decode                # targetsmodel.emu_decode_all drives the decoder under this name
    L.emu_quant.restype = ctypes.c_int
    L.emu_quant.argtypes = [V, U64, V, U64, V, V, V, U32, V, U32, V, U32, V, U32, V, U32, V, V]
    L.emu_quant_points.restype = ctypes.c_int
    L.emu_quant_points.argtypes = [V, V, U32, U32, V, U32, V, U32, V]
    return L


def emu_quant(L, plan, dec, qs, pcts, exclude=0, fail_blocks=()):
    """The calls of Encoder.decode_coverage_quant on the emulation: one per contig that has queries, intervals and blocks.
    dec: targetsmodel.emu_decode_all.  Returns a dict: quant ([n_q][len(pcts)]), rcs (per call), kept, ncp (per call)."""
    ts = qs.targets
    P = len(pcts)
    pct = np.ascontiguousarray(pcts, dtype=np.uint32)
    length = (qs.end0 - qs.start0).astype(np.uint64)
    xq = np.zeros((qs.n_q, P), dtype=np.uint32)
    rcs, kept, ncp = [], [], []
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
        qd, out = np.full((len(idx), P), 0xEE, dtype=np.uint32), np.zeros(3, dtype=np.uint64)
        rc = L.emu_quant(dec["recs"].ctypes.data, dec["nrec"], dec["seq"].ctypes.data, dec["seq"].size, bl.ctypes.data, ws.ctypes.data,
                         res.ctypes.data, nb, iv.ctypes.data, n, biv.ctypes.data, exclude, q.ctypes.data, len(idx), pct.ctypes.data, P,
                         qd.ctypes.data, out.ctypes.data)
        assert rc in (0, -4), rc
        xq[idx] = qd
        rcs.append(rc); kept.append(int(out[0])); ncp.append(int(out[1]))
    return dict(quant=[[int(x) for x in r] for r in xq], rcs=rcs, kept=kept, ncp=ncp)


def emu_points(L, cp_pos, cp_dep, slots, pcts, q):
    """Fabricated change points straight into the selection body.  Returns [[quantile per p] per query]."""
    pos, dep = np.ascontiguousarray(cp_pos, dtype=np.uint32), np.ascontiguousarray(cp_dep, dtype=np.uint32)
    pct = np.ascontiguousarray(pcts, dtype=np.uint32)
    qq = np.ascontiguousarray(q, dtype=np.uint32).reshape(-1, 2)
    out = np.full((len(qq), len(pct)), 0xEE, dtype=np.uint32)
    rc = L.emu_quant_points(pos.ctypes.data, dep.ctypes.data, len(pos), slots, pct.ctypes.data, len(pct), qq.ctypes.data, len(qq), out.ctypes.data)
    assert rc == 0, rc
    return [[int(x) for x in r] for r in out]
