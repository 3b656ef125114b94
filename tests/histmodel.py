"""Depth histogram in plain Python: what `cbc -x --depth-hist` must write.  Brute force and nothing new
as ground truth: the per-base depth of a contig is depthmodel.depth_array (through covmodel.Depth; the two interval models of
section 4.13 must agree before either is used: depthmodel.assert_models_agree), restricted to the merged intervals, binned with
np.bincount and folded at max_depth; the fraction rule is restated in Python integers.  Also the ctypes wrapper of the emulation
library (tests/hist_emu)."""
import ctypes

import numpy as np

import targetsmodel as tm


# ---- ground truth ------------------------------------------------------------------------------------------------------------
def expected(depth, lens, ivs=None, max_depth=0):
    """depth: covmodel.Depth.  ivs: [(contig, beg, end)] 1-based inclusive, in any order and overlapping (None: every contig
    whole).  Returns [(contig, [(depth, bases)] ascending with bases > 0, size)] for the contigs an interval lies on."""
    merged = tm.merge(ivs) if ivs is not None else [(c, 1, n) for c, n in enumerate(lens)]
    out = []
    for c in sorted({m[0] for m in merged}):
        d = depth.contig(c)
        vals = np.concatenate([d[b - 1:e] for cc, b, e in merged if cc == c])          # merged: every position once
        size = int(sum(e - b + 1 for cc, b, e in merged if cc == c))
        assert len(vals) == size
        if max_depth:
            vals = np.minimum(vals, max_depth)
        cnt = np.bincount(vals)
        out.append((c, [(int(k), int(n)) for k, n in enumerate(cnt.tolist()) if n], size))
    return out


def fraction(bases, size):
    """The integer rule of the issue: m = (bases * 10^6 + size / 2) / size, printed as m / 10^6 '.' six digits."""
    if size == 0:
        return b"0.000000"
    m = (bases * 10 ** 6 + size // 2) // size
    return b"%d.%06d" % (m // 10 ** 6, m % 10 ** 6)


def genome(rows):
    """The bins summed over the listed contigs, and the sum of their sizes."""
    tot = {}
    for _, bins, _ in rows:
        for k, n in bins:
            tot[k] = tot.get(k, 0) + n
    return sorted(tot.items()), sum(s for _, _, s in rows)


def text(rows, names):
    """The lines `cbc -x --depth-hist` writes: per contig chrom, depth, bases, size, fraction; then the genome block (none when
    no contig is listed)."""
    out = [b"%s\t%d\t%d\t%d\t%s\n" % (names[c], k, n, size, fraction(n, size)) for c, bins, size in rows for k, n in bins]
    if rows:
        g, gs = genome(rows)
        out += [b"genome\t%d\t%d\t%d\t%s\n" % (k, n, gs, fraction(n, gs)) for k, n in g]
    return b"".join(out)


def as_rows(result):
    """What Encoder.decode_depth_hist / emu_hist return, as the model's rows."""
    return [(c, list(zip([int(x) for x in d], [int(x) for x in b])), int(size)) for c, d, b, size in result]


def points_expected(cp_pos, cp_dep, max_depth=0):
    """Python integers: run j = [cp_pos[j], cp_pos[j + 1]) has depth cp_dep[j]; runs of depth 0 are left out."""
    tot = {}
    for j in range(len(cp_pos) - 1):
        d = int(cp_dep[j])
        if d:
            k = min(d, max_depth) if max_depth else d
            tot[k] = tot.get(k, 0) + int(cp_pos[j + 1]) - int(cp_pos[j])
    return sorted(tot.items())


# ---- the emulation library -----------------------------------------------------------------------------------------------------
def emu_load(path):
    L = ctypes.CDLL(path)
    V, U32, U64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    L.emu_hist_decode.restype = ctypes.c_int
    L.emu_hist_decode.argtypes = [V, U32]
    L.emu_targets_decode = L.emu_hist_decode                 # targetsmodel.emu_decode_all drives the decoder under this name
    L.emu_hist.restype = ctypes.c_int
    L.emu_hist.argtypes = [V, U64, V, U64, V, V, V, U32, V, U32, V, U32, U32, V, V, U32, V, V]
    L.emu_hist_points.restype = ctypes.c_int
    L.emu_hist_points.argtypes = [V, V, U32, U64, U32, U32, V, V, U32, V]
    return L


def emu_hist(L, plan, dec, ts, exclude=0, max_depth=0, fail_blocks=()):
    """The calls of Encoder.decode_depth_hist on the emulation: one per contig that has intervals and blocks; the depth-0 bin is
    size less the others, as the host does it.  dec: targetsmodel.emu_decode_all.  Returns (rows as as_rows gives them, [rc per
    call])."""
    rows, rcs = [], []
    for c in range(ts.n_contigs):
        k0, nb, f, n = int(ts.contig_blk_first[c]), int(ts.contig_blk_count[c]), int(ts.contig_first[c]), int(ts.contig_count[c])
        if not n:
            continue
        size = ts.size[c]
        bins = []
        if nb:
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
            cap = max(1, min(int(bl["n_reads"].astype(np.int64).sum()), max_depth or 0xffffffff))
            bd, bb = np.full(cap + 1, 0xEEEEEEEE, dtype=np.uint32), np.full(cap + 1, 0xEEEEEEEE, dtype=np.uint32)
            nbin, out = np.zeros(1, dtype=np.uint32), np.zeros(3, dtype=np.uint64)
            rc = L.emu_hist(dec["recs"].ctypes.data, dec["nrec"], dec["seq"].ctypes.data, dec["seq"].size, bl.ctypes.data, ws.ctypes.data,
                            res.ctypes.data, nb, iv.ctypes.data, n, biv.ctypes.data, exclude, max_depth, bd.ctypes.data, bb.ctypes.data,
                            cap, nbin.ctypes.data, out.ctypes.data)
            assert rc in (0, -4), rc
            assert int(out[2]) == int((iv[:, 1].astype(np.int64) - iv[:, 0] + 2).sum())          # memory follows the set
            k = int(nbin[0])
            assert (bd[k:] == 0xEEEEEEEE).all() and (bb[k:] == 0xEEEEEEEE).all() and (rc == 0 or k == 0)
            bins = list(zip(bd[:k].tolist(), bb[:k].tolist()))
            rcs.append(rc)
        zero = size - sum(b for _, b in bins)
        assert zero >= 0
        rows.append((c, ([(0, zero)] if zero else []) + bins, size))
    return rows, rcs


def emu_points(L, cp_pos, cp_dep, reads, max_depth=0, grid=0, bin_cap=None):
    """Fabricated change points straight into the zero / accumulate / count / scan / write bodies.  Returns (rc, n_bins,
    [(depth, bases)])."""
    pos, dep = np.ascontiguousarray(cp_pos, dtype=np.uint32), np.ascontiguousarray(cp_dep, dtype=np.uint32)
    cap = len(pos) if bin_cap is None else bin_cap
    bd, bb = np.full(cap + 1, 0xEEEEEEEE, dtype=np.uint32), np.full(cap + 1, 0xEEEEEEEE, dtype=np.uint32)
    nbin = np.zeros(1, dtype=np.uint32)
    rc = L.emu_hist_points(pos.ctypes.data, dep.ctypes.data, len(pos), reads, max_depth, grid, bd.ctypes.data, bb.ctypes.data, cap, nbin.ctypes.data)
    k = int(nbin[0]) if rc == 0 else 0
    assert (bd[k:] == 0xEEEEEEEE).all() and (bb[k:] == 0xEEEEEEEE).all(), "pairs written past the count"
    return rc, int(nbin[0]), list(zip(bd[:k].tolist(), bb[:k].tolist()))
