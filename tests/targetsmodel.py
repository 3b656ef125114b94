"""Decode of a set of regions in plain Python: what `cbc -x --region A --region B --regions-file F`
must write.  Nothing here is new ground truth: reads are regionmodel.selected OR-ed over the merged intervals, SAM lines the
same selection through sammodel.line, the depth the concatenation of depthmodel.expected per merged interval, the block list
the union of regionmodel.expected_blocks.  Also the interval sets the CPU and the GPU tests share and the ctypes wrapper of the
emulation library (tests/targets_emu)."""
import bisect
import ctypes

import numpy as np

import blockref
import depthmodel as dm
import regionmodel as rm
import sammodel as sm
from cbc_amd import host


# ---- the set ---------------------------------------------------------------------------------------------------------------
def merge(ivs):
    """[(contig, beg, end)] -> sorted per contig, overlapping or adjacent (end + 1 >= next beg) intervals merged."""
    out = []
    for c, b, e in sorted(ivs):
        if out and out[-1][0] == c and out[-1][2] + 1 >= b:
            out[-1] = (c, out[-1][1], max(out[-1][2], e))
        else:
            out.append((c, b, e))
    return out


def bed(ivs, names, sep=b"\t", eol=b"\n"):
    """BED text of 1-based inclusive intervals: chrom, start0, end0."""
    return b"".join(names[c] + sep + b"%d" % (b - 1) + sep + b"%d" % e + eol for c, b, e in ivs)


def region_strings(ivs, names):
    return [b"%s:%d-%d" % (names[c], b, e) for c, b, e in ivs]


# ---- ground truth from the existing models ---------------------------------------------------------------------------------
def kept_records(recs, merged, vectorised=None):
    """Indices of the records (regionmodel.records order = container order) that overlap at least one interval."""
    if not (len(merged) > 400 if vectorised is None else vectorised):
        ids = {id(r) for c, b, e in merged for r in rm.selected(recs, c, b, e)}
        return [i for i, r in enumerate(recs) if id(r) in ids]
    # the rule of regionmodel.selected, vectorised for the large sets (held equal to it on the small ones by the tests)
    rc = np.array([r[1] for r in recs]); pos = np.array([r[2] for r in recs], dtype=np.int64)
    last = pos + np.array([r[3] for r in recs], dtype=np.int64) - 1
    keep = np.zeros(len(recs), dtype=bool)
    for c, b, e in merged:
        keep |= (rc == c) & (pos <= e) & (last >= b)
    return np.flatnonzero(keep).tolist()


def expected_reads(recs, merged):
    return b"".join(recs[i][4] + b"\n" for i in kept_records(recs, merged))


def expected_sam(recs, flags, names, merged):
    """The alignment lines (no header) of the kept records; flags: FLAG per record in container order."""
    return b"".join(sm.line(flags[i], names[recs[i][1]], recs[i][2], recs[i][4]) for i in kept_records(recs, merged))


def expected_depth(iv, names, lens, merged, exclude=0, skip_blocks=()):
    """(bytes, runs) = depthmodel.expected per merged interval, appended.  Only the reads near an interval are handed to the
    model (the others cannot overlap it): a read starts at most `reach` bases in front of the interval."""
    reach = max([x[2] for x in iv] + [1])
    by_c = {}
    for x in iv:
        by_c.setdefault(x[0], []).append(x)
    for c in by_c:
        by_c[c].sort(key=lambda x: x[1])
    keys = {c: [x[1] for x in v] for c, v in by_c.items()}
    out, runs = [], 0
    for c, b, e in merged:
        v = by_c.get(c, [])
        near = v[bisect.bisect_left(keys.get(c, []), b - reach):bisect.bisect_right(keys.get(c, []), e)]
        t, r, _ = dm.expected(near, names, lens, (c, b, e), exclude, skip_blocks)
        out.append(t); runs += r
    return b"".join(out), runs


def expected_blocks(pb, merged, smax):
    s = set()
    for c, b, e in merged:
        w = rm.expected_blocks(pb, c, b, e, smax)
        if w:
            s.update(range(w[0], w[1]))
    return sorted(s)


# ---- interval sets -----------------------------------------------------------------------------------------------------------
def special_set(pb, recs, block_reads):
    """The hand-picked cases on the mixed dataset, as (contig, beg, end): a read overlapped by two intervals, 1-base intervals,
    an interval wholly between two reads, intervals touching at a block's first POS, adjacent / overlapping / duplicate /
    unsorted input, the deletion read's reach into block 1 -- all on contigs 0 and 2; contig 1 gets none."""
    c0 = [r for r in recs if r[1] == 0]
    # one read, two intervals: its first 3 and its last 3 bases -- the first read from the middle of the contig on for which
    # each interval also selects a read the other one does not (so neither interval alone gives the union's output)
    for mid in c0[len(c0) // 2:]:
        two = [(0, mid[2], mid[2] + 2), (0, mid[2] + mid[3] - 3, mid[2] + mid[3] - 1)]
        sa, sb = ({id(r) for r in rm.selected(recs, *t)} for t in two)
        if mid[3] > 6 and sa - sb and sb - sa:
            break
    else:
        raise AssertionError("no read whose two ends are shared with different neighbours")
    gap = None
    ends = 0
    for a in c0:                                                  # a stretch no read covers: wholly between two reads
        if ends and a[2] > ends + 3:
            gap = (0, ends + 1, a[2] - 1); break
        ends = max(ends, a[2] + a[3] - 1)
    assert gap is not None
    F1 = int(pb.info[1]["window_start"]) + 1                       # intervals touching at block 1's first POS
    touch = [(0, F1 - 20, F1 - 1), (0, F1, F1 + 20)]
    dpos = int(pb.recs[block_reads - 1]["pos"]) + int(pb.info[0]["window_start"])
    L3 = int(pb.contigs[2]["length"])
    out = two + [gap] + touch + [(0, dpos + 130, dpos + 135), (0, 5, 5), (0, 7, 7), (2, 1, 1), (2, L3, L3),
                                 (2, 3000, 3100), (2, 3050, 3200), (2, 3201, 3300), (2, 3000, 3100), (2, 900, 1000), (2, 100, 100)]
    return out, dict(two=two, read=mid, gap=gap, touch=touch)


def dense_set(contig, first, n, step, width):
    """n intervals of `width` bases every `step` bases from `first` on: more than one wavefront / one tile of intervals."""
    return [(contig, first + i * step, first + i * step + width - 1) for i in range(n)]


# ---- the emulation library ------------------------------------------------------------------------------------------------------
def emu_load(path):
    L = ctypes.CDLL(path)
    V, U32, U64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    L.emu_targets_decode.restype = ctypes.c_int
    L.emu_targets_decode.argtypes = [V, U32]
    L.emu_targets.restype = ctypes.c_int
    L.emu_targets.argtypes = [V, U64, V, U64, V, V, V, U32, V, V, U32, V, U32, V, ctypes.c_int, V, U64, U32, V]
    L.emu_targets_depth.restype = ctypes.c_int
    L.emu_targets_depth.argtypes = [V, U64, V, U64, V, V, V, U32, ctypes.c_char_p, U32, V, U32, V, U32, V, U64, V]
    return L


def emu_decode_all(L, plan, smax):
    """Every block of the plan, in the plan's own layout, by the emulated span decoder; a target set gathers from it."""
    bl = plan.blocks.copy()
    nrec = int(bl["n_reads"].sum())
    pay = np.concatenate([np.ascontiguousarray(plan.payloads), np.zeros(16, dtype=np.uint8)])
    recs = np.zeros(max(nrec, 1), dtype=host.REC_DTYPE)
    seq = np.zeros(nrec * plan.seq_stride + 40, dtype=np.uint8)
    res = np.zeros(plan.n_blocks, dtype=host.RESULT_DTYPE)
    vs = np.zeros(max(plan.n_blocks * plan.cap_var, 1), dtype=np.uint32)
    db = blockref.DecDeviceBatch(pay.ctypes.data, pay.size, bl.ctypes.data, plan.n_blocks, plan.ref.ctypes.data, len(plan.ref),
                                 recs.ctypes.data, nrec, seq.ctypes.data, seq.size, res.ctypes.data, vs.ctypes.data, vs.size,
                                 host.LdsCaps(plan.cap_pos, plan.cap_var))
    assert L.emu_targets_decode(ctypes.byref(db), smax) == 0
    assert (res["status"] == 0).all()
    return dict(bl=bl, recs=recs, seq=seq, res=res, nrec=nrec)


def _name(plan, c):
    off = int(plan.contig_name_off[c])
    return off, plan.names[off:].tobytes().split(b"\0", 1)[0]


def emu_text(L, plan, dec, ts, sam, n_waves=4, cap=None, fail_blocks=()):
    """One reads / SAM call of cbc_gpu_decode_targets on the emulation.  Returns (rc, text, reads kept, text bytes)."""
    if ts.n_blocks == 0:
        return 0, b"", 0, 0
    sel = ts.blocks.astype(np.int64)
    bl = np.ascontiguousarray(dec["bl"][sel])
    ws = np.ascontiguousarray(plan.window_start[sel], dtype=np.uint64)
    res = dec["res"][sel].copy()
    for b in fail_blocks:
        res[b]["status"] = 2
    bn = np.array([[_name(plan, int(plan.block_contig[b]))[0], len(_name(plan, int(plan.block_contig[b]))[1])] for b in sel], dtype=np.uint32)
    names = np.ascontiguousarray(plan.names)
    iv = np.ascontiguousarray(ts.iv, dtype=np.uint32); biv = np.ascontiguousarray(ts.block_iv, dtype=np.uint32)
    cap = (ts.text_cap_sam if sam else ts.text_cap_reads) if cap is None else cap
    text = np.full(cap + 16, 0xEE, dtype=np.uint8)
    out = np.zeros(2, dtype=np.uint64)
    rc = L.emu_targets(dec["recs"].ctypes.data, dec["nrec"], dec["seq"].ctypes.data, dec["seq"].size, bl.ctypes.data, ws.ctypes.data,
                       res.ctypes.data, len(sel), bn.ctypes.data, names.ctypes.data, names.size, iv.ctypes.data, ts.n_iv,
                       biv.ctypes.data, int(sam), text.ctypes.data, cap, n_waves, out.ctypes.data)
    total = int(out[0])
    assert (text[total if rc == 0 else 0:] == 0xEE).all(), "bytes written outside the text"
    return rc, (text[:total].tobytes() if rc == 0 else b""), int(out[1]), total


def emu_depth(L, plan, dec, ts, exclude=0, fail_blocks=(), name=None):
    """The depth calls of cbc_gpu_decode_targets on the emulation, one per contig with intervals and blocks, texts appended.
    Returns (text, lines, reads counted, words of the difference arrays)."""
    text, lines, kept, words = [], 0, 0, 0
    for c in range(ts.n_contigs):
        k0, nb = int(ts.contig_blk_first[c]), int(ts.contig_blk_count[c])
        if not nb:
            continue
        sel = ts.blocks[k0:k0 + nb].astype(np.int64)
        bl = np.ascontiguousarray(dec["bl"][sel])
        ws = np.ascontiguousarray(plan.window_start[sel], dtype=np.uint64)
        res = dec["res"][sel].copy()
        for b in fail_blocks:
            if k0 <= b < k0 + nb:
                res[b - k0]["status"] = 2
        f, n = int(ts.contig_first[c]), int(ts.contig_count[c])
        iv = np.ascontiguousarray(ts.iv[f:f + n], dtype=np.uint32)
        biv = np.ascontiguousarray(ts.block_iv[k0:k0 + nb], dtype=np.uint32).copy()
        biv[:, 0] -= np.uint32(f)
        nm = _name(plan, c)[1] if name is None else name
        cap = ts.depth_cap[c]
        buf = np.full(cap + 16, 0xEE, dtype=np.uint8)
        out = np.zeros(5, dtype=np.uint64)
        rc = L.emu_targets_depth(dec["recs"].ctypes.data, dec["nrec"], dec["seq"].ctypes.data, dec["seq"].size, bl.ctypes.data,
                                 ws.ctypes.data, res.ctypes.data, nb, nm, len(nm), iv.ctypes.data, n, biv.ctypes.data, exclude,
                                 buf.ctypes.data, cap, out.ctypes.data)
        assert rc == 0, rc
        assert (buf[int(out[0]):] == 0xEE).all(), "bytes written outside the text"
        assert int(out[4]) == int((iv[:, 1].astype(np.int64) - iv[:, 0] + 2).sum())        # memory follows the set
        text.append(buf[:int(out[0])].tobytes()); lines += int(out[1]); kept += int(out[2]); words += int(out[4])
    return b"".join(text), lines, kept, words


def selfcheck(L):
    """A small mixed dataset and the ramp through every pass: what the AddressSanitizer child of tests/test_targets.py runs."""
    for make, kw in ((dm.ramp, {}), (dm.mixed, dict(seed=3, block_reads=64, n=400))):
        fa, sam, pb, contigs = make(**kw)
        ivm = dm.assert_models_agree(pb, sam)
        names, lens = dm.names_lens(None, contigs)
        recs = rm.records(pb)
        flags = [x[3] for x in ivm]
        plan = host.UnpackPlan(rm.container(pb), fa)
        rng = np.random.default_rng(9)
        ivs = []
        for _ in range(150):
            c = int(rng.integers(0, len(lens)))
            b = int(rng.integers(1, lens[c] + 1))
            ivs.append((c, b, min(lens[c], b + int(rng.choice([0, 1, 40, 300])))))
        merged = merge(ivs)
        ts = plan.targets(region_strings(ivs[:70], names), bed(ivs[70:], names))
        assert ts.intervals() == merged
        dec = emu_decode_all(L, plan, ts.smax)
        for n_waves in (1, 4):
            rc, t, k, _ = emu_text(L, plan, dec, ts, 0, n_waves)
            assert rc == 0 and t == expected_reads(recs, merged)
            rc, t, k, _ = emu_text(L, plan, dec, ts, 1, n_waves)
            assert rc == 0 and t == expected_sam(recs, flags, names, merged)
        for ex in (0, 16):
            t, lines, kept, _ = emu_depth(L, plan, dec, ts, ex)
            assert (t, lines) == expected_depth(ivm, names, lens, merged, ex), (make.__name__, ex)
        plan.close(); pb.close()
    return True
