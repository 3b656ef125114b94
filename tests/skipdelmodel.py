"""Deletion-aware coverage in plain Python: what `--skip-deletions` must make of `cbc -x --depth`,
`--bedcov` and `--depth-hist`.  The depth at a position is the kept reads with an ALIGNED base there.  Two independent models of
it -- (a) the codec's view: the span depth of depthmodel.depth_array over the packer's arrays, less the deleted bases that the
mapping of pileupmodel.reads_a places (POS + dc[d] + d, inside the span); (b) POS + CIGAR of the SAM text that was compressed:
M, = and X count, D does not -- which must agree before either is used.  Everything behind the depth array is the EXISTING
models (depthmodel.bedgraph, covmodel, covxmodel, quantmodel, histmodel) fed with it through `Depth`.  Also the datasets the CPU
and the GPU tests share and the ctypes wrapper of the emulation library (tests/skipdel_emu)."""
import ctypes
import re

import numpy as np

import blockref
import depthmodel as dm
import pileupmodel as pm
import regionmodel as rm
import synth
from cbc_amd import host

_CIGAR = re.compile(rb"(\d+)([MIDNSHP=X])")


# ---- model (a): the packed arrays ----------------------------------------------------------------------------------------------
def intervals(reads):
    """pileupmodel.reads_a -> the tuples depthmodel.depth_array and covxmodel.Reads take: the SPAN intervals."""
    return [(r["contig"], r["pos"], r["span"], r["flag"], r["block"]) for r in reads]


def deleted(rd):
    """The reference positions read `rd` deletes, inside its span: POS + dc[d] + d."""
    off = rd["dc"] + np.arange(len(rd["dc"]), dtype=np.int64)
    return rd["pos"] + off[off < rd["span"]]


def depth_a(reads, contig, beg, end, exclude=0, skip_blocks=()):
    """(depth of positions beg..end as int64, reads kept, deleted bases taken off): the span depth less the kept reads'
    deleted bases inside the window.  Kept is the span rule of depthmodel.depth_array."""
    d, kept = dm.depth_array(intervals(reads), contig, beg, end, exclude, skip_blocks)
    d = d.copy()
    off = 0
    for r in reads:
        if r["contig"] != contig or r["span"] < 1 or r["flag"] & exclude or r["pos"] > end or r["pos"] + r["span"] - 1 < beg or r["block"] in skip_blocks:
            continue
        p = deleted(r)
        p = p[(p >= beg) & (p <= end)]
        np.subtract.at(d, p - beg, 1)
        off += len(p)
    assert (d >= 0).all()
    return d, kept, off


# ---- model (b): the SAM text ---------------------------------------------------------------------------------------------------
def depth_b(sam: bytes, names, contig, beg, end, exclude=0):
    """The same from POS and CIGAR alone: M, = and X cover, D and N do not; a read is kept when its reference interval (M D N = X)
    overlaps the window."""
    W = end - beg + 1
    diff = np.zeros(W + 1, dtype=np.int64)
    kept = 0
    for ln in sam.split(b"\n"):
        if not ln or ln.startswith(b"@"):
            continue
        c = ln.split(b"\t")
        if int(c[1]) & 4 or names.index(c[2]) != contig or int(c[1]) & exclude:
            continue
        pos = rp = int(c[3])
        pieces = []
        for n, op in _CIGAR.findall(c[5]):
            n = int(n)
            if op in b"M=X":
                pieces.append((rp, rp + n - 1)); rp += n
            elif op in b"DN":
                rp += n
        if rp == pos or pos > end or rp - 1 < beg:
            continue
        kept += 1
        for a, b in pieces:
            if a <= end and b >= beg:
                diff[max(a, beg) - beg] += 1
                diff[min(b, end) + 1 - beg] -= 1
    return np.cumsum(diff[:W]), kept


def assert_models_agree(pb, sam, names, lens):
    """On input without soft clips (and without reads whose edits cancel) the two models give the same depth and the same kept
    reads on every contig, with and without an exclude mask -- behind pileupmodel.assert_models_agree, which compares the reads one
    by one.  A dataset where they do not is the wrong dataset for a test that lets either stand as ground truth.  Returns model
    (a)'s reads."""
    reads = pm.assert_models_agree(pb, sam, names, lens)
    for c in range(len(names)):
        for ex in (0, 16):
            da, ka, _ = depth_a(reads, c, 1, lens[c], ex)
            db, kb = depth_b(sam, names, c, 1, lens[c], ex)
            assert ka == kb and np.array_equal(da, db), "the depths of the two models differ on contig %d" % c
    return reads


class Depth:
    """covmodel.Depth's interface (contig(c) -> the per-base depth of the whole contig) over model (a): what covmodel, covxmodel,
    quantmodel and histmodel take as their `depth`."""

    def __init__(self, reads, lens, exclude=0, skip_blocks=()):
        self.reads, self.lens, self.exclude, self.skip = reads, lens, exclude, tuple(skip_blocks)
        self._d = {}

    def contig(self, c):
        if c not in self._d:
            self._d[c] = depth_a(self.reads, c, 1, self.lens[c], self.exclude, self.skip)[0]
        return self._d[c]


def expected(reads, names, lens, region=None, exclude=0, skip_blocks=()):
    """bedGraph of the whole container (every contig in table order) or of region = (contig, beg, end), by depthmodel.bedgraph.
    Returns (bytes, runs, reads kept)."""
    calls = [region] if region is not None else [(c, 1, lens[c]) for c in range(len(names))]
    out, runs, kept = [], 0, 0
    for c, beg, end in calls:
        d, k, _ = depth_a(reads, c, beg, end, exclude, skip_blocks)
        t, r = dm.bedgraph(names[c], beg, d)
        out.append(t); runs += r; kept += k
    return b"".join(out), runs, kept


def expected_targets(reads, names, lens, merged, exclude=0, skip_blocks=()):
    """bedGraph restricted to the merged intervals [(contig, beg, end)] in order: per interval what `expected` gives for it as a
    region.  Returns (bytes, runs)."""
    out, runs = [], 0
    full = Depth(reads, lens, exclude, skip_blocks)
    for c, beg, end in merged:
        t, r = dm.bedgraph(names[c], beg, full.contig(c)[beg - 1:end])
        out.append(t); runs += r
    return b"".join(out), runs


# ---- datasets ------------------------------------------------------------------------------------------------------------------
def read(contig, pos, ops, flag=0):
    """A read at `pos` (1-based) that follows the reference through `ops` = [("M", n) | ("D", n), ...], starting and ending in M."""
    p, seq, md, run, nm = pos - 1, [], [], 0, 0
    for op, n in ops:
        if op == "M":
            seq.append(contig[p:p + n].tobytes()); run += n
        else:
            md.append("%d^%s" % (run, contig[p:p + n].tobytes().decode())); run = 0; nm += n
        p += n
    md.append(str(run))
    return dict(pos=pos, flag=flag, cigar="".join("%d%s" % (n, op) for op, n in ops), seq=b"".join(seq), md="".join(md), nm=nm)


def open_reads(contigs, recs_by_contig, block_reads=64):
    """[(name, contig)], [[record dicts in POS order] per contig] -> the dict the tests work on: texts, packed batch, container,
    plan, names, lens and the reads of model (a), the two models checked against each other."""
    fa = synth.fasta_text(contigs)
    sam = synth.sam_text([(n, len(c), r) for (n, c), r in zip(contigs, recs_by_contig)])
    return open_packed(fa, sam, host.pack_sam(sam, fa, block_reads=block_reads, var_length=True), contigs)


def open_packed(fa, sam, pb, contigs):
    blob = rm.container(pb)
    names, lens = dm.names_lens(None, contigs)
    reads = assert_models_agree(pb, sam, names, lens)
    return dict(fa=fa, sam=sam, pb=pb, blob=blob, plan=host.UnpackPlan(blob, fa), names=names, lens=lens, reads=reads)


def close(d):
    d["plan"].close(); d["pb"].close()


def one_read():
    """Case 1: one read with one deletion in its middle, alone on its contig (a second contig holds one plain read)."""
    rng = np.random.default_rng(31)
    c, c2 = synth.make_contig(rng, 1000), synth.make_contig(rng, 600)
    return open_reads([("solo", c), ("other", c2)], [[read(c, 101, [("M", 40), ("D", 3), ("M", 40)])], [read(c2, 200, [("M", 90)])]])


def apart(n=64, runs=3):
    """Case 2: n reads that do not overlap, `runs` separate deletion runs each: 2 + 2 * runs change points per read."""
    c = synth.make_contig(np.random.default_rng(32), 200 * n + 400)
    ops = [("M", 20)]
    for k in range(runs):
        ops += [("D", 1 + k), ("M", 20)]
    return open_reads([("apart", c)], [[read(c, 50 + 200 * i, ops) for i in range(n)]])


def cancel():
    """Case 3: two reads deleting the same positions; a deletion of 2 bases next to one of 1 base of another read; a run of 70
    deleted bases; a block of 65 reads with the deletion in read 64 (block_reads = 65: the first block holds them all)."""
    c = synth.make_contig(np.random.default_rng(33), 9000)
    recs = [read(c, 100, [("M", 50), ("D", 4), ("M", 50)]), read(c, 110, [("M", 40), ("D", 4), ("M", 50)]),     # 150..153 twice
            read(c, 400, [("M", 50), ("D", 2), ("M", 50)]), read(c, 410, [("M", 42), ("D", 1), ("M", 50)]),     # 450, 451 | 452
            read(c, 700, [("M", 60), ("D", 70), ("M", 60)])]
    recs += [read(c, 1000 + 20 * i, [("M", 100)]) for i in range(59)]
    recs.append(read(c, 2300, [("M", 30), ("D", 5), ("M", 70)]))                                              # read 64 of block 0
    recs += [read(c, 2500 + 30 * i, [("M", 50), ("D", 1), ("M", 49)] if i % 7 == 0 else [("M", 100)]) for i in range(60)]
    return open_reads([("cancel", c)], [recs], block_reads=65)


def edges():
    """Case 4: deletions for the windows and intervals of the tests to cut: one across positions 4090..4101 (a window from 1 puts
    the tile boundary, index 4096, inside it), one at 6000..6009, reads around them, a second contig."""
    rng = np.random.default_rng(34)
    c, c2 = synth.make_contig(rng, 12000), synth.make_contig(rng, 3000)
    recs = [read(c, 3990 + 10 * i, [("M", 100)]) for i in range(5)]
    recs += [read(c, 4040, [("M", 50), ("D", 12), ("M", 50)]), read(c, 4050, [("M", 100)]), read(c, 4095, [("M", 100)])]
    recs += [read(c, 5950, [("M", 50), ("D", 10), ("M", 50)]), read(c, 5960, [("M", 100)]), read(c, 5990, [("M", 30), ("D", 2), ("M", 60)])]
    recs += [read(c, 8000 + 25 * i, [("M", 40), ("D", 3), ("M", 60)] if i % 3 == 0 else [("M", 100)], flag=16 * (i % 2)) for i in range(70)]
    r2 = [read(c2, 100 + 15 * i, [("M", 30), ("D", 6), ("M", 64)] if i % 4 == 1 else [("M", 100)]) for i in range(80)]
    return open_reads([("edgeA", c), ("edgeB", c2)], [recs, r2])


def shared():
    """Case 6: pileupmodel.shared(), the synth.shared_variant_dataset with indel_sites = 8 -- shared variant sites and errors.  As
    synth.py stands the dataset holds NO indel whatever indel_sites says, so the identities are also checked on mixed()."""
    fa, sam, pb, contigs = pm.shared()
    return open_packed(fa, sam, pb, contigs)


def mixed(n=600):
    """Case 6 on reads that do delete: depthmodel.mixed -- three contigs, read lengths 100 and 150, indels in 30 % of the reads,
    both strands, the 40-base deletion read whose span reaches into the next block."""
    fa, sam, pb, contigs = dm.mixed(7, 64, n=n)
    return open_packed(fa, sam, pb, contigs)


# ---- the emulation library -----------------------------------------------------------------------------------------------------
def emu_load(path):
    L = ctypes.CDLL(path)
    V, U32, U64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    L.emu_skipdel_decode.restype = ctypes.c_int
    L.emu_skipdel_decode.argtypes = [V, U32, U32, V, V]
    L.emu_skipdel_cp_cap.restype = U64
    L.emu_skipdel_cp_cap.argtypes = [U64, U64, U32, U32]
    L.emu_skipdel.restype = ctypes.c_int
    L.emu_skipdel.argtypes = [V, U64, V, U64, V, V, V, U32, V, V, U32, ctypes.c_char_p, U32, U64, U64, V, U32, V, U32, U32, V, U64, V, V]
    return L


def emu_decode_all(L, plan, smax, per_read=16, check=True):
    """Every block of the plan, in the plan's own layout, by the emulated edit-reporting decoder; side array and arena at exactly
    their sizes.  A window's or a target set's blocks are gathered from it."""
    bl = plan.blocks.copy()
    nrec = int(bl["n_reads"].sum())
    pay = np.concatenate([np.ascontiguousarray(plan.payloads), np.zeros(16, dtype=np.uint8)])
    recs = np.zeros(max(nrec, 1), dtype=host.REC_DTYPE)
    seq = np.zeros(nrec * plan.seq_stride + 40, dtype=np.uint8)
    res = np.zeros(plan.n_blocks, dtype=host.RESULT_DTYPE)
    vs = np.zeros(max(plan.n_blocks * plan.cap_var, 1), dtype=np.uint32)
    side = np.zeros((max(nrec, 1), 2), dtype=np.uint32)
    arena = np.full(max(nrec * per_read, 1), 0xEEEE, dtype=np.uint16)
    db = blockref.DecDeviceBatch(pay.ctypes.data, pay.size, bl.ctypes.data, plan.n_blocks, plan.ref.ctypes.data, len(plan.ref),
                                 recs.ctypes.data, nrec, seq.ctypes.data, seq.size, res.ctypes.data, vs.ctypes.data, vs.size,
                                 host.LdsCaps(plan.cap_pos, plan.cap_var))
    assert L.emu_skipdel_decode(ctypes.byref(db), smax, per_read, side.ctypes.data, arena.ctypes.data) == 0
    assert not check or (res["status"] == 0).all()
    return dict(bl=bl, recs=recs, seq=seq, res=res, nrec=nrec, side=side, arena=arena, per_read=per_read)


def _name(plan, c):
    off = int(plan.contig_name_off[c])
    return plan.names[off:].tobytes().split(b"\0", 1)[0]


def _call(L, plan, dec, blocks, contig, beg, end, iv, biv, exclude, skip, cap, fail_blocks, n_waves):
    """One emu_skipdel over the blocks `blocks` (indices into the plan).  Returns dict(rc, text, lines, kept, total, points =
    [(position or slot, depth)], words, bound)."""
    sel = np.ascontiguousarray(blocks).astype(np.int64)
    bl = np.ascontiguousarray(dec["bl"][sel])
    ws = np.ascontiguousarray(plan.window_start[sel], dtype=np.uint64)
    res = dec["res"][sel].copy()
    for b in fail_blocks:
        res[b]["status"] = 2
    n_iv = 0 if iv is None else len(iv)
    per_read = dec["per_read"] if skip else 0
    d_words = end - beg + 2 if iv is None else int((iv[:, 1].astype(np.int64) - iv[:, 0] + 2).sum())
    bound = int(L.emu_skipdel_cp_cap(d_words, dec["nrec"], n_iv, per_read))
    text = np.full(cap + 16, 0xEE, dtype=np.uint8)
    cp = np.full((bound + 1, 2), 0xEEEEEEEE, dtype=np.uint32)
    out = np.zeros(6, dtype=np.uint64)
    name = _name(plan, contig)
    rc = L.emu_skipdel(dec["recs"].ctypes.data, dec["nrec"], dec["seq"].ctypes.data, dec["seq"].size, bl.ctypes.data, ws.ctypes.data,
                       res.ctypes.data, len(sel), dec["side"].ctypes.data, dec["arena"].ctypes.data, per_read, name, len(name), beg, end,
                       None if iv is None else iv.ctypes.data, n_iv, None if biv is None else biv.ctypes.data, exclude, n_waves,
                       text.ctypes.data, cap, cp.ctypes.data, out.ctypes.data)
    total, wrote = int(out[0]), rc in (0, -4)
    assert (text[total if wrote else 0:] == 0xEE).all(), "bytes written outside the text"
    assert int(out[5]) == bound and int(out[3]) <= bound and (cp[int(out[3]):] == 0xEEEEEEEE).all()
    return dict(rc=rc, text=text[:total].tobytes() if wrote else b"", lines=int(out[1]), kept=int(out[2]), total=total,
                points=[tuple(x) for x in cp[:int(out[3])].tolist()], words=int(out[4]), bound=bound)


def emu_window(L, plan, dec, sel, exclude=0, skip=True, cap=None, fail_blocks=(), n_waves=4):
    """One cbc_gpu_decode_depth on the emulation over the selection `sel` (plan.region / plan.contig_blocks)."""
    if sel.b1 == sel.b0:
        return dict(rc=0, text=b"", lines=0, kept=0, total=0, points=[], words=0, bound=0)
    if cap is None:
        cap = plan.depth_skipdel_text_cap(sel.b0, sel.b1, sel.contig, sel.beg, sel.end, sel.smax) if skip else plan.depth_text_cap(sel.b0, sel.b1, sel.contig)
    return _call(L, plan, dec, np.arange(sel.b0, sel.b1), sel.contig, sel.beg, sel.end, None, None, exclude, skip, cap, fail_blocks, n_waves)


def emu_whole(L, plan, dec, exclude=0, skip=True):
    """Every contig that has blocks, in table order, texts appended: what `cbc -x --depth [--skip-deletions]` does."""
    text, runs, kept = [], 0, 0
    for c in range(plan.n_contigs):
        r = emu_window(L, plan, dec, plan.contig_blocks(c), exclude, skip)
        assert r["rc"] == 0
        text.append(r["text"]); runs += r["lines"]; kept += r["kept"]
    return b"".join(text), runs, kept


def emu_targets(L, plan, dec, ts, exclude=0, skip=True, fail_blocks=(), n_waves=4):
    """The depth calls of cbc_gpu_decode_targets on the emulation, one per contig with intervals and blocks, texts appended.
    Returns (text, lines, reads kept, [the calls' results])."""
    text, lines, kept, calls = [], 0, 0, []
    for c in range(ts.n_contigs):
        k0, nb = int(ts.contig_blk_first[c]), int(ts.contig_blk_count[c])
        if not nb:
            continue
        f, n = int(ts.contig_first[c]), int(ts.contig_count[c])
        iv = np.ascontiguousarray(ts.iv[f:f + n], dtype=np.uint32)
        biv = np.ascontiguousarray(ts.block_iv[k0:k0 + nb], dtype=np.uint32).copy()
        biv[:, 0] -= np.uint32(f)
        cap = ts.depth_skipdel_cap[c] if skip else ts.depth_cap[c]
        r = _call(L, plan, dec, ts.blocks[k0:k0 + nb], c, 1, 1, iv, biv, exclude, skip, cap, [b - k0 for b in fail_blocks if k0 <= b < k0 + nb], n_waves)
        assert r["rc"] in (0, -4), r["rc"]
        assert r["words"] == int((iv[:, 1].astype(np.int64) - iv[:, 0] + 2).sum())
        text.append(r["text"]); lines += r["lines"]; kept += r["kept"]; calls.append(r)
    return b"".join(text), lines, kept, calls


def points_of(depth):
    """The change points of a depth array laid from index 0 with depth 0 in front and behind: [(index, depth from there on)]."""
    d = np.concatenate([depth, [0]])
    cut = np.flatnonzero(np.diff(d, prepend=0))
    return [(int(i), int(d[i])) for i in cut.tolist()]
