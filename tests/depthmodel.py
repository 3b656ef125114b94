"""Coverage output in plain Python: what `cbc -x --depth` must write.  Two independent models of a
read's reference interval -- (a) the codec's view, from the packed arrays (regionmodel.records: POS and span), and (b) the SAM
text that was compressed (POS and the reference-consuming CIGAR operations) -- one difference-array / run-length routine that
turns intervals into bedGraph bytes, the datasets the CPU and the GPU tests share, and the ctypes wrapper of the emulation
library (tests/depth_emu)."""
import ctypes
import re

import numpy as np

import blockref
import regionmodel as rm
import synth
from cbc_amd import host

_CIGAR = re.compile(rb"(\d+)([MIDNSHP=X])")


# ---- the two models of the intervals ---------------------------------------------------------------------------------------
def intervals_a(pb):
    """Model (a): per record (contig, POS, span, FLAG, block) as the codec sees it, in container order."""
    recs = rm.records(pb)
    flags = [int(pb.recs[int(pb.blocks[b]["rec_base"]) + k]["flag"]) for b in range(pb.n_blocks) for k in range(int(pb.blocks[b]["n_reads"]))]
    assert len(flags) == len(recs)
    return [(c, pos, span, flags[i], b) for i, (b, c, pos, span, _) in enumerate(recs)]


def intervals_b(sam: bytes, names=None):
    """Model (b): per mapped alignment line (contig index, POS, reference bases of the CIGAR: M D N = X, FLAG).  The contig
    index is the place of RNAME in `names` (default: the @SQ lines in order; a container's table lists only contigs with reads)."""
    given, names, out = names is not None, list(names or []), []
    for ln in sam.split(b"\n"):
        if ln.startswith(b"@SQ") and not given:
            names.append(dict(x.split(b":", 1) for x in ln.split(b"\t")[1:])[b"SN"])
        if not ln or ln.startswith(b"@"):
            continue
        c = ln.split(b"\t")
        if int(c[1]) & 4:
            continue
        span = sum(int(n) for n, op in _CIGAR.findall(c[5]) if op in b"MDN=X")
        out.append((names.index(c[2]), int(c[3]), span, int(c[1])))
    return out


def assert_models_agree(pb, sam, names=None):
    """On input without soft clips (and without reads whose edits cancel) the two models give the same interval for EVERY
    read; a dataset where they do not is the wrong dataset for a test that lets either model stand as ground truth."""
    a, b = intervals_a(pb), intervals_b(sam, names)
    assert len(a) == len(b)
    bad = [(i, x, y) for i, (x, y) in enumerate(zip(a, b)) if x[:4] != y]
    assert not bad, "models (a) and (b) differ on %d reads, first: %r" % (len(bad), bad[0])
    return a


# ---- intervals -> bedGraph ---------------------------------------------------------------------------------------------------
def depth_array(iv, contig, beg, end, exclude=0, skip_blocks=()):
    """Depth of positions beg..end (1-based, inclusive) of `contig` as an int64 array, and the reads counted."""
    sel = [x for x in iv if x[0] == contig and x[2] >= 1 and not (x[3] & exclude) and x[1] <= end and x[1] + x[2] - 1 >= beg
           and (len(x) < 5 or x[4] not in skip_blocks)]
    W = end - beg + 1
    diff = np.zeros(W + 1, dtype=np.int64)
    if sel:
        pos = np.array([x[1] for x in sel], dtype=np.int64)
        span = np.array([x[2] for x in sel], dtype=np.int64)
        np.add.at(diff, np.maximum(pos, beg) - beg, 1)
        np.add.at(diff, np.minimum(pos + span - 1, end) + 1 - beg, -1)
    return np.cumsum(diff[:W]), len(sel)


def bedgraph(name: bytes, beg, depth):
    """One line per maximal run of equal non-zero depth: name, 0-based start, end (half-open), depth.  Returns (bytes, runs)."""
    W = len(depth)
    if W == 0:
        return b"", 0
    cut = np.flatnonzero(np.diff(depth, prepend=0))                          # where the depth changes: run starts
    ends = np.append(cut[1:], W)
    keep = depth[cut] != 0
    s, e, d = cut[keep] + (beg - 1), ends[keep] + (beg - 1), depth[cut][keep]
    return b"".join(b"%s\t%d\t%d\t%d\n" % (name, a, b, c) for a, b, c in zip(s.tolist(), e.tolist(), d.tolist())), int(keep.sum())


def expected(iv, names, lens, region=None, exclude=0, skip_blocks=()):
    """bedGraph of the whole container (every contig in table order) or of region = (contig, beg, end).
    Returns (bytes, runs, reads counted)."""
    calls = [region] if region is not None else [(c, 1, lens[c]) for c in range(len(names))]
    out, runs, kept = [], 0, 0
    for c, beg, end in calls:
        d, k = depth_array(iv, c, beg, end, exclude, skip_blocks)
        t, r = bedgraph(names[c], beg, d)
        out.append(t); runs += r; kept += k
    return b"".join(out), runs, kept


def parse(text: bytes):
    """[(name, start0, end0, depth)] of bedGraph text written by the code under test."""
    assert text == b"" or text.endswith(b"\n")
    out = []
    for ln in text.split(b"\n")[:-1]:
        c = ln.split(b"\t")
        assert len(c) == 4, ln
        out.append((c[0], int(c[1]), int(c[2]), int(c[3])))
    return out


# ---- datasets ------------------------------------------------------------------------------------------------------------------
def mixed(seed, block_reads, n=3000, **kw):
    """The dataset of tests/test_region.py and tests/test_sam.py: three contigs (the last 3000 bases of each free of reads),
    read lengths 100 and 150 mixed, indels, both strands, and the 40-base deletion read as the last read of block 0, whose span
    reaches into block 1.  No soft clips unless asked for through kw.  Returns (fasta, sam, packed batch, contigs)."""
    fa, rbc, contigs = rm.mixed_dataset(seed, [60_000, 45_000, 20_000], [n, n // 2, 400], sub_rate=0.004, indel_frac=0.3,
                                        gap_tail=3000, **kw)
    recs = rbc[0][2]
    recs[block_reads - 1] = rm.deletion_read(contigs[0][1], recs[block_reads - 1]["pos"])
    sam = synth.sam_text(rbc)
    return fa, sam, host.pack_sam(sam, fa, block_reads=block_reads, var_length=True), contigs


def ramp(seed=5, first=99_951, n=130, L=100, flags=(16, 1040), block_reads=64):
    """`n` perfect reads of L bases at first, first + 1, ...: the depth climbs 1, 2, ... L (through 9 -> 10 and 99 -> 100) while
    the run boundaries pass 99999 -> 100000, then falls again; a second contig holds two far-apart reads; FLAG alternates
    between `flags`.  Returns (fasta, sam, packed batch, contigs)."""
    rng = np.random.default_rng(seed)
    c1, c2 = synth.make_contig(rng, first + n + L + 500), synth.make_contig(rng, 5000)
    r1 = [dict(pos=first + i, flag=flags[i % len(flags)], cigar="%dM" % L, seq=c1[first + i - 1:first + i - 1 + L].tobytes(), md=str(L), nm=0)
          for i in range(n)]
    r2 = [dict(pos=p, flag=flags[0], cigar="%dM" % L, seq=c2[p - 1:p - 1 + L].tobytes(), md=str(L), nm=0) for p in (1, 4000)]
    contigs = [("rampA", c1), ("rampB", c2)]
    rbc = [("rampA", len(c1), r1), ("rampB", len(c2), r2)]
    fa, sam = synth.fasta_text(contigs), synth.sam_text(rbc)
    return fa, sam, host.pack_sam(sam, fa, block_reads=block_reads, var_length=True), contigs


def names_lens(pb_or_plan_names, contigs):
    return [n.encode() for n, _ in contigs], [len(c) for _, c in contigs]


def windows(pb, iv, block_reads, lens, n_random, seed):
    """(region string, contig, beg, end): random windows, the edge cases of test_region._regions, and windows cut through the
    deletion read (inside the deleted bases, on its last covered base, just past it)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_random):
        c = int(rng.integers(0, len(lens)))
        beg = int(rng.integers(1, lens[c] + 1))
        end = min(lens[c], beg + int(rng.choice([0, 1, 50, 300, 2000, 20000])))
        out.append((c, beg, end))
    for b in range(pb.n_blocks):                                             # windows that end / begin on a block's first POS
        c, f = int(pb.info[b]["contig"]), int(pb.info[b]["window_start"]) + 1
        out += [(c, max(1, f - 40), f), (c, f, min(lens[c], f + 10))]
    d = [x for x in iv if x[4] == 0][-1]                                     # the deletion read: 140 reference bases
    assert d[2] == 140 and len(out) > 0
    dp = d[1]
    out += [(0, dp + 60, dp + 80), (0, dp + 139, dp + 139), (0, dp + 140, dp + 150), (0, dp + 100, dp + 300), (0, dp - 5, dp + 139)]
    for c, L in enumerate(lens):
        out += [(c, 1, 1), (c, L, L), (c, 1, L), (c, L - 1500, L - 1000), (c, L // 2, L), (c, L // 2, L // 2)]
    return [("chr%d:%d-%d" % (c + 1, b, e), c, b, e) for c, b, e in out]


# ---- the emulation library -----------------------------------------------------------------------------------------------------
def emu_load(path):
    L = ctypes.CDLL(path)
    L.emu_depth_decode.restype = ctypes.c_int
    L.emu_depth_decode.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    L.emu_depth.restype = ctypes.c_int
    L.emu_depth.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                            ctypes.c_void_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64,
                            ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    return L


def emu_decode(L, plan, b0, b1, smax):
    """Blocks [b0, b1) laid out from 0 (as cbc_gpu_decode_depth does) and decoded by the emulated span decoder."""
    bl = plan.blocks[b0:b1].copy()
    stride = plan.seq_stride
    nrec = int(bl["n_reads"].sum())
    bl["rec_base"] = np.concatenate([[0], np.cumsum(bl["n_reads"])[:-1]]).astype(np.uint64)
    bl["seq_base"] = bl["rec_base"] * np.uint64(stride)
    pay = np.concatenate([np.ascontiguousarray(plan.payloads), np.zeros(16, dtype=np.uint8)])
    recs = np.zeros(max(nrec, 1), dtype=host.REC_DTYPE)
    seq = np.zeros(nrec * stride + 40, dtype=np.uint8)
    res = np.zeros(b1 - b0, dtype=host.RESULT_DTYPE)
    vs = np.zeros(max((b1 - b0) * plan.cap_var, 1), dtype=np.uint32)
    db = blockref.DecDeviceBatch(pay.ctypes.data, pay.size, bl.ctypes.data, b1 - b0, plan.ref.ctypes.data, len(plan.ref),
                                 recs.ctypes.data, nrec, seq.ctypes.data, seq.size, res.ctypes.data, vs.ctypes.data, vs.size,
                                 host.LdsCaps(plan.cap_pos, plan.cap_var))
    assert L.emu_depth_decode(ctypes.byref(db), smax) == 0
    assert (res["status"] == 0).all()
    return bl, recs, seq, res, nrec


def emu_call(L, plan, sel, exclude=0, cap=None, fail_blocks=(), dec=None, name=None):
    """One cbc_gpu_decode_depth on the emulation: span decode of the selection, then every pass.  Returns (rc, text, lines,
    reads kept, text bytes); the guard bytes behind the text (all of it when rc != 0) must be untouched.  fail_blocks: blocks
    of the selection whose decode status is set to a failure before the passes run."""
    if sel.b1 == sel.b0:
        return 0, b"", 0, 0, 0
    bl, recs, seq, res, nrec = dec if dec is not None else emu_decode(L, plan, sel.b0, sel.b1, sel.smax)
    res = res.copy()
    for b in fail_blocks:
        res[b]["status"] = 2
    ws = np.ascontiguousarray(plan.window_start[sel.b0:sel.b1], dtype=np.uint64)
    off = int(plan.contig_name_off[sel.contig])
    name = plan.names[off:].tobytes().split(b"\0", 1)[0] if name is None else name
    cap = plan.depth_text_cap(sel.b0, sel.b1, sel.contig) if cap is None else cap
    text = np.full(cap + 16, 0xEE, dtype=np.uint8)
    out = np.zeros(4, dtype=np.uint64)
    rc = L.emu_depth(recs.ctypes.data, nrec, seq.ctypes.data, seq.size, bl.ctypes.data, ws.ctypes.data, res.ctypes.data,
                     sel.b1 - sel.b0, name, len(name), sel.beg, sel.end, exclude, text.ctypes.data, cap, out.ctypes.data)
    total = int(out[0])
    assert (text[total if rc == 0 else 0:] == 0xEE).all(), "bytes written outside the text"
    return rc, (text[:total].tobytes() if rc == 0 else b""), int(out[1]), int(out[2]), total


def emu_whole(L, plan, exclude=0):
    """Every contig that has blocks, in table order, texts appended: what `cbc -x --depth` does."""
    text, runs, kept = [], 0, 0
    for c in range(plan.n_contigs):
        rc, t, r, k, _ = emu_call(L, plan, plan.contig_blocks(c), exclude)
        assert rc == 0
        text.append(t); runs += r; kept += k
    return b"".join(text), runs, kept


def selfcheck(L, block_reads=64):
    """The ramp dataset and a small mixed one through every pass, whole and by window, with and without an exclude mask:
    what the AddressSanitizer child of tests/test_depth.py runs."""
    for make, kw in ((ramp, {}), (mixed, dict(seed=3, block_reads=block_reads, n=400))):
        fa, sam, pb, contigs = make(**kw)
        iv = assert_models_agree(pb, sam)
        names, lens = names_lens(None, contigs)
        plan = host.UnpackPlan(rm.container(pb), fa)
        for ex in (0, 16, 1024):
            got = emu_whole(L, plan, ex)
            assert got == expected(iv, names, lens, None, ex), (make.__name__, ex)
        for c, L_ in enumerate(lens):
            for beg, end in ((1, 1), (L_, L_), (L_ // 3, L_ // 3 + 700), (max(1, L_ // 2 - 50), L_)):
                sel = plan.region(b"%s:%d-%d" % (names[c], beg, end))
                rc, t, r, k, _ = emu_call(L, plan, sel)
                assert rc == 0 and (t, r, k) == expected(iv, names, lens, (c, beg, end)), (make.__name__, c, beg, end)
        plan.close(); pb.close()
    return True
