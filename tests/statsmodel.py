"""Read statistics in plain Python: what `cbc -x --stats` must write.  Brute force and nothing new as
ground truth: the reads are (FLAG, SEQ) pairs derived twice -- from the SAM text the dataset was packed from and from the packer's
`recs` and `seq` -- and the two lists must agree before either is used (assert_models_agree); the tables are numpy counts over a
padded byte matrix, the text is restated with Python integers.  Also the selection rule of a target set, the fabricated dataset
of the smallest shapes at which the kernel can go wrong, and the ctypes wrapper of the emulation library (tests/stats_emu)."""
import ctypes

import numpy as np

import depthmodel as dm
import synth
from cbc_amd import host

FS_NAMES = [b"total", b"primary", b"secondary", b"supplementary", b"duplicates", b"primary duplicates", b"mapped", b"primary mapped",
            b"paired in sequencing", b"read1", b"read2", b"properly paired", b"with itself and mate mapped", b"singletons",
            b"reverse strand"]
_COMP = np.arange(256, dtype=np.uint8)
for _a, _b in (b"AT", b"CG"):
    _COMP[_a], _COMP[_b] = _b, _a


# ---- the reads, twice ----------------------------------------------------------------------------------------------------------
def reads_from_sam(sam: bytes):
    """(FLAG, SEQ) of every mapped alignment line, in file order."""
    out = []
    for ln in sam.split(b"\n"):
        if not ln or ln.startswith(b"@"):
            continue
        c = ln.split(b"\t")
        if not int(c[1]) & 4:
            out.append((int(c[1]), c[9]))
    return out


def reads_from_packed(pb):
    """(FLAG, SEQ) of every record of the packer's arrays, in container order."""
    out = []
    for b in range(pb.n_blocks):
        bd = pb.blocks[b]
        for k in range(int(bd["n_reads"])):
            r = pb.recs[int(bd["rec_base"]) + k]
            s0 = int(bd["seq_base"]) + int(r["seq_off"])
            out.append((int(r["flag"]), pb.seq[s0:s0 + int(r["rlen"])].tobytes()))
    return out


def assert_models_agree(pb, sam):
    a, b = reads_from_packed(pb), reads_from_sam(sam)
    assert len(a) == len(b)
    bad = [(i, x, y) for i, (x, y) in enumerate(zip(a, b)) if x != y]
    assert not bad, "the packer's reads and the SAM text differ on %d reads, first: %r" % (len(bad), bad[0])
    return a


def packed_arrays(pb):
    """(flags, lengths, byte matrix padded with 0) straight from the packer's arrays, vectorised (the mid-size panel)."""
    blk = np.repeat(np.arange(pb.n_blocks), pb.blocks["n_reads"].astype(np.int64))
    off = pb.blocks["seq_base"].astype(np.int64)[blk] + pb.recs["seq_off"].astype(np.int64)
    lens = pb.recs["rlen"].astype(np.int64)
    w = int(lens.max()) if len(lens) else 0
    col = np.arange(w)
    idx = np.minimum(off[:, None] + col[None, :], len(pb.seq) - 1)
    m = np.where(col[None, :] < lens[:, None], pb.seq[idx], 0).astype(np.uint8)
    return pb.recs["flag"].astype(np.int64), lens, m


def arrays(reads):
    flags = np.array([f for f, _ in reads], dtype=np.int64)
    lens = np.array([len(s) for _, s in reads], dtype=np.int64)
    m = np.zeros((len(reads), int(lens.max()) if len(reads) else 0), dtype=np.uint8)
    for i, (_, s) in enumerate(reads):
        m[i, :len(s)] = np.frombuffer(s, dtype=np.uint8)
    return flags, lens, m


# ---- the tables ------------------------------------------------------------------------------------------------------------------
def tables(reads, exclude=0, keep=None):
    """reads: [(FLAG, SEQ)] or (flags, lengths, matrix); keep: a boolean array, the selection (None: all)."""
    flags, lens, m = arrays(reads) if isinstance(reads, list) else reads
    if keep is not None:
        flags, lens, m = flags[keep], lens[keep], m[keep]
    ex = (flags & exclude) != 0
    out = dict(excluded=int(ex.sum()))
    flags, lens, m = flags[~ex], lens[~ex], m[~ex]
    n, w = m.shape
    assert w <= 256
    out["reads"] = n
    out["flag"] = np.bincount(flags, minlength=65536).astype(np.uint32)
    out["len"] = np.bincount(lens, minlength=257).astype(np.uint32)
    col = np.arange(w)
    valid = col[None, :] < lens[:, None]
    rev = (flags & 16) != 0
    src = np.where(rev[:, None], lens[:, None] - 1 - col[None, :], col[None, :])
    byt = np.take_along_axis(m, np.clip(src, 0, max(w - 1, 0)), axis=1) if w else m
    byt = np.where(rev[:, None], _COMP[byt], byt)
    cyc = np.zeros((5, 256), dtype=np.uint32)
    for k, ch in enumerate(b"ACGT"):
        cyc[k, :w] = (valid & (byt == ch)).sum(axis=0)
    cyc[4, :w] = valid.sum(axis=0) - cyc[:4, :w].sum(axis=0)
    out["cyc"] = cyc
    gcn = (((m == ord("G")) | (m == ord("C"))) & valid).sum(axis=1)
    has = lens >= 1
    out["gc"] = np.bincount((100 * gcn[has]) // lens[has], minlength=101).astype(np.uint32)
    return out


def zero_tables():
    return dict(reads=0, excluded=0, flag=np.zeros(65536, np.uint32), len=np.zeros(257, np.uint32), gc=np.zeros(101, np.uint32),
                cyc=np.zeros((5, 256), np.uint32))


def same(a, b):
    return (a["reads"] == b["reads"] and a["excluded"] == b["excluded"]
            and all(np.array_equal(np.asarray(a[k]).reshape(-1), np.asarray(b[k]).reshape(-1)) for k in ("flag", "len", "gc", "cyc")))


def diff(a, b):
    """Where two sets of tables differ (for an assertion's message)."""
    out = [(k, a[k], b[k]) for k in ("reads", "excluded") if a[k] != b[k]]
    for k in ("flag", "len", "gc", "cyc"):
        x, y = np.asarray(a[k]).reshape(-1).astype(np.int64), np.asarray(b[k]).reshape(-1).astype(np.int64)
        w = np.nonzero(x != y)[0][:4]
        out += [(k, int(i), int(x[i]), int(y[i])) for i in w]
    return out


def selected(iv, given):
    """iv: depthmodel.intervals_a (contig, POS, span, FLAG, block) per read; given: [(contig, beg, end)].  The reads
    cbc_gpu_decode_targets keeps: those that overlap at least one interval."""
    keep = np.zeros(len(iv), dtype=bool)
    for i, x in enumerate(iv):
        keep[i] = any(x[0] == c and x[1] <= e and x[1] + x[2] - 1 >= b for c, b, e in given)
    return keep


# ---- the text --------------------------------------------------------------------------------------------------------------------
def mean(total, n):
    """The integer rule of cbc_coverage_mean: two decimals, rounded half up."""
    if n == 0:
        return b"0.00"
    m = (total // n) * 100 + ((total % n) * 100 + n // 2) // n
    return b"%d.%02d" % (m // 100, m % 100)


def text(t):
    flag, ln, gc, cyc = (np.asarray(t[k]).astype(np.int64) for k in ("flag", "len", "gc", "cyc"))
    cyc = cyc.reshape(5, 256)
    occ = np.nonzero(ln)[0]
    bases = int((np.arange(257) * ln).sum())
    assert bases == int(cyc.sum()) and int(ln.sum()) == t["reads"] == int(flag.sum())
    out = [b"SN\treads\t%d\n" % t["reads"], b"SN\treads excluded\t%d\n" % t["excluded"], b"SN\tbases\t%d\n" % bases,
           b"SN\tminimum length\t%d\n" % (int(occ[0]) if len(occ) else 0), b"SN\tmaximum length\t%d\n" % (int(occ[-1]) if len(occ) else 0),
           b"SN\taverage length\t%s\n" % mean(bases, t["reads"])]
    out += [b"SN\tbases %s\t%d\n" % (nm, int(cyc[k].sum())) for k, nm in enumerate([b"A", b"C", b"G", b"T", b"other"])]
    fs = [[0, 0] for _ in FS_NAMES]
    for f in np.nonzero(flag)[0].tolist():
        n = int(flag[f])
        sec = bool(f & 0x100)
        sup = not sec and bool(f & 0x800)
        pri = not sec and not sup
        mapped, pair = not f & 4, pri and bool(f & 1)
        member = [True, pri, sec, sup, bool(f & 0x400), pri and bool(f & 0x400), mapped, pri and mapped, pair, pair and bool(f & 0x40),
                  pair and bool(f & 0x80), pair and bool(f & 2) and mapped, pair and mapped and not f & 8, pair and mapped and bool(f & 8),
                  bool(f & 16)]
        for k, inside in enumerate(member):
            if inside:
                fs[k][1 if f & 0x200 else 0] += n
    out += [b"FS\t%s\t%d\t%d\n" % (nm, fs[k][0], fs[k][1]) for k, nm in enumerate(FS_NAMES)]
    out += [b"FL\t%d\t%d\n" % (f, flag[f]) for f in np.nonzero(flag)[0].tolist()]
    out += [b"RL\t%d\t%d\n" % (x, ln[x]) for x in occ.tolist()]
    out += [b"GC\t%d\t%d\n" % (p, gc[p]) for p in np.nonzero(gc)[0].tolist()]
    out += [b"BC\t%d\t%d\t%d\t%d\t%d\t%d\n" % ((c + 1,) + tuple(int(cyc[k, c]) for k in range(5))) for c in range(int(occ[-1]) if len(occ) else 0)]
    return b"".join(out)


# ---- the fabricated dataset ------------------------------------------------------------------------------------------------------
LENGTHS = (1, 3, 4, 5, 63, 64, 65, 150, 251, 252)
FLAGS = (0, 16, 99, 147, 1024, 2048 + 16, 256, 512 + 83, 4095 & ~4, 4096 + 16, 4096 + 2048 + 1)     # the last: above the LDS bound


def shapes(block_reads=64, seed=41):
    """Every length of LENGTHS once forward and once with FLAG 16; reads with N at the first base, at the last base and in the
    dword that straddles the length; an all-G and an all-A read (on homopolymer stretches of the contig); every FLAG of FLAGS;
    then 64 reads that carry one FLAG, placed so that they fill one block; a few hundred reads in all, on two contigs.
    Returns (fasta, sam, packed batch, contigs, first read of the one-FLAG block)."""
    rng = np.random.default_rng(seed)
    c1, c2 = synth.make_contig(rng, 9000), synth.make_contig(rng, 3000)
    c1[3000:3300] = ord("G")
    c1[3400:3700] = ord("A")

    def rd(c, p, L, flag, n_at=()):
        seq = bytearray(c[p - 1:p - 1 + L].tobytes())
        for i in n_at:
            seq[i] = ord("N")
        md, nm = synth._md_and_nm(c, p - 1, [("M", L)], bytes(seq))
        return dict(pos=p, flag=flag, cigar="%dM" % L, seq=bytes(seq), md=md, nm=nm)
    r1, p = [], 10
    for L in LENGTHS:
        for f in (0, 16):
            r1.append(rd(c1, p, L, f)); p += 7
    for L in (5, 64, 150, 251):                            # N first, last, and in the last (partial or full) dword; both strands
        for f in (0, 16):
            r1.append(rd(c1, p, L, f, (0,))); p += 3
            r1.append(rd(c1, p, L, f, (L - 1,))); p += 3
            r1.append(rd(c1, p, L, f, (L - 1 - (L - 1) % 4,))); p += 3
            r1.append(rd(c1, p, L, f, (0, L // 2, L - 1))); p += 3
    for i, f in enumerate(FLAGS * 3):
        r1.append(rd(c1, p, 100 + (i % 3), f)); p += 5
    while len(r1) % block_reads:                             # fill the block, so that the next one starts at the one-FLAG reads
        r1.append(rd(c1, p, 100, 16 * (len(r1) & 1))); p += 2
    same_at = len(r1)
    r1 += [rd(c1, p + i, 100, 83) for i in range(64)]
    p += 64
    for f in (0, 16, 1024, 1040):                            # the homopolymer stretches: GC 100 and GC 0
        r1.append(rd(c1, 3001 + (f & 15), 150, f))
        r1.append(rd(c1, 3401 + (f & 15), 150, f))
    r1.sort(key=lambda r: r["pos"])                          # stable: the one-FLAG reads stay together, behind everything in front
    r2 = [rd(c2, 20 + 9 * i, LENGTHS[i % len(LENGTHS)], FLAGS[i % len(FLAGS)]) for i in range(90)]
    contigs = [("shpA", c1), ("shpB", c2)]
    fa, sam = synth.fasta_text(contigs), synth.sam_text([("shpA", len(c1), r1), ("shpB", len(c2), r2)])
    return fa, sam, host.pack_sam(sam, fa, block_reads=block_reads, var_length=True), contigs, same_at


# ---- the emulation library -------------------------------------------------------------------------------------------------------
def emu_load(path):
    L = ctypes.CDLL(path)
    V, U32, U64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    L.emu_stats_decode.restype = ctypes.c_int
    L.emu_stats_decode.argtypes = [V, U32]
    L.emu_targets_decode = L.emu_stats_decode                # targetsmodel.emu_decode_all drives the decoder under this name
    L.emu_stats.restype = ctypes.c_int
    L.emu_stats.argtypes = [V, U64, V, U64, V, V, V, U32, V, U32, V, U32, U32, U32, ctypes.POINTER(host.GpuStats)]
    L.emu_stats_lds_flags.restype = U32
    return L


def as_tables(st):
    return dict(reads=int(st.reads), excluded=int(st.excluded), flag=np.ctypeslib.as_array(st.flag).copy(),
                len=np.ctypeslib.as_array(st.len).copy(), gc=np.ctypeslib.as_array(st.gc).copy(),
                cyc=np.ctypeslib.as_array(st.cyc).copy().reshape(5, 256))


def emu_stats(L, plan, dec, ts=None, exclude=0, grid=0, n_waves=4, fail_blocks=()):
    """One cbc_gpu_decode_stats on the emulation.  dec: targetsmodel.emu_decode_all; ts: a host.TargetSet or None (every block).
    Returns (rc, tables)."""
    sel = np.arange(plan.n_blocks, dtype=np.int64) if ts is None else ts.blocks.astype(np.int64)
    st = host.GpuStats()
    if len(sel) == 0:
        return 0, as_tables(st)
    bl = np.ascontiguousarray(dec["bl"][sel])
    ws = np.ascontiguousarray(plan.window_start[sel], dtype=np.uint64)
    res = dec["res"][sel].copy()
    for b in fail_blocks:
        res[b]["status"] = 2
    iv = biv = None
    if ts is not None:
        iv, biv = np.ascontiguousarray(ts.iv, dtype=np.uint32), np.ascontiguousarray(ts.block_iv, dtype=np.uint32)
    rc = L.emu_stats(dec["recs"].ctypes.data, dec["nrec"], dec["seq"].ctypes.data, dec["seq"].size, bl.ctypes.data, ws.ctypes.data,
                     res.ctypes.data, len(sel), iv.ctypes.data if ts is not None else None, ts.n_iv if ts is not None else 0,
                     biv.ctypes.data if ts is not None else None, exclude, grid, n_waves, ctypes.byref(st))
    return rc, as_tables(st)
