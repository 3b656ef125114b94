"""The alignment tables of the read statistics in plain Python: what `cbc -x --stats --alignment` must
count.  Two independent models that must agree on every table of every dataset before either is used -- (a) the codec's view,
from the packed arrays through pileupmodel.reads_a (dc, oi) and the element order of cigarmodel.tags_a: per matched coordinate m
the inserted read indices in front of aligned base m, the deleted bases with dc = m, aligned base m; (b) SAM-with-CIGAR text
alone: FLAG, CIGAR, SEQ, MD and NM of every line, the mismatches placed by walking MD along the CIGAR.  (b) is applied to
cigarmodel.expected() here and to what decode_sam(cigar=True) returns on the device.  Then the text restated in Python
integers, the datasets, and the ctypes wrapper of the emulation library (tests/alnstats_emu)."""
import ctypes
import re

import numpy as np

import blockref
import cigarmodel as cm
import pileupmodel as pm
import synth
from cbc_amd import host

_CIGAR = re.compile(r"(\d+)([MIDS])")
_MD = re.compile(r"(\d+)|(\^[^0-9]+)|([^0-9^])")
TABLES = (("len", 257, np.uint32), ("mm", 257, np.uint32), ("unal", 257, np.uint32), ("ins_cyc", 257, np.uint32),
          ("del_cyc", 257, np.uint32), ("nm", 767, np.uint32), ("ins_len", 256, np.uint64), ("del_len", 256, np.uint64))


def zero_tables():
    t = dict(reads=0, invalid=0)
    for name, n, dt in TABLES:
        t[name] = np.zeros(n, dtype=dt)
    return t


def same(a, b):
    return a["reads"] == b["reads"] and a["invalid"] == b["invalid"] and all(
        np.array_equal(np.asarray(a[k]).astype(np.uint64), np.asarray(b[k]).astype(np.uint64)) for k, _, _ in TABLES)


def diff(a, b):
    out = [(k, a[k], b[k]) for k in ("reads", "invalid") if a[k] != b[k]]
    for k, _, _ in TABLES:
        x, y = np.asarray(a[k]).astype(np.int64), np.asarray(b[k]).astype(np.int64)
        out += [(k, int(i), int(x[i]), int(y[i])) for i in np.nonzero(x != y)[0][:4]]
    return out


def _cyc(q, rl, rev):
    return rl - q if rev else q + 1


# ---- model (a): the packed arrays ----------------------------------------------------------------------------------------------
def count_a(t, rd, ref):
    """One counted read of pileupmodel.reads_a into the tables; ref: the uploaded bytes of its contig."""
    seq, dc, oi, pos = rd["seq"], [int(x) for x in rd["dc"]], [int(x) for x in rd["oi"]], rd["pos"]
    rl, nd, ni, rev = len(seq), len(dc), len(oi), bool(rd["flag"] & 16)
    T = rl - ni
    bad = rl == 0 or nd > 255 or ni > 255 or ni > rl or any(d > T for d in dc) or any(a > b for a, b in zip(dc, dc[1:])) or \
        any(o >= rl for o in oi) or any(a >= b for a, b in zip(oi, oi[1:])) or pos - 1 + T + nd > len(ref)
    if bad:
        t["invalid"] += 1
        return
    ins = set(oi)
    el, q, di, x = [], 0, 0, pos - 1                    # the element order of cigarmodel.tags_a
    for m in range(T + 1):
        while q < rl and q in ins:
            el.append(("I", q, None)); q += 1
        while di < nd and dc[di] == m:
            el.append(("D", None, x)); x += 1; di += 1
        if m < T:
            el.append(("M", q, x)); q += 1; x += 1
    assert q == rl and di == nd
    t["reads"] += 1
    t["len"][rl] += 1
    n_al, seen, nm, i = T, 0, 0, 0
    while i < len(el):
        j = i
        while j < len(el) and el[j][0] == el[i][0]:
            j += 1
        op, n = el[i][0], j - i
        if op == "I":
            for _, qq, _ in el[i:j]:
                t["unal"][_cyc(qq, rl, rev)] += 1
            if seen != 0 and seen != n_al:              # an aligned base before it in the read, and one after it
                t["ins_len"][n] += 1; nm += n
                t["ins_cyc"][_cyc(el[j - 1][1] if rev else el[i][1], rl, rev)] += 1
        elif op == "D":
            k = el[j][1] if j < len(el) else rl         # the aligned base behind the run; rl at T
            t["del_len"][n] += 1; nm += n
            t["del_cyc"][rl - k if rev else k] += 1
        else:
            for _, qq, xx in el[i:j]:
                seen += 1
                if int(seq[qq]) != int(ref[xx]):
                    t["mm"][_cyc(qq, rl, rev)] += 1; nm += 1
        i = j
    t["nm"][nm] += 1


def tables_a(pb, reads, exclude=0, keep=None, skip_blocks=()):
    """keep: a boolean array over reads, the selection (None: all).  Returns (tables, reads excluded)."""
    refs = [pm.contig_ref(pb, c) for c in range(len(pb.contigs))]
    t, excluded = zero_tables(), 0
    for i, rd in enumerate(reads):
        if (keep is not None and not keep[i]) or rd["block"] in skip_blocks:
            continue
        if rd["flag"] & exclude:
            excluded += 1
            continue
        count_a(t, rd, refs[rd["contig"]])
    return t, excluded


# ---- model (b): SAM text with CIGAR, NM and MD ---------------------------------------------------------------------------------
def count_b(t, ln: bytes):
    """One alignment line of `--sam --cigar` into the tables, from its FLAG, CIGAR, SEQ, MD and NM columns alone."""
    c = ln.split(b"\t")
    flag, cigar, seq = int(c[1]), c[5].decode(), c[9]
    rl, rev = len(seq), bool(flag & 16)
    if cigar == "*":
        t["invalid"] += 1
        return
    assert len(c) == 13 and c[11].startswith(b"NM:i:") and c[12].startswith(b"MD:Z:"), ln
    ops = [(op, int(n)) for n, op in _CIGAR.findall(cigar)]
    assert "".join("%d%s" % (n, op) for op, n in ops) == cigar, ln
    t["reads"] += 1
    t["len"][rl] += 1
    t["nm"][int(c[11][5:])] += 1
    q, aligned = 0, []                                  # aligned: the read index of every M base, in order
    for op, n in ops:
        if op == "M":
            aligned += range(q, q + n); q += n
        elif op == "D":
            t["del_len"][n] += 1
            t["del_cyc"][rl - q if rev else q] += 1     # q: the read index of the base behind it, rl at the end
        else:
            for qq in range(q, q + n):
                t["unal"][_cyc(qq, rl, rev)] += 1
            if op == "I":
                t["ins_len"][n] += 1
                t["ins_cyc"][_cyc(q + n - 1 if rev else q, rl, rev)] += 1
            q += n
    assert q == rl, ln
    i = 0
    for num, dele, sub in _MD.findall(c[12][5:].decode("latin-1")):
        if num:
            i += int(num)
        elif sub:
            t["mm"][_cyc(aligned[i], rl, rev)] += 1; i += 1
    assert i == len(aligned), ln


def tables_b(text: bytes, exclude=0):
    """Every alignment line of a SAM text (header lines skipped).  Returns (tables, reads excluded)."""
    t, excluded = zero_tables(), 0
    for ln in text.split(b"\n"):
        if not ln or ln.startswith(b"@"):
            continue
        if int(ln.split(b"\t", 2)[1]) & exclude:
            excluded += 1
            continue
        count_b(t, ln)
    return t, excluded


def assert_models_agree(d):
    """Both models on every table of the dataset, whole and per strand, before either stands as ground truth."""
    pb, reads, names = d["pb"], d["reads"], d["names"]
    text, n = cm.expected(pb, reads, names, d["tags"])
    assert n == len(reads)
    for ex in (0, 16):
        a, xa = tables_a(pb, reads, ex)
        b, xb = tables_b(text, ex)
        assert xa == xb and same(a, b), diff(a, b)
    return tables_a(pb, reads)[0]


# ---- the text --------------------------------------------------------------------------------------------------------------------
def fraction(num, den):
    """The integer rule of cbc_hist_fraction: six decimals, rounded half up."""
    if den == 0:
        return b"0.000000"
    m = (num * 1000000 + den // 2) // den
    return b"%d.%06d" % (m // 1000000, m % 1000000)


def text(t):
    """The sections cbc_stats_aln_text writes, from Python integers."""
    ln = [int(x) for x in t["len"]]
    unal, mm = [int(x) for x in t["unal"]], [int(x) for x in t["mm"]]
    lmax = max([l for l in range(1, 257) if ln[l]], default=0)
    aligned = [0] + [sum(ln[c:]) - unal[c] for c in range(1, 257)]
    il, dl = [int(x) for x in t["ins_len"]], [int(x) for x in t["del_len"]]
    bi, bd = sum(l * n for l, n in enumerate(il)), sum(l * n for l, n in enumerate(dl))
    out = [b"AS\treads\t%d\n" % t["reads"], b"AS\treads without alignment\t%d\n" % t["invalid"], b"AS\tbases aligned\t%d\n" % sum(aligned),
           b"AS\tmismatches\t%d\n" % sum(mm), b"AS\tmismatch rate\t%s\n" % fraction(sum(mm), sum(aligned)),
           b"AS\tinsertions\t%d\n" % sum(il), b"AS\tdeletions\t%d\n" % sum(dl), b"AS\tbases inserted\t%d\n" % bi,
           b"AS\tbases deleted\t%d\n" % bd, b"AS\tbases soft-clipped\t%d\n" % (sum(unal) - bi), b"AS\treads with NM 0\t%d\n" % int(t["nm"][0])]
    out += [b"MC\t%d\t%d\t%d\n" % (c, aligned[c], mm[c]) for c in range(1, lmax + 1)]
    out += [b"IC\t%d\t%d\t%d\n" % (c, int(t["ins_cyc"][c]), int(t["del_cyc"][c])) for c in range(257) if int(t["ins_cyc"][c]) or int(t["del_cyc"][c])]
    out += [b"ID\t%d\t%d\t%d\n" % (l, il[l], dl[l]) for l in range(1, 256) if il[l] or dl[l]]
    out += [b"NM\t%d\t%d\n" % (n, int(t["nm"][n])) for n in range(767) if int(t["nm"][n])]
    return b"".join(out)


# ---- datasets ------------------------------------------------------------------------------------------------------------------
HANDMADE2 = [cg for cg, _ in cm.HANDMADE] + ["3D97M", "97M3D", "2D50M1D1M2D47M4D", "5M1D1M1D94M", "1M", "1S", "20M2I30M1D48M"]


def handmade2_dataset(seed=9):
    """Every CIGAR of cigarmodel.HANDMADE and of HANDMADE2 on both strands, variable lengths: a leading and a trailing D, two D runs
    around one aligned base, reads of length 1.  Each read has one substituted base in its first aligned run of 8 or more."""
    rng = np.random.default_rng(seed)
    c = synth.make_contig(rng, 6000)
    recs = []
    for k, cg in enumerate(HANDMADE2 + HANDMADE2):
        ops = [(op, int(n)) for n, op in re.findall(r"(\d+)([MIDS])", cg)]
        s, parts, first = 200 + 150 * k, [], None
        rp = s
        for op, n in ops:
            if op == "M":
                part = c[rp:rp + n].copy()
                if first is None and n >= 8:
                    first = True
                    part[7] = ord("A") if part[7] != ord("A") else ord("C")
                parts.append(part); rp += n
            elif op in "IS":
                parts.append(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)])
            else:
                rp += n
        seq = np.concatenate(parts)
        md, nm = synth._md_and_nm(c, s, ops, seq)
        recs.append(dict(pos=s + 1, flag=16 if k >= len(HANDMADE2) else 0, cigar=cg, seq=seq.tobytes(), md=md, nm=nm))
    fa, sam = synth.fasta_text([("hand", c)]), synth.sam_text([("hand", len(c), recs)])
    return cm._open(fa, sam, host.pack_sam(sam, fa, block_reads=8, var_length=True), [("hand", c)])


DATASETS = dict(indel=cm.indel_dataset, handmade=cm.handmade_dataset, genome=cm.genome_dataset, handmade2=handmade2_dataset)


def open_dataset(name):
    """The dataset with its plan, the reads and tags of model (a), the intervals of every read, and the whole-file tables both
    models agree on."""
    import depthmodel as dm
    d = DATASETS[name]()
    d["plan"] = host.UnpackPlan(d["blob"], d["fa"])
    d["reads"] = pm.reads_a(d["pb"])
    d["tags"] = cm.all_tags_a(d["pb"], d["reads"])
    d["iv"] = dm.intervals_a(d["pb"])
    d["whole"] = assert_models_agree(d)
    return d


# ---- the emulation library -------------------------------------------------------------------------------------------------------
def emu_load(path):
    L = ctypes.CDLL(path)
    V, U32, U64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    L.emu_aln_decode.restype = ctypes.c_int
    L.emu_aln_decode.argtypes = [V, U32, U32, V, V]
    L.emu_stats_aln.restype = ctypes.c_int
    L.emu_stats_aln.argtypes = [V, U64, V, U64, V, V, V, U32, V, U32, V, U32, V, V, U32, V, U64, U32, U32, V,
                                ctypes.POINTER(host.GpuStats), ctypes.POINTER(host.GpuStatsAln)]
    L.emu_aln_words.restype = U32
    L.emu_aln_words.argtypes = [U32]
    return L


def emu_decode_all(L, plan, per_read=16):
    """Every block of the plan, in the plan's own layout, by the emulated edits decoder against the container's span bound; a
    target set gathers from it."""
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
    assert L.emu_aln_decode(ctypes.byref(db), plan.max_read_len + plan.read_length - 1, per_read, side.ctypes.data, arena.ctypes.data) == 0
    return dict(bl=bl, recs=recs, seq=seq, res=res, nrec=nrec, side=side, arena=arena, per_read=per_read)


def emu_stats_aln(L, plan, dec, ts=None, exclude=0, grid=0, n_waves=4, fail_blocks=()):
    """One cbc_gpu_decode_stats_aln on the emulation.  dec: emu_decode_all; ts: a host.TargetSet or None (every block).  Returns
    (rc, statistics tables as statsmodel has them, alignment tables)."""
    import statsmodel as sm
    sel = np.arange(plan.n_blocks, dtype=np.int64) if ts is None else ts.blocks.astype(np.int64)
    st, al = host.GpuStats(), host.GpuStatsAln()
    if len(sel) == 0:
        return 0, sm.as_tables(st), host.stats_aln_dict(al)
    bl = np.ascontiguousarray(dec["bl"][sel])
    ws = np.ascontiguousarray(plan.window_start[sel], dtype=np.uint64)
    res = dec["res"][sel].copy()
    for b in fail_blocks:
        res[b]["status"] = 2
    iv = biv = None
    if ts is not None:
        iv, biv = np.ascontiguousarray(ts.iv, dtype=np.uint32), np.ascontiguousarray(ts.block_iv, dtype=np.uint32)
    rc = L.emu_stats_aln(dec["recs"].ctypes.data, dec["nrec"], dec["seq"].ctypes.data, dec["seq"].size, bl.ctypes.data, ws.ctypes.data,
                         res.ctypes.data, len(sel), iv.ctypes.data if ts is not None else None, ts.n_iv if ts is not None else 0,
                         biv.ctypes.data if ts is not None else None, exclude, dec["side"].ctypes.data, dec["arena"].ctypes.data,
                         dec["per_read"], plan.ref.ctypes.data, len(plan.ref), grid, n_waves, None, ctypes.byref(st), ctypes.byref(al))
    return rc, sm.as_tables(st), host.stats_aln_dict(al)
