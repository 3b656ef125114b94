"""CIGAR, NM and MD of the SAM output in plain Python: what `cbc -x --sam --cigar` must write.  Two
independent models -- (a) the codec's view, from the packed arrays through pileupmodel.reads_a (dc, oi) and the element order of
include/cbc_gpu.h: per matched coordinate m the inserted read indices in front of aligned base m, the deleted bases with dc = m,
aligned base m; (b) the SAM text that was compressed: its CIGAR with = and X folded into M, NM and MD recomputed with
synth._md_and_nm under the byte rule, with ONE normalisation: a read whose SEQ equals its reference window is <rl>M, 0, <rl>
(the codec stores it as perfect) -- a third check that needs no model (check_line: SEQ + CIGAR + MD give back the reference), and
the ctypes wrapper of the emulation library (tests/cigar_emu)."""
import ctypes
import re

import numpy as np

import blockref
import pileupmodel as pm
import sammodel as sm
import synth
from cbc_amd import host

_CIGAR = re.compile(r"(\d+)([MIDNSHP=X])")
_MD = re.compile(r"(\d+)|(\^[^0-9]+)|([^0-9^])")


# ---- model (a): the packed arrays ----------------------------------------------------------------------------------------------
def tags_a(rd, ref):
    """(CIGAR, NM, MD) of one read of pileupmodel.reads_a; ref: the uploaded bytes of its contig.  None for lists that are not
    what the decoder writes (the plain line)."""
    seq, dc, oi, pos = rd["seq"], [int(x) for x in rd["dc"]], [int(x) for x in rd["oi"]], rd["pos"]
    rl, nd, ni = len(seq), len(dc), len(oi)
    if rl == 0 or nd > 255 or ni > 255 or ni > rl:
        return None
    T = rl - ni
    if any(d > T for d in dc) or any(a > b for a, b in zip(dc, dc[1:])):
        return None
    if any(o >= rl for o in oi) or any(a >= b for a, b in zip(oi, oi[1:])):
        return None
    ins = set(oi)
    el, q, di, x = [], 0, 0, pos - 1                    # elements: (kind, read index or None, reference index or None)
    for m in range(T + 1):
        while q < rl and q in ins:
            el.append(("I", q, None)); q += 1
        while di < nd and dc[di] == m:
            el.append(("D", None, x)); x += 1; di += 1
        if m < T:
            el.append(("M", q, x)); q += 1; x += 1
    assert q == rl and di == nd
    if x > len(ref):
        return None
    cigar, md, nm, n, i = [], [], 0, 0, 0
    n_al = sum(1 for e in el if e[0] == "M")
    seen = 0
    while i < len(el):
        j = i
        while j < len(el) and el[j][0] == el[i][0]:
            j += 1
        op = el[i][0]
        if op == "I":
            if seen == 0 or seen == n_al:
                op = "S"                                # no aligned base before it in the read, or none after it
            else:
                nm += j - i
        elif op == "D":
            md.append("%d^%s" % (n, bytes(ref[el[i][2]:el[j - 1][2] + 1]).decode("latin-1"))); n = 0; nm += j - i
        else:
            for _, qq, xx in el[i:j]:
                seen += 1
                if int(seq[qq]) == int(ref[xx]):
                    n += 1
                else:
                    md.append("%d%c" % (n, int(ref[xx]))); n = 0; nm += 1
        cigar.append("%d%s" % (j - i, op))
        i = j
    md.append(str(n))
    return "".join(cigar), nm, "".join(md)


def line(flag, rname, pos, seq, tags):
    """The alignment line; tags None: the plain one of sammodel."""
    if tags is None:
        return sm.line(flag, rname, pos, seq)
    return b"*\t%d\t%s\t%d\t255\t%s\t*\t0\t0\t%s\t*\tNM:i:%d\tMD:Z:%s\n" % (flag, rname, pos, tags[0].encode(), seq, tags[1],
                                                                          tags[2].encode("latin-1"))


def all_tags_a(pb, reads):
    refs = [pm.contig_ref(pb, c) for c in range(len(pb.contigs))]
    return [tags_a(rd, refs[rd["contig"]]) for rd in reads]


def expected(pb, reads, names, tags, region=None, skip_blocks=()):
    """The lines of the whole container or of region = (contig, beg, end) (the overlap rule of the region decode: POS <= end and
    POS + span - 1 >= beg), in container order.  Returns (bytes, reads)."""
    out = []
    for rd, t in zip(reads, tags):
        if rd["block"] in skip_blocks:
            continue
        if region is not None and (rd["contig"] != region[0] or rd["pos"] > region[2] or rd["pos"] + rd["span"] - 1 < region[1]):
            continue
        out.append(line(rd["flag"], names[rd["contig"]], rd["pos"], rd["seq"].tobytes(), t))
    return b"".join(out), len(out)


# ---- model (b): the SAM text ---------------------------------------------------------------------------------------------------
def tags_b(sam: bytes, pb, names):
    """(CIGAR, NM, MD) per mapped alignment line from its own CIGAR (= and X folded into M) and SEQ against the uploaded
    reference, under the byte rule; a read whose SEQ equals its reference window: <rl>M, 0, <rl>.  Returns (tags, normalised)."""
    refs = [pm.contig_ref(pb, c) for c in range(len(names))]
    out, normalised = [], 0
    for ln in sam.split(b"\n"):
        if not ln or ln.startswith(b"@"):
            continue
        c = ln.split(b"\t")
        if int(c[1]) & 4:
            continue
        ref, pos, seq = refs[names.index(c[2])], int(c[3]), np.frombuffer(c[9], dtype=np.uint8)
        ops = []
        for n, op in _CIGAR.findall(c[5].decode()):
            op = "M" if op in "=X" else op
            if ops and ops[-1][0] == op:
                ops[-1] = (op, ops[-1][1] + int(n))
            else:
                ops.append((op, int(n)))
        rl = len(seq)
        if ops != [("M", rl)] and seq.tobytes() == ref[pos - 1:pos - 1 + rl].tobytes():
            ops = [("M", rl)]; normalised += 1
        md, nm = synth._md_and_nm(ref, pos - 1, ops, seq, synth.byte_mismatch)
        out.append(("".join("%d%s" % (n, op) for op, n in ops), nm, md))
    return out, normalised


def assert_models_agree(pb, sam, names, max_normalised=5):
    """Both models on every read before either stands as ground truth.  Returns (reads of model (a), their tags)."""
    reads = pm.reads_a(pb)
    ta = all_tags_a(pb, reads)
    tb, normalised = tags_b(sam, pb, names)
    assert len(ta) == len(tb) and normalised <= max_normalised, (len(ta), len(tb), normalised)
    bad = [i for i, (x, y) in enumerate(zip(ta, tb)) if x != y]
    assert not bad, "models (a) and (b) differ on %d reads, first %d: %r / %r" % (len(bad), bad[0], ta[bad[0]], tb[bad[0]])
    return reads, ta


# ---- the check that needs no model ---------------------------------------------------------------------------------------------
def check_line(ln: bytes, ref):
    """SEQ + CIGAR + MD of one written line give back the reference bytes at POS over M and D, and NM is the count of
    mismatches, I bases and D bases.  ref: the uploaded bytes of the line's contig.  Returns the CIGAR."""
    c = ln.split(b"\t")
    assert len(c) == 13 and c[0] == b"*" and c[4] == b"255" and c[6:9] == [b"*", b"0", b"0"] and c[10] == b"*", ln
    assert c[11].startswith(b"NM:i:") and c[12].startswith(b"MD:Z:"), ln
    pos, seq, cigar, nm, md = int(c[3]), c[9], c[5].decode(), int(c[11][5:]), c[12][5:].decode("latin-1")
    ops = [(op, int(n)) for n, op in _CIGAR.findall(cigar)]
    assert "".join("%d%s" % (n, op) for op, n in ops) == cigar and all(op in "MIDS" and n > 0 for op, n in ops), ln
    assert all(a[0] != b[0] for a, b in zip(ops, ops[1:])), ln
    aligned, q = [], 0                                  # the read bytes of the M bases, None per deleted base
    for op, n in ops:
        if op == "M":
            aligned += list(seq[q:q + n]); q += n
        elif op == "D":
            aligned += [None] * n
        else:
            q += n
    assert q == len(seq), ln
    rebuilt, i, count = [], 0, sum(n for op, n in ops if op in "ID")
    for num, dele, sub in _MD.findall(md):
        if num:
            k = int(num)
            assert all(b is not None for b in aligned[i:i + k]), ln
            rebuilt += aligned[i:i + k]; i += k
        elif dele:
            k = len(dele) - 1
            assert aligned[i:i + k] == [None] * k and (i + k == len(aligned) or aligned[i + k] is not None) and \
                (i == 0 or aligned[i - 1] is not None), ln
            rebuilt += list(dele[1:].encode("latin-1")); i += k
        else:
            assert aligned[i] is not None and aligned[i] != ord(sub), ln
            rebuilt.append(ord(sub)); i += 1; count += 1
    assert i == len(aligned) and bytes(rebuilt) == ref[pos - 1:pos - 1 + len(aligned)].tobytes(), ln
    assert count == nm, ln
    return cigar


def check_text(text: bytes, pb, names):
    """check_line on every alignment line with a CIGAR; returns (lines, lines with tags)."""
    refs = {n: pm.contig_ref(pb, c) for c, n in enumerate(names)}
    n = tagged = 0
    for ln in text.split(b"\n")[:-1]:
        if ln.startswith(b"@"):
            continue
        n += 1
        c = ln.split(b"\t")
        if c[5] != b"*":
            check_line(ln, refs[c[2]]); tagged += 1
    return n, tagged


def strip(text: bytes):
    """The lines with CIGAR put back to '*' and the tags dropped: what decode_sam(cigar=False) writes."""
    out = []
    for ln in text.split(b"\n")[:-1]:
        c = ln.split(b"\t")
        if not ln.startswith(b"@") and len(c) == 13:
            c = c[:5] + [b"*"] + c[6:11]
        out.append(b"\t".join(c) + b"\n")
    return b"".join(out)


# ---- the emulation library -----------------------------------------------------------------------------------------------------
def emu_load(path):
    L = ctypes.CDLL(path)
    L.emu_cigar_decode.restype = ctypes.c_int
    L.emu_cigar_decode.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    L.emu_sam_cigar.restype = ctypes.c_int
    L.emu_sam_cigar.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int,
                                ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p,
                                ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    return L


def emu_decode(L, plan, b0, b1, smax, per_read=16):
    """pileupmodel.emu_decode through this library's decoder entry: (blocks, recs, rows, results, records, side, arena)."""
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
    side = np.zeros((max(nrec, 1), 2), dtype=np.uint32)
    arena = np.full(max(nrec * per_read, 1), 0xEEEE, dtype=np.uint16)
    db = blockref.DecDeviceBatch(pay.ctypes.data, pay.size, bl.ctypes.data, b1 - b0, plan.ref.ctypes.data, len(plan.ref),
                                 recs.ctypes.data, nrec, seq.ctypes.data, seq.size, res.ctypes.data, vs.ctypes.data, vs.size,
                                 host.LdsCaps(plan.cap_pos, plan.cap_var))
    assert L.emu_cigar_decode(ctypes.byref(db), smax, per_read, side.ctypes.data, arena.ctypes.data) == 0
    return bl, recs, seq, res, nrec, side, arena


def emu_call(L, plan, sel=None, per_read=16, cap=None, fail_blocks=(), dec=None, n_waves=4):
    """One cbc_gpu_decode_sam_cigar on the emulation: edits decode of the selection (None: every block, against the container's
    span bound), then the three passes.  Returns (rc, text, reads, text bytes); the guard bytes behind the text (all of it
    when nothing may be written) must be untouched."""
    b0, b1 = (sel.b0, sel.b1) if sel is not None else (0, plan.n_blocks)
    if b1 == b0:
        return 0, b"", 0, 0
    smax = sel.smax if sel is not None else plan.max_read_len + plan.read_length - 1
    bl, recs, seq, res, nrec, side, arena = dec if dec is not None else emu_decode(L, plan, b0, b1, smax, per_read)
    res = res.copy()
    for b in fail_blocks:
        res[b]["status"] = 2
    ws = np.ascontiguousarray(plan.window_start[b0:b1], dtype=np.uint64)
    bn = np.zeros(2 * (b1 - b0), dtype=np.uint32)
    for k, c in enumerate(plan.block_contig[b0:b1]):
        off = int(plan.contig_name_off[int(c)])
        bn[2 * k], bn[2 * k + 1] = off, plan.names[off:].tobytes().index(b"\0")
    names = np.ascontiguousarray(plan.names)
    cap = plan.sam_cigar_text_cap(b0, b1, per_read) if cap is None else cap
    text = np.full(cap + 16, 0xEE, dtype=np.uint8)
    out = np.zeros(2, dtype=np.uint64)
    beg, end = (sel.beg, sel.end) if sel is not None else (0, 0)
    rc = L.emu_sam_cigar(recs.ctypes.data, nrec, seq.ctypes.data, seq.size, bl.ctypes.data, ws.ctypes.data, res.ctypes.data, b1 - b0,
                         bn.ctypes.data, names.ctypes.data, names.size, 1 if sel is not None else 0, beg, end, side.ctypes.data,
                         arena.ctypes.data, per_read, plan.ref.ctypes.data, len(plan.ref), n_waves, text.ctypes.data, cap,
                         out.ctypes.data)
    total = int(out[0])
    wrote = rc in (0, -4)
    assert (text[total if wrote else 0:] == 0xEE).all(), "bytes written outside the text"
    return rc, (text[:total].tobytes() if wrote else b""), int(out[1]), total


# ---- datasets ------------------------------------------------------------------------------------------------------------------
def _open(fa, sam, pb, contigs):
    import depthmodel as dm
    import regionmodel as rm
    names, lens = dm.names_lens(None, contigs)
    return dict(fa=fa, sam=sam, pb=pb, blob=rm.container(pb), names=names, lens=lens)


def indel_dataset():
    """Indels in a quarter of the reads, trailing soft clips in a quarter, SNPs at 1 %: every kind of line many times."""
    fa, sam, rbc, contigs = synth.dataset(11, [30000, 12000], [700, 300], 150, indel_frac=0.25, trailing_s_frac=0.25, sub_rate=0.01)
    d = _open(fa, sam, host.pack_sam(sam, fa, block_reads=128), contigs)
    d["rbc"] = rbc
    return d


HANDMADE = [("5S95M", "5S95M"), ("4S90M6S", "4S90M6S"), ("5S45M2I48M", "5S45M2I48M"), ("40M2D3I57M", "40M3I2D57M"),
            ("40M3I2D57M", "40M3I2D57M"), ("95M5I", "95M5S")]


def handmade_dataset(seed=3):
    """One read per CIGAR of HANDMADE (input, what comes back), each with one substituted base in its first aligned run."""
    rng = np.random.default_rng(seed)
    c = synth.make_contig(rng, 4000)
    recs = []
    for k, (cg, _) in enumerate(HANDMADE):
        ops = [(op, int(n)) for n, op in _CIGAR.findall(cg)]
        s, parts, rp, first = 200 + 150 * k, [], 200 + 150 * k, None
        for op, n in ops:
            if op == "M":
                part = c[rp:rp + n].copy()
                if first is None:
                    first = True
                    part[7] = ord("A") if part[7] != ord("A") else ord("C")
                parts.append(part); rp += n
            elif op in "IS":
                parts.append(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)])
            else:
                rp += n
        seq = np.concatenate(parts)
        md, nm = synth._md_and_nm(c, s, ops, seq)
        recs.append(dict(pos=s + 1, flag=0, cigar=cg, seq=seq.tobytes(), md=md, nm=nm))
    fa, sam = synth.fasta_text([("hand", c)]), synth.sam_text([("hand", len(c), recs)])
    return _open(fa, sam, host.pack_sam(sam, fa, block_reads=64, var_length=True), [("hand", c)])


def genome_dataset():
    """N gaps, IUPAC codes and soft-masking in the reference, N-rich reads; the generator lists N over N in the input's MD for
    half the reads and folds it into the match run for the others (its nn_listed is drawn per read), so the input's own MD is
    no yardstick here: model (b) recomputes it under the byte rule."""
    fa, sam, rbc, contigs = synth.genome_dataset(17, contig_lens=(40_000, 12_000), reads_per_contig=(500, 150),
                                                 contig_kw=dict(n_gaps=3, max_gap=2000))
    return _open(fa, sam, host.pack_sam(sam, fa, block_reads=128), contigs)
