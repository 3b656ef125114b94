"""The consensus record in plain Python: what `cbc -x --consensus` must write.  No alignment logic of its
own: the counts are pileupmodel.tables() -- code that is not under test here --, the call rule is the four steps of
include/cbc_gpu.h in Python integers, one position at a time, and the FASTA layout is a header plus the emitted bytes cut into
lines.  Also the two datasets the consensus tests add to those of tests/test_pileup.py (`boundary`, `deep`), and the ctypes wrapper
of the emulation library (tests/consensus_emu)."""
import ctypes

import numpy as np

import pileupmodel as pm
import synth
from cbc_amd import host

SHOW_DEL, FILL_REF, IUPAC = 1, 2, 4
KEYS = ("emitted", "ref", "alt", "del", "ambiguous", "low_depth", "no_call", "ins_skipped")
_CODE = b"NACMGRSVTWYHKDBN"                                     # bit s of the index = base s of A, C, G, T


def reaches(x, depth, ppm):
    return x * 1_000_000 >= ppm * depth


def call(c, d, ins, ref, min_depth=1, ppm=750_000, flags=0):
    """One position.  c: the five class counts, d: deleted bases, ins: insertion events, ref: the reference byte.
    Returns (byte or None, counter name, ins_skipped, tie) with tie = "ref" / "order" when more than one candidate holds the
    highest count and the reference's class / the order decided, else ""."""
    depth = sum(c) + d
    if depth < min_depth:
        b = ref
        if flags & FILL_REF:
            b = ref | 0x20 if 0x41 <= (ref & 0xDF) <= 0x5A else ref
        return (b if flags & FILL_REF else ord("N")), "low_depth", False, ""
    skipped = reaches(ins, depth, ppm)
    cand = [c[0], c[1], c[2], c[3], d]
    top = max(cand)
    tied = [k for k in range(5) if cand[k] == top]
    cr = int(pm.klass(ref))
    w = cr if cr in tied else tied[0]
    tie = "" if len(tied) == 1 else ("ref" if cr in tied else "order")
    if reaches(top, depth, ppm):
        if w == 4:
            return (ord("*") if flags & SHOW_DEL else None), "del", skipped, tie
        return b"ACGT"[w], ("ref" if w == cr else "alt"), skipped, tie
    if flags & IUPAC:
        best = None
        for t in sorted({c[i] for i in range(4) if c[i] > 0}):
            s = [j for j in range(4) if c[j] >= t]
            if reaches(sum(c[j] for j in s), depth, ppm):
                best = s                                             # ascending t: the last one that reaches is the largest
        if best is not None:
            return _CODE[sum(1 << j for j in best)], "ambiguous", skipped, tie
    return ord("N"), "no_call", skipped, tie


def calls(pb, reads, c, beg, end, exclude=0, min_depth=1, ppm=750_000, flags=0, skip_blocks=()):
    """Every position of the window: ([call(...)], reads kept)."""
    cnt, dl, ins, kept = pm.tables(reads, c, beg, end, exclude, skip_blocks)
    ref = pm.contig_ref(pb, c)[beg - 1:end]
    W = end - beg + 1
    refb = np.full(W, ord("N"), dtype=np.int64)                      # past the contig's bytes: N, as on the device
    refb[:len(ref)] = ref
    depth = cnt.sum(axis=0) + dl
    low = call([0] * 5, 0, 0, ord("N"), min_depth, ppm, flags)
    out = [low] * W
    for i in np.flatnonzero((depth >= min_depth) | (bool(flags & FILL_REF))).tolist():
        out[i] = call([int(x) for x in cnt[:, i]], int(dl[i]), int(ins[i]), int(refb[i]), min_depth, ppm, flags)
    return out, kept


def record(name: bytes, beg, end, body: bytes, width=60, with_range=False) -> bytes:
    hdr = b">%s:%d-%d\n" % (name, beg, end) if with_range else b">%s\n" % name
    return hdr + b"".join(body[i:i + width] + b"\n" for i in range(0, len(body), width))


def expected(pb, reads, names, lens, region=None, exclude=0, min_depth=1, ppm=750_000, width=60, flags=0, skip_blocks=(), with_range=None):
    """The records of the whole container (every contig of the table in table order) or of region = (contig, beg, end), which
    carries its range in the header (with_range=False: it does not).  Returns (fasta bytes, counts dict, reads kept)."""
    todo = [region] if region is not None else [(c, 1, lens[c]) for c in range(len(names))]
    out, kept, cnt = [], 0, dict.fromkeys(KEYS, 0)
    for c, beg, end in todo:
        cs, k = calls(pb, reads, c, beg, end, exclude, min_depth, ppm, flags, skip_blocks)
        body = bytes(b for b, _, _, _ in cs if b is not None)
        out.append(record(names[c], beg, end, body, width, region is not None if with_range is None else with_range))
        kept += k
        cnt["emitted"] += len(body)
        for _, kind, skipped, _ in cs:
            cnt[kind] += 1
            cnt["ins_skipped"] += bool(skipped)
    return b"".join(out), cnt, kept


def body_of(fasta: bytes):
    """(header line, the bytes of the lines joined) of ONE record; asserts the layout: every line ends in a newline, none is
    empty, every line but the last has the first line's width."""
    assert fasta.startswith(b">") and fasta.endswith(b"\n")
    lines = fasta[:-1].split(b"\n")
    assert all(lines[1:]) and all(len(x) == len(lines[1]) for x in lines[1:-1]) and (len(lines) < 3 or len(lines[-1]) <= len(lines[1]))
    return lines[0], b"".join(lines[1:])


# ---- datasets ------------------------------------------------------------------------------------------------------------------
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _other(base, k=1):
    return int(_ACGT[(int(np.where(_ACGT == base)[0][0]) + k) % 4])


def _layered(contig, n_layers, dels, inss, snps, gaps, first_len, L=100):
    """n_layers layers of reads, each tiling the contig end to end (so the depth is n_layers wherever no gap is): layer l starts
    with a read of first_len(l) bases, then reads of L.  dels: (pos1, length, layers) -- the reads of those layers delete
    reference positions pos1 .. pos1 + length - 1; inss: (pos1, length, layers): they insert `length` bases behind position
    pos1; snps: (pos1, {layer: base}); gaps: (pos1, length): no read of any layer covers them.  A read keeps 8 matched bases on
    both sides of a deletion or an insertion: one that would end closer in front of it is made longer and carries it, and one
    that would leave fewer than 30 bases in front of a gap or of the contig's end takes them.  Layer l is on the reverse strand
    when l is odd.  Returns the records sorted by POS."""
    n = len(contig)
    snp_at = {p: m for p, m in snps}
    recs = []
    for l in range(n_layers):
        feats = sorted([(p, ln, "D") for p, ln, ls in dels if l in ls] + [(p + 1, ln, "I") for p, ln, ls in inss if l in ls] +
                       [(p, ln, "G") for p, ln in gaps])
        pos, want = 1, first_len(l)
        while pos <= n:
            gap = next(((p, ln) for p, ln, k in feats if k == "G" and p <= pos < p + ln), None)
            if gap:
                pos, want = gap[0] + gap[1], L
                continue
            ops, q, r, target, used = [], 0, pos, want, set()
            while True:
                f = next((x for x in feats if x[0] >= r and x not in used), None)
                avail = (f[0] if f else n + 1) - r                   # matched bases in front of the next feature or the end
                need = target - q
                if need <= avail:
                    if f and f[2] != "G" and avail - need < 8:
                        target += 16 + f[1]
                        continue
                    if (f is None or f[2] == "G") and avail - need < 30:
                        need = avail
                    ops.append(("M", need)); r += need
                    break
                ops.append(("M", avail)); q += avail; r += avail
                if f is None or f[2] == "G":
                    break
                assert avail >= 8 or len(ops) > 1, "a feature within 8 bases of a read's start"
                used.add(f)
                ops.append((f[2], f[1]))
                if f[2] == "D":
                    r += f[1]
                else:
                    q += f[1]
                target = max(target, q + 8)
            merged = []
            for op, ln in ops:
                if ln and merged and merged[-1][0] == op:
                    merged[-1] = (op, merged[-1][1] + ln)
                elif ln:
                    merged.append((op, ln))
            parts, rp = [], pos
            for op, ln in merged:
                if op == "M":
                    seg = contig[rp - 1:rp - 1 + ln].copy()
                    for p in range(rp, rp + ln):
                        if p in snp_at and l in snp_at[p]:
                            seg[p - rp] = snp_at[p][l]
                    parts.append(seg); rp += ln
                elif op == "I":
                    parts.append(np.array([_other(contig[rp - 1], 1 + i % 3) for i in range(ln)], dtype=np.uint8))
                else:
                    rp += ln
            assert rp == r
            seq = np.concatenate(parts)
            md, nm = synth._md_and_nm(contig, pos - 1, merged, seq)
            recs.append(dict(pos=pos, flag=16 * (l & 1), cigar="".join("%d%s" % (ln, op) for op, ln in merged), seq=seq.tobytes(), md=md, nm=nm))
            pos, want = r, L
    recs.sort(key=lambda x: x["pos"])
    return recs


BOUNDARY = dict(del_tile0=(4094, 3), del_tile1=(6000, 3), del_half=(2000, 2), ins_all=3000, ins_half=3200, snp_all=(500, 4500),
                snp_3of4=(900, 5200), snp_half_ref=(1300, 5600), snp_half_two=(1700, 6400), gap=(7000, 150), length=2 * 4096 + 200)


def boundary(seed=11, block_reads=64):
    """One contig of 2 * 4096 + 200 bases under eight layers of reads (depth 8 wherever covered), the features of BOUNDARY: a
    3-base deletion every read carries on the last three positions of tile 0 and one inside tile 1, a 2-base deletion half the
    reads carry, a 2-base insertion every read / half the reads carry, SNP sites whose alternative all, 6 of 8 and 4 of 8 layers
    carry -- the 4-of-8 ones against the reference base and against a second alternative --, and 150 uncovered bases.  Even
    layers are forward, so under exclusion mask 16 the fractions are 4 of 4, 3 of 4 and 2 of 4.  Returns (fasta, sam, packed
    batch, contigs)."""
    B = BOUNDARY
    rng = np.random.default_rng(seed)
    contig = synth.make_contig(rng, B["length"])
    every, half, six = set(range(8)), {0, 1, 2, 3}, {0, 1, 2, 3, 4, 5}
    snps = []
    for p in B["snp_all"]:
        snps.append((p, {l: _other(contig[p - 1]) for l in every}))
    for p in B["snp_3of4"]:
        snps.append((p, {l: _other(contig[p - 1], 2) for l in six}))
    for p in B["snp_half_ref"]:
        snps.append((p, {l: _other(contig[p - 1], 3) for l in half}))
    for p in B["snp_half_two"]:
        snps.append((p, {l: _other(contig[p - 1], 1 if l in half else 2) for l in every}))
    recs = _layered(contig, 8, [B["del_tile0"] + (every,), B["del_tile1"] + (every,), B["del_half"] + (half,)],
                    [(B["ins_all"], 2, every), (B["ins_half"], 2, half)], snps, [B["gap"]], lambda l: 100 - 11 * l)
    fa = synth.fasta_text([("bnd", contig)])
    sam = synth.sam_text([("bnd", len(contig), recs)])
    return fa, sam, host.pack_sam(sam, fa, block_reads=block_reads, var_length=True), [("bnd", contig)]


DEEP = dict(site_3750=60, site_3749=70, site_2500=80, reads=5000)


def deep(seed=13, block_reads=256):
    """A 150-base contig under 5 000 reads of 100 bases, all of which cover positions 51..100: depth * 10^6 passes 2^32 from
    depth 4 295, so a 32-bit product shows here.  The alternative at DEEP's three sites is carried by exactly 3 750, 3 749 and
    2 500 reads, chosen across the start positions.  Returns (fasta, sam, packed batch, contigs)."""
    rng = np.random.default_rng(seed)
    contig = synth.make_contig(rng, 150)
    n = DEEP["reads"]
    starts = np.sort(np.arange(n) % 51)
    order = rng.permutation(n)
    recs = []
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n)
    for i in range(n):
        s = int(starts[i])
        seq = contig[s:s + 100].copy()
        for site, k in ((DEEP["site_3750"], 3750), (DEEP["site_3749"], 3749), (DEEP["site_2500"], 2500)):
            if rank[i] < k:
                seq[site - 1 - s] = _other(contig[site - 1])
        md, nm = synth._md_and_nm(contig, s, [("M", 100)], seq)
        recs.append(dict(pos=s + 1, flag=16 * (i & 1), cigar="100M", seq=seq.tobytes(), md=md, nm=nm))
    fa = synth.fasta_text([("deep", contig)])
    sam = synth.sam_text([("deep", 150, recs)])
    return fa, sam, host.pack_sam(sam, fa, block_reads=block_reads), [("deep", contig)]


# ---- the emulation library -----------------------------------------------------------------------------------------------------
def emu_load(path):
    L = ctypes.CDLL(path)
    L.emu_consensus.restype = ctypes.c_int
    L.emu_consensus.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p,
                                ctypes.c_uint64, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64] + \
                               [ctypes.c_uint32] * 7 + [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    return L


def emu_call(L, Ldec, plan, sel, with_range, exclude=0, min_depth=1, ppm=750_000, width=60, flags=0, per_read=16, cap=None, fail_blocks=(),
             dec=None, n_waves=4):
    """One cbc_gpu_decode_consensus on the emulation: the edits decode of the selection by tests/pileup_emu's library Ldec (or
    `dec`, an earlier one), then every pass; a selection without blocks takes its record from the host function, as the binding
    does.  Returns (rc, text, counts dict, reads kept, text bytes); the guard bytes behind the text must be untouched."""
    if sel.b1 == sel.b0:
        text, cnt = plan.consensus_empty(sel.contig, sel.beg, sel.end, host.ConsensusOpts(min_depth, ppm, width, flags), with_range)
        return 0, text, cnt, 0, len(text)
    bl, recs, seq, res, nrec, side, arena = dec if dec is not None else pm.emu_decode(Ldec, plan, sel.b0, sel.b1, sel.smax, per_read)
    res = res.copy()
    for b in fail_blocks:
        res[b]["status"] = 2
    ws = np.ascontiguousarray(plan.window_start[sel.b0:sel.b1], dtype=np.uint64)
    off = int(plan.contig_name_off[sel.contig])
    name = plan.names[off:].tobytes().split(b"\0", 1)[0]
    cap = plan.consensus_text_cap(sel.contig, sel.beg, sel.end, width, with_range) if cap is None else cap
    text = np.full(cap + 16, 0xEE, dtype=np.uint8)
    out = np.zeros(10, dtype=np.uint64)
    c0 = int(plan.blocks[sel.b0]["ref_off"]) - int(ws[0])
    rc = L.emu_consensus(recs.ctypes.data, nrec, seq.ctypes.data, seq.size, bl.ctypes.data, ws.ctypes.data, res.ctypes.data,
                         sel.b1 - sel.b0, side.ctypes.data, arena.ctypes.data, per_read, plan.ref.ctypes.data, len(plan.ref), c0,
                         name, len(name), sel.beg, sel.end, exclude, min_depth, ppm, width, flags, int(bool(with_range)), n_waves,
                         text.ctypes.data, cap, out.ctypes.data)
    total = int(out[0])
    wrote = rc in (0, -4)
    assert (text[total if wrote else min(total, cap):] == 0xEE).all(), "bytes written outside the text"
    return rc, (text[:total].tobytes() if wrote else b""), dict(zip(KEYS, (int(x) for x in out[2:10]))), int(out[1]), total


def emu_whole(L, Ldec, plan, decs=None, **kw):
    """Every contig of the table in table order, records appended: what `cbc -x --consensus` does.  decs: a dict that keeps every
    contig's decode for the next call."""
    text, kept, cnt = [], 0, dict.fromkeys(KEYS, 0)
    for c in range(plan.n_contigs):
        sel = plan.contig_blocks(c)
        dec = None
        if decs is not None and sel.b1 > sel.b0:
            if c not in decs:
                decs[c] = pm.emu_decode(Ldec, plan, sel.b0, sel.b1, sel.smax, 16)
            dec = decs[c]
        rc, t, n, k, _ = emu_call(L, Ldec, plan, sel, False, dec=dec, **kw)
        assert rc == 0
        text.append(t); kept += k
        for key in KEYS:
            cnt[key] += n[key]
    return b"".join(text), cnt, kept
