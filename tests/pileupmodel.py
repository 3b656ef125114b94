"""Per-position allele counts in plain Python: what `cbc -x --pileup` must write.  Two independent
models of what a read shows where -- (a) the codec's view, from the packed arrays (recs, seq, tok): the CIGAR tokens give the
deleted bases' matched coordinates and the inserted bases' read indices (a trailing S is an insertion), and the mapping of
include/cbc_gpu.h places every base; (b) POS + CIGAR + SEQ of the SAM text that was compressed, walked operation by operation
-- one table / formatter routine in Python integers, the datasets the CPU and the GPU tests share, and the ctypes wrapper of the
emulation library (tests/pileup_emu)."""
import ctypes
import re

import numpy as np

import blockref
import synth
from cbc_amd import host

_CIGAR = re.compile(rb"(\d+)([MIDNSHP=X])")
_CLASS = np.full(256, 4, dtype=np.int64)
for _i, _ch in enumerate(b"ACGT"):
    _CLASS[_ch] = _CLASS[_ch | 0x20] = _i


def klass(b):
    """0..3 = A, C, G, T in either case, 4 = anything else: the class of byte & 0xDF."""
    return _CLASS[b]


# ---- model (a): the packed arrays ----------------------------------------------------------------------------------------------
def reads_a(pb):
    """Per record, in container order: dict(contig, pos, span, flag, block, seq, dc, oi).  A read whose SEQ equals its
    reference window is coded as perfect and has no edits; any other takes them from its CIGAR tokens: dc = the matched bases in
    front of every deleted base, oi = the read index of every inserted (I or S) base."""
    out = []
    for b in range(pb.n_blocks):
        bd, inf = pb.blocks[b], pb.info[b]
        c, ws = int(inf["contig"]), int(inf["window_start"])
        ref0 = int(pb.contigs[c]["ref_off"])
        for k in range(int(bd["n_reads"])):
            r = pb.recs[int(bd["rec_base"]) + k]
            rl = int(r["rlen"])
            s0 = int(bd["seq_base"]) + int(r["seq_off"])
            seq = pb.seq[s0:s0 + rl]
            pos = ws + int(r["pos"])
            t0 = int(bd["tok_base"]) + int(r["tok_off"])
            dc, oi = [], []
            if seq.tobytes() != pb.ref[ref0 + pos - 1: ref0 + pos - 1 + rl].tobytes():
                n_cigar = int(pb.tok[t0]) & 0xffff
                q = m = 0
                for w in pb.tok[t0 + 2: t0 + 2 + n_cigar].tolist():
                    ln, op = w >> 4, w & 15
                    if op == 0:
                        q += ln; m += ln
                    elif op in (1, 3):
                        oi += range(q, q + ln); q += ln
                    elif op == 2:
                        dc += [m] * ln
                    else:
                        raise AssertionError("op %d in the tokens" % op)
                assert q == rl
                w1 = int(pb.tok[t0 + 1])
                assert (w1 & 0xffff, w1 >> 16) == (len(dc), len(oi))
            out.append(dict(contig=c, pos=pos, span=rl + len(dc) - len(oi), flag=int(r["flag"]), block=b, seq=seq.copy(),
                            dc=np.array(dc, dtype=np.int64), oi=np.array(oi, dtype=np.int64)))
    return out


def events_a(rd):
    """(aligned positions, their bases, deleted positions, insertion anchors) of one read by the mapping of include/cbc_gpu.h;
    whatever falls outside [POS, POS + span - 1] is dropped."""
    pos, span, seq, dc, oi = rd["pos"], rd["span"], rd["seq"], rd["dc"], rd["oi"]
    q = np.arange(len(seq), dtype=np.int64)
    isins = np.isin(q, oi)
    m = q - np.searchsorted(oi, q, side="left")                      # oi ascends: #{oi < q}
    x = m + np.searchsorted(dc, m, side="right")                     # dc ascends: #{dc <= m}
    al = ~isins & (x < span)
    dl = dc + np.arange(len(dc), dtype=np.int64)
    dl = dl[dl < span]
    first = isins & ~np.concatenate([[False], isins[:-1]])           # the first index of every run
    anchors = []
    for s in np.flatnonzero(first).tolist():
        anchors.append(0 if m[s] == 0 else int(x[s - 1]))            # no aligned base in front: POS
    an = np.array([a for a in anchors if a < span], dtype=np.int64)
    return pos + x[al], seq[al], pos + dl, pos + an


# ---- model (b): the SAM text ---------------------------------------------------------------------------------------------------
def reads_b(sam: bytes, names=None):
    """Per mapped alignment line: dict(contig, pos, span, flag, al, bases, dl, an) from POS, CIGAR and SEQ alone."""
    given, names, out = names is not None, list(names or []), []
    for ln in sam.split(b"\n"):
        if ln.startswith(b"@SQ") and not given:
            names.append(dict(x.split(b":", 1) for x in ln.split(b"\t")[1:])[b"SN"])
        if not ln or ln.startswith(b"@"):
            continue
        c = ln.split(b"\t")
        if int(c[1]) & 4:
            continue
        pos, seq = int(c[3]), np.frombuffer(c[9], dtype=np.uint8)
        rp, q, last, run = pos, 0, None, False
        al, idx, dl, an = [], [], [], []
        for n, op in _CIGAR.findall(c[5]):
            n = int(n)
            if op in b"M=X":
                al += range(rp, rp + n); idx += range(q, q + n); rp += n; q += n; last = rp - 1; run = False
            elif op in b"IS":
                if not run:
                    an.append(pos if last is None else last)
                run = True; q += n
            elif op in b"DN":
                dl += range(rp, rp + n); rp += n
        out.append(dict(contig=names.index(c[2]), pos=pos, span=rp - pos, flag=int(c[1]), al=np.array(al, dtype=np.int64),
                        bases=seq[np.array(idx, dtype=np.int64)] if idx else seq[:0], dl=np.array(dl, dtype=np.int64),
                        an=np.array(an, dtype=np.int64)))
    return out


# ---- reads -> tables -> text ---------------------------------------------------------------------------------------------------
def tables(reads, contig, beg, end, exclude=0, skip_blocks=(), a=True):
    """cnt[5][W], del[W], ins[W] of positions beg..end of `contig` and the reads kept (the keep rule of the depth)."""
    W = end - beg + 1
    cnt, dl, ins, kept = np.zeros((5, W), dtype=np.int64), np.zeros(W, dtype=np.int64), np.zeros(W, dtype=np.int64), 0
    P, B, D, I = [], [], [], []
    for rd in reads:
        if rd["contig"] != contig or rd["span"] < 1 or rd["flag"] & exclude or rd["pos"] > end or rd["pos"] + rd["span"] - 1 < beg:
            continue
        if a and rd["block"] in skip_blocks:
            continue
        kept += 1
        p, b, d, i = events_a(rd) if a else (rd["al"], rd["bases"], rd["dl"], rd["an"])
        P.append(p); B.append(b); D.append(d); I.append(i)
    if kept:
        p, b = np.concatenate(P), np.concatenate(B)
        w = (p >= beg) & (p <= end)
        np.add.at(cnt, (klass(b[w]), p[w] - beg), 1)
        for arr, src in ((dl, np.concatenate(D)), (ins, np.concatenate(I))):
            src = src[(src >= beg) & (src <= end)]
            np.add.at(arr, src - beg, 1)
    return cnt, dl, ins, kept


def text_of(name: bytes, beg, ref, cnt, dl, ins, min_alt=1):
    """The lines of the positions with nonref >= min_alt, in Python integers.  ref: the reference bytes of beg..end.
    Returns (bytes, lines)."""
    depth = cnt.sum(axis=0) + dl
    same = cnt[klass(ref), np.arange(len(ref))]
    nonref = depth - same + ins
    out = []
    for i in np.flatnonzero(nonref >= min_alt).tolist():
        out.append(b"%s\t%d\t%c\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (name, beg + i, int(ref[i]), int(depth[i]), int(cnt[0, i]), int(cnt[1, i]),
                                                                   int(cnt[2, i]), int(cnt[3, i]), int(cnt[4, i]), int(dl[i]), int(ins[i])))
    return b"".join(out), len(out)


def contig_ref(pb, c):
    """The reference bytes of contig c as the packer lays them out: what is uploaded."""
    o, n = int(pb.contigs[c]["ref_off"]), int(pb.contigs[c]["length"])
    return pb.ref[o:o + n]


def expected(pb, reads, names, lens, region=None, exclude=0, min_alt=1, skip_blocks=(), a=True):
    """The text of the whole container (every contig in table order) or of region = (contig, beg, end).
    Returns (bytes, lines, reads kept)."""
    calls = [region] if region is not None else [(c, 1, lens[c]) for c in range(len(names))]
    out, lines, kept = [], 0, 0
    for c, beg, end in calls:
        cnt, dl, ins, k = tables(reads, c, beg, end, exclude, skip_blocks, a)
        t, n = text_of(names[c], beg, contig_ref(pb, c)[beg - 1:end], cnt, dl, ins, min_alt)
        out.append(t); lines += n; kept += k
    return b"".join(out), lines, kept


def assert_models_agree(pb, sam, names, lens):
    """On input without soft clips (and without reads whose edits cancel) the two models give the same tables on every contig
    and the same interval for every read; a dataset where they do not is the wrong dataset for a test that lets either stand as
    ground truth.  Returns model (a)'s reads."""
    ra, rb = reads_a(pb), reads_b(sam, names)
    assert len(ra) == len(rb)
    bad = [i for i, (x, y) in enumerate(zip(ra, rb)) if (x["contig"], x["pos"], x["span"], x["flag"]) != (y["contig"], y["pos"], y["span"], y["flag"])]
    assert not bad, "models (a) and (b) differ on %d reads, first: %d" % (len(bad), bad[0])
    for c in range(len(names)):
        ta, tb = tables(ra, c, 1, lens[c]), tables(rb, c, 1, lens[c], a=False)
        for x, y in zip(ta[:3], tb[:3]):
            assert np.array_equal(x, y), "the tables of the two models differ on contig %d" % c
        assert ta[3] == tb[3]
    return ra


def parse(text: bytes):
    """[(name, pos1, ref, depth, A, C, G, T, N, del, ins)] of text written by the code under test."""
    assert text == b"" or text.endswith(b"\n")
    out = []
    for ln in text.split(b"\n")[:-1]:
        c = ln.split(b"\t")
        assert len(c) == 11 and len(c[2]) == 1, ln
        out.append((c[0], int(c[1]), c[2]) + tuple(int(x) for x in c[3:]))
    return out


# ---- datasets ------------------------------------------------------------------------------------------------------------------
def shared(seed=5, n=600, block_reads=64):
    """Shared variant sites (every covering read carries the alternative base), independent errors, and eight indel reads laid
    over the same sites.  Returns (fasta, sam, packed batch, contigs)."""
    fa, body = synth.shared_variant_dataset(seed, 20_000, n, 100, site_every=50, err=0.005, indel_sites=8)
    contig = np.frombuffer(b"".join(fa.split(b"\n")[1:]), dtype=np.uint8)
    sam = b"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:c\tLN:%d\n" % len(contig) + body
    return fa, sam, host.pack_sam(sam, fa, block_reads=block_reads, var_length=True), [("c", contig)]


def windows(pb, reads, lens, n_random, seed):
    """(region string, contig, beg, end): random windows, windows that start and end inside a read with indels, inside its
    deleted bases and on its insertion's anchor, and the contigs' edges."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_random):
        c = int(rng.integers(0, len(lens)))
        beg = int(rng.integers(1, lens[c] + 1))
        out.append((c, beg, min(lens[c], beg + int(rng.choice([0, 1, 50, 300, 2000, 20000])))))
    for rd in [r for r in reads if len(r["dc"])][:3]:
        d = rd["pos"] + int(rd["dc"][0])
        out += [(rd["contig"], d, d), (rd["contig"], rd["pos"] + 3, d), (rd["contig"], d, rd["pos"] + rd["span"] + 5)]
    for rd in [r for r in reads if len(r["oi"]) and r["oi"][0] > 0][:3]:
        a = rd["pos"] + int(rd["oi"][0]) - 1 + int((rd["dc"] <= rd["oi"][0] - 1).sum())
        out += [(rd["contig"], a, a), (rd["contig"], a + 1, a + 40), (rd["contig"], max(1, a - 30), a)]
    for c, L in enumerate(lens):
        out += [(c, 1, 1), (c, L, L), (c, 1, L)]
    names = [pb.names[int(pb.contigs[c]["name_off"]):].tobytes().split(b"\0")[0].decode() for c in range(len(lens))]
    return [("%s:%d-%d" % (names[c], b, e), c, b, e) for c, b, e in out]


# ---- the emulation library -----------------------------------------------------------------------------------------------------
def emu_load(path):
    L = ctypes.CDLL(path)
    L.emu_pileup_decode.restype = ctypes.c_int
    L.emu_pileup_decode.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    L.emu_pileup.restype = ctypes.c_int
    L.emu_pileup.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                             ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p,
                             ctypes.c_uint64, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64,
                             ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    return L


def emu_decode(L, plan, b0, b1, smax, per_read=16):
    """Blocks [b0, b1) laid out from 0 (as cbc_gpu_decode_pileup does) and decoded by the emulated edit-reporting decoder; side
    array and arena at exactly their sizes.  Returns (blocks, recs, rows, results, records, side, arena)."""
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
    assert L.emu_pileup_decode(ctypes.byref(db), smax, per_read, side.ctypes.data, arena.ctypes.data) == 0
    return bl, recs, seq, res, nrec, side, arena


def emu_call(L, plan, sel, exclude=0, min_alt=1, per_read=16, cap=None, fail_blocks=(), dec=None, n_waves=4):
    """One cbc_gpu_decode_pileup on the emulation: edits decode of the selection, then every pass.  Returns (rc, text, lines,
    reads kept, text bytes, decode results); the guard bytes behind the text (all of it when nothing may be written) must be
    untouched.  fail_blocks: blocks of the selection whose decode status is set to a failure before the passes run."""
    if sel.b1 == sel.b0:
        return 0, b"", 0, 0, 0, np.zeros(0, dtype=host.RESULT_DTYPE)
    bl, recs, seq, res, nrec, side, arena = dec if dec is not None else emu_decode(L, plan, sel.b0, sel.b1, sel.smax, per_read)
    res = res.copy()
    for b in fail_blocks:
        res[b]["status"] = 2
    ws = np.ascontiguousarray(plan.window_start[sel.b0:sel.b1], dtype=np.uint64)
    off = int(plan.contig_name_off[sel.contig])
    name = plan.names[off:].tobytes().split(b"\0", 1)[0]
    cap = plan.pileup_text_cap(sel.b0, sel.b1, sel.contig, sel.beg, sel.end, sel.smax) if cap is None else cap
    text = np.full(cap + 16, 0xEE, dtype=np.uint8)
    out = np.zeros(4, dtype=np.uint64)
    c0 = int(plan.blocks[sel.b0]["ref_off"]) - int(ws[0])
    rc = L.emu_pileup(recs.ctypes.data, nrec, seq.ctypes.data, seq.size, bl.ctypes.data, ws.ctypes.data, res.ctypes.data,
                      sel.b1 - sel.b0, side.ctypes.data, arena.ctypes.data, per_read, plan.ref.ctypes.data, len(plan.ref), c0,
                      name, len(name), sel.beg, sel.end, exclude, min_alt, n_waves, text.ctypes.data, cap, out.ctypes.data)
    total = int(out[0])
    wrote = rc in (0, -4)
    assert (text[total if wrote else 0:] == 0xEE).all(), "bytes written outside the text"
    return rc, (text[:total].tobytes() if wrote else b""), int(out[1]), int(out[2]), total, res


def emu_whole(L, plan, exclude=0, min_alt=1):
    """Every contig that has blocks, in table order, texts appended: what `cbc -x --pileup` does."""
    text, lines, kept = [], 0, 0
    for c in range(plan.n_contigs):
        rc, t, n, k, _, _ = emu_call(L, plan, plan.contig_blocks(c), exclude, min_alt)
        assert rc == 0
        text.append(t); lines += n; kept += k
    return b"".join(text), lines, kept
