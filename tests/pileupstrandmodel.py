"""Per-strand counts and the minimum alternative fraction of the pileup in plain Python: what
`cbc -x --pileup --by-strand --min-alt-frac F` must write.  No alignment logic of its own: the totals are
pileupmodel.tables(..., exclude=E), the plus tables pileupmodel.tables(..., exclude=E | 16), the line rule is the two inequalities
in Python integers, and the text is pileupmodel.text_of's line, widened.  Also the conditions the tests' datasets must meet, and
the ctypes wrapper of the emulation library (tests/pileup_strand_emu)."""
import ctypes

import numpy as np

import pileupmodel as pm
from cbc_amd import host


def rule(nonref, depth, min_alt=1, ppm=0):
    """nonref >= K and nonref * 10^6 >= ppm * depth, in Python integers."""
    return nonref >= min_alt and nonref * 1_000_000 >= ppm * depth


def text_of(name: bytes, beg, ref, tot, plus, min_alt=1, ppm=0, by_strand=False):
    """tot, plus: (cnt[5][W], del[W], ins[W]) of every kept read and of the kept forward reads.  Returns (bytes, lines)."""
    cnt, dl, ins = tot
    depth = cnt.sum(axis=0) + dl
    same = cnt[pm.klass(ref), np.arange(len(ref))]
    nonref = depth - same + ins
    out = []
    for i in range(len(ref)):
        if not rule(int(nonref[i]), int(depth[i]), min_alt, ppm):
            continue
        cols = [int(depth[i])] + [int(cnt[k, i]) for k in range(5)] + [int(dl[i]), int(ins[i])]
        if by_strand:
            cols += [int(plus[0][k, i]) for k in range(5)] + [int(plus[1][i]), int(plus[2][i])]
        out.append(b"%s\t%d\t%c\t" % (name, beg + i, int(ref[i])) + b"\t".join(b"%d" % x for x in cols) + b"\n")
    return b"".join(out), len(out)


def expected(pb, reads, names, lens, region=None, exclude=0, min_alt=1, ppm=0, by_strand=False, skip_blocks=()):
    """The text of the whole container (every contig in table order) or of region = (contig, beg, end).
    Returns (bytes, lines, reads kept)."""
    calls = [region] if region is not None else [(c, 1, lens[c]) for c in range(len(names))]
    out, lines, kept = [], 0, 0
    for c, beg, end in calls:
        tot = pm.tables(reads, c, beg, end, exclude, skip_blocks)
        plus = pm.tables(reads, c, beg, end, exclude | 16, skip_blocks)
        t, n = text_of(names[c], beg, pm.contig_ref(pb, c)[beg - 1:end], tot[:3], plus[:3], min_alt, ppm, by_strand)
        out.append(t); lines += n; kept += tot[3]
    return b"".join(out), lines, kept


def parse(text: bytes):
    """[(name, pos1, ref, depth, A, C, G, T, N, del, ins, A+, C+, G+, T+, N+, del+, ins+)] of text written by the code under test."""
    assert text == b"" or text.endswith(b"\n")
    out = []
    for ln in text.split(b"\n")[:-1]:
        c = ln.split(b"\t")
        assert len(c) == 18 and len(c[2]) == 1, ln
        out.append((c[0], int(c[1]), c[2]) + tuple(int(x) for x in c[3:]))
    return out


def first_eleven(text: bytes) -> bytes:
    """The lines of a by-strand text cut back to their first eleven columns."""
    return b"".join(b"\t".join(ln.split(b"\t")[:11]) + b"\n" for ln in text.split(b"\n")[:-1])


def passing(text: bytes, min_alt, ppm) -> bytes:
    """The lines of a pileup text (eleven or eighteen columns) that pass the rule, computed from their own columns."""
    out = []
    for ln in text.split(b"\n")[:-1]:
        c = ln.split(b"\t")
        depth, cnt, ins = int(c[3]), [int(x) for x in c[4:9]], int(c[10])
        if rule(depth - cnt[int(pm.klass(c[2][0]))] + ins, depth, min_alt, ppm):
            out.append(ln + b"\n")
    return b"".join(out)


# ---- datasets ------------------------------------------------------------------------------------------------------------------
def assert_both_strands(pb, reads, names, lens, exclude=0, min_both=20):
    """The conditions a dataset must meet before a by-strand test relies on it: at least 20 % of its kept reads on each strand,
    and at least min_both reported positions where both strands show a non-reference observation.  Returns that number."""
    kept = [r for r in reads if r["span"] >= 1 and not r["flag"] & exclude]
    fwd = sum(1 for r in kept if not r["flag"] & 16)
    assert kept and 0.2 * len(kept) <= fwd <= 0.8 * len(kept), (fwd, len(kept))
    both = 0
    for c in range(len(names)):
        ref = pm.contig_ref(pb, c)[:lens[c]]
        cls = pm.klass(ref)
        nr = []
        for ex in (exclude, exclude | 16):
            cnt, dl, ins, _ = pm.tables(reads, c, 1, lens[c], ex)
            depth = cnt.sum(axis=0) + dl
            nr.append(depth - cnt[cls, np.arange(len(ref))] + ins)
        both += int(((nr[1] >= 1) & (nr[0] - nr[1] >= 1)).sum())
    assert both >= min_both, both
    return both


# ---- the emulation library -----------------------------------------------------------------------------------------------------
def emu_load(path):
    L = ctypes.CDLL(path)
    L.emu_pileup_ext.restype = ctypes.c_int
    L.emu_pileup_ext.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                 ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p,
                                 ctypes.c_uint64, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64,
                                 ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                 ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    return L


def emu_call(L, Ldec, plan, sel, exclude=0, min_alt=1, ppm=0, by_strand=False, per_read=16, cap=None, fail_blocks=(), dec=None, n_waves=4):
    """One cbc_gpu_decode_pileup_ext on the emulation: the edits decode of the selection by tests/pileup_emu's library Ldec (or
    `dec`, an earlier one), then every pass.  Returns (rc, text, lines, reads kept, text bytes); the guard bytes behind the text
    (all of it when nothing may be written) must be untouched."""
    if sel.b1 == sel.b0:
        return 0, b"", 0, 0, 0
    bl, recs, seq, res, nrec, side, arena = dec if dec is not None else pm.emu_decode(Ldec, plan, sel.b0, sel.b1, sel.smax, per_read)
    res = res.copy()
    for b in fail_blocks:
        res[b]["status"] = 2
    ws = np.ascontiguousarray(plan.window_start[sel.b0:sel.b1], dtype=np.uint64)
    off = int(plan.contig_name_off[sel.contig])
    name = plan.names[off:].tobytes().split(b"\0", 1)[0]
    cap = plan.pileup_text_cap(sel.b0, sel.b1, sel.contig, sel.beg, sel.end, sel.smax, by_strand) if cap is None else cap
    text = np.full(cap + 16, 0xEE, dtype=np.uint8)
    out = np.zeros(4, dtype=np.uint64)
    c0 = int(plan.blocks[sel.b0]["ref_off"]) - int(ws[0])
    rc = L.emu_pileup_ext(recs.ctypes.data, nrec, seq.ctypes.data, seq.size, bl.ctypes.data, ws.ctypes.data, res.ctypes.data,
                          sel.b1 - sel.b0, side.ctypes.data, arena.ctypes.data, per_read, plan.ref.ctypes.data, len(plan.ref), c0,
                          name, len(name), sel.beg, sel.end, exclude, min_alt, ppm, int(bool(by_strand)), n_waves, 0, 0,
                          text.ctypes.data, cap, out.ctypes.data)
    total = int(out[0])
    wrote = rc in (0, -4)
    assert (text[total if wrote else 0:] == 0xEE).all(), "bytes written outside the text"
    return rc, (text[:total].tobytes() if wrote else b""), int(out[1]), int(out[2]), total


def emu_whole(L, Ldec, plan, exclude=0, min_alt=1, ppm=0, by_strand=False, decs=None):
    """Every contig that has blocks, in table order, texts appended: what `cbc -x --pileup` does.  decs: a dict that keeps every
    contig's decode for the next call."""
    text, lines, kept = [], 0, 0
    for c in range(plan.n_contigs):
        sel = plan.contig_blocks(c)
        dec = None
        if decs is not None and sel.b1 > sel.b0:
            if c not in decs:
                decs[c] = pm.emu_decode(Ldec, plan, sel.b0, sel.b1, sel.smax, 16)
            dec = decs[c]
        rc, t, n, k, _ = emu_call(L, Ldec, plan, sel, exclude, min_alt, ppm, by_strand, dec=dec)
        assert rc == 0
        text.append(t); lines += n; kept += k
    return b"".join(text), lines, kept
