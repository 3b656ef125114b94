"""Exact inputs for the long-read format (stream version 3): every read is given as POS, FLAG and a list of
CIGAR runs with the mismatches of its M runs, over a seeded random ACGT contig, so that a case reaches the threshold it is named
for -- a model's rescale point, a run or gap or edit count at a limit of the kernel -- by construction and not by chance.

build() returns the FASTA and SAM texts, the expected read text and, per read, the edit list (gap, kind, prev_kind, strand) as the
format defines it (oracle/cbc_long.c), derived here from the construction alone: the tests assert from it that a case really
reaches what it claims, before any codec sees it.  The named builders below are shared by tests/test_long_edges.py (CPU
emulation against the CPU statement) and tests/test_long_edges_gpu.py (the HIP kernels)."""
import collections

import numpy as np

NAME = b"chrL"
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_N = ord("N")
_CODE = np.zeros(256, dtype=np.int64)
for _k, _c in enumerate(b"ACGT"):
    _CODE[_c] = _k
RESCALE = 1 << 20                                   # stream_model.c: a model halves its counts when its total reaches this
EDIT_HALF, EDIT_CAP = 4096, 8192                    # CBC_LONG_EDIT_HALF, CBC_LONG_EDIT_CAP (cbc_long_body.h)

Case = collections.namedtuple("Case", "fasta sam text edits pos flag rlen")


def uses_to_rescale(card, step, init=1):
    """Uses after which a model of `card` symbols (initial count `init`) reaches the rescale point for the first time."""
    return -(-(RESCALE - card * init) // step)


def contig(seed, length, n_stretches=()):
    c = _ACGT[np.random.default_rng(seed).integers(0, 4, size=length)]
    for s, l in n_stretches:
        c[s:s + l] = _N
    return c


def fasta(c, name=NAME, width=60):
    full = len(c) // width
    body = np.empty((full, width + 1), dtype=np.uint8)
    body[:, :width] = c[:full * width].reshape(full, width)
    body[:, width] = 10
    tail = c[full * width:].tobytes()
    return b">" + name + b"\n" + body.tobytes() + (tail + b"\n" if tail else b"")


def _one(c, rng, pos, flag, ops):
    """One read.  ops: (op, len) or (op, len, extra) with op in M I D S; extra of an M run = the offsets of its mismatches, or
    (offsets, bases) to name the read's bases there; extra of an I / S run = its bases (default: random ACGT)."""
    n = len(ops)
    op = np.array([b"MIDS".index(o[0].encode()) for o in ops])
    ln = np.array([o[1] for o in ops], dtype=np.int64)
    assert n and (ln > 0).all()
    isM, isI, isD = op == 0, (op == 1) | (op == 3), op == 2
    di, dj, dm = np.where(isM | isI, ln, 0), np.where(isM | isD, ln, 0), np.where(isM, ln, 0)
    i0, j0, m0 = np.cumsum(di) - di, np.cumsum(dj) - dj + (pos - 1), np.cumsum(dm) - dm
    rl = int(di.sum())
    assert pos >= 1 and j0[-1] + dj[-1] <= len(c), "the read runs off the contig"
    run = np.repeat(np.arange(n), di)                              # the run of every read base
    off = np.arange(rl) - i0[run]
    in_m = isM[run]
    seq = np.empty(rl, dtype=np.uint8)
    seq[in_m] = c[(j0[run] + off)[in_m]]
    seq[~in_m] = _ACGT[rng.integers(0, 4, size=int((~in_m).sum()))]
    s_run, s_off = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)]
    for r, o in enumerate(ops):
        if len(o) < 3 or o[2] is None:
            continue
        if isM[r]:
            offs, bases = o[2] if isinstance(o[2], tuple) else (o[2], None)
            offs = np.asarray(offs, dtype=np.int64)
            assert offs.size == 0 or (offs[0] >= 0 and offs[-1] < ln[r] and (np.diff(offs) > 0).all())
            refb = c[j0[r] + offs]
            new = _ACGT[(_CODE[refb] + rng.integers(1, 4, size=offs.size)) % 4] if bases is None else np.frombuffer(bases, dtype=np.uint8)
            assert (new != refb).all()                             # for an N in the reference any of C, G, T
            seq[i0[r] + offs] = new
            s_run.append(np.full(offs.size, r, dtype=np.int64)); s_off.append(offs)
        else:
            assert isI[r] and len(o[2]) == ln[r]
            seq[i0[r]:i0[r] + ln[r]] = np.frombuffer(o[2], dtype=np.uint8)
    # the edits in read order: (run, offset inside the run) sorts them; M coordinate = matched-or-substituted bases in front
    ind = isI | isD
    x_run = np.repeat(np.arange(n)[ind], ln[ind])
    x_off = np.arange(x_run.size) - np.repeat(np.cumsum(ln[ind]) - ln[ind], ln[ind])
    e_run, e_off = np.concatenate(s_run + [x_run]), np.concatenate(s_off + [x_off])
    order = np.lexsort((e_off, e_run))
    e_run, e_off = e_run[order], e_off[order]
    kind = np.where(isM[e_run], 0, np.where(isI[e_run], 1, 2))
    mc = m0[e_run] + np.where(kind == 0, e_off, 0)
    mend = mc + (kind == 0)
    ed = np.zeros((kind.size, 4), dtype=np.int64)
    ed[:, 0] = mc - np.concatenate([[0], mend[:-1]])
    ed[:, 1] = kind
    ed[:, 2] = np.concatenate([[3], kind[:-1]])
    ed[:, 3] = (flag >> 4) & 1
    assert (ed[:, 0] >= 0).all()
    return seq, ed, "".join("%d%s" % (o[1], o[0]) for o in ops).encode()


def build(c, reads, seed=1, name=NAME):
    """reads: [(pos, flag, ops)] in POS order.  Returns a Case: FASTA text, SAM text, the reads one per line, the edit lists
    (one int64 array [n_edits, 4] per read: gap, kind, prev_kind, strand), and POS / FLAG / length per read."""
    rng = np.random.default_rng(seed)
    lines, texts, edits, lens = [], [], [], []
    assert all(a[0] <= b[0] for a, b in zip(reads, reads[1:])), "reads in POS order"
    for k, (pos, flag, ops) in enumerate(reads):
        seq, ed, cigar = _one(c, rng, pos, flag, ops)
        s = seq.tobytes()
        lines.append(b"r%d\t%d\t%s\t%d\t60\t%s\t*\t0\t0\t%s\t*\n" % (k, flag, name, pos, cigar, s))
        texts.append(s + b"\n"); edits.append(ed); lens.append(len(s))
    hdr = b"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:%s\tLN:%d\n" % (name, len(c))
    return Case(fasta(c, name), hdr + b"".join(lines), b"".join(texts), edits,
                [r[0] for r in reads], [r[1] for r in reads], lens)


def concat(cases):
    """Cases over the SAME contig as one input, reads in POS order (stable)."""
    assert all(x.fasta == cases[0].fasta for x in cases)
    rows = []
    for x in cases:
        body = [ln + b"\n" for ln in x.sam.split(b"\n") if ln and not ln.startswith(b"@")]
        rows += list(zip(x.pos, body, x.text.splitlines(keepends=True), x.edits, x.flag, x.rlen))
    rows.sort(key=lambda t: t[0])
    hdr = b"".join(ln + b"\n" for ln in cases[0].sam.split(b"\n") if ln.startswith(b"@"))
    return Case(cases[0].fasta, hdr + b"".join(t[1] for t in rows), b"".join(t[2] for t in rows), [t[3] for t in rows],
                [t[0] for t in rows], [t[4] for t in rows], [t[5] for t in rows])


# ------------------------------------------------------------------------------------------------ the rescale cases
def _rescale_gaps(rng, n):
    """~98.5 % in 1..2, 1 % in 3..63, 0.45 % in 64..254, 0.05 % in 255..399: both halves of a gap table (symbols 0..63 in LDS,
    64..255 in global memory) hold odd counts when it is halved, and some batches carry the two gx bytes."""
    u = rng.random(n)
    g = rng.integers(1, 3, size=n)
    g = np.where(u >= 0.985, rng.integers(3, 64, size=n), g)
    g = np.where(u >= 0.995, rng.integers(64, 255, size=n), g)
    g = np.where(u >= 0.9995, rng.integers(255, 400, size=n), g)
    return g


def _rescale(kind, flag, seed, n_reads=12, rl=60_000):
    """One block of n_reads x rl bases whose edits are almost all of `kind` on one strand: the gap context 2 * kind + strand,
    kindm[kind] and (insertions) chars row 5 pass their rescale points."""
    rng = np.random.default_rng(seed)
    c = contig(seed + 1000, 200_000)
    reads = []
    for r in range(n_reads):
        gaps = _rescale_gaps(rng, rl)
        kinds = np.where(rng.random(rl) < 0.996, kind, (kind + rng.integers(1, 3, size=rl)) % 3)
        ops, mlen, mm, used = [], 0, [], 0                 # the open M run, its mismatches, read bases so far
        for g, k in zip(gaps.tolist(), kinds.tolist()):
            if used + g + (k != 2) + 1 > rl:
                break
            mlen += g; used += g + (k != 2)
            if k == 0:
                mm.append(mlen); mlen += 1
            else:
                ops.append(("M", mlen, mm or None)); mlen, mm = 0, []
                ops.append(("I" if k == 1 else "D", 1))
        ops.append(("M", mlen + rl - used, mm or None))
        reads.append((1 + 997 * r, flag, ops))
    return build(c, reads, seed)


def rescale_sub():
    return _rescale(0, 0, 101)


def rescale_ins():
    return _rescale(1, 16, 102)


def rescale_del():
    return _rescale(2, 0, 103)


# ------------------------------------------------------------------------------------------------ the threshold cases
_C100K = None


def _c100k():
    global _C100K
    if _C100K is None:
        _C100K = contig(7, 100_000)
    return _C100K


def runs():
    """I / S / D runs of 64, 65 and far beyond (the lane-per-run walk takes <= 64, the fallback the rest, the read window moves in
    256-byte chunks), M runs of 256 / 257 / 5000 with mismatches at 0, 255, 256 and the last base; both strands."""
    a = [("S", 200), ("M", 256, [0, 255]), ("I", 64), ("M", 257, [0, 255, 256]), ("D", 64), ("M", 5000, [0, 255, 256, 4999]),
         ("I", 65), ("M", 300), ("D", 65), ("M", 256, [255]), ("I", 300), ("M", 100), ("D", 300), ("M", 100, [99]),
         ("I", 1000), ("M", 50), ("S", 700)]
    b = [("S", 200), ("M", 5000, [0, 255, 256, 4999]), ("D", 300), ("M", 257, [256]), ("I", 1000), ("M", 256, [0, 255]),
         ("D", 65), ("M", 64), ("I", 65), ("M", 65, [64]), ("D", 64), ("M", 1), ("I", 64), ("M", 256), ("I", 300), ("M", 257, [0]),
         ("S", 700)]
    short = [("M", 256, [0, 255]), ("I", 64), ("M", 256, [255]), ("D", 64), ("M", 40)]        # all of it in the lane form
    i65 = [("M", 100), ("I", 65), ("M", 100, [50])]                                          # 65 and nothing longer: the whole read falls back
    d65 = [("M", 100, [99]), ("D", 65), ("M", 100)]
    return build(_c100k(), [(400, 0, i65), (500, 16, d65), (1000, 0, a), (1500, 16, b), (3000, 16, a), (3000, 0, b), (9000, 0, short),
                            (9100, 16, short)], 11)


GAPS = [0, 1, 62, 63, 64, 65, 254, 255, 256, 509, 510, 511, 65533]


def gaps():
    """One read per gap g: a single mismatch after g matches (63 / 64: LDS or global half of the table; 254 / 255 / 256: the
    escape and gx (0, 0), (0, 1); 510 / 511: the gx high byte; 65533); a 65535-base read without an edit; one with its only
    edit at base 65534."""
    c = contig(8, 300_000)
    reads = [(100 + 50 * k, 16 * (k & 1), [("M", min(g + 21, 65535), [g])]) for k, g in enumerate(GAPS)]
    reads.append((5000, 0, [("M", 65535)]))
    reads.append((6000, 16, [("M", 65535, [65534])]))
    return build(c, reads, 12)


COUNTS = [63, 64, 65, 4095, 4096, 4097, 8191, 8192, 8193, 65535]
COUNTS_LANE = [4095, 4096, 4097]


def counts():
    """Reads with exactly n edits for n around a batch (64), a half of the edit buffer (4096), the buffer (8192) and the u16
    limit of the stream (65535); strands alternate.  The 4097-edit read is the block's second: its half of the edit buffer is the
    last thing in the block's scratch.  One M run each (beyond 124 edits it is longer than 256 bases: the run-by-run walk); the
    reads of COUNTS_LANE reach 4095 / 4096 / 4097 edits in runs the lane-per-run walk takes (M 128 with 63 mismatches + D 1 = 64
    edits a pair, 32 pairs a step), so that walk meets a half that is exactly full."""
    order = [4096, 4097, 63, 64, 65, 4095, 8191, 8192, 8193, 65535]
    reads = []
    for k, n in enumerate(order):
        if n < 65535:
            ops = [("M", 2 * n + 7, np.arange(n) * 2 + 1)]
        else:
            ops = [("M", 50_000, np.arange(25_000) * 2), ("D", 30_535), ("I", 10_000), ("M", 10)]
        reads.append((10 + 300 * k, 16 * (k & 1), ops))
    for k, n in enumerate(COUNTS_LANE):
        ops = []
        for q in range(63):
            ops += [("M", 128, np.arange(63) * 2 + 1), ("D", 1)]
        ops += [("M", 128, np.arange(min(n - 4033, 63)) * 2 + 1), ("D", 1), ("M", 20, [7] if n == 4097 else None)]     # 62, 63, 63 (+ 1)
        reads.append((5000 + 300 * k, 16 * (k & 1), ops))
    return build(_c100k(), reads, 13)


NCIG = [63, 64, 65, 127, 128, 129]


def ncig():
    """CIGARs of exactly n runs for n around the 64 runs a step of the walk takes; M / I / D inside, S at both ends."""
    reads = []
    for k, n in enumerate(NCIG):
        inner = n - 2 if n % 2 else n - 1                  # M x M y ... M between the clips: an odd count; an even n has no end clip
        ops = [("S", 5)]
        for q in range(inner):
            ops.append(("M", 20 + (q % 7), [3] if q % 4 == 0 else None) if q % 2 == 0 else (("I", 1 + q % 3) if q % 4 == 1 else ("D", 1 + q % 5)))
        if n % 2:
            ops.append(("S", 9))
        assert len(ops) == n
        reads.append((20_000 + 100 * k, 16 * (k & 1), ops))
    return build(_c100k(), reads, 14)


def ends():
    """Reads at POS 1, and reads whose last M, I and D run end on the contig's last base (behind it: the reference pad only)."""
    c = _c100k(); L = len(c)
    reads = [(1, 0, [("M", 300, [0, 299])]), (1, 16, [("S", 10), ("M", 500, [0])]), (1, 0, [("D", 3), ("M", 100)]),
             (L - 999, 0, [("M", 1000, [0, 999])]),                             # the last M base is the contig's last, a mismatch
             (L - 699, 16, [("M", 700), ("I", 5)]),                             # an insertion behind the last base
             (L - 399, 0, [("M", 300, [299]), ("D", 100)]),                     # a deletion of the last 100 bases
             (L - 64, 16, [("M", 65)]), (L, 0, [("M", 1, [0])])]
    return build(c, reads, 15)


def lists():
    """One block of 64 reads with 64 distinct lengths, 64 distinct FLAGs and 64 distinct POS steps: the sparse per-read lists
    (len, ne), the FLAG pairs and the pos alphabet at what a block can hold."""
    reads, pos = [], 500
    for k in range(64):
        pos += 3 + k                                      # steps 4 .. 67 after the block's first read: all distinct
        flag = (k & 1) * 16 | (k >> 1) << 5               # 64 values, bit 2 (unmapped) clear, both strands
        reads.append((pos, flag, [("M", 300 + 257 * k, [k, 299 + k] if k % 3 else None)]))   # lengths differ in both bytes
    return build(_c100k(), reads, 16)


def big_step():
    """A contig of ~17 Mbases and a POS step of 2^24 and more inside one block: all four bytes of the pos escape."""
    c = contig(9, 17_000_000)
    reads = [(5, 0, [("M", 200, [7])]), (5 + (1 << 24) + 77, 16, [("M", 150), ("I", 2), ("M", 100, [99])]),
             (5 + (1 << 24) + 77, 0, [("M", 90)])]
    return build(c, reads, 17)


def n_bases():
    """N runs in the reference under M runs (N over N matches: the compare is by byte), N in the read over ACGT (a substitution
    to symbol 4), concrete bases over N (chars row 4), inserted N."""
    c = contig(10, 50_000, n_stretches=[(1000, 300), (5000, 64), (5100, 1), (9000, 2000)])
    def at(p, l):                                         # the contig's bases [p, p + l) (0-based) as a read would match them
        return c[p:p + l]
    reads = []
    # N over N: the read takes the reference's N
    reads.append((901, 0, [("M", 600)]))
    # concrete bases over the reference's N run: 300 substitutions in row 4
    reads.append((951, 16, [("M", 500, np.arange(50, 350))]))
    # N in the read over ACGT, next to N over N
    reads.append((4901, 0, [("M", 300, ([10, 20, 98, 170, 250], b"NNNNN"))]))
    # inserted N, clipped N
    reads.append((4951, 16, [("S", 4, b"NNNN"), ("M", 100), ("I", 3, b"NAN"), ("M", 200, ([20], b"N")), ("I", 70, b"N" * 70), ("M", 30)]))
    # a read inside the long N run, a deletion of N
    reads.append((9501, 0, [("M", 400), ("D", 10), ("M", 400, [5])]))
    assert (at(900, 600) == _N).sum() == 300
    return build(c, reads, 18)


def too_many_edits(n_del=5536):
    """`10M <n_del>D 60000I 10M` between two healthy reads, and three more healthy reads behind them (packed with block_reads=3:
    a second block).  5536: 65536 edits, one more than the stream's u16 holds -- the first block is refused at that read.
    5535: 65535 edits, legal."""
    ok = [("M", 400, [17, 200])]
    reads = [(100, 0, ok), (200, 16, [("M", 10), ("D", n_del), ("I", 60_000), ("M", 10)]), (300, 0, ok),
             (7000, 16, ok), (7100, 0, [("M", 300), ("I", 2), ("M", 98)]), (7200, 16, ok)]
    return build(_c100k(), reads, 19)


_BUILDERS = dict(rescale_sub=rescale_sub, rescale_ins=rescale_ins, rescale_del=rescale_del, runs=runs, gaps=gaps, counts=counts,
                 ncig=ncig, ends=ends, lists=lists, big_step=big_step, n_bases=n_bases)
NAMES = list(_BUILDERS)
_cache = {}


def case(name):
    """The named case, built once per process."""
    if name not in _cache:
        _cache[name] = _BUILDERS[name]()
    return _cache[name]


def context_uses(c):
    """From the edit lists alone: uses of every gap context 2 * prev_kind + strand, of every kind context, of chars row 5
    (inserted bases); gap symbols >= 64 and gaps >= 255 among them."""
    e = np.concatenate(c.edits) if c.edits else np.zeros((0, 4), dtype=np.int64)
    gap_ctx = np.bincount(2 * e[:, 2] + e[:, 3], minlength=8)
    return dict(gap_ctx=gap_ctx, kind_ctx=np.bincount(e[:, 2], minlength=4), kinds=np.bincount(e[:, 1], minlength=3),
                ins=int((e[:, 1] == 1).sum()), sym64=int((e[:, 0] >= 64).sum()), g255=int((e[:, 0] >= 255).sum()))
