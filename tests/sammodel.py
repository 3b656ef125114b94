"""SAM output in plain Python: what `cbc -x --sam` must write, computed from the SAM text that was
compressed (FLAG, RNAME, POS, SEQ of every mapped record), the hand-made record arrays the emulated passes are fed with,
and the ctypes wrapper of the emulation library (tests/sam_emu)."""
import ctypes

import numpy as np

from cbc_amd import host

MAX_NAME = 255
MAX_POS = 2 ** 31 - 1


def header(contigs):
    """contigs: list of (name bytes, length)."""
    return b"@HD\tVN:1.6\tSO:coordinate\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (n, l) for n, l in contigs)


def line(flag, rname, pos, seq):
    return b"*\t%d\t%s\t%d\t255\t*\t*\t0\t0\t%s\t*\n" % (flag, rname, pos, seq)


def line_len(flag, rname, pos, rlen):
    return 20 + len(str(flag)) + len(rname) + len(str(pos)) + rlen


def input_records(sam: bytes):
    """(FLAG, RNAME, POS, SEQ) of every alignment line with FLAG & 4 == 0, in file order: columns 2, 3, 4 and 10."""
    out = []
    for ln in sam.split(b"\n"):
        if not ln or ln.startswith(b"@"):
            continue
        c = ln.split(b"\t")
        if int(c[1]) & 4:
            continue
        out.append((int(c[1]), c[2], int(c[3]), c[9]))
    return out


def header_of_sam(sam: bytes):
    """(name, length) of the @SQ lines of the input."""
    out = []
    for ln in sam.split(b"\n"):
        if ln.startswith(b"@SQ"):
            f = dict(x.split(b":", 1) for x in ln.split(b"\t")[1:])
            out.append((f[b"SN"], int(f[b"LN"])))
        elif ln and not ln.startswith(b"@"):
            break
    return out


def expected_text(inp, seqs=None):
    """Alignment lines of input records; seqs (one bytes per record) replaces column 10 where decode != SEQ."""
    return b"".join(line(f, n, p, s if seqs is None else seqs[i]) for i, (f, n, p, s) in enumerate(inp))


def split_lines(text: bytes):
    """(header lines, [(flag, rname, pos, seq)]) of SAM text written by the code under test; checks the constant fields."""
    hdr, recs = [], []
    for ln in text.split(b"\n")[:-1]:
        if ln.startswith(b"@"):
            hdr.append(ln)
            continue
        c = ln.split(b"\t")
        assert len(c) == 11 and c[0] == b"*" and c[4:9] == [b"255", b"*", b"*", b"0", b"0"] and c[10] == b"*", ln
        recs.append((int(c[1]), c[2], int(c[3]), c[9]))
    assert text.endswith(b"\n")
    return hdr, recs


# ---- hand-made records for the two passes (no decoder, no reference bases) ------------------------------------------------
FLAGS = [0, 9, 10, 99, 16, 1024, 65531]
LOCAL_POS = [1, 9, 10, 99_999, 100_000, 5, 2, 12_345_678]
WINDOW_STARTS = [0, 0, 5, 99_990, 123_456_789, MAX_POS - 5, 0]
NAME_LENS = [1, 3, 4, 5, 64, MAX_NAME]


def handmade(seed, stride, sizes, failed=()):
    """Blocks of `sizes` reads; block b is on contig b % len(NAME_LENS) (name lengths 1, 3, 4, 5, 64 and the limit), its window
    starts at WINDOW_STARTS[b % ...]; the records cycle through FLAGS, LOCAL_POS and the read lengths 1, 3, 4, 5, stride - 1,
    stride (and random ones).  Blocks in `failed` carry a decode status that is not OK.  Returns a dict of arrays + the
    model lines per block."""
    rng = np.random.default_rng(seed)
    names_list = [bytes(rng.choice(np.frombuffer(b"abcXYZ019_.:*-", dtype=np.uint8), size=n)) for n in NAME_LENS]
    names = b"".join(n + b"\0" for n in names_list)
    name_off = np.cumsum([0] + [len(n) + 1 for n in names_list[:-1]]).astype(np.uint32)
    nb, n = len(sizes), int(sum(sizes))
    blocks = np.zeros(nb, dtype=host.DEC_BLOCK_DTYPE)
    recs = np.zeros(n, dtype=host.REC_DTYPE)
    seq = rng.choice(np.frombuffer(b"ACGTN", dtype=np.uint8), size=n * stride + 8).astype(np.uint8)
    ws = np.zeros(nb, dtype=np.uint64)
    block_name = np.zeros(2 * nb, dtype=np.uint32)
    res = np.zeros(nb, dtype=host.RESULT_DTYPE)
    rls = [1, 3, 4, 5, stride - 1, stride]
    lines, at = [], 0
    for b, sz in enumerate(sizes):
        c = b % len(NAME_LENS)
        w = WINDOW_STARTS[b % len(WINDOW_STARTS)]
        ws[b] = w
        block_name[2 * b], block_name[2 * b + 1] = name_off[c], len(names_list[c])
        blocks[b]["rec_base"], blocks[b]["seq_base"] = at, at * stride
        blocks[b]["n_reads"], blocks[b]["seq_stride"] = sz, stride
        res[b]["nbytes"], res[b]["status"] = sz, (2 if b in failed else 0)
        bl = []
        for k in range(sz):
            r = at + k
            rl = rls[(k + b) % 6] if k % 3 else int(rng.integers(1, stride + 1))
            lp = min(LOCAL_POS[(k // 2 + b) % len(LOCAL_POS)] if k % 2 else int(rng.integers(1, 2 ** 27)), MAX_POS - w)
            fl = FLAGS[(k + b) % len(FLAGS)] if k % 5 else int(rng.integers(0, 65536))
            recs[r] = (lp, fl, rl, k * stride, 0)
            bl.append(line(fl, names_list[c], w + lp, seq[r * stride: r * stride + rl].tobytes()))
        lines.append([] if b in failed else bl)
        at += sz
    return dict(blocks=blocks, recs=recs, seq=seq, ws=ws, block_name=block_name, names=np.frombuffer(names, dtype=np.uint8).copy(),
                res=res, lines=lines, n=n, stride=stride, names_list=names_list)


# ---- the emulation library ------------------------------------------------------------------------------------------------
def emu_load(path):
    L = ctypes.CDLL(path)
    L.emu_sam_decode.restype = ctypes.c_int
    L.emu_sam_decode.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
    L.emu_sam.restype = ctypes.c_int
    L.emu_sam.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                          ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int,
                          ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                          ctypes.c_uint32]
    return L


def emu_passes(L, recs, n, seq, blocks, ws, res, block_name, names, cap, n_waves=4, region=None):
    """Count pass, scan and write pass on the emulation.  Returns (rc, text, counts, offsets); the guard bytes behind the
    text (and all of it when rc != 0) must be untouched, which is asserted here."""
    nb = len(blocks)
    text = np.full(cap + 16, 0xEE, dtype=np.uint8)
    counts = np.zeros(nb, dtype=host.RESULT_DTYPE)
    offs = np.zeros(nb + 1, dtype=np.uint64)
    beg, end = region if region else (0, 0)
    rc = L.emu_sam(recs.ctypes.data, n, seq.ctypes.data, seq.size, blocks.ctypes.data, ws.ctypes.data, res.ctypes.data, nb,
                   block_name.ctypes.data, names.ctypes.data, names.size, 1 if region else 0, beg, end, text.ctypes.data, cap,
                   counts.ctypes.data, offs.ctypes.data, n_waves)
    total = int(offs[nb])
    assert (text[total if rc == 0 else 0:] == 0xEE).all(), "bytes written outside the text"
    return rc, text[:total].tobytes() if rc == 0 else b"", counts, offs


def check_handmade(L, case, n_waves):
    """The two passes on a hand-made case against its model lines (used in-process and by the ASan child)."""
    want = [b"".join(bl) for bl in case["lines"]]
    total = sum(len(w) for w in want)
    rc, text, counts, offs = emu_passes(L, case["recs"], case["n"], case["seq"], case["blocks"], case["ws"], case["res"],
                                        case["block_name"], case["names"], total, n_waves)
    assert rc == 0
    assert [int(x) for x in counts["nbytes"]] == [len(w) for w in want]
    assert [int(x) for x in counts["n_symbols"]] == [len(bl) for bl in case["lines"]]
    assert [int(x) for x in offs] == [0] + list(np.cumsum([len(w) for w in want]))
    assert text == b"".join(want)
    return total
