"""SAM output without a GPU: the header and its refusals in libcbc_host, and the count and write
bodies of cbc_sam_body.h on the lock-step wave emulation (tests/sam_emu) against the Python model (sammodel.py), fed by
hand-made record arrays and by the emulated decoders.  Ground truth is the SAM text that was compressed."""
import ctypes
import os
import struct
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import blockref
import regionmodel as rm
import sammodel as sm
import synth
from cbc_amd import host
from oracle import oracle
from test_region import _regions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "sam_emu")


@pytest.fixture(scope="module")
def emu(built):
    subprocess.check_call(["make", "-C", EMU_DIR, "libcbc_sam_emu.so"], stdout=subprocess.DEVNULL)
    return sm.emu_load(os.path.join(EMU_DIR, "libcbc_sam_emu.so"))


# ---- header -----------------------------------------------------------------------------------------------------------------
def _plan(names, clen=3000, reads=30, L=100):
    rng = np.random.default_rng(len(names))
    contigs = [(n, synth.make_contig(rng, clen + 10 * i)) for i, n in enumerate(names)]
    rbc = [(n, len(c), synth.make_reads(rng, c, reads, L)) for n, c in contigs]
    fa, sam = synth.fasta_text(contigs), synth.sam_text(rbc)
    pb = host.pack_sam(sam, fa, block_reads=256, var_length=True)
    blob = rm.container(pb)
    pb.close()
    return host.UnpackPlan(blob, fa), sam, fa, blob


@pytest.mark.parametrize("names", [["chr1"], ["chr1", "HLA-A*01:01:01:01", "x"], ["c%d" % i for i in range(24)]])
def test_header_bytes(built, names):
    plan, sam, fa, _ = _plan(names)
    want = sm.header(sm.header_of_sam(sam))
    assert want.count(b"@SQ") == len(names)
    assert plan.sam_header() == want
    assert want == b"@HD\tVN:1.6\tSO:coordinate\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (n.encode(), 3000 + 10 * i) for i, n in enumerate(names))
    plan.close()


def _names_at(blob):
    nc, nb, nbytes = struct.unpack_from("<III", blob, 12)
    return 36, nbytes, 36 + ((nbytes + 3) & ~3)


def test_header_refusals(built):
    plan, sam, fa, blob = _plan(["chr1", "chr2"])
    plan.close()
    n0, nbytes, ctab = _names_at(blob)
    b = bytearray(blob); b[n0 + 2] = 9                                       # a tab inside "chr1"
    p = host.UnpackPlan(bytes(b), fa)
    with pytest.raises(host.CbcInputError, match="holds a tab or a newline"):
        p.sam_header()
    p.close()
    b = bytearray(blob); struct.pack_into("<I", b, ctab + 16, 10 ** 6)       # name offset of contig 1 outside the table
    p = host.UnpackPlan(bytes(b), fa)
    with pytest.raises(host.CbcInputError, match="outside the name table"):
        p.sam_header()
    assert p.sam_text_cap() == 0
    p.close()
    # a contig longer than 2^31 - 1: the plan's table is patched in place (a FASTA of that size is not made here)
    p = host.UnpackPlan(blob, fa)
    p.contig_len[1] = 2 ** 31
    with pytest.raises(host.CbcInputError, match="longer than 2\\^31 - 1 bases"):
        p.sam_header()
    p.contig_len[1] = 2 ** 31 - 1
    assert p.sam_header().endswith(b"\tLN:2147483647\n")
    p.close()


def test_header_refuses_a_long_read_plan(built):
    pb, sam, fa = host.synth_long(5, 200_000, 40, read_len=2000, want_text=True)
    flat, offs, res = oracle.cpu_encode_blocks(pb, long_reads=True, return_flat=True)
    plan = host.UnpackPlan(pb.container(flat, offs), fa)
    with pytest.raises(host.CbcInputError, match="long-read"):
        plan.sam_header()
    assert plan.sam_text_cap() == 0
    plan.close(); pb.close()


def _renamed(blob, names):
    """The container with its name table replaced (the packer itself stops at 125 characters; the format does not)."""
    nc, nb, nbytes = struct.unpack_from("<III", blob, 12)
    assert nc == len(names)
    tab = b"".join(n + b"\0" for n in names)
    offs = np.cumsum([0] + [len(n) + 1 for n in names[:-1]])
    out = bytearray(blob[:36]) + tab + b"\0" * (-len(tab) % 4) + blob[36 + ((nbytes + 3) & ~3):]
    struct.pack_into("<I", out, 20, len(tab))
    for c in range(nc):
        struct.pack_into("<I", out, 36 + ((len(tab) + 3) & ~3) + 16 * c, int(offs[c]))
    return bytes(out)


def test_name_length_limit(built):
    plan, sam, fa, blob = _plan(["chr1", "chr2"])
    plan.close()
    ok, long = b"n" * sm.MAX_NAME, b"m" * (sm.MAX_NAME + 1)
    p = host.UnpackPlan(_renamed(blob, [ok, b"chr2"]), fa)
    assert p.sam_header() == sm.header([(ok, 3000), (b"chr2", 3010)])
    assert p.sam_text_cap() == sum(int(b["n_reads"]) * (35 + (255 if int(c) == 0 else 4) + p.seq_stride)
                                   for b, c in zip(p.blocks, p.block_contig))
    p.close()
    p = host.UnpackPlan(_renamed(blob, [b"chr1", long]), fa)
    with pytest.raises(host.CbcInputError, match="longer than 255 bytes"):
        p.sam_header()
    p.close()


# ---- the two passes on hand-made records -------------------------------------------------------------------------------------
SIZES = [1, 63, 64, 65, 7, 16384, 3, 9]
FAILED = (6,)


@pytest.fixture(scope="module", params=[152, 256])
def case(request):
    return sm.handmade(31 + request.param, request.param, SIZES, FAILED)


def test_handmade_case_covers_what_it_should(case):
    """Asserted on the model alone: every FLAG, POS, name length, read length and output alignment the passes must handle."""
    lines = [ln for bl in case["lines"] for ln in bl]
    cols = [ln.split(b"\t") for ln in lines]
    flags, poss = {int(c[1]) for c in cols}, {int(c[3]) for c in cols}
    assert set(sm.FLAGS) <= flags and {len(str(f)) for f in flags} == {1, 2, 3, 4, 5}
    assert {1, 9, 10, 99_999, 100_000, sm.MAX_POS} <= poss and {len(str(p)) for p in poss} >= {1, 2, 5, 6, 8, 9, 10}
    assert {len(c[2]) for c in cols} == set(sm.NAME_LENS)
    assert {1, 3, 4, 5, case["stride"] - 1, case["stride"]} <= {len(c[9]) for c in cols}
    starts = np.cumsum([0] + [len(ln) for ln in lines])
    assert set(int(s) % 4 for s in starts) == {0, 1, 2, 3}
    assert all(len(ln) == sm.line_len(int(c[1]), c[2], int(c[3]), len(c[9])) for ln, c in zip(lines, cols))
    assert case["lines"][FAILED[0]] == [] and int(case["res"][FAILED[0]]["status"]) != 0
    assert sum(len(bl) for bl in case["lines"]) == sum(SIZES) - SIZES[FAILED[0]]


@pytest.mark.parametrize("n_waves", [1, 4, 16])
def test_passes_match_the_model_on_handmade_records(emu, case, n_waves):
    total = sm.check_handmade(emu, case, n_waves)
    assert total > 16384 * 40


def test_text_cap_one_byte_short(emu, case):
    total = sum(len(ln) for bl in case["lines"] for ln in bl)
    rc, text, counts, offs = sm.emu_passes(emu, case["recs"], case["n"], case["seq"], case["blocks"], case["ws"], case["res"],
                                           case["block_name"], case["names"], total - 1)
    assert rc == -1 and int(offs[-1]) == total and text == b""


def test_asan_build_of_the_emulation(built, tmp_path):
    """The same hand-made case on an AddressSanitizer / UBSan build of the emulation library, in a child process."""
    subprocess.check_call(["make", "-C", EMU_DIR, "asan"], stdout=subprocess.DEVNULL)
    code = textwrap.dedent("""
        import sys
        sys.path[:0] = [%r, %r]
        import sammodel as sm
        L = sm.emu_load(%r)
        for stride in (152, 256):
            case = sm.handmade(5 + stride, stride, [1, 63, 64, 65, 7, 700, 3], (4,))
            for w in (1, 4):
                sm.check_handmade(L, case, w)
        print("SAM EMU OK")
    """ % (ROOT, os.path.join(ROOT, "tests"), os.path.join(EMU_DIR, "libcbc_sam_emu_asan.so")))
    env = dict(os.environ, LD_PRELOAD=subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip(),
               ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and "SAM EMU OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- fed by the emulated decoders: full decode and regions against the SAM that was compressed ----------------------------
def _dataset(seed, block_reads, n=3000):
    """The dataset of tests/test_region.py (same generator, same arguments, same deletion read), with its SAM text kept."""
    fa, rbc, contigs = rm.mixed_dataset(seed, [60_000, 45_000, 20_000], [n, n // 2, 400], sub_rate=0.004, indel_frac=0.3,
                                        gap_tail=3000)
    recs = rbc[0][2]
    recs[block_reads - 1] = rm.deletion_read(contigs[0][1], recs[block_reads - 1]["pos"])
    sam = synth.sam_text(rbc)
    pb = host.pack_sam(sam, fa, block_reads=block_reads, var_length=True)
    return fa, sam, pb


@pytest.fixture(scope="module", params=[256, 1024])
def data(request, built):
    fa, sam, pb = _dataset(7 + request.param, request.param)
    plan = host.UnpackPlan(rm.container(pb), fa)
    inp = sm.input_records(sam)
    recs = [r + (i,) for i, r in enumerate(rm.records(pb))]                   # regionmodel's view + the index into `inp`
    assert len(inp) == len(recs) == pb.n_recs
    assert all(inp[i][2] == r[2] and inp[i][3] == r[4] for i, r in enumerate(recs))
    yield dict(fa=fa, sam=sam, pb=pb, plan=plan, inp=inp, recs=recs, block_reads=request.param)
    plan.close(); pb.close()


def _emu_decode(emu, plan, b0, b1, smax):
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
    assert emu.emu_sam_decode(ctypes.byref(db), smax) == 0
    assert (res["status"] == 0).all()
    return bl, recs, seq, res, nrec


def _emu_sam_text(emu, plan, sel=None, n_waves=4):
    b0, b1 = (sel.b0, sel.b1) if sel else (0, plan.n_blocks)
    if b1 == b0:
        return b""
    bl, recs, seq, res, nrec = _emu_decode(emu, plan, b0, b1, sel.smax if sel else 0)
    ws = np.ascontiguousarray(plan.window_start[b0:b1], dtype=np.uint64)
    bn = np.zeros(2 * (b1 - b0), dtype=np.uint32)
    for k, c in enumerate(plan.block_contig[b0:b1]):
        off = int(plan.contig_name_off[int(c)])
        bn[2 * k], bn[2 * k + 1] = off, plan.names[off:].tobytes().index(b"\0")
    names = np.ascontiguousarray(plan.names)
    rc, text, counts, offs = sm.emu_passes(emu, recs, nrec, seq, bl, ws, res, bn, names, plan.sam_text_cap(b0, b1), n_waves,
                                           (sel.beg, sel.end) if sel else None)
    assert rc == 0
    return text


def test_emulated_full_decode_is_the_input(emu, data):
    plan, inp = data["plan"], data["inp"]
    assert plan.sam_header() == sm.header(sm.header_of_sam(data["sam"]))
    text = _emu_sam_text(emu, plan)
    assert text == sm.expected_text(inp)                                      # FLAG, RNAME, POS, SEQ of the SAM compressed
    plain_recs, plain_seq, _ = blockref.emu_decode(plan)                      # and SEQ as the plain decode gives it
    assert [r[3] for r in sm.split_lines(text)[1]] == plan.text(plain_recs, plain_seq).split(b"\n")[:-1]
    assert len({r[0] for r in inp}) >= 2 and len({r[1] for r in inp}) == 3


@pytest.mark.parametrize("n_waves", [1, 4])
def test_emulated_regions_match_the_model(emu, data, n_waves):
    plan, inp, recs = data["plan"], data["inp"], data["recs"]
    regs = _regions(data, 100, 5)
    want = [[inp[r[5]] for r in rm.selected(recs, c, beg, end)] for _, c, beg, end in regs]
    n_hit = sum(1 for w in want if w)
    assert len(regs) >= 100 and n_hit >= 0.8 * len(regs) and len(regs) - n_hit >= 5, (len(regs), n_hit)
    for (s, c, beg, end), w in zip(regs, want):
        assert _emu_sam_text(emu, plan, plan.region(s), n_waves) == sm.expected_text(w), s
