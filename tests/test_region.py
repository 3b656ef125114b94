"""Region decode without a GPU: the region parser and the block selection of libcbc_host
(cbc_unpack_region) against a brute-force model of the packed records, hostile block indexes on the AddressSanitizer
build, the refusals, and the span decode + filter + text bodies on the lock-step wave emulation."""
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
import synth
from cbc_amd import host
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "region_emu")


def _dataset(seed, block_reads, n=3000):
    fa, rbc, contigs = rm.mixed_dataset(seed, [60_000, 45_000, 20_000], [n, n // 2, 400], sub_rate=0.004, indel_frac=0.3,
                                        gap_tail=3000)
    recs = rbc[0][2]                 # the last read of block 0 gets a 40-base deletion
    recs[block_reads - 1] = rm.deletion_read(contigs[0][1], recs[block_reads - 1]["pos"])
    pb = rm.pack(fa, rbc, block_reads)
    return fa, pb, contigs


@pytest.fixture(scope="module", params=[256, 1024])
def data(request, built):
    fa, pb, contigs = _dataset(7 + request.param, request.param)
    blob = rm.container(pb)
    plan = host.UnpackPlan(blob, fa)
    yield dict(fa=fa, pb=pb, contigs=contigs, blob=blob, plan=plan, recs=rm.records(pb), block_reads=request.param)
    plan.close()
    pb.close()


def _regions(d, n_random, seed):
    """(region string, contig, beg, end) -- random ones plus the edge cases."""
    pb, rng = d["pb"], np.random.default_rng(seed)
    lens = [int(c["length"]) for c in pb.contigs]
    out = []
    for _ in range(n_random):
        c = int(rng.integers(0, len(lens)))
        beg = int(rng.integers(1, lens[c] + 1))
        end = min(lens[c], beg + int(rng.choice([0, 1, 50, 300, 2000, 20000])))
        out.append(("chr%d:%d-%d" % (c + 1, beg, end), c, beg, end))
    for b in range(pb.n_blocks):                                  # a region ending exactly at a block's first POS
        c, f = int(pb.info[b]["contig"]), int(pb.info[b]["window_start"]) + 1
        out.append(("chr%d:%d-%d" % (c + 1, max(1, f - 40), f), c, max(1, f - 40), f))
    dpos = int(pb.recs[d["block_reads"] - 1]["pos"]) + int(pb.info[0]["window_start"])
    nxt = int(pb.info[1]["window_start"]) + 1                     # BEG past the next block's first POS, reached by the deletion
    assert dpos <= nxt < dpos + 129
    out.append(("chr1:%d-%d" % (dpos + 130, dpos + 135), 0, dpos + 130, dpos + 135))
    for c, L in enumerate(lens):
        n = "chr%d" % (c + 1)
        out += [(n + ":1-1", c, 1, 1), (n + ":%d-%d" % (L, L), c, L, L), (n, c, 1, L),
                (n + ":%d-%d" % (L - 1500, L - 1000), c, L - 1500, L - 1000),       # the tail without reads
                (n + ":%d" % (L // 2), c, L // 2, L), (n + ":10-%d" % (L + 10 ** 9), c, 10, L)]
    return out


def test_deletion_read_reaches_into_the_next_block(data):
    d = data
    recs = [r for r in d["recs"] if r[0] == 0]
    assert len(recs) == d["block_reads"] and recs[-1][3] == 140 and int(d["pb"].info[1]["contig"]) == 0


def test_selection_matches_the_model(data):
    d, plan, pb = data, data["plan"], data["pb"]
    smax = pb.max_read_len + pb.read_length - 1
    regs = _regions(d, 300, 1)
    n_nonempty = 0
    for s, c, beg, end in regs:
        sel = plan.region(s)
        assert (sel.contig, sel.beg, sel.end, sel.smax) == (c, beg, end, smax), s
        want = rm.expected_blocks(pb, c, beg, end, smax)
        if want is None:
            assert sel.b0 == sel.b1, s
        else:
            assert (sel.b0, sel.b1) == want, s
        hit = {r[0] for r in rm.selected(d["recs"], c, beg, end)}
        assert all(sel.b0 <= b < sel.b1 for b in hit), (s, sorted(hit), sel)
        n_nonempty += bool(hit)
    assert n_nonempty > 200
    assert any(r[3] > len(r[4]) for r in d["recs"])                    # reads with deletions are in the data


def test_parser_forms_and_errors(data):
    plan, pb = data["plan"], data["pb"]
    L1 = int(pb.contigs[0]["length"])
    assert (plan.region("chr1").beg, plan.region("chr1").end) == (1, L1)
    assert (plan.region("chr1:100").beg, plan.region("chr1:100").end) == (100, L1)
    assert (plan.region(b"chr2:5-9").contig, plan.region("chr2:5-9").end) == (1, 9)
    assert plan.region("chr1:7-%d" % (L1 + 5)).end == L1                      # clamped
    for bad, what in [("chrX", "unknown contig"), ("chrX:1-5", "unknown contig"), ("chr1:0-5", "before base 1"),
                      ("chr1:9-5", "ends before"), ("chr1:", "malformed"), ("chr1:5-", "malformed"), ("chr1:a-5", "malformed"),
                      ("chr1:1-2-3", "malformed"), ("chr1:%d" % (L1 + 1), "past the end"), ("chr1:-5", "malformed"),
                      ("chr1:99999999999999999999", "malformed"), ("", "unknown contig")]:
        with pytest.raises(host.CbcInputError, match=what):
            plan.region(bad)


def test_name_containing_a_colon(built):
    rng = np.random.default_rng(3)
    names = ["HLA-A*01:01:01:01", "HLA-A*01:01:01:01:1-5", "plain"]
    contigs = [(n, synth.make_contig(rng, 3000)) for n in names]
    rbc = [(n, 3000, synth.make_reads(rng, c, 50, 100)) for n, c in contigs]
    pb = rm.pack(synth.fasta_text(contigs), rbc, 256)
    plan = host.UnpackPlan(rm.container(pb), synth.fasta_text(contigs))
    s = plan.region("HLA-A*01:01:01:01")                                     # the whole string is a name
    assert (s.contig, s.beg, s.end) == (0, 1, 3000)
    s = plan.region("HLA-A*01:01:01:01:1-5")                                 # a name, although it parses as NAME:BEG-END
    assert (s.contig, s.beg, s.end) == (1, 1, 3000)
    s = plan.region("HLA-A*01:01:01:01:20-30")                               # split at the last ':'
    assert (s.contig, s.beg, s.end) == (0, 20, 30)
    plan.close(); pb.close()


# ---- the bodies on the lock-step emulation: span decode, filter, text ----------------------------------------------------
_emu = None


def _emu_lib():
    global _emu
    if _emu is None:
        subprocess.check_call(["make", "-C", EMU_DIR, "libcbc_region_emu.so"], stdout=subprocess.DEVNULL)
        L = ctypes.CDLL(os.path.join(EMU_DIR, "libcbc_region_emu.so"))
        L.emu_decode_span.restype = ctypes.c_int
        L.emu_decode_span.argtypes = [ctypes.POINTER(blockref.DecDeviceBatch), ctypes.c_uint32]
        L.emu_region.restype = ctypes.c_int
        L.emu_region.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64,
                                 ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
        _emu = L
    return _emu


def _emu_span_decode(plan, b0, b1, smax):
    """The selected blocks laid out from 0 (as cbc_gpu_decode_region does) and decoded with the spans reported."""
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
    assert _emu_lib().emu_decode_span(ctypes.byref(db), smax) == 0
    return bl, recs, seq, res, nrec


def _emu_region_text(plan, sel, n_waves=4):
    if sel.b1 == sel.b0:
        return b""
    bl, recs, seq, res, nrec = _emu_span_decode(plan, sel.b0, sel.b1, sel.smax)
    assert (res["status"] == 0).all()
    nb = sel.b1 - sel.b0
    ws = np.ascontiguousarray(plan.window_start[sel.b0:sel.b1], dtype=np.uint64)
    cap = nrec * (plan.seq_stride + 1)
    text = np.full(cap + 16, 0xEE, dtype=np.uint8)
    counts = np.zeros(nb, dtype=host.RESULT_DTYPE)
    offs = np.zeros(nb + 1, dtype=np.uint64)
    rc = _emu_lib().emu_region(recs.ctypes.data, nrec, seq.ctypes.data, seq.size, bl.ctypes.data, ws.ctypes.data, res.ctypes.data,
                               nb, sel.beg, sel.end, text.ctypes.data, cap, counts.ctypes.data, offs.ctypes.data, n_waves)
    assert rc == 0
    n = int(offs[nb])
    assert (text[n:] == 0xEE).all()                                          # nothing written past the text
    return text[:n].tobytes()


def test_emulated_span_decode_reports_the_packer_span(data):
    plan = data["plan"]
    smax = data["pb"].max_read_len + data["pb"].read_length - 1
    bl, recs, seq, res, nrec = _emu_span_decode(plan, 0, plan.n_blocks, smax)
    assert (res["status"] == 0).all()
    spans = np.array([r[3] for r in data["recs"]])
    assert (recs["tok_off"][:nrec] == spans).all()
    plain_recs, plain_seq, _ = blockref.emu_decode(plan)                     # pos / flag / rlen / bases as the plain decoder's
    for k in ("pos", "flag", "rlen", "seq_off"):
        assert (plain_recs[k] == recs[k][:nrec]).all()
    assert (plain_recs["tok_off"] == 0).all()
    assert plain_seq[:nrec * plan.seq_stride].tobytes() == seq[:nrec * plan.seq_stride].tobytes()


def test_emulated_span_bound_fails_the_block(data):
    plan = data["plan"]
    _, _, _, res, _ = _emu_span_decode(plan, 0, 1, 139)                      # block 0 holds the 140-base span
    assert int(res[0]["status"]) == 8                                       # CBC_ST_SPAN


@pytest.mark.parametrize("n_waves", [1, 4])
def test_emulated_region_text_matches_the_model(data, n_waves):
    plan, recs = data["plan"], data["recs"]
    regs = _regions(data, 40, 2)
    for s, c, beg, end in regs:
        sel = plan.region(s)
        assert _emu_region_text(plan, sel, n_waves) == rm.expected_text(recs, c, beg, end), s


def test_emulated_region_write_guards(data):
    """The guards of the write pass through the region member of the reads-text skeleton: a failed block, a block that keeps
    nothing and a block whose text would end past text_cap write nothing; the other blocks' bytes stay where the scan put them."""
    plan, recs = data["plan"], data["recs"]
    sel = plan.region("chr1")
    nb = sel.b1 - sel.b0
    assert nb >= 3
    bl, rr, seq, res, nrec = _emu_span_decode(plan, sel.b0, sel.b1, sel.smax)
    assert (res["status"] == 0).all()
    ws = np.ascontiguousarray(plan.window_start[sel.b0:sel.b1], dtype=np.uint64)
    full = nrec * (plan.seq_stride + 1)

    def passes(res, beg, end, cap):
        text = np.full(full + 16, 0xEE, dtype=np.uint8)
        counts = np.zeros(nb, dtype=host.RESULT_DTYPE)
        offs = np.zeros(nb + 1, dtype=np.uint64)
        assert _emu_lib().emu_region(rr.ctypes.data, nrec, seq.ctypes.data, seq.size, bl.ctypes.data, ws.ctypes.data,
                                     res.ctypes.data, nb, beg, end, text.ctypes.data, cap, counts.ctypes.data, offs.ctypes.data, 4) == 0
        return text, counts, offs

    whole = rm.expected_text(recs, 0, sel.beg, sel.end)
    text, counts, offs = passes(res, sel.beg, sel.end, full)
    assert text[:int(offs[nb])].tobytes() == whole and (counts["nbytes"] > 0).all()
    # block not ok: its count is 0 and the text is that of the other blocks
    bad = res.copy()
    bad[1]["status"] = 8
    text, counts, offs = passes(bad, sel.beg, sel.end, full)
    without = [r for r in recs if r[0] != sel.b0 + 1]
    assert int(counts[1]["nbytes"]) == 0 and text[:int(offs[nb])].tobytes() == rm.expected_text(without, 0, sel.beg, sel.end)
    assert (text[int(offs[nb]):] == 0xEE).all()
    # zero bytes: every block decoded and in reach of the window, no read overlaps the contig's tail
    tail = int(data["pb"].contigs[0]["length"]) - 1000
    text, counts, offs = passes(res, tail, tail, full)
    assert int(offs[nb]) == 0 and (counts["status"] == 0).all() and (text == 0xEE).all()
    # the text one byte short: the last block would end past text_cap and is not written, the others are
    text, counts, offs = passes(res, sel.beg, sel.end, len(whole) - 1)
    cut = int(offs[nb - 1])
    assert int(offs[nb]) == len(whole) and text[:cut].tobytes() == whole[:cut] and (text[cut:] == 0xEE).all()


# ---- refusals and hostile containers -------------------------------------------------------------------------------------
def test_long_read_container_is_refused(built):
    pb, sam, fa = host.synth_long(5, 200_000, 40, read_len=2000, want_text=True)
    flat, offs, res = oracle.cpu_encode_blocks(pb, long_reads=True, return_flat=True)
    plan = host.UnpackPlan(pb.container(flat, offs), fa)
    with pytest.raises(host.CbcInputError, match="long-read"):
        plan.region("chrL:1-1000")
    plan.close(); pb.close()


def test_compat_stream_is_refused(built):
    fa, sam, _, _ = synth.dataset(4, [5000], [100], 100)
    stream = oracle.encode(sam, fa)
    with pytest.raises(host.CbcInputError, match="not a cbc block container"):
        host.UnpackPlan(stream, fa)


def _index_entry(blob, b):
    nc, nb, nbytes = struct.unpack_from("<III", blob, 12)
    return 36 + ((nbytes + 3) & ~3) + 16 * nc + 32 * b


def test_hostile_block_index_is_rejected_under_asan(built, data, tmp_path):
    """Crafted index entries -- wrapping payload offsets, a contig past the table, window starts out of order, blocks of a
    contig out of contig order, a name offset past the names -- are refused by plan creation or by the region selection,
    on an AddressSanitizer build of libcbc_host in a child process."""
    blob, fa = bytearray(data["blob"]), data["fa"]
    cases = []
    e1 = _index_entry(blob, 1)
    b = bytearray(blob); struct.pack_into("<Q", b, e1 + 16, 2 ** 64 - 8); cases.append(("plan", b))           # payload_off wraps
    b = bytearray(blob); struct.pack_into("<I", b, e1 + 24, 2 ** 32 - 1); cases.append(("plan", b))           # payload_bytes
    b = bytearray(blob); struct.pack_into("<I", b, e1, 7); cases.append(("plan", b))                          # contig >= n_contigs
    b = bytearray(blob); struct.pack_into("<Q", b, e1 + 8, 0); struct.pack_into("<Q", b, _index_entry(b, 0) + 8, 500)
    cases.append(("region", b))                                                                              # window_start falls
    b = bytearray(blob); struct.pack_into("<I", b, _index_entry(b, 0), 1); cases.append(("region", b))        # contig order
    nc = struct.unpack_from("<I", blob, 12)[0]
    names_pad = (struct.unpack_from("<I", blob, 20)[0] + 3) & ~3
    b = bytearray(blob); struct.pack_into("<I", b, 36 + names_pad, 10 ** 6); cases.append(("region", b))     # name offset
    tmp = str(tmp_path / "hostile.bin")
    csrc = os.path.join(ROOT, "cbc_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "libcbc_host_asan.so"], stdout=subprocess.DEVNULL)
    with open(tmp, "wb") as f:
        for _, blb in cases:
            f.write(struct.pack("<Q", len(blb)) + bytes(blb))
    code = textwrap.dedent("""
        import struct, sys
        sys.path.insert(0, %r)
        from cbc_amd import host
        host.HOST_LIB = %r
        fa = open(%r, "rb").read()
        raw = open(%r, "rb").read(); at = 0; n = 0
        while at < len(raw):
            k = struct.unpack_from("<Q", raw, at)[0]; blob = raw[at + 8: at + 8 + k]; at += 8 + k
            try:
                p = host.UnpackPlan(blob, fa)
            except host.CbcInputError:
                n += 1; print("PLAN"); continue
            for r in ("chr1", "chr1:1000-2000", "chr2:5-9", "chr3"):
                try:
                    p.region(r)
                except host.CbcInputError as e:
                    n += 1; print("REGION", e); break
            p.close()
        print("REJECTED", n)
    """ % (ROOT, os.path.join(csrc, "libcbc_host_asan.so"), tmp + ".fa", tmp))
    with open(tmp + ".fa", "wb") as f:
        f.write(fa)
    env = dict(os.environ, LD_PRELOAD=subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip(),
               ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert "REJECTED %d" % len(cases) in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    kinds = [ln.split()[0] for ln in r.stdout.splitlines() if ln.startswith(("PLAN", "REGION"))]
    assert kinds == [k.upper() for k, _ in cases], r.stdout
