"""SAM output on the MI355X: Encoder.decode_sam and `cbc -x --sam`, full and by region, against the
SAM text that was compressed (FLAG, RNAME, POS, SEQ) and against the plain decode (SEQ), the refusals of the CLI, and one run
at a million reads where the text passes 100 MB."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import regionmodel as rm
import sammodel as sm
import synth
from cbc_amd import gpu, host
from oracle import oracle
from test_genome_shapes import check_features, genome
from test_region import _regions

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cbc_amd", "csrc", "cbc")
FLAGS = (0, 16, 99, 147, 1040, 2064)


@pytest.fixture(scope="module")
def enc():
    e = gpu.Encoder(0)
    yield e
    e.close()


def _dataset(seed, block_reads, n=3000):
    """Three contigs (last 3000 bases free of reads), read lengths 100 and 150 mixed, indels, trailing soft clips, both
    strands and several FLAG values, the deletion read of tests/test_region.py at the end of block 0."""
    fa, rbc, contigs = rm.mixed_dataset(seed, [60_000, 45_000, 20_000], [n, n // 2, 400], sub_rate=0.004, indel_frac=0.3,
                                        gap_tail=3000, flags=FLAGS, trailing_s_frac=0.1)
    recs = rbc[0][2]
    recs[block_reads - 1] = rm.deletion_read(contigs[0][1], recs[block_reads - 1]["pos"])
    sam = synth.sam_text(rbc)
    return fa, sam, host.pack_sam(sam, fa, block_reads=block_reads, var_length=True), rbc


@pytest.fixture(scope="module", params=[256, 1024])
def small(request, built):
    fa, sam, pb, rbc = _dataset(7 + request.param, request.param)
    blob = rm.container(pb)
    plan = host.UnpackPlan(blob, fa)
    inp = sm.input_records(sam)
    recs = [r + (i,) for i, r in enumerate(rm.records(pb))]
    assert len(inp) == len(recs) == pb.n_recs and all(inp[i][2] == r[2] and inp[i][3] == r[4] for i, r in enumerate(recs))
    cig = [r["cigar"] for _, _, rr in rbc for r in rr]
    assert sum("I" in c or "D" in c for c in cig) > 500 and sum(c.endswith("S") for c in cig) > 100
    assert {r[0] for r in inp} == set(FLAGS) and {len(r[3]) for r in inp} == {100, 150}
    yield dict(fa=fa, sam=sam, pb=pb, blob=blob, plan=plan, inp=inp, recs=recs, block_reads=request.param,
               hdr=sm.header(sm.header_of_sam(sam)))
    plan.close(); pb.close()


def test_full_decode_is_the_input(enc, small):
    plan, inp = small["plan"], small["inp"]
    enc.upload_reference(plan.ref)
    text, n, sel, res = enc.decode_sam(plan, results=True)
    assert (res["status"] == 0).all() and sel is None and n == len(inp)
    assert text == small["hdr"] + sm.expected_text(inp)
    recs, seq, _ = enc.decode_blocks(plan)                                   # SEQ line for line as the plain decode gives it
    assert [r[3] for r in sm.split_lines(text)[1]] == plan.text(recs, seq).split(b"\n")[:-1]
    dec, cnt, txt = enc.last_sam_ms()
    assert dec > 0 and cnt >= 0 and txt > 0


def test_regions_match_the_model(enc, small):
    plan, inp, recs = small["plan"], small["inp"], small["recs"]
    enc.upload_reference(plan.ref)
    regs = _regions(small, 100, 11)
    want = [[inp[r[5]] for r in rm.selected(recs, c, beg, end)] for _, c, beg, end in regs]
    n_hit = sum(1 for w in want if w)
    assert len(regs) >= 100 and n_hit >= 0.8 * len(regs) and len(regs) - n_hit >= 5, (len(regs), n_hit)
    for (s, c, beg, end), w in zip(regs, want):
        text, n, sel, res = enc.decode_sam(plan, s, results=True)
        assert (res["status"] == 0).all(), s
        assert text == small["hdr"] + sm.expected_text(w) and n == len(w), s


def test_text_cap_one_byte_short(enc, small):
    plan, inp = small["plan"], small["inp"]
    enc.upload_reference(plan.ref)
    total = len(sm.expected_text(inp))
    with pytest.raises(gpu.CbcGpuError, match="text_cap too small"):
        enc.decode_sam(plan, text_cap=total - 1)
    assert enc.last_sam_text_bytes == total
    assert enc.decode_sam(plan, text_cap=total) == small["hdr"] + sm.expected_text(inp)


def test_genome_shaped_input(enc, built):
    """N runs, lower case and IUPAC codes in the reference: FLAG / RNAME / POS against the SAM, SEQ against the plain decode
    (on such input the decode is not always the SEQ column)."""
    fa, sam, rbc, contigs = genome()
    check_features(rbc, contigs)
    pb = host.pack_sam(sam, fa, block_reads=1024)
    plan = host.UnpackPlan(rm.container(pb), fa)
    enc.upload_reference(plan.ref)
    inp = sm.input_records(sam)
    text, n, _, res = enc.decode_sam(plan, results=True)
    assert (res["status"] == 0).all() and n == len(inp) == pb.n_recs
    recs, seq, _ = enc.decode_blocks(plan)
    plain = plan.text(recs, seq).split(b"\n")[:-1]
    assert text == plan.sam_header() + sm.expected_text(inp, plain)
    assert sm.split_lines(text)[0] == sm.header(sm.header_of_sam(sam)).split(b"\n")[:-1]
    plan.close(); pb.close()


def test_a_million_reads(enc, built):
    """cfg2 shape at 1 M reads: > 100 MB of text over 245 blocks, so the 64-bit block offsets are real.  FLAG and POS are
    checked against the packed arrays, the packer's view of the input; SEQ against the plain decode."""
    pb = host.synth(0xCBC05A3, 248_956_422, 1_000_000, 150, block_reads=4096)
    enc.upload_reference(pb.ref)
    _, res, offs, flat = enc.encode_blocks(pb, want_payload_list=False)
    assert (res["status"] == 0).all()
    c = pb.contigs[0]
    fa = synth.fasta_text([("chr1", pb.ref[int(c["ref_off"]): int(c["ref_off"]) + int(c["length"])])])
    plan = host.UnpackPlan(pb.container(flat, offs), fa)
    enc.upload_reference(plan.ref)
    text, n, _, res = enc.decode_sam(plan, results=True)
    assert (res["status"] == 0).all() and n == pb.n_recs and plan.n_blocks > 200
    hdr = plan.sam_header()
    assert text.startswith(hdr) and hdr == b"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chr1\tLN:248956422\n"
    body = text[len(hdr):]
    assert len(body) > 100_000_000 and body.count(b"\n") == pb.n_recs
    recs, seq, _ = enc.decode_blocks(plan)
    plain = plan.text(recs, seq).split(b"\n")[:-1]
    blk = np.repeat(np.arange(pb.n_blocks), pb.blocks["n_reads"].astype(np.int64))
    pos = pb.info["window_start"][blk].astype(np.int64) + pb.recs["pos"].astype(np.int64)
    assert (np.diff(pos) >= 0).all()
    flags = pb.recs["flag"]
    # every line rebuilt from the packed arrays and the plain decode, compared in slices to bound memory
    lines = body.split(b"\n")[:-1]
    assert len(lines) == pb.n_recs
    for a in range(0, pb.n_recs, 50_000):
        want = [b"*\t%d\tchr1\t%d\t255\t*\t*\t0\t0\t%s\t*" % (int(flags[i]), int(pos[i]), plain[i]) for i in range(a, min(a + 50_000, pb.n_recs))]
        assert lines[a:a + 50_000] == want, a
    got_pos = np.array([int(ln.split(b"\t", 4)[3]) for ln in lines[::97]])
    assert (np.diff(got_pos) >= 0).all()
    plan.close(); pb.close()


def _cli(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def test_cli_sam(small, tmp_path):
    pb, inp, recs, hdr = small["pb"], small["inp"], small["recs"], small["hdr"]
    (tmp_path / "in.cbc").write_bytes(small["blob"]); (tmp_path / "ref.fa").write_bytes(small["fa"])
    files = (tmp_path / "in.cbc", tmp_path / "out.sam", tmp_path / "ref.fa")
    r = _cli("-x", *files, "--sam", "--verbose")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "out.sam").read_bytes() == hdr + sm.expected_text(inp)
    assert "kernels: decode" in r.stdout and "count + scan" in r.stdout and "text " in r.stdout and "reads written as SAM" in r.stdout
    # regions in the first, a middle and the last block; one that selects nothing
    nb = pb.n_blocks
    regs = []
    for b in (0, nb // 2, nb - 1):
        c, f = int(pb.info[b]["contig"]), int(pb.info[b]["window_start"]) + 1
        regs.append(("chr%d:%d-%d" % (c + 1, f + 5, f + 400), c, f + 5, f + 400))
    L2 = int(pb.contigs[1]["length"])
    regs.append(("chr2:%d-%d" % (L2 - 10, L2), 1, L2 - 10, L2))
    for k, (s, c, beg, end) in enumerate(regs):
        w = [inp[x[5]] for x in rm.selected(recs, c, beg, end)]
        assert bool(w) == (k < 3), s
        r = _cli("-d", *files, "--sam", "--region", s, "--verbose")
        assert r.returncode == 0, r.stderr
        assert (tmp_path / "out.sam").read_bytes() == hdr + sm.expected_text(w), s
        assert ("kernels: decode" in r.stdout) or not w
    # a region past every block's first POS is decided by the index alone: the header, exit 0
    r = _cli("-x", *files, "--sam", "--region", "chr3:%d" % (int(pb.contigs[2]["length"]) - 5))
    assert r.returncode == 0 and (tmp_path / "out.sam").read_bytes() == hdr
    # a region in front of the contig's first read selects no block: the header alone, no device opened
    first = min(x[2] for x in recs if x[1] == 0)
    assert first > 1 and small["plan"].region("chr1:1-%d" % (first - 1)).b1 == small["plan"].region("chr1:1-%d" % (first - 1)).b0
    r = _cli("-x", *files, "--sam", "--region", "chr1:1-%d" % (first - 1), "--verbose")
    assert r.returncode == 0 and (tmp_path / "out.sam").read_bytes() == hdr and "kernels:" not in r.stdout
    # the plain paths give the bytes they gave before
    r = _cli("-x", tmp_path / "in.cbc", tmp_path / "all.txt", tmp_path / "ref.fa")
    assert r.returncode == 0 and (tmp_path / "all.txt").read_bytes() == b"".join(x[3] + b"\n" for x in inp)
    s, c, beg, end = regs[1]
    r = _cli("-x", tmp_path / "in.cbc", tmp_path / "reg.txt", tmp_path / "ref.fa", "--region", s)
    assert r.returncode == 0 and (tmp_path / "reg.txt").read_bytes() == rm.expected_text(recs, c, beg, end)


def test_cli_sam_refusals(built, small, tmp_path):
    (tmp_path / "in.cbc").write_bytes(small["blob"]); (tmp_path / "ref.fa").write_bytes(small["fa"])
    (tmp_path / "in.sam").write_bytes(small["sam"])
    r = _cli("-c", tmp_path / "in.sam", tmp_path / "o.cbc", tmp_path / "ref.fa", "--sam")
    assert r.returncode == 1 and "--sam applies to decompression" in r.stderr, r.stderr
    r = _cli("-x", tmp_path / "in.cbc", tmp_path / "o.sam", tmp_path / "ref.fa", "--sam", "--devices", "0,1")
    assert r.returncode == 1 and "one device" in r.stderr, r.stderr
    fa, sam, _, _ = synth.dataset(4, [5000], [100], 100)
    (tmp_path / "c.cbc").write_bytes(oracle.encode(sam, fa)); (tmp_path / "c.fa").write_bytes(fa)
    r = _cli("-x", tmp_path / "c.cbc", tmp_path / "o.sam", tmp_path / "c.fa", "--sam")
    assert r.returncode == 1 and "single-stream (--compat) file" in r.stderr, r.stderr
    pb, _, lfa = host.synth_long(5, 200_000, 40, read_len=2000, want_text=True)
    flat, offs, _ = oracle.cpu_encode_blocks(pb, long_reads=True, return_flat=True)
    (tmp_path / "l.cbc").write_bytes(pb.container(flat, offs)); (tmp_path / "l.fa").write_bytes(lfa)
    r = _cli("-x", tmp_path / "l.cbc", tmp_path / "o.sam", tmp_path / "l.fa", "--sam")
    assert r.returncode == 1 and "long-read" in r.stderr, r.stderr
    pb.close()


@pytest.mark.skipif(shutil.which("samtools") is None, reason="samtools is not installed on this machine")
def test_samtools_reads_the_file(small, tmp_path):
    (tmp_path / "in.cbc").write_bytes(small["blob"]); (tmp_path / "ref.fa").write_bytes(small["fa"])
    assert _cli("-x", tmp_path / "in.cbc", tmp_path / "out.sam", tmp_path / "ref.fa", "--sam").returncode == 0
    r = subprocess.run(["samtools", "view", "-c", str(tmp_path / "out.sam")], capture_output=True, text=True)
    assert r.returncode == 0 and int(r.stdout) == len(small["inp"]), r.stderr
