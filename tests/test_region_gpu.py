"""Region decode on the MI355X: the span-reporting decoder against the packer's spans at 1 M reads,
Encoder.decode_region and `cbc -x --region` against the Python model, and the refusals of the CLI."""
import os
import subprocess

import numpy as np
import pytest

import regionmodel as rm
import synth
from cbc_amd import gpu, host
from oracle import oracle
from test_region import _dataset, _regions

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cbc_amd", "csrc", "cbc")


@pytest.fixture(scope="module")
def enc():
    e = gpu.Encoder(0)
    yield e
    e.close()


def _spans(pb):
    """Packer-derived span of every record, vectorised (fixed-length reads of the C generator)."""
    n = pb.n_recs
    rec_blk = np.repeat(np.arange(pb.n_blocks), pb.blocks["n_reads"].astype(np.int64))
    tok_at = pb.blocks["tok_base"][rec_blk].astype(np.int64) + pb.recs["tok_off"].astype(np.int64) + 1
    w1 = pb.tok[tok_at].astype(np.int64)
    rl = pb.recs["rlen"].astype(np.int64)
    L = int(rl[0])
    assert (rl == L).all()
    s0 = pb.blocks["seq_base"][rec_blk].astype(np.int64) + pb.recs["seq_off"].astype(np.int64)
    r0 = pb.blocks["ref_off"][rec_blk].astype(np.int64) + pb.recs["pos"].astype(np.int64) - 1
    perfect = np.zeros(n, dtype=bool)
    for a in range(0, n, 100_000):
        k = np.arange(L)
        seq = pb.seq[s0[a:a + 100_000, None] + k]
        ref = pb.ref[r0[a:a + 100_000, None] + k]
        perfect[a:a + 100_000] = (seq == ref).all(axis=1)
    return np.where(perfect, rl, rl + (w1 & 0xff) - ((w1 >> 16) & 0xff))


@pytest.fixture(scope="module")
def big(enc, built):
    """1 M indel-rich reads on one contig, coded on the GPU, as a container + FASTA."""
    pb = host.synth(0xCBC0BEEF, 30_000_000, 1_000_000, 150, sub_rate=0.004, indel_frac=0.3, block_reads=4096)
    enc.upload_reference(pb.ref)
    _, res, offs, flat = enc.encode_blocks(pb, want_payload_list=False)
    assert (res["status"] == 0).all()
    c = pb.contigs[0]
    fa = synth.fasta_text([("chr1", pb.ref[int(c["ref_off"]): int(c["ref_off"]) + int(c["length"])])])
    plan = host.UnpackPlan(pb.container(flat, offs), fa)
    yield pb, plan
    plan.close(); pb.close()


def test_span_decode_at_a_million_reads(enc, big):
    pb, plan = big
    enc.upload_reference(plan.ref)
    smax = pb.max_read_len + pb.read_length - 1
    recs, seq, res = enc.decode_blocks_span(plan, smax)
    assert (res["status"] == 0).all()
    spans = _spans(pb)
    assert (spans != 150).sum() > 100_000                                  # indel-rich
    assert (recs["tok_off"].astype(np.int64) == spans).all()
    prec, pseq, pres = enc.decode_blocks(plan)
    assert (pres["status"] == 0).all() and (prec["tok_off"] == 0).all()
    for k in ("pos", "flag", "rlen", "seq_off"):
        assert (prec[k] == recs[k]).all()
    assert pseq.tobytes() == seq.tobytes()
    # a bound one below the longest span fails the blocks that hold one, with CBC_ST_SPAN
    _, _, res = enc.decode_blocks_span(plan, int(spans.max()) - 1)
    assert (res["status"] == 8).any() and set(np.unique(res["status"])) <= {0, 8}


def test_whole_contig_region_at_a_million_reads(enc, big):
    pb, plan = big
    enc.upload_reference(plan.ref)
    text, nsel, sel, res = enc.decode_region(plan, "chr1", results=True)
    assert (res["status"] == 0).all() and (sel.b0, sel.b1) == (0, plan.n_blocks)
    recs, seq, _ = enc.decode_blocks(plan)
    assert nsel == pb.n_recs and text == plan.text(recs, seq)               # the whole of what `cbc -x` writes
    dec, flt, txt = enc.last_region_ms()
    assert dec > 0 and flt >= 0 and txt >= 0
    # a 10 kb locus: a handful of blocks
    mid = int(pb.contigs[0]["length"]) // 2
    text, nsel, sel, _ = enc.decode_region(plan, "chr1:%d-%d" % (mid, mid + 9999), results=True)
    assert 0 < sel.b1 - sel.b0 <= 4 and nsel > 0
    lo = int(plan.blocks[sel.b0]["rec_base"]); hi = int(plan.blocks[sel.b1 - 1]["rec_base"] + plan.blocks[sel.b1 - 1]["n_reads"])
    spans = _spans(pb)[lo:hi]
    blk = np.repeat(np.arange(pb.n_blocks), pb.blocks["n_reads"].astype(np.int64))[lo:hi]
    pos = pb.info["window_start"][blk].astype(np.int64) + pb.recs["pos"][lo:hi].astype(np.int64)
    keep = (pos <= mid + 9999) & (pos + spans - 1 >= mid)
    rows = recs[lo:hi]
    exp = b"".join(seq[(lo + i) * plan.seq_stride:(lo + i) * plan.seq_stride + int(rows[i]["rlen"])].tobytes() + b"\n"
                   for i in np.nonzero(keep)[0])
    assert nsel == int(keep.sum()) and text == exp


@pytest.fixture(scope="module", params=[256, 1024])
def small(request, built):
    fa, pb, contigs = _dataset(7 + request.param, request.param)
    blob = rm.container(pb)
    plan = host.UnpackPlan(blob, fa)
    yield dict(fa=fa, pb=pb, blob=blob, plan=plan, recs=rm.records(pb), block_reads=request.param)
    plan.close(); pb.close()


def test_region_text_matches_the_model(enc, small):
    plan, recs = small["plan"], small["recs"]
    enc.upload_reference(plan.ref)
    regs = _regions(small, 100, 11)
    for s, c, beg, end in regs:
        text, nsel, sel, res = enc.decode_region(plan, s, results=True)
        exp = rm.expected_text(recs, c, beg, end)
        assert (res["status"] == 0).all(), s
        assert text == exp and nsel == exp.count(b"\n"), s


def test_region_selecting_no_reads(enc, small):
    plan, pb = small["plan"], small["pb"]
    enc.upload_reference(plan.ref)
    L = int(pb.contigs[1]["length"])
    text, nsel, sel, res = enc.decode_region(plan, "chr2:%d-%d" % (L - 10, L), results=True)
    assert sel.b1 > sel.b0 and text == b"" and nsel == 0 and (res["status"] == 0).all()


def _cli(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def test_cli_region(small, tmp_path):
    (tmp_path / "in.cbc").write_bytes(small["blob"]); (tmp_path / "ref.fa").write_bytes(small["fa"])
    regs = _regions(small, 5, 12)
    for s, c, beg, end in regs[:5] + regs[-8:]:
        r = _cli("-x", tmp_path / "in.cbc", tmp_path / "out.txt", tmp_path / "ref.fa", "--region", s, "--verbose")
        assert r.returncode == 0, r.stderr
        assert (tmp_path / "out.txt").read_bytes() == rm.expected_text(small["recs"], c, beg, end), s
        assert "selected" in r.stdout
    # the full decode of the same container is untouched by the option's existence
    r = _cli("-x", tmp_path / "in.cbc", tmp_path / "all.txt", tmp_path / "ref.fa")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "all.txt").read_bytes() == b"".join(x[4] + b"\n" for x in small["recs"])
    # refusals
    for args, msg in [(("--region", "chrX:1-5"), "unknown contig"), (("--region", "chr1:5-1"), "ends before"),
                      (("--region", "chr1:1-5", "--devices", "0,1"), "one device")]:
        r = _cli("-x", tmp_path / "in.cbc", tmp_path / "bad.txt", tmp_path / "ref.fa", *args)
        assert r.returncode == 1 and msg in r.stderr, (args, r.stderr)


def test_cli_region_refuses_compat_and_long_read_files(built, tmp_path):
    fa, sam, _, _ = synth.dataset(4, [5000], [100], 100)
    (tmp_path / "c.cbc").write_bytes(oracle.encode(sam, fa)); (tmp_path / "c.fa").write_bytes(fa)
    r = _cli("-x", tmp_path / "c.cbc", tmp_path / "o.txt", tmp_path / "c.fa", "--region", "chr1:1-100")
    assert r.returncode == 1 and "no block index" in r.stderr, r.stderr
    pb, _, lfa = host.synth_long(5, 200_000, 40, read_len=2000, want_text=True)
    flat, offs, _ = oracle.cpu_encode_blocks(pb, long_reads=True, return_flat=True)
    (tmp_path / "l.cbc").write_bytes(pb.container(flat, offs)); (tmp_path / "l.fa").write_bytes(lfa)
    r = _cli("-x", tmp_path / "l.cbc", tmp_path / "o.txt", tmp_path / "l.fa", "--region", "chrL:1-1000")
    assert r.returncode == 1 and "long-read" in r.stderr, r.stderr
    pb.close()
