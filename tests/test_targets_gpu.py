"""Decode of a set of regions on the MI355X: Encoder.decode_targets and `cbc -x` with repeated
--region and --regions-file against the models of the single-region paths (targetsmodel.py), a mid-size case against the full
decode filtered on the host and against Encoder.decode_depth per merged interval, a failed block, and the CLI's refusals."""
import os
import subprocess

import numpy as np
import pytest

import depthmodel as dm
import regionmodel as rm
import synth
import targetsmodel as tm
from cbc_amd import gpu, host
from oracle import oracle
from test_region import _dataset, _regions

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cbc_amd", "csrc", "cbc")
NAMES = [b"chr1", b"chr2", b"chr3"]


@pytest.fixture(scope="module")
def enc():
    e = gpu.Encoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module", params=[256, 1024])
def small(request, built):
    fa, pb, contigs = _dataset(7 + request.param, request.param)
    blob = rm.container(pb)
    plan = host.UnpackPlan(blob, fa)
    d = dict(fa=fa, pb=pb, blob=blob, plan=plan, recs=rm.records(pb), block_reads=request.param, iv=dm.intervals_a(pb),
             lens=[len(c) for _, c in contigs])
    d["flags"] = [x[3] for x in d["iv"]]
    yield d
    plan.close(); pb.close()


def _sets(d):
    special, _ = tm.special_set(d["pb"], d["recs"], d["block_reads"])
    return dict(random200=[(c, b, e) for _, c, b, e in _regions(d, 200, 21)], special=special,
                dense4100=tm.dense_set(0, 500, 4100, 13, 6), one=[(1, 12_000, 12_400)])


def _want(d, merged, exclude=0):
    reads = tm.expected_reads(d["recs"], merged)
    return reads, d["plan"].sam_header() + tm.expected_sam(d["recs"], d["flags"], NAMES, merged), \
        tm.expected_depth(d["iv"], NAMES, d["lens"], merged, exclude)


def test_small_datasets_all_outputs(enc, small):
    d, plan = small, small["plan"]
    enc.upload_reference(plan.ref)
    for name, ivs in _sets(d).items():
        merged = tm.merge(ivs)
        h = len(ivs) // 2
        ts = plan.targets(tm.region_strings(ivs[:h], NAMES), tm.bed(ivs[h:], NAMES))
        assert ts.intervals() == merged
        reads, sam, (depth, runs) = _want(d, merged)
        text, n, _, res = enc.decode_targets(plan, ts, "reads", results=True)
        assert (res["status"] == 0).all() and len(res) == ts.n_blocks, name
        assert text == reads and n == reads.count(b"\n"), name
        text, n, _, _ = enc.decode_targets(plan, ts, "sam", results=True)
        assert text == sam and n == reads.count(b"\n"), name
        text, _, nr, _ = enc.decode_targets(plan, ts, "depth", results=True)
        assert (text, nr) == (depth, runs), name
        ms = enc.last_targets_ms()
        assert len(ms) == 4 and all(x >= 0 for x in ms)
    merged = tm.merge(_sets(d)["random200"])
    ts = plan.targets(tm.region_strings(merged, NAMES))
    assert enc.decode_targets(plan, ts, "depth", exclude_flags=16) == _want(d, merged, 16)[2][0]
    one = plan.targets(["chr2:12000-12400"])                                   # one interval: the single-region calls' bytes
    assert enc.decode_targets(plan, one) == enc.decode_region(plan, "chr2:12000-12400")
    assert enc.decode_targets(plan, one, "sam") == enc.decode_sam(plan, "chr2:12000-12400")
    assert enc.decode_targets(plan, one, "depth") == enc.decode_depth(plan, "chr2:12000-12400")
    want = tm.expected_reads(d["recs"], merged)
    with pytest.raises(gpu.CbcGpuError, match="text_cap too small"):
        enc.decode_targets(plan, ts, text_cap=len(want) - 1)
    assert enc.last_targets_text_bytes == len(want)
    assert enc.decode_targets(plan, ts, text_cap=len(want)) == want
    empty = plan.targets((), b"chrUn\t1\t9\n")
    assert enc.decode_targets(plan, empty) == b"" and enc.decode_targets(plan, empty, "sam") == plan.sam_header()


def _cli(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def test_cli_regions_and_bed(enc, small, tmp_path):
    d, plan = small, small["plan"]
    (tmp_path / "in.cbc").write_bytes(d["blob"]); (tmp_path / "ref.fa").write_bytes(d["fa"])
    files = (tmp_path / "in.cbc", tmp_path / "out.txt", tmp_path / "ref.fa")
    # two regions that share a read: written once (the parent kept only the last --region)
    _, info = tm.special_set(d["pb"], d["recs"], d["block_reads"])
    a, b = info["two"]
    two = [x for s in tm.region_strings([a, b], NAMES) for x in ("--region", s.decode())]
    r = _cli("-x", *files, *two)
    assert r.returncode == 0, r.stderr
    got = (tmp_path / "out.txt").read_bytes()
    assert got == tm.expected_reads(d["recs"], [a, b])
    assert got != rm.expected_text(d["recs"], *b) and got != rm.expected_text(d["recs"], *a)     # neither region alone
    assert got.count(info["read"][4] + b"\n") == sum(1 for x in d["recs"] if x[4] == info["read"][4])
    # repeated --region, a BED file, both together: reads, --sam, --depth
    ivs = _sets(d)["special"]
    merged = tm.merge(ivs)
    reads, sam, (depth, runs) = _want(d, merged)
    (tmp_path / "all.bed").write_bytes(b"# panel\n" + tm.bed(ivs, NAMES) + b"chrUn_x\t5\t50\n")
    (tmp_path / "half.bed").write_bytes(tm.bed(ivs[len(ivs) // 2:], NAMES))
    rs = [x for s in tm.region_strings(ivs, NAMES) for x in ("--region", s.decode())]
    forms = [rs, ["--regions-file", tmp_path / "all.bed"], rs[:2 * (len(ivs) // 2)] + ["--regions-file", tmp_path / "half.bed"]]
    for form in forms:
        for extra, want in (((), reads), (("--sam",), sam), (("--depth",), depth)):
            r = _cli("-x", *files, *form, *extra, "--verbose")
            assert r.returncode == 0, r.stderr
            assert (tmp_path / "out.txt").read_bytes() == want, (form, extra)
            assert "kernels: decode" in r.stdout and "intervals after merging" in r.stdout
    assert "1 BED lines selected nothing" in _cli("-x", *files, "--regions-file", tmp_path / "all.bed", "--verbose").stdout
    r = _cli("-x", *files, "--regions-file", tmp_path / "all.bed", "--depth", "--depth-exclude-flags", "16")
    assert r.returncode == 0 and (tmp_path / "out.txt").read_bytes() == _want(d, merged, 16)[2][0]
    # one --region and no file: the single-region code, its bytes and its report
    enc.upload_reference(plan.ref)
    for extra, want in (((), enc.decode_region(plan, "chr1:1000-9000")), (("--sam",), enc.decode_sam(plan, "chr1:1000-9000")),
                        (("--depth",), enc.decode_depth(plan, "chr1:1000-9000"))):
        r = _cli("-x", *files, "--region", "chr1:1000-9000", *extra)
        assert r.returncode == 0 and (tmp_path / "out.txt").read_bytes() == want and "intervals" not in r.stdout, r.stdout
    r = _cli("-x", *files)
    assert r.returncode == 0 and (tmp_path / "out.txt").read_bytes() == b"".join(x[4] + b"\n" for x in d["recs"])


def _spans(pb):
    """Packer-derived span of every record, vectorised (fixed-length reads of the C generator): the recipe of
    tests/test_region_gpu.py."""
    n = pb.n_recs
    rec_blk = np.repeat(np.arange(pb.n_blocks), pb.blocks["n_reads"].astype(np.int64))
    tok_at = pb.blocks["tok_base"][rec_blk].astype(np.int64) + pb.recs["tok_off"].astype(np.int64) + 1
    w1 = pb.tok[tok_at].astype(np.int64)
    rl = pb.recs["rlen"].astype(np.int64)
    L = int(rl[0])
    assert (rl == L).all()
    s0 = pb.blocks["seq_base"][rec_blk].astype(np.int64) + pb.recs["seq_off"].astype(np.int64)
    r0 = pb.blocks["ref_off"][rec_blk].astype(np.int64) + pb.recs["pos"].astype(np.int64) - 1
    k = np.arange(L)
    perfect = (pb.seq[s0[:, None] + k] == pb.ref[r0[:, None] + k]).all(axis=1)
    return np.where(perfect, rl, rl + (w1 & 0xff) - ((w1 >> 16) & 0xff))


def test_mid_size_panel(enc, built):
    """100 000 x 150 bp indel-rich reads on one contig in 4096-read blocks (the parameters of test_region_gpu.big, a tenth of
    it), 2000 seeded intervals of 1 to 2000 bases."""
    pb = host.synth(0xCBC0BEEF, 3_000_000, 100_000, 150, sub_rate=0.004, indel_frac=0.3, block_reads=4096)
    enc.upload_reference(pb.ref)
    _, res, offs, flat = enc.encode_blocks(pb, want_payload_list=False)
    assert (res["status"] == 0).all()
    c = pb.contigs[0]
    clen = int(c["length"])
    fa = synth.fasta_text([("chr1", pb.ref[int(c["ref_off"]): int(c["ref_off"]) + clen])])
    plan = host.UnpackPlan(pb.container(flat, offs), fa)
    enc.upload_reference(plan.ref)
    rng = np.random.default_rng(2000)
    beg = rng.integers(1, clen + 1, 2000)
    ivs = [(0, int(b), min(clen, int(b) + int(w) - 1)) for b, w in zip(beg, rng.integers(1, 2001, 2000))]
    merged = tm.merge(ivs)
    ts = plan.targets((), tm.bed(ivs, [b"chr1"]))
    assert ts.intervals() == merged and 100 < len(merged) < 2000 and 0 < ts.n_blocks <= plan.n_blocks
    # reads and SAM: the full decode, filtered on the host by the packer-derived spans
    spans = _spans(pb).astype(np.int64)
    blk = np.repeat(np.arange(pb.n_blocks), pb.blocks["n_reads"].astype(np.int64))
    pos = pb.info["window_start"][blk].astype(np.int64) + pb.recs["pos"].astype(np.int64)
    mb = np.array([m[1] for m in merged], dtype=np.int64); me = np.array([m[2] for m in merged], dtype=np.int64)
    j = np.searchsorted(me, pos)                                            # the first interval that ends at or behind POS
    keep = (j < len(merged)) & (mb[np.minimum(j, len(merged) - 1)] <= pos + spans - 1)
    assert 1000 < int(keep.sum()) < pb.n_recs
    recs, seq, _ = enc.decode_blocks(plan)
    st = plan.seq_stride
    rows = [seq[i * st:i * st + int(recs[i]["rlen"])].tobytes() for i in np.flatnonzero(keep)]
    text, n, _, res = enc.decode_targets(plan, ts, "reads", results=True)
    assert len(res) == ts.n_blocks and (res["status"] == 0).all()           # blocks outside the selection are not decoded
    assert ts.n_blocks < plan.n_blocks or len(merged) > 500
    assert n == int(keep.sum()) and text == b"".join(r + b"\n" for r in rows)
    ms = enc.last_targets_ms()
    print("targets kernel ms (decode, filter + scan, -, text):", ms)
    assert len(ms) == 4 and all(x >= 0 for x in ms) and ms[0] > 0
    import sammodel as sm
    want = plan.sam_header() + b"".join(sm.line(int(recs[i]["flag"]), b"chr1", int(pos[i]), r) for i, r in zip(np.flatnonzero(keep), rows))
    text, n, _, res = enc.decode_targets(plan, ts, "sam", results=True)
    assert len(res) == ts.n_blocks and n == int(keep.sum()) and text == want
    # depth: Encoder.decode_depth per merged interval, appended
    want = b"".join(enc.decode_depth(plan, "chr1:%d-%d" % (b, e)) for _, b, e in merged)
    text, _, runs, res = enc.decode_targets(plan, ts, "depth", results=True)
    assert len(res) == ts.n_blocks and text == want and runs == want.count(b"\n") > 1000
    ms = enc.last_targets_ms()
    print("targets depth kernel ms (decode, mark, scan + compact, text):", ms)
    assert all(x >= 0 for x in ms)
    plan.close(); pb.close()


def test_failed_block_contributes_nothing(enc, small):
    """A payload byte of block 1 flipped: the block fails to decode (an error status, no fault), the call returns CBC_E_BLOCK,
    and the block's reads are missing from every output."""
    d = small
    blob = bytearray(d["blob"])
    base = len(blob) - d["plan"].payloads.size
    blob[base + int(d["plan"].blocks[1]["in_off"]) + int(d["plan"].blocks[1]["in_bytes"]) // 2] ^= 0x55
    plan = host.UnpackPlan(bytes(blob), d["fa"])
    enc.upload_reference(plan.ref)
    ivs = _sets(d)["random200"]
    merged = tm.merge(ivs)
    ts = plan.targets(tm.region_strings(ivs, NAMES))
    assert ts.blocks[1] == 1
    recs_wo = [r for r in d["recs"] if r[0] != 1]
    flags_wo = [f for f, r in zip(d["flags"], d["recs"]) if r[0] != 1]
    text, n, _, res = enc.decode_targets(plan, ts, "reads", results=True)
    assert [b for b in range(ts.n_blocks) if res[b]["status"] != 0] == [1]
    assert text == tm.expected_reads(recs_wo, merged) != tm.expected_reads(d["recs"], merged)
    text, n, _, res = enc.decode_targets(plan, ts, "sam", results=True)
    assert text == plan.sam_header() + tm.expected_sam(recs_wo, flags_wo, NAMES, merged)
    text, _, runs, res = enc.decode_targets(plan, ts, "depth", results=True)
    assert (text, runs) == tm.expected_depth(d["iv"], NAMES, d["lens"], merged, 0, (1,))
    for out in ("reads", "sam", "depth"):
        with pytest.raises(gpu.CbcGpuError, match=r"block 1\b"):
            enc.decode_targets(plan, ts, out)
    d_ok = d["plan"]
    enc.upload_reference(d_ok.ref)
    assert enc.decode_targets(d_ok, d_ok.targets(tm.region_strings(ivs, NAMES))) == tm.expected_reads(d["recs"], merged)
    plan.close()


def test_cli_refusals(built, small, tmp_path):
    d = small
    (tmp_path / "in.cbc").write_bytes(d["blob"]); (tmp_path / "ref.fa").write_bytes(d["fa"])
    (tmp_path / "t.bed").write_bytes(b"chr1\t10\t20\n")
    (tmp_path / "bad.bed").write_bytes(b"chr1\t10\t20\n\nchr1\t30\n")
    files = (tmp_path / "in.cbc", tmp_path / "o.txt", tmp_path / "ref.fa")
    two = ("--region", "chr1:1-5", "--region", "chr2:1-5")
    for args, msg in [(two + ("--devices", "0,1"), "one device"), (("--regions-file", tmp_path / "t.bed", "--devices", "0,1"), "one device"),
                      (two + ("--depth", "--sam"), "--depth and --sam"), (("--region", "chr1:1-5", "--region", "chrX:1-5"), "unknown contig"),
                      (("--region", "chr1:9-5", "--regions-file", tmp_path / "t.bed"), "ends before"),
                      (("--regions-file", tmp_path / "bad.bed"), "BED line 3: fewer than three columns")]:
        r = _cli("-x", *files, *args)
        assert r.returncode == 1 and msg in r.stderr, (args, r.stderr)
    r = _cli("-c", tmp_path / "in.sam", tmp_path / "o.cbc", tmp_path / "ref.fa", *two)
    assert r.returncode == 1 and "--region applies to decompression" in r.stderr, r.stderr
    r = _cli("-c", tmp_path / "in.sam", tmp_path / "o.cbc", tmp_path / "ref.fa", "--regions-file", tmp_path / "t.bed")
    assert r.returncode == 1 and "--regions-file applies to decompression" in r.stderr, r.stderr
    fa, sam, _, _ = synth.dataset(4, [5000], [100], 100)
    (tmp_path / "c.cbc").write_bytes(oracle.encode(sam, fa)); (tmp_path / "c.fa").write_bytes(fa)
    r = _cli("-x", tmp_path / "c.cbc", tmp_path / "o.txt", tmp_path / "c.fa", *two)
    assert r.returncode == 1 and "single-stream (--compat) file" in r.stderr, r.stderr
    pb, _, lfa = host.synth_long(5, 200_000, 40, read_len=2000, want_text=True)
    flat, offs, _ = oracle.cpu_encode_blocks(pb, long_reads=True, return_flat=True)
    (tmp_path / "l.cbc").write_bytes(pb.container(flat, offs)); (tmp_path / "l.fa").write_bytes(lfa)
    r = _cli("-x", tmp_path / "l.cbc", tmp_path / "o.txt", tmp_path / "l.fa", "--regions-file", tmp_path / "t.bed", "--sam")
    assert r.returncode == 1 and "long-read" in r.stderr, r.stderr
    pb.close()
    b = bytearray(d["blob"]); b[36 + 2] = 9                                   # a tab inside "chr1": refused for plain reads too
    (tmp_path / "t.cbc").write_bytes(bytes(b))
    r = _cli("-x", tmp_path / "t.cbc", tmp_path / "o.txt", tmp_path / "ref.fa", "--region", "chr2:1-5", "--region", "chr2:9-10")
    assert r.returncode == 1 and "holds a tab or a newline" in r.stderr, r.stderr
