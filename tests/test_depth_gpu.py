"""Coverage output on the MI355X: Encoder.decode_depth and `cbc -x --depth`, whole containers and
windows, against the codec's view of every read (model (a), depthmodel.py) and, where the input has no soft clips, against the
SAM text that was compressed (model (b)); genome-shaped input; a million reads; a failed block; determinism."""
import os
import subprocess

import numpy as np
import pytest

import depthmodel as dm
import regionmodel as rm
from cbc_amd import gpu, host
from test_genome_shapes import check_features, genome
from test_region_gpu import _spans

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cbc_amd", "csrc", "cbc")
FLAGS = (0, 16, 99, 147, 1040, 2064)


@pytest.fixture(scope="module")
def enc():
    e = gpu.Encoder(0)
    yield e
    e.close()


def _open(fa, sam, pb, contigs, **extra):
    blob = rm.container(pb)
    names, lens = dm.names_lens(None, contigs)
    return dict(fa=fa, sam=sam, pb=pb, blob=blob, plan=host.UnpackPlan(blob, fa), names=names, lens=lens, **extra)


@pytest.fixture(scope="module", params=[256, 1024])
def small(request, built):
    """No soft clips: models (a) and (b) must agree on every read, then either is ground truth."""
    d = _open(*dm.mixed(7 + request.param, request.param, flags=FLAGS), block_reads=request.param)
    d["iv"] = dm.assert_models_agree(d["pb"], d["sam"])
    assert {x[3] for x in d["iv"]} == set(FLAGS)
    yield d
    d["plan"].close(); d["pb"].close()


def test_whole_container_matches_both_models(enc, small):
    plan, iv = small["plan"], small["iv"]
    enc.upload_reference(plan.ref)
    want = dm.expected(iv, small["names"], small["lens"])
    assert want == dm.expected(dm.intervals_b(small["sam"]), small["names"], small["lens"])
    text, runs, kept, res = enc.decode_depth(plan, results=True)
    assert (res["status"] == 0).all() and len(res) == plan.n_blocks
    assert (text, runs, kept) == want and kept == small["pb"].n_recs
    assert enc.decode_depth(plan) == want[0]
    ms = enc.last_depth_ms()
    assert len(ms) == 4 and ms[0] > 0 and all(x >= 0 for x in ms)


def test_windows_match_the_model(enc, small):
    plan, iv = small["plan"], small["iv"]
    enc.upload_reference(plan.ref)
    ivb = dm.intervals_b(small["sam"])
    wins = dm.windows(small["pb"], iv, small["block_reads"], small["lens"], 100, 11)
    n_hit = 0
    for s, c, beg, end in wins:
        want = dm.expected(iv, small["names"], small["lens"], (c, beg, end))
        assert want == dm.expected(ivb, small["names"], small["lens"], (c, beg, end)), s
        text, runs, kept, res = enc.decode_depth(plan, s, results=True)
        assert (res["status"] == 0).all(), s
        assert (text, runs, kept) == want, s
        n_hit += bool(text)
    assert len(wins) >= 130 and n_hit >= 0.7 * len(wins) and len(wins) - n_hit >= 4, (len(wins), n_hit)


def test_exclude_flags(enc, small):
    plan, iv = small["plan"], small["iv"]
    enc.upload_reference(plan.ref)
    for ex in (16, 0x704, 0xffff):
        want = dm.expected(iv, small["names"], small["lens"], None, ex)
        text, runs, kept, _ = enc.decode_depth(plan, exclude_flags=ex, results=True)
        assert (text, runs, kept) == want, ex
        assert kept == sum(1 for x in iv if not x[3] & ex)
    assert dm.expected(iv, small["names"], small["lens"], None, 16)[0] == \
        dm.expected([x for x in iv if not x[3] & 16], small["names"], small["lens"])[0]


def test_soft_clips_the_codecs_view_rules(enc, built):
    """Trailing soft clips: the packer codes them as insertions, so span = M + D as in the SAM -- except where the clipped
    bases equal the reference and the read is coded as perfect.  Model (a) alone is the truth here."""
    d = _open(*dm.mixed(31, 512, flags=FLAGS, trailing_s_frac=0.15), block_reads=512)
    plan, iv = d["plan"], dm.intervals_a(d["pb"])
    assert sum(1 for ln in d["sam"].split(b"\n") if b"S\t" in ln) > 300
    enc.upload_reference(plan.ref)
    text, runs, kept, res = enc.decode_depth(plan, results=True)
    assert (res["status"] == 0).all() and (text, runs, kept) == dm.expected(iv, d["names"], d["lens"])
    for s, c, beg, end in dm.windows(d["pb"], iv, 512, d["lens"], 20, 3):
        assert enc.decode_depth(plan, s, results=True)[:3] == dm.expected(iv, d["names"], d["lens"], (c, beg, end)), s
    plan.close(); d["pb"].close()


def test_genome_shaped_input(enc, built):
    """N gaps, IUPAC codes and soft-masking in the reference, N-rich reads: model (a) from the packed arrays."""
    fa, sam, rbc, contigs = genome()
    check_features(rbc, contigs)
    pb = host.pack_sam(sam, fa, block_reads=1024)
    plan = host.UnpackPlan(rm.container(pb), fa)
    enc.upload_reference(plan.ref)
    iv = dm.intervals_a(pb)
    names, lens = dm.names_lens(None, contigs)
    assert [plan.names[int(o):].tobytes().split(b"\0")[0] for o in plan.contig_name_off] == names
    text, runs, kept, res = enc.decode_depth(plan, results=True)
    assert (res["status"] == 0).all() and kept == pb.n_recs
    assert (text, runs, kept) == dm.expected(iv, names, lens)
    rng = np.random.default_rng(4)
    for _ in range(12):
        c = int(rng.integers(0, len(lens)))
        beg = int(rng.integers(1, lens[c]))
        end = min(lens[c], beg + int(rng.choice([0, 500, 30_000])))
        got = enc.decode_depth(plan, b"%s:%d-%d" % (names[c], beg, end), results=True)[:3]
        assert got == dm.expected(iv, names, lens, (c, beg, end)), (c, beg, end)
    plan.close(); pb.close()


def test_a_million_reads(enc, built):
    """1 M indel-rich reads in 4096-read blocks on a 30 Mb contig: the depth summed over the runs equals the kept spans
    inside the window, and the bytes equal the model's."""
    pb = host.synth(0xCBC0BEEF, 30_000_000, 1_000_000, 150, sub_rate=0.004, indel_frac=0.3, block_reads=4096)
    enc.upload_reference(pb.ref)
    _, res, offs, flat = enc.encode_blocks(pb, want_payload_list=False)
    assert (res["status"] == 0).all()
    c0 = pb.contigs[0]
    import synth
    fa = synth.fasta_text([("chr1", pb.ref[int(c0["ref_off"]): int(c0["ref_off"]) + int(c0["length"])])])
    plan = host.UnpackPlan(pb.container(flat, offs), fa)
    enc.upload_reference(plan.ref)
    spans = _spans(pb).astype(np.int64)
    blk = np.repeat(np.arange(pb.n_blocks), pb.blocks["n_reads"].astype(np.int64))
    pos = pb.info["window_start"][blk].astype(np.int64) + pb.recs["pos"].astype(np.int64)
    clen = int(c0["length"])
    assert (spans != 150).sum() > 100_000 and plan.n_blocks > 200
    for region, beg, end in ((None, 1, clen), ("chr1:10000001-20000000", 10_000_001, 20_000_000)):
        text, runs, kept, res = enc.decode_depth(plan, region, results=True)
        assert (res["status"] == 0).all()
        keep = (pos <= end) & (pos + spans - 1 >= beg) & (spans >= 1)
        s, e = np.maximum(pos[keep], beg), np.minimum(pos[keep] + spans[keep] - 1, end)
        rows = np.array([ln.split(b"\t")[1:] for ln in text.split(b"\n")[:-1]], dtype=np.int64)
        assert kept == int(keep.sum()) and runs == len(rows)
        assert int(((rows[:, 1] - rows[:, 0]) * rows[:, 2]).sum()) == int((e - s + 1).sum())      # summed once, on the host
        diff = np.zeros(end - beg + 2, dtype=np.int64)
        np.add.at(diff, s - beg, 1); np.add.at(diff, e + 1 - beg, -1)
        want, nruns = dm.bedgraph(b"chr1", beg, np.cumsum(diff[:-1]))
        assert nruns == runs and text == want
        if region is None:
            assert runs > 1_000_000 and kept == pb.n_recs and enc.decode_depth(plan) == text       # twice: identical bytes
    plan.close(); pb.close()


def test_determinism(enc, small):
    plan = small["plan"]
    enc.upload_reference(plan.ref)
    a = enc.decode_depth(plan)
    for _ in range(3):
        assert enc.decode_depth(plan) == a
    assert enc.decode_depth(plan, "chr1:1000-30000") == enc.decode_depth(plan, "chr1:1000-30000")


def test_text_cap_one_byte_short(enc, small):
    plan, iv = small["plan"], small["iv"]
    enc.upload_reference(plan.ref)
    want = dm.expected(iv, small["names"], small["lens"], (1, 1, small["lens"][1]))[0]
    with pytest.raises(gpu.CbcGpuError, match="text_cap too small"):
        enc.decode_depth(plan, "chr2", text_cap=len(want) - 1)
    assert enc.last_depth_text_bytes == len(want)
    assert enc.decode_depth(plan, "chr2", text_cap=len(want)) == want


def test_failed_block_marks_nothing(enc, built):
    """The way the region tests fail a block: a span bound one below the longest span gives CBC_ST_SPAN for the blocks that
    hold a read of that span, and for no other.  In the shared datasets every block holds a read of the longest span (150
    bases and three deleted), so this one gives the last read of blocks 1 and 3 a 40-base deletion in 150 bases, 190 on the
    reference, which no other read reaches.  The two blocks contribute nothing and the call reports CBC_E_BLOCK."""
    import synth
    BR, bad = 256, [1, 3]
    fa, rbc, contigs = rm.mixed_dataset(19, [60_000, 45_000, 20_000], [1500, 700, 400], sub_rate=0.004, indel_frac=0.3, gap_tail=3000)
    recs = rbc[0][2]
    for b in bad:
        recs[(b + 1) * BR - 1] = rm.deletion_read(contigs[0][1], recs[(b + 1) * BR - 1]["pos"], 75, 40, 75)
    sam = synth.sam_text(rbc)
    d = _open(fa, sam, host.pack_sam(sam, fa, block_reads=BR, var_length=True), contigs)
    plan, names, lens = d["plan"], d["names"], d["lens"]
    iv = dm.assert_models_agree(d["pb"], sam)
    chr1 = [x for x in iv if x[0] == 0]
    n_blocks = len({x[4] for x in chr1})
    assert max(x[2] for x in chr1) == 190 and sorted({x[4] for x in chr1 if x[2] == 190}) == bad and n_blocks >= 5
    assert max(x[2] for x in chr1 if x[2] != 190) < 189
    enc.upload_reference(plan.ref)
    text, runs, kept, res = enc.decode_depth(plan, "chr1", results=True, smax=189)
    assert len(res) == n_blocks and [b for b in range(n_blocks) if res[b]["status"] != 0] == bad
    assert (res["status"][bad] == 8).all()
    want = dm.expected(iv, names, lens, (0, 1, lens[0]), 0, tuple(bad))
    assert (text, runs, kept) == want and kept == sum(1 for x in chr1 if x[4] not in bad) > 0
    assert text != dm.expected(iv, names, lens, (0, 1, lens[0]))[0]        # the two blocks' reads are missing from the track
    with pytest.raises(gpu.CbcGpuError, match=r"block 1\b"):
        enc.decode_depth(plan, "chr1", smax=189)
    assert enc.decode_depth(plan, "chr1") == dm.expected(iv, names, lens, (0, 1, lens[0]))[0]
    plan.close(); d["pb"].close()


def _cli(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def test_cli_depth(enc, small, tmp_path):
    plan, iv, names, lens = small["plan"], small["iv"], small["names"], small["lens"]
    (tmp_path / "in.cbc").write_bytes(small["blob"]); (tmp_path / "ref.fa").write_bytes(small["fa"])
    files = (tmp_path / "in.cbc", tmp_path / "out.bg", tmp_path / "ref.fa")
    r = _cli("-x", *files, "--depth", "--verbose")
    assert r.returncode == 0, r.stderr
    got = (tmp_path / "out.bg").read_bytes()
    enc.upload_reference(plan.ref)
    per_contig = [enc.decode_depth(plan, n) for n in names]                   # the contigs' own texts, in table order
    assert got == b"".join(per_contig) == dm.expected(iv, names, lens)[0] and all(per_contig)
    for w in ("kernels: decode", "mark", "scan + compact", "text"):
        assert w in r.stdout, r.stdout
    for s, c, beg, end in dm.windows(small["pb"], iv, small["block_reads"], lens, 3, 5)[:3] + [("chr2:100-9000", 1, 100, 9000), ("chr3", 2, 1, lens[2])]:
        r = _cli("-d", *files, "--depth", "--region", s)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / "out.bg").read_bytes() == dm.expected(iv, names, lens, (c, beg, end))[0], s
    r = _cli("-x", *files, "--depth", "--depth-exclude-flags", "16")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "out.bg").read_bytes() == dm.expected([x for x in iv if not x[3] & 16], names, lens)[0]
    r = _cli("-x", *files, "--depth", "--depth-exclude-flags", "0x704", "--region", "chr1")
    assert r.returncode == 0 and (tmp_path / "out.bg").read_bytes() == dm.expected(iv, names, lens, (0, 1, lens[0]), 0x704)[0]
    # the other outputs give the bytes they gave before
    r = _cli("-x", tmp_path / "in.cbc", tmp_path / "all.txt", tmp_path / "ref.fa")
    assert r.returncode == 0 and (tmp_path / "all.txt").read_bytes() == b"".join(x[4] + b"\n" for x in rm.records(small["pb"]))
