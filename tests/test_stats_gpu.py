"""Read statistics on the MI355X: Encoder.decode_stats and `cbc -x --stats` against the brute-force
model (statsmodel.py) on the fabricated shapes, on blocks of 1, 63, 64 and 65 reads, on the mixed dataset of the other GPU tests
with and without regions and exclusion, on the mid-size panel, with a failed block, and the CLI's refusals; and identities
against decode_sam and decode_targets, which are not under test.  Every comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

import depthmodel as dm
import regionmodel as rm
import statsmodel as sm
import synth
import targetsmodel as tm
from cbc_amd import gpu, host
from oracle import oracle
from test_region import _dataset
from test_targets_gpu import _spans

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cbc_amd", "csrc", "cbc")


@pytest.fixture(scope="module")
def enc():
    e = gpu.Encoder(0)
    yield e
    e.close()


def _wrap(fa, pb, reads, names):
    blob = rm.container(pb)
    return dict(fa=fa, pb=pb, blob=blob, plan=host.UnpackPlan(blob, fa), reads=reads, names=names, iv=dm.intervals_a(pb))


@pytest.fixture(scope="module")
def shapes(built):
    fa, sam, pb, contigs, same_at = sm.shapes(64)
    d = _wrap(fa, pb, sm.assert_models_agree(pb, sam), [n.encode() for n, _ in contigs])
    d["same_at"] = same_at
    yield d
    d["plan"].close(); pb.close()


@pytest.fixture(scope="module")
def mixed(built):
    fa, pb, contigs = _dataset(7 + 64, 64)                    # the mixed dataset of the other GPU tests at block_reads 64
    d = _wrap(fa, pb, sm.reads_from_packed(pb), [n.encode() for n, _ in contigs])
    yield d
    d["plan"].close(); pb.close()


def _cli(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def _check(enc, d, given=None, regions=(), extra_bed=b"", exclude=0, cli_dir=None):
    """decode_stats (and, with cli_dir, `cbc -x --stats` on the same selection) against the model.  given: [(contig, beg, end)]
    as a BED text (None: the whole file); regions: [(string, interval)].  Returns (tables, target set or None)."""
    plan = d["plan"]
    ts, keep, bed = None, None, None
    if given is not None or regions:
        bed = tm.bed(given or [], d["names"]) + extra_bed
        ts = plan.targets([r for r, _ in regions], bed)
        keep = sm.selected(d["iv"], [q for _, q in regions] + list(given or []))
    got = enc.decode_stats(plan, ts, exclude)
    want = sm.tables(d["reads"], exclude, keep)
    assert sm.same(got, want), sm.diff(got, want)
    assert got["reads"] + got["excluded"] == (len(d["reads"]) if keep is None else int(keep.sum()))
    assert all(got[k].dtype == np.uint32 for k in ("flag", "len", "gc", "cyc")) and got["cyc"].shape == (5, 256)
    assert host.stats_text(got) == sm.text(want)
    if cli_dir is not None:
        (cli_dir / "in.cbc").write_bytes(d["blob"]); (cli_dir / "ref.fa").write_bytes(d["fa"])
        args = [x for r, _ in regions for x in ("--region", r.decode())]
        if bed:
            (cli_dir / "q.bed").write_bytes(bed)
            args += ["--regions-file", cli_dir / "q.bed"]
        if exclude:
            args += ["--stats-exclude-flags", exclude]
        r = _cli("-x", cli_dir / "in.cbc", cli_dir / "out.txt", cli_dir / "ref.fa", "--stats", "--verbose", *args)
        assert r.returncode == 0, r.stderr
        assert (cli_dir / "out.txt").read_bytes() == sm.text(want)
        assert "statistics of %d reads (%d excluded)" % (want["reads"], want["excluded"]) in r.stdout
        assert ("kernels: decode" in r.stdout) == (ts is None or ts.n_blocks > 0)
    return got, ts


def test_shapes_python_and_cli(enc, shapes, tmp_path):
    """Lengths 1 .. 252 on both strands, N at the first and last base and in the dword that straddles the length, all-G and all-A
    reads, every FLAG of the list (one above the LDS bound), a block whose 64 reads carry one FLAG; exclusion 0, 16 and 0x400."""
    d = shapes
    pb = d["pb"]
    assert {len(s) for _, s in d["reads"]} >= set(sm.LENGTHS) and {f for f, _ in d["reads"]} >= set(sm.FLAGS) and max(sm.FLAGS) >= 4096
    first = int(pb.blocks[d["same_at"] // 64]["rec_base"])
    assert d["same_at"] % 64 == 0 and set(pb.recs["flag"][first:first + 64].tolist()) == {83}
    enc.upload_reference(d["plan"].ref)
    total = len(d["reads"])
    for ex in (0, 16, 0x400):
        got, _ = _check(enc, d, exclude=ex, cli_dir=tmp_path)
        assert got["reads"] + got["excluded"] == total and (got["excluded"] == 0) == (ex == 0)
    got, _ = _check(enc, d)
    assert got["gc"][0] >= 2 and got["gc"][100] >= 2 and got["cyc"][4].sum() > 0 and got["len"][252] >= 2 and got["len"][1] >= 2
    _check(enc, d, [(0, 1, 200), (1, 100, 400)], exclude=0x400, cli_dir=tmp_path)
    ms = enc.last_stats_ms()
    assert len(ms) == 2 and ms[0] > 0 and ms[1] > 0


def test_block_sizes(enc, built):
    """Blocks of 1, 63, 64 and 65 reads: the record-group boundary."""
    for n in (1, 63, 64, 65):
        fa, sam, _, contigs = synth.dataset(n, [20_000], [n + 64 + 3], 100, sub_rate=0.01)
        pb = host.pack_sam(sam, fa, block_reads=n, var_length=True)
        d = _wrap(fa, pb, sm.assert_models_agree(pb, sam), [b"chr1"])
        assert n in pb.blocks["n_reads"].tolist()
        enc.upload_reference(d["plan"].ref)
        _check(enc, d)
        _check(enc, d, exclude=16)
        d["plan"].close(); pb.close()


def test_mixed_dataset_regions_and_identities(enc, mixed, tmp_path):
    d = mixed
    plan = d["plan"]
    enc.upload_reference(plan.ref)
    L = [int(c["length"]) for c in d["pb"].contigs]
    got, _ = _check(enc, d, cli_dir=tmp_path)
    # identities against code that is not under test, on the same plan
    _, n_sam, _, _ = enc.decode_sam(plan, results=True)
    assert got["reads"] == n_sam == len(d["reads"])
    first = min(x[1] for x in d["iv"] if x[0] == 0)
    one = (0, first + 20, first + 160)
    rs = b"chr1:%d-%d" % one[1:]
    got, ts = _check(enc, d, regions=[(rs, one)], cli_dir=tmp_path)
    _, n_sam, _, _ = enc.decode_sam(plan, rs, results=True)
    assert got["reads"] == n_sam > 0
    ivs = [(0, first + 10, first + 40), (0, first + 41, first + 60), (0, first + 55, first + 120), (0, first + 10, first + 40),
           (len(L) - 1, 1, 300), (0, first, first), (0, first + 200, first + 201), (0, 1, 3), (1, 5000, 9000)]
    extra = b"chrUn_gl0\t5\t900\nchr1\t700\t700\n"
    for ex in (0, 16):
        got, ts = _check(enc, d, ivs, extra_bed=extra, exclude=ex, cli_dir=tmp_path)
        text, n_reads, _, _ = enc.decode_targets(plan, ts, output="reads", results=True)
        assert got["reads"] + got["excluded"] == n_reads and 0 < n_reads < len(d["reads"])
        if ex == 0:
            assert int((np.arange(257) * got["len"].astype(np.int64)).sum()) == len(text) - n_reads      # bases = text bytes - reads
    # the deletion read at the end of block 0, kept by its span
    dpos = int(d["pb"].recs[63]["pos"]) + int(d["pb"].info[0]["window_start"])
    got, _ = _check(enc, d, [(0, dpos + 130, dpos + 135)])
    assert got["len"][100] >= 1
    # a BED that selects nothing, and one that names only an unknown contig: nothing runs, all-zero tables
    for bed in (b"chr1\t5\t5\n", b"chrUn\t1\t500\n"):
        ts = plan.targets((), bed)
        assert ts.n_blocks == 0 and sm.same(enc.decode_stats(plan, ts), sm.zero_tables())
        (tmp_path / "e.bed").write_bytes(bed)
        r = _cli("-x", tmp_path / "in.cbc", tmp_path / "out.txt", tmp_path / "ref.fa", "--stats", "--regions-file", tmp_path / "e.bed")
        assert r.returncode == 0 and (tmp_path / "out.txt").read_bytes() == sm.text(sm.zero_tables()), r.stderr


def test_mid_size_panel(enc, built, tmp_path):
    """The 100 000-read dataset of test_hist_gpu.test_mid_size_panel: bins above 65 535 and many workgroups flushing into one
    table; the model comes from the packer's arrays.  Whole file, with exclusion, a 2000-line BED, and the CLI."""
    pb = host.synth(0xCBC0BEEF, 3_000_000, 100_000, 150, sub_rate=0.004, indel_frac=0.3, block_reads=4096)
    enc.upload_reference(pb.ref)
    _, res, offs, flat = enc.encode_blocks(pb, want_payload_list=False)
    assert (res["status"] == 0).all()
    c = pb.contigs[0]
    clen = int(c["length"])
    fa = synth.fasta_text([("chr1", pb.ref[int(c["ref_off"]): int(c["ref_off"]) + clen])])
    blob = pb.container(flat, offs)
    plan = host.UnpackPlan(blob, fa)
    enc.upload_reference(plan.ref)
    arr = sm.packed_arrays(pb)
    want = sm.tables(arr)
    assert want["reads"] == 100_000 and int(want["len"].max()) > 65_535 and int(want["cyc"].max()) > 0
    got = enc.decode_stats(plan)
    assert sm.same(got, want), sm.diff(got, want)
    print("statistics kernel ms (decode, zero + statistics):", enc.last_stats_ms())
    want16 = sm.tables(arr, 16)
    got = enc.decode_stats(plan, exclude_flags=16)
    assert sm.same(got, want16) and got["excluded"] > 0, sm.diff(got, want16)
    rng = np.random.default_rng(2000)
    beg = rng.integers(1, clen + 1, 2000)
    ivs = [(0, int(b), min(clen, int(b) + int(w) - 1)) for b, w in zip(beg, rng.integers(1, 2001, 2000))]
    blk = np.repeat(np.arange(pb.n_blocks), pb.blocks["n_reads"].astype(np.int64))
    pos = pb.info["window_start"][blk].astype(np.int64) + pb.recs["pos"].astype(np.int64)
    end = pos + _spans(pb).astype(np.int64) - 1
    keep = np.zeros(pb.n_recs, dtype=bool)
    for _, b, e in tm.merge(ivs):
        keep |= (pos <= e) & (end >= b)
    ts = plan.targets((), tm.bed(ivs, [b"chr1"]))
    wantp = sm.tables(arr, 0, keep)
    got = enc.decode_stats(plan, ts)
    assert sm.same(got, wantp) and 0 < got["reads"] < 100_000, sm.diff(got, wantp)
    _, n_reads, _, _ = enc.decode_targets(plan, ts, output="reads", results=True)
    assert got["reads"] == n_reads
    (tmp_path / "in.cbc").write_bytes(blob); (tmp_path / "ref.fa").write_bytes(fa)
    r = _cli("-x", tmp_path / "in.cbc", tmp_path / "out.txt", tmp_path / "ref.fa", "--stats", "--stats-exclude-flags", 16)
    assert r.returncode == 0 and (tmp_path / "out.txt").read_bytes() == sm.text(want16), r.stderr
    plan.close(); pb.close()


def test_failed_block_zeroes_every_table(enc, mixed):
    """A payload byte of block 1 flipped: the block fails to decode (an error status, no fault), the call reports CBC_E_BLOCK
    naming the block and every table stays zero; the next good call is correct again."""
    d = mixed
    blob = bytearray(d["blob"])
    base = len(blob) - d["plan"].payloads.size
    blob[base + int(d["plan"].blocks[1]["in_off"]) + int(d["plan"].blocks[1]["in_bytes"]) // 2] ^= 0x55
    plan = host.UnpackPlan(bytes(blob), d["fa"])
    enc.upload_reference(plan.ref)
    got, res = enc.decode_stats(plan, results=True)
    assert [b for b in range(len(res)) if res[b]["status"] != 0] == [1]
    assert sm.same(got, sm.zero_tables())
    with pytest.raises(gpu.CbcGpuError, match=r"block 1\b"):
        enc.decode_stats(plan)
    ts = plan.targets([b"chr1"])
    got, res = enc.decode_stats(plan, ts, results=True)
    assert [b for b in range(len(res)) if res[b]["status"] != 0] == [1] and sm.same(got, sm.zero_tables())
    enc.upload_reference(d["plan"].ref)
    _check(enc, d)
    plan.close()


def test_cli_refusals(built, mixed, tmp_path):
    d = mixed
    (tmp_path / "in.cbc").write_bytes(d["blob"]); (tmp_path / "ref.fa").write_bytes(d["fa"])
    (tmp_path / "bad.bed").write_bytes(b"chr1\t10\t20\n\nchr1\t30\n")
    files = (tmp_path / "in.cbc", tmp_path / "o.txt", tmp_path / "ref.fa")
    for args, msg in [(("--stats", "--sam"), "different outputs"), (("--stats", "--depth"), "different outputs"),
                      (("--stats", "--bedcov"), "different outputs"), (("--stats", "--depth-hist"), "different outputs"),
                      (("--stats", "--devices", "0,1"), "one device"), (("--stats-exclude-flags", "16"), "--stats-exclude-flags applies to --stats"),
                      (("--stats", "--region", "chr1:9-5"), "ends before"),
                      (("--stats", "--regions-file", tmp_path / "bad.bed"), "BED line 3: fewer than three columns")]:
        r = _cli("-x", *files, *args)
        assert r.returncode == 1 and msg in r.stderr, (args, r.stderr)
    r = _cli("-c", tmp_path / "in.sam", tmp_path / "o.cbc", tmp_path / "ref.fa", "--stats")
    assert r.returncode == 1 and "--stats applies to decompression" in r.stderr, r.stderr
    fa, sam, _, _ = synth.dataset(4, [5000], [100], 100)
    (tmp_path / "c.cbc").write_bytes(oracle.encode(sam, fa)); (tmp_path / "c.fa").write_bytes(fa)
    r = _cli("-x", tmp_path / "c.cbc", tmp_path / "o.txt", tmp_path / "c.fa", "--stats")
    assert r.returncode == 1 and "single-stream (--compat) file" in r.stderr, r.stderr
    pb, _, lfa = host.synth_long(5, 200_000, 40, read_len=2000, want_text=True)
    flat, offs, _ = oracle.cpu_encode_blocks(pb, long_reads=True, return_flat=True)
    (tmp_path / "l.cbc").write_bytes(pb.container(flat, offs)); (tmp_path / "l.fa").write_bytes(lfa)
    r = _cli("-x", tmp_path / "l.cbc", tmp_path / "o.txt", tmp_path / "l.fa", "--stats")
    assert r.returncode == 1 and "long-read" in r.stderr, r.stderr
    pb.close()
