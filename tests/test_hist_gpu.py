"""Depth histogram on the MI355X: Encoder.decode_depth_hist and `cbc -x --depth-hist` against the
brute-force model (histmodel.py) on the small datasets of the other GPU tests, two identities against the existing
Encoder.decode_coverage on the same selection, a pile-up deeper than CBC_HIST_LDS (the direct-global path), the mid-size panel
with a 2000-line BED, a failed block, and the CLI's refusals.  Every comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

import covmodel as cm
import depthmodel as dm
import histmodel as hm
import regionmodel as rm
import synth
import targetsmodel as tm
from cbc_amd import gpu, host
from oracle import oracle
from test_region import _dataset
from test_targets_gpu import _spans

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cbc_amd", "csrc", "cbc")
NAMES = [b"chr1", b"chr2", b"chr3"]


@pytest.fixture(scope="module")
def enc():
    e = gpu.Encoder(0)
    yield e
    e.close()


def _wrap(fa, pb, names, lens, iv):
    blob = rm.container(pb)
    return dict(fa=fa, pb=pb, blob=blob, plan=host.UnpackPlan(blob, fa), names=names, lens=lens, iv=iv, depth=cm.Depth(iv, lens))


@pytest.fixture(scope="module")
def mixed(built):
    fa, pb, contigs = _dataset(7 + 64, 64)                    # the mixed dataset of the other GPU tests at block_reads 64
    d = _wrap(fa, pb, NAMES, [len(c) for _, c in contigs], dm.intervals_a(pb))
    yield d
    d["plan"].close(); pb.close()


@pytest.fixture(scope="module")
def ramp(built):
    fa, sam, pb, contigs = dm.ramp()
    names, lens = dm.names_lens(None, contigs)
    d = _wrap(fa, pb, names, lens, dm.assert_models_agree(pb, sam))
    yield d
    d["plan"].close(); pb.close()


def _cli(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def _check(enc, d, ts, given, exclude=0, max_depth=0, depth=None):
    got = enc.decode_depth_hist(d["plan"], ts, exclude, max_depth)
    for _, dep, bases, size in got:
        assert dep.dtype == np.uint32 and bases.dtype == np.uint64 and int(bases.sum()) == size and (bases > 0).all()
    want = hm.expected(depth or d["depth"], d["lens"], given, max_depth)
    rows = hm.as_rows(got)
    assert rows == want, [(a, b) for a, b in zip(rows, want) if a != b][:2]
    return want


def _forms(d):
    """(name, region strings, intervals of a BED text, extra BED text, the intervals the model takes)."""
    L, names = d["lens"], d["names"]
    first = min(x[1] for x in d["iv"] if x[0] == 0)
    one = (0, first + 20, first + 160)
    ivs = [(0, first + 10, first + 40), (0, first + 41, first + 60), (0, first + 55, first + 120), (0, first + 10, first + 40),
           (len(L) - 1, 1, 300), (0, first, first), (0, first + 200, first + 201), (0, 1, 3)]
    extra = b"chrUn_gl0\t5\t900\n%s\t700\t700\n%s\t999999999\t1000000005\n" % (names[0], names[0])
    a = L[0] // 3
    tiles = [(0, a + 1, a + 4095), (0, a + 4096 + 11, a + 4096 + 30), (0, a + 2 * 4096 + 1, a + 3 * 4096 + 7)]
    return [("whole", [], None, b"", None), ("one region", tm.region_strings([one], names), None, b"", [one]),
            ("bed set", [], ivs, extra, ivs), ("tiles", tm.region_strings(tiles[:1], names), tiles[1:], b"", tiles)]


def test_small_datasets_python_and_cli(enc, mixed, ramp, tmp_path):
    for tag, d in (("mixed", mixed), ("ramp", ramp)):
        plan, names, lens = d["plan"], d["names"], d["lens"]
        enc.upload_reference(plan.ref)
        (tmp_path / "in.cbc").write_bytes(d["blob"]); (tmp_path / "ref.fa").write_bytes(d["fa"])
        files = (tmp_path / "in.cbc", tmp_path / "out.txt", tmp_path / "ref.fa")
        top = int(max(d["depth"].contig(c).max() for c in range(len(lens))))
        for name, regs, ivs, extra, given in _forms(d):
            if tag == "ramp" and name == "tiles":
                continue                                      # the ramp's reads sit at the contig's end
            bed = None if ivs is None else tm.bed(ivs, names) + extra
            ts = None if given is None else plan.targets(regs, bed)
            args = [x for r in regs for x in ("--region", r.decode())]
            if bed is not None:
                (tmp_path / "q.bed").write_bytes(bed)
                args += ["--regions-file", tmp_path / "q.bed"]
            want = _check(enc, d, ts, given)
            r = _cli("-x", *files, "--depth-hist", *args, "--verbose")
            assert r.returncode == 0, r.stderr
            assert (tmp_path / "out.txt").read_bytes() == hm.text(want, names), (tag, name)
            assert "kernels: decode" in r.stdout and "%d contigs" % len(want) in r.stdout
            for md, ex in ((1, 0), (top, 0), (top + 1, 16), (3, 16)):
                want = _check(enc, d, ts, given, ex, md, cm.Depth(d["iv"], lens, ex))
                if (md, name) in ((3, "bed set"), (1, "whole")):              # the options through the CLI: once folded, once both
                    r = _cli("-x", *files, "--depth-hist", *args, "--hist-max", md, "--depth-exclude-flags", ex)
                    assert r.returncode == 0 and (tmp_path / "out.txt").read_bytes() == hm.text(want, names), (tag, name, md, ex, r.stderr)
        ms = enc.last_hist_ms()
        assert len(ms) == 5 and all(x >= 0 for x in ms) and ms[0] > 0
    # a selection without a contig: nothing runs, nothing is listed
    assert enc.decode_depth_hist(ramp["plan"], ramp["plan"].targets((), b"chrUn\t1\t9\nrampA\t5\t5\n")) == []


def test_identities_against_the_existing_coverage_summary(enc, mixed, ramp):
    """On the whole-contig selection, without folding: sum of depth * bases = the `sum` of decode_coverage for the contig's
    query, and the bases at depth >= D = its `covered` for min_depth D -- the existing path, not the code under test."""
    for d in (mixed, ramp):
        plan = d["plan"]
        enc.upload_reference(plan.ref)
        rows = hm.as_rows(enc.decode_depth_hist(plan))
        qs = plan.queries()
        for D in (1, 2, 5):
            contig, _, _, total, covered = enc.decode_coverage(plan, qs, 0, D)
            assert contig.tolist() == [r[0] for r in rows]
            for (c, bins, size), t, k in zip(rows, total.tolist(), covered.tolist()):
                assert sum(dep * n for dep, n in bins) == t and sum(n for dep, n in bins if dep >= D) == k
        assert sum(total.tolist()) > 0


def test_pile_up_deeper_than_the_lds_table(enc, built):
    """About 1500 copies of one read position plus a ramp on a short contig, and 1000 copies of another under a second ramp:
    depths far above CBC_HIST_LDS and 1023, 1024, 1025 themselves, so that the accumulate pass takes its direct-global path on
    hardware next to the LDS one, with and without a fold at and next to the threshold."""
    rng = np.random.default_rng(77)
    c1 = synth.make_contig(rng, 4000)
    L = 100
    rd = lambda p, f: dict(pos=p, flag=f, cigar="%dM" % L, seq=c1[p - 1:p - 1 + L].tobytes(), md=str(L), nm=0)
    reads = [rd(200 + i, 0) for i in range(300)] + [rd(1500, 16 * (i & 1)) for i in range(1500)] + [rd(1500 + i, 0) for i in range(1, 700)]
    reads += [rd(2500, 0) for i in range(1000)] + [rd(2500 + i, 0) for i in range(1, 150)]      # a second pile: depths 1000 .. 1099
    reads.sort(key=lambda r: r["pos"])
    fa, sam = synth.fasta_text([("pile", c1)]), synth.sam_text([("pile", len(c1), reads)])
    pb = host.pack_sam(sam, fa, block_reads=256, var_length=True)
    d = _wrap(fa, pb, [b"pile"], [len(c1)], dm.assert_models_agree(pb, sam))
    top = int(d["depth"].contig(0).max())
    assert top > 1024 + 400 and all(int((d["depth"].contig(0) == k).sum()) > 0 for k in (1023, 1024, 1025))
    enc.upload_reference(d["plan"].ref)
    for md in (0, 1023, 1024, 1025, top, 40):
        want = _check(enc, d, None, None, 0, md)
        assert max(k for k, _ in want[0][1]) == (min(md, top) if md else top)
    _check(enc, d, d["plan"].targets([b"pile:1400-1700", b"pile:300-310"]), [(0, 1400, 1700), (0, 300, 310)], 16, 0, cm.Depth(d["iv"], d["lens"], 16))
    d["plan"].close(); pb.close()


def test_mid_size_panel(enc, built):
    """The 100 000-read dataset of test_targets_gpu.test_mid_size_panel with a 2000-line BED (the lines overlap in part), and
    the whole contig; the spans are the packer-derived ones."""
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
    assert len(tm.merge(ivs)) < len(ivs)
    blk = np.repeat(np.arange(pb.n_blocks), pb.blocks["n_reads"].astype(np.int64))
    pos = pb.info["window_start"][blk].astype(np.int64) + pb.recs["pos"].astype(np.int64)
    iv = list(zip([0] * pb.n_recs, pos.tolist(), _spans(pb).astype(np.int64).tolist(), pb.recs["flag"].astype(np.int64).tolist(), blk.tolist()))
    d = dict(plan=plan, names=[b"chr1"], lens=[clen], depth=cm.Depth(iv, [clen]))
    want = _check(enc, d, plan.targets((), tm.bed(ivs, d["names"])), ivs)
    assert len(want[0][1]) > 5
    _check(enc, d, None, None, 0, 6)
    print("histogram kernel ms (decode, mark, scan + compact, zero + accumulate, bin compaction):", enc.last_hist_ms())
    plan.close(); pb.close()


def test_failed_block_gives_no_bins(enc, mixed):
    """A payload byte of block 1 flipped: the block fails to decode (an error status, no fault), the call reports CBC_E_BLOCK
    and returns no bins."""
    d = mixed
    blob = bytearray(d["blob"])
    base = len(blob) - d["plan"].payloads.size
    blob[base + int(d["plan"].blocks[1]["in_off"]) + int(d["plan"].blocks[1]["in_bytes"]) // 2] ^= 0x55
    plan = host.UnpackPlan(bytes(blob), d["fa"])
    enc.upload_reference(plan.ref)
    ts = plan.targets([b"chr1"])
    assert ts.blocks[1] == 1
    got, res = enc.decode_depth_hist(plan, ts, results=True)
    assert [b for b in range(len(res)) if res[b]["status"] != 0] == [1]
    assert hm.as_rows(got) == [(0, [(0, d["lens"][0])], d["lens"][0])]
    with pytest.raises(gpu.CbcGpuError, match=r"block 1\b"):
        enc.decode_depth_hist(plan, ts)
    enc.upload_reference(d["plan"].ref)
    _check(enc, d, d["plan"].targets([b"chr1"]), [(0, 1, d["lens"][0])])
    plan.close()


def test_cli_refusals(built, mixed, tmp_path):
    d = mixed
    (tmp_path / "in.cbc").write_bytes(d["blob"]); (tmp_path / "ref.fa").write_bytes(d["fa"])
    (tmp_path / "bad.bed").write_bytes(b"chr1\t10\t20\n\nchr1\t30\n")
    files = (tmp_path / "in.cbc", tmp_path / "o.txt", tmp_path / "ref.fa")
    for args, msg in [(("--depth-hist", "--sam"), "different outputs"), (("--depth-hist", "--depth"), "different outputs"),
                      (("--depth-hist", "--bedcov"), "different outputs"), (("--depth-hist", "--devices", "0,1"), "one device"),
                      (("--hist-max", "9", "--depth"), "--hist-max applies to --depth-hist"), (("--depth-hist", "--hist-max", "0"), "--hist-max wants"),
                      (("--depth-hist", "--window", "5"), "--window applies to --bedcov"), (("--depth-hist", "--region", "chr1:9-5"), "ends before"),
                      (("--depth-hist", "--regions-file", tmp_path / "bad.bed"), "BED line 3: fewer than three columns")]:
        r = _cli("-x", *files, *args)
        assert r.returncode == 1 and msg in r.stderr, (args, r.stderr)
    r = _cli("-c", tmp_path / "in.sam", tmp_path / "o.cbc", tmp_path / "ref.fa", "--depth-hist")
    assert r.returncode == 1 and "--depth-hist applies to decompression" in r.stderr, r.stderr
    fa, sam, _, _ = synth.dataset(4, [5000], [100], 100)
    (tmp_path / "c.cbc").write_bytes(oracle.encode(sam, fa)); (tmp_path / "c.fa").write_bytes(fa)
    r = _cli("-x", tmp_path / "c.cbc", tmp_path / "o.txt", tmp_path / "c.fa", "--depth-hist")
    assert r.returncode == 1 and "single-stream (--compat) file" in r.stderr, r.stderr
    pb, _, lfa = host.synth_long(5, 200_000, 40, read_len=2000, want_text=True)
    flat, offs, _ = oracle.cpu_encode_blocks(pb, long_reads=True, return_flat=True)
    (tmp_path / "l.cbc").write_bytes(pb.container(flat, offs)); (tmp_path / "l.fa").write_bytes(lfa)
    r = _cli("-x", tmp_path / "l.cbc", tmp_path / "o.txt", tmp_path / "l.fa", "--depth-hist")
    assert r.returncode == 1 and "long-read" in r.stderr, r.stderr
    pb.close()
