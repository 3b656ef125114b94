"""Per-target coverage summary on the MI355X: Encoder.decode_coverage and `cbc -x --bedcov` against
the brute-force model (covmodel.py) on the small datasets of tests/test_targets_gpu.py, a cross-check of the sums against the
bedGraph of the existing Encoder.decode_targets(output="depth"), the mid-size panel with 2000 unmerged lines and with windows,
a failed block, and the CLI's refusals.  Every comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

import covmodel as cm
import depthmodel as dm
import regionmodel as rm
import synth
import targetsmodel as tm
from cbc_amd import gpu, host
from oracle import oracle
from test_region import _dataset, _regions
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


def _wrap(fa, pb, names, lens, iv, block_reads):
    blob = rm.container(pb)
    plan = host.UnpackPlan(blob, fa)
    return dict(fa=fa, pb=pb, blob=blob, plan=plan, names=names, lens=lens, iv=iv, depth=cm.Depth(iv, lens), block_reads=block_reads)


@pytest.fixture(scope="module")
def mixed(built):
    fa, pb, contigs = _dataset(7 + 64, 64)                    # the mixed dataset of the other GPU tests at block_reads 64
    d = _wrap(fa, pb, NAMES, [len(c) for _, c in contigs], dm.intervals_a(pb), 64)
    d["recs"] = rm.records(pb)
    yield d
    d["plan"].close(); pb.close()


@pytest.fixture(scope="module")
def ramp(built):
    fa, sam, pb, contigs = dm.ramp()
    names, lens = dm.names_lens(None, contigs)
    d = _wrap(fa, pb, names, lens, dm.assert_models_agree(pb, sam), 64)
    yield d
    d["plan"].close(); pb.close()


def _sets(d):
    special, _ = tm.special_set(d["pb"], d["recs"], d["block_reads"])
    return dict(random200=[(c, b, e) for _, c, b, e in _regions(d, 200, 21)], special=special,
                dense=tm.dense_set(0, 500, 4100, 13, 6), one=[(1, 12_000, 12_400)])


def _cli(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def _check(enc, d, qs, want, exclude=0, min_depth=1, depth=None):
    cm.check_queryset(qs, want, d["names"])
    contig, s0, e0, total, covered = enc.decode_coverage(d["plan"], qs, exclude, min_depth)
    assert total.dtype == np.uint64 and covered.dtype == np.uint32 and contig.tolist() == [q[0] for q in want]
    ws, wc = cm.expected(depth or d["depth"], want, min_depth)
    assert [int(x) for x in total] == ws and [int(x) for x in covered] == wc
    return ws, wc


def test_small_datasets_python_and_cli(enc, mixed, ramp, tmp_path):
    for tag, d in (("mixed", mixed), ("ramp", ramp)):
        plan, names, lens = d["plan"], d["names"], d["lens"]
        enc.upload_reference(plan.ref)
        (tmp_path / "in.cbc").write_bytes(d["blob"]); (tmp_path / "ref.fa").write_bytes(d["fa"])
        files = (tmp_path / "in.cbc", tmp_path / "out.txt", tmp_path / "ref.fa")
        if tag == "mixed":
            sets = {k: cm.of_intervals(v) for k, v in _sets(d).items()}
            sets["special"] += [(-1, 5, 50), (2, 700, 700), (0, 10 ** 9, 10 ** 9 + 5)]
        else:
            sets = dict(ramp=[(0, 99_900, 100_300), (1, 0, 200), (0, 99_990, 100_010), (1, 3990, 4100), (0, 99_900, 100_300)])
        for name, given in sets.items():
            qs_in = [cm.clamp(*q, lens) if q[0] >= 0 else q for q in given]
            bed = cm.bed(given, names)
            (tmp_path / "q.bed").write_bytes(bed)
            # --regions-file
            ws, wc = _check(enc, d, plan.queries((), bed), qs_in)
            r = _cli("-x", *files, "--bedcov", "--regions-file", tmp_path / "q.bed", "--verbose")
            assert r.returncode == 0, r.stderr
            chroms = [names[c] if c >= 0 else b"chrUn_gl0" for c, _, _ in qs_in]
            assert (tmp_path / "out.txt").read_bytes() == cm.text(chroms, qs_in, ws, wc), (tag, name)
            assert "kernels: decode" in r.stdout and "intervals after merging" in r.stdout and "%d queries" % len(qs_in) in r.stdout
            # --window (the last window of a query may be short), --min-depth and --depth-exclude-flags
            cutq = cm.cut(qs_in, 37)
            if len(cutq) <= 40_000:
                ws, wc = _check(enc, d, plan.queries((), bed, 37), cutq, 16, 2, cm.Depth(d["iv"], lens, 16))
                r = _cli("-x", *files, "--bedcov", "--regions-file", tmp_path / "q.bed", "--window", 37, "--min-depth", 2, "--depth-exclude-flags", 16)
                assert r.returncode == 0, r.stderr
                assert (tmp_path / "out.txt").read_bytes() == cm.text([names[c] if c >= 0 else b"chrUn_gl0" for c, _, _ in cutq], cutq, ws, wc)
        # --region, repeated, in command-line order and unmerged; then with a file behind them
        regs = [(0, 99_990, 100_020), (1, 0, 150), (0, 99_950, 100_100)] if tag == "ramp" else [(2, 2999, 3300), (0, 100, 5000), (2, 2999, 3300), (1, 0, lens[1])]
        strs = [b"%s:%d-%d" % (names[c], s + 1, e) for c, s, e in regs]
        ws, wc = _check(enc, d, plan.queries(strs), regs)
        r = _cli("-x", *files, "--bedcov", *[x for s in strs for x in ("--region", s.decode())])
        assert r.returncode == 0 and (tmp_path / "out.txt").read_bytes() == cm.text([names[c] for c, _, _ in regs], regs, ws, wc), r.stderr
        both = regs + [(0, 10, 20)]
        ws, wc = _check(enc, d, plan.queries(strs, b"%s\t10\t20\n" % names[0]), both)
        # neither: one query per contig, whole, in table order; and the same cut into windows
        whole = [(c, 0, n) for c, n in enumerate(lens)]
        ws, wc = _check(enc, d, plan.queries(), whole)
        r = _cli("-x", *files, "--bedcov")
        assert r.returncode == 0 and (tmp_path / "out.txt").read_bytes() == cm.text(names, whole, ws, wc), r.stderr
        cutq = cm.cut(whole, 1000)
        ws, wc = _check(enc, d, plan.queries(window=1000), cutq)
        r = _cli("-x", *files, "--bedcov", "--window", 1000)
        assert r.returncode == 0 and (tmp_path / "out.txt").read_bytes() == cm.text([names[c] for c, _, _ in cutq], cutq, ws, wc), r.stderr
        ms = enc.last_coverage_ms()
        assert len(ms) == 7 and all(x >= 0 for x in ms) and ms[0] > 0
    # min_depth above the maximum: nothing is covered, the sums stay
    top = int(ramp["depth"].contig(0).max())
    enc.upload_reference(ramp["plan"].ref)
    for md in (top, top + 1):
        _check(enc, ramp, ramp["plan"].queries(window=500), cm.cut([(c, 0, n) for c, n in enumerate(ramp["lens"])], 500), 0, md)
    with pytest.raises(gpu.CbcGpuError, match="min_depth >= 1"):
        enc.decode_coverage(ramp["plan"], ramp["plan"].queries(), 0, 0)
    empty = ramp["plan"].queries((), b"chrUn\t1\t9\nrampA\t5\t5\n")
    out = enc.decode_coverage(ramp["plan"], empty)
    assert out[0].tolist() == [-1, 0] and out[3].tolist() == [0, 0] and out[4].tolist() == [0, 0]


def test_sums_equal_the_existing_depth_track(enc, mixed):
    """For every merged interval of one set: sum = the depth times the length over the lines the existing depth output writes
    for it -- the existing path, not the code under test."""
    d, plan = mixed, mixed["plan"]
    enc.upload_reference(plan.ref)
    ivs = _sets(d)["random200"]
    merged = tm.merge(ivs)
    ts = plan.targets(tm.region_strings(ivs, NAMES))
    rows = dm.parse(enc.decode_targets(plan, ts, "depth"))
    qs = plan.queries(tm.region_strings(merged, NAMES))
    assert qs.targets.intervals() == merged
    _, s0, e0, total, covered = enc.decode_coverage(plan, qs)
    for (c, b, e), t, k in zip(merged, total.tolist(), covered.tolist()):
        mine = [r for r in rows if r[0] == NAMES[c] and r[1] >= b - 1 and r[2] <= e]
        assert t == sum(r[3] * (r[2] - r[1]) for r in mine) and k == sum(r[2] - r[1] for r in mine)
    assert sum(total.tolist()) == sum(r[3] * (r[2] - r[1]) for r in rows) > 0


def test_mid_size_panel_unmerged_and_windows(enc, built):
    """The 100 000-read dataset of test_targets_gpu.test_mid_size_panel with its 2000 intervals left unmerged (they overlap
    in part), and the same cut into windows of 100 bases; the spans are the packer-derived ones."""
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
    given = cm.of_intervals(ivs)
    bed = cm.bed(given, d["names"])
    ws, _ = _check(enc, d, plan.queries((), bed), given)
    assert max(ws) > 0 and plan.queries((), bed).targets.n_iv < 2000
    cutq = cm.cut(given, 100)
    assert len(cutq) > 15_000
    _check(enc, d, plan.queries((), bed, 100), cutq, 0, 3)
    print("coverage kernel ms (decode, mark, scan + compact, weights, weight scans, prefixes, lookup):", enc.last_coverage_ms())
    plan.close(); pb.close()


def test_failed_block_contributes_nothing(enc, mixed):
    """A payload byte of block 1 flipped: the block fails to decode (an error status, no fault), the call reports it, and the
    block's reads are missing from the numbers."""
    d = mixed
    blob = bytearray(d["blob"])
    base = len(blob) - d["plan"].payloads.size
    blob[base + int(d["plan"].blocks[1]["in_off"]) + int(d["plan"].blocks[1]["in_bytes"]) // 2] ^= 0x55
    plan = host.UnpackPlan(bytes(blob), d["fa"])
    enc.upload_reference(plan.ref)
    given = [(0, 0, d["lens"][0]), (0, 100, 4000), (1, 0, 3000)]
    qs = plan.queries((), cm.bed(given, NAMES))
    assert qs.targets.blocks[1] == 1
    *_, total, covered, res = enc.decode_coverage(plan, qs, results=True)
    assert [b for b in range(len(res)) if res[b]["status"] != 0] == [1]
    ws, wc = cm.expected(cm.Depth(d["iv"], d["lens"], 0, (1,)), given)
    assert [int(x) for x in total] == ws and [int(x) for x in covered] == wc and ws != cm.expected(d["depth"], given)[0]
    with pytest.raises(gpu.CbcGpuError, match=r"block 1\b"):
        enc.decode_coverage(plan, qs)
    enc.upload_reference(d["plan"].ref)
    _check(enc, d, d["plan"].queries((), cm.bed(given, NAMES)), given)
    plan.close()


def test_cli_refusals(built, mixed, tmp_path):
    d = mixed
    (tmp_path / "in.cbc").write_bytes(d["blob"]); (tmp_path / "ref.fa").write_bytes(d["fa"])
    (tmp_path / "bad.bed").write_bytes(b"chr1\t10\t20\n\nchr1\t30\n")
    files = (tmp_path / "in.cbc", tmp_path / "o.txt", tmp_path / "ref.fa")
    for args, msg in [(("--bedcov", "--sam"), "different outputs"), (("--bedcov", "--depth"), "different outputs"),
                      (("--bedcov", "--devices", "0,1"), "one device"), (("--window", "100"), "--window applies to --bedcov"),
                      (("--min-depth", "2", "--depth"), "--min-depth applies to --bedcov"), (("--bedcov", "--window", "0"), "--window wants"),
                      (("--bedcov", "--region", "chr1:9-5"), "ends before"),
                      (("--bedcov", "--regions-file", tmp_path / "bad.bed"), "BED line 3: fewer than three columns")]:
        r = _cli("-x", *files, *args)
        assert r.returncode == 1 and msg in r.stderr, (args, r.stderr)
    r = _cli("-c", tmp_path / "in.sam", tmp_path / "o.cbc", tmp_path / "ref.fa", "--bedcov")
    assert r.returncode == 1 and "--bedcov applies to decompression" in r.stderr, r.stderr
    fa, sam, _, _ = synth.dataset(4, [5000], [100], 100)
    (tmp_path / "c.cbc").write_bytes(oracle.encode(sam, fa)); (tmp_path / "c.fa").write_bytes(fa)
    r = _cli("-x", tmp_path / "c.cbc", tmp_path / "o.txt", tmp_path / "c.fa", "--bedcov")
    assert r.returncode == 1 and "single-stream (--compat) file" in r.stderr, r.stderr
    pb, _, lfa = host.synth_long(5, 200_000, 40, read_len=2000, want_text=True)
    flat, offs, _ = oracle.cpu_encode_blocks(pb, long_reads=True, return_flat=True)
    (tmp_path / "l.cbc").write_bytes(pb.container(flat, offs)); (tmp_path / "l.fa").write_bytes(lfa)
    r = _cli("-x", tmp_path / "l.cbc", tmp_path / "o.txt", tmp_path / "l.fa", "--bedcov")
    assert r.returncode == 1 and "long-read" in r.stderr, r.stderr
    pb.close()
