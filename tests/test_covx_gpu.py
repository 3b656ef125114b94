"""Per-query read counts and depth thresholds on the MI355X: Encoder.decode_coverage(thresholds=,
count_reads=) and `cbc -x --bedcov --thresholds .. --count-reads` against the brute-force model (covxmodel.py) on the small
datasets of tests/test_coverage_gpu.py, cross-checks against existing device paths that share none of the new kernels (the depth
histogram, the reads of decode_targets, the call's own count of kept reads), a pile-up on one slot, the mid-size panel unmerged
and in windows, a failed block, the refusals and the kernel-time getters.  Every comparison is exact."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import covmodel as cm
import covxmodel as cx
import depthmodel as dm
import synth
import targetsmodel as tm
from cbc_amd import gpu, host
from test_coverage_gpu import NAMES, _sets, _wrap
from test_region import _dataset
from test_targets_gpu import _spans

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cbc_amd", "csrc", "cbc")
THR = (1, 2, 5)


@pytest.fixture(scope="module")
def enc():
    e = gpu.Encoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def mixed(built):
    fa, pb, contigs = _dataset(7 + 64, 64)
    d = _wrap(fa, pb, NAMES, [len(c) for _, c in contigs], dm.intervals_a(pb), 64)
    d["recs"] = __import__("regionmodel").records(pb)
    d["reads"] = cx.Reads(d["iv"])
    yield d
    d["plan"].close(); pb.close()


@pytest.fixture(scope="module")
def ramp(built):
    fa, sam, pb, contigs = dm.ramp()
    names, lens = dm.names_lens(None, contigs)
    d = _wrap(fa, pb, names, lens, dm.assert_models_agree(pb, sam), 64)
    d["reads"] = cx.Reads(d["iv"])
    yield d
    d["plan"].close(); pb.close()


def _cli(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def _check(enc, d, qs, want, exclude=0, min_depth=1, thr=THR, depth=None, reads=None):
    """The extended call against the model, its sum and covered against the plain call's.  Returns the model's columns."""
    cm.check_queryset(qs, want, d["names"])
    plain = enc.decode_coverage(d["plan"], qs, exclude, min_depth)
    contig, s0, e0, total, covered, xthr, xrd = enc.decode_coverage(d["plan"], qs, exclude, min_depth, thresholds=thr, count_reads=True)
    assert xthr.dtype == np.uint32 and xthr.shape == (len(want), len(thr)) and xrd.dtype == np.uint32 and xrd.shape == (len(want),)
    assert len(plain) == 5 and (plain[3] == total).all() and (plain[4] == covered).all()
    dep = depth or d["depth"]
    ws, wc = cm.expected(dep, want, min_depth)
    assert [int(x) for x in total] == ws and [int(x) for x in covered] == wc
    wt, wr = cx.thr_expected(dep, want, thr), cx.reads_expected(reads or d["reads"], want)
    assert xthr.tolist() == wt and xrd.tolist() == wr
    return ws, wc, wt, wr


def test_small_datasets_python_and_cli(enc, mixed, ramp, tmp_path):
    opts = ("--thresholds", ",".join(str(t) for t in THR), "--count-reads")
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
        for name, given in sets.items():                     # a BED file; then the same in windows with the other options
            qs_in = [cm.clamp(*q, lens) if q[0] >= 0 else q for q in given]
            bed = cm.bed(given, names)
            (tmp_path / "q.bed").write_bytes(bed)
            cols = _check(enc, d, plan.queries((), bed), qs_in)
            if name != "dense":
                r = _cli("-x", *files, "--bedcov", "--regions-file", tmp_path / "q.bed", "--verbose", *opts)
                assert r.returncode == 0, r.stderr
                chroms = [names[c] if c >= 0 else b"chrUn_gl0" for c, _, _ in qs_in]
                assert (tmp_path / "out.txt").read_bytes() == cx.text(chroms, qs_in, *cols), (tag, name)
                assert "kernels: decode" in r.stdout and "kernels: start points" in r.stdout
            cutq = cm.cut(qs_in, 37)
            if len(cutq) <= 40_000:
                cols = _check(enc, d, plan.queries((), bed, 37), cutq, 16, 2, (2, 3), cm.Depth(d["iv"], lens, 16), cx.Reads(d["iv"], 16))
                assert [r[0] for r in cols[2]] == cols[1]    # a threshold equal to --min-depth: the covered column
                if name not in ("special", "ramp"):          # the CLI in this form: once per dataset
                    continue
                r = _cli("-x", *files, "--bedcov", "--regions-file", tmp_path / "q.bed", "--window", 37, "--min-depth", 2, "--depth-exclude-flags", 16,
                         "--count-reads", "--thresholds", "2,3")
                assert r.returncode == 0, r.stderr
                assert (tmp_path / "out.txt").read_bytes() == cx.text([names[c] if c >= 0 else b"chrUn_gl0" for c, _, _ in cutq], cutq, *cols)
        # --region, repeated, unmerged and in command-line order
        regs = [(0, 99_990, 100_020), (1, 0, 150), (0, 99_950, 100_100)] if tag == "ramp" else [(2, 2999, 3300), (0, 100, 5000), (2, 2999, 3300), (1, 0, lens[1])]
        strs = [b"%s:%d-%d" % (names[c], s + 1, e) for c, s, e in regs]
        cols = _check(enc, d, plan.queries(strs), regs)
        r = _cli("-x", *files, "--bedcov", *opts, *[x for s in strs for x in ("--region", s.decode())])
        assert r.returncode == 0 and (tmp_path / "out.txt").read_bytes() == cx.text([names[c] for c, _, _ in regs], regs, *cols), r.stderr
        # no regions: one query per contig; the read count of a whole contig is the call's own count of kept reads
        whole = [(c, 0, n) for c, n in enumerate(lens)]
        cols = _check(enc, d, plan.queries(), whole)
        r = _cli("-x", *files, "--bedcov", *opts)
        assert r.returncode == 0 and (tmp_path / "out.txt").read_bytes() == cx.text(names, whole, *cols), r.stderr
        m = re.search(r"coverage of (\d+) queries from (\d+) reads", r.stdout)
        assert m and int(m.group(1)) == len(whole) and int(m.group(2)) == sum(cols[3]) == len(d["iv"])
        # each option adds only its own columns
        r = _cli("-x", *files, "--bedcov", "--count-reads")
        assert r.returncode == 0 and (tmp_path / "out.txt").read_bytes() == cx.text(names, whole, cols[0], cols[1], None, cols[3])
        r = _cli("-x", *files, "--bedcov", "--thresholds", "1,2,5")
        assert r.returncode == 0 and (tmp_path / "out.txt").read_bytes() == cx.text(names, whole, cols[0], cols[1], cols[2], None)
        out = enc.decode_coverage(plan, plan.queries(), count_reads=True)
        assert len(out) == 6 and out[5].tolist() == cols[3]
        out = enc.decode_coverage(plan, plan.queries(), thresholds=[5])
        assert len(out) == 6 and out[5].tolist() == [[r[2]] for r in cols[2]]
        # --window over whole contigs
        cutq = cm.cut(whole, 1000)
        cols = _check(enc, d, plan.queries(window=1000), cutq, thr=(1, 2, 3, 4, 5, 6, 50, 100))
        r = _cli("-x", *files, "--bedcov", "--window", 1000, "--thresholds", "1,2,3,4,5,6,50,100", "--count-reads")
        assert r.returncode == 0 and (tmp_path / "out.txt").read_bytes() == cx.text([names[c] for c, _, _ in cutq], cutq, *cols), r.stderr
        ms = enc.last_coverage_ext_ms()
        assert len(ms) == 12 and all(math.isfinite(x) and x >= 0 for x in ms) and ms[0] > 0
    top = int(ramp["depth"].contig(0).max())
    enc.upload_reference(ramp["plan"].ref)
    cols = _check(enc, ramp, ramp["plan"].queries(window=500), cm.cut([(c, 0, n) for c, n in enumerate(ramp["lens"])], 500), thr=(top, top + 1, 2 ** 32 - 1))
    assert all(r[1:] == [0, 0] for r in cols[2]) and any(r[0] for r in cols[2])
    empty = ramp["plan"].queries((), b"chrUn\t1\t9\nrampA\t5\t5\n")
    out = enc.decode_coverage(ramp["plan"], empty, thresholds=THR, count_reads=True)
    assert out[5].tolist() == [[0, 0, 0]] * 2 and out[6].tolist() == [0, 0]


def test_cross_checks_against_existing_device_paths(enc, mixed):
    """Single-interval targets: the threshold columns against the bins of decode_depth_hist over that target, the read count
    against the lines decode_targets writes for that one region (exclude_flags 0, no span-0 read in the data)."""
    d, plan, lens = mixed, mixed["plan"], mixed["lens"]
    enc.upload_reference(plan.ref)
    assert all(x[2] >= 1 for x in d["iv"])
    thr = (1, 2, 3, 5, 8)
    targets = [(0, 1, lens[0]), (1, 12_000, 12_400), (0, 500, 4100), (2, 3000, 3300), (0, 30_000, 30_001), (1, 1, 7000)]
    strs = tm.region_strings(targets, NAMES)
    out = enc.decode_coverage(plan, plan.queries(strs), thresholds=thr, count_reads=True)
    for i, s in enumerate(strs):
        ts = plan.targets([s])
        (c, depth, bases, size), = enc.decode_depth_hist(plan, ts)
        assert c == targets[i][0] and size == targets[i][2] - targets[i][1] + 1
        assert out[5][i].tolist() == [int(bases[depth >= t].sum()) for t in thr], s
        text, n_reads, _, _ = enc.decode_targets(plan, ts, "reads", results=True)
        assert int(out[6][i]) == text.count(b"\n") == n_reads, s
    assert int(out[6][0]) > 1000 and int(out[5][0, 0]) > 0


def test_pile_up_on_one_start_slot(enc, built):
    """1500 copies of one read: that many atomic adds land on one word of the starts array (and two of the difference array)."""
    rng = np.random.default_rng(5)
    c = synth.make_contig(rng, 12_000)
    recs = [dict(pos=4000, flag=0, cigar="100M", seq=c[3999:4099].tobytes(), md="100", nm=0)] * 1500
    recs.append(dict(pos=4050, flag=16, cigar="100M", seq=c[4049:4149].tobytes(), md="100", nm=0))
    fa, sam = synth.fasta_text([("pile", c)]), synth.sam_text([("pile", len(c), recs)])
    pb = host.pack_sam(sam, fa, block_reads=64, var_length=True)
    d = _wrap(fa, pb, [b"pile"], [len(c)], dm.assert_models_agree(pb, sam), 64)
    d["reads"] = cx.Reads(d["iv"])
    enc.upload_reference(d["plan"].ref)
    given = [(0, 3999, 4000), (0, 4098, 4099), (0, 4099, 4100), (0, 3000, 3999), (0, 4049, 4050), (0, 0, len(c)), (0, 4100, 4200)]
    cols = _check(enc, d, d["plan"].queries((), cm.bed(given, d["names"])), given, thr=(1, 1500, 1501, 1502))
    assert cols[3] == [1500, 1501, 1, 0, 1501, 1501, 1] and cols[2][5] == [150, 100, 50, 0]
    d["plan"].close(); pb.close()


def test_mid_size_panel_unmerged_and_windows(enc, built):
    """The 100 000-read dataset of test_coverage_gpu with its 2000 intervals left unmerged, and the same cut into windows of 100."""
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
    blk = np.repeat(np.arange(pb.n_blocks), pb.blocks["n_reads"].astype(np.int64))
    pos = pb.info["window_start"][blk].astype(np.int64) + pb.recs["pos"].astype(np.int64)
    iv = list(zip([0] * pb.n_recs, pos.tolist(), _spans(pb).astype(np.int64).tolist(), pb.recs["flag"].astype(np.int64).tolist(), blk.tolist()))
    d = dict(plan=plan, names=[b"chr1"], lens=[clen], depth=cm.Depth(iv, [clen]), reads=cx.Reads(iv))
    given = cm.of_intervals(ivs)
    bed = cm.bed(given, d["names"])
    cols = _check(enc, d, plan.queries((), bed), given, thr=(1, 3, 5, 10))
    assert max(cols[3]) > 50 and plan.queries((), bed).targets.n_iv < 2000
    cutq = cm.cut(given, 100)
    assert len(cutq) > 15_000
    _check(enc, d, plan.queries((), bed, 100), cutq, 16, 3, (1, 3, 5, 10), cm.Depth(iv, [clen], 16), cx.Reads(iv, 16))
    print("coverage ext kernel ms (the 7 of the summary; start points, threshold weights, scans, prefixes, lookup):", enc.last_coverage_ext_ms())
    plan.close(); pb.close()


def test_failed_block_gives_the_error_and_zeros(enc, mixed):
    """A payload byte of block 1 flipped: the block fails to decode (an error status, no fault); the call returns CBC_E_BLOCK
    and every output is zero."""
    d = mixed
    blob = bytearray(d["blob"])
    base = len(blob) - d["plan"].payloads.size
    blob[base + int(d["plan"].blocks[1]["in_off"]) + int(d["plan"].blocks[1]["in_bytes"]) // 2] ^= 0x55
    plan = host.UnpackPlan(bytes(blob), d["fa"])
    enc.upload_reference(plan.ref)
    given = [(0, 0, d["lens"][0]), (0, 100, 4000), (1, 0, 3000)]
    qs = plan.queries((), cm.bed(given, NAMES))
    assert qs.targets.blocks[1] == 1
    *_, total, covered, xthr, xrd, res = enc.decode_coverage(plan, qs, results=True, thresholds=THR, count_reads=True)
    assert [b for b in range(len(res)) if res[b]["status"] != 0] == [1]
    good = cx.reads_expected(d["reads"], given)
    assert total.tolist()[:2] == [0, 0] and covered.tolist()[:2] == [0, 0] and xthr.tolist()[:2] == [[0, 0, 0]] * 2 and xrd.tolist()[:2] == [0, 0]
    assert int(xrd[2]) == good[2] > 0                         # the other contig's call is whole
    with pytest.raises(gpu.CbcGpuError, match=r"block 1\b"):
        enc.decode_coverage(plan, qs, thresholds=THR)
    enc.upload_reference(d["plan"].ref)
    _check(enc, d, d["plan"].queries((), cm.bed(given, NAMES)), given)
    plan.close()


def test_refusals(enc, built, mixed, tmp_path):
    d, plan = mixed, mixed["plan"]
    for bad in ((0,), (2, 2), (3, 1), (1, 2, 3, 4, 5, 6, 7, 8, 9), (2 ** 32,)):
        with pytest.raises(ValueError, match="thresholds"):
            enc.decode_coverage(plan, plan.queries(), thresholds=bad)
    enc.upload_reference(plan.ref)
    with pytest.raises(gpu.CbcGpuError, match="min_depth >= 1"):
        enc.decode_coverage(plan, plan.queries(), 0, 0, count_reads=True)
    (tmp_path / "in.cbc").write_bytes(d["blob"]); (tmp_path / "ref.fa").write_bytes(d["fa"])
    files = (tmp_path / "in.cbc", tmp_path / "o.txt", tmp_path / "ref.fa")
    for args, msg in [(("--count-reads",), "--count-reads applies to --bedcov"), (("--thresholds", "1"), "--thresholds applies to --bedcov"),
                      (("--bedcov", "--thresholds", "0"), "--thresholds wants"), (("--bedcov", "--thresholds", "2,1"), "--thresholds wants"),
                      (("--bedcov", "--thresholds", "1,2,3,4,5,6,7,8,9"), "--thresholds wants"), (("--bedcov", "--thresholds", "1,a"), "--thresholds wants"),
                      (("--bedcov", "--count-reads", "--sam"), "different outputs"), (("--bedcov", "--count-reads", "--region", "chr1:9-5"), "ends before")]:
        r = _cli("-x", *files, *args)
        assert r.returncode == 1 and msg in r.stderr, (args, r.stderr)


def test_kernel_time_getters_answer_for_their_own_kind(mixed):
    """cbc_gpu_last_coverage_ext_ms answers after the extended call and after nothing else; the summary's getter does not answer
    after the extended call, nor the reverse."""
    plan = mixed["plan"]
    enc = gpu.Encoder(0)
    L = gpu.lib()

    def ext():
        a, b = (ctypes.c_float * 7)(), (ctypes.c_float * 5)()
        return L.cbc_gpu_last_coverage_ext_ms(enc._ctx, a, b), list(a) + list(b)

    def plain():
        v = [ctypes.c_float() for _ in range(7)]
        return L.cbc_gpu_last_coverage_ms(enc._ctx, *[ctypes.byref(x) for x in v])

    def hist():
        v = [ctypes.c_float() for _ in range(5)]
        return L.cbc_gpu_last_hist_ms(enc._ctx, *[ctypes.byref(x) for x in v])
    try:
        assert ext()[0] == -1 and plain() == -1
        enc.upload_reference(plan.ref)
        enc.decode_coverage(plan, plan.queries(), thresholds=THR, count_reads=True)
        rc, ms = ext()
        assert rc == 0 and all(math.isfinite(x) and x >= 0 for x in ms) and plain() == -1 and hist() == -1
        assert len(enc.last_coverage_ext_ms()) == 12
        with pytest.raises(gpu.CbcGpuError):
            enc.last_coverage_ms()
        enc.decode_coverage(plan, plan.queries())
        assert ext()[0] == -1 and plain() == 0
        with pytest.raises(gpu.CbcGpuError):
            enc.last_coverage_ext_ms()
        enc.decode_coverage(plan, plan.queries(), count_reads=True)       # no thresholds: their passes take no time
        rc, ms = ext()
        assert rc == 0 and plain() == -1
        enc.decode_depth_hist(plan)
        assert ext()[0] == -1 and hist() == 0
        enc.decode_blocks(plan)                                           # a plain decode has no post-decode stage
        assert ext()[0] == -1 and hist() == 0
    finally:
        enc.close()
