"""Per-query depth quantiles on the MI355X: Encoder.decode_coverage_quant and
`cbc -x --bedcov --quantiles ..` against the brute-force model (quantmodel.py) on the small datasets of
tests/test_coverage_gpu.py, a cross-check against the depth histogram (a device path that shares none of the new code), a
pile-up deeper than the selection's LDS table, the mid-size panel unmerged and in windows, a failed block, the refusals and the
kernel-time getter.  Every comparison is exact."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import covmodel as cm
import covxmodel as cx
import depthmodel as dm
import quantmodel as qm
import regionmodel as rm
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
PCT = (0, 25, 50, 75, 100)
P8 = (0, 1, 25, 50, 75, 90, 99, 100)


@pytest.fixture(scope="module")
def enc():
    e = gpu.Encoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def mixed(built):
    fa, pb, contigs = _dataset(7 + 64, 64)
    d = _wrap(fa, pb, NAMES, [len(c) for _, c in contigs], dm.intervals_a(pb), 64)
    d["recs"] = rm.records(pb)
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


def _opts(thr, pct, rd):
    return (("--thresholds", ",".join(map(str, thr))) if thr else ()) + ("--quantiles", ",".join(map(str, pct))) + (("--count-reads",) if rd else ())


def _check(enc, d, qs, want, exclude=0, min_depth=1, pct=PCT, thr=THR, depth=None, reads=None):
    """The quantile call alone and together with thresholds and read counts: the new column against the model, every other
    column against the existing calls (and those against the model).  Returns the model's columns sum, covered, thr, quant, reads."""
    cm.check_queryset(qs, want, d["names"])
    plan = d["plan"]
    plain = enc.decode_coverage(plan, qs, exclude, min_depth)
    ext = enc.decode_coverage(plan, qs, exclude, min_depth, thresholds=thr, count_reads=True)
    alone = enc.decode_coverage_quant(plan, qs, pct, exclude, min_depth)
    both = enc.decode_coverage_quant(plan, qs, pct, exclude, min_depth, thresholds=thr, count_reads=True)
    assert len(alone) == 6 and len(both) == 8 and len(ext) == 7
    dep = depth or d["depth"]
    wq = qm.quant_expected(dep, want, pct)
    for q in (alone[5], both[6]):
        assert q.dtype == np.uint32 and q.shape == (len(want), len(pct))
        assert q.tolist() == wq, [(x, a, b) for x, a, b in zip(want, q.tolist(), wq) if a != b][:5]
    for k in (3, 4):
        assert (plain[k] == alone[k]).all() and (plain[k] == both[k]).all() and (plain[k] == ext[k]).all()
    assert (both[5] == ext[5]).all() and (both[7] == ext[6]).all()      # thr in front of quant, reads behind it
    ws, wc = cm.expected(dep, want, min_depth)
    assert [int(x) for x in plain[3]] == ws and [int(x) for x in plain[4]] == wc
    wt, wr = cx.thr_expected(dep, want, thr), cx.reads_expected(reads or d["reads"], want)
    assert ext[5].tolist() == wt and ext[6].tolist() == wr
    return ws, wc, wt, wq, wr


def test_small_datasets_python_and_cli(enc, mixed, ramp, tmp_path):
    for tag, d in (("mixed", mixed), ("ramp", ramp)):
        plan, names, lens = d["plan"], d["names"], d["lens"]
        enc.upload_reference(plan.ref)
        (tmp_path / "in.cbc").write_bytes(d["blob"]); (tmp_path / "ref.fa").write_bytes(d["fa"])
        files = (tmp_path / "in.cbc", tmp_path / "out.txt", tmp_path / "ref.fa")

        def cli_is(args, chroms, qs_in, cols, thr=THR, pct=PCT, rd=True, verbose=False):
            r = _cli("-x", *files, "--bedcov", *args, *_opts(thr, pct, rd), *(("--verbose",) if verbose else ()))
            assert r.returncode == 0, r.stderr
            ws, wc, wt, wq, wr = cols
            assert (tmp_path / "out.txt").read_bytes() == qm.text(chroms, qs_in, ws, wc, wt if thr else None, wq, wr if rd else None), (tag, args)
            return r
        if tag == "mixed":
            sets = {k: cm.of_intervals(v) for k, v in _sets(d).items() if k != "dense"}
            sets["special"] += [(-1, 5, 50), (2, 700, 700), (0, 10 ** 9, 10 ** 9 + 5)]
        else:
            sets = dict(ramp=[(0, 99_900, 100_300), (1, 0, 200), (0, 99_990, 100_010), (1, 3990, 4100), (0, 99_900, 100_300)])
        for name, given in sets.items():                     # a BED file; then the same in windows with the other options
            qs_in = [cm.clamp(*q, lens) if q[0] >= 0 else q for q in given]
            bed = cm.bed(given, names)
            (tmp_path / "q.bed").write_bytes(bed)
            cols = _check(enc, d, plan.queries((), bed), qs_in)
            chroms = [names[c] if c >= 0 else b"chrUn_gl0" for c, _, _ in qs_in]
            if name != "random200":                          # the Python call has checked that set; the CLI takes the others
                r = cli_is(("--regions-file", tmp_path / "q.bed"), chroms, qs_in, cols, verbose=True)
                assert "kernels: decode" in r.stdout and "kernels: start points" in r.stdout and "kernels: quantile selection" in r.stdout
            if name in ("one", "ramp"):                      # the new columns alone
                cli_is(("--regions-file", tmp_path / "q.bed"), chroms, qs_in, cols, thr=(), rd=False)
            cutq = cm.cut(qs_in, 37)
            if len(cutq) <= 40_000 and name in ("special", "ramp"):
                cols = _check(enc, d, plan.queries((), bed, 37), cutq, 16, 2, (25, 50, 75), (2, 3), cm.Depth(d["iv"], lens, 16), cx.Reads(d["iv"], 16))
                cli_is(("--regions-file", tmp_path / "q.bed", "--window", 37, "--min-depth", 2, "--depth-exclude-flags", 16),
                       [names[c] if c >= 0 else b"chrUn_gl0" for c, _, _ in cutq], cutq, cols, thr=(2, 3), pct=(25, 50, 75))
        # --region, repeated, unmerged and in command-line order
        regs = [(0, 99_990, 100_020), (1, 0, 150), (0, 99_950, 100_100)] if tag == "ramp" else [(2, 2999, 3300), (0, 100, 5000), (2, 2999, 3300), (1, 0, lens[1])]
        strs = [b"%s:%d-%d" % (names[c], s + 1, e) for c, s, e in regs]
        cols = _check(enc, d, plan.queries(strs), regs, pct=P8)
        cli_is([x for s in strs for x in ("--region", s.decode())], [names[c] for c, _, _ in regs], regs, cols, pct=P8)
        # no regions: one query per contig (thousands of runs each: the table form); each option adds only its own columns
        whole = [(c, 0, n) for c, n in enumerate(lens)]
        cols = _check(enc, d, plan.queries(), whole)
        for thr, rd in (((), False), (THR, True)):
            cli_is((), names, whole, cols, thr=thr, rd=rd)
        assert [r[-1] for r in cols[3]] == [int(d["depth"].contig(c).max()) for c in range(len(lens))]
        ms = enc.last_coverage_quant_ms()
        assert len(ms) == 13 and all(math.isfinite(x) and x >= 0 for x in ms) and ms[0] > 0
    empty = ramp["plan"].queries((), b"chrUn\t1\t9\nrampA\t5\t5\n")
    out = enc.decode_coverage_quant(ramp["plan"], empty, PCT, thresholds=THR, count_reads=True)
    assert out[5].tolist() == [[0, 0, 0]] * 2 and out[6].tolist() == [[0] * 5] * 2 and out[7].tolist() == [0, 0]


def test_cross_check_against_the_depth_histogram(enc, mixed):
    """Single-interval targets: the quantiles derived on the host from the bins of decode_depth_hist over that target equal the new
    column; p = 100 is the histogram's highest depth and p = 0 is 0 exactly when its depth-0 bin is not empty."""
    d, plan, lens = mixed, mixed["plan"], mixed["lens"]
    enc.upload_reference(plan.ref)
    pct = tuple(range(0, 101, 15)) + (100,)                  # 0 15 30 45 60 75 90 100
    targets = [(0, 1, lens[0]), (1, 12_000, 12_400), (0, 500, 4100), (2, 3000, 3300), (0, 30_000, 30_001), (1, 1, 7000), (0, 30_010, 30_060)]
    strs = tm.region_strings(targets, NAMES)
    out = enc.decode_coverage_quant(plan, plan.queries(strs), pct)
    zero_min = 0
    for i, s in enumerate(strs):
        (c, depth, bases, size), = enc.decode_depth_hist(plan, plan.targets([s]))
        assert c == targets[i][0] and size == targets[i][2] - targets[i][1] + 1
        assert out[5][i].tolist() == qm.hist_quantiles(depth, bases, size, pct), s
        assert int(out[5][i, -1]) == (int(depth[-1]) if len(depth) else 0)
        assert int(bases.sum()) == size                      # the binding lists the depth-0 bin among the others
        assert (int(out[5][i, 0]) == 0) == (len(depth) > 0 and int(depth[0]) == 0)
        zero_min += int(out[5][i, 0]) == 0
    assert 0 < zero_min < len(strs) and int(out[5][0, -1]) > 5


def _pile():
    """1500 copies of one 100-base read at 4000 and one more read across them from 4050: depths 1500 and 1501.  In front of
    them 70 reads of 10 bases, 12 apart: 140 runs of depth 1 and 0."""
    rng = np.random.default_rng(5)
    c = synth.make_contig(rng, 12_000)

    def read(pos, n, flag=0):
        return dict(pos=pos, flag=flag, cigar="%dM" % n, seq=c[pos - 1:pos - 1 + n].tobytes(), md="%d" % n, nm=0)
    recs = [read(3000 + 12 * i, 10) for i in range(70)] + [read(4000, 100)] * 1500 + [read(4050, 100, 16)]
    fa, sam = synth.fasta_text([("pile", c)]), synth.sam_text([("pile", len(c), recs)])
    pb = host.pack_sam(sam, fa, block_reads=64, var_length=True)
    d = _wrap(fa, pb, [b"pile"], [len(c)], dm.assert_models_agree(pb, sam), 64)
    d["reads"] = cx.Reads(d["iv"])
    return d


PILE_Q = [(0, 3999, 4099),                                   # on the pile: 50 positions of 1500, 50 of 1501 (register form)
          (0, 2990, 4200), (0, 2999, 4149), (0, 0, 12_000),  # across it with the 140 runs in front: the table form, ranks in the tail
          (0, 2990, 3850), (0, 2999, 3839), (0, 3005, 3800), # beside it: more than 64 runs of depth 1 and 0
          (0, 4049, 4050), (0, 4098, 4100), (0, 4099, 4160), (0, 4150, 4300), (0, 3990, 4010)]
PILE_P = (0, 50, 51, 92, 95, 96, 99, 100)


def test_pile_up_deeper_than_the_table(enc, built):
    """Depth 1501 lies past the selection's LDS table of 1024 bins, so the tail counter and its bisection run on the device."""
    d = _pile()
    enc.upload_reference(d["plan"].ref)
    cols = _check(enc, d, d["plan"].queries((), cm.bed(PILE_Q, d["names"])), PILE_Q, pct=PILE_P, thr=(1, 1500, 1501, 1502))
    assert cols[3][0] == [1500, 1500, 1501, 1501, 1501, 1501, 1501, 1501]
    assert cols[3][1] == cols[3][2] == [0, 1, 1, 1500, 1500, 1501, 1501, 1501]      # the ranks on either side of the table's end and in the tail
    assert cols[3][3] == [0, 0, 0, 0, 1, 1, 1, 1501] and cols[3][4][-1] == 1
    _check(enc, d, d["plan"].queries((), cm.bed(PILE_Q[:4], d["names"]), 30), cm.cut(PILE_Q[:4], 30), pct=(50,))
    d["plan"].close(); d["pb"].close()


def test_mid_size_panel_unmerged_and_windows(enc, built):
    """The 100 000-read dataset of test_coverage_gpu with its 2000 intervals left unmerged, and the same cut into windows of 100
    (more than 15 000 queries: the register form)."""
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
    depth = cm.Depth(iv, [clen])
    given = cm.of_intervals(ivs)
    bed = cm.bed(given, [b"chr1"])
    for qs, want, ex, dep in ((plan.queries((), bed), given, 0, depth), (plan.queries((), bed, 100), cm.cut(given, 100), 16, cm.Depth(iv, [clen], 16))):
        cm.check_queryset(qs, want, [b"chr1"])
        plain = enc.decode_coverage(plan, qs, ex)
        out = enc.decode_coverage_quant(plan, qs, (25, 50, 75), ex)
        wq = qm.quant_expected(dep, want, (25, 50, 75))
        assert out[5].tolist() == wq, [(x, a, b) for x, a, b in zip(want, out[5].tolist(), wq) if a != b][:5]
        assert (out[3] == plain[3]).all() and (out[4] == plain[4]).all()
    assert len(want) > 15_000 and max(r[1] for r in wq) > 3
    print("coverage quant kernel ms (the 7 of the summary; the 5 of the extension; the selection):", enc.last_coverage_quant_ms())
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
    *_, total, covered, xthr, xq, xrd, res = enc.decode_coverage_quant(plan, qs, PCT, results=True, thresholds=THR, count_reads=True)
    assert [b for b in range(len(res)) if res[b]["status"] != 0] == [1]
    good = qm.quant_expected(d["depth"], given, PCT)
    assert total.tolist()[:2] == [0, 0] and covered.tolist()[:2] == [0, 0] and xthr.tolist()[:2] == [[0, 0, 0]] * 2 and xrd.tolist()[:2] == [0, 0]
    assert xq.tolist()[:2] == [[0] * 5] * 2
    assert xq.tolist()[2] == good[2] and good[2][-1] > 0      # the other contig's call is whole
    with pytest.raises(gpu.CbcGpuError, match=r"block 1\b"):
        enc.decode_coverage_quant(plan, qs, PCT)
    enc.upload_reference(d["plan"].ref)
    _check(enc, d, d["plan"].queries((), cm.bed(given, NAMES)), given)
    plan.close()


def test_refusals(enc, built, mixed, tmp_path):
    d, plan = mixed, mixed["plan"]
    for bad in ((), (101,), (-1,), (50, 50), (75, 25), tuple(range(9)), (2 ** 32,), (12.5,), ("x",)):
        with pytest.raises(ValueError, match="quantiles"):
            enc.decode_coverage_quant(plan, plan.queries(), bad)
    enc.upload_reference(plan.ref)
    with pytest.raises(gpu.CbcGpuError, match="min_depth >= 1"):
        enc.decode_coverage_quant(plan, plan.queries(), (50,), 0, 0)
    with pytest.raises(ValueError, match="thresholds"):
        enc.decode_coverage_quant(plan, plan.queries(), (50,), thresholds=(2, 1))
    (tmp_path / "in.cbc").write_bytes(d["blob"]); (tmp_path / "ref.fa").write_bytes(d["fa"])
    files = (tmp_path / "in.cbc", tmp_path / "o.txt", tmp_path / "ref.fa")
    want = "--quantiles wants 1 to 8 percentages in 0..100, separated by commas and strictly ascending"
    for args, msg in [(("--quantiles", "50"), "--quantiles applies to --bedcov"), (("--depth", "--quantiles", "50"), "--quantiles applies to --bedcov"),
                      (("--bedcov", "--quantiles", "101"), want), (("--bedcov", "--quantiles", "50,25"), want),
                      (("--bedcov", "--quantiles", "0,1,2,3,4,5,6,7,8"), want), (("--bedcov", "--quantiles", "1,a"), want),
                      (("--bedcov", "--quantiles", "50", "--sam"), "different outputs"), (("--bedcov", "--quantiles", "50", "--region", "chr1:9-5"), "ends before")]:
        r = _cli("-x", *files, *args)
        assert r.returncode == 1 and msg in r.stderr, (args, r.stderr)


def test_kernel_time_getter_answers_for_its_own_kind(mixed):
    """cbc_gpu_last_coverage_quant_ms answers after the quantile call and after nothing else; the summary's and the extension's
    getters do not answer after the quantile call."""
    plan = mixed["plan"]
    enc = gpu.Encoder(0)
    L = gpu.lib()

    def quant():
        a, b, c = (ctypes.c_float * 7)(), (ctypes.c_float * 5)(), (ctypes.c_float * 1)()
        return L.cbc_gpu_last_coverage_quant_ms(enc._ctx, a, b, c), list(a) + list(b) + list(c)

    def ext():
        a, b = (ctypes.c_float * 7)(), (ctypes.c_float * 5)()
        return L.cbc_gpu_last_coverage_ext_ms(enc._ctx, a, b)

    def plain():
        v = [ctypes.c_float() for _ in range(7)]
        return L.cbc_gpu_last_coverage_ms(enc._ctx, *[ctypes.byref(x) for x in v])
    try:
        assert quant()[0] == -1
        enc.upload_reference(plan.ref)
        enc.decode_coverage_quant(plan, plan.queries(), (50,))
        rc, ms = quant()
        assert rc == 0 and len(ms) == 13 and all(math.isfinite(x) and x >= 0 for x in ms) and ext() == -1 and plain() == -1
        assert len(enc.last_coverage_quant_ms()) == 13
        with pytest.raises(gpu.CbcGpuError):
            enc.last_coverage_ms()
        with pytest.raises(gpu.CbcGpuError):
            enc.last_coverage_ext_ms()
        enc.decode_coverage(plan, plan.queries(), thresholds=THR, count_reads=True)
        assert quant()[0] == -1 and ext() == 0
        with pytest.raises(gpu.CbcGpuError):
            enc.last_coverage_quant_ms()
        enc.decode_coverage(plan, plan.queries())
        assert quant()[0] == -1 and plain() == 0
        enc.decode_coverage_quant(plan, plan.queries(), (0, 100), thresholds=THR)
        assert quant()[0] == 0 and ext() == -1 and plain() == -1
        enc.decode_depth_hist(plan)
        assert quant()[0] == -1
    finally:
        enc.close()
