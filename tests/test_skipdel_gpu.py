"""Deletion-aware coverage on the MI355X: skip_deletions=True of Encoder.decode_depth, decode_targets
and decode_depth_hist, decode_coverage and decode_coverage_quant inside `with enc.skip_deletions():`, and `cbc -x --depth |
--bedcov | --depth-hist --skip-deletions`, against the two models of skipdelmodel.py and the existing models fed with its depth;
identities against code that is not under test (decode_pileup, decode_depth without the option); and the guard that nothing
moves without the option.  Every comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

import covmodel as cm
import covxmodel as cx
import depthmodel as dm
import histmodel as hm
import pileupmodel as pm
import quantmodel as qm
import skipdelmodel as sm
from cbc_amd import gpu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cbc_amd", "csrc", "cbc")


@pytest.fixture(scope="module")
def enc():
    e = gpu.Encoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def sets(built):
    """Every dataset once: the two models agree on each, or this raises."""
    d = {k: getattr(sm, k)() for k in ("one_read", "apart", "cancel", "edges", "shared", "mixed")}
    yield d
    for x in d.values():
        sm.close(x)


def _cli(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def _files(d, tmp_path):
    (tmp_path / "in.cbc").write_bytes(d["blob"]); (tmp_path / "ref.fa").write_bytes(d["fa"])
    return tmp_path / "in.cbc", tmp_path / "out.txt", tmp_path / "ref.fa"


def _depth_of(text, name, length):
    d = np.zeros(length, dtype=np.int64)
    for n, s, e, v in dm.parse(text):
        if n == name:
            d[s:e] = v
    return d


def test_one_read_with_one_deletion(enc, sets, tmp_path):
    """Case 1, the test that fails without the feature: two lines where the span depth has one, through the binding and the
    binary."""
    d = sets["one_read"]
    plan = d["plan"]
    enc.upload_reference(plan.ref)
    text, runs, kept, res = enc.decode_depth(plan, "solo", skip_deletions=True, results=True)
    assert (res["status"] == 0).all() and text == b"solo\t100\t140\t1\nsolo\t143\t183\t1\n" and (runs, kept) == (2, 1)
    assert enc.decode_depth(plan, "solo") == b"solo\t100\t183\t1\n"
    files = _files(d, tmp_path)
    r = _cli("-x", *files, "--depth", "--skip-deletions", "--verbose")
    assert r.returncode == 0, r.stderr
    assert files[1].read_bytes() == b"solo\t100\t140\t1\nsolo\t143\t183\t1\nother\t199\t289\t1\n" == sm.expected(d["reads"], d["names"], d["lens"])[0]
    assert "3 runs from 2 reads" in r.stdout and "mark + unmark" in r.stdout and "deleted bases not counted, edits per read 16" in r.stdout
    r = _cli("-x", *files, "--depth")
    assert r.returncode == 0 and files[1].read_bytes() == b"solo\t100\t183\t1\nother\t199\t289\t1\n"


def _columns(enc, d, qs, want, depth, reads, thr=(1,), pct=(50,), exclude=0, **kw):
    """One decode_coverage_quant with thresholds and read counts against the existing models fed with `depth`."""
    with enc.skip_deletions(kw.get("max_edits_per_read", 16), kw.get("skip_deletions", False)):
        out = enc.decode_coverage_quant(d["plan"], qs, list(pct), exclude, thresholds=thr, count_reads=True)
    total, covered, xthr, xq, xrd = out[3:8]
    ws, wc = cm.expected(depth, want)
    wt, wq, wr = cx.thr_expected(depth, want, thr), qm.quant_expected(depth, want, list(pct)), cx.reads_expected(reads, want)
    assert [int(x) for x in total] == ws and [int(x) for x in covered] == wc
    assert xthr.tolist() == wt and xq.tolist() == wq and xrd.tolist() == wr
    return ws, wc, wt, wq, wr


def test_change_points_past_two_per_read(enc, sets, tmp_path):
    """Case 2: 8 change points per read, four times the span depth's bound: every run appears in the text, and the arenas that
    follow the change points hold the sums, thresholds, quantiles and bins of the same depth."""
    d = sets["apart"]
    plan, reads, names, lens = d["plan"], d["reads"], d["names"], d["lens"]
    enc.upload_reference(plan.ref)
    want = sm.expected(reads, names, lens)
    assert want[1] == 256
    for epr in (16, 6):
        text, runs, kept, res = enc.decode_depth(plan, skip_deletions=True, max_edits_per_read=epr, results=True)
        assert (res["status"] == 0).all() and (text, runs, kept) == want, epr
    depth, spans = sm.Depth(reads, lens), cx.Reads(sm.intervals(reads))
    whole = [(0, 0, lens[0])]
    cols = _columns(enc, d, plan.queries(), whole, depth, spans, skip_deletions=True)
    cut = cm.cut(whole, 37)
    _columns(enc, d, plan.queries((), None, 37), cut, depth, spans, thr=(1, 2), pct=(0, 50, 100), skip_deletions=True)
    hist = enc.decode_depth_hist(plan, skip_deletions=True)
    assert hm.as_rows(hist) == hm.expected(depth, lens) and hm.as_rows(hist) != hm.as_rows(enc.decode_depth_hist(plan))
    files = _files(d, tmp_path)
    r = _cli("-x", *files, "--bedcov", "--skip-deletions", "--thresholds", "1", "--quantiles", "50", "--count-reads")
    assert r.returncode == 0 and files[1].read_bytes() == qm.text(names, whole, cols[0], cols[1], cols[2], cols[3], cols[4]), r.stderr
    r = _cli("-x", *files, "--depth-hist", "--skip-deletions")
    assert r.returncode == 0 and files[1].read_bytes() == hm.text(hm.expected(depth, lens), names), r.stderr
    ts = plan.targets(["apart:1-%d" % (lens[0] // 2), "apart:%d-%d" % (lens[0] // 2 + 2, lens[0])])
    text, nrd, runs, _ = enc.decode_targets(plan, ts, "depth", skip_deletions=True, results=True)
    assert (text, runs) == sm.expected_targets(reads, names, lens, ts.intervals()) and nrd == 64


def test_cancellation(enc, sets):
    """Case 3."""
    d = sets["cancel"]
    plan, reads, names, lens = d["plan"], d["reads"], d["names"], d["lens"]
    enc.upload_reference(plan.ref)
    assert int(plan.blocks[0]["n_reads"]) == 65 and len(reads[64]["dc"]) == 5 and len(reads[4]["dc"]) == 70
    text, runs, kept, res = enc.decode_depth(plan, skip_deletions=True, max_edits_per_read=80, results=True)
    assert (res["status"] == 0).all() and (text, runs, kept) == sm.expected(reads, names, lens)
    got = _depth_of(text, names[0], lens[0])
    assert got[149:153].tolist() == [0] * 4 and got[448:453].tolist() == [2, 1, 1, 1, 2] and (got[759:829] == 0).all() and got[2328:2334].tolist() == [1, 0, 0, 0, 0, 0]


def test_edges(enc, sets, tmp_path):
    """Case 4: windows and intervals cut through deleted bases, the tile boundary, merged regions; the binary on one of each."""
    d = sets["edges"]
    plan, reads, names, lens = d["plan"], d["reads"], d["names"], d["lens"]
    enc.upload_reference(plan.ref)
    files = _files(d, tmp_path)
    for beg, end in ((1, 4095), (4095, 4099), (4092, 4200), (1, 4097), (4097, 9000), (4101, 4101), (4102, 6004), (1, lens[0])):
        got = enc.decode_depth(plan, "edgeA:%d-%d" % (beg, end), skip_deletions=True, results=True)
        assert got[:3] == sm.expected(reads, names, lens, (0, beg, end)), (beg, end)
    r = _cli("-x", *files, "--depth", "--skip-deletions", "--region", "edgeA:4095-4099")
    assert r.returncode == 0 and files[1].read_bytes() == sm.expected(reads, names, lens, (0, 4095, 4099))[0], r.stderr
    sets_ = [["edgeA:4000-4101"], ["edgeA:4000-4095", "edgeA:8000-8100"], ["edgeA:4000-4093", "edgeA:4097-4300"],
             ["edgeA:5900-5990", "edgeA:5991-6100"], ["edgeA:4090-4090", "edgeA:4101-4101", "edgeA:6000-6009", "edgeB:1-3000"]]
    for regs in sets_:
        ts = plan.targets(regs)
        for ex in (0, 16):
            text, nrd, runs, res = enc.decode_targets(plan, ts, "depth", ex, skip_deletions=True, results=True)
            assert (res["status"] == 0).all() and (text, runs) == sm.expected_targets(reads, names, lens, ts.intervals(), ex), (regs, ex)
            assert nrd == enc.decode_targets(plan, ts, "depth", ex, results=True)[1]
        # the same intervals as queries: sums and read counts per query, the histogram over them
        want = cm.of_intervals(ts.intervals())
        _columns(enc, d, plan.queries(regs), [(0 if r.startswith("edgeA") else 1, int(r.split(":")[1].split("-")[0]) - 1, int(r.split("-")[1])) for r in regs],
                 sm.Depth(reads, lens), cx.Reads(sm.intervals(reads)), thr=(1, 2), pct=(0, 50), skip_deletions=True)
        assert hm.as_rows(enc.decode_depth_hist(plan, ts, skip_deletions=True)) == hm.expected(sm.Depth(reads, lens), lens, ts.intervals()), (regs, want)
    regs = sets_[2]
    r = _cli("-x", *files, "--depth", "--skip-deletions", *[x for s in regs for x in ("--region", s)])
    assert r.returncode == 0 and files[1].read_bytes() == sm.expected_targets(reads, names, lens, plan.targets(regs).intervals())[0], r.stderr


def test_keep_rule(enc, sets, tmp_path):
    """Case 5: the exclude mask, a failed block, an arena too small."""
    d = sets["edges"]
    plan, reads, names, lens = d["plan"], d["reads"], d["names"], d["lens"]
    enc.upload_reference(plan.ref)
    assert any(r["flag"] & 16 and len(r["dc"]) for r in reads)
    assert enc.decode_depth(plan, exclude_flags=16, skip_deletions=True, results=True)[:3] == sm.expected(reads, names, lens, None, 16)
    # the block of the read with 12 deleted bases does not fit one entry per read
    with pytest.raises(gpu.CbcGpuError, match="max-edits-per-read"):
        enc.decode_depth(plan, skip_deletions=True, max_edits_per_read=1)
    text, runs, kept, res = enc.decode_depth(plan, skip_deletions=True, max_edits_per_read=1, results=True)
    bad = tuple(np.flatnonzero(res["status"] != 0).tolist())
    assert bad and (res["status"][list(bad)] == 9).all()
    assert (text, runs, kept) == sm.expected(reads, names, lens, skip_blocks=bad)
    r = _cli("-x", *_files(d, tmp_path), "--depth", "--skip-deletions", "--max-edits-per-read", "1")
    assert r.returncode == 1 and "--max-edits-per-read" in r.stderr
    with pytest.raises(ValueError):
        enc.decode_depth(plan, skip_deletions=True, max_edits_per_read=511)
    with pytest.raises(ValueError):
        enc.decode_targets(plan, plan.targets(["edgeA:1-100"]), "sam", skip_deletions=True)
    pay = plan.payloads.copy()                                 # a flipped payload byte fails its block: it contributes nothing
    hurt = 1
    plan.payloads[int(plan.blocks[hurt]["in_off"]) + int(plan.blocks[hurt]["in_bytes"]) // 2] ^= 0x55
    try:
        text, runs, kept, res = enc.decode_depth(plan, skip_deletions=True, results=True)
        assert int(res[hurt]["status"]) != 0 and (np.delete(res["status"], hurt) == 0).all()
        assert (text, runs, kept) == sm.expected(reads, names, lens, skip_blocks=(hurt,))
        with pytest.raises(gpu.CbcGpuError, match=r"block %d\b" % hurt):
            enc.decode_depth(plan, "edgeA", skip_deletions=True)
    finally:
        plan.payloads[:] = pay
    assert enc.decode_depth(plan) == dm.expected(sm.intervals(reads), names, lens)[0]          # the setting did not stay behind


@pytest.mark.parametrize("kind", ["shared", "mixed"])
def test_identities(enc, sets, kind, tmp_path):
    """Case 6, against code that is not under test: where decode_pileup(min_alt=1) reports a position the new depth is its
    depth - del, everywhere else it is the span depth of decode_depth; n_reads_kept does not move; --bedcov --count-reads keeps
    its reads column and loses exactly the model's deleted bases in its sums.  (The shared-variant dataset holds no deletion --
    synth.py ignores indel_sites --, so there everything is equal; the mixed one has them.)"""
    d = sets[kind]
    plan, reads, names, lens = d["plan"], d["reads"], d["names"], d["lens"]
    enc.upload_reference(plan.ref)
    new, runs, kept, res = enc.decode_depth(plan, skip_deletions=True, results=True)
    span, _, kept0, _ = enc.decode_depth(plan, results=True)
    assert (res["status"] == 0).all() and kept == kept0 == len(reads) and (new, runs, kept) == sm.expected(reads, names, lens)
    rows = pm.parse(enc.decode_pileup(plan))
    dels = sum(r[9] for r in rows)
    assert dels > 100 if kind == "mixed" else dels == 0
    for c in range(len(names)):
        nd, sd = _depth_of(new, names[c], lens[c]), _depth_of(span, names[c], lens[c])
        seen = np.zeros(lens[c], dtype=bool)
        for r in rows:
            if r[0] == names[c]:
                assert nd[r[1] - 1] == r[3] - r[9], r
                seen[r[1] - 1] = True
        assert np.array_equal(nd[~seen], sd[~seen])
    rng = np.random.default_rng(4)
    qs_in = []
    for _ in range(40):
        c = int(rng.integers(0, len(lens)))
        s = int(rng.integers(0, lens[c] - 1))
        qs_in.append((c, s, min(lens[c], s + int(rng.choice([1, 30, 400, 5000])))))
    bed = cm.bed(qs_in, names)
    qs = plan.queries((), bed)
    a = enc.decode_coverage(plan, qs, count_reads=True)
    with enc.skip_deletions():
        b = enc.decode_coverage(plan, qs, count_reads=True)
    assert (a[5] == b[5]).all() and b[5].tolist() == cx.reads_expected(cx.Reads(sm.intervals(reads)), qs_in)
    off = [sum(int(((p >= s + 1) & (p <= e)).sum()) for r in reads if r["contig"] == c for p in [sm.deleted(r)]) for c, s, e in qs_in]
    assert [int(x) - int(y) for x, y in zip(a[3], b[3])] == off and (sum(off) > 0) == (kind == "mixed")
    (tmp_path / "q.bed").write_bytes(bed)
    files = _files(d, tmp_path)
    r = _cli("-x", *files, "--bedcov", "--count-reads", "--skip-deletions", "--regions-file", tmp_path / "q.bed")
    assert r.returncode == 0, r.stderr
    assert files[1].read_bytes() == cx.text([names[c] for c, _, _ in qs_in], qs_in, [int(x) for x in b[3]], [int(x) for x in b[4]], None, b[5].tolist())


def test_nothing_moves_without_the_option(enc, sets, tmp_path):
    """Case 7, the guard against drift (passes before and after the change): decode_depth, one --bedcov call and --depth-hist
    without the option give the bytes of the span model."""
    d = sets["mixed"]
    plan, reads, names, lens = d["plan"], d["reads"], d["names"], d["lens"]
    enc.upload_reference(plan.ref)
    iv = sm.intervals(reads)
    for ex in (0, 16):
        assert enc.decode_depth(plan, exclude_flags=ex, results=True)[:3] == dm.expected(iv, names, lens, None, ex)
    depth = cm.Depth(iv, lens)
    whole = [(c, 0, n) for c, n in enumerate(lens)]
    out = enc.decode_coverage(plan, plan.queries(), thresholds=(1, 5), count_reads=True)
    ws, wc = cm.expected(depth, whole)
    assert [int(x) for x in out[3]] == ws and [int(x) for x in out[4]] == wc and out[5].tolist() == cx.thr_expected(depth, whole, (1, 5))
    assert out[6].tolist() == cx.reads_expected(cx.Reads(iv), whole)
    assert hm.as_rows(enc.decode_depth_hist(plan)) == hm.expected(depth, lens)
    files = _files(d, tmp_path)
    r = _cli("-x", *files, "--depth")
    assert r.returncode == 0 and files[1].read_bytes() == dm.expected(iv, names, lens)[0]
    r = _cli("-x", *files, "--bedcov", "--thresholds", "1,5", "--count-reads")
    assert r.returncode == 0 and files[1].read_bytes() == cx.text(names, whole, ws, wc, out[5].tolist(), out[6].tolist())
    r = _cli("-x", *files, "--depth-hist")
    assert r.returncode == 0 and files[1].read_bytes() == hm.text(hm.expected(depth, lens), names)


def test_setter_refusals(enc, sets):
    L = gpu.lib()
    assert L.cbc_gpu_set_depth_skip_deletions(enc._ctx, 511) == -1 and b"1..510" in L.cbc_gpu_last_error(enc._ctx)
    assert L.cbc_gpu_set_depth_skip_deletions(None, 16) == -1
    d = sets["one_read"]
    enc.upload_reference(d["plan"].ref)
    assert enc.decode_depth(d["plan"], "solo") == b"solo\t100\t183\t1\n"          # a refused setting changes nothing
    assert L.cbc_gpu_set_depth_skip_deletions(enc._ctx, 510) == 0
    try:
        assert enc.decode_depth(d["plan"], "solo") == b"solo\t100\t140\t1\nsolo\t143\t183\t1\n"
        assert pm.parse(enc.decode_pileup(d["plan"], "solo"))[0][3] == 1               # the pileup's depth column keeps its span meaning
    finally:
        assert L.cbc_gpu_set_depth_skip_deletions(enc._ctx, 0) == 0
    assert enc.decode_depth(d["plan"], "solo") == b"solo\t100\t183\t1\n"
