"""Deletion-aware coverage without a GPU: the edit-reporting decoder and the unmark bodies on the
lock-step emulation (tests/skipdel_emu) against the two models of skipdelmodel.py -- one window and a target set, the change
points at their exact bound --; the stand-alone check under ASan / UBSan; the two text bounds; and what the CLI decides without
a device."""
import os
import subprocess

import numpy as np
import pytest

import depthmodel as dm
import pileupmodel as pm
import skipdelmodel as sm
import targetsmodel as tm
from cbc_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "skipdel_emu")
EXE = os.path.join(ROOT, "cbc_amd", "csrc", "cbc")


@pytest.fixture(scope="module")
def emu(built):
    subprocess.check_call(["make", "-C", EMU_DIR, "libcbc_skipdel_emu.so"], stdout=subprocess.DEVNULL)
    return sm.emu_load(os.path.join(EMU_DIR, "libcbc_skipdel_emu.so"))


def _smax(plan):
    return max(plan.contig_blocks(c).smax for c in range(plan.n_contigs))


@pytest.fixture(scope="module", params=["one_read", "apart", "cancel", "edges", "shared", "mixed"])
def data(request, built, emu):
    d = getattr(sm, request.param)()                       # the two models agree, or this raises
    d["kind"] = request.param
    d["dec"] = sm.emu_decode_all(emu, d["plan"], _smax(d["plan"]))
    yield d
    sm.close(d)


def _depth_of(text, name, length):
    """bedGraph lines of one contig -> its per-base depth."""
    d = np.zeros(length, dtype=np.int64)
    for n, s, e, v in dm.parse(text):
        if n == name:
            d[s:e] = v
    return d


def test_emulation_matches_the_model(emu, data):
    plan, reads, names, lens, dec = data["plan"], data["reads"], data["names"], data["lens"], data["dec"]
    for ex in (0, 16):
        assert sm.emu_whole(emu, plan, dec, ex) == sm.expected(reads, names, lens, None, ex), ex
    # without the option: every byte the span model's (no unmark pass, the change points at the old bound)
    assert sm.emu_whole(emu, plan, dec, skip=False) == dm.expected(sm.intervals(reads), names, lens)
    for waves in (1, 3):
        r = sm.emu_window(emu, plan, dec, plan.contig_blocks(0), n_waves=waves)
        assert (r["rc"], r["text"], r["lines"], r["kept"]) == (0,) + sm.expected(reads, names, lens, (0, 1, lens[0])), waves
    # n_reads_kept keeps its span meaning
    assert sm.emu_whole(emu, plan, dec)[2] == sm.emu_whole(emu, plan, dec, skip=False)[2]


def test_one_read_with_one_deletion(emu, built):
    """Case 1: two lines where the span depth has one."""
    d = sm.one_read()
    plan = d["plan"]
    dec = sm.emu_decode_all(emu, plan, _smax(plan))
    sel = plan.region("solo")
    r = sm.emu_window(emu, plan, dec, sel)
    assert r["text"] == b"solo\t100\t140\t1\nsolo\t143\t183\t1\n" and (r["lines"], r["kept"]) == (2, 1)
    assert r["points"] == [(100, 1), (140, 0), (143, 1), (183, 0)]
    s = sm.emu_window(emu, plan, dec, sel, skip=False)
    assert s["text"] == b"solo\t100\t183\t1\n" and (s["lines"], s["kept"]) == (1, 1) and s["points"] == [(100, 1), (183, 0)]
    sm.close(d)


def test_change_points_past_two_per_read(emu, built):
    """Case 2: 64 reads apart with three deletion runs each: 8 change points per read, four times the span depth's bound.  Every
    run appears, also with an arena of exactly the six entries a read needs, where the proved bound is 2 * 64 * 7."""
    d = sm.apart()
    plan, reads, names, lens = d["plan"], d["reads"], d["names"], d["lens"]
    sel = plan.contig_blocks(0)
    want = sm.expected(reads, names, lens)
    assert want[1] == 64 * 4
    for per_read in (16, 6):
        dec = sm.emu_decode_all(emu, plan, sel.smax, per_read)
        r = sm.emu_window(emu, plan, dec, sel)
        assert (r["text"], r["lines"], r["kept"]) == want
        assert len(r["points"]) == 64 * 8 > 2 * 64 and r["bound"] == min(lens[0] + 1, 2 * 64 * (1 + per_read))
        assert r["points"] == sm.points_of(sm.depth_a(reads, 0, 1, lens[0])[0])
    ts = plan.targets(["apart:1-%d" % (lens[0] // 2), "apart:%d-%d" % (lens[0] // 2 + 2, lens[0])])
    text, lines, kept, calls = sm.emu_targets(emu, plan, dec, ts)
    assert (text, lines) == sm.expected_targets(reads, names, lens, ts.intervals()) and kept == 64 and len(calls[0]["points"]) == 64 * 8
    sm.close(d)


def test_cancellation(emu, built):
    """Case 3: the same positions deleted twice, deletions of two reads side by side, a run of 70, the deletion in read 64 of a
    block of 65."""
    d = sm.cancel()
    plan, reads, names, lens = d["plan"], d["reads"], d["names"], d["lens"]
    assert int(plan.blocks[0]["n_reads"]) == 65 and len(reads[64]["dc"]) == 5 and len(reads[4]["dc"]) == 70
    dec = sm.emu_decode_all(emu, plan, _smax(plan), 80)
    depth = sm.depth_a(reads, 0, 1, lens[0])[0]
    assert depth[149:153].tolist() == [0] * 4 and depth[448:453].tolist() == [2, 1, 1, 1, 2] and (depth[759:829] == 0).all()
    assert depth[2329:2334].tolist() == [0] * 5 and depth[2328] == 1
    for waves in (1, 4):
        r = sm.emu_window(emu, plan, dec, plan.contig_blocks(0), n_waves=waves)
        assert (r["text"], r["lines"], r["kept"]) == sm.expected(reads, names, lens) and r["points"] == sm.points_of(depth)
    sm.close(d)


def _slot_depths(iv, points):
    """The depth of every slot of the compressed coordinate from a call's change points."""
    slots = int((iv[:, 1].astype(np.int64) - iv[:, 0] + 2).sum())
    d = np.zeros(slots + 1, dtype=np.int64)
    for (p, v), nxt in zip(points, points[1:] + [(slots, 0)]):
        d[p:nxt[0]] = v
    return d


def test_edges(emu, built):
    """Case 4: windows that cut a deletion, the tile boundary inside one, intervals that end on a deleted base, a gap across a
    deletion, two regions that merge."""
    d = sm.edges()
    plan, reads, names, lens = d["plan"], d["reads"], d["names"], d["lens"]
    dec = sm.emu_decode_all(emu, plan, _smax(plan))
    assert sm.deleted(reads[5]).tolist() == list(range(4090, 4102))          # index 4096 of a window from 1 is position 4097
    for beg, end in ((1, 4095), (4095, 4099), (4092, 4200), (1, 4097), (4097, 9000), (4101, 4101), (4102, 6004), (6005, 6005), (1, lens[0])):
        r = sm.emu_window(emu, plan, dec, plan.region("edgeA:%d-%d" % (beg, end)))
        assert (r["rc"], r["text"], r["lines"], r["kept"]) == (0,) + sm.expected(reads, names, lens, (0, beg, end)), (beg, end)
    sets = [["edgeA:4000-4101"], ["edgeA:4000-4095", "edgeA:8000-8100"], ["edgeA:4000-4093", "edgeA:4097-4300"],
            ["edgeA:5900-5990", "edgeA:5991-6100"], ["edgeA:4090-4090", "edgeA:4101-4101", "edgeA:6000-6009", "edgeB:1-3000"],
            ["edgeA:1-12000", "edgeB:100-160", "edgeB:162-170"]]
    for regs in sets:
        ts = plan.targets(regs)
        merged = ts.intervals()
        assert merged == tm.merge([(0 if r.startswith("edgeA") else 1,) + tuple(int(x) for x in r.split(":")[1].split("-")) for r in regs])
        for ex in (0, 16):
            text, lines, kept, calls = sm.emu_targets(emu, plan, dec, ts, ex)
            assert (text, lines) == sm.expected_targets(reads, names, lens, merged, ex), (regs, ex)
            assert kept == sum(1 for r in reads if not r["flag"] & ex and any(c == r["contig"] and r["pos"] <= e and r["pos"] + r["span"] - 1 >= b for c, b, e in merged))
            for call, c in zip(calls, sorted({m[0] for m in merged})):     # the spare slot behind every interval ends at depth 0
                iv = np.array([(b, e) for cc, b, e in merged if cc == c], dtype=np.uint32)
                sd = _slot_depths(iv, call["points"])
                assert (sd[np.cumsum(iv[:, 1].astype(np.int64) - iv[:, 0] + 2) - 1] == 0).all(), regs
    assert len(plan.targets(sets[3]).intervals()) == 1
    sm.close(d)


def test_keep_rule(emu, built):
    """Case 5: a read dropped by the exclude mask takes nothing off; a failed block contributes nothing; one arena entry per
    read fails the block of a read with two deleted bases with CBC_ST_EDITS."""
    d = sm.edges()
    plan, reads, names, lens = d["plan"], d["reads"], d["names"], d["lens"]
    dec = sm.emu_decode_all(emu, plan, _smax(plan))
    assert any(r["flag"] & 16 and len(r["dc"]) for r in reads)
    sel = plan.contig_blocks(0)
    assert sel.b1 - sel.b0 >= 2
    r = sm.emu_window(emu, plan, dec, sel, 16)
    assert (r["text"], r["lines"], r["kept"]) == sm.expected(reads, names, lens, (0, 1, lens[0]), 16)
    r = sm.emu_window(emu, plan, dec, sel, fail_blocks=(1,))
    assert r["rc"] == -4 and (r["text"], r["lines"], r["kept"]) == sm.expected(reads, names, lens, (0, 1, lens[0]), skip_blocks=(sel.b0 + 1,))
    assert r["text"] != sm.expected(reads, names, lens, (0, 1, lens[0]))[0]
    ts = plan.targets(["edgeA:4000-6100"])
    text, lines, kept, _ = sm.emu_targets(emu, plan, dec, ts, fail_blocks=(0,))
    assert (text, lines) == sm.expected_targets(reads, names, lens, ts.intervals(), skip_blocks=(int(ts.blocks[0]),))
    short = sm.emu_decode_all(emu, plan, _smax(plan), 1, check=False)
    assert int(short["res"][0]["status"]) == 9                             # CBC_ST_EDITS: 12 deleted bases, 11 entries in front of them
    r = sm.emu_window(emu, plan, short, plan.region("edgeA:1-5000"))
    assert r["rc"] == -4 and (r["text"], r["lines"], r["kept"]) == sm.expected(reads, names, lens, (0, 1, 5000), skip_blocks=(0,))
    sm.close(d)


@pytest.mark.parametrize("kind", ["shared", "mixed"])
def test_identities_with_the_pileup(emu, built, kind):
    """Case 6: where `--pileup --min-alt 1` reports a position, the new depth is its depth - del; everywhere else it is the span
    depth; the kept reads are the same.  The shared-variant dataset holds no deletion (synth.py ignores its indel_sites), so there
    the two depths are equal; the mixed dataset has them."""
    d = getattr(sm, kind)()
    plan, pb, reads, names, lens = d["plan"], d["pb"], d["reads"], d["names"], d["lens"]
    dec = sm.emu_decode_all(emu, plan, _smax(plan))
    new, _, kept = sm.emu_whole(emu, plan, dec)
    span, _, kept0 = sm.emu_whole(emu, plan, dec, skip=False)
    assert kept == kept0 == len(reads)
    rows = pm.parse(pm.expected(pb, reads, names, lens)[0])
    dels = sum(r[9] for r in rows)
    assert dels == sum(len(sm.deleted(r)) for r in reads) and (dels > 100 if kind == "mixed" else dels == 0)
    for c in range(len(names)):
        nd, sd = _depth_of(new, names[c], lens[c]), _depth_of(span, names[c], lens[c])
        seen = np.zeros(lens[c], dtype=bool)
        for r in rows:
            if r[0] == names[c]:
                assert nd[r[1] - 1] == r[3] - r[9], r
                seen[r[1] - 1] = True
        assert np.array_equal(nd[~seen], sd[~seen]) and int((sd - nd).sum()) == sum(r[9] for r in rows if r[0] == names[c])
    sm.close(d)


def test_text_caps(built):
    d = sm.edges()
    plan, reads, names, lens = d["plan"], d["reads"], d["names"], d["lens"]
    for c in range(plan.n_contigs):
        sel = plan.contig_blocks(c)
        k = int(plan.blocks[sel.b0:sel.b1]["n_reads"].sum())
        cap = plan.depth_skipdel_text_cap(sel.b0, sel.b1, c, sel.beg, sel.end, sel.smax)
        assert cap == min(lens[c], k * sel.smax) * (len(names[c]) + 34)
        text, n, _ = sm.expected(reads, names, lens, (c, 1, lens[c]))
        assert n <= min(lens[c], k * sel.smax) and len(text) <= cap
    a = sm.apart()                                         # the span depth's bound, two runs per read less one, no longer holds
    text, n, _ = sm.expected(a["reads"], a["names"], a["lens"])
    sel = a["plan"].contig_blocks(0)
    assert n == 256 > 2 * 64 - 1 and len(text) <= a["plan"].depth_skipdel_text_cap(sel.b0, sel.b1, 0, 1, a["lens"][0], sel.smax)
    sm.close(a)
    assert plan.depth_skipdel_text_cap(0, plan.n_blocks + 1, 0, 1, 10, 100) == 0 and plan.depth_skipdel_text_cap(0, 1, plan.n_contigs, 1, 10, 100) == 0
    assert plan.depth_skipdel_text_cap(0, 1, 0, 0, 10, 100) == 0 and plan.depth_skipdel_text_cap(0, 1, 0, 11, 10, 100) == 0
    assert plan.depth_skipdel_text_cap(0, 1, 0, 1, 2 ** 31, 100) == 0
    line = b"%s\t%d\t%d\t%d\n" % (names[0], 2 ** 31 - 2, 2 ** 31 - 1, 2 ** 32 - 1)        # the longest line there is
    assert len(line) == len(names[0]) + 34
    ts = plan.targets(["edgeA:4000-4101", "edgeB:1-3000", "edgeA:6000-6100"])
    for c in range(2):
        k = int(plan.blocks[ts.blocks[int(ts.contig_blk_first[c]):][:int(ts.contig_blk_count[c])]]["n_reads"].sum())
        size = sum(e - b + 1 for cc, b, e in ts.intervals() if cc == c)
        assert ts.depth_skipdel_cap[c] == min(size, k * ts.smax) * (len(names[c]) + 34)
    sm.close(d)


def test_the_emulated_text_cap_one_byte_short(emu, data):
    plan, dec = data["plan"], data["dec"]
    sel = plan.contig_blocks(0)
    want = sm.expected(data["reads"], data["names"], data["lens"], (0, 1, data["lens"][0]))[0]
    r = sm.emu_window(emu, plan, dec, sel, cap=len(want) - 1)
    assert r["rc"] == -1 and r["total"] == len(want) and r["text"] == b""
    assert sm.emu_window(emu, plan, dec, sel, cap=len(want))["text"] == want


def test_sanitizer_build_of_the_stand_alone_check(built):
    """skipdel_emu_check: fabricated records and arena entries (every length, deletions in front of the first and behind the
    last base, runs of 70, hostile entries, blocks of 0 .. 65 reads, windows and intervals cut through deleted bases, the change
    points at exactly their bound) in a program of its own under AddressSanitizer / UBSan, every table at its exact size; it
    exits non-zero on a finding or a mismatch."""
    subprocess.check_call(["make", "-C", EMU_DIR, "asan_check"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(EMU_DIR, "skipdel_emu_check")], capture_output=True, text=True)
    assert r.returncode == 0 and "SKIPDEL EMU CHECK OK" in r.stdout and "MISMATCH" not in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- the CLI where no device is needed -----------------------------------------------------------------------------------------
def _cli(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def test_cli_refusals_and_empty_selection(built, tmp_path):
    d = sm.edges()
    (tmp_path / "in.cbc").write_bytes(d["blob"]); (tmp_path / "ref.fa").write_bytes(d["fa"])
    files = (tmp_path / "in.cbc", tmp_path / "o.txt", tmp_path / "ref.fa")
    where = "--skip-deletions applies to --depth, --bedcov or --depth-hist"
    for args, msg in [(("--skip-deletions",), where), (("--skip-deletions", "--sam"), where), (("--skip-deletions", "--stats"), where),
                      (("--skip-deletions", "--region", "edgeA"), where), (("--skip-deletions", "--pileup"), "the del column of --pileup already says it"),
                      (("--skip-deletions", "--max-edits-per-read", "4"), where),
                      (("--depth", "--max-edits-per-read", "4"), "--max-edits-per-read applies to --pileup"),
                      (("--depth", "--skip-deletions", "--max-edits-per-read", "511"), "1..510"),
                      (("--depth", "--skip-deletions", "--max-edits-per-read", "0"), "1..510"),
                      (("--depth", "--bedcov", "--skip-deletions"), "different outputs"),
                      (("--depth", "--skip-deletions", "--devices", "0,1"), "one device"),
                      (("--depth", "--skip-deletions", "--region", "nope"), "nope")]:
        r = _cli("-x", *files, *args)
        assert r.returncode == 1 and msg in r.stderr, (args, r.stderr)
    r = _cli("-c", tmp_path / "ref.fa", tmp_path / "o.cbc", tmp_path / "ref.fa", "--skip-deletions")
    assert r.returncode == 1 and "--skip-deletions applies to decompression" in r.stderr
    (tmp_path / "stream.cbc").write_bytes(b"\x00\x00\x00\x64" + bytes(60))                # a compat file
    r = _cli("-x", tmp_path / "stream.cbc", tmp_path / "o.txt", tmp_path / "ref.fa", "--depth", "--skip-deletions")
    assert r.returncode == 1 and "needs a block container" in r.stderr
    # windows and intervals in front of the contig's first read: no block selected, an empty file (the queries' zeros), exit 0,
    # no device opened
    first = min(r["pos"] for r in d["reads"] if r["contig"] == 0)
    assert first > 10
    r = _cli("-x", *files, "--depth", "--skip-deletions", "--region", "edgeA:1-%d" % (first - 1), "--verbose")
    assert r.returncode == 0 and (tmp_path / "o.txt").read_bytes() == b"" and "0 runs from 0 reads in 0 of" in r.stdout, r.stdout + r.stderr
    assert "kernels:" not in r.stdout
    r = _cli("-x", *files, "--depth", "--skip-deletions", "--region", "edgeA:1-5", "--region", "edgeA:7-9", "--verbose")
    assert r.returncode == 0 and (tmp_path / "o.txt").read_bytes() == b"" and "kernels:" not in r.stdout, r.stdout + r.stderr
    r = _cli("-x", *files, "--bedcov", "--skip-deletions", "--region", "edgeA:1-5", "--verbose")
    assert r.returncode == 0 and (tmp_path / "o.txt").read_bytes() == b"edgeA\t0\t5\t0\t0\t0.00\n" and "kernels:" not in r.stdout
    r = _cli("-x", *files, "--depth-hist", "--skip-deletions", "--region", "edgeA:1-5", "--verbose")
    assert r.returncode == 0 and (tmp_path / "o.txt").read_bytes().startswith(b"edgeA\t0\t5\t5\t1.000000\n") and "kernels:" not in r.stdout
    assert "--skip-deletions" in _cli().stderr                                             # the usage names it
    sm.close(d)


def test_exports_and_headers(built):
    from cbc_amd import gpu
    assert "cbc_gpu_set_depth_skip_deletions" in gpu.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "cbc_gpu.h")).read()
    assert "cbc_gpu_set_depth_skip_deletions(" in hdr and "#define CBC_ABI_VERSION 1" in hdr.replace("  ", " ")
    hosth = open(os.path.join(ROOT, "include", "cbc_host.h")).read()
    assert "cbc_unpack_depth_skipdel_text_cap(" in hosth and "cbc_unpack_targets_depth_skipdel_cap(" in hosth
    import inspect
    for fn in (gpu.Encoder.decode_depth, gpu.Encoder.decode_targets, gpu.Encoder.decode_depth_hist):
        p = inspect.signature(fn).parameters
        assert p["skip_deletions"].default is False and p["max_edits_per_read"].default == 16
    # decode_coverage and decode_coverage_quant keep their parameter lists: they are used inside `with enc.skip_deletions():`
    assert inspect.signature(gpu.Encoder.skip_deletions).parameters["max_edits_per_read"].default == 16
