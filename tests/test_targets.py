"""Decode of a set of regions without a GPU: cbc_unpack_targets (region strings + BED text -> merged
intervals, block list, per-block interval ranges, text caps) against the existing models, the BED parser with every accepted
form and every error, hostile BED text on the AddressSanitizer build, the refusals, and the keep / count / write / depth bodies
of cbc_targets_body.h on the lock-step wave emulation (tests/targets_emu), also under ASan / UBSan.  Ground truth is the
existing models and the existing single-region emulations (targetsmodel.py), never the new code."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import depthmodel as dm
import regionmodel as rm
import synth
import targetsmodel as tm
from cbc_amd import host
from oracle import oracle
from test_region import _dataset, _emu_region_text, _regions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "targets_emu")
EXE = os.path.join(ROOT, "cbc_amd", "csrc", "cbc")
NAMES = [b"chr1", b"chr2", b"chr3"]


@pytest.fixture(scope="module")
def emu(built):
    subprocess.check_call(["make", "-C", EMU_DIR, "libcbc_targets_emu.so"], stdout=subprocess.DEVNULL)
    return tm.emu_load(os.path.join(EMU_DIR, "libcbc_targets_emu.so"))


@pytest.fixture(scope="module")
def depth_emu(built):
    d = os.path.join(ROOT, "tests", "depth_emu")
    subprocess.check_call(["make", "-C", d, "libcbc_depth_emu.so"], stdout=subprocess.DEVNULL)
    return dm.emu_load(os.path.join(d, "libcbc_depth_emu.so"))


@pytest.fixture(scope="module", params=[256, 1024])
def data(request, built):
    fa, pb, contigs = _dataset(7 + request.param, request.param)
    blob = rm.container(pb)
    plan = host.UnpackPlan(blob, fa)
    d = dict(fa=fa, pb=pb, contigs=contigs, blob=blob, plan=plan, recs=rm.records(pb), block_reads=request.param,
             iv=dm.intervals_a(pb), lens=[len(c) for _, c in contigs], smax=pb.max_read_len + pb.read_length - 1)
    d["flags"] = [x[3] for x in d["iv"]]
    yield d
    plan.close(); pb.close()


@pytest.fixture(scope="module")
def dec(emu, data):
    return tm.emu_decode_all(emu, data["plan"], data["smax"])


@pytest.fixture(scope="module")
def ramp(built):
    fa, sam, pb, contigs = dm.ramp()
    plan = host.UnpackPlan(rm.container(pb), fa)
    names, lens = dm.names_lens(None, contigs)
    yield dict(plan=plan, pb=pb, iv=dm.assert_models_agree(pb, sam), names=names, lens=lens)
    plan.close(); pb.close()


def _sets(d):
    """name -> list of (contig, beg, end), unmerged, as the user would give them."""
    regs = [(c, b, e) for _, c, b, e in _regions(d, 200, 21)]
    special, _ = tm.special_set(d["pb"], d["recs"], d["block_reads"])
    return dict(random200=regs, special=special,
                dense70=tm.dense_set(0, 20_000, 70, 37, 11),               # > 64 intervals on one contig
                dense4100=tm.dense_set(0, 500, 4100, 13, 6),               # > 4096: the search runs past one tile of intervals
                one=[(1, 12_000, 12_400)])


def _check_all(emu, d, dec, ivs, how, n_waves=4):
    """One set through the host function and every output of the emulation, against the models.  how: the set given as
    region strings, as a BED text, or half and half."""
    plan, merged = d["plan"], tm.merge(ivs)
    h = len(ivs) // 2
    regions, bed = {"regions": (tm.region_strings(ivs, NAMES), None), "bed": ((), tm.bed(ivs, NAMES)),
                    "both": (tm.region_strings(ivs[:h], NAMES), tm.bed(ivs[h:], NAMES))}[how]
    ts = plan.targets(regions, bed)
    assert ts.intervals() == merged and ts.smax == d["smax"] and ts.n_input == len(ivs) and ts.bed_unselected == 0
    assert ts.blocks.tolist() == tm.expected_blocks(d["pb"], merged, d["smax"])
    rc, text, kept, _ = tm.emu_text(emu, plan, dec, ts, 0, n_waves)
    want = tm.expected_reads(d["recs"], merged)
    assert rc == 0 and text == want and kept == want.count(b"\n")
    rc, text, kept, _ = tm.emu_text(emu, plan, dec, ts, 1, n_waves)
    assert rc == 0 and text == tm.expected_sam(d["recs"], d["flags"], NAMES, merged) and kept == want.count(b"\n")
    text, lines, _, _ = tm.emu_depth(emu, plan, dec, ts)
    assert (text, lines) == tm.expected_depth(d["iv"], NAMES, d["lens"], merged)
    return ts, merged


@pytest.mark.parametrize("name,how", [("random200", "both"), ("special", "regions"), ("dense70", "bed"), ("dense4100", "bed"),
                                      ("one", "regions")])
def test_sets_match_the_models(emu, data, dec, name, how):
    _check_all(emu, data, dec, _sets(data)[name], how)


def test_the_vectorised_selection_is_the_models(data):
    for name in ("random200", "special", "dense70"):
        merged = tm.merge(_sets(data)[name])
        assert tm.kept_records(data["recs"], merged, False) == tm.kept_records(data["recs"], merged, True)


def test_special_set_holds_what_it_should(emu, data, dec):
    d, plan = data, data["plan"]
    ivs, info = tm.special_set(d["pb"], d["recs"], d["block_reads"])
    merged = tm.merge(ivs)
    assert len(merged) < len(ivs) and ivs != sorted(ivs)                          # merged; given unsorted
    assert (2, 3000, 3300) in merged                                              # overlapping + adjacent + duplicate -> one
    assert info["touch"][0] not in merged and (0, info["touch"][0][1], info["touch"][1][2]) in merged
    assert not rm.selected(d["recs"], *info["gap"])                               # wholly between two reads
    ts = plan.targets(tm.region_strings(ivs, NAMES))
    assert ts.contig_count[1] == 0 and ts.contig_blk_count[1] == 0
    assert not any(int(d["pb"].info[b]["contig"]) == 1 for b in ts.blocks)        # a contig without intervals: no block of it
    # the read under two intervals: once in reads and SAM, marked in both intervals in the depth
    a, b = info["two"]
    r = info["read"]
    two = plan.targets(tm.region_strings([a, b], NAMES))
    assert two.n_iv == 2
    _, text, kept, _ = tm.emu_text(emu, plan, dec, two, 0)
    assert text.count(r[4] + b"\n") == sum(1 for x in d["recs"] if x[4] == r[4]) and kept == text.count(b"\n")
    assert text == tm.expected_reads(d["recs"], [a, b])
    text, lines, _, _ = tm.emu_depth(emu, plan, dec, two)
    rows = dm.parse(text)
    assert any(a[1] - 1 <= x[1] and x[2] <= a[2] for x in rows) and any(b[1] - 1 <= x[1] and x[2] <= b[2] for x in rows)
    assert not any(x[1] < a[2] and x[2] > a[2] for x in rows)                      # no run crosses the gap
    # 1-base intervals; runs are not cut where two input intervals were merged
    assert {(0, 5, 5), (0, 7, 7), (2, 1, 1)} <= set(merged)
    t1 = plan.targets(tm.region_strings(info["touch"], NAMES))
    text, _, _, _ = tm.emu_depth(emu, plan, dec, t1)
    assert text == tm.expected_depth(d["iv"], NAMES, d["lens"], tm.merge(info["touch"]))[0]
    # ... where the model, run on each input interval by itself, does cut a run that spans the seam of (2, 3050-3200 | 3201-3300)
    seam = plan.targets((), tm.bed([(2, 3050, 3200), (2, 3201, 3300)], NAMES))
    text, _, _, _ = tm.emu_depth(emu, plan, dec, seam)
    whole = tm.expected_depth(d["iv"], NAMES, d["lens"], [(2, 3050, 3300)])[0]
    parts = tm.expected_depth(d["iv"], NAMES, d["lens"], [(2, 3050, 3200), (2, 3201, 3300)])[0]
    assert text == whole
    if not any(x[0] == 2 and x[1] == 3201 or x[1] + x[2] == 3201 for x in d["iv"]):     # no read edge on the seam itself
        assert whole != parts and whole.count(b"\n") == parts.count(b"\n") - 1


def test_one_interval_equals_the_single_region_emulations(emu, depth_emu, data, dec):
    """One interval only: the bytes of the single-region emulations (region text, depth window)."""
    d, plan = data, data["plan"]
    for s in ("chr2:12000-12400", "chr1", "chr3:19000-20000"):
        sel = plan.region(s)
        ts = plan.targets([s])
        assert ts.n_iv == 1 and ts.blocks.tolist() == list(range(sel.b0, sel.b1)) and ts.intervals() == [(sel.contig, sel.beg, sel.end)]
        rc, text, _, _ = tm.emu_text(emu, plan, dec, ts, 0)
        assert rc == 0 and text == _emu_region_text(plan, sel)
        text, lines, kept, _ = tm.emu_depth(emu, plan, dec, ts)
        rc, want, wl, wk, _ = dm.emu_call(depth_emu, plan, sel)
        assert rc == 0 and (text, lines, kept) == (want, wl, wk)


def test_depth_equals_the_single_window_calls_appended(emu, depth_emu, data, dec):
    """The second source of the depth: the existing single-window emulation per merged interval, appended."""
    d, plan = data, data["plan"]
    ivs, _ = tm.special_set(d["pb"], d["recs"], d["block_reads"])
    merged = tm.merge(ivs)
    ts = plan.targets((), tm.bed(ivs, NAMES))
    for ex in (0, 16):
        want = b"".join(dm.emu_call(depth_emu, plan, plan.region(s), ex)[1] for s in tm.region_strings(merged, NAMES))
        text, lines, _, _ = tm.emu_depth(emu, plan, dec, ts, ex)
        assert text == want and lines == want.count(b"\n")
        assert text == tm.expected_depth(d["iv"], NAMES, d["lens"], merged, ex)[0]


def test_ramp_depth_digits_and_exclude(emu, ramp):
    plan = ramp["plan"]
    ivs = [(0, 99_960, 99_999), (0, 100_001, 100_040), (0, 100_050, 100_050), (1, 1, 50), (1, 4000, 4099), (1, 4100, 4200)]
    merged = tm.merge(ivs)
    ts = plan.targets((), tm.bed(ivs, ramp["names"]))
    dec = tm.emu_decode_all(emu, plan, ts.smax)
    for ex in (0, 1024, 16):
        text, lines, _, _ = tm.emu_depth(emu, plan, dec, ts, ex)
        assert (text, lines) == tm.expected_depth(ramp["iv"], ramp["names"], ramp["lens"], merged, ex), ex
    rows = dm.parse(tm.emu_depth(emu, plan, dec, ts)[0])
    assert {9, 10}.issubset({r[3] for r in rows}) or max(r[3] for r in rows) >= 10
    assert any(r[2] == 99_999 for r in rows) and any(r[1] == 100_000 for r in rows)


def test_empty_selection_and_failed_block(emu, data, dec):
    d, plan = data, data["plan"]
    first = min(x[1] for x in d["iv"] if x[0] == 0)
    ts = plan.targets(["chr1:1-%d" % (first - 1)], b"chrUn\t5\t9\nchr2\t0\t0\n")
    assert ts.n_blocks == 0 and ts.n_iv == 1 and ts.bed_unselected == 2
    assert tm.emu_text(emu, plan, dec, ts, 0)[:3] == (0, b"", 0) and tm.emu_depth(emu, plan, dec, ts)[0] == b""
    assert plan.targets().n_iv == 0 and plan.targets().n_blocks == 0
    # a failed block contributes nothing (the model: its records skipped)
    ivs = _sets(d)["random200"]
    merged = tm.merge(ivs)
    ts = plan.targets(tm.region_strings(ivs, NAMES))
    k = 1
    blk = int(ts.blocks[k])
    rc, text, _, _ = tm.emu_text(emu, plan, dec, ts, 0, fail_blocks=(k,))
    recs_wo = [r for r in d["recs"] if r[0] != blk]
    assert rc == 0 and text == tm.expected_reads(recs_wo, merged) and text != tm.expected_reads(d["recs"], merged)
    text, lines, _, _ = tm.emu_depth(emu, plan, dec, ts, fail_blocks=(k,))
    assert (text, lines) == tm.expected_depth(d["iv"], NAMES, d["lens"], merged, 0, (blk,))


def test_sam_failed_block_and_name_longer_than_the_limit(emu, data, dec):
    """Through the target-set members of the shared passes: a failed block contributes no SAM line; with a name of
    CBC_SAM_MAX_NAME + 1 bytes the run text counts no line and writes nothing (the helper checks every byte of the buffers)."""
    d, plan = data, data["plan"]
    ivs = _sets(d)["random200"]
    merged = tm.merge(ivs)
    ts = plan.targets(tm.region_strings(ivs, NAMES))
    blk = int(ts.blocks[1])
    rc, text, _, _ = tm.emu_text(emu, plan, dec, ts, 1, fail_blocks=(1,))
    recs_wo = [r for r in d["recs"] if r[0] != blk]
    flags_wo = [f for r, f in zip(d["recs"], d["flags"]) if r[0] != blk]
    assert rc == 0 and text == tm.expected_sam(recs_wo, flags_wo, NAMES, merged)
    assert text != tm.expected_sam(d["recs"], d["flags"], NAMES, merged)
    text, lines, kept, _ = tm.emu_depth(emu, plan, dec, ts, name=b"n" * 256)
    assert (text, lines) == (b"", 0) and kept > 0
    text, lines, kept2, _ = tm.emu_depth(emu, plan, dec, ts)
    assert lines > 0 and kept2 == kept and text
    # zero bytes: no block marks anything, so there is no run; every text tile counts 0 bytes and its write pass ends there
    assert tm.emu_depth(emu, plan, dec, ts, fail_blocks=range(ts.n_blocks))[:3] == (b"", 0, 0)


def test_text_caps(emu, data, dec):
    d, plan = data, data["plan"]
    ts = plan.targets(tm.region_strings(_sets(d)["special"], NAMES))
    nr = [int(plan.blocks[b]["n_reads"]) for b in ts.blocks]
    assert ts.text_cap_reads == sum(nr) * (plan.seq_stride + 1)
    assert ts.text_cap_sam == sum(plan.sam_text_cap(int(b), int(b) + 1) for b in ts.blocks)
    for c in range(3):
        k = sum(int(plan.blocks[b]["n_reads"]) for b in ts.blocks[int(ts.contig_blk_first[c]):][:int(ts.contig_blk_count[c])])
        n = int(ts.contig_count[c])
        assert ts.depth_cap[c] == ((2 * k + 2 * n - 1) * (4 + 34) if n and k else 0)
    want = tm.expected_reads(d["recs"], ts.intervals())
    rc, text, _, total = tm.emu_text(emu, plan, dec, ts, 0, cap=len(want))
    assert rc == 0 and text == want
    rc, text, _, total = tm.emu_text(emu, plan, dec, ts, 0, cap=len(want) - 1)            # one byte short: reported
    assert rc == -1 and total == len(want) and text == b""


# ---- the BED parser ----------------------------------------------------------------------------------------------------------
def test_bed_forms(data):
    plan, L1 = data["plan"], data["lens"][0]
    bed = (b"# a comment\n"
           b"track name=panel\n"
           b"browser position chr1:1-100\n"
           b"\n"
           b"chr1\t99\t200\tgeneA\t0\t+\n"                  # further columns ignored
           b"chr1   300    400\n"                          # runs of spaces
           b"chr2 \t 10\t20\r\n"                           # CRLF, mixed separators
           b"chr1\t500\t500\n"                             # start == end: nothing
           b"chrUn_1\t5\t10\n"                             # not in the container: nothing
           b"chr1\t%d\t%d\n"                               # starts at the contig's end: nothing
           b"chr1\t%d\t%d\n"                               # end past the contig: clamped
           b"chr3\t0\t1" % (L1, L1 + 5, L1 - 10, L1 + 10 ** 9))   # no trailing newline
    ts = plan.targets((), bed)
    assert ts.intervals() == [(0, 100, 200), (0, 301, 400), (0, L1 - 9, L1), (1, 11, 20), (2, 1, 1)]
    assert ts.bed_unselected == 3 and ts.n_input == 5
    assert plan.targets(["chr1:150-310"], bed).intervals()[0] == (0, 100, 400)      # a region string bridges two BED lines
    assert plan.targets((), b"").n_iv == 0 and plan.targets((), b"\n\n#x").n_iv == 0


def test_bed_errors_name_the_line(data):
    plan = data["plan"]
    ok = b"chr1\t1\t5\n#c\n"
    for bad, what in [(b"chr1\t9\t5\n", "start is past end"), (b"chr1\t1\n", "fewer than three columns"), (b"chr1\n", "fewer than three"),
                      (b"chr1\tx\t5\n", "malformed or overflowing"), (b"chr1\t1\t5x\n", "malformed or overflowing"),
                      (b"chr1\t-1\t5\n", "malformed or overflowing"), (b"chr1\t1\t9999999999999999999\n", "malformed or overflowing"),
                      (b"chrUn\t9\t5\n", "start is past end"), (b"chr1\t1\t" + b"7" * 70_000 + b"\n", "longer than 65536"),
                      (b"chr1\t1\t5\0\n", "malformed or overflowing")]:
        with pytest.raises(host.CbcInputError, match="BED line 3: " + what):
            plan.targets((), ok + bad + b"chr1\t1\t2\n")
    for bad, what in [("chrX:1-5", "unknown contig"), ("chr1:9-5", "ends before"), ("chr1:0-5", "before base 1")]:
        with pytest.raises(host.CbcInputError, match=what):
            plan.targets(["chr1:1-5", bad], ok)


def test_bed_name_containing_a_colon(built):
    rng = np.random.default_rng(3)
    names = ["HLA-A*01:01:01:01", "HLA-A*01:01:01:01:1-5", "plain"]
    contigs = [(n, synth.make_contig(rng, 3000)) for n in names]
    rbc = [(n, 3000, synth.make_reads(rng, c, 50, 100)) for n, c in contigs]
    pb = rm.pack(synth.fasta_text(contigs), rbc, 256)
    plan = host.UnpackPlan(rm.container(pb), synth.fasta_text(contigs))
    ts = plan.targets(["HLA-A*01:01:01:01:20-30", "HLA-A*01:01:01:01:1-5"], b"HLA-A*01:01:01:01\t99\t200\nHLA-A*01:01:01:01:1-5\t0\t7\n")
    assert ts.intervals() == [(0, 20, 30), (0, 100, 200), (1, 1, 3000)]
    plan.close(); pb.close()


def test_too_many_intervals_are_refused(data):
    n = (1 << 24) + 1
    pos = np.arange(n, dtype=np.int64) * 2
    bed = b"".join(b"chr1\t%d\t%d\n" % (p, p + 1) for p in pos[:50]) * 0 + b"\n".join(
        np.char.add(np.char.add(np.char.add("chr1\t", pos.astype(str)), "\t"), (pos + 1).astype(str)).astype("S").tolist()) + b"\n"
    p2 = host.UnpackPlan(data["blob"], data["fa"])
    p2.contig_len[0] = 2 ** 31 - 1                      # room for 2^24 + 1 intervals one base apart
    with pytest.raises(host.CbcInputError, match="more than 2\\^24 intervals"):
        p2.targets((), bed)
    p2.close()


def test_refusals(built, data):
    pb, sam, fa = host.synth_long(5, 200_000, 40, read_len=2000, want_text=True)
    flat, offs, res = oracle.cpu_encode_blocks(pb, long_reads=True, return_flat=True)
    plan = host.UnpackPlan(pb.container(flat, offs), fa)
    with pytest.raises(host.CbcInputError, match="long-read"):
        plan.targets(["chrL:1-1000", "chrL:5000-6000"])
    plan.close(); pb.close()
    fa, sam, _, _ = synth.dataset(4, [5000], [100], 100)
    with pytest.raises(host.CbcInputError, match="not a cbc block container"):
        host.UnpackPlan(oracle.encode(sam, fa), fa)
    # names and lengths cbc_unpack_sam_header refuses: the plain-reads form too
    b = bytearray(data["blob"]); b[36 + 2] = 9                                # a tab inside "chr1"
    p = host.UnpackPlan(bytes(b), data["fa"])
    with pytest.raises(host.CbcInputError, match="holds a tab or a newline"):
        p.targets(["chr2:1-5", "chr2:9-10"])
    p.close()
    p = host.UnpackPlan(data["blob"], data["fa"])
    p.contig_len[1] = 2 ** 31
    with pytest.raises(host.CbcInputError, match="longer than 2\\^31 - 1 bases"):
        p.targets(["chr1:1-5"])
    p.close()


def _asan_env():
    return dict(os.environ, LD_PRELOAD=subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip(),
                ASAN_OPTIONS="detect_leaks=0")


def test_hostile_bed_under_asan(built, data, tmp_path):
    """Hostile BED text on the AddressSanitizer build of libcbc_host, in a child process: huge numbers, a line of 1 MB, NUL
    bytes, text that ends inside a field, inside a number and on a CR; every buffer is exactly as long as the text."""
    csrc = os.path.join(ROOT, "cbc_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "libcbc_host_asan.so"], stdout=subprocess.DEVNULL)
    (tmp_path / "in.cbc").write_bytes(data["blob"]); (tmp_path / "ref.fa").write_bytes(data["fa"])
    code = textwrap.dedent("""
        import sys
        sys.path.insert(0, %r)
        from cbc_amd import host
        host.HOST_LIB = %r
        p = host.UnpackPlan(open(%r, "rb").read(), open(%r, "rb").read())
        good = b"chr1\\t10\\t20\\nchr2 5 9\\r\\n"
        cases = [b"chr1\\t" + b"9" * 40 + b"\\t5\\n", b"chr1\\t1\\t" + b"9" * 19 + b"\\n", b"chr1\\t1\\t" + b"1" * (1 << 20) + b"\\n",
                 b"#" + b"x" * (1 << 20) + b"\\n", b"chr1\\0\\t1\\t5\\n", b"\\0\\0\\0", b"chr1\\t1\\0\\t5\\n", b"chr1\\t1\\t5\\0",
                 b"chr1", b"chr1\\t", b"chr1\\t1", b"chr1\\t1\\t", b"chr1\\t1\\t5\\r", b"\\r", b"\\t\\t\\t", b"   ", b"track", b"brows",
                 b"chr1\\t18446744073709551615\\t18446744073709551616\\n", b"\\xff\\xfe\\t1\\t2\\n"]
        n_err = n_ok = 0
        for c in cases:
            for text in (c, good + c, good + c + good):
                for cut in (len(text), len(text) - 1, len(text) // 2):
                    try:
                        p.targets((), text[:cut]); n_ok += 1
                    except host.CbcInputError as e:
                        assert "BED line" in str(e), e
                        n_err += 1
        print("HOSTILE OK", n_ok, n_err)
    """ % (ROOT, os.path.join(csrc, "libcbc_host_asan.so"), str(tmp_path / "in.cbc"), str(tmp_path / "ref.fa")))
    r = subprocess.run([sys.executable, "-c", code], env=_asan_env(), capture_output=True, text=True)
    assert r.returncode == 0 and "HOSTILE OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    n_ok, n_err = (int(x) for x in r.stdout.split("HOSTILE OK")[1].split())
    assert n_ok > 20 and n_err > 20


def test_asan_build_of_the_emulation(built):
    """Every pass, fed by the emulated decoder, on an AddressSanitizer / UBSan build of the emulation library in a child
    process: every table is allocated to its exact size there, so an index one past it is a finding."""
    subprocess.check_call(["make", "-C", EMU_DIR, "asan"], stdout=subprocess.DEVNULL)
    code = textwrap.dedent("""
        import sys
        sys.path[:0] = [%r, %r]
        import targetsmodel as tm
        L = tm.emu_load(%r)
        assert tm.selfcheck(L)
        print("TARGETS EMU OK")
    """ % (ROOT, os.path.join(ROOT, "tests"), os.path.join(EMU_DIR, "libcbc_targets_emu_asan.so")))
    r = subprocess.run([sys.executable, "-c", code], env=_asan_env(), capture_output=True, text=True)
    assert r.returncode == 0 and "TARGETS EMU OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- the CLI where no device is needed -----------------------------------------------------------------------------------------
def _cli(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def test_cli_refusals_and_empty_selection(built, data, tmp_path):
    (tmp_path / "in.cbc").write_bytes(data["blob"]); (tmp_path / "ref.fa").write_bytes(data["fa"])
    (tmp_path / "t.bed").write_bytes(b"chr1\t10\t20\n")
    (tmp_path / "bad.bed").write_bytes(b"chr1\t10\t20\nchr1\t30\t20\n")
    files = (tmp_path / "in.cbc", tmp_path / "o.txt", tmp_path / "ref.fa")
    two = ("--region", "chr1:1-5", "--region", "chr2:1-5")
    for args, msg in [(two + ("--devices", "0,1"), "one device"), (("--regions-file", tmp_path / "t.bed", "--devices", "0,1"), "one device"),
                      (two + ("--depth", "--sam"), "--depth and --sam"), (("--region", "chr1:1-5", "--region", "chrX:1-5"), "unknown contig"),
                      (("--regions-file", tmp_path / "bad.bed"), "BED line 2: start is past end"),
                      (("--regions-file", tmp_path / "none.bed"), "cannot open")]:
        r = _cli("-x", *files, *args)
        assert r.returncode == 1 and msg in r.stderr, (args, r.stderr)
    r = _cli("-c", tmp_path / "in.sam", tmp_path / "o.cbc", tmp_path / "ref.fa", "--regions-file", tmp_path / "t.bed")
    assert r.returncode == 1 and "--regions-file applies to decompression" in r.stderr, r.stderr
    fa, sam, _, _ = synth.dataset(4, [5000], [100], 100)
    (tmp_path / "c.cbc").write_bytes(oracle.encode(sam, fa)); (tmp_path / "c.fa").write_bytes(fa)
    r = _cli("-x", tmp_path / "c.cbc", tmp_path / "o.txt", tmp_path / "c.fa", "--regions-file", tmp_path / "t.bed")
    assert r.returncode == 1 and "single-stream (--compat) file" in r.stderr, r.stderr
    pb, _, lfa = host.synth_long(5, 200_000, 40, read_len=2000, want_text=True)
    flat, offs, _ = oracle.cpu_encode_blocks(pb, long_reads=True, return_flat=True)
    (tmp_path / "l.cbc").write_bytes(pb.container(flat, offs)); (tmp_path / "l.fa").write_bytes(lfa)
    r = _cli("-x", tmp_path / "l.cbc", tmp_path / "o.txt", tmp_path / "l.fa", "--region", "chrL:1-10", "--region", "chrL:50-60")
    assert r.returncode == 1 and "long-read" in r.stderr, r.stderr
    pb.close()
    # an empty selection: nothing opened on the device, an empty file (the header alone for --sam), status 0
    first = min(x[1] for x in data["iv"] if x[0] == 0)
    (tmp_path / "e.bed").write_bytes(b"chrUn\t1\t5\nchr1\t0\t%d\n" % (first - 1))
    for extra, want in (((), b""), (("--depth",), b""), (("--sam",), data["plan"].sam_header())):
        (tmp_path / "o.txt").write_bytes(b"stale")
        r = _cli("-x", *files, "--regions-file", tmp_path / "e.bed", "--verbose", *extra)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / "o.txt").read_bytes() == want and "kernels:" not in r.stdout and "1 BED lines selected nothing" in r.stdout


def test_exports_name_the_targets_entry_points(built):
    from cbc_amd import gpu
    assert {"cbc_gpu_decode_targets", "cbc_gpu_last_targets_ms"} <= set(gpu.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "cbc_gpu.h")).read()
    assert "cbc_gpu_decode_targets(" in hdr and "cbc_gpu_last_targets_ms(" in hdr
