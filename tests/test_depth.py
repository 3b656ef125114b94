"""Coverage output without a GPU: the mark, tile, change-point, count and write bodies of
cbc_depth_body.h on the lock-step wave emulation (tests/depth_emu), fed by the emulated span decoder, against the Python
models (depthmodel.py); the same under ASan / UBSan; cbc_unpack_depth_text_cap; and what the CLI decides without a device."""
import os
import struct
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import depthmodel as dm
import regionmodel as rm
import synth
from cbc_amd import host
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "depth_emu")
EXE = os.path.join(ROOT, "cbc_amd", "csrc", "cbc")


@pytest.fixture(scope="module")
def emu(built):
    subprocess.check_call(["make", "-C", EMU_DIR, "libcbc_depth_emu.so"], stdout=subprocess.DEVNULL)
    return dm.emu_load(os.path.join(EMU_DIR, "libcbc_depth_emu.so"))


def _open(fa, sam, pb, contigs, **extra):
    blob = rm.container(pb)
    names, lens = dm.names_lens(None, contigs)
    return dict(fa=fa, sam=sam, pb=pb, blob=blob, plan=host.UnpackPlan(blob, fa), names=names, lens=lens, **extra)


@pytest.fixture(scope="module", params=[256, 1024])
def data(request, built):
    """Several contigs, mixed read lengths, indels, the deletion read across the first block boundary; no soft clips, so the
    codec's view and the SAM text must agree on every read before either is used."""
    d = _open(*dm.mixed(7 + request.param, request.param), block_reads=request.param)
    d["iv"] = dm.assert_models_agree(d["pb"], d["sam"])
    assert d["iv"] == [x + (y[4],) for x, y in zip(dm.intervals_b(d["sam"]), d["iv"])]
    yield d
    d["plan"].close(); d["pb"].close()


@pytest.fixture(scope="module")
def ramp(built):
    d = _open(*dm.ramp())
    d["iv"] = dm.assert_models_agree(d["pb"], d["sam"])
    yield d
    d["plan"].close(); d["pb"].close()


def test_models_on_a_known_answer():
    """The model itself, by hand: three reads on a 20-base contig."""
    iv = [(0, 2, 5, 0, 0), (0, 4, 5, 16, 0), (0, 15, 3, 0, 0), (0, 9, 0, 0, 0)]        # the last one covers nothing
    assert dm.expected(iv, [b"c"], [20]) == (b"c\t1\t3\t1\nc\t3\t6\t2\nc\t6\t8\t1\nc\t14\t17\t1\n", 4, 3)
    assert dm.expected(iv, [b"c"], [20], (0, 5, 15)) == (b"c\t4\t6\t2\nc\t6\t8\t1\nc\t14\t15\t1\n", 3, 3)
    assert dm.expected(iv, [b"c"], [20], None, 16) == (b"c\t1\t6\t1\nc\t14\t17\t1\n", 2, 2)
    assert dm.expected(iv, [b"c"], [20], (0, 9, 13)) == (b"", 0, 0)
    sam = b"@SQ\tSN:c\tLN:20\nr\t0\tc\t2\t60\t2S3M2D1I1N1X1=\t*\t0\t0\tAAAAAAAA\t*\n"
    assert dm.intervals_b(sam) == [(0, 2, 8, 0)]


def test_whole_container_matches_both_models(emu, data):
    plan, iv = data["plan"], data["iv"]
    want = dm.expected(iv, data["names"], data["lens"])
    assert want == dm.expected(dm.intervals_b(data["sam"]), data["names"], data["lens"])       # model (b): the SAM text
    got = dm.emu_whole(emu, plan)
    assert got == want
    rows = dm.parse(got[0])
    assert [r[0] for r in rows] == sorted((r[0] for r in rows), key=data["names"].index)       # contigs in table order
    assert {r[0] for r in rows} == set(data["names"]) and want[2] == data["pb"].n_recs
    for n in data["names"]:                                                                 # runs in position order, maximal
        rr = [r for r in rows if r[0] == n]
        assert all(a[2] <= b[1] for a, b in zip(rr, rr[1:])) and all(r[1] < r[2] and r[3] > 0 for r in rr)
        assert not any(a[2] == b[1] and a[3] == b[3] for a, b in zip(rr, rr[1:]))
    assert len({len(s) for _, _, _, _, s in rm.records(data["pb"])}) == 2                     # mixed read lengths


def test_windows_match_the_model(emu, data):
    plan, iv, pb = data["plan"], data["iv"], data["pb"]
    wins = dm.windows(pb, iv, data["block_reads"], data["lens"], 60, 2)
    n_cut = n_empty = 0
    for s, c, beg, end in wins:
        sel = plan.region(s)
        assert (sel.contig, sel.beg, sel.end) == (c, beg, end)
        want = dm.expected(iv, data["names"], data["lens"], (c, beg, end))
        rc, text, runs, kept, _ = dm.emu_call(emu, plan, sel)
        assert rc == 0 and (text, runs, kept) == want, s
        rows = dm.parse(text)
        assert all(beg - 1 <= r[1] and r[2] <= end for r in rows), s                          # reads clipped to the window
        n_cut += any(x[0] == c and (x[1] < beg <= x[1] + x[2] - 1 or x[1] <= end < x[1] + x[2] - 1) for x in iv)
        n_empty += not rows
    assert n_cut >= 40 and n_empty >= 4, (n_cut, n_empty)                                    # windows inside reads; without reads
    assert sum(1 for s, c, b, e in wins if b == e) >= 6                                      # one-base windows


def test_deletion_read_counts_its_deleted_bases(emu, data):
    """The span of the deletion read (50M40D50M) is 140: the 40 deleted bases are covered, in block 1's territory too."""
    plan, iv = data["plan"], data["iv"]
    d = [x for x in iv if x[4] == 0][-1]
    assert d[2] == 140 and int(plan.window_start[1]) + 1 < d[1] + 139
    for at in (d[1] + 60, d[1] + 139):
        sel = plan.region("chr1:%d-%d" % (at, at))
        rc, text, runs, kept, _ = dm.emu_call(emu, plan, sel)
        want = dm.expected(iv, data["names"], data["lens"], (0, at, at))
        assert rc == 0 and (text, runs, kept) == want and runs == 1
        without = dm.expected([x for x in iv if x is not d], data["names"], data["lens"], (0, at, at))
        assert dm.parse(text)[0][3] == (dm.parse(without[0])[0][3] if without[0] else 0) + 1


def test_exclude_masks(emu, data, ramp):
    plan, iv = data["plan"], data["iv"]
    n16 = sum(1 for x in iv if x[3] & 16)
    assert 0 < n16 < len(iv)
    got = dm.emu_whole(emu, plan, 16)
    assert got == dm.expected(iv, data["names"], data["lens"], None, 16) and got[2] == len(iv) - n16
    assert got == dm.expected([x for x in iv if not x[3] & 16], data["names"], data["lens"])
    # the ramp's reads carry FLAG 16 or 1040: 1024 drops every second read, 16 drops all of them
    p2, iv2 = ramp["plan"], ramp["iv"]
    got = dm.emu_whole(emu, p2, 1024)
    assert got == dm.expected(iv2, ramp["names"], ramp["lens"], None, 1024) and 0 < got[2] < len(iv2)
    assert dm.emu_whole(emu, p2, 16) == (b"", 0, 0)
    assert dm.emu_whole(emu, p2, 0xffff) == (b"", 0, 0)


def test_digit_count_edges(emu, ramp):
    """Depth through 9 -> 10 and 99 -> 100, positions through 99999 -> 100000 (the hi * 10^5 + lo split of the digits)."""
    plan, iv = ramp["plan"], ramp["iv"]
    want = dm.expected(iv, ramp["names"], ramp["lens"])
    got = dm.emu_whole(emu, plan)
    assert got == want
    rows = dm.parse(got[0])
    depths = [r[3] for r in rows if r[0] == b"rampA"]
    assert {9, 10, 99, 100} <= set(depths) and max(depths) == 100
    assert any(r[1] == 99_999 and r[2] == 100_000 for r in rows) and any(r[1] == 100_000 for r in rows)
    assert [r for r in rows if r[0] == b"rampB"] == [(b"rampB", 0, 100, 1), (b"rampB", 3999, 4099, 1)]
    for beg, end in ((99_999, 100_000), (100_000, 100_000), (99_990, 100_010), (1, 99_999)):
        rc, text, runs, kept, _ = dm.emu_call(emu, plan, plan.region("rampA:%d-%d" % (beg, end)))
        assert rc == 0 and (text, runs, kept) == dm.expected(iv, ramp["names"], ramp["lens"], (0, beg, end)), (beg, end)


def test_failed_block_marks_nothing(emu, data):
    plan, iv = data["plan"], data["iv"]
    sel = plan.contig_blocks(0)
    assert sel.b1 - sel.b0 >= 3 and (sel.beg, sel.end) == (1, data["lens"][0])
    rc, text, runs, kept, _ = dm.emu_call(emu, plan, sel, fail_blocks=(1,))
    assert rc == 0 and (text, runs, kept) == dm.expected(iv, data["names"], data["lens"], (0, 1, data["lens"][0]), 0, (1,))
    assert kept == sum(1 for x in iv if x[0] == 0 and x[4] != 1)


def test_name_longer_than_the_limit_writes_nothing(emu, data):
    """The name_len guard of the run-text skeleton through the window member: no line is counted, nothing is written (the
    helper checks every byte of the buffer), while the mark pass still counts the reads."""
    plan = data["plan"]
    sel = plan.contig_blocks(0)
    rc, text, lines, kept, total = dm.emu_call(emu, plan, sel, name=b"n" * 256)               # CBC_SAM_MAX_NAME + 1
    assert (rc, text, lines, total) == (0, b"", 0, 0) and kept > 0
    cap = plan.depth_text_cap(sel.b0, sel.b1, 0) // 34 * (255 + 34)                             # the cap counts the real name
    rc, text, lines, kept2, total = dm.emu_call(emu, plan, sel, name=b"n" * 255, cap=cap)
    assert rc == 0 and lines > 0 and kept2 == kept and text.startswith(b"n" * 255 + b"\t") and total == len(text)
    # zero bytes: no block marks anything, so there is no run; every text tile counts 0 bytes and its write pass ends there
    assert dm.emu_call(emu, plan, sel, fail_blocks=range(sel.b1 - sel.b0)) == (0, b"", 0, 0, 0)


def test_text_cap(emu, data, ramp):
    for d in (data, ramp):
        plan, iv = d["plan"], d["iv"]
        for c in range(plan.n_contigs):
            sel = plan.contig_blocks(c)
            want = dm.expected(iv, d["names"], d["lens"], (c, 1, d["lens"][c]))
            k = sum(int(plan.blocks[b]["n_reads"]) for b in range(sel.b0, sel.b1))
            cap = plan.depth_text_cap(sel.b0, sel.b1, c)
            assert cap == (2 * k - 1) * (len(d["names"][c]) + 34) and len(want[0]) <= cap and want[1] <= 2 * k - 1
            rc, text, runs, kept, total = dm.emu_call(emu, plan, sel, cap=len(want[0]))
            assert rc == 0 and text == want[0]
            rc, text, runs, kept, total = dm.emu_call(emu, plan, sel, cap=len(want[0]) - 1)         # one byte short: reported
            assert rc == -1 and total == len(want[0]) and text == b""
        assert plan.depth_text_cap(0, plan.n_blocks + 1, 0) == 0 and plan.depth_text_cap(2, 1, 0) == 0
        assert plan.depth_text_cap(0, 1, plan.n_contigs) == 0 and plan.depth_text_cap(0, 0, 0) == 0


def test_contig_blocks(data):
    plan, pb = data["plan"], data["pb"]
    for c in range(plan.n_contigs):
        sel = plan.contig_blocks(c)
        bs = [b for b in range(pb.n_blocks) if int(pb.info[b]["contig"]) == c]
        assert (sel.contig, sel.b0, sel.b1, sel.beg, sel.end) == (c, bs[0], bs[-1] + 1, 1, data["lens"][c])
        assert sel.smax == pb.max_read_len + pb.read_length - 1


def test_asan_build_of_the_emulation(built):
    """Every pass, fed by the emulated decoder, on an AddressSanitizer / UBSan build of the emulation library, in a child
    process: arrays are allocated to their exact sizes there, so an index one past a table is a finding."""
    subprocess.check_call(["make", "-C", EMU_DIR, "asan"], stdout=subprocess.DEVNULL)
    code = textwrap.dedent("""
        import sys
        sys.path[:0] = [%r, %r]
        import depthmodel as dm
        L = dm.emu_load(%r)
        assert dm.selfcheck(L)
        print("DEPTH EMU OK")
    """ % (ROOT, os.path.join(ROOT, "tests"), os.path.join(EMU_DIR, "libcbc_depth_emu_asan.so")))
    env = dict(os.environ, LD_PRELOAD=subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip(),
               ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and "DEPTH EMU OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- the CLI where no device is needed -----------------------------------------------------------------------------------------
def _cli(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def test_cli_refusals(built, data, tmp_path):
    (tmp_path / "in.cbc").write_bytes(data["blob"]); (tmp_path / "ref.fa").write_bytes(data["fa"])
    (tmp_path / "in.sam").write_bytes(data["sam"])
    files = (tmp_path / "in.cbc", tmp_path / "o.bg", tmp_path / "ref.fa")
    r = _cli("-c", tmp_path / "in.sam", tmp_path / "o.cbc", tmp_path / "ref.fa", "--depth")
    assert r.returncode == 1 and "--depth applies to decompression" in r.stderr, r.stderr
    r = _cli("-x", *files, "--depth", "--sam")
    assert r.returncode == 1 and "--depth and --sam" in r.stderr, r.stderr
    r = _cli("-x", *files, "--depth", "--devices", "0,1")
    assert r.returncode == 1 and "one device" in r.stderr, r.stderr
    r = _cli("-x", *files, "--depth", "--depth-exclude-flags", "70000")
    assert r.returncode == 1 and "FLAG mask" in r.stderr, r.stderr
    r = _cli("-x", *files, "--depth", "--region", "chrX:1-5")
    assert r.returncode == 1 and "unknown contig" in r.stderr, r.stderr
    r = _cli("-x", *files, "--depth", "--region", "chr1:9-5")
    assert r.returncode == 1 and "ends before" in r.stderr, r.stderr
    fa, sam, _, _ = synth.dataset(4, [5000], [100], 100)
    (tmp_path / "c.cbc").write_bytes(oracle.encode(sam, fa)); (tmp_path / "c.fa").write_bytes(fa)
    r = _cli("-x", tmp_path / "c.cbc", tmp_path / "o.bg", tmp_path / "c.fa", "--depth")
    assert r.returncode == 1 and "single-stream (--compat) file" in r.stderr, r.stderr
    pb, _, lfa = host.synth_long(5, 200_000, 40, read_len=2000, want_text=True)
    flat, offs, _ = oracle.cpu_encode_blocks(pb, long_reads=True, return_flat=True)
    (tmp_path / "l.cbc").write_bytes(pb.container(flat, offs)); (tmp_path / "l.fa").write_bytes(lfa)
    r = _cli("-x", tmp_path / "l.cbc", tmp_path / "o.bg", tmp_path / "l.fa", "--depth")
    assert r.returncode == 1 and "long-read" in r.stderr, r.stderr
    pb.close()
    # a name the text cannot carry: the check of cbc_unpack_sam_header, not a second one
    b = bytearray(data["blob"]); b[36 + 2] = 9                                # a tab inside "chr1"
    (tmp_path / "t.cbc").write_bytes(bytes(b))
    r = _cli("-x", tmp_path / "t.cbc", tmp_path / "o.bg", tmp_path / "ref.fa", "--depth")
    assert r.returncode == 1 and "holds a tab or a newline" in r.stderr, r.stderr
    p = host.UnpackPlan(bytes(b), data["fa"])
    with pytest.raises(host.CbcInputError, match="holds a tab or a newline"):
        p.sam_header()
    p.close()


def test_cli_empty_selection_needs_no_device(built, data, tmp_path):
    """A window in front of the contig's first read selects no block: an empty file, status 0, no device opened."""
    (tmp_path / "in.cbc").write_bytes(data["blob"]); (tmp_path / "ref.fa").write_bytes(data["fa"])
    first = min(x[1] for x in data["iv"] if x[0] == 0)
    assert first > 1
    sel = data["plan"].region("chr1:1-%d" % (first - 1))
    assert sel.b0 == sel.b1
    (tmp_path / "o.bg").write_bytes(b"stale")
    r = _cli("-x", tmp_path / "in.cbc", tmp_path / "o.bg", tmp_path / "ref.fa", "--depth", "--region", "chr1:1-%d" % (first - 1), "--verbose")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "o.bg").read_bytes() == b"" and "kernels:" not in r.stdout and "0 runs" in r.stdout


def test_exports_name_the_depth_entry_points(built):
    from cbc_amd import gpu
    assert {"cbc_gpu_decode_depth", "cbc_gpu_last_depth_ms"} <= set(gpu.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "cbc_gpu.h")).read()
    assert "cbc_gpu_decode_depth(" in hdr and "cbc_gpu_last_depth_ms(" in hdr
