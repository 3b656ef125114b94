"""Depth histogram without a GPU: the accumulate / count / write bodies of cbc_hist_body.h on the
lock-step wave emulation (tests/hist_emu) behind the emulated decode and depth passes and on fabricated change points (both
sides of CBC_HIST_LDS, bins past 2^31, folded depths), the stand-alone sanitizer program, the fraction rule through the CLI's
formatter, and the CLI where no device is needed.  Ground truth is histmodel.py: brute force over depthmodel.depth_array,
compared exactly."""
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
from cbc_amd import host
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "hist_emu")
EXE = os.path.join(ROOT, "cbc_amd", "csrc", "cbc")
TILE, LINES, LDS = 4096, 1024, 1024                         # CBC_DEPTH_TILE, CBC_DEPTH_LINES, CBC_HIST_LDS


@pytest.fixture(scope="module")
def emu(built):
    subprocess.check_call(["make", "-C", EMU_DIR, "libcbc_hist_emu.so"], stdout=subprocess.DEVNULL)
    return hm.emu_load(os.path.join(EMU_DIR, "libcbc_hist_emu.so"))


def _load(emu, make, **kw):
    fa, sam, pb, contigs = make(**kw)
    iv = dm.assert_models_agree(pb, sam)                    # the two models of section 4.13 agree before either is used
    names, lens = dm.names_lens(None, contigs)
    blob = rm.container(pb)
    plan = host.UnpackPlan(blob, fa)
    d = dict(fa=fa, pb=pb, blob=blob, plan=plan, iv=iv, names=names, lens=lens, depth=cm.Depth(iv, lens))
    d["dec"] = tm.emu_decode_all(emu, plan, pb.max_read_len + pb.read_length - 1)
    return d


@pytest.fixture(scope="module")
def mixed(emu):
    d = _load(emu, dm.mixed, seed=11, block_reads=64, n=3000)
    yield d
    d["plan"].close(); d["pb"].close()


@pytest.fixture(scope="module")
def ramp(emu):
    d = _load(emu, dm.ramp)
    yield d
    d["plan"].close(); d["pb"].close()


def _run(emu, d, ivs=None, regions=(), extra_bed=b"", exclude=0, max_depth=0, depth=None, fail_blocks=()):
    """ivs ((contig, beg, end), 1-based inclusive) as a BED text behind the region strings `regions` (given with their own
    intervals as (string, (contig, beg, end))); neither: every contig whole.  Through cbc_unpack_targets / cbc_unpack_queries
    and the emulation, against the model."""
    plan = d["plan"]
    if ivs is None and not regions:
        ts, given = plan.queries().targets, None
    else:
        ts = plan.targets([r for r, _ in regions], tm.bed(ivs or [], d["names"]) + extra_bed)
        given = [q for _, q in regions] + list(ivs or [])
    rows, rcs = hm.emu_hist(emu, plan, d["dec"], ts, exclude, max_depth, fail_blocks)
    want = hm.expected(depth or d["depth"], d["lens"], given, max_depth)
    assert rows == want, [(a, b) for a, b in zip(rows, want) if a != b][:2]
    for _, bins, size in rows:
        assert sum(n for _, n in bins) == size and [k for k, _ in bins] == sorted(k for k, _ in bins)
    return ts, rows, rcs


def _bed_set(d):
    """Touching, overlapping, duplicate and unsorted lines on two contigs, with empty and unknown lines between them."""
    L = d["lens"]
    first = min(x[1] for x in d["iv"] if x[0] == 0)
    ivs = [(0, first + 10, first + 40), (0, first + 41, first + 60), (0, first + 55, first + 120), (0, first + 10, first + 40),
           (len(L) - 1, 1, 300), (0, first, first), (0, first + 200, first + 201), (0, 1, 3)]
    assert first + 201 <= L[0] and L[-1] >= 300
    extra = b"chrUn_gl0\t5\t900\n%s\t700\t700\n%s\t999999999\t1000000005\n" % (d["names"][0], d["names"][0])
    return ivs, extra


def test_whole_region_and_bed_sets(emu, mixed, ramp):
    for d in (mixed, ramp):
        L, names = d["lens"], d["names"]
        ts, rows, rcs = _run(emu, d)                         # every contig whole, in table order
        assert [r[0] for r in rows] == list(range(len(L))) and [r[2] for r in rows] == L and all(rc == 0 for rc in rcs)
        assert max(L) + 1 > TILE and all(r[1][0][0] == 0 for r in rows)          # depth 0 has bases on every contig
        c = 0
        mid = L[c] // 2 if d is mixed else 100_000
        ts, rows, _ = _run(emu, d, regions=[(b"%s:%d-%d" % (names[c], mid - 40, mid + 600), (c, mid - 40, mid + 600))])
        assert [r[0] for r in rows] == [c] and rows[0][2] == 641 and mid + 600 <= L[c]
        ivs, extra = _bed_set(d)
        ts, rows, _ = _run(emu, d, ivs, extra_bed=extra)
        assert ts.bed_unselected == 3 and [r[0] for r in rows] == [0, len(L) - 1] and ts.n_iv < len(ivs)
        # a region string and a file together; the same interval twice counts once
        _run(emu, d, ivs[:3], regions=[(b"%s:%d-%d" % (names[0], ivs[0][1], ivs[0][2]), ivs[0])])


def test_interval_sets_that_cross_a_tile(emu, mixed):
    """Slots that cross CBC_DEPTH_TILE inside an interval and exactly at an interval's spare slot, and more intervals than one
    wavefront: the spare slots never reach a bin."""
    d = mixed
    a = d["lens"][0] // 3
    _, rows, _ = _run(emu, d, [(0, a + 1, a + TILE - 1), (0, a + TILE + 11, a + TILE + 30), (0, a + 2 * TILE + 1, a + 3 * TILE + 7)])
    assert rows[0][2] == TILE - 1 + 20 + TILE + 7
    _, rows, _ = _run(emu, d, tm.dense_set(0, 500, 4100, 13, 6))
    assert rows[0][2] == 4100 * 6


def test_exclude_flags(emu, mixed, ramp):
    for ex in (16, 1024, 1040):                              # the ramp alternates FLAG 16 and 1040
        _, rows, _ = _run(emu, ramp, exclude=ex, depth=cm.Depth(ramp["iv"], ramp["lens"], ex))
        assert (rows[0][1] == [(0, ramp["lens"][0])]) == bool(ex & 16)
    ivs, extra = _bed_set(mixed)
    _run(emu, mixed, ivs, extra_bed=extra, exclude=16, depth=cm.Depth(mixed["iv"], mixed["lens"], 16))
    _run(emu, mixed, exclude=16, max_depth=3, depth=cm.Depth(mixed["iv"], mixed["lens"], 16))


def test_max_depth(emu, mixed, ramp):
    top = int(ramp["depth"].contig(0).max())
    assert top == 100
    plain = _run(emu, ramp)[1]
    for md in (1, 2, top - 1, top, top + 1, 2 ** 32 - 1, 0):
        _, rows, _ = _run(emu, ramp, max_depth=md)
        assert max(k for k, _ in rows[0][1]) == (min(md, top) if md else top)
        assert (rows == plain) == (md == 0 or md >= top)
    _, rows, _ = _run(emu, ramp, max_depth=1)
    assert len(rows[0][1]) == 2 and rows[0][1][1][1] == int((ramp["depth"].contig(0) > 0).sum())
    mtop = int(mixed["depth"].contig(0).max())
    for md in (1, mtop, mtop + 5):
        _run(emu, mixed, max_depth=md)


def test_failed_block_gives_no_bins(emu, mixed):
    d = mixed
    ts = d["plan"].queries().targets
    k = 1
    assert int(ts.blocks[k]) == 1 and int(ts.contig_blk_first[0]) == 0
    rows, rcs = hm.emu_hist(emu, d["plan"], d["dec"], ts, fail_blocks=(k,))
    assert rcs == [-4, 0, 0]                                 # CBC_E_BLOCK from the call that held the block
    assert rows[0] == (0, [(0, d["lens"][0])], d["lens"][0])                     # no bins: everything stays in depth 0
    assert rows[1:] == hm.expected(d["depth"], d["lens"])[1:]


def test_empty_selections(emu, mixed):
    d, L = mixed, mixed["lens"]
    first, f3 = (min(x[1] for x in d["iv"] if x[0] == c) for c in (0, 2))
    assert first > 3 and f3 > 3
    # contigs whose intervals no block reaches: depth 0 = size, and no call
    ts, rows, rcs = _run(emu, d, [(0, 1, first - 1), (2, 2, f3 - 1), (0, 2, 3)])
    assert ts.n_blocks == 0 and rcs == [] and rows == [(0, [(0, first - 1)], first - 1), (2, [(0, f3 - 2)], f3 - 2)]
    assert hm.text(rows, d["names"]) == (b"chr1\t0\t%d\t%d\t1.000000\nchr3\t0\t%d\t%d\t1.000000\ngenome\t0\t%d\t%d\t1.000000\n"
                                         % (first - 1, first - 1, f3 - 2, f3 - 2, first + f3 - 3, first + f3 - 3))
    # intervals behind the last read: the contig's last block is selected and decoded, and every position has depth 0
    ts, rows, rcs = _run(emu, d, [(2, L[2] - 99, L[2])])
    assert ts.n_blocks == 1 and rcs == [0] and rows == [(2, [(0, 100)], 100)]
    # no contig at all
    ts = d["plan"].targets((), b"chrUn\t1\t5\nchr2\t9\t9\n")
    assert hm.emu_hist(emu, d["plan"], d["dec"], ts) == ([], []) and hm.text([], d["names"]) == b""


def _points(runs, start=5):
    """[(depth, length)] -> change points; the last one has depth 0."""
    pos, dep, at = [], [], start
    for k, n in runs:
        pos.append(at); dep.append(k); at += n
    return pos + [at], dep + [0]


def test_fabricated_change_points(emu):
    def check(pos, dep, reads, md=0, grid=0):
        rc, n, bins = hm.emu_points(emu, pos, dep, reads, md, grid)
        want = hm.points_expected(pos, dep, md)
        assert rc == 0 and n == len(want) and bins == want, (md, grid, bins[:4], want[:4])
        return bins
    # both sides of CBC_HIST_LDS; folds that send both paths into the same bin; zero-depth runs between non-zero ones
    pos, dep = _points([(LDS - 1, 10), (LDS, 11), (LDS + 1, 12), (0, 13), (1, 14), (LDS - 1, 15), (0, 16), (0, 17), (LDS, 18), (2000, 19),
                        (LDS + 1, 20), (7, 21), (LDS - 1, 22)])
    assert [k for k, _ in check(pos, dep, 2000)] == [1, 7, LDS - 1, LDS, LDS + 1, 2000]
    for md in (LDS + 1, LDS, LDS - 1, 2, 1, 1999, 2000, 2001):
        check(pos, dep, 2000, md)
    assert check(pos, dep, 2000, LDS)[-1] == (LDS, 11 + 12 + 18 + 19 + 20)
    # three runs of 10^9 slots at one depth: the bin passes 2^31, in the LDS table and in the global one
    for k in (3, 3000):
        pos, dep = _points([(k, 10 ** 9), (0, 7)] * 3, 0)
        assert check(pos, dep, 5000) == [(k, 3 * 10 ** 9)] and 3 * 10 ** 9 > 2 ** 31
    # a depth near 4 * 10^9 folded by M
    pos, dep = _points([(4_000_000_000, 12345), (3_999_999_999, 1), (5000, 9), (4999, 4)], 100)
    assert check(pos, dep, 2 ** 30 - 1, 5000) == [(4999, 4), (5000, 12355)]
    assert check(pos, dep, 2 ** 30 - 1, 900) == [(900, 12359)]
    # ncp of 0, 1 and 2
    assert check([], [], 10) == [] and check([9], [0], 10) == [] and check([9, 49], [6, 0], 10) == [(6, 40)]
    # more runs than grid * tile: the stride loop turns; the last tile is partial
    runs = [(0 if i % 5 == 0 else 1 + (i * 7) % 1500, 1 + i % 9) for i in range(5 * LINES + 77)]
    pos, dep = _points(runs, 1)
    a = check(pos, dep, 1500, 0, 2)
    assert a == check(pos, dep, 1500, 0, 1) == check(pos, dep, 1500, 0, 0) and len(a) > LDS
    check(pos, dep, 1500, 1100, 2)
    # bin_cap one too small: the count comes back, no pair does
    pos, dep = _points([(3, 5), (9, 5), (3, 1), (2000, 2)])
    assert hm.emu_points(emu, pos, dep, 2000, bin_cap=2) == (-1, 3, [])
    assert hm.emu_points(emu, pos, dep, 2000, bin_cap=3) == (0, 3, [(3, 6), (9, 5), (2000, 2)])


def test_sanitizer_build_of_the_stand_alone_check(built):
    """hist_emu_check: the fabricated cases in a program of its own under AddressSanitizer / UBSan, every table at its exact
    size; it exits non-zero on a finding or a mismatch."""
    subprocess.check_call(["make", "-C", EMU_DIR, "asan_check"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(EMU_DIR, "hist_emu_check")], capture_output=True, text=True)
    assert r.returncode == 0 and "HIST EMU CHECK OK" in r.stdout and "MISMATCH" not in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_fraction_rule_through_the_formatter(built):
    for bases, size, want in [(1, 1, b"1.000000"), (0, 1, b"0.000000"), (1, 3, b"0.333333"), (2, 3, b"0.666667"), (3, 3, b"1.000000"),
                              (1, 2 ** 31, b"0.000000"), (1074, 2 ** 31, b"0.000001"), (1073, 2 ** 31, b"0.000000"), (2 ** 31, 2 ** 31, b"1.000000"),
                              (2 ** 31 - 1, 2 ** 31, b"1.000000"), (2 ** 30, 2 ** 31, b"0.500000"), (0, 0, b"0.000000"), (5, 0, b"0.000000"),
                              (1, 2_000_000, b"0.000001"), (1, 2_000_001, b"0.000000"), (2 ** 62, 2 ** 63, b"0.500000"), (2 ** 63 + 5, 2 ** 63 + 5, None)]:
        got = host.hist_fraction(bases, size)
        assert got == hm.fraction(bases, size) and (want is None or got == want), (bases, size, got)


# ---- the CLI where no device is needed -----------------------------------------------------------------------------------------
def _cli(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def test_cli_refusals_and_empty_selection(built, mixed, tmp_path):
    d = mixed
    (tmp_path / "in.cbc").write_bytes(d["blob"]); (tmp_path / "ref.fa").write_bytes(d["fa"])
    files = (tmp_path / "in.cbc", tmp_path / "o.txt", tmp_path / "ref.fa")
    for args, msg in [(("--depth-hist", "--sam"), "different outputs"), (("--depth-hist", "--depth"), "different outputs"),
                      (("--depth-hist", "--bedcov"), "different outputs"), (("--depth-hist", "--devices", "0,1"), "one device"),
                      (("--hist-max", "5"), "--hist-max applies to --depth-hist"), (("--depth", "--hist-max", "5"), "--hist-max applies to --depth-hist"),
                      (("--depth-hist", "--hist-max", "0"), "--hist-max wants"), (("--depth-hist", "--hist-max", "x"), "--hist-max wants"),
                      (("--depth-hist", "--hist-max", "4294967296"), "--hist-max wants"),
                      (("--depth-hist", "--window", "100"), "--window applies to --bedcov"), (("--depth-hist", "--min-depth", "2"), "--min-depth applies to --bedcov"),
                      (("--depth-exclude-flags", "4"), "--depth-exclude-flags applies to --depth"),
                      (("--depth-hist", "--region", "chrX:1-5"), "unknown contig"), (("--depth-hist", "--regions-file", tmp_path / "none.bed"), "cannot open")]:
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
    for extra in ((), ("--region", "chr1:1-50")):
        r = _cli("-x", tmp_path / "l.cbc", tmp_path / "o.txt", tmp_path / "l.fa", "--depth-hist", *extra)
        assert r.returncode == 1 and "long-read" in r.stderr, r.stderr
    pb.close()
    b = bytearray(d["blob"]); b[36 + 2] = 9                                   # a tab inside "chr1": what cbc_unpack_sam_header refuses
    (tmp_path / "t.cbc").write_bytes(bytes(b))
    for extra in ((), ("--region", "chr2:1-5")):
        r = _cli("-x", tmp_path / "t.cbc", tmp_path / "o.txt", tmp_path / "ref.fa", "--depth-hist", *extra)
        assert r.returncode == 1 and "holds a tab or a newline" in r.stderr, r.stderr
    # intervals that no block reaches: no device is opened, the depth-0 lines and the genome block are written, status 0
    first, f3 = (min(x[1] for x in d["iv"] if x[0] == c) for c in (0, 2))
    assert first > 3 and f3 > 3
    (tmp_path / "e.bed").write_bytes(b"chrUn\t1\t5\nchr1\t0\t%d\nchr2\t9\t9\nchr3\t1\t%d\nchr1\t2\t4\n" % (first - 1, f3 - 1))
    (tmp_path / "o.txt").write_bytes(b"stale")
    r = _cli("-x", *files, "--depth-hist", "--regions-file", tmp_path / "e.bed", "--verbose", "--hist-max", "7", "--depth-exclude-flags", "16")
    assert r.returncode == 0, r.stderr
    rows = [(0, [(0, first - 1)], first - 1), (2, [(0, f3 - 2)], f3 - 2)]
    assert (tmp_path / "o.txt").read_bytes() == hm.text(rows, d["names"]) != b""
    assert "kernels:" not in r.stdout and "2 contigs" in r.stdout and "2 BED lines selected nothing" in r.stdout
    # no contig at all: an empty file, status 0
    (tmp_path / "n.bed").write_bytes(b"chrUn\t1\t5\nchr2\t9\t9\n")
    (tmp_path / "o.txt").write_bytes(b"stale")
    r = _cli("-x", *files, "--depth-hist", "--regions-file", tmp_path / "n.bed")
    assert r.returncode == 0 and (tmp_path / "o.txt").read_bytes() == b"", r.stderr


def test_exports_name_the_histogram_entry_points(built):
    from cbc_amd import gpu
    assert {"cbc_gpu_decode_depth_hist", "cbc_gpu_last_hist_ms"} <= set(gpu.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "cbc_gpu.h")).read()
    assert "cbc_gpu_decode_depth_hist(" in hdr and "cbc_gpu_last_hist_ms(" in hdr
    hdr = open(os.path.join(ROOT, "include", "cbc_host.h")).read()
    assert "cbc_hist_fraction(" in hdr and "cbc_unpack_targets_size(" in hdr
    for f in ("cbc_hist_fraction", "cbc_unpack_targets_size"):
        getattr(host.lib(), f)
    assert hasattr(gpu.Encoder, "decode_depth_hist") and hasattr(gpu.Encoder, "last_hist_ms")
