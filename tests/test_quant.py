"""Per-query depth quantiles without a GPU: the selection body of cbc_quant_body.h on the lock-step wave
emulation (tests/quant_emu) on fabricated change points and behind the emulated decode, mark, tile and compact passes; the
stand-alone sanitizer check of the emulation; the CLI where no device is needed.  Ground truth is quantmodel.py: a sort of the
per-base depth of every query, or of the (depth, length) pairs of fabricated runs, compared exactly."""
import inspect
import itertools
import os
import subprocess

import numpy as np
import pytest

import covmodel as cm
import depthmodel as dm
import quantmodel as qm
import regionmodel as rm
import targetsmodel as tm
from cbc_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "quant_emu")
EXE = os.path.join(ROOT, "cbc_amd", "csrc", "cbc")
LINES, LDS = 1024, 1024                                     # CBC_DEPTH_LINES, CBC_QUANT_LDS
P5 = (0, 1, 50, 99, 100)
P8 = (0, 1, 25, 50, 75, 90, 99, 100)


@pytest.fixture(scope="module")
def emu(built):
    subprocess.check_call(["make", "-C", EMU_DIR, "libcbc_quant_emu.so"], stdout=subprocess.DEVNULL)
    return qm.emu_load(os.path.join(EMU_DIR, "libcbc_quant_emu.so"))


def _points(emu, pos, dep, slots, pcts, q):
    got, want = qm.emu_points(emu, pos, dep, slots, pcts, q), qm.points_expected(pos, dep, pcts, q)
    assert got == want, [(x, a, b) for x, a, b in zip(q, got, want) if a != b][:5]
    for row in got:
        assert all(a <= b for a, b in zip(row, row[1:]))     # a higher percentage never gives less
    return got


# ---- fabricated change points ----------------------------------------------------------------------------------------------------
def test_no_run_one_position_and_change_points(emu):
    qq = [(0, 100), (5, 0), (9, 1), (8, 1), (48, 1), (49, 1), (100, 0), (0, 9), (0, 10), (9, 40), (8, 42), (20, 5), (50, 50)]
    assert qm.emu_points(emu, [], [], 100, P5, qq) == [[0] * 5] * len(qq)                      # ncp 0
    assert qm.emu_points(emu, [49], [7], 100, P5, qq) == [[0] * 5] * len(qq)                   # ncp 1: a change point starts no run
    got = _points(emu, [9, 49], [6, 0], 100, P5, qq)                                            # ncp 2: one run
    assert got[0] == [0, 0, 0, 6, 6] and got[2] == [6] * 5 and got[3] == [0] * 5 and got[4] == [6] * 5 and got[5] == [0] * 5
    assert got[1] == got[6] == [0] * 5                       # no position
    assert got[9] == [6] * 5 and got[10] == [0, 0, 6, 6, 6]  # the run exactly; one zero on either side
    # in front of the first change point, behind the last, inside a zero run, inside one run, starting / ending on a change point
    pos, dep = [10, 20, 30, 40, 50, 60], [3, 0, 9, 9, 2, 0]
    qq = [(0, 10), (0, 5), (60, 30), (70, 5), (20, 10), (22, 5), (32, 5), (10, 10), (30, 20), (29, 2), (30, 1), (39, 2), (59, 1), (59, 2), (5, 80)]
    got = _points(emu, pos, dep, 90, P5, qq)
    assert got[:6] == [[0] * 5] * 6 and got[6] == [9] * 5 and got[7] == [3] * 5 and got[9] == [0, 0, 0, 9, 9] and got[13] == [0, 0, 0, 2, 2]
    assert got[14] == [0, 0, 0, 9, 9]                        # 40 of its 80 positions have depth 0: the lower median is 0
    for p in range(0, 101):                                  # every percentage on a query of 7 positions with depths 0 0 3 3 3 9 9
        assert _points(emu, [2, 5, 7], [3, 9, 0], 10, (p,), [(0, 7)])[0] == [sorted([0, 0, 3, 3, 3, 9, 9])[qm.rank(p, 7) - 1]]


def test_run_counts_around_the_forms(emu):
    """63, 64 and 65 runs in a query (the register form ends at 64), more than CBC_DEPTH_LINES runs, runs across a tile of change
    points; distinct and tied depths."""
    rng = np.random.default_rng(5)
    n = 3 * LINES + 100
    pos = np.cumsum(rng.integers(1, 9, n)) + 3
    dep = rng.integers(0, 40, n)
    dep[-1] = 0
    slots = int(pos[-1]) + 7
    q = []
    for j0 in (0, 1, 500, LINES - 40, LINES - 1, LINES, 2 * LINES - 64, n - 70):
        for runs in (1, 2, 63, 64, 65, 66, 128, 129):
            if j0 + runs < n:
                q.append((int(pos[j0]), int(pos[j0 + runs] - pos[j0])))                          # exactly `runs` whole runs
                q.append((int(pos[j0]) + (1 if pos[j0 + 1] - pos[j0] > 1 else 0), int(pos[j0 + runs] - pos[j0]) - 1))
    q += [(0, slots), (int(pos[7]), int(pos[LINES + 9] - pos[7])), (int(pos[LINES - 3]), int(pos[2 * LINES + 3] - pos[LINES - 3])),
          (0, int(pos[64])), (0, int(pos[63])), (int(pos[n - 65]), slots - int(pos[n - 65])), (int(pos[n - 64]), slots - int(pos[n - 64]))]
    _points(emu, pos, dep, slots, P8, q)
    _points(emu, pos, dep, slots, (50,), q)
    # ties: hundreds of runs of one depth between runs of another, and of depth 0
    dep2 = np.where(np.arange(n) % 2 == 0, 17, 0)
    dep3 = np.where(np.arange(n) % 3 == 0, 17, 4)
    dep3[-1] = 0
    for d in (dep2, dep3):
        _points(emu, pos, d, slots, P8, q[::3])


def test_rank_on_the_zeros_the_first_and_the_last_depth(emu):
    # 100 positions: 40 zeros (two gaps), 30 of depth 2, 29 of depth 5, 1 of depth 11
    pos, dep = [10, 40, 60, 89, 90, 110], [2, 0, 5, 11, 0, 0]
    q = [(0, 100)]
    for p, want in ((0, 0), (1, 0), (40, 0), (41, 2), (70, 2), (71, 5), (99, 5), (100, 11), (50, 2)):
        assert _points(emu, pos, dep, 120, (p,), q)[0] == [want], p
    assert _points(emu, pos, dep, 120, (0, 40, 41, 70, 71, 99, 100), q)[0] == [0, 0, 2, 2, 5, 5, 11]
    assert _points(emu, pos, dep, 120, (1, 39, 40, 41, 69, 70, 71, 100), q)[0] == [0, 0, 0, 2, 2, 2, 5, 11]    # eight at once
    # the same shape in more than 64 runs: 70 runs of depth 2 and length 1, then zeros, then the deep ones
    pos = list(range(10, 80)) + [80, 100, 129, 130]
    dep = [2] * 70 + [0, 5, 11, 0]
    assert _points(emu, pos, dep, 140, (0, 16, 17, 75, 76, 99, 100), [(0, 140), (10, 120)])[1] == [0, 0, 2, 2, 5, 5, 11]


def test_depths_around_the_table(emu):
    """Depths CBC_QUANT_LDS - 1, CBC_QUANT_LDS, CBC_QUANT_LDS + 1, the rank just below, at and above the tail; both forms."""
    for reps in (1, 30):                                     # 4 runs (register form) and 120 runs (table form)
        pos, dep, at = [], [], 5
        for _ in range(reps):
            for d in (LDS - 1, LDS, 0, LDS + 1):
                pos.append(at); dep.append(d); at += 10
        pos.append(at); dep.append(0)
        n = 40 * reps                                        # positions: a quarter each of 0, LDS - 1, LDS, LDS + 1
        q = [(5, n)]
        assert _points(emu, pos, dep, at + 5, (25, 26, 50, 51, 75, 76, 100), q)[0] == [0, LDS - 1, LDS - 1, LDS, LDS, LDS + 1, LDS + 1]
        assert _points(emu, pos, dep, at + 5, (0, 49, 50, 51, 52, 74, 99), q)[0][1:] == [LDS - 1, LDS - 1, LDS, LDS, LDS, LDS + 1]
        _points(emu, pos, dep, at + 5, P8, [(5, n), (6, n - 2), (0, at + 5), (15, n - 10), (25, 10), (14, 2)])
    # depths near 4 * 10^9 in the tail of the table form and in the register form, one small depth among them
    rng = np.random.default_rng(8)
    for n in (40, 200):
        pos = np.cumsum(rng.integers(1, 50, n)) + 2
        dep = rng.integers(3_900_000_000, 2 ** 32, n)
        dep[n // 2] = 3; dep[n // 3] = 0; dep[-1] = 0; dep[5] = 2 ** 32 - 1
        slots = int(pos[-1]) + 3
        _points(emu, pos, dep, slots, P8, [(0, slots), (int(pos[0]), int(pos[-1] - pos[0])), (int(pos[2]) + 1, int(pos[n - 3] - pos[2])),
                                           (int(pos[5]), 1), (int(pos[n // 2]), int(pos[n // 2 + 1] - pos[n // 2]))])


def test_big_runs_pass_32_bits(emu):
    """Runs near 10^6 slots x 2500: p * len passes 2^32 and the cumulative lengths pass 2^31."""
    pos, dep, slots = cm.carry_points()
    assert slots > 2 ** 31 and 99 * slots > 2 ** 32
    rng = np.random.default_rng(4)
    q = [(0, slots), (0, int(pos[0])), (int(pos[0]), 1), (int(pos[-1]), 5), (int(pos[-1]) - 1, 6), (slots, 0), (int(pos[5]), 0)]
    q += [(int(pos[i]), int(pos[i + 1] - pos[i])) for i in (0, 1023, 1024, 2047, 2048, len(pos) - 2)]
    q += [(int(pos[100]), int(pos[100 + r] - pos[100])) for r in (63, 64, 65)]
    for _ in range(40):
        a = int(rng.integers(0, slots))
        q.append((a, int(rng.integers(0, slots - a + 1))))
    got = _points(emu, pos, dep, slots, P8, q)
    assert got[0][0] == 0 and got[0][-1] >= 4_100_000_000
    small = np.minimum(dep, 700)                             # the same lengths with every depth inside the table
    small[-1] = 0
    _points(emu, pos, small, slots, P5, q)


def test_asan_check_of_the_emulation(built):
    """The stand-alone program (its own main) under AddressSanitizer / UBSan: fabricated cases with every table at its exact size."""
    subprocess.check_call(["make", "-C", EMU_DIR, "asan_check"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(EMU_DIR, "quant_emu_check")], capture_output=True, text=True)
    assert r.returncode == 0 and "QUANT EMU CHECK OK" in r.stdout and "MISMATCH" not in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- datasets through the emulated passes ------------------------------------------------------------------------------------------
def _load(emu, make, **kw):
    fa, sam, pb, contigs = make(**kw)
    iv = dm.assert_models_agree(pb, sam)
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


def _run(emu, d, queries, regions=(), window=0, pcts=P5, exclude=0, depth=None, fail_blocks=()):
    plan, lens = d["plan"], d["lens"]
    qs = plan.queries([r for r, _ in regions], cm.bed(queries, d["names"]) if queries is not None else None, window)
    given = [q for _, q in regions] + [cm.clamp(*q, lens) if q[0] >= 0 else q for q in (queries or [])]
    if queries is None and not regions:
        given = [(c, 0, n) for c, n in enumerate(lens)]
    want = cm.cut(given, window)
    cm.check_queryset(qs, want, d["names"])
    got = qm.emu_quant(emu, plan, d["dec"], qs, pcts, exclude, fail_blocks)
    wq = qm.quant_expected(depth or d["depth"], want, pcts)
    assert got["quant"] == wq, [(q, a, b) for q, a, b in zip(want, got["quant"], wq) if a != b][:5]
    return got, want


def test_query_sets(emu, mixed, ramp):
    """Duplicate, overlapping, touching, empty and unknown lines, on and between change points, more than 64 queries."""
    d, L = mixed, mixed["lens"]
    cps = np.flatnonzero(np.diff(d["depth"].contig(0), prepend=0))
    k = len(cps) // 2
    a, first, last = int(cps[k]), int(cps[0]), int(cps[-1])
    queries = [(0, a, a + 50), (0, a - 30, a), (0, a, a + 1), (0, 0, first), (0, 0, first + 1), (0, last, last + 10), (0, last + 1, L[0]),
               (0, a - 500, a + 300), (0, a - 100, a + 700), (0, a - 500, a + 300), (0, a + 300, a + 400),
               (2, 700, 700), (2, 10 ** 9, 10 ** 9 + 5), (2, L[2] - 5, L[2] + 500), (-1, 5, 900), (1, 0, 1), (0, 0, L[0])]
    got, _ = _run(emu, d, queries, pcts=P8)
    assert got["quant"][7] == got["quant"][9] and got["quant"][11] == got["quant"][12] == got["quant"][14] == [0] * 8
    assert got["quant"][-1][-1] == int(d["depth"].contig(0).max()) and got["quant"][3] == [0] * 8
    rng = np.random.default_rng(31)
    rnd = []
    for _ in range(200):
        c = int(rng.integers(0, 3))
        s = int(rng.integers(0, L[c]))
        rnd.append((c, s, s + int(rng.choice([1, 2, 40, 150, 300, 5000]))))
    _run(emu, d, rnd, pcts=(25, 50, 75))
    _run(emu, d, [(1, 50, 90)], regions=[("chr3:100-200", (2, 99, 200)), ("chr1", (0, 0, L[0])), ("chr3:100-200", (2, 99, 200))])
    got, _ = _run(emu, ramp, [(0, 99_900, 100_300), (0, 99_990, 100_010), (1, 0, 200), (1, 3990, 4100), (0, 0, ramp["lens"][0])], pcts=P8)
    assert max(r[-1] for r in got["quant"]) == 100


def test_whole_contigs_windows_and_excluded_flags(emu, mixed, ramp):
    for d in (mixed, ramp):
        got, _ = _run(emu, d, None, pcts=P8)
        assert max(got["ncp"]) > 64                          # whole contigs: the table form
    _run(emu, mixed, [(0, 1000, 1950), (1, 5, 5), (-1, 0, 250), (2, mixed["lens"][2] - 130, mixed["lens"][2] + 9)], window=100)
    _run(emu, mixed, None, window=977, pcts=(50,))
    _run(emu, mixed, [(0, 30_000, 30_300)], window=1, pcts=(0, 50, 100))
    _run(emu, ramp, None, window=37, pcts=(25, 50, 75))
    _run(emu, mixed, [(0, 0, mixed["lens"][0]), (1, 100, 9000), (0, 500, 640)], pcts=P8, exclude=16, depth=cm.Depth(mixed["iv"], mixed["lens"], 16))


def test_failed_block_contributes_nothing(emu, mixed):
    d = mixed
    queries = [(0, 0, d["lens"][0]), (0, 500, 4000), (1, 0, 3000), (0, 200, 260)]
    qs = d["plan"].queries((), cm.bed(queries, d["names"]))
    blk = int(qs.targets.blocks[1])
    got, want = _run(emu, d, queries, pcts=P8, depth=cm.Depth(d["iv"], d["lens"], 0, (blk,)), fail_blocks=(1,))
    assert got["rcs"] == [-4, 0]                             # CBC_E_BLOCK from the call that held the block
    assert got["quant"] != qm.quant_expected(d["depth"], want, P8)


# ---- the CLI where no device is needed -----------------------------------------------------------------------------------------
def _cli(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def test_cli_refusals_and_zero_lines(built, mixed, tmp_path):
    d = mixed
    (tmp_path / "in.cbc").write_bytes(d["blob"]); (tmp_path / "ref.fa").write_bytes(d["fa"])
    files = (tmp_path / "in.cbc", tmp_path / "o.txt", tmp_path / "ref.fa")
    want = "--quantiles wants 1 to 8 percentages in 0..100, separated by commas and strictly ascending"
    cases = [(("--quantiles", "50"), "--quantiles applies to --bedcov"), (("--depth", "--quantiles", "50"), "--quantiles applies to --bedcov"),
             (("--depth-hist", "--quantiles", "25,75"), "--quantiles applies to --bedcov")]
    cases += [(("--bedcov", "--quantiles", v), want) for v in ("", "x", "1,", ",1", "1,,2", "1;2", "-1", "1.5", "101", "50,50", "50,49", "100,101",
                                                               "0,1,2,3,4,5,6,7,8", "0x10", " 5", "1000", "4294967346")]
    cases += [(("--bedcov", "--quantiles", "50", "--sam"), "different outputs"), (("--bedcov", "--quantiles", "50", "--depth"), "different outputs"),
              (("--bedcov", "--quantiles", "50", "--devices", "0,1"), "one device"), (("--bedcov", "--quantiles", "50", "--min-depth", "0"), "--min-depth wants"),
              (("--bedcov", "--quantiles", "50", "--thresholds", "0"), "--thresholds wants"),
              (("--bedcov", "--quantiles", "50", "--region", "chrX:1-5"), "unknown contig")]
    for args, msg in cases:
        r = _cli("-x", *files, *args)
        assert r.returncode == 1 and msg in r.stderr, (args, r.stderr)
    r = _cli("-c", tmp_path / "in.sam", tmp_path / "o.cbc", tmp_path / "ref.fa", "--bedcov", "--quantiles", "50")
    assert r.returncode == 1 and "--bedcov applies to decompression" in r.stderr, r.stderr
    assert "--quantiles P1,P2,..." in _cli("-h").stdout + _cli("-h").stderr
    # a query list that selects no block: no device is opened, the zero lines carry the new columns; every combination of the
    # three options gives its columns in the order thresholds, quantiles, reads
    first = min(x[1] for x in d["iv"] if x[0] == 0)
    assert first > 3
    (tmp_path / "e.bed").write_bytes(b"chrUn\t1\t5\nchr1\t0\t%d\nchr2\t9\t9\n" % (first - 1))
    qs = [(-1, 1, 5), (0, 0, first - 1), (1, 9, 9)]
    chroms = [b"chrUn", b"chr1", b"chr2"]
    for thr, pct, rd in itertools.product(((), (1, 2, 4294967295)), ((), (50,), P8), (False, True)):
        args = (("--thresholds", ",".join(map(str, thr))) if thr else ()) + (("--quantiles", ",".join(map(str, pct))) if pct else ()) + \
               (("--count-reads",) if rd else ())
        (tmp_path / "o.txt").write_bytes(b"stale")
        r = _cli("-x", *files, "--bedcov", "--regions-file", tmp_path / "e.bed", "--verbose", *args)
        assert r.returncode == 0, r.stderr
        text = qm.text(chroms, qs, [0] * 3, [0] * 3, [[0] * len(thr)] * 3 if thr else None, [[0] * len(pct)] * 3 if pct else None, [0] * 3 if rd else None)
        assert (tmp_path / "o.txt").read_bytes() == text, args
        assert text.count(b"\t") == 3 * (5 + len(thr) + len(pct) + rd)
        assert "kernels:" not in r.stdout and "3 queries" in r.stdout
    r = _cli("-x", *files, "--bedcov", "--regions-file", tmp_path / "e.bed", "--window", "2", "--quantiles", "0,100", "--count-reads")
    assert r.returncode == 0 and (tmp_path / "o.txt").read_bytes().startswith(b"chrUn\t1\t3\t0\t0\t0.00\t0\t0\t0\nchrUn\t3\t5\t0\t0\t0.00\t0\t0\t0\nchr1\t0\t2\t")


def test_model_text_puts_the_columns_in_order():
    assert qm.text([b"c"], [(0, 2, 12)], [25], [7], [[7, 1]], [[0, 3, 9]], [4]) == b"c\t2\t12\t25\t7\t2.50\t7\t1\t0\t3\t9\t4\n"
    assert qm.text([b"c"], [(0, 2, 12)], [25], [7], None, [[3]], None) == b"c\t2\t12\t25\t7\t2.50\t3\n"
    assert qm.rank(0, 9) == 1 and qm.rank(1, 9) == 1 and qm.rank(50, 9) == 5 and qm.rank(100, 9) == 9 and qm.rank(50, 10) == 5 and qm.rank(51, 10) == 6
    assert qm.hist_quantiles([2, 5], [3, 1], 6, (0, 33, 34, 83, 84, 100)) == [0, 0, 2, 2, 5, 5]


def test_exports_name_the_new_entry_points(built):
    from cbc_amd import gpu
    assert {"cbc_gpu_decode_coverage_quant", "cbc_gpu_last_coverage_quant_ms"} <= set(gpu.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "cbc_gpu.h")).read()
    assert "cbc_gpu_decode_coverage_quant(" in hdr and "cbc_gpu_last_coverage_quant_ms(" in hdr and "#define CBC_QUANT_MAX 8u" in hdr
    sig = inspect.signature(gpu.Encoder.decode_coverage_quant)
    assert list(sig.parameters)[1:] == ["plan", "queries", "quantiles", "exclude_flags", "min_depth", "results", "thresholds", "count_reads"]
    assert sig.parameters["quantiles"].default is inspect.Parameter.empty and sig.parameters["thresholds"].default == ()
    old = inspect.signature(gpu.Encoder.decode_coverage)         # the existing call keeps its parameters
    assert list(old.parameters)[1:] == ["plan", "queries", "exclude_flags", "min_depth", "results", "thresholds", "count_reads"]
    assert hasattr(gpu.Encoder, "last_coverage_quant_ms")
