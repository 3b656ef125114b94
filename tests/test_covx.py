"""Per-query read counts and depth thresholds without a GPU: the weights / apply / lookup bodies of
cbc_covx_body.h and the mark pass that notes the pieces' starts on the lock-step wave emulation (tests/covx_emu) behind the
emulated decode, tile and compact passes, and on fabricated change points and start points; the stand-alone sanitizer check of
the emulation; the CLI where no device is needed.  Ground truth is covxmodel.py: brute force over depthmodel.depth_array and over
the read list, compared exactly."""
import os
import subprocess

import numpy as np
import pytest

import covmodel as cm
import covxmodel as cx
import depthmodel as dm
import regionmodel as rm
import synth
import targetsmodel as tm
from cbc_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "covx_emu")
EXE = os.path.join(ROOT, "cbc_amd", "csrc", "cbc")
TILE, LINES = 4096, 1024                                    # CBC_DEPTH_TILE, CBC_DEPTH_LINES
THR3 = (1, 2, 5)


@pytest.fixture(scope="module")
def emu(built):
    subprocess.check_call(["make", "-C", EMU_DIR, "libcbc_covx_emu.so"], stdout=subprocess.DEVNULL)
    return cx.emu_load(os.path.join(EMU_DIR, "libcbc_covx_emu.so"))


def _load(emu, make, **kw):
    fa, sam, pb, contigs = make(**kw)
    iv = dm.assert_models_agree(pb, sam)                    # the packed arrays and POS + CIGAR agree read by read ...
    names, lens = dm.names_lens(None, contigs)
    ivb = dm.intervals_b(sam)
    probe = [(c, s, min(lens[c], s + w)) for c in range(len(lens)) for s in range(0, lens[c], max(1, lens[c] // 7)) for w in (1, 150, 4000)]
    assert cx.reads_expected(cx.Reads(iv), probe) == cx.reads_expected(cx.Reads(ivb), probe)     # ... and count alike
    blob = rm.container(pb)
    plan = host.UnpackPlan(blob, fa)
    d = dict(fa=fa, pb=pb, blob=blob, plan=plan, iv=iv, names=names, lens=lens, depth=cm.Depth(iv, lens), reads=cx.Reads(iv))
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


LONE, EXCL, P70, P1100 = 6000, 5000, 1000, 3000             # POS of the reads of the pile dataset (1-based), every read 100 bases


def _pile():
    """One contig: 70 copies of a read at P70, 1100 copies at P1100, one read with FLAG 1024 at EXCL, one lone read at LONE."""
    rng = np.random.default_rng(23)
    c = synth.make_contig(rng, 20_000)

    def read(pos, flag):
        return dict(pos=pos, flag=flag, cigar="100M", seq=c[pos - 1:pos + 99].tobytes(), md="100", nm=0)
    recs = [read(P70, 0)] * 70 + [read(P1100, 16)] * 1100 + [read(EXCL, 1024), read(LONE, 0)]
    contigs = [("pile", c)]
    fa, sam = synth.fasta_text(contigs), synth.sam_text([("pile", len(c), recs)])
    return fa, sam, host.pack_sam(sam, fa, block_reads=64, var_length=True), contigs


@pytest.fixture(scope="module")
def pile(emu):
    d = _load(emu, _pile)
    yield d
    d["plan"].close(); d["pb"].close()


def _run(emu, d, queries, regions=(), window=0, thr=THR3, count_reads=True, exclude=0, min_depth=1, depth=None, reads=None, fail_blocks=(),
         dec=None):
    """`queries` ((contig or -1, start0, end0), as the BED lines give them) through cbc_unpack_queries and the emulation, every
    column against the model.  Returns (the emulation's dict, the clamped and cut queries)."""
    plan, lens = d["plan"], d["lens"]
    qs = plan.queries([r for r, _ in regions], cm.bed(queries, d["names"]) if queries is not None else None, window)
    given = [q for _, q in regions] + [cm.clamp(*q, lens) if q[0] >= 0 else q for q in (queries or [])]
    if queries is None and not regions:
        given = [(c, 0, n) for c, n in enumerate(lens)]
    want = cm.cut(given, window)
    cm.check_queryset(qs, want, d["names"])
    got = cx.emu_covx(emu, plan, dec or d["dec"], qs, thr, count_reads, exclude, min_depth, fail_blocks)
    dep = depth or d["depth"]
    ws, wc = cm.expected(dep, want, min_depth)
    assert got["sum"] == ws and got["covered"] == wc
    wt = cx.thr_expected(dep, want, thr)
    assert got["thr"] == wt, [(q, a, b) for q, a, b in zip(want, got["thr"], wt) if a != b][:5]
    for row in got["thr"]:
        assert all(a >= b for a, b in zip(row, row[1:]))     # a higher threshold never covers more
    if count_reads:
        wr = cx.reads_expected(reads or d["reads"], want)
        assert got["reads"] == wr, [(q, a, b) for q, a, b in zip(want, got["reads"], wr) if a != b][:5]
    else:
        assert got["reads"] is None
    return got, want


def _change_points(d, c):
    return np.flatnonzero(np.diff(d["depth"].contig(c), prepend=0))


def test_query_sets_of_the_summary(emu, mixed, ramp):
    """The query sets of tests/test_coverage.py: random, on and between change points, touching, overlapping, duplicate, empty,
    unknown, clamped, interleaved over the contigs (more than 64 queries), region strings in front of a file."""
    d, L = mixed, mixed["lens"]
    cps = _change_points(d, 0)
    k = len(cps) // 2
    inside = next(i for i in range(k, len(cps) - 1) if cps[i + 1] - cps[i] >= 5)
    a, b = int(cps[inside]), int(cps[inside + 1])
    first, last = int(cps[0]), int(cps[-1])
    mid = a + 2
    queries = [(0, int(cps[k]), int(cps[k]) + 50), (0, int(cps[k]) - 30, int(cps[k])), (0, a + 1, b - 1), (0, a, b), (0, a + 2, a + 3),
               (0, 0, first), (0, 0, first - 1), (0, 0, first + 1), (0, last, last + 10), (0, last + 1, L[0]), (0, L[0] - 1000, L[0] - 500),
               (0, mid - 40, mid), (0, mid, mid + 40), (0, a - 500, a + 300), (0, a - 100, a + 700), (0, a - 500, a + 300),
               (2, 700, 700), (2, 10 ** 9, 10 ** 9 + 5), (2, L[2] - 5, L[2] + 500), (-1, 5, 900), (1, 0, 1), (0, 0, L[0])]
    got, want = _run(emu, d, queries)
    assert got["reads"][13] == got["reads"][15] > 0 and got["reads"][16:20] == [0, 0, 0, 0] and got["reads"][5] == 0
    assert got["reads"][-1] == d["reads"].kept(0) == got["kept"][0]     # the whole contig: every kept read of the call
    rng = np.random.default_rng(31)
    rnd = []
    for _ in range(200):
        c = int(rng.integers(0, 3))
        s = int(rng.integers(0, L[c]))
        rnd.append((c, s, s + int(rng.choice([1, 2, 40, 150, 300, 5000]))))
    got, _ = _run(emu, d, rnd, thr=(1, 2, 3, 4, 5, 6, 8, 11))          # n_thr 8, more than 64 queries
    assert max(r[-1] for r in got["thr"]) > 0
    inter = [q for t in zip([(0, 100 * i, 100 * i + 150) for i in range(40)], [(1, 90 * i, 90 * i + 10) for i in range(40)],
                            [(2, 70 * i, 70 * i + 200) for i in range(40)]) for q in t]
    _run(emu, d, inter, thr=(3,))                                       # n_thr 1
    _run(emu, d, [(1, 50, 90)], regions=[("chr3:100-200", (2, 99, 200)), ("chr1", (0, 0, L[0])), ("chr3:100-200", (2, 99, 200))])
    _run(emu, ramp, [(0, 99_900, 100_300), (0, 99_990, 100_010), (1, 0, 200), (1, 3990, 4100), (0, 0, ramp["lens"][0])], thr=(1, 10, 99, 100))


def test_whole_contigs_and_windows(emu, mixed, ramp):
    for d in (mixed, ramp):
        got, want = _run(emu, d, None)
        assert got["reads"] == [d["reads"].kept(c) for c in range(len(d["lens"]))] and sum(got["kept"]) == sum(got["reads"])
    # contig 0 of the mixed set whole: more start points than one tile of runs, on both sides of a tile edge of the starts array
    starts = np.unique(mixed["reads"].by[0][:, 0])
    assert got is not None and len(starts) > LINES and (starts < TILE).any() and (starts > TILE).any()
    got, _ = _run(emu, mixed, [(0, 0, mixed["lens"][0])])
    assert got["nsp"] == [len(starts)]                                  # one start point per distinct first slot
    got, want = _run(emu, mixed, [(0, 1000, 1950), (1, 5, 5), (-1, 0, 250), (2, mixed["lens"][2] - 130, mixed["lens"][2] + 9)], window=100)
    assert got["reads"][10:14] == [0, 0, 0, 0]
    got, _ = _run(emu, mixed, [(0, 30_000, 30_300)], window=1, thr=(1, 3))
    assert got["reads"] == [int(x) for x in mixed["depth"].contig(0)[30_000:30_300]]      # one base: the reads on it are its depth
    _run(emu, mixed, None, window=977)
    _run(emu, mixed, [(0, 100, 200)], regions=[("chr2:11-1000", (1, 10, 1000))], window=333)
    a = int(_change_points(mixed, 0)[len(_change_points(mixed, 0)) // 3])
    _run(emu, mixed, [(0, a, a + TILE - 1), (0, a + TILE + 10, a + TILE + 30), (0, a + 2 * TILE, a + 3 * TILE + 7)])


def test_read_edges_clipped_starts_and_gaps(emu, pile):
    """The lone read covers LONE .. LONE + 99 (1-based), that is 0-based [LONE - 1, LONE + 99)."""
    d, s0 = pile, LONE - 1
    q = [(0, s0, s0 + 11),                                   # starts exactly on the read's first base
         (0, s0 + 99, s0 + 111),                             # starts on its last base
         (0, s0 + 300, s0 + 311)]                            # (apart from the others: an interval of its own)
    got, _ = _run(emu, d, q)
    assert got["reads"] == [1, 1, 0]
    got, _ = _run(emu, d, [(0, s0 + 100, s0 + 111)])         # starts one past its last base
    assert got["reads"] == [0] and got["sum"] == [0]
    got, _ = _run(emu, d, [(0, s0 + 50, s0 + 51), (0, s0 + 50, s0 + 50), (0, s0 + 98, s0 + 99), (0, s0 - 1, s0)])     # one base, length 0
    assert got["reads"] == [1, 0, 1, 0]
    # the read reaches into an interval from in front of it: its piece starts on the interval's first slot
    got, _ = _run(emu, d, [(0, s0 + 40, s0 + 60)])
    assert got["reads"] == [1] and got["nsp"] == [1] and got["thr"] == [[20, 0, 0]]
    # one read over two intervals with a gap: once in each, not in the interval behind the gap's neighbour; the same cut in windows
    gap = [(0, s0 + 10, s0 + 20), (0, s0 + 50, s0 + 60), (0, s0 + 150, s0 + 160)]
    got, _ = _run(emu, d, gap)
    assert got["reads"] == [1, 1, 0] and d["plan"].queries((), cm.bed(gap, d["names"])).targets.n_iv == 3
    got, _ = _run(emu, d, gap, window=5)
    assert got["reads"] == [1, 1, 1, 1, 0, 0]                # two windows of one target: the read counts in both
    # overlapping targets merged into one interval, touching ones too: a read in both queries counts in both
    got, _ = _run(emu, d, [(0, s0 - 20, s0 + 5), (0, s0 + 3, s0 + 200), (0, s0 + 200, s0 + 400)])
    assert got["reads"] == [1, 1, 0]


def test_pile_ups_on_one_slot(emu, pile):
    d = pile
    q = [(0, P70 - 1, P70 + 99), (0, P70 + 98, P70 + 99), (0, P70 + 99, P70 + 150), (0, P70 - 50, P70 - 1),
         (0, P1100 - 1, P1100), (0, P1100 + 50, P1100 + 300), (0, P1100 - 10, P1100 - 1), (0, 0, d["lens"][0])]
    got, _ = _run(emu, d, q, thr=(1, 70, 71, 1100, 1101))
    assert got["reads"] == [70, 70, 0, 0, 1100, 1100, 0, 1172]
    assert got["thr"][0] == [100, 100, 0, 0, 0] and got["thr"][4] == [1, 1, 1, 1, 0]
    assert got["thr"][-1] == [400, 200, 100, 100, 0]         # a threshold above the deepest depth: zeros
    # excluded flags: the FLAG-1024 read and the 1100 reverse-strand copies drop out
    for ex, kept in ((1024, 1171), (16, 72), (1040, 71)):
        got, _ = _run(emu, d, q + [(0, EXCL - 1, EXCL + 10)], exclude=ex, depth=cm.Depth(d["iv"], d["lens"], ex), reads=cx.Reads(d["iv"], ex))
        assert got["reads"][-2] == kept and got["reads"][-1] == (0 if ex & 1024 else 1) and got["kept"] == [kept]


def test_span_zero_read(emu, pile):
    """The decoder's record of the lone read with its span set to 0: kept by nobody."""
    d = pile
    dec = dict(d["dec"], recs=d["dec"]["recs"].copy())
    i = len(d["iv"]) - 1
    assert d["iv"][i][1] == LONE and int(dec["recs"][i]["tok_off"]) == 100
    dec["recs"][i]["tok_off"] = 0
    iv = list(d["iv"])
    iv[i] = (iv[i][0], iv[i][1], 0) + tuple(iv[i][3:])
    got, _ = _run(emu, d, [(0, LONE - 1, LONE + 50), (0, 0, d["lens"][0])], dec=dec, depth=cm.Depth(iv, d["lens"]), reads=cx.Reads(iv))
    assert got["reads"] == [0, 1171]


def test_threshold_columns(emu, mixed, ramp):
    d = ramp
    top = int(max(d["depth"].contig(0).max(), d["depth"].contig(1).max()))
    assert top == 100
    queries = [(0, 99_900, 100_300), (0, 99_990, 100_010), (1, 0, 200), (1, 3990, 4100), (0, 0, d["lens"][0])]
    got, _ = _run(emu, d, queries, thr=(top + 1,))
    assert got["thr"] == [[0]] * len(queries) and got["sum"][0] > 0            # above the deepest depth: all zeros
    got, _ = _run(emu, d, queries, thr=(top, 2 ** 32 - 1))
    assert got["thr"][0][0] > 0 and all(r[1] == 0 for r in got["thr"])
    for md in (1, 7, top):                                                       # a threshold equal to --min-depth: the covered column
        got, _ = _run(emu, d, queries, thr=(md, md + 1) if md < top else (1, md), min_depth=md)
        assert [r[0 if md < top else 1] for r in got["thr"]] == got["covered"]
    got, _ = _run(emu, mixed, [(0, 0, mixed["lens"][0]), (1, 100, 9000)], thr=(2, 3), exclude=16, min_depth=3,
                  depth=cm.Depth(mixed["iv"], mixed["lens"], 16), reads=cx.Reads(mixed["iv"], 16))
    assert [r[1] for r in got["thr"]] == got["covered"]


def test_only_one_of_the_two_and_neither(emu, mixed):
    """thresholds alone, read counts alone; with neither only sum and covered come back, those of the plain call's emulation."""
    d = mixed
    queries = [(0, 0, d["lens"][0]), (0, 500, 4000), (1, 0, 3000), (0, 200, 260), (2, 5, 5)]
    _run(emu, d, queries, thr=THR3, count_reads=False)
    _run(emu, d, queries, thr=())
    got, want = _run(emu, d, queries, thr=(), count_reads=False)
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cov_emu"), "libcbc_cov_emu.so"], stdout=subprocess.DEVNULL)
    old = cm.emu_load(os.path.join(ROOT, "tests", "cov_emu", "libcbc_cov_emu.so"))
    s, c, rcs, _ = cm.emu_cov(old, d["plan"], d["dec"], d["plan"].queries((), cm.bed(queries, d["names"])))
    assert (got["sum"], got["covered"], got["rcs"]) == (s, c, rcs) and got["thr"] == [[]] * len(queries)


def test_failed_block_contributes_nothing(emu, mixed):
    d = mixed
    queries = [(0, 0, d["lens"][0]), (0, 500, 4000), (1, 0, 3000), (0, 200, 260)]
    qs = d["plan"].queries((), cm.bed(queries, d["names"]))
    k = 1
    blk = int(qs.targets.blocks[k])
    got, want = _run(emu, d, queries, depth=cm.Depth(d["iv"], d["lens"], 0, (blk,)), reads=cx.Reads(d["iv"], 0, (blk,)), fail_blocks=(k,))
    assert got["rcs"] == [-4, 0]                             # CBC_E_BLOCK from the call that held the block
    assert got["reads"] != cx.reads_expected(d["reads"], want)


def test_fabricated_points(emu):
    """Change points and start points fed straight to the bodies, against Python integers."""
    pos, dep, slots = cm.carry_points()                      # runs near 10^6 slots x 2500, depths near 4 * 10^9
    rng = np.random.default_rng(4)
    sp = np.sort(rng.choice(np.arange(17, slots - 5), 3000, replace=False))
    inc = rng.integers(1_000_000, 2_000_000, len(sp))
    sc = np.cumsum(inc) % 2 ** 32                            # the cumulative count passes 2^31 and wraps 2^32
    assert int(np.cumsum(inc)[-1]) > 2 ** 32 and len(sp) > 2 * LINES
    q = [(0, slots), (0, int(pos[0])), (int(pos[0]), 1), (int(pos[-1]), 5), (int(pos[-1]) - 1, 6), (slots, 0), (int(pos[5]), 0)]
    q += [(int(pos[i]), int(pos[i + 1] - pos[i])) for i in (0, 1023, 1024, 2047, 2048, len(pos) - 2)]
    q += [(int(sp[i]), 1) for i in (0, 1, 1023, 1024, 2999)] + [(int(sp[i]) - 1, 2) for i in (0, 1024)] + [(int(sp[7]) + 1, int(sp[9] - sp[7]))]
    for _ in range(80):
        a = int(rng.integers(0, slots))
        q.append((a, int(rng.integers(0, slots - a + 1))))
    for thr in ((1, 2 ** 32 - 1), (1, 2, 3_900_000_000, 4_000_000_000, 4_100_000_000, 4_199_999_999, 4_200_000_000, 2 ** 32 - 1)):
        got = cx.emu_points(emu, pos, dep, sp, sc, slots, thr, q)
        want = cx.points_expected(pos, dep, sp, sc, thr, q)
        assert got == want, thr
    assert got[0][0][0] > 2 ** 31 and all(r[-1] == 0 for r in got[0])
    # ncp 0, 1 and 2, and no start point at all
    qq = [(0, 100), (5, 0), (9, 1), (8, 1), (48, 1), (49, 1)]
    assert cx.emu_points(emu, [], [], [], [], 100, (1, 6), qq) == ([[0, 0]] * 6, [0] * 6)
    assert cx.emu_points(emu, [49], [0], [], [], 100, (1,), qq) == ([[0]] * 6, [0] * 6)
    got = cx.emu_points(emu, [9, 49], [6, 0], [], [], 100, (1, 6, 7), qq)
    assert got == cx.points_expected([9, 49], [6, 0], [], [], (1, 6, 7), qq) and got[0][0] == [40, 40, 0] and got[1] == [0, 0, 6, 0, 6, 0]
    got = cx.emu_points(emu, [9, 49], [6, 0], [9], [6], 100, (6,), qq)
    assert got == cx.points_expected([9, 49], [6, 0], [9], [6], (6,), qq) and got[1] == [6, 0, 6, 0, 6, 0]
    got = cx.emu_points(emu, pos, dep, [], [], slots, (), q[:20])
    assert got == cx.points_expected(pos, dep, [], [], (), q[:20])


def test_asan_check_of_the_emulation(built):
    """The stand-alone program (its own main) under AddressSanitizer / UBSan: fabricated cases with every table at its exact size."""
    subprocess.check_call(["make", "-C", EMU_DIR, "asan_check"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(EMU_DIR, "covx_emu_check")], capture_output=True, text=True)
    assert r.returncode == 0 and "COVX EMU CHECK OK" in r.stdout and "MISMATCH" not in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- the CLI where no device is needed -----------------------------------------------------------------------------------------
def _cli(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def test_cli_refusals_and_zero_lines(built, mixed, tmp_path):
    d = mixed
    (tmp_path / "in.cbc").write_bytes(d["blob"]); (tmp_path / "ref.fa").write_bytes(d["fa"])
    files = (tmp_path / "in.cbc", tmp_path / "o.txt", tmp_path / "ref.fa")
    want = "--thresholds wants 1 to 8 depths"
    for args, msg in [(("--count-reads",), "--count-reads applies to --bedcov"), (("--thresholds", "1,2"), "--thresholds applies to --bedcov"),
                      (("--depth", "--count-reads"), "--count-reads applies to --bedcov"),
                      (("--depth-hist", "--thresholds", "5"), "--thresholds applies to --bedcov"),
                      (("--bedcov", "--thresholds", ""), want), (("--bedcov", "--thresholds", "x"), want),
                      (("--bedcov", "--thresholds", "1,"), want), (("--bedcov", "--thresholds", ",1"), want),
                      (("--bedcov", "--thresholds", "1,,2"), want), (("--bedcov", "--thresholds", "1;2"), want),
                      (("--bedcov", "--thresholds", "-1"), want), (("--bedcov", "--thresholds", "1.5"), want),
                      (("--bedcov", "--thresholds", "0"), want), (("--bedcov", "--thresholds", "1,0"), want),
                      (("--bedcov", "--thresholds", "5,5"), want), (("--bedcov", "--thresholds", "5,4"), want),
                      (("--bedcov", "--thresholds", "4294967296"), want), (("--bedcov", "--thresholds", "1,2,3,4,5,6,7,8,9"), want),
                      (("--bedcov", "--count-reads", "--sam"), "different outputs"), (("--bedcov", "--thresholds", "3", "--depth"), "different outputs"),
                      (("--bedcov", "--count-reads", "--devices", "0,1"), "one device"),
                      (("--bedcov", "--count-reads", "--min-depth", "0"), "--min-depth wants"),
                      (("--bedcov", "--thresholds", "1", "--region", "chrX:1-5"), "unknown contig")]:
        r = _cli("-x", *files, *args)
        assert r.returncode == 1 and msg in r.stderr, (args, r.stderr)
    r = _cli("-c", tmp_path / "in.sam", tmp_path / "o.cbc", tmp_path / "ref.fa", "--bedcov", "--count-reads")
    assert r.returncode == 1 and "--bedcov applies to decompression" in r.stderr, r.stderr
    fa, sam, _, _ = synth.dataset(4, [5000], [100], 100)
    (tmp_path / "c.cbc").write_bytes(host_compat(sam, fa)); (tmp_path / "c.fa").write_bytes(fa)
    r = _cli("-x", tmp_path / "c.cbc", tmp_path / "o.txt", tmp_path / "c.fa", "--bedcov", "--count-reads")
    assert r.returncode == 1 and "single-stream (--compat) file" in r.stderr, r.stderr
    # a query list that selects no block: no device is opened, the zero lines carry the extra columns, in their order
    first = min(x[1] for x in d["iv"] if x[0] == 0)
    assert first > 3
    (tmp_path / "e.bed").write_bytes(b"chrUn\t1\t5\nchr1\t0\t%d\nchr2\t9\t9\n" % (first - 1))
    lines = [b"chrUn\t1\t5\t0\t0\t0.00", b"chr1\t0\t%d\t0\t0\t0.00" % (first - 1), b"chr2\t9\t9\t0\t0\t0.00"]
    for args, extra in [(("--thresholds", "1,2,4294967295", "--count-reads"), 4), (("--count-reads",), 1), (("--thresholds", "10,20,30,40,50,60,70,80"), 8),
                        ((), 0)]:
        (tmp_path / "o.txt").write_bytes(b"stale")
        r = _cli("-x", *files, "--bedcov", "--regions-file", tmp_path / "e.bed", "--verbose", *args)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / "o.txt").read_bytes() == b"".join(ln + b"\t0" * extra + b"\n" for ln in lines), args
        assert "kernels:" not in r.stdout and "3 queries" in r.stdout
    r = _cli("-x", *files, "--bedcov", "--regions-file", tmp_path / "e.bed", "--window", "2", "--thresholds", "3", "--count-reads")
    assert r.returncode == 0 and (tmp_path / "o.txt").read_bytes().startswith(b"chrUn\t1\t3\t0\t0\t0.00\t0\t0\nchrUn\t3\t5\t0\t0\t0.00\t0\t0\nchr1\t0\t2\t")


def host_compat(sam, fa):
    from oracle import oracle
    return oracle.encode(sam, fa)


def test_exports_name_the_new_entry_points(built):
    from cbc_amd import gpu
    assert {"cbc_gpu_decode_coverage_ext", "cbc_gpu_last_coverage_ext_ms"} <= set(gpu.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "cbc_gpu.h")).read()
    assert "cbc_gpu_decode_coverage_ext(" in hdr and "cbc_gpu_last_coverage_ext_ms(" in hdr
    import inspect
    sig = inspect.signature(gpu.Encoder.decode_coverage)
    assert list(sig.parameters)[1:] == ["plan", "queries", "exclude_flags", "min_depth", "results", "thresholds", "count_reads"]
    assert sig.parameters["thresholds"].default == () and sig.parameters["count_reads"].default is False
    assert hasattr(gpu.Encoder, "last_coverage_ext_ms")
