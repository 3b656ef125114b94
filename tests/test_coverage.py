"""Per-target coverage summary without a GPU: cbc_unpack_queries (the unmerged query list, the
windows, the slots, the refusals), the weights / apply / lookup bodies of cbc_cov_body.h on the lock-step wave emulation
(tests/cov_emu) behind the emulated decode and depth passes and on fabricated change points with 64-bit carries, also under
ASan / UBSan, the mean rule through the CLI's formatter, and the CLI where no device is needed.  Ground truth is covmodel.py:
brute force over depthmodel.depth_array, compared exactly."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import covmodel as cm
import depthmodel as dm
import regionmodel as rm
import synth
import targetsmodel as tm
from cbc_amd import host
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "cov_emu")
EXE = os.path.join(ROOT, "cbc_amd", "csrc", "cbc")
TILE, LINES = 4096, 1024                                    # CBC_DEPTH_TILE, CBC_DEPTH_LINES


@pytest.fixture(scope="module")
def emu(built):
    subprocess.check_call(["make", "-C", EMU_DIR, "libcbc_cov_emu.so"], stdout=subprocess.DEVNULL)
    return cm.emu_load(os.path.join(EMU_DIR, "libcbc_cov_emu.so"))


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


def _run(emu, d, queries, regions=(), window=0, exclude=0, min_depth=1, depth=None, fail_blocks=()):
    """`queries` ((contig or -1, start0, end0), as the BED lines give them) through cbc_unpack_queries and the emulation,
    against the model; regions: region strings in front of them, given as (string, (contig, start0, end0))."""
    plan, lens = d["plan"], d["lens"]
    qs = plan.queries([r for r, _ in regions], cm.bed(queries, d["names"]) if queries is not None else None, window)
    given = [q for _, q in regions] + [cm.clamp(*q, lens) if q[0] >= 0 else q for q in (queries or [])]
    if queries is None and not regions:
        given = [(c, 0, n) for c, n in enumerate(lens)]      # no input: every contig as a whole
    want = cm.cut(given, window)
    cm.check_queryset(qs, want, d["names"])
    s, c, rcs, slots = cm.emu_cov(emu, plan, d["dec"], qs, exclude, min_depth, fail_blocks)
    ws, wc = cm.expected(depth or d["depth"], want, min_depth)
    assert s == ws and c == wc, [(q, a, b, x, y) for q, a, b, x, y in zip(want, s, ws, c, wc) if (a, x) != (b, y)][:5]
    return qs, want, s, c, rcs, slots


def _change_points(d, c):
    """0-based positions of contig c where the depth changes (the starts of the runs)."""
    return np.flatnonzero(np.diff(d["depth"].contig(c), prepend=0))


def test_query_edges_on_and_between_change_points(emu, mixed):
    d, L = mixed, mixed["lens"]
    cps = _change_points(d, 0)
    assert len(cps) > LINES                                  # more than one tile of runs in the whole-contig case below
    k = len(cps) // 2
    inside = next(i for i in range(k, len(cps) - 1) if cps[i + 1] - cps[i] >= 5)          # a run of 5 bases or more
    a, b = int(cps[inside]), int(cps[inside + 1])
    first, last = int(cps[0]), int(cps[-1])
    assert first > 2 and last < L[0] - 1500
    mid = a + 2                                              # a seam strictly inside a run
    assert mid not in cps
    queries = [(0, int(cps[k]), int(cps[k]) + 50), (0, int(cps[k]) - 30, int(cps[k])),     # starts / ends on a change point
               (0, a + 1, b - 1), (0, a, b), (0, a + 2, a + 3),                            # inside one run; the run itself; 1 base
               (0, 0, first), (0, 0, first - 1), (0, 0, first + 1),                        # in front of the first change point
               (0, last, last + 10), (0, last + 1, L[0]), (0, L[0] - 1000, L[0] - 500),    # behind the last one: depth 0
               (0, mid - 40, mid), (0, mid, mid + 40),                                     # two touching lines: one interval
               (0, a - 500, a + 300), (0, a - 100, a + 700), (0, a - 500, a + 300),        # overlapping, duplicate
               (2, 700, 700), (2, 10 ** 9, 10 ** 9 + 5), (2, L[2] - 5, L[2] + 500),        # empty; past the end; clamped
               (-1, 5, 900), (1, 0, 1), (0, 0, L[0])]
    qs, want, s, c, rcs, _ = _run(emu, d, queries)
    assert qs.targets.bed_unselected == 3 and rcs and all(r == 0 for r in rcs)
    assert (0, mid - 39, mid + 40) in qs.targets.intervals() or any(i[0] == 0 and i[1] <= mid - 39 and i[2] >= mid + 40 for i in qs.targets.intervals())
    assert s[11] > 0 and s[12] > 0 and s[10] == 0 and s[16:20] == [0, 0, 0, 0] and c[9] == 0
    assert s[13] == s[15] and s[-1] == sum(s for s in cm.expected(d["depth"], [(0, 0, L[0])])[0])
    # the same lines interleaved over the contigs: the output keeps the input's order
    inter = [q for t in zip([(0, 100 * i, 100 * i + 150) for i in range(40)], [(1, 90 * i, 90 * i + 10) for i in range(40)],
                            [(2, 70 * i, 70 * i + 200) for i in range(40)]) for q in t]
    qs, want, s, c, _, _ = _run(emu, d, inter)
    assert qs.contig.tolist()[:6] == [0, 1, 2, 0, 1, 2] and qs.n_q == 120 > 64
    # region strings come first, then the file's lines
    _run(emu, d, [(1, 50, 90)], regions=[("chr3:100-200", (2, 99, 200)), ("chr1", (0, 0, L[0])), ("chr3:100-200", (2, 99, 200))])


def test_no_input_is_one_query_per_contig(emu, mixed, ramp):
    for d in (mixed, ramp):
        L = d["lens"]
        qs, want, s, c, rcs, slots = _run(emu, d, None)
        assert want == [(i, 0, L[i]) for i in range(len(L))] and slots == sum(L) + len(L)
        assert max(L) + 1 > TILE                             # the compressed array crosses a tile of the difference array
        assert all(x > 0 for x in s)


def test_tile_boundary_of_the_compressed_array(emu, mixed):
    """An interval set whose slots cross CBC_DEPTH_TILE inside an interval and exactly at an interval's spare slot."""
    d = mixed
    cps = _change_points(d, 0)
    a = int(cps[len(cps) // 3])
    queries = [(0, a, a + TILE - 1),                         # slots 0 .. TILE - 2, spare TILE - 1: the next interval starts a tile
               (0, a + TILE + 10, a + TILE + 30), (0, a + 2 * TILE, a + 3 * TILE + 7)]
    qs, *_ = _run(emu, d, queries)
    assert qs.q["slot"].tolist() == [0, TILE, TILE + 21]


def test_windows(emu, mixed):
    d, L = mixed, mixed["lens"]
    qs, want, s, c, _, _ = _run(emu, d, [(0, 1000, 1950), (1, 5, 5), (-1, 0, 250), (2, L[2] - 130, L[2] + 9)], window=100)
    assert [e - b for _, b, e in want[:10]] == [100] * 9 + [50] and want[10] == (1, 5, 5)     # the last window is short
    assert want[11:14] == [(-1, 0, 100), (-1, 100, 200), (-1, 200, 250)] and want[14:] == [(2, L[2] - 130, L[2] - 30), (2, L[2] - 30, L[2])]
    qs, want, s, c, _, _ = _run(emu, d, [(0, 30_000, 30_300)], window=1)
    assert qs.n_q == 300 and s == [int(x) for x in d["depth"].contig(0)[30_000:30_300]]
    _run(emu, d, None, window=977)
    _run(emu, d, [(0, 100, 200)], regions=[("chr2:11-1000", (1, 10, 1000))], window=333)


def test_query_limit(mixed):
    plan = mixed["plan"]
    with pytest.raises(host.CbcInputError, match="more than 2\\^24 coverage queries after cutting"):
        plan.queries((), b"chrUn\t0\t100000000\n", 1)
    with pytest.raises(host.CbcInputError, match="more than 2\\^24 coverage queries"):
        plan.queries(["chr1"], b"chr1\t0\t60000\n" * 300, 1)
    assert plan.queries((), b"chrUn\t0\t16777216\n", 64).n_q == 1 << 18     # the limit counts windows, not bases
    with pytest.raises(host.CbcInputError, match="unknown contig"):
        plan.queries(["chrUn:1-5"])
    with pytest.raises(host.CbcInputError, match="BED line 2: start is past end"):
        plan.queries((), b"chr1\t1\t5\nchr1\t9\t5\n")
    assert plan.queries((), b"").n_q == 0 and plan.queries((), b"#x\n\n").n_q == 0


def test_min_depth_and_exclude(emu, mixed, ramp):
    d = ramp
    L = d["lens"]
    top = int(max(d["depth"].contig(0).max(), d["depth"].contig(1).max()))
    assert top == 100
    queries = [(0, 99_900, 100_300), (0, 99_990, 100_010), (1, 0, 200), (1, 3990, 4100), (0, 0, L[0])]
    for md in (1, 2, 10, top, top + 1, 2 ** 32 - 1):
        qs, want, s, c, _, _ = _run(emu, d, queries, min_depth=md)
        if md > top:
            assert c == [0] * len(queries) and s[0] > 0
    for ex in (16, 1024, 1040):                              # the ramp alternates FLAG 16 and 1040
        dep = cm.Depth(d["iv"], L, ex)
        qs, want, s, c, _, _ = _run(emu, d, queries, exclude=ex, min_depth=2, depth=dep)
        assert (s[0] == 0) == bool(ex & 16)
    _run(emu, mixed, [(0, 0, mixed["lens"][0]), (1, 100, 9000)], exclude=16, min_depth=3, depth=cm.Depth(mixed["iv"], mixed["lens"], 16))


def test_sixty_four_bit_carries(emu):
    """Change points fed straight to the four bodies: every weight, every tile total and every prefix passes 2^32."""
    pos, dep, slots = cm.carry_points()
    assert len(pos) > 2 * LINES and int(dep[0]) * int(pos[1] - pos[0]) > 2 ** 50
    rng = np.random.default_rng(4)
    q = [(0, slots), (0, int(pos[0])), (int(pos[0]), 1), (int(pos[-1]), 5), (int(pos[-1]) - 1, 6), (slots, 0), (int(pos[5]), 0)]
    q += [(int(pos[i]), int(pos[i + 1] - pos[i])) for i in (0, 1023, 1024, 2047, 2048, len(pos) - 2)]        # whole runs at the tile seams
    q += [(int(pos[1000]) + 7, int(pos[1100] - pos[1000])), (int(pos[len(pos) // 2]) - 3, 20), (int(pos[len(pos) // 3]) - 3, 20)]
    for _ in range(120):
        a = int(rng.integers(0, slots))
        q.append((a, int(rng.integers(0, slots - a + 1))))
    for md in (1, 2, 4_000_000_000):
        got = cm.emu_points(emu, pos, dep, slots, q, md)
        assert got == cm.points_expected(pos, dep, q, md), md
    assert got[0][0] > 2 ** 63 // 2 and max(got[0]) < 2 ** 64
    # no change point at all, and a single one
    assert cm.emu_points(emu, [], [], 100, [(0, 100), (5, 0)]) == ([0, 0], [0, 0])
    assert cm.emu_points(emu, [7], [0], 100, [(0, 100)]) == ([0], [0])


def test_failed_block_contributes_nothing(emu, mixed):
    d = mixed
    queries = [(0, 0, d["lens"][0]), (0, 500, 4000), (1, 0, 3000), (0, 200, 260)]
    qs = d["plan"].queries((), cm.bed(queries, d["names"]))
    k = 1
    blk = int(qs.targets.blocks[k])
    dep = cm.Depth(d["iv"], d["lens"], 0, (blk,))
    qs, want, s, c, rcs, _ = _run(emu, d, queries, depth=dep, fail_blocks=(k,))
    assert rcs == [-4, 0]                                    # CBC_E_BLOCK from the call that held the block
    assert s != cm.expected(d["depth"], want)[0]


def test_mean_rule_through_the_formatter(built):
    for total, length, want in [(7, 3, b"2.33"), (5, 2, b"2.50"), (1, 8, b"0.13"), (0, 0, b"0.00"), (9, 0, b"0.00"), (0, 5, b"0.00"),
                                (199, 200, b"1.00"), (1, 200, b"0.01"), (1, 201, b"0.00"), (2 ** 63, 2 ** 31 - 1, None),
                                (4294967295 * 2147483647, 2147483647, b"4294967295.00"), (12345678901234, 1000, b"12345678901.23")]:
        got = host.coverage_mean(total, length)
        assert got == cm.mean_text(total, length) and (want is None or got == want), (total, length, got)


def test_asan_build_of_the_emulation(built):
    subprocess.check_call(["make", "-C", EMU_DIR, "asan"], stdout=subprocess.DEVNULL)
    code = textwrap.dedent("""
        import sys
        sys.path[:0] = [%r, %r]
        import covmodel as cm
        L = cm.emu_load(%r)
        assert cm.selfcheck(L)
        print("COV EMU OK")
    """ % (ROOT, os.path.join(ROOT, "tests"), os.path.join(EMU_DIR, "libcbc_cov_emu_asan.so")))
    env = dict(os.environ, LD_PRELOAD=subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip(),
               ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and "COV EMU OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_hostile_queries_under_asan(built, mixed, tmp_path):
    """cbc_unpack_queries on the AddressSanitizer build of libcbc_host: BED text that ends inside a field, unknown contigs whose
    names end the buffer, windows over empty and clamped lines; every buffer exactly as long as the text."""
    csrc = os.path.join(ROOT, "cbc_amd", "csrc")
    subprocess.check_call(["make", "-C", csrc, "libcbc_host_asan.so"], stdout=subprocess.DEVNULL)
    (tmp_path / "in.cbc").write_bytes(mixed["blob"]); (tmp_path / "ref.fa").write_bytes(mixed["fa"])
    code = textwrap.dedent("""
        import sys
        sys.path.insert(0, %r)
        from cbc_amd import host
        host.HOST_LIB = %r
        p = host.UnpackPlan(open(%r, "rb").read(), open(%r, "rb").read())
        good = b"chr1\\t10\\t20\\nchrUn 5 9\\r\\nchr2\\t7\\t7\\n"
        n = 0
        for c in [b"chr1\\t1\\t5", b"zz\\t1\\t5", b"chr3\\t0\\t999999999999", b"chr1\\t99999999\\t999999999", b"q\\t1", b"chr1\\t5\\t5\\r"]:
            for text in (c, good + c, c + b"\\n" + good):
                for cut in (len(text), len(text) - 1):
                    for w in (0, 1, 7):
                        try:
                            qs = p.queries([b"chr2:5-50"], text[:cut], w)
                            assert qs.n_q >= 1 and [qs.chrom(i) for i in range(qs.n_q)]
                            n += 1
                        except host.CbcInputError as e:
                            assert "BED line" in str(e), e
        assert p.queries(window=5000).n_q > 3
        print("QUERIES OK", n)
    """ % (ROOT, os.path.join(csrc, "libcbc_host_asan.so"), str(tmp_path / "in.cbc"), str(tmp_path / "ref.fa")))
    env = dict(os.environ, LD_PRELOAD=subprocess.check_output(["gcc", "-print-file-name=libasan.so"], text=True).strip(),
               ASAN_OPTIONS="detect_leaks=0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and "QUERIES OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- the CLI where no device is needed -----------------------------------------------------------------------------------------
def _cli(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def test_cli_refusals_and_empty_selection(built, mixed, tmp_path):
    d = mixed
    (tmp_path / "in.cbc").write_bytes(d["blob"]); (tmp_path / "ref.fa").write_bytes(d["fa"])
    (tmp_path / "t.bed").write_bytes(b"chr1\t10\t20\n")
    files = (tmp_path / "in.cbc", tmp_path / "o.txt", tmp_path / "ref.fa")
    for args, msg in [(("--bedcov", "--sam"), "different outputs"), (("--bedcov", "--depth"), "different outputs"),
                      (("--bedcov", "--devices", "0,1"), "one device"), (("--window", "100"), "--window applies to --bedcov"),
                      (("--min-depth", "2"), "--min-depth applies to --bedcov"), (("--depth", "--window", "5"), "--window applies to --bedcov"),
                      (("--bedcov", "--window", "0"), "--window wants"), (("--bedcov", "--window", "x"), "--window wants"),
                      (("--bedcov", "--min-depth", "0"), "--min-depth wants"), (("--bedcov", "--region", "chrX:1-5"), "unknown contig"),
                      (("--bedcov", "--regions-file", tmp_path / "none.bed"), "cannot open")]:
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
    b = bytearray(d["blob"]); b[36 + 2] = 9                                   # a tab inside "chr1": what cbc_unpack_sam_header refuses
    (tmp_path / "t.cbc").write_bytes(bytes(b))
    r = _cli("-x", tmp_path / "t.cbc", tmp_path / "o.txt", tmp_path / "ref.fa", "--bedcov", "--region", "chr2:1-5")
    assert r.returncode == 1 and "holds a tab or a newline" in r.stderr, r.stderr
    # a query list that selects no block: no device is opened, the all-zero lines are written, status 0
    first = min(x[1] for x in d["iv"] if x[0] == 0)
    assert first > 3
    (tmp_path / "e.bed").write_bytes(b"chrUn\t1\t5\nchr1\t0\t%d\nchr2\t9\t9\nchr3\t999999\t9999999\n" % (first - 1))
    (tmp_path / "o.txt").write_bytes(b"stale")
    r = _cli("-x", *files, "--bedcov", "--regions-file", tmp_path / "e.bed", "--verbose")
    assert r.returncode == 0, r.stderr
    L3 = d["lens"][2]
    assert (tmp_path / "o.txt").read_bytes() == (b"chrUn\t1\t5\t0\t0\t0.00\nchr1\t0\t%d\t0\t0\t0.00\nchr2\t9\t9\t0\t0\t0.00\n"
                                                 b"chr3\t%d\t%d\t0\t0\t0.00\n" % (first - 1, L3, L3))
    assert "kernels:" not in r.stdout and "4 queries" in r.stdout and "3 BED lines selected nothing" in r.stdout
    r = _cli("-x", *files, "--bedcov", "--regions-file", tmp_path / "e.bed", "--window", "2", "--min-depth", "3")
    assert r.returncode == 0 and (tmp_path / "o.txt").read_bytes().startswith(b"chrUn\t1\t3\t0\t0\t0.00\nchrUn\t3\t5\t0\t0\t0.00\nchr1\t0\t2\t")


def test_exports_name_the_coverage_entry_points(built):
    from cbc_amd import gpu
    assert {"cbc_gpu_decode_coverage", "cbc_gpu_last_coverage_ms"} <= set(gpu.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "cbc_gpu.h")).read()
    assert "cbc_gpu_decode_coverage(" in hdr and "cbc_gpu_last_coverage_ms(" in hdr
    hdr = open(os.path.join(ROOT, "include", "cbc_host.h")).read()
    assert "cbc_unpack_queries(" in hdr and "cbc_queries_free(" in hdr
    for f in ("cbc_unpack_queries", "cbc_queries_free", "cbc_coverage_mean"):
        getattr(host.lib(), f)
