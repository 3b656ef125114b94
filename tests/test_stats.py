"""Read statistics without a GPU: the zero / accumulate / flush bodies of cbc_stats_body.h on the
lock-step wave emulation (tests/stats_emu) behind the emulated decode, on the fabricated shapes (statsmodel.shapes) and on the
mixed dataset of the other tests; the stand-alone sanitizer program; the formatter's text against the model's text; and the CLI
where no device is needed.  Ground truth is statsmodel.py: two derivations of the reads that must agree, counted by brute force
and compared exactly."""
import os
import subprocess

import numpy as np
import pytest

import depthmodel as dm
import regionmodel as rm
import statsmodel as sm
import synth
import targetsmodel as tm
from cbc_amd import host
from oracle import oracle
from test_region import _dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "stats_emu")
EXE = os.path.join(ROOT, "cbc_amd", "csrc", "cbc")


@pytest.fixture(scope="module")
def emu(built):
    subprocess.check_call(["make", "-C", EMU_DIR, "libcbc_stats_emu.so"], stdout=subprocess.DEVNULL)
    return sm.emu_load(os.path.join(EMU_DIR, "libcbc_stats_emu.so"))


def _wrap(emu, fa, pb, reads, names):
    blob = rm.container(pb)
    plan = host.UnpackPlan(blob, fa)
    d = dict(fa=fa, pb=pb, blob=blob, plan=plan, reads=reads, names=names, iv=dm.intervals_a(pb))
    d["dec"] = tm.emu_decode_all(emu, plan, pb.max_read_len + pb.read_length - 1)
    return d


@pytest.fixture(scope="module")
def shapes(emu):
    fa, sam, pb, contigs, same_at = sm.shapes(64)
    d = _wrap(emu, fa, pb, sm.assert_models_agree(pb, sam), [n.encode() for n, _ in contigs])
    d["same_at"] = same_at
    yield d
    d["plan"].close(); pb.close()


@pytest.fixture(scope="module")
def mixed(emu):
    fa, pb, contigs = _dataset(7 + 64, 64)
    d = _wrap(emu, fa, pb, sm.reads_from_packed(pb), [n.encode() for n, _ in contigs])
    yield d
    d["plan"].close(); pb.close()


def _check(emu, d, given=None, regions=(), extra_bed=b"", exclude=0, **kw):
    """given: [(contig, beg, end)] as a BED text (None: the whole file); regions: [(string, interval)]."""
    plan = d["plan"]
    ts, keep = None, None
    if given is not None or regions:
        ts = plan.targets([r for r, _ in regions], tm.bed(given or [], d["names"]) + extra_bed)
        keep = sm.selected(d["iv"], [q for _, q in regions] + list(given or []))
    rc, got = sm.emu_stats(emu, plan, d["dec"], ts, exclude, **kw)
    want = sm.tables(d["reads"], exclude, keep)
    assert rc == 0 and sm.same(got, want), sm.diff(got, want)
    assert got["reads"] + got["excluded"] == (len(d["reads"]) if keep is None else int(keep.sum()))
    assert host.stats_text(got) == sm.text(want)
    return got


def test_shapes_whole_file(emu, shapes):
    d = shapes
    pb = d["pb"]
    assert sorted(set(pb.blocks["n_reads"].tolist())) != [64] and pb.n_blocks >= 4       # a last block that is not full
    assert {len(s) for _, s in d["reads"]} >= set(sm.LENGTHS) and {f for f, _ in d["reads"]} >= set(sm.FLAGS)
    assert max(sm.FLAGS) >= emu.emu_stats_lds_flags() > 2048 + 16
    b = d["same_at"] // 64                                                      # a block whose 64 reads carry one FLAG
    first = int(pb.blocks[b]["rec_base"])
    assert d["same_at"] % 64 == 0 and set(pb.recs["flag"][first:first + 64].tolist()) == {83}
    got = _check(emu, d)
    assert got["gc"][0] >= 2 and got["gc"][100] >= 2 and got["cyc"][4].sum() > 0 and got["len"][252] >= 2 and got["len"][1] >= 2
    for grid, waves in ((1, 1), (2, 3), (5, 4)):
        _check(emu, d, grid=grid, n_waves=waves)


def test_exclusion(emu, shapes, mixed):
    for d in (shapes, mixed):
        n = len(d["reads"])
        for ex in (0, 16, 0x400, 0xffff):
            got = _check(emu, d, exclude=ex)
            assert got["reads"] + got["excluded"] == n and (got["excluded"] == 0) == (ex == 0 or (ex == 0x400 and d is mixed))
    got = _check(emu, shapes, exclude=0xffff)
    assert got["reads"] == int(got["flag"][0]) > 0                             # only FLAG 0 passes every mask


def test_block_sizes(emu):
    """Blocks of 1, 63, 64 and 65 reads: the record-group boundary."""
    for n in (1, 63, 64, 65):
        fa, sam, _, contigs = synth.dataset(n, [20_000], [n + 64 + 3], 100, sub_rate=0.01)
        pb = host.pack_sam(sam, fa, block_reads=n, var_length=True)
        d = _wrap(emu, fa, pb, sm.assert_models_agree(pb, sam), [b"chr1"])
        assert n in pb.blocks["n_reads"].tolist()
        _check(emu, d)
        _check(emu, d, exclude=16, n_waves=2)
        d["plan"].close(); pb.close()


def test_mixed_dataset_and_regions(emu, mixed, shapes):
    d = mixed
    L = [int(c["length"]) for c in d["pb"].contigs]
    _check(emu, d)
    first = min(x[1] for x in d["iv"] if x[0] == 0)
    one = (0, first + 20, first + 160)
    _check(emu, d, regions=[(b"chr1:%d-%d" % one[1:], one)])
    ivs = [(0, first + 10, first + 40), (0, first + 41, first + 60), (0, first + 55, first + 120), (0, first + 10, first + 40),
           (len(L) - 1, 1, 300), (0, first, first), (0, first + 200, first + 201), (0, 1, 3), (1, 5000, 9000)]
    extra = b"chrUn_gl0\t5\t900\nchr1\t700\t700\n"
    got = _check(emu, d, ivs, extra_bed=extra, exclude=16)
    assert 0 < got["reads"] + got["excluded"] < len(d["reads"])
    # the deletion read at the end of block 0 reaches an interval that starts behind its last base of SEQ: kept by its span
    dpos = int(d["pb"].recs[63]["pos"]) + int(d["pb"].info[0]["window_start"])
    got = _check(emu, d, [(0, dpos + 130, dpos + 135)])
    assert got["len"][100] >= 1
    # a BED that selects nothing, and one that names only an unknown contig: nothing runs, all-zero tables
    for bed in (b"chr1\t5\t5\n", b"chrUn\t1\t500\n"):
        ts = d["plan"].targets((), bed)
        assert ts.n_blocks == 0
        rc, got = sm.emu_stats(emu, d["plan"], d["dec"], ts)
        assert rc == 0 and sm.same(got, sm.zero_tables())
    _check(emu, shapes, [(0, 1, 200), (1, 100, 400)], exclude=0x400)


def test_failed_block_zeroes_every_table(emu, mixed):
    rc, got = sm.emu_stats(emu, mixed["plan"], mixed["dec"], fail_blocks=(1,))
    assert rc == -4 and sm.same(got, sm.zero_tables())
    _check(emu, mixed)


def test_text_rules(built):
    z = sm.zero_tables()
    t = host.stats_text(z)
    assert t == sm.text(z) and t.startswith(b"SN\treads\t0\nSN\treads excluded\t0\nSN\tbases\t0\nSN\tminimum length\t0\nSN\tmaximum length\t0\n"
                                            b"SN\taverage length\t0.00\nSN\tbases A\t0\n")
    assert t.count(b"\n") == 11 + 15 and b"FL\t" not in t and b"BC\t" not in t and t.endswith(b"FS\treverse strand\t0\t0\n")
    # FLAG classes: secondary wins over supplementary; qc-failed goes to the second column; values of 4096 and above are listed
    reads = [(0x900, b"ACGT"), (0x800 | 16, b"AC"), (0x200 | 99, b"GGGGG"), (147, b"N"), (4096 + 16, b"ACGTN"), (0x400, b""), (73, b"T"),
             (65535 & ~4, b"A")]
    tb = sm.tables(reads)
    t = host.stats_text(tb)
    assert t == sm.text(tb)
    lines = t.split(b"\n")
    assert b"FS\tsecondary\t1\t1" in lines and b"FS\tsupplementary\t1\t0" in lines and b"FS\tproperly paired\t1\t1" in lines
    assert b"FS\tsingletons\t1\t0" in lines and b"FL\t4112\t1" in lines and b"FL\t65531\t1" in lines and b"RL\t0\t1" in lines
    assert b"SN\tminimum length\t0" in lines and b"SN\tmaximum length\t5" in lines and b"SN\taverage length\t2.38" in lines
    assert b"GC\t100\t1" in lines and b"BC\t5\t0\t0\t1\t1\t0" in lines and b"SN\tbases other\t2" in lines
    # the size bound holds the text of tables with every line at its longest
    cap = int(host.lib().cbc_stats_text_cap())
    full = dict(reads=2 ** 64 - 1, excluded=2 ** 64 - 1, flag=np.full(65536, 2 ** 32 - 1, np.uint32), len=np.full(257, 2 ** 32 - 1, np.uint32),
                gc=np.full(101, 2 ** 32 - 1, np.uint32), cyc=np.full((5, 256), 2 ** 32 - 1, np.uint32))
    assert len(host.stats_text(full)) <= cap < 2 * 1024 * 1024
    for total, n in ((0, 0), (1, 3), (2, 3), (299, 2), (10 ** 12 + 1, 7)):
        assert host.coverage_mean(total, n) == sm.mean(total, n)


def test_sanitizer_build_of_the_stand_alone_check(built):
    """stats_emu_check: fabricated records and rows (bytes past the length never zero, strides 4 .. 256) in a program of its own
    under AddressSanitizer / UBSan, every table at its exact size; it exits non-zero on a finding or a mismatch."""
    subprocess.check_call(["make", "-C", EMU_DIR, "asan_check"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(EMU_DIR, "stats_emu_check")], capture_output=True, text=True)
    assert r.returncode == 0 and "STATS EMU CHECK OK" in r.stdout and "MISMATCH" not in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- the CLI where no device is needed -----------------------------------------------------------------------------------------
def _cli(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def test_cli_refusals_and_empty_selection(built, mixed, tmp_path):
    d = mixed
    (tmp_path / "in.cbc").write_bytes(d["blob"]); (tmp_path / "ref.fa").write_bytes(d["fa"])
    files = (tmp_path / "in.cbc", tmp_path / "o.txt", tmp_path / "ref.fa")
    for args, msg in [(("--stats", "--sam"), "different outputs"), (("--stats", "--depth"), "different outputs"),
                      (("--stats", "--bedcov"), "different outputs"), (("--stats", "--depth-hist"), "different outputs"),
                      (("--stats", "--devices", "0,1"), "one device"), (("--stats-exclude-flags", "16"), "--stats-exclude-flags applies to --stats"),
                      (("--sam", "--stats-exclude-flags", "16"), "--stats-exclude-flags applies to --stats"),
                      (("--stats", "--stats-exclude-flags", "65536"), "--stats-exclude-flags wants"),
                      (("--stats", "--stats-exclude-flags", "x"), "--stats-exclude-flags wants"),
                      (("--stats", "--hist-max", "5"), "--hist-max applies to --depth-hist"),
                      (("--stats", "--depth-exclude-flags", "4"), "--depth-exclude-flags applies to --depth"),
                      (("--stats", "--region", "chrX:1-5"), "unknown contig"), (("--stats", "--regions-file", tmp_path / "none.bed"), "cannot open")]:
        r = _cli("-x", *files, *args)
        assert r.returncode == 1 and msg in r.stderr, (args, r.stderr)
    r = _cli("-c", tmp_path / "in.sam", tmp_path / "o.cbc", tmp_path / "ref.fa", "--stats")
    assert r.returncode == 1 and "--stats applies to decompression" in r.stderr, r.stderr
    fa, sam, _, _ = synth.dataset(4, [5000], [100], 100)
    (tmp_path / "c.cbc").write_bytes(oracle.encode(sam, fa)); (tmp_path / "c.fa").write_bytes(fa)
    r = _cli("-x", tmp_path / "c.cbc", tmp_path / "o.txt", tmp_path / "c.fa", "--stats")
    assert r.returncode == 1 and "single-stream (--compat) file" in r.stderr, r.stderr
    pb, _, lfa = host.synth_long(5, 200_000, 40, read_len=2000, want_text=True)
    flat, offs, _ = oracle.cpu_encode_blocks(pb, long_reads=True, return_flat=True)
    (tmp_path / "l.cbc").write_bytes(pb.container(flat, offs)); (tmp_path / "l.fa").write_bytes(lfa)
    for extra in ((), ("--region", "chr1:1-50")):
        r = _cli("-x", tmp_path / "l.cbc", tmp_path / "o.txt", tmp_path / "l.fa", "--stats", *extra)
        assert r.returncode == 1 and "long-read" in r.stderr, r.stderr
    pb.close()
    # a BED that selects nothing, and one that names only an unknown contig: no device is opened, all-zero tables, status 0
    for bed in (b"chr1\t5\t5\n", b"chrUn\t1\t500\n"):
        (tmp_path / "e.bed").write_bytes(bed)
        (tmp_path / "o.txt").write_bytes(b"stale")
        r = _cli("-x", *files, "--stats", "--regions-file", tmp_path / "e.bed", "--verbose", "--stats-exclude-flags", "0x400")
        assert r.returncode == 0, r.stderr
        assert (tmp_path / "o.txt").read_bytes() == sm.text(sm.zero_tables())
        assert "kernels:" not in r.stdout and "statistics of 0 reads" in r.stdout and "1 BED lines selected nothing" in r.stdout


def test_exports_name_the_statistics_entry_points(built):
    from cbc_amd import gpu
    assert {"cbc_gpu_decode_stats", "cbc_gpu_last_stats_ms"} <= set(gpu.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "cbc_gpu.h")).read()
    assert "cbc_gpu_decode_stats(" in hdr and "cbc_gpu_last_stats_ms(" in hdr and "typedef struct cbc_gpu_stats" in hdr
    hdr = open(os.path.join(ROOT, "include", "cbc_host.h")).read()
    assert "cbc_stats_text(" in hdr and "cbc_stats_text_cap(" in hdr
    import ctypes
    assert ctypes.sizeof(host.GpuStats) == 16 + 4 * (65536 + 257 + 101 + 5 * 256)
    assert hasattr(gpu.Encoder, "decode_stats") and hasattr(gpu.Encoder, "last_stats_ms") and hasattr(host, "stats_text")
