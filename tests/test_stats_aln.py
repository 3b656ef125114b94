"""The alignment tables of the read statistics without a GPU: the edit-reporting decoder, the three
bodies of cbc_stats_body.h and the three of cbc_stats_aln_body.h on the lock-step wave emulation (tests/alnstats_emu) against the
two models of alnstatsmodel.py, whole file and with regions; the formatter's text against the model's text; the stand-alone
sanitizer program; and the CLI where no device is needed."""
import os
import subprocess

import numpy as np
import pytest

import alnstatsmodel as am
import statsmodel as sm
import targetsmodel as tm
from cbc_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "alnstats_emu")
EXE = os.path.join(ROOT, "cbc_amd", "csrc", "cbc")


@pytest.fixture(scope="module")
def emu(built):
    subprocess.check_call(["make", "-C", EMU_DIR, "libcbc_alnstats_emu.so"], stdout=subprocess.DEVNULL)
    return am.emu_load(os.path.join(EMU_DIR, "libcbc_alnstats_emu.so"))


@pytest.fixture(scope="module")
def data(emu):
    ds = {}
    for name in am.DATASETS:
        d = am.open_dataset(name)                       # models (a) and (b) agree on every table, or this fails
        d["dec"] = am.emu_decode_all(emu, d["plan"])
        assert (d["dec"]["res"]["status"] == 0).all()
        d["stat_reads"] = sm.reads_from_packed(d["pb"])
        ds[name] = d
    yield ds
    for d in ds.values():
        d["plan"].close(); d["pb"].close()


def _check(emu, d, given=None, regions=(), exclude=0, **kw):
    """given: [(contig, beg, end)] as a BED text (None: the whole file); regions: [(string, interval)]."""
    plan = d["plan"]
    ts, keep = None, None
    if given is not None or regions:
        ts = plan.targets([r for r, _ in regions], tm.bed(given or [], d["names"]))
        keep = sm.selected(d["iv"], [q for _, q in regions] + list(given or []))
    rc, st, al = am.emu_stats_aln(emu, plan, d["dec"], ts, exclude, **kw)
    want, excluded = am.tables_a(d["pb"], d["reads"], exclude, keep)
    assert rc == 0 and am.same(al, want), am.diff(al, want)
    want_st = sm.tables(d["stat_reads"], exclude, keep)
    assert sm.same(st, want_st), sm.diff(st, want_st)  # `out` is what the statistics call gives for the selection
    assert st["excluded"] == excluded and st["reads"] == al["reads"] + al["invalid"]
    t = host.stats_aln_text(al)
    assert t == am.text(want)
    # the identities: every valid read has one NM, and the NM values add up to the edits counted
    nm = np.asarray(al["nm"]).astype(np.int64)
    il, dl = np.asarray(al["ins_len"]).astype(np.int64), np.asarray(al["del_len"]).astype(np.int64)
    assert nm.sum() == al["reads"]
    assert (np.arange(767) * nm).sum() == int(np.asarray(al["mm"]).sum()) + (np.arange(256) * il).sum() + (np.arange(256) * dl).sum()
    assert int(np.asarray(al["ins_cyc"]).sum()) == il.sum() and int(np.asarray(al["del_cyc"]).sum()) == dl.sum()
    return st, al, t


def test_datasets_hold_every_kind(data):
    w = data["handmade2"]["whole"]
    assert w["del_cyc"][0] >= 2 and w["len"][1] >= 4 and w["reads"] == 2 * len(am.HANDMADE2) and w["invalid"] == 0
    tags = [t[0] for t in data["handmade2"]["tags"]]
    assert {"3D97M", "97M3D", "2D50M1D1M2D47M4D", "5M1D1M1D94M", "1M", "1S"} <= set(tags)
    flags = [rd["flag"] & 16 for rd in data["handmade2"]["reads"]]
    assert flags.count(0) == flags.count(16) == len(am.HANDMADE2)
    w = data["indel"]["whole"]
    assert w["reads"] == 1000 and w["ins_len"].sum() >= 50 and w["del_len"].sum() >= 50 and w["mm"].sum() >= 500
    assert {rd["flag"] & 16 for rd in data["indel"]["reads"]} == {0, 16}
    assert data["genome"]["whole"]["reads"] >= 600 and data["handmade"]["whole"]["reads"] == 6


@pytest.mark.parametrize("name", list(am.DATASETS))
def test_emulation_matches_the_models_whole_file(emu, data, name):
    d = data[name]
    st, al, t = _check(emu, d)
    assert am.same(al, d["whole"])
    assert t.startswith(b"AS\treads\t%d\nAS\treads without alignment\t0\n" % len(d["reads"]))
    for grid, waves in ((1, 1), (2, 3)):
        _check(emu, d, grid=grid, n_waves=waves)
    _check(emu, d, exclude=16, n_waves=2)


@pytest.mark.parametrize("name", list(am.DATASETS))
def test_emulation_matches_the_models_with_regions(emu, data, name):
    d = data[name]
    nm0, first = d["names"][0], min(x[1] for x in d["iv"] if x[0] == 0)
    one = (0, first + 20, first + 160)
    st, al, _ = _check(emu, d, regions=[(b"%s:%d-%d" % ((nm0,) + one[1:]), one)])
    assert 0 < st["reads"] < len(d["reads"])
    last = max(x[1] for x in d["iv"] if x[0] == 0)
    two = (0, last - 30, last + 5)
    given = [(0, first + 300, first + 420), (len(d["names"]) - 1, 1, 900)]
    st, al, _ = _check(emu, d, given, regions=[(b"%s:%d-%d" % ((nm0,) + one[1:]), one), (b"%s:%d-%d" % ((nm0,) + two[1:]), two)], exclude=16)
    assert 0 < st["reads"] + st["excluded"] <= len(d["reads"])
    # a window cut through one read: an interval of one base inside its span
    k = len(d["iv"]) // 2
    x = d["iv"][k]
    _check(emu, d, [(x[0], x[1] + 1, x[1] + 1)])


def test_failed_block_zeroes_every_table(emu, data):
    d = data["indel"]
    rc, st, al = am.emu_stats_aln(emu, d["plan"], d["dec"], fail_blocks=(1,))
    assert rc == -4 and sm.same(st, sm.zero_tables()) and am.same(al, am.zero_tables())


def test_a_selection_without_blocks(emu, data):
    d = data["indel"]
    for bed in (b"%s\t5\t5\n" % d["names"][0], b"chrUn\t1\t500\n"):
        ts = d["plan"].targets((), bed)
        assert ts.n_blocks == 0
        rc, st, al = am.emu_stats_aln(emu, d["plan"], d["dec"], ts)
        assert rc == 0 and sm.same(st, sm.zero_tables()) and am.same(al, am.zero_tables())


def test_text_rules(built):
    z = am.zero_tables()
    t = host.stats_aln_text(z)
    assert t == am.text(z) == (b"AS\treads\t0\nAS\treads without alignment\t0\nAS\tbases aligned\t0\nAS\tmismatches\t0\n"
                               b"AS\tmismatch rate\t0.000000\nAS\tinsertions\t0\nAS\tdeletions\t0\nAS\tbases inserted\t0\n"
                               b"AS\tbases deleted\t0\nAS\tbases soft-clipped\t0\nAS\treads with NM 0\t0\n")
    # two reads of length 4 and 2: one mismatch in cycle 4, a 2-base insertion at cycle 2, a deletion in front of the first base,
    # one soft-clipped base in cycle 1; counters past 2^32 in the 64-bit tables
    a = am.zero_tables()
    a["reads"], a["invalid"] = 2, 3
    a["len"][4] = a["len"][2] = 1
    a["mm"][4] = 1; a["unal"][1] = 1; a["unal"][2] = 1; a["unal"][3] = 1
    a["ins_cyc"][2] = 1; a["del_cyc"][0] = 1; a["ins_len"][2] = 1; a["del_len"][255] = 2 ** 33; a["nm"][0] = 1; a["nm"][766] = 1
    t = host.stats_aln_text(a)
    assert t == am.text(a)
    lines = t.split(b"\n")
    assert b"AS\tbases aligned\t3" in lines and b"AS\tmismatch rate\t0.333333" in lines and b"AS\tbases soft-clipped\t1" in lines
    assert b"AS\tbases deleted\t%d" % (255 * 2 ** 33) in lines and b"AS\treads without alignment\t3" in lines
    assert b"MC\t1\t1\t0" in lines and b"MC\t2\t1\t0" in lines and b"MC\t3\t0\t0" in lines and b"MC\t4\t1\t1" in lines and b"MC\t5\t0\t0" not in lines
    assert b"IC\t0\t0\t1" in lines and b"IC\t2\t1\t0" in lines and b"ID\t2\t1\t0" in lines and b"ID\t255\t0\t%d" % 2 ** 33 in lines
    assert b"NM\t0\t1" in lines and b"NM\t766\t1" in lines
    # the size bound holds the text of tables with every line at its longest
    cap = int(host.lib().cbc_stats_aln_text_cap())
    full = dict(reads=2 ** 64 - 1, invalid=2 ** 64 - 1)
    for name, n, dt in am.TABLES:
        full[name] = np.full(n, np.iinfo(dt).max, dtype=dt)
    full["unal"][:] = 0
    assert len(host.stats_aln_text(full)) <= cap < 256 * 1024
    assert am.fraction(1, 3) == host.hist_fraction(1, 3) and am.fraction(5, 0) == host.hist_fraction(5, 0)


def test_sanitizer_build_of_the_stand_alone_check(built):
    """alnstats_emu_check: fabricated records, rows and arena entries in a program of its own under AddressSanitizer / UBSan,
    every table at its exact size; it exits non-zero on a finding or a mismatch."""
    subprocess.check_call(["make", "-C", EMU_DIR, "asan_check"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(EMU_DIR, "alnstats_emu_check")], capture_output=True, text=True)
    assert r.returncode == 0 and "ALNSTATS EMU CHECK OK" in r.stdout and "MISMATCH" not in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    assert "preloaded to 0xFFFFFFF0" in r.stdout and "ins_len[1] 4294967" in r.stdout


# ---- the CLI where no device is needed -----------------------------------------------------------------------------------------
def _cli(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def test_cli_refusals_and_empty_selection(built, data, tmp_path):
    d = data["indel"]
    (tmp_path / "in.cbc").write_bytes(d["blob"]); (tmp_path / "ref.fa").write_bytes(d["fa"])
    files = (tmp_path / "in.cbc", tmp_path / "o.txt", tmp_path / "ref.fa")
    for args, msg in [(("--alignment",), "--alignment applies to --stats"), (("--sam", "--alignment"), "--alignment applies to --stats"),
                      (("--pileup", "--alignment"), "--alignment applies to --stats"),
                      (("--stats", "--alignment", "--sam"), "different outputs"), (("--stats", "--alignment", "--pileup"), "different outputs"),
                      (("--stats", "--alignment", "--devices", "0,1"), "one device"),
                      (("--stats", "--max-edits-per-read", "4"), "--max-edits-per-read applies to --pileup"),
                      (("--stats", "--alignment", "--max-edits-per-read", "511"), "--max-edits-per-read wants"),
                      (("--stats", "--alignment", "--stats-exclude-flags", "65536"), "--stats-exclude-flags wants"),
                      (("--stats", "--alignment", "--region", "chrX:1-5"), "unknown contig"),
                      (("--stats", "--alignment", "--regions-file", tmp_path / "none.bed"), "cannot open")]:
        r = _cli("-x", *files, *args)
        assert r.returncode == 1 and msg in r.stderr, (args, r.stderr)
    r = _cli("-c", tmp_path / "in.sam", tmp_path / "o.cbc", tmp_path / "ref.fa", "--stats", "--alignment")
    assert r.returncode == 1 and "--stats applies to decompression" in r.stderr, r.stderr
    # a BED that selects nothing, and one that names only an unknown contig: no device is opened; the zeros of --stats, then
    # all-zero AS lines and no table lines
    for bed in (b"%s\t5\t5\n" % d["names"][0], b"chrUn\t1\t500\n"):
        (tmp_path / "e.bed").write_bytes(bed)
        (tmp_path / "o.txt").write_bytes(b"stale")
        r = _cli("-x", *files, "--stats", "--alignment", "--regions-file", tmp_path / "e.bed", "--verbose", "--max-edits-per-read", "8")
        assert r.returncode == 0, r.stderr
        assert (tmp_path / "o.txt").read_bytes() == sm.text(sm.zero_tables()) + am.text(am.zero_tables())
        assert "kernels:" not in r.stdout and "statistics of 0 reads" in r.stdout
        (tmp_path / "p.txt").write_bytes(b"stale")
        r = _cli("-x", tmp_path / "in.cbc", tmp_path / "p.txt", tmp_path / "ref.fa", "--stats", "--regions-file", tmp_path / "e.bed")
        assert r.returncode == 0 and (tmp_path / "p.txt").read_bytes() == sm.text(sm.zero_tables())


def test_exports_name_the_new_entry_points(built):
    import ctypes
    from cbc_amd import gpu
    assert {"cbc_gpu_decode_stats_aln", "cbc_gpu_last_stats_aln_ms"} <= set(gpu.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "cbc_gpu.h")).read()
    assert "cbc_gpu_decode_stats_aln(" in hdr and "cbc_gpu_last_stats_aln_ms(" in hdr and "typedef struct cbc_gpu_stats_aln" in hdr
    hdr = open(os.path.join(ROOT, "include", "cbc_host.h")).read()
    assert "cbc_stats_aln_text(" in hdr and "cbc_stats_aln_text_cap(" in hdr
    assert ctypes.sizeof(host.GpuStatsAln) == 16 + 4 * (5 * 257 + 767) + 8 * 2 * 256
    assert hasattr(gpu.Encoder, "decode_stats_aln") and hasattr(gpu.Encoder, "last_stats_aln_ms") and hasattr(host, "stats_aln_text")
