"""The alignment tables of the read statistics on the MI355X: Encoder.decode_stats_aln and
`cbc -x --stats --alignment` against model (a) of alnstatsmodel.py on the four datasets, whole file and with regions; `out`
against decode_stats; the tables against model (b) applied to what decode_sam(cigar=True) returns, which this change does not
touch; a panel whose bins pass 65 535; a failed block; an arena too small.  Every comparison is exact."""
import os
import subprocess

import numpy as np
import pytest

import alnstatsmodel as am
import statsmodel as sm
import synth
import targetsmodel as tm
from cbc_amd import gpu, host

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cbc_amd", "csrc", "cbc")


@pytest.fixture(scope="module")
def enc():
    e = gpu.Encoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def data(built):
    ds = {}
    for name in am.DATASETS:
        ds[name] = am.open_dataset(name)                # models (a) and (b) agree on every table, or this fails
    yield ds
    for d in ds.values():
        d["plan"].close(); d["pb"].close()


def _cli(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def _check(enc, d, given=None, regions=(), exclude=0, cli_dir=None):
    """decode_stats_aln (and, with cli_dir, the CLI on the same selection) against model (a) and against decode_stats.
    given: [(contig, beg, end)] as a BED text (None: the whole file); regions: [(string, interval)]."""
    plan = d["plan"]
    ts, keep, bed = None, None, None
    if given is not None or regions:
        bed = tm.bed(given or [], d["names"])
        ts = plan.targets([r for r, _ in regions], bed)
        keep = sm.selected(d["iv"], [q for _, q in regions] + list(given or []))
    st, al = enc.decode_stats_aln(plan, ts, exclude)
    want, excluded = am.tables_a(d["pb"], d["reads"], exclude, keep)
    assert am.same(al, want), am.diff(al, want)
    plain = enc.decode_stats(plan, ts, exclude)
    assert sm.same(st, plain), sm.diff(st, plain)      # `out` equals decode_stats of the same selection
    assert st["excluded"] == excluded and st["reads"] == al["reads"] + al["invalid"]
    assert all(al[k].dtype == dt for k, _, dt in am.TABLES)
    assert host.stats_aln_text(al) == am.text(want)
    if cli_dir is not None:
        (cli_dir / "in.cbc").write_bytes(d["blob"]); (cli_dir / "ref.fa").write_bytes(d["fa"])
        args = [x for r, _ in regions for x in ("--region", r.decode())]
        if bed:
            (cli_dir / "q.bed").write_bytes(bed)
            args += ["--regions-file", cli_dir / "q.bed"]
        if exclude:
            args += ["--stats-exclude-flags", exclude]
        r = _cli("-x", cli_dir / "in.cbc", cli_dir / "out.txt", cli_dir / "ref.fa", "--stats", "--alignment", "--verbose", *args)
        assert r.returncode == 0, r.stderr
        # exactly the bytes of --stats for the same selection, then the new sections
        assert (cli_dir / "out.txt").read_bytes() == host.stats_text(plain) + am.text(want)
        assert "kernels: edits decode" in r.stdout and "alignment: %d reads, %d without alignment" % (want["reads"], want["invalid"]) in r.stdout
        r = _cli("-x", cli_dir / "in.cbc", cli_dir / "plain.txt", cli_dir / "ref.fa", "--stats", *args)
        assert r.returncode == 0 and (cli_dir / "plain.txt").read_bytes() == host.stats_text(plain), r.stderr
    return st, al, ts


def _intervals(d):
    nm0, first = d["names"][0], min(x[1] for x in d["iv"] if x[0] == 0)
    last = max(x[1] for x in d["iv"] if x[0] == 0)
    one, two = (0, first + 20, first + 160), (0, last - 30, last + 5)
    return (b"%s:%d-%d" % ((nm0,) + one[1:]), one), (b"%s:%d-%d" % ((nm0,) + two[1:]), two), \
        [(0, first + 300, first + 420), (len(d["names"]) - 1, 1, 900)]


@pytest.mark.parametrize("name", list(am.DATASETS))
def test_python_and_cli_against_model_a(enc, data, name, tmp_path):
    d = data[name]
    enc.upload_reference(d["plan"].ref)
    st, al, _ = _check(enc, d, cli_dir=tmp_path)
    assert am.same(al, d["whole"]) and al["invalid"] == 0
    ms = enc.last_stats_aln_ms()
    assert len(ms) == 3 and all(x > 0 for x in ms)
    _check(enc, d, exclude=16)
    one, two, given = _intervals(d)
    st, al, _ = _check(enc, d, regions=[one], cli_dir=tmp_path)
    assert 0 < st["reads"] < len(d["reads"])
    _check(enc, d, given, regions=[one, two], exclude=16, cli_dir=tmp_path)
    # a BED that selects nothing: nothing runs, all-zero tables
    ts = d["plan"].targets((), b"chrUn\t1\t500\n")
    st, al = enc.decode_stats_aln(d["plan"], ts)
    assert ts.n_blocks == 0 and sm.same(st, sm.zero_tables()) and am.same(al, am.zero_tables())


@pytest.mark.parametrize("name", list(am.DATASETS))
def test_tables_equal_model_b_on_the_sam_text(enc, data, name):
    """Model (b) reads nothing but the text decode_sam(cigar=True) writes."""
    d = data[name]
    plan = d["plan"]
    enc.upload_reference(plan.ref)
    want, _ = am.tables_b(enc.decode_sam(plan, cigar=True))
    st, al = enc.decode_stats_aln(plan)
    assert am.same(al, want), am.diff(al, want)
    one, _, _ = _intervals(d)
    want, _ = am.tables_b(enc.decode_sam(plan, one[0], cigar=True))
    st, al = enc.decode_stats_aln(plan, plan.targets([one[0]]))
    assert want["reads"] > 0 and am.same(al, want), am.diff(al, want)


def test_panel_past_65535(enc, built):
    """70 000 identical 100-base reads on one place, each with one mismatch and one 1-base insertion: many workgroups flush into
    the same few words, and the bins pass 65 535."""
    n = 70_000
    rng = np.random.default_rng(5)
    c = synth.make_contig(rng, 2000)
    s = 500
    seq = np.concatenate([c[s:s + 50], np.frombuffer(b"A", dtype=np.uint8), c[s + 50:s + 99]]).copy()
    seq[10] = ord("A") if seq[10] != ord("A") else ord("C")
    ops = [("M", 50), ("I", 1), ("M", 49)]
    md, nm = synth._md_and_nm(c, s, ops, seq)
    assert nm == 2
    rec = dict(pos=s + 1, flag=0, cigar="50M1I49M", seq=seq.tobytes(), md=md, nm=nm)
    fa, sam = synth.fasta_text([("p", c)]), synth.sam_text([("p", len(c), [rec] * n)])
    pb = host.pack_sam(sam, fa, block_reads=4096)
    import regionmodel as rm
    plan = host.UnpackPlan(rm.container(pb), fa)
    enc.upload_reference(plan.ref)
    st, al = enc.decode_stats_aln(plan)
    want = am.zero_tables()
    want["reads"] = n
    for k, i in (("len", 100), ("mm", 11), ("unal", 51), ("ins_cyc", 51), ("ins_len", 1), ("nm", 2)):
        want[k][i] = n
    assert am.same(al, want), am.diff(al, want)
    assert st["reads"] == n and n > 65_535
    print("alignment statistics kernel ms (edits decode, zero + statistics, alignment):", enc.last_stats_aln_ms())
    plan.close(); pb.close()


def test_failed_block_zeroes_every_table(enc, data):
    """A payload byte of block 1 flipped: the block fails to decode (an error status, no fault), the call reports CBC_E_BLOCK
    naming the block and every table of both structs stays zero; the next good call is correct again."""
    d = data["indel"]
    blob = bytearray(d["blob"])
    base = len(blob) - d["plan"].payloads.size
    blob[base + int(d["plan"].blocks[1]["in_off"]) + int(d["plan"].blocks[1]["in_bytes"]) // 2] ^= 0x55
    plan = host.UnpackPlan(bytes(blob), d["fa"])
    enc.upload_reference(plan.ref)
    st, al, res = enc.decode_stats_aln(plan, results=True)
    assert [b for b in range(len(res)) if res[b]["status"] != 0] == [1]
    assert sm.same(st, sm.zero_tables()) and am.same(al, am.zero_tables())
    with pytest.raises(gpu.CbcGpuError, match=r"block 1\b"):
        enc.decode_stats_aln(plan)
    enc.upload_reference(d["plan"].ref)
    _check(enc, d)
    plan.close()


def test_an_arena_too_small_fails_with_the_option_named(enc, data, tmp_path):
    d = data["indel"]
    enc.upload_reference(d["plan"].ref)
    st, al, res = enc.decode_stats_aln(d["plan"], edits_per_read=1, results=True)
    assert 9 in set(res["status"].tolist()) and set(res["status"].tolist()) <= {0, 9}      # CBC_ST_EDITS
    assert sm.same(st, sm.zero_tables()) and am.same(al, am.zero_tables())
    with pytest.raises(gpu.CbcGpuError, match="max-edits-per-read"):
        enc.decode_stats_aln(d["plan"], edits_per_read=1)
    (tmp_path / "in.cbc").write_bytes(d["blob"]); (tmp_path / "ref.fa").write_bytes(d["fa"])
    r = _cli("-x", tmp_path / "in.cbc", tmp_path / "o.txt", tmp_path / "ref.fa", "--stats", "--alignment", "--max-edits-per-read", 1)
    assert r.returncode == 1 and "--max-edits-per-read" in r.stderr, r.stderr
    _check(enc, d)
