"""Per-strand counts and the minimum alternative fraction of the pileup on the MI355X:
Encoder.decode_pileup(by_strand=, min_alt_ppm=) and `cbc -x --pileup --by-strand --min-alt-frac F` against pileupstrandmodel.py;
identities against code that is not under test (the existing decode_pileup and decode_depth); counters past 65 535 with the
rule's products past 2^32; a block that fails; a text_cap too small.

The datasets are those of tests/test_pileup_gpu.py.  What the by-strand tests rely on is asserted in the first test: at least
20 % of the kept reads on each strand and at least 20 reported positions where both strands show a non-reference observation --
except that `mixed` has both strands but only 10 such positions (its coverage is thin); it is kept and held to one.  The
fractions 0.3 and 0.5 were chosen from the model: on each dataset the rule keeps and drops at least 10 % of the lines of the call
without it (0.02 and 0.2 drop under 10 % at these depths, 1 keeps under 10 % of `mixed`); 0.2 and 1 are used where the issue
names them, for the subset identity."""
import os
import subprocess

import numpy as np
import pytest

import depthmodel as dm
import pileupmodel as pm
import pileupstrandmodel as psm
import synth
from cbc_amd import gpu, host
from test_pileup_gpu import _make, _open, _tiled

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cbc_amd", "csrc", "cbc")
FRACTIONS = (300_000, 500_000)
FRACTION_TEXT = {300_000: "0.3", 500_000: "0.5"}
MIN_BOTH = {"shared": 20, "mixed": 1, "genome": 20}


@pytest.fixture(scope="module")
def enc():
    e = gpu.Encoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module", params=["shared", "mixed", "genome"])
def data(request, built):
    d = _make(request.param)
    d["kind"] = request.param
    yield d
    d["plan"].close(); d["pb"].close()


def _cli(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def _pos(text):
    return [int(ln.split(b"\t")[1]) for ln in text.split(b"\n")[:-1]]


def test_by_strand_and_fraction_match_the_model(enc, data, tmp_path):
    """Fails without the feature: the binding and the binary against the model's bytes, whole file and five windows; by_strand
    with and without a fraction, a fraction alone, exclusion masks 4 and 16."""
    plan, pb, reads, names, lens = data["plan"], data["pb"], data["reads"], data["names"], data["lens"]
    assert FRACTION_TEXT and all(gpu.alt_frac_ppm(s) == p for p, s in FRACTION_TEXT.items())
    psm.assert_both_strands(pb, reads, names, lens, min_both=MIN_BOTH[data["kind"]])
    base = psm.expected(pb, reads, names, lens)[1]
    for ppm in FRACTIONS:
        n = psm.expected(pb, reads, names, lens, ppm=ppm)[1]
        assert 0.1 * base <= n <= 0.9 * base, (ppm, n, base)
    enc.upload_reference(plan.ref)
    (tmp_path / "in.cbc").write_bytes(data["blob"]); (tmp_path / "ref.fa").write_bytes(data["fa"])
    files = (tmp_path / "in.cbc", tmp_path / "out.txt", tmp_path / "ref.fa")
    for i, (bs, ppm, ex, k) in enumerate(((True, 0, 0, 1), (True, FRACTIONS[0], 0, 1), (False, FRACTIONS[1], 0, 1), (True, 0, 4, 1),
                                         (True, FRACTIONS[1], 16, 2))):
        want = psm.expected(pb, reads, names, lens, None, ex, k, ppm, bs)
        text, lines, kept, res = enc.decode_pileup(plan, exclude_flags=ex, min_alt=k, by_strand=bs, min_alt_ppm=ppm, results=True)
        assert (res["status"] == 0).all() and len(res) == plan.n_blocks
        assert (lines, kept) == want[1:] and text == want[0], (bs, ppm, ex, k)
        if i in (1, 2, 4):
            opts = (["--by-strand"] if bs else []) + (["--min-alt-frac", FRACTION_TEXT[ppm]] if ppm else [])
            r = _cli("-x", *files, "--pileup", "--min-alt", k, "--depth-exclude-flags", ex, *opts, "--verbose")
            assert r.returncode == 0, r.stderr
            assert (tmp_path / "out.txt").read_bytes() == want[0], (bs, ppm, ex, k)
            assert "kernels: edits decode" in r.stdout and "%d positions from %d reads" % want[1:] in r.stdout, r.stdout
    ms = enc.last_pileup_ms()
    assert len(ms) == 4 and ms[0] > 0 and all(x >= 0 for x in ms)
    wins = pm.windows(pb, reads, lens, 5, 3)[:5]
    for i, (s, c, beg, end) in enumerate(wins):
        ppm, k = (0, FRACTIONS[0], FRACTIONS[1])[i % 3], 1 + 2 * (i % 2)
        want = psm.expected(pb, reads, names, lens, (c, beg, end), 0, k, ppm, True)
        got = enc.decode_pileup(plan, s, min_alt=k, by_strand=True, min_alt_ppm=ppm, results=True)
        assert (got[0], got[1], got[2]) == want, (s, k, ppm)
    s, c, beg, end = wins[0]
    r = _cli("-d", *files, "--pileup", "--by-strand", "--region", s)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "out.txt").read_bytes() == psm.expected(pb, reads, names, lens, (c, beg, end), by_strand=True)[0], s


def test_identities_against_the_plain_pileup(enc, data):
    """Against code not under test.  The first eleven columns and the set of lines of a by_strand call are the bytes of the
    existing decode_pileup; every line of the existing decode_pileup(exclude_flags=E | 16) has a by-strand line at its position
    whose seven + columns are that line's seven counts; X+ <= X everywhere; with a fraction the text is exactly the lines of
    the call without one that pass the rule, computed in Python from their own columns; pos_of(F = 1) is a subset of
    pos_of(F = 0.2), which is a subset of pos_of(no fraction)."""
    plan = data["plan"]
    enc.upload_reference(plan.ref)
    for E in (0, 4):
        plain = enc.decode_pileup(plan, exclude_flags=E)
        text = enc.decode_pileup(plan, exclude_flags=E, by_strand=True)
        assert psm.first_eleven(text) == plain
        by_key = {(r[0], r[1]): r for r in psm.parse(text)}
        assert len(by_key) == len(psm.parse(text))
        fwd = pm.parse(enc.decode_pileup(plan, exclude_flags=E | 16))
        assert len(fwd) > 20
        for f in fwd:
            assert by_key[(f[0], f[1])][11:] == f[4:11], f
        assert all(r[11 + j] <= r[4 + j] for r in by_key.values() for j in range(7))
        for k, ppm in ((1, FRACTIONS[0]), (2, FRACTIONS[1]), (1, 1_000_000), (1, 1)):
            assert enc.decode_pileup(plan, exclude_flags=E, min_alt=k, min_alt_ppm=ppm) == psm.passing(plain, k, ppm), (E, k, ppm)
            assert enc.decode_pileup(plan, exclude_flags=E, min_alt=k, min_alt_ppm=ppm, by_strand=True) == psm.passing(text, k, ppm), (E, k, ppm)
    none = set(_names_pos(enc.decode_pileup(plan)))
    p02 = set(_names_pos(enc.decode_pileup(plan, min_alt_ppm=200_000)))
    p1 = set(_names_pos(enc.decode_pileup(plan, min_alt_ppm=1_000_000)))
    assert p1 <= p02 <= none and p1 and len(p1) < len(none)


def _names_pos(text):
    return [tuple(ln.split(b"\t")[:2]) for ln in text.split(b"\n")[:-1]]


def test_reference_only_plus_columns_against_depth(enc, built):
    """On _tiled(), over the window from position 2 (every covered position is reported there): the by-strand lines that the
    forward-only call does not report hold, in their + columns, only the reference class, with del+ = ins+ = 0; and the sum of
    the + columns A+ .. del+ of every line, run-length encoded, is the text of decode_depth(exclude_flags=E | 16)."""
    d = _open(*_tiled())
    plan, reads = d["plan"], d["reads"]
    psm.assert_both_strands(d["pb"], reads, d["names"], d["lens"])
    enc.upload_reference(plan.ref)
    last = max(r["pos"] + r["span"] - 1 for r in reads)
    region = "tile:2-%d" % last
    for E in (0, 256):                                               # no read carries FLAG 256: the mask alone differs
        rows = psm.parse(enc.decode_pileup(plan, region, exclude_flags=E, by_strand=True))
        fwd_pos = {r[1] for r in pm.parse(enc.decode_pileup(plan, region, exclude_flags=E | 16))}
        rest = [r for r in rows if r[1] not in fwd_pos]
        assert len(rest) >= 1
        for r in rest:
            plus, cls = list(r[11:16]), int(pm.klass(r[2][0]))
            assert r[16] == r[17] == 0 and all(x == 0 for j, x in enumerate(plus) if j != cls), r
        bg = enc.decode_depth(plan, region, exclude_flags=E | 16)
        full = np.zeros(last - 1, dtype=np.int64)
        for r in rows:
            full[r[1] - 2] = sum(r[11:17])
        covered = sum(e - s for _, s, e, _ in dm.parse(enc.decode_depth(plan, region, exclude_flags=E)))
        assert len(rows) == covered                                  # every covered position has its line
        assert dm.bedgraph(b"tile", 2, full)[0] == bg
    plan.close(); d["pb"].close()


def _md(seq, ref):
    """MD:Z and NM:i of an ungapped read against its reference window."""
    out, run, nm = [], 0, 0
    for a, b in zip(seq, ref):
        if a == b:
            run += 1
        else:
            out.append(b"%d%c" % (run, b)); run = 0; nm += 1
    return b"".join(out) + b"%d" % run, nm


def test_plus_counters_pass_65535_and_the_rule_passes_2_to_32(enc, built):
    """The dataset of test_counters_pass_255_and_65535 with FLAG 16 on every other read -- at 140 000 reads, not its 100 000, of
    which only 50 000 would be forward and no plus plane could pass 65 535 --, and with the alternative
    base taken back to the reference's in 3 of 10 reads at the second of the sites the reads cover, so that the sites' fractions
    differ: the plus planes pass 65 535, nonref * 10^6 passes 2^32, and with F between two sites' fractions exactly the
    expected sites remain.  The expected tables are numpy sums over the SAM records; the container is coded on the device."""
    fa, body = synth.shared_variant_dataset(9, 150, 140_000, 100, site_every=50, err=0.0)
    contig = np.frombuffer(b"".join(fa.split(b"\n")[1:]), dtype=np.uint8)
    cols = [ln.split(b"\t") for ln in body.split(b"\n") if ln]
    start = np.array([int(c[3]) for c in cols], dtype=np.int64)
    seqs = np.frombuffer(b"".join(c[9] for c in cols), dtype=np.uint8).reshape(len(cols), 100).copy()
    at = start[:, None] - 1 + np.arange(100)[None, :]
    sites = np.unique(at[seqs != contig[at]])
    assert len(sites) == 2                                           # the third site lies behind the last read
    idx = np.arange(len(cols))
    for j, s in enumerate(sites.tolist()):
        rows = np.flatnonzero((start - 1 <= s) & (s < start + 99) & (idx % 10 < 3 * j))
        seqs[rows, s - (start[rows] - 1)] = contig[s]
    flag = 16 * (idx & 1)
    lines = []
    for i, c in enumerate(cols):
        md, nm = _md(seqs[i].tobytes(), contig[start[i] - 1:start[i] + 99].tobytes())
        lines.append(b"\t".join([c[0], b"%d" % flag[i]] + c[2:9] + [seqs[i].tobytes(), c[10], b"MD:Z:" + md, b"NM:i:%d" % nm]))
    body = b"\n".join(lines) + b"\n"
    sam = b"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:c\tLN:150\n" + body
    pb = host.pack_sam(sam, fa, block_reads=4096, var_length=True)
    enc.upload_reference(pb.ref)
    _, res, offs, flat = enc.encode_blocks(pb, want_payload_list=False)
    assert (res["status"] == 0).all()
    plan = host.UnpackPlan(pb.container(flat, offs), fa)
    enc.upload_reference(plan.ref)
    zero = np.zeros(150, dtype=np.int64)
    tabs = []
    for keep in (np.ones(len(cols), dtype=bool), flag == 0):
        cnt = np.zeros((5, 150), dtype=np.int64)
        np.add.at(cnt, (pm.klass(seqs[keep]).ravel(), at[keep].ravel()), 1)
        tabs.append((cnt, zero, zero))
    depth, cls = tabs[0][0].sum(axis=0), pm.klass(contig)
    nonref = depth - tabs[0][0][cls, np.arange(150)]
    frac = sorted((int(nonref[s]) * 1_000_000 // int(depth[s]), int(s)) for s in sites.tolist())
    assert frac[0][0] + 1000 < frac[1][0] and all(int(nonref[s]) * 1_000_000 > 2 ** 32 for s in sites.tolist())
    assert max(int(tabs[1][0][:, s].max()) for s in sites.tolist()) > 65_535          # a forward plane
    assert max(int((tabs[0][0] - tabs[1][0])[:, s].max()) for s in sites.tolist()) > 65_535      # and a reverse one
    for ppm, left in ((0, 2), (frac[0][0], 2), (frac[0][0] + 1, 1), (frac[0][0] + 500, 1), (frac[1][0], 1)):
        want, n = psm.text_of(b"c", 1, contig, tabs[0], tabs[1], 1, ppm, True)
        text, nl, kept, res = enc.decode_pileup(plan, by_strand=True, min_alt_ppm=ppm, results=True)
        assert (res["status"] == 0).all() and kept == 140_000
        assert (text, nl) == (want, n) and n == left, ppm
        assert sorted(_pos(text)) == sorted(s + 1 for f, s in frac[2 - left:])
    plan.close(); pb.close()


def test_a_failed_block_contributes_to_neither_strand(enc, data):
    """A flipped payload byte fails its block, and on `mixed` one arena entry per read fails the block of the 40-base deletion:
    the call names the block, and with results=True it reports it and writes what the other blocks show, as the plain call does."""
    plan, pb, reads, names, lens = data["plan"], data["pb"], data["reads"], data["names"], data["lens"]
    enc.upload_reference(plan.ref)
    if data["kind"] == "mixed":
        with pytest.raises(gpu.CbcGpuError, match="max-edits-per-read"):
            enc.decode_pileup(plan, edits_per_read=1, by_strand=True)
        text, lines, kept, pres = enc.decode_pileup(plan, edits_per_read=1, by_strand=True, min_alt_ppm=FRACTIONS[0], results=True)
        bad = tuple(np.flatnonzero(pres["status"] != 0).tolist())
        assert bad and (pres["status"][list(bad)] == 9).all()
        assert (text, lines, kept) == psm.expected(pb, reads, names, lens, ppm=FRACTIONS[0], by_strand=True, skip_blocks=bad)
    pay = plan.payloads.copy()
    hurt = plan.n_blocks // 2
    at = int(plan.blocks[hurt]["in_off"]) + int(plan.blocks[hurt]["in_bytes"]) // 2
    plan.payloads[at] ^= 0x55
    try:
        with pytest.raises(gpu.CbcGpuError, match=r"block %d\b" % hurt):
            enc.decode_pileup(plan, by_strand=True)
        text, lines, kept, pres = enc.decode_pileup(plan, by_strand=True, results=True)
        assert int(pres[hurt]["status"]) != 0 and (np.delete(pres["status"], hurt) == 0).all()
        assert (text, lines, kept) == psm.expected(pb, reads, names, lens, by_strand=True, skip_blocks=(hurt,))
        assert psm.first_eleven(text) == enc.decode_pileup(plan, results=True)[0]
    finally:
        plan.payloads[:] = pay


def test_text_cap_too_small_and_bad_arguments(enc, data):
    """CBC_E_ARG with *text_bytes set when the buffer is one byte short, for the longer line too; min_alt_ppm above 10^6 and
    by_strand above 1 are CBC_E_ARG at the C entry point; 0, 0 writes the bytes of cbc_gpu_decode_pileup."""
    import ctypes
    plan = data["plan"]
    enc.upload_reference(plan.ref)
    c = plan.n_contigs - 1
    name = data["names"][c].decode()
    for bs, ppm in ((True, 0), (False, FRACTIONS[0])):
        want = enc.decode_pileup(plan, name, by_strand=bs, min_alt_ppm=ppm)
        assert len(want) > 1
        with pytest.raises(gpu.CbcGpuError, match="text_cap too small for the pileup text"):
            enc.decode_pileup(plan, name, by_strand=bs, min_alt_ppm=ppm, text_cap=len(want) - 1)
        assert enc.last_pileup_text_bytes == len(want)
        assert enc.decode_pileup(plan, name, by_strand=bs, min_alt_ppm=ppm, text_cap=len(want)) == want
    with pytest.raises(ValueError):
        enc.decode_pileup(plan, min_alt_ppm=1_000_001)
    sel = plan.contig_blocks(c)
    caps, pay, _, _ = enc._plan_args(plan)
    blocks, ws, _ = enc._gather(plan, slice(sel.b0, sel.b1))
    plain = enc.decode_pileup(plan, name)
    for ppm, bs, rc_want in ((1_000_001, 0, -1), (0, 2, -1), (0, 0, 0)):
        text = np.zeros(len(plain) + 1, dtype=np.uint8)
        nb, nl, nk = ctypes.c_uint64(7), ctypes.c_uint64(), ctypes.c_uint64()
        rc = gpu.lib().cbc_gpu_decode_pileup_ext(enc._ctx, pay.ctypes.data, pay.size, blocks.ctypes.data, sel.b1 - sel.b0, ctypes.byref(caps),
                                                 ws.ctypes.data, name.encode(), len(name), sel.beg, sel.end, sel.smax, 0, 1, 0, ppm, bs,
                                                 text.ctypes.data, len(plain), ctypes.byref(nb), ctypes.byref(nl), ctypes.byref(nk), None)
        assert rc == rc_want, (ppm, bs, rc)
        assert text[:nb.value].tobytes() == (plain if rc == 0 else b"")
