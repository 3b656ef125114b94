"""The consensus record without a GPU: the bodies of cbc_gpu_decode_consensus on the lock-step emulation
(tests/consensus_emu, behind the emulated edits decoder of tests/pileup_emu) against consensusmodel.py, byte for byte and counter
for counter; the model against pileupmodel.expected; the host's text bound and no-blocks record; the stand-alone check under
ASan / UBSan; what the CLI decides without a device, its grammar of F held against gpu.alt_frac_ppm.

The datasets are those of tests/test_pileup.py plus consensusmodel.boundary and .deep.  What each is for is asserted on the model's
output (test_datasets_exercise_the_rule): boundary has 6 dropped bases, 3 in tile 0 and 3 in tile 1, 4 positions where the
reference wins a tie and 2 where the order does (all six called at F = 0.5), 6 positions that miss F = 0.75 at depth 8, 150 of
low depth, and E = 8386 = 139 * 60 + 46; deep calls the 3 750 site, leaves the 3 749 site N and writes a two-base code at the
2 500 site under iupac; shared has 396 alt calls and genome 21 or more."""
import os
import subprocess

import numpy as np
import pytest

import consensusmodel as cm
import pileupmodel as pm
from cbc_amd import gpu, host
from test_pileup import _make, _open
from test_pileup_strand import ACCEPTED, REFUSED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "consensus_emu")
DEC_DIR = os.path.join(ROOT, "tests", "pileup_emu")
EXE = os.path.join(ROOT, "cbc_amd", "csrc", "cbc")
B = cm.BOUNDARY


@pytest.fixture(scope="module")
def emu(built):
    """(the emulation of the bodies under test, the emulated edits decoder of tests/pileup_emu)"""
    subprocess.check_call(["make", "-C", EMU_DIR, "libcbc_consensus_emu.so"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", DEC_DIR, "libcbc_pileup_emu.so"], stdout=subprocess.DEVNULL)
    return cm.emu_load(os.path.join(EMU_DIR, "libcbc_consensus_emu.so")), pm.emu_load(os.path.join(DEC_DIR, "libcbc_pileup_emu.so"))


_DATA = {}


def make(kind):
    """The dataset `kind`, made once for the module (tests/test_consensus_gpu.py shares the function, not the cache)."""
    if kind not in _DATA:
        d = _open(*cm.boundary()) if kind == "boundary" else _open(*cm.deep()) if kind == "deep" else _make(kind)
        d["kind"], d["decs"] = kind, {}
        _DATA[kind] = d
    return _DATA[kind]


@pytest.fixture(scope="module")
def datasets(built):
    yield make
    for d in _DATA.values():
        d["plan"].close(); d["pb"].close()
    _DATA.clear()


def _args(d):
    return d["pb"], d["reads"], d["names"], d["lens"]


def _whole(emu, d, n_waves=4, **kw):
    L, Ldec = emu
    return cm.emu_whole(L, Ldec, d["plan"], d["decs"], n_waves=n_waves, **kw)


def test_datasets_exercise_the_rule(datasets):
    """Conditions on the MODEL's output, not measurements of the code under test."""
    d = datasets("boundary")
    pb, reads, names, lens = _args(d)
    assert lens[0] == 2 * 4096 + 200
    cs, _ = cm.calls(pb, reads, 0, 1, lens[0])
    dropped = [i + 1 for i, x in enumerate(cs) if x[1] == "del"]
    assert dropped == [4094, 4095, 4096, 6000, 6001, 6002] and {(p - 1) // 4096 for p in dropped} == {0, 1}
    assert sum(x[3] == "ref" for x in cs) >= 1 and sum(x[3] == "order" for x in cs) >= 1
    cnt, dl, _, _ = pm.tables(reads, 0, 1, lens[0])
    depth = cnt.sum(axis=0) + dl
    assert depth[:B["gap"][0] - 1].min() >= 8 and depth[B["gap"][0] + B["gap"][1] - 1:].min() >= 8
    assert sum(x[1] == "no_call" for x in cs) >= 1 and sum(x[1] == "low_depth" for x in cs) >= 100
    half = cm.calls(pb, reads, 0, 1, lens[0], ppm=500_000)[0]
    assert all(half[p - 1][1:] == ("ref", False, "ref") for p in B["snp_half_ref"])
    assert all(half[p - 1][1] == "alt" and half[p - 1][3] == "order" for p in B["snp_half_two"])
    assert all(cs[p - 1][1] == "alt" for p in B["snp_all"] + B["snp_3of4"])         # 6 of 8 is exactly 0.75
    assert all(cm.calls(pb, reads, 0, 1, lens[0], ppm=750_001)[0][p - 1][1] == "no_call" for p in B["snp_3of4"])
    e = cm.expected(pb, reads, names, lens)[1]
    assert e["emitted"] == lens[0] - 6 and e["emitted"] % 60 != 0 and e["ins_skipped"] >= 1
    d = datasets("deep")
    pb, reads, names, lens = _args(d)
    D = cm.DEEP
    cs, amb = cm.calls(pb, reads, 0, 1, lens[0])[0], cm.calls(pb, reads, 0, 1, lens[0], flags=cm.IUPAC)[0]
    assert cs[D["site_3750"] - 1][1] == "alt" and cs[D["site_3749"] - 1][1] == "no_call" and cs[D["site_2500"] - 1][1] == "no_call"
    assert amb[D["site_2500"] - 1][1] == "ambiguous" and chr(amb[D["site_2500"] - 1][0]) in "RYSWKM"
    assert pm.tables(reads, 0, 60, 60)[3] == 5000
    for kind in ("shared", "genome"):
        assert cm.expected(*_args(datasets(kind)))[1]["alt"] >= 20, kind


@pytest.mark.parametrize("kind", ["shared", "mixed", "genome", "boundary", "deep"])
def test_emulation_matches_the_model_whole_file(emu, datasets, kind):
    """Fails without the feature (the bodies do not exist).  Bytes, the eight counters, the reads kept."""
    d = datasets(kind)
    assert _whole(emu, d) == cm.expected(*_args(d))


def test_emulation_matches_the_model_option_sets(emu, datasets):
    """boundary under every line width, flag and threshold of the issue's list, one and four wavefronts in the events pass; the
    thresholds and masks again on shared."""
    d = datasets("boundary")
    for width in (1, 7, 60, 64, 65535):
        assert _whole(emu, d, width=width) == cm.expected(*_args(d), width=width), width
    for flags in (cm.SHOW_DEL, cm.FILL_REF, cm.IUPAC, cm.SHOW_DEL | cm.FILL_REF | cm.IUPAC):
        assert _whole(emu, d, flags=flags) == cm.expected(*_args(d), flags=flags), flags
    i = 0
    for kind in ("boundary", "shared"):
        d = datasets(kind)
        for min_depth in (1, 4):
            for ppm in (500_000, 750_000, 1_000_000):
                for ex in (0, 16):
                    i += 1
                    flags, waves = (0, cm.IUPAC, cm.SHOW_DEL | cm.FILL_REF)[i % 3], (1, 4)[(i // 2 + (min_depth == 4)) & 1]   # both wave counts under both masks
                    kw = dict(exclude=ex, min_depth=min_depth, ppm=ppm, flags=flags)
                    assert _whole(emu, d, n_waves=waves, **kw) == cm.expected(*_args(d), **kw), (kind, kw, waves)
    d = datasets("deep")
    for kw in (dict(flags=cm.IUPAC), dict(ppm=749_800), dict(ppm=750_000, exclude=16, min_depth=4)):
        assert _whole(emu, d, n_waves=1, **kw) == cm.expected(*_args(d), **kw), kw


def _special_windows(d):
    """boundary: inside the shared deletion, ending on 4096, beginning on 4097, and two whose E is the width and twice the width"""
    return [(0, 4094, 4096, 60, 0), (0, 4095, 4095, 60, cm.SHOW_DEL), (0, 3000, 4096, 60, 0), (0, 4097, 5000, 60, 0), (0, 1, 4096, 7, cm.IUPAC),
            (0, 101, 160, 60, 0), (0, 101, 220, 60, 0), (0, 4090, 4100, 8, 0), (0, 4090, 4105, 8, cm.SHOW_DEL), (0, 6990, 7160, 64, cm.FILL_REF)]


def test_windows(emu, datasets):
    """Regions carry their range in the header; newline placement, no trailing empty line, the header alone when E = 0."""
    L, Ldec = emu
    for kind in ("shared", "boundary"):
        d = datasets(kind)
        plan, pb, reads, names, lens = d["plan"], *_args(d)
        wins = [(c, beg, end, (60, 7, 1)[i % 3], (0, cm.IUPAC, cm.SHOW_DEL)[i % 3]) for i, (_, c, beg, end) in enumerate(pm.windows(pb, reads, lens, 8, 2))]
        for i, (c, beg, end, width, flags) in enumerate(wins + (_special_windows(d) if kind == "boundary" else [])):
            sel = plan.region("%s:%d-%d" % (names[c].decode(), beg, end))
            rc, t, cnt, kept, total = cm.emu_call(L, Ldec, plan, sel, True, width=width, flags=flags, n_waves=1 + 3 * (i & 1))
            want = cm.expected(pb, reads, names, lens, (c, beg, end), width=width, flags=flags)
            assert rc == 0 and (t, cnt, kept) == want and total == len(t), (kind, beg, end, width, flags)
            hdr, body = cm.body_of(t)
            assert hdr == b">%s:%d-%d" % (names[c], beg, end) and len(body) == cnt["emitted"]
            assert len(t) == len(hdr) + 1 + len(body) + -(-len(body) // width)
    d = datasets("boundary")
    exp = lambda beg, end, width, flags=0: cm.expected(*_args(d), (0, beg, end), width=width, flags=flags)
    assert exp(4094, 4096, 60)[0] == b">bnd:4094-4096\n" and exp(4094, 4096, 60)[1]["emitted"] == 0
    assert exp(101, 160, 60)[0].count(b"\n") == 2 and exp(101, 220, 60)[0].count(b"\n") == 3      # E = the width, twice the width
    assert exp(4090, 4100, 8)[1]["emitted"] == 8 and exp(4090, 4105, 8, cm.SHOW_DEL)[1]["emitted"] == 16


def test_failed_block_contributes_nothing(emu, datasets):
    L, Ldec = emu
    for kind in ("shared", "boundary"):
        d = datasets(kind)
        plan, pb, reads, names, lens = d["plan"], *_args(d)
        sel = plan.contig_blocks(0)
        assert sel.b1 - sel.b0 >= 3
        rc, t, cnt, kept, _ = cm.emu_call(L, Ldec, plan, sel, False, fail_blocks=(1,), dec=d["decs"].get(0))
        want = cm.expected(pb, reads, names, lens, skip_blocks=(sel.b0 + 1,))
        assert rc == -4 and (t, cnt, kept) == want
        assert t != cm.expected(pb, reads, names, lens)[0]


def test_model_against_the_pileup_model(datasets):
    """Code not under test: with show-del the body has one byte per position, and wherever the model's letter is not the
    upper-cased reference base, pileupmodel.expected(min_alt=1) has a line."""
    for kind in ("shared", "mixed", "genome", "boundary"):
        pb, reads, names, lens = _args(datasets(kind))
        for c in range(len(names)):
            for beg, end in ((1, lens[c]), (max(1, lens[c] // 3), min(lens[c], lens[c] // 3 + 700))):
                t = cm.expected(pb, reads, names, lens, (c, beg, end), flags=cm.SHOW_DEL)[0]
                body = np.frombuffer(cm.body_of(t)[1], dtype=np.uint8)
                assert len(body) == end - beg + 1
                ref = pm.contig_ref(pb, c)[beg - 1:end]
                up = np.where(pm.klass(ref) < 4, ref & 0xDF, ord("N"))
                differs = set((np.flatnonzero(body != up) + beg).tolist())
                lines = {r[1] for r in pm.parse(pm.expected(pb, reads, names, lens, (c, beg, end), 0, 1)[0])}
                cnt, dl, _, _ = pm.tables(reads, c, beg, end)
                covered = set((np.flatnonzero(cnt.sum(axis=0) + dl > 0) + beg).tolist())
                assert differs & covered <= lines, (kind, c, sorted(differs & covered - lines)[:5])
                assert all(body[p - beg] == ord("N") for p in differs - covered)


def test_text_bound_and_the_no_blocks_record(datasets):
    """cbc_unpack_consensus_text_cap = header + w + ceil(w / W): the text's size with show-del, a bound without; the host's
    record of a window without blocks equals the model's, with fill-ref and without."""
    for kind in ("boundary", "genome"):
        d = datasets(kind)
        plan, pb, reads, names, lens = d["plan"], *_args(d)
        for c in range(len(names)):
            for width in (1, 60, 65535):
                for rng in (False, True):
                    beg, end = (7, lens[c] - 5) if rng else (1, lens[c])
                    cap = plan.consensus_text_cap(c, beg, end, width, rng)
                    hdr = len(names[c]) + 2 + (2 + len(str(beg)) + len(str(end)) if rng else 0)
                    assert cap == hdr + (end - beg + 1) + -(-(end - beg + 1) // width)
                    if width == 60:
                        texts = [cm.expected(pb, reads, names, lens, (c, beg, end), flags=f, with_range=rng)[0] for f in (cm.SHOW_DEL, 0)]
                        assert len(texts[0]) == cap and len(texts[1]) <= cap
    d = datasets("boundary")
    plan, pb, reads, names, lens = d["plan"], *_args(d)
    assert len(cm.expected(pb, reads, names, lens)[0]) < plan.consensus_text_cap(0, 1, lens[0])
    cap_c = host.lib().cbc_unpack_consensus_text_cap
    assert cap_c(plan._ptr, 1, 1, 10, 60, 0) == 0 and cap_c(plan._ptr, 0, 0, 10, 60, 0) == 0 and cap_c(plan._ptr, 0, 5, 4, 60, 0) == 0
    assert cap_c(plan._ptr, 0, 1, 2 ** 31, 60, 0) == 0 and cap_c(plan._ptr, 0, 1, 10, 0, 0) == 0 and cap_c(plan._ptr, 0, 1, 10, 65536, 0) == 0
    assert cap_c(plan._ptr, 0, 1, 10, 60, 2) == 0
    g0, g1 = B["gap"][0] + 20, B["gap"][0] + 120                    # inside the uncovered stretch: no block is selected?  either way
    for flags in (0, cm.FILL_REF, cm.FILL_REF | cm.SHOW_DEL | cm.IUPAC):
        for rng, (beg, end) in ((True, (g0, g1)), (False, (1, lens[0]))):
            o = host.ConsensusOpts(9, 750_000, 7, flags)             # min_depth above every depth: the whole contig is low depth
            text, cnt = plan.consensus_empty(0, beg, end, o, rng)
            want = cm.expected(pb, reads, names, lens, (0, beg, end) if rng else None, min_depth=9, width=7, flags=flags)
            assert (text, cnt) == want[:2], (flags, rng)
    g = datasets("genome")                                          # a later contig: its reference offset is the sum over those in front
    gplan, gpb, greads, gnames, glens = g["plan"], *_args(g)
    assert len(gnames) >= 2
    c = len(gnames) - 1
    for rng, (beg, end) in ((True, (glens[c] // 2, glens[c] // 2 + 333)), (False, (1, glens[c]))):
        text, cnt = gplan.consensus_empty(c, beg, end, host.ConsensusOpts(10 ** 6, 750_000, 60, cm.FILL_REF), rng)
        want = cm.expected(gpb, greads, gnames, glens, (c, beg, end), min_depth=10 ** 6, flags=cm.FILL_REF, with_range=rng)
        assert (text, cnt) == want[:2] and cm.body_of(text)[1] == pm.contig_ref(gpb, c)[beg - 1:end].tobytes().lower(), rng
    assert pm.contig_ref(gpb, c)[:glens[c]].tobytes() != pm.contig_ref(gpb, 0)[:glens[c]].tobytes()
    with pytest.raises(ValueError):
        plan.consensus_empty(0, 1, 10, host.ConsensusOpts(0, 750_000, 60, 0))
    with pytest.raises(ValueError):
        plan.consensus_empty(0, 1, 10, host.ConsensusOpts(1, 750_000, 60, 8))


def test_sanitizer_build_of_the_stand_alone_check(built):
    """consensus_emu_check: the fabricated reads of tests/pileup_emu's check through the emulated bodies -- every line-width path
    (1, 2..63, 64 and more), the eight flag sets, a failed block, a window inside a shared deletion, a 255-byte name at the last
    position of the coordinate, text_cap one byte short -- against the rule in a host loop, in a program of its own under
    AddressSanitizer / UBSan, every table at its exact size; it exits non-zero on a finding or a mismatch."""
    subprocess.check_call(["make", "-C", EMU_DIR, "consensus_emu_check"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(EMU_DIR, "consensus_emu_check")], capture_output=True, text=True)
    assert r.returncode == 0 and "CONSENSUS EMU CHECK OK" in r.stdout and "MISMATCH" not in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- the CLI where no device is needed -----------------------------------------------------------------------------------------
def _cli(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def test_cli_refusals_and_grammar(built, datasets, tmp_path):
    """Every refusal names its option and exits 1; the grammar of F is gpu.alt_frac_ppm's: the CLI refuses exactly the strings
    that function raises on."""
    d = datasets("mixed")
    (tmp_path / "in.cbc").write_bytes(d["blob"]); (tmp_path / "ref.fa").write_bytes(d["fa"])
    files = (tmp_path / "in.cbc", tmp_path / "o.fa", tmp_path / "ref.fa")
    for args, msg in [(("--call-min-depth", "2"), "cbc: --call-min-depth applies to --consensus\n"),
                      (("--call-frac", "0.5"), "cbc: --call-frac applies to --consensus\n"),
                      (("--line-width", "70"), "cbc: --line-width applies to --consensus\n"),
                      (("--show-del",), "cbc: --show-del applies to --consensus\n"),
                      (("--fill-ref",), "cbc: --fill-ref applies to --consensus\n"),
                      (("--iupac",), "cbc: --iupac applies to --consensus\n"),
                      (("--pileup", "--iupac"), "cbc: --iupac applies to --consensus\n"),
                      (("--consensus", "--sam"), "--consensus, --pileup"), (("--consensus", "--depth"), "--consensus, --pileup"),
                      (("--consensus", "--bedcov"), "--consensus, --pileup"), (("--consensus", "--depth-hist"), "--consensus, --pileup"),
                      (("--consensus", "--stats"), "--consensus, --pileup"), (("--consensus", "--pileup"), "--consensus, --pileup"),
                      (("--consensus", "--sam", "--cigar"), "--consensus, --pileup"),
                      (("--consensus", "--skip-deletions"), "--skip-deletions applies to --depth"),
                      (("--consensus", "--region", "chr1", "--region", "chr2"), "cbc: --consensus takes at most one --region and no --regions-file\n"),
                      (("--consensus", "--regions-file", "x.bed"), "cbc: --consensus takes at most one --region and no --regions-file\n"),
                      (("--consensus", "--devices", "0,1"), "cbc: --consensus decodes on one device"),
                      (("--consensus", "--min-alt", "2"), "cbc: --min-alt applies to --pileup\n"),
                      (("--consensus", "--call-min-depth", "0"), "cbc: --call-min-depth wants"), (("--consensus", "--call-min-depth", "x"), "cbc: --call-min-depth wants"),
                      (("--consensus", "--line-width", "0"), "cbc: --line-width wants"), (("--consensus", "--line-width", "65536"), "cbc: --line-width wants"),
                      (("--consensus", "--line-width", "6x"), "cbc: --line-width wants")]:
        r = _cli("-x", *files, *args)
        assert r.returncode == 1 and (r.stderr == msg if msg.endswith("\n") else msg in r.stderr), (args, r.stderr)
    r = _cli("-c", tmp_path / "ref.fa", tmp_path / "o.cbc", tmp_path / "ref.fa", "--consensus")
    assert r.returncode == 1 and r.stderr == "cbc: --consensus applies to decompression (-d / -x)\n"
    (tmp_path / "compat.cbc").write_bytes(b"not a block container")
    r = _cli("-x", tmp_path / "compat.cbc", tmp_path / "o.fa", tmp_path / "ref.fa", "--consensus")
    assert r.returncode == 1 and "--consensus needs a block container" in r.stderr
    # a long-read container: the refusal of cbc_unpack_sam_header, in the binary and in the binding
    from oracle import oracle
    pb, _, lfa = host.synth_long(5, 200_000, 40, read_len=2000, want_text=True)
    flat, offs, _ = oracle.cpu_encode_blocks(pb, long_reads=True, return_flat=True)
    lblob = pb.container(flat, offs)
    (tmp_path / "l.cbc").write_bytes(lblob); (tmp_path / "l.fa").write_bytes(lfa)
    pb.close()
    for extra in ((), ("--region", "chrL:1-500")):
        r = _cli("-x", tmp_path / "l.cbc", tmp_path / "o.fa", tmp_path / "l.fa", "--consensus", *extra)
        assert r.returncode == 1 and "--consensus" in r.stderr and "long-read" in r.stderr, r.stderr
    lplan = host.UnpackPlan(lblob, lfa)
    for region in (None, "chrL:1-500"):
        with pytest.raises(host.CbcInputError, match="long-read"):
            gpu.Encoder.decode_consensus(None, lplan, region)     # refused before the context is touched: no device needed
    lplan.close()
    first = min(r["pos"] for r in d["reads"] if r["contig"] == 0)
    assert first > 3
    empty = ("--consensus", "--region", "chr1:2-%d" % (first - 1))
    for s in REFUSED:
        with pytest.raises(ValueError):
            gpu.alt_frac_ppm(s)
        r = _cli("-x", *files, *empty, "--call-frac", s)
        assert r.returncode == 1 and r.stderr.startswith("cbc: --call-frac wants"), (s, r.stderr)
    want = b">chr1:2-%d\n" % (first - 1) + b"".join(b"N" * min(60, first - 2 - i) + b"\n" for i in range(0, first - 2, 60))
    for s in ACCEPTED:
        gpu.alt_frac_ppm(s)
        r = _cli("-x", *files, *empty, "--call-frac", s, "--verbose")
        assert r.returncode == 0 and (tmp_path / "o.fa").read_bytes() == want, (s, r.stdout + r.stderr)
        assert "consensus: %d bases (0 ref, 0 alt, 0 deleted, 0 ambiguous, %d low depth, 0 no call; 0 insertions not applied) from 0 reads in 0 blocks\n" % (
            first - 2, first - 2) in r.stdout and "kernels:" not in r.stdout
    u = _cli("-h")
    for o in ("--consensus", "--call-min-depth", "--call-frac", "--line-width", "--show-del", "--fill-ref", "--iupac"):
        assert o in u.stdout + u.stderr, o


def test_cli_contig_without_blocks_is_written_on_the_host(built, tmp_path):
    """A container whose only contig has no blocks (the packer writes none; this one is laid out by hand: the 36-byte header,
    the name, one contig-table entry, no block index, no payload): the record comes from cbc_unpack_consensus_empty, with
    fill-ref the reference in lower case; no device is opened (no kernel line under --verbose)."""
    import struct
    import synth
    contig = synth.make_contig(np.random.default_rng(3), 130)
    fa = synth.fasta_text([("solo", contig)])
    blob = struct.pack("<9I", 0x42434243, 2, 100, 1, 0, 5, 64, 64, 100) + b"solo\0\0\0\0" + struct.pack("<IIQ", 0, 0, 130)
    (tmp_path / "in.cbc").write_bytes(blob); (tmp_path / "ref.fa").write_bytes(fa)
    plan = host.UnpackPlan(blob, fa)
    assert (plan.n_contigs, plan.n_blocks) == (1, 0)
    sel = plan.contig_blocks(0)
    assert (sel.b0, sel.b1, sel.beg, sel.end) == (0, 0, 1, 130)
    plan.close()
    for extra, body, width in (((), b"N" * 130, 60), (("--fill-ref", "--line-width", "50"), contig.tobytes().lower(), 50)):
        r = _cli("-x", tmp_path / "in.cbc", tmp_path / "o.fa", tmp_path / "ref.fa", "--consensus", "--verbose", *extra)
        assert r.returncode == 0 and (tmp_path / "o.fa").read_bytes() == cm.record(b"solo", 1, 130, body, width), r.stdout + r.stderr
        assert "kernels:" not in r.stdout and "consensus: 130 bases (0 ref, 0 alt, 0 deleted, 0 ambiguous, 130 low depth, 0 no call; " \
            "0 insertions not applied) from 0 reads in 0 blocks\n" in r.stdout
    r = _cli("-x", tmp_path / "in.cbc", tmp_path / "o.fa", tmp_path / "ref.fa", "--consensus", "--region", "solo:11-20", "--fill-ref")
    assert r.returncode == 0 and (tmp_path / "o.fa").read_bytes() == b">solo:11-20\n" + contig[10:20].tobytes().lower() + b"\n"


def test_exports_headers_and_docs(built):
    assert "cbc_gpu_decode_consensus" in gpu.EXPORTS and "cbc_gpu_last_consensus_ms" in gpu.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "cbc_gpu.h")).read()
    assert "cbc_gpu_decode_consensus(" in hdr and "CBC_CONS_IUPAC" in hdr and gpu.lib().cbc_gpu_abi_version() == 1
    hh = open(os.path.join(ROOT, "include", "cbc_host.h")).read()
    assert "cbc_unpack_consensus_text_cap(" in hh and "cbc_unpack_consensus_empty(" in hh
    for name in ("README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, name)).read()
        assert "--consensus" in text and "--call-frac" in text, name
    assert "4.25" in open(os.path.join(ROOT, "DESIGN.md")).read()
