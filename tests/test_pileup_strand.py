"""Per-strand counts and the minimum alternative fraction of the pileup without a GPU: the bodies of
cbc_gpu_decode_pileup_ext on the lock-step emulation (tests/pileup_strand_emu) against pileupstrandmodel.py; the stand-alone
check under ASan / UBSan; cbc_unpack_pileup_ext_text_cap; what the CLI decides without a device, and its grammar of F held
against gpu.alt_frac_ppm.

The datasets are those of tests/test_pileup.py.  What the by-strand tests rely on is asserted: at least 20 % of the kept reads on
each strand, and at least 20 reported positions where both strands show a non-reference observation -- except that `mixed` (600
reads here, 1200 on the GPU) has both strands but only 3 (10) such positions, its coverage being thin; it is kept as a dataset
and held to one such position.  The fractions 0.3 and 0.5 were chosen from the model: on each of these datasets the rule keeps
and drops at least 10 % of the lines of the call without it (0.02 and 0.2 drop under 10 % at this depth, 1 keeps under 10 % of
`mixed`)."""
import os
import subprocess

import pytest

import pileupmodel as pm
import pileupstrandmodel as psm
from cbc_amd import gpu
from test_pileup import _make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "pileup_strand_emu")
DEC_DIR = os.path.join(ROOT, "tests", "pileup_emu")
EXE = os.path.join(ROOT, "cbc_amd", "csrc", "cbc")
FRACTIONS = (300_000, 500_000)
MIN_BOTH = {"shared": 20, "mixed": 1, "genome": 20}


@pytest.fixture(scope="module")
def emu(built):
    """(the emulation of the bodies under test, the emulated edits decoder of tests/pileup_emu)"""
    subprocess.check_call(["make", "-C", EMU_DIR, "libcbc_pileup_strand_emu.so"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", DEC_DIR, "libcbc_pileup_emu.so"], stdout=subprocess.DEVNULL)
    return psm.emu_load(os.path.join(EMU_DIR, "libcbc_pileup_strand_emu.so")), pm.emu_load(os.path.join(DEC_DIR, "libcbc_pileup_emu.so"))


@pytest.fixture(scope="module", params=["shared", "mixed", "genome"])
def data(request, built):
    d = _make(request.param)
    d["kind"] = request.param
    d["decs"] = {}
    yield d
    d["plan"].close(); d["pb"].close()


def test_emulation_matches_the_model(emu, data):
    """Fails without the feature (the bodies do not exist): by_strand with and without a fraction, a fraction alone, exclusion
    masks 4 and 16, the whole file and the windows of pileupmodel.windows."""
    L, Ldec = emu
    plan, pb, reads, names, lens = data["plan"], data["pb"], data["reads"], data["names"], data["lens"]
    psm.assert_both_strands(pb, reads, names, lens, min_both=MIN_BOTH[data["kind"]])
    base = psm.expected(pb, reads, names, lens)[1]
    for ppm in FRACTIONS:
        n = psm.expected(pb, reads, names, lens, ppm=ppm)[1]
        assert 0.1 * base <= n <= 0.9 * base, (ppm, n, base)
    for bs, ppm, ex, k in ((True, 0, 0, 1), (True, FRACTIONS[0], 0, 1), (False, FRACTIONS[1], 0, 1), (True, 0, 4, 1), (True, 0, 16, 2),
                           (True, FRACTIONS[1], 16, 1), (False, FRACTIONS[0], 4, 2), (False, 0, 0, 1)):
        want = psm.expected(pb, reads, names, lens, None, ex, k, ppm, bs)
        assert psm.emu_whole(L, Ldec, plan, ex, k, ppm, bs, data["decs"]) == want, (bs, ppm, ex, k)
    assert psm.expected(pb, reads, names, lens, by_strand=False) == pm.expected(pb, reads, names, lens)
    for i, (s, c, beg, end) in enumerate(pm.windows(pb, reads, lens, 8, 2)):
        ppm, k = (0, FRACTIONS[0], FRACTIONS[1])[i % 3], 1 + (i % 4 == 3)
        sel = plan.region(s)
        rc, t, n, kept, _ = psm.emu_call(L, Ldec, plan, sel, 0, k, ppm, True, n_waves=1 + 3 * (i & 1))
        assert rc == 0 and (t, n, kept) == psm.expected(pb, reads, names, lens, (c, beg, end), 0, k, ppm, True), (s, k, ppm)


def test_plus_columns_against_the_plain_model(data):
    """The model itself: the first eleven columns are pileupmodel's text, X+ <= X, and under exclusion mask 16 every X+ is X."""
    pb, reads, names, lens = data["pb"], data["reads"], data["names"], data["lens"]
    text = psm.expected(pb, reads, names, lens, by_strand=True)[0]
    assert psm.first_eleven(text) == pm.expected(pb, reads, names, lens)[0]
    rows = psm.parse(text)
    assert all(r[11 + j] <= r[4 + j] for r in rows for j in range(7))
    assert all(r[11:] == r[4:11] for r in psm.parse(psm.expected(pb, reads, names, lens, exclude=16, by_strand=True)[0]))
    assert any(r[11:] != r[4:11] for r in rows)


def test_failed_block_contributes_to_neither_strand(emu, data):
    L, Ldec = emu
    plan, pb, reads, names, lens = data["plan"], data["pb"], data["reads"], data["names"], data["lens"]
    sel = plan.contig_blocks(0)
    assert sel.b1 - sel.b0 >= 2
    rc, t, n, kept, _ = psm.emu_call(L, Ldec, plan, sel, by_strand=True, fail_blocks=(1,), dec=data["decs"].get(0))
    want = psm.expected(pb, reads, names, lens, (0, 1, lens[0]), by_strand=True, skip_blocks=(sel.b0 + 1,))
    assert rc == -4 and (t, n, kept) == want
    assert t != psm.expected(pb, reads, names, lens, (0, 1, lens[0]), by_strand=True)[0]


def test_text_cap(emu, data):
    """cbc_unpack_pileup_ext_text_cap: len(name) + 102 + 7 * 11 bytes a line with by_strand, the plain bound without; the
    emulated call one byte short reports the size and writes nothing."""
    L, Ldec = emu
    plan, pb, reads, names, lens = data["plan"], data["pb"], data["reads"], data["names"], data["lens"]
    for c in range(plan.n_contigs):
        sel = plan.contig_blocks(c)
        k = int(plan.blocks[sel.b0:sel.b1]["n_reads"].sum())
        cap = plan.pileup_text_cap(sel.b0, sel.b1, c, sel.beg, sel.end, sel.smax, by_strand=True)
        assert cap == min(lens[c], k * sel.smax) * (len(names[c]) + 102 + 77)
        assert plan.pileup_text_cap(sel.b0, sel.b1, c, sel.beg, sel.end, sel.smax, by_strand=False) == \
            plan.pileup_text_cap(sel.b0, sel.b1, c, sel.beg, sel.end, sel.smax) == min(lens[c], k * sel.smax) * (len(names[c]) + 102)
        text = psm.expected(pb, reads, names, lens, (c, 1, lens[c]), by_strand=True)[0]
        assert len(text) <= cap and max((len(x) for x in text.split(b"\n")), default=0) + 1 <= len(names[c]) + 179
    from cbc_amd import host
    cap_c = host.lib().cbc_unpack_pileup_ext_text_cap
    assert cap_c(plan._ptr, 0, 1, 0, 1, 10, 100, 2) == 0 and cap_c(plan._ptr, 0, plan.n_blocks + 1, 0, 1, 10, 100, 1) == 0
    assert cap_c(plan._ptr, 0, 1, 0, 0, 10, 100, 1) == 0 and cap_c(plan._ptr, 0, 1, 0, 1, 2 ** 31, 100, 1) == 0
    line = b"%s\t%d\tN" % (names[0], 2 ** 31 - 1) + b"\t4294967295" * 15 + b"\n"          # ten digits in every number
    assert len(line) == len(names[0]) + 179
    sel = plan.contig_blocks(0)
    want = psm.expected(pb, reads, names, lens, (0, 1, lens[0]), by_strand=True)[0]
    rc, t, n, kept, total = psm.emu_call(L, Ldec, plan, sel, by_strand=True, cap=len(want) - 1, dec=data["decs"].get(0))
    assert rc == -1 and total == len(want) and t == b""
    assert psm.emu_call(L, Ldec, plan, sel, by_strand=True, cap=len(want), dec=data["decs"].get(0))[1] == want


def test_sanitizer_build_of_the_stand_alone_check(built):
    """pileup_strand_emu_check: the fabricated cases of tests/pileup_emu's check with forward, reverse and mixed strands, the
    fraction rule at equality and one below it (1 of 20 at 0.05 and at 0.050001), a position with ins > depth, text_cap one byte
    short of every text, and the longest line (a 255-byte name, sixteen ten-digit numbers), in a program of its own under
    AddressSanitizer / UBSan, every table at its exact size; it exits non-zero on a finding or a mismatch."""
    subprocess.check_call(["make", "-C", EMU_DIR, "pileup_strand_emu_check"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(EMU_DIR, "pileup_strand_emu_check")], capture_output=True, text=True)
    assert r.returncode == 0 and "PILEUP STRAND EMU CHECK OK" in r.stdout and "MISMATCH" not in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    assert "300 cases over the three strand settings" in r.stdout


# ---- the CLI where no device is needed -----------------------------------------------------------------------------------------
def _cli(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


REFUSED = ["", "x", "0", "0.0", ".5", "1.000001", "1.5", "-0.1", "1e-3", "0.1234567", "0.", "1.", "0x1", " 0.5", "0.5 ", "+0.5", "0,5", "2",
           "00.0000000", "0.0000001", "١"]
ACCEPTED = {"0.000001": 1, "1": 1_000_000, "1.0": 1_000_000, "1.000000": 1_000_000, "0.02": 20_000, "0.2": 200_000, "0.5": 500_000,
            "0.050001": 50_001, "0.07": 70_000, "0.999999": 999_999, "00.5": 500_000, "01": 1_000_000, "0.123456": 123_456}


def test_alt_frac_ppm():
    for s, ppm in ACCEPTED.items():
        assert gpu.alt_frac_ppm(s) == ppm, s
    for s in REFUSED + ["0.5\n"]:
        with pytest.raises(ValueError):
            gpu.alt_frac_ppm(s)
    with pytest.raises(ValueError):
        gpu.alt_frac_ppm(0.5)


def test_cli_refusals_and_grammar(built, tmp_path):
    """The owner refusals in the CLI's existing form and order, and the grammar of F: the CLI refuses, with a message that names
    the option and status 1, exactly the strings gpu.alt_frac_ppm raises on; an accepted F with a window that selects no block
    ends with status 0 and an empty file without a device."""
    d = _make("mixed")
    (tmp_path / "in.cbc").write_bytes(d["blob"]); (tmp_path / "ref.fa").write_bytes(d["fa"])
    files = (tmp_path / "in.cbc", tmp_path / "o.txt", tmp_path / "ref.fa")
    for args, msg in [(("--by-strand",), "cbc: --by-strand applies to --pileup\n"),
                      (("--min-alt-frac", "0.02"), "cbc: --min-alt-frac applies to --pileup\n"),
                      (("--by-strand", "--min-alt-frac", "0.02"), "cbc: --by-strand applies to --pileup\n"),
                      (("--min-alt", "2", "--by-strand"), "cbc: --min-alt applies to --pileup\n"),
                      (("--max-edits-per-read", "4", "--min-alt-frac", "0.5"), "cbc: --max-edits-per-read applies to --pileup\n"),
                      (("--depth", "--by-strand"), "cbc: --by-strand applies to --pileup\n"),
                      (("--sam", "--cigar", "--max-edits-per-read", "4", "--min-alt-frac", "0.5"), "cbc: --min-alt-frac applies to --pileup\n"),
                      (("--pileup", "--by-strand", "--sam"), "different outputs"),
                      (("--pileup", "--by-strand", "--devices", "0,1"), "one device"),
                      (("--pileup", "--min-alt-frac", "0.02", "--region", "chr1", "--region", "chr2"), "at most one --region"),
                      (("--pileup", "--by-strand", "--regions-file", "x.bed"), "at most one --region"),
                      (("--pileup", "--by-strand", "--skip-deletions"), "--skip-deletions applies to --depth")]:
        r = _cli("-x", *files, *args)
        assert r.returncode == 1 and (r.stderr == msg if msg.endswith("\n") else msg in r.stderr), (args, r.stderr)
    for args, msg in [(("--pileup", "--by-strand"), "cbc: --pileup applies to decompression (-d / -x)\n"),
                      (("--pileup", "--min-alt-frac", "0.1"), "cbc: --pileup applies to decompression (-d / -x)\n"),
                      (("--by-strand",), "cbc: --by-strand applies to --pileup\n")]:
        r = _cli("-c", tmp_path / "ref.fa", tmp_path / "o.cbc", tmp_path / "ref.fa", *args)
        assert r.returncode == 1 and r.stderr == msg, (args, r.stderr)
    first = min(r["pos"] for r in d["reads"] if r["contig"] == 0)
    assert first > 1
    empty = ("--pileup", "--region", "chr1:1-%d" % (first - 1))
    for s in REFUSED:
        with pytest.raises(ValueError):
            gpu.alt_frac_ppm(s)
        r = _cli("-x", *files, *empty, "--min-alt-frac", s)
        assert r.returncode == 1 and r.stderr.startswith("cbc: --min-alt-frac wants"), (s, r.stderr)
    for s in ACCEPTED:
        gpu.alt_frac_ppm(s)
        (tmp_path / "o.txt").write_bytes(b"x")
        r = _cli("-x", *files, *empty, "--min-alt-frac", s, "--by-strand", "--verbose")
        assert r.returncode == 0 and (tmp_path / "o.txt").read_bytes() == b"" and "0 positions from 0 reads in 0 of" in r.stdout, (s, r.stdout + r.stderr)
        assert "kernels:" not in r.stdout
    r = _cli("-h")
    assert "--by-strand" in r.stdout + r.stderr and "--min-alt-frac" in r.stdout + r.stderr
    d["plan"].close(); d["pb"].close()


def test_exports_and_headers(built):
    assert "cbc_gpu_decode_pileup_ext" in gpu.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "cbc_gpu.h")).read()
    assert "cbc_gpu_decode_pileup_ext(" in hdr and "cbc_gpu_decode_pileup(" in hdr and gpu.lib().cbc_gpu_abi_version() == 1
    assert "cbc_unpack_pileup_ext_text_cap(" in open(os.path.join(ROOT, "include", "cbc_host.h")).read()
    for name in ("README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, name)).read()
        assert "--by-strand" in text and "--min-alt-frac" in text, name
