"""CIGAR, NM and MD in the SAM output without a GPU: the edit-reporting decoder and the measure, count
and write bodies of cbc_cigar_body.h on the lock-step emulation (tests/cigar_emu) against the two models of cigarmodel.py and
the check that needs no model; the stand-alone check under ASan / UBSan; cbc_unpack_sam_cigar_text_cap; and what the CLI decides
without a device."""
import os
import re
import subprocess

import numpy as np
import pytest

import cigarmodel as cm
import pileupmodel as pm
import regionmodel as rm
import synth
from cbc_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "cigar_emu")
EXE = os.path.join(ROOT, "cbc_amd", "csrc", "cbc")


@pytest.fixture(scope="module")
def emu(built):
    subprocess.check_call(["make", "-C", EMU_DIR, "libcbc_cigar_emu.so"], stdout=subprocess.DEVNULL)
    return cm.emu_load(os.path.join(EMU_DIR, "libcbc_cigar_emu.so"))


@pytest.fixture(scope="module")
def indel(built):
    d = cm.indel_dataset()
    d["plan"] = host.UnpackPlan(d["blob"], d["fa"])
    d["reads"], d["tags"] = cm.assert_models_agree(d["pb"], d["sam"], d["names"])      # (a) == (b) before either stands
    yield d
    d["plan"].close(); d["pb"].close()


def test_the_dataset_holds_every_kind_of_line(indel):
    recs = [r for _, _, rs in indel["rbc"] for r in rs]
    mism = [len(re.sub(r"\^[A-Z]+", "", r["md"]).translate({ord(c): None for c in "0123456789"})) for r in recs]
    kinds = dict(perfect=sum(r["cigar"] == "150M" and m == 0 for r, m in zip(recs, mism)),
                 snp_only=sum(r["cigar"] == "150M" and m > 0 for r, m in zip(recs, mism)),
                 ins=sum("I" in r["cigar"] for r in recs), dele=sum("D" in r["cigar"] for r in recs),
                 clip=sum("S" in r["cigar"] for r in recs),
                 clip_indel=sum("S" in r["cigar"] and ("I" in r["cigar"] or "D" in r["cigar"]) for r in recs),
                 indel_snp=sum(("I" in r["cigar"] or "D" in r["cigar"]) and m > 0 for r, m in zip(recs, mism)))
    assert all(v >= 50 for v in kinds.values()), kinds
    assert cm.tags_b(indel["sam"], indel["pb"], indel["names"])[1] <= 5         # the normalisation cannot hide a failure
    got = {t[0] for t in indel["tags"]}
    assert "150M" in got and any("I" in g for g in got) and any("D" in g for g in got) and any(g.endswith("S") for g in got)


def test_emulation_matches_the_models(emu, indel):
    plan, pb, reads, tags, names, lens = indel["plan"], indel["pb"], indel["reads"], indel["tags"], indel["names"], indel["lens"]
    want, n = cm.expected(pb, reads, names, tags)
    for waves in (1, 4):
        rc, text, nr, total = cm.emu_call(emu, plan, n_waves=waves)
        assert rc == 0 and nr == n == pb.n_recs and text == want, waves
    assert cm.check_text(want, pb, names) == (n, n)
    assert total <= plan.sam_text_cap() + 64 * n                    # the buffer the CLI and the binding try first holds it
    wins = pm.windows(pb, reads, lens, 8, 2)
    assert len(wins) >= 20
    for i, (s, c, beg, end) in enumerate(wins):
        w, k = cm.expected(pb, reads, names, tags, (c, beg, end))
        rc, text, nr, _ = cm.emu_call(emu, plan, plan.region(s), n_waves=1 + 3 * (i % 2))
        assert rc == 0 and (text, nr) == (w, k), s
        assert cm.check_text(text, pb, names) == (k, k)


def test_handwritten_lines(emu, built):
    d = cm.handmade_dataset()
    pb, plan = d["pb"], host.UnpackPlan(d["blob"], d["fa"])
    reads = pm.reads_a(pb)
    tags = cm.all_tags_a(pb, reads)
    assert [t[0] for t in tags] == [back for _, back in cm.HANDMADE]
    assert [int(x) for x in reads[0]["oi"]] == [0, 1, 2, 3, 4]
    assert [int(x) for x in reads[1]["oi"]] == [0, 1, 2, 3] + list(range(94, 100))
    assert [int(x) for x in reads[3]["dc"]] == [40, 40] == [int(x) for x in reads[4]["dc"]]
    assert [int(x) for x in reads[3]["oi"]] == [40, 41, 42] == [int(x) for x in reads[4]["oi"]]
    # model (b) sees the input: it differs from (a) in the two stated ways and in nothing else
    tb, _ = cm.tags_b(d["sam"], pb, d["names"])
    assert [i for i, (x, y) in enumerate(zip(tags, tb)) if x != y] == [3, 5]
    assert tb[3] == ("40M2D3I57M",) + tags[3][1:] and tb[5][0] == "95M5I" and tb[5][1] == tags[5][1] + 5 and tb[5][2] == tags[5][2]
    want, n = cm.expected(pb, reads, d["names"], tags)
    rc, text, nr, _ = cm.emu_call(emu, plan)
    assert rc == 0 and (text, nr) == (want, n) and cm.check_text(text, pb, d["names"]) == (6, 6)
    plan.close(); pb.close()


def test_genome_shaped_reference(emu, built):
    """MD letters are the uploaded reference bytes (N and IUPAC codes too), and an N over an N is a match."""
    d = cm.genome_dataset()
    pb, plan, names = d["pb"], host.UnpackPlan(d["blob"], d["fa"]), d["names"]
    reads, tags = cm.assert_models_agree(pb, d["sam"], names)
    want, n = cm.expected(pb, reads, names, tags)
    rc, text, nr, _ = cm.emu_call(emu, plan)
    assert rc == 0 and (text, nr) == (want, n) and cm.check_text(text, pb, names) == (n, n)
    letters = set("".join(t[2] for t in tags)) - set("0123456789^")
    assert "N" in letters and letters - set("ACGTN")
    nn = 0
    for rd, t in zip(reads, tags):
        if t[0] == "%dM" % len(rd["seq"]):
            ref = pm.contig_ref(pb, rd["contig"])[rd["pos"] - 1:rd["pos"] - 1 + len(rd["seq"])]
            both = (rd["seq"] == ord("N")) & (ref == ord("N"))
            if both.any():
                nn += 1
                assert t[1] == int((rd["seq"] != ref).sum())         # NM counts none of them
    assert nn >= 5
    assert len(text) <= plan.sam_cigar_text_cap()
    plan.close(); pb.close()


def test_arena_too_small_and_failed_blocks(emu, indel):
    plan, pb, reads, tags, names = indel["plan"], indel["pb"], indel["reads"], indel["tags"], indel["names"]
    smax = plan.max_read_len + plan.read_length - 1
    dec = cm.emu_decode(emu, plan, 0, plan.n_blocks, smax, 1)
    assert (dec[3]["status"] == 9).all()                                       # CBC_ST_EDITS: one entry per read holds no block's edits
    assert cm.emu_call(emu, plan, per_read=1, dec=dec) == (-4, b"", 0, 0)
    rc, text, nr, _ = cm.emu_call(emu, plan, fail_blocks=(1, 4))
    assert rc == -4 and (text, nr) == cm.expected(pb, reads, names, tags, skip_blocks=(1, 4))
    need = max(sum(len(r["dc"]) + len(r["oi"]) for r in reads if r["block"] == b) / int(plan.blocks[b]["n_reads"])
               for b in range(plan.n_blocks))
    assert 1 < need <= 2
    rc, text, nr, _ = cm.emu_call(emu, plan, per_read=2)                       # the smallest arena that holds every block
    assert rc == 0 and (text, nr) == cm.expected(pb, reads, names, tags)


def test_text_cap(emu, indel):
    plan, pb = indel["plan"], indel["pb"]
    want = cm.expected(pb, indel["reads"], indel["names"], indel["tags"])[0]
    rc, text, nr, total = cm.emu_call(emu, plan, cap=len(want) - 1)
    assert rc == -1 and total == len(want) and text == b""
    assert cm.emu_call(emu, plan, cap=len(want))[1] == want
    nl = [len(n) for n in indel["names"]]
    for epr in (0, 1, 16, 510):
        cap = plan.sam_cigar_text_cap(0, plan.n_blocks, epr)
        assert cap == sum(int(b["n_reads"]) * (56 + nl[int(c)] + 3 * plan.seq_stride + 16 * (epr or 16))
                          for b, c in zip(plan.blocks, plan.block_contig))
        assert len(want) <= cap
    assert plan.sam_cigar_text_cap(0, plan.n_blocks, 511) == 0 and plan.sam_cigar_text_cap(0, plan.n_blocks + 1) == 0
    assert plan.sam_cigar_text_cap(2, 1) == 0 and plan.sam_cigar_text_cap(1, 1) == 0
    # the longest line a read can have: every base of a full row its own token
    for b0 in range(plan.n_blocks):
        sel_want = cm.expected(pb, [r for r in indel["reads"] if r["block"] == b0], indel["names"],
                               [t for r, t in zip(indel["reads"], indel["tags"]) if r["block"] == b0])[0]
        assert len(sel_want) <= plan.sam_cigar_text_cap(b0, b0 + 1, 2)


def test_sanitizer_build_of_the_stand_alone_check(built):
    """cigar_emu_check: fabricated records, rows and arena entries (read lengths 1 .. 256, mismatches at the turn's edges, every
    digit count, deletions at 0, 64 and T, runs and lists longer than 64, clips at both ends, every kind of invalid record,
    blocks of 0 .. 65 reads, failed blocks, regions cut through reads, the text one byte short) in a program of its own under
    AddressSanitizer / UBSan, every table at its exact size; it exits non-zero on a finding or a mismatch."""
    subprocess.check_call(["make", "-C", EMU_DIR, "asan_check"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(EMU_DIR, "cigar_emu_check")], capture_output=True, text=True)
    assert r.returncode == 0 and "CIGAR EMU CHECK OK" in r.stdout and "MISMATCH" not in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- the CLI where no device is needed -----------------------------------------------------------------------------------------
def _cli(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def test_cli_refusals_and_empty_selection(indel, tmp_path):
    (tmp_path / "in.cbc").write_bytes(indel["blob"]); (tmp_path / "ref.fa").write_bytes(indel["fa"])
    files = (tmp_path / "in.cbc", tmp_path / "o.sam", tmp_path / "ref.fa")
    for args, msg in [(("--cigar",), "--cigar applies to --sam"), (("--cigar", "--region", "chr1"), "--cigar applies to --sam"),
                      (("--cigar", "--pileup"), "--cigar applies to --sam"),
                      (("--sam", "--cigar", "--region", "chr1", "--region", "chr2"), "at most one --region"),
                      (("--sam", "--cigar", "--regions-file", "x.bed"), "at most one --region"),
                      (("--sam", "--cigar", "--devices", "0,1"), "one device"),
                      (("--sam", "--cigar", "--pileup"), "different outputs"),
                      (("--sam", "--cigar", "--max-edits-per-read", "511"), "1..510"),
                      (("--sam", "--cigar", "--max-edits-per-read", "0"), "1..510"),
                      (("--sam", "--max-edits-per-read", "4"), "--max-edits-per-read applies to --pileup"),
                      (("--max-edits-per-read", "4"), "--max-edits-per-read applies to --pileup"),
                      (("--sam", "--cigar", "--region", "nope"), "nope")]:
        r = _cli("-x", *files, *args)
        assert r.returncode == 1 and msg in r.stderr, (args, r.stderr)
    for args in (("--sam", "--cigar"), ("--cigar",)):
        r = _cli("-c", tmp_path / "ref.fa", tmp_path / "o.cbc", tmp_path / "ref.fa", *args)
        assert r.returncode == 1 and ("applies to decompression" in r.stderr or "--cigar applies to --sam" in r.stderr), r.stderr
    # a compat file
    (tmp_path / "stream.cbc").write_bytes(b"\x00\x00\x00\x64" + bytes(60))
    r = _cli("-x", tmp_path / "stream.cbc", tmp_path / "o.sam", tmp_path / "ref.fa", "--sam", "--cigar")
    assert r.returncode == 1 and "needs a block container" in r.stderr
    # a window in front of the contig's first read: no block selected, the header alone, exit 0, no device opened
    first = min(r["pos"] for r in indel["reads"] if r["contig"] == 0)
    assert first > 1
    r = _cli("-x", *files, "--sam", "--cigar", "--region", "chr1:1-%d" % (first - 1), "--verbose")
    assert r.returncode == 0 and (tmp_path / "o.sam").read_bytes() == indel["plan"].sam_header() and "kernels:" not in r.stdout, r.stdout + r.stderr
    assert "--cigar" in _cli("--help").stdout + _cli("--help").stderr


def test_exports_and_headers(built):
    from cbc_amd import gpu
    assert {"cbc_gpu_decode_sam_cigar", "cbc_gpu_last_sam_cigar_ms"} <= set(gpu.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "cbc_gpu.h")).read()
    assert "cbc_gpu_decode_sam_cigar(" in hdr and "cbc_gpu_last_sam_cigar_ms(" in hdr and "#define CBC_ABI_VERSION" in hdr
    assert "cbc_unpack_sam_cigar_text_cap(" in open(os.path.join(ROOT, "include", "cbc_host.h")).read()
    assert "cbc_cigar_body.h" in open(os.path.join(ROOT, "cbc_amd", "csrc", "Makefile")).read()
