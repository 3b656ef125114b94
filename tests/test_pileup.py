"""Per-position allele counts without a GPU: the edit-reporting decoder and the pileup bodies on the
lock-step emulation (tests/pileup_emu) against the two models of pileupmodel.py; the stand-alone check under ASan / UBSan;
cbc_unpack_pileup_text_cap; and what the CLI decides without a device."""
import os
import subprocess

import numpy as np
import pytest

import depthmodel as dm
import pileupmodel as pm
import regionmodel as rm
import synth
from cbc_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_DIR = os.path.join(ROOT, "tests", "pileup_emu")
EXE = os.path.join(ROOT, "cbc_amd", "csrc", "cbc")


@pytest.fixture(scope="module")
def emu(built):
    subprocess.check_call(["make", "-C", EMU_DIR, "libcbc_pileup_emu.so"], stdout=subprocess.DEVNULL)
    return pm.emu_load(os.path.join(EMU_DIR, "libcbc_pileup_emu.so"))


def _open(fa, sam, pb, contigs, agree=True):
    blob = rm.container(pb)
    names, lens = dm.names_lens(None, contigs)
    reads = pm.assert_models_agree(pb, sam, names, lens) if agree else pm.reads_a(pb)
    return dict(fa=fa, sam=sam, pb=pb, blob=blob, plan=host.UnpackPlan(blob, fa), names=names, lens=lens, reads=reads)


def _make(kind):
    if kind == "shared":
        return _open(*pm.shared())
    if kind == "mixed":
        return _open(*dm.mixed(7, 64, n=600))
    # N gaps, IUPAC codes and soft-masking in the reference, N-rich reads, at the smallest size that still holds them all
    fa, sam, rbc, contigs = synth.genome_dataset(17, contig_lens=(40_000, 12_000), reads_per_contig=(500, 150),
                                                 contig_kw=dict(n_gaps=3, max_gap=2000))
    return _open(fa, sam, host.pack_sam(sam, fa, block_reads=128), contigs, agree=False)


@pytest.fixture(scope="module", params=["shared", "mixed", "genome"])
def data(request, built):
    d = _make(request.param)
    d["kind"] = request.param
    yield d
    d["plan"].close(); d["pb"].close()


def test_emulation_matches_the_model(emu, data):
    plan, pb, reads, names, lens = data["plan"], data["pb"], data["reads"], data["names"], data["lens"]
    for k, ex in ((1, 0), (2, 0), (3, 16)):
        want = pm.expected(pb, reads, names, lens, None, ex, k)
        assert pm.emu_whole(emu, plan, ex, k) == want, (k, ex)
    assert pm.expected(pb, reads, names, lens)[1] > 50
    if data["kind"] == "genome":                           # the reference column carries the uploaded bytes: N and IUPAC codes too
        refs = {r[2] for r in pm.parse(pm.expected(pb, reads, names, lens)[0])}   # (the packer upper-cases a soft-masked FASTA;
        assert b"N" in refs and refs - set(b"ACGTN"[i:i + 1] for i in range(5))   # lower-case bytes: the stand-alone check)
    top = max(r[3] for r in pm.parse(pm.expected(pb, reads, names, lens)[0]))
    assert pm.emu_whole(emu, plan, 0, top + 50) == (b"", 0, pm.expected(pb, reads, names, lens)[2])     # above every depth
    for i, (s, c, beg, end) in enumerate(pm.windows(pb, reads, lens, 8, 2)):
        k = 1 + (i % 3 == 2)
        sel = plan.region(s)
        for waves in (1, 4):
            rc, t, n, kept, _, _ = pm.emu_call(emu, plan, sel, 0, k, n_waves=waves)
            assert rc == 0 and (t, n, kept) == pm.expected(pb, reads, names, lens, (c, beg, end), 0, k), (s, k, waves)


def test_edits_decoder_on_the_emulation(emu, data):
    """Side array and arena equal model (a); records, rows and spans are what the span decoder writes (depthmodel's emulation)."""
    plan, reads = data["plan"], data["reads"]
    L2 = dm.emu_load(_depth_emu())
    smax = plan.contig_blocks(0).smax
    bl, recs, seq, res, nrec, side, arena = pm.emu_decode(emu, plan, 0, plan.n_blocks, smax)
    bl0, recs0, seq0, res0, _ = dm.emu_decode(L2, plan, 0, plan.n_blocks, smax)
    assert (res["status"] == 0).all() and recs.tobytes() == recs0.tobytes() and seq.tobytes() == seq0.tobytes()
    for b in range(plan.n_blocks):
        r0, n, used = int(bl[b]["rec_base"]), int(bl[b]["n_reads"]), 0
        for r in range(r0, r0 + n):
            dc, oi = reads[r]["dc"], reads[r]["oi"]
            assert int(side[r, 1]) == len(dc) | len(oi) << 16, r
            if len(dc) + len(oi):
                assert int(side[r, 0]) == used
                assert np.array_equal(arena[r0 * 16 + used: r0 * 16 + used + len(dc) + len(oi)].astype(np.int64), np.concatenate([dc, oi])), r
                used += len(dc) + len(oi)
        assert (arena[r0 * 16 + used:(r0 + n) * 16] == 0xEEEE).all()              # nothing behind the entries in use


def _depth_emu():
    d = os.path.join(ROOT, "tests", "depth_emu")
    subprocess.check_call(["make", "-C", d, "libcbc_depth_emu.so"], stdout=subprocess.DEVNULL)
    return os.path.join(d, "libcbc_depth_emu.so")


def test_arena_of_exactly_the_needed_size_and_one_entry_less(emu, built):
    """One block of three reads that need 3 + 2 + 1 = 6 entries: two per read hold them, with the arena full to its last entry;
    one entry per read (three in all) fails the block with CBC_ST_EDITS at the read that does not fit, and the block
    contributes nothing."""
    rng = np.random.default_rng(2)
    c = synth.make_contig(rng, 2000)
    recs = [rm.deletion_read(c, 100, 50, 3, 50)]
    p = 119
    seq = c[p:p + 40].tobytes() + b"GG" + c[p + 40:p + 98].tobytes()
    recs.append(dict(pos=p + 1, flag=0, cigar="40M2I58M", seq=seq, md="98", nm=2))
    recs.append(rm.deletion_read(c, 150, 30, 1, 70))
    fa, sam = synth.fasta_text([("one", c)]), synth.sam_text([("one", len(c), recs)])
    pb = host.pack_sam(sam, fa, block_reads=64, var_length=True)
    d = _open(fa, sam, pb, [("one", c)])
    plan, sel = d["plan"], d["plan"].contig_blocks(0)
    assert plan.n_blocks == 1 and sum(len(r["dc"]) + len(r["oi"]) for r in d["reads"]) == 6
    dec = pm.emu_decode(emu, plan, 0, 1, sel.smax, 2)
    assert int(dec[3][0]["status"]) == 0 and (dec[6] != 0xEEEE).all()
    rc, t, n, kept, _, _ = pm.emu_call(emu, plan, sel, per_read=2, dec=dec)
    assert rc == 0 and (t, n, kept) == pm.expected(pb, d["reads"], d["names"], d["lens"]) and n == 5         # three deleted bases, one, and the insertion's anchor
    dec = pm.emu_decode(emu, plan, 0, 1, sel.smax, 1)
    assert int(dec[3][0]["status"]) == 9 and int(dec[3][0]["fail_read"]) == 1 and (dec[6][3:] == 0xEEEE).all()
    rc, t, n, kept, total, _ = pm.emu_call(emu, plan, sel, per_read=1, dec=dec)
    assert (rc, t, n, kept, total) == (-4, b"", 0, 0, 0)
    plan.close(); pb.close()


def test_failed_block_contributes_nothing(emu, data):
    plan, pb, reads, names, lens = data["plan"], data["pb"], data["reads"], data["names"], data["lens"]
    sel = plan.contig_blocks(0)
    assert sel.b1 - sel.b0 >= 2
    rc, t, n, kept, _, _ = pm.emu_call(emu, plan, sel, fail_blocks=(1,))
    assert rc == -4 and (t, n, kept) == pm.expected(pb, reads, names, lens, (0, 1, lens[0]), skip_blocks=(sel.b0 + 1,))
    assert t != pm.expected(pb, reads, names, lens, (0, 1, lens[0]))[0]


def test_text_cap(built, data):
    plan, pb, reads, names, lens = data["plan"], data["pb"], data["reads"], data["names"], data["lens"]
    for c in range(plan.n_contigs):
        sel = plan.contig_blocks(c)
        k = int(plan.blocks[sel.b0:sel.b1]["n_reads"].sum())
        cap = plan.pileup_text_cap(sel.b0, sel.b1, c, sel.beg, sel.end, sel.smax)
        assert cap == min(lens[c], k * sel.smax) * (len(names[c]) + 102)
        text, n, _ = pm.expected(pb, reads, names, lens, (c, 1, lens[c]))
        assert n <= min(lens[c], k * sel.smax) and len(text) <= cap
        assert max((len(x) for x in text.split(b"\n")), default=0) + 1 <= len(names[c]) + 102
    assert plan.pileup_text_cap(0, plan.n_blocks + 1, 0, 1, 10, 100) == 0 and plan.pileup_text_cap(0, 1, plan.n_contigs, 1, 10, 100) == 0
    assert plan.pileup_text_cap(0, 1, 0, 0, 10, 100) == 0 and plan.pileup_text_cap(0, 1, 0, 11, 10, 100) == 0
    assert plan.pileup_text_cap(0, 1, 0, 1, 2 ** 31, 100) == 0
    # the longest line there is: ten digits in every number
    line = b"%s\t%d\tN" % (names[0], 2 ** 31 - 1) + b"\t4294967295" * 8 + b"\n"
    assert len(line) == len(names[0]) + 102


def test_the_emulated_text_cap_one_byte_short(emu, data):
    plan = data["plan"]
    sel = plan.contig_blocks(0)
    want = pm.expected(data["pb"], data["reads"], data["names"], data["lens"], (0, 1, data["lens"][0]))[0]
    rc, t, n, kept, total, _ = pm.emu_call(emu, plan, sel, cap=len(want) - 1)
    assert rc == -1 and total == len(want) and t == b""
    assert pm.emu_call(emu, plan, sel, cap=len(want))[1] == want


def test_sanitizer_build_of_the_stand_alone_check(built):
    """pileup_emu_check: fabricated records, rows and arena entries (every length, deletions in front of the first and behind
    the last base, insertion runs at both ends, hostile entries, blocks of 0 .. 65 reads, windows cut through reads) in a program
    of its own under AddressSanitizer / UBSan, every table at its exact size; it exits non-zero on a finding or a mismatch."""
    subprocess.check_call(["make", "-C", EMU_DIR, "asan_check"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(EMU_DIR, "pileup_emu_check")], capture_output=True, text=True)
    assert r.returncode == 0 and "PILEUP EMU CHECK OK" in r.stdout and "MISMATCH" not in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- the CLI where no device is needed -----------------------------------------------------------------------------------------
def _cli(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def test_cli_refusals_and_empty_selection(built, tmp_path):
    d = _make("mixed")
    (tmp_path / "in.cbc").write_bytes(d["blob"]); (tmp_path / "ref.fa").write_bytes(d["fa"])
    files = (tmp_path / "in.cbc", tmp_path / "o.txt", tmp_path / "ref.fa")
    for args, msg in [(("--pileup", "--sam"), "different outputs"), (("--pileup", "--depth"), "different outputs"),
                      (("--pileup", "--bedcov"), "different outputs"), (("--pileup", "--depth-hist"), "different outputs"),
                      (("--pileup", "--stats"), "different outputs"), (("--pileup", "--devices", "0,1"), "one device"),
                      (("--min-alt", "2"), "--min-alt applies to --pileup"), (("--pileup", "--min-alt", "0"), "--min-alt wants"),
                      (("--max-edits-per-read", "4"), "--max-edits-per-read applies to --pileup"),
                      (("--pileup", "--max-edits-per-read", "511"), "1..510"), (("--pileup", "--max-edits-per-read", "0"), "1..510"),
                      (("--pileup", "--region", "chr1", "--region", "chr2"), "at most one --region"),
                      (("--pileup", "--regions-file", "x.bed"), "at most one --region"),
                      (("--pileup", "--region", "nope"), "nope")]:
        r = _cli("-x", *files, *args)
        assert r.returncode == 1 and msg in r.stderr, (args, r.stderr)
    r = _cli("-c", tmp_path / "ref.fa", tmp_path / "o.cbc", tmp_path / "ref.fa", "--pileup")
    assert r.returncode == 1 and "applies to decompression" in r.stderr
    # a compat file and a long-read container
    (tmp_path / "stream.cbc").write_bytes(b"\x00\x00\x00\x64" + bytes(60))
    r = _cli("-x", tmp_path / "stream.cbc", tmp_path / "o.txt", tmp_path / "ref.fa", "--pileup")
    assert r.returncode == 1 and "needs a block container" in r.stderr
    # a window in front of the contig's first read: no block selected, an empty file, exit 0, no device opened
    first = min(r["pos"] for r in d["reads"] if r["contig"] == 0)
    assert first > 1
    r = _cli("-x", *files, "--pileup", "--region", "chr1:1-%d" % (first - 1), "--verbose")
    assert r.returncode == 0 and (tmp_path / "o.txt").read_bytes() == b"" and "0 positions from 0 reads in 0 of" in r.stdout, r.stdout + r.stderr
    assert "kernels:" not in r.stdout
    d["plan"].close(); d["pb"].close()


def test_exports_and_headers(built):
    from cbc_amd import gpu
    assert {"cbc_gpu_decode_pileup", "cbc_gpu_last_pileup_ms", "cbc_gpu_decode_blocks_edits"} <= set(gpu.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "cbc_gpu.h")).read()
    assert "cbc_gpu_decode_pileup(" in hdr and "cbc_gpu_decode_blocks_edits(" in hdr and "#define CBC_ST_EDITS" in hdr
    assert "cbc_unpack_pileup_text_cap(" in open(os.path.join(ROOT, "include", "cbc_host.h")).read()
    assert gpu.EDITS_PER_READ == 16
