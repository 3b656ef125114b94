"""The long-read format (stream version 3) at its model rescales and at every threshold of its kernels, on
inputs built to reach them (tests/longcases.py): the kernel bodies on the CPU wave emulation == oracle/cbc_long.c byte for byte,
and decode(encode(x)) == x.  The random workloads of tests/test_long.py stay a factor of three short of any rescale point and
hit the thresholds only by chance.  The same cases run on the HIP kernels in tests/test_long_edges_gpu.py.

What a case claims to reach is asserted from its edit lists (derived from the construction, not from a codec) by arithmetic on
the models' initial counts, steps and the rescale point 2^20."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import blockref
import longcases as lc
from cbc_amd import host
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LONG_EMU_DIR = os.path.join(ROOT, "tests", "long_emu")
ST_OK, ST_ASSERT = 0, 2


def check_case(c, **pack_kw):
    """Emulated encoder == CPU statement (payloads, n_symbols, status); emulated decoder of the container == the case's reads,
    POS, FLAG and lengths; the CPU statement's decoder agrees on every block.  Returns (packed batch, encoder results)."""
    pb = host.pack_sam(c.sam, c.fasta, long_reads=True, **pack_kw)
    assert pb.long_reads and pb.n_recs == len(c.pos)
    ep, eres = blockref.emu_long_encode(pb)
    cp, cres = oracle.cpu_encode_blocks(pb, return_payloads=True, long_reads=True)
    assert (cres["status"] == ST_OK).all() and (eres["status"] == cres["status"]).all()
    assert ep == cp and (eres["n_symbols"] == cres["n_symbols"]).all() and all(len(p) > 8 for p in ep)
    plan = host.UnpackPlan(blockref.container_from_payloads(pb, ep), c.fasta)
    assert plan.long_reads and plan.n_recs == pb.n_recs and plan.n_blocks == pb.n_blocks
    recs, seq, dres = blockref.emu_long_decode(plan)
    assert (dres["status"] == ST_OK).all() and (dres["n_symbols"] == eres["n_symbols"]).all()
    assert plan.text(recs, seq) == c.text
    assert (recs["flag"] == np.array(c.flag)).all() and (recs["rlen"] == np.array(c.rlen)).all() and (recs["pos"] == pb.recs["pos"]).all()
    for b in range(pb.n_blocks):
        r0, n, nb, s0 = int(pb.blocks[b]["rec_base"]), int(pb.blocks[b]["n_reads"]), int(pb.info[b]["n_bases"]), int(pb.blocks[b]["seq_base"])
        assert (recs["pos"][r0:r0 + n].astype(np.int64) + int(plan.window_start[b]) == np.array(c.pos[r0:r0 + n])).all()
        crecs, cseq = oracle.cpu_long_decode_block(ep[b], pb.ref, int(pb.blocks[b]["ref_off"]), n + 1, nb + 16)
        assert len(crecs) == n and (cseq[:nb] == pb.seq[s0:s0 + nb]).all()
        assert (crecs["pos"] == pb.recs["pos"][r0:r0 + n]).all() and (crecs["flag"] == pb.recs["flag"][r0:r0 + n]).all()
    return pb, eres


# ------------------------------------------------------------------------------------------------ the models' rescales
# uses after which a table halves for the first time; a second halving follows after about half as many again
GAP_FIRST = lc.uses_to_rescale(256, 10)             # 104 832
SMALL3_FIRST = lc.uses_to_rescale(3, 8)             # kindm: 131 072 less a use
CHARS_FIRST = (lc.RESCALE - 5 + 7) // 8             # a chars row's counts start at 1 or more: no later than this


@pytest.mark.parametrize("name,kind,strand", [("rescale_sub", 0, 0), ("rescale_ins", 1, 1), ("rescale_del", 2, 0)])
def test_models_rescale(built, name, kind, strand):
    """One gap table (both halves: LDS and global), one kind context and, with insertions, chars row 5 pass 2^20 -- the gap table
    twice -- inside one block; batches near a rescale point take the serial path, some carry the gx bytes."""
    c = lc.case(name)
    u = lc.context_uses(c)
    assert 104_000 < GAP_FIRST < 105_000 and 170_000 > GAP_FIRST + GAP_FIRST // 2 + 6_000    # halved total ~2^19 + 128: two rescales by 170 000 uses
    assert u["gap_ctx"][2 * kind + strand] >= 170_000
    assert u["kind_ctx"][kind] >= 135_000 > SMALL3_FIRST
    if kind == 1:
        assert u["ins"] >= 135_000 > CHARS_FIRST
    assert u["sym64"] >= 300 and u["g255"] >= 30
    assert max(len(e) for e in c.edits) <= 65535 and len(c.edits) == 12 and set(c.rlen) == {60_000}
    assert min(u["kinds"]) > 0                                                      # not only one kind: every kindm row is in use
    pb, _ = check_case(c)
    assert pb.n_blocks == 1


# ------------------------------------------------------------------------------------------------ the thresholds
def _cigars(c):
    return [ln.split(b"\t")[5].decode() for ln in c.sam.splitlines() if ln and not ln.startswith(b"@")]


def test_runs_beyond_the_lane_walk(built):
    c = lc.case("runs")
    runs = [(int(n), op) for cg in _cigars(c) for n, op in re.findall(r"(\d+)([MIDS])", cg)]
    for op, want in (("I", {64, 65, 300, 1000}), ("D", {64, 65, 300}), ("S", {200, 700}), ("M", {256, 257, 5000})):
        assert want <= {n for n, o in runs if o == op}
    assert set(c.flag) == {0, 16}
    check_case(c)


def test_gaps_at_every_escape(built):
    c = lc.case("gaps")
    got = [int(e[0, 0]) for e in c.edits if len(e)]
    assert got == lc.GAPS + [65534] and [len(e) for e in c.edits] == [1] * len(lc.GAPS) + [0, 1]
    assert c.rlen[-2:] == [65535, 65535]
    check_case(c)


def test_edit_counts_at_the_buffer_limits(built):
    c = lc.case("counts")
    n = [len(e) for e in c.edits]
    assert n[:len(lc.COUNTS)][:2] == [lc.EDIT_HALF, lc.EDIT_HALF + 1] and sorted(n[:len(lc.COUNTS)]) == lc.COUNTS
    assert n[len(lc.COUNTS):] == lc.COUNTS_LANE == [lc.EDIT_HALF - 1, lc.EDIT_HALF, lc.EDIT_HALF + 1]
    for cg in _cigars(c)[len(lc.COUNTS):]:                                          # all of it in the lane-per-run walk's reach
        assert all(int(k) <= (256 if op == "M" else 64) for k, op in re.findall(r"(\d+)([MIDS])", cg))
    assert set(c.flag) == {0, 16} and max(c.rlen) <= 65535
    pb, _ = check_case(c)
    assert pb.n_blocks == 1


def test_cigar_run_counts_around_a_walk_step(built):
    c = lc.case("ncig")
    cg = _cigars(c)
    assert [len(re.findall(r"\d+[MIDS]", x)) for x in cg] == lc.NCIG
    assert all(set("MIDS") <= set(re.sub(r"\d", "", x)) for x in cg)
    check_case(c)


def test_reads_at_both_ends_of_the_contig(built):
    c = lc.case("ends")
    clen = int(re.search(rb"LN:(\d+)", c.sam).group(1))
    assert c.pos[:3] == [1, 1, 1]
    span = [sum(int(n) for n, op in re.findall(r"(\d+)([MIDS])", x) if op in "MD") for x in _cigars(c)]
    assert sum(p + s - 1 == clen for p, s in zip(c.pos, span)) >= 4 and {x[-1] for x in _cigars(c)} == {"M", "I", "D"}
    check_case(c)


def test_full_lists_and_a_four_byte_pos_step(built):
    c = lc.case("lists")
    assert len(set(c.rlen)) == 64 and len(set(c.flag)) == 64 and len(set(np.diff(c.pos))) == 63
    assert len({x >> 8 for x in c.rlen}) == 64 and len({x & 255 for x in c.rlen}) == 64
    pb, _ = check_case(c)
    assert pb.n_blocks == 1 and int(pb.blocks[0]["n_reads"]) == 64
    c = lc.case("big_step")
    assert c.pos[1] - c.pos[0] + 1 >= 1 << 24
    pb, _ = check_case(c)
    assert pb.n_blocks == 1


def test_n_in_read_and_reference(built):
    c = lc.case("n_bases")
    assert b"N" in c.text and c.fasta.count(b"N") >= 2365
    e = np.concatenate(c.edits)
    assert len(c.edits[0]) == 0 and (c.edits[1][:, 1] == 0).sum() == 300                # N over N matches; 300 bases over the N run
    assert (e[:, 1] == 2).sum() == 10
    check_case(c)


def test_too_many_edits_is_refused_and_the_limit_codes(built):
    """65536 edits in one read: the same status, fail_read and empty payload from the emulation and the CPU statement, the
    block's other reads not coded, the other block as ever.  65535 edits code and round-trip."""
    c = lc.too_many_edits()
    assert [len(e) for e in c.edits][:3] == [2, 65536, 2]
    pb = host.pack_sam(c.sam, c.fasta, long_reads=True, block_reads=3)
    assert pb.n_blocks == 2
    ep, eres = blockref.emu_long_encode(pb)
    cp, cres = oracle.cpu_encode_blocks(pb, return_payloads=True, long_reads=True)
    assert eres["status"][0] == cres["status"][0] == ST_ASSERT and eres["fail_read"][0] == cres["fail_read"][0] == 1
    assert eres["nbytes"][0] == cres["nbytes"][0] == 0 and ep[0] == cp[0] == b""
    assert eres["status"][1] == cres["status"][1] == ST_OK and ep[1] == cp[1] and len(ep[1]) > 8
    twin = lc.too_many_edits(5535)
    assert [len(e) for e in twin.edits][:3] == [2, 65535, 2]
    pb2, _ = check_case(twin, block_reads=3)
    assert pb2.n_blocks == 2


# ------------------------------------------------------------------------------------------------ the packer's long mode
def _line(k, pos, n):
    return b"r%d\t0\t%s\t%d\t60\t%dM\t*\t0\t0\t%s\t*\n" % (k, lc.NAME, pos, n, b"A" * n)


def test_packer_long_limits(built):
    c = lc.contig(3, 1_200_000); c[:] = ord("A")
    fa = lc.fasta(c)
    with pytest.raises(host.CbcInputError, match="65535"):
        host.pack_sam(_line(0, 1, 65536), fa, long_reads=True)
    pb = host.pack_sam(_line(0, 1, 65535), fa, long_reads=True)
    assert pb.n_recs == 1 and pb.max_read_len == 65535
    # a 65th read opens a new block
    pb = host.pack_sam(b"".join(_line(k, 1 + k, 100) for k in range(65)), fa, long_reads=True)
    assert list(pb.blocks["n_reads"]) == [64, 1]
    # 16 reads of 65535 bases are 1 048 560 bases; a 17th of 17 would pass 1 Mbase by one: 16 fills the block to the base
    body = [_line(k, 1 + k, 65535) for k in range(16)]
    pb = host.pack_sam(b"".join(body + [_line(16, 20, 16)]), fa, long_reads=True)
    assert list(pb.blocks["n_reads"]) == [17] and int(pb.info[0]["n_bases"]) == 1 << 20
    pb = host.pack_sam(b"".join(body + [_line(16, 20, 17)]), fa, long_reads=True)
    assert list(pb.blocks["n_reads"]) == [16, 1] and int(pb.info[1]["n_bases"]) == 17


# ------------------------------------------------------------------------------------------------ corrupt payloads, stand-alone
def _ref_span(cigar):
    return sum(int(n) for n, op in re.findall(r"(\d+)([MIDS])", cigar) if op in "MD")


def test_long_decoder_on_corrupt_payloads_under_sanitizers(built, tmp_path):
    """A program of its own (tests/long_emu, AddressSanitizer / UBSan) runs cbc_long_decode on the wave emulation over seeded
    corruptions of a real container -- bit flips, truncations, a block index off by one base, a reference cut short -- with every
    buffer at exactly the size the call is told.  It exits 0 only if every trial returned with a documented status and never
    wrote outside the block's declared bases."""
    c = lc.concat([lc.case("runs"), lc.case("ncig")])
    pb = host.pack_sam(c.sam, c.fasta, long_reads=True, block_reads=7)
    assert pb.n_blocks == 2
    ep, eres = blockref.emu_long_encode(pb)
    assert (eres["status"] == ST_OK).all()
    plan = host.UnpackPlan(blockref.container_from_payloads(pb, ep), c.fasta)
    spans = [_ref_span(x) for x in _cigars(c)]
    dump = [struct.pack("<8sQQQQ", b"CBLEDGE1", plan.n_blocks, plan.cap_pos, len(plan.ref), len(plan.payloads))]
    for b in range(plan.n_blocks):
        r0, n = int(plan.blocks[b]["rec_base"]), int(plan.blocks[b]["n_reads"])
        need = max(int(pb.recs["pos"][r]) - 1 + spans[r] for r in range(r0, r0 + n))        # reference bytes the block's reads reach
        dump.append(plan.blocks[b:b + 1].tobytes() + struct.pack("<Q", int(plan.blocks[b]["ref_off"]) + need))
    dump += [plan.payloads.tobytes(), plan.ref.tobytes()]
    path = tmp_path / "long.dump"
    path.write_bytes(b"".join(dump))
    subprocess.check_call(["make", "-C", LONG_EMU_DIR, "asan_check"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(LONG_EMU_DIR, "long_emu_check"), str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and "LONG EMU CHECK OK" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
    assert int(re.search(r"trials=(\d+)", r.stdout).group(1)) >= 200
