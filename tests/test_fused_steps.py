"""The coder's remainder test (cbc_encode_body.h: CbcEnc::rem_flag2, the exact form in the block kernels) and its two fused
quiet steps (CbcEnc::step_sameref_rl0, CbcEnc::step_known0_x3: A/B switches of the kernel build, CBC_FUSE_SR / CBC_FUSE_X3, which
the counting emulation of tests/emu/emu_paths.cpp defines; there they cross-check themselves against the single steps run on a
copy of the state) on the CPU lock-step emulation: the fused form and the two-thread form against the CPU port
(oracle.cpu_encode_blocks) on the same packed batch -- payload bytes, status, fail_read, nbytes and n_symbols of every block
-- and the counts of the paths taken.  Shapes: tests/fusedsteps.py; the GPU counterpart is tests/test_fused_steps_gpu.py."""
import pytest

import fusedsteps
from oracle import oracle


def check_blocks(payloads, res, wantp, want):
    """payload bytes, status, fail_read, nbytes of every block; n_symbols of every block that was coded (that of a failed
    block is unspecified: include/cbc_gpu.h)"""
    for field in ("status", "fail_read", "nbytes"):
        assert [int(x) for x in res[field]] == [int(x) for x in want[field]], field
    ok = want["status"] == 0
    assert (res["n_symbols"][ok] == want["n_symbols"][ok]).all()
    assert payloads == wantp


def both_forms_equal_cpu_port(pb):
    wantp, want = oracle.cpu_encode_blocks(pb, return_payloads=True)
    assert (want["status"] == 0).all()
    counts = None
    for two_wave in (False, True):
        payloads, res, c = fusedsteps.emu_encode_counted(pb, two_wave=two_wave)
        check_blocks(payloads, res, wantp, want)
        assert counts is None or c == counts          # the same steps take the same paths in both forms
        counts = c
    return counts


@pytest.mark.timeout(300)
def test_one_length_takes_every_path(built):
    """2 blocks x 1024 records of one length.  Block 0 alone, counted: 1023 records go through each fused form;
    same_ref + rlength[0] takes its fused exit 820 times, falls back 141 times because something shifts and 62 times on a
    remainder flag; rlength[1..3] 654 / 317 / 52.  At least 50 of each are asked for."""
    pb = fusedsteps.one_length()
    assert [int(x) for x in pb.blocks["n_reads"]] == [1024, 1024]
    both_forms_equal_cpu_port(pb)
    wantp, want = oracle.cpu_encode_blocks(pb, blocks=[0], return_payloads=True)
    payloads, res, c = fusedsteps.emu_encode_counted(pb, blocks=[0])
    check_blocks(payloads, res, wantp, want)
    tot = {k: sum(v) for k, v in c.items()}
    print("block 0 path counts:", tot)
    assert tot["sr"] == 1023 and tot["x3"] == 1023
    for k in ("sr_exit", "x3_exit", "sr_fb_shift", "x3_fb_shift", "sr_fb_rem", "x3_fb_rem"):
        assert tot[k] >= 50, (k, tot[k])
    assert tot["sr_exit"] + tot["sr_fb_shift"] + tot["sr_fb_rem"] == tot["sr"]
    assert tot["x3_exit"] + tot["x3_fb_shift"] + tot["x3_fb_rem"] == tot["x3"]
    # a fallback codes its steps one at a time; record 0 does so too (same_ref there is no step_known0)
    assert tot["known0"] == 3 * (tot["x3"] - tot["x3_exit"]) + (tot["sr"] - tot["sr_exit"]) + 3
    assert tot["quiet"] == tot["sr"] - tot["sr_exit"] + 1


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", ["two_lengths", "three_lengths"])
def test_several_lengths_fall_back_through_the_ordinary_tail(built, name):
    """700 records of two (150 / 151) or three (1, 150, 252) lengths in turn: rlength[0] is not near its model's total, its
    step shifts on most records, and same_ref + rlength[0] must fall back: fused exits on fewer than 20 % of the records,
    at least 300 fallbacks.  Counted: two_lengths 56 fused exits, 643 fallbacks; three_lengths 0 and 699."""
    pb = getattr(fusedsteps, name)()
    assert [int(x) for x in pb.blocks["n_reads"]] == [700]
    c = both_forms_equal_cpu_port(pb)
    tot = {k: sum(v) for k, v in c.items()}
    print(name, "path counts:", tot)
    assert tot["sr"] == 699
    assert tot["sr_exit"] < 0.2 * 700
    assert tot["sr_fb_shift"] + tot["sr_fb_rem"] >= 300


@pytest.mark.timeout(300)
def test_escapes(built):
    """700 records, every one of the first 80 with a POS delta not seen before, repeats afterwards: the Esc and Look
    instantiations of the record body run the fused forms next to pos_alpha()."""
    pb = fusedsteps.escapes()
    assert [int(x) for x in pb.blocks["n_reads"]] == [700]
    c = both_forms_equal_cpu_port(pb)
    assert sum(c["sr"]) == 699 and sum(c["x3"]) == 699


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n", sorted(fusedsteps.SHORT))
def test_short_blocks(built, n):
    """Blocks of 1, 2, 63, 64 and 65 records: record 0 alone (no fused step at all), then the fused forms straight after the
    peeled first record."""
    pb = fusedsteps.short_block(n)
    c = both_forms_equal_cpu_port(pb)
    assert sum(c["sr"]) == pb.n_recs - pb.n_blocks and sum(c["x3"]) == pb.n_recs - pb.n_blocks


@pytest.mark.timeout(300)
def test_block_that_stops_with_a_full_pos_table(built):
    """A block whose POS table (cap_pos = 96) is full at a record beyond 600: CBC_ST_CAP_POS at the record that brings the
    96th distinct delta, no payload, from both forms -- the fused forms commit nothing that a later failure would have to
    undo.  The CPU port keeps no POS table (tests/lookahead.py: coder_stops_first) and codes the block whole, so for the
    block that stops the record is counted from the input (fusedsteps.pos_table_full); the block behind it carries the CPU
    port's bytes."""
    pb, blk, rec = fusedsteps.pos_table_full()
    assert rec > 600
    wantp, want = oracle.cpu_encode_blocks(pb, return_payloads=True)
    assert (want["status"] == 0).all()
    for two_wave in (False, True):
        payloads, res, _ = fusedsteps.emu_encode_counted(pb, two_wave=two_wave)
        assert (int(res[blk]["status"]), int(res[blk]["fail_read"]), int(res[blk]["nbytes"])) == (3, rec, 0)
        assert payloads[blk] == b""
        o = 1 - blk
        assert int(res[o]["status"]) == 0 and payloads[o] == wantp[o] and int(res[o]["n_symbols"]) == int(want[o]["n_symbols"])
        assert int(res[o]["nbytes"]) == int(want[o]["nbytes"])
