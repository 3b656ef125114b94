"""The coder wavefront's look-ahead, lane writes and quiet rlength[0] step on the CPU lock-step emulation
(cbc_encode_body.h: look_ahead, CbcEnc::q_put / rec_put / step_fixed_quiet, which cross-checks itself there): the fused emulation and the two-wavefront emulation against the CPU port on the same packed
batch and against oracle.encode on each block's own SAM text.  Shapes: tests/lookahead.py; the GPU counterpart is
tests/test_lookahead_gpu.py."""
import pytest

import blockref
import lookahead
from oracle import oracle
from test_group_prep import check_against_oracle


def check_against_cpu_port(pb, payloads, res):
    wantp, want = oracle.cpu_encode_blocks(pb, return_payloads=True)
    for field in ("status", "fail_read", "nbytes"):
        assert [int(x) for x in res[field]] == [int(x) for x in want[field]], field
    assert payloads == wantp


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", sorted(lookahead.CASES))
def test_emulation_equals_cpu_port_and_oracle_per_block(built, name):
    pb, sam = lookahead.packed(name)
    if name.startswith("group_count"):
        assert [int(x) for x in pb.blocks["n_reads"]] == [int(name.split("_")[-1])]
    if name == "one_record_last_block":
        assert [int(x) for x in pb.blocks["n_reads"]] == [193, 1]
    for two_wave in (False, True):
        payloads, res = blockref.emu_encode(pb, two_wave=two_wave)
        check_against_cpu_port(pb, payloads, res)
        check_against_oracle(pb, sam, payloads, res)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("place", sorted(lookahead.PLACES))
@pytest.mark.parametrize("kind", lookahead.KINDS)
def test_unusable_record_by_group(built, kind, place):
    """An unusable record in group 0, 1, 2 (first and last lane), 3 and the last, partial group of a block: status and record
    are the CPU port's where it looks at what was spoilt (CBC_ST_ASSERT at the record where it does not), from both forms of
    the emulation; the other blocks are coded as ever."""
    pb, blk, rec, cpu_too = lookahead.unusable(kind, place)
    assert rec // 64 == lookahead.PLACES[place] // 64
    wantp, want = oracle.cpu_encode_blocks(pb, return_payloads=True)
    if cpu_too:
        assert int(want[blk]["status"]) == 2 and int(want[blk]["fail_read"]) == rec
    for two_wave in (False, True):
        payloads, res = blockref.emu_encode(pb, two_wave=two_wave)
        assert [int(x) for x in res["status"]] == [2 if b == blk else 0 for b in range(pb.n_blocks)]
        assert int(res[blk]["fail_read"]) == rec and payloads[blk] == b""
        assert all(payloads[b] == wantp[b] for b in range(pb.n_blocks) if b != blk)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("ahead", [1, 2])
def test_coder_stops_before_an_unusable_group(built, ahead):
    """The coder stops by itself (POS table full, record 95) in group 1 while group 2 or group 3 holds an unusable record.
    The fused form meets the records in order and reports the full table either way.  The two-wavefront form validates
    group 2 at the top of group 1, before any record of group 1 is coded, so there the unusable record of group 2 is what
    the block reports; group 3 would be validated at the top of group 2, which is never reached, and the block reports the
    full table.  Both wavefronts end (the call returns) and the other block reports its own full table."""
    pb, blk, rec = lookahead.coder_stops_first(ahead)
    _, fused = blockref.emu_encode(pb)
    _, two = blockref.emu_encode(pb, two_wave=True)
    assert [int(x) for x in fused["status"]] == [3, 3] and [int(x) for x in fused["fail_read"]] == [95, 95]
    assert int(two[1 - blk]["status"]) == 3 and int(two[1 - blk]["fail_read"]) == 95
    if ahead == 1:
        assert int(two[blk]["status"]) == 2 and int(two[blk]["fail_read"]) == rec
    else:
        assert int(two[blk]["status"]) == 3 and int(two[blk]["fail_read"]) == 95
    assert int(two[blk]["nbytes"]) == 0 and int(fused[blk]["nbytes"]) == 0


@pytest.mark.timeout(300)
@pytest.mark.parametrize("ahead", [1, 2])
def test_output_area_too_small_before_an_unusable_group(built, ahead):
    """The same with the other cause: block 0's payload area is too small and the coder stops with CBC_ST_OUT_FULL at record
    185, in group 2, while group 3 or group 4 holds an unusable record.  The fused form meets the records in order and
    reports OUT_FULL at 185 either way.  The two-wavefront form has validated group 3 at the top of group 2, so the
    unusable record of group 3 is what the block reports; group 4 is never looked at and the block reports OUT_FULL at 185.
    No payload either way, both wavefronts end, block 1 is coded as the CPU port codes it."""
    pb, blk, rec = lookahead.output_full_first(ahead)
    assert lookahead.OUT_FULL_AT // 64 == 2 and rec // 64 == 2 + ahead
    wantp, _ = oracle.cpu_encode_blocks(pb, return_payloads=True)
    fp, fused = blockref.emu_encode(pb, shrink_block=blk)
    tp, two = blockref.emu_encode(pb, two_wave=True, shrink_block=blk)
    assert (int(fused[blk]["status"]), int(fused[blk]["fail_read"]), int(fused[blk]["nbytes"])) == (1, lookahead.OUT_FULL_AT, 0)
    want = (2, rec, 0) if ahead == 1 else (1, lookahead.OUT_FULL_AT, 0)
    assert (int(two[blk]["status"]), int(two[blk]["fail_read"]), int(two[blk]["nbytes"])) == want
    for p, r in ((fp, fused), (tp, two)):
        assert int(r[1 - blk]["status"]) == 0 and p[1 - blk] == wantp[1 - blk] and p[blk] == b""


_JITTER_CHILD = r"""
import sys, json
sys.path.insert(0, %r); sys.path.insert(0, %r)
import blockref, lookahead
out = {}
for name in ("group_count_193", "one_length_151", "longest_record_placement", "two_lengths_alternating"):
    pb, _ = lookahead.packed(name)
    p, r = blockref.emu_encode(pb, two_wave=True)
    out[name] = [[int(x) for x in r["status"]], [int(x) for x in r["fail_read"]], [q.hex() for q in p]]
for ahead in (1, 2):
    pb, blk, rec = lookahead.coder_stops_first(ahead)
    p, r = blockref.emu_encode(pb, two_wave=True)
    out["stops-%%d" %% ahead] = [[int(x) for x in r["status"]], [int(x) for x in r["fail_read"]], [q.hex() for q in p]]
print("RESULT " + json.dumps(out))
"""


@pytest.mark.timeout(300)
def test_two_wavefront_form_with_random_pauses(built):
    """The two-thread emulation with random pauses around every hand-off operation (CBC_EMU_JITTER, read once per process:
    hence the child processes): whichever wavefront runs ahead, payloads, status and record stay what they are.  Every
    group of these inputs holds an imperfect record, so the coder cannot pass a whole group without the model wavefront
    ("mask mailbox")."""
    import json, os, subprocess, sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = _JITTER_CHILD % (os.path.dirname(here), here)
    runs = []
    for seed in (None, 3, 11):
        env = dict(os.environ)
        env.pop("CBC_EMU_JITTER", None)
        if seed is not None:
            env["CBC_EMU_JITTER"] = str(seed)
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=280)
        assert r.returncode == 0, r.stderr[-2000:]
        runs.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][0][7:]))
    assert runs[1] == runs[0] and runs[2] == runs[0]
    assert runs[0]["stops-1"][0][0] == 2 and runs[0]["stops-2"][0][0] == 3
