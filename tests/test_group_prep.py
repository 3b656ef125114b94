"""The group pass of the block encoder on the CPU lock-step emulation: the match test with one lane per record, the
token headers and SNP-count symbols prepared per group (cbc_encode_body.h: match_group, prep_group).
The fused emulation and the two-wavefront emulation against oracle.encode on each block's own SAM text; the shapes are
those of tests/groupprep.py.  The GPU counterpart is tests/test_group_prep_gpu.py."""
import pytest

import blockref
import groupprep
from oracle import oracle


def check_against_oracle(pb, sam, payloads, res):
    assert (res["status"] == 0).all(), res[res["status"] != 0]
    lines = blockref.mapped_sam_lines(sam)
    assert len(lines) == pb.n_recs
    for b in range(pb.n_blocks):
        bsam, bfa = blockref.block_alone_inputs(pb, lines, b)
        exp, st = oracle.encode(bsam, bfa, return_stats=True)
        assert payloads[b] == exp, "block %d: %d bytes vs oracle %d" % (b, len(payloads[b]), len(exp))
        assert int(res[b]["n_symbols"]) == st.n_symbols


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", sorted(groupprep.CASES))
def test_emulation_equals_oracle_per_block(built, name):
    pb, sam = groupprep.packed(name)
    if name.startswith("mixed_lengths"):
        assert [int(x) for x in pb.blocks["n_reads"]] == [200, int(name.split("_")[-1]) - 200]
    if name == "single_record_block":
        assert int(pb.blocks["n_reads"][-1]) == 1
    p1, r1 = blockref.emu_encode(pb)
    check_against_oracle(pb, sam, p1, r1)
    p2, r2 = blockref.emu_encode(pb, two_wave=True)
    check_against_oracle(pb, sam, p2, r2)


KINDS = ["header", "length", "md_count", "md_past_end"]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind", KINDS)
def test_unusable_record_in_the_middle_of_a_group(built, kind):
    """Status and record are those of the CPU port on the same packed block where the CPU port looks at what was spoilt, and
    CBC_ST_ASSERT at the record where it does not; from both forms of the emulation; the blocks around it are coded as ever."""
    pb, blk, rec, cpu_too = groupprep.broken(kind)
    wantp, want = oracle.cpu_encode_blocks(pb, return_payloads=True)
    if cpu_too:
        assert int(want[blk]["status"]) == 2 and int(want[blk]["fail_read"]) == rec
    for two_wave in (False, True):
        payloads, res = blockref.emu_encode(pb, two_wave=two_wave)
        assert [int(x) for x in res["status"]] == [2 if b == blk else 0 for b in range(pb.n_blocks)]
        assert int(res[blk]["fail_read"]) == rec and payloads[blk] == b""
        assert all(payloads[b] == wantp[b] for b in range(pb.n_blocks) if b != blk)
