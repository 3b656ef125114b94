"""The group pass of the block encoder on the GPU (cbc_encode_body.h: match_group with one lane per record, prep_group):
the HIP kernel against the lock-step emulation and against the oracle, block by block -- payload bytes and
cbc_block_result.  Shapes: tests/groupprep.py; the CPU counterpart is tests/test_group_prep.py."""
import pytest

import blockref
import groupprep
from oracle import oracle
from cbc_amd import gpu
from test_group_prep import KINDS, check_against_oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def enc():
    e = gpu.Encoder(0)
    yield e
    e.close()


def _gpu_vs_emu(enc, pb):
    enc.upload_reference(pb.ref)
    payloads, res, offs, flat = enc.encode_blocks(pb)
    ep, eres = blockref.emu_encode(pb)
    for field in ("status", "fail_read", "nbytes"):
        assert [int(x) for x in res[field]] == [int(x) for x in eres[field]], field
    # n_symbols of a failed block is unspecified (include/cbc_gpu.h): where its coder wavefront stood when the failure reached it
    ok = res["status"] == 0
    assert (res["n_symbols"][ok] == eres["n_symbols"][ok]).all()
    assert payloads == ep
    return payloads, res


@pytest.mark.parametrize("name", sorted(groupprep.CASES))
def test_kernel_equals_emulation_and_oracle_per_block(enc, built, name):
    pb, sam = groupprep.packed(name)
    payloads, res = _gpu_vs_emu(enc, pb)
    check_against_oracle(pb, sam, payloads, res)


@pytest.mark.parametrize("kind", KINDS)
def test_unusable_record_in_the_middle_of_a_group(enc, built, kind):
    """Status and record of the CPU port on the same packed block (CBC_ST_ASSERT at the record where the CPU port does not look
    at what was spoilt); the other blocks of the launch are intact."""
    pb, blk, rec, cpu_too = groupprep.broken(kind)
    wantp, want = oracle.cpu_encode_blocks(pb, return_payloads=True)
    payloads, res = _gpu_vs_emu(enc, pb)
    if cpu_too:
        assert int(want[blk]["status"]) == 2 and int(want[blk]["fail_read"]) == rec
    assert [int(x) for x in res["status"]] == [2 if b == blk else 0 for b in range(pb.n_blocks)]
    assert int(res[blk]["fail_read"]) == rec and payloads[blk] == b""
    assert all(payloads[b] == wantp[b] for b in range(pb.n_blocks) if b != blk)
