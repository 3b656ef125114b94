"""The SNP run pass of the block encoder on the CPU lock-step emulation (cbc_encode_body.h: run_pass, run_record):
positions, var contexts, chars symbols and snpInRef marks of a run of ordinary records, one lane per SNP.
The fused emulation and the two-wavefront emulation against oracle.encode on each block's own SAM text; the shapes, and
what each of them holds according to a plain model of snpInRef, are those of tests/snppass.py.  The GPU counterpart is
tests/test_snp_pass_gpu.py."""
import os

import pytest

import blockref
import snppass
from oracle import oracle
from test_group_prep import check_against_oracle

KINDS = ["gap", "past_end"]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", sorted(snppass.CASES))
def test_emulation_equals_oracle_per_block(built, name):
    pb, sam = snppass.packed(name)
    p1, r1 = blockref.emu_encode(pb)
    check_against_oracle(pb, sam, p1, r1)
    p2, r2 = blockref.emu_encode(pb, two_wave=True)
    check_against_oracle(pb, sam, p2, r2)


def expected_of_spoilt(pb, blk, rec, kind):
    """(payloads of the CPU port, status, fail_read) the kernel has to report for the spoilt block.
      `gap`       the CPU port has no test of a gap against the var model's alphabet (it reports 0 for this block): the
                  kernel's own contract holds, CBC_ST_ASSERT at the record (include/cbc_gpu.h)
      `past_end`  the CPU port looks: it stops at the read's end and accepts the block, and so does the kernel -- status and
                  fail_read are the CPU port's.  What the two code for the token past the end differs (the kernel reads a
                  zero byte there), so this block's bytes are those the serial walk of the encoder produced before the run
                  pass existed: tests/golden/snp_pass_past_end_block1.bin, taken from the emulation of that form."""
    wantp, want = oracle.cpu_encode_blocks(pb, return_payloads=True)
    print("CPU port on the spoilt block: status %d, fail_read %d, %d bytes" % (int(want[blk]["status"]), int(want[blk]["fail_read"]), len(wantp[blk])))
    if kind == "gap":
        assert int(want[blk]["status"]) == 0
        return wantp, 2, rec
    return wantp, int(want[blk]["status"]), int(want[blk]["fail_read"])


def check_spoilt(pb, blk, wantp, st, fr, payloads, res):
    assert [int(x) for x in res["status"]] == [st if b == blk else 0 for b in range(pb.n_blocks)]
    assert int(res[blk]["fail_read"]) == fr
    assert (payloads[blk] == b"") == (st != 0)
    if st == 0:
        assert payloads[blk] == open(os.path.join(os.path.dirname(__file__), "golden", "snp_pass_past_end_block1.bin"), "rb").read()
    assert all(payloads[b] == wantp[b] for b in range(pb.n_blocks) if b != blk)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("kind", KINDS)
def test_spoilt_token_in_the_middle_of_a_run(built, kind):
    pb, blk, rec = snppass.spoilt(kind)
    wantp, st, fr = expected_of_spoilt(pb, blk, rec, kind)
    seen = []
    for two_wave in (False, True):
        payloads, res = blockref.emu_encode(pb, two_wave=two_wave)
        print("emulation (two_wave=%s): status %s, fail_read %s" % (two_wave, list(res["status"]), list(res["fail_read"])))
        check_spoilt(pb, blk, wantp, st, fr, payloads, res)
        seen.append(payloads[blk])
    assert seen[0] == seen[1]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", ["shared_sites", "indels_between"])
def test_chars_guard_fallback_equals_oracle(built, name):
    """A build whose chars guard is lowered codes the first runs of a block in counting form and the later ones by
    small_code(): both forms in one stream, the bytes still the oracle's."""
    pb, sam = snppass.packed(name)
    counted, fallback = snppass.chars_guard_runs(sam)
    assert counted >= 1 and fallback >= 1
    for two_wave in (False, True):
        p, r = snppass.emu_encode_chars_guard(pb, two_wave=two_wave)
        check_against_oracle(pb, sam, p, r)
