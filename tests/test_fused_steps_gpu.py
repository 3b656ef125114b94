"""The block kernels with the exact remainder test (cbc_encode_body.h: CbcEnc::rem_flag2) on the shapes of the coder's quiet
steps: the HIP kernel against the lock-step emulation and against the CPU port on the same packed batch -- payload bytes,
status, fail_read, nbytes and n_symbols of every block.  (The fused quiet steps, CbcEnc::step_sameref_rl0 and
CbcEnc::step_known0_x3, are A/B switches of the kernel build and run in tests/test_fused_steps.py, on the counting emulation.)
Shapes: tests/fusedsteps.py."""
import pytest
import torch

import blockref
import fusedsteps
from oracle import oracle
from cbc_amd import gpu
from test_fused_steps import check_blocks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def enc():
    e = gpu.Encoder(0)
    yield e
    e.close()


def _gpu_vs_emu_and_cpu_port(enc, pb):
    enc.upload_reference(pb.ref)
    payloads, res, offs, flat = enc.encode_blocks(pb)
    ep, eres = blockref.emu_encode(pb)
    check_blocks(payloads, res, ep, eres)
    wantp, want = oracle.cpu_encode_blocks(pb, return_payloads=True)
    assert (want["status"] == 0).all()
    check_blocks(payloads, res, wantp, want)


CASES = {"one_length": fusedsteps.one_length, "two_lengths": fusedsteps.two_lengths, "three_lengths": fusedsteps.three_lengths,
         "escapes": fusedsteps.escapes}


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_equals_emulation_and_cpu_port(enc, built, name):
    _gpu_vs_emu_and_cpu_port(enc, CASES[name]())


@pytest.mark.parametrize("n", sorted(fusedsteps.SHORT))
def test_short_blocks(enc, built, n):
    _gpu_vs_emu_and_cpu_port(enc, fusedsteps.short_block(n))


def test_block_that_stops_with_a_full_pos_table(enc, built):
    """CBC_ST_CAP_POS at a record beyond 600, no payload: status, record and nbytes are the emulation's and the record is the
    one counted from the input; the block behind it carries the CPU port's bytes (the CPU port keeps no POS table and is no
    reference for the block that stops: tests/test_fused_steps.py)."""
    pb, blk, rec = fusedsteps.pos_table_full()
    enc.upload_reference(pb.ref)
    payloads, res, offs, flat = enc.encode_blocks(pb)
    ep, eres = blockref.emu_encode(pb, two_wave=True)
    check_blocks(payloads, res, ep, eres)
    assert (int(res[blk]["status"]), int(res[blk]["fail_read"]), int(res[blk]["nbytes"])) == (3, rec, 0) and rec > 600
    wantp, want = oracle.cpu_encode_blocks(pb, return_payloads=True)
    o = 1 - blk
    assert int(res[o]["status"]) == 0 and payloads[o] == wantp[o] and int(res[o]["n_symbols"]) == int(want[o]["n_symbols"])


def test_six_wave_kernel_every_block_vs_cpu_port(enc, built):
    """10 x CU count + 1 blocks of 640 records (about 1.6 M records): more than ten blocks per CU, so the library launches
    the 6-waves-per-SIMD build of the kernel.  Every block against the CPU port,
    every 64th against the emulation."""
    n_blocks = 10 * torch.cuda.get_device_properties(0).multi_processor_count + 1
    pb = fusedsteps.many_blocks(n_blocks)
    assert pb.n_blocks == n_blocks and (pb.blocks["n_reads"] == 640).all()
    enc.upload_reference(pb.ref)
    payloads, res, offs, flat = enc.encode_blocks(pb)
    assert enc.last_kernel_variant() == 6
    wantp, want = oracle.cpu_encode_blocks(pb, return_payloads=True)
    assert (want["status"] == 0).all()
    for field in ("status", "fail_read", "nbytes", "n_symbols"):
        assert (res[field] == want[field]).all(), field
    bad = [b for b in range(n_blocks) if payloads[b] != wantp[b]]
    assert not bad, bad[:8]
    for b, p, r in blockref.emu_encode_blocks(pb, range(0, n_blocks, 64)):
        assert p == payloads[b] and int(r["status"]) == 0
        assert int(r["nbytes"]) == int(res[b]["nbytes"]) and int(r["n_symbols"]) == int(res[b]["n_symbols"])
