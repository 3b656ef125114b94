"""The coder wavefront's look-ahead, lane writes and quiet rlength[0] step on the GPU (cbc_encode_body.h: look_ahead,
CbcEnc::q_put / rec_put / step_fixed_quiet; cbc_wave_gpu.h: set_lane2_uv / set_lane3): the HIP kernel against the lock-step emulation and against the CPU port on
the same packed batch -- payload bytes, status, fail_read and nbytes of every block.  Shapes: tests/lookahead.py; the CPU
counterpart is tests/test_lookahead.py."""
import ctypes

import numpy as np
import pytest
import torch

import blockref
import lookahead
from oracle import oracle
from cbc_amd import gpu, host
from test_lookahead import check_against_cpu_port

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def enc():
    e = gpu.Encoder(0)
    yield e
    e.close()


def _gpu_vs_emu(enc, pb, two_wave=False):
    enc.upload_reference(pb.ref)
    payloads, res, offs, flat = enc.encode_blocks(pb)
    ep, eres = blockref.emu_encode(pb, two_wave=two_wave)
    for field in ("status", "fail_read", "nbytes"):
        assert [int(x) for x in res[field]] == [int(x) for x in eres[field]], field
    ok = res["status"] == 0                      # n_symbols of a failed block is unspecified (include/cbc_gpu.h)
    assert (res["n_symbols"][ok] == eres["n_symbols"][ok]).all()
    assert payloads == ep
    return payloads, res


@pytest.mark.parametrize("name", sorted(lookahead.CASES))
def test_kernel_equals_emulation_and_cpu_port(enc, built, name):
    pb, sam = lookahead.packed(name)
    payloads, res = _gpu_vs_emu(enc, pb)
    check_against_cpu_port(pb, payloads, res)


@pytest.mark.parametrize("place", sorted(lookahead.PLACES))
@pytest.mark.parametrize("kind", lookahead.KINDS)
def test_unusable_record_by_group(enc, built, kind, place):
    """Status and record of the CPU port on the same packed block (CBC_ST_ASSERT at the record where the CPU port does not look
    at what was spoilt); the other blocks of the launch are intact."""
    pb, blk, rec, cpu_too = lookahead.unusable(kind, place)
    wantp, want = oracle.cpu_encode_blocks(pb, return_payloads=True)
    payloads, res = _gpu_vs_emu(enc, pb)
    if cpu_too:
        assert int(want[blk]["status"]) == 2 and int(want[blk]["fail_read"]) == rec
    assert [int(x) for x in res["status"]] == [2 if b == blk else 0 for b in range(pb.n_blocks)]
    assert int(res[blk]["fail_read"]) == rec and payloads[blk] == b""
    assert all(payloads[b] == wantp[b] for b in range(pb.n_blocks) if b != blk)


@pytest.mark.parametrize("ahead", [1, 2])
def test_coder_stops_before_an_unusable_group(enc, built, ahead):
    """The coder stops by itself (POS table full) in group 1 while group 2 / group 3 holds an unusable record: status and
    record are the two-wavefront emulation's (group 2 is validated before group 1 is coded and wins; group 3 is never
    looked at); the launch returns and the other block reports its own full table."""
    pb, blk, rec = lookahead.coder_stops_first(ahead)
    payloads, res = _gpu_vs_emu(enc, pb, two_wave=True)
    assert int(res[1 - blk]["status"]) == 3 and int(res[1 - blk]["fail_read"]) == 95
    if ahead == 1:
        assert int(res[blk]["status"]) == 2 and int(res[blk]["fail_read"]) == rec
    else:
        assert int(res[blk]["status"]) == 3 and int(res[blk]["fail_read"]) == 95


def _gpu_encode_shrunk(enc, pb, shrink_block):
    """The device-pointer entry point on a batch whose output plan is the library's, except that `shrink_block` keeps only
    lookahead.SHRUNK_PAYLOAD bytes of payload area (what blockref.emu_encode(shrink_block=...) does to the emulation)."""
    L = gpu.lib()
    dev = torch.device("cuda", 0)
    blocks = pb.blocks.copy()
    total = int(L.cbc_gpu_plan_output(blocks.ctypes.data, pb.n_blocks, pb.recs.ctypes.data, pb.tok.ctypes.data))
    blocks[shrink_block]["reserved"] = lookahead.SHRUNK_PAYLOAD
    td = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    d = [td(x) for x in (pb.recs, pb.seq, pb.tok, pb.names, blocks, pb.ref)]
    d_out = torch.zeros(total, dtype=torch.uint8, device=dev)
    d_res = torch.zeros(pb.n_blocks * host.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    db = gpu.DeviceBatch(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), pb.n_blocks,
                         d[5].data_ptr(), d[5].numel(), d_out.data_ptr(), total, d_res.data_ptr(), d[1].numel(), pb.n_tok,
                         pb.n_recs, host.LdsCaps(pb.cap_pos, pb.cap_var))
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.cbc_gpu_encode_blocks_device(enc._ctx, ctypes.byref(db), stream)
    torch.cuda.synchronize()
    assert rc in (0, -4), rc                         # -4: some block reports a status of its own
    res = d_res.cpu().numpy().view(host.RESULT_DTYPE)
    out = d_out.cpu().numpy()
    return [out[int(b["out_off"]):int(b["out_off"]) + int(r["nbytes"])].tobytes() for b, r in zip(blocks, res)], res


@pytest.mark.parametrize("ahead", [1, 2])
def test_output_area_too_small_before_an_unusable_group(enc, built, ahead):
    """Block 0's payload area is too small (the coder stops with CBC_ST_OUT_FULL at record 185, in group 2) while group 3 /
    group 4 holds an unusable record: status, record and nbytes are the two-wavefront emulation's -- the unusable record of
    group 3, validated before group 2 is coded, wins; group 4 is never looked at and the block reports OUT_FULL at 185, as
    the fused emulation does.  The launch returns and block 1 carries the CPU port's bytes."""
    pb, blk, rec = lookahead.output_full_first(ahead)
    payloads, res = _gpu_encode_shrunk(enc, pb, blk)
    ep, eres = blockref.emu_encode(pb, two_wave=True, shrink_block=blk)
    for field in ("status", "fail_read", "nbytes"):
        assert [int(x) for x in res[field]] == [int(x) for x in eres[field]], field
    want = (2, rec, 0) if ahead == 1 else (1, lookahead.OUT_FULL_AT, 0)
    assert (int(res[blk]["status"]), int(res[blk]["fail_read"]), int(res[blk]["nbytes"])) == want
    wantp, _ = oracle.cpu_encode_blocks(pb, return_payloads=True)
    assert payloads == ep and payloads[1 - blk] == wantp[1 - blk] and payloads[blk] == b""
