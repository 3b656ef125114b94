"""The cases of tests/longcases.py on the HIP kernels: the three-wavefront encoder (walker -> model -> coder, the mailbox, the two
halves of the edit buffer, `over` and the second walk across wavefronts run only here -- the CPU emulation is one fused
wavefront) == oracle/cbc_long.c byte for byte per block, and the decoder returns the reads.  Only well-formed input: corrupt
payloads are the CPU emulation's (tests/test_long_edges.py)."""
import os
import subprocess

import numpy as np
import pytest

import longcases as lc
from cbc_amd import gpu, host
from oracle import oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST_OK, ST_ASSERT = 0, 2


@pytest.fixture(scope="module")
def enc():
    e = gpu.Encoder(0)
    yield e
    e.close()


def _round_trip(enc, c, **pack_kw):
    pb = host.pack_sam(c.sam, c.fasta, long_reads=True, **pack_kw)
    assert pb.n_recs == len(c.pos)
    enc.upload_reference(pb.ref)
    payloads, res, offs, flat = enc.encode_long_blocks(pb)
    assert (res["status"] == ST_OK).all(), res[res["status"] != 0][:4]
    cp, cres = oracle.cpu_encode_blocks(pb, return_payloads=True, long_reads=True)
    assert (cres["status"] == ST_OK).all()
    assert [len(p) for p in payloads] == [len(p) for p in cp] and payloads == cp
    assert (res["n_symbols"] == cres["n_symbols"]).all()
    plan = host.UnpackPlan(pb.container(flat, offs), c.fasta)
    enc.upload_reference(plan.ref)
    recs, seq, dres = enc.decode_long_blocks(plan)
    assert (dres["status"] == ST_OK).all() and (dres["n_symbols"] == res["n_symbols"]).all()
    assert plan.text(recs, seq) == c.text
    assert (recs["flag"] == np.array(c.flag)).all() and (recs["rlen"] == np.array(c.rlen)).all() and (recs["pos"] == pb.recs["pos"]).all()
    for b in range(pb.n_blocks):
        r0, n = int(pb.blocks[b]["rec_base"]), int(pb.blocks[b]["n_reads"])
        assert (recs["pos"][r0:r0 + n].astype(np.int64) + int(plan.window_start[b]) == np.array(c.pos[r0:r0 + n])).all()
    return pb


@pytest.mark.parametrize("name", lc.NAMES)
def test_gpu_long_edge_case(enc, built, name):
    """What each case reaches is asserted from its edit lists in tests/test_long_edges.py."""
    _round_trip(enc, lc.case(name))


def test_gpu_too_many_edits_reaches_the_result(enc, built):
    """65536 edits in one read: the walker wavefront's refusal travels walker -> model -> coder -> results with the CPU statement's
    status and fail_read; the neighbouring block is coded as ever.  65535 edits code and round-trip."""
    c = lc.too_many_edits()
    pb = host.pack_sam(c.sam, c.fasta, long_reads=True, block_reads=3)
    assert pb.n_blocks == 2
    cp, cres = oracle.cpu_encode_blocks(pb, return_payloads=True, long_reads=True)
    enc.upload_reference(pb.ref)
    payloads, res, offs, flat = enc.encode_long_blocks(pb)
    assert res["status"][0] == cres["status"][0] == ST_ASSERT and res["fail_read"][0] == cres["fail_read"][0] == 1
    assert res["nbytes"][0] == 0 and payloads[0] == b""
    assert res["status"][1] == ST_OK and payloads[1] == cp[1] and res["n_symbols"][1] == cres["n_symbols"][1]
    assert _round_trip(enc, lc.too_many_edits(5535), block_reads=3).n_blocks == 2


def test_cli_long_edges_round_trip(built, tmp_path):
    """cbc -c --long, then cbc -d, over runs + ncig + lists in POS order."""
    exe = os.path.join(ROOT, "cbc_amd", "csrc", "cbc")
    c = lc.concat([lc.case("runs"), lc.case("ncig"), lc.case("lists")])
    (tmp_path / "in.sam").write_bytes(c.sam); (tmp_path / "ref.fa").write_bytes(c.fasta)
    r = subprocess.run([exe, "-c", "--long", str(tmp_path / "in.sam"), str(tmp_path / "out.cbc"), str(tmp_path / "ref.fa")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "-d", str(tmp_path / "out.cbc"), str(tmp_path / "reads.txt"), str(tmp_path / "ref.fa")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "reads.txt").read_bytes() == c.text
