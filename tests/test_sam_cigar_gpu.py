"""CIGAR, NM and MD in the SAM output on the device: Encoder.decode_sam(cigar=True) and `cbc -x --sam
--cigar` against the bytes of the models of cigarmodel.py (which agree with each other and with the lock-step emulation in
test_sam_cigar.py), whole file and through regions cut through reads with indels; the line minus CIGAR and tags is the line
without --cigar; a block that does not fit its arena fails and contributes nothing."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cigarmodel as cm
import pileupmodel as pm
from cbc_amd import gpu, host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cbc_amd", "csrc", "cbc")


@pytest.fixture(scope="module")
def enc(built):
    e = gpu.Encoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module", params=["indel", "handmade", "genome"])
def data(request, built):
    d = dict(indel=cm.indel_dataset, handmade=cm.handmade_dataset, genome=cm.genome_dataset)[request.param]()
    d["kind"] = request.param
    d["plan"] = host.UnpackPlan(d["blob"], d["fa"])
    d["reads"] = pm.reads_a(d["pb"])
    d["tags"] = cm.all_tags_a(d["pb"], d["reads"])
    yield d
    d["plan"].close(); d["pb"].close()


def _cli(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def test_whole_file_and_regions_match_the_model(enc, data, tmp_path):
    plan, pb, reads, tags, names, lens = data["plan"], data["pb"], data["reads"], data["tags"], data["names"], data["lens"]
    enc.upload_reference(plan.ref)
    hdr = plan.sam_header()
    (tmp_path / "in.cbc").write_bytes(data["blob"]); (tmp_path / "ref.fa").write_bytes(data["fa"])
    files = (tmp_path / "in.cbc", tmp_path / "out.sam", tmp_path / "ref.fa")
    want, n = cm.expected(pb, reads, names, tags)
    text, nrd, sel, res = enc.decode_sam(plan, cigar=True, results=True)
    assert (res["status"] == 0).all() and len(res) == plan.n_blocks and sel is None
    assert nrd == n == pb.n_recs and text == hdr + want
    assert cm.check_text(text, pb, names) == (n, n)                  # every line rebuilds the reference it lies on
    assert enc.last_sam_text_bytes == len(want)
    ms = enc.last_sam_cigar_ms()
    assert len(ms) == 4 and ms[0] > 0 and all(x >= 0 for x in ms)
    # minus CIGAR and tags: the line without --cigar, and as many of them
    plain = enc.decode_sam(plan)
    assert cm.strip(text) == plain and text.count(b"\n") == plain.count(b"\n")
    r = _cli("-x", *files, "--sam", "--cigar", "--verbose")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "out.sam").read_bytes() == hdr + want
    assert "kernels: edits decode" in r.stdout and "%d reads written as SAM" % n in r.stdout, r.stdout
    wins = pm.windows(pb, reads, lens, 4, 2)
    assert any(len(r["dc"]) for r in reads) and any(len(r["oi"]) for r in reads)
    for s, c, beg, end in wins:
        w, k = cm.expected(pb, reads, names, tags, (c, beg, end))
        got = enc.decode_sam(plan, region=s, cigar=True, results=True)
        assert got[0] == hdr + w and got[1] == k, s
        assert cm.strip(got[0]) == enc.decode_sam(plan, region=s), s
    for s, c, beg, end in wins[:4]:
        r = _cli("-d", *files, "--sam", "--cigar", "--region", s, "--max-edits-per-read", 32)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / "out.sam").read_bytes() == hdr + cm.expected(pb, reads, names, tags, (c, beg, end))[0], s


def test_without_cigar_the_bytes_are_those_of_the_direct_call(enc, data):
    plan = data["plan"]
    enc.upload_reference(plan.ref)
    blocks, ws, bc = enc._gather(plan, slice(0, plan.n_blocks))
    caps, pay, names, noff = enc._plan_args(plan)
    cap = plan.sam_text_cap()
    text = np.zeros(cap, dtype=np.uint8)
    nbytes, nrd = ctypes.c_uint64(), ctypes.c_uint64()
    rc = gpu.lib().cbc_gpu_decode_sam(enc._ctx, pay.ctypes.data, pay.size, blocks.ctypes.data, plan.n_blocks, ctypes.byref(caps),
                                      ws.ctypes.data, bc.ctypes.data, names.ctypes.data, names.size, noff.ctypes.data, plan.n_contigs,
                                      None, text.ctypes.data, cap, ctypes.byref(nbytes), ctypes.byref(nrd), None)
    assert rc == 0
    assert enc.decode_sam(plan, cigar=False) == plan.sam_header() + text[:int(nbytes.value)].tobytes()
    with pytest.raises(ValueError):
        enc.decode_sam(plan, edits_per_read=4)


def test_the_buffer_is_tried_small_first_and_an_explicit_one_too_small_is_refused(enc, data):
    plan = data["plan"]
    enc.upload_reference(plan.ref)
    want = enc.decode_sam(plan, cigar=True)
    n = len(want) - len(plan.sam_header())
    assert enc.decode_sam(plan, cigar=True, text_cap=n) == want
    with pytest.raises(gpu.CbcGpuError, match="text_cap too small"):
        enc.decode_sam(plan, cigar=True, text_cap=n - 1)
    assert enc.last_sam_text_bytes == n


def test_an_arena_too_small_fails_the_block_and_a_failed_block_contributes_nothing(enc, built):
    """One entry per read holds the edits of no block of the indel dataset: every block fails with CBC_ST_EDITS and the error
    names the option.  A flipped payload byte fails its block alone, and with results=True the other blocks' lines come back."""
    d = cm.indel_dataset()
    plan, pb, names = host.UnpackPlan(d["blob"], d["fa"]), d["pb"], d["names"]
    reads = pm.reads_a(pb)
    tags = cm.all_tags_a(pb, reads)
    enc.upload_reference(plan.ref)
    with pytest.raises(gpu.CbcGpuError, match="max-edits-per-read"):
        enc.decode_sam(plan, cigar=True, edits_per_read=1)
    text, nrd, _, res = enc.decode_sam(plan, cigar=True, edits_per_read=1, results=True)
    need = [sum(len(r["dc"]) + len(r["oi"]) for r in reads if r["block"] == b) for b in range(plan.n_blocks)]
    bad = tuple(b for b in range(plan.n_blocks) if need[b] > int(plan.blocks[b]["n_reads"]))
    assert bad and tuple(np.flatnonzero(res["status"] != 0).tolist()) == bad and (res["status"][list(bad)] == 9).all()
    assert (text, nrd) == (plan.sam_header() + cm.expected(pb, reads, names, tags, skip_blocks=bad)[0], pb.n_recs - sum(
        int(plan.blocks[b]["n_reads"]) for b in bad))
    pay = plan.payloads.copy()
    hurt = plan.n_blocks // 2
    at = int(plan.blocks[hurt]["in_off"]) + int(plan.blocks[hurt]["in_bytes"]) // 2
    plan.payloads[at] ^= 0x55
    try:
        with pytest.raises(gpu.CbcGpuError, match=r"block %d\b" % hurt):
            enc.decode_sam(plan, cigar=True)
        text, nrd, _, res = enc.decode_sam(plan, cigar=True, results=True)
        assert int(res[hurt]["status"]) != 0 and (np.delete(res["status"], hurt) == 0).all()
        want, n = cm.expected(pb, reads, names, tags, skip_blocks=(hurt,))
        assert text == plan.sam_header() + want and nrd == n
    finally:
        plan.payloads[:] = pay
    plan.close(); pb.close()
