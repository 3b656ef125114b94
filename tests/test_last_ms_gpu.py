"""Which of the six cbc_gpu_last_*_ms answers, on the MI355X: the context remembers the kind of the most recent call that ran a
post-decode stage (region, SAM, depth, targets, coverage, histogram).  Before any such call all six return CBC_E_ARG; after a
call of one kind exactly its entry point returns 0 with finite, non-negative times and the other five return CBC_E_ARG; a plain
decode in between changes nothing.  The C entry points are called directly: three of the Python wrappers keep sums of their
own."""
import ctypes
import math

import pytest

import regionmodel as rm
from cbc_amd import gpu, host

pytestmark = pytest.mark.gpu
CBC_E_ARG = -1
N_OUT = {"region": 3, "sam": 3, "depth": 4, "targets": 4, "coverage": 7, "hist": 5}


@pytest.fixture(scope="module")
def small(built):
    """Two contigs, 300 and 200 reads of 100 bases, 64 reads to a block: five and four blocks."""
    fa, rbc, _ = rm.mixed_dataset(31, [8000, 6000], [300, 200], lengths=(100,), sub_rate=0.004)
    pb = rm.pack(fa, rbc, 64)
    plan = host.UnpackPlan(rm.container(pb), fa)
    assert [int((plan.block_contig == c).sum()) for c in (0, 1)] == [5, 4]
    yield plan
    plan.close(); pb.close()


def _ask(enc):
    """name -> (return code, the times) of every cbc_gpu_last_*_ms."""
    out = {}
    for name, n in N_OUT.items():
        v = [ctypes.c_float(float("nan")) for _ in range(n)]
        rc = getattr(gpu.lib(), "cbc_gpu_last_%s_ms" % name)(enc._ctx, *[ctypes.byref(x) for x in v])
        out[name] = (rc, [float(x.value) for x in v])
    return out


def _only(enc, name, what):
    got = _ask(enc)
    for other, (rc, ms) in got.items():
        if other != name:
            assert rc == CBC_E_ARG, (what, other, rc)
    if name is None:
        return None
    rc, ms = got[name]
    assert rc == 0 and all(math.isfinite(x) and x >= 0 for x in ms), (what, name, rc, ms)
    return ms


def test_only_the_last_kind_answers(small):
    plan = small
    enc = gpu.Encoder(0)
    try:
        _only(enc, None, "fresh context")
        enc.upload_reference(plan.ref)
        _only(enc, None, "reference uploaded")
        enc.decode_blocks(plan)
        _only(enc, None, "plain decode")
        ts = plan.targets([b"chr1:500-2500", b"chr2:300-900", b"chr2:2000-2600"])
        assert len(enc.decode_region(plan, "chr1:1000-3000")) > 0
        _only(enc, "region", "decode_region")
        assert enc.decode_sam(plan) != plan.sam_header()
        _only(enc, "sam", "decode_sam")
        enc.decode_blocks(plan)                               # a plain decode has no post-decode stage: the answer stays
        _only(enc, "sam", "decode_blocks after decode_sam")
        assert len(enc.decode_depth(plan, "chr2:100-4000")) > 0
        _only(enc, "depth", "decode_depth")
        assert len(enc.decode_targets(plan, ts, "reads")) > 0
        assert _only(enc, "targets", "decode_targets reads")[2] == 0.0
        assert enc.decode_targets(plan, ts, "sam") != plan.sam_header()
        assert _only(enc, "targets", "decode_targets sam")[2] == 0.0
        assert len(enc.decode_targets(plan, ts, "depth")) > 0
        _only(enc, "targets", "decode_targets depth")
        assert int(enc.decode_coverage(plan, plan.queries())[3].sum()) > 0
        _only(enc, "coverage", "decode_coverage")
        assert len(enc.decode_depth_hist(plan)) == 2
        _only(enc, "hist", "decode_depth_hist")
        assert len(enc.decode_region(plan, "chr2:1-500")) > 0  # and back to the first kind
        _only(enc, "region", "decode_region again")
    finally:
        enc.close()
