"""The block kernel with the hot var context as a count table in registers (cbc_encode_body.h: CbcEnc::hot_code) on the shapes
of tests/hotctx.py: the HIP kernel against the CPU port (oracle.cpu_encode_blocks) on the same packed batch -- payload bytes,
status, fail_read, nbytes of every block, n_symbols of every block that was coded.  The counts of what var_code does on these
shapes, with and without the table, are asserted on the emulation in tests/test_hot_ctx.py."""
import pytest

import hotctx
from oracle import oracle
from cbc_amd import gpu
from test_hot_ctx import check_blocks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def enc():
    e = gpu.Encoder(0)
    yield e
    e.close()


def _gpu_vs_cpu_port(enc, pb):
    """Whatever the CPU port reports, status included, is the answer."""
    enc.upload_reference(pb.ref)
    payloads, res, offs, flat = enc.encode_blocks(pb)
    assert enc.last_kernel_variant() == 5           # the build that holds the table
    wantp, want = oracle.cpu_encode_blocks(pb, return_payloads=True)
    check_blocks(payloads, res, wantp, want)


CASES = {"overflow": hotctx.overflow, "field_neighbours": hotctx.field_neighbours, "mixed_lengths": hotctx.mixed_lengths,
         "both_call_sites": hotctx.both_call_sites}


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_equals_cpu_port(enc, built, name):
    _gpu_vs_cpu_port(enc, CASES[name]())


@pytest.mark.parametrize("L0", hotctx.EDGE_LENGTHS)
def test_edges_of_the_class(enc, built, L0):
    _gpu_vs_cpu_port(enc, hotctx.edge(L0))


@pytest.mark.parametrize("n", sorted(hotctx.SHORT))
def test_short_blocks(enc, built, n):
    _gpu_vs_cpu_port(enc, hotctx.short_block(n))
