"""The SNP run pass of the block encoder on the GPU (cbc_encode_body.h: run_pass, run_record): the HIP kernel against the
lock-step emulation and against the oracle, block by block -- payload bytes and cbc_block_result.  Shapes: tests/snppass.py;
the CPU counterpart is tests/test_snp_pass.py."""
import pytest

import snppass
from cbc_amd import gpu
from test_group_prep import check_against_oracle
from test_group_prep_gpu import _gpu_vs_emu
from test_snp_pass import KINDS, check_spoilt, expected_of_spoilt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def enc():
    e = gpu.Encoder(0)
    yield e
    e.close()


@pytest.mark.parametrize("name", sorted(snppass.CASES))
def test_kernel_equals_emulation_and_oracle_per_block(enc, built, name):
    pb, sam = snppass.packed(name)
    payloads, res = _gpu_vs_emu(enc, pb)
    check_against_oracle(pb, sam, payloads, res)


@pytest.mark.parametrize("kind", KINDS)
def test_spoilt_token_in_the_middle_of_a_run(enc, built, kind):
    pb, blk, rec = snppass.spoilt(kind)
    wantp, st, fr = expected_of_spoilt(pb, blk, rec, kind)
    payloads, res = _gpu_vs_emu(enc, pb)
    check_spoilt(pb, blk, wantp, st, fr, payloads, res)


def test_chars_guard_fallback_on_the_gpu(built):
    """The test build with the lowered chars guard (counting form for a block's first runs, small_code() for the later
    ones) against the oracle.  Runs in a child process because the library is chosen at import time."""
    import os, subprocess, sys, textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "cbc_amd", "csrc", "libcbc_gpu_charsguard.so")
    assert os.path.exists(lib)
    code = textwrap.dedent("""
        import sys
        sys.path.insert(0, %r); sys.path.insert(0, %r)
        import snppass
        from cbc_amd import gpu
        from test_group_prep import check_against_oracle
        enc = gpu.Encoder(0)
        for name in ("shared_sites", "indels_between"):
            pb, sam = snppass.packed(name)
            counted, fallback = snppass.chars_guard_runs(sam)
            assert counted >= 1 and fallback >= 1
            enc.upload_reference(pb.ref)
            payloads, res, offs, flat = enc.encode_blocks(pb)
            check_against_oracle(pb, sam, payloads, res)
        enc.close()
        print("charsguard ok")
    """ % (root, os.path.join(root, "tests")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, CBC_GPU_LIB=lib), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "charsguard ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
