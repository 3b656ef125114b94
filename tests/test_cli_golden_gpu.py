"""The `cbc` command line on the device against tests/golden/cli_matrix_gpu.json: a few --verbose runs of every decode
mode over the small two-contig container of tests/golden/cli/ -- plain, with a region, with a BED file whose first contig
selects nothing (the device opens on a later call) or that names an unknown contig, and with the mode's own options.
Exit code, stderr, stdout (times masked) and the output file's bytes are what the recording build gave
(tests/golden/make_cli_matrix.py --gpu)."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_cli_matrix", os.path.join(HERE, "golden", "make_cli_matrix.py"))
mk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mk)


@pytest.fixture(scope="module")
def golden(built):
    with open(mk.GPU_JSON) as f:
        return json.load(f)


def test_every_case_is_recorded(golden):
    assert {m: len(v) for m, v in golden["cases"].items()} == {m: len(v) for m, v in mk.gpu_cases().items()}
    assert all(k >= 0 for v in golden["cases"].values() for k in v) and not golden["dropped"]


@pytest.mark.parametrize("mode", sorted(mk.gpu_cases()))
def test_cli_matches_the_recording(golden, mode, tmp_path):
    cases = mk.gpu_cases()[mode]
    assert 3 <= len(cases) <= 5
    for (cid, argv), k in zip(cases, golden["cases"][mode]):
        got, want = mk.run_case(mk.EXE, argv, str(tmp_path / "w"), prefix=("timeout", "-k", "10", "60")), golden["results"][k]
        assert got[0] == want[0] == 0, (cid, got[0], got[1])
        for what, g, w in zip(("stderr", "stdout", "output file"), got[1:], want[1:]):
            assert g == w, (cid, what)
        assert "kernels: " in got[2], cid
