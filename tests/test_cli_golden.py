"""The `cbc` command line against tests/golden/cli_matrix.json: for every recorded decode invocation that ends without a
device -- main()'s refusals over the whole option matrix, the value parsers, and the full runs of every mode whose
selection holds no block -- the exit code, stderr, stdout (times masked) and the output file's bytes are what the
recording build gave (tests/golden/make_cli_matrix.py)."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_cli_matrix", os.path.join(HERE, "golden", "make_cli_matrix.py"))
mk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mk)


@pytest.fixture(scope="module")
def golden(built):
    with open(mk.CPU_JSON) as f:
        return json.load(f)


def _group(tag):
    return [(cid, argv) for cid, argv in mk.cpu_cases() if cid.startswith(tag + "/")]


def test_every_case_is_recorded_or_listed_as_dropped(golden):
    ids = [cid for cid, _ in mk.cpu_cases()]
    assert len(set(ids)) == len(ids)
    assert {t: len(v) for t, v in golden["cases"].items()} == {t: len(_group(t)) for t in ("matrix", "compress", "owner", "value", "run")}
    assert (len(_group("matrix")), len(_group("compress")), len(_group("owner"))) == (318, 7, 42 + 7)
    # the dropped ones need a device: none of the refusals, only full runs
    assert golden["dropped"] == [cid for t, v in golden["cases"].items() for (cid, _), k in zip(_group(t), v) if k < 0]
    assert golden["dropped"] and all(i.startswith("run/") for i in golden["dropped"])


@pytest.mark.parametrize("tag", ["matrix", "compress", "owner", "value", "run"])
def test_cli_matches_the_recording(golden, tag, tmp_path):
    bad = []
    for (cid, argv), k in zip(_group(tag), golden["cases"][tag]):
        if k < 0:
            continue
        got, want = mk.run_case(mk.EXE, argv, str(tmp_path / "w")), golden["results"][k]
        for what, g, w in zip(("exit code", "stderr", "stdout", "output file"), got, want):
            if g != w:
                bad.append("%s: %s\n  want %r\n  got  %r" % (cid, what, w, g))
    assert not bad, "\n".join(bad[:20])
