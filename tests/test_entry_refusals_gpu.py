"""The decode entry points of libcbc_gpu.so against tests/golden/entry_refusals.json: for every bad-argument call of
tests/golden/make_entry_refusals.py -- each NULL that is checked, a context without a reference, no blocks, bad windows, names,
interval tables and descriptors, and pairs of defects that pin which refusal wins -- the return code, the text of
cbc_gpu_last_error and the out-parameters are what the recording build gave; and so is which cbc_gpu_last_*_ms answers after a
small run of every kind, and what each says to a NULL out-pointer.  No refusal launches a kernel."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_entry_refusals", os.path.join(HERE, "golden", "make_entry_refusals.py"))
mk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mk)


@pytest.fixture(scope="module")
def golden(built):
    with open(mk.JSON) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def fx(built):
    f = mk.Fixture()
    yield f
    f.close()


def test_every_row_is_recorded(golden, fx):
    rows = mk.rows(fx)
    assert list(golden["rows"]) == [fn + ": " + label for fn, label, _, _ in rows]
    assert {fn for fn, _, _, _ in rows} == set(mk.SIGS)
    # the only calls that succeed are those without blocks or queries: nothing else may reach the device
    assert all(("no blocks" in k or "no query" in k) and "reference not uploaded" not in k for k, r in golden["rows"].items() if r[0] == 0)


@pytest.mark.parametrize("fn", sorted(mk.SIGS))
def test_refusals_match_the_recording(golden, fx, fn):
    mine = [r for r in mk.rows(fx) if r[0] == fn]
    assert len(mine) >= 20
    bad = []
    for row in mine:
        rid = fn + ": " + row[1]
        got, want = mk.run_row(fx, row), golden["rows"][rid]
        for what, g, w in zip(("return code", "error text", "out-parameters"), got, want):
            if g != w:
                bad.append("%s: %s\n  want %r\n  got  %r" % (rid, what, w, g))
    assert not bad, "\n".join(bad[:20])


def test_last_ms_match_the_recording(golden, fx):
    got = mk.last_ms_rows(fx)
    assert list(got) == list(golden["last_ms"])
    bad = ["%s\n  want %r\n  got  %r" % (k, golden["last_ms"][k], json.loads(json.dumps(v))) for k, v in got.items()
           if json.loads(json.dumps(v)) != golden["last_ms"][k]]
    assert not bad, "\n".join(bad[:20])
