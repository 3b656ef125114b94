"""The rule for one SAM line (cbc_amd/csrc/cbc_tok_core.h) at its edges, held to a record of the host packer from BEFORE it
took its parsing from that header: tests/golden/packer_quirks.json, written by tests/packer_corpus.py with the parent
commit's libcbc_host.so.  Per corpus file: return code, message and the sha256 of every array of the packed batch."""
import json

import pytest

import blockref
import packer_corpus
from cbc_amd import gpu, host
from test_tokenise import _emu_pack, _same

with open(packer_corpus.GOLDEN) as _f:
    GOLD = json.load(_f)["files"]
CORPUS = {name: (fa, sam, kw) for name, fa, sam, kw in packer_corpus.corpus()}
NAMES = sorted(CORPUS)


def test_fixture_covers_the_corpus():
    assert sorted(GOLD) == NAMES
    for name, g in GOLD.items():
        # what the device path says of a file follows from what the host packer says of it
        # (3 says nothing: the host packer may still refuse the file it is handed)
        assert g["rc"] == 0 if g["tok_status"] == 0 else g["rc"] != 0 or g["tok_status"] == 3, name
        assert (g["tok_line"] is None) == (g["tok_status"] == 0), name


def test_fixture_entries_show_their_edge():
    """an edited line that the packer skips, or an edit it does not notice, pins nothing: the entries that could fall for that"""
    tok = lambda name: GOLD[name]["sha256"]["tok"]
    # the MD behind 20 other aux fields is NOT seen: the record is coded like the one whose MD was taken away, not like the plain file
    assert tok("md_behind_20_aux_imperfect") == tok("md_less_inherits_imperfect") != tok("xd_for_md")
    # the record without SEQ is a mapped one: QUAL's bytes are in the bases
    assert GOLD["seq_empty"]["sha256"]["seq"] != GOLD["md_less_inherits"]["sha256"]["seq"]
    # the tail of the first of two MD fields shows behind the unterminated text of the soft clip
    assert "MD:Z:96A10C10G10T10A10C10G7" in GOLD["md_fields_several"]["err"]


def _entry(name):
    return {k: v for k, v in GOLD[name].items() if k not in ("tok_status", "tok_line", "parent_threads4")}


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("name", NAMES)
def test_host_packer_reproduces_the_parent(built, name, threads):
    """threads=4 gives what threads=1 gives, but for nul_in_rname: the threaded path's RNAME pre-scan (chunk_phase1, which the
    packer keeps as it was) does not end a line at a NUL, so it numbers a contig that the serial path never sees and reports that
    first.  The fixture keeps what the parent did there as parent_threads4."""
    fa, sam, kw = CORPUS[name]
    want = GOLD[name].get("parent_threads4", _entry(name)) if threads == 4 else _entry(name)
    assert packer_corpus.result(host.pack_sam, sam, fa, threads=threads, **kw) == want


@pytest.mark.parametrize("name", NAMES)
def test_emulated_device_path_reproduces_the_parent(built, name):
    fa, sam, kw = CORPUS[name]
    g = GOLD[name]
    if g["tok_status"] != 0:
        with pytest.raises(ValueError) as e:
            blockref.emu_tokenise(sam)
        assert e.value.args[0] == (g["tok_status"], g["tok_line"])
        return
    t = blockref.emu_tokenise(sam)
    assert packer_corpus.result(lambda s, f, **k: host.pack_from_device_tokens(
        s, f, t["summaries"], t["rname_change"], t["change_off"], t["change_len"], t["n_unmapped"], seq=t["seq"], tok=t["tok"],
        seq_bytes=t["seq_bytes"], n_tok=t["n_tok"], **k), sam, fa, **kw) == _entry(name)
    _same(_emu_pack(sam, fa, **kw), host.pack_sam(sam, fa, threads=1, **kw))


@pytest.mark.gpu
def test_gpu_tokeniser_on_the_corpus(built):
    enc = gpu.Encoder(0)
    for name in NAMES:
        fa, sam, kw = CORPUS[name]
        g = GOLD[name]
        if g["tok_status"] == 0:
            pd, tr = enc.tokenise_sam(sam, fa, fetch=True, **kw)
            _same(pd, host.pack_sam(sam, fa, **kw))
            enc.tokenise_free(tr)
            continue
        with pytest.raises(host.CbcInputError) as e:
            enc.tokenise_sam(sam, fa, **kw)
        assert "line %d: %s (status %d)" % (g["tok_line"] + 1, gpu.TOK_STATUS[g["tok_status"]], g["tok_status"]) in str(e.value), name
    enc.close()
