"""The consensus record on the MI355X: Encoder.decode_consensus and `cbc -x --consensus` against
consensusmodel.py on the five datasets of tests/test_consensus.py; two identities against code that is not under test
(decode_pileup's own columns with the rule re-applied, decode_depth on reads without edits); the failures of the edits decoder
as the call reports them."""
import os
import subprocess

import numpy as np
import pytest

import consensusmodel as cm
import pileupmodel as pm
import synth
from cbc_amd import gpu, host
from test_consensus import _args, make, _special_windows
from test_pileup import _open
import test_pileup_gpu as tpg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cbc_amd", "csrc", "cbc")
KINDS = ["shared", "mixed", "genome", "boundary", "deep"]
# the defaults; width 7 with show-del and iupac; fill-ref with min_depth 4, exclusion mask 16 and call_frac 1
OPTION_SETS = [dict(), dict(width=7, flags=cm.SHOW_DEL | cm.IUPAC), dict(flags=cm.FILL_REF, min_depth=4, exclude=16, ppm=1_000_000)]


@pytest.fixture(scope="module")
def enc():
    e = gpu.Encoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module", autouse=True)
def _close_datasets():
    yield
    import test_consensus
    for d in test_consensus._DATA.values():
        d["plan"].close(); d["pb"].close()
    test_consensus._DATA.clear()


def _kw(o):
    """an option set of the model as the binding's keywords and the binary's options"""
    f = o.get("flags", 0)
    frac = {750_000: "0.75", 1_000_000: "1", 500_000: "0.5"}[o.get("ppm", 750_000)]
    kw = dict(exclude_flags=o.get("exclude", 0), min_depth=o.get("min_depth", 1), call_frac=frac, line_width=o.get("width", 60),
              show_del=bool(f & cm.SHOW_DEL), fill_ref=bool(f & cm.FILL_REF), iupac=bool(f & cm.IUPAC))
    cli = ["--depth-exclude-flags", kw["exclude_flags"], "--call-min-depth", kw["min_depth"], "--call-frac", frac, "--line-width", kw["line_width"]]
    cli += [x for x, on in (("--show-del", kw["show_del"]), ("--fill-ref", kw["fill_ref"]), ("--iupac", kw["iupac"])) if on]
    return kw, cli


def _cli(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def _summary(cnt, kept, blocks):
    return "consensus: %d bases (%d ref, %d alt, %d deleted, %d ambiguous, %d low depth, %d no call; %d insertions not applied) from %d reads in %d blocks\n" % (
        cnt["emitted"], cnt["ref"], cnt["alt"], cnt["del"], cnt["ambiguous"], cnt["low_depth"], cnt["no_call"], cnt["ins_skipped"], kept, blocks)


@pytest.mark.parametrize("kind", KINDS)
def test_consensus_matches_the_model(enc, built, kind, tmp_path):
    """Fails without the feature: the binding and the binary against the model's bytes, counters and reads kept -- the whole
    file under the three option sets, then five windows."""
    d = make(kind)
    plan, pb, reads, names, lens = d["plan"], *_args(d)
    enc.upload_reference(plan.ref)
    (tmp_path / "in.cbc").write_bytes(d["blob"]); (tmp_path / "ref.fa").write_bytes(d["fa"])
    files = (tmp_path / "in.cbc", tmp_path / "out.fa", tmp_path / "ref.fa")
    for o in OPTION_SETS:
        kw, cli = _kw(o)
        want = cm.expected(pb, reads, names, lens, **o)
        text, cnt, kept, res = enc.decode_consensus(plan, results=True, **kw)
        assert (res["status"] == 0).all() and len(res) == plan.n_blocks
        assert (cnt, kept) == want[1:] and text == want[0], o
        assert enc.last_consensus_text_bytes == len(want[0])
        r = _cli("-x", *files, "--consensus", "--verbose", *cli)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / "out.fa").read_bytes() == want[0], o
        assert _summary(want[1], want[2], plan.n_blocks) in r.stdout and "kernels: edits decode" in r.stdout and "text " in r.stdout, r.stdout
    ms = enc.last_consensus_ms()
    assert len(ms) == 4 and ms[0] > 0 and all(x >= 0 for x in ms)
    if kind == "boundary":
        wins = [("bnd:%d-%d" % (b, e), c, b, e) for c, b, e, _, _ in _special_windows(d)[:5]]
    else:
        wins = pm.windows(pb, reads, lens, 5, 3)[:5]
    for i, (s, c, beg, end) in enumerate(wins):
        o = OPTION_SETS[i % 3]
        kw, cli = _kw(o)
        want = cm.expected(pb, reads, names, lens, (c, beg, end), **o)
        assert enc.decode_consensus(plan, s, **kw) == want, (s, o)
        r = _cli("-d", *files, "--consensus", "--region", s, *cli)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / "out.fa").read_bytes() == want[0], (s, o)


@pytest.mark.parametrize("kind", ["shared", "boundary"])
def test_identity_against_decode_pileup(enc, built, kind):
    """Code not under test: with show-del byte i of the body is position beg + i; the rule re-applied to every line of
    decode_pileup(min_alt=1) from that line's own columns gives the consensus byte; a position without a line is the
    upper-cased reference base or a low-depth byte; the reads kept are decode_depth's."""
    d = make(kind)
    plan, pb, reads, names, lens = d["plan"], *_args(d)
    enc.upload_reference(plan.ref)
    for ex, ppm, frac, flags in ((0, 750_000, "0.75", 0), (16, 500_000, "0.5", cm.IUPAC)):
        text, cnt, kept = enc.decode_consensus(plan, exclude_flags=ex, call_frac=frac, show_del=True, iupac=bool(flags))
        body = cm.body_of(text)[1]
        assert len(body) == lens[0] and cnt["emitted"] == lens[0]
        ptext, _, pkept, _ = enc.decode_pileup(plan, exclude_flags=ex, min_alt=1, results=True)
        have = set()
        for row in pm.parse(ptext):
            b = cm.call(list(row[4:9]), row[9], row[10], row[2][0], 1, ppm, flags | cm.SHOW_DEL)[0]
            assert body[row[1] - 1] == b, row
            have.add(row[1])
        assert have == {r[1] for r in pm.parse(pm.expected(pb, reads, names, lens, None, ex, 1)[0])} and len(have) >= 18   # boundary: 8 SNP sites, 8 deleted positions, 2 insertion anchors
        ref = pm.contig_ref(pb, 0)[:lens[0]]
        up = np.where(pm.klass(ref) < 4, ref & 0xDF, ord("N"))
        rest = np.array([p for p in range(1, lens[0] + 1) if p not in have], dtype=np.int64)
        got = np.frombuffer(body, dtype=np.uint8)[rest - 1]
        assert ((got == up[rest - 1]) | (got == ord("N"))).all()
        assert kept == pkept == enc.decode_depth(plan, exclude_flags=ex, results=True)[2]


def test_identity_against_decode_depth(enc, built):
    """Reads without any edit: the consensus is the upper-cased reference wherever decode_depth reports depth >= 1, N elsewhere."""
    import depthmodel as dm
    rng = np.random.default_rng(21)
    contig = synth.make_contig(rng, 9000)
    recs = synth.make_reads(rng, contig, 150, 100, sub_rate=0, indel_frac=0)
    fa, sam = synth.fasta_text([("plain", contig)]), synth.sam_text([("plain", 9000, recs)])
    d = _open(fa, sam, host.pack_sam(sam, fa, block_reads=64), [("plain", contig)])
    plan = d["plan"]
    enc.upload_reference(plan.ref)
    text, cnt, kept = enc.decode_consensus(plan)
    body = np.frombuffer(cm.body_of(text)[1], dtype=np.uint8)
    covered = np.zeros(9000, dtype=bool)
    bg, _, dkept, _ = enc.decode_depth(plan, results=True)
    for _, s, e, dep in dm.parse(bg):
        covered[s:e] = dep >= 1
    assert 1000 < covered.sum() < 9000 and kept == dkept == 150
    assert (body == np.where(covered, contig, ord("N"))).all()
    assert cnt == dict(emitted=9000, ref=int(covered.sum()), alt=0, ambiguous=0, low_depth=int((~covered).sum()), no_call=0, ins_skipped=0, **{"del": 0})
    plan.close(); d["pb"].close()


def test_failures(enc, built):
    """Mirrors test_edits_decoder of tests/test_pileup_gpu.py: an arena too small for a block fails that block (status 9) and the
    message names the option; with results=True the text is the model's with those blocks skipped; a flipped payload byte names
    its block; a text_cap too small is CBC_E_ARG with the needed size.  None of them faults the device."""
    d = tpg._make("mixed")
    plan, pb, reads, names, lens = d["plan"], *_args(d)
    enc.upload_reference(plan.ref)
    with pytest.raises(gpu.CbcGpuError, match="max-edits-per-read"):
        enc.decode_consensus(plan, edits_per_read=1)
    text, cnt, kept, res = enc.decode_consensus(plan, edits_per_read=1, results=True)
    bad = tuple(np.flatnonzero(res["status"] != 0).tolist())
    assert bad and (res["status"][list(bad)] == 9).all()
    assert (text, cnt, kept) == cm.expected(pb, reads, names, lens, skip_blocks=bad)
    pay = plan.payloads.copy()
    hurt = plan.n_blocks // 2
    at = int(plan.blocks[hurt]["in_off"]) + int(plan.blocks[hurt]["in_bytes"]) // 2
    plan.payloads[at] ^= 0x55
    try:
        with pytest.raises(gpu.CbcGpuError, match=r"block %d\b" % hurt):
            enc.decode_consensus(plan)
    finally:
        plan.payloads[:] = pay
    want = cm.expected(pb, reads, names, lens, (0, 1, lens[0]), with_range=False)[0]
    sel = plan.contig_blocks(0)
    if plan.n_contigs == 1:
        with pytest.raises(gpu.CbcGpuError, match="text_cap too small"):
            enc.decode_consensus(plan, text_cap=len(want) - 1)
        assert enc.last_consensus_text_bytes == len(want)
        assert enc.decode_consensus(plan, text_cap=len(want))[0] == want
    else:                                                             # one call per contig: probe the first alone
        region = "%s:1-%d" % (names[0].decode(), lens[0])
        want = cm.expected(pb, reads, names, lens, (0, 1, lens[0]))[0]
        with pytest.raises(gpu.CbcGpuError, match="text_cap too small"):
            enc.decode_consensus(plan, region, text_cap=len(want) - 1)
        assert enc.last_consensus_text_bytes == len(want)
        assert enc.decode_consensus(plan, region, text_cap=len(want))[0] == want
    for bad_kw in (dict(min_depth=0), dict(line_width=0), dict(line_width=65536), dict(call_frac="0"), dict(call_frac="1.5")):
        with pytest.raises(ValueError):
            enc.decode_consensus(plan, **bad_kw)
    o = host.ConsensusOpts(1, 750_000, 60, 8)                       # an unknown flag bit, straight at the C call
    blocks, ws, _ = enc._gather(plan, slice(sel.b0, sel.b1))
    caps, pay2, _, _ = enc._plan_args(plan)
    import ctypes
    nbytes, nk, cc = ctypes.c_uint64(), ctypes.c_uint64(), host.ConsensusCounts()
    for opts, wr in ((o, 0), (host.ConsensusOpts(0, 750_000, 60, 0), 0), (host.ConsensusOpts(1, 0, 60, 0), 0), (host.ConsensusOpts(1, 1_000_001, 60, 0), 0),
                     (host.ConsensusOpts(1, 750_000, 0, 0), 0), (host.ConsensusOpts(1, 750_000, 65536, 0), 0), (host.ConsensusOpts(1, 750_000, 60, 0), 2)):
        rc = gpu.lib().cbc_gpu_decode_consensus(enc._ctx, pay2.ctypes.data, pay2.size, blocks.ctypes.data, sel.b1 - sel.b0, ctypes.byref(caps),
                                                ws.ctypes.data, names[0], len(names[0]), 1, lens[0], sel.smax, 0, 0, ctypes.byref(opts), wr,
                                                None, 0, ctypes.byref(nbytes), ctypes.byref(cc), ctypes.byref(nk), None)
        assert rc == -1, (opts.min_depth, opts.call_ppm, opts.line_width, opts.flags, wr)
    plan.close(); d["pb"].close()
