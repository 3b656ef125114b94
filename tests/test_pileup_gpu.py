"""Per-position allele counts on the MI355X: Encoder.decode_pileup and `cbc -x --pileup` against the
two models of pileupmodel.py; the edit-reporting decoder against the span decoder and model (a); three identities against code
that is not under test (decode_depth, decode_sam); counters past 255 and 65 535."""
import os
import subprocess

import numpy as np
import pytest

import depthmodel as dm
import pileupmodel as pm
import regionmodel as rm
import synth
from cbc_amd import gpu, host
from test_genome_shapes import genome

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cbc_amd", "csrc", "cbc")


@pytest.fixture(scope="module")
def enc():
    e = gpu.Encoder(0)
    yield e
    e.close()


def _open(fa, sam, pb, contigs, agree=True):
    blob = rm.container(pb)
    names, lens = dm.names_lens(None, contigs)
    reads = pm.assert_models_agree(pb, sam, names, lens) if agree else pm.reads_a(pb)
    return dict(fa=fa, sam=sam, pb=pb, blob=blob, plan=host.UnpackPlan(blob, fa), names=names, lens=lens, reads=reads)


def _make(kind):
    if kind == "shared":
        return _open(*pm.shared())
    if kind == "mixed":
        return _open(*dm.mixed(7, 64, n=1200))             # block 0 ends in the 40-base deletion read
    fa, sam, rbc, contigs = genome()                      # N gaps, IUPAC, soft-masking; N-rich reads: model (a) alone
    return _open(fa, sam, host.pack_sam(sam, fa, block_reads=1024), contigs, agree=False)


@pytest.fixture(scope="module", params=["shared", "mixed", "genome"])
def data(request, built):
    d = _make(request.param)
    d["kind"] = request.param
    yield d
    d["plan"].close(); d["pb"].close()


def _cli(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


def test_pileup_matches_the_model(enc, data, tmp_path):
    """Fails without the feature: the binding and the binary against the model's bytes, whole file, five random windows,
    min_alt 1 and 3, an exclusion mask."""
    plan, pb, reads, names, lens = data["plan"], data["pb"], data["reads"], data["names"], data["lens"]
    enc.upload_reference(plan.ref)
    (tmp_path / "in.cbc").write_bytes(data["blob"]); (tmp_path / "ref.fa").write_bytes(data["fa"])
    files = (tmp_path / "in.cbc", tmp_path / "out.txt", tmp_path / "ref.fa")
    for k, ex in ((1, 0), (3, 0), (1, 16)):
        want = pm.expected(pb, reads, names, lens, None, ex, k)
        text, lines, kept, res = enc.decode_pileup(plan, exclude_flags=ex, min_alt=k, results=True)
        assert (res["status"] == 0).all() and len(res) == plan.n_blocks
        assert (lines, kept) == want[1:] and text == want[0], (k, ex)
        r = _cli("-x", *files, "--pileup", "--min-alt", k, "--depth-exclude-flags", ex, "--verbose")
        assert r.returncode == 0, r.stderr
        assert (tmp_path / "out.txt").read_bytes() == want[0], (k, ex)
        assert "kernels: edits decode" in r.stdout and "%d positions from %d reads" % want[1:] in r.stdout, r.stdout
    assert pm.expected(pb, reads, names, lens)[1] > 100
    ms = enc.last_pileup_ms()
    assert len(ms) == 4 and ms[0] > 0 and all(x >= 0 for x in ms)
    wins = pm.windows(pb, reads, lens, 5, 3)
    for i, (s, c, beg, end) in enumerate(wins):
        k = 1 + 2 * (i % 2)
        want = pm.expected(pb, reads, names, lens, (c, beg, end), 0, k)
        got = enc.decode_pileup(plan, s, min_alt=k, results=True)
        assert (got[0], got[1], got[2]) == want, (s, k)
    for s, c, beg, end in wins[:5]:
        r = _cli("-d", *files, "--pileup", "--region", s)
        assert r.returncode == 0, r.stderr
        assert (tmp_path / "out.txt").read_bytes() == pm.expected(pb, reads, names, lens, (c, beg, end))[0], s


def test_edits_decoder(enc, data):
    """Records, rows and spans byte-identical to the span decoder's; side array and arena equal to model (a); an arena
    too small for a block fails that block with CBC_ST_EDITS; a flipped payload byte fails its block."""
    plan, reads = data["plan"], data["reads"]
    enc.upload_reference(plan.ref)
    smax = plan.contig_blocks(0).smax
    recs0, seq0, res0 = enc.decode_blocks_span(plan, smax)
    for epr in (16, 1):
        recs, seq, res, side, arena = enc.decode_blocks_edits(plan, smax, epr)
        for b in range(plan.n_blocks):
            r0, n = int(plan.blocks[b]["rec_base"]), int(plan.blocks[b]["n_reads"])
            need = sum(len(reads[r]["dc"]) + len(reads[r]["oi"]) for r in range(r0, r0 + n))
            if need > n * epr:
                assert int(res[b]["status"]) == 9, (b, epr)
                continue
            assert int(res[b]["status"]) == 0, (b, epr)
            assert recs[r0:r0 + n].tobytes() == recs0[r0:r0 + n].tobytes()
            assert seq[r0 * plan.seq_stride:(r0 + n) * plan.seq_stride].tobytes() == seq0[r0 * plan.seq_stride:(r0 + n) * plan.seq_stride].tobytes()
            used = 0
            for r in range(r0, r0 + n):
                dc, oi = reads[r]["dc"], reads[r]["oi"]
                assert int(side[r, 1]) == len(dc) | len(oi) << 16, r
                if len(dc) + len(oi):
                    assert int(side[r, 0]) == used, r
                    got = arena[r0 * epr + used: r0 * epr + used + len(dc) + len(oi)].astype(np.int64)
                    assert np.array_equal(got, np.concatenate([dc, oi])), r
                    used += len(dc) + len(oi)
        if epr == 16:
            assert (res["status"] == 0).all() and (res0["status"] == 0).all()
    if data["kind"] == "mixed":                           # 64 reads, 40 deleted bases in one of them: one entry per read does not hold them
        assert int(res[0]["status"]) == 9
        with pytest.raises(gpu.CbcGpuError, match="max-edits-per-read"):
            enc.decode_pileup(plan, edits_per_read=1)
        text, lines, kept, pres = enc.decode_pileup(plan, edits_per_read=1, results=True)
        bad = tuple(np.flatnonzero(pres["status"] != 0).tolist())
        assert bad and (pres["status"][list(bad)] == 9).all()
        assert (text, lines, kept) == pm.expected(data["pb"], reads, data["names"], data["lens"], skip_blocks=bad)
    pay = plan.payloads.copy()
    hurt = plan.n_blocks // 2
    at = int(plan.blocks[hurt]["in_off"]) + int(plan.blocks[hurt]["in_bytes"]) // 2
    plan.payloads[at] ^= 0x55
    try:
        res = enc.decode_blocks_edits(plan, smax)[2]
        assert int(res[hurt]["status"]) != 0 and (np.delete(res["status"], hurt) == 0).all()
        with pytest.raises(gpu.CbcGpuError, match=r"block %d\b" % hurt):
            enc.decode_pileup(plan)
    finally:
        plan.payloads[:] = pay


def _tiled(seed=3, n=400, L=100, n_indel=80):
    """A dataset whose every covered position past the first is reported at min_alt 1: read s starts at s and differs from
    the reference in every base but its first (L - 1 SNPs, the most a record holds), so position p >= 2 holds the mismatching
    second base of the read before it; indel-rich ordinary reads lie over them."""
    rng = np.random.default_rng(seed)
    c = synth.make_contig(rng, n + L + 50)
    nxt = np.zeros(256, dtype=np.uint8)
    for a, b in zip(b"ACGT", b"CGTA"):
        nxt[a] = b
    recs = []
    for s in range(n):
        seq = nxt[c[s:s + L]]
        seq[0] = c[s]
        md, nm = synth._md_and_nm(c, s, [("M", L)], seq)
        recs.append(dict(pos=s + 1, flag=16 * (s & 1), cigar="%dM" % L, seq=seq.tobytes(), md=md, nm=nm))
    recs += synth.make_reads(rng, c, n_indel, L, sub_rate=0.01, indel_frac=1.0, max_start=n)
    recs.sort(key=lambda r: r["pos"])
    contigs = [("tile", c)]
    fa, sam = synth.fasta_text(contigs), synth.sam_text([("tile", len(c), recs)])
    return fa, sam, host.pack_sam(sam, fa, block_reads=64, var_length=True), contigs


def test_identities_against_depth_and_sam(enc, built):
    """Against code not under test: the depth column, run-length encoded, is the text of decode_depth under the same exclusion
    (over a window whose every covered position is reported); n_reads_kept is decode_depth's; the sum of A + C + G + T + N is
    the bases of the kept reads (decode_sam) less their inserted bases (the model)."""
    d = _open(*_tiled())
    plan, reads = d["plan"], d["reads"]
    enc.upload_reference(plan.ref)
    last = max(r["pos"] + r["span"] - 1 for r in reads)
    assert sum(1 for r in reads if len(r["dc"])) > 10 and sum(1 for r in reads if len(r["oi"])) > 10
    for ex in (0, 16):
        region = "tile:2-%d" % last
        text, lines, kept, res = enc.decode_pileup(plan, region, exclude_flags=ex, results=True)
        assert (res["status"] == 0).all()
        rows = pm.parse(text)
        bg, runs, dkept, _ = enc.decode_depth(plan, region, exclude_flags=ex, results=True)
        assert kept == dkept
        pos = np.array([r[1] for r in rows], dtype=np.int64)
        dep = np.array([r[3] for r in rows], dtype=np.int64)
        covered = sum(e - s for _, s, e, _ in dm.parse(bg))
        assert lines == len(rows) == covered                        # every covered position has its line
        full = np.zeros(last - 1, dtype=np.int64)
        full[pos - 2] = dep
        assert dm.bedgraph(b"tile", 2, full)[0] == bg
        assert all(r[3] == sum(r[4:10]) for r in rows)
    text, lines, kept, _ = enc.decode_pileup(plan, "tile:2-%d" % last, results=True)
    cols = [ln.split(b"\t") for ln in enc.decode_sam(plan).split(b"\n") if ln and not ln.startswith(b"@")]
    bases, at_one = sum(len(c[9]) for c in cols), sum(1 for c in cols if int(c[3]) == 1)
    # every position from 2 on that holds an aligned base is reported (above); a read at POS 1 has one aligned base in front
    assert kept == len(cols) and at_one >= 1
    assert sum(sum(r[4:9]) for r in pm.parse(text)) == bases - sum(len(r["oi"]) for r in reads) - at_one
    plan.close(); d["pb"].close()


def test_counters_pass_255_and_65535(enc, built):
    """100 000 reads of 100 bases over a 150-base contig with three shared variant sites: the depth and the sites' mismatch
    counters pass 65 535.  The expected tables are numpy sums over the SAM records; the container is coded on the device."""
    fa, body = synth.shared_variant_dataset(9, 150, 100_000, 100, site_every=50, err=0.0)
    contig = np.frombuffer(b"".join(fa.split(b"\n")[1:]), dtype=np.uint8)
    sam = b"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:c\tLN:150\n" + body
    pb = host.pack_sam(sam, fa, block_reads=4096, var_length=True)
    enc.upload_reference(pb.ref)
    _, res, offs, flat = enc.encode_blocks(pb, want_payload_list=False)
    assert (res["status"] == 0).all()
    plan = host.UnpackPlan(pb.container(flat, offs), fa)
    enc.upload_reference(plan.ref)
    cols = [ln.split(b"\t") for ln in body.split(b"\n") if ln]
    start = np.array([int(c[3]) for c in cols], dtype=np.int64)
    seqs = np.frombuffer(b"".join(c[9] for c in cols), dtype=np.uint8).reshape(len(cols), 100)
    cnt = np.zeros((5, 150), dtype=np.int64)
    np.add.at(cnt, (pm.klass(seqs).ravel(), (start[:, None] - 1 + np.arange(100)[None, :]).ravel()), 1)
    zero = np.zeros(150, dtype=np.int64)
    want, n = pm.text_of(b"c", 1, contig, cnt, zero, zero)
    text, lines, kept, res = enc.decode_pileup(plan, results=True)
    assert (res["status"] == 0).all() and kept == 100_000
    rows = pm.parse(text)
    assert max(r[3] for r in rows) > 65_535 and sum(1 for r in rows if r[3] - r[4 + int(pm.klass(r[2][0]))] > 65_535) >= 1
    assert (text, lines) == (want, n)
    plan.close(); pb.close()
