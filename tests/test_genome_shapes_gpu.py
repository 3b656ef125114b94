"""Genome-shaped input on the MI355X (-m gpu): N gaps, IUPAC codes, soft-masked FASTA and N-rich reads through the HIP
block, stream, 2-bit, long-read, tokeniser and region paths, each against the oracle or the input itself.  The inputs and
their feature checks are those of test_genome_shapes.py, whose emulation tests must pass first."""
import os
import subprocess

import numpy as np
import pytest

import blockref
import regionmodel as rm
import synth
from cbc_amd import gpu, host
from oracle import oracle
from test_genome_shapes import check_features, decoded_seq, dense_iupac, expected_bases, genome, long_genome, row4_snps

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "cbc_amd", "csrc", "cbc")
_N = ord("N")


@pytest.fixture(scope="module")
def enc():
    e = gpu.Encoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def data(built):
    fa, sam, rbc, contigs = genome()
    check_features(rbc, contigs)
    return fa, sam, rbc, contigs


def _cli(*args):
    return subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True)


@pytest.mark.parametrize("br", [512, 4096, 16384])
def test_gpu_block_encode_equals_oracle(enc, data, br):
    fa, sam, rbc, contigs = data
    pb = host.pack_sam(sam, fa, block_reads=br)
    enc.upload_reference(pb.ref)
    payloads, res, _, _ = enc.encode_blocks(pb)
    assert (res["status"] == 0).all(), res
    lines = blockref.mapped_sam_lines(sam)
    for b in range(pb.n_blocks):
        bsam, bfa = blockref.block_alone_inputs(pb, lines, b)
        exp, st = oracle.encode(bsam, bfa, return_stats=True)
        assert payloads[b] == exp and int(res[b]["n_symbols"]) == st.n_symbols, "block %d" % b


def test_gpu_block_decode(enc, built):
    """Decode == the reads (bytes outside ACGTN as N unless equal to the reference), and == the oracle's decoder."""
    fa, sam, rbc, contigs = genome(seed=22, exotic_frac=0.05)
    pb = host.pack_sam(sam, fa, block_reads=1024)
    enc.upload_reference(pb.ref)
    payloads, res, offs, flat = enc.encode_blocks(pb)
    assert (res["status"] == 0).all()
    plan = host.UnpackPlan(pb.container(flat, offs), fa)
    enc.upload_reference(plan.ref)
    recs, seq, dres = enc.decode_blocks(plan)
    assert (dres["status"] == 0).all() and (dres["n_symbols"] == res["n_symbols"]).all()
    want = expected_bases(rbc, contigs)
    assert plan.text(recs, seq) == b"".join(w + b"\n" for w in want)
    assert sum(w != r["seq"] for w, r in zip(want, [r for _, _, rr in rbc for r in rr])) >= 100      # N where SEQ was not
    lines = blockref.mapped_sam_lines(sam)
    for b in (0, pb.n_blocks // 2, pb.n_blocks - 1):
        bsam, bfa = blockref.block_alone_inputs(pb, lines, b)
        text, nr = oracle.decode(payloads[b], bfa)
        first = int(pb.blocks[b]["rec_base"])
        assert text == b"".join(want[first + k] + b"\n" for k in range(nr)) and nr == int(pb.blocks[b]["n_reads"])


def test_cli_compat_on_soft_masked_fasta(data, tmp_path):
    fa, sam, rbc, contigs = data
    (tmp_path / "in.sam").write_bytes(sam); (tmp_path / "ref.fa").write_bytes(fa)
    r = _cli("-c", "1", "--compat", tmp_path / "in.sam", tmp_path / "out.cbc", tmp_path / "ref.fa")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "out.cbc").read_bytes() == oracle.encode(sam, fa)
    r = _cli("-x", tmp_path / "out.cbc", tmp_path / "reads.txt", tmp_path / "ref.fa")
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "reads.txt").read_bytes() == b"".join(w + b"\n" for w in expected_bases(rbc, contigs))


def test_gpu_stream_rescales_chars_row_4(enc, built):
    fa, sam, rbc, contigs = dense_iupac()
    assert row4_snps(rbc, contigs) > 131_072 + 2000             # (2^20 - 41) / 8 symbols rescale a chars row
    pb = host.pack_sam(sam, fa, whole_file=True)
    expect, st = oracle.encode(sam, fa, return_stats=True)
    enc.upload_reference(pb.ref)
    stream, sr = enc.encode_stream(pb)
    assert sr.status == 0 and stream == expect and sr.n_symbols == st.n_symbols
    recs, bases, dr = enc.decode_stream(stream, pb.contigs)
    want = expected_bases(rbc, contigs)
    assert dr.status == 0 and len(recs) == len(want)
    assert all(bases[i, :len(w)].tobytes() == w for i, w in enumerate(want))


def test_gpu_2bit_reference_with_thousands_of_runs(enc, built):
    """The reference at 2 bits per base with its exceptions as runs: single IUPAC bytes, adjacent runs, long gaps."""
    fa, sam, rbc, contigs = dense_iupac()
    pb = host.pack_sam(sam, fa, block_reads=4096)
    rc, rr = host.pack_2bit(pb.ref)
    starts, lens = rr["start"].astype(np.int64), rr["length"].astype(np.int64)
    assert len(rr) > 50_000 and (lens == 1).sum() > 10_000 and lens.max() >= 10_000
    assert (starts[1:] == starts[:-1] + lens[:-1]).sum() > 1000                 # adjacent runs of different bytes
    enc.upload_reference(pb.ref)
    p1, r1, _, _ = enc.encode_blocks(pb)
    assert (r1["status"] == 0).all()
    enc.upload_reference_2bit(rc, rr, len(pb.ref))
    p2, r2, _, _ = enc.encode_blocks(pb)
    assert p2 == p1 and (r2["status"] == 0).all()
    sc, sr = host.pack_2bit(pb.seq)
    assert len(sr) > 1000
    p3, r3, _, _ = enc.encode_blocks_2bit(pb, sc, sr)
    assert p3 == p1 and (r3["status"] == 0).all()


def test_gpu_2bit_encode_with_n_in_every_shared_code_word(enc, built):
    """The chunk-cut shape of test_gpu_2bit_encode_with_cuts_inside_a_code_word (4001 reads per block, three chunks,
    cuts off a 16-byte boundary) with an N at each side of a cut: before it and after it in the code word the two chunks
    share (the earlier chunk expands and patches that word), and in the word after it (the later chunk's first).  One
    pass per side.  Each N is the only N of its read, a read equal to its reference window, and lies over reference A,
    the base the 2-bit code holds under an exception: left unpatched, it turns its read perfect again.  Each pass first
    checks that its N change the 1-byte payloads, then that the 2-bit transport gives the same bytes."""
    from test_chunk_plan import rule, vols
    pb = host.synth(29, 5_000_000, 4_000_000, 150, block_reads=4001)
    vol = vols(pb.n_recs, len(pb.seq), pb.n_tok)[1]
    contiguous, cuts = rule(pb.blocks, pb.n_recs, len(pb.seq), pb.n_tok, vol)
    assert contiguous and len(cuts) >= 3
    rec_blk = np.repeat(np.arange(pb.n_blocks), pb.blocks["n_reads"].astype(np.int64))
    s0 = pb.blocks["seq_base"][rec_blk].astype(np.int64) + pb.recs["seq_off"].astype(np.int64)
    r0 = pb.blocks["ref_off"][rec_blk].astype(np.int64) + pb.recs["pos"].astype(np.int64) - 1
    assert (pb.recs["rlen"] == 150).all() and (np.diff(s0) == 150).all()

    def site(lo, hi):
        """The first byte of [lo, hi) that lies in a read equal to its reference, over reference A: (read, byte) or None."""
        for p in range(lo, hi):
            k = int(np.searchsorted(s0, p, side="right")) - 1
            if (pb.seq[s0[k]:s0[k] + 150] == pb.ref[r0[k]:r0[k] + 150]).all() and pb.ref[r0[k] + p - s0[k]] == ord("A"):
                return k, p
        return None

    passes = {"before the cut": [], "after the cut": [], "word after": []}
    for c in cuts[1:]:
        s = int(pb.blocks["seq_base"][c])
        assert s % 16
        w = s // 16 * 16
        for name, (lo, hi) in zip(passes, ((w, s), (s, w + 16), (w + 16, w + 32))):
            hit = site(lo, hi)
            if hit:
                passes[name].append(hit)
    assert all(passes.values()), passes                     # each side met at one cut at least
    n_pad_runs = len(host.pack_2bit(pb.seq)[1])             # the zero bytes behind the last read
    try:
        enc.upload_reference(pb.ref)
        _, r0_, o0, f0 = enc.encode_blocks(pb, want_payload_list=False)
        assert (r0_["status"] == 0).all()
        for name, hits in passes.items():
            assert len({k for k, _ in hits}) == len(hits)     # one N per read
            for _, p in hits:
                pb.seq[p] = _N
            codes, runs = host.pack_2bit(pb.seq)
            assert len(runs) == n_pad_runs + len(hits)
            _, r1, o1, f1 = enc.encode_blocks(pb, want_payload_list=False)
            assert (r1["status"] == 0).all() and not np.array_equal(f1, f0), name      # the N matter to the payload
            _, r2, o2, f2 = enc.encode_blocks_2bit(pb, codes, runs, want_payload_list=False)
            assert enc.last_e2e()["n_chunks"] >= 3
            assert (r2["status"] == 0).all() and (o2 == o1).all() and np.array_equal(f2, f1), name
            for _, p in hits:
                pb.seq[p] = ord("A")
    finally:
        pb.close()


def test_gpu_2bit_decode_with_more_than_4_n_per_read(enc, built):
    fa, sam, rbc, contigs = synth.genome_dataset(26, (200_000,), (3000,), 100, n_read_frac=0.7)
    want = expected_bases(rbc, contigs)
    n_n = sum(w.count(b"N") for w in want)
    assert n_n > 4 * len(want) and n_n > 1024
    pb = host.pack_sam(sam, fa, block_reads=1024)
    enc.upload_reference(pb.ref)
    _, res, offs, flat = enc.encode_blocks(pb)
    assert (res["status"] == 0).all()
    plan = host.UnpackPlan(pb.container(flat, offs), fa)
    recs, bases, dres, _ = enc.decode_blocks_2bit(plan)
    assert (dres["status"] == 0).all()
    assert all(bases[i, :len(w)].tobytes() == w for i, w in enumerate(want))


def test_gpu_long_reads_on_gapped_reference(enc, built):
    fa, sam, c, crossing = long_genome()
    pb = host.pack_sam(sam, fa, long_reads=True)
    enc.upload_reference(pb.ref)
    gp, gres, offs, flat = enc.encode_long_blocks(pb)
    cp, cres = oracle.cpu_encode_blocks(pb, return_payloads=True, long_reads=True)
    assert (gres["status"] == 0).all()
    for b in range(pb.n_blocks):
        assert gp[b] == cp[b] and int(gres[b]["n_symbols"]) == int(cres[b]["n_symbols"]), b
    plan = host.UnpackPlan(pb.container(flat, offs), fa)
    recs, seq, dres = enc.decode_long_blocks(plan)
    assert (dres["status"] == 0).all()
    assert plan.text(recs, seq) == b"".join(ln.split(b"\t")[9] + b"\n" for ln in sam.splitlines() if not ln.startswith(b"@"))


def test_gpu_tokeniser_and_device_parse(enc, data, tmp_path):
    from test_tokenise import _same
    fa, sam, rbc, contigs = data
    pd, tr = enc.tokenise_sam(sam, fa, fetch=True, block_reads=1024)
    _same(pd, host.pack_sam(sam, fa, block_reads=1024))
    enc.tokenise_free(tr)
    (tmp_path / "in.sam").write_bytes(sam); (tmp_path / "ref.fa").write_bytes(fa)
    outs = []
    for extra in ([], ["--device-parse"]):
        o = tmp_path / ("o%d.cbc" % len(outs))
        r = _cli("-c", tmp_path / "in.sam", o, tmp_path / "ref.fa", "--block-reads", "1000", *extra)
        assert r.returncode == 0, r.stderr
        outs.append(o.read_bytes())
    assert outs[0] == outs[1]


def test_region_starting_inside_an_n_gap(enc, data, tmp_path):
    fa, sam, rbc, contigs = data
    pb = host.pack_sam(sam, fa, block_reads=512)
    recs = rm.records(pb)
    blob = rm.container(pb)
    g0, gl = max((g for g in synth.n_runs(contigs[0][1], 1000) if g[0] > 0), key=lambda g: g[1])
    beg, end = g0 + gl // 2, g0 + gl + 3000                   # 1-based: starts inside the gap, ends past it
    exp = rm.expected_text(recs, 0, beg, end)
    assert exp.count(b"\n") >= 20 and b"NNNN" in exp
    plan = host.UnpackPlan(blob, fa)
    enc.upload_reference(plan.ref)
    text, nsel, sel, res = enc.decode_region(plan, "chr1:%d-%d" % (beg, end), results=True)
    assert (res["status"] == 0).all() and text == exp and nsel == exp.count(b"\n")
    (tmp_path / "in.cbc").write_bytes(blob); (tmp_path / "ref.fa").write_bytes(fa)
    r = _cli("-x", tmp_path / "in.cbc", tmp_path / "out.txt", tmp_path / "ref.fa", "--region", "chr1:%d-%d" % (beg, end))
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "out.txt").read_bytes() == exp
    plan.close()
