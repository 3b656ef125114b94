"""Genome-shaped input (tests/synth.py genome_dataset): N gaps at contig ends and inside, IUPAC codes, soft-masked FASTA,
reads with N calls, N over N in both MD forms, bases over IUPAC sites, reads at POS 1 and on a contig's last base.  These
reach chars row 4 (a reference base outside ACGT) and the zero pad behind a contig, which iid ACGT input never does.
CPU part: the kernel bodies on the lock-step emulation against the oracle.  The GPU part is test_genome_shapes_gpu.py."""
import re

import numpy as np
import pytest

import blockref
import synth
from cbc_amd import host
from oracle import oracle

_ACGTN = np.frombuffer(b"ACGTN", dtype=np.uint8)


def genome(seed=21, exotic_frac=0.0):
    """The short-read input of this file and the GPU one: two contigs (the first starts and ends in an N gap)."""
    return synth.genome_dataset(seed, (300_000, 120_000), (4000, 1500), 100, exotic_frac=exotic_frac)


def dense_iupac(seed=23):
    """One stream whose chars row 4 passes the 2^20 rescale: IUPAC at 30 % of the reference bases."""
    return synth.genome_dataset(seed, (400_000,), (16_000,), 100, contig_kw=dict(iupac_rate=0.3, n_gaps=2), n_read_frac=0.2)


def check_features(rbc, contigs):
    """Every edge the generator is there to produce is present, so a later change to it cannot silently drop one."""
    f = synth.genome_features(rbc, contigs)
    assert f["n_gaps"] >= 8 and f["gap_edges_crossed"] >= 30, f
    assert f["iupac_sites_under_reads"] >= 500 and f["md_iupac_letters"] >= 500, f
    assert f["reads_at_pos1"] >= 6 and f["reads_at_end"] >= 6, f
    assert f["reads_over_4n"] >= 100 and f["all_n_reads"] >= 3 and f["nn_pairs"] >= 1000, f
    mds = [r["md"] for _, _, recs in rbc for r in recs]
    assert any(re.search(r"\dN\d", m) for m in mds)                       # N over N listed as a mismatch ...
    assert f["nn_pairs"] > sum(m.count("N") for m in mds) // 2              # ... and folded into match runs
    return f


def decoded_seq(r, contig):
    """The bases a decode gives back for a record: SEQ, with a byte outside ACGTN as N unless it equals its reference
    byte (MD lists it as a mismatch; the SNP's target is chars symbol 4)."""
    seq = np.frombuffer(r["seq"], dtype=np.uint8).copy()
    bad = ~np.isin(seq, _ACGTN)
    if bad.any():
        q, rp = 0, r["pos"] - 1
        for ln, op in re.findall(r"(\d+)([MIDS])", r["cigar"]):
            ln = int(ln)
            if op == "M":
                w = bad[q:q + ln] & (seq[q:q + ln] != contig[rp:rp + ln])
                seq[q:q + ln][w] = ord("N")
                q += ln; rp += ln
            elif op in "IS":
                seq[q:q + ln][bad[q:q + ln]] = ord("N"); q += ln
            else:
                rp += ln
    return seq.tobytes()


def expected_bases(rbc, contigs):
    return [decoded_seq(r, c) for (_, _, recs), (_, c) in zip(rbc, contigs) for r in recs]


def row4_snps(rbc, contigs):
    """SNPs coded against a reference base outside ACGT: MD letters other than ACGT of the records that are not equal to
    their reference window (a byte-equal record is coded as perfect, its MD unread)."""
    n = 0
    for (_, _, recs), (_, c) in zip(rbc, contigs):
        for r in recs:
            if r["cigar"] == "%dM" % len(r["seq"]) and r["seq"] == c[r["pos"] - 1:r["pos"] - 1 + len(r["seq"])].tobytes():
                continue
            n += len(re.findall(r"[^ACGT0-9]", re.sub(r"\^[A-Z]+", "", r["md"])))
    return n


def _block_check(pb, sam, payloads, res):
    lines = blockref.mapped_sam_lines(sam)
    assert len(lines) == pb.n_recs and (res["status"] == 0).all(), res[res["status"] != 0]
    for b in range(pb.n_blocks):
        bsam, bfa = blockref.block_alone_inputs(pb, lines, b)
        exp, st = oracle.encode(bsam, bfa, return_stats=True)
        assert payloads[b] == exp, "block %d" % b
        assert int(res[b]["n_symbols"]) == st.n_symbols


def test_generator_features_and_old_generators_unchanged(built):
    fa, sam, rbc, contigs = genome()
    check_features(rbc, contigs)
    assert re.search(rb"\n[acgtn]{60}\n", fa) and re.search(rb"\n[ACGTN]{60}\n", fa)          # soft-masked FASTA text
    assert fa.startswith(b">chr1\nNNNN") and fa.split(b">chr2")[0].rstrip().endswith(b"NNNN")  # gaps at both ends of chr1
    up = contigs[0][1]
    assert len(synth.n_runs(up, 10)) >= 4 and max(g for _, g in synth.n_runs(up, 10)) >= 30_000
    assert (up[:100] == ord("N")).all() and np.isin(up, synth._IUPAC).sum() > 300
    # the existing seeded inputs are byte-identical to what they were before the genome-shaped additions (digest recorded
    # from the generator as it stood then)
    import hashlib
    fa0, sam0, rbc0, _ = synth.dataset(5, [300000, 120000], [4000, 1500], 150, sub_rate=0.01, indel_frac=0.2,
                                       trailing_s_frac=0.1, dup_pos_frac=0.05)
    h = hashlib.sha256(fa0 + sam0 + synth.sam_text(rbc0, md_last=True))
    h.update(b"".join(synth.shared_variant_dataset(3, 50000, 500, 100, 50, 0.01)))
    assert h.hexdigest() == "b6ba16c19a475e197c7b7fb6d7510d450f9261ca00144dcaa2b5774e96965066"
    assert synth._md_and_nm(np.frombuffer(b"ANGT", dtype=np.uint8), 0, [("M", 4)], np.frombuffer(b"ANCT", dtype=np.uint8)) == ("2G1", 1)
    assert synth._md_and_nm(np.frombuffer(b"ANGT", dtype=np.uint8), 0, [("M", 4)], np.frombuffer(b"ANCT", dtype=np.uint8),
                            mismatch=synth.calmd_mismatch) == ("1N0G1", 2)


@pytest.mark.parametrize("br", [512, 4096])
def test_block_encode_equals_oracle(built, br):
    """Each block's payload == the oracle on the block's own text; == the CPU port of the whole batch."""
    fa, sam, rbc, contigs = genome()
    pb = host.pack_sam(sam, fa, block_reads=br)
    payloads, res = blockref.emu_encode(pb)
    _block_check(pb, sam, payloads, res)
    cp, cres = oracle.cpu_encode_blocks(pb, return_payloads=True)
    assert cp == payloads and (cres["n_symbols"] == res["n_symbols"]).all()


def test_block_encode_with_seq_bytes_outside_acgtn(built):
    """Lower-case and IUPAC bytes in SEQ (the short-read path takes them): encode parity holds, and they decode as N
    unless equal to the reference byte."""
    fa, sam, rbc, contigs = genome(seed=22, exotic_frac=0.05)
    f = check_features(rbc, contigs)
    assert f["exotic_bytes"] >= 300
    assert any(b in r["seq"] for _, _, recs in rbc for r in recs for b in (b"a", b"c", b"g", b"t"))
    pb = host.pack_sam(sam, fa, block_reads=1024)
    payloads, res = blockref.emu_encode(pb)
    _block_check(pb, sam, payloads, res)
    plan = host.UnpackPlan(blockref.container_from_payloads(pb, payloads), fa)
    recs, seq, dres = blockref.emu_decode(plan)
    assert (dres["status"] == 0).all() and (dres["n_symbols"] == res["n_symbols"]).all()
    want = expected_bases(rbc, contigs)
    assert plan.text(recs, seq) == b"".join(w + b"\n" for w in want)
    kept = sum(w.count(b) for w in want for b in b"RYKMSWBDHV")
    assert kept >= 1                                      # an IUPAC read byte equal to its reference byte comes back as itself


def test_block_decode_equals_reads_and_oracle_decoder(built):
    fa, sam, rbc, contigs = genome()
    pb = host.pack_sam(sam, fa, block_reads=1024)
    payloads, res = blockref.emu_encode(pb)
    plan = host.UnpackPlan(blockref.container_from_payloads(pb, payloads), fa)
    recs, seq, dres = blockref.emu_decode(plan)
    assert (dres["status"] == 0).all() and (dres["n_symbols"] == res["n_symbols"]).all()
    want = expected_bases(rbc, contigs)
    assert plan.text(recs, seq) == b"".join(w + b"\n" for w in want)
    lines = blockref.mapped_sam_lines(sam)
    for b in range(pb.n_blocks):
        bsam, bfa = blockref.block_alone_inputs(pb, lines, b)
        text, nr = oracle.decode(payloads[b], bfa)
        first = int(pb.blocks[b]["rec_base"])
        assert nr == int(pb.blocks[b]["n_reads"]) and text == b"".join(want[first + k] + b"\n" for k in range(nr)), b


def test_stream_body_on_soft_masked_fasta(built):
    """The whole-file stream (compat) == the oracle's encode of the SAM with the raw, soft-masked FASTA text."""
    fa, sam, rbc, contigs = genome()
    pb = host.pack_sam(sam, fa, whole_file=True)
    expect, st = oracle.encode(sam, fa, return_stats=True)
    payloads, res = blockref.emu_encode_stream(pb)
    assert int(res[0]["status"]) == 0 and payloads[0] == expect and int(res[0]["n_symbols"]) == st.n_symbols
    recs, bases, dres = blockref.emu_decode_stream(expect, pb.ref, pb.contigs, pb.n_recs + 3)
    want = expected_bases(rbc, contigs)
    assert int(dres["status"]) == 0 and len(recs) == len(want)
    assert all(bases[i, :len(w)].tobytes() == w for i, w in enumerate(want))


def test_stream_body_rescales_chars_row_4(built):
    """Dense IUPAC sites: more than (2^20 - 41) / 8 SNPs against non-ACGT reference bases in one stream, so chars row 4
    is rescaled inside it (counted from the input, so the coverage cannot silently vanish)."""
    fa, sam, rbc, contigs = dense_iupac()
    assert row4_snps(rbc, contigs) > 131_072 + 2000
    pb = host.pack_sam(sam, fa, whole_file=True)
    expect, st = oracle.encode(sam, fa, return_stats=True)
    payloads, res = blockref.emu_encode_stream(pb)
    assert int(res[0]["status"]) == 0 and payloads[0] == expect and int(res[0]["n_symbols"]) == st.n_symbols


def test_tokeniser_core_equals_host_packer(built):
    from test_tokenise import _emu_pack, _same
    for seed, ex in ((21, 0.0), (22, 0.05)):
        fa, sam, _, _ = genome(seed, ex)
        _same(_emu_pack(sam, fa, block_reads=1024), host.pack_sam(sam, fa, block_reads=1024, threads=1))


def long_genome():
    fa, sam, c, crossing = synth.genome_long_dataset(25)
    assert len(crossing) >= 8
    gaps = [g for g in synth.n_runs(c, 200) if 0 < g[0] < len(c) - g[1]]
    assert len(gaps) >= 6 and all(300 <= g[1] <= 900 for g in gaps[:6])
    return fa, sam, c, crossing


def test_long_bodies_on_gapped_reference(built):
    """Long reads over N gaps and IUPAC sites (reads crossing a gap carry bases there: hundreds of mismatches in one M
    run, more than the lane walk holds): encoder body == oracle/cbc_long.c, decode == the reads."""
    fa, sam, c, crossing = long_genome()
    pb = host.pack_sam(sam, fa, long_reads=True)
    ep, eres = blockref.emu_long_encode(pb)
    cp, cres = oracle.cpu_encode_blocks(pb, return_payloads=True, long_reads=True)
    assert (eres["status"] == 0).all() and ep == cp and (eres["n_symbols"] == cres["n_symbols"]).all()
    plan = host.UnpackPlan(blockref.container_from_payloads(pb, ep), fa)
    recs, seq, dres = blockref.emu_long_decode(plan)
    assert (dres["status"] == 0).all()
    assert plan.text(recs, seq) == b"".join(ln.split(b"\t")[9] + b"\n" for ln in sam.splitlines() if not ln.startswith(b"@"))


def test_md_letter_against_an_iupac_reference_byte_is_the_references_behaviour(built):
    """MD text inconsistent with the FASTA: a mismatch whose MD letter is an ACGT base where the reference holds an IUPAC
    code.  The reference's encoder takes the chars row from the MD letter (row 0..3), its decoder from the reference byte
    (row 4), so the file it writes does not decode back.  The block body encodes such input
    exactly as the oracle does, and neither decoder gives the read back."""
    fa, _, rbc, contigs = synth.genome_dataset(24, (60_000,), (400,), 100, contig_kw=dict(n_gaps=0, edge_gaps=False))
    c = contigs[0][1]
    for i, r in enumerate(rbc[0][2]):
        w = c[r["pos"] - 1:r["pos"] + 99]
        iu = np.nonzero(np.isin(w, synth._IUPAC))[0]
        if r["cigar"] == "100M" and len(iu) == 1 and r["md"].count(chr(w[iu[0]])) == 1:
            r["md"] = r["md"].replace(chr(w[iu[0]]), "A" if r["seq"][iu[0]] != ord("A") else "C")
            target = i
            break
    sam = synth.sam_text(rbc)
    pb = host.pack_sam(sam, fa, block_reads=4096)
    payloads, res = blockref.emu_encode(pb)
    _block_check(pb, sam, payloads, res)
    want = b"".join(r["seq"] + b"\n" for r in rbc[0][2])
    try:
        text, _ = oracle.decode(oracle.encode(sam, fa), fa)
    except oracle.OracleError:
        text = None
    assert text != want
    plan = host.UnpackPlan(blockref.container_from_payloads(pb, payloads), fa)
    recs, seq, dres = blockref.emu_decode(plan)
    assert (dres["status"] != 0).any() or plan.text(recs, seq).split(b"\n")[target] != rbc[0][2][target]["seq"]
