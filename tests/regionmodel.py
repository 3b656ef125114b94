"""Region decode in plain Python, from the packed arrays (the packer's view of every record): the model the tests hold
cbc_unpack_region, the span decode and the region text against."""
import numpy as np

import synth
from cbc_amd import host
from oracle import oracle


def container(pb):
    """Block container of a packed batch, coded by the CPU port (no GPU)."""
    flat, offs, res = oracle.cpu_encode_blocks(pb, return_flat=True)
    assert (res["status"] == 0).all(), res
    return pb.container(flat, offs)


def records(pb):
    """Per record: block, contig, POS (contig coordinate), span, SEQ bytes.  span = rlen for a read whose SEQ equals its
    reference window (the encoder codes it as perfect), else rlen + nDel - nIns with the counts of token word 1 (the
    encoder codes each as one byte)."""
    out = []
    for b in range(pb.n_blocks):
        bd, inf = pb.blocks[b], pb.info[b]
        c = int(inf["contig"])
        ws = int(inf["window_start"])
        ref0 = int(pb.contigs[c]["ref_off"])
        for k in range(int(bd["n_reads"])):
            r = pb.recs[int(bd["rec_base"]) + k]
            rl = int(r["rlen"])
            s0 = int(bd["seq_base"]) + int(r["seq_off"])
            seq = pb.seq[s0:s0 + rl].tobytes()
            pos = ws + int(r["pos"])
            w1 = int(pb.tok[int(bd["tok_base"]) + int(r["tok_off"]) + 1])
            perfect = seq == pb.ref[ref0 + pos - 1: ref0 + pos - 1 + rl].tobytes()
            span = rl if perfect else rl + (w1 & 0xff) - ((w1 >> 16) & 0xff)
            out.append((b, c, pos, span, seq))
    return out


def selected(recs, contig, beg, end):
    return [r for r in recs if r[1] == contig and r[2] <= end and r[2] + r[3] - 1 >= beg]


def expected_text(recs, contig, beg, end):
    return b"".join(r[4] + b"\n" for r in selected(recs, contig, beg, end))


def expected_blocks(pb, contig, beg, end, smax):
    """[b0, b1) by the rule of include/cbc_host.h: F(b) <= END and (last block of the contig or F(next) >= BEG - SMAX + 1)."""
    bs = [b for b in range(pb.n_blocks) if int(pb.info[b]["contig"]) == contig]
    if not bs:
        return None
    F = {b: int(pb.info[b]["window_start"]) + 1 for b in bs}
    need = [b for i, b in enumerate(bs) if F[b] <= end and (i == len(bs) - 1 or F[bs[i + 1]] >= beg - smax + 1)]
    return (need[0], need[-1] + 1) if need else None


def mixed_dataset(seed, contig_lens, reads_per_contig, lengths=(100, 150), gap_tail=0, **kw):
    """Reads of several lengths on every contig (merged in position order), optionally none in the last `gap_tail`
    bases of each contig.  Returns (fasta, records_by_contig, contigs)."""
    rng = np.random.default_rng(seed)
    contigs, rbc = [], []
    for ci, (clen, nr) in enumerate(zip(contig_lens, reads_per_contig)):
        name = "chr%d" % (ci + 1)
        c = synth.make_contig(rng, clen)
        recs = []
        for L in lengths:
            recs += synth.make_reads(rng, c, nr // len(lengths), L, max_start=clen - max(lengths) - 8 - gap_tail, **kw)
        recs.sort(key=lambda r: r["pos"])
        contigs.append((name, c))
        rbc.append((name, clen, recs))
    return synth.fasta_text(contigs), rbc, contigs


def deletion_read(contig, pos, m1=50, d=40, m2=50):
    """A read at `pos` whose CIGAR m1 M, d D, m2 M reaches d bases further on the reference than its length."""
    p = pos - 1
    seq = contig[p:p + m1].tobytes() + contig[p + m1 + d:p + m1 + d + m2].tobytes()
    md = "%d^%s%d" % (m1, contig[p + m1:p + m1 + d].tobytes().decode(), m2)
    return dict(pos=pos, flag=0, cigar="%dM%dD%dM" % (m1, d, m2), seq=seq, md=md, nm=d)


def pack(fasta, rbc, block_reads):
    return host.pack_sam(synth.sam_text(rbc), fasta, block_reads=block_reads, var_length=True)
