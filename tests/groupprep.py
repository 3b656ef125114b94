"""Inputs for the group-pass tests (tests/test_group_prep.py on the CPU emulation, tests/test_group_prep_gpu.py on the
GPU): the shapes at which the lane-per-record match test and the group pass of the model wavefront (token headers as lane
masks, the counted SNP-count model) of cbc_encode_body.h can go wrong.  Every case is small (a few hundred reads, blocks of 200..300) and is built once.

A block's header read length is the SEQ length of its SECOND record (get_read_length, sam_file_allocation.c:26-79), for
the packed file and for the oracle's run on the block alone, so every case keeps that record at the case's full length."""
import functools

import numpy as np

import synth
from cbc_amd import host

_ACGT = synth._ACGT


def _alt(rng, base):
    k = int(np.where(_ACGT == base)[0][0]) if base in _ACGT else 0
    return _ACGT[(k + int(rng.integers(1, 4))) % 4]


def read(rng, contig, s, L, flag=0, subs=(), ops=None):
    """One record at 0-based start s.  subs: indices into the read's M bases that get a substitution.  ops: CIGAR as
    [(op, len)] over M / I / D (default one M of length L)."""
    ops = ops or [("M", L)]
    parts, mpos, rpos, qpos = [], [], s, 0
    for op, ln in ops:
        if op == "M":
            parts.append(contig[rpos:rpos + ln].copy()); mpos.extend(range(qpos, qpos + ln)); rpos += ln; qpos += ln
        elif op == "I":
            parts.append(_ACGT[rng.integers(0, 4, size=ln)]); qpos += ln
        else:
            rpos += ln
    seq = np.concatenate(parts)
    assert len(seq) == L
    for w in subs:
        seq[mpos[w]] = _alt(rng, seq[mpos[w]])
    md, nm = synth._md_and_nm(contig, s, ops, seq)
    return dict(pos=s + 1, flag=flag, cigar="".join("%d%s" % (ln, op) for op, ln in ops), seq=seq.tobytes(), md=md, nm=nm)


def sam_text(name, clen, recs):
    out = [b"@HD\tVN:1.6\tSO:coordinate\n", ("@SQ\tSN:%s\tLN:%d\n" % (name, clen)).encode()]
    for i, r in enumerate(recs):
        out.append(b"%s\t%d\t%s\t%d\t60\t%s\t*\t0\t0\t%s\t%s\tMD:Z:%s\tNM:i:%d\n" % (
            r.get("qname", "r%d" % i).encode(), r["flag"], name.encode(), r["pos"], r["cigar"].encode(), r["seq"],
            b"I" * len(r["seq"]), r["md"].encode(), r["nm"]))
    return b"".join(out)


# ------------------------------------------------------------------------------------------------ match test
LENGTHS = [252, 1, 2, 3, 4, 5, 6, 7, 8, 9, 150, 151, 149, 148, 251, 250, 249, 100, 33, 34, 35, 36, 63, 64, 65, 127, 128, 129,
           252, 17, 18, 19, 20, 200, 201, 202, 203]


@functools.lru_cache(maxsize=None)
def mixed_lengths(n_reads, block_reads=200):
    """Read lengths mixed inside every group over 1..252 (every rl mod 4, rl < 4, rl = 252); records whose only mismatch is
    the first base, or the last; perfect records in between (what follows a record's bases in the packed buffer is the next
    record's first base, what follows in the reference is the base behind it: the tail mask has to hide both).  The last
    record ends on the contig's last base and is the last of the packed buffers.  Returns (fasta, sam, block_reads)."""
    rng = np.random.default_rng(1000 + n_reads)
    clen = 8 * n_reads + 600
    contig = synth.make_contig(rng, clen)
    recs, s = [], 3
    for i in range(n_reads):
        L = 252 if i % block_reads == 1 else LENGTHS[(i * 7 + i // 37) % len(LENGTHS)]
        s += int(rng.integers(0, 9))
        if i == n_reads - 1:
            s = clen - L
        kind = i % 5
        subs = [0] if kind == 1 else [L - 1] if kind == 2 else sorted(set(int(x) for x in rng.integers(0, L, size=2))) if kind == 4 else []
        recs.append(read(rng, contig, s, L, flag=16 * (i % 3 == 0), subs=subs))
    hidden = sum(1 for a, b in zip(recs, recs[1:]) if a["nm"] == 0 and len(a["seq"]) % 4 and a["pos"] - 1 + len(a["seq"]) < clen
                 and b["seq"][0] != contig[a["pos"] - 1 + len(a["seq"])])
    assert hidden >= n_reads // 8, hidden
    assert recs[-1]["pos"] - 1 + len(recs[-1]["seq"]) == clen
    return synth.fasta_text([("chrM", contig)]), sam_text("chrM", clen, recs), block_reads


@functools.lru_cache(maxsize=None)
def single_record_block(block_reads=200):
    """block_reads + 1 records: the last block holds ONE record.  get_read_length() of a one-record file is the length of its
    text line, so the record's name is padded until the line of the block-alone run is as long as the file's read length."""
    rng = np.random.default_rng(77)
    L0, clen = 150, 4000
    contig = synth.make_contig(rng, clen)
    recs = [read(rng, contig, 5 + 9 * i, L0, flag=16 * (i % 2), subs=[i % L0] if i % 3 == 0 else []) for i in range(block_reads)]
    last = read(rng, contig, 5 + 9 * block_reads, 21, subs=[20])
    fa = synth.fasta_text([("chr1", contig)])
    import blockref
    for pad in range(1, 120):
        last["qname"] = "q" * pad
        sam = sam_text("chr1", clen, recs + [last])
        pb = host.pack_sam(sam, fa, block_reads=block_reads)
        bsam, _ = blockref.block_alone_inputs(pb, blockref.mapped_sam_lines(sam), pb.n_blocks - 1)
        if len(bsam) == L0:
            return fa, sam, block_reads
    raise AssertionError("no name length makes the line %d bytes long" % L0)


# ------------------------------------------------------------------------------------------------ SNP counts, SNP positions
@functools.lru_cache(maxsize=None)
def snp_counts():
    """L = 150, blocks of 300: a group where most records carry exactly one SNP; counts of 4 and more (the wave-sum path of
    dense_lookup); a read with 70 SNPs (not "ordinary"); reads with indels between SNP-only reads; SNPs at base 0 and at
    the last base, both strands; an all-perfect and an all-imperfect stretch of whole groups."""
    rng = np.random.default_rng(2024)
    L, n, clen = 150, 700, 9000
    contig = synth.make_contig(rng, clen)
    recs = []
    for i in range(n):
        s = 4 + 11 * i + int(rng.integers(0, 5))
        fl = 16 * (i & 1)
        g = i // 64
        if i % 300 == 1 or g == 2:                                  # the header record; group 2: all perfect
            subs, ops = [], None
        elif g == 0:                                                # mostly one SNP
            subs, ops = ([] if i % 9 == 0 else [int(rng.integers(0, L))]), None
        elif g == 1:                                                # 4..12 SNPs
            subs, ops = sorted(set(int(x) for x in rng.integers(0, L, size=4 + i % 9))), None
        elif g == 3:                                                # all imperfect, indels between SNP-only reads
            if i % 3 == 0:
                o, k = 20 + i % 50, 1 + i % 3
                ops = [("M", o), ("I", k), ("M", L - o - k)] if i % 2 else [("M", o), ("D", k), ("M", L - o)]
                subs = [5, 100] if i % 6 == 0 else []
            else:
                subs, ops = [0] if i % 3 == 1 else [L - 1], None       # first / last base
        elif i == 300 + 17:
            subs, ops = list(range(0, 140, 2)), None                    # 70 SNPs
        else:
            k = int(rng.integers(0, 4))
            subs, ops = sorted(set(int(x) for x in rng.integers(0, L, size=k))), None
            if i % 17 == 0:
                ops = [("M", 40), ("D", 2), ("M", L - 40)]
            if i == 400:                                            # the record broken() spoils
                ops = [("M", 40), ("I", 2), ("M", L - 42)]
        recs.append(read(rng, contig, s, L, flag=fl, subs=subs, ops=ops))
    return synth.fasta_text([("chr1", contig)]), sam_text("chr1", clen, recs), 300


@functools.lru_cache(maxsize=None)
def perfect_and_imperfect_blocks():
    """Blocks of 200: one all perfect, one all imperfect, one mixed (90 records)."""
    rng = np.random.default_rng(31)
    L, clen = 100, 6000
    contig = synth.make_contig(rng, clen)
    recs = []
    for i in range(490):
        b = i // 200
        subs = [] if b == 0 else [int(rng.integers(0, L))] * (1 if b == 1 or i % 2 else 0)
        recs.append(read(rng, contig, 2 + 10 * i, L, flag=16 * (i % 2), subs=subs))
    return synth.fasta_text([("chr1", contig)]), sam_text("chr1", clen, recs), 200


@functools.lru_cache(maxsize=None)
def short_reads_L50():
    """L = 50 < 64: no record is "ordinary", every one goes through the general form with a counted SNP-count symbol."""
    fa, sam, _, _ = synth.dataset(50, [30000], [600], 50, sub_rate=0.02, indel_frac=0.1)
    return fa, sam, 250


@functools.lru_cache(maxsize=None)
def genome_shaped():
    """N and IUPAC letters in reads and reference (chars rows and symbols 4), reads on gap edges and contig ends."""
    fa, sam, _, _ = synth.genome_dataset(61, contig_lens=(60_000,), reads_per_contig=(900,), L=100, sub_rate=0.01,
                                         contig_kw=dict(n_gaps=4, max_gap=3000, iupac_rate=0.01, n_rate=0.003))
    return fa, sam, 400


@functools.lru_cache(maxsize=None)
def many_cigar_tokens():
    """Records whose MD tokens lie behind more than 62 CIGAR tokens -- token index 64 and up, past the 64 prefetched lanes:
    SNP-only records with the M run cut into 75 pieces, and a record of 32 one-base insertions."""
    rng = np.random.default_rng(8)
    L, clen = 150, 5000
    contig = synth.make_contig(rng, clen)
    recs = []
    for i in range(260):
        s, fl = 3 + 12 * i, 16 * (i % 2)
        if i % 20 == 7:
            recs.append(read(rng, contig, s, L, flag=fl, subs=[0, 77, L - 1][:1 + i % 3], ops=[("M", 2)] * 75))
        elif i % 20 == 13:
            recs.append(read(rng, contig, s, L, flag=fl, subs=[3], ops=[("M", 3), ("I", 1)] * 32 + [("M", L - 128)]))
        else:
            recs.append(read(rng, contig, s, L, flag=fl, subs=[i % L] if i % 2 else []))
    return synth.fasta_text([("chr1", contig)]), sam_text("chr1", clen, recs), 260


CASES = {
    "snp_counts": snp_counts, "perfect_and_imperfect_blocks": perfect_and_imperfect_blocks, "short_reads_L50": short_reads_L50,
    "genome_shaped": genome_shaped, "many_cigar_tokens": many_cigar_tokens, "single_record_block": single_record_block,
}
for _n in (63, 64, 65, 130):
    CASES["mixed_lengths_%d" % (200 + _n)] = functools.partial(mixed_lengths, 200 + _n)


@functools.lru_cache(maxsize=None)
def packed(name):
    fa, sam, br = CASES[name]()
    return host.pack_sam(sam, fa, block_reads=br), sam


# ------------------------------------------------------------------------------------------------ failures
def _tokens_of(pb, blk, k):
    """(index into pb.tok of the token header, number of tokens) of record k of block blk; 0 tokens = a perfect record."""
    bd = pb.blocks[blk]
    first, n = int(bd["rec_base"]), int(bd["n_reads"])
    off = int(pb.recs[first + k]["tok_off"])
    end = int(pb.recs[first + k + 1]["tok_off"]) if k + 1 < n else int(bd["n_tok"])
    return int(bd["tok_base"]) + off, end - off


def broken(kind):
    """A packed batch (blocks of 300) with one record of block 1 made unusable.  Returns (batch, block, record, whether the CPU
    port refuses it too).
      `header`       record 100, in the middle of a group, has one insertion; its token header and its CIGAR token claim 1500
                     inserted bases (the CPU port walks the CIGAR and refuses it as well)
      `length`       record 100 has read length 255, whose low byte is outside the alphabet of rlength[0] (the CPU port too)
      `md_count`     a SNP-only record in the middle of a group whose header claims 2000 MD tokens
      `md_past_end`  the last imperfect record of the block, SNP-only, claims 63 MD tokens: fewer than 64, so only the bounds
                     of the block's token area keep it from being taken for an ordinary record
    The CPU port trusts the two counts of a SNP-only record's header (it stops at the read's end), so for the last two the
    expectation is the kernel's own contract: CBC_ST_ASSERT at that record (include/cbc_gpu.h)."""
    fa, sam, br = snp_counts()
    pb = host.pack_sam(sam, fa, block_reads=br)
    blk, rec, cpu_too = 1, 100, True
    r = br * blk + rec
    if kind == "header":
        t, _ = _tokens_of(pb, blk, rec)
        n_cig = int(pb.tok[t]) & 0xffff
        assert n_cig == 3 and int(pb.tok[t + 1]) >> 16 == 2 and int(pb.tok[t + 3]) >> 4 == 2      # 40M 2I 108M
        pb.tok[t + 1] = (int(pb.tok[t + 1]) & 0xffff) | (1500 << 16)
        pb.tok[t + 3] = (int(pb.tok[t + 3]) & 15) | (1500 << 4)
    elif kind == "length":
        pb.recs["rlen"][r] = 255
    else:
        n = int(pb.blocks[blk]["n_reads"])
        snp_only = lambda k: _tokens_of(pb, blk, k)[1] > 0 and int(pb.tok[_tokens_of(pb, blk, k)[0] + 1]) == 0
        if kind == "md_count":
            rec = next(k for k in range(105, 125) if snp_only(k))
            claim = 2000
        else:
            rec = next(k for k in range(n - 1, 0, -1) if _tokens_of(pb, blk, k)[1] > 0)
            assert snp_only(rec)
            claim = 63
        t, ntok = _tokens_of(pb, blk, rec)
        assert int(pb.blocks[blk]["tok_base"]) + int(pb.blocks[blk]["n_tok"]) - t < 2 + claim      # runs past the block's tokens
        pb.tok[t] = (int(pb.tok[t]) & 0xffff) | (claim << 16)
        cpu_too = False
    return pb, blk, rec, cpu_too
