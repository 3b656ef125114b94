"""Inputs for the look-ahead tests (tests/test_lookahead.py on the CPU emulation, tests/test_lookahead_gpu.py on the GPU):
the shapes at which the coder wavefront's look-ahead (cbc_encode_body.h: look_ahead -- a group's validation and match test,
run one group before its coding and posted to the model wavefront), the lane writes of the coder (W::set_lane2_uv,
W::set_lane3: every recorded step, every queued symbol) and the quiet rlength[0] step (CbcEnc::step_fixed_quiet) can go wrong.  Every case is a few blocks of at most ~260 records,
except one block of 620 records of one length, and is built once.

The match test takes 8 dwords of every record per round (CHUNK_DW); groups 0 and 1 of a block are tested before anything is
coded, group g + 1 at the top of group g from then on.

As in tests/groupprep.py, the second record of every block carries the case's full read length (the block header's)."""
import functools

import numpy as np

import synth
from cbc_amd import host
from groupprep import read, sam_text, _tokens_of

CHUNK_DW = 8                                   # dwords per round of match_group (cbc_encode_body.h)


def _pack(contig, recs, block_reads, name="chr1"):
    fa = synth.fasta_text([(name, contig)])
    sam = sam_text(name, len(contig), recs)
    return host.pack_sam(sam, fa, block_reads=block_reads), sam


# ------------------------------------------------------------------------------------------------ group counts
GROUP_COUNTS = [63, 64, 65, 128, 129, 192, 193]


@functools.lru_cache(maxsize=None)
def group_count(n):
    """One block of n records, L = 150, every third record with one SNP (position varies), both strands: one group and a
    partial one, exactly full groups and groups one over, up to four groups."""
    rng = np.random.default_rng(500 + n)
    L, clen = 150, 12 * n + 400
    contig = synth.make_contig(rng, clen)
    recs = [read(rng, contig, 3 + 11 * i + int(rng.integers(0, 3)), L, flag=16 * (i & 1), subs=[(7 * i) % L] if i % 3 == 0 else [])
            for i in range(n)]
    return _pack(contig, recs, n)


@functools.lru_cache(maxsize=None)
def one_record_last_block():
    """193 + 1 records in blocks of 193: a block of ONE record behind one with a one-record last group."""
    import groupprep
    fa, sam, br = groupprep.single_record_block(block_reads=193)
    return host.pack_sam(sam, fa, block_reads=br), sam


# ------------------------------------------------------------------------------------------------ read lengths, mismatch positions
READ_LENGTHS = [1, 3, 4, 5, 7, 8, 9, 4 * CHUNK_DW - 1, 4 * CHUNK_DW, 4 * CHUNK_DW + 1, 150, 151, 252]


def _mismatch_sites(L):
    """first dword; last dword of a chunk; first dword of the next chunk; last whole dword; last byte (of the partial dword)"""
    c = 4 * CHUNK_DW
    sites = {0, min(3, L - 1), L - 1}
    if L >= c:
        sites |= {c - 4, c - 1}
    if L > c:
        sites |= {c, min(c + 3, L - 1)}
    if L >= 4:
        sites |= {4 * (L // 4) - 4, 4 * (L // 4) - 1}
    if L >= 150:
        sites |= {4 * CHUNK_DW * 4 - 1, 4 * CHUNK_DW * 4}
    return sorted(sites)


@functools.lru_cache(maxsize=None)
def one_length(L):
    """One block of 200 records (groups 0..3, the last partial), all of length L (the second record, whose length goes into the
    block header, is at least 40 long: the edit-count models' size comes from it).  Records whose ONLY mismatch is at one of
    _mismatch_sites(L), perfect records between them.  A perfect record's bases are followed in the packed buffer by the next
    record's first base and in the reference by the base behind the read: for most of them the two differ, and the record
    must stay a match."""
    rng = np.random.default_rng(9000 + L)
    n, clen = 200, 200 * 6 + L + 80
    contig = synth.make_contig(rng, clen)
    sites = _mismatch_sites(L)
    recs, s = [], 2
    for i in range(n):
        s += int(rng.integers(1, 6))
        subs = [sites[(i // 2) % len(sites)]] if i % 2 and i != 1 else []
        recs.append(read(rng, contig, s, max(L, 40) if i == 1 else L, flag=16 * (i % 3 == 0), subs=subs))
    hidden = sum(1 for a, b in zip(recs, recs[1:]) if a["nm"] == 0 and b["seq"][0] != contig[a["pos"] - 1 + len(a["seq"])])
    assert hidden >= n // 4, hidden
    return _pack(contig, recs, n)


@functools.lru_cache(maxsize=None)
def longest_record_placement():
    """Three blocks of 202 records, lengths 20..60 mixed inside every group, and ONE record of 252 in a later group of the
    block: lane 0 of group 2, lane 63 of group 2, lane 5 of the partial last group (records 192..201).  The number of
    rounds of a group's match test is set by its longest record; every other lane's loads are masked off long before."""
    rng = np.random.default_rng(4242)
    br, clen = 202, 3 * 202 * 7 + 600
    contig = synth.make_contig(rng, clen)
    long_at = {0: 128, 1: 191, 2: 197}
    recs, s = [], 2
    for i in range(3 * br):
        b, k = divmod(i, br)
        L = 252 if k == 1 or k == long_at[b] else 20 + (i * 13) % 41
        s += int(rng.integers(1, 8))
        subs = [L - 1] if i % 4 == 0 and k != 1 else [0] if i % 4 == 2 and k != 1 else []
        recs.append(read(rng, contig, s, L, flag=16 * (i & 1), subs=subs))
    return _pack(contig, recs, br)


# ------------------------------------------------------------------------------------------------ the quiet rlength[0] step
@functools.lru_cache(maxsize=None)
def constant_length_perfect():
    """One block of 620 perfect records of one length: after the first few hundred, nearly every rlength[0] step is quiet
    (it shifts nothing, records nothing and takes no lane), like the same_ref / rlength[1..3] steps."""
    rng = np.random.default_rng(71)
    n, L = 620, 100
    contig = synth.make_contig(rng, 5 * n + 300)
    recs = [read(rng, contig, 2 + 5 * i, L, flag=16 * (i % 2)) for i in range(n)]
    return _pack(contig, recs, 640)


@functools.lru_cache(maxsize=None)
def two_lengths_alternating():
    """260 records alternating between two lengths: both rlength[0] symbols stay far from the model's total, quiet and
    recorded steps mix."""
    rng = np.random.default_rng(72)
    n = 260
    contig = synth.make_contig(rng, 6 * n + 400)
    recs = [read(rng, contig, 2 + 6 * i, 150 if i % 2 else 97, flag=16 * (i % 3 == 0), subs=[i % 90] if i % 5 == 0 and i != 1 else [])
            for i in range(n)]
    return _pack(contig, recs, n)


@functools.lru_cache(maxsize=None)
def first_70():
    """A block of 70 records of one length: the start of a block, where the rlength[0] step still shifts often."""
    rng = np.random.default_rng(73)
    n, L = 70, 150
    contig = synth.make_contig(rng, 9 * n + 300)
    recs = [read(rng, contig, 2 + 9 * i, L, flag=16 * (i % 2), subs=[(3 * i) % L] if i % 4 == 0 else []) for i in range(n)]
    return _pack(contig, recs, n)


CASES = {"one_record_last_block": one_record_last_block, "longest_record_placement": longest_record_placement,
         "constant_length_perfect": constant_length_perfect, "two_lengths_alternating": two_lengths_alternating, "first_70": first_70}
for _n in GROUP_COUNTS:
    CASES["group_count_%d" % _n] = functools.partial(group_count, _n)
for _L in READ_LENGTHS:
    CASES["one_length_%d" % _L] = functools.partial(one_length, _L)


def packed(name):
    return CASES[name]()


# ------------------------------------------------------------------------------------------------ unusable records
PLACES = {"group0": 5, "group1": 100, "group2_first_lane": 128, "group2_last_lane": 191, "group3": 200, "last_partial_group": 299}


def broken_at(kind, place):
    """groupprep.snp_counts() (blocks of 300: groups 0..4, the last one partial) with one record of block 1 made unusable,
    at or just behind record PLACES[place].  Returns (batch, block, record, whether the CPU port refuses it too).
      `length`    read length 255: refused by the coder wavefront's validation of the group (load_group's checks, one
                  group ahead of the coding); the CPU port refuses it too
      `md_count`  a SNP-only record whose header claims 2000 MD tokens: refused by the model wavefront, while the coder
                  wavefront is a group ahead; the CPU port trusts the header, the kernel's contract is CBC_ST_ASSERT there"""
    import groupprep
    fa, sam, br = groupprep.snp_counts()
    pb = host.pack_sam(sam, fa, block_reads=br)
    blk, rec = 1, PLACES[place]
    if kind == "length":
        pb.recs["rlen"][br * blk + rec] = 255
        return pb, blk, rec, True
    assert kind == "md_count"
    n = int(pb.blocks[blk]["n_reads"])
    snp_only = lambda k: _tokens_of(pb, blk, k)[1] > 3 and int(pb.tok[_tokens_of(pb, blk, k)[0] + 1]) == 0   # has MD tokens
    g = rec // 64
    cand = [k for k in list(range(rec, min(64 * g + 64, n))) + list(range(rec - 1, 64 * g - 1, -1)) if k != 1 and snp_only(k)]
    rec = cand[0]
    t, _ = _tokens_of(pb, blk, rec)
    assert int(pb.blocks[blk]["tok_base"]) + int(pb.blocks[blk]["n_tok"]) - t < 2 + 2000
    pb.tok[t] = (int(pb.tok[t]) & 0xffff) | (2000 << 16)
    return pb, blk, rec, False


@functools.lru_cache(maxsize=None)
def _insertion_blocks():
    """Two blocks of 300 records, L = 150: every third record with one SNP, a 2-base deletion now and then, and in every block
    a record with ONE insertion (40M 2I 108M) at each of PLACES -- the records header_at() spoils."""
    rng = np.random.default_rng(1234)
    n, L, br = 600, 150, 300
    contig = synth.make_contig(rng, 11 * n + 400)
    at = set(PLACES.values())
    recs = []
    for i in range(n):
        k = i % br
        s, fl = 3 + 11 * i + int(rng.integers(0, 4)), 16 * (i & 1)
        if k in at:
            recs.append(read(rng, contig, s, L, flag=fl, ops=[("M", 40), ("I", 2), ("M", L - 42)]))
        elif k != 1 and i % 19 == 0:
            recs.append(read(rng, contig, s, L, flag=fl, ops=[("M", 60), ("D", 2), ("M", L - 60)]))
        else:
            recs.append(read(rng, contig, s, L, flag=fl, subs=[(5 * i) % L] if i % 3 == 0 and k != 1 else []))
    return synth.fasta_text([("chr1", contig)]), sam_text("chr1", len(contig), recs), br


def header_at(place):
    """The `header` kind of groupprep.broken at record PLACES[place] of block 1: a record with one insertion whose token
    header and CIGAR token claim 1500 inserted bases.  The model wavefront refuses it while it walks the CIGAR, with queued
    symbols of the record behind it; the CPU port walks the CIGAR and refuses it too.  Returns (batch, block, record, True)."""
    fa, sam, br = _insertion_blocks()
    pb = host.pack_sam(sam, fa, block_reads=br)
    blk, rec = 1, PLACES[place]
    t, _ = _tokens_of(pb, blk, rec)
    assert int(pb.tok[t]) & 0xffff == 3 and int(pb.tok[t + 1]) >> 16 == 2 and int(pb.tok[t + 3]) >> 4 == 2      # 40M 2I 108M
    pb.tok[t + 1] = (int(pb.tok[t + 1]) & 0xffff) | (1500 << 16)
    pb.tok[t + 3] = (int(pb.tok[t + 3]) & 15) | (1500 << 4)
    return pb, blk, rec, True


def unusable(kind, place):
    return header_at(place) if kind == "header" else broken_at(kind, place)


KINDS = ["header", "length", "md_count"]        # groupprep's `md_past_end` is the block's last imperfect record by construction


OUT_FULL_AT = 185                               # where output_full_first()'s block 0 runs out of its payload area
SHRUNK_PAYLOAD = 256                            # bytes of payload area left to block 0 (blockref.emu_encode(shrink_block=0))


def output_full_first(ahead):
    """_insertion_blocks() with block 0's payload area cut to SHRUNK_PAYLOAD bytes: the bit writer stores 64 words at a time,
    so the coder stops with CBC_ST_OUT_FULL at the flush that would pass 256 bytes -- at record OUT_FULL_AT = 185, in group 2
    of the block (the tests check that) -- while a record of group 2 + `ahead` (ahead = 1: record 200, ahead = 2: record 270)
    is unusable (length 255).  Returns (batch, block, unusable record).  Block 1 has room and is coded as ever.  (The CPU port
    lays out its own output area and never runs out of it, so it is no reference for this case: the fused emulation, which
    meets the records in order, is.)"""
    fa, sam, br = _insertion_blocks()
    pb = host.pack_sam(sam, fa, block_reads=br)
    rec = {1: 200, 2: 270}[ahead]
    pb.recs["rlen"][rec] = 255
    return pb, 0, rec


@functools.lru_cache(maxsize=None)
def _sparse():
    """Two blocks of 260 records whose POS deltas are all different (a new alphabet entry per record)."""
    rng = np.random.default_rng(99)
    n, L = 520, 100
    gaps = rng.permutation(np.arange(40, 40 + n))
    contig = synth.make_contig(rng, int(gaps.sum()) + L + 50)
    recs, s = [], 1
    for i in range(n):
        s += int(gaps[i])
        recs.append(read(rng, contig, s, L, flag=16 * (i & 1), subs=[i % L] if i % 3 == 0 and i % 260 != 1 else []))
    return contig, recs


def coder_stops_first(ahead):
    """The coder stops by itself in group 1 of block 0 -- its POS table (cap_pos = 96) is full at the block's 96th new delta,
    record 95 -- while a record of group 1 + `ahead` (ahead = 1: record 130, ahead = 2: record 200) is unusable (length
    255).  Returns (batch, block, unusable record).  Block 1 hits the cap too, with nothing else wrong.  (The CPU port has
    no POS table to fill, so it is no reference for this case: the fused emulation, which meets the records in order, is.)"""
    contig, recs = _sparse()
    pb, _ = _pack(contig, recs, 260)
    assert pb.cap_pos > 96
    pb.cap_pos = 96
    rec = {1: 130, 2: 200}[ahead]
    pb.recs["rlen"][rec] = 255
    return pb, 0, rec
