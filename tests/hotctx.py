"""Inputs for the hot var context of the block kernels (cbc_encode_body.h: CbcEnc::hot_code -- the context "first edit of a
full-length read, no known SNP ahead", d = L0 + 2, kept as a count table in registers) and the emulation build that counts
what CbcEnc::var_code does (tests/emu/emu_varpaths.cpp).  Used by tests/test_hot_ctx.py on the CPU emulation and
tests/test_hot_ctx_gpu.py on the GPU.  Every case is built once.

As in tests/groupprep.py, the second record of every file carries the case's header read length.  Records are spaced by
more than a read length wherever a case wants the hot context: a record then starts behind every SNP of the records before
it, so its first SNP has no known SNP ahead."""
import ctypes
import functools
import os
import subprocess

import numpy as np

import blockref
import synth
from cbc_amd import host
from groupprep import read, sam_text

_EMU_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")

# order of the CBC_VC_* enum of cbc_encode_body.h
COUNTERS = ["calls", "p0", "hot", "full", "bloom", "scan", "scan_p0"]
MAX_BLOCKS = 64                                 # CBC_VC_MAX_BLOCKS of emu_varpaths.cpp

_lib = None


def var_lib():
    """libcbc_emu_varpaths.so: what libcbc_emu.so exports, with the counters of var_code compiled in, emu_var_counts() and
    the switch emu_var_hot()."""
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", _EMU_DIR, "-f", "varpaths_emu.mk"], stdout=subprocess.DEVNULL)
        L = ctypes.CDLL(os.path.join(_EMU_DIR, "libcbc_emu_varpaths.so"))
        for f in (L.emu_encode_blocks, L.emu_encode_blocks_two_wave):
            f.restype = ctypes.c_int
            f.argtypes = [ctypes.POINTER(blockref.DeviceBatch)]
        L.emu_plan_output.restype = ctypes.c_uint64
        L.emu_plan_output.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
        L.emu_var_counts.restype = ctypes.c_uint32
        L.emu_var_counts.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int]
        L.emu_var_hot.restype = None
        L.emu_var_hot.argtypes = [ctypes.c_int]
        assert L.emu_var_counts(None, 0, 1) == len(COUNTERS)
        _lib = L
    return _lib


def emu_encode_counted(pb, two_wave=False, blocks=None, hot=True):
    """blockref.emu_encode() on the counting build, for all blocks or the listed ones; hot=False: with the hot table switched
    off (every context through the buckets and lists, the form before it).  Returns (payloads, results, counts):
    counts[b][name] = (strand 0, strand 1) of the b-th block coded."""
    L = var_lib()
    bl = pb.blocks.copy() if blocks is None else np.ascontiguousarray(pb.blocks[list(blocks)])
    nb = len(bl)
    assert nb <= MAX_BLOCKS
    total = int(L.emu_plan_output(bl.ctypes.data, nb, pb.recs.ctypes.data, pb.tok.ctypes.data))
    out = np.full(total, 0xAA, dtype=np.uint8)
    res = np.zeros(nb, dtype=host.RESULT_DTYPE)
    db = blockref.DeviceBatch(pb.recs.ctypes.data, pb.seq.ctypes.data, pb.tok.ctypes.data, pb.names.ctypes.data,
                              bl.ctypes.data, nb, pb.ref.ctypes.data, len(pb.ref), out.ctypes.data, total,
                              res.ctypes.data, len(pb.seq), pb.n_tok, pb.n_recs, host.LdsCaps(pb.cap_pos, pb.cap_var))
    L.emu_var_counts(None, 0, 1)
    L.emu_var_hot(1 if hot else 0)
    try:
        rc = (L.emu_encode_blocks_two_wave if two_wave else L.emu_encode_blocks)(ctypes.byref(db))
    finally:
        L.emu_var_hot(1)
    if rc != 0:
        raise RuntimeError("emulation reported an invariant violation (rc=%d)" % rc)
    raw = np.zeros(nb * 2 * len(COUNTERS), dtype=np.uint64)
    L.emu_var_counts(raw.ctypes.data, nb, 1)
    raw = raw.reshape(nb, 2, len(COUNTERS))
    counts = [{name: (int(raw[b, 0, k]), int(raw[b, 1, k])) for k, name in enumerate(COUNTERS)} for b in range(nb)]
    payloads = [out[int(b["out_off"]):int(b["out_off"]) + int(r["nbytes"])].tobytes() for b, r in zip(bl, res)]
    return payloads, res, counts


def _pack(contig, recs, block_reads, name="chr1"):
    fa = synth.fasta_text([(name, contig)])
    return host.pack_sam(sam_text(name, len(contig), recs), fa, block_reads=block_reads)


# ------------------------------------------------------------------------------------------------ 1: overflow
@functools.lru_cache(maxsize=None)
def overflow():
    """2 blocks x 1024 records, L = 150, strands alternating, every record one SNP at read offset 7i mod 150 and no known
    SNP ahead of it: 512 uses of the hot context per strand and block.  Through the buckets that is four times a bucket's 128
    events, and every call behind the overflow scans the global list."""
    rng = np.random.default_rng(3201)
    n, L = 2048, 150
    contig = synth.make_contig(rng, 151 * n + 400)
    recs = [read(rng, contig, 3 + 151 * i, L, flag=16 * (i & 1), subs=[(7 * i) % L]) for i in range(n)]
    return _pack(contig, recs, 1024)


# ------------------------------------------------------------------------------------------------ 2: field neighbours
NEIGHBOUR_OFFSETS = (10, 74, 138, 9, 11)


@functools.lru_cache(maxsize=None)
def field_neighbours():
    """One block of 2048 records, L = 150.  The SNP offsets 10, 74, 138 share lane 10 of the count table (fields 0, 1, 2), 9
    and 11 are its neighbouring lanes; seven records of eight are on strand 0, so each offset is used about 358 times
    there and its field passes 255: a carry into the neighbouring field or a wrong field select changes the bytes."""
    rng = np.random.default_rng(3202)
    n, L = 2048, 150
    contig = synth.make_contig(rng, 151 * n + 400)
    recs = [read(rng, contig, 3 + 151 * i, L, flag=16 * (i % 8 == 7), subs=[NEIGHBOUR_OFFSETS[i % 5]]) for i in range(n)]
    return _pack(contig, recs, n)


# ------------------------------------------------------------------------------------------------ 3: edges of the class
EDGE_LENGTHS = (63, 64, 252, 253, 254)


@functools.lru_cache(maxsize=None)
def edge(L0):
    """One block of 200 records for the header read length L0, every record with one SNP and none known ahead.  63: no
    record is "ordinary", every var symbol comes from edits().  64, 252: the hot table is live.  253, 254: d_hot = L0 + 2
    reaches the unused-half marker 255 and the table is off; a read has at most 252 bases, so the records are those of 252
    under a block header that names the longer length."""
    rng = np.random.default_rng(3300 + L0)
    n, L = 200, min(L0, 252)
    contig = synth.make_contig(rng, (L + 1) * n + 400)
    recs = [read(rng, contig, 3 + (L + 1) * i, L, flag=16 * (i & 1), subs=[(7 * i) % L]) for i in range(n)]
    pb = _pack(contig, recs, n)
    assert pb.n_blocks == 1 and int(pb.blocks["read_length"][0]) == L
    pb.blocks["read_length"][:] = L0
    return pb


# ------------------------------------------------------------------------------------------------ 4: mixed lengths
@functools.lru_cache(maxsize=None)
def mixed_lengths():
    """One block, header length 150: 900 records of length 100, whose "no SNP ahead" context d = 102 goes through its
    bucket, overflows it and spills to the global list as before, and 300 of length 150 (the hot table), interleaved
    three to one; the strand changes every two records.  Both representations live in one stream."""
    rng = np.random.default_rng(3204)
    n = 1200
    contig = synth.make_contig(rng, 151 * n + 400)
    recs = []
    for i in range(n):
        L = 150 if i % 4 == 1 else 100
        recs.append(read(rng, contig, 3 + 151 * i, L, flag=16 * ((i >> 1) & 1), subs=[(7 * i) % L]))
    return _pack(contig, recs, n)


# ------------------------------------------------------------------------------------------------ 5: both call sites
@functools.lru_cache(maxsize=None)
def both_call_sites():
    """One block of 600 records, L = 150.  Every fourth has an indel (an insertion or a deletion in turn) and a SNP in front of
    or behind it and goes through edits(), no known SNP ahead of its first edit; the rest are SNP-only records, coded by
    run_record().  The hot context is fed from both."""
    rng = np.random.default_rng(3205)
    n, L = 600, 150
    contig = synth.make_contig(rng, 160 * n + 400)
    recs = []
    for i in range(n):
        ops = None
        if i % 4 == 2:
            ops = [("M", 60), ("I", 2), ("M", 88)] if i % 8 == 2 else [("M", 70), ("D", 3), ("M", 80)]
        w = (7 * i) % (148 if ops and ops[1][0] == "I" else L)                 # index into the read's M bases
        recs.append(read(rng, contig, 3 + 160 * i, L, flag=16 * (i & 1), subs=[w], ops=ops))
    return _pack(contig, recs, n)


# ------------------------------------------------------------------------------------------------ 6: short blocks
SHORT = {1: (65, 1), 2: (65, 2), 65: (65, 1)}       # records in a block -> (block size, records behind it)


@functools.lru_cache(maxsize=None)
def short_block(n):
    """A batch with a block of exactly n records (1, 2, 65): one full block and a shorter last one, every record with one
    SNP in the hot context."""
    br, tail = SHORT[n]
    rng = np.random.default_rng(3210 + br + tail)
    L, m = 150, br + tail
    contig = synth.make_contig(rng, 151 * m + 400)
    recs = [read(rng, contig, 3 + 151 * i, L, flag=16 * (i & 1), subs=[(5 * i) % L]) for i in range(m)]
    pb = _pack(contig, recs, br)
    assert n in [int(x) for x in pb.blocks["n_reads"]]
    return pb


# ------------------------------------------------------------------------------------------------ 7: the benchmark's own data
CFG2_BLOCKS = (2, 3)


@functools.lru_cache(maxsize=None)
def cfg2_sample():
    """12 blocks of 4096 reads from the packer's generator with the benchmark's seed, coverage and error rates (bench.py,
    cfg2); the tests code blocks 2 and 3."""
    nr = 12 * 4096
    return host.synth(0xCBC00002, nr * 248_956_422 // 10_000_000, nr, 150, 0.003, 0.02, block_reads=4096)
