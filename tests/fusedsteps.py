"""Inputs for the coder's quiet steps (cbc_encode_body.h): the remainder test, CbcEnc::rem_flag2, and the two fused quiet steps
-- CbcEnc::step_sameref_rl0, same_ref + rlength[0], and CbcEnc::step_known0_x3, rlength[1..3]; A/B switches of the kernel build
that the counting emulation defines -- and that emulation build, which counts the paths taken (tests/emu/emu_paths.cpp).  Used by
tests/test_fused_steps.py on the CPU emulation and tests/test_fused_steps_gpu.py on the GPU.  Every case is built once.

As in tests/groupprep.py, the second record of every block carries the case's longest read length (the block header's)."""
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

# order of the CBC_PC_* enum of cbc_encode_body.h
COUNTERS = ["code1", "code1_rem", "code1_rem_exact", "quiet", "quiet_rem", "quiet_rem_exact", "known0", "known0_rem",
            "x3", "x3_exit", "x3_fb_shift", "x3_fb_rem", "sr", "sr_exit", "sr_fb_shift", "sr_fb_rem"]
LATE = 512                                      # CBC_PC_LATE of emu_paths.cpp: the second row counts records from here on

_lib = None


def paths_lib():
    """libcbc_emu_paths.so: what libcbc_emu.so exports, with the fused quiet steps and the path counters compiled in, and
    emu_path_counts()."""
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", _EMU_DIR, "-f", "paths_emu.mk"], stdout=subprocess.DEVNULL)
        L = ctypes.CDLL(os.path.join(_EMU_DIR, "libcbc_emu_paths.so"))
        for f in (L.emu_encode_blocks, L.emu_encode_blocks_two_wave):
            f.restype = ctypes.c_int
            f.argtypes = [ctypes.POINTER(blockref.DeviceBatch)]
        L.emu_plan_output.restype = ctypes.c_uint64
        L.emu_plan_output.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
        L.emu_path_counts.restype = ctypes.c_uint32
        L.emu_path_counts.argtypes = [ctypes.c_void_p, ctypes.c_int]
        assert L.emu_path_counts(None, 1) == len(COUNTERS)
        _lib = L
    return _lib


def emu_encode_counted(pb, two_wave=False, blocks=None):
    """blockref.emu_encode() on the counting build, for all blocks or the listed ones.  Returns (payloads, results, counts):
    counts[name] = (records below LATE, records from LATE on) summed over the blocks coded."""
    L = paths_lib()
    bl = pb.blocks.copy() if blocks is None else np.ascontiguousarray(pb.blocks[list(blocks)])
    nb = len(bl)
    total = int(L.emu_plan_output(bl.ctypes.data, nb, pb.recs.ctypes.data, pb.tok.ctypes.data))
    out = np.full(total, 0xAA, dtype=np.uint8)
    res = np.zeros(nb, dtype=host.RESULT_DTYPE)
    db = blockref.DeviceBatch(pb.recs.ctypes.data, pb.seq.ctypes.data, pb.tok.ctypes.data, pb.names.ctypes.data,
                              bl.ctypes.data, nb, pb.ref.ctypes.data, len(pb.ref), out.ctypes.data, total,
                              res.ctypes.data, len(pb.seq), pb.n_tok, pb.n_recs, host.LdsCaps(pb.cap_pos, pb.cap_var))
    L.emu_path_counts(None, 1)
    rc = (L.emu_encode_blocks_two_wave if two_wave else L.emu_encode_blocks)(ctypes.byref(db))
    if rc != 0:
        raise RuntimeError("emulation reported an invariant violation (rc=%d)" % rc)
    raw = np.zeros(2 * len(COUNTERS), dtype=np.uint64)
    L.emu_path_counts(raw.ctypes.data, 1)
    counts = {name: (int(raw[k]), int(raw[len(COUNTERS) + k])) for k, name in enumerate(COUNTERS)}
    payloads = [out[int(b["out_off"]):int(b["out_off"]) + int(r["nbytes"])].tobytes() for b, r in zip(bl, res)]
    return payloads, res, counts


def _pack(contig, recs, block_reads, name="chr1"):
    fa = synth.fasta_text([(name, contig)])
    return host.pack_sam(sam_text(name, len(contig), recs), fa, block_reads=block_reads)


# ------------------------------------------------------------------------------------------------ 1: one length
@functools.lru_cache(maxsize=None)
def one_length():
    """2 blocks x 1024 records, L = 150, every third record with one SNP, both strands: rlength[0] sits next to its model's
    total, so both fused forms take their fused exit on most records and fall back on some.  (The seed is one at which
    block 0 has 50 fallbacks by a remainder flag in either form: about 48 are expected, three low words at 1 in 64 each.)"""
    rng = np.random.default_rng(1505)
    n, L = 2048, 150
    contig = synth.make_contig(rng, 9 * n + 400)
    recs = [read(rng, contig, 3 + 9 * i + int(rng.integers(0, 3)), L, flag=16 * (i & 1),
                 subs=[(7 * i) % L] if i % 3 == 0 and i % 1024 != 1 else []) for i in range(n)]
    return _pack(contig, recs, 1024)


# ------------------------------------------------------------------------------------------------ 2: several lengths
def _lengths(lens, seed):
    rng = np.random.default_rng(seed)
    n = 700
    contig = synth.make_contig(rng, 7 * n + 600)
    recs = []
    for i in range(n):
        L = lens[i % len(lens)]
        recs.append(read(rng, contig, 2 + 7 * i, L, flag=16 * (i % 3 == 0), subs=[i % L] if i % 5 == 0 and i != 1 and L > 1 else []))
    return _pack(contig, recs, n)


@functools.lru_cache(maxsize=None)
def two_lengths():
    """700 records alternating 150 / 151 (record 1: 151): rlength[0]'s symbols have half the model each, the step shifts on
    most records, and same_ref + rlength[0] falls back to the single steps."""
    return _lengths((150, 151), 1502)


@functools.lru_cache(maxsize=None)
def three_lengths():
    """700 records of lengths 150, 252, 1 in turn (record 1: 252)."""
    return _lengths((150, 252, 1), 1503)


# ------------------------------------------------------------------------------------------------ 3: escapes
@functools.lru_cache(maxsize=None)
def escapes():
    """700 records whose POS deltas are all distinct for the first 80 records (every record an escape: the Esc / Look
    instantiations of the record body, the fused forms next to pos_alpha()) and then repeat (deltas seen before, in changing
    order: plain records with an escape-free run between two looks)."""
    rng = np.random.default_rng(1504)
    n, L = 700, 150
    first = [int(x) for x in rng.permutation(np.arange(20, 100))]
    gaps = first + [first[int(rng.integers(0, 80))] for _ in range(n - 80)]
    contig = synth.make_contig(rng, sum(gaps) + L + 60)
    recs, s = [], 1
    for i in range(n):
        s += gaps[i]
        recs.append(read(rng, contig, s, L, flag=16 * (i & 1), subs=[(11 * i) % L] if i % 3 == 0 and i != 1 else []))
    return _pack(contig, recs, n)


# ------------------------------------------------------------------------------------------------ 4: short blocks
SHORT = {1: (65, 1), 2: (65, 2), 63: (64, 63), 64: (64, 63), 65: (65, 1)}      # records in a block -> (block size, records behind it)


@functools.lru_cache(maxsize=None)
def short_block(n):
    """A batch with a block of exactly n records (1, 2, 63, 64, 65): one full block and a shorter last one.  Record 0 alone,
    then the fused forms with thr0 straight after the peeled first record."""
    br, tail = SHORT[n]
    rng = np.random.default_rng(1510 + br + tail)
    L, m = 150, br + tail
    contig = synth.make_contig(rng, 8 * m + 400)
    recs = [read(rng, contig, 2 + 8 * i, L, flag=16 * (i & 1), subs=[(5 * i) % L] if i % 3 == 0 and i % br != 1 else []) for i in range(m)]
    pb = _pack(contig, recs, br)
    assert n in [int(x) for x in pb.blocks["n_reads"]]
    return pb


# ------------------------------------------------------------------------------------------------ 6: a block that stops
STOP_CAP_POS = 96
STOP_FROM = 520


@functools.lru_cache(maxsize=None)
def _stops():
    rng = np.random.default_rng(1506)
    n, L = 1400, 150
    gaps = []
    for i in range(n):
        k = i % 700
        gaps.append(5 + (k % 4) if i >= 700 or k < STOP_FROM else 40 + k)         # block 0: a new delta per record from STOP_FROM on
    contig = synth.make_contig(rng, sum(gaps) + L + 1060)
    recs, s = [], 1000                                        # the first record's own delta is like no other
    for i in range(n):
        s += gaps[i]
        recs.append(read(rng, contig, s, L, flag=16 * (i & 1), subs=[(3 * i) % L] if i % 3 == 0 and i % 700 != 1 else []))
    return contig, recs


def pos_table_full():
    """Two blocks of 700 records, cap_pos lowered to STOP_CAP_POS.  Block 0 meets four POS deltas in turn up to record
    STOP_FROM - 1 and a new one with every record from there on, so its POS table is full at a record beyond 600; block 1
    keeps to four deltas and is coded whole.  Returns (batch, block that stops, record it stops at): the record is the one
    that brings the block's STOP_CAP_POS-th distinct delta, counted here from the packed POS values (tests/lookahead.py,
    coder_stops_first: all deltas distinct, cap_pos = 96, stops at record 95)."""
    contig, recs = _stops()
    pb = _pack(contig, recs, 700)
    assert pb.cap_pos > STOP_CAP_POS
    pb.cap_pos = STOP_CAP_POS
    pos = [int(x) for x in pb.recs["pos"][:700]]
    seen, stop = set(), None
    for i in range(700):
        seen.add(pos[i] - (pos[i - 1] if i else 0))
        if len(seen) == STOP_CAP_POS:
            stop = i
            break
    assert stop is not None and stop > 600
    return pb, 0, stop


# ------------------------------------------------------------------------------------------------ 5 (GPU): the 6-wave kernel
def many_blocks(n_blocks):
    """n_blocks blocks of 640 records from the packer's own generator (L = 150): with more than ten blocks per CU the
    library launches the 6-waves-per-SIMD build of the kernel."""
    return host.synth(0xF05ED, 30_000_000, 640 * n_blocks, 150, block_reads=640)
