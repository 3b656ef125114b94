"""The chunks of the host-buffer pipeline (cbc_plan_chunks in cbc_plan.h, exported by the emulation library): the rule
restated in Python, and the 2-bit encode across chunk boundaries that fall inside a code word."""
import ctypes

import numpy as np
import pytest

import blockref
from cbc_amd import gpu, host

MAX_CHUNKS = 8


class Chunk(ctypes.Structure):
    _fields_ = [("b0", ctypes.c_uint32), ("b1", ctypes.c_uint32)] + \
               [(k, ctypes.c_uint64) for k in ("r0", "r1", "s0", "s1", "t0", "t1", "w0", "w1")]


class ChunkPlan(ctypes.Structure):
    _fields_ = [("n_chunks", ctypes.c_uint32), ("contiguous", ctypes.c_uint32), ("c", Chunk * MAX_CHUNKS)]


def plan(blocks, n_recs, seq_bytes, n_tok, vol, split=True):
    L = blockref.emu_lib()
    L.emu_plan_chunks.restype = None
    L.emu_plan_chunks.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                  ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(ChunkPlan)]
    blocks = np.ascontiguousarray(blocks)
    p = ChunkPlan()
    L.emu_plan_chunks(blocks.ctypes.data, len(blocks), n_recs, seq_bytes, n_tok, vol, int(split), ctypes.byref(p))
    return [{k: int(getattr(p.c[c], k)) for k, _ in Chunk._fields_} for c in range(p.n_chunks)], bool(p.contiguous)


def rule(blocks, n_recs, seq_bytes, n_tok, vol):
    """The chunk rule: (contiguous, first block of every chunk)."""
    nb = len(blocks)
    rb, sb, tb = (blocks[k].astype(np.int64) for k in ("rec_base", "seq_base", "tok_base"))
    nr = blocks["n_reads"].astype(np.int64)
    contiguous = (nb > 0 and (rb[1:] == rb[:-1] + nr[:-1]).all() and (sb[1:] >= sb[:-1]).all() and (tb[1:] >= tb[:-1]).all()
                  and rb[0] <= n_recs and rb[-1] + nr[-1] <= n_recs and sb[-1] <= seq_bytes and tb[-1] <= max(n_tok, 1))
    n = 1
    if contiguous and nb >= 512:
        want = min(vol // (64 << 20), MAX_CHUNKS, nb // 256)     # chunks of >= 64 MiB and >= 256 blocks
        if want >= 2:
            n = want
    cuts = [0]
    for c in range(1, n):                                     # the first block at or past an equal share of the records
        target = rb[0] + (rb[-1] + nr[-1] - rb[0]) * c // n
        lo, hi = cuts[-1] + 1, nb - (n - c)
        while lo < hi:
            mid = (lo + hi) // 2
            lo, hi = (mid + 1, hi) if rb[mid] < target else (lo, mid)
        cuts.append(lo)
    return contiguous, cuts


def packed_blocks(n_blocks, reads_per_block, read_len, tok_per_read):
    """A descriptor list laid out as the packers lay it out: records, bases and tokens back to back."""
    b = np.zeros(n_blocks, dtype=host.BLOCK_DTYPE)
    b["n_reads"] = reads_per_block
    b["rec_base"] = np.arange(n_blocks, dtype=np.uint64) * reads_per_block
    b["seq_base"] = b["rec_base"] * read_len
    b["tok_base"] = b["rec_base"] * tok_per_read
    n_recs = n_blocks * reads_per_block
    return b, n_recs, n_recs * read_len, n_recs * tok_per_read


def vols(n_recs, seq_bytes, n_tok):
    """H2D volume at one byte per base and in 2-bit form (encode_blocks_impl)."""
    return n_recs * 16 + seq_bytes + max(n_tok, 1) * 4, n_recs * 16 + seq_bytes // 4 + max(n_tok, 1) * 4


def check_ranges(chunks, n_blocks, n_recs, seq_bytes, n_tok):
    """The chunks partition the blocks; records, bases, tokens and 2-bit words abut and end at the arrays' ends."""
    assert chunks[0]["b0"] == 0 and chunks[-1]["b1"] == n_blocks
    for k in ("r", "s", "t", "w"):
        assert chunks[0][k + "0"] == 0
        for a, b in zip(chunks, chunks[1:]):
            assert a[k + "1"] == b[k + "0"], (k, a, b)
    for a, b in zip(chunks, chunks[1:]):
        assert a["b1"] == b["b0"] and a["b0"] < a["b1"]
    assert chunks[-1]["r1"] == n_recs and chunks[-1]["s1"] == seq_bytes and chunks[-1]["t1"] == n_tok
    assert chunks[-1]["w1"] == (seq_bytes + 15) // 16
    for c in chunks:                                          # a chunk's words hold its last base; the first may be shared
        assert c["w1"] == max(c["w0"], (c["s1"] + 15) // 16)


def test_fewer_than_512_blocks_is_one_whole_chunk(built):
    b, n_recs, seq_bytes, n_tok = packed_blocks(511, 4096, 150, 2)
    chunks, contiguous = plan(b, n_recs, seq_bytes, n_tok, vols(n_recs, seq_bytes, n_tok)[0])
    assert contiguous and len(chunks) == 1
    check_ranges(chunks, 511, n_recs, seq_bytes, n_tok)


@pytest.mark.parametrize("two_bit", [False, True])
def test_cfg2_shape_gives_the_rule_s_chunks(built, two_bit):
    b, n_recs, seq_bytes, n_tok = packed_blocks(2442, 4096, 150, 2)
    vol = vols(n_recs, seq_bytes, n_tok)[1 if two_bit else 0]
    chunks, contiguous = plan(b, n_recs, seq_bytes, n_tok, vol)
    want_contiguous, cuts = rule(b, n_recs, seq_bytes, n_tok, vol)
    assert contiguous and want_contiguous and len(cuts) == MAX_CHUNKS
    assert [c["b0"] for c in chunks] == cuts
    check_ranges(chunks, 2442, n_recs, seq_bytes, n_tok)
    # long reads: one chunk whatever the volume
    one, _ = plan(b, n_recs, seq_bytes, n_tok, vol, split=False)
    assert len(one) == 1
    check_ranges(one, 2442, n_recs, seq_bytes, n_tok)


def test_unaligned_cuts_give_the_shared_word_to_the_earlier_chunk(built):
    b, n_recs, seq_bytes, n_tok = packed_blocks(1000, 4001, 150, 3)
    b["n_reads"][-1] = 3001; n_recs -= 1000; seq_bytes -= 150_000; n_tok -= 3000
    vol = vols(n_recs, seq_bytes, n_tok)[1]
    chunks, _ = plan(b, n_recs, seq_bytes, n_tok, vol)
    assert [c["b0"] for c in chunks] == rule(b, n_recs, seq_bytes, n_tok, vol)[1] and len(chunks) == 3
    assert all(c["s0"] % 16 for c in chunks[1:])
    assert all(c["w0"] == c["s0"] // 16 + 1 for c in chunks[1:])
    check_ranges(chunks, 1000, n_recs, seq_bytes, n_tok)


@pytest.mark.parametrize("breakage", ["rec_gap", "seq_descends", "tok_descends", "past_the_end"])
def test_a_non_contiguous_list_is_one_whole_chunk(built, breakage):
    b, n_recs, seq_bytes, n_tok = packed_blocks(1024, 4096, 150, 2)
    vol = vols(n_recs, seq_bytes, n_tok)[0]
    if breakage == "rec_gap":
        b["rec_base"][600:] += 1; n_recs += 1
    elif breakage == "seq_descends":
        b["seq_base"][600] = b["seq_base"][598]
    elif breakage == "tok_descends":
        b["tok_base"][600] = 0
    else:
        b["n_reads"][-1] += 1
    chunks, contiguous = plan(b, n_recs, seq_bytes, n_tok, vol)
    assert not contiguous and not rule(b, n_recs, seq_bytes, n_tok, vol)[0]
    assert len(chunks) == 1
    c = chunks[0]
    assert (c["b0"], c["b1"], c["r0"], c["r1"], c["s0"], c["s1"], c["t0"], c["t1"]) == (0, 1024, 0, n_recs, 0, seq_bytes, 0, n_tok)
    assert (c["w0"], c["w1"]) == (0, (seq_bytes + 15) // 16)


@pytest.mark.gpu
def test_gpu_2bit_encode_with_cuts_inside_a_code_word(built):
    """Three chunks whose first bases share a code word with the previous chunk's last (150-base reads, 4001 per block):
    the 2-bit transport codes the same bytes as the 1-byte path.  The context's base buffer first holds another batch's
    bases, so a word that no chunk expands, or that an encode reads before its expansion, shows up as a difference."""
    pb = host.synth(29, 5_000_000, 4_000_000, 150, block_reads=4001)
    other = host.synth(31, 5_000_000, 4_000_000, 150, block_reads=4001)
    assert len(other.seq) == len(pb.seq)                      # same arena size: the 2-bit call reuses the dirty buffer
    vol = vols(pb.n_recs, len(pb.seq), pb.n_tok)[1]
    contiguous, cuts = rule(pb.blocks, pb.n_recs, len(pb.seq), pb.n_tok, vol)
    assert contiguous and len(cuts) >= 3
    assert all(int(pb.blocks["seq_base"][c]) % 16 for c in cuts[1:])
    enc = gpu.Encoder(0)
    try:
        enc.upload_reference(other.ref)
        _, ro, _, _ = enc.encode_blocks(other, want_payload_list=False)
        assert (ro["status"] == 0).all()
        enc.upload_reference(pb.ref)
        codes, runs = host.pack_2bit(pb.seq)
        _, r2, o2, f2 = enc.encode_blocks_2bit(pb, codes, runs, want_payload_list=False)
        assert enc.last_e2e()["n_chunks"] >= 3
        _, r1, o1, f1 = enc.encode_blocks(pb, want_payload_list=False)
        assert (r1["status"] == 0).all() and (r2["status"] == 0).all()
        assert (o2 == o1).all() and np.array_equal(f2, f1)
    finally:
        enc.close()
