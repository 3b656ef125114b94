"""The hot var context of the block kernels (cbc_encode_body.h: CbcEnc::hot_code -- d = L0 + 2 as a count table in registers,
outside the buckets, the filter and the global list) on the CPU lock-step emulation: the fused form and the two-thread form
against the CPU port (oracle.cpu_encode_blocks) on the same packed batch -- payload bytes, status, fail_read, nbytes of every
block, n_symbols of every block that was coded -- and the counts of what var_code did, from the counting build of
tests/emu/emu_varpaths.cpp, with the table and with its switch off (the form before it).  Shapes: tests/hotctx.py; the GPU
counterpart is tests/test_hot_ctx_gpu.py."""
import pytest

import hotctx
from oracle import oracle


def check_blocks(payloads, res, wantp, want):
    """payload bytes, status, fail_read, nbytes of every block; n_symbols of every block that was coded (that of a failed
    block is unspecified: include/cbc_gpu.h)"""
    for field in ("status", "fail_read", "nbytes"):
        assert [int(x) for x in res[field]] == [int(x) for x in want[field]], field
    ok = want["status"] == 0
    assert (res["n_symbols"][ok] == want["n_symbols"][ok]).all()
    assert payloads == wantp


def both_forms_equal_cpu_port(pb, blocks=None, hot=True):
    """Whatever the CPU port reports, status included, is the answer.  Returns the counts (the same in both forms)."""
    wantp, want = oracle.cpu_encode_blocks(pb, blocks=blocks, return_payloads=True)
    counts = None
    for two_wave in (False, True):
        payloads, res, c = hotctx.emu_encode_counted(pb, two_wave=two_wave, blocks=blocks, hot=hot)
        check_blocks(payloads, res, wantp, want)
        assert counts is None or c == counts
        counts = c
    return counts


def tot(c, name):
    return sum(c[name])


@pytest.mark.timeout(300)
def test_overflow(built):
    """512 uses of the hot context per strand and block.  With the table: none of them in a bucket, no p = 0 scan.  With the
    switch off the same input fills buckets 0 and 8 four times over and scans the list at least 250 times per block."""
    pb = hotctx.overflow()
    assert [int(x) for x in pb.blocks["n_reads"]] == [1024, 1024]
    counts = both_forms_equal_cpu_port(pb)
    before = both_forms_equal_cpu_port(pb, hot=False)
    for b in range(2):
        print("block %d with the table:" % b, counts[b], "without:", before[b])
        assert counts[b]["hot"][0] >= 400 and counts[b]["hot"][1] >= 400
        assert tot(counts[b], "scan_p0") == 0 and tot(counts[b], "full") == 0
        assert tot(before[b], "hot") == 0 and tot(before[b], "scan") >= 250
        assert counts[b]["calls"] == before[b]["calls"] and counts[b]["p0"] == before[b]["p0"]


@pytest.mark.timeout(300)
def test_field_neighbours(built):
    """Each of the offsets 10, 74, 138, 9, 11 at least 300 times on strand 0: three fields of one lane and a field of each
    neighbouring lane pass 255."""
    pb = hotctx.field_neighbours()
    assert [int(x) for x in pb.blocks["n_reads"]] == [2048]
    per = {o: sum(1 for i in range(2048) if i % 8 != 7 and hotctx.NEIGHBOUR_OFFSETS[i % 5] == o) for o in hotctx.NEIGHBOUR_OFFSETS}
    assert min(per.values()) >= 300, per
    counts = both_forms_equal_cpu_port(pb)
    assert counts[0]["hot"] == (1792, 256) and tot(counts[0], "scan_p0") == 0


@pytest.mark.timeout(300)
@pytest.mark.parametrize("L0", hotctx.EDGE_LENGTHS)
def test_edges_of_the_class(built, L0):
    """Header lengths 63 (every call from edits()), 64 and 252 (table live), 253 and 254 (d_hot >= 255: table off)."""
    pb = hotctx.edge(L0)
    assert [int(x) for x in pb.blocks["n_reads"]] == [200] and int(pb.blocks["read_length"][0]) == L0
    counts = both_forms_equal_cpu_port(pb)
    print(L0, counts[0])
    if L0 <= 252:
        assert tot(counts[0], "hot") == 200 and tot(counts[0], "calls") == 200
    else:
        assert tot(counts[0], "hot") == 0 and tot(counts[0], "p0") == 200


@pytest.mark.timeout(300)
def test_mixed_lengths(built):
    """900 records of length 100 through bucket, overflow and list (d = 102), 300 of length 150 through the table."""
    pb = hotctx.mixed_lengths()
    assert [int(x) for x in pb.blocks["n_reads"]] == [1200] and int(pb.blocks["read_length"][0]) == 150
    counts = both_forms_equal_cpu_port(pb)
    c = counts[0]
    print(c)
    assert tot(c, "hot") == 300 and tot(c, "p0") == 1200
    assert tot(c, "full") >= 600 and tot(c, "scan_p0") >= 600       # 450 events per strand in a bucket of 128


@pytest.mark.timeout(300)
def test_both_call_sites(built):
    """150 records with an indel through edits(), 450 SNP-only records through run_record(): 600 uses of the table, and the
    indels' own var symbols beside them."""
    pb = hotctx.both_call_sites()
    assert [int(x) for x in pb.blocks["n_reads"]] == [600]
    counts = both_forms_equal_cpu_port(pb)
    c = counts[0]
    print(c)
    assert tot(c, "hot") == 600
    assert tot(c, "calls") == 600 + 75 * 2 + 75 * 3                  # an insertion of 2, a deletion of 3: one symbol per base


@pytest.mark.timeout(300)
@pytest.mark.parametrize("n", sorted(hotctx.SHORT))
def test_short_blocks(built, n):
    pb = hotctx.short_block(n)
    counts = both_forms_equal_cpu_port(pb)
    assert sum(tot(c, "hot") for c in counts) == pb.n_recs


@pytest.mark.timeout(300)
def test_cfg2_blocks_scan_less_than_a_quarter(built):
    """Blocks 2 and 3 of the benchmark's own data, 4096 reads each: bytes equal the CPU port's, and the scans of the global
    list drop below a quarter of what the same build makes with the table switched off.  (Counted when this was written:
    494 -> 88 and 478 -> 97.)"""
    pb = hotctx.cfg2_sample()
    blocks = list(hotctx.CFG2_BLOCKS)
    assert [int(pb.blocks["n_reads"][b]) for b in blocks] == [4096, 4096]
    wantp, want = oracle.cpu_encode_blocks(pb, blocks=blocks, return_payloads=True)
    assert (want["status"] == 0).all()
    payloads, res, counts = hotctx.emu_encode_counted(pb, blocks=blocks)
    check_blocks(payloads, res, wantp, want)
    payloads, res, c2 = hotctx.emu_encode_counted(pb, blocks=blocks, two_wave=True)
    check_blocks(payloads, res, wantp, want)
    assert c2 == counts
    payloads, res, before = hotctx.emu_encode_counted(pb, blocks=blocks, hot=False)
    check_blocks(payloads, res, wantp, want)
    for k in range(2):
        print("block %d with the table:" % blocks[k], counts[k], "without:", before[k])
        assert tot(before[k], "hot") == 0 and tot(counts[k], "hot") > 0 and tot(counts[k], "scan_p0") < tot(before[k], "scan_p0")
        assert 4 * tot(counts[k], "scan") < tot(before[k], "scan")
