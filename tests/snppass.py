"""Inputs for the SNP run-pass tests (tests/test_snp_pass.py on the CPU emulation, tests/test_snp_pass_gpu.py on the GPU):
the shapes at which run_pass() of cbc_encode_body.h -- positions, var contexts, chars symbols and snpInRef marks of a run
of ordinary records, one lane per SNP -- can go wrong, and a plain model of snpInRef over the SAM lines that says what
each shape really holds, so that no case can go trivial.  Every case is a few hundred reads in blocks of 200 (see
tests/groupprep.py for the helpers and for why the second record of every block keeps the case's full read length).

snpInRef (read_compression.c:589, 703-718): every SNP marks the position POS + p - 1, p = the sum of (gap + 1) over the
record's MD mismatches so far (matched bases only: deleted bases do not count); a SNP asks for the first mark in
[POS + p_before, POS + rl).  Marks are only ever set, and the window starts empty in every block."""
import functools
import re

import numpy as np

import groupprep
import synth
from cbc_amd import host

BLOCK = 200


# ------------------------------------------------------------------------------------------------ model
def md_gaps(md):
    """Gaps (matched bases since the previous mismatch) of the MD mismatches, in order."""
    gaps, run = [], 0
    for num, dele, mis in re.findall(r"(\d+)|(\^[A-Za-z]+)|([A-Za-z])", md):
        if num:
            run += int(num)
        elif mis:
            gaps.append(run); run = 0
    return gaps


def snp_events(sam, block_reads=BLOCK):
    """One dict per SNP in stream order: rec (index in the file), blk, k, pos, rl, q (absolute query start), mark (absolute
    position it marks), found (absolute position of the mark it reports, or None), beyond (the first mark at or after q,
    wherever it lies, or None)."""
    out = []
    for r, ln in enumerate(groupprep_lines(sam)):
        f = ln.split(b"\t")
        if r % block_reads == 0:
            marks = set()
        pos, rl = int(f[3]), len(f[9])
        md = [x for x in f[11:] if x.startswith(b"MD:Z:")][0][5:].decode().strip()
        p = 0
        for k, g in enumerate(md_gaps(md)):
            q = pos + p
            ahead = [m for m in marks if m >= q]
            beyond = min(ahead) if ahead else None
            found = beyond if beyond is not None and p < rl and beyond < pos + rl else None
            p += g + 1
            out.append(dict(rec=r, blk=r // block_reads, k=k, pos=pos, rl=rl, q=q, mark=pos + p - 1, found=found, beyond=beyond,
                            indel=f[5] != b"%dM" % rl))
            marks.add(pos + p - 1)
    return out


def groupprep_lines(sam):
    return [ln for ln in sam.splitlines() if ln and not ln.startswith(b"@")]


def overtaken(ev, within=3):
    """SNPs that report an older mark although a LATER record (at most `within` records on, same block) marks a position
    between their query start and that mark."""
    n = 0
    for i, e in enumerate(ev):
        if e["found"] is None:
            continue
        for l in ev[i + 1:]:
            if l["rec"] > e["rec"] + within or l["blk"] != e["blk"]:
                break
            if l["rec"] > e["rec"] and e["q"] <= l["mark"] < e["found"]:
                n += 1
                break
    return n


def _full(i, L, lengths):
    return L if i % BLOCK == 1 else lengths[i % len(lengths)]


# ------------------------------------------------------------------------------------------------ shapes
@functools.lru_cache(maxsize=None)
def shared_sites():
    """Variant sites every 40 bp carried by every covering read, both strands, reads of 50..150 bp; a read that ends one
    base before a site carries a private SNP on its last base (the mark one past the read must not be reported)."""
    rng = np.random.default_rng(401)
    n, clen, L = 400, 2600, 150
    contig = synth.make_contig(rng, clen)
    lengths = [50 + (i * 37) % 101 for i in range(101)]
    recs = []
    for i in range(n):
        s, ln = 2 + 5 * i, _full(i, L, lengths)
        subs = [x - s for x in range(17, clen, 40) if s <= x < s + ln]
        if (s + ln) % 40 == 17 and ln - 1 not in subs:
            subs.append(ln - 1)
        recs.append(groupprep.read(rng, contig, s, ln, flag=16 * (i % 2), subs=sorted(subs)))
    sam = groupprep.sam_text("chr1", clen, recs)
    ev = snp_events(sam)
    assert sum(e["found"] is not None for e in ev) >= 50
    assert any(e["found"] == e["q"] for e in ev)                                         # d = 0
    assert any(e["found"] == e["pos"] + e["rl"] - 1 for e in ev)                         # the mark on the read's last base
    assert any(e["found"] is None and e["beyond"] == e["pos"] + e["rl"] for e in ev)     # a mark one past it: not found
    return synth.fasta_text([("chr1", contig)]), sam, BLOCK


@functools.lru_cache(maxsize=None)
def order_in_run():
    """Pairs of records with equal POS or POS one apart whose SNPs interleave: the first carries the shared sites (marked
    by earlier records), the second private SNPs a few bases in front of them -- marks that the first must not see."""
    rng = np.random.default_rng(402)
    n, clen, L = 300, 2400, 120
    contig = synth.make_contig(rng, clen)
    recs = []
    for i in range(n):
        pair, second = i // 2, i % 2
        s = 4 + 12 * pair + (second if pair % 2 else 0)
        sites = [x - s for x in range(31, clen, 50) if s <= x < s + L]
        if second:
            subs = sorted(set(x - 3 - pair % 5 for x in sites if x - 3 - pair % 5 >= 0) | set(x + 10 for x in sites if x + 10 < L))
        else:
            subs = sorted(set(sites) | set(x + 20 for x in sites if x + 20 < L))
        recs.append(groupprep.read(rng, contig, s, L, flag=16 * (pair % 2), subs=subs))
    sam = groupprep.sam_text("chr1", clen, recs)
    ev = snp_events(sam)
    assert overtaken(ev, within=1) >= 5, overtaken(ev, within=1)
    return synth.fasta_text([("chr1", contig)]), sam, BLOCK


@functools.lru_cache(maxsize=None)
def run_limits():
    """Records of 9 SNPs (the 8th of them holds a run's 64th and 65th SNP); a record with 63 SNPs and one with 70 (not
    ordinary); groups with far more than 64 SNPs; records 64..127 of block 1 all start inside 100 bp."""
    rng = np.random.default_rng(403)
    n, clen, L = 400, 4200, 150
    contig = synth.make_contig(rng, clen)
    recs, s = [], 3
    for i in range(n):
        dense = 200 + 64 <= i < 200 + 128
        s += 1 if dense else 9
        if i % BLOCK == 1:
            subs = []
        elif i == 30:
            subs = list(range(0, 126, 2))                       # 63 SNPs: ordinary
        elif i == 40:
            subs = list(range(0, 140, 2))                       # 70 SNPs: not ordinary
        elif i < 128:
            subs = [3 + 16 * k + i % 5 for k in range(9)]       # 9 each
        elif dense:
            subs = sorted(set([(i * 7) % L] + ([(i * 7 + 50) % L] if i % 2 else [])))
        else:
            subs = sorted(set(int(x) for x in rng.integers(0, L, size=i % 4)))
        recs.append(groupprep.read(rng, contig, s, L, flag=16 * (i % 3 == 0), subs=subs))
    sam = groupprep.sam_text("chr1", clen, recs)
    lines = groupprep_lines(sam)
    span = [int(lines[i].split(b"\t")[3]) for i in (264, 327)]
    assert span[1] - span[0] < 100
    ev = snp_events(sam)
    per_rec = np.bincount([e["rec"] for e in ev], minlength=n)
    assert per_rec[30] == 63 and per_rec[40] == 70 and (per_rec[2:30] == 9).all()
    assert all(per_rec[g:g + 64].sum() > 64 for g in (0, 64, 264))
    # group 0 by the encoder's rule (a run: consecutive ordinary records, at most 64 SNPs): some record that does not fit
    # holds the 64th and the 65th SNP counted from its run's start, and opens the next run
    straddles, cum = 0, 0
    for n_snp in per_rec[:64]:
        if not 0 < n_snp < 64:
            cum = 0 if n_snp else cum                               # a perfect record is skipped, any other one ends the run
            continue
        if cum + n_snp > 64:
            straddles += cum < 64
            cum = 0
        cum += n_snp
    assert straddles >= 2, straddles
    return synth.fasta_text([("chr1", contig)]), sam, BLOCK


@functools.lru_cache(maxsize=None)
def indels_between():
    """Shared sites every 30 bp; every 7th record carries an insertion or a deletion in front of its SNPs (the bases of an
    insertion shift the read byte against the marked position): its SNPs are searched against the run before it and the
    run after it sees its marks."""
    rng = np.random.default_rng(404)
    n, clen, L = 300, 2600, 120
    contig = synth.make_contig(rng, clen)
    recs = []
    for i in range(n):
        s = 5 + 8 * i
        ops, shift = None, 0
        if i % 7 == 3 and i % BLOCK != 1:
            k = 1 + i % 3
            if i % 2:
                ops, shift = [("M", 12), ("I", k), ("M", L - 12 - k)], 0
            else:
                ops, shift = [("M", 12), ("D", k), ("M", L - 12)], k
        nm = L - (ops[1][1] if ops and ops[1][0] == "I" else 0)      # M bases of the read
        subs = []
        for x in range(11, clen, 30):                                # index into the M bases of the site's base
            w = x - s
            if 12 <= w < 12 + shift:
                continue                                             # a deleted base
            if w >= 12:
                w -= shift
            if 0 <= w < nm:
                subs.append(w)
        if i % 5 == 2:
            subs.append(nm - 1)
        recs.append(groupprep.read(rng, contig, s, L, flag=16 * (i % 2), subs=sorted(set(subs)), ops=ops))
    sam = groupprep.sam_text("chr1", clen, recs)
    ev = snp_events(sam)
    by_rec = {}
    for e in ev:
        by_rec.setdefault(e["rec"], []).append(e)
    ind = sorted(r for r, es in by_rec.items() if es[0]["indel"])
    assert len(ind) >= 30
    assert sum(any(e["found"] is not None for e in by_rec[r]) for r in ind) >= 20       # searched against the run before
    marks_of_indels = set(e["mark"] for r in ind for e in by_rec[r])
    assert sum(e["found"] in marks_of_indels for e in ev if not e["indel"]) >= 50
    return synth.fasta_text([("chr1", contig)]), sam, BLOCK


@functools.lru_cache(maxsize=None)
def jumps():
    """265 records (blocks of 200 and 65): neighbours more than 256 bp apart inside a group and between two runs, a group
    spanning more than 2000 bp, and a site marked by record 63 of a block that record 64 (the next group's first) reports."""
    rng = np.random.default_rng(405)
    n, clen, L = 265, 16000, 100
    contig = synth.make_contig(rng, clen)
    recs, s = [], 10
    for i in range(n):
        s += 300 if i % 16 == 5 else 700 if i % 64 == 40 else 2 if i % BLOCK == 64 else 6
        subs = [] if i % BLOCK == 1 else [x - s for x in range(s - s % 25 + 25, s + L, 25) if x - s < L]
        ops = None
        if i % 16 == 6 and subs:                                    # the record after a jump is now and then not ordinary
            ops, subs = [("M", 50), ("D", 1), ("M", L - 50)], [x for x in subs if x < 50]
        recs.append(groupprep.read(rng, contig, s, L, flag=16 * (i % 2), subs=subs, ops=ops))
    sam = groupprep.sam_text("chr1", clen, recs)
    pos = [int(ln.split(b"\t")[3]) for ln in groupprep_lines(sam)]
    assert pos[63] - pos[0] > 2000 and any(b - a > 256 for a, b in zip(pos[:64], pos[1:64]))
    ev = snp_events(sam)
    m63 = set(e["mark"] for e in ev if e["rec"] == 63)
    assert m63 and any(e["rec"] == 64 and e["found"] in m63 for e in ev)
    return synth.fasta_text([("chr1", contig)]), sam, BLOCK


CASES = {"shared_sites": shared_sites, "order_in_run": order_in_run, "run_limits": run_limits, "indels_between": indels_between,
         "jumps": jumps, "single_record_block": groupprep.single_record_block}


@functools.lru_cache(maxsize=None)
def packed(name):
    fa, sam, br = CASES[name]()
    pb = host.pack_sam(sam, fa, block_reads=br)
    if name == "jumps":
        assert [int(x) for x in pb.blocks["n_reads"]] == [200, 65]
    if name == "single_record_block":
        assert int(pb.blocks["n_reads"][-1]) == 1
    return pb, sam


# ------------------------------------------------------------------------------------------------ spoilt tokens
def runs_of_group(pb, blk, g):
    """The runs of group g of block blk by the encoder's rule, as lists of record numbers, from the packed tokens."""
    n = int(pb.blocks[blk]["n_reads"])
    runs, cur, cum = [], [], 0
    for rec in range(64 * g, min(64 * g + 64, n)):
        t, ntok = groupprep._tokens_of(pb, blk, rec)
        if ntok == 0:
            continue                                                # a perfect record
        n_md = int(pb.tok[t]) >> 16
        if int(pb.tok[t + 1]) != 0 or n_md >= 64:                   # not ordinary: ends the run
            if cur:
                runs.append(cur)
            cur, cum = [], 0
            continue
        if cum + n_md > 64:
            runs.append(cur)
            cur, cum = [], 0
        cur.append(rec); cum += n_md
    if cur:
        runs.append(cur)
    return runs


def spoilt(kind):
    """shared_sites with one MD token of a record in the middle of a run of block 1 spoilt.  Returns (batch, block, record).
      `gap`       its second SNP's gap becomes L0 (outside the var model's alphabet)
      `past_end`  a record of 60..100 bases whose second SNP's gap becomes 140 (below L0 = 150): the token lies past the
                  read's end"""
    fa, sam, br = shared_sites()
    pb = host.pack_sam(sam, fa, block_reads=br)
    blk = 1
    bd = pb.blocks[blk]
    L0, first = int(bd["read_length"]), int(bd["rec_base"])
    assert L0 == 150
    for rec in range(70, 120):                                      # inside group 1 of the block, ordinary neighbours
        t, ntok = groupprep._tokens_of(pb, blk, rec)
        if ntok == 0 or int(pb.tok[t + 1]) != 0:
            continue
        n_cig, n_md, rl = int(pb.tok[t]) & 0xffff, int(pb.tok[t]) >> 16, int(pb.recs["rlen"][first + rec])
        if n_md >= 2 and (kind == "gap" or 60 <= rl <= 100):
            run = [r for r in runs_of_group(pb, blk, rec // 64) if rec in r][0]      # taken before the token is spoilt
            if run[0] == rec or run[-1] == rec:
                continue                                            # the middle of a run, not its head or its tail
            w = t + 2 + n_cig + 1
            pb.tok[w] = ((L0 if kind == "gap" else 140) << 8) | (int(pb.tok[w]) & 0xff)
            return pb, blk, rec
    raise AssertionError("no record to spoil")


# ------------------------------------------------------------------------------------------------ chars guard
CHARS_GUARD_AT = 600          # cbc_amd/csrc/Makefile, libcbc_gpu_charsguard.so: the run pass's chars guard of the test builds


def chars_guard_runs(sam, block_reads=BLOCK, guard=CHARS_GUARD_AT):
    """(runs coded in counting form, runs coded by small_code) of a build whose chars guard stands at `guard`: the encoder's
    rule replayed on the SAM lines.  A chars row (the reference letter of the SNP) starts a block at a total of 41 (33 for
    a letter outside ACGT: sam_models.c:372-401) and gains 8 per SNP, whoever codes it; a run (consecutive ordinary records
    of a group of 64, at most 64 SNPs) is counted unless a row it touches stands at `guard` - 8 * (the run's SNPs) or more."""
    counted = fallback = 0
    rows, run, cum = {}, [], 0

    def close():
        nonlocal counted, fallback, run, cum
        if run:
            if any(rows.get(x, 41 if x in "ACGT" else 33) + 8 * len(run) >= guard for x in run):
                fallback += 1
            else:
                counted += 1
            for x in run:
                rows[x] = rows.get(x, 41 if x in "ACGT" else 33) + 8
        run, cum = [], 0

    for r, ln in enumerate(groupprep_lines(sam)):
        if r % block_reads == 0:
            close(); rows = {}
        if (r % block_reads) % 64 == 0:
            close()
        f = ln.split(b"\t")
        md = [x for x in f[11:] if x.startswith(b"MD:Z:")][0][5:].decode().strip()
        letters = [m for _, d, m in re.findall(r"(\d+)|(\^[A-Za-z]+)|([A-Za-z])", md) if m]
        letters = [x if x in "ACGT" else "N" for x in letters]
        if f[5] == b"%dM" % len(f[9]) and not letters:
            continue                                                 # a perfect record
        if f[5] != b"%dM" % len(f[9]) or len(letters) >= 64:       # not ordinary: edits() codes it, its SNPs by small_code
            close()
            for x in letters:
                rows[x] = rows.get(x, 41 if x in "ACGT" else 33) + 8
            continue
        if cum + len(letters) > 64:
            close()
        run += letters; cum += len(letters)
    close()
    return counted, fallback


def emu_encode_chars_guard(pb, two_wave=False):
    """blockref.emu_encode on a build of the emulation with the lowered guard (built beside the ordinary one)."""
    import ctypes
    import os
    import subprocess
    import blockref
    d = blockref._EMU_DIR
    lib = os.path.join(d, "libcbc_emu_charsguard.so")
    srcs = [os.path.join(d, "emu_encode.cpp"), os.path.join(d, "wave_emu.h"),
            os.path.join(d, "..", "..", "cbc_amd", "csrc", "cbc_encode_body.h"), os.path.join(d, "..", "..", "cbc_amd", "csrc", "cbc_plan.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(x) > os.path.getmtime(lib) for x in srcs):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wno-unused-function", "-fPIC", "-fvisibility=hidden", "-pthread",
                               "-DCBC_CHARS_GUARD_AT=%du" % CHARS_GUARD_AT, "-shared", "-o", lib, "emu_encode.cpp"], cwd=d)
    blockref.emu_lib()
    L = ctypes.CDLL(lib)
    L.emu_encode_blocks.restype = ctypes.c_int
    L.emu_encode_blocks.argtypes = [ctypes.POINTER(blockref.DeviceBatch)]
    L.emu_plan_output.restype = ctypes.c_uint64
    L.emu_plan_output.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    saved, blockref._emu = blockref._emu, L
    try:
        return blockref.emu_encode(pb, two_wave=two_wave)
    finally:
        blockref._emu = saved
