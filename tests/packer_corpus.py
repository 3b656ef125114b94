"""A seeded corpus of small SAM files at the edges of the per-line rule (column split, CIGAR scan, MD scan, replay), and
the recorder of tests/golden/packer_quirks.json: what the host packer made of every file BEFORE its parsing moved into
cbc_tok_core.h.  tests/test_packer_quirks.py holds the packer, the emulated device path and the GPU to that record.

    python tests/packer_corpus.py --write-dir DIR                   the files, as DIR/<name>.sam and DIR/<name>.fa
    python tests/packer_corpus.py --record LIB --label HASH --tok   rewrite the fixture from the libcbc_host.so at LIB
                                                                    (--tok: and the device path's status from tests/emu)
"""
import hashlib
import json
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import synth  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "packer_quirks.json")
ARRAYS = ("recs", "seq", "tok", "blocks", "info", "names", "contigs")
SCALARS = ("cap_pos", "cap_var", "read_length", "n_bases", "n_skipped_unmapped")
PERFECT = b"MD:Z:100"


def _split(sam):
    ls = sam.splitlines(keepends=True)
    n = sum(1 for l in ls if l.startswith(b"@"))
    return ls[:n], ls[n:]


def _edit(line, fn):
    """fn(list of columns) -> list of columns, on one line that keeps its '\\n'"""
    return b"\t".join(fn(line.rstrip(b"\n").split(b"\t"))) + b"\n"


def _set(col, val):
    return lambda f: f[:col] + [val(f[col]) if callable(val) else val] + f[col + 1:]


def _md(val):
    return lambda f: [(b"MD:Z:" + (val(c[5:]) if callable(val) else val)) if c.startswith(b"MD:Z:") else c for c in f]


def _drop_md(f):
    return [c for c in f if not c.startswith(b"MD:Z:")]


def _flag(line):
    return int(line.split(b"\t")[1])


def _perfect_pairs(body):
    """indices i whose line and whose previous line are perfect reads (an MD-less line i then inherits a text that fits)"""
    return [i for i in range(1, len(body)) if PERFECT in body[i] and PERFECT in body[i - 1]]


def _clip_records(seed, kinds):
    """One record per entry of kinds, all with a leading soft clip unless 'plain':
    'perfect' the bases behind the clip match; 'snp' one mismatch in the middle; 'last' the mismatch is the last base, so the
    text the packer derives ends in a letter and is not terminated; 'junk' as 'last' with a long MD of its own, whose tail
    then follows the derived text; 'less' a perfect read without an MD field (it inherits whatever the buffer holds)."""
    rng = np.random.default_rng(seed)
    contig = synth.make_contig(rng, 20000)
    A, L, pos, recs = synth._ACGT, 100, 50, []
    for kind in kinds:
        pos += int(rng.integers(1, 30))
        if kind in ("plain", "less"):
            recs.append(dict(pos=pos, flag=0, cigar="100M", seq=contig[pos - 1:pos - 1 + L].tobytes(), md="100", nm=0, less=kind == "less"))
            continue
        k = int(rng.integers(1, 6))
        body = contig[pos - 1:pos - 1 + L - k].copy()
        md = str(L - k)
        if kind != "perfect":
            q = L - k - 1 if kind in ("last", "junk") else int(rng.integers(5, L - k - 5))
            old = body[q]
            body[q] = A[(int(np.where(A == old)[0][0]) + 1) % 4]
            md = "%d%s%d" % (q, chr(old), L - k - q - 1)
            if kind == "junk":
                md = "10A10C10G10T10A10C10G7"
        seq = np.concatenate([A[rng.integers(0, 4, size=k)], body]).tobytes()
        recs.append(dict(pos=pos, flag=16 if len(recs) % 3 == 0 else 0, cigar="%dS%dM" % (k, L - k), seq=seq, md=md, nm=0, less=False))
    sam = synth.sam_text([("chrS", 20000, recs)])
    head, body = _split(sam)
    body = [_edit(l, _drop_md) if r["less"] else l for l, r in zip(body, recs)]
    return synth.fasta_text([("chrS", contig)]), b"".join(head + body)


def _numeral(digits, low):
    """a numeral of `digits` digits; up to 14 digits its low 32 bits are `low` (20 digits: beyond 2^63, atoi saturates)"""
    if digits == 20:
        return b"%d" % (2 ** 64 + low)
    k = {10: 1, 11: 20, 14: 3000}[digits]
    v = k * 2 ** 32 + low
    assert len(str(v)) == digits
    return b"%d" % v


def corpus():
    """-> list of (name, fasta, sam, pack_sam keywords).  Deterministic."""
    out = []

    def add(name, fa, head, body, **kw):
        kw.setdefault("block_reads", 16)
        sam = b"".join(head + body) if isinstance(body, list) else body
        assert sam.count(b"\n") <= 300
        out.append((name, fa, sam, kw))

    fa, sam, rbc, _ = synth.dataset(101, [20000], [40], 100, sub_rate=0.02, indel_frac=0.3)
    head, body = _split(sam)
    fa_p, sam_p, rbc_p, _ = synth.dataset(102, [20000, 9000], [40, 12], 100, sub_rate=0.003, indel_frac=0.0, flags=(0, 16, 4))
    head_p, body_p = _split(sam_p)
    pairs = _perfect_pairs(body_p)
    assert len(pairs) > 12
    mapped = [i for i in pairs if not _flag(body_p[i]) & 4]          # ... and the line itself is a mapped record
    assert len(mapped) > 8

    # ---- the column split
    b = [l.replace(b"\t60\t", b"\t\t60\t") if i % 3 == 0 else l for i, l in enumerate(body)]
    b[4] = b"\t" + b[4]; b[5] = b[5].rstrip(b"\n") + b"\t\t\n"
    add("tabs_consecutive", fa, head, b)
    add("md_last_column", fa, [], synth.sam_text(rbc, md_last=True))
    add("xd_for_md", fa, head, [l.replace(b"MD:Z:", b"XD:Z:") for l in body])
    b = list(body_p)
    b[pairs[0]] = b[pairs[0]].replace(PERFECT, b"MD:Z"); b[pairs[2]] = b[pairs[2]].replace(PERFECT, b"MD"); b[pairs[4]] = b[pairs[4]].replace(PERFECT, b"XD:")
    add("md_tag_short", fa_p, head_p, b)
    aux = [b"Y%c:i:%d" % (65 + j, j) for j in range(20)]                          # no filler tag may itself read as [MX]D
    assert not any(a[0] in b"MX" and a[1] == ord("D") for a in aux)
    b = list(body_p)
    b[mapped[1]] = _edit(b[mapped[1]], lambda f: f[:11] + aux[:19] + f[11:])     # seen: 19 other fields in front of the MD
    b[mapped[3]] = _edit(b[mapped[3]], lambda f: f[:11] + aux + f[11:])          # not seen: the scan stops at the 20th other field
    imperfect = next(i for i in range(1, len(body)) if PERFECT not in body[i] and b"\t100M\t" in body[i] and b"\t100M\t" in body[i - 1]
                     and not _flag(body[i]) & 4 and body[i].split(b"\t")[11] != body[i - 1].split(b"\t")[11])
    add("md_behind_20_aux", fa_p, head_p, b)
    b2 = list(body); b2[imperfect] = _edit(b2[imperfect], lambda f: f[:11] + aux + f[11:])
    add("md_behind_20_aux_imperfect", fa, head, b2)
    b = list(body_p)
    for i in pairs[::2]:
        b[i] = _edit(b[i], _drop_md)
    assert any(int(body_p[i - 1].split(b"\t")[1]) & 4 for i in pairs[::2]) and any(not int(body_p[i - 1].split(b"\t")[1]) & 4 for i in pairs[::2])
    add("md_less_inherits", fa_p, head_p, b)
    b2 = list(body); b2[imperfect] = _edit(b2[imperfect], _drop_md)
    add("md_less_inherits_imperfect", fa, head, b2)
    fa_q, sam_q, _, _ = synth.dataset(103, [20000], [60], 100, sub_rate=0.0, indel_frac=0.0)
    head_q, body_q = _split(sam_q)
    add("md_less_chunk_start", fa_q, head_q, body_q[:1] + [_edit(l, _drop_md) for l in body_q[1:]])
    add("md_less_from_the_start", fa_q, head_q, [_edit(l, _drop_md) for l in body_q])
    add("columns_10", fa, head, body[:7] + [_edit(body[7], lambda f: f[:10])] + body[8:])
    add("last_line_no_newline", fa, head, b"".join(head + body).rstrip(b"\n"))
    add("last_line_no_newline_md_last", fa, [], synth.sam_text(rbc, md_last=True).rstrip(b"\n"))
    add("empty_lines", fa, head, [b"\n"] + body[:5] + [b"\n", b"\n"] + body[5:] + [b"\n"])
    # a mapped record without SEQ: strtok skips the empty column, so QUAL is read as SEQ and the first aux field as QUAL
    k = mapped[5]
    assert not _flag(body_p[k]) & 4
    add("seq_empty", fa_p, head_p, body_p[:k] + [_edit(body_p[k], _set(9, b""))] + body_p[k + 1:])
    for L in (252, 253):
        f, s, _, _ = synth.dataset(104, [20000], [12], L, sub_rate=0.01, indel_frac=0.2)
        add("seq_%d" % L, f, [], s)
    for n in (1023, 1024):
        pad = n - len(body[3]) - len(b"\tXX:Z:")
        add("line_%d_bytes" % n, fa, head, body[:3] + [body[3].rstrip(b"\n") + b"\tXX:Z:" + b"y" * pad + b"\n"] + body[4:])
        assert len(out[-1][2].splitlines(keepends=True)[len(head) + 3]) == n

    # ---- the CIGAR scan
    b = list(body_p)
    b[pairs[0]] = _edit(b[pairs[0]], _set(5, b"5H95M")); b[pairs[2]] = _edit(b[pairs[2]], _set(5, b"3=4X93M")); b[pairs[4]] = _edit(b[pairs[4]], _set(5, b"100MZ7"))
    add("cigar_letters_in_segment", fa_p, head_p, b)
    add("cigar_star", fa, head, body[:9] + [_edit(body[9], _set(5, b"*"))] + body[10:])
    f, s, _, _ = synth.dataset(105, [20000], [40], 100, sub_rate=0.01, indel_frac=0.3, trailing_s_frac=0.5)
    add("clip_trailing", f, [], s)
    f, s = _clip_records(106, ["plain", "perfect", "plain", "perfect", "perfect", "plain"])
    add("clip_leading_perfect", f, [], s)
    f, s = _clip_records(107, ["plain", "snp", "less", "plain", "snp", "plain", "less"])
    add("clip_leading_imperfect", f, [], s)
    f, s = _clip_records(108, ["plain", "last", "less", "plain", "snp", "last", "less", "less", "plain"])
    add("clip_leading_unterminated", f, [], s)
    f, s = _clip_records(109, ["plain", "junk", "less", "plain"])
    add("clip_leading_unterminated_tail", f, [], s)

    # several MD / XD fields on one line: each is copied in turn, the last one wins, and a longer earlier one leaves its tail in
    # the buffer, where the unterminated text of a leading soft clip exposes it
    f, s = _clip_records(110, ["plain", "last", "less", "plain"])
    hd, bd = _split(s)
    bd[1] = _edit(bd[1], lambda c: c[:11] + [b"XD:Z:10A10C10G10T10A10C10G7", b"MD:Z:7"] + [x for x in c[11:] if not x.startswith(b"MD:Z:")])
    add("md_fields_several", f, hd, bd)
    b = list(body)
    b[imperfect] = _edit(b[imperfect], lambda c: c[:11] + [b"MD:Z:100", b"XD:Z:3"] + c[11:])      # the record's own, third one wins
    add("md_fields_several_last_wins", fa, head, b)

    # ---- numerals
    pos0 = int(body_q[0].split(b"\t")[3]); pos1 = int(body_q[1].split(b"\t")[3])
    add("pos_plus_and_space", fa_q, head_q, [_edit(body_q[0], _set(3, b"+%d" % pos0)), _edit(body_q[1], _set(3, b" %d" % pos1))] + body_q[2:])
    add("pos_negative", fa_q, head_q, body_q[:2] + [_edit(body_q[2], _set(3, lambda p: b"-" + p))] + body_q[3:])
    for d in (10, 11, 14, 20):
        k = 3
        pos = int(body_q[k].split(b"\t")[3])
        add("flag_%d_digits" % d, fa_q, head_q, body_q[:k] + [_edit(body_q[k], _set(1, _numeral(d, 16)))] + body_q[k + 1:12])
        add("pos_%d_digits" % d, fa_q, head_q, body_q[:k] + [_edit(body_q[k], _set(3, _numeral(d, pos)))] + body_q[k + 1:12])
        add("cigar_%d_digits" % d, fa_q, head_q, body_q[:k] + [_edit(body_q[k], _set(5, _numeral(d, 100) + b"M"))] + body_q[k + 1:12])
        add("md_gap_%d_digits" % d, fa_q, head_q, body_q[:k] + [_edit(body_q[k], _md(_numeral(d, 100)))] + body_q[k + 1:12])
    add("cigar_12_digits", fa_q, head_q, body_q[:3] + [_edit(body_q[3], _set(5, b"%dM" % (100 * 2 ** 32 + 100)))] + body_q[4:12])

    # ---- the MD scan
    b = list(body_q[:12])
    b[2] = _edit(b[2], _md(b"100^")); b[4] = _edit(b[4], _md(b"100^AC")); b[6] = _edit(b[6], _md(b"50^AC50")); b[8] = _edit(b[8], _md(b"^"))
    add("md_ends_in_caret", fa_q, head_q, b)
    add("md_gap_too_large", fa_q, head_q, body_q[:5] + [_edit(body_q[5], _md(b"16777216A"))] + body_q[6:12])
    add("md_gap_largest", fa_q, head_q, body_q[:5] + [_edit(body_q[5], _md(b"16777215A"))] + body_q[6:12])
    add("md_names_more_than_seq", fa, head, body[:imperfect] + [_edit(body[imperfect], _set(9, lambda s: s[:10]))] + body[imperfect + 1:])

    # ---- a NUL inside a line: the C string ends there, the next line starts behind the '\n'
    def nul_in(col, where):
        return lambda f: f[:col] + [f[col][:where] + b"\0" + f[col][where + 1:]] + f[col + 1:]
    add("nul_in_rname", fa_q, head_q, body_q[:4] + [_edit(body_q[4], nul_in(2, 2))] + body_q[5:12])
    add("nul_in_seq", fa_q, head_q, body_q[:4] + [_edit(body_q[4], nul_in(9, 40))] + body_q[5:12])
    k = next(i for i, l in enumerate(body) if re.search(rb"MD:Z:\d+[ACGT]\d+[ACGT]\d", l) and b"\t100M\t" in l)
    add("nul_in_md", fa, head, body[:k] + [_edit(body[k], _md(lambda m: re.sub(rb"^(\d+[ACGT]\d+)[ACGT]", lambda g: g.group(1) + b"\0", m)))] + body[k + 1:])
    add("nul_in_md_caret_run", fa_q, head_q, body_q[:4] + [_edit(body_q[4], _md(b"50^A\x00C5T44"))] + body_q[5:12])   # as a byte of the run it would be skipped
    add("nul_in_md_perfect", fa_q, head_q, body_q[:4] + [_edit(body_q[4], _md(b"100\x00A0"))] + body_q[5:12])
    assert len({n for n, _, _, _ in out}) == len(out)
    return out


def result(pack, sam, fa, **kw):
    """what the fixture keeps of one pack_sam call"""
    from cbc_amd import host
    try:
        p = pack(sam, fa, **kw)
    except host.CbcInputError as e:
        m = re.match(r"cbc_pack_sam failed \((-?\d+)\): (.*)$", str(e), re.S)
        return dict(rc=int(m.group(1)), err=m.group(2))
    return dict(rc=0, err="", sha256={k: hashlib.sha256(getattr(p, k).tobytes()).hexdigest() for k in ARRAYS},
                **{k: int(getattr(p, k)) for k in SCALARS})


def main(argv):
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--write-dir"); ap.add_argument("--record"); ap.add_argument("--label", default=""); ap.add_argument("--tok", action="store_true")
    a = ap.parse_args(argv)
    files = corpus()
    if a.write_dir:
        os.makedirs(a.write_dir, exist_ok=True)
        for name, fa, sam, _ in files:
            open(os.path.join(a.write_dir, name + ".sam"), "wb").write(sam)
            open(os.path.join(a.write_dir, name + ".fa"), "wb").write(fa)
    if a.record:
        from cbc_amd import host
        host.HOST_LIB = os.path.abspath(a.record)
        old = json.load(open(GOLDEN))["files"] if os.path.exists(GOLDEN) else {}
        rec = {}
        for name, fa, sam, kw in files:
            e = result(host.pack_sam, sam, fa, threads=1, **kw)
            e4 = result(host.pack_sam, sam, fa, threads=4, **kw)
            if e4 != e:
                e["parent_threads4"] = e4
            for k in ("tok_status", "tok_line"):
                if name in old and k in old[name]:
                    e[k] = old[name][k]
            rec[name] = e
        json.dump(dict(recorded_from="cbc_pack_sam of the packer at commit %s (its libcbc_host.so), threads=1; parent_threads4 where threads=4 "
                                     "gave something else.  NOT from that commit: tok_status / tok_line, which packer_corpus.py --tok wrote "
                                     "from the emulation of the tree that holds this file (the code under test); they say what the device path "
                                     "(cbc_tok_core.h) reports for the file: 0 = it tokenises the file, 3 = it hands the file to the host "
                                     "packer, >= 4 = it refuses the line" % a.label,
                       parent=a.label, files=rec), open(GOLDEN, "w"), indent=1, sort_keys=True)
    if a.tok:
        import blockref
        g = json.load(open(GOLDEN))
        for name, fa, sam, kw in files:
            try:
                blockref.emu_tokenise(sam)
                st, line = 0, None
            except ValueError as e:
                st, line = e.args[0]
            g["files"][name]["tok_status"] = st; g["files"][name]["tok_line"] = line
        json.dump(g, open(GOLDEN, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main(sys.argv[1:])
