"""Seeded synthetic FASTA + SAM generator for the parity tests (SURVEY.md section 8(d) recipe).

Contigs are uniform iid ACGT.  Reads: start positions uniform then sorted per contig, FLAG in
{0,16} (or a caller-supplied set), per-base substitution rate `sub_rate`, a fraction `indel_frac`
of reads carry one insertion or deletion of length 1..3 at least 10 bases from either end,
CIGAR uses M/I/D (optionally a trailing S), `MD:Z` is followed by `NM:i` (as BWA writes it),
QUAL constant 'I', QNAME r<index>, MAPQ 60, RNEXT * PNEXT 0 TLEN 0.
"""
import re

import numpy as np

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def make_contig(rng, n):
    return _ACGT[rng.integers(0, 4, size=n, dtype=np.uint8)]


def fasta_text(contigs, width=60):
    """contigs: list of (name, uint8 array).  Returns FASTA bytes with `width` bases per line."""
    out = []
    for name, seq in contigs:
        out.append(b">" + name.encode() + b"\n")
        n = len(seq)
        full = (n // width) * width
        if full:
            body = seq[:full].reshape(-1, width)
            lines = np.concatenate([body, np.full((body.shape[0], 1), 10, dtype=np.uint8)], axis=1)
            out.append(lines.tobytes())
        if n > full:
            out.append(seq[full:].tobytes() + b"\n")
    return b"".join(out)


def _md_and_nm(ref, start, ops, seq, mismatch=None):
    """Build MD string and NM from the aligned pairs.  ops: list of (op, len).  mismatch(read_byte, ref_byte): the
    comparison rule of an M base (default: the bytes differ)."""
    md = []
    run = 0
    nm = 0
    rpos = start
    qpos = 0
    prev_del = False
    for op, ln in ops:
        if op == "M":
            for _ in range(ln):
                if (seq[qpos] == ref[rpos]) if mismatch is None else not mismatch(seq[qpos], ref[rpos]):
                    run += 1
                else:
                    md.append(str(run))
                    md.append(chr(ref[rpos]))
                    run = 0
                    nm += 1
                rpos += 1
                qpos += 1
            prev_del = False
        elif op == "I" or op == "S":
            qpos += ln
            if op == "I":
                nm += ln
        elif op == "D":
            md.append(str(run))
            md.append("^" + bytes(ref[rpos:rpos + ln]).decode())
            run = 0
            rpos += ln
            nm += ln
            prev_del = True
    md.append(str(run))
    return "".join(md), nm


def make_reads(rng, contig, n_reads, L, sub_rate=0.003, indel_frac=0.02, flags=(0, 16),
               trailing_s_frac=0.0, dup_pos_frac=0.0, max_start=None):
    """Returns list of dict(pos, flag, cigar, seq, md, nm) sorted by pos (1-based POS)."""
    n = len(contig)
    hi = (n - L - 8) if max_start is None else max_start
    starts = np.sort(rng.integers(0, hi, size=n_reads))
    if dup_pos_frac > 0:
        dup = rng.random(n_reads) < dup_pos_frac
        for i in range(1, n_reads):
            if dup[i]:
                starts[i] = starts[i - 1]
    flag_choices = np.asarray(flags)
    fl = flag_choices[rng.integers(0, len(flag_choices), size=n_reads)]
    nsub = rng.binomial(L, sub_rate, size=n_reads) if sub_rate > 0 else np.zeros(n_reads, dtype=np.int64)
    has_indel = rng.random(n_reads) < indel_frac
    has_s = rng.random(n_reads) < trailing_s_frac
    recs = []
    for i in range(n_reads):
        s = int(starts[i])
        if nsub[i] == 0 and not has_indel[i] and not has_s[i]:
            seq = contig[s:s + L]
            recs.append(dict(pos=s + 1, flag=int(fl[i]), cigar="%dM" % L, seq=seq.tobytes(), md=str(L), nm=0))
            continue
        ops = [("M", L)]
        body_len = L
        if has_s[i]:
            k = int(rng.integers(1, 6))
            body_len = L - k
            ops = [("M", body_len), ("S", k)]
        if has_indel[i] and body_len > 30:
            k = int(rng.integers(1, 4))
            o = int(rng.integers(10, body_len - 10 - k))
            tail = ops[1:] if len(ops) > 1 else []
            if rng.random() < 0.5:
                ops = [("M", o), ("I", k), ("M", body_len - o - k)] + tail
            else:
                ops = [("M", o), ("D", k), ("M", body_len - o)] + tail
        # assemble the read from the reference
        parts = []
        rpos = s
        mpos = []  # read indices that are M bases
        qpos = 0
        for op, ln in ops:
            if op == "M":
                parts.append(contig[rpos:rpos + ln].copy())
                mpos.extend(range(qpos, qpos + ln))
                rpos += ln
                qpos += ln
            elif op == "I" or op == "S":
                parts.append(_ACGT[rng.integers(0, 4, size=ln)])
                qpos += ln
            elif op == "D":
                rpos += ln
        seq = np.concatenate(parts)
        assert len(seq) == L
        if nsub[i] > 0:
            where = rng.choice(len(mpos), size=min(int(nsub[i]), len(mpos)), replace=False)
            for w in where:
                q = mpos[int(w)]
                old = seq[q]
                alt = _ACGT[(int(np.where(_ACGT == old)[0][0]) + int(rng.integers(1, 4))) % 4]
                seq[q] = alt
        md, nm = _md_and_nm(contig, s, ops, seq)
        cigar = "".join("%d%s" % (ln, op) for op, ln in ops)
        recs.append(dict(pos=s + 1, flag=int(fl[i]), cigar=cigar, seq=seq.tobytes(), md=md, nm=nm))
    return recs


def sam_text(records_by_contig, header=True, md_last=False, qual_char=b"I", start_index=0):
    """records_by_contig: list of (name, contig_len, [records]).  Returns SAM bytes."""
    out = []
    if header:
        out.append(b"@HD\tVN:1.6\tSO:coordinate\n")
        for name, clen, _ in records_by_contig:
            out.append(("@SQ\tSN:%s\tLN:%d\n" % (name, clen)).encode())
    idx = start_index
    for name, _, recs in records_by_contig:
        nb = name.encode()
        for r in recs:
            seq = r["seq"]
            qual = qual_char * len(seq)
            if md_last:
                tags = ("NM:i:%d\tMD:Z:%s" % (r["nm"], r["md"])).encode()
            else:
                tags = ("MD:Z:%s\tNM:i:%d" % (r["md"], r["nm"])).encode()
            out.append(b"r%d\t%d\t%s\t%d\t60\t%s\t*\t0\t0\t%s\t%s\t%s\n" % (
                idx, r["flag"], nb, r["pos"], r["cigar"].encode(), seq, qual, tags))
            idx += 1
    return b"".join(out)


def dataset(seed, contig_lens, reads_per_contig, L, names=None, **kw):
    """Convenience: returns (fasta_bytes, sam_bytes, records_by_contig, contigs)."""
    rng = np.random.default_rng(seed)
    contigs = []
    rbc = []
    for ci, (clen, nr) in enumerate(zip(contig_lens, reads_per_contig)):
        name = names[ci] if names else "chr%d" % (ci + 1)
        c = make_contig(rng, clen)
        contigs.append((name, c))
        rbc.append((name, clen, make_reads(rng, c, nr, L, **kw)))
    return fasta_text(contigs), sam_text(rbc), rbc, contigs


def shared_variant_dataset(seed, clen, n_reads, L, site_every, err, indel_sites=0):
    """Reads whose SNPs are SHARED: every read covering a variant site carries the site's alternative base
    (plus independent errors at rate `err`).  This is what real alignments look like, and it is the case
    where var contexts repeat ("the known variant d bases ahead").  Returns (fasta_bytes, sam_bytes)."""
    rng = np.random.default_rng(seed)
    contig = make_contig(rng, clen)
    alt = contig.copy()
    sites = rng.choice(clen, size=max(clen // site_every, 1), replace=False)
    for s in sites:
        alt[s] = _ACGT[(int(np.where(_ACGT == contig[s])[0][0]) + 1 + int(rng.integers(0, 3))) % 4]
    starts = np.sort(rng.integers(0, clen - L - 8, size=n_reads))
    out = []
    for i, s in enumerate(starts):
        s = int(s)
        seq = alt[s:s + L].copy()
        ne = int(rng.binomial(L, err)) if err > 0 else 0
        for q in (rng.choice(L, size=ne, replace=False) if ne else []):
            seq[q] = _ACGT[(int(np.where(_ACGT == seq[q])[0][0]) + 1 + int(rng.integers(0, 3))) % 4]
        md, nm = _md_and_nm(contig, s, [("M", L)], seq)
        out.append(b"r%d\t%d\tc\t%d\t60\t%dM\t*\t0\t0\t%s\t%s\tMD:Z:%s\tNM:i:%d\n" % (
            i, 16 * int(rng.integers(0, 2)), s + 1, L, seq.tobytes(), b"I" * L, md.encode(), nm))
    return fasta_text([("c", contig)]), b"".join(out)


# ------------------------------------------------------------------------------------------------ genome-shaped inputs
# What a real reference holds and make_contig does not: N gaps (at contig ends too), scattered IUPAC codes, soft-masked
# lower case; and what real reads hold: N calls, N over N, bases over IUPAC sites, reads at both contig ends.

_IUPAC = np.frombuffer(b"RYKMSWBDHV", dtype=np.uint8)
_N = ord("N")


def calmd_mismatch(read_byte, ref_byte):
    """The MD rule of samtools calmd / BWA against the upper-cased reference: the bytes differ, or either is N (an N over
    an N is listed as a mismatch, `40N59`)."""
    return read_byte != ref_byte or read_byte == _N or ref_byte == _N


def byte_mismatch(read_byte, ref_byte):
    """N over N folded into the match run: the byte comparison the reference's own perfect-read test uses."""
    return read_byte != ref_byte


def n_runs(arr, min_len=1):
    """(start, length) of every run of N in a uint8 array, of at least min_len bytes."""
    isn = np.concatenate([[False], arr == _N, [False]])
    d = np.diff(isn.astype(np.int8))
    st, en = np.nonzero(d == 1)[0], np.nonzero(d == -1)[0]
    keep = (en - st) >= min_len
    return list(zip(st[keep].tolist(), (en - st)[keep].tolist()))


def make_genome_contig(rng, n, n_gaps=10, max_gap=50_000, edge_gaps=True, iupac_rate=0.002, n_rate=0.0005,
                       soft_frac=0.5, gap_lens=None):
    """Returns (mixed-case FASTA bases, upper-cased bases) of a contig of n bases: N gaps at both ends (edge_gaps) and
    n_gaps inside, lengths log-uniform in 1..max_gap (or gap_lens), the longest max_gap; single N and IUPAC letters at
    the given rates; lower-case stretches of 100..5000 bases over about soft_frac of the contig."""
    up = make_contig(rng, n).copy()
    k = n_gaps + (2 if edge_gaps else 0)
    if gap_lens is None:
        gap_lens = np.exp(rng.uniform(0.0, np.log(max_gap), size=k)).astype(np.int64) + 1
        gap_lens[:1] = max_gap
        gap_lens = np.minimum(gap_lens, max_gap)
    lens = [int(x) for x in gap_lens]
    inner = lens[2:] if edge_gaps else lens
    slot = n // (len(inner) + 1)
    for i, g in enumerate(inner):                      # one gap per slot: they never merge
        g = min(g, slot // 2)
        s = (i + 1) * slot + int(rng.integers(0, max(slot // 4, 1)))
        up[s:s + g] = _N
    if edge_gaps:
        up[:min(lens[0], n // 8)] = _N
        up[n - min(lens[1], n // 8):] = _N
    for code, rate in ((None, iupac_rate), (_N, n_rate)):
        where = np.nonzero((rng.random(n) < rate) & (up != _N))[0]          # gaps stay whole
        up[where] = _IUPAC[rng.integers(0, len(_IUPAC), size=len(where))] if code is None else code
    soft = np.zeros(n, dtype=bool)
    while soft.sum() < soft_frac * n:
        s = int(rng.integers(0, n)); soft[s:s + int(rng.integers(100, 5001))] = True
    text = np.where(soft, up | 0x20, up).astype(np.uint8)
    return text, up


def _genome_read(rng, contig, s, L, sub_rate=0.003, indel=False, n_mode=None, fill_n=False, nn_listed=True, exotic=False):
    """One record at 0-based start s over the upper-cased contig.  The read carries a concrete base over every IUPAC site
    (a mismatch whose MD letter is the IUPAC code), N over reference N unless fill_n, substitutions at sub_rate, optionally
    one indel, and N calls by n_mode (None, "isolated", "run", "all").  nn_listed: an N over an N is a mismatch in MD
    (calmd), else folded into the match run.  exotic: a few SEQ bytes outside ACGTN (lower case, IUPAC, a byte equal to
    an IUPAC reference byte)."""
    ops = [("M", L)]
    if indel and L > 30:
        k = int(rng.integers(1, 4)); o = int(rng.integers(10, L - 10 - k))
        ops = [("M", o), ("I", k), ("M", L - o - k)] if rng.random() < 0.5 else [("M", o), ("D", k), ("M", L - o)]
    parts, mpos, rpos, q = [], [], s, 0
    for op, ln in ops:
        if op == "M":
            parts.append(contig[rpos:rpos + ln].copy()); mpos.extend(range(q, q + ln)); rpos += ln; q += ln
        elif op == "I":
            parts.append(_ACGT[rng.integers(0, 4, size=ln)]); q += ln
        else:
            rpos += ln
    seq = np.concatenate(parts)
    mpos = np.asarray(mpos)
    conc = ~np.isin(seq[mpos], _ACGT)
    if not fill_n:
        conc &= seq[mpos] != _N
    seq[mpos[conc]] = _ACGT[rng.integers(0, 4, size=int(conc.sum()))]
    for w in mpos[rng.random(len(mpos)) < sub_rate]:
        old = seq[w]
        seq[w] = _ACGT[(int(np.nonzero(_ACGT == old)[0][0]) + int(rng.integers(1, 4))) % 4] if old in _ACGT else _ACGT[rng.integers(0, 4)]
    if n_mode == "isolated":
        seq[rng.choice(L, size=int(rng.integers(1, 4)), replace=False)] = _N
    elif n_mode == "run":
        k = int(rng.integers(5, 31)); o = int(rng.integers(0, L - k + 1)); seq[o:o + k] = _N
    elif n_mode == "all":
        seq[:] = _N
    elif n_mode == "most":                             # every base but one an N call: L - 1 SNPs, the most a record holds
        keep = int(rng.choice(mpos[np.isin(contig[s + mpos], _ACGT)])) if len(ops) == 1 else -1
        seq[:] = _N
        if keep >= 0:
            seq[keep] = contig[s + keep]
    if exotic:
        for w in rng.choice(mpos, size=3, replace=False):
            seq[w] = seq[w] | 0x20 if rng.random() < 0.5 else _IUPAC[rng.integers(0, len(_IUPAC))]
        iu = mpos[np.isin(contig[s + mpos], _IUPAC)] if len(ops) == 1 else mpos[:0]
        if len(iu):
            seq[iu[0]] = contig[s + iu[0]]                 # equal to the IUPAC reference byte: a match
    # the reference codes at most L - 1 SNPs per record (its snps model has L symbols): N over N listed as mismatches
    # can pass that on a read that is not otherwise perfect, so such a read folds them into the match run instead
    md, nm = _md_and_nm(contig, s, ops, seq, mismatch=calmd_mismatch if nn_listed else byte_mismatch)
    if nn_listed and len(re.findall(r"[A-Z]", re.sub(r"\^[A-Z]+", "", md))) >= len(seq):
        md, nm = _md_and_nm(contig, s, ops, seq, mismatch=byte_mismatch)
    return dict(pos=s + 1, flag=int(rng.integers(0, 2)) * 16, cigar="".join("%d%s" % (ln, op) for op, ln in ops),
                seq=seq.tobytes(), md=md, nm=nm)


def make_genome_reads(rng, contig, n_reads, L, sub_rate=0.003, indel_frac=0.02, n_read_frac=0.05, exotic_frac=0.0,
                      edge_reads=3):
    """Random reads plus reads placed on purpose: straddling both edges of every N gap (of 10 or more bases), at POS 1,
    ending on the contig's last base, and all-N reads.  Sorted by POS."""
    n = len(contig)
    starts = rng.integers(0, n - L - 3, size=3 * n_reads)
    starts = [int(x) for x in starts[(contig[starts] != _N) | (contig[starts + L - 1] != _N)][:n_reads]]   # not inside a gap
    kinds = [None] * len(starts)
    for g0, gl in n_runs(contig, 10):
        for edge in (g0, g0 + gl):                     # the read holds both contig[edge - 1] and contig[edge]
            if 0 < edge < n:
                for _ in range(edge_reads):
                    s = edge - int(rng.integers(1, L))
                    if 0 <= s <= n - L - 3:
                        starts.append(s); kinds.append("edge")
    starts += [0] * edge_reads + [n - L] * edge_reads
    kinds += ["ends"] * (2 * edge_reads)
    inside = [g0 + int(rng.integers(0, gl - L)) for g0, gl in n_runs(contig, L + 1)][:edge_reads]
    most = [x for x in starts if np.isin(contig[x:x + L], _ACGT).any()][:edge_reads]
    starts += inside + most
    kinds += ["all"] * len(inside) + ["most"] * len(most)
    recs = []
    for s, kind in zip(starts, kinds):
        nn_listed = rng.random() < 0.5
        if kind == "edge":
            r = _genome_read(rng, contig, s, L, sub_rate, fill_n=rng.random() < 0.5, nn_listed=nn_listed)
        elif kind == "ends":
            r = _genome_read(rng, contig, s, L, sub_rate, nn_listed=nn_listed)
        elif kind in ("all", "most"):
            r = _genome_read(rng, contig, s, L, 0.0, n_mode=kind, nn_listed=nn_listed)
        else:
            u = rng.random()
            n_mode = None if u >= n_read_frac else ("isolated", "run")[int(rng.integers(0, 2))]
            r = _genome_read(rng, contig, s, L, sub_rate, indel=rng.random() < indel_frac, n_mode=n_mode,
                             nn_listed=nn_listed, exotic=rng.random() < exotic_frac)
        recs.append(r)
    recs.sort(key=lambda r: r["pos"])
    return recs


def genome_dataset(seed, contig_lens=(300_000, 120_000), reads_per_contig=(4000, 1500), L=100, contig_kw=None, **kw):
    """Genome-shaped counterpart of dataset(): even-numbered contigs start and end in an N gap, odd ones in bases.
    Returns (soft-masked fasta_bytes, sam_bytes, records_by_contig, upper-cased contigs)."""
    rng = np.random.default_rng(seed)
    texts, contigs, rbc = [], [], []
    for ci, (clen, nr) in enumerate(zip(contig_lens, reads_per_contig)):
        name = "chr%d" % (ci + 1)
        text, up = make_genome_contig(rng, clen, **dict(dict(edge_gaps=ci % 2 == 0), **(contig_kw or {})))
        texts.append((name, text)); contigs.append((name, up))
        rbc.append((name, clen, make_genome_reads(rng, up, nr, L, **kw)))
    return fasta_text(texts), sam_text(rbc), rbc, contigs


def genome_features(rbc, contigs):
    """What a genome-shaped input holds, counted from the records themselves (the tests assert these)."""
    f = dict(n_gaps=0, gap_edges_crossed=0, iupac_sites_under_reads=0, nn_pairs=0, reads_at_pos1=0, reads_at_end=0,
             reads_over_4n=0, all_n_reads=0, n_in_reads=0, n_reads=0, exotic_bytes=0, md_iupac_letters=0)
    for (name, clen, recs), (_, c) in zip(rbc, contigs):
        gaps = n_runs(c, 10)
        f["n_gaps"] += len(gaps)
        edges = np.array(sorted({e for g0, gl in gaps for e in (g0, g0 + gl) if 0 < e < clen}), dtype=np.int64)
        for r in recs:
            s = r["pos"] - 1
            seq = np.frombuffer(r["seq"], dtype=np.uint8)
            m = re.findall(r"(\d+)([MIDS])", r["cigar"])
            span = sum(int(k) for k, op in m if op in "MD")
            f["n_reads"] += 1
            f["reads_at_pos1"] += s == 0
            f["reads_at_end"] += s + span == clen
            k = int((seq == _N).sum())
            f["n_in_reads"] += k
            f["reads_over_4n"] += k > 4
            f["all_n_reads"] += k == len(seq)
            f["exotic_bytes"] += int((~np.isin(seq, np.frombuffer(b"ACGTN", dtype=np.uint8))).sum())
            f["gap_edges_crossed"] += int(((edges > s) & (edges < s + span)).sum())
            f["md_iupac_letters"] += sum(ch in "RYKMSWBDHV" for ch in re.sub(r"\^[A-Z]+", "", r["md"]))
            if len(m) == 1:
                w = c[s:s + len(seq)]
                f["iupac_sites_under_reads"] += int(np.isin(w, _IUPAC).sum())
                f["nn_pairs"] += int(((w == _N) & (seq == _N)).sum())
    return f


def genome_long_dataset(seed, clen=1_500_000, n_reads=120, read_len=(5000, 10000), edit_rate=0.03, n_cross=8):
    """Long reads (ACGTN only, no MD: the long-read format) over a genome-shaped contig whose inner gaps are a few
    hundred bases long; n_cross reads are placed across such a gap and carry concrete bases over it (hundreds of
    mismatches in one M run).  Returns (soft-masked fasta_bytes, sam_bytes, upper-cased contig, starts of the crossing reads)."""
    rng = np.random.default_rng(seed)
    text, c = make_genome_contig(rng, clen, n_gaps=6, edge_gaps=True, gap_lens=[3000, 2000] + [int(x) for x in rng.integers(300, 900, size=6)])
    gaps = [g for g in n_runs(c, 200) if 0 < g[0] and g[0] + g[1] < clen]
    lens = rng.integers(read_len[0], read_len[1] + 1, size=n_reads)
    starts = [int(rng.integers(0, clen - int(l) - 300)) for l in lens]
    fill = [False] * n_reads
    for i in range(n_cross):
        g0, gl = gaps[i % len(gaps)]
        starts[i] = max(g0 - int(rng.integers(100, int(lens[i]) - gl - 100)), 0); fill[i] = True
    order = np.argsort(starts, kind="stable")
    lines, crossing = [], []
    for j, i in enumerate(order):
        s, Lr = starts[i], int(lens[i])
        ops, q, rpos, parts = [], 0, s, []
        while q < Lr:
            m = min(int(rng.integers(20, 400)), Lr - q)
            parts.append(c[rpos:rpos + m].copy()); ops.append(("M", m)); q += m; rpos += m
            if q < Lr and rng.random() < edit_rate * 20:
                k = min(int(rng.integers(1, 4)), Lr - q)
                if rng.random() < 0.5:
                    parts.append(_ACGT[rng.integers(0, 4, size=k)]); ops.append(("I", k)); q += k
                else:
                    ops.append(("D", k)); rpos += k
        seq = np.concatenate(parts)
        bad = ~np.isin(seq, _ACGT) & ((seq != _N) | fill[i])
        seq[bad] = _ACGT[rng.integers(0, 4, size=int(bad.sum()))]
        sub = rng.random(Lr) < edit_rate
        seq[sub] = _ACGT[rng.integers(0, 4, size=int(sub.sum()))]
        merged = []
        for op, ln in ops:
            if merged and merged[-1][0] == op:
                merged[-1] = (op, merged[-1][1] + ln)
            else:
                merged.append((op, ln))
        if fill[i]:
            crossing.append(s)
        lines.append(b"r%d\t%d\tchrL\t%d\t60\t%s\t*\t0\t0\t%s\t*\n" % (
            j, 16 * int(rng.integers(0, 2)), s + 1, "".join("%d%s" % (ln, op) for op, ln in merged).encode(), seq.tobytes()))
    hdr = b"@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:chrL\tLN:%d\n" % clen
    return fasta_text([("chrL", text)]), hdr + b"".join(lines), c, crossing
