/*
 * cbc_tok_core.h -- the rule for one SAM line, as plain functions over byte ranges.  It is stated here once and compiled three
 * ways: by hipcc, one GPU thread per line (cbc_tokenise.h); by g++ under the CPU tests (tests/emu); and by gcc as C11 into
 * the host packer (cbc_pack.c), which adds only what is serial state (see below).
 *
 * The rule is the reference's, restated for one line / one record:
 *   load_sam_line()         src/sam_file_allocation.c:437-529   strtok("\t") columns of a line that still carries its
 *                                                                '\n' (quirk Q2), FLAG / POS via atoi, MD|XD aux field
 *   CIGAR scan              src/read_compression.c:308-352       atoi() of the UNCONSUMED segment at every M I D S *
 *   MD scan                 src/read_compression.c:613-701       (gap << 8) | letter per mismatch, '^' runs add to the gap
 *   consistency replay      src/read_compression.c:551-552, 656-659  every MD mismatch must be consumed by the read
 * The reference works on C strings: a line ends at its first NUL byte (the next one still starts behind the '\n'), and
 * its numbers are glibc's atoi() on LP64.  Both hold here, on every path.
 * A record without an MD / XD field inherits the text of the nearest earlier line that has one (read_line_t.edits persists
 * across load_sam_line calls: src/sam_file_allocation.c:505-511).  The host packer keeps that buffer (packer_t.edits) and
 * hands it to cbc_tok_md() as a plain range; the device looks back over the lines already split, at most
 * CBC_TOK_MD_LOOKBACK of them (cbc_tok_md_source()).
 * What only the host packer does: a record whose CIGAR starts with a soft clip -- quirk Q6: the reference rewrites that
 * record's MD text IN the buffer that persists across records and does not terminate what it wrote
 * (read_compression.c:357-468, :460), so the text depends on the buffer's whole history, which is serial state.  The CIGAR
 * scan takes one parameter for it; without it, and for an MD-less record with no MD within the look-back, the device path
 * reports CBC_TOK_NEEDS_HOST and the caller falls back to the host packer.
 */
#ifndef CBC_TOK_CORE_H
#define CBC_TOK_CORE_H

#include <stdint.h>
#include "../../include/cbc_gpu.h"

#if defined(__HIPCC__)
#define CBC_TOK_FN __host__ __device__ static inline
#else
#define CBC_TOK_FN static inline
#endif

#define CBC_TOK_MD_LOOKBACK 4096u         /* lines an MD-less record looks back for its text (beyond: the host packer) */
#define CBC_TOK_LINE_MAX 1023u            /* fgets(buffer, 1024, ...): longer lines are refused */

enum { CBC_TOK_OK = 0, CBC_TOK_SKIP = 1 /* no token on the line */, CBC_TOK_UNMAPPED = 2,
       CBC_TOK_NEEDS_HOST = 3, CBC_TOK_E_COLUMNS = 4, CBC_TOK_E_LINE_LONG = 5, CBC_TOK_E_CIGAR = 6, CBC_TOK_E_STAR = 7,
       CBC_TOK_E_MD = 8, CBC_TOK_E_INCONSISTENT = 9, CBC_TOK_E_READ_LEN = 10, CBC_TOK_E_POS = 11, CBC_TOK_E_TOO_MANY = 12 };

/* one line after the column split: offsets into the text */
typedef struct cbc_tok_line {
    uint64_t rname, cigar, seq, md;       /* byte offsets of the tokens in the SAM text */
    uint32_t rname_len, cigar_len, seq_len, md_len;   /* md_len includes a trailing '\n' when MD is the last column (Q2) */
    int32_t  pos; uint32_t flag;
    uint32_t status, has_md;              /* has_md: how many MD / XD fields the line has; md is the last one's text */
} cbc_tok_line;

/* what the host needs of a mapped record to cut blocks (cbc_pack.c place_record) */
typedef cbc_tok_record_summary cbc_tok_summary;         /* the one public 16-byte struct (include/cbc_gpu.h): nt | ev << 16, line index */

CBC_TOK_FN int cbc_tok_isdigit(uint8_t c) { return c >= '0' && c <= '9'; }
CBC_TOK_FN int cbc_tok_isspace(uint8_t c) { return c == ' ' || (c >= 9 && c <= 13); }
/* glibc's atoi() on LP64 over [p, e): leading white space, one sign, digits; the exact value, saturating at 2^63 - 1 / -2^63
 * like the strtol() behind it.  The callers' casts then take the low bits, as atoi's own cast to int does. */
CBC_TOK_FN long long cbc_tok_atoi(const uint8_t *p, const uint8_t *e)
{
    while (p < e && cbc_tok_isspace(*p)) p++;
    uint32_t neg = 0;
    if (p < e && (*p == '-' || *p == '+')) { neg = *p == '-'; p++; }
    const unsigned long long lim = 0x7fffffffffffffffull + neg, cut = 0x7fffffffffffffffull / 10u;   /* |LONG_MIN| / 10 is the same */
    unsigned long long v = 0;
    for (; p < e && cbc_tok_isdigit(*p); p++) {
        const uint32_t d = (uint32_t)(*p - '0');
        v = (v > cut || (v == cut && d > 7u + neg)) ? lim : v * 10u + d;
    }
    return (long long)(neg ? 0ull - v : v);
}
CBC_TOK_FN uint32_t cbc_tok_num_digits(uint32_t x)      /* compute_num_digits read_compression.c:720-743 */
{
    return x < 10 ? 1 : x < 100 ? 2 : x < 1000 ? 3 : x < 10000 ? 4 : x < 100000 ? 5 : x < 1000000 ? 6 : x < 10000000 ? 7 : x < 100000000 ? 8 : 9;
}

/* strtok(line, "\t") over [b, e) (e = one past the line's '\n', or the end of the text; the line ends earlier at a NUL): the 11
 * compulsory columns and the MD / XD aux field (the LAST one seen wins; at most 20 other aux fields are looked at: MAX_AUX_FIELDS) */
CBC_TOK_FN void cbc_tok_split(const uint8_t *sam, uint64_t b, uint64_t e, cbc_tok_line *L)
{
    L->status = CBC_TOK_OK; L->has_md = 0; L->md = 0; L->md_len = 0;
    L->rname = L->cigar = L->seq = 0; L->rname_len = L->cigar_len = L->seq_len = 0; L->pos = 0; L->flag = 0;
    if (e - b > CBC_TOK_LINE_MAX) { L->status = CBC_TOK_E_LINE_LONG; return; }
    uint64_t p = b; uint32_t nf = 0, aux = 0;
    for (;;) {
        while (p < e && sam[p] == '\t') p++;
        if (p >= e || sam[p] == 0) break;
        uint64_t q = p;
        while (q < e && sam[q] != '\t' && sam[q] != 0) q++;
        if (nf < 11) {
            if (nf == 1) L->flag = (uint32_t)(uint16_t)cbc_tok_atoi(sam + p, sam + q);
            else if (nf == 2) { L->rname = p; L->rname_len = (uint32_t)(q - p); }
            else if (nf == 3) L->pos = (int32_t)cbc_tok_atoi(sam + p, sam + q);
            else if (nf == 5) { L->cigar = p; L->cigar_len = (uint32_t)(q - p); }
            else if (nf == 9) { L->seq = p; L->seq_len = (uint32_t)(q - p); }
            nf++;
        } else {
            if (q - p >= 2 && (sam[p] == 'M' || sam[p] == 'X') && sam[p + 1] == 'D') {
                L->has_md++;
                if (q - p >= 5) { L->md = p + 5; L->md_len = (uint32_t)(q - p - 5); } else { L->md = p; L->md_len = 0; }
            } else if (++aux == 20) break;
        }
        p = q;
    }
    if (nf == 0) { L->status = CBC_TOK_SKIP; return; }
    if (nf < 11) { L->status = CBC_TOK_E_COLUMNS; return; }
    if ((L->flag & 4u) == 4u) { L->status = CBC_TOK_UNMAPPED; return; }
    /* no MD / XD field: the caller gives the record the text it inherits before the MD scan */
}
#ifdef __cplusplus
/* Where an MD-less record at line k takes its MD text from on the device path: get(j) returns line j's split (NULL for a line
 * that is not part of the body: '@' headers).  An unmapped line's MD counts too -- load_sam_line() has copied it before
 * compress_line() looks at the FLAG.  *md / *md_len: the text (empty when no earlier body line has one: the buffer starts zeroed). */
template <class GET>
CBC_TOK_FN uint32_t cbc_tok_md_source(uint64_t k, GET get, uint64_t *md, uint32_t *md_len)
{
    *md = 0; *md_len = 0;
    for (uint64_t back = 1; back <= k; back++) {
        const cbc_tok_line *P = get(k - back);
        if (!P) return CBC_TOK_OK;                           /* reached the header: nothing to inherit */
        if (P->has_md) { *md = P->md; *md_len = P->md_len; return CBC_TOK_OK; }
        if (back >= CBC_TOK_MD_LOOKBACK) return CBC_TOK_NEEDS_HOST;
    }
    return CBC_TOK_OK;
}
#endif

/* CIGAR scan (read_compression.c:308-549 scanning rule): a segment runs from the end of the previous recognised op to the next
 * M I D S *; its length is atoi() of the whole segment, so letters that are no ops stay inside it.  tk: NULL (count only) or
 * room for the op words, (len << 4) | op.  *ev = the ops' bound on var symbols.  *bad (optional): the length that was refused.
 * A leading soft clip is quirk Q6, which needs the host packer's persisting MD buffer: with lead_clip == NULL the scan returns
 * CBC_TOK_NEEDS_HOST; the host packer passes a pointer and gets the op stored as CBC_OP_I (the kernels code the clipped bases
 * like an insertion at matched coordinate 0) and *lead_clip = 1. */
CBC_TOK_FN uint32_t cbc_tok_cigar(const uint8_t *cig, const uint8_t *ce, uint32_t *tk, int *lead_clip, uint32_t *n_cig_out,
                                  uint32_t *ev_out, long long *bad)
{
    uint32_t n_cig = 0, ev = 0;
    const uint8_t *seg = cig;
    if (lead_clip) *lead_clip = 0;
    for (const uint8_t *c = cig; c < ce; c++) {
        const uint8_t ch = *c;
        if (cbc_tok_isdigit(ch)) continue;
        uint32_t op = ch == 'M' ? CBC_OP_M : ch == 'I' ? CBC_OP_I : ch == 'D' ? CBC_OP_D : ch == 'S' ? CBC_OP_S : ch == '*' ? CBC_OP_STAR : 0xffu;
        if (op == 0xffu) continue;                      /* not an op: it stays inside the segment */
        const int v = (int)cbc_tok_atoi(seg, c + 1);    /* atoi() of the unconsumed segment */
        if (v < 0 || v > 0x0fffffff) { if (bad) *bad = v; return CBC_TOK_E_CIGAR; }
        if (n_cig >= 2046u) return CBC_TOK_E_TOO_MANY;
        if (op == CBC_OP_STAR) return CBC_TOK_E_STAR;
        if (op == CBC_OP_S && n_cig == 0) { if (!lead_clip) return CBC_TOK_NEEDS_HOST; *lead_clip = 1; op = CBC_OP_I; }
        if (tk) tk[n_cig] = ((uint32_t)v << 4) | op;
        n_cig++;
        if (op != CBC_OP_M) ev += (uint32_t)v;
        seg = c + 1;
    }
    *n_cig_out = n_cig; *ev_out = ev;
    return CBC_TOK_OK;
}

/* a number of the MD text: it is stepped over by the digits of its VALUE, not of its text */
CBC_TOK_FN const uint8_t *cbc_tok_md_number(const uint8_t *p, const uint8_t *me, uint32_t *v)
{
    *v = (uint32_t)cbc_tok_atoi(p, me);
    const uint32_t nd = cbc_tok_num_digits(*v);
    return (uint64_t)(me - p) < nd ? me : p + nd;
}
/* One step of add_snps_to_array's scan at *pp: the gap in front of the next mismatch ('^' runs add their number to it) and the
 * mismatch's letter.  0 = the text ends without another mismatch. */
CBC_TOK_FN int cbc_tok_md_step(const uint8_t **pp, const uint8_t *me, uint32_t *gap_out, uint8_t *ch_out)
{
    uint32_t gap, v;
    const uint8_t *p = cbc_tok_md_number(*pp, me, &gap);
    uint8_t ch = p < me ? *p++ : 0;
    while (ch == '^') {
        while (p < me && !cbc_tok_isdigit(*p)) p++;
        if (p >= me) { ch = 0; break; }
        p = cbc_tok_md_number(p, me, &v); gap += v;
        ch = p < me ? *p++ : 0;
    }
    *pp = p; *gap_out = gap; *ch_out = ch;
    return ch != 0;
}
/* MD scan over [md, me), a plain range that need not lie in the SAM text.  tk: NULL (count only) or room for the mismatch
 * words, (gap << 8) | letter; n_cig: the words the CIGAR took (the record's limit is shared).  *bad (optional): the refused gap. */
CBC_TOK_FN uint32_t cbc_tok_md(const uint8_t *md, const uint8_t *me, uint32_t *tk, uint32_t n_cig, uint32_t *n_md_out, long long *bad)
{
    uint32_t n_md = 0, gap; uint8_t ch;
    const uint8_t *p = md;
    while (p < me && cbc_tok_md_step(&p, me, &gap, &ch)) {
        if (gap > 0x00ffffffu) { if (bad) *bad = gap; return CBC_TOK_E_MD; }
        if (2u + n_cig + n_md >= 4095u) return CBC_TOK_E_TOO_MANY;
        if (tk) tk[n_md] = (gap << 8) | ch;
        n_md++;
    }
    *n_md_out = n_md;
    return CBC_TOK_OK;
}

/* Consistency replay: compress_edits' CIGAR walk with add_snps_to_array's early-return rule; every one of the n_md mismatches
 * must be consumed.  An MD text that names more bases than the read has makes the reference leave its parser statics dirty
 * for the NEXT record (undefined behaviour there); such input is refused.  Both texts are read again, in order, so that the
 * counting pass needs no token words.  lead_clip: the first op is the soft clip that cbc_tok_cigar() stored as an insertion.
 * *del_ins = deleted | inserted << 16 bases, token word 1. */
CBC_TOK_FN uint32_t cbc_tok_replay(const uint8_t *cig, const uint8_t *ce, const uint8_t *md, const uint8_t *me, uint32_t rl,
                                   uint32_t n_md, int lead_clip, uint32_t *del_ins)
{
    uint32_t nDel = 0, nIns = 0, nS = 0, cum = 0, Mc = 0, o = 0, gap = 0;
    int more = 1, have_gap = 0; uint8_t letter;
    const uint8_t *seg = cig;
    for (const uint8_t *c = cig; ; c++) {
        uint32_t op, len;
        if (c < ce) {
            const uint8_t ch = *c;
            if (cbc_tok_isdigit(ch)) continue;
            op = ch == 'M' ? CBC_OP_M : ch == 'I' ? CBC_OP_I : ch == 'D' ? CBC_OP_D : ch == 'S' ? CBC_OP_S : 0xffu;
            if (op == 0xffu) continue;
            len = (uint32_t)cbc_tok_atoi(seg, c + 1); seg = c + 1;
            if (o++ == 0 && lead_clip) op = CBC_OP_I;
        } else { op = 99u; len = 1u; }                  /* the end of the read: whatever is left must fit */
        if (op == CBC_OP_M) { Mc += len; continue; }
        if (op == CBC_OP_D) { nDel += len; continue; }
        for (uint32_t i = 0; i < len; i++) {
            if ((op == CBC_OP_I || op == 99u) && more) {
                const uint32_t limit = op == 99u ? rl + 1u : Mc + nIns;
                more = 0;
                while (nS < n_md) {
                    if (!have_gap) { (void)cbc_tok_md_step(&md, me, &gap, &letter); have_gap = 1; }
                    if (cum + gap >= limit) { cum++; more = 1; break; }
                    cum += gap + 1u; nS++; have_gap = 0;
                }
            }
            if (op == 99u) break;
            nIns++;
        }
        if (op == 99u) break;
    }
    if (nS != n_md) return CBC_TOK_E_INCONSISTENT;
    if (nDel > 0xffffu || nIns > 0xffffu) return CBC_TOK_E_TOO_MANY;
    *del_ins = nDel | (nIns << 16);
    return CBC_TOK_OK;
}

/* CIGAR + MD of one mapped record of the device path -> token words.  `tk` may be NULL (count only).  Returns a CBC_TOK_*
 * status; *nt_out = words, *ev_out = the record's bound on var symbols. */
CBC_TOK_FN uint32_t cbc_tok_record(const uint8_t *sam, const cbc_tok_line *L, uint32_t *tk, uint32_t *nt_out, uint32_t *ev_out)
{
    const uint8_t *cig = sam + L->cigar, *ce = cig + L->cigar_len;
    const uint8_t *md = sam + L->md, *me = md + L->md_len;
    if (L->seq_len == 0 || L->seq_len > CBC_MAX_READ_LEN) return CBC_TOK_E_READ_LEN;
    if (L->pos < 1) return CBC_TOK_E_POS;
    uint32_t n_cig = 0, n_md = 0, ev = 0, del_ins = 0;
    uint32_t st = cbc_tok_cigar(cig, ce, tk ? tk + 2 : tk, (int *)0, &n_cig, &ev, (long long *)0);
    if (st == CBC_TOK_OK) st = cbc_tok_md(md, me, tk ? tk + 2 + n_cig : tk, n_cig, &n_md, (long long *)0);
    if (st == CBC_TOK_OK) st = cbc_tok_replay(cig, ce, md, me, L->seq_len, n_md, 0, &del_ins);
    if (st != CBC_TOK_OK) return st;
    if (tk) { tk[0] = n_cig | (n_md << 16); tk[1] = del_ins; }
    *nt_out = 2u + n_cig + n_md; *ev_out = ev + n_md;
    return CBC_TOK_OK;
}

#endif /* CBC_TOK_CORE_H */
