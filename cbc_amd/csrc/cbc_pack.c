/*
 * cbc_pack.c -- host packer: SAM text + FASTA text -> packed record blocks for the HIP encoder.
 *
 * Restates, for the product, the parsing rules of the reference's record loader and FASTA loader
 * (they decide which bytes the models see, so they are load-bearing for bit-exactness):
 *   get_read_length()            src/sam_file_allocation.c:26-79
 *   store_reference_in_memory()  src/read_decompression.c:17-53
 *   the MD rebuild of compress_edits() behind a leading soft clip (quirk Q6)   src/read_compression.c:357-468
 * takes the rule for one SAM line (load_sam_line(), the CIGAR scan, the MD scan, the consistency replay) from
 * cbc_tok_core.h, which the device tokeniser runs too, keeping only the MD buffer that persists from line to line,
 * and cuts the record stream into independent blocks (hard part 1): one
 * contig per block, POS rebased so that the block's first record has POS 1, at most
 * opts.block_reads records, and never more distinct POS deltas / var symbols / FLAG values than
 * the kernel's LDS tables hold.
 *
 * No arithmetic coding happens here.
 */
#include <ctype.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <pthread.h>
#include <time.h>
#include <unistd.h>
#include "../../include/cbc_host.h"
#include "cbc_tok_core.h"          /* the rule for one SAM line: column split, CIGAR scan, MD scan, replay */

#define LINE_BUF 1024              /* fgets(buffer, 1024, ...) in the reference */
#define API __attribute__((visibility("default")))

/* ------------------------------------------------------------------------------------------ */
static int grow(void **p, uint64_t *cap, uint64_t need, size_t elt)
{
    if (need <= *cap) return 0;
    uint64_t nc = *cap ? *cap : 1024;
    while (nc < need) nc += nc / 2 + 1024;
    void *q = realloc(*p, (size_t)(nc * elt));
    if (!q) return CBC_E_NOMEM;
    *p = q; *cap = nc;
    return 0;
}
static int grow32(void **p, uint32_t *cap, uint64_t need, size_t elt)
{
    uint64_t c = *cap; int rc = grow(p, &c, need, elt);
    *cap = (uint32_t)c; return rc;
}

typedef struct {
    cbc_packed *P;
    cbc_pack_opts o;
    char *err; size_t errlen;
    /* current contig / block */
    char prev_name[LINE_BUF];
    int have_contig;
    uint32_t contig;               /* index of current contig */
    uint32_t n_fasta;              /* contigs available in ref */
    int blk_open;
    uint64_t blk_first_pos;        /* absolute POS of the block's first record */
    uint32_t blk_prev_pos;         /* absolute POS of the previous record in the block */
    uint32_t blk_reads, blk_var, blk_nflags, blk_ndelta;
    int seg_continues;             /* whole-file mode: the segment being opened continues the previous one's contig */
    uint64_t blk_bases;
    uint16_t blk_flags[CBC_CAP_FLAG];
    uint8_t *wf_seen;                                  /* whole-file mode: one bit per POS step below MAX_ALPHA seen so far */
    uint32_t *dset; uint32_t *dstamp; uint32_t dmask, depoch;   /* distinct-delta hash set */
    char edits[2 * LINE_BUF];      /* persists across records like read_line_t.edits */
    uint32_t tokbuf[4 * LINE_BUF];
} packer_t;

static int fail(packer_t *S, int code, const char *fmt, const char *a, long long b)
{
    if (S->err && S->errlen) snprintf(S->err, S->errlen, fmt, a ? a : "", b);
    return code;
}

/* FASTA: every record, in file order (the reference consumes the NEXT record at each RNAME change
 * and ignores the FASTA header text, read_decompression.c:28-42). */
static int load_fasta(packer_t *S, const char *fa, size_t len)
{
    cbc_packed *P = S->P;
    size_t off = 0;
    int first_line = 1, in_contig = 0;
    uint64_t start = 0;
    S->n_fasta = 0;
    while (off < len) {
        size_t e; { const char *nl = (const char *)memchr(fa + off, '\n', len - off); e = nl ? (size_t)(nl - fa) : len; }
        size_t ll = e - off;
        if (ll >= LINE_BUF - 1) return fail(S, CBC_E_INPUT, "FASTA line longer than %s1022 bytes at offset %lld (reference loader limit)", "", (long long)off);
        int is_hdr = (ll > 0 && fa[off] == '>') || (first_line && off == 0);
        if (is_hdr) {
            if (in_contig) {                            /* a '>' line ends the record being read */
                if (grow((void **)&P->ref, &P->cap_ref, P->ref_bytes + CBC_REF_PAD, 1)) return CBC_E_NOMEM;
                memset(P->ref + P->ref_bytes, 0, CBC_REF_PAD);
                if (grow32((void **)&P->contigs, &P->cap_contigs, (uint64_t)S->n_fasta + 1, sizeof(cbc_contig_info))) return CBC_E_NOMEM;
                P->contigs[S->n_fasta].ref_off = start; P->contigs[S->n_fasta].length = P->ref_bytes - start;
                P->contigs[S->n_fasta].name_off = 0; P->contigs[S->n_fasta].reserved = 0;
                P->ref_bytes += CBC_REF_PAD; S->n_fasta++;
            }
            in_contig = 1; start = P->ref_bytes;
        } else {
            if (!in_contig) { in_contig = 1; start = P->ref_bytes; }
            if (grow((void **)&P->ref, &P->cap_ref, P->ref_bytes + ll, 1)) return CBC_E_NOMEM;
            {   /* toupper() in the C locale, written so that it vectorises */
                uint8_t *d = P->ref + P->ref_bytes; const uint8_t *q = (const uint8_t *)fa + off;
                for (size_t i = 0; i < ll; i++) { uint8_t ch = q[i]; d[i] = (uint8_t)(ch - (((uint8_t)(ch - 'a') < 26u) << 5)); }
            }
            P->ref_bytes += ll;
        }
        first_line = 0;
        off = e + 1;
    }
    if (in_contig) {
        if (grow((void **)&P->ref, &P->cap_ref, P->ref_bytes + CBC_REF_PAD, 1)) return CBC_E_NOMEM;
        memset(P->ref + P->ref_bytes, 0, CBC_REF_PAD);
        if (grow32((void **)&P->contigs, &P->cap_contigs, (uint64_t)S->n_fasta + 1, sizeof(cbc_contig_info))) return CBC_E_NOMEM;
        P->contigs[S->n_fasta].ref_off = start; P->contigs[S->n_fasta].length = P->ref_bytes - start;
        P->contigs[S->n_fasta].name_off = 0; P->contigs[S->n_fasta].reserved = 0;
        P->ref_bytes += CBC_REF_PAD; S->n_fasta++;
    }
    return 0;
}

/* ---- the same loader on several threads: the text is cut at line starts; pass 1 counts,
 * per chunk, the header lines and the sequence bytes before / after each of them; a serial prefix turns the
 * counts into contig records and output offsets; pass 2 copies and upper-cases.  Byte-identical to
 * load_fasta() (tests).  Used for texts of 8 MiB and more. */
typedef struct {
    const char *fa; size_t beg, end, len;
    int first_chunk;
    /* pass 1 */
    uint64_t n_hdr, seq_before_first_hdr, seq_total; int too_long; size_t bad_off;
    uint64_t *seg; uint64_t cap_seg;             /* sequence bytes after each header line of the chunk */
    /* pass 2 */
    uint8_t *out; uint64_t out_pos;              /* where this chunk's first sequence byte goes */
    int phase;
} fa_chunk_t;

static inline int fa_is_hdr(const fa_chunk_t *c, size_t off, size_t ll) { return (ll > 0 && c->fa[off] == '>') || off == 0; }

static void *fa_run(void *arg)
{
    fa_chunk_t *c = (fa_chunk_t *)arg;
    const char *fa = c->fa;
    size_t off = c->beg;
    uint64_t cur = 0; int seen_hdr = 0;
    uint8_t *d = c->out ? c->out + c->out_pos : NULL;
    while (off < c->end) {
        const char *nl = (const char *)memchr(fa + off, '\n', c->len - off);
        size_t e = nl ? (size_t)(nl - fa) : c->len;
        size_t ll = e - off;
        if (c->phase == 1 && ll >= LINE_BUF - 1 && !c->too_long) { c->too_long = 1; c->bad_off = off; }
        if (fa_is_hdr(c, off, ll)) {
            if (c->phase == 1) {
                if (!seen_hdr) c->seq_before_first_hdr = cur; else c->seg[c->n_hdr - 1] = cur;
                if (grow((void **)&c->seg, &c->cap_seg, c->n_hdr + 1, sizeof(uint64_t))) { c->too_long = 2; return NULL; }
                c->n_hdr++; seen_hdr = 1; cur = 0;
            } else if (off != 0) {                 /* a header line closes the contig before it: its pad */
                memset(d, 0, CBC_REF_PAD); d += CBC_REF_PAD;
            }
        } else if (c->phase == 1) { cur += ll; c->seq_total += ll; }
        else {
            const uint8_t *q = (const uint8_t *)fa + off;
            for (size_t i = 0; i < ll; i++) { uint8_t ch = q[i]; d[i] = (uint8_t)(ch - (((uint8_t)(ch - 'a') < 26u) << 5)); }
            d += ll;
        }
        off = e + 1;
    }
    if (c->phase == 1) { if (!seen_hdr) c->seq_before_first_hdr = cur; else c->seg[c->n_hdr - 1] = cur; }
    return NULL;
}

static int load_fasta_mt(packer_t *S, const char *fa, size_t len, int nthreads)
{
    cbc_packed *P = S->P;
    fa_chunk_t *ch = (fa_chunk_t *)calloc((size_t)nthreads, sizeof(fa_chunk_t));
    pthread_t *th = (pthread_t *)calloc((size_t)nthreads, sizeof(pthread_t));
    int rc = 0;
    if (!ch || !th) { free(ch); free(th); return CBC_E_NOMEM; }
    size_t b = 0;
    for (int t = 0; t < nthreads; t++) {
        size_t e = (t == nthreads - 1) ? len : len / (size_t)nthreads * (size_t)(t + 1);
        if (e < b) e = b;
        if (e < len && t != nthreads - 1) { const char *nl = (const char *)memchr(fa + e, '\n', len - e); e = nl ? (size_t)(nl - fa) + 1 : len; }
        ch[t].fa = fa; ch[t].beg = b; ch[t].end = e; ch[t].len = len; ch[t].phase = 1; b = e;
    }
    for (int pass = 1; pass <= 2 && !rc; pass++) {
        int started = 0;
        for (int t = 0; t < nthreads; t++) { ch[t].phase = pass; if (pthread_create(&th[t], NULL, fa_run, &ch[t]) != 0) break; started++; }
        for (int t = started; t < nthreads; t++) fa_run(&ch[t]);
        for (int t = 0; t < started; t++) pthread_join(th[t], NULL);
        if (pass == 2) break;
        /* serial prefix: contig records and output offsets */
        for (int t = 0; t < nthreads && !rc; t++) {
            if (ch[t].too_long == 2) rc = CBC_E_NOMEM;
            else if (ch[t].too_long) rc = fail(S, CBC_E_INPUT, "FASTA line longer than %s1022 bytes at offset %lld (reference loader limit)", "", (long long)ch[t].bad_off);
        }
        if (rc) break;
        uint64_t n_hdr = 0, seq = 0;
        for (int t = 0; t < nthreads; t++) { n_hdr += ch[t].n_hdr; seq += ch[t].seq_total; }
        S->n_fasta = 0;
        if (n_hdr == 0) break;                                    /* empty text: no contig (len == 0) */
        uint64_t total = seq + n_hdr * CBC_REF_PAD;               /* one pad after every contig */
        if (grow((void **)&P->ref, &P->cap_ref, total, 1) ||
            grow32((void **)&P->contigs, &P->cap_contigs, n_hdr, sizeof(cbc_contig_info))) { rc = CBC_E_NOMEM; break; }
        uint64_t pos = 0; uint64_t cur_start = 0, cur_len = 0; int open = 0; uint32_t nc = 0;
        for (int t = 0; t < nthreads; t++) {
            ch[t].out = P->ref; ch[t].out_pos = pos;
            cur_len += ch[t].seq_before_first_hdr; pos += ch[t].seq_before_first_hdr;
            for (uint64_t k = 0; k < ch[t].n_hdr; k++) {
                if (open) {                                       /* this header closes the contig before it */
                    P->contigs[nc].ref_off = cur_start; P->contigs[nc].length = cur_len; P->contigs[nc].name_off = 0; P->contigs[nc].reserved = 0;
                    nc++; pos += CBC_REF_PAD;
                }
                open = 1; cur_start = pos; cur_len = ch[t].seg[k]; pos += ch[t].seg[k];
            }
        }
        P->contigs[nc].ref_off = cur_start; P->contigs[nc].length = cur_len; P->contigs[nc].name_off = 0; P->contigs[nc].reserved = 0;
        nc++;
        memset(P->ref + pos, 0, CBC_REF_PAD); pos += CBC_REF_PAD;
        P->ref_bytes = pos; S->n_fasta = nc;
    }
    for (int t = 0; t < nthreads; t++) free(ch[t].seg);
    free(ch); free(th);
    return rc;
}

static int online_cpus(void)
{
    long nc = sysconf(_SC_NPROCESSORS_ONLN);
    return nc < 1 ? 1 : nc > 64 ? 64 : (int)nc;
}
/* the FASTA loader behind both the packer and the unpack plan: threaded for big texts */
static int load_reference(packer_t *S, const char *fa, size_t len, uint32_t n_threads)
{
    int nt = n_threads ? (int)n_threads : online_cpus();
    if (nt > 64) nt = 64;
    if (nt > 1 && (n_threads > 1 || len >= ((size_t)8 << 20))) return load_fasta_mt(S, fa, len, nt);
    return load_fasta(S, fa, len);
}

static void close_block(packer_t *S)
{
    cbc_packed *P = S->P;
    if (!S->blk_open) return;
    cbc_block_desc *bd = &P->blocks[P->n_blocks];
    cbc_block_info *bi = &P->info[P->n_blocks];
    bd->n_reads = S->blk_reads;
    bd->n_tok = (uint32_t)(P->n_tok - bd->tok_base);
    bi->n_reads = S->blk_reads; bi->n_bases = S->blk_bases;
    uint32_t need_pos = S->blk_ndelta + 2, need_var = S->blk_var + 1;
    if (need_pos > P->caps.cap_pos) P->caps.cap_pos = need_pos;
    if (need_var > P->caps.cap_var) P->caps.cap_var = need_var;
    P->n_blocks++;
    S->blk_open = 0;
}

static int open_block(packer_t *S, uint32_t pos)
{
    cbc_packed *P = S->P;
    if (grow32((void **)&P->blocks, &P->cap_blocks, (uint64_t)P->n_blocks + 1, sizeof(cbc_block_desc))) return CBC_E_NOMEM;
    {   /* info array shares the block capacity */
        cbc_block_info *ni = (cbc_block_info *)realloc(P->info, sizeof(cbc_block_info) * (size_t)P->cap_blocks);
        if (!ni) return CBC_E_NOMEM;
        P->info = ni;
    }
    cbc_block_desc *bd = &P->blocks[P->n_blocks];
    cbc_block_info *bi = &P->info[P->n_blocks];
    memset(bd, 0, sizeof *bd); memset(bi, 0, sizeof *bi);
    const cbc_contig_info *c = &P->contigs[S->contig];
    bd->rec_base = P->n_recs; bd->seq_base = P->seq_bytes; bd->tok_base = P->n_tok;
    if (S->o.whole_file) pos = 1;                       /* a segment of the whole-file stream keeps the SAM's POS */
    bd->ref_off = c->ref_off + (uint64_t)(pos - 1);
    bd->name_off = c->name_off; bd->read_length = P->read_length;
    bi->contig = S->contig; bi->window_start = (uint64_t)(pos - 1);
    S->blk_open = 1; S->blk_first_pos = pos;
    S->blk_reads = 0; S->blk_bases = 0;
    if (S->o.whole_file && S->seg_continues) { S->seg_continues = 0; return 0; }   /* same contig, same stream state */
    S->blk_prev_pos = 0;
    if (S->o.whole_file) return 0;                      /* the models run on: flags and POS steps count per file */
    S->blk_var = 0; S->blk_nflags = 0; S->blk_ndelta = 0;
    S->depoch++;
    if (S->depoch == 0) { memset(S->dstamp, 0, sizeof(uint32_t) * (S->dmask + 1)); S->depoch = 1; }
    return 0;
}

static int delta_seen(packer_t *S, uint32_t x, int insert)
{
    uint32_t h = (x * 2654435761u) & S->dmask;
    for (;;) {
        if (S->dstamp[h] != S->depoch) {
            if (insert) { S->dstamp[h] = S->depoch; S->dset[h] = x; }
            return 0;
        }
        if (S->dset[h] == x) return 1;
        h = (h + 1) & S->dmask;
    }
}

/* RNAME change (compress_rname strcmp, id_compression.c:46): the next FASTA record becomes current. */
static int contig_open(packer_t *S, const char *rname, size_t nl)
{
    cbc_packed *P = S->P;
    close_block(S);
    uint32_t ci = S->have_contig ? S->contig + 1 : 0;
    char nm[64]; snprintf(nm, sizeof nm, "%.*s", (int)(nl < 60 ? nl : 60), rname);
    if (ci >= S->n_fasta) return fail(S, CBC_E_INPUT, "RNAME %s is contig #%lld of the SAM but the FASTA has fewer records (contigs are consumed in FASTA order)", nm, (long long)ci + 1);
    if (nl + 3 > CBC_CAP_NAME) return fail(S, CBC_E_INPUT, "RNAME %s longer than %lld characters", nm, (long long)CBC_CAP_NAME - 3);
    if (grow32((void **)&P->names, &P->cap_names, (uint64_t)P->names_bytes + nl + 1, 1)) return CBC_E_NOMEM;
    memcpy(P->names + P->names_bytes, rname, nl); P->names[P->names_bytes + nl] = 0;
    P->contigs[ci].name_off = P->names_bytes;
    P->names_bytes += (uint32_t)nl + 1;
    S->contig = ci; S->have_contig = 1;
    if (P->n_contigs < ci + 1) P->n_contigs = ci + 1;
    return 0;
}


/* ---- MD text derived from an alignment (quirk Q6: what the reference's compress_edits leaves in the record's
 * MD buffer when the CIGAR starts with a soft clip and the read is imperfect, read_compression.c:357-468).
 * Walk the ops after the clip with a cursor in the read (starts behind the clip) and one in the contig (starts
 * at POS): an M op compares base by base and writes "<run><contig letter>" for every mismatch (run 0 included);
 * I skips read bases; D closes the current run (only if > 0), writes '^' and the deleted contig letters -- taken
 * one base FURTHER than the cursor (no -1 there, :425) -- and moves the contig cursor; a trailing S only closes
 * the run; at the end the run is written if > 0.  Nothing terminates the text except the NUL that comes with a
 * number, so when the last thing written is a letter the buffer's older content follows it (:460 clears a
 * pointer, not the string) -- which is why this writes into the persistent buffer and not into a fresh one.
 * Returns 0, -1 = an op runs past SEQ or past the contig + pad, -2 = no room in the buffer. */
typedef struct { char *at, *end; } md_text;
static int md_number(md_text *w, uint32_t v)
{
    if (w->end - w->at < 12) return -2;
    w->at += sprintf(w->at, "%u", v);            /* leaves its NUL at *w->at */
    return 0;
}
static int md_letter(md_text *w, uint8_t c)
{
    if (w->end - w->at < 2) return -2;
    *w->at++ = (char)c;                          /* no terminator: see above */
    return 0;
}
static int md_from_alignment(char *buf, size_t buf_len, const uint32_t *ops, uint32_t n_ops, uint32_t clip_len,
                             const uint8_t *read, uint32_t read_len, const uint8_t *contig, uint32_t pos, uint64_t contig_avail)
{
    md_text w = { buf, buf + buf_len };
    uint64_t in_read = clip_len, in_contig = pos;         /* next read index (0-based); next contig base (1-based) */
    uint32_t run = 0;
    int rc = 0;
    for (uint32_t k = 0; k < n_ops && !rc; k++) {
        const uint32_t kind = ops[k] & 15u; const uint64_t n = ops[k] >> 4;
        if (kind == CBC_OP_M) {
            if (in_read + n > read_len || in_contig - 1 + n > contig_avail) return -1;
            for (uint64_t j = 0; j < n && !rc; j++) {
                const uint8_t have = read[in_read + j], want = contig[in_contig - 1 + j];
                if (have == want) run++;
                else { rc = md_number(&w, run); if (!rc) rc = md_letter(&w, want); run = 0; }
            }
            in_read += n; in_contig += n;
        } else if (kind == CBC_OP_I) in_read += n;
        else if (kind == CBC_OP_D) {
            if (in_contig + n > contig_avail) return -1;
            if (run) { rc = md_number(&w, run); run = 0; }
            if (!rc) rc = md_letter(&w, '^');
            for (uint64_t j = 0; j < n && !rc; j++) rc = md_letter(&w, (uint8_t)toupper(contig[in_contig + j]));
            in_contig += n;
        } else if (kind == CBC_OP_S) { if (run) { rc = md_number(&w, run); run = 0; } }
    }
    if (!rc && run) rc = md_number(&w, run);
    return rc;
}

/* CIGAR + MD of one mapped record (columns by pointer and length; the MD text: S->edits) -> token words tk[0..*nt_out)
 * and the record's var-symbol bound.  The scans are cbc_tok_core.h's; what this packer adds is the contig-end check and quirk
 * Q6, which sits between the CIGAR scan and the MD scan because it rewrites the text the MD scan reads.
 * Reads only shared, already final state (P->ref, the contig table), so worker threads may call it. */
static int tokenise_record(packer_t *S, const cbc_contig_info *ctg, int32_t pos_i, const char *cigar, size_t cl,
                           const char *seq, size_t rl, uint32_t *tk, uint32_t *nt_out, uint32_t *ev_out)
{
    cbc_packed *P = S->P;
    const char *rname = (const char *)P->names + ctg->name_off;
    const uint8_t *cig = (const uint8_t *)cigar, *ce = cig + cl;
    if (rl == 0 || rl > CBC_MAX_READ_LEN)
        return fail(S, CBC_E_INPUT, "read length %s%lld outside 1..252 (var-context limit of the reference, sam_models.c:317)", "", (long long)rl);
    if (pos_i < 1) return fail(S, CBC_E_INPUT, "POS %s%lld < 1", "", pos_i);
    const uint32_t pos = (uint32_t)pos_i;
    if ((uint64_t)pos - 1 + rl > ctg->length + CBC_REF_PAD - 8)
        return fail(S, CBC_E_INPUT, "record at %s POS %lld runs past the contig end + pad", rname, pos);

    uint32_t n_cig = 0, n_md = 0, ev = 0, del_ins = 0;   /* ev: upper bound on var symbols of this record */
    int lead_clip = 0;                                  /* the first CIGAR op is a soft clip (quirk Q6) */
    long long bad = 0;
    uint32_t st = cbc_tok_cigar(cig, ce, tk + 2, &lead_clip, &n_cig, &ev, &bad);
    if (st != CBC_TOK_OK) {
        char text[LINE_BUF]; snprintf(text, sizeof text, "%.*s", (int)cl, cigar);
        if (st == CBC_TOK_E_CIGAR) return fail(S, CBC_E_INPUT, "CIGAR %s: bad length %lld", text, bad);
        if (st == CBC_TOK_E_STAR) return fail(S, CBC_E_INPUT, "CIGAR '*' on a mapped record at %s:%lld (the reference aborts on it)", rname, pos);
        return fail(S, CBC_E_INPUT, "CIGAR %s too long%lld", text, 0);
    }
    if (lead_clip) {
        /* Leading soft clip (quirk Q6, read_compression.c:357-468).  The clipped bases are coded exactly like
         * an insertion at matched coordinate 0 (the scan stored the op as CBC_OP_I, which the kernels
         * already code that way), and for an IMPERFECT read the reference first replaces the record's MD
         * text by one it derives from the alignment itself (over the ops after the clip).  Only then. */
        const uint8_t *contig_bases = P->ref + ctg->ref_off;
        if (memcmp(seq, contig_bases + (pos - 1), rl) != 0) {
            int rc = md_from_alignment(S->edits, 2 * LINE_BUF, tk + 3, n_cig - 1, tk[2] >> 4, (const uint8_t *)seq, (uint32_t)rl,
                                       contig_bases, pos, ctg->length + CBC_REF_PAD);
            if (rc == -1) return fail(S, CBC_E_INPUT, "CIGAR of the soft-clipped record at %s:%lld runs past SEQ or past the contig", rname, pos);
            if (rc == -2) return fail(S, CBC_E_INPUT, "derived MD too long at %s:%lld", rname, pos);
        }
    }
    /* S->edits is deliberately not terminated by what Q6 wrote: the text runs to the first NUL, whoever left it there */
    const uint8_t *md = (const uint8_t *)S->edits, *me = md + strlen(S->edits);
    st = cbc_tok_md(md, me, tk + 2 + n_cig, n_cig, &n_md, &bad);
    if (st == CBC_TOK_E_MD) return fail(S, CBC_E_INPUT, "MD %s: gap %lld too large", S->edits, bad);
    if (st != CBC_TOK_OK) return fail(S, CBC_E_INPUT, "MD %s too long%lld", S->edits, 0);
    st = cbc_tok_replay(cig, ce, md, me, (uint32_t)rl, n_md, lead_clip, &del_ins);
    if (st == CBC_TOK_E_INCONSISTENT)
        return fail(S, CBC_E_INPUT, "MD:Z:%s is inconsistent with CIGAR/SEQ at POS %lld (it names more bases than the read has)", S->edits, pos);
    if (st != CBC_TOK_OK) return fail(S, CBC_E_INPUT, "too many inserted/deleted bases%s%lld", "", 0);
    tk[0] = n_cig | (n_md << 16); tk[1] = del_ins;
    ev += n_md;
    if (ev + 1 > S->o.max_cap_var) return fail(S, CBC_E_INPUT, "record at %s:%lld has more edits than max_cap_var", rname, pos);
    *nt_out = 2 + n_cig + n_md; *ev_out = ev;
    return 0;
}

/* Block cut decision + the record's cbc_read_rec.  Advances P->seq_bytes / P->n_tok as counters; the
 * caller stores the SEQ bytes and token words at the offsets they had on entry. */
static int place_record(packer_t *S, uint32_t pos, uint32_t flag, size_t rl, uint32_t ev, uint32_t nt)
{
    cbc_packed *P = S->P;
    const char *rname = (const char *)P->names + P->contigs[S->contig].name_off;
    int need_new = !S->blk_open;
    uint32_t x = 0;
    if (S->o.whole_file) {
        /* one stream per file: cut only where a 32-bit offset of cbc_read_rec would overflow */
        if (S->blk_open) {
            const cbc_block_desc *cur = &P->blocks[P->n_blocks];
            if (pos < S->blk_prev_pos) return fail(S, CBC_E_INPUT, "SAM is not sorted by position at %s:%lld", rname, pos);
            if (P->seq_bytes - cur->seq_base + rl > 0xfff00000ull || P->n_tok - cur->tok_base + nt > 0xfff00000ull ||
                S->blk_reads >= 0xfff00000u) { need_new = 1; S->seg_continues = 1; }
        }
        x = pos - (S->blk_open ? S->blk_prev_pos : 0u) + 1;   /* prevPos is 0 at a contig's first record (compress_pos :123-124) */
        if (x >= 5000000u)
            return fail(S, CBC_E_INPUT, "POS step of 5 000 000 or more at %s:%lld: outside the reference's pos alphabet (MAX_ALPHA); use block mode", rname, pos);
        if (need_new) { close_block(S); int rc = open_block(S, pos); if (rc) return rc; }
        /* every POS step below MAX_ALPHA and every 16-bit FLAG is in the reference's tables (sam_block.h:54-55,
         * sam_models.c:96-130), so the whole-file stream takes them all: the stream kernels keep what does not fit their
         * registers / LDS in global memory.  The distinct steps are counted exactly (one bit per possible step): the
         * count sizes the kernels' pos tables. */
        if (!(S->wf_seen[x >> 3] & (1u << (x & 7u)))) { S->wf_seen[x >> 3] |= (uint8_t)(1u << (x & 7u)); S->blk_ndelta++; }
        goto record;
    }
    if (S->blk_open) {
        if (pos < S->blk_prev_pos) return fail(S, CBC_E_INPUT, "SAM is not sorted by position at %s:%lld", rname, pos);
        x = pos - S->blk_prev_pos + 1;
        int newflag = 1;
        for (uint32_t i = 0; i < S->blk_nflags; i++) if (S->blk_flags[i] == (uint16_t)flag) { newflag = 0; break; }
        int newdelta = !delta_seen(S, x, 0);
        if (S->blk_reads >= S->o.block_reads) need_new = 1;
        else if (S->o.long_reads && S->blk_bases + rl > CBC_LONG_BLOCK_BASES) need_new = 1;
        else if (x >= 5000000u && !S->o.long_reads) need_new = 1;              /* MAX_ALPHA sam_block.h:54 */
        else if (newdelta && S->blk_ndelta + 3 > S->o.max_cap_pos) need_new = 1;
        else if (S->blk_var + ev + 1 > S->o.max_cap_var) need_new = 1;
        else if (newflag && S->blk_nflags >= CBC_CAP_FLAG) need_new = 1;
        else if ((uint64_t)pos - S->blk_first_pos > 0xfff00000ull) need_new = 1;
    }
    if (need_new) {
        close_block(S);
        int rc = open_block(S, pos);
        if (rc) return rc;
        x = 2;                                          /* local POS 1, prevPos 0 */
    }
    if (!delta_seen(S, x, 1)) S->blk_ndelta++;
    {
        int newflag = 1;
        for (uint32_t i = 0; i < S->blk_nflags; i++) if (S->blk_flags[i] == (uint16_t)flag) { newflag = 0; break; }
        if (newflag) S->blk_flags[S->blk_nflags++] = (uint16_t)flag;
    }
    S->blk_var += ev;

record:;
    /* ---- record ---- */
    cbc_block_desc *bd = &P->blocks[P->n_blocks];
    if (grow((void **)&P->recs, &P->cap_recs, P->n_recs + 1, sizeof(cbc_read_rec))) return CBC_E_NOMEM;
    cbc_read_rec *r = &P->recs[P->n_recs++];
    r->pos = (uint32_t)((uint64_t)pos - S->blk_first_pos + 1);
    r->flag = (uint16_t)flag; r->rlen = (uint16_t)rl;
    r->seq_off = (uint32_t)(P->seq_bytes - bd->seq_base);
    r->tok_off = (uint32_t)(P->n_tok - bd->tok_base);
    P->seq_bytes += rl; P->n_tok += nt;
    S->blk_reads++; S->blk_bases += rl; S->blk_prev_pos = pos;
    P->n_bases += rl;
    if (rl > P->max_read_len) P->max_read_len = (uint32_t)rl;
    return 0;
}

/* One mapped record of the serial path: the columns by pointer and length, the MD text in S->edits. */
static int add_record(packer_t *S, const char *rname, size_t nl, uint32_t flag, int32_t pos_i, const char *cigar, size_t cl,
                      const char *seq, size_t rl)
{
    cbc_packed *P = S->P;
    if (!S->have_contig || nl != strlen(S->prev_name) || memcmp(rname, S->prev_name, nl) != 0) {
        int rc = contig_open(S, rname, nl);
        if (rc) return rc;
        memcpy(S->prev_name, rname, nl); S->prev_name[nl] = 0;
    }
    uint32_t nt = 0, ev = 0;
    int rc = tokenise_record(S, &P->contigs[S->contig], pos_i, cigar, cl, seq, rl, S->tokbuf, &nt, &ev);
    if (rc) return rc;
    uint64_t so = P->seq_bytes, to = P->n_tok;
    if (grow((void **)&P->seq, &P->cap_seq, so + rl + 8, 1)) return CBC_E_NOMEM;
    if (grow((void **)&P->tok, &P->cap_tok, to + nt, sizeof(uint32_t))) return CBC_E_NOMEM;
    rc = place_record(S, (uint32_t)pos_i, flag, rl, ev, nt);
    if (rc) return rc;
    memcpy(P->seq + so, seq, rl);
    memcpy(P->tok + to, S->tokbuf, sizeof(uint32_t) * nt);
    return 0;
}


/* ================================= long-read format ====================== */
/* One mapped record of a long-read SAM: fields by pointer and length (lines are not copied: a 10 kb read's line
 * is ~20 kB).  Tokens: word 0 = n_cigar, word 1 = 0, then (len << 4) | op per CIGAR op; MD is not used -- the
 * kernels derive the edits from read vs reference.  SEQ must be over {A,C,G,T,N} so that the round trip is exact
 * (the base models code basepair classes, sam_models.c:11-33). */
static int add_record_long(packer_t *S, const char *rname, size_t nl, uint32_t flag, int64_t pos_i, const char *cigar, size_t cl,
                           const char *seq, size_t rl)
{
    cbc_packed *P = S->P;
    if (!S->have_contig || nl != strlen(S->prev_name) || memcmp(rname, S->prev_name, nl) != 0) {
        if (nl >= LINE_BUF) return fail(S, CBC_E_INPUT, "RNAME longer than %s%lld characters", "", (long long)LINE_BUF - 1);
        int rc = contig_open(S, rname, nl);
        if (rc) return rc;
        memcpy(S->prev_name, rname, nl); S->prev_name[nl] = 0;
    }
    const cbc_contig_info *ctg = &P->contigs[S->contig];
    const char *nm = (const char *)P->names + ctg->name_off;
    if (rl == 0 || rl > CBC_LONG_MAX_READ_LEN) return fail(S, CBC_E_INPUT, "read length %s%lld outside 1..65535", "", (long long)rl);
    if (pos_i < 1 || pos_i > 0x7fffffff) return fail(S, CBC_E_INPUT, "POS %s%lld outside 1..2^31-1", "", (long long)pos_i);
    for (size_t i = 0; i < rl; i++) {
        char c = seq[i];
        if (!(c == 'A' || c == 'C' || c == 'G' || c == 'T' || c == 'N'))
            return fail(S, CBC_E_INPUT, "SEQ at %s:%lld holds a character outside ACGTN (long-read format)", nm, (long long)pos_i);
    }
    /* CIGAR -> tokens, and what it consumes */
    uint64_t to = P->n_tok, nt = 2, in_read = 0, in_ref = 0; uint32_t n_cig = 0;
    {
        size_t i = 0;
        while (i < cl) {
            uint64_t v = 0; size_t d0 = i;
            while (i < cl && cigar[i] >= '0' && cigar[i] <= '9') { v = v * 10 + (uint64_t)(cigar[i] - '0'); if (v > 0x0fffffff) break; i++; }
            if (i >= cl || i == d0 || v == 0 || v > 0x0fffffff) return fail(S, CBC_E_INPUT, "malformed CIGAR at %s:%lld", nm, (long long)pos_i);
            char c = cigar[i++];
            uint32_t op;
            if (c == 'M' || c == '=' || c == 'X') { op = CBC_OP_M; in_read += v; in_ref += v; }
            else if (c == 'I' || c == 'S') { op = (c == 'I') ? CBC_OP_I : CBC_OP_S; in_read += v; }
            else if (c == 'D' || c == 'N') { op = CBC_OP_D; in_ref += v; }
            else if (c == 'H' || c == 'P') continue;                      /* consume nothing, code nothing */
            else return fail(S, CBC_E_INPUT, "CIGAR operation not understood at %s:%lld", nm, (long long)pos_i);
            if (grow((void **)&P->tok, &P->cap_tok, to + nt + 1, sizeof(uint32_t))) return CBC_E_NOMEM;
            P->tok[to + nt++] = ((uint32_t)v << 4) | op; n_cig++;
            if (n_cig > 0xffff) return fail(S, CBC_E_INPUT, "more than 65535 CIGAR operations at %s:%lld", nm, (long long)pos_i);
        }
    }
    if (in_read != rl) return fail(S, CBC_E_INPUT, "CIGAR and SEQ lengths differ at %s:%lld", nm, (long long)pos_i);
    if ((uint64_t)pos_i - 1 + in_ref > ctg->length + CBC_REF_PAD - 8) return fail(S, CBC_E_INPUT, "record at %s POS %lld runs past the contig end + pad", nm, (long long)pos_i);
    if (grow((void **)&P->tok, &P->cap_tok, to + 2, sizeof(uint32_t))) return CBC_E_NOMEM;
    P->tok[to] = n_cig; P->tok[to + 1] = 0;
    uint64_t so = P->seq_bytes;
    if (grow((void **)&P->seq, &P->cap_seq, so + rl + 8, 1)) return CBC_E_NOMEM;
    int rc = place_record(S, (uint32_t)pos_i, flag, rl, 0, (uint32_t)nt);
    if (rc) return rc;
    memcpy(P->seq + so, seq, rl);
    return 0;
}

/* the body of a long-read SAM: lines of any length, the 11 compulsory columns by tab */
static int pack_body_long(packer_t *S, const char *sam, size_t off, size_t sam_len)
{
    while (off < sam_len) {
        const char *nlp = (const char *)memchr(sam + off, '\n', sam_len - off);
        size_t e = nlp ? (size_t)(nlp - sam) : sam_len;
        const char *f[11]; size_t fl[11]; int nf = 0;
        size_t p = off;
        while (nf < 11 && p <= e) {
            const char *t = (const char *)memchr(sam + p, '\t', e - p);
            size_t q = t ? (size_t)(t - sam) : e;
            f[nf] = sam + p; fl[nf] = q - p; nf++;
            if (!t) break;
            p = q + 1;
        }
        size_t line_off = off;
        off = e + 1;
        if (nf == 0 || (nf == 1 && fl[0] == 0)) continue;
        if (nf < 11) return fail(S, CBC_E_INPUT, "SAM record with fewer than 11 columns near offset %s%lld", "", (long long)line_off);
        char num[24]; size_t l = fl[1] < 23 ? fl[1] : 23; memcpy(num, f[1], l); num[l] = 0;
        uint32_t flag = (uint16_t)atoi(num);
        if ((flag & 4) == 4) { S->P->n_skipped_unmapped++; continue; }
        l = fl[3] < 23 ? fl[3] : 23; memcpy(num, f[3], l); num[l] = 0;
        int rc = add_record_long(S, f[2], fl[2], flag, atoll(num), f[5], fl[5], f[9], fl[9]);
        if (rc) return rc;
    }
    return 0;
}

static int finish_pack(packer_t *S)
{
    cbc_packed *P = S->P;
    close_block(S);
    if (grow((void **)&P->seq, &P->cap_seq, P->seq_bytes + 8, 1)) return CBC_E_NOMEM;
    memset(P->seq + P->seq_bytes, 0, 8); P->seq_bytes += 8;          /* the kernel reads whole dwords */
    if (P->caps.cap_pos < 64) P->caps.cap_pos = 64;
    if (P->caps.cap_var < 64) P->caps.cap_var = 64;
    P->caps.cap_pos = (P->caps.cap_pos + 63u) & ~63u;
    P->caps.cap_var = (P->caps.cap_var + 63u) & ~63u;
    if (P->n_tok == 0) { if (grow((void **)&P->tok, &P->cap_tok, 1, sizeof(uint32_t))) return CBC_E_NOMEM; P->tok[0] = 0; }
    P->whole_file = S->o.long_reads ? 2u : S->o.whole_file ? 1u : 0u;
    return 0;
}

static int packer_init(packer_t *S, const cbc_pack_opts *opts, char *errbuf, size_t errlen)
{
    memset(S, 0, sizeof *S);
    if (opts) S->o = *opts; else cbc_pack_default_opts(&S->o);
    if (S->o.long_reads) {                                  /* blocks are cut by bases: 64 reads of 10 kb fill one */
        S->o.whole_file = 0;
        if (S->o.block_reads == 0 || S->o.block_reads > 64) S->o.block_reads = 64;   /* format limit: the per-read models keep <= 64 entries */
    }
    if (S->o.block_reads == 0) S->o.block_reads = 4096;
    if (S->o.block_reads > CBC_MAX_BLOCK_READS) S->o.block_reads = CBC_MAX_BLOCK_READS;
    if (S->o.max_cap_pos < 64) S->o.max_cap_pos = 2048;
    if (S->o.max_cap_var < 64) S->o.max_cap_var = 8192;
    if (S->o.whole_file) S->o.max_cap_pos = 8192;                  /* (sizes the hash set below, which whole-file mode does not use) */
    if (S->o.max_cap_pos > 4096 && !S->o.whole_file) S->o.max_cap_pos = 4096;
    if (S->o.max_cap_var > 32768) S->o.max_cap_var = 32768;       /* keeps L0 + 10*uses < 2^20 */
    S->err = errbuf; S->errlen = errlen;
    if (errbuf && errlen) errbuf[0] = 0;
    S->P = (cbc_packed *)calloc(1, sizeof(cbc_packed));
    if (!S->P) return CBC_E_NOMEM;
    uint32_t sz = 1; while (sz < 4 * S->o.max_cap_pos) sz <<= 1;
    S->dmask = sz - 1;
    S->dset = (uint32_t *)calloc(sz, sizeof(uint32_t));
    S->dstamp = (uint32_t *)calloc(sz, sizeof(uint32_t));
    if (!S->dset || !S->dstamp) return CBC_E_NOMEM;
    S->depoch = 1;                                  /* stamps start at 0 = "never used" */
    if (S->o.whole_file) {
        S->wf_seen = (uint8_t *)calloc(5000000u / 8u + 1u, 1);
        if (!S->wf_seen) return CBC_E_NOMEM;
    }
    return 0;
}
static void packer_release(packer_t *S) { free(S->dset); free(S->dstamp); free(S->wf_seen); }

API void cbc_pack_default_opts(cbc_pack_opts *o)
{
    o->block_reads = 4096; o->max_cap_pos = 2048; o->max_cap_var = 8192; o->var_length = 0; o->n_threads = 0; o->whole_file = 0; o->long_reads = 0;
}

API void cbc_packed_free(cbc_packed *p)
{
    if (!p) return;
    free(p->recs); free(p->seq); free(p->tok); free(p->names); free(p->blocks); free(p->info);
    free(p->contigs); free(p->ref); free(p);
}
API void cbc_free(void *p) { free(p); }

/* get_read_length (sam_file_allocation.c:26-79): skip '@' lines, skip the first record line, take
 * the 10th whitespace-separated field of what follows; a file with a single record makes the
 * reference's fscanf fail and it returns strlen() of that first line. */
static uint32_t header_read_length(const char *sam, size_t len, size_t *body_off, int var_length)
{
    size_t off = 0;
    while (off < len && sam[off] == '@') { while (off < len && sam[off] != '\n') off++; if (off < len) off++; }
    *body_off = off;
    size_t e = off; while (e < len && sam[e] != '\n') e++;
    size_t first_len = (e < len ? e + 1 : e) - off; if (first_len > 4095) first_len = 4095;
    size_t q = e < len ? e + 1 : e;
    uint32_t result = 0; int got = 0;
    for (;;) {
        int field = 0; size_t s = q, t = q; int ok = 0;
        while (s < len) {
            while (s < len && isspace((unsigned char)sam[s])) s++;
            if (s >= len) break;
            t = s; while (t < len && !isspace((unsigned char)sam[t])) t++;
            if (++field == 10) { ok = 1; break; }
            s = t;
        }
        if (!ok) break;
        uint32_t l = (uint32_t)(t - s);
        if (!var_length) { result = l; got = 1; break; }
        if (l > result) result = l;
        got = 1;
        while (t < len && sam[t] != '\n') t++;
        if (t >= len) break;
        q = t + 1;
    }
    if (!got && !var_length) return (uint32_t)first_len;
    return result;
}

/* one past the '\n' of the line that starts at b: a line keeps its '\n', as fgets leaves it */
static inline size_t line_end(const char *sam, size_t b, size_t end)
{
    const char *nl = (const char *)memchr(sam + b, '\n', end - b);
    return nl ? (size_t)(nl - sam) + 1 : end;
}
/* One text line [b, e) -> the column split of cbc_tok_core.h, and the MD/XD text copied into S->edits, which otherwise keeps
 * the previous line's value (read_line_t.edits persists, sam_file_allocation.c:437-529; an unmapped line's text counts too).
 * Returns CBC_TOK_OK = mapped record, CBC_TOK_UNMAPPED, CBC_TOK_SKIP = nothing on the line, < 0 = error. */
static int split_line(packer_t *S, const char *sam, size_t b, size_t e, cbc_tok_line *L)
{
    cbc_tok_split((const uint8_t *)sam, b, e, L);
    if (L->status == CBC_TOK_E_LINE_LONG) return fail(S, CBC_E_INPUT, "SAM line longer than %s1023 bytes at offset %lld (reference fgets limit)", "", (long long)b);
    if (L->status == CBC_TOK_E_COLUMNS) return fail(S, CBC_E_INPUT, "SAM record with fewer than 11 columns near offset %s%lld", "", (long long)e);
    if (L->has_md > 1) {
        /* load_sam_line() copies every MD / XD field as it meets it, so a longer earlier one leaves its tail behind the last
         * one's NUL, where quirk Q6's unterminated text can expose it.  The field before the last is the last one of the line
         * cut off where the last one's token starts: do that first. */
        size_t cut = L->md;
        while (cut > b && sam[cut - 1] != '\t') cut--;
        cbc_tok_line before;
        (void)split_line(S, sam, b, cut, &before);
    }
    if (L->has_md) { memcpy(S->edits, sam + L->md, L->md_len); S->edits[L->md_len] = 0; }
    return (int)L->status;
}

/* =============================== multi-threaded text path ================================= */
/* The SAM body is cut into one chunk per thread at line boundaries.
 *   phase 1 (parallel)   RNAME changes inside each chunk (mapped records only)
 *   phase 1b (serial)    contig numbering across chunks, names table
 *   phase 2 (parallel)   split + tokenise every line into chunk-local record / SEQ / token pools
 *   phase 3 (serial)     block cutting over the 16-byte record summaries  } run
 *   phase 4 (parallel)   pools -> the final SEQ / token arrays             } concurrently
 * The result is identical, array for array, to the serial path.  A chunk whose first lines carry no
 * MD/XD field would need the previous chunk's (possibly rewritten) MD text: that case, which real
 * aligner output does not produce, returns MT_FALLBACK and the serial path runs instead. */
#define MT_FALLBACK   1000
#define MT_MAX_THREADS 64
#define MT_MIN_BYTES  (1u << 20)

typedef struct { uint32_t pos; uint16_t flag, rl; uint32_t nt_ev; uint32_t contig; } lrec_t;   /* nt | ev << 16 */
typedef struct { uint64_t ord; const char *name; uint32_t len, contig; } chg_t;

typedef struct chunk {
    packer_t *S;                       /* thread-local parse state; S->P is the shared result */
    const char *sam; size_t beg, end;
    /* phase 1 */
    uint64_t n_lines, n_mapped, seq_pred;
    chg_t *chg; uint64_t n_chg, cap_chg;
    const char *first_name, *last_name; uint32_t first_len, last_len;
    /* phase 1b */
    uint32_t contig0;                  /* contig of the chunk's first mapped record */
    /* phase 2 */
    lrec_t *lr; uint64_t n_lr;
    uint8_t *seq; uint64_t n_seq;      /* written in place: P->seq + seq_dst, seq_pred bytes */
    uint32_t *tok; uint64_t n_tok, cap_tok;
    uint64_t n_unmapped;
    int rc; char err[512];
    /* phase 4 */
    uint64_t seq_dst, tok_dst;
    int phase;
} chunk_t;

/* Phase 1 keeps a column scan of its own (memchr to the next tab, the first three columns and the 10th only) instead of
 * cbc_tok_split(), which reads every byte of the line: with the split here the phase took 0.289 s instead of 0.081 s and the
 * whole 16-thread pack of 4 M reads 0.953 s instead of 0.778 s, beyond the runs' spread of 0.14 s (profiles/packer_core.log).
 * It only has to find the RNAME changes and the SEQ bytes of well-formed mapped lines; phase 2, which runs the core on every
 * line, reports whatever is wrong with the others. */
static inline const char *next_field(const char *p, const char *e, const char **tok_end)
{   /* strtok("\t"): skip tabs, the token runs to the next tab or the line end */
    while (p < e && *p == '\t') p++;
    if (p >= e) return NULL;
    const char *q = (const char *)memchr(p, '\t', (size_t)(e - p));
    *tok_end = q ? q : e;
    return p;
}

static void chunk_phase1(chunk_t *c)
{
    const char *p = c->sam + c->beg, *end = c->sam + c->end;
    while (p < end) {
        const char *nl = (const char *)memchr(p, '\n', (size_t)(end - p));
        const char *e = nl ? nl + 1 : end;
        c->n_lines++;
        const char *t1e, *t2e, *t3e;
        const char *t1 = next_field(p, e, &t1e);
        const char *t2 = t1 ? next_field(t1e, e, &t2e) : NULL;
        const char *t3 = t2 ? next_field(t2e, e, &t3e) : NULL;
        if (t3 && t3e < e && *t3e == '\t') {
            char num[16]; size_t l = (size_t)(t2e - t2); if (l > 15) l = 15;
            memcpy(num, t2, l); num[l] = 0;
            uint32_t flag = (uint16_t)atoi(num);
            if ((flag & 4) != 4) {
                const char *q = t3e, *qe = t3e, *t10 = NULL;
                for (int k = 4; k <= 10 && q; k++) { t10 = next_field(qe, e, &qe); q = t10; }
                if (t10 && qe < e && *qe == '\t') c->seq_pred += (uint64_t)(qe - t10);   /* an 11th column follows */
                uint32_t len = (uint32_t)(t3e - t3);
                if (c->n_mapped == 0) { c->first_name = t3; c->first_len = len; }
                else if (len != c->last_len || memcmp(t3, c->last_name, len) != 0) {
                    if (grow((void **)&c->chg, &c->cap_chg, c->n_chg + 1, sizeof(chg_t))) { c->rc = CBC_E_NOMEM; return; }
                    c->chg[c->n_chg].ord = c->n_mapped; c->chg[c->n_chg].name = t3; c->chg[c->n_chg].len = len; c->chg[c->n_chg].contig = 0;
                    c->n_chg++;
                }
                c->last_name = t3; c->last_len = len;
                c->n_mapped++;
            }
        }
        p = e;
    }
}

static void chunk_phase2(chunk_t *c)
{
    packer_t *S = c->S; cbc_packed *P = S->P;
    const char *sam = c->sam;
    size_t off = c->beg;
    int have_md = 0;
    uint64_t ord = 0, k = 0; uint32_t contig = c->contig0;
    c->lr = (lrec_t *)malloc(sizeof(lrec_t) * (size_t)(c->n_mapped ? c->n_mapped : 1));
    if (!c->lr) { c->rc = CBC_E_NOMEM; return; }
    while (off < c->end) {
        cbc_tok_line L;
        const size_t e = line_end(sam, off, c->end);
        const int st = split_line(S, sam, off, e, &L);
        off = e;
        if (st < 0) { c->rc = st; return; }
        if (st == CBC_TOK_SKIP) continue;
        if (L.has_md) have_md = 1;
        else if (!have_md) { c->rc = MT_FALLBACK; return; }       /* would inherit MD text from before the chunk */
        if (st == CBC_TOK_UNMAPPED) { c->n_unmapped++; continue; }
        if (ord >= c->n_mapped) { c->rc = fail(S, CBC_E_INPUT, "internal: chunk record count changed%s%lld", "", 0); return; }
        if (k < c->n_chg && c->chg[k].ord == ord) contig = c->chg[k++].contig;
        const size_t rl = L.seq_len;
        uint32_t nt = 0, ev = 0;
        if (grow((void **)&c->tok, &c->cap_tok, c->n_tok + 4 * LINE_BUF, sizeof(uint32_t))) { c->rc = CBC_E_NOMEM; return; }
        int rc = tokenise_record(S, &P->contigs[contig], L.pos, sam + L.cigar, L.cigar_len, sam + L.seq, rl, c->tok + c->n_tok, &nt, &ev);
        if (rc) { c->rc = rc; return; }
        if (c->n_seq + rl > c->seq_pred) { c->rc = fail(S, CBC_E_INPUT, "internal: chunk SEQ bytes changed%s%lld", "", 0); return; }
        memcpy(c->seq + c->n_seq, sam + L.seq, rl);
        c->n_seq += rl; c->n_tok += nt;
        lrec_t *l = &c->lr[ord++];
        l->pos = (uint32_t)L.pos; l->flag = (uint16_t)L.flag; l->rl = (uint16_t)rl; l->nt_ev = nt | (ev << 16); l->contig = contig;
    }
    c->n_lr = ord;
}

static void chunk_phase4(chunk_t *c)
{
    cbc_packed *P = c->S->P;
    if (c->n_tok) memcpy(P->tok + c->tok_dst, c->tok, sizeof(uint32_t) * (size_t)c->n_tok);
    free(c->tok); c->tok = NULL;
}

static void *chunk_run(void *arg)
{
    chunk_t *c = (chunk_t *)arg;
    if (c->phase == 1) chunk_phase1(c); else if (c->phase == 2) chunk_phase2(c); else chunk_phase4(c);
    return NULL;
}

static int run_phase(chunk_t *ch, pthread_t *th, int n, int phase, int wait)
{
    int started = 0;
    for (int t = 0; t < n; t++) {
        ch[t].phase = phase;
        if (pthread_create(&th[t], NULL, chunk_run, &ch[t]) != 0) break;
        started++;
    }
    for (int t = started; t < n; t++) chunk_run(&ch[t]);           /* could not spawn: do it here */
    if (wait) for (int t = 0; t < started; t++) pthread_join(th[t], NULL);
    return started;
}

static double mt_now(void) { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; }

static int pack_body_mt(packer_t *S, const char *sam, size_t off, size_t sam_len, int nthreads)
{
    cbc_packed *P = S->P;
    chunk_t *ch = (chunk_t *)calloc((size_t)nthreads, sizeof(chunk_t));
    pthread_t *th = (pthread_t *)calloc((size_t)nthreads, sizeof(pthread_t));
    packer_t *ps = (packer_t *)calloc((size_t)nthreads, sizeof(packer_t));
    int rc = 0, committed = 0;
    if (!ch || !th || !ps) { rc = CBC_E_NOMEM; goto out; }
    {   /* chunk boundaries at line starts */
        size_t body = sam_len - off, b = off;
        for (int t = 0; t < nthreads; t++) {
            size_t e = (t == nthreads - 1) ? sam_len : off + body / (size_t)nthreads * (size_t)(t + 1);
            if (e < b) e = b;
            if (e < sam_len && t != nthreads - 1) {
                const char *nl = (const char *)memchr(sam + e, '\n', sam_len - e);
                e = nl ? (size_t)(nl - sam) + 1 : sam_len;
            }
            ch[t].sam = sam; ch[t].beg = b; ch[t].end = e; b = e;
            ps[t].P = P; ps[t].o = S->o; ps[t].err = ch[t].err; ps[t].errlen = sizeof ch[t].err; ps[t].n_fasta = S->n_fasta;
            ch[t].S = &ps[t];
        }
    }
    double T0 = mt_now();
    run_phase(ch, th, nthreads, 1, 1);
    double T1 = mt_now();
    for (int t = 0; t < nthreads; t++) if (ch[t].rc) { rc = ch[t].rc; goto out; }
    /* phase 1b: contig numbering in file order */
    {
        const char *prev = NULL; uint32_t prev_len = 0;
        uint32_t names0 = P->names_bytes;
        for (int t = 0; t < nthreads && !rc; t++) {
            chunk_t *c = &ch[t];
            if (c->n_mapped == 0) { c->contig0 = S->contig; continue; }
            if (!S->have_contig || c->first_len != prev_len || memcmp(c->first_name, prev, prev_len) != 0)
                rc = contig_open(S, c->first_name, c->first_len);
            c->contig0 = S->contig;
            for (uint64_t k = 0; k < c->n_chg && !rc; k++) {
                rc = contig_open(S, c->chg[k].name, c->chg[k].len);
                c->chg[k].contig = S->contig;
            }
            prev = c->last_name; prev_len = c->last_len;
        }
        if (rc) goto out;           /* contig errors are input errors, not fallbacks */
        (void)names0;
    }
    {   /* SEQ bytes go straight to their final place: phase 1 measured them */
        uint64_t nseq = P->seq_bytes;
        for (int t = 0; t < nthreads; t++) { ch[t].seq_dst = nseq; nseq += ch[t].seq_pred; }
        if (grow((void **)&P->seq, &P->cap_seq, nseq + 8, 1)) { rc = CBC_E_NOMEM; goto out; }
        for (int t = 0; t < nthreads; t++) ch[t].seq = P->seq + ch[t].seq_dst;
    }
    double T2 = mt_now();
    run_phase(ch, th, nthreads, 2, 1);
    double T3 = mt_now();
    for (int t = 0; t < nthreads; t++) if (ch[t].rc == MT_FALLBACK) { rc = MT_FALLBACK; goto out; }
    for (int t = 0; t < nthreads; t++) if (ch[t].rc) {
        rc = ch[t].rc;
        if (S->err && S->errlen) snprintf(S->err, S->errlen, "%s", ch[t].err);
        goto out;
    }
    /* sizes -> final arrays */
    {
        uint64_t nrec = 0, nseq = 0, ntok = 0;
        for (int t = 0; t < nthreads; t++) {
            if (ch[t].n_seq != ch[t].seq_pred) { rc = fail(S, CBC_E_INPUT, "internal: chunk SEQ bytes changed%s%lld", "", 0); goto out; }
            ch[t].tok_dst = ntok; nrec += ch[t].n_lr; nseq += ch[t].n_seq; ntok += ch[t].n_tok; P->n_skipped_unmapped += ch[t].n_unmapped;
        }
        if (grow((void **)&P->recs, &P->cap_recs, nrec + 1, sizeof(cbc_read_rec)) ||
            grow((void **)&P->tok, &P->cap_tok, ntok + 1, sizeof(uint32_t))) { rc = CBC_E_NOMEM; goto out; }
    }
    committed = 1;
    double T3b = mt_now();
    {
        int started = run_phase(ch, th, nthreads, 4, 0);
        /* phase 3 on this thread while the pools are copied */
        S->have_contig = 0;                              /* replay the contig sequence for block cutting */
        uint32_t cur = 0;
        for (int t = 0; t < nthreads && !rc; t++) {
            const lrec_t *lr = ch[t].lr;
            for (uint64_t i = 0; i < ch[t].n_lr; i++) {
                const lrec_t *l = &lr[i];
                if (!S->have_contig || l->contig != cur) { close_block(S); cur = l->contig; S->contig = cur; S->have_contig = 1; }
                rc = place_record(S, l->pos, l->flag, l->rl, l->nt_ev >> 16, l->nt_ev & 0xffffu);
                if (rc) break;
            }
        }
        double T4 = mt_now();
        for (int t = 0; t < started; t++) pthread_join(th[t], NULL);
        if (getenv("CBC_PACK_TIMES")) fprintf(stderr, "pack_mt: scan %.3f  contigs %.3f  tokenise %.3f  alloc %.3f  place %.3f  copy-wait %.3f s\n", T1 - T0, T2 - T1, T3 - T2, T3b - T3, T4 - T3b, mt_now() - T4);
    }
out:
    if (ch) for (int t = 0; t < nthreads; t++) { free(ch[t].chg); free(ch[t].lr); free(ch[t].tok); }
    free(ch); free(th); free(ps);
    if (rc == MT_FALLBACK && !committed) {
        /* undo phase 1b so that the serial path starts clean */
        P->names_bytes = 0; P->n_contigs = 0; S->have_contig = 0; S->contig = 0; P->n_skipped_unmapped = 0;
    }
    return rc;
}

API int cbc_pack_sam(const char *sam, size_t sam_len, const char *fasta, size_t fasta_len,
                     const cbc_pack_opts *opts, cbc_packed **out, char *errbuf, size_t errlen)
{
    if (!sam || !fasta || !out) return CBC_E_ARG;
    packer_t *S = (packer_t *)malloc(sizeof(packer_t));
    if (!S) return CBC_E_NOMEM;
    int rc = packer_init(S, opts, errbuf, errlen);
    if (rc) goto done;
    rc = load_reference(S, fasta, fasta_len, S->o.n_threads);
    if (rc) goto done;
    size_t off = 0;
    S->P->read_length = header_read_length(sam, sam_len, &off, (int)S->o.var_length);
    if (S->o.long_reads) {
        if (S->P->read_length < 1) S->P->read_length = 1;       /* not part of the long-read stream */
        if (S->P->read_length > 256) S->P->read_length = 256;
        rc = pack_body_long(S, sam, off, sam_len);
        if (!rc) rc = finish_pack(S);
        goto done;
    }
    if (S->P->read_length < 1 || S->P->read_length > 256) {
        rc = fail(S, CBC_E_INPUT, "header read length %s%lld outside 1..256 (the reference's limit is 252 bases per read; longer reads need the long-read format: cbc --long / long_reads)", "", S->P->read_length); goto done;
    }
    if (S->o.n_threads != 1) {
        int nt = (int)S->o.n_threads;
        if (nt == 0) {                                  /* auto: one per online CPU, serial for small inputs */
            long nc = sysconf(_SC_NPROCESSORS_ONLN);
            nt = nc < 1 ? 1 : nc > MT_MAX_THREADS ? MT_MAX_THREADS : (int)nc;
            if (sam_len - off < MT_MIN_BYTES) nt = 1;
        }
        if (nt > MT_MAX_THREADS) nt = MT_MAX_THREADS;
        if (nt > 1) {
            rc = pack_body_mt(S, sam, off, sam_len, nt);
            if (rc != MT_FALLBACK) { if (!rc) rc = finish_pack(S); goto done; }
            rc = 0;                                     /* nothing was committed: run the serial path */
        }
    }
    while (off < sam_len) {
        cbc_tok_line L;
        const size_t e = line_end(sam, off, sam_len);
        const int st = split_line(S, sam, off, e, &L);
        off = e;
        if (st < 0) { rc = st; goto done; }
        if (st == CBC_TOK_UNMAPPED) S->P->n_skipped_unmapped++;             /* compression.c:50-52 */
        if (st != CBC_TOK_OK) continue;
        rc = add_record(S, sam + L.rname, L.rname_len, L.flag, L.pos, sam + L.cigar, L.cigar_len, sam + L.seq, L.seq_len);
        if (rc) goto done;
    }
    rc = finish_pack(S);
done:
    packer_release(S);
    if (rc) { cbc_packed_free(S->P); *out = NULL; } else *out = S->P;
    free(S);
    return rc;
}

/* ================================= synthetic workload ===================================== */
typedef struct { uint64_t s[4]; } rng_t;
static uint64_t splitmix64(uint64_t *x) { uint64_t z = (*x += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
static inline uint64_t rotl(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
static inline uint64_t rng_next(rng_t *r)          /* xoshiro256** */
{
    uint64_t *s = r->s, res = rotl(s[1] * 5, 7) * 9, t = s[1] << 17;
    s[2] ^= s[0]; s[3] ^= s[1]; s[1] ^= s[2]; s[0] ^= s[3]; s[2] ^= t; s[3] = rotl(s[3], 45);
    return res;
}
static inline double rng_unit(rng_t *r) { return (double)(rng_next(r) >> 11) * (1.0 / 9007199254740992.0); }
static inline uint64_t rng_below(rng_t *r, uint64_t n) { return (uint64_t)(rng_unit(r) * (double)n); }
static int cmp_u32(const void *a, const void *b) { uint32_t x = *(const uint32_t *)a, y = *(const uint32_t *)b; return x < y ? -1 : x > y; }

API int cbc_synth_packed(const cbc_synth_opts *so, const cbc_pack_opts *po, cbc_packed **out,
                         char **sam_out, size_t *sam_len, char **fasta_out, size_t *fasta_len,
                         char *errbuf, size_t errlen)
{
    if (!so || !out || so->read_len < 30 || so->read_len > CBC_MAX_READ_LEN || so->contig_len < (uint64_t)so->read_len + 64 ||
        so->contig_len > 0xf0000000ull) return CBC_E_ARG;
    static const char ACGT[4] = { 'A', 'C', 'G', 'T' };
    const char *name = so->name ? so->name : "chr1";
    const uint32_t L = so->read_len;
    packer_t *S = (packer_t *)malloc(sizeof(packer_t));
    if (!S) return CBC_E_NOMEM;
    uint32_t *starts = NULL; char *sam = NULL; size_t samcap = 0, samn = 0;
    int rc = packer_init(S, po, errbuf, errlen);
    if (rc) goto done;
    cbc_packed *P = S->P;
    rng_t R; uint64_t sd = so->seed;
    for (int i = 0; i < 4; i++) R.s[i] = splitmix64(&sd);
    /* contig */
    if (grow((void **)&P->ref, &P->cap_ref, so->contig_len + CBC_REF_PAD, 1)) { rc = CBC_E_NOMEM; goto done; }
    for (uint64_t i = 0; i < so->contig_len; i += 32) {
        uint64_t w = rng_next(&R);
        for (int k = 0; k < 32 && i + k < so->contig_len; k++) { P->ref[i + k] = (uint8_t)ACGT[w & 3]; w >>= 2; }
    }
    memset(P->ref + so->contig_len, 0, CBC_REF_PAD);
    P->ref_bytes = so->contig_len + CBC_REF_PAD;
    if (grow32((void **)&P->contigs, &P->cap_contigs, 1, sizeof(cbc_contig_info))) { rc = CBC_E_NOMEM; goto done; }
    P->contigs[0].ref_off = 0; P->contigs[0].length = so->contig_len; P->contigs[0].name_off = 0; P->contigs[0].reserved = 0;
    S->n_fasta = 1;
    P->read_length = L;
    /* sorted start positions */
    starts = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)(so->n_reads ? so->n_reads : 1));
    if (!starts) { rc = CBC_E_NOMEM; goto done; }
    uint64_t span = so->contig_len - L - 8;
    for (uint64_t i = 0; i < so->n_reads; i++) starts[i] = (uint32_t)rng_below(&R, span);
    qsort(starts, (size_t)so->n_reads, sizeof(uint32_t), cmp_u32);
    char seq[LINE_BUF], cigar[64], qual[LINE_BUF];
    char *const md = S->edits;                          /* where add_record() expects the record's MD text */
    memset(qual, 'I', L); qual[L] = 0;
    for (uint64_t i = 0; i < so->n_reads; i++) {
        const uint8_t *ref = P->ref + starts[i];
        uint32_t flag = (rng_next(&R) & 1) ? 16u : 0u;
        int has_indel = rng_unit(&R) < so->indel_frac;
        uint32_t o = 0, k = 0; int is_ins = 0;
        if (has_indel) { k = 1 + (uint32_t)rng_below(&R, 3); o = 10 + (uint32_t)rng_below(&R, L - 20 - k); is_ins = (int)(rng_next(&R) & 1); }
        /* assemble read and the per-base reference it aligns to (0 = inserted base) */
        uint8_t rb[LINE_BUF]; uint32_t q = 0, rp = 0, nm = 0;
        if (!has_indel) { memcpy(seq, ref, L); memcpy(rb, ref, L); }
        else if (is_ins) {
            for (q = 0; q < o; q++) { seq[q] = (char)ref[rp]; rb[q] = ref[rp++]; }
            for (uint32_t c = 0; c < k; c++, q++) { seq[q] = ACGT[rng_next(&R) & 3]; rb[q] = 0; }
            for (; q < L; q++) { seq[q] = (char)ref[rp]; rb[q] = ref[rp++]; }
        } else {
            for (q = 0; q < o; q++) { seq[q] = (char)ref[rp]; rb[q] = ref[rp++]; }
            rp += k;
            for (; q < L; q++) { seq[q] = (char)ref[rp]; rb[q] = ref[rp++]; }
        }
        seq[L] = 0;
        /* substitutions on aligned bases */
        int nsub = 0;
        if (so->sub_rate > 0) {
            for (uint32_t b = 0; b < L; b++) {
                if (rb[b] && rng_unit(&R) < so->sub_rate) {
                    char old = seq[b]; char alt;
                    do { alt = ACGT[rng_next(&R) & 3]; } while (alt == old);
                    seq[b] = alt; nsub++;
                }
            }
        }
        /* CIGAR + MD */
        if (!has_indel) snprintf(cigar, sizeof cigar, "%uM", L);
        else if (is_ins) snprintf(cigar, sizeof cigar, "%uM%uI%uM", o, k, L - o - k);
        else snprintf(cigar, sizeof cigar, "%uM%uD%uM", o, k, L - o);
        {
            char *m = md; uint32_t run = 0;
            for (uint32_t b = 0; b < L; b++) {
                if (has_indel && !is_ins && b == o) {
                    m += sprintf(m, "%u^", run); run = 0;
                    for (uint32_t c = 0; c < k; c++) *m++ = (char)ref[o + c];
                    nm += k;
                }
                if (!rb[b]) { nm++; continue; }
                if ((uint8_t)seq[b] == rb[b]) run++;
                else { m += sprintf(m, "%u%c", run, (char)rb[b]); run = 0; nm++; }
            }
            m += sprintf(m, "%u", run);
            *m = 0;
        }
        rc = add_record(S, name, strlen(name), flag, (int32_t)starts[i] + 1, cigar, strlen(cigar), seq, L);
        if (rc) goto done;
        if (sam_out) {
            if (samn + 2 * LINE_BUF > samcap) {
                size_t nc = samcap ? samcap * 2 : (1u << 20);
                char *ns = (char *)realloc(sam, nc); if (!ns) { rc = CBC_E_NOMEM; goto done; }
                sam = ns; samcap = nc;
            }
            samn += (size_t)sprintf(sam + samn, "r%llu\t%u\t%s\t%u\t60\t%s\t*\t0\t0\t%s\t%s\tMD:Z:%s\tNM:i:%u\n",
                                    (unsigned long long)i, flag, name, starts[i] + 1, cigar, seq, qual, md, nm);
        }
    }
    rc = finish_pack(S);
    if (rc) goto done;
    if (sam_out) {
        if (!sam) { sam = (char *)malloc(1); if (!sam) { rc = CBC_E_NOMEM; goto done; } }
        *sam_out = sam; *sam_len = samn; sam = NULL;
    }
    if (fasta_out) {
        uint64_t nlines = (so->contig_len + 59) / 60;
        size_t cap = (size_t)(so->contig_len + nlines + strlen(name) + 8);
        char *fa = (char *)malloc(cap); if (!fa) { rc = CBC_E_NOMEM; goto done; }
        size_t n = (size_t)sprintf(fa, ">%s\n", name);
        for (uint64_t i = 0; i < so->contig_len; i += 60) {
            uint64_t c = so->contig_len - i < 60 ? so->contig_len - i : 60;
            memcpy(fa + n, P->ref + i, (size_t)c); n += (size_t)c; fa[n++] = '\n';
        }
        *fasta_out = fa; *fasta_len = n;
    }
done:
    free(starts); free(sam);
    packer_release(S);
    if (rc) { cbc_packed_free(S->P); *out = NULL; } else *out = S->P;
    free(S);
    return rc;
}


/* ================================= cfg5: synthetic long reads ============================== */
typedef struct {
    const cbc_synth_opts *so; const uint8_t *ref; const uint32_t *starts;
    uint64_t r0, r1;                       /* reads [r0, r1) */
    uint8_t *seq;                          /* final array: read r at r * read_len */
    uint32_t *tok; uint64_t n_tok, cap_tok; uint32_t *tok_of; uint16_t *flags;
    char *sam; size_t samn, samcap; int want_sam; const char *name;
    int rc;
} long_job;

static void *long_gen(void *arg)
{
    long_job *J = (long_job *)arg;
    static const char ACGT[4] = { 'A', 'C', 'G', 'T' };
    const uint32_t L = J->so->read_len;
    char *cig = (char *)malloc(16 * (size_t)L + 64);
    if (!cig) { J->rc = CBC_E_NOMEM; return NULL; }
    for (uint64_t r = J->r0; r < J->r1 && !J->rc; r++) {
        rng_t R; uint64_t sd = J->so->seed ^ (0x9e3779b97f4a7c15ull * (r + 1));
        for (int i = 0; i < 4; i++) R.s[i] = splitmix64(&sd);
        const uint8_t *ref = J->ref + J->starts[r];
        uint8_t *out = J->seq + r * (uint64_t)L;
        if (grow((void **)&J->tok, &J->cap_tok, J->n_tok + 2 + 2 * (uint64_t)L + 8, sizeof(uint32_t))) { J->rc = CBC_E_NOMEM; break; }
        uint32_t *t = J->tok + J->n_tok; uint32_t nt = 2, n_cig = 0;
        J->tok_of[r - J->r0] = (uint32_t)J->n_tok;          /* relative to the job's pool; rebased when placed */
        J->flags[r - J->r0] = (rng_next(&R) & 1) ? 16 : 0;
        uint32_t i = 0, j = 0, run = 0;
#define EMIT(op_, n_) do { if ((n_)) { if (n_cig && (t[nt - 1] & 15u) == (op_)) t[nt - 1] += (uint32_t)(n_) << 4; else { t[nt++] = ((uint32_t)(n_) << 4) | (op_); n_cig++; } } } while (0)
        while (i < L) {
            double u = rng_unit(&R);
            if (u >= J->so->sub_rate || i == 0 || i + 1 >= L) { out[i++] = ref[j++]; run++; continue; }
            uint32_t kind = (uint32_t)(rng_next(&R) % 3);
            if (kind == 0) { char alt; do { alt = ACGT[rng_next(&R) & 3]; } while ((uint8_t)alt == ref[j]); out[i++] = (uint8_t)alt; j++; run++; }
            else if (kind == 1) { EMIT(CBC_OP_M, run); run = 0; out[i++] = (uint8_t)ACGT[rng_next(&R) & 3]; EMIT(CBC_OP_I, 1u); }
            else { EMIT(CBC_OP_M, run); run = 0; j++; EMIT(CBC_OP_D, 1u); }
        }
        EMIT(CBC_OP_M, run);
#undef EMIT
        t[0] = n_cig; t[1] = 0;
        J->n_tok += nt;
        if (J->want_sam) {
            size_t cl = 0;
            for (uint32_t k = 0; k < n_cig; k++) cl += (size_t)sprintf(cig + cl, "%u%c", t[2 + k] >> 4, "MIDS"[t[2 + k] & 15u]);
            size_t need = J->samn + 2 * (size_t)L + cl + 256;
            if (need > J->samcap) { size_t nc = J->samcap ? J->samcap * 2 : (1u << 20); while (nc < need) nc *= 2;
                                    char *ns = (char *)realloc(J->sam, nc); if (!ns) { J->rc = CBC_E_NOMEM; break; } J->sam = ns; J->samcap = nc; }
            J->samn += (size_t)sprintf(J->sam + J->samn, "r%llu\t%u\t%s\t%u\t60\t%s\t*\t0\t0\t", (unsigned long long)r, J->flags[r - J->r0], J->name, J->starts[r] + 1, cig);
            memcpy(J->sam + J->samn, out, L); J->samn += L; J->sam[J->samn++] = '\t';
            memset(J->sam + J->samn, 'I', L); J->samn += L; J->sam[J->samn++] = '\n';
        }
    }
    free(cig);
    return NULL;
}

API int cbc_synth_long(const cbc_synth_opts *so, const cbc_pack_opts *po, cbc_packed **out,
                       char **sam_out, size_t *sam_len, char **fasta_out, size_t *fasta_len, char *errbuf, size_t errlen)
{
    if (!so || !out || so->read_len < 64 || so->read_len > CBC_LONG_MAX_READ_LEN || so->contig_len < 2ull * so->read_len + 64 ||
        so->contig_len > 0xf0000000ull || so->sub_rate < 0 || so->sub_rate > 0.5) return CBC_E_ARG;
    static const char ACGT[4] = { 'A', 'C', 'G', 'T' };
    const char *name = so->name ? so->name : "chrL";
    const uint32_t L = so->read_len;
    cbc_pack_opts o; if (po) o = *po; else cbc_pack_default_opts(&o);
    o.long_reads = 1;
    packer_t *S = (packer_t *)malloc(sizeof(packer_t));
    if (!S) return CBC_E_NOMEM;
    uint32_t *starts = NULL; long_job *jobs = NULL; pthread_t *th = NULL;
    int nt = o.n_threads ? (int)o.n_threads : online_cpus();
    if (nt > 64) nt = 64;
    if ((uint64_t)nt > so->n_reads) nt = so->n_reads ? (int)so->n_reads : 1;
    int rc = packer_init(S, &o, errbuf, errlen);
    if (rc) goto done;
    cbc_packed *P = S->P;
    rng_t R; uint64_t sd = so->seed;
    for (int i = 0; i < 4; i++) R.s[i] = splitmix64(&sd);
    if (grow((void **)&P->ref, &P->cap_ref, so->contig_len + CBC_REF_PAD, 1)) { rc = CBC_E_NOMEM; goto done; }
    for (uint64_t i = 0; i < so->contig_len; i += 32) {
        uint64_t w = rng_next(&R);
        for (int k = 0; k < 32 && i + k < so->contig_len; k++) { P->ref[i + k] = (uint8_t)ACGT[w & 3]; w >>= 2; }
    }
    memset(P->ref + so->contig_len, 0, CBC_REF_PAD);
    P->ref_bytes = so->contig_len + CBC_REF_PAD;
    if (grow32((void **)&P->contigs, &P->cap_contigs, 1, sizeof(cbc_contig_info))) { rc = CBC_E_NOMEM; goto done; }
    P->contigs[0].ref_off = 0; P->contigs[0].length = so->contig_len; P->contigs[0].name_off = 0; P->contigs[0].reserved = 0;
    S->n_fasta = 1; P->read_length = L > 256 ? 256 : L;
    starts = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)(so->n_reads ? so->n_reads : 1));
    jobs = (long_job *)calloc((size_t)nt, sizeof(long_job)); th = (pthread_t *)calloc((size_t)nt, sizeof(pthread_t));
    if (!starts || !jobs || !th) { rc = CBC_E_NOMEM; goto done; }
    {   /* every read may consume up to 2 L reference bases (deletions) */
        uint64_t span = so->contig_len - 2ull * L - 8;
        for (uint64_t i = 0; i < so->n_reads; i++) starts[i] = (uint32_t)rng_below(&R, span);
        qsort(starts, (size_t)so->n_reads, sizeof(uint32_t), cmp_u32);
    }
    if (grow((void **)&P->seq, &P->cap_seq, so->n_reads * (uint64_t)L + 8, 1)) { rc = CBC_E_NOMEM; goto done; }
    for (int t = 0; t < nt; t++) {
        long_job *J = &jobs[t];
        J->so = so; J->ref = P->ref; J->starts = starts; J->seq = P->seq; J->name = name; J->want_sam = sam_out != NULL;
        J->r0 = so->n_reads * (uint64_t)t / (uint64_t)nt; J->r1 = so->n_reads * (uint64_t)(t + 1) / (uint64_t)nt;
        J->tok_of = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)(J->r1 - J->r0 + 1));
        J->flags = (uint16_t *)malloc(sizeof(uint16_t) * (size_t)(J->r1 - J->r0 + 1));
        if (!J->tok_of || !J->flags) { rc = CBC_E_NOMEM; goto done; }
    }
    {
        int started = 0;
        for (int t = 0; t < nt; t++) { if (pthread_create(&th[t], NULL, long_gen, &jobs[t]) != 0) break; started++; }
        for (int t = started; t < nt; t++) long_gen(&jobs[t]);
        for (int t = 0; t < started; t++) pthread_join(th[t], NULL);
    }
    for (int t = 0; t < nt; t++) if (jobs[t].rc) { rc = jobs[t].rc; goto done; }
    {   /* block cutting over the reads in order; the SEQ bytes are already in place, the tokens are copied per read */
        rc = contig_open(S, name, strlen(name));
        if (rc) goto done;
        uint64_t ntok = 0;
        for (int t = 0; t < nt; t++) ntok += jobs[t].n_tok;
        if (grow((void **)&P->tok, &P->cap_tok, ntok + 1, sizeof(uint32_t))) { rc = CBC_E_NOMEM; goto done; }
        for (int t = 0; t < nt && !rc; t++) {
            long_job *J = &jobs[t];
            for (uint64_t r = J->r0; r < J->r1; r++) {
                const uint32_t *tk = J->tok + J->tok_of[r - J->r0];
                uint32_t n = 2 + (tk[0] & 0xffffu);
                uint64_t to = P->n_tok;
                rc = place_record(S, starts[r] + 1, J->flags[r - J->r0], L, 0, n);
                if (rc) break;
                memcpy(P->tok + to, tk, sizeof(uint32_t) * n);
            }
        }
        if (rc) goto done;
    }
    rc = finish_pack(S);
    if (rc) goto done;
    if (sam_out) {
        size_t total = 0;
        for (int t = 0; t < nt; t++) total += jobs[t].samn;
        char *sam = (char *)malloc(total + 1);
        if (!sam) { rc = CBC_E_NOMEM; goto done; }
        size_t n = 0;
        for (int t = 0; t < nt; t++) { memcpy(sam + n, jobs[t].sam, jobs[t].samn); n += jobs[t].samn; }
        *sam_out = sam; *sam_len = n;
    }
    if (fasta_out) {
        uint64_t nlines = (so->contig_len + 59) / 60;
        size_t cap = (size_t)(so->contig_len + nlines + strlen(name) + 8);
        char *fa = (char *)malloc(cap); if (!fa) { rc = CBC_E_NOMEM; goto done; }
        size_t n = (size_t)sprintf(fa, ">%s\n", name);
        for (uint64_t i = 0; i < so->contig_len; i += 60) {
            uint64_t c = so->contig_len - i < 60 ? so->contig_len - i : 60;
            memcpy(fa + n, P->ref + i, (size_t)c); n += (size_t)c; fa[n++] = '\n';
        }
        *fasta_out = fa; *fasta_len = n;
    }
done:
    if (jobs) for (int t = 0; t < nt; t++) { free(jobs[t].tok); free(jobs[t].tok_of); free(jobs[t].flags); free(jobs[t].sam); }
    free(jobs); free(th); free(starts);
    packer_release(S);
    if (rc) { cbc_packed_free(S->P); *out = NULL; } else *out = S->P;
    free(S);
    return rc;
}

/* ================================= block container ======================================== */
/* layout (little-endian), version 2:
 *   u32 magic "CBCB", u32 version, u32 read_length, u32 n_contigs, u32 n_blocks, u32 names_bytes,
 *   u32 cap_pos, u32 cap_var, u32 max_read_len                                   (36 bytes)
 *   names blob, padded to 4
 *   n_contigs x { u32 name_off, u32 reserved, u64 length }
 *   n_blocks  x { u32 contig, u32 n_reads, u64 window_start, u64 payload_off, u32 payload_bytes, u32 reserved }
 *   payloads, concatenated in block order
 */
#define CBC_CONTAINER_HDR 36ull
static uint64_t container_header_bytes(const cbc_packed *p)
{
    return CBC_CONTAINER_HDR + ((p->names_bytes + 3u) & ~3u) + 16ull * p->n_contigs + 32ull * p->n_blocks;
}
API int64_t cbc_container_size(const cbc_packed *p, const uint64_t *out_offsets)
{
    if (!p || !out_offsets) return CBC_E_ARG;
    return (int64_t)(container_header_bytes(p) + out_offsets[p->n_blocks]);
}
static void w32(uint8_t **d, uint32_t v) { memcpy(*d, &v, 4); *d += 4; }
static void w64(uint8_t **d, uint64_t v) { memcpy(*d, &v, 8); *d += 8; }
API int64_t cbc_container_write(const cbc_packed *p, const uint8_t *payloads, const uint64_t *out_offsets,
                                uint8_t *dst, uint64_t dst_cap)
{
    if (!p || !payloads || !out_offsets || !dst) return CBC_E_ARG;
    uint64_t hb = container_header_bytes(p), total = hb + out_offsets[p->n_blocks];
    if (dst_cap < total) return CBC_E_ARG;
    uint8_t *d = dst;
    w32(&d, CBC_CONTAINER_MAGIC); w32(&d, p->whole_file == 2 ? CBC_CONTAINER_VERSION_LONG : CBC_CONTAINER_VERSION); w32(&d, p->read_length);
    w32(&d, p->n_contigs); w32(&d, p->n_blocks); w32(&d, p->names_bytes);
    w32(&d, p->caps.cap_pos); w32(&d, p->caps.cap_var); w32(&d, p->max_read_len);
    uint32_t nb = (p->names_bytes + 3u) & ~3u;
    memset(d, 0, nb); memcpy(d, p->names, p->names_bytes); d += nb;
    for (uint32_t i = 0; i < p->n_contigs; i++) { w32(&d, p->contigs[i].name_off); w32(&d, 0); w64(&d, p->contigs[i].length); }
    for (uint32_t b = 0; b < p->n_blocks; b++) {
        w32(&d, p->info[b].contig); w32(&d, p->info[b].n_reads); w64(&d, p->info[b].window_start);
        w64(&d, out_offsets[b]); w32(&d, (uint32_t)(out_offsets[b + 1] - out_offsets[b]));
        w32(&d, p->whole_file == 2 ? (uint32_t)p->info[b].n_bases : 0u);     /* version 3: the decoder writes the bases compactly */
    }
    memcpy(d, payloads, (size_t)out_offsets[p->n_blocks]);
    return (int64_t)total;
}



/* ================================= after the device tokeniser ============ */
API uint64_t cbc_sam_body_offset(const char *sam, size_t len)
{
    size_t off = 0;
    if (!sam) return 0;
    (void)header_read_length(sam, len, &off, 0);
    return off;
}

typedef cbc_tok_record_summary dev_summary;             /* the one public struct (include/cbc_gpu.h) */
_Static_assert(sizeof(cbc_tok_record_summary) == 16, "record summary crosses the device/host seam as 16 bytes");

API int cbc_pack_from_device_tokens(const char *sam, size_t sam_len, const char *fasta, size_t fasta_len, const cbc_pack_opts *opts,
                                    const void *summaries, const uint8_t *rname_change, const uint64_t *change_name_off,
                                    const uint32_t *change_name_len, uint64_t n_recs, uint64_t n_unmapped,
                                    uint8_t *seq, uint64_t seq_bytes, uint32_t *tok, uint64_t n_tok,
                                    cbc_packed **out, char *errbuf, size_t errlen)
{
    if (!sam || !fasta || !out || (n_recs && (!summaries || !rname_change || !change_name_off || !change_name_len))) return CBC_E_ARG;
    packer_t *S = (packer_t *)malloc(sizeof(packer_t));
    if (!S) return CBC_E_NOMEM;
    int rc = packer_init(S, opts, errbuf, errlen);
    if (rc) goto done;
    if (S->o.whole_file || S->o.long_reads) { rc = fail(S, CBC_E_ARG, "the device tokeniser feeds block mode only%s%lld", "", 0); goto done; }
    rc = load_reference(S, fasta, fasta_len, S->o.n_threads);
    if (rc) goto done;
    cbc_packed *P = S->P;
    {
        size_t off = 0;
        P->read_length = header_read_length(sam, sam_len, &off, (int)S->o.var_length);
        if (P->read_length < 1 || P->read_length > 256) { rc = fail(S, CBC_E_INPUT, "header read length %s%lld outside 1..256", "", P->read_length); goto done; }
    }
    if (grow((void **)&P->recs, &P->cap_recs, n_recs + 1, sizeof(cbc_read_rec))) { rc = CBC_E_NOMEM; goto done; }
    {
        const dev_summary *sm = (const dev_summary *)summaries;
        uint64_t k = 0;
        for (uint64_t r = 0; r < n_recs && !rc; r++) {
            if (rname_change[r]) {
                if (change_name_off[k] + change_name_len[k] > sam_len) { rc = fail(S, CBC_E_ARG, "contig name outside the text%s%lld", "", 0); break; }
                rc = contig_open(S, sam + change_name_off[k], change_name_len[k]); k++;
                if (rc) break;
            }
            const cbc_contig_info *ctg = &P->contigs[S->contig];
            const uint32_t nt = sm[r].nt_ev & 0xffffu, ev = sm[r].nt_ev >> 16;
            if ((uint64_t)sm[r].pos - 1 + sm[r].rl > ctg->length + CBC_REF_PAD - 8) {
                rc = fail(S, CBC_E_INPUT, "record at %s POS %lld runs past the contig end + pad", (const char *)P->names + ctg->name_off, sm[r].pos); break; }
            if (ev + 1 > S->o.max_cap_var) { rc = fail(S, CBC_E_INPUT, "record at %s:%lld has more edits than max_cap_var", (const char *)P->names + ctg->name_off, sm[r].pos); break; }
            rc = place_record(S, sm[r].pos, sm[r].flag, sm[r].rl, ev, nt);
        }
        if (rc) goto done;
    }
    if (P->seq_bytes != seq_bytes || P->n_tok != n_tok) { rc = fail(S, CBC_E_ARG, "summaries and array sizes disagree%s%lld", "", 0); goto done; }
    P->n_skipped_unmapped = n_unmapped;
    close_block(S);
    if (seq) { free(P->seq); P->seq = seq; P->cap_seq = seq_bytes + 8; memset(P->seq + seq_bytes, 0, 8); }
    if (tok) { free(P->tok); P->tok = tok; P->cap_tok = n_tok; }
    P->seq_bytes += 8;                                  /* the 8 readable pad bytes (the device array has them too) */
    if (P->caps.cap_pos < 64) P->caps.cap_pos = 64;
    if (P->caps.cap_var < 64) P->caps.cap_var = 64;
    P->caps.cap_pos = (P->caps.cap_pos + 63u) & ~63u;
    P->caps.cap_var = (P->caps.cap_var + 63u) & ~63u;
    if (P->n_tok == 0 && !P->tok) { if (grow((void **)&P->tok, &P->cap_tok, 1, sizeof(uint32_t))) { rc = CBC_E_NOMEM; goto done; } P->tok[0] = 0; }
    P->whole_file = 0;
done:
    packer_release(S);
    if (rc) { if (seq && S->P && S->P->seq == seq) S->P->seq = NULL; if (tok && S->P && S->P->tok == tok) S->P->tok = NULL; cbc_packed_free(S->P); *out = NULL; }
    else *out = S->P;
    free(S);
    return rc;
}

/* ================================= 2-bit transport ======================= */
typedef struct { const uint8_t *b; uint32_t *codes; uint64_t i0, i1; cbc_2bit_run *runs; uint64_t n_runs, cap_runs; int rc; } twobit_job;

static inline uint32_t base_code(uint8_t c) { return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u; }

static void *twobit_run(void *arg)
{
    twobit_job *J = (twobit_job *)arg;                     /* [i0, i1) is a multiple of 16 bases except at the very end */
    const uint8_t *b = J->b;
    for (uint64_t i = J->i0; i < J->i1; i += 16) {
        uint32_t w = 0;
        const uint64_t e = i + 16 < J->i1 ? i + 16 : J->i1;
        for (uint64_t k = i; k < e; k++) {
            uint32_t c = base_code(b[k]);
            if (c < 4u) w |= c << (2u * (uint32_t)(k & 15u));
            else {                                          /* an exception: extend the current run or open one */
                cbc_2bit_run *last = J->n_runs ? &J->runs[J->n_runs - 1] : NULL;
                if (last && last->start + last->length == k && last->byte == b[k] && last->length < 0xffffffffu) last->length++;
                else {
                    if (grow((void **)&J->runs, &J->cap_runs, J->n_runs + 1, sizeof(cbc_2bit_run))) { J->rc = CBC_E_NOMEM; return NULL; }
                    J->runs[J->n_runs].start = k; J->runs[J->n_runs].length = 1; J->runs[J->n_runs].byte = b[k]; J->n_runs++;
                }
            }
        }
        J->codes[i >> 4] = w;
    }
    return NULL;
}

API void cbc_2bit_free(cbc_2bit *p) { if (p) { free(p->codes); free(p->runs); free(p); } }

API int cbc_2bit_pack(const uint8_t *bases, uint64_t n, uint32_t n_threads, cbc_2bit **out)
{
    if (!bases || !out) return CBC_E_ARG;
    *out = NULL;
    int nt = n_threads ? (int)n_threads : online_cpus();
    if (nt > 64) nt = 64;
    if (n < ((uint64_t)1 << 22)) nt = 1;
    cbc_2bit *P = (cbc_2bit *)calloc(1, sizeof(cbc_2bit));
    twobit_job *jobs = (twobit_job *)calloc((size_t)nt, sizeof(twobit_job));
    pthread_t *th = (pthread_t *)calloc((size_t)nt, sizeof(pthread_t));
    int rc = 0;
    if (!P || !jobs || !th) { rc = CBC_E_NOMEM; goto done; }
    P->n_bases = n;
    P->codes = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)((n + 15) / 16 + 1));
    if (!P->codes) { rc = CBC_E_NOMEM; goto done; }
    {
        const uint64_t words = (n + 15) / 16;
        int started = 0;
        for (int t = 0; t < nt; t++) {
            jobs[t].b = bases; jobs[t].codes = P->codes;
            jobs[t].i0 = words * (uint64_t)t / (uint64_t)nt * 16; jobs[t].i1 = (t == nt - 1) ? n : words * (uint64_t)(t + 1) / (uint64_t)nt * 16;
            if (jobs[t].i1 > n) jobs[t].i1 = n;
        }
        for (int t = 0; t < nt; t++) { if (pthread_create(&th[t], NULL, twobit_run, &jobs[t]) != 0) break; started++; }
        for (int t = started; t < nt; t++) twobit_run(&jobs[t]);
        for (int t = 0; t < started; t++) pthread_join(th[t], NULL);
    }
    {   /* concatenate the threads' runs, merging a run that continues across a boundary */
        uint64_t total = 0;
        for (int t = 0; t < nt; t++) { if (jobs[t].rc) rc = jobs[t].rc; total += jobs[t].n_runs; }
        if (rc) goto done;
        P->runs = (cbc_2bit_run *)malloc(sizeof(cbc_2bit_run) * (size_t)(total ? total : 1));
        if (!P->runs) { rc = CBC_E_NOMEM; goto done; }
        for (int t = 0; t < nt; t++)
            for (uint64_t k = 0; k < jobs[t].n_runs; k++) {
                cbc_2bit_run *r = &jobs[t].runs[k], *last = P->n_runs ? &P->runs[P->n_runs - 1] : NULL;
                if (last && last->start + last->length == r->start && last->byte == r->byte && (uint64_t)last->length + r->length <= 0xffffffffull) last->length += r->length;
                else P->runs[P->n_runs++] = *r;
            }
    }
    *out = P; P = NULL;
done:
    if (jobs) for (int t = 0; t < nt; t++) free(jobs[t].runs);
    free(jobs); free(th); cbc_2bit_free(P);
    return rc;
}

API int cbc_2bit_unpack(const cbc_2bit *p, uint8_t *bases)
{
    if (!p || !bases || (p->n_bases && !p->codes) || (p->n_runs && !p->runs)) return CBC_E_ARG;
    static const char ACGT[4] = { 'A', 'C', 'G', 'T' };
    for (uint64_t i = 0; i < p->n_bases; i++) bases[i] = (uint8_t)ACGT[(p->codes[i >> 4] >> (2u * (uint32_t)(i & 15u))) & 3u];
    for (uint64_t k = 0; k < p->n_runs; k++) {
        /* no `start + length`: that sum wraps in u64 for a crafted run (round-2 advisor finding) */
        if (p->runs[k].start > p->n_bases || p->runs[k].length > p->n_bases - p->runs[k].start) return CBC_E_INPUT;
        memset(bases + p->runs[k].start, (int)p->runs[k].byte, p->runs[k].length);
    }
    return 0;
}

/* ================================= sharding =============================================== */
API uint64_t cbc_checksum64(const uint8_t *bytes, uint64_t n)
{
    uint64_t acc = 0;
    if (!bytes) return 0;
    for (uint64_t i = 0; i < n; i++) acc += CBC_CHECKSUM_TERM(i, bytes[i]);
    return acc;
}

API int cbc_assign_contigs(const cbc_packed *p, uint32_t n_parts, uint32_t *part_of_contig)
{
    if (!p || !part_of_contig || n_parts == 0) return CBC_E_ARG;
    uint32_t nc = p->n_contigs;
    uint64_t *reads = (uint64_t *)calloc(nc ? nc : 1, sizeof(uint64_t)), *load = (uint64_t *)calloc(n_parts, sizeof(uint64_t));
    uint8_t *done = (uint8_t *)calloc(nc ? nc : 1, 1);
    if (!reads || !load || !done) { free(reads); free(load); free(done); return CBC_E_NOMEM; }
    for (uint32_t b = 0; b < p->n_blocks; b++) reads[p->info[b].contig] += p->info[b].n_reads;
    for (uint32_t k = 0; k < nc; k++) {                     /* largest remaining contig -> least loaded part */
        uint32_t best = 0; int have = 0;
        for (uint32_t c = 0; c < nc; c++) if (!done[c] && (!have || reads[c] > reads[best])) { best = c; have = 1; }
        uint32_t part = 0;
        for (uint32_t q = 1; q < n_parts; q++) if (load[q] < load[part]) part = q;
        part_of_contig[best] = part; load[part] += reads[best]; done[best] = 1;
    }
    free(reads); free(load); free(done);
    return 0;
}

/* ================================= reference alone ======================================== */
API void cbc_reference_free(cbc_reference *r)
{
    if (!r) return;
    free(r->bases); free(r->contig_off); free(r->contig_len); free(r);
}
API int cbc_reference_load(const char *fasta, size_t fasta_len, uint32_t n_threads, cbc_reference **out, char *errbuf, size_t errlen)
{
    if (!fasta || !out) return CBC_E_ARG;
    *out = NULL;
    packer_t *S = (packer_t *)calloc(1, sizeof(packer_t));
    cbc_reference *r = (cbc_reference *)calloc(1, sizeof(cbc_reference));
    if (!S || !r) { free(S); free(r); return CBC_E_NOMEM; }
    S->err = errbuf; S->errlen = errlen;
    if (errbuf && errlen) errbuf[0] = 0;
    int rc = CBC_E_NOMEM;
    S->P = (cbc_packed *)calloc(1, sizeof(cbc_packed));
    if (S->P) rc = load_reference(S, fasta, fasta_len, n_threads);
    if (!rc && S->n_fasta == 0) rc = fail(S, CBC_E_INPUT, "the FASTA holds no sequence%s%lld", "", 0);
    if (!rc) {
        r->contig_off = (uint64_t *)calloc(S->n_fasta, sizeof(uint64_t));
        r->contig_len = (uint64_t *)calloc(S->n_fasta, sizeof(uint64_t));
        if (!r->contig_off || !r->contig_len) rc = CBC_E_NOMEM;
    }
    if (!rc) {
        for (uint32_t i = 0; i < S->n_fasta; i++) { r->contig_off[i] = S->P->contigs[i].ref_off; r->contig_len[i] = S->P->contigs[i].length; }
        r->n_contigs = S->n_fasta; r->bases = S->P->ref; r->n_bytes = S->P->ref_bytes; S->P->ref = NULL;
        *out = r;
    } else cbc_reference_free(r);
    if (S->P) cbc_packed_free(S->P);
    free(S);
    return rc;
}

/* ================================= unpack side ============================================ */
static uint32_t r32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }
static uint64_t r64(const uint8_t *p) { uint64_t v; memcpy(&v, p, 8); return v; }

API void cbc_unpack_plan_free(cbc_unpack_plan *u)
{
    if (!u) return;
    free(u->blocks); free(u->window_start); free(u->ref);
    free(u->block_contig); free(u->names); free(u->contig_name_off); free(u->contig_len); free(u);
}

/* Parse a container, load the FASTA the way the packer does (contigs in file order, upper-cased,
 * padded) and lay out the decode launch: one cbc_dec_block_desc per block. */
API int cbc_unpack_plan_create(const uint8_t *blob, uint64_t len, const char *fasta, size_t fasta_len,
                               cbc_unpack_plan **out, char *errbuf, size_t errlen)
{
    if (!blob || !fasta || !out) return CBC_E_ARG;
    *out = NULL;
    packer_t *S = (packer_t *)calloc(1, sizeof(packer_t));
    cbc_unpack_plan *u = (cbc_unpack_plan *)calloc(1, sizeof(cbc_unpack_plan));
    if (!S || !u) { free(S); free(u); return CBC_E_NOMEM; }
    S->err = errbuf; S->errlen = errlen;
    if (errbuf && errlen) errbuf[0] = 0;
    int rc = 0;
    S->P = (cbc_packed *)calloc(1, sizeof(cbc_packed));
    if (!S->P) { rc = CBC_E_NOMEM; goto fail; }
    if (len < CBC_CONTAINER_HDR || r32(blob) != CBC_CONTAINER_MAGIC) { rc = fail(S, CBC_E_INPUT, "not a cbc block container%s%lld", "", 0); goto fail; }
    const int is_long = r32(blob + 4) == CBC_CONTAINER_VERSION_LONG;
    if (r32(blob + 4) != CBC_CONTAINER_VERSION && !is_long) { rc = fail(S, CBC_E_INPUT, "unsupported container version %s%lld", "", r32(blob + 4)); goto fail; }
    {
        uint32_t L0 = r32(blob + 8), nc = r32(blob + 12), nb = r32(blob + 16), nbytes = r32(blob + 20);
        uint32_t cap_pos = r32(blob + 24), cap_var = r32(blob + 28), max_rl = r32(blob + 32);
        uint64_t names_pad = ((uint64_t)nbytes + 3u) & ~3ull;
        uint64_t hdr = CBC_CONTAINER_HDR + names_pad + 16ull * nc + 32ull * nb;
        if (hdr > len || L0 < 1 || (L0 > 256 && !is_long) || max_rl < 1 || max_rl > (is_long ? CBC_LONG_MAX_READ_LEN : CBC_MAX_READ_LEN) || cap_pos < 2 || cap_pos > 8192 ||
            cap_var < 1 || cap_var > 32768) { rc = fail(S, CBC_E_INPUT, "corrupt container header%s%lld", "", 0); goto fail; }
        const uint8_t *ctab = blob + CBC_CONTAINER_HDR + names_pad, *btab = ctab + 16ull * nc, *pay = btab + 32ull * nb;
        uint64_t pay_bytes = len - hdr;
        rc = load_reference(S, fasta, fasta_len, 0u);
        if (rc) goto fail;
        if (S->n_fasta < nc) { rc = fail(S, CBC_E_INPUT, "the FASTA has fewer records than the container has contigs%s%lld", "", 0); goto fail; }
        for (uint32_t i = 0; i < nc; i++)
            if (r64(ctab + 16ull * i + 8) != S->P->contigs[i].length) {
                rc = fail(S, CBC_E_INPUT, "contig %s#%lld has a different length in the FASTA than at compression time", "", (long long)i + 1); goto fail; }
        u->blocks = (cbc_dec_block_desc *)calloc(nb ? nb : 1, sizeof(cbc_dec_block_desc));
        u->window_start = (uint64_t *)calloc(nb ? nb : 1, sizeof(uint64_t));
        u->block_contig = (uint32_t *)calloc(nb ? nb : 1, sizeof(uint32_t));
        u->names = (char *)calloc((size_t)nbytes + 1, 1);
        u->contig_name_off = (uint32_t *)calloc(nc ? nc : 1, sizeof(uint32_t));
        u->contig_len = (uint64_t *)calloc(nc ? nc : 1, sizeof(uint64_t));
        if (!u->blocks || !u->window_start || !u->block_contig || !u->names || !u->contig_name_off || !u->contig_len) { rc = CBC_E_NOMEM; goto fail; }
        memcpy(u->names, blob + CBC_CONTAINER_HDR, nbytes);   /* the header check above keeps the blob inside `len` */
        u->names_bytes = nbytes; u->n_contigs = nc;
        for (uint32_t i = 0; i < nc; i++) { u->contig_name_off[i] = r32(ctab + 16ull * i); u->contig_len[i] = r64(ctab + 16ull * i + 8); }
        uint32_t stride = is_long ? 0u : ((max_rl + 3u) & ~3u);
        uint64_t nrec = 0, nbases = 0;
        for (uint32_t b = 0; b < nb; b++) {
            const uint8_t *e = btab + 32ull * b;
            uint32_t contig = r32(e), nreads = r32(e + 4), pbytes = r32(e + 24), blk_bases = r32(e + 28);
            uint64_t w0 = r64(e + 8), poff = r64(e + 16);
            /* no sums of file-supplied values: poff + pbytes could wrap */
            if (contig >= nc || poff > pay_bytes || pbytes > pay_bytes - poff || w0 >= S->P->contigs[contig].length + 1 ||
                nreads > CBC_MAX_BLOCK_READS || (is_long && (uint64_t)blk_bases > (uint64_t)nreads * CBC_LONG_MAX_READ_LEN)) {
                rc = fail(S, CBC_E_INPUT, "corrupt block index entry %s%lld", "", b); goto fail; }
            cbc_dec_block_desc *d = &u->blocks[b];
            d->in_off = poff; d->in_bytes = pbytes; d->ref_off = S->P->contigs[contig].ref_off + w0;
            d->rec_base = nrec; d->seq_base = is_long ? nbases : nrec * stride; d->n_reads = nreads; d->read_length = L0; d->seq_stride = stride;
            d->reserved[0] = is_long ? blk_bases : 0u;
            u->window_start[b] = w0; u->block_contig[b] = contig;
            nrec += nreads; nbases += ((uint64_t)blk_bases + 7u) & ~7ull;
        }
        u->n_blocks = nb; u->payloads = pay; u->payload_bytes = pay_bytes; u->caps.cap_pos = cap_pos; u->caps.cap_var = cap_var;
        u->read_length = L0; u->seq_stride = stride; u->n_recs = nrec;
        u->long_reads = is_long ? 1u : 0u; u->max_read_len = max_rl; u->seq_total = is_long ? nbases + 8 : nrec * stride + 8;
        u->ref = S->P->ref; u->ref_bytes = S->P->ref_bytes; S->P->ref = NULL;
    }
    cbc_packed_free(S->P); free(S);
    *out = u;
    return 0;
fail:
    if (S->P) cbc_packed_free(S->P);
    free(S); cbc_unpack_plan_free(u);
    return rc;
}

/* ---- region decode: parse NAME[:BEG[-END]] and select the blocks (include/cbc_host.h) ---- */
static int region_err(char *errbuf, size_t errlen, const char *fmt, const char *a, int alen)
{
    if (errbuf && errlen) snprintf(errbuf, errlen, fmt, alen, a);
    return CBC_E_INPUT;
}

/* the contig whose name is exactly s[0 .. n), -1 if none; -2: a name offset outside the blob or a name without its NUL */
static int64_t region_contig(const cbc_unpack_plan *u, const char *s, size_t n)
{
    for (uint32_t c = 0; c < u->n_contigs; c++) {
        const uint32_t off = u->contig_name_off[c];
        if (off >= u->names_bytes) return -2;
        const char *nm = u->names + off;
        const size_t len = strnlen(nm, u->names_bytes - off);
        if (len == u->names_bytes - off) return -2;
        if (len == n && memcmp(nm, s, n) == 0) return c;
    }
    return -1;
}

/* a decimal number of 1..18 digits filling s[0 .. n) */
static int region_number(const char *s, size_t n, uint64_t *v)
{
    if (n < 1 || n > 18) return -1;
    uint64_t x = 0;
    for (size_t i = 0; i < n; i++) { if (s[i] < '0' || s[i] > '9') return -1; x = x * 10u + (uint64_t)(s[i] - '0'); }
    *v = x;
    return 0;
}

/* the block index, checked in one bounded pass: contigs in file order, positions in order within a contig (the packer
 * writes nothing else); then contig c's run of blocks [c0, c1) (0, 0: it has none).  -1: the index is out of order */
static int region_contig_run(const cbc_unpack_plan *u, uint32_t c, uint32_t *r0, uint32_t *r1)
{
    uint32_t c0 = u->n_blocks, c1 = u->n_blocks;
    for (uint32_t b = 0; b < u->n_blocks; b++) {
        const uint32_t cb = u->block_contig[b];
        if (b > 0 && (cb < u->block_contig[b - 1] || (cb == u->block_contig[b - 1] && u->window_start[b] < u->window_start[b - 1])))
            return -1;
        if (cb == c && c0 == u->n_blocks) c0 = b;
        if (cb == c) c1 = b + 1;
    }
    if (c0 == u->n_blocks) c0 = c1 = 0;
    *r0 = c0; *r1 = c1;
    return 0;
}

/* Span bound.  In block mode the decoder takes nDel as one symbol of the L0-symbol indel-count alphabet (indel_counts,
 * cbc_decode_body.h) and nIns >= 0, so span = rl + nDel - nIns <= max_read_len + L0 - 1 for every read it reconstructs.
 * The packer itself accepts any nDel up to 0xffff (tokenise_record, cbc_pack.c), but the encoder codes nDel & 0xff as that
 * symbol and fails the block with CBC_ST_ASSERT when it is >= L0 (dense_code, cbc_encode_body.h): a container holds no
 * record whose decoded nDel reaches L0, and the decoder refuses a read longer than the row (rl <= seq_stride).  The span
 * decode checks the bound on every read (CBC_ST_SPAN), so a crafted payload cannot slip a read past the selection. */
static uint32_t region_smax(const cbc_unpack_plan *u) { return u->max_read_len + u->read_length - 1u; }

/* the selection rule of include/cbc_host.h over the contig's run [c0, c1): the blocks [b0, b1) that can hold a read
 * overlapping [beg, end] */
static void region_pick(const cbc_unpack_plan *u, uint32_t c0, uint32_t c1, uint64_t beg, uint64_t end, uint32_t smax,
                        uint32_t *p0, uint32_t *p1)
{
    uint32_t b1 = c0, b0 = c0;
    while (b1 < c1 && u->window_start[b1] + 1u <= end) b1++;                   /* F(b) <= END */
    while (b0 + 1 < c1 && u->window_start[b0 + 1] + 1u + smax < beg + 1u) b0++;  /* F(next(b)) >= BEG - SMAX + 1 */
    if (b0 > b1) b0 = b1;
    *p0 = b0; *p1 = b1;
}

API int cbc_unpack_region(const cbc_unpack_plan *u, const char *region, cbc_region_sel *sel, char *errbuf, size_t errlen)
{
    if (!u || !region || !sel) return CBC_E_ARG;
    if (errbuf && errlen) errbuf[0] = 0;
    memset(sel, 0, sizeof *sel);
    if (u->long_reads)
        return region_err(errbuf, errlen, "region decode of a long-read (version 3) container is not supported: its deletions have no small "
                          "bound, so the index cannot tell which blocks hold a locus%.*s", "", 0);
    if (!u->block_contig || !u->names || !u->contig_name_off || !u->contig_len) return CBC_E_ARG;
    const size_t n = strlen(region);
    const int ilen = n > 200 ? 200 : (int)n;
    uint64_t beg = 1, end = UINT64_MAX;
    int64_t c = region_contig(u, region, n);
    if (c == -1) {                                       /* not a name as a whole: NAME:BEG or NAME:BEG-END */
        const char *colon = strrchr(region, ':');
        if (!colon) return region_err(errbuf, errlen, "unknown contig in region \"%.*s\"", region, ilen);
        c = region_contig(u, region, (size_t)(colon - region));
        if (c == -1) return region_err(errbuf, errlen, "unknown contig in region \"%.*s\"", region, ilen);
        if (c >= 0) {
            const char *num = colon + 1, *dash = strchr(num, '-');
            const size_t nlen = dash ? (size_t)(dash - num) : strlen(num);
            if (region_number(num, nlen, &beg) || (dash && region_number(dash + 1, strlen(dash + 1), &end)))
                return region_err(errbuf, errlen, "malformed coordinates in region \"%.*s\" (want NAME, NAME:BEG or NAME:BEG-END)", region, ilen);
            if (beg < 1) return region_err(errbuf, errlen, "region \"%.*s\" begins before base 1", region, ilen);
            if (beg > end) return region_err(errbuf, errlen, "region \"%.*s\" ends before it begins", region, ilen);
        }
    }
    if (c == -2) return region_err(errbuf, errlen, "corrupt container: a contig name lies outside the name table%.*s", "", 0);
    const uint64_t clen = u->contig_len[c];
    if (end > clen) end = clen;
    if (beg > end) return region_err(errbuf, errlen, "region \"%.*s\" begins past the end of its contig", region, ilen);
    uint32_t c0, c1, b0, b1;
    if (region_contig_run(u, (uint32_t)c, &c0, &c1))
        return region_err(errbuf, errlen, "corrupt container: the block index is not in contig and position order%.*s", "", 0);
    const uint32_t smax = region_smax(u);
    region_pick(u, c0, c1, beg, end, smax, &b0, &b1);
    sel->contig = (uint32_t)c; sel->b0 = b0; sel->b1 = b1; sel->smax = smax;
    sel->beg = beg; sel->end = end; sel->contig_len = clen;
    return 0;
}

/* ---- SAM output (include/cbc_host.h): the header, and the size of the records' text ---- */
/* length of contig c's name, checked as region_contig checks it; -1: offset outside the table or no NUL */
static int64_t sam_name_len(const cbc_unpack_plan *u, uint32_t c)
{
    const uint32_t off = u->contig_name_off[c];
    if (off >= u->names_bytes) return -1;
    const size_t len = strnlen(u->names + off, u->names_bytes - off);
    return len == u->names_bytes - off ? -1 : (int64_t)len;
}

API int64_t cbc_unpack_sam_header(const cbc_unpack_plan *u, char *dst, uint64_t cap, char *errbuf, size_t errlen)
{
    if (!u) return CBC_E_ARG;
    if (errbuf && errlen) errbuf[0] = 0;
    if (u->long_reads)
        return region_err(errbuf, errlen, "SAM output of a long-read (version 3) container is not supported%.*s", "", 0);
    if (!u->names || !u->contig_name_off || !u->contig_len) return CBC_E_ARG;
    static const char hd[] = "@HD\tVN:1.6\tSO:coordinate\n";
    uint64_t n = sizeof hd - 1;
    if (dst) { if (n > cap) return CBC_E_ARG; memcpy(dst, hd, (size_t)n); }
    for (uint32_t c = 0; c < u->n_contigs; c++) {
        const int64_t nl = sam_name_len(u, c);
        if (nl < 0) return region_err(errbuf, errlen, "corrupt container: a contig name lies outside the name table%.*s", "", 0);
        const char *nm = u->names + u->contig_name_off[c];
        if (nl < 1 || nl > (int64_t)CBC_SAM_MAX_NAME)
            return region_err(errbuf, errlen, "SAM output: contig name \"%.*s\" is empty or longer than 255 bytes", nm, nl > 60 ? 60 : (int)nl);
        if (memchr(nm, '\t', (size_t)nl) || memchr(nm, '\n', (size_t)nl))
            return region_err(errbuf, errlen, "SAM output: contig name \"%.*s\" holds a tab or a newline", nm, nl > 60 ? 60 : (int)nl);
        if (u->contig_len[c] > CBC_SAM_MAX_POS)
            return region_err(errbuf, errlen, "SAM output: contig \"%.*s\" is longer than 2^31 - 1 bases, the largest POS of SAM", nm, nl > 60 ? 60 : (int)nl);
        char ln[64];
        const int k = snprintf(ln, sizeof ln, "\tLN:%llu\n", (unsigned long long)u->contig_len[c]);
        if (dst) {
            if (7u + (uint64_t)nl + (uint64_t)k > cap - n) return CBC_E_ARG;
            memcpy(dst + n, "@SQ\tSN:", 7); memcpy(dst + n + 7, nm, (size_t)nl); memcpy(dst + n + 7 + nl, ln, (size_t)k);
        }
        n += 7u + (uint64_t)nl + (uint64_t)k;
    }
    return (int64_t)n;
}

/* bytes that always hold the alignment lines of blocks [b0, b1): every read kept, FLAG 5 and POS 10 digits, SEQ a full row */
API uint64_t cbc_unpack_sam_text_cap(const cbc_unpack_plan *u, uint32_t b0, uint32_t b1)
{
    if (!u || u->long_reads || !u->block_contig || !u->names || !u->contig_name_off || b0 > b1 || b1 > u->n_blocks) return 0;
    uint64_t n = 0;
    for (uint32_t b = b0; b < b1; b++) {
        const uint32_t c = u->block_contig[b];
        const int64_t nl = c < u->n_contigs ? sam_name_len(u, c) : -1;
        if (nl < 0) return 0;
        n += (uint64_t)u->blocks[b].n_reads * (35ull + (uint64_t)nl + u->seq_stride);
    }
    return n;
}

/* Bytes that always hold the lines of blocks [b0, b1) with CIGAR, NM and MD (cbc_gpu_decode_sam_cigar).  Per block of n reads
 * on a contig whose name has nl bytes, with the arena of n * edits_per_read entries its reads with indels share:
 *   every read: the SAM line at its longest, 35 + nl + seq_stride (cbc_unpack_sam_text_cap), whose '*' the CIGAR replaces;
 *     rl <= seq_stride <= 256 and the counts are <= 255, so every number of CIGAR and MD has at most 3 digits and NM
 *     (<= rl + nDel) has 3; "\tNM:i:" and "\tMD:Z:" are 12 bytes: + 15;
 *     a read with e arena entries (deleted and inserted bases) has at most 1 + 2e runs of read indices and deleted runs (an
 *     inserted run adds itself and the aligned run behind it, a deleted run itself and the aligned run behind it), 4 bytes
 *     each: 4 - 1 + 8e for the CIGAR;
 *     MD: a mismatch's token is digits(n) + 1 <= 2 (n + 1) bytes for the n + 1 aligned bases it covers, so the aligned bases
 *     cost at most 2 seq_stride; a deleted run costs digits(n) + 1 + its bases <= 5 per deleted entry (the '0' of a mismatch
 *     behind it is that mismatch's); the last count 3;
 *   in all n * (35 + nl + seq_stride + 15 + 3 + 2 seq_stride + 3) + 13 * (entries in use) <= n * (56 + nl + 3 seq_stride +
 *   16 edits_per_read), the constant per entry rounded up.  A read whose entries are not the decoder's gets the plain line.
 * edits_per_read: 0 = CBC_EDITS_PER_READ.  0 for a plan cbc_unpack_sam_header refuses, a bad range or edits_per_read above
 * CBC_EDITS_MAX.  About three times cbc_unpack_sam_text_cap: callers try less first (include/cbc_gpu.h). */
API uint64_t cbc_unpack_sam_cigar_text_cap(const cbc_unpack_plan *u, uint32_t b0, uint32_t b1, uint32_t edits_per_read)
{
    if (!u || u->long_reads || !u->block_contig || !u->names || !u->contig_name_off || b0 > b1 || b1 > u->n_blocks) return 0;
    if (edits_per_read == 0) edits_per_read = CBC_EDITS_PER_READ;
    if (edits_per_read > CBC_EDITS_MAX) return 0;
    uint64_t n = 0;
    for (uint32_t b = b0; b < b1; b++) {
        const uint32_t c = u->block_contig[b];
        const int64_t nl = c < u->n_contigs ? sam_name_len(u, c) : -1;
        if (nl < 0) return 0;
        n += (uint64_t)u->blocks[b].n_reads * (56ull + (uint64_t)nl + 3ull * u->seq_stride + 16ull * edits_per_read);
    }
    return n;
}

/* ---- coverage output (include/cbc_host.h) ---- */
API int cbc_unpack_contig_blocks(const cbc_unpack_plan *u, uint32_t contig, cbc_region_sel *sel, char *errbuf, size_t errlen)
{
    if (!u || !sel || !u->names || !u->contig_name_off || contig >= u->n_contigs) return CBC_E_ARG;
    if (sam_name_len(u, contig) < 0)
        return region_err(errbuf, errlen, "corrupt container: a contig name lies outside the name table%.*s", "", 0);
    const int rc = cbc_unpack_region(u, u->names + u->contig_name_off[contig], sel, errbuf, errlen);   /* a whole name: the contig */
    if (rc) return rc;
    if (sel->contig != contig)
        return region_err(errbuf, errlen, "contig name \"%.*s\" occurs twice in the container", u->names + u->contig_name_off[contig], 60);
    return 0;
}

API uint64_t cbc_unpack_depth_text_cap(const cbc_unpack_plan *u, uint32_t b0, uint32_t b1, uint32_t contig)
{
    if (!u || u->long_reads || !u->names || !u->contig_name_off || b0 > b1 || b1 > u->n_blocks || contig >= u->n_contigs) return 0;
    const int64_t nl = sam_name_len(u, contig);
    if (nl < 0) return 0;
    uint64_t k = 0;
    for (uint32_t b = b0; b < b1; b++) k += u->blocks[b].n_reads;
    return k ? (2u * k - 1u) * ((uint64_t)nl + 34u) : 0u;
}

/* ---- per-position allele counts (include/cbc_host.h) ----
 * Proof of the bound.  A line stands for a position p of the window [beg, end] with nonref(p) >= 1, so lines <= end - beg + 1.
 * nonref(p) >= 1 needs a kept read with an aligned base of another class at p, a deleted base at p, or an insertion anchored
 * at p; all three lie inside that read's span [POS, POS + span - 1] (what falls outside is not counted), the decoder fails the
 * block of a read with span > smax (CBC_ST_SPAN), and a failed block contributes nothing: so lines <= reads * smax as well.
 * A line is the name, ten tabs, the reference byte, '\n' and nine numbers below 2^32 -- pos1 <= 2^31 - 1 has at most 10
 * digits, the eight counts at most 10 each --: name + 12 + 90 = name + 2 + 10 + 2 + 8 * 11 bytes. */
static uint64_t pileup_text_cap(const cbc_unpack_plan *u, uint32_t b0, uint32_t b1, uint32_t contig, uint64_t beg, uint64_t end,
                                uint32_t smax, uint32_t line)        /* line: the bytes of a line beside the name */
{
    if (!u || u->long_reads || !u->names || !u->contig_name_off || b0 > b1 || b1 > u->n_blocks || contig >= u->n_contigs || beg < 1 ||
        beg > end || end > 0x7fffffffull) return 0;
    const int64_t nl = sam_name_len(u, contig);
    if (nl < 0) return 0;
    uint64_t k = 0;
    for (uint32_t b = b0; b < b1; b++) k += u->blocks[b].n_reads;
    const uint64_t w = end - beg + 1u, by_reads = k * smax;          /* k < 2^32 blocks * 2^14 reads, smax < 2^32: no wrap */
    return (w < by_reads ? w : by_reads) * ((uint64_t)nl + line);
}

API uint64_t cbc_unpack_pileup_text_cap(const cbc_unpack_plan *u, uint32_t b0, uint32_t b1, uint32_t contig, uint64_t beg, uint64_t end,
                                        uint32_t smax)
{
    return pileup_text_cap(u, b0, b1, contig, beg, end, smax, 102u);
}

/* ---- per-strand counts and the fraction rule (include/cbc_host.h) ----
 * The proof above, extended.  The fraction rule only takes lines away, and which positions get a line is decided on the totals, so
 * the two bounds on the number of lines stand as they are.  With by_strand a line carries seven more columns, each a tab and a
 * number below 2^32 of at most 10 digits (X+ counts a subset of what X counts; the reference class's X+ is depth+ - del+ -
 * mismatches+, a 32-bit value whatever the tables hold): 7 * 11 bytes more, name + 179.  Lines < 2^31 and a line < 2^9: no wrap. */
API uint64_t cbc_unpack_pileup_ext_text_cap(const cbc_unpack_plan *u, uint32_t b0, uint32_t b1, uint32_t contig, uint64_t beg, uint64_t end,
                                            uint32_t smax, uint32_t by_strand)
{
    return by_strand > 1u ? 0u : pileup_text_cap(u, b0, b1, contig, beg, end, smax, by_strand ? 102u + 7u * 11u : 102u);
}

/* ---- consensus (include/cbc_host.h) ----
 * The record of a window holds its header, at most one byte per position (a called deletion drops its byte, or writes '*') and a
 * newline behind every line_width bytes and behind the last: header + w + ceil(w / line_width) with w = end - beg + 1, exact when
 * every position writes a byte.  w < 2^31, the header < 2^9: no wrap. */
static uint32_t cons_ndig(uint64_t x) { uint32_t d = 1; for (; x >= 10u; x /= 10u) d++; return d; }

API uint64_t cbc_unpack_consensus_text_cap(const cbc_unpack_plan *u, uint32_t contig, uint64_t beg, uint64_t end, uint32_t line_width,
                                           uint32_t with_range)
{
    if (!u || u->long_reads || !u->names || !u->contig_name_off || contig >= u->n_contigs || beg < 1 || beg > end || end > 0x7fffffffull ||
        line_width < 1 || line_width > 65535u || with_range > 1u) return 0;
    const int64_t nl = sam_name_len(u, contig);
    if (nl < 0) return 0;
    const uint64_t w = end - beg + 1u;
    return (uint64_t)nl + 2u + (with_range ? 2u + cons_ndig(beg) + cons_ndig(end) : 0u) + w + (w + line_width - 1u) / line_width;
}

/* The record of a window no read covers: every position is low depth (step 1 of the rule), so no device is asked.  The reference
 * byte of position p of contig c is ref[sum over the contigs in front of c of (length + CBC_REF_PAD) + p - 1], as load_reference
 * lays the FASTA out (cbc_unpack_plan_create holds table index == FASTA index).  A position past the contig's end is written as
 * 'N'; cbc_unpack_region and cbc_unpack_contig_blocks clamp a window to its contig, so neither path meets one through them (the
 * device call, given such a window directly, reads what the uploaded reference holds there: the zero pad, then the next contig). */
API int64_t cbc_unpack_consensus_empty(const cbc_unpack_plan *u, uint32_t contig, uint64_t beg, uint64_t end, const cbc_consensus_opts *o,
                                       uint32_t with_range, uint8_t *text, uint64_t text_cap, cbc_consensus_counts *counts)
{
    if (!u || !o || !counts || (text_cap && !text) || o->min_depth < 1 || o->call_ppm < 1 || o->call_ppm > 1000000u ||
        (o->flags & ~(CBC_CONS_SHOW_DEL | CBC_CONS_FILL_REF | CBC_CONS_IUPAC))) return CBC_E_ARG;
    const uint64_t need = cbc_unpack_consensus_text_cap(u, contig, beg, end, o->line_width, with_range);
    if (need == 0 || need > text_cap) return CBC_E_ARG;
    memset(counts, 0, sizeof *counts);
    const char *nm = u->names + u->contig_name_off[contig];
    uint64_t ref0 = 0;
    for (uint32_t c = 0; c < contig; c++) ref0 += u->contig_len[c] + CBC_REF_PAD;
    uint8_t *p = text;
    p += with_range ? sprintf((char *)p, ">%s:%llu-%llu\n", nm, (unsigned long long)beg, (unsigned long long)end) : sprintf((char *)p, ">%s\n", nm);
    const uint64_t w = end - beg + 1u;
    for (uint64_t i = 0; i < w; i++) {
        const uint64_t q = beg - 1u + i;
        uint8_t b = 'N';
        if (o->flags & CBC_CONS_FILL_REF) {
            b = q < u->contig_len[contig] && ref0 + q < u->ref_bytes ? u->ref[ref0 + q] : (uint8_t)'N';
            if ((b & 0xdfu) >= 'A' && (b & 0xdfu) <= 'Z') b |= 0x20u;
        }
        *p++ = b;
        if ((i + 1u) % o->line_width == 0u || i + 1u == w) *p++ = '\n';
    }
    counts->emitted = counts->low_depth = w;
    return (int64_t)(p - text);
}

/* ---- deletion-aware coverage (include/cbc_host.h) ----
 * Proof of the bound.  Under skip_deletions a read's deletion cuts its cover, so "K reads give at most 2K - 1 runs" no longer
 * holds.  A line stands for a maximal run of equal non-zero depth inside the window [beg, end]; runs are disjoint and each
 * holds at least one position of the window, so lines <= end - beg + 1.  A position of non-zero depth carries an aligned base
 * of a kept read; those lie inside the read's span [POS, POS + span - 1], the decoder fails the block of a read with
 * span > smax (CBC_ST_SPAN), and a failed block contributes nothing: so such positions, and with them the lines, are
 * <= reads * smax as well.  A line is the name, three tabs, '\n' and three numbers below 2^32 of at most 10 digits: name + 34
 * bytes, as for cbc_unpack_depth_text_cap. */
API uint64_t cbc_unpack_depth_skipdel_text_cap(const cbc_unpack_plan *u, uint32_t b0, uint32_t b1, uint32_t contig, uint64_t beg,
                                               uint64_t end, uint32_t smax)
{
    if (!u || u->long_reads || !u->names || !u->contig_name_off || b0 > b1 || b1 > u->n_blocks || contig >= u->n_contigs || beg < 1 ||
        beg > end || end > 0x7fffffffull) return 0;
    const int64_t nl = sam_name_len(u, contig);
    if (nl < 0) return 0;
    uint64_t k = 0;
    for (uint32_t b = b0; b < b1; b++) k += u->blocks[b].n_reads;
    const uint64_t w = end - beg + 1u, by_reads = k * smax;          /* k < 2^32 blocks * 2^14 reads, smax < 2^32: no wrap */
    return (w < by_reads ? w : by_reads) * ((uint64_t)nl + 34u);
}

/* ---- a set of regions (include/cbc_host.h) ---- */
typedef struct { uint32_t contig, beg, end; } target_raw;

static int target_cmp(const void *a, const void *b)
{
    const target_raw *x = (const target_raw *)a, *y = (const target_raw *)b;
    if (x->contig != y->contig) return x->contig < y->contig ? -1 : 1;
    if (x->beg != y->beg) return x->beg < y->beg ? -1 : 1;
    return x->end < y->end ? -1 : x->end > y->end;
}

static int target_push(target_raw **raw, uint64_t *n, uint64_t *cap, uint32_t contig, uint64_t beg, uint64_t end)
{
    if (*n == *cap) {
        const uint64_t nc = *cap ? *cap * 2u : 1024u;
        target_raw *p = (target_raw *)realloc(*raw, (size_t)nc * sizeof(target_raw));
        if (!p) return CBC_E_NOMEM;
        *raw = p; *cap = nc;
    }
    (*raw)[*n].contig = contig; (*raw)[*n].beg = (uint32_t)beg; (*raw)[*n].end = (uint32_t)end;   /* <= 2^31 - 1: checked */
    (*n)++;
    return 0;
}

/* the unmerged query list of cbc_unpack_queries; NULL where only the set is wanted */
typedef struct { cbc_query *q; uint64_t n, cap; } query_list;

/* a query of a known contig: [beg, end] 1-based inclusive, beg == end + 1 when it holds no position */
static int query_push(query_list *L, uint32_t contig, uint64_t beg, uint64_t end, size_t name_off, size_t name_len, uint64_t s0, uint64_t e0)
{
    if (!L) return 0;
    if (L->n == L->cap) {
        const uint64_t nc = L->cap ? L->cap * 2u : 1024u;
        cbc_query *p = (cbc_query *)realloc(L->q, (size_t)nc * sizeof(cbc_query));
        if (!p) return CBC_E_NOMEM;
        L->q = p; L->cap = nc;
    }
    cbc_query *x = &L->q[L->n++];
    memset(x, 0, sizeof *x);
    x->contig = contig; x->beg = (uint32_t)beg; x->end = (uint32_t)end;
    x->name_off = (uint32_t)name_off; x->name_len = (uint32_t)name_len;
    x->start0 = contig == CBC_QUERY_UNKNOWN ? s0 : beg - 1u; x->end0 = contig == CBC_QUERY_UNKNOWN ? e0 : end;
    return 0;
}

static int bed_err(char *errbuf, size_t errlen, uint64_t line, const char *what)
{
    if (errbuf && errlen) snprintf(errbuf, errlen, "BED line %llu: %s", (unsigned long long)line, what);
    return CBC_E_INPUT;
}

static inline int bed_sep(char c) { return c == ' ' || c == '\t'; }

/* the lines of a BED text into raw[]; every read stays inside bed[0 .. len) */
static int bed_parse(const cbc_unpack_plan *u, const char *bed, size_t len, target_raw **raw, uint64_t *n, uint64_t *cap,
                     uint64_t *unselected, query_list *ql, char *errbuf, size_t errlen)
{
    uint64_t line = 0;
    for (size_t at = 0; at < len; ) {
        const char *s = bed + at;
        const char *nl = (const char *)memchr(s, '\n', len - at);
        size_t ll = nl ? (size_t)(nl - s) : len - at;
        at += ll + (nl ? 1u : 0u);
        line++;
        if (ll > CBC_BED_MAX_LINE) return bed_err(errbuf, errlen, line, "longer than 65536 bytes");
        if (ll && s[ll - 1] == '\r') ll--;
        if (ll == 0 || s[0] == '#' || (ll >= 5 && !memcmp(s, "track", 5)) || (ll >= 7 && !memcmp(s, "browser", 7))) continue;
        size_t f0[3], fl[3], k = 0;
        int nf = 0;
        while (nf < 3) {
            while (k < ll && bed_sep(s[k])) k++;
            if (k == ll) break;
            f0[nf] = k;
            while (k < ll && !bed_sep(s[k])) k++;
            fl[nf] = k - f0[nf];
            nf++;
        }
        if (nf < 3) return bed_err(errbuf, errlen, line, "fewer than three columns (want chrom, start, end)");
        uint64_t st = 0, en = 0;
        if (region_number(s + f0[1], fl[1], &st) || region_number(s + f0[2], fl[2], &en))
            return bed_err(errbuf, errlen, line, "malformed or overflowing number");
        if (st > en) return bed_err(errbuf, errlen, line, "start is past end");
        const int64_t c = region_contig(u, s + f0[0], fl[0]);
        if (c == -2) return region_err(errbuf, errlen, "corrupt container: a contig name lies outside the name table%.*s", "", 0);
        if (c < 0 || st == en || st >= u->contig_len[c]) {
            (*unselected)++;
            /* still a query: the chrom text and the numbers as given, or both ends clamped to the contig (no position) */
            const uint64_t cl = c < 0 ? 0u : u->contig_len[c];
            const int qrc = c < 0 ? query_push(ql, CBC_QUERY_UNKNOWN, 1u, 0u, (size_t)(s + f0[0] - bed), fl[0], st, en)
                                  : query_push(ql, (uint32_t)c, (st < cl ? st : cl) + 1u, en < cl ? en : cl, 0, 0, 0, 0);
            if (qrc) return qrc;
            continue;
        }
        if (en > u->contig_len[c]) en = u->contig_len[c];
        int rc = target_push(raw, n, cap, (uint32_t)c, st + 1u, en);
        if (!rc) rc = query_push(ql, (uint32_t)c, st + 1u, en, 0, 0, 0, 0);
        if (rc) return rc;
    }
    return 0;
}

static int targets_build(const cbc_unpack_plan *u, cbc_targets *t, target_raw *raw, uint64_t n, char *errbuf, size_t errlen);

API void cbc_targets_free(cbc_targets *t)
{
    if (!t) return;
    free(t->iv); free(t->contig_first); free(t->contig_count); free(t->blocks); free(t->block_iv);
    free(t->contig_blk_first); free(t->contig_blk_count); free(t);
}

API int cbc_unpack_targets(const cbc_unpack_plan *u, const char *const *regions, uint32_t n_regions, const char *bed, size_t bed_len,
                           cbc_targets **out, char *errbuf, size_t errlen)
{
    if (!u || !out || (n_regions && !regions) || (bed_len && !bed)) return CBC_E_ARG;
    *out = NULL;
    if (errbuf && errlen) errbuf[0] = 0;
    /* long-read containers, names and lengths the text cannot carry; contigs <= 2^31 - 1 bases, so coordinates fit 32 bits */
    const int64_t hdr = cbc_unpack_sam_header(u, NULL, 0, errbuf, errlen);
    if (hdr < 0) return (int)hdr;
    if (!u->block_contig) return CBC_E_ARG;
    target_raw *raw = NULL;
    uint64_t n = 0, cap = 0;
    int rc = 0;
    cbc_targets *t = (cbc_targets *)calloc(1, sizeof *t);
    if (!t) return CBC_E_NOMEM;
    for (uint32_t r = 0; r < n_regions && !rc; r++) {
        cbc_region_sel sel;
        if (!regions[r]) { rc = CBC_E_ARG; break; }
        rc = cbc_unpack_region(u, regions[r], &sel, errbuf, errlen);
        if (!rc) rc = target_push(&raw, &n, &cap, sel.contig, sel.beg, sel.end);
    }
    if (!rc && bed) rc = bed_parse(u, bed, bed_len, &raw, &n, &cap, &t->bed_unselected, NULL, errbuf, errlen);
    if (!rc) rc = targets_build(u, t, raw, n, errbuf, errlen);
    if (rc) goto fail;
    free(raw);
    *out = t;
    return 0;
fail:
    free(raw);
    cbc_targets_free(t);
    return rc;
}

/* raw[0 .. n) (any order; sorted and merged in place) -> the intervals, the blocks and the per-block ranges of t */
static int targets_build(const cbc_unpack_plan *u, cbc_targets *t, target_raw *raw, uint64_t n, char *errbuf, size_t errlen)
{
    int rc = 0;
    t->n_input = n;
    t->n_contigs = u->n_contigs;
    t->smax = region_smax(u);
    if (n) qsort(raw, (size_t)n, sizeof *raw, target_cmp);
    /* merge in place: overlapping or adjacent intervals of a contig become one */
    uint64_t m = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (m && raw[m - 1].contig == raw[i].contig && (uint64_t)raw[m - 1].end + 1u >= raw[i].beg) {
            if (raw[i].end > raw[m - 1].end) raw[m - 1].end = raw[i].end;
        } else raw[m++] = raw[i];
    }
    if (m > CBC_TARGETS_MAX_IV)
        return region_err(errbuf, errlen, "the set of regions has more than 2^24 intervals after merging%.*s", "", 0);
    t->n_iv = (uint32_t)m;
    {
        const size_t nc = u->n_contigs ? u->n_contigs : 1u;
        t->iv = (cbc_target_iv *)calloc(m ? (size_t)m : 1u, sizeof(cbc_target_iv));
        t->contig_first = (uint32_t *)calloc(nc, 4); t->contig_count = (uint32_t *)calloc(nc, 4);
        t->contig_blk_first = (uint32_t *)calloc(nc, 4); t->contig_blk_count = (uint32_t *)calloc(nc, 4);
        t->blocks = (uint32_t *)calloc(u->n_blocks ? u->n_blocks : 1u, 4);
        t->block_iv = (uint32_t *)calloc(u->n_blocks ? u->n_blocks : 1u, 8);
        if (!t->iv || !t->contig_first || !t->contig_count || !t->contig_blk_first || !t->contig_blk_count || !t->blocks || !t->block_iv)
            return CBC_E_NOMEM;
    }
    for (uint64_t i = 0; i < m; i++) {
        t->iv[i].beg = raw[i].beg; t->iv[i].end = raw[i].end;
        if (t->contig_count[raw[i].contig]++ == 0) t->contig_first[raw[i].contig] = (uint32_t)i;
    }
    /* the blocks: per contig with intervals, the union of the runs the single-region rule picks (both ends of a run grow with
     * the interval, so the union is made by appending), and per block the intervals its reads can reach */
    for (uint32_t c = 0; c < u->n_contigs; c++) {
        if (!t->contig_count[c]) continue;
        uint32_t c0, c1;
        if (region_contig_run(u, c, &c0, &c1))
            return region_err(errbuf, errlen, "corrupt container: the block index is not in contig and position order%.*s", "", 0);
        const cbc_target_iv *iv = t->iv + t->contig_first[c];
        const uint32_t ni = t->contig_count[c];
        t->contig_blk_first[c] = t->n_blocks;
        uint32_t next = c0;
        for (uint32_t i = 0; i < ni; i++) {
            uint32_t b0, b1;
            region_pick(u, c0, c1, iv[i].beg, iv[i].end, t->smax, &b0, &b1);
            for (uint32_t b = b0 > next ? b0 : next; b < b1; b++) { t->blocks[t->n_blocks++] = b; next = b + 1; }
        }
        t->contig_blk_count[c] = t->n_blocks - t->contig_blk_first[c];
        uint32_t lo = 0, hi = 0;                          /* both move forward with the block */
        for (uint32_t k = t->contig_blk_first[c]; k < t->n_blocks; k++) {
            const uint32_t b = t->blocks[k];
            const uint64_t F = u->window_start[b] + 1u;
            const uint64_t reach = b + 1 < c1 ? u->window_start[b + 1] + 1u + t->smax : UINT64_MAX;
            while (lo < ni && iv[lo].end < F) lo++;
            if (hi < lo) hi = lo;
            while (hi < ni && iv[hi].beg <= reach) hi++;
            t->block_iv[2 * k] = t->contig_first[c] + lo; t->block_iv[2 * k + 1] = hi - lo;
        }
    }
    return rc;
}

API uint64_t cbc_unpack_targets_text_cap(const cbc_unpack_plan *u, const cbc_targets *t, int sam)
{
    if (!u || !t || u->long_reads || !u->block_contig || !u->names || !u->contig_name_off) return 0;
    uint64_t n = 0;
    for (uint32_t k = 0; k < t->n_blocks; k++) {
        const uint32_t b = t->blocks[k];
        if (b >= u->n_blocks) return 0;
        n += sam ? cbc_unpack_sam_text_cap(u, b, b + 1) : (uint64_t)u->blocks[b].n_reads * (u->seq_stride + 1ull);
    }
    return n;
}

API uint64_t cbc_unpack_targets_depth_cap(const cbc_unpack_plan *u, const cbc_targets *t, uint32_t contig)
{
    if (!u || !t || u->long_reads || !u->names || !u->contig_name_off || contig >= u->n_contigs || contig >= t->n_contigs) return 0;
    const int64_t nl = sam_name_len(u, contig);
    if (nl < 0 || !t->contig_count[contig] || !t->contig_blk_count[contig]) return 0;
    uint64_t k = 0;
    for (uint32_t i = 0; i < t->contig_blk_count[contig]; i++) {
        const uint32_t b = t->blocks[t->contig_blk_first[contig] + i];
        if (b >= u->n_blocks) return 0;
        k += u->blocks[b].n_reads;
    }
    return (2u * k + 2ull * t->contig_count[contig] - 1u) * ((uint64_t)nl + 34u);
}

/* the same under skip_deletions: the proof of cbc_unpack_depth_skipdel_text_cap with the positions of
 * the contig's merged intervals in the window's place -- a run lies inside one interval */
API uint64_t cbc_unpack_targets_depth_skipdel_cap(const cbc_unpack_plan *u, const cbc_targets *t, uint32_t contig)
{
    if (!u || !t || u->long_reads || !u->names || !u->contig_name_off || contig >= u->n_contigs || contig >= t->n_contigs) return 0;
    const int64_t nl = sam_name_len(u, contig);
    if (nl < 0 || !t->contig_count[contig] || !t->contig_blk_count[contig]) return 0;
    uint64_t k = 0, w = 0;
    for (uint32_t i = 0; i < t->contig_blk_count[contig]; i++) {
        const uint32_t b = t->blocks[t->contig_blk_first[contig] + i];
        if (b >= u->n_blocks) return 0;
        k += u->blocks[b].n_reads;
    }
    for (uint32_t i = 0; i < t->contig_count[contig]; i++) {
        const cbc_target_iv *v = &t->iv[t->contig_first[contig] + i];
        w += (uint64_t)(v->end - v->beg) + 1u;
    }
    const uint64_t by_reads = k * t->smax;
    return (w < by_reads ? w : by_reads) * ((uint64_t)nl + 34u);
}

/* ---- per-target coverage summary (include/cbc_host.h) ---- */
API void cbc_queries_free(cbc_queries *q)
{
    if (!q) return;
    free(q->q); cbc_targets_free(q->targets); free(q);
}

API int cbc_coverage_mean(uint64_t sum, uint64_t len, char *dst)
{
    if (!dst) return CBC_E_ARG;
    uint64_t m = 0;
    if (len) { const uint64_t q = sum / len, r = sum % len; m = q * 100u + (r * 100u + len / 2u) / len; }
    return sprintf(dst, "%llu.%02u", (unsigned long long)(m / 100u), (unsigned)(m % 100u));
}

/* ---- read statistics (include/cbc_host.h) ---- */
#define STATS_N_FS 15
static const char *const stats_fs_name[STATS_N_FS] = {
    "total", "primary", "secondary", "supplementary", "duplicates", "primary duplicates", "mapped", "primary mapped",
    "paired in sequencing", "read1", "read2", "properly paired", "with itself and mate mapped", "singletons", "reverse strand" };

API uint64_t cbc_stats_text_cap(void)
{
    /* per line: the tag and its tab, the longest name or key, a tab and the longest number per column, the newline */
    return 11u * (3u + 14u + 1u + 23u + 1u) + STATS_N_FS * (3u + 27u + 2u * (1u + 20u) + 1u) + (uint64_t)CBC_STATS_FLAG_BINS * (3u + 5u + 1u + 10u + 1u) +
           CBC_STATS_LEN_BINS * (3u + 3u + 1u + 10u + 1u) + CBC_STATS_GC_BINS * (3u + 3u + 1u + 10u + 1u) + CBC_STATS_CYCLES * (3u + 3u + 5u * (1u + 10u) + 1u);
}

API int64_t cbc_stats_text(const cbc_gpu_stats *s, char *dst, uint64_t cap)
{
    if (!s || !dst || cap < cbc_stats_text_cap()) return CBC_E_ARG;
    char *p = dst;
    uint64_t bases = 0, sym[5] = { 0, 0, 0, 0, 0 }, fs[STATS_N_FS][2];
    uint32_t lmin = 0, lmax = 0;
    int any = 0;
    for (uint32_t l = 0; l < CBC_STATS_LEN_BINS; l++)
        if (s->len[l]) { bases += (uint64_t)l * s->len[l]; if (!any) lmin = l; lmax = l; any = 1; }
    for (uint32_t k = 0; k < 5u; k++) for (uint32_t c = 0; c < CBC_STATS_CYCLES; c++) sym[k] += s->cyc[k * CBC_STATS_CYCLES + c];
    char mean[32];
    (void)cbc_coverage_mean(bases, s->reads, mean);
    p += sprintf(p, "SN\treads\t%llu\nSN\treads excluded\t%llu\nSN\tbases\t%llu\n", (unsigned long long)s->reads, (unsigned long long)s->excluded,
                 (unsigned long long)bases);
    p += sprintf(p, "SN\tminimum length\t%u\nSN\tmaximum length\t%u\nSN\taverage length\t%s\n", lmin, lmax, mean);
    p += sprintf(p, "SN\tbases A\t%llu\nSN\tbases C\t%llu\nSN\tbases G\t%llu\nSN\tbases T\t%llu\nSN\tbases other\t%llu\n", (unsigned long long)sym[0],
                 (unsigned long long)sym[1], (unsigned long long)sym[2], (unsigned long long)sym[3], (unsigned long long)sym[4]);
    memset(fs, 0, sizeof fs);
    for (uint32_t f = 0; f < CBC_STATS_FLAG_BINS; f++) {
        const uint64_t n = s->flag[f];
        if (!n) continue;
        const int q = (f & 0x200u) != 0, sec = (f & 0x100u) != 0, sup = !sec && (f & 0x800u), pri = !sec && !sup;
        const int dup = (f & 0x400u) != 0, map = !(f & 0x4u), pair = pri && (f & 0x1u);
        const int in[STATS_N_FS] = { 1, pri, sec, sup, dup, pri && dup, map, pri && map, pair, pair && (f & 0x40u), pair && (f & 0x80u),
                                     pair && (f & 0x2u) && map, pair && map && !(f & 0x8u), pair && map && (f & 0x8u), (f & 0x10u) != 0 };
        for (int k = 0; k < STATS_N_FS; k++) if (in[k]) fs[k][q] += n;
    }
    for (int k = 0; k < STATS_N_FS; k++)
        p += sprintf(p, "FS\t%s\t%llu\t%llu\n", stats_fs_name[k], (unsigned long long)fs[k][0], (unsigned long long)fs[k][1]);
    for (uint32_t f = 0; f < CBC_STATS_FLAG_BINS; f++) if (s->flag[f]) p += sprintf(p, "FL\t%u\t%u\n", f, s->flag[f]);
    for (uint32_t l = 0; l < CBC_STATS_LEN_BINS; l++) if (s->len[l]) p += sprintf(p, "RL\t%u\t%u\n", l, s->len[l]);
    for (uint32_t g = 0; g < CBC_STATS_GC_BINS; g++) if (s->gc[g]) p += sprintf(p, "GC\t%u\t%u\n", g, s->gc[g]);
    for (uint32_t c = 0; c < lmax && c < CBC_STATS_CYCLES; c++)
        p += sprintf(p, "BC\t%u\t%u\t%u\t%u\t%u\t%u\n", c + 1u, s->cyc[c], s->cyc[CBC_STATS_CYCLES + c], s->cyc[2u * CBC_STATS_CYCLES + c],
                     s->cyc[3u * CBC_STATS_CYCLES + c], s->cyc[4u * CBC_STATS_CYCLES + c]);
    return (int64_t)(p - dst);
}

/* ---- alignment tables of the read statistics (include/cbc_host.h) ---- */
API uint64_t cbc_stats_aln_text_cap(void)
{
    /* per line: the tag and its tab, the longest name or key, a tab and the longest number per column, the newline */
    return 11u * (3u + 23u + 1u + 21u + 1u) + (CBC_STATS_ALN_CYC - 1u) * (3u + 3u + 2u * (1u + 20u) + 1u) + CBC_STATS_ALN_CYC * (3u + 3u + 2u * (1u + 10u) + 1u) +
           (CBC_STATS_ALN_LEN - 1u) * (3u + 3u + 2u * (1u + 20u) + 1u) + CBC_STATS_ALN_NM * (3u + 3u + 1u + 10u + 1u);
}

API int64_t cbc_stats_aln_text(const cbc_gpu_stats_aln *a, char *dst, uint64_t cap)
{
    if (!a || !dst || cap < cbc_stats_aln_text_cap()) return CBC_E_ARG;
    char *p = dst;
    uint64_t aligned[CBC_STATS_ALN_CYC], al = 0, mm = 0, unal = 0, ins = 0, del = 0, bi = 0, bd = 0, reach = 0;
    uint32_t lmax = 0;
    for (uint32_t l = 1; l < CBC_STATS_ALN_CYC; l++) { reach += a->len[l]; if (a->len[l]) lmax = l; }
    aligned[0] = 0;
    for (uint32_t c = 1; c < CBC_STATS_ALN_CYC; c++) {               /* reach: the valid reads of length >= c */
        aligned[c] = reach - a->unal[c];
        al += aligned[c]; mm += a->mm[c]; unal += a->unal[c];
        reach -= a->len[c];
    }
    for (uint32_t l = 1; l < CBC_STATS_ALN_LEN; l++) {
        ins += a->ins_len[l]; del += a->del_len[l]; bi += (uint64_t)l * a->ins_len[l]; bd += (uint64_t)l * a->del_len[l];
    }
    char rate[40];
    (void)cbc_hist_fraction(mm, al, rate);
    p += sprintf(p, "AS\treads\t%llu\nAS\treads without alignment\t%llu\nAS\tbases aligned\t%llu\nAS\tmismatches\t%llu\nAS\tmismatch rate\t%s\n",
                 (unsigned long long)a->reads, (unsigned long long)a->invalid, (unsigned long long)al, (unsigned long long)mm, rate);
    p += sprintf(p, "AS\tinsertions\t%llu\nAS\tdeletions\t%llu\nAS\tbases inserted\t%llu\nAS\tbases deleted\t%llu\nAS\tbases soft-clipped\t%llu\n",
                 (unsigned long long)ins, (unsigned long long)del, (unsigned long long)bi, (unsigned long long)bd, (unsigned long long)(unal - bi));
    p += sprintf(p, "AS\treads with NM 0\t%u\n", a->nm[0]);
    for (uint32_t c = 1; c <= lmax; c++) p += sprintf(p, "MC\t%u\t%llu\t%u\n", c, (unsigned long long)aligned[c], a->mm[c]);
    for (uint32_t c = 0; c < CBC_STATS_ALN_CYC; c++) if (a->ins_cyc[c] | a->del_cyc[c]) p += sprintf(p, "IC\t%u\t%u\t%u\n", c, a->ins_cyc[c], a->del_cyc[c]);
    for (uint32_t l = 1; l < CBC_STATS_ALN_LEN; l++)
        if (a->ins_len[l] | a->del_len[l]) p += sprintf(p, "ID\t%u\t%llu\t%llu\n", l, (unsigned long long)a->ins_len[l], (unsigned long long)a->del_len[l]);
    for (uint32_t n = 0; n < CBC_STATS_ALN_NM; n++) if (a->nm[n]) p += sprintf(p, "NM\t%u\t%u\n", n, a->nm[n]);
    return (int64_t)(p - dst);
}

/* ---- depth histogram (include/cbc_host.h) ---- */
API uint64_t cbc_unpack_targets_size(const cbc_targets *t, uint32_t contig)
{
    if (!t || contig >= t->n_contigs) return 0;
    uint64_t n = 0;
    for (uint32_t i = 0; i < t->contig_count[contig]; i++) {
        const cbc_target_iv *v = &t->iv[t->contig_first[contig] + i];
        n += (uint64_t)(v->end - v->beg) + 1u;
    }
    return n;
}

API int cbc_hist_fraction(uint64_t bases, uint64_t size, char *dst)
{
    if (!dst) return CBC_E_ARG;
    uint64_t m = 0;
    if (size) m = (uint64_t)(((unsigned __int128)bases * 1000000u + size / 2u) / size);   /* 128 bits: a genome's sums are 64 */
    return sprintf(dst, "%llu.%06u", (unsigned long long)(m / 1000000u), (unsigned)(m % 1000000u));
}

API int cbc_unpack_queries(const cbc_unpack_plan *u, const char *const *regions, uint32_t n_regions, const char *bed, size_t bed_len,
                           uint64_t window, cbc_queries **out, char *errbuf, size_t errlen)
{
    if (!u || !out || (n_regions && !regions) || (bed_len && !bed) || (uint64_t)bed_len > 0xffffffffull) return CBC_E_ARG;
    *out = NULL;
    if (errbuf && errlen) errbuf[0] = 0;
    const int64_t hdr = cbc_unpack_sam_header(u, NULL, 0, errbuf, errlen);   /* what cbc_unpack_targets refuses */
    if (hdr < 0) return (int)hdr;
    if (!u->block_contig) return CBC_E_ARG;
    target_raw *raw = NULL;
    uint64_t n = 0, cap = 0;
    query_list L = { NULL, 0, 0 };
    uint32_t *iv_slot = NULL;
    int rc = 0;
    cbc_queries *Q = (cbc_queries *)calloc(1, sizeof *Q);
    cbc_targets *t = (cbc_targets *)calloc(1, sizeof *t);
    if (!Q || !t) { free(Q); free(t); return CBC_E_NOMEM; }
    Q->targets = t;
    for (uint32_t r = 0; r < n_regions && !rc; r++) {
        cbc_region_sel sel;
        if (!regions[r]) { rc = CBC_E_ARG; break; }
        rc = cbc_unpack_region(u, regions[r], &sel, errbuf, errlen);
        if (!rc) rc = target_push(&raw, &n, &cap, sel.contig, sel.beg, sel.end);
        if (!rc) rc = query_push(&L, sel.contig, sel.beg, sel.end, 0, 0, 0, 0);
    }
    if (!rc && bed) rc = bed_parse(u, bed, bed_len, &raw, &n, &cap, &t->bed_unselected, &L, errbuf, errlen);
    for (uint32_t c = 0; !n_regions && !bed && c < u->n_contigs && !rc; c++) {   /* no input: every contig as a whole */
        cbc_region_sel sel;
        rc = cbc_unpack_contig_blocks(u, c, &sel, errbuf, errlen);
        if (!rc) rc = target_push(&raw, &n, &cap, sel.contig, sel.beg, sel.end);
        if (!rc) rc = query_push(&L, sel.contig, sel.beg, sel.end, 0, 0, 0, 0);
    }
    if (!rc) rc = targets_build(u, t, raw, n, errbuf, errlen);
    if (rc) goto fail;
    {
        /* the windows: counted first, so that a refused list allocates nothing */
        uint64_t total = 0;
        for (uint64_t i = 0; i < L.n && total <= CBC_TARGETS_MAX_IV; i++) {
            const uint64_t len = L.q[i].end0 - L.q[i].start0;
            total += window && len ? (len - 1u) / window + 1u : 1u;
        }
        if (total > CBC_TARGETS_MAX_IV) {
            rc = region_err(errbuf, errlen, "more than 2^24 coverage queries%.*s", window ? " after cutting into windows" : "", 64);
            goto fail;
        }
        Q->q = (cbc_query *)calloc(total ? (size_t)total : 1u, sizeof(cbc_query));
        if (!Q->q) { rc = CBC_E_NOMEM; goto fail; }
        for (uint64_t i = 0; i < L.n; i++) {
            const cbc_query *x = &L.q[i];
            const uint64_t len = x->end0 - x->start0, step = window && len ? window : (len ? len : 1u);
            for (uint64_t o = 0; o == 0 || o < len; o += step) {
                cbc_query *y = &Q->q[Q->n_q++];
                *y = *x;
                y->start0 = x->start0 + o;
                y->end0 = len - o > step ? y->start0 + step : x->end0;
                if (x->contig != CBC_QUERY_UNKNOWN) { y->beg = (uint32_t)(y->start0 + 1u); y->end = (uint32_t)y->end0; }
            }
        }
    }
    /* the slots: per contig the merged intervals end to end with one spare slot behind each (at most 2^31 + 2^24 of them) */
    iv_slot = (uint32_t *)malloc(((size_t)t->n_iv + 1u) * 4u);
    if (!iv_slot) { rc = CBC_E_NOMEM; goto fail; }
    for (uint32_t c = 0; c < t->n_contigs; c++) {
        uint64_t run = 0;
        for (uint32_t i = 0; i < t->contig_count[c]; i++) {
            const cbc_target_iv *v = &t->iv[t->contig_first[c] + i];
            iv_slot[t->contig_first[c] + i] = (uint32_t)run;
            run += (uint64_t)(v->end - v->beg) + 2u;
        }
    }
    for (uint64_t i = 0; i < Q->n_q; i++) {
        cbc_query *y = &Q->q[i];
        if (y->contig == CBC_QUERY_UNKNOWN || y->end0 == y->start0) continue;
        const cbc_target_iv *iv = t->iv + t->contig_first[y->contig];
        uint32_t lo = 0, hi = t->contig_count[y->contig];            /* the last interval with beg <= the query's */
        while (hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if (iv[mid].beg <= y->beg) lo = mid; else hi = mid; }
        if (hi == 0 || iv[lo].beg > y->beg || iv[lo].end < y->end) { rc = CBC_E_ARG; goto fail; }   /* merging lost a query: never */
        y->slot = iv_slot[t->contig_first[y->contig] + lo] + (y->beg - iv[lo].beg);
    }
    free(iv_slot); free(raw); free(L.q);
    *out = Q;
    return 0;
fail:
    free(iv_slot); free(raw); free(L.q);
    cbc_queries_free(Q);
    return rc;
}

/* One reconstructed read per line (print_line, src/compression.c:16-40). */
API int64_t cbc_unpack_write_text(const cbc_unpack_plan *u, const cbc_read_rec *recs, const uint8_t *seq,
                                  char *dst, uint64_t cap)
{
    if (!u || !recs || !seq || !dst) return CBC_E_ARG;
    uint64_t n = 0;
    if (u->long_reads) {                                 /* bases are compact: block base + the record's offset */
        for (uint32_t b = 0; b < u->n_blocks; b++) {
            const cbc_dec_block_desc *d = &u->blocks[b];
            for (uint32_t k = 0; k < d->n_reads; k++) {
                const cbc_read_rec *r = &recs[d->rec_base + k];
                if ((uint64_t)r->seq_off + r->rlen > d->reserved[0] || n + r->rlen + 1 > cap) return CBC_E_ARG;
                memcpy(dst + n, seq + d->seq_base + r->seq_off, r->rlen); n += r->rlen;
                dst[n++] = '\n';
            }
        }
        return (int64_t)n;
    }
    for (uint64_t r = 0; r < u->n_recs; r++) {
        uint32_t rl = recs[r].rlen;
        if (rl > u->seq_stride || n + rl + 1 > cap) return CBC_E_ARG;
        memcpy(dst + n, seq + r * u->seq_stride, rl); n += rl;
        dst[n++] = '\n';
    }
    return (int64_t)n;
}
