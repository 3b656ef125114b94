/*
 * cbc_cli_unpack.c -- `cbc -d / -x`: container + FASTA -> one reconstructed read per line, decoded
 * on the GPU (decompress(), src/compression.c:173-216; print_line :16-40).
 */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <pthread.h>
#include <time.h>
#include "../../include/cbc_host.h"
#include "cbc_cli.h"

static char *slurp2(const char *path, size_t *len)
{
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cbc: cannot open %s: %s\n", path, strerror(errno)); return NULL; }
    fseek(f, 0, SEEK_END); long n = ftell(f); rewind(f);
    if (n < 0) { fclose(f); return NULL; }
    char *buf = (char *)malloc((size_t)n + 1);
    if (!buf || fread(buf, 1, (size_t)n, f) != (size_t)n) { fclose(f); free(buf); fprintf(stderr, "cbc: cannot read %s\n", path); return NULL; }
    fclose(f); buf[n] = 0; *len = (size_t)n;
    return buf;
}

/* a file that does not start with the container magic is the reference's own format: one stream (decompress(),
 * src/compression.c:173-216).  The record count is not known in advance: the buffers grow until the kernel stops
 * reporting OUT_FULL. */
static int decompress_stream(const uint8_t *blob, size_t blob_len, const char *fa, size_t fa_len, const char *out, int device)
{
    char err[512];
    cbc_reference *R = NULL;
    if (cbc_reference_load(fa, fa_len, 0, &R, err, sizeof err)) { fprintf(stderr, "cbc: %s\n", err); return 1; }
    uint32_t L0 = cbc_stream_read_length(blob, blob_len);
    if (L0 < 1 || L0 > 256) { fprintf(stderr, "cbc: not a cbc file (neither a block container nor a stream with a sane read length)\n"); return 1; }
    cbc_gpu_ctx *ctx = NULL;
    int rc = cbc_gpu_init(device, &ctx);
    if (rc) { fprintf(stderr, "cbc: no usable MI355X (cbc_gpu_init = %d); there is no CPU fallback\n", rc); return 1; }
    if (cbc_gpu_upload_reference(ctx, R->bases, R->n_bytes)) { fprintf(stderr, "cbc: %s\n", cbc_gpu_last_error(ctx)); return 1; }
    /* rows of the header read length rounded up to 4 (the decoder refuses a longer read: quirk Q7 makes fixed-length input
     * the only kind that decodes), room for one record per stream byte to begin with (files run at 1.4 - 2 bytes per read),
     * doubled while the kernel reports OUT_FULL; the record count is capped where rec_cap stops fitting 32 bits */
    const uint32_t stride = ((L0 < 4 ? 4 : L0) + 3u) & ~3u;
    uint64_t cap = (uint64_t)blob_len + 65536;
    for (;;) {
        if (cap > 0xffffffffull) cap = 0xffffffffull;
        cbc_read_rec *recs = (cbc_read_rec *)malloc((size_t)cap * sizeof(cbc_read_rec));
        uint8_t *seq = (uint8_t *)malloc((size_t)(cap * stride + 8));
        if (!recs || !seq) { fprintf(stderr, "cbc: out of memory\n"); return 1; }
        cbc_stream_result sr; memset(&sr, 0, sizeof sr);
        rc = cbc_gpu_decode_stream(ctx, blob, blob_len, R->contig_off, R->contig_len, R->n_contigs, recs, cap, seq, cap * stride + 8, stride, &sr);
        if (rc == CBC_E_BLOCK && sr.status == CBC_ST_OUT_FULL && cap < 0xffffffffull) { free(recs); free(seq); cap *= 2; continue; }
        if (rc) { fprintf(stderr, "cbc: decode failed: %s\n", cbc_gpu_last_error(ctx)); return 1; }
        FILE *fo = fopen(out, "wb");
        if (!fo) { fprintf(stderr, "cbc: cannot write %s\n", out); return 1; }
        for (uint64_t r = 0; r < sr.nbytes; r++) {                 /* print_line, src/compression.c:16-40 */
            fwrite(seq + r * stride, 1, recs[r].rlen, fo); fputc('\n', fo);
        }
        if (fclose(fo) != 0) { fprintf(stderr, "cbc: cannot write %s\n", out); return 1; }
        printf("%llu reads decompressed from one stream\n", (unsigned long long)sr.nbytes);
        free(recs); free(seq);
        break;
    }
    cbc_gpu_shutdown(ctx);
    cbc_reference_free(R);
    return 0;
}

/* one device's share of the blocks: a contiguous range, decoded into its slice of the output arrays */
typedef struct { const cbc_unpack_plan *u; int device; uint32_t b0, b1; cbc_read_rec *recs; uint8_t *seq; int rc; char err[512]; } dec_job;

static void *dev_decode(void *arg)
{
    dec_job *J = (dec_job *)arg;
    const cbc_unpack_plan *u = J->u;
    if (J->b1 <= J->b0) return NULL;
    cbc_gpu_ctx *ctx = NULL;
    J->rc = cbc_gpu_init(J->device, &ctx);
    if (J->rc) { snprintf(J->err, sizeof J->err, "no usable MI355X at ordinal %d (cbc_gpu_init = %d)", J->device, J->rc); return NULL; }
    J->rc = cbc_gpu_upload_reference(ctx, u->ref, u->ref_bytes);
    if (!J->rc) {
        const uint32_t nb = J->b1 - J->b0;
        cbc_dec_block_desc *bl = (cbc_dec_block_desc *)malloc((size_t)nb * sizeof(cbc_dec_block_desc));
        if (!bl) J->rc = CBC_E_NOMEM;
        else {
            memcpy(bl, u->blocks + J->b0, (size_t)nb * sizeof(cbc_dec_block_desc));
            const uint64_t in0 = bl[0].in_off, r0 = bl[0].rec_base;
            uint64_t in1 = 0, nrec = 0;
            for (uint32_t k = 0; k < nb; k++) {
                if (bl[k].in_off + bl[k].in_bytes > in1) in1 = bl[k].in_off + bl[k].in_bytes;
                bl[k].in_off -= in0; bl[k].rec_base -= r0; bl[k].seq_base = bl[k].rec_base * u->seq_stride; nrec += bl[k].n_reads;
            }
            J->rc = cbc_gpu_decode_blocks(ctx, u->payloads + in0, in1 - in0, bl, nb, &u->caps, J->recs + r0, nrec,
                                          J->seq + r0 * u->seq_stride, nrec * u->seq_stride, NULL);   /* exactly this range's bytes: the next range belongs to another thread */
            free(bl);
        }
    }
    if (J->rc) snprintf(J->err, sizeof J->err, "%s", cbc_gpu_last_error(ctx));
    cbc_gpu_shutdown(ctx);
    return NULL;
}

int cbc_cli_decompress(const char *in, const char *out, const char *ref, const int *devs, int ndev)
{
    const int device = devs[0];
    size_t blob_len = 0, fa_len = 0;
    char *blob = slurp2(in, &blob_len), *fa = slurp2(ref, &fa_len);
    if (!blob || !fa) return 1;
    if (blob_len < 4 || memcmp(blob, "CBCB", 4) != 0) {
        int rc = decompress_stream((const uint8_t *)blob, blob_len, fa, fa_len, out, device);
        free(blob); free(fa);
        return rc;
    }
    char err[512];
    cbc_unpack_plan *u = NULL;
    int rc = cbc_unpack_plan_create((const uint8_t *)blob, blob_len, fa, fa_len, &u, err, sizeof err);
    free(fa);
    if (rc) { fprintf(stderr, "cbc: %s\n", err); return 1; }
    cbc_gpu_ctx *ctx = NULL;
    rc = cbc_gpu_init(device, &ctx);
    if (rc) { fprintf(stderr, "cbc: no usable MI355X (cbc_gpu_init = %d); there is no CPU fallback\n", rc); return 1; }
    if (cbc_gpu_upload_reference(ctx, u->ref, u->ref_bytes)) { fprintf(stderr, "cbc: %s\n", cbc_gpu_last_error(ctx)); return 1; }
    uint64_t seq_bytes = u->long_reads ? u->seq_total : u->n_recs * u->seq_stride + 8;
    const uint64_t text_cap = (u->long_reads ? u->seq_total : u->n_recs * u->seq_stride) + u->n_recs + 16;
    cbc_read_rec *recs = (cbc_read_rec *)calloc((size_t)(u->n_recs ? u->n_recs : 1), sizeof(cbc_read_rec));
    uint8_t *seq = (uint8_t *)calloc((size_t)seq_bytes, 1);
    char *text = (char *)malloc((size_t)text_cap);
    if (!recs || !seq || !text) { fprintf(stderr, "cbc: out of memory\n"); return 1; }
    if (u->long_reads) {
        rc = cbc_gpu_long_decode_blocks(ctx, u->payloads, u->payload_bytes, u->blocks, u->n_blocks, &u->caps, recs, u->n_recs, seq, seq_bytes, NULL);
        if (rc) { fprintf(stderr, "cbc: decode failed: %s\n", cbc_gpu_last_error(ctx)); return 1; }
    } else if (ndev > 1) {
        /* contiguous block ranges balanced by record count, one host thread and one context per device */
        dec_job jobs[16]; pthread_t th[16];
        if (ndev > 16) ndev = 16;
        uint32_t b = 0; uint64_t done = 0;
        for (int d = 0; d < ndev; d++) {
            memset(&jobs[d], 0, sizeof jobs[d]);
            jobs[d].u = u; jobs[d].device = devs[d]; jobs[d].recs = recs; jobs[d].seq = seq; jobs[d].b0 = b;
            uint64_t target = u->n_recs * (uint64_t)(d + 1) / (uint64_t)ndev;
            while (b < u->n_blocks && (done < target || d == ndev - 1)) { done += u->blocks[b].n_reads; b++; }
            jobs[d].b1 = b;
            if (pthread_create(&th[d], NULL, dev_decode, &jobs[d]) != 0) { fprintf(stderr, "cbc: cannot start a device thread\n"); return 1; }
        }
        for (int d = 0; d < ndev; d++) { pthread_join(th[d], NULL); if (jobs[d].rc) { fprintf(stderr, "cbc: device %d: decode failed: %s\n", devs[d], jobs[d].err); rc = 1; } }
        if (rc) return 1;
    } else {
    rc = cbc_gpu_decode_blocks(ctx, u->payloads, u->payload_bytes, u->blocks, u->n_blocks, &u->caps, recs, u->n_recs, seq, seq_bytes, NULL);
    if (rc) { fprintf(stderr, "cbc: decode failed: %s\n", cbc_gpu_last_error(ctx)); return 1; }
    }
    int64_t n = cbc_unpack_write_text(u, recs, seq, text, text_cap);
    if (n < 0) { fprintf(stderr, "cbc: text assembly failed\n"); return 1; }
    FILE *fo = fopen(out, "wb");
    if (!fo || fwrite(text, 1, (size_t)n, fo) != (size_t)n || fclose(fo) != 0) { fprintf(stderr, "cbc: cannot write %s\n", out); return 1; }
    printf("%llu reads decompressed from %u blocks\n", (unsigned long long)u->n_recs, u->n_blocks);
    free(text); free(seq); free(recs); free(blob);
    cbc_gpu_shutdown(ctx);
    cbc_unpack_plan_free(u);
    return 0;
}

/* ---- the decode modes that write something other than every read (DESIGN.md sections 4.10 - 4.22).  The steps they share are
 * written once, cli_open .. cli_close; each mode function below is what it selects, its call loop and what it prints. ---- */
static double now2(void) { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; }

typedef struct cli_run {
    char *blob, *bed;                 /* the container; the BED text, kept to the end (bedcov prints unknown contig names out of it) */
    size_t blob_len, bed_len;
    cbc_unpack_plan *u;
    cbc_gpu_ctx *ctx;                 /* opened by the first cli_device */
    int device, used;                 /* used: a device was opened, so there are kernel times to print */
    double t0, t1, t_init, t_dev;     /* start, selection done (set by the mode), seconds in cli_device, seconds in the decode calls */
} cli_run;

/* container and FASTA read, the magic checked (opt: the option the message names; lacks: what a single stream does not have),
 * then the BED file, then the plan */
static int cli_open(cli_run *r, const char *in, const char *ref, const char *bed_path, int device, const char *opt, const char *lacks)
{
    memset(r, 0, sizeof *r);
    r->t0 = now2();
    r->device = device;
    size_t fa_len = 0;
    r->blob = slurp2(in, &r->blob_len);
    char *fa = slurp2(ref, &fa_len);
    if (!r->blob || !fa) return 1;
    if (r->blob_len < 4 || memcmp(r->blob, "CBCB", 4) != 0) {
        fprintf(stderr, "cbc: %s needs a block container; %s is a single-stream (--compat) file, which %s\n", opt, in, lacks);
        return 1;
    }
    if (bed_path && !(r->bed = slurp2(bed_path, &r->bed_len))) return 1;
    char err[512];
    const int rc = cbc_unpack_plan_create((const uint8_t *)r->blob, r->blob_len, fa, fa_len, &r->u, err, sizeof err);
    free(fa);
    if (rc) { fprintf(stderr, "cbc: %s\n", err); return 1; }
    return 0;
}

/* --skip-deletions: a setting of the run, as the library has it a setting of the context; the depth
 * modes read it for their text bounds and their messages, cli_device hands it to the device it opens */
static uint32_t g_skip_edits = 0;
void cbc_cli_skip_deletions(uint32_t edits_per_read) { g_skip_edits = edits_per_read; }

/* the device, opened and given the reference when the first call needs it: a selection without blocks needs none */
static int cli_device(cli_run *r)
{
    if (r->ctx) return 0;
    const double a = now2();
    const int rc = cbc_gpu_init(r->device, &r->ctx);
    if (rc) { fprintf(stderr, "cbc: no usable MI355X (cbc_gpu_init = %d); there is no CPU fallback\n", rc); return 1; }
    if (cbc_gpu_upload_reference(r->ctx, r->u->ref, r->u->ref_bytes)) { fprintf(stderr, "cbc: %s\n", cbc_gpu_last_error(r->ctx)); return 1; }
    if (g_skip_edits && cbc_gpu_set_depth_skip_deletions(r->ctx, g_skip_edits)) { fprintf(stderr, "cbc: --skip-deletions: %s\n", cbc_gpu_last_error(r->ctx)); return 1; }
    r->used = 1;
    r->t_init = now2() - a;
    return 0;
}

static void cli_close(cli_run *r)
{
    if (r->ctx) cbc_gpu_shutdown(r->ctx);
    free(r->bed); free(r->blob);
    cbc_unpack_plan_free(r->u);
}

/* descriptors, window starts and (bc != NULL) contigs of the blocks sel[0 .. nb), or of blocks 0 .. nb when sel == NULL */
static int cli_gather(const cbc_unpack_plan *u, const uint32_t *sel, uint32_t nb, cbc_dec_block_desc **bl, uint64_t **ws, uint32_t **bc)
{
    *bl = (cbc_dec_block_desc *)malloc((size_t)(nb ? nb : 1) * sizeof **bl);
    *ws = (uint64_t *)malloc((size_t)(nb ? nb : 1) * 8);
    if (bc) *bc = (uint32_t *)malloc((size_t)(nb ? nb : 1) * 4);
    if (!*bl || !*ws || (bc && !*bc)) { fprintf(stderr, "cbc: out of memory\n"); return 1; }
    for (uint32_t k = 0; k < nb; k++) {
        const uint32_t b = sel ? sel[k] : k;
        (*bl)[k] = u->blocks[b]; (*ws)[k] = u->window_start[b];
        if (bc) (*bc)[k] = u->block_contig[b];
    }
    return 0;
}

static void add_ms(float *sum, const float *ms, int n) { for (int i = 0; i < n; i++) sum[i] += ms[i]; }
static int cannot_write(const char *out) { fprintf(stderr, "cbc: cannot write %s\n", out); return 1; }

/* `cbc -d|-x ... --region NAME[:BEG[-END]]`: the index selects the blocks that can hold a read overlapping the locus
 * (cbc_unpack_region), the device decodes only those, filters the reads and assembles their text (cbc_gpu_decode_region);
 * the output is what `cbc -x` writes for those reads, in the same order. */
int cbc_cli_decompress_region(const char *in, const char *out, const char *ref, int device, const char *region, int verbose)
{
    cli_run r;
    if (cli_open(&r, in, ref, NULL, device, "--region", "has no block index")) return 1;
    const cbc_unpack_plan *u = r.u;
    char err[512];
    cbc_region_sel sel;
    int rc = cbc_unpack_region(u, region, &sel, err, sizeof err);
    if (rc) { fprintf(stderr, "cbc: %s\n", rc == CBC_E_INPUT ? err : "region selection failed"); return 1; }
    const uint32_t nb = sel.b1 - sel.b0;
    uint64_t cap = 0;
    for (uint32_t b = sel.b0; b < sel.b1; b++) cap += (uint64_t)u->blocks[b].n_reads * (u->seq_stride + 1u);
    char *text = (char *)malloc((size_t)(cap ? cap : 1));
    if (!text) { fprintf(stderr, "cbc: out of memory\n"); return 1; }
    r.t1 = now2();
    uint64_t text_bytes = 0, n_sel = 0;
    float ms[3] = { 0, 0, 0 };
    if (nb) {                                            /* no block can hold such a read: no device needed */
        if (cli_device(&r)) return 1;
        const double b = now2();
        rc = cbc_gpu_decode_region(r.ctx, u->payloads, u->payload_bytes, u->blocks + sel.b0, nb, &u->caps, u->window_start + sel.b0,
                                   sel.beg, sel.end, sel.smax, (uint8_t *)text, cap, &text_bytes, &n_sel, NULL);
        if (rc) { fprintf(stderr, "cbc: region decode failed: %s\n", cbc_gpu_last_error(r.ctx)); return 1; }
        r.t_dev = now2() - b;
        if (verbose) (void)cbc_gpu_last_region_ms(r.ctx, &ms[0], &ms[1], &ms[2]);
    }
    const double t3 = now2();
    FILE *fo = fopen(out, "wb");
    if (!fo || (text_bytes && fwrite(text, 1, (size_t)text_bytes, fo) != (size_t)text_bytes) || fclose(fo) != 0) return cannot_write(out);
    printf("%llu reads in %s:%llu-%llu decompressed from %u of %u blocks\n", (unsigned long long)n_sel,
           u->names + u->contig_name_off[sel.contig], (unsigned long long)sel.beg, (unsigned long long)sel.end, nb, u->n_blocks);
    if (verbose) {
        printf("region: blocks [%u, %u) of %u selected, %llu reads written, %llu text bytes, span bound %u\n", sel.b0, sel.b1, u->n_blocks,
               (unsigned long long)n_sel, (unsigned long long)text_bytes, sel.smax);
        printf("time: read + plan + select %.3f s, device init + reference upload %.3f s, decode + filter + text %.3f s, write %.3f s\n",
               r.t1 - r.t0, r.t_init, r.t_dev, now2() - t3);
        if (r.used) printf("kernels: decode %.3f ms, filter + scan %.3f ms, text %.3f ms\n", ms[0], ms[1], ms[2]);
    }
    free(text);
    cli_close(&r);
    return 0;
}

/* `cbc -d|-x ... --sam [--region NAME[:BEG[-END]]]`: the same reads as without --sam, as SAM: the
 * header from the container's contig table (host), one alignment line per read assembled on the device
 * (cbc_gpu_decode_sam); only the text crosses PCIe. */
/* --cigar: the lines with CIGAR, NM and MD (cbc_gpu_decode_sam_cigar) behind the edit-reporting decoder
 * with an arena of edits_per_read entries per read (0: the default); the buffer is the plain lines' bound plus 64 bytes per read,
 * and the call is repeated once at the text's own size when that is too small */
int cbc_cli_decompress_sam(const char *in, const char *out, const char *ref, int device, const char *region, int cigar,
                           uint32_t edits_per_read, int verbose)
{
    cli_run r;
    if (cli_open(&r, in, ref, NULL, device, "--sam", "stores no contig table")) return 1;
    const cbc_unpack_plan *u = r.u;
    char err[512];
    const int64_t hdr = cbc_unpack_sam_header(u, NULL, 0, err, sizeof err);
    if (hdr < 0) { fprintf(stderr, "cbc: %s\n", hdr == CBC_E_INPUT ? err : "SAM header failed"); return 1; }
    cbc_region_sel sel;
    memset(&sel, 0, sizeof sel);
    sel.b1 = u->n_blocks;
    int rc = region ? cbc_unpack_region(u, region, &sel, err, sizeof err) : 0;
    if (rc) { fprintf(stderr, "cbc: %s\n", rc == CBC_E_INPUT ? err : "region selection failed"); return 1; }
    const uint32_t nb = sel.b1 - sel.b0;
    uint64_t cap = cbc_unpack_sam_text_cap(u, sel.b0, sel.b1);
    const uint64_t bound = cigar ? cbc_unpack_sam_cigar_text_cap(u, sel.b0, sel.b1, edits_per_read) : cap;
    if (cigar) {
        for (uint32_t q = sel.b0; q < sel.b1; q++) cap += 64ull * u->blocks[q].n_reads;
        if (cap > bound) cap = bound;
    }
    char *text = (char *)malloc((size_t)hdr + (size_t)cap + 1);
    if (!text || cbc_unpack_sam_header(u, text, (uint64_t)hdr, err, sizeof err) != hdr) { fprintf(stderr, "cbc: out of memory\n"); return 1; }
    r.t1 = now2();
    uint64_t text_bytes = 0, n_reads = 0;
    float ms[4] = { 0, 0, 0, 0 };
    if (nb) {                                            /* no block to decode: the header alone, no device needed */
        if (cli_device(&r)) return 1;
        const double b = now2();
        cbc_sam_region rg = { sel.beg, sel.end, sel.smax, 0 };
        for (int attempt = 0; attempt < 2; attempt++) {
            if (cigar)
                rc = cbc_gpu_decode_sam_cigar(r.ctx, u->payloads, u->payload_bytes, u->blocks + sel.b0, nb, &u->caps, u->window_start + sel.b0,
                                              u->block_contig + sel.b0, u->names, u->names_bytes, u->contig_name_off, u->n_contigs,
                                              region ? &rg : NULL, u->max_read_len + u->read_length - 1u, edits_per_read,
                                              (uint8_t *)text + hdr, cap, &text_bytes, &n_reads, NULL);
            else
                rc = cbc_gpu_decode_sam(r.ctx, u->payloads, u->payload_bytes, u->blocks + sel.b0, nb, &u->caps, u->window_start + sel.b0,
                                        u->block_contig + sel.b0, u->names, u->names_bytes, u->contig_name_off, u->n_contigs,
                                        region ? &rg : NULL, (uint8_t *)text + hdr, cap, &text_bytes, &n_reads, NULL);
            if (!(cigar && rc == CBC_E_ARG && text_bytes > cap && text_bytes <= bound)) break;
            cap = text_bytes;                            /* the text's own size */
            char *t2 = (char *)realloc(text, (size_t)hdr + (size_t)cap + 1);
            if (!t2) { fprintf(stderr, "cbc: out of memory\n"); return 1; }
            text = t2;
        }
        if (rc) { fprintf(stderr, "cbc: SAM decode failed: %s\n", cbc_gpu_last_error(r.ctx)); return 1; }
        r.t_dev = now2() - b;
        if (verbose && cigar) (void)cbc_gpu_last_sam_cigar_ms(r.ctx, &ms[0], &ms[1], &ms[2], &ms[3]);
        else if (verbose) (void)cbc_gpu_last_sam_ms(r.ctx, &ms[0], &ms[1], &ms[2]);
    }
    const double t3 = now2();
    const size_t total = (size_t)hdr + (size_t)text_bytes;
    FILE *fo = fopen(out, "wb");
    if (!fo || fwrite(text, 1, total, fo) != total || fclose(fo) != 0) return cannot_write(out);
    if (region)
        printf("%llu reads in %s:%llu-%llu written as SAM from %u of %u blocks\n", (unsigned long long)n_reads,
               u->names + u->contig_name_off[sel.contig], (unsigned long long)sel.beg, (unsigned long long)sel.end, nb, u->n_blocks);
    else printf("%llu reads written as SAM from %u blocks\n", (unsigned long long)n_reads, u->n_blocks);
    if (verbose) {
        printf("sam: blocks [%u, %u) of %u, %llu reads, %lld header bytes, %llu text bytes\n", sel.b0, sel.b1, u->n_blocks,
               (unsigned long long)n_reads, (long long)hdr, (unsigned long long)text_bytes);
        printf("time: read + plan + header %.3f s, device init + reference upload %.3f s, decode + count + text %.3f s, write %.3f s\n",
               r.t1 - r.t0, r.t_init, r.t_dev, now2() - t3);
        if (r.used && cigar) printf("kernels: edits decode %.3f ms, measure %.3f ms, count + scan %.3f ms, text %.3f ms\n", ms[0], ms[1], ms[2], ms[3]);
        else if (r.used) printf("kernels: decode %.3f ms, count + scan %.3f ms, text %.3f ms\n", ms[0], ms[1], ms[2]);
    }
    free(text);
    cli_close(&r);
    return 0;
}

/* `cbc -d|-x ... --depth [--region NAME[:BEG[-END]]]`: the coverage of the reads instead of the reads,
 * bedGraph computed and formatted on the device (cbc_gpu_decode_depth): one call for the region's window, or one per contig
 * that has blocks, in the order of the contig table, the texts appended.  Only the track crosses PCIe.  A call's buffer is the
 * bound of its blocks.
 * pu != NULL, `--pileup`: what the reads show at the positions where they disagree with the reference,
 * counted and formatted on the device (cbc_gpu_decode_pileup), the calls as for --depth.  A call starts with a buffer of 64 MiB
 * + 64 bytes per read of its blocks (or the bound, if that is less); the library reports the size of a text that does not fit,
 * and the call is made once more with exactly that.
 * --skip-deletions: the depth of the aligned bases alone; its bound is a line per position, not two per
 * read, so its buffer is handled as the pileup's.
 * --by-strand, --min-alt-frac: the same calls through cbc_gpu_decode_pileup_ext with the longer line's
 * bound; without either option the call is cbc_gpu_decode_pileup as before. */
typedef struct cli_pileup { uint32_t min_alt, edits_per_read, min_alt_ppm, by_strand; } cli_pileup;

static int decompress_window(const char *in, const char *out, const char *ref, int device, const char *region, uint32_t exclude,
                             const cli_pileup *pu, int verbose)
{
    const char *opt = pu ? "--pileup" : "--depth", *mode = opt + 2, *noun = pu ? "positions" : "runs";
    cli_run r;
    if (cli_open(&r, in, ref, NULL, device, opt, "stores no contig table")) return 1;
    const cbc_unpack_plan *u = r.u;
    char err[512];
    /* what SAM output refuses, these refuse: a long-read container, names and lengths the text cannot carry */
    if (cbc_unpack_sam_header(u, NULL, 0, err, sizeof err) < 0) { fprintf(stderr, "cbc: %s: %s\n", opt, err[0] ? err : "the contig table is not usable"); return 1; }
    /* the calls: the region's selection, or every contig as a whole */
    const uint32_t n_calls = region ? 1u : u->n_contigs;
    cbc_region_sel *sels = (cbc_region_sel *)calloc(n_calls ? n_calls : 1u, sizeof(cbc_region_sel));
    if (!sels) { fprintf(stderr, "cbc: out of memory\n"); return 1; }
    int rc;
    for (uint32_t k = 0; k < n_calls; k++) {
        rc = region ? cbc_unpack_region(u, region, &sels[k], err, sizeof err) : cbc_unpack_contig_blocks(u, k, &sels[k], err, sizeof err);
        if (rc) { fprintf(stderr, "cbc: %s\n", rc == CBC_E_INPUT ? err : "block selection failed"); return 1; }
    }
    r.t1 = now2();
    FILE *fo = fopen(out, "wb");
    if (!fo) return cannot_write(out);
    uint64_t total = 0, lines = 0, kept = 0, have = 0;
    char *text = NULL;
    uint32_t blocks_used = 0;
    float ms[4] = { 0, 0, 0, 0 }, m[4];
    for (uint32_t k = 0; k < n_calls; k++) {
        const cbc_region_sel *s = &sels[k];
        const uint32_t nb = s->b1 - s->b0;
        if (!nb) continue;                              /* no block can hold a read of the window: no line, no device needed */
        if (cli_device(&r)) return 1;
        const double b = now2();
        const char *nm = u->names + u->contig_name_off[s->contig];
        const int capped = pu || g_skip_edits;            /* a bound per position: start smaller, repeat once at the text's size */
        const int ext = pu && (pu->by_strand || pu->min_alt_ppm);
        const uint64_t bound = pu ? cbc_unpack_pileup_ext_text_cap(u, s->b0, s->b1, s->contig, s->beg, s->end, s->smax, pu->by_strand)
                             : g_skip_edits ? cbc_unpack_depth_skipdel_text_cap(u, s->b0, s->b1, s->contig, s->beg, s->end, s->smax)
                                            : cbc_unpack_depth_text_cap(u, s->b0, s->b1, s->contig);
        uint64_t cap = bound, first = 64ull << 20, tb = 0, nl = 0, nk = 0;
        for (uint32_t q = s->b0; q < s->b1; q++) first += 64ull * u->blocks[q].n_reads;
        if (capped && first < cap) cap = first;
        for (int attempt = 0; attempt < (capped ? 2 : 1); attempt++) {
            if (cap > have || !text) { free(text); text = (char *)malloc((size_t)cap + 1); have = cap; }
            if (!text) { fprintf(stderr, "cbc: out of memory\n"); return 1; }
            rc = ext ? cbc_gpu_decode_pileup_ext(r.ctx, u->payloads, u->payload_bytes, u->blocks + s->b0, nb, &u->caps, u->window_start + s->b0,
                                                 nm, (uint32_t)strlen(nm), s->beg, s->end, s->smax, exclude, pu->min_alt, pu->edits_per_read,
                                                 pu->min_alt_ppm, pu->by_strand, (uint8_t *)text, cap, &tb, &nl, &nk, NULL)
               : pu ? cbc_gpu_decode_pileup(r.ctx, u->payloads, u->payload_bytes, u->blocks + s->b0, nb, &u->caps, u->window_start + s->b0,
                                            nm, (uint32_t)strlen(nm), s->beg, s->end, s->smax, exclude, pu->min_alt, pu->edits_per_read,
                                            (uint8_t *)text, cap, &tb, &nl, &nk, NULL)
                    : cbc_gpu_decode_depth(r.ctx, u->payloads, u->payload_bytes, u->blocks + s->b0, nb, &u->caps, u->window_start + s->b0,
                                           nm, (uint32_t)strlen(nm), s->beg, s->end, s->smax, exclude, (uint8_t *)text, cap, &tb, &nl, &nk, NULL);
            if (!(rc == CBC_E_ARG && tb > cap && tb <= bound)) break;
            cap = tb;                                   /* the text's own size */
        }
        if (rc) { fprintf(stderr, "cbc: %s failed: %s\n", mode, cbc_gpu_last_error(r.ctx)); return 1; }
        r.t_dev += now2() - b;
        if (verbose && (pu ? cbc_gpu_last_pileup_ms : cbc_gpu_last_depth_ms)(r.ctx, &m[0], &m[1], &m[2], &m[3]) == 0) add_ms(ms, m, 4);
        if (tb && fwrite(text, 1, (size_t)tb, fo) != (size_t)tb) return cannot_write(out);
        total += tb; lines += nl; kept += nk; blocks_used += nb;
    }
    if (fclose(fo) != 0) return cannot_write(out);
    if (region)
        printf("%s of %s:%llu-%llu: %llu %s from %llu reads in %u of %u blocks\n", mode, u->names + u->contig_name_off[sels[0].contig],
               (unsigned long long)sels[0].beg, (unsigned long long)sels[0].end, (unsigned long long)lines, noun, (unsigned long long)kept,
               blocks_used, u->n_blocks);
    else printf("%s: %llu %s from %llu reads in %u blocks\n", mode, (unsigned long long)lines, noun, (unsigned long long)kept, blocks_used);
    if (verbose) {
        printf("%s: %llu text bytes, exclude flags 0x%x", mode, (unsigned long long)total, exclude);
        if (pu) printf(", min alt %u, edits per read %u", pu->min_alt, pu->edits_per_read ? pu->edits_per_read : CBC_EDITS_PER_READ);
        else if (g_skip_edits) printf(", deleted bases not counted, edits per read %u", g_skip_edits);
        printf("\ntime: read + plan %.3f s, device init + reference upload %.3f s, decode + %s + write %.3f s\n", r.t1 - r.t0, r.t_init, mode, r.t_dev);
        if (r.used) printf(pu ? "kernels: edits decode %.3f ms, mark + events %.3f ms, scans %.3f ms, text %.3f ms\n"
                              : g_skip_edits ? "kernels: edits decode %.3f ms, mark + unmark %.3f ms, scan + compact %.3f ms, text %.3f ms\n"
                              : "kernels: decode %.3f ms, mark %.3f ms, scan + compact %.3f ms, text %.3f ms\n", ms[0], ms[1], ms[2], ms[3]);
    }
    free(text); free(sels);
    cli_close(&r);
    return 0;
}

int cbc_cli_decompress_depth(const char *in, const char *out, const char *ref, int device, const char *region, uint32_t exclude, int verbose)
{
    return decompress_window(in, out, ref, device, region, exclude, NULL, verbose);
}

int cbc_cli_decompress_pileup(const char *in, const char *out, const char *ref, int device, const char *region, uint32_t exclude,
                              uint32_t min_alt, uint32_t edits_per_read, uint32_t min_alt_ppm, int by_strand, int verbose)
{
    const cli_pileup pu = { min_alt, edits_per_read, min_alt_ppm, by_strand ? 1u : 0u };
    return decompress_window(in, out, ref, device, region, exclude, &pu, verbose);
}

/* `cbc -d|-x ... --consensus [--region NAME[:BEG[-END]]]`: the sequence the reads spell, one FASTA record
 * per call, called and written on the device (cbc_gpu_decode_consensus): one call for the region's window (`>NAME:BEG-END`), or
 * one per contig of the table in table order (`>NAME`).  A call's buffer is its record's bound (cbc_unpack_consensus_text_cap), so
 * no call is repeated.  A selection without blocks, or whose blocks hold no read, is all low depth: its record is written on the
 * host (cbc_unpack_consensus_empty) and needs no device. */
int cbc_cli_decompress_consensus(const char *in, const char *out, const char *ref, int device, const char *region, uint32_t exclude,
                                 uint32_t min_depth, uint32_t call_ppm, uint32_t line_width, uint32_t flags, uint32_t edits_per_read, int verbose)
{
    cli_run r;
    if (cli_open(&r, in, ref, NULL, device, "--consensus", "stores no contig table")) return 1;
    const cbc_unpack_plan *u = r.u;
    char err[512];
    int status = 1;                                     /* every way out but the last goes through `done` */
    FILE *fo = NULL;
    char *text = NULL;
    if (cbc_unpack_sam_header(u, NULL, 0, err, sizeof err) < 0) { fprintf(stderr, "cbc: --consensus: %s\n", err[0] ? err : "the contig table is not usable"); goto done; }
    const uint32_t n_calls = region ? 1u : u->n_contigs, with_range = region ? 1u : 0u;
    const cbc_consensus_opts o = { min_depth, call_ppm, line_width, flags };
    r.t1 = now2();
    fo = fopen(out, "wb");
    if (!fo) { cannot_write(out); goto done; }
    cbc_consensus_counts tot, c;
    memset(&tot, 0, sizeof tot);
    uint64_t total = 0, kept = 0, have = 0;
    uint32_t blocks_used = 0;
    float ms[4] = { 0, 0, 0, 0 }, m[4];
    for (uint32_t k = 0; k < n_calls; k++) {
        cbc_region_sel s;
        int rc = region ? cbc_unpack_region(u, region, &s, err, sizeof err) : cbc_unpack_contig_blocks(u, k, &s, err, sizeof err);
        if (rc) { fprintf(stderr, "cbc: %s\n", rc == CBC_E_INPUT ? err : "block selection failed"); goto done; }
        const uint64_t cap = cbc_unpack_consensus_text_cap(u, s.contig, s.beg, s.end, line_width, with_range);
        if (!cap) { fprintf(stderr, "cbc: --consensus: the window %llu-%llu is not usable\n", (unsigned long long)s.beg, (unsigned long long)s.end); goto done; }
        if (cap > have || !text) { free(text); text = (char *)malloc((size_t)cap + 1); have = cap; }
        if (!text) { fprintf(stderr, "cbc: out of memory\n"); goto done; }
        uint32_t nb = s.b1 - s.b0;
        uint64_t reads = 0, tb = 0, nk = 0;
        for (uint32_t q = s.b0; q < s.b1; q++) reads += u->blocks[q].n_reads;
        if (!reads) nb = 0;
        if (!nb) {                                      /* no read can cover the window: all low depth, no device needed */
            const int64_t n = cbc_unpack_consensus_empty(u, s.contig, s.beg, s.end, &o, with_range, (uint8_t *)text, cap, &c);
            if (n < 0) { fprintf(stderr, "cbc: --consensus: the record of a window without reads failed (%lld)\n", (long long)n); goto done; }
            tb = (uint64_t)n;
        } else {
            if (cli_device(&r)) goto done;
            const double b = now2();
            const char *nm = u->names + u->contig_name_off[s.contig];
            rc = cbc_gpu_decode_consensus(r.ctx, u->payloads, u->payload_bytes, u->blocks + s.b0, nb, &u->caps, u->window_start + s.b0,
                                          nm, (uint32_t)strlen(nm), s.beg, s.end, s.smax, exclude, edits_per_read, &o, with_range,
                                          (uint8_t *)text, cap, &tb, &c, &nk, NULL);
            if (rc) { fprintf(stderr, "cbc: consensus failed: %s\n", cbc_gpu_last_error(r.ctx)); goto done; }
            r.t_dev += now2() - b;
            if (verbose && cbc_gpu_last_consensus_ms(r.ctx, &m[0], &m[1], &m[2], &m[3]) == 0) add_ms(ms, m, 4);
        }
        if (tb && fwrite(text, 1, (size_t)tb, fo) != (size_t)tb) { cannot_write(out); goto done; }
        total += tb; kept += nk; blocks_used += nb;
        tot.emitted += c.emitted; tot.ref += c.ref; tot.alt += c.alt; tot.del += c.del; tot.ambiguous += c.ambiguous;
        tot.low_depth += c.low_depth; tot.no_call += c.no_call; tot.ins_skipped += c.ins_skipped;
    }
    { FILE *f2 = fo; fo = NULL; if (fclose(f2) != 0) { cannot_write(out); goto done; } }
    printf("consensus: %llu bases (%llu ref, %llu alt, %llu deleted, %llu ambiguous, %llu low depth, %llu no call; %llu insertions not applied) from %llu reads in %u blocks\n",
           (unsigned long long)tot.emitted, (unsigned long long)tot.ref, (unsigned long long)tot.alt, (unsigned long long)tot.del,
           (unsigned long long)tot.ambiguous, (unsigned long long)tot.low_depth, (unsigned long long)tot.no_call,
           (unsigned long long)tot.ins_skipped, (unsigned long long)kept, blocks_used);
    if (verbose) {
        printf("consensus: %llu text bytes, exclude flags 0x%x, min depth %u, call fraction %u ppm, line width %u, flags %u, edits per read %u\n",
               (unsigned long long)total, exclude, min_depth, call_ppm, line_width, flags, edits_per_read ? edits_per_read : CBC_EDITS_PER_READ);
        printf("time: read + plan %.3f s, device init + reference upload %.3f s, decode + consensus + write %.3f s\n", r.t1 - r.t0, r.t_init, r.t_dev);
        if (r.used) printf("kernels: edits decode %.3f ms, mark + events %.3f ms, scans %.3f ms, text %.3f ms\n", ms[0], ms[1], ms[2], ms[3]);
    }
    status = 0;
done:
    if (fo) { fclose(fo); remove(out); }                /* a failed call leaves no partial record file behind */
    free(text);
    cli_close(&r);
    return status;
}

/* `cbc -d|-x ... --region A --region B ... [--regions-file FILE]`: the union of the loci in one pass.
 * The target set and its blocks come from cbc_unpack_targets; reads and SAM are one call over the selected blocks of all
 * contigs, the depth one call per contig that has intervals and blocks, the texts appended in contig-table order. */
int cbc_cli_decompress_targets(const char *in, const char *out, const char *ref, int device, const char *const *regions, uint32_t n_regions,
                               const char *bed_path, uint32_t output, uint32_t exclude, int verbose)
{
    const int depth = output == CBC_TARGETS_DEPTH, sam = output == CBC_TARGETS_SAM;
    cli_run r;
    if (cli_open(&r, in, ref, bed_path, device, bed_path ? "--regions-file" : depth ? "--depth" : sam ? "--sam" : "--region", "has no block index")) return 1;
    const cbc_unpack_plan *u = r.u;
    char err[512];
    cbc_targets *T = NULL;
    int rc = cbc_unpack_targets(u, regions, n_regions, r.bed, r.bed_len, &T, err, sizeof err);
    if (rc) { fprintf(stderr, "cbc: %s\n", rc == CBC_E_INPUT && err[0] ? err : "target selection failed"); return 1; }
    const int64_t hdr = sam ? cbc_unpack_sam_header(u, NULL, 0, err, sizeof err) : 0;
    if (hdr < 0) { fprintf(stderr, "cbc: %s\n", err); return 1; }
    const uint32_t nb = T->n_blocks;
    cbc_dec_block_desc *bl; uint64_t *ws; uint32_t *bc;
    if (cli_gather(u, T->blocks, nb, &bl, &ws, &bc)) return 1;
    /* --depth --skip-deletions: the bound is a line per position of the intervals; the buffer starts at 64 MiB + 64 bytes per read,
     * and a call whose text does not fit is made once more with exactly its size (as decompress_window does) */
    const int capped = depth && g_skip_edits;
    uint64_t cap = 0, bound = 0;
    if (depth) {
        for (uint32_t c = 0; c < u->n_contigs; c++) {
            const uint64_t x = capped ? cbc_unpack_targets_depth_skipdel_cap(u, T, c) : cbc_unpack_targets_depth_cap(u, T, c);
            if (x > cap) cap = x;
        }
    } else cap = cbc_unpack_targets_text_cap(u, T, sam);
    bound = cap;
    if (capped) {
        uint64_t first = 64ull << 20;
        for (uint32_t k = 0; k < nb; k++) first += 64ull * bl[k].n_reads;
        if (first < cap) cap = first;
    }
    char *text = (char *)malloc((size_t)hdr + (size_t)cap + 1);
    if (!text || (hdr && cbc_unpack_sam_header(u, text, (uint64_t)hdr, err, sizeof err) != hdr)) { fprintf(stderr, "cbc: out of memory\n"); return 1; }
    r.t1 = now2();
    FILE *fo = fopen(out, "wb");
    if (!fo || (hdr && fwrite(text, 1, (size_t)hdr, fo) != (size_t)hdr)) return cannot_write(out);
    uint64_t total = 0, reads = 0, runs = 0;
    float ms[4] = { 0, 0, 0, 0 }, m[4];
    const uint32_t n_calls = !nb ? 0u : depth ? u->n_contigs : 1u;
    for (uint32_t k = 0; k < n_calls; k++) {
        const uint32_t k0 = depth ? T->contig_blk_first[k] : 0u, kn = depth ? T->contig_blk_count[k] : nb;
        if (!kn) continue;                              /* no block can hold a read of the contig's intervals */
        if (cli_device(&r)) return 1;
        const double b = now2();
        const cbc_gpu_targets g = { (const uint32_t *)T->iv, T->block_iv + 2 * (size_t)k0, T->n_iv, T->smax };
        uint64_t tb = 0, nr = 0, nn = 0;
        for (int attempt = 0; attempt < (capped ? 2 : 1); attempt++) {
            rc = cbc_gpu_decode_targets(r.ctx, u->payloads, u->payload_bytes, bl + k0, kn, &u->caps, ws + k0, bc + k0, u->names, u->names_bytes,
                                        u->contig_name_off, u->n_contigs, &g, output, exclude, (uint8_t *)text, cap, &tb, &nr, &nn, NULL);
            if (!(rc == CBC_E_ARG && tb > cap && tb <= bound)) break;
            cap = tb;                                   /* the text's own size; no header in front of a depth text */
            char *t2 = (char *)realloc(text, (size_t)cap + 1);
            if (!t2) { fprintf(stderr, "cbc: out of memory\n"); return 1; }
            text = t2;
        }
        if (rc) { fprintf(stderr, "cbc: targets decode failed: %s\n", cbc_gpu_last_error(r.ctx)); return 1; }
        r.t_dev += now2() - b;
        if (verbose && cbc_gpu_last_targets_ms(r.ctx, &m[0], &m[1], &m[2], &m[3]) == 0) add_ms(ms, m, 4);
        if (tb && fwrite(text, 1, (size_t)tb, fo) != (size_t)tb) return cannot_write(out);
        total += tb; reads += nr; runs += nn;
    }
    if (fclose(fo) != 0) return cannot_write(out);
    if (depth)
        printf("depth of %u intervals: %llu runs from %llu reads in %u of %u blocks\n", T->n_iv, (unsigned long long)runs,
               (unsigned long long)reads, nb, u->n_blocks);
    else printf("%llu reads in %u intervals %s from %u of %u blocks\n", (unsigned long long)reads, T->n_iv,
                sam ? "written as SAM" : "decompressed", nb, u->n_blocks);
    if (verbose) {
        printf("targets: %llu regions and BED lines taken, %u intervals after merging, %llu BED lines selected nothing, %llu text bytes, span bound %u\n",
               (unsigned long long)T->n_input, T->n_iv, (unsigned long long)T->bed_unselected, (unsigned long long)total, T->smax);
        printf("time: read + plan + select %.3f s, device init + reference upload %.3f s, decode + text + write %.3f s\n", r.t1 - r.t0, r.t_init, r.t_dev);
        if (r.used) printf("kernels: decode %.3f ms, %s %.3f ms, scan + compact %.3f ms, text %.3f ms\n", ms[0],
                           depth ? "mark" : "filter + scan", ms[1], ms[2], ms[3]);
    }
    free(text); free(bl); free(ws); free(bc);
    cbc_targets_free(T);
    cli_close(&r);
    return 0;
}

/* `cbc -d|-x ... --bedcov [--region A ...] [--regions-file FILE] [--window N] [--min-depth D]`: one line per query -- per
 * --region, per BED line (unmerged, in input order), per contig when neither is given, or per window of those -- with the sum
 * of the depth, the positions with depth >= D and the mean.  The numbers come from one
 * cbc_gpu_decode_coverage per contig that has intervals and blocks; the text is formatted here, so that it comes out in input
 * order across contigs.  12 bytes per query cross PCIe.
 * `--thresholds T1,..` / `--count-reads`: n_thr more columns, the positions with depth >= Ti, and one
 * last column, the kept reads with a base in the query, from cbc_gpu_decode_coverage_ext; with neither (n_thr == 0 and
 * !count_reads), the call, the kernels, the bytes and the messages are those of the plain summary.
 * `--quantiles P1,..`: n_pct more columns behind the thresholds' and in front of the read count, the
 * nearest-rank depth quantiles of the query's positions, from cbc_gpu_decode_coverage_quant; without it nothing changes. */
int cbc_cli_decompress_bedcov(const char *in, const char *out, const char *ref, int device, const char *const *regions, uint32_t n_regions,
                              const char *bed_path, uint64_t window, uint32_t min_depth, uint32_t exclude, int verbose,
                              const uint32_t *thr, uint32_t n_thr, int count_reads, const uint32_t *pct, uint32_t n_pct)
{
    const int ext = n_thr || count_reads || n_pct;
    cli_run r;
    if (cli_open(&r, in, ref, bed_path, device, "--bedcov", "has no block index")) return 1;
    const cbc_unpack_plan *u = r.u;
    char err[512];
    cbc_queries *Q = NULL;
    int rc = cbc_unpack_queries(u, regions, n_regions, r.bed, r.bed_len, window, &Q, err, sizeof err);
    if (rc) { fprintf(stderr, "cbc: --bedcov: %s\n", rc == CBC_E_INPUT && err[0] ? err : "query selection failed"); return 1; }
    const cbc_targets *T = Q->targets;
    const uint64_t nq = Q->n_q;
    const uint32_t nb = T->n_blocks, nc = u->n_contigs;
    cbc_dec_block_desc *bl; uint64_t *ws; uint32_t *bc;
    if (cli_gather(u, T->blocks, nb, &bl, &ws, &bc)) return 1;
    uint64_t *sum = (uint64_t *)calloc((size_t)(nq ? nq : 1), 8), *csum = (uint64_t *)malloc((size_t)(nq ? nq : 1) * 8);
    uint32_t *cov = (uint32_t *)calloc((size_t)(nq ? nq : 1), 4), *ccov = (uint32_t *)malloc((size_t)(nq ? nq : 1) * 4);
    uint32_t *qq = (uint32_t *)malloc((size_t)(nq ? nq : 1) * 8), *qi = (uint32_t *)malloc((size_t)(nq ? nq : 1) * 4);
    uint64_t *cfirst = (uint64_t *)calloc((size_t)nc + 2, 8);
    /* the extra columns, gathered and scattered per contig like sum and covered */
    uint32_t *xthr = (uint32_t *)calloc((size_t)(nq ? nq : 1) * (n_thr ? n_thr : 1), 4), *cthr = (uint32_t *)malloc((size_t)(nq ? nq : 1) * (n_thr ? n_thr : 1) * 4);
    uint32_t *xrd = (uint32_t *)calloc((size_t)(nq ? nq : 1), 4), *crd = (uint32_t *)malloc((size_t)(nq ? nq : 1) * 4);
    uint32_t *xqd = (uint32_t *)calloc((size_t)(nq ? nq : 1) * (n_pct ? n_pct : 1), 4), *cqd = (uint32_t *)malloc((size_t)(nq ? nq : 1) * (n_pct ? n_pct : 1) * 4);
    if (!sum || !csum || !cov || !ccov || !qq || !qi || !cfirst || !xthr || !cthr || !xrd || !crd || !xqd || !cqd) { fprintf(stderr, "cbc: out of memory\n"); return 1; }
    /* the queries that hold a position, grouped per contig (a counting sort: the order inside a contig stays the input's) */
    for (uint64_t i = 0; i < nq; i++) if (Q->q[i].contig != CBC_QUERY_UNKNOWN && Q->q[i].end0 > Q->q[i].start0) cfirst[Q->q[i].contig + 2]++;
    for (uint32_t c = 0; c < nc; c++) cfirst[c + 2] += cfirst[c + 1];
    for (uint64_t i = 0; i < nq; i++) {
        const cbc_query *x = &Q->q[i];
        if (x->contig == CBC_QUERY_UNKNOWN || x->end0 == x->start0) continue;
        const uint64_t at = cfirst[x->contig + 1]++;
        qq[2 * at] = x->slot; qq[2 * at + 1] = x->end + 1u - x->beg; qi[at] = (uint32_t)i;
    }                                                    /* now cfirst[c] .. cfirst[c + 1]: contig c's part */
    r.t1 = now2();
    uint64_t reads = 0;
    uint32_t blocks_used = 0;
    float ms[7] = { 0, 0, 0, 0, 0, 0, 0 }, xms[5] = { 0, 0, 0, 0, 0 }, m[7], xm[5], qms = 0, qm;
    for (uint32_t c = 0; c < nc && nb; c++) {
        const uint32_t k0 = T->contig_blk_first[c], kn = T->contig_blk_count[c];
        const uint64_t q0 = cfirst[c], qn = cfirst[c + 1] - cfirst[c];
        if (!kn || !qn || !T->contig_count[c]) continue;   /* no block can hold a read of the contig's intervals: zeros */
        if (cli_device(&r)) return 1;
        const double b = now2();
        const cbc_gpu_targets g = { (const uint32_t *)T->iv, T->block_iv + 2 * (size_t)k0, T->n_iv, T->smax };
        uint64_t nr = 0;
        if (n_pct)
            rc = cbc_gpu_decode_coverage_quant(r.ctx, u->payloads, u->payload_bytes, bl + k0, kn, &u->caps, ws + k0, bc + k0, u->names, u->names_bytes,
                                               u->contig_name_off, u->n_contigs, &g, T->contig_first[c], T->contig_count[c], qq + 2 * q0,
                                               (uint32_t)qn, exclude, min_depth, csum + q0, ccov + q0, &nr, NULL, thr, n_thr,
                                               cthr + q0 * n_thr, count_reads ? crd + q0 : NULL, pct, n_pct, cqd + q0 * n_pct);
        else if (ext)
            rc = cbc_gpu_decode_coverage_ext(r.ctx, u->payloads, u->payload_bytes, bl + k0, kn, &u->caps, ws + k0, bc + k0, u->names, u->names_bytes,
                                             u->contig_name_off, u->n_contigs, &g, T->contig_first[c], T->contig_count[c], qq + 2 * q0,
                                             (uint32_t)qn, exclude, min_depth, csum + q0, ccov + q0, &nr, NULL, thr, n_thr,
                                             cthr + q0 * n_thr, count_reads ? crd + q0 : NULL);
        else
            rc = cbc_gpu_decode_coverage(r.ctx, u->payloads, u->payload_bytes, bl + k0, kn, &u->caps, ws + k0, bc + k0, u->names, u->names_bytes,
                                         u->contig_name_off, u->n_contigs, &g, T->contig_first[c], T->contig_count[c], qq + 2 * q0,
                                         (uint32_t)qn, exclude, min_depth, csum + q0, ccov + q0, &nr, NULL);
        if (rc) { fprintf(stderr, "cbc: coverage failed: %s\n", cbc_gpu_last_error(r.ctx)); return 1; }
        r.t_dev += now2() - b;
        if (verbose && n_pct) { if (cbc_gpu_last_coverage_quant_ms(r.ctx, m, xm, &qm) == 0) { add_ms(ms, m, 7); add_ms(xms, xm, 5); qms += qm; } }
        else if (verbose && ext) { if (cbc_gpu_last_coverage_ext_ms(r.ctx, m, xm) == 0) { add_ms(ms, m, 7); add_ms(xms, xm, 5); } }
        else if (verbose && cbc_gpu_last_coverage_ms(r.ctx, &m[0], &m[1], &m[2], &m[3], &m[4], &m[5], &m[6]) == 0) add_ms(ms, m, 7);
        for (uint64_t k = q0; k < q0 + qn; k++) { sum[qi[k]] = csum[k]; cov[qi[k]] = ccov[k]; }
        for (uint64_t k = q0; ext && k < q0 + qn; k++) {
            for (uint32_t t = 0; t < n_thr; t++) xthr[(size_t)qi[k] * n_thr + t] = cthr[k * n_thr + t];
            if (count_reads) xrd[qi[k]] = crd[k];
            for (uint32_t t = 0; t < n_pct; t++) xqd[(size_t)qi[k] * n_pct + t] = cqd[k * n_pct + t];
        }
        reads += nr; blocks_used += kn;
    }
    const double t2 = now2();
    FILE *fo = fopen(out, "wb");
    if (!fo) return cannot_write(out);
    for (uint64_t i = 0; i < nq; i++) {
        const cbc_query *x = &Q->q[i];
        char mean[32];
        (void)cbc_coverage_mean(sum[i], x->end0 - x->start0, mean);
        const char *nm = x->contig == CBC_QUERY_UNKNOWN ? r.bed + x->name_off : u->names + u->contig_name_off[x->contig];
        const int nl = x->contig == CBC_QUERY_UNKNOWN ? (int)x->name_len : (int)strlen(nm);
        int bad = fprintf(fo, "%.*s\t%llu\t%llu\t%llu\t%u\t%s", nl, nm, (unsigned long long)x->start0, (unsigned long long)x->end0,
                          (unsigned long long)sum[i], cov[i], mean) < 0;
        for (uint32_t t = 0; t < n_thr && !bad; t++) bad = fprintf(fo, "\t%u", xthr[(size_t)i * n_thr + t]) < 0;
        for (uint32_t t = 0; t < n_pct && !bad; t++) bad = fprintf(fo, "\t%u", xqd[(size_t)i * n_pct + t]) < 0;
        if (count_reads && !bad) bad = fprintf(fo, "\t%u", xrd[i]) < 0;
        if (bad || fputc('\n', fo) == EOF) return cannot_write(out);
    }
    if (fclose(fo) != 0) return cannot_write(out);
    printf("coverage of %llu queries from %llu reads in %u of %u blocks\n", (unsigned long long)nq, (unsigned long long)reads, blocks_used, u->n_blocks);
    if (verbose) {
        printf("bedcov: %llu queries, %u intervals after merging, %u blocks selected, %llu BED lines selected nothing, window %llu, min depth %u, exclude flags 0x%x\n",
               (unsigned long long)nq, T->n_iv, nb, (unsigned long long)T->bed_unselected, (unsigned long long)window, min_depth, exclude);
        printf("time: read + plan + select %.3f s, device init + reference upload %.3f s, decode + coverage %.3f s, format + write %.3f s\n",
               r.t1 - r.t0, r.t_init, r.t_dev, now2() - t2);
        if (r.used) printf("kernels: decode %.3f ms, mark %.3f ms, scan + compact %.3f ms, weights %.3f ms, weight scans %.3f ms, prefixes %.3f ms, lookup %.3f ms\n",
                           ms[0], ms[1], ms[2], ms[3], ms[4], ms[5], ms[6]);
        if (r.used && ext) printf("kernels: start points %.3f ms, threshold weights %.3f ms, their scans %.3f ms, their prefixes %.3f ms, threshold + read lookup %.3f ms\n",
                                  xms[0], xms[1], xms[2], xms[3], xms[4]);
        if (r.used && n_pct) printf("kernels: quantile selection %.3f ms\n", qms);
    }
    free(xthr); free(cthr); free(xrd); free(crd); free(xqd); free(cqd);
    free(bl); free(ws); free(bc); free(sum); free(csum); free(cov); free(ccov); free(qq); free(qi); free(cfirst);
    cbc_queries_free(Q);
    cli_close(&r);
    return 0;
}

/* `cbc -d|-x ... --depth-hist [--region A ...] [--regions-file FILE] [--hist-max M]`: per contig how many positions have each
 * depth, then the same summed over the listed contigs under the name "genome" (DESIGN.md section 4.16).  Without regions every
 * contig of the table is counted whole; with them the merged intervals, every position once, and a contig is listed when an
 * interval lies on it.  The non-zero bins come from one cbc_gpu_decode_depth_hist per contig that has blocks; the depth-0 bin,
 * the genome sums and the text are made here.  A few hundred bytes per contig cross PCIe. */
typedef struct hist_bin { uint64_t depth, bases; } hist_bin;
static int hist_bin_cmp(const void *a, const void *b)
{
    const uint64_t x = ((const hist_bin *)a)->depth, y = ((const hist_bin *)b)->depth;
    return x < y ? -1 : x > y;
}
static int hist_line(FILE *fo, const char *name, uint64_t depth, uint64_t bases, uint64_t size)
{
    char fr[40];
    (void)cbc_hist_fraction(bases, size, fr);
    return fprintf(fo, "%s\t%llu\t%llu\t%llu\t%s\n", name, (unsigned long long)depth, (unsigned long long)bases, (unsigned long long)size, fr) < 0;
}

int cbc_cli_decompress_hist(const char *in, const char *out, const char *ref, int device, const char *const *regions, uint32_t n_regions,
                            const char *bed_path, uint32_t max_depth, uint32_t exclude, int verbose)
{
    cli_run r;
    if (cli_open(&r, in, ref, bed_path, device, "--depth-hist", "has no block index")) return 1;
    const cbc_unpack_plan *u = r.u;
    char err[512];
    /* the intervals and their blocks: the target set of the regions, or every contig whole (the query list's own set) */
    cbc_targets *T = NULL;
    cbc_queries *Q = NULL;
    int rc;
    if (n_regions || bed_path) rc = cbc_unpack_targets(u, regions, n_regions, r.bed, r.bed_len, &T, err, sizeof err);
    else { rc = cbc_unpack_queries(u, NULL, 0, NULL, 0, 0, &Q, err, sizeof err); if (!rc) T = Q->targets; }
    if (rc) { fprintf(stderr, "cbc: --depth-hist: %s\n", rc == CBC_E_INPUT && err[0] ? err : "target selection failed"); return 1; }
    const uint32_t nb = T->n_blocks, nc = u->n_contigs;
    cbc_dec_block_desc *bl; uint64_t *ws; uint32_t *bc;
    if (cli_gather(u, T->blocks, nb, &bl, &ws, &bc)) return 1;
    r.t1 = now2();
    FILE *fo = fopen(out, "wb");
    if (!fo) return cannot_write(out);
    hist_bin *all = NULL;                                    /* every contig's bins, for the genome block */
    size_t n_all = 0, cap_all = 0;
    uint64_t reads = 0, gsize = 0;
    uint32_t blocks_used = 0, listed = 0;
    float ms[5] = { 0, 0, 0, 0, 0 }, m[5];
    for (uint32_t c = 0; c < nc && c < T->n_contigs; c++) {
        if (!T->contig_count[c]) continue;                  /* no interval on the contig: not listed */
        const uint32_t k0 = T->contig_blk_first[c], kn = T->contig_blk_count[c];
        const uint64_t size = cbc_unpack_targets_size(T, c);
        const char *nm = u->names + u->contig_name_off[c];
        uint32_t n_bins = 0, *bd = NULL, *bb = NULL;
        if (kn) {                                           /* else no block can hold a read of the intervals: depth 0 everywhere */
            if (cli_device(&r)) return 1;
            const double b = now2();
            uint64_t k_reads = 0, nr = 0;
            for (uint32_t k = 0; k < kn; k++) k_reads += bl[k0 + k].n_reads;
            const uint64_t fold = max_depth ? max_depth : 0xffffffffull;
            const uint32_t cap = (uint32_t)(k_reads < fold ? k_reads : fold);   /* a depth cannot pass the reads */
            bd = (uint32_t *)malloc((size_t)(cap ? cap : 1) * 4); bb = (uint32_t *)malloc((size_t)(cap ? cap : 1) * 4);
            if (!bd || !bb) { fprintf(stderr, "cbc: out of memory\n"); return 1; }
            const cbc_gpu_targets g = { (const uint32_t *)T->iv, T->block_iv + 2 * (size_t)k0, T->n_iv, T->smax };
            rc = cbc_gpu_decode_depth_hist(r.ctx, u->payloads, u->payload_bytes, bl + k0, kn, &u->caps, ws + k0, bc + k0, u->names, u->names_bytes,
                                           u->contig_name_off, u->n_contigs, &g, T->contig_first[c], T->contig_count[c], exclude, max_depth,
                                           bd, bb, cap, &n_bins, &nr, NULL);
            if (rc) { fprintf(stderr, "cbc: depth histogram failed: %s\n", cbc_gpu_last_error(r.ctx)); return 1; }
            r.t_dev += now2() - b;
            if (verbose && cbc_gpu_last_hist_ms(r.ctx, &m[0], &m[1], &m[2], &m[3], &m[4]) == 0) add_ms(ms, m, 5);
            reads += nr; blocks_used += kn;
        }
        uint64_t covered = 0;
        for (uint32_t i = 0; i < n_bins; i++) covered += bb[i];
        if (covered > size) { fprintf(stderr, "cbc: depth histogram failed: the bins of %s hold more positions than its intervals\n", nm); return 1; }
        if (n_all + n_bins + 1u > cap_all) {
            cap_all = (n_all + n_bins + 1u) * 2u;
            all = (hist_bin *)realloc(all, cap_all * sizeof *all);
            if (!all) { fprintf(stderr, "cbc: out of memory\n"); return 1; }
        }
        int bad = 0;
        if (size - covered) { bad |= hist_line(fo, nm, 0, size - covered, size); all[n_all].depth = 0; all[n_all++].bases = size - covered; }
        for (uint32_t i = 0; i < n_bins; i++) { bad |= hist_line(fo, nm, bd[i], bb[i], size); all[n_all].depth = bd[i]; all[n_all++].bases = bb[i]; }
        if (bad) return cannot_write(out);
        free(bd); free(bb);
        gsize += size; listed++;
    }
    if (listed) {                                            /* the genome block: the bins summed over the listed contigs, 64 bits */
        qsort(all, n_all, sizeof *all, hist_bin_cmp);
        for (size_t i = 0; i < n_all; ) {
            uint64_t bases = 0;
            size_t j = i;
            for (; j < n_all && all[j].depth == all[i].depth; j++) bases += all[j].bases;
            if (hist_line(fo, "genome", all[i].depth, bases, gsize)) return cannot_write(out);
            i = j;
        }
    }
    if (fclose(fo) != 0) return cannot_write(out);
    printf("depth histogram of %u contigs, %llu positions, from %llu reads in %u of %u blocks\n", listed, (unsigned long long)gsize,
           (unsigned long long)reads, blocks_used, u->n_blocks);
    if (verbose) {
        printf("depth-hist: %u intervals after merging, %u blocks selected, %llu BED lines selected nothing, fold at %u, exclude flags 0x%x\n",
               T->n_iv, nb, (unsigned long long)T->bed_unselected, max_depth, exclude);
        printf("time: read + plan + select %.3f s, device init + reference upload %.3f s, decode + histogram + write %.3f s\n", r.t1 - r.t0, r.t_init, r.t_dev);
        if (r.used) printf("kernels: decode %.3f ms, mark %.3f ms, scan + compact %.3f ms, zero + accumulate %.3f ms, bin compaction %.3f ms\n",
                           ms[0], ms[1], ms[2], ms[3], ms[4]);
    }
    free(all); free(bl); free(ws); free(bc);
    if (Q) cbc_queries_free(Q); else cbc_targets_free(T);
    cli_close(&r);
    return 0;
}

/* `cbc -d|-x ... --stats [--region A ...] [--regions-file FILE] [--stats-exclude-flags N]`: the tables of a first look at the reads
 *  instead of the reads.  Without regions every block is decoded by the plain decoder; with them the
 * selected blocks of the target set by the span decoder, each selected read counted once.  One cbc_gpu_decode_stats; the tables
 * (about 270 KB) cross PCIe and cbc_stats_text makes the text.
 * alignment (--alignment): one cbc_gpu_decode_stats_aln instead -- the edits decoder against the
 * container's span bound or the target set's, with an arena of edits_per_read entries per read (0: the default) -- and the
 * sections of cbc_stats_aln_text behind the same text. */
int cbc_cli_decompress_stats(const char *in, const char *out, const char *ref, int device, const char *const *regions, uint32_t n_regions,
                             const char *bed_path, uint32_t exclude, int alignment, uint32_t edits_per_read, int verbose)
{
    cli_run r;
    if (cli_open(&r, in, ref, bed_path, device, "--stats", "has no block index")) return 1;
    const cbc_unpack_plan *u = r.u;
    char err[512];
    /* what SAM output refuses, the statistics refuse: a long-read container, names and lengths the coordinates cannot carry */
    if (cbc_unpack_sam_header(u, NULL, 0, err, sizeof err) < 0) { fprintf(stderr, "cbc: --stats: %s\n", err[0] ? err : "the contig table is not usable"); return 1; }
    cbc_targets *T = NULL;                                   /* NULL: the whole file */
    int rc = n_regions || bed_path ? cbc_unpack_targets(u, regions, n_regions, r.bed, r.bed_len, &T, err, sizeof err) : 0;
    if (rc) { fprintf(stderr, "cbc: --stats: %s\n", rc == CBC_E_INPUT && err[0] ? err : "target selection failed"); return 1; }
    const uint32_t nb = T ? T->n_blocks : u->n_blocks;
    cbc_dec_block_desc *bl; uint64_t *ws;
    cbc_gpu_stats *st = (cbc_gpu_stats *)calloc(1, sizeof *st);
    cbc_gpu_stats_aln *al = (cbc_gpu_stats_aln *)calloc(1, sizeof *al);
    const uint64_t cap = cbc_stats_text_cap(), acap = alignment ? cbc_stats_aln_text_cap() : 0u;
    char *text = (char *)malloc((size_t)(cap + acap));
    if (!st || !al || !text) { fprintf(stderr, "cbc: out of memory\n"); return 1; }
    if (cli_gather(u, T ? T->blocks : NULL, nb, &bl, &ws, NULL)) return 1;
    r.t1 = now2();
    float ms[3] = { 0, 0, 0 };
    if (nb) {                                                /* else nothing runs: all-zero tables */
        if (cli_device(&r)) return 1;
        const double b = now2();
        const cbc_gpu_targets gt = { T ? (const uint32_t *)T->iv : NULL, T ? T->block_iv : NULL, T ? T->n_iv : 0u, T ? T->smax : 0u };
        if (alignment)
            rc = cbc_gpu_decode_stats_aln(r.ctx, u->payloads, u->payload_bytes, bl, nb, &u->caps, ws, T ? &gt : NULL,
                                          u->max_read_len + u->read_length - 1u, exclude, edits_per_read, st, al, NULL);
        else rc = cbc_gpu_decode_stats(r.ctx, u->payloads, u->payload_bytes, bl, nb, &u->caps, ws, T ? &gt : NULL, exclude, st, NULL);
        if (rc) { fprintf(stderr, "cbc: statistics failed: %s\n", cbc_gpu_last_error(r.ctx)); return 1; }
        r.t_dev = now2() - b;
        if (verbose && alignment) (void)cbc_gpu_last_stats_aln_ms(r.ctx, &ms[0], &ms[1], &ms[2]);
        else if (verbose) (void)cbc_gpu_last_stats_ms(r.ctx, &ms[0], &ms[1]);
    }
    int64_t n = cbc_stats_text(st, text, cap);
    if (n >= 0 && alignment) {
        const int64_t m = cbc_stats_aln_text(al, text + n, acap);
        n = m < 0 ? m : n + m;
    }
    FILE *fo = n < 0 ? NULL : fopen(out, "wb");
    if (!fo || fwrite(text, 1, (size_t)n, fo) != (size_t)n || fclose(fo) != 0) return cannot_write(out);
    printf("statistics of %llu reads (%llu excluded) from %u of %u blocks\n", (unsigned long long)st->reads, (unsigned long long)st->excluded, nb, u->n_blocks);
    if (verbose) {
        if (T) printf("stats: %u intervals after merging, %u blocks selected, %llu BED lines selected nothing, exclude flags 0x%x\n",
                      T->n_iv, nb, (unsigned long long)T->bed_unselected, exclude);
        else printf("stats: the whole file, exclude flags 0x%x\n", exclude);
        printf("time: read + plan + select %.3f s, device init + reference upload %.3f s, decode + statistics %.3f s\n", r.t1 - r.t0, r.t_init, r.t_dev);
        if (alignment) printf("alignment: %llu reads, %llu without alignment\n", (unsigned long long)al->reads, (unsigned long long)al->invalid);
        if (r.used && alignment) printf("kernels: edits decode %.3f ms, statistics %.3f ms, alignment %.3f ms\n", ms[0], ms[1], ms[2]);
        else if (r.used) printf("kernels: decode %.3f ms, statistics %.3f ms\n", ms[0], ms[1]);
    }
    free(text); free(st); free(al); free(bl); free(ws);
    if (T) cbc_targets_free(T);
    cli_close(&r);
    return 0;
}
