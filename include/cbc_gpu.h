/*
 * cbc_gpu.h -- C ABI of the MI355X-native cbc hot path (libcbc_gpu.so, built from cbc_amd/csrc).
 *
 * The reference (1mishra/cbc) has no plugin/FFI seam: its hot path sits behind a CLI and a file
 * format.  The entry points below are what a maintainer would bind in
 * place of the per-file encode loop
 *      compress()              src/compression.c:112-170
 *        compress_line()       src/compression.c:42-69
 *          compress_rname()    src/id_compression.c:39-65
 *          compress_read()     src/read_compression.c:15-44   (pos/flag/match/edits/var/chars)
 *            send_value_to_as  src/stream_model.c:53-76  + update_model :31-51
 *            arithmetic_encoder_step  src/Arithmetic_stream.c:274-345
 *        encoder_last_step()   src/Arithmetic_stream.c:348-371
 * operating on *packed* records (the output of the load_sam_line() tokeniser,
 * src/sam_file_allocation.c:437-529) instead of SAM text.
 *
 * Unit of work: a BLOCK = up to N consecutive records of one contig, with POS rebased so that
 * the block's first record has POS 1.  The payload produced for a block is byte-identical to the
 * file the reference encoder (built with -DDEBUG, i.e. constant WELL seed) writes when it is run
 * on that block alone: a SAM holding just those records with the rebased POS and a one-contig
 * FASTA holding the reference window that starts at the block's first base.  One block is one
 * independent arithmetic stream, coded by one workgroup (encode: a model wavefront feeding a coder
 * wavefront through LDS; decode: one wavefront).
 *
 * Plain C: pointers and sizes only, caller owns every buffer, no global state, every function
 * returns 0 on success or a negative CBC_E_* code.  One host thread per context.
 */
#ifndef CBC_GPU_H
#define CBC_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CBC_ABI_VERSION 1

/* ---- error / status codes ---------------------------------------------------------------- */
#define CBC_OK              0
#define CBC_E_ARG          -1   /* bad argument                                                */
#define CBC_E_NODEV        -2   /* no HIP device / HIP runtime error (see cbc_gpu_last_error)   */
#define CBC_E_NOMEM        -3
#define CBC_E_BLOCK        -4   /* at least one block finished with status != CBC_ST_OK         */
#define CBC_E_INPUT        -5   /* input violates a reference limit (message in last_error)     */
#define CBC_E_IO           -6

/* per-block status written by the kernel (cbc_block_result.status) */
#define CBC_ST_OK           0
#define CBC_ST_OUT_FULL     1   /* out_cap too small                                            */
#define CBC_ST_ASSERT       2   /* the reference would abort here: zero-count symbol, symbol >= */
                                /* alphabet, unsorted POS, var context >= 65535 ...             */
#define CBC_ST_CAP_POS      3   /* more distinct POS deltas than lds.cap_pos                    */
#define CBC_ST_CAP_FLAG     4   /* more than CBC_CAP_FLAG distinct FLAG values                  */
#define CBC_ST_CAP_VAR      5   /* more var symbols than lds.cap_var.  Counted are the symbols  */
                                /* that take a list entry: not those held in the LDS buckets,   */
                                /* and, in the block encode kernel of five wavefronts per SIMD, */
                                /* not those of the context "first edit of a full-length read,  */
                                /* no known SNP ahead" (d = read_length + 2), which it keeps as */
                                /* counts in registers -- with a cap_var below the packer's a    */
                                /* block may be coded (same bytes) that stopped here before     */
#define CBC_ST_CAP_NAME     6   /* contig name longer than CBC_CAP_NAME-3                       */
#define CBC_ST_UNSUPPORTED  7   /* raw leading-S / '*' op in the tokens (the packer emits a leading  */
                                /* soft clip as an I op after rebuilding MD, quirk Q6); a block    */
                                /* of more than CBC_MAX_BLOCK_READS records; a LOSSY stream         */
#define CBC_ST_SPAN         8   /* region decode: a read covers more reference bases than the bound */
                                /* the block selection assumed (cbc_gpu_decode_region, smax)        */
#define CBC_ST_EDITS        9   /* edit-reporting decode: the block's reads with indels hold more   */
                                /* deleted and inserted bases than its arena (edits_per_read)       */

/* ---- packed record layout (device and host share it) ---------------------------------------- */

/* One per mapped record, 16 bytes, array-of-structs so a wavefront loads 64 records with one
 * 16-byte-per-lane coalesced access.  Mirrors struct read_line_t (include/sam_block.h:177-185). */
typedef struct cbc_read_rec {
    uint32_t pos;       /* POS, 1-based, relative to the block's reference window               */
    uint16_t flag;      /* SAM FLAG (read_line_t.invFlag)                                       */
    uint16_t rlen;      /* strlen(SEQ), <= CBC_MAX_READ_LEN                                     */
    uint32_t seq_off;   /* byte offset of SEQ in seq[], relative to the block's seq_base        */
    uint32_t tok_off;   /* word offset of the CIGAR/MD tokens in tok[], relative to tok_base    */
} cbc_read_rec;

/* Token stream of one record at tok[tok_base + tok_off]:
 *   word 0            : n_cigar | (n_md << 16)
 *   word 1            : n_deleted_bases | (n_inserted_bases << 16)   (sum of D lengths; sum of I and
 *                       trailing-S lengths) -- the counts compress_edits() codes first (:557-565);
 *                       the number of SNPs is n_md (the packer rejects MD strings that are
 *                       inconsistent with the read)
 *   n_cigar words     : (len << 4) | op      op: CBC_OP_M/I/D/S/STAR; len = atoi() of the CIGAR
 *                       segment exactly as compress_edits() reads it (read_compression.c:308-352)
 *   n_md words        : (gap << 8) | letter  one per mismatch letter of MD:Z, gap = matched bases
 *                       since the previous mismatch (numbers on both sides of a '^' run add up,
 *                       add_snps_to_array read_compression.c:613-701); letter is the raw byte,
 *                       so the trailing '\n' of an MD that is the last column survives (quirk Q2)
 */
#define CBC_OP_M    0u
#define CBC_OP_I    1u
#define CBC_OP_D    2u
#define CBC_OP_S    3u
#define CBC_OP_STAR 4u

/* One per block, 64 bytes. */
typedef struct cbc_block_desc {
    uint64_t rec_base;     /* index of the block's first cbc_read_rec                           */
    uint64_t seq_base;     /* byte offset of the block's bases in seq[]                         */
    uint64_t tok_base;     /* word offset of the block's tokens in tok[]                        */
    uint64_t ref_off;      /* byte offset in the device reference of the base that is POS 1     */
    uint64_t out_off;      /* byte offset of this block's payload area in out[] (4-aligned)     */
    uint32_t out_cap;      /* bytes available at out_off (multiple of 256)                      */
    uint32_t n_reads;
    uint32_t name_off;     /* offset in names[] of the NUL-terminated contig name               */
    uint32_t read_length;  /* header read length L0 (get_read_length, sam_file_allocation.c:26) */
    uint32_t n_tok;        /* words of tok[] owned by this block (bounds the token prefetch)    */
    uint32_t reserved;     /* set by cbc_gpu_plan_output: bytes of the out area that are payload; */
                           /* the rest, up to out_cap, holds the block's var-event list          */
} cbc_block_desc;

typedef struct cbc_block_result {
    uint32_t nbytes;       /* payload bytes written at out_off                                  */
    uint32_t status;       /* CBC_ST_*                                                          */
    uint32_t n_symbols;    /* arithmetic-coder steps taken                                      */
    uint32_t fail_read;    /* block-local index of the record being coded when status was set   */
} cbc_block_result;

/* limits of the LDS-resident model tables; the packer cuts blocks so that they hold */
#define CBC_MAX_READ_LEN   252u    /* var context (((L+2)<<7)+L)*2+1 must stay < 65535 (sam_models.c:317) */
#define CBC_CAP_FLAG       64u     /* distinct FLAG values per block                              */
#define CBC_CAP_NAME       128u    /* (context,char) pairs of the contig-name model               */
#define CBC_MAX_BLOCK_READS 16384u /* keeps every adaptive total below the 2^20 rescale point     */
#define CBC_REF_PAD        512u    /* zero bytes the caller appends after every contig            */
#define CBC_WELL_SEED      0x55555555u  /* sam_file_allocation.c:399, the -DDEBUG constant         */

typedef struct cbc_lds_caps {
    uint32_t cap_pos;      /* entries of the POS-delta alphabet in LDS (>= max distinct deltas + 1) */
    uint32_t cap_var;      /* var symbols per block: sizes the event list, which lives in global    */
                           /* memory (behind the payload area on encode, in d_var_scratch on decode) */
} cbc_lds_caps;

/* ---- context ------------------------------------------------------------------------------------ */
typedef struct cbc_gpu_ctx cbc_gpu_ctx;

int  cbc_gpu_abi_version(void);
int  cbc_gpu_device_count(void);
int  cbc_gpu_init(int device_ordinal, cbc_gpu_ctx **ctx);
int  cbc_gpu_shutdown(cbc_gpu_ctx *ctx);
const char *cbc_gpu_last_error(cbc_gpu_ctx *ctx);

/* Upload the reference the blocks' ref_off point into: upper-cased contig bases, one byte per
 * base, each contig followed by CBC_REF_PAD zero bytes (what store_reference_in_memory,
 * src/read_decompression.c:17-53, keeps in `reference[]`, for all contigs at once). */
int  cbc_gpu_upload_reference(cbc_gpu_ctx *ctx, const uint8_t *bases, uint64_t nbytes);
/* The same from several host pieces, laid end to end on the device in the order given (piece k starts at the sum of the
 * sizes before it): a device that codes some contigs of a genome uploads those contigs, not all of it. */
int  cbc_gpu_upload_reference_parts(cbc_gpu_ctx *ctx, const uint8_t *const *parts, const uint64_t *bytes, uint32_t n_parts);

/* Host-buffer entry point: copies the batch to the device, codes every block, copies the payloads
 * back *compacted*: block b's payload is out[out_offsets[b] .. out_offsets[b+1]).  `blocks[].out_off`
 * and `.out_cap` are filled in by the library.  results may be NULL. */
typedef struct cbc_host_batch {
    const cbc_read_rec   *recs;   uint64_t n_recs;
    const uint8_t        *seq;    uint64_t seq_bytes;
    const uint32_t       *tok;    uint64_t n_tok;
    const uint8_t        *names;  uint32_t names_bytes;
    cbc_block_desc       *blocks; uint32_t n_blocks;
    cbc_lds_caps          caps;
} cbc_host_batch;

int  cbc_gpu_encode_blocks(cbc_gpu_ctx *ctx, const cbc_host_batch *batch,
                           uint8_t *out, uint64_t out_cap, uint64_t *out_offsets /* n_blocks+1 */,
                           cbc_block_result *results /* n_blocks or NULL */);

/* The host-buffer entry points run as a pipeline (chunked H2D on a copy stream overlapped with the launches of the chunks
 * already on the device; device arrays kept in the context between calls).  What the most recent one did: */
typedef struct cbc_e2e_times {
    double   total_s;        /* whole call                                                                  */
    double   alloc_s;        /* growing the context's device arenas (0 once they have their size)           */
    double   issue_s;        /* until the last chunk's copies and launch had been handed to the runtime     */
    double   kernels_done_s; /* until every block had been coded and the sizes were on the host            */
    uint64_t h2d_bytes, d2h_bytes;
    uint32_t n_chunks, reserved;
} cbc_e2e_times;
int  cbc_gpu_last_e2e(cbc_gpu_ctx *ctx, cbc_e2e_times *out);
/* Page-lock caller-owned host memory the entry points read from or write to (hipHostRegister): DMA then runs at the link
 * rate and asynchronously.  Worth it for buffers that are reused; the entry points accept pageable memory as well. */
int  cbc_gpu_host_register(cbc_gpu_ctx *ctx, const void *p, uint64_t bytes);
int  cbc_gpu_host_unregister(cbc_gpu_ctx *ctx, const void *p);

/* ---- several devices in one process: the exchange step -------------------------------------------
 * cbc_gpu_encode_blocks (and _2bit / _tokenised) with out == NULL keep the compacted bitstreams ON THE DEVICE, appended to the
 * context's stash (out_offsets are relative to the call, as always).  A group over one context per device then moves every
 * member's stash to member 0's device with grouped ncclSend / ncclRecv (RCCL over xGMI), checks a checksum taken on the
 * sending device against one taken on the receiving device, and hands the bytes to the host in member order.  librccl.so is
 * loaded when the first group is created.  A one-member group sends to itself (self-test of the call sites).
 * Without RCCL (or with two contexts on one device) cbc_gpu_stash_fetch() brings a member's stash back over PCIe instead. */
typedef struct cbc_gpu_group cbc_gpu_group;
int  cbc_gpu_group_create(cbc_gpu_ctx *const *ctxs, int n, cbc_gpu_group **out);       /* CBC_E_ARG when two contexts share a device */
int  cbc_gpu_group_gather(cbc_gpu_group *g, uint8_t *out, uint64_t out_cap, uint64_t *nbytes /* n */, uint64_t *sums /* n or NULL */);
void cbc_gpu_group_destroy(cbc_gpu_group *g);
const char *cbc_gpu_group_last_error(cbc_gpu_group *g);
int  cbc_gpu_stash_reset(cbc_gpu_ctx *ctx);
uint64_t cbc_gpu_stash_bytes(cbc_gpu_ctx *ctx);
int  cbc_gpu_stash_fetch(cbc_gpu_ctx *ctx, uint8_t *out, uint64_t out_cap);

/* Device-pointer entry point (what bench.py and the multi-GPU host use): every pointer is a
 * device address, the launch is asynchronous on `hip_stream`, a hipStream_t used exactly as given
 * (NULL is HIP's null stream, which is what torch's default stream is).  Everything the launch reads
 * or overwrites must be ordered before it ON THAT STREAM by the caller.  out_off/out_cap in d_blocks
 * must already be set (cbc_gpu_plan_output). */
typedef struct cbc_device_batch {
    const cbc_read_rec   *d_recs;
    const uint8_t        *d_seq;
    const uint32_t       *d_tok;
    const uint8_t        *d_names;
    const cbc_block_desc *d_blocks;  uint32_t n_blocks;
    const uint8_t        *d_ref;     uint64_t ref_bytes;
    uint8_t              *d_out;     uint64_t out_bytes;
    cbc_block_result     *d_results;
    uint64_t              seq_bytes;
    uint64_t              n_tok;
    uint64_t              n_recs;
    cbc_lds_caps          caps;
} cbc_device_batch;

int  cbc_gpu_encode_blocks_device(cbc_gpu_ctx *ctx, const cbc_device_batch *batch, void *hip_stream);

/* Device-side compaction of the per-block payload areas written by the encode launch: an exclusive
 * scan of cbc_block_result.nbytes into d_offsets[n_blocks+1], then a gather into d_packed
 * (block b -> d_packed[d_offsets[b] .. d_offsets[b+1])).  Asynchronous on `hip_stream`. */
int  cbc_gpu_compact_device(cbc_gpu_ctx *ctx, const uint8_t *d_scratch, const cbc_block_desc *d_blocks,
                            const cbc_block_result *d_results, uint32_t n_blocks, uint64_t *d_offsets,
                            uint8_t *d_packed, uint64_t packed_cap, void *hip_stream);

/* Checksum of payload bytes, for the exchange step of the multi-GPU path: every rank sums its
 * compacted payloads on the device before the gather, the receiver sums what arrived (on its device, or on the host with
 * libcbc_host's cbc_checksum64 -- same value) and compares.  sum over i of (byte[i] + 1) * (((i + 1) * 0x9E3779B97F4A7C15) | 1)
 * mod 2^64: order-free, so it is exact under any reduction order; position-weighted, so a shifted, truncated, padded or
 * permuted buffer does not pass.  *d_sum (device, 8 bytes) is valid once `hip_stream` has reached this point. */
#define CBC_CHECKSUM_TERM(i, byte) ((uint64_t)((uint32_t)(byte) + 1u) * ((((uint64_t)(i) + 1u) * 0x9E3779B97F4A7C15ull) | 1ull))
int  cbc_gpu_checksum_device(cbc_gpu_ctx *ctx, const uint8_t *d_bytes, uint64_t n, uint64_t *d_sum, void *hip_stream);

/* Fills blocks[b].out_off / out_cap with a worst-case bound (every coded symbol costs at most 20
 * bits because every model total stays below 2^20) and returns the scratch bytes needed. */
uint64_t cbc_gpu_plan_output(cbc_block_desc *blocks, uint32_t n_blocks,
                             const cbc_read_rec *recs, const uint32_t *tok);

/* The same bound from the caps alone, without reading the records: no block holds more than caps->cap_var - 1 edit
 * events (the packers cut blocks that way).  O(blocks); what the host-buffer entry points use, and what sizes their `out`. */
uint64_t cbc_gpu_plan_output_caps(cbc_block_desc *blocks, uint32_t n_blocks, const cbc_lds_caps *caps);
/* Grow the context's device buffers for a batch of this shape before the batch exists (allocation of gigabytes takes
 * tens of milliseconds the first time: a CLI does it on the device-init thread while the host still parses the text). */
int  cbc_gpu_reserve_encode(cbc_gpu_ctx *ctx, uint64_t n_recs, uint64_t seq_bytes, uint64_t n_tok, uint32_t n_blocks,
                            uint64_t scratch_bytes);

/* Dynamic LDS bytes one block's workgroup needs for `caps` (workgroups per CU = 160 KiB / this). */
uint32_t cbc_gpu_lds_bytes(const cbc_lds_caps *caps);

/* ---- decode direction (replaces decompress(), src/compression.c:173-216,
 *      decompress_read()/reconstruct_read(), src/read_decompression.c:59-529) ----------------------- */
typedef struct cbc_dec_block_desc {
    uint64_t in_off;       /* byte offset of the block's payload in in[]                          */
    uint64_t ref_off;      /* byte offset in the device reference of the base that is POS 1       */
    uint64_t rec_base;     /* index of the block's first output cbc_read_rec                      */
    uint64_t seq_base;     /* byte offset of the block's output bases (n_reads * seq_stride)      */
    uint32_t in_bytes;     /* payload bytes                                                       */
    uint32_t n_reads;      /* records the container index says the block holds                    */
    uint32_t read_length;  /* header read length L0 (checked against the stream)                  */
    uint32_t seq_stride;   /* bytes reserved per read in seq_out: multiple of 4, >= longest read  */
    uint32_t reserved[4];
} cbc_dec_block_desc;      /* 64 bytes */

typedef struct cbc_dec_device_batch {
    const uint8_t            *d_in;      uint64_t in_bytes;   /* payloads + >= 3 spare bytes        */
    const cbc_dec_block_desc *d_blocks;  uint32_t n_blocks;
    const uint8_t            *d_ref;     uint64_t ref_bytes;
    cbc_read_rec             *d_recs;    uint64_t n_recs;     /* out: pos (block-local), flag, rlen */
    uint8_t                  *d_seq;     uint64_t seq_bytes;  /* out: bases; >= sum + 8             */
    cbc_block_result         *d_results;                      /* nbytes = records decoded           */
    uint32_t                 *d_var_scratch; uint64_t var_scratch_words; /* n_blocks * caps.cap_var words */
    cbc_lds_caps              caps;                           /* from the container header          */
} cbc_dec_device_batch;

int  cbc_gpu_decode_blocks_device(cbc_gpu_ctx *ctx, const cbc_dec_device_batch *batch, void *hip_stream);

/* Host-buffer form: payloads in, records + bases out (recs[n_recs], seq[n_recs * seq_stride]). */
int  cbc_gpu_decode_blocks(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes,
                           cbc_dec_block_desc *blocks, uint32_t n_blocks, const cbc_lds_caps *caps,
                           cbc_read_rec *recs, uint64_t n_recs, uint8_t *seq, uint64_t seq_bytes,
                           cbc_block_result *results /* n_blocks or NULL */);
uint32_t cbc_gpu_decode_lds_bytes(const cbc_lds_caps *caps);

/* ---- region decode (block container version 2) ------------------------------------------------
 * Decode only `blocks` (a contiguous run of one contig's blocks, as cbc_unpack_region in libcbc_host selects them) and keep
 * the reads that overlap the region [beg, end] (1-based, inclusive): POS <= end and POS + span - 1 >= beg, where POS =
 * window_start[b] + the decoded block-local POS and span = the reference bases the decoder's reconstruction covers (rlen for
 * a read coded as perfect, rlen + nDel - nIns otherwise).  The decode kernel writes each span into cbc_read_rec.tok_off and
 * fails the block with CBC_ST_SPAN if one exceeds `smax`; a filter kernel counts the kept reads and their text bytes per
 * block, a scan places the blocks, and a text kernel writes every kept read + '\n' into one dense buffer -- exactly what
 * `cbc -x` writes for those records, in container order.  Records and bases stay on the device; only the text comes back.
 * blocks[].in_off index `in`; rec_base / seq_base are laid out by the library (the caller's array is not modified).
 * *text_bytes = bytes of text (also when text_cap is too small: CBC_E_ARG, nothing copied), *n_selected = reads kept. */
int  cbc_gpu_decode_region(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const cbc_dec_block_desc *blocks,
                           uint32_t n_blocks, const cbc_lds_caps *caps, const uint64_t *window_start /* n_blocks */,
                           uint64_t beg, uint64_t end, uint32_t smax, uint8_t *text, uint64_t text_cap,
                           uint64_t *text_bytes, uint64_t *n_selected, cbc_block_result *results /* n_blocks or NULL */);
/* cbc_gpu_decode_blocks with the spans reported: recs[r].tok_off = span of record r, CBC_ST_SPAN for a span above smax (the
 * decoder the region path runs, with its records and rows returned; what the tests check the spans with) */
int  cbc_gpu_decode_blocks_span(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, cbc_dec_block_desc *blocks,
                                uint32_t n_blocks, const cbc_lds_caps *caps, uint32_t smax, cbc_read_rec *recs, uint64_t n_recs,
                                uint8_t *seq, uint64_t seq_bytes, cbc_block_result *results /* n_blocks or NULL */);
/* Kernel times of the most recent cbc_gpu_decode_region (HIP events on its stream): the span-reporting decode, the filter
 * (count pass + block scan) and the text assembly. */
int  cbc_gpu_last_region_ms(cbc_gpu_ctx *ctx, float *decode_ms, float *filter_ms, float *text_ms);

/* ---- SAM output of a decode ---------------------------------------------------------------------
 * Decode `blocks` and write one SAM alignment line per read, text assembled on the device, in container order:
 *     *\t<FLAG>\t<RNAME>\t<POS>\t255\t*\t*\t0\t0\t<SEQ>\t*\n
 * FLAG = the decoded flag; RNAME = the name of the block's contig (names[contig_name_off[block_contig[b]]], NUL-terminated,
 * at most CBC_SAM_MAX_NAME bytes, no tab or newline); POS = window_start[b] + the decoded block-local POS, at most
 * CBC_SAM_MAX_POS; SEQ = the bases `cbc -x` writes for the read.  What the file does not store is spelled "not available".
 * The records part only: the @HD / @SQ header is host text (cbc_unpack_sam_header, libcbc_host).
 * region == NULL: every read of the blocks, decoded by the plain decoder.  Otherwise the blocks are a selection of
 * cbc_unpack_region, decoded by the span-reporting decoder against region->smax (CBC_ST_SPAN), and the reads kept are those
 * cbc_gpu_decode_region keeps for [beg, end].  A block that fails to decode contributes no line and the call returns
 * CBC_E_BLOCK, as cbc_gpu_decode_region does.  blocks[].in_off index `in`; rec_base / seq_base are laid out by the library.
 * *text_bytes = bytes of text (also when text_cap is too small: CBC_E_ARG, nothing copied), *n_reads = lines written.
 * A line is 20 + digits(FLAG) + len(RNAME) + digits(POS) + rlen bytes: text_cap = sum over blocks of n_reads * (35 +
 * len(RNAME) + seq_stride) always suffices (cbc_unpack_sam_text_cap). */
#define CBC_SAM_MAX_NAME 255u
#define CBC_SAM_MAX_POS  0x7fffffffu
typedef struct cbc_sam_region { uint64_t beg, end; uint32_t smax, reserved; } cbc_sam_region;
int  cbc_gpu_decode_sam(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const cbc_dec_block_desc *blocks,
                        uint32_t n_blocks, const cbc_lds_caps *caps, const uint64_t *window_start /* n_blocks */,
                        const uint32_t *block_contig /* n_blocks */, const char *names, uint32_t names_bytes,
                        const uint32_t *contig_name_off /* n_contigs */, uint32_t n_contigs,
                        const cbc_sam_region *region /* or NULL */, uint8_t *text, uint64_t text_cap,
                        uint64_t *text_bytes, uint64_t *n_reads, cbc_block_result *results /* n_blocks or NULL */);
/* Kernel times of the most recent cbc_gpu_decode_sam (HIP events on its stream): the decode, the count pass + block scan,
 * and the text assembly. */
int  cbc_gpu_last_sam_ms(cbc_gpu_ctx *ctx, float *decode_ms, float *count_ms, float *text_ms);
/* cbc_gpu_decode_sam with CIGAR, NM and MD: the same selection, order, FLAG, RNAME, POS and SEQ, the
 * line
 *     *\t<FLAG>\t<RNAME>\t<POS>\t255\t<CIGAR>\t*\t0\t0\t<SEQ>\t*\tNM:i:<n>\tMD:Z:<md>\n
 * from the alignment the edit-reporting decoder keeps (cbc_gpu_decode_blocks_edits below): per read with indels nDel matched
 * coordinates dc[] and nIns read indices oi[]; T = rl - nIns.  The read's elements in order, for m = 0 .. T: the inserted read
 * indices in front of aligned base m (those q in oi with q - #{oi < q} = m), then the deleted bases with dc = m, then aligned
 * base m (m < T): an insertion run is anchored at the aligned base before it, and an input that had the deletion first comes back
 * with the insertion first.  CIGAR = maximal runs of one kind: M (never = or X), D, I; an inserted run with no aligned base
 * before it or none after it in the read is S (a leading or trailing I of the input comes back as S).  A mismatch is an aligned
 * read byte that differs from the byte of the uploaded reference (a plain byte compare: N over N is a match, which samtools
 * calmd counts as a mismatch).  NM = mismatches + bases of I runs + deleted bases.  MD: the standard grammar over the aligned and
 * deleted elements (n matches; a mismatch: n, the reference byte; a deleted run: n, '^', its reference bytes; n at the end).  A
 * read coded as perfect is <rl>M, NM:i:0, MD:Z:<rl>.  A record whose side / arena entries are not what the decoder writes
 * (counts above 255, entries outside the block's arena, dc not ascending or above T, oi not strictly ascending or >= rl, rl = 0,
 * reference bytes outside the upload) is written as cbc_gpu_decode_sam writes it, CIGAR '*' and no tags.
 * region = NULL: every read, decoded against smax (> 0: the container's span bound, as cbc_gpu_decode_blocks_span takes it);
 * otherwise smax is not read and region->smax is the bound.  edits_per_read (1..CBC_EDITS_MAX, 0 = CBC_EDITS_PER_READ) sizes the
 * arena as for cbc_gpu_decode_pileup: a block that needs more fails with CBC_ST_EDITS.  A failed block writes nothing and the
 * call returns CBC_E_BLOCK.  *text_bytes is also set when text_cap is too small (CBC_E_ARG, nothing copied):
 * cbc_unpack_sam_cigar_text_cap always suffices but is about three times the text, so a caller may try less and repeat once at
 * *text_bytes.  One chunk, one stream, no host round trip between the kernels. */
int  cbc_gpu_decode_sam_cigar(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const cbc_dec_block_desc *blocks,
                              uint32_t n_blocks, const cbc_lds_caps *caps, const uint64_t *window_start /* n_blocks */,
                              const uint32_t *block_contig /* n_blocks */, const char *names, uint32_t names_bytes,
                              const uint32_t *contig_name_off /* n_contigs */, uint32_t n_contigs,
                              const cbc_sam_region *region /* or NULL */, uint32_t smax, uint32_t edits_per_read,
                              uint8_t *text, uint64_t text_cap, uint64_t *text_bytes, uint64_t *n_reads,
                              cbc_block_result *results /* n_blocks or NULL */);
/* Kernel times of the most recent cbc_gpu_decode_sam_cigar: the edits decode, the measure pass, the count pass + block scan,
 * and the text assembly. */
int  cbc_gpu_last_sam_cigar_ms(cbc_gpu_ctx *ctx, float *decode_ms, float *measure_ms, float *count_ms, float *text_ms);

/* ---- coverage of a decode -------------------------------------------------------------------------
 * Decode `blocks` -- a selection of cbc_unpack_region on ONE contig, decoded by the span-reporting decoder against smax --
 * and write the depth of the window [beg, end] (1-based, inclusive, end <= CBC_SAM_MAX_POS) as bedGraph, computed and
 * formatted on the device: one line per maximal run of equal, non-zero depth, 0-based half-open, in position order, no header:
 *     <name>\t<start0>\t<end0>\t<depth>\n
 * Depth at position p = the kept reads with POS <= p <= POS + span - 1, POS = window_start[b] + the block-local POS and span
 * the reference bases the codec's reconstruction covers (rlen for a read coded as perfect, rlen + nDel - nIns otherwise; 0
 * covers nothing).  This is a SPAN coverage: deleted bases count as covered (this pass reads only the span; where they lie
 * is what cbc_gpu_decode_pileup keeps) -- for ordinary CIGARs the interval M + D + N, what `bedtools genomecov -bg` and `samtools depth -J` count.  Kept =
 * every read cbc_gpu_decode_region keeps for [beg, end] with (FLAG & exclude_flags) == 0.  Reads are clipped to the window and
 * runs that reach its edge end there.  `name` (name_bytes of it, 1..CBC_SAM_MAX_NAME, no tab / newline / NUL) is the text of
 * the first column.  A block that fails to decode marks nothing and the call returns CBC_E_BLOCK, as cbc_gpu_decode_region
 * does.  *text_bytes = bytes of text (also when text_cap is too small: CBC_E_ARG, nothing copied), *n_runs = lines,
 * *n_reads_kept = reads counted.  K reads give at most 2K - 1 runs and a line is at most name_bytes + 34 bytes
 * (cbc_unpack_depth_text_cap).  The window costs 4 bytes of device memory per position: CBC_E_NOMEM when that cannot be had. */
int  cbc_gpu_decode_depth(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const cbc_dec_block_desc *blocks,
                          uint32_t n_blocks, const cbc_lds_caps *caps, const uint64_t *window_start /* n_blocks */,
                          const char *name, uint32_t name_bytes, uint64_t beg, uint64_t end, uint32_t smax,
                          uint32_t exclude_flags, uint8_t *text, uint64_t text_cap, uint64_t *text_bytes, uint64_t *n_runs,
                          uint64_t *n_reads_kept, cbc_block_result *results /* n_blocks or NULL */);
/* Kernel times of the most recent cbc_gpu_decode_depth (HIP events on its stream): the span decode; zeroing + mark; tile
 * sums, scans and change points; line count, scan and the text. */
int  cbc_gpu_last_depth_ms(cbc_gpu_ctx *ctx, float *decode_ms, float *mark_ms, float *scan_ms, float *text_ms);

/* ---- per-position allele counts of a decode -------------------------------------------------------
 * Decode `blocks` -- a selection of cbc_unpack_region or cbc_unpack_contig_blocks on ONE contig -- with the decoder that keeps
 * the alignment it reconstructs with, and write what the kept reads show at the positions of the window [beg, end] (1-based,
 * inclusive, end <= CBC_SAM_MAX_POS) where they disagree with the reference; computed and formatted on the device, tab-separated,
 * no header, in position order:
 *     <name>\t<pos1>\t<ref>\t<depth>\t<A>\t<C>\t<G>\t<T>\t<N>\t<del>\t<ins>\n
 * ref = the byte of the uploaded reference; every other column a decimal integer.  Kept = the reads cbc_gpu_decode_depth keeps
 * under the same exclude_flags.  The alignment is the codec's: a read without indels (coded as perfect, or SNPs only) has read
 * base q at POS + q.  A read with nDel deleted bases at matched coordinates dc[] and nIns inserted bases at read indices oi[]
 * (both as the decoder holds them): q == oi[i] is inserted; any other q has m = q - #{i : oi[i] < q} and is aligned to
 * POS + m + #{d : dc[d] <= m}; deleted base d (decode order) is POS + dc[d] + d.  Whatever that maps outside the read's span
 * [POS, POS + span - 1] is not counted.  The class of a byte is byte & 0xDF: A, C, G, T, anything else is N.  A..N = the aligned
 * read bases of the class; del = deleted bases; ins = insertion events, an event being a maximal run of inserted read indices,
 * anchored at the position of the nearest aligned base before it, or at POS when there is none (a trailing soft clip is stored
 * as insertions and shows as one event at the read's last aligned base).  depth = A + C + G + T + N + del, which is the depth
 * cbc_gpu_decode_depth reports.  Position p gets a line when depth - (count of ref's class) + ins >= min_alt (>= 1).  Reads are
 * clipped to the window; an event whose anchor lies outside it is not counted.
 * edits_per_read (1..CBC_EDITS_MAX, 0 = CBC_EDITS_PER_READ) sizes the arena the alignment is kept in: a block of n reads has
 * room for n * edits_per_read deleted and inserted bases of its reads with indels, 2 bytes each; a block that needs more fails
 * with CBC_ST_EDITS, nothing is truncated.  A block that fails to decode contributes nothing and the call returns CBC_E_BLOCK.
 * *text_bytes = bytes of text (also when text_cap is too small: CBC_E_ARG, nothing copied), *n_lines = lines, *n_reads_kept =
 * reads counted.  text_cap = min(window, reads * smax) * (name_bytes + 102) always suffices (cbc_unpack_pileup_text_cap).  The
 * window costs 4 + 28 bytes of device memory per position: CBC_E_NOMEM when that cannot be had.  One chunk, one stream, no host
 * round trip between the kernels. */
#define CBC_EDITS_PER_READ 16u
#define CBC_EDITS_MAX      510u
int  cbc_gpu_decode_pileup(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const cbc_dec_block_desc *blocks,
                           uint32_t n_blocks, const cbc_lds_caps *caps, const uint64_t *window_start /* n_blocks */,
                           const char *name, uint32_t name_bytes, uint64_t beg, uint64_t end, uint32_t smax,
                           uint32_t exclude_flags, uint32_t min_alt, uint32_t edits_per_read, uint8_t *text, uint64_t text_cap,
                           uint64_t *text_bytes, uint64_t *n_lines, uint64_t *n_reads_kept,
                           cbc_block_result *results /* n_blocks or NULL */);
/* cbc_gpu_decode_pileup with a least alternative fraction and per-strand counts.  With min_alt_ppm = 0
 * and by_strand = 0 it writes the bytes of cbc_gpu_decode_pileup; any other value than min_alt_ppm in 0..1 000 000 and by_strand
 * in 0..1 is CBC_E_ARG.
 * min_alt_ppm > 0: with nonref = depth - (count of ref's class) + ins, position p gets a line when nonref >= min_alt AND
 * nonref * 10^6 >= min_alt_ppm * depth, in exact integer arithmetic (both products are below 2^52).  Insertion events are not part
 * of depth, so nonref can exceed it; such a position passes every fraction.
 * by_strand = 1: every line keeps its eleven columns and seven more follow, tab-separated:
 *     ... <del>\t<ins>\t<A+>\t<C+>\t<G+>\t<T+>\t<N+>\t<del+>\t<ins+>\n
 * X+ = column X counted over the kept reads with FLAG & 16 == 0 only (the reverse strand's count is X - X+).  Which positions get
 * a line is decided on the totals.  exclude_flags applies first: with bit 16 in it every X+ equals X.
 * text_cap = min(window, reads * smax) * (name_bytes + 102 + 77 * by_strand) always suffices (cbc_unpack_pileup_ext_text_cap).
 * With by_strand the window costs 8 + 56 bytes of device memory per position, otherwise 4 + 28: CBC_E_NOMEM when that cannot be
 * had.  Everything else is as for cbc_gpu_decode_pileup. */
int  cbc_gpu_decode_pileup_ext(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const cbc_dec_block_desc *blocks,
                               uint32_t n_blocks, const cbc_lds_caps *caps, const uint64_t *window_start /* n_blocks */,
                               const char *name, uint32_t name_bytes, uint64_t beg, uint64_t end, uint32_t smax,
                               uint32_t exclude_flags, uint32_t min_alt, uint32_t edits_per_read, uint32_t min_alt_ppm,
                               uint32_t by_strand, uint8_t *text, uint64_t text_cap, uint64_t *text_bytes, uint64_t *n_lines,
                               uint64_t *n_reads_kept, cbc_block_result *results /* n_blocks or NULL */);
/* Kernel times of the most recent cbc_gpu_decode_pileup or _ext (HIP events on its stream): the edits decode; zeroing + mark(s) +
 * events; tile sums, their scan(s), the line count and its scan; the text. */
int  cbc_gpu_last_pileup_ms(cbc_gpu_ctx *ctx, float *decode_ms, float *events_ms, float *scan_ms, float *text_ms);

/* ---- consensus ------------------------------------------------------------------------------------
 * The sequence the kept reads spell over the window [beg, end] of contig `name`, as one FASTA record, called and written on the
 * device behind the passes of cbc_gpu_decode_pileup.  The arguments up to edits_per_read, the kept reads, the alignment and the
 * failure behaviour are that call's: a block that fails to decode (CBC_ST_EDITS included) contributes nothing and the call returns
 * CBC_E_BLOCK behind the text of the others.
 * Per position p, with c[0..3] = the aligned read bases of class A, C, G, T, c[4] = those of any other class, d = the deleted
 * bases, ins = the insertion events -- the numbers cbc_gpu_decode_pileup prints for p under the same exclude_flags --, depth =
 * c[0] + ... + c[4] + d, ref = the byte of the uploaded reference, and reaches(x) meaning x * 10^6 >= call_ppm * depth in exact
 * integers (both products are below 2^52), in this order:
 *   1  depth < min_depth: 'N'; with CBC_CONS_FILL_REF the reference byte in lower case (ref | 0x20 when ref & 0xDF is in A..Z,
 *      the byte unchanged otherwise).
 *   2  of the five candidates A, C, G, T, DEL with the counts c[0..3], d, the highest; among ties the reference's class when it is
 *      one of them, otherwise the first in the order A, C, G, T, DEL.  When reaches(that count) the position is called: a base
 *      writes its upper-case letter, DEL writes nothing -- the base is dropped from the sequence -- or '*' with CBC_CONS_SHOW_DEL.
 *      The other class counts in depth and is never a candidate.
 *   3  with CBC_CONS_IUPAC, when 2 did not call: for every base count t = c[i] > 0 let S(t) be the bases with c[j] >= t; the
 *      largest t with reaches(sum of the counts of S(t)) writes the IUPAC letter of S(t) (R Y S W K M B D H V, N for all four);
 *      none: 'N'.
 *   4  otherwise 'N'.
 * Insertions are NOT applied: the planes count insertion events, not their bases.  counts->ins_skipped is the number of positions
 * with depth >= min_depth and reaches(ins); a trailing soft clip is stored as insertions and shows as one such event at the
 * read's last aligned base.  ref is read where the window lies in the uploaded reference: a window is expected to end inside its
 * contig (the selections of cbc_unpack_region and cbc_unpack_contig_blocks do); past it the bytes are the pad's and the next
 * contig's, and only past the whole reference 'N'.
 * The text: `>NAME\n` (with_range = 0) or `>NAME:BEG-END\n` (with_range = 1; 1-based, inclusive), then the E emitted bytes in
 * position order, line_width a line, every line ending in '\n' -- the last too, no empty line, the header alone when E = 0:
 * header + E + ceil(E / line_width) bytes; cbc_unpack_consensus_text_cap (include/cbc_host.h) gives the bound for E = the window.
 * counts: emitted = E; ref, alt = called bases of the reference's class and of another; del = called deletions (emitted only with
 * SHOW_DEL); ambiguous = letters of step 3; low_depth = step 1; no_call = the 'N' of steps 3 and 4: the six sum to the window.
 * min_depth == 0, call_ppm outside 1..1 000 000, line_width outside 1..65 535, a flag bit beyond the three and with_range > 1 are
 * CBC_E_ARG.  *text_bytes = bytes of text (also when text_cap is too small: CBC_E_ARG, nothing copied).  Blocks without a single
 * read are as no blocks: CBC_OK and no text -- the record of such a window is cbc_unpack_consensus_empty's.  The window costs
 * 4 + 28 bytes of device memory per position: CBC_E_NOMEM when that cannot be had. */
#define CBC_CONS_SHOW_DEL 1u
#define CBC_CONS_FILL_REF 2u
#define CBC_CONS_IUPAC    4u
typedef struct cbc_consensus_opts   { uint32_t min_depth, call_ppm, line_width, flags; } cbc_consensus_opts;
typedef struct cbc_consensus_counts { uint64_t emitted, ref, alt, del, ambiguous, low_depth, no_call, ins_skipped; } cbc_consensus_counts;
int  cbc_gpu_decode_consensus(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const cbc_dec_block_desc *blocks,
                              uint32_t n_blocks, const cbc_lds_caps *caps, const uint64_t *window_start /* n_blocks */,
                              const char *name, uint32_t name_bytes, uint64_t beg, uint64_t end, uint32_t smax,
                              uint32_t exclude_flags, uint32_t edits_per_read, const cbc_consensus_opts *opts, uint32_t with_range,
                              uint8_t *text, uint64_t text_cap, uint64_t *text_bytes, cbc_consensus_counts *counts,
                              uint64_t *n_reads_kept, cbc_block_result *results /* n_blocks or NULL */);
/* Kernel times of the most recent cbc_gpu_decode_consensus: the edits decode; zeroing + mark + events; tile sums, their scan, the
 * call count and its scan; the text. */
int  cbc_gpu_last_consensus_ms(cbc_gpu_ctx *ctx, float *decode_ms, float *events_ms, float *scan_ms, float *text_ms);
/* cbc_gpu_decode_blocks_span with the edits reported as well (the decoder the pileup runs, with everything it leaves returned;
 * what the tests check it with): side[2 r] = the first arena entry of record r relative to its block's, side[2 r + 1] =
 * nDel | nIns << 16 (both 0 for a read without indels); block b owns arena entries [rec_base * edits_per_read, (rec_base +
 * n_reads) * edits_per_read); a record's entries are its nDel matched coordinates, then its nIns read indices.  side holds
 * 2 * n_recs words, arena n_recs * edits_per_read entries. */
int  cbc_gpu_decode_blocks_edits(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, cbc_dec_block_desc *blocks,
                                 uint32_t n_blocks, const cbc_lds_caps *caps, uint32_t smax, uint32_t edits_per_read,
                                 cbc_read_rec *recs, uint64_t n_recs, uint8_t *seq, uint64_t seq_bytes, uint32_t *side,
                                 uint16_t *arena, cbc_block_result *results /* n_blocks or NULL */);

/* ---- deletion-aware coverage ----------------------------------------------------------------------
 * A setting of the context.  edits_per_read = 0 (the default) leaves every call as it is: the depth is the SPAN depth, a read
 * covers POS .. POS + span - 1, the bases it deletes included.  edits_per_read in 1..510 (CBC_EDITS_PER_READ is the usual
 * choice; more is CBC_E_ARG and changes nothing): from then on the depth at position p, in every call that reports a depth
 * but the pileup -- cbc_gpu_decode_depth, cbc_gpu_decode_targets with the depth output, cbc_gpu_decode_coverage, _ext and _quant,
 * cbc_gpu_decode_depth_hist --, is the kept reads with an ALIGNED base at p: the span depth less the deleted bases of the kept
 * reads at p (the `depth - del` of cbc_gpu_decode_pileup; what samtools depth without -J, mosdepth and bedtools genomecov -split
 * count).  Inserted bases and soft clips change nothing; a deleted base outside its read's span, the window or the intervals is
 * not counted.  "Kept" keeps its meaning, and so do n_reads_kept / n_reads and the `reads` of cbc_gpu_decode_coverage_ext: a
 * read whose only bases inside a query are deleted still overlaps it (samtools bedcov -c counts it too).
 * These calls then run the decoder that keeps the alignment, with an arena of edits_per_read entries per read as for the pileup
 * (2 bytes each; a block whose reads hold more deleted and inserted bases fails with CBC_ST_EDITS and the call returns
 * CBC_E_BLOCK), and one more stage behind the mark kernel that takes the deleted bases off the difference array.  The change
 * points -- two per read before -- are sized min(difference-array words, 2 * reads * (1 + edits_per_read) (+ 2 per interval)),
 * 8 bytes each (and 12 + 4 per threshold more in the coverage calls): CBC_E_NOMEM, with a message that names the setting, when
 * that cannot be had.  text_cap of cbc_gpu_decode_depth: min(window, reads * smax) * (name_bytes + 34) always suffices
 * (cbc_unpack_depth_skipdel_text_cap; cbc_unpack_targets_depth_skipdel_cap for a target set); the 2K - 1 runs of the span depth
 * no longer hold.  The cbc_gpu_last_*_ms of these calls keep their meaning: the new stage's time falls into the mark stretch
 * ("zeroing + mark"), the decode stretch is the edits decode. */
int  cbc_gpu_set_depth_skip_deletions(cbc_gpu_ctx *ctx, uint32_t edits_per_read);

/* ---- decode of a set of regions -------------------------------------------------------------------
 * `blocks` are the blocks a target set selects (cbc_unpack_targets of libcbc_host: the union of the single-region selections
 * of its merged intervals), gathered by the caller with their window starts and contigs; they are decoded ONCE by the
 * span-reporting decoder against t->smax.  t->iv holds n_iv intervals as pairs beg, end (1-based, inclusive, <= CBC_SAM_MAX_POS),
 * grouped per contig, ascending, disjoint and not touching inside a contig; t->block_iv gives for block b of the call the first
 * interval and the count of the intervals of its contig that its reads can reach.  A read is selected when it overlaps at
 * least one interval: POS <= end and POS + span - 1 >= beg, the rule of cbc_gpu_decode_region.
 *   CBC_TARGETS_READS  every selected read once, in the order of the blocks, the bytes cbc_gpu_decode_region writes for it
 *   CBC_TARGETS_SAM    the same reads as the alignment lines cbc_gpu_decode_sam writes (no header)
 *   CBC_TARGETS_DEPTH  the blocks of ONE contig: the bedGraph of cbc_gpu_decode_depth restricted to the intervals -- byte for
 *                      byte the texts of its calls for each interval in turn; reads with FLAG & exclude_flags != 0 left out.
 *                      Device memory follows the set (4 bytes per position inside the intervals), not the contig.
 * *n_reads = reads selected (depth: reads counted), *n_runs = lines of a depth call.  A block that fails to decode contributes
 * nothing and the call returns CBC_E_BLOCK; *text_bytes is also set when text_cap is too small (CBC_E_ARG, nothing copied). */
#define CBC_TARGETS_READS 0u
#define CBC_TARGETS_SAM   1u
#define CBC_TARGETS_DEPTH 2u
typedef struct cbc_gpu_targets {
    const uint32_t *iv;          /* n_iv pairs beg, end */
    const uint32_t *block_iv;    /* per block of the call: first interval, count */
    uint32_t n_iv, smax;
} cbc_gpu_targets;
int  cbc_gpu_decode_targets(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const cbc_dec_block_desc *blocks,
                            uint32_t n_blocks, const cbc_lds_caps *caps, const uint64_t *window_start /* n_blocks */,
                            const uint32_t *block_contig /* n_blocks */, const char *names, uint32_t names_bytes,
                            const uint32_t *contig_name_off /* n_contigs */, uint32_t n_contigs, const cbc_gpu_targets *t,
                            uint32_t output, uint32_t exclude_flags, uint8_t *text, uint64_t text_cap, uint64_t *text_bytes,
                            uint64_t *n_reads, uint64_t *n_runs, cbc_block_result *results /* n_blocks or NULL */);
/* Kernel times of the most recent cbc_gpu_decode_targets: the span decode; the count pass + scan (depth: zeroing + mark); for
 * the depth the tile sums, scans and change points (else 0); the text. */
int  cbc_gpu_last_targets_ms(cbc_gpu_ctx *ctx, float *decode_ms, float *filter_ms, float *scan_ms, float *text_ms);

/* ---- per-query coverage summary -------------------------------------------------------------------
 * The depth form of cbc_gpu_decode_targets -- the selected blocks of ONE contig, decoded once, marked in the compressed
 * coordinate of the contig's merged intervals -- without the text: for every query the sum of the depth over its positions and
 * the number of its positions with depth >= min_depth (>= 1), computed on the device from the change points; 12 bytes per query
 * come back.  Depth is that of cbc_gpu_decode_depth (span coverage, reads with FLAG & exclude_flags != 0 left out).
 *   t, iv_first, iv_count   the interval table of cbc_unpack_queries / cbc_unpack_targets and the contig's part of it
 *                           (contig_first[c], contig_count[c]); t->block_iv as for cbc_gpu_decode_targets.  The compressed
 *                           coordinate lays these intervals end to end with one spare slot behind each.
 *   q                       n_q <= 2^24 pairs slot, len: the query's first slot and its length; a query lies inside one
 *                           interval (slot = slots in front of the interval + start - interval beg: cbc_query.slot)
 *   sum[n_q], covered[n_q]  the results, in the order of q; all zero when no block reaches an interval
 * One call runs as one chunk on one stream with no host round trip between its kernels.  A block that fails to decode
 * contributes nothing and the call returns CBC_E_BLOCK; CBC_E_NOMEM when the difference array or the prefix tables (12 bytes
 * per change point) cannot be had; CBC_E_ARG for a query that reaches past the slots.  *n_reads = reads counted. */
int  cbc_gpu_decode_coverage(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const cbc_dec_block_desc *blocks,
                             uint32_t n_blocks, const cbc_lds_caps *caps, const uint64_t *window_start /* n_blocks */,
                             const uint32_t *block_contig /* n_blocks */, const char *names, uint32_t names_bytes,
                             const uint32_t *contig_name_off /* n_contigs */, uint32_t n_contigs, const cbc_gpu_targets *t,
                             uint32_t iv_first, uint32_t iv_count, const uint32_t *q /* n_q pairs slot, len */, uint32_t n_q,
                             uint32_t exclude_flags, uint32_t min_depth, uint64_t *sum, uint32_t *covered, uint64_t *n_reads,
                             cbc_block_result *results /* n_blocks or NULL */);
/* Kernel times of the most recent cbc_gpu_decode_coverage: the span decode; zeroing + mark; tile sums, scans and change
 * points; then the four new passes: run weights, the scans of their tile totals, the prefixes, the lookup. */
int  cbc_gpu_last_coverage_ms(cbc_gpu_ctx *ctx, float *decode_ms, float *mark_ms, float *scan_ms, float *weights_ms,
                              float *wscan_ms, float *apply_ms, float *lookup_ms);

/* ---- per-query read counts and depth thresholds ------------------------------------------------------
 * cbc_gpu_decode_coverage with two more answers per query, from data that call already leaves on the device:
 *   thresholds[n_thr]       0 .. 8 depths, each >= 1, strictly ascending (CBC_E_ARG otherwise)
 *   thr_covered[n_q * n_thr] query-major: the positions of query i with depth >= thresholds[t] at [i * n_thr + t]
 *   reads[n_q] or NULL      the kept reads (FLAG & exclude_flags == 0, span >= 1) with at least one covered base in the query:
 *                           POS <= end and POS + span - 1 >= beg.  A read that overlaps two queries counts in both.
 * sum and covered are those of cbc_gpu_decode_coverage.  With reads != NULL the call keeps a second array of the difference
 * array's size (4 bytes per slot) and 8 bytes per start point; the thresholds cost 4 bytes per threshold and change point:
 * CBC_E_NOMEM when they cannot be had.  4 * (n_thr + 1) more bytes per query come back.  One chunk, one stream, no host round
 * trip between the kernels.  A block that fails to decode contributes nothing and the call returns CBC_E_BLOCK with all four
 * outputs zeroed. */
int  cbc_gpu_decode_coverage_ext(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const cbc_dec_block_desc *blocks,
                                 uint32_t n_blocks, const cbc_lds_caps *caps, const uint64_t *window_start /* n_blocks */,
                                 const uint32_t *block_contig /* n_blocks */, const char *names, uint32_t names_bytes,
                                 const uint32_t *contig_name_off /* n_contigs */, uint32_t n_contigs, const cbc_gpu_targets *t,
                                 uint32_t iv_first, uint32_t iv_count, const uint32_t *q /* n_q pairs slot, len */, uint32_t n_q,
                                 uint32_t exclude_flags, uint32_t min_depth, uint64_t *sum, uint32_t *covered, uint64_t *n_reads,
                                 cbc_block_result *results /* n_blocks or NULL */, const uint32_t *thresholds, uint32_t n_thr,
                                 uint32_t *thr_covered /* n_q * n_thr, query-major */, uint32_t *reads /* n_q or NULL */);
/* Kernel times of the most recent cbc_gpu_decode_coverage_ext.  cov_ms[7]: the stretches of cbc_gpu_last_coverage_ms, the mark
 * being the one that also notes where the pieces start.  ext_ms[5]: the start points (tile sums, scans, compact over the
 * starts); the thresholds' weights; the scans of their tile totals; their prefixes; the lookup.  A pass that was not asked for
 * takes no time. */
int  cbc_gpu_last_coverage_ext_ms(cbc_gpu_ctx *ctx, float *cov_ms /* 7 */, float *ext_ms /* 5 */);

/* ---- per-query depth quantiles ------------------------------------------------------------------------
 * cbc_gpu_decode_coverage_ext with one more answer per query, selected on the device from the change points that call leaves:
 *   quantiles[n_quant]      1 .. CBC_QUANT_MAX integer percentages in 0..100, strictly ascending (CBC_E_ARG otherwise);
 *                           n_quant == 0: the call is cbc_gpu_decode_coverage_ext
 *   quant_depth[n_q * n_quant] query-major: with the depths of the len positions of query i sorted ascending, d(0) <= .. <=
 *                           d(len - 1), the value d(k - 1) for k = max(1, ceil(p * len / 100)) -- the nearest-rank (lower)
 *                           quantile: p = 0 the minimum, 50 the lower median, 100 the maximum.  Zero-depth positions count.
 *                           A query of no position gives 0.
 * One wavefront selects all quantiles of one query; its table is in LDS, so the pass takes no device memory beyond 4 more bytes
 * per quantile and query in the result arena, which also come back.  One chunk, one stream, no host round trip between the
 * kernels.  A block that fails to decode contributes nothing and the call returns CBC_E_BLOCK with all five outputs zeroed. */
#define CBC_QUANT_MAX 8u
int  cbc_gpu_decode_coverage_quant(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const cbc_dec_block_desc *blocks,
                                   uint32_t n_blocks, const cbc_lds_caps *caps, const uint64_t *window_start /* n_blocks */,
                                   const uint32_t *block_contig /* n_blocks */, const char *names, uint32_t names_bytes,
                                   const uint32_t *contig_name_off /* n_contigs */, uint32_t n_contigs, const cbc_gpu_targets *t,
                                   uint32_t iv_first, uint32_t iv_count, const uint32_t *q /* n_q pairs slot, len */, uint32_t n_q,
                                   uint32_t exclude_flags, uint32_t min_depth, uint64_t *sum, uint32_t *covered, uint64_t *n_reads,
                                   cbc_block_result *results /* n_blocks or NULL */, const uint32_t *thresholds, uint32_t n_thr,
                                   uint32_t *thr_covered /* n_q * n_thr, query-major */, uint32_t *reads /* n_q or NULL */,
                                   const uint32_t *quantiles, uint32_t n_quant,
                                   uint32_t *quant_depth /* n_q * n_quant, query-major */);
/* Kernel times of the most recent cbc_gpu_decode_coverage_quant (with n_quant >= 1): cov_ms[7] and ext_ms[5] as
 * cbc_gpu_last_coverage_ext_ms gives them, quant_ms[1] the selection pass. */
int  cbc_gpu_last_coverage_quant_ms(cbc_gpu_ctx *ctx, float *cov_ms /* 7 */, float *ext_ms /* 5 */, float *quant_ms /* 1 */);

/* ---- depth histogram --------------------------------------------------------------------------------
 * The depth form of cbc_gpu_decode_targets -- the selected blocks of ONE contig, decoded once, marked in the compressed
 * coordinate of all the contig's merged intervals (t, iv_first, iv_count as for cbc_gpu_decode_coverage) -- without the text:
 * how many positions inside the intervals have each depth >= 1, binned on the device from the change points.  Depth is that of
 * cbc_gpu_decode_depth (span coverage, reads with FLAG & exclude_flags != 0 left out).  max_depth > 0: every depth >= max_depth
 * is counted in bin max_depth (0: no folding).
 *   bin_depth[bin_cap], bin_bases[bin_cap]   the bins with bases > 0, ascending in depth.  The depth-0 bin is never among
 *                           them: it is the positions of the intervals less the sum of bin_bases, the caller's subtraction.
 *   *n_bins                 how many there are, also when bin_cap is too small (CBC_E_ARG, nothing copied); at most
 *                           min(max_depth or 2^32 - 1, reads of the call's blocks)
 * A bin is 32 bits on the device and exact: its bases are at most the slots of one contig's compressed coordinate,
 * <= 2^31 + 2^24 < 2^32.  The bin table costs 4 bytes per depth up to min(max_depth, reads): CBC_E_NOMEM when it or the
 * difference array cannot be had.  One call runs as one chunk on one stream with no host round trip between its kernels.  A
 * block that fails to decode contributes nothing; the call returns CBC_E_BLOCK with *n_bins = 0.  *n_reads = reads counted. */
int  cbc_gpu_decode_depth_hist(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const cbc_dec_block_desc *blocks,
                               uint32_t n_blocks, const cbc_lds_caps *caps, const uint64_t *window_start /* n_blocks */,
                               const uint32_t *block_contig /* n_blocks */, const char *names, uint32_t names_bytes,
                               const uint32_t *contig_name_off /* n_contigs */, uint32_t n_contigs, const cbc_gpu_targets *t,
                               uint32_t iv_first, uint32_t iv_count, uint32_t exclude_flags, uint32_t max_depth,
                               uint32_t *bin_depth, uint32_t *bin_bases, uint32_t bin_cap, uint32_t *n_bins, uint64_t *n_reads,
                               cbc_block_result *results /* n_blocks or NULL */);
/* Kernel times of the most recent cbc_gpu_decode_depth_hist: the span decode; zeroing + mark; tile sums, scans and change
 * points; then the new passes: zeroing the bins + accumulate, and the count, scan and write of the non-zero bins. */
int  cbc_gpu_last_hist_ms(cbc_gpu_ctx *ctx, float *decode_ms, float *mark_ms, float *scan_ms, float *accum_ms, float *compact_ms);

/* ---- read statistics ----------------------------------------------------------------------------------
 * The tables of a first look at an alignment file (flag categories, read lengths, GC content per read, base composition per
 * sequencing cycle), counted on the device in one streaming pass over the decoded records and rows; about 270 KB come back
 * whatever the size of the file.
 *   t == NULL   every read of the blocks, decoded by the plain decoder (window_start is not looked at beyond its presence)
 *   t != NULL   the reads cbc_gpu_decode_targets selects for the interval table (the same keep rule, each read once), decoded by
 *               the span-reporting decoder; the blocks may lie on several contigs, block_iv indexes the whole table
 * A read with FLAG & exclude_flags != 0 is counted in `excluded` and nowhere else.
 *   flag[f]            reads with FLAG f
 *   len[l]             reads of length l (a row holds at most 256 bases)
 *   gc[p]              reads of length >= 1 with floor(100 * (bytes 'G' and 'C') / length) = p
 *   cyc[s * 256 + c]   s = 0 .. 4 for A, C, G, T, other: reads whose base in sequencing cycle c (0-based) is s.  Cycle c of a
 *                      read with FLAG & 16 == 0 is SEQ[c]; with FLAG & 16 it is the complement (A <-> T, C <-> G) of
 *                      SEQ[len - 1 - c].  A base is A, C, G or T only if its byte is exactly that letter.
 *   reads              the reads counted = the sum of len[]
 * Every counter is 32 bits on the device and exact: none can pass the reads of the call, and a call over more than 2^32 - 1
 * reads is CBC_E_ARG.  One call runs as one chunk on one stream with no host round trip between its kernels.  A block that fails
 * to decode contributes nothing; the call returns CBC_E_BLOCK with *out all zero. */
#define CBC_STATS_FLAG_BINS 65536u
#define CBC_STATS_LEN_BINS  257u
#define CBC_STATS_GC_BINS   101u
#define CBC_STATS_CYCLES    256u
typedef struct cbc_gpu_stats {
    uint64_t reads, excluded;
    uint32_t flag[CBC_STATS_FLAG_BINS];
    uint32_t len[CBC_STATS_LEN_BINS];
    uint32_t gc[CBC_STATS_GC_BINS];
    uint32_t cyc[5u * CBC_STATS_CYCLES];
} cbc_gpu_stats;
int  cbc_gpu_decode_stats(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const cbc_dec_block_desc *blocks,
                          uint32_t n_blocks, const cbc_lds_caps *caps, const uint64_t *window_start /* n_blocks */,
                          const cbc_gpu_targets *t /* or NULL */, uint32_t exclude_flags, cbc_gpu_stats *out,
                          cbc_block_result *results /* n_blocks or NULL */);
/* Kernel times of the most recent cbc_gpu_decode_stats: the decode; zeroing the tables + the statistics pass. */
int  cbc_gpu_last_stats_ms(cbc_gpu_ctx *ctx, float *decode_ms, float *stats_ms);

/* ---- read statistics with the alignment tables --------------------------------------------------------
 * cbc_gpu_decode_stats behind the edit-reporting decoder (cbc_gpu_decode_blocks_edits), with one more pass that counts how the
 * reads agree with the reference.  *out is what cbc_gpu_decode_stats returns for the same selection.  The alignment is that of
 * cbc_gpu_decode_sam_cigar above: its element order, its S rule (an inserted run with no aligned base before it, or none after
 * it, in the read), its mismatch (a plain byte compare of the aligned read byte with the uploaded reference byte) and its valid
 * record; a counted read -- kept and not excluded -- that cbc_gpu_decode_sam_cigar would write with CIGAR '*' is counted in
 * `invalid` and in no table below.  The cycle of read index q is q + 1 for FLAG & 16 == 0, else rl - q (1-based, the
 * orientation of cbc_gpu_stats.cyc).
 *   reads, invalid   the counted reads that are valid, and those that are not; reads = the sum of len[]
 *   len[l]           valid counted reads of length l
 *   mm[c]            mismatches in cycle c
 *   unal[c]          inserted bases (I and S) in cycle c: the aligned bases of cycle c are the reads of length >= c less unal[c]
 *   ins_cyc[c]       I runs whose first-sequenced base has cycle c: index q0 + 1 forward, rl - q1 reverse for a run over q0 .. q1
 *   del_cyc[c]       D runs behind the base of cycle c: with k the read index of the aligned base behind the run (rl for the
 *                    run that ends the read), c = k forward and rl - k reverse; c = 0 is in front of the first sequenced base
 *   nm[n]            reads with NM = mismatches + I bases + D bases = n, the NM:i: of cbc_gpu_decode_sam_cigar
 *   ins_len[l], del_len[l]   I runs and D runs of l bases
 * Index 0 of the cycle tables is used by del_cyc alone.  smax > 0 is the span bound the decoder checks (t == NULL; otherwise
 * t->smax); edits_per_read sizes the arena as for cbc_gpu_decode_pileup (CBC_ST_EDITS).  Every 32-bit counter is bounded by the
 * reads of the call (2^32 - 1 at most, as for cbc_gpu_decode_stats); ins_len and del_len are exact in 64 bits; a call whose
 * blocks x record groups of the largest block pass 2^29 is CBC_E_ARG.  One call, one chunk, one stream, no host round trip
 * between the kernels.  A failed block contributes nothing; the call returns CBC_E_BLOCK with both structs all zero. */
#define CBC_STATS_ALN_CYC 257u
#define CBC_STATS_ALN_NM  767u
#define CBC_STATS_ALN_LEN 256u
typedef struct cbc_gpu_stats_aln {
    uint64_t reads, invalid;
    uint32_t len[CBC_STATS_ALN_CYC], mm[CBC_STATS_ALN_CYC], unal[CBC_STATS_ALN_CYC], ins_cyc[CBC_STATS_ALN_CYC], del_cyc[CBC_STATS_ALN_CYC];
    uint32_t nm[CBC_STATS_ALN_NM];
    uint64_t ins_len[CBC_STATS_ALN_LEN], del_len[CBC_STATS_ALN_LEN];
} cbc_gpu_stats_aln;
int  cbc_gpu_decode_stats_aln(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const cbc_dec_block_desc *blocks,
                              uint32_t n_blocks, const cbc_lds_caps *caps, const uint64_t *window_start /* n_blocks */,
                              const cbc_gpu_targets *t /* or NULL */, uint32_t smax, uint32_t exclude_flags, uint32_t edits_per_read,
                              cbc_gpu_stats *out, cbc_gpu_stats_aln *aln, cbc_block_result *results /* n_blocks or NULL */);
/* Kernel times of the most recent cbc_gpu_decode_stats_aln: the edits decode; zeroing the tables + the statistics pass; the
 * alignment pass. */
int  cbc_gpu_last_stats_aln_ms(cbc_gpu_ctx *ctx, float *decode_ms, float *stats_ms, float *aln_ms);

/* ---- whole-file stream ("compat" mode): the reference's own file format --------------------------------------
 * compress() / decompress(), src/compression.c:112-216: ONE arithmetic stream per file, models never reset.
 * `batch` is a cbc_host_batch packed with cbc_pack_opts.whole_file = 1: its `blocks` are SEGMENTS of the one
 * stream (POS not rebased).  The bytes written to `out` are the bytes `program -c 1 in.sam out ref.fa` (-DDEBUG
 * build) writes, decodable by the reference's `-x`.  One wavefront codes the stream with the general (rescaling)
 * form of every model (cbc_stream_body.h); throughput is that of one serial chain.
 * cbc_gpu_encode_stream_blocks() runs the same general-form coder over ordinary (rebased) blocks, one stream per
 * block, in cbc_gpu_encode_blocks' output format: the fallback for blocks of more than CBC_MAX_BLOCK_READS records. */
typedef struct cbc_stream_result {
    uint64_t nbytes;       /* stream bytes written / records decoded                               */
    uint32_t status;       /* CBC_ST_*                                                              */
    uint32_t fail_read;    /* index (in stream order, low 32 bits) of the record being coded        */
    uint64_t n_symbols;
} cbc_stream_result;

int  cbc_gpu_encode_stream(cbc_gpu_ctx *ctx, const cbc_host_batch *batch, uint8_t *out, uint64_t out_cap,
                           cbc_stream_result *result);
int  cbc_gpu_encode_stream_blocks(cbc_gpu_ctx *ctx, const cbc_host_batch *batch, uint8_t *out, uint64_t out_cap,
                                  uint64_t *out_offsets /* n_blocks+1 */, cbc_block_result *results /* or NULL */);

/* The decode twin of cbc_gpu_encode_stream_blocks: block b's payload (in[in_off .. + in_bytes)) is decoded as a one-contig
 * stream whose contig is the block's reference window; records and bases go where cbc_gpu_decode_blocks would put them
 * (recs[rec_base ..], seq[seq_base + r * seq_stride]; cbc_read_rec.seq_off = r * seq_stride, .tok_off = 0). */
int  cbc_gpu_decode_stream_blocks(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const cbc_dec_block_desc *blocks,
                                  uint32_t n_blocks, cbc_read_rec *recs, uint64_t n_recs, uint8_t *seq, uint64_t seq_bytes,
                                  cbc_block_result *results /* n_blocks or NULL */);

/* Decode a whole-file stream.  contig_off[c] / contig_len[c]: where contig c (FASTA order) starts in the uploaded
 * reference and its length; the stream names contigs only by "next one" (decompress_line, compression.c:71-108).
 * recs[r] = { POS (1-based in its contig), FLAG, length, r * seq_stride (mod 2^32), contig index }, bases of record
 * r at seq[r * seq_stride].  result->nbytes = records decoded; CBC_ST_OUT_FULL with rec_cap too small (the caller
 * retries with larger buffers). */
int  cbc_gpu_decode_stream(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes,
                           const uint64_t *contig_off, const uint64_t *contig_len, uint32_t n_contigs,
                           cbc_read_rec *recs, uint64_t rec_cap, uint8_t *seq, uint64_t seq_bytes, uint32_t seq_stride,
                           cbc_stream_result *result);
/* header read length of a whole-file stream (its first four bytes come out verbatim), 0 if too short */
uint32_t cbc_stream_read_length(const uint8_t *in, uint64_t in_bytes);

/* ---- long-read format extension (stream version 3) ------------
 * Reads up to 65535 bases, POS steps up to 2^31, edits derived from read vs reference along the CIGAR -- everything
 * the reference's limits (include/sam_block.h:38,54, src/sam_models.c:317) exclude, so this is a format of its own:
 * no reference parity exists for it (oracle/cbc_long.c is its CPU statement).  Batches come from cbc_pack_sam /
 * cbc_synth_long with cbc_pack_opts.long_reads = 1; cbc_device_batch / cbc_dec_device_batch are used as in block
 * mode (caps.cap_var is ignored).  cbc_dec_block_desc.reserved[0] = bases of the block, seq_base = where they go
 * (the decoder writes the bases compactly; cbc_read_rec.seq_off = offset inside the block).
 * cbc_gpu_long_encode_blocks / cbc_gpu_long_decode_blocks go through the same pipeline as cbc_gpu_encode_blocks /
 * cbc_gpu_decode_blocks, as one chunk: their device arrays are the context's grow-only arenas (no allocation per call once
 * the arenas have their size), and they fill cbc_gpu_last_e2e.  The encode plans 0.5 bytes of payload per base and runs
 * the whole batch once more with the worst-case areas when a block reports CBC_ST_OUT_FULL; out == NULL is refused.
 * A call that fails before the blocks have run leaves every result's status at 0xffffffff.  The long decode returns zero
 * bytes in the parts of seq the decoder does not write, as the block decode does. */
uint64_t cbc_gpu_long_plan_output(cbc_block_desc *blocks, uint32_t n_blocks, const cbc_read_rec *recs, uint32_t bytes_per_16_bases);
uint32_t cbc_gpu_long_lds_bytes(const cbc_lds_caps *caps);
int  cbc_gpu_long_encode_blocks_device(cbc_gpu_ctx *ctx, const cbc_device_batch *batch, void *hip_stream);
int  cbc_gpu_long_decode_blocks_device(cbc_gpu_ctx *ctx, const cbc_dec_device_batch *batch, void *hip_stream);
int  cbc_gpu_long_encode_blocks(cbc_gpu_ctx *ctx, const cbc_host_batch *batch, uint8_t *out, uint64_t out_cap,
                                uint64_t *out_offsets /* n_blocks+1 */, cbc_block_result *results /* or NULL */);
int  cbc_gpu_long_decode_blocks(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, cbc_dec_block_desc *blocks,
                                uint32_t n_blocks, const cbc_lds_caps *caps, cbc_read_rec *recs, uint64_t n_recs,
                                uint8_t *seq, uint64_t seq_bytes, cbc_block_result *results /* or NULL */);

/* ---- 2-bit transport of bases over PCIe (layout: include/cbc_host.h cbc_2bit) ------------
 * The codec kernels read and write one byte per base in HBM; what crosses PCIe can be a quarter of that.  Host side:
 * cbc_2bit_pack() (libcbc_host).  Device side: an expand kernel (16 bases per lane: one code word in, one 16-byte
 * store out) followed by the exception runs, and the inverse pack kernel for decoded reads.
 *   cbc_gpu_upload_reference_2bit   reference as 2-bit codes + exception runs (N-runs, the pads) -> the same device
 *                                   reference cbc_gpu_upload_reference() makes (bit-identical bytes)
 *   cbc_gpu_encode_blocks_2bit      as cbc_gpu_encode_blocks, the batch's bases given as codes + runs (batch->seq may be
 *                                   NULL; batch->seq_bytes = number of bases incl. the 8 pad bytes)
 *   cbc_gpu_decode_blocks_2bit      as cbc_gpu_decode_blocks, but the bases come back as 2-bit rows: read r occupies
 *                                   words [r * row_words, (r + 1) * row_words) of codes_out (row_words = seq_stride / 16,
 *                                   seq_stride a multiple of 16), and every base of a read that is not A/C/G/T comes back
 *                                   in exc_idx[] (= r * seq_stride + position) / exc_val[]; *n_exc = how many (CBC_E_ARG if
 *                                   more than exc_cap) */
typedef struct cbc_2bit_run_dev { uint64_t start; uint32_t length; uint32_t byte; } cbc_2bit_run_dev;   /* = cbc_2bit_run */
int  cbc_gpu_upload_reference_2bit(cbc_gpu_ctx *ctx, const uint32_t *codes, uint64_t n_bases,
                                   const cbc_2bit_run_dev *runs, uint64_t n_runs);
int  cbc_gpu_encode_blocks_2bit(cbc_gpu_ctx *ctx, const cbc_host_batch *batch, const uint32_t *seq_codes,
                                const cbc_2bit_run_dev *seq_runs, uint64_t n_seq_runs,
                                uint8_t *out, uint64_t out_cap, uint64_t *out_offsets, cbc_block_result *results);
int  cbc_gpu_decode_blocks_2bit(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, cbc_dec_block_desc *blocks,
                                uint32_t n_blocks, const cbc_lds_caps *caps, cbc_read_rec *recs, uint64_t n_recs,
                                uint32_t *codes_out, uint64_t *exc_idx, uint8_t *exc_val, uint64_t exc_cap, uint64_t *n_exc,
                                cbc_block_result *results);

/* ---- SAM text -> packed records on the device (rules: cbc_amd/csrc/cbc_tok_core.h) ----------
 * load_sam_line(), src/sam_file_allocation.c:437-529, one GPU thread per line.  The text is copied to the device once;
 * bases and token words are produced in device memory (where cbc_gpu_encode_blocks_tokenised reads them) and the host
 * gets 16 bytes per mapped record + one change flag, from which libcbc_host's cbc_pack_from_device_tokens() cuts the
 * blocks exactly as cbc_pack_sam() does (the arrays are identical; tests).  status != 0: the first offending line
 * (bad_line, 0-based, '@' lines included) and why (CBC_TOK_* of cbc_tok_core.h: 3 = the file needs the host packer --
 * a leading soft clip or a record without MD -- 4.. = malformed input). */
typedef struct cbc_tok_record_summary { uint32_t pos; uint16_t flag, rl; uint32_t nt_ev /* words | var bound << 16 */; uint32_t line; } cbc_tok_record_summary;
typedef struct cbc_tok_result {
    uint64_t n_lines, n_recs, n_unmapped, seq_bytes /* without the 8 pad bytes */, n_tok;
    cbc_tok_record_summary *summaries;      /* host, n_recs                                                     */
    uint8_t  *rname_change;                 /* host, n_recs: RNAME differs from the previous mapped record's    */
    uint64_t *change_name_off; uint32_t *change_name_len; uint64_t n_changes;   /* host: where each new RNAME sits in the text */
    uint8_t  *d_seq; uint32_t *d_tok;       /* device: seq_bytes + 8 zero bytes; n_tok words                    */
    uint32_t status; uint64_t bad_line;
} cbc_tok_result;
int  cbc_gpu_tokenise_sam(cbc_gpu_ctx *ctx, const char *sam, uint64_t sam_len, uint64_t body_off, cbc_tok_result *out);
int  cbc_gpu_tokenise_fetch(cbc_gpu_ctx *ctx, const cbc_tok_result *t, uint8_t *seq /* seq_bytes + 8 */, uint32_t *tok /* n_tok */);
void cbc_gpu_tokenise_free(cbc_gpu_ctx *ctx, cbc_tok_result *t);
/* cbc_gpu_encode_blocks over a batch whose bases and tokens are the tokeniser's device arrays (batch->seq / tok unused) */
int  cbc_gpu_encode_blocks_tokenised(cbc_gpu_ctx *ctx, const cbc_tok_result *t, const cbc_host_batch *batch,
                                     uint8_t *out, uint64_t out_cap, uint64_t *out_offsets, cbc_block_result *results);

/* Timing of the most recent encode launch made through this context, measured with HIP events
 * recorded on the launch stream around the kernel (valid after the stream has been synchronised). */
int  cbc_gpu_last_kernel_ms(cbc_gpu_ctx *ctx, float *ms);
/* Which register budget of the encode kernel the most recent launch used: 5 or 6 wavefronts per SIMD
 * (cbc_encode_blocks_kernel / cbc_encode_blocks_kernel_w6; chosen from blocks per CU), 0 before any launch. */
int  cbc_gpu_last_kernel_variant(cbc_gpu_ctx *ctx);
int  cbc_gpu_synchronize(cbc_gpu_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* CBC_GPU_H */
