/*
 * cbc_host.h -- host side of the cbc hot path (libcbc_host.so, plain C): the record packer that
 * stands where the reference's tokeniser and FASTA loader stand, the block container, and the
 * seeded synthetic workload generator used by bench.py and the parity tests.
 *
 *   load_sam_line()              src/sam_file_allocation.c:437-529  -> cbc_pack_sam()
 *   get_read_length()            src/sam_file_allocation.c:26-79    -> cbc_packed.read_length
 *   store_reference_in_memory()  src/read_decompression.c:17-53     -> cbc_packed.ref
 *
 * No arithmetic coding happens on the host: payload bytes only ever come from the HIP kernels.
 */
#ifndef CBC_HOST_H
#define CBC_HOST_H

#include "cbc_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cbc_block_info {
    uint32_t contig;        /* index of the contig (order of appearance = FASTA record order)   */
    uint32_t n_reads;
    uint64_t window_start;  /* 0-based offset in the contig of the base that is local POS 1      */
    uint64_t n_bases;       /* sum of SEQ lengths                                                */
} cbc_block_info;

typedef struct cbc_contig_info {
    uint64_t ref_off;       /* offset of the contig's first base in cbc_packed.ref               */
    uint64_t length;
    uint32_t name_off;      /* offset of its NUL-terminated SAM RNAME in cbc_packed.names        */
    uint32_t reserved;
} cbc_contig_info;

typedef struct cbc_packed {
    cbc_read_rec    *recs;    uint64_t n_recs;
    uint8_t         *seq;     uint64_t seq_bytes;     /* includes 8 trailing pad bytes            */
    uint32_t        *tok;     uint64_t n_tok;
    uint8_t         *names;   uint32_t names_bytes;
    cbc_block_desc  *blocks;  uint32_t n_blocks;
    cbc_block_info  *info;
    cbc_contig_info *contigs; uint32_t n_contigs;
    uint8_t         *ref;     uint64_t ref_bytes;     /* contigs, each + CBC_REF_PAD zero bytes   */
    cbc_lds_caps     caps;
    uint32_t         read_length;                     /* header read length L0                    */
    uint64_t         n_bases;
    uint64_t         n_skipped_unmapped;
    uint32_t         max_read_len;                    /* longest SEQ packed                        */
    uint32_t         whole_file;                      /* 1: packed for the whole-file stream (cbc_pack_opts.whole_file); 2: long-read format */
    /* allocation bookkeeping (private) */
    uint64_t cap_recs, cap_seq, cap_tok, cap_ref; uint32_t cap_names, cap_blocks, cap_contigs;
} cbc_packed;

typedef struct cbc_pack_opts {
    uint32_t block_reads;   /* records per block (default 4096, max CBC_MAX_BLOCK_READS)          */
    uint32_t max_cap_pos;   /* cut a block before it needs more POS-delta entries (default 2048)  */
    uint32_t max_cap_var;   /* cut a block before it can hold more var symbols (default 8192)     */
    uint32_t var_length;    /* reference's -l: header read length = max over the file             */
    uint32_t n_threads;     /* text-path worker threads: 0 = one per online CPU, 1 = serial       */
    uint32_t whole_file;    /* 1 = "compat" mode: pack for ONE stream per file, the reference's own output format
                             * (compress(), src/compression.c:112-170): POS is NOT rebased, `blocks` become SEGMENTS
                             * (consecutive records of one contig; a new segment only at a contig change or when a
                             * 32-bit offset would overflow), caps.cap_pos counts the distinct POS steps of the whole
                             * file.  Inputs the reference cannot represent are refused: a POS step of 5 000 000 or
                             * more (MAX_ALPHA, sam_block.h:54), more than CBC_CAP_FLAG distinct FLAG values. */
    uint32_t long_reads;    /* 1 = the long-read format extension (stream version 3):
                             * SEQ up to CBC_LONG_MAX_READ_LEN bases and SAM lines of any length (the reference's limits
                             * are 252 bases / 1023 bytes), tokens = the CIGAR only (MD is ignored: edits are derived from
                             * read vs reference), blocks cut at block_reads (default 64) or CBC_LONG_BLOCK_BASES bases. */
} cbc_pack_opts;

#define CBC_LONG_MAX_READ_LEN 65535u
#define CBC_LONG_BLOCK_BASES  (1u << 20)

void cbc_pack_default_opts(cbc_pack_opts *o);

/* Tokenise SAM text + FASTA text into packed blocks.  errbuf receives a message on failure. */
int  cbc_pack_sam(const char *sam, size_t sam_len, const char *fasta, size_t fasta_len,
                  const cbc_pack_opts *opts, cbc_packed **out, char *errbuf, size_t errlen);
void cbc_packed_free(cbc_packed *p);

/* Seeded synthetic workload: one uniform-ACGT contig of `contig_len`
 * bases named `name`, `n_reads` reads of `read_len` bases at sorted uniform positions, FLAG in
 * {0,16}, per-base substitution rate `sub_rate`, `indel_frac` of reads with one 1..3-base
 * insertion or deletion >= 10 bases from either end, CIGAR M/I/D, MD:Z then NM:i.
 * Records go through the same path as cbc_pack_sam().  If sam_out/fasta_out are non-NULL the
 * equivalent SAM and FASTA text is returned too (malloc'ed, caller frees with cbc_free). */
typedef struct cbc_synth_opts {
    uint64_t seed;
    uint64_t contig_len;
    uint64_t n_reads;
    uint32_t read_len;
    double   sub_rate;
    double   indel_frac;
    const char *name;
} cbc_synth_opts;

int  cbc_synth_packed(const cbc_synth_opts *so, const cbc_pack_opts *po, cbc_packed **out,
                      char **sam_out, size_t *sam_len, char **fasta_out, size_t *fasta_len,
                      char *errbuf, size_t errlen);

/* cfg5 workload: long reads of `read_len` bases at sorted uniform positions on one uniform-ACGT
 * contig, FLAG in {0,16}; every aligned base is, with probability `edit_rate`, the site of one edit: substitution,
 * 1-base insertion or 1-base deletion (one third each).  Packed for the long-read format (long_reads = 1); the
 * generator runs on `po->n_threads` threads.  sam_out / fasta_out as in cbc_synth_packed (small cases only). */
int  cbc_synth_long(const cbc_synth_opts *so, const cbc_pack_opts *po, cbc_packed **out,
                    char **sam_out, size_t *sam_len, char **fasta_out, size_t *fasta_len,
                    char *errbuf, size_t errlen);
void cbc_free(void *p);

/* ---- block container (block mode of the CLI) ----------------------------------------------
 * magic "CBCB", version, header read length, contig table, block index, then the payloads.
 * Every payload follows the reference's stream grammar byte for byte. */
#define CBC_CONTAINER_MAGIC 0x42434243u   /* "CBCB" little-endian */
#define CBC_CONTAINER_VERSION 2u
#define CBC_CONTAINER_VERSION_LONG 3u     /* long-read format: same layout, per-block base counts in the index */

int64_t cbc_container_size(const cbc_packed *p, const uint64_t *out_offsets);
int64_t cbc_container_write(const cbc_packed *p, const uint8_t *payloads, const uint64_t *out_offsets,
                            uint8_t *dst, uint64_t dst_cap);

/* ---- the serial half of packing after the DEVICE tokeniser ------------------------------
 * cbc_gpu_tokenise_sam() (libcbc_gpu) turns the SAM text into bases, token words and one 16-byte summary per mapped
 * record; what is inherently serial -- contig numbering in file order, block cutting -- happens here, with the very
 * code path cbc_pack_sam() uses, so the resulting cbc_packed is identical to cbc_pack_sam()'s (tests).  seq / tok:
 * host copies of the tokeniser's arrays (then owned by the result) or NULL when they stay on the device (the result
 * then carries the sizes only).  summaries / rname_change / change_name_*: cbc_tok_result's arrays. */
int  cbc_pack_from_device_tokens(const char *sam, size_t sam_len, const char *fasta, size_t fasta_len, const cbc_pack_opts *opts,
                                 const void *summaries /* cbc_tok_record_summary[n_recs] */, const uint8_t *rname_change,
                                 const uint64_t *change_name_off, const uint32_t *change_name_len, uint64_t n_recs, uint64_t n_unmapped,
                                 uint8_t *seq, uint64_t seq_bytes, uint32_t *tok, uint64_t n_tok,
                                 cbc_packed **out, char *errbuf, size_t errlen);
/* offset of the first record line (behind the '@' header lines): the tokeniser's body_off */
uint64_t cbc_sam_body_offset(const char *sam, size_t sam_len);

/* ---- 2-bit transport of bases ------------------------------------------------
 * Bases travel to the device (reference, reads) and back (decoded reads) at 2 bits each: A C G T = 0 1 2 3, sixteen
 * bases per 32-bit word, base i in bits 2 (i & 15) of word i >> 4.  Every byte that is not one of 'A' 'C' 'G' 'T'
 * ('N', other IUPAC letters, the zero pad behind a contig) is an EXCEPTION, kept exactly: runs of one repeated byte
 * as (start, length, byte) -- an N-run of a chromosome is one entry -- so that unpacking restores the byte array
 * bit for bit (the match test compares bytes: src/read_compression.c:291-296).  cbc_2bit_pack runs on n_threads
 * threads (0 = one per CPU); cbc_2bit_unpack is the host inverse (the device inverse is cbc_gpu_expand_2bit). */
typedef struct cbc_2bit_run { uint64_t start; uint32_t length; uint32_t byte; } cbc_2bit_run;
typedef struct cbc_2bit {
    uint32_t     *codes;   uint64_t n_bases;     /* (n_bases + 15) / 16 words */
    cbc_2bit_run *runs;    uint64_t n_runs;      /* sorted by start, disjoint  */
} cbc_2bit;
int  cbc_2bit_pack(const uint8_t *bases, uint64_t n_bases, uint32_t n_threads, cbc_2bit **out);
int  cbc_2bit_unpack(const cbc_2bit *p, uint8_t *bases /* n_bases */);
void cbc_2bit_free(cbc_2bit *p);

/* ---- sharding over devices ---------------------------------------------------------
 * Blocks are independent streams; a contig's blocks share its reference, so whole contigs are dealt to the parts,
 * largest first, each to the part with the least records so far (cfg4: chromosome-sharded).  part_of_contig[c]
 * receives the part of contig c.  Deterministic: ties go to the lower part index. */
int  cbc_assign_contigs(const cbc_packed *p, uint32_t n_parts, uint32_t *part_of_contig /* n_contigs */);
/* host twin of cbc_gpu_checksum_device (include/cbc_gpu.h, CBC_CHECKSUM_TERM): what the receiving side of the bitstream
 * gather recomputes when the bytes arrive in host memory */
uint64_t cbc_checksum64(const uint8_t *bytes, uint64_t n);

/* ---- the reference alone (whole-file stream decode: the stream names contigs only by "next one") ----
 * FASTA text -> upper-cased contig bases, each + CBC_REF_PAD zero bytes, and the contig table in file order
 * (store_reference_in_memory, src/read_decompression.c:17-53).  Free with cbc_reference_free. */
typedef struct cbc_reference {
    uint8_t *bases; uint64_t n_bytes;
    uint64_t *contig_off, *contig_len; uint32_t n_contigs;
} cbc_reference;
int  cbc_reference_load(const char *fasta, size_t fasta_len, uint32_t n_threads, cbc_reference **out, char *errbuf, size_t errlen);
void cbc_reference_free(cbc_reference *r);

/* ---- unpack side: container + FASTA -> decode launch plan -> text ------------------------- */
typedef struct cbc_unpack_plan {
    cbc_dec_block_desc *blocks;   uint32_t n_blocks;
    const uint8_t      *payloads; uint64_t payload_bytes;   /* points into the caller's container blob */
    uint8_t            *ref;      uint64_t ref_bytes;       /* owned: contigs + pads, as the packer lays them out */
    uint64_t           *window_start;                        /* per block: add to a decoded POS for the contig POS */
    cbc_lds_caps        caps;
    uint32_t            read_length, seq_stride;
    uint64_t            n_recs;
    uint32_t            long_reads;                          /* container version 3: blocks[b].reserved[0] = bases of block b, */
    uint32_t            max_read_len;                        /* blocks[b].seq_base = where they start in the output (compact)  */
    uint64_t            seq_total;                           /* bytes of bases the decode writes (+ 8 spare)                   */
    /* the container's contig table, kept for region decode (cbc_unpack_region) */
    uint32_t           *block_contig;                        /* per block: its contig                                           */
    uint32_t            n_contigs;
    uint32_t            names_bytes;
    char               *names;                               /* owned copy of the names blob (NUL-terminated SAM RNAMEs)        */
    uint32_t           *contig_name_off;                     /* per contig: its name in names[] (checked to be inside it)       */
    uint64_t           *contig_len;                          /* per contig                                                      */
} cbc_unpack_plan;

/* Region decode.  `region` is NAME, NAME:BEG or NAME:BEG-END, 1-based and inclusive (samtools); a
 * string that is a contig name as a whole means that contig, otherwise it is split at the last ':'.  END is clamped to the
 * contig length.  The blocks [b0, b1) are the ones that can hold a read overlapping [beg, end]: with F(b) = window_start[b]
 * + 1 and smax = max_read_len + read_length - 1 (no read the decoder reconstructs covers more reference bases), block b of
 * the contig is selected iff F(b) <= end and (b is the contig's last block or F(next block) + smax >= beg + 1).
 * b0 == b1: no block can hold such a read.  Returns CBC_E_INPUT with a message for a malformed or unknown region, a
 * long-read (version 3) container, or a block index that is not in contig / position order. */
typedef struct cbc_region_sel {
    uint32_t contig;
    uint32_t b0, b1;        /* selected blocks: a contiguous run of the contig's blocks */
    uint32_t smax;          /* span bound the selection assumed (cbc_gpu_decode_region checks it) */
    uint64_t beg, end;      /* 1-based, inclusive, end clamped to the contig length */
    uint64_t contig_len;
} cbc_region_sel;
int     cbc_unpack_region(const cbc_unpack_plan *u, const char *region, cbc_region_sel *sel, char *errbuf, size_t errlen);

/* SAM output (the alignment lines come from cbc_gpu_decode_sam).  cbc_unpack_sam_header writes
 *     @HD\tVN:1.6\tSO:coordinate\n   and one   @SQ\tSN:<name>\tLN:<length>\n   per contig of the container's table, in table order
 * into dst (dst == NULL: only the size) and returns the bytes, CBC_E_ARG when cap is too small, or CBC_E_INPUT with a message:
 * a long-read (version 3) container; a name offset outside the name table; a name that is empty, longer than
 * CBC_SAM_MAX_NAME (255) bytes -- the limit the device path takes -- or holds a tab or a newline; a contig longer than
 * 2^31 - 1 bases (CBC_SAM_MAX_POS: SAM has no larger POS).  cbc_unpack_sam_text_cap: a text_cap that always holds the lines of
 * blocks [b0, b1) (0 for a plan the header function refuses or a bad range). */
int64_t  cbc_unpack_sam_header(const cbc_unpack_plan *u, char *dst, uint64_t cap, char *errbuf, size_t errlen);
uint64_t cbc_unpack_sam_text_cap(const cbc_unpack_plan *u, uint32_t b0, uint32_t b1);
/* The same for the lines with CIGAR, NM and MD (cbc_gpu_decode_sam_cigar) and an arena of edits_per_read
 * entries per read (0: CBC_EDITS_PER_READ): per block n_reads * (56 + len(RNAME) + 3 seq_stride + 16 edits_per_read); the proof
 * stands at the function.  0 also for edits_per_read above CBC_EDITS_MAX. */
uint64_t cbc_unpack_sam_cigar_text_cap(const cbc_unpack_plan *u, uint32_t b0, uint32_t b1, uint32_t edits_per_read);

/* Coverage output (the text comes from cbc_gpu_decode_depth).  cbc_unpack_contig_blocks: the
 * selection of contig `contig` as a whole -- its blocks [b0, b1) (b0 == b1: the contig has none), beg = 1, end = its length,
 * smax -- with the checks and errors of cbc_unpack_region (CBC_E_INPUT also when another contig carries the same name).
 * cbc_unpack_depth_text_cap: a text_cap that always holds the bedGraph of blocks [b0, b1) of contig `contig`: K reads give at
 * most 2K - 1 runs of at most len(name) + 34 bytes (0 for a plan cbc_unpack_sam_header refuses or a bad range). */
int      cbc_unpack_contig_blocks(const cbc_unpack_plan *u, uint32_t contig, cbc_region_sel *sel, char *errbuf, size_t errlen);
uint64_t cbc_unpack_depth_text_cap(const cbc_unpack_plan *u, uint32_t b0, uint32_t b1, uint32_t contig);

/* Per-position allele counts (the text comes from cbc_gpu_decode_pileup).  A text_cap that always holds
 * the lines of blocks [b0, b1) of contig `contig` for the window [beg, end] and the span bound smax of their selection: a line
 * per position of the window at most, and per reference base a kept read spans, of at most len(name) + 102 bytes each (0 for a
 * plan cbc_unpack_sam_header refuses, a bad range or a bad window).  The proof stands at the function. */
uint64_t cbc_unpack_pileup_text_cap(const cbc_unpack_plan *u, uint32_t b0, uint32_t b1, uint32_t contig, uint64_t beg, uint64_t end,
                                    uint32_t smax);
/* The same for cbc_gpu_decode_pileup_ext: by_strand = 1 adds seven columns of at most 11 bytes to every
 * line, len(name) + 102 + 7 * 11; the number of lines is bounded as above, and the fraction rule only takes lines away.
 * by_strand = 0 gives cbc_unpack_pileup_text_cap; anything but 0 or 1 gives 0. */
uint64_t cbc_unpack_pileup_ext_text_cap(const cbc_unpack_plan *u, uint32_t b0, uint32_t b1, uint32_t contig, uint64_t beg, uint64_t end,
                                        uint32_t smax, uint32_t by_strand);

/* Consensus (the record comes from cbc_gpu_decode_consensus).  cbc_unpack_consensus_text_cap: the bytes
 * of the record of window [beg, end] of contig `contig` when every position writes a byte -- the header (`>NAME\n`, or
 * `>NAME:BEG-END\n` with with_range = 1), w = end - beg + 1 bytes, ceil(w / line_width) newlines: exact under CBC_CONS_SHOW_DEL, a
 * bound otherwise (a called deletion drops its byte).  0 for a plan cbc_unpack_sam_header refuses, a bad contig or window,
 * line_width outside 1..65535 or with_range > 1.
 * cbc_unpack_consensus_empty: the record of a window that no block touches (a contig without reads, a region without blocks),
 * written on the host: every position is low depth, 'N', or with CBC_CONS_FILL_REF the plan's reference byte in lower case; a
 * position past the contig's end is written as 'N' (the selections of cbc_unpack_region and cbc_unpack_contig_blocks hold none).  Returns the bytes written, and in *counts emitted = low_depth = w; CBC_E_ARG for
 * the options cbc_gpu_decode_consensus refuses, a window the bound refuses, or text_cap below the bound. */
uint64_t cbc_unpack_consensus_text_cap(const cbc_unpack_plan *u, uint32_t contig, uint64_t beg, uint64_t end, uint32_t line_width,
                                       uint32_t with_range);
int64_t  cbc_unpack_consensus_empty(const cbc_unpack_plan *u, uint32_t contig, uint64_t beg, uint64_t end, const cbc_consensus_opts *opts,
                                    uint32_t with_range, uint8_t *text, uint64_t text_cap, cbc_consensus_counts *counts);

/* Deletion-aware coverage (the text comes from cbc_gpu_decode_depth after
 * cbc_gpu_set_depth_skip_deletions).  A deletion cuts a read's cover in two, so the 2K - 1 runs of cbc_unpack_depth_text_cap no
 * longer hold.  A text_cap that always holds the bedGraph of blocks [b0, b1) of contig `contig` for the window [beg, end] and the
 * span bound smax of their selection: a line per position of the window at most, and per reference base a kept read spans, of
 * at most len(name) + 34 bytes each (0 for a plan cbc_unpack_sam_header refuses, a bad range or a bad window).  The proof
 * stands at the function. */
uint64_t cbc_unpack_depth_skipdel_text_cap(const cbc_unpack_plan *u, uint32_t b0, uint32_t b1, uint32_t contig, uint64_t beg,
                                           uint64_t end, uint32_t smax);

/* Decode of a set of regions (the text comes from cbc_gpu_decode_targets).  The set is every string of
 * `regions` (parsed, clamped and refused exactly as cbc_unpack_region does) plus the lines of the BED text `bed` (bed_len bytes,
 * need not end in a newline or a NUL; NULL: none).  BED: fields separated by tabs or runs of spaces, at least `chrom start0 end0`
 * (0-based, half-open), further columns ignored; empty lines and lines starting with '#', "track" or "browser" are skipped; CRLF
 * line ends are taken; end0 past the contig's end is clamped.  A line with start0 == end0, a line naming a contig that is not in
 * the container's table (the packer lists only contigs that have reads) and a line starting at or past its contig's end select
 * nothing and are counted in bed_unselected.  start0 > end0, a number that is malformed or longer than 18 digits, fewer than
 * three columns or a line longer than CBC_BED_MAX_LINE bytes is CBC_E_INPUT with a message naming the line (1-based).
 * Per contig the intervals are sorted and merged where they overlap or touch (end + 1 >= next beg); contigs come in table order.
 * More than CBC_TARGETS_MAX_IV intervals after merging are refused, and so is what cbc_unpack_sam_header refuses (long-read
 * containers, names and lengths the text and the 32-bit device coordinates cannot carry).
 *   iv[contig_first[c] .. + contig_count[c])   contig c's merged intervals, 1-based inclusive
 *   blocks[n_blocks]                           the selected blocks, ascending: the union of the cbc_unpack_region selections
 *                                              of the merged intervals (the same rule, the same index check)
 *   block_iv[2 b], block_iv[2 b + 1]           for selected block b: first interval (index in iv) and count of the intervals
 *                                              its reads can reach: end >= F(b) and beg <= F(next block of the contig) + smax
 *   contig_blk_first / contig_blk_count        contig c's part of blocks[]
 * Free with cbc_targets_free. */
#define CBC_TARGETS_MAX_IV (1u << 24)
#define CBC_BED_MAX_LINE   65536u
typedef struct cbc_target_iv { uint32_t beg, end; } cbc_target_iv;
typedef struct cbc_targets {
    cbc_target_iv *iv;        uint32_t n_iv;
    uint32_t       n_contigs;
    uint32_t      *contig_first, *contig_count;
    uint32_t      *blocks;    uint32_t n_blocks;
    uint32_t       smax;
    uint32_t      *block_iv;
    uint32_t      *contig_blk_first, *contig_blk_count;
    uint64_t       bed_unselected;       /* BED lines that selected nothing */
    uint64_t       n_input;              /* regions + BED lines taken, before merging */
} cbc_targets;
int      cbc_unpack_targets(const cbc_unpack_plan *u, const char *const *regions, uint32_t n_regions, const char *bed, size_t bed_len,
                            cbc_targets **out, char *errbuf, size_t errlen);
void     cbc_targets_free(cbc_targets *t);
/* text_cap that always holds the output of the set: the sum of the per-block bounds of the selected blocks (sam = 0: rlen + 1
 * bytes per read; 1: the bound of cbc_unpack_sam_text_cap), and for the depth of contig c: K reads in its selected blocks and n
 * intervals change the depth at no more than 2K + 2n positions, so at most 2K + 2n - 1 runs of len(name) + 34 bytes (0: no
 * intervals or no blocks there, or a bad argument) */
uint64_t cbc_unpack_targets_text_cap(const cbc_unpack_plan *u, const cbc_targets *t, int sam);
uint64_t cbc_unpack_targets_depth_cap(const cbc_unpack_plan *u, const cbc_targets *t, uint32_t contig);
/* the depth of contig c under cbc_gpu_set_depth_skip_deletions: a line per position of the contig's merged intervals at most,
 * and per reference base a read of its selected blocks spans (t->smax), of len(name) + 34 bytes */
uint64_t cbc_unpack_targets_depth_skipdel_cap(const cbc_unpack_plan *u, const cbc_targets *t, uint32_t contig);

/* Per-target coverage summary (the numbers come from cbc_gpu_decode_coverage).  The QUERY list, in this
 * order and never merged or de-duplicated: every string of `regions` (parsed, clamped and refused as cbc_unpack_region does),
 * then every line of the BED text that cbc_unpack_targets would take or count in bed_unselected (the same parser, the same
 * errors) -- a line that selects nothing stays in the list with len = 0, so the list joins 1:1 with the input; with neither a
 * region nor a BED text, one query per contig of the container's table, the whole contig, in table order
 * (cbc_unpack_contig_blocks).  window > 0: every query is replaced by consecutive windows of `window` bases from its own
 * start on, the last one possibly shorter.  More than CBC_TARGETS_MAX_IV queries are CBC_E_INPUT with a message.
 *   q[i].contig            index in the container's table, CBC_QUERY_UNKNOWN for a BED line whose chrom is not in it
 *   q[i].beg, q[i].end     known contig: 1-based inclusive, both clamped to the contig's length; len = end + 1 - beg may be 0
 *                          (start0 == end0, or a start at or past the contig's end)
 *   q[i].slot              len > 0: the query's first slot in the compressed coordinate of its contig -- the contig's merged
 *                          intervals end to end, one spare slot behind each: the slots in front of the interval that holds
 *                          the query + beg - that interval's beg
 *   q[i].name_off/name_len unknown contig: the chrom text, bed[name_off .. + name_len)
 *   q[i].start0, q[i].end0 what the output echoes, 0-based half-open: beg - 1 and end for a known contig, the coordinates as
 *                          given (cut into windows like any other) for an unknown one
 *   targets                the cbc_targets that cbc_unpack_targets builds from the same (uncut) input
 * Free with cbc_queries_free. */
#define CBC_QUERY_UNKNOWN 0xffffffffu
typedef struct cbc_query {
    uint32_t contig, beg, end, slot;
    uint32_t name_off, name_len;
    uint64_t start0, end0;
} cbc_query;
typedef struct cbc_queries {
    cbc_query   *q;  uint64_t n_q;
    cbc_targets *targets;
} cbc_queries;
int      cbc_unpack_queries(const cbc_unpack_plan *u, const char *const *regions, uint32_t n_regions, const char *bed, size_t bed_len,
                            uint64_t window, cbc_queries **out, char *errbuf, size_t errlen);
void     cbc_queries_free(cbc_queries *q);
/* "<m / 100>.<two digits of m % 100>" of the mean sum / len rounded half up in integers: q = sum / len, r = sum % len,
 * m = q * 100 + (r * 100 + len / 2) / len; len == 0: "0.00".  Returns the characters written (dst holds at least 24). */
int      cbc_coverage_mean(uint64_t sum, uint64_t len, char *dst);

/* Depth histogram (the bins come from cbc_gpu_decode_depth_hist).  The interval table and the selected
 * blocks are those of cbc_unpack_targets, or of cbc_unpack_queries without regions for "every contig whole".
 * cbc_unpack_targets_size: the positions counted on contig c = the sum of the lengths of its merged intervals (0: none).
 * cbc_hist_fraction: "<m / 10^6>.<six digits of m % 10^6>" of bases / size rounded half up in integers,
 * m = (bases * 10^6 + size / 2) / size; size == 0: "0.000000".  Returns the characters written (dst holds at least 32). */
uint64_t cbc_unpack_targets_size(const cbc_targets *t, uint32_t contig);
int      cbc_hist_fraction(uint64_t bases, uint64_t size, char *dst);

/* Read statistics (the tables come from cbc_gpu_decode_stats).  cbc_stats_text writes what
 * `cbc -x --stats` writes, tab-separated, in this order: 11 SN lines (reads, reads excluded, bases, minimum length, maximum
 * length, average length, bases A, bases C, bases G, bases T, bases other), 15 FS lines (category, qc-passed, qc-failed; the
 * classes of `samtools flagstat`), then one FL line per FLAG value that occurs, one RL line per length that occurs, one GC line
 * per percent that occurs, each ascending, and one BC line per cycle 1 .. maximum length (A, C, G, T, other).  Every number is
 * an integer from the tables except the average length, which has two decimals by the rule of cbc_coverage_mean(bases, reads).
 * Minimum and maximum length are 0 and the average is "0.00" when there are no reads.  Returns the bytes written, or CBC_E_ARG
 * when cap is below cbc_stats_text_cap(), the size that holds the text of any tables (every line at its longest). */
uint64_t cbc_stats_text_cap(void);
int64_t  cbc_stats_text(const cbc_gpu_stats *s, char *dst, uint64_t cap);

/* The alignment tables of the read statistics (the tables come from cbc_gpu_decode_stats_aln).
 * cbc_stats_aln_text writes the sections `cbc -x --stats --alignment` appends to the text of cbc_stats_text, tab-separated, in
 * this order: 11 AS lines (reads, reads without alignment, bases aligned, mismatches, mismatch rate, insertions, deletions,
 * bases inserted, bases deleted, bases soft-clipped, reads with NM 0), one MC line `cycle, aligned, mismatches` per cycle
 * 1 .. the longest counted valid read, one IC line `cycle, insertions, deletions` per cycle 0 .. 256 where either is non-zero,
 * one ID line `length, insertions, deletions` per length 1 .. 255 where either is non-zero, one NM line `value, reads` per value
 * that occurs.  Every number is an integer derived from the tables in 64 bits -- aligned[c] = the reads of length >= c less
 * unal[c], bases soft-clipped = the sum of unal[] less bases inserted -- except the mismatch rate, which is
 * cbc_hist_fraction(mismatches, bases aligned).  Returns the bytes written, or CBC_E_ARG when cap is below
 * cbc_stats_aln_text_cap(). */
uint64_t cbc_stats_aln_text_cap(void);
int64_t  cbc_stats_aln_text(const cbc_gpu_stats_aln *a, char *dst, uint64_t cap);

int     cbc_unpack_plan_create(const uint8_t *blob, uint64_t len, const char *fasta, size_t fasta_len,
                               cbc_unpack_plan **out, char *errbuf, size_t errlen);
void    cbc_unpack_plan_free(cbc_unpack_plan *u);
int64_t cbc_unpack_write_text(const cbc_unpack_plan *u, const cbc_read_rec *recs, const uint8_t *seq,
                              char *dst, uint64_t cap);

#ifdef __cplusplus
}
#endif
#endif
