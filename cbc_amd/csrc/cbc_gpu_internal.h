/*
 * cbc_gpu_internal.h -- what the translation units of libcbc_gpu.so share on the host side: the context and its arenas, the
 * error helpers, the request a post-decode stage is described by, and the few host functions that cross a file boundary.
 * Not installed and not part of the C ABI (that is include/cbc_gpu.h).
 *
 *   cbc_gpu.hip         every codec kernel (block, span, edits, whole-file, long) and the utility kernels their pipelines
 *                       launch; the context; encode_blocks_impl / decode_blocks_impl; every entry point but the tokeniser's (the
 *                       cbc_gpu_decode_region ... _stats_aln ones with their checks and relayout_blocks are next to move out:
 *                       bench.py hashes this file for its measured kernels)
 *   cbc_gpu_post.hip    the post-decode stage of decode_blocks_impl: its kernels, post_arenas, post_h2d, the launch_* sequences
 *                       with post_launch to pick among them, post_fetch_sizes / post_fetch_output
 *   cbc_gpu_tok.hip     the tokeniser's kernels, scan_u32 and entry points
 *
 * A kernel is launched only from the file that defines it: a file that needs another's kernel calls a host function defined
 * beside it (launch_scan_sizes).  The functions declared here have hidden visibility like everything the Makefile builds
 * (-fvisibility=hidden); tests/test_gpu_exports.py holds the library to the C ABI.
 */
#ifndef CBC_GPU_INTERNAL_H
#define CBC_GPU_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>

#include "../../include/cbc_gpu.h"
#include "cbc_plan.h"               /* CBC_MAX_CHUNKS */

#define API extern "C" __attribute__((visibility("default")))
/* internal marker: "use the context's own stream" (host-buffer entry points only) */
#define CBC_CTX_STREAM ((void *)(uintptr_t)1)

/* grow-only device buffer owned by the context: the host-buffer entry points keep their device arrays between calls
 * (a hipMalloc / hipFree pair per array and call cost more than the copies they framed: profiles/r02_final_pcie.log) */
struct cbc_arena { void *p; uint64_t cap; };
enum { A_RECS, A_SEQ, A_TOK, A_NAMES, A_BLOCKS, A_OUT, A_RES, A_OFF, A_PACKED, A_CODES, A_RUNS, A_VS, A_IN, A_EXC_I, A_EXC_V, A_CNT, A_LSCR, A_STASH, A_GATHER, A_TEXT, A_RWS, A_RCNT, A_SNAMES, A_SBN, A_DDIFF, A_DTILE, A_DTOFF, A_DCP, A_DCTR, A_TIV, A_TBIV, A_TOFF, A_CVTILE, A_CVPRE, A_CVQ, A_CVOUT, A_HBINS, A_HTILE, A_HOUT, A_XSTARTS, A_XTILE, A_XSP, A_XTHR, A_XPRE, A_XOUT, A_STATS, A_ESIDE, A_EARENA, A_PTAB, A_CIGAR, A_SALN, A_COUNT };
#define CBC_N_KSTREAMS 8           /* every chunk's launch on a stream of its own: launches of different chunks share the chip */

/* what decode_blocks_impl runs behind the decode (its post-decode stage): nothing (plain, 2-bit, span, long reads), or the
 * stage of cbc_gpu_decode_region, _sam, _depth, _targets (reads, SAM, depth), _coverage, _depth_hist, _coverage_ext, _stats (whole
 * file, target set), _pileup, _sam_cigar, _stats_aln (whole file, target set), _consensus */
enum post_kind { POST_NONE, POST_REGION, POST_SAM, POST_DEPTH, POST_TG_READS, POST_TG_SAM, POST_TG_DEPTH, POST_COV, POST_HIST, POST_COVX,
                 POST_STATS, POST_TG_STATS, POST_COVQ, POST_PILEUP, POST_SAM_CIGAR, POST_STATS_ALN, POST_TG_STATS_ALN, POST_CONSENSUS };

struct cbc_gpu_ctx {
    int device;
    hipStream_t stream;
    hipStream_t s_copy;            /* H2D / D2H of the chunked host-buffer paths */
    hipStream_t s_k[CBC_N_KSTREAMS];   /* their kernel launches, chunk c on stream c % CBC_N_KSTREAMS */
    hipEvent_t ev0, ev1;
    hipEvent_t ev_chunk[CBC_MAX_CHUNKS], ev_done[CBC_N_KSTREAMS];
    hipEvent_t ev_rg[5];           /* region decode: before and after the decode, after the filter + scan, after the text kernel;
                                    * coverage: decode, mark, scan + compact, text (the fifth event) */
    hipEvent_t ev_cov[4];          /* cbc_gpu_decode_coverage: behind ev_rg[3], after the weights, their scans, the apply and the lookup */
    hipEvent_t ev_covx[5];         /* cbc_gpu_decode_coverage_ext: behind ev_cov[3], after the start points' scans + compact, the thresholds'
                                    * weights, their scans, their prefixes and the lookup */
    hipEvent_t ev_hist[2];         /* cbc_gpu_decode_depth_hist: behind ev_rg[3], after zeroing + accumulate and after the bin compaction */
    hipEvent_t ev_quant;           /* cbc_gpu_decode_coverage_quant: behind ev_covx[4], after the selection */
    uint32_t skipdel_edits;        /* cbc_gpu_set_depth_skip_deletions: > 0, the depth kinds count aligned bases only, behind the edits
                                    * decoder with that many arena entries per read; 0 (the default): the span depth */
    post_kind last_post;           /* whose times those events hold: the kind of the most recent call with a post-decode stage
                                    * (POST_NONE: none yet), set by post_launch and asked by the cbc_gpu_last_*_ms */
    int have_timing;
    int last_variant;              /* waves per SIMD of the encode build launched last */
    int n_cus;                     /* compute units of the device (block residency decides the kernel build) */
    uint8_t *d_ref; uint64_t ref_bytes;
    cbc_arena arena[A_COUNT];
    uint64_t stash_len;            /* bitstreams kept on the device by encode calls with out == NULL (cbc_gpu_group_gather moves them) */
    cbc_e2e_times last_e2e;
    char err[512];
};

/* cbc_gpu.hip */
int set_err(cbc_gpu_ctx *c, int code, const char *what, hipError_t e);
#define HIPCHK(call, what) do { hipError_t e_ = (call); if (e_ != hipSuccess) return set_err(ctx, CBC_E_NODEV, what, e_); } while (0)
/* the same inside a function that cleans up: `rc` takes the error and control goes to its `done:` label */
#define GO(call, what) do { hipError_t e_ = (call); if (e_ != hipSuccess) { rc = set_err(ctx, CBC_E_NODEV, what, e_); goto done; } } while (0)

/* at least `bytes` in arena k; growing frees the old buffer (hipFree waits for the device) */
int arena_need(cbc_gpu_ctx *ctx, int k, uint64_t bytes, const char *what);
#define NEED(k, bytes, what) do { rc = arena_need(ctx, k, bytes, what); if (rc) goto done; } while (0)

/* the first block whose status is not CBC_ST_OK becomes the call's error: "block <b> <verb> with status ..." */
int blocks_failed(cbc_gpu_ctx *ctx, const cbc_block_result *res, uint32_t n_blocks, const char *verb);

/* cbc_scan_sizes_kernel (cbc_gpu.hip), the exclusive scan every post-decode family runs over its sizes, on stream s */
void launch_scan_sizes(hipStream_t s, const cbc_block_result *sizes, uint64_t *offsets, uint32_t n);

static inline bool post_is_covx(post_kind k) { return k == POST_COVX || k == POST_COVQ; }
static inline bool post_is_cov(post_kind k) { return k == POST_COV || post_is_covx(k); }
/* PILEUP shares the depth kinds' arenas, counters and text fetch; it has no change points and its text tiles are the position tiles.
 * CONSENSUS is PILEUP up to the tile sums' scan, with its own call counters and two passes of its own behind */
static inline bool post_is_pileup(post_kind k) { return k == POST_PILEUP || k == POST_CONSENSUS; }
static inline bool post_is_depth(post_kind k) { return k == POST_DEPTH || k == POST_TG_DEPTH || post_is_cov(k) || k == POST_HIST || post_is_pileup(k); }
static inline bool post_is_sam(post_kind k) { return k == POST_SAM || k == POST_TG_SAM || k == POST_SAM_CIGAR; }
static inline bool post_is_targets(post_kind k) { return k == POST_TG_READS || k == POST_TG_SAM || k == POST_TG_DEPTH || post_is_cov(k) || k == POST_HIST || k == POST_TG_STATS || k == POST_TG_STATS_ALN; }
/* STATS_ALN is STATS behind the edits decoder with one more table and one more kernel */
static inline bool post_is_stats_aln(post_kind k) { return k == POST_STATS_ALN || k == POST_TG_STATS_ALN; }
static inline bool post_is_stats(post_kind k) { return k == POST_STATS || k == POST_TG_STATS || post_is_stats_aln(k); }

/* the queries (n_q pairs slot, len in the compressed coordinate), the depth that counts as covered, where the results go */
struct cov_req { const uint32_t *q; uint32_t n_q, min_depth; uint64_t *sum; uint32_t *covered;
                 /* COVX: the thresholds, where their n_q * n_thr counts go, where the read counts go (NULL: none) */
                 bool ext; const uint32_t *thr; uint32_t n_thr; uint32_t *thr_covered, *reads;
                 /* COVQ: the percentages, where the n_q * n_quant depths go */
                 const uint32_t *pct; uint32_t n_quant; uint32_t *quant; };
/* the depth from which the bins fold (2^32 - 1: none), where the pairs go (bin_cap of each) and how many there are */
struct hist_req { uint32_t fold; uint32_t *bin_depth, *bin_bases; uint32_t bin_cap; uint32_t *n_bins; };

/* What decode_blocks_impl does behind the decode of a one-chunk call.  `kind` alone says which post-decode stage runs;
 * the members below it are read by the kinds named in front of them and are zero otherwise. */
struct post_req {
    post_kind kind;
    uint32_t smax;                 /* > 0: the span-reporting decoder.  POST_NONE reads nothing else (cbc_gpu_decode_blocks_span) */
    /* every other kind: per block its window start, where the output text goes and what came of it (coverage and
     * histogram: text_cap = 0); n_selected = reads kept */
    const uint64_t *window_start;
    uint8_t *text; uint64_t text_cap; uint64_t *text_bytes, *n_selected;
    /* REGION, SAM, SAM_CIGAR, DEPTH: keep by [beg, end]; SAM with region == 0 keeps every read (smax = 0; SAM_CIGAR: the
     * container's span bound, its decoder reports spans).  Targets kinds: 1, 2^64 - 1 */
    uint64_t beg, end; int region;
    /* SAM, TG_SAM: the contig-name table and per block the (offset, length) of its name; depth kinds: the one contig name */
    const uint8_t *names; uint32_t names_bytes; const uint32_t *block_name;
    /* depth kinds: the flags that drop a read, where the number of runs goes */
    uint32_t exclude; uint64_t *n_runs;
    /* targets kinds: the interval table (n_iv pairs), per block its range of it, and for the depth kinds the first slot of
     * every interval in the compressed coordinate (n_iv + 1 entries) */
    const uint32_t *iv; uint32_t n_iv; const uint32_t *block_iv, *iv_off;
    cov_req cov;                   /* COV, COVX */
    hist_req hist;                 /* HIST */
    /* STATS, TG_STATS (with `exclude`): where the tables go, the record groups of the largest block */
    cbc_gpu_stats *stats; uint32_t stats_gmax;
    cbc_gpu_stats_aln *stats_aln;  /* STATS_ALN, TG_STATS_ALN (with edits_per_read): where the alignment tables go */
    /* edits_per_read > 0 (with smax > 0): the edit-reporting decoder.  SAM_CIGAR, STATS_ALN: nothing more; PILEUP: the line rule and the
     * contig's first reference byte; NONE (cbc_gpu_decode_blocks_edits): where the side array (2 words per record) and the arena go */
    uint32_t edits_per_read, min_alt; uint64_t ref_c0;
    /* PILEUP through cbc_gpu_decode_pileup_ext: the least alternative fraction in parts per million (0:
     * none) and whether the line carries the per-strand columns -- then the window holds two difference arrays and 14 planes */
    uint32_t min_alt_ppm; bool by_strand;
    uint32_t *edit_side; uint16_t *edit_arena;
    /* CONSENSUS (with edits_per_read and ref_c0 as for PILEUP): the rule's options, the header's form and
     * length, where the counters go.  text_bytes takes header + E + ceil(E / line_width) */
    cbc_consensus_opts cons; uint32_t with_range, cons_hdr; cbc_consensus_counts *cons_counts;
    /* the depth kinds but PILEUP, under cbc_gpu_set_depth_skip_deletions: deleted bases do not count -- the
     * edits decoder (edits_per_read is set with it) and the unmark stage behind the mark kernel */
    bool skip_del;
};

/* sizes derived from the request: tiles of the difference array (d_words = W + 1 words), change points (two per read at most,
 * two per interval edge -- more under skip_del, see post_sizes_of; start points: one per read and interval), text tiles of the runs, entries the text's size scan runs over; histogram: min(fold, reads) + 1 bins
 * in whole tiles, the non-zero ones are fewer than the bins and than the runs */
struct post_sizes { uint64_t d_words, h_bins; uint32_t n_tiles, cp_cap, n_ttiles, n_sized, n_btiles, h_out_cap, sp_cap; };

/* what post_fetch_sizes brings to the host for post_fetch_output; decode_blocks_impl zeroes it and frees cnt and stats */
struct post_got { uint32_t dctr[4], cctr[8]; /* CONSENSUS: the call counters */ uint64_t total, h_count; cbc_block_result *cnt; /* region / SAM / reads: the filter's per-block counts */
                  uint32_t *stats; /* STATS: the device's tables, CBC_STATS_WORDS; STATS_ALN: CBC_SALN_WORDS more behind them */ };

/* cbc_gpu_post.hip: the post-decode stage in the order decode_blocks_impl goes through it -- the sizes, the arenas, the small
 * tables H2D on the copy stream, the kind's launches on the decode's stream ks, the small results, the output */
post_sizes post_sizes_of(const post_req *rg, uint32_t n_blocks, uint64_t n_recs);
int post_arenas(cbc_gpu_ctx *ctx, const post_req *rg, const post_sizes &z, uint32_t n_blocks, uint64_t n_recs);
int post_h2d(cbc_gpu_ctx *ctx, const post_req *rg, uint32_t n_blocks, hipStream_t sc);
int post_launch(cbc_gpu_ctx *ctx, hipStream_t ks, const post_req *rg, const post_sizes &z, uint32_t n_blocks, uint64_t n_recs, uint64_t seq_bytes);
int post_fetch_sizes(cbc_gpu_ctx *ctx, const post_req *rg, const post_sizes &z, uint32_t n_blocks, hipStream_t sc, post_got *g);
int post_fetch_output(cbc_gpu_ctx *ctx, const post_req *rg, const post_sizes &z, uint32_t n_blocks, const cbc_block_result *res,
                      hipStream_t sc, const post_got *g, uint64_t *d2h_bytes);

#endif
