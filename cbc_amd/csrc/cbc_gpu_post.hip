/*
 * cbc_gpu_post.hip -- libcbc_gpu.so: the post-decode stage of decode_blocks_impl (cbc_gpu.hip) -- the kernels that turn decoded
 * records into text, depth, coverage numbers and statistics on the device, the launch sequence of every kind, and the stage's
 * arenas, copies and fetches.  The entry points that ask for a stage (cbc_gpu_decode_region ... _stats_aln) are in cbc_gpu.hip.
 */
#include "cbc_gpu_internal.h"
#include "cbc_wave_gpu.h"
#include "cbc_region_body.h"
#include "cbc_sam_body.h"
#include "cbc_depth_body.h"
#include "cbc_targets_body.h"
#include "cbc_cov_body.h"
#include "cbc_covx_body.h"
#include "cbc_quant_body.h"
#include "cbc_hist_body.h"
#include "cbc_stats_body.h"
#include "cbc_pileup_body.h"
#include "cbc_consensus_body.h"
#include "cbc_skipdel_body.h"
#include "cbc_cigar_body.h"
#include "cbc_stats_aln_body.h"

/* ------------------------------------------------------------------------------------------------
 * kernels
 * ---------------------------------------------------------------------------------------------- */
/* behind the edits decoder (cbc_decode_blocks_edits_kernel, cbc_gpu.hip): the unmark stage of the deletion-aware depth
 * (cbc_skipdel_body.h) and the per-position allele counts (cbc_pileup_body.h) -- behind cbc_depth_mark_kernel, CBC_PILEUP_WAVES
 * wavefronts per block add the events, and one wavefront per tile of positions counts and writes the lines */
__global__ void __launch_bounds__(64 * CBC_SKIPDEL_WAVES)
cbc_skipdel_unmark_kernel(cbc_skipdel_args A)
{
    if (blockIdx.x < A.D.R.n_blocks) cbc_skipdel_unmark<WaveGPU>(A, blockIdx.x, WaveGPU::uni(threadIdx.x >> 6), CBC_SKIPDEL_WAVES);
}
__global__ void __launch_bounds__(64 * CBC_SKIPDEL_WAVES)
cbc_skipdel_targets_unmark_kernel(cbc_tskipdel_args A)
{
    if (blockIdx.x < A.T.D.R.n_blocks) cbc_skipdel_targets_unmark<WaveGPU>(A, blockIdx.x, WaveGPU::uni(threadIdx.x >> 6), CBC_SKIPDEL_WAVES);
}
__global__ void __launch_bounds__(64 * CBC_PILEUP_WAVES)
cbc_pileup_events_kernel(cbc_pileup_args A)
{
    if (blockIdx.x < A.D.R.n_blocks) cbc_pileup_events<WaveGPU>(A, blockIdx.x, WaveGPU::uni(threadIdx.x >> 6), CBC_PILEUP_WAVES);
}
__global__ void __launch_bounds__(64)
cbc_pileup_count_kernel(cbc_pileup_args A) { cbc_pileup_count<WaveGPU>(A, blockIdx.x); }
__global__ void __launch_bounds__(64)
cbc_pileup_write_kernel(cbc_pileup_args A) { cbc_pileup_write<WaveGPU>(A, blockIdx.x); }
/* cbc_gpu_decode_pileup_ext: the events into the planes of the read's strand, and the line passes with
 * the fraction rule (M = CBC_PILEUP_FRAC) or with it and the per-strand columns (CBC_PILEUP_STRAND); the kernels above are the
 * plain call's and are not touched by it */
__global__ void __launch_bounds__(64 * CBC_PILEUP_WAVES)
cbc_pileup_events_strand_kernel(cbc_pileup_args A)
{
    if (blockIdx.x < A.D.R.n_blocks) cbc_pileup_events<WaveGPU, true>(A, blockIdx.x, WaveGPU::uni(threadIdx.x >> 6), CBC_PILEUP_WAVES);
}
template <int M> __global__ void __launch_bounds__(64)
cbc_pileup_count_ext_kernel(cbc_pileup_args A, cbc_pileup_sx X) { cbc_pileup_count<WaveGPU, M>(A, blockIdx.x, &X); }
template <int M> __global__ void __launch_bounds__(64)
cbc_pileup_write_ext_kernel(cbc_pileup_args A, cbc_pileup_sx X) { cbc_pileup_write<WaveGPU, M>(A, blockIdx.x, &X); }
/* cbc_gpu_decode_consensus (cbc_consensus_body.h): behind the plain call's mark, events and tile kernels
 * above, one wavefront per tile of positions applies the call rule and counts the bytes it emits, and (after the scan) writes them */
__global__ void __launch_bounds__(64)
cbc_consensus_count_kernel(cbc_consensus_args A) { cbc_consensus_count<WaveGPU>(A, blockIdx.x); }
__global__ void __launch_bounds__(64)
cbc_consensus_write_kernel(cbc_consensus_args A) { cbc_consensus_write<WaveGPU>(A, blockIdx.x); }

/* SAM text with CIGAR, NM and MD (cbc_gpu_decode_sam_cigar, cbc_cigar_body.h): behind the edits decoder CBC_CIGAR_WAVES wavefronts
 * per block measure every kept read's CIGAR, NM and MD; then the count (one wavefront per block) and the text assembly
 * (CBC_SAM_WAVES wavefronts per block) of the SAM text with the longer line */
__global__ void __launch_bounds__(64 * CBC_CIGAR_WAVES)
cbc_sam_cigar_measure_kernel(cbc_cigar_args A)
{
    if (blockIdx.x < A.S.R.n_blocks) cbc_cigar_measure<WaveGPU>(A, blockIdx.x, WaveGPU::uni(threadIdx.x >> 6), CBC_CIGAR_WAVES);
}
__global__ void __launch_bounds__(64)
cbc_sam_cigar_count_kernel(cbc_cigar_args A) { if (blockIdx.x < A.S.R.n_blocks) cbc_sam_cigar_count<WaveGPU>(A, blockIdx.x); }

__global__ void __launch_bounds__(64)
cbc_region_count_kernel(cbc_region_args A) { if (blockIdx.x < A.n_blocks) cbc_region_count<WaveGPU>(A, blockIdx.x); }

#define CBC_REGION_WAVES 4u
__global__ void __launch_bounds__(64 * CBC_REGION_WAVES)
cbc_region_write_kernel(cbc_region_args A)
{
    if (blockIdx.x >= A.n_blocks) return;
    cbc_region_write<WaveGPU>(A, blockIdx.x, WaveGPU::uni(threadIdx.x >> 6), CBC_REGION_WAVES);
}

/* SAM output (cbc_gpu_decode_sam, cbc_sam_body.h): line lengths per block (one wavefront per block), then the lines
 * (CBC_SAM_WAVES wavefronts per block, a line per wavefront at a time) */
__global__ void __launch_bounds__(64)
cbc_sam_count_kernel(cbc_sam_args A) { if (blockIdx.x < A.R.n_blocks) cbc_sam_count<WaveGPU>(A, blockIdx.x); }

#define CBC_SAM_WAVES 4u
__global__ void __launch_bounds__(64 * CBC_SAM_WAVES)
cbc_sam_write_kernel(cbc_sam_args A)
{
    if (blockIdx.x >= A.R.n_blocks) return;
    cbc_sam_write<WaveGPU>(A, blockIdx.x, WaveGPU::uni(threadIdx.x >> 6), CBC_SAM_WAVES);
}
__global__ void __launch_bounds__(64 * CBC_SAM_WAVES)
cbc_sam_cigar_write_kernel(cbc_cigar_args A)
{
    if (blockIdx.x >= A.S.R.n_blocks) return;
    cbc_sam_cigar_write<WaveGPU>(A, blockIdx.x, WaveGPU::uni(threadIdx.x >> 6), CBC_SAM_WAVES);
}

/* Coverage (cbc_gpu_decode_depth, cbc_depth_body.h): one wavefront per block marks the reads in the difference array, one
 * per tile sums it and (after the scans) writes the change points, one per CBC_DEPTH_LINES runs counts and writes the lines */
__global__ void __launch_bounds__(64)
cbc_depth_mark_kernel(cbc_depth_args A) { if (blockIdx.x < A.R.n_blocks) cbc_depth_mark<WaveGPU>(A, blockIdx.x); }
__global__ void __launch_bounds__(64)
cbc_depth_tile_kernel(cbc_depth_args A) { cbc_depth_tile<WaveGPU>(A, blockIdx.x); }
__global__ void __launch_bounds__(64)
cbc_depth_compact_kernel(cbc_depth_args A) { cbc_depth_compact<WaveGPU>(A, blockIdx.x); }
__global__ void __launch_bounds__(64)
cbc_depth_count_kernel(cbc_depth_args A) { if (blockIdx.x < A.n_ttiles) cbc_depth_count<WaveGPU>(A, blockIdx.x); }
__global__ void __launch_bounds__(64)
cbc_depth_write_kernel(cbc_depth_args A) { cbc_depth_write<WaveGPU>(A, blockIdx.x); }

/* A set of regions (cbc_gpu_decode_targets, cbc_targets_body.h): the count / write pairs of the region and the SAM text with
 * the keep rule over the interval table, and for the depth the mark and the text passes in the compressed coordinate (the
 * tile, scan and compact passes between them are the kernels above) */
__global__ void __launch_bounds__(64)
cbc_targets_count_kernel(cbc_targets_args A) { if (blockIdx.x < A.S.R.n_blocks) cbc_targets_count<WaveGPU>(A, blockIdx.x); }
__global__ void __launch_bounds__(64 * CBC_REGION_WAVES)
cbc_targets_write_kernel(cbc_targets_args A)
{
    if (blockIdx.x >= A.S.R.n_blocks) return;
    cbc_targets_write<WaveGPU>(A, blockIdx.x, WaveGPU::uni(threadIdx.x >> 6), CBC_REGION_WAVES);
}
__global__ void __launch_bounds__(64)
cbc_targets_sam_count_kernel(cbc_targets_args A) { if (blockIdx.x < A.S.R.n_blocks) cbc_targets_sam_count<WaveGPU>(A, blockIdx.x); }
__global__ void __launch_bounds__(64 * CBC_SAM_WAVES)
cbc_targets_sam_write_kernel(cbc_targets_args A)
{
    if (blockIdx.x >= A.S.R.n_blocks) return;
    cbc_targets_sam_write<WaveGPU>(A, blockIdx.x, WaveGPU::uni(threadIdx.x >> 6), CBC_SAM_WAVES);
}
__global__ void __launch_bounds__(64)
cbc_targets_mark_kernel(cbc_tdepth_args A) { if (blockIdx.x < A.D.R.n_blocks) cbc_targets_mark<WaveGPU>(A, blockIdx.x); }
__global__ void __launch_bounds__(64)
cbc_targets_depth_count_kernel(cbc_tdepth_args A) { if (blockIdx.x < A.D.n_ttiles) cbc_targets_depth_count<WaveGPU>(A, blockIdx.x); }
__global__ void __launch_bounds__(64)
cbc_targets_depth_write_kernel(cbc_tdepth_args A) { cbc_targets_depth_write<WaveGPU>(A, blockIdx.x); }

/* Per-query coverage summary (cbc_gpu_decode_coverage, cbc_cov_body.h), behind the mark / tile / scan / compact passes above:
 * one wavefront per CBC_DEPTH_LINES runs weighs them and (after the scans) stores the prefixes, one lane per query looks up */
__global__ void __launch_bounds__(64)
cbc_cov_weights_kernel(cbc_cov_args A) { cbc_cov_weights<WaveGPU>(A, blockIdx.x); }
__global__ void __launch_bounds__(64)
cbc_cov_apply_kernel(cbc_cov_args A) { cbc_cov_apply<WaveGPU>(A, blockIdx.x); }
__global__ void __launch_bounds__(64)
cbc_cov_lookup_kernel(cbc_cov_args A) { cbc_cov_lookup<WaveGPU>(A, blockIdx.x); }

/* Read counts and depth thresholds per query (cbc_gpu_decode_coverage_ext, cbc_covx_body.h): the mark pass that also notes
 * where every piece starts (the tile, scan and compact kernels above then run over the starts as they do over the difference
 * array), one wavefront per CBC_DEPTH_LINES runs for the thresholds' weights and prefixes, one lane per query for the lookup */
__global__ void __launch_bounds__(64)
cbc_targets_mark_starts_kernel(cbc_tdepth_args A, uint32_t *starts) { if (blockIdx.x < A.D.R.n_blocks) cbc_targets_mark<WaveGPU, true>(A, blockIdx.x, starts); }
__global__ void __launch_bounds__(64)
cbc_covx_weights_kernel(cbc_covx_args A) { cbc_covx_weights<WaveGPU>(A, blockIdx.x); }
__global__ void __launch_bounds__(64)
cbc_covx_apply_kernel(cbc_covx_args A) { cbc_covx_apply<WaveGPU>(A, blockIdx.x); }
__global__ void __launch_bounds__(64)
cbc_covx_lookup_kernel(cbc_covx_args A) { cbc_covx_lookup<WaveGPU>(A, blockIdx.x); }

/* Depth quantiles per query (cbc_gpu_decode_coverage_quant, cbc_quant_body.h), behind the passes above: one wavefront per query
 * selects all its quantiles from the runs it holds, in registers up to 64 runs and through its own LDS table beyond */
__global__ void __launch_bounds__(64)
cbc_quant_select_kernel(cbc_quant_args A)
{
    __shared__ uint32_t tab[CBC_QUANT_LDS];
    cbc_quant_select<WaveGPU>(A, blockIdx.x, tab);
}

/* Depth histogram (cbc_gpu_decode_depth_hist, cbc_hist_body.h), behind the same mark / tile / scan / compact passes: a bounded
 * grid of one-wavefront workgroups adds the runs' lengths to the bins of their depths (shallow bins in the workgroup's LDS table,
 * flushed once), then one wavefront per tile of bins counts and (after the scan) writes the non-zero ones as pairs */
__global__ void __launch_bounds__(64)
cbc_hist_accum_kernel(cbc_hist_args A)
{
#ifndef CBC_HIST_NO_LDS
    __shared__ uint32_t tab[CBC_HIST_LDS];
#else
    uint32_t *tab = NULL;
#endif
    cbc_hist_accum<WaveGPU>(A, blockIdx.x, tab);
}
__global__ void __launch_bounds__(64)
cbc_hist_count_kernel(cbc_hist_args A) { cbc_hist_count<WaveGPU>(A, blockIdx.x); }
__global__ void __launch_bounds__(64)
cbc_hist_write_kernel(cbc_hist_args A) { cbc_hist_write<WaveGPU>(A, blockIdx.x); }

/* Read statistics (cbc_gpu_decode_stats, cbc_stats_body.h), behind the plain decode or the span decode of a target set: a bounded
 * grid of workgroups of CBC_STATS_WAVES wavefronts strides over the record groups; the wavefronts of a workgroup share its count
 * tables in LDS (zero, barrier, accumulate, barrier, flush) */
template <bool TG>
static __device__ __forceinline__ void cbc_stats_workgroup(const cbc_stats_args &A)
{
    __shared__ uint32_t tab[CBC_STATS_LDS];
    const uint32_t wave = WaveGPU::uni(threadIdx.x >> 6);      /* wave-uniform: the unit's block and rows stay in scalar registers */
    cbc_stats_zero<WaveGPU>(tab, wave, CBC_STATS_WAVES);
    __syncthreads();
    cbc_stats_accum<WaveGPU, TG>(A, blockIdx.x, wave, CBC_STATS_WAVES, tab);
    __syncthreads();
    cbc_stats_flush<WaveGPU>(A, tab, wave, CBC_STATS_WAVES);
}
__global__ void __launch_bounds__(64 * CBC_STATS_WAVES)
cbc_stats_kernel(cbc_stats_args A) { cbc_stats_workgroup<false>(A); }
__global__ void __launch_bounds__(64 * CBC_STATS_WAVES)
cbc_targets_stats_kernel(cbc_stats_args A) { cbc_stats_workgroup<true>(A); }

/* The alignment tables of the statistics (cbc_gpu_decode_stats_aln, cbc_stats_aln_body.h), behind the edits decode and the
 * statistics kernel above: the same grid and workgroup shape over the same units, with its own count tables in LDS */
template <bool TG>
static __device__ __forceinline__ void cbc_stats_aln_workgroup(const cbc_stats_aln_args &A)
{
    __shared__ uint32_t tab[CBC_SALN_LDS];
    const uint32_t wave = WaveGPU::uni(threadIdx.x >> 6);
    cbc_stats_aln_zero<WaveGPU>(tab, wave, CBC_STATS_WAVES);
    __syncthreads();
    cbc_stats_aln_accum<WaveGPU, TG>(A, blockIdx.x, wave, CBC_STATS_WAVES, tab);
    __syncthreads();
    cbc_stats_aln_flush<WaveGPU>(A, tab, wave, CBC_STATS_WAVES);
}
__global__ void __launch_bounds__(64 * CBC_STATS_WAVES)
cbc_stats_aln_kernel(cbc_stats_aln_args A) { cbc_stats_aln_workgroup<false>(A); }
__global__ void __launch_bounds__(64 * CBC_STATS_WAVES)
cbc_targets_stats_aln_kernel(cbc_stats_aln_args A) { cbc_stats_aln_workgroup<true>(A); }

post_sizes post_sizes_of(const post_req *rg, uint32_t n_blocks, uint64_t n_recs)
{
    post_sizes z;
    memset(&z, 0, sizeof z);
    z.n_sized = n_blocks;
    if (!rg || !post_is_depth(rg->kind)) return z;
    const bool tg = post_is_targets(rg->kind);
    z.d_words = tg ? rg->iv_off[rg->n_iv] : rg->end - rg->beg + 2u;
    z.n_tiles = (uint32_t)((z.d_words + CBC_DEPTH_TILE - 1u) / CBC_DEPTH_TILE);
    z.cp_cap = (uint32_t)(2u * n_recs + (tg ? 2u * (uint64_t)rg->n_iv : 0u));
    if (rg->skip_del) {
        /* Change points under skip_del.  A change point is a non-zero word of the difference array, and a word is non-zero only
         * where somebody added to it.  The mark pass adds at two words per kept piece: at most 2 * n_recs (+ 2 * n_iv in the
         * compressed coordinate: the bound the span depth has).  The unmark pass adds at two words per deleted base it counts
         * (x and x + 1; neighbours share one, which only lowers the number), and it counts no base that has no arena entry.  A
         * block's arena holds at most n * edits_per_read entries -- a block that needs more has failed with CBC_ST_EDITS and
         * contributes nothing (cbc_region_block), and a hostile side array is held to the block's part of the arena by
         * cbc_edits_read_ok -- so the deleted bases of a call are at most n_recs * edits_per_read and the words at most
         * 2 * n_recs * (1 + edits_per_read) (+ 2 * n_iv).  No more words than the array has can be non-zero: min with d_words.
         * n_recs < 2^30 and edits_per_read <= 510: the product stays inside 64 bits, and d_words <= 2^31 + 2^24 + 1 fits the
         * 32-bit tables.  The compact pass refuses a tile that would write past cp_cap (cbc_depth_compact). */
        const uint64_t by_edits = 2u * n_recs * (1u + (uint64_t)rg->edits_per_read) + (tg ? 2u * (uint64_t)rg->n_iv : 0u);
        z.cp_cap = (uint32_t)(by_edits < z.d_words ? by_edits : z.d_words);
    }
    z.n_ttiles = (z.cp_cap + CBC_DEPTH_LINES - 1u) / CBC_DEPTH_LINES;
    if (post_is_pileup(rg->kind)) { z.cp_cap = 0; z.n_ttiles = z.n_tiles; }
    z.n_sized = z.n_ttiles;
    /* start points: a piece starts where its read starts or on an interval's first slot */
    if (post_is_covx(rg->kind)) z.sp_cap = (uint32_t)(n_recs + rg->n_iv);
    if (rg->kind != POST_HIST) return z;
    z.h_bins = (n_recs < rg->hist.fold ? n_recs : rg->hist.fold) + 1u;
    z.n_btiles = (uint32_t)((z.h_bins + CBC_DEPTH_TILE - 1u) / CBC_DEPTH_TILE);
    z.h_out_cap = (uint32_t)(z.h_bins - 1u < z.cp_cap ? z.h_bins - 1u : z.cp_cap);
    return z;
}

/* PILEUP's counter arena: seven planes of the difference array's size; by_strand: fourteen, behind them the forward reads'
 * difference array, its tile sums and non-zero counts and the scan of the sums (the second half of the 8 + 56 bytes per position) */
static uint64_t pileup_tab_bytes(const post_req *rg, const post_sizes &z)
{
    const uint64_t plane = (uint64_t)z.n_tiles * CBC_DEPTH_TILE * 4;
    if (!rg->by_strand) return plane * CBC_PILEUP_PLANES;
    return plane * (2u * CBC_PILEUP_PLANES + 1u) + (uint64_t)z.n_tiles * 2 * sizeof(cbc_block_result) + ((uint64_t)z.n_tiles + 1) * 8;
}

/* no device memory for an arena that grows with the change points: under skip_del the message names the option that grew it */
static int nomem_points(cbc_gpu_ctx *ctx, const post_req *rg, const char *what)
{
    char msg[256];
    (void)hipGetLastError();
    snprintf(msg, sizeof msg, "%s%s", what, rg->skip_del ? "; skip_deletions (--skip-deletions) sizes the change points by edits_per_read: "
             "lower edits_per_read (--max-edits-per-read) or take a smaller window" : "");
    return set_err(ctx, CBC_E_NOMEM, msg, hipSuccess);
}

/* post stage, step 1: its arenas */
int post_arenas(cbc_gpu_ctx *ctx, const post_req *rg, const post_sizes &z, uint32_t n_blocks, uint64_t n_recs)
{
    const post_kind k = rg->kind;
    int rc = CBC_OK;
    NEED(A_TEXT, rg->text_cap + 16, "hipMalloc region text");
    NEED(A_RWS, (uint64_t)n_blocks * 8, "hipMalloc window starts");
    NEED(A_RCNT, (uint64_t)z.n_sized * sizeof(cbc_block_result), "hipMalloc region counts");
    NEED(A_OFF, ((uint64_t)z.n_sized + 1) * 8, "hipMalloc region offsets");
    if (post_is_depth(k)) {
        if (arena_need(ctx, A_DDIFF, (uint64_t)z.n_tiles * CBC_DEPTH_TILE * 4, "hipMalloc depth window")) {
            (void)hipGetLastError();
            return set_err(ctx, CBC_E_NOMEM, "no device memory for the window's difference array (4 bytes per position)", hipSuccess);
        }
        NEED(A_DTILE, (uint64_t)z.n_tiles * 2 * sizeof(cbc_block_result), "hipMalloc depth tiles");
        NEED(A_DTOFF, ((uint64_t)z.n_tiles + 1) * 2 * 8, "hipMalloc depth tile offsets");
        if (arena_need(ctx, A_DCP, (uint64_t)z.cp_cap * 2 * 4 + 16, "hipMalloc depth change points"))
            return nomem_points(ctx, rg, "no device memory for the depth's change points (8 bytes each)");
        NEED(A_DCTR, k == POST_CONSENSUS ? 16 + 4 * CBC_CONS_CTRS + 4 : 16, "hipMalloc depth counters");   /* CONSENSUS: its call counters behind the four */
        NEED(A_SNAMES, (uint64_t)rg->names_bytes + 16, "hipMalloc contig name");
    }
    if (post_is_sam(k)) {
        NEED(A_SNAMES, (uint64_t)rg->names_bytes + 16, "hipMalloc contig names");
        NEED(A_SBN, (uint64_t)n_blocks * 8, "hipMalloc block names");
    }
    if (post_is_targets(k)) {
        NEED(A_TIV, (uint64_t)rg->n_iv * 8 + 16, "hipMalloc intervals");
        NEED(A_TBIV, (uint64_t)n_blocks * 8, "hipMalloc block intervals");
        if (post_is_depth(k)) NEED(A_TOFF, ((uint64_t)rg->n_iv + 1) * 4, "hipMalloc interval slots");
    }
    if (post_is_cov(k)) {
        NEED(A_CVTILE, (uint64_t)z.n_ttiles * 3 * sizeof(cbc_block_result) + ((uint64_t)z.n_ttiles + 1) * 3 * 8, "hipMalloc coverage tiles");
        if (arena_need(ctx, A_CVPRE, (uint64_t)z.cp_cap * 12 + 16, "hipMalloc coverage prefixes"))
            return nomem_points(ctx, rg, "no device memory for the coverage prefixes (12 bytes per change point)");
        NEED(A_CVQ, (uint64_t)rg->cov.n_q * 8 + 16, "hipMalloc coverage queries");
        NEED(A_CVOUT, (uint64_t)rg->cov.n_q * 12 + 16, "hipMalloc coverage results");
    }
    if (post_is_covx(k)) {
        const cov_req *cv = &rg->cov;
        if (cv->reads) {                                       /* the pieces' first slots: a second array of the difference array's size */
            if (arena_need(ctx, A_XSTARTS, (uint64_t)z.n_tiles * CBC_DEPTH_TILE * 4, "hipMalloc start slots")) {
                (void)hipGetLastError();
                return set_err(ctx, CBC_E_NOMEM, "no device memory for the pieces' start slots (4 bytes per position)", hipSuccess);
            }
            NEED(A_XTILE, (uint64_t)z.n_tiles * 2 * sizeof(cbc_block_result) + ((uint64_t)z.n_tiles + 1) * 2 * 8, "hipMalloc start tiles");
            NEED(A_XSP, (uint64_t)z.sp_cap * 2 * 4 + 16, "hipMalloc start points");
        }
        if (cv->n_thr) {
            NEED(A_XTHR, (uint64_t)cv->n_thr * (z.n_ttiles * sizeof(cbc_block_result) + ((uint64_t)z.n_ttiles + 1) * 8), "hipMalloc threshold tiles");
            if (arena_need(ctx, A_XPRE, (uint64_t)z.cp_cap * 4 * cv->n_thr + 16, "hipMalloc threshold prefixes"))
                return nomem_points(ctx, rg, "no device memory for the threshold prefixes (4 bytes per threshold and change point)");
        }
        NEED(A_XOUT, (uint64_t)cv->n_q * 4 * (cv->n_thr + 1ull + (k == POST_COVQ ? cv->n_quant : 0u)) + 16, "hipMalloc threshold and read counts");
    }
    if (k == POST_HIST) {
        if (arena_need(ctx, A_HBINS, (uint64_t)z.n_btiles * CBC_DEPTH_TILE * 4, "hipMalloc histogram bins") ||
            arena_need(ctx, A_HOUT, (uint64_t)z.h_out_cap * 8 + 16, "hipMalloc histogram pairs")) {
            (void)hipGetLastError();
            return set_err(ctx, CBC_E_NOMEM, "no device memory for the histogram's bins (4 bytes per bin, 8 per non-zero one)", hipSuccess);
        }
        NEED(A_HTILE, (uint64_t)z.n_btiles * sizeof(cbc_block_result) + ((uint64_t)z.n_btiles + 1) * 8, "hipMalloc histogram tiles");
    }
    if (post_is_stats(k)) NEED(A_STATS, (uint64_t)CBC_STATS_WORDS * 4, "hipMalloc statistics tables");
    if (post_is_stats_aln(k)) NEED(A_SALN, (uint64_t)CBC_SALN_WORDS * 4, "hipMalloc alignment tables");
    if (post_is_pileup(k) && arena_need(ctx, A_PTAB, pileup_tab_bytes(rg, z), "hipMalloc pileup counters")) {
        (void)hipGetLastError();
        return set_err(ctx, CBC_E_NOMEM, rg->by_strand ? "no device memory for the window's per-strand allele counters and forward difference array (56 + 4 bytes per position)"
                                                       : "no device memory for the window's allele counters (28 bytes per position)", hipSuccess);
    }
    if (k == POST_SAM_CIGAR) NEED(A_CIGAR, n_recs * 8 + 16, "hipMalloc measured CIGAR, NM and MD sizes");
done:
    return rc;
}

/* post stage, step 2: its small tables go H2D on the copy stream, behind the payloads */
int post_h2d(cbc_gpu_ctx *ctx, const post_req *rg, uint32_t n_blocks, hipStream_t sc)
{
    const post_kind k = rg->kind;
    HIPCHK(hipMemcpyAsync(ctx->arena[A_RWS].p, rg->window_start, (uint64_t)n_blocks * 8, hipMemcpyHostToDevice, sc), "H2D window starts");
    if (post_is_depth(k)) HIPCHK(hipMemcpyAsync(ctx->arena[A_SNAMES].p, rg->names, rg->names_bytes, hipMemcpyHostToDevice, sc), "H2D contig name");
    if (post_is_sam(k)) {
        HIPCHK(hipMemcpyAsync(ctx->arena[A_SNAMES].p, rg->names, rg->names_bytes, hipMemcpyHostToDevice, sc), "H2D contig names");
        HIPCHK(hipMemcpyAsync(ctx->arena[A_SBN].p, rg->block_name, (uint64_t)n_blocks * 8, hipMemcpyHostToDevice, sc), "H2D block names");
    }
    if (post_is_targets(k)) {
        HIPCHK(hipMemcpyAsync(ctx->arena[A_TIV].p, rg->iv, (uint64_t)rg->n_iv * 8, hipMemcpyHostToDevice, sc), "H2D intervals");
        HIPCHK(hipMemcpyAsync(ctx->arena[A_TBIV].p, rg->block_iv, (uint64_t)n_blocks * 8, hipMemcpyHostToDevice, sc), "H2D block intervals");
        if (post_is_depth(k)) HIPCHK(hipMemcpyAsync(ctx->arena[A_TOFF].p, rg->iv_off, ((uint64_t)rg->n_iv + 1) * 4, hipMemcpyHostToDevice, sc), "H2D interval slots");
    }
    if (post_is_cov(k)) HIPCHK(hipMemcpyAsync(ctx->arena[A_CVQ].p, rg->cov.q, (uint64_t)rg->cov.n_q * 8, hipMemcpyHostToDevice, sc), "H2D coverage queries");
    return CBC_OK;
}

/* post stage, step 3: the launches, on the decode's stream.  Every kind's kernels take the region arguments first. */
static void post_region_args(cbc_gpu_ctx *ctx, const post_req *rg, uint32_t n_blocks, uint64_t n_recs, uint64_t seq_bytes, cbc_region_args *ra)
{
    memset(ra, 0, sizeof *ra);
    ra->recs = (cbc_read_rec *)ctx->arena[A_RECS].p; ra->seq = (uint8_t *)ctx->arena[A_SEQ].p;
    ra->blocks = (cbc_dec_block_desc *)ctx->arena[A_BLOCKS].p; ra->window_start = (const uint64_t *)ctx->arena[A_RWS].p;
    ra->dec_results = (cbc_block_result *)ctx->arena[A_RES].p; ra->counts = (cbc_block_result *)ctx->arena[A_RCNT].p;
    ra->offsets = (const uint64_t *)ctx->arena[A_OFF].p;
    ra->text = (uint8_t *)ctx->arena[A_TEXT].p; ra->text_cap = rg->text_cap; ra->n_recs = n_recs; ra->seq_bytes = seq_bytes + 32;
    ra->beg = rg->beg; ra->end = rg->end; ra->n_blocks = n_blocks;
}

/* region text: filter + count, scan, write */
static int launch_region_text(cbc_gpu_ctx *ctx, hipStream_t ks, const cbc_region_args &ra)
{
    hipLaunchKernelGGL(cbc_region_count_kernel, dim3(ra.n_blocks), dim3(64), 0, ks, ra);
    HIPCHK(hipGetLastError(), "launch cbc_region_count_kernel");
    launch_scan_sizes(ks, ra.counts, (uint64_t *)ctx->arena[A_OFF].p, ra.n_blocks);
    HIPCHK(hipGetLastError(), "launch cbc_scan_sizes_kernel");
    HIPCHK(hipEventRecord(ctx->ev_rg[2], ks), "hipEventRecord");
    hipLaunchKernelGGL(cbc_region_write_kernel, dim3(ra.n_blocks), dim3(64 * CBC_REGION_WAVES), 0, ks, ra);
    HIPCHK(hipGetLastError(), "launch cbc_region_write_kernel");
    HIPCHK(hipEventRecord(ctx->ev_rg[3], ks), "hipEventRecord");
    return CBC_OK;
}

/* SAM text: the same three steps with the SAM bodies */
static int launch_sam_text(cbc_gpu_ctx *ctx, hipStream_t ks, const post_req *rg, const cbc_region_args &ra)
{
    cbc_sam_args sa;
    memset(&sa, 0, sizeof sa);
    sa.R = ra; sa.block_name = (const uint32_t *)ctx->arena[A_SBN].p; sa.names = (const uint8_t *)ctx->arena[A_SNAMES].p;
    sa.names_bytes = rg->names_bytes; sa.region = rg->region ? 1u : 0u;
    hipLaunchKernelGGL(cbc_sam_count_kernel, dim3(ra.n_blocks), dim3(64), 0, ks, sa);
    HIPCHK(hipGetLastError(), "launch cbc_sam_count_kernel");
    launch_scan_sizes(ks, ra.counts, (uint64_t *)ctx->arena[A_OFF].p, ra.n_blocks);
    HIPCHK(hipGetLastError(), "launch cbc_scan_sizes_kernel");
    HIPCHK(hipEventRecord(ctx->ev_rg[2], ks), "hipEventRecord");
    hipLaunchKernelGGL(cbc_sam_write_kernel, dim3(ra.n_blocks), dim3(64 * CBC_SAM_WAVES), 0, ks, sa);
    HIPCHK(hipGetLastError(), "launch cbc_sam_write_kernel");
    HIPCHK(hipEventRecord(ctx->ev_rg[3], ks), "hipEventRecord");
    return CBC_OK;
}

/* SAM text with CIGAR, NM and MD: the measure pass over the edits the decoder kept, then the same three steps with the longer line */
static int launch_sam_cigar_text(cbc_gpu_ctx *ctx, hipStream_t ks, const post_req *rg, const cbc_region_args &ra, uint64_t n_recs)
{
    cbc_cigar_args ca;
    memset(&ca, 0, sizeof ca);
    ca.S.R = ra; ca.S.block_name = (const uint32_t *)ctx->arena[A_SBN].p; ca.S.names = (const uint8_t *)ctx->arena[A_SNAMES].p;
    ca.S.names_bytes = rg->names_bytes; ca.S.region = rg->region ? 1u : 0u;
    ca.side = (const uint32_t *)ctx->arena[A_ESIDE].p; ca.arena = (const uint16_t *)ctx->arena[A_EARENA].p;
    ca.arena_entries = n_recs * rg->edits_per_read; ca.per_read = rg->edits_per_read;
    ca.ref = ctx->d_ref; ca.ref_bytes = ctx->ref_bytes; ca.meas = (uint32_t *)ctx->arena[A_CIGAR].p;
    hipLaunchKernelGGL(cbc_sam_cigar_measure_kernel, dim3(ra.n_blocks), dim3(64 * CBC_CIGAR_WAVES), 0, ks, ca);
    HIPCHK(hipGetLastError(), "launch cbc_sam_cigar_measure_kernel");
    HIPCHK(hipEventRecord(ctx->ev_rg[2], ks), "hipEventRecord");
    hipLaunchKernelGGL(cbc_sam_cigar_count_kernel, dim3(ra.n_blocks), dim3(64), 0, ks, ca);
    HIPCHK(hipGetLastError(), "launch cbc_sam_cigar_count_kernel");
    launch_scan_sizes(ks, ra.counts, (uint64_t *)ctx->arena[A_OFF].p, ra.n_blocks);
    HIPCHK(hipGetLastError(), "launch cbc_scan_sizes_kernel");
    HIPCHK(hipEventRecord(ctx->ev_rg[3], ks), "hipEventRecord");
    hipLaunchKernelGGL(cbc_sam_cigar_write_kernel, dim3(ra.n_blocks), dim3(64 * CBC_SAM_WAVES), 0, ks, ca);
    HIPCHK(hipGetLastError(), "launch cbc_sam_cigar_write_kernel");
    HIPCHK(hipEventRecord(ctx->ev_rg[4], ks), "hipEventRecord");
    return CBC_OK;
}

/* a set of regions, reads or SAM: the same three steps, kept by the interval table */
static int launch_targets_text(cbc_gpu_ctx *ctx, hipStream_t ks, const post_req *rg, const cbc_region_args &ra)
{
    const bool sam = rg->kind == POST_TG_SAM;
    cbc_targets_args ta;
    memset(&ta, 0, sizeof ta);
    ta.S.R = ra; ta.iv = (const uint32_t *)ctx->arena[A_TIV].p; ta.block_iv = (const uint32_t *)ctx->arena[A_TBIV].p; ta.n_iv = rg->n_iv;
    if (sam) {
        ta.S.block_name = (const uint32_t *)ctx->arena[A_SBN].p; ta.S.names = (const uint8_t *)ctx->arena[A_SNAMES].p;
        ta.S.names_bytes = rg->names_bytes;
        hipLaunchKernelGGL(cbc_targets_sam_count_kernel, dim3(ra.n_blocks), dim3(64), 0, ks, ta);
    } else hipLaunchKernelGGL(cbc_targets_count_kernel, dim3(ra.n_blocks), dim3(64), 0, ks, ta);
    HIPCHK(hipGetLastError(), "launch cbc_targets_count_kernel");
    launch_scan_sizes(ks, ra.counts, (uint64_t *)ctx->arena[A_OFF].p, ra.n_blocks);
    HIPCHK(hipGetLastError(), "launch cbc_scan_sizes_kernel");
    HIPCHK(hipEventRecord(ctx->ev_rg[2], ks), "hipEventRecord");
    if (sam) hipLaunchKernelGGL(cbc_targets_sam_write_kernel, dim3(ra.n_blocks), dim3(64 * CBC_SAM_WAVES), 0, ks, ta);
    else hipLaunchKernelGGL(cbc_targets_write_kernel, dim3(ra.n_blocks), dim3(64 * CBC_REGION_WAVES), 0, ks, ta);
    HIPCHK(hipGetLastError(), "launch cbc_targets_write_kernel");
    HIPCHK(hipEventRecord(ctx->ev_rg[3], ks), "hipEventRecord");
    return CBC_OK;
}

/* what every depth kind's kernels take, out of the context's arenas, with the difference array and the counters zeroed */
static int depth_args_zeroed(cbc_gpu_ctx *ctx, hipStream_t ks, const post_req *rg, const post_sizes &z, const cbc_region_args &ra, cbc_depth_args *da)
{
    const uint32_t n_tiles = z.n_tiles;
    memset(da, 0, sizeof *da);
    da->R = ra;
    da->diff = (uint32_t *)ctx->arena[A_DDIFF].p; da->diff_words = (uint64_t)n_tiles * CBC_DEPTH_TILE;
    da->tile_sum = (cbc_block_result *)ctx->arena[A_DTILE].p; da->tile_cnt = da->tile_sum + n_tiles;
    uint64_t *toff = (uint64_t *)ctx->arena[A_DTOFF].p;
    da->sum_off = toff; da->cnt_off = toff + n_tiles + 1;
    da->cp_pos = (uint32_t *)ctx->arena[A_DCP].p; da->cp_dep = da->cp_pos + z.cp_cap; da->cp_cap = z.cp_cap;
    da->ctr = (uint32_t *)ctx->arena[A_DCTR].p; da->name = (const uint8_t *)ctx->arena[A_SNAMES].p;
    da->name_len = rg->names_bytes; da->exclude = rg->exclude; da->n_tiles = n_tiles; da->n_ttiles = z.n_ttiles;
    HIPCHK(hipMemsetAsync(da->diff, 0, da->diff_words * 4, ks), "memset depth window");
    HIPCHK(hipMemsetAsync(da->ctr, 0, 16, ks), "memset depth counters");
    return CBC_OK;
}

static int launch_coverage_ext(cbc_gpu_ctx *ctx, hipStream_t ks, const cov_req *cov, const post_sizes &z, const cbc_depth_args &da, int reads_phase);

/* the front of every depth kind: mark, (skip_del: unmark,) tile sums, their two scans, the change points.  `da` and `ta` (filled
 * for the targets kinds, whose mark kernel reads the interval table) are what the tails go on with.  The unmark stage
 * (cbc_skipdel_body.h) takes the deleted bases of the kept reads off the difference array, on the same stream and inside the
 * mark stretch of the events.  The read counts of the coverage calls keep their span meaning under skip_del, and their formula
 * reads the depth at a query's first slot (cbc_covx_body.h): so they are taken from the SPAN depth, by a first run of the passes
 * behind the mark -- tile sums, scans, change points, then the start points and the lookup (launch_coverage_ext, phase 1) -- in
 * front of the unmark; the passes then run again over the unmarked array. */
static int launch_depth_front(cbc_gpu_ctx *ctx, hipStream_t ks, const post_req *rg, const post_sizes &z, const cbc_region_args &ra,
                              cbc_depth_args *da, cbc_tdepth_args *ta)
{
    const uint32_t n_tiles = z.n_tiles;
    uint64_t *toff = (uint64_t *)ctx->arena[A_DTOFF].p;
    int rc = depth_args_zeroed(ctx, ks, rg, z, ra, da);
    if (rc) return rc;
    memset(ta, 0, sizeof *ta);
    if (post_is_targets(rg->kind)) {
        ta->D = *da; ta->iv = (const uint32_t *)ctx->arena[A_TIV].p; ta->iv_off = (const uint32_t *)ctx->arena[A_TOFF].p;
        ta->block_iv = (const uint32_t *)ctx->arena[A_TBIV].p; ta->n_iv = rg->n_iv;
        if (post_is_covx(rg->kind) && rg->cov.reads) {        /* the mark that also notes the pieces' first slots */
            uint32_t *starts = (uint32_t *)ctx->arena[A_XSTARTS].p;
            HIPCHK(hipMemsetAsync(starts, 0, da->diff_words * 4, ks), "memset start slots");
            hipLaunchKernelGGL(cbc_targets_mark_starts_kernel, dim3(ra.n_blocks), dim3(64), 0, ks, *ta, starts);
        } else hipLaunchKernelGGL(cbc_targets_mark_kernel, dim3(ra.n_blocks), dim3(64), 0, ks, *ta);
    } else hipLaunchKernelGGL(cbc_depth_mark_kernel, dim3(ra.n_blocks), dim3(64), 0, ks, *da);
    HIPCHK(hipGetLastError(), "launch cbc_depth_mark_kernel");
    if (rg->skip_del && post_is_covx(rg->kind) && rg->cov.reads) {
        hipLaunchKernelGGL(cbc_depth_tile_kernel, dim3(n_tiles), dim3(64), 0, ks, *da);
        launch_scan_sizes(ks, da->tile_sum, toff, n_tiles);
        launch_scan_sizes(ks, da->tile_cnt, toff + n_tiles + 1, n_tiles);
        hipLaunchKernelGGL(cbc_depth_compact_kernel, dim3(n_tiles), dim3(64), 0, ks, *da);
        HIPCHK(hipGetLastError(), "launch the span depth's change points");
        if ((rc = launch_coverage_ext(ctx, ks, &rg->cov, z, *da, 1))) return rc;
    }
    if (rg->skip_del) {
        cbc_skipdel_edits se;
        memset(&se, 0, sizeof se);
        se.side = (const uint32_t *)ctx->arena[A_ESIDE].p; se.arena = (const uint16_t *)ctx->arena[A_EARENA].p;
        se.arena_entries = ra.n_recs * rg->edits_per_read; se.per_read = rg->edits_per_read;
        if (post_is_targets(rg->kind)) {
            cbc_tskipdel_args xa;
            xa.T = *ta; xa.E = se;
            hipLaunchKernelGGL(cbc_skipdel_targets_unmark_kernel, dim3(ra.n_blocks), dim3(64 * CBC_SKIPDEL_WAVES), 0, ks, xa);
        } else {
            cbc_skipdel_args xa;
            xa.D = *da; xa.E = se;
            hipLaunchKernelGGL(cbc_skipdel_unmark_kernel, dim3(ra.n_blocks), dim3(64 * CBC_SKIPDEL_WAVES), 0, ks, xa);
        }
        HIPCHK(hipGetLastError(), "launch cbc_skipdel_unmark_kernel");
    }
    HIPCHK(hipEventRecord(ctx->ev_rg[2], ks), "hipEventRecord");
    hipLaunchKernelGGL(cbc_depth_tile_kernel, dim3(n_tiles), dim3(64), 0, ks, *da);
    HIPCHK(hipGetLastError(), "launch cbc_depth_tile_kernel");
    launch_scan_sizes(ks, da->tile_sum, toff, n_tiles);
    launch_scan_sizes(ks, da->tile_cnt, toff + n_tiles + 1, n_tiles);
    HIPCHK(hipGetLastError(), "launch cbc_scan_sizes_kernel");
    hipLaunchKernelGGL(cbc_depth_compact_kernel, dim3(n_tiles), dim3(64), 0, ks, *da);
    HIPCHK(hipGetLastError(), "launch cbc_depth_compact_kernel");
    HIPCHK(hipEventRecord(ctx->ev_rg[3], ks), "hipEventRecord");
    return CBC_OK;
}

/* depth text: lines per text tile, scan, write; the targets kernels name the runs by their interval */
static int launch_depth_text(cbc_gpu_ctx *ctx, hipStream_t ks, bool tg, const post_sizes &z, const cbc_depth_args &da, const cbc_tdepth_args &ta)
{
    const uint32_t n_ttiles = z.n_ttiles;
    if (tg) hipLaunchKernelGGL(cbc_targets_depth_count_kernel, dim3(n_ttiles), dim3(64), 0, ks, ta);
    else hipLaunchKernelGGL(cbc_depth_count_kernel, dim3(n_ttiles), dim3(64), 0, ks, da);
    HIPCHK(hipGetLastError(), "launch cbc_depth_count_kernel");
    launch_scan_sizes(ks, da.R.counts, (uint64_t *)ctx->arena[A_OFF].p, n_ttiles);
    HIPCHK(hipGetLastError(), "launch cbc_scan_sizes_kernel");
    if (tg) hipLaunchKernelGGL(cbc_targets_depth_write_kernel, dim3(n_ttiles), dim3(64), 0, ks, ta);
    else hipLaunchKernelGGL(cbc_depth_write_kernel, dim3(n_ttiles), dim3(64), 0, ks, da);
    HIPCHK(hipGetLastError(), "launch cbc_depth_write_kernel");
    HIPCHK(hipEventRecord(ctx->ev_rg[4], ks), "hipEventRecord");
    return CBC_OK;
}

/* coverage: weights, their scans, prefixes, lookup: no text */
static int launch_coverage(cbc_gpu_ctx *ctx, hipStream_t ks, const cov_req *cov, const post_sizes &z, const cbc_depth_args &da)
{
    const uint32_t n_ttiles = z.n_ttiles, cp_cap = z.cp_cap;
    cbc_cov_args ca;
    memset(&ca, 0, sizeof ca);
    ca.cp_pos = da.cp_pos; ca.cp_dep = da.cp_dep; ca.cnt_off = da.cnt_off;
    ca.tile_wlo = (cbc_block_result *)ctx->arena[A_CVTILE].p; ca.tile_whi = ca.tile_wlo + n_ttiles; ca.tile_cov = ca.tile_whi + n_ttiles;
    uint64_t *woff = (uint64_t *)(ca.tile_cov + n_ttiles);
    ca.wlo_off = woff; ca.whi_off = woff + (n_ttiles + 1); ca.cov_off = woff + 2 * ((uint64_t)n_ttiles + 1);
    ca.pre_lo = (uint32_t *)ctx->arena[A_CVPRE].p; ca.pre_hi = ca.pre_lo + cp_cap; ca.pre_cov = ca.pre_hi + cp_cap;
    ca.q = (const uint32_t *)ctx->arena[A_CVQ].p; ca.sum = (uint32_t *)ctx->arena[A_CVOUT].p; ca.covered = ca.sum + 2 * (uint64_t)cov->n_q;
    ca.cp_cap = cp_cap; ca.n_tiles = z.n_tiles; ca.n_ttiles = n_ttiles; ca.n_q = cov->n_q; ca.min_depth = cov->min_depth;
    ca.slots = (uint32_t)z.d_words;
    hipLaunchKernelGGL(cbc_cov_weights_kernel, dim3(n_ttiles), dim3(64), 0, ks, ca);
    HIPCHK(hipGetLastError(), "launch cbc_cov_weights_kernel");
    HIPCHK(hipEventRecord(ctx->ev_cov[0], ks), "hipEventRecord");
    launch_scan_sizes(ks, ca.tile_wlo, woff, n_ttiles);
    launch_scan_sizes(ks, ca.tile_whi, woff + (n_ttiles + 1), n_ttiles);
    launch_scan_sizes(ks, ca.tile_cov, woff + 2 * ((uint64_t)n_ttiles + 1), n_ttiles);
    HIPCHK(hipGetLastError(), "launch cbc_scan_sizes_kernel");
    HIPCHK(hipEventRecord(ctx->ev_cov[1], ks), "hipEventRecord");
    hipLaunchKernelGGL(cbc_cov_apply_kernel, dim3(n_ttiles), dim3(64), 0, ks, ca);
    HIPCHK(hipGetLastError(), "launch cbc_cov_apply_kernel");
    HIPCHK(hipEventRecord(ctx->ev_cov[2], ks), "hipEventRecord");
    hipLaunchKernelGGL(cbc_cov_lookup_kernel, dim3((cov->n_q + 63u) / 64u), dim3(64), 0, ks, ca);
    HIPCHK(hipGetLastError(), "launch cbc_cov_lookup_kernel");
    HIPCHK(hipEventRecord(ctx->ev_cov[3], ks), "hipEventRecord");
    return CBC_OK;
}

/* read counts and thresholds, behind launch_coverage: the start points (tile sums, scans, compact over the starts), the
 * thresholds' weights, their scans and prefixes, the lookup.  A pass nobody asked for is not launched; its event still is.
 * reads_phase 0: all of it.  Under skip_del (launch_depth_front): 1 = the read counts alone, over the span depth's change points,
 * in front of the unmark; 2 = everything but the read counts, which are done. */
static int launch_coverage_ext(cbc_gpu_ctx *ctx, hipStream_t ks, const cov_req *cov, const post_sizes &z, const cbc_depth_args &da, int reads_phase)
{
    const uint32_t n_tiles = z.n_tiles, n_ttiles = z.n_ttiles, n_thr = reads_phase == 1 ? 0u : cov->n_thr;
    const bool want_reads = cov->reads && reads_phase != 2;
    cbc_covx_args xa;
    memset(&xa, 0, sizeof xa);
    xa.cp_pos = da.cp_pos; xa.cp_dep = da.cp_dep; xa.cnt_off = da.cnt_off;
    xa.q = (const uint32_t *)ctx->arena[A_CVQ].p;
    xa.thr_covered = (uint32_t *)ctx->arena[A_XOUT].p;
    xa.n_thr = n_thr; xa.cp_cap = z.cp_cap; xa.sp_cap = z.sp_cap; xa.n_tiles = n_tiles; xa.n_ttiles = n_ttiles; xa.n_q = cov->n_q;
    xa.slots = (uint32_t)z.d_words;
    for (uint32_t t = 0; t < n_thr; t++) xa.thr[t] = cov->thr[t];
    if (want_reads) {
        cbc_depth_args sa = da;                                /* the depth passes over the starts: CS in the place of the depth */
        sa.diff = (uint32_t *)ctx->arena[A_XSTARTS].p;
        sa.tile_sum = (cbc_block_result *)ctx->arena[A_XTILE].p; sa.tile_cnt = sa.tile_sum + n_tiles;
        uint64_t *soff = (uint64_t *)(sa.tile_cnt + n_tiles);
        sa.sum_off = soff; sa.cnt_off = soff + n_tiles + 1;
        sa.cp_pos = (uint32_t *)ctx->arena[A_XSP].p; sa.cp_dep = sa.cp_pos + z.sp_cap; sa.cp_cap = z.sp_cap;
        hipLaunchKernelGGL(cbc_depth_tile_kernel, dim3(n_tiles), dim3(64), 0, ks, sa);
        HIPCHK(hipGetLastError(), "launch cbc_depth_tile_kernel");
        launch_scan_sizes(ks, sa.tile_sum, soff, n_tiles);
        launch_scan_sizes(ks, sa.tile_cnt, soff + n_tiles + 1, n_tiles);
        HIPCHK(hipGetLastError(), "launch cbc_scan_sizes_kernel");
        hipLaunchKernelGGL(cbc_depth_compact_kernel, dim3(n_tiles), dim3(64), 0, ks, sa);
        HIPCHK(hipGetLastError(), "launch cbc_depth_compact_kernel");
        xa.sp_pos = sa.cp_pos; xa.sp_cnt = sa.cp_dep; xa.sp_off = sa.cnt_off;
        xa.reads = xa.thr_covered + (uint64_t)cov->n_q * cov->n_thr;
    }
    HIPCHK(hipEventRecord(ctx->ev_covx[0], ks), "hipEventRecord");
    if (n_thr) {
        xa.tile_thr = (cbc_block_result *)ctx->arena[A_XTHR].p;
        uint64_t *toff = (uint64_t *)(xa.tile_thr + (uint64_t)n_thr * n_ttiles);
        xa.thr_off = toff;
        xa.pre_thr = (uint32_t *)ctx->arena[A_XPRE].p;
        hipLaunchKernelGGL(cbc_covx_weights_kernel, dim3(n_ttiles), dim3(64), 0, ks, xa);
        HIPCHK(hipGetLastError(), "launch cbc_covx_weights_kernel");
        HIPCHK(hipEventRecord(ctx->ev_covx[1], ks), "hipEventRecord");
        for (uint32_t t = 0; t < n_thr; t++) launch_scan_sizes(ks, xa.tile_thr + (uint64_t)t * n_ttiles, toff + (uint64_t)t * (n_ttiles + 1u), n_ttiles);
        HIPCHK(hipGetLastError(), "launch cbc_scan_sizes_kernel");
        HIPCHK(hipEventRecord(ctx->ev_covx[2], ks), "hipEventRecord");
        hipLaunchKernelGGL(cbc_covx_apply_kernel, dim3(n_ttiles), dim3(64), 0, ks, xa);
        HIPCHK(hipGetLastError(), "launch cbc_covx_apply_kernel");
        HIPCHK(hipEventRecord(ctx->ev_covx[3], ks), "hipEventRecord");
    } else
        for (int k = 1; k < 4; k++) HIPCHK(hipEventRecord(ctx->ev_covx[k], ks), "hipEventRecord");
    if (n_thr || want_reads) {
        hipLaunchKernelGGL(cbc_covx_lookup_kernel, dim3((cov->n_q + 63u) / 64u), dim3(64), 0, ks, xa);
        HIPCHK(hipGetLastError(), "launch cbc_covx_lookup_kernel");
    }
    HIPCHK(hipEventRecord(ctx->ev_covx[4], ks), "hipEventRecord");
    return CBC_OK;
}

/* depth quantiles, behind launch_coverage_ext: one wavefront per query; its results behind the thresholds' and the read counts' */
static int launch_coverage_quant(cbc_gpu_ctx *ctx, hipStream_t ks, const cov_req *cov, const post_sizes &z, const cbc_depth_args &da)
{
    cbc_quant_args qa;
    memset(&qa, 0, sizeof qa);
    qa.cp_pos = da.cp_pos; qa.cp_dep = da.cp_dep; qa.cnt_off = da.cnt_off;
    qa.q = (const uint32_t *)ctx->arena[A_CVQ].p;
    qa.quant = (uint32_t *)ctx->arena[A_XOUT].p + (uint64_t)cov->n_q * (cov->n_thr + 1ull);
    qa.n_quant = cov->n_quant; qa.cp_cap = z.cp_cap; qa.n_tiles = z.n_tiles; qa.n_q = cov->n_q; qa.slots = (uint32_t)z.d_words;
    for (uint32_t t = 0; t < cov->n_quant; t++) qa.pct[t] = cov->pct[t];
    hipLaunchKernelGGL(cbc_quant_select_kernel, dim3(cov->n_q), dim3(64), 0, ks, qa);
    HIPCHK(hipGetLastError(), "launch cbc_quant_select_kernel");
    HIPCHK(hipEventRecord(ctx->ev_quant, ks), "hipEventRecord");
    return CBC_OK;
}

/* histogram: zero, accumulate, count + scan + write of the bins: no text */
static int launch_hist(cbc_gpu_ctx *ctx, hipStream_t ks, const hist_req *hist, const post_sizes &z, const cbc_depth_args &da)
{
    const uint32_t n_btiles = z.n_btiles;
    cbc_hist_args ha;
    memset(&ha, 0, sizeof ha);
    ha.cp_pos = da.cp_pos; ha.cp_dep = da.cp_dep; ha.cnt_off = da.cnt_off;
    ha.bins = (uint32_t *)ctx->arena[A_HBINS].p;
    ha.tile_nz = (cbc_block_result *)ctx->arena[A_HTILE].p;
    uint64_t *hoff = (uint64_t *)(ha.tile_nz + n_btiles);
    ha.nz_off = hoff;
    ha.out_depth = (uint32_t *)ctx->arena[A_HOUT].p; ha.out_bases = ha.out_depth + z.h_out_cap;
    ha.cp_cap = z.cp_cap; ha.n_tiles = z.n_tiles; ha.n_ttiles = z.n_ttiles; ha.fold = hist->fold;
    ha.n_bins = (uint32_t)z.h_bins; ha.n_btiles = n_btiles; ha.out_cap = z.h_out_cap;
    ha.grid = z.n_ttiles < CBC_HIST_GRID ? z.n_ttiles : CBC_HIST_GRID;
    HIPCHK(hipMemsetAsync(ha.bins, 0, (uint64_t)n_btiles * CBC_DEPTH_TILE * 4, ks), "memset histogram bins");
    hipLaunchKernelGGL(cbc_hist_accum_kernel, dim3(ha.grid), dim3(64), 0, ks, ha);
    HIPCHK(hipGetLastError(), "launch cbc_hist_accum_kernel");
    HIPCHK(hipEventRecord(ctx->ev_hist[0], ks), "hipEventRecord");
    hipLaunchKernelGGL(cbc_hist_count_kernel, dim3(n_btiles), dim3(64), 0, ks, ha);
    HIPCHK(hipGetLastError(), "launch cbc_hist_count_kernel");
    launch_scan_sizes(ks, ha.tile_nz, hoff, n_btiles);
    HIPCHK(hipGetLastError(), "launch cbc_scan_sizes_kernel");
    hipLaunchKernelGGL(cbc_hist_write_kernel, dim3(n_btiles), dim3(64), 0, ks, ha);
    HIPCHK(hipGetLastError(), "launch cbc_hist_write_kernel");
    HIPCHK(hipEventRecord(ctx->ev_hist[1], ks), "hipEventRecord");
    return CBC_OK;
}

/* per-position allele counts: zero, the depth's mark pass and the events; the depth's tile sums and their scan; lines per tile
 * of positions, scan, write */
static int launch_consensus(cbc_gpu_ctx *ctx, hipStream_t ks, const post_req *rg, const post_sizes &z, const cbc_pileup_args &pa);

static int launch_pileup(cbc_gpu_ctx *ctx, hipStream_t ks, const post_req *rg, const post_sizes &z, const cbc_region_args &ra, uint64_t n_recs)
{
    const uint32_t n_tiles = z.n_tiles;
    cbc_pileup_args pa;
    memset(&pa, 0, sizeof pa);
    int rc = depth_args_zeroed(ctx, ks, rg, z, ra, &pa.D);
    if (rc) return rc;
    pa.side = (const uint32_t *)ctx->arena[A_ESIDE].p; pa.arena = (const uint16_t *)ctx->arena[A_EARENA].p;
    pa.arena_entries = n_recs * rg->edits_per_read; pa.per_read = rg->edits_per_read;
    pa.ref = ctx->d_ref; pa.ref_bytes = ctx->ref_bytes; pa.ref_c0 = rg->ref_c0; pa.min_alt = rg->min_alt;
    pa.tab = (uint32_t *)ctx->arena[A_PTAB].p; pa.plane = pa.D.diff_words;
    const bool bs = rg->by_strand, ext = bs || rg->min_alt_ppm != 0u;
    const uint32_t planes = bs ? 2u * CBC_PILEUP_PLANES : CBC_PILEUP_PLANES;
    /* by_strand: behind the planes the forward reads' difference array, marked by the mark kernel under exclude | 16 with the
     * spare counter word [2] for its count, and the tile sums of that array with their scan */
    cbc_depth_args df = pa.D;
    cbc_pileup_sx sx;
    memset(&sx, 0, sizeof sx);
    sx.ppm = rg->min_alt_ppm;
    if (bs) {
        df.diff = pa.tab + pa.plane * planes; df.exclude = rg->exclude | 16u; df.ctr = pa.D.ctr + 2;
        df.tile_sum = (cbc_block_result *)(df.diff + pa.plane); df.tile_cnt = df.tile_sum + n_tiles;
        df.sum_off = (const uint64_t *)(df.tile_cnt + n_tiles);
        sx.diff_f = df.diff; sx.sum_off_f = df.sum_off;
    }
    HIPCHK(hipMemsetAsync(pa.tab, 0, pa.plane * 4 * (planes + (bs ? 1u : 0u)), ks), "memset pileup counters");
    hipLaunchKernelGGL(cbc_depth_mark_kernel, dim3(ra.n_blocks), dim3(64), 0, ks, pa.D);
    HIPCHK(hipGetLastError(), "launch cbc_depth_mark_kernel");
    if (bs) {
        hipLaunchKernelGGL(cbc_depth_mark_kernel, dim3(ra.n_blocks), dim3(64), 0, ks, df);
        HIPCHK(hipGetLastError(), "launch cbc_depth_mark_kernel");
        hipLaunchKernelGGL(cbc_pileup_events_strand_kernel, dim3(ra.n_blocks), dim3(64 * CBC_PILEUP_WAVES), 0, ks, pa);
    } else hipLaunchKernelGGL(cbc_pileup_events_kernel, dim3(ra.n_blocks), dim3(64 * CBC_PILEUP_WAVES), 0, ks, pa);
    HIPCHK(hipGetLastError(), "launch cbc_pileup_events_kernel");
    HIPCHK(hipEventRecord(ctx->ev_rg[2], ks), "hipEventRecord");
    hipLaunchKernelGGL(cbc_depth_tile_kernel, dim3(n_tiles), dim3(64), 0, ks, pa.D);
    HIPCHK(hipGetLastError(), "launch cbc_depth_tile_kernel");
    launch_scan_sizes(ks, pa.D.tile_sum, (uint64_t *)ctx->arena[A_DTOFF].p, n_tiles);
    if (bs) {
        hipLaunchKernelGGL(cbc_depth_tile_kernel, dim3(n_tiles), dim3(64), 0, ks, df);
        HIPCHK(hipGetLastError(), "launch cbc_depth_tile_kernel");
        launch_scan_sizes(ks, df.tile_sum, (uint64_t *)df.sum_off, n_tiles);
    }
    if (rg->kind == POST_CONSENSUS) return launch_consensus(ctx, ks, rg, z, pa);
    if (bs) hipLaunchKernelGGL(cbc_pileup_count_ext_kernel<CBC_PILEUP_STRAND>, dim3(n_tiles), dim3(64), 0, ks, pa, sx);
    else if (ext) hipLaunchKernelGGL(cbc_pileup_count_ext_kernel<CBC_PILEUP_FRAC>, dim3(n_tiles), dim3(64), 0, ks, pa, sx);
    else hipLaunchKernelGGL(cbc_pileup_count_kernel, dim3(n_tiles), dim3(64), 0, ks, pa);
    HIPCHK(hipGetLastError(), "launch cbc_pileup_count_kernel");
    launch_scan_sizes(ks, ra.counts, (uint64_t *)ctx->arena[A_OFF].p, n_tiles);
    HIPCHK(hipGetLastError(), "launch cbc_scan_sizes_kernel");
    HIPCHK(hipEventRecord(ctx->ev_rg[3], ks), "hipEventRecord");
    if (bs) hipLaunchKernelGGL(cbc_pileup_write_ext_kernel<CBC_PILEUP_STRAND>, dim3(n_tiles), dim3(64), 0, ks, pa, sx);
    else if (ext) hipLaunchKernelGGL(cbc_pileup_write_ext_kernel<CBC_PILEUP_FRAC>, dim3(n_tiles), dim3(64), 0, ks, pa, sx);
    else hipLaunchKernelGGL(cbc_pileup_write_kernel, dim3(n_tiles), dim3(64), 0, ks, pa);
    HIPCHK(hipGetLastError(), "launch cbc_pileup_write_kernel");
    HIPCHK(hipEventRecord(ctx->ev_rg[4], ks), "hipEventRecord");
    return CBC_OK;
}

/* the consensus behind the pileup's front: its counters zeroed, the call count per tile of positions, its scan, the record */
static int launch_consensus(cbc_gpu_ctx *ctx, hipStream_t ks, const post_req *rg, const post_sizes &z, const cbc_pileup_args &pa)
{
    cbc_consensus_args ca;
    memset(&ca, 0, sizeof ca);
    ca.P = pa; ca.cctr = pa.D.ctr + 4;
    ca.min_depth = rg->cons.min_depth; ca.ppm = rg->cons.call_ppm; ca.line_width = rg->cons.line_width; ca.flags = rg->cons.flags;
    ca.with_range = rg->with_range;
    HIPCHK(hipMemsetAsync(ca.cctr, 0, 4 * CBC_CONS_CTRS, ks), "memset consensus counters");
    hipLaunchKernelGGL(cbc_consensus_count_kernel, dim3(z.n_tiles), dim3(64), 0, ks, ca);
    HIPCHK(hipGetLastError(), "launch cbc_consensus_count_kernel");
    launch_scan_sizes(ks, pa.D.R.counts, (uint64_t *)ctx->arena[A_OFF].p, z.n_tiles);
    HIPCHK(hipGetLastError(), "launch cbc_scan_sizes_kernel");
    HIPCHK(hipEventRecord(ctx->ev_rg[3], ks), "hipEventRecord");
    hipLaunchKernelGGL(cbc_consensus_write_kernel, dim3(z.n_tiles), dim3(64), 0, ks, ca);
    HIPCHK(hipGetLastError(), "launch cbc_consensus_write_kernel");
    HIPCHK(hipEventRecord(ctx->ev_rg[4], ks), "hipEventRecord");
    return CBC_OK;
}

/* read statistics: zero the tables, one pass over the records and rows: no text */
static int launch_stats(cbc_gpu_ctx *ctx, hipStream_t ks, const post_req *rg, const cbc_region_args &ra)
{
    cbc_stats_args sa;
    memset(&sa, 0, sizeof sa);
    sa.R = ra; sa.tab = (uint32_t *)ctx->arena[A_STATS].p; sa.exclude = rg->exclude; sa.gmax = rg->stats_gmax;
    const uint64_t units = (uint64_t)ra.n_blocks * sa.gmax, wgs = (units + CBC_STATS_WAVES - 1u) / CBC_STATS_WAVES;
    sa.grid = wgs < CBC_STATS_GRID ? (uint32_t)wgs : CBC_STATS_GRID;
    HIPCHK(hipMemsetAsync(sa.tab, 0, (uint64_t)CBC_STATS_WORDS * 4, ks), "memset statistics tables");
    if (post_is_stats_aln(rg->kind)) HIPCHK(hipMemsetAsync(ctx->arena[A_SALN].p, 0, (uint64_t)CBC_SALN_WORDS * 4, ks), "memset alignment tables");
    if (sa.grid) {
        if (post_is_targets(rg->kind)) {
            sa.iv = (const uint32_t *)ctx->arena[A_TIV].p; sa.block_iv = (const uint32_t *)ctx->arena[A_TBIV].p; sa.n_iv = rg->n_iv;
            hipLaunchKernelGGL(cbc_targets_stats_kernel, dim3(sa.grid), dim3(64 * CBC_STATS_WAVES), 0, ks, sa);
        } else hipLaunchKernelGGL(cbc_stats_kernel, dim3(sa.grid), dim3(64 * CBC_STATS_WAVES), 0, ks, sa);
        HIPCHK(hipGetLastError(), "launch cbc_stats_kernel");
    }
    HIPCHK(hipEventRecord(ctx->ev_rg[2], ks), "hipEventRecord");
    if (!post_is_stats_aln(rg->kind)) return CBC_OK;
    /* the alignment pass over the same units: the side array and arena the edits decoder has left, the device reference */
    cbc_stats_aln_args aa;
    memset(&aa, 0, sizeof aa);
    aa.S = sa; aa.tab = (uint32_t *)ctx->arena[A_SALN].p;
    aa.side = (const uint32_t *)ctx->arena[A_ESIDE].p; aa.arena = (const uint16_t *)ctx->arena[A_EARENA].p;
    aa.arena_entries = ra.n_recs * rg->edits_per_read; aa.per_read = rg->edits_per_read;
    aa.ref = ctx->d_ref; aa.ref_bytes = ctx->ref_bytes;
    if (sa.grid) {
        if (post_is_targets(rg->kind)) hipLaunchKernelGGL(cbc_targets_stats_aln_kernel, dim3(sa.grid), dim3(64 * CBC_STATS_WAVES), 0, ks, aa);
        else hipLaunchKernelGGL(cbc_stats_aln_kernel, dim3(sa.grid), dim3(64 * CBC_STATS_WAVES), 0, ks, aa);
        HIPCHK(hipGetLastError(), "launch cbc_stats_aln_kernel");
    }
    HIPCHK(hipEventRecord(ctx->ev_rg[3], ks), "hipEventRecord");
    return CBC_OK;
}

/* ... and the one sequence of them that the request's kind picks, behind the decode on its stream ks */
int post_launch(cbc_gpu_ctx *ctx, hipStream_t ks, const post_req *rg, const post_sizes &z, uint32_t n_blocks, uint64_t n_recs, uint64_t seq_bytes)
{
    cbc_region_args ra;
    cbc_depth_args da;
    cbc_tdepth_args ta;
    int rc = CBC_OK;
    post_region_args(ctx, rg, n_blocks, n_recs, seq_bytes, &ra);
    switch (rg->kind) {
    case POST_NONE: break;
    case POST_REGION: rc = launch_region_text(ctx, ks, ra); break;
    case POST_SAM: rc = launch_sam_text(ctx, ks, rg, ra); break;
    case POST_TG_READS: case POST_TG_SAM: rc = launch_targets_text(ctx, ks, rg, ra); break;
    case POST_DEPTH: case POST_TG_DEPTH:
        rc = launch_depth_front(ctx, ks, rg, z, ra, &da, &ta);
        if (!rc) rc = launch_depth_text(ctx, ks, rg->kind == POST_TG_DEPTH, z, da, ta);
        break;
    case POST_COV:
        rc = launch_depth_front(ctx, ks, rg, z, ra, &da, &ta);
        if (!rc) rc = launch_coverage(ctx, ks, &rg->cov, z, da);
        break;
    case POST_COVX:
        rc = launch_depth_front(ctx, ks, rg, z, ra, &da, &ta);
        if (!rc) rc = launch_coverage(ctx, ks, &rg->cov, z, da);
        if (!rc) rc = launch_coverage_ext(ctx, ks, &rg->cov, z, da, rg->skip_del && rg->cov.reads ? 2 : 0);
        break;
    case POST_COVQ:
        rc = launch_depth_front(ctx, ks, rg, z, ra, &da, &ta);
        if (!rc) rc = launch_coverage(ctx, ks, &rg->cov, z, da);
        if (!rc) rc = launch_coverage_ext(ctx, ks, &rg->cov, z, da, rg->skip_del && rg->cov.reads ? 2 : 0);
        if (!rc) rc = launch_coverage_quant(ctx, ks, &rg->cov, z, da);
        break;
    case POST_HIST:
        rc = launch_depth_front(ctx, ks, rg, z, ra, &da, &ta);
        if (!rc) rc = launch_hist(ctx, ks, &rg->hist, z, da);
        break;
    case POST_STATS: case POST_TG_STATS: case POST_STATS_ALN: case POST_TG_STATS_ALN: rc = launch_stats(ctx, ks, rg, ra); break;
    case POST_PILEUP: case POST_CONSENSUS: rc = launch_pileup(ctx, ks, rg, z, ra, n_recs); break;
    case POST_SAM_CIGAR: rc = launch_sam_cigar_text(ctx, ks, rg, ra, n_recs); break;
    }
    if (!rc) ctx->last_post = rg->kind;                        /* the events now hold this call's times */
    return rc;
}

/* post stage, step 4: its results.  First the small ones, queued behind the block results and ahead of the call's one wait:
 * the counters, the size of the text or of the histogram, the coverage numbers. */
int post_fetch_sizes(cbc_gpu_ctx *ctx, const post_req *rg, const post_sizes &z, uint32_t n_blocks, hipStream_t sc, post_got *g)
{
    if (post_is_depth(rg->kind)) {
        HIPCHK(hipMemcpyAsync(g->dctr, ctx->arena[A_DCTR].p, 16, hipMemcpyDeviceToHost, sc), "D2H depth counters");
        if (rg->kind == POST_CONSENSUS)
            HIPCHK(hipMemcpyAsync(g->cctr, (uint32_t *)ctx->arena[A_DCTR].p + 4, 4 * CBC_CONS_CTRS, hipMemcpyDeviceToHost, sc), "D2H consensus counters");
        if (rg->kind == POST_HIST)
            HIPCHK(hipMemcpyAsync(&g->h_count, (uint64_t *)((cbc_block_result *)ctx->arena[A_HTILE].p + z.n_btiles) + z.n_btiles, 8, hipMemcpyDeviceToHost, sc), "D2H histogram size");
        else if (!post_is_cov(rg->kind))
            HIPCHK(hipMemcpyAsync(&g->total, (uint64_t *)ctx->arena[A_OFF].p + z.n_ttiles, 8, hipMemcpyDeviceToHost, sc), "D2H text size");
        else {                                                 /* the numbers, not the track: 12 bytes per query */
            HIPCHK(hipMemcpyAsync(rg->cov.sum, ctx->arena[A_CVOUT].p, (uint64_t)rg->cov.n_q * 8, hipMemcpyDeviceToHost, sc), "D2H coverage sums");
            HIPCHK(hipMemcpyAsync(rg->cov.covered, (uint64_t *)ctx->arena[A_CVOUT].p + rg->cov.n_q, (uint64_t)rg->cov.n_q * 4, hipMemcpyDeviceToHost, sc), "D2H coverage counts");
            if (post_is_covx(rg->kind) && rg->cov.n_thr)      /* + 4 bytes per threshold and query, + 4 for the read count */
                HIPCHK(hipMemcpyAsync(rg->cov.thr_covered, ctx->arena[A_XOUT].p, (uint64_t)rg->cov.n_q * rg->cov.n_thr * 4, hipMemcpyDeviceToHost, sc), "D2H threshold counts");
            if (post_is_covx(rg->kind) && rg->cov.reads)
                HIPCHK(hipMemcpyAsync(rg->cov.reads, (uint32_t *)ctx->arena[A_XOUT].p + (uint64_t)rg->cov.n_q * rg->cov.n_thr, (uint64_t)rg->cov.n_q * 4, hipMemcpyDeviceToHost, sc), "D2H read counts");
            if (rg->kind == POST_COVQ)                         /* + 4 bytes per quantile and query, behind the read counts' place */
                HIPCHK(hipMemcpyAsync(rg->cov.quant, (uint32_t *)ctx->arena[A_XOUT].p + (uint64_t)rg->cov.n_q * (rg->cov.n_thr + 1ull), (uint64_t)rg->cov.n_q * rg->cov.n_quant * 4, hipMemcpyDeviceToHost, sc), "D2H depth quantiles");
        }
        return CBC_OK;
    }
    if (post_is_stats(rg->kind)) {                             /* the tables are the output: about 270 KB, no second wait */
        g->stats = (uint32_t *)malloc((size_t)(CBC_STATS_WORDS + CBC_SALN_WORDS) * 4);
        if (!g->stats) return CBC_E_NOMEM;
        HIPCHK(hipMemcpyAsync(g->stats, ctx->arena[A_STATS].p, (uint64_t)CBC_STATS_WORDS * 4, hipMemcpyDeviceToHost, sc), "D2H statistics tables");
        if (post_is_stats_aln(rg->kind))
            HIPCHK(hipMemcpyAsync(g->stats + CBC_STATS_WORDS, ctx->arena[A_SALN].p, (uint64_t)CBC_SALN_WORDS * 4, hipMemcpyDeviceToHost, sc), "D2H alignment tables");
        return CBC_OK;
    }
    g->cnt = (cbc_block_result *)malloc((size_t)n_blocks * sizeof(cbc_block_result));
    if (!g->cnt) return CBC_E_NOMEM;
    HIPCHK(hipMemcpyAsync(g->cnt, ctx->arena[A_RCNT].p, (uint64_t)n_blocks * sizeof(cbc_block_result), hipMemcpyDeviceToHost, sc), "D2H region counts");
    HIPCHK(hipMemcpyAsync(&g->total, (uint64_t *)ctx->arena[A_OFF].p + n_blocks, 8, hipMemcpyDeviceToHost, sc), "D2H text size");
    return CBC_OK;
}

/* ... then, once those are on the host, the output itself in one copy of exactly its size: the text, or the histogram's
 * pairs (none when a block failed).  A second wait only when there is something to fetch. */
int post_fetch_output(cbc_gpu_ctx *ctx, const post_req *rg, const post_sizes &z, uint32_t n_blocks, const cbc_block_result *res,
                      hipStream_t sc, const post_got *g, uint64_t *d2h_bytes)
{
    const bool depth = post_is_depth(rg->kind);
    uint64_t kept = 0;
    if (post_is_stats(rg->kind)) {                             /* all zero when a block failed */
        for (uint32_t b = 0; b < n_blocks; b++) if (res[b].status != CBC_ST_OK) return CBC_OK;
        cbc_stats_finish(g->stats, rg->stats);
        *d2h_bytes = (uint64_t)CBC_STATS_WORDS * 4;
        if (post_is_stats_aln(rg->kind)) {
            cbc_stats_aln_finish(g->stats + CBC_STATS_WORDS, rg->stats_aln);
            *d2h_bytes += (uint64_t)CBC_SALN_WORDS * 4;
        }
        return CBC_OK;
    }
    if (depth) { kept = g->dctr[0]; *rg->n_runs = g->dctr[1]; }
    else for (uint32_t b = 0; b < n_blocks; b++) kept += g->cnt[b].n_symbols;
    if (rg->kind == POST_CONSENSUS) {                          /* g->total = E, the emitted bytes: the record is the header, they, their newlines */
        cbc_consensus_counts *c = rg->cons_counts;
        const uint64_t e = g->total, bytes = rg->cons_hdr + e + (e + rg->cons.line_width - 1u) / rg->cons.line_width;
        c->emitted = e; c->ref = g->cctr[CBC_CONS_REF]; c->alt = g->cctr[CBC_CONS_ALT]; c->del = g->cctr[CBC_CONS_DEL];
        c->ambiguous = g->cctr[CBC_CONS_AMB]; c->low_depth = g->cctr[CBC_CONS_LOW]; c->no_call = g->cctr[CBC_CONS_NONE];
        c->ins_skipped = g->cctr[CBC_CONS_INS];
        *rg->text_bytes = bytes; *rg->n_selected = kept;
        if (bytes > rg->text_cap) return set_err(ctx, CBC_E_ARG, "text_cap too small for the consensus record", hipSuccess);
        HIPCHK(hipMemcpyAsync(rg->text, ctx->arena[A_TEXT].p, bytes, hipMemcpyDeviceToHost, sc), "D2H consensus record");
        HIPCHK(hipStreamSynchronize(sc), "D2H consensus record");
        *d2h_bytes = bytes;
        return CBC_OK;
    }
    *rg->text_bytes = g->total; *rg->n_selected = kept;
    if (g->total > rg->text_cap)
        return set_err(ctx, CBC_E_ARG, rg->kind == POST_PILEUP ? "text_cap too small for the pileup text" : depth ? "text_cap too small for the depth text" : post_is_sam(rg->kind) ? "text_cap too small for the SAM text" : "text_cap too small for the region's text", hipSuccess);
    if (g->total) {
        HIPCHK(hipMemcpyAsync(rg->text, ctx->arena[A_TEXT].p, g->total, hipMemcpyDeviceToHost, sc), "D2H region text");
        HIPCHK(hipStreamSynchronize(sc), "D2H region text");
    }
    *d2h_bytes = g->total;
    if (rg->kind != POST_HIST) return CBC_OK;
    for (uint32_t b = 0; b < n_blocks; b++) if (res[b].status != CBC_ST_OK) return CBC_OK;
    const hist_req *hist = &rg->hist;
    const uint64_t h_count = g->h_count;
    *hist->n_bins = h_count > 0xffffffffull ? 0xffffffffu : (uint32_t)h_count;
    if (h_count > z.h_out_cap || h_count > hist->bin_cap) return set_err(ctx, CBC_E_ARG, "bin_cap too small for the histogram's non-zero bins", hipSuccess);
    if (h_count) {
        HIPCHK(hipMemcpyAsync(hist->bin_depth, ctx->arena[A_HOUT].p, h_count * 4, hipMemcpyDeviceToHost, sc), "D2H histogram depths");
        HIPCHK(hipMemcpyAsync(hist->bin_bases, (uint32_t *)ctx->arena[A_HOUT].p + z.h_out_cap, h_count * 4, hipMemcpyDeviceToHost, sc), "D2H histogram bases");
        HIPCHK(hipStreamSynchronize(sc), "D2H histogram");
    }
    *d2h_bytes = h_count * 8;
    return CBC_OK;
}
