/*
 * cbc_gpu.hip -- libcbc_gpu.so: the codec kernels, the context, the host-buffer pipelines and the entry points of the C ABI of
 * include/cbc_gpu.h (gfx950 only).  The kernels and launches of the post-decode stage and the tokeniser are translation units of
 * their own (cbc_gpu_internal.h says which file holds what); what bench.py measures is built from and launched by this file.
 *
 * Launch shape: one workgroup per block = per arithmetic stream (encode: 128 threads = model wavefront +
 * coder wavefront; decode: 64 threads); the model tables live in dynamic LDS (cbc_gpu_lds_bytes()), so
 * workgroups per CU = 160 KiB / that.  The grid is the number of blocks (thousands) >> 256 CUs.
 */
#include <new>
#include <time.h>
#include <dlfcn.h>
#include <rccl/rccl.h>              /* types and prototypes only: librccl.so (573 MB) is loaded when a group is created */

#include "cbc_gpu_internal.h"
#include "cbc_wave_gpu.h"
#include "cbc_encode_body.h"
#include "cbc_decode_body.h"
#include "cbc_stream_body.h"
#include "cbc_long_body.h"
#include "cbc_covx_body.h"           /* CBC_COVX_MAX_THR and */
#include "cbc_stats_aln_body.h"      /* CBC_SALN_MAX_UNITS: limits the decode entry points check */

/* the block kernels take their lane writes under one mask from the GPU policy; without this the body would fall back to
 * the plain form silently (same bytes, slower) if a helper were renamed or overloaded */
static_assert(CbcHasLaneN<WaveGPU>::value, "WaveGPU must supply set_lane2_uv and set_lane3");

/* ------------------------------------------------------------------------------------------------
 * kernels
 * ---------------------------------------------------------------------------------------------- */
extern __shared__ uint32_t cbc_lds[];

/* One workgroup = one block = one arithmetic stream, coded by TWO wavefronts: wavefront 0 (model)
 * runs the match test and the edit models and sends END-terminated segments of the symbol stream
 * through an LDS ring; wavefront 1 (coder) owns the per-record models, computes their symbols one
 * lane per record and runs the range coder (cbc_encode_body.h, CbcEnc::publish / pull).
 * Workgroups are dealt round-robin to the 8 XCDs; blocks of one contig are neighbours in the
 * batch and share nothing but read-only reference lines, so the identity map is kept and the
 * per-XCD L2s each see a strided slice of the record stream. */
template <bool HOT>
static __device__ __forceinline__ void cbc_encode_block(const cbc_enc_args &A)
{
    uint32_t blk = blockIdx.x;
    if (blk >= A.n_blocks) return;
    const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (wid == 0u) cbc_encode_stream<WaveGPU, CBC_ROLE_MODEL, HOT>(A, blk, cbc_lds);
    else cbc_encode_stream<WaveGPU, CBC_ROLE_CODER, HOT>(A, blk, cbc_lds);
}

/* Two register budgets of the same code.  Up to ten blocks per CU (cfg2: 9.5) everything is resident at
 * 5 wavefronts per SIMD and the kernel is latency-bound: the 84-register build is the faster one.  With
 * more blocks than that (cfg3-sized input) the CU is throughput-bound and a sixth wavefront per SIMD (80
 * registers, one spilled) gains 6 %; it costs 5 % at cfg2.  One wave fewer than 5 costs 25-30 %.
 * The five-wave build keeps the hot var context in four more registers (CbcEnc::hot_code); the six-wave build has none
 * to spare (with the table: 28 bytes of scratch per lane) and keeps every context in the buckets and lists
 * (-DCBC_HOT_CTX_W6=1 to look again). */
#ifndef CBC_HOT_CTX_W6
#define CBC_HOT_CTX_W6 0
#endif
__global__ void __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(5)))
cbc_encode_blocks_kernel(cbc_enc_args A) { cbc_encode_block<CBC_HOT_CTX != 0>(A); }

__global__ void __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(6)))
cbc_encode_blocks_kernel_w6(cbc_enc_args A) { cbc_encode_block<CBC_HOT_CTX_W6 != 0>(A); }

__global__ void __launch_bounds__(64)
cbc_decode_blocks_kernel(cbc_dec_args A)
{
    uint32_t blk = blockIdx.x;
    if (blk >= A.n_blocks) return;
    cbc_decode_stream<WaveGPU>(A, blk, cbc_lds);
}

/* region decode (cbc_gpu_decode_region): the same decoder with each read's span in cbc_read_rec.tok_off, checked against
 * smax; then the filter (one wavefront per block) and the text assembly (CBC_REGION_WAVES wavefronts per block) */
__global__ void __launch_bounds__(64)
cbc_decode_blocks_span_kernel(cbc_dec_args A, uint32_t smax)
{
    uint32_t blk = blockIdx.x;
    if (blk >= A.n_blocks) return;
    cbc_decode_stream<WaveGPU, true>(A, blk, cbc_lds, smax);
}

/* per-position allele counts (cbc_gpu_decode_pileup, cbc_pileup_body.h): the span decoder that also leaves the alignment of
 * the reads with indels (cbc_dec_edits); then, behind cbc_depth_mark_kernel, CBC_PILEUP_WAVES wavefronts per block add the
 * mismatches, deleted bases and insertion events, and one wavefront per tile of positions counts and writes the lines */
__global__ void __launch_bounds__(64)
cbc_decode_blocks_edits_kernel(cbc_dec_args A, uint32_t smax, cbc_dec_edits E)
{
    uint32_t blk = blockIdx.x;
    if (blk >= A.n_blocks) return;
    cbc_decode_stream<WaveGPU, true, true>(A, blk, cbc_lds, smax, &E);
}

/* Whole-file stream / general-form fallback (cbc_stream_body.h): one wavefront per stream.  Workgroup w codes streams
 * w, w + gridDim, ... with var table w of the pool, which it re-zeroes between streams. */
__global__ void __launch_bounds__(64)
cbc_encode_whole_kernel(cbc_stream_args A)
{
    const uint32_t n_streams = A.per_segment ? A.n_segs : 1u;
    for (uint32_t s = blockIdx.x; s < n_streams; s += gridDim.x) {
        if (s != blockIdx.x) {
            uint4 *t = (uint4 *)(A.vtab + (uint64_t)blockIdx.x * CBC_VTAB_WORDS);
            for (uint64_t i = threadIdx.x; i < CBC_VTAB_WORDS / 4; i += 64) t[i] = make_uint4(0, 0, 0, 0);
            __threadfence();
        }
        cbc_encode_whole<WaveGPU>(A, s, blockIdx.x, cbc_lds);
    }
}

__global__ void __launch_bounds__(64)
cbc_decode_whole_kernel(cbc_dstream_args A) { cbc_decode_whole<WaveGPU>(A, cbc_lds); }

/* long-read format (cbc_long_body.h): encode = three wavefronts per block (model, coder, walker), decode = one */
#ifndef CBC_LONG_ENC_WAVES
#define CBC_LONG_ENC_WAVES 8           /* wavefronts per SIMD the register budget is cut for (A/B: profiles/r03_ab_kernels.log) */
#endif
__global__ void __launch_bounds__(192) __attribute__((amdgpu_waves_per_eu(CBC_LONG_ENC_WAVES)))
cbc_long_encode_kernel(cbc_long_args A)
{
    if (blockIdx.x >= A.n_blocks) return;
    const uint32_t wid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (wid == 0u) cbc_long_encode<WaveGPU, CBC_ROLE_MODEL>(A, blockIdx.x, cbc_lds);
    else if (wid == 1u) cbc_long_encode<WaveGPU, CBC_ROLE_CODER>(A, blockIdx.x, cbc_lds);
    else cbc_long_encode<WaveGPU, CBC_ROLE_WALKER>(A, blockIdx.x, cbc_lds);
}
__global__ void __launch_bounds__(64)
cbc_long_decode_kernel(cbc_dec_args A) { if (blockIdx.x < A.n_blocks) cbc_long_decode<WaveGPU>(A, blockIdx.x, cbc_lds); }

/* ---- 2-bit transport (include/cbc_gpu.h): expand = one code word per lane -> 16 bases, one 16-byte store per lane ---- */
__global__ void __launch_bounds__(256)
cbc_expand_2bit_kernel(const uint32_t *__restrict__ codes, uint64_t n_words, uint8_t *__restrict__ out, uint64_t n_bases)
{
    const uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (w >= n_words) return;
    const uint32_t c = codes[w];
    uint32_t v[4];
    for (int q = 0; q < 4; q++) {
        uint32_t x = 0;
        for (int k = 0; k < 4; k++) {
            const uint32_t code = (c >> (2 * (4 * q + k))) & 3u;
            x |= (uint32_t)("ACGT"[code]) << (8 * k);
        }
        v[q] = x;
    }
    const uint64_t b0 = w * 16;
    if (b0 + 16 <= n_bases && ((uintptr_t)(out + b0) & 15) == 0) *(uint4 *)(out + b0) = make_uint4(v[0], v[1], v[2], v[3]);
    else for (int k = 0; k < 16 && b0 + k < n_bases; k++) out[b0 + k] = (uint8_t)(v[k >> 2] >> (8 * (k & 3)));
}
/* exception runs: workgroup = run, threads stride over its bytes */
__global__ void __launch_bounds__(256)
cbc_apply_runs_kernel(const cbc_2bit_run_dev *__restrict__ runs, uint64_t n_runs, uint8_t *__restrict__ out, uint64_t n_bases,
                      uint64_t lo, uint64_t hi /* only the bytes of [lo, hi): the chunk that has just been expanded */)
{
    const uint64_t r = blockIdx.x;
    if (r >= n_runs) return;
    const uint64_t s0 = runs[r].start; const uint32_t len = runs[r].length; const uint8_t b = (uint8_t)runs[r].byte;
    if (s0 > n_bases || len > n_bases - s0 || s0 >= hi || s0 + len <= lo) return;
    for (uint32_t i = threadIdx.x; i < len; i += 256) if (s0 + i >= lo && s0 + i < hi) out[s0 + i] = b;
}
/* pack decoded reads: thread = one 16-base word of one read row; bases past the read's length are not looked at */
__global__ void __launch_bounds__(256)
cbc_pack_2bit_kernel(const uint8_t *__restrict__ seq, const cbc_read_rec *__restrict__ recs, uint64_t rec0, uint64_t rec1, uint32_t stride,
                     uint32_t *__restrict__ codes, uint64_t *__restrict__ exc_idx, uint8_t *__restrict__ exc_val,
                     uint64_t exc_cap, unsigned long long *__restrict__ n_exc)
{
    const uint32_t row_words = stride >> 4;
    const uint64_t w = rec0 * row_words + (uint64_t)blockIdx.x * 256 + threadIdx.x;      /* records [rec0, rec1): one chunk of the decode */
    if (w >= rec1 * row_words) return;
    const uint64_t r = w / row_words; const uint32_t k0 = (uint32_t)(w % row_words) * 16u;
    const uint32_t rl = recs[r].rlen;
    const uint4 raw = *(const uint4 *)(seq + r * stride + k0);             /* rows are 16-byte aligned (stride % 16 == 0) */
    const uint32_t v[4] = { raw.x, raw.y, raw.z, raw.w };
    uint32_t c = 0;
    for (uint32_t k = 0; k < 16u; k++) {
        if (k0 + k >= rl) break;
        const uint8_t b = (uint8_t)(v[k >> 2] >> (8 * (k & 3)));
        const uint32_t code = b == 'A' ? 0u : b == 'C' ? 1u : b == 'G' ? 2u : b == 'T' ? 3u : 4u;
        if (code < 4u) c |= code << (2 * k);
        else {
            const unsigned long long at = atomicAdd(n_exc, 1ull);
            if (at < exc_cap) { exc_idx[at] = r * stride + k0 + k; exc_val[at] = b; }
        }
    }
    codes[w] = c;
}

/* exclusive scan of the per-block payload sizes -> offsets[n_blocks+1]; one workgroup */
__global__ void __launch_bounds__(1024)
cbc_scan_sizes_kernel(const cbc_block_result *__restrict__ results, uint64_t *__restrict__ offsets, uint32_t n_blocks)
{
    __shared__ uint64_t part[1024];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (n_blocks + 1023u) / 1024u;
    const uint32_t b0 = t * per, b1 = min(n_blocks, b0 + per);
    uint64_t s = 0;
    for (uint32_t b = b0; b < b1; b++) s += results[b].status == CBC_ST_OK ? results[b].nbytes : 0u;
    part[t] = s;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        uint64_t v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint64_t run = part[t] - s;
    for (uint32_t b = b0; b < b1; b++) { offsets[b] = run; run += results[b].status == CBC_ST_OK ? results[b].nbytes : 0u; }
    if (t == 1023u) offsets[n_blocks] = part[1023];
}

/* gather the per-block payload areas into one compacted buffer, 16 bytes per lane where aligned */
__global__ void __launch_bounds__(256)
cbc_compact_kernel(const uint8_t *__restrict__ scratch, const cbc_block_desc *__restrict__ blocks,
                   const uint64_t *__restrict__ dst_off, uint8_t *__restrict__ dst, uint64_t dst_cap, uint32_t n_blocks)
{
    uint32_t b = blockIdx.x;
    if (b >= n_blocks) return;
    const uint64_t so = blocks[b].out_off, d0 = dst_off[b];
    uint64_t n = dst_off[b + 1] - d0;
    if (d0 + n > dst_cap) return;
    for (uint64_t i = threadIdx.x; i < n; i += blockDim.x) dst[d0 + i] = scratch[so + i];
}

/* 64-bit checksum of a byte range (cbc_gpu_checksum_device): sum of CBC_CHECKSUM_TERM(i, byte) mod 2^64 -- the sum is
 * order-free, so lanes, wavefronts and workgroups add their parts in any order and the value is exact */
__global__ void __launch_bounds__(256)
cbc_checksum_kernel(const uint8_t *__restrict__ p, uint64_t n, unsigned long long *__restrict__ sum)
{
    uint64_t acc = 0;
    const uint64_t n16 = n / 16;                              /* 16 bytes per lane where the base is aligned */
    if (((uintptr_t)p & 15) == 0) {
        for (uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x; w < n16; w += (uint64_t)gridDim.x * 256) {
            const uint4 v = ((const uint4 *)p)[w];
            const uint32_t q[4] = { v.x, v.y, v.z, v.w };
            for (uint32_t k = 0; k < 16u; k++) acc += CBC_CHECKSUM_TERM(w * 16 + k, (uint8_t)(q[k >> 2] >> (8 * (k & 3))));
        }
        for (uint64_t i = n16 * 16 + (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) acc += CBC_CHECKSUM_TERM(i, p[i]);
    } else
        for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) acc += CBC_CHECKSUM_TERM(i, p[i]);
    for (int d = 32; d > 0; d >>= 1) acc += __shfl_down((unsigned long long)acc, d, 64);
    if ((threadIdx.x & 63u) == 0u && acc) atomicAdd(sum, (unsigned long long)acc);
}

/* ------------------------------------------------------------------------------------------------
 * context
 * ---------------------------------------------------------------------------------------------- */
int set_err(cbc_gpu_ctx *c, int code, const char *what, hipError_t e)
{
    if (c) snprintf(c->err, sizeof c->err, "%s: %s", what, e == hipSuccess ? "" : hipGetErrorString(e));
    return code;
}

/* at least `bytes` in arena k; growing frees the old buffer (hipFree waits for the device) */
int arena_need(cbc_gpu_ctx *ctx, int k, uint64_t bytes, const char *what)
{
    cbc_arena *a = &ctx->arena[k];
    if (a->p && a->cap >= bytes) return CBC_OK;
    if (a->p) { (void)hipFree(a->p); a->p = NULL; a->cap = 0; }
    const uint64_t want = (bytes + (bytes >> 3) + (2ull << 20)) & ~((2ull << 20) - 1);      /* 1/8 headroom, 2 MiB granules */
    HIPCHK(hipMalloc(&a->p, want), what);
    a->cap = want;
    return CBC_OK;
}

/* the first block whose status is not CBC_ST_OK becomes the call's error: "block <b> <verb> with status ..." */
int blocks_failed(cbc_gpu_ctx *ctx, const cbc_block_result *res, uint32_t n_blocks, const char *verb)
{
    for (uint32_t b = 0; b < n_blocks; b++)
        if (res[b].status != CBC_ST_OK) {
            if (res[b].status == CBC_ST_EDITS)
                snprintf(ctx->err, sizeof ctx->err, "block %u %s with status %u at record %u: its reads with indels hold more deleted and inserted "
                         "bases than its edit arena (raise --max-edits-per-read / edits_per_read)", b, verb, res[b].status, res[b].fail_read);
            else
                snprintf(ctx->err, sizeof ctx->err, "block %u %s with status %u at record %u", b, verb, res[b].status, res[b].fail_read);
            return CBC_E_BLOCK;
        }
    return CBC_OK;
}
static double wall_now(void) { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; }

API int cbc_gpu_abi_version(void) { return CBC_ABI_VERSION; }

API int cbc_gpu_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

API int cbc_gpu_init(int device_ordinal, cbc_gpu_ctx **out)
{
    if (!out) return CBC_E_ARG;
    *out = NULL;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device_ordinal < 0 || device_ordinal >= n) return CBC_E_NODEV;
    cbc_gpu_ctx *ctx = new (std::nothrow) cbc_gpu_ctx();
    if (!ctx) return CBC_E_NOMEM;
    memset(ctx, 0, sizeof *ctx);
    ctx->device = device_ordinal;
    if (hipSetDevice(device_ordinal) != hipSuccess ||
        hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&ctx->s_copy, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess) {
        delete ctx; return CBC_E_NODEV;
    }
    for (int k = 0; k < CBC_N_KSTREAMS; k++)
        if (hipStreamCreateWithFlags(&ctx->s_k[k], hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&ctx->ev_done[k], hipEventDisableTiming) != hipSuccess) { delete ctx; return CBC_E_NODEV; }
    for (int k = 0; k < CBC_MAX_CHUNKS; k++)
        if (hipEventCreateWithFlags(&ctx->ev_chunk[k], hipEventDisableTiming) != hipSuccess) { delete ctx; return CBC_E_NODEV; }
    for (int k = 0; k < 5; k++)
        if (hipEventCreate(&ctx->ev_rg[k]) != hipSuccess) { delete ctx; return CBC_E_NODEV; }
    for (int k = 0; k < 4; k++)
        if (hipEventCreate(&ctx->ev_cov[k]) != hipSuccess) { delete ctx; return CBC_E_NODEV; }
    for (int k = 0; k < 2; k++)
        if (hipEventCreate(&ctx->ev_hist[k]) != hipSuccess) { delete ctx; return CBC_E_NODEV; }
    for (int k = 0; k < 5; k++)
        if (hipEventCreate(&ctx->ev_covx[k]) != hipSuccess) { delete ctx; return CBC_E_NODEV; }
    if (hipEventCreate(&ctx->ev_quant) != hipSuccess) { delete ctx; return CBC_E_NODEV; }
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_ordinal) != hipSuccess || cus <= 0) cus = 256;
        ctx->n_cus = cus;
    }
    /* the kernel's dynamic LDS can exceed the 64 KiB default */
    (void)hipFuncSetAttribute((const void *)cbc_encode_blocks_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void *)cbc_encode_blocks_kernel_w6, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void *)cbc_decode_blocks_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void *)cbc_decode_blocks_span_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void *)cbc_decode_blocks_edits_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void *)cbc_encode_whole_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void *)cbc_long_encode_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void *)cbc_long_decode_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void *)cbc_decode_whole_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    *out = ctx;
    return CBC_OK;
}

API int cbc_gpu_shutdown(cbc_gpu_ctx *ctx)
{
    if (!ctx) return CBC_E_ARG;
    (void)hipSetDevice(ctx->device);
    (void)hipDeviceSynchronize();
    if (ctx->d_ref) (void)hipFree(ctx->d_ref);
    for (int k = 0; k < A_COUNT; k++) if (ctx->arena[k].p) (void)hipFree(ctx->arena[k].p);
    (void)hipEventDestroy(ctx->ev0); (void)hipEventDestroy(ctx->ev1);
    for (int k = 0; k < CBC_MAX_CHUNKS; k++) (void)hipEventDestroy(ctx->ev_chunk[k]);
    for (int k = 0; k < 5; k++) (void)hipEventDestroy(ctx->ev_rg[k]);
    for (int k = 0; k < 4; k++) (void)hipEventDestroy(ctx->ev_cov[k]);
    for (int k = 0; k < 2; k++) (void)hipEventDestroy(ctx->ev_hist[k]);
    for (int k = 0; k < 5; k++) (void)hipEventDestroy(ctx->ev_covx[k]);
    (void)hipEventDestroy(ctx->ev_quant);
    for (int k = 0; k < CBC_N_KSTREAMS; k++) { (void)hipEventDestroy(ctx->ev_done[k]); (void)hipStreamDestroy(ctx->s_k[k]); }
    (void)hipStreamDestroy(ctx->s_copy);
    (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return CBC_OK;
}

API const char *cbc_gpu_last_error(cbc_gpu_ctx *ctx) { return ctx ? ctx->err : "no context"; }

API int cbc_gpu_upload_reference(cbc_gpu_ctx *ctx, const uint8_t *bases, uint64_t nbytes)
{
    if (!ctx || !bases || nbytes == 0) return CBC_E_ARG;
    HIPCHK(hipSetDevice(ctx->device), "hipSetDevice");
    if (ctx->d_ref) { (void)hipFree(ctx->d_ref); ctx->d_ref = NULL; ctx->ref_bytes = 0; }
    HIPCHK(hipMalloc((void **)&ctx->d_ref, nbytes), "hipMalloc(reference)");
    HIPCHK(hipMemcpy(ctx->d_ref, bases, nbytes, hipMemcpyHostToDevice), "hipMemcpy(reference)");
    ctx->ref_bytes = nbytes;
    return CBC_OK;
}

/* the reference as several host pieces laid end to end on the device (a device that owns some contigs uploads just those) */
API int cbc_gpu_upload_reference_parts(cbc_gpu_ctx *ctx, const uint8_t *const *parts, const uint64_t *bytes, uint32_t n_parts)
{
    if (!ctx || !parts || !bytes || n_parts == 0) return CBC_E_ARG;
    uint64_t total = 0;
    for (uint32_t k = 0; k < n_parts; k++) { if (!parts[k] && bytes[k]) return CBC_E_ARG; total += bytes[k]; }
    if (total == 0) return CBC_E_ARG;
    HIPCHK(hipSetDevice(ctx->device), "hipSetDevice");
    if (ctx->d_ref) { (void)hipFree(ctx->d_ref); ctx->d_ref = NULL; ctx->ref_bytes = 0; }
    HIPCHK(hipMalloc((void **)&ctx->d_ref, total + 16), "hipMalloc(reference)");
    uint64_t at = 0;
    for (uint32_t k = 0; k < n_parts; k++) {
        if (bytes[k]) HIPCHK(hipMemcpyAsync(ctx->d_ref + at, parts[k], bytes[k], hipMemcpyHostToDevice, ctx->stream), "hipMemcpy(reference part)");
        at += bytes[k];
    }
    HIPCHK(hipMemsetAsync(ctx->d_ref + total, 0, 16, ctx->stream), "memset reference pad");
    HIPCHK(hipStreamSynchronize(ctx->stream), "reference upload");
    ctx->ref_bytes = total;
    return CBC_OK;
}

API uint64_t cbc_gpu_plan_output(cbc_block_desc *blocks, uint32_t n_blocks, const cbc_read_rec *recs, const uint32_t *tok)
{
    return cbc_plan_output(blocks, n_blocks, recs, tok);
}
API uint64_t cbc_gpu_plan_output_caps(cbc_block_desc *blocks, uint32_t n_blocks, const cbc_lds_caps *caps)
{
    return (blocks && caps) ? cbc_plan_output_caps(blocks, n_blocks, caps) : 0;
}
API uint32_t cbc_gpu_lds_bytes(const cbc_lds_caps *caps) { return caps ? cbc_plan_lds_bytes(caps) : 0; }

/* grow the context's arenas for a batch of this shape before the batch exists (a CLI does it while the host still parses) */
API int cbc_gpu_reserve_encode(cbc_gpu_ctx *ctx, uint64_t n_recs, uint64_t seq_bytes, uint64_t n_tok, uint32_t n_blocks, uint64_t scratch_bytes)
{
    if (!ctx) return CBC_E_ARG;
    HIPCHK(hipSetDevice(ctx->device), "hipSetDevice");
    int rc;
    if ((rc = arena_need(ctx, A_RECS, n_recs * sizeof(cbc_read_rec) + 16, "hipMalloc recs"))) return rc;
    if ((rc = arena_need(ctx, A_SEQ, seq_bytes + 32, "hipMalloc seq"))) return rc;
    if ((rc = arena_need(ctx, A_TOK, (n_tok ? n_tok : 1) * 4 + 16, "hipMalloc tok"))) return rc;
    if ((rc = arena_need(ctx, A_BLOCKS, (uint64_t)(n_blocks ? n_blocks : 1) * sizeof(cbc_block_desc), "hipMalloc blocks"))) return rc;
    if ((rc = arena_need(ctx, A_RES, (uint64_t)(n_blocks ? n_blocks : 1) * sizeof(cbc_block_result), "hipMalloc results"))) return rc;
    if ((rc = arena_need(ctx, A_OFF, ((uint64_t)n_blocks + 1) * 8, "hipMalloc offsets"))) return rc;
    if ((rc = arena_need(ctx, A_OUT, scratch_bytes ? scratch_bytes : 1, "hipMalloc out scratch"))) return rc;
    return CBC_OK;
}

/* resident_blocks: how many blocks compete for the chip while this launch runs (the chunked host-buffer path makes several
 * launches that run side by side): it, not the launch's own grid, decides the register budget of the build */
static int encode_blocks_launch(cbc_gpu_ctx *ctx, const cbc_device_batch *b, void *hip_stream, uint64_t resident_blocks)
{
    if (!ctx || !b) return CBC_E_ARG;
    if (b->n_blocks == 0) return CBC_OK;
    if (!b->d_recs || !b->d_seq || !b->d_tok || !b->d_names || !b->d_blocks || !b->d_ref || !b->d_out || !b->d_results)
        return set_err(ctx, CBC_E_ARG, "null device pointer in cbc_device_batch", hipSuccess);
    if (b->caps.cap_pos < 2 || b->caps.cap_pos > 8192 || b->caps.cap_var < 1 || b->caps.cap_var > 32768)
        return set_err(ctx, CBC_E_ARG, "lds caps out of range", hipSuccess);
    const uint32_t lds = cbc_plan_lds_bytes(&b->caps);
    if (lds > 160u * 1024u) return set_err(ctx, CBC_E_ARG, "lds caps need more than 160 KiB", hipSuccess);
    HIPCHK(hipSetDevice(ctx->device), "hipSetDevice");
    hipStream_t s = hip_stream == CBC_CTX_STREAM ? ctx->stream : (hipStream_t)hip_stream;
    cbc_enc_args A;
    A.recs = b->d_recs; A.seq = b->d_seq; A.tok = b->d_tok; A.names = b->d_names; A.blocks = b->d_blocks;
    A.ref = b->d_ref; A.out = b->d_out; A.results = b->d_results;
    A.ref_bytes = b->ref_bytes; A.out_bytes = b->out_bytes; A.seq_bytes = b->seq_bytes; A.n_tok = b->n_tok;
    A.n_recs = b->n_recs; A.n_blocks = b->n_blocks; A.cap_pos = b->caps.cap_pos; A.cap_var = b->caps.cap_var;
    A.names_bytes = 0x7fffffffu;   /* names are NUL-terminated; bounded by CBC_CAP_NAME in the kernel */
    HIPCHK(hipEventRecord(ctx->ev0, s), "hipEventRecord");
    if (resident_blocks > 10ull * (uint64_t)ctx->n_cus)           /* more blocks than are resident at 5 waves per SIMD */
        { hipLaunchKernelGGL(cbc_encode_blocks_kernel_w6, dim3(b->n_blocks), dim3(128), lds, s, A); ctx->last_variant = 6; }
    else
        { hipLaunchKernelGGL(cbc_encode_blocks_kernel, dim3(b->n_blocks), dim3(128), lds, s, A); ctx->last_variant = 5; }
    HIPCHK(hipGetLastError(), "launch cbc_encode_blocks_kernel");
    HIPCHK(hipEventRecord(ctx->ev1, s), "hipEventRecord");
    ctx->have_timing = 1;
    return CBC_OK;
}
API int cbc_gpu_encode_blocks_device(cbc_gpu_ctx *ctx, const cbc_device_batch *b, void *hip_stream)
{
    return encode_blocks_launch(ctx, b, hip_stream, b ? b->n_blocks : 0);
}

API int cbc_gpu_last_kernel_ms(cbc_gpu_ctx *ctx, float *ms)
{
    if (!ctx || !ms || !ctx->have_timing) return CBC_E_ARG;
    HIPCHK(hipEventSynchronize(ctx->ev1), "hipEventSynchronize");
    HIPCHK(hipEventElapsedTime(ms, ctx->ev0, ctx->ev1), "hipEventElapsedTime");
    return CBC_OK;
}

API int cbc_gpu_last_kernel_variant(cbc_gpu_ctx *ctx) { return ctx ? ctx->last_variant : 0; }

API int cbc_gpu_synchronize(cbc_gpu_ctx *ctx)
{
    if (!ctx) return CBC_E_ARG;
    HIPCHK(hipSetDevice(ctx->device), "hipSetDevice");
    HIPCHK(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize");
    return CBC_OK;
}

API int cbc_gpu_compact_device(cbc_gpu_ctx *ctx, const uint8_t *d_scratch, const cbc_block_desc *d_blocks,
                               const cbc_block_result *d_results, uint32_t n_blocks, uint64_t *d_offsets,
                               uint8_t *d_packed, uint64_t packed_cap, void *hip_stream)
{
    if (!ctx || !d_scratch || !d_blocks || !d_results || !d_offsets || !d_packed) return CBC_E_ARG;
    if (n_blocks == 0) return CBC_OK;
    HIPCHK(hipSetDevice(ctx->device), "hipSetDevice");
    hipStream_t s = hip_stream == CBC_CTX_STREAM ? ctx->stream : (hipStream_t)hip_stream;
    hipLaunchKernelGGL(cbc_scan_sizes_kernel, dim3(1), dim3(1024), 0, s, d_results, d_offsets, n_blocks);
    HIPCHK(hipGetLastError(), "launch cbc_scan_sizes_kernel");
    hipLaunchKernelGGL(cbc_compact_kernel, dim3(n_blocks), dim3(256), 0, s, d_scratch, d_blocks,
                       (const uint64_t *)d_offsets, d_packed, packed_cap, n_blocks);
    HIPCHK(hipGetLastError(), "launch cbc_compact_kernel");
    return CBC_OK;
}

API int cbc_gpu_checksum_device(cbc_gpu_ctx *ctx, const uint8_t *d_bytes, uint64_t n, uint64_t *d_sum, void *hip_stream)
{
    if (!ctx || !d_sum || (n && !d_bytes)) return CBC_E_ARG;
    HIPCHK(hipSetDevice(ctx->device), "hipSetDevice");
    hipStream_t s = hip_stream == CBC_CTX_STREAM ? ctx->stream : (hipStream_t)hip_stream;
    HIPCHK(hipMemsetAsync(d_sum, 0, 8, s), "memset checksum");
    if (n == 0) return CBC_OK;
    const uint64_t want = (n / 16 + 255) / 256 + 1;
    const unsigned grid = (unsigned)(want < 4096 ? want : 4096);
    hipLaunchKernelGGL(cbc_checksum_kernel, dim3(grid), dim3(256), 0, s, d_bytes, n, (unsigned long long *)d_sum);
    HIPCHK(hipGetLastError(), "launch cbc_checksum_kernel");
    return CBC_OK;
}

static int expand_2bit(cbc_gpu_ctx *ctx, const uint32_t *codes, uint64_t n_bases, const cbc_2bit_run_dev *runs, uint64_t n_runs,
                       uint8_t *d_out, void **d_tmp_codes, void **d_tmp_runs)
{
    const uint64_t n_words = (n_bases + 15) / 16;
    if (n_words == 0) return CBC_OK;
    if (n_runs > 0x7fffffffull || n_words > 0x7fffffffull * 256ull) return set_err(ctx, CBC_E_ARG, "2-bit transport: too many words or runs", hipSuccess);
    HIPCHK(hipMalloc(d_tmp_codes, n_words * 4), "hipMalloc 2-bit codes");
    HIPCHK(hipMemcpyAsync(*d_tmp_codes, codes, n_words * 4, hipMemcpyHostToDevice, ctx->stream), "H2D 2-bit codes");
    hipLaunchKernelGGL(cbc_expand_2bit_kernel, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, ctx->stream,
                       (const uint32_t *)*d_tmp_codes, n_words, d_out, n_bases);
    HIPCHK(hipGetLastError(), "launch cbc_expand_2bit_kernel");
    if (n_runs) {
        HIPCHK(hipMalloc(d_tmp_runs, n_runs * sizeof(cbc_2bit_run_dev)), "hipMalloc 2-bit runs");
        HIPCHK(hipMemcpyAsync(*d_tmp_runs, runs, n_runs * sizeof(cbc_2bit_run_dev), hipMemcpyHostToDevice, ctx->stream), "H2D 2-bit runs");
        hipLaunchKernelGGL(cbc_apply_runs_kernel, dim3((unsigned)n_runs), dim3(256), 0, ctx->stream,
                           (const cbc_2bit_run_dev *)*d_tmp_runs, n_runs, d_out, n_bases, (uint64_t)0, n_bases);
        HIPCHK(hipGetLastError(), "launch cbc_apply_runs_kernel");
    }
    return CBC_OK;
}

API int cbc_gpu_upload_reference_2bit(cbc_gpu_ctx *ctx, const uint32_t *codes, uint64_t n_bases, const cbc_2bit_run_dev *runs, uint64_t n_runs)
{
    if (!ctx || !codes || n_bases == 0 || (n_runs && !runs)) return CBC_E_ARG;
    HIPCHK(hipSetDevice(ctx->device), "hipSetDevice");
    if (ctx->d_ref) { (void)hipFree(ctx->d_ref); ctx->d_ref = NULL; ctx->ref_bytes = 0; }
    HIPCHK(hipMalloc((void **)&ctx->d_ref, n_bases + 16), "hipMalloc(reference)");
    void *d_codes = NULL, *d_runs = NULL;
    int rc = expand_2bit(ctx, codes, n_bases, runs, n_runs, ctx->d_ref, &d_codes, &d_runs);
    if (!rc && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = set_err(ctx, CBC_E_NODEV, "2-bit reference expansion", hipGetLastError());
    if (d_codes) (void)hipFree(d_codes); if (d_runs) (void)hipFree(d_runs);
    if (rc) { (void)hipFree(ctx->d_ref); ctx->d_ref = NULL; return rc; }
    ctx->ref_bytes = n_bases;
    return CBC_OK;
}

/* The host-buffer encode path (timed region ii), as a pipeline -- every host-buffer encode entry point
 * (bytes, 2-bit, tokenised, long reads) is this function with the payload areas its caller planned (`scratch` bytes):
 *   - device arrays are the context's grow-only arenas (no hipMalloc / hipFree per call once they have their size);
 *   - the batch is cut into up to CBC_MAX_CHUNKS runs of consecutive blocks (cbc_plan_chunks); chunk c's records, bases
 *     (bytes or 2-bit codes) and tokens go H2D on the copy stream, followed there by its 2-bit expansion, and an event
 *     later its encode launch runs on kernel stream c -- so chunk c + 1 crosses PCIe while chunk c is being coded, and
 *     launches of neighbouring chunks share the chip (a block is one serial chain: a launch of few blocks cannot fill it
 *     alone); the copy stream's order puts every expansion, the code word two chunks share included, before the encodes
 *     that read it;
 *   - one size scan + compaction over all blocks and one D2H of the compacted bitstreams (2 bytes per read) end it.
 * Long reads (long_reads) take the long-read launcher and stay one chunk: their launches share the context's table
 * scratch (A_LSCR), so two of them on two streams would overwrite each other's tables.
 * Source buffers that are page-locked (cbc_gpu_host_register, or the caller's own hipHostMalloc) are read by DMA at the
 * link rate; pageable ones go through the runtime's staging, which blocks this thread but not the launches already made. */
static int encode_blocks_impl(cbc_gpu_ctx *ctx, const cbc_host_batch *hb, uint64_t scratch, const uint32_t *seq_codes,
                              const cbc_2bit_run_dev *seq_runs, uint64_t n_seq_runs, uint8_t *out, uint64_t out_cap,
                              uint64_t *out_offsets, cbc_block_result *results, const uint8_t *d_seq_ext = NULL,
                              const uint32_t *d_tok_ext = NULL, bool long_reads = false)
{
    if (!ctx || !hb || !out_offsets) return CBC_E_ARG;     /* out == NULL: the bitstreams stay on the device (the context's stash) */
    if (!ctx->d_ref) return set_err(ctx, CBC_E_ARG, "cbc_gpu_upload_reference has not been called", hipSuccess);
    const uint32_t nb = hb->n_blocks;
    out_offsets[0] = 0;
    if (nb == 0) return CBC_OK;
    HIPCHK(hipSetDevice(ctx->device), "hipSetDevice");
    const double T0 = wall_now();
    cbc_e2e_times tm; memset(&tm, 0, sizeof tm);
    cbc_block_result *res = NULL;
    uint8_t *d_compact = NULL;
    int rc = CBC_OK;
    uint64_t total = 0;
    const uint64_t ntok = hb->n_tok ? hb->n_tok : 1;
    const bool two_bit = seq_codes && !d_seq_ext;
    NEED(A_RECS, hb->n_recs * sizeof(cbc_read_rec) + 16, "hipMalloc recs");
    if (!d_seq_ext) NEED(A_SEQ, hb->seq_bytes + 32, "hipMalloc seq");
    if (!d_tok_ext) NEED(A_TOK, ntok * 4 + 16, "hipMalloc tok");
    NEED(A_NAMES, hb->names_bytes + 16, "hipMalloc names");
    NEED(A_BLOCKS, (uint64_t)nb * sizeof(cbc_block_desc), "hipMalloc blocks");
    NEED(A_OUT, scratch, "hipMalloc out scratch");
    NEED(A_RES, (uint64_t)nb * sizeof(cbc_block_result), "hipMalloc results");
    NEED(A_OFF, ((uint64_t)nb + 1) * 8, "hipMalloc offsets");
    if (two_bit) {
        NEED(A_CODES, ((hb->seq_bytes + 15) / 16) * 4 + 16, "hipMalloc 2-bit codes");
        if (n_seq_runs) NEED(A_RUNS, n_seq_runs * sizeof(cbc_2bit_run_dev), "hipMalloc 2-bit runs");
        if (n_seq_runs > 0x7fffffffull) { rc = set_err(ctx, CBC_E_ARG, "2-bit transport: too many runs", hipSuccess); goto done; }
    }
    tm.alloc_s = wall_now() - T0;
    {
        uint8_t *d_recs = (uint8_t *)ctx->arena[A_RECS].p, *d_seq = d_seq_ext ? NULL : (uint8_t *)ctx->arena[A_SEQ].p;
        uint32_t *d_tok = d_tok_ext ? NULL : (uint32_t *)ctx->arena[A_TOK].p, *d_codes = (uint32_t *)ctx->arena[A_CODES].p;
        cbc_block_desc *d_blocks = (cbc_block_desc *)ctx->arena[A_BLOCKS].p;
        cbc_block_result *d_res = (cbc_block_result *)ctx->arena[A_RES].p;
        hipStream_t sc = ctx->s_copy;
        cbc_chunk_plan P;
        cbc_plan_chunks(hb->blocks, nb, hb->n_recs, hb->seq_bytes, hb->n_tok,
                        hb->n_recs * 16 + (d_seq_ext ? 0 : seq_codes ? hb->seq_bytes / 4 : hb->seq_bytes) + (d_tok_ext ? 0 : ntok * 4),
                        !long_reads, &P);
        tm.n_chunks = P.n_chunks;
        /* small things first: descriptors, names, result slots, exception runs */
        GO(hipMemcpyAsync(d_blocks, hb->blocks, (uint64_t)nb * sizeof(cbc_block_desc), hipMemcpyHostToDevice, sc), "H2D blocks");
        GO(hipMemcpyAsync(ctx->arena[A_NAMES].p, hb->names, hb->names_bytes, hipMemcpyHostToDevice, sc), "H2D names");
        GO(hipMemsetAsync(d_res, 0xff, (uint64_t)nb * sizeof(cbc_block_result), sc), "memset results");
        if (two_bit && n_seq_runs)
            GO(hipMemcpyAsync(ctx->arena[A_RUNS].p, seq_runs, n_seq_runs * sizeof(cbc_2bit_run_dev), hipMemcpyHostToDevice, sc), "H2D 2-bit runs");
        tm.h2d_bytes = (uint64_t)nb * sizeof(cbc_block_desc) + hb->names_bytes + (two_bit ? n_seq_runs * sizeof(cbc_2bit_run_dev) : 0);
        for (uint32_t c = 0; c < P.n_chunks; c++) {
            const cbc_chunk &k = P.c[c];
            GO(hipMemcpyAsync(d_recs + k.r0 * 16, (const uint8_t *)hb->recs + k.r0 * 16, (k.r1 - k.r0) * 16, hipMemcpyHostToDevice, sc), "H2D recs");
            tm.h2d_bytes += (k.r1 - k.r0) * 16;
            if (two_bit) {                                         /* 2-bit transport: a quarter of the bytes cross PCIe, expanded on the device */
                if (k.w1 > k.w0) GO(hipMemcpyAsync(d_codes + k.w0, seq_codes + k.w0, (k.w1 - k.w0) * 4, hipMemcpyHostToDevice, sc), "H2D 2-bit codes");
                tm.h2d_bytes += (k.w1 - k.w0) * 4;
            } else if (!d_seq_ext && k.s1 > k.s0) {
                GO(hipMemcpyAsync(d_seq + k.s0, hb->seq + k.s0, k.s1 - k.s0, hipMemcpyHostToDevice, sc), "H2D seq");
                tm.h2d_bytes += k.s1 - k.s0;
            }
            if (!d_tok_ext && k.t1 > k.t0) {
                GO(hipMemcpyAsync(d_tok + k.t0, hb->tok + k.t0, (k.t1 - k.t0) * 4, hipMemcpyHostToDevice, sc), "H2D tok");
                tm.h2d_bytes += (k.t1 - k.t0) * 4;
            }
            if (two_bit && k.w1 > k.w0) {
                /* on the copy stream, in chunk order: chunks meet inside a code word, which chunk c expands and patches with
                 * its runs, and chunk c + 1's encode reads it.  (A cross-stream event behind each expansion instead cost
                 * 2.5 ms of a cfg2 call; this costs 0.2-0.4 ms: profiles/host_pipeline_ab.json) */
                if (k.w1 - k.w0 > 0x7fffffffull * 256ull) { rc = set_err(ctx, CBC_E_ARG, "2-bit transport: too many words", hipSuccess); goto done; }
                hipLaunchKernelGGL(cbc_expand_2bit_kernel, dim3((unsigned)((k.w1 - k.w0 + 255) / 256)), dim3(256), 0, sc,
                                   (const uint32_t *)(d_codes + k.w0), k.w1 - k.w0, d_seq + k.w0 * 16, hb->seq_bytes - k.w0 * 16);
                GO(hipGetLastError(), "launch cbc_expand_2bit_kernel");
                if (n_seq_runs) {
                    hipLaunchKernelGGL(cbc_apply_runs_kernel, dim3((unsigned)n_seq_runs), dim3(256), 0, sc,
                                       (const cbc_2bit_run_dev *)ctx->arena[A_RUNS].p, n_seq_runs, d_seq, hb->seq_bytes, k.w0 * 16, k.w1 * 16);
                    GO(hipGetLastError(), "launch cbc_apply_runs_kernel");
                }
            }
            GO(hipEventRecord(ctx->ev_chunk[c], sc), "hipEventRecord");
            hipStream_t ks = ctx->s_k[c % CBC_N_KSTREAMS];
            GO(hipStreamWaitEvent(ks, ctx->ev_chunk[c], 0), "hipStreamWaitEvent");
            cbc_device_batch db;
            memset(&db, 0, sizeof db);
            db.d_recs = (const cbc_read_rec *)d_recs; db.d_seq = d_seq_ext ? d_seq_ext : d_seq; db.d_tok = d_tok_ext ? d_tok_ext : d_tok;
            db.d_names = (const uint8_t *)ctx->arena[A_NAMES].p; db.d_blocks = d_blocks + k.b0; db.n_blocks = k.b1 - k.b0;
            db.d_ref = ctx->d_ref; db.ref_bytes = ctx->ref_bytes; db.d_out = (uint8_t *)ctx->arena[A_OUT].p; db.out_bytes = scratch;
            db.d_results = d_res + k.b0; db.seq_bytes = hb->seq_bytes; db.n_tok = ntok; db.n_recs = hb->n_recs;
            db.caps = hb->caps;
            rc = long_reads ? cbc_gpu_long_encode_blocks_device(ctx, &db, ks) : encode_blocks_launch(ctx, &db, ks, nb);
            if (rc) goto done;
        }
        /* the context's own stream joins the kernel streams, then: sizes -> offsets -> compaction -> D2H */
        for (int k = 0; k < CBC_N_KSTREAMS; k++) {
            GO(hipEventRecord(ctx->ev_done[k], ctx->s_k[k]), "hipEventRecord");
            GO(hipStreamWaitEvent(ctx->stream, ctx->ev_done[k], 0), "hipStreamWaitEvent");
        }
        tm.issue_s = wall_now() - T0;
        hipLaunchKernelGGL(cbc_scan_sizes_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const cbc_block_result *)d_res,
                           (uint64_t *)ctx->arena[A_OFF].p, nb);
        GO(hipGetLastError(), "launch cbc_scan_sizes_kernel");
        res = results ? results : (cbc_block_result *)malloc((size_t)nb * sizeof(cbc_block_result));
        if (!res) { rc = CBC_E_NOMEM; goto done; }
        GO(hipMemcpyAsync(res, d_res, (uint64_t)nb * sizeof(cbc_block_result), hipMemcpyDeviceToHost, ctx->stream), "D2H results");
        GO(hipMemcpyAsync(out_offsets, ctx->arena[A_OFF].p, ((uint64_t)nb + 1) * 8, hipMemcpyDeviceToHost, ctx->stream), "D2H offsets");
        GO(hipStreamSynchronize(ctx->stream), "encode kernel");
        tm.kernels_done_s = wall_now() - T0;
        /* the compacted bitstreams (2 bytes per read) go where the batch's bases were: they are dead now, and a second
         * worst-case-sized buffer would cost more to allocate than the whole call takes */
        total = out_offsets[nb];
        if (!d_seq_ext && total <= ctx->arena[A_SEQ].cap) d_compact = (uint8_t *)ctx->arena[A_SEQ].p;
        else { NEED(A_PACKED, total + 16, "hipMalloc packed"); d_compact = (uint8_t *)ctx->arena[A_PACKED].p; }
        if (total) {
            hipLaunchKernelGGL(cbc_compact_kernel, dim3(nb), dim3(256), 0, ctx->stream, (const uint8_t *)ctx->arena[A_OUT].p,
                               (const cbc_block_desc *)d_blocks, (const uint64_t *)ctx->arena[A_OFF].p, d_compact, total, nb);
            GO(hipGetLastError(), "launch cbc_compact_kernel");
        }
    }
    rc = blocks_failed(ctx, res, nb, "failed");
    if (!out) {
        /* keep them: appended to the stash (a grow-with-copy buffer), for cbc_gpu_group_gather / cbc_gpu_stash_fetch */
        if (total) {
            const uint64_t need = ctx->stash_len + total + 16;
            if (ctx->arena[A_STASH].cap < need) {
                void *np = NULL; const uint64_t want = (need + (need >> 1) + (4ull << 20)) & ~((2ull << 20) - 1);
                GO(hipMalloc(&np, want), "hipMalloc stash");
                if (ctx->stash_len) GO(hipMemcpyAsync(np, ctx->arena[A_STASH].p, ctx->stash_len, hipMemcpyDeviceToDevice, ctx->stream), "stash copy");
                GO(hipStreamSynchronize(ctx->stream), "stash copy");
                if (ctx->arena[A_STASH].p) (void)hipFree(ctx->arena[A_STASH].p);
                ctx->arena[A_STASH].p = np; ctx->arena[A_STASH].cap = want;
            }
            GO(hipMemcpyAsync((uint8_t *)ctx->arena[A_STASH].p + ctx->stash_len, d_compact, total, hipMemcpyDeviceToDevice, ctx->stream), "D2D stash");
            GO(hipStreamSynchronize(ctx->stream), "D2D stash");
            ctx->stash_len += total;
        }
    } else {
        if (total > out_cap) { rc = set_err(ctx, CBC_E_ARG, "out_cap too small for the compacted payloads", hipSuccess); goto done; }
        if (total) {
            GO(hipMemcpyAsync(out, d_compact, total, hipMemcpyDeviceToHost, ctx->stream), "D2H payloads");
            GO(hipStreamSynchronize(ctx->stream), "D2H payloads");
        }
    }
    tm.d2h_bytes = total + (uint64_t)nb * (sizeof(cbc_block_result) + 8) + 8;
done:
    if (rc && rc != CBC_E_BLOCK) (void)hipDeviceSynchronize();   /* nothing of a failed call may still be running over the arenas */
    if (res && res != results) free(res);
    tm.total_s = wall_now() - T0;
    ctx->last_e2e = tm;
    return rc;
}

/* host-buffer entry points: payload areas from the caps alone (O(blocks)); a batch whose cap_var is not a bound -- not from
 * the packers -- gets OUT_FULL / CAP_VAR statuses from the kernel, never a wrong byte */
API int cbc_gpu_encode_blocks(cbc_gpu_ctx *ctx, const cbc_host_batch *hb, uint8_t *out, uint64_t out_cap,
                              uint64_t *out_offsets, cbc_block_result *results)
{
    if (!hb || !hb->seq) return CBC_E_ARG;
    return encode_blocks_impl(ctx, hb, cbc_plan_output_caps(hb->blocks, hb->n_blocks, &hb->caps), NULL, NULL, 0,
                              out, out_cap, out_offsets, results);
}
API int cbc_gpu_encode_blocks_2bit(cbc_gpu_ctx *ctx, const cbc_host_batch *hb, const uint32_t *seq_codes, const cbc_2bit_run_dev *seq_runs,
                                   uint64_t n_seq_runs, uint8_t *out, uint64_t out_cap, uint64_t *out_offsets, cbc_block_result *results)
{
    if (!hb || !seq_codes || (n_seq_runs && !seq_runs)) return CBC_E_ARG;
    return encode_blocks_impl(ctx, hb, cbc_plan_output_caps(hb->blocks, hb->n_blocks, &hb->caps), seq_codes, seq_runs, n_seq_runs,
                              out, out_cap, out_offsets, results);
}

API int cbc_gpu_last_e2e(cbc_gpu_ctx *ctx, cbc_e2e_times *out)
{
    if (!ctx || !out) return CBC_E_ARG;
    *out = ctx->last_e2e;
    return CBC_OK;
}

API int cbc_gpu_host_register(cbc_gpu_ctx *ctx, const void *p, uint64_t bytes)
{
    if (!ctx || !p || !bytes) return CBC_E_ARG;
    HIPCHK(hipSetDevice(ctx->device), "hipSetDevice");
    HIPCHK(hipHostRegister((void *)p, bytes, hipHostRegisterDefault), "hipHostRegister");
    return CBC_OK;
}
API int cbc_gpu_host_unregister(cbc_gpu_ctx *ctx, const void *p)
{
    if (!ctx || !p) return CBC_E_ARG;
    HIPCHK(hipSetDevice(ctx->device), "hipSetDevice");
    HIPCHK(hipHostUnregister((void *)p), "hipHostUnregister");
    return CBC_OK;
}

/* ------------------------------------------------------------------------------------------------
 * the exchange step of the multi-device path: every device's bitstreams to device 0 over RCCL
 * (grouped ncclSend / ncclRecv over xGMI), checksummed on both sides, then one D2H.  One process, one context per device --
 * the shape of `cbc --devices a,b,...`; bench.py's one-process-per-GPU form makes the same exchange through
 * torch.distributed's "nccl" backend, which is this library too.  librccl.so is loaded here, not at program start.
 * ---------------------------------------------------------------------------------------------- */
struct cbc_rccl_api {
    void *so;
    ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *);
    ncclResult_t (*CommDestroy)(ncclComm_t);
    ncclResult_t (*GroupStart)(void);
    ncclResult_t (*GroupEnd)(void);
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t);
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t);
    const char *(*GetErrorString)(ncclResult_t);
};
struct cbc_gpu_group { int n; cbc_gpu_ctx **ctx; ncclComm_t *comm; cbc_rccl_api api; char err[256]; };

static int rccl_load(cbc_rccl_api *a, char *err, size_t errlen)
{
    const char *names[] = { "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1" };
    a->so = NULL;
    for (unsigned k = 0; k < 3 && !a->so; k++) a->so = dlopen(names[k], RTLD_NOW | RTLD_LOCAL);
    if (!a->so) { snprintf(err, errlen, "cannot load librccl: %s", dlerror()); return CBC_E_NODEV; }
#define SYM(field, name) do { *(void **)&a->field = dlsym(a->so, name); if (!a->field) { snprintf(err, errlen, "librccl has no %s", name); return CBC_E_NODEV; } } while (0)
    SYM(CommInitAll, "ncclCommInitAll"); SYM(CommDestroy, "ncclCommDestroy"); SYM(GroupStart, "ncclGroupStart"); SYM(GroupEnd, "ncclGroupEnd");
    SYM(Send, "ncclSend"); SYM(Recv, "ncclRecv"); SYM(GetErrorString, "ncclGetErrorString");
#undef SYM
    return CBC_OK;
}

API const char *cbc_gpu_group_last_error(cbc_gpu_group *g) { return g ? g->err : "no group"; }

API void cbc_gpu_group_destroy(cbc_gpu_group *g)
{
    if (!g) return;
    if (g->comm) { for (int k = 0; k < g->n; k++) if (g->comm[k]) { (void)hipSetDevice(g->ctx[k]->device); (void)g->api.CommDestroy(g->comm[k]); } }
    free(g->comm); free(g->ctx);
    /* the library stays loaded: unloading RCCL while HIP is alive is not worth the risk */
    delete g;
}

API int cbc_gpu_group_create(cbc_gpu_ctx *const *ctxs, int n, cbc_gpu_group **out)
{
    if (!ctxs || !out || n < 1 || n > 64) return CBC_E_ARG;
    *out = NULL;
    for (int k = 0; k < n; k++) { if (!ctxs[k]) return CBC_E_ARG; for (int j = 0; j < k; j++) if (ctxs[j]->device == ctxs[k]->device) return CBC_E_ARG; }   /* one rank per device */
    cbc_gpu_group *g = new (std::nothrow) cbc_gpu_group();
    if (!g) return CBC_E_NOMEM;
    memset(g, 0, sizeof *g);
    g->n = n;
    g->ctx = (cbc_gpu_ctx **)calloc((size_t)n, sizeof(cbc_gpu_ctx *)); g->comm = (ncclComm_t *)calloc((size_t)n, sizeof(ncclComm_t));
    int *devs = (int *)calloc((size_t)n, sizeof(int));
    int rc = (g->ctx && g->comm && devs) ? CBC_OK : CBC_E_NOMEM;
    if (!rc) rc = rccl_load(&g->api, g->err, sizeof g->err);
    if (!rc) {
        for (int k = 0; k < n; k++) { g->ctx[k] = ctxs[k]; devs[k] = ctxs[k]->device; }
        const ncclResult_t r = g->api.CommInitAll(g->comm, n, devs);
        if (r != ncclSuccess) { snprintf(g->err, sizeof g->err, "ncclCommInitAll: %s", g->api.GetErrorString(r)); rc = CBC_E_NODEV; memset(g->comm, 0, (size_t)n * sizeof(ncclComm_t)); }
    }
    free(devs);
    if (rc) { if (ctxs[0]) snprintf(ctxs[0]->err, sizeof ctxs[0]->err, "%s", g->err); cbc_gpu_group_destroy(g); return rc; }
    *out = g;
    return CBC_OK;
}

API int cbc_gpu_stash_reset(cbc_gpu_ctx *ctx) { if (!ctx) return CBC_E_ARG; ctx->stash_len = 0; return CBC_OK; }
API uint64_t cbc_gpu_stash_bytes(cbc_gpu_ctx *ctx) { return ctx ? ctx->stash_len : 0; }
API int cbc_gpu_stash_fetch(cbc_gpu_ctx *ctx, uint8_t *out, uint64_t out_cap)
{
    if (!ctx || (ctx->stash_len && !out) || out_cap < ctx->stash_len) return CBC_E_ARG;
    HIPCHK(hipSetDevice(ctx->device), "hipSetDevice");
    if (ctx->stash_len) HIPCHK(hipMemcpy(out, ctx->arena[A_STASH].p, ctx->stash_len, hipMemcpyDeviceToHost), "D2H stash");
    return CBC_OK;
}

static int device_checksum_now(cbc_gpu_ctx *ctx, const uint8_t *d, uint64_t n, uint64_t *sum)
{
    int rc = arena_need(ctx, A_CNT, 8, "hipMalloc checksum"); if (rc) return rc;
    rc = cbc_gpu_checksum_device(ctx, d, n, (uint64_t *)ctx->arena[A_CNT].p, CBC_CTX_STREAM); if (rc) return rc;
    HIPCHK(hipMemcpyAsync(sum, ctx->arena[A_CNT].p, 8, hipMemcpyDeviceToHost, ctx->stream), "D2H checksum");
    HIPCHK(hipStreamSynchronize(ctx->stream), "checksum");
    return CBC_OK;
}

/* Member k's stash -> out[sum of the earlier members' bytes ...], through member 0's device.  nbytes[k] / sums[k] (may be
 * NULL): what member k held and the checksum it took of it before the exchange; the call fails with CBC_E_IO when what
 * member 0 received sums to something else. */
API int cbc_gpu_group_gather(cbc_gpu_group *g, uint8_t *out, uint64_t out_cap, uint64_t *nbytes, uint64_t *sums)
{
    if (!g || !nbytes) return CBC_E_ARG;
    cbc_gpu_ctx *c0 = g->ctx[0];
    cbc_gpu_ctx *ctx = c0;                                      /* for HIPCHK / set_err */
    uint64_t total = 0, sent[64], got = 0;
    for (int k = 0; k < g->n; k++) { nbytes[k] = g->ctx[k]->stash_len; total += nbytes[k]; }
    if (total > out_cap || (total && !out)) return set_err(c0, CBC_E_ARG, "out_cap too small for the gathered bitstreams", hipSuccess);
    for (int k = 0; k < g->n; k++) {                          /* every member sums its own bytes on its own device */
        cbc_gpu_ctx *ck = g->ctx[k];
        HIPCHK(hipSetDevice(ck->device), "hipSetDevice");
        int rc = device_checksum_now(ck, (const uint8_t *)ck->arena[A_STASH].p, nbytes[k], &sent[k]); if (rc) return rc;
        if (sums) sums[k] = sent[k];
    }
    HIPCHK(hipSetDevice(c0->device), "hipSetDevice");
    { int rc = arena_need(c0, A_GATHER, total + 16, "hipMalloc gather"); if (rc) return rc; }
    uint8_t *dst = (uint8_t *)c0->arena[A_GATHER].p;
    /* one group: every send and its receive (a one-member group sends to itself: the self-test of the call sites) */
    ncclResult_t r = g->api.GroupStart();
    uint64_t at = 0;
    for (int k = 0; k < g->n && r == ncclSuccess; k++) {
        if (nbytes[k]) {
            (void)hipSetDevice(g->ctx[k]->device);
            r = g->api.Send(g->ctx[k]->arena[A_STASH].p, (size_t)nbytes[k], ncclUint8, 0, g->comm[k], g->ctx[k]->stream);
            if (r == ncclSuccess) { (void)hipSetDevice(c0->device); r = g->api.Recv(dst + at, (size_t)nbytes[k], ncclUint8, k, g->comm[0], c0->stream); }
        }
        at += nbytes[k];
    }
    { const ncclResult_t e = g->api.GroupEnd(); if (r == ncclSuccess) r = e; }
    if (r != ncclSuccess) { snprintf(g->err, sizeof g->err, "RCCL send/recv: %s", g->api.GetErrorString(r)); return set_err(c0, CBC_E_NODEV, g->err, hipSuccess); }
    for (int k = 0; k < g->n; k++) { HIPCHK(hipSetDevice(g->ctx[k]->device), "hipSetDevice"); HIPCHK(hipStreamSynchronize(g->ctx[k]->stream), "RCCL exchange"); }
    HIPCHK(hipSetDevice(c0->device), "hipSetDevice");
    at = 0;
    for (int k = 0; k < g->n; k++) {                          /* ... and member 0 sums what arrived */
        int rc = device_checksum_now(c0, dst + at, nbytes[k], &got); if (rc) return rc;
        if (got != sent[k]) { snprintf(g->err, sizeof g->err, "member %d: checksum %016llx sent, %016llx received", k, (unsigned long long)sent[k], (unsigned long long)got); return set_err(c0, CBC_E_IO, g->err, hipSuccess); }
        at += nbytes[k];
    }
    if (total) HIPCHK(hipMemcpy(out, dst, total, hipMemcpyDeviceToHost), "D2H gathered bitstreams");
    return CBC_OK;
}

/* ------------------------------------------------------------------------------------------------
 * decode direction
 * ---------------------------------------------------------------------------------------------- */
API uint32_t cbc_gpu_decode_lds_bytes(const cbc_lds_caps *caps) { return caps ? cbc_plan_dec_lds_bytes(caps) : 0; }

/* smax = 0: the plain decoder; otherwise the span-reporting one (region decode), with E the one that reports its edits too */
static int decode_blocks_launch(cbc_gpu_ctx *ctx, const cbc_dec_device_batch *b, void *hip_stream, uint32_t smax, const cbc_dec_edits *E = NULL)
{
    if (!ctx || !b) return CBC_E_ARG;
    if (b->n_blocks == 0) return CBC_OK;
    if (!b->d_in || !b->d_blocks || !b->d_ref || !b->d_recs || !b->d_seq || !b->d_results || !b->d_var_scratch)
        return set_err(ctx, CBC_E_ARG, "null device pointer in cbc_dec_device_batch", hipSuccess);
    if (b->caps.cap_pos < 2 || b->caps.cap_pos > 8192 || b->caps.cap_var < 1 || b->caps.cap_var > 32768)
        return set_err(ctx, CBC_E_ARG, "lds caps out of range", hipSuccess);
    const uint32_t lds = cbc_plan_dec_lds_bytes(&b->caps);
    if (lds > 160u * 1024u) return set_err(ctx, CBC_E_ARG, "lds caps need more than 160 KiB", hipSuccess);
    HIPCHK(hipSetDevice(ctx->device), "hipSetDevice");
    hipStream_t s = hip_stream == CBC_CTX_STREAM ? ctx->stream : (hipStream_t)hip_stream;
    cbc_dec_args A;
    A.in = b->d_in; A.blocks = b->d_blocks; A.ref = b->d_ref; A.recs = b->d_recs; A.seq = b->d_seq; A.results = b->d_results;
    A.in_bytes = b->in_bytes; A.ref_bytes = b->ref_bytes; A.n_recs = b->n_recs; A.seq_bytes = b->seq_bytes;
    A.n_blocks = b->n_blocks; A.cap_pos = b->caps.cap_pos; A.cap_var = b->caps.cap_var;
    A.var_scratch = b->d_var_scratch; A.var_scratch_words = b->var_scratch_words;
    HIPCHK(hipEventRecord(ctx->ev0, s), "hipEventRecord");
    if (smax && E) hipLaunchKernelGGL(cbc_decode_blocks_edits_kernel, dim3(b->n_blocks), dim3(64), lds, s, A, smax, *E);
    else if (smax) hipLaunchKernelGGL(cbc_decode_blocks_span_kernel, dim3(b->n_blocks), dim3(64), lds, s, A, smax);
    else hipLaunchKernelGGL(cbc_decode_blocks_kernel, dim3(b->n_blocks), dim3(64), lds, s, A);
    HIPCHK(hipGetLastError(), "launch cbc_decode_blocks_kernel");
    HIPCHK(hipEventRecord(ctx->ev1, s), "hipEventRecord");
    ctx->have_timing = 1;
    return CBC_OK;
}

API int cbc_gpu_decode_blocks_device(cbc_gpu_ctx *ctx, const cbc_dec_device_batch *b, void *hip_stream)
{
    return decode_blocks_launch(ctx, b, hip_stream, 0u);
}

/* for the post-decode stage (cbc_gpu_post.hip), whose every family scans its sizes with this kernel */
void launch_scan_sizes(hipStream_t s, const cbc_block_result *sizes, uint64_t *offsets, uint32_t n)
{
    hipLaunchKernelGGL(cbc_scan_sizes_kernel, dim3(1), dim3(1024), 0, s, sizes, offsets, n);
}

/* The host-buffer decode path as a pipeline, mirror of encode_blocks_impl: the payloads (2 bytes per read) go H2D at once;
 * the blocks are decoded in chunks (cbc_plan_chunks) on the kernel streams, and chunk c's records and bases (bytes, or 2-bit
 * rows packed by cbc_pack_2bit_kernel) come back on the copy stream while the later chunks are still being decoded.  Device
 * arrays are the context's arenas.  Long reads (their launches share the context's table scratch, A_LSCR; the long decoder
 * takes no var scratch) are one chunk.  So is a call with a post-decode stage (rg->kind != POST_NONE): nothing comes back
 * before its output is built, so its four steps (cbc_gpu_post.hip) -- post_arenas, post_h2d, post_launch with the launch sequence
 * of the kind, post_fetch_sizes / post_fetch_output -- hang off the one chunk, on its kernel stream, and take the place of the
 * chunked D2H. */
static int decode_blocks_impl(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, cbc_dec_block_desc *blocks,
                              uint32_t n_blocks, const cbc_lds_caps *caps, cbc_read_rec *recs, uint64_t n_recs,
                              uint8_t *seq, uint64_t seq_bytes, uint32_t *codes_out, uint64_t *exc_idx, uint8_t *exc_val,
                              uint64_t exc_cap, uint64_t *n_exc, cbc_block_result *results, const post_req *rg = NULL,
                              bool long_reads = false)
{
    if (!ctx->d_ref) return set_err(ctx, CBC_E_ARG, "cbc_gpu_upload_reference has not been called", hipSuccess);
    if (n_blocks == 0) return CBC_OK;
    HIPCHK(hipSetDevice(ctx->device), "hipSetDevice");
    const double T0 = wall_now();
    cbc_e2e_times tm; memset(&tm, 0, sizeof tm);
    const bool two_bit = codes_out != NULL, post = rg && rg->kind != POST_NONE, edits = rg && rg->smax && rg->edits_per_read;
    const post_sizes z = post_sizes_of(rg, n_blocks, n_recs);
    post_got pg; memset(&pg, 0, sizeof pg);
    const uint32_t stride = blocks[0].seq_stride;
    cbc_block_result *res = NULL;
    int rc = CBC_OK;
    const uint64_t n_words = two_bit ? n_recs * (stride >> 4) : 0;
    unsigned long long got = 0;
    if (!long_reads) NEED(A_VS, (uint64_t)n_blocks * caps->cap_var * 4 + 16, "hipMalloc var scratch");
    NEED(A_IN, in_bytes + 16, "hipMalloc in");
    NEED(A_BLOCKS, (uint64_t)n_blocks * sizeof(cbc_dec_block_desc), "hipMalloc blocks");
    NEED(A_RECS, n_recs * sizeof(cbc_read_rec) + 16, "hipMalloc recs");
    NEED(A_SEQ, seq_bytes + 32, "hipMalloc seq");
    NEED(A_RES, (uint64_t)n_blocks * sizeof(cbc_block_result), "hipMalloc results");
    if (two_bit) {
        NEED(A_CODES, n_words * 4 + 16, "hipMalloc codes");
        NEED(A_EXC_I, (exc_cap ? exc_cap : 1) * 8, "hipMalloc exceptions");
        NEED(A_EXC_V, (exc_cap ? exc_cap : 1), "hipMalloc exceptions");
        NEED(A_CNT, 8, "hipMalloc counter");
    }
    if (edits) {
        NEED(A_ESIDE, n_recs * 8 + 16, "hipMalloc edit side array");
        if (arena_need(ctx, A_EARENA, n_recs * rg->edits_per_read * 2 + 16, "hipMalloc edit arena")) {
            (void)hipGetLastError();
            rc = set_err(ctx, CBC_E_NOMEM, "no device memory for the edit arena (2 bytes per read and entry of edits_per_read)", hipSuccess);
            goto done;
        }
    }
    if (post && (rc = post_arenas(ctx, rg, z, n_blocks, n_recs)) != CBC_OK) goto done;
    tm.alloc_s = wall_now() - T0;
    {
        uint8_t *d_in = (uint8_t *)ctx->arena[A_IN].p, *d_seq = (uint8_t *)ctx->arena[A_SEQ].p;
        cbc_dec_block_desc *d_blocks = (cbc_dec_block_desc *)ctx->arena[A_BLOCKS].p;
        cbc_read_rec *d_recs = (cbc_read_rec *)ctx->arena[A_RECS].p;
        cbc_block_result *d_res = (cbc_block_result *)ctx->arena[A_RES].p;
        hipStream_t sc = ctx->s_copy;
        GO(hipMemsetAsync(d_in + in_bytes, 0, 16, sc), "memset pad");
        GO(hipMemcpyAsync(d_in, in, in_bytes, hipMemcpyHostToDevice, sc), "H2D payloads");
        GO(hipMemcpyAsync(d_blocks, blocks, (uint64_t)n_blocks * sizeof(cbc_dec_block_desc), hipMemcpyHostToDevice, sc), "H2D blocks");
        GO(hipMemsetAsync(d_res, 0xff, (uint64_t)n_blocks * sizeof(cbc_block_result), sc), "memset results");
        if (two_bit) GO(hipMemsetAsync(ctx->arena[A_CNT].p, 0, 8, sc), "memset counter");
        if (edits) GO(hipMemsetAsync(ctx->arena[A_ESIDE].p, 0, n_recs * 8, sc), "memset edit side array");
        if (post && (rc = post_h2d(ctx, rg, n_blocks, sc)) != CBC_OK) goto done;
        GO(hipEventRecord(ctx->ev_done[0], sc), "hipEventRecord");       /* inputs are on the device */
        tm.h2d_bytes = in_bytes + (uint64_t)n_blocks * sizeof(cbc_dec_block_desc);
        cbc_chunk_plan P;
        cbc_plan_chunks(blocks, n_blocks, n_recs, seq_bytes, 0, n_recs * 16 + (two_bit ? n_words * 4 : seq_bytes), !long_reads && !post, &P);
        tm.n_chunks = P.n_chunks;
        for (uint32_t c = 0; c < P.n_chunks; c++) {
            const cbc_chunk &k = P.c[c];
            hipStream_t ks = ctx->s_k[c % CBC_N_KSTREAMS];
            GO(hipStreamWaitEvent(ks, ctx->ev_done[0], 0), "hipStreamWaitEvent");
            if (k.s1 > k.s0) GO(hipMemsetAsync(d_seq + k.s0, 0, k.s1 - k.s0 + (k.b1 == n_blocks ? 32 : 0), ks), "memset seq");
            cbc_dec_device_batch db;
            memset(&db, 0, sizeof db);
            db.d_in = d_in; db.in_bytes = in_bytes + 16; db.d_blocks = d_blocks + k.b0; db.n_blocks = k.b1 - k.b0;
            db.d_ref = ctx->d_ref; db.ref_bytes = ctx->ref_bytes; db.d_recs = d_recs; db.n_recs = n_recs;
            db.d_seq = d_seq; db.d_results = d_res + k.b0; db.caps = *caps;
            if (post) GO(hipEventRecord(ctx->ev_rg[0], ks), "hipEventRecord");
            if (long_reads) {
                db.seq_bytes = seq_bytes + 16;
                rc = cbc_gpu_long_decode_blocks_device(ctx, &db, ks);
            } else {
                db.seq_bytes = seq_bytes + 32;
                db.d_var_scratch = (uint32_t *)ctx->arena[A_VS].p + (uint64_t)k.b0 * caps->cap_var;
                db.var_scratch_words = (uint64_t)(k.b1 - k.b0) * caps->cap_var;
                cbc_dec_edits de;
                memset(&de, 0, sizeof de);
                if (edits) {
                    de.side = (uint32_t *)ctx->arena[A_ESIDE].p; de.arena = (uint16_t *)ctx->arena[A_EARENA].p;
                    de.arena_entries = n_recs * rg->edits_per_read; de.per_read = rg->edits_per_read;
                }
                rc = decode_blocks_launch(ctx, &db, ks, rg ? rg->smax : 0u, edits ? &de : NULL);
            }
            if (rc) goto done;
            if (post) {                                        /* one chunk: the stage's launches on the decode's stream */
                GO(hipEventRecord(ctx->ev_rg[1], ks), "hipEventRecord");
                if ((rc = post_launch(ctx, ks, rg, z, n_blocks, n_recs, seq_bytes)) != CBC_OK) goto done;
            }
            if (two_bit && k.r1 > k.r0) {
                const uint64_t w0 = k.r0 * (stride >> 4), w1 = k.r1 * (stride >> 4);
                hipLaunchKernelGGL(cbc_pack_2bit_kernel, dim3((unsigned)((w1 - w0 + 255) / 256)), dim3(256), 0, ks,
                                   (const uint8_t *)d_seq, (const cbc_read_rec *)d_recs, k.r0, k.r1, stride, (uint32_t *)ctx->arena[A_CODES].p,
                                   (uint64_t *)ctx->arena[A_EXC_I].p, (uint8_t *)ctx->arena[A_EXC_V].p, exc_cap, (unsigned long long *)ctx->arena[A_CNT].p);
                GO(hipGetLastError(), "launch cbc_pack_2bit_kernel");
            }
            GO(hipEventRecord(ctx->ev_chunk[c], ks), "hipEventRecord");
        }
        tm.issue_s = wall_now() - T0;
        for (uint32_t c = 0; c < P.n_chunks && !post; c++) {         /* the chunks come back in order while later ones are being decoded */
            const cbc_chunk &k = P.c[c];
            GO(hipStreamWaitEvent(sc, ctx->ev_chunk[c], 0), "hipStreamWaitEvent");
            if (k.r1 > k.r0) GO(hipMemcpyAsync(recs + k.r0, d_recs + k.r0, (k.r1 - k.r0) * sizeof(cbc_read_rec), hipMemcpyDeviceToHost, sc), "D2H recs");
            tm.d2h_bytes += (k.r1 - k.r0) * sizeof(cbc_read_rec);
            if (two_bit) {
                const uint64_t w0 = k.r0 * (stride >> 4), w1 = k.r1 * (stride >> 4);
                if (w1 > w0) GO(hipMemcpyAsync(codes_out + w0, (uint32_t *)ctx->arena[A_CODES].p + w0, (w1 - w0) * 4, hipMemcpyDeviceToHost, sc), "D2H codes");
                tm.d2h_bytes += (w1 - w0) * 4;
            } else if (k.s1 > k.s0) {
                GO(hipMemcpyAsync(seq + k.s0, d_seq + k.s0, k.s1 - k.s0, hipMemcpyDeviceToHost, sc), "D2H seq");
                tm.d2h_bytes += k.s1 - k.s0;
            }
        }
        if (edits && !post) {                                  /* cbc_gpu_decode_blocks_edits: behind the last chunk's records and rows */
            GO(hipMemcpyAsync(rg->edit_side, ctx->arena[A_ESIDE].p, n_recs * 8, hipMemcpyDeviceToHost, sc), "D2H edit side array");
            GO(hipMemcpyAsync(rg->edit_arena, ctx->arena[A_EARENA].p, n_recs * rg->edits_per_read * 2, hipMemcpyDeviceToHost, sc), "D2H edit arena");
            tm.d2h_bytes += n_recs * (8 + 2ull * rg->edits_per_read);
        }
        res = results ? results : (cbc_block_result *)malloc((size_t)n_blocks * sizeof(cbc_block_result));
        if (!res) { rc = CBC_E_NOMEM; goto done; }
        if (post) GO(hipStreamWaitEvent(sc, ctx->ev_chunk[0], 0), "hipStreamWaitEvent");
        GO(hipMemcpyAsync(res, d_res, (uint64_t)n_blocks * sizeof(cbc_block_result), hipMemcpyDeviceToHost, sc), "D2H results");
        if (two_bit) GO(hipMemcpyAsync(&got, ctx->arena[A_CNT].p, 8, hipMemcpyDeviceToHost, sc), "D2H counter");
        if (post && (rc = post_fetch_sizes(ctx, rg, z, n_blocks, sc, &pg)) != CBC_OK) goto done;
        GO(hipStreamSynchronize(sc), "decode kernel");
        tm.kernels_done_s = wall_now() - T0;
        if (post && (rc = post_fetch_output(ctx, rg, z, n_blocks, res, sc, &pg, &tm.d2h_bytes)) != CBC_OK) goto done;
        if (two_bit) {
            *n_exc = got;
            if (got > exc_cap) { rc = set_err(ctx, CBC_E_ARG, "more non-ACGT bases than exc_cap", hipSuccess); goto done; }
            if (got) {
                GO(hipMemcpyAsync(exc_idx, ctx->arena[A_EXC_I].p, got * 8, hipMemcpyDeviceToHost, sc), "D2H exceptions");
                GO(hipMemcpyAsync(exc_val, ctx->arena[A_EXC_V].p, got, hipMemcpyDeviceToHost, sc), "D2H exceptions");
                GO(hipStreamSynchronize(sc), "D2H exceptions");
                tm.d2h_bytes += got * 9;
            }
        }
    }
    rc = blocks_failed(ctx, res, n_blocks, "failed to decode");
done:
    if (rc && rc != CBC_E_BLOCK) (void)hipDeviceSynchronize();
    if (res && res != results) free(res);
    free(pg.cnt); free(pg.stats);
    tm.total_s = wall_now() - T0;
    ctx->last_e2e = tm;
    return rc;
}

API int cbc_gpu_decode_blocks(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, cbc_dec_block_desc *blocks,
                              uint32_t n_blocks, const cbc_lds_caps *caps, cbc_read_rec *recs, uint64_t n_recs,
                              uint8_t *seq, uint64_t seq_bytes, cbc_block_result *results)
{
    if (!ctx || !in || !blocks || !caps || !recs || !seq) return CBC_E_ARG;
    return decode_blocks_impl(ctx, in, in_bytes, blocks, n_blocks, caps, recs, n_recs, seq, seq_bytes, NULL, NULL, NULL, 0, NULL, results);
}

/* The blocks a region / SAM / depth / targets call selected, laid out afresh: payloads from in0, records and rows from 0.
 * With the contig-name tables (SAM, targets) also bn, per block the (offset, length) of its contig's name, and name_sum,
 * the bytes all the reads' contig names take. */
struct name_tables { const uint64_t *window_start; const uint32_t *block_contig; const char *names; uint32_t names_bytes;
                     const uint32_t *contig_name_off; uint32_t n_contigs; };
struct block_layout { cbc_dec_block_desc *bl; uint32_t *bn; uint64_t in0, in1, nrec, name_sum; };

static void layout_free(block_layout *L) { free(L->bl); free(L->bn); L->bl = NULL; L->bn = NULL; }

static int layout_err(cbc_gpu_ctx *ctx, const char *who, const char *what)
{
    char msg[192];
    snprintf(msg, sizeof msg, "%s%s", who, what);
    return set_err(ctx, CBC_E_ARG, msg, hipSuccess);
}

/* `who` opens the messages ("region decode", "SAM decode", "depth", "targets decode").  Per block: its range in `in`, then
 * (nt != NULL) its contig, the name and the window start.  On an error nothing stays allocated; after CBC_OK the caller
 * ends with layout_free. */
static int relayout_blocks(cbc_gpu_ctx *ctx, const char *who, uint64_t in_bytes, const cbc_dec_block_desc *blocks, uint32_t n_blocks,
                           const name_tables *nt, block_layout *L)
{
    memset(L, 0, sizeof *L);
    L->in0 = UINT64_MAX;
    const uint32_t stride = blocks[0].seq_stride;
    if (stride < 4 || stride > 256 || (stride & 3u)) return layout_err(ctx, who, " wants seq_stride in 4..256, a multiple of 4");
    L->bl = (cbc_dec_block_desc *)malloc((size_t)n_blocks * sizeof(cbc_dec_block_desc));
    if (nt) L->bn = (uint32_t *)malloc((size_t)n_blocks * 8);
    if (!L->bl || (nt && !L->bn)) { layout_free(L); return CBC_E_NOMEM; }
    const char *bad = NULL;
    for (uint32_t b = 0; b < n_blocks; b++) {                  /* no sums of caller values that could wrap */
        const cbc_dec_block_desc *d = &blocks[b];
        size_t nl = 0;
        if (d->seq_stride != stride || d->in_off > in_bytes || d->in_bytes > in_bytes - d->in_off || d->n_reads > CBC_MAX_BLOCK_READS) {
            bad = ": block out of range of `in`, or strides differ"; break; }
        if (nt) {
            if (nt->block_contig[b] >= nt->n_contigs || nt->contig_name_off[nt->block_contig[b]] >= nt->names_bytes) {
                bad = ": a block's contig or its name lies outside the tables"; break; }
            const uint32_t off = nt->contig_name_off[nt->block_contig[b]];
            const char *name = nt->names + off;
            nl = strnlen(name, nt->names_bytes - off);
            if (nl == nt->names_bytes - off || nl < 1 || nl > CBC_SAM_MAX_NAME || memchr(name, '\t', nl) || memchr(name, '\n', nl)) {
                bad = ": a contig name is empty, unterminated, longer than 255 bytes or holds a tab or a newline"; break; }
            if (nt->window_start[b] > CBC_SAM_MAX_POS) { bad = ": a block starts past POS 2^31 - 1"; break; }
            L->bn[2 * b] = off; L->bn[2 * b + 1] = (uint32_t)nl;
        }
        if (d->in_off < L->in0) L->in0 = d->in_off;
        if (d->in_off + d->in_bytes > L->in1) L->in1 = d->in_off + d->in_bytes;
        L->bl[b] = *d;
        L->bl[b].rec_base = L->nrec; L->bl[b].seq_base = L->nrec * stride;
        L->nrec += d->n_reads;
        L->name_sum += (uint64_t)d->n_reads * nl;
    }
    if (bad) { layout_free(L); return layout_err(ctx, who, bad); }
    for (uint32_t b = 0; b < n_blocks; b++) L->bl[b].in_off -= L->in0;
    return CBC_OK;
}

/* the request every laid-out call starts from, and the call itself: records and rows stay on the device */
static void post_req_init(post_req *rg, post_kind kind, uint32_t smax, const uint64_t *window_start, uint8_t *text, uint64_t text_cap,
                          uint64_t need, uint64_t *text_bytes, uint64_t *n_selected)
{
    memset(rg, 0, sizeof *rg);
    rg->kind = kind; rg->smax = smax; rg->window_start = window_start; rg->region = 1;
    rg->text = text; rg->text_cap = text_cap < need ? text_cap : need; rg->text_bytes = text_bytes; rg->n_selected = n_selected;
}

static int decode_laid_out(cbc_gpu_ctx *ctx, const uint8_t *in, const block_layout *L, uint32_t n_blocks, const cbc_lds_caps *caps,
                           cbc_block_result *results, const post_req *rg)
{
    return decode_blocks_impl(ctx, in + L->in0, L->in1 - L->in0, L->bl, n_blocks, caps, (cbc_read_rec *)NULL, L->nrec, (uint8_t *)NULL,
                              L->nrec * L->bl[0].seq_stride + 8, NULL, NULL, NULL, 0, NULL, results, rg);
}

/* Kernel times of the most recent call with a post-decode stage, for the entry point that call belongs to (`mine`): out[i] =
 * the time between the i-th and the next of the call's events, for its first n stretches.  The events in the order the call
 * recorded them: ev_rg[0..3], then the histogram's two, or the coverage's four, the extension's five and the quantiles' one, or
 * ev_rg[4]. */
static int last_ms(cbc_gpu_ctx *ctx, bool mine, float *const *out, int n)
{
    if (!mine) return CBC_E_ARG;
    for (int i = 0; i < n; i++) if (!out[i]) return CBC_E_ARG;
    hipEvent_t ev[14];
    int k = 0;
    for (int i = 0; i < 4; i++) ev[k++] = ctx->ev_rg[i];
    if (ctx->last_post == POST_HIST) { ev[k++] = ctx->ev_hist[0]; ev[k++] = ctx->ev_hist[1]; }
    else if (post_is_cov(ctx->last_post)) {
        for (int i = 0; i < 4; i++) ev[k++] = ctx->ev_cov[i];
        for (int i = 0; i < 5; i++) ev[k++] = ctx->ev_covx[i];
        ev[k++] = ctx->ev_quant;
    } else ev[k++] = ctx->ev_rg[4];
    HIPCHK(hipEventSynchronize(ev[n]), "hipEventSynchronize");
    for (int i = 0; i < n; i++) HIPCHK(hipEventElapsedTime(out[i], ev[i], ev[i + 1]), "hipEventElapsedTime");
    return CBC_OK;
}
#define LAST_IS(test) (ctx && (test))                          /* `mine` of last_ms: no context, no kind */

/* The checks the decode entry points share.  `who` opens the message as for relayout_blocks; each returns CBC_OK or the
 * refusal, with the message set. */

/* after the NULL checks and the zeroing of the out-parameters: > 0 go on, otherwise the call's return code (no reference: a
 * refusal; no blocks: CBC_OK; `ptrs`, the pointers a call with blocks needs, not all there: CBC_E_ARG) */
static int call_ready(cbc_gpu_ctx *ctx, uint32_t n_blocks, bool ptrs)
{
    if (!ctx->d_ref) return set_err(ctx, CBC_E_ARG, "cbc_gpu_upload_reference has not been called", hipSuccess);
    if (n_blocks == 0) return CBC_OK;
    return ptrs ? 1 : CBC_E_ARG;
}

/* the window of a region, SAM region (pos_max false), depth or pileup call (true: end <= 2^31 - 1 too) */
static int check_window(cbc_gpu_ctx *ctx, const char *who, uint64_t beg, uint64_t end, uint32_t smax, bool pos_max)
{
    if (smax == 0 || beg < 1 || beg > end || (pos_max && end > CBC_SAM_MAX_POS))
        return layout_err(ctx, who, pos_max ? " wants 1 <= beg <= end <= 2^31 - 1 and smax > 0" : " wants 1 <= beg <= end and smax > 0");
    return CBC_OK;
}

/* the contig name of a depth or pileup call */
static int check_window_name(cbc_gpu_ctx *ctx, const char *who, const char *name, uint32_t name_bytes)
{
    if (name_bytes < 1 || name_bytes > CBC_SAM_MAX_NAME || memchr(name, '\t', name_bytes) || memchr(name, '\n', name_bytes) || memchr(name, 0, name_bytes))
        return layout_err(ctx, who, ": the contig name is empty, longer than 255 bytes or holds a tab, a newline or a NUL");
    return CBC_OK;
}

/* the arena size of a call behind the edits decoder, 0 replaced by the default; who_wants: "pileup wants ", or "" */
static int check_edits(cbc_gpu_ctx *ctx, const char *who_wants, uint32_t *edits_per_read)
{
    if (*edits_per_read == 0) *edits_per_read = CBC_EDITS_PER_READ;
    if (*edits_per_read > CBC_EDITS_MAX) return layout_err(ctx, who_wants, "edits_per_read in 1..510 (0: the default)");
    return CBC_OK;
}

/* the interval table of a target set */
static int check_intervals(cbc_gpu_ctx *ctx, const char *who, const cbc_gpu_targets *t)
{
    for (uint32_t i = 0; i < t->n_iv; i++)
        if (t->iv[2 * i] < 1 || t->iv[2 * i] > t->iv[2 * i + 1] || t->iv[2 * i + 1] > CBC_SAM_MAX_POS)
            return layout_err(ctx, who, ": an interval is not 1 <= beg <= end <= 2^31 - 1");
    return CBC_OK;
}

/* block b's range of the interval table, and (window_start != NULL; with the name tables relayout_blocks looks) its window start */
static int check_block_iv(cbc_gpu_ctx *ctx, const char *who, const cbc_gpu_targets *t, uint32_t b, const uint64_t *window_start)
{
    const uint32_t f = t->block_iv[2 * b], c = t->block_iv[2 * b + 1];
    if (f > t->n_iv || c > t->n_iv - f) return layout_err(ctx, who, ": a block's interval range lies outside the table");
    if (window_start && window_start[b] > CBC_SAM_MAX_POS) return layout_err(ctx, who, ": a block starts past POS 2^31 - 1");
    return CBC_OK;
}

/* region decode: the selected blocks are laid out afresh, decoded with the spans reported, filtered and assembled into text
 * on the device (cbc_region_body.h) */
API int cbc_gpu_decode_region(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const cbc_dec_block_desc *blocks,
                              uint32_t n_blocks, const cbc_lds_caps *caps, const uint64_t *window_start,
                              uint64_t beg, uint64_t end, uint32_t smax, uint8_t *text, uint64_t text_cap,
                              uint64_t *text_bytes, uint64_t *n_selected, cbc_block_result *results)
{
    if (!ctx || !blocks || !caps || !window_start || !text_bytes || !n_selected || (text_cap && !text)) return CBC_E_ARG;
    *text_bytes = 0; *n_selected = 0;
    int rc = call_ready(ctx, n_blocks, in != NULL);
    if (rc <= 0) return rc;
    if ((rc = check_window(ctx, "region decode", beg, end, smax, false))) return rc;
    block_layout L;
    rc = relayout_blocks(ctx, "region decode", in_bytes, blocks, n_blocks, NULL, &L);
    if (rc) return rc;
    post_req rg;                                               /* every read kept: rl + 1 <= stride + 1 bytes each */
    post_req_init(&rg, POST_REGION, smax, window_start, text, text_cap, L.nrec * (blocks[0].seq_stride + 1ull), text_bytes, n_selected);
    rg.beg = beg; rg.end = end;
    rc = decode_laid_out(ctx, in, &L, n_blocks, caps, results, &rg);
    layout_free(&L);
    return rc;
}

API int cbc_gpu_decode_blocks_span(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, cbc_dec_block_desc *blocks,
                                   uint32_t n_blocks, const cbc_lds_caps *caps, uint32_t smax, cbc_read_rec *recs, uint64_t n_recs,
                                   uint8_t *seq, uint64_t seq_bytes, cbc_block_result *results)
{
    if (!ctx || !in || !blocks || !caps || !recs || !seq || smax == 0) return CBC_E_ARG;
    post_req rg;
    memset(&rg, 0, sizeof rg);
    rg.kind = POST_NONE; rg.smax = smax;
    return decode_blocks_impl(ctx, in, in_bytes, blocks, n_blocks, caps, recs, n_recs, seq, seq_bytes, NULL, NULL, NULL, 0, NULL, results, &rg);
}

/* SAM output: the blocks laid out afresh as for a region decode, the per-block name table made and checked on the host,
 * then decode + count + scan + write on the device (cbc_sam_body.h).  cg != NULL: with CIGAR, NM and MD (DESIGN.md section
 * 4.21) -- the edits decoder, and the measure pass in front of the count (cbc_cigar_body.h); the bound on the text is
 * cbc_unpack_sam_cigar_text_cap's. */
struct sam_cigar_opt { uint32_t smax, edits_per_read; };
static int decode_sam_impl(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const cbc_dec_block_desc *blocks,
                           uint32_t n_blocks, const cbc_lds_caps *caps, const uint64_t *window_start,
                           const uint32_t *block_contig, const char *names, uint32_t names_bytes,
                           const uint32_t *contig_name_off, uint32_t n_contigs, const cbc_sam_region *region, const sam_cigar_opt *cg,
                           uint8_t *text, uint64_t text_cap, uint64_t *text_bytes, uint64_t *n_reads, cbc_block_result *results)
{
    if (!ctx || !blocks || !caps || !window_start || !block_contig || !names || !contig_name_off || !text_bytes || !n_reads ||
        (text_cap && !text)) return CBC_E_ARG;
    *text_bytes = 0; *n_reads = 0;
    int rc = call_ready(ctx, n_blocks, in != NULL);
    if (rc <= 0) return rc;
    if (region && (rc = check_window(ctx, "SAM region decode", region->beg, region->end, region->smax, false))) return rc;
    uint32_t edits_per_read = 0;
    if (cg) {
        if (!region && cg->smax == 0) return set_err(ctx, CBC_E_ARG, "SAM decode with CIGAR wants smax > 0 (the container's span bound)", hipSuccess);
        edits_per_read = cg->edits_per_read;
        if ((rc = check_edits(ctx, "SAM decode with CIGAR wants ", &edits_per_read))) return rc;
    }
    const name_tables nt = { window_start, block_contig, names, names_bytes, contig_name_off, n_contigs };
    block_layout L;
    rc = relayout_blocks(ctx, "SAM decode", in_bytes, blocks, n_blocks, &nt, &L);
    if (rc) return rc;
    if (cg && L.nrec > 0x3fffffffull) rc = set_err(ctx, CBC_E_ARG, "SAM decode with CIGAR: more than 2^30 - 1 reads in one call", hipSuccess);
    else {
        post_req rg;                                           /* every read kept, every field (and token) at its longest */
        const uint64_t per_read = cg ? 56ull + 3ull * blocks[0].seq_stride + 16ull * edits_per_read : 35ull + blocks[0].seq_stride;
        post_req_init(&rg, cg ? POST_SAM_CIGAR : POST_SAM, region ? region->smax : cg ? cg->smax : 0u, window_start, text, text_cap,
                      L.nrec * per_read + L.name_sum, text_bytes, n_reads);
        rg.beg = region ? region->beg : 1u; rg.end = region ? region->end : UINT64_MAX; rg.region = region != NULL;
        rg.names = (const uint8_t *)names; rg.names_bytes = names_bytes; rg.block_name = L.bn;
        rg.edits_per_read = edits_per_read;
        rc = decode_laid_out(ctx, in, &L, n_blocks, caps, results, &rg);
    }
    layout_free(&L);
    return rc;
}

API int cbc_gpu_decode_sam(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const cbc_dec_block_desc *blocks,
                           uint32_t n_blocks, const cbc_lds_caps *caps, const uint64_t *window_start,
                           const uint32_t *block_contig, const char *names, uint32_t names_bytes,
                           const uint32_t *contig_name_off, uint32_t n_contigs, const cbc_sam_region *region,
                           uint8_t *text, uint64_t text_cap, uint64_t *text_bytes, uint64_t *n_reads, cbc_block_result *results)
{
    return decode_sam_impl(ctx, in, in_bytes, blocks, n_blocks, caps, window_start, block_contig, names, names_bytes, contig_name_off,
                           n_contigs, region, NULL, text, text_cap, text_bytes, n_reads, results);
}

API int cbc_gpu_decode_sam_cigar(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const cbc_dec_block_desc *blocks,
                                 uint32_t n_blocks, const cbc_lds_caps *caps, const uint64_t *window_start,
                                 const uint32_t *block_contig, const char *names, uint32_t names_bytes,
                                 const uint32_t *contig_name_off, uint32_t n_contigs, const cbc_sam_region *region, uint32_t smax,
                                 uint32_t edits_per_read, uint8_t *text, uint64_t text_cap, uint64_t *text_bytes, uint64_t *n_reads,
                                 cbc_block_result *results)
{
    const sam_cigar_opt cg = { smax, edits_per_read };
    return decode_sam_impl(ctx, in, in_bytes, blocks, n_blocks, caps, window_start, block_contig, names, names_bytes, contig_name_off,
                           n_contigs, region, &cg, text, text_cap, text_bytes, n_reads, results);
}

/* coverage: the window's blocks laid out afresh as for a region decode, then span decode + mark + scan + text on the device
 * (cbc_depth_body.h).  pu != NULL: per-position allele counts -- the edits decoder, then mark + events +
 * scans + text (cbc_pileup_body.h), for the blocks of one contig.  co != NULL (with pu): the consensus record (DESIGN.md section
 * 4.25) -- the pileup's passes up to the tile sums' scan, then the call count, its scan and the record (cbc_consensus_body.h). */
struct pileup_opt { uint32_t min_alt, edits_per_read, min_alt_ppm, by_strand; };
struct consensus_opt { const cbc_consensus_opts *o; uint32_t with_range; cbc_consensus_counts *counts; };
/* the decimal digits of a window's bound, at most ten (end <= 2^31 - 1) */
static uint32_t ndig10(uint64_t x) { uint32_t d = 1; for (; x >= 10u; x /= 10u) d++; return d; }
static int decode_window_impl(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const cbc_dec_block_desc *blocks,
                              uint32_t n_blocks, const cbc_lds_caps *caps, const uint64_t *window_start, const char *name,
                              uint32_t name_bytes, uint64_t beg, uint64_t end, uint32_t smax, uint32_t exclude_flags, const pileup_opt *pu,
                              uint8_t *text, uint64_t text_cap, uint64_t *text_bytes, uint64_t *n_runs, uint64_t *n_reads_kept,
                              cbc_block_result *results, const consensus_opt *co = NULL)
{
    const char *who = co ? "consensus" : pu ? "pileup" : "depth";
    if (!ctx || !blocks || !caps || !window_start || !name || !text_bytes || !n_runs || !n_reads_kept || (text_cap && !text)) return CBC_E_ARG;
    *text_bytes = 0; *n_runs = 0; *n_reads_kept = 0;
    if (co && (co->o->min_depth < 1 || co->o->call_ppm < 1 || co->o->call_ppm > 1000000u || co->o->line_width < 1 || co->o->line_width > 65535u ||
               (co->o->flags & ~(CBC_CONS_SHOW_DEL | CBC_CONS_FILL_REF | CBC_CONS_IUPAC)) || co->with_range > 1u))
        return set_err(ctx, CBC_E_ARG, "consensus wants min_depth >= 1, call_ppm in 1..1000000, line_width in 1..65535, known flag bits and with_range 0 or 1", hipSuccess);
    int rc = call_ready(ctx, n_blocks, in != NULL);
    if (rc <= 0) return rc;
    if ((rc = check_window(ctx, who, beg, end, smax, true))) return rc;
    uint32_t edits_per_read = 0;
    if (pu) {
        if (pu->min_alt < 1) return set_err(ctx, CBC_E_ARG, "pileup wants min_alt >= 1", hipSuccess);
        if (pu->min_alt_ppm > 1000000u || pu->by_strand > 1u)
            return set_err(ctx, CBC_E_ARG, "pileup wants min_alt_ppm in 0..1000000 (0: no fraction rule) and by_strand 0 or 1", hipSuccess);
        edits_per_read = pu->edits_per_read;
        if ((rc = check_edits(ctx, co ? "consensus wants " : "pileup wants ", &edits_per_read))) return rc;
    }
    const bool skip_del = !pu && ctx->skipdel_edits != 0u;            /* cbc_gpu_set_depth_skip_deletions */
    if ((rc = check_window_name(ctx, who, name, name_bytes))) return rc;
    /* one contig: every block's window lies at the same place of the reference */
    for (uint32_t b = 0; pu && b < n_blocks; b++)
        if (blocks[b].ref_off < window_start[b] || blocks[b].ref_off - window_start[b] != blocks[0].ref_off - window_start[0])
            return set_err(ctx, CBC_E_ARG, co ? "consensus takes the blocks of one contig" : "pileup takes the blocks of one contig", hipSuccess);
    block_layout L;
    rc = relayout_blocks(ctx, who, in_bytes, blocks, n_blocks, NULL, &L);
    if (rc) return rc;
    if (L.nrec > 0x3fffffffull) rc = layout_err(ctx, who, ": more than 2^30 - 1 reads in one call");
    else if (L.nrec) {                                         /* blocks without reads: no line */
        /* depth: K reads give at most 2K - 1 runs; pileup, and the depth under skip_del (cbc_unpack_depth_skipdel_text_cap): a line
         * per position of the window at most, and per reference base a kept read spans (span <= smax) */
        const uint64_t w = end - beg + 1u, by_reads = L.nrec * smax, by_pos = w < by_reads ? w : by_reads;
        /* consensus: the header, a byte per position at most, their newlines */
        const uint32_t hdr = co ? name_bytes + 2u + (co->with_range ? 2u + ndig10(beg) + ndig10(end) : 0u) : 0u;
        post_req rg;
        post_req_init(&rg, co ? POST_CONSENSUS : pu ? POST_PILEUP : POST_DEPTH, smax, window_start, text, text_cap,
                      co ? hdr + w + (w + co->o->line_width - 1u) / co->o->line_width :
                      pu ? by_pos * (name_bytes + 102ull + (pu->by_strand ? 77ull : 0ull)) : skip_del ? by_pos * (name_bytes + 34ull) : (2u * L.nrec - 1u) * (name_bytes + 34ull),
                      text_bytes, n_reads_kept);
        rg.beg = beg; rg.end = end;
        rg.names = (const uint8_t *)name; rg.names_bytes = name_bytes; rg.exclude = exclude_flags; rg.n_runs = n_runs;
        if (pu) { rg.edits_per_read = edits_per_read; rg.min_alt = pu->min_alt; rg.ref_c0 = blocks[0].ref_off - window_start[0];
                  rg.min_alt_ppm = pu->min_alt_ppm; rg.by_strand = pu->by_strand != 0u; }
        if (co) { rg.cons = *co->o; rg.with_range = co->with_range; rg.cons_hdr = hdr; rg.cons_counts = co->counts; }
        if (skip_del) { rg.skip_del = true; rg.edits_per_read = ctx->skipdel_edits; }
        rc = decode_laid_out(ctx, in, &L, n_blocks, caps, results, &rg);
    }
    layout_free(&L);
    return rc;
}

API int cbc_gpu_decode_depth(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const cbc_dec_block_desc *blocks,
                             uint32_t n_blocks, const cbc_lds_caps *caps, const uint64_t *window_start, const char *name,
                             uint32_t name_bytes, uint64_t beg, uint64_t end, uint32_t smax, uint32_t exclude_flags,
                             uint8_t *text, uint64_t text_cap, uint64_t *text_bytes, uint64_t *n_runs, uint64_t *n_reads_kept,
                             cbc_block_result *results)
{
    return decode_window_impl(ctx, in, in_bytes, blocks, n_blocks, caps, window_start, name, name_bytes, beg, end, smax, exclude_flags, NULL,
                              text, text_cap, text_bytes, n_runs, n_reads_kept, results);
}

API int cbc_gpu_decode_pileup(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const cbc_dec_block_desc *blocks,
                              uint32_t n_blocks, const cbc_lds_caps *caps, const uint64_t *window_start, const char *name,
                              uint32_t name_bytes, uint64_t beg, uint64_t end, uint32_t smax, uint32_t exclude_flags, uint32_t min_alt,
                              uint32_t edits_per_read, uint8_t *text, uint64_t text_cap, uint64_t *text_bytes, uint64_t *n_lines,
                              uint64_t *n_reads_kept, cbc_block_result *results)
{
    const pileup_opt pu = { min_alt, edits_per_read, 0u, 0u };
    return decode_window_impl(ctx, in, in_bytes, blocks, n_blocks, caps, window_start, name, name_bytes, beg, end, smax, exclude_flags, &pu,
                              text, text_cap, text_bytes, n_lines, n_reads_kept, results);
}

/* the pileup with a least alternative fraction and the per-strand columns; 0, 0 is the call above */
API int cbc_gpu_decode_pileup_ext(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const cbc_dec_block_desc *blocks,
                                  uint32_t n_blocks, const cbc_lds_caps *caps, const uint64_t *window_start, const char *name,
                                  uint32_t name_bytes, uint64_t beg, uint64_t end, uint32_t smax, uint32_t exclude_flags, uint32_t min_alt,
                                  uint32_t edits_per_read, uint32_t min_alt_ppm, uint32_t by_strand, uint8_t *text, uint64_t text_cap,
                                  uint64_t *text_bytes, uint64_t *n_lines, uint64_t *n_reads_kept, cbc_block_result *results)
{
    const pileup_opt pu = { min_alt, edits_per_read, min_alt_ppm, by_strand };
    return decode_window_impl(ctx, in, in_bytes, blocks, n_blocks, caps, window_start, name, name_bytes, beg, end, smax, exclude_flags, &pu,
                              text, text_cap, text_bytes, n_lines, n_reads_kept, results);
}

/* the consensus record behind the pileup's passes */
API int cbc_gpu_decode_consensus(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const cbc_dec_block_desc *blocks,
                                 uint32_t n_blocks, const cbc_lds_caps *caps, const uint64_t *window_start, const char *name,
                                 uint32_t name_bytes, uint64_t beg, uint64_t end, uint32_t smax, uint32_t exclude_flags,
                                 uint32_t edits_per_read, const cbc_consensus_opts *opts, uint32_t with_range, uint8_t *text,
                                 uint64_t text_cap, uint64_t *text_bytes, cbc_consensus_counts *counts, uint64_t *n_reads_kept,
                                 cbc_block_result *results)
{
    if (!opts || !counts) return CBC_E_ARG;
    memset(counts, 0, sizeof *counts);
    const pileup_opt pu = { 1u, edits_per_read, 0u, 0u };
    const consensus_opt co = { opts, with_range, counts };
    uint64_t n_lines = 0;
    return decode_window_impl(ctx, in, in_bytes, blocks, n_blocks, caps, window_start, name, name_bytes, beg, end, smax, exclude_flags, &pu,
                              text, text_cap, text_bytes, &n_lines, n_reads_kept, results, &co);
}

/* cbc_gpu_decode_blocks_span with the edits reported too: the decoder the pileup runs, with everything it leaves returned */
API int cbc_gpu_decode_blocks_edits(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, cbc_dec_block_desc *blocks,
                                    uint32_t n_blocks, const cbc_lds_caps *caps, uint32_t smax, uint32_t edits_per_read,
                                    cbc_read_rec *recs, uint64_t n_recs, uint8_t *seq, uint64_t seq_bytes, uint32_t *side,
                                    uint16_t *arena, cbc_block_result *results)
{
    if (!ctx || !in || !blocks || !caps || !recs || !seq || !side || !arena || smax == 0) return CBC_E_ARG;
    if (check_edits(ctx, "", &edits_per_read)) return CBC_E_ARG;
    post_req rg;
    memset(&rg, 0, sizeof rg);
    rg.kind = POST_NONE; rg.smax = smax; rg.edits_per_read = edits_per_read; rg.edit_side = side; rg.edit_arena = arena;
    return decode_blocks_impl(ctx, in, in_bytes, blocks, n_blocks, caps, recs, n_recs, seq, seq_bytes, NULL, NULL, NULL, 0, NULL, results, &rg);
}

/* deletion-aware coverage: a setting of the context, read by every depth kind but the pileup when its
 * request is made (decode_window_impl, decode_targets_impl) */
API int cbc_gpu_set_depth_skip_deletions(cbc_gpu_ctx *ctx, uint32_t edits_per_read)
{
    if (!ctx) return CBC_E_ARG;
    if (edits_per_read > CBC_EDITS_MAX) return layout_err(ctx, "skip_deletions wants ", "edits_per_read in 1..510 (0: off)");
    ctx->skipdel_edits = edits_per_read;
    return CBC_OK;
}

/* a set of regions: the selected blocks laid out afresh as for a region decode, the tables checked
 * on the host, then span decode + keep by the interval table + scan + text on the device (cbc_targets_body.h) */
/* cov != NULL (cbc_gpu_decode_coverage) or hist != NULL (cbc_gpu_decode_depth_hist): a depth call whose compressed
 * coordinate is laid over the intervals [iv_first, iv_first + iv_count) -- the contig's, whether a block reaches them or
 * not -- and that ends in the query passes or in the bins */
static int decode_targets_impl(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const cbc_dec_block_desc *blocks,
                               uint32_t n_blocks, const cbc_lds_caps *caps, const uint64_t *window_start,
                               const uint32_t *block_contig, const char *names, uint32_t names_bytes,
                               const uint32_t *contig_name_off, uint32_t n_contigs, const cbc_gpu_targets *t, uint32_t output,
                               uint32_t exclude_flags, uint8_t *text, uint64_t text_cap, uint64_t *text_bytes, uint64_t *n_reads,
                               uint64_t *n_runs, cbc_block_result *results, const cov_req *cov, uint32_t iv_first, uint32_t iv_count,
                               const hist_req *hist = NULL)
{
    const bool whole = cov || hist;                            /* the compressed coordinate over all the contig's intervals */
    if (!ctx || !blocks || !caps || !window_start || !block_contig || !names || !contig_name_off || !t || !text_bytes || !n_reads ||
        !n_runs || (text_cap && !text) || output > CBC_TARGETS_DEPTH) return CBC_E_ARG;
    *text_bytes = 0; *n_reads = 0; *n_runs = 0;
    int rc = call_ready(ctx, n_blocks, in && t->iv && t->block_iv);
    if (rc <= 0) return rc;
    if (t->smax == 0 || t->n_iv == 0 || t->n_iv > (1u << 24))
        return set_err(ctx, CBC_E_ARG, "targets decode wants smax > 0 and 1 .. 2^24 intervals", hipSuccess);
    const bool depth = output == CBC_TARGETS_DEPTH, sam = output == CBC_TARGETS_SAM;
    if ((rc = check_intervals(ctx, "targets decode", t))) return rc;
    const name_tables nt = { window_start, block_contig, names, names_bytes, contig_name_off, n_contigs };
    block_layout L;
    rc = relayout_blocks(ctx, "targets decode", in_bytes, blocks, n_blocks, &nt, &L);
    if (rc) return rc;
    uint32_t *biv = NULL, *ioff = NULL;
    uint32_t lo = UINT32_MAX, hi = 0;                           /* depth: the intervals the call's blocks reach */
    const uint32_t stride = blocks[0].seq_stride;
    const char *bad = NULL;                                     /* a defect found below: its message, then out */
    post_req rg;
    for (uint32_t b = 0; b < n_blocks; b++) {
        const uint32_t f = t->block_iv[2 * b], c = t->block_iv[2 * b + 1];
        if ((rc = check_block_iv(ctx, "targets decode", t, b, NULL))) goto out;
        if (depth && block_contig[b] != block_contig[0]) { bad = "targets decode: a depth call takes the blocks of one contig"; goto out; }
        if (whole && c && (f < iv_first || f - iv_first > iv_count || c > iv_count - (f - iv_first))) {
            bad = "coverage: a block's interval range lies outside the contig's intervals"; goto out; }
        if (c) { if (f < lo) lo = f; if (f + c > hi) hi = f + c; }
    }
    if (depth && L.nrec > 0x3fffffffull) { bad = "targets decode: more than 2^30 - 1 reads in one depth call"; goto out; }
    if (!L.nrec || (depth && lo >= hi)) goto out;               /* no read, or none that reaches an interval: CBC_OK */
    post_req_init(&rg, cov ? (cov->n_quant ? POST_COVQ : cov->ext ? POST_COVX : POST_COV) : hist ? POST_HIST : depth ? POST_TG_DEPTH : sam ? POST_TG_SAM : POST_TG_READS, t->smax,
                  window_start, text, text_cap, sam ? L.nrec * (35ull + stride) + L.name_sum : L.nrec * (stride + 1ull), text_bytes, n_reads);
    rg.beg = 1u; rg.end = UINT64_MAX;
    rg.names = (const uint8_t *)names; rg.names_bytes = names_bytes; rg.block_name = sam ? L.bn : NULL;
    rg.iv = t->iv; rg.n_iv = t->n_iv; rg.block_iv = t->block_iv;
    if (depth) {
        /* the contig's intervals [lo, hi): disjoint, ascending and not touching (they are merged); block ranges relative to
         * lo; the slots of the compressed coordinate, one spare behind each interval */
        if (whole) { lo = iv_first; hi = iv_first + iv_count; }          /* the slots of the queries count from the contig's first interval */
        const uint32_t n = hi - lo, nl0 = L.bn[1];
        biv = (uint32_t *)malloc((size_t)n_blocks * 8);
        ioff = (uint32_t *)malloc(((size_t)n + 1) * 4);
        if (!biv || !ioff) { rc = CBC_E_NOMEM; goto out; }
        uint64_t run = 0;
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t *p = t->iv + 2 * (size_t)(lo + i);
            if (i && p[0] <= p[-1] + 1u) { bad = "targets decode: the intervals of a depth call are not ascending and apart"; goto out; }
            ioff[i] = (uint32_t)run;
            run += (uint64_t)(p[1] - p[0]) + 2u;
        }
        ioff[n] = (uint32_t)run;                                /* <= 2^31 + 2^24 */
        for (uint32_t i = 0; cov && i < cov->n_q; i++)          /* no query reaches past the slots */
            if (cov->q[2 * i] > ioff[n] || cov->q[2 * i + 1] > ioff[n] - cov->q[2 * i]) {
                bad = "coverage: a query lies outside the compressed coordinate"; goto out; }
        for (uint32_t b = 0; b < n_blocks; b++) {
            const uint32_t c = t->block_iv[2 * b + 1];
            biv[2 * b] = c ? t->block_iv[2 * b] - lo : 0u; biv[2 * b + 1] = c;
        }
        rg.iv = t->iv + 2 * (size_t)lo; rg.n_iv = n; rg.block_iv = biv; rg.iv_off = ioff;
        rg.names = (const uint8_t *)names + L.bn[0]; rg.names_bytes = nl0; rg.exclude = exclude_flags; rg.n_runs = n_runs;
        if (cov) rg.cov = *cov;
        if (hist) rg.hist = *hist;
        uint64_t need = (2u * L.nrec + 2ull * n - 1u) * (nl0 + 34ull);   /* K reads, n intervals: at most 2K + 2n - 1 runs */
        if (ctx->skipdel_edits) {                               /* cbc_gpu_set_depth_skip_deletions: every depth kind of a target set */
            /* a run per position of the intervals at most, and per reference base a read spans (cbc_unpack_targets_depth_skipdel_cap) */
            const uint64_t w = run - n, by_reads = L.nrec * t->smax;
            need = (w < by_reads ? w : by_reads) * (nl0 + 34ull);
            rg.skip_del = true; rg.edits_per_read = ctx->skipdel_edits;
        }
        rg.text_cap = text_cap < need ? text_cap : need;
    }
    rc = decode_laid_out(ctx, in, &L, n_blocks, caps, results, &rg);
out:
    if (bad) rc = set_err(ctx, CBC_E_ARG, bad, hipSuccess);
    layout_free(&L); free(biv); free(ioff);
    return rc;
}

API int cbc_gpu_decode_targets(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const cbc_dec_block_desc *blocks,
                               uint32_t n_blocks, const cbc_lds_caps *caps, const uint64_t *window_start,
                               const uint32_t *block_contig, const char *names, uint32_t names_bytes,
                               const uint32_t *contig_name_off, uint32_t n_contigs, const cbc_gpu_targets *t, uint32_t output,
                               uint32_t exclude_flags, uint8_t *text, uint64_t text_cap, uint64_t *text_bytes, uint64_t *n_reads,
                               uint64_t *n_runs, cbc_block_result *results)
{
    return decode_targets_impl(ctx, in, in_bytes, blocks, n_blocks, caps, window_start, block_contig, names, names_bytes, contig_name_off,
                               n_contigs, t, output, exclude_flags, text, text_cap, text_bytes, n_reads, n_runs, results, NULL, 0u, 0u);
}

/* per-query coverage summary: the depth form of cbc_gpu_decode_targets up to the change points, then
 * the weights, their scans, the prefixes and the lookup (cbc_cov_body.h); only the numbers come back */
API int cbc_gpu_decode_coverage(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const cbc_dec_block_desc *blocks,
                                uint32_t n_blocks, const cbc_lds_caps *caps, const uint64_t *window_start,
                                const uint32_t *block_contig, const char *names, uint32_t names_bytes,
                                const uint32_t *contig_name_off, uint32_t n_contigs, const cbc_gpu_targets *t,
                                uint32_t iv_first, uint32_t iv_count, const uint32_t *q, uint32_t n_q, uint32_t exclude_flags,
                                uint32_t min_depth, uint64_t *sum, uint32_t *covered, uint64_t *n_reads, cbc_block_result *results)
{
    if (!ctx || !t || !n_reads || (n_q && (!q || !sum || !covered))) return CBC_E_ARG;
    *n_reads = 0;
    if (n_q) { memset(sum, 0, (size_t)n_q * 8); memset(covered, 0, (size_t)n_q * 4); }
    if (min_depth < 1 || n_q > (1u << 24) || iv_count < 1 || iv_first > t->n_iv || iv_count > t->n_iv - iv_first)
        return set_err(ctx, CBC_E_ARG, "coverage wants min_depth >= 1, at most 2^24 queries and the contig's intervals inside the table", hipSuccess);
    if (n_q == 0) return CBC_OK;
    const cov_req cq = { q, n_q, min_depth, sum, covered, false, NULL, 0u, NULL, NULL, NULL, 0u, NULL };
    uint64_t text_bytes = 0, n_runs = 0;
    return decode_targets_impl(ctx, in, in_bytes, blocks, n_blocks, caps, window_start, block_contig, names, names_bytes, contig_name_off,
                               n_contigs, t, CBC_TARGETS_DEPTH, exclude_flags, NULL, 0, &text_bytes, n_reads, &n_runs, results, &cq,
                               iv_first, iv_count);
}

/* read counts and depth thresholds per query: cbc_gpu_decode_coverage with the mark pass that notes
 * the pieces' first slots, then the start points, the thresholds' weights, scans and prefixes and one lookup (cbc_covx_body.h);
 * with n_quant != 0 the depth quantiles per query behind them: one wavefront per query selects them
 * from the change points (cbc_quant_body.h) */
static int decode_coverage_ext_impl(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const cbc_dec_block_desc *blocks,
                                    uint32_t n_blocks, const cbc_lds_caps *caps, const uint64_t *window_start,
                                    const uint32_t *block_contig, const char *names, uint32_t names_bytes,
                                    const uint32_t *contig_name_off, uint32_t n_contigs, const cbc_gpu_targets *t,
                                    uint32_t iv_first, uint32_t iv_count, const uint32_t *q, uint32_t n_q, uint32_t exclude_flags,
                                    uint32_t min_depth, uint64_t *sum, uint32_t *covered, uint64_t *n_reads, cbc_block_result *results,
                                    const uint32_t *thresholds, uint32_t n_thr, uint32_t *thr_covered, uint32_t *reads,
                                    const uint32_t *quantiles, uint32_t n_quant, uint32_t *quant_depth)
{
    if (!ctx || !t || !n_reads || (n_q && (!q || !sum || !covered)) || (n_thr && !thresholds) || (n_q && n_thr && !thr_covered) ||
        (n_quant && (!quantiles || (n_q && !quant_depth)))) return CBC_E_ARG;
    *n_reads = 0;
    if (n_q) { memset(sum, 0, (size_t)n_q * 8); memset(covered, 0, (size_t)n_q * 4); }
    if (n_q <= (1u << 24) && n_thr <= CBC_COVX_MAX_THR && n_quant <= CBC_QUANT_MAX) {
        if (n_thr) memset(thr_covered, 0, (size_t)n_q * n_thr * 4);
        if (reads) memset(reads, 0, (size_t)n_q * 4);
        if (n_quant && n_q) memset(quant_depth, 0, (size_t)n_q * n_quant * 4);
    }
    if (min_depth < 1 || n_q > (1u << 24) || iv_count < 1 || iv_first > t->n_iv || iv_count > t->n_iv - iv_first)
        return set_err(ctx, CBC_E_ARG, "coverage wants min_depth >= 1, at most 2^24 queries and the contig's intervals inside the table", hipSuccess);
    bool asc = n_thr <= CBC_COVX_MAX_THR;
    for (uint32_t i = 0; asc && i < n_thr; i++) asc = thresholds[i] >= 1u && (i == 0 || thresholds[i] > thresholds[i - 1]);
    if (!asc) return set_err(ctx, CBC_E_ARG, "coverage wants at most 8 thresholds, each >= 1 and strictly ascending", hipSuccess);
    asc = n_quant <= CBC_QUANT_MAX;
    for (uint32_t i = 0; asc && i < n_quant; i++) asc = quantiles[i] <= 100u && (i == 0 || quantiles[i] > quantiles[i - 1]);
    if (!asc) return set_err(ctx, CBC_E_ARG, "coverage wants 1 to 8 quantiles, percentages in 0..100 and strictly ascending", hipSuccess);
    if (n_q == 0) return CBC_OK;
    const cov_req cq = { q, n_q, min_depth, sum, covered, true, thresholds, n_thr, thr_covered, reads, quantiles, n_quant, quant_depth };
    uint64_t text_bytes = 0, n_runs = 0;
    const int rc = decode_targets_impl(ctx, in, in_bytes, blocks, n_blocks, caps, window_start, block_contig, names, names_bytes,
                                       contig_name_off, n_contigs, t, CBC_TARGETS_DEPTH, exclude_flags, NULL, 0, &text_bytes, n_reads, &n_runs,
                                       results, &cq, iv_first, iv_count);
    if (rc == CBC_E_BLOCK) {                                   /* a failed block: no numbers */
        memset(sum, 0, (size_t)n_q * 8); memset(covered, 0, (size_t)n_q * 4);
        if (n_thr) memset(thr_covered, 0, (size_t)n_q * n_thr * 4);
        if (reads) memset(reads, 0, (size_t)n_q * 4);
        if (n_quant) memset(quant_depth, 0, (size_t)n_q * n_quant * 4);
    }
    return rc;
}

API int cbc_gpu_decode_coverage_ext(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const cbc_dec_block_desc *blocks,
                                    uint32_t n_blocks, const cbc_lds_caps *caps, const uint64_t *window_start,
                                    const uint32_t *block_contig, const char *names, uint32_t names_bytes,
                                    const uint32_t *contig_name_off, uint32_t n_contigs, const cbc_gpu_targets *t,
                                    uint32_t iv_first, uint32_t iv_count, const uint32_t *q, uint32_t n_q, uint32_t exclude_flags,
                                    uint32_t min_depth, uint64_t *sum, uint32_t *covered, uint64_t *n_reads, cbc_block_result *results,
                                    const uint32_t *thresholds, uint32_t n_thr, uint32_t *thr_covered, uint32_t *reads)
{
    return decode_coverage_ext_impl(ctx, in, in_bytes, blocks, n_blocks, caps, window_start, block_contig, names, names_bytes, contig_name_off,
                                   n_contigs, t, iv_first, iv_count, q, n_q, exclude_flags, min_depth, sum, covered, n_reads, results, thresholds,
                                   n_thr, thr_covered, reads, NULL, 0u, NULL);
}

/* depth quantiles per query; n_quant == 0: the call above */
API int cbc_gpu_decode_coverage_quant(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const cbc_dec_block_desc *blocks,
                                      uint32_t n_blocks, const cbc_lds_caps *caps, const uint64_t *window_start,
                                      const uint32_t *block_contig, const char *names, uint32_t names_bytes,
                                      const uint32_t *contig_name_off, uint32_t n_contigs, const cbc_gpu_targets *t,
                                      uint32_t iv_first, uint32_t iv_count, const uint32_t *q, uint32_t n_q, uint32_t exclude_flags,
                                      uint32_t min_depth, uint64_t *sum, uint32_t *covered, uint64_t *n_reads, cbc_block_result *results,
                                      const uint32_t *thresholds, uint32_t n_thr, uint32_t *thr_covered, uint32_t *reads,
                                      const uint32_t *quantiles, uint32_t n_quant, uint32_t *quant_depth)
{
    return decode_coverage_ext_impl(ctx, in, in_bytes, blocks, n_blocks, caps, window_start, block_contig, names, names_bytes, contig_name_off,
                                   n_contigs, t, iv_first, iv_count, q, n_q, exclude_flags, min_depth, sum, covered, n_reads, results, thresholds,
                                   n_thr, thr_covered, reads, quantiles, n_quant, quant_depth);
}

/* depth histogram: the depth form of cbc_gpu_decode_targets up to the change points, laid over all the
 * contig's intervals as for the coverage summary, then zero + accumulate and the compaction of the bins (cbc_hist_body.h); only
 * the non-zero bins come back */
API int cbc_gpu_decode_depth_hist(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const cbc_dec_block_desc *blocks,
                                  uint32_t n_blocks, const cbc_lds_caps *caps, const uint64_t *window_start,
                                  const uint32_t *block_contig, const char *names, uint32_t names_bytes,
                                  const uint32_t *contig_name_off, uint32_t n_contigs, const cbc_gpu_targets *t,
                                  uint32_t iv_first, uint32_t iv_count, uint32_t exclude_flags, uint32_t max_depth,
                                  uint32_t *bin_depth, uint32_t *bin_bases, uint32_t bin_cap, uint32_t *n_bins, uint64_t *n_reads,
                                  cbc_block_result *results)
{
    if (!ctx || !t || !n_reads || !n_bins || (bin_cap && (!bin_depth || !bin_bases))) return CBC_E_ARG;
    *n_reads = 0; *n_bins = 0;
    if (iv_count < 1 || iv_first > t->n_iv || iv_count > t->n_iv - iv_first)
        return set_err(ctx, CBC_E_ARG, "depth histogram wants the contig's intervals inside the table", hipSuccess);
    const hist_req hq = { max_depth ? max_depth : 0xffffffffu, bin_depth, bin_bases, bin_cap, n_bins };
    uint64_t text_bytes = 0, n_runs = 0;
    return decode_targets_impl(ctx, in, in_bytes, blocks, n_blocks, caps, window_start, block_contig, names, names_bytes, contig_name_off,
                               n_contigs, t, CBC_TARGETS_DEPTH, exclude_flags, NULL, 0, &text_bytes, n_reads, &n_runs, results, NULL,
                               iv_first, iv_count, &hq);
}

/* read statistics: the blocks laid out afresh as for a region decode, the plain decode (t == NULL) or the
 * span decode and the keep rule of a target set, then one pass over the records and rows (cbc_stats_body.h); only the tables
 * come back.  aln != NULL: with the alignment tables -- the edits decoder (smax, edits_per_read), and the
 * alignment pass (cbc_stats_aln_body.h) behind the statistics pass; both tables come back in the one small-results fetch, and
 * both are zero after any refusal or failure. */
static int decode_stats_impl(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const cbc_dec_block_desc *blocks,
                             uint32_t n_blocks, const cbc_lds_caps *caps, const uint64_t *window_start, const cbc_gpu_targets *t,
                             uint32_t smax, uint32_t exclude_flags, uint32_t edits_per_read, cbc_gpu_stats *out, cbc_gpu_stats_aln *aln,
                             cbc_block_result *results)
{
    if (!ctx || !out) return CBC_E_ARG;
    memset(out, 0, sizeof *out);
    if (aln) memset(aln, 0, sizeof *aln);
    if (!blocks || !caps || !window_start) return CBC_E_ARG;
    int rc = call_ready(ctx, n_blocks, in && (!t || (t->iv && t->block_iv)));
    if (rc <= 0) return rc;
    if (t && (t->smax == 0 || t->n_iv == 0 || t->n_iv > (1u << 24)))
        return set_err(ctx, CBC_E_ARG, "statistics of a target set want smax > 0 and 1 .. 2^24 intervals", hipSuccess);
    if (aln) {
        if (!t && smax == 0) return set_err(ctx, CBC_E_ARG, "statistics with alignment tables want smax > 0 (the container's span bound)", hipSuccess);
        if ((rc = check_edits(ctx, "statistics with alignment tables want ", &edits_per_read))) return rc;
    }
    if (t && (rc = check_intervals(ctx, "statistics", t))) return rc;
    uint32_t most = 0;
    for (uint32_t b = 0; b < n_blocks; b++) {
        if (blocks[b].n_reads > most) most = blocks[b].n_reads;
        if (t && (rc = check_block_iv(ctx, "statistics", t, b, window_start))) return rc;
    }
    /* the bound on a workgroup's run-length counts (cbc_stats_aln_body.h) */
    if (aln && (uint64_t)n_blocks * ((most + 63u) / 64u) > CBC_SALN_MAX_UNITS)
        return set_err(ctx, CBC_E_ARG, "statistics with alignment tables: blocks x record groups of the largest block pass 2^29", hipSuccess);
    block_layout L;
    rc = relayout_blocks(ctx, "statistics", in_bytes, blocks, n_blocks, NULL, &L);
    if (rc) return rc;
    if (L.nrec > 0xffffffffull) { layout_free(&L); return set_err(ctx, CBC_E_ARG, "statistics: more than 2^32 - 1 reads in one call", hipSuccess); }
    if (L.nrec) {
        uint64_t text_bytes = 0, n_sel = 0;
        post_req rg;
        post_req_init(&rg, aln ? (t ? POST_TG_STATS_ALN : POST_STATS_ALN) : (t ? POST_TG_STATS : POST_STATS), t ? t->smax : aln ? smax : 0u,
                      window_start, NULL, 0, 0, &text_bytes, &n_sel);
        rg.beg = 1u; rg.end = UINT64_MAX;
        if (t) { rg.iv = t->iv; rg.n_iv = t->n_iv; rg.block_iv = t->block_iv; }
        rg.exclude = exclude_flags; rg.stats = out; rg.stats_gmax = (most + 63u) / 64u;
        if (aln) { rg.stats_aln = aln; rg.edits_per_read = edits_per_read; }
        rc = decode_laid_out(ctx, in, &L, n_blocks, caps, results, &rg);
        if (rc && aln) { memset(out, 0, sizeof *out); memset(aln, 0, sizeof *aln); }
    }
    layout_free(&L);
    return rc;
}

API int cbc_gpu_decode_stats(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const cbc_dec_block_desc *blocks,
                             uint32_t n_blocks, const cbc_lds_caps *caps, const uint64_t *window_start, const cbc_gpu_targets *t,
                             uint32_t exclude_flags, cbc_gpu_stats *out, cbc_block_result *results)
{
    return decode_stats_impl(ctx, in, in_bytes, blocks, n_blocks, caps, window_start, t, 0u, exclude_flags, 0u, out, NULL, results);
}

API int cbc_gpu_decode_stats_aln(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const cbc_dec_block_desc *blocks,
                                 uint32_t n_blocks, const cbc_lds_caps *caps, const uint64_t *window_start, const cbc_gpu_targets *t,
                                 uint32_t smax, uint32_t exclude_flags, uint32_t edits_per_read, cbc_gpu_stats *out,
                                 cbc_gpu_stats_aln *aln, cbc_block_result *results)
{
    if (!aln) return CBC_E_ARG;
    return decode_stats_impl(ctx, in, in_bytes, blocks, n_blocks, caps, window_start, t, smax, exclude_flags, edits_per_read, out, aln, results);
}

/* Kernel times of the most recent call, per entry point (last_ms): the kinds it answers for and the stretches it reports.  A
 * NULL out-pointer is CBC_E_ARG before anything waits. */
#define LAST_MS(kinds, ...) do { float *const out[] = { __VA_ARGS__ }; \
                                 return last_ms(ctx, LAST_IS(kinds), out, (int)(sizeof out / sizeof out[0])); } while (0)

API int cbc_gpu_last_region_ms(cbc_gpu_ctx *ctx, float *decode_ms, float *filter_ms, float *text_ms)
{ LAST_MS(ctx->last_post == POST_REGION, decode_ms, filter_ms, text_ms); }

API int cbc_gpu_last_sam_ms(cbc_gpu_ctx *ctx, float *decode_ms, float *count_ms, float *text_ms)
{ LAST_MS(ctx->last_post == POST_SAM, decode_ms, count_ms, text_ms); }

API int cbc_gpu_last_sam_cigar_ms(cbc_gpu_ctx *ctx, float *decode_ms, float *measure_ms, float *count_ms, float *text_ms)
{ LAST_MS(ctx->last_post == POST_SAM_CIGAR, decode_ms, measure_ms, count_ms, text_ms); }

API int cbc_gpu_last_depth_ms(cbc_gpu_ctx *ctx, float *decode_ms, float *mark_ms, float *scan_ms, float *text_ms)
{ LAST_MS(ctx->last_post == POST_DEPTH, decode_ms, mark_ms, scan_ms, text_ms); }

API int cbc_gpu_last_pileup_ms(cbc_gpu_ctx *ctx, float *decode_ms, float *events_ms, float *scan_ms, float *text_ms)
{ LAST_MS(ctx->last_post == POST_PILEUP, decode_ms, events_ms, scan_ms, text_ms); }
API int cbc_gpu_last_consensus_ms(cbc_gpu_ctx *ctx, float *decode_ms, float *events_ms, float *scan_ms, float *text_ms)
{ LAST_MS(ctx->last_post == POST_CONSENSUS, decode_ms, events_ms, scan_ms, text_ms); }

/* not after a call with the alignment tables: that one has a third stretch, and an entry point of its own */
API int cbc_gpu_last_stats_ms(cbc_gpu_ctx *ctx, float *decode_ms, float *stats_ms)
{ LAST_MS(post_is_stats(ctx->last_post) && !post_is_stats_aln(ctx->last_post), decode_ms, stats_ms); }

API int cbc_gpu_last_stats_aln_ms(cbc_gpu_ctx *ctx, float *decode_ms, float *stats_ms, float *aln_ms)
{ LAST_MS(post_is_stats_aln(ctx->last_post), decode_ms, stats_ms, aln_ms); }

API int cbc_gpu_last_hist_ms(cbc_gpu_ctx *ctx, float *decode_ms, float *mark_ms, float *scan_ms, float *accum_ms, float *compact_ms)
{ LAST_MS(ctx->last_post == POST_HIST, decode_ms, mark_ms, scan_ms, accum_ms, compact_ms); }

API int cbc_gpu_last_coverage_ms(cbc_gpu_ctx *ctx, float *decode_ms, float *mark_ms, float *scan_ms, float *weights_ms,
                                 float *wscan_ms, float *apply_ms, float *lookup_ms)
{ LAST_MS(ctx->last_post == POST_COV, decode_ms, mark_ms, scan_ms, weights_ms, wscan_ms, apply_ms, lookup_ms); }

/* cov_ms[7] as cbc_gpu_last_coverage_ms gives them (the mark is the one that also notes the starts), ext_ms[5] the added
 * passes, and after a call with quantiles quant_ms[1], the selection */
static int last_coverage_ext_ms(cbc_gpu_ctx *ctx, post_kind kind, float *cov_ms, float *ext_ms, float *quant_ms)
{
    if (!cov_ms || !ext_ms) return CBC_E_ARG;
    float *out[13];
    for (int i = 0; i < 7; i++) out[i] = cov_ms + i;
    for (int i = 0; i < 5; i++) out[7 + i] = ext_ms + i;
    out[12] = quant_ms;
    return last_ms(ctx, LAST_IS(ctx->last_post == kind), out, kind == POST_COVQ ? 13 : 12);
}

API int cbc_gpu_last_coverage_ext_ms(cbc_gpu_ctx *ctx, float *cov_ms, float *ext_ms)
{
    return last_coverage_ext_ms(ctx, POST_COVX, cov_ms, ext_ms, NULL);
}

API int cbc_gpu_last_coverage_quant_ms(cbc_gpu_ctx *ctx, float *cov_ms, float *ext_ms, float *quant_ms)
{
    return last_coverage_ext_ms(ctx, POST_COVQ, cov_ms, ext_ms, quant_ms);
}

/* a reads / SAM call has no scan stretch of its own: scan_ms = 0 */
API int cbc_gpu_last_targets_ms(cbc_gpu_ctx *ctx, float *decode_ms, float *filter_ms, float *scan_ms, float *text_ms)
{
    if (!ctx || !decode_ms || !filter_ms || !scan_ms || !text_ms) return CBC_E_ARG;
    if (ctx->last_post == POST_TG_DEPTH) LAST_MS(true, decode_ms, filter_ms, scan_ms, text_ms);
    if (ctx->last_post != POST_TG_READS && ctx->last_post != POST_TG_SAM) return CBC_E_ARG;
    *scan_ms = 0.0f;
    LAST_MS(true, decode_ms, filter_ms, text_ms);
}

/* ------------------------------------------------------------------------------------------------
 * whole-file stream ("compat" mode) and the general-form fallback over blocks
 * ---------------------------------------------------------------------------------------------- */
API uint32_t cbc_stream_read_length(const uint8_t *in, uint64_t in_bytes)
{
    /* the header's first int goes through four untouched 256-symbol models: its bytes come out verbatim */
    if (!in || in_bytes < 4) return 0;
    return ((uint32_t)in[0] << 24) | ((uint32_t)in[1] << 16) | ((uint32_t)in[2] << 8) | in[3];
}

static int stream_encode(cbc_gpu_ctx *ctx, const cbc_host_batch *hb, int per_segment, uint8_t *out, uint64_t out_cap,
                         uint64_t *out_offsets, cbc_block_result *results, cbc_stream_result *sres)
{
    if (!ctx || !hb || !out) return CBC_E_ARG;
    if (!ctx->d_ref) return set_err(ctx, CBC_E_ARG, "cbc_gpu_upload_reference has not been called", hipSuccess);
    const uint32_t nb = hb->n_blocks;
    if (nb == 0) return set_err(ctx, CBC_E_ARG, "no records", hipSuccess);
    HIPCHK(hipSetDevice(ctx->device), "hipSetDevice");
    const uint32_t n_streams = per_segment ? nb : 1u;
    cbc_block_desc *segs = (cbc_block_desc *)malloc((size_t)nb * sizeof(cbc_block_desc));
    cbc_block_result *res = (cbc_block_result *)malloc((size_t)n_streams * sizeof(cbc_block_result));
    if (!segs || !res) { free(segs); free(res); return CBC_E_NOMEM; }
    memcpy(segs, hb->blocks, (size_t)nb * sizeof(cbc_block_desc));
    /* output areas: < 20 bits per coded symbol; symbols per record <= 17 + 2 per edit (cf. cbc_plan_output) */
    uint64_t scratch = 0;
    {
        uint64_t whole = 4096;
        for (uint32_t b = 0; b < nb; b++) {
            uint64_t cap = (4096 + 48ull * segs[b].n_reads + 8ull * segs[b].n_tok + 255) & ~255ull;
            if (per_segment) {
                if (cap > 0xffffff00ull) cap = 0xffffff00ull;
                segs[b].out_off = scratch; segs[b].out_cap = (uint32_t)cap; scratch += cap;
            } else whole += cap;
        }
        if (!per_segment) {
            if (whole > 0xffffff00ull) whole = 0xffffff00ull;
            whole &= ~255ull;
            for (uint32_t b = 0; b < nb; b++) { segs[b].out_off = 0; segs[b].out_cap = (uint32_t)whole; }
            scratch = whole;
        }
    }
    cbc_stream_caps caps; caps.cap_pos = hb->caps.cap_pos < 64 ? 64 : hb->caps.cap_pos; caps.cap_name = hb->names_bytes + 2u * (per_segment ? 1u : nb) + 16u;
    const uint32_t lds = cbc_stream_lds_bytes(&caps);
    int rc = CBC_OK;
    void *d_recs = NULL, *d_seq = NULL, *d_tok = NULL, *d_names = NULL, *d_segs = NULL, *d_out = NULL, *d_res = NULL, *d_vtab = NULL, *d_aux = NULL;
    const uint64_t ntok = hb->n_tok ? hb->n_tok : 1;
    uint32_t grid = n_streams < 32u ? n_streams : 32u;            /* pool of var tables: 67 MB each */
    if (caps.cap_pos > CBC_STREAM_POS_MAX) { free(segs); free(res); return set_err(ctx, CBC_E_ARG, "cap_pos beyond MAX_ALPHA", hipSuccess); }
    if (lds > 160u * 1024u) { free(segs); free(res); return set_err(ctx, CBC_E_ARG, "stream tables need more than 160 KiB of LDS", hipSuccess); }
    GO(hipMalloc(&d_recs, hb->n_recs * sizeof(cbc_read_rec) + 16), "hipMalloc recs");
    GO(hipMalloc(&d_seq, hb->seq_bytes + 16), "hipMalloc seq");
    GO(hipMalloc(&d_tok, ntok * 4 + 16), "hipMalloc tok");
    GO(hipMalloc(&d_names, hb->names_bytes + 16), "hipMalloc names");
    GO(hipMalloc(&d_segs, (uint64_t)nb * sizeof(cbc_block_desc)), "hipMalloc segments");
    GO(hipMalloc(&d_out, scratch), "hipMalloc out");
    GO(hipMalloc(&d_res, (uint64_t)n_streams * sizeof(cbc_block_result)), "hipMalloc results");
    GO(hipMalloc(&d_vtab, (uint64_t)grid * CBC_VTAB_WORDS * 4), "hipMalloc var tables");
    GO(hipMemsetAsync(d_vtab, 0, (uint64_t)grid * CBC_VTAB_WORDS * 4, ctx->stream), "memset var tables");
    GO(hipMalloc(&d_aux, (uint64_t)grid * cbc_stream_aux_words(caps.cap_pos) * 4), "hipMalloc flag / pos overflow tables");
    GO(hipMemcpyAsync(d_recs, hb->recs, hb->n_recs * sizeof(cbc_read_rec), hipMemcpyHostToDevice, ctx->stream), "H2D recs");
    GO(hipMemcpyAsync(d_seq, hb->seq, hb->seq_bytes, hipMemcpyHostToDevice, ctx->stream), "H2D seq");
    GO(hipMemcpyAsync(d_tok, hb->tok, hb->n_tok * 4, hipMemcpyHostToDevice, ctx->stream), "H2D tok");
    GO(hipMemcpyAsync(d_names, hb->names, hb->names_bytes, hipMemcpyHostToDevice, ctx->stream), "H2D names");
    GO(hipMemcpyAsync(d_segs, segs, (uint64_t)nb * sizeof(cbc_block_desc), hipMemcpyHostToDevice, ctx->stream), "H2D segments");
    GO(hipMemsetAsync(d_res, 0xff, (uint64_t)n_streams * sizeof(cbc_block_result), ctx->stream), "memset results");
    {
        cbc_stream_args A;
        memset(&A, 0, sizeof A);
        A.recs = (const cbc_read_rec *)d_recs; A.seq = (const uint8_t *)d_seq; A.tok = (const uint32_t *)d_tok;
        A.names = (const uint8_t *)d_names; A.segs = (const cbc_block_desc *)d_segs; A.ref = ctx->d_ref;
        A.out = (uint8_t *)d_out; A.results = (cbc_block_result *)d_res; A.vtab = (uint32_t *)d_vtab; A.aux = (uint32_t *)d_aux;
        A.ref_bytes = ctx->ref_bytes; A.out_bytes = scratch; A.seq_bytes = hb->seq_bytes; A.n_tok = ntok; A.n_recs = hb->n_recs;
        A.n_segs = nb; A.cap_pos = caps.cap_pos; A.cap_name = caps.cap_name; A.names_bytes = hb->names_bytes;
        A.per_segment = per_segment ? 1u : 0u; A.n_vtab = grid;
        GO(hipEventRecord(ctx->ev0, ctx->stream), "hipEventRecord");
        hipLaunchKernelGGL(cbc_encode_whole_kernel, dim3(grid), dim3(64), lds, ctx->stream, A);
        GO(hipGetLastError(), "launch cbc_encode_whole_kernel");
        GO(hipEventRecord(ctx->ev1, ctx->stream), "hipEventRecord");
        ctx->have_timing = 1;
    }
    GO(hipMemcpyAsync(res, d_res, (uint64_t)n_streams * sizeof(cbc_block_result), hipMemcpyDeviceToHost, ctx->stream), "D2H results");
    GO(hipStreamSynchronize(ctx->stream), "stream encode kernel");
    {
        uint64_t off = 0;
        if (out_offsets) out_offsets[0] = 0;
        for (uint32_t s = 0; s < n_streams; s++) {
            if (res[s].status != CBC_ST_OK) {
                if (rc == CBC_OK) { snprintf(ctx->err, sizeof ctx->err, "stream %u failed with status %u at record %u", s, res[s].status, res[s].fail_read); rc = CBC_E_BLOCK; }
                res[s].nbytes = 0;
            }
            if (off + res[s].nbytes > out_cap) { rc = set_err(ctx, CBC_E_ARG, "out_cap too small for the stream", hipSuccess); goto done; }
            if (res[s].nbytes) GO(hipMemcpyAsync(out + off, (uint8_t *)d_out + segs[per_segment ? s : 0].out_off, res[s].nbytes, hipMemcpyDeviceToHost, ctx->stream), "D2H stream");
            off += res[s].nbytes;
            if (out_offsets) out_offsets[s + 1] = off;
            if (results) results[s] = res[s];
        }
        GO(hipStreamSynchronize(ctx->stream), "D2H stream");
        if (sres) { sres->nbytes = off; sres->status = res[0].status; sres->fail_read = res[0].fail_read; sres->n_symbols = res[0].n_symbols; }
    }
done:
    free(segs); free(res);
    if (d_recs) (void)hipFree(d_recs); if (d_seq) (void)hipFree(d_seq); if (d_tok) (void)hipFree(d_tok);
    if (d_names) (void)hipFree(d_names); if (d_segs) (void)hipFree(d_segs); if (d_out) (void)hipFree(d_out);
    if (d_res) (void)hipFree(d_res); if (d_vtab) (void)hipFree(d_vtab); if (d_aux) (void)hipFree(d_aux);
    return rc;
}

API int cbc_gpu_encode_stream(cbc_gpu_ctx *ctx, const cbc_host_batch *hb, uint8_t *out, uint64_t out_cap, cbc_stream_result *result)
{
    return stream_encode(ctx, hb, 0, out, out_cap, NULL, NULL, result);
}
API int cbc_gpu_encode_stream_blocks(cbc_gpu_ctx *ctx, const cbc_host_batch *hb, uint8_t *out, uint64_t out_cap,
                                     uint64_t *out_offsets, cbc_block_result *results)
{
    if (!out_offsets) return CBC_E_ARG;
    return stream_encode(ctx, hb, 1, out, out_cap, out_offsets, results, NULL);
}

API int cbc_gpu_decode_stream(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes,
                              const uint64_t *contig_off, const uint64_t *contig_len, uint32_t n_contigs,
                              cbc_read_rec *recs, uint64_t rec_cap, uint8_t *seq, uint64_t seq_bytes, uint32_t seq_stride,
                              cbc_stream_result *result)
{
    if (!ctx || !in || !contig_off || !contig_len || !recs || !seq || !result || n_contigs == 0) return CBC_E_ARG;
    if (!ctx->d_ref) return set_err(ctx, CBC_E_ARG, "cbc_gpu_upload_reference has not been called", hipSuccess);
    const uint32_t L0 = cbc_stream_read_length(in, in_bytes);
    if (L0 < 1 || L0 > 256 || seq_stride < 4 || seq_stride > 256 || (seq_stride & 3u) || rec_cap == 0 || rec_cap > 0xffffffffull ||
        seq_bytes < rec_cap * seq_stride + 8) return set_err(ctx, CBC_E_ARG, "bad stream header or buffer sizes", hipSuccess);
    HIPCHK(hipSetDevice(ctx->device), "hipSetDevice");
    /* the stream does not say how many distinct POS steps it holds: room for the reference's whole alphabet (MAX_ALPHA),
     * CBC_STREAM_POS_LDS entries of it in LDS, the rest in the aux area (40 MB) */
    cbc_stream_caps caps; caps.cap_pos = CBC_STREAM_POS_MAX; caps.cap_name = 2048;
    const uint32_t lds = cbc_stream_lds_bytes(&caps);
    void *d_in = NULL, *d_co = NULL, *d_cl = NULL, *d_recs = NULL, *d_seq = NULL, *d_res = NULL, *d_vtab = NULL, *d_aux = NULL;
    cbc_block_result res; memset(&res, 0xff, sizeof res);
    int rc = CBC_OK;
    GO(hipMalloc(&d_in, in_bytes + 16), "hipMalloc in");
    GO(hipMalloc(&d_co, (uint64_t)n_contigs * 8), "hipMalloc contigs");
    GO(hipMalloc(&d_cl, (uint64_t)n_contigs * 8), "hipMalloc contigs");
    GO(hipMalloc(&d_recs, rec_cap * sizeof(cbc_read_rec) + 16), "hipMalloc recs");
    GO(hipMalloc(&d_seq, seq_bytes + 16), "hipMalloc seq");
    GO(hipMalloc(&d_res, sizeof(cbc_block_result)), "hipMalloc result");
    GO(hipMalloc(&d_vtab, CBC_VTAB_WORDS * 4), "hipMalloc var table");
    GO(hipMemsetAsync(d_vtab, 0, CBC_VTAB_WORDS * 4, ctx->stream), "memset var table");
    GO(hipMalloc(&d_aux, cbc_stream_aux_words(caps.cap_pos) * 4), "hipMalloc flag / pos overflow tables");
    GO(hipMemsetAsync((uint8_t *)d_in + in_bytes, 0, 16, ctx->stream), "memset pad");
    GO(hipMemcpyAsync(d_in, in, in_bytes, hipMemcpyHostToDevice, ctx->stream), "H2D stream");
    GO(hipMemcpyAsync(d_co, contig_off, (uint64_t)n_contigs * 8, hipMemcpyHostToDevice, ctx->stream), "H2D contigs");
    GO(hipMemcpyAsync(d_cl, contig_len, (uint64_t)n_contigs * 8, hipMemcpyHostToDevice, ctx->stream), "H2D contigs");
    GO(hipMemsetAsync(d_res, 0xff, sizeof(cbc_block_result), ctx->stream), "memset result");
    {
        cbc_dstream_args A;
        memset(&A, 0, sizeof A);
        A.in = (const uint8_t *)d_in; A.ref = ctx->d_ref; A.contig_off = (const uint64_t *)d_co; A.contig_len = (const uint64_t *)d_cl;
        A.recs = (cbc_read_rec *)d_recs; A.seq = (uint8_t *)d_seq; A.results = (cbc_block_result *)d_res; A.vtab = (uint32_t *)d_vtab;
        A.aux = (uint32_t *)d_aux;
        A.in_bytes = in_bytes; A.ref_bytes = ctx->ref_bytes; A.rec_cap = rec_cap; A.seq_bytes = seq_bytes + 16;
        A.n_contigs = n_contigs; A.cap_pos = caps.cap_pos; A.cap_name = caps.cap_name; A.seq_stride = seq_stride; A.read_length = L0;
        GO(hipEventRecord(ctx->ev0, ctx->stream), "hipEventRecord");
        hipLaunchKernelGGL(cbc_decode_whole_kernel, dim3(1), dim3(64), lds, ctx->stream, A);
        GO(hipGetLastError(), "launch cbc_decode_whole_kernel");
        GO(hipEventRecord(ctx->ev1, ctx->stream), "hipEventRecord");
        ctx->have_timing = 1;
    }
    GO(hipMemcpyAsync(&res, d_res, sizeof res, hipMemcpyDeviceToHost, ctx->stream), "D2H result");
    GO(hipStreamSynchronize(ctx->stream), "stream decode kernel");
    result->nbytes = res.nbytes; result->status = res.status; result->fail_read = res.fail_read; result->n_symbols = res.n_symbols;
    if (res.nbytes <= rec_cap && res.nbytes) {
        GO(hipMemcpyAsync(recs, d_recs, (uint64_t)res.nbytes * sizeof(cbc_read_rec), hipMemcpyDeviceToHost, ctx->stream), "D2H recs");
        GO(hipMemcpyAsync(seq, d_seq, (uint64_t)res.nbytes * seq_stride, hipMemcpyDeviceToHost, ctx->stream), "D2H seq");
        GO(hipStreamSynchronize(ctx->stream), "D2H");
    }
    if (res.status != CBC_ST_OK) {
        snprintf(ctx->err, sizeof ctx->err, "stream decode stopped with status %u at record %u", res.status, res.fail_read);
        rc = CBC_E_BLOCK;
    }
done:
    if (d_in) (void)hipFree(d_in); if (d_co) (void)hipFree(d_co); if (d_cl) (void)hipFree(d_cl); if (d_recs) (void)hipFree(d_recs);
    if (d_seq) (void)hipFree(d_seq); if (d_res) (void)hipFree(d_res); if (d_vtab) (void)hipFree(d_vtab); if (d_aux) (void)hipFree(d_aux);
    return rc;
}

/* The decode twin of cbc_gpu_encode_stream_blocks: every block's payload is a stream of its own in the general (rescaling)
 * form of the models -- what a block of more than CBC_MAX_BLOCK_READS records needs, and what the block decoder refuses.
 * A block is decoded as a one-contig file whose contig is the block's reference window (decompress(), src/compression.c:
 * 173-216; the models never rescale-free here: src/stream_model.c:78-117).  One launch per block: a rare path. */
API int cbc_gpu_decode_stream_blocks(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, const cbc_dec_block_desc *blocks,
                                     uint32_t n_blocks, cbc_read_rec *recs, uint64_t n_recs, uint8_t *seq, uint64_t seq_bytes,
                                     cbc_block_result *results)
{
    if (!ctx || !in || !blocks || !recs || !seq) return CBC_E_ARG;
    if (!ctx->d_ref) return set_err(ctx, CBC_E_ARG, "cbc_gpu_upload_reference has not been called", hipSuccess);
    int rc = CBC_OK;
    for (uint32_t b = 0; b < n_blocks; b++) {
        const cbc_dec_block_desc *bd = &blocks[b];
        cbc_stream_result sr; memset(&sr, 0, sizeof sr);
        int one = CBC_E_ARG;
        if (bd->in_off <= in_bytes && bd->in_bytes <= in_bytes - bd->in_off && bd->rec_base <= n_recs && bd->n_reads <= n_recs - bd->rec_base &&
            bd->seq_stride >= 4 && bd->seq_stride <= 256 && (bd->seq_stride & 3u) == 0 && bd->seq_base <= seq_bytes &&
            (uint64_t)bd->n_reads * bd->seq_stride + 8 <= seq_bytes - bd->seq_base && bd->ref_off + CBC_REF_PAD < ctx->ref_bytes) {
            const uint64_t co = bd->ref_off, cl = ctx->ref_bytes - bd->ref_off - CBC_REF_PAD;      /* the window: from POS 1 of the block to the end */
            one = cbc_gpu_decode_stream(ctx, in + bd->in_off, bd->in_bytes, &co, &cl, 1, recs + bd->rec_base, bd->n_reads,
                                        seq + bd->seq_base, (uint64_t)bd->n_reads * bd->seq_stride + 8, bd->seq_stride, &sr);
            if (one == CBC_OK && sr.nbytes != bd->n_reads) { sr.status = CBC_ST_ASSERT; one = CBC_E_BLOCK; }     /* the index and the stream disagree */
        }
        if (results) { results[b].nbytes = (uint32_t)sr.nbytes; results[b].status = one == CBC_E_ARG ? CBC_ST_ASSERT : sr.status;
                       results[b].n_symbols = (uint32_t)sr.n_symbols; results[b].fail_read = sr.fail_read; }
        if (one != CBC_OK && rc == CBC_OK) {
            rc = one == CBC_E_ARG ? CBC_E_ARG : CBC_E_BLOCK;
            if (one == CBC_E_ARG) (void)set_err(ctx, CBC_E_ARG, "block descriptor outside the buffers", hipSuccess);
        }
    }
    return rc;
}

/* ------------------------------------------------------------------------------------------------
 * long-read format extension
 * ---------------------------------------------------------------------------------------------- */
API uint32_t cbc_gpu_long_lds_bytes(const cbc_lds_caps *caps) { return caps ? cbc_long_lds_bytes(caps->cap_pos) : 0; }

/* payload areas: 4096 + 64 per read + bytes_per_16_bases / 16 per base (typical streams need < 1 bit per base; the
 * worst case, every base an edit with an escaped gap, is 5 symbols of < 20 bits = 12.5 bytes per base = 200) */
API uint64_t cbc_gpu_long_plan_output(cbc_block_desc *blocks, uint32_t n_blocks, const cbc_read_rec *recs, uint32_t bytes_per_16_bases)
{
    uint64_t off = 0;
    for (uint32_t b = 0; b < n_blocks; b++) {
        uint64_t bases = 0;
        for (uint32_t r = 0; r < blocks[b].n_reads; r++) bases += recs[blocks[b].rec_base + r].rlen;
        uint64_t cap = (4096 + 64ull * blocks[b].n_reads + bases * bytes_per_16_bases / 16 + 255) & ~255ull;
        if (cap > 0xffffff00ull) cap = 0xffffff00ull;
        blocks[b].out_off = off; blocks[b].out_cap = (uint32_t)cap; blocks[b].reserved = (uint32_t)cap;
        off += cap;
    }
    return off;
}

API int cbc_gpu_long_encode_blocks_device(cbc_gpu_ctx *ctx, const cbc_device_batch *b, void *hip_stream)
{
    if (!ctx || !b) return CBC_E_ARG;
    if (b->n_blocks == 0) return CBC_OK;
    if (!b->d_recs || !b->d_seq || !b->d_tok || !b->d_names || !b->d_blocks || !b->d_ref || !b->d_out || !b->d_results)
        return set_err(ctx, CBC_E_ARG, "null device pointer in cbc_device_batch", hipSuccess);
    if (b->caps.cap_pos < 2 || b->caps.cap_pos > 8192) return set_err(ctx, CBC_E_ARG, "lds caps out of range", hipSuccess);
    const uint32_t lds = cbc_long_lds_bytes(b->caps.cap_pos);
    HIPCHK(hipSetDevice(ctx->device), "hipSetDevice");
    hipStream_t s = hip_stream == CBC_CTX_STREAM ? ctx->stream : (hipStream_t)hip_stream;
    cbc_long_args A;
    A.recs = b->d_recs; A.seq = b->d_seq; A.tok = b->d_tok; A.names = b->d_names; A.blocks = b->d_blocks;
    A.ref = b->d_ref; A.out = b->d_out; A.results = b->d_results;
    A.ref_bytes = b->ref_bytes; A.out_bytes = b->out_bytes; A.seq_bytes = b->seq_bytes; A.n_tok = b->n_tok;
    A.n_recs = b->n_recs; A.n_blocks = b->n_blocks; A.cap_pos = b->caps.cap_pos; A.names_bytes = 0x7fffffffu;
    /* the blocks' global-memory table parts (gap symbols 64.., gx): a buffer of the context, grown when a larger batch
     * comes (which waits for the device once); the kernel zeroes what it uses */
    { int rc_ = arena_need(ctx, A_LSCR, (uint64_t)b->n_blocks * CBC_LONG_SCRATCH_WORDS * 4 + 256, "hipMalloc long-read table scratch"); if (rc_) return rc_; }
    A.scratch = (uint32_t *)ctx->arena[A_LSCR].p;
    HIPCHK(hipEventRecord(ctx->ev0, s), "hipEventRecord");
    hipLaunchKernelGGL(cbc_long_encode_kernel, dim3(b->n_blocks), dim3(192), lds, s, A);
    HIPCHK(hipGetLastError(), "launch cbc_long_encode_kernel");
    HIPCHK(hipEventRecord(ctx->ev1, s), "hipEventRecord");
    ctx->have_timing = 1; ctx->last_variant = 0;
    return CBC_OK;
}

API int cbc_gpu_long_decode_blocks_device(cbc_gpu_ctx *ctx, const cbc_dec_device_batch *b, void *hip_stream)
{
    if (!ctx || !b) return CBC_E_ARG;
    if (b->n_blocks == 0) return CBC_OK;
    if (!b->d_in || !b->d_blocks || !b->d_ref || !b->d_recs || !b->d_seq || !b->d_results)
        return set_err(ctx, CBC_E_ARG, "null device pointer in cbc_dec_device_batch", hipSuccess);
    if (b->caps.cap_pos < 2 || b->caps.cap_pos > 8192) return set_err(ctx, CBC_E_ARG, "lds caps out of range", hipSuccess);
    const uint32_t lds = cbc_long_dec_lds_bytes(b->caps.cap_pos);
    HIPCHK(hipSetDevice(ctx->device), "hipSetDevice");
    hipStream_t s = hip_stream == CBC_CTX_STREAM ? ctx->stream : (hipStream_t)hip_stream;
    cbc_dec_args A;
    memset(&A, 0, sizeof A);
    A.in = b->d_in; A.blocks = b->d_blocks; A.ref = b->d_ref; A.recs = b->d_recs; A.seq = b->d_seq; A.results = b->d_results;
    A.in_bytes = b->in_bytes; A.ref_bytes = b->ref_bytes; A.n_recs = b->n_recs; A.seq_bytes = b->seq_bytes;
    A.n_blocks = b->n_blocks; A.cap_pos = b->caps.cap_pos; A.cap_var = 0;
    /* the blocks' global-memory table parts (cbc_long_body.h): the context's own buffer -- batch->d_var_scratch is not used */
    { int rc_ = arena_need(ctx, A_LSCR, (uint64_t)b->n_blocks * CBC_LONG_TABLE_WORDS * 4 + 256, "hipMalloc long-read table scratch"); if (rc_) return rc_; }
    A.var_scratch = (uint32_t *)ctx->arena[A_LSCR].p; A.var_scratch_words = (uint64_t)b->n_blocks * CBC_LONG_TABLE_WORDS;
    HIPCHK(hipEventRecord(ctx->ev0, s), "hipEventRecord");
    hipLaunchKernelGGL(cbc_long_decode_kernel, dim3(b->n_blocks), dim3(64), lds, s, A);
    HIPCHK(hipGetLastError(), "launch cbc_long_decode_kernel");
    HIPCHK(hipEventRecord(ctx->ev1, s), "hipEventRecord");
    ctx->have_timing = 1;
    return CBC_OK;
}

/* host buffers in, compacted payloads out: the block pipeline (encode_blocks_impl) as one chunk.  The areas are planned at
 * 0.5 bytes per base; a block whose area was too small (CBC_ST_OUT_FULL) makes the whole batch run once more with the
 * worst-case areas.  out == NULL is refused: the stash is for block-mode bitstreams. */
API int cbc_gpu_long_encode_blocks(cbc_gpu_ctx *ctx, const cbc_host_batch *hb, uint8_t *out, uint64_t out_cap,
                                   uint64_t *out_offsets, cbc_block_result *results)
{
    if (!ctx || !hb || !hb->seq || !out || !out_offsets) return CBC_E_ARG;
    const uint32_t nb = hb->n_blocks;
    cbc_block_result *res = results ? results : (cbc_block_result *)malloc(((size_t)nb + 1) * sizeof(cbc_block_result));
    if (!res) return CBC_E_NOMEM;
    memset(res, 0xff, (size_t)nb * sizeof(cbc_block_result)); /* a call that fails before the results arrive: no status, no retry */
    int rc = encode_blocks_impl(ctx, hb, cbc_gpu_long_plan_output(hb->blocks, nb, hb->recs, 8u), NULL, NULL, 0,
                                out, out_cap, out_offsets, res, NULL, NULL, true);
    bool full = false;
    for (uint32_t b = 0; b < nb; b++) full = full || res[b].status == CBC_ST_OUT_FULL;
    if (full)
        rc = encode_blocks_impl(ctx, hb, cbc_gpu_long_plan_output(hb->blocks, nb, hb->recs, 200u), NULL, NULL, 0,
                                out, out_cap, out_offsets, res, NULL, NULL, true);
    if (res != results) free(res);
    return rc;
}

API int cbc_gpu_long_decode_blocks(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, cbc_dec_block_desc *blocks,
                                   uint32_t n_blocks, const cbc_lds_caps *caps, cbc_read_rec *recs, uint64_t n_recs,
                                   uint8_t *seq, uint64_t seq_bytes, cbc_block_result *results)
{
    if (!ctx || !in || !blocks || !caps || !recs || !seq) return CBC_E_ARG;
    return decode_blocks_impl(ctx, in, in_bytes, blocks, n_blocks, caps, recs, n_recs, seq, seq_bytes, NULL, NULL, NULL, 0, NULL,
                              results, NULL, true);
}

/* decode with the bases returned as 2-bit rows (include/cbc_gpu.h) */
API int cbc_gpu_decode_blocks_2bit(cbc_gpu_ctx *ctx, const uint8_t *in, uint64_t in_bytes, cbc_dec_block_desc *blocks,
                                   uint32_t n_blocks, const cbc_lds_caps *caps, cbc_read_rec *recs, uint64_t n_recs,
                                   uint32_t *codes_out, uint64_t *exc_idx, uint8_t *exc_val, uint64_t exc_cap, uint64_t *n_exc,
                                   cbc_block_result *results)
{
    if (!ctx || !in || !blocks || !caps || !recs || !codes_out || !n_exc || (exc_cap && (!exc_idx || !exc_val))) return CBC_E_ARG;
    if (!ctx->d_ref) return set_err(ctx, CBC_E_ARG, "cbc_gpu_upload_reference has not been called", hipSuccess);
    *n_exc = 0;
    if (n_blocks == 0) return CBC_OK;
    const uint32_t stride = blocks[0].seq_stride;
    if (stride < 16 || stride > 256 || (stride & 15u)) return set_err(ctx, CBC_E_ARG, "2-bit decode wants seq_stride to be a multiple of 16", hipSuccess);
    for (uint32_t b = 0; b < n_blocks; b++) if (blocks[b].seq_stride != stride || blocks[b].seq_base != blocks[b].rec_base * stride)
        return set_err(ctx, CBC_E_ARG, "2-bit decode wants one stride and seq_base = rec_base * stride", hipSuccess);
    return decode_blocks_impl(ctx, in, in_bytes, blocks, n_blocks, caps, recs, n_recs, NULL, n_recs * stride, codes_out, exc_idx, exc_val,
                              exc_cap, n_exc, results);
}

API int cbc_gpu_encode_blocks_tokenised(cbc_gpu_ctx *ctx, const cbc_tok_result *t, const cbc_host_batch *hb,
                                        uint8_t *out, uint64_t out_cap, uint64_t *out_offsets, cbc_block_result *results)
{
    if (!t || !t->d_seq || !t->d_tok || !hb) return CBC_E_ARG;
    if (hb->seq_bytes != t->seq_bytes + 8 || hb->n_tok != t->n_tok) return set_err(ctx, CBC_E_ARG, "batch and tokeniser result disagree", hipSuccess);
    if (!t->summaries || hb->n_recs != t->n_recs) return set_err(ctx, CBC_E_ARG, "batch and tokeniser result disagree", hipSuccess);
    return encode_blocks_impl(ctx, hb, cbc_plan_output_summaries(hb->blocks, hb->n_blocks, t->summaries), NULL, NULL, 0,
                              out, out_cap, out_offsets, results, t->d_seq, t->d_tok);
}
