/*
 * targets_emu.cpp -- the target-set bodies (cbc_amd/csrc/cbc_targets_body.h) on the CPU through the lock-step wave emulation.
 * TEST AID ONLY: the keep rule over the interval table, the count / write passes for reads and SAM, and the depth passes in
 * the compressed coordinate are checked against the Python models and the single-region emulations under ASan-able host
 * code before anything runs on a GPU.  The scans between the passes are the host loops below (on the device:
 * cbc_scan_sizes_kernel).  Every table is copied into an allocation of its exact size, so an index past it is an ASan finding.
 */
#include <vector>
#include "../depth_emu/wave_emu_depth.h"
#include "../../cbc_amd/csrc/cbc_encode_body.h"
#include "../../cbc_amd/csrc/cbc_decode_body.h"
#include "../../cbc_amd/csrc/cbc_plan.h"
#include "../../cbc_amd/csrc/cbc_targets_body.h"

static int g_emu_errors = 0;
extern "C" void emu_oob(const char *what) { fprintf(stderr, "[emu] invariant violated: %s\n", what); g_emu_errors++; }

/* the span-reporting decoder over every block of the batch */
extern "C" __attribute__((visibility("default")))
int emu_targets_decode(const cbc_dec_device_batch *b, uint32_t smax)
{
    cbc_dec_args A;
    memset(&A, 0, sizeof A);
    A.in = b->d_in; A.blocks = b->d_blocks; A.ref = b->d_ref; A.recs = b->d_recs; A.seq = b->d_seq; A.results = b->d_results;
    A.in_bytes = b->in_bytes; A.ref_bytes = b->ref_bytes; A.n_recs = b->n_recs; A.seq_bytes = b->seq_bytes;
    A.n_blocks = b->n_blocks; A.cap_pos = b->caps.cap_pos; A.cap_var = b->caps.cap_var;
    A.var_scratch = b->d_var_scratch; A.var_scratch_words = b->var_scratch_words;
    g_emu_errors = 0;
    uint32_t words = cbc_plan_dec_lds_bytes(&b->caps) / 4;
    for (uint32_t blk = 0; blk < b->n_blocks; blk++) {
        std::vector<uint32_t> lds(words, 0xdeadbeefu);
        cbc_decode_stream<WaveEmuDepth, true>(A, blk, lds.data(), smax);
    }
    return g_emu_errors ? -100 : 0;
}

static void scan(const cbc_block_result *r, uint64_t *off, uint32_t n)
{
    uint64_t run = 0;
    for (uint32_t i = 0; i < n; i++) { off[i] = run; run += r[i].status == CBC_ST_OK ? r[i].nbytes : 0u; }
    off[n] = run;
}

/* reads (sam = 0) or SAM lines (sam != 0): count pass, scan, write pass (n_waves wavefronts per block, one after the other).
 * out[0] = text bytes, out[1] = reads kept.  Returns -1 (CBC_E_ARG) with out[] set and nothing written when the text does not
 * fit text_cap, as cbc_gpu_decode_targets does. */
extern "C" __attribute__((visibility("default")))
int emu_targets(const cbc_read_rec *recs, uint64_t n_recs, const uint8_t *seq, uint64_t seq_bytes, const cbc_dec_block_desc *blocks,
                const uint64_t *window_start, const cbc_block_result *dec_results, uint32_t n_blocks, const uint32_t *block_name,
                const uint8_t *names, uint32_t names_bytes, const uint32_t *iv, uint32_t n_iv, const uint32_t *block_iv, int sam,
                uint8_t *text, uint64_t text_cap, uint32_t n_waves, uint64_t *out)
{
    std::vector<uint32_t> ivv(iv, iv + 2u * (size_t)n_iv), biv(block_iv, block_iv + 2u * (size_t)n_blocks);
    std::vector<cbc_block_result> counts(n_blocks);
    std::vector<uint64_t> offs(n_blocks + 1u);
    cbc_targets_args A;
    memset(&A, 0, sizeof A);
    A.S.R.recs = recs; A.S.R.seq = seq; A.S.R.blocks = blocks; A.S.R.window_start = window_start; A.S.R.dec_results = dec_results;
    A.S.R.counts = counts.data(); A.S.R.offsets = offs.data(); A.S.R.text = text; A.S.R.text_cap = text_cap; A.S.R.n_recs = n_recs;
    A.S.R.seq_bytes = seq_bytes; A.S.R.beg = 1u; A.S.R.end = UINT64_MAX; A.S.R.n_blocks = n_blocks;
    A.S.block_name = block_name; A.S.names = names; A.S.names_bytes = names_bytes; A.S.region = 0u;
    A.iv = ivv.data(); A.block_iv = biv.data(); A.n_iv = n_iv;
    g_emu_errors = 0;
    for (uint32_t b = 0; b < n_blocks; b++) { if (sam) cbc_targets_sam_count<WaveEmuDepth>(A, b); else cbc_targets_count<WaveEmuDepth>(A, b); }
    scan(counts.data(), offs.data(), n_blocks);
    out[0] = offs[n_blocks]; out[1] = 0;
    for (uint32_t b = 0; b < n_blocks; b++) out[1] += counts[b].n_symbols;
    if (out[0] > text_cap) return CBC_E_ARG;
    for (uint32_t b = 0; b < n_blocks; b++)
        for (uint32_t w = 0; w < n_waves; w++) {
            if (sam) cbc_targets_sam_write<WaveEmuDepth>(A, b, w, n_waves); else cbc_targets_write<WaveEmuDepth>(A, b, w, n_waves);
        }
    return g_emu_errors ? -100 : 0;
}

/* the depth of ONE contig's intervals (iv: its n_iv pairs; block_iv relative to them), every pass in the order of
 * cbc_gpu_decode_targets.  out[0] = text bytes, out[1] = lines, out[2] = reads counted, out[3] = change points, out[4] = words
 * of the difference array. */
extern "C" __attribute__((visibility("default")))
int emu_targets_depth(const cbc_read_rec *recs, uint64_t n_recs, const uint8_t *seq, uint64_t seq_bytes, const cbc_dec_block_desc *blocks,
                      const uint64_t *window_start, const cbc_block_result *dec_results, uint32_t n_blocks, const uint8_t *name,
                      uint32_t name_len, const uint32_t *iv, uint32_t n_iv, const uint32_t *block_iv, uint32_t exclude,
                      uint8_t *text, uint64_t text_cap, uint64_t *out)
{
    g_emu_errors = 0;
    out[0] = out[1] = out[2] = out[3] = out[4] = 0;
    if (n_recs > 0x3fffffffull || n_iv == 0) return CBC_E_ARG;
    std::vector<uint32_t> ivv(iv, iv + 2u * (size_t)n_iv), biv(block_iv, block_iv + 2u * (size_t)n_blocks), ioff(n_iv + 1u);
    uint64_t run = 0;
    for (uint32_t i = 0; i < n_iv; i++) {
        if (iv[2 * i] < 1 || iv[2 * i] > iv[2 * i + 1] || iv[2 * i + 1] > CBC_SAM_MAX_POS || (i && iv[2 * i] <= iv[2 * i - 1] + 1u)) return CBC_E_ARG;
        ioff[i] = (uint32_t)run; run += (uint64_t)(iv[2 * i + 1] - iv[2 * i]) + 2u;
    }
    ioff[n_iv] = (uint32_t)run;
    const uint64_t d_words = run;
    const uint32_t n_tiles = (uint32_t)((d_words + CBC_DEPTH_TILE - 1u) / CBC_DEPTH_TILE);
    const uint32_t cp_cap = (uint32_t)(2u * n_recs + 2u * (uint64_t)n_iv), n_ttiles = (cp_cap + CBC_DEPTH_LINES - 1u) / CBC_DEPTH_LINES;
    std::vector<uint32_t> diff((size_t)n_tiles * CBC_DEPTH_TILE, 0u), cp_pos(cp_cap + 1u, 0xEEEEEEEEu), cp_dep(cp_cap + 1u, 0xEEEEEEEEu);
    std::vector<cbc_block_result> tsum(n_tiles), tcnt(n_tiles), counts(n_ttiles + 1u);
    std::vector<uint64_t> soff(n_tiles + 1u), coff(n_tiles + 1u), toff(n_ttiles + 1u);
    std::vector<uint8_t> nm(name, name + name_len);
    uint32_t ctr[4] = { 0, 0, 0, 0 };
    cbc_tdepth_args A;
    memset(&A, 0, sizeof A);
    A.D.R.recs = recs; A.D.R.seq = seq; A.D.R.blocks = blocks; A.D.R.window_start = window_start; A.D.R.dec_results = dec_results;
    A.D.R.counts = counts.data(); A.D.R.offsets = toff.data(); A.D.R.text = text; A.D.R.text_cap = text_cap; A.D.R.n_recs = n_recs;
    A.D.R.seq_bytes = seq_bytes; A.D.R.beg = 1u; A.D.R.end = UINT64_MAX; A.D.R.n_blocks = n_blocks;
    A.D.diff = diff.data(); A.D.diff_words = diff.size(); A.D.tile_sum = tsum.data(); A.D.tile_cnt = tcnt.data();
    A.D.sum_off = soff.data(); A.D.cnt_off = coff.data(); A.D.cp_pos = cp_pos.data(); A.D.cp_dep = cp_dep.data(); A.D.cp_cap = cp_cap;
    A.D.ctr = ctr; A.D.name = nm.data(); A.D.name_len = name_len; A.D.exclude = exclude; A.D.n_tiles = n_tiles; A.D.n_ttiles = n_ttiles;
    A.iv = ivv.data(); A.iv_off = ioff.data(); A.block_iv = biv.data(); A.n_iv = n_iv;
    for (uint32_t b = 0; b < n_blocks; b++) cbc_targets_mark<WaveEmuDepth>(A, b);
    for (uint32_t t = 0; t < n_tiles; t++) cbc_depth_tile<WaveEmuDepth>(A.D, t);
    scan(tsum.data(), soff.data(), n_tiles);
    scan(tcnt.data(), coff.data(), n_tiles);
    for (uint32_t t = 0; t < n_tiles; t++) cbc_depth_compact<WaveEmuDepth>(A.D, t);
    if (cp_pos[cp_cap] != 0xEEEEEEEEu || cp_dep[cp_cap] != 0xEEEEEEEEu) emu_oob("change point written past the table");
    if (coff[n_tiles] > cp_cap) emu_oob("more change points than 2K + 2n");
    for (uint32_t t = 0; t < n_ttiles; t++) cbc_targets_depth_count<WaveEmuDepth>(A, t);
    scan(counts.data(), toff.data(), n_ttiles);
    out[0] = toff[n_ttiles]; out[1] = ctr[1]; out[2] = ctr[0]; out[3] = coff[n_tiles]; out[4] = d_words;
    if (out[0] > text_cap) return CBC_E_ARG;
    for (uint32_t t = 0; t < n_ttiles; t++) cbc_targets_depth_write<WaveEmuDepth>(A, t);
    return g_emu_errors ? -100 : 0;
}
