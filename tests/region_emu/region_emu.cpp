/*
 * region_emu.cpp -- the region decode bodies on the CPU through the lock-step wave emulation (tests/emu/wave_emu.h).
 * TEST AID ONLY: the span-reporting decoder and the filter / text passes are checked against the Python model under
 * ASan-able host code before anything runs on a GPU.  The scan between the passes is the host loop below (on the device
 * it is cbc_scan_sizes_kernel, shared with the encode path).
 */
#include <vector>
#include "../emu/wave_emu.h"
#include "../../cbc_amd/csrc/cbc_encode_body.h"
#include "../../cbc_amd/csrc/cbc_decode_body.h"
#include "../../cbc_amd/csrc/cbc_plan.h"
#include "../../cbc_amd/csrc/cbc_region_body.h"

static int g_emu_errors = 0;
extern "C" void emu_oob(const char *what) { fprintf(stderr, "[emu] invariant violated: %s\n", what); g_emu_errors++; }

/* cbc_decode_stream<WaveEmu, true> over every block of the batch */
extern "C" __attribute__((visibility("default")))
int emu_decode_span(const cbc_dec_device_batch *b, uint32_t smax)
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
        cbc_decode_stream<WaveEmu, true>(A, blk, lds.data(), smax);
    }
    return g_emu_errors ? -100 : 0;
}

/* count pass, exclusive scan, write pass (n_waves wavefronts per block, run one after the other) */
extern "C" __attribute__((visibility("default")))
int emu_region(const cbc_read_rec *recs, uint64_t n_recs, const uint8_t *seq, uint64_t seq_bytes, const cbc_dec_block_desc *blocks,
               const uint64_t *window_start, const cbc_block_result *dec_results, uint32_t n_blocks, uint64_t beg, uint64_t end,
               uint8_t *text, uint64_t text_cap, cbc_block_result *counts, uint64_t *offsets, uint32_t n_waves)
{
    cbc_region_args A;
    memset(&A, 0, sizeof A);
    A.recs = recs; A.seq = seq; A.blocks = blocks; A.window_start = window_start; A.dec_results = dec_results;
    A.counts = counts; A.offsets = offsets; A.text = text; A.text_cap = text_cap; A.n_recs = n_recs; A.seq_bytes = seq_bytes;
    A.beg = beg; A.end = end; A.n_blocks = n_blocks;
    g_emu_errors = 0;
    for (uint32_t b = 0; b < n_blocks; b++) cbc_region_count<WaveEmu>(A, b);
    uint64_t run = 0;
    for (uint32_t b = 0; b < n_blocks; b++) { offsets[b] = run; run += counts[b].status == CBC_ST_OK ? counts[b].nbytes : 0u; }
    offsets[n_blocks] = run;
    for (uint32_t b = 0; b < n_blocks; b++)
        for (uint32_t w = 0; w < n_waves; w++) cbc_region_write<WaveEmu>(A, b, w, n_waves);
    return g_emu_errors ? -100 : 0;
}
