/*
 * region_emu.cpp -- the region decode bodies on the CPU through the lock-step wave emulation (tests/emu/wave_emu.h).
 * TEST AID ONLY: the span-reporting decoder and the filter / text passes are checked against the Python model under
 * ASan-able host code before anything runs on a GPU.  The scan between the passes is the host loop of tests/emu/post_emu.h (on
 * the device it is cbc_scan_sizes_kernel, shared with the encode path).
 */
#include "../emu/post_emu.h"
#include "../../cbc_amd/csrc/cbc_region_body.h"

/* the span-reporting decoder over every block of the batch, on the plain WaveEmu */
extern "C" __attribute__((visibility("default")))
int emu_decode_span(const cbc_dec_device_batch *b, uint32_t smax) { return emu_decode_blocks<WaveEmu, true>(b, smax); }

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
    scan(counts, offsets, n_blocks);
    for (uint32_t b = 0; b < n_blocks; b++)
        for (uint32_t w = 0; w < n_waves; w++) cbc_region_write<WaveEmu>(A, b, w, n_waves);
    return g_emu_errors ? -100 : 0;
}
