/*
 * sam_emu.cpp -- the SAM text bodies (cbc_amd/csrc/cbc_sam_body.h) on the CPU through the lock-step wave emulation.
 * TEST AID ONLY: the count and the write pass are checked against the Python model (tests/sammodel.py) under ASan-able host
 * code before anything runs on a GPU.  The records come from the emulated decoders (plain, or span-reporting for a region) or
 * from arrays the test builds.  The scan between the passes is the host loop of tests/emu/post_emu.h (on the device:
 * cbc_scan_sizes_kernel).
 */
#include "../emu/post_emu.h"
#include "../../cbc_amd/csrc/cbc_sam_body.h"

/* the decoder over every block of the batch: smax = 0 the plain one, otherwise the span-reporting one */
extern "C" __attribute__((visibility("default")))
int emu_sam_decode(const cbc_dec_device_batch *b, uint32_t smax) { return smax ? emu_decode_blocks<WP, true>(b, smax) : emu_decode_blocks<WP, false>(b, 0u); }

/* count pass, exclusive scan, write pass (n_waves wavefronts per block, run one after the other).  region != 0: keep by
 * [beg, end].  Returns -1 (CBC_E_ARG) with offsets[n_blocks] set and nothing written when the text does not fit text_cap,
 * as cbc_gpu_decode_sam does. */
extern "C" __attribute__((visibility("default")))
int emu_sam(const cbc_read_rec *recs, uint64_t n_recs, const uint8_t *seq, uint64_t seq_bytes, const cbc_dec_block_desc *blocks,
            const uint64_t *window_start, const cbc_block_result *dec_results, uint32_t n_blocks, const uint32_t *block_name,
            const uint8_t *names, uint32_t names_bytes, int region, uint64_t beg, uint64_t end,
            uint8_t *text, uint64_t text_cap, cbc_block_result *counts, uint64_t *offsets, uint32_t n_waves)
{
    cbc_sam_args A;
    memset(&A, 0, sizeof A);
    A.R.recs = recs; A.R.seq = seq; A.R.blocks = blocks; A.R.window_start = window_start; A.R.dec_results = dec_results;
    A.R.counts = counts; A.R.offsets = offsets; A.R.text = text; A.R.text_cap = text_cap; A.R.n_recs = n_recs; A.R.seq_bytes = seq_bytes;
    A.R.beg = region ? beg : 1u; A.R.end = region ? end : UINT64_MAX; A.R.n_blocks = n_blocks;
    A.block_name = block_name; A.names = names; A.names_bytes = names_bytes; A.region = region ? 1u : 0u;
    g_emu_errors = 0;
    for (uint32_t b = 0; b < n_blocks; b++) cbc_sam_count<WP>(A, b);
    scan(counts, offsets, n_blocks);
    if (offsets[n_blocks] > text_cap) return CBC_E_ARG;
    for (uint32_t b = 0; b < n_blocks; b++)
        for (uint32_t w = 0; w < n_waves; w++) cbc_sam_write<WP>(A, b, w, n_waves);
    return g_emu_errors ? -100 : 0;
}
