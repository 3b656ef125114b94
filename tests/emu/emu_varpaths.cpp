/*
 * emu_varpaths.cpp -- the lock-step emulation of emu_encode.cpp built with the counters of CbcEnc::var_code (CBC_VAR_COUNTS,
 * cbc_amd/csrc/cbc_encode_body.h): per block and strand, how many calls there were, how many of the p = 0 class, how many
 * the hot context's count table answered, how many found their bucket full, went through the Bloom branch, scanned the
 * global event list.  emu_var_hot(0) switches the hot table off, which is the form before it: the same bytes by the other
 * route, for the counts to be compared.  TEST AID ONLY, like the rest of this directory; the device code carries no
 * counter and no switch.  Built by varpaths_emu.mk into libcbc_emu_varpaths.so, which exports what libcbc_emu.so exports
 * and emu_var_counts() / emu_var_hot() besides.
 */
#define CBC_VAR_COUNTS
#include "emu_encode.cpp"

#define CBC_VC_MAX_BLOCKS 64u                   /* blocks of one call that are counted apart; later ones add to the last row */
static uint64_t g_var_counts[CBC_VC_MAX_BLOCKS][2][CBC_VC_N];
static int g_var_hot_off = 0;
static thread_local uint32_t g_var_blk = 0;     /* the model thread of the two-thread form sets its own */

extern "C" void cbc_var_block(uint32_t blk) { g_var_blk = blk < CBC_VC_MAX_BLOCKS ? blk : CBC_VC_MAX_BLOCKS - 1u; }
extern "C" void cbc_var_count(uint32_t what, uint32_t strand)
{
    if (what < CBC_VC_N) __atomic_fetch_add(&g_var_counts[g_var_blk][strand & 1u][what], 1ull, __ATOMIC_RELAXED);
}
extern "C" int cbc_var_hot_off(void) { return g_var_hot_off; }

/* on != 0: the hot context in its count table (the kernel's form); 0: every context through the buckets and lists */
extern "C" __attribute__((visibility("default")))
void emu_var_hot(int on) { g_var_hot_off = on ? 0 : 1; }

/* copies the counts of the first n_blocks blocks (n_blocks x 2 strands x CBC_VC_N, order: the CBC_VC_* enum) to `out`, clears
 * all of them if `reset`; returns CBC_VC_N */
extern "C" __attribute__((visibility("default")))
uint32_t emu_var_counts(uint64_t *out, uint32_t n_blocks, int reset)
{
    for (uint32_t b = 0; b < CBC_VC_MAX_BLOCKS; b++)
        for (uint32_t s = 0; s < 2u; s++)
            for (uint32_t k = 0; k < CBC_VC_N; k++) {
                if (out && b < n_blocks) out[(b * 2u + s) * CBC_VC_N + k] = __atomic_load_n(&g_var_counts[b][s][k], __ATOMIC_RELAXED);
                if (reset) __atomic_store_n(&g_var_counts[b][s][k], 0ull, __ATOMIC_RELAXED);
            }
    return CBC_VC_N;
}
