/*
 * emu_paths.cpp -- the lock-step emulation of emu_encode.cpp built with the coder's path counters (CBC_PATH_COUNTS,
 * cbc_amd/csrc/cbc_encode_body.h) and with the two fused quiet steps that the default kernel build leaves out (CBC_FUSE_SR,
 * CBC_FUSE_X3): how often the remainder branch of each step kind was taken, and how often the fused quiet steps took their
 * fused exit or fell back, by a shift or by a remainder flag.  TEST AID ONLY, like the rest of this
 * directory; the device code carries no counter.  Built by paths_emu.mk into libcbc_emu_paths.so, which exports what
 * libcbc_emu.so exports and emu_path_counts() besides.
 */
#define CBC_PATH_COUNTS
#ifndef CBC_PATHS_NO_FUSE                       /* -DCBC_PATHS_NO_FUSE: the counters on the steps of the default kernel build */
#define CBC_FUSE_SR                             /* the two fused quiet steps: A/B switches of the kernel build, run and */
#define CBC_FUSE_X3                             /* cross-checked here                                                   */
#endif
#include "emu_encode.cpp"

/* [0]: records below CBC_PC_LATE of their block, [1]: the rest.  Only a block's coder runs the counted steps, but the
 * two-thread form runs it beside the model thread: relaxed atomics. */
#define CBC_PC_LATE 512u
static uint64_t g_path_counts[2][CBC_PC_N];
static thread_local int g_path_mute = 0;

extern "C" void cbc_path_count(uint32_t what, uint32_t read)
{
    if (g_path_mute || what >= CBC_PC_N) return;
    __atomic_fetch_add(&g_path_counts[read >= CBC_PC_LATE ? 1 : 0][what], 1ull, __ATOMIC_RELAXED);
}
extern "C" void cbc_path_mute(int on) { g_path_mute = on; }

/* copies the 2 x CBC_PC_N counts (order: the CBC_PC_* enum) to `out`, clears them if `reset`; returns CBC_PC_N */
extern "C" __attribute__((visibility("default")))
uint32_t emu_path_counts(uint64_t *out, int reset)
{
    for (uint32_t h = 0; h < 2u; h++)
        for (uint32_t k = 0; k < CBC_PC_N; k++) {
            if (out) out[h * CBC_PC_N + k] = __atomic_load_n(&g_path_counts[h][k], __ATOMIC_RELAXED);
            if (reset) __atomic_store_n(&g_path_counts[h][k], 0ull, __ATOMIC_RELAXED);
        }
    return CBC_PC_N;
}
