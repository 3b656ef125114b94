/*
 * wave_emu_hist.h -- the lock-step emulation (tests/emu/wave_emu.h with what tests/sam_emu and tests/depth_emu add) as the
 * histogram bodies of cbc_hist_body.h use it.  TEST AID ONLY, like the files it extends.  The accumulate body is the first of
 * the depth family to keep a table in LDS: here that table is a plain array per emulated workgroup, which the driver names with
 * wg_table() before it runs the workgroup, and every zero / add / read of it is checked against its length.  The adds go highest
 * lane first, like the list_add of the depth twin: lanes may name the same word, and the sum must not depend on their order.
 */
#ifndef CBC_WAVE_EMU_HIST_H
#define CBC_WAVE_EMU_HIST_H

#include "../depth_emu/wave_emu_depth.h"

struct WaveEmuHist : WaveEmuDepth {
    static uint32_t *&tab() { static thread_local uint32_t *t = nullptr; return t; }
    static uint32_t &tab_words() { static thread_local uint32_t n = 0; return n; }
    static void wg_table(uint32_t *p, uint32_t words) { tab() = p; tab_words() = words; }
    /* while a workgroup's table is named, every LDS operation must stay inside it; with none named (the decoder's own LDS
     * tables, which its driver allocates) the operation is the base class's */
    static bool in(const uint32_t *p, uint32_t i)
    {
        if (tab() == nullptr) return true;
        if (p != tab() || i >= tab_words()) { emu_oob("index outside the workgroup's LDS table"); return false; }
        return true;
    }
    static void lds_zero(uint32_t *p, const V32 &idx, const Mask &m) { for (int i = 0; i < 64; i++) if (m.b[i] && in(p, idx.v[i])) p[idx.v[i]] = 0u; }
    static void lds_add(uint32_t *p, const V32 &idx, const V32 &val, const Mask &m)
    { for (int i = 63; i >= 0; i--) if (m.b[i] && in(p, idx.v[i])) p[idx.v[i]] += val.v[i]; }
    static V32 lds_read(const uint32_t *p, const V32 &idx, const Mask &m)
    { V32 r; for (int i = 0; i < 64; i++) r.v[i] = m.b[i] && in(p, idx.v[i]) ? p[idx.v[i]] : 0u; return r; }
};

#endif
