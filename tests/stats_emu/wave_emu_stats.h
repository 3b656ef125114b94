/*
 * wave_emu_stats.h -- the lock-step emulation (tests/hist_emu/wave_emu_hist.h and the files it extends) as the statistics bodies
 * of cbc_stats_body.h use it.  TEST AID ONLY, like the files it extends.  The bodies need no operation of their own.  The
 * workgroup's table in LDS is the bounds-checked table of the histogram twin (wg_table()); what this twin adds is the same check
 * for the global count table: while the driver has named it with global_table(), every list_add must stay inside it.
 */
#ifndef CBC_WAVE_EMU_STATS_H
#define CBC_WAVE_EMU_STATS_H

#include "../hist_emu/wave_emu_hist.h"

struct WaveEmuStats : WaveEmuHist {
    static uint32_t *&gtab() { static thread_local uint32_t *t = nullptr; return t; }
    static uint32_t &gtab_words() { static thread_local uint32_t n = 0; return n; }
    static void global_table(uint32_t *p, uint32_t words) { gtab() = p; gtab_words() = words; }
    static void list_add(uint32_t *p, const V32 &idx, const V32 &val, const Mask &m)
    {
        for (int i = 63; i >= 0; i--) {
            if (!m.b[i]) continue;
            if (gtab() != nullptr && (p != gtab() || idx.v[i] >= gtab_words())) { emu_oob("index outside the global count table"); continue; }
            p[idx.v[i]] += val.v[i];
        }
    }
};

#endif
