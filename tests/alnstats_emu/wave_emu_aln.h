/*
 * wave_emu_aln.h -- the lock-step emulation (tests/cigar_emu/wave_emu_cigar.h and the files it extends) as the alignment-table
 * bodies of cbc_stats_aln_body.h and the statistics bodies of cbc_stats_body.h use it.  TEST AID ONLY, like the files it extends.
 * The bodies need no operation of their own.  The cigar twin brings the edit arena's 16-bit operations and the named word ranges
 * every list_add must fall into (the two global tables); what this twin adds is the workgroup's table in LDS as tests/hist_emu
 * keeps it: a plain array the driver names with wg_table(), every zero / add / read checked against its length, the adds highest
 * lane first.
 */
#ifndef CBC_WAVE_EMU_ALN_H
#define CBC_WAVE_EMU_ALN_H

#include "../cigar_emu/wave_emu_cigar.h"

struct WaveEmuAln : WaveEmuCigar {
    static uint32_t *&tab() { static thread_local uint32_t *t = nullptr; return t; }
    static uint32_t &tab_words() { static thread_local uint32_t n = 0; return n; }
    static void wg_table(uint32_t *p, uint32_t words) { tab() = p; tab_words() = words; }
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
