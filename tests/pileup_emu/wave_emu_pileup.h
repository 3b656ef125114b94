/*
 * wave_emu_pileup.h -- the lock-step emulation (tests/depth_emu/wave_emu_depth.h and the files it extends) as the edit-reporting
 * decoder (cbc_decode_body.h, EDITS = true) and the pileup bodies (cbc_pileup_body.h) use it.  TEST AID ONLY, like the files it
 * extends.  What the bodies need beyond them are the three 16-bit operations of the edit arena.  What this twin adds as checks:
 * while the driver has named the arena with edit_arena(), every 16-bit access must stay inside it; while it has named word
 * ranges with add_range(), every list_add must fall into one of them (the difference array, the counter planes, the counters).
 */
#ifndef CBC_WAVE_EMU_PILEUP_H
#define CBC_WAVE_EMU_PILEUP_H

#include <vector>
#include "../depth_emu/wave_emu_depth.h"

struct WaveEmuPileup : WaveEmuDepth {
    struct range { const uint32_t *lo, *hi; };
    static std::vector<range> &ranges() { static thread_local std::vector<range> r; return r; }
    static void add_range(const uint32_t *p, uint64_t words) { range r = { p, p + words }; ranges().push_back(r); }
    static void clear_ranges() { ranges().clear(); }
    static const uint16_t *&ar_lo() { static thread_local const uint16_t *p = nullptr; return p; }
    static uint64_t &ar_n() { static thread_local uint64_t n = 0; return n; }
    static void edit_arena(const uint16_t *p, uint64_t entries) { ar_lo() = p; ar_n() = entries; }
    static bool in_arena(const uint16_t *p, uint32_t idx)
    {
        if (ar_lo() == nullptr) return true;
        if (p >= ar_lo() && (uint64_t)(p - ar_lo()) + idx < ar_n()) return true;
        emu_oob("16-bit access outside the edit arena");
        return false;
    }
    static void list_add(uint32_t *p, const V32 &idx, const V32 &val, const Mask &m)
    {
        for (int i = 63; i >= 0; i--) {
            if (!m.b[i]) continue;
            const uint32_t *at = p + idx.v[i];
            bool ok = ranges().empty();
            for (size_t k = 0; k < ranges().size() && !ok; k++) ok = at >= ranges()[k].lo && at < ranges()[k].hi;
            if (!ok) { emu_oob("list_add outside the named tables"); continue; }
            p[idx.v[i]] += val.v[i];
        }
    }
    static void store16(uint16_t *p, const V32 &idx, const V32 &val, const Mask &m)
    {
        for (int i = 0; i < 64; i++) {
            if (!m.b[i] || !in_arena(p, idx.v[i])) continue;
            if (val.v[i] > 0xffffu) emu_oob("an arena entry does not fit 16 bits");
            p[idx.v[i]] = (uint16_t)val.v[i];
        }
    }
    static V32 load16(const uint16_t *p, const V32 &idx, const Mask &m)
    { V32 r; for (int i = 0; i < 64; i++) r.v[i] = (m.b[i] && in_arena(p, idx.v[i])) ? p[idx.v[i]] : 0u; return r; }
    static uint32_t read_uni16(const uint16_t *p, uint32_t idx) { return in_arena(p, idx) ? p[idx] : 0u; }
};

#endif
