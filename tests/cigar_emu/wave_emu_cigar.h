/*
 * wave_emu_cigar.h -- the lock-step emulation (tests/pileup_emu/wave_emu_pileup.h and the files it extends) as the SAM CIGAR /
 * NM / MD bodies (cbc_cigar_body.h) use it.  TEST AID ONLY, like the files it extends.  The bodies need no operation of their
 * own.  What this twin adds as checks: while the driver has named the text with text_range(), every byte and dword store must
 * fall inside it, and no byte of it may be stored twice (a line's fields, tokens and tags are disjoint); while it has named word
 * ranges with add_range(), every write_uni must fall into one of them (the per-record words of the measure pass, the counts).
 */
#ifndef CBC_WAVE_EMU_CIGAR_H
#define CBC_WAVE_EMU_CIGAR_H

#include <vector>
#include "../pileup_emu/wave_emu_pileup.h"

struct WaveEmuCigar : WaveEmuPileup {
    static uint8_t *&tx_lo() { static thread_local uint8_t *p = nullptr; return p; }
    static std::vector<uint8_t> &tx_seen() { static thread_local std::vector<uint8_t> s; return s; }
    static void text_range(uint8_t *p, uint64_t bytes) { tx_lo() = p; tx_seen().assign(p ? (size_t)bytes : 0u, 0u); }
    static bool text_ok(const uint8_t *at, uint32_t n)
    {
        if (tx_lo() == nullptr) return true;
        if (at < tx_lo() || (uint64_t)(at - tx_lo()) + n > tx_seen().size()) { emu_oob("store outside the text"); return false; }
        for (uint32_t i = 0; i < n; i++) {
            uint8_t &s = tx_seen()[(size_t)(at - tx_lo()) + i];
            if (s) emu_oob("a byte of the text is stored twice");
            s = 1u;
        }
        return true;
    }
    static void store8(uint8_t *p, const V32 &off, const V32 &val, const Mask &m)
    { for (int i = 0; i < 64; i++) if (m.b[i] && text_ok(p + off.v[i], 1u)) p[off.v[i]] = (uint8_t)val.v[i]; }
    static void store32_bytes(uint8_t *p, const V32 &off, const V32 &val, const Mask &m)
    { for (int i = 0; i < 64; i++) if (m.b[i] && text_ok(p + off.v[i], 4u)) memcpy(p + off.v[i], &val.v[i], 4); }
    static void write_uni(uint32_t *p, uint32_t idx, uint32_t val)
    {
        bool ok = ranges().empty();
        for (size_t k = 0; k < ranges().size() && !ok; k++) ok = p + idx >= ranges()[k].lo && p + idx < ranges()[k].hi;
        if (!ok) { emu_oob("write_uni outside the named tables"); return; }
        p[idx] = val;
    }
};

#endif
