/*
 * wave_emu_sam.h -- the lock-step emulation (tests/emu/wave_emu.h) with the policy operations cbc_sam_body.h adds.
 * TEST AID ONLY, like the file it extends.
 */
#ifndef CBC_WAVE_EMU_SAM_H
#define CBC_WAVE_EMU_SAM_H

#include "../emu/wave_emu.h"

struct WaveEmuSam : WaveEmu {
    /* high word of the 64-bit product, per lane */
    static V32 mulhi(const V32 &a, const V32 &b)
    { V32 r; for (int i = 0; i < 64; i++) r.v[i] = (uint32_t)(((uint64_t)a.v[i] * b.v[i]) >> 32); return r; }
};

#endif
