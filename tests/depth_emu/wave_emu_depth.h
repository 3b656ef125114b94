/*
 * wave_emu_depth.h -- the lock-step emulation (tests/emu/wave_emu.h with the operations tests/sam_emu adds) as the coverage
 * bodies of cbc_depth_body.h use it.  TEST AID ONLY, like the files it extends.  The bodies need no operation of their own
 * (the agent-scope atomic add is the policy's list_add); what this twin adds is the check that lock-step execution hides:
 * lanes of one list_add may name the same word, and the sum must not depend on their order.
 */
#ifndef CBC_WAVE_EMU_DEPTH_H
#define CBC_WAVE_EMU_DEPTH_H

#include "../sam_emu/wave_emu_sam.h"

struct WaveEmuDepth : WaveEmuSam {
    /* += into a list in global memory, highest lane first (the base class goes lowest first): integer adds commute */
    static void list_add(uint32_t *p, const V32 &idx, const V32 &val, const Mask &m)
    { for (int i = 63; i >= 0; i--) if (m.b[i]) p[idx.v[i]] += val.v[i]; }
};

#endif
