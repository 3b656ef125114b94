/*
 * wave_emu_post.h -- the lock-step emulation (wave_emu.h) as the post-decode bodies use it: the SAM text, coverage, histogram,
 * statistics, pileup, CIGAR and alignment-table bodies (cbc_amd/csrc/cbc_*_body.h) and the edit-reporting decoder.  TEST AID
 * ONLY, like the file it extends.  One policy for every driver under tests/<name>_emu.  Beyond the few operations the bodies add,
 * it holds the checks that lock-step execution hides.  Every check is opt-in: it is inactive until the driver names a range, an
 * arena, a text or a table, and inactive again once the driver takes the name back.  The state is thread_local, and each
 * library and check program keeps its own copy.
 */
#ifndef CBC_WAVE_EMU_POST_H
#define CBC_WAVE_EMU_POST_H

#include <vector>
#include "wave_emu.h"

struct __attribute__((visibility("hidden"))) WaveEmuPost : WaveEmu {
    /* ---- cbc_sam_body.h: high word of the 64-bit product, per lane ---- */
    static V32 mulhi(const V32 &a, const V32 &b)
    { V32 r; for (int i = 0; i < 64; i++) r.v[i] = (uint32_t)(((uint64_t)a.v[i] * b.v[i]) >> 32); return r; }

    /* ---- named word ranges: add_range(), add_uni_range() ----
     * While the driver has named word ranges with add_range(), every list_add must fall into one of them (pileup: the
     * difference array, the counter planes, the counters; the alignment tables: the two global tables).  While it has named
     * word ranges with add_uni_range(), every write_uni must fall into one of those (CIGAR: the per-record words of the measure
     * pass, the counts). */
    struct range { const uint32_t *lo, *hi; };
    typedef std::vector<range> range_list;
    static range_list &ranges() { static thread_local range_list r; return r; }
    static range_list &uni_ranges() { static thread_local range_list r; return r; }
    static void add_range(const uint32_t *p, uint64_t words) { range r = { p, p + words }; ranges().push_back(r); }
    static void add_uni_range(const uint32_t *p, uint64_t words) { range r = { p, p + words }; uni_ranges().push_back(r); }
    static void clear_ranges() { ranges().clear(); uni_ranges().clear(); }
    static bool in_ranges(const range_list &l, const uint32_t *at)
    {
        bool ok = l.empty();
        for (size_t k = 0; k < l.size() && !ok; k++) ok = at >= l[k].lo && at < l[k].hi;
        return ok;
    }
    /* ---- the global count table of cbc_stats_body.h: global_table() ----
     * While the driver has named it, every list_add must stay inside it. */
    static uint32_t *&gtab() { static thread_local uint32_t *t = nullptr; return t; }
    static uint32_t &gtab_words() { static thread_local uint32_t n = 0; return n; }
    static void global_table(uint32_t *p, uint32_t words) { gtab() = p; gtab_words() = words; }
    /* The coverage bodies need no operation of their own (the agent-scope atomic add is the policy's list_add); what lock-step
     * execution hides is that lanes of one list_add may name the same word, and the sum must not depend on their order: += into
     * a list in global memory, highest lane first (the base class goes lowest first): integer adds commute */
    static void list_add(uint32_t *p, const V32 &idx, const V32 &val, const Mask &m)
    {
        for (int i = 63; i >= 0; i--) {
            if (!m.b[i]) continue;
            if (gtab() != nullptr && (p != gtab() || idx.v[i] >= gtab_words())) { emu_oob("index outside the global count table"); continue; }
            if (!in_ranges(ranges(), p + idx.v[i])) { emu_oob("list_add outside the named tables"); continue; }
            p[idx.v[i]] += val.v[i];
        }
    }
    static void write_uni(uint32_t *p, uint32_t idx, uint32_t val)
    {
        if (!in_ranges(uni_ranges(), p + idx)) { emu_oob("write_uni outside the named tables"); return; }
        p[idx] = val;
    }

    /* ---- the workgroup's table in LDS: wg_table() ----
     * The accumulate body of cbc_hist_body.h is the first of the depth family to keep a table in LDS (the statistics, quantile
     * and alignment-table bodies follow it): here that table is a plain array per emulated workgroup, which the driver names
     * before it runs the workgroup, and every zero / add / read of it is checked against its length.  The adds go highest lane
     * first, like list_add: lanes may name the same word, and the sum must not depend on their order. */
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

    /* ---- the edit arena: edit_arena() ----
     * What the edit-reporting decoder (cbc_decode_body.h, EDITS = true) and the bodies behind it need beyond the rest are the
     * three 16-bit operations of the edit arena.  While the driver has named the arena, every 16-bit access must stay inside
     * it. */
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

    /* ---- the text: text_range() ----
     * While the driver of the SAM CIGAR / NM / MD bodies (cbc_cigar_body.h) has named the text, every byte and dword store must
     * fall inside it, and no byte of it may be stored twice (a line's fields, tokens and tags are disjoint). */
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
};

#endif
