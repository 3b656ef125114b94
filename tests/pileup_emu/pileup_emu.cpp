/*
 * pileup_emu.cpp -- the edit-reporting decoder (cbc_amd/csrc/cbc_decode_body.h, EDITS = true) and the pileup bodies
 * (cbc_amd/csrc/cbc_pileup_body.h) on the CPU through the lock-step wave emulation.  TEST AID ONLY: the passes of
 * cbc_gpu_decode_pileup are run in its order -- zero, cbc_depth_mark, events, cbc_depth_tile, the scan, count, the scan, write --
 * behind the emulated decoder, or on records, rows and arena entries the stand-alone program fabricates, under ASan-able host
 * code before anything runs on a GPU.  Every table is an allocation of exactly its size and named to the emulation, so an index
 * past one is a finding.  With -DPILEUP_EMU_MAIN the file is a stand-alone program that builds the fabricated cases itself,
 * compares them with a base-by-base host loop and exits non-zero on a mismatch (make asan_check).
 */
#include "../emu/post_emu.h"

/* the edit-reporting decoder over every block of the batch: side = 2 * n_recs words, arena = n_recs * per_read entries exactly */
extern "C" __attribute__((visibility("default")))
int emu_pileup_decode(const cbc_dec_device_batch *b, uint32_t smax, uint32_t per_read, uint32_t *side, uint16_t *arena)
{ return emu_decode_blocks<WP, true, true>(b, smax, per_read, side, arena); }

/* ONE cbc_gpu_decode_pileup behind the decode: the plain bodies through the driver of tests/emu/post_emu.h.  out[0] = text bytes
 * (also when text_cap is too small: CBC_E_ARG, nothing written), out[1] = lines, out[2] = reads kept.  CBC_E_BLOCK (after the
 * text of the other blocks) when a block of the call failed.  n_waves wavefronts share a block in the events pass. */
extern "C" __attribute__((visibility("default")))
int emu_pileup(const cbc_read_rec *recs, uint64_t n_recs, const uint8_t *seq, uint64_t seq_bytes, const cbc_dec_block_desc *blocks,
               const uint64_t *window_start, const cbc_block_result *dec_results, uint32_t n_blocks, const uint32_t *side,
               const uint16_t *arena, uint32_t per_read, const uint8_t *ref, uint64_t ref_bytes, uint64_t ref_c0, const char *name,
               uint32_t name_len, uint64_t beg, uint64_t end, uint32_t exclude, uint32_t min_alt, uint32_t n_waves, uint8_t *text,
               uint64_t text_cap, uint64_t *out)
{
    return emu_pileup_call(recs, n_recs, seq, seq_bytes, blocks, window_start, dec_results, n_blocks, side, arena, per_read, ref, ref_bytes, ref_c0,
                           name, name_len, beg, end, exclude, min_alt, 0u, 0u, n_waves, 0u, 0u, text, text_cap, out);
}

#ifdef PILEUP_EMU_MAIN
#include "../emu/fab_reads.h"
/* ---- the stand-alone check: fabricated records, rows and arena entries against a base-by-base host loop ---------------------- */
static std::string want_text(const fab &f, const std::string &name, uint64_t beg, uint64_t end, uint32_t min_alt, const tables &T, uint64_t &lines)
{
    std::string out;
    lines = 0;
    for (uint64_t p = beg; p <= end; p++) {
        const size_t i = (size_t)(p - beg);
        const uint8_t rb = f.ref[p - 1u];
        uint64_t mis = 0, c[5];
        for (uint32_t k = 0; k < 5u; k++) { c[k] = T.cnt[k][i]; if (k != klass(rb)) mis += c[k]; }
        /* the device's view: depth is the span depth, the reference's class takes what the others leave */
        c[klass(rb)] = T.depth[i] - T.del[i] - mis;
        if (mis + T.del[i] + T.ins[i] < min_alt) continue;
        char buf[512];
        snprintf(buf, sizeof buf, "%s\t%llu\t%c\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\t%llu\n", name.c_str(), (unsigned long long)p, rb,
                 (unsigned long long)(uint32_t)T.depth[i], (unsigned long long)(uint32_t)c[0], (unsigned long long)(uint32_t)c[1], (unsigned long long)(uint32_t)c[2],
                 (unsigned long long)(uint32_t)c[3], (unsigned long long)(uint32_t)c[4], (unsigned long long)T.del[i], (unsigned long long)T.ins[i]);
        out += buf; lines++;
    }
    return out;
}

/* arena_short: entries taken off the LAST non-empty block's arena need (0: exactly the needed size per block) */
static int fab_check(const char *what, const fab &f, uint64_t beg, uint64_t end, uint32_t exclude, uint32_t min_alt, uint32_t n_waves,
                     int fail_block = -1)
{
    const std::string name = "ctg";
    fab_arrays a;
    if (!fab_build(f, a, fail_block)) { printf("%-66s BAD FIXTURE\n", what); return 1; }
    tables T;
    want_tables(f, beg, end, exclude, a.failed, T);
    uint64_t lines = 0;
    const std::string want = want_text(f, name, beg, end, min_alt, T, lines);
    std::vector<uint8_t> text(want.size() + 16u, 0xEEu);
    uint64_t out[4] = { 0, 0, 0, 0 };
    auto call = [&](uint8_t *t, uint64_t cap) {
        return emu_pileup(a.recs.data(), f.reads.size(), a.rows.data(), a.rows.size(), a.blocks.data(), a.ws.data(), a.res.data(), (uint32_t)a.blocks.size(),
                          a.side.data(), a.arena.data(), f.per_read, f.ref.data(), f.ref.size(), 0u, name.c_str(), (uint32_t)name.size(), beg, end,
                          exclude, min_alt, n_waves, t, cap, out);
    };
    const int rc = call(text.data(), want.size());
    int bad = rc != (fail_block >= 0 ? CBC_E_BLOCK : 0) || out[0] != want.size() || out[1] != lines || out[2] != T.kept ||
              memcmp(text.data(), want.data(), want.size()) != 0;
    for (size_t i = want.size(); i < text.size(); i++) bad |= text[i] != 0xEEu;
    printf("%-66s %s (rc %d, %llu lines, %llu reads)\n", what, bad ? "MISMATCH" : "ok", rc, (unsigned long long)out[1], (unsigned long long)out[2]);
    if (!bad && want.size() > 0) bad |= fab_short_probe(what, 66, call, want.size(), out);
    return bad;
}

int main()
{
    int bad = 0;
    fab f;
    uint32_t pos;
    fab_pileup_cases(f, pos);
    const uint64_t last = pos + 160u;
    if (last > f.ref.size()) { printf("BAD FIXTURE: the reference is too short\n"); return 1; }
    bad |= fab_check("every case, whole window, one wavefront per block", f, 1u, last, 0u, 1u, 1u);
    bad |= fab_check("every case, whole window, four wavefronts per block", f, 1u, last, 0u, 1u, 4u);
    bad |= fab_check("min_alt 2, exclude 16, three wavefronts", f, 1u, last, 16u, 2u, 3u);
    bad |= fab_check("min_alt above every depth: empty", f, 1u, last, 0u, 100000u, 4u);
    bad |= fab_check("exclude 0xffff keeps the FLAG 0 reads", f, 1u, last, 0xffffu, 1u, 4u);
    bad |= fab_check("a failed block", f, 1u, last, 0u, 1u, 4u, 3);
    /* windows that start and end inside a read, inside its deleted bases, and on an insertion's anchor */
    const fread_ &r2 = f.reads[f.reads.size() - 9u];
    for (size_t i = 0; i < f.reads.size(); i += 5u) {
        const fread_ &r = f.reads[i];
        char what[96];
        snprintf(what, sizeof what, "window inside read %zu", i);
        bad |= fab_check(what, f, r.pos + 1u, r.pos + (r.span > 2u ? r.span - 2u : 1u), 0u, 1u, 2u);
        if (!r.dc.empty()) { snprintf(what, sizeof what, "window on the deleted bases of read %zu", i); bad |= fab_check(what, f, r.pos + r.dc[0], r.pos + r.dc[0], 0u, 1u, 4u); }
        if (!r.oi.empty() && r.oi[0] > 0u) {
            snprintf(what, sizeof what, "window ends on / starts behind the anchor of read %zu", i);
            bad |= fab_check(what, f, 1u, r.pos + r.oi[0] - 1u, 0u, 1u, 4u);
            bad |= fab_check(what, f, r.pos + r.oi[0], last, 0u, 1u, 4u);
        }
    }
    bad |= fab_check("one position", f, r2.pos, r2.pos, 0u, 1u, 4u);
    bad |= fab_check("a window of more than one tile", f, 1u, 6000u, 0u, 1u, 4u);
    {   /* counters: 300 reads at one place, all mismatching, one deletion and one insertion each */
        fab g; g.stride = 8u; g.per_read = 2u;
        g.ref.assign(64u, 'A');
        for (uint32_t i = 0; i < 300u; i++) { fab_read(g, 3u, 0u, 6u, vu{ 2u }, vu{ 4u }); g.reads.back().seq = "CCGGTT"; }
        g.block_n.push_back(300u);
        bad |= fab_check("300 reads on one position: an arena of exactly the needed size", g, 1u, 40u, 0u, 1u, 4u);
    }
    if (g_emu_errors) bad = 1;
    printf(bad ? "PILEUP EMU CHECK FAILED\n" : "PILEUP EMU CHECK OK\n");
    return bad;
}
#endif
