/*
 * consensus_emu.cpp -- the bodies of cbc_gpu_decode_consensus (cbc_amd/csrc/cbc_consensus_body.h) on the CPU
 * through the lock-step wave emulation.  TEST AID ONLY: the passes are run in the call's order -- zero, cbc_depth_mark, the plain
 * events, cbc_depth_tile and the scan (all the pileup's own), then the call count, the scan and the write -- behind the emulated
 * edits decoder of tests/pileup_emu, or on records, rows and arena entries the stand-alone program fabricates, under ASan-able host
 * code before anything runs on a GPU.  Every table is an allocation of exactly its size and named to the emulation, so an index
 * past one is a finding, and the text is named too: a byte stored twice or outside it is one.  With -DCONSENSUS_EMU_MAIN the file
 * is a stand-alone program that builds the fabricated reads of tests/pileup_emu's check, applies the rule position by position in
 * a host loop and exits non-zero on a mismatch (make asan_check).
 */
#include "../emu/post_emu.h"
#include "../../cbc_amd/csrc/cbc_consensus_body.h"

/* ONE cbc_gpu_decode_consensus behind the decode.  out[0] = text bytes (also when text_cap is too small: CBC_E_ARG; tile 0 has
 * then still written the header where that fits -- it does so before it looks at the record's size -- and no byte of the body;
 * harmless on the device, whose host side copies nothing back in that case), out[1] = reads kept, out[2 .. 9] = emitted, ref, alt, del, ambiguous, low_depth, no_call, ins_skipped.
 * CBC_E_BLOCK (after the text of the other blocks) when a block of the call failed.  n_waves wavefronts share a block in the
 * events pass. */
extern "C" __attribute__((visibility("default")))
int emu_consensus(const cbc_read_rec *recs, uint64_t n_recs, const uint8_t *seq, uint64_t seq_bytes, const cbc_dec_block_desc *blocks,
                  const uint64_t *window_start, const cbc_block_result *dec_results, uint32_t n_blocks, const uint32_t *side,
                  const uint16_t *arena, uint32_t per_read, const uint8_t *ref, uint64_t ref_bytes, uint64_t ref_c0, const char *name,
                  uint32_t name_len, uint64_t beg, uint64_t end, uint32_t exclude, uint32_t min_depth, uint32_t ppm, uint32_t line_width,
                  uint32_t flags, uint32_t with_range, uint32_t n_waves, uint8_t *text, uint64_t text_cap, uint64_t *out)
{
    g_emu_errors = 0;
    for (int i = 0; i < 10; i++) out[i] = 0;
    if (beg < 1 || beg > end || end > CBC_SAM_MAX_POS || n_waves < 1u || n_waves > 16u || min_depth < 1u || ppm < 1u || ppm > 1000000u ||
        line_width < 1u || line_width > 65535u || (flags & ~7u) || with_range > 1u)
        return CBC_E_ARG;
    const uint64_t d_words = end - beg + 2u;
    const uint32_t n_tiles = (uint32_t)((d_words + CBC_DEPTH_TILE - 1u) / CBC_DEPTH_TILE);
    const size_t plane = (size_t)n_tiles * CBC_DEPTH_TILE;
    std::vector<uint32_t> diff(plane, 0u), tab(plane * CBC_PILEUP_PLANES, 0u), ctr(4, 0u), cctr(CBC_CONS_CTRS, 0u);
    std::vector<cbc_block_result> tile_sum(n_tiles), tile_cnt(n_tiles), counts(n_tiles);
    std::vector<uint64_t> sum_off(n_tiles + 1u, 0u), offsets(n_tiles + 1u, 0u);
    std::vector<uint8_t> dname(name, name + name_len);
    cbc_consensus_args C;
    memset(&C, 0, sizeof C);
    cbc_pileup_args &A = C.P;
    cbc_region_args &R = A.D.R;
    R.recs = recs; R.seq = seq; R.blocks = blocks; R.window_start = window_start; R.dec_results = dec_results;
    R.counts = counts.data(); R.offsets = offsets.data(); R.text = text; R.text_cap = text_cap;
    R.n_recs = n_recs; R.seq_bytes = seq_bytes; R.beg = beg; R.end = end; R.n_blocks = n_blocks;
    A.D.diff = diff.data(); A.D.diff_words = diff.size(); A.D.tile_sum = tile_sum.data(); A.D.tile_cnt = tile_cnt.data();
    A.D.sum_off = sum_off.data(); A.D.cnt_off = sum_off.data(); A.D.ctr = ctr.data(); A.D.name = dname.data();
    A.D.name_len = name_len; A.D.exclude = exclude; A.D.n_tiles = n_tiles; A.D.n_ttiles = n_tiles;
    A.side = side; A.arena = arena; A.arena_entries = n_recs * per_read; A.per_read = per_read;
    A.ref = ref; A.ref_bytes = ref_bytes; A.ref_c0 = ref_c0; A.tab = tab.data(); A.plane = plane; A.min_alt = 1u;
    C.cctr = cctr.data(); C.min_depth = min_depth; C.ppm = ppm; C.line_width = line_width; C.flags = flags; C.with_range = with_range;
    WP::clear_ranges();
    WP::add_range(diff.data(), d_words);                             /* the window's own words only */
    for (uint32_t k = 0; k < CBC_PILEUP_PLANES; k++) WP::add_range(tab.data() + (size_t)k * plane, d_words - 1u);
    WP::add_range(ctr.data(), 2);
    WP::add_range(cctr.data(), CBC_CONS_CTRS);
    WP::edit_arena(arena, A.arena_entries);
    for (uint32_t b = 0; b < n_blocks; b++) cbc_depth_mark<WP>(A.D, b);
    for (uint32_t b = 0; b < n_blocks; b++)
        for (uint32_t w = 0; w < n_waves; w++) cbc_pileup_events<WP>(A, b, w, n_waves);
    for (uint32_t t = 0; t < n_tiles; t++) cbc_depth_tile<WP>(A.D, t);
    for (uint32_t t = 0; t < n_tiles; t++) sum_off[t + 1u] = sum_off[t] + tile_sum[t].nbytes;
    for (uint32_t t = 0; t < n_tiles; t++) cbc_consensus_count<WP>(C, t);
    scan(counts.data(), offsets.data(), n_tiles);
    const uint64_t e = offsets[n_tiles];
    out[0] = cbc_consensus_hdr_len(C) + e + (e + line_width - 1u) / line_width;
    out[1] = ctr[0]; out[2] = e;
    for (uint32_t k = 0; k < CBC_CONS_CTRS; k++) out[3u + k] = cctr[k];
    WP::text_range(text, text_cap);
    for (uint32_t t = 0; t < n_tiles; t++) cbc_consensus_write<WP>(C, t);
    if (out[0] <= text_cap) {                                        /* every byte of the record written, exactly once */
        for (uint64_t i = 0; i < out[0]; i++) if (!WP::tx_seen()[(size_t)i]) { emu_oob("a byte of the record was not written"); break; }
    }
    WP::text_range(nullptr, 0);
    WP::clear_ranges();
    WP::edit_arena(nullptr, 0);
    if (g_emu_errors) return -100;
    if (out[0] > text_cap) return CBC_E_ARG;
    for (uint32_t b = 0; b < n_blocks; b++) if (dec_results[b].status != CBC_ST_OK) return CBC_E_BLOCK;
    return 0;
}

#ifdef CONSENSUS_EMU_MAIN
#include "../emu/fab_reads.h"
/* ---- the stand-alone check: fabricated records, rows and arena entries against the rule applied in a host loop ---------------- */
struct opt { uint32_t exclude, min_depth, ppm, width, flags, with_range, n_waves; int fail_block; };

static bool reaches(uint64_t x, uint64_t depth, uint32_t ppm) { return x * 1000000ull >= (uint64_t)ppm * depth; }

static std::string want_text(const fab &f, const std::string &name, uint64_t beg, uint64_t end, const opt &o, const tables &T, uint64_t *cnt)
{
    std::string body;
    for (int k = 0; k < 8; k++) cnt[k] = 0;
    for (uint64_t p = beg; p <= end; p++) {
        const size_t i = (size_t)(p - beg);
        const uint8_t rb = p - 1u < f.ref.size() ? f.ref[p - 1u] : (uint8_t)'N';
        const uint64_t depth = T.depth[i], d = T.del[i];
        uint64_t c[5], mis = 0;
        for (uint32_t k = 0; k < 5u; k++) { c[k] = k != klass(rb) ? T.cnt[k][i] : 0u; mis += c[k]; }
        c[klass(rb)] = depth - d - mis;                              /* as the device: the reference's class takes what the others leave */
        if (depth >= o.min_depth && reaches(T.ins[i], depth, o.ppm)) cnt[7]++;
        if (depth < o.min_depth) {
            uint8_t b = 'N';
            if (o.flags & CBC_CONS_FILL_REF) b = ((rb & 0xdfu) >= 'A' && (rb & 0xdfu) <= 'Z') ? (uint8_t)(rb | 0x20u) : rb;
            body.push_back((char)b); cnt[5]++;
            continue;
        }
        const uint64_t cand[5] = { c[0], c[1], c[2], c[3], d };
        uint64_t top = 0;
        for (int k = 0; k < 5; k++) if (cand[k] > top) top = cand[k];
        int w = -1;
        if (klass(rb) < 4u && cand[klass(rb)] == top) w = (int)klass(rb);
        for (int k = 0; w < 0 && k < 5; k++) if (cand[k] == top) w = k;
        if (reaches(top, depth, o.ppm)) {
            if (w == 4) { cnt[3]++; if (o.flags & CBC_CONS_SHOW_DEL) body.push_back('*'); }
            else { body.push_back("ACGT"[w]); cnt[(uint32_t)w == klass(rb) ? 1 : 2]++; }
            continue;
        }
        uint64_t bt = 0; uint32_t bs = 0;
        for (int k = 0; (o.flags & CBC_CONS_IUPAC) && k < 4; k++) {
            if (c[k] == 0u || c[k] <= bt) continue;
            uint64_t sum = 0; uint32_t set = 0;
            for (int j = 0; j < 4; j++) if (c[j] >= c[k]) { sum += c[j]; set |= 1u << j; }
            if (reaches(sum, depth, o.ppm)) { bt = c[k]; bs = set; }
        }
        if (bt) { body.push_back("NACMGRSVTWYHKDBN"[bs]); cnt[4]++; }
        else { body.push_back('N'); cnt[6]++; }
    }
    cnt[0] = body.size();
    char hdr[512];
    if (o.with_range) snprintf(hdr, sizeof hdr, ">%s:%llu-%llu\n", name.c_str(), (unsigned long long)beg, (unsigned long long)end);
    else snprintf(hdr, sizeof hdr, ">%s\n", name.c_str());
    std::string out = hdr;
    for (size_t i = 0; i < body.size(); i += o.width) { out += body.substr(i, o.width); out += "\n"; }
    return out;
}

static int fab_check(const char *what, const fab &f, uint64_t beg, uint64_t end, const opt &o, const std::string &name = "ctg")
{
    fab_arrays a;
    if (!fab_build(f, a, o.fail_block)) { printf("%-72s BAD FIXTURE\n", what); return 1; }
    tables T;
    want_tables(f, beg, end, o.exclude, a.failed, T);
    uint64_t cnt[8];
    const std::string want = want_text(f, name, beg, end, o, T, cnt);
    std::vector<uint8_t> text(want.size() + 16u, 0xEEu);
    uint64_t out[10];
    auto call = [&](uint8_t *t, uint64_t cap) {
        return emu_consensus(a.recs.data(), f.reads.size(), a.rows.data(), a.rows.size(), a.blocks.data(), a.ws.data(), a.res.data(),
                             (uint32_t)a.blocks.size(), a.side.data(), a.arena.data(), f.per_read, f.ref.data(), f.ref.size(), 0u, name.c_str(),
                             (uint32_t)name.size(), beg, end, o.exclude, o.min_depth, o.ppm, o.width, o.flags, o.with_range, o.n_waves, t, cap, out);
    };
    const int rc = call(text.data(), want.size());
    int bad = rc != (o.fail_block >= 0 ? CBC_E_BLOCK : 0) || out[0] != want.size() || out[1] != T.kept || memcmp(text.data(), want.data(), want.size()) != 0;
    for (int k = 0; k < 8; k++) bad |= out[2 + k] != cnt[k];
    for (size_t i = want.size(); i < text.size(); i++) bad |= text[i] != 0xEEu;
    printf("%-72s %s (rc %d, %llu bytes, %llu emitted, %llu reads)\n", what, bad ? "MISMATCH" : "ok", rc, (unsigned long long)out[0],
           (unsigned long long)out[2], (unsigned long long)out[1]);
    if (!bad) {                                                      /* one byte short: the size reported, the header at most written (see emu_consensus) */
        std::vector<uint8_t> t2(want.size() + 16u, 0xEEu);
        const int rc2 = call(t2.data(), want.size() - 1u);
        const size_t hdr = want.find('\n') + 1u;
        bad |= rc2 != CBC_E_ARG || out[0] != want.size();
        for (size_t i = hdr; i < t2.size(); i++) bad |= t2[i] != 0xEEu;
        if (bad) printf("%-72s MISMATCH (text_cap one byte short: rc %d)\n", what, rc2);
    }
    return bad;
}

int main()
{
    int bad = 0;
    g_rng = 2463534242u;
    fab f;
    uint32_t pos;
    fab_pileup_cases(f, pos);
    const uint64_t last = pos + 160u;
    if (last > f.ref.size()) { printf("BAD FIXTURE: the reference is too short\n"); return 1; }
    const opt def = { 0u, 1u, 750000u, 60u, 0u, 0u, 4u, -1 };
    bad |= fab_check("every case, whole window, the defaults", f, 1u, last, def);
    for (uint32_t w : { 1u, 2u, 7u, 63u, 64u, 65u, 65535u }) {
        opt o = def; o.width = w; o.flags = w & 7u; o.with_range = w & 1u;
        char what[96];
        snprintf(what, sizeof what, "line width %u, flags %u", w, o.flags);
        bad |= fab_check(what, f, 1u, last, o);
    }
    for (uint32_t fl = 0; fl < 8u; fl++) {
        opt o = def; o.flags = fl; o.ppm = fl & 1u ? 500000u : 1000000u; o.min_depth = 1u + fl % 3u; o.exclude = fl & 2u ? 16u : 0u; o.n_waves = 1u + fl % 4u;
        char what[96];
        snprintf(what, sizeof what, "flags %u, ppm %u, min depth %u, exclude %u", fl, o.ppm, o.min_depth, o.exclude);
        bad |= fab_check(what, f, 1u, last, o);
    }
    { opt o = def; o.with_range = 1u; o.flags = 7u; bad |= fab_check("a window of more than one tile, with its range", f, 3u, 6000u, o); }
    { opt o = def; o.fail_block = 3; bad |= fab_check("a failed block", f, 1u, last, o); }
    { opt o = def; o.with_range = 1u; bad |= fab_check("one position", f, 40u, 40u, o); }
    {   /* a window inside a deletion every read carries: the header alone; and the three ties */
        fab g; g.stride = 16u; g.per_read = 4u;
        g.ref.assign(64u, 'A');
        for (uint32_t i = 0; i < 4u; i++) { fab_read(g, 3u, 0u, 8u, vu{ 4u, 4u, 4u }, vu()); g.reads.back().seq = i < 2u ? "AAAACCCC" : "AAAAGGTC"; }
        g.block_n.push_back(4u);
        opt o = def; o.with_range = 1u;
        bad |= fab_check("a window inside a shared deletion: the header alone", g, 7u, 9u, o);
        o.flags = CBC_CONS_SHOW_DEL; o.width = 3u;
        bad |= fab_check("the same with show-del: exactly one line", g, 7u, 9u, o);
        o.flags = CBC_CONS_IUPAC; o.ppm = 750000u; o.width = 60u;
        bad |= fab_check("ties and two-base sets", g, 1u, 20u, o);
        bad |= fab_check("a 255-byte name, the last position of the coordinate", g, 2147483000u, 2147483647u, o, std::string(255u, 'n'));
    }
    if (g_emu_errors) bad = 1;
    printf(bad ? "CONSENSUS EMU CHECK FAILED\n" : "CONSENSUS EMU CHECK OK\n");
    return bad;
}
#endif
