/*
 * cigar_emu.cpp -- the edit-reporting decoder (cbc_amd/csrc/cbc_decode_body.h, EDITS = true) and the SAM CIGAR / NM / MD bodies
 * (cbc_amd/csrc/cbc_cigar_body.h) on the CPU through the lock-step wave emulation.  TEST AID ONLY: the passes of
 * cbc_gpu_decode_sam_cigar are run in its order -- measure, count, the scan, write -- behind the emulated decoder, or on records,
 * rows and arena entries the stand-alone program fabricates, under ASan-able host code before anything runs on a GPU.  Every
 * table is an allocation of exactly its size and named to the emulation, so an index past one is a finding.  With
 * -DCIGAR_EMU_MAIN the file is a stand-alone program that builds the fabricated cases itself, compares them with an
 * element-by-element host loop and exits non-zero on a mismatch (make asan_check).
 */
#include "../emu/post_emu.h"
#include "../../cbc_amd/csrc/cbc_cigar_body.h"

/* the edit-reporting decoder over every block of the batch: side = 2 * n_recs words, arena = n_recs * per_read entries exactly */
extern "C" __attribute__((visibility("default")))
int emu_cigar_decode(const cbc_dec_device_batch *b, uint32_t smax, uint32_t per_read, uint32_t *side, uint16_t *arena)
{ return emu_decode_blocks<WP, true, true>(b, smax, per_read, side, arena); }

/* ONE cbc_gpu_decode_sam_cigar behind the decode.  out[0] = text bytes (also when text_cap is too small: CBC_E_ARG, nothing
 * written), out[1] = reads.  CBC_E_BLOCK (after the text of the other blocks) when a block of the call failed.  n_waves
 * wavefronts share a block in the measure and in the write pass. */
extern "C" __attribute__((visibility("default")))
int emu_sam_cigar(const cbc_read_rec *recs, uint64_t n_recs, const uint8_t *seq, uint64_t seq_bytes, const cbc_dec_block_desc *blocks,
                  const uint64_t *window_start, const cbc_block_result *dec_results, uint32_t n_blocks, const uint32_t *block_name,
                  const uint8_t *names, uint32_t names_bytes, int region, uint64_t beg, uint64_t end, const uint32_t *side,
                  const uint16_t *arena, uint32_t per_read, const uint8_t *ref, uint64_t ref_bytes, uint32_t n_waves, uint8_t *text,
                  uint64_t text_cap, uint64_t *out)
{
    g_emu_errors = 0;
    out[0] = out[1] = 0;
    if (n_waves < 1u || n_waves > 16u) return CBC_E_ARG;
    std::vector<cbc_block_result> counts(n_blocks ? n_blocks : 1u);
    std::vector<uint64_t> offsets(n_blocks + 1u, 0u);
    std::vector<uint32_t> meas((size_t)(n_recs ? n_recs : 1u) * 2u, 0xEEEEEEEEu);
    cbc_cigar_args A;
    memset(&A, 0, sizeof A);
    cbc_region_args &R = A.S.R;
    R.recs = recs; R.seq = seq; R.blocks = blocks; R.window_start = window_start; R.dec_results = dec_results;
    R.counts = counts.data(); R.offsets = offsets.data(); R.text = text; R.text_cap = text_cap;
    R.n_recs = n_recs; R.seq_bytes = seq_bytes; R.beg = region ? beg : 1u; R.end = region ? end : UINT64_MAX; R.n_blocks = n_blocks;
    A.S.block_name = block_name; A.S.names = names; A.S.names_bytes = names_bytes; A.S.region = region ? 1u : 0u;
    A.side = side; A.arena = arena; A.ref = ref; A.meas = meas.data();
    A.arena_entries = n_recs * per_read; A.ref_bytes = ref_bytes; A.per_read = per_read;
    WP::clear_ranges();
    WP::add_range(meas.data(), n_recs * 2u); WP::add_uni_range(meas.data(), n_recs * 2u);
    WP::add_range((const uint32_t *)counts.data(), (uint64_t)n_blocks * 4u); WP::add_uni_range((const uint32_t *)counts.data(), (uint64_t)n_blocks * 4u);
    WP::edit_arena(arena, A.arena_entries);
    for (uint32_t b = 0; b < n_blocks; b++)
        for (uint32_t w = 0; w < n_waves; w++) cbc_cigar_measure<WP>(A, b, w, n_waves);
    for (uint32_t b = 0; b < n_blocks; b++) cbc_sam_cigar_count<WP>(A, b);
    for (uint32_t b = 0; b < n_blocks; b++) { offsets[b + 1u] = offsets[b] + counts[b].nbytes; out[1] += counts[b].n_symbols; }
    out[0] = offsets[n_blocks];
    int rc = 0;
    if (out[0] > text_cap) rc = CBC_E_ARG;
    else {
        WP::text_range(text, out[0]);
        for (uint32_t b = 0; b < n_blocks; b++)
            for (uint32_t w = 0; w < n_waves; w++) cbc_sam_cigar_write<WP>(A, b, w, n_waves);
        for (size_t i = 0; i < WP::tx_seen().size(); i++) if (!WP::tx_seen()[i]) { emu_oob("a byte of the text is not written"); break; }
        WP::text_range(nullptr, 0);
    }
    WP::clear_ranges();
    WP::edit_arena(nullptr, 0);
    if (g_emu_errors) return -100;
    if (rc) return rc;
    for (uint32_t b = 0; b < n_blocks; b++) if (dec_results[b].status != CBC_ST_OK) return CBC_E_BLOCK;
    return 0;
}

#ifdef CIGAR_EMU_MAIN
#include "../emu/fab_reads.h"
/* ---- the stand-alone check: fabricated records, rows and arena entries against an element-by-element host loop --------------- */
/* the semantics of include/cbc_gpu.h, one element at a time; false: not what the decoder writes */
static bool host_tags(const fab &f, const fread_ &r, std::string &out)
{
    const uint32_t rl = (uint32_t)r.seq.size(), nd = (uint32_t)r.dc.size(), ni = (uint32_t)r.oi.size();
    if (rl == 0u || nd > 255u || ni > 255u || ni > rl) return false;
    const uint32_t T = rl - ni;
    for (uint32_t i = 0; i < nd; i++) if (r.dc[i] > T || (i && r.dc[i] < r.dc[i - 1u])) return false;
    for (uint32_t i = 0; i < ni; i++) if (r.oi[i] >= rl || (i && r.oi[i] <= r.oi[i - 1u])) return false;
    if ((uint64_t)r.pos - 1u + T + nd > f.ref.size()) return false;
    std::vector<bool> isins(rl, false);
    for (uint32_t o : r.oi) isins[o] = true;
    struct el { char k; uint32_t q, x; };
    std::vector<el> E;
    uint32_t q = 0, di = 0, x = 0;
    for (uint32_t m = 0; m <= T; m++) {
        while (q < rl && isins[q]) { E.push_back(el{ 'I', q, 0u }); q++; }
        while (di < nd && r.dc[di] == m) { E.push_back(el{ 'D', 0u, x++ }); di++; }
        if (m < T) { E.push_back(el{ 'M', q, x++ }); q++; }
    }
    if (q != rl || di != nd) return false;
    std::string cigar, md;
    uint32_t nm = 0, n = 0, aligned_seen = 0;
    for (size_t i = 0; i < E.size();) {
        size_t j = i;
        while (j < E.size() && E[j].k == E[i].k) j++;
        char op = E[i].k;
        if (op == 'I') {
            uint32_t after = 0;
            for (size_t k = j; k < E.size(); k++) after += E[k].k == 'M';
            if (aligned_seen == 0u || after == 0u) op = 'S'; else nm += (uint32_t)(j - i);
        }
        cigar += std::to_string(j - i) + op;
        if (op == 'D') {
            md += std::to_string(n) + "^"; n = 0; nm += (uint32_t)(j - i);
            for (size_t k = i; k < j; k++) md.push_back((char)f.ref[r.pos - 1u + E[k].x]);
        }
        if (op == 'M')
            for (size_t k = i; k < j; k++) {
                const uint8_t rb = f.ref[r.pos - 1u + E[k].x];
                aligned_seen++;
                if ((uint8_t)r.seq[E[k].q] == rb) n++;
                else { md += std::to_string(n); md.push_back((char)rb); n = 0; nm++; }
            }
        i = j;
    }
    md += std::to_string(n);
    out = cigar + "\t" + std::to_string(nm) + "\t" + md;
    return true;
}

static std::string sam_line(const fread_ &r, const std::string &name, const std::string &tags)
{
    std::string s = "*\t" + std::to_string(r.flag) + "\t" + name + "\t" + std::to_string(r.pos) + "\t255\t";
    if (tags.empty()) return s + "*\t*\t0\t0\t" + r.seq + "\t*\n";
    const size_t a = tags.find('\t'), b = tags.find('\t', a + 1u);
    return s + tags.substr(0, a) + "\t*\t0\t0\t" + r.seq + "\t*\tNM:i:" + tags.substr(a + 1u, b - a - 1u) + "\tMD:Z:" + tags.substr(b + 1u) + "\n";
}

static int fab_check(const char *what, fab &f, int region, uint64_t beg, uint64_t end, uint32_t n_waves, int fail_block = -1,
                     uint32_t fail_status = 2u)
{
    const std::string name = "ctg";
    const size_t nb = f.block_n.size();
    fab_arrays a;
    if (!fab_build(f, a, fail_block, fail_status)) { printf("%-66s BAD FIXTURE\n", what); return 1; }
    vu bn;
    for (size_t b = 0; b < nb; b++) { bn.push_back(0u); bn.push_back((uint32_t)name.size()); }
    std::string want;
    uint64_t kept = 0;
    size_t at = 0;
    for (size_t b = 0; b < nb; b++)
        for (uint32_t k = 0; k < f.block_n[b]; k++, at++) {
            const fread_ &r = f.reads[at];
            if ((int)b == fail_block) continue;
            if (region && (r.pos > end || (uint64_t)r.pos + r.span < beg + 1u)) continue;
            std::string tags;
            if (r.raw_cnt >= 0 || r.raw_e0 >= 0 || !host_tags(f, r, tags)) tags.clear();
            if (!r.want.empty() && r.want != tags) { printf("%-66s BAD FIXTURE: read %zu is %s, meant %s\n", what, at, tags.c_str(), r.want.c_str()); return 1; }
            want += sam_line(r, name, tags); kept++;
        }
    std::vector<uint8_t> text(want.size() + 16u, 0xEEu);
    uint64_t out[2] = { 0, 0 };
    auto call = [&](uint8_t *t, uint64_t cap) {
        return emu_sam_cigar(a.recs.data(), f.reads.size(), a.rows.data(), a.rows.size(), a.blocks.data(), a.ws.data(), a.res.data(), (uint32_t)nb, bn.data(),
                             (const uint8_t *)name.data(), (uint32_t)name.size(), region, beg, end, a.side.data(), a.arena.data(), f.per_read,
                             f.ref.data(), f.ref.size(), n_waves, t, cap, out);
    };
    const int rc = call(text.data(), want.size());
    int bad = rc != (fail_block >= 0 ? CBC_E_BLOCK : 0) || out[0] != want.size() || out[1] != kept || memcmp(text.data(), want.data(), want.size()) != 0;
    for (size_t i = want.size(); i < text.size(); i++) bad |= text[i] != 0xEEu;
    printf("%-66s %s (rc %d, %llu bytes, %llu reads)\n", what, bad ? "MISMATCH" : "ok", rc, (unsigned long long)out[0], (unsigned long long)out[1]);
    if (bad && out[0] == want.size()) {
        size_t i = 0;
        while (i < want.size() && text[i] == (uint8_t)want[i]) i++;
        size_t a = i; while (a > 0 && want[a - 1] != '\n') a--;
        size_t e = want.find('\n', i);
        printf("  want: %s\n  got:  %.*s\n", want.substr(a, e - a).c_str(), (int)(e - a), (const char *)text.data() + a);
    }
    if (!bad && want.size() > 0) bad |= fab_short_probe(what, 66, call, want.size(), out);
    return bad;
}

int main()
{
    int bad = 0;
    fab f; f.stride = 256u; f.per_read = 16u; f.on_ref = true;
    for (uint32_t i = 0; i < 9000u; i++) f.ref.push_back("ACGTNacgtnRYk"[rnd() % 13u]);    /* lower-case and IUPAC reference bytes */
    static const uint32_t lens[] = { 1, 63, 64, 65, 127, 128, 129, 150, 256 };
    uint32_t pos = 5;
    for (size_t i = 0; i < sizeof lens / sizeof lens[0]; i++) {
        const uint32_t L = lens[i];
        fab_read(f, pos += 7u, 0u, L, vu(), vu()).want = std::to_string(L) + "M\t0\t" + std::to_string(L);      /* perfect */
        fab_read(f, pos += 1u, 16u, L, vu(), vu(), vu{ 0u });                     /* mismatches at 0, 63, 64, rl - 1 */
        fab_read(f, pos += 1u, 0u, L, vu(), vu(), vu{ 63u });
        fab_read(f, pos += 1u, 0u, L, vu(), vu(), vu{ 64u });
        fab_read(f, pos += 1u, 0u, L, vu(), vu(), vu{ L - 1u });
        fab_read(f, pos += 1u, 0u, L, vu(), vu(), vu{ 0u, 63u, 64u, L - 1u });
        fab_read(f, pos += 1u, 0u, L, vu(), vu(), vu{ 9u, 20u, 120u, 221u });     /* match runs of 9, 10, 99, 100 bases */
        fab_read(f, pos += 1u, 0u, L, vu(), vu(), vu{ 30u, 31u });                /* two adjacent mismatches */
        fab_read(f, pos += 1u, 16u, L, vu{ 0u }, vu());                           /* a deletion before the first base */
        fab_read(f, pos += 1u, 0u, L, vu{ L }, vu());                             /* one after the last, at matched coordinate T */
        fab_read(f, pos += 1u, 16u, L, vu{ L / 2u, L / 2u }, vu());               /* two deletions at one coordinate */
        fab_read(f, pos += 1u, 0u, L, vu(), vu{ 0u });                            /* an insertion run at read index 0: S */
        fab_read(f, pos += 1u, 1024u, L, vu(), vu{ L - 1u });                     /* and one at rl - 1: S */
        if (L >= 65u) {
            fab_read(f, pos += 1u, 0u, L, vu{ 64u }, vu());                       /* a deletion at coordinate 64 */
            fab_read(f, pos += 1u, 0u, L, vu{ 2u, 2u }, vu(), vu{ 2u });          /* a mismatch directly behind a deletion: ^xx0y */
            fab_read(f, pos += 1u, 0u, L, vu(), vu{ 0u, 1u, L - 2u, L - 1u });    /* both clips in one read */
            fab_read(f, pos += 1u, 0u, L, vu(), vu{ 30u, 31u, 32u });             /* an I run in the middle */
            fab_read(f, pos += 1u, 0u, L, vu{ 40u, 40u }, vu{ 40u, 41u, 42u });   /* a run directly in front of a deletion: 40M3I2D */
            fab_read(f, pos += 1u, 16u, L, vu{ 1u, 3u, 3u }, vu{ 0u, 1u, 62u, 63u, 64u, L - 2u, L - 1u }, vu{ 5u, 70u });
        }
        vu all; for (uint32_t q = 0; q < L; q++) all.push_back(q);
        if (L <= 129u) {
            fab_read(f, pos += 1u, 0u, L, vu{ 0u, 0u }, all);                     /* nothing but insertions over two deleted bases: <rl>S2D */
            fab_read(f, pos += 1u, 0u, L, vu(), all).want = std::to_string(L) + "S\t0\t0";
        }
    }
    pos += 1u;
    fab_read(f, pos, 0u, 100u, vu{ 40u, 40u }, vu{ 40u, 41u, 42u }).want = "40M3I2D57M\t5\t40^" + std::string(1, (char)f.ref[pos - 1u + 40u]) + std::string(1, (char)f.ref[pos - 1u + 41u]) + "57";
    fab_read(f, pos += 1u, 0u, 100u, vu(), vu{ 0u, 1u, 2u, 3u, 94u, 95u, 96u, 97u, 98u, 99u }).want = "4S90M6S\t0\t90";
    fab_read(f, pos += 1u, 0u, 100u, vu(), vu{ 95u, 96u, 97u, 98u, 99u }).want = "95M5S\t0\t95";
    /* not what the decoder writes: the plain line */
    fab_read(f, pos += 1u, 0u, 50u, vu(), vu()).raw_cnt = 256;                     /* nDel above 255 */
    fab_read(f, pos += 1u, 0u, 50u, vu(), vu()).raw_cnt = 256 << 16;               /* nIns above 255 */
    { fread_ &r = fab_read(f, pos += 1u, 0u, 50u, vu(), vu()); r.raw_cnt = 2; r.raw_e0 = 1 << 20; }      /* entries outside the block's arena */
    fab_read(f, pos += 1u, 0u, 50u, vu{ 5u, 3u }, vu()).want = "";                 /* dc descending */
    fab_read(f, pos += 1u, 0u, 50u, vu{ 51u }, vu());                              /* dc above T */
    fab_read(f, pos += 1u, 0u, 50u, vu(), vu{ 3u, 3u });                           /* oi not strictly ascending */
    fab_read(f, pos += 1u, 0u, 50u, vu(), vu{ 50u });                              /* oi >= rl */
    fab_read(f, pos += 1u, 0u, 0u, vu(), vu());                                    /* rl = 0 */
    while (f.reads.size() < 0u + 1u + 63u + 64u + 65u + 40u) fab_read(f, pos += 3u, (rnd() & 1u) * 16u, 100u, rnd() % 3u ? vu() : vu{ 40u, 40u, 41u }, rnd() % 4u ? vu() : vu{ 10u, 11u, 50u }, rnd() % 2u ? vu() : vu{ rnd() % 100u, rnd() % 100u });
    {
        const uint32_t sizes[] = { 0, 1, 63, 64, 65 };
        uint32_t at = 0;
        for (int i = 0; i < 5; i++) { f.block_n.push_back(sizes[i]); at += sizes[i]; }
        f.block_n.push_back((uint32_t)f.reads.size() - at);
    }
    if (pos + 600u > f.ref.size()) { printf("BAD FIXTURE: the reference is too short\n"); return 1; }
    bad |= fab_check("every case, whole file, one wavefront per block", f, 0, 0u, 0u, 1u);
    bad |= fab_check("every case, whole file, four wavefronts per block", f, 0, 0u, 0u, 4u);
    bad |= fab_check("a failed block", f, 0, 0u, 0u, 4u, 3);
    bad |= fab_check("a block that failed with CBC_ST_EDITS", f, 0, 0u, 0u, 4u, 5, CBC_ST_EDITS);
    for (size_t i = 0; i < f.reads.size(); i += 9u) {                /* a region window cutting through reads */
        const fread_ &r = f.reads[i];
        char what[96];
        snprintf(what, sizeof what, "region inside read %zu", i);
        bad |= fab_check(what, f, 1, r.pos + 1u, r.pos + 2u, 2u);
        if (!r.dc.empty()) { snprintf(what, sizeof what, "region on the deleted bases of read %zu", i); bad |= fab_check(what, f, 1, r.pos + r.dc[0], r.pos + r.dc[0], 4u); }
    }
    {   /* long lists: a deletion run of 70 bases, 70 inserted bases, 200 + 40 entries in one read; an arena of exactly the needed size */
        fab g; g.stride = 256u; g.per_read = 117u; g.on_ref = true; g.ref = f.ref;               /* 70 + 70 + 240 + 88 = 4 * 117 entries */
        vu d70(70u, 100u), d200, i70, i40;
        for (uint32_t i = 0; i < 200u; i++) d200.push_back(10u + i / 2u);
        for (uint32_t i = 0; i < 70u; i++) i70.push_back(60u + i);
        for (uint32_t i = 0; i < 40u; i++) i40.push_back(3u * i + 5u);
        fab_read(g, 10u, 0u, 200u, d70, vu(), vu{ 100u });
        fab_read(g, 20u, 0u, 250u, vu(), i70, vu{ 3u, 200u });
        fab_read(g, 30u, 0u, 256u, d200, i40, vu{ 0u, 255u });
        fab_read(g, 40u, 0u, 256u, vu(88u, 200u), vu(), vu());
        g.block_n.push_back(4u);
        bad |= fab_check("long lists, an arena of exactly the needed size", g, 0, 0u, 0u, 4u);
        bad |= fab_check("long lists, one wavefront", g, 0, 0u, 0u, 1u);
    }
    if (g_emu_errors) bad = 1;
    printf(bad ? "CIGAR EMU CHECK FAILED\n" : "CIGAR EMU CHECK OK\n");
    return bad;
}
#endif
