"""Per-strand counts and the minimum alternative fraction of the pileup at cfg2 size (10 M x 150 bp on a chr1-sized contig,
4096-read blocks): the whole contig through Encoder.decode_pileup as the plain call, with
by_strand=True, with by_strand=True and F = 0.02, with F = 0.02 alone and with F = 0.2 alone, alternated in one job after a
warm-up round, the bytes of every round identical.  Per call the four kernel times of cbc_gpu_last_pileup_ms (device events: edits decode; zero +
mark + events; scans; text), medians over the rounds, and the ratio of every post-decode stretch to the plain call's; lines and
text bytes with and without the fraction.  Prints one JSON line and, given a third argument, writes it to that file.
Usage: python tools/pileup_strand_bench.py [reads] [rounds] [result.json]"""
import json, os, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import synth
from cbc_amd import gpu, host

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
RESULT = sys.argv[3] if len(sys.argv) > 3 else None
PPM = gpu.alt_frac_ppm("0.02")
CALLS = [("plain", dict()), ("by_strand", dict(by_strand=True)), ("by_strand_frac", dict(by_strand=True, min_alt_ppm=PPM)),
         ("frac", dict(min_alt_ppm=PPM)), ("frac_0.2", dict(min_alt_ppm=gpu.alt_frac_ppm("0.2")))]
pb = host.synth(0xCBC00002, 248_956_422, N, 150, block_reads=4096)
enc = gpu.Encoder(0)
enc.upload_reference(pb.ref)
_, res, offs, flat = enc.encode_blocks(pb, want_payload_list=False)
assert (res["status"] == 0).all()
c = pb.contigs[0]
fa = synth.fasta_text([("chr1", pb.ref[int(c["ref_off"]): int(c["ref_off"]) + int(c["length"])])])
plan = host.UnpackPlan(pb.container(flat, offs), fa)
enc.upload_reference(plan.ref)
# the bound of plan.pileup_text_cap grows with the window; the call reports the text's size when the buffer is too small
cap = {}
for name, kw in CALLS:
    cap[name] = 256 << 20
    try:
        enc.decode_pileup(plan, text_cap=cap[name], **kw)
    except gpu.CbcGpuError:
        cap[name] = enc.last_pileup_text_bytes
ms = {name: [] for name, _ in CALLS}
wall = {name: [] for name, _ in CALLS}
first, lines, nbytes = {}, {}, {}
for it in range(ROUNDS + 1):                                   # round 0 is the warm-up (arenas grow, pages are touched)
    for name, kw in CALLS:
        t = time.time(); text, n, kept, r = enc.decode_pileup(plan, results=True, text_cap=cap[name], **kw); w = time.time() - t
        assert (r["status"] == 0).all() and kept == pb.n_recs
        if it == 0:
            first[name], lines[name], nbytes[name] = text, n, len(text)
        else:
            assert text == first[name]                         # integer atomics commute: the same bytes every time
            ms[name].append(enc.last_pileup_ms()); wall[name].append(w)
        del text
# the by-strand lines carry the plain call's eleven columns, and the fraction only takes lines away
head = [b"\t".join(x.split(b"\t")[:11]) for x in first["by_strand"].split(b"\n", 20000)[:20000]]
assert head == first["plain"].split(b"\n", 20000)[:20000]
assert lines["by_strand"] == lines["plain"] and lines["frac_0.2"] <= lines["by_strand_frac"] == lines["frac"] <= lines["plain"]
med = lambda xs: float(np.median(xs))
STRETCH = ("edits_decode", "zero_mark_events", "scans", "text")
doc = {"reads": N, "blocks": plan.n_blocks, "rounds": ROUNDS, "min_alt_ppm": PPM, "calls": {}}
for name, _ in CALLS:
    m = [med([x[k] for x in ms[name]]) for k in range(4)]
    doc["calls"][name] = {"lines": lines[name], "text_bytes": nbytes[name], "ms": {s: round(v, 3) for s, v in zip(STRETCH, m)},
                          "post_decode_ms": round(sum(m[1:]), 3), "all": [[round(v, 3) for v in x] for x in ms[name]],
                          "wall_s_min": round(min(wall[name]), 3)}
p = doc["calls"]["plain"]
for name in ("by_strand", "by_strand_frac", "frac", "frac_0.2"):
    q = doc["calls"][name]
    q["over_plain"] = {s: round(q["ms"][s] / p["ms"][s], 3) for s in STRETCH}
    q["over_plain"]["post_decode"] = round(q["post_decode_ms"] / p["post_decode_ms"], 3)
doc["by_strand_post_decode_within_2x"] = bool(doc["calls"]["by_strand"]["over_plain"]["post_decode"] <= 2.0)
print(json.dumps(doc))
enc.close()
if RESULT:
    with open(RESULT, "w") as f:
        json.dump(doc, f, indent=1); f.write("\n")
