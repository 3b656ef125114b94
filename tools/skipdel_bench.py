"""Deletion-aware coverage at cfg2 size (10 M x 150 bp on a chr1-sized contig, 4096-read blocks): the
whole contig through Encoder.decode_depth(skip_deletions=True), Encoder.decode_depth and Encoder.decode_pileup, alternated in one
job after a warm-up round, kernel times by device events (the four stretches of cbc_gpu_last_depth_ms / cbc_gpu_last_pileup_ms),
medians of the rounds.  Reported, none of them a gate: edits decode / span decode; mark + unmark beside the span depth's mark
and beside the pileup's zero + mark + events; the text sizes, runs and deleted bases.  Prints one JSON line and, given a third
argument, writes it to that file as one JSON document.
Usage: python tools/skipdel_bench.py [reads] [rounds] [result.json]"""
import json, os, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import synth
from cbc_amd import gpu, host

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
RESULT = sys.argv[3] if len(sys.argv) > 3 else None
pb = host.synth(0xCBC00002, 248_956_422, N, 150, block_reads=4096)
enc = gpu.Encoder(0)
enc.upload_reference(pb.ref)
_, res, offs, flat = enc.encode_blocks(pb, want_payload_list=False)
assert (res["status"] == 0).all()
c = pb.contigs[0]
fa = synth.fasta_text([("chr1", pb.ref[int(c["ref_off"]): int(c["ref_off"]) + int(c["length"])])])
plan = host.UnpackPlan(pb.container(flat, offs), fa)
enc.upload_reference(plan.ref)
# the bounds of the two per-position texts grow with the window; a call reports the text's size when the buffer is too small
caps = {}
for name, call in (("skip", lambda cap: enc.decode_depth(plan, skip_deletions=True, text_cap=cap)), ("pileup", lambda cap: enc.decode_pileup(plan, text_cap=cap))):
    caps[name] = 256 << 20
    try:
        call(caps[name])
    except gpu.CbcGpuError:
        caps[name] = enc.last_depth_text_bytes if name == "skip" else enc.last_pileup_text_bytes
ms = {"skip": [], "span": [], "pileup": []}
wall = {"skip": [], "span": [], "pileup": []}
info = {}
first = {}
for it in range(ROUNDS + 1):                                   # round 0 is the warm-up (arenas grow, pages are touched)
    for name in ("skip", "span", "pileup"):
        t = time.time()
        if name == "skip":
            text, n, kept, r = enc.decode_depth(plan, skip_deletions=True, results=True, text_cap=caps["skip"]); m = enc.last_depth_ms()
        elif name == "span":
            text, n, kept, r = enc.decode_depth(plan, results=True); m = enc.last_depth_ms()
        else:
            text, n, kept, r = enc.decode_pileup(plan, results=True, text_cap=caps["pileup"]); m = enc.last_pileup_ms()
        w = time.time() - t
        assert (r["status"] == 0).all() and kept == pb.n_recs
        if it == 0:
            first[name] = text
            info[name] = {"text_bytes": len(text), "lines": n}
            if name == "pileup":                               # the deleted bases the unmark pass takes off: the pileup's del column
                info["deleted_bases"] = int(sum(int(ln.split(b"\t")[9]) for ln in text.split(b"\n")[:-1]))
        else:
            assert text == first[name]                         # integer atomics commute: the same bytes every time
            ms[name].append(m); wall[name].append(w)
        del text
med = lambda xs: float(np.median(xs))
col = lambda name, k: round(med([x[k] for x in ms[name]]), 3)
doc = {"reads": N, "blocks": plan.n_blocks, "rounds": ROUNDS, "edits_per_read": 16, **info,
       "skip_ms": {"edits_decode": col("skip", 0), "zero_mark_unmark": col("skip", 1), "scan_compact": col("skip", 2), "text": col("skip", 3),
                   "all": [[round(v, 3) for v in x] for x in ms["skip"]]},
       "span_ms": {"span_decode": col("span", 0), "zero_mark": col("span", 1), "scan_compact": col("span", 2), "text": col("span", 3),
                   "all": [[round(v, 3) for v in x] for x in ms["span"]]},
       "pileup_ms": {"edits_decode": col("pileup", 0), "zero_mark_events": col("pileup", 1), "scans": col("pileup", 2), "text": col("pileup", 3),
                     "all": [[round(v, 3) for v in x] for x in ms["pileup"]]},
       "edits_over_span_decode": round(col("skip", 0) / col("span", 0), 4),
       "unmark_ms_over_mark": round(col("skip", 1) - col("span", 1), 3),
       "mark_unmark_over_pileup_events": round(col("skip", 1) / col("pileup", 1), 4),
       "wall_s_min": {k: round(min(v), 3) for k, v in wall.items()}}
print(json.dumps(doc))
enc.close()
if RESULT:
    with open(RESULT, "w") as f:
        json.dump(doc, f, indent=1); f.write("\n")
