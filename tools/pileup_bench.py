"""Per-position allele counts at cfg2 size (10 M x 150 bp on a chr1-sized contig, 4096-read blocks):
the whole contig through Encoder.decode_pileup (the four kernel times: edits decode, zero + mark + events, scans, text)
alternated with Encoder.decode_depth after a warm-up round, the bytes of every round identical.  Two bars, both against the span
decode of the alternated depth call: (i) events + scans + text <= that decode; (ii) the ratio of the edits decode to it, reported.
Then `cbc -x --pileup` beside `cbc -x --depth` with the files in a directory of your choice (/dev/shm for the numbers in
DESIGN.md).  Prints one JSON line per measurement and, given a fourth argument, writes them to that file as one JSON document.
Usage: python tools/pileup_bench.py [reads] [out_dir] [rounds] [result.json]"""
import json, os, subprocess, sys, tempfile, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import synth
from cbc_amd import gpu, host

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
OUT = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp()
ROUNDS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
RESULT = sys.argv[4] if len(sys.argv) > 4 else None
pb = host.synth(0xCBC00002, 248_956_422, N, 150, block_reads=4096)
enc = gpu.Encoder(0)
enc.upload_reference(pb.ref)
_, res, offs, flat = enc.encode_blocks(pb, want_payload_list=False)
assert (res["status"] == 0).all()
c = pb.contigs[0]
fa = synth.fasta_text([("chr1", pb.ref[int(c["ref_off"]): int(c["ref_off"]) + int(c["length"])])])
blob = pb.container(flat, offs)
plan = host.UnpackPlan(blob, fa)
enc.upload_reference(plan.ref)
# the bound of plan.pileup_text_cap grows with the window (26 GB here); the call reports the text's size when the buffer is
# too small, so the first call finds it
cap = 256 << 20
try:
    enc.decode_pileup(plan, text_cap=cap)
except gpu.CbcGpuError:
    cap = enc.last_pileup_text_bytes
pil_ms, dep_ms, pil_wall, dep_wall = [], [], [], []
for it in range(ROUNDS + 1):                                   # round 0 is the warm-up (arenas grow, pages are touched)
    t = time.time(); text, lines, kept, r = enc.decode_pileup(plan, results=True, text_cap=cap); w = time.time() - t
    assert (r["status"] == 0).all() and kept == pb.n_recs
    p_ = enc.last_pileup_ms(); pil_bytes = len(text)
    if it == 0:
        first = text
        head = [ln.split(b"\t") for ln in text[:4_000_000].split(b"\n")[:-1]]
        assert all(len(x) == 11 and int(x[3]) == sum(int(v) for v in x[4:10]) for x in head)
    else:
        assert text == first                                   # integer atomics commute: the same bytes every time
    del text
    t = time.time(); bg, runs, dkept, r = enc.decode_depth(plan, results=True); w2 = time.time() - t
    assert (r["status"] == 0).all() and dkept == kept
    d_ = enc.last_depth_ms(); dep_bytes = len(bg)
    del bg
    if it:
        pil_ms.append(p_); dep_ms.append(d_); pil_wall.append(w); dep_wall.append(w2)
med = lambda xs: float(np.median(xs))
dec, ev, scan, txt = (med([x[k] for x in pil_ms]) for k in range(4))
span_dec = med([x[0] for x in dep_ms])
doc = [{"reads": N, "blocks": plan.n_blocks, "rounds": ROUNDS, "pileup_text_bytes": pil_bytes, "lines": lines, "depth_text_bytes": dep_bytes,
        "pileup_ms": {"edits_decode": round(dec, 3), "zero_mark_events": round(ev, 3), "scans": round(scan, 3), "text": round(txt, 3),
                      "all": [[round(v, 3) for v in x] for x in pil_ms]},
        "depth_ms": {"span_decode": round(span_dec, 3), "mark": round(med([x[1] for x in dep_ms]), 3),
                     "scan_compact": round(med([x[2] for x in dep_ms]), 3), "text": round(med([x[3] for x in dep_ms]), 3),
                     "all": [[round(v, 3) for v in x] for x in dep_ms]},
        "bar_limit_ms": round(span_dec, 3), "new_passes_ms": round(ev + scan + txt, 3), "bar_holds": bool(ev + scan + txt <= span_dec),
        "edits_over_span_decode": round(dec / span_dec, 4),
        "pileup_wall_s_min": round(min(pil_wall), 3), "depth_wall_s_min": round(min(dep_wall), 3)}]
print(json.dumps(doc[0]))
enc.close()
os.makedirs(OUT, exist_ok=True)
open(os.path.join(OUT, "cfg2.cbc"), "wb").write(blob); open(os.path.join(OUT, "chr1.fa"), "wb").write(fa)
exe = os.path.join(R, "cbc_amd", "csrc", "cbc")
for name, extra, outf in [("cbc -x --depth", ["--depth", "--verbose"], "out.bg"), ("cbc -x --pileup", ["--pileup", "--verbose"], "out.pileup")]:
    t = time.time()
    p = subprocess.run([exe, "-x", os.path.join(OUT, "cfg2.cbc"), os.path.join(OUT, outf), os.path.join(OUT, "chr1.fa")] + extra,
                       capture_output=True, text=True, timeout=900)
    doc.append({"cli": name, "rc": p.returncode, "wall_s": round(time.time() - t, 3),
                "out_bytes": os.path.getsize(os.path.join(OUT, outf)) if os.path.exists(os.path.join(OUT, outf)) else -1,
                "stdout": p.stdout.strip().splitlines(), "stderr": p.stderr[-500:]})
    print(json.dumps(doc[-1]))
for f in ("cfg2.cbc", "chr1.fa", "out.bg", "out.pileup"):
    if os.path.exists(os.path.join(OUT, f)):
        os.remove(os.path.join(OUT, f))
if RESULT:
    with open(RESULT, "w") as f:
        json.dump(doc, f, indent=1); f.write("\n")
