"""Coverage output at cfg2 size (10 M x 150 bp on a chr1-sized contig, 4096-read blocks): the whole
contig through Encoder.decode_depth (the four kernel times: span decode, mark, scan + compact, text) alternated with
Encoder.decode_sam after a warm-up round; the bar is mark + scan + text <= the span decode of the same call.  Then
`cbc -x --depth` beside `cbc -x --sam` with the files in a directory of your choice (/dev/shm for the numbers in DESIGN.md).
Prints one JSON line per measurement and, given a fourth argument, writes them to that file as one JSON document.
Usage: python tools/depth_bench.py [reads] [out_dir] [rounds] [result.json]"""
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
hdr = plan.sam_header()
dep_ms, sam_ms, dep_wall, sam_wall = [], [], [], []
for it in range(ROUNDS + 1):                                   # round 0 is the warm-up (arenas grow, pages are touched)
    t = time.time(); text, runs, kept, r = enc.decode_depth(plan, results=True); w = time.time() - t
    assert (r["status"] == 0).all() and kept == pb.n_recs
    d_ = enc.last_depth_ms(); dep_bytes = len(text)
    if it == 0:                                                # the depth summed over the runs = the bases of the reads' spans
        first = text
        rows = np.array([ln.split(b"\t")[1:] for ln in text[:40_000_000].split(b"\n")[:-1]], dtype=np.int64)
        assert (rows[:, 0] < rows[:, 1]).all() and (rows[1:, 0] >= rows[:-1, 1]).all() and (rows[:, 2] > 0).all()
    else:
        assert text == first                                   # integer atomics commute: the same bytes every time
    del text
    t = time.time(); sam, n, _, r = enc.decode_sam(plan, results=True); w2 = time.time() - t
    assert (r["status"] == 0).all() and n == pb.n_recs
    s_ = enc.last_sam_ms(); sam_bytes = len(sam) - len(hdr)
    del sam
    if it:
        dep_ms.append(d_); sam_ms.append(s_); dep_wall.append(w); sam_wall.append(w2)
med = lambda xs: float(np.median(xs))
dec, mark, scan, txt = (med([x[k] for x in dep_ms]) for k in range(4))
doc = [{"reads": N, "blocks": plan.n_blocks, "rounds": ROUNDS, "depth_text_bytes": dep_bytes, "runs": runs, "sam_text_bytes": sam_bytes,
        "depth_ms": {"span_decode": round(dec, 3), "mark": round(mark, 3), "scan_compact": round(scan, 3), "text": round(txt, 3),
                     "all": [[round(v, 3) for v in x] for x in dep_ms]},
        "sam_ms": {"decode": round(med([x[0] for x in sam_ms]), 3), "count_scan": round(med([x[1] for x in sam_ms]), 3),
                   "text": round(med([x[2] for x in sam_ms]), 3)},
        "bar_limit_ms": round(dec, 3), "new_passes_ms": round(mark + scan + txt, 3), "bar_holds": bool(mark + scan + txt <= dec),
        "depth_wall_s_min": round(min(dep_wall), 3), "sam_wall_s_min": round(min(sam_wall), 3)}]
print(json.dumps(doc[0]))
enc.close()
os.makedirs(OUT, exist_ok=True)
open(os.path.join(OUT, "cfg2.cbc"), "wb").write(blob); open(os.path.join(OUT, "chr1.fa"), "wb").write(fa)
exe = os.path.join(R, "cbc_amd", "csrc", "cbc")
for name, extra, outf in [("cbc -x --sam", ["--sam", "--verbose"], "out.sam"), ("cbc -x --depth", ["--depth", "--verbose"], "out.bg")]:
    t = time.time()
    p = subprocess.run([exe, "-x", os.path.join(OUT, "cfg2.cbc"), os.path.join(OUT, outf), os.path.join(OUT, "chr1.fa")] + extra,
                       capture_output=True, text=True, timeout=900)
    doc.append({"cli": name, "rc": p.returncode, "wall_s": round(time.time() - t, 3),
                "out_bytes": os.path.getsize(os.path.join(OUT, outf)) if os.path.exists(os.path.join(OUT, outf)) else -1,
                "stdout": p.stdout.strip().splitlines(), "stderr": p.stderr[-500:]})
    print(json.dumps(doc[-1]))
for f in ("cfg2.cbc", "chr1.fa", "out.sam", "out.bg"):
    if os.path.exists(os.path.join(OUT, f)):
        os.remove(os.path.join(OUT, f))
if RESULT:
    with open(RESULT, "w") as f:
        json.dump(doc, f, indent=1); f.write("\n")
