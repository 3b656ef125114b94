"""Decode of a set of regions at cfg2 size (10 M x 150 bp on a chr1-sized contig, 4096-read blocks).
1. One interval covering the whole contig through Encoder.decode_targets, alternated with the existing single-region call of
   the same output (decode_region / decode_sam / decode_depth on "chr1") after a warm-up round, medians of the rounds, device
   events; the bytes must be identical and the passes behind the decode may exceed the existing path's median by at most 10 %.
2. A panel-shaped set, 2000 seeded intervals of 200 to 2000 bases: blocks selected and the pass times of the three outputs,
   then `cbc -x --regions-file` beside the full `cbc -x --sam` with the files in a directory of your choice.
Every CLI step runs under its own time limit and the script stops at the first failure.  Prints one JSON line per measurement
and, given a fourth argument, writes them to that file as one JSON document.
Usage: python tools/targets_bench.py [reads] [out_dir] [rounds] [result.json]"""
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
clen = int(c["length"])
fa = synth.fasta_text([("chr1", pb.ref[int(c["ref_off"]): int(c["ref_off"]) + clen])])
blob = pb.container(flat, offs)
plan = host.UnpackPlan(blob, fa)
enc.upload_reference(plan.ref)
med = lambda xs: float(np.median(xs))
doc = []
whole = plan.targets(["chr1"])
assert whole.n_iv == 1 and whole.n_blocks == plan.n_blocks
old_calls = {"reads": (lambda: enc.decode_region(plan, "chr1"), enc.last_region_ms),
             "sam": (lambda: enc.decode_sam(plan, "chr1"), enc.last_sam_ms),
             "depth": (lambda: enc.decode_depth(plan, "chr1"), enc.last_depth_ms)}
for out, (old, old_ms) in old_calls.items():
    new_ms, ref_ms = [], []
    for it in range(ROUNDS + 1):                               # round 0 is the warm-up (arenas grow, pages are touched)
        a = enc.decode_targets(plan, whole, out); m1 = enc.last_targets_ms()
        b = old(); m2 = old_ms()
        assert a == b, "decode_targets(%s) over the whole contig differs from the single-region call" % out
        del a, b
        if it:
            new_ms.append(m1); ref_ms.append(m2)
    new_after = med([sum(x[1:]) for x in new_ms]); ref_after = med([sum(x[1:]) for x in ref_ms])
    doc.append({"case": "whole contig, one interval", "output": out, "reads": N, "blocks": plan.n_blocks, "rounds": ROUNDS,
                "targets_ms": [[round(v, 3) for v in x] for x in new_ms], "existing_ms": [[round(v, 3) for v in x] for x in ref_ms],
                "targets_after_decode_ms": round(new_after, 3), "existing_after_decode_ms": round(ref_after, 3),
                "bar_limit_ms": round(1.1 * ref_after, 3), "bar_holds": bool(new_after <= 1.1 * ref_after), "bytes_identical": True})
    print(json.dumps(doc[-1]), flush=True)
rng = np.random.default_rng(2000)
beg = np.sort(rng.integers(1, clen - 2000, 2000))
bed = b"".join(b"chr1\t%d\t%d\n" % (int(b) - 1, int(b) - 1 + int(w)) for b, w in zip(beg, rng.integers(200, 2001, 2000)))
panel = plan.targets((), bed)
for out in ("reads", "sam", "depth"):
    ms = []
    for it in range(ROUNDS + 1):
        text, n, runs, r = enc.decode_targets(plan, panel, out, results=True)
        assert (r["status"] == 0).all()
        if it:
            ms.append(enc.last_targets_ms())
    doc.append({"case": "panel, 2000 intervals of 200..2000 bases", "output": out, "intervals_merged": panel.n_iv,
                "blocks_selected": panel.n_blocks, "blocks": plan.n_blocks, "reads_or_kept": n, "runs": runs, "text_bytes": len(text),
                "ms_decode_filter_scan_text": [[round(v, 3) for v in x] for x in ms],
                "median_ms": [round(med([x[k] for x in ms]), 3) for k in range(4)]})
    print(json.dumps(doc[-1]), flush=True)
enc.close()
os.makedirs(OUT, exist_ok=True)
P = lambda f: os.path.join(OUT, f)
open(P("cfg2.cbc"), "wb").write(blob); open(P("chr1.fa"), "wb").write(fa); open(P("panel.bed"), "wb").write(bed)
exe = os.path.join(R, "cbc_amd", "csrc", "cbc")
rc = 0
for name, extra, outf in [("cbc -x --regions-file", ["--regions-file", P("panel.bed"), "--verbose"], "out.txt"),
                          ("cbc -x --regions-file --sam", ["--regions-file", P("panel.bed"), "--sam", "--verbose"], "out.sam"),
                          ("cbc -x --regions-file --depth", ["--regions-file", P("panel.bed"), "--depth", "--verbose"], "out.bg"),
                          ("cbc -x --sam", ["--sam", "--verbose"], "full.sam")]:
    t = time.time()
    p = subprocess.run([exe, "-x", P("cfg2.cbc"), P(outf), P("chr1.fa")] + extra, capture_output=True, text=True, timeout=600)
    doc.append({"cli": name, "rc": p.returncode, "wall_s": round(time.time() - t, 3),
                "out_bytes": os.path.getsize(P(outf)) if os.path.exists(P(outf)) else -1,
                "stdout": p.stdout.strip().splitlines(), "stderr": p.stderr[-500:]})
    print(json.dumps(doc[-1]), flush=True)
    if p.returncode:                                           # stop at the first failure: nothing more is started on the device
        rc = 1
        break
for f in ("cfg2.cbc", "chr1.fa", "panel.bed", "out.txt", "out.sam", "out.bg", "full.sam"):
    if os.path.exists(P(f)):
        os.remove(P(f))
if RESULT:
    with open(RESULT, "w") as f:
        json.dump(doc, f, indent=1); f.write("\n")
sys.exit(rc)
