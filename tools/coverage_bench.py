"""Per-target coverage summary at cfg2 size (10 M x 150 bp on a chr1-sized contig, 4096-read blocks).
1. The whole contig cut into windows of 1000 and of 100 bases through Encoder.decode_coverage, alternated with the existing
   Encoder.decode_depth(region=<contig>) after a warm-up round, medians of the rounds, device events.  The four new passes
   (weights, weight scans, prefixes, lookup) may take at most 1.25 x the text pass (count + scan + write) of decode_depth as
   measured in the same job; on a miss the pass that carries it is named.
2. `cbc -x --bedcov --regions-file` for a 2000-line panel beside `cbc -x --depth --regions-file` for the same file.
Every CLI step runs under its own time limit and the script stops at the first failure.  Prints one JSON line per measurement
and, given a fourth argument, writes them to that file as one JSON document.
Usage: python tools/coverage_bench.py [reads] [out_dir] [rounds] [result.json]"""
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
NAMES = ("weights", "weight_scans", "prefixes", "lookup")
doc = []
for window in (1000, 100):
    qs = plan.queries(window=window)
    cov_ms, dep_ms = [], []
    for it in range(ROUNDS + 1):                               # round 0 is the warm-up (arenas grow, pages are touched)
        _, s0, e0, total, covered = enc.decode_coverage(plan, qs)
        m1 = enc.last_coverage_ms()
        text = enc.decode_depth(plan, "chr1"); m2 = enc.last_depth_ms()
        if it == 0:                                            # the sums add up to the track's area, the covered counts to its length
            rows = np.array([ln.split(b"\t")[1:] for ln in text.split(b"\n")[:-1]], dtype=np.int64)
            assert int(total.sum()) == int(((rows[:, 1] - rows[:, 0]) * rows[:, 2]).sum())
            assert int(covered.sum()) == int((rows[:, 1] - rows[:, 0]).sum())
            first = (total.copy(), covered.copy())
        else:
            assert (total == first[0]).all() and (covered == first[1]).all()
        del text
        if it:
            cov_ms.append(m1); dep_ms.append(m2)
    new = [med([x[3 + k] for x in cov_ms]) for k in range(4)]
    text_pass = med([x[3] for x in dep_ms])
    hold = sum(new) <= 1.25 * text_pass
    doc.append({"case": "whole contig in windows", "window": window, "queries": qs.n_q, "reads": N, "blocks": plan.n_blocks, "rounds": ROUNDS,
                "coverage_ms": [[round(v, 3) for v in x] for x in cov_ms], "depth_ms": [[round(v, 3) for v in x] for x in dep_ms],
                "new_passes_ms": {n: round(v, 3) for n, v in zip(NAMES, new)}, "new_passes_sum_ms": round(sum(new), 3),
                "existing_text_pass_ms": round(text_pass, 3), "bar_limit_ms": round(1.25 * text_pass, 3), "bar_holds": bool(hold),
                "largest_pass": NAMES[int(np.argmax(new))]})
    print(json.dumps(doc[-1]), flush=True)
enc.close()
rng = np.random.default_rng(2000)
beg = np.sort(rng.integers(1, clen - 2000, 2000))
bed = b"".join(b"chr1\t%d\t%d\n" % (int(b) - 1, int(b) - 1 + int(w)) for b, w in zip(beg, rng.integers(200, 2001, 2000)))
os.makedirs(OUT, exist_ok=True)
P = lambda f: os.path.join(OUT, f)
open(P("cfg2.cbc"), "wb").write(blob); open(P("chr1.fa"), "wb").write(fa); open(P("panel.bed"), "wb").write(bed)
exe = os.path.join(R, "cbc_amd", "csrc", "cbc")
rc = 0
for name, extra, outf in [("cbc -x --bedcov --regions-file", ["--bedcov", "--regions-file", P("panel.bed"), "--verbose"], "out.cov"),
                          ("cbc -x --depth --regions-file", ["--depth", "--regions-file", P("panel.bed"), "--verbose"], "out.bg")]:
    t = time.time()
    p = subprocess.run([exe, "-x", P("cfg2.cbc"), P(outf), P("chr1.fa")] + extra, capture_output=True, text=True, timeout=600)
    doc.append({"cli": name, "rc": p.returncode, "wall_s": round(time.time() - t, 3),
                "out_bytes": os.path.getsize(P(outf)) if os.path.exists(P(outf)) else -1,
                "stdout": p.stdout.strip().splitlines(), "stderr": p.stderr[-500:]})
    print(json.dumps(doc[-1]), flush=True)
    if p.returncode:                                           # stop at the first failure: nothing more is started on the device
        rc = 1
        break
for f in ("cfg2.cbc", "chr1.fa", "panel.bed", "out.cov", "out.bg"):
    if os.path.exists(P(f)):
        os.remove(P(f))
if RESULT:
    with open(RESULT, "w") as f:
        json.dump(doc, f, indent=1); f.write("\n")
sys.exit(rc)
