"""Depth histogram at cfg2 size (10 M x 150 bp on a chr1-sized contig, 4096-read blocks).
1. The whole contig through Encoder.decode_depth_hist, alternated with the existing Encoder.decode_depth(region=<contig>) after a
   warm-up round, medians of the rounds, device events.  The new passes (zero + accumulate, bin compaction) may take no longer
   than the text passes (count + scan + write) of decode_depth as measured in the same job.
2. The same histogram calls in a child process on libcbc_gpu_hist_nolds.so (make -C cbc_amd/csrc libcbc_gpu_hist_nolds.so), where
   every run goes to the global bin table: the A/B of the LDS table.  Skipped with a note when that library is not built.
3. `cbc -x --depth-hist` beside `cbc -x --depth` on the same files, wall time.
Every child runs under its own time limit and the script stops at the first failure.  Prints one JSON line per measurement and,
given a fourth argument, writes them to that file as one JSON document.
Usage: python tools/hist_bench.py [reads] [out_dir] [rounds] [result.json]"""
import json, os, subprocess, sys, tempfile, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import synth
from cbc_amd import gpu, host

CHILD = len(sys.argv) > 1 and sys.argv[1] == "--child"      # --child <container> <fasta> <rounds>: the histogram calls alone
med = lambda xs: float(np.median(xs))


def hist_rounds(enc, plan, rounds, with_depth):
    h_ms, d_ms, first = [], [], None
    for it in range(rounds + 1):                             # round 0 is the warm-up (arenas grow, pages are touched)
        got = enc.decode_depth_hist(plan)
        m1 = enc.last_hist_ms()
        rows = [(c, d.tolist(), b.tolist(), s) for c, d, b, s in got]
        if with_depth:
            text = enc.decode_depth(plan, "chr1"); m2 = enc.last_depth_ms()
            if it == 0:                                      # the bins add up to the track: area and covered length
                t = np.array([ln.split(b"\t")[1:] for ln in text.split(b"\n")[:-1]], dtype=np.int64)
                assert sum(d * b for d, b in zip(rows[0][1], rows[0][2])) == int(((t[:, 1] - t[:, 0]) * t[:, 2]).sum())
                assert sum(b for d, b in zip(rows[0][1], rows[0][2]) if d) == int((t[:, 1] - t[:, 0]).sum())
            del text
            if it:
                d_ms.append(m2)
        if it == 0:
            first = rows
        else:
            assert rows == first
            h_ms.append(m1)
    return h_ms, d_ms, first


if CHILD:
    plan = host.UnpackPlan(open(sys.argv[2], "rb").read(), open(sys.argv[3], "rb").read())
    enc = gpu.Encoder(0)
    enc.upload_reference(plan.ref)
    h_ms, _, first = hist_rounds(enc, plan, int(sys.argv[4]), False)
    print(json.dumps({"hist_ms": [[round(v, 3) for v in x] for x in h_ms], "bins": len(first[0][1]), "lib": os.path.basename(gpu.GPU_LIB)}))
    enc.close()
    sys.exit(0)

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
doc = []
h_ms, d_ms, first = hist_rounds(enc, plan, ROUNDS, True)
enc.close()
accum, compact = med([x[3] for x in h_ms]), med([x[4] for x in h_ms])
text_pass = med([x[3] for x in d_ms])
doc.append({"case": "whole contig", "reads": N, "blocks": plan.n_blocks, "rounds": ROUNDS, "bins": len(first[0][1]),
            "max_depth_seen": int(first[0][1][-1]), "hist_ms": [[round(v, 3) for v in x] for x in h_ms],
            "depth_ms": [[round(v, 3) for v in x] for x in d_ms],
            "new_passes_ms": {"zero_accumulate": round(accum, 3), "bin_compaction": round(compact, 3)}, "new_passes_sum_ms": round(accum + compact, 3),
            "existing_text_pass_ms": round(text_pass, 3), "bar_holds": bool(accum + compact <= text_pass)})
print(json.dumps(doc[-1]), flush=True)
os.makedirs(OUT, exist_ok=True)
P = lambda f: os.path.join(OUT, f)
open(P("cfg2.cbc"), "wb").write(blob); open(P("chr1.fa"), "wb").write(fa)
rc = 0
nolds = os.path.join(R, "cbc_amd", "csrc", "libcbc_gpu_hist_nolds.so")
if os.path.exists(nolds):
    runs = {}
    for tag, lib in (("lds", gpu.GPU_LIB), ("no_lds", nolds)):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", P("cfg2.cbc"), P("chr1.fa"), str(ROUNDS)],
                           env=dict(os.environ, CBC_GPU_LIB=lib), capture_output=True, text=True, timeout=600)
        if p.returncode:                                     # stop at the first failure: nothing more is started on the device
            doc.append({"ab": tag, "rc": p.returncode, "stderr": p.stderr[-500:]}); print(json.dumps(doc[-1]), flush=True)
            rc = 1
            break
        runs[tag] = json.loads(p.stdout.strip().splitlines()[-1])
    if not rc:
        a, b = ([x[3] for x in runs[t]["hist_ms"]] for t in ("lds", "no_lds"))
        doc.append({"ab": "zero + accumulate, LDS table against direct list_add", "lds_ms": a, "no_lds_ms": b, "lds_median_ms": round(med(a), 3),
                    "no_lds_median_ms": round(med(b), 3), "lds_faster_beyond_spread": bool(max(a) < min(b)), "same_bins": runs["lds"]["bins"] == runs["no_lds"]["bins"]})
        print(json.dumps(doc[-1]), flush=True)
else:
    doc.append({"ab": "skipped: libcbc_gpu_hist_nolds.so is not built"}); print(json.dumps(doc[-1]), flush=True)
exe = os.path.join(R, "cbc_amd", "csrc", "cbc")
for name, extra, outf in [("cbc -x --depth-hist", ["--depth-hist", "--verbose"], "out.hist"), ("cbc -x --depth", ["--depth", "--verbose"], "out.bg")]:
    if rc:
        break
    t = time.time()
    p = subprocess.run([exe, "-x", P("cfg2.cbc"), P(outf), P("chr1.fa")] + extra, capture_output=True, text=True, timeout=600)
    doc.append({"cli": name, "rc": p.returncode, "wall_s": round(time.time() - t, 3),
                "out_bytes": os.path.getsize(P(outf)) if os.path.exists(P(outf)) else -1,
                "stdout": p.stdout.strip().splitlines(), "stderr": p.stderr[-500:]})
    print(json.dumps(doc[-1]), flush=True)
    if p.returncode:
        rc = 1
for f in ("cfg2.cbc", "chr1.fa", "out.hist", "out.bg"):
    if os.path.exists(P(f)):
        os.remove(P(f))
if RESULT:
    with open(RESULT, "w") as f:
        json.dump(doc, f, indent=1); f.write("\n")
sys.exit(rc)
