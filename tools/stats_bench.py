"""Read statistics at cfg2 size (10 M x 150 bp on a chr1-sized contig, 4096-read blocks).
1. The whole file through Encoder.decode_stats: one warm-up round (arenas grow, code objects load), then `rounds` timed rounds,
   device events, medians and the spread.  Beside the statistics pass go its two yardsticks: the decode kernel's time in the same
   call (existing code; the ratio is recorded, not required) and the streaming floor -- the rows' bytes over the 6.3 TB/s the
   microarchitecture guide gives as the achievable HBM rate.  The tables of every round are compared with the first round's, and
   the first round's with numpy counts over the packer's arrays (FLAG and length tables, the base count).
2. The same calls in child processes, alternated, on the shipped library and on libcbc_gpu_stats_flagglobal.so
   (make -C cbc_amd/csrc libcbc_gpu_stats_flagglobal.so), where every FLAG goes to the global table with one atomic add: the A/B
   of the FLAG table in LDS.  Skipped with a note when that library is not built.
3. `cbc -x --stats --verbose` on the same files, wall time.
Every child runs under its own time limit and the script stops at the first failure.  Prints one JSON line per measurement and,
given a fourth argument, writes them to that file as one JSON document.
Usage: python tools/stats_bench.py [reads] [out_dir] [rounds] [result.json]"""
import json, os, subprocess, sys, tempfile, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import synth
from cbc_amd import gpu, host

CHILD = len(sys.argv) > 1 and sys.argv[1] == "--child"      # --child <container> <fasta> <rounds>: the statistics calls alone
HBM_TBS = 6.3
med = lambda xs: float(np.median(xs))


def key(st):
    return (st["reads"], st["excluded"], st["flag"].tobytes(), st["len"].tobytes(), st["gc"].tobytes(), st["cyc"].tobytes())


def stats_rounds(enc, plan, rounds):
    ms, first = [], None
    for it in range(rounds + 1):                             # round 0 is the warm-up
        st = enc.decode_stats(plan)
        if it == 0:
            first = st
        else:
            assert key(st) == key(first)
            ms.append(enc.last_stats_ms())
    return ms, first


if CHILD:
    plan = host.UnpackPlan(open(sys.argv[2], "rb").read(), open(sys.argv[3], "rb").read())
    enc = gpu.Encoder(0)
    enc.upload_reference(plan.ref)
    ms, first = stats_rounds(enc, plan, int(sys.argv[4]))
    print(json.dumps({"stats_ms": [[round(v, 3) for v in x] for x in ms], "reads": first["reads"], "flags": int((first["flag"] > 0).sum()),
                      "lib": os.path.basename(gpu.GPU_LIB)}))
    enc.close()
    sys.exit(0)

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
OUT = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp()
ROUNDS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
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
ms, first = stats_rounds(enc, plan, ROUNDS)
enc.close()
assert first["reads"] == N and first["excluded"] == 0
assert np.array_equal(first["flag"], np.bincount(pb.recs["flag"], minlength=65536).astype(np.uint32))
assert np.array_equal(first["len"], np.bincount(pb.recs["rlen"], minlength=257).astype(np.uint32))
assert int(first["cyc"].astype(np.int64).sum()) == int(pb.recs["rlen"].astype(np.int64).sum())
row_bytes = N * plan.seq_stride + N * 16                     # the rows and the 16-byte records the pass streams
floor_ms = row_bytes / (HBM_TBS * 1e12) * 1e3
dec, st = [x[0] for x in ms], [x[1] for x in ms]
doc.append({"case": "whole file", "reads": N, "blocks": plan.n_blocks, "rounds": ROUNDS, "seq_stride": plan.seq_stride,
            "stats_ms": [[round(v, 3) for v in x] for x in ms], "decode_median_ms": round(med(dec), 3), "stats_median_ms": round(med(st), 3),
            "stats_min_ms": round(min(st), 3), "stats_max_ms": round(max(st), 3), "stats_over_decode": round(med(st) / med(dec), 4),
            "streamed_bytes": row_bytes, "hbm_tb_per_s_assumed": HBM_TBS, "streaming_floor_ms": round(floor_ms, 3),
            "stats_over_floor": round(med(st) / floor_ms, 2), "achieved_tb_per_s": round(row_bytes / (med(st) * 1e-3) / 1e12, 3),
            "d2h_bytes": 4 * (65536 + 257 + 101 + 4 * 256 + 2), "flag_values": int((first["flag"] > 0).sum())})
print(json.dumps(doc[-1]), flush=True)
os.makedirs(OUT, exist_ok=True)
P = lambda f: os.path.join(OUT, f)
open(P("cfg2.cbc"), "wb").write(blob); open(P("chr1.fa"), "wb").write(fa)
rc = 0
ab = os.path.join(R, "cbc_amd", "csrc", "libcbc_gpu_stats_flagglobal.so")
if os.path.exists(ab):
    runs = {"lds": [], "global": []}
    for tag, lib in (("lds", gpu.GPU_LIB), ("global", ab)) * 2:                  # alternated: lds, global, lds, global
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", P("cfg2.cbc"), P("chr1.fa"), str(ROUNDS)],
                           env=dict(os.environ, CBC_GPU_LIB=lib), capture_output=True, text=True, timeout=600)
        if p.returncode:                                     # stop at the first failure: nothing more is started on the device
            doc.append({"ab": tag, "rc": p.returncode, "stderr": p.stderr[-500:]}); print(json.dumps(doc[-1]), flush=True)
            rc = 1
            break
        runs[tag].append(json.loads(p.stdout.strip().splitlines()[-1]))
    if not rc:
        a, b = ([x[1] for r in runs[t] for x in r["stats_ms"]] for t in ("lds", "global"))
        doc.append({"ab": "statistics pass, FLAG table in LDS against every FLAG to the global table", "lds_ms": a, "global_ms": b,
                    "lds_median_ms": round(med(a), 3), "global_median_ms": round(med(b), 3), "lds_faster_beyond_spread": bool(max(a) < min(b)),
                    "same_reads": len({r["reads"] for t in runs for r in runs[t]}) == 1})
        print(json.dumps(doc[-1]), flush=True)
else:
    doc.append({"ab": "skipped: libcbc_gpu_stats_flagglobal.so is not built"}); print(json.dumps(doc[-1]), flush=True)
exe = os.path.join(R, "cbc_amd", "csrc", "cbc")
if not rc:
    t = time.time()
    p = subprocess.run([exe, "-x", P("cfg2.cbc"), P("out.stats"), P("chr1.fa"), "--stats", "--verbose"], capture_output=True, text=True, timeout=600)
    doc.append({"cli": "cbc -x --stats", "rc": p.returncode, "wall_s": round(time.time() - t, 3),
                "out_bytes": os.path.getsize(P("out.stats")) if os.path.exists(P("out.stats")) else -1,
                "stdout": p.stdout.strip().splitlines(), "stderr": p.stderr[-500:]})
    print(json.dumps(doc[-1]), flush=True)
    rc = 1 if p.returncode else 0
for f in ("cfg2.cbc", "chr1.fa", "out.stats"):
    if os.path.exists(P(f)):
        os.remove(P(f))
if RESULT:
    with open(RESULT, "w") as f:
        json.dump(doc, f, indent=1); f.write("\n")
sys.exit(rc)
