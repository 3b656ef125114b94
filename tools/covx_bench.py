"""Per-query read counts and depth thresholds at cfg2 size (10 M x 150 bp on a chr1-sized contig, 4096-read blocks; DESIGN.md
section 4.17).
1. The whole contig cut into windows of 1000 and of 100 bases: the plain Encoder.decode_coverage and the extended call (four
   thresholds and count_reads) alternated in one job after a warm-up round, medians of the rounds, device events.  The extended
   call's kernel time behind the decode may be at most 3 x the plain call's as measured in the same job; on a miss the pass that
   carries it is named.  Checked on the way: sum and covered of the two calls are equal, the threshold-1 column adds up to the
   covered length of the bedGraph of Encoder.decode_depth, the read count of the whole contig is the number of kept reads.
2. `cbc -x --bedcov --thresholds 10,20,30 --count-reads --regions-file` for a 2000-line panel beside the plain `--bedcov`.
Every CLI step runs under its own time limit and the script stops at the first failure.  Prints one JSON line per measurement
and, given a fourth argument, writes them to that file as one JSON document.
Usage: python tools/covx_bench.py [reads] [out_dir] [rounds] [result.json]"""
import json, os, subprocess, sys, tempfile, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import synth
from cbc_amd import gpu, host

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
OUT = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp()
ROUNDS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
RESULT = sys.argv[4] if len(sys.argv) > 4 else None
THR = (1, 5, 10, 20)
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
PLAIN = ("mark", "scan_compact", "weights", "weight_scans", "prefixes", "lookup")
EXT = PLAIN + ("start_points", "thr_weights", "thr_scans", "thr_prefixes", "thr_read_lookup")
doc = []
# the whole contig as one query: its read count is every kept read
out = enc.decode_coverage(plan, plan.queries(), thresholds=THR, count_reads=True)
assert out[6].tolist() == [N], out[6]
text = enc.decode_depth(plan, "chr1")
rows = np.array([ln.split(b"\t")[1:] for ln in text.split(b"\n")[:-1]], dtype=np.int64)
del text
track_len = int((rows[:, 1] - rows[:, 0]).sum())
assert int(out[5][0][0]) == track_len and int(out[3][0]) == int(((rows[:, 1] - rows[:, 0]) * rows[:, 2]).sum())
del rows
for window in (1000, 100):
    qs = plan.queries(window=window)
    p_ms, x_ms = [], []
    for it in range(ROUNDS + 1):                               # round 0 is the warm-up (arenas grow, pages are touched)
        _, s0, e0, total, covered = enc.decode_coverage(plan, qs)
        m1 = enc.last_coverage_ms()
        _, s0, e0, xtotal, xcovered, xthr, xrd = enc.decode_coverage(plan, qs, thresholds=THR, count_reads=True)
        m2 = enc.last_coverage_ext_ms()
        assert (total == xtotal).all() and (covered == xcovered).all()
        if it == 0:
            assert int(xthr[:, 0].sum()) == track_len == int(covered.sum())
            assert (xthr[:, :-1] >= xthr[:, 1:]).all() and int(xrd.sum()) >= N and int(xrd.max()) > 0
            first = (xthr.copy(), xrd.copy())
        else:
            assert (xthr == first[0]).all() and (xrd == first[1]).all()
            p_ms.append(m1); x_ms.append(m2)
    plain = [med([x[1 + k] for x in p_ms]) for k in range(6)]
    ext = [med([x[1 + k] for x in x_ms]) for k in range(11)]
    hold = sum(ext) <= 3.0 * sum(plain)
    added = [ext[0] - plain[0]] + ext[6:]                      # the second list_add of the mark, then the passes of their own
    doc.append({"case": "whole contig in windows", "window": window, "queries": qs.n_q, "reads": N, "blocks": plan.n_blocks, "rounds": ROUNDS,
                "thresholds": list(THR), "plain_ms": [[round(v, 3) for v in x] for x in p_ms], "ext_ms": [[round(v, 3) for v in x] for x in x_ms],
                "plain_passes_ms": {n: round(v, 3) for n, v in zip(PLAIN, plain)}, "ext_passes_ms": {n: round(v, 3) for n, v in zip(EXT, ext)},
                "plain_non_decode_ms": round(sum(plain), 3), "ext_non_decode_ms": round(sum(ext), 3), "ratio": round(sum(ext) / sum(plain), 3),
                "bar_limit_ms": round(3.0 * sum(plain), 3), "bar_holds": bool(hold),
                "largest_added_pass": (("mark_starts",) + EXT[6:])[int(np.argmax(added))]})
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
                          ("cbc -x --bedcov --thresholds 10,20,30 --count-reads --regions-file",
                           ["--bedcov", "--thresholds", "10,20,30", "--count-reads", "--regions-file", P("panel.bed"), "--verbose"], "out.covx")]:
    t = time.time()
    p = subprocess.run([exe, "-x", P("cfg2.cbc"), P(outf), P("chr1.fa")] + extra, capture_output=True, text=True, timeout=600)
    doc.append({"cli": name, "rc": p.returncode, "wall_s": round(time.time() - t, 3),
                "out_bytes": os.path.getsize(P(outf)) if os.path.exists(P(outf)) else -1,
                "stdout": p.stdout.strip().splitlines(), "stderr": p.stderr[-500:]})
    print(json.dumps(doc[-1]), flush=True)
    if p.returncode:                                           # stop at the first failure: nothing more is started on the device
        rc = 1
        break
if rc == 0:                                                    # the first six columns of the two outputs are the same bytes
    a = [ln.split(b"\t") for ln in open(P("out.cov"), "rb").read().split(b"\n")[:-1]]
    b = [ln.split(b"\t") for ln in open(P("out.covx"), "rb").read().split(b"\n")[:-1]]
    assert len(a) == len(b) == 2000 and all(x == y[:6] and len(y) == 10 for x, y in zip(a, b))
for f in ("cfg2.cbc", "chr1.fa", "panel.bed", "out.cov", "out.covx"):
    if os.path.exists(P(f)):
        os.remove(P(f))
if RESULT:
    with open(RESULT, "w") as f:
        json.dump(doc, f, indent=1); f.write("\n")
sys.exit(rc)
