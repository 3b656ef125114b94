"""Read statistics with the alignment tables at cfg2 size (10 M x 150 bp on a chr1-sized contig, 4096-read blocks; DESIGN.md
section 4.22).  In one process, Encoder.decode_stats and Encoder.decode_stats_aln alternated: one warm-up round of each (arenas
grow, code objects load), then `rounds` timed rounds of each, device events, medians.  The tables of every round must equal the
first round's, and the statistics tables of the two calls each other's.
  bar (i)  zeroing + statistics pass + alignment pass <= the edits-decode kernel of the same call (existing code: the yardstick)
Beside it, without a bar: the alignment pass against a streaming floor -- rows, reference, records and side words once at the
6.3 TB/s the microarchitecture guide gives as the achievable HBM rate -- and against the existing statistics pass.
Prints one JSON line per measurement and, given a third argument, writes them to that file as one JSON document.
Usage: python tools/stats_aln_bench.py [reads] [rounds] [result.json]"""
import json, os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import synth
from cbc_amd import gpu, host

HBM_TBS = 6.3
N = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
RESULT = sys.argv[3] if len(sys.argv) > 3 else None
med = lambda xs: float(np.median(xs))
r3 = lambda x: round(float(x), 3)


def key(t):
    return tuple(int(v) if np.isscalar(v) or isinstance(v, int) else np.asarray(v).tobytes() for _, v in sorted(t.items()))


pb = host.synth(0xCBC00002, 248_956_422, N, 150, block_reads=4096)
enc = gpu.Encoder(0)
enc.upload_reference(pb.ref)
_, res, offs, flat = enc.encode_blocks(pb, want_payload_list=False)
assert (res["status"] == 0).all()
c = pb.contigs[0]
clen = int(c["length"])
fa = synth.fasta_text([("chr1", pb.ref[int(c["ref_off"]): int(c["ref_off"]) + clen])])
plan = host.UnpackPlan(pb.container(flat, offs), fa)
enc.upload_reference(plan.ref)
plain_ms, aln_ms, first = [], [], None
for it in range(ROUNDS + 1):                                 # round 0 is the warm-up of both calls
    st = enc.decode_stats(plan)
    a = enc.last_stats_ms()
    st2, al = enc.decode_stats_aln(plan)
    b = enc.last_stats_aln_ms()
    assert key(st) == key(st2)                               # `out` equals decode_stats of the same selection
    if it == 0:
        first = (key(st), key(al), al)
    else:
        assert (key(st), key(al)) == first[:2]               # the tables of every round are identical
        plain_ms.append(a); aln_ms.append(b)
enc.close()
al = first[2]
assert al["reads"] + al["invalid"] == N and al["invalid"] == 0
nm = al["nm"].astype(np.int64)
edits = int(al["mm"].astype(np.int64).sum() + (np.arange(256) * al["ins_len"].astype(np.int64)).sum() + (np.arange(256) * al["del_len"].astype(np.int64)).sum())
assert int(nm.sum()) == N and int((np.arange(767) * nm).sum()) == edits
bases = int((np.arange(257) * al["len"].astype(np.int64)).sum())
streamed = N * plan.seq_stride + bases + N * 16 + N * 8       # rows, the reference bytes under them, records, side words
floor_ms = streamed / (HBM_TBS * 1e12) * 1e3
dec, stp, alp = ([x[i] for x in aln_ms] for i in range(3))
behind = [x[1] + x[2] for x in aln_ms]
doc = [{"case": "whole file, decode_stats and decode_stats_aln alternated", "reads": N, "blocks": plan.n_blocks, "rounds": ROUNDS,
        "seq_stride": plan.seq_stride, "reads_with_indels_percent": r3(100.0 * (int(al["ins_cyc"].sum()) + int(al["del_cyc"].sum())) / N),
        "mismatches": int(al["mm"].astype(np.int64).sum()), "stats_ms": [[r3(v) for v in x] for x in plain_ms],
        "stats_aln_ms": [[r3(v) for v in x] for x in aln_ms],
        "plain_decode_median_ms": r3(med([x[0] for x in plain_ms])), "plain_stats_median_ms": r3(med([x[1] for x in plain_ms])),
        "edits_decode_median_ms": r3(med(dec)), "stats_median_ms": r3(med(stp)), "aln_median_ms": r3(med(alp)),
        "aln_min_ms": r3(min(alp)), "aln_max_ms": r3(max(alp)),
        "bar_i_behind_the_decode_median_ms": r3(med(behind)), "bar_i_holds": bool(med(behind) <= med(dec)),
        "behind_over_decode": round(med(behind) / med(dec), 4),
        "streamed_bytes": streamed, "hbm_tb_per_s_assumed": HBM_TBS, "streaming_floor_ms": r3(floor_ms),
        "aln_over_floor": round(med(alp) / floor_ms, 2), "aln_over_existing_stats_pass": round(med(alp) / med([x[1] for x in plain_ms]), 2),
        "d2h_bytes_more": 4 * (5 * 257 + 767 + 4 * 256 + 2), "tables_identical_every_round": True}]
print(json.dumps(doc[-1]), flush=True)
if RESULT:
    with open(RESULT, "w") as f:
        json.dump(doc, f, indent=1); f.write("\n")
sys.exit(0 if doc[0]["bar_i_holds"] else 2)
