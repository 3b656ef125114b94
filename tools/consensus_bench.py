"""The consensus record beside the pileup: Encoder.decode_consensus and Encoder.decode_pileup of the same
container alternated in one job after a warm-up round, the bytes of every round identical -- first the `shared` dataset of the
tests (600 reads, 20 kb), then the cfg2 workload (10 M x 150 bp on a chr1-sized contig, 4096-read blocks; fewer reads when
asked).  Per call the four kernel times of cbc_gpu_last_consensus_ms / cbc_gpu_last_pileup_ms (device events: edits decode; zero +
mark + events; scans; text), medians over the rounds.  The pileup's figures are the comparison, not the code under test.
Prints one JSON line and, given a third argument, writes it to that file.
Usage: python tools/consensus_bench.py [reads] [rounds] [result.json]"""
import json, os, sys, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import pileupmodel as pm
import regionmodel as rm
import synth
from cbc_amd import gpu, host

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
RESULT = sys.argv[3] if len(sys.argv) > 3 else None
STRETCH = ("edits_decode", "zero_mark_events", "scans", "text")
med = lambda xs: float(np.median(xs))
enc = gpu.Encoder(0)


def measure(plan, n_recs):
    enc.upload_reference(plan.ref)
    cap = 256 << 20                                            # the pileup's bound grows with the window: ask for the text's own size
    try:
        enc.decode_pileup(plan, text_cap=cap)
    except gpu.CbcGpuError:
        cap = enc.last_pileup_text_bytes
    ms, wall, first, out = {"consensus": [], "pileup": []}, {"consensus": [], "pileup": []}, {}, {}
    for it in range(ROUNDS + 1):                               # round 0 is the warm-up (arenas grow, pages are touched)
        for name in ("consensus", "pileup"):
            t = time.time()
            if name == "consensus":
                text, cnt, kept = enc.decode_consensus(plan)
                m = enc.last_consensus_ms()
            else:
                text, cnt, kept, _ = enc.decode_pileup(plan, results=True, text_cap=cap)
                m = enc.last_pileup_ms()
            w = time.time() - t
            assert kept == n_recs
            if it == 0:
                first[name] = text
                out[name] = {"text_bytes": len(text), "counts" if name == "consensus" else "lines": cnt}
            else:
                assert text == first[name]                     # integer atomics commute: the same bytes every time
                ms[name].append(m); wall[name].append(w)
            del text
    c = out["consensus"]["counts"]
    assert sum(c[k] for k in ("ref", "alt", "del", "ambiguous", "low_depth", "no_call")) == sum(plan.contig_blocks(k).end for k in range(plan.n_contigs))
    for name in ("consensus", "pileup"):
        m = [med([x[k] for x in ms[name]]) for k in range(4)]
        out[name].update(ms={s: round(v, 3) for s, v in zip(STRETCH, m)}, post_decode_ms=round(sum(m[1:]), 3),
                         all=[[round(v, 3) for v in x] for x in ms[name]], wall_s_min=round(min(wall[name]), 3))
    return out


doc = {"rounds": ROUNDS, "note": "a single run on a shared machine"}
fa, sam, pb, _ = pm.shared()
plan = host.UnpackPlan(rm.container(pb), fa)
doc["shared"] = dict(reads=int(pb.n_recs), blocks=plan.n_blocks, **measure(plan, pb.n_recs))
plan.close(); pb.close()
pb = host.synth(0xCBC00002, 248_956_422, N, 150, block_reads=4096)
enc.upload_reference(pb.ref)
_, res, offs, flat = enc.encode_blocks(pb, want_payload_list=False)
assert (res["status"] == 0).all()
c = pb.contigs[0]
fa = synth.fasta_text([("chr1", pb.ref[int(c["ref_off"]): int(c["ref_off"]) + int(c["length"])])])
plan = host.UnpackPlan(pb.container(flat, offs), fa)
doc["cfg2"] = dict(reads=N, blocks=plan.n_blocks, **measure(plan, pb.n_recs))
print(json.dumps(doc))
enc.close()
if RESULT:
    with open(RESULT, "w") as f:
        json.dump(doc, f, indent=1); f.write("\n")
