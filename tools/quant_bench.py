"""Per-query depth quantiles at cfg2 size (10 M x 150 bp on a chr1-sized contig, 4096-read blocks).
The whole contig cut three ways -- windows of 1000 bases (about 80 runs per query: the table form), windows of 100 (the register
form) and the contig as one query (millions of runs walked by one wavefront: the known limit) -- with the quantiles 25, 50, 75:
the plain Encoder.decode_coverage and the quantile call alternated in one job after a warm-up round, medians of the rounds,
device events.  Reported: the selection pass against the plain call's kernel time behind the decode taken in the same job (a
ratio, no bar: there is no earlier implementation to derive one from), and against the decode kernel in front of it.  Checked
in every round: sum and covered of the two calls are equal; on the way: the whole-contig quantiles equal those derived from the
bins of Encoder.decode_depth_hist.  Prints one JSON line per measurement and, given a third argument, writes them to that file
as one JSON document.
Usage: python tools/quant_bench.py [reads] [rounds] [result.json]"""
import json, os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import synth
from cbc_amd import gpu, host

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
RESULT = sys.argv[3] if len(sys.argv) > 3 else None
PCT = (25, 50, 75)
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
med = lambda xs: float(np.median(xs))
PLAIN = ("mark", "scan_compact", "weights", "weight_scans", "prefixes", "lookup")


def rank(p, n):
    return max(1, -((-p * n) // 100))


# the whole contig's quantiles from the depth histogram, a path that shares none of the new code
(hc, hdepth, hbases, hsize), = enc.decode_depth_hist(plan)
cum = np.cumsum(hbases.astype(np.int64))
assert int(cum[-1]) == hsize == clen
hist_q = [int(hdepth[int(np.searchsorted(cum, rank(p, clen)))]) for p in PCT]
doc = []
for case, window in (("windows", 1000), ("windows", 100), ("one query", 0)):
    qs = plan.queries(window=window) if window else plan.queries()
    p_ms, q_ms, first = [], [], None
    for it in range(ROUNDS + 1):                               # round 0 is the warm-up (arenas grow, pages are touched)
        _, s0, e0, total, covered = enc.decode_coverage(plan, qs)
        m1 = enc.last_coverage_ms()
        _, s0, e0, qtotal, qcovered, quant = enc.decode_coverage_quant(plan, qs, PCT)
        m2 = enc.last_coverage_quant_ms()
        assert (total == qtotal).all() and (covered == qcovered).all()
        assert (quant[:, :-1] <= quant[:, 1:]).all()
        if first is None:
            first = quant.copy()
            if not window:
                assert quant.tolist() == [hist_q], (quant.tolist(), hist_q)
        else:
            assert (quant == first).all()
            p_ms.append(m1); q_ms.append(m2)
    plain = [med([x[1 + k] for x in p_ms]) for k in range(6)]
    dec, sel = med([x[0] for x in q_ms]), med([x[12] for x in q_ms])
    doc.append({"case": case, "window": window, "queries": qs.n_q, "reads": N, "blocks": plan.n_blocks, "rounds": ROUNDS, "quantiles": list(PCT),
                "plain_ms": [[round(v, 3) for v in x] for x in p_ms], "quant_ms": [[round(v, 3) for v in x] for x in q_ms],
                "plain_passes_ms": {n: round(v, 3) for n, v in zip(PLAIN, plain)}, "plain_non_decode_ms": round(sum(plain), 3),
                "decode_ms": round(dec, 3), "selection_ms": round(sel, 3), "selection_over_plain_non_decode": round(sel / sum(plain), 3),
                "selection_over_decode": round(sel / dec, 3), "selection_exceeds_decode": bool(sel > dec),
                "median_of_medians": int(np.median(first[:, 1])), "whole_contig_quantiles_from_histogram": hist_q})
    print(json.dumps(doc[-1]), flush=True)
enc.close()
if RESULT:
    with open(RESULT, "w") as f:
        json.dump(doc, f, indent=1); f.write("\n")
