"""SAM output with CIGAR, NM and MD at cfg2 size (10 M x 150 bp on a chr1-sized contig, 4096-read blocks; DESIGN.md section
4.21): the whole container through Encoder.decode_sam (plain decode, count + scan, text) and through
Encoder.decode_sam(cigar=True) (edits decode, measure, count + scan, text), alternated after a warm-up round, device-event times,
medians of the rounds; the bytes of every round must be identical, and the lines minus CIGAR and tags must be the plain lines.
Bar (i): measure + count + scan + text of the --cigar call <= its edits decode.  Then `cbc -x --sam --cigar` beside `cbc -x
--sam` with files in a directory of your choice (/dev/shm for the numbers in DESIGN.md).  Prints one JSON line per measurement;
with a fourth argument the first line is also written to that file.
Usage: python tools/sam_cigar_bench.py [reads] [out_dir] [rounds] [json_out]"""
import hashlib, json, os, subprocess, sys, tempfile, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import synth
from cbc_amd import gpu, host

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
OUT = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp()
ROUNDS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
JSON_OUT = sys.argv[4] if len(sys.argv) > 4 else None
say = lambda *a: print(*a, file=sys.stderr, flush=True)
pb = host.synth(0xCBC00002, 248_956_422, N, 150, block_reads=4096)
say("workload made")
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
say("container made: %d blocks" % plan.n_blocks)
sam_ms, cig_ms, sam_wall, cig_wall, sums = [], [], [], [], set()
for it in range(ROUNDS + 1):                                   # round 0 is the warm-up (arenas grow, pages are touched)
    t = time.time(); sam, n, _, r = enc.decode_sam(plan, results=True); w = time.time() - t
    assert (r["status"] == 0).all() and n == pb.n_recs
    sm_ = enc.last_sam_ms(); sam_bytes = len(sam) - len(hdr)
    t = time.time(); cig, n2, _, r = enc.decode_sam(plan, results=True, cigar=True); w2 = time.time() - t
    assert (r["status"] == 0).all() and n2 == pb.n_recs
    cm_ = enc.last_sam_cigar_ms(); cig_bytes = len(cig) - len(hdr)
    sums.add((hashlib.sha256(sam).hexdigest(), hashlib.sha256(cig).hexdigest()))
    if it == 0:                                                # minus CIGAR and tags: the plain lines, line for line
        a = [ln.split(b"\t") for ln in cig[len(hdr):len(hdr) + 40_000_000].split(b"\n")[:-1]]
        b = sam[len(hdr):].split(b"\n", len(a))[:len(a)]
        assert all(len(x) == 13 and x[5] != b"*" for x in a)
        assert [b"\t".join(x[:5] + [b"*"] + x[6:11]) for x in a] == b
        kinds = {"lines_checked": len(a), "with_I": sum(b"I" in x[5] for x in a), "with_D": sum(b"D" in x[5] for x in a),
                 "with_S": sum(b"S" in x[5] for x in a), "NM_0": sum(x[11] == b"NM:i:0" for x in a)}
        del a, b
    del sam, cig
    say("round %d: sam %s ms, sam --cigar %s ms" % (it, [round(v, 2) for v in sm_], [round(v, 2) for v in cm_]))
    if it:
        sam_ms.append(sm_); cig_ms.append(cm_); sam_wall.append(w); cig_wall.append(w2)
assert len(sums) == 1, "the bytes differ between rounds"
med = lambda xs: float(np.median(xs))
dec, meas, cnt, txt = (med([x[i] for x in cig_ms]) for i in range(4))
line = {"reads": N, "blocks": plan.n_blocks, "rounds": ROUNDS, "sam_text_bytes": sam_bytes, "sam_cigar_text_bytes": cig_bytes,
        "first_lines": kinds,
        "sam_ms": {"decode": round(med([x[0] for x in sam_ms]), 3), "count_scan": round(med([x[1] for x in sam_ms]), 3),
                   "text": round(med([x[2] for x in sam_ms]), 3), "all": [[round(v, 3) for v in x] for x in sam_ms]},
        "sam_cigar_ms": {"edits_decode": round(dec, 3), "measure": round(meas, 3), "count_scan": round(cnt, 3), "text": round(txt, 3),
                         "all": [[round(v, 3) for v in x] for x in cig_ms]},
        "behind_decode_ms": round(meas + cnt + txt, 3), "bar_i_holds": bool(meas + cnt + txt <= dec),
        "text_ratio_cigar_over_plain": round(txt / med([x[2] for x in sam_ms]), 3),
        "sam_wall_s_min": round(min(sam_wall), 3), "sam_cigar_wall_s_min": round(min(cig_wall), 3)}
print(json.dumps(line))
if JSON_OUT:
    open(JSON_OUT, "w").write(json.dumps(line, indent=1) + "\n")
enc.close()
os.makedirs(OUT, exist_ok=True)
open(os.path.join(OUT, "cfg2.cbc"), "wb").write(blob); open(os.path.join(OUT, "chr1.fa"), "wb").write(fa)
exe = os.path.join(R, "cbc_amd", "csrc", "cbc")
for name, extra in [("cbc -x --sam", ["--sam", "--verbose"]), ("cbc -x --sam --cigar", ["--sam", "--cigar", "--verbose"])]:
    t = time.time()
    p = subprocess.run([exe, "-x", os.path.join(OUT, "cfg2.cbc"), os.path.join(OUT, "out.sam"), os.path.join(OUT, "chr1.fa")] + extra,
                       capture_output=True, text=True, timeout=900)
    print(json.dumps({"cli": name, "rc": p.returncode, "wall_s": round(time.time() - t, 3),
                      "out_bytes": os.path.getsize(os.path.join(OUT, "out.sam")) if os.path.exists(os.path.join(OUT, "out.sam")) else -1,
                      "stdout": p.stdout.strip().splitlines(), "stderr": p.stderr[-500:]}))
for f in ("cfg2.cbc", "chr1.fa", "out.sam"):
    if os.path.exists(os.path.join(OUT, f)):
        os.remove(os.path.join(OUT, f))
