"""SAM output at cfg2 size (10 M x 150 bp on a chr1-sized contig, 4096-read blocks): the whole
container through Encoder.decode_sam (the three kernel times: plain decode, count + scan, text) next to the region text pass
over the whole contig (Encoder.decode_region, the yardstick of bar 2: SAM text ms <= 2 * r * region text ms with r = SAM text
bytes / region text bytes), alternated after a warm-up; then `cbc -x --sam` against `cbc -x` with files in a directory of
your choice (/dev/shm for the numbers in DESIGN.md).  Prints one JSON line per measurement.
Usage: python tools/sam_bench.py [reads] [out_dir] [rounds]"""
import json, os, subprocess, sys, tempfile, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import synth
from cbc_amd import gpu, host

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
OUT = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp()
ROUNDS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
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
sam_ms, reg_ms, sam_wall, reg_wall = [], [], [], []
for it in range(ROUNDS + 1):                                   # round 0 is the warm-up (arenas grow, pages are touched)
    t = time.time(); text, nsel, sel, r = enc.decode_region(plan, "chr1", results=True); w = time.time() - t
    assert (r["status"] == 0).all() and nsel == pb.n_recs
    rm_ = enc.last_region_ms(); reg_bytes = len(text)
    if it == 0:
        seqs = text
    del text
    t = time.time(); sam, n, _, r = enc.decode_sam(plan, results=True); w2 = time.time() - t
    assert (r["status"] == 0).all() and n == pb.n_recs
    sm_ = enc.last_sam_ms(); sam_bytes = len(sam) - len(hdr)
    if it == 0:                                                # SEQ column == the region pass's text, line for line
        a = [ln.split(b"\t")[9] for ln in sam[len(hdr):len(hdr) + 50_000_000].split(b"\n")[:-1]]
        assert a == seqs.split(b"\n")[:len(a)]
        del seqs, a
    del sam
    if it:
        sam_ms.append(sm_); reg_ms.append(rm_); sam_wall.append(w2); reg_wall.append(w)
ratio = sam_bytes / reg_bytes
med = lambda xs: float(np.median(xs))
sam_text, reg_text = med([x[2] for x in sam_ms]), med([x[2] for x in reg_ms])
print(json.dumps({"reads": N, "blocks": plan.n_blocks, "rounds": ROUNDS, "sam_text_bytes": sam_bytes, "region_text_bytes": reg_bytes,
                  "r": round(ratio, 4),
                  "sam_ms": {"decode": round(med([x[0] for x in sam_ms]), 3), "count_scan": round(med([x[1] for x in sam_ms]), 3),
                             "text": round(sam_text, 3), "text_all": [round(x[2], 3) for x in sam_ms]},
                  "region_ms": {"span_decode": round(med([x[0] for x in reg_ms]), 3), "filter_scan": round(med([x[1] for x in reg_ms]), 3),
                                "text": round(reg_text, 3), "text_all": [round(x[2], 3) for x in reg_ms]},
                  "bar2_limit_ms": round(2 * ratio * reg_text, 3), "bar2_holds": bool(sam_text <= 2 * ratio * reg_text),
                  "sam_wall_s_min": round(min(sam_wall), 3), "region_wall_s_min": round(min(reg_wall), 3)}))
enc.close()
os.makedirs(OUT, exist_ok=True)
open(os.path.join(OUT, "cfg2.cbc"), "wb").write(blob); open(os.path.join(OUT, "chr1.fa"), "wb").write(fa)
exe = os.path.join(R, "cbc_amd", "csrc", "cbc")
for name, extra, outf in [("cbc -x", [], "out.txt"), ("cbc -x --sam", ["--sam", "--verbose"], "out.sam")]:
    t = time.time()
    p = subprocess.run([exe, "-x", os.path.join(OUT, "cfg2.cbc"), os.path.join(OUT, outf), os.path.join(OUT, "chr1.fa")] + extra,
                       capture_output=True, text=True, timeout=900)
    print(json.dumps({"cli": name, "rc": p.returncode, "wall_s": round(time.time() - t, 3),
                      "out_bytes": os.path.getsize(os.path.join(OUT, outf)) if os.path.exists(os.path.join(OUT, outf)) else -1,
                      "stdout": p.stdout.strip().splitlines(), "stderr": p.stderr[-500:]}))
for f in ("cfg2.cbc", "chr1.fa", "out.txt", "out.sam"):
    if os.path.exists(os.path.join(OUT, f)):
        os.remove(os.path.join(OUT, f))
