"""Region decode at cfg2 size (10 M x 150 bp on a chr1-sized contig, block container of 4096-read blocks): a 10 kb locus
and the whole contig through Encoder.decode_region (wall time + the three kernels: span decode, filter + scan, text), the
plain decode kernel of the same blocks for comparison, and `cbc -x --region` for the 10 kb locus (its --verbose stage times:
device init dominates).  Usage: python tools/region_bench.py [reads] [out_dir]"""
import json, os, subprocess, sys, tempfile, time
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
import numpy as np
import synth
from cbc_amd import gpu, host

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
OUT = sys.argv[2] if len(sys.argv) > 2 else tempfile.mkdtemp()
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
clen = int(c["length"])
mid = clen // 2
for name, region in [("10kb", "chr1:%d-%d" % (mid, mid + 9999)), ("whole_contig", "chr1")]:
    walls = []
    for _ in range(3):
        t = time.time(); text, nsel, sel, r = enc.decode_region(plan, region, results=True); walls.append(time.time() - t)
        assert (r["status"] == 0).all()
    dec, flt, txt = enc.last_region_ms()
    print(json.dumps({"region": name, "blocks": sel.b1 - sel.b0, "of_blocks": plan.n_blocks, "reads": nsel, "text_bytes": len(text),
                      "wall_s_min": round(min(walls), 4), "decode_ms": round(dec, 3), "filter_scan_ms": round(flt, 3),
                      "text_ms": round(txt, 3), "filter_plus_text_pct_of_decode": round(100 * (flt + txt) / dec, 2)}))
# the plain decoder over every block, one launch (device pointers; what bench.py --mode decode times)
recs, seq, r = enc.decode_blocks(plan)
assert (r["status"] == 0).all()
full_text = plan.text(recs, seq)
assert full_text == text, "whole-contig region text differs from the full decode"
print(json.dumps({"full_decode_host_path": enc.last_e2e()}))
enc.close()
os.makedirs(OUT, exist_ok=True)
open(os.path.join(OUT, "cfg2.cbc"), "wb").write(blob); open(os.path.join(OUT, "chr1.fa"), "wb").write(fa)
exe = os.path.join(R, "cbc_amd", "csrc", "cbc")
for region in ["chr1:%d-%d" % (mid, mid + 9999)]:
    t = time.time()
    p = subprocess.run([exe, "-x", os.path.join(OUT, "cfg2.cbc"), os.path.join(OUT, "region.txt"), os.path.join(OUT, "chr1.fa"),
                        "--region", region, "--verbose"], capture_output=True, text=True, timeout=600)
    print(json.dumps({"cli_region": region, "rc": p.returncode, "wall_s": round(time.time() - t, 3), "stdout": p.stdout.strip().splitlines(),
                      "stderr": p.stderr[-500:]}))
for f in ("cfg2.cbc", "chr1.fa", "region.txt"):
    if os.path.exists(os.path.join(OUT, f)):
        os.remove(os.path.join(OUT, f))
