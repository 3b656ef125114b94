"""Same-box A/B of host-buffer calls across source trees (each already built): python tools/host_ab.py ROOT...
For each tree, in its own process: cfg2 through cbc_gpu_encode_blocks_2bit (12 calls) and cbc_gpu_encode_blocks (6 calls) with
the arrays page-locked, and cbc_gpu_long_encode_blocks / cbc_gpu_long_decode_blocks on a 4 k x 10 kb batch (6 calls each).
Prints one JSON line per tree: min / median ms, every 2-bit call, and the long calls' times."""
import json, os, statistics, subprocess, sys, time


def one(root):
    sys.path.insert(0, root)
    from cbc_amd import host, gpu
    ms = lambda v: (round(min(v) * 1e3, 2), round(statistics.median(v) * 1e3, 2))
    out = {"tree": os.path.basename(os.path.abspath(root))}
    pb = host.synth(0xCBC00002, 248956422, 10_000_000, 150, block_reads=4096)
    sc, sr = host.pack_2bit(pb.seq)
    enc = gpu.Encoder(0)
    enc.upload_reference(pb.ref)
    for a in (pb.recs, pb.seq, pb.tok, sc):
        enc.host_register(a)
    t2, t1 = [], []
    for _ in range(12):
        t = time.time(); _, r2, o2, f2 = enc.encode_blocks_2bit(pb, sc, sr, want_payload_list=False); t2.append(time.time() - t)
    out["chunks"] = enc.last_e2e()["n_chunks"]
    for _ in range(6):
        t = time.time(); _, r1, o1, f1 = enc.encode_blocks(pb, want_payload_list=False); t1.append(time.time() - t)
    assert (r1["status"] == 0).all() and (r2["status"] == 0).all() and (f1 == f2).all()
    out.update(two_bit_min_med_ms=ms(t2), one_byte_min_med_ms=ms(t1), two_bit_all_ms=[round(x * 1e3, 1) for x in t2])
    for a in (pb.recs, pb.seq, pb.tok, sc):
        enc.host_unregister(a)
    enc.close()
    del pb, sc, sr
    pl, sam, fa = host.synth_long(0xCBC00005, 20_000_000, 4_000, 10_000, 0.05, want_text=True)
    enc = gpu.Encoder(0)
    enc.upload_reference(pl.ref)
    te, td = [], []
    for _ in range(6):
        t = time.time(); _, res, offs, flat = enc.encode_long_blocks(pl); te.append(time.time() - t)
    plan = host.UnpackPlan(pl.container(flat, offs), fa)
    enc.upload_reference(plan.ref)
    for _ in range(6):
        t = time.time(); _, _, dres = enc.decode_long_blocks(plan); td.append(time.time() - t)
    assert (res["status"] == 0).all() and (dres["status"] == 0).all()
    out.update(long_encode_ms=[round(x * 1e3, 1) for x in te], long_decode_ms=[round(x * 1e3, 1) for x in td])
    enc.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--one":
        one(sys.argv[2])
    else:
        for root in sys.argv[1:]:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--one", root], check=True)
