"""A/B of the host packer across two builds of libcbc_host.so: python tools/packer_ab.py LIB_A LIB_B [n_reads] [runs]
The packer loop of tools/e2e.py (synthetic reads of 150 bases as SAM text, cbc_pack_sam with 1 and with 16 threads,
CBC_PACK_TIMES=1), one child process per library and run, A and B alternating.  Prints every wall time, the threaded packer's
own "scan" and "tokenise" phase times, and per library and thread count the median and the spread (max - min).
With --tokeniser the same scheme times enc.tokenise_sam (the device tokeniser, in process) for two builds of libcbc_gpu.so."""
import json, os, statistics, subprocess, sys, time

TEXT = os.path.join(os.environ.get("TMPDIR", "/tmp"), "cbc_packer_ab")


def one(lib, threads):
    sys.path.insert(0, ".")
    from cbc_amd import host
    host.HOST_LIB = lib
    sam, fa = open(TEXT + ".sam", "rb").read(), open(TEXT + ".fa", "rb").read()
    os.environ["CBC_PACK_TIMES"] = "1"
    for th in threads:
        t = time.time(); q = host.pack_sam(sam, fa, threads=th); dt = time.time() - t
        print(json.dumps(dict(threads=th, wall_s=round(dt, 4), n_recs=int(q.n_recs))), flush=True)
        del q


def one_tokeniser(lib):
    os.environ["CBC_GPU_LIB"] = lib
    sys.path.insert(0, ".")
    from cbc_amd import gpu
    sam, fa = open(TEXT + ".sam", "rb").read(), open(TEXT + ".fa", "rb").read()
    enc = gpu.Encoder(0)
    for rep in range(2):                              # the first one is the warm-up
        t = time.time(); pd, tr = enc.tokenise_sam(sam, fa); dt = time.time() - t
        enc.tokenise_free(tr); del pd
        print(json.dumps(dict(rep=rep, wall_s=round(dt, 4))), flush=True)
    enc.close()


def main(argv):
    tok = "--tokeniser" in argv
    argv = [a for a in argv if a != "--tokeniser"]
    libs = [os.path.abspath(a) for a in argv[:2]]
    n = int(argv[2]) if len(argv) > 2 else 4_000_000
    runs = int(argv[3]) if len(argv) > 3 else 3 if tok else 5
    sys.path.insert(0, ".")
    from cbc_amd import host
    _, sam, fa = host.synth(7, 200_000_000, n, want_text=True)
    open(TEXT + ".sam", "wb").write(sam); open(TEXT + ".fa", "wb").write(fa)
    print("text: %d reads, %.0f MB" % (n, len(sam) / 1e6), flush=True)
    del sam, fa
    res = {}
    try:
        for run in range(runs):
            for which, lib in zip("AB", libs):
                cmd = [sys.executable, os.path.abspath(__file__), "--one-tokeniser" if tok else "--one", lib]
                r = subprocess.run(cmd, capture_output=True, text=True, check=True, timeout=300)   # a child that hangs ends the chain
                phases = [l for l in r.stderr.splitlines() if l.startswith("pack_mt:")]
                for l in r.stdout.splitlines():
                    d = json.loads(l)
                    if tok:
                        if d["rep"]:
                            res.setdefault((which, "tokenise_sam"), []).append(d["wall_s"])
                        print(which, l, flush=True)
                        continue
                    res.setdefault((which, "wall", d["threads"]), []).append(d["wall_s"])
                    if d["threads"] > 1:
                        w = phases.pop(0).split()
                        res.setdefault((which, "scan", d["threads"]), []).append(float(w[2]))
                        res.setdefault((which, "tokenise", d["threads"]), []).append(float(w[6]))
                    print(which, "run", run, l, flush=True)
    finally:
        os.remove(TEXT + ".sam"); os.remove(TEXT + ".fa")
    for k in sorted(res, key=str):
        v = res[k]
        print(" ".join(str(x) for x in k), "all", v, "median %.4f spread %.4f" % (statistics.median(v), max(v) - min(v)), flush=True)


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--one":
        one(sys.argv[2], (1, 16))
    elif len(sys.argv) >= 3 and sys.argv[1] == "--one-tokeniser":
        one_tokeniser(sys.argv[2])
    else:
        main(sys.argv[1:])
