"""Same-box A/B of WHOLE launches: python tools/ab_launch.py <rounds> <reads,reads,...> lib1.so lib2.so ...
Each build of libcbc_gpu.so (from scratch/abl/) codes cfg2's generator at each size in its own process, all blocks in ONE launch
through the device-pointer entry point -- what bench.py times.  (tools/ab.py goes through the host-buffer call, which cuts 10 M
reads into chunks: its figure is the last chunk's kernel, a launch of a few blocks per CU, and the two regimes can disagree --
profiles/fused_steps_ab.log.)  Prints median / min / max kernel ms of 7 launches after 2 warm-up ones, failed blocks, payload
bytes and a hash of the output area; libraries alternate within a round; stops at the first child that fails."""
import sys, os, subprocess
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
code = r'''
import sys, os, ctypes, hashlib
sys.path.insert(0, %r)
import numpy as np, torch
from cbc_amd import host, gpu
NR = int(sys.argv[1])
pb = host.synth(0xCBC00002, 248956422, NR, 150, block_reads=4096)
enc = gpu.Encoder(0); L = gpu.lib(); dev = torch.device('cuda', 0)
blocks = pb.blocks.copy()
total = int(L.cbc_gpu_plan_output(blocks.ctypes.data, pb.n_blocks, pb.recs.ctypes.data, pb.tok.ctypes.data))
td = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)
d = [td(x) for x in (pb.recs, pb.seq, pb.tok, pb.names, blocks, pb.ref)]
d_out = torch.zeros(total, dtype=torch.uint8, device=dev); d_res = torch.zeros(pb.n_blocks * 16, dtype=torch.uint8, device=dev)
db = gpu.DeviceBatch(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), pb.n_blocks, d[5].data_ptr(), d[5].numel(),
                     d_out.data_ptr(), total, d_res.data_ptr(), d[1].numel(), pb.n_tok, pb.n_recs, host.LdsCaps(pb.cap_pos, pb.cap_var))
st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
ts = []
for _ in range(9):
    enc.encode_device(db, st); torch.cuda.synchronize(); ts.append(enc.last_kernel_ms())
res = d_res.cpu().numpy().view(host.RESULT_DTYPE)
ts = sorted(ts[2:])
print("RESULT median %%.4f min %%.4f max %%.4f" %% (ts[len(ts) // 2], ts[0], ts[-1]), "failed", int((res["status"] != 0).sum()), "bytes", int(res["nbytes"].sum()),
      "sha", hashlib.sha256(d_out.cpu().numpy().tobytes()).hexdigest()[:12])
''' % R
rounds, sizes, libs = int(sys.argv[1]), [int(x) for x in sys.argv[2].split(",")], sys.argv[3:]
for rnd in range(rounds):
    for reads in sizes:
        for lib in libs:
            env = dict(os.environ, CBC_GPU_LIB=os.path.join(R, "scratch", "abl", lib))
            r = subprocess.run([sys.executable, "-c", code, str(reads)], env=env, capture_output=True, text=True, timeout=240)
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT")]
            print("round %d %-14s reads %9d  %s" % (rnd, lib, reads, line[0][7:] if line else "FAILED rc=%d %s" % (r.returncode, r.stderr[-400:])), flush=True)
            if r.returncode != 0 or not line:
                sys.exit(1)
