#!/usr/bin/env python3
"""Records what the `cbc` program prints, returns and writes for a fixed list of decode invocations:
tests/golden/cli_matrix.json (no device needed) and tests/golden/cli_matrix_gpu.json (recorded on an MI355X).

WHAT THESE ARE: regression vectors of the command line itself -- the order of main()'s refusals, the messages of every
decode mode and the bytes of its output file -- taken from the build of one commit so that a later change of
cbc_main.c / cbc_cli_unpack.c can be held against it.  tests/test_cli_golden.py and tests/test_cli_golden_gpu.py import
the case lists and the runner from this file, so the recorded and the tested invocations cannot drift apart.

The inputs are the files of tests/golden/cli/ (made once by --make-inputs; they are committed so that no random generator
stands between a recording and a later test).  Every case runs with copies of them in an empty directory, as cwd and with
relative names, because the messages quote the paths.

  python tests/golden/make_cli_matrix.py [--exe PATH]          the device-free matrix (run where no MI355X is visible:
                                                               cases that reach the device are dropped and listed)
  python tests/golden/make_cli_matrix.py --gpu [--exe PATH]    the device cases, on an MI355X
  python tests/golden/make_cli_matrix.py --make-inputs         tests/golden/cli/ from tests/regionmodel.py
"""
import argparse
import hashlib
import itertools
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
INPUTS = os.path.join(HERE, "cli")
EXE = os.path.join(ROOT, "cbc_amd", "csrc", "cbc")
CPU_JSON = os.path.join(HERE, "cli_matrix.json")
GPU_JSON = os.path.join(HERE, "cli_matrix_gpu.json")

OUTPUTS = ["--sam", "--depth", "--bedcov", "--depth-hist", "--stats"]
SELECTIONS = [[], ["--region", "chr1:100-200"], ["--region", "chr1:100-200", "--region", "chr2"],
              ["--regions-file", "normal.bed"], ["--region", "chr1:100-200", "--regions-file", "normal.bed"]]
OWNED = [["--window", "5"], ["--min-depth", "2"], ["--thresholds", "1,2"], ["--count-reads"], ["--hist-max", "3"],
         ["--depth-exclude-flags", "4"], ["--stats-exclude-flags", "4"]]
# every value parser with the output option that owns it, and the values held against each of them
PARSERS = [("--depth-exclude-flags", "--depth"), ("--stats-exclude-flags", "--stats"), ("--window", "--bedcov"),
           ("--min-depth", "--bedcov"), ("--hist-max", "--depth-hist"), ("--thresholds", "--bedcov")]
VALUES = ["", "x", "0", "1", "0x10", "-1", "65535", "65536", "4294967295", "4294967296", "1234567890123456789", "1,1", "2,1",
          "1,2,3,4,5,6,7,8", "1,2,3,4,5,6,7,8,9", "1,2,", ",1"]
# the decode modes that take several regions or a BED file, as the options that select them
SEVERAL = [[], ["--sam"], ["--depth"], ["--bedcov"], ["--depth-hist"], ["--stats"]]
ALL_MODES = SEVERAL                                          # with a single --region: the single-region functions too
EDITS_MODES = [["--pileup"], ["--sam", "--cigar"], ["--stats", "--alignment"]]
NOT_A_CONTAINER = ["stream.bin", "out.txt", "ref.fa"]
CONTAINER = ["reads.cbc", "out.txt", "ref.fa"]


def cpu_cases():
    """[(id, argv)]: everything that ends without a device on a machine that has none."""
    out, count = [], {}
    def add(tag, args):
        count[tag] = count.get(tag, 0) + 1
        out.append(("%s/%03d %s" % (tag, count[tag] - 1, " ".join(args)), list(args)))
    for k in range(len(OUTPUTS) + 1):
        for opts in itertools.combinations(OUTPUTS, k):
            for sel in SELECTIONS:
                for dev in ([], ["--devices", "0,1"]):
                    if opts or sel:
                        add("matrix", ["-x"] + list(opts) + sel + dev + NOT_A_CONTAINER)
    for o in [["--regions-file", "normal.bed"], ["--region", "chr1"]] + [[o] for o in OUTPUTS]:
        add("compress", ["-c"] + o + NOT_A_CONTAINER)
    for own in OWNED:
        for o in [[]] + [[o] for o in OUTPUTS]:
            add("owner", ["-x"] + own + o + NOT_A_CONTAINER)
        add("owner", ["-c"] + own + NOT_A_CONTAINER)
    for opt, owner in PARSERS:
        for v in VALUES:
            add("value", ["-x", owner, opt, v] + NOT_A_CONTAINER)
    run = ["-x", "--verbose"]
    def beds(mode):
        for bed in ("empty.bed", "unknown.bed", "missing.bed"):
            add("run", run + mode + ["--regions-file", bed] + CONTAINER)
    def regions(mode):
        for region in ("chrX", "chrX:5-9", "chr1:5-x", "chr1:9-5", "chr1:0-5", "chr1:1-1"):
            add("run", run + mode + ["--region", region] + CONTAINER)
        add("run", run + mode + ["--region", "chrX", "--region", "chr1:5-x"] + CONTAINER)
        for sel in ([["--region", "chr1"], ["--region", "chr1", "--region", "chr2"]] if not mode or mode[0] in ("--sam", "--depth")
                    else [["--region", "chr1"]]):
            add("run", run + mode + sel + ["missing.cbc", "out.txt", "ref.fa"])
            add("run", run + mode + sel + ["reads.cbc", "out.txt", "missing.fa"])
            add("run", run + mode + sel + ["reads.cbc", "no_such_dir/out.txt", "ref.fa"])
    for mode in SEVERAL:
        beds(mode)
    for bed in ("empty.bed", "unknown.bed"):
        add("run", run + ["--bedcov", "--window", "100", "--regions-file", bed] + CONTAINER)
        add("run", run + ["--bedcov", "--thresholds", "1,5", "--count-reads", "--regions-file", bed] + CONTAINER)
    for mode in ALL_MODES:
        regions(mode)
    # the modes behind the edits decoder came later: their cases stand behind the older ones, whose ids and order stay
    for mode in EDITS_MODES:
        beds(mode)
    for mode in EDITS_MODES:
        regions(mode)
    return out


def gpu_cases():
    """{mode: [(id, argv)]}: a few runs of every decode mode on the device, --verbose throughout."""
    run = ["-x", "--verbose"]
    modes = {
        "region": [["--region", "chr1:100-400"], ["--region", "chr2"], ["--region", "chr1:2600-2700"]],
        "sam": [["--sam"], ["--sam", "--region", "chr2:50-300"], ["--sam", "--region", "chr1:2600-2700"]],
        "depth": [["--depth"], ["--depth", "--region", "chr1:100-400"], ["--depth", "--depth-exclude-flags", "16"],
                  ["--depth", "--region", "chr2", "--depth-exclude-flags", "0x10"]],
        "targets": [["--region", "chr1:100-400", "--region", "chr2:50-300"], ["--regions-file", "late.bed"],
                    ["--sam", "--regions-file", "mixed.bed"], ["--depth", "--regions-file", "late.bed"],
                    ["--depth", "--regions-file", "normal.bed", "--region", "chr2:1500-1600", "--depth-exclude-flags", "16"]],
        "bedcov": [["--bedcov"], ["--bedcov", "--region", "chr1:100-400"], ["--bedcov", "--regions-file", "late.bed"],
                   ["--bedcov", "--regions-file", "mixed.bed", "--window", "500", "--min-depth", "2"],
                   ["--bedcov", "--regions-file", "normal.bed", "--depth-exclude-flags", "16"]],
        "bedcov_ext": [["--bedcov", "--thresholds", "1,5", "--count-reads"], ["--bedcov", "--count-reads", "--region", "chr2:50-300"],
                       ["--bedcov", "--thresholds", "2", "--regions-file", "late.bed"],
                       ["--bedcov", "--thresholds", "1,3,9", "--count-reads", "--regions-file", "mixed.bed", "--window", "700",
                        "--depth-exclude-flags", "16"]],
        "hist": [["--depth-hist"], ["--depth-hist", "--region", "chr1:100-400"], ["--depth-hist", "--regions-file", "late.bed"],
                 ["--depth-hist", "--regions-file", "mixed.bed", "--hist-max", "3", "--depth-exclude-flags", "16"]],
        "stats": [["--stats"], ["--stats", "--region", "chr1:100-400"], ["--stats", "--regions-file", "late.bed"],
                  ["--stats", "--regions-file", "mixed.bed", "--stats-exclude-flags", "16"]],
        "pileup": [["--pileup"], ["--pileup", "--region", "chr1:100-400"],
                   ["--pileup", "--min-alt", "2", "--max-edits-per-read", "32", "--depth-exclude-flags", "16"]],
        "sam_cigar": [["--sam", "--cigar"], ["--sam", "--cigar", "--region", "chr1:100-400"], ["--sam", "--cigar", "--region", "chr2:50-300"]],
        "stats_aln": [["--stats", "--alignment"], ["--stats", "--alignment", "--region", "chr1:100-400"],
                      ["--stats", "--alignment", "--regions-file", "late.bed"],
                      ["--stats", "--alignment", "--regions-file", "mixed.bed", "--stats-exclude-flags", "16"]],
    }
    return {m: [("%s/%d %s" % (m, i, " ".join(a)), run + a + CONTAINER) for i, a in enumerate(v)] for m, v in modes.items()}


_TIME = re.compile(r"\d+\.\d{3} (s|ms)")


def _short(text):
    """A text as the fixtures hold it: itself, or over 1 KiB its length and SHA-256 (the statistics tables, SAM text)."""
    if text is None or len(text) <= 1024:
        return text
    return "%d bytes, sha256 %s" % (len(text), hashlib.sha256(text.encode("latin-1")).hexdigest())


def run_case(exe, argv, workdir, prefix=()):
    """One invocation with workdir as cwd: a copy of the inputs (made on first use; the program only reads them) without an
    output file.  Returns what is compared, [exit code, stderr, stdout with the times masked, bytes of the output file (None:
    it does not exist)], the three texts as _short gives them."""
    if not os.path.exists(workdir):
        shutil.copytree(INPUTS, workdir)
    path = os.path.join(workdir, argv[-2])
    if os.path.exists(path):
        os.remove(path)
    p = subprocess.run(list(prefix) + [exe] + argv, cwd=workdir, capture_output=True, stdin=subprocess.DEVNULL)
    data = None
    if os.path.exists(path):
        with open(path, "rb") as f:
            data = f.read().decode("latin-1")
    return [p.returncode, _short(p.stderr.decode("latin-1")), _short(_TIME.sub(r"T \1", p.stdout.decode("latin-1"))), _short(data)]


def make_inputs():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import regionmodel as rm
    fa, rbc, _ = rm.mixed_dataset(11, [3000, 2000], [200, 120], lengths=(100,), gap_tail=600, sub_rate=0.004, indel_frac=0.3)
    pb = rm.pack(fa, rbc, 64)
    files = {
        "reads.cbc": bytes(rm.container(pb)), "ref.fa": fa, "stream.bin": b"not a block container\n",
        "empty.bed": b"chr1\t100\t100\n", "unknown.bed": b"chrX\t0\t100\n",
        "normal.bed": b"chr1\t100\t400\nchr2\t50\t300\nchr1\t350\t600\n",
        # nothing selected on the first contig, so the device is opened for the second
        "late.bed": b"chr1\t500\t500\nchr2\t50\t300\nchr2\t1000\t1200\n",
        # a contig the container does not list between two it does
        "mixed.bed": b"chr2\t50\t300\nchrUn\t10\t90\nchr1\t100\t400\nchr1\t2500\t2700\n",
    }
    os.makedirs(INPUTS, exist_ok=True)
    for name, data in files.items():
        with open(os.path.join(INPUTS, name), "wb") as f:
            f.write(data)
    print("%d reads in %d blocks, container %d bytes, FASTA %d bytes" % (pb.n_recs, pb.n_blocks, len(files["reads.cbc"]), len(fa)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--exe", default=EXE)
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--make-inputs", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.make_inputs:
        return make_inputs()
    exe = os.path.abspath(a.exe)
    # the fixture: every distinct result once, and per group of cases the index of each case's result, in the order of the
    # case list (-1: dropped, the run needs a device)
    results, cases, dropped = [], {}, []
    with tempfile.TemporaryDirectory() as tmp:
        work = os.path.join(tmp, "w")
        groups = gpu_cases() if a.gpu else {}
        for cid, argv in ([] if a.gpu else cpu_cases()):
            groups.setdefault(cid.split("/")[0], []).append((cid, argv))
        for tag, lst in groups.items():
            for cid, argv in lst:
                # on the device every run has its own time limit, and the recording stops at the first status a healthy run cannot give
                r = run_case(exe, argv, work, prefix=("timeout", "-k", "10", "60") if a.gpu else ())
                if a.gpu and r[0] != 0:
                    sys.exit("%s: exit status %d\n%s" % (cid, r[0], r[1]))
                if "no usable MI355X" in r[1]:
                    dropped.append(cid)
                    r = None
                elif r not in results:
                    results.append(r)
                cases.setdefault(tag, []).append(-1 if r is None else results.index(r))
    print("%d cases, %d distinct results, %d dropped for needing a device:" % (sum(map(len, cases.values())), len(results), len(dropped)))
    for d in dropped:
        print("  " + d)
    with open(a.out or (GPU_JSON if a.gpu else CPU_JSON), "w") as f:
        f.write('{"results": [\n' + ",\n".join(json.dumps(r) for r in results) + '\n],\n"cases": ' + json.dumps(cases, sort_keys=True)
                + ',\n"dropped": ' + json.dumps(dropped) + "}\n")


if __name__ == "__main__":
    main()
