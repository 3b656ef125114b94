#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of libcbc_gpu.so, kernel by kernel.

    tools/isa_diff.py TREE_A TREE_B [-DNAME[=VALUE] ...] [--keep DIR] [-j N]
    tools/isa_diff.py A.s B.s

Given two source trees, it compiles every GPU translation unit of each -- the GPU_UNITS of that tree's cbc_amd/csrc/Makefile, or
cbc_gpu.hip alone where the Makefile names none -- with the Makefile's HIPFLAGS plus `--cuda-device-only -S` and the -D flags
given (both trees and all units get the same), then compares the kernels of all of a tree's listings with those of the
other's, by name: which unit holds a kernel does not matter; given two .s files it compares those.  Per kernel (a symbol with an .amdhsa_kernel descriptor) the
instruction lines are taken between the kernel's label and its .Lfunc_end: comments and assembler directives are dropped
and the numbers of the .LBB branch labels are replaced by their order of first appearance, so that only the instructions
and the control flow between them are compared.  Kernels that differ are listed with their instruction-line counts and the
register / scratch / LDS lines of their descriptors on both sides.  Exit status 0: every kernel identical; 1: a difference
(a kernel missing on one side counts as one); 2: usage or build failure.

It compares and counts; it does not look for particular instructions.
"""
import argparse
import os
import re
import shlex
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

DESCRIPTOR_LINES = ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")
LABEL = re.compile(r"\.LBB\d+_\d+")


def makefile_var(makefile, name, default=None):
    for line in open(makefile):
        m = re.match(r"\s*%s\s*\??=\s*(.*)" % re.escape(name), line)
        if m:
            return m.group(1).strip()
    if default is not None:
        return default
    raise SystemExit("isa_diff: no %s in %s" % (name, makefile))


def build_listings(tree, defines, stem, ex):
    """the tree's GPU units compiled side by side on the executor: futures of the listings, <stem>.<unit>.s"""
    csrc = os.path.join(tree, "cbc_amd", "csrc")
    mk = os.path.join(csrc, "Makefile")
    flags = makefile_var(mk, "HIPFLAGS").replace("$(ARCH)", os.environ.get("ARCH", makefile_var(mk, "ARCH")))
    hipcc = os.environ.get("HIPCC", makefile_var(mk, "HIPCC"))

    def one(unit):
        out = "%s.%s.s" % (stem, unit)
        cmd = [hipcc] + shlex.split(flags) + ["--cuda-device-only", "-S"] + defines + ["-o", out, unit + ".hip"]
        r = subprocess.run(cmd, cwd=csrc, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout)
            raise SystemExit(2)
        return out
    return [ex.submit(one, u) for u in makefile_var(mk, "GPU_UNITS", "cbc_gpu").split()]


def kernels_of(paths):
    """{kernel: (instruction lines, {descriptor key: line})} of one build: the kernels of all its listings"""
    out = {}
    for path in paths:
        for k, v in kernels_of_listing(path).items():
            if k in out:
                raise SystemExit("isa_diff: %s is defined in two units (%s)" % (k, path))
            out[k] = v
    return out


def kernels_of_listing(path):
    lines = open(path).read().splitlines()
    desc, name = {}, None
    for ln in lines:
        t = ln.strip()
        if t.startswith(".amdhsa_kernel "):
            name = t.split()[1]
            desc[name] = {}
        elif t == ".end_amdhsa_kernel":
            name = None
        elif name is not None:
            for key in DESCRIPTOR_LINES:
                if t.startswith(".amdhsa_" + key + " "):
                    desc[name][key] = t
    out, cur, body = {}, None, None
    for ln in lines:
        t = ln.split(";", 1)[0].strip()                  # none of these listings holds a ';' inside a string operand
        if cur is None:
            if t.endswith(":") and t[:-1] in desc:
                cur, body = t[:-1], []
            continue
        if t.startswith(".Lfunc_end"):
            out[cur] = (normalise(body), desc[cur])
            cur = None
        elif t and not t.startswith(".") or LABEL.match(t):
            body.append(t)
    return out


def normalise(body):
    order = {}

    def rename(m):
        return ".L%d" % order.setdefault(m.group(0), len(order))
    return [LABEL.sub(rename, " ".join(t.split())) for t in body]


def n_instructions(body):
    return sum(1 for t in body if not t.endswith(":"))


def compare(a_paths, b_paths):
    a, b = kernels_of(a_paths), kernels_of(b_paths)
    a_path, b_path = " ".join(a_paths), " ".join(b_paths)
    names = sorted(set(a) | set(b))
    differ = 0
    for k in names:
        if k not in a or k not in b:
            differ += 1
            print("DIFFERENT  %s: only in %s" % (k, a_path if k in a else b_path))
            continue
        if a[k][0] == b[k][0]:
            continue
        differ += 1
        print("DIFFERENT  %s: %d / %d instruction lines" % (k, n_instructions(a[k][0]), n_instructions(b[k][0])))
        for key in DESCRIPTOR_LINES:
            print("    %-58s | %s" % (a[k][1].get(key, "-"), b[k][1].get(key, "-")))
    print("%d of %d kernels identical" % (len(names) - differ, len(names)))
    return 1 if differ or not names else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--keep", metavar="DIR", help="write the listings there (a.<unit>.s, b.<unit>.s) instead of a temporary directory")
    ap.add_argument("-j", type=int, default=min(8, os.cpu_count() or 1), help="compiles at the same time, over both trees' units (1: one after the other)")
    args, defines = ap.parse_known_args()
    if any(not d.startswith("-D") for d in defines):
        ap.error("only -D flags are passed on to the compiler")
    if os.path.isfile(args.a) and os.path.isfile(args.b):
        return compare([args.a], [args.b])
    if not (os.path.isdir(args.a) and os.path.isdir(args.b)):
        ap.error("give two source trees or two .s files")
    with tempfile.TemporaryDirectory() as tmp:
        d = args.keep or tmp
        os.makedirs(d, exist_ok=True)
        with ThreadPoolExecutor(max(1, args.j)) as ex:
            fa = build_listings(os.path.abspath(args.a), defines, os.path.join(os.path.abspath(d), "a"), ex)
            fb = build_listings(os.path.abspath(args.b), defines, os.path.join(os.path.abspath(d), "b"), ex)
            return compare([f.result() for f in fa], [f.result() for f in fb])


if __name__ == "__main__":
    sys.exit(main())
