#!/usr/bin/env python3
"""Records what the decode entry points of libcbc_gpu.so answer to bad arguments: tests/golden/entry_refusals.json, recorded on
an MI355X (a context needs a device; no refusal launches a kernel).

WHAT THESE ARE: regression vectors of the library's argument checking -- per call the return code, the text of
cbc_gpu_last_error and the out-parameters as the call left them -- taken from the build of one commit so that a later change of
the host part of cbc_gpu.hip can be held against it: which refusal wins when two apply, the wording of every message, and which
out-parameters are zeroed when.  tests/test_entry_refusals_gpu.py imports the rows and the runner from this file.

One table, ROWS: (entry point, label, the arguments that differ from a good call).  A good call is GOOD: the two blocks of a
one-contig container of 40 reads over a 1 KiB reference.  Every row starts from an error text of its own (PRIMER), and its
out-parameters from a fill pattern, so that "left alone" and "zeroed" read differently.  The cbc_gpu_last_*_ms rows come from
last_ms_rows(): after one small run of every kind, which of them answer, and what each says to a NULL out-pointer.

  python tests/golden/make_entry_refusals.py          on an MI355X, after `make -C cbc_amd/csrc`
"""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
JSON = os.path.join(HERE, "entry_refusals.json")
FILL = 0xAA
PRIMER = "edits_per_read in 1..510 (0: the default): "

HEAD = ["in", "in_bytes", "blocks", "n_blocks", "caps", "ws"]
TABLES = ["bc", "names", "names_bytes", "noff", "n_contigs"]
TEXT = ["text", "text_cap", "text_bytes"]
WINDOW = ["name", "name_bytes", "beg", "end", "smax", "exclude"]
COV = HEAD + TABLES + ["t", "iv_first", "iv_count", "q", "n_q", "exclude", "min_depth", "sum", "covered", "n_reads", "results"]
SIGS = {
    "region": HEAD + ["beg", "end", "smax"] + TEXT + ["n_sel", "results"],
    "sam": HEAD + TABLES + ["region"] + TEXT + ["n_reads", "results"],
    "sam_cigar": HEAD + TABLES + ["region", "smax", "epr"] + TEXT + ["n_reads", "results"],
    "depth": HEAD + WINDOW + TEXT + ["n_runs", "n_kept", "results"],
    "pileup": HEAD + WINDOW + ["min_alt", "epr"] + TEXT + ["n_runs", "n_kept", "results"],
    "targets": HEAD + TABLES + ["t", "output", "exclude"] + TEXT + ["n_reads", "n_runs", "results"],
    "coverage": COV,
    "coverage_ext": COV + ["thr", "n_thr", "thr_covered", "reads"],
    "coverage_quant": COV + ["thr", "n_thr", "thr_covered", "reads", "quant", "n_quant", "quant_depth"],
    "depth_hist": HEAD + TABLES + ["t", "iv_first", "iv_count", "exclude", "max_depth", "bin_depth", "bin_bases", "bin_cap", "n_bins",
                                   "n_reads", "results"],
    "stats": HEAD + ["t", "exclude", "stats", "results"],
    "stats_aln": HEAD + ["t", "smax", "exclude", "epr", "stats", "aln", "results"],
}
# the out-parameters, as (kind, element type): made afresh for every call unless the row gives None (a NULL)
OUTS = {"text_bytes": ("scalar", ctypes.c_uint64), "n_sel": ("scalar", ctypes.c_uint64), "n_reads": ("scalar", ctypes.c_uint64),
        "n_runs": ("scalar", ctypes.c_uint64), "n_kept": ("scalar", ctypes.c_uint64), "n_bins": ("scalar", ctypes.c_uint32),
        "sum": ("array", np.uint64), "covered": ("array", np.uint32), "thr_covered": ("array", np.uint32), "reads": ("array", np.uint32),
        "quant_depth": ("array", np.uint32), "bin_depth": ("array", np.uint32), "bin_bases": ("array", np.uint32),
        "stats": ("struct", "GpuStats"), "aln": ("struct", "GpuStatsAln")}
U32 = np.uint32


class Fixture:
    """The container, the arrays of a good call (GOOD) and the two contexts: `ready` has the reference, `fresh` has not."""

    def __init__(self):
        import regionmodel as rm
        import synth
        from cbc_amd import gpu, host
        self.gpu, self.host = gpu, host
        fa, _, rbc, _ = synth.dataset(7, [1024], [40], 50)
        self.pb = rm.pack(fa, rbc, 20)
        self.plan = plan = host.UnpackPlan(rm.container(self.pb), fa)
        assert (plan.n_blocks, plan.n_contigs, int(plan.contig_len[0])) == (2, 1, 1024), (plan.n_blocks, plan.n_contigs)
        smax = plan.max_read_len + plan.read_length - 1
        self.good = dict(
            in_bytes=plan.payloads.size, blocks=np.ascontiguousarray(plan.blocks), n_blocks=2,
            caps=host.LdsCaps(plan.cap_pos, plan.cap_var), ws=np.ascontiguousarray(plan.window_start, dtype=np.uint64),
            bc=np.zeros(2, dtype=U32), names=np.frombuffer(b"chr1\0", dtype=np.uint8), names_bytes=5, noff=np.zeros(1, dtype=U32),
            n_contigs=1, region=None, beg=1, end=1000, smax=smax, epr=0, name=b"chr1", name_bytes=4, exclude=0, min_alt=1,
            text=np.zeros(4096, dtype=np.uint8), text_cap=4096, results=np.zeros(1 << 16, dtype=host.RESULT_DTYPE),
            t=True, iv=np.array([[100, 200], [400, 500]], dtype=U32), block_iv=np.array([[0, 2], [0, 2]], dtype=U32), n_iv=2, t_smax=smax,
            output=0, iv_first=0, iv_count=2, q=np.array([[0, 10]], dtype=U32), n_q=1, min_depth=1, thr=np.array([1, 5], dtype=U32),
            n_thr=2, quant=np.array([50], dtype=U32), n_quant=1, max_depth=0, bin_cap=8)
        self.good["in"] = np.ascontiguousarray(plan.payloads)
        self.ready, self.fresh = gpu.Encoder(0), gpu.Encoder(0)
        self.ready.upload_reference(plan.ref)

    def close(self):
        self.ready.close(); self.fresh.close(); self.plan.close(); self.pb.close()

    def blocks(self, n=2, **fields):
        """The good descriptors (n > 2: n copies of the first) with fields replaced: name=value for all, name=(b, value) for one."""
        bl = self.good["blocks"].copy() if n == 2 else np.repeat(self.good["blocks"][:1], n)
        for k, v in fields.items():
            if isinstance(v, tuple):
                bl[k][v[0]] = v[1]
            else:
                bl[k] = v
        return bl


def rows(fx):
    """[(entry point, label, {argument: value}, context)]: see the module text."""
    g = fx.good
    out = []
    def add(fn, label, ctx="ready", **over):
        out.append((fn, label, over, ctx))
    arr = lambda v, dt=U32: np.array(v, dtype=dt)
    far = fx.blocks(in_off=(1, g["in_bytes"] + 1))
    mixed = fx.blocks(seq_stride=(1, int(g["blocks"]["seq_stride"][0]) + 4))
    other_contig = fx.blocks(ref_off=(1, int(g["blocks"]["ref_off"][1]) + 7))
    unordered, past = arr([[200, 100], [400, 500]]), arr([[100, 200], [400, 0x80000000]])
    two = dict(bc=arr([0, 1]), names=np.frombuffer(b"chr1\0chrB\0", dtype=np.uint8), names_bytes=10, noff=arr([0, 5]), n_contigs=2)
    region0 = dict(region=(0, 5, g["smax"]))
    nulls = {
        "region": ["blocks", "caps", "ws", "text_bytes", "n_sel", "text", "in"],
        "sam": ["blocks", "caps", "ws", "bc", "names", "noff", "text_bytes", "n_reads", "text", "in"],
        "depth": ["blocks", "caps", "ws", "name", "text_bytes", "n_runs", "n_kept", "text", "in"],
        "targets": ["blocks", "caps", "ws", "bc", "names", "noff", "t", "text_bytes", "n_reads", "n_runs", "text", "in", "iv", "block_iv"],
        "coverage": ["t", "n_reads", "q", "sum", "covered", "blocks", "caps", "ws", "bc", "names", "noff", "in", "iv", "block_iv"],
        "depth_hist": ["t", "n_reads", "n_bins", "bin_depth", "bin_bases", "blocks", "caps", "ws", "in", "iv"],
        "stats": ["stats", "blocks", "caps", "ws", "in", "iv", "block_iv"],
    }
    nulls["sam_cigar"], nulls["pileup"] = nulls["sam"], nulls["depth"]
    nulls["coverage_ext"] = nulls["coverage"] + ["thr", "thr_covered"]
    nulls["coverage_quant"] = nulls["coverage_ext"] + ["quant", "quant_depth"]
    nulls["stats_aln"] = nulls["stats"] + ["aln"]
    for fn in SIGS:
        add(fn, "ctx NULL", ctx=None)
        for name in nulls[fn]:
            add(fn, name + " NULL", **{name: None})
        add(fn, "reference not uploaded", ctx="fresh")
        add(fn, "reference not uploaded, in NULL", ctx="fresh", **{"in": None})
        add(fn, "reference not uploaded, no blocks", ctx="fresh", n_blocks=0)
        add(fn, "no blocks", n_blocks=0)
        add(fn, "no blocks, in NULL", n_blocks=0, **{"in": None})
        add(fn, "a block out of range of in", blocks=far)
        add(fn, "mixed strides", blocks=mixed)
        add(fn, "stride 6", blocks=fx.blocks(seq_stride=6))
    for fn in ("region", "depth", "pileup"):
        add(fn, "beg 0", beg=0)
        add(fn, "beg > end", beg=9, end=5)
        add(fn, "smax 0", smax=0)
        add(fn, "smax 0, mixed strides", smax=0, blocks=mixed)
    for fn in ("depth", "pileup"):
        add(fn, "end 2^31", end=0x80000000)
        add(fn, "name empty", name_bytes=0)
        add(fn, "name 256 bytes", name=b"a" * 256, name_bytes=256)
        add(fn, "name with a tab", name=b"ch\tr")
        add(fn, "name with a newline", name=b"ch\nr")
        add(fn, "name with a NUL", name=b"ch\0r")
        add(fn, "beg 0, name empty", beg=0, name_bytes=0)
        add(fn, "name empty, mixed strides", name_bytes=0, blocks=mixed)
        add(fn, "name empty, a block out of range", name_bytes=0, blocks=far)
        add(fn, "2^30 reads", blocks=fx.blocks(65536, n_reads=16384), n_blocks=65536, ws=np.repeat(g["ws"][:1], 65536))
    add("pileup", "min_alt 0", min_alt=0)
    add("pileup", "edits_per_read 511", epr=511)
    add("pileup", "edits_per_read 510, beg 0", epr=510, beg=0)
    add("pileup", "blocks of two contigs", blocks=other_contig)
    add("pileup", "a block in front of its window", ws=arr([int(g["blocks"]["ref_off"][0]) + 1, int(g["ws"][1])], np.uint64))
    add("pileup", "smax 0, min_alt 0", smax=0, min_alt=0)
    add("pileup", "min_alt 0, edits_per_read 511", min_alt=0, epr=511)
    add("pileup", "edits_per_read 511, name empty", epr=511, name_bytes=0)
    add("pileup", "name with a tab, blocks of two contigs", name=b"ch\tr", blocks=other_contig)
    add("pileup", "blocks of two contigs, mixed strides", blocks=fx.blocks(ref_off=(1, int(g["blocks"]["ref_off"][1]) + 7),
                                                                          seq_stride=(1, int(g["blocks"]["seq_stride"][0]) + 4)))
    for fn in ("sam", "sam_cigar"):
        add(fn, "region beg 0", **region0)
        add(fn, "region beg > end", region=(9, 5, g["smax"]))
        add(fn, "region smax 0", region=(1, 5, 0))
        add(fn, "region beg 0, mixed strides", blocks=mixed, **region0)
        add(fn, "region beg 0, in NULL", **{"in": None}, **region0)
    add("sam_cigar", "smax 0 without a region", smax=0)
    add("sam_cigar", "edits_per_read 511", epr=511)
    add("sam_cigar", "region smax 0, edits_per_read 511", region=(1, 5, 0), epr=511)
    add("sam_cigar", "smax 0 without a region, edits_per_read 511", smax=0, epr=511)
    add("sam_cigar", "edits_per_read 511, mixed strides", epr=511, blocks=mixed)
    add("sam_cigar", "edits_per_read 511, a contig outside the table", epr=511, bc=arr([0, 5]))
    add("sam_cigar", "2^30 reads", blocks=fx.blocks(65536, n_reads=16384), n_blocks=65536, ws=np.repeat(g["ws"][:1], 65536),
        bc=np.zeros(65536, dtype=U32))
    for fn in ("sam", "sam_cigar", "targets", "coverage", "depth_hist"):
        add(fn, "a contig outside the table", bc=arr([0, 5]))
        add(fn, "a name offset outside the names", noff=arr([9]))
        add(fn, "contig name with a tab", names=np.frombuffer(b"c\tr1\0", dtype=np.uint8))
        add(fn, "contig name unterminated", names=np.frombuffer(b"chr1x", dtype=np.uint8))
        add(fn, "a block starts past POS 2^31 - 1", ws=arr([int(g["ws"][0]), 0x80000000], np.uint64))
        add(fn, "mixed strides, a contig outside the table", blocks=mixed, bc=arr([5, 0]))
    for fn in ("targets", "coverage", "coverage_ext", "coverage_quant", "depth_hist", "stats", "stats_aln"):
        add(fn, "targets smax 0", t_smax=0)
        add(fn, "no interval", n_iv=0, iv_first=0, iv_count=0)
        add(fn, "2^24 + 1 intervals", n_iv=(1 << 24) + 1)
        add(fn, "an interval unordered", iv=unordered)
        add(fn, "an interval ends past 2^31 - 1", iv=past)
        add(fn, "an interval begins at 0", iv=arr([[0, 200], [400, 500]]))
        add(fn, "block_iv count out of range", block_iv=arr([[0, 2], [0, 3]]))
        add(fn, "block_iv first out of range", block_iv=arr([[0, 2], [3, 0]]))
        add(fn, "an interval unordered, block_iv out of range", iv=unordered, block_iv=arr([[0, 3], [0, 2]]))
        add(fn, "block_iv out of range, mixed strides", block_iv=arr([[0, 3], [0, 2]]), blocks=mixed)
        add(fn, "targets smax 0, an interval unordered", t_smax=0, iv=unordered)
    add("targets", "output 3", output=3)
    add("targets", "depth: blocks of two contigs", output=2, **two)
    add("targets", "depth: blocks of two contigs, block_iv out of range", output=2, block_iv=arr([[0, 2], [0, 3]]), **two)
    add("targets", "depth: intervals touch", output=2, iv=arr([[100, 200], [201, 300]]))
    add("targets", "depth: 2^30 reads", output=2, blocks=fx.blocks(65536, n_reads=16384), n_blocks=65536,
        ws=np.repeat(g["ws"][:1], 65536), bc=np.zeros(65536, dtype=U32), block_iv=np.tile(arr([0, 2]), (65536, 1)))
    for fn in ("coverage", "coverage_ext", "coverage_quant", "depth_hist"):
        add(fn, "blocks of two contigs", **two)
        add(fn, "intervals touch", iv=arr([[100, 200], [201, 300]]))
        add(fn, "iv_first outside the table", iv_first=3)
        add(fn, "iv_count 0", iv_count=0)
        add(fn, "iv_count outside the table", iv_count=3)
        add(fn, "a block's intervals outside the contig's", iv_first=1, iv_count=1)
        add(fn, "iv_count 0, blocks NULL", iv_count=0, blocks=None)
    for fn in ("coverage", "coverage_ext", "coverage_quant"):
        add(fn, "min_depth 0", min_depth=0)
        add(fn, "no query", n_q=0)
        add(fn, "a query outside the compressed coordinate", q=arr([[1000000, 5]]))
        add(fn, "min_depth 0, iv_count 0, in NULL", min_depth=0, iv_count=0, **{"in": None})
    for fn in ("coverage_ext", "coverage_quant"):
        add(fn, "nine thresholds", thr=arr(range(1, 10)), n_thr=9)
        add(fn, "thresholds not ascending", thr=arr([5, 1]))
        add(fn, "a threshold of 0", thr=arr([0, 1]))
        add(fn, "min_depth 0, thresholds not ascending", min_depth=0, thr=arr([5, 1]))
        add(fn, "thresholds not ascending, no query", thr=arr([5, 1]), n_q=0)
    add("coverage_quant", "nine quantiles", quant=arr(range(1, 10)), n_quant=9)
    add("coverage_quant", "quantiles not ascending", quant=arr([50, 10]), n_quant=2)
    add("coverage_quant", "a quantile of 101", quant=arr([101]))
    add("coverage_quant", "thresholds and quantiles not ascending", thr=arr([5, 1]), quant=arr([50, 10]), n_quant=2)
    for fn in ("stats", "stats_aln"):
        add(fn, "whole file: mixed strides", t=False, blocks=mixed)
        add(fn, "whole file: no blocks", t=False, n_blocks=0)
        add(fn, "a block starts past POS 2^31 - 1", ws=arr([int(g["ws"][0]), 0x80000000], np.uint64))
        add(fn, "block_iv out of range, a block starts past POS 2^31 - 1", block_iv=arr([[0, 2], [0, 3]]),
            ws=arr([int(g["ws"][0]), 0x80000000], np.uint64))
        # 130 blocks of 2^32 - 256 reads: 130 x 2^22 record groups pass 2^29, and no block may hold that many reads
        add(fn, "2^29 units", t=False, blocks=fx.blocks(130, n_reads=0xffffff00), n_blocks=130)
        add(fn, "2^29 units, stride 6", t=False, blocks=fx.blocks(130, n_reads=0xffffff00, seq_stride=6), n_blocks=130)
    add("stats_aln", "whole file: smax 0", t=False, smax=0)
    add("stats_aln", "edits_per_read 511", epr=511)
    add("stats_aln", "targets smax 0, edits_per_read 511", t_smax=0, epr=511)
    add("stats_aln", "whole file: smax 0, edits_per_read 511", t=False, smax=0, epr=511)
    add("stats_aln", "edits_per_read 511, an interval unordered", epr=511, iv=unordered)
    add("stats_aln", "edits_per_read 511, mixed strides", epr=511, blocks=mixed)
    add("stats_aln", "2^29 units, edits_per_read 511", t=False, blocks=fx.blocks(130, n_reads=0xffffff00), n_blocks=130, epr=511)
    ids = [fn + ": " + label for fn, label, _, _ in out]
    assert len(set(ids)) == len(ids)
    return out


def _prime(fx, enc):
    """Leaves PRIMER as the context's error text: a refusal of cbc_gpu_decode_blocks_edits that needs no reference."""
    g, one = fx.good, np.zeros(64, dtype=np.uint8)
    rc = fx.gpu.lib().cbc_gpu_decode_blocks_edits(enc._ctx, g["in"].ctypes.data, g["in_bytes"], g["blocks"].ctypes.data, 2, ctypes.byref(g["caps"]),
                                                  1, 511, one.ctypes.data, 0, one.ctypes.data, 0, one.ctypes.data, one.ctypes.data,
                                                  g["results"].ctypes.data)
    assert rc == -1 and fx.gpu.lib().cbc_gpu_last_error(enc._ctx).decode() == PRIMER


def _summary(raw):
    if raw.count(0) == len(raw):
        return "zeroed"
    return "as filled" if raw.count(FILL) == len(raw) else "sha256 " + hashlib.sha256(raw).hexdigest()


def run_row(fx, row):
    """One call.  Returns what is compared: [return code, error text (None without a context), {out-parameter: what it holds}]."""
    fn, _, over, which = row
    v = dict(fx.good, **over)
    enc = {"ready": fx.ready, "fresh": fx.fresh, None: None}[which]
    n_q = v["n_q"] if v["n_q"] <= 16 else 0
    sizes = {"sum": n_q, "covered": n_q, "reads": n_q, "thr_covered": n_q * min(v["n_thr"], 8), "quant_depth": n_q * min(v["n_quant"], 8),
             "bin_depth": v["bin_cap"], "bin_bases": v["bin_cap"]}
    held, args = {}, []
    for name in SIGS[fn]:
        if name in OUTS and name not in over:
            kind, ty = OUTS[name]
            if kind == "scalar":
                v[name] = ty(int.from_bytes(bytes([FILL]) * ctypes.sizeof(ty), "little"))
            elif kind == "array":
                v[name] = np.frombuffer(bytes([FILL]) * (max(sizes[name], 1) * np.dtype(ty).itemsize), dtype=ty).copy()
            else:
                v[name] = getattr(fx.host, ty)()
                ctypes.memset(ctypes.byref(v[name]), FILL, ctypes.sizeof(v[name]))
            held[name] = v[name]
        x = v[name]
        if name == "t" and x:
            held["t"] = x = fx.gpu.GpuTargets(None if v["iv"] is None else v["iv"].ctypes.data,
                                              None if v["block_iv"] is None else v["block_iv"].ctypes.data, v["n_iv"], v["t_smax"])
        elif name == "t":
            x = None
        elif name == "region" and x is not None:
            held["region"] = x = fx.gpu.SamRegion(x[0], x[1], x[2], 0)
        if isinstance(x, np.ndarray):
            x = x.ctypes.data
        elif isinstance(x, (ctypes.Structure, ctypes.c_uint64, ctypes.c_uint32)):
            x = ctypes.byref(x)
        args.append(x)
    if enc is not None:
        _prime(fx, enc)
    L = fx.gpu.lib()
    rc = getattr(L, "cbc_gpu_decode_" + fn)(enc._ctx if enc is not None else None, *args)
    outs = {}
    for name in SIGS[fn]:
        if name in OUTS:
            x = held.get(name)
            outs[name] = (None if x is None else int(x.value) if OUTS[name][0] == "scalar" else _summary(bytes(x)) if OUTS[name][0] == "struct"
                          else _summary(x.tobytes()))
    return [rc, L.cbc_gpu_last_error(enc._ctx).decode() if enc is not None else None, outs]


# every cbc_gpu_last_*_ms with the number of its pointer arguments, and the small runs that set the kind of the last call
LAST_MS = {"region": 3, "sam": 3, "sam_cigar": 4, "depth": 4, "pileup": 4, "targets": 4, "coverage": 7, "coverage_ext": 2,
           "coverage_quant": 3, "hist": 5, "stats": 2, "stats_aln": 3}
FLOATS = {"coverage_ext": (7, 5), "coverage_quant": (7, 5, 1)}


def _runs(fx):
    enc, plan = fx.ready, fx.plan
    ts = plan.targets([b"chr1:100-300", b"chr1:600-700"])
    return [("region", lambda: enc.decode_region(plan, "chr1:100-400")), ("sam", lambda: enc.decode_sam(plan)),
            ("sam_cigar", lambda: enc.decode_sam(plan, cigar=True)), ("depth", lambda: enc.decode_depth(plan)),
            ("pileup", lambda: enc.decode_pileup(plan)), ("targets reads", lambda: enc.decode_targets(plan, ts, "reads")),
            ("targets sam", lambda: enc.decode_targets(plan, ts, "sam")), ("targets depth", lambda: enc.decode_targets(plan, ts, "depth")),
            ("coverage", lambda: enc.decode_coverage(plan, plan.queries())),
            ("coverage_ext", lambda: enc.decode_coverage(plan, plan.queries(), thresholds=(1, 2))),
            ("coverage_quant", lambda: enc.decode_coverage_quant(plan, plan.queries(), (50,))),
            ("hist", lambda: enc.decode_depth_hist(plan)), ("stats", lambda: enc.decode_stats(plan)),
            ("stats of targets", lambda: enc.decode_stats(plan, ts)), ("stats_aln", lambda: enc.decode_stats_aln(plan)),
            ("stats_aln of targets", lambda: enc.decode_stats_aln(plan, ts)), ("plain decode behind them", lambda: enc.decode_blocks(plan))]


def _ask(fx, name, null=None):
    """(return code, the floats as they stand after the call: "nan" where the call wrote nothing) of one cbc_gpu_last_<name>_ms,
    with its pointer argument `null` NULL."""
    bufs = [(ctypes.c_float * n)(*([float("nan")] * n)) for n in FLOATS.get(name, (1,) * LAST_MS[name])]
    rc = getattr(fx.gpu.lib(), "cbc_gpu_last_%s_ms" % name)(fx.ready._ctx, *[None if i == null else ctypes.cast(b, ctypes.POINTER(ctypes.c_float))
                                                                              for i, b in enumerate(bufs)])
    return rc, [x for b in bufs for x in b]


def last_ms_rows(fx):
    """{label: result}: before any run and after each of _runs, the return code of every cbc_gpu_last_*_ms ("0 scan 0" where
    cbc_gpu_last_targets_ms gives scan_ms = 0); and after the run of its own kind, per pointer argument the return code with that
    one NULL and whether any float was written."""
    out = {}
    def all_of(label):
        res = {}
        for name in LAST_MS:
            rc, ms = _ask(fx, name)
            assert rc != 0 or all(x == x and x >= 0 for x in ms), (label, name, ms)
            res[name] = "0 scan 0" if rc == 0 and name == "targets" and ms[2] == 0.0 else rc
        out[label] = res
    all_of("reference uploaded")
    for label, run in _runs(fx):
        run()
        all_of("after " + label)
        for name in LAST_MS:
            if label.split()[0] == name and _ask(fx, name)[0] == 0:
                out["after %s: %s with a NULL" % (label, name)] = [[rc, any(x == x for x in ms)] for rc, ms in
                                                                   (_ask(fx, name, k) for k in range(LAST_MS[name]))]
    return out


def collect(fx):
    """The fixture file's content: the refusal rows first (none launches a kernel), then the cbc_gpu_last_*_ms rows."""
    got = {fn + ": " + label: run_row(fx, (fn, label, over, ctx)) for fn, label, over, ctx in rows(fx)}
    return {"rows": got, "last_ms": last_ms_rows(fx)}


def main():
    fx = Fixture()
    try:
        got = collect(fx)
    finally:
        fx.close()
    ok = [k for k, r in got["rows"].items() if r[0] == 0]
    print("%d rows, %d of them return 0 (the calls without blocks or queries):" % (len(got["rows"]), len(ok)))
    for k in ok:
        print("  " + k)
    with open(JSON, "w") as f:
        f.write('{"rows": {\n' + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(r, sort_keys=True)) for k, r in got["rows"].items())
                + '\n},\n"last_ms": {\n' + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(r, sort_keys=True)) for k, r in got["last_ms"].items())
                + "\n}}\n")


if __name__ == "__main__":
    main()
