"""ctypes view of libcbc_host.so (the plain-C host side: packer, container, synthetic workload).

Mirrors, for the hot path only, the reference's record loader / FASTA loader seam
(src/sam_file_allocation.c:437-529, src/read_decompression.c:17-53): text in, packed blocks out.
Python is plumbing here; the work is done by cbc_amd/csrc/cbc_pack.c.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
HOST_LIB = os.path.join(_CSRC, "libcbc_host.so")

CBC_CAP_FLAG = 64
CBC_CAP_NAME = 128
CBC_REF_PAD = 512
CBC_MAX_READ_LEN = 252


class ReadRec(ctypes.Structure):
    _fields_ = [("pos", ctypes.c_uint32), ("flag", ctypes.c_uint16), ("rlen", ctypes.c_uint16),
                ("seq_off", ctypes.c_uint32), ("tok_off", ctypes.c_uint32)]


class BlockDesc(ctypes.Structure):
    _fields_ = [("rec_base", ctypes.c_uint64), ("seq_base", ctypes.c_uint64), ("tok_base", ctypes.c_uint64),
                ("ref_off", ctypes.c_uint64), ("out_off", ctypes.c_uint64), ("out_cap", ctypes.c_uint32),
                ("n_reads", ctypes.c_uint32), ("name_off", ctypes.c_uint32), ("read_length", ctypes.c_uint32),
                ("n_tok", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class BlockResult(ctypes.Structure):
    _fields_ = [("nbytes", ctypes.c_uint32), ("status", ctypes.c_uint32), ("n_symbols", ctypes.c_uint32),
                ("fail_read", ctypes.c_uint32)]


class BlockInfo(ctypes.Structure):
    _fields_ = [("contig", ctypes.c_uint32), ("n_reads", ctypes.c_uint32), ("window_start", ctypes.c_uint64),
                ("n_bases", ctypes.c_uint64)]


class ContigInfo(ctypes.Structure):
    _fields_ = [("ref_off", ctypes.c_uint64), ("length", ctypes.c_uint64), ("name_off", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class LdsCaps(ctypes.Structure):
    _fields_ = [("cap_pos", ctypes.c_uint32), ("cap_var", ctypes.c_uint32)]


class ConsensusOpts(ctypes.Structure):
    """cbc_consensus_opts: flags = 1 show_del | 2 fill_ref | 4 iupac."""
    _fields_ = [("min_depth", ctypes.c_uint32), ("call_ppm", ctypes.c_uint32), ("line_width", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


class ConsensusCounts(ctypes.Structure):
    """cbc_consensus_counts."""
    _fields_ = [(k, ctypes.c_uint64) for k in ("emitted", "ref", "alt", "del", "ambiguous", "low_depth", "no_call", "ins_skipped")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class Packed(ctypes.Structure):
    _fields_ = [
        ("recs", ctypes.POINTER(ReadRec)), ("n_recs", ctypes.c_uint64),
        ("seq", ctypes.POINTER(ctypes.c_uint8)), ("seq_bytes", ctypes.c_uint64),
        ("tok", ctypes.POINTER(ctypes.c_uint32)), ("n_tok", ctypes.c_uint64),
        ("names", ctypes.POINTER(ctypes.c_uint8)), ("names_bytes", ctypes.c_uint32),
        ("blocks", ctypes.POINTER(BlockDesc)), ("n_blocks", ctypes.c_uint32),
        ("info", ctypes.POINTER(BlockInfo)),
        ("contigs", ctypes.POINTER(ContigInfo)), ("n_contigs", ctypes.c_uint32),
        ("ref", ctypes.POINTER(ctypes.c_uint8)), ("ref_bytes", ctypes.c_uint64),
        ("caps", LdsCaps),
        ("read_length", ctypes.c_uint32),
        ("n_bases", ctypes.c_uint64),
        ("n_skipped_unmapped", ctypes.c_uint64),
        ("max_read_len", ctypes.c_uint32), ("whole_file", ctypes.c_uint32),
        ("cap_recs", ctypes.c_uint64), ("cap_seq", ctypes.c_uint64), ("cap_tok", ctypes.c_uint64),
        ("cap_ref", ctypes.c_uint64), ("cap_names", ctypes.c_uint32), ("cap_blocks", ctypes.c_uint32),
        ("cap_contigs", ctypes.c_uint32),
    ]


class DecBlockDesc(ctypes.Structure):
    _fields_ = [("in_off", ctypes.c_uint64), ("ref_off", ctypes.c_uint64), ("rec_base", ctypes.c_uint64),
                ("seq_base", ctypes.c_uint64), ("in_bytes", ctypes.c_uint32), ("n_reads", ctypes.c_uint32),
                ("read_length", ctypes.c_uint32), ("seq_stride", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 4)]


class UnpackPlanC(ctypes.Structure):
    _fields_ = [("blocks", ctypes.POINTER(DecBlockDesc)), ("n_blocks", ctypes.c_uint32),
                ("payloads", ctypes.POINTER(ctypes.c_uint8)), ("payload_bytes", ctypes.c_uint64),
                ("ref", ctypes.POINTER(ctypes.c_uint8)), ("ref_bytes", ctypes.c_uint64),
                ("window_start", ctypes.POINTER(ctypes.c_uint64)),
                ("caps", LdsCaps), ("read_length", ctypes.c_uint32), ("seq_stride", ctypes.c_uint32),
                ("n_recs", ctypes.c_uint64), ("long_reads", ctypes.c_uint32), ("max_read_len", ctypes.c_uint32),
                ("seq_total", ctypes.c_uint64),
                ("block_contig", ctypes.POINTER(ctypes.c_uint32)), ("n_contigs", ctypes.c_uint32),
                ("names_bytes", ctypes.c_uint32), ("names", ctypes.c_void_p),
                ("contig_name_off", ctypes.POINTER(ctypes.c_uint32)), ("contig_len", ctypes.POINTER(ctypes.c_uint64))]


class TargetsC(ctypes.Structure):
    _fields_ = [("iv", ctypes.POINTER(ctypes.c_uint32)), ("n_iv", ctypes.c_uint32), ("n_contigs", ctypes.c_uint32),
                ("contig_first", ctypes.POINTER(ctypes.c_uint32)), ("contig_count", ctypes.POINTER(ctypes.c_uint32)),
                ("blocks", ctypes.POINTER(ctypes.c_uint32)), ("n_blocks", ctypes.c_uint32), ("smax", ctypes.c_uint32),
                ("block_iv", ctypes.POINTER(ctypes.c_uint32)),
                ("contig_blk_first", ctypes.POINTER(ctypes.c_uint32)), ("contig_blk_count", ctypes.POINTER(ctypes.c_uint32)),
                ("bed_unselected", ctypes.c_uint64), ("n_input", ctypes.c_uint64)]


class QueriesC(ctypes.Structure):
    _fields_ = [("q", ctypes.c_void_p), ("n_q", ctypes.c_uint64), ("targets", ctypes.POINTER(TargetsC))]


QUERY_DTYPE = np.dtype([("contig", "<u4"), ("beg", "<u4"), ("end", "<u4"), ("slot", "<u4"), ("name_off", "<u4"), ("name_len", "<u4"),
                        ("start0", "<u8"), ("end0", "<u8")])
QUERY_UNKNOWN = 0xffffffff


class RegionSelC(ctypes.Structure):
    _fields_ = [("contig", ctypes.c_uint32), ("b0", ctypes.c_uint32), ("b1", ctypes.c_uint32), ("smax", ctypes.c_uint32),
                ("beg", ctypes.c_uint64), ("end", ctypes.c_uint64), ("contig_len", ctypes.c_uint64)]


class PackOpts(ctypes.Structure):
    _fields_ = [("block_reads", ctypes.c_uint32), ("max_cap_pos", ctypes.c_uint32),
                ("max_cap_var", ctypes.c_uint32), ("var_length", ctypes.c_uint32),
                ("n_threads", ctypes.c_uint32), ("whole_file", ctypes.c_uint32), ("long_reads", ctypes.c_uint32)]


class SynthOpts(ctypes.Structure):
    _fields_ = [("seed", ctypes.c_uint64), ("contig_len", ctypes.c_uint64), ("n_reads", ctypes.c_uint64),
                ("read_len", ctypes.c_uint32), ("sub_rate", ctypes.c_double), ("indel_frac", ctypes.c_double),
                ("name", ctypes.c_char_p)]


class TwoBitRun(ctypes.Structure):
    _fields_ = [("start", ctypes.c_uint64), ("length", ctypes.c_uint32), ("byte", ctypes.c_uint32)]


class TwoBitC(ctypes.Structure):
    _fields_ = [("codes", ctypes.POINTER(ctypes.c_uint32)), ("n_bases", ctypes.c_uint64),
                ("runs", ctypes.POINTER(TwoBitRun)), ("n_runs", ctypes.c_uint64)]


RUN_DTYPE = np.dtype([("start", "<u8"), ("length", "<u4"), ("byte", "<u4")])


class CbcInputError(ValueError):
    """The input violates a limit of the reference format (message from the packer)."""


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(HOST_LIB):
            raise RuntimeError("libcbc_host.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "or `make -C cbc_amd/csrc`")
        L = ctypes.CDLL(HOST_LIB)
        L.cbc_pack_default_opts.argtypes = [ctypes.POINTER(PackOpts)]
        L.cbc_pack_sam.restype = ctypes.c_int
        L.cbc_pack_sam.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                                   ctypes.POINTER(PackOpts), ctypes.POINTER(ctypes.POINTER(Packed)),
                                   ctypes.c_char_p, ctypes.c_size_t]
        L.cbc_packed_free.argtypes = [ctypes.POINTER(Packed)]
        L.cbc_synth_packed.restype = ctypes.c_int
        L.cbc_synth_packed.argtypes = [ctypes.POINTER(SynthOpts), ctypes.POINTER(PackOpts),
                                       ctypes.POINTER(ctypes.POINTER(Packed)),
                                       ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t),
                                       ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t),
                                       ctypes.c_char_p, ctypes.c_size_t]
        L.cbc_synth_long.restype = ctypes.c_int
        L.cbc_synth_long.argtypes = L.cbc_synth_packed.argtypes
        L.cbc_free.argtypes = [ctypes.c_void_p]
        L.cbc_container_size.restype = ctypes.c_int64
        L.cbc_container_size.argtypes = [ctypes.POINTER(Packed), ctypes.POINTER(ctypes.c_uint64)]
        L.cbc_container_write.restype = ctypes.c_int64
        L.cbc_container_write.argtypes = [ctypes.POINTER(Packed), ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64),
                                          ctypes.c_void_p, ctypes.c_uint64]
        L.cbc_pack_from_device_tokens.restype = ctypes.c_int
        L.cbc_pack_from_device_tokens.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(PackOpts),
                                                  ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64,
                                                  ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                                  ctypes.POINTER(ctypes.POINTER(Packed)), ctypes.c_char_p, ctypes.c_size_t]
        L.cbc_sam_body_offset.restype = ctypes.c_uint64
        L.cbc_sam_body_offset.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
        L.cbc_2bit_pack.restype = ctypes.c_int
        L.cbc_2bit_pack.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(ctypes.POINTER(TwoBitC))]
        L.cbc_2bit_unpack.restype = ctypes.c_int
        L.cbc_2bit_unpack.argtypes = [ctypes.POINTER(TwoBitC), ctypes.c_void_p]
        L.cbc_2bit_free.argtypes = [ctypes.POINTER(TwoBitC)]
        L.cbc_assign_contigs.restype = ctypes.c_int
        L.cbc_assign_contigs.argtypes = [ctypes.POINTER(Packed), ctypes.c_uint32, ctypes.c_void_p]
        L.cbc_checksum64.restype = ctypes.c_uint64
        L.cbc_checksum64.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
        L.cbc_unpack_plan_create.restype = ctypes.c_int
        L.cbc_unpack_plan_create.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_size_t,
                                             ctypes.POINTER(ctypes.POINTER(UnpackPlanC)), ctypes.c_char_p, ctypes.c_size_t]
        L.cbc_unpack_plan_free.argtypes = [ctypes.POINTER(UnpackPlanC)]
        L.cbc_unpack_region.restype = ctypes.c_int
        L.cbc_unpack_region.argtypes = [ctypes.POINTER(UnpackPlanC), ctypes.c_char_p, ctypes.POINTER(RegionSelC),
                                        ctypes.c_char_p, ctypes.c_size_t]
        L.cbc_unpack_write_text.restype = ctypes.c_int64
        L.cbc_unpack_write_text.argtypes = [ctypes.POINTER(UnpackPlanC), ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_uint64]
        L.cbc_unpack_sam_header.restype = ctypes.c_int64
        L.cbc_unpack_sam_header.argtypes = [ctypes.POINTER(UnpackPlanC), ctypes.c_void_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_size_t]
        L.cbc_unpack_sam_text_cap.restype = ctypes.c_uint64
        L.cbc_unpack_sam_text_cap.argtypes = [ctypes.POINTER(UnpackPlanC), ctypes.c_uint32, ctypes.c_uint32]
        L.cbc_unpack_contig_blocks.restype = ctypes.c_int
        L.cbc_unpack_contig_blocks.argtypes = [ctypes.POINTER(UnpackPlanC), ctypes.c_uint32, ctypes.POINTER(RegionSelC), ctypes.c_char_p, ctypes.c_size_t]
        L.cbc_unpack_depth_text_cap.restype = ctypes.c_uint64
        L.cbc_unpack_depth_text_cap.argtypes = [ctypes.POINTER(UnpackPlanC), ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
        L.cbc_unpack_sam_cigar_text_cap.restype = ctypes.c_uint64
        L.cbc_unpack_sam_cigar_text_cap.argtypes = [ctypes.POINTER(UnpackPlanC), ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
        L.cbc_unpack_pileup_text_cap.restype = ctypes.c_uint64
        L.cbc_unpack_pileup_text_cap.argtypes = [ctypes.POINTER(UnpackPlanC), ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                                 ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32]
        L.cbc_unpack_pileup_ext_text_cap.restype = ctypes.c_uint64
        L.cbc_unpack_pileup_ext_text_cap.argtypes = [ctypes.POINTER(UnpackPlanC), ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                                     ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32]
        L.cbc_unpack_consensus_text_cap.restype = ctypes.c_uint64
        L.cbc_unpack_consensus_text_cap.argtypes = [ctypes.POINTER(UnpackPlanC), ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64,
                                                    ctypes.c_uint32, ctypes.c_uint32]
        L.cbc_unpack_consensus_empty.restype = ctypes.c_int64
        L.cbc_unpack_consensus_empty.argtypes = [ctypes.POINTER(UnpackPlanC), ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64,
                                                 ctypes.POINTER(ConsensusOpts), ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64,
                                                 ctypes.POINTER(ConsensusCounts)]
        L.cbc_unpack_depth_skipdel_text_cap.restype = ctypes.c_uint64
        L.cbc_unpack_depth_skipdel_text_cap.argtypes = [ctypes.POINTER(UnpackPlanC), ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                                        ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32]
        L.cbc_unpack_targets.restype = ctypes.c_int
        L.cbc_unpack_targets.argtypes = [ctypes.POINTER(UnpackPlanC), ctypes.POINTER(ctypes.c_char_p), ctypes.c_uint32, ctypes.c_void_p,
                                         ctypes.c_size_t, ctypes.POINTER(ctypes.POINTER(TargetsC)), ctypes.c_char_p, ctypes.c_size_t]
        L.cbc_targets_free.restype = None
        L.cbc_targets_free.argtypes = [ctypes.POINTER(TargetsC)]
        L.cbc_unpack_targets_text_cap.restype = ctypes.c_uint64
        L.cbc_unpack_targets_text_cap.argtypes = [ctypes.POINTER(UnpackPlanC), ctypes.POINTER(TargetsC), ctypes.c_int]
        L.cbc_unpack_targets_depth_cap.restype = ctypes.c_uint64
        L.cbc_unpack_targets_depth_cap.argtypes = [ctypes.POINTER(UnpackPlanC), ctypes.POINTER(TargetsC), ctypes.c_uint32]
        L.cbc_unpack_targets_depth_skipdel_cap.restype = ctypes.c_uint64
        L.cbc_unpack_targets_depth_skipdel_cap.argtypes = [ctypes.POINTER(UnpackPlanC), ctypes.POINTER(TargetsC), ctypes.c_uint32]
        L.cbc_unpack_queries.restype = ctypes.c_int
        L.cbc_unpack_queries.argtypes = [ctypes.POINTER(UnpackPlanC), ctypes.POINTER(ctypes.c_char_p), ctypes.c_uint32, ctypes.c_void_p,
                                         ctypes.c_size_t, ctypes.c_uint64, ctypes.POINTER(ctypes.POINTER(QueriesC)), ctypes.c_char_p,
                                         ctypes.c_size_t]
        L.cbc_queries_free.restype = None
        L.cbc_queries_free.argtypes = [ctypes.POINTER(QueriesC)]
        L.cbc_coverage_mean.restype = ctypes.c_int
        L.cbc_coverage_mean.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_char_p]
        L.cbc_unpack_targets_size.restype = ctypes.c_uint64
        L.cbc_unpack_targets_size.argtypes = [ctypes.POINTER(TargetsC), ctypes.c_uint32]
        L.cbc_hist_fraction.restype = ctypes.c_int
        L.cbc_hist_fraction.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_char_p]
        L.cbc_stats_text_cap.restype = ctypes.c_uint64
        L.cbc_stats_text_cap.argtypes = []
        L.cbc_stats_text.restype = ctypes.c_int64
        L.cbc_stats_text.argtypes = [ctypes.POINTER(GpuStats), ctypes.c_char_p, ctypes.c_uint64]
        L.cbc_stats_aln_text_cap.restype = ctypes.c_uint64
        L.cbc_stats_aln_text_cap.argtypes = []
        L.cbc_stats_aln_text.restype = ctypes.c_int64
        L.cbc_stats_aln_text.argtypes = [ctypes.POINTER(GpuStatsAln), ctypes.c_char_p, ctypes.c_uint64]
        _lib = L
    return _lib


class GpuStats(ctypes.Structure):
    """cbc_gpu_stats (include/cbc_gpu.h): the tables of cbc_gpu_decode_stats."""
    _fields_ = [("reads", ctypes.c_uint64), ("excluded", ctypes.c_uint64), ("flag", ctypes.c_uint32 * 65536),
                ("len", ctypes.c_uint32 * 257), ("gc", ctypes.c_uint32 * 101), ("cyc", ctypes.c_uint32 * (5 * 256))]


def stats_text(stats) -> bytes:
    """What `cbc -x --stats` writes for the tables (cbc_stats_text).  stats: the dict of Encoder.decode_stats -- reads, excluded,
    flag (65536), len (257), gc (101), cyc (5, 256) -- or a GpuStats."""
    if not isinstance(stats, GpuStats):
        st = GpuStats()
        st.reads, st.excluded = int(stats["reads"]), int(stats["excluded"])
        for name, n in (("flag", 65536), ("len", 257), ("gc", 101), ("cyc", 1280)):
            a = np.ascontiguousarray(stats[name], dtype=np.uint32).reshape(-1)
            if a.size != n:
                raise ValueError("stats[%r] wants %d counters" % (name, n))
            ctypes.memmove(getattr(st, name), a.ctypes.data, 4 * n)
        stats = st
    cap = int(lib().cbc_stats_text_cap())
    buf = ctypes.create_string_buffer(cap)
    n = lib().cbc_stats_text(ctypes.byref(stats), buf, cap)
    if n < 0:
        raise ValueError("cbc_stats_text failed (%d)" % n)
    return buf.raw[:n]


class GpuStatsAln(ctypes.Structure):
    """cbc_gpu_stats_aln (include/cbc_gpu.h): the alignment tables of cbc_gpu_decode_stats_aln."""
    _fields_ = [("reads", ctypes.c_uint64), ("invalid", ctypes.c_uint64), ("len", ctypes.c_uint32 * 257), ("mm", ctypes.c_uint32 * 257),
                ("unal", ctypes.c_uint32 * 257), ("ins_cyc", ctypes.c_uint32 * 257), ("del_cyc", ctypes.c_uint32 * 257),
                ("nm", ctypes.c_uint32 * 767), ("ins_len", ctypes.c_uint64 * 256), ("del_len", ctypes.c_uint64 * 256)]


STATS_ALN_TABLES = (("len", 257, np.uint32), ("mm", 257, np.uint32), ("unal", 257, np.uint32), ("ins_cyc", 257, np.uint32),
                    ("del_cyc", 257, np.uint32), ("nm", 767, np.uint32), ("ins_len", 256, np.uint64), ("del_len", 256, np.uint64))


def stats_aln_dict(st: "GpuStatsAln") -> dict:
    """A GpuStatsAln as the dict Encoder.decode_stats_aln returns: reads, invalid (int) and the tables as arrays."""
    out = dict(reads=int(st.reads), invalid=int(st.invalid))
    for name, _, _ in STATS_ALN_TABLES:
        out[name] = np.ctypeslib.as_array(getattr(st, name)).copy()
    return out


def stats_aln_text(aln) -> bytes:
    """The sections `cbc -x --stats --alignment` writes behind the text of stats_text (cbc_stats_aln_text).  aln: the second dict
    of Encoder.decode_stats_aln -- reads, invalid, len, mm, unal, ins_cyc, del_cyc (257), nm (767), ins_len, del_len (256, 64
    bits) -- or a GpuStatsAln."""
    if not isinstance(aln, GpuStatsAln):
        st = GpuStatsAln()
        st.reads, st.invalid = int(aln["reads"]), int(aln["invalid"])
        for name, n, dt in STATS_ALN_TABLES:
            a = np.ascontiguousarray(aln[name], dtype=dt).reshape(-1)
            if a.size != n:
                raise ValueError("aln[%r] wants %d counters" % (name, n))
            ctypes.memmove(getattr(st, name), a.ctypes.data, a.nbytes)
        aln = st
    cap = int(lib().cbc_stats_aln_text_cap())
    buf = ctypes.create_string_buffer(cap)
    n = lib().cbc_stats_aln_text(ctypes.byref(aln), buf, cap)
    if n < 0:
        raise ValueError("cbc_stats_aln_text failed (%d)" % n)
    return buf.raw[:n]


def hist_fraction(bases: int, size: int) -> bytes:
    """bases / size with six decimals by the integer rule of cbc_hist_fraction (what `cbc --depth-hist` prints)."""
    buf = ctypes.create_string_buffer(40)
    n = lib().cbc_hist_fraction(int(bases), int(size), buf)
    if n < 0:
        raise ValueError("cbc_hist_fraction failed (%d)" % n)
    return buf.raw[:n]


def coverage_mean(total: int, length: int) -> bytes:
    """The mean depth total / length with two decimals by the integer rule of cbc_coverage_mean (what `cbc --bedcov` prints)."""
    buf = ctypes.create_string_buffer(32)
    n = lib().cbc_coverage_mean(int(total), int(length), buf)
    if n < 0:
        raise ValueError("cbc_coverage_mean failed (%d)" % n)
    return buf.raw[:n]


def _opts(block_reads=None, max_cap_pos=None, max_cap_var=None, var_length=False, threads=None, whole_file=False,
          long_reads=False):
    o = PackOpts()
    lib().cbc_pack_default_opts(ctypes.byref(o))
    if block_reads is not None:
        o.block_reads = block_reads
    if max_cap_pos is not None:
        o.max_cap_pos = max_cap_pos
    if max_cap_var is not None:
        o.max_cap_var = max_cap_var
    o.var_length = 1 if var_length else 0
    if threads is not None:
        o.n_threads = threads                  # 0 = one per online CPU, 1 = serial text path
    o.whole_file = 1 if whole_file else 0      # "compat": one stream per file, the reference's own format
    o.long_reads = 1 if long_reads else 0      # the long-read format extension (stream version 3)
    if long_reads and block_reads is None:
        o.block_reads = 64
    return o


def _np_view(ptr, n, dtype):
    if n == 0:
        return np.zeros(0, dtype=dtype)
    addr = ctypes.addressof(ptr.contents)
    nbytes = int(n) * np.dtype(dtype).itemsize
    buf = (ctypes.c_uint8 * nbytes).from_address(addr)
    return np.frombuffer(buf, dtype=dtype)


REC_DTYPE = np.dtype([("pos", "<u4"), ("flag", "<u2"), ("rlen", "<u2"), ("seq_off", "<u4"), ("tok_off", "<u4")])
BLOCK_DTYPE = np.dtype([("rec_base", "<u8"), ("seq_base", "<u8"), ("tok_base", "<u8"), ("ref_off", "<u8"),
                        ("out_off", "<u8"), ("out_cap", "<u4"), ("n_reads", "<u4"), ("name_off", "<u4"),
                        ("read_length", "<u4"), ("n_tok", "<u4"), ("reserved", "<u4")])
RESULT_DTYPE = np.dtype([("nbytes", "<u4"), ("status", "<u4"), ("n_symbols", "<u4"), ("fail_read", "<u4")])
INFO_DTYPE = np.dtype([("contig", "<u4"), ("n_reads", "<u4"), ("window_start", "<u8"), ("n_bases", "<u8")])
CONTIG_DTYPE = np.dtype([("ref_off", "<u8"), ("length", "<u8"), ("name_off", "<u4"), ("reserved", "<u4")])
DEC_BLOCK_DTYPE = np.dtype([("in_off", "<u8"), ("ref_off", "<u8"), ("rec_base", "<u8"), ("seq_base", "<u8"),
                            ("in_bytes", "<u4"), ("n_reads", "<u4"), ("read_length", "<u4"), ("seq_stride", "<u4"),
                            ("reserved", "<u4", (4,))])
assert REC_DTYPE.itemsize == 16 and BLOCK_DTYPE.itemsize == 64 and RESULT_DTYPE.itemsize == 16
assert DEC_BLOCK_DTYPE.itemsize == 64


class PackedBatch:
    """Owns a cbc_packed* and exposes its arrays as numpy views (zero copy)."""

    def __init__(self, ptr):
        self._ptr = ptr
        p = ptr.contents
        self.recs = _np_view(p.recs, p.n_recs, REC_DTYPE)
        # a batch from the device tokeniser may carry sizes only: the bases and tokens are resident on the GPU
        self.seq = _np_view(p.seq, p.seq_bytes, np.uint8) if p.seq else np.zeros(0, dtype=np.uint8)
        self.tok = _np_view(p.tok, max(int(p.n_tok), 1), np.uint32) if p.tok else np.zeros(0, dtype=np.uint32)
        self.names = _np_view(p.names, p.names_bytes, np.uint8)
        self.blocks = _np_view(p.blocks, p.n_blocks, BLOCK_DTYPE)
        self.info = _np_view(p.info, p.n_blocks, INFO_DTYPE)
        self.contigs = _np_view(p.contigs, p.n_contigs, CONTIG_DTYPE)
        self.ref = _np_view(p.ref, p.ref_bytes, np.uint8)
        self.cap_pos = int(p.caps.cap_pos)
        self.cap_var = int(p.caps.cap_var)
        self.read_length = int(p.read_length)
        self.n_bases = int(p.n_bases)
        self.n_recs = int(p.n_recs)
        self.n_tok = int(p.n_tok)
        self.n_blocks = int(p.n_blocks)
        self.n_skipped_unmapped = int(p.n_skipped_unmapped)
        self.whole_file = int(p.whole_file) == 1
        self.long_reads = int(p.whole_file) == 2
        self.max_read_len = int(p.max_read_len)

    @property
    def c_ptr(self):
        return self._ptr

    def contig_name(self, ci):
        off = int(self.contigs[ci]["name_off"])
        raw = self.names[off:].tobytes()
        return raw[:raw.index(b"\0")]

    def assign_contigs(self, n_parts):
        """Whole contigs dealt to n_parts, largest first to the least loaded part (cbc_assign_contigs).  Returns the
        part of every contig; blocks_of_part() turns it into block index lists."""
        out = np.zeros(max(len(self.contigs), 1), dtype=np.uint32)
        rc = lib().cbc_assign_contigs(self._ptr, n_parts, out.ctypes.data)
        if rc != 0:
            raise RuntimeError("cbc_assign_contigs failed: %d" % rc)
        return out[:len(self.contigs)]

    def blocks_of_part(self, part_of_contig, part):
        return [b for b in range(self.n_blocks) if int(part_of_contig[int(self.info[b]["contig"])]) == part]

    def container(self, payloads: np.ndarray, out_offsets: np.ndarray) -> bytes:
        offs = np.ascontiguousarray(out_offsets, dtype=np.uint64)
        po = offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        n = lib().cbc_container_size(self._ptr, po)
        if n < 0:
            raise RuntimeError("cbc_container_size failed: %d" % n)
        dst = np.zeros(int(n), dtype=np.uint8)
        pl = np.ascontiguousarray(payloads, dtype=np.uint8)
        w = lib().cbc_container_write(self._ptr, pl.ctypes.data, po, dst.ctypes.data, int(n))
        if w != n:
            raise RuntimeError("cbc_container_write failed: %d" % w)
        return dst.tobytes()

    def close(self):
        if self._ptr is not None:
            # drop the numpy views before the C memory goes away
            for k in ("recs", "seq", "tok", "names", "blocks", "info", "contigs", "ref"):
                setattr(self, k, None)
            lib().cbc_packed_free(self._ptr)
            self._ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


SUMMARY_DTYPE = np.dtype([("pos", "<u4"), ("flag", "<u2"), ("rl", "<u2"), ("nt_ev", "<u4"), ("line", "<u4")])


def sam_body_offset(sam: bytes) -> int:
    return int(lib().cbc_sam_body_offset(sam, len(sam)))


def pack_from_device_tokens(sam: bytes, fasta: bytes, summaries, rname_change, change_off, change_len, n_unmapped,
                            seq=None, tok=None, seq_bytes=None, n_tok=None, **kw) -> PackedBatch:
    """The serial half of packing after the device tokeniser (cbc_pack_from_device_tokens): contig numbering and block
    cutting over the record summaries.  seq / tok: numpy copies of the tokeniser's arrays (the C side keeps its own
    copies) or None when they stay on the device."""
    o = _opts(**kw)
    out = ctypes.POINTER(Packed)()
    err = ctypes.create_string_buffer(512)
    summaries = np.ascontiguousarray(summaries, dtype=SUMMARY_DTYPE)
    rname_change = np.ascontiguousarray(rname_change, dtype=np.uint8)
    change_off = np.ascontiguousarray(change_off, dtype=np.uint64); change_len = np.ascontiguousarray(change_len, dtype=np.uint32)
    n = len(summaries)
    cseq = ctok = None
    if seq is not None:                       # hand the C side malloc'ed copies it may own
        libc = ctypes.CDLL(None)
        libc.malloc.restype = ctypes.c_void_p
        seq_bytes, n_tok = int(seq_bytes if seq_bytes is not None else len(seq) - 8), int(n_tok if n_tok is not None else len(tok))
        cseq = libc.malloc(seq_bytes + 16); ctok = libc.malloc(max(n_tok, 1) * 4)
        ctypes.memmove(cseq, np.ascontiguousarray(seq, dtype=np.uint8).ctypes.data, seq_bytes)
        ctypes.memmove(ctok, np.ascontiguousarray(tok, dtype=np.uint32).ctypes.data, n_tok * 4)
    rc = lib().cbc_pack_from_device_tokens(sam, len(sam), fasta, len(fasta), ctypes.byref(o), summaries.ctypes.data,
                                           rname_change.ctypes.data, change_off.ctypes.data, change_len.ctypes.data, n, n_unmapped,
                                           cseq, int(seq_bytes), ctok, int(n_tok), ctypes.byref(out), err, 512)
    if rc != 0:
        raise CbcInputError("cbc_pack_from_device_tokens failed (%d): %s" % (rc, err.value.decode(errors="replace")))
    return PackedBatch(out)


def pack_2bit(bases: np.ndarray, threads=0):
    """Bases -> 2-bit transport form (cbc_2bit_pack): (codes uint32 array, exception runs array of RUN_DTYPE)."""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    out = ctypes.POINTER(TwoBitC)()
    rc = lib().cbc_2bit_pack(bases.ctypes.data, bases.size, threads, ctypes.byref(out))
    if rc != 0:
        raise RuntimeError("cbc_2bit_pack failed: %d" % rc)
    p = out.contents
    codes = _np_view(p.codes, (int(p.n_bases) + 15) // 16, np.uint32).copy()
    runs = _np_view(p.runs, p.n_runs, RUN_DTYPE).copy() if p.n_runs else np.zeros(0, dtype=RUN_DTYPE)
    lib().cbc_2bit_free(out)
    return codes, runs


def unpack_2bit(codes: np.ndarray, runs: np.ndarray, n_bases: int) -> np.ndarray:
    """Host inverse of pack_2bit (cbc_2bit_unpack)."""
    codes = np.ascontiguousarray(codes, dtype=np.uint32)
    runs = np.ascontiguousarray(runs, dtype=RUN_DTYPE)
    c = TwoBitC(codes.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), n_bases,
                ctypes.cast(runs.ctypes.data, ctypes.POINTER(TwoBitRun)) if len(runs) else None, len(runs))
    out = np.zeros(n_bases, dtype=np.uint8)
    rc = lib().cbc_2bit_unpack(ctypes.byref(c), out.ctypes.data)
    if rc != 0:
        raise RuntimeError("cbc_2bit_unpack failed: %d" % rc)
    return out


def checksum64(data) -> int:
    """cbc_checksum64 over a bytes object or a uint8 numpy array (host twin of the device checksum)."""
    a = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else data, dtype=np.uint8)
    return int(lib().cbc_checksum64(a.ctypes.data if a.size else None, a.size))


def pack_sam(sam: bytes, fasta: bytes, **kw) -> PackedBatch:
    """SAM text + FASTA text -> packed blocks (the load_sam_line / store_reference_in_memory seam)."""
    o = _opts(**kw)
    out = ctypes.POINTER(Packed)()
    err = ctypes.create_string_buffer(512)
    rc = lib().cbc_pack_sam(sam, len(sam), fasta, len(fasta), ctypes.byref(o), ctypes.byref(out), err, 512)
    if rc != 0:
        raise CbcInputError("cbc_pack_sam failed (%d): %s" % (rc, err.value.decode(errors="replace")))
    return PackedBatch(out)


def synth_long(seed, contig_len, n_reads, read_len=10_000, edit_rate=0.05, name=b"chrL", want_text=False, **kw):
    """cfg5 workload: long reads with an indel + substitution mix, packed for the long-read format."""
    return synth(seed, contig_len, n_reads, read_len, edit_rate, 0.0, name, want_text, _long=True, **kw)


def synth(seed, contig_len, n_reads, read_len=150, sub_rate=0.003, indel_frac=0.02, name=b"chr1",
          want_text=False, _long=False, **kw):
    """Seeded synthetic workload.  Returns PackedBatch, or (PackedBatch, sam, fasta)."""
    so = SynthOpts(seed, contig_len, n_reads, read_len, sub_rate, indel_frac, name)
    o = _opts(long_reads=_long, **kw)
    out = ctypes.POINTER(Packed)()
    err = ctypes.create_string_buffer(512)
    sam_p, fa_p = ctypes.c_void_p(), ctypes.c_void_p()
    sam_n, fa_n = ctypes.c_size_t(), ctypes.c_size_t()
    fn = lib().cbc_synth_long if _long else lib().cbc_synth_packed
    rc = fn(ctypes.byref(so), ctypes.byref(o), ctypes.byref(out),
                                ctypes.byref(sam_p) if want_text else None, ctypes.byref(sam_n),
                                ctypes.byref(fa_p) if want_text else None, ctypes.byref(fa_n), err, 512)
    if rc != 0:
        raise CbcInputError("cbc_synth_packed failed (%d): %s" % (rc, err.value.decode(errors="replace")))
    pb = PackedBatch(out)
    if not want_text:
        return pb
    # ctypes.string_at takes a C int: texts of 2 GiB and more (10 M reads) go through a buffer view
    sam = bytes((ctypes.c_char * sam_n.value).from_address(sam_p.value)) if sam_n.value else b""
    fa = bytes((ctypes.c_char * fa_n.value).from_address(fa_p.value)) if fa_n.value else b""
    lib().cbc_free(sam_p)
    lib().cbc_free(fa_p)
    return pb, sam, fa


class RegionSelection:
    """What cbc_unpack_region chose: contig index, blocks [b0, b1), the clamped 1-based inclusive [beg, end], the span bound."""

    def __init__(self, contig, b0, b1, beg, end, smax, contig_len):
        self.contig, self.b0, self.b1, self.beg, self.end, self.smax, self.contig_len = contig, b0, b1, beg, end, smax, contig_len

    def __repr__(self):
        return "RegionSelection(contig=%d, blocks=[%d, %d), beg=%d, end=%d, smax=%d)" % (
            self.contig, self.b0, self.b1, self.beg, self.end, self.smax)


class TargetSet:
    """What cbc_unpack_targets made of a list of regions and a BED text (copies; nothing of the C object is kept):
    iv            (n_iv, 2) uint32: the merged intervals beg, end, 1-based inclusive, grouped per contig in table order
    contig_first, contig_count      per contig: its part of iv
    blocks        the selected blocks, ascending (the union of the single-region selections of the merged intervals)
    block_iv      (n_blocks, 2) uint32: per selected block the first interval and the count of those its reads can reach
    contig_blk_first, contig_blk_count   per contig: its part of blocks
    smax, bed_unselected (BED lines that selected nothing), n_input (regions + BED lines taken, before merging),
    text_cap_reads, text_cap_sam, depth_cap[c]: buffer sizes that always hold the output;
    size[c]: the positions inside contig c's merged intervals (cbc_unpack_targets_size)."""

    def __init__(self, plan, ptr):
        t = ptr.contents
        n_iv, nb, nc = int(t.n_iv), int(t.n_blocks), int(t.n_contigs)
        self.n_iv, self.n_blocks, self.n_contigs, self.smax = n_iv, nb, nc, int(t.smax)
        self.iv = _np_view(t.iv, 2 * n_iv, np.uint32).copy().reshape(n_iv, 2) if n_iv else np.zeros((0, 2), dtype=np.uint32)
        self.contig_first = _np_view(t.contig_first, nc, np.uint32).copy()
        self.contig_count = _np_view(t.contig_count, nc, np.uint32).copy()
        self.blocks = _np_view(t.blocks, nb, np.uint32).copy() if nb else np.zeros(0, dtype=np.uint32)
        self.block_iv = _np_view(t.block_iv, 2 * nb, np.uint32).copy().reshape(nb, 2) if nb else np.zeros((0, 2), dtype=np.uint32)
        self.contig_blk_first = _np_view(t.contig_blk_first, nc, np.uint32).copy()
        self.contig_blk_count = _np_view(t.contig_blk_count, nc, np.uint32).copy()
        self.bed_unselected, self.n_input = int(t.bed_unselected), int(t.n_input)
        self.text_cap_reads = int(lib().cbc_unpack_targets_text_cap(plan._ptr, ptr, 0))
        self.text_cap_sam = int(lib().cbc_unpack_targets_text_cap(plan._ptr, ptr, 1))
        self.depth_cap = [int(lib().cbc_unpack_targets_depth_cap(plan._ptr, ptr, c)) for c in range(nc)]
        self.depth_skipdel_cap = [int(lib().cbc_unpack_targets_depth_skipdel_cap(plan._ptr, ptr, c)) for c in range(nc)]
        self.size = [int(lib().cbc_unpack_targets_size(ptr, c)) for c in range(nc)]

    def intervals(self):
        """[(contig, beg, end)] of the merged intervals, in order."""
        return [(c, int(b), int(e)) for c in range(self.n_contigs)
                for b, e in self.iv[int(self.contig_first[c]):int(self.contig_first[c]) + int(self.contig_count[c])]]

    def __repr__(self):
        return "TargetSet(%d intervals, %d blocks, smax=%d)" % (self.n_iv, self.n_blocks, self.smax)


class QuerySet:
    """What cbc_unpack_queries made of a list of regions, a BED text and a window (copies; nothing of the C object is kept):
    q             structured array (QUERY_DTYPE), one entry per query in input order: contig (QUERY_UNKNOWN: not in the table),
                  beg / end (1-based inclusive, clamped), slot (first slot in the contig's compressed coordinate), name_off /
                  name_len (unknown contig: the chrom text inside the BED text), start0 / end0 (what the output echoes)
    contig        int64, -1 for an unknown contig;  start0, end0: uint64;  length = end0 - start0
    targets       the TargetSet of the same input (merged intervals, selected blocks)"""

    def __init__(self, plan, ptr, bed):
        c = ptr.contents
        self.n_q = int(c.n_q)
        self.q = _np_view(ctypes.cast(c.q, ctypes.POINTER(ctypes.c_uint8)), self.n_q * QUERY_DTYPE.itemsize, np.uint8).copy().view(QUERY_DTYPE) \
            if self.n_q else np.zeros(0, dtype=QUERY_DTYPE)
        self.targets = TargetSet(plan, c.targets)
        self.contig = np.where(self.q["contig"] == QUERY_UNKNOWN, -1, self.q["contig"].astype(np.int64))
        self.start0, self.end0 = self.q["start0"].copy(), self.q["end0"].copy()
        self._bed = bytes(bed) if bed else b""
        self._names = [plan.names[int(o):].tobytes().split(b"\0", 1)[0] for o in plan.contig_name_off]

    def chrom(self, i):
        """The first column of query i: the contig's name, or the BED line's own text for a contig the container does not list."""
        x = self.q[i]
        if int(x["contig"]) == QUERY_UNKNOWN:
            return self._bed[int(x["name_off"]):int(x["name_off"]) + int(x["name_len"])]
        return self._names[int(x["contig"])]

    def __repr__(self):
        return "QuerySet(%d queries, %r)" % (self.n_q, self.targets)


class UnpackPlan:
    """Container + FASTA -> decode launch plan (cbc_unpack_plan_create).  Keeps the container bytes alive."""

    def __init__(self, container: bytes, fasta: bytes):
        self._blob = np.frombuffer(container, dtype=np.uint8).copy()
        out = ctypes.POINTER(UnpackPlanC)()
        err = ctypes.create_string_buffer(512)
        rc = lib().cbc_unpack_plan_create(self._blob.ctypes.data, self._blob.size, fasta, len(fasta),
                                          ctypes.byref(out), err, 512)
        if rc != 0:
            raise CbcInputError("cbc_unpack_plan_create failed (%d): %s" % (rc, err.value.decode(errors="replace")))
        self._ptr = out
        p = out.contents
        self.n_blocks = int(p.n_blocks)
        self.n_recs = int(p.n_recs)
        self.read_length = int(p.read_length)
        self.seq_stride = int(p.seq_stride)
        self.cap_pos, self.cap_var = int(p.caps.cap_pos), int(p.caps.cap_var)
        self.blocks = _np_view(p.blocks, p.n_blocks, DEC_BLOCK_DTYPE)
        self.payloads = _np_view(p.payloads, p.payload_bytes, np.uint8)
        self.ref = _np_view(p.ref, p.ref_bytes, np.uint8)
        self.window_start = _np_view(p.window_start, p.n_blocks, np.uint64)
        self.long_reads = bool(p.long_reads)
        self.max_read_len = int(p.max_read_len)
        self.seq_total = int(p.seq_total)
        # the container's contig table (SAM output: @SQ lines, RNAME)
        self.n_contigs = int(p.n_contigs)
        self.block_contig = _np_view(p.block_contig, p.n_blocks, np.uint32)
        self.contig_name_off = _np_view(p.contig_name_off, p.n_contigs, np.uint32)
        self.contig_len = _np_view(p.contig_len, p.n_contigs, np.uint64)
        self.names = np.frombuffer((ctypes.c_uint8 * (int(p.names_bytes) + 1)).from_address(p.names), dtype=np.uint8)[:int(p.names_bytes)]

    def region(self, region):
        """Blocks that can hold a read overlapping `region` (NAME, NAME:BEG or NAME:BEG-END, 1-based inclusive):
        cbc_unpack_region.  Returns a RegionSelection; raises CbcInputError for a malformed or unknown region and for a
        long-read container."""
        if isinstance(region, str):
            region = region.encode()
        sel = RegionSelC()
        err = ctypes.create_string_buffer(512)
        rc = lib().cbc_unpack_region(self._ptr, region, ctypes.byref(sel), err, 512)
        if rc != 0:
            raise CbcInputError("cbc_unpack_region failed (%d): %s" % (rc, err.value.decode(errors="replace")))
        return RegionSelection(int(sel.contig), int(sel.b0), int(sel.b1), int(sel.beg), int(sel.end), int(sel.smax),
                               int(sel.contig_len))

    def targets(self, regions=(), bed=None):
        """The target set of the region strings `regions` (each NAME, NAME:BEG or NAME:BEG-END, as for region()) and the BED
        text `bed` (bytes; None: no file): cbc_unpack_targets.  Returns a TargetSet; raises CbcInputError for what region()
        refuses, for a BED line that is malformed (the message names the line) and for what sam_header() refuses."""
        if isinstance(regions, (str, bytes)):
            regions = [regions]
        rs = [r.encode() if isinstance(r, str) else bytes(r) for r in regions]
        arr = (ctypes.c_char_p * max(len(rs), 1))(*rs)
        if isinstance(bed, str):
            bed = bed.encode()
        buf = np.frombuffer(bed, dtype=np.uint8).copy() if bed else None       # exactly the bytes: no terminator behind them
        out = ctypes.POINTER(TargetsC)()
        err = ctypes.create_string_buffer(512)
        rc = lib().cbc_unpack_targets(self._ptr, arr, len(rs), buf.ctypes.data if buf is not None else None,
                                      buf.size if buf is not None else 0, ctypes.byref(out), err, 512)
        if rc != 0:
            raise CbcInputError("cbc_unpack_targets failed (%d): %s" % (rc, err.value.decode(errors="replace")))
        try:
            return TargetSet(self, out)
        finally:
            lib().cbc_targets_free(out)

    def queries(self, regions=(), bed=None, window=0):
        """The query list of a per-target coverage summary (cbc_unpack_queries): every region string, then every BED line,
        unmerged and in input order -- lines that select nothing included, with length 0 -- or one query per contig when
        regions is empty and bed is None; window > 0 cuts every query into windows of that many bases.  Returns a QuerySet;
        raises CbcInputError for what targets() refuses and for more than 2^24 queries."""
        if isinstance(regions, (str, bytes)):
            regions = [regions]
        rs = [r.encode() if isinstance(r, str) else bytes(r) for r in regions]
        arr = (ctypes.c_char_p * max(len(rs), 1))(*rs)
        if isinstance(bed, str):
            bed = bed.encode()
        # exactly the bytes: no terminator behind them; an empty text is still a text (no line), not "no file"
        buf = None if bed is None else np.frombuffer(bed, dtype=np.uint8).copy() if len(bed) else np.zeros(1, dtype=np.uint8)
        out = ctypes.POINTER(QueriesC)()
        err = ctypes.create_string_buffer(512)
        rc = lib().cbc_unpack_queries(self._ptr, arr, len(rs), buf.ctypes.data if buf is not None else None,
                                      len(bed) if bed is not None else 0, int(window), ctypes.byref(out), err, 512)
        if rc != 0:
            raise CbcInputError("cbc_unpack_queries failed (%d): %s" % (rc, err.value.decode(errors="replace")))
        try:
            return QuerySet(self, out, bed)
        finally:
            lib().cbc_queries_free(out)

    def contig_blocks(self, contig: int):
        """The selection of contig `contig` as a whole (cbc_unpack_contig_blocks): its blocks, beg = 1, end = its length."""
        sel = RegionSelC()
        err = ctypes.create_string_buffer(512)
        rc = lib().cbc_unpack_contig_blocks(self._ptr, int(contig), ctypes.byref(sel), err, 512)
        if rc != 0:
            raise CbcInputError("cbc_unpack_contig_blocks failed (%d): %s" % (rc, err.value.decode(errors="replace")))
        return RegionSelection(int(sel.contig), int(sel.b0), int(sel.b1), int(sel.beg), int(sel.end), int(sel.smax),
                               int(sel.contig_len))

    def depth_text_cap(self, b0, b1, contig) -> int:
        """Bytes that always hold the bedGraph of blocks [b0, b1) of contig `contig` (cbc_unpack_depth_text_cap)."""
        return int(lib().cbc_unpack_depth_text_cap(self._ptr, b0, b1, contig))

    def depth_skipdel_text_cap(self, b0, b1, contig, beg, end, smax) -> int:
        """Bytes that always hold the bedGraph of blocks [b0, b1) of contig `contig` for the window [beg, end] and the span bound
        smax when deleted bases do not count (Encoder.decode_depth(skip_deletions=True); cbc_unpack_depth_skipdel_text_cap)."""
        return int(lib().cbc_unpack_depth_skipdel_text_cap(self._ptr, b0, b1, contig, beg, end, smax))

    def pileup_text_cap(self, b0, b1, contig, beg, end, smax, by_strand=False) -> int:
        """Bytes that always hold the pileup lines of blocks [b0, b1) of contig `contig` for the window [beg, end] and the span
        bound smax (cbc_unpack_pileup_text_cap); by_strand=True: the lines with the seven per-strand columns
        (cbc_unpack_pileup_ext_text_cap)."""
        if by_strand:
            return int(lib().cbc_unpack_pileup_ext_text_cap(self._ptr, b0, b1, contig, beg, end, smax, 1))
        return int(lib().cbc_unpack_pileup_text_cap(self._ptr, b0, b1, contig, beg, end, smax))

    def consensus_text_cap(self, contig, beg, end, line_width=60, with_range=False) -> int:
        """The bytes of the consensus record of window [beg, end] of contig `contig` when every position writes a byte
        (cbc_unpack_consensus_text_cap): exact with show_del, a bound otherwise; 0 for a window or a width it refuses."""
        return int(lib().cbc_unpack_consensus_text_cap(self._ptr, contig, beg, end, line_width, int(bool(with_range))))

    def consensus_empty(self, contig, beg, end, opts: "ConsensusOpts", with_range=False):
        """The consensus record of a window no read covers, written on the host (cbc_unpack_consensus_empty): every position low
        depth.  Returns (fasta bytes, counts dict)."""
        cap = self.consensus_text_cap(contig, beg, end, opts.line_width, with_range)
        text = np.zeros(max(cap, 1), dtype=np.uint8)
        cnt = ConsensusCounts()
        n = int(lib().cbc_unpack_consensus_empty(self._ptr, contig, beg, end, ctypes.byref(opts), int(bool(with_range)), text.ctypes.data,
                                                  cap, ctypes.byref(cnt)))
        if cap == 0 or n < 0:
            raise ValueError("consensus: a window, a line width or an option the record cannot be written for")
        return text[:n].tobytes(), cnt.as_dict()

    def sam_header(self) -> bytes:
        """@HD and one @SQ line per contig of the container's table (cbc_unpack_sam_header): what precedes the alignment
        lines of Encoder.decode_sam.  Raises CbcInputError for what SAM cannot carry: a long-read container, a contig longer
        than 2^31 - 1 bases, a name that is empty, longer than 255 bytes or holds a tab or a newline."""
        err = ctypes.create_string_buffer(512)
        n = lib().cbc_unpack_sam_header(self._ptr, None, 0, err, 512)
        if n < 0:
            raise CbcInputError("cbc_unpack_sam_header failed (%d): %s" % (n, err.value.decode(errors="replace")))
        dst = np.zeros(int(n), dtype=np.uint8)
        w = lib().cbc_unpack_sam_header(self._ptr, dst.ctypes.data, int(n), err, 512)
        if w != n:
            raise RuntimeError("cbc_unpack_sam_header failed: %d" % w)
        return dst.tobytes()

    def sam_text_cap(self, b0=0, b1=None) -> int:
        """Bytes that always hold the alignment lines of blocks [b0, b1) (cbc_unpack_sam_text_cap)."""
        return int(lib().cbc_unpack_sam_text_cap(self._ptr, b0, self.n_blocks if b1 is None else b1))

    def sam_cigar_text_cap(self, b0=0, b1=None, edits_per_read=0) -> int:
        """Bytes that always hold the alignment lines of blocks [b0, b1) with CIGAR, NM and MD, for an arena of edits_per_read
        entries per read (0: the default) (cbc_unpack_sam_cigar_text_cap)."""
        return int(lib().cbc_unpack_sam_cigar_text_cap(self._ptr, b0, self.n_blocks if b1 is None else b1, edits_per_read))

    def text(self, recs: np.ndarray, seq: np.ndarray) -> bytes:
        """One reconstructed read per line (what `cbc -d` writes)."""
        cap = (int(self.seq_total) + int(self.n_recs) + 16) if self.long_reads else int(self.n_recs) * (self.seq_stride + 1) + 16
        dst = np.zeros(cap, dtype=np.uint8)
        recs = np.ascontiguousarray(recs)
        seq = np.ascontiguousarray(seq)
        n = lib().cbc_unpack_write_text(self._ptr, recs.ctypes.data, seq.ctypes.data, dst.ctypes.data, cap)
        if n < 0:
            raise RuntimeError("cbc_unpack_write_text failed: %d" % n)
        return dst[:int(n)].tobytes()

    def close(self):
        if self._ptr is not None:
            for k in ("blocks", "payloads", "ref", "window_start", "block_contig", "contig_name_off", "contig_len", "names"):
                setattr(self, k, None)
            lib().cbc_unpack_plan_free(self._ptr)
            self._ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
