"""ctypes binding of libcbc_gpu.so -- the C ABI of include/cbc_gpu.h (HIP kernels for gfx950).

There is no CPU fallback: if the library is not built or no MI355X is visible, every entry point
raises.  Python here only moves pointers; `torch` (when used by bench.py / the multi-GPU host) only
owns device memory and process groups.
"""
import contextlib
import ctypes
import os
import re

import numpy as np

from . import host

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
GPU_LIB = os.environ.get("CBC_GPU_LIB", os.path.join(_CSRC, "libcbc_gpu.so"))   # override = kernel experiments only

ST_NAMES = {0: "OK", 1: "OUT_FULL", 2: "ASSERT", 3: "CAP_POS", 4: "CAP_FLAG", 5: "CAP_VAR", 6: "CAP_NAME",
            7: "UNSUPPORTED"}


class HostBatch(ctypes.Structure):
    _fields_ = [
        ("recs", ctypes.c_void_p), ("n_recs", ctypes.c_uint64),
        ("seq", ctypes.c_void_p), ("seq_bytes", ctypes.c_uint64),
        ("tok", ctypes.c_void_p), ("n_tok", ctypes.c_uint64),
        ("names", ctypes.c_void_p), ("names_bytes", ctypes.c_uint32),
        ("blocks", ctypes.c_void_p), ("n_blocks", ctypes.c_uint32),
        ("caps", host.LdsCaps),
    ]


class DeviceBatch(ctypes.Structure):
    _fields_ = [
        ("d_recs", ctypes.c_void_p), ("d_seq", ctypes.c_void_p), ("d_tok", ctypes.c_void_p),
        ("d_names", ctypes.c_void_p), ("d_blocks", ctypes.c_void_p), ("n_blocks", ctypes.c_uint32),
        ("d_ref", ctypes.c_void_p), ("ref_bytes", ctypes.c_uint64),
        ("d_out", ctypes.c_void_p), ("out_bytes", ctypes.c_uint64),
        ("d_results", ctypes.c_void_p),
        ("seq_bytes", ctypes.c_uint64), ("n_tok", ctypes.c_uint64), ("n_recs", ctypes.c_uint64),
        ("caps", host.LdsCaps),
    ]


class DecDeviceBatch(ctypes.Structure):
    _fields_ = [
        ("d_in", ctypes.c_void_p), ("in_bytes", ctypes.c_uint64),
        ("d_blocks", ctypes.c_void_p), ("n_blocks", ctypes.c_uint32),
        ("d_ref", ctypes.c_void_p), ("ref_bytes", ctypes.c_uint64),
        ("d_recs", ctypes.c_void_p), ("n_recs", ctypes.c_uint64),
        ("d_seq", ctypes.c_void_p), ("seq_bytes", ctypes.c_uint64),
        ("d_results", ctypes.c_void_p),
        ("d_var_scratch", ctypes.c_void_p), ("var_scratch_words", ctypes.c_uint64),
        ("caps", host.LdsCaps),
    ]


class StreamResult(ctypes.Structure):
    _fields_ = [("nbytes", ctypes.c_uint64), ("status", ctypes.c_uint32), ("fail_read", ctypes.c_uint32),
                ("n_symbols", ctypes.c_uint64)]


class TokResult(ctypes.Structure):
    _fields_ = [("n_lines", ctypes.c_uint64), ("n_recs", ctypes.c_uint64), ("n_unmapped", ctypes.c_uint64), ("seq_bytes", ctypes.c_uint64),
                ("n_tok", ctypes.c_uint64), ("summaries", ctypes.c_void_p), ("rname_change", ctypes.c_void_p),
                ("change_name_off", ctypes.c_void_p), ("change_name_len", ctypes.c_void_p), ("n_changes", ctypes.c_uint64),
                ("d_seq", ctypes.c_void_p), ("d_tok", ctypes.c_void_p), ("status", ctypes.c_uint32), ("bad_line", ctypes.c_uint64)]


TOK_STATUS = {3: "the file needs the host packer (leading soft clip or a record without MD)", 4: "fewer than 11 columns",
              5: "line longer than 1023 bytes", 6: "bad CIGAR length", 7: "CIGAR '*' on a mapped record", 8: "MD gap too large",
              9: "MD inconsistent with CIGAR/SEQ", 10: "read length outside 1..252", 11: "POS < 1", 12: "too many CIGAR/MD tokens"}


class E2ETimes(ctypes.Structure):
    _fields_ = [("total_s", ctypes.c_double), ("alloc_s", ctypes.c_double), ("issue_s", ctypes.c_double), ("kernels_done_s", ctypes.c_double),
                ("h2d_bytes", ctypes.c_uint64), ("d2h_bytes", ctypes.c_uint64), ("n_chunks", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class GpuTargets(ctypes.Structure):
    _fields_ = [("iv", ctypes.c_void_p), ("block_iv", ctypes.c_void_p), ("n_iv", ctypes.c_uint32), ("smax", ctypes.c_uint32)]


class SamRegion(ctypes.Structure):
    _fields_ = [("beg", ctypes.c_uint64), ("end", ctypes.c_uint64), ("smax", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class CbcGpuError(RuntimeError):
    pass


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(GPU_LIB):
            raise CbcGpuError("libcbc_gpu.so is not built (cbc_amd/csrc): the HIP path is the only path; "
                              "run __graft_entry__.build() or `make -C cbc_amd/csrc`")
        L = ctypes.CDLL(GPU_LIB)
        L.cbc_gpu_abi_version.restype = ctypes.c_int
        L.cbc_gpu_device_count.restype = ctypes.c_int
        L.cbc_gpu_init.restype = ctypes.c_int
        L.cbc_gpu_init.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
        L.cbc_gpu_shutdown.restype = ctypes.c_int
        L.cbc_gpu_shutdown.argtypes = [ctypes.c_void_p]
        L.cbc_gpu_last_error.restype = ctypes.c_char_p
        L.cbc_gpu_last_error.argtypes = [ctypes.c_void_p]
        L.cbc_gpu_upload_reference.restype = ctypes.c_int
        L.cbc_gpu_upload_reference.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
        L.cbc_gpu_encode_blocks.restype = ctypes.c_int
        L.cbc_gpu_encode_blocks.argtypes = [ctypes.c_void_p, ctypes.POINTER(HostBatch), ctypes.c_void_p,
                                            ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
        L.cbc_gpu_encode_blocks_device.restype = ctypes.c_int
        L.cbc_gpu_encode_blocks_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(DeviceBatch), ctypes.c_void_p]
        L.cbc_gpu_compact_device.restype = ctypes.c_int
        L.cbc_gpu_compact_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                             ctypes.c_void_p]
        L.cbc_gpu_decode_blocks_device.restype = ctypes.c_int
        L.cbc_gpu_decode_blocks_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(DecDeviceBatch), ctypes.c_void_p]
        L.cbc_gpu_decode_blocks.restype = ctypes.c_int
        L.cbc_gpu_decode_blocks.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                            ctypes.c_uint32, ctypes.POINTER(host.LdsCaps), ctypes.c_void_p,
                                            ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
        L.cbc_gpu_decode_lds_bytes.restype = ctypes.c_uint32
        L.cbc_gpu_decode_lds_bytes.argtypes = [ctypes.POINTER(host.LdsCaps)]
        L.cbc_gpu_plan_output.restype = ctypes.c_uint64
        L.cbc_gpu_plan_output.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
        L.cbc_gpu_plan_output_caps.restype = ctypes.c_uint64
        L.cbc_gpu_plan_output_caps.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(host.LdsCaps)]
        L.cbc_gpu_reserve_encode.restype = ctypes.c_int
        L.cbc_gpu_reserve_encode.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64]
        L.cbc_gpu_lds_bytes.restype = ctypes.c_uint32
        L.cbc_gpu_lds_bytes.argtypes = [ctypes.POINTER(host.LdsCaps)]
        L.cbc_gpu_last_kernel_ms.restype = ctypes.c_int
        L.cbc_gpu_last_kernel_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]
        L.cbc_gpu_encode_stream.restype = ctypes.c_int
        L.cbc_gpu_encode_stream.argtypes = [ctypes.c_void_p, ctypes.POINTER(HostBatch), ctypes.c_void_p, ctypes.c_uint64,
                                            ctypes.POINTER(StreamResult)]
        L.cbc_gpu_encode_stream_blocks.restype = ctypes.c_int
        L.cbc_gpu_encode_stream_blocks.argtypes = [ctypes.c_void_p, ctypes.POINTER(HostBatch), ctypes.c_void_p, ctypes.c_uint64,
                                                   ctypes.c_void_p, ctypes.c_void_p]
        L.cbc_gpu_decode_stream.restype = ctypes.c_int
        L.cbc_gpu_decode_stream.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                            ctypes.c_uint32, ctypes.POINTER(StreamResult)]
        L.cbc_gpu_decode_stream_blocks.restype = ctypes.c_int
        L.cbc_gpu_decode_stream_blocks.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32,
                                                   ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
        L.cbc_gpu_group_create.restype = ctypes.c_int
        L.cbc_gpu_group_create.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
        L.cbc_gpu_group_gather.restype = ctypes.c_int
        L.cbc_gpu_group_gather.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
        L.cbc_gpu_group_destroy.argtypes = [ctypes.c_void_p]
        L.cbc_gpu_group_last_error.restype = ctypes.c_char_p
        L.cbc_gpu_group_last_error.argtypes = [ctypes.c_void_p]
        L.cbc_gpu_stash_reset.restype = ctypes.c_int
        L.cbc_gpu_stash_reset.argtypes = [ctypes.c_void_p]
        L.cbc_gpu_stash_bytes.restype = ctypes.c_uint64
        L.cbc_gpu_stash_bytes.argtypes = [ctypes.c_void_p]
        L.cbc_gpu_stash_fetch.restype = ctypes.c_int
        L.cbc_gpu_stash_fetch.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
        L.cbc_stream_read_length.restype = ctypes.c_uint32
        L.cbc_stream_read_length.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
        L.cbc_gpu_tokenise_sam.restype = ctypes.c_int
        L.cbc_gpu_tokenise_sam.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(TokResult)]
        L.cbc_gpu_tokenise_fetch.restype = ctypes.c_int
        L.cbc_gpu_tokenise_fetch.argtypes = [ctypes.c_void_p, ctypes.POINTER(TokResult), ctypes.c_void_p, ctypes.c_void_p]
        L.cbc_gpu_tokenise_free.argtypes = [ctypes.c_void_p, ctypes.POINTER(TokResult)]
        L.cbc_gpu_encode_blocks_tokenised.restype = ctypes.c_int
        L.cbc_gpu_encode_blocks_tokenised.argtypes = [ctypes.c_void_p, ctypes.POINTER(TokResult), ctypes.POINTER(HostBatch), ctypes.c_void_p,
                                                      ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
        L.cbc_gpu_upload_reference_2bit.restype = ctypes.c_int
        L.cbc_gpu_upload_reference_2bit.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64]
        L.cbc_gpu_encode_blocks_2bit.restype = ctypes.c_int
        L.cbc_gpu_encode_blocks_2bit.argtypes = [ctypes.c_void_p, ctypes.POINTER(HostBatch), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                                 ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
        L.cbc_gpu_decode_blocks_2bit.restype = ctypes.c_int
        L.cbc_gpu_decode_blocks_2bit.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32,
                                                 ctypes.POINTER(host.LdsCaps), ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
                                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p]
        L.cbc_gpu_long_plan_output.restype = ctypes.c_uint64
        L.cbc_gpu_long_plan_output.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32]
        L.cbc_gpu_long_lds_bytes.restype = ctypes.c_uint32
        L.cbc_gpu_long_lds_bytes.argtypes = [ctypes.POINTER(host.LdsCaps)]
        L.cbc_gpu_long_encode_blocks_device.restype = ctypes.c_int
        L.cbc_gpu_long_encode_blocks_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(DeviceBatch), ctypes.c_void_p]
        L.cbc_gpu_long_decode_blocks_device.restype = ctypes.c_int
        L.cbc_gpu_long_decode_blocks_device.argtypes = [ctypes.c_void_p, ctypes.POINTER(DecDeviceBatch), ctypes.c_void_p]
        L.cbc_gpu_long_encode_blocks.restype = ctypes.c_int
        L.cbc_gpu_long_encode_blocks.argtypes = L.cbc_gpu_encode_blocks.argtypes
        L.cbc_gpu_long_decode_blocks.restype = ctypes.c_int
        L.cbc_gpu_long_decode_blocks.argtypes = L.cbc_gpu_decode_blocks.argtypes
        L.cbc_gpu_last_kernel_variant.restype = ctypes.c_int
        L.cbc_gpu_last_kernel_variant.argtypes = [ctypes.c_void_p]
        L.cbc_gpu_synchronize.restype = ctypes.c_int
        L.cbc_gpu_synchronize.argtypes = [ctypes.c_void_p]
        L.cbc_gpu_upload_reference_parts.restype = ctypes.c_int
        L.cbc_gpu_upload_reference_parts.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
        L.cbc_gpu_last_e2e.restype = ctypes.c_int
        L.cbc_gpu_last_e2e.argtypes = [ctypes.c_void_p, ctypes.POINTER(E2ETimes)]
        L.cbc_gpu_host_register.restype = ctypes.c_int
        L.cbc_gpu_host_register.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
        L.cbc_gpu_host_unregister.restype = ctypes.c_int
        L.cbc_gpu_host_unregister.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.cbc_gpu_checksum_device.restype = ctypes.c_int
        L.cbc_gpu_checksum_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
        L.cbc_gpu_decode_region.restype = ctypes.c_int
        L.cbc_gpu_decode_region.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32,
                                            ctypes.POINTER(host.LdsCaps), ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64,
                                            ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64),
                                            ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p]
        L.cbc_gpu_decode_blocks_span.restype = ctypes.c_int
        L.cbc_gpu_decode_blocks_span.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32,
                                                 ctypes.POINTER(host.LdsCaps), ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64,
                                                 ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
        L.cbc_gpu_last_region_ms.restype = ctypes.c_int
        L.cbc_gpu_last_region_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float),
                                             ctypes.POINTER(ctypes.c_float)]
        L.cbc_gpu_decode_sam.restype = ctypes.c_int
        L.cbc_gpu_decode_sam.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32,
                                         ctypes.POINTER(host.LdsCaps), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(SamRegion),
                                         ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64),
                                         ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p]
        L.cbc_gpu_last_sam_ms.restype = ctypes.c_int
        L.cbc_gpu_last_sam_ms.argtypes = L.cbc_gpu_last_region_ms.argtypes
        L.cbc_gpu_decode_sam_cigar.restype = ctypes.c_int
        L.cbc_gpu_decode_sam_cigar.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32,
                                               ctypes.POINTER(host.LdsCaps), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(SamRegion),
                                               ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64,
                                               ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p]
        L.cbc_gpu_last_sam_cigar_ms.restype = ctypes.c_int
        L.cbc_gpu_last_sam_cigar_ms.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_float)] * 4
        L.cbc_gpu_decode_depth.restype = ctypes.c_int
        L.cbc_gpu_decode_depth.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32,
                                           ctypes.POINTER(host.LdsCaps), ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint32,
                                           ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                           ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
                                           ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p]
        L.cbc_gpu_decode_targets.restype = ctypes.c_int
        L.cbc_gpu_decode_targets.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32,
                                             ctypes.POINTER(host.LdsCaps), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(GpuTargets),
                                             ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64,
                                             ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64),
                                             ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p]
        L.cbc_gpu_last_targets_ms.restype = ctypes.c_int
        L.cbc_gpu_last_targets_ms.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_float)] * 4
        L.cbc_gpu_decode_coverage.restype = ctypes.c_int
        L.cbc_gpu_decode_coverage.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32,
                                              ctypes.POINTER(host.LdsCaps), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                              ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(GpuTargets),
                                              ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                                              ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64),
                                              ctypes.c_void_p]
        L.cbc_gpu_decode_coverage_ext.restype = ctypes.c_int
        L.cbc_gpu_decode_coverage_ext.argtypes = L.cbc_gpu_decode_coverage.argtypes + [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p,
                                                                                       ctypes.c_void_p]
        L.cbc_gpu_last_coverage_ext_ms.restype = ctypes.c_int
        L.cbc_gpu_last_coverage_ext_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
        L.cbc_gpu_decode_coverage_quant.restype = ctypes.c_int
        L.cbc_gpu_decode_coverage_quant.argtypes = L.cbc_gpu_decode_coverage_ext.argtypes + [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
        L.cbc_gpu_last_coverage_quant_ms.restype = ctypes.c_int
        L.cbc_gpu_last_coverage_quant_ms.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_float)] * 3
        L.cbc_gpu_last_coverage_ms.restype = ctypes.c_int
        L.cbc_gpu_last_coverage_ms.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_float)] * 7
        L.cbc_gpu_decode_depth_hist.restype = ctypes.c_int
        L.cbc_gpu_decode_depth_hist.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32,
                                                ctypes.POINTER(host.LdsCaps), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(GpuTargets),
                                                ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32),
                                                ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p]
        L.cbc_gpu_last_hist_ms.restype = ctypes.c_int
        L.cbc_gpu_last_hist_ms.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_float)] * 5
        L.cbc_gpu_decode_stats.restype = ctypes.c_int
        L.cbc_gpu_decode_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32,
                                           ctypes.POINTER(host.LdsCaps), ctypes.c_void_p, ctypes.POINTER(GpuTargets), ctypes.c_uint32,
                                           ctypes.POINTER(host.GpuStats), ctypes.c_void_p]
        L.cbc_gpu_last_stats_ms.restype = ctypes.c_int
        L.cbc_gpu_last_stats_ms.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_float)] * 2
        L.cbc_gpu_decode_stats_aln.restype = ctypes.c_int
        L.cbc_gpu_decode_stats_aln.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32,
                                               ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.cbc_gpu_last_stats_aln_ms.restype = ctypes.c_int
        L.cbc_gpu_last_stats_aln_ms.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_float)] * 3
        L.cbc_gpu_last_depth_ms.restype = ctypes.c_int
        L.cbc_gpu_last_depth_ms.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_float)] * 4
        L.cbc_gpu_decode_pileup.restype = ctypes.c_int
        L.cbc_gpu_decode_pileup.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32,
                                            ctypes.POINTER(host.LdsCaps), ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint32,
                                            ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                            ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64),
                                            ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p]
        L.cbc_gpu_decode_pileup_ext.restype = ctypes.c_int
        L.cbc_gpu_decode_pileup_ext.argtypes = L.cbc_gpu_decode_pileup.argtypes[:15] + [ctypes.c_uint32, ctypes.c_uint32] + \
                                                L.cbc_gpu_decode_pileup.argtypes[15:]
        L.cbc_gpu_set_depth_skip_deletions.restype = ctypes.c_int
        L.cbc_gpu_set_depth_skip_deletions.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
        L.cbc_gpu_last_pileup_ms.restype = ctypes.c_int
        L.cbc_gpu_last_pileup_ms.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_float)] * 4
        L.cbc_gpu_decode_consensus.restype = ctypes.c_int
        L.cbc_gpu_decode_consensus.argtypes = L.cbc_gpu_decode_pileup.argtypes[:13] + \
            [ctypes.c_uint32, ctypes.POINTER(host.ConsensusOpts), ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64,
             ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(host.ConsensusCounts), ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p]
        L.cbc_gpu_last_consensus_ms.restype = ctypes.c_int
        L.cbc_gpu_last_consensus_ms.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_float)] * 4
        L.cbc_gpu_decode_blocks_edits.restype = ctypes.c_int
        L.cbc_gpu_decode_blocks_edits.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32,
                                                  ctypes.POINTER(host.LdsCaps), ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p,
                                                  ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p,
                                                  ctypes.c_void_p]
        if L.cbc_gpu_abi_version() != 1:
            raise CbcGpuError("libcbc_gpu.so ABI version mismatch")
        _lib = L
    return _lib


EXPORTS = ["cbc_gpu_abi_version", "cbc_gpu_device_count", "cbc_gpu_init", "cbc_gpu_shutdown", "cbc_gpu_last_error",
           "cbc_gpu_upload_reference", "cbc_gpu_encode_blocks", "cbc_gpu_encode_blocks_device", "cbc_gpu_compact_device",
           "cbc_gpu_plan_output", "cbc_gpu_lds_bytes", "cbc_gpu_decode_blocks_device", "cbc_gpu_decode_blocks",
           "cbc_gpu_decode_lds_bytes", "cbc_gpu_last_kernel_ms", "cbc_gpu_last_kernel_variant", "cbc_gpu_synchronize",
           "cbc_gpu_encode_stream", "cbc_gpu_encode_stream_blocks", "cbc_gpu_decode_stream", "cbc_stream_read_length",
           "cbc_gpu_tokenise_sam", "cbc_gpu_tokenise_fetch", "cbc_gpu_tokenise_free", "cbc_gpu_encode_blocks_tokenised",
           "cbc_gpu_upload_reference_2bit", "cbc_gpu_encode_blocks_2bit", "cbc_gpu_decode_blocks_2bit",
           "cbc_gpu_long_plan_output", "cbc_gpu_long_lds_bytes", "cbc_gpu_long_encode_blocks_device",
           "cbc_gpu_long_decode_blocks_device", "cbc_gpu_long_encode_blocks", "cbc_gpu_long_decode_blocks",
           "cbc_gpu_checksum_device", "cbc_gpu_upload_reference_parts", "cbc_gpu_last_e2e", "cbc_gpu_host_register",
           "cbc_gpu_host_unregister", "cbc_gpu_plan_output_caps", "cbc_gpu_reserve_encode",
           "cbc_gpu_decode_stream_blocks", "cbc_gpu_group_create", "cbc_gpu_group_gather", "cbc_gpu_group_destroy", "cbc_gpu_group_last_error",
           "cbc_gpu_stash_reset", "cbc_gpu_stash_bytes", "cbc_gpu_stash_fetch", "cbc_gpu_decode_region",
           "cbc_gpu_decode_blocks_span", "cbc_gpu_last_region_ms", "cbc_gpu_decode_sam", "cbc_gpu_last_sam_ms",
           "cbc_gpu_decode_depth", "cbc_gpu_last_depth_ms", "cbc_gpu_decode_targets", "cbc_gpu_last_targets_ms",
           "cbc_gpu_decode_coverage", "cbc_gpu_last_coverage_ms", "cbc_gpu_decode_depth_hist", "cbc_gpu_last_hist_ms", "cbc_gpu_decode_stats",
           "cbc_gpu_last_stats_ms", "cbc_gpu_decode_stats_aln", "cbc_gpu_last_stats_aln_ms",
           "cbc_gpu_decode_coverage_ext", "cbc_gpu_last_coverage_ext_ms",
           "cbc_gpu_decode_coverage_quant", "cbc_gpu_last_coverage_quant_ms",
           "cbc_gpu_decode_pileup", "cbc_gpu_decode_pileup_ext", "cbc_gpu_last_pileup_ms", "cbc_gpu_decode_blocks_edits",
           "cbc_gpu_decode_sam_cigar", "cbc_gpu_last_sam_cigar_ms", "cbc_gpu_set_depth_skip_deletions",
           "cbc_gpu_decode_consensus", "cbc_gpu_last_consensus_ms"]

EDITS_PER_READ = 16           # CBC_EDITS_PER_READ: the library's default arena size, entries per read of a block

_ALT_FRAC = re.compile(r"[0-9]+(\.[0-9]{1,6})?\Z")


def alt_frac_ppm(text) -> int:
    """The value of `cbc -x --pileup --min-alt-frac F` in parts per million, by digit arithmetic: F is [0-9]+(\\.[0-9]{1,6})? with
    a value in (0, 1] -- "0.000001" gives 1, "1" and "1.0" give 1 000 000.  ValueError for exactly the strings the CLI refuses."""
    if not isinstance(text, str) or not _ALT_FRAC.match(text):
        raise ValueError("min_alt_frac wants a decimal fraction in (0, 1] with at most six decimals, not %r" % (text,))
    whole, _, frac = text.partition(".")
    ppm = int(whole) * 1_000_000 + int((frac + "000000")[:6])
    if not 1 <= ppm <= 1_000_000:
        raise ValueError("min_alt_frac wants a decimal fraction in (0, 1] with at most six decimals, not %r" % (text,))
    return ppm


class Encoder:
    """One context per device (mirrors the lifetime of the reference's compress() call)."""

    def __init__(self, device=0):
        L = lib()
        if L.cbc_gpu_device_count() <= 0:
            raise CbcGpuError("no HIP device visible: the cbc hot path has no CPU fallback")
        self._ctx = ctypes.c_void_p()
        rc = L.cbc_gpu_init(device, ctypes.byref(self._ctx))
        if rc != 0:
            raise CbcGpuError("cbc_gpu_init(%d) failed: %d" % (device, rc))
        self.device = device

    def _check(self, rc, what):
        if rc != 0:
            msg = lib().cbc_gpu_last_error(self._ctx)
            raise CbcGpuError("%s failed (%d): %s" % (what, rc, msg.decode(errors="replace") if msg else ""))

    # ---- what the decode_* wrappers below share ----

    @contextlib.contextmanager
    def skip_deletions(self, max_edits_per_read=EDITS_PER_READ, on=True):
        """`with enc.skip_deletions():` -- every depth call made inside (decode_depth, decode_targets(output="depth"),
        decode_coverage, decode_coverage_quant, decode_depth_hist; not decode_pileup) counts ALIGNED bases only: the bases a read
        deletes do not count, as in samtools depth without -J, mosdepth and bedtools genomecov -split
        (cbc_gpu_set_depth_skip_deletions).  The reads counted, and the `reads` of decode_coverage(count_reads=True), keep their
        span meaning: a read whose only bases inside a query are deleted still overlaps it (samtools bedcov -c counts it too).
        The calls run the decoder that keeps the alignment, with max_edits_per_read (1..510) arena entries per read as for
        decode_pileup: a block that needs more fails with status 9.  The encoder is back at the span depth afterwards, whatever
        happened.  decode_depth, decode_targets and decode_depth_hist take the same as keywords; decode_coverage and
        decode_coverage_quant, whose parameter lists are fixed, are used inside this block.  on=False: nothing is set."""
        if not on:
            yield
            return
        epr = int(max_edits_per_read)
        if not 1 <= epr <= 510:
            raise ValueError("max_edits_per_read is in 1..510")
        self._check(lib().cbc_gpu_set_depth_skip_deletions(self._ctx, epr), "cbc_gpu_set_depth_skip_deletions")
        try:
            yield
        finally:
            lib().cbc_gpu_set_depth_skip_deletions(self._ctx, 0)

    def _check_blocks(self, rc, what, results):
        """_check, except that with results=True a failed block (rc -4) passes: the caller hands out the per-block results."""
        if rc != 0 and not (results and rc == -4):
            self._check(rc, what)

    @staticmethod
    def _plan_args(plan):
        """(caps, payloads, names, name offsets) of a plan as the C calls take them; the caller keeps them alive over the call."""
        return (host.LdsCaps(plan.cap_pos, plan.cap_var), np.ascontiguousarray(plan.payloads), np.ascontiguousarray(plan.names),
                np.ascontiguousarray(plan.contig_name_off, dtype=np.uint32))

    @staticmethod
    def _gather(plan, sel, biv=None):
        """(descriptors, window starts, contigs) of the blocks `sel`, a slice or an array of block indices, as contiguous arrays;
        biv: the rows of a target set's block_iv that go with them, appended as a fourth."""
        if not isinstance(sel, slice):
            sel = np.ascontiguousarray(sel).astype(np.int64)
        out = (np.ascontiguousarray(plan.blocks[sel]), np.ascontiguousarray(plan.window_start[sel], dtype=np.uint64),
               np.ascontiguousarray(plan.block_contig[sel], dtype=np.uint32))
        return out if biv is None else out + (np.ascontiguousarray(biv, dtype=np.uint32),)

    @staticmethod
    def _cat(allres):
        return np.concatenate(allres) if allres else np.zeros(0, dtype=host.RESULT_DTYPE)

    def _last_ms(self, name, n, at=None, must=False):
        """The n floats of lib().<name> (a cbc_gpu_last_*_ms) as a tuple, None when the call reports none (must=True: raise).
        at: where in the n floats each pointer argument starts (default: one argument per float)."""
        buf = (ctypes.c_float * n)()
        rc = getattr(lib(), name)(self._ctx, *[ctypes.cast(ctypes.byref(buf, 4 * i), ctypes.POINTER(ctypes.c_float))
                                               for i in (at or range(n))])
        if must:
            self._check(rc, name)
        return tuple(buf) if rc == 0 else None

    def _add_ms(self, attr, name, n, at=None, must=False):
        """Adds the kernel milliseconds of the last call (_last_ms) to the tuple in self.<attr>, which starts as None."""
        ms, old = self._last_ms(name, n, at, must), getattr(self, attr)
        if ms is not None:
            setattr(self, attr, ms if old is None else tuple(a + b for a, b in zip(old, ms)))

    def upload_reference(self, ref: np.ndarray):
        ref = np.ascontiguousarray(ref, dtype=np.uint8)
        self._check(lib().cbc_gpu_upload_reference(self._ctx, ref.ctypes.data, ref.size), "cbc_gpu_upload_reference")

    def tokenise_sam(self, sam: bytes, fasta: bytes, fetch=False, **kw):
        """SAM text -> packed batch with the tokenising done on the device (cbc_gpu_tokenise_sam + the host's serial half,
        cbc_pack_from_device_tokens).  Returns (PackedBatch, TokResult): with fetch=False the batch carries no bases / tokens
        (they stay on the device for encode_blocks_tokenised); fetch=True copies them back (parity tests).  Raises
        host.CbcInputError with the offending line when the text is malformed or needs the host packer."""
        tr = TokResult()
        rc = lib().cbc_gpu_tokenise_sam(self._ctx, sam, len(sam), host.sam_body_offset(sam), ctypes.byref(tr))
        self._check(rc, "cbc_gpu_tokenise_sam")
        if tr.status:
            st, line = int(tr.status), int(tr.bad_line)
            lib().cbc_gpu_tokenise_free(self._ctx, ctypes.byref(tr))
            raise host.CbcInputError("device tokeniser: line %d: %s (status %d)" % (line + 1, TOK_STATUS.get(st, "?"), st))
        n, nc = int(tr.n_recs), int(tr.n_changes)
        def view(ptr, count, dtype):
            if count == 0:
                return np.zeros(0, dtype=dtype)
            return np.frombuffer((ctypes.c_uint8 * (count * np.dtype(dtype).itemsize)).from_address(ptr), dtype=dtype)
        summ = view(tr.summaries, n, host.SUMMARY_DTYPE); chg = view(tr.rname_change, n, np.uint8)
        coff = view(tr.change_name_off, nc, np.uint64); clen = view(tr.change_name_len, nc, np.uint32)
        seq = tok = None
        if fetch:
            seq = np.zeros(int(tr.seq_bytes) + 8, dtype=np.uint8); tok = np.zeros(max(int(tr.n_tok), 1), dtype=np.uint32)
            self._check(lib().cbc_gpu_tokenise_fetch(self._ctx, ctypes.byref(tr), seq.ctypes.data, tok.ctypes.data), "cbc_gpu_tokenise_fetch")
        try:
            pb = host.pack_from_device_tokens(sam, fasta, summ, chg, coff, clen, int(tr.n_unmapped), seq=seq, tok=tok,
                                              seq_bytes=int(tr.seq_bytes), n_tok=int(tr.n_tok), **kw)
        except Exception:
            lib().cbc_gpu_tokenise_free(self._ctx, ctypes.byref(tr))
            raise
        return pb, tr

    def tokenise_free(self, tr):
        lib().cbc_gpu_tokenise_free(self._ctx, ctypes.byref(tr))

    def encode_blocks_tokenised(self, pb, tr):
        """cbc_gpu_encode_blocks over the tokeniser's device-resident bases and tokens."""
        nb = pb.n_blocks
        blocks = pb.blocks.copy()
        hb = HostBatch(pb.recs.ctypes.data, pb.n_recs, None, int(tr.seq_bytes) + 8, None, int(tr.n_tok),
                       pb.names.ctypes.data, len(pb.names), blocks.ctypes.data, nb, host.LdsCaps(pb.cap_pos, pb.cap_var))
        # the planner wants the tokens: worst case from the summaries instead (3 bytes per symbol, 16 per record + 2 per var symbol)
        total = int(4096 * nb + 3 * (16 * pb.n_recs + 2 * int(tr.n_tok)) + 256 * nb + 8 * int(tr.n_tok))
        out = np.zeros(total, dtype=np.uint8)
        offs = np.zeros(nb + 1, dtype=np.uint64)
        res = np.zeros(nb, dtype=host.RESULT_DTYPE)
        rc = lib().cbc_gpu_encode_blocks_tokenised(self._ctx, ctypes.byref(tr), ctypes.byref(hb), out.ctypes.data, out.size,
                                                   offs.ctypes.data, res.ctypes.data)
        if rc != 0 and rc != -4:
            self._check(rc, "cbc_gpu_encode_blocks_tokenised")
        return [out[int(offs[b]):int(offs[b + 1])].tobytes() for b in range(nb)], res, offs, out[:int(offs[nb])]

    def upload_reference_2bit(self, codes: np.ndarray, runs: np.ndarray, n_bases: int):
        """The reference over PCIe at 2 bits per base (host.pack_2bit), expanded on the device."""
        codes = np.ascontiguousarray(codes, dtype=np.uint32)
        runs = np.ascontiguousarray(runs, dtype=host.RUN_DTYPE)
        self._check(lib().cbc_gpu_upload_reference_2bit(self._ctx, codes.ctypes.data, n_bases, runs.ctypes.data if len(runs) else None,
                                                        len(runs)), "cbc_gpu_upload_reference_2bit")

    def encode_blocks_2bit(self, pb: "host.PackedBatch", codes: np.ndarray, runs: np.ndarray, want_payload_list=True):
        """cbc_gpu_encode_blocks with the batch's bases given in 2-bit transport form (host.pack_2bit(pb.seq))."""
        nb = pb.n_blocks
        hb, blocks = self._host_batch(pb)
        hb.seq = None
        total = lib().cbc_gpu_plan_output_caps(blocks.ctypes.data, nb, ctypes.byref(hb.caps))
        out = np.zeros(int(total), dtype=np.uint8)
        offs = np.zeros(nb + 1, dtype=np.uint64)
        res = np.zeros(nb, dtype=host.RESULT_DTYPE)
        codes = np.ascontiguousarray(codes, dtype=np.uint32); runs = np.ascontiguousarray(runs, dtype=host.RUN_DTYPE)
        rc = lib().cbc_gpu_encode_blocks_2bit(self._ctx, ctypes.byref(hb), codes.ctypes.data, runs.ctypes.data if len(runs) else None, len(runs),
                                              out.ctypes.data, out.size, offs.ctypes.data, res.ctypes.data)
        if rc != 0 and rc != -4:
            self._check(rc, "cbc_gpu_encode_blocks_2bit")
        return ([out[int(offs[b]):int(offs[b + 1])].tobytes() for b in range(nb)] if want_payload_list else None), res, offs, out[:int(offs[nb])]

    def decode_blocks_2bit(self, plan: "host.UnpackPlan", stride=None):
        """cbc_gpu_decode_blocks with the bases coming back as 2-bit rows.  Returns (recs, bases[n, stride] rebuilt on the
        host, results, bytes that crossed PCIe for the bases)."""
        nb = plan.n_blocks
        stride = stride or (plan.seq_stride + 15) // 16 * 16
        blocks = plan.blocks.copy()
        blocks["seq_stride"] = stride
        blocks["seq_base"] = blocks["rec_base"] * stride
        recs = np.zeros(plan.n_recs, dtype=host.REC_DTYPE)
        row_words = stride // 16
        codes = np.zeros(plan.n_recs * row_words + 4, dtype=np.uint32)
        n_exc = ctypes.c_uint64(0)
        res = np.zeros(nb, dtype=host.RESULT_DTYPE)
        caps = host.LdsCaps(plan.cap_pos, plan.cap_var)
        pay = np.ascontiguousarray(plan.payloads)
        need = 0
        # more non-ACGT bases than the guess: the call reports how many and copies none, so the whole decode runs again
        # once with room for all of them (a second full decode, not a fetch: rare, batches of over 4 N per read)
        for _ in range(2):
            cap = max(1024, plan.n_recs * 4, need)
            ei = np.zeros(cap, dtype=np.uint64); ev = np.zeros(cap, dtype=np.uint8)
            rc = lib().cbc_gpu_decode_blocks_2bit(self._ctx, pay.ctypes.data, pay.size, blocks.ctypes.data, nb, ctypes.byref(caps),
                                                  recs.ctypes.data, plan.n_recs, codes.ctypes.data, ei.ctypes.data, ev.ctypes.data, cap,
                                                  ctypes.byref(n_exc), res.ctypes.data)
            need = int(n_exc.value)
            if not (rc == -1 and need > cap):
                break
        if rc != 0 and rc != -4:
            self._check(rc, "cbc_gpu_decode_blocks_2bit")
        lut = np.frombuffer(b"ACGT", dtype=np.uint8)
        c = codes[:plan.n_recs * row_words]
        bases = lut[(c[:, None] >> (2 * np.arange(16, dtype=np.uint32))[None, :]) & 3].reshape(plan.n_recs, stride)
        k = int(n_exc.value)
        if k:
            bases.reshape(-1)[ei[:k].astype(np.int64)] = ev[:k]
        return recs, bases, res, c.nbytes + 9 * k

    def encode_blocks(self, pb: "host.PackedBatch", which=None, want_payload_list=True):
        """Host-buffer path.  Returns (list of payload bytes per block, results array, out_offsets, flat payload bytes).
        which: optional list of block indices (a rank's share of the batch); the descriptors carry absolute bases into the
        batch's arrays, so any subset is a batch of its own."""
        blocks = pb.blocks.copy() if which is None else np.ascontiguousarray(pb.blocks[list(which)])
        nb = len(blocks)
        hb = HostBatch(pb.recs.ctypes.data, pb.n_recs, pb.seq.ctypes.data, len(pb.seq), pb.tok.ctypes.data, pb.n_tok,
                       pb.names.ctypes.data, len(pb.names), blocks.ctypes.data, nb, host.LdsCaps(pb.cap_pos, pb.cap_var))
        total = lib().cbc_gpu_plan_output_caps(blocks.ctypes.data, nb, ctypes.byref(hb.caps))
        out = np.zeros(int(total), dtype=np.uint8)
        offs = np.zeros(nb + 1, dtype=np.uint64)
        res = np.zeros(nb, dtype=host.RESULT_DTYPE)
        rc = lib().cbc_gpu_encode_blocks(self._ctx, ctypes.byref(hb), out.ctypes.data, out.size, offs.ctypes.data,
                                         res.ctypes.data)
        if rc != 0 and rc != -4:
            self._check(rc, "cbc_gpu_encode_blocks")
        payloads = [out[int(offs[b]):int(offs[b + 1])].tobytes() for b in range(nb)] if want_payload_list else None
        return payloads, res, offs, out[:int(offs[nb])]

    def decode_blocks(self, plan: "host.UnpackPlan"):
        """Host-buffer decode of every block of an UnpackPlan.  Returns (recs, seq, results)."""
        nb = plan.n_blocks
        blocks = plan.blocks.copy()
        recs = np.zeros(plan.n_recs, dtype=host.REC_DTYPE)
        seq = np.zeros(plan.n_recs * plan.seq_stride + 8, dtype=np.uint8)
        res = np.zeros(nb, dtype=host.RESULT_DTYPE)
        caps = host.LdsCaps(plan.cap_pos, plan.cap_var)
        pay = np.ascontiguousarray(plan.payloads)
        rc = lib().cbc_gpu_decode_blocks(self._ctx, pay.ctypes.data, pay.size, blocks.ctypes.data, nb, ctypes.byref(caps),
                                         recs.ctypes.data, plan.n_recs, seq.ctypes.data, seq.size, res.ctypes.data)
        if rc != 0 and rc != -4:
            self._check(rc, "cbc_gpu_decode_blocks")
        return recs, seq, res

    def decode_blocks_span(self, plan: "host.UnpackPlan", smax):
        """decode_blocks with every read's span in recs["tok_off"] (cbc_gpu_decode_blocks_span).  Returns (recs, seq, results)."""
        nb = plan.n_blocks
        blocks = plan.blocks.copy()
        recs = np.zeros(plan.n_recs, dtype=host.REC_DTYPE)
        seq = np.zeros(plan.n_recs * plan.seq_stride + 8, dtype=np.uint8)
        res = np.zeros(nb, dtype=host.RESULT_DTYPE)
        caps = host.LdsCaps(plan.cap_pos, plan.cap_var)
        pay = np.ascontiguousarray(plan.payloads)
        rc = lib().cbc_gpu_decode_blocks_span(self._ctx, pay.ctypes.data, pay.size, blocks.ctypes.data, nb, ctypes.byref(caps), smax,
                                              recs.ctypes.data, plan.n_recs, seq.ctypes.data, seq.size, res.ctypes.data)
        if rc != 0 and rc != -4:
            self._check(rc, "cbc_gpu_decode_blocks_span")
        return recs, seq, res

    def decode_region(self, plan: "host.UnpackPlan", region, results=False):
        """The reads of `region` (NAME, NAME:BEG or NAME:BEG-END) as the text `cbc -x` writes for them: the index selects the
        blocks (UnpackPlan.region), the device decodes those, filters and assembles the text (cbc_gpu_decode_region).  The
        reference must have been uploaded (upload_reference(plan.ref)).  With results=True returns (text, n_selected,
        selection, per-block decode results)."""
        sel = plan.region(region)
        nb = sel.b1 - sel.b0
        res = np.zeros(max(nb, 1), dtype=host.RESULT_DTYPE)
        if nb == 0:
            return (b"", 0, sel, res[:0]) if results else b""
        blocks, ws, _ = self._gather(plan, slice(sel.b0, sel.b1))
        cap = int(blocks["n_reads"].astype(np.uint64).sum()) * (plan.seq_stride + 1)
        text = np.zeros(max(cap, 1), dtype=np.uint8)
        nbytes, nsel = ctypes.c_uint64(), ctypes.c_uint64()
        caps, pay, _, _ = self._plan_args(plan)
        rc = lib().cbc_gpu_decode_region(self._ctx, pay.ctypes.data, pay.size, blocks.ctypes.data, nb, ctypes.byref(caps),
                                         ws.ctypes.data, sel.beg, sel.end, sel.smax, text.ctypes.data, cap,
                                         ctypes.byref(nbytes), ctypes.byref(nsel), res.ctypes.data)
        self._check_blocks(rc, "cbc_gpu_decode_region", results)
        out = text[:int(nbytes.value)].tobytes()
        return (out, int(nsel.value), sel, res[:nb]) if results else out

    def decode_sam(self, plan: "host.UnpackPlan", region=None, results=False, text_cap=None, cigar=False, edits_per_read=None):
        """The reads of the container, or with `region` (NAME, NAME:BEG or NAME:BEG-END) the reads decode_region selects, as
        SAM text: plan.sam_header() + one alignment line per read, assembled on the device (cbc_gpu_decode_sam).  The
        reference must have been uploaded (upload_reference(plan.ref)).  An empty selection gives the header alone and runs
        nothing on the device.  With results=True returns (text, n_reads, selection or None, per-block decode results).
        text_cap: size of the buffer for the lines (default: plan.sam_text_cap of the blocks).
        cigar=True: every line carries CIGAR, NM:i and MD:Z in the codec's view of the alignment (cbc_gpu_decode_sam_cigar: an
        insertion run is written in front of a deletion at the same place, an inserted run at a read's end is S, a mismatch is
        a plain byte compare with the uploaded reference); edits_per_read sizes the arena as for decode_pileup (a block that
        needs more fails, the error names the option).  Its default buffer is plan.sam_text_cap plus 64 bytes per read, and the
        call is repeated once at the text's own size when that is too small; plan.sam_cigar_text_cap always suffices."""
        if not cigar and edits_per_read is not None:
            raise ValueError("edits_per_read applies to decode_sam(cigar=True)")
        hdr = plan.sam_header()
        epr = 0 if edits_per_read is None else int(edits_per_read)
        if edits_per_read is not None and not 1 <= epr <= 510:
            raise ValueError("edits_per_read in 1..510")
        sel = plan.region(region) if region is not None else None
        b0, b1 = (sel.b0, sel.b1) if sel is not None else (0, plan.n_blocks)
        nb = b1 - b0
        res = np.zeros(max(nb, 1), dtype=host.RESULT_DTYPE)
        if cigar:
            self.last_sam_text_bytes = 0
        if nb == 0:
            return (hdr, 0, sel, res[:0]) if results else hdr
        blocks, ws, bc = self._gather(plan, slice(b0, b1))
        caps, pay, names, noff = self._plan_args(plan)
        # the plain text starts at its bound, so nothing is ever repeated for it; with CIGAR the first buffer is a guess
        bound = cap = plan.sam_text_cap(b0, b1)
        fn, extra = "cbc_gpu_decode_sam", ()
        if cigar:
            bound = plan.sam_cigar_text_cap(b0, b1, epr)
            cap = min(cap + 64 * int(plan.blocks[b0:b1]["n_reads"].sum()), bound)
            # the container's span bound, the one every selection carries
            fn, extra = "cbc_gpu_decode_sam_cigar", (plan.max_read_len + plan.read_length - 1, epr)
        if text_cap is not None:
            cap = int(text_cap)
        nbytes, nrd = ctypes.c_uint64(), ctypes.c_uint64()
        rg = SamRegion(sel.beg, sel.end, sel.smax, 0) if sel is not None else None
        for _ in range(2):
            text = np.zeros(max(cap, 1), dtype=np.uint8)
            rc = getattr(lib(), fn)(self._ctx, pay.ctypes.data, pay.size, blocks.ctypes.data, nb, ctypes.byref(caps), ws.ctypes.data,
                                    bc.ctypes.data, names.ctypes.data, names.size, noff.ctypes.data, plan.n_contigs,
                                    ctypes.byref(rg) if rg is not None else None, *extra, text.ctypes.data, cap,
                                    ctypes.byref(nbytes), ctypes.byref(nrd), res.ctypes.data)
            if not (text_cap is None and rc == -1 and cap < int(nbytes.value) <= bound):
                break
            cap = int(nbytes.value)                           # the text's own size
        self.last_sam_text_bytes = int(nbytes.value)
        self._check_blocks(rc, fn, results)
        out = hdr + text[:int(nbytes.value)].tobytes()
        return (out, int(nrd.value), sel, res[:nb]) if results else out

    def _decode_windows(self, plan, region, results, text_cap, fn, rest, cap_of, bytes_attr, ms_attr, ms_fn):
        """What decode_depth and decode_pileup share: one call of lib().<fn> per selection -- the region's, or every contig's that
        has blocks -- with rest(sel), the arguments between the window's end and the text buffer; the buffer is cap_of(sel) or
        text_cap bytes and the call is never repeated.  The texts' bytes are summed in self.<bytes_attr>, the kernel times of
        lib().<ms_fn> in self.<ms_attr>.  Returns (text, n_runs or n_lines, n_reads_kept, per-block results), or the text."""
        sels = [plan.region(region)] if region is not None else [plan.contig_blocks(c) for c in range(plan.n_contigs)]
        out, n_out, n_kept, allres = [], 0, 0, []
        setattr(self, bytes_attr, 0)
        setattr(self, ms_attr, None)
        caps, pay, _, _ = self._plan_args(plan)
        for sel in sels:
            nb = sel.b1 - sel.b0
            if nb == 0:
                continue
            blocks, ws, _ = self._gather(plan, slice(sel.b0, sel.b1))
            off = int(plan.contig_name_off[sel.contig])
            name = plan.names[off:].tobytes().split(b"\0", 1)[0]
            cap = cap_of(sel) if text_cap is None else int(text_cap)
            text = np.zeros(max(cap, 1), dtype=np.uint8)
            res = np.zeros(nb, dtype=host.RESULT_DTYPE)
            nbytes, no, nk = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
            rc = getattr(lib(), fn)(self._ctx, pay.ctypes.data, pay.size, blocks.ctypes.data, nb, ctypes.byref(caps), ws.ctypes.data,
                                    name, len(name), sel.beg, sel.end, *rest(sel), text.ctypes.data, cap, ctypes.byref(nbytes),
                                    ctypes.byref(no), ctypes.byref(nk), res.ctypes.data)
            setattr(self, bytes_attr, getattr(self, bytes_attr) + int(nbytes.value))
            self._check_blocks(rc, fn, results)
            self._add_ms(ms_attr, ms_fn, 4, must=True)
            out.append(text[:int(nbytes.value)].tobytes())
            n_out += int(no.value); n_kept += int(nk.value); allres.append(res)
        text = b"".join(out)
        if results:
            return text, n_out, n_kept, self._cat(allres)
        return text

    def decode_depth(self, plan: "host.UnpackPlan", region=None, exclude_flags=0, results=False, text_cap=None, smax=None,
                     skip_deletions=False, max_edits_per_read=EDITS_PER_READ):
        """Coverage of the container's reads as bedGraph bytes (cbc_gpu_decode_depth): per maximal run of equal non-zero
        depth `NAME\\tstart\\tend\\tdepth\\n`, 0-based half-open.  A read covers POS .. POS + span - 1, the bases it deletes
        included (a span coverage); reads with FLAG & exclude_flags != 0 are left out.  region=None: every contig that has
        blocks, as a whole, in the order of the contig table; otherwise (NAME, NAME:BEG or NAME:BEG-END) only the window, reads
        clipped to it.  The reference must have been uploaded (upload_reference(plan.ref)).  A selection without blocks gives
        b"" and runs nothing on the device.  With results=True returns (text, n_runs, n_reads_kept, per-block decode results
        of the blocks used) and lets a failed block pass (it marks nothing); text_cap: size of the buffer of one call (default:
        plan.depth_text_cap of its blocks); smax: the span bound the decode checks (default: the selection's).
        skip_deletions=True: the depth at a position is the kept reads with an ALIGNED base there -- the bases a read deletes do
        not count, as in samtools depth without -J, mosdepth and bedtools genomecov -split; inserted bases and soft clips change
        nothing, and n_reads_kept keeps its span meaning.  The calls then run the decoder that keeps the alignment, with
        max_edits_per_read (1..510) arena entries per read as for decode_pileup (a block that needs more fails with status 9),
        and text_cap defaults to plan.depth_skipdel_text_cap.  False (the default): every byte as without the keyword."""
        plan.sam_header()                                     # refuses what the text cannot carry, and long-read containers
        cap_of = (lambda sel: plan.depth_skipdel_text_cap(sel.b0, sel.b1, sel.contig, sel.beg, sel.end,
                                                          sel.smax if smax is None else int(smax))) if skip_deletions else \
                 (lambda sel: plan.depth_text_cap(sel.b0, sel.b1, sel.contig))
        with self.skip_deletions(max_edits_per_read, skip_deletions):
            return self._decode_windows(plan, region, results, text_cap, "cbc_gpu_decode_depth",
                                        lambda sel: (sel.smax if smax is None else int(smax), int(exclude_flags)), cap_of,
                                        "last_depth_text_bytes", "_depth_ms", "cbc_gpu_last_depth_ms")

    def decode_pileup(self, plan: "host.UnpackPlan", region=None, exclude_flags=0, min_alt=1, edits_per_read=None, results=False,
                      text_cap=None, by_strand=False, min_alt_ppm=0):
        """What the container's reads show at the positions where they disagree with the reference (cbc_gpu_decode_pileup):
        per position with at least min_alt non-reference observations `NAME\\tpos1\\tref\\tdepth\\tA\\tC\\tG\\tT\\tN\\tdel\\tins\\n`,
        in the codec's view of the alignment; reads with FLAG & exclude_flags != 0 are left out.  region=None: every contig that
        has blocks, as a whole, in the order of the contig table; otherwise (NAME, NAME:BEG or NAME:BEG-END) only the window.  The
        reference must have been uploaded (upload_reference(plan.ref)).  A selection without blocks gives b"" and runs nothing
        on the device.  edits_per_read (1..510, default 16) sizes the arena the decoder keeps the alignment in: a block that
        needs more fails with status 9 (CBC_ST_EDITS).  With results=True returns (text, n_lines, n_reads_kept, per-block decode
        results of the blocks used) and lets a failed block pass (it contributes nothing); text_cap: size of the buffer of one
        call (default: plan.pileup_text_cap of its blocks and window).
        by_strand=True or min_alt_ppm > 0 (cbc_gpu_decode_pileup_ext; the defaults give the call as it was): min_alt_ppm in
        1..1 000 000 (alt_frac_ppm("0.02") = 20 000) also asks nonref * 10^6 >= min_alt_ppm * depth of a position, nonref = depth
        - count(class(ref)) + ins, in exact integers; by_strand appends `\\tA+\\tC+\\tG+\\tT+\\tN+\\tdel+\\tins+` to every line, the
        same columns counted over the kept reads with FLAG & 16 == 0 only."""
        plan.sam_header()                                     # refuses what the text cannot carry, and long-read containers
        if int(min_alt) < 1:
            raise ValueError("min_alt is 1 or more")
        if not 0 <= int(min_alt_ppm) <= 1_000_000:
            raise ValueError("min_alt_ppm is in 0..1000000")
        epr = EDITS_PER_READ if edits_per_read is None else int(edits_per_read)
        if not 1 <= epr <= 510:
            raise ValueError("edits_per_read is in 1..510")
        if by_strand or int(min_alt_ppm):
            bs = bool(by_strand)
            return self._decode_windows(plan, region, results, text_cap, "cbc_gpu_decode_pileup_ext",
                                        lambda sel: (sel.smax, int(exclude_flags), int(min_alt), epr, int(min_alt_ppm), int(bs)),
                                        lambda sel: plan.pileup_text_cap(sel.b0, sel.b1, sel.contig, sel.beg, sel.end, sel.smax, bs),
                                        "last_pileup_text_bytes", "_pileup_ms", "cbc_gpu_last_pileup_ms")
        return self._decode_windows(plan, region, results, text_cap, "cbc_gpu_decode_pileup",
                                    lambda sel: (sel.smax, int(exclude_flags), int(min_alt), epr),
                                    lambda sel: plan.pileup_text_cap(sel.b0, sel.b1, sel.contig, sel.beg, sel.end, sel.smax),
                                    "last_pileup_text_bytes", "_pileup_ms", "cbc_gpu_last_pileup_ms")

    def _summed_ms(self, attr, what):
        """The kernel milliseconds _add_ms summed in self.<attr>; CbcGpuError while no <what> has run."""
        ms = getattr(self, attr, None)
        if ms is None:
            raise CbcGpuError("no %s has run on the device" % what)
        return ms

    def last_pileup_ms(self):
        """(edits decode, zero + mark + events, scans, text) kernel milliseconds of the last decode_pileup, summed over its calls."""
        return self._summed_ms("_pileup_ms", "decode_pileup")

    def decode_consensus(self, plan: "host.UnpackPlan", region=None, exclude_flags=0, min_depth=1, call_frac="0.75", line_width=60,
                         show_del=False, fill_ref=False, iupac=False, edits_per_read=None, results=False, text_cap=None):
        """The sequence the container's reads spell, as FASTA bytes (cbc_gpu_decode_consensus): region=None gives one record
        `>NAME` per contig of the table, in table order -- contigs without reads included --, otherwise (NAME, NAME:BEG or
        NAME:BEG-END) the one record `>NAME:BEG-END` of the window.  Per position, over the counts decode_pileup prints under the
        same exclude_flags: depth < min_depth writes N (fill_ref: the reference base in lower case); else the most frequent of A, C,
        G, T and deletion -- ties go to the reference's class, then in that order -- is called when count * 10^6 >= call_ppm *
        depth, call_ppm = alt_frac_ppm(call_frac): a base writes its letter, a deletion drops the base (show_del: `*`); else with
        iupac the code of the smallest top set of bases, closed under ties, that reaches the fraction; else N.  Insertions are
        counted, not applied.  Lines hold line_width (1..65535) bytes.  The reference must have been uploaded.  A selection
        without blocks (or reads) gets its all-low-depth record from the host (plan.consensus_empty) and runs nothing on the
        device.  Returns (fasta, counts, reads kept) with counts = dict(emitted, ref, alt, del, ambiguous, low_depth, no_call,
        ins_skipped), summed over the records; ins_skipped = positions with depth >= min_depth whose insertion events reach the
        fraction (a trailing soft clip shows as one such event).  With results=True a fourth value, the per-block decode results
        of the blocks used, and a failed block passes (it contributes nothing).  text_cap: size of the buffer of one call
        (default: plan.consensus_text_cap of its window)."""
        plan.sam_header()                                     # refuses what the text cannot carry, and long-read containers
        ppm = alt_frac_ppm(call_frac)
        if int(min_depth) < 1 or int(min_depth) > 0xffffffff:
            raise ValueError("min_depth is in 1..4294967295")
        if not 1 <= int(line_width) <= 65535:
            raise ValueError("line_width is in 1..65535")
        epr = EDITS_PER_READ if edits_per_read is None else int(edits_per_read)
        if not 1 <= epr <= 510:
            raise ValueError("edits_per_read is in 1..510")
        opts = host.ConsensusOpts(int(min_depth), ppm, int(line_width), (1 if show_del else 0) | (2 if fill_ref else 0) | (4 if iupac else 0))
        rng = region is not None
        sels = [plan.region(region)] if rng else [plan.contig_blocks(c) for c in range(plan.n_contigs)]
        out, total, n_kept, allres = [], host.ConsensusCounts().as_dict(), 0, []
        self.last_consensus_text_bytes = 0
        self._consensus_ms = None
        caps, pay, _, _ = self._plan_args(plan)
        for sel in sels:
            nb = sel.b1 - sel.b0
            if nb == 0 or int(plan.blocks[sel.b0:sel.b1]["n_reads"].sum()) == 0:
                text, cnt = plan.consensus_empty(sel.contig, sel.beg, sel.end, opts, rng)
            else:
                blocks, ws, _ = self._gather(plan, slice(sel.b0, sel.b1))
                off = int(plan.contig_name_off[sel.contig])
                name = plan.names[off:].tobytes().split(b"\0", 1)[0]
                cap = plan.consensus_text_cap(sel.contig, sel.beg, sel.end, opts.line_width, rng) if text_cap is None else int(text_cap)
                buf = np.zeros(max(cap, 1), dtype=np.uint8)
                res = np.zeros(nb, dtype=host.RESULT_DTYPE)
                nbytes, nk, cc = ctypes.c_uint64(), ctypes.c_uint64(), host.ConsensusCounts()
                rc = lib().cbc_gpu_decode_consensus(self._ctx, pay.ctypes.data, pay.size, blocks.ctypes.data, nb, ctypes.byref(caps),
                                                    ws.ctypes.data, name, len(name), sel.beg, sel.end, sel.smax, int(exclude_flags), epr,
                                                    ctypes.byref(opts), int(rng), buf.ctypes.data, cap, ctypes.byref(nbytes),
                                                    ctypes.byref(cc), ctypes.byref(nk), res.ctypes.data)
                self.last_consensus_text_bytes += int(nbytes.value)
                self._check_blocks(rc, "cbc_gpu_decode_consensus", results)
                self._add_ms("_consensus_ms", "cbc_gpu_last_consensus_ms", 4, must=True)
                text, cnt = buf[:int(nbytes.value)].tobytes(), cc.as_dict()
                n_kept += int(nk.value); allres.append(res)
            out.append(text)
            for k, v in cnt.items():
                total[k] += v
        text = b"".join(out)
        return (text, total, n_kept, self._cat(allres)) if results else (text, total, n_kept)

    def last_consensus_ms(self):
        """(edits decode, zero + mark + events, scans, text) kernel milliseconds of the last decode_consensus, summed over its calls."""
        return self._summed_ms("_consensus_ms", "decode_consensus")

    def decode_blocks_edits(self, plan: "host.UnpackPlan", smax, edits_per_read=None):
        """decode_blocks_span with the alignment of the reads with indels kept as well (cbc_gpu_decode_blocks_edits).  Returns
        (recs, seq, results, side, arena): side[r] = (first arena entry of record r relative to its block's, nDel | nIns << 16),
        arena = uint16 entries, block b owning [rec_base * edits_per_read, (rec_base + n_reads) * edits_per_read)."""
        nb = plan.n_blocks
        epr = EDITS_PER_READ if edits_per_read is None else int(edits_per_read)
        blocks = plan.blocks.copy()
        recs = np.zeros(plan.n_recs, dtype=host.REC_DTYPE)
        seq = np.zeros(plan.n_recs * plan.seq_stride + 8, dtype=np.uint8)
        res = np.zeros(nb, dtype=host.RESULT_DTYPE)
        side = np.zeros((max(plan.n_recs, 1), 2), dtype=np.uint32)
        arena = np.zeros(max(plan.n_recs * epr, 1), dtype=np.uint16)
        caps = host.LdsCaps(plan.cap_pos, plan.cap_var)
        pay = np.ascontiguousarray(plan.payloads)
        rc = lib().cbc_gpu_decode_blocks_edits(self._ctx, pay.ctypes.data, pay.size, blocks.ctypes.data, nb, ctypes.byref(caps), smax, epr,
                                               recs.ctypes.data, plan.n_recs, seq.ctypes.data, seq.size, side.ctypes.data,
                                               arena.ctypes.data, res.ctypes.data)
        if rc != 0 and rc != -4:
            self._check(rc, "cbc_gpu_decode_blocks_edits")
        return recs, seq, res, side[:plan.n_recs], arena[:plan.n_recs * epr]

    def decode_targets(self, plan: "host.UnpackPlan", targets, output="reads", exclude_flags=0, results=False, text_cap=None,
                       skip_deletions=False, max_edits_per_read=EDITS_PER_READ):
        """The reads that overlap at least one interval of `targets` (a host.TargetSet of plan.targets()), in one decode of the
        selected blocks (cbc_gpu_decode_targets).  output="reads": the text `cbc -x` writes for them, each read once, in
        container order; "sam": plan.sam_header() + their alignment lines; "depth": the bedGraph of decode_depth restricted to
        the set -- per merged interval what decode_depth(region=...) gives, appended in contig-table and position order, one
        call and one decode per contig (reads with FLAG & exclude_flags != 0 left out).  An empty selection runs nothing on
        the device.  With results=True returns (text, n_reads, n_runs, per-block decode results of the blocks decoded) and
        lets a failed block pass (it contributes nothing); text_cap: size of the buffer of one call (default: the set's).
        skip_deletions / max_edits_per_read: with output="depth" as for decode_depth (ValueError with another output)."""
        kind = {"reads": 0, "sam": 1, "depth": 2}[output]
        if skip_deletions and kind != 2:
            raise ValueError("skip_deletions applies to output=\"depth\"")
        with self.skip_deletions(max_edits_per_read, skip_deletions):
            return self._decode_targets(plan, targets, kind, exclude_flags, results, text_cap, bool(skip_deletions))

    def _decode_targets(self, plan, targets, kind, exclude_flags, results, text_cap, skip_deletions):
        hdr = plan.sam_header()                               # refuses what the text cannot carry, and long-read containers
        self._targets_ms = None
        self.last_targets_text_bytes = 0
        caps, pay, names, noff = self._plan_args(plan)
        iv = np.ascontiguousarray(targets.iv, dtype=np.uint32)
        if kind == 2:
            caps_of = targets.depth_skipdel_cap if skip_deletions else targets.depth_cap
            calls = [(int(targets.contig_blk_first[c]), int(targets.contig_blk_count[c]), caps_of[c])
                     for c in range(targets.n_contigs) if targets.contig_blk_count[c]]
        else:
            calls = [(0, targets.n_blocks, targets.text_cap_sam if kind == 1 else targets.text_cap_reads)] if targets.n_blocks else []
        out, n_reads, n_runs, allres = [], 0, 0, []
        for k0, nb, cap in calls:
            blocks, ws, bc, biv = self._gather(plan, targets.blocks[k0:k0 + nb], targets.block_iv[k0:k0 + nb])
            cap = cap if text_cap is None else int(text_cap)
            text = np.zeros(max(cap, 1), dtype=np.uint8)
            res = np.zeros(nb, dtype=host.RESULT_DTYPE)
            nbytes, nrd, nrn = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
            tg = GpuTargets(iv.ctypes.data, biv.ctypes.data, targets.n_iv, targets.smax)
            rc = lib().cbc_gpu_decode_targets(self._ctx, pay.ctypes.data, pay.size, blocks.ctypes.data, nb, ctypes.byref(caps),
                                              ws.ctypes.data, bc.ctypes.data, names.ctypes.data, names.size, noff.ctypes.data,
                                              plan.n_contigs, ctypes.byref(tg), kind, int(exclude_flags), text.ctypes.data, cap,
                                              ctypes.byref(nbytes), ctypes.byref(nrd), ctypes.byref(nrn), res.ctypes.data)
            self.last_targets_text_bytes += int(nbytes.value)
            self._check_blocks(rc, "cbc_gpu_decode_targets", results)
            self._add_ms("_targets_ms", "cbc_gpu_last_targets_ms", 4)
            out.append(text[:int(nbytes.value)].tobytes() if rc in (0, -4) else b"")
            n_reads += int(nrd.value); n_runs += int(nrn.value); allres.append(res)
        text = (hdr if kind == 1 else b"") + b"".join(out)
        if results:
            return text, n_reads, n_runs, self._cat(allres)
        return text

    def decode_coverage(self, plan: "host.UnpackPlan", queries, exclude_flags=0, min_depth=1, results=False, thresholds=(),
                        count_reads=False):
        """Per-query coverage summary (cbc_gpu_decode_coverage): for every query of `queries` (a host.QuerySet of
        plan.queries()) the sum of the depth over its positions and the number of its positions with depth >= min_depth; depth
        as decode_depth counts it (reads with FLAG & exclude_flags != 0 left out).  One call and one decode per contig that has
        queries, intervals and blocks; only the numbers cross PCIe.  Returns numpy arrays in query order: contig (int64, -1:
        not in the container's table), start0, end0 (uint64, 0-based half-open), sum (uint64), covered (uint32).
        thresholds (1 to 8 depths >= 1, strictly ascending) and / or count_reads=True go through
        cbc_gpu_decode_coverage_ext: then thr (uint32, shape [n_q, T]: the positions with depth >= thresholds[t]) and / or reads
        (uint32: the kept reads with at least one covered base in the query) follow covered, in that order.  With
        results=True the per-block decode results of the blocks decoded are appended and a failed block passes (it contributes
        nothing); otherwise it raises CbcGpuError.  Inside `with enc.skip_deletions():` the depth is decode_depth's with
        skip_deletions=True -- sum, covered and thr lose the deleted bases; `reads` does not change."""
        return self._coverage(plan, queries, exclude_flags, min_depth, results, thresholds, count_reads, ())

    def decode_coverage_quant(self, plan: "host.UnpackPlan", queries, quantiles, exclude_flags=0, min_depth=1, results=False,
                              thresholds=(), count_reads=False):
        """decode_coverage with the depth quantiles of every query (cbc_gpu_decode_coverage_quant).  quantiles: 1 to 8 integer
        percentages in 0..100, strictly ascending (ValueError otherwise).  The result of decode_coverage gains quant (uint32,
        shape [n_q, len(quantiles)]) after thr, when thresholds were asked for, and before reads, when reads were asked for;
        results stays last.  With the depths of the query's positions sorted ascending, zeros included, quant is the value of
        rank max(1, ceil(p * len / 100)): p = 0 the minimum, 50 the lower median, 100 the maximum; a query that selects nothing
        gives 0."""
        try:
            pct = [int(p) for p in quantiles]
            if any(p != x for p, x in zip(pct, quantiles)):
                raise ValueError
        except (TypeError, ValueError):
            raise ValueError("quantiles are 1 to 8 integer percentages in 0..100, strictly ascending") from None
        if not 1 <= len(pct) <= 8 or any(p < 0 or p > 100 for p in pct) or any(b <= a for a, b in zip(pct, pct[1:])):
            raise ValueError("quantiles are 1 to 8 integer percentages in 0..100, strictly ascending")
        return self._coverage(plan, queries, exclude_flags, min_depth, results, thresholds, count_reads, pct)

    def _coverage(self, plan, queries, exclude_flags, min_depth, results, thresholds, count_reads, pct):
        """decode_coverage (pct empty) and decode_coverage_quant (pct: the checked percentages)."""
        plan.sam_header()                                     # refuses what the coordinates cannot carry, and long-read containers
        ts = queries.targets
        thr = np.ascontiguousarray([int(t) for t in thresholds], dtype=np.uint64)
        ext = bool(len(thr)) or bool(count_reads)
        if len(thr) > 8 or (len(thr) and (thr.min() < 1 or thr.max() > 0xffffffff or (np.diff(thr.astype(np.int64)) <= 0).any())):
            raise ValueError("thresholds are 1 to 8 depths in 1 .. 2^32 - 1, strictly ascending")
        thr = thr.astype(np.uint32)
        T = len(thr)
        pct = np.ascontiguousarray(pct, dtype=np.uint32)
        Q = len(pct)
        xquant = np.zeros((queries.n_q, Q), dtype=np.uint32)
        xthr = np.zeros((queries.n_q, T), dtype=np.uint32)
        xreads = np.zeros(queries.n_q, dtype=np.uint32)
        self._coverage_ms = None
        self._coverage_ext_ms = None
        self._coverage_quant_ms = None
        caps, pay, names, noff = self._plan_args(plan)
        iv = np.ascontiguousarray(ts.iv, dtype=np.uint32)
        total = np.zeros(queries.n_q, dtype=np.uint64)
        covered = np.zeros(queries.n_q, dtype=np.uint32)
        length = (queries.end0 - queries.start0).astype(np.uint64)
        allres = []
        for c in range(ts.n_contigs):
            k0, nb, ni = int(ts.contig_blk_first[c]), int(ts.contig_blk_count[c]), int(ts.contig_count[c])
            idx = np.flatnonzero((queries.contig == c) & (length > 0))
            if not nb or not ni or not len(idx):
                continue
            blocks, ws, bc, biv = self._gather(plan, ts.blocks[k0:k0 + nb], ts.block_iv[k0:k0 + nb])
            q = np.ascontiguousarray(np.stack([queries.q["slot"][idx], length[idx].astype(np.uint32)], axis=1), dtype=np.uint32)
            s, cv = np.zeros(len(idx), dtype=np.uint64), np.zeros(len(idx), dtype=np.uint32)
            res = np.zeros(nb, dtype=host.RESULT_DTYPE)
            nrd = ctypes.c_uint64()
            tg = GpuTargets(iv.ctypes.data, biv.ctypes.data, ts.n_iv, ts.smax)
            args = (self._ctx, pay.ctypes.data, pay.size, blocks.ctypes.data, nb, ctypes.byref(caps),
                    ws.ctypes.data, bc.ctypes.data, names.ctypes.data, names.size, noff.ctypes.data,
                    plan.n_contigs, ctypes.byref(tg), int(ts.contig_first[c]), ni, q.ctypes.data, len(idx),
                    int(exclude_flags), int(min_depth), s.ctypes.data, cv.ctypes.data, ctypes.byref(nrd),
                    res.ctypes.data)
            if Q:
                tc, rd = np.zeros((len(idx), T), dtype=np.uint32), np.zeros(len(idx), dtype=np.uint32)
                qd = np.zeros((len(idx), Q), dtype=np.uint32)
                rc = lib().cbc_gpu_decode_coverage_quant(*args, thr.ctypes.data if T else None, T, tc.ctypes.data if T else None,
                                                         rd.ctypes.data if count_reads else None, pct.ctypes.data, Q, qd.ctypes.data)
                self._check_blocks(rc, "cbc_gpu_decode_coverage_quant", results)
                self._add_ms("_coverage_quant_ms", "cbc_gpu_last_coverage_quant_ms", 13, at=(0, 7, 12))
                xthr[idx], xreads[idx], xquant[idx] = tc, rd, qd
            elif ext:
                tc, rd = np.zeros((len(idx), T), dtype=np.uint32), np.zeros(len(idx), dtype=np.uint32)
                rc = lib().cbc_gpu_decode_coverage_ext(*args, thr.ctypes.data if T else None, T, tc.ctypes.data if T else None,
                                                       rd.ctypes.data if count_reads else None)
                self._check_blocks(rc, "cbc_gpu_decode_coverage_ext", results)
                self._add_ms("_coverage_ext_ms", "cbc_gpu_last_coverage_ext_ms", 12, at=(0, 7))
                xthr[idx], xreads[idx] = tc, rd
            else:
                rc = lib().cbc_gpu_decode_coverage(*args)
                self._check_blocks(rc, "cbc_gpu_decode_coverage", results)
                self._add_ms("_coverage_ms", "cbc_gpu_last_coverage_ms", 7)
            total[idx], covered[idx] = s, cv
            allres.append(res)
        out = (queries.contig.copy(), queries.start0.copy(), queries.end0.copy(), total, covered)
        if T:
            out += (xthr,)
        if Q:
            out += (xquant,)
        if count_reads:
            out += (xreads,)
        if results:
            return out + (self._cat(allres),)
        return out

    def last_coverage_ms(self):
        """(decode, mark, scan + compact, weights, weight scans, prefixes, lookup) kernel milliseconds of the last
        decode_coverage, summed over its calls."""
        return self._summed_ms("_coverage_ms", "decode_coverage")

    def last_coverage_ext_ms(self):
        """Kernel milliseconds of the last decode_coverage with thresholds or count_reads, summed over its calls: the seven of
        last_coverage_ms (the mark also notes where the pieces start), then the start points (tile sums, scans, compact), the
        thresholds' weights, their scans, their prefixes, the lookup."""
        return self._summed_ms("_coverage_ext_ms", "decode_coverage with thresholds or count_reads")

    def last_coverage_quant_ms(self):
        """Kernel milliseconds of the last decode_coverage_quant, summed over its calls: the twelve of
        last_coverage_ext_ms, then the selection pass."""
        return self._summed_ms("_coverage_quant_ms", "decode_coverage_quant")

    def decode_depth_hist(self, plan: "host.UnpackPlan", targets=None, exclude_flags=0, max_depth=0, results=False,
                          skip_deletions=False, max_edits_per_read=EDITS_PER_READ):
        """Depth histogram (cbc_gpu_decode_depth_hist): per contig how many positions have each depth; depth as decode_depth
        counts it (reads with FLAG & exclude_flags != 0 left out).  targets=None: every contig of the container's table, whole;
        a host.TargetSet of plan.targets(): the positions of its merged intervals, every position once, and a contig is listed
        when an interval lies on it.  max_depth > 0: every depth >= max_depth is counted in bin max_depth.  One call and one
        decode per contig that has blocks; only the non-zero bins cross PCIe, and the depth-0 bin is size less their sum.
        Returns a list, in table order, of (contig, depth (uint32, ascending), bases (uint64, all > 0), size) with
        bases.sum() == size.  With results=True returns (that list, the per-block decode results of the blocks decoded) and
        lets a failed block pass (its contig's call gives no bins: everything in depth 0); otherwise it raises CbcGpuError.
        skip_deletions / max_edits_per_read: the depth as decode_depth counts it with them."""
        with self.skip_deletions(max_edits_per_read, skip_deletions):
            return self._depth_hist(plan, targets, exclude_flags, max_depth, results)

    def _depth_hist(self, plan, targets, exclude_flags, max_depth, results):
        plan.sam_header()                                     # refuses what the coordinates cannot carry, and long-read containers
        ts = plan.queries().targets if targets is None else targets
        if not 0 <= int(max_depth) <= 0xffffffff:
            raise ValueError("max_depth is 0 (no folding) or 1 .. 2^32 - 1")
        self._hist_ms = None
        caps, pay, names, noff = self._plan_args(plan)
        iv = np.ascontiguousarray(ts.iv, dtype=np.uint32)
        out, allres = [], []
        for c in range(ts.n_contigs):
            k0, nb, f, ni = int(ts.contig_blk_first[c]), int(ts.contig_blk_count[c]), int(ts.contig_first[c]), int(ts.contig_count[c])
            if not ni:
                continue
            size = ts.size[c]
            depth, bases = np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint64)
            if nb:
                blocks, ws, bc, biv = self._gather(plan, ts.blocks[k0:k0 + nb], ts.block_iv[k0:k0 + nb])
                cap = max(1, min(int(blocks["n_reads"].astype(np.int64).sum()), int(max_depth) or 0xffffffff))
                bd, bb = np.zeros(cap, dtype=np.uint32), np.zeros(cap, dtype=np.uint32)
                res = np.zeros(nb, dtype=host.RESULT_DTYPE)
                nbin, nrd = ctypes.c_uint32(), ctypes.c_uint64()
                tg = GpuTargets(iv.ctypes.data, biv.ctypes.data, ts.n_iv, ts.smax)
                rc = lib().cbc_gpu_decode_depth_hist(self._ctx, pay.ctypes.data, pay.size, blocks.ctypes.data, nb, ctypes.byref(caps),
                                                     ws.ctypes.data, bc.ctypes.data, names.ctypes.data, names.size, noff.ctypes.data,
                                                     plan.n_contigs, ctypes.byref(tg), f, ni, int(exclude_flags), int(max_depth),
                                                     bd.ctypes.data, bb.ctypes.data, cap, ctypes.byref(nbin), ctypes.byref(nrd),
                                                     res.ctypes.data)
                self._check_blocks(rc, "cbc_gpu_decode_depth_hist", results)
                self._add_ms("_hist_ms", "cbc_gpu_last_hist_ms", 5)
                n = int(nbin.value)
                depth, bases = bd[:n].copy(), bb[:n].astype(np.uint64)
                allres.append(res)
            zero = size - int(bases.sum())
            if zero < 0:
                raise CbcGpuError("cbc_gpu_decode_depth_hist: the bins of contig %d hold more positions than its intervals" % c)
            if zero:
                depth, bases = np.concatenate([np.zeros(1, dtype=np.uint32), depth]), np.concatenate([np.array([zero], dtype=np.uint64), bases])
            out.append((c, depth, bases, size))
        if results:
            return out, self._cat(allres)
        return out

    def last_hist_ms(self):
        """(decode, mark, scan + compact, zero + accumulate, bin compaction) kernel milliseconds of the last decode_depth_hist,
        summed over its calls."""
        return self._summed_ms("_hist_ms", "decode_depth_hist")

    def decode_stats(self, plan: "host.UnpackPlan", targets=None, exclude_flags=0, results=False):
        """Read statistics (cbc_gpu_decode_stats): the count tables of a first look at the reads, filled on the device in one pass
        over the decoded records and rows.  targets=None: every read of the container (plain decode); a host.TargetSet of
        plan.targets(): the reads decode_targets selects for it, each once.  A read with FLAG & exclude_flags != 0 is counted in
        `excluded` and nowhere else.  Returns a dict: reads, excluded (int), flag (65536,), len (257,), gc (101,) and cyc (5, 256;
        rows A, C, G, T, other by sequencing cycle), uint32 arrays.  A selection without blocks runs nothing and gives all-zero
        tables.  With results=True returns (that dict, the per-block decode results) and lets a failed block pass (the tables are
        all zero then); otherwise it raises CbcGpuError."""
        return self._decode_stats(plan, targets, exclude_flags, results, False, None)

    def _decode_stats(self, plan, targets, exclude_flags, results, aln, edits_per_read):
        """decode_stats, and with aln=True decode_stats_aln."""
        plan.sam_header()                                     # refuses what the coordinates cannot carry, and long-read containers
        if not 0 <= int(exclude_flags) <= 0xffff:
            raise ValueError("exclude_flags is a FLAG mask in 0 .. 65535")
        per_read = 0 if edits_per_read is None else int(edits_per_read)
        if edits_per_read is not None and not 1 <= per_read <= 510:
            raise ValueError("edits_per_read is in 1 .. 510")
        ms_attr = "_stats_aln_ms" if aln else "_stats_ms"
        setattr(self, ms_attr, None)
        st, al = host.GpuStats(), host.GpuStatsAln()
        nb = plan.n_blocks if targets is None else len(targets.blocks)
        res = np.zeros(nb, dtype=host.RESULT_DTYPE)
        if nb:
            caps, pay, _, _ = self._plan_args(plan)
            tg = None
            if targets is None:
                blocks, ws, _ = self._gather(plan, slice(0, nb))
            else:
                blocks, ws, _, biv = self._gather(plan, targets.blocks, targets.block_iv)
                iv = np.ascontiguousarray(targets.iv, dtype=np.uint32)
                tg = GpuTargets(iv.ctypes.data, biv.ctypes.data, targets.n_iv, targets.smax)
            head = (self._ctx, pay.ctypes.data, pay.size, blocks.ctypes.data, nb, ctypes.byref(caps), ws.ctypes.data,
                    ctypes.byref(tg) if tg is not None else None)
            if aln:
                rc = lib().cbc_gpu_decode_stats_aln(*head, plan.max_read_len + plan.read_length - 1, int(exclude_flags), per_read,
                                                    ctypes.byref(st), ctypes.byref(al), res.ctypes.data)
            else:
                rc = lib().cbc_gpu_decode_stats(*head, int(exclude_flags), ctypes.byref(st), res.ctypes.data)
            self._check_blocks(rc, "cbc_gpu_decode_stats_aln" if aln else "cbc_gpu_decode_stats", results)
            self._add_ms(ms_attr, "cbc_gpu_last_stats_aln_ms" if aln else "cbc_gpu_last_stats_ms", 3 if aln else 2)
        out = (dict(reads=int(st.reads), excluded=int(st.excluded), flag=np.ctypeslib.as_array(st.flag).copy(),
                    len=np.ctypeslib.as_array(st.len).copy(), gc=np.ctypeslib.as_array(st.gc).copy(),
                    cyc=np.ctypeslib.as_array(st.cyc).copy().reshape(5, 256)),)
        if aln:
            out += (host.stats_aln_dict(al),)
        if results:
            return out + (res,)
        return out if aln else out[0]

    def decode_stats_aln(self, plan: "host.UnpackPlan", targets=None, exclude_flags=0, edits_per_read=None, results=False):
        """Read statistics with the alignment tables (cbc_gpu_decode_stats_aln): decode_stats behind the edit-reporting decoder and
        one more pass that counts how the counted reads agree with the reference, in the view of decode_sam(cigar=True).  Returns
        (the dict of decode_stats, the alignment dict): reads, invalid (int), len, mm, unal, ins_cyc, del_cyc (257,), nm (767,)
        uint32 and ins_len, del_len (256,) uint64 -- the cycle tables indexed by the 1-based sequencing cycle.  edits_per_read as
        for decode_pileup (None: the default).  A selection without blocks runs nothing and gives all-zero tables.  With
        results=True returns (stats, aln, the per-block decode results) and lets a failed block pass (all tables zero then);
        otherwise it raises CbcGpuError."""
        return self._decode_stats(plan, targets, exclude_flags, results, True, edits_per_read)

    def last_stats_aln_ms(self):
        """(edits decode, zeroing + statistics pass, alignment pass) kernel milliseconds of the last decode_stats_aln."""
        return self._summed_ms("_stats_aln_ms", "decode_stats_aln")

    def last_stats_ms(self):
        """(decode, zeroing + statistics pass) kernel milliseconds of the last decode_stats."""
        return self._summed_ms("_stats_ms", "decode_stats")

    def last_targets_ms(self):
        """(decode, count + scan or mark, depth scan + compact or 0, text) kernel milliseconds of the last decode_targets,
        summed over its calls."""
        return self._summed_ms("_targets_ms", "decode_targets")

    def last_depth_ms(self, _one=False):
        """(decode, mark, scan + compact, text) kernel milliseconds of the last decode_depth, summed over its calls."""
        if not _one:
            return self._summed_ms("_depth_ms", "decode_depth")
        return self._last_ms("cbc_gpu_last_depth_ms", 4, must=True)

    def last_sam_ms(self):
        """(decode, count + scan, text) kernel milliseconds of the last decode_sam."""
        return self._last_ms("cbc_gpu_last_sam_ms", 3, must=True)

    def last_sam_cigar_ms(self):
        """(edits decode, measure, count + scan, text) kernel milliseconds of the last decode_sam(cigar=True)."""
        return self._last_ms("cbc_gpu_last_sam_cigar_ms", 4, must=True)

    def last_region_ms(self):
        """(decode, filter + scan, text) kernel milliseconds of the last decode_region."""
        return self._last_ms("cbc_gpu_last_region_ms", 3, must=True)

    def _host_batch(self, pb):
        blocks = pb.blocks.copy()
        hb = HostBatch(pb.recs.ctypes.data, pb.n_recs, pb.seq.ctypes.data, len(pb.seq), pb.tok.ctypes.data, pb.n_tok,
                       pb.names.ctypes.data, len(pb.names), blocks.ctypes.data, pb.n_blocks, host.LdsCaps(pb.cap_pos, pb.cap_var))
        return hb, blocks

    def encode_stream(self, pb: "host.PackedBatch"):
        """Whole-file stream ("compat" mode): pb packed with whole_file=True.  Returns (stream bytes, StreamResult)."""
        hb, keep = self._host_batch(pb)
        cap = int(4096 + 48 * pb.n_recs + 8 * pb.n_tok)
        out = np.zeros(cap, dtype=np.uint8)
        sr = StreamResult()
        rc = lib().cbc_gpu_encode_stream(self._ctx, ctypes.byref(hb), out.ctypes.data, cap, ctypes.byref(sr))
        if rc != 0 and rc != -4:
            self._check(rc, "cbc_gpu_encode_stream")
        return out[:int(sr.nbytes)].tobytes() if rc == 0 else b"", sr

    def encode_stream_blocks(self, pb: "host.PackedBatch"):
        """The general-form coder over ordinary blocks (fallback for blocks of more than CBC_MAX_BLOCK_READS records)."""
        hb, keep = self._host_batch(pb)
        nb = pb.n_blocks
        cap = int(4096 * nb + 48 * pb.n_recs + 8 * pb.n_tok)
        out = np.zeros(cap, dtype=np.uint8)
        offs = np.zeros(nb + 1, dtype=np.uint64)
        res = np.zeros(nb, dtype=host.RESULT_DTYPE)
        rc = lib().cbc_gpu_encode_stream_blocks(self._ctx, ctypes.byref(hb), out.ctypes.data, cap, offs.ctypes.data, res.ctypes.data)
        if rc != 0 and rc != -4:
            self._check(rc, "cbc_gpu_encode_stream_blocks")
        return [out[int(offs[b]):int(offs[b + 1])].tobytes() for b in range(nb)], res

    def decode_stream_blocks(self, payloads, pb: "host.PackedBatch", stride=None):
        """cbc_gpu_decode_stream_blocks over the payloads of encode_stream_blocks(pb): general-form streams, one per block
        (the fallback for blocks of more than CBC_MAX_BLOCK_READS records).  Returns (recs, bases[n, stride], results)."""
        nb = pb.n_blocks
        stride = stride or (pb.read_length + 3) // 4 * 4
        flat = np.frombuffer(b"".join(payloads) + b"\0" * 16, dtype=np.uint8)
        offs = np.concatenate([[0], np.cumsum([len(p) for p in payloads])]).astype(np.uint64)
        blocks = np.zeros(nb, dtype=host.DEC_BLOCK_DTYPE)
        rb = np.concatenate([[0], np.cumsum(pb.blocks["n_reads"].astype(np.uint64))])
        blocks["in_off"] = offs[:-1]; blocks["in_bytes"] = np.diff(offs).astype(np.uint32)
        blocks["ref_off"] = pb.blocks["ref_off"]; blocks["rec_base"] = rb[:-1]; blocks["seq_base"] = rb[:-1] * stride
        blocks["n_reads"] = pb.blocks["n_reads"]; blocks["read_length"] = pb.read_length; blocks["seq_stride"] = stride
        n = int(rb[-1])
        recs = np.zeros(n, dtype=host.REC_DTYPE)
        seq = np.zeros(n * stride + 16, dtype=np.uint8)
        res = np.zeros(nb, dtype=host.RESULT_DTYPE)
        rc = lib().cbc_gpu_decode_stream_blocks(self._ctx, flat.ctypes.data, flat.size - 16, blocks.ctypes.data, nb, recs.ctypes.data, n,
                                                seq.ctypes.data, seq.size, res.ctypes.data)
        if rc != 0 and rc != -4:
            self._check(rc, "cbc_gpu_decode_stream_blocks")
        return recs, seq[:n * stride].reshape(n, stride), res

    def decode_stream(self, stream: bytes, contigs, rec_cap=None):
        """Decode a whole-file stream against the uploaded reference; contigs = the packer's contig table
        (ref_off / length in FASTA order).  Retries with larger buffers while the kernel reports OUT_FULL."""
        L0 = int(lib().cbc_stream_read_length(stream, len(stream)))
        stride = min(256, (max(L0, 4) + 3) // 4 * 4)                # rows of the header read length (quirk Q7: fixed-length input)
        buf = np.frombuffer(stream, dtype=np.uint8)
        co = np.ascontiguousarray(contigs["ref_off"], dtype=np.uint64)
        cl = np.ascontiguousarray(contigs["length"], dtype=np.uint64)
        cap = int(rec_cap) if rec_cap else max(1 << 16, len(stream))   # files run at 1.4 - 2 bytes per read
        while True:
            cap = min(cap, 0xffffffff)
            recs = np.zeros(cap, dtype=host.REC_DTYPE)
            seq = np.zeros(cap * stride + 8, dtype=np.uint8)
            sr = StreamResult()
            rc = lib().cbc_gpu_decode_stream(self._ctx, buf.ctypes.data, buf.size, co.ctypes.data, cl.ctypes.data, len(co),
                                             recs.ctypes.data, cap, seq.ctypes.data, seq.size, stride, ctypes.byref(sr))
            if rc == -4 and sr.status == 1 and cap < 0xffffffff:     # OUT_FULL: more records than the buffers hold
                cap *= 2
                continue
            if rc != 0 and rc != -4:
                self._check(rc, "cbc_gpu_decode_stream")
            n = int(sr.nbytes) if sr.status == 0 else 0
            return recs[:n], seq[:n * stride].reshape(n, stride), sr

    def encode_long_blocks(self, pb: "host.PackedBatch"):
        """Long-read format (pb packed with long_reads=True).  Returns (payload list, results, offsets, flat)."""
        hb, blocks = self._host_batch(pb)
        nb = pb.n_blocks
        cap = int(8192 * nb + 13 * pb.n_bases + 64 * pb.n_recs)
        cap = min(cap, int(8192 * nb + 2 * pb.n_bases + 64 * pb.n_recs) if pb.n_bases > (1 << 28) else cap)
        out = np.zeros(cap, dtype=np.uint8)
        offs = np.zeros(nb + 1, dtype=np.uint64)
        res = np.zeros(nb, dtype=host.RESULT_DTYPE)
        rc = lib().cbc_gpu_long_encode_blocks(self._ctx, ctypes.byref(hb), out.ctypes.data, cap, offs.ctypes.data, res.ctypes.data)
        if rc != 0 and rc != -4:
            self._check(rc, "cbc_gpu_long_encode_blocks")
        return [out[int(offs[b]):int(offs[b + 1])].tobytes() for b in range(nb)], res, offs, out[:int(offs[nb])]

    def decode_long_blocks(self, plan: "host.UnpackPlan"):
        """Long-read format: returns (recs, flat bases, results); plan.text(recs, seq) gives the reads."""
        nb = plan.n_blocks
        blocks = plan.blocks.copy()
        recs = np.zeros(plan.n_recs, dtype=host.REC_DTYPE)
        seq = np.zeros(plan.seq_total + 16, dtype=np.uint8)
        res = np.zeros(nb, dtype=host.RESULT_DTYPE)
        caps = host.LdsCaps(plan.cap_pos, plan.cap_var)
        pay = np.ascontiguousarray(plan.payloads)
        rc = lib().cbc_gpu_long_decode_blocks(self._ctx, pay.ctypes.data, pay.size, blocks.ctypes.data, nb, ctypes.byref(caps),
                                              recs.ctypes.data, plan.n_recs, seq.ctypes.data, plan.seq_total, res.ctypes.data)
        if rc != 0 and rc != -4:
            self._check(rc, "cbc_gpu_long_decode_blocks")
        return recs, seq, res

    def encode_long_device(self, db: DeviceBatch, stream=None):
        self._check(lib().cbc_gpu_long_encode_blocks_device(self._ctx, ctypes.byref(db), stream), "cbc_gpu_long_encode_blocks_device")

    def decode_long_device(self, db: DecDeviceBatch, stream=None):
        self._check(lib().cbc_gpu_long_decode_blocks_device(self._ctx, ctypes.byref(db), stream), "cbc_gpu_long_decode_blocks_device")

    def decode_device(self, db: DecDeviceBatch, stream=None):
        self._check(lib().cbc_gpu_decode_blocks_device(self._ctx, ctypes.byref(db), stream), "cbc_gpu_decode_blocks_device")

    def encode_device(self, db: DeviceBatch, stream=None):
        self._check(lib().cbc_gpu_encode_blocks_device(self._ctx, ctypes.byref(db), stream), "cbc_gpu_encode_blocks_device")

    def compact_device(self, d_scratch, d_blocks, d_results, n_blocks, d_offsets, d_packed, packed_cap, stream=None):
        self._check(lib().cbc_gpu_compact_device(self._ctx, d_scratch, d_blocks, d_results, n_blocks, d_offsets,
                                                 d_packed, packed_cap, stream), "cbc_gpu_compact_device")

    def last_e2e(self):
        """What the most recent host-buffer call did (cbc_gpu_last_e2e): stage times, bytes over PCIe, chunks."""
        t = E2ETimes()
        self._check(lib().cbc_gpu_last_e2e(self._ctx, ctypes.byref(t)), "cbc_gpu_last_e2e")
        return {k: getattr(t, k) for k, _ in E2ETimes._fields_ if k != "reserved"}

    def host_register(self, arr):
        """Page-lock a numpy array the entry points read from / write to (cbc_gpu_host_register)."""
        if arr.nbytes:
            self._check(lib().cbc_gpu_host_register(self._ctx, arr.ctypes.data, arr.nbytes), "cbc_gpu_host_register")

    def host_unregister(self, arr):
        if arr.nbytes:
            self._check(lib().cbc_gpu_host_unregister(self._ctx, arr.ctypes.data), "cbc_gpu_host_unregister")

    def checksum_device(self, d_bytes, n, d_sum, stream=None):
        """cbc_gpu_checksum_device: *d_sum (device, 8 bytes) = checksum of n device bytes, asynchronous on `stream`."""
        self._check(lib().cbc_gpu_checksum_device(self._ctx, d_bytes, n, d_sum, stream), "cbc_gpu_checksum_device")

    def last_kernel_ms(self):
        ms = ctypes.c_float()
        self._check(lib().cbc_gpu_last_kernel_ms(self._ctx, ctypes.byref(ms)), "cbc_gpu_last_kernel_ms")
        return float(ms.value)

    def last_kernel_variant(self):
        return int(lib().cbc_gpu_last_kernel_variant(self._ctx))

    def synchronize(self):
        self._check(lib().cbc_gpu_synchronize(self._ctx), "cbc_gpu_synchronize")

    def close(self):
        if self._ctx:
            lib().cbc_gpu_shutdown(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
