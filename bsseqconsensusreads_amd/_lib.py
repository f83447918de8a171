"""ctypes binding of libbsdc (include/bsdc.h).  Loading fails loudly: there is no CPU fallback."""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# BSDC_LIB_PATH: an alternative build of the same library (profiling A/B runs only)
LIB_PATH = os.environ.get("BSDC_LIB_PATH") or os.path.join(HERE, "libbsdc.so")

BSDC_ABI_VERSION = 19
SMALL_BUCKETS = 8  # BSDC_SMALL_BUCKETS
LARGE_BUCKETS = 6  # BSDC_LARGE_BUCKETS
MODE_CONVERT, MODE_EXTEND, MODE_VOTE, MODE_DUMP = 1, 2, 4, 8
MODE_SKIP_SMALL, MODE_SKIP_LARGE = 16, 32
MODE_TAGS = 64  # single-strand reads + column statistics for the consensus tags
FILT_MINREADS, FILT_READERR, FILT_NOCALL, FILT_MEANQ = 1, 2, 4, 8  # bsdc_filter's reason bits


class Params(C.Structure):
    _fields_ = [("error_rate_pre_umi", C.c_double), ("error_rate_post_umi", C.c_double),
                ("min_input_base_quality", C.c_int32), ("consensus_call_overlapping_bases", C.c_int32),
                ("min_reads", C.c_int32), ("min_consensus_base_quality", C.c_int32)]


class FilterParamsC(C.Structure):
    _fields_ = [("min_reads", C.c_int32 * 3), ("max_read_error_rate", C.c_double * 3),
                ("max_base_error_rate", C.c_double * 3), ("min_base_quality", C.c_int32),
                ("max_no_call_fraction", C.c_double), ("min_mean_base_quality", C.c_int32),
                ("require_single_strand_agreement", C.c_int32)]


class InflateBlockC(C.Structure):  # bsdc_inflate_block
    _fields_ = [("src", C.c_int64), ("clen", C.c_int32), ("isize", C.c_int32), ("dst", C.c_int64)]


# bsdc_bgzf_inflate's status codes (BSDC_INFLATE_E*)
(INFLATE_EBTYPE, INFLATE_ESTORED, INFLATE_ELENGTHS, INFLATE_EREPEAT, INFLATE_ESYMBOL, INFLATE_EDIST, INFLATE_EOVERFLOW,
 INFLATE_ESHORT, INFLATE_EINPUT, INFLATE_ECOUNTS, INFLATE_ENOEOB, INFLATE_ECODE, INFLATE_ERANGE) = range(1, 14)


# bsdc_toolrec_rec as a numpy record: the tool-stage records' table (toolrec.tables)
TOOLREC_REC = [("name_off", "<i8"), ("cig_off", "<i8"), ("aux_off", "<i8"), ("aux_len", "<i4"), ("n_cig", "<i4"),
               ("ref_id", "<i4"), ("next_ref_id", "<i4"), ("next_pos", "<i4"), ("tlen", "<i4"), ("flag", "<u2"),
               ("mapq", "u1"), ("name_len", "u1"), ("reserved", "<i4")]


# bsdc_zip_rec / bsdc_zip_src as numpy records: cli zipper's tables (zipper.py)
ZIP_REC = [("rec_off", "<i8"), ("part_off", "<i8"), ("rec_len", "<i4"), ("aux_start", "<i4"), ("part_len", "<i4"),
           ("flag_or", "<u4")]
ZIP_SRC = [("off", "<i8"), ("len", "<i4"), ("aux", "<i4"), ("ref_id", "<i4"), ("pos", "<i4"), ("flag", "<u2"),
           ("name_len", "u1"), ("reserved0", "u1"), ("reserved", "<i4")]
ZIP_MAX_TAGS = 32  # BSDC_ZIP_MAX_TAGS
# bsdc_group_rec as a numpy record: cli group's record table (group.py)
GROUP_REC = [("off", "<i8"), ("len", "<i4"), ("aux", "<i4")]


class ZipTagsC(C.Structure):  # bsdc_zip_tags
    _fields_ = [("reverse", C.c_uint8 * (2 * ZIP_MAX_TAGS)), ("revcomp", C.c_uint8 * (2 * ZIP_MAX_TAGS)),
                ("remove", C.c_uint8 * (2 * ZIP_MAX_TAGS)), ("n_reverse", C.c_int32), ("n_revcomp", C.c_int32),
                ("n_remove", C.c_int32), ("reserved", C.c_int32)]


# bsdc_image_rec as a numpy record: the gather's table (batch.FamilyBatch.gather)
IMAGE_REC = [("src", "<i8"), ("l_seq", "<i4"), ("skip", "<i4"), ("len", "<i4"), ("slot", "<u4")]


class FamilyBatchC(C.Structure):
    _fields_ = [("n_rec", C.c_int64), ("n_fam", C.c_int64),
                ("fam_off", C.c_void_p), ("rec", C.c_void_p), ("rec_win", C.c_void_p),
                ("cig_off", C.c_void_p), ("cig_info", C.c_void_p), ("cigar", C.c_void_p),
                ("rt", C.c_void_p), ("seq", C.c_void_p), ("qual", C.c_void_p),
                ("small_fams", C.c_void_p), ("n_small", C.c_int64 * SMALL_BUCKETS), ("small_arena", C.c_int32 * SMALL_BUCKETS),
                ("large_fams", C.c_void_p), ("n_large", C.c_int64 * LARGE_BUCKETS), ("large_arena", C.c_int32 * LARGE_BUCKETS),
                ("max_len", C.c_int32), ("split_part_arena", C.c_int32),
                ("split_parts", C.c_void_p), ("n_split_parts", C.c_int64), ("split_part_recs", C.c_void_p),
                ("split_fams", C.c_void_p),
                ("n_split_fams", C.c_int64), ("split_partial_off", C.c_int64)]


class ConsensusC(C.Structure):
    _fields_ = [("stride", C.c_int32), ("reserved", C.c_int32),
                ("status", C.c_void_p), ("len", C.c_void_p), ("seq", C.c_void_p), ("qual", C.c_void_p),
                ("dump_pos", C.c_void_p), ("dump_len", C.c_void_p), ("dump_tags", C.c_void_p),
                ("dump_seq", C.c_void_p), ("dump_qual", C.c_void_p), ("scratch", C.c_void_p),
                ("ss_len", C.c_void_p), ("ss_base", C.c_void_p), ("ss_qual", C.c_void_p), ("ss_depth", C.c_void_p),
                ("ss_err", C.c_void_p), ("ss_wide", C.c_void_p), ("ss_wdepth", C.c_void_p), ("ss_werr", C.c_void_p)]


EXPORTS = ("bsdc_abi_version", "bsdc_ctx_create", "bsdc_ctx_set_params", "bsdc_ctx_destroy", "bsdc_last_error",
           "bsdc_load_reference", "bsdc_run", "bsdc_convert", "bsdc_extend", "bsdc_duplex_call",
           "bsdc_family_arena_bytes", "bsdc_small_arena_bytes", "bsdc_get_tables", "bsdc_model_tables",
           "bsdc_model_tables_fp64", "bsdc_agree_tables", "bsdc_phred_buckets", "bsdc_bgzf_scratch_bytes",
           "bsdc_bgzf_deflate", "bsdc_bgzf_pack", "bsdc_host_register", "bsdc_host_unregister", "bsdc_filter",
           "bsdc_bgzf_inflate", "bsdc_bgzf_inflate_host", "bsdc_fastq_text_bound", "bsdc_fastq_tmp_bytes",
           "bsdc_fastq_format", "bsdc_bgzf_crc32", "bsdc_bam_bytes_bound", "bsdc_bam_tmp_bytes", "bsdc_bam_format",
           "bsdc_image_gather", "bsdc_image_gather_host", "bsdc_image_last_error", "bsdc_metrics_words", "bsdc_metrics",
           "bsdc_metrics_filter", "bsdc_metrics_host", "bsdc_metrics_filter_host", "bsdc_metrics_last_error",
           "bsdc_toolrec_bytes_bound", "bsdc_toolrec_tmp_bytes", "bsdc_toolrec_format", "bsdc_toolrec_host",
           "bsdc_toolrec_last_error", "bsdc_zip_sort_tile", "bsdc_zip_sort_tmp_bytes", "bsdc_zip_sort",
           "bsdc_zip_sort_host", "bsdc_zip_bytes_bound", "bsdc_zip_format_tmp_bytes", "bsdc_zip_format",
           "bsdc_zip_format_host", "bsdc_zip_scan_host", "bsdc_zip_scan_prefix_host", "bsdc_zip_gather_tmp_bytes",
           "bsdc_zip_gather", "bsdc_zip_gather_host", "bsdc_zip_last_error", "bsdc_group_lds_nodes",
           "bsdc_group_tmp_bytes", "bsdc_group_assign", "bsdc_group_assign_host", "bsdc_group_bytes_bound",
           "bsdc_group_format_tmp_bytes", "bsdc_group_format", "bsdc_group_format_host", "bsdc_group_last_error")

_lib = None


def load(path: str = LIB_PATH):
    """Load libbsdc.so (built by __graft_entry__.build()); raises if it is missing."""
    global _lib
    if _lib is not None and path == LIB_PATH:
        return _lib
    if not os.path.exists(path):
        raise RuntimeError("libbsdc.so not built (%s): run `python -c 'import __graft_entry__ as g; g.build()'`" % path)
    lib = C.CDLL(path)
    lib.bsdc_abi_version.restype = C.c_int32
    lib.bsdc_ctx_create.argtypes = [C.c_int32, C.POINTER(Params), C.POINTER(C.c_void_p)]
    lib.bsdc_ctx_create.restype = C.c_int32
    lib.bsdc_ctx_set_params.argtypes = [C.c_void_p, C.POINTER(Params)]
    lib.bsdc_ctx_set_params.restype = C.c_int32
    lib.bsdc_ctx_destroy.argtypes = [C.c_void_p]
    lib.bsdc_ctx_destroy.restype = None
    lib.bsdc_last_error.argtypes = [C.c_void_p]
    lib.bsdc_last_error.restype = C.c_char_p
    lib.bsdc_load_reference.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32]
    lib.bsdc_load_reference.restype = C.c_int32
    lib.bsdc_run.argtypes = [C.c_void_p, C.POINTER(FamilyBatchC), C.POINTER(ConsensusC), C.c_int32, C.c_void_p]
    lib.bsdc_run.restype = C.c_int32
    for fn in ("bsdc_convert", "bsdc_extend"):
        getattr(lib, fn).argtypes = [C.c_void_p, C.POINTER(FamilyBatchC), C.POINTER(ConsensusC), C.c_void_p]
        getattr(lib, fn).restype = C.c_int32
    lib.bsdc_duplex_call.argtypes = [C.c_void_p, C.POINTER(FamilyBatchC), C.POINTER(ConsensusC), C.c_int32, C.c_void_p]
    lib.bsdc_duplex_call.restype = C.c_int32
    lib.bsdc_family_arena_bytes.argtypes = [C.c_int32, C.c_int64, C.c_int32, C.c_int64]
    lib.bsdc_family_arena_bytes.restype = C.c_int64
    lib.bsdc_small_arena_bytes.argtypes = [C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_int32]
    lib.bsdc_small_arena_bytes.restype = C.c_int64
    lib.bsdc_get_tables.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bsdc_get_tables.restype = C.c_int32
    lib.bsdc_model_tables.argtypes = [C.c_double, C.c_double, C.c_void_p, C.c_void_p]
    lib.bsdc_model_tables.restype = None
    lib.bsdc_model_tables_fp64.argtypes = [C.c_double, C.c_double, C.c_void_p, C.c_void_p]
    lib.bsdc_model_tables_fp64.restype = None
    lib.bsdc_agree_tables.argtypes = [C.c_double, C.c_double, C.c_void_p, C.c_void_p]
    lib.bsdc_agree_tables.restype = None
    lib.bsdc_bgzf_scratch_bytes.argtypes = [C.c_int64]
    lib.bsdc_bgzf_scratch_bytes.restype = C.c_int64
    lib.bsdc_bgzf_deflate.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bsdc_bgzf_deflate.restype = C.c_int32
    lib.bsdc_bgzf_pack.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    lib.bsdc_bgzf_pack.restype = C.c_int32
    lib.bsdc_host_register.argtypes = [C.c_int32, C.c_void_p, C.c_int64]
    lib.bsdc_host_register.restype = C.c_int32
    lib.bsdc_host_unregister.argtypes = [C.c_int32, C.c_void_p]
    lib.bsdc_host_unregister.restype = C.c_int32
    lib.bsdc_phred_buckets.argtypes = [C.c_double, C.c_double, C.c_void_p]
    lib.bsdc_phred_buckets.restype = None
    lib.bsdc_filter.argtypes = [C.c_void_p, C.POINTER(FilterParamsC), C.c_int32, C.c_int64, C.POINTER(ConsensusC),
                                C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bsdc_filter.restype = C.c_int32
    lib.bsdc_bgzf_inflate.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                      C.c_void_p]
    lib.bsdc_bgzf_inflate.restype = C.c_int32
    lib.bsdc_bgzf_inflate_host.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
    lib.bsdc_bgzf_inflate_host.restype = C.c_int32
    lib.bsdc_fastq_text_bound.argtypes = [C.c_int64, C.c_int64, C.c_int32]
    lib.bsdc_fastq_text_bound.restype = C.c_int64
    lib.bsdc_fastq_tmp_bytes.argtypes = [C.c_int64]
    lib.bsdc_fastq_tmp_bytes.restype = C.c_int64
    lib.bsdc_fastq_format.argtypes = [C.POINTER(ConsensusC), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                      C.c_void_p]
    lib.bsdc_fastq_format.restype = C.c_int32
    lib.bsdc_bgzf_crc32.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    lib.bsdc_bgzf_crc32.restype = C.c_int32
    lib.bsdc_bam_bytes_bound.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32]
    lib.bsdc_bam_bytes_bound.restype = C.c_int64
    lib.bsdc_bam_tmp_bytes.argtypes = [C.c_int64]
    lib.bsdc_bam_tmp_bytes.restype = C.c_int64
    lib.bsdc_bam_format.argtypes = [C.POINTER(ConsensusC), C.c_void_p, C.c_int32, C.c_int32, C.c_int64] + \
        [C.c_void_p] * 8 + [C.c_int64, C.c_void_p, C.c_void_p]
    lib.bsdc_bam_format.restype = C.c_int32
    lib.bsdc_image_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                      C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bsdc_image_gather.restype = C.c_int32
    lib.bsdc_image_gather_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64,
                                           C.c_void_p, C.c_void_p]
    lib.bsdc_image_gather_host.restype = C.c_int32
    lib.bsdc_image_last_error.restype = C.c_char_p
    lib.bsdc_metrics_words.argtypes = [C.c_int32]
    lib.bsdc_metrics_words.restype = C.c_int64
    lib.bsdc_metrics.argtypes = [C.c_void_p, C.POINTER(ConsensusC), C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                                 C.c_void_p]
    lib.bsdc_metrics.restype = C.c_int32
    lib.bsdc_metrics_filter.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.bsdc_metrics_filter.restype = C.c_int32
    lib.bsdc_metrics_host.argtypes = [C.c_void_p, C.POINTER(ConsensusC), C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                      C.c_void_p]
    lib.bsdc_metrics_host.restype = C.c_int32
    lib.bsdc_metrics_filter_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.bsdc_metrics_filter_host.restype = C.c_int32
    lib.bsdc_metrics_last_error.restype = C.c_char_p
    lib.bsdc_toolrec_bytes_bound.argtypes = [C.c_int64] * 5
    lib.bsdc_toolrec_bytes_bound.restype = C.c_int64
    lib.bsdc_toolrec_tmp_bytes.argtypes = [C.c_int64]
    lib.bsdc_toolrec_tmp_bytes.restype = C.c_int64
    lib.bsdc_toolrec_format.argtypes = [C.POINTER(ConsensusC), C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                        C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.bsdc_toolrec_format.restype = C.c_int32
    lib.bsdc_toolrec_host.argtypes = [C.POINTER(ConsensusC), C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                      C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                      C.c_int64]
    lib.bsdc_toolrec_host.restype = C.c_int32
    lib.bsdc_toolrec_last_error.restype = C.c_char_p
    lib.bsdc_zip_sort_tile.restype = C.c_int32
    lib.bsdc_zip_sort_tmp_bytes.argtypes = [C.c_int64]
    lib.bsdc_zip_sort_tmp_bytes.restype = C.c_int64
    lib.bsdc_zip_sort.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.bsdc_zip_sort.restype = C.c_int32
    lib.bsdc_zip_sort_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32]
    lib.bsdc_zip_sort_host.restype = C.c_int32
    lib.bsdc_zip_bytes_bound.argtypes = [C.c_void_p, C.c_int64]
    lib.bsdc_zip_bytes_bound.restype = C.c_int64
    lib.bsdc_zip_format_tmp_bytes.argtypes = [C.c_int64]
    lib.bsdc_zip_format_tmp_bytes.restype = C.c_int64
    lib.bsdc_zip_format.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                    C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(ZipTagsC), C.c_void_p, C.c_void_p,
                                    C.c_int64, C.c_void_p, C.c_void_p]
    lib.bsdc_zip_format.restype = C.c_int32
    lib.bsdc_zip_format_host.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                         C.POINTER(ZipTagsC), C.c_void_p, C.c_void_p, C.c_int64]
    lib.bsdc_zip_format_host.restype = C.c_int32
    lib.bsdc_zip_scan_host.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
    lib.bsdc_zip_scan_host.restype = C.c_int64
    lib.bsdc_zip_scan_prefix_host.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    lib.bsdc_zip_scan_prefix_host.restype = C.c_int64
    lib.bsdc_zip_gather_tmp_bytes.argtypes = [C.c_int64]
    lib.bsdc_zip_gather_tmp_bytes.restype = C.c_int64
    lib.bsdc_zip_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.bsdc_zip_gather.restype = C.c_int32
    lib.bsdc_zip_gather_host.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                         C.c_void_p, C.c_int64]
    lib.bsdc_zip_gather_host.restype = C.c_int32
    lib.bsdc_zip_last_error.restype = C.c_char_p
    lib.bsdc_group_lds_nodes.restype = C.c_int32
    lib.bsdc_group_tmp_bytes.argtypes = [C.c_int64]
    lib.bsdc_group_tmp_bytes.restype = C.c_int64
    lib.bsdc_group_assign.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                      C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bsdc_group_assign.restype = C.c_int32
    lib.bsdc_group_assign_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.bsdc_group_assign_host.restype = C.c_int32
    lib.bsdc_group_bytes_bound.argtypes = [C.c_void_p, C.c_int64]
    lib.bsdc_group_bytes_bound.restype = C.c_int64
    lib.bsdc_group_format_tmp_bytes.argtypes = [C.c_int64]
    lib.bsdc_group_format_tmp_bytes.restype = C.c_int64
    lib.bsdc_group_format.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_int64, C.c_char_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                      C.c_void_p]
    lib.bsdc_group_format.restype = C.c_int32
    lib.bsdc_group_format_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                           C.c_char_p, C.c_void_p, C.c_void_p, C.c_int64]
    lib.bsdc_group_format_host.restype = C.c_int32
    lib.bsdc_group_last_error.restype = C.c_char_p
    if lib.bsdc_abi_version() != BSDC_ABI_VERSION:
        raise RuntimeError("libbsdc ABI %d != %d" % (lib.bsdc_abi_version(), BSDC_ABI_VERSION))
    if path == LIB_PATH:
        _lib = lib
    return lib
