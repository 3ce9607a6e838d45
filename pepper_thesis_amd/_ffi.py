"""ctypes binding of the C-ABI declared in include/pepper_hip.h.

This is the only place the shared library is loaded. There is no CPU fallback: if
``libpepper_hip.so`` has not been built (``__graft_entry__.build()`` / ``pepper_thesis_amd.build``)
the import of the library fails loudly, and ``pv_create`` fails loudly when no HIP device exists.

Replaces the pybind11 module import ``from pepper_variant.build import PEPPER_VARIANT``
(reference: pepper_variant/modules/python/AlignmentSummarizer.py:1, pybind_api.h:24-279).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PEPPER_HIP_LIB") or os.path.join(_HERE, "csrc", "libpepper_hip.so")  # env override: A/B builds

c_i64_p = C.POINTER(C.c_int64)
c_i32_p = C.POINTER(C.c_int32)
c_u32_p = C.POINTER(C.c_uint32)
c_u8_p = C.POINTER(C.c_uint8)
c_i8_p = C.POINTER(C.c_int8)
c_f32_p = C.POINTER(C.c_float)

PV_OK = 0
PV_ERR_INVALID = -1
PV_ERR_NO_DEVICE = -2
PV_ERR_HIP = -3
PV_ERR_CAPACITY = -4
PV_ERR_LIMIT = -5
PV_ERR_STATE = -6

PV_WINDOW_ROWS = 33
PV_FEATURES = 26
PV_WINDOW_BYTES = PV_WINDOW_ROWS * PV_FEATURES
PV_HP_WINDOW_ROWS = 21
PV_HP_FEATURES = 48
PV_HP_WINDOW_BYTES = PV_HP_WINDOW_ROWS * PV_HP_FEATURES

# per-block statuses of pv_bgzf_inflate[_dev]
PV_BGZF_OK = 0
PV_BGZF_BAD_BTYPE = 1
PV_BGZF_STORED_LEN = 2
PV_BGZF_BAD_CODE_LENGTHS = 3
PV_BGZF_BAD_SYMBOL = 4
PV_BGZF_DIST_TOO_FAR = 5
PV_BGZF_OUTPUT_OVERFLOW = 6
PV_BGZF_OUTPUT_SHORT = 7
PV_BGZF_INPUT_OVERRUN = 8
PV_BGZF_CRC_MISMATCH = 9
PV_BGZF_BAD_ARGS = 10
BGZF_STATUS_NAMES = {0: "ok", 1: "BTYPE 3", 2: "stored LEN/NLEN mismatch", 3: "invalid code lengths", 4: "invalid symbol",
                     5: "distance too far back", 6: "output exceeds ISIZE", 7: "output shorter than ISIZE",
                     8: "payload read past its end", 9: "CRC32 mismatch", 10: "bad block table entry"}

# per-interval statuses of pv_bam_scan_dev
PV_BAMDEC_OK = 0
PV_BAMDEC_BAD_BLOCK = 1
PV_BAMDEC_BAD_RECORD = 2
PV_BAMDEC_CIGAR_LONGER = 3
PV_BAMDEC_BLOCK_SIZE = 4
PV_BAMDEC_PAST_PLAN = 5
PV_BAMDEC_SEEK = 6
PV_BAMDEC_BAD_TABLE = 7

# pv_polish_edit.kind
PV_EDIT_SUB = 1
PV_EDIT_DEL = 2
PV_EDIT_INS = 3

# pv_assess
PV_ASSESS_K = 32
PV_ASSESS_W = 128
PV_ASSESS_MAX_DIFF = 96
PV_ASSESS_TOTALS = 16
PV_ASSESS_SEG_ALIGNED = 0
PV_ASSESS_SEG_UNALIGNED = 1
PV_ASSESS_SEG_BROKEN = 2
PV_ASSESS_QBINS = 94
PV_ASSESS_ERR_SUB = 1
PV_ASSESS_ERR_INS = 2
PV_ASSESS_ERR_DEL = 3
# pv_assess_place
PV_ASSESS_PLACE_TILE = 4096
PV_ASSESS_PLACE_MAX_TRUTH = 8192
PV_ASSESS_PLACED = 0
PV_ASSESS_UNPLACED = 1
PV_ASSESS_MISPLACED = 2
# pv_kmer_support
PV_KMER_MIN_K = 11
PV_KMER_MAX_K = 31
PV_KMER_MAX_CAP = 1 << 30
PV_KMER_TILE = 4096
PV_KMER_SORT_SPAN = 2048
PV_KMER_HIST = 256
PV_KMER_NO_KEY = 0xFFFFFFFF
PV_KMER_READS_MIN_SLOTS = 1024
PV_KMER_READS_MAX_SLOTS = 1 << 34
PV_KMER_READS_PROBES = 1024
PV_KMER_MAX_PARTS = 4096

PV_PLAN_P1_LSTM = 1
PV_PLAN_P2_GRU = 2
PV_DTYPE_F32 = 0
PV_DTYPE_BF16_INPUT_GEMM = 1


class pv_params(C.Structure):
    _fields_ = [
        ("min_snp_baseq", C.c_double),
        ("min_indel_baseq", C.c_double),
        ("snp_freq_threshold", C.c_double),
        ("insert_freq_threshold", C.c_double),
        ("delete_freq_threshold", C.c_double),
        ("min_coverage_threshold", C.c_double),
        ("snp_candidate_freq_threshold", C.c_double),
        ("indel_candidate_freq_threshold", C.c_double),
        ("candidate_support_threshold", C.c_double),
        ("skip_indels", C.c_int32),
        ("candidate_window_size", C.c_int32),
        ("feature_size", C.c_int32),
        ("reserved", C.c_int32),
    ]


class pv_batch_in(C.Structure):
    _fields_ = [
        ("n_regions", C.c_int32),
        ("reserved", C.c_int32),
        ("ref_start", C.c_void_p),
        ("ref_end", C.c_void_p),
        ("cand_start", C.c_void_p),
        ("cand_end", C.c_void_p),
        ("ref_off", C.c_void_p),
        ("ref", C.c_void_p),
        ("read_off", C.c_void_p),
        ("read_pos", C.c_void_p),
        ("read_flags", C.c_void_p),
        ("read_mapq", C.c_void_p),
        ("base_off", C.c_void_p),
        ("bases", C.c_void_p),
        ("quals", C.c_void_p),
        ("cigar_off", C.c_void_p),
        ("cigar", C.c_void_p),
    ]


class pv_bam_decode_in(C.Structure):
    _fields_ = [
        ("data", C.c_void_p), ("data_bytes", C.c_int64), ("n_blocks", C.c_int64),
        ("coffset", C.c_void_p), ("next_coffset", C.c_void_p), ("out_off", C.c_void_p),
        ("isize", C.c_void_p), ("blk_status", C.c_void_p),
        ("n_intervals", C.c_int32), ("include_supplementary", C.c_int32), ("min_mapq", C.c_int32), ("reserved", C.c_int32),
        ("iv_tid", C.c_void_p), ("iv_rs", C.c_void_p), ("iv_re", C.c_void_p), ("iv_blk0", C.c_void_p), ("iv_blk1", C.c_void_p),
        ("iv_chunk_off", C.c_void_p), ("chunk_beg", C.c_void_p), ("chunk_end", C.c_void_p), ("iv_dropped", C.c_void_p),
        ("iv_rec_off", C.c_void_p), ("rec_slots", C.c_int64), ("n_chunks", C.c_int64),
    ]


class pv_batch_out(C.Structure):
    _fields_ = [
        ("capacity", C.c_int64),
        ("str_capacity", C.c_int64),
        ("region", C.c_void_p),
        ("position", C.c_void_p),
        ("depth", C.c_void_p),
        ("cand_freq", C.c_void_p),
        ("images", C.c_void_p),
        ("images_i32", C.c_void_p),
        ("cand_str", C.c_void_p),
        ("cand_off", C.c_void_p),
        ("n_out", C.c_int64),
        ("str_bytes", C.c_int64),
    ]


class pv_polish_out(C.Structure):
    _fields_ = [
        ("chunk_capacity", C.c_int64),
        ("row_capacity", C.c_int64),
        ("images", C.c_void_p),
        ("position", C.c_void_p),
        ("index", C.c_void_p),
        ("region", C.c_void_p),
        ("chunk_id", C.c_void_p),
        ("flat_images", C.c_void_p),
        ("flat_position", C.c_void_p),
        ("flat_index", C.c_void_p),
        ("region_row_off", C.c_void_p),
        ("n_chunks", C.c_int64),
        ("n_rows", C.c_int64),
        ("depth", C.c_void_p),
        ("counts", C.c_void_p),
    ]


class pv_polish_edit(C.Structure):
    _fields_ = [("position", C.c_int64), ("index", C.c_int32), ("kind", C.c_uint8), ("draft", C.c_uint8), ("base", C.c_uint8),
                ("qual", C.c_uint8)]


class pv_polish_evidence(C.Structure):
    _fields_ = [("depth", C.c_uint16), ("ref", C.c_uint16), ("alt_fwd", C.c_uint16), ("alt_rev", C.c_uint16)]


class pv_realign_out(C.Structure):
    _fields_ = [
        ("cigar_capacity", C.c_int64),
        ("read_pos", C.c_void_p),
        ("cigar_off", C.c_void_p),
        ("cigar", C.c_void_p),
        ("score", C.c_void_p),
        ("ends", C.c_void_p),
        ("state", C.c_void_p),
        ("band", C.c_void_p),
        ("n_cigar", C.c_int64),
        ("n_realigned", C.c_int64),
        ("n_dropped", C.c_int64),
    ]


class pv_assess_seg(C.Structure):
    _fields_ = [("a_start", C.c_int64), ("b_start", C.c_int64), ("n_rows", C.c_int32), ("n_cols", C.c_int32),
                ("status", C.c_int32), ("edge", C.c_int32), ("match", C.c_int32), ("sub", C.c_int32), ("ins", C.c_int32),
                ("del", C.c_int32), ("hp_ins", C.c_int32), ("hp_del", C.c_int32), ("anchor", C.c_int32), ("pair", C.c_int32)]


class pv_assess_error(C.Structure):
    _fields_ = [("a_pos", C.c_int64), ("b_pos", C.c_int64), ("pair", C.c_int32), ("segment", C.c_int32), ("kind", C.c_uint8),
                ("a_base", C.c_uint8), ("b_base", C.c_uint8), ("hp", C.c_uint8), ("qual", C.c_uint8), ("pad", C.c_uint8 * 3)]


class pv_assess_placement(C.Structure):
    _fields_ = [("b_lo", C.c_int64), ("b_hi", C.c_int64), ("truth", C.c_int32), ("strand", C.c_int32), ("status", C.c_int32),
                ("tried", C.c_int32), ("hits", C.c_int32), ("agree", C.c_int32)]


class pv_select_out(C.Structure):
    _fields_ = [
        ("read_capacity", C.c_int64),
        ("base_capacity", C.c_int64),
        ("cigar_capacity", C.c_int64),
        ("read_off", C.c_void_p),
        ("read_pos", C.c_void_p),
        ("read_flags", C.c_void_p),
        ("read_mapq", C.c_void_p),
        ("base_off", C.c_void_p),
        ("bases", C.c_void_p),
        ("quals", C.c_void_p),
        ("cigar_off", C.c_void_p),
        ("cigar", C.c_void_p),
        ("read_hp", C.c_void_p),
        ("src_read", C.c_void_p),
        ("n_reads", C.c_int64),
        ("n_bases", C.c_int64),
        ("n_cigar", C.c_int64),
    ]


class pv_rnn_dir(C.Structure):
    _fields_ = [("w_ih", C.c_void_p), ("w_hh", C.c_void_p), ("b_ih", C.c_void_p), ("b_hh", C.c_void_p)]


class pv_weights_p1(C.Structure):
    _fields_ = [
        ("encoder", pv_rnn_dir * 2),
        ("decoder", pv_rnn_dir * 2),
        ("linear_w", C.c_void_p * 5),
        ("linear_b", C.c_void_p * 5),
        ("out_w", C.c_void_p),
        ("out_b", C.c_void_p),
    ]


class pv_weights_p2(C.Structure):
    _fields_ = [
        ("encoder", pv_rnn_dir * 2),
        ("decoder", pv_rnn_dir * 2),
        ("dense_w", C.c_void_p),
        ("dense_b", C.c_void_p),
    ]


# every symbol include/pepper_hip.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("pv_create", C.c_void_p, [C.c_int]),
    ("pv_destroy", None, [C.c_void_p]),
    ("pv_last_error", C.c_char_p, []),
    ("pv_stream", C.c_void_p, [C.c_void_p]),
    ("pv_synchronize", C.c_int, [C.c_void_p]),
    ("pv_summarize_regions", C.c_int, [C.c_void_p, C.POINTER(pv_batch_in), C.POINTER(pv_params), C.POINTER(pv_batch_out)]),
    ("pv_summarize_regions_dev", C.c_int,
     [C.c_void_p, C.POINTER(pv_batch_in), C.POINTER(pv_params), C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
      C.POINTER(pv_batch_out), C.c_void_p, C.c_void_p]),
    ("pv_upload_batch", C.c_int, [C.c_void_p, C.POINTER(pv_batch_in), C.POINTER(pv_batch_in), C.POINTER(C.c_int64), C.c_void_p]),
    ("pv_upload_batches", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.POINTER(pv_batch_in)), C.POINTER(pv_batch_in), C.POINTER(C.c_int64), C.c_void_p]),
    ("pv_summarize_regions_hp", C.c_int,
     [C.c_void_p, C.POINTER(pv_batch_in), C.POINTER(C.c_int32), C.POINTER(pv_params), C.POINTER(pv_batch_out)]),
    ("pv_summarize_regions_hp_dev", C.c_int,
     [C.c_void_p, C.POINTER(pv_batch_in), C.c_void_p, C.POINTER(pv_params), C.c_int64, C.c_int64, C.c_int64, C.c_int64,
      C.POINTER(pv_batch_out), C.c_void_p, C.c_void_p]),
    ("pv_polish_summarize_regions", C.c_int, [C.c_void_p, C.POINTER(pv_batch_in), C.c_int, C.c_int, C.POINTER(pv_polish_out)]),
    ("pv_polish_summarize_regions_dev", C.c_int,
     [C.c_void_p, C.POINTER(pv_batch_in), C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int,
      C.POINTER(pv_polish_out), C.c_void_p, C.c_void_p]),
    ("pv_polish_stitch_dev", C.c_int,
     [C.c_void_p, C.POINTER(pv_polish_out), C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
      C.c_int64, C.c_void_p, C.c_void_p]),
    ("pv_polish_stitch", C.c_int,
     [C.c_void_p, C.POINTER(pv_polish_out), C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
      C.c_int64, C.POINTER(C.c_int64)]),
    ("pv_polish_row_qual_dev", C.c_int,
     [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pv_polish_row_qual", C.c_int,
     [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int64)]),
    ("pv_polish_qual_threshold", C.c_float, [C.c_int]),
    ("pv_polish_stitch_qual_dev", C.c_int,
     [C.c_void_p, C.POINTER(pv_polish_out), C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
      C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pv_polish_stitch_qual", C.c_int,
     [C.c_void_p, C.POINTER(pv_polish_out), C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
      C.c_int64, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p]),
    ("pv_polish_edits_dev", C.c_int,
     [C.c_void_p, C.POINTER(pv_polish_out), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int,
      C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ("pv_polish_edits", C.c_int,
     [C.c_void_p, C.POINTER(pv_polish_out), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int,
      C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    ("pv_polish_edits_evidence_dev", C.c_int,
     [C.c_void_p, C.POINTER(pv_polish_out), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int,
      C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ("pv_polish_edits_evidence", C.c_int,
     [C.c_void_p, C.POINTER(pv_polish_out), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int,
      C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    ("pv_polish_mask_low_depth_dev", C.c_int,
     [C.c_void_p, C.POINTER(pv_polish_out), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int,
      C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pv_polish_mask_low_depth", C.c_int,
     [C.c_void_p, C.POINTER(pv_polish_out), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int,
      C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]),
    ("pv_polish_filter_low_qual_dev", C.c_int,
     [C.c_void_p, C.POINTER(pv_polish_out), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int,
      C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pv_polish_filter_low_qual", C.c_int,
     [C.c_void_p, C.POINTER(pv_polish_out), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int,
      C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]),
    ("pv_polish_filter_low_support_dev", C.c_int,
     [C.c_void_p, C.POINTER(pv_polish_out), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int,
      C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pv_polish_filter_low_support", C.c_int,
     [C.c_void_p, C.POINTER(pv_polish_out), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int,
      C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]),
    ("pv_polish_vote_dev", C.c_int,
     [C.c_void_p, C.POINTER(pv_polish_out), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.c_int, C.c_void_p,
      C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pv_polish_vote", C.c_int,
     [C.c_void_p, C.POINTER(pv_polish_out), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.c_int, C.c_void_p,
      C.c_void_p, C.POINTER(C.c_int64)]),
    ("pv_polish_vote_runs_dev", C.c_int,
     [C.c_void_p, C.POINTER(pv_polish_out), C.c_int64, C.POINTER(pv_batch_in), C.c_int64, C.c_int64, C.c_int64, C.c_int64,
      C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pv_polish_vote_runs", C.c_int,
     [C.c_void_p, C.POINTER(pv_polish_out), C.c_int64, C.POINTER(pv_batch_in), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
      C.POINTER(C.c_int64)]),
    ("pv_polish_realign", C.c_int, [C.c_void_p, C.POINTER(pv_batch_in), C.c_void_p, C.c_void_p, C.POINTER(pv_realign_out)]),
    ("pv_polish_realign_dev", C.c_int,
     [C.c_void_p, C.POINTER(pv_batch_in), C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(pv_realign_out),
      C.c_void_p, C.c_void_p]),
    ("pv_batch_select_hp_dev", C.c_int,
     [C.c_void_p, C.POINTER(pv_batch_in), C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.POINTER(pv_select_out),
      C.c_void_p, C.c_void_p]),
    ("pv_batch_select_hp", C.c_int, [C.c_void_p, C.POINTER(pv_batch_in), C.c_void_p, C.c_int, C.POINTER(pv_select_out)]),
    ("pv_bgzf_inflate_dev", C.c_int,
     [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
      C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pv_bgzf_inflate", C.c_int,
     [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
      C.c_int64, C.c_void_p, C.POINTER(C.c_int64)]),
    ("pv_bam_decode_ws_bytes", C.c_int64, [C.c_int64, C.c_int64]),
    ("pv_bam_scan_dev", C.c_int, [C.c_void_p, C.POINTER(pv_bam_decode_in), C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ("pv_bam_fill_dev", C.c_int,
     [C.c_void_p, C.POINTER(pv_bam_decode_in), C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
      C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.POINTER(pv_batch_in), C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pv_rnn_load_p1", C.c_int, [C.c_void_p, C.POINTER(pv_weights_p1), C.c_int]),
    ("pv_rnn_load_p2", C.c_int, [C.c_void_p, C.POINTER(pv_weights_p2), C.c_int]),
    ("pv_rnn_forward_p1", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    ("pv_rnn_forward_p1_dev", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ("pv_rnn_forward_p1_debug", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pv_rnn_forward_p2", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ("pv_rnn_forward_p2_dev", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pv_rnn_forward_p2_window", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ("pv_comm_unique_id", C.c_int, [C.c_void_p, C.c_char_p]),
    ("pv_comm_create", C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    ("pv_comm_destroy", None, [C.c_void_p]),
    ("pv_gather", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_int, C.c_void_p]),
    ("pv_gather_counts", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.c_void_p]),
    ("pv_debug_gemm_bf16x3", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_void_p, C.POINTER(C.c_float)]),
    ("pv_debug_gemm_bf16x6", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_void_p, C.POINTER(C.c_float)]),
    ("pv_debug_gemm_x6_stream", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int,
                                           C.c_void_p, C.POINTER(C.c_float)]),
    ("pv_profile_begin", C.c_int, [C.c_void_p]),
    ("pv_profile_begin_only", C.c_int, [C.c_void_p, C.c_char_p]),
    ("pv_profile_end", C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_int), C.c_int]),
    ("pv_rnn_exchange_timeouts", C.c_int, [C.c_void_p]),
    ("pv_set_option", C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    ("pv_get_option", C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_int)]),
    ("pv_graph_begin", C.c_int, [C.c_void_p, C.c_void_p]),
    ("pv_graph_end", C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    ("pv_graph_launch", C.c_int, [C.c_void_p, C.c_void_p]),
    ("pv_graph_destroy", None, [C.c_void_p]),
    ("pv_assess_dev", C.c_int,
     [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p,
      C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ("pv_assess", C.c_int,
     [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p,
      C.c_void_p, C.POINTER(C.c_int64)]),
    ("pv_assess_scratch_bytes", C.c_int64, [C.c_int64, C.c_void_p, C.c_int]),
    ("pv_assess_errors_dev", C.c_int,
     [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p,
      C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ("pv_assess_errors", C.c_int,
     [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p,
      C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]),
    ("pv_assess_errors_scratch_bytes", C.c_int64, [C.c_int64, C.c_void_p, C.c_int]),
    ("pv_assess_place_dev", C.c_int,
     [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
      C.c_int64, C.c_void_p, C.c_void_p]),
    ("pv_assess_place", C.c_int,
     [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p,
      C.POINTER(C.c_int64)]),
    ("pv_assess_place_scratch_bytes", C.c_int64, [C.c_int64, C.c_void_p, C.c_int]),
    ("pv_kmer_table_build_dev", C.c_int,
     [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    ("pv_kmer_count_reads_dev", C.c_int,
     [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    ("pv_kmer_support_dev", C.c_int,
     [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
      C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pv_kmer_support", C.c_int,
     [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int,
      C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]),
    ("pv_kmer_table_bytes", C.c_int64, [C.c_int64, C.c_void_p]),
    ("pv_kmer_reads_table_bytes", C.c_int64, [C.c_int64]),
    ("pv_kmer_reads_table_init_dev", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p]),
    ("pv_kmer_count_reads_all_dev", C.c_int,
     [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int,
      C.c_void_p]),
    ("pv_kmer_reads_flush_dev", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pv_kmer_spectrum_dev", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pv_kmer_spectrum", C.c_int,
     [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int,
      C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]),
    ("pv_workspace_bytes", C.c_int64, [C.c_void_p]),
    ("pv_version", C.c_int, []),
]

_lib = None


class PepperHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("pepper_hip error %d: %s" % (code, msg))
        self.code = code


def load():
    """Load libpepper_hip.so (once) and set prototypes. Raises if the library was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libpepper_hip.so is missing at %s - build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
    try:
        # PyTorch-ROCm wheels carry their own libamdhip64 / libhsa-runtime64. Load them FIRST so that this library's
        # DT_NEEDED entries resolve to the copies already in the process: two HIP runtimes in one process cannot both
        # open the device (torch then reports "No HIP GPUs are available" when it initialises second).
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, res, args in SYMBOLS:
        fn = getattr(lib, name)  # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(code):
    if code != PV_OK:
        msg = load().pv_last_error()
        raise PepperHipError(code, msg.decode() if msg else "")
    return code


def ptr(a):
    """address of a numpy array (must be C-contiguous) or 0 for None"""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data
