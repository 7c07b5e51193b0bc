"""ctypes binding of libsfgpu.so (the C ABI declared in include/sfgpu.h).

The HIP library is the product path: there is no CPU fallback.  If the shared object is
missing, or a compute entry point fails, this module raises -- loudly.
"""
import ctypes as C
import os

import torch  # noqa: F401  (imported first so libamdhip64.so.7 resolves to torch's HIP runtime)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SFGPU_LIB_PATH", os.path.join(_HERE, "csrc", "libsfgpu.so"))   # override: kernel-tuning builds

OK, ERR_INVALID, ERR_HIP, ERR_NO_ACTIVE, ERR_ALPHA_SUM, ERR_RANGE, ERR_STATE, ERR_UNSUPPORTED, ERR_FORMAT, ERR_IO, ERR_CAPACITY = range(11)


class SfgpuError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libsfgpu error {code}: {msg}")
        self.code = code


class Problem(C.Structure):
    _fields_ = [("M", C.c_uint64), ("d_len", C.c_void_p), ("C", C.c_uint64), ("d_rowptr", C.c_void_p),
                ("d_ids", C.c_void_p), ("d_counts", C.c_void_p), ("num_mapped", C.c_uint64)]


class EmOpts(C.Structure):
    _fields_ = [("use_vbem", C.c_int), ("tol", C.c_double), ("min_iter", C.c_uint32), ("max_iter", C.c_uint32),
                ("check_mode", C.c_int), ("iters_per_launch", C.c_uint32)]


class EmStats(C.Structure):
    _fields_ = [("iters", C.c_uint32), ("converged", C.c_uint32), ("max_rel_diff", C.c_double),
                ("alpha_sum", C.c_double), ("n_active", C.c_uint64), ("loop_ms", C.c_double),
                ("fused", C.c_uint32), ("persistent", C.c_uint32)]

    def as_dict(self):
        return dict(iters=self.iters, converged=bool(self.converged), max_rel_diff=self.max_rel_diff,
                    alpha_sum=self.alpha_sum, n_active=self.n_active, loop_ms=self.loop_ms, fused=bool(self.fused), persistent=bool(self.persistent))


class EmPlanInfo(C.Structure):
    """struct sfgpu_em_plan_info"""
    _fields_ = [("n_tiles", C.c_uint32), ("tile_nnz", C.c_uint32), ("redone", C.c_uint32), ("most_classes", C.c_uint32),
                ("P", C.c_uint64), ("E", C.c_uint64), ("renumbered", C.c_uint32), ("gather", C.c_uint32),
                ("cover_tiles", C.c_uint32), ("most_far_slots", C.c_uint32), ("longest_far_list", C.c_uint32), ("fused_ok", C.c_uint32),
                ("n1", C.c_uint64), ("n2", C.c_uint64), ("n3", C.c_uint64), ("n4", C.c_uint64), ("n_ov", C.c_uint64),
                ("persist_verdict", C.c_uint32), ("pad_", C.c_uint32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "pad_"}


class EqStats(C.Structure):
    _fields_ = [("insert_ms", C.c_double), ("insert_launches", C.c_uint64), ("table_grows", C.c_uint64),
                ("deferred_reads", C.c_uint64), ("table_slots", C.c_uint64),
                ("hot_reads", C.c_uint64), ("spilled_reads", C.c_uint64), ("pipeline_drains", C.c_uint64)]


class EqTextResult(C.Structure):
    _fields_ = [("n_lines", C.c_uint64), ("n_ids", C.c_uint64), ("sum_counts", C.c_uint64), ("n_chunks", C.c_uint64),
                ("err_line", C.c_uint64), ("err_kind", C.c_int32), ("pad_", C.c_int32),
                ("stage_ms", C.c_double), ("h2d_ms", C.c_double), ("parse_ms", C.c_double), ("fold_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad_"}


class ReadsResult(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_bases", C.c_uint64), ("consumed", C.c_uint64), ("n_lines", C.c_uint64),
                ("error_record", C.c_uint64), ("error_line", C.c_uint64), ("format", C.c_int32), ("error_kind", C.c_int32),
                ("ms_copy", C.c_double), ("ms_kernels", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class BgzfResult(C.Structure):
    _fields_ = [("n_members", C.c_uint64), ("consumed", C.c_uint64), ("n_bytes_out", C.c_uint64), ("n_stored_blocks", C.c_uint64),
                ("n_fixed_blocks", C.c_uint64), ("n_dynamic_blocks", C.c_uint64), ("error_member", C.c_uint64),
                ("error_kind", C.c_int32), ("pad_", C.c_int32), ("ms_copy", C.c_double), ("ms_kernels", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad_"}


class GzrdResult(C.Structure):
    _fields_ = [("consumed", C.c_uint64), ("n_bytes_out", C.c_uint64), ("n_chunks", C.c_uint64), ("n_candidates", C.c_uint64),
                ("n_false_starts", C.c_uint64), ("n_stored_blocks", C.c_uint64), ("n_fixed_blocks", C.c_uint64),
                ("n_dynamic_blocks", C.c_uint64), ("need_cap", C.c_uint64), ("error_offset", C.c_uint64), ("member_end", C.c_int32),
                ("error_kind", C.c_int32), ("ms_copy", C.c_double), ("ms_find", C.c_double), ("ms_decode", C.c_double),
                ("ms_propagate", C.c_double), ("ms_emit", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class EqTextWriteResult(C.Structure):
    _fields_ = [("n_bytes", C.c_uint64), ("n_lines", C.c_uint64), ("n_ids", C.c_uint64), ("n_chunks", C.c_uint64),
                ("max_line_bytes", C.c_uint64), ("format_ms", C.c_double), ("d2h_ms", C.c_double), ("sink_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class QuantWriteResult(C.Structure):
    _fields_ = [("n_bytes", C.c_uint64), ("n_rows", C.c_uint64), ("n_chunks", C.c_uint64), ("max_row_bytes", C.c_uint64),
                ("n_slow", C.c_uint64), ("format_ms", C.c_double), ("d2h_ms", C.c_double), ("sink_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class GenesResult(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("n_genes", C.c_uint64), ("n_slow", C.c_uint64), ("max_rows_per_gene", C.c_uint64),
                ("aggregate_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class GmapAddResult(C.Structure):
    _fields_ = [("n_lines", C.c_uint64), ("n_records", C.c_uint64), ("consumed", C.c_uint64), ("needs_host", C.c_uint32),
                ("pad_", C.c_uint32), ("ms_copy", C.c_double), ("ms_kernels", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad_"}


class GmapResult(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_transcripts", C.c_uint64), ("n_genes", C.c_uint64), ("tname_bytes", C.c_uint64),
                ("gname_bytes", C.c_uint64), ("needs_host", C.c_uint32), ("sort_rounds", C.c_uint32), ("ms_kernels", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class SamcInfo(C.Structure):
    _fields_ = [("n_lines", C.c_uint64), ("n_reads", C.c_uint64), ("n_hits", C.c_uint64), ("n_pairs", C.c_uint64), ("state_bytes", C.c_uint64),
                ("sort_rounds", C.c_uint32), ("pad_", C.c_uint32), ("ms_collect", C.c_double), ("ms_finish", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad_"}


class SamResult(C.Structure):
    _fields_ = [("n_lines", C.c_uint64), ("n_header", C.c_uint64), ("n_reads", C.c_uint64), ("n_hits", C.c_uint64), ("n_pairs", C.c_uint64),
                ("consumed", C.c_uint64), ("need_hits", C.c_uint64), ("need_reads", C.c_uint64), ("bad_line", C.c_uint64), ("bad", C.c_uint32),
                ("pad_", C.c_uint32), ("ms_copy", C.c_double), ("ms_kernels", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad_"}


class SamWriteResult(C.Structure):
    _fields_ = [("n_bytes", C.c_uint64), ("n_lines", C.c_uint64), ("n_chunks", C.c_uint64), ("max_unit_bytes", C.c_uint64),
                ("error_read", C.c_uint64), ("error_record", C.c_uint64), ("error_kind", C.c_uint32), ("pad_", C.c_uint32),
                ("format_ms", C.c_double), ("d2h_ms", C.c_double), ("sink_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad_"}


class ReadWriteResult(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_selected", C.c_uint64), ("n_bytes", C.c_uint64), ("n_chunks", C.c_uint64),
                ("max_record_bytes", C.c_uint64), ("error_record", C.c_uint64), ("error_kind", C.c_int32), ("pad_", C.c_int32),
                ("format_ms", C.c_double), ("d2h_ms", C.c_double), ("sink_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_ if k != "pad_"}


class GzResult(C.Structure):
    _fields_ = [("n_bytes_in", C.c_uint64), ("n_bytes_out", C.c_uint64), ("n_blocks", C.c_uint64), ("n_stored_blocks", C.c_uint64),
                ("n_chunks", C.c_uint64), ("encode_ms", C.c_double), ("d2h_ms", C.c_double), ("sink_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class BgzwResult(C.Structure):
    _fields_ = [("n_bytes_in", C.c_uint64), ("n_bytes_out", C.c_uint64), ("n_members", C.c_uint64), ("n_stored_members", C.c_uint64),
                ("n_matches", C.c_uint64), ("n_literals", C.c_uint64), ("n_chunks", C.c_uint64), ("encode_ms", C.c_double),
                ("d2h_ms", C.c_double), ("sink_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class BamsortResult(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_no_coor", C.c_uint64), ("n_bytes", C.c_uint64), ("state_bytes", C.c_uint64),
                ("index_bytes", C.c_uint64), ("n_pieces", C.c_uint64), ("n_index_chunks", C.c_uint64), ("n_index_bins", C.c_uint64),
                ("sort_ms", C.c_double), ("gather_ms", C.c_double), ("index_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


_LOG_CB = C.CFUNCTYPE(None, C.c_int, C.c_char_p)
TEXT_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_void_p)      # sfgpu_text_sink
ALLREDUCE_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p)      # sfgpu_allreduce_fn
SAMPLE_CB = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_double), C.c_uint64, C.c_void_p)
GIBBS_CB = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_int32), C.c_uint64, C.c_void_p)
_lib = None
_log_keepalive = None

_P = C.c_void_p
class LibFmt(C.Structure):
    _fields_ = [("type", C.c_uint8), ("orientation", C.c_uint8), ("strandedness", C.c_uint8), ("pad_", C.c_uint8)]


class FilterOpts(C.Structure):
    _fields_ = [("max_read_occs", C.c_uint32), ("max_frag_len", C.c_uint32), ("paired_library", C.c_int32),
                ("discard_orphans", C.c_int32), ("ignore_compat", C.c_int32), ("enforce_compat", C.c_int32),
                ("can_dovetail", C.c_int32), ("expected", LibFmt)]


class FilterStats(C.Structure):
    _fields_ = [("n_observed", C.c_uint64), ("n_mapped", C.c_uint64), ("total_hits", C.c_uint64),
                ("upper_bound_hits", C.c_uint64), ("n_fwd", C.c_uint64), ("n_rc", C.c_uint64), ("fl_sampled", C.c_uint64)]


class VerifyOpts(C.Structure):
    _fields_ = [("min_identity_permille", C.c_uint32), ("keep_best", C.c_int32)]


class VerifyStats(C.Structure):
    _fields_ = [("records_in", C.c_uint64), ("records_out", C.c_uint64), ("reads_in", C.c_uint64), ("reads_out", C.c_uint64),
                ("failed_identity", C.c_uint64), ("dropped_not_best", C.c_uint64), ("sum_mism", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class VerifyGOpts(C.Structure):
    _fields_ = [("min_identity_permille", C.c_uint32), ("keep_best", C.c_int32), ("max_indel", C.c_uint32)]


class VerifyGStats(C.Structure):
    _fields_ = [("records_in", C.c_uint64), ("records_out", C.c_uint64), ("reads_in", C.c_uint64), ("reads_out", C.c_uint64),
                ("failed_identity", C.c_uint64), ("dropped_not_best", C.c_uint64), ("sum_edits", C.c_uint64), ("rescued", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class RescueOpts(C.Structure):
    _fields_ = [("min_identity_permille", C.c_uint32), ("window", C.c_uint32)]


class RescueStats(C.Structure):
    _fields_ = [("reads_eligible", C.c_uint64), ("records_orphan", C.c_uint64), ("jobs_with_candidates", C.c_uint64), ("candidates", C.c_uint64),
                ("reads_rescued", C.c_uint64), ("records_rescued", C.c_uint64), ("records_dropped", C.c_uint64), ("sum_mism", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class AlignGOpts(C.Structure):
    _fields_ = [("max_indel", C.c_uint32), ("reserved", C.c_uint32), ("scratch_cap_bytes", C.c_uint64)]


class AlignGStats(C.Structure):
    _fields_ = [("jobs", C.c_uint64), ("jobs_traced", C.c_uint64), ("unalignable", C.c_uint64), ("sum_nm", C.c_uint64), ("words", C.c_uint64),
                ("scratch_bytes", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class MdTagStats(C.Structure):
    _fields_ = [("slots", C.c_uint64), ("sum_nm", C.c_uint64), ("md_bytes", C.c_uint64), ("max_md_bytes", C.c_uint64), ("slots_plain", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class BiasSampler(C.Structure):
    _fields_ = [("d_seq", C.c_void_p), ("d_seq_off", C.c_void_p), ("d_ref_len", C.c_void_p), ("d_read_bias", C.c_void_p),
                ("remaining_bias_samples", C.POINTER(C.c_int64)), ("d_observed_gc", C.c_void_p), ("d_gc_prefix", C.c_void_p),
                ("n_bias_sampled", C.c_uint64), ("n_gc_sampled", C.c_uint64), ("gc_size_samp", C.c_uint32), ("pad_", C.c_uint32)]


class BiasInputs(C.Structure):
    _fields_ = [("M", C.c_uint64), ("d_seq", C.c_void_p), ("d_seq_off", C.c_void_p), ("d_ref_len", C.c_void_p),
                ("d_txp_eff_len", C.c_void_p), ("h_fl_counts", C.c_void_p), ("max_frag_len", C.c_uint32),
                ("gc_speed_samp", C.c_uint32), ("h_read_bias", C.c_void_p), ("h_observed_gc", C.c_void_p),
                ("num_fwd", C.c_int64), ("num_rc", C.c_int64), ("seq_bias", C.c_int32), ("gc_bias", C.c_int32),
                ("gc_size_samp", C.c_uint32), ("pad_", C.c_uint32)]


class BiasStats(C.Structure):
    _fields_ = [("status", C.c_int32), ("fld_low", C.c_int32), ("fld_high", C.c_int32), ("pad_", C.c_int32),
                ("n_corrected", C.c_uint64), ("n_uncorrected", C.c_uint64)]

    def as_dict(self):
        return dict(status=self.status, fld_low=self.fld_low, fld_high=self.fld_high,
                    n_corrected=self.n_corrected, n_uncorrected=self.n_uncorrected)


# The batch of the alignment writers (sfgpu_sam_write_text, sfgpu_sam_write_bgzf, sfgpu_bamsort_collect): sfgpu_samw_batch, every
# pointer a device address or None (a group left None is not written).
class SamwBatch(C.Structure):
    _fields_ = [("hits", _P), ("hit_off", _P), ("n_reads", C.c_uint32), ("paired", C.c_int), ("ref_names", _P), ("ref_name_off", _P),
                ("n_refs", C.c_uint32), ("qnames", _P), ("qname_off", _P), ("seq1", _P), ("seq1_off", _P), ("seq2", _P), ("seq2_off", _P),
                ("read_index_base", C.c_uint64), ("qual1", _P), ("qual2", _P), ("oriented", C.c_int), ("aln_pos", _P), ("aln_op_off", _P),
                ("aln_ops", _P), ("tag_nm", _P), ("tag_md_off", _P), ("tag_md", _P), ("tag_zw_rec", _P), ("tag_zw_f32", _P)]


class PosteriorStats(C.Structure):
    _fields_ = [("reads", C.c_uint64), ("reads_mapped", C.c_uint64), ("reads_multi", C.c_uint64), ("records", C.c_uint64), ("reads_flat", C.c_uint64),
                ("records_zero", C.c_uint64), ("max_records", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class LibdetOpts(C.Structure):
    _fields_ = [("max_read_occs", C.c_uint32), ("paired_library", C.c_int32), ("can_dovetail", C.c_int32), ("has_expected", C.c_int32),
                ("expected", LibFmt)]


LIBDET_KINDS = 13


class LibdetStats(C.Structure):
    _fields_ = [("reads", C.c_uint64), ("reads_mapped", C.c_uint64), ("reads_over_occs", C.c_uint64), ("reads_mixed", C.c_uint64),
                ("reads_compatible", C.c_uint64), ("votes", C.c_uint64), ("records_kind", C.c_uint64 * LIBDET_KINDS),
                ("reads_kind", C.c_uint64 * LIBDET_KINDS), ("votes_kind", C.c_uint64 * LIBDET_KINDS)]

    def as_dict(self):
        return {k: [int(v) for v in getattr(self, k)] if k.endswith("_kind") else int(getattr(self, k)) for k, _ in self._fields_}


class CovStats(C.Structure):
    _fields_ = [("reads", C.c_uint64), ("records", C.c_uint64), ("lines", C.c_uint64), ("intervals", C.c_uint64), ("empty_intervals", C.c_uint64),
                ("bases_added", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class CovResult(C.Structure):
    _fields_ = [("n_runs", C.c_uint64), ("bases_covered", C.c_uint64), ("bases_total", C.c_uint64), ("residue", C.c_uint64), ("state_bytes", C.c_uint64),
                ("n_bytes", C.c_uint64), ("n_chunks", C.c_uint64), ("max_row_bytes", C.c_uint64), ("finish_ms", C.c_double), ("format_ms", C.c_double),
                ("d2h_ms", C.c_double), ("sink_ms", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class CovgResult(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("n_pieces", "n_events", "n_keys", "n_runs", "bases_covered", "runs_unplaced", "bases_unplaced", "bases_off_model",
                                          "transcripts_placed", "transcripts_length_mismatch", "state_bytes", "n_bytes", "n_chunks", "max_row_bytes")] + \
               [(k, C.c_double) for k in ("project_ms", "format_ms", "d2h_ms", "sink_ms", "emit_ms", "sort_ms", "sum_ms", "runs_ms")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# sfgpu_galn_batch / sfgpu_galn_out / sfgpu_galn_stats: every pointer a device address or None
class GalnBatch(C.Structure):
    _fields_ = [("hits", _P), ("hit_off", _P), ("n_reads", C.c_uint32), ("pad_", C.c_uint32), ("aln_pos", _P), ("aln_op_off", _P), ("aln_ops", _P),
                ("aln_nm", _P), ("tag_nm", _P), ("tag_md_off", _P), ("tag_md", _P)]


class GalnOut(C.Structure):
    _fields_ = [("hits", _P), ("hit_off", _P), ("aln_pos", _P), ("aln_nm", _P), ("aln_op_off", _P), ("aln_ops", _P), ("cap_ops", C.c_uint64),
                ("tag_nm", _P), ("tag_md_off", _P), ("tag_md", _P), ("cap_md", C.c_uint64), ("src_record", _P)]


class GalnStats(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("records_in", "records_out", "records_unplaced", "records_unalignable", "records_off_range", "reads_emptied",
                                          "lines", "lines_spliced", "n_operations", "lines_reversed", "columns_beyond_model", "words_in", "words_out")] + \
               [(k, C.c_double) for k in ("project_ms", "size_ms", "scan_ms", "emit_ms")]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


_SIGS = {
    "sfgpu_version": (C.c_int, []),
    "sfgpu_has_variants": (C.c_int, []),
    "sfgpu_last_error": (C.c_char_p, []),
    "sfgpu_set_logger": (None, [_LOG_CB]),
    "sfgpu_pool_trim": (C.c_int, []),
    "sfgpu_pool_set_large_limit": (C.c_int, [C.c_longlong]),
    "sfgpu_index_set_seeds": (C.c_int, [_P, C.c_uint32]),
    "sfgpu_index_set_scan": (C.c_int, [_P, C.c_uint32]),
    "sfgpu_device_info": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_uint64)]),
    "sfgpu_xxh64_labels": (C.c_int, [_P, _P, C.c_uint32, _P, _P]),
    "sfgpu_eq_create": (C.c_int, [C.POINTER(_P), C.c_uint64, _P]),
    "sfgpu_eq_destroy": (C.c_int, [_P]),
    "sfgpu_eq_start": (C.c_int, [_P]),
    "sfgpu_eq_add_batch_host": (C.c_int, [_P, _P, _P, C.c_uint32]),
    "sfgpu_eq_add_batch_device": (C.c_int, [_P, _P, _P, C.c_uint32]),
    "sfgpu_eq_add_weighted_device": (C.c_int, [_P, _P, _P, _P, C.c_uint32]),
    "sfgpu_eq_add_text_host": (C.c_int, [_P, _P, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(EqTextResult)]),
    "sfgpu_reads_parse_host": (C.c_int, [_P, C.c_uint64, C.c_int, C.c_uint64, _P, C.c_uint64, _P, _P, C.POINTER(ReadsResult), _P]),
    "sfgpu_reads_parse_device": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_int, C.c_uint64, _P, C.c_uint64, _P, _P, C.POINTER(ReadsResult), _P]),
    "sfgpu_reads_parse_host_q": (C.c_int, [_P, C.c_uint64, C.c_int, C.c_uint64, _P, _P, C.c_uint64, _P, _P, C.POINTER(ReadsResult), _P]),
    "sfgpu_reads_parse_device_q": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_int, C.c_uint64, _P, _P, C.c_uint64, _P, _P, C.POINTER(ReadsResult), _P]),
    "sfgpu_reads_parse_host_n": (C.c_int, [_P, C.c_uint64, C.c_int, C.c_uint64, _P, _P, C.c_uint64, _P, _P, _P, C.c_uint64, _P,
                                           C.POINTER(C.c_uint64), C.POINTER(ReadsResult), _P]),
    "sfgpu_reads_parse_device_n": (C.c_int, [_P, C.c_uint64, C.c_uint64, C.c_int, C.c_uint64, _P, _P, C.c_uint64, _P, _P, _P, C.c_uint64, _P,
                                             C.POINTER(C.c_uint64), C.POINTER(ReadsResult), _P]),
    "sfgpu_reads_names_match": (C.c_int, [_P, _P, _P, _P, C.c_uint64, C.POINTER(C.c_uint64), _P]),
    "sfgpu_bgzf_inflate_host": (C.c_int, [_P, C.c_uint64, C.c_int, _P, C.c_uint64, C.POINTER(BgzfResult), _P]),
    "sfgpu_gzrd_open": (C.c_int, [C.POINTER(_P), C.c_uint32]),
    "sfgpu_gzrd_plan_host": (C.c_int, [_P, _P, C.c_uint64, C.c_int, C.c_uint64, C.POINTER(GzrdResult), _P]),
    "sfgpu_gzrd_emit": (C.c_int, [_P, _P, C.POINTER(GzrdResult), _P]),
    "sfgpu_gzrd_close": (C.c_int, [_P]),
    "sfgpu_eqvec_write_text": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_uint64, TEXT_SINK, _P, C.POINTER(EqTextWriteResult), _P]),
    "sfgpu_quant_write_text": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_uint64, C.c_uint64, TEXT_SINK, _P, C.POINTER(QuantWriteResult), _P]),
    "sfgpu_genes_aggregate": (C.c_int, [_P, _P, _P, _P, _P, C.c_uint64, C.c_uint64, C.c_int, _P, _P, _P, _P, _P, C.POINTER(GenesResult), _P]),
    "sfgpu_genes_write_text": (C.c_int, [_P, _P, C.c_uint64, _P, _P, _P, _P, _P, C.c_uint64, C.c_uint64, TEXT_SINK, _P,
                                         C.POINTER(QuantWriteResult), _P]),
    "sfgpu_gmap_open": (C.c_int, [C.POINTER(_P), C.c_int, C.c_char_p, C.c_uint32]),
    "sfgpu_gmap_from_host": (C.c_int, [C.POINTER(_P), _P, _P, _P, C.c_uint64, _P, _P, C.c_uint64]),
    "sfgpu_gmap_add_text_host": (C.c_int, [_P, _P, C.c_uint64, C.c_int, C.POINTER(GmapAddResult), _P]),
    "sfgpu_gmap_add_text_device": (C.c_int, [_P, _P, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(GmapAddResult), _P]),
    "sfgpu_gmap_finish": (C.c_int, [_P, C.POINTER(GmapResult), _P]),
    "sfgpu_gmap_export": (C.c_int, [_P, _P, _P, _P, _P, _P, _P]),
    "sfgpu_gmap_lookup": (C.c_int, [_P, _P, _P, C.c_uint64, _P, C.POINTER(C.c_uint64), _P]),
    "sfgpu_gmap_close": (C.c_int, [_P]),
    "sfgpu_sam_open": (C.c_int, [C.POINTER(_P), _P, _P, C.c_uint64, C.c_int, _P]),
    "sfgpu_sam_parse_host": (C.c_int, [_P, _P, C.c_uint64, C.c_int, _P, C.c_uint64, _P, C.c_uint64, C.POINTER(SamResult), _P]),
    "sfgpu_sam_parse_device": (C.c_int, [_P, _P, C.c_uint64, C.c_uint64, C.c_int, _P, C.c_uint64, _P, C.c_uint64, C.POINTER(SamResult), _P]),
    "sfgpu_sam_close": (C.c_int, [_P]),
    "sfgpu_bam_open": (C.c_int, [C.POINTER(_P), _P, _P, C.c_uint64, _P, _P, C.c_uint64, C.c_uint64, C.c_int, _P]),
    "sfgpu_bam_parse_host": (C.c_int, [_P, _P, C.c_uint64, C.c_int, _P, C.c_uint64, _P, C.c_uint64, C.POINTER(SamResult), _P]),
    "sfgpu_bam_parse_device": (C.c_int, [_P, _P, C.c_uint64, C.c_uint64, C.c_int, _P, C.c_uint64, _P, C.c_uint64, C.POINTER(SamResult), _P]),
    "sfgpu_bam_close": (C.c_int, [_P]),
    "sfgpu_samc_open": (C.c_int, [C.POINTER(_P), C.c_int, _P]),
    "sfgpu_sam_collect_host": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_int, C.POINTER(SamResult), _P]),
    "sfgpu_sam_collect_device": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(SamResult), _P]),
    "sfgpu_bam_collect_host": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_int, C.POINTER(SamResult), _P]),
    "sfgpu_bam_collect_device": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(SamResult), _P]),
    "sfgpu_samc_finish": (C.c_int, [_P, C.POINTER(SamcInfo), _P]),
    "sfgpu_samc_emit": (C.c_int, [_P, C.c_uint64, C.c_uint64, _P, C.c_uint64, _P, C.POINTER(SamResult), _P]),
    "sfgpu_samc_close": (C.c_int, [_P]),
    "sfgpu_sam_write_text": (C.c_int, [C.POINTER(SamwBatch), C.c_uint64, TEXT_SINK, _P, C.POINTER(SamWriteResult), _P]),
    "sfgpu_gz_open": (C.c_int, [C.POINTER(_P), TEXT_SINK, _P, C.c_uint64]),
    "sfgpu_gz_write_device": (C.c_int, [_P, _P, C.c_uint64, _P]),
    "sfgpu_gz_close": (C.c_int, [_P, C.POINTER(GzResult)]),
    "sfgpu_bgzw_open": (C.c_int, [C.POINTER(_P), TEXT_SINK, _P, C.c_uint64]),
    "sfgpu_bgzw_write_device": (C.c_int, [_P, _P, C.c_uint64, _P]),
    "sfgpu_bgzw_close": (C.c_int, [_P, C.POINTER(BgzwResult)]),
    "sfgpu_bgzw_track_members": (C.c_int, [_P]),
    "sfgpu_bgzw_member_sizes": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_uint64)]),
    "sfgpu_bamsort_open": (C.c_int, [C.POINTER(_P)]),
    "sfgpu_bamsort_collect": (C.c_int, [_P, C.POINTER(SamwBatch), C.POINTER(SamWriteResult), _P]),
    "sfgpu_bamsort_finish": (C.c_int, [_P, _P, C.c_uint32, C.c_uint64, TEXT_SINK, _P, C.POINTER(BamsortResult), _P]),
    "sfgpu_bamsort_close": (C.c_int, [_P]),
    "sfgpu_sam_write_bgzf": (C.c_int, [C.POINTER(SamwBatch), C.c_uint64, _P, C.c_int, C.POINTER(SamWriteResult), _P]),
    "sfgpu_reads_write_text": (C.c_int, [_P, _P, C.c_uint64, _P, _P, _P, C.c_uint64, _P, C.c_uint64, TEXT_SINK, _P, C.POINTER(ReadWriteResult), _P]),
    "sfgpu_reads_write_bgzf": (C.c_int, [_P, _P, C.c_uint64, _P, _P, _P, C.c_uint64, _P, C.c_uint64, _P, C.POINTER(ReadWriteResult), _P]),
    "sfgpu_eq_get_stats": (C.c_int, [_P, C.POINTER(EqStats)]),
    "sfgpu_eq_finish": (C.c_int, [_P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "sfgpu_eq_export_device": (C.c_int, [_P, _P, _P, _P, _P]),
    "sfgpu_eq_export_host": (C.c_int, [_P, _P, _P, _P, _P]),
    "sfgpu_cf_gaussian": (C.c_int, [C.c_uint32, C.c_uint64, C.c_uint64, _P]),
    "sfgpu_cf_counts": (C.c_int, [_P, C.c_uint32, _P]),
    "sfgpu_efflen_smoothed": (C.c_int, [_P, C.c_uint64, _P, C.c_uint32, _P, _P]),
    "sfgpu_efflen_empirical": (C.c_int, [_P, C.c_uint32, _P, C.c_uint64, _P, _P]),
    "sfgpu_index_build": (C.c_int, [C.POINTER(_P), _P, _P, _P, C.c_uint64, C.c_uint32, C.c_uint32, _P]),
    "sfgpu_index_destroy": (C.c_int, [_P]),
    "sfgpu_index_info": (C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "sfgpu_map_reads": (C.c_int, [_P, _P, _P, _P, _P, C.c_uint32, _P, C.c_uint64, _P, C.POINTER(C.c_uint64), _P]),
    "sfgpu_filter_hits": (C.c_int, [_P, _P, C.c_uint32, C.POINTER(FilterOpts), _P, _P, _P, C.POINTER(C.c_int64),
                                    C.POINTER(FilterStats), _P]),
    "sfgpu_hits_verify": (C.c_int, [_P, _P, _P, _P, _P, C.c_uint32, _P, _P, C.POINTER(VerifyOpts), _P, _P, _P, C.POINTER(C.c_uint64),
                                    C.POINTER(VerifyStats), _P]),
    "sfgpu_hits_rescue_mates": (C.c_int, [_P, _P, _P, _P, _P, C.c_uint32, _P, _P, C.POINTER(RescueOpts), _P, _P, _P, C.POINTER(C.c_uint64),
                                          C.POINTER(RescueStats), _P]),
    "sfgpu_hits_verify_gapped": (C.c_int, [_P, _P, _P, _P, _P, C.c_uint32, _P, _P, C.POINTER(VerifyGOpts), _P, _P, _P, C.POINTER(C.c_uint64),
                                           C.POINTER(VerifyGStats), _P]),
    "sfgpu_hits_align_gapped": (C.c_int, [_P, _P, _P, _P, _P, C.c_uint32, _P, _P, C.POINTER(AlignGOpts), _P, _P, _P, _P, C.c_uint64, C.POINTER(C.c_uint64),
                                          C.POINTER(AlignGStats), _P]),
    "sfgpu_hits_md_tags": (C.c_int, [_P, _P, _P, _P, _P, C.c_uint32, _P, _P, _P, _P, _P, _P, _P, _P, C.c_uint64, C.POINTER(C.c_uint64),
                                     C.POINTER(MdTagStats), _P]),
    "sfgpu_hits_posteriors": (C.c_int, [_P, _P, C.c_uint32, _P, C.c_uint64, _P, _P, _P, C.POINTER(PosteriorStats), _P]),
    "sfgpu_hits_library_kinds": (C.c_int, [_P, _P, C.c_uint32, C.POINTER(LibdetOpts), C.POINTER(C.c_int64), C.POINTER(LibdetStats), _P]),
    "sfgpu_cov_open": (C.c_int, [C.POINTER(_P), _P, C.c_uint64, _P]),
    "sfgpu_cov_close": (C.c_int, [_P]),
    "sfgpu_cov_add": (C.c_int, [_P, _P, _P, C.c_uint32, _P, _P, _P, _P, C.POINTER(CovStats), _P]),
    "sfgpu_cov_finish": (C.c_int, [_P, C.POINTER(CovResult), _P]),
    "sfgpu_cov_runs": (C.c_int, [_P, _P, _P, _P, _P]),
    "sfgpu_cov_summary": (C.c_int, [_P, _P, _P, _P]),
    "sfgpu_cov_write_text": (C.c_int, [_P, _P, _P, C.c_uint64, TEXT_SINK, _P, C.POINTER(CovResult), _P]),
    "sfgpu_cov_write_bgzf": (C.c_int, [_P, _P, _P, C.c_uint64, _P, C.POINTER(CovResult), _P]),
    "sfgpu_covg_open": (C.c_int, [C.POINTER(_P), _P, _P, _P, _P, _P, _P, C.c_uint64, C.c_uint32, _P]),
    "sfgpu_covg_close": (C.c_int, [_P]),
    "sfgpu_covg_event_cap": (C.c_int, [_P, C.c_uint64]),
    "sfgpu_covg_project": (C.c_int, [_P, _P, C.POINTER(CovgResult), _P]),
    "sfgpu_covg_runs": (C.c_int, [_P, _P, _P, _P, _P]),
    "sfgpu_covg_write_text": (C.c_int, [_P, _P, _P, C.c_uint64, TEXT_SINK, _P, C.POINTER(CovgResult), _P]),
    "sfgpu_covg_write_bgzf": (C.c_int, [_P, _P, _P, C.c_uint64, _P, C.POINTER(CovgResult), _P]),
    "sfgpu_galn_open": (C.c_int, [C.POINTER(_P), _P, _P, _P, _P, _P, _P, C.c_uint64, C.c_uint32, _P]),
    "sfgpu_galn_close": (C.c_int, [_P]),
    "sfgpu_galn_project": (C.c_int, [_P, C.POINTER(GalnBatch), C.POINTER(GalnOut), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(GalnStats), _P]),
    "sfgpu_gc_prefix": (C.c_int, [_P, _P, _P, C.c_uint64, _P, _P]),
    "sfgpu_sample_bias": (C.c_int, [_P, _P, C.c_uint32, C.POINTER(FilterOpts), C.POINTER(BiasSampler), _P]),
    "sfgpu_bias_create": (C.c_int, [C.POINTER(_P), C.POINTER(BiasInputs), _P]),
    "sfgpu_bias_destroy": (C.c_int, [_P]),
    "sfgpu_bias_update": (C.c_int, [_P, _P, _P, _P, C.POINTER(BiasStats), _P]),
    "sfgpu_bias_expected": (C.c_int, [_P, _P, _P]),
    "sfgpu_em_optimize_bias": (C.c_int, [_P, C.POINTER(EmOpts), _P, _P, _P, _P, C.POINTER(C.c_uint32), C.POINTER(EmStats)]),
    "sfgpu_em_create": (C.c_int, [C.POINTER(_P), C.POINTER(Problem), _P]),
    "sfgpu_em_destroy": (C.c_int, [_P]),
    "sfgpu_em_optimize": (C.c_int, [_P, C.POINTER(EmOpts), _P, _P, C.POINTER(EmStats)]),
    "sfgpu_em_begin": (C.c_int, [_P, C.POINTER(EmOpts)]),
    "sfgpu_em_init": (C.c_int, [_P]),
    "sfgpu_em_sweep": (C.c_int, [_P]),
    "sfgpu_em_update": (C.c_int, [_P]),
    "sfgpu_em_poll": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(EmStats)]),
    "sfgpu_em_finish": (C.c_int, [_P, _P, _P, C.POINTER(EmStats)]),
    "sfgpu_em_optimize_sharded": (C.c_int, [_P, C.POINTER(EmOpts), ALLREDUCE_CB, _P, C.c_uint32, _P, _P, C.POINTER(EmStats)]),
    "sfgpu_em_sharded_fused_ok": (C.c_int, [_P]),
    "sfgpu_em_set_sharded_fused": (C.c_int, [_P, C.c_int]),
    "sfgpu_em_stream": (_P, [_P]),
    "sfgpu_comm_available": (C.c_int, []),
    "sfgpu_comm_unique_id": (C.c_int, [_P]),
    "sfgpu_comm_create": (C.c_int, [C.POINTER(_P), _P, C.c_int, C.c_int]),
    "sfgpu_comm_count": (C.c_int, [_P, C.POINTER(C.c_int)]),
    "sfgpu_comm_destroy": (C.c_int, [_P]),
    "sfgpu_comm_allreduce_sum_f64": (C.c_int, [_P, _P, C.c_uint64, _P]),
    "sfgpu_comm_allreduce_fn": (_P, []),
    "sfgpu_comm_time_allreduce": (C.c_int, [_P, _P, C.c_uint64, C.c_uint32, _P, C.POINTER(C.c_double)]),
    "sfgpu_eqvec_owner_sizes": (C.c_int, [_P, _P, C.c_uint64, C.c_uint32, _P, _P, _P]),
    "sfgpu_eqvec_pack_by_owner": (C.c_int, [_P, _P, _P, _P, C.c_uint64, C.c_uint32, _P, _P, _P, _P, _P]),
    "sfgpu_eq_add_block_device": (C.c_int, [_P, _P, C.c_uint64, C.c_uint64, _P]),
    "sfgpu_eqvec_export_block": (C.c_int, [_P, _P, _P, _P, C.c_uint64, C.c_uint64, _P, _P]),
    "sfgpu_eqvec_merge_disjoint": (C.c_int, [_P, _P, _P, C.c_uint32, _P, _P, _P, _P, C.POINTER(C.c_int), _P]),
    "sfgpu_em_alpha_out": (_P, [_P]),
    "sfgpu_em_alpha": (_P, [_P]),
    "sfgpu_em_lengths": (_P, [_P]),
    "sfgpu_em_set_bounds": (C.c_int, [_P, C.c_uint32, C.c_uint32]),
    "sfgpu_em_allow_persistent": (C.c_int, [C.c_int]),
    "sfgpu_vb_eval": (C.c_int, [C.c_int, _P, _P, _P, C.c_uint64, _P, _P]),
    "sfgpu_em_rebase": (C.c_int, [_P, _P]),
    "sfgpu_em_time_sweep": (C.c_int, [_P, C.POINTER(EmOpts), C.c_uint32, C.POINTER(C.c_double)]),
    "sfgpu_em_plan_info": (C.c_int, [_P, C.POINTER(EmPlanInfo)]),
    "sfgpu_bootstrap": (C.c_int, [_P, C.POINTER(EmOpts), C.c_uint32, C.c_uint64, _P, SAMPLE_CB, _P, _P]),
    "sfgpu_bootstrap_counts": (C.c_int, [_P, C.c_uint64, C.c_uint64, _P]),
    "sfgpu_gibbs_sample": (C.c_int, [C.POINTER(Problem), _P, C.c_uint32, C.c_uint32, C.c_uint64, _P, GIBBS_CB, _P, _P]),
    "sfgpu_rng_eval": (C.c_int, [C.c_int, C.c_uint64, _P, _P, _P, _P, _P, C.c_uint32, C.c_uint64, _P, _P]),
    "sfgpu_chain_eval": (C.c_int, [C.c_int, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, _P, _P]),
    "sfgpu_mn_tree_eval": (C.c_int, [_P, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, _P, _P]),
    "sfgpu_tpm": (C.c_int, [_P, _P, C.c_uint64, C.c_double, _P, _P]),
}


def exported_symbols():
    """Names include/sfgpu.h declares (kept in lock-step with _SIGS by tests/test_abi.py)."""
    return sorted(_SIGS)


def lib():
    """Load libsfgpu.so (built in-tree by __graft_entry__.build()). Raises if absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(there is no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc):
    if rc != OK:
        raise SfgpuError(rc, lib().sfgpu_last_error().decode("utf-8", "replace"))


def set_logger(fn):
    """fn(level:int, msg:str) or None -- forwarded from the library (the jointLog hook)."""
    global _log_keepalive
    if fn is None:
        _log_keepalive = _LOG_CB(0)
    else:
        _log_keepalive = _LOG_CB(lambda lvl, msg: fn(lvl, msg.decode("utf-8", "replace")))
    lib().sfgpu_set_logger(_log_keepalive)


def current_stream_ptr():
    """hipStream_t of torch's current stream on the current device (0 = null stream)."""
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Device (or host) address of a contiguous tensor / numpy array."""
    if t is None:
        return C.c_void_p(0)
    if isinstance(t, torch.Tensor):
        assert t.is_contiguous()
        return C.c_void_p(t.data_ptr())
    return C.c_void_p(t.ctypes.data)
