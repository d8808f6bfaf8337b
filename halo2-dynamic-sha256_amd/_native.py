"""ctypes binding of libhsw.so -- the C ABI declared in include/hsw.h.

The library is built in-tree by csrc/Makefile (hipcc, gfx950).  There is no
fallback: if it is missing the import of the engine fails loudly.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HSW_LIB_OVERRIDE") or os.path.join(_HERE, "libhsw.so")   # override: A/B tuning only
CSRC = os.path.join(_HERE, "csrc")

HSW_OK = 0
HSW_ERR_INVALID_ARG = 1
HSW_ERR_SHAPE = 2
HSW_ERR_NO_DEVICE = 3
HSW_ERR_HIP = 4
HSW_ERR_UNSUPPORTED = 5
HSW_ERR_TOO_LARGE = 6
HSW_ERR_NOMEM = 7

HSW_REPR_CANONICAL = 0
HSW_REPR_MONTGOMERY = 1
HSW_SKIP_GATE = 2
HSW_SKIP_CHIP = 4
HSW_HOST_REGISTER = 8
HSW_REPR_COMPACT64 = 16
HSW_CHAINED = 32
HSW_MODE_DEFAULT = 0
HSW_MODE_HALO2_INTERNALS = 1
HSW_MAX_BREAKS = 16
HSW_CELL_BYTES = 32
HSW_GADGET_WHOLE_DIGEST = 1
HSW_GADGET_INDEPENDENT = 2
HSW_GADGET_CONTEXT_IMAGES = 4
HSW_GADGET_SHARED_CONTEXT = 8
HSW_GADGET_MAX_COLUMNS = 1024
NO_CELL = (1 << 64) - 1


class Shape(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in (
        "num_bits_lookup", "num_advice_columns", "limbs_per_spread", "cells_per_spread",
        "cells_per_state_spread", "cells_per_sigma", "cells_per_ch", "cells_per_maj",
        "cells_per_sched_step", "cells_per_round", "off_words", "off_msg_spread", "off_sched",
        "off_state_spread", "off_rounds", "off_feed", "gate_cells_per_block",
        "spread_calls_per_block", "limb_calls_per_block", "chip_cells_per_block")] + [
        ("algorithmic_bytes_per_block", C.c_uint64), ("mode", C.c_uint32),
        ("lookup_cells_per_block", C.c_uint32), ("gate_calls_per_block", C.c_uint32),
        ("reserved_", C.c_uint32)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class PackPlan(C.Structure):
    _fields_ = [("n_breaks", C.c_uint32), ("columns_touched", C.c_uint32),
                ("break_cell", C.c_uint64 * HSW_MAX_BREAKS), ("break_gap", C.c_uint64 * HSW_MAX_BREAKS),
                ("span_cells", C.c_uint64), ("end_row", C.c_uint64)]


class WitnessArgs(C.Structure):
    _fields_ = [("d_blocks", C.c_void_p), ("d_pre_states", C.c_void_p), ("n_blocks", C.c_size_t),
                ("spread_cursor0", C.c_uint64), ("d_gate", C.c_void_p), ("d_chip_dense", C.c_void_p),
                ("d_chip_spread", C.c_void_p), ("chip_col_stride", C.c_size_t), ("d_next_states", C.c_void_p),
                ("d_lookup", C.c_void_p), ("flags", C.c_uint32), ("pack", C.POINTER(PackPlan)),
                ("frame_every", C.c_uint64), ("frame_cells", C.c_uint64), ("frame_lookups", C.c_uint64)]


class LaunchInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("limbs", "tile_cells", "tile_rows", "repr", "internals", "parts", "split",
                                          "seq")] + [("n_blocks", C.c_uint64), ("grid", C.c_uint64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}

    def kernel_name(self):
        if self.split & 4:      # a gadget bound by hsw_gadget_bind_columns: the wide table-path instantiations
            if self.split & 2:
                return "hsw::hsw_small_table_kernel<%d, %d, true>" % (self.limbs, self.repr)
            return "hsw::hsw_expand_table_kernel<%d, %d, %d, %d, true>" % (self.limbs, self.tile_cells, self.tile_rows, self.repr)
        if self.split == 2:
            return "hsw::hsw_small_kernel<%d, %d, %s>" % (self.limbs, self.repr, "true" if self.internals else "false")
        return "hsw::hsw_expand_kernel<%d, %d, %d, %d, %s>" % (self.limbs, self.tile_cells, self.tile_rows, self.repr,
                                                              "true" if self.internals else "false")


class WideCell(C.Structure):
    _fields_ = [("stream", C.c_uint64), ("index", C.c_uint64), ("value", C.c_uint64 * 4)]


class RegionCompact(C.Structure):
    _fields_ = [("gate", C.c_void_p), ("lookup", C.c_void_p), ("chip_dense", C.c_void_p), ("chip_spread", C.c_void_p),
                ("wide", C.c_void_p), ("wide_cap", C.c_size_t), ("n_wide", C.c_size_t)]


class ResultCells(C.Structure):
    _fields_ = [("input_len_cell", C.c_uint64), ("input_bytes_cell0", C.c_uint64), ("n_input_bytes", C.c_uint64),
                ("output_byte_cells", C.c_uint64 * 32), ("input_len_pos", C.c_uint64 * 2),
                ("input_bytes_pos0", C.c_uint64 * 2), ("output_byte_pos", (C.c_uint64 * 2) * 32)]


class DigestsArgs(C.Structure):
    """hsw_digests_args (descs: pointer to FrameDesc, declared below -> void pointer here)."""
    _fields_ = [("blocks", WitnessArgs), ("descs", C.c_void_p), ("n_digests", C.c_size_t), ("d_blocks0", C.c_void_p),
                ("d_pre_states0", C.c_void_p), ("d_next_states0", C.c_void_p), ("d_gate0", C.c_void_p),
                ("d_lookup0", C.c_void_p), ("frame_pack", C.POINTER(PackPlan)), ("host_next_states", C.c_void_p)]


class FrameShape(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "n_blocks", "prologue_cells", "epilogue_cells", "prologue_lookups", "epilogue_lookups",
        "prologue_calls", "epilogue_calls", "digest_cells", "digest_lookups")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class FrameDesc(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "input_len", "first_block", "prologue_cell", "epilogue_cell", "prologue_lookup",
        "epilogue_lookup", "zero_cell")] + [(n, C.c_uint32) for n in (
        "n_blocks", "num_round", "precomputed_round", "is_input_range_check")]


class DigestInfo(C.Structure):
    _fields_ = [("num_round", C.c_size_t), ("precomputed_round", C.c_size_t),
                ("target_round", C.c_size_t), ("n_blocks", C.c_size_t)]


class HashResult(C.Structure):
    _fields_ = [("input_len", C.c_uint64), ("first_block", C.c_size_t), ("n_blocks", C.c_size_t),
                ("spread_cursor0", C.c_uint64), ("num_round", C.c_size_t), ("target_round", C.c_size_t),
                ("output_bytes", C.c_uint8 * 32)] + [(n, C.c_uint64) for n in (
        "prologue_cell", "block_cell", "epilogue_cell", "end_cell",
        "prologue_lookup", "block_lookup", "epilogue_lookup")]


class StructureCounts(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("gate_cells", "gate_rows", "assert_eq", "ranges", "lookups", "limb_calls")]


class VerifyReport(C.Structure):
    _fields_ = [("violations", C.c_uint64), ("checks", C.c_uint64), ("first_block", C.c_uint64),
                ("first_cell", C.c_int64), ("first_class", C.c_uint32), ("kernel_ms", C.c_float)]
    CLASSES = {1: "constant", 2: "copy", 3: "gate row", 4: "assert_equal", 5: "range", 6: "chip", 7: "lookup",
               8: "next state"}


class FrameStructureCounts(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("cells", "gate_rows", "assert_eq", "assert_const", "ranges", "lookups")]


class RegionHost(C.Structure):
    _fields_ = [("gate", C.c_void_p), ("lookup", C.c_void_p), ("chip_dense", C.c_void_p), ("chip_spread", C.c_void_p)]


class RegionTape(C.Structure):
    _fields_ = [("n_distinct", C.c_uint64), ("distinct_capacity", C.c_uint64), ("gate_cells", C.c_uint64),
                ("lookup_cells", C.c_uint64), ("limb_calls", C.c_uint64), ("gate_code", C.POINTER(C.c_uint32)),
                ("lookup_code", C.POINTER(C.c_uint32)), ("chip_dense_code", C.POINTER(C.c_uint32)),
                ("chip_spread_code", C.POINTER(C.c_uint32)), ("consts", C.c_void_p), ("n_consts", C.c_uint64)]


HSW_TAPE_CONST = 0x80000000


class GadgetView(C.Structure):
    _fields_ = [("d_gate", C.c_void_p), ("d_chip_dense", C.c_void_p), ("d_chip_spread", C.c_void_p),
                ("d_next_states", C.c_void_p), ("chip_col_stride", C.c_size_t), ("blocks_done", C.c_size_t),
                ("capacity_blocks", C.c_size_t), ("num_limb_sum", C.c_uint64), ("cur_hash_idx", C.c_size_t),
                ("gate_cells", C.c_uint64), ("gate_capacity", C.c_uint64), ("d_lookup", C.c_void_p),
                ("lookup_cells", C.c_uint64), ("lookup_capacity", C.c_uint64),
                ("max_rows", C.c_uint64), ("columns", C.c_uint64),
                ("origin_column", C.c_uint64), ("origin_row", C.c_uint64), ("origin_lookups", C.c_uint64),
                ("origin_zero_loaded", C.c_uint32), ("reserved_", C.c_uint32)]


class RegionBinding(C.Structure):
    """hsw_region_binding: caller-owned device columns a gadget's region is bound to, pitches in cells."""
    _fields_ = [("d_columns", C.c_void_p), ("column_pitch", C.c_uint64), ("columns_capacity", C.c_uint64), ("context_pitch", C.c_uint64),
                ("d_lookup", C.c_void_p), ("lookup_capacity", C.c_uint64), ("lookup_pitch", C.c_uint64),
                ("d_chip_dense", C.c_void_p), ("d_chip_spread", C.c_void_p), ("chip_col_stride", C.c_uint64),
                ("chip_rows_capacity", C.c_uint64), ("chip_context_pitch", C.c_uint64)]


class ColumnTables(C.Structure):
    """hsw_column_tables: host arrays of device pointers, one per column per proof (hsw_gadget_bind_column_tables)."""
    _fields_ = [("d_column_ptrs", C.POINTER(C.c_void_p)), ("n_column_ptrs", C.c_size_t),
                ("d_lookup_ptrs", C.POINTER(C.c_void_p)), ("n_lookup_ptrs", C.c_size_t),
                ("d_chip_dense_ptrs", C.POINTER(C.c_void_p)), ("d_chip_spread_ptrs", C.POINTER(C.c_void_p)),
                ("n_chip_ptrs", C.c_size_t)]


class ContextRegion(C.Structure):
    """hsw_context_region: where proof h of an HSW_GADGET_CONTEXT_IMAGES gadget lives on the device."""
    _fields_ = [("d_image", C.c_void_p), ("d_lookup", C.c_void_p), ("d_chip_dense", C.c_void_p), ("d_chip_spread", C.c_void_p)] + \
               [(n, C.c_uint64) for n in ("columns", "max_rows", "last_column_rows", "stream_cells", "first_stream_cell",
                                          "lookup_cells", "chip_rows", "chip_col_stride", "origin_column", "origin_row",
                                          "origin_lookups")] + \
               [("assigned", C.c_uint32), ("reserved_", C.c_uint32)]


class CellTie(C.Structure):
    """hsw_cell_tie: input-byte cell dst_byte of digest dst_hash equals output-byte cell src_byte of digest src_hash."""
    _fields_ = [("src_hash", C.c_uint64), ("dst_hash", C.c_uint64), ("src_byte", C.c_uint32), ("dst_byte", C.c_uint32),
                ("src_cell", C.c_uint64), ("dst_cell", C.c_uint64)]


class TieReport(C.Structure):
    _fields_ = [("violations", C.c_uint64), ("checks", C.c_uint64), ("first", C.c_uint64), ("kernel_ms", C.c_float)]


HSW_LOOKUP_RANGE, HSW_LOOKUP_SPREAD = 0, 1
HSW_LOOKUP_ACCUMULATE = 1


class LookupRun(C.Structure):
    """hsw_lookup_run: n lookup entries of proof `context` as consecutive device cells (hsw_gadget_lookup_runs)."""
    _fields_ = [("context", C.c_uint64), ("table", C.c_uint32), ("column", C.c_uint32), ("first", C.c_uint64), ("n", C.c_uint64),
                ("d_cells", C.c_void_p), ("d_spread", C.c_void_p)]


class LookupCounts(C.Structure):
    """hsw_lookup_counts: the caller's per-proof multiplicity tables (hsw_gadget_lookup_multiplicities)."""
    _fields_ = [("d_range", C.c_void_p), ("d_spread", C.c_void_p), ("range_pitch", C.c_uint64), ("spread_pitch", C.c_uint64),
                ("flags", C.c_uint32), ("reserved_", C.c_uint32)]


class LookupReport(C.Structure):
    _fields_ = [("range_entries", C.c_uint64), ("spread_entries", C.c_uint64), ("not_in_table", C.c_uint64),
                ("first_context", C.c_uint64), ("first_entry", C.c_uint64), ("first_table", C.c_uint32), ("first_column", C.c_uint32),
                ("kernel_ms", C.c_float), ("reserved_", C.c_uint32)]


HSW_PERMUTED_GIVEN_M, HSW_PERMUTED_THETA_ON_SPREAD = 1, 2


class LookupPermuted(C.Structure):
    """hsw_lookup_permuted: the A' and S' columns of every argument of one table (hsw_gadget_lookup_permuted)."""
    _fields_ = [("table", C.c_uint32), ("flags", C.c_uint32), ("usable_rows", C.c_uint64), ("n_arguments", C.c_size_t),
                ("d_input_columns", C.POINTER(C.c_void_p)), ("d_table_columns", C.POINTER(C.c_void_p)), ("thetas", C.c_void_p),
                ("d_m", C.c_void_p), ("m_pitch", C.c_uint64)]


class PermutedReport(C.Structure):
    _fields_ = [("arguments", C.c_uint64), ("entries", C.c_uint64), ("written", C.c_uint64), ("not_in_table", C.c_uint64),
                ("first_context", C.c_uint64), ("first_entry", C.c_uint64), ("first_table", C.c_uint32), ("first_column", C.c_uint32),
                ("overflow_arguments", C.c_uint64), ("kernel_ms", C.c_float), ("prepare_ms", C.c_float), ("write_ms", C.c_float),
                ("reserved_", C.c_uint32)]


HSW_PRODUCT_OPEN, HSW_PRODUCT_ZERO_DENOM, HSW_PRODUCT_CELL_NOT_BELOW_P = 1, 2, 4


class LookupProduct(C.Structure):
    """hsw_lookup_product: the grand-product column Z of every argument of one table (hsw_gadget_lookup_product)."""
    _fields_ = [("table", C.c_uint32), ("flags", C.c_uint32), ("usable_rows", C.c_uint64), ("n_arguments", C.c_size_t),
                ("d_inputs", C.POINTER(C.c_void_p)), ("d_inputs_spread", C.POINTER(C.c_void_p)), ("input_rows", C.POINTER(C.c_uint64)),
                ("d_permuted_inputs", C.POINTER(C.c_void_p)), ("d_permuted_tables", C.POINTER(C.c_void_p)),
                ("d_products", C.POINTER(C.c_void_p)), ("thetas", C.c_void_p), ("betas", C.c_void_p), ("gammas", C.c_void_p),
                ("status", C.POINTER(C.c_uint32))]


class ProductReport(C.Structure):
    _fields_ = [("arguments", C.c_uint64), ("written", C.c_uint64), ("open_arguments", C.c_uint64), ("first_open", C.c_uint64),
                ("refused_arguments", C.c_uint64), ("first_refused", C.c_uint64), ("tile_rows", C.c_uint32), ("reserved_", C.c_uint32),
                ("kernel_ms", C.c_float), ("tiles_ms", C.c_float), ("scan_ms", C.c_float), ("write_ms", C.c_float)]


class PermutationProduct(C.Structure):
    """hsw_permutation_product: the permutation argument's grand products of every proof (hsw_gadget_permutation_product)."""
    _fields_ = [("flags", C.c_uint32), ("chunk_columns", C.c_uint32), ("usable_rows", C.c_uint64), ("n_columns", C.c_size_t),
                ("d_columns", C.POINTER(C.c_void_p)), ("column_rows", C.POINTER(C.c_uint64)), ("d_sigmas", C.POINTER(C.c_void_p)),
                ("d_products", C.POINTER(C.c_void_p)), ("betas", C.c_void_p), ("gammas", C.c_void_p), ("omega", C.c_void_p),
                ("delta", C.c_void_p), ("status", C.POINTER(C.c_uint32))]


class PermutationReport(C.Structure):
    _fields_ = [("proofs", C.c_uint64), ("products", C.c_uint64), ("written", C.c_uint64), ("open_proofs", C.c_uint64),
                ("first_open", C.c_uint64), ("refused_proofs", C.c_uint64), ("first_refused", C.c_uint64), ("tile_rows", C.c_uint32),
                ("reserved_", C.c_uint32), ("kernel_ms", C.c_float), ("tiles_ms", C.c_float), ("scan_ms", C.c_float), ("write_ms", C.c_float)]


HSW_NTT_SHIFT_AFTER, HSW_NTT_CELL_NOT_BELOW_P = 1, 4


class Ntt(C.Structure):
    """hsw_ntt: the Fr NTT of device columns (hsw_gadget_ntt)."""
    _fields_ = [("flags", C.c_uint32), ("log_n", C.c_uint32), ("pass_log", C.c_uint32), ("reserved_", C.c_uint32), ("n_columns", C.c_size_t),
                ("d_inputs", C.POINTER(C.c_void_p)), ("input_rows", C.POINTER(C.c_uint64)), ("d_outputs", C.POINTER(C.c_void_p)),
                ("omega", C.c_void_p), ("shift", C.c_void_p), ("scale", C.c_void_p), ("status", C.POINTER(C.c_uint32))]


class NttReport(C.Structure):
    _fields_ = [("columns", C.c_uint64), ("written", C.c_uint64), ("refused_columns", C.c_uint64), ("first_refused", C.c_uint64),
                ("twiddle_bytes", C.c_uint64), ("scratch_bytes", C.c_uint64), ("launches", C.c_uint32), ("pass_log", C.c_uint32),
                ("kernel_ms", C.c_float), ("twiddle_ms", C.c_float)]


HSW_MSM_CELL_NOT_BELOW_P, HSW_MSM_BASE_NOT_BELOW_Q, HSW_MSM_MAX_WINDOW_BITS = 4, 8, 8


class Msm(C.Structure):
    """hsw_msm: the commitments of device columns, the BN254 G1 MSM (hsw_gadget_msm)."""
    _fields_ = [("flags", C.c_uint32), ("window_bits", C.c_uint32), ("slice_rows", C.c_uint32), ("reserved_", C.c_uint32), ("n_columns", C.c_size_t),
                ("n_bases", C.c_uint64), ("d_bases", C.c_void_p), ("d_scalars", C.POINTER(C.c_void_p)), ("input_rows", C.POINTER(C.c_uint64)),
                ("out_points", C.c_void_p), ("status", C.POINTER(C.c_uint32))]


class MsmReport(C.Structure):
    _fields_ = [("columns", C.c_uint64), ("refused_columns", C.c_uint64), ("first_refused", C.c_uint64), ("bad_bases", C.c_uint64),
                ("first_bad_base", C.c_uint64), ("scratch_bytes", C.c_uint64), ("window_bits", C.c_uint32), ("windows", C.c_uint32),
                ("slice_rows", C.c_uint32), ("slices", C.c_uint32), ("launches", C.c_uint32), ("reserved_", C.c_uint32),
                ("kernel_ms", C.c_float), ("finish_ms", C.c_float)]


HSW_OPEN_CELL_NOT_BELOW_P, HSW_OPEN_MIN_TILE_ROWS, HSW_OPEN_THREAD_ROWS = 4, 256, 8


class Evaluate(C.Structure):
    """hsw_evaluate: device columns evaluated at points (hsw_gadget_evaluate)."""
    _fields_ = [("flags", C.c_uint32), ("tile_rows", C.c_uint32), ("rows", C.c_uint64), ("n_columns", C.c_size_t),
                ("d_columns", C.POINTER(C.c_void_p)), ("input_rows", C.POINTER(C.c_uint64)), ("n_points", C.c_size_t), ("points", C.c_void_p),
                ("n_queries", C.c_size_t), ("query_column", C.POINTER(C.c_uint32)), ("query_point", C.POINTER(C.c_uint32)),
                ("out_evals", C.c_void_p), ("status", C.POINTER(C.c_uint32))]


class EvaluateReport(C.Structure):
    _fields_ = [("columns", C.c_uint64), ("queries", C.c_uint64), ("refused_columns", C.c_uint64), ("refused_queries", C.c_uint64),
                ("first_refused", C.c_uint64), ("scratch_bytes", C.c_uint64), ("tile_rows", C.c_uint32), ("tiles", C.c_uint32),
                ("thread_rows", C.c_uint32), ("launches", C.c_uint32), ("kernel_ms", C.c_float), ("reserved_", C.c_uint32)]


class Open(C.Structure):
    """hsw_open: groups of device columns opened at a point each, the quotients of GWC (hsw_gadget_open)."""
    _fields_ = [("flags", C.c_uint32), ("tile_rows", C.c_uint32), ("rows", C.c_uint64), ("n_columns", C.c_size_t),
                ("d_columns", C.POINTER(C.c_void_p)), ("input_rows", C.POINTER(C.c_uint64)), ("n_groups", C.c_size_t),
                ("group_first", C.POINTER(C.c_uint64)), ("group_columns", C.POINTER(C.c_uint32)), ("points", C.c_void_p),
                ("challenges", C.c_void_p), ("d_quotients", C.POINTER(C.c_void_p)), ("out_evals", C.c_void_p), ("status", C.POINTER(C.c_uint32))]


class OpenReport(C.Structure):
    _fields_ = [("groups", C.c_uint64), ("written", C.c_uint64), ("refused_groups", C.c_uint64), ("first_refused", C.c_uint64),
                ("scratch_bytes", C.c_uint64), ("tile_rows", C.c_uint32), ("tiles", C.c_uint32), ("thread_rows", C.c_uint32),
                ("launches", C.c_uint32), ("batches", C.c_uint32), ("reserved_", C.c_uint32), ("kernel_ms", C.c_float), ("reserved2_", C.c_float)]


HSW_SHPLONK_CELL_NOT_BELOW_P, HSW_SHPLONK_MAX_SET_POINTS = 4, 16


class Shplonk(C.Structure):
    """hsw_shplonk: rotation sets of device columns, the arguments of both calls of SHPLONK's multi-point opening
    (hsw_gadget_shplonk_quotient, hsw_gadget_shplonk_open)."""
    _fields_ = [("flags", C.c_uint32), ("tile_rows", C.c_uint32), ("rows", C.c_uint64), ("n_columns", C.c_size_t),
                ("d_columns", C.POINTER(C.c_void_p)), ("input_rows", C.POINTER(C.c_uint64)), ("n_points", C.c_size_t), ("points", C.c_void_p),
                ("n_sets", C.c_size_t), ("set_first", C.POINTER(C.c_uint64)), ("set_columns", C.POINTER(C.c_uint32)),
                ("set_point_first", C.POINTER(C.c_uint64)), ("set_points", C.POINTER(C.c_uint32)), ("y", C.c_void_p), ("v", C.c_void_p),
                ("u", C.c_void_p), ("d_h", C.c_void_p), ("d_out", C.c_void_p), ("status", C.POINTER(C.c_uint32))]


class ShplonkReport(C.Structure):
    _fields_ = [("sets", C.c_uint64), ("items", C.c_uint64), ("columns", C.c_uint64), ("written", C.c_uint64), ("refused", C.c_uint64),
                ("scratch_bytes", C.c_uint64), ("tile_rows", C.c_uint32), ("tiles", C.c_uint32), ("thread_rows", C.c_uint32),
                ("launches", C.c_uint32), ("kernel_ms", C.c_float), ("reserved_", C.c_uint32)]


HSW_QUOTIENT_CELL_NOT_BELOW_P, HSW_QUOTIENT_MAX_FACTORS, HSW_QUOTIENT_MAX_EXTENSION = 4, 8, 8


class QuotientGates(C.Structure):
    """hsw_quotient_gates: the gates as sums of monomials."""
    _fields_ = [("n_gates", C.c_size_t), ("n_terms", C.c_size_t), ("n_factors", C.c_size_t), ("gate_first_term", C.POINTER(C.c_uint32)),
                ("term_coeffs", C.c_void_p), ("term_first_factor", C.POINTER(C.c_uint32)), ("factor_column", C.POINTER(C.c_uint32)),
                ("factor_rotation", C.POINTER(C.c_int32))]


class QuotientLookups(C.Structure):
    """hsw_quotient_lookups: the lookup arguments, their columns folded with theta."""
    _fields_ = [("n_lookups", C.c_size_t), ("first_input", C.POINTER(C.c_uint32)), ("inputs", C.POINTER(C.c_uint32)),
                ("first_table", C.POINTER(C.c_uint32)), ("tables", C.POINTER(C.c_uint32)), ("d_permuted_inputs", C.POINTER(C.c_void_p)),
                ("d_permuted_tables", C.POINTER(C.c_void_p)), ("d_products", C.POINTER(C.c_void_p)), ("thetas", C.c_void_p)]


class Quotient(C.Structure):
    """hsw_quotient: the quotient h(X) of device columns on the extended coset (hsw_gadget_quotient)."""
    _fields_ = [("flags", C.c_uint32), ("log_rows", C.c_uint32), ("log_n", C.c_uint32), ("chunk_columns", C.c_uint32),
                ("usable_rows", C.c_uint64), ("n_proofs", C.c_size_t), ("n_columns", C.c_size_t), ("n_fixed", C.c_size_t),
                ("d_columns", C.POINTER(C.c_void_p)), ("d_fixed", C.POINTER(C.c_void_p)), ("d_l0", C.c_void_p), ("d_l_last", C.c_void_p),
                ("d_l_active", C.c_void_p), ("gates", QuotientGates), ("n_perm_columns", C.c_size_t), ("perm_columns", C.POINTER(C.c_uint32)),
                ("d_sigmas", C.POINTER(C.c_void_p)), ("d_perm_products", C.POINTER(C.c_void_p)), ("lookups", QuotientLookups),
                ("betas", C.c_void_p), ("gammas", C.c_void_p), ("ys", C.c_void_p), ("omega_ext", C.c_void_p), ("zeta", C.c_void_p),
                ("delta", C.c_void_p), ("d_h", C.POINTER(C.c_void_p)), ("status", C.POINTER(C.c_uint32))]


class QuotientReport(C.Structure):
    _fields_ = [("proofs", C.c_uint64), ("written", C.c_uint64), ("refused_proofs", C.c_uint64), ("first_refused", C.c_uint64),
                ("expressions", C.c_uint64), ("scratch_bytes", C.c_uint64), ("launches", C.c_uint32), ("rows_per_thread", C.c_uint32),
                ("kernel_ms", C.c_float), ("gates_ms", C.c_float), ("permutation_ms", C.c_float), ("lookups_ms", C.c_float),
                ("finish_ms", C.c_float)]


# every symbol include/hsw.h declares (tests check the library exports them all)
SYMBOLS = (
    "hsw_shape_query", "hsw_chip_rows", "hsw_engine_create", "hsw_engine_destroy",
    "hsw_engine_shape", "hsw_engine_synchronize", "hsw_witness_blocks", "hsw_sha256_chain",
    "hsw_witness_blocks_host", "hsw_last_kernel_ms", "hsw_set_timing", "hsw_strerror",
    "hsw_last_error", "hsw_abi_version", "hsw_engine_set_option", "hsw_fill_calibrate",
    "hsw_engine_stream", "hsw_digest_prepare", "hsw_gadget_create", "hsw_gadget_destroy",
    "hsw_gadget_digest", "hsw_gadget_digest_batch", "hsw_gadget_streams", "hsw_gadget_input_bytes",
    "hsw_gadget_set_repr", "hsw_download", "hsw_host_alloc", "hsw_host_free",
    "hsw_shape_query_ex", "hsw_engine_create_ex", "hsw_pack_plan_query", "hsw_gate_tape",
    "hsw_witness_blocks_ex", "hsw_spread_table", "hsw_cell_bytes", "hsw_neg_cells",
    "hsw_frame_query", "hsw_frame_tape", "hsw_witness_frames", "hsw_gadget_create_ex",
    "hsw_gadget_set_columns", "hsw_gadget_cell_position", "hsw_gadget_reset", "hsw_gadget_seek", "hsw_gadget_place", "hsw_device_alloc", "hsw_device_free", "hsw_gadget_download_region",
    "hsw_block_structure", "hsw_frame_structure", "hsw_verify_blocks",
    "hsw_verify_frames", "hsw_gadget_verify", "hsw_last_launch", "hsw_witness_digests",
    "hsw_gadget_download_region_compact", "hsw_region_widen", "hsw_gadget_result_cells",
    "hsw_gadget_set_origin", "hsw_gadget_region_tape", "hsw_gadget_download_region_distinct", "hsw_gadget_replay_region",
    "hsw_gadget_context_region", "hsw_gadget_set_digest_origin", "hsw_gadget_create_contexts",
    "hsw_gadget_bind_region", "hsw_gadget_region_binding", "hsw_gadget_bind_columns", "hsw_gadget_bind_column_tables",
    "hsw_gadget_digest_batch_device", "hsw_gadget_digest_levels_device",
    "hsw_gadget_ties", "hsw_gadget_cell_address", "hsw_gadget_verify_ties", "hsw_gadget_verify_equal",
    "hsw_gadget_lookup_runs", "hsw_gadget_lookup_multiplicities", "hsw_gadget_lookup_permuted",
    "hsw_gadget_lookup_product", "hsw_gadget_permutation_product", "hsw_gadget_ntt",
    "hsw_gadget_msm", "hsw_gadget_evaluate", "hsw_gadget_open", "hsw_gadget_quotient",
    "hsw_gadget_shplonk_quotient", "hsw_gadget_shplonk_open",
)


def build(force=False):
    """Compile libhsw.so for gfx950 (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-C", CSRC, "-s", "clean"])
    subprocess.check_call(["make", "-C", CSRC, "-s", "-j8"])
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libhsw.so was not produced by csrc/Makefile")
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libhsw.so is missing: build it with `make -C %s` (hipcc, gfx950). "
            "There is no CPU fallback for the witness engine." % CSRC)
    L = C.CDLL(LIB_PATH)
    vp, u8p, u32p = C.c_void_p, C.c_void_p, C.c_void_p
    L.hsw_abi_version.restype = C.c_uint32
    L.hsw_strerror.restype = C.c_char_p
    L.hsw_strerror.argtypes = [C.c_int]
    L.hsw_last_error.restype = C.c_char_p
    L.hsw_last_error.argtypes = [vp]
    L.hsw_shape_query.restype = C.c_int
    L.hsw_shape_query.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(Shape)]
    L.hsw_chip_rows.restype = C.c_uint64
    L.hsw_chip_rows.argtypes = [C.POINTER(Shape), C.c_uint64, C.c_uint64]
    L.hsw_engine_create.restype = C.c_int
    L.hsw_engine_create.argtypes = [C.c_int, vp, C.c_uint32, C.c_uint32, C.POINTER(vp)]
    L.hsw_engine_destroy.restype = None
    L.hsw_engine_destroy.argtypes = [vp]
    L.hsw_engine_shape.restype = C.c_int
    L.hsw_engine_shape.argtypes = [vp, C.POINTER(Shape)]
    L.hsw_engine_synchronize.restype = C.c_int
    L.hsw_engine_synchronize.argtypes = [vp]
    L.hsw_witness_blocks.restype = C.c_int
    L.hsw_witness_blocks.argtypes = [vp, u8p, u32p, C.c_size_t, C.c_uint64, vp, vp, vp,
                                     C.c_size_t, u32p, C.c_uint32]
    L.hsw_sha256_chain.restype = C.c_int
    L.hsw_sha256_chain.argtypes = [vp, u8p, C.c_size_t, C.c_size_t, u32p, u32p]
    L.hsw_witness_blocks_host.restype = C.c_int
    L.hsw_witness_blocks_host.argtypes = [vp, u8p, u32p, C.c_size_t, C.c_uint64, vp, vp, vp,
                                          C.c_size_t, u32p, C.c_uint32]
    L.hsw_last_kernel_ms.restype = C.c_int
    L.hsw_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
    if hasattr(L, "hsw_engine_set_option"):   # absent only in pre-ABI-1 A/B builds
        L.hsw_engine_set_option.restype = C.c_int
        L.hsw_engine_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
    if hasattr(L, "hsw_fill_calibrate"):
        L.hsw_fill_calibrate.restype = C.c_int
        L.hsw_fill_calibrate.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_float)]
    L.hsw_set_timing.restype = C.c_int
    L.hsw_set_timing.argtypes = [vp, C.c_int]
    if hasattr(L, "hsw_gadget_create"):
        L.hsw_engine_stream.restype = C.c_int
        L.hsw_engine_stream.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int)]
        L.hsw_digest_prepare.restype = C.c_int
        L.hsw_digest_prepare.argtypes = [vp, C.c_size_t, C.c_size_t, C.c_size_t, vp, vp, C.POINTER(DigestInfo)]
        L.hsw_gadget_create.restype = C.c_int
        L.hsw_gadget_create.argtypes = [vp, C.POINTER(C.c_size_t), C.c_size_t, C.c_int, C.POINTER(vp)]
        L.hsw_gadget_destroy.restype = None
        L.hsw_gadget_destroy.argtypes = [vp]
        L.hsw_gadget_digest.restype = C.c_int
        L.hsw_gadget_digest.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.POINTER(HashResult)]
        L.hsw_gadget_digest_batch.restype = C.c_int
        L.hsw_gadget_digest_batch.argtypes = [vp, C.c_size_t, C.POINTER(vp), C.POINTER(C.c_size_t),
                                              C.POINTER(C.c_size_t), C.POINTER(HashResult)]
        L.hsw_gadget_digest_batch_device.restype = C.c_int
        L.hsw_gadget_digest_batch_device.argtypes = [vp, C.c_size_t, C.POINTER(vp), C.POINTER(C.c_size_t),
                                                     C.POINTER(C.c_size_t), C.POINTER(HashResult)]
        L.hsw_gadget_digest_levels_device.restype = C.c_int
        L.hsw_gadget_digest_levels_device.argtypes = [vp, C.c_size_t, C.POINTER(vp), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t),
                                                      C.POINTER(C.c_uint32), C.POINTER(vp), C.POINTER(HashResult)]
        if hasattr(L, "hsw_gadget_ties"):   # absent only in A/B builds of an earlier commit (HSW_LIB_OVERRIDE)
            L.hsw_gadget_ties.restype = C.c_int
            L.hsw_gadget_ties.argtypes = [vp, C.POINTER(CellTie), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)]
            L.hsw_gadget_cell_address.restype = C.c_int
            L.hsw_gadget_cell_address.argtypes = [vp, C.c_uint64, C.POINTER(vp)]
            L.hsw_gadget_verify_ties.restype = C.c_int
            L.hsw_gadget_verify_ties.argtypes = [vp, C.POINTER(TieReport)]
            L.hsw_gadget_verify_equal.restype = C.c_int
            L.hsw_gadget_verify_equal.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(TieReport)]
        if hasattr(L, "hsw_gadget_lookup_runs"):   # absent only in A/B builds of an earlier commit (HSW_LIB_OVERRIDE)
            L.hsw_gadget_lookup_runs.restype = C.c_int
            L.hsw_gadget_lookup_runs.argtypes = [vp, C.POINTER(LookupRun), C.c_size_t, C.POINTER(C.c_size_t)]
            L.hsw_gadget_lookup_multiplicities.restype = C.c_int
            L.hsw_gadget_lookup_multiplicities.argtypes = [vp, C.POINTER(LookupCounts), C.POINTER(LookupReport)]
        if hasattr(L, "hsw_gadget_lookup_permuted"):   # absent only in A/B builds of an earlier commit (HSW_LIB_OVERRIDE)
            L.hsw_gadget_lookup_permuted.restype = C.c_int
            L.hsw_gadget_lookup_permuted.argtypes = [vp, C.POINTER(LookupPermuted), C.POINTER(PermutedReport)]
        if hasattr(L, "hsw_gadget_lookup_product"):    # likewise
            L.hsw_gadget_lookup_product.restype = C.c_int
            L.hsw_gadget_lookup_product.argtypes = [vp, C.POINTER(LookupProduct), C.POINTER(ProductReport)]
        if hasattr(L, "hsw_gadget_permutation_product"):   # likewise
            L.hsw_gadget_permutation_product.restype = C.c_int
            L.hsw_gadget_permutation_product.argtypes = [vp, C.POINTER(PermutationProduct), C.POINTER(PermutationReport)]
        if hasattr(L, "hsw_gadget_ntt"):   # likewise
            L.hsw_gadget_ntt.restype = C.c_int
            L.hsw_gadget_ntt.argtypes = [vp, C.POINTER(Ntt), C.POINTER(NttReport)]
        if hasattr(L, "hsw_gadget_msm"):   # likewise
            L.hsw_gadget_msm.restype = C.c_int
            L.hsw_gadget_msm.argtypes = [vp, C.POINTER(Msm), C.POINTER(MsmReport)]
        if hasattr(L, "hsw_gadget_evaluate"):   # likewise
            L.hsw_gadget_evaluate.restype = C.c_int
            L.hsw_gadget_evaluate.argtypes = [vp, C.POINTER(Evaluate), C.POINTER(EvaluateReport)]
        if hasattr(L, "hsw_gadget_open"):   # likewise
            L.hsw_gadget_open.restype = C.c_int
            L.hsw_gadget_open.argtypes = [vp, C.POINTER(Open), C.POINTER(OpenReport)]
        if hasattr(L, "hsw_gadget_quotient"):   # likewise
            L.hsw_gadget_quotient.restype = C.c_int
            L.hsw_gadget_quotient.argtypes = [vp, C.POINTER(Quotient), C.POINTER(QuotientReport)]
        if hasattr(L, "hsw_gadget_shplonk_quotient"):   # likewise
            L.hsw_gadget_shplonk_quotient.restype = C.c_int
            L.hsw_gadget_shplonk_quotient.argtypes = [vp, C.POINTER(Shplonk), C.POINTER(ShplonkReport)]
            L.hsw_gadget_shplonk_open.restype = C.c_int
            L.hsw_gadget_shplonk_open.argtypes = [vp, C.POINTER(Shplonk), C.POINTER(ShplonkReport)]
        L.hsw_gadget_streams.restype = C.c_int
        L.hsw_gadget_streams.argtypes = [vp, C.POINTER(GadgetView)]
        L.hsw_gadget_input_bytes.restype = C.c_int
        L.hsw_gadget_input_bytes.argtypes = [vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.hsw_shape_query_ex.restype = C.c_int
        L.hsw_shape_query_ex.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(Shape)]
        L.hsw_engine_create_ex.restype = C.c_int
        L.hsw_engine_create_ex.argtypes = [C.c_int, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(vp)]
        L.hsw_pack_plan_query.restype = C.c_int
        L.hsw_pack_plan_query.argtypes = [C.POINTER(Shape), C.c_size_t, C.c_uint64, C.c_uint64, C.POINTER(PackPlan)]
        L.hsw_gate_tape.restype = C.c_int
        L.hsw_gate_tape.argtypes = [C.POINTER(Shape), vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.hsw_witness_blocks_ex.restype = C.c_int
        L.hsw_witness_blocks_ex.argtypes = [vp, C.POINTER(WitnessArgs)]
        L.hsw_cell_bytes.restype = C.c_uint32
        L.hsw_cell_bytes.argtypes = [C.c_uint32]
        L.hsw_neg_cells.restype = C.c_int
        L.hsw_neg_cells.argtypes = [C.POINTER(Shape), vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.hsw_spread_table.restype = C.c_int
        L.hsw_spread_table.argtypes = [C.c_uint32, vp, vp]
        L.hsw_host_alloc.restype = C.c_int
        L.hsw_host_alloc.argtypes = [C.c_size_t, C.POINTER(vp)]
        L.hsw_host_free.restype = None
        L.hsw_host_free.argtypes = [vp]
        L.hsw_download.restype = C.c_int
        L.hsw_download.argtypes = [vp, vp, vp, C.c_size_t]
        L.hsw_gadget_set_repr.restype = C.c_int
        L.hsw_gadget_set_repr.argtypes = [vp, C.c_uint32]
        L.hsw_frame_query.restype = C.c_int
        L.hsw_frame_query.argtypes = [C.POINTER(Shape), C.c_size_t, C.c_int, C.POINTER(FrameShape)]
        L.hsw_frame_tape.restype = C.c_int
        L.hsw_frame_tape.argtypes = [C.POINTER(Shape), C.c_size_t, C.c_int, C.c_int, vp, C.c_size_t,
                                     C.POINTER(C.c_size_t)]
        L.hsw_witness_frames.restype = C.c_int
        L.hsw_witness_frames.argtypes = [vp, C.POINTER(FrameDesc), C.c_size_t, vp, vp, vp, vp, vp,
                                         C.POINTER(PackPlan), C.c_uint32]
        L.hsw_gadget_set_columns.restype = C.c_int
        L.hsw_gadget_set_columns.argtypes = [vp, C.c_uint64, C.POINTER(C.c_uint64)]
        L.hsw_gadget_region_tape.restype = C.c_int
        L.hsw_gadget_region_tape.argtypes = [vp, C.POINTER(RegionTape)]
        L.hsw_gadget_download_region_distinct.restype = C.c_int
        L.hsw_gadget_download_region_distinct.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.hsw_gadget_replay_region.restype = C.c_int
        L.hsw_gadget_replay_region.argtypes = [vp, vp, C.POINTER(RegionHost), C.c_uint]
        L.hsw_gadget_set_origin.restype = C.c_int
        L.hsw_gadget_set_origin.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_int, C.c_uint64]
        L.hsw_verify_frames.restype = C.c_int
        L.hsw_verify_frames.argtypes = [vp, C.POINTER(FrameDesc), C.c_size_t, vp, vp, vp, vp, vp, C.POINTER(PackPlan),
                                        C.c_uint32, C.POINTER(VerifyReport)]
        L.hsw_gadget_verify.restype = C.c_int
        L.hsw_gadget_verify.argtypes = [vp, C.POINTER(VerifyReport)]
        L.hsw_verify_blocks.restype = C.c_int
        L.hsw_verify_blocks.argtypes = [vp, C.POINTER(WitnessArgs), C.POINTER(VerifyReport)]
        L.hsw_frame_structure.restype = C.c_int
        L.hsw_frame_structure.argtypes = [C.POINTER(Shape), C.c_size_t, C.c_int, C.c_int,
                                          C.POINTER(FrameStructureCounts)] + [vp] * 7
        L.hsw_block_structure.restype = C.c_int
        L.hsw_block_structure.argtypes = [C.POINTER(Shape), C.POINTER(StructureCounts)] + [vp] * 8
        L.hsw_gadget_download_region.restype = C.c_int
        L.hsw_gadget_download_region.argtypes = [vp, C.POINTER(RegionHost)]
        L.hsw_gadget_seek.restype = C.c_int
        L.hsw_gadget_seek.argtypes = [vp, C.c_size_t]
        L.hsw_device_alloc.restype = C.c_int
        L.hsw_device_alloc.argtypes = [C.c_int, C.c_size_t, C.c_size_t, C.POINTER(C.c_void_p)]
        L.hsw_device_free.restype = C.c_int
        L.hsw_device_free.argtypes = [vp]
        L.hsw_gadget_place.restype = C.c_int
        L.hsw_gadget_place.argtypes = [vp, C.c_uint, C.POINTER(C.c_float), C.POINTER(C.c_uint)]
        L.hsw_gadget_reset.restype = C.c_int
        L.hsw_gadget_reset.argtypes = [vp]
        L.hsw_gadget_cell_position.restype = C.c_int
        L.hsw_gadget_cell_position.argtypes = [vp, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.hsw_gadget_set_digest_origin.restype = C.c_int
        L.hsw_gadget_set_digest_origin.argtypes = [vp, C.c_size_t, C.c_uint64, C.c_uint64, C.c_uint64]
        L.hsw_gadget_context_region.restype = C.c_int
        L.hsw_gadget_context_region.argtypes = [vp, C.c_size_t, C.POINTER(ContextRegion)]
        L.hsw_gadget_bind_region.restype = C.c_int
        L.hsw_gadget_bind_region.argtypes = [vp, C.POINTER(RegionBinding)]
        L.hsw_gadget_bind_columns.restype = C.c_int
        L.hsw_gadget_bind_columns.argtypes = [vp, C.POINTER(RegionBinding), C.POINTER(C.c_void_p), C.c_size_t]
        L.hsw_gadget_bind_column_tables.restype = C.c_int
        L.hsw_gadget_bind_column_tables.argtypes = [vp, C.POINTER(RegionBinding), C.POINTER(ColumnTables)]
        L.hsw_gadget_region_binding.restype = C.c_int
        L.hsw_gadget_region_binding.argtypes = [vp, C.POINTER(RegionBinding)]
        L.hsw_gadget_create_contexts.restype = C.c_int
        L.hsw_gadget_create_contexts.argtypes = [vp, C.POINTER(C.c_size_t), C.c_size_t, C.c_size_t, C.c_int, C.c_uint32,
                                                 C.POINTER(vp)]
        L.hsw_gadget_create_ex.restype = C.c_int
        L.hsw_gadget_create_ex.argtypes = [vp, C.POINTER(C.c_size_t), C.c_size_t, C.c_int, C.c_uint32,
                                           C.POINTER(vp)]
        L.hsw_last_launch.restype = C.c_int
        L.hsw_last_launch.argtypes = [vp, C.POINTER(LaunchInfo)]
        L.hsw_witness_digests.restype = C.c_int
        L.hsw_witness_digests.argtypes = [vp, C.POINTER(DigestsArgs)]
        L.hsw_gadget_download_region_compact.restype = C.c_int
        L.hsw_gadget_download_region_compact.argtypes = [vp, C.POINTER(RegionCompact)]
        L.hsw_gadget_result_cells.restype = C.c_int
        L.hsw_gadget_result_cells.argtypes = [vp, C.c_size_t, C.POINTER(ResultCells)]
        L.hsw_region_widen.restype = C.c_int
        L.hsw_region_widen.argtypes = [vp, C.c_size_t, C.c_uint64, vp, C.c_size_t, vp]
    _lib = L
    return L


class HswError(RuntimeError):
    def __init__(self, status, detail=""):
        self.status = status
        msg = lib().hsw_strerror(status).decode()
        super().__init__("hsw status %d (%s)%s" % (status, msg, (": " + detail) if detail else ""))


def digest_prepare(message: bytes, max_variable_byte_size: int, precomputed_input_len: int = 0):
    """Host-only lib.rs:77-160: returns (blocks bytes, init_state list, DigestInfo dict)."""
    import numpy as np
    msg = bytes(message)
    buf = (C.c_uint8 * max(len(msg), 1)).from_buffer_copy(msg if msg else b"\0")
    blocks = np.zeros(max(max_variable_byte_size, 1), dtype=np.uint8)
    init = np.zeros(8, dtype=np.uint32)
    info = DigestInfo()
    rc = lib().hsw_digest_prepare(C.addressof(buf) if msg else None, len(msg), precomputed_input_len,
                                  max_variable_byte_size, blocks.ctypes.data, init.ctypes.data, C.byref(info))
    if rc != HSW_OK:
        raise HswError(rc)
    return blocks[:max_variable_byte_size], init, {k: int(getattr(info, k)) for k, _ in DigestInfo._fields_}


def shape_query(num_bits_lookup=8, num_advice_columns=2, mode=HSW_MODE_DEFAULT):
    s = Shape()
    rc = lib().hsw_shape_query_ex(num_bits_lookup, num_advice_columns, mode, C.byref(s))
    if rc != HSW_OK:
        raise HswError(rc)
    return s


def spread_table(num_bits_lookup=8):
    """SpreadConfig::load rows (spread.rs:165-194) as two numpy uint64 arrays."""
    import numpy as np
    n = 1 << num_bits_lookup
    d, s = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    rc = lib().hsw_spread_table(num_bits_lookup, d.ctypes.data, s.ctypes.data)
    if rc != HSW_OK:
        raise HswError(rc)
    return d, s


def neg_cells(shape):
    """Block-relative gate cells holding field negations (hsw_neg_cells), numpy uint32."""
    import numpy as np
    out = np.zeros(256, dtype=np.uint32)
    n = C.c_size_t()
    rc = lib().hsw_neg_cells(C.byref(shape), out.ctypes.data, 256, C.byref(n))
    if rc != HSW_OK:
        raise HswError(rc)
    return out[: n.value]


def gate_tape(shape):
    """assign_region call lengths of one block (numpy uint8), hsw_gate_tape."""
    import numpy as np
    n = C.c_size_t()
    rc = lib().hsw_gate_tape(C.byref(shape), None, 0, C.byref(n))
    if rc != HSW_OK:
        raise HswError(rc)
    lens = np.zeros(n.value, dtype=np.uint8)
    rc = lib().hsw_gate_tape(C.byref(shape), lens.ctypes.data, lens.size, None)
    if rc != HSW_OK:
        raise HswError(rc)
    return lens


def pack_plan(shape, n_blocks, start_row, max_rows):
    p = PackPlan()
    rc = lib().hsw_pack_plan_query(C.byref(shape), n_blocks, start_row, max_rows, C.byref(p))
    if rc != HSW_OK:
        raise HswError(rc)
    return p


def frame_query(shape, max_variable_byte_size, is_input_range_check=False):
    """hsw_frame_query: cell counts of the digest frame."""
    fs = FrameShape()
    rc = lib().hsw_frame_query(C.byref(shape), max_variable_byte_size, 1 if is_input_range_check else 0, C.byref(fs))
    if rc != HSW_OK:
        raise HswError(rc)
    return fs


def frame_tape(shape, max_variable_byte_size, is_input_range_check, section):
    """assign_region call lengths of the prologue (section 0) / epilogue (1), numpy uint8."""
    import numpy as np
    n = C.c_size_t()
    rc = lib().hsw_frame_tape(C.byref(shape), max_variable_byte_size, 1 if is_input_range_check else 0, section,
                              None, 0, C.byref(n))
    if rc != HSW_OK:
        raise HswError(rc)
    lens = np.zeros(n.value, dtype=np.uint8)
    rc = lib().hsw_frame_tape(C.byref(shape), max_variable_byte_size, 1 if is_input_range_check else 0, section,
                              lens.ctypes.data, lens.size, None)
    if rc != HSW_OK:
        raise HswError(rc)
    return lens


def block_structure(shape):
    """hsw_block_structure as a dict of numpy arrays: kind (G,) u8, ref (G,) i64, gate_rows (n,) u32,
    assert_eq (n,2), range (n,2), lookup_src (LK,), chip (LC,2), next_state (8,) -- all i64 cell ids."""
    import numpy as np
    c = StructureCounts()
    rc = lib().hsw_block_structure(C.byref(shape), C.byref(c), None, None, None, None, None, None, None, None)
    if rc != HSW_OK:
        raise HswError(rc)
    kind = np.zeros(c.gate_cells, dtype=np.uint8)
    ref = np.zeros(c.gate_cells, dtype=np.int64)
    rows = np.zeros(c.gate_rows, dtype=np.uint32)
    aeq = np.zeros((c.assert_eq, 2), dtype=np.int64)
    rng = np.zeros((c.ranges, 2), dtype=np.int64)
    lk = np.zeros(c.lookups, dtype=np.int64)
    chip = np.zeros((c.limb_calls, 2), dtype=np.int64)
    ns = np.zeros(8, dtype=np.int64)
    rc = lib().hsw_block_structure(C.byref(shape), None, kind.ctypes.data, ref.ctypes.data, rows.ctypes.data,
                                   aeq.ctypes.data, rng.ctypes.data, lk.ctypes.data, chip.ctypes.data, ns.ctypes.data)
    if rc != HSW_OK:
        raise HswError(rc)
    return dict(kind=kind, ref=ref, gate_rows=rows, assert_eq=aeq, range=rng, lookup_src=lk, chip=chip, next_state=ns)


def frame_structure(shape, max_variable_byte_size, is_input_range_check, section):
    """hsw_frame_structure as a dict of numpy arrays (section 0 = prologue, 1 = epilogue)."""
    import numpy as np
    c = FrameStructureCounts()
    args = (C.byref(shape), max_variable_byte_size, 1 if is_input_range_check else 0, section)
    rc = lib().hsw_frame_structure(*args, C.byref(c), None, None, None, None, None, None, None)
    if rc != HSW_OK:
        raise HswError(rc)
    kind = np.zeros(c.cells, dtype=np.uint8)
    ref = np.zeros(c.cells, dtype=np.int64)
    rows = np.zeros(c.gate_rows, dtype=np.uint32)
    aeq = np.zeros((c.assert_eq, 2), dtype=np.int64)
    ac = np.zeros((c.assert_const, 2), dtype=np.int64)
    rng = np.zeros((c.ranges, 2), dtype=np.int64)
    lk = np.zeros(c.lookups, dtype=np.int64)
    rc = lib().hsw_frame_structure(*args, None, kind.ctypes.data, ref.ctypes.data, rows.ctypes.data, aeq.ctypes.data,
                                   ac.ctypes.data, rng.ctypes.data, lk.ctypes.data)
    if rc != HSW_OK:
        raise HswError(rc)
    return dict(kind=kind, ref=ref, gate_rows=rows, assert_eq=aeq, assert_const=ac, range=rng, lookup_src=lk)
