"""ctypes binding of ``librsqp_hip.so`` (the C ABI declared in ``include/rsqp_hip.h``).

This is the only way Python reaches the engine: no CPU fallback exists. Loading fails loudly
when the library has not been built (``__graft_entry__.build()`` / ``restartsqp_amd.build``),
and every call that needs a GPU returns ``RSQP_ERR_DEVICE`` -> ``RsqpError`` without one.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RSQP_LIB") or os.path.join(_HERE, "lib", "librsqp_hip.so")   # RSQP_LIB: tuning builds (tools/)

OK = 0
ERR_ARG, ERR_DEVICE, ERR_TOO_LARGE, ERR_WORKING_SET = -1, -2, -3, -4
VEC_G, VEC_LB, VEC_UB, VEC_LBA, VEC_UBA = range(5)
HU_SET, HU_BOUNDS, HU_DELTA, HU_PENALTY, HU_GRAD, HU_UBA = 1, 2, 4, 8, 16, 32   # RSQP_HU_*: the words of Batch.handler_update
HM_JAC, HM_HESS = 1, 2                                                          # RSQP_HM_*: the words of Batch.handler_set_matrices
MODE_COLD, MODE_HOT_VECTORS, MODE_HOT_MATRICES, MODE_WARM_REINIT = range(4)
QP_OPTIMAL, QPERROR_INFEASIBLE, QPERROR_UNBOUNDED = 20, 22, 23
ACTIVE_ABOVE, ACTIVE_BELOW, ACTIVE_BOTH_SIDE, INACTIVE = 1, -1, -99, 0

ip = C.POINTER(C.c_int)
dp = C.POINTER(C.c_double)

# every exported symbol of include/rsqp_hip.h: name -> (restype, argtypes)
fp = C.POINTER(C.c_float)
SYMBOLS = {
    "rsqp_dense_gemm": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_double), C.c_int,
                                  C.POINTER(C.c_double), C.c_int, C.c_double, C.POINTER(C.c_double), C.c_int, C.c_int, fp]),
    "rsqp_dense_qr": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                C.c_double, C.POINTER(C.c_int), fp]),
    "rsqp_dense_chol_inverse": (C.c_int, [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.c_double,
                                          C.POINTER(C.c_int), fp]),
    "rsqp_version": (C.c_char_p, []),
    "rsqp_build_hash": (C.c_char_p, []),
    "rsqp_device_count": (C.c_int, []),
    "rsqp_last_error": (C.c_char_p, []),
    "rsqp_create": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "rsqp_destroy": (None, [C.c_void_p]),
    "rsqp_set_options": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "rsqp_set_reinit_guess": (C.c_int, [C.c_void_p, C.c_int]),
    "rsqp_get_last_mode": (C.c_int, [C.c_void_p]),
    "rsqp_get_large_path": (C.c_int, [C.c_void_p]),
    "rsqp_get_nV": (C.c_int, [C.c_void_p]),
    "rsqp_get_nC": (C.c_int, [C.c_void_p]),
    "rsqp_write_qp_dump": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, dp, dp, dp, dp, dp, ip, ip, dp, ip, ip, dp]),
    "rsqp_write_qp_data": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "rsqp_read_qore_dump_sizes": (C.c_int, [C.c_char_p, ip, ip, ip, ip]),
    "rsqp_read_qore_dump": (C.c_int, [C.c_char_p, dp, dp, dp, dp, dp, ip, ip, dp, ip, ip, dp]),
    "rsqp_set_engine_profiling": (C.c_int, [C.c_void_p, C.c_int]),
    "rsqp_get_engine_profile": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "rsqp_engine_profile_names": (C.c_int, [C.c_void_p, C.c_int]),
    "rsqp_get_setup_profile": (C.c_int, [C.c_void_p, dp]),
    "rsqp_get_structure_seconds": (C.c_double, [C.c_void_p, C.c_int]),
    "rsqp_set_engine": (C.c_int, [C.c_void_p, C.c_int]),
    "rsqp_get_engine": (C.c_int, [C.c_void_p]),
    "rsqp_set_A_triplet": (C.c_int, [C.c_void_p, C.c_int, ip, ip, dp, C.c_int, ip, ip, ip, dp]),
    "rsqp_set_H_triplet": (C.c_int, [C.c_void_p, C.c_int, ip, ip, dp, C.c_int]),
    "rsqp_set_A_csc": (C.c_int, [C.c_void_p, ip, ip, dp]),
    "rsqp_set_H_csc": (C.c_int, [C.c_void_p, ip, ip, dp]),
    "rsqp_get_A_nnz": (C.c_int, [C.c_void_p]),
    "rsqp_get_H_nnz": (C.c_int, [C.c_void_p]),
    "rsqp_get_A_csc": (C.c_int, [C.c_void_p, ip, ip, dp, ip]),
    "rsqp_get_H_csc": (C.c_int, [C.c_void_p, ip, ip, dp, ip]),
    "rsqp_set_vector": (C.c_int, [C.c_void_p, C.c_int, dp]),
    "rsqp_set_entry": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double]),
    "rsqp_get_vector": (C.c_int, [C.c_void_p, C.c_int, dp]),
    "rsqp_reset_constraints": (C.c_int, [C.c_void_p]),
    "rsqp_optimize_qp": (C.c_int, [C.c_void_p, ip]),
    "rsqp_optimize_lp": (C.c_int, [C.c_void_p, ip]),
    "rsqp_solve": (C.c_int, [C.c_void_p, C.c_int, ip, dp, dp, ip]),
    "rsqp_get_primal": (C.c_int, [C.c_void_p, dp]),
    "rsqp_get_dual": (C.c_int, [C.c_void_p, dp]),
    "rsqp_get_objective": (C.c_double, [C.c_void_p]),
    "rsqp_get_status": (C.c_int, [C.c_void_p]),
    "rsqp_is_solved": (C.c_int, [C.c_void_p]),
    "rsqp_get_working_set_raw": (C.c_int, [C.c_void_p, ip, ip]),
    "rsqp_get_working_set": (C.c_int, [C.c_void_p, ip, ip]),
    "rsqp_test_optimality": (C.c_int, [C.c_void_p, ip, ip, C.c_void_p]),
    "rsqp_A_times": (C.c_int, [C.c_void_p, dp, dp]),
    "rsqp_A_transposed_times": (C.c_int, [C.c_void_p, dp, dp]),
    "rsqp_H_times": (C.c_int, [C.c_void_p, dp, dp]),
    "rsqp_batch_create": (C.c_int, [C.c_int, ip, ip, ip, ip, dp, ip, ip, dp, C.c_int, C.POINTER(C.c_void_p)]),
    "rsqp_batch_destroy": (None, [C.c_void_p]),
    "rsqp_batch_set_vectors": (C.c_int, [C.c_void_p, dp, dp, dp, dp, dp]),
    "rsqp_batch_set_matrix_values": (C.c_int, [C.c_void_p, dp, dp]),
    "rsqp_batch_set_warm_start": (C.c_int, [C.c_void_p, dp, dp, ip]),
    "rsqp_batch_set_options": (C.c_int, [C.c_void_p, C.c_int]),
    "rsqp_batch_solve": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "rsqp_batch_optimize_qp": (C.c_int, [C.c_void_p, ip]),
    "rsqp_batch_set_lp_options": (C.c_int, [C.c_void_p, C.c_int]),
    "rsqp_batch_optimize_lp": (C.c_int, [C.c_void_p, ip]),
    "rsqp_batch_get_dispatch": (C.c_int, [C.c_void_p, ip, ip]),
    "rsqp_batch_set_members": (C.c_int, [C.c_void_p, ip]),
    "rsqp_batch_set_matrix_values_of": (C.c_int, [C.c_void_p, ip, dp, dp]),
    "rsqp_batch_set_vectors_of": (C.c_int, [C.c_void_p, ip, dp, dp, dp, dp, dp]),
    "rsqp_batch_handler_set_problem": (C.c_int, [C.c_void_p, dp, dp, dp, dp]),
    "rsqp_batch_handler_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "rsqp_batch_handler_get_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "rsqp_batch_get_vectors": (C.c_int, [C.c_void_p, dp, dp, dp, dp, dp]),
    "rsqp_batch_handler_set_matrices": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "rsqp_batch_get_matrix_values": (C.c_int, [C.c_void_p, dp, dp]),
    "rsqp_batch_sync": (C.c_int, [C.c_void_p]),
    "rsqp_batch_set_keep_state": (C.c_int, [C.c_void_p, C.c_int]),
    "rsqp_batch_get_last_kernel": (C.c_int, [C.c_void_p]),
    "rsqp_batch_get_lane_hblock": (C.c_int, [C.c_void_p]),
    "rsqp_describe_small_launch": (C.c_int, [ip, C.c_int, ip, C.c_int]),
    "rsqp_batch_get_last_plan": (C.c_int, [C.c_void_p, ip, C.c_int]),
    "rsqp_batch_last_solve_ms": (C.c_float, [C.c_void_p]),
    "rsqp_batch_timer_start": (C.c_int, [C.c_void_p]),
    "rsqp_batch_timer_stop_ms": (C.c_float, [C.c_void_p]),
    "rsqp_batch_get_results": (C.c_int, [C.c_void_p, dp, dp, ip, ip, ip, ip, dp]),
    "rsqp_batch_set_results": (C.c_int, [C.c_void_p, dp, dp, ip, ip]),
    "rsqp_batch_test_optimality": (C.c_int, [C.c_void_p, C.c_void_p, ip]),
    "rsqp_batch_get_working_set": (C.c_int, [C.c_void_p, ip, ip]),
    "rsqp_batch_record_stride": (C.c_int, [C.c_void_p]),
    "rsqp_batch_pack_records_dev": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rsqp_batch_pack_records_host": (C.c_int, [C.c_void_p, dp]),
    "rsqp_shard_range": (C.c_int, [C.c_int, C.c_int, C.c_int, ip, ip]),
    "rsqp_balanced_shard": (C.c_int, [C.c_int, ip, ip, C.c_int, C.c_int, ip, ip]),
    "rsqp_rccl_unique_id": (C.c_int, [C.c_char_p]),
    "rsqp_rccl_comm_create": (C.c_int, [C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "rsqp_rccl_comm_destroy": (C.c_int, [C.c_void_p]),
    "rsqp_rccl_broadcast_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_void_p]),
    "rsqp_batch_allgather_records": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "rsqp_time_value_refresh": (C.c_int, [C.c_void_p, C.c_int, fp, fp]),
    "rsqp_time_value_refresh_fused": (C.c_int, [C.c_void_p, C.c_int, fp]),
    "rsqp_time_large_kernel": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, fp]),
    "rsqp_spmv_plan_create": (C.c_int, [C.c_int, C.c_int, ip, ip, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "rsqp_spmv_plan_destroy": (None, [C.c_void_p]),
    "rsqp_spmv_plan_upload": (C.c_int, [C.c_void_p, dp, dp, C.c_int]),
    "rsqp_spmv_plan_run": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float)]),
    "rsqp_spmv_plan_download": (C.c_int, [C.c_void_p, dp, C.c_int]),
    "rsqp_spmv_plan_variant": (C.c_int, [C.c_void_p, C.c_int, ip]),
}


# ... of its extension include/rsqp_hip_lane.h (which build of the lane-per-problem kernel a batch's last launch took)
LANE_SYMBOLS = {
    "rsqp_batch_get_lane_shape": (C.c_int, [C.c_void_p]),
}
# ... and of its extension include/rsqp_hip_handover.h (the hand-over switch of a batch), bound by lib() like the table above
HANDOVER_SYMBOLS = {
    "rsqp_batch_set_handover": (C.c_int, [C.c_void_p, C.c_int]),
    "rsqp_batch_get_handover": (C.c_int, [C.c_void_p, ip, ip]),
}
# ... and of include/rsqp_hip_lane_warm.h (hot starts with new matrices / warm re-initialisations on the lane-per-problem kernel)
LANE_WARM_SYMBOLS = {
    "rsqp_batch_set_lane_warm": (C.c_int, [C.c_void_p, C.c_int]),
    "rsqp_batch_get_lane_warm": (C.c_int, [C.c_void_p]),
}
# ... and of include/rsqp_hip_lane_hot.h (hot starts on new vectors on the lane-per-problem kernel)
LANE_HOT_SYMBOLS = {
    "rsqp_batch_set_lane_hot": (C.c_int, [C.c_void_p, C.c_int]),
    "rsqp_batch_get_lane_hot": (C.c_int, [C.c_void_p]),
}
# ... and of include/rsqp_hip_dense_check.h (the dense building blocks called the way the engine calls them; the GEMM's launch plan)
_ll = C.c_longlong
_buf = [dp, _ll, _ll, _ll]      # a whole host buffer: pointer, length, offset and leading dimension of the operand inside it
DENSE_CHECK_SYMBOLS = {
    "rsqp_dense_describe_gemm": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ll, ip, C.c_int]),
    "rsqp_dense_check_gemm": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double] + 3 * _buf + [_ll]),
    "rsqp_dense_check_work_create": (C.c_int, [_ll, C.POINTER(C.c_void_p)]),
    "rsqp_dense_check_work_destroy": (C.c_int, [C.c_void_p]),
    "rsqp_dense_check_qr": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double] + 3 * _buf + [ip, ip]),
    "rsqp_dense_check_chol": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double] + 3 * _buf + [ip]),
}
# ... and of include/rsqp_hip_nlp_step.h (the decisions of a lock-step SQP loop per member: infeasibility, ratio test, NLP KKT check)
NLP_STEP_SYMBOLS = {
    "rsqp_nlp_step_default_options": (C.c_int, [C.c_void_p]),
    "rsqp_batch_handler_infeasibility": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "rsqp_batch_handler_ratio_test": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "rsqp_batch_handler_check_optimality": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
}
# ... and of include/rsqp_hip_penalty.h (update_penalty_parameter per member of a QP batch and the LP batch paired with it)
PENALTY_SYMBOLS = {
    "rsqp_penalty_default_options": (C.c_int, [C.c_void_p]),
    "rsqp_batch_handler_pair_lp": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rsqp_batch_handler_update_penalty": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
}
# ... and of include/rsqp_hip_band_check.h (the banded H^-1 operator of the HBM-resident engine called the way the engine calls it)
_vec = [dp, _ll, _ll]           # a whole host buffer holding one vector (or the columns of a matrix): pointer, length, offset
BAND_CHECK_SYMBOLS = {
    "rsqp_band_check_factor": (C.c_int, [C.c_int, dp, dp, dp, ip, ip, ip, dp, dp, _ll, dp, _ll, dp, _ll]),
    "rsqp_band_check_create": (C.c_int, [C.c_int, dp, dp, dp, C.POINTER(C.c_void_p)]),
    "rsqp_band_check_destroy": (C.c_int, [C.c_void_p]),
    "rsqp_band_check_apply": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _ll, C.c_int] + 3 * _vec + [ip, C.POINTER(_ll)]),
    "rsqp_band_check_apply_q": (C.c_int, [C.c_void_p, C.c_int, ip, dp, dp, dp, dp] + 2 * _vec + [ip, C.POINTER(_ll)]),
}
BAND_KERNEL_ENGINE, BAND_KERNEL_1WG = 0, 1                                                              # RSQP_BAND_KERNEL_*
BAND_MAX_N, BAND_THREADS = 16384, 1024                                                                  # RSQP_BAND_MAX_N, _THREADS
# ... and of include/rsqp_hip_soc.h (second_order_correction per member of a batch, and the setter of the objective pool)
SOC_SYMBOLS = {
    "rsqp_soc_default_options": (C.c_int, [C.c_void_p]),
    "rsqp_batch_handler_soc_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "rsqp_batch_handler_soc_end": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "rsqp_batch_set_objective": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
}
# every table above by the header under include/ that declares its entry points: lib() binds them all, and a name stands in one table only
SYMBOL_TABLES = {"rsqp_hip.h": SYMBOLS, "rsqp_hip_lane.h": LANE_SYMBOLS, "rsqp_hip_handover.h": HANDOVER_SYMBOLS,
                 "rsqp_hip_lane_warm.h": LANE_WARM_SYMBOLS, "rsqp_hip_lane_hot.h": LANE_HOT_SYMBOLS,
                 "rsqp_hip_dense_check.h": DENSE_CHECK_SYMBOLS, "rsqp_hip_nlp_step.h": NLP_STEP_SYMBOLS,
                 "rsqp_hip_penalty.h": PENALTY_SYMBOLS, "rsqp_hip_band_check.h": BAND_CHECK_SYMBOLS, "rsqp_hip_soc.h": SOC_SYMBOLS}
SOC_TEST, SOC_CORRECT = 1, 2                                                                             # RSQP_SOC_*: bits of what[q]
EXIT_UNKNOWN, EXIT_TRUST_REGION_TOO_SMALL = -99, 4                                                      # RSQP_EXIT_*
KKT_PRIMAL, KKT_DUAL, KKT_COMPL, KKT_STAT, KKT_FIRST_ORDER_OPT = 1, 2, 4, 8, 16                         # RSQP_KKT_*: the verdict bits
DENSE_GEMM_PLAIN, DENSE_GEMM_UPPER, DENSE_GEMM_KTRI1, DENSE_GEMM_KTRI2, DENSE_GEMM_KTRI3 = range(5)      # RSQP_DENSE_GEMM_*
DENSE_INV_UPPER, DENSE_INV_MIRROR, DENSE_INV_TRI2 = range(3)                                            # RSQP_DENSE_INV_*
DENSE_PLAN_OUT = ("TM", "TN", "splits", "kc", "skinny")                                                 # the words of rsqp_dense_describe_gemm


class OptimalityStatus(C.Structure):
    _fields_ = [("primal_violation", C.c_double), ("dual_violation", C.c_double),
                ("compl_violation", C.c_double), ("stationarity_violation", C.c_double),
                ("KKT_error", C.c_double)]


def _pointer_struct(rows):
    """(_fields_, IN, INOUT, OUT, INTS) of a struct of host or device addresses of pooled arguments from its table, one row per field
    in the header's order: (name, role "in" / "inout" / "out", length "nq" / "sN" (NLP layout) / "sC" (constraint layout), element
    type "float64" / "int32"). A call converts its "in" arrays and writes the others in place (Batch._pooled)"""
    names = lambda test: tuple(r[0] for r in rows if test(r))
    return ([(r[0], C.c_void_p) for r in rows], names(lambda r: r[1] == "in"), names(lambda r: r[1] == "inout"),
            names(lambda r: r[1] == "out"), names(lambda r: r[3] == "int32"))


class HandlerIterate(C.Structure):
    """rsqp_handler_iterate: host or device addresses, as handler_update's on_device says"""
    ROWS = (("what", "in", "nq", "int32"), ("delta", "in", "nq", "float64"), ("rho", "in", "nq", "float64"), ("x_k", "in", "sN", "float64"),
            ("grad", "in", "sN", "float64"), ("c_k", "in", "sC", "float64"))
    _fields_, IN, INOUT, OUT, INTS = _pointer_struct(ROWS)


class _Options(C.Structure):
    """the option structs: a new one holds the library's defaults (the entry point DEFAULTS names), keyword arguments override
    fields of the C struct C_NAME"""

    def __init__(self, **fields):
        super().__init__()
        check(getattr(lib(), self.DEFAULTS)(C.addressof(self)))
        for k, v in fields.items():
            if k not in dict(self._fields_):
                raise TypeError("%s has no field %r" % (self.C_NAME, k))
            setattr(self, k, v)

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class NlpStepOptions(_Options):
    """rsqp_nlp_step_options: the defaults of src/Options.cpp:28-42"""
    _fields_ = [(k, C.c_double) for k in ("active_set_tol", "opt_prim_fea_tol", "opt_dual_fea_tol", "opt_compl_tol", "opt_stat_tol",
                                          "eta_s", "eta_c", "eta_e", "gamma_c", "gamma_e", "delta_min", "delta_max", "tol")] + \
               [("refresh_ubA", C.c_int)]
    C_NAME, DEFAULTS = "rsqp_nlp_step_options", "rsqp_nlp_step_default_options"


class NlpTrial(C.Structure):
    """rsqp_nlp_trial: host or device addresses, as handler_ratio_test's on_device says"""
    ROWS = (("what", "in", "nq", "int32"), ("rho", "in", "nq", "float64"), ("f_trial", "in", "nq", "float64"),
            ("c_trial", "in", "sC", "float64"), ("x_k", "inout", "sN", "float64"), ("c_k", "inout", "sC", "float64"),
            ("f_k", "inout", "nq", "float64"), ("infea_k", "inout", "nq", "float64"), ("delta", "inout", "nq", "float64"),
            ("actual_reduction", "out", "nq", "float64"),
            ("pred_reduction", "out", "nq", "float64"), ("infea_trial", "out", "nq", "float64"), ("accept", "out", "nq", "int32"),
            ("hu_word", "out", "nq", "int32"), ("hm_word", "out", "nq", "int32"), ("exitflag", "out", "nq", "int32"))
    _fields_, IN, INOUT, OUT, INTS = _pointer_struct(ROWS)


class NlpPoint(C.Structure):
    """rsqp_nlp_point: host or device addresses, as handler_check_optimality's on_device says"""
    ROWS = (("what", "in", "nq", "int32"), ("x_k", "in", "sN", "float64"), ("grad", "in", "sN", "float64"), ("c_k", "in", "sC", "float64"),
            ("infea", "in", "nq", "float64"))
    _fields_, IN, INOUT, OUT, INTS = _pointer_struct(ROWS)


class PenaltyOptions(_Options):
    """rsqp_penalty_options: the defaults of src/Options.cpp:43-52"""
    _fields_ = [("penalty_update_tol", C.c_double), ("increase_parm", C.c_double), ("rho_max", C.c_double), ("penalty_iter_max", C.c_int),
                ("eps1_change_parm", C.c_double), ("eps2", C.c_double)]
    C_NAME, DEFAULTS = "rsqp_penalty_options", "rsqp_penalty_default_options"


class PenaltyState(C.Structure):
    """rsqp_penalty_state: host or device addresses, as handler_update_penalty's on_device says"""
    ROWS = (("what", "in", "nq", "int32"), ("infea_k", "in", "nq", "float64"), ("delta", "in", "nq", "float64"),
            ("x_k", "in", "sN", "float64"), ("c_k", "in", "sC", "float64"), ("rho", "inout", "nq", "float64"),
            ("eps1", "inout", "nq", "float64"), ("trial", "inout", "nq", "int32"), ("succ", "inout", "nq", "int32"),
            ("fail", "inout", "nq", "int32"), ("infea_model", "out", "nq", "float64"), ("infea_infty", "out", "nq", "float64"),
            ("hu_word", "out", "nq", "int32"), ("exitflag", "out", "nq", "int32"), ("nwsr_qp", "out", "nq", "int32"),
            ("nwsr_lp", "out", "nq", "int32"), ("rounds", "out", "nq", "int32"))
    _fields_, IN, INOUT, OUT, INTS = _pointer_struct(ROWS)


class SocOptions(_Options):
    """rsqp_soc_options: composite_pred = 0 by default, the reference as found"""
    _fields_ = [("composite_pred", C.c_int)]
    C_NAME, DEFAULTS = "rsqp_soc_options", "rsqp_soc_default_options"


class SocTrial(C.Structure):
    """rsqp_soc_trial: host or device addresses, as handler_soc_begin's / handler_soc_end's on_device says. The fields of NlpTrial,
    then six of its own"""
    ROWS = NlpTrial.ROWS + (("grad", "in", "sN", "float64"), ("infea_model", "in", "nq", "float64"), ("x_trial", "out", "sN", "float64"),
                            ("soc", "out", "nq", "int32"), ("qp_obj", "out", "nq", "float64"), ("nwsr_soc", "out", "nq", "int32"))
    _fields_, IN, INOUT, OUT, INTS = _pointer_struct(ROWS)


class RsqpError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("rsqp error %d: %s" % (code, msg))
        self.code = code


_LIB = None
_TORCH_FIRST = False    # torch was imported before the library was loaded: its copy of the HIP runtime serves both (device_torch)


def lib():
    """Load librsqp_hip.so; raises if it is missing (there is no fallback path)."""
    global _LIB, _TORCH_FIRST
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s not built: run `python -c 'import __graft_entry__ as g; g.build()'`" % LIB_PATH)
        _TORCH_FIRST = "torch" in sys.modules
        L = C.CDLL(LIB_PATH)
        for table in SYMBOL_TABLES.values():
            for name, (res, args) in table.items():
                f = getattr(L, name)
                f.restype = res
                f.argtypes = args
        _LIB = L
    return _LIB


# the words of rsqp_describe_small_launch, in the order of include/rsqp_hip.h
SMALL_LAUNCH_IN = ("engine", "lanes", "waves", "no_tiny", "lane", "nq", "nVmax", "nCmax", "mat_bytes_max", "mode", "hbm", "state_engine",
                   "tiny_ok", "uniV", "uniC", "uni_pat", "desc", "keep_state", "skip_mark", "member_mode", "done_flag", "cert_out", "x0", "y0",
                   "guess_b", "lane_hblock", "uni_hreg")
SMALL_LAUNCH_OUT = ("invalid", "empty", "family", "engine", "L", "mat_lds", "W", "shape", "mc", "keep", "uni", "hb", "first", "grid", "block",
                    "lds", "stride", "mode", "state_family", "skip_mark")


def describe_small_launch(**words):
    """the launch plan for the given words of SMALL_LAUNCH_IN (all of them, by name) as a dict over SMALL_LAUNCH_OUT; needs no GPU
    (rsqp_describe_small_launch)"""
    a = np.array([words[k] for k in SMALL_LAUNCH_IN], np.int32)
    assert len(words) == len(SMALL_LAUNCH_IN)
    out = np.zeros(len(SMALL_LAUNCH_OUT), np.int32)
    check(lib().rsqp_describe_small_launch(_ip(a), len(a), _ip(out), len(out)))
    return dict(zip(SMALL_LAUNCH_OUT, out.tolist()))


def describe_dense_gemm(m, n, k, batch=1, ws_cap=None):
    """the launch plan of the dense GEMM for an m x n result with inner dimension k as a dict over DENSE_PLAN_OUT; ws_cap: the
    doubles of the split-K workspace the launcher is given (None: none). Needs no GPU (rsqp_dense_describe_gemm)"""
    out = np.zeros(len(DENSE_PLAN_OUT), np.int32)
    check(lib().rsqp_dense_describe_gemm(m, n, k, batch, int(ws_cap is not None), ws_cap or 0, _ip(out), len(out)))
    return dict(zip(DENSE_PLAN_OUT, out.tolist()))


def band_factor(d0, e1, e2):
    """the host side of the banded H^-1 operator for the bands d0 = H[i][i], e1 = H[i][i-1], e2 = H[i][i-2] as a dict: built, c (rows
    per chunk), build (the C of the kernels), growth, and -- when built -- the chunk-interleaved m1i, m2i and sinv exactly as they are
    uploaded (else None). Needs no GPU (rsqp_band_check_factor)"""
    d0, e1, e2 = _d(d0), _d(e1), _d(e2)
    n = len(d0)
    c = (n + BAND_THREADS - 1) // BAND_THREADS
    m1i, m2i, sinv = np.zeros(BAND_THREADS * (c + 1)), np.zeros(BAND_THREADS * (c + 2)), np.zeros(max(n, 1))
    w = [C.c_int(0) for _ in range(3)]
    growth = C.c_double(0.0)
    check(lib().rsqp_band_check_factor(n, _dp(d0), _dp(e1), _dp(e2), *[C.byref(v) for v in w], C.byref(growth), _dp(m1i), len(m1i),
                                       _dp(m2i), len(m2i), _dp(sinv), len(sinv)))
    built = bool(w[0].value)
    return dict(built=built, c=w[1].value, build=w[2].value, growth=growth.value, m1i=m1i if built else None,
                m2i=m2i if built else None, sinv=sinv[:n] if built else None)


class _Handle:
    """the owner of one library handle, _h: close() gives it to the entry point DESTROY names, once -- also on an object whose
    constructor raised before it had a handle. A class whose objects close when they are collected says __del__ = _Handle.close"""

    def close(self):
        if getattr(self, "_h", None):
            getattr(lib(), self.DESTROY)(self._h)
            self._h = None


class BandCheck(_Handle):
    """the uploaded banded factor of one Hessian (rsqp_band_check): apply / apply_q launch the engine's kernels on whole host
    buffers, which are float64 ndarrays WRITTEN IN PLACE (every double of them comes back from the device)"""
    DESTROY = "rsqp_band_check_destroy"
    __del__ = _Handle.close

    def __init__(self, d0, e1, e2):
        d0, e1, e2 = _d(d0), _d(e1), _d(e2)
        self.n = len(d0)
        h = C.c_void_p()
        check(lib().rsqp_band_check_create(self.n, _dp(d0), _dp(e1), _dp(e2), C.byref(h)))
        self._h = h
        self.seq = 0        # the tag of the last multi-workgroup product

    @staticmethod
    def _whole(a, name):
        if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.ndim == 1 and a.flags.c_contiguous and a.flags.writeable):
            raise ValueError("%s is written in place: a contiguous one-dimensional float64 ndarray is needed" % name)
        return a

    def apply(self, buf_in, off_in=0, ncols=1, ld=None, sub=None, off_sub=0, buf_out=None, off_out=0, kernel=BAND_KERNEL_ENGINE):
        """out(:, j) = H^-1 (in(:, j) - sub), j < ncols; buf_out None: in place (the result replaces the operand in buf_in).
        Returns the err word"""
        a = self._whole(buf_in, "buf_in")
        o = None if buf_out is None else self._whole(buf_out, "buf_out")
        s = _d(sub)
        err, seq = C.c_int(0), C.c_longlong(0)
        check(lib().rsqp_band_check_apply(self._h, kernel, ncols, self.n if ld is None else ld, int(o is None), _dp(a), len(a), off_in,
                                          _dp(s), 0 if s is None else len(s), off_sub, _dp(o), 0 if o is None else len(o), off_out,
                                          C.byref(err), C.byref(seq)))
        self.seq = seq.value
        return err.value

    def apply_q(self, Sb, ATdy, dy, gN, g, buf_Hdx, off_h, buf_dx, off_x, kernel=BAND_KERNEL_ENGINE):
        """the step direction's form of one vector: Hdx = (ATdy + (Sb ? dy : 0)) - (gN - g) on every row, dx = H^-1 Hdx on the rows
        with Sb == 0. Returns the err word"""
        Sb = _i(Sb)
        v = [_d(x) for x in (ATdy, dy, gN, g)]
        if len(Sb) != self.n or any(len(x) != self.n for x in v):
            raise ValueError("Sb, ATdy, dy, gN, g have %d entries each" % self.n)
        hb, xb = self._whole(buf_Hdx, "buf_Hdx"), self._whole(buf_dx, "buf_dx")
        err, seq = C.c_int(0), C.c_longlong(0)
        check(lib().rsqp_band_check_apply_q(self._h, kernel, _ip(Sb), *[_dp(x) for x in v], _dp(hb), len(hb), off_h, _dp(xb), len(xb),
                                            off_x, C.byref(err), C.byref(seq)))
        self.seq = seq.value
        return err.value


def plan_builds(plan):
    """the kernel instantiations a launch plan (describe_small_launch, Batch.last_plan) starts, each by the plan words that tell it
    from the other builds of its kernel: ("qp", engine, L, mat_lds, W, shape) small_qp_kernel, ("qpg", first) small_qpg_kernel,
    which goes first where the plan says so, ("tiny", mc, W) tiny_qp_kernel, ("lane", keep, uni, hb) lane_qp_kernel,
    ("qph", engine) small_qph_kernel. An invalid or empty plan starts none"""
    if plan["invalid"] or plan["empty"]:
        return []
    fam = plan["family"]
    if fam == 1:
        return [("tiny", plan["mc"], plan["W"])]
    if fam == 2:
        return [("lane", plan["keep"], plan["uni"], plan["hb"])]
    if fam == 3:
        return [("qph", plan["engine"])]
    first = [("qpg", plan["first"])] if plan["first"] else []
    return first + [("qp", plan["engine"], plan["L"], plan["mat_lds"], plan["W"], plan["shape"])]


def device_torch():
    """torch, for the calls that take or make device tensors. torch ships its own copy of the HIP runtime, with the soname the
    library asks for: imported BEFORE the library is loaded, that copy serves both and a tensor's data_ptr() is memory of the
    runtime the batch runs on. The other order leaves two runtimes in the process, and torch finds no GPU."""
    lib()
    if not _TORCH_FIRST:
        raise RuntimeError("device tensors need `import torch` before restartsqp_amd.capi loads librsqp_hip.so (one HIP runtime)")
    import torch
    return torch


def check(rc):
    if rc < 0:
        raise RsqpError(rc, lib().rsqp_last_error().decode())
    return rc


def _d(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def _i(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int32)


def _dp(a):
    return None if a is None else a.ctypes.data_as(dp)


def _ip(a):
    return None if a is None else a.ctypes.data_as(ip)


def device_count():
    return lib().rsqp_device_count()


DUMP_QPOASES, DUMP_QORE = 0, 1


def write_qp_dump(path, qp, layout=DUMP_QORE):
    """WriteQPDataToFile in the reference's layouts (host only): `qp` has the QPData fields."""
    a = [_d(qp.lb), _d(qp.ub), _d(qp.lbA), _d(qp.ubA), _d(qp.g)]
    Ajc, Air, Aval = _i(qp.A_jc), _i(qp.A_ir), _d(qp.A_val)
    Hjc, Hir, Hval = _i(qp.H_jc), _i(qp.H_ir), _d(qp.H_val)
    check(lib().rsqp_write_qp_dump(os.fsencode(path), layout, qp.nV, qp.nC, *[_dp(v) for v in a], _ip(Ajc), _ip(Air),
                                   _dp(Aval), _ip(Hjc), _ip(Hir), _dp(Hval)))


def read_qore_dump(path):
    """C reader of the QORE dump layout -> dict of arrays (CSC matrices)."""
    n = [C.c_int(0) for _ in range(4)]
    check(lib().rsqp_read_qore_dump_sizes(os.fsencode(path), *[C.byref(v) for v in n]))
    nV, nC, nnzA, nnzH = (v.value for v in n)
    d = dict(nV=nV, nC=nC, lb=np.zeros(nV), ub=np.zeros(nV), lbA=np.zeros(nC), ubA=np.zeros(nC), g=np.zeros(nV),
             A_jc=np.zeros(nV + 1, np.int32), A_ir=np.zeros(nnzA, np.int32), A_val=np.zeros(nnzA),
             H_jc=np.zeros(nV + 1, np.int32), H_ir=np.zeros(nnzH, np.int32), H_val=np.zeros(nnzH))
    check(lib().rsqp_read_qore_dump(os.fsencode(path), _dp(d["lb"]), _dp(d["ub"]), _dp(d["lbA"]), _dp(d["ubA"]), _dp(d["g"]),
                                    _ip(d["A_jc"]), _ip(d["A_ir"]), _dp(d["A_val"]), _ip(d["H_jc"]), _ip(d["H_ir"]),
                                    _dp(d["H_val"])))
    return d


class Solver(_Handle):
    """Thin RAII wrapper over one ``rsqp_solver`` handle."""
    DESTROY = "rsqp_destroy"
    __del__ = _Handle.close

    def __init__(self, nV, nC, device=-1):
        self.nV, self.nC = nV, nC
        h = C.c_void_p()
        check(lib().rsqp_create(nV, nC, device, C.byref(h)))
        self._h = h

    def write_qp_data(self, path, layout=DUMP_QPOASES):
        """WriteQPDataToFile for the data held by this handle."""
        check(lib().rsqp_write_qp_data(self._h, os.fsencode(path), layout))

    def set_engine_profiling(self, on=True):
        check(lib().rsqp_set_engine_profiling(self._h, int(bool(on))))

    def engine_profile(self):
        """per-kernel-class device time / algorithmic bytes of the HBM-resident engine since its creation
        (rsqp_get_engine_profile), or None when the handle runs the LDS-resident engine"""
        n = lib().rsqp_get_engine_profile(self._h, None, 0)
        if n <= 0:
            return None
        buf = (C.c_double * (4 * n))()
        names = (C.c_char_p * n)()
        lib().rsqp_get_engine_profile(self._h, C.cast(buf, C.c_void_p), n)
        lib().rsqp_engine_profile_names(C.cast(names, C.c_void_p), n)
        out = {}
        for k in range(n):
            calls, ms, byts, peak = buf[4 * k], buf[4 * k + 1], buf[4 * k + 2], buf[4 * k + 3]
            if calls > 0:
                out[names[k].decode()] = {"calls": int(calls), "ms_total": ms, "us_per_call": 1e3 * ms / calls,
                                          "algorithmic_bytes": byts, "achieved": byts / (ms * 1e-3) / 1e9 if ms > 0 else None,
                                          "unit": "GB/s", "peak": 8000.0, "bound": "hbm",
                                          "frac": byts / (ms * 1e-3) / 1e9 / 8000.0 if ms > 0 else None}
        return out

    def setup_profile(self):
        """the last blocked (matrix-core) set-up on the HBM-resident engine (rsqp_get_setup_profile), or None"""
        buf = np.zeros(8)
        if lib().rsqp_get_setup_profile(self._h, buf.ctypes.data_as(dp)) != 1:
            return None
        return {"nFR": int(buf[0]), "nAC": int(buf[1]), "nZ": int(buf[2]), "ms_qr_q_rinv": buf[3], "ms_zhz_chol_inv": buf[4],
                "flops_qr_q_rinv": buf[5], "flops_zhz_chol_inv": buf[6], "range_space": bool(buf[7])}

    def structure_seconds(self, which=0):
        return lib().rsqp_get_structure_seconds(self._h, which)

    def time_value_refresh(self, repeats=50):
        a, b = C.c_float(0), C.c_float(0)
        check(lib().rsqp_time_value_refresh(self._h, repeats, C.byref(a), C.byref(b)))
        return a.value, b.value

    def time_value_refresh_fused(self, repeats=50):
        a = C.c_float(0)
        check(lib().rsqp_time_value_refresh_fused(self._h, repeats, C.byref(a)))
        return a.value

    def set_engine(self, engine):
        """0 automatic, 1 LDS-resident kernel, 2 HBM-resident engine."""
        check(lib().rsqp_set_engine(self._h, engine))

    @property
    def engine(self):
        return lib().rsqp_get_engine(self._h)

    def set_reinit_guess(self, from_y0):
        """warm re-initialisation without guessed constraints: from_y0=False as qpOASES, from A x0 (the library default, the
        reference's behaviour) or -- opt-in, from_y0=True -- sides from sign(y0). No default argument: a bare call must not
        silently leave the reference's rule"""
        check(lib().rsqp_set_reinit_guess(self._h, int(bool(from_y0))))

    MODE_NAMES = {-1: "none", 0: "init (cold)", 1: "hotstart(g, lb, ub, lbA, ubA)", 2: "hotstart(H, g, A, ..) -- new matrices",
                  3: "init(.., x_qp, y_qp, &bounds) -- status flip"}

    def last_mode(self):
        """RSQP_MODE_* the dispatch of the last optimize_qp / optimize_lp chose"""
        return lib().rsqp_get_last_mode(self._h)

    LARGE_PATHS = {-1: "none", 0: "null-space", 1: "range-space (diagonal H)", 2: "general range-space (banded H^-1)",
                   3: "general range-space (dense H^-1)", 4: "general range-space (dense H^-1 + static tableau [I; A] H^-1 [I A'])"}

    def large_path(self):
        """which formulation of the HBM-resident engine holds this handle's factors (rsqp_get_large_path)"""
        return lib().rsqp_get_large_path(self._h)

    def set_options(self, qp_maxiter=1000, lp_maxiter=100):
        check(lib().rsqp_set_options(self._h, qp_maxiter, lp_maxiter))

    def set_A_triplet(self, irow, jcol, val, ident=()):
        irow, jcol, val = _i(irow), _i(jcol), _d(val)
        ii = _i([b[0] for b in ident]); ij = _i([b[1] for b in ident])
        isz = _i([b[2] for b in ident]); iv = _d([b[3] for b in ident])
        check(lib().rsqp_set_A_triplet(self._h, len(val), _ip(irow), _ip(jcol), _dp(val), len(ident), _ip(ii), _ip(ij),
                                       _ip(isz), _dp(iv)))

    def set_H_triplet(self, irow, jcol, val, is_symmetric=True):
        irow, jcol, val = _i(irow), _i(jcol), _d(val)
        check(lib().rsqp_set_H_triplet(self._h, len(val), _ip(irow), _ip(jcol), _dp(val), int(is_symmetric)))

    def set_A_csc(self, jc, ir, val):
        jc, ir, val = _i(jc), _i(ir), _d(val)
        check(lib().rsqp_set_A_csc(self._h, _ip(jc), _ip(ir), _dp(val)))

    def set_H_csc(self, jc, ir, val):
        jc, ir, val = _i(jc), _i(ir), _d(val)
        check(lib().rsqp_set_H_csc(self._h, _ip(jc), _ip(ir), _dp(val)))

    def _get_csc(self, which):
        nnz = check(getattr(lib(), "rsqp_get_%s_nnz" % which)(self._h))
        ncol = self.nV
        jc = np.zeros(ncol + 1, np.int32); ir = np.zeros(nnz, np.int32); val = np.zeros(nnz)
        order = np.zeros(nnz, np.int32)
        check(getattr(lib(), "rsqp_get_%s_csc" % which)(self._h, _ip(jc), _ip(ir), _dp(val), _ip(order)))
        return jc, ir, val, order

    def get_A_csc(self):
        return self._get_csc("A")

    def get_H_csc(self):
        return self._get_csc("H")

    def set_vector(self, which, v):
        v = _d(v)
        n = self.nV if which <= VEC_UB else self.nC
        if len(v) < n:
            raise ValueError("vector too short")
        check(lib().rsqp_set_vector(self._h, which, _dp(v)))

    def set_entry(self, which, loc, value):
        check(lib().rsqp_set_entry(self._h, which, loc, float(value)))

    def get_vector(self, which):
        out = np.zeros(self.nV if which <= VEC_UB else self.nC)
        check(lib().rsqp_get_vector(self._h, which, _dp(out)))
        return out

    def reset_constraints(self):
        check(lib().rsqp_reset_constraints(self._h))

    def optimize_qp(self):
        n = C.c_int(0)
        check(lib().rsqp_optimize_qp(self._h, C.byref(n)))
        return n.value

    def optimize_lp(self):
        n = C.c_int(0)
        check(lib().rsqp_optimize_lp(self._h, C.byref(n)))
        return n.value

    def solve(self, mode, nWSR, x0=None, y0=None, guess_b=None):
        n = C.c_int(nWSR)
        x0, y0, gb = _d(x0), _d(y0), _i(guess_b)
        check(lib().rsqp_solve(self._h, mode, C.byref(n), _dp(x0), _dp(y0), _ip(gb)))
        return n.value

    @property
    def x(self):
        out = np.zeros(self.nV)
        check(lib().rsqp_get_primal(self._h, _dp(out)))
        return out

    @property
    def y(self):
        out = np.zeros(self.nV + self.nC)
        check(lib().rsqp_get_dual(self._h, _dp(out)))
        return out

    @property
    def objective(self):
        return lib().rsqp_get_objective(self._h)

    @property
    def status(self):
        return lib().rsqp_get_status(self._h)

    def is_solved(self):
        return bool(lib().rsqp_is_solved(self._h))

    def working_set_raw(self):
        wb = np.zeros(self.nV, np.int32); wc = np.zeros(self.nC, np.int32)
        check(lib().rsqp_get_working_set_raw(self._h, _ip(wb), _ip(wc)))
        return wb, wc

    def working_set(self):
        Wc = np.zeros(self.nC, np.int32); Wb = np.zeros(self.nV, np.int32)
        check(lib().rsqp_get_working_set(self._h, _ip(Wc), _ip(Wb)))
        return Wc, Wb

    def test_optimality(self):
        Wc = np.zeros(self.nC, np.int32); Wb = np.zeros(self.nV, np.int32)
        st = OptimalityStatus()
        rc = check(lib().rsqp_test_optimality(self._h, _ip(Wc), _ip(Wb), C.byref(st)))
        return bool(rc), st, Wc, Wb

    def A_times(self, p):
        p = _d(p); out = np.zeros(self.nC)
        check(lib().rsqp_A_times(self._h, _dp(p), _dp(out)))
        return out

    def A_transposed_times(self, p):
        p = _d(p); out = np.zeros(self.nV)
        check(lib().rsqp_A_transposed_times(self._h, _dp(p), _dp(out)))
        return out

    def H_times(self, p):
        p = _d(p); out = np.zeros(self.nV)
        check(lib().rsqp_H_times(self._h, _dp(p), _dp(out)))
        return out


class Batch(_Handle):
    """A batch of independent QPs (``rsqp_batch``): problems given as a list of QPData-like
    objects with fields nV, nC, A_jc/A_ir/A_val, H_jc/H_ir/H_val, g, lb, ub, lbA, ubA."""
    DESTROY = "rsqp_batch_destroy"
    __del__ = _Handle.close

    def __init__(self, problems, device=-1):
        self.problems = problems
        self.nq = len(problems)
        self.nV = _i([p.nV for p in problems]); self.nC = _i([p.nC for p in problems])
        Ajc = _i(np.concatenate([p.A_jc for p in problems]))
        Air = _i(np.concatenate([p.A_ir for p in problems] + [np.zeros(0, np.int32)]))
        Aval = _d(np.concatenate([p.A_val for p in problems] + [np.zeros(0)]))
        haveH = all(p.H_jc is not None for p in problems)
        Hjc = _i(np.concatenate([p.H_jc for p in problems])) if haveH else None
        Hir = _i(np.concatenate([p.H_ir for p in problems] + [np.zeros(0, np.int32)])) if haveH else None
        Hval = _d(np.concatenate([p.H_val for p in problems] + [np.zeros(0)])) if haveH else None
        h = C.c_void_p()
        check(lib().rsqp_batch_create(self.nq, _ip(self.nV), _ip(self.nC), _ip(Ajc), _ip(Air), _dp(Aval), _ip(Hjc),
                                      _ip(Hir), _dp(Hval), device, C.byref(h)))
        self._h = h
        self.device = device
        self.offV = np.concatenate([[0], np.cumsum(self.nV)]).astype(np.int64)
        self.offC = np.concatenate([[0], np.cumsum(self.nC)]).astype(np.int64)
        # entries per member in the caller's layout: of J (columns [0, nV - 2 nC) of A: handler_set_matrices), of A and of H
        self.jnz = np.array([int(p.A_jc[max(p.nV - 2 * p.nC, 0)]) for p in problems], np.int64)
        self.annz = np.array([int(p.A_jc[p.nV]) for p in problems], np.int64)
        self.hnnz = np.array([int(p.H_jc[p.nV]) for p in problems], np.int64) if haveH else None
        self.set_vectors_from(problems)

    @functools.cached_property
    def sizes(self):
        """(nq, sN, sC, sV): the members, and the pooled entries of the NLP layout (member q owns nV[q] - 2 nC[q]), of the constraint
        layout (that of lbA) and of the variable layout (that of g); fixed when the batch is created"""
        sV, sC = int(np.sum(self.nV)), int(np.sum(self.nC))
        return self.nq, sV - 2 * sC, sC, sV

    def _handler_sizes(self):
        """(sN, sC) of `sizes`, under the name the tests of the handler calls ask by"""
        return self.sizes[1:3]

    def _mask(self, mask):
        """a per-member mask as nq ints (None stays None: everybody)"""
        if mask is None:
            return None
        m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.int32)
        if m.ndim != 1 or m.size != self.nq:
            raise ValueError("the mask has %d entries, the batch has %d members" % (m.size, self.nq))
        return m

    def set_members(self, mask=None):
        """who takes part in the following optimize_qp / optimize_lp calls (mask[q] != 0); None = everybody. A member that sits out
        keeps everything it has; its nWSR_used is 0 and dispatch() reports mode -1 for it"""
        m = self._mask(mask)
        check(lib().rsqp_batch_set_members(self._h, _ip(m)))

    def set_vectors(self, g, lb, ub, lbA, ubA, members=None):
        """members: a mask -- only the named members' entries are written (the others' may be anything of the right size)"""
        g, lb, ub, lbA, ubA = _d(g), _d(lb), _d(ub), _d(lbA), _d(ubA)
        if members is None:
            check(lib().rsqp_batch_set_vectors(self._h, _dp(g), _dp(lb), _dp(ub), _dp(lbA), _dp(ubA)))
        else:
            m = self._mask(members)
            check(lib().rsqp_batch_set_vectors_of(self._h, _ip(m), _dp(g), _dp(lb), _dp(ub), _dp(lbA), _dp(ubA)))

    def set_vectors_from(self, problems, members=None):
        cat = lambda name: np.concatenate([getattr(p, name) for p in problems] + [np.zeros(0)])
        self.set_vectors(cat("g"), cat("lb"), cat("ub"), cat("lbA"), cat("ubA"), members=members)

    def set_matrix_values(self, Aval=None, Hval=None, members=None):
        """members: a mask -- only the named members' values are written, and only they count as updated (Update_A / Update_H)"""
        Aval, Hval = _d(Aval), _d(Hval)
        if members is None:
            check(lib().rsqp_batch_set_matrix_values(self._h, _dp(Aval), _dp(Hval)))
        else:
            m = self._mask(members)
            check(lib().rsqp_batch_set_matrix_values_of(self._h, _ip(m), _dp(Aval), _dp(Hval)))

    # ---- the QPhandler of every member (rsqp_batch_handler_*): NLP layout = member q owns nV[q] - 2 nC[q] entries, pooled ----
    @staticmethod
    def _sized(a, n, name, dtype=np.float64):
        """a host array of exactly n entries (None stays None)"""
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dtype)
        if a.ndim != 1 or a.size != n:
            raise ValueError("%s has %d entries, the batch needs %d" % (name, a.size, n))
        return a

    def _addr(self, a, n, name, on_device, dtype="float64", writable=False):
        """the address of a pooled argument of n entries: a device tensor (torch, or anything with data_ptr / numel / dtype /
        is_contiguous), or a host array -- which is converted unless the call writes it (then it must be a contiguous ndarray of the
        right type: it is written in place); (address, what keeps it alive until the call is over), (None, None) for None"""
        if a is None:
            return None, None
        if on_device:
            if int(a.numel()) != n:
                raise ValueError("%s has %d entries, the batch needs %d" % (name, int(a.numel()), n))
            if not str(a.dtype).endswith(dtype) or not a.is_contiguous() or not getattr(a, "is_cuda", True):
                raise ValueError("%s must be a contiguous %s tensor on the batch's device" % (name, dtype))
            return int(a.data_ptr()), a
        if not writable:
            a = self._sized(a, n, name, dtype)
        elif not (isinstance(a, np.ndarray) and a.dtype == dtype and a.flags.c_contiguous and a.flags.writeable):
            raise ValueError("%s is written in place: a contiguous %s ndarray is needed" % (name, dtype))
        elif a.size != n:
            raise ValueError("%s has %d entries, the batch needs %d" % (name, a.size, n))
        return a.ctypes.data, a

    def _new_out(self, n, on_device, dtype="float64", cols=None, fill=True):
        """a new output of n entries (n rows of `cols`): a host array of zeros, or with on_device a tensor on the batch's device --
        of zeros, or with fill=False of whatever the memory holds (for a call that writes every entry a caller may read)"""
        shape = n if cols is None else (n, cols)
        if not on_device:
            return np.zeros(shape, dtype)
        torch = device_torch()
        dev = "cuda" if getattr(self, "device", -1) < 0 else "cuda:%d" % self.device
        return (torch.zeros if fill else torch.empty)(shape, dtype=getattr(torch, dtype), device=dev)

    def _pooled(self, cls, given, out, on_device, optional=()):
        """the pointer struct `cls` of a per-member call, filled from its table: `given` holds the call's inputs and in/out arrays in
        the order cls.IN + cls.INOUT, each required unless its layout is empty or `optional` names it; an output is the array of
        `out` where it has one, else a new zero-filled one. Returns (the struct, what keeps the converted inputs alive: hold it
        until the call is over, `out` complete)"""
        size = dict(zip(("nq", "sN", "sC"), self.sizes))
        out = dict(out or {})
        for k, role, length, dtype in cls.ROWS:
            if role == "out" and out.get(k) is None:
                out[k] = self._new_out(size[length], on_device, dtype)
        given = dict(zip(cls.IN + cls.INOUT, given))
        s, keep = cls(), []
        for turn in ("in", "inout", "out"):
            for k, role, length, dtype in cls.ROWS:
                if role != turn:
                    continue
                a = out[k] if role == "out" else given[k]
                if a is None and size[length] > 0 and k not in optional:
                    raise ValueError("%s is required" % k)
                addr, a = self._addr(a, size[length], k, on_device, dtype, writable=role != "in")
                setattr(s, k, addr); keep.append(a)
        return s, keep, out

    def handler_set_problem(self, x_l, x_u, c_l=None, c_u=None):
        """the NLP bounds of every member, fixed for a run: x_l, x_u in the NLP layout, c_l, c_u in the layout of lbA"""
        _, sN, sC, _ = self.sizes
        x_l, x_u = self._sized(x_l, sN, "x_l"), self._sized(x_u, sN, "x_u")
        c_l, c_u = self._sized(c_l, sC, "c_l"), self._sized(c_u, sC, "c_u")
        if x_l is None or x_u is None or (sC > 0 and (c_l is None or c_u is None)):
            raise ValueError("x_l, x_u (and c_l, c_u when the batch has constraints) are required")
        check(lib().rsqp_batch_handler_set_problem(self._h, _dp(x_l), _dp(x_u), _dp(c_l), _dp(c_u)))

    def handler_update(self, what, delta, rho, x_k, c_k, grad=None, on_device=False):
        """QPhandler's setters for every member on the device: what[q] = HU_* bits (0: member q is not touched); delta, rho: nq;
        x_k, grad: NLP layout (grad None: the LP handler's set_g(rho)); c_k: the layout of lbA. on_device: every argument is a
        tensor on the batch's device (what: int32, the others float64), complete before the call"""
        given = (what, delta, rho, x_k, grad, c_k)
        it, keep, _ = self._pooled(HandlerIterate, given, None, on_device, optional=HandlerIterate.IN)
        size = dict(zip(("nq", "sN", "sC"), self.sizes))
        for (k, _, length, _), a in zip(HandlerIterate.ROWS, given):        # (this call sizes every argument before it misses one)
            if a is None and k != "grad" and size[length] > 0:
                raise ValueError("%s is required" % k)
        check(lib().rsqp_batch_handler_update(self._h, C.addressof(it), int(bool(on_device))))

    def handler_step(self, on_device=False, out=None):
        """what Algorithm reads from the last solve, as a dict: p, lam_x (NLP layout), lam_c (layout of lbA), infea_model, norm_p
        (nq). on_device: written into float64 tensors on the batch's device -- those of `out` (same keys), else new torch tensors"""
        nq, sN, sC, _ = self.sizes
        sizes = (("p", sN), ("lam_c", sC), ("lam_x", sN), ("infea_model", nq), ("norm_p", nq))
        if out is None or not on_device:
            out = {k: self._new_out(n, on_device, fill=False) for k, n in sizes}
        addr = [self._addr(out[k], n, k, on_device, writable=True)[0] for k, n in sizes]
        check(lib().rsqp_batch_handler_get_step(self._h, *addr, int(bool(on_device))))
        return out

    # ---- the decisions of the SQP loop per member (include/rsqp_hip_nlp_step.h) ----
    def handler_infeasibility(self, c, on_device=False, out=None):
        """cal_infea(c, c_l, c_u) of every member (rsqp_batch_handler_infeasibility): c in the layout of lbA, the result nq entries
        -- `out`, else a new array (on_device: tensors on the batch's device)"""
        nq, _, sC, _ = self.sizes
        if out is None:
            out = self._new_out(nq, on_device)
        ca, keep = self._addr(c, sC, "c", on_device)
        oa, _ = self._addr(out, nq, "out", on_device, writable=True)
        check(lib().rsqp_batch_handler_infeasibility(self._h, ca, oa, int(bool(on_device))))
        return out

    def handler_ratio_test(self, what, rho, f_trial, c_trial, x_k, c_k, f_k, infea_k, delta, options=None, on_device=False, out=None):
        """ratio_test + update_radius for every member with what[q] != 0 (rsqp_batch_handler_ratio_test), on the step of the last
        solve. what (int32), rho, f_trial: nq; c_trial: the layout of lbA. x_k (NLP layout), c_k, f_k, infea_k, delta are the
        members' iterates and are WRITTEN IN PLACE: contiguous float64 ndarrays, or with on_device tensors on the batch's device,
        complete before the call. Returns the outputs as a dict over NlpTrial.OUT (accept, hu_word, hm_word, exitflag: int32) --
        the arrays of `out` where it has them (a member with word 0 keeps their bytes), else new zero-filled ones"""
        t, keep, out = self._pooled(NlpTrial, (what, rho, f_trial, c_trial, x_k, c_k, f_k, infea_k, delta), out, on_device)
        o = options or NlpStepOptions()
        check(lib().rsqp_batch_handler_ratio_test(self._h, C.addressof(t), C.addressof(o), int(bool(on_device))))
        return out

    def handler_check_optimality(self, what, x_k, grad, c_k, infea, options=None, on_device=False, out=None, verdict=None):
        """check_optimality for every member with what[q] != 0 (rsqp_batch_handler_check_optimality), with the multipliers of the
        last solve and the Jacobian as it stands in the batch's A pool (handler_set_matrices with the point's J comes first).
        x_k, grad: NLP layout; c_k: the layout of lbA; infea: nq. Returns (status, verdict): status [nq, 5] over CERTIFICATE_FIELDS,
        verdict int32 with the KKT_* bits -- `out` / `verdict` where given (a member with word 0 keeps their bytes), else new
        zero-filled ones; on_device: tensors on the batch's device"""
        nq = self.nq
        if out is None:
            out = self._new_out(nq, on_device, cols=5)
        if verdict is None:
            verdict = self._new_out(nq, on_device, "int32")
        p, keep, _ = self._pooled(NlpPoint, (what, x_k, grad, c_k, infea), None, on_device)
        oa, _ = self._addr(out, 5 * nq, "out", on_device, writable=True)
        va, _ = self._addr(verdict, nq, "verdict", on_device, "int32", writable=True)
        o = options or NlpStepOptions()
        check(lib().rsqp_batch_handler_check_optimality(self._h, C.addressof(p), C.addressof(o), oa, va, int(bool(on_device))))
        return out, verdict

    # ---- update_penalty_parameter per member, across this batch and its LP batch (include/rsqp_hip_penalty.h) ----
    def handler_pair_lp(self, lp):
        """`lp` becomes the LP handler of this batch (myLP_ beside myQP_, rsqp_batch_handler_pair_lp): another Batch of the same
        members -- sizes and canonical A pattern member by member --, on the same device, with handler_set_problem called on both;
        None unpairs. The pair keeps `lp` alive"""
        check(lib().rsqp_batch_handler_pair_lp(self._h, None if lp is None else lp._h))
        self._lp_pair = lp

    def handler_update_penalty(self, what, infea_k, delta, x_k, c_k, rho, eps1, trial, succ, fail, options=None, on_device=False, out=None):
        """update_penalty_parameter for every member with what[q] != 0 (rsqp_batch_handler_update_penalty), between the QP solve and
        the ratio test: on the results of this batch's last solve, with the LP batch of handler_pair_lp. what (int32), infea_k,
        delta: nq; x_k: NLP layout; c_k: the layout of lbA. rho, eps1 (float64) and trial, succ, fail (int32) are the members' state
        and are WRITTEN IN PLACE: contiguous ndarrays, or with on_device tensors on the batch's device, complete before the call.
        Returns the outputs as a dict over PenaltyState.OUT (infea_model, infea_infty: float64, the others int32) -- the arrays of
        `out` where it has them (a member with word 0 keeps their bytes), else new zero-filled ones"""
        s, keep, out = self._pooled(PenaltyState, (what, infea_k, delta, x_k, c_k, rho, eps1, trial, succ, fail), out, on_device)
        o = options or PenaltyOptions()
        check(lib().rsqp_batch_handler_update_penalty(self._h, C.addressof(s), C.addressof(o), int(bool(on_device))))
        return out

    # ---- second_order_correction per member (include/rsqp_hip_soc.h) ----
    def _soc_call(self, fn, given, optional, options, soc_options, on_device, out):
        t, keep, out = self._pooled(SocTrial, given, out, on_device, optional)
        o, so = options or NlpStepOptions(), soc_options or SocOptions()
        check(fn(self._h, C.addressof(t), C.addressof(o), C.addressof(so), int(bool(on_device))))
        return out

    def handler_soc_begin(self, what, rho, f_trial, c_trial, x_k, c_k, f_k, infea_k, delta, grad=None, infea_model=None, options=None,
                          soc_options=None, on_device=False, out=None):
        """the ratio test with second_order_correction for every member with what[q] != 0 (rsqp_batch_handler_soc_begin), called
        INSTEAD OF handler_ratio_test: what[q] = SOC_TEST | SOC_CORRECT bits; the other arguments as handler_ratio_test takes them,
        plus grad (NLP layout: grad_f at x_k, required when a word has SOC_CORRECT) and infea_model (nq, optional: as the penalty
        call left it). x_k, c_k, f_k, infea_k, delta are WRITTEN IN PLACE. Returns the outputs as a dict over SocTrial.OUT (x_trial:
        NLP layout; accept, hu_word, hm_word, exitflag, soc, nwsr_soc: int32) -- the arrays of `out` where it has them (a member
        with word 0 keeps their bytes), else new zero-filled ones. The members with soc == 1 await f and c at x_trial and
        handler_soc_end"""
        given = (what, rho, f_trial, c_trial, grad, infea_model, x_k, c_k, f_k, infea_k, delta)
        return self._soc_call(lib().rsqp_batch_handler_soc_begin, given, ("grad", "infea_model"), options, soc_options, on_device, out)

    def handler_soc_end(self, rho, f_trial, c_trial, x_k, c_k, f_k, infea_k, delta, out, options=None, soc_options=None,
                        on_device=False):
        """the second ratio test, the restore of a rejected correction and update_radius for every member with out["soc"][q] != 0
        that the last handler_soc_begin set going (rsqp_batch_handler_soc_end): f_trial, c_trial at the x_trial of that call; `out`
        is the dict that call returned (soc is required) and is returned with this call's outputs"""
        if dict(out or {}).get("soc") is None:
            raise ValueError("soc is required: the array handler_soc_begin wrote")
        given = (None, rho, f_trial, c_trial, None, None, x_k, c_k, f_k, infea_k, delta)
        optional = ("what", "grad", "infea_model")
        return self._soc_call(lib().rsqp_batch_handler_soc_end, given, optional, options, soc_options, on_device, out)

    def set_objective(self, obj, members=None):
        """the objective pool of the named members (a mask; None: everybody) := obj (nq entries); nothing else is touched
        (rsqp_batch_set_objective)"""
        obj = self._sized(obj, self.nq, "obj")
        if obj is None:
            raise ValueError("obj is required")
        check(lib().rsqp_batch_set_objective(self._h, _ip(self._mask(members)), _dp(obj)))

    def get_vectors(self):
        """(g, lb, ub, lbA, ubA) as the pools hold them on the device, in the layout of set_vectors"""
        _, _, sC, sV = self.sizes
        v = [np.zeros(sV), np.zeros(sV), np.zeros(sV), np.zeros(sC), np.zeros(sC)]
        check(lib().rsqp_batch_get_vectors(self._h, *[_dp(a) for a in v]))
        return tuple(v)

    def _matrix_sizes(self):
        """(entries of jac, of the A value pool, of the H value pool -- None without H) in the layout the batch was created with"""
        return int(np.sum(self.jnz)), int(np.sum(self.annz)), None if self.hnnz is None else int(np.sum(self.hnnz))

    def handler_set_matrices(self, what, jac=None, hess=None, on_device=False):
        """QPhandler's set_A / set_H, update_A / update_H for every member on the device: what[q] = HM_* bits (0: member q is not
        touched). jac: pooled, member q owns the entries of its J -- columns [0, n_q) of its A, in the order of its A_val; the
        identity entries are never written. hess: the layout of the H values the batch was created with (ignored when the batch has
        no H). on_device: what (int32), jac and hess (float64) are tensors on the batch's device, complete before the call; a
        missing jac / hess then promises that no word carries its bit"""
        nJ, nA, nH = self._matrix_sizes()
        spec = (("what", what, self.nq, "int32"), ("jac", jac, nJ, "float64"), ("hess", None if nH is None else hess, nH, "float64"))
        if what is None:
            raise ValueError("what is required")
        addr, keep = zip(*[self._addr(a, n, name, on_device, dtype) for name, a, n, dtype in spec])
        if not on_device:
            seen = int(np.bitwise_or.reduce(keep[0])) if self.nq else 0
            if (seen & HM_JAC and keep[1] is None) or (seen & HM_HESS and nH is not None and keep[2] is None):
                raise ValueError("a word names a matrix that is not given")
        check(lib().rsqp_batch_handler_set_matrices(self._h, *addr, int(bool(on_device))))

    def get_matrix_values(self):
        """(Aval, Hval) as the pools hold them on the device, in the layout the batch was created with; Hval None without H"""
        nJ, nA, nH = self._matrix_sizes()
        A, H = np.zeros(nA), (None if nH is None else np.zeros(nH))
        check(lib().rsqp_batch_get_matrix_values(self._h, _dp(A), _dp(H)))
        return A, H

    def solve(self, mode=MODE_COLD, max_nWSR=1000, sync=True):
        check(lib().rsqp_batch_solve(self._h, mode, max_nWSR))
        if sync:
            check(lib().rsqp_batch_sync(self._h))

    def set_warm_start(self, x0=None, y0=None, guess_b=None):
        """inputs of solve(MODE_WARM_REINIT), pooled like the vectors (y0: the layout of y); None = absent for every member"""
        x0, y0, guess_b = _d(x0), _d(y0), _i(guess_b)
        sV, sC = int(self.offV[-1]), int(self.offC[-1])
        for a, n, name in ((x0, sV, "x0"), (y0, sV + sC, "y0"), (guess_b, sV, "guess_b")):
            if a is not None and a.size != n:
                raise ValueError("%s has %d entries, the batch needs %d" % (name, a.size, n))
        check(lib().rsqp_batch_set_warm_start(self._h, _dp(x0), _dp(y0), _ip(guess_b)))

    def set_options(self, qp_maxiter=1000, lp_maxiter=None):
        check(lib().rsqp_batch_set_options(self._h, int(qp_maxiter)))
        if lp_maxiter is not None:
            check(lib().rsqp_batch_set_lp_options(self._h, int(lp_maxiter)))

    def optimize_qp(self):
        """optimizeQP for every member (dispatch + handle_error per member); returns nWSR_used per member"""
        used = np.zeros(self.nq, np.int32)
        check(lib().rsqp_batch_optimize_qp(self._h, _ip(used)))
        return used

    def optimize_lp(self):
        """optimizeLP for every member (H ignored: regVal*I, dispatch + handle_error's LP branch + one regularisation step per
        member); returns nWSR_used per member"""
        used = np.zeros(self.nq, np.int32)
        check(lib().rsqp_batch_optimize_lp(self._h, _ip(used)))
        return used

    def dispatch(self):
        """(mode, rescue) per member of the last optimize_qp / optimize_lp: MODE_* of its first solve (an LP call runs a flip,
        MODE_WARM_REINIT, as a plain init; -1: the member sat out, set_members); 0 none / 1 from scratch / 2 slack point"""
        mode = np.zeros(self.nq, np.int32); rescue = np.zeros(self.nq, np.int32)
        check(lib().rsqp_batch_get_dispatch(self._h, _ip(mode), _ip(rescue)))
        return mode, rescue

    def set_keep_state(self, keep):
        check(lib().rsqp_batch_set_keep_state(self._h, int(bool(keep))))

    def set_handover(self, on):
        """on: every launch on the register-resident tableau kernels (last_kernel() 1 or 2) is followed by a masked launch of the
        Givens / TQ kernel that takes over the members they give up on at set-up, as a single Solver re-solves such a call
        (rsqp_batch_set_handover); off (the default): those members come back unsolved"""
        check(lib().rsqp_batch_set_handover(self._h, int(bool(on))))

    def set_lane_warm(self, on):
        """on: a batch the lane-per-problem kernel takes (last_kernel() 2 for its cold start) and that keeps its state also runs its
        hot starts with new matrices, its warm re-initialisations and the first solve of an optimize_qp() that follows
        set_matrix_values() on that kernel (rsqp_batch_set_lane_warm); off (the default): on the 8-lane kernel, as before"""
        check(lib().rsqp_batch_set_lane_warm(self._h, int(bool(on))))

    def lane_warm(self):
        """the switch of set_lane_warm (rsqp_batch_get_lane_warm)"""
        return bool(check(lib().rsqp_batch_get_lane_warm(self._h)))

    def set_lane_hot(self, on):
        """on: while set_lane_warm is on as well (alone this switch changes nothing), a batch the lane-per-problem kernel serves and
        that keeps its state also runs its hot starts on new vectors (solve(MODE_HOT_VECTORS)) and the first solve of every
        optimize_qp() call behind the first -- update marks batch-wide, per member or absent -- on that kernel
        (rsqp_batch_set_lane_hot); off (the default): as before"""
        check(lib().rsqp_batch_set_lane_hot(self._h, int(bool(on))))

    def lane_hot(self):
        """the switch of set_lane_hot (rsqp_batch_get_lane_hot)"""
        return bool(check(lib().rsqp_batch_get_lane_hot(self._h)))

    def handover(self, handed=None):
        """(handed, count) of the last solve / optimize call: handed[q] = 1 where member q was handed over to the Givens / TQ kernel
        (in either solve of an optimize call), count of them (rsqp_batch_get_handover). handed: an int32 array of nq entries to fill"""
        if handed is None:
            handed = np.zeros(self.nq, np.int32)
        elif not (isinstance(handed, np.ndarray) and handed.dtype == np.int32 and handed.ndim == 1 and handed.size == self.nq
                  and handed.flags.c_contiguous):
            raise ValueError("handed: a contiguous int32 array of %d entries, one per member" % self.nq)
        count = C.c_int(0)
        check(lib().rsqp_batch_get_handover(self._h, _ip(handed), C.byref(count)))
        return handed, count.value

    def last_kernel(self):
        """0 LDS null-space kernels, 1 tableau kernel with 8 lanes per problem, 2 lane-per-problem kernel, 3 HBM-resident
        null-space kernel (batches beyond the LDS fit) (rsqp_batch_get_last_kernel)"""
        return lib().rsqp_batch_get_last_kernel(self._h)

    def lane_hblock(self):
        """the lane-per-problem kernel's build of the last launch: 4 = H as its leading 4 x 4 block, 8 = the full triangle
        (RSQP_LANE_HBLOCK=0 forces it), 0 = another kernel ran (rsqp_batch_get_lane_hblock)"""
        return lib().rsqp_batch_get_lane_hblock(self._h)

    def lane_shape(self):
        """8 * 256 + 2 = the last launch ran the lane-per-problem kernel's full-shape build (nV = 8, nC = 2 as compile-time
        constants), 0 = its shape was a run-time value (RSQP_LANE_SHAPE=0 forces it) or another kernel ran (rsqp_batch_get_lane_shape)"""
        return lib().rsqp_batch_get_lane_shape(self._h)

    def last_plan(self):
        """the launch plan of the solve last_kernel() reports, as a dict over SMALL_LAUNCH_OUT: which instantiation ran
        (rsqp_batch_get_last_plan)"""
        out = np.zeros(len(SMALL_LAUNCH_OUT), np.int32)
        check(lib().rsqp_batch_get_last_plan(self._h, _ip(out), len(out)))
        return dict(zip(SMALL_LAUNCH_OUT, out.tolist()))

    def last_solve_ms(self):
        return lib().rsqp_batch_last_solve_ms(self._h)

    def timer_start(self):
        check(lib().rsqp_batch_timer_start(self._h))

    def timer_stop_ms(self):
        return lib().rsqp_batch_timer_stop_ms(self._h)

    def results(self):
        sV, sC = int(self.offV[-1]), int(self.offC[-1])
        x = np.zeros(sV); y = np.zeros(sV + sC); wb = np.zeros(sV, np.int32); wc = np.zeros(sC, np.int32)
        st = np.zeros(self.nq, np.int32); nw = np.zeros(self.nq, np.int32); obj = np.zeros(self.nq)
        check(lib().rsqp_batch_get_results(self._h, _dp(x), _dp(y), _ip(wb), _ip(wc), _ip(st), _ip(nw), _dp(obj)))
        out = []
        for q in range(self.nq):
            v0, v1, c0, c1 = self.offV[q], self.offV[q + 1], self.offC[q], self.offC[q + 1]
            yo = v0 + c0
            out.append(dict(x=x[v0:v1], y=y[yo:yo + (v1 - v0) + (c1 - c0)], ws_b=wb[v0:v1], ws_c=wc[c0:c1],
                            status=int(st[q]), nWSR=int(nw[q]), obj=float(obj[q])))
        return out

    @property
    def record_stride(self):
        return lib().rsqp_batch_record_stride(self._h)

    def pack_records_dev(self, dev_ptr):
        """fixed-stride result records (parallel.pack_records layout) into device memory at `dev_ptr`
        (nq * record_stride doubles, e.g. a torch tensor's data_ptr()); asynchronous on the batch's stream"""
        check(lib().rsqp_batch_pack_records_dev(self._h, C.c_void_p(dev_ptr)))

    def pack_records(self):
        """the same records, packed on the device and copied to the host: array [nq, record_stride]"""
        out = np.zeros(self.nq * self.record_stride)
        check(lib().rsqp_batch_pack_records_host(self._h, _dp(out)))
        return out.reshape(self.nq, self.record_stride)

    def test_optimality(self):
        st = (OptimalityStatus * self.nq)()
        ok = np.zeros(self.nq, np.int32)
        check(lib().rsqp_batch_test_optimality(self._h, C.cast(st, C.c_void_p), _ip(ok)))
        return ok, [st[q].KKT_error for q in range(self.nq)]

    CERTIFICATE_FIELDS = ("primal_violation", "dual_violation", "compl_violation", "stationarity_violation", "KKT_error")

    def certificates(self):
        """the whole certificate of every member: (ok, fields) with ok[q] = 1 optimal / 0 not / ERR_WORKING_SET and fields an array
        [nq, 5] over CERTIFICATE_FIELDS (rsqp_batch_test_optimality)"""
        st = (OptimalityStatus * self.nq)()
        ok = np.zeros(self.nq, np.int32)
        check(lib().rsqp_batch_test_optimality(self._h, C.cast(st, C.c_void_p), _ip(ok)))
        return ok, np.array([[getattr(st[q], f) for f in self.CERTIFICATE_FIELDS] for q in range(self.nq)]).reshape(self.nq, 5)

    def mapped_working_sets(self):
        """(W_b, W_c) per member as the last certificate mapped them (rsqp_batch_get_working_set)"""
        Wb, Wc = np.zeros(int(self.offV[-1]), np.int32), np.zeros(int(self.offC[-1]), np.int32)
        check(lib().rsqp_batch_get_working_set(self._h, _ip(Wb), _ip(Wc)))
        return [(Wb[self.offV[q]:self.offV[q + 1]], Wc[self.offC[q]:self.offC[q + 1]]) for q in range(self.nq)]

    def set_results(self, x=None, y=None, ws_b=None, ws_c=None):
        """verification: overwrite the result pools (the layout of rsqp_batch_get_results: x and ws_b sum(nV) entries, y member by
        member bounds then constraints, ws_c sum(nC)); None leaves a pool as it is (rsqp_batch_set_results)"""
        sV, sC = int(self.offV[-1]), int(self.offC[-1])
        x, y = self._sized(x, sV, "x"), self._sized(y, sV + sC, "y")
        ws_b, ws_c = self._sized(ws_b, sV, "ws_b", np.int32), self._sized(ws_c, sC, "ws_c", np.int32)
        check(lib().rsqp_batch_set_results(self._h, _dp(x), _dp(y), _ip(ws_b), _ip(ws_c)))

    def allgather_records(self, comm, count_per_rank, all_dev_ptr):
        """native RCCL: pack this rank's records into its slot of the DEVICE buffer at `all_dev_ptr`
        (world * count_per_rank * record_stride doubles) and all-gather in place; returns when done"""
        check(lib().rsqp_batch_allgather_records(self._h, comm._h, int(count_per_rank), C.c_void_p(all_dev_ptr)))


def rccl_unique_id():
    """ncclGetUniqueId through the C ABI: 128 bytes that rank 0 ships to every other rank"""
    buf = C.create_string_buffer(128)
    check(lib().rsqp_rccl_unique_id(buf))
    return buf.raw


class RcclComm(_Handle):
    """an ncclComm_t created through the C ABI (rsqp_rccl_comm_create): one per rank, bound to `device`; closed by close() alone"""
    DESTROY = "rsqp_rccl_comm_destroy"

    def __init__(self, uid, rank, world, device):
        c = C.c_void_p()
        check(lib().rsqp_rccl_comm_create(C.create_string_buffer(bytes(uid), 128), rank, world, device, C.byref(c)))
        self._h, self.rank, self.world = c, rank, world

    def broadcast_dev(self, dev_ptr, nbytes, root=0, stream=None):
        check(lib().rsqp_rccl_broadcast_dev(self._h, C.c_void_p(dev_ptr), int(nbytes), root, C.c_void_p(stream or 0)))


class SpmvPlan(_Handle):
    DESTROY = "rsqp_spmv_plan_destroy"
    __del__ = _Handle.close

    def __init__(self, nrow, ncol, jc, ir, nbatch, device=-1):
        jc, ir = _i(jc), _i(ir)
        self.nrow, self.ncol, self.nnz, self.nbatch = nrow, ncol, int(jc[ncol]), nbatch
        h = C.c_void_p()
        check(lib().rsqp_spmv_plan_create(nrow, ncol, _ip(jc), _ip(ir), nbatch, device, C.byref(h)))
        self._h = h

    def upload(self, vals=None, xin=None, transposed=False):
        vals, xin = _d(vals), _d(xin)
        check(lib().rsqp_spmv_plan_upload(self._h, _dp(vals), _dp(xin), int(transposed)))

    def run(self, transposed=False, repeats=1):
        ms = C.c_float(0)
        check(lib().rsqp_spmv_plan_run(self._h, int(transposed), repeats, C.byref(ms)))
        return ms.value

    def variant(self, transposed=False):
        """(kernel code, uses 16-bit indices) of the product -- see rsqp_spmv_plan_variant."""
        i16 = C.c_int(0)
        v = check(lib().rsqp_spmv_plan_variant(self._h, int(transposed), C.byref(i16)))
        return v, bool(i16.value)

    def download(self, transposed=False):
        out = np.zeros(self.nbatch * (self.ncol if transposed else self.nrow))
        check(lib().rsqp_spmv_plan_download(self._h, _dp(out), int(transposed)))
        return out.reshape(self.nbatch, -1)
