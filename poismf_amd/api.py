"""Python host side above the C-ABI (include/poismf_hip.h).

Mirrors the reference's binding layer for this path:

* ``_run_poismf``  -- same positional order, defaults, checks and exceptions as the Cython entry point
  (ref: poismf/poismf_c_wrapper.pxi:57-107; note *indices before indptr* here, the reverse of the C
  signature it forwards to);
* ``PoisMF``       -- the fit-path subset of the reference class (ref: poismf/__init__.py:205-232
  constructor, :336-374 ``fit``, :427-439 ``_fit``, :441-495 ``fit_unsafe``);
* ``Session``      -- the device-resident half-sweep API used by bench.py and the multi-GPU driver.

There is no CPU fallback anywhere in this module: if the HIP library cannot be loaded, or there is no
GPU, the calls raise.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build
from . import harness
from . import serving
# the serving calls' argument checks and helpers live in serving.py; every name stays reachable here
from .serving import (_batch_rc, _csr_list, _diverse_outputs, _eval_lists_args, _eval_ranking_args, _include_of_rows, _include_rows,
                      _index_array, _inv_norms, _list_eval_args, _list_eval_outputs, _list_eval_scratch, _list_rows, _new_rows_args, _append_rows_args,
                      _new_stats, _opt_ptr, _outside_shard, _ptr, _rank_batch_args, _rank_include_list, _shared_table_args,
                      _similar_args, _similar_scores, _topn_adjusted_args, _topn_batch_args, _topn_deep_args, _topn_diverse_args,
                      _topn_include_args, _topn_outputs, _topn_quota_args, _topn_shared_args, _topn_weighted_args, _unite_rows)

_METHOD = {"tncg": 1, "cg": 2, "pg": 3}  # ref: src/poismf.h:225
_LIBS = {}


class poismf_hip_params(C.Structure):
    pass


def _params_type(c_real):
    class Params(C.Structure):
        _fields_ = [("l2_reg", c_real), ("l1_reg", c_real), ("w_mult", c_real), ("step_size", c_real),
                    ("method", C.c_int), ("limit_step", C.c_int), ("maxupd", C.c_size_t),
                    ("early_stop", C.c_int), ("reuse_prev", C.c_int)]
    return Params


# every symbol include/poismf_hip.h declares
EXPORTED_SYMBOLS = (
    "run_poismf", "factors_multiple", "poismf_hip_coo_to_csr_csc", "predict_multiple", "topN", "poismf_hip_session_create", "poismf_hip_session_destroy", "poismf_hip_session_A",
    "poismf_hip_session_B", "poismf_hip_session_set_factors", "poismf_hip_session_get_factors",
    "poismf_hip_half_sweep", "poismf_hip_session_profile", "poismf_hip_session_kernel_time",
    "poismf_hip_session_nnz", "poismf_hip_selftest_log", "poismf_hip_session_eval_stats",
    "poismf_hip_session_create_coo", "poismf_hip_session_stream", "poismf_hip_session_factors_dirty", "poismf_hip_session_run",
    "poismf_hip_session_set_segments", "poismf_hip_session_segment_rows", "poismf_hip_half_sweep_segment", "poismf_hip_session_plan",
    "poismf_hip_session_add_coo", "poismf_hip_session_get_matrix", "poismf_hip_half_sweep_rows",
    "poismf_hip_session_sub_coo", "poismf_hip_session_remove_rows",
    "poismf_hip_session_append_rows", "poismf_hip_session_adopt_new",
    "poismf_hip_session_scale",
    "poismf_hip_session_launch_profile", "poismf_hip_session_decisions", "poismf_hip_session_decision_stats", "poismf_hip_factors_multiple_decisions",
    "poismf_hip_session_predict", "poismf_hip_session_topn", "poismf_hip_debug_row_eval", "poismf_hip_release_cache",
    "poismf_hip_set_device_cache_mb", "poismf_hip_session_colsum_blocks", "poismf_hip_session_colsum_partial", "poismf_hip_session_partials",
    "poismf_hip_session_partials_ready", "eval_llk", "poismf_hip_session_llk", "poismf_hip_debug_plan",
    "poismf_hip_debug_plan_widths", "poismf_hip_debug_plan_engines", "poismf_hip_debug_plan_missing", "poismf_hip_debug_lane_full_width", "poismf_hip_debug_reg_quad_off",
    "poismf_hip_topn_batch", "poismf_hip_session_topn_batch", "poismf_hip_topn_batch_scratch_bytes",
    "poismf_hip_rank_batch", "poismf_hip_session_rank_batch", "poismf_hip_rank_batch_scratch_bytes",
    "poismf_hip_rank_include", "poismf_hip_session_rank_include", "poismf_hip_rank_include_scratch_bytes",
    "poismf_hip_topn_include", "poismf_hip_session_topn_include", "poismf_hip_topn_include_scratch_bytes", "poismf_hip_topn_include_slice",
    "poismf_hip_topn_shared", "poismf_hip_session_topn_shared", "poismf_hip_topn_shared_scratch_bytes",
    "poismf_hip_rank_shared", "poismf_hip_session_rank_shared", "poismf_hip_rank_shared_scratch_bytes",
    "poismf_hip_topn_deep", "poismf_hip_session_topn_deep", "poismf_hip_topn_deep_scratch_bytes",
    "poismf_hip_session_factors_new", "poismf_hip_session_topn_new", "poismf_hip_session_rank_new", "poismf_hip_topn_new",
    "poismf_hip_topn_quota", "poismf_hip_session_topn_quota", "poismf_hip_topn_quota_scratch_bytes",
    "poismf_hip_topn_weighted", "poismf_hip_session_topn_weighted", "poismf_hip_topn_weighted_scratch_bytes",
    "poismf_hip_topn_diverse", "poismf_hip_session_topn_diverse", "poismf_hip_topn_diverse_scratch_bytes",
    "poismf_hip_list_eval", "poismf_hip_session_list_eval", "poismf_hip_list_eval_scratch_bytes",
    "poismf_hip_topn_adjusted", "poismf_hip_session_topn_adjusted", "poismf_hip_topn_adjusted_scratch_bytes", "poismf_hip_topn_adjusted_slices",
)
TOPN_BATCH_MAX_N_TOP = 128   # POISMF_HIP_TOPN_BATCH_MAX_N_TOP of include/poismf_hip.h (tests/test_topn_batch_cpu.py compares the two)
RANK_EXCLUDED = 0xFFFFFFFF   # the rank-excluded mark, RANK_BATCH_MAX_ROW the longest held-out row and RANK_BATCH_BUDGET_MB the scratch bound
RANK_BATCH_MAX_ROW = 65536   # of include/poismf_hip.h section 1g (tests/test_rank_batch_cpu.py compares them with the header)
RANK_BATCH_BUDGET_MB = 256
RANK_INCLUDE_SLICE = 1024    # POISMF_HIP_RANK_INCLUDE_SLICE and _GROUP of section 1j (tests/test_rank_include_cpu.py compares them with the header)
RANK_INCLUDE_GROUP = 128
TOPN_NONE = 2**64 - 1               # POISMF_HIP_TOPN_NONE and POISMF_HIP_TOPN_INCLUDE_MAX_ROW of include/poismf_hip.h section 1h
TOPN_INCLUDE_MAX_ROW = 16777216     # (tests/test_topn_include_cpu.py compares them with the header)
TOPN_SHARED_MAX_CELLS = 2**24       # POISMF_HIP_TOPN_SHARED_MAX_CELLS of section 1i (tests/test_topn_shared_cpu.py compares the two)
RANK_SHARED_CHUNK_CELLS = 2**19     # POISMF_HIP_RANK_SHARED_CHUNK_CELLS of section 1k (tests/test_rank_shared_cpu.py compares the two)
TOPN_DEEP_MAX_N_TOP = 1024          # POISMF_HIP_TOPN_DEEP_MAX_N_TOP and POISMF_HIP_TOPN_DEEP_BUDGET_MB of section 1l
TOPN_DEEP_BUDGET_MB = 1024          # (tests/test_topn_deep_cpu.py compares them with the header)
TOPN_QUOTA_MAX_ITEMS = 2**24        # POISMF_HIP_TOPN_QUOTA_MAX_ITEMS of section 1n (tests/test_topn_quota_cpu.py compares the two)
TOPN_WEIGHTED_MAX_ITEMS = 2**24     # POISMF_HIP_TOPN_WEIGHTED_MAX_ITEMS of section 1o (tests/test_topn_weighted_cpu.py compares the two)
TOPN_DIVERSE_MAX_ITEMS = 2**24      # POISMF_HIP_TOPN_DIVERSE_MAX_ITEMS and POISMF_HIP_TOPN_DIVERSE_BUDGET_MB of section 1p
TOPN_DIVERSE_BUDGET_MB = 1152       # (tests/test_topn_diverse_cpu.py compares them with the header)
LIST_ABSENT = 0xFFFFFFFE            # POISMF_HIP_LIST_ABSENT, POISMF_HIP_LIST_COS_SHIFT, POISMF_HIP_LIST_EVAL_BUDGET_MB and
LIST_COS_SHIFT = 40                 # POISMF_HIP_LIST_EVAL_MAX_ITEMS of section 1q (tests/test_list_eval_cpu.py compares them with
LIST_EVAL_BUDGET_MB = 256           # the header)
LIST_EVAL_MAX_ITEMS = 2**24
TOPN_ADJUSTED_MAX_ITEMS = 2**24     # POISMF_HIP_TOPN_ADJUSTED_MAX_ITEMS and POISMF_HIP_TOPN_ADJUSTED_MAX_ROW of section 1r
TOPN_ADJUSTED_MAX_ROW = 2**22       # (tests/test_topn_adjusted_cpu.py compares them with the header)


def load_library(use_float):
    """dlopen libpoismf_hip_{d,f}.so (built in-tree by poismf_amd.build) and declare its prototypes.  use_float = "r" loads
    libpoismf_hip_r.so, the reference's R ABI (int indices, double): same prototypes, index arrays are int32."""
    key = "r" if use_float == "r" else bool(use_float)
    if key in _LIBS:
        return _LIBS[key]
    path = _build.lib_path(key)
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: build it with `python -m poismf_amd.build` "
                           "(there is no CPU fallback for this path)")
    lib = C.CDLL(path)
    r = C.c_float if key is True else C.c_double
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    lib.run_poismf.argtypes = [vp] * 8 + [sz] * 3 + [r] * 4 + [i, C.c_bool, sz, sz] + [C.c_bool] * 3 + [i]
    lib.run_poismf.restype = i
    lib.factors_multiple.argtypes = [vp] * 7 + [i, sz, r, r, r, sz, sz, i, C.c_bool, C.c_bool, i]
    lib.factors_multiple.restype = i
    lib.poismf_hip_factors_multiple_decisions.argtypes = [vp] * 7 + [i, sz, r, r, r, sz, sz, i, C.c_bool, C.c_bool, vp]
    lib.poismf_hip_factors_multiple_decisions.restype = i
    lib.poismf_hip_session_decisions.argtypes = [vp, i, vp, sz]
    lib.poismf_hip_session_decisions.restype = i
    lib.poismf_hip_session_decision_stats.argtypes = [vp, i, C.POINTER(C.c_ulonglong)]
    lib.poismf_hip_session_decision_stats.restype = i
    lib.poismf_hip_release_cache.argtypes = []
    lib.poismf_hip_release_cache.restype = None
    lib.poismf_hip_set_device_cache_mb.argtypes = [sz]
    lib.poismf_hip_set_device_cache_mb.restype = sz
    lib.poismf_hip_session_colsum_blocks.argtypes = [vp, i]
    lib.poismf_hip_session_colsum_blocks.restype = i
    lib.poismf_hip_session_colsum_partial.argtypes = [vp, i, i, i]
    lib.poismf_hip_session_colsum_partial.restype = i
    lib.poismf_hip_session_partials.argtypes = [vp]
    lib.poismf_hip_session_partials.restype = vp
    lib.poismf_hip_session_partials_ready.argtypes = [vp]
    lib.poismf_hip_session_partials_ready.restype = None
    lib.predict_multiple.argtypes = [vp, vp, vp, vp, vp, sz, i, i]
    lib.predict_multiple.restype = None
    lib.topN.argtypes = [vp, vp, i, vp, sz, vp, sz, vp, vp, sz, sz, i]
    lib.topN.restype = i
    lib.poismf_hip_coo_to_csr_csc.argtypes = [vp, vp, vp, sz, sz, sz] + [vp] * 6 + [C.POINTER(sz)]
    lib.poismf_hip_coo_to_csr_csc.restype = i
    lib.poismf_hip_session_create.argtypes = [C.POINTER(vp), i, vp] + [vp] * 6 + [sz] * 3 + [sz] * 4
    lib.poismf_hip_session_create.restype = i
    lib.poismf_hip_session_create_coo.argtypes = [C.POINTER(vp), i, vp, vp, vp, vp, sz] + [sz] * 3 + [sz] * 4
    lib.poismf_hip_session_create_coo.restype = i
    lib.poismf_hip_session_destroy.argtypes = [vp]
    lib.poismf_hip_session_destroy.restype = None
    lib.poismf_hip_session_stream.argtypes = [vp]
    lib.poismf_hip_session_stream.restype = vp
    lib.poismf_hip_session_factors_dirty.argtypes = [vp, i]
    lib.poismf_hip_session_factors_dirty.restype = None
    for name in ("poismf_hip_session_A", "poismf_hip_session_B"):
        getattr(lib, name).argtypes = [vp]
        getattr(lib, name).restype = vp
    for name in ("poismf_hip_session_set_factors", "poismf_hip_session_get_factors"):
        getattr(lib, name).argtypes = [vp, vp, vp]
        getattr(lib, name).restype = i
    lib.params_t = _params_type(r)
    lib.poismf_hip_half_sweep.argtypes = [vp, i, C.POINTER(lib.params_t), r, r, C.POINTER(sz)]
    lib.poismf_hip_half_sweep.restype = i
    lib.poismf_hip_session_set_segments.argtypes = [vp, i, i]
    lib.poismf_hip_session_set_segments.restype = i
    lib.poismf_hip_session_segment_rows.argtypes = [vp, i, i, C.POINTER(sz), C.POINTER(sz)]
    lib.poismf_hip_session_segment_rows.restype = i
    lib.poismf_hip_half_sweep_segment.argtypes = [vp, i, C.POINTER(lib.params_t), r, r, i, C.POINTER(sz)]
    lib.poismf_hip_half_sweep_segment.restype = i
    lib.poismf_hip_session_add_coo.argtypes = [vp, vp, vp, vp, sz, C.POINTER(sz)]
    lib.poismf_hip_session_add_coo.restype = i
    lib.poismf_hip_session_sub_coo.argtypes = [vp, vp, vp, vp, sz, i, C.POINTER(sz), C.POINTER(sz)]
    lib.poismf_hip_session_sub_coo.restype = i
    lib.poismf_hip_session_remove_rows.argtypes = [vp, i, vp, sz, C.POINTER(sz)]
    lib.poismf_hip_session_remove_rows.restype = i
    lib.poismf_hip_session_append_rows.argtypes = [vp, i, sz, vp, vp, vp, vp, C.POINTER(sz)]
    lib.poismf_hip_session_append_rows.restype = i
    lib.poismf_hip_session_adopt_new.argtypes = [vp, C.POINTER(sz), C.POINTER(sz)]
    lib.poismf_hip_session_adopt_new.restype = i
    lib.poismf_hip_session_scale.argtypes = [vp, r, vp, vp, r, C.POINTER(sz)]
    lib.poismf_hip_session_scale.restype = i
    lib.poismf_hip_session_get_matrix.argtypes = [vp, i, vp, vp, vp]
    lib.poismf_hip_session_get_matrix.restype = i
    lib.poismf_hip_half_sweep_rows.argtypes = [vp, i, vp, sz, C.POINTER(lib.params_t), r, r, C.POINTER(sz)]
    lib.poismf_hip_half_sweep_rows.restype = i
    lib.poismf_hip_session_predict.argtypes = [vp, vp, vp, sz, vp]
    lib.poismf_hip_session_predict.restype = i
    lib.eval_llk.argtypes = [vp] * 5 + [sz, i, C.c_bool, C.c_bool, sz, sz, i]
    lib.eval_llk.restype = C.c_longdouble
    lib.poismf_hip_session_llk.argtypes = [vp, i, i, C.POINTER(C.c_double)]
    lib.poismf_hip_session_llk.restype = i
    lib.poismf_hip_session_topn.argtypes = [vp, sz, vp, sz, vp, sz, vp, vp, sz]
    lib.poismf_hip_session_topn.restype = i
    lib.poismf_hip_topn_batch.argtypes = [vp, vp, i, sz, sz, vp, sz, sz, vp, vp, vp, vp]
    lib.poismf_hip_topn_batch.restype = i
    lib.poismf_hip_session_topn_batch.argtypes = [vp, vp, sz, sz, i, vp, vp, vp, vp]
    lib.poismf_hip_session_topn_batch.restype = i
    lib.poismf_hip_topn_batch_scratch_bytes.argtypes = [sz, sz, sz, sz]
    lib.poismf_hip_topn_batch_scratch_bytes.restype = sz
    lib.poismf_hip_topn_deep.argtypes = [vp, vp, i, sz, sz, vp, sz, sz, vp, vp, vp, vp]
    lib.poismf_hip_topn_deep.restype = i
    lib.poismf_hip_session_topn_deep.argtypes = [vp, vp, sz, sz, i, vp, vp, vp, vp]
    lib.poismf_hip_session_topn_deep.restype = i
    lib.poismf_hip_topn_deep_scratch_bytes.argtypes = [sz, sz, sz, sz]
    lib.poismf_hip_topn_deep_scratch_bytes.restype = sz
    lib.poismf_hip_topn_quota.argtypes = [vp, vp, i, sz, sz, vp, sz, sz, vp, sz, vp, vp, vp, vp, vp]
    lib.poismf_hip_topn_quota.restype = i
    lib.poismf_hip_session_topn_quota.argtypes = [vp, vp, sz, sz, vp, sz, vp, i, vp, vp, vp, vp]
    lib.poismf_hip_session_topn_quota.restype = i
    lib.poismf_hip_topn_quota_scratch_bytes.argtypes = [sz, sz, sz, sz, sz]
    lib.poismf_hip_topn_quota_scratch_bytes.restype = sz
    lib.poismf_hip_topn_weighted.argtypes = [vp, vp, i, sz, sz, vp, sz, sz, vp, vp, vp, vp, vp]
    lib.poismf_hip_topn_weighted.restype = i
    lib.poismf_hip_session_topn_weighted.argtypes = [vp, vp, sz, sz, vp, i, i, vp, vp, vp, vp]
    lib.poismf_hip_session_topn_weighted.restype = i
    lib.poismf_hip_topn_weighted_scratch_bytes.argtypes = [sz, sz, sz, sz]
    lib.poismf_hip_topn_weighted_scratch_bytes.restype = sz
    lib.poismf_hip_topn_adjusted.argtypes = [vp, vp, i, sz, sz, vp, sz, sz, vp, vp, vp, vp, vp, vp, vp]
    lib.poismf_hip_topn_adjusted.restype = i
    lib.poismf_hip_session_topn_adjusted.argtypes = [vp, vp, sz, sz, vp, vp, vp, i, vp, vp, vp, vp]
    lib.poismf_hip_session_topn_adjusted.restype = i
    lib.poismf_hip_topn_adjusted_scratch_bytes.argtypes = [sz, sz, sz, sz, sz]
    lib.poismf_hip_topn_adjusted_scratch_bytes.restype = sz
    lib.poismf_hip_topn_adjusted_slices.argtypes = [sz, sz, i]
    lib.poismf_hip_topn_adjusted_slices.restype = sz
    lib.poismf_hip_topn_diverse.argtypes = [vp, vp, i, sz, sz, vp, sz, sz, sz, C.c_double, vp, vp, vp, vp, vp, vp]
    lib.poismf_hip_topn_diverse.restype = i
    lib.poismf_hip_session_topn_diverse.argtypes = [vp, vp, sz, sz, sz, C.c_double, vp, i, vp, vp, vp, vp, vp]
    lib.poismf_hip_session_topn_diverse.restype = i
    lib.poismf_hip_topn_diverse_scratch_bytes.argtypes = [sz, sz, sz, sz, sz]
    lib.poismf_hip_topn_diverse_scratch_bytes.restype = sz
    lib.poismf_hip_list_eval.argtypes = [vp, i, sz, vp, sz, sz, vp, vp, vp, sz, vp, vp, vp, vp]
    lib.poismf_hip_list_eval.restype = i
    lib.poismf_hip_session_list_eval.argtypes = [vp, vp, sz, sz, vp, vp, vp, sz, vp, vp, vp, vp]
    lib.poismf_hip_session_list_eval.restype = i
    lib.poismf_hip_list_eval_scratch_bytes.argtypes = [sz, sz, sz, sz, sz]
    lib.poismf_hip_list_eval_scratch_bytes.restype = sz
    lib.poismf_hip_rank_batch.argtypes = [vp, vp, i, sz, sz, vp, sz, vp, vp, vp, vp, vp, vp]
    lib.poismf_hip_rank_batch.restype = i
    lib.poismf_hip_session_rank_batch.argtypes = [vp, vp, sz, vp, vp, i, vp, vp, vp, vp]
    lib.poismf_hip_session_rank_batch.restype = i
    lib.poismf_hip_rank_batch_scratch_bytes.argtypes = [sz, sz, sz, sz]
    lib.poismf_hip_rank_batch_scratch_bytes.restype = sz
    lib.poismf_hip_rank_include.argtypes = [vp, vp, i, sz, sz, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.poismf_hip_rank_include.restype = i
    lib.poismf_hip_session_rank_include.argtypes = [vp, vp, sz, vp, vp, vp, vp, i, vp, vp, vp, vp]
    lib.poismf_hip_session_rank_include.restype = i
    lib.poismf_hip_rank_include_scratch_bytes.argtypes = [sz, sz, sz, sz, sz]
    lib.poismf_hip_rank_include_scratch_bytes.restype = sz
    lib.poismf_hip_topn_include.argtypes = [vp, vp, i, sz, sz, vp, sz, sz, vp, vp, vp, vp, vp, vp]
    lib.poismf_hip_topn_include.restype = i
    lib.poismf_hip_session_topn_include.argtypes = [vp, vp, sz, sz, vp, vp, i, vp, vp, vp, vp]
    lib.poismf_hip_session_topn_include.restype = i
    lib.poismf_hip_topn_include_scratch_bytes.argtypes = [sz, sz, sz, sz, sz]
    lib.poismf_hip_topn_include_scratch_bytes.restype = sz
    lib.poismf_hip_topn_include_slice.argtypes = [sz, sz]
    lib.poismf_hip_topn_include_slice.restype = sz
    lib.poismf_hip_topn_shared.argtypes = [vp, vp, i, sz, sz, vp, sz, sz, vp, vp, sz, vp, vp, vp, vp, vp]
    lib.poismf_hip_topn_shared.restype = i
    lib.poismf_hip_session_topn_shared.argtypes = [vp, vp, sz, sz, vp, vp, sz, vp, i, vp, vp, vp, vp]
    lib.poismf_hip_session_topn_shared.restype = i
    lib.poismf_hip_topn_shared_scratch_bytes.argtypes = [sz, sz, sz, sz, sz, sz]
    lib.poismf_hip_topn_shared_scratch_bytes.restype = sz
    lib.poismf_hip_rank_shared.argtypes = [vp, vp, i, sz, sz, vp, sz, vp, vp, vp, vp, sz, vp, i, vp, vp, vp, vp]
    lib.poismf_hip_rank_shared.restype = i
    lib.poismf_hip_session_rank_shared.argtypes = [vp, vp, sz, vp, vp, vp, vp, sz, vp, i, i, vp, vp, vp, vp]
    lib.poismf_hip_session_rank_shared.restype = i
    lib.poismf_hip_rank_shared_scratch_bytes.argtypes = [sz, sz, sz, sz, sz, sz]
    lib.poismf_hip_rank_shared_scratch_bytes.restype = sz
    new_rows = [vp, vp, vp, vp, sz, vp, vp, C.POINTER(lib.params_t), sz]   # session, Xr, indptr, indices, n_new, Bsum, Amean, p, niter
    lib.poismf_hip_session_factors_new.argtypes = new_rows + [vp]
    lib.poismf_hip_session_factors_new.restype = i
    lib.poismf_hip_session_topn_new.argtypes = new_rows + [sz, i, vp, vp, vp, vp, vp]
    lib.poismf_hip_session_topn_new.restype = i
    lib.poismf_hip_session_rank_new.argtypes = new_rows + [vp, vp, i, vp, vp, vp, vp, vp]
    lib.poismf_hip_session_rank_new.restype = i
    lib.poismf_hip_topn_new.argtypes = [vp] * 6 + [i, sz, sz, r, r, r, sz, sz, i, C.c_bool, C.c_bool, sz, i, vp, vp, vp, vp, vp]
    lib.poismf_hip_topn_new.restype = i
    lib.poismf_hip_session_plan.argtypes = [vp, i, C.c_char_p, sz]
    lib.poismf_hip_session_plan.restype = sz
    lib.poismf_hip_session_launch_profile.argtypes = [vp, i, C.c_char_p, sz]
    lib.poismf_hip_session_launch_profile.restype = sz
    lib.poismf_hip_session_run.argtypes = [vp, C.POINTER(lib.params_t), sz, i]
    lib.poismf_hip_session_run.restype = i
    lib.poismf_hip_session_profile.argtypes = [vp, i]
    lib.poismf_hip_session_profile.restype = None
    lib.poismf_hip_session_kernel_time.argtypes = [vp, i, C.POINTER(C.c_double), C.POINTER(sz)]
    lib.poismf_hip_session_kernel_time.restype = i
    lib.poismf_hip_session_nnz.argtypes = [vp, i]
    lib.poismf_hip_session_nnz.restype = sz
    lib.poismf_hip_selftest_log.argtypes = [sz, C.POINTER(C.c_ulonglong), C.POINTER(C.c_uint)]
    lib.poismf_hip_selftest_log.restype = i
    lib.poismf_hip_session_eval_stats.argtypes = [vp, i, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    lib.poismf_hip_session_eval_stats.restype = i
    lib.real_t = r
    _LIBS[key] = lib
    return lib


def release_cache(use_float=None):
    """Hand the device arrays the library keeps from finished calls (only when the caller opted in, see set_device_cache_mb) back
    to the driver.  use_float = None: every flavour loaded in this process (each shared library keeps its own list)."""
    for key, lib in list(_LIBS.items()):
        if use_float is None or key == ("r" if use_float == "r" else bool(use_float)):
            lib.poismf_hip_release_cache()


def set_device_cache_mb(mb, use_float=None):
    """Opt in (mb > 0) to / out (0, the default) of keeping released device arrays for the next call: the reference frees everything
    before run_poismf returns (ref src/poismf.c:610-619) and so does this library unless told otherwise here or through
    POISMF_HIP_DEVICE_CACHE_MB.  Returns {flavour: previous limit in MB}.  use_float = None: every flavour ALREADY loaded in this process (as
    release_cache does; nothing is loaded -- or built -- for the sake of a limit); a named flavour is loaded if need be."""
    if use_float is None:
        return {k_: int(lib.poismf_hip_set_device_cache_mb(int(mb))) for k_, lib in list(_LIBS.items())}
    key = "r" if use_float == "r" else bool(use_float)
    return {key: int(load_library(key).poismf_hip_set_device_cache_mb(int(mb)))}


def _check_arrays(use_float, reals, idx):
    dt = np.float32 if use_float else np.float64
    for a in reals:
        if a.dtype != dt or not a.flags["C_CONTIGUOUS"]:
            raise TypeError(f"expected C-contiguous {dt.__name__} arrays")
    for a in idx:
        if a.dtype != np.uint64 or not a.flags["C_CONTIGUOUS"]:
            raise TypeError("index arrays must be C-contiguous size_t (uint64)")


def _run_poismf(Xr, Xr_indices, Xr_indptr, Xc, Xc_indices, Xc_indptr, A, B, method="tncg", limit_step=0,
                l2_reg=1e9, l1_reg=0, w_mult=1., step_size=1e-7, niter=10, maxupd=1, early_stop=1,
                reuse_prev=1, handle_interrupt=1, nthreads=1):
    """Drop-in for c_funs_{float,double}._run_poismf (ref: poismf/poismf_c_wrapper.pxi:57-107).
    The precision is taken from A's dtype (the reference ships one module per precision)."""
    if Xr.shape[0] == 0:
        raise ValueError("'X' contains no non-zero entries.")                      # ref: pxi:74
    INT_MAX = np.iinfo(C.c_int).max
    if max(A.shape[0], A.shape[1], B.shape[0]) > INT_MAX:                           # ref: pxi:78-80
        raise ValueError("Error: integer overflow. Dimensions cannot be larger than 2^31-1.")
    use_float = A.dtype == np.float32
    _check_arrays(use_float, (Xr, Xc, A, B), (Xr_indices, Xr_indptr, Xc_indices, Xc_indptr))
    lib = load_library(use_float)
    c_method = _METHOD.get(method, 1)                                               # ref: pxi:85-91
    ret = lib.run_poismf(_ptr(A), _ptr(Xr), _ptr(Xr_indptr), _ptr(Xr_indices),
                         _ptr(B), _ptr(Xc), _ptr(Xc_indptr), _ptr(Xc_indices),
                         A.shape[0], B.shape[0], A.shape[1], l2_reg, l1_reg, w_mult, step_size, c_method,
                         bool(limit_step), int(niter), int(maxupd), bool(early_stop), bool(reuse_prev),
                         bool(handle_interrupt), int(nthreads))
    if ret == 1:
        raise MemoryError("Could not allocate enough memory.")                      # ref: pxi:104-105
    elif ret == 2 and not handle_interrupt:
        raise InterruptedError("Procedure was interrupted")                         # ref: pxi:106-107
    return ret


def _coo_arrays(coo, use_float):
    """(row, col, val) of a COO-like object as C-contiguous size_t / size_t / real_t arrays (no copy when they already are;
    non-negative int64 indices are reinterpreted in place)"""
    def ix(a):
        a = np.asarray(a)
        if a.dtype == np.int64 and a.flags["C_CONTIGUOUS"]:
            return a.view(np.uint64)
        return np.ascontiguousarray(a, dtype=np.uint64)
    return ix(coo.row), ix(coo.col), np.ascontiguousarray(coo.data, dtype=np.float32 if use_float else np.float64)


def coo_to_csr_csc(coo, use_float):
    """GPU replacement of harness.process_data (ref: poismf/__init__.py:404-414): SciPy COO -> (csr, csc) tuples of
    (data real_t, indices size_t, indptr size_t) with indices sorted and duplicates summed by the rule of section 1c of
    include/poismf_hip.h (a cell's triplets added in input order).  ValueError for an index outside the matrix."""
    lib = load_library(use_float)
    dt = np.float32 if use_float else np.float64
    n = coo.nnz
    if n == 0:
        raise ValueError("'X' contains no non-zero entries.")
    row, col, val = _coo_arrays(coo, use_float)
    dimA, dimB = coo.shape
    cv, ci, cp = np.empty(n, dt), np.empty(n, np.uint64), np.empty(dimA + 1, np.uint64)
    kv, ki, kp = np.empty(n, dt), np.empty(n, np.uint64), np.empty(dimB + 1, np.uint64)
    nnz = C.c_size_t(0)
    rc = lib.poismf_hip_coo_to_csr_csc(_ptr(row), _ptr(col), _ptr(val), n, dimA, dimB, _ptr(cv), _ptr(ci), _ptr(cp), _ptr(kv),
                                       _ptr(ki), _ptr(kp), C.byref(nnz))
    if rc == 3:
        raise ValueError("a row / column index of the triplets lies outside the matrix")
    if rc:
        raise MemoryError("Could not allocate enough memory.")
    m = nnz.value
    return (cv[:m].copy(), ci[:m].copy(), cp), (kv[:m].copy(), ki[:m].copy(), kp)


def _predict_multiple(out, A, B, ix_u, ix_i, nthreads=1):
    """Drop-in for c_funs._predict_multiple (ref: poismf/poismf_c_wrapper.pxi:109-112): out[i] = A[ix_u[i]] . B[ix_i[i]]."""
    use_float = A.dtype == np.float32
    _check_arrays(use_float, (out, A, B), (ix_u, ix_i))
    load_library(use_float).predict_multiple(_ptr(out), _ptr(A), _ptr(B), _ptr(ix_u), _ptr(ix_i), ix_u.shape[0], A.shape[1],
                                             int(nthreads))


def _call_topN(a_vec, B, include_ix, exclude_ix, top_n=10, output_score=0, nthreads=1):
    """Drop-in for c_funs._call_topN (ref: poismf/poismf_c_wrapper.pxi:207-246): returns (indices, scores)."""
    use_float = B.dtype == np.float32
    _check_arrays(use_float, (a_vec, B), (include_ix, exclude_ix))
    dt = B.dtype
    n_inc = include_ix.shape[0]
    n_exc = 0 if n_inc else exclude_ix.shape[0]
    outp_ix = np.empty(top_n, dtype=np.uint64)
    outp_score = np.empty(top_n if output_score else 0, dtype=dt)
    rc = load_library(use_float).topN(_ptr(a_vec), _ptr(B), B.shape[1], _ptr(include_ix) if n_inc else None, n_inc,
                                      _ptr(exclude_ix) if n_exc else None, n_exc, _ptr(outp_ix),
                                      _ptr(outp_score) if output_score else None, int(top_n), B.shape[0], int(nthreads))
    if rc == 1:
        raise MemoryError("Could not allocate enough memory.")
    if rc == 2:
        raise ValueError("invalid combination of include / exclude / top_n")
    return outp_ix, outp_score


def _predict_factors_multiple(B, Bsum, Amean, Xr_indptr, Xr_indices, Xr, l2_reg=1e9, w_mult=1., step_size=1e-7,
                              niter=10, maxupd=1, method="tncg", limit_step=0, reuse_mean=1, nthreads=1):
    """Drop-in for c_funs_{float,double}._predict_factors_multiple (ref: poismf/poismf_c_wrapper.pxi:147-199):
    same positional order and defaults; returns the new factors A [n_new x k]."""
    use_float = B.dtype == np.float32
    _check_arrays(use_float, (B, Bsum, Amean, Xr), (Xr_indptr, Xr_indices))
    lib = load_library(use_float)
    k = B.shape[1]
    dimA = Xr_indptr.shape[0] - 1
    A = np.empty((dimA, k), dtype=B.dtype)
    ret = lib.factors_multiple(_ptr(A), _ptr(B), _ptr(Bsum), _ptr(Amean), _ptr(Xr) if Xr.shape[0] else None, _ptr(Xr_indptr),
                               _ptr(Xr_indices) if Xr_indices.shape[0] else None, k, dimA, l2_reg, w_mult, step_size,
                               int(niter), int(maxupd), _METHOD.get(method, 1), bool(limit_step), bool(reuse_mean),
                               int(nthreads))
    if ret:
        raise MemoryError("Could not allocate enough memory.")                      # ref: pxi:205-206
    return A


def factors_multiple_with_decisions(B, Bsum, Amean, Xr_indptr, Xr_indices, Xr, l2_reg=1e9, w_mult=1., step_size=1e-7,
                                    niter=10, maxupd=1, method="tncg", limit_step=0, reuse_mean=1):
    """_predict_factors_multiple plus what each row's solver decided: returns (A, iterations, evaluations, rc) -- the
    numbers the reference's minimize_nonneg_cg / tnc hand back (testing aid, include/poismf_hip.h)."""
    use_float = B.dtype == np.float32
    _check_arrays(use_float, (B, Bsum, Amean, Xr), (Xr_indptr, Xr_indices))
    lib = load_library(use_float)
    k = B.shape[1]
    dimA = Xr_indptr.shape[0] - 1
    A = np.empty((dimA, k), dtype=B.dtype)
    dec = np.zeros((dimA, 2), dtype=np.uint32)
    ret = lib.poismf_hip_factors_multiple_decisions(_ptr(A), _ptr(B), _ptr(Bsum), _ptr(Amean), _ptr(Xr) if Xr.shape[0] else None,
                                                    _ptr(Xr_indptr), _ptr(Xr_indices) if Xr_indices.shape[0] else None, k, dimA, l2_reg,
                                                    w_mult, step_size, int(niter), int(maxupd), _METHOD.get(method, 1), bool(limit_step),
                                                    bool(reuse_mean), _ptr(dec))
    if ret:
        raise MemoryError("Could not allocate enough memory.")
    return A, (dec[:, 0] & 0xffffff).astype(np.int64), dec[:, 1].astype(np.int64), (dec[:, 0] >> 24).astype(np.int64)


def debug_row_eval(B, Bsum, point, Xr_indptr, Xr_indices, Xr, l2_reg, w_mult=1., which=0):
    """Testing aid (include/poismf_hip.h, poismf_hip_debug_row_eval): the device's fun_single + grad_single (which = 0) or fun_and_grad
    (which = 1) at `point` for every row of the CSR; returns (f [n] float64, G [n x k])."""
    use_float = B.dtype == np.float32
    _check_arrays(use_float, (B, Bsum, point, Xr), (Xr_indptr, Xr_indices))
    lib = load_library(use_float)
    k = B.shape[1]
    n = Xr_indptr.shape[0] - 1
    G = np.empty((n, k), dtype=B.dtype)
    f = np.empty(n, dtype=np.float64)
    real = C.c_float if use_float else C.c_double
    fn = lib.poismf_hip_debug_row_eval
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] * 8 + [C.c_int, C.c_size_t, real, real, C.c_int]
    ret = fn(_ptr(G), _ptr(f), _ptr(B), _ptr(Bsum), _ptr(point), _ptr(Xr), _ptr(Xr_indptr), _ptr(Xr_indices), k, n, l2_reg, w_mult, int(which))
    if ret:
        raise MemoryError("poismf_hip_debug_row_eval failed")
    return f, G


def debug_plan(row_nnz, k, dimF, method, use_float, nseg=1, seg=-1, maxupd=1, w_mult=1., limit_step=True, num_cu=256, widths=False, engines=False,
               missing=False):
    """Testing aid (include/poismf_hip.h, poismf_hip_debug_plan): the launches the planner gives a half whose rows have row_nnz nonzeros,
    cut into nseg segments, for one call over segment `seg` (< 0: all of them): [(kernel instance, rows), ...].  Needs no GPU.
    widths: poismf_hip_debug_plan_widths -- a lane instance specialised on the used width of its factor rows is marked "[KU=<width>]";
    engines: poismf_hip_debug_plan_engines -- that, and a one-wave register launch on the quad engine is marked "[quad]";
    missing: poismf_hip_debug_plan_missing -- of that listing, only the launches the dispatcher has no kernel instance for (none, normally).
    method: "pg", "cg", "tncg", or "eval" (the evaluation-only kernels of debug_row_eval, planned like CG)."""
    lib = load_library(use_float)
    row_nnz = np.ascontiguousarray(row_nnz, dtype=np.uint32)
    real = C.c_float if use_float else C.c_double
    fn = (lib.poismf_hip_debug_plan_missing if missing else lib.poismf_hip_debug_plan_engines if engines else
          lib.poismf_hip_debug_plan_widths if widths else lib.poismf_hip_debug_plan)
    fn.restype = C.c_size_t
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.c_size_t, real, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
    args = (_ptr(row_nnz), len(row_nnz), int(nseg), int(seg), int(k), int(dimF), 4 if method == "eval" else _METHOD[method], int(maxupd), w_mult, int(bool(limit_step)), int(num_cu))
    buf = C.create_string_buffer(int(fn(*args, None, 0)) + 1)
    fn(*args, buf, len(buf))
    return [(name.strip(), int(rows)) for name, rows in (item.rsplit(" rows=", 1) for item in buf.value.decode().split(";") if item.strip())]


def lane_full_width(use_float, full):
    """Testing aid (poismf_hip_debug_lane_full_width): full -- the lane launches this process plans from now on carry every element of their
    slots, also where an instance specialised on the used width exists; not full -- the default again.  Returns the previous setting."""
    fn = load_library(use_float).poismf_hip_debug_lane_full_width
    fn.restype, fn.argtypes = C.c_int, [C.c_int]
    return bool(fn(int(bool(full))))


def reg_quad_off(use_float, off):
    """Testing aid (poismf_hip_debug_reg_quad_off): off -- the one-wave register launches this process plans from now on take the sixteen-lane
    engine also where the quad engine exists; not off -- the default again.  Returns the previous setting."""
    fn = load_library(use_float).poismf_hip_debug_reg_quad_off
    fn.restype, fn.argtypes = C.c_int, [C.c_int]
    return bool(fn(int(bool(off))))


class PoisMF:
    """Fit-path subset of the reference's PoisMF (ref: poismf/__init__.py:205-495).  Only what sits on
    the factor-update path is mirrored: constructor arguments that reach run_poismf, ``fit`` for SciPy
    COO input, ``fit_unsafe``, and the post-fit ``Bsum`` / ``Amean``."""

    def __init__(self, k=50, method="tncg", l2_reg="auto", l1_reg=0.0, niter="auto", maxupd="auto",
                 limit_step=True, initial_step=1e-7, early_stop=True, reuse_prev=False, weight_mult=1.0,
                 random_state=1, use_float=True, handle_interrupt=True, nthreads=-1):
        assert method in ("tncg", "cg", "pg")
        self.k = int(k)
        self.method = method
        self.l2_reg_, self.maxupd_, self.niter_ = harness.auto_defaults(method, self.k, l2_reg, maxupd, niter)
        assert self.k > 0 and self.niter_ >= 1 and self.maxupd_ >= 1
        assert self.l2_reg_ >= 0. and l1_reg >= 0. and initial_step > 0. and weight_mult > 0.
        self.l1_reg_ = float(l1_reg)
        self.limit_step = bool(limit_step)
        self.initial_step = float(initial_step)
        self.early_stop = bool(early_stop)
        self.reuse_prev = bool(reuse_prev)
        self.weight_mult = float(weight_mult)
        self.random_state = random_state
        self.use_float = bool(use_float)
        self.handle_interrupt = bool(handle_interrupt)
        self.nthreads_ = 1 if nthreads < 1 else int(nthreads)
        self.is_fitted = False

    def fit(self, X):
        # COO -> CSR + CSC on the device (the reference's _process_data; SciPy's bits for integer counts, section 1c's sums otherwise);
        # the converted matrix stays in HBM and the alternation runs on it in place (run_poismf's loop, same return
        # codes and exceptions) -- nothing but the triplets goes up and nothing but the factors comes back
        import scipy.sparse as sp
        self.nusers, self.nitems = X.shape
        self.A, self.B = harness.initialize_matrices(self.nusers, self.nitems, self.k, self.use_float,
                                                     self.random_state)
        sess = Session.from_coo(sp.coo_matrix(X), self.k, self.use_float)
        try:
            sess.set_factors(self.A, self.B)
            p = sess.make_params(self.method, self.l2_reg_, self.l1_reg_, self.weight_mult, self.initial_step, self.limit_step,
                                 self.maxupd_, self.early_stop, self.reuse_prev)
            ret = sess.run(p, self.niter_, self.handle_interrupt)
            A, B = sess.get_factors()
            self.A[...] = A
            self.B[...] = B
        finally:
            sess.close()
        if ret == 1:
            raise MemoryError("Could not allocate enough memory.")
        elif ret == 2 and not self.handle_interrupt:
            raise InterruptedError("Procedure was interrupted")
        self.Bsum = self.B.sum(axis=0) + self.l1_reg_
        self.Amean = self.A.mean(axis=0)
        self.is_fitted = True
        return self

    def fit_unsafe(self, A, B, Xcsr, Xcsc):
        self.A, self.B = A, B
        self.nusers, self.nitems = A.shape[0], B.shape[0]
        self._fit((Xcsr.data, Xcsr.indices, Xcsr.indptr), (Xcsc.data, Xcsc.indices, Xcsc.indptr))
        self.is_fitted = True
        return self

    def eval_llk(self, X, full_llk=False, include_missing=False):
        """Poisson log-likelihood of the fitted factors on the cells of X (include/poismf_hip.h section 1e; the reference
        declares eval_llk in src/poismf.h:258-269 and defines it nowhere).  X: a SciPy sparse matrix or synth.Triplets whose
        rows and columns index this model's users and items; duplicate cells are summed.  full_llk adds the -lgamma(x + 1)
        terms; include_missing counts every cell of the users x items matrix, a missing one as x = 0.  No regularisation."""
        if not self.is_fitted:
            raise ValueError("Model has not been fitted.")
        import scipy.sparse as sp
        coo = sp.coo_matrix(X) if sp.issparse(X) else X
        row, col, val = _coo_arrays(coo, self.use_float)
        if len(val) and (int(row.max()) >= self.nusers or int(col.max()) >= self.nitems):
            raise IndexError("a row / column index of X lies outside the fitted model's users / items")
        dt = np.float32 if self.use_float else np.float64
        A = np.ascontiguousarray(self.A, dtype=dt)
        B = np.ascontiguousarray(self.B, dtype=dt)
        lib = load_library(self.use_float)
        return float(lib.eval_llk(_ptr(A), _ptr(B), _ptr(row), _ptr(col), _ptr(val), len(val), self.k, bool(full_llk),
                                  bool(include_missing), self.nusers, self.nitems, self.nthreads_))

    def _fit(self, csr, csc):                                                        # ref: __init__.py:427-439
        _run_poismf(csr[0], csr[1], csr[2], csc[0], csc[1], csc[2], self.A, self.B, self.method,
                    self.limit_step, self.l2_reg_, self.l1_reg_, self.weight_mult, self.initial_step,
                    self.niter_, self.maxupd_, self.early_stop, self.reuse_prev, self.handle_interrupt,
                    self.nthreads_)
        self.Bsum = self.B.sum(axis=0) + self.l1_reg_
        self.Amean = self.A.mean(axis=0)


def _transform(self, X):
    """Factors for new rows given as a SciPy CSR / COO matrix (ref: poismf/__init__.py:619-692, transform)."""
    import scipy.sparse as sp
    assert self.is_fitted and X.shape[0] > 0
    csr = sp.csr_matrix(X)
    csr.sum_duplicates(); csr.sort_indices()
    dt = np.float32 if self.use_float else np.float64
    return _predict_factors_multiple(
        self.B, self.Bsum.astype(dt), self.Amean.astype(dt), csr.indptr.astype(np.uint64), csr.indices.astype(np.uint64),
        csr.data.astype(dt), self.l2_reg_, self.weight_mult, self.initial_step, self.niter_, self.maxupd_, self.method,
        self.limit_step, self.reuse_prev, self.nthreads_)


PoisMF.transform = _transform


class _HostFactors:
    """Host factors A [dimA x k], B [dimB x k] as the target of a serving call (serving.py): what a Session offers that path, with
    the factors going up on every call.  They are brought to the model's real_t only once a call needs them."""

    def __init__(self, A, B, dimA, dimB, k, use_float):
        self.A, self.B, self.dimA, self.dimB, self.k, self.use_float = A, B, int(dimA), int(dimB), int(k), bool(use_float)

    def _factors(self):
        dt = np.float32 if self.use_float else np.float64
        self.A, self.B = np.ascontiguousarray(self.A, dtype=dt), np.ascontiguousarray(self.B, dtype=dt)
        return self.A, self.B

    def item_norms(self):
        """n2[j] = the fused chain of row j of B with itself, predict_multiple's bits (Session.item_norms on host factors)"""
        B = self._factors()[1]
        every = np.arange(self.dimB, dtype=np.uint64)
        n2 = np.empty(self.dimB, B.dtype)
        _predict_multiple(n2, B, B, every, every)
        return n2

    def _entry(self, name, exclude_seen):
        A, B = self._factors()
        return getattr(load_library(self.use_float), "poismf_hip_" + name), (_ptr(A), _ptr(B), self.k, self.dimA, self.dimB), ()


def _host(self):
    """a fitted model's factors as a serving target"""
    if not self.is_fitted:
        raise ValueError("Model has not been fitted.")
    return _HostFactors(self.A, self.B, self.nusers, self.nitems, self.k, self.use_float)


def _topN_batch(self, users, n=10, exclude=None, output_score=False, include=None, include_of=None):
    """The n best items of every user in `users` (rows of the fitted A) under "score descending, item index ascending", in one
    fused pass on the GPU (include/poismf_hip.h section 1f).  exclude: None, a SciPy sparse matrix with one row per entry of
    `users` (its nonzero columns are left out: passing the training matrix's rows excludes what a user has seen -- the model
    does not keep X) or an (indptr, indices) pair with strictly ascending rows.  Returns (items uint64 [m x n], scores [m x n],
    empty unless output_score).  For new users: topN_new (a resident model: Session.topn_new).
    include: a candidate list per user, in the same two forms (a sparse matrix's stored columns): each user is ranked among its
    own list only and only those rows of B are read (section 1h).  n may then exceed what a user has left: the row is padded
    with TOPN_NONE and -inf.
    include_of: with it, `include` is a TABLE of lists shared between users (any number of rows G >= 1) and include_of names each
    user's row of it: an integer array with one entry per user, or one int for all (section 1i).  The answers are those of
    include= with every user's list written out, bit for bit; the table is read once, and users of one list share the rows of B
    they read.  Few lists for many users belong here, a list per user belongs in include= alone."""
    return serving.topn_batch(_host(self), users, n, False, exclude, output_score, include, include_of)


PoisMF.topN_batch = _topN_batch


def _topN_deep(self, users, n=1000, exclude=None, output_score=False):
    """topN_batch for deep lists -- candidate generation for a re-ranker: the n <= TOPN_DEEP_MAX_N_TOP best items of every user in
    `users` under "score descending, item index ascending", in one fused pass on the GPU (include/poismf_hip.h section 1l).
    exclude as in topN_batch.  n may exceed what a user has left, or the number of items: the row is padded with TOPN_NONE and
    -inf.  Up to n = TOPN_BATCH_MAX_N_TOP the answers are topN_batch's bit for bit, which keeps its lists on chip and is the faster
    of the two there.  Returns (items uint64 [m x n], scores [m x n], empty unless output_score)."""
    return serving.topn_deep(_host(self), users, n, False, exclude, output_score)


PoisMF.topN_deep = _topN_deep


def _topN_quota(self, users, n=10, group_of=None, quota=1, exclude=None, output_score=False):
    """topN_batch with "at most quota[g] items of group g on a page": the user's complete ranked list ("score descending, item index
    ascending", minus `exclude` as in topN_batch) is walked and an item is taken iff fewer than quota[g] items of its group
    group_of[item] were taken before it, until n <= TOPN_BATCH_MAX_N_TOP are taken -- in one fused pass on the GPU
    (include/poismf_hip.h section 1n).  group_of: one group id per item.  quota: one int for every group, or an array with one
    entry per group; 0 bars a group, n or more leaves it unconstrained.  A user for whom the quotas admit fewer than n items gets a
    row padded with TOPN_NONE and -inf.  Returns (items uint64 [m x n], scores [m x n], empty unless output_score)."""
    return serving.topn_quota(_host(self), users, n, group_of, quota, False, exclude, output_score)


PoisMF.topN_quota = _topN_quota


def _topN_weighted(self, users, n=10, item_weight=None, exclude=None, output_score=False):
    """topN_batch under score x item_weight[item] -- expected revenue (rate x price), a popularity discount, a freshness decay, a
    boost or a penalty: the n <= TOPN_BATCH_MAX_N_TOP best items of every user in `users` under "weighted score descending, item
    index ascending", minus `exclude` as in topN_batch, the multiplication made on the GPU in the same fused pass before anything
    is pruned (include/poismf_hip.h section 1o).  item_weight: one finite weight >= 0 per item, or one number for all.  A weight
    of 0 does not bar an item -- it scores 0 and ties with its like by index; exclude= bars one.  The scores returned are the
    weighted ones: predict's, times the weight, rounded once.  n may exceed what a user has left: the row is padded with TOPN_NONE
    and -inf.  Returns (items uint64 [m x n], scores [m x n], empty unless output_score)."""
    return serving.topn_weighted(_host(self), users, n, item_weight, False, exclude, output_score)


PoisMF.topN_weighted = _topN_weighted


def _topN_adjusted(self, users, n=10, adjust=None, exclude=None, output_score=False):
    """topN_batch where single cells of the score matrix carry a factor of their own -- an impression discount, a discount on the
    user's seen items instead of barring them, a per-user boost: the n <= TOPN_BATCH_MAX_N_TOP best items of every user in `users`
    under "adjusted score descending, item index ascending", minus `exclude` as in topN_batch, exact and in one call on the GPU
    (include/poismf_hip.h section 1r).  adjust: a SciPy sparse matrix with one row per user of the batch whose stored values are
    finite factors >= 0 (stored zeros are kept), or an (indptr, indices, factors) triple; None lists no cell.  A listed cell scores
    predict's score times its factor, rounded once; every other cell predict's score.  A factor of 0 does not bar a cell -- it
    scores 0 and ties with its like by index; a cell both listed and excluded is excluded.  n may exceed what a user has left: the
    row is padded with TOPN_NONE and -inf.  Returns (items uint64 [m x n], scores [m x n], empty unless output_score)."""
    return serving.topn_adjusted(_host(self), users, n, adjust, False, exclude, output_score)


PoisMF.topN_adjusted = _topN_adjusted


def _similar_items(self, items, n=10, output_score=False, exclude_self=True, item_norm=None):
    """The n best items by cosine similarity of their rows of B to each item of `items`, under "similarity descending, item index
    ascending" -- the weighted call with rows of B as the queries (section 1o):
        n2[j]  = predict_multiple(B, B, j, j), the fused chain of B[j] with itself (item_norm= takes it precomputed)
        inv[j] = 1 / sqrt(n2[j]) in the model's precision, 0 where n2[j] == 0
        rows   = the weighted top-N of B[i] against B with item_weight = inv, minus the query itself when exclude_self
        score  = weighted score x inv[i], a second rounded multiplication
    A zero row of B has similarity 0 to everything, as a query and as a candidate; such rows come in index order.  Returns (items
    uint64 [m x n], similarities [m x n], empty unless output_score); a row is padded with TOPN_NONE and -inf past the last item."""
    if not self.is_fitted:
        raise ValueError("Model has not been fitted.")
    rows_of_B = _HostFactors(self.B, self.B, self.nitems, self.nitems, self.k, self.use_float)   # (the queries and the corpus)
    return serving.similar_items(rows_of_B, items, n, output_score, exclude_self, item_norm)


PoisMF.similar_items = _similar_items


def _topN_diverse(self, users, n=10, pool=100, lam=0.7, exclude=None, output_score=False, output_value=False, item_norm=None):
    """topN_batch diversified from the factors themselves -- no group label per item, as topN_quota needs one: greedy maximal marginal
    relevance on the GPU (include/poismf_hip.h section 1p).  Of every user's best `pool` <= TOPN_DEEP_MAX_N_TOP items (topN_deep's
    list, minus `exclude` as in topN_batch) n <= TOPN_BATCH_MAX_N_TOP are picked one by one, each the unpicked one with the largest
        lam x (score / the user's best score)  -  (1 - lam) x (largest cosine of its row of B to the row of an item already picked)
    ties to the better-ranked item; the cosine is similar_items'.  lam = 1 gives topN_deep's first n, lam = 0 ignores the scores
    beyond the pool.  item_norm= takes the squared norms precomputed (Session.item_norms()), as similar_items does.  A row the pool
    leaves short is padded with TOPN_NONE and -inf.  Returns (items uint64 [m x n] in pick order, their scores [m x n] -- predict's,
    empty unless output_score --, the value each was picked at [m x n], empty unless output_value)."""
    return serving.topn_diverse(_host(self), users, n, pool, lam, False, exclude, output_score, output_value, item_norm)


PoisMF.topN_diverse = _topN_diverse


def _topN_new(self, X, n=10, exclude=None, exclude_own=True, output_score=False):
    """The n best items of users the model has never seen (ref: poismf/__init__.py, topN_new), one row of X per new user: their
    factors are obtained as transform(X) obtains them -- the model's own method and hyper-parameters -- and ranked against B under
    "score descending, item index ascending" without leaving the device, B going up once (poismf_hip_topn_new, include/poismf_hip.h
    section 1m).  exclude_own leaves out the items of the user's own row of X; exclude (a SciPy sparse matrix with one row per row
    of X, or an (indptr, indices) pair with strictly ascending rows) leaves out more.  Returns (items uint64 [m x n], scores
    [m x n], empty unless output_score): those of topN_batch on transform(X)'s factors, bit for bit."""
    if not self.is_fitted:
        raise ValueError("Model has not been fitted.")
    data, indptr, indices = _new_rows_args(X, self.nitems, self.use_float)
    m, n = len(indptr) - 1, int(n)
    _, ep, ei = _topn_batch_args(np.arange(m, dtype=np.uint64), n, exclude, max(m, 1), self.nitems)
    dt = np.float32 if self.use_float else np.float64
    ix, sc = _topn_outputs(m, n, dt, output_score)
    if m == 0:
        return ix, sc
    B = np.ascontiguousarray(self.B, dtype=dt)
    Bsum, Amean = _new_stats(self.Bsum, self.Amean, self.k, self.use_float)
    _batch_rc(load_library(self.use_float).poismf_hip_topn_new(
        _ptr(B), _ptr(Bsum), _ptr(Amean), _opt_ptr(data), _ptr(indptr), _opt_ptr(indices), self.k, self.nitems, m, self.l2_reg_,
        self.weight_mult, self.initial_step, int(self.niter_), int(self.maxupd_), _METHOD[self.method], bool(self.limit_step),
        bool(self.reuse_prev), n, int(bool(exclude_own)), _opt_ptr(ep), _opt_ptr(ei), _ptr(ix), _opt_ptr(sc), None), "top-N of new rows")
    return ix, sc


PoisMF.topN_new = _topN_new


def rank_batch(A, B, users, test, exclude=None, include=None, include_of=None, unite_test=False):
    """poismf_hip_rank_batch on host factors A [dimA x k], B [dimB x k] (float32 or float64, both alike): for every cell of `test`
    (a SciPy sparse matrix with one row per entry of `users`, or an (indptr, indices) pair with strictly ascending rows) the
    0-based position of its item in the user's complete ranked list, exclusion set left out (include/poismf_hip.h section 1g).
    Returns (ranks uint32, one per cell in row order, RANK_EXCLUDED where the item is in the user's `exclude` row; n_adm uint32
    [m], the admissible items of each user).  include: a candidate list per user, in the same two forms (a sparse matrix's stored
    columns), passed as given: every cell is ranked among its user's own list only, minus `exclude`, only those rows of B are
    read, and a cell whose item is not listed gets RANK_EXCLUDED too (poismf_hip_rank_include, section 1j).
    include_of: with it, `include` is a TABLE of lists shared between users (any number of rows G >= 1) and include_of names each
    user's row of it: an integer array with one entry per batch entry, or one int for all (poismf_hip_rank_shared, section 1k).
    The answers are those of include= with every user's list written out; the table is read once, and users of one list share
    the rows of B they read.  unite_test (with include_of only): every user is ranked among its list united with its own
    held-out row, so a shared pool of negatives may be passed as it is; only excluded cells get RANK_EXCLUDED."""
    A, B = np.asarray(A), np.asarray(B)
    if A.ndim != 2 or B.ndim != 2 or A.shape[1] != B.shape[1] or A.dtype != B.dtype or A.dtype not in (np.float32, np.float64):
        raise ValueError("A and B must be float32 or float64 matrices with the same number of columns")
    target = _HostFactors(A, B, A.shape[0], B.shape[0], A.shape[1], A.dtype == np.float32)
    return serving.rank_batch(target, users, test, False, exclude, include, include_of, unite_test)


def _ranking_result(tp, ranks, n_adm, k, per_user):
    from . import metrics
    each = metrics.metrics_from_ranks(tp, ranks, n_adm, k)
    out = metrics.mean_metrics(each)
    if per_user:
        out["per_user"] = each
        out["ranks"], out["n_adm"], out["test_indptr"] = ranks, n_adm, tp
    return out


def _eval_ranking(self, X_test, k=10, exclude=None, users=None, per_user=False, include=None, include_of=None):
    """Held-out ranking metrics of the fitted model, from exact ranks computed in one fused pass on the GPU (include/poismf_hip.h
    section 1g; the definitions are those of poismf_amd/metrics.py).  X_test: a SciPy sparse matrix with the model's shape whose
    stored cells are the held-out positives (values play no part; explicit zeros dropped, duplicates merged).  users: the rows to
    evaluate, by default every row of X_test with a stored cell.  exclude: None, or a sparse matrix with the model's shape whose
    stored cells leave the ranking (the training matrix; its rows for `users` are taken here), or an (indptr, indices) pair with
    one strictly ascending row per entry of `users`; a held-out cell that is excluded takes no part in any metric.  Returns a dict
    of the means of hit, precision, recall, ap, ndcg, rr, auc at cut-off k over the users that counted, plus n_users; with per_user
    also "per_user" (the same names, one value per user), "ranks", "n_adm" and "test_indptr".
    include: sampled evaluation (section 1j) -- a candidate list per user, as a sparse matrix with the model's shape (its rows for
    `users` are taken) or an (indptr, indices) pair with one strictly ascending row per entry of `users`.  Every user is ranked
    among its own list only, and only those rows of B are read.  Each user's held-out row is united into its list first, so the
    sampled negatives alone may be passed; lists that already hold the positives change nothing.
    include_of: with it, `include` is a TABLE of pools shared between users (section 1k) -- a sparse matrix or an (indptr, indices)
    pair with any number of rows and at most the model's number of columns -- and include_of names each user's row of it: one int
    for all, or an integer array with one entry per user of the model (indexed by user id; the entries of `users` are taken here).
    The held-out rows are united in on the device, so a pool of negatives sampled once for everybody is passed as it is and no
    per-user list is built."""
    if not self.is_fitted:
        raise ValueError("Model has not been fitted.")
    users, test, exclude, k = _eval_ranking_args(X_test, exclude, users, k, self.nusers, self.nitems)
    dt = np.float32 if self.use_float else np.float64
    if include_of is not None:
        ranks, n_adm = rank_batch(np.ascontiguousarray(self.A, dtype=dt), np.ascontiguousarray(self.B, dtype=dt), users, test, exclude,
                                  include=include, include_of=_include_of_rows(include_of, users, self.nusers), unite_test=True)
        return _ranking_result(test[0], ranks, n_adm, k, per_user)
    if include is not None:
        include = _unite_rows(_include_rows(include, users, self.nusers, self.nitems), test)
    ranks, n_adm = rank_batch(np.ascontiguousarray(self.A, dtype=dt), np.ascontiguousarray(self.B, dtype=dt), users, test, exclude,
                              include=include)
    return _ranking_result(test[0], ranks, n_adm, k, per_user)


PoisMF.eval_ranking = _eval_ranking


def list_eval(B, items, test=None, item_norm=None, budget_mb=None):
    """poismf_hip_list_eval on host factors B [dimB x k] (float32 or float64): list-wise evaluation of the lists `items` [m x n] --
    what any topN_* call returned, from any source (include/poismf_hip.h section 1q).  test: the held-out items, a SciPy sparse
    matrix with one row per row of `items` or an (indptr, indices) pair with strictly ascending rows.  item_norm: the squared norms
    of the rows of B as similar_items takes them (Session.item_norms()); without it no cosine is computed.  budget_mb: the bound of
    the call's scratch, LIST_EVAL_BUDGET_MB by default; a smaller one cuts the rows into more chunks and changes no answer.
    Returns (pos uint32, one per cell of `test` in row order: the item's 0-based position in its row, LIST_ABSENT when the row does
    not list it -- None without test; cos_sum int64 [m]: the sum over the row's pairs of items of their cosine, similar_items',
    in units of 2^-LIST_COS_SHIFT -- None without item_norm; length uint32 [m]: the row's items; exposure uint32 [dimB]: the rows
    that list each item)."""
    B = np.asarray(B)
    if B.ndim != 2 or B.dtype not in (np.float32, np.float64):
        raise ValueError("B must be a float32 or float64 matrix")
    dt = B.dtype.type
    lists, tp, ti, inv, budget = _list_eval_args(items, test, item_norm, budget_mb, B.shape[0], B.shape[1], dt)
    pos, cos, length, expo = _list_eval_outputs(lists, ti, inv, B.shape[0])
    if lists.shape[0] == 0:
        return pos, cos, length, expo
    B = np.ascontiguousarray(B)
    lib = load_library(dt == np.float32)
    _batch_rc(lib.poismf_hip_list_eval(_ptr(B), B.shape[1], B.shape[0], _ptr(lists), lists.shape[0], lists.shape[1], _opt_ptr(inv),
                                       _opt_ptr(tp), _opt_ptr(ti), budget, _opt_ptr(pos), _opt_ptr(cos), _ptr(length), _ptr(expo)),
              "list evaluation")
    return pos, cos, length, expo


def _lists_result(lists, test, pos, cos, length, expo, item_pop, per_user):
    from . import metrics
    k = lists.shape[1]
    each = {}
    out = {}
    if test is not None:
        each.update(metrics.metrics_from_positions(test[0], pos, k))
        out.update(metrics.mean_metrics(each, metrics.LIST_METRICS))
    else:
        out["n_users"] = 0
    each["ild"] = metrics.ild(cos, length)
    if item_pop is not None:
        each["novelty"] = metrics.novelty(lists, item_pop)
    for name in ("ild", "novelty"):
        if name in each:
            out[name] = metrics.nan_mean(each[name])
    out["coverage"], out["gini"] = metrics.coverage(expo), metrics.gini(expo)
    out["n_lists"] = int(lists.shape[0])
    if per_user:
        out["per_user"] = each
        out["positions"], out["test_indptr"] = pos, (test[0] if test is not None else None)
        out["cos_sum"], out["length"], out["exposure"] = cos, length, expo
    return out


_EVAL_LISTS_DOC = """List-wise evaluation of the lists `items` [m x n] -- what any topN_* call returned, or pages from anywhere else -- in one
    pass on the GPU (include/poismf_hip.h section 1q; the definitions are those of poismf_amd/metrics.py).  users: the user of each
    row, by default rows 0 .. m-1 of the model; repeats allowed.  k: evaluate items[:, :k], by default the lists' width.  X_test: a
    SciPy sparse matrix with the model's shape whose stored cells are the held-out positives, as in eval_ranking; its rows for
    `users` are taken.  exclude: as in eval_ranking -- a held-out cell that is excluded is removed here, on the host, and takes no
    part.  item_norm: the squared norms of the rows of B as similar_items takes them (Session.item_norms(), computed once per
    model), computed when absent -- on a session that brings the factors to the host on every call.  item_pop: one
    non-negative number per item, how often it was seen in training, for `novelty`.  Returns a dict: the means of hit, precision,
    recall, ap, ndcg, rr at k (only with X_test; a held-out item the list lacks still counts in the denominators), ild (1 - the
    mean pairwise cosine of a list's items), coverage and gini of the exposure counts, novelty (only with item_pop), n_users (the
    users with a valid held-out cell) and n_lists; with per_user also "per_user" (one value per row), "positions", "test_indptr",
    "cos_sum", "length" and "exposure"."""


def _eval_lists(self, items, users=None, X_test=None, k=None, exclude=None, item_norm=None, item_pop=None, per_user=False):
    if not self.is_fitted:
        raise ValueError("Model has not been fitted.")
    dt = np.float32 if self.use_float else np.float64
    lists, test, item_pop = _eval_lists_args(items, users, X_test, k, exclude, item_pop, self.nusers, self.nitems)
    B = np.ascontiguousarray(self.B, dtype=dt)
    if item_norm is None:
        _list_eval_args(lists, test, None, None, self.nitems, self.k, dt)   # (everything else is judged before the norms are computed)
        every = np.arange(self.nitems, dtype=np.uint64)
        item_norm = np.empty(self.nitems, dt)
        _predict_multiple(item_norm, B, B, every, every)
    pos, cos, length, expo = list_eval(B, lists, test, item_norm)
    return _lists_result(lists, test, pos, cos, length, expo, item_pop, per_user)


_eval_lists.__doc__ = _EVAL_LISTS_DOC
PoisMF.eval_lists = _eval_lists



class _DevArray:
    """Minimal __cuda_array_interface__ carrier so torch can alias session-owned device memory."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False),
                                         "version": 2, "strides": None}


class Session:
    """Device-resident half-sweeps (include/poismf_hip.h section 2).  X, A and B stay in HBM; each call
    runs one half of the alternation on this session's row shard."""

    def __init__(self, csr, csc, dimA, dimB, k, use_float, device=0, stream=None, shardA=None, shardB=None, _coo=None):
        self.lib = load_library(use_float)
        self.use_float = bool(use_float)
        self.dimA, self.dimB, self.k = int(dimA), int(dimB), int(k)
        self.shardA = tuple(shardA) if shardA is not None else (0, self.dimA)
        self.shardB = tuple(shardB) if shardB is not None else (0, self.dimB)
        h = C.c_void_p()
        if _coo is not None:
            row, col, val = _coo
            rc = self.lib.poismf_hip_session_create_coo(
                C.byref(h), int(device), C.c_void_p(stream or 0), _ptr(row), _ptr(col), _ptr(val), len(val),
                self.dimA, self.dimB, self.k, self.shardA[0], self.shardA[1], self.shardB[0], self.shardB[1])
            if rc == 3:
                raise ValueError("a row / column index of the triplets lies outside the matrix")
        else:
            _check_arrays(use_float, (csr[0], csc[0]), (csr[1], csr[2], csc[1], csc[2]))
            if len(csr[0]) == 0:
                raise ValueError("'X' contains no non-zero entries.")
            rc = self.lib.poismf_hip_session_create(
                C.byref(h), int(device), C.c_void_p(stream or 0), _ptr(csr[0]), _ptr(csr[2]), _ptr(csr[1]),
                _ptr(csc[0]), _ptr(csc[2]), _ptr(csc[1]), self.dimA, self.dimB, self.k,
                self.shardA[0], self.shardA[1], self.shardB[0], self.shardB[1])
        if rc != 0 or not h.value:
            raise MemoryError("poismf_hip_session_create failed (no usable HIP device or out of memory)")
        self.h = h

    @classmethod
    def from_coo(cls, coo, k, use_float, device=0, stream=None, shardA=None, shardB=None):
        """Session whose CSR and CSC are built on the device from the triplets of a SciPy COO matrix (indices sorted, duplicates
        summed: the sums of section 1c of include/poismf_hip.h -- a cell's triplets added in input order; SciPy's bits where the
        values are integers); with shards, only the triplets of the shard's rows (CSR) / columns (CSC) are kept, and a kept cell
        has the bits it has without shards."""
        if coo.nnz == 0:
            raise ValueError("'X' contains no non-zero entries.")
        return cls(None, None, coo.shape[0], coo.shape[1], k, use_float, device, stream, shardA, shardB,
                   _coo=_coo_arrays(coo, use_float))

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.lib.poismf_hip_session_destroy(self.h)
            self.h = C.c_void_p()

    __del__ = close

    def set_factors(self, A, B):
        _check_arrays(self.use_float, (A, B), ())
        assert A.shape == (self.dimA, self.k) and B.shape == (self.dimB, self.k)
        if self.lib.poismf_hip_session_set_factors(self.h, _ptr(A), _ptr(B)):
            raise RuntimeError("poismf_hip_session_set_factors failed")

    def get_factors(self, out=None):
        """(A, B) on the host; out = (A, B): into these C-contiguous arrays of the session's shapes and precision."""
        dt = np.float32 if self.use_float else np.float64
        if out is not None:
            A, B = out
            for M, n in ((A, self.dimA), (B, self.dimB)):
                if M.dtype != dt or M.shape != (n, self.k) or not M.flags.c_contiguous:
                    raise ValueError("get_factors: out arrays must be C-contiguous, of the session's shapes and precision")
        else:
            A = np.empty((self.dimA, self.k), dt)
            B = np.empty((self.dimB, self.k), dt)
        if self.lib.poismf_hip_session_get_factors(self.h, _ptr(A), _ptr(B)):
            raise RuntimeError("poismf_hip_session_get_factors failed")
        return A, B

    def device_arrays(self):
        """(A, B) as objects exposing __cuda_array_interface__ over the session's device buffers."""
        ts = "<f4" if self.use_float else "<f8"
        return (_DevArray(self.lib.poismf_hip_session_A(self.h), (self.dimA, self.k), ts),
                _DevArray(self.lib.poismf_hip_session_B(self.h), (self.dimB, self.k), ts))

    def make_params(self, method, l2_reg, l1_reg=0.0, w_mult=1.0, step_size=1e-7, limit_step=True, maxupd=1,
                    early_stop=False, reuse_prev=False):
        return self.lib.params_t(l2_reg, l1_reg, w_mult, step_size, _METHOD[method], int(limit_step), int(maxupd),
                                 int(early_stop), int(reuse_prev))

    def half_sweep(self, which, params, step_size, cnst_div, want_unchanged=False, seg=None):
        """One half-sweep over the session's shard, or (seg = j) over its segment j only."""
        n = C.c_size_t(0)
        if seg is None:
            rc = self.lib.poismf_hip_half_sweep(self.h, int(which), C.byref(params), step_size, cnst_div,
                                                C.byref(n) if want_unchanged else None)
        else:
            rc = self.lib.poismf_hip_half_sweep_segment(self.h, int(which), C.byref(params), step_size, cnst_div, int(seg),
                                                        C.byref(n) if want_unchanged else None)
        if rc:
            raise RuntimeError("poismf_hip_half_sweep failed")
        return n.value

    def set_segments(self, which, nseg):
        n = self.lib.poismf_hip_session_set_segments(self.h, int(which), int(nseg))
        if n < 1:
            raise RuntimeError("poismf_hip_session_set_segments failed")
        return n

    def segment_rows(self, which, seg):
        b, e = C.c_size_t(0), C.c_size_t(0)
        if self.lib.poismf_hip_session_segment_rows(self.h, int(which), int(seg), C.byref(b), C.byref(e)):
            raise IndexError("no such segment")
        return b.value, e.value

    def real(self, v):
        """v rounded to the session's real_t, as a Python float (run_poismf does its step / divisor arithmetic in
        real_t, ref: src/poismf.c:511, :532)"""
        return float(np.float32(v)) if self.use_float else float(v)

    def cnst_div(self, l2_reg, step_size):
        """The PG divisor 1 / (1 + 2 l2 step) evaluated as run_poismf evaluates it (ref: src/poismf.c:511): l2 and the
        step are real_t, the expression is double, the result is stored as real_t."""
        return self.real(1. / (1. + 2. * self.real(l2_reg) * self.real(step_size)))

    def sweep(self, params, step_size):
        """One full outer iteration with the reference's schedule (ref: src/poismf.c:506-608): B half, then
        (PG) halve the step, then A half.  Returns the step for the next iteration."""
        step_size = self.real(step_size)
        cnst_div = self.cnst_div(params.l2_reg, step_size)
        self.half_sweep(0, params, step_size, cnst_div)
        if params.method == _METHOD["pg"]:
            step_size = self.real(step_size * 0.5)
        self.half_sweep(1, params, step_size, cnst_div)
        return step_size

    def run(self, params, niter, handle_interrupt=True):
        """run_poismf's whole loop on this session (return codes 0 / 1 / 2 as run_poismf)"""
        return self.lib.poismf_hip_session_run(self.h, C.byref(params), int(niter), int(bool(handle_interrupt)))

    def llk(self, full_llk=False, include_missing=False):
        """Poisson log-likelihood of this session's CSR shard under its resident factors (include/poismf_hip.h section 1e): the
        same bits as PoisMF.eval_llk / eval_llk on the same matrix and factors for a single-GPU session"""
        out = C.c_double(0)
        if self.lib.poismf_hip_session_llk(self.h, int(bool(full_llk)), int(bool(include_missing)), C.byref(out)):
            raise RuntimeError("poismf_hip_session_llk failed")
        return out.value

    def stream(self):
        """the hipStream_t this session enqueues on, as an integer handle"""
        return self.lib.poismf_hip_session_stream(self.h) or 0

    def factors_dirty(self, which):
        """tell the session that factor `which` (0: B, 1: A) was written through a device pointer obtained earlier"""
        self.lib.poismf_hip_session_factors_dirty(self.h, int(which))

    def colsum_blocks(self, which):
        """blocks the column sums over the FIXED factor of half `which` are cut into (include/poismf_hip.h)"""
        return int(self.lib.poismf_hip_session_colsum_blocks(self.h, int(which)))

    def colsum_partial(self, which, b_lo, b_hi):
        if self.lib.poismf_hip_session_colsum_partial(self.h, int(which), int(b_lo), int(b_hi)):
            raise RuntimeError("poismf_hip_session_colsum_partial failed")

    def partials_array(self, which):
        """the session's [blocks x k] partial sums of half `which`, as a __cuda_array_interface__ object aliasing device memory"""
        nb = self.colsum_blocks(which)
        return _DevArray(self.lib.poismf_hip_session_partials(self.h), (nb, self.k), "<f4" if self.use_float else "<f8")

    def partials_ready(self):
        self.lib.poismf_hip_session_partials_ready(self.h)

    def profile(self, enable=True):
        self.lib.poismf_hip_session_profile(self.h, int(enable))

    def kernel_time(self, which):
        ms, n = C.c_double(0), C.c_size_t(0)
        if self.lib.poismf_hip_session_kernel_time(self.h, int(which), C.byref(ms), C.byref(n)):
            raise RuntimeError("poismf_hip_session_kernel_time failed")
        return ms.value, n.value

    def eval_stats(self, which):
        """(tile passes, sum over rows of passes x nonzeros) of this half since profile(True)"""
        a, b = C.c_ulonglong(0), C.c_ulonglong(0)
        if self.lib.poismf_hip_session_eval_stats(self.h, int(which), C.byref(a), C.byref(b)):
            raise RuntimeError("poismf_hip_session_eval_stats failed")
        return a.value, b.value

    def decisions(self, which):
        """(iterations, evaluations, rc) per row of this session's shard of half `which` (0: B rows, 1: A rows) in the most recent
        half-sweep since profile(True) -- what the reference's minimize_nonneg_cg / tnc return and its drivers drop"""
        lo, hi = self.shardA if which else self.shardB
        dec = np.zeros((hi - lo, 2), dtype=np.uint32)
        if self.lib.poismf_hip_session_decisions(self.h, int(which), _ptr(dec), hi - lo):
            raise RuntimeError("poismf_hip_session_decisions: profiling is off")
        return (dec[:, 0] & 0xffffff).astype(np.int64), dec[:, 1].astype(np.int64), (dec[:, 0] >> 24).astype(np.int64)

    def decision_stats(self, which):
        """sums over this shard's rows of half `which` in the most recent half-sweep since profile(True):
        dict(iterations, evaluations, nnz_iterations, nnz_evaluations)"""
        out = (C.c_ulonglong * 4)()
        if self.lib.poismf_hip_session_decision_stats(self.h, int(which), out):
            raise RuntimeError("poismf_hip_session_decision_stats: profiling is off")
        return dict(iterations=out[0], evaluations=out[1], nnz_iterations=out[2], nnz_evaluations=out[3])

    def nnz(self, which):
        return self.lib.poismf_hip_session_nnz(self.h, int(which))

    def add(self, coo):
        """X += coo on the resident matrix, both orientations, merged on the device (include/poismf_hip.h section 2b).  coo: a SciPy
        sparse matrix (or any object with row / col / data / shape) of the session's shape whose values are finite and > 0;
        triplets repeated inside it are summed first (in input order, section 1c), a cell the session already stores then gets one rounded addition, a new
        cell is inserted at its place.  Returns the number of cells that were not stored before.  ValueError -- before anything
        changes -- for a wrong shape, an index outside the matrix, a value that is not finite and positive, and for a session
        that cannot be merged into: one that holds a shard, or whose host CSR / CSC had a row that was not strictly ascending."""
        if hasattr(coo, "tocoo"):
            coo = coo.tocoo()
        if tuple(coo.shape) != (self.dimA, self.dimB):
            raise ValueError(f"add: the update has shape {tuple(coo.shape)}, the session {(self.dimA, self.dimB)}")
        row, col = _index_array(coo.row, "add: row indices"), _index_array(coo.col, "add: column indices")
        val = np.ascontiguousarray(coo.data, dtype=np.float32 if self.use_float else np.float64)
        if not (row.ndim == col.ndim == val.ndim == 1 and len(row) == len(col) == len(val)):
            raise ValueError("add: row, col and data must be one-dimensional and of one length")
        if len(val) == 0:
            return 0
        if int(row.max()) >= self.dimA or int(col.max()) >= self.dimB:
            raise ValueError("add: a row / column index lies outside the matrix")
        if not (np.isfinite(val).all() and (val > 0).all()):
            raise ValueError("add: every value must be finite and > 0 (counts are taken back with subtract / remove)")
        if len(val) >= 2 ** 32:
            raise ValueError("add: at most 2^32 - 1 triplets per call")
        fresh = C.c_size_t(0)
        rc = self.lib.poismf_hip_session_add_coo(self.h, _ptr(row), _ptr(col), _ptr(val), len(val), C.byref(fresh))
        if rc == 3:
            raise ValueError("add: a row / column index lies outside the matrix")
        if rc == 4:
            raise ValueError("add: every value must be finite and > 0 (counts are taken back with subtract / remove)")
        if rc == 5:
            raise ValueError("add: this session cannot be merged into: it holds a shard of the matrix, or a row of its CSR / CSC "
                             "is not strictly ascending (Session.from_coo sessions always qualify)")
        if rc:
            raise MemoryError("poismf_hip_session_add_coo failed (out of memory or a device error)")
        return fresh.value

    def _take_back(self, name, coo, values, missing):
        """subtract's and remove's checks and call: (row, col[, val]) of coo against the session, then poismf_hip_session_sub_coo"""
        if missing not in ("raise", "ignore"):
            raise ValueError(f"{name}: missing must be 'raise' or 'ignore', not {missing!r}")
        if hasattr(coo, "tocoo"):
            coo = coo.tocoo()
        if tuple(coo.shape) != (self.dimA, self.dimB):
            raise ValueError(f"{name}: the update has shape {tuple(coo.shape)}, the session {(self.dimA, self.dimB)}")
        row, col = _index_array(coo.row, f"{name}: row indices"), _index_array(coo.col, f"{name}: column indices")
        val = np.ascontiguousarray(coo.data, dtype=np.float32 if self.use_float else np.float64) if values else None
        if not (row.ndim == col.ndim == 1 and len(row) == len(col)) or (values and not (val.ndim == 1 and len(val) == len(row))):
            raise ValueError(f"{name}: row, col{' and data' if values else ''} must be one-dimensional and of one length")
        if len(row) == 0:
            return 0
        if int(row.max()) >= self.dimA or int(col.max()) >= self.dimB:
            raise ValueError(f"{name}: a row / column index lies outside the matrix")
        if values and not (np.isfinite(val).all() and (val > 0).all()):
            raise ValueError(f"{name}: every value must be finite and > 0")
        if len(row) >= 2 ** 32:
            raise ValueError(f"{name}: at most 2^32 - 1 triplets per call")
        removed, absent = C.c_size_t(0), C.c_size_t(0)
        rc = self.lib.poismf_hip_session_sub_coo(self.h, _ptr(row), _ptr(col), _ptr(val) if values else None, len(row), int(missing == "raise"),
                                                 C.byref(removed), C.byref(absent))
        if rc == 3:
            raise ValueError(f"{name}: a row / column index lies outside the matrix")
        if rc == 4:
            raise ValueError(f"{name}: every value must be finite and > 0")
        if rc == 5:
            raise ValueError(f"{name}: this session cannot be changed in place: it holds a shard of the matrix, or a row of its CSR / CSC "
                             "is not strictly ascending (Session.from_coo sessions always qualify)")
        if rc == 6:
            raise ValueError(f"{name}: {absent.value} listed cell(s) are not stored in the session (missing='ignore' skips them); nothing was changed")
        if rc:
            raise MemoryError("poismf_hip_session_sub_coo failed (out of memory or a device error)")
        return removed.value

    def subtract(self, coo, missing="raise"):
        """X -= coo on the resident matrix, both orientations, on the device (include/poismf_hip.h section 2c).  coo: a SciPy sparse matrix
        (or any object with row / col / data / shape) of the session's shape whose values are finite and > 0; triplets repeated inside it are
        summed first (in input order, section 1c), a stored cell then gets one rounded subtraction and stays if and only if the difference
        is > 0: otherwise the cell leaves the matrix (no zero or negative value is ever stored).  A listed cell the session does not store
        raises ValueError with missing="raise" -- before anything changes -- and is skipped with missing="ignore".  Returns the number of
        cells removed.  ValueError, before anything changes, also for a wrong shape, an index outside the matrix, a value that is not finite
        and positive, and a session that cannot be changed in place (add's rule).  The factors are untouched: see retract."""
        return self._take_back("subtract", coo, True, missing)

    def remove(self, cells, missing="ignore"):
        """The listed cells leave the resident matrix, whatever they hold (section 2c).  cells: a sparse matrix or any object with row, col
        and shape; its values are not read, a cell listed twice is removed once.  missing as in subtract.  Returns the number of cells removed."""
        return self._take_back("remove", cells, False, missing)

    def forget(self, which, rows):
        """Every stored cell of the listed users (which = 1) or items (which = 0) leaves the resident matrix, in both orientations (section 2c):
        the rows stay, with length 0, and so do their factor rows.  rows: global, distinct, inside the matrix, any order.  Returns the
        number of cells removed."""
        if which not in (0, 1):
            raise ValueError(f"forget: which must be 0 (items) or 1 (users), not {which!r}")
        dim = self.dimA if which else self.dimB
        rows = np.asarray(rows)
        if rows.ndim != 1:
            raise ValueError("forget: rows must be one-dimensional")
        if rows.size and not (np.issubdtype(rows.dtype, np.integer) and rows.dtype != np.bool_):
            raise ValueError("forget: rows must be integers")
        if rows.size and (int(rows.min()) < 0 or int(rows.max()) >= dim):
            raise ValueError(f"forget: a row lies outside the matrix's rows [0, {dim})")
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        if len(np.unique(rows)) != len(rows):
            raise ValueError("forget: a row is listed twice")
        if len(rows) == 0:
            return 0
        removed = C.c_size_t(0)
        rc = self.lib.poismf_hip_session_remove_rows(self.h, int(which), _ptr(rows), len(rows), C.byref(removed))
        if rc == 3:
            raise ValueError("forget: rows must be distinct and inside the matrix")
        if rc == 5:
            raise ValueError("forget: this session cannot be changed in place: it holds a shard of the matrix, or a row of its CSR / CSC "
                             "is not strictly ascending (Session.from_coo sessions always qualify)")
        if rc:
            raise MemoryError("poismf_hip_session_remove_rows failed (out of memory or a device error)")
        return removed.value

    def decay(self, gamma=1.0, floor=0.0, users=None, items=None):
        """Every stored count is scaled on the device, in both orientations, and what fades leaves (include/poismf_hip.h section 2e): cell
        (u, i) holding x becomes ((x * gamma) * users[u]) * items[i] -- three multiplications in the session's precision, in this order,
        each rounded once -- and stays if and only if that is > floor; otherwise the cell leaves the matrix (no zero or negative value is
        ever stored; a subnormal result stays).  gamma, floor: finite and >= 0, rounded to the session's precision.  users / items: an
        array-like of one factor per user (length dimA) / per item (length dimB), finite and >= 0, or None: all ones; a 0 forgets the row.
        Time decay is decay(0.9) once per period.  Returns the number of cells removed; when it is 0 only the values were rewritten, in
        place.  ValueError -- before anything changes -- for a gamma, floor or factor that is negative, NaN or infinite, a vector that is
        not one-dimensional, of the wrong length or boolean, a scaled value that is not finite (a factor above 1 overflowed), and a session
        that cannot be changed in place (add's rule).  The factors are untouched, and every row has changed: refit with sweep or half_sweep."""
        dt = np.float32 if self.use_float else np.float64
        scalars = {}
        for name, v in (("gamma", gamma), ("floor", floor)):
            v = self.real(v)
            if not (np.isfinite(v) and v >= 0):
                raise ValueError(f"decay: {name} must be finite and >= 0, not {v!r}")
            scalars[name] = v
        vectors = {}
        for name, v, dim in (("users", users, self.dimA), ("items", items, self.dimB)):
            if v is None:
                vectors[name] = None
                continue
            v = np.asarray(v)
            if v.ndim != 1:
                raise ValueError(f"decay: {name} must be one-dimensional")
            if v.dtype == np.bool_:
                raise ValueError(f"decay: {name} must be numbers, not booleans")
            if len(v) != dim:
                raise ValueError(f"decay: {name} has {len(v)} entries, the session {dim}")
            v = np.ascontiguousarray(v, dtype=dt)
            if not (np.isfinite(v).all() and (v >= 0).all()):
                raise ValueError(f"decay: every entry of {name} must be finite and >= 0")
            vectors[name] = v
        removed = C.c_size_t(0)
        su, si = (None if v is None else _ptr(v) for v in (vectors["users"], vectors["items"]))
        rc = self.lib.poismf_hip_session_scale(self.h, scalars["gamma"], su, si, scalars["floor"], C.byref(removed))
        if rc == 4:
            raise ValueError("decay: gamma, floor and every entry of users / items must be finite and >= 0")
        if rc == 5:
            raise ValueError("decay: this session cannot be changed in place: it holds a shard of the matrix, or a row of its CSR / CSC "
                             "is not strictly ascending (Session.from_coo sessions always qualify)")
        if rc == 7:
            raise ValueError("decay: a scaled value is not finite; nothing was changed")
        if rc:
            raise MemoryError("poismf_hip_session_scale failed (out of memory or a device error)")
        return removed.value

    def _grown(self, which, n):
        """the Python object follows a growth the library has made: the dimension and the shard every serving check reads"""
        if which:
            self.dimA += n
            self.shardA = (0, self.dimA)
        else:
            self.dimB += n
            self.shardB = (0, self.dimB)

    def _append_rc(self, rc, name):
        if rc == 3:
            raise ValueError("append: an index of the new rows lies outside the other dimension, or a row is not strictly ascending")
        if rc == 4:
            raise ValueError("append: every value must be finite and > 0")
        if rc == 5:
            raise ValueError("append: this session cannot grow in place: it holds a shard of the matrix, a row of its CSR / CSC is not strictly "
                             "ascending (Session.from_coo sessions always qualify), or there are no new rows to adopt")
        if rc:
            raise MemoryError(f"{name} failed (out of memory, a device error, or a dimension beyond 2^31 - 1)")

    def append(self, which, X_new=None, factors=None, n_new=None):
        """New users (which = 1) or new items (which = 0) join the resident model in place (include/poismf_hip.h section 2d): the matrix
        gets n new rows (users) or columns (items) numbered from the old dimension on, the factor n new rows.  X_new: a SciPy sparse matrix
        with one row per new row and the OTHER dimension's width (dimB columns for users, dimA for items), values finite and > 0; it is
        converted to CSR with duplicates summed and indices sorted; None: the new rows are empty, and n_new says how many.  factors:
        [n x k], the new rows of the factor; None: zeros.  Afterwards the session is bit for bit a fresh Session.from_coo on the grown
        matrix with set_factors of the grown factors.  Returns the first new row number.  ValueError -- before anything changes -- for
        a which other than 0 / 1, a wrong width, a wrong factor shape, factors that are not finite, values that are not finite and
        positive, and a session that cannot grow in place (add's rule); MemoryError when the device runs out of memory."""
        if which not in (0, 1) or isinstance(which, bool):
            raise ValueError(f"append: which must be 0 (items) or 1 (users), not {which!r}")
        other = self.dimB if which else self.dimA
        n, data, indptr, indices, F = _append_rows_args(X_new, factors, n_new, other, self.k, self.use_float)
        first = C.c_size_t(self.dimA if which else self.dimB)
        if n == 0:
            return first.value
        rc = self.lib.poismf_hip_session_append_rows(self.h, int(which), n, _ptr(F) if F is not None else None, _opt_ptr(data),
                                                     _ptr(indptr) if indptr is not None else None, _opt_ptr(indices), C.byref(first))
        self._append_rc(rc, "poismf_hip_session_append_rows")
        self._grown(which, n)
        return first.value

    def adopt_new(self):
        """The rows of the last transform / topn_new / rank_new call become resident users, their solved factors their rows of A, without
        leaving the device (section 2d).  Returns (first new user, number of new users).  ValueError when there is no such call to adopt,
        when one of its rows was not strictly ascending or held a value that is not > 0, and for a session that cannot grow in place."""
        first, n = C.c_size_t(self.dimA), C.c_size_t(0)
        self._append_rc(self.lib.poismf_hip_session_adopt_new(self.h, C.byref(first), C.byref(n)), "poismf_hip_session_adopt_new")
        self._grown(1, n.value)
        return first.value, n.value

    def append_users(self, X_new, params, niter, factors=None, Bsum=None, Amean=None):
        """New users join the model.  factors=None: transform(X_new, params, niter, Bsum, Amean) folds them in against the resident B, then
        adopt_new() makes them resident -- rows, cells and solved factors stay on the device (Bsum / Amean as in transform: serving
        code passes them in).  Otherwise append(1, X_new, factors).  Returns the new users' numbers."""
        if factors is not None:
            first = self.append(1, X_new, factors)
            return np.arange(first, self.dimA, dtype=np.int64)
        _append_rows_args(X_new, None, None, self.dimB, self.k, self.use_float)   # (adopt_new refuses what append would: say so before the solve)
        if X_new.shape[0] == 0:
            return np.zeros(0, np.int64)
        self.transform(X_new, params, niter, Bsum=Bsum, Amean=Amean)
        first, n = self.adopt_new()
        return np.arange(first, first + n, dtype=np.int64)

    def append_items(self, X_new, params, step_size, start=None):
        """New items join the model: append(0, X_new, factors = start in every row), then half_sweep_rows(0, the new items) with this step and
        cnst_div(params.l2_reg, step_size).  ONE LOCAL REFIT of the new rows of B against the resident A, not the reference's step
        schedule (as in update).  X_new: one row per new item, dimA columns.  start: a [k] vector, the point every new item starts from;
        its default is the column means of the resident B, AT THE COST OF DOWNLOADING BOTH FACTORS: serving code computes it once and
        passes it in.  Returns the new items' numbers."""
        dt = np.float32 if self.use_float else np.float64
        if start is None:
            start = self.get_factors()[1].mean(axis=0)
        start = np.ascontiguousarray(start, dtype=dt).reshape(-1)
        if len(start) != self.k:
            raise ValueError(f"append_items: start must have k = {self.k} entries")
        n = X_new.shape[0] if hasattr(X_new, "shape") and len(X_new.shape) == 2 else 0
        first = self.append(0, X_new, np.ascontiguousarray(np.broadcast_to(start, (n, self.k))))
        items = np.arange(first, self.dimB, dtype=np.int64)
        step_size = self.real(step_size)
        self.half_sweep_rows(0, items, params, step_size, self.cnst_div(params.l2_reg, step_size))
        return items

    def matrix(self, which):
        """(values, indices, indptr) of the resident CSR shard (which = 1) or CSC shard (which = 0), downloaded: the layout of the
        csr / csc tuples Session() takes, indptr local to the shard.  The only way to see the CSR of a from_coo session."""
        lo, hi = self.shardA if which else self.shardB
        nnz = self.nnz(which)
        val = np.empty(nnz, np.float32 if self.use_float else np.float64)
        ind, ptr = np.empty(nnz, np.uint64), np.empty(hi - lo + 1, np.uint64)
        if self.lib.poismf_hip_session_get_matrix(self.h, int(bool(which)), _ptr(ptr), _ptr(ind), _ptr(val)):
            raise RuntimeError("poismf_hip_session_get_matrix failed")
        return val, ind, ptr

    def half_sweep_rows(self, which, rows, params, step_size, cnst_div, want_unchanged=False):
        """half_sweep over the listed rows of half `which` only (0: rows of B, 1: rows of A; global row numbers, distinct, inside
        the shard, any order): every listed row gets the bits a full half_sweep from the same factors would give it, every other
        row of the moving factor keeps its own.  Returns the listed rows found unchanged (TNCG early stop, want_unchanged)."""
        lo, hi = self.shardA if which else self.shardB
        rows = np.asarray(rows)
        if rows.ndim != 1:
            raise ValueError("half_sweep_rows: rows must be one-dimensional")
        if rows.size and not (np.issubdtype(rows.dtype, np.integer) and rows.dtype != np.bool_):
            raise ValueError("half_sweep_rows: rows must be integers")
        if rows.size and (int(rows.min()) < lo or int(rows.max()) >= hi):
            raise ValueError(f"half_sweep_rows: a row lies outside the session's rows [{lo}, {hi})")
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        if len(np.unique(rows)) != len(rows):
            raise ValueError("half_sweep_rows: a row is listed twice")
        if len(rows) == 0:
            return 0
        n = C.c_size_t(0)
        rc = self.lib.poismf_hip_half_sweep_rows(self.h, int(bool(which)), _ptr(rows), len(rows), C.byref(params), step_size, cnst_div,
                                                 C.byref(n) if want_unchanged else None)
        if rc == 3:
            raise ValueError("half_sweep_rows: rows must be distinct and inside the session's shard")
        if rc:
            raise RuntimeError("poismf_hip_half_sweep_rows failed")
        return n.value

    def update(self, coo, params, step_size):
        """A returning user: add(coo), then half_sweep_rows(1, users) and half_sweep_rows(0, items) over the sorted distinct rows /
        columns of coo, both with this step and cnst_div(params.l2_reg, step_size).  ONE LOCAL REFIT of the touched rows against
        the current factors, not the reference's step schedule (no halving between the halves, no sweep over the other rows).
        Returns (users, items)."""
        if hasattr(coo, "tocoo"):
            coo = coo.tocoo()
        self.add(coo)
        users, items = np.unique(np.asarray(coo.row)).astype(np.int64), np.unique(np.asarray(coo.col)).astype(np.int64)
        step_size = self.real(step_size)
        cnst_div = self.cnst_div(params.l2_reg, step_size)
        self.half_sweep_rows(1, users, params, step_size, cnst_div)
        self.half_sweep_rows(0, items, params, step_size, cnst_div)
        return users, items

    def retract(self, coo, params, step_size, remove=False):
        """Counts taken back from known users: subtract(coo) -- or remove(coo) with remove=True -- then half_sweep_rows(1, users) and
        half_sweep_rows(0, items) over the sorted distinct rows / columns of coo, both with this step and cnst_div(params.l2_reg, step_size):
        exactly update's refit.  ONE LOCAL REFIT of the touched rows against the current factors, not the reference's step schedule.
        Returns (users, items)."""
        if hasattr(coo, "tocoo"):
            coo = coo.tocoo()
        if remove:
            self.remove(coo)
        else:
            self.subtract(coo)
        users, items = np.unique(np.asarray(coo.row)).astype(np.int64), np.unique(np.asarray(coo.col)).astype(np.int64)
        step_size = self.real(step_size)
        cnst_div = self.cnst_div(params.l2_reg, step_size)
        self.half_sweep_rows(1, users, params, step_size, cnst_div)
        self.half_sweep_rows(0, items, params, step_size, cnst_div)
        return users, items

    def predict(self, ix_u, ix_i):
        """A[ix_u[i]] . B[ix_i[i]] from the resident factors (ref: src/pred.c:42-64)"""
        ix_u = np.ascontiguousarray(ix_u, dtype=np.uint64)
        ix_i = np.ascontiguousarray(ix_i, dtype=np.uint64)
        out = np.empty(len(ix_u), np.float32 if self.use_float else np.float64)
        rc = self.lib.poismf_hip_session_predict(self.h, _ptr(ix_u), _ptr(ix_i), len(ix_u), _ptr(out))
        if rc == 2:
            raise IndexError("user / item index out of range")
        if rc:
            raise MemoryError("poismf_hip_session_predict failed")
        return out

    def topn(self, user, top_n=10, include_ix=(), exclude_ix=(), output_score=False):
        """top-N items of user `user` (row of the resident A) by score, descending (ref: src/topN.c:112-284)"""
        inc = np.ascontiguousarray(include_ix, dtype=np.uint64)
        exc = np.ascontiguousarray(exclude_ix, dtype=np.uint64)
        ix = np.empty(top_n, np.uint64)
        sc = np.empty(top_n if output_score else 0, np.float32 if self.use_float else np.float64)
        rc = self.lib.poismf_hip_session_topn(self.h, int(user), _ptr(inc) if len(inc) else None, len(inc), _ptr(exc) if len(exc) else None,
                                              len(exc), _ptr(ix), _ptr(sc) if output_score else None, int(top_n))
        if rc == 2:
            raise ValueError("invalid combination of include / exclude / top_n, or an index out of range")
        if rc:
            raise MemoryError("poismf_hip_session_topn failed")
        return ix, sc

    def _entry(self, name, exclude_seen):
        """a serving call (serving.py) on this session: the library's function for `name`, its leading argument, and what stands in
        front of the exclusion lists"""
        return getattr(self.lib, "poismf_hip_session_" + name), (self.h,), (int(bool(exclude_seen)),)

    def topn_batch(self, users, top_n=10, exclude_seen=False, exclude=None, output_score=False, include=None, include_of=None):
        """The top_n best items of every user in `users` from the resident factors, in one fused pass (include/poismf_hip.h section
        1f): "score descending, item index ascending", scores bit for bit those of predict().  exclude_seen leaves out the items of
        the user's row of the session's own CSR; exclude (a SciPy sparse matrix with one row per entry of `users`, or an
        (indptr, indices) pair with strictly ascending rows) leaves out more.  Returns (items uint64 [m x top_n], scores [m x top_n],
        empty unless output_score).  include (same two forms) gives every user a candidate list of its own: it is ranked among
        that list only, and only those rows of B are read (section 1h); top_n may then exceed what a user has left, and the row
        is padded with TOPN_NONE and -inf.  include_of makes `include` a TABLE of lists shared between users (G >= 1 rows) and
        names each user's row of it -- an integer array with one entry per user, or one int for all (section 1i): the same answers
        bit for bit, the table read once and the rows of B shared by the users of a list.  Few lists for many users belong
        there, a list per user in include= alone."""
        return serving.topn_batch(self, users, top_n, exclude_seen, exclude, output_score, include, include_of)

    def topn_deep(self, users, top_n=1000, exclude_seen=False, exclude=None, output_score=False):
        """topn_batch for deep lists: the top_n <= TOPN_DEEP_MAX_N_TOP best items of every user in `users` from the resident factors
        in one fused pass (include/poismf_hip.h section 1l); order, scores, exclude_seen and exclude as in topn_batch.  top_n may
        exceed what a user has left, or the number of items: the row is padded with TOPN_NONE and -inf.  Up to
        TOPN_BATCH_MAX_N_TOP the answers are topn_batch's bit for bit.  Returns (items uint64 [m x top_n], scores [m x top_n], empty
        unless output_score)."""
        return serving.topn_deep(self, users, top_n, exclude_seen, exclude, output_score)

    def topn_quota(self, users, top_n=10, group_of=None, quota=1, exclude_seen=False, exclude=None, output_score=False):
        """topn_batch with "at most quota[g] items of group g on a page", from the resident factors in one fused pass
        (include/poismf_hip.h section 1n): the user's complete ranked list (order, scores, exclude_seen and exclude as in topn_batch) is
        walked and an item is taken iff fewer than quota[g] items of its group group_of[item] were taken before it, until
        top_n <= TOPN_BATCH_MAX_N_TOP are taken.  group_of: one group id per item.  quota: one int for every group, or an array with
        one entry per group; 0 bars a group, top_n or more leaves it unconstrained.  A row the quotas leave short is padded with
        TOPN_NONE and -inf.  Returns (items uint64 [m x top_n], scores [m x top_n], empty unless output_score)."""
        return serving.topn_quota(self, users, top_n, group_of, quota, exclude_seen, exclude, output_score)

    def topn_weighted(self, users, top_n=10, item_weight=None, exclude_seen=False, exclude=None, output_score=False, query_items=False):
        """topn_batch under score x item_weight[item], from the resident factors in one fused pass (include/poismf_hip.h section 1o):
        the top_n <= TOPN_BATCH_MAX_N_TOP best items of every user under "weighted score descending, item index ascending";
        exclude_seen and exclude as in topn_batch.  item_weight: one finite weight >= 0 per item, or one number for all.  A weight of
        0 does not bar an item -- it scores 0 and ties with its like by index; exclude= bars one.  The scores returned are the
        weighted ones.  A short row is padded with TOPN_NONE and -inf.  query_items: `users` are rows of the resident B instead --
        the queries of an item-to-item call (similar_items); exclude_seen has no meaning then.  Returns (items uint64 [m x top_n],
        scores [m x top_n], empty unless output_score)."""
        return serving.topn_weighted(self, users, top_n, item_weight, exclude_seen, exclude, output_score, bool(query_items))

    def topn_adjusted(self, users, top_n=10, adjust=None, exclude_seen=False, exclude=None, output_score=False):
        """topn_batch where single cells of the score matrix carry a factor of their own, from the resident factors, exact and in
        one call (include/poismf_hip.h section 1r): the top_n <= TOPN_BATCH_MAX_N_TOP best items of every user under "adjusted score
        descending, item index ascending"; exclude_seen and exclude as in topn_batch.  adjust: a SciPy sparse matrix with one row
        per user of the batch whose stored values are finite factors >= 0 (stored zeros are kept), or an (indptr, indices, factors)
        triple; None lists no cell.  A factor of 0 does not bar a cell -- it scores 0 and ties with its like by index; a cell both
        listed and excluded is excluded.  The scores returned are the adjusted ones.  A short row is padded with TOPN_NONE and -inf.
        Returns (items uint64 [m x top_n], scores [m x top_n], empty unless output_score)."""
        return serving.topn_adjusted(self, users, top_n, adjust, exclude_seen, exclude, output_score)

    def item_norms(self):
        """n2[j] = the fused chain of row j of the resident B with itself, predict_multiple's bits: what similar_items takes as
        item_norm=.  The factors come to the host for it, so a serving loop computes it once per model."""
        B = self.get_factors()[1]
        every = np.arange(self.dimB, dtype=np.uint64)
        n2 = np.empty(self.dimB, B.dtype)
        _predict_multiple(n2, B, B, every, every)
        return n2

    def similar_items(self, items, top_n=10, output_score=False, exclude_self=True, item_norm=None):
        """The top_n best items by cosine similarity of their rows of the resident B to each item of `items`: PoisMF.similar_items from
        the session, through topn_weighted(query_items=True).  item_norm: item_norms(), computed once per model; without it every
        call computes it again, which brings the factors to the host."""
        return serving.similar_items(self, items, top_n, output_score, exclude_self, item_norm, query_items=True)

    def topn_diverse(self, users, top_n=10, pool=100, lam=0.7, exclude_seen=False, exclude=None, output_score=False, output_value=False,
                     item_norm=None):
        """topn_batch diversified from the factors themselves, from the resident factors: PoisMF.topN_diverse from the session
        (include/poismf_hip.h section 1p) -- of every user's best `pool` items (topn_deep's list; exclude_seen and exclude as in
        topn_batch) top_n are picked one by one by greedy maximal marginal relevance with weight lam on the relevance.  item_norm:
        item_norms(), computed once per model; without it every call computes it again, which brings the factors to the host.
        Returns (items uint64 [m x top_n] in pick order, their scores, empty unless output_score, the values they were picked at,
        empty unless output_value); a short row is padded with TOPN_NONE and -inf."""
        return serving.topn_diverse(self, users, top_n, pool, lam, exclude_seen, exclude, output_score, output_value, item_norm)

    def rank_batch(self, users, test, exclude_seen=False, exclude=None, include=None, include_of=None, unite_test=False):
        """For every cell of `test` (a SciPy sparse matrix with one row per entry of `users`, or an (indptr, indices) pair with
        strictly ascending rows) the 0-based position of its item in the user's complete ranked list from the resident factors
        (include/poismf_hip.h section 1g); exclude_seen / exclude as in topn_batch.  Returns (ranks uint32, one per cell in row
        order, RANK_EXCLUDED where the item is excluded; n_adm uint32 [m], the admissible items of each user).  include (same two
        forms, passed as given) gives every user a candidate list of its own: a cell is ranked among that list only, minus the
        exclusions, only those rows of B are read, and a cell whose item is not listed gets RANK_EXCLUDED too (section 1j).
        include_of makes `include` a TABLE of lists shared between users (G >= 1 rows) and names each user's row of it -- an integer
        array with one entry per batch entry, or one int for all (section 1k): the same answers, the table read once and the rows
        of B shared by the users of a list.  unite_test (with include_of only) ranks every user among its list united with its own
        held-out row, which is what a shared pool of negatives needs."""
        return serving.rank_batch(self, users, test, exclude_seen, exclude, include, include_of, unite_test)

    def eval_ranking(self, X_test, k=10, exclude_seen=True, exclude=None, users=None, per_user=False, include=None, include_of=None):
        """PoisMF.eval_ranking from the resident factors; exclude_seen leaves out the items of the user's row of the session's own
        CSR (nothing is uploaded), exclude leaves out more; include as there (sampled evaluation, section 1j), include with
        include_of as there too (pools shared between users, section 1k)."""
        users, test, exclude, k = _eval_ranking_args(X_test, exclude, users, k, self.dimA, self.dimB)
        if include_of is not None:
            ranks, n_adm = self.rank_batch(users, test, exclude_seen=exclude_seen, exclude=exclude, include=include,
                                           include_of=_include_of_rows(include_of, users, self.dimA), unite_test=True)
            return _ranking_result(test[0], ranks, n_adm, k, per_user)
        if include is not None:
            include = _unite_rows(_include_rows(include, users, self.dimA, self.dimB), test)
        ranks, n_adm = self.rank_batch(users, test, exclude_seen=exclude_seen, exclude=exclude, include=include)
        return _ranking_result(test[0], ranks, n_adm, k, per_user)

    def list_eval(self, items, test=None, item_norm=None, budget_mb=None):
        """api.list_eval against the resident B (include/poismf_hip.h section 1q): no factor is uploaded.  Returns (pos, cos_sum,
        length, exposure) as there."""
        dt = np.float32 if self.use_float else np.float64
        lists, tp, ti, inv, budget = _list_eval_args(items, test, item_norm, budget_mb, self.dimB, self.k, dt)
        pos, cos, length, expo = _list_eval_outputs(lists, ti, inv, self.dimB)
        if lists.shape[0] == 0:
            return pos, cos, length, expo
        _batch_rc(self.lib.poismf_hip_session_list_eval(self.h, _ptr(lists), lists.shape[0], lists.shape[1], _opt_ptr(inv), _opt_ptr(tp),
                                                        _opt_ptr(ti), budget, _opt_ptr(pos), _opt_ptr(cos), _ptr(length), _ptr(expo)),
                  "list evaluation")
        return pos, cos, length, expo

    def eval_lists(self, items, users=None, X_test=None, k=None, exclude=None, item_norm=None, item_pop=None, per_user=False):
        lists, test, item_pop = _eval_lists_args(items, users, X_test, k, exclude, item_pop, self.dimA, self.dimB)
        if item_norm is None:
            dt = np.float32 if self.use_float else np.float64
            _list_eval_args(lists, test, None, None, self.dimB, self.k, dt)   # (everything else is judged before the norms are computed)
            item_norm = self.item_norms()
        pos, cos, length, expo = self.list_eval(lists, test, item_norm)
        return _lists_result(lists, test, pos, cos, length, expo, item_pop, per_user)

    eval_lists.__doc__ = _EVAL_LISTS_DOC

    def _new_rows(self, X_new, params, niter, Bsum, Amean):
        """what every fold-in call starts with (include/poismf_hip.h section 1m): the leading arguments of the C entry point, the
        number of new rows, and the arrays those arguments point into"""
        data, indptr, indices = _new_rows_args(X_new, self.dimB, self.use_float)
        if Bsum is None or Amean is None:
            if self.shardA != (0, self.dimA) or self.shardB != (0, self.dimB):
                raise ValueError("this session updates only a shard of the factors: pass Bsum and Amean of the whole model")
            A, B = self.get_factors()
            Bsum = B.sum(axis=0) + params.l1_reg if Bsum is None else Bsum      # as PoisMF.fit leaves them
            Amean = A.mean(axis=0) if Amean is None else Amean
        Bsum, Amean = _new_stats(Bsum, Amean, self.k, self.use_float)
        keep = (data, indptr, indices, Bsum, Amean)
        return [self.h, _opt_ptr(data), _ptr(indptr), _opt_ptr(indices), len(indptr) - 1, _ptr(Bsum), _ptr(Amean), C.byref(params),
                int(niter)], len(indptr) - 1, keep

    def transform(self, X_new, params, niter, Bsum=None, Amean=None):
        """Factors A_new [n_new x k] of users the model has never seen, against the resident B (section 1m): bit for bit those of
        factors_multiple / PoisMF.transform with the same B, Bsum, Amean and solver arguments, without B travelling.  X_new: a SciPy
        CSR / COO matrix with dimB columns, one row per new user (duplicates summed, indices sorted).  params as make_params gives
        them (method, l2_reg, w_mult, step_size, limit_step, maxupd; reuse_prev starts every row at Amean also for tncg; l1_reg
        and early_stop play no part in the solve).  Bsum (column sums of B plus l1) and Amean (column means of A) default to what
        PoisMF.fit would leave for the resident factors -- B.sum(axis=0) + params.l1_reg and A.mean(axis=0) -- AT THE COST OF
        DOWNLOADING BOTH FACTORS: serving code computes them once and passes them in."""
        args, m, keep = self._new_rows(X_new, params, niter, Bsum, Amean)
        A_new = np.empty((m, self.k), np.float32 if self.use_float else np.float64)
        if m:
            _batch_rc(self.lib.poismf_hip_session_factors_new(*args, _ptr(A_new)), "factors of new rows")
        return A_new

    def topn_new(self, X_new, params, niter, top_n=10, exclude_own=True, exclude=None, output_score=False, return_factors=False,
                 Bsum=None, Amean=None):
        """The top_n best items of every new user of X_new: transform()'s factors ranked against the resident B as topn_batch ranks
        resident users, in one call, the factors staying on the device unless return_factors (section 1m).  exclude_own leaves
        out the items of the user's own row of X_new (read from the copy the solve uses); exclude (a SciPy sparse matrix with one
        row per new user, or an (indptr, indices) pair with strictly ascending rows) leaves out more.  Bsum / Amean as in
        transform().  Returns (items uint64 [m x top_n], scores [m x top_n], empty unless output_score), and with return_factors
        a third entry, A_new."""
        args, m, keep = self._new_rows(X_new, params, niter, Bsum, Amean)
        n = int(top_n)
        _, ep, ei = _topn_batch_args(np.arange(m, dtype=np.uint64), n, exclude, max(m, 1), self.dimB)
        dt = np.float32 if self.use_float else np.float64
        ix, sc = _topn_outputs(m, n, dt, output_score)
        A_new = np.empty((m, self.k), dt) if return_factors else None
        if m:
            _batch_rc(self.lib.poismf_hip_session_topn_new(*args, n, int(bool(exclude_own)), _opt_ptr(ep), _opt_ptr(ei), _ptr(ix),
                                                           _opt_ptr(sc), _opt_ptr(A_new)), "top-N of new rows")
        return (ix, sc, A_new) if return_factors else (ix, sc)

    def rank_new(self, X_new, test, params, niter, exclude_own=True, exclude=None, return_factors=False, Bsum=None, Amean=None):
        """For every cell of `test` (a SciPy sparse matrix with one row per new user, or an (indptr, indices) pair with strictly
        ascending rows) the 0-based position of its item in the new user's complete ranked list, as rank_batch gives it for a
        resident user, from transform()'s factors (section 1m); exclude_own / exclude / Bsum / Amean as in topn_new.  Returns (ranks
        uint32, one per cell in row order, RANK_EXCLUDED where the item is excluded; n_adm uint32 [m]), and with return_factors a
        third entry, A_new."""
        args, m, keep = self._new_rows(X_new, params, niter, Bsum, Amean)
        _, tp, ti, ep, ei = _rank_batch_args(np.arange(m, dtype=np.uint64), test, exclude, max(m, 1), self.dimB, self.k)
        ranks, n_adm = np.empty(len(ti), np.uint32), np.empty(m, np.uint32)
        A_new = np.empty((m, self.k), np.float32 if self.use_float else np.float64) if return_factors else None
        if m:
            _batch_rc(self.lib.poismf_hip_session_rank_new(*args, _ptr(tp), _opt_ptr(ti), int(bool(exclude_own)), _opt_ptr(ep),
                                                           _opt_ptr(ei), _ptr(ranks), _ptr(n_adm), _opt_ptr(A_new)), "ranks of new rows")
        return (ranks, n_adm, A_new) if return_factors else (ranks, n_adm)

    def eval_ranking_new(self, X_observed, X_test, params, niter, k=10, per_user=False, exclude_own=True, exclude=None, Bsum=None,
                         Amean=None):
        """Held-out ranking metrics under strong generalisation: users held out of training are folded in on X_observed (one row per
        user, dimB columns) and ranked on X_test (same shape; its stored cells are the held-out positives, values play no part,
        explicit zeros dropped).  The ranks are rank_new's, the metrics those of poismf_amd/metrics.py, the result eval_ranking's:
        the means of hit, precision, recall, ap, ndcg, rr, auc at cut-off k over the users that counted, plus n_users; with
        per_user also "per_user", "ranks", "n_adm" and "test_indptr"."""
        import scipy.sparse as sp
        k = int(k)
        if k < 1:
            raise ValueError("k must be at least 1")
        if not sp.issparse(X_test) or X_test.shape != X_observed.shape:
            raise ValueError("X_test must be a SciPy sparse matrix of X_observed's shape")
        test = sp.csr_matrix(X_test)
        test.sum_duplicates(); test.eliminate_zeros(); test.sort_indices()
        tp = np.asarray(test.indptr, np.uint64)
        ranks, n_adm = self.rank_new(X_observed, (tp, np.asarray(test.indices, np.uint64)), params, niter, exclude_own=exclude_own,
                                     exclude=exclude, Bsum=Bsum, Amean=Amean)
        return _ranking_result(tp, ranks, n_adm, k, per_user)

    def _text(self, fn, which):
        """a text report of the library, whole: ask for the length first (a fixed buffer cut long plans mid-item)"""
        n = fn(self.h, int(which), None, 0)
        buf = C.create_string_buffer(int(n) + 1)
        fn(self.h, int(which), buf, len(buf))
        return [item.strip() for item in buf.value.decode().split(";") if item.strip()]

    def plan(self, which):
        """the launches of the most recent half-sweep of half `which`: [(kernel instance, rows), ...]"""
        out = []
        for item in self._text(self.lib.poismf_hip_session_plan, which):
            name, rows = item.rsplit(" rows=", 1)
            out.append((name.strip(), int(rows)))
        return out

    def launch_profile(self, which):
        """per-launch timings of half `which` since profile(True): [dict(kernel, rows, nnz, calls, ms)], ms summed over calls"""
        out = []
        for item in self._text(self.lib.poismf_hip_session_launch_profile, which):
            name, rest = item.split(" rows=", 1)
            f = dict(kv.split("=") for kv in ("rows=" + rest).split())
            out.append(dict(kernel=name.strip(), rows=int(f["rows"]), nnz=int(f["nnz"]), calls=int(f["calls"]), ms=float(f["ms"])))
        return out
