"""ctypes binding of the bn-pp MI355X engine (include/bnpp.h).

This is plumbing for tests and bench.py: every call goes straight to
bn-pp_amd/lib/libbnpp.so.  There is no Python or CPU fallback — a missing
library raises ImportError and a missing GPU raises BnppError(NO_DEVICE).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Iterable, List, Optional, Sequence

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.normpath(os.path.join(_HERE, "..", "..", "lib", "libbnpp.so"))
if os.environ.get("BNPP_LIB"):          # A/B of alternative builds (experiments only)
    LIB_PATH = os.environ["BNPP_LIB"]

if not os.path.exists(LIB_PATH):
    raise ImportError("libbnpp.so not built (%s); run `make -C bn-pp_amd` or __graft_entry__.build()" % LIB_PATH)

# One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64.  When it
# is installed, load it first so libbnpp binds to that same runtime (with two
# runtimes in one process, whichever initialises second sees no device).
# BNPP_NO_TORCH=1 leaves PyTorch out of a process that does not use it: libbnpp
# then binds to ROCm's runtime.  That is also the way to run under
# HIP_ENABLE_DEFERRED_LOADING=0, where `import torch` itself segfaults on this
# image (PyTorch 2.10+rocm7.0, inside `from torch._C import *`).
if os.environ.get("BNPP_NO_TORCH") != "1":
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
_lib = C.CDLL(LIB_PATH)

OK, ERR_INVALID, ERR_NO_DEVICE, ERR_OOM, ERR_HIP, ERR_IO, ERR_UNSUPPORTED = 0, -1, -2, -3, -4, -5, -6
F64, F32 = 0, 1
LIK_LOG = 2                             # OR-ed into a _dv call's lik_dtype: natural logs (BNPP_LIK_LOG)
ORDER_GIVEN, MIN_FILL, WEIGHTED_MIN_FILL, MIN_DEGREE = 0, 1, 2, 3
HEURISTICS = {"given": ORDER_GIVEN, "mf": MIN_FILL, "wmf": WEIGHTED_MIN_FILL, "md": MIN_DEGREE}

_P = C.c_void_p
_I = C.c_int
_IP = C.POINTER(C.c_int)
_DP = C.POINTER(C.c_double)
_LP = C.POINTER(C.c_int64)
_UBP = C.POINTER(C.c_ubyte)
# bnpp_collective_fn (include/bnpp.h): (user, op, send, recv, bytes, stream) -> 0 on success
COLLECTIVE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)
COLL_ALLGATHER, COLL_ALLTOALL = 0, 1

_SIGS = {
    "bnpp_strerror": (C.c_char_p, [_I]),
    "bnpp_last_error": (C.c_char_p, []),
    "bnpp_version": (_I, []),
    "bnpp_last_timing": (_I, [_DP, _I]),
    "bnpp_device_count": (_I, [_IP]),
    "bnpp_ctx_create": (_I, [_I, C.POINTER(_P)]),
    "bnpp_ctx_destroy": (_I, [_P]),
    "bnpp_ctx_stream": (_I, [_P, C.POINTER(_P)]),
    "bnpp_ctx_trim": (_I, [_P]),
    "bnpp_ctx_set_max_grid": (_I, [_P, _I]),
    "bnpp_malloc": (_I, [_P, C.c_size_t, C.POINTER(_P)]),
    "bnpp_free": (_I, [_P, _P]),
    "bnpp_memcpy_h2d": (_I, [_P, _P, _P, C.c_size_t]),
    "bnpp_memcpy_d2h": (_I, [_P, _P, _P, C.c_size_t]),
    "bnpp_synchronize": (_I, [_P, _P]),
    "bnpp_out_scope": (_I, [_I, _IP, C.POINTER(_IP), _I, _I, _IP, _IP]),
    "bnpp_bucket_eliminate": (_I, [_P, _P, _I, _I, _IP, _I, C.POINTER(_P), _IP, C.POINTER(_IP), _I, _P, _I, _IP, _P]),
    "bnpp_bucket_max": (_I, [_P, _P, _I, _I, _IP, _I, C.POINTER(_P), _IP, C.POINTER(_IP), _I, _P, _I, _IP, _P]),
    "bnpp_bucket_sample": (_I, [_P, _P, _I, _I, _IP, _I, C.POINTER(_P), _IP, C.POINTER(_IP), _I, C.c_int64, C.c_int64,
                                C.c_uint64, _P, _P]),
    "bnpp_product": (_I, [_P, _P, _I, _I, _IP, _P, _I, _IP, _P, _I, _IP, _P, _I, _IP, _P]),
    "bnpp_divide": (_I, [_P, _P, _I, _I, _IP, _P, _I, _IP, _P, _I, _IP, _P, _I, _IP, _P]),
    "bnpp_sum_out": (_I, [_P, _P, _I, _I, _IP, _P, _I, _IP, _I, _P, _I, _IP, _P]),
    "bnpp_condition": (_I, [_P, _P, _I, _I, _IP, _P, _I, _IP, _I, _IP, _IP, _P, _P]),
    "bnpp_model_load_uai": (_I, [C.c_char_p, C.POINTER(_P)]),
    "bnpp_model_from_arrays": (_I, [_I, _I, _IP, _I, _IP, _IP, _DP, C.POINTER(_P)]),
    "bnpp_model_free": (_I, [_P]),
    "bnpp_model_info": (_I, [_P, _IP, _IP, _IP]),
    "bnpp_model_cards": (_I, [_P, _IP]),
    "bnpp_evidence_load": (_I, [C.c_char_p, _I, _IP, _IP, _IP]),
    "bnpp_ordering": (_I, [_P, _I, _IP, _IP, _I, _IP, _I, _IP, _IP]),
    "bnpp_partition": (_I, [_P, _P, _I, _IP, _IP, _I, _IP, _I, _I, _DP, _DP, _DP]),
    "bnpp_mpe": (_I, [_P, _P, _I, _IP, _IP, _I, _IP, _I, _I, _DP, _IP, _DP]),
    "bnpp_sample": (_I, [_P, _P, _I, _IP, _IP, _I, _IP, _I, _I, C.c_int64, C.c_int64, C.c_uint64, _P, _DP, _LP, _DP]),
    "bnpp_marginals": (_I, [_P, _P, _I, _IP, _IP, _I, _I, _IP, _I, _DP, _DP]),
    "bnpp_sum_product": (_I, [_P, _P, _I, C.c_double, _DP, _IP, _DP]),
    "bnpp_marginals_tree": (_I, [_P, _P, _I, _IP, _IP, _I, _IP, _I, _I, _IP, _I, _DP, _DP]),
    "bnpp_marginals_tree_part": (_I, [_P, _P, _I, _IP, _IP, _I, _IP, _I, _I, _IP, _I, _I, _I, _DP, _IP, _DP]),
    "bnpp_plan_tree_part": (_I, [_P, _I, _IP, _IP, _I, _IP, _I, _I, _I, _I, _IP, _DP, _I]),
    "bnpp_marginals_tree_sliced": (_I, [_P, _P, _I, _IP, _IP, _I, _IP, _I, _I, _IP, _I, _I, COLLECTIVE_FN, _P,
                                        C.c_double, _I, _DP, _LP, _DP]),
    "bnpp_collective_loopback": (_I, [_P, _I, _P, _P, C.c_int64, _P]),
    "bnpp_plan_tree_sliced": (_I, [_P, _I, _IP, _IP, _I, _IP, _I, _I, _I, _I, _IP, _DP, _I]),
    "bnpp_variable_elimination": (_I, [_P, _P, _I, _IP, _I, _I, _I, _IP, _IP, C.c_int64, C.POINTER(C.c_int64), _DP,
                                       C.POINTER(C.c_int64)]),
    "bnpp_plan_stats": (_I, [_P, _I, _I, _IP, _IP, _I, _IP, _I, _I, _DP, _I]),
    "bnpp_plan_single": (_I, [_I, _I, _IP, _I, _IP, C.POINTER(_IP), _I, _I, _IP, _I, _I, _IP, _IP, _LP, _I]),
    "bnpp_plan_max_single": (_I, [_I, _I, _IP, _I, _IP, C.POINTER(_IP), _I, _I, _IP, _LP, _I]),
    "bnpp_kernel_keys": (_I, [_I, _I, _I, _IP, _I, _IP]),
    "bnpp_chain_key_supported": (_I, [_I, _I, _IP]),
    "bnpp_plan_groups": (_I, [_P, _I, _I, _IP, _IP, _I, _IP, _I, _I, _I, _I, _LP, _I, _IP]),
    "bnpp_plan_mpe_groups": (_I, [_P, _I, _IP, _IP, _I, _IP, _I, _I, _LP, _I, _IP]),
    "bnpp_plan_sample": (_I, [_P, _I, _IP, _IP, _I, _IP, _I, _I, C.c_int64, _DP, _I, _LP, _I, _IP]),
    "bnpp_condition_batch": (_I, [_P, _P, _I, _I, _IP, _P, _I, _IP, _I, _IP, C.c_int64, _P, _P]),
    "bnpp_evidence_load_batch": (_I, [C.c_char_p, _I, C.c_int64, _IP, _IP, _LP, _IP]),
    "bnpp_partition_batch": (_I, [_P, _P, _I, _IP, C.c_int64, _IP, _I, _IP, _I, _I, C.c_int64, _DP, _DP, _DP]),
    "bnpp_posterior_batch": (_I, [_P, _P, _I, _IP, C.c_int64, _IP, _I, _I, _I, C.c_int64, _DP, _DP]),
    "bnpp_plan_batch": (_I, [_P, _I, _IP, _I, _IP, _I, _I, _I, C.c_int64, _DP, _I, _LP, _I, _IP, _IP, _IP]),
    "bnpp_mpe_batch": (_I, [_P, _P, _I, _IP, C.c_int64, _IP, _I, _IP, _I, _I, C.c_int64, _DP, _IP, _DP]),
    "bnpp_plan_mpe_batch": (_I, [_P, _I, _IP, _I, _IP, _I, _I, C.c_int64, _DP, _I, _LP, _I, _IP]),
    "bnpp_sample_batch": (_I, [_P, _P, _I, _IP, C.c_int64, _IP, _I, _IP, _I, _I, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                               C.c_uint64, _P, _DP, _LP, _DP]),
    "bnpp_plan_sample_batch": (_I, [_P, _I, _IP, _I, _IP, _I, _I, C.c_int64, C.c_int64, _DP, _I, _LP, _I, _IP]),
    "bnpp_counts_size": (_I, [_P, _LP]),
    "bnpp_expected_counts": (_I, [_P, _P, _I, _IP, C.c_int64, _IP, _DP, _I, _IP, _I, _I, C.c_int64, _DP, _DP, _LP, _DP]),
    "bnpp_plan_counts": (_I, [_P, _I, _IP, _I, _IP, _I, _I, C.c_int64, _DP, _I, _LP, _I, _IP, _IP, _IP, _I, _IP, _IP]),
    "bnpp_bucket_counts": (_I, [_P, _P, _I, _I, _IP, _P, _I, _IP, _I, _IP, C.c_int64, C.c_int64, _P, _P, _P, _I, _P]),
    "bnpp_marginals_batch": (_I, [_P, _P, _I, _IP, C.c_int64, _IP, _I, _IP, _I, _I, _IP, _I, C.c_int64, _DP, _DP, _DP]),
    "bnpp_plan_marginals_batch": (_I, [_P, _I, _IP, _I, _IP, _I, _I, _IP, _I, C.c_int64, _DP, _I, _LP, _I, _IP, _IP]),
    "bnpp_bucket_marginal_rows": (_I, [_P, _P, _I, _I, _IP, C.POINTER(_P), _IP, _IP, C.c_int64, C.c_int64, _P, _P]),
    # missing values: the _mv siblings take partial[n_ev] (after ev_vals; the plan entries: after ev_vars, and
    # return mask_factor[n_ev] last)
    "bnpp_partition_batch_mv": (_I, [_P, _P, _I, _IP, C.c_int64, _IP, _UBP, _I, _IP, _I, _I, C.c_int64, _DP, _DP, _DP]),
    "bnpp_posterior_batch_mv": (_I, [_P, _P, _I, _IP, C.c_int64, _IP, _UBP, _I, _I, _I, C.c_int64, _DP, _DP]),
    "bnpp_plan_batch_mv": (_I, [_P, _I, _IP, _UBP, _I, _IP, _I, _I, _I, C.c_int64, _DP, _I, _LP, _I, _IP, _IP, _IP, _IP]),
    "bnpp_mpe_batch_mv": (_I, [_P, _P, _I, _IP, C.c_int64, _IP, _UBP, _I, _IP, _I, _I, C.c_int64, _DP, _IP, _DP]),
    "bnpp_plan_mpe_batch_mv": (_I, [_P, _I, _IP, _UBP, _I, _IP, _I, _I, C.c_int64, _DP, _I, _LP, _I, _IP, _IP]),
    "bnpp_sample_batch_mv": (_I, [_P, _P, _I, _IP, C.c_int64, _IP, _UBP, _I, _IP, _I, _I, C.c_int64, C.c_int64, C.c_int64,
                                  C.c_int64, C.c_uint64, _P, _DP, _LP, _DP]),
    "bnpp_plan_sample_batch_mv": (_I, [_P, _I, _IP, _UBP, _I, _IP, _I, _I, C.c_int64, C.c_int64, _DP, _I, _LP, _I, _IP,
                                       _IP]),
    "bnpp_expected_counts_mv": (_I, [_P, _P, _I, _IP, C.c_int64, _IP, _UBP, _DP, _I, _IP, _I, _I, C.c_int64, _DP, _DP, _LP,
                                     _DP]),
    "bnpp_plan_counts_mv": (_I, [_P, _I, _IP, _UBP, _I, _IP, _I, _I, C.c_int64, _DP, _I, _LP, _I, _IP, _IP, _IP, _I, _IP,
                                 _IP, _IP]),
    "bnpp_marginals_batch_mv": (_I, [_P, _P, _I, _IP, C.c_int64, _IP, _UBP, _I, _IP, _I, _I, _IP, _I, C.c_int64, _DP, _DP,
                                     _DP]),
    "bnpp_plan_marginals_batch_mv": (_I, [_P, _I, _IP, _UBP, _I, _IP, _I, _I, _IP, _I, C.c_int64, _DP, _I, _LP, _I, _IP,
                                          _IP, _IP]),
    "bnpp_condition_batch_mv": (_I, [_P, _P, _I, _I, _IP, _P, _I, _IP, _I, _IP, _UBP, C.c_int64, _P, _P]),
    "bnpp_evidence_load_batch_mv": (_I, [C.c_char_p, _I, C.c_int64, _IP, _IP, _LP, _IP, _UBP]),
    # soft evidence: the _sv siblings take (n_soft, soft_vars, lik) after partial; the plan entries also return
    # lam_factor[n_soft] last
    "bnpp_partition_batch_sv": (_I, [_P, _P, _I, _IP, C.c_int64, _IP, _UBP, _I, _IP, _DP, _I, _IP, _I, _I, C.c_int64, _DP,
                                     _DP, _DP]),
    "bnpp_posterior_batch_sv": (_I, [_P, _P, _I, _IP, C.c_int64, _IP, _UBP, _I, _IP, _DP, _I, _I, _I, C.c_int64, _DP, _DP]),
    "bnpp_plan_batch_sv": (_I, [_P, _I, _IP, _UBP, _I, _IP, _DP, _I, _IP, _I, _I, _I, C.c_int64, _DP, _I, _LP, _I, _IP, _IP,
                                _IP, _IP, _IP]),
    "bnpp_mpe_batch_sv": (_I, [_P, _P, _I, _IP, C.c_int64, _IP, _UBP, _I, _IP, _DP, _I, _IP, _I, _I, C.c_int64, _DP, _IP,
                               _DP]),
    "bnpp_plan_mpe_batch_sv": (_I, [_P, _I, _IP, _UBP, _I, _IP, _DP, _I, _IP, _I, _I, C.c_int64, _DP, _I, _LP, _I, _IP, _IP,
                                    _IP]),
    "bnpp_sample_batch_sv": (_I, [_P, _P, _I, _IP, C.c_int64, _IP, _UBP, _I, _IP, _DP, _I, _IP, _I, _I, C.c_int64,
                                  C.c_int64, C.c_int64, C.c_int64, C.c_uint64, _P, _DP, _LP, _DP]),
    "bnpp_plan_sample_batch_sv": (_I, [_P, _I, _IP, _UBP, _I, _IP, _DP, _I, _IP, _I, _I, C.c_int64, C.c_int64, _DP, _I, _LP,
                                       _I, _IP, _IP, _IP]),
    "bnpp_expected_counts_sv": (_I, [_P, _P, _I, _IP, C.c_int64, _IP, _UBP, _I, _IP, _DP, _DP, _I, _IP, _I, _I, C.c_int64,
                                     _DP, _DP, _LP, _DP]),
    "bnpp_plan_counts_sv": (_I, [_P, _I, _IP, _UBP, _I, _IP, _DP, _I, _IP, _I, _I, C.c_int64, _DP, _I, _LP, _I, _IP, _IP,
                                 _IP, _I, _IP, _IP, _IP, _IP]),
    "bnpp_marginals_batch_sv": (_I, [_P, _P, _I, _IP, C.c_int64, _IP, _UBP, _I, _IP, _DP, _I, _IP, _I, _I, _IP, _I,
                                     C.c_int64, _DP, _DP, _DP]),
    "bnpp_plan_marginals_batch_sv": (_I, [_P, _I, _IP, _UBP, _I, _IP, _DP, _I, _IP, _I, _I, _IP, _I, C.c_int64, _DP, _I, _LP,
                                          _I, _IP, _IP, _IP, _IP]),
    "bnpp_condition_batch_sv": (_I, [_P, _P, _I, _I, _IP, _P, _I, _IP, _I, _IP, _UBP, _I, _IP, _P, C.c_int64, _P, _P]),
    "bnpp_likelihood_load": (_I, [_P, C.c_char_p, _I, C.c_int64, _IP, _IP, _LP, _DP]),
    # device-resident batched calls: the _dv siblings take ev_vals and lik as device pointers, lik_dtype after lik,
    # and write device arrays (bnpp.tensor wraps them); then their four steps on caller-owned device buffers
    "bnpp_partition_batch_dv": (_I, [_P, _P, _I, _IP, C.c_int64, _P, _UBP, _I, _IP, _P, _I, _I, _IP, _I, _I, C.c_int64, _P,
                                     _P, _DP]),
    "bnpp_marginals_batch_dv": (_I, [_P, _P, _I, _IP, C.c_int64, _P, _UBP, _I, _IP, _P, _I, _I, _IP, _I, _I, _IP, _I,
                                     C.c_int64, _P, _P, _DP]),
    "bnpp_mpe_batch_dv": (_I, [_P, _P, _I, _IP, C.c_int64, _P, _UBP, _I, _IP, _P, _I, _I, _IP, _I, _I, C.c_int64, _P, _P,
                               _DP]),
    "bnpp_sample_batch_dv": (_I, [_P, _P, _I, _IP, C.c_int64, _P, _UBP, _I, _IP, _P, _I, _I, _IP, _I, _I, C.c_int64,
                                  C.c_int64, C.c_int64, C.c_int64, C.c_uint64, _P, _P, _P, _DP]),
    "bnpp_stage_evidence_rows": (_I, [_P, _P, _I, _IP, _UBP, C.c_int64, C.c_int64, C.c_int64, _P, _P, _P]),
    "bnpp_stage_likelihoods": (_I, [_P, _P, _I, _I, _I, _IP, C.c_int64, C.c_int64, C.c_int64, _P, _P, _P, _P]),
    "bnpp_emit_row_scalars": (_I, [_P, _P, _I, _P, _I, _P, _P, C.c_int64, C.c_int64, _P, _P]),
    "bnpp_emit_row_states": (_I, [_P, _P, _I, _I, _IP, _UBP, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _P, _P, _I, _P,
                                  _I, _P, C.c_int64, _P, _P]),
    # log-space soft evidence: lik_dtype | LIK_LOG in the _dv calls, the two steps of the log form (top after e_row;
    # n_soft, top, R after e_row and ln_z first of the outputs) and ln Z with the soft posteriors (ln_z, post)
    "bnpp_stage_loglikelihoods": (_I, [_P, _P, _I, _I, _I, _IP, C.c_int64, C.c_int64, C.c_int64, _P, _P, _P, _P, _P]),
    "bnpp_emit_row_logs": (_I, [_P, _P, _I, _P, _I, _P, _P, _I, _P, C.c_int64, C.c_int64, C.c_int64, _P, _P, _P]),
    "bnpp_log_partition_dv": (_I, [_P, _P, _I, _IP, C.c_int64, _P, _UBP, _I, _IP, _P, _I, _I, _IP, _I, _I, C.c_int64, _P,
                                   _P, _DP]),
    # device-resident model tables (bnpp.tensor.Tables): the table set, its staging step on caller-owned buffers,
    # expected counts on device arrays (tables after the model, weights and flags after lik_dtype, ln_z after
    # log10_z) and the M step
    "bnpp_model_values": (_I, [_P, _DP]),
    "bnpp_tables_create": (_I, [_P, _P, _I, C.POINTER(_P)]),
    "bnpp_tables_free": (_I, [_P]),
    "bnpp_tables_set_dv": (_I, [_P, _P, _I]),
    "bnpp_stage_tables": (_I, [_P, _P, _I, _I, _I, _LP, _P, _P, _P, _P, _P]),
    "bnpp_expected_counts_dv": (_I, [_P, _P, _P, _I, _IP, C.c_int64, _P, _UBP, _I, _IP, _P, _I, _P, _I, _I, _IP, _I, _I,
                                     C.c_int64, _P, _P, _P, _P, _DP]),
    "bnpp_mstep_dv": (_I, [_P, _P, _P, _P, C.c_double, _P, _P]),
    "bnpp_batch_job_key": (_I, [_P, _I, _IP, _UBP, _I, _IP, _I, C.c_int64, C.POINTER(C.c_uint64)]),
    "bnpp_job_create": (_I, [_P, _P, _I, _I, _IP, _IP, _I, _IP, _I, _I, _IP, _I, C.POINTER(_P)]),
    "bnpp_job_stats": (_I, [_P, _DP, _I]),
    "bnpp_job_launch": (_I, [_P, _P]),
    "bnpp_job_results": (_I, [_P, _P, _DP]),
    "bnpp_job_free": (_I, [_P]),
}
for _name, (_res, _args) in _SIGS.items():
    _f = getattr(_lib, _name)
    _f.restype = _res
    _f.argtypes = _args

EXPORTED = sorted(_SIGS)

# The signature table above is for this ABI version (include/bnpp.h
# BNPP_VERSION); a library of another version would take shifted arguments.
ABI_VERSION = 205
if _lib.bnpp_version() != ABI_VERSION:
    raise ImportError("libbnpp.so ABI version %d, this binding expects %d (%s)"
                      % (_lib.bnpp_version(), ABI_VERSION, LIB_PATH))


class BnppError(RuntimeError):
    def __init__(self, status: int, where: str):
        self.status = status
        super().__init__("%s: %s (%s)" % (where, _lib.bnpp_strerror(status).decode(), _lib.bnpp_last_error().decode()))


def _check(rc: int, where: str) -> None:
    if rc != OK:
        raise BnppError(rc, where)


def _ints(xs: Iterable[int]):
    xs = list(xs)
    return (C.c_int * max(len(xs), 1))(*xs)


def _dbls(xs: Iterable[float]):
    xs = list(xs)
    return (C.c_double * max(len(xs), 1))(*xs)


TIMING_PHASES = ("plan_ms", "upload_ms", "program_ms", "launch_ms", "run_fetch_ms", "free_ms", "total_ms",
                 "arena_reused", "arena_alloc_ms")


def last_timing() -> Dict[str, float]:
    """Phase split of this thread's last partition / marginals call (bnpp_last_timing)."""
    out = (C.c_double * len(TIMING_PHASES))()
    _check(_lib.bnpp_last_timing(out, len(TIMING_PHASES)), "bnpp_last_timing")
    return dict(zip(TIMING_PHASES, list(out)))


def device_count() -> int:
    n = C.c_int(0)
    _check(_lib.bnpp_device_count(C.byref(n)), "bnpp_device_count")
    return n.value


class Context:
    """One device context (bnpp_ctx_create).  Fails with NO_DEVICE without a GPU."""

    def __init__(self, device: int = 0):
        self._h = _P()
        _check(_lib.bnpp_ctx_create(device, C.byref(self._h)), "bnpp_ctx_create")
        self.device = device

    @property
    def handle(self):
        return self._h

    def trim(self) -> None:
        """Release the device memory kept between calls (cached arena, buffers)."""
        _check(_lib.bnpp_ctx_trim(self.handle), "bnpp_ctx_trim")

    def set_max_grid(self, n: int) -> None:
        """Testing: at most n workgroups per persistent launch from now on (0: the
        default grids), so that tile loops iterate on small inputs (bnpp_ctx_set_max_grid)."""
        _check(_lib.bnpp_ctx_set_max_grid(self.handle, n), "bnpp_ctx_set_max_grid")

    def stream(self) -> int:
        s = _P()
        _check(_lib.bnpp_ctx_stream(self._h, C.byref(s)), "bnpp_ctx_stream")
        return s.value or 0

    def synchronize(self, stream: Optional[int] = None) -> None:
        _check(_lib.bnpp_synchronize(self._h, _P(stream) if stream else None), "bnpp_synchronize")

    def close(self) -> None:
        if self._h:
            _lib.bnpp_ctx_destroy(self._h)
            self._h = _P()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Model:
    """A UAI model held by the engine (host memory)."""

    def __init__(self, handle):
        self._h = handle
        ib, nv, nf = C.c_int(), C.c_int(), C.c_int()
        _check(_lib.bnpp_model_info(self._h, C.byref(ib), C.byref(nv), C.byref(nf)), "bnpp_model_info")
        self.is_bayes, self.n_vars, self.n_factors = bool(ib.value), nv.value, nf.value
        cards = (C.c_int * max(nv.value, 1))()
        _check(_lib.bnpp_model_cards(self._h, cards), "bnpp_model_cards")
        self.cards = list(cards[: nv.value])

    @classmethod
    def load(cls, path: str) -> "Model":
        h = _P()
        _check(_lib.bnpp_model_load_uai(path.encode(), C.byref(h)), "bnpp_model_load_uai")
        return cls(h)

    @classmethod
    def from_dict(cls, m: dict) -> "Model":
        widths = [len(s) for s in m["scopes"]]
        scopes = [v for s in m["scopes"] for v in s]
        values = [x for vals in m["values"] for x in vals]
        h = _P()
        _check(_lib.bnpp_model_from_arrays(1 if m.get("type") == "BAYES" else 0, len(m["cards"]), _ints(m["cards"]),
                                           len(widths), _ints(widths), _ints(scopes), _dbls(values), C.byref(h)),
               "bnpp_model_from_arrays")
        return cls(h)

    @classmethod
    def from_arrays(cls, cards: Sequence[int], scopes: Sequence[Sequence[int]], values, is_bayes: bool = False
                    ) -> "Model":
        """A model from one flat float64 array of every factor's table in
        order (numpy, C-contiguous, passed by pointer: no per-entry Python
        objects, so tables of billions of entries load in seconds)."""
        import numpy as np
        vals = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        widths = [len(s) for s in scopes]
        flat = [v for s in scopes for v in s]
        h = _P()
        _check(_lib.bnpp_model_from_arrays(1 if is_bayes else 0, len(cards), _ints(cards), len(widths), _ints(widths),
                                           _ints(flat), vals.ctypes.data_as(_DP), C.byref(h)),
               "bnpp_model_from_arrays")
        return cls(h)

    @property
    def handle(self):
        return self._h

    def __del__(self):
        try:
            if self._h:
                _lib.bnpp_model_free(self._h)
                self._h = _P()
        except Exception:
            pass


def _ev(evidence: Optional[Dict[int, int]]):
    evidence = evidence or {}
    ks = sorted(evidence)
    return len(ks), _ints(ks), _ints([evidence[k] for k in ks])


def load_evidence(path: str) -> Dict[int, int]:
    cap = 1 << 16
    n = C.c_int()
    vs, xs = (C.c_int * cap)(), (C.c_int * cap)()
    _check(_lib.bnpp_evidence_load(path.encode(), cap, C.byref(n), vs, xs), "bnpp_evidence_load")
    return {vs[i]: xs[i] for i in range(n.value)}


def ordering(model: Model, evidence=None, heuristic: str = "mf", variables: Optional[Sequence[int]] = None):
    n, ev_v, ev_x = _ev(evidence)
    out = (C.c_int * max(model.n_vars, 1))()
    w = C.c_int()
    if variables is None:
        _check(_lib.bnpp_ordering(model.handle, n, ev_v, ev_x, 0, None, HEURISTICS[heuristic], out, C.byref(w)),
               "bnpp_ordering")
        cnt = model.n_vars - len(evidence or {})
    else:
        variables = list(variables)
        _check(_lib.bnpp_ordering(model.handle, n, ev_v, ev_x, len(variables), _ints(variables), HEURISTICS[heuristic],
                                  out, C.byref(w)), "bnpp_ordering")
        cnt = len(variables)
    return list(out[:cnt]), w.value


def out_scope(scopes: Sequence[Sequence[int]], elim: int = -1) -> List[int]:
    arrs = [_ints(s) for s in scopes]
    ptrs = (_IP * max(len(arrs), 1))(*[C.cast(a, _IP) for a in arrs])
    nd = _ints([len(s) for s in scopes])
    cap = sum(len(s) for s in scopes) + 1
    out = (C.c_int * cap)()
    n = C.c_int()
    _check(_lib.bnpp_out_scope(len(scopes), nd, ptrs, elim, cap, C.byref(n), out), "bnpp_out_scope")
    return list(out[: n.value])


def plan_stats(model: Model, kind: int = 0, evidence=None, heuristic: str = "mf", dtype: int = F64,
               order: Optional[Sequence[int]] = None) -> List[float]:
    n, ev_v, ev_x = _ev(evidence)
    st = (C.c_double * 8)()
    oa = _ints(order) if order is not None else None
    h = ORDER_GIVEN if order is not None else HEURISTICS[heuristic]
    _check(_lib.bnpp_plan_stats(model.handle, kind, n, ev_v, ev_x, h, oa, len(order) if order is not None else 0,
                                dtype, st, 8), "bnpp_plan_stats")
    return list(st)


PLAN_SINGLE_FIELDS = ("family", "key", "n_in", "k", "v1", "v2", "bcls", "o32", "n_tiles", "lanes", "slab_y2",
                      "instantiated")
FAMILIES = ("generic", "stream", "slab", "chain", "max")


def plan_single(dtype: int, cards: Sequence[int], scopes: Sequence[Sequence[int]], elim: int,
                out_vars: Sequence[int], divide: bool = False, evidence: Optional[Dict[int, int]] = None
                ) -> Dict[str, int]:
    """Planning introspection for tests (bnpp_plan_single, host only): the
    kernel bucket_eliminate / divide / condition would launch for these
    arguments, as a dict of PLAN_SINGLE_FIELDS."""
    arrs = [_ints(s) for s in scopes]
    ptrs = (_IP * max(len(arrs), 1))(*[C.cast(a, _IP) for a in arrs])
    n, ev_v, ev_x = _ev(evidence)
    info = (C.c_int64 * len(PLAN_SINGLE_FIELDS))()
    _check(_lib.bnpp_plan_single(dtype, len(cards), _ints(cards), len(scopes), _ints([len(s) for s in scopes]), ptrs,
                                 elim, len(out_vars), _ints(out_vars), 1 if divide else 0, n, ev_v, ev_x, info,
                                 len(PLAN_SINGLE_FIELDS)), "bnpp_plan_single")
    return dict(zip(PLAN_SINGLE_FIELDS, list(info)))


def plan_max_single(dtype: int, cards: Sequence[int], scopes: Sequence[Sequence[int]], elim: int,
                    out_vars: Sequence[int]) -> Dict[str, int]:
    """Planning introspection for tests (bnpp_plan_max_single, host only): the
    max-family kernel bucket_max would launch, as a dict of PLAN_SINGLE_FIELDS."""
    arrs = [_ints(s) for s in scopes]
    ptrs = (_IP * max(len(arrs), 1))(*[C.cast(a, _IP) for a in arrs])
    info = (C.c_int64 * len(PLAN_SINGLE_FIELDS))()
    _check(_lib.bnpp_plan_max_single(dtype, len(cards), _ints(cards), len(scopes), _ints([len(s) for s in scopes]),
                                     ptrs, elim, len(out_vars), _ints(out_vars), info, len(PLAN_SINGLE_FIELDS)),
           "bnpp_plan_max_single")
    return dict(zip(PLAN_SINGLE_FIELDS, list(info)))


def kernel_keys(dtype: int, family: int, level: bool = False) -> List[int]:
    """The dispatch keys instantiated for `dtype` in a family (index into
    FAMILIES), for single-op or level launches (bnpp_kernel_keys)."""
    n = C.c_int()
    _check(_lib.bnpp_kernel_keys(dtype, 1 if level else 0, family, None, 0, C.byref(n)), "bnpp_kernel_keys")
    out = (C.c_int * max(n.value, 1))()
    _check(_lib.bnpp_kernel_keys(dtype, 1 if level else 0, family, out, n.value, C.byref(n)), "bnpp_kernel_keys")
    return list(out[: n.value])


def chain_key_supported(dtype: int, key: int) -> bool:
    """The planner's chain_supported predicate for a dispatch key (bnpp_chain_key_supported)."""
    out = C.c_int()
    _check(_lib.bnpp_chain_key_supported(dtype, key, C.byref(out)), "bnpp_chain_key_supported")
    return bool(out.value)


PLAN_GROUP_FIELDS = ("batch", "level", "key", "n_desc", "vblocks", "lane")


def plan_groups(model: Model, kind: int = 0, evidence=None, heuristic: str = "mf", dtype: int = F64,
                order: Optional[Sequence[int]] = None, part: int = 0, n_parts: int = 1) -> List[Dict[str, int]]:
    """Planning introspection for tests (bnpp_plan_groups, host only): the launch
    groups of the plan plan_stats reports on, one dict of PLAN_GROUP_FIELDS
    each.  n_desc tells which kernel a split chain key runs: 1 its one-run
    kernel, more its multi-run kernel."""
    n, ev_v, ev_x = _ev(evidence)
    oa = _ints(order) if order is not None else None
    h = ORDER_GIVEN if order is not None else HEURISTICS[heuristic]
    no = len(order) if order is not None else 0
    nf = len(PLAN_GROUP_FIELDS)
    cnt = C.c_int()
    _check(_lib.bnpp_plan_groups(model.handle, kind, n, ev_v, ev_x, h, oa, no, dtype, part, n_parts, None, 0,
                                 C.byref(cnt)), "bnpp_plan_groups")
    rows = (C.c_int64 * max(cnt.value * nf, 1))()
    _check(_lib.bnpp_plan_groups(model.handle, kind, n, ev_v, ev_x, h, oa, no, dtype, part, n_parts, rows, cnt.value,
                                 C.byref(cnt)), "bnpp_plan_groups")
    return [dict(zip(PLAN_GROUP_FIELDS, rows[i * nf:(i + 1) * nf])) for i in range(cnt.value)]


def plan_mpe_groups(model: Model, evidence=None, heuristic: str = "mf", dtype: int = F64,
                    order: Optional[Sequence[int]] = None) -> List[Dict[str, int]]:
    """The launch groups of the plan mpe() runs (bnpp_plan_mpe_groups, host
    only), one dict of PLAN_GROUP_FIELDS each; plan_groups takes the sum plans only."""
    n, ev_v, ev_x = _ev(evidence)
    oa = _ints(order) if order is not None else None
    h = ORDER_GIVEN if order is not None else HEURISTICS[heuristic]
    no = len(order) if order is not None else 0
    nf = len(PLAN_GROUP_FIELDS)
    cnt = C.c_int()
    _check(_lib.bnpp_plan_mpe_groups(model.handle, n, ev_v, ev_x, h, oa, no, dtype, None, 0, C.byref(cnt)),
           "bnpp_plan_mpe_groups")
    rows = (C.c_int64 * max(cnt.value * nf, 1))()
    _check(_lib.bnpp_plan_mpe_groups(model.handle, n, ev_v, ev_x, h, oa, no, dtype, rows, cnt.value, C.byref(cnt)),
           "bnpp_plan_mpe_groups")
    return [dict(zip(PLAN_GROUP_FIELDS, rows[i * nf:(i + 1) * nf])) for i in range(cnt.value)]


def partition(ctx: Context, model: Model, evidence=None, heuristic: str = "mf", dtype: int = F64,
              order: Optional[Sequence[int]] = None):
    """BN::partition (model.cpp:250-301) -> (log10 Z, Z, uptime_ms)."""
    n, ev_v, ev_x = _ev(evidence)
    lz, z, up = C.c_double(), C.c_double(), C.c_double()
    if order is not None:
        order = list(order)
        _check(_lib.bnpp_partition(ctx.handle, model.handle, n, ev_v, ev_x, ORDER_GIVEN, _ints(order), len(order), dtype,
                                   C.byref(lz), C.byref(z), C.byref(up)), "bnpp_partition")
    else:
        _check(_lib.bnpp_partition(ctx.handle, model.handle, n, ev_v, ev_x, HEURISTICS[heuristic], None, 0, dtype,
                                   C.byref(lz), C.byref(z), C.byref(up)), "bnpp_partition")
    return lz.value, z.value, up.value


def mpe(ctx: Context, model: Model, evidence=None, heuristic: str = "mf", dtype: int = F64,
        order: Optional[Sequence[int]] = None):
    """Most probable explanation (bnpp_mpe; no reference counterpart) ->
    (log10 of the maximum, [x_0 .. x_{n-1}] with evidence values kept, uptime_ms).
    Ties resolve to the lowest value of each variable as it is maximised."""
    n, ev_v, ev_x = _ev(evidence)
    lv, up = C.c_double(), C.c_double()
    x = (C.c_int * max(model.n_vars, 1))()
    oa = _ints(order) if order is not None else None
    h = ORDER_GIVEN if order is not None else HEURISTICS[heuristic]
    _check(_lib.bnpp_mpe(ctx.handle, model.handle, n, ev_v, ev_x, h, oa, len(order) if order is not None else 0, dtype,
                         C.byref(lv), x, C.byref(up)), "bnpp_mpe")
    return lv.value, list(x[: model.n_vars]), up.value


SAMPLE_KEY = (1 << 24) + 8192      # the launch-group key of the sampling step (plan.hpp kSampleKey)
PLAN_SAMPLE_STATS = ("entries", "arena_bytes", "levels", "buckets", "width", "max_table", "bytes_moved", "batches",
                     "sample_rows", "sample_bytes")


def plan_sample(model: Model, n: int, evidence=None, heuristic: str = "mf", dtype: int = F64,
                order: Optional[Sequence[int]] = None):
    """Host-only planning of sample() (bnpp_plan_sample) -> (stats, groups):
    stats a dict of PLAN_SAMPLE_STATS, groups one dict of PLAN_GROUP_FIELDS per
    launch group; the sampling step is the last group, key SAMPLE_KEY."""
    ne, ev_v, ev_x = _ev(evidence)
    oa = _ints(order) if order is not None else None
    h = ORDER_GIVEN if order is not None else HEURISTICS[heuristic]
    no = len(order) if order is not None else 0
    nf = len(PLAN_GROUP_FIELDS)
    st = (C.c_double * len(PLAN_SAMPLE_STATS))()
    cnt = C.c_int()
    _check(_lib.bnpp_plan_sample(model.handle, ne, ev_v, ev_x, h, oa, no, dtype, n, st, len(PLAN_SAMPLE_STATS), None, 0,
                                 C.byref(cnt)), "bnpp_plan_sample")
    rows = (C.c_int64 * max(cnt.value * nf, 1))()
    _check(_lib.bnpp_plan_sample(model.handle, ne, ev_v, ev_x, h, oa, no, dtype, n, st, len(PLAN_SAMPLE_STATS), rows,
                                 cnt.value, C.byref(cnt)), "bnpp_plan_sample")
    return (dict(zip(PLAN_SAMPLE_STATS, list(st))),
            [dict(zip(PLAN_GROUP_FIELDS, rows[i * nf:(i + 1) * nf])) for i in range(cnt.value)])


def sample(ctx: Context, model: Model, n: int, evidence=None, seed: int = 0, first_sample: int = 0,
           heuristic: str = "mf", dtype: int = F64, order: Optional[Sequence[int]] = None):
    """n exact joint samples of P(x | evidence) (bnpp_sample; no reference
    counterpart) -> (samples, log10 Z, n_degenerate).  samples: a numpy uint8
    view of shape (n, n_vars), the transpose of the fetched variable-major
    buffer; evidence variables keep their value.  Sample s has the global index
    first_sample + s and depends on (seed, that index) only."""
    import numpy as np
    ne, ev_v, ev_x = _ev(evidence)
    oa = _ints(order) if order is not None else None
    h = ORDER_GIVEN if order is not None else HEURISTICS[heuristic]
    buf = np.zeros((max(model.n_vars, 1), max(int(n), 1)), dtype=np.uint8)
    lz, up = C.c_double(), C.c_double()
    deg = C.c_int64()
    _check(_lib.bnpp_sample(ctx.handle, model.handle, ne, ev_v, ev_x, h, oa, len(order) if order is not None else 0,
                            dtype, int(n), int(first_sample), int(seed) & 0xFFFFFFFFFFFFFFFF, _P(buf.ctypes.data),
                            C.byref(lz), C.byref(deg), C.byref(up)), "bnpp_sample")
    return buf[: model.n_vars].T, lz.value, deg.value


COND_BATCH_KEY = (1 << 24) + 12288   # the launch-group key of a gather step (plan.hpp kCondBatchKey)
PLAN_BATCH_STATS = ("entries", "arena_bytes", "levels", "buckets", "width", "max_table", "bytes_moved", "batches",
                    "rows_per_launch", "gather_steps")


def _ev_rows(ev_vars: Sequence[int], rows):
    """(n_ev, ev_vars as c ints, n_rows, the rows as a C-contiguous int32 array, its pointer)."""
    import numpy as np
    ev_vars = [int(v) for v in ev_vars]
    a = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1, len(ev_vars)) if len(ev_vars)
                             else np.zeros((len(rows), 0), dtype=np.int64))
    if a.size and (a.max() > 2 ** 31 - 1 or a.min() < -2 ** 31):
        raise ValueError("evidence values must fit an int32")
    a32 = np.ascontiguousarray(a.astype(np.intc))
    return len(ev_vars), _ints(ev_vars), a32.shape[0], a32, a32.ctypes.data_as(_IP)


MISSING = -1                         # a missing value of a partial evidence variable (include/bnpp.h BNPP_MISSING)
COND_BATCH_MASK_KEY = (1 << 24) + 32768   # the launch-group key of a masked gather step (plan.hpp kCondBatchMaskKey)


def _partial_flags(ev_vars: Sequence[int], partial, rows=None):
    """partial as the _mv entries take it: None (the call without the argument),
    else one unsigned byte per evidence variable.  partial: None, "auto" (the
    columns of `rows` that hold a MISSING) or a sequence of variable ids."""
    if partial is None:
        return None
    ev_vars = [int(v) for v in ev_vars]
    flags = (C.c_ubyte * max(len(ev_vars), 1))()
    if isinstance(partial, str):
        if partial != "auto":
            raise ValueError('partial must be None, "auto" or a sequence of variable ids')
        if rows is None:
            raise ValueError('partial="auto" needs the rows')
        for j in range(len(ev_vars)):
            flags[j] = 1 if rows.shape[0] and bool((rows[:, j] == MISSING).any()) else 0
        return flags
    ids = [int(v) for v in partial]
    for v in ids:
        if v not in ev_vars:
            raise ValueError("partial variable %d is not an evidence variable" % v)
    for j, v in enumerate(ev_vars):
        flags[j] = 1 if v in ids else 0
    return flags


def _mv(name: str, pf):
    """(the entry point, its name, the partial argument as a tuple to splice in)."""
    if pf is None:
        return getattr(_lib, name), name, ()
    return getattr(_lib, name + "_mv"), name + "_mv", (pf,)


COND_BATCH_SOFT_KEY = (1 << 24) + 36864   # the launch-group key of a weighted gather step (plan.hpp kCondBatchSoftKey)


def _soft_vars(soft):
    """The soft variable ids of a `soft` argument: (soft_vars, lik), or for a plan function the ids alone."""
    if isinstance(soft, (tuple, list)) and len(soft) == 2 and hasattr(soft[0], "__len__"):   # (ids, lik), as the run calls
        soft = soft[0]
    return [int(v) for v in soft]


def _soft_args(model: "Model", soft, n_rows: int):
    """soft = (soft_vars, lik) as the _sv run entries take it -> (n_soft, the ids as c ints, the (n, Ws) float64
    array (keep it alive), its pointer).  lik: an (n, Ws) array, Ws the sum of the soft cards with the variables'
    blocks in the listed order (what marginals_batch returns), or a list of one (n, card) array per variable."""
    import numpy as np
    if not (isinstance(soft, (tuple, list)) and len(soft) == 2):
        raise ValueError("soft must be (soft_vars, lik)")
    ids = [int(v) for v in soft[0]]
    lik = soft[1]
    cards = [model.cards[v] if 0 <= v < model.n_vars else None for v in ids]
    if isinstance(lik, (list, tuple)) and len(lik) == len(ids) and all(getattr(a, "ndim", 0) == 2 for a in lik):
        for v, k, a in zip(ids, cards, lik):
            if k is not None and a.shape != (n_rows, k):
                raise ValueError("the likelihoods of soft variable %d must have shape (%d, %d), not %s"
                                 % (v, n_rows, k, tuple(a.shape)))
        lik = np.concatenate([np.asarray(a, dtype=np.float64) for a in lik], axis=1) if ids else np.zeros((n_rows, 0))
    a = np.ascontiguousarray(lik, dtype=np.float64)
    if None not in cards:
        ws = sum(cards)
        if a.ndim != 2 or a.shape != (n_rows, ws):
            raise ValueError("lik must have shape (%d, %d): one row per evidence row, the sum of the soft cards wide; "
                             "got %s" % (n_rows, ws, tuple(a.shape)))
    elif a.ndim != 2 or a.shape[0] != n_rows:      # a bad id: the library names it
        raise ValueError("lik must have one row per evidence row")
    return len(ids), _ints(ids) if ids else (C.c_int * 1)(), a, a.ctypes.data_as(_DP)


def _sv(name: str, pf, soft, model=None, n_rows=None):
    """_mv, or with `soft` the _sv entry point -> (fn, name, the arguments to splice in after the evidence, what
    to keep alive).  n_rows None: a plan entry (ids only, no likelihoods)."""
    if soft is None:
        return _mv(name, pf) + (None,)
    if n_rows is None:
        ids = _soft_vars(soft)
        return getattr(_lib, name + "_sv"), name + "_sv", (pf, len(ids), _ints(ids) if ids else (C.c_int * 1)(), None), None
    ns, sv, keep, lp = _soft_args(model, soft, n_rows)
    return getattr(_lib, name + "_sv"), name + "_sv", (pf, ns, sv, lp), keep


def _plan_tail(pf, n_ev, soft, tail=lambda: ()):
    """_mask_tail, and with `soft` also lam_factor -> (tail, what to append to the plan function's result)."""
    if soft is None:
        t, mask = _mask_tail(pf, n_ev, tail)
        return t, (lambda: (mask(),) if pf is not None else ())
    n_soft = len(_soft_vars(soft))
    mf, lf = (C.c_int * max(n_ev, 1))(), (C.c_int * max(n_soft, 1))()
    return ((lambda: (*tail(), mf, lf)),
            (lambda: (([mf[j] for j in range(n_ev)],) if pf is not None else ()) + ([lf[j] for j in range(n_soft)],)))


def _mask_tail(pf, n_ev, tail=lambda: ()):
    """The tail of a plan entry with mask_factor appended for the _mv entries; the list that reads it back."""
    mf = (C.c_int * max(n_ev, 1))()
    if pf is None:
        return tail, lambda: None
    return (lambda: (*tail(), mf)), (lambda: [mf[j] for j in range(n_ev)])


def _h(ctx):
    return ctx.handle if ctx is not None else None


def _order_args(order, heuristic):
    """(heuristic, order, n_order) as the C ABI takes them: an explicit order wins over the heuristic's name."""
    if order is None:
        return HEURISTICS[heuristic], None, 0
    return ORDER_GIVEN, _ints(order), len(order)


def _plan_call(fn, name, stat_names, head, tail=lambda: ()):
    """A batched plan entry point called twice, for the number of launch groups
    and then for the groups -> (stats dict, one dict of PLAN_GROUP_FIELDS per
    group).  head: the arguments before the stats; tail(): those after n_rows,
    asked for before either call."""
    nf = len(PLAN_GROUP_FIELDS)
    st = (C.c_double * len(stat_names))()
    cnt = C.c_int()
    _check(fn(*head, st, len(stat_names), None, 0, C.byref(cnt), *tail()), name)
    rows = (C.c_int64 * max(cnt.value * nf, 1))()
    _check(fn(*head, st, len(stat_names), rows, cnt.value, C.byref(cnt), *tail()), name)
    return (dict(zip(stat_names, list(st))),
            [dict(zip(PLAN_GROUP_FIELDS, rows[i * nf:(i + 1) * nf])) for i in range(cnt.value)])


def load_evidence_batch(path: str, missing: bool = False):
    """An .evid file of any number of samples over one variable set
    (bnpp_evidence_load_batch) -> (ev_vars ascending, rows as an (n, n_ev) numpy int array).
    missing=True (bnpp_evidence_load_batch_mv): the samples may observe differing
    variable sets -> (the union ascending, rows with MISSING where a sample is
    silent, the variables some sample lacks: what to pass as `partial`)."""
    import numpy as np
    n_ev, n_rows = C.c_int(), C.c_int64()
    if missing:
        fn, name = _lib.bnpp_evidence_load_batch_mv, "bnpp_evidence_load_batch_mv"
        rc = fn(path.encode(), 0, 0, C.byref(n_ev), None, C.byref(n_rows), None, None)
        if rc != OK and not (rc == ERR_INVALID and (n_ev.value > 0 or n_rows.value > 0)):
            raise BnppError(rc, name)
        vs = (C.c_int * max(n_ev.value, 1))()
        pf = (C.c_ubyte * max(n_ev.value, 1))()
        rows = np.zeros((n_rows.value, n_ev.value), dtype=np.intc)
        _check(fn(path.encode(), n_ev.value, n_rows.value, C.byref(n_ev), vs, C.byref(n_rows), rows.ctypes.data_as(_IP), pf),
               name)
        return [vs[i] for i in range(n_ev.value)], rows, [vs[i] for i in range(n_ev.value) if pf[i]]
    rc = _lib.bnpp_evidence_load_batch(path.encode(), 0, 0, C.byref(n_ev), None, C.byref(n_rows), None)
    if rc != OK and not (rc == ERR_INVALID and (n_ev.value > 0 or n_rows.value > 0)):
        raise BnppError(rc, "bnpp_evidence_load_batch")
    vs = (C.c_int * max(n_ev.value, 1))()
    rows = np.zeros((n_rows.value, n_ev.value), dtype=np.intc)
    _check(_lib.bnpp_evidence_load_batch(path.encode(), n_ev.value, n_rows.value, C.byref(n_ev), vs, C.byref(n_rows),
                                         rows.ctypes.data_as(_IP)), "bnpp_evidence_load_batch")
    return [vs[i] for i in range(n_ev.value)], rows


def load_likelihoods(model: Model, path: str):
    """A likelihood file (bnpp_likelihood_load; synth.write_likelihoods writes one): n_soft, the ids, n_rows, then
    per row the Ws likelihoods -> (soft_vars, lik as an (n_rows, Ws) float64 array): what to pass as `soft`."""
    import numpy as np
    ns, nr = C.c_int(), C.c_int64()
    rc = _lib.bnpp_likelihood_load(model.handle, path.encode(), 0, 0, C.byref(ns), None, C.byref(nr), None)
    if rc != OK and not (rc == ERR_INVALID and (ns.value > 0 or nr.value > 0)):
        raise BnppError(rc, "bnpp_likelihood_load")
    vs = (C.c_int * max(ns.value, 1))()
    _lib.bnpp_likelihood_load(model.handle, path.encode(), ns.value, 0, C.byref(ns), vs, C.byref(nr), None)
    ids = [vs[i] for i in range(ns.value)]
    ws = sum(model.cards[v] for v in ids)
    lik = np.zeros((nr.value, ws))
    _check(_lib.bnpp_likelihood_load(model.handle, path.encode(), ns.value, nr.value * ws, C.byref(ns), vs, C.byref(nr),
                                     lik.ctypes.data_as(_DP)), "bnpp_likelihood_load")
    return ids, lik


def batch_job_key(model: Model, ev_vars: Sequence[int], partial=None, soft=None, dtype: int = F64,
                  rows_per_launch: int = 0) -> int:
    """The job cache key of a partition_batch call of this shape (bnpp_batch_job_key): it depends on the variable
    lists, never on values, and a call without `soft` keeps the key it had before soft evidence existed."""
    ev_vars = [int(v) for v in ev_vars]
    ids = _soft_vars(soft) if soft is not None else []
    key = C.c_uint64()
    _check(_lib.bnpp_batch_job_key(model.handle, len(ev_vars), _ints(ev_vars) if ev_vars else None,
                                   _partial_flags(ev_vars, partial), len(ids), _ints(ids) if ids else None, dtype,
                                   int(rows_per_launch), C.byref(key)), "bnpp_batch_job_key")
    return key.value


def plan_batch(model: Model, ev_vars: Sequence[int], target: Optional[int] = None, heuristic: str = "mf",
               dtype: int = F64, rows_per_launch: int = 0, order: Optional[Sequence[int]] = None, partial=None,
               soft=None):
    """partial (here and in every batched call and plan function): None, or the
    evidence variables that may be MISSING in a row -- a sequence of ids, or
    "auto" in the run calls for the columns that hold a MISSING (include/bnpp.h,
    missing values).  A plan function given `partial` also returns mask_factor
    (per evidence variable the factor that carries its mask, -1: none) last.

    Host-only planning of partition_batch (target None) or posterior_batch
    (bnpp_plan_batch) -> (stats, groups, result_scope): stats a dict of
    PLAN_BATCH_STATS, groups one dict of PLAN_GROUP_FIELDS per launch group (the
    gather steps: level 0, key COND_BATCH_KEY), result_scope the result
    table's variables with the row variable B reported as model.n_vars."""
    ev_vars = [int(v) for v in ev_vars]
    nrs = C.c_int()
    rs = (C.c_int * 2)()
    t = -1 if target is None else int(target)
    fn, name, pa, _ = _sv("bnpp_plan_batch", _partial_flags(ev_vars, partial), soft)
    tail, extra = _plan_tail(pa[0] if pa else None, len(ev_vars), soft, lambda: (rs, C.byref(nrs)))
    st, groups = _plan_call(fn, name, PLAN_BATCH_STATS,
                            (model.handle, len(ev_vars), _ints(ev_vars), *pa, *_order_args(order, heuristic), t, dtype,
                             int(rows_per_launch)), tail)
    res = st, groups, [rs[i] for i in range(min(nrs.value, 2))]
    return res + extra()


def partition_batch(ctx: Context, model: Model, ev_vars: Sequence[int], rows, heuristic: str = "mf", dtype: int = F64,
                    rows_per_launch: int = 0, order: Optional[Sequence[int]] = None, partial=None,
                    soft=None):
    """log10 Z and Z of every evidence row from one plan (bnpp_partition_batch)
    -> (log10_z, z, uptime_ms), numpy float64 arrays of length n.  rows: an
    (n, len(ev_vars)) integer array, rows[r][j] the value of ev_vars[j]."""
    import numpy as np
    ne, ev_v, n, keep, ev_x = _ev_rows(ev_vars, rows)
    h, oa, no = _order_args(order, heuristic)
    lz, z = np.zeros(max(n, 1)), np.zeros(max(n, 1))
    up = C.c_double()
    fn, name, pa, keep_lik = _sv("bnpp_partition_batch", _partial_flags(ev_vars, partial, keep), soft, model, n)
    _check(fn(_h(ctx), model.handle, ne, ev_v, n, ev_x, *pa, h, oa, no, dtype, int(rows_per_launch),
              lz.ctypes.data_as(_DP), z.ctypes.data_as(_DP), C.byref(up)), name)
    del keep, keep_lik
    return lz[:n], z[:n], up.value


def posterior_batch(ctx: Context, model: Model, ev_vars: Sequence[int], rows, target: int, heuristic: str = "mf",
                    dtype: int = F64, rows_per_launch: int = 0, partial=None, soft=None):
    """P(target | evidence row) for every row from one plan (bnpp_posterior_batch)
    -> (an (n, card(target)) numpy float64 array, uptime_ms)."""
    import numpy as np
    ne, ev_v, n, keep, ev_x = _ev_rows(ev_vars, rows)
    t = int(target)
    k = model.cards[t] if 0 <= t < model.n_vars else 1
    out = np.zeros((max(n, 1), max(k, 1)))
    up = C.c_double()
    fn, name, pa, keep_lik = _sv("bnpp_posterior_batch", _partial_flags(ev_vars, partial, keep), soft, model, n)
    _check(fn(_h(ctx), model.handle, ne, ev_v, n, ev_x, *pa, HEURISTICS[heuristic], t, dtype,
              int(rows_per_launch), out.ctypes.data_as(_DP), C.byref(up)), name)
    del keep, keep_lik
    return out[:n, :k], up.value


MPE_DECODE_BATCH_KEY = (1 << 24) + 20480   # the launch-group key of the batched traceback (plan.hpp kMpeDecodeBatchKey)
PLAN_MPE_BATCH_STATS = PLAN_BATCH_STATS + ("arg_bytes", "max_buckets", "arg_tables_b", "arg_tables_no_b",
                                           "arg_entries_per_row", "arg_entries_no_b")


def plan_mpe_batch(model: Model, ev_vars: Sequence[int], heuristic: str = "mf", dtype: int = F64,
                   rows_per_launch: int = 0, order: Optional[Sequence[int]] = None, partial=None,
                   soft=None):
    """Host-only planning of mpe_batch (bnpp_plan_mpe_batch) -> (stats, groups):
    stats a dict of PLAN_MPE_BATCH_STATS (arg_bytes = arg_entries_per_row *
    rows_per_launch + arg_entries_no_b), groups one dict of PLAN_GROUP_FIELDS per
    launch group: the gather steps (level 0, COND_BATCH_KEY), max and product
    buckets, and the traceback step last (MPE_DECODE_BATCH_KEY)."""
    ev_vars = [int(v) for v in ev_vars]
    fn, name, pa, _ = _sv("bnpp_plan_mpe_batch", _partial_flags(ev_vars, partial), soft)
    tail, extra = _plan_tail(pa[0] if pa else None, len(ev_vars), soft)
    res = _plan_call(fn, name, PLAN_MPE_BATCH_STATS,
                     (model.handle, len(ev_vars), _ints(ev_vars), *pa, *_order_args(order, heuristic), dtype,
                      int(rows_per_launch)), tail)
    return res + extra()


def mpe_batch(ctx: Context, model: Model, ev_vars: Sequence[int], rows, heuristic: str = "mf", dtype: int = F64,
              order: Optional[Sequence[int]] = None, rows_per_launch: int = 0, partial=None, soft=None):
    """The most probable completion of every evidence row from one plan
    (bnpp_mpe_batch) -> (log10_value float64[n], assignment int32 (n, n_vars),
    uptime_ms).  rows: an (n, len(ev_vars)) integer array, rows[r][j] the value
    of ev_vars[j]; row r's answer is mpe()'s for that evidence."""
    import numpy as np
    ne, ev_v, n, keep, ev_x = _ev_rows(ev_vars, rows)
    h, oa, no = _order_args(order, heuristic)
    lv = np.zeros(max(n, 1))
    x = np.zeros((max(n, 1), max(model.n_vars, 1)), dtype=np.intc)
    up = C.c_double()
    fn, name, pa, keep_lik = _sv("bnpp_mpe_batch", _partial_flags(ev_vars, partial, keep), soft, model, n)
    _check(fn(_h(ctx), model.handle, ne, ev_v, n, ev_x, *pa, h, oa, no, dtype, int(rows_per_launch),
              lv.ctypes.data_as(_DP), x.ctypes.data_as(_IP), C.byref(up)), name)
    del keep, keep_lik
    return lv[:n], x[:n, :model.n_vars].astype(np.int32, copy=False), up.value


SAMPLE_BATCH_KEY = (1 << 24) + 24576   # the launch-group key of the batched draw step (plan.hpp kSampleBatchKey)
PLAN_SAMPLE_BATCH_STATS = PLAN_BATCH_STATS + ("n_per_row", "state_bytes", "draw_rows", "draw_rows_b", "draw_rows_no_b")


def plan_sample_batch(model: Model, ev_vars: Sequence[int], n_per_row: int = 1, heuristic: str = "mf", dtype: int = F64,
                      rows_per_launch: int = 0, order: Optional[Sequence[int]] = None, partial=None,
                      soft=None):
    """Host-only planning of sample_batch (bnpp_plan_sample_batch) -> (stats,
    groups): stats a dict of PLAN_SAMPLE_BATCH_STATS (state_bytes = n_vars *
    rows_per_launch * n_per_row; draw_rows = draw_rows_b + draw_rows_no_b, with
    and without an input that carries the row variable), groups one dict of
    PLAN_GROUP_FIELDS per launch group: the gather steps (level 0,
    COND_BATCH_KEY), sum and product buckets, and the draw step last
    (SAMPLE_BATCH_KEY)."""
    ev_vars = [int(v) for v in ev_vars]
    fn, name, pa, _ = _sv("bnpp_plan_sample_batch", _partial_flags(ev_vars, partial), soft)
    tail, extra = _plan_tail(pa[0] if pa else None, len(ev_vars), soft)
    res = _plan_call(fn, name, PLAN_SAMPLE_BATCH_STATS,
                     (model.handle, len(ev_vars), _ints(ev_vars), *pa, *_order_args(order, heuristic), dtype,
                      int(rows_per_launch), int(n_per_row)), tail)
    return res + extra()


def sample_batch(ctx: Context, model: Model, ev_vars: Sequence[int], rows, n_per_row: int, seed: int = 0,
                 first_sample: int = 0, row_stride: Optional[int] = None, heuristic: str = "mf", dtype: int = F64,
                 order: Optional[Sequence[int]] = None, rows_per_launch: int = 0, partial=None, soft=None):
    """n_per_row exact joint samples of P(x | evidence row) for every evidence
    row from one plan (bnpp_sample_batch) -> (samples uint8 (n, n_per_row,
    n_vars), log10_z float64[n], n_degenerate int64[n]).  rows: an (n,
    len(ev_vars)) integer array.  samples[b, s] is sample()'s draw for evidence
    row b with the same seed at the global index first_sample + b * row_stride
    + s, byte for byte.  row_stride None: n_per_row (disjoint streams, rows
    independent); 0: every row sees the same random numbers."""
    import numpy as np
    ne, ev_v, n, keep, ev_x = _ev_rows(ev_vars, rows)
    h, oa, no = _order_args(order, heuristic)
    k = int(n_per_row)
    stride = k if row_stride is None else int(row_stride)
    out = np.zeros((max(n, 1), max(k, 1), max(model.n_vars, 1)), dtype=np.uint8)
    lz = np.zeros(max(n, 1))
    deg = np.zeros(max(n, 1), dtype=np.int64)
    up = C.c_double()
    fn, name, pa, keep_lik = _sv("bnpp_sample_batch", _partial_flags(ev_vars, partial, keep), soft, model, n)
    _check(fn(_h(ctx), model.handle, ne, ev_v, n, ev_x, *pa, h, oa, no, dtype, int(rows_per_launch), k,
              int(first_sample), stride, int(seed) & 0xFFFFFFFFFFFFFFFF, _P(out.ctypes.data),
              lz.ctypes.data_as(_DP), deg.ctypes.data_as(_LP), C.byref(up)), name)
    del keep, keep_lik
    return out[:n, :k, :model.n_vars], lz[:n], deg[:n]


COUNTS_KEY = (1 << 24) + 16384      # the launch-group key of an accumulate step (plan.hpp kCountsKey)
PLAN_COUNTS_STATS = PLAN_BATCH_STATS + ("count_steps", "forward_levels")


def plan_counts(model: Model, ev_vars: Sequence[int], heuristic: str = "mf", dtype: int = F64,
                rows_per_launch: int = 0, order: Optional[Sequence[int]] = None, partial=None,
                soft=None):
    """Host-only planning of expected_counts (bnpp_plan_counts) -> (stats,
    groups, beliefs, no_b_elim): stats a dict of PLAN_COUNTS_STATS, groups one
    dict of PLAN_GROUP_FIELDS per launch group (the accumulate steps: key
    COUNTS_KEY, one group per factor; the groups up to level
    stats["forward_levels"] are plan_batch's), beliefs per factor the variables
    of the belief table its accumulate step reads (B reported as model.n_vars),
    no_b_elim whether no bucket sums B or merges it into a composite."""
    ev_vars = [int(v) for v in ev_vars]
    nb, flag = C.c_int(), C.c_int()
    off = (C.c_int * (model.n_factors + 1))()
    bvs = []

    def beliefs():                  # room for the belief variables the call before counted (at first: none)
        bvs.append((C.c_int * max(nb.value, 1))())
        return off, bvs[-1], nb.value, C.byref(nb), C.byref(flag)

    fn, name, pa, _ = _sv("bnpp_plan_counts", _partial_flags(ev_vars, partial), soft)
    tail, extra = _plan_tail(pa[0] if pa else None, len(ev_vars), soft, beliefs)
    st, groups = _plan_call(fn, name, PLAN_COUNTS_STATS,
                            (model.handle, len(ev_vars), _ints(ev_vars), *pa, *_order_args(order, heuristic), dtype,
                             int(rows_per_launch)), tail)
    bv = bvs[-1]
    res = st, groups, [[bv[j] for j in range(off[f], off[f + 1])] for f in range(model.n_factors)], bool(flag.value)
    return res + extra()


def expected_counts(ctx: Context, model: Model, ev_vars: Sequence[int], rows, weights=None, heuristic: str = "mf",
                    dtype: int = F64, rows_per_launch: int = 0, order: Optional[Sequence[int]] = None, partial=None,
                    soft=None):
    """Expected sufficient statistics of the evidence rows (bnpp_expected_counts)
    -> (counts, log10_z, n_impossible): counts one flat float64 array, the
    factors in model order, each N_f(x_S) = sum_b w_b P(x_S | row b) in its
    natural layout over its full scope (split_counts shapes them); log10_z per
    row as partition_batch's; n_impossible the rows with Z = 0, which count
    nowhere.  weights: None (all 1) or one finite weight >= 0 per row.  All
    rows share the evidence variables ev_vars: group rows with different missing
    patterns by pattern, call once per pattern and add the counts -- or declare
    the variables that are missing somewhere `partial` and pass MISSING."""
    import numpy as np
    ne, ev_v, n, keep, ev_x = _ev_rows(ev_vars, rows)
    h, oa, no = _order_args(order, heuristic)
    total = C.c_int64()
    _check(_lib.bnpp_counts_size(model.handle, C.byref(total)), "bnpp_counts_size")
    counts, lz = np.zeros(max(total.value, 1)), np.zeros(max(n, 1))
    w = None
    if weights is not None:
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        if w.shape[0] != n:
            raise ValueError("one weight per row is needed")
    ni = C.c_int64()
    up = C.c_double()
    fn, name, pa, keep_lik = _sv("bnpp_expected_counts", _partial_flags(ev_vars, partial, keep), soft, model, n)
    _check(fn(_h(ctx), model.handle, ne, ev_v, n, ev_x, *pa,
              w.ctypes.data_as(_DP) if w is not None else None, h, oa, no, dtype, int(rows_per_launch),
              counts.ctypes.data_as(_DP), lz.ctypes.data_as(_DP), C.byref(ni), C.byref(up)), name)
    del keep, keep_lik
    return counts[:total.value], lz[:n], ni.value


def split_counts(model_dict: dict, counts):
    """The flat counts of expected_counts as one array per factor, shaped by
    the cards of the factor's scope (model_dict: cards, scopes)."""
    import numpy as np
    counts = np.asarray(counts, dtype=np.float64).reshape(-1)
    out, at = [], 0
    for s in model_dict["scopes"]:
        shape = tuple(model_dict["cards"][v] for v in s)
        size = int(np.prod(shape, dtype=np.int64)) if shape else 1
        out.append(counts[at:at + size].reshape(shape))
        at += size
    if at != counts.shape[0]:
        raise ValueError("counts do not match the model's factors")
    return out


MARG_ROWS_KEY = (1 << 24) + 28672   # the launch-group key of the emit step of batched marginals (plan.hpp kMargRowsKey)
PLAN_MARGINALS_BATCH_STATS = PLAN_BATCH_STATS + ("emit_steps", "forward_levels", "belief_cols", "evidence_cols",
                                                 "free_cols", "width", "out_bytes", "belief_cols_b")
COL_KINDS = {1: "belief_b", 0: "belief", -1: "evidence", -2: "free"}


def _targets_arg(model: Model, targets):
    """(the target list, n_targets, targets as the C ABI takes them); None: all variables."""
    if targets is None:
        return list(range(model.n_vars)), 0, None
    ts = [int(t) for t in targets]
    return ts, len(ts), _ints(ts) if ts else (C.c_int * 1)()


def plan_marginals_batch(model: Model, ev_vars: Sequence[int], targets: Optional[Sequence[int]] = None,
                         heuristic: str = "mf", dtype: int = F64, rows_per_launch: int = 0,
                         order: Optional[Sequence[int]] = None, partial=None,
                         soft=None):
    """Host-only planning of marginals_batch (bnpp_plan_marginals_batch) ->
    (stats, groups, col_kinds): stats a dict of PLAN_MARGINALS_BATCH_STATS,
    groups one dict of PLAN_GROUP_FIELDS per launch group (the groups up to
    level stats["forward_levels"] are plan_batch's; the emit step is the last
    group, key MARG_ROWS_KEY, at a level of its own), col_kinds per target one
    of COL_KINDS' names: "belief_b" (its table carries the row variable),
    "belief" (no evidence reaches it), "evidence" or "free"."""
    ev_vars = [int(v) for v in ev_vars]
    ts, nt, ta = _targets_arg(model, targets)
    kinds = (C.c_int * max(len(ts), 1))()
    fn, name, pa, _ = _sv("bnpp_plan_marginals_batch", _partial_flags(ev_vars, partial), soft)
    tail, extra = _plan_tail(pa[0] if pa else None, len(ev_vars), soft, lambda: (kinds,))
    st, groups = _plan_call(fn, name, PLAN_MARGINALS_BATCH_STATS,
                            (model.handle, len(ev_vars), _ints(ev_vars), *pa, *_order_args(order, heuristic), nt, ta, dtype,
                             int(rows_per_launch)), tail)
    res = st, groups, [COL_KINDS[kinds[j]] for j in range(len(ts))]
    return res + extra()


def marginals_batch(ctx: Context, model: Model, ev_vars: Sequence[int], rows, targets: Optional[Sequence[int]] = None,
                    heuristic: str = "mf", dtype: int = F64, rows_per_launch: int = 0,
                    order: Optional[Sequence[int]] = None, out=None, partial=None, soft=None):
    """Every posterior marginal P(X_t | evidence row) of every row from one
    plan (bnpp_marginals_batch) -> (out, log10_z): out an (n, W) float64 array,
    row-major, W = sum of the targets' cards, the targets' blocks in the given
    order (None: all variables; split_marginals gives per-target views) -- the
    library writes it directly; log10_z per row as partition_batch's.  A target
    that is an evidence variable reads one-hot; a row with Z = 0 reads NaN in
    its other columns.  All rows share the evidence variables ev_vars.
    out: a C-contiguous (n, W) float64 array to write instead of a new one (a
    fresh array of 2^16 x 105 doubles costs more in page faults than the
    device-to-host copy that fills it)."""
    import numpy as np
    ne, ev_v, n, keep, ev_x = _ev_rows(ev_vars, rows)
    h, oa, no = _order_args(order, heuristic)
    ts, nt, ta = _targets_arg(model, targets)
    width = sum(model.cards[t] for t in ts if 0 <= t < model.n_vars)
    if out is None:
        out = np.empty((max(n, 1), max(width, 1)))
    elif not (isinstance(out, np.ndarray) and out.dtype == np.float64 and out.flags.c_contiguous and out.flags.writeable
              and out.shape == (max(n, 1), max(width, 1))):
        raise ValueError("out must be a writeable C-contiguous float64 array of shape (n, W)")
    lz = np.zeros(max(n, 1))
    up = C.c_double()
    fn, name, pa, keep_lik = _sv("bnpp_marginals_batch", _partial_flags(ev_vars, partial, keep), soft, model, n)
    _check(fn(_h(ctx), model.handle, ne, ev_v, n, ev_x, *pa, h, oa, no,
              nt, ta, dtype, int(rows_per_launch), out.ctypes.data_as(_DP), lz.ctypes.data_as(_DP),
              C.byref(up)), name)
    del keep, keep_lik
    return out[:n], lz[:n]


def split_marginals(cards: Sequence[int], targets: Optional[Sequence[int]], out):
    """The (n, W) array of marginals_batch as one (n, card) view per target, in
    the targets' order (None: all variables)."""
    ts = list(range(len(cards))) if targets is None else [int(t) for t in targets]
    if out.ndim != 2 or out.shape[1] != sum(cards[t] for t in ts):
        raise ValueError("the array does not match the targets' cards")
    views, at = [], 0
    for t in ts:
        views.append(out[:, at:at + cards[t]])
        at += cards[t]
    return views


def marginals(ctx: Context, model: Model, evidence=None, heuristic: str = "mf", dtype: int = F64,
              targets: Optional[Sequence[int]] = None):
    """BN::marginals (model.cpp:303-346) -> ({var: [p_0..p_k-1]}, uptime_ms)."""
    n, ev_v, ev_x = _ev(evidence)
    tg = list(range(model.n_vars)) if targets is None else list(targets)
    total = sum(model.cards[t] for t in tg)
    out = (C.c_double * max(total, 1))()
    up = C.c_double()
    _check(_lib.bnpp_marginals(ctx.handle, model.handle, n, ev_v, ev_x, HEURISTICS[heuristic], len(tg), _ints(tg),
                               dtype, out, C.byref(up)), "bnpp_marginals")
    res, o = {}, 0
    for t in tg:
        res[t] = list(out[o:o + model.cards[t]])
        o += model.cards[t]
    return res, up.value


def sum_product(ctx: Context, model: Model, max_iter: int = 10000, eps: float = 0.001):
    """BN::marginals with options["sum-product"] (model.cpp:313-317): loopy BP
    on the device (bnpp_sum_product) -> ({var: [p_0..p_k-1]}, iterations, uptime_ms).
    Evidence is not used on this path, as in the reference."""
    out = (C.c_double * max(sum(model.cards), 1))()
    it, up = C.c_int(), C.c_double()
    _check(_lib.bnpp_sum_product(ctx.handle, model.handle, max_iter, eps, out, C.byref(it), C.byref(up)),
           "bnpp_sum_product")
    res, o = {}, 0
    for t in range(model.n_vars):
        res[t] = list(out[o:o + model.cards[t]])
        o += model.cards[t]
    return res, it.value, up.value


def marginals_tree(ctx: Context, model: Model, evidence=None, heuristic: str = "mf", dtype: int = F64,
                   targets: Optional[Sequence[int]] = None, order: Optional[Sequence[int]] = None,
                   part: int = 0, n_parts: int = 1):
    """All marginals from one two-pass bucket tree (bnpp_marginals_tree) ->
    ({var: [p_0..p_k-1]}, uptime_ms).  Same output as marginals(), to rounding.
    part / n_parts (bnpp_marginals_tree_part): only the targets this part owns."""
    n, ev_v, ev_x = _ev(evidence)
    tg = list(range(model.n_vars)) if targets is None else list(targets)
    total = sum(model.cards[t] for t in tg)
    out = (C.c_double * max(total, 1))()
    owned = (C.c_int * max(len(tg), 1))()
    up = C.c_double()
    oa = _ints(list(order)) if order is not None else None
    h = ORDER_GIVEN if order is not None else HEURISTICS[heuristic]
    _check(_lib.bnpp_marginals_tree_part(ctx.handle, model.handle, n, ev_v, ev_x, h, oa,
                                         len(order) if order is not None else 0, len(tg), _ints(tg), part, n_parts,
                                         dtype, out, owned, C.byref(up)), "bnpp_marginals_tree_part")
    res, o = {}, 0
    for i, t in enumerate(tg):
        if owned[i]:
            res[t] = list(out[o:o + model.cards[t]])
        o += model.cards[t]
    return res, up.value


def plan_tree_part(model: Model, part: int, n_parts: int, evidence=None, heuristic: str = "mf", dtype: int = F64,
                   order: Optional[Sequence[int]] = None):
    """Host-only plan of one part of the bucket-tree marginals ->
    (owned variable ids, stats list as Job)."""
    n, ev_v, ev_x = _ev(evidence)
    owned = (C.c_int * max(model.n_vars, 1))()
    st = (C.c_double * 8)()
    oa = _ints(list(order)) if order is not None else None
    h = ORDER_GIVEN if order is not None else HEURISTICS[heuristic]
    _check(_lib.bnpp_plan_tree_part(model.handle, n, ev_v, ev_x, h, oa, len(order) if order is not None else 0,
                                    part, n_parts, dtype, owned, st, 8), "bnpp_plan_tree_part")
    return [v for v in range(model.n_vars) if owned[v]], list(st)


NO_EXP = -(1 << 40)       # out_exp2 of an all-zero share (include/bnpp.h)


def marginals_tree_sliced(ctx: Context, model: Model, rank: int, n_ranks: int, collective, evidence=None,
                          heuristic: str = "mf", dtype: int = F32, targets: Optional[Sequence[int]] = None,
                          order: Optional[Sequence[int]] = None, budget_gb: float = 0.0):
    """This rank's share of the message-sliced bucket-tree marginals
    (bnpp_marginals_tree_sliced) -> ({var: mantissas}, {var: exp2}, uptime_ms);
    the marginal of v is the normalised sum over ranks of mantissas * 2^exp2
    (bnpp.dist.sliced_tree_marginals).  collective: "loopback" (one GPU, a
    world of identical ranks: timing only; "loopback-nocopy": no bytes move)
    or callable(op, send, recv, nbytes,
    stream) with op COLL_ALLGATHER / COLL_ALLTOALL and device addresses.
    budget_gb > 0: the memory budget the plan must fit (every rank must pass
    the same: it sets the checkpoint count); 0: this device's free memory."""
    n, ev_v, ev_x = _ev(evidence)
    tg = list(range(model.n_vars)) if targets is None else list(targets)
    total = sum(model.cards[t] for t in tg)
    out = (C.c_double * max(total, 1))()
    exps = (C.c_int64 * max(len(tg), 1))()
    up = C.c_double()
    oa = _ints(list(order)) if order is not None else None
    h = ORDER_GIVEN if order is not None else HEURISTICS[heuristic]
    errors = []
    user = None
    if isinstance(collective, str) and collective.startswith("loopback"):
        # "loopback" (copies), "loopback-nocopy", "loopback-model:<MB/s per link>:<latency us>"
        # (no copies; each exchange's stream waits the modelled xGMI time)
        fn = COLLECTIVE_FN(C.cast(_lib.bnpp_collective_loopback, C.c_void_p).value)
        if collective.startswith("loopback-model"):
            _, rate, lat = collective.split(":")
            nr = (C.c_int * 4)(n_ranks, 3, int(rate), int(lat))
        else:
            nr = (C.c_int * 4)(n_ranks, 1 if collective == "loopback-nocopy" else 0, 0, 0)
        user = C.cast(nr, C.c_void_p)
    else:
        def _cb(_user, op, send, recv, nbytes, stream):
            try:
                collective(op, send, recv, nbytes, stream)
                return 0
            except BaseException as e:          # never unwind through the C frames
                errors.append(e)
                return 1
        fn = COLLECTIVE_FN(_cb)
    rc = _lib.bnpp_marginals_tree_sliced(ctx.handle, model.handle, n, ev_v, ev_x, h, oa,
                                         len(order) if order is not None else 0, len(tg), _ints(tg), rank, n_ranks,
                                         fn, user, C.c_double(budget_gb), dtype, out, exps, C.byref(up))
    if errors:
        raise errors[0]
    _check(rc, "bnpp_marginals_tree_sliced")
    mant, ex, o = {}, {}, 0
    for i, t in enumerate(tg):
        mant[t] = list(out[o:o + model.cards[t]])
        ex[t] = exps[i]
        o += model.cards[t]
    return mant, ex, up.value


def plan_tree_sliced(model: Model, rank: int, n_ranks: int, evidence=None, heuristic: str = "mf", dtype: int = F32,
                     order: Optional[Sequence[int]] = None):
    """Host-only plan of one rank of the sliced bucket tree -> (slice bit per
    variable, stats: Job's 8 then [8] exchanges, [9] bytes sent per call)."""
    n, ev_v, ev_x = _ev(evidence)
    sb = (C.c_int * max(model.n_vars, 1))()
    st = (C.c_double * 10)()
    oa = _ints(list(order)) if order is not None else None
    h = ORDER_GIVEN if order is not None else HEURISTICS[heuristic]
    _check(_lib.bnpp_plan_tree_sliced(model.handle, n, ev_v, ev_x, h, oa, len(order) if order is not None else 0,
                                      rank, n_ranks, dtype, sb, st, 10), "bnpp_plan_tree_sliced")
    return list(sb)[:model.n_vars], list(st)


def variable_elimination(ctx: Context, model: Model, variables: Sequence[int], heuristic: str = "given",
                         dtype: int = F64, cap_values: int = 1 << 20):
    """BN::variable_elimination over the model's factors as given ->
    (scope, values (scaled), exp2): true value = values * 2**exp2."""
    variables = list(variables)
    cap_vars = model.n_vars + 1
    ov = (C.c_int * cap_vars)()
    nd = C.c_int()
    size, e2 = C.c_int64(), C.c_int64()
    vals = (C.c_double * cap_values)()
    _check(_lib.bnpp_variable_elimination(ctx.handle, model.handle, len(variables), _ints(variables),
                                          HEURISTICS[heuristic], dtype, cap_vars, C.byref(nd), ov, cap_values,
                                          C.byref(size), vals, C.byref(e2)), "bnpp_variable_elimination")
    return list(ov[: nd.value]), list(vals[: size.value]), e2.value


class Job:
    """A prepared, device-resident inference (bnpp_job_*): launch() only enqueues."""

    def __init__(self, ctx: Context, model: Model, kind: str = "pr", evidence=None, heuristic: str = "mf",
                 dtype: int = F64, order: Optional[Sequence[int]] = None, targets: Optional[Sequence[int]] = None):
        n, ev_v, ev_x = _ev(evidence)
        self.model = model
        self.kind = {"pr": 0, "mar": 1, "mar_tree": 3, "mpe": 4}[kind]
        self.targets = list(range(model.n_vars)) if targets is None else list(targets)
        self._h = _P()
        order_arr = _ints(order) if order is not None else None
        h = ORDER_GIVEN if order is not None else HEURISTICS[heuristic]
        _check(_lib.bnpp_job_create(ctx.handle, model.handle, self.kind, n, ev_v, ev_x, h, order_arr,
                                    len(order) if order is not None else 0, len(self.targets), _ints(self.targets),
                                    dtype, C.byref(self._h)), "bnpp_job_create")
        st = (C.c_double * 8)()
        _check(_lib.bnpp_job_stats(self._h, st, 8), "bnpp_job_stats")
        (self.entries, self.arena_bytes, self.levels, self.buckets, self.width, self.max_table,
         self.alg_bytes, self.batches) = st[0], st[1], int(st[2]), int(st[3]), int(st[4]), st[5], st[6], int(st[7])

    def launch(self, stream: Optional[int] = None) -> None:
        _check(_lib.bnpp_job_launch(self._h, _P(stream) if stream else None), "bnpp_job_launch")

    def results(self, stream: Optional[int] = None):
        if self.kind == 0:
            out = (C.c_double * 1)()
            _check(_lib.bnpp_job_results(self._h, _P(stream) if stream else None, out), "bnpp_job_results")
            return out[0]
        if self.kind == 4:                   # (log10 of the maximum, the assignment)
            nv = self.model.n_vars
            out = (C.c_double * (1 + nv))()
            _check(_lib.bnpp_job_results(self._h, _P(stream) if stream else None, out), "bnpp_job_results")
            return out[0], [int(v) for v in out[1:1 + nv]]
        total = sum(self.model.cards[t] for t in self.targets)
        out = (C.c_double * max(total, 1))()
        _check(_lib.bnpp_job_results(self._h, _P(stream) if stream else None, out), "bnpp_job_results")
        res, o = {}, 0
        for t in self.targets:
            res[t] = list(out[o:o + self.model.cards[t]])
            o += self.model.cards[t]
        return res

    def close(self):
        if self._h:
            _lib.bnpp_job_free(self._h)
            self._h = _P()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def bucket_eliminate(ctx: Context, dtype: int, cards: Sequence[int], tables: Sequence[int],
                     scopes: Sequence[Sequence[int]], elim: int, out: int, out_vars: Sequence[int],
                     stream: Optional[int] = None, out_sum: Optional[int] = None) -> None:
    """Fused bucket on caller-owned device buffers (addresses as ints, e.g. torch
    tensor.data_ptr()).  Only enqueues on `stream`.  out_sum: device address of
    a float64 that receives the reference's partition sum (include/bnpp.h)."""
    arrs = [_ints(s) for s in scopes]
    ptrs = (_IP * len(arrs))(*[C.cast(a, _IP) for a in arrs])
    tabs = (_P * len(tables))(*[_P(t) for t in tables])
    _check(_lib.bnpp_bucket_eliminate(ctx.handle, _P(stream) if stream else None, dtype, len(cards), _ints(cards), len(tables),
                                      tabs, _ints([len(s) for s in scopes]), ptrs, elim, _P(out), len(out_vars),
                                      _ints(out_vars), _P(out_sum) if out_sum else None), "bnpp_bucket_eliminate")


def bucket_max(ctx: Context, dtype: int, cards: Sequence[int], tables: Sequence[int],
               scopes: Sequence[Sequence[int]], elim: int, out: int, out_vars: Sequence[int],
               out_arg: Optional[int] = None, stream: Optional[int] = None) -> None:
    """Max bucket on caller-owned device buffers (bnpp_bucket_max): out = the
    maximum over `elim` of the inputs' chain product, out_arg (uint8 per output
    entry, may be None) the lowest maximising value.  Only enqueues on `stream`."""
    arrs = [_ints(s) for s in scopes]
    ptrs = (_IP * len(arrs))(*[C.cast(a, _IP) for a in arrs])
    tabs = (_P * len(tables))(*[_P(t) for t in tables])
    _check(_lib.bnpp_bucket_max(ctx.handle, _P(stream) if stream else None, dtype, len(cards), _ints(cards), len(tables),
                                tabs, _ints([len(s) for s in scopes]), ptrs, elim, _P(out), len(out_vars),
                                _ints(out_vars), _P(out_arg) if out_arg else None), "bnpp_bucket_max")


def bucket_sample(ctx: Context, dtype: int, cards: Sequence[int], tables: Sequence[int],
                  scopes: Sequence[Sequence[int]], var: int, n_samples: int, x: int, seed: int = 0,
                  first_sample: int = 0, n_degenerate: Optional[int] = None, stream: Optional[int] = None) -> None:
    """One posterior-sampling draw per sample on caller-owned device buffers
    (bnpp_bucket_sample): reads the rows of the other scope variables from x
    (uint8[len(cards)][n_samples], variable-major) and writes row `var`;
    n_degenerate: a device int64 (may be None).  Only enqueues on `stream`."""
    arrs = [_ints(s) for s in scopes]
    ptrs = (_IP * max(len(arrs), 1))(*[C.cast(a, _IP) for a in arrs])
    tabs = (_P * max(len(tables), 1))(*[_P(t) for t in tables])
    _check(_lib.bnpp_bucket_sample(ctx.handle, _P(stream) if stream else None, dtype, len(cards), _ints(cards),
                                   len(tables), tabs, _ints([len(s) for s in scopes]), ptrs, var, int(n_samples),
                                   int(first_sample), int(seed) & 0xFFFFFFFFFFFFFFFF, _P(x),
                                   _P(n_degenerate) if n_degenerate else None), "bnpp_bucket_sample")


def divide(ctx: Context, dtype: int, cards: Sequence[int], a: int, a_scope: Sequence[int], b: int,
           b_scope: Sequence[int], out: int, out_vars: Sequence[int], stream: Optional[int] = None,
           out_sum: Optional[int] = None) -> None:
    """Factor::divide (factor.cpp:149-180) on caller-owned device buffers:
    out = a / b over the union scope (out_vars in any order of it)."""
    _check(_lib.bnpp_divide(ctx.handle, _P(stream) if stream else None, dtype, len(cards), _ints(cards), _P(a), len(a_scope),
                            _ints(a_scope), _P(b), len(b_scope), _ints(b_scope), _P(out), len(out_vars),
                            _ints(out_vars), _P(out_sum) if out_sum else None), "bnpp_divide")


def condition_batch(ctx: Context, dtype: int, cards: Sequence[int], table: int, scope: Sequence[int],
                    ev_vars: Sequence[int], n_rows: int, ev: int, out: int, stream: Optional[int] = None,
                    partial=None, soft=None) -> None:
    """Batched conditioning on caller-owned device buffers (bnpp_condition_batch):
    out[rest][b] = table conditioned on evidence row b; ev: a device
    int32[len(ev_vars)][n_rows], variable-major.  Only enqueues on `stream`.
    partial: the evidence variables that stay dims of `out` under the row's mask
    (bnpp_condition_batch_mv): a negative value is missing.
    soft: (soft_vars, lam) -- the weighted gather (bnpp_condition_batch_sv): the
    soft variables of the scope stay dims of `out`, scaled by lam, a device
    T[Ws][n_rows] in the call's dtype, (variable, value)-major, used as it is."""
    fn, name, pa = _mv("bnpp_condition_batch", _partial_flags(ev_vars, partial))
    if soft is not None:
        ids = [int(v) for v in soft[0]]
        fn, name = _lib.bnpp_condition_batch_sv, "bnpp_condition_batch_sv"
        pa = (pa[0] if pa else None, len(ids), _ints(ids) if ids else (C.c_int * 1)(), _P(soft[1]) if soft[1] else None)
    _check(fn(ctx.handle, _P(stream) if stream else None, dtype, len(cards), _ints(cards), _P(table),
              len(scope), _ints(scope), len(ev_vars), _ints(ev_vars), *pa, int(n_rows), _P(ev), _P(out)), name)


def bucket_counts(ctx: Context, dtype: int, cards: Sequence[int], table: int, scope: Sequence[int],
                  ev_vars: Sequence[int], n_rows: int, rows_live: int, ev: int, acc: int, weights: int = 0,
                  valid: int = 0, has_b: bool = True, stream: Optional[int] = None) -> None:
    """The accumulate step of expected_counts on caller-owned device buffers
    (bnpp_bucket_counts): the belief `table` over (scope minus ev_vars, b) is
    normalised row by row and added, times the row's weight, into `acc`, the
    factor's float64 table over `scope`.  ev: a device int32[len(ev_vars)][n_rows];
    weights: a device float64[n_rows] (0: all 1); valid: a device table of
    n_rows entries of the dtype (0: none).  Only enqueues on `stream`."""
    _check(_lib.bnpp_bucket_counts(ctx.handle, _P(stream) if stream else None, dtype, len(cards), _ints(cards), _P(table),
                                   len(scope), _ints(scope), len(ev_vars), _ints(ev_vars), int(n_rows), int(rows_live),
                                   _P(ev) if ev else None, _P(weights) if weights else None,
                                   _P(valid) if valid else None, 1 if has_b else 0, _P(acc)), "bnpp_bucket_counts")


def bucket_marginal_rows(ctx: Context, dtype: int, cards: Sequence[int], tables: Sequence[int], has_b: Sequence[bool],
                         ev_row: Sequence[int], n_rows: int, rows_live: int, ev: int, out: int,
                         stream: Optional[int] = None) -> None:
    """The emit step of marginals_batch on caller-owned device buffers
    (bnpp_bucket_marginal_rows): target j's table tables[j] over (x, b) -- b
    fastest, n_rows rows; has_b[j] false: no b -- is normalised row by row into
    columns off_j.. of out, a device float64[n_rows][sum(cards)], row-major.
    tables[j] 0: an evidence block (ev_row[j] >= 0, the row of ev = device
    int32[.][n_rows]) or a free block (1 / card).  Only enqueues on `stream`."""
    tabs = (_P * max(len(cards), 1))(*[_P(t) if t else None for t in tables])
    _check(_lib.bnpp_bucket_marginal_rows(ctx.handle if ctx is not None else None, _P(stream) if stream else None, dtype,
                                          len(cards), _ints(cards), tabs, _ints([1 if b else 0 for b in has_b]),
                                          _ints(ev_row), int(n_rows), int(rows_live), _P(ev) if ev else None, _P(out)),
           "bnpp_bucket_marginal_rows")


def condition(ctx: Context, dtype: int, cards: Sequence[int], table: int, scope: Sequence[int],
              evidence: Dict[int, int], out: int, stream: Optional[int] = None, out_sum: Optional[int] = None) -> None:
    n, ev_v, ev_x = _ev(evidence)
    _check(_lib.bnpp_condition(ctx.handle, _P(stream) if stream else None, dtype, len(cards), _ints(cards), _P(table), len(scope),
                               _ints(scope), n, ev_v, ev_x, _P(out), _P(out_sum) if out_sum else None), "bnpp_condition")
