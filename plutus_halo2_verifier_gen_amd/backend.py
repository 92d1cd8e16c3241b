"""ctypes binding of the C-ABI library (include/h2v.h -> libh2v_hip.so, built in-tree by __graft_entry__.build()).

There is deliberately NO fallback: if the HIP library is missing, or no GPU is present, every entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
from typing import Optional

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libh2v_hip.so")

H2V_OK = 0
ST_BAD_SCALAR, ST_INVERSE_OF_ZERO, ST_SHORT_PROOF, ST_BAD_POINT, ST_PAIRING, ST_RECURSION = 1, 2, 4, 8, 16, 32


class H2VError(RuntimeError):
    pass


class Batch(C.Structure):
    _fields_ = [("n", C.c_uint64), ("proofs", C.c_void_p), ("proof_off", C.c_void_p), ("instances", C.c_void_p),
                ("committed", C.c_void_p)]


class MixedBatch(C.Structure):
    """h2v_mixed_batch: plan_of is HOST memory in both forms of the call"""
    _fields_ = [("n", C.c_uint64), ("plan_of", C.c_void_p), ("proofs", C.c_void_p), ("proof_off", C.c_void_p),
                ("instances", C.c_void_p), ("committed", C.c_void_p)]


class Timings(C.Structure):
    _fields_ = [("transcript_combiner_ms", C.c_float), ("g1_decompress_ms", C.c_float), ("g1_msm_ms", C.c_float),
                ("pairing_ms", C.c_float), ("total_ms", C.c_float), ("launches", C.c_uint32),
                ("msm_lanes_per_term", C.c_uint32), ("pairing_lanes_per_proof", C.c_uint32),
                ("g1_msm_fixed_ms", C.c_float), ("msm_var_lanes_per_term", C.c_uint32)]


class PipProbe(C.Structure):
    """h2v_pip_probe (include/h2v.h)"""
    _fields_ = [("n", C.c_uint32), ("halves", C.c_uint32), ("scalars", C.c_char_p), ("n_points", C.c_uint32), ("n_pool0", C.c_uint32),
                ("points_compressed", C.c_char_p), ("pidx", C.POINTER(C.c_uint32)), ("out_xy_be", C.c_void_p), ("dump", C.POINTER(C.c_uint32))]


class RlcOpts(C.Structure):
    _fields_ = [("seed", C.c_uint8 * 32), ("flags", C.c_uint32)]


class RlcTimings(C.Structure):
    _fields_ = [("transcript_combiner_ms", C.c_float), ("g1_decompress_ms", C.c_float), ("prepare_ms", C.c_float),
                ("bucket_sort_ms", C.c_float), ("bucket_accumulate_ms", C.c_float), ("bucket_reduce_ms", C.c_float),
                ("pairing_ms", C.c_float), ("total_ms", C.c_float), ("msm_terms", C.c_uint32),
                ("window_bits", C.c_uint32), ("windows", C.c_uint32), ("max_chain", C.c_uint32)]


class AggregateInfo(C.Structure):
    """h2v_aggregate_info (include/h2v.h): what is needed to recompute the coefficients of an aggregate call"""
    _fields_ = [("seed_used", C.c_uint8 * 32), ("chunk", C.c_uint32), ("n_chunks", C.c_uint32), ("msm_terms", C.c_uint32),
                ("reserved", C.c_uint32)]        # the seed source, under the header's name for the word

    @property
    def seed_source(self) -> int:
        """0: seed_used was drawn or given; 1: derived (RLC_SEED_TRANSCRIPT) - H2V_AGGREGATE_SEED_SOURCE of the header"""
        return self.reserved


class PlanOpts(C.Structure):
    _fields_ = [("fixed_base_window_bits", C.c_uint32), ("reserved", C.c_uint32 * 7)]


class TuneReport(C.Structure):
    _fields_ = [("n_measured", C.c_uint32), ("calls_in_flight", C.c_uint32), ("default_ms", C.c_float), ("best_ms", C.c_float),
                ("pairing_engine", C.c_int32), ("msm_terms_per_lane", C.c_int32), ("reserved", C.c_uint32 * 4)]


# h2v_workspace_set_option / h2v_probe_set_option ids (include/h2v.h)
OPT_MSM_TERMS_PER_LANE, OPT_PAIRING_ENGINE, OPT_STREAMS, OPT_MSM_LANES_PER_TERM, OPT_MSM_BLOCK_SIZE, OPT_MSM_FIXED_SPLIT = 1, 2, 3, 4, 5, 6
OPT_COMBINER_SCHEDULE, OPT_COMBINER_PROOFS_PER_BLOCK = 7, 8   # (9 and 10 are retired)
OPT_RLC_GROUP_STAGE, OPT_RLC_WINDOW_BITS, OPT_RLC_CHAIN, OPT_RLC_ROUTE, OPT_COALESCE = 11, 12, 13, 14, 15
OPT_COUNT = 16

RLC_SEED_GIVEN = 1
RLC_ONE_STREAM = 2
RLC_FOLD_PAIRS = 4   # recursive plans: combine the pairs (el', er') the fold leaves (include/h2v.h)
RLC_GROUPED = 16     # h2v_aggregate_mixed(_device) only: the MIXED_GROUPED form of the call (bit 8 stays unknown)
RLC_SEED_TRANSCRIPT = 32   # the seed is derived from the batch itself (seed.py has the rule); never beside RLC_SEED_GIVEN
RLC_SEED_KEYED = 64        # the mixed calls' derived seed: form 3, keyed leaves (seed.mixed_seed); never beside the two above
SUBMIT_RLC = 1
MIXED_RLC = 1          # h2v_verify_mixed: ONE pairing for the call
MIXED_FOLD_MSM = 2     # ... and ONE bucket MSM over the call's per-proof terms (only together with MIXED_RLC)
MIXED_GROUPED = 4      # ... and phase 1 of every groupable plan in ONE launch per kernel (only together with both)
MIXED_ACROSS_SRS = 16  # ... with MIXED_RLC: the listed plans may be on several SRS; ONE multi-pairing for the call (bit 8 stays unknown)
MIXED_MAX_PLANS = 64   # H2V_MIXED_MAX_PLANS
MULTI_SRS_MAX = 16     # H2V_MULTI_SRS_MAX: ranges (plans listed) in one h2v_check_pairs_multi call
MIXED_GROUPED_MAX_PLANS = 1024   # H2V_MIXED_GROUPED_MAX_PLANS: plans listed in a MIXED_GROUPED call
MIXED_GROUPED_MAX_OTHER = 62     # H2V_MIXED_GROUPED_MAX_OTHER: ... of which plans that cannot be grouped and have proofs
BATCH_NOT_CHECKED = 2  # H2V_BATCH_NOT_CHECKED: batch_accepted of an aggregate call (Workspace.rlc_verdict)


def _rlc_opts(seed, one_stream: bool = False, fold_pairs: bool = False, grouped: bool = False, derive_seed: bool = False,
              keyed_seed: bool = False):
    """derive_seed / keyed_seed beside a seed or beside each other go to the library as they are: the library answers H2V_E_ARG"""
    if seed is None and not one_stream and not fold_pairs and not grouped and not derive_seed and not keyed_seed:
        return None
    flags = ((RLC_ONE_STREAM if one_stream else 0) | (RLC_FOLD_PAIRS if fold_pairs else 0) | (RLC_GROUPED if grouped else 0) |
             (RLC_SEED_TRANSCRIPT if derive_seed else 0) | (RLC_SEED_KEYED if keyed_seed else 0))
    if seed is None:
        return RlcOpts((C.c_uint8 * 32)(), flags)
    seed = bytes(seed)
    if len(seed) != 32:
        raise ValueError("the RLC seed is 32 bytes")
    return RlcOpts((C.c_uint8 * 32)(*seed), flags | RLC_SEED_GIVEN)


EXPORTS = [
    "h2v_plan_load", "h2v_plan_load_ex", "h2v_plan_free", "h2v_plan_info", "h2v_plan_compile", "h2v_blob_free", "h2v_workspace_create", "h2v_workspace_free",
    "h2v_workspace_timings", "h2v_workspace_hint_in_flight", "h2v_workspace_create_lanes", "h2v_workspace_create_multi", "h2v_workspace_defer_joins",
    "h2v_workspace_join", "h2v_workspace_lanes", "h2v_workspace_depth", "h2v_workspace_set_option", "h2v_workspace_get_option", "h2v_workspace_tune", "h2v_probe_set_option",
    "h2v_verify_batch", "h2v_verify_batch_submit", "h2v_verify_batch_wait", "h2v_verify_batch_device", "h2v_verify_batch_rlc", "h2v_verify_batch_rlc_device",
    "h2v_workspace_rlc_result", "h2v_probe_g1_msm_pippenger", "h2v_probe_g1_msm_pippenger_ex", "h2v_plan_trace_slots", "h2v_trace", "h2v_probe_vm", "h2v_probe_field",
    "h2v_probe_blake2b", "h2v_probe_g1_decompress", "h2v_probe_g1_msm", "h2v_probe_g1_msm_multi", "h2v_probe_g1_msm_fixed", "h2v_probe_quad_madd", "h2v_probe_f28_dot2", "h2v_probe_pairing", "h2v_probe_pairing_ex",
    "h2v_probe_pairing_states",
    "h2v_last_error", "h2v_build_id",
    "h2v_device_count", "h2v_shutdown",
    "h2v_prepare_batch", "h2v_prepare_batch_device", "h2v_check_pairs", "h2v_check_pairs_device",
    "h2v_check_pairs_rlc", "h2v_check_pairs_rlc_device", "h2v_check_pairs_multi", "h2v_check_pairs_multi_device",
    "h2v_plan_transcript", "h2v_probe_blake2b_ex",
    "h2v_verify_mixed", "h2v_verify_mixed_device", "h2v_probe_mixed_fold_sums", "h2v_probe_mixed_fold_sums_multi", "h2v_probe_decompress",
    "h2v_aggregate_batch", "h2v_aggregate_batch_device", "h2v_aggregate_mixed", "h2v_aggregate_mixed_device", "h2v_plan_same_srs",
    "h2v_workspace_seed_used", "h2v_workspace_seed_ms", "h2v_probe_batch_seed", "h2v_plan_key_tag",
    "h2v_probe_mixed_seed",
]
# exported for the tests alone and not part of include/h2v.h (csrc/h2v_probes.hpp)
PROBE_ONLY_EXPORTS = ["h2v_probe_device_memory", "h2v_probe_six_call", "h2v_probe_coop_call"]

# transcript hash kinds of a plan (include/h2v.h: H2V_TRANSCRIPT_*; vk.TRANSCRIPT_KINDS)
TRANSCRIPT_CARDANO_BLAKE2B_256, TRANSCRIPT_BLAKE2B_512 = 0, 1
TRANSCRIPT_NAMES = {TRANSCRIPT_CARDANO_BLAKE2B_256: "cardano-blake2b-256", TRANSCRIPT_BLAKE2B_512: "blake2b-512"}

_lib = None


def lib():
    """Loads libh2v_hip.so.  Raises if it has not been built: the HIP extension is mandatory."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise H2VError("HIP backend library %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback)" % LIB_PATH)
        # PyTorch-ROCm bundles its own copy of the HIP runtime under the system's soname.  If this library came first, the
        # process would hold /opt/rocm's runtime and a later `import torch` could no longer see the GPU ("No HIP GPUs are
        # available"): a Python host that may hand over torch tensors lets torch load its runtime first.
        if "torch" not in sys.modules and os.environ.get("H2V_NO_TORCH_PRELOAD") is None:
            try:
                import torch  # noqa: F401
            except Exception:
                pass
        L = C.CDLL(LIB_PATH)
        L.h2v_last_error.restype = C.c_char_p
        L.h2v_build_id.restype = C.c_char_p
        L.h2v_plan_load.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.POINTER(C.c_void_p)]
        L.h2v_plan_load_ex.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.POINTER(PlanOpts), C.POINTER(C.c_void_p)]
        L.h2v_plan_free.argtypes = [C.c_void_p]
        L.h2v_plan_compile.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
        L.h2v_blob_free.argtypes = [C.c_void_p]
        L.h2v_plan_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_uint32)] * 4
        L.h2v_workspace_create.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]
        L.h2v_workspace_free.argtypes = [C.c_void_p]
        L.h2v_workspace_create_lanes.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
        L.h2v_workspace_create_multi.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
        L.h2v_workspace_defer_joins.argtypes = [C.c_void_p, C.c_int]
        L.h2v_workspace_join.argtypes = [C.c_void_p, C.c_void_p]
        L.h2v_workspace_lanes.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.h2v_workspace_depth.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_uint32)]
        L.h2v_workspace_set_option.argtypes = [C.c_void_p, C.c_uint32, C.c_int32]
        L.h2v_workspace_get_option.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_int32)]
        L.h2v_probe_set_option.argtypes = [C.c_uint32, C.c_int32]
        L.h2v_workspace_tune.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(TuneReport)]
        L.h2v_workspace_timings.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(Timings)]
        L.h2v_verify_batch.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_void_p]
        L.h2v_verify_batch_device.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.POINTER(Timings)]
        L.h2v_verify_batch_submit.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_uint32, C.POINTER(RlcOpts)]
        L.h2v_verify_batch_wait.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
        L.h2v_verify_batch_rlc.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_void_p, C.POINTER(RlcOpts),
                                           C.POINTER(C.c_int)]
        L.h2v_verify_batch_rlc_device.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.POINTER(RlcOpts)]
        L.h2v_workspace_rlc_result.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(RlcTimings)]
        L.h2v_probe_g1_msm_pippenger.argtypes = [C.c_int, C.c_uint32, C.c_char_p, C.c_char_p, C.c_void_p]
        L.h2v_probe_g1_msm_pippenger_ex.argtypes = [C.c_int, C.c_uint32, C.POINTER(PipProbe), C.c_uint32]
        L.h2v_plan_trace_slots.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32)]
        L.h2v_plan_transcript.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p, C.POINTER(C.c_uint32)]
        L.h2v_probe_blake2b_ex.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_void_p]
        L.h2v_trace.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_char_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)]
        L.h2v_probe_vm.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.h2v_probe_decompress.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
        L.h2v_probe_field.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.h2v_probe_f28_dot2.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.h2v_probe_blake2b.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_char_p, C.c_void_p]
        L.h2v_probe_g1_decompress.argtypes = [C.c_int, C.c_uint32, C.c_char_p, C.c_void_p, C.c_void_p]
        L.h2v_probe_g1_msm.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_char_p, C.c_char_p, C.c_void_p]
        L.h2v_probe_g1_msm_multi.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_char_p, C.c_char_p, C.c_void_p]
        L.h2v_probe_g1_msm_fixed.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_void_p, C.POINTER(C.c_uint32)]
        L.h2v_probe_pairing.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_char_p, C.c_void_p]
        L.h2v_probe_pairing_ex.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_char_p, C.c_void_p, C.c_int, C.c_void_p]
        L.h2v_probe_pairing_states.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
        L.h2v_shutdown.argtypes = [C.c_int]
        L.h2v_prepare_batch.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_void_p, C.c_void_p]
        L.h2v_prepare_batch_device.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.h2v_check_pairs.argtypes = [C.c_void_p, C.c_uint64, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.h2v_check_pairs_device.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.h2v_check_pairs_rlc.argtypes = [C.c_void_p, C.c_uint64, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RlcOpts),
                                          C.POINTER(C.c_int)]
        L.h2v_check_pairs_rlc_device.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.POINTER(RlcOpts)]
        L.h2v_check_pairs_multi.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.c_uint64), C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.POINTER(RlcOpts), C.POINTER(C.c_int)]
        L.h2v_check_pairs_multi_device.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.POINTER(RlcOpts)]
        L.h2v_verify_mixed.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(MixedBatch), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                       C.POINTER(RlcOpts), C.POINTER(C.c_int)]
        L.h2v_verify_mixed_device.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(MixedBatch), C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_uint32, C.POINTER(RlcOpts)]
        L.h2v_probe_mixed_fold_sums.argtypes = [C.c_void_p, C.c_void_p]
        L.h2v_probe_mixed_fold_sums_multi.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]
        L.h2v_plan_same_srs.argtypes = [C.c_void_p, C.c_void_p]
        L.h2v_workspace_seed_used.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
        L.h2v_workspace_seed_ms.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_float)]
        L.h2v_probe_batch_seed.argtypes = [C.c_int, C.c_uint32, C.c_char_p, C.POINTER(Batch), C.c_uint32, C.c_uint32, C.c_void_p]
        L.h2v_probe_mixed_seed.argtypes = [C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.h2v_plan_key_tag.argtypes = [C.c_void_p, C.c_void_p]
        L.h2v_probe_device_memory.argtypes = [C.c_int, C.POINTER(C.c_uint64)]
        L.h2v_probe_six_call.argtypes = [C.c_int, C.c_int, C.c_uint32, C.c_uint32] + [C.c_void_p] * 7
        L.h2v_probe_coop_call.argtypes = [C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32] + [C.c_void_p] * 7
        L.h2v_aggregate_batch.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RlcOpts),
                                          C.POINTER(AggregateInfo)]
        L.h2v_aggregate_batch_device.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.POINTER(RlcOpts), C.POINTER(AggregateInfo)]
        L.h2v_aggregate_mixed.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(MixedBatch), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.POINTER(RlcOpts), C.POINTER(AggregateInfo)]
        L.h2v_aggregate_mixed_device.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(MixedBatch), C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.POINTER(RlcOpts), C.POINTER(AggregateInfo)]
        # h2v_shutdown before the interpreter goes down: the library's pool streams (hardware queues of their own) must not
        # outlive the HIP runtime / a profiler's tool library (include/h2v.h: library lifecycle).  Handles that Python still
        # holds afterwards are empty shells; their __del__ frees the host structs only.
        import atexit
        atexit.register(L.h2v_shutdown, -1)
        _lib = L
    return _lib


def check(rc: int):
    if rc != H2V_OK:
        raise H2VError("h2v error %d: %s" % (rc, (lib().h2v_last_error() or b"").decode()))


def probe_set_option(option: int, value: int) -> None:
    """h2v_probe_set_option: the launch-shape option the h2v_probe_* calls of this thread run with (0 = the launcher's choice)"""
    check(lib().h2v_probe_set_option(option, value))


def plan_compile(vk_json: str) -> bytes:
    """h2v_plan_compile: the C++ plan compiler behind the C-ABI (host-only; byte-identical with plan.compile_plan)."""
    raw = vk_json.encode()
    out, n = C.c_void_p(), C.c_size_t()
    check(lib().h2v_plan_compile(raw, len(raw), C.byref(out), C.byref(n)))
    try:
        return C.string_at(out, n.value)
    finally:
        lib().h2v_blob_free(out)


def device_count() -> int:
    return lib().h2v_device_count()


def shutdown(device: int = -1) -> None:
    """h2v_shutdown: release everything the library owns on `device` (-1: every device); later calls raise H2VError."""
    check(lib().h2v_shutdown(device))


class DevicePlan:
    """A plan uploaded to one GPU (h2v_plan*)."""

    def __init__(self, plan_bytes: bytes, device: int = 0, fixed_base_window_bits: int = 0):
        """fixed_base_window_bits (h2v_plan_load_ex): 0 = the library's choice, or 4 / 8 / 12"""
        self._h = C.c_void_p()
        self.device = device
        if fixed_base_window_bits:
            opts = PlanOpts(fixed_base_window_bits, (C.c_uint32 * 7)())
            check(lib().h2v_plan_load_ex(plan_bytes, len(plan_bytes), device, C.byref(opts), C.byref(self._h)))
        else:
            check(lib().h2v_plan_load(plan_bytes, len(plan_bytes), device, C.byref(self._h)))
        v = [C.c_uint32() for _ in range(4)]
        check(lib().h2v_plan_info(self._h, *[C.byref(x) for x in v]))
        self.proof_len, self.n_pi, self.n_ci, self.n_terms = [x.value for x in v]
        n = C.c_uint32()
        check(lib().h2v_plan_trace_slots(self._h, None, 0, C.byref(n)))
        slots = (C.c_uint32 * max(1, n.value))()
        check(lib().h2v_plan_trace_slots(self._h, slots, n.value, C.byref(n)))
        self.trace_slots = list(slots[:n.value])
        kind, klen, key = C.c_uint32(), C.c_uint32(), C.create_string_buffer(64)
        check(lib().h2v_plan_transcript(self._h, C.byref(kind), key, C.byref(klen)))
        # the transcript hash of the plan's key (TRANSCRIPT_*) and its blake2b key: what api.prepare holds a transcript's tag against
        self.transcript_kind, self.transcript_key = kind.value, key.raw[:klen.value]
        tag = C.create_string_buffer(32)
        check(lib().h2v_plan_key_tag(self._h, tag))
        self.key_tag = tag.raw      # seed.key_tag(plan_bytes): what a derived batch seed binds the key with

    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, "_h", None):
            lib().h2v_plan_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- host-buffer batch verify
    def _host_batch(self, proofs: bytes, proof_off, instances: bytes, committed: Optional[bytes]):
        n = len(proof_off) - 1
        if n < 0 or any(proof_off[i + 1] < proof_off[i] for i in range(n)) or (n >= 0 and proof_off[0] < 0):
            raise H2VError("proof offsets must be non-decreasing")
        if n > 0 and proof_off[-1] > len(proofs):
            raise H2VError("proof_off[n] = %d exceeds the %d proof bytes handed over" % (proof_off[-1], len(proofs)))
        if self.n_pi and len(instances or b"") < 32 * self.n_pi * n:
            raise H2VError("instances: expected %d bytes" % (32 * self.n_pi * n))
        if self.n_ci and len(committed or b"") < 48 * n:
            raise H2VError("committed: expected %d bytes" % (48 * n))
        off = (C.c_uint64 * (n + 1))(*proof_off)
        pbuf = C.create_string_buffer(proofs, len(proofs)) if proofs else C.create_string_buffer(1)
        ibuf = C.create_string_buffer(instances, len(instances)) if instances else None
        cbuf = C.create_string_buffer(committed, len(committed)) if committed else None
        b = Batch(n, C.cast(pbuf, C.c_void_p), C.cast(off, C.c_void_p),
                  C.cast(ibuf, C.c_void_p) if ibuf is not None else None,
                  C.cast(cbuf, C.c_void_p) if cbuf is not None else None)
        return n, b, (off, pbuf, ibuf, cbuf)   # (the buffers must outlive the call)

    def verify_batch(self, proofs: bytes, proof_off, instances: bytes, committed: Optional[bytes], ws=None) -> bytes:
        n, b, _keep = self._host_batch(proofs, proof_off, instances, committed)
        acc = (C.c_uint8 * max(1, n))()
        check(lib().h2v_verify_batch(self._h, C.byref(b), acc, ws.handle if ws else None))
        return bytes(acc[:n])

    def host_batch(self, proofs: bytes, proof_off, instances: bytes, committed: Optional[bytes]):
        """The batch as ctypes buffers a caller owns (what a Rust / C caller hands over): (h2v_batch, keep-alive)."""
        n, b, keep = self._host_batch(proofs, proof_off, instances, committed)
        return b, keep

    def submit(self, batch: "Batch", ws, rlc: bool = False, seed: Optional[bytes] = None, one_stream: bool = False,
               fold_pairs: bool = False, derive_seed: bool = False):
        """h2v_verify_batch_submit: copy + upload + verification + download enqueued on the workspace's stream."""
        opts = _rlc_opts(seed, one_stream, fold_pairs, derive_seed=derive_seed)
        check(lib().h2v_verify_batch_submit(self._h, C.byref(batch), ws.handle, SUBMIT_RLC if rlc else 0,
                                            C.byref(opts) if opts is not None else None))

    def verify_batch_rlc(self, proofs: bytes, proof_off, instances: bytes, committed: Optional[bytes], ws=None,
                         seed: Optional[bytes] = None, fold_pairs: bool = False, derive_seed: bool = False):
        """Batch-accept fast path (h2v_verify_batch_rlc): returns (accept bytes, fell_back).  fold_pairs (RLC_FOLD_PAIRS):
        the batch form of recursive plans, which starts after the fold; ignored by any other plan.  derive_seed
        (RLC_SEED_TRANSCRIPT): the seed is a digest of the batch (seed.batch_seed); ws.seed_used() has it afterwards."""
        n, b, _keep = self._host_batch(proofs, proof_off, instances, committed)
        acc = (C.c_uint8 * max(1, n))()
        fb = C.c_int(0)
        opts = _rlc_opts(seed, fold_pairs=fold_pairs, derive_seed=derive_seed)
        check(lib().h2v_verify_batch_rlc(self._h, C.byref(b), acc, ws.handle if ws else None,
                                         C.byref(opts) if opts is not None else None, C.byref(fb)))
        return bytes(acc[:n]), bool(fb.value)

    def verify_batch_rlc_device(self, n, d_proofs, d_off, d_inst, d_ci, d_accept, d_status=None, ws=None, stream=None,
                                seed: Optional[bytes] = None, one_stream: bool = False, fold_pairs: bool = False,
                                derive_seed: bool = False):
        b = Batch(n, d_proofs, d_off, d_inst, d_ci)
        opts = _rlc_opts(seed, one_stream, fold_pairs, derive_seed=derive_seed)
        check(lib().h2v_verify_batch_rlc_device(self._h, C.byref(b), d_accept, d_status, ws.handle if ws else None, stream,
                                                C.byref(opts) if opts is not None else None))

    # ---- device-resident batch verify (pointers = torch tensor data_ptr())
    def verify_batch_device(self, n, d_proofs, d_off, d_inst, d_ci, d_accept, d_status=None, ws=None, stream=None,
                            timings: bool = False):
        b = Batch(n, d_proofs, d_off, d_inst, d_ci)
        tm = Timings() if timings else None
        check(lib().h2v_verify_batch_device(self._h, C.byref(b), d_accept, d_status, ws.handle if ws else None, stream,
                                            C.byref(tm) if timings else None))
        return tm

    # ---- prepare (the pairing's two points per proof) and the pair check (include/h2v.h)
    def prepare_batch(self, proofs: bytes, proof_off, instances: bytes, committed: Optional[bytes], ws=None):
        """h2v_prepare_batch: (pairs, status) - pairs = n x 96 bytes compress(L) || compress(R) (96 zero bytes for a proof
        rejected before the pairing), status = the verify call's status words without ST_PAIRING."""
        n, b, _keep = self._host_batch(proofs, proof_off, instances, committed)
        pairs = C.create_string_buffer(96 * max(1, n))
        st = (C.c_uint32 * max(1, n))()
        check(lib().h2v_prepare_batch(self._h, C.byref(b), pairs, st, ws.handle if ws else None))
        return pairs.raw[:96 * n], list(st[:n])

    def prepare_batch_device(self, n, d_proofs, d_off, d_inst, d_ci, d_pairs, d_status=None, ws=None, stream=None):
        """h2v_prepare_batch_device: enqueues on `stream`; d_pairs = n x 96 bytes of device memory (4-byte aligned)"""
        b = Batch(n, d_proofs, d_off, d_inst, d_ci)
        check(lib().h2v_prepare_batch_device(self._h, C.byref(b), d_pairs, d_status, ws.handle if ws else None, stream))

    def check_pairs(self, pairs: bytes, ws=None):
        """h2v_check_pairs: (accept bytes, status) for n = len(pairs) / 96 pairs compress(L) || compress(R)"""
        if len(pairs) % 96:
            raise H2VError("pairs: a multiple of 96 bytes")
        n = len(pairs) // 96
        acc = (C.c_uint8 * max(1, n))()
        st = (C.c_uint32 * max(1, n))()
        check(lib().h2v_check_pairs(self._h, n, bytes(pairs), acc, st, ws.handle if ws else None))
        return bytes(acc[:n]), list(st[:n])

    def check_pairs_device(self, n, d_pairs, d_accept, d_status=None, ws=None, stream=None):
        """h2v_check_pairs_device: enqueues on `stream`"""
        check(lib().h2v_check_pairs_device(self._h, n, d_pairs, d_accept, d_status, ws.handle if ws else None, stream))

    def check_pairs_rlc(self, pairs: bytes, ws=None, seed: Optional[bytes] = None, derive_seed: bool = False):
        """h2v_check_pairs_rlc: (accept bytes, status, fell_back) - check_pairs's outputs with ONE pairing for the batch
        when every decoded pair's equation holds; fell_back: the batch check failed and the per-pair kernels ran."""
        if len(pairs) % 96:
            raise H2VError("pairs: a multiple of 96 bytes")
        n = len(pairs) // 96
        acc = (C.c_uint8 * max(1, n))()
        st = (C.c_uint32 * max(1, n))()
        fb = C.c_int(0)
        opts = _rlc_opts(seed, derive_seed=derive_seed)
        check(lib().h2v_check_pairs_rlc(self._h, n, bytes(pairs), acc, st, ws.handle if ws else None,
                                        C.byref(opts) if opts is not None else None, C.byref(fb)))
        return bytes(acc[:n]), list(st[:n]), bool(fb.value)

    def check_pairs_rlc_device(self, n, d_pairs, d_accept, d_status=None, ws=None, stream=None, seed: Optional[bytes] = None,
                               derive_seed: bool = False):
        """h2v_check_pairs_rlc_device: enqueues on `stream`; ws.rlc_result() has the batch verdict afterwards"""
        opts = _rlc_opts(seed, derive_seed=derive_seed)
        check(lib().h2v_check_pairs_rlc_device(self._h, n, d_pairs, d_accept, d_status, ws.handle if ws else None, stream,
                                               C.byref(opts) if opts is not None else None))

    # ---- aggregate calls: the batch's ONE pair instead of a pairing on it (include/h2v.h: h2v_aggregate_batch)
    def aggregate_batch(self, proofs: bytes, proof_off, instances: bytes, committed: Optional[bytes], ws=None,
                        seed: Optional[bytes] = None, one_stream: bool = False, derive_seed: bool = False):
        """h2v_aggregate_batch: (pair, included, status, info) - pair = 96 bytes compress(L) || compress(R) with L = sum r_i L_i,
        R = sum r_i R_i over the included proofs; included = n bytes, 1 = not rejected before the pairing (NOT a verdict);
        status = h2v_prepare_batch's; info = an AggregateInfo (the seed and the chunking the coefficients follow)."""
        n, b, _keep = self._host_batch(proofs, proof_off, instances, committed)
        pair = C.create_string_buffer(96)
        inc = (C.c_uint8 * max(1, n))()
        st = (C.c_uint32 * max(1, n))()
        info = AggregateInfo()
        opts = _rlc_opts(seed, one_stream, derive_seed=derive_seed)
        check(lib().h2v_aggregate_batch(self._h, C.byref(b), pair, inc, st, ws.handle if ws else None,
                                        C.byref(opts) if opts is not None else None, C.byref(info)))
        return pair.raw, bytes(inc[:n]), list(st[:n]), info

    def aggregate_batch_device(self, n, d_proofs, d_off, d_inst, d_ci, d_pair, d_included, d_status=None, ws=None, stream=None,
                               seed: Optional[bytes] = None, one_stream: bool = False, derive_seed: bool = False) -> AggregateInfo:
        """h2v_aggregate_batch_device: enqueues on `stream`; d_pair = 96 bytes of device memory (4-byte aligned), d_included = n.
        Returns the call's AggregateInfo (host memory, filled in before the call returns)."""
        b = Batch(n, d_proofs, d_off, d_inst, d_ci)
        info = AggregateInfo()
        opts = _rlc_opts(seed, one_stream, derive_seed=derive_seed)
        check(lib().h2v_aggregate_batch_device(self._h, C.byref(b), d_pair, d_included, d_status, ws.handle if ws else None, stream,
                                               C.byref(opts) if opts is not None else None, C.byref(info)))
        return info

    def trace(self, proof: bytes, instances: bytes, committed: Optional[bytes]):
        nt = len(self.trace_slots)
        sc = C.create_string_buffer(32 * max(1, nt))
        ms = C.create_string_buffer(32 * self.n_terms)
        el = C.create_string_buffer(96)
        er = C.create_string_buffer(96)
        st = C.c_uint32()
        acc = C.c_uint8()
        check(lib().h2v_trace(self._h, proof, len(proof), instances, committed, sc, ms, el, er, C.byref(st), C.byref(acc)))
        scal = {self.trace_slots[k]: int.from_bytes(sc.raw[32 * k:32 * k + 32], "little") for k in range(nt)}
        msm = [int.from_bytes(ms.raw[32 * k:32 * k + 32], "little") for k in range(self.n_terms)]

        def pt(b):
            return None if b == bytes(96) else (int.from_bytes(b[:48], "big"), int.from_bytes(b[48:], "big"))

        return {"scalars": scal, "msm_scalars": msm, "el": pt(el.raw), "er": pt(er.raw), "status": st.value,
                "accept": acc.value}


class Workspace:
    """h2v_workspace.  lanes / chunk given (0 = the library's choice): a LANED workspace (h2v_workspace_create_lanes) -
    calls on it are cut into chunks that are pipelined through library-owned lanes; plain Workspace(plan, n) is laned by
    itself from FOUR TIMES the plan's chunk size up (h2v_workspace_create), an ordinary workspace below that.  A laned
    workspace has at most 16 lanes (= host batches in flight through submit / wait), no trace buffer, and - with deferred
    joins - refuses the legacy NULL stream: its lanes run on blocking streams, which any NULL-stream work (PyTorch's
    default stream, a synchronous hipMemcpy) would drain (include/h2v.h: h2v_workspace_defer_joins)."""

    def __init__(self, plan: DevicePlan, max_batch: int, lanes: Optional[int] = None, chunk: Optional[int] = None):
        self._h = C.c_void_p()
        if lanes is None and chunk is None:
            check(lib().h2v_workspace_create(plan.handle, max_batch, C.byref(self._h)))
        else:
            check(lib().h2v_workspace_create_lanes(plan.handle, max_batch, lanes or 0, chunk or 0, C.byref(self._h)))
        self.max_batch = max_batch

    @classmethod
    def multi(cls, plans, max_batch: int, lanes: int = 0, chunk: int = 0) -> "Workspace":
        """h2v_workspace_create_multi: ONE laned workspace for several plans of one device (calls name their plan as usual)"""
        self = cls.__new__(cls)
        self._h = C.c_void_p()
        arr = (C.c_void_p * len(plans))(*[p.handle for p in plans])
        check(lib().h2v_workspace_create_multi(arr, len(plans), max_batch, lanes, chunk, C.byref(self._h)))
        self.max_batch = max_batch
        return self

    def lanes(self):
        """(number of lanes, chunk size); (1, max_batch) for a workspace that is not laned"""
        a, b = C.c_uint32(), C.c_uint32()
        check(lib().h2v_workspace_lanes(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def depth(self, n: int, rlc: bool = False) -> int:
        """h2v_workspace_depth: calls of n proofs the workspace keeps in flight before a call waits for a lane"""
        a = C.c_uint32()
        check(lib().h2v_workspace_depth(self._h, n, 1 if rlc else 0, C.byref(a)))
        return a.value

    OPT_MSM_TERMS_PER_LANE, OPT_PAIRING_ENGINE, OPT_STREAMS = 1, 2, 3

    def set_option(self, option: int, value: int) -> None:
        """h2v_workspace_set_option: a launch shape instead of the launcher's choice (0 = back to its choice)"""
        check(lib().h2v_workspace_set_option(self._h, option, value))

    def get_option(self, option: int) -> int:
        v = C.c_int32()
        check(lib().h2v_workspace_get_option(self._h, option, C.byref(v)))
        return v.value

    def tune(self, plan: "DevicePlan", n, d_proofs, d_off, d_inst, d_ci, stream) -> "TuneReport":
        """h2v_workspace_tune: measure the candidate launch shapes on this device-resident batch, keep the fastest"""
        b = Batch(n, d_proofs, d_off, d_inst, d_ci)
        rep = TuneReport()
        check(lib().h2v_workspace_tune(plan.handle, C.byref(b), self._h, stream, 0, C.byref(rep)))
        return rep

    def defer_joins(self, on: bool = True) -> None:
        """h2v_workspace_defer_joins: device-resident calls return without making the caller's stream wait, so that
        consecutive calls overlap in the lanes; join() orders a stream behind everything submitted so far."""
        check(lib().h2v_workspace_defer_joins(self._h, 1 if on else 0))

    def join(self, stream=None) -> None:
        check(lib().h2v_workspace_join(self._h, stream))

    @property
    def handle(self):
        return self._h

    def timings(self, calls_back: int = 0) -> Timings:
        tm = Timings()
        check(lib().h2v_workspace_timings(self._h, calls_back, C.byref(tm)))
        return tm

    def hint_in_flight(self, n: int) -> None:
        """h2v_workspace_hint_in_flight: the caller keeps n batches in flight (a tuning hint; results do not depend on it)."""
        check(lib().h2v_workspace_hint_in_flight(self._h, C.c_uint32(n)))

    def wait(self, n: int):
        """h2v_verify_batch_wait for the batch submitted on this workspace: (accept bytes, fell_back)."""
        acc = (C.c_uint8 * max(1, n))()
        fb = C.c_int(0)
        check(lib().h2v_verify_batch_wait(self._h, acc, C.byref(fb)))
        return bytes(acc[:n]), bool(fb.value)

    def rlc_result(self, calls_back: int = 0, timings: bool = True):
        """(batch check passed?, RlcTimings) of a past RLC call on this workspace; synchronise its stream first."""
        ok = C.c_uint32(0)
        tm = RlcTimings() if timings else None
        check(lib().h2v_workspace_rlc_result(self._h, calls_back, C.byref(ok), C.byref(tm) if timings else None))
        return bool(ok.value), tm

    def seed_used(self, calls_back: int = 0) -> bytes:
        """h2v_workspace_seed_used: the 32-byte seed a past call with derive_seed derived; synchronise its stream first.  Raises
        H2VError for a call that derived nothing."""
        out = C.create_string_buffer(32)
        check(lib().h2v_workspace_seed_used(self._h, calls_back, out))
        return out.raw

    def seed_ms(self, calls_back: int = 0) -> float:
        """h2v_workspace_seed_ms: device time of that call's digest launches"""
        ms = C.c_float(0)
        check(lib().h2v_workspace_seed_ms(self._h, calls_back, C.byref(ms)))
        return ms.value

    def rlc_verdict(self, calls_back: int = 0) -> int:
        """batch_accepted of h2v_workspace_rlc_result as the library reports it: 1 passed, 0 failed / routed, BATCH_NOT_CHECKED (2)
        for an aggregate call"""
        ok = C.c_uint32(0)
        check(lib().h2v_workspace_rlc_result(self._h, calls_back, C.byref(ok), None))
        return ok.value

    def close(self):
        if getattr(self, "_h", None):
            lib().h2v_workspace_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- mixed-key batches (include/h2v.h: h2v_verify_mixed)
def _mixed_mode(mode: str, fold_msm: bool = False, grouped: bool = False, across_srs: bool = False) -> int:
    if mode not in ("per-proof", "rlc"):
        raise ValueError("mode is 'per-proof' or 'rlc'")
    if across_srs and mode != "rlc":
        raise ValueError("across_srs needs mode='rlc' (H2V_MIXED_ACROSS_SRS is valid only together with H2V_MIXED_RLC)")
    if fold_msm and mode != "rlc":
        raise ValueError("fold_msm needs mode='rlc' (H2V_MIXED_FOLD_MSM is valid only together with H2V_MIXED_RLC)")
    # (grouped without fold_msm goes to the library as it is: the library answers H2V_E_ARG)
    return ((MIXED_RLC if mode == "rlc" else 0) | (MIXED_FOLD_MSM if fold_msm else 0) | (MIXED_GROUPED if grouped else 0) |
            (MIXED_ACROSS_SRS if across_srs else 0))


def verify_mixed(plans, plan_of, proofs: bytes, proof_off, instances: Optional[bytes], committed: Optional[bytes], ws=None,
                 mode: str = "per-proof", seed: Optional[bytes] = None, fold_msm: bool = False, grouped: bool = False,
                 keyed_seed: bool = False, across_srs: bool = False):
    """h2v_verify_mixed: n proofs of several plans on ONE SRS (across_srs: on several) in one call; proof i belongs to plans[plan_of[i]], its public
    inputs (and committed instance, where its plan has one) follow those of the proofs before it.  Returns (accept bytes,
    status list, fell_back) in the caller's order.  mode="rlc": ONE pairing for the call (fell_back: the batch check failed
    and the per-pair kernels produced accept[]).  fold_msm (mode="rlc" only; MIXED_FOLD_MSM): ONE bucket MSM over the call's
    per-proof terms as well - no ladder MSM unless the check fails, in which case the call runs again without it (fell_back).
    grouped (with fold_msm only; MIXED_GROUPED): phase 1 of every groupable plan in one launch per kernel, up to
    MIXED_GROUPED_MAX_PLANS plans - the same results.  keyed_seed (mode="rlc"; RLC_SEED_KEYED): the seed is a digest of the call
    (seed.mixed_seed: every leaf binds its own proof's key), the same in every form; ws.seed_used() has it afterwards.
    across_srs (mode="rlc" only; MIXED_ACROSS_SRS): the plans may be on up to MULTI_SRS_MAX SRS with proofs, and the call ends in
    ONE multi-pairing - with fold_msm over one left-hand bucket sum per SRS, without it over the proofs' pairs.  ws: typically Workspace.multi over the same plans; None: a temporary one."""
    n = len(proof_off) - 1
    if n < 0 or len(plan_of) != n:
        raise H2VError("plan_of: one entry per proof")
    if any(proof_off[i + 1] < proof_off[i] for i in range(n)) or (n > 0 and (proof_off[0] < 0 or proof_off[-1] > len(proofs))):
        raise H2VError("proof offsets must be non-decreasing and within the proof bytes handed over")
    arr = (C.c_void_p * max(1, len(plans)))(*[p.handle for p in plans])
    po = (C.c_uint32 * max(1, n))(*plan_of)
    off = (C.c_uint64 * (n + 1))(*proof_off)
    pbuf = C.create_string_buffer(proofs, len(proofs)) if proofs else C.create_string_buffer(1)
    ibuf = C.create_string_buffer(instances, len(instances)) if instances else None
    cbuf = C.create_string_buffer(committed, len(committed)) if committed else None
    b = MixedBatch(n, C.cast(po, C.c_void_p), C.cast(pbuf, C.c_void_p), C.cast(off, C.c_void_p),
                   C.cast(ibuf, C.c_void_p) if ibuf is not None else None, C.cast(cbuf, C.c_void_p) if cbuf is not None else None)
    acc = (C.c_uint8 * max(1, n))()
    st = (C.c_uint32 * max(1, n))()
    fb = C.c_int(0)
    flags = _mixed_mode(mode, fold_msm, grouped, across_srs)
    opts = _rlc_opts(seed, keyed_seed=keyed_seed)
    check(lib().h2v_verify_mixed(arr, len(plans), C.byref(b), acc, st, ws.handle if ws else None, flags,
                                 C.byref(opts) if opts is not None else None, C.byref(fb)))
    return bytes(acc[:n]), list(st[:n]), bool(fb.value)


def verify_mixed_device(plans, plan_of, n: int, d_proofs, d_off, d_inst, d_ci, d_accept, d_status=None, ws=None, stream=None,
                        mode: str = "per-proof", seed: Optional[bytes] = None, fold_msm: bool = False, grouped: bool = False,
                        keyed_seed: bool = False, across_srs: bool = False) -> None:
    """h2v_verify_mixed_device: enqueues on `stream`; plan_of is a host list, every d_* a device pointer.  `stream` has
    waited for the call's lanes when this returns (a join point, deferred joins or not); ws.rlc_result() has the batch
    verdict of an mode="rlc" call once the stream is synchronised.  fold_msm: as verify_mixed; the call then returns only
    after the batch verdict is known (it synchronises `stream` once).  across_srs: as verify_mixed."""
    if len(plan_of) != n:
        raise H2VError("plan_of: one entry per proof")
    flags = _mixed_mode(mode, fold_msm, grouped, across_srs)
    arr = (C.c_void_p * max(1, len(plans)))(*[p.handle for p in plans])
    po = (C.c_uint32 * max(1, n))(*plan_of)
    b = MixedBatch(n, C.cast(po, C.c_void_p), d_proofs, d_off, d_inst, d_ci)
    opts = _rlc_opts(seed, keyed_seed=keyed_seed)
    check(lib().h2v_verify_mixed_device(arr, len(plans), C.byref(b), d_accept, d_status, ws.handle if ws else None, stream,
                                        flags, C.byref(opts) if opts is not None else None))


def aggregate_mixed(plans, plan_of, proofs: bytes, proof_off, instances: Optional[bytes], committed: Optional[bytes], ws=None,
                    seed: Optional[bytes] = None, grouped: bool = False, keyed_seed: bool = False):
    """h2v_aggregate_mixed: the fold_msm form of verify_mixed without its verdict - (pair, included, status, info) for the call,
    included / status in the caller's order; the coefficient of proof i follows its position in the call (info.chunk = 0).
    grouped (RLC_GROUPED): phase 1 as verify_mixed(grouped=True) runs it - the same pair.  keyed_seed (RLC_SEED_KEYED): the seed
    is seed.mixed_seed of the call - info.seed_source = 1, info.seed_used has it."""
    n = len(proof_off) - 1
    if n < 0 or len(plan_of) != n:
        raise H2VError("plan_of: one entry per proof")
    if any(proof_off[i + 1] < proof_off[i] for i in range(n)) or (n > 0 and (proof_off[0] < 0 or proof_off[-1] > len(proofs))):
        raise H2VError("proof offsets must be non-decreasing and within the proof bytes handed over")
    arr = (C.c_void_p * max(1, len(plans)))(*[p.handle for p in plans])
    po = (C.c_uint32 * max(1, n))(*plan_of)
    off = (C.c_uint64 * (n + 1))(*proof_off)
    pbuf = C.create_string_buffer(proofs, len(proofs)) if proofs else C.create_string_buffer(1)
    ibuf = C.create_string_buffer(instances, len(instances)) if instances else None
    cbuf = C.create_string_buffer(committed, len(committed)) if committed else None
    b = MixedBatch(n, C.cast(po, C.c_void_p), C.cast(pbuf, C.c_void_p), C.cast(off, C.c_void_p),
                   C.cast(ibuf, C.c_void_p) if ibuf is not None else None, C.cast(cbuf, C.c_void_p) if cbuf is not None else None)
    pair = C.create_string_buffer(96)
    inc = (C.c_uint8 * max(1, n))()
    st = (C.c_uint32 * max(1, n))()
    info = AggregateInfo()
    opts = _rlc_opts(seed, grouped=grouped, keyed_seed=keyed_seed)
    check(lib().h2v_aggregate_mixed(arr, len(plans), C.byref(b), pair, inc, st, ws.handle if ws else None,
                                    C.byref(opts) if opts is not None else None, C.byref(info)))
    return pair.raw, bytes(inc[:n]), list(st[:n]), info


def aggregate_mixed_device(plans, plan_of, n: int, d_proofs, d_off, d_inst, d_ci, d_pair, d_included, d_status=None, ws=None,
                           stream=None, seed: Optional[bytes] = None, grouped: bool = False, keyed_seed: bool = False) -> AggregateInfo:
    """h2v_aggregate_mixed_device: enqueues on `stream` and returns - no verdict comes down, the stream is not synchronised
    (keyed_seed: info.seed_used is zero, ws.seed_used() has the seed once the stream is synchronised)"""
    if len(plan_of) != n:
        raise H2VError("plan_of: one entry per proof")
    arr = (C.c_void_p * max(1, len(plans)))(*[p.handle for p in plans])
    po = (C.c_uint32 * max(1, n))(*plan_of)
    b = MixedBatch(n, C.cast(po, C.c_void_p), d_proofs, d_off, d_inst, d_ci)
    info = AggregateInfo()
    opts = _rlc_opts(seed, grouped=grouped, keyed_seed=keyed_seed)
    check(lib().h2v_aggregate_mixed_device(arr, len(plans), C.byref(b), d_pair, d_included, d_status, ws.handle if ws else None, stream,
                                           C.byref(opts) if opts is not None else None, C.byref(info)))
    return info


def check_pairs_multi(plans, counts, pairs: bytes, ws=None, seed: Optional[bytes] = None):
    """h2v_check_pairs_multi: ONE batch check over pairs on several SRS.  The first counts[0] pairs (96 bytes each) are checked
    against the SRS of plans[0], the next counts[1] against plans[1], ...; at most MULTI_SRS_MAX ranges.  Returns (accept bytes,
    status list, fell_back) - position for position what plans[k].check_pairs gives for range k; fell_back: the one check
    failed and the per-pair kernels produced accept[].  ws: any workspace check_pairs would take for n pairs; None: a temporary one."""
    if len(plans) != len(counts):
        raise H2VError("counts: one entry per plan")
    n = sum(counts)
    if len(pairs) != 96 * n:
        raise H2VError("pairs: 96 bytes per pair, sum(counts) pairs")
    arr = (C.c_void_p * max(1, len(plans)))(*[p.handle for p in plans])
    cnt = (C.c_uint64 * max(1, len(counts)))(*counts)
    acc = (C.c_uint8 * max(1, n))()
    st = (C.c_uint32 * max(1, n))()
    fb = C.c_int(0)
    opts = _rlc_opts(seed)
    check(lib().h2v_check_pairs_multi(arr, len(plans), cnt, bytes(pairs), acc, st, ws.handle if ws else None,
                                      C.byref(opts) if opts is not None else None, C.byref(fb)))
    return bytes(acc[:n]), list(st[:n]), bool(fb.value)


def check_pairs_multi_device(plans, counts, d_pairs, d_accept, d_status=None, ws=None, stream=None, seed: Optional[bytes] = None) -> None:
    """h2v_check_pairs_multi_device: enqueues on `stream` (counts is a host list, every d_* a device pointer; ws is required);
    ws.rlc_result() has the batch verdict once the stream is synchronised"""
    if len(plans) != len(counts):
        raise H2VError("counts: one entry per plan")
    arr = (C.c_void_p * max(1, len(plans)))(*[p.handle for p in plans])
    cnt = (C.c_uint64 * max(1, len(counts)))(*counts)
    opts = _rlc_opts(seed)
    check(lib().h2v_check_pairs_multi_device(arr, len(plans), cnt, d_pairs, d_accept, d_status, ws.handle if ws else None, stream,
                                             C.byref(opts) if opts is not None else None))


def probe_mixed_fold_sums(ws):
    """h2v_probe_mixed_fold_sums: (L, R) of the most recent fold_msm call on ws as affine (x, y) integer pairs, None = infinity"""
    out = C.create_string_buffer(192)
    check(lib().h2v_probe_mixed_fold_sums(ws.handle, out))
    return _unxy(out.raw[:96]), _unxy(out.raw[96:])


def probe_mixed_fold_sums_multi(ws, cap: int = 16):
    """h2v_probe_mixed_fold_sums_multi: (R, [L_k per SRS class with proofs, in class order]) of the most recent across_srs +
    fold_msm call on ws, as affine (x, y) integer pairs, None = infinity"""
    out = C.create_string_buffer((1 + cap) * 96)
    nc = C.c_uint32(0)
    check(lib().h2v_probe_mixed_fold_sums_multi(ws.handle, cap, out, C.byref(nc)))
    return _unxy(out.raw[:96]), [_unxy(out.raw[96 * (1 + k):96 * (2 + k)]) for k in range(nc.value)]


def probe_device_memory(device: int = 0):
    """h2v_probe_device_memory: what the library's owners hold on `device` right now - (device blocks, device bytes, pinned
    blocks, pinned bytes, events).  Counts; no GPU is touched."""
    out = (C.c_uint64 * 5)()
    check(lib().h2v_probe_device_memory(device, out))
    return tuple(int(v) for v in out)


def probe_batch_seed(form: int, key_tag: bytes, proofs: bytes, proof_off=None, instances: Optional[bytes] = None,
                     committed: Optional[bytes] = None, n_pi: int = 0, n_ci: int = 0, device: int = 0) -> bytes:
    """h2v_probe_batch_seed: the digest kernels of a derived seed alone, on bytes that need not be proofs.  form 1: proof i =
    proofs[proof_off[i] : proof_off[i + 1]] with n_pi x 32 instance bytes and n_ci x 48 committed bytes; form 2: n = len(proofs) /
    96 pairs.  Returns the 32-byte seed (seed.batch_seed states the same)."""
    if form == 2:
        n, off = len(proofs) // 96, None
    else:
        n = len(proof_off) - 1
        off = (C.c_uint64 * (n + 1))(*proof_off)
    pbuf = C.create_string_buffer(proofs, len(proofs)) if proofs else C.create_string_buffer(1)
    ibuf = C.create_string_buffer(instances, len(instances)) if instances else None
    cbuf = C.create_string_buffer(committed, len(committed)) if committed else None
    b = Batch(n, C.cast(pbuf, C.c_void_p), C.cast(off, C.c_void_p) if off is not None else None,
              C.cast(ibuf, C.c_void_p) if ibuf is not None else None, C.cast(cbuf, C.c_void_p) if cbuf is not None else None)
    out = C.create_string_buffer(32)
    check(lib().h2v_probe_batch_seed(device, form, bytes(key_tag), C.byref(b), n_pi, n_ci, out))
    return out.raw


def probe_mixed_seed(tags, shapes, plan_of, proofs: bytes, proof_off, instances: Optional[bytes] = None,
                     committed: Optional[bytes] = None, device: int = 0) -> bytes:
    """h2v_probe_mixed_seed: the digest kernels of a keyed seed (form 3) alone, on bytes that need not be proofs.  tags: 32 bytes
    per listed plan; shapes[k] = (n_pi, n_ci); the rest as an h2v_mixed_batch (a descending pair of offsets is an empty proof).
    Returns the 32-byte seed (seed.mixed_seed_flat states the same)."""
    n, k = len(proof_off) - 1, len(tags)
    if len(plan_of) != n or len(shapes) != k:
        raise H2VError("plan_of: one entry per proof; shapes: one per tag")
    tbuf = C.create_string_buffer(b"".join(bytes(t) for t in tags), 32 * max(1, k))
    npi = (C.c_uint32 * max(1, k))(*[s[0] for s in shapes])
    nci = (C.c_uint32 * max(1, k))(*[s[1] for s in shapes])
    po = (C.c_uint32 * max(1, n))(*plan_of)
    off = (C.c_uint64 * (n + 1))(*proof_off)
    pbuf = C.create_string_buffer(proofs, len(proofs)) if proofs else C.create_string_buffer(1)
    ibuf = C.create_string_buffer(instances, len(instances)) if instances else None
    cbuf = C.create_string_buffer(committed, len(committed)) if committed else None
    b = MixedBatch(n, C.cast(po, C.c_void_p), C.cast(pbuf, C.c_void_p), C.cast(off, C.c_void_p),
                   C.cast(ibuf, C.c_void_p) if ibuf is not None else None, C.cast(cbuf, C.c_void_p) if cbuf is not None else None)
    out = C.create_string_buffer(32)
    check(lib().h2v_probe_mixed_seed(device, k, tbuf, npi, nci, C.byref(b), out))
    return out.raw


# ---- primitive probes (GPU parity tests)
class BatchStream:
    """Keeps up to `depth` host-buffer batches in flight on ONE laned workspace (h2v_workspace_create_lanes with `depth`
    lanes, one chunk per batch) through h2v_verify_batch_submit / _wait: push() hands a host batch over and returns the
    (accept bytes, fell_back) of the OLDEST batch once `depth` are in flight, or None; drain() returns the rest, oldest
    first.  The counterpart of h2v::BatchStream.  (Round 2 needed `depth` workspaces for this.)"""

    def __init__(self, plan: "DevicePlan", max_batch: int, depth: int, rlc: bool = False, seed: bytes = None):
        if depth < 1 or depth > 16:
            raise H2VError("BatchStream: depth must be 1 .. 16 (a laned workspace has at most 16 lanes)")
        self.plan, self.rlc, self.seed, self.depth = plan, rlc, seed, depth
        self.ws = Workspace(plan, max_batch, lanes=depth, chunk=max_batch)
        self._n = []          # proofs of the batches in flight, oldest first

    def push(self, host_batch, n: int):
        """host_batch: DevicePlan.host_batch(...)[0]; n: its number of proofs"""
        out = None
        if len(self._n) >= self.depth:     # every lane holds a batch: collect the oldest
            out = self.ws.wait(self._n.pop(0))
        self.plan.submit(host_batch, self.ws, rlc=self.rlc, seed=self.seed)
        self._n.append(n)
        return out

    def drain(self):
        out = []
        while self._n:
            out.append(self.ws.wait(self._n.pop(0)))
        return out

    def close(self):
        if self.ws is not None:
            self.ws.close()
            self.ws = None


def probe_vm(plan: DevicePlan, proofs: bytes, proof_off, instances: bytes, committed: Optional[bytes], want_trace: bool = True):
    """h2v_probe_vm: the transcript + combiner interpreter alone on a batch.  Returns (status words, scalars[n][n_terms],
    trace) with trace = one {slot id: register value} dict per proof, or None without want_trace (which forces the plan's
    narrow schedule: the trace table names its registers).  The launch shape comes from probe_set_option."""
    n, b, _keep = plan._host_batch(proofs, proof_off, instances, committed)
    nt, T = len(plan.trace_slots), plan.n_terms
    st = (C.c_uint32 * max(1, n))()
    ms = C.create_string_buffer(32 * T * max(1, n))
    tr = C.create_string_buffer(32 * max(1, nt * n)) if want_trace else None
    check(lib().h2v_probe_vm(plan.handle, C.byref(b), 1 if want_trace else 0, st, ms, tr))
    raw = ms.raw
    scal = [[int.from_bytes(raw[32 * (i * T + k):32 * (i * T + k + 1)], "little") for k in range(T)] for i in range(n)]
    trace = None
    if want_trace:
        raw = tr.raw
        trace = [{plan.trace_slots[k]: int.from_bytes(raw[32 * (i * nt + k):32 * (i * nt + k + 1)], "little") for k in range(nt)}
                 for i in range(n)]
    return list(st[:n]), scal, trace


def probe_decompress(plan: DevicePlan, slots: int, proofs: bytes, proof_off, instances: bytes, committed: Optional[bytes], tables: bool = True):
    """h2v_probe_decompress: the decompression launch of the pipelines alone on a batch.  slots = point slots per proof (proof
    points + committed instance + 2 accumulator points of a recursive plan).  Returns (xy, valid, valid_sub, tab, blocks) over
    the n * slots points, proof by proof: xy = 96 bytes x || y big-endian per point in one bytes object, valid / valid_sub = one
    byte per point, tab = 1792 bytes (448 little-endian dwords) per point or None without `tables` (the launch then builds
    none), blocks = the grid of the launch."""
    n, b, _keep = plan._host_batch(proofs, proof_off, instances, committed)
    m = max(1, n * slots)
    xy, valid, sub = C.create_string_buffer(96 * m), C.create_string_buffer(m), C.create_string_buffer(m)
    tab = C.create_string_buffer(1792 * m) if tables else None
    blocks = C.c_uint32()
    check(lib().h2v_probe_decompress(plan.handle, C.byref(b), 1 if tables else 0, xy, valid, sub, tab, C.byref(blocks)))
    return xy.raw, valid.raw, sub.raw, tab.raw if tables else None, blocks.value


def probe_field(op: int, a_list, b_list, device: int = 0):
    nl = 12 if op < 4 else 8
    n = len(a_list)
    nb = nl * 4

    def pack(vals):
        return b"".join(int(v).to_bytes(nb, "little") for v in vals)

    out = C.create_string_buffer(n * nb)
    pa, pb = pack(a_list), pack(b_list)
    check(lib().h2v_probe_field(device, op, n, pa, pb, out))
    return [int.from_bytes(out.raw[nb * i:nb * (i + 1)], "little") for i in range(n)]


def probe_blake2b(msgs, device: int = 0):
    n = len(msgs)
    ln = len(msgs[0])
    assert all(len(m) == ln for m in msgs)
    out = C.create_string_buffer(32 * n)
    check(lib().h2v_probe_blake2b(device, n, ln, b"".join(msgs), out))
    return [out.raw[32 * i:32 * i + 32] for i in range(n)]


def probe_blake2b_ex(msgs, digest_len: int = 64, key: bytes = b"", device: int = 0):
    """blake2b of `digest_len` (32 / 64) bytes keyed with `key` of equally long messages, through the transcript code of the
    keyed flavour (tr_put / tr_digest behind a host-computed state)."""
    n = len(msgs)
    ln = len(msgs[0])
    assert all(len(m) == ln for m in msgs)
    out = C.create_string_buffer(digest_len * n)
    check(lib().h2v_probe_blake2b_ex(device, n, ln, b"".join(msgs), digest_len, bytes(key), len(key), out))
    return [out.raw[digest_len * i:digest_len * (i + 1)] for i in range(n)]


def _unxy(b):
    return None if b == bytes(96) else (int.from_bytes(b[:48], "big"), int.from_bytes(b[48:], "big"))


def probe_g1_decompress(compressed_list, device: int = 0):
    n = len(compressed_list)
    out = C.create_string_buffer(96 * n)
    valid = C.create_string_buffer(n)
    check(lib().h2v_probe_g1_decompress(device, n, b"".join(compressed_list), out, valid))
    return [(valid.raw[i] == 1, _unxy(out.raw[96 * i:96 * i + 96])) for i in range(n)]


def probe_g1_msm(scalar_groups, base_groups, device: int = 0):
    """scalar_groups[i] = list of T ints, base_groups[i] = list of T 48-byte compressed points."""
    n = len(scalar_groups)
    T = len(scalar_groups[0])
    sc = b"".join(int(s).to_bytes(32, "little") for g in scalar_groups for s in g)
    bs = b"".join(b for g in base_groups for b in g)
    out = C.create_string_buffer(96 * n)
    check(lib().h2v_probe_g1_msm(device, n, T, sc, bs, out))
    return [_unxy(out.raw[96 * i:96 * i + 96]) for i in range(n)]


def probe_g1_msm_multi(scalar_groups, base_groups, halves_per_lane: int, device: int = 0):
    """probe_g1_msm's sums through k_g1_msm_multi alone, `halves_per_lane` (3 .. 8) GLV halves per lane."""
    n = len(scalar_groups)
    T = len(scalar_groups[0])
    assert all(len(g) == T for g in scalar_groups) and all(len(g) == T for g in base_groups) and len(base_groups) == n
    sc = b"".join(int(s).to_bytes(32, "little") for g in scalar_groups for s in g)
    bs = b"".join(b for g in base_groups for b in g)
    out = C.create_string_buffer(96 * n)
    check(lib().h2v_probe_g1_msm_multi(device, n, T, halves_per_lane, sc, bs, out))
    return [_unxy(out.raw[96 * i:96 * i + 96]) for i in range(n)]


def probe_g1_msm_fixed(plan: DevicePlan, scalar_rows, bases_per_lane: int = 1):
    """sum_t s_t * B_t over the plan's VK-base terms through the all-window tables (k_g1_msm_fixed); scalar_rows[i] = the
    n_fix scalars of proof i (ints < r), in the order of the plan's VK-base terms.  n_fix() = probe_g1_msm_fixed(plan, None)."""
    nf = C.c_uint32()
    if scalar_rows is None:
        lib().h2v_probe_g1_msm_fixed(plan.handle, 0, 1, None, None, C.byref(nf))
        return nf.value
    n = len(scalar_rows)
    sc = b"".join(int(s).to_bytes(32, "little") for row in scalar_rows for s in row)
    out = C.create_string_buffer(96 * n)
    check(lib().h2v_probe_g1_msm_fixed(plan.handle, n, bases_per_lane, sc, out, C.byref(nf)))
    assert all(len(row) == nf.value for row in scalar_rows)
    return [_unxy(out.raw[96 * i:96 * i + 96]) for i in range(n)]


# h2v_probe_f28_dot2 op codes (include/h2v.h)
DOT2_MUL, DOT2_SQR, DOT2_SQR2, DOT2_DBL, DOT2_MADD, DOT2_ADD, DOT2_INLINE, DOT2_NEG_Q = 0, 1, 2, 8, 9, 10, 16, 64
DOT2_PLAIN_MUL, DOT2_PLAIN_SQR = 3, 4   # a b through fp_mont28, a^2 through fp_montsqr28


def probe_f28_dot2(op: int, a, b=None, c=None, d=None, device: int = 0):
    """h2v_probe_f28_dot2 on raw lazily reduced records.  Field ops (0..4): a, b, c, d are lists of 14-limb records (one the op does not
    use may be left out), the result a list of 14-limb records.  Point ops (8..10): a and b are lists of (X, Y, Z) triples of 14-limb records, the result a list
    of ((X, Y, Z) records, return code)."""
    n = len(a)
    field = (op & 15) < 8

    def pack(recs):
        if recs is None:
            return None
        flat = [l for r in recs for l in (r if field else [x for rec in r for x in rec])]
        assert len(flat) == n * (14 if field else 42)
        return (C.c_uint32 * len(flat))(*flat)

    out = (C.c_uint32 * (n * (14 if field else 44)))()
    if field:
        b, c, d = (a if r is None else r for r in (b, c, d))
    check(lib().h2v_probe_f28_dot2(device, op, n, pack(a), pack(b), pack(c), pack(d), out))
    if field:
        return [list(out[14 * i:14 * i + 14]) for i in range(n)]
    return [(tuple(list(out[44 * i + 14 * j:44 * i + 14 * j + 14]) for j in range(3)), int(out[44 * i + 42])) for i in range(n)]


# h2v_probe_six_call ops (csrc/h2v_pairing_six.hpp: SIX_PROBE_*)
SIX_MUL, SIX_SQR, SIX_LINE1, SIX_LINE2, SIX_PROD2, SIX_ROUND, SIX_CSQR, SIX_CONJ, SIX_FROB, SIX_INV, SIX_FOLD = range(11)
PROBE_SIX_GUARD = 10          # H2V_PROBE_SIX_GUARD: groups' worth of preset records behind the last group


class SixCall:
    """What h2v_probe_six_call brought back.  parts: per group the 12 limb vectors (14 integers each) re, im of coefficients 0..5 as
    six_result yields them - for SIX_PROD2 the 8 vectors of slots 22..29.  ok: per group the inverter's flag (SIX_INV; else None).
    guard_clean: everything behind group n - 1, and every word of a record that the op does not write, is still the preset."""
    __slots__ = ("parts", "ok", "guard_clean")


def probe_six_call(op: int, a, b=None, pts=None, flags=None, lines=None, csqr_n: int = 0, device: int = 0) -> SixCall:
    """One six-lane engine call per group on raw limb vectors.  a: per group 12 vectors of 14 limbs; b: the same (SIX_MUL; the lines:
    vectors 0..7 are the T slots, the rest is ignored); pts: per group 4 vectors PX1, PY1, PX2, PY2; flags: per group bit 0 skip1,
    bit 1 skip2; lines: 8 vectors [A0, A1, B0, B1] of loop 1, then loop 2, for the whole launch.  Arguments go to the library as they
    are given: what an op needs and does not get is the library's H2V_E_ARG."""
    n = len(a)

    def pack(groups, per_group):
        if groups is None:
            return None
        flat = [l for g in groups for v in g for l in v]
        assert len(flat) == len(groups) * per_group * 14
        return (C.c_uint32 * len(flat))(*flat)

    cap = n + PROBE_SIX_GUARD
    out = (C.c_uint32 * (cap * 168))()
    ok = (C.c_uint32 * cap)()
    check(lib().h2v_probe_six_call(device, op, n, csqr_n, pack(a, 12), pack(b, 12), pack(pts, 4),
                                   (C.c_uint32 * n)(*flags) if flags is not None else None, pack([lines], 8) if lines is not None else None, out, ok))
    r = SixCall()
    n_vec = 8 if op == SIX_PROD2 else 12
    r.parts = [[list(out[168 * i + 14 * j:168 * i + 14 * j + 14]) for j in range(n_vec)] for i in range(n)]
    r.ok = [int(ok[i]) for i in range(n)] if op == SIX_INV else None
    preset = 0xa5a5a5a5
    r.guard_clean = (all(v == preset for v in out[168 * n:]) and all(v == preset for v in ok[n:]) and
                     all(out[168 * i + q] == preset for i in range(n) for q in range(14 * n_vec, 168)) and
                     (op == SIX_INV or all(v == preset for v in ok[:n])))
    return r


# h2v_probe_coop_call: engine shapes and ops (csrc/h2v_pairing_coop.hpp: COOP_PROBE_*)
COOP_ENGINES = {"normal": 0, "wide": 1, "narrow": 2, "twelve": 3}
COOP_MUL, COOP_SQR, COOP_CSQR, COOP_LINE1, COOP_LINE2, COOP_PROD, COOP_ROUND, COOP_CONJ, COOP_FROB, COOP_INV = range(10)
PROBE_COOP_GUARD = 5          # H2V_PROBE_COOP_GUARD: groups' worth of preset records behind the last group


class CoopCall:
    """What h2v_probe_coop_call brought back.  parts: per group the 12 limb vectors (14 integers each) of the call's result, flat order
    2k + part - for COOP_PROD the 8 vectors of the slots T1, T2.  spare: per group the four T slots the spare lanes wrote (the line
    ops and COOP_ROUND of the shapes that have spare lanes; else None).  ok: per group the inverter's flag (1 for every other op).
    lanes_agree: per group, every lane of each pair or quad returned the same limbs.  guard_clean: everything behind group n - 1,
    and every word of a record that the op does not write, is still the preset."""
    __slots__ = ("parts", "spare", "ok", "lanes_agree", "guard_clean")


def probe_coop_call(engine: str, op: int, a, b=None, pts=None, flags=None, lines=None, csqr_n: int = 0, device: int = 0) -> CoopCall:
    """One cooperative-engine call per group on raw limb vectors.  a: per group 12 vectors of 14 limbs; b: the same (COOP_MUL; the line
    ops: vectors 0..3 are the loop's T slots, the rest is ignored); pts: per group 4 vectors PX1, PY1, PX2, PY2; flags: per group bit 0
    skip1, bit 1 skip2; lines: 4 lines of 8 vectors - loop 1's lines 0 and 1, then loop 2's - for the whole launch.  Arguments go to
    the library as they are given: what an op needs and does not get is the library's H2V_E_ARG."""
    n = len(a)

    def pack(groups, per_group):
        if groups is None:
            return None
        flat = [l for g in groups for v in g for l in v]
        assert len(flat) == len(groups) * per_group * 14
        return (C.c_uint32 * len(flat))(*flat)

    cap = n + PROBE_COOP_GUARD
    out = (C.c_uint32 * (cap * 224))()
    ok = (C.c_uint32 * (cap * 2))()
    check(lib().h2v_probe_coop_call(device, COOP_ENGINES[engine], op, n, csqr_n, pack(a, 12), pack(b, 12), pack(pts, 4),
                                    (C.c_uint32 * n)(*flags) if flags is not None else None,
                                    pack([[v for line in lines for v in line]], 32) if lines is not None else None, out, ok))
    r = CoopCall()
    has_spare = op in (COOP_LINE1, COOP_LINE2, COOP_ROUND) and engine != "twelve"
    n_vec = 8 if op == COOP_PROD else 16 if has_spare else 12
    vec = lambda i, j: list(out[224 * i + 14 * j:224 * i + 14 * j + 14])
    r.parts = [[vec(i, j) for j in range(min(n_vec, 12))] for i in range(n)]
    r.spare = [[vec(i, j) for j in range(12, 16)] for i in range(n)] if has_spare else None
    r.ok = [int(ok[2 * i]) for i in range(n)]
    r.lanes_agree = [int(ok[2 * i + 1]) == 1 for i in range(n)]
    preset = 0xa5a5a5a5
    r.guard_clean = (all(v == preset for v in out[224 * n:]) and all(v == preset for v in ok[2 * n:]) and
                     all(out[224 * i + q] == preset for i in range(n) for q in range(14 * n_vec, 224)))
    return r


def probe_quad_madd(p_xy, q_xy, neg: bool, device: int = 0):
    """2P + (-)Q as Jacobian (X, Y, Z) integers: [one-lane result, quad lane 0, 1, 2, 3] (h2v_probe_quad_madd)."""
    def limbs(v):
        return [(v >> (32 * i)) & 0xffffffff for i in range(12)]
    pq = (C.c_uint32 * 48)(*(limbs(p_xy[0]) + limbs(p_xy[1]) + limbs(q_xy[0]) + limbs(q_xy[1])))
    out = (C.c_uint32 * 210)()
    check(lib().h2v_probe_quad_madd(device, pq, 1 if neg else 0, out))
    from . import bls12_381 as bls
    rinv = pow(1 << 392, -1, bls.P)

    def val(o):
        return sum(out[o + k] << (28 * k) for k in range(14)) * rinv % bls.P
    return [(val(42 * j), val(42 * j + 14), val(42 * j + 28)) for j in range(5)]


def probe_g1_msm_pippenger(scalars, bases_compressed, device: int = 0):
    """sum_n s_n * B_n through the bucket MSM (scalars: ints < r; bases: 48-byte compressed)."""
    n = len(scalars)
    sc = b"".join(int(s).to_bytes(32, "little") for s in scalars)
    out = C.create_string_buffer(96)
    check(lib().h2v_probe_g1_msm_pippenger(device, n, sc, b"".join(bases_compressed), out))
    return _unxy(out.raw)


PIP_DUMP_DWORDS = 20514   # H2V_PIP_DUMP_DWORDS


def probe_g1_msm_pippenger_ex(problems, acc_grid_cap: int = 0, dump: bool = False, device: int = 0):
    """h2v_probe_g1_msm_pippenger_ex: 1 or 2 bucket MSMs side by side in the same launches.  Each problem is a dict with
    scalars (ints), points (48-byte compressed: the pool), and optionally halves (2), n_pool0 (the pool size: one pool) and pidx
    (None: the identity map).  Returns one (sum, dump) per problem: the affine sum or None, and - with dump=True - a dict with
    the launcher's shape c, W, NB, chain, the accumulate grid acc_blocks, and cls, off, order as k_pip_scan wrote them."""
    recs = (PipProbe * len(problems))()
    keep = []
    for r, p in zip(recs, problems):
        scalars, points, pidx = p["scalars"], p["points"], p.get("pidx")
        r.n, r.halves = len(scalars), p.get("halves", 2)
        r.scalars = b"".join(int(s).to_bytes(32, "little") for s in scalars)
        r.n_points = len(points)
        r.n_pool0 = len(points) if p.get("n_pool0") is None else p["n_pool0"]
        r.points_compressed = b"".join(points)
        out = C.create_string_buffer(96)
        idx = None if pidx is None else (C.c_uint32 * len(pidx))(*pidx)
        if pidx is not None and len(pidx) != len(scalars):
            raise ValueError("one point index per scalar")
        dmp = (C.c_uint32 * PIP_DUMP_DWORDS)() if dump else None
        r.pidx = idx if idx is not None else C.POINTER(C.c_uint32)()
        r.out_xy_be = C.cast(out, C.c_void_p)
        r.dump = dmp if dmp is not None else C.POINTER(C.c_uint32)()
        keep.append((out, idx, dmp))
    check(lib().h2v_probe_g1_msm_pippenger_ex(device, len(problems), recs, acc_grid_cap))
    res = []
    for out, _, dmp in keep:
        d = None
        if dmp is not None:
            c, W, NB, chain, blocks = dmp[0:5]
            nb = W * NB
            d = {"c": c, "W": W, "NB": NB, "chain": chain, "acc_blocks": blocks, "cls": list(dmp[5:33]),
                 "off": list(dmp[33:33 + nb + 1]), "order": list(dmp[34 + nb:34 + 2 * nb])}
        res.append((_unxy(out.raw), d))
    return res


def probe_pairing(plan: DevicePlan, p1_list, p2_list):
    n = len(p1_list)
    out = C.create_string_buffer(n)
    check(lib().h2v_probe_pairing(plan.handle, n, b"".join(p1_list), b"".join(p2_list), out))
    return [out.raw[i] for i in range(n)]


def probe_pairing_ex(plan: DevicePlan, p1_list, p2_list, impl: int, dump: bool = True):
    """returns (accept list, per proof [f_miller (12 ints), f_final (12 ints)]) with the chosen kernel"""
    n = len(p1_list)
    out = C.create_string_buffer(n)
    dbg = C.create_string_buffer(n * 24 * 48) if dump else None
    check(lib().h2v_probe_pairing_ex(plan.handle, n, b"".join(p1_list), b"".join(p2_list), out, impl, dbg))
    vals = []
    if dump:
        for i in range(n):
            row = [int.from_bytes(dbg.raw[(i * 24 + q) * 48:(i * 24 + q + 1) * 48], "little") for q in range(24)]
            vals.append((row[:12], row[12:]))
    return [out.raw[i] for i in range(n)], vals


PROBE_PAIRING_GUARD = 64      # H2V_PROBE_PAIRING_GUARD: proofs' worth of preset records behind the batch


def g1_jacobian_limbs(pt, z: int = 1) -> bytes:
    """The 36 dwords X, Y, Z (h2v_probe_pairing_states: el_jac_in) of the affine point pt = (x, y) scaled to the Jacobian
    representative with the chosen Z != 0 mod p: (x Z^2, y Z^3, Z), each as bls12_381.fp_mont_bytes has it (the kernels' Montgomery
    form, R = 2^392, 12 little-endian 32-bit limbs).  pt None: infinity as g1j_set_inf writes it, (1, 1, 0)."""
    from . import bls12_381 as bls
    if pt is None:
        return bls.fp_mont_bytes(1) + bls.fp_mont_bytes(1) + bls.fp_mont_bytes(0)
    if z % bls.P == 0:
        raise ValueError("Z = 0 is infinity")
    x, y = pt
    return bls.fp_mont_bytes(x * z * z) + bls.fp_mont_bytes(y * z * z * z) + bls.fp_mont_bytes(z)


class PairingStates:
    """What h2v_probe_pairing_states brought back.  accept / status / values: per proof (values: (Miller, final), 12 integers each,
    None where the kernel left all 24 records at the preset; a record partly written is given as the integers it holds).  guard_clean:
    every byte behind proof n - 1 of all three outputs is still the preset.  lanes: the engine that ran, in lanes per proof."""
    __slots__ = ("accept", "status", "values", "guard_clean", "lanes")


def probe_pairing_states(plan: DevicePlan, p1_list, p2_list, impl: int, status_in=None, valid_sub_in=None, el_jac_in=None) -> PairingStates:
    """status_in: n integers; valid_sub_in: n pairs (slot p1, slot p2) of 0 / 1; el_jac_in: n byte strings from g1_jacobian_limbs.
    Each may be None (the pipelines' plain first launch)."""
    n = len(p1_list)
    cap = n + PROBE_PAIRING_GUARD
    if len(p2_list) != n or any(v is not None and len(v) != n for v in (status_in, valid_sub_in, el_jac_in)):
        raise ValueError("one entry per proof")
    st_in = (C.c_uint32 * n)(*status_in) if status_in is not None else None
    sub_in = bytes(b for pair in valid_sub_in for b in pair) if valid_sub_in is not None else None
    el_in = b"".join(el_jac_in) if el_jac_in is not None else None
    if el_in is not None and len(el_in) != n * 144:
        raise ValueError("el_jac_in: 144 bytes per proof")
    st_out = (C.c_uint32 * cap)()
    acc = C.create_string_buffer(cap)
    dbg = C.create_string_buffer(cap * 24 * 48)
    lanes = C.c_uint32(0)
    check(lib().h2v_probe_pairing_states(plan.handle, n, b"".join(p1_list), b"".join(p2_list), impl, st_in, sub_in, el_in,
                                         st_out, acc, dbg, C.byref(lanes)))
    raw, preset = dbg.raw, b"\xa5" * (24 * 48)
    r = PairingStates()
    r.accept = [acc.raw[i] for i in range(n)]
    r.status = [st_out[i] for i in range(n)]
    r.values = []
    for i in range(n):
        rec = raw[i * 24 * 48:(i + 1) * 24 * 48]
        if rec == preset:
            r.values.append(None)
            continue
        row = [int.from_bytes(rec[q * 48:(q + 1) * 48], "little") for q in range(24)]
        r.values.append((row[:12], row[12:]))
    r.guard_clean = (raw[n * 24 * 48:] == b"\xa5" * (PROBE_PAIRING_GUARD * 24 * 48) and acc.raw[n:cap] == b"\xa5" * PROBE_PAIRING_GUARD
                     and all(st_out[i] == 0xa5a5a5a5 for i in range(n, cap)))
    r.lanes = lanes.value
    return r
