"""ctypes binding of libquits_amd.so (include/quits_amd.h).

There is no CPU fallback: if the HIP library is missing or no MI355X is visible, construction of any decoder
raises.  (The CPU restatement under oracle/ is test infrastructure and is never imported from here.)
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("QUITS_AMD_LIB", os.path.join(_HERE, "lib", "libquits_amd.so"))

QD_BP = {"product_sum": 0, "ps": 0, "prod_sum": 0, "minimum_sum": 1, "min_sum": 1, "ms": 1, 0: 0, 1: 1}
QD_SCHEDULE = {"parallel": 0, "p": 0, "serial": 1, "s": 1, 0: 0, 1: 1}
QD_OSD = {"osd_off": 0, "off": 0, "osd_0": 1, "osd0": 1, "osd_e": 2, "osde": 2, "exhaustive": 2,
          "osd_cs": 3, "osdcs": 3, "combination_sweep": 3, "lsd_0": 4, "lsd_e": 5, "lsd_cs": 6, 0: 0, 1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 6}

STATUS_ITER_MASK = 0x3FFF
STATUS_COARSE_GRID = 1 << 14
STATUS_INEXACT = 1 << 15
STATUS_CONVERGED = 1 << 16
STATUS_OSD = 1 << 17
STATUS_INCONSISTENT = 1 << 18
STATUS_ZERO = 1 << 19
STATUS_RELAY_LEG_SHIFT = 20                                             # Relay-BP: bits 20..29 = the leg of the returned candidate
STATUS_RELAY_LEG_MASK = 0x3FF << STATUS_RELAY_LEG_SHIFT
SHOT_POST, SHOT_INCONSISTENT, SHOT_INEXACT, SHOT_COARSE = 1, 2, 4, 8     # QD_SHOT_*: the flag byte qd_shot_flags_fold keeps per shot
SHOT_FLAG_NAMES = ("post", "inconsistent", "inexact", "coarse")         # ... bit j <-> name j
TALLY_HEAD = 10                                                         # QD_TALLY_HEAD
FAULT_HIST = 256                                                        # QD_FAULT_HIST
RELAY_FLAG_MARGINALS_DEVICE = 1                                         # QD_RELAY_FLAG_MARGINALS_DEVICE (qd_relay_params.reserved)
SHRINK_STATE = 8                                                        # QD_SHRINK_STATE
SHRINK_FAILS, SHRINK_MINIMAL, SHRINK_ENDED = 1, 2, 4                    # QD_SHRINK_*: the flag word of a parent's state
SOFT_FIELDS, SOFT_BINS = 6, 1024                                        # QD_SOFT_FIELDS, QD_SOFT_BINS
QD_ECAPACITY = -4                                                       # a model beyond a kernel's limits


class QdParams(C.Structure):
    _fields_ = [("bp_method", C.c_int32), ("schedule", C.c_int32), ("max_iter", C.c_int32),
                ("osd_method", C.c_int32), ("osd_order", C.c_int32), ("reserved", C.c_int32),
                ("ms_scaling_factor", C.c_double)]


class QdRelayParams(C.Structure):
    _fields_ = [("pre_iter", C.c_int32), ("num_sets", C.c_int32), ("set_max_iter", C.c_int32), ("stop_nconv", C.c_int32),
                ("gamma0", C.c_float), ("reserved", C.c_int32)]


class QdError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libquits_amd error %d: %s" % (code, msg))
        self.code = code


_lib = None

EXPORTS = [
    "qd_version", "qd_last_error", "qd_device_count", "qd_graph_create", "qd_graph_destroy", "qd_graph_info", "qd_graph_info_ex",
    "qd_decoder_create", "qd_decoder_info", "qd_decoder_fast_start", "qd_decoder_postproc_kernel", "qd_decoder_destroy", "qd_decoder_reserve", "qd_decoder_set_workspace_limit", "qd_decoder_release_workspace", "qd_decode_batch", "qd_decode_stage", "qd_osd0_batch", "qd_decoder_failed_llr",
    "qd_decoder_set_profiling", "qd_decoder_profile", "qd_decoder_post_head_start", "qd_decoder_debug_counters", "qd_spmat_create", "qd_spmat_destroy", "qd_gf2_spmv_batch",
    "qd_unpack_bits", "qd_count_mismatch", "qd_sample_dem",
    "qd_circuit_create", "qd_circuit_destroy", "qd_circuit_info", "qd_sample_circuit",
    "qd_shot_flags_fold", "qd_tally_batch", "qd_sample_circuit_shots", "qd_sample_dem_shots",
    "qd_unpack_b8", "qd_pack_b8",
    "qd_sample_dem_faults", "qd_commit_bits", "qd_fault_stats_batch",
    "qd_strata_create", "qd_strata_destroy", "qd_strata_info", "qd_sample_dem_strata",
    "qd_decoder_create_relay", "qd_decoder_relay_info",
    "qd_shrink_begin", "qd_shrink_step",
    "qd_search_create", "qd_search_destroy", "qd_search_reset", "qd_search_seed", "qd_search_level", "qd_search_counters", "qd_search_found",
    "qd_search_chain",
    "qd_soft_fold", "qd_soft_weigh", "qd_soft_tally",
    "qd_isd_create", "qd_isd_destroy", "qd_isd_info", "qd_isd_run", "qd_isd_hist", "qd_isd_reset",
    "qd_bit_planes", "qd_calib_create", "qd_calib_destroy", "qd_calib_info", "qd_parity_counts",
]


def load():
    """Load the shared library (no GPU needed for this step)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "quits_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback." % LIB_PATH)
    # One HIP runtime per process: PyTorch ships its own libamdhip64 and this library links the system one by the same
    # SONAME.  Whichever is loaded first serves both; loading this library first and torch afterwards leaves two runtimes, and
    # the second one sees no device.  So torch (the owner of device memory and streams on this path) goes first.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
    L.qd_version.restype = C.c_int
    if L.qd_version() < 104:              # 104: the circuit sampler; 103: qd_decoder_post_head_start (the pipelined driver); 102: qd_graph_info_ex
        raise RuntimeError("quits_amd: %s is version %d, this package needs >= 104 -- rebuild it (`python -c 'import __graft_entry__ as g; g.build()'`)"
                           % (LIB_PATH, L.qd_version()))
    L.qd_last_error.restype = C.c_char_p
    L.qd_device_count.restype = C.c_int
    L.qd_graph_create.argtypes = [i32, i32, vp, vp, vp, i32, C.POINTER(vp)]
    L.qd_graph_destroy.argtypes = [vp]
    L.qd_graph_destroy.restype = None
    L.qd_graph_info.argtypes = [vp, vp]
    L.qd_graph_info_ex.argtypes = [vp, vp, i32]
    L.qd_decoder_create.argtypes = [vp, C.POINTER(QdParams), C.POINTER(vp)]
    L.qd_decoder_info.argtypes = [vp, vp]
    L.qd_decoder_postproc_kernel.argtypes = [vp]
    if hasattr(L, "qd_decoder_fast_start"):         # (library version 105; a 104 library named by QUITS_AMD_LIB has no fast start to report)
        L.qd_decoder_fast_start.argtypes = [vp]
        L.qd_decoder_fast_start.restype = C.c_int
    L.qd_decoder_postproc_kernel.restype = C.c_int
    L.qd_decoder_destroy.argtypes = [vp]
    L.qd_decoder_destroy.restype = None
    L.qd_decoder_reserve.argtypes = [vp, i64]
    L.qd_decoder_set_workspace_limit.argtypes = [vp, i64]
    L.qd_decoder_release_workspace.argtypes = [vp]
    L.qd_decode_batch.argtypes = [vp, vp, i64, i64, vp, i64, i32, i64, vp, vp, vp]
    L.qd_decode_stage.argtypes = [vp, vp, i64, i64, vp, i64, i32, i64, vp, vp, i32, vp]
    L.qd_osd0_batch.argtypes = [vp, vp, i64, i64, vp, i64, i32, i64, vp, vp, vp, vp]
    L.qd_decoder_failed_llr.argtypes = [vp, i64, vp, vp]
    L.qd_decoder_set_profiling.argtypes = [vp, i32]
    L.qd_decoder_post_head_start.argtypes = [vp, i32, vp]
    L.qd_decoder_profile.argtypes = [vp, vp, i32]
    L.qd_decoder_debug_counters.argtypes = [vp, vp]
    L.qd_spmat_create.argtypes = [i32, i32, vp, vp, i32, C.POINTER(vp)]
    L.qd_spmat_destroy.argtypes = [vp]
    L.qd_spmat_destroy.restype = None
    L.qd_gf2_spmv_batch.argtypes = [vp, vp, i64, i64, vp, i64, i32, vp]
    L.qd_unpack_bits.argtypes = [vp, i64, i32, i64, vp, i64, vp]
    L.qd_count_mismatch.argtypes = [vp, vp, i32, i64, vp, vp]
    L.qd_sample_dem.argtypes = [vp, vp, vp, u64, i64, i64, vp, i64, vp, i64, vp]
    L.qd_circuit_create.argtypes = [vp, i64, i32, i32, i32, i32, vp, i32, i32, i32, C.POINTER(vp)]
    L.qd_circuit_destroy.argtypes = [vp]
    L.qd_circuit_destroy.restype = None
    L.qd_circuit_info.argtypes = [vp, vp]
    L.qd_sample_circuit.argtypes = [vp, u64, i64, i64, vp, i64, vp, i64, vp]
    if hasattr(L, "qd_tally_batch"):                # (library version 108; an older library named by QUITS_AMD_LIB samples and decodes as before)
        L.qd_shot_flags_fold.argtypes = [vp, i64, vp, vp]
        L.qd_tally_batch.argtypes = [vp, i64, vp, i64, i32, i64, vp, vp, vp, vp]
        L.qd_sample_circuit_shots.argtypes = [vp, u64, vp, i64, vp, i64, vp, i64, vp]
        L.qd_sample_dem_shots.argtypes = [vp, vp, vp, u64, vp, i64, vp, i64, vp, i64, vp]
    if hasattr(L, "qd_unpack_b8"):                  # (library version 109; an older library named by QUITS_AMD_LIB takes unpacked samples as before)
        L.qd_unpack_b8.argtypes = [vp, i64, i64, i32, i64, vp, i64, vp]
        L.qd_pack_b8.argtypes = [vp, i64, i32, i64, vp, i64, vp]
    if hasattr(L, "qd_commit_bits"):                # (library version 110; an older library named by QUITS_AMD_LIB returns logical predictions as before)
        L.qd_sample_dem_faults.argtypes = [vp, vp, vp, u64, i64, vp, i64, vp, i64, vp, i64, vp, i64, vp]
        L.qd_commit_bits.argtypes = [vp, i64, i32, i64, vp, i64, i64, vp]
        L.qd_fault_stats_batch.argtypes = [vp, vp, i64, i32, vp, i64, i32, vp, i64, i64, vp, vp, vp, vp]
    if hasattr(L, "qd_strata_create"):              # (library version 111; an older library named by QUITS_AMD_LIB samples independent faults as before)
        L.qd_strata_create.argtypes = [i32, i32, vp, i32, C.POINTER(vp)]
        L.qd_strata_destroy.argtypes = [vp]
        L.qd_strata_destroy.restype = None
        L.qd_strata_info.argtypes = [vp, vp]
        L.qd_sample_dem_strata.argtypes = [vp, vp, vp, u64, i64, vp, vp, i64, vp, i64, vp, i64, vp, i64, vp]
    if hasattr(L, "qd_decoder_create_relay"):       # (library version 112; an older library named by QUITS_AMD_LIB decodes with BP + OSD / LSD as before)
        L.qd_decoder_create_relay.argtypes = [vp, C.POINTER(QdParams), C.POINTER(QdRelayParams), vp, C.POINTER(vp)]
    if hasattr(L, "qd_decoder_relay_info"):         # (library version 113; an older library named by QUITS_AMD_LIB keeps every Relay-BP decoder's marginals in LDS)
        L.qd_decoder_relay_info.argtypes = [vp, vp]
    if hasattr(L, "qd_shrink_begin"):               # (library version 114; an older library named by QUITS_AMD_LIB samples and decodes as before)
        L.qd_shrink_begin.argtypes = [vp, vp, vp, i64, i64, vp, vp, vp, vp, i64, vp, i64, vp, i64, vp, i64, vp, vp, vp]
        L.qd_shrink_step.argtypes = [vp, vp, vp, i64, i64, vp, vp, i64, vp, vp, vp, vp, i64, vp, i64, vp, i64, vp, i64, vp, vp, vp]
    if hasattr(L, "qd_search_create"):              # (library version 115; an older library named by QUITS_AMD_LIB samples and decodes as before)
        L.qd_search_create.argtypes = [i32, i32, vp, vp, vp, vp, i32, i32, i32, i64, i64, i64, i32, C.POINTER(vp)]
        L.qd_search_destroy.argtypes = [vp]
        L.qd_search_destroy.restype = None
        L.qd_search_reset.argtypes = [vp]
        L.qd_search_seed.argtypes = [vp, vp, i64, vp]
        L.qd_search_level.argtypes = [vp, i64, vp]
        L.qd_search_counters.argtypes = [vp, vp]
        L.qd_search_found.argtypes = [vp, i64, vp, vp]
        L.qd_search_chain.argtypes = [vp, C.c_uint32, i32, vp, C.POINTER(i32)]
    if hasattr(L, "qd_soft_fold"):                  # (library version 116; an older library named by QUITS_AMD_LIB returns predictions and corrections as before)
        L.qd_soft_fold.argtypes = [vp, i64, vp, i64, vp]
        L.qd_soft_weigh.argtypes = [vp, i64, i32, vp, vp, i64, i32, i64, vp, i64, vp]
        L.qd_soft_tally.argtypes = [vp, i64, i64, vp, vp, vp, vp]
    if hasattr(L, "qd_isd_create"):                 # (library version 117; an older library named by QUITS_AMD_LIB samples, decodes and searches as before)
        L.qd_isd_create.argtypes = [i32, i32, vp, vp, vp, i32, C.POINTER(vp)]
        L.qd_isd_destroy.argtypes = [vp]
        L.qd_isd_destroy.restype = None
        L.qd_isd_info.argtypes = [vp, vp]
        L.qd_isd_run.argtypes = [vp, u64, i64, i64, vp, vp]
        L.qd_isd_hist.argtypes = [vp, vp]
        L.qd_isd_reset.argtypes = [vp]
    if hasattr(L, "qd_calib_create"):               # (library version 118; an older library named by QUITS_AMD_LIB keeps the model's own priors as before)
        L.qd_bit_planes.argtypes = [vp, i64, i32, i64, vp, i64, vp]
        L.qd_calib_create.argtypes = [i32, i32, vp, vp, i32, C.POINTER(vp)]
        L.qd_calib_destroy.argtypes = [vp]
        L.qd_calib_destroy.restype = None
        L.qd_calib_info.argtypes = [vp, vp]
        L.qd_parity_counts.argtypes = [vp, vp, i64, i64, vp, vp]
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise QdError(rc, load().qd_last_error().decode(errors="replace"))


# One row per group of entry points newer than the oldest library load() accepts: the suffix of require_<suffix>, the symbol whose presence
# stands for the group, the library version that brought it, and what needs it (the subject and verb of the error message).
ENTRY_POINT_GROUPS = (
    ("experiment", "qd_tally_batch", 108, "the device-resident memory experiment needs"),
    ("bitpack", "qd_unpack_b8", 109, "bit-packed samples need"),
    ("faults", "qd_commit_bits", 110, "fault-level outputs need"),
    ("strata", "qd_strata_create", 111, "stratified sampling needs"),
    ("relay", "qd_decoder_create_relay", 112, "Relay-BP needs"),
    ("relay_forms", "qd_decoder_relay_info", 113, "choosing where Relay-BP keeps its marginals needs"),
    ("shrink", "qd_shrink_begin", 114, "shrinking fault sets needs"),
    ("search", "qd_search_create", 115, "the logical-fault search needs"),
    ("soft", "qd_soft_fold", 116, "soft outputs need"),
    ("distance", "qd_isd_create", 117, "the distance estimate needs"),
    ("calibrate", "qd_calib_create", 118, "fitting priors needs"),
)


def _require(suffix, probe, version, phrase):
    def require(L):
        if not hasattr(L, probe):
            raise RuntimeError("quits_amd: %s is version %d; %s >= %d -- rebuild it" % (LIB_PATH, L.qd_version(), phrase, version))
        return L
    require.__name__ = require.__qualname__ = "require_" + suffix
    require.__doc__ = "`L`, if it has the entry points of library version %d (%s): a clear error from an older library." % (version, probe)
    return require


# require_experiment(L), require_bitpack(L), ..., require_calibrate(L)
for _row in ENTRY_POINT_GROUPS:
    globals()["require_" + _row[0]] = _require(*_row)


def require_gpu():
    """Fail loudly when the device path cannot run (no silent CPU fallback)."""
    L = load()
    import torch
    if not torch.cuda.is_available() or L.qd_device_count() < 1:
        raise RuntimeError("quits_amd: no HIP device visible; the decoder has no CPU fallback "
                           "(the CPU restatement lives in oracle/ and is test infrastructure only)")
    return L
