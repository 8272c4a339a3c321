"""ctypes mirror of include/hypo_gpu.h (structs and constants only; no library is loaded here).

Reference types mirrored: ScoreParams (include/globalDefs.hpp:58-66), hypo::Window data members
(include/Window.hpp:123-135).
"""
import ctypes as C

ABI_VERSION = 11

HYPO_OK = 0
HYPO_E_INVALID = -1
HYPO_E_NODEVICE = -2
HYPO_E_HIP = -3
HYPO_E_WORKSPACE = -4
HYPO_E_NOTINIT = -5
HYPO_E_CAPACITY = -6
HYPO_E_UNSUPPORTED = -7

# hypo_gpu_kset_query_track: what hypo_amd.capi puts into the interval arrays before a call (no position or count is that large)
TRACK_UNTOUCHED = 0xFFFFFFFFFFFFFFFF

# hypo_gpu_kset_query_fixes (HYPO_KSET_MAX_FIX_REGION, HYPO_KSET_MAX_FIX_SPAN); hypo_amd.capi fills the outputs with the sentinels
# before a call (no count and no candidate index is that large)
KSET_MAX_FIX_REGION = 31
KSET_MAX_FIX_SPAN = 2048
FIXES_UNTOUCHED64 = 0xFFFFFFFFFFFFFFFF
FIXES_UNTOUCHED32 = 0xFFFFFFFF

# hypo_gpu_kset_query_walks (HYPO_KSET_MAX_WALK, HYPO_KSET_MAX_WALK_BUDGET, HYPO_WALK_*); hypo_amd.capi fills the outputs with the
# sentinels before a call (no status, step count or length is that large, and no base is that byte)
KSET_MAX_WALK = 256
KSET_MAX_WALK_BUDGET = 65536
WALK_NONE, WALK_UNIQUE, WALK_AMBIGUOUS, WALK_BUDGET, WALK_NOANCHOR = 0, 1, 2, 3, 4
WALKS_UNTOUCHED32 = 0xFFFFFFFF
WALKS_UNTOUCHED8 = 0xFF
# hypo_gpu_kset_query_walk_sets (HYPO_KSET_MAX_WALKS, HYPO_WALK_MANY); the sentinels are those above
KSET_MAX_WALKS = 4
WALK_MANY = 5

# hypo_gpu_kset_counts_enable / _mark / _spectrum (HYPO_KSET_MAX_TEXTS, HYPO_KSET_SPECTRUM_BINS): hist[count * 5 + min(copies, 4)]
KSET_MAX_TEXTS = 4
KSET_SPECTRUM_ROWS, KSET_SPECTRUM_COLS = 256, 5
KSET_SPECTRUM_BINS = KSET_SPECTRUM_ROWS * KSET_SPECTRUM_COLS

# hypo_gpu_kset_query_depth (HYPO_KSET_DEPTH_MIN_BIN, HYPO_KSET_DEPTH_MAX_BIN); hypo_amd.capi fills the outputs with the sentinels
# before a call (no bin has that many windows; a median of 255 is possible, so a test that looks for untouched bytes uses the u32 arrays)
KSET_DEPTH_MIN_BIN, KSET_DEPTH_MAX_BIN = 32, 65536
DEPTH_UNTOUCHED32 = 0xFFFFFFFF
DEPTH_UNTOUCHED8 = 0xFF

# hypo_gpu_kset_export / _import (HYPO_KSET_EXPORT_END): the cursor a finished export sequence leaves
KSET_EXPORT_END = 0xFFFFFFFFFFFFFFFF

ST_OK = 0
ST_CONS_OVERFLOW = 1
ST_CAPACITY = 2
ST_UNDEFINED = 3
ST_INVALID = 4

WIN_SHORT = 0
WIN_LONG = 1


class ScoreParams(C.Structure):
    _fields_ = [("sr_match", C.c_int8), ("sr_mismatch", C.c_int8), ("sr_gap", C.c_int8),
                ("lr_match", C.c_int8), ("lr_mismatch", C.c_int8), ("lr_gap", C.c_int8)]


# reference defaults: src/main.cpp:100-113
DEFAULT_SCORES = (5, -4, -8, 3, -5, -4)


class Window(C.Structure):
    _fields_ = [("type", C.c_uint8), ("reserved", C.c_uint8 * 3), ("draft_len", C.c_uint32),
                ("draft_off", C.c_uint64), ("first_arm", C.c_uint32), ("n_internal", C.c_uint32),
                ("n_prefix", C.c_uint32), ("n_suffix", C.c_uint32), ("n_empty", C.c_uint32),
                ("reserved2", C.c_uint32)]


assert C.sizeof(Window) == 40


class WindowBatch(C.Structure):
    _fields_ = [("n_windows", C.c_uint32), ("n_arms", C.c_uint32), ("windows", C.c_void_p),
                ("draft4", C.c_void_p), ("draft4_bytes", C.c_uint64), ("arm_off", C.c_void_p),
                ("arm_len", C.c_void_p), ("arms2", C.c_void_p), ("arms2_bytes", C.c_uint64)]


class ConsensusBatch(C.Structure):
    _fields_ = [("bases", C.c_void_p), ("off", C.c_void_p), ("len", C.c_void_p),
                ("status", C.c_void_p)]


class PoaStats(C.Structure):
    _fields_ = [("n_windows", C.c_uint64), ("n_trivial", C.c_uint64), ("n_class", C.c_uint64 * 8),
                ("n_escalated", C.c_uint64), ("n_failed", C.c_uint64), ("dp_cells", C.c_uint64),
                ("n_alignments", C.c_uint64), ("alg_bytes", C.c_uint64 * 8),
                ("n_reused", C.c_uint64), ("n_threaded", C.c_uint64), ("cells_scored", C.c_uint64),
                ("cells_threaded", C.c_uint64), ("n_carried", C.c_uint64)]


class EditBatch(C.Structure):
    _fields_ = [("n_pairs", C.c_uint32), ("_pad", C.c_uint32), ("a", C.c_void_p), ("a_off", C.c_void_p),
                ("b", C.c_void_p), ("b_off", C.c_void_p)]


# numpy dtype equivalent of HypoWindow (40 bytes, same offsets)
import numpy as _np

WINDOW_DTYPE = _np.dtype({
    "names": ["type", "draft_len", "draft_off", "first_arm", "n_internal", "n_prefix", "n_suffix",
              "n_empty"],
    "formats": ["u1", "<u4", "<u8", "<u4", "<u4", "<u4", "<u4", "<u4"],
    "offsets": [0, 4, 8, 16, 20, 24, 28, 32],
    "itemsize": 40,
})
