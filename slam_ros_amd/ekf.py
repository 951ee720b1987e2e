"""Host-side mirror of the reference `class Robot` over the C-ABI of libslam_ekf.so.

`Robot` mirrors slam_ros/Robot.h:21-77 (constructor pose, `localize(lines, rot, encoder)`,
`getEllipse()`, `xPos/yPos/thetaPos`, `P_t0`, `lineIntervals`) and adds the two halves
`predict(encoder)` / `update(lines)`. `Ensemble` drives E independent
instances per call — the benchmark and multi-GPU path.

All arithmetic runs in the HIP kernels of libslam_ekf.so (gfx950). There is no CPU
fallback: if the library or a GPU is missing, constructing a context raises.
"""
from __future__ import annotations

import ctypes
import math
import os

import numpy as np

from . import build as _build

EKF_MAX_LINES = 64
PREC_F64, PREC_F32, PREC_F16 = 0, 1, 2
R_INTENDED, R_AS_WRITTEN = 0, 1
ARITH_EXACT, ARITH_BF16X6, ARITH_F16X3 = 0, 1, 2   # fp32 flush arithmetic (slam_ekf.h EKF_ARITH_*)
ST_SINGULAR_S, ST_CAPACITY, ST_NONSYM, ST_SYNC_TIMEOUT, ST_RANGE, ST_PRECISION = 1, 2, 4, 8, 16, 32
EXP_AUTO = -1000
# per-context options (slam_ekf.h EKF_OPT_*, ekf_set_option)
OPT_SPECULATE, OPT_SPIN_LOG2, OPT_FLUSH_FORM, OPT_FLUSH_BLOCKS_PER_CU = 1, 2, 3, 4
OPT_MFMA_REPLAY, OPT_SCAN_STAMPS, OPT_TEST_DROP_WG, OPT_TEST_VERDICT_TIMEOUT = 5, 6, 7, 8
OPT_ACTIVE_FLUSH, OPT_SCAN_THREADS = 9, 10
OPTIONS = {"speculate": OPT_SPECULATE, "spin_log2": OPT_SPIN_LOG2, "flush_form": OPT_FLUSH_FORM,
           "flush_blocks_per_cu": OPT_FLUSH_BLOCKS_PER_CU, "mfma_replay": OPT_MFMA_REPLAY,
           "scan_stamps": OPT_SCAN_STAMPS, "test_drop_wg": OPT_TEST_DROP_WG,
           "test_verdict_timeout": OPT_TEST_VERDICT_TIMEOUT, "active_flush": OPT_ACTIVE_FLUSH,
           "scan_threads": OPT_SCAN_THREADS}

LIB_PATH = _build.LIB_PATH

# symbols declared by include/slam_ekf.h (checked by tests/test_abi.py)
EXPORTED = [
    "ekf_config_init", "ekf_strerror", "ekf_abi_version", "ekf_create", "ekf_destroy",
    "ekf_set_stream", "ekf_sync", "ekf_set_option", "ekf_get_option", "ekf_reset_instance", "ekf_localize", "ekf_localize_device",
    "ekf_predict", "ekf_update", "ekf_read_results", "ekf_upload_state", "ekf_download_state",
    "ekf_init_lowrank", "ekf_storage_exponent", "ekf_rescale", "ekf_get_pose_cov", "ekf_get_ellipse", "ekf_ellipse_of_block",
    "ekf_query_joint", "ekf_query_marginals", "ekf_query_joint_device",
    "ekf_gate_lines", "ekf_gate_lines_device", "ekf_gate_joint", "ekf_gate_joint_device",
    "ekf_associate_joint", "ekf_associate_joint_device", "ekf_gate_landmarks", "ekf_gate_landmarks_device",
    "ekf_resample", "ekf_copy_instance",
    "ekf_gate_candidates_device", "ekf_assoc_weights_device", "ekf_resample_plan_device", "ekf_resample_device",
    "ekf_instance_image_bytes", "ekf_export_instances", "ekf_import_instances",
    "ekf_export_instances_device", "ekf_import_instances_device",
    "ekf_landmark_block_bytes",
    "ekf_state_dim", "ekf_profile_enable", "ekf_profile_read", "ekf_profile_flushes",
    "ekf_flush_kernel_name", "ekf_debug_scan_stamps", "ekf_debug_result_words",
    "ekf_shard_create", "ekf_shard_tiles", "ekf_shard_buffer_words", "ekf_shard_begin", "ekf_shard_line",
    "ekf_shard_apply", "ekf_shard_end", "ekf_shard_abort", "ekf_shard_spec_buffer_words",
    "ekf_shard_speculate", "ekf_shard_run", "ekf_shard_resume",
    "ekf_rccl_unique_id", "ekf_shard_attach_rccl", "ekf_shard_localize",
]


class EkfConfig(ctypes.Structure):
    _fields_ = [
        ("capacity", ctypes.c_int32), ("instances", ctypes.c_int32),
        ("precision", ctypes.c_int32), ("device", ctypes.c_int32),
        ("max_lines", ctypes.c_int32), ("r_mode", ctypes.c_int32),
        ("reset_margin", ctypes.c_int32), ("pipeline", ctypes.c_int32),
        ("flush_interval", ctypes.c_int32), ("arith", ctypes.c_int32),
        ("mahalanobis", ctypes.c_double), ("encoder_noise", ctypes.c_double),
    ]


class EkfLine(ctypes.Structure):
    _fields_ = [("alpha", ctypes.c_double), ("r", ctypes.c_double), ("R", ctypes.c_double * 4)]


class EkfResult(ctypes.Structure):
    _fields_ = [
        ("pose", ctypes.c_double * 3), ("matches", ctypes.c_int32),
        ("new_landmarks", ctypes.c_int32), ("saved", ctypes.c_int32),
        ("reset", ctypes.c_int32), ("status", ctypes.c_int32), ("nlines", ctypes.c_int32),
        ("match", ctypes.c_int32 * EKF_MAX_LINES),
    ]


class EkfGateHit(ctypes.Structure):
    """ekf_gate_hit (slam_ekf.h): one trial line against the map."""
    _fields_ = [
        ("first", ctypes.c_int32), ("nearest", ctypes.c_int32), ("npass", ctypes.c_int32),
        ("status", ctypes.c_int32), ("d2_first", ctypes.c_double), ("d2_nearest", ctypes.c_double),
        ("S", ctypes.c_double * 4), ("v", ctypes.c_double * 2),
    ]


ekf_gate_hit = EkfGateHit   # (the C name)


class EkfJointHit(ctypes.Structure):
    """ekf_joint_hit (slam_ekf.h): one hypothesis' stacked innovation against the map."""
    _fields_ = [
        ("m", ctypes.c_int32), ("status", ctypes.c_int32), ("d2", ctypes.c_double), ("logdet", ctypes.c_double),
    ]


ekf_joint_hit = EkfJointHit   # (the C name)

PH_FLIP_NEAREST, PH_FLIP_FIRST, PH_SINGULAR = 1, 2, 4   # ekf_pair_hit.status


class EkfPairHit(ctypes.Structure):
    """ekf_pair_hit (slam_ekf.h): one landmark against every other saved landmark."""
    _fields_ = [
        ("nearest", ctypes.c_int32), ("first", ctypes.c_int32), ("npass", ctypes.c_int32),
        ("status", ctypes.c_int32), ("d2_nearest", ctypes.c_double), ("d2_first", ctypes.c_double),
        ("C", ctypes.c_double * 3), ("delta", ctypes.c_double * 2),
    ]


ekf_pair_hit = EkfPairHit   # (the C name)
# the same record as a numpy structured type (Ensemble.gate_landmarks returns an array of it)
PAIR_HIT_DTYPE = np.dtype([("nearest", "<i4"), ("first", "<i4"), ("npass", "<i4"), ("status", "<i4"),
                           ("d2_nearest", "<f8"), ("d2_first", "<f8"), ("C", "<f8", (3,)), ("delta", "<f8", (2,))])

ASSOC_MAX_CAND, ASSOC_MAX_LINES, ASSOC_MAX_TOTAL, ASSOC_MAX_NODES = 8, 16, 64, 1 << 22
AS_TRUNCATED, AS_SINGULAR, AS_INVALID = 1, 2, 4   # ekf_assoc_hit.status


class EkfAssocHit(ctypes.Structure):
    """ekf_assoc_hit (slam_ekf.h): the best jointly compatible assignment of a scan's lines."""
    _fields_ = [
        ("m", ctypes.c_int32), ("status", ctypes.c_int32), ("nodes", ctypes.c_int32), ("reserved", ctypes.c_int32),
        ("d2", ctypes.c_double), ("logdet", ctypes.c_double), ("assign", ctypes.c_int32 * EKF_MAX_LINES),
    ]


ekf_assoc_hit = EkfAssocHit   # (the C name)


RP_INVALID, RP_KEPT = 1, 2   # ekf_plan_info.status


class EkfPlanInfo(ctypes.Structure):
    """ekf_plan_info (slam_ekf.h): what ekf_resample_plan_device reports beside its list."""
    _fields_ = [
        ("status", ctypes.c_int32), ("copies", ctypes.c_int32), ("ess", ctypes.c_double), ("total", ctypes.c_double),
    ]


ekf_plan_info = EkfPlanInfo   # (the C name)


class EkfImageDesc(ctypes.Structure):
    """ekf_image_desc (slam_ekf.h): the host-side label of one instance image; travels with it."""
    _fields_ = [
        ("magic", ctypes.c_uint32), ("version", ctypes.c_uint32), ("key", ctypes.c_uint64),
        ("bytes", ctypes.c_uint64), ("pending", ctypes.c_int32), ("has_step", ctypes.c_int32),
        ("epoch", ctypes.c_uint32), ("groups", ctypes.c_int32), ("storage_exp", ctypes.c_int32),
        ("reserved", ctypes.c_int32 * 5),
    ]


ekf_image_desc = EkfImageDesc   # (the C name)


class EkfError(RuntimeError):
    code = 0   # the EKF_E* status of the failed call


_lib = None
loaded_path = None   # the file load_library() loaded


def load_library(path: str = ""):
    """Load libslam_ekf.so (never builds implicitly on a GPU box: fail loudly instead).
    SLAM_EKF_LIB selects another build of the same library (A/B experiments)."""
    global _lib, loaded_path
    if _lib is not None:
        return _lib
    path = path or os.environ.get("SLAM_EKF_LIB") or LIB_PATH
    if not os.path.exists(path):
        raise EkfError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`"
                       " (HIP extension required; there is no CPU fallback)")
    L = ctypes.CDLL(path)
    loaded_path = path
    vp, i32, d, sz = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double, ctypes.c_size_t
    dp = ctypes.POINTER(ctypes.c_double)
    ip = ctypes.POINTER(ctypes.c_int32)
    cp = ctypes.POINTER(vp)
    sig = {
        "ekf_config_init": (None, [ctypes.POINTER(EkfConfig)]),
        "ekf_strerror": (ctypes.c_char_p, [ctypes.c_int]),
        "ekf_abi_version": (ctypes.c_int, []),
        "ekf_create": (ctypes.c_int, [ctypes.POINTER(EkfConfig), cp]),
        "ekf_destroy": (ctypes.c_int, [vp]),
        "ekf_set_stream": (ctypes.c_int, [vp, vp]),
        "ekf_sync": (ctypes.c_int, [vp]),
        "ekf_set_option": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int]),
        "ekf_get_option": (ctypes.c_int, [vp, ctypes.c_int, ip]),
        "ekf_reset_instance": (ctypes.c_int, [vp, ctypes.c_int, d, d, d]),
        "ekf_localize": (ctypes.c_int, [vp, dp, vp, ip, vp]),
        "ekf_localize_device": (ctypes.c_int, [vp, vp, vp, vp]),
        "ekf_predict": (ctypes.c_int, [vp, dp]),
        "ekf_update": (ctypes.c_int, [vp, vp, ip, vp]),
        "ekf_read_results": (ctypes.c_int, [vp, vp]),
        "ekf_upload_state": (ctypes.c_int, [vp, ctypes.c_int, dp, dp, ctypes.c_int, dp]),
        "ekf_download_state": (ctypes.c_int, [vp, ctypes.c_int, dp, dp, ip, dp]),
        "ekf_init_lowrank": (ctypes.c_int, [vp, ctypes.c_int, dp, dp, ctypes.c_int, dp,
                                            ctypes.c_int, dp]),
        "ekf_storage_exponent": (ctypes.c_int, [vp, ctypes.c_int]),
        "ekf_rescale": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int]),
        "ekf_get_pose_cov": (ctypes.c_int, [vp, ctypes.c_int, dp]),
        "ekf_get_ellipse": (ctypes.c_int, [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_float),
                                           ctypes.POINTER(ctypes.c_float)]),
        "ekf_ellipse_of_block": (ctypes.c_int, [dp, ctypes.POINTER(ctypes.c_float),
                                                ctypes.POINTER(ctypes.c_float)]),
        "ekf_query_joint": (ctypes.c_int, [vp, ctypes.c_int, ip, ctypes.c_int, dp, dp]),
        "ekf_query_marginals": (ctypes.c_int, [vp, ctypes.c_int, ip, ctypes.c_int, dp, dp, dp]),
        "ekf_query_joint_device": (ctypes.c_int, [vp, vp, ctypes.c_int, vp, vp]),
        "ekf_gate_lines": (ctypes.c_int, [vp, ctypes.c_int, dp, vp, ctypes.c_int, vp, dp]),
        "ekf_gate_lines_device": (ctypes.c_int, [vp, vp, vp, vp, vp, vp]),
        "ekf_gate_joint": (ctypes.c_int, [vp, ctypes.c_int, dp, vp, ctypes.c_int, vp, ctypes.c_int, vp, dp]),
        "ekf_gate_joint_device": (ctypes.c_int, [vp, vp, vp, vp, vp, ctypes.c_int, vp, vp]),
        "ekf_associate_joint": (ctypes.c_int, [vp, ctypes.c_int, dp, vp, ctypes.c_int, vp, ctypes.c_int, dp,
                                               ctypes.c_int, vp]),
        "ekf_associate_joint_device": (ctypes.c_int, [vp, vp, vp, vp, vp, ctypes.c_int, vp, ctypes.c_int, vp]),
        "ekf_gate_landmarks": (ctypes.c_int, [vp, ctypes.c_int, d, vp, dp]),
        "ekf_gate_landmarks_device": (ctypes.c_int, [vp, d, vp, vp]),
        "ekf_resample": (ctypes.c_int, [vp, ip]),
        "ekf_copy_instance": (ctypes.c_int, [vp, ctypes.c_int, ctypes.c_int]),
        "ekf_gate_candidates_device": (ctypes.c_int, [vp, vp, vp, ctypes.c_int, d, vp, vp]),
        "ekf_assoc_weights_device": (ctypes.c_int, [vp, vp, vp, d, vp, vp]),
        "ekf_resample_plan_device": (ctypes.c_int, [vp, vp, d, d, vp, vp]),
        "ekf_resample_device": (ctypes.c_int, [vp, vp, vp]),
        "ekf_instance_image_bytes": (sz, [vp]),
        "ekf_export_instances": (ctypes.c_int, [vp, ip, ctypes.c_int, vp, vp]),
        "ekf_import_instances": (ctypes.c_int, [vp, ip, ctypes.c_int, vp, vp]),
        "ekf_export_instances_device": (ctypes.c_int, [vp, ip, ctypes.c_int, vp, vp]),
        "ekf_import_instances_device": (ctypes.c_int, [vp, ip, ctypes.c_int, vp, vp]),
        "ekf_landmark_block_bytes": (sz, [vp]),
        "ekf_state_dim": (ctypes.c_int, [vp]),
        "ekf_profile_enable": (ctypes.c_int, [vp, ctypes.c_int]),
        "ekf_profile_read": (ctypes.c_int, [vp, dp, dp, dp, ip]),
        "ekf_profile_flushes": (ctypes.c_int, [vp, ctypes.c_int, ip, ctypes.POINTER(ctypes.c_float)]),
        "ekf_flush_kernel_name": (ctypes.c_char_p, [vp, ctypes.c_int]),
        "ekf_debug_scan_stamps": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_ulonglong)]),
        "ekf_debug_result_words": (ctypes.c_int, [vp, ctypes.c_int, ip]),
        "ekf_shard_create": (ctypes.c_int, [ctypes.POINTER(EkfConfig), ctypes.c_int, ctypes.c_int, cp]),
        "ekf_shard_tiles": (ctypes.c_int, [vp, ip, ip]),
        "ekf_shard_buffer_words": (sz, [vp]),
        "ekf_shard_begin": (ctypes.c_int, [vp, dp, vp, ctypes.c_int, vp]),
        "ekf_shard_line": (ctypes.c_int, [vp, ctypes.c_int, vp]),
        "ekf_shard_apply": (ctypes.c_int, [vp, ctypes.c_int, vp]),
        "ekf_shard_end": (ctypes.c_int, [vp, vp]),
        "ekf_shard_abort": (ctypes.c_int, [vp]),
        "ekf_shard_spec_buffer_words": (sz, [vp]),
        "ekf_shard_speculate": (ctypes.c_int, [vp, vp, vp]),
        "ekf_shard_run": (ctypes.c_int, [vp, vp, vp]),
        "ekf_rccl_unique_id": (ctypes.c_int, [vp]),
        "ekf_shard_attach_rccl": (ctypes.c_int, [vp, vp, ctypes.c_int, ctypes.c_int]),
        "ekf_shard_localize": (ctypes.c_int, [vp, vp, vp, ctypes.c_int, vp]),
        "ekf_shard_resume": (ctypes.c_int, [vp, ctypes.c_int]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def _check(rc: int, what: str):
    if rc != 0:
        msg = load_library().ekf_strerror(rc).decode()
        err = EkfError(f"{what}: {msg} ({rc})")
        err.code = rc
        raise err


def _dp(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def lines_array(lines, max_lines: int, instances: int = 1) -> np.ndarray:
    """(E, max_lines, 6) float64 array → contiguous ekf_line buffer (zero padded)."""
    arr = np.asarray(lines, dtype=np.float64)
    if arr.ndim == 2:
        arr = arr[None]
    out = np.zeros((instances, max_lines, 6))
    L = min(arr.shape[1], max_lines)
    out[: arr.shape[0], :L] = arr[:, :L, :6]
    return np.ascontiguousarray(out)


def ellipse_of_block(P22):
    """Robot::getEllipse arithmetic (Robot.cpp:73-124) on a given 2x2 block, host side of the
    library (no device): (ok, [axii0, axii1], angle)."""
    blk = np.ascontiguousarray(np.asarray(P22, dtype=np.float64).reshape(4))
    axii = (ctypes.c_float * 2)()
    ang = ctypes.c_float()
    rc = load_library().ekf_ellipse_of_block(_dp(blk), axii, ctypes.byref(ang))
    if rc < 0:
        _check(-rc, "ekf_ellipse_of_block")
    return rc == 1, [axii[0], axii[1]], ang.value


def gate_candidates(d2, C: int, gate: float) -> np.ndarray:
    """The candidate lists ekf_associate_joint takes, from the individual distances d2 [L, N] of
    ekf_gate_lines: per line the up to C landmarks with the smallest sqrt|d2| inside `gate`, ascending
    (the lower landmark first on ties), padded with -1: [L, C] int32. Good children come first, so the
    search's incumbent tightens early. NaN and +inf (at and past savedLineCount) are never candidates."""
    d = np.sqrt(np.abs(np.asarray(d2, dtype=np.float64)))
    d = d.reshape(-1, d.shape[-1]) if d.ndim else d.reshape(0, 0)
    out = np.full((d.shape[0], int(C)), -1, dtype=np.int32)
    for i, row in enumerate(d):
        ok = np.flatnonzero(row <= gate)          # (NaN fails)
        ok = ok[np.argsort(row[ok], kind="stable")][:C]
        out[i, :len(ok)] = ok
    return out


def duplicate_clusters(hits, d2=None) -> list[list[int]]:
    """The landmark groups of size >= 2 that Ensemble.gate_landmarks' passing pairs connect (union-find),
    each ascending, in ascending order of their lowest member. With the matrix d2 [N, N] every passing pair
    is used: the passing partners of row a are its hits[a]["npass"] smallest entries (pass is a threshold on
    d2, so no gate is needed). Without it only the pairs the records name, (a, first) and (a, nearest) where
    something passes: a subset of the passing pairs, so a group may come out in parts. Host only."""
    h = np.asarray(hits)
    n = int(h.shape[0])
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    def union(a, b):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)

    for a in range(n):
        k = int(h["npass"][a])
        if k <= 0:
            continue
        if d2 is None:
            union(a, int(h["first"][a]))
            union(a, int(h["nearest"][a]))
        else:
            row = np.asarray(d2[a], dtype=np.float64)
            thr = np.sort(np.where(np.isnan(row), np.inf, row))[k - 1]
            for b in np.flatnonzero(row <= thr):
                union(a, int(b))
    groups: dict[int, list[int]] = {}
    for a in range(n):
        groups.setdefault(find(a), []).append(a)
    return [g for _, g in sorted(groups.items()) if len(g) >= 2]


def chi2_cdf_even(x: float, m: int) -> float:
    """P(X <= x) for chi-square with 2m degrees of freedom: 1 - e^(-x/2) sum_{k<m} (x/2)^k / k!."""
    h, term, acc = 0.5 * float(x), 1.0, 0.0
    for k in range(int(m)):
        acc += term
        term *= h / (k + 1)
    return 1.0 - float(np.exp(-h)) * acc


def chi2_bounds(L: int, confidence: float) -> np.ndarray:
    """bound[m], m = 0..L, for ekf_associate_joint: the chi-square quantile at `confidence` for 2m degrees
    of freedom (bound[0] = 0), from the closed form for even degrees of freedom solved by bisection."""
    if not 0.0 < confidence < 1.0:
        raise ValueError("confidence must lie in (0, 1)")
    out = np.zeros(int(L) + 1)
    for m in range(1, int(L) + 1):
        lo, hi = 0.0, 2.0 * m
        while chi2_cdf_even(hi, m) < confidence:
            hi *= 2.0
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            if mid == lo or mid == hi:
                break
            if chi2_cdf_even(mid, m) < confidence:
                lo = mid
            else:
                hi = mid
        out[m] = hi
    return out


def resample_plan(weights, u: float) -> list[int]:
    """Systematic resampling as a list Ensemble.resample accepts. With the weights normalised by their
    sum, n_e is the number of points (u + k) / E, k = 0 .. E − 1, in instance e's interval of the
    cumulative weights. Every e with n_e >= 1 keeps its state (src[e] = e); the slots with n_e == 0, in
    ascending order, take the surplus copies of the survivors in ascending survivor order."""
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    E = int(w.size)
    if E == 0 or not np.all(np.isfinite(w)) or np.any(w < 0.0):
        raise ValueError("resample_plan: the weights must be finite and non-negative")
    total = float(w.sum())
    if not (total > 0.0) or not math.isfinite(total):
        raise ValueError("resample_plan: the weights sum to zero")
    if not 0.0 <= u < 1.0:
        raise ValueError("resample_plan: u outside [0, 1)")
    edges = np.cumsum(w / total)
    points = (u + np.arange(E)) / E
    # (every point is below 1: rounding in the sum must not push one past the last positive weight)
    hit = np.minimum(np.searchsorted(edges, points, side="right"), np.flatnonzero(w > 0.0)[-1])
    counts = np.bincount(hit, minlength=E)
    src = list(range(E))
    surplus = [e for e in range(E) for _ in range(int(counts[e]) - 1)]
    for slot, e in zip([e for e in range(E) if counts[e] == 0], surplus):
        src[slot] = e
    return src


class Ensemble:
    """E independent EKF instances of capacity N on one GPU (one C-ABI context)."""

    def __init__(self, capacity: int, instances: int = 1, precision: int = PREC_F64,
                 max_lines: int = 20, device: int = -1, r_mode: int = R_INTENDED,
                 reset_margin: int = 10, mahalanobis: float = 0.4, encoder_noise: float = 0.024,
                 pipeline: bool = False, flush_interval: int = 1, arith: int = ARITH_EXACT,
                 options: dict | None = None, shard: tuple[int, int] | None = None):
        """shard = (rank, world): a partitioned instance (slam_ekf.h ekf_shard_create; instances = 1)
        storing its share of the landmark block only; rowshard_gpu.ShardedInstance drives it."""
        self._lib = load_library()
        cfg = EkfConfig()
        self._lib.ekf_config_init(ctypes.byref(cfg))
        cfg.capacity, cfg.instances, cfg.precision = capacity, instances, precision
        cfg.device, cfg.max_lines, cfg.r_mode = device, max_lines, r_mode
        cfg.reset_margin, cfg.mahalanobis, cfg.encoder_noise = reset_margin, mahalanobis, encoder_noise
        cfg.pipeline = 1 if pipeline else 0
        cfg.flush_interval = int(flush_interval)
        cfg.arith = int(arith)
        h = ctypes.c_void_p()
        if shard is None:
            _check(self._lib.ekf_create(ctypes.byref(cfg), ctypes.byref(h)), "ekf_create")
        else:
            _check(self._lib.ekf_shard_create(ctypes.byref(cfg), int(shard[0]), int(shard[1]), ctypes.byref(h)),
                   "ekf_shard_create")
        self._h = h
        self.capacity, self.instances, self.precision = capacity, instances, precision
        self.max_lines = max_lines
        self.arith = int(arith)
        self.n = self._lib.ekf_state_dim(h)
        self._res = (EkfResult * instances)()
        for k, v in (options or {}).items():
            self.set_option(k, v)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.ekf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def set_stream(self, stream_handle: int | None):
        _check(self._lib.ekf_set_stream(self._h, ctypes.c_void_p(stream_handle or 0)), "ekf_set_stream")

    def sync(self):
        _check(self._lib.ekf_sync(self._h), "ekf_sync")

    def set_option(self, option, value: int):
        """ekf_set_option: option is an OPT_* number or an OPTIONS name (e.g. "speculate")."""
        opt = OPTIONS[option] if isinstance(option, str) else int(option)
        _check(self._lib.ekf_set_option(self._h, opt, int(value)), f"ekf_set_option({option}, {value})")

    def get_option(self, option) -> int:
        opt = OPTIONS[option] if isinstance(option, str) else int(option)
        v = ctypes.c_int32()
        _check(self._lib.ekf_get_option(self._h, opt, ctypes.byref(v)), f"ekf_get_option({option})")
        return v.value

    def reset(self, e: int = -1, x: float = 0.0, y: float = 0.0, theta: float = 0.0):
        _check(self._lib.ekf_reset_instance(self._h, e, x, y, theta), "ekf_reset_instance")

    def _results(self) -> list[dict]:
        out = []
        for r in self._res:
            out.append(dict(pose=np.array(r.pose[:]), matches=r.matches,
                            new_landmarks=r.new_landmarks, saved=r.saved, reset=r.reset,
                            status=r.status, match=list(r.match[: r.nlines])))
        return out

    def localize(self, encoder, lines, nlines=None) -> list[dict]:
        enc = np.ascontiguousarray(np.asarray(encoder, dtype=np.float64).reshape(self.instances, 3))
        la = lines_array(lines, self.max_lines, self.instances)
        if nlines is None:
            nl = np.array([min(np.asarray(lines).reshape(self.instances, -1, 6).shape[1],
                               self.max_lines)] * self.instances, dtype=np.int32)
        else:
            nl = np.ascontiguousarray(np.asarray(nlines, dtype=np.int32).reshape(self.instances))
        _check(self._lib.ekf_localize(self._h, _dp(enc), la.ctypes.data_as(ctypes.c_void_p),
                                      nl.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                      ctypes.byref(self._res)), "ekf_localize")
        return self._results()

    def localize_device(self, d_enc: int, d_lines: int, d_nlines: int):
        """Inputs already in device memory (raw pointers); asynchronous on the context stream."""
        _check(self._lib.ekf_localize_device(self._h, ctypes.c_void_p(d_enc), ctypes.c_void_p(d_lines),
                                             ctypes.c_void_p(d_nlines)), "ekf_localize_device")

    def predict(self, encoder):
        enc = np.ascontiguousarray(np.asarray(encoder, dtype=np.float64).reshape(self.instances, 3))
        _check(self._lib.ekf_predict(self._h, _dp(enc)), "ekf_predict")

    def update(self, lines, nlines=None) -> list[dict]:
        la = lines_array(lines, self.max_lines, self.instances)
        if nlines is None:
            nl = np.array([min(np.asarray(lines).reshape(self.instances, -1, 6).shape[1],
                               self.max_lines)] * self.instances, dtype=np.int32)
        else:
            nl = np.ascontiguousarray(np.asarray(nlines, dtype=np.int32).reshape(self.instances))
        _check(self._lib.ekf_update(self._h, la.ctypes.data_as(ctypes.c_void_p),
                                    nl.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                    ctypes.byref(self._res)), "ekf_update")
        return self._results()

    def read_results(self) -> list[dict]:
        _check(self._lib.ekf_read_results(self._h, ctypes.byref(self._res)), "ekf_read_results")
        return self._results()

    def upload_state(self, e: int, P=None, y=None, saved: int = 0, pose=None):
        Pc = None if P is None else np.ascontiguousarray(P, dtype=np.float64)
        yc = None if y is None else np.ascontiguousarray(y, dtype=np.float64)
        pc = None if pose is None else np.ascontiguousarray(pose, dtype=np.float64)
        _check(self._lib.ekf_upload_state(self._h, e, _dp(Pc), _dp(yc), int(saved), _dp(pc)),
               "ekf_upload_state")

    def init_lowrank(self, e: int, diag, U, y, saved: int, pose=(0.0, 0.0, 0.0)):
        dc = np.ascontiguousarray(diag, dtype=np.float64)
        Uc = np.ascontiguousarray(U, dtype=np.float64)
        yc = np.ascontiguousarray(y, dtype=np.float64)
        pc = np.ascontiguousarray(pose, dtype=np.float64)
        _check(self._lib.ekf_init_lowrank(self._h, e, _dp(dc), _dp(Uc), int(Uc.shape[1]), _dp(yc),
                                          int(saved), _dp(pc)), "ekf_init_lowrank")

    def download_state(self, e: int, with_P: bool = True):
        P = np.zeros((self.n, self.n)) if with_P else None
        y = np.zeros(self.n)
        saved = ctypes.c_int32()
        pose = np.zeros(3)
        _check(self._lib.ekf_download_state(self._h, e, _dp(P), _dp(y), ctypes.byref(saved), _dp(pose)),
               "ekf_download_state")
        return P, y, saved.value, pose

    def storage_exponent(self, e: int = 0) -> int:
        """fp16 storage: the landmark block holds fp16(2^exp·P); 0 for f32 / f64."""
        return int(self._lib.ekf_storage_exponent(self._h, e))

    def rescale(self, e: int = 0, exp: int = EXP_AUTO):
        """Re-choose (or set) instance e's fp16 storage exponent (after ST_RANGE)."""
        _check(self._lib.ekf_rescale(self._h, e, int(exp)), "ekf_rescale")

    def pose_cov(self, e: int = 0) -> np.ndarray:
        out = np.zeros(9)
        _check(self._lib.ekf_get_pose_cov(self._h, e, _dp(out)), "ekf_get_pose_cov")
        return out.reshape(3, 3)

    def query_joint(self, e: int, landmarks):
        """Joint marginal of the pose and the given landmarks of instance e, read without draining
        (slam_ekf.h ekf_query_joint): (cov, mean) = (P[rows][:, rows], y[rows]) for rows
        {0, 1, 2, 3 + 2j, 4 + 2j : j in landmarks}; duplicates and any order are allowed."""
        lm = np.ascontiguousarray(np.asarray(landmarks, dtype=np.int32).reshape(-1))
        K = int(lm.size)
        cov = np.zeros((3 + 2 * K, 3 + 2 * K))
        mean = np.zeros(3 + 2 * K)
        _check(self._lib.ekf_query_joint(self._h, e, lm.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), K,
                                         _dp(cov), _dp(mean)), "ekf_query_joint")
        return cov, mean

    def query_marginals(self, e: int, landmarks=None, count=None):
        """Per-landmark marginals of instance e, read without draining (ekf_query_marginals):
        (blocks [K, 2, 2], cross [K, 3, 2] = P[0:3, 3 + 2j : 5 + 2j], mean [K, 2]). landmarks None:
        the first `count` landmarks (default: all of the capacity)."""
        if landmarks is None:
            lm, K = None, self.capacity if count is None else int(count)
        else:
            lm = np.ascontiguousarray(np.asarray(landmarks, dtype=np.int32).reshape(-1))
            K = int(lm.size) if count is None else int(count)
        blocks, cross, mean = np.zeros((K, 2, 2)), np.zeros((K, 3, 2)), np.zeros((K, 2))
        lp = None if lm is None else lm.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        _check(self._lib.ekf_query_marginals(self._h, e, lp, K, _dp(blocks), _dp(cross), _dp(mean)),
               "ekf_query_marginals")
        return blocks, cross, mean

    def query_joint_device(self, d_landmarks: int, K: int, d_cov: int, d_mean: int):
        """The joint query of every instance, buffers in device memory (raw pointers: landmarks
        [E, K] int32, cov [E, (3 + 2K)²], mean [E, 3 + 2K]; either output may be 0); asynchronous on
        the context stream."""
        _check(self._lib.ekf_query_joint_device(self._h, ctypes.c_void_p(d_landmarks or None), int(K),
                                                ctypes.c_void_p(d_cov or None), ctypes.c_void_p(d_mean or None)),
               "ekf_query_joint_device")

    def gate_lines(self, e: int, lines, encoder=None, distances: bool = False):
        """Trial lines scored against instance e's map, state untouched (slam_ekf.h ekf_gate_lines):
        every line on its own, as the first line of a scan. encoder given: the predict is applied on
        read, so hits[0]["first"] is the match localize(encoder, lines) would report for line 0; None:
        the committed pose and strip (between predict and update: what update would use). Returns a
        list of dicts (first, nearest, npass, status, d2_first, d2_nearest, S [2, 2], v [2]), and
        with distances=True also d2 [L, N] (+inf at and past savedLineCount)."""
        la = np.ascontiguousarray(np.asarray(lines, dtype=np.float64).reshape(-1, 6))
        L = int(la.shape[0])
        enc = None if encoder is None else np.ascontiguousarray(np.asarray(encoder, dtype=np.float64).reshape(3))
        hits = (EkfGateHit * max(L, 1))()
        d2 = np.zeros((L, self.capacity)) if distances else None
        _check(self._lib.ekf_gate_lines(self._h, int(e), _dp(enc), la.ctypes.data_as(ctypes.c_void_p), L,
                                        ctypes.byref(hits), _dp(d2)), "ekf_gate_lines")
        out = [self._hit(hits[i]) for i in range(L)]
        return (out, d2) if distances else out

    @staticmethod
    def _hit(h) -> dict:
        return dict(first=h.first, nearest=h.nearest, npass=h.npass, status=h.status, d2_first=h.d2_first,
                    d2_nearest=h.d2_nearest, S=np.array(h.S[:]).reshape(2, 2), v=np.array(h.v[:]))

    def gate_lines_device(self, d_enc: int, d_lines: int, d_nlines: int, d_hits: int, d_d2: int = 0):
        """The gate of every instance at once, buffers in device memory (raw pointers: enc [E, 3] or 0,
        lines [E, max_lines] ekf_line, nlines [E] int32, hits [E, max_lines] ekf_gate_hit, d2
        [E, max_lines, N] or 0); asynchronous on the context stream."""
        _check(self._lib.ekf_gate_lines_device(self._h, ctypes.c_void_p(d_enc or None), ctypes.c_void_p(d_lines or None),
                                               ctypes.c_void_p(d_nlines or None), ctypes.c_void_p(d_hits or None),
                                               ctypes.c_void_p(d_d2 or None)), "ekf_gate_lines_device")

    def gate_landmarks(self, e: int, gate: float, want_d2: bool = False):
        """Every saved landmark of instance e scored against every other, state untouched (slam_ekf.h
        ekf_gate_landmarks): the landmark pairs that are one line, in the same direction or flipped
        (alpha + pi, -r). Returns hits, a [N] array of PAIR_HIT_DTYPE (nearest, first, npass, status,
        d2_nearest, d2_first, C [3], delta [2]), and with want_d2=True also d2 [N, N] (+inf on the diagonal
        and at and past savedLineCount). A pair passes when d2 <= gate²; duplicate_clusters groups them."""
        hits = np.zeros(self.capacity, dtype=PAIR_HIT_DTYPE)
        d2 = np.zeros((self.capacity, self.capacity)) if want_d2 else None
        _check(self._lib.ekf_gate_landmarks(self._h, int(e), float(gate), hits.ctypes.data_as(ctypes.c_void_p),
                                            _dp(d2)), "ekf_gate_landmarks")
        return (hits, d2) if want_d2 else hits

    def gate_landmarks_device(self, gate: float, d_hits: int, d_d2: int = 0):
        """gate_landmarks of every instance at once, buffers in device memory (raw pointers: hits [E, N]
        ekf_pair_hit, d2 [E, N, N] or 0); asynchronous on the context stream."""
        _check(self._lib.ekf_gate_landmarks_device(self._h, float(gate), ctypes.c_void_p(d_hits or None),
                                                   ctypes.c_void_p(d_d2 or None)), "ekf_gate_landmarks_device")

    def gate_joint(self, e: int, lines, assign, encoder=None, each: bool = False):
        """Joint compatibility of hypotheses against instance e's map, state untouched (slam_ekf.h
        ekf_gate_joint). assign [H, L] int32: the landmark of each line or -1. Returns a list of H dicts
        (m, status, d2, logdet): d2 = v^T S^-1 v of the stacked innovation, logdet = log det S; the
        log-likelihood is -(d2 + logdet) / 2 - m log(2 pi). With each=True also d2_each [H, L], every
        pair's own distance (NaN where unassigned). encoder as for gate_lines."""
        la = np.ascontiguousarray(np.asarray(lines, dtype=np.float64).reshape(-1, 6))
        L = int(la.shape[0])
        aa = np.ascontiguousarray(np.asarray(assign, dtype=np.int32).reshape(-1, L) if L else
                                  np.zeros((len(assign), 0), dtype=np.int32))
        H = int(aa.shape[0])
        enc = None if encoder is None else np.ascontiguousarray(np.asarray(encoder, dtype=np.float64).reshape(3))
        hits = (EkfJointHit * max(H, 1))()
        d2 = np.zeros((H, L)) if each else None
        _check(self._lib.ekf_gate_joint(self._h, int(e), _dp(enc), la.ctypes.data_as(ctypes.c_void_p), L,
                                        aa.ctypes.data_as(ctypes.c_void_p), H, ctypes.byref(hits), _dp(d2)),
               "ekf_gate_joint")
        out = [self._joint_hit(hits[h]) for h in range(H)]
        return (out, d2) if each else out

    @staticmethod
    def _joint_hit(h) -> dict:
        return dict(m=h.m, status=h.status, d2=h.d2, logdet=h.logdet)

    def gate_joint_device(self, d_enc: int, d_lines: int, d_nlines: int, d_assign: int, H: int, d_hits: int,
                          d_d2_each: int = 0):
        """The hypotheses of every instance at once, buffers in device memory (raw pointers: enc [E, 3]
        or 0, lines [E, max_lines] ekf_line, nlines [E] int32, assign [E, H, max_lines] int32, hits
        [E, H] ekf_joint_hit, d2_each [E, H, max_lines] or 0); asynchronous on the context stream."""
        _check(self._lib.ekf_gate_joint_device(self._h, ctypes.c_void_p(d_enc or None), ctypes.c_void_p(d_lines or None),
                                               ctypes.c_void_p(d_nlines or None), ctypes.c_void_p(d_assign or None), int(H),
                                               ctypes.c_void_p(d_hits or None), ctypes.c_void_p(d_d2_each or None)),
               "ekf_gate_joint_device")

    def associate_joint(self, e: int, lines, cand, bound, encoder=None, max_nodes: int = 1 << 16):
        """The joint-compatibility search against instance e's map, state untouched (slam_ekf.h
        ekf_associate_joint): cand [L, C] int32, each line's candidate landmarks or -1 (gate_candidates);
        bound [L + 1], the joint distance allowed with m pairings (chi2_bounds). Returns a dict (m, status,
        nodes, d2, logdet, assign [L]): the jointly compatible assignment with the most pairings, then the
        smallest d2; d2 and logdet are gate_joint's for `assign`, bit for bit. status carries AS_TRUNCATED
        when max_nodes ran out (the result is then feasible but not guaranteed optimal) and AS_SINGULAR
        when a child was pruned by a failed pivot. encoder as for gate_lines."""
        la = np.ascontiguousarray(np.asarray(lines, dtype=np.float64).reshape(-1, 6))
        L = int(la.shape[0])
        ca = np.ascontiguousarray(np.asarray(cand, dtype=np.int32).reshape(L, -1) if L else np.zeros((0, 1), dtype=np.int32))
        C = int(ca.shape[1])
        ba = np.ascontiguousarray(np.asarray(bound, dtype=np.float64).reshape(-1))
        if ba.shape[0] < L + 1:
            raise ValueError("bound needs L + 1 entries")
        enc = None if encoder is None else np.ascontiguousarray(np.asarray(encoder, dtype=np.float64).reshape(3))
        hit = EkfAssocHit()
        _check(self._lib.ekf_associate_joint(self._h, int(e), _dp(enc), la.ctypes.data_as(ctypes.c_void_p), L,
                                             ca.ctypes.data_as(ctypes.c_void_p), C, _dp(ba), int(max_nodes),
                                             ctypes.byref(hit)), "ekf_associate_joint")
        return self._assoc_hit(hit, L)

    @staticmethod
    def _assoc_hit(h, L: int = EKF_MAX_LINES) -> dict:
        return dict(m=h.m, status=h.status, nodes=h.nodes, d2=h.d2, logdet=h.logdet,
                    assign=np.array(h.assign[:L], dtype=np.int32))

    def associate_joint_device(self, d_enc: int, d_lines: int, d_nlines: int, d_cand: int, C: int, d_bound: int,
                               d_hits: int, max_nodes: int = 1 << 16):
        """The search of every instance at once, buffers in device memory (raw pointers: enc [E, 3] or 0,
        lines [E, max_lines] ekf_line, nlines [E] int32, cand [E, max_lines, C] int32, bound
        [max_lines + 1] shared by the instances, hits [E] ekf_assoc_hit); asynchronous on the context
        stream."""
        _check(self._lib.ekf_associate_joint_device(self._h, ctypes.c_void_p(d_enc or None), ctypes.c_void_p(d_lines or None),
                                                    ctypes.c_void_p(d_nlines or None), ctypes.c_void_p(d_cand or None), int(C),
                                                    ctypes.c_void_p(d_bound or None), int(max_nodes),
                                                    ctypes.c_void_p(d_hits or None)), "ekf_associate_joint_device")

    def resample(self, src):
        """Instance e takes the whole state of instance src[e] on the device, pending steps included,
        without a drain or a flush (slam_ekf.h ekf_resample). Every source must keep its own state
        (src[src[e]] == src[e]); resample_plan gives such a list. Asynchronous on the context stream."""
        sa = np.ascontiguousarray(np.asarray(src, dtype=np.int32).reshape(-1))
        if sa.size != self.instances:
            raise ValueError(f"resample: {sa.size} sources for {self.instances} instances")
        _check(self._lib.ekf_resample(self._h, sa.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))), "ekf_resample")

    def gate_candidates_device(self, d_d2: int, d_nlines: int, C: int, gate: float, d_cand: int, d_count: int = 0):
        """gate_candidates on the device, for every line of every instance (slam_ekf.h
        ekf_gate_candidates_device; raw pointers: d2 [E, max_lines, N] as gate_lines_device wrote it, nlines
        [E] int32, cand [E, max_lines, C] int32, count [E, max_lines] int32 or 0: the members before the
        cut). The lists are gate_candidates' bit for bit; asynchronous on the context stream."""
        _check(self._lib.ekf_gate_candidates_device(self._h, ctypes.c_void_p(d_d2 or None), ctypes.c_void_p(d_nlines or None),
                                                    int(C), float(gate), ctypes.c_void_p(d_cand or None),
                                                    ctypes.c_void_p(d_count or None)), "ekf_gate_candidates_device")

    def assoc_weights_device(self, d_hits: int, d_nlines: int, d_weights: int, log_unassigned: float = 0.0,
                             d_logprior: int = 0):
        """The instances' weights from associate_joint_device's hits (ekf_assoc_weights_device; raw
        pointers: hits [E] ekf_assoc_hit, nlines [E] int32, weights [E], logprior [E] or 0):
        exp(lw - max lw) with lw = -(d2 + logdet) / 2 - m log(2 pi) + (nlines - m) log_unassigned + logprior;
        0 for an instance whose hit is AS_INVALID or whose lw is not finite. Asynchronous."""
        _check(self._lib.ekf_assoc_weights_device(self._h, ctypes.c_void_p(d_hits or None), ctypes.c_void_p(d_nlines or None),
                                                  float(log_unassigned), ctypes.c_void_p(d_logprior or None),
                                                  ctypes.c_void_p(d_weights or None)), "ekf_assoc_weights_device")

    def resample_plan_device(self, d_weights: int, u: float, d_src: int, ess_below: float = math.inf, d_info: int = 0):
        """resample_plan on the device (ekf_resample_plan_device; raw pointers: weights [E], src [E] int32,
        info one ekf_plan_info or 0): the list resample_device takes. The identity list when the effective
        sample size is not below ess_below (RP_KEPT) or the weights are unusable (RP_INVALID).
        Asynchronous."""
        _check(self._lib.ekf_resample_plan_device(self._h, ctypes.c_void_p(d_weights or None), float(u), float(ess_below),
                                                  ctypes.c_void_p(d_src or None), ctypes.c_void_p(d_info or None)),
               "ekf_resample_plan_device")

    def resample_device(self, d_src: int, d_status: int = 0):
        """resample with the list in device memory (ekf_resample_device; raw pointers: src [E] int32,
        status one int32 or 0). The list is checked on the device: a list resample would refuse copies
        nothing and leaves EKF_EINVAL or EKF_ERANGE in status. Asynchronous on the context stream."""
        _check(self._lib.ekf_resample_device(self._h, ctypes.c_void_p(d_src or None), ctypes.c_void_p(d_status or None)),
               "ekf_resample_device")

    def copy_instance(self, dst: int, src: int):
        """Instance dst becomes a copy of instance src (ekf_copy_instance): forks a hypothesis."""
        _check(self._lib.ekf_copy_instance(self._h, int(dst), int(src)), "ekf_copy_instance")

    def instance_image_bytes(self) -> int:
        """Bytes of one instance's image as the context stands now (ekf_instance_image_bytes): it grows
        with the steps pending in the open flush group."""
        return int(self._lib.ekf_instance_image_bytes(self._h))

    @staticmethod
    def _inst_list(inst):
        ia = np.ascontiguousarray(np.asarray(inst, dtype=np.int32).reshape(-1))
        # (an empty list still hands the library a pointer)
        return ia, (ia if ia.size else np.zeros(1, dtype=np.int32)).ctypes.data_as(ctypes.POINTER(ctypes.c_int32))

    @staticmethod
    def _desc_array(descs, K: int):
        arr = (EkfImageDesc * max(K, 1))()
        if len(descs) != K:
            raise ValueError(f"import_instances: {len(descs)} descriptors for {K} instances")
        for k, d in enumerate(descs):
            ctypes.memmove(ctypes.byref(arr[k]), ctypes.byref(d), ctypes.sizeof(EkfImageDesc))
        return arr

    def export_instances(self, inst):
        """Images of the instances `inst` in host memory (slam_ekf.h ekf_export_instances): (descs,
        images) with images a uint8 array [K, bytes]. A raw copy of everything the instances own, the
        pending steps included; nothing in the context changes, nothing drains. Synchronous."""
        ia, ip = self._inst_list(inst)
        K = int(ia.size)
        images = np.zeros((K, self.instance_image_bytes()), dtype=np.uint8)
        descs = (EkfImageDesc * max(K, 1))()
        buf = images if images.size else np.zeros(16, dtype=np.uint8)
        _check(self._lib.ekf_export_instances(self._h, ip, K, buf.ctypes.data_as(ctypes.c_void_p), ctypes.byref(descs)),
               "ekf_export_instances")
        return [descs[k] for k in range(K)], images

    def import_instances(self, inst, images, descs):
        """Slot inst[k] takes image k (ekf_import_instances): afterwards it reads, and from then on
        computes, bit for bit as the exported instance did. The context must be congruent with the
        descriptors (same configuration, as many steps pending); its other instances are untouched and
        nothing drains. Synchronous."""
        ia, ip = self._inst_list(inst)
        K = int(ia.size)
        im = np.ascontiguousarray(np.asarray(images, dtype=np.uint8).reshape(K, -1) if K else np.zeros((0, 16), dtype=np.uint8))
        arr = self._desc_array(list(descs), K)
        if any(int(arr[k].bytes) != im.shape[1] for k in range(K)):   # (the library reads desc.bytes per image)
            raise ValueError("import_instances: the images are not of their descriptors' size")
        buf = im if im.size else np.zeros(16, dtype=np.uint8)
        _check(self._lib.ekf_import_instances(self._h, ip, K, buf.ctypes.data_as(ctypes.c_void_p), ctypes.byref(arr)),
               "ekf_import_instances")

    def export_instances_device(self, inst, d_images: int):
        """The export into device memory at address d_images (K · instance_image_bytes() bytes; one
        launch, asynchronous on the context stream): returns the descriptors. Nothing orders another
        context's import after it: share a stream (set_stream, before the first step) or sync() first,
        which drains."""
        ia, ip = self._inst_list(inst)
        K = int(ia.size)
        descs = (EkfImageDesc * max(K, 1))()
        _check(self._lib.ekf_export_instances_device(self._h, ip, K, ctypes.c_void_p(d_images or None), ctypes.byref(descs)),
               "ekf_export_instances_device")
        return [descs[k] for k in range(K)]

    def import_instances_device(self, inst, d_images: int, descs):
        """The import from device memory at address d_images (one launch, asynchronous on the context
        stream)."""
        ia, ip = self._inst_list(inst)
        K = int(ia.size)
        arr = self._desc_array(list(descs), K)
        _check(self._lib.ekf_import_instances_device(self._h, ip, K, ctypes.c_void_p(d_images or None), ctypes.byref(arr)),
               "ekf_import_instances_device")

    def ellipse(self, e: int = 0):
        axii = (ctypes.c_float * 2)()
        ang = ctypes.c_float()
        rc = self._lib.ekf_get_ellipse(self._h, e, axii, ctypes.byref(ang))
        if rc < 0:
            _check(-rc, "ekf_get_ellipse")
        return rc == 1, [axii[0], axii[1]], ang.value

    def profile_flushes(self) -> list[tuple[int, float]]:
        """(steps, ms) of every flush launch timed since the last profile() call."""
        n = self._lib.ekf_profile_flushes(self._h, 0, None, None)
        if n < 0:
            _check(-n, "ekf_profile_flushes")
        ns = (ctypes.c_int32 * max(n, 1))()
        ms = (ctypes.c_float * max(n, 1))()
        n = self._lib.ekf_profile_flushes(self._h, n, ns, ms)
        if n < 0:
            _check(-n, "ekf_profile_flushes")
        return [(ns[k], ms[k]) for k in range(n)]

    def flush_kernel_name(self, nsteps: int) -> str:
        return self._lib.ekf_flush_kernel_name(self._h, int(nsteps)).decode()

    def result_words(self, e: int = 0) -> list[int]:
        out = (ctypes.c_int32 * 16)()
        _check(self._lib.ekf_debug_result_words(self._h, e, out), "ekf_debug_result_words")
        return list(out)

    def scan_stamps(self) -> list[int]:
        out = (ctypes.c_ulonglong * 32)()
        _check(self._lib.ekf_debug_scan_stamps(self._h, out), "ekf_debug_scan_stamps")
        return list(out)

    def landmark_block_bytes(self) -> int:
        return int(self._lib.ekf_landmark_block_bytes(self._h))

    def profile(self, level: int = 2):
        """HIP-event timing: 0 off, 1 the flush only, 2 also every association kernel
        (True = 2)."""
        level = 2 if level is True else int(level)
        _check(self._lib.ekf_profile_enable(self._h, level), "ekf_profile_enable")

    def profile_read(self):
        s, dd, a = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        k = ctypes.c_int32()
        _check(self._lib.ekf_profile_read(self._h, ctypes.byref(s), ctypes.byref(dd), ctypes.byref(a),
                                          ctypes.byref(k)), "ekf_profile_read")
        return dict(scan_ms=s.value, downdate_ms=dd.value, augment_ms=a.value, launches=k.value)


class Robot:
    """Mirror of `class Robot` (Robot.h:21-77) for one EKF instance on the GPU.

    `localize(lines, rot=None, encoder=None)` follows Robot.cpp:126-904 with
    SIMULATIONOFF == true (Robot.h:18): the encoder pose drives the motion model and `rot` is
    ignored. `lines` is a sequence of (alfa, r, C_AR[4]) or objects with `.alfa`, `.r`,
    `.C_AR` and optional `.lineInterval` [(alfa, r), (alfa, r)] endpoints.
    """

    def __init__(self, x: float, y: float, theta: float, capacity: int = 100,
                 precision: int = PREC_F64, max_lines: int = 20, r_mode: int = R_INTENDED):
        self._ens = Ensemble(capacity, 1, precision, max_lines, r_mode=r_mode)
        self._ens.reset(0, x, y, theta)
        self.xPos, self.yPos, self.thetaPos = float(x), float(y), float(theta)
        self.lineIntervals: list[float] = []
        self.matchesNum = 0
        self.savedLineCount = 0
        self.last = None

    @staticmethod
    def _as_rows(lines):
        rows, intervals = [], []
        for ln in lines:
            if hasattr(ln, "alfa"):
                R = np.asarray(ln.C_AR, dtype=np.float64).reshape(4)
                rows.append([ln.alfa, ln.r, *R])
                intervals.append(getattr(ln, "lineInterval", None))
            else:
                a = np.asarray(ln, dtype=np.float64).reshape(-1)
                rows.append(list(a[:6]))
                intervals.append(None)
        return np.array(rows, dtype=np.float64).reshape(-1, 6), intervals

    def _store_intervals(self, res, intervals):
        # Robot.cpp:870-879: endpoints of every appended line, world frame, float32
        for i, m in enumerate(res["match"]):
            iv = intervals[i] if i < len(intervals) else None
            if m >= 0 or iv is None or len(iv) != 2:
                continue
            for (alfa_r, r_r) in (iv[0], iv[-1]):
                alpha = float(np.float32(alfa_r))
                a = alpha + self.thetaPos
                rr = r_r + self.xPos * math.cos(alpha) + self.yPos * math.sin(alpha)
                self.lineIntervals.append(float(np.float32(math.cos(a) * rr)))
                self.lineIntervals.append(float(np.float32(math.sin(a) * rr)))

    def _commit(self, res, intervals):
        self.xPos, self.yPos, self.thetaPos = (float(v) for v in res["pose"])
        self.matchesNum = res["matches"]
        self.savedLineCount = res["saved"]
        self.last = res
        self._store_intervals(res, intervals)

    def localize(self, lines, rot=None, encoder=None):
        if encoder is None:
            raise EkfError("encoder pose required (SIMULATIONOFF == true, Robot.cpp:140-145)")
        rows, intervals = self._as_rows(lines)
        res = self._ens.localize(np.asarray(encoder, dtype=np.float64)[None], rows[None],
                                 [len(rows)])[0]
        self._commit(res, intervals)

    def predict(self, encoder):
        self._ens.predict(np.asarray(encoder, dtype=np.float64)[None])

    def update(self, lines):
        rows, intervals = self._as_rows(lines)
        res = self._ens.update(rows[None], [len(rows)])[0]
        self._commit(res, intervals)

    def gateLines(self, lines, encoder=None):
        """Which landmark localize would pick for each line taken alone, how far away it is and
        whether a second one passes (the reference has no such member: its association is first-fit
        inside localize, Robot.cpp:313-498). The state is untouched. See Ensemble.gate_lines."""
        rows, _ = self._as_rows(lines)
        return self._ens.gate_lines(0, rows, encoder)

    def gateJoint(self, lines, assign, encoder=None, each=False):
        """Joint compatibility of hypotheses (assign [H, L]: the landmark of each line or -1): per
        hypothesis the stacked innovation's v^T S^-1 v and log det S (the reference has no such
        member). The state is untouched. See Ensemble.gate_joint."""
        rows, _ = self._as_rows(lines)
        return self._ens.gate_joint(0, rows, assign, encoder, each)

    def associateJoint(self, lines, cand, bound, encoder=None, max_nodes: int = 1 << 16):
        """The best jointly compatible assignment of the lines to their candidate landmarks (cand [L, C],
        bound [L + 1]); the reference's association is first-fit and has no such member. The state is
        untouched. See Ensemble.associate_joint."""
        rows, _ = self._as_rows(lines)
        return self._ens.associate_joint(0, rows, cand, bound, encoder, max_nodes)

    def getEllipse(self):
        ok, axii, angle = self._ens.ellipse(0)
        return ok, axii, angle

    def landmarkEllipse(self, j: int):
        """getEllipse's arithmetic (Robot.cpp:73-124) on landmark j's 2x2 block, read without
        draining the flush (the reference has no such member): (ok, axii, angle)."""
        blocks, _, _ = self._ens.query_marginals(0, [int(j)])
        return ellipse_of_block(blocks[0])

    @property
    def P_t0(self) -> np.ndarray:
        return self._ens.download_state(0)[0]

    @property
    def y(self) -> np.ndarray:
        return self._ens.download_state(0, with_P=False)[1]

    def set_state(self, P, y, saved, pose):
        self._ens.upload_state(0, P, y, saved, pose)
        self.xPos, self.yPos, self.thetaPos = (float(v) for v in pose)
        self.savedLineCount = int(saved)
