"""Cost of the landmark-pair call's device form (ekf_gate_landmarks_device): N = 256, 1024 and 4096, 8
instances, fp32 storage, EKF_ARITH_F16X3, T = 20. Timed with nothing pending (the state as initialised)
and mid-group (19 steps pending: every block behind the full pll_blocks chain), with and without the
distance matrix; HIP events on the context's stream bracket the two launches, wall time beside them. At
N = 1024 the joint query of all N landmarks (ekf_query_joint_device, K = N) is timed on the same state in
the same process: the call that would otherwise hand the host the blocks. Prints one JSON line per N
(DESIGN.md §4.4i holds the table)."""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from slam_ros_amd import ekf, scan_gen as G   # noqa: E402

SIZES = [int(s) for s in os.environ.get("N", "256,1024,4096").split(",")]
QUERY_AT = int(os.environ.get("QUERY_AT", 1024))
E = int(os.environ.get("E", 8))
T = int(os.environ.get("T", 20))
L = int(os.environ.get("L", 8))
REPS = int(os.environ.get("REPS", 10))
GATE = 3.0

ekf.load_library()
hip = ctypes.CDLL("libamdhip64.so.7")
hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
hip.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
hip.hipEventSynchronize.argtypes = [ctypes.c_void_p]
hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
hip.hipFree.argtypes = [ctypes.c_void_p]
hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: hip error {rc}")


stream = ctypes.c_void_p()
check(hip.hipStreamCreate(ctypes.byref(stream)), "hipStreamCreate")
ev0, ev1 = ctypes.c_void_p(), ctypes.c_void_p()
check(hip.hipEventCreate(ctypes.byref(ev0)), "hipEventCreate")
check(hip.hipEventCreate(ctypes.byref(ev1)), "hipEventCreate")


def timed(call, reps):
    """median (event ms, wall ms) of `call`, which leaves its work on the stream"""
    evs, walls = [], []
    for _ in range(reps):
        check(hip.hipEventRecord(ev0, stream), "hipEventRecord")
        t = time.perf_counter()
        call()
        check(hip.hipEventRecord(ev1, stream), "hipEventRecord")
        check(hip.hipEventSynchronize(ev1), "hipEventSynchronize")
        walls.append((time.perf_counter() - t) * 1e3)
        ms = ctypes.c_float()
        check(hip.hipEventElapsedTime(ctypes.byref(ms), ev0, ev1), "hipEventElapsedTime")
        evs.append(ms.value)
    return round(statistics.median(evs), 4), round(statistics.median(walls), 4)


def device(nbytes):
    p = ctypes.c_void_p()
    check(hip.hipMalloc(ctypes.byref(p), nbytes), "hipMalloc")
    return p


def run(N):
    w = G.make_world(N)
    st = G.initial_state(w)
    ens = ekf.Ensemble(N, E, ekf.PREC_F32, max_lines=L, flush_interval=T, arith=ekf.ARITH_F16X3)
    for e in range(E):
        ens.init_lowrank(e, st.diag, st.U, st.y, st.saved, st.pose)
    ens.set_stream(stream.value)
    ens.profile(2)
    out = {"N": N, "E": E, "T": T, "saved": int(st.saved), "reps": REPS}
    d_hits = device(E * N * ctypes.sizeof(ekf.ekf_pair_hit))
    d_d2 = device(E * N * N * 8)
    nq = 3 + 2 * N
    d_cov = device(E * nq * nq * 8) if N == QUERY_AT else None
    d_mean = device(E * nq * 8) if N == QUERY_AT else None
    d_lm = None
    if N == QUERY_AT:
        lm = np.ascontiguousarray(np.tile(np.arange(N, dtype=np.int32), (E, 1)))
        d_lm = device(lm.nbytes)
        check(hip.hipMemcpy(d_lm, lm.ctypes.data_as(ctypes.c_void_p), lm.nbytes, 1), "hipMemcpy")

    def measure(tag):
        ens.gate_landmarks_device(GATE, d_hits.value, d_d2.value)          # (first use allocates)
        check(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")   # (ekf_sync would drain the pending steps)
        out[tag + "_with_d2_ms"] = timed(lambda: ens.gate_landmarks_device(GATE, d_hits.value, d_d2.value), REPS)
        out[tag + "_hits_only_ms"] = timed(lambda: ens.gate_landmarks_device(GATE, d_hits.value, 0), REPS)
        if d_cov:
            ens.query_joint_device(d_lm.value, N, d_cov.value, d_mean.value)
            check(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
            out[tag + "_query_joint_ms"] = timed(lambda: ens.query_joint_device(d_lm.value, N, d_cov.value, d_mean.value), REPS)
        raw = np.zeros(E * N, dtype=ekf.PAIR_HIT_DTYPE)
        check(hip.hipMemcpy(raw.ctypes.data_as(ctypes.c_void_p), d_hits, raw.nbytes, 2), "hipMemcpy")
        out[tag + "_landmarks_with_a_partner"] = int((raw["npass"] > 0).sum())

    measure("pending_0")
    for step in range(1, T):
        enc, lines, nl = G.make_scan(w, step, instances=E, lines=L)
        ens.localize(enc, lines, nl)
    assert ens.profile_flushes() == []
    measure("pending_%d" % (T - 1))
    assert ens.profile_flushes() == []    # the call flushed nothing
    for p in (d_hits, d_d2, d_cov, d_mean, d_lm):
        if p:
            hip.hipFree(p)
    ens.close()
    return out


for n in SIZES:
    print(json.dumps(run(n)), flush=True)
