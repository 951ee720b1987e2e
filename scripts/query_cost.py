"""Cost of the covariance queries (ekf_query_joint / ekf_query_marginals / ekf_query_joint_device)
mid-group, beside ekf_download_state with P, on one context: N = 4096, 8 instances, fp32 storage,
EKF_ARITH_F16X3, T = 20, ten steps pending. HIP events on the context's stream bracket each call
(kernel + copy for the host forms, the kernel alone for the device form); wall time beside them.
Prints one JSON line ("Covariance queries", holds the table)."""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from slam_ros_amd import ekf, scan_gen as G   # noqa: E402

N = int(os.environ.get("N", 4096))
E = int(os.environ.get("E", 8))
T = int(os.environ.get("T", 20))
PEND = int(os.environ.get("PEND", 10))
K = int(os.environ.get("K", 64))
REPS = int(os.environ.get("REPS", 20))

ekf.load_library()
hip = ctypes.CDLL("libamdhip64.so.7")
hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
hip.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
hip.hipEventSynchronize.argtypes = [ctypes.c_void_p]
hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: hip error {rc}")


w = G.make_world(N)
st = G.initial_state(w)
ens = ekf.Ensemble(N, E, ekf.PREC_F32, max_lines=8, flush_interval=T, arith=ekf.ARITH_F16X3)
for e in range(E):
    ens.init_lowrank(e, st.diag, st.U, st.y, st.saved, st.pose)
stream = ctypes.c_void_p()
check(hip.hipStreamCreate(ctypes.byref(stream)), "hipStreamCreate")
ens.set_stream(stream.value)
ens.profile(1)
ev0, ev1 = ctypes.c_void_p(), ctypes.c_void_p()
check(hip.hipEventCreate(ctypes.byref(ev0)), "hipEventCreate")
check(hip.hipEventCreate(ctypes.byref(ev1)), "hipEventCreate")
for step in range(1, PEND + 1):
    enc, lines, nl = G.make_scan(w, step, instances=E)
    ens.localize(enc, lines, nl)


def timed(call, reps):
    """median (event ms, wall ms) of `call`, which leaves its work on the stream or waits for it"""
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


rng = np.random.default_rng(1)
lm = rng.integers(0, st.saved, K).astype(np.int32)
nq = 3 + 2 * K
d_lm, d_cov, d_mean = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
check(hip.hipMalloc(ctypes.byref(d_lm), 4 * E * K), "hipMalloc")
check(hip.hipMalloc(ctypes.byref(d_cov), 8 * E * nq * nq), "hipMalloc")
check(hip.hipMalloc(ctypes.byref(d_mean), 8 * E * nq), "hipMalloc")
lists = np.ascontiguousarray(np.tile(lm, (E, 1)))
check(hip.hipMemcpy(d_lm, lists.ctypes.data_as(ctypes.c_void_p), lists.nbytes, 1), "hipMemcpy")

out = {"N": N, "E": E, "T": T, "pending": PEND, "K": K, "reps": REPS}
ens.query_joint(0, lm)          # (first use allocates the context's query buffers)
ens.query_marginals(0)
out["joint_host_ms"] = timed(lambda: ens.query_joint(0, lm), REPS)
out["joint_device_all_instances_ms"] = timed(
    lambda: ens.query_joint_device(d_lm.value, K, d_cov.value, d_mean.value), REPS)
out["marginals_host_ms"] = timed(lambda: ens.query_marginals(0), REPS)
assert ens.profile_flushes() == []
# the dense download drains first: the first call flushes the pending steps (and allocates the n × n
# scratch), the later ones find nothing pending
out["download_P_first_ms"] = timed(lambda: ens.download_state(0), 1)
out["download_P_ms"] = timed(lambda: ens.download_state(0), 3)
out["dense_scratch_MB"] = round(8 * ens.n * ens.n / 1e6, 1)
print(json.dumps(out))
