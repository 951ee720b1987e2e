"""Cost of the gate query's device form (ekf_gate_lines_device) beside the association kernel of the
same context: N = 4096, 8 instances, 8 lines, fp32 storage, EKF_ARITH_F16X3, T = 20. Timed mid-group
(19 steps pending: every landmark's diagonal block behind the full pll_block chain) and just after
the group's flush (0 pending), with and without the distance matrix; HIP events on the context's
stream bracket the two launches, wall time beside them. scan_ms is ekf_profile_read's average of the
association kernels run so far. Prints one JSON line (DESIGN.md §4.4c holds the table)."""
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
L = int(os.environ.get("L", 8))
REPS = int(os.environ.get("REPS", 20))

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


w = G.make_world(N)
st = G.initial_state(w)
ens = ekf.Ensemble(N, E, ekf.PREC_F32, max_lines=L, flush_interval=T, arith=ekf.ARITH_F16X3)
for e in range(E):
    ens.init_lowrank(e, st.diag, st.U, st.y, st.saved, st.pose)
stream = ctypes.c_void_p()
check(hip.hipStreamCreate(ctypes.byref(stream)), "hipStreamCreate")
ens.set_stream(stream.value)
ens.profile(2)
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


def device(host):
    p = ctypes.c_void_p()
    host = np.ascontiguousarray(host)
    check(hip.hipMalloc(ctypes.byref(p), host.nbytes), "hipMalloc")
    check(hip.hipMemcpy(p, host.ctypes.data_as(ctypes.c_void_p), host.nbytes, 1), "hipMemcpy")
    return p


out = {"N": N, "E": E, "T": T, "L": L, "reps": REPS}
d_hits = device(np.zeros(E * L * ctypes.sizeof(ekf.ekf_gate_hit), dtype=np.uint8))
d_d2 = device(np.zeros((E, L, N)))
step = 0


def scans(count):
    global step
    for _ in range(count):
        step += 1
        enc, lines, nl = G.make_scan(w, step, instances=E, lines=L)
        ens.localize(enc, lines, nl)


def measure(tag):
    enc, lines, nl = G.make_scan(w, step + 1, instances=E, lines=L)   # the scan that would come next
    bufs = [device(enc), device(lines), device(nl.astype(np.int32))]
    ens.gate_lines_device(bufs[0].value, bufs[1].value, bufs[2].value, d_hits.value, d_d2.value)   # (first use allocates)
    check(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")   # (ekf_sync would drain the pending steps)
    out[tag + "_with_d2_ms"] = timed(
        lambda: ens.gate_lines_device(bufs[0].value, bufs[1].value, bufs[2].value, d_hits.value, d_d2.value), REPS)
    out[tag + "_hits_only_ms"] = timed(
        lambda: ens.gate_lines_device(bufs[0].value, bufs[1].value, bufs[2].value, d_hits.value, 0), REPS)
    raw = (ekf.ekf_gate_hit * (E * L))()
    check(hip.hipMemcpy(ctypes.byref(raw), d_hits, ctypes.sizeof(raw), 2), "hipMemcpy")
    out[tag + "_lines_with_a_hit"] = sum(h.first >= 0 for h in raw)
    for b in bufs:
        hip.hipFree(b)


scans(T - 1)                      # 19 pending
assert ens.profile_flushes() == []
measure("pending_%d" % (T - 1))
assert ens.profile_flushes() == []    # the gate flushed nothing
scans(1)                          # the group's flush
assert len(ens.profile_flushes()) == 1
measure("pending_0")
pr = ens.profile_read()
out["scan_ms"] = round(pr["scan_ms"], 4)
out["flush_ms"] = round(pr["downdate_ms"], 4)
print(json.dumps(out))
