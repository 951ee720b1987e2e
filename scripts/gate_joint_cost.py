"""Cost of the joint gate's device form (ekf_gate_joint_device) beside ekf_gate_lines_device and the
association kernel of the same context: N = 4096, 8 instances, 8 lines, 256 hypotheses per instance,
fp32 storage, EKF_ARITH_F16X3, T = 20. Timed mid-group (19 steps pending: every block behind the full
pll_block chain) and just after the group's flush (0 pending); HIP events on the context's stream
bracket the launch, median of 20, wall time beside them. Hypotheses: "mixed" perturbs the gate's own
answer (each line keeps its first match, takes a random landmark, or is left out, a third each);
"full" assigns every line (2m = 16). A second context (N = 1024, max_lines = 64, EKF_ARITH_EXACT, nothing pending)
times 256 hypotheses of m = 64 (2m = 128), the factorisation's largest case. scan_ms is
ekf_profile_read's average of the association kernels run so far. Prints one JSON line (DESIGN.md
§4.4d holds the table)."""
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
H = int(os.environ.get("H", 256))
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


out = {"N": N, "E": E, "T": T, "L": L, "H": H, "reps": REPS}
d_hits = device(np.zeros(E * L * ctypes.sizeof(ekf.ekf_gate_hit), dtype=np.uint8))
d_jhits = device(np.zeros(E * H * ctypes.sizeof(ekf.EkfJointHit), dtype=np.uint8))
d_each = device(np.zeros((E, H, L)))
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
    gate = lambda: ens.gate_lines_device(bufs[0].value, bufs[1].value, bufs[2].value, d_hits.value, 0)   # noqa: E731
    gate()                                                             # (first use allocates)
    check(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")   # (ekf_sync would drain the pending steps)
    out[tag + "_gate_lines_ms"] = timed(gate, REPS)
    raw = (ekf.ekf_gate_hit * (E * L))()
    check(hip.hipMemcpy(ctypes.byref(raw), d_hits, ctypes.sizeof(raw), 2), "hipMemcpy")
    first = np.array([h.first for h in raw], dtype=np.int32).reshape(E, 1, L)
    rng = np.random.default_rng(17)
    rand = rng.integers(0, st.saved, size=(E, H, L)).astype(np.int32)
    pick = rng.integers(0, 3, size=(E, H, L))
    mixed = np.where(pick == 0, first, np.where(pick == 1, rand, -1)).astype(np.int32)
    full = np.where(first >= 0, first, rand).astype(np.int32)
    full[:, 1:, :] = np.where(pick[:, 1:, :] == 0, full[:, 1:, :], rand[:, 1:, :])
    for name, asg in (("mixed", mixed), ("full", full)):
        d_asg = device(asg)
        for each, suffix in ((d_each.value, "_with_each_ms"), (0, "_ms")):
            call = lambda: ens.gate_joint_device(bufs[0].value, bufs[1].value, bufs[2].value, d_asg.value, H,   # noqa: E731
                                                 d_jhits.value, each)
            call()
            check(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
            out[f"{tag}_joint_{name}{suffix}"] = timed(call, REPS)
        jr = (ekf.EkfJointHit * (E * H))()
        check(hip.hipMemcpy(ctypes.byref(jr), d_jhits, ctypes.sizeof(jr), 2), "hipMemcpy")
        out[f"{tag}_joint_{name}_mean_m"] = round(float(np.mean([h.m for h in jr])), 2)
        out[f"{tag}_joint_{name}_singular"] = sum(h.status != 0 for h in jr)
        hip.hipFree(d_asg)
    for b in bufs:
        hip.hipFree(b)


scans(T - 1)                      # 19 pending
assert ens.profile_flushes() == []
measure("pending_%d" % (T - 1))
assert ens.profile_flushes() == []    # the queries flushed nothing
scans(1)                          # the group's flush
assert len(ens.profile_flushes()) == 1
measure("pending_0")
pr = ens.profile_read()
out["scan_ms"] = round(pr["scan_ms"], 4)
out["flush_ms"] = round(pr["downdate_ms"], 4)

# the widest case: 2m = 128
NW, LW = int(os.environ.get("NW", 1024)), 64
ww = G.make_world(NW)
sw = G.initial_state(ww)
wide = ekf.Ensemble(NW, E, ekf.PREC_F32, max_lines=LW, flush_interval=8)   # (the split arithmetics stop at 8 lines)
for e in range(E):
    wide.init_lowrank(e, sw.diag, sw.U, sw.y, sw.saved, sw.pose)
wide.set_stream(stream.value)
enc, lines, nl = G.make_scan(ww, 1, instances=E, lines=LW)
rng = np.random.default_rng(19)
asg = np.stack([np.stack([rng.permutation(sw.saved)[:LW] for _ in range(H)]) for _ in range(E)]).astype(np.int32)
bufs = [device(enc), device(lines), device(nl.astype(np.int32)), device(asg),
        device(np.zeros(E * H * ctypes.sizeof(ekf.EkfJointHit), dtype=np.uint8))]
call = lambda: wide.gate_joint_device(bufs[0].value, bufs[1].value, bufs[2].value, bufs[3].value, H, bufs[4].value, 0)   # noqa: E731
call()
check(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
out["wide_N"], out["wide_m"] = NW, LW
out["wide_joint_ms"] = timed(call, REPS)
jr = (ekf.EkfJointHit * (E * H))()
check(hip.hipMemcpy(ctypes.byref(jr), bufs[4], ctypes.sizeof(jr), 2), "hipMemcpy")
out["wide_singular"] = sum(h.status != 0 for h in jr)
print(json.dumps(out))
