"""Cost of the ensemble's hypothesis loop with its four device stages (ekf_gate_candidates_device,
ekf_assoc_weights_device, ekf_resample_plan_device, ekf_resample_device) beside the recipe they replace:
N = 4096, 8 instances, 8 lines, C = 4, fp32 storage, EKF_ARITH_F16X3, T = 20 (scripts/assoc_joint_cost.py's
configuration), 19 steps pending.
  (a) the device chain: gate, candidates, search, weights, plan, copy enqueued on the context's stream with
      no host read in between; HIP events bracket the six calls, wall time beside them, median of REPS.
      The stages are also timed one by one (events), so the chain can be held against the sum of its
      kernels. The prior keeps two instances alive so that every repetition overwrites the same number.
  (b) today's recipe on the same context: download d2, gate_candidates, upload, search, download the hits,
      numpy weights, resample_plan, ekf_resample; wall time to the end of the copy.
  (c) ekf_resample_device beside ekf_resample with the same list, 1, 4 and 7 overwritten instances, with 19
      and with 0 steps pending: median of REPS, three repeats (their spread is the run's noise), ms and
      GB/s of the bytes read plus written.
Prints one JSON line (DESIGN.md §4.4h holds the tables)."""
import ctypes
import json
import math
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
C = int(os.environ.get("C", 4))
REPS = int(os.environ.get("REPS", 20))
LOOSE, CONF, U = 30.0, 0.99, 0.3125

ekf.load_library()
hip = ctypes.CDLL("libamdhip64.so.7")
hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
hip.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
hip.hipEventSynchronize.argtypes = [ctypes.c_void_p]
hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: hip error {rc}")


stream = ctypes.c_void_p()
check(hip.hipStreamCreate(ctypes.byref(stream)), "hipStreamCreate")
ev0, ev1 = ctypes.c_void_p(), ctypes.c_void_p()
check(hip.hipEventCreate(ctypes.byref(ev0)), "hipEventCreate")
check(hip.hipEventCreate(ctypes.byref(ev1)), "hipEventCreate")


def timed(call, reps=REPS):
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


def wall(call, reps):
    """median wall ms of `call`, which ends with the stream idle"""
    walls = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        check(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
        walls.append((time.perf_counter() - t) * 1e3)
    return round(statistics.median(walls), 4)


def device(host):
    p = ctypes.c_void_p()
    host = np.ascontiguousarray(host)
    check(hip.hipMalloc(ctypes.byref(p), host.nbytes), "hipMalloc")
    check(hip.hipMemcpy(p, host.ctypes.data_as(ctypes.c_void_p), host.nbytes, 1), "hipMemcpy")
    return p


def upload(p, host):
    host = np.ascontiguousarray(host)
    check(hip.hipMemcpy(p, host.ctypes.data_as(ctypes.c_void_p), host.nbytes, 1), "hipMemcpy")


def download(p, dtype, shape):
    host = np.zeros(shape, dtype=dtype)
    check(hip.hipMemcpy(host.ctypes.data_as(ctypes.c_void_p), p, host.nbytes, 2), "hipMemcpy")
    return host


out = {"N": N, "E": E, "T": T, "L": L, "C": C, "reps": REPS, "gate": LOOSE, "u": U}
w = G.make_world(N)
st = G.initial_state(w)
ens = ekf.Ensemble(N, E, ekf.PREC_F32, max_lines=L, flush_interval=T, arith=ekf.ARITH_F16X3)
for e in range(E):
    ens.init_lowrank(e, st.diag, st.U, st.y, st.saved, st.pose)
ens.set_stream(stream.value)
ens.profile(1)
AH = ctypes.sizeof(ekf.EkfAssocHit)
d_ghits = device(np.zeros(E * L * ctypes.sizeof(ekf.ekf_gate_hit), dtype=np.uint8))
d_d2 = device(np.zeros((E, L, N)))
d_cand = device(np.zeros((E, L, C), dtype=np.int32))
d_hits = device(np.zeros(E * AH, dtype=np.uint8))
d_weights = device(np.zeros(E))
d_src = device(np.zeros(E, dtype=np.int32))
d_info = device(np.zeros(ctypes.sizeof(ekf.EkfPlanInfo), dtype=np.uint8))
d_status = device(np.zeros(1, dtype=np.int32))
bound = ekf.chi2_bounds(L, CONF)
d_bound = device(bound)
# two instances stay alive whatever the scores are: every repetition overwrites the same instances
prior = np.full(E, -1e4)
prior[[1, E - 2]] = 0.0
d_prior = device(prior)
step = 0


def scans(count):
    global step
    for _ in range(count):
        step += 1
        enc, lines, nl = G.make_scan(w, step, instances=E, lines=L)
        ens.localize(enc, lines, nl)


scans(T - 1)                      # 19 pending
assert ens.profile_flushes() == []
enc, lines, nl = G.make_scan(w, step + 1, instances=E, lines=L)   # the scan that would come next
nl = nl.astype(np.int32)
d_enc, d_lines, d_nl = device(enc), device(lines), device(nl)

stages = {
    "gate": lambda: ens.gate_lines_device(d_enc.value, d_lines.value, d_nl.value, d_ghits.value, d_d2.value),
    "candidates": lambda: ens.gate_candidates_device(d_d2.value, d_nl.value, C, LOOSE, d_cand.value),
    "search": lambda: ens.associate_joint_device(d_enc.value, d_lines.value, d_nl.value, d_cand.value, C, d_bound.value,
                                                 d_hits.value),
    "weights": lambda: ens.assoc_weights_device(d_hits.value, d_nl.value, d_weights.value, 0.0, d_prior.value),
    "plan": lambda: ens.resample_plan_device(d_weights.value, U, d_src.value, math.inf, d_info.value),
    "copy": lambda: ens.resample_device(d_src.value, d_status.value),
}


def chain():
    for call in stages.values():
        call()


chain()                           # (first use allocates; the instances are now the survivors and their copies)
check(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
info = (ekf.EkfPlanInfo * 1)()
check(hip.hipMemcpy(ctypes.byref(info), d_info, ctypes.sizeof(info), 2), "hipMemcpy")
out["chain_copies"] = info[0].copies
out["chain_src"] = download(d_src, np.int32, (E,)).tolist()
out["chain_status"] = int(download(d_status, np.int32, (1,))[0])
out["chain_ms"] = timed(chain)
for name, call in stages.items():
    out[f"stage_{name}_ms"] = timed(call)[0]
out["stages_sum_ms"] = round(sum(out[f"stage_{k}_ms"] for k in stages), 4)


def recipe():
    """Today's loop: three host stops."""
    stages["gate"]()
    check(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
    d2 = download(d_d2, np.float64, (E, L, N))
    cand = np.stack([ekf.gate_candidates(d2[e], C, LOOSE) for e in range(E)])
    upload(d_cand, cand)
    stages["search"]()
    check(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
    raw = (ekf.EkfAssocHit * E)()
    check(hip.hipMemcpy(ctypes.byref(raw), d_hits, ctypes.sizeof(raw), 2), "hipMemcpy")
    lw = np.array([-(h.d2 + h.logdet) / 2 - h.m * math.log(2 * math.pi) if not h.status & ekf.AS_INVALID else -np.inf
                   for h in raw]) + prior
    ens.resample(ekf.resample_plan(np.exp(lw - lw.max()), U))


recipe()
check(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
out["recipe_wall_ms"] = wall(recipe, REPS)
out["chain_wall_ms"] = wall(chain, REPS)
assert ens.profile_flushes() == []    # nothing above flushed


# (c) the copy alone, device form beside host form
def bytes_per_instance():
    return ens.instance_image_bytes()   # (what an instance owns now, 16-byte padded per item)


def copies(tag):
    per = bytes_per_instance()
    out[f"{tag}_instance_mb"] = round(per / 1e6, 2)
    for k in (1, 4, 7):
        src = list(range(E))
        for e in range(1, k + 1):
            src[e] = 0
        upload(d_src, np.array(src, dtype=np.int32))
        host = lambda: ens.resample(src)                                     # noqa: E731
        dev = lambda: ens.resample_device(d_src.value, d_status.value)       # noqa: E731
        host(), dev()
        check(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
        for name, call in (("host", host), ("device", dev)):
            runs = [timed(call)[0] for _ in range(3)]
            out[f"{tag}_{k}_{name}_ms"] = runs
            out[f"{tag}_{k}_{name}_gbs"] = round(2 * k * per / (statistics.median(runs) * 1e-3) / 1e9, 1)


copies("pending_%d" % (T - 1))
assert ens.profile_flushes() == []
scans(1)                          # the group's flush
assert len(ens.profile_flushes()) == 1
copies("pending_0")
print(json.dumps(out))
