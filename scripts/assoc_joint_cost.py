"""Cost of the joint-compatibility search's device form (ekf_associate_joint_device) beside the recipe it
replaces, the level-by-level search through ekf_gate_joint's host form (one call per depth and instance):
N = 4096, 8 instances, 8 lines, fp32 storage, EKF_ARITH_F16X3, T = 20, the joint gate's configuration
(scripts/gate_joint_cost.py). Timed mid-group (19 steps pending) and just after the group's flush (0
pending); HIP events on the context's stream bracket the launches, median of 20, wall time beside them.
Candidates: ekf_gate_lines_device's distances through gate_candidates with C = 4, once under the loose gate
of the tests (30) and once under the association's own gate (0.4, where most lines have one candidate).
With max_nodes = 1 the search stops at its first expansion, so that figure is the tables, the launches and
the reduce. A second context (N = 1024, max_lines = 16, EKF_ARITH_EXACT, nothing pending) runs the widest
shape, 16 lines x 4 candidates, with an R so large that every pairing is nearly free: the tree does not
collapse, the budget (2^16) runs out, and time / nodes is the search kernel's rate per scored child, which
sets EKF_ASSOC_MAX_NODES' worst-case run time. Prints one JSON line (DESIGN.md §4.4g holds the table)."""
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
C = int(os.environ.get("C", 4))
REPS = int(os.environ.get("REPS", 20))
LOOSE, OWN, CONF = 30.0, 0.4, 0.99

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


def device(host):
    p = ctypes.c_void_p()
    host = np.ascontiguousarray(host)
    check(hip.hipMalloc(ctypes.byref(p), host.nbytes), "hipMalloc")
    check(hip.hipMemcpy(p, host.ctypes.data_as(ctypes.c_void_p), host.nbytes, 1), "hipMemcpy")
    return p


def read_hits(d_hits, count):
    raw = (ekf.EkfAssocHit * count)()
    check(hip.hipMemcpy(ctypes.byref(raw), d_hits, ctypes.sizeof(raw), 2), "hipMemcpy")
    return raw


def recipe(ctx, e, enc, lines, cand, bound, saved):
    """The hand recipe: per depth one ekf_gate_joint call (host form) on the children of the level, pruned
    by the bound on the host. Returns (assign, m, d2, hypotheses scored)."""
    n = len(lines)
    level, scored = [((), 0, 0.0)], 0
    for i in range(n):
        usable = [int(j) for j in cand[i] if 0 <= j < saved]
        kids = [(k, j) for k, (pre, m, d2) in enumerate(level) for j in usable if j not in pre]
        res = ctx.gate_joint(e, lines, np.array([list(level[k][0]) + [j] + [-1] * (n - i - 1) for k, j in kids],
                                                dtype=np.int32).reshape(-1, n), enc) if kids else []
        scored += len(kids)
        keep = {}
        for (k, j), h in zip(kids, res):
            if h["status"] == 0 and h["d2"] <= bound[h["m"]]:
                keep.setdefault(k, []).append((level[k][0] + (j,), h["m"], h["d2"]))
        level = [x for k, (pre, m, d2) in enumerate(level) for x in keep.get(k, []) + [(pre + (-1,), m, d2)]]
    best = None
    for leaf in level:
        if best is None or leaf[1] > best[1] or (leaf[1] == best[1] and leaf[2] < best[2]):
            best = leaf
    return list(best[0]), best[1], best[2], scored


out = {"N": N, "E": E, "T": T, "L": L, "C": C, "reps": REPS, "loose_gate": LOOSE, "confidence": CONF}
w = G.make_world(N)
st = G.initial_state(w)
ens = ekf.Ensemble(N, E, ekf.PREC_F32, max_lines=L, flush_interval=T, arith=ekf.ARITH_F16X3)
for e in range(E):
    ens.init_lowrank(e, st.diag, st.U, st.y, st.saved, st.pose)
ens.set_stream(stream.value)
ens.profile(2)
d_ghits = device(np.zeros(E * L * ctypes.sizeof(ekf.ekf_gate_hit), dtype=np.uint8))
d_d2 = device(np.zeros((E, L, N)))
d_hits = device(np.zeros(E * ctypes.sizeof(ekf.EkfAssocHit), dtype=np.uint8))
bound = ekf.chi2_bounds(L, CONF)
d_bound = device(bound)
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
    ens.gate_lines_device(bufs[0].value, bufs[1].value, bufs[2].value, d_ghits.value, d_d2.value)
    check(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")   # (ekf_sync would drain the pending steps)
    d2 = np.zeros((E, L, N))
    check(hip.hipMemcpy(d2.ctypes.data_as(ctypes.c_void_p), d_d2, d2.nbytes, 2), "hipMemcpy")
    saved = int(np.sum(np.isfinite(d2[0, 0])))
    for name, gate in (("loose", LOOSE), ("own", OWN)):
        cand = np.stack([ekf.gate_candidates(d2[e], C, gate) for e in range(E)])
        d_cand = device(cand)
        for mn, suffix in ((1 << 16, "_ms"), (1, "_tables_ms")):
            call = lambda: ens.associate_joint_device(bufs[0].value, bufs[1].value, bufs[2].value, d_cand.value, C,   # noqa: E731
                                                      d_bound.value, d_hits.value, mn)
            call()                                                     # (first use allocates)
            check(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
            out[f"{tag}_{name}_assoc{suffix}"] = timed(call, REPS)
            if mn > 1:
                hits = read_hits(d_hits, E)
        nodes = [h.nodes for h in hits]
        out[f"{tag}_{name}_usable"] = round(float(np.mean(np.sum(cand >= 0, axis=(1, 2)))), 2)
        out[f"{tag}_{name}_nodes"] = round(float(np.mean(nodes)), 1)
        out[f"{tag}_{name}_mean_m"] = round(float(np.mean([h.m for h in hits])), 2)
        out[f"{tag}_{name}_status"] = sorted({h.status for h in hits})
        search_ms = out[f"{tag}_{name}_assoc_ms"][0] - out[f"{tag}_{name}_assoc_tables_ms"][0]
        out[f"{tag}_{name}_ns_per_child"] = round(1e6 * search_ms / max(sum(nodes), 1), 1)
        # the recipe on the same inputs: all instances, wall time
        walls, scored, same = [], 0, True
        for rep in range(max(REPS // 4, 3)):
            t = time.perf_counter()
            res = [recipe(ens, e, enc[e], lines[e, :nl[e]], cand[e], bound, saved) for e in range(E)]
            walls.append((time.perf_counter() - t) * 1e3)
        for e in range(E):
            asg, m, dd, sc = res[e]
            scored += sc
            same &= asg == list(hits[e].assign[:nl[e]]) and dd == hits[e].d2
        out[f"{tag}_{name}_recipe_wall_ms"] = round(statistics.median(walls), 3)
        out[f"{tag}_{name}_recipe_scored"] = round(scored / E, 1)
        out[f"{tag}_{name}_recipe_same_bits"] = bool(same)
        hip.hipFree(d_cand)
    for b in bufs:
        hip.hipFree(b)


scans(T - 1)                      # 19 pending
assert ens.profile_flushes() == []
measure("pending_%d" % (T - 1))
assert ens.profile_flushes() == []    # the searches flushed nothing
scans(1)                          # the group's flush
assert len(ens.profile_flushes()) == 1
measure("pending_0")
pr = ens.profile_read()
out["scan_ms"] = round(pr["scan_ms"], 4)

# the search kernel's rate: the widest shape on a tree that does not collapse
NW, LW, CW = int(os.environ.get("NW", 1024)), 16, 4
ww = G.make_world(NW)
sw = G.initial_state(ww)
wide = ekf.Ensemble(NW, E, ekf.PREC_F32, max_lines=LW, flush_interval=8)
for e in range(E):
    wide.init_lowrank(e, sw.diag, sw.U, sw.y, sw.saved, sw.pose)
wide.set_stream(stream.value)
enc, lines, nl = G.make_scan(ww, 1, instances=E, lines=LW)
lines[:, :, 2:6] = np.array([1e8, 0.0, 0.0, 1e8])
cand = np.tile((np.arange(LW * CW) % sw.saved).reshape(1, LW, CW), (E, 1, 1)).astype(np.int32)
bufs = [device(enc), device(lines), device(nl.astype(np.int32)), device(cand), device(np.full(LW + 1, 1e12)),
        device(np.zeros(E * ctypes.sizeof(ekf.EkfAssocHit), dtype=np.uint8))]
out["wide_N"], out["wide_lines"], out["wide_C"] = NW, LW, CW
for mn in (1 << 16, 1):
    call = lambda: wide.associate_joint_device(bufs[0].value, bufs[1].value, bufs[2].value, bufs[3].value, CW,   # noqa: E731
                                               bufs[4].value, bufs[5].value, mn)
    call()
    check(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
    out["wide_assoc_ms" if mn > 1 else "wide_tables_ms"] = timed(call, max(REPS // 4, 3))
    if mn > 1:
        hits = read_hits(bufs[5], E)
nodes = [h.nodes for h in hits]
out["wide_nodes"] = round(float(np.mean(nodes)), 1)
out["wide_mean_m"] = round(float(np.mean([h.m for h in hits])), 2)
out["wide_status"] = sorted({h.status for h in hits})
rate = 1e6 * (out["wide_assoc_ms"][0] - out["wide_tables_ms"][0]) / max(float(np.mean(nodes)), 1.0)
out["wide_ns_per_child_per_instance"] = round(rate, 1)
out["max_nodes_worst_case_s"] = round(rate * 1e-9 * ekf.ASSOC_MAX_NODES, 2)
print(json.dumps(out))
