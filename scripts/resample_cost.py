"""Cost of ekf_resample beside what it replaces: fp32 storage, EKF_ARITH_F16X3, T = 20, 8 instances, at
N = 4096 and N = 1024, with 19 and with 0 steps pending, overwriting 1, 4 and 7 of the 8 instances.

Three figures per case, medians of REPS: the call (HIP events on the context stream around it; a long
device copy is enqueued in front, so the host's work on the table hides behind it and the events
bracket the device's work alone), the call's wall time on an idle stream, and the runtime's own
device-to-device hipMemcpyAsync of the same landmark-block bytes, one call per destination, timed the
same way. GB/s counts bytes read plus bytes written. Last, one ekf_download_state + ekf_upload_state
round trip of one instance (wall time): the route the call replaces. Prints one JSON line per N
(DESIGN.md §4.4e holds the table)."""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from slam_ros_amd import ekf, scan_gen as G   # noqa: E402

SIZES = [int(v) for v in os.environ.get("N", "4096,1024").split(",")]
E = int(os.environ.get("E", 8))
T = int(os.environ.get("T", 20))
L = int(os.environ.get("L", 8))
REPS = int(os.environ.get("REPS", 20))

ekf.load_library()
hip = ctypes.CDLL("libamdhip64.so.7")
hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
hip.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
hip.hipEventSynchronize.argtypes = [ctypes.c_void_p]
hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
hip.hipFree.argtypes = [ctypes.c_void_p]
hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
D2D = 3


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: hip error {rc}")


stream = ctypes.c_void_p()
check(hip.hipStreamCreate(ctypes.byref(stream)), "hipStreamCreate")
ev0, ev1 = ctypes.c_void_p(), ctypes.c_void_p()
check(hip.hipEventCreate(ctypes.byref(ev0)), "hipEventCreate")
check(hip.hipEventCreate(ctypes.byref(ev1)), "hipEventCreate")
# the copy enqueued in front of a timed call: 256 MB, about a fifth of a millisecond of device work
BLOCK = 256 << 20
blk = ctypes.c_void_p()
check(hip.hipMalloc(ctypes.byref(blk), 2 * BLOCK), "hipMalloc")
check(hip.hipMemsetAsync(blk, 0, 2 * BLOCK, stream), "hipMemsetAsync")


def timed(call, reps, behind_a_copy):
    out = []
    for _ in range(reps):
        if behind_a_copy:
            check(hip.hipMemcpyAsync(blk.value + BLOCK, blk, BLOCK, D2D, stream), "hipMemcpyAsync")
        check(hip.hipEventRecord(ev0, stream), "hipEventRecord")
        t = time.perf_counter()
        call()
        check(hip.hipEventRecord(ev1, stream), "hipEventRecord")
        check(hip.hipEventSynchronize(ev1), "hipEventSynchronize")
        wall = (time.perf_counter() - t) * 1e3
        ms = ctypes.c_float()
        check(hip.hipEventElapsedTime(ctypes.byref(ms), ev0, ev1), "hipEventElapsedTime")
        out.append(ms.value if behind_a_copy else wall)
    return statistics.median(out)


def bytes_per_destination(N, block_bytes, pending):
    """What one overwritten instance receives (csrc/ekf_resample_plan.h): fp32 storage, symmetric
    operands (V rows only), two fp16 planes, max_lines = L <= 8 (kmax = 16)."""
    n, M = 3 + 2 * N, 2 * N
    nb = (M + 31) // 32
    rec = 4 * (16 + 2 * ekf.EKF_MAX_LINES + 4)
    sync = 4 * ((4 + (N + 63) // 64 + 15) // 16 * 16)
    fixed = block_bytes + 2 * 8 * (3 * n + n + 4 * N) + 16 + 48 + 8 + sync
    rows = nb * 64 * 8
    slot = rows * 4 + rows * 2 * 2 + 8 * L * (2 * M + 4) + rec
    return fixed + pending * slot + (rec if pending == 0 else 0)


SOURCES = {1: [0, 1, 2, 3, 4, 5, 6, 0], 4: [0, 1, 2, 3, 0, 1, 2, 3], 7: [0] * 8}


def run(N):
    w = G.make_world(N)
    st = G.initial_state(w)
    ens = ekf.Ensemble(N, E, ekf.PREC_F32, max_lines=L, flush_interval=T, arith=ekf.ARITH_F16X3)
    for e in range(E):
        ens.init_lowrank(e, st.diag, st.U, st.y, st.saved, st.pose)
    ens.set_stream(stream.value)
    ens.profile(1)
    block = ens.landmark_block_bytes()
    scratch = ctypes.c_void_p()
    check(hip.hipMalloc(ctypes.byref(scratch), block * E), "hipMalloc")
    check(hip.hipMemsetAsync(scratch, 0, block * E, stream), "hipMemsetAsync")
    out = {"N": N, "E": E, "T": T, "reps": REPS, "block_MB": round(block / 1e6, 2)}
    step = 0

    def scans(count):
        nonlocal step
        for _ in range(count):
            step += 1
            ens.localize(*G.make_scan(w, step, instances=E, lines=L))

    def runtime_copy(src):
        for d, s in enumerate(src):
            if s != d:
                check(hip.hipMemcpyAsync(scratch.value + d * block, scratch.value + s * block, block, D2D, stream),
                      "hipMemcpyAsync")

    def measure(pending):
        for ndst, src in SOURCES.items():
            moved = 2 * ndst * bytes_per_destination(N, block, pending)
            ens.resample(src)   # (first use allocates the table)
            check(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
            ms = timed(lambda: ens.resample(src), REPS, True)
            wall = timed(lambda: ens.resample(src), REPS, False)
            ref = timed(lambda: runtime_copy(src), REPS, True)
            out[f"pending_{pending}_dst_{ndst}"] = {
                "resample_ms": round(ms, 4), "resample_wall_ms": round(wall, 4), "GBps": round(moved / ms / 1e6, 1),
                "memcpy_block_ms": round(ref, 4), "memcpy_GBps": round(2 * ndst * block / ref / 1e6, 1),
                "ratio_per_destination": round(ms / ref, 3), "MB_moved": round(moved / 1e6, 2)}

    scans(T - 1)
    measure(T - 1)
    assert ens.profile_flushes() == []          # nothing flushed: the calls left the group pending
    scans(1)
    assert [n for n, _ in ens.profile_flushes()] == [T]
    measure(0)
    t = time.perf_counter()
    P, y, saved, pose = ens.download_state(1)
    ens.upload_state(0, P, y, saved, pose)
    out["download_upload_wall_ms"] = round((time.perf_counter() - t) * 1e3, 2)
    ens.close()
    hip.hipFree(scratch)
    print(json.dumps(out), flush=True)


for size in SIZES:
    run(size)
