"""Cost of the instance images' device forms beside the runtime's copy of the same bytes: fp32 storage,
EKF_ARITH_F16X3, T = 20, 8 instances, at N = 4096 and N = 1024, with 19 and with 0 steps pending, for 1,
4 and 7 instances: ekf_export_instances_device, ekf_import_instances_device, the two in a row, and
ekf_resample with as many destinations.

The method of scripts/resample_cost.py: medians of REPS, HIP events on the context stream around the
call with a long device copy enqueued in front, so that the host's work on the table hides behind it
and the events bracket the device's work alone. The yardstick is the runtime's own device-to-device
hipMemcpyAsync of the image bytes, one call per instance, timed the same way in the same run. Prints
one JSON line per N (DESIGN.md §4.4f holds the table)."""
import ctypes
import json
import os
import statistics
import sys

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


def timed(call, reps):
    out = []
    for _ in range(reps):
        check(hip.hipMemcpyAsync(blk.value + BLOCK, blk, BLOCK, D2D, stream), "hipMemcpyAsync")
        check(hip.hipEventRecord(ev0, stream), "hipEventRecord")
        call()
        check(hip.hipEventRecord(ev1, stream), "hipEventRecord")
        check(hip.hipEventSynchronize(ev1), "hipEventSynchronize")
        ms = ctypes.c_float()
        check(hip.hipEventElapsedTime(ctypes.byref(ms), ev0, ev1), "hipEventElapsedTime")
        out.append(ms.value)
    return statistics.median(out)


# instances exported, the slots that take them, and the resample list with as many destinations
CASES = {1: ([0], [7], [0, 1, 2, 3, 4, 5, 6, 0]), 4: ([0, 1, 2, 3], [4, 5, 6, 7], [0, 1, 2, 3, 0, 1, 2, 3]),
         7: ([0] * 7, [1, 2, 3, 4, 5, 6, 7], [0] * 8)}


def run(N):
    w = G.make_world(N)
    st = G.initial_state(w)
    ens = ekf.Ensemble(N, E, ekf.PREC_F32, max_lines=L, flush_interval=T, arith=ekf.ARITH_F16X3)
    for e in range(E):
        ens.init_lowrank(e, st.diag, st.U, st.y, st.saved, st.pose)
    ens.set_stream(stream.value)
    ens.profile(1)
    out = {"N": N, "E": E, "T": T, "reps": REPS}
    step = 0

    def scans(count):
        nonlocal step
        for _ in range(count):
            step += 1
            ens.localize(*G.make_scan(w, step, instances=E, lines=L))

    def measure(pending):
        nbytes = ens.instance_image_bytes()
        img, scratch = ctypes.c_void_p(), ctypes.c_void_p()
        check(hip.hipMalloc(ctypes.byref(img), 7 * nbytes), "hipMalloc")
        check(hip.hipMalloc(ctypes.byref(scratch), 7 * nbytes), "hipMalloc")
        check(hip.hipMemsetAsync(scratch, 0, 7 * nbytes, stream), "hipMemsetAsync")
        out[f"pending_{pending}_image_MB"] = round(nbytes / 1e6, 2)

        def runtime_copy(k):
            for i in range(k):
                check(hip.hipMemcpyAsync(scratch.value + i * nbytes, img.value + i * nbytes, nbytes, D2D, stream),
                      "hipMemcpyAsync")

        for k, (src, dst, rs) in CASES.items():
            descs = ens.export_instances_device(src, img.value)    # (first use allocates the table)
            ens.import_instances_device(dst, img.value, descs)
            ens.resample(rs)
            check(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
            ex = timed(lambda: ens.export_instances_device(src, img.value), REPS)
            im = timed(lambda: ens.import_instances_device(dst, img.value, descs), REPS)

            def both():
                d = ens.export_instances_device(src, img.value)
                ens.import_instances_device(dst, img.value, d)

            bo = timed(both, REPS)
            rs_ms = timed(lambda: ens.resample(rs), REPS)
            ref = timed(lambda: runtime_copy(k), REPS)
            moved = 2 * k * nbytes
            out[f"pending_{pending}_k_{k}"] = {
                "export_ms": round(ex, 4), "import_ms": round(im, 4), "export_import_ms": round(bo, 4),
                "resample_ms": round(rs_ms, 4), "memcpy_ms": round(ref, 4), "export_ratio": round(ex / ref, 3),
                "import_ratio": round(im / ref, 3), "export_GBps": round(moved / ex / 1e6, 1),
                "import_GBps": round(moved / im / 1e6, 1), "memcpy_GBps": round(moved / ref / 1e6, 1)}
        check(hip.hipStreamSynchronize(stream), "hipStreamSynchronize")
        hip.hipFree(img)
        hip.hipFree(scratch)

    scans(T - 1)
    measure(T - 1)
    assert ens.profile_flushes() == []          # nothing flushed: the calls left the group pending
    scans(1)
    assert [n for n, _ in ens.profile_flushes()] == [T]
    measure(0)
    ens.close()
    print(json.dumps(out), flush=True)


for size in SIZES:
    run(size)
