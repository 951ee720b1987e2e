"""Covariance queries without a drain (slam_ekf.h ekf_query_joint / ekf_query_marginals /
ekf_query_joint_device): blocks of chosen landmarks read on the device with the pending steps of
the flush group applied on read, against a twin context flushed and drained after every scan.

CPU: the header, the binding's export list, the NULL-context returns. GPU: bit identity mid-group
under EKF_ARITH_EXACT (every storage precision, both schedules, partial tiles, symmetric and stored
U operands), the parity bar on the split arithmetics, the device form, the errors, the drop-in.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from slam_ros_amd import scan_gen as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUERY_FUNCTIONS = ("ekf_query_joint", "ekf_query_marginals", "ekf_query_joint_device")


def rows_of(landmarks):
    rows = [0, 1, 2]
    for j in landmarks:
        rows += [3 + 2 * int(j), 4 + 2 * int(j)]
    return np.array(rows)


def marginals_of(P, y, landmarks):
    """(blocks, cross, mean) of a dense P and y, as ekf_query_marginals lays them out."""
    lm = [int(j) for j in landmarks]
    blocks = np.stack([P[3 + 2 * j:5 + 2 * j, 3 + 2 * j:5 + 2 * j] for j in lm])
    cross = np.stack([P[0:3, 3 + 2 * j:5 + 2 * j] for j in lm])
    mean = np.stack([y[3 + 2 * j:5 + 2 * j] for j in lm])
    return blocks, cross, mean


def check_joint(a, b, e, landmarks, where):
    """a's joint query of instance e equals the entries of b's dense state, bit for bit."""
    Pb, yb, _, _ = b.download_state(e)
    rows = rows_of(landmarks)
    cov, mean = a.query_joint(e, landmarks)
    want = Pb[np.ix_(rows, rows)]
    assert np.array_equal(cov, want), (where, e, np.argwhere(cov != want)[:8].tolist())
    assert np.array_equal(mean, yb[rows]), (where, e)
    return Pb, yb


def check_marginals(a, Pb, yb, e, landmarks, where):
    blocks, cross, mean = a.query_marginals(e, landmarks)
    wb, wc, wm = marginals_of(Pb, yb, range(a.capacity) if landmarks is None else landmarks)
    assert np.array_equal(blocks, wb), (where, e, np.argwhere(blocks != wb)[:8].tolist())
    assert np.array_equal(cross, wc), (where, e)
    assert np.array_equal(mean, wm), (where, e)


# ---------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------
def test_header_declares_the_queries():
    from tests.test_abi import declared_functions
    names = declared_functions()
    for fn in QUERY_FUNCTIONS:
        assert fn in names, fn
    src = open(os.path.join(ROOT, "include", "slam_ekf.h")).read()
    assert "#define SLAM_EKF_ABI_VERSION 3" in src   # entry points only: the number stays


def test_binding_exports_the_queries(ekf_mod):
    for fn in QUERY_FUNCTIONS:
        assert fn in ekf_mod.EXPORTED, fn
    for name in ("query_joint", "query_marginals", "query_joint_device"):
        assert callable(getattr(ekf_mod.Ensemble, name))
    assert callable(ekf_mod.Robot.landmarkEllipse)


def test_null_context_is_einval(ekf_mod):
    """No context: EKF_EINVAL before any HIP call (as test_abi.test_cpu_only_calls)."""
    lib = ekf_mod.load_library()
    lm = (ctypes.c_int32 * 2)(0, 1)
    out = (ctypes.c_double * 64)()
    assert lib.ekf_query_joint(None, 0, lm, 2, out, out) == 1
    assert lib.ekf_query_marginals(None, 0, lm, 2, out, out, out) == 1
    assert lib.ekf_query_marginals(None, 0, None, 0, None, None, None) == 1
    assert lib.ekf_query_joint_device(None, None, 0, None, None) == 1


def test_query_driver_compiles(tmp_path, ekf_mod):
    """BasicRobot::landmarkEllipse compiles against the public header (C++11, -Wall -Werror)."""
    build_query_driver(tmp_path, ekf_mod)


def build_query_driver(tmp_path, ekf_mod):
    exe = tmp_path / "query_driver"
    libdir = os.path.dirname(ekf_mod.LIB_PATH)
    subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
                    f"-I{os.path.join(ROOT, 'slam_ros_amd', 'host')}",
                    os.path.join(ROOT, "tests", "cpp", "query_driver.cpp"), "-o", str(exe),
                    f"-L{libdir}", "-lslam_ekf", f"-Wl,-rpath,{libdir}"], check=True)
    return exe


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
def scans_with_extras(w, steps, instances, lines, rng, extra_every):
    """The scans of test_gpu_parity.test_deferred_flush_equals_drained: `lines` re-observations per
    scan plus two random lines (new landmarks) every extra_every-th step."""
    for step in range(1, steps + 1):
        enc, ln, nl = G.make_scan(w, step, instances=instances, lines=lines)
        if extra_every and step % extra_every == 0:
            ex = G.random_lines(rng, 2)[None].repeat(instances, axis=0)
            ln = np.concatenate([ln, ex], axis=1)
            nl = np.full(instances, ln.shape[1], dtype=np.int32)
        yield step, enc, ln, nl


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [0, 1, 2])
@pytest.mark.parametrize("pipeline,T", [(False, 8), (True, 8), (False, 16), (True, 3)])
def test_mid_group_identity(ekf_mod, prec, pipeline, T):
    """After every scan of a deferred-flush trajectory (matches, augmented rows, a capacity reset
    inside a group), the joint query of landmarks on both sides of a tile edge, in both orientations
    and with a duplicate, and the marginals of the whole map equal the dense state of a twin flushed
    and drained after every scan, bit for bit; the queried context ends bit-identical to the twin and
    ran exactly the flushes of a context that was never queried."""
    N, E = 64, 2
    w = G.make_world(N, active=N - 14)
    st = G.initial_state(w)
    a = ekf_mod.Ensemble(N, E, prec, max_lines=8, pipeline=pipeline, flush_interval=T)
    c = ekf_mod.Ensemble(N, E, prec, max_lines=8, pipeline=pipeline, flush_interval=T)
    b = ekf_mod.Ensemble(N, E, prec, max_lines=8)
    for ens in (a, b, c):
        for e in range(E):
            ens.init_lowrank(e, st.diag, st.U, st.y, st.saved, st.pose)
    a.profile(1)
    c.profile(1)
    lm = [40, 3, 16, 15, 3]
    resets = 0
    for step, enc, ln, nl in scans_with_extras(w, 20, E, 6, np.random.default_rng(11), 3):
        ra = a.localize(enc, ln, nl)
        rb = b.localize(enc, ln, nl)
        c.localize(enc, ln, nl)
        resets += ra[0]["reset"]
        for e in range(E):
            assert ra[e]["match"] == rb[e]["match"], (step, e)
            Pb, yb = check_joint(a, b, e, lm, step)      # (b's download drains b: T = 1, every step)
            check_marginals(a, Pb, yb, e, None, step)
    assert resets >= 1
    fa = [n for n, _ in a.profile_flushes()]
    fc = [n for n, _ in c.profile_flushes()]
    assert fa == fc == [T] * (20 // T), (fa, fc)          # the queries never drained
    for e in range(E):
        Pa, ya, sa, pa = a.download_state(e)
        Pb, yb, sb, pb = b.download_state(e)
        assert np.array_equal(Pa, Pb), (e, np.argwhere(Pa != Pb)[:8].tolist())
        assert np.array_equal(ya, yb) and np.array_equal(pa, pb) and sa == sb


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("N,active,margin", [(37, 25, 10), (5, 3, 1)])
def test_partial_tile_and_small_maps(ekf_mod, prec, N, active, margin):
    """M = 74 (a partial last tile) and N = 5: three pending scans (one adds a landmark), the joint
    query of every landmark against the drained twin; K = 0 is the pose block."""
    w = G.make_world(N, active=active)
    st = G.initial_state(w)
    a = ekf_mod.Ensemble(N, 1, prec, max_lines=8, flush_interval=4, reset_margin=margin)
    b = ekf_mod.Ensemble(N, 1, prec, max_lines=8, reset_margin=margin)
    for ens in (a, b):
        ens.init_lowrank(0, st.diag, st.U, st.y, st.saved, st.pose)
    rng = np.random.default_rng(3)
    for step in range(1, 4):
        enc, ln, nl = G.make_scan(w, step, lines=min(6, active))
        if step == 2:
            ln = np.concatenate([ln, G.random_lines(rng, 1)[None]], axis=1)
            nl = np.full(1, ln.shape[1], dtype=np.int32)
        ra = a.localize(enc, ln, nl)[0]
        rb = b.localize(enc, ln, nl)[0]
        assert ra["match"] == rb["match"] and not ra["reset"], step
        Pb, yb = check_joint(a, b, 0, list(range(N)), step)
        check_marginals(a, Pb, yb, 0, None, step)
    assert ra["saved"] == active + 1
    cov, mean = a.query_joint(0, [])
    assert cov.shape == (3, 3) and np.array_equal(cov, a.pose_cov(0)) and np.array_equal(cov, Pb[:3, :3])
    assert np.array_equal(mean, yb[:3])
    assert np.array_equal(a.download_state(0)[0], b.download_state(0)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("r_mode", [0, 1])
def test_symmetric_operands_and_many_workgroups(ekf_mod, r_mode):
    """N = 256, fp32: with EKF_R_INTENDED the U rows are not stored (read as −2^x·V), and an instance
    spans several association workgroups; with EKF_R_AS_WRITTEN the U rows are stored and the block is
    not symmetric. Five pending scans; the values are those ekf_download_state returns."""
    N = 256
    w = G.make_world(N)
    st = G.initial_state(w)
    a = ekf_mod.Ensemble(N, 1, 1, max_lines=8, flush_interval=8, r_mode=r_mode)
    b = ekf_mod.Ensemble(N, 1, 1, max_lines=8, r_mode=r_mode)
    for ens in (a, b):
        ens.init_lowrank(0, st.diag, st.U, st.y, st.saved, st.pose)
    a.profile(1)
    matched = 0
    for step in range(1, 6):
        enc, ln, nl = G.make_scan(w, step)
        ra = a.localize(enc, ln, nl)[0]
        rb = b.localize(enc, ln, nl)[0]
        assert ra["match"] == rb["match"], step
        matched += ra["matches"]
    assert matched > 0
    lm = list(np.random.default_rng(17).integers(0, st.saved, 24)) + [191, 192]
    Pb, yb = check_joint(a, b, 0, lm, "joint")
    check_marginals(a, Pb, yb, 0, None, "marginals")
    check_marginals(a, Pb, yb, 0, lm, "marginals of a list")
    print(f"r_mode {r_mode}: matches {matched}, asymmetric entries {int((Pb[3:, 3:] != Pb[3:, 3:].T).sum())}")
    assert a.profile_flushes() == []      # five steps pending, none flushed
    assert np.array_equal(a.download_state(0)[0], b.download_state(0)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("at", [7, 6])
@pytest.mark.parametrize("arith,prec,T", [(1, 1, 12), (2, 1, 12), (2, 2, 8)])
def test_split_arithmetics_within_the_bar(ekf_mod, arith, prec, T, at):
    """Split arithmetics: the query reads the pending steps by the exact per-element chain, the
    flush of the same group by split products, so mid-group the joint query of every saved landmark
    and the drained dense P agree to twice the per-group bar (1e-6 fp32 storage, 1e-3 fp16: each is
    held to the bar against the fp64 result from the same base). At step 7 the drain's odd partial
    group takes the EXACT flush forms; at step 6 it takes the split flush. With fp16 storage every
    value is a stored value: the group's one rounding was applied.

    Measured ‖Q − P‖_F / ‖P‖_F (printed on every run), step 7: BF16X6 fp32 0, F16X3 fp32 0 (the
    same exact chain on both sides), F16X3 fp16 5.98e-4 (the exact flush rounds after every step, the
    query once). Step 6: BF16X6 fp32 4.48e-7, F16X3 fp32 3.25e-7, F16X3 fp16 8.51e-6."""
    N = 256
    bar = {1: 1e-6, 2: 1e-3}[prec]
    w = G.make_world(N)
    st = G.initial_state(w)
    a = ekf_mod.Ensemble(N, 1, prec, max_lines=8, flush_interval=T, arith=arith)
    a.init_lowrank(0, st.diag, st.U, st.y, st.saved, st.pose)
    for step in range(1, at + 1):
        enc, ln, nl = G.make_scan(w, step)
        r = a.localize(enc, ln, nl)[0]
        assert r["status"] == 0 and r["matches"] == 8, (step, r)
    saved = r["saved"]
    rows = rows_of(range(saved))
    Q, mean = a.query_joint(0, list(range(saved)))
    P, y, s, _ = a.download_state(0)      # drains: the flush of the pending steps
    assert s == saved
    want = P[np.ix_(rows, rows)]
    ratio = np.linalg.norm(Q - want) / np.linalg.norm(want)
    print(f"query vs drained flush ({a.flush_kernel_name(at)}): arith {arith} prec {prec} T {T} step {at}: "
          f"{ratio:.3e} (bound {2 * bar:.0e})")
    assert ratio <= 2 * bar, ratio
    assert np.array_equal(mean, y[rows])
    assert np.array_equal(Q[:3], want[:3]) and np.array_equal(Q[:, :3], want[:, :3])   # the fp64 strip
    if prec == 2:
        ex = a.storage_exponent(0)
        ll = Q[3:, 3:]
        stored = (ll * 2.0 ** ex).astype(np.float16).astype(np.float64) * 2.0 ** -ex
        assert np.array_equal(stored, ll)


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline", [False, True])
def test_device_form(ekf_mod, pipeline):
    """ekf_query_joint_device: a different list per instance, results in device memory equal to the
    host form's; an index of N gives NaN in exactly that landmark's rows, columns and mean entries;
    the trajectory continues bit-identical to the twin (pipelined: the drain that follows the query
    must wait for it before it rewrites the buffer the query reads)."""
    from tests.hipmem import DeviceArray, hip
    N, E, T, K = 64, 2, 8, 4
    nq = 3 + 2 * K
    w = G.make_world(N, active=N - 14)
    st = G.initial_state(w)
    a = ekf_mod.Ensemble(N, E, 1, max_lines=8, pipeline=pipeline, flush_interval=T)
    b = ekf_mod.Ensemble(N, E, 1, max_lines=8)
    for ens in (a, b):
        for e in range(E):
            ens.init_lowrank(e, st.diag, st.U, st.y, st.saved, st.pose)
    scans = list(scans_with_extras(w, 16, E, 6, np.random.default_rng(11), 3))
    for step, enc, ln, nl in scans[:11]:     # step 11: three steps into the second group
        a.localize(enc, ln, nl)
        b.localize(enc, ln, nl)

    def from_device(dev, shape):
        out = np.zeros(shape)
        assert hip().hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), dev.ptr, out.nbytes, 2) == 0
        return out

    lists = np.array([[40, 3, 16, 15], [7, 50, 31, 32]], dtype=np.int32)
    d_cov, d_mean = DeviceArray(np.full((E, nq, nq), -1.0)), DeviceArray(np.full((E, nq), -1.0))
    d_lm = DeviceArray(lists)
    a.query_joint_device(d_lm.address, K, d_cov.address, d_mean.address)
    host = [a.query_joint(e, lists[e]) for e in range(E)]      # (synchronous on the same stream)
    cov, mean = from_device(d_cov, (E, nq, nq)), from_device(d_mean, (E, nq))
    for e in range(E):
        assert np.array_equal(cov[e], host[e][0]) and np.array_equal(mean[e], host[e][1]), e
        check_joint(a, b, e, lists[e], "host form")
    bad = lists.copy()
    bad[1, 2] = N
    d_bad = DeviceArray(bad)
    a.query_joint_device(d_bad.address, K, d_cov.address, d_mean.address)
    a.query_joint(0, [0])                                      # waits for the stream, drains nothing
    cov2, mean2 = from_device(d_cov, (E, nq, nq)), from_device(d_mean, (E, nq))
    hit = np.zeros((nq, nq), dtype=bool)
    hit[7:9, :] = hit[:, 7:9] = True
    assert np.array_equal(cov2[0], cov[0]) and np.array_equal(mean2[0], mean[0])
    assert np.isnan(cov2[1][hit]).all() and np.array_equal(cov2[1][~hit], cov[1][~hit])
    assert np.isnan(mean2[1][7:9]).all() and np.array_equal(np.delete(mean2[1], [7, 8]), np.delete(mean[1], [7, 8]))
    # an asynchronous query, then a drain right behind it, then the rest of the trajectory
    a.query_joint_device(d_lm.address, K, d_cov.address, d_mean.address)
    a.sync()
    cov3 = from_device(d_cov, (E, nq, nq))
    assert np.array_equal(cov3, cov)
    for step, enc, ln, nl in scans[11:]:
        a.localize(enc, ln, nl)
        b.localize(enc, ln, nl)
        a.query_joint_device(d_lm.address, K, d_cov.address, 0)
    for e in range(E):
        Pa, ya, sa, _ = a.download_state(e)
        Pb, yb, sb, _ = b.download_state(e)
        assert np.array_equal(Pa, Pb) and np.array_equal(ya, yb) and sa == sb, e
    for d in (d_cov, d_mean, d_lm, d_bad):
        d.close()


@pytest.mark.gpu
def test_errors(ekf_mod):
    N, E = 16, 2
    a = ekf_mod.Ensemble(N, E, 1, max_lines=8, flush_interval=4)
    lib, h = ekf_mod.load_library(), a.handle
    out = (ctypes.c_double * ((3 + 2 * (N + 1)) ** 2))()
    many = (ctypes.c_int32 * (N + 1))(*([0] * (N + 1)))
    neg = (ctypes.c_int32 * 2)(1, -1)
    past = (ctypes.c_int32 * 2)(N, 1)
    ok = (ctypes.c_int32 * 2)(1, 1)
    ERANGE, EINVAL = 4, 1
    assert lib.ekf_query_joint(h, 0, many, N + 1, out, out) == ERANGE
    assert lib.ekf_query_marginals(h, 0, many, N + 1, out, out, out) == ERANGE
    assert lib.ekf_query_joint(h, 0, many, -1, out, out) == ERANGE
    assert lib.ekf_query_joint(h, 0, neg, 2, out, out) == ERANGE
    assert lib.ekf_query_marginals(h, 0, past, 2, out, out, out) == ERANGE
    assert lib.ekf_query_joint(h, E, ok, 2, out, out) == ERANGE
    assert lib.ekf_query_marginals(h, -1, ok, 2, out, out, out) == ERANGE
    assert lib.ekf_query_joint_device(h, None, N + 1, None, None) == ERANGE
    assert lib.ekf_query_joint(h, 0, ok, 2, out, out) == 0
    with pytest.raises(ekf_mod.EkfError):
        a.query_joint(0, [N])
    s = ekf_mod.Ensemble(64, 1, 1, max_lines=8, flush_interval=4, shard=(0, 1))
    assert lib.ekf_query_joint(s.handle, 0, ok, 2, out, out) == EINVAL
    assert lib.ekf_query_marginals(s.handle, 0, ok, 2, out, out, out) == EINVAL
    assert lib.ekf_query_joint_device(s.handle, None, 0, None, None) == EINVAL


@pytest.mark.gpu
def test_landmark_ellipse(tmp_path, ekf_mod):
    """Robot.landmarkEllipse and BasicRobot::landmarkEllipse: getEllipse's arithmetic on the queried
    block = ekf_ellipse_of_block of the dense state's 2x2 block."""
    rob = ekf_mod.Robot(0.0, 0.0, 0.0, capacity=32, precision=1, max_lines=8)
    rng = np.random.default_rng(2)
    first = G.random_lines(rng, 6)
    rob.localize(first, encoder=[0.01, 0.0, 0.0])
    rob.localize(first[:4], encoder=[0.02, 0.0, 0.001])
    assert rob.savedLineCount >= 6
    P = rob.P_t0
    for j in (1, 5):
        want = ekf_mod.ellipse_of_block(P[3 + 2 * j:5 + 2 * j, 3 + 2 * j:5 + 2 * j])
        assert want[0] and rob.landmarkEllipse(j) == want, j
    exe = build_query_driver(tmp_path, ekf_mod)
    out = subprocess.run([str(exe), "0", "3"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    rows = [ln.split() for ln in out.stdout.strip().splitlines()]
    assert [int(r[1]) for r in rows] == [0, 3]
    for r in rows:
        ok, axii, angle = ekf_mod.ellipse_of_block([float(v) for v in r[6:10]])
        assert ok and int(r[2]) == 1
        got = [np.float32(r[3]), np.float32(r[4]), np.float32(r[5])]
        assert got == [np.float32(axii[0]), np.float32(axii[1]), np.float32(angle)], (r, axii, angle)
