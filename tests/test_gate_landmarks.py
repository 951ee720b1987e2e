"""Landmark pairs that are one line (slam_ekf.h ekf_gate_landmarks / ekf_gate_landmarks_device): every
saved landmark scored against every other, in the same direction and flipped (alpha + pi, -r), read on
the device without draining the flush.

CPU: the header, the binding's export list and structure size, the NULL-context returns, the C++ driver,
duplicate_clusters, and the numpy reference pairs_ref written out from the header's formulas. GPU: the
matrix, the records, C and delta against pairs_ref on the blocks ekf_query_joint returns at the same
moment (every storage precision, EXACT and F16X3, mid-group, with an augmenting and a resetting step
pending); the records as a pure function of the matrix; symmetry; the device form; a twin never queried;
between predict and update; the edges.

The bar. The device and pairs_ref take bit-identical inputs (the queried blocks and the committed mean),
and C and delta are additions and the IEEE remainder, bit-identical too. What differs is the Cholesky
and the two triangular solves: contraction into fma, the device's sqrt and divide. Measured on the CPU
over the test states below (the oracle's states of the same trajectories), the largest
|d2_fp64 - d2_longdouble| / d2_longdouble between the fp64 and the longdouble evaluation of pairs_ref is
SPREAD; the GPU bar is 2^10 times that, test_gate.py's convention.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from slam_ros_amd import scan_gen as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIR_FUNCTIONS = ("ekf_gate_landmarks", "ekf_gate_landmarks_device")
GATE = 3.0                      # d2 <= 9: about the 99 % quantile of chi-square with 2 degrees of freedom
PH_FLIP_NEAREST, PH_FLIP_FIRST, PH_SINGULAR = 1, 2, 4
# measured on the CPU: 5.714e-13 (test_reference_spread_and_stable_decisions measures it again and holds it
# to this figure), so BAR = 5.9e-10. The largest terms are the flipped pairs': (alpha_lo - alpha_hi) - pi
# leaves about 1e-3 of a difference rounded at pi's ulp.
SPREAD = 5.8e-13
BAR = 2.0 ** 10 * SPREAD
EINVAL, ERANGE = 1, 4


# ---------------------------------------------------------------------------------------------
# The reference: the header's formulas in numpy, every pair at once, in a chosen precision
# ---------------------------------------------------------------------------------------------
def _remainder(x, dt):
    """IEEE remainder(x, 2 pi), 2 pi the fp64 constant."""
    if dt is np.float64:
        return np.array([math.remainder(float(v), 2.0 * math.pi) for v in x], dtype=np.float64)
    tp = dt(2.0 * math.pi)
    return x - tp * np.rint(x / tp)


def _form(c00, c01, c11, d0, d1):
    with np.errstate(all="ignore"):
        ok0 = (c00 > 0) & np.isfinite(c00)
        l00 = np.sqrt(np.where(ok0, c00, 1))
        l10 = c01 / l00
        t = c11 - l10 * l10
        ok1 = (t > 0) & np.isfinite(t)
        l11 = np.sqrt(np.where(ok1, t, 1))
        z0 = d0 / l00
        z1 = (d1 - l10 * z0) / l11
        d = z0 * z0 + z1 * z1
    return np.where(ok0 & ok1, d, np.nan)


def pairs_ref(cov, mean, saved, gate, dt=np.float64):
    """cov [(3 + 2s)^2], mean [3 + 2s] of the pose and the s = saved landmarks in order (what
    ekf_query_joint returns for landmarks 0 .. s - 1). Returns d2 [s, s] (+inf on the diagonal), the two
    forms' values same / flipped [s, s], flip [s, s], C [s, s, 3], delta [s, s, 2] of the form that won,
    and hits, the records of the s landmarks."""
    s = int(saved)
    d2 = np.full((s, s), np.inf, dtype=dt)
    same = np.full((s, s), np.nan, dtype=dt)
    flipped = np.full((s, s), np.nan, dtype=dt)
    flip = np.zeros((s, s), dtype=bool)
    C = np.zeros((s, s, 3), dtype=dt)
    delta = np.zeros((s, s, 2), dtype=dt)
    if s >= 2:
        cov = np.asarray(cov, dtype=dt)
        mean = np.asarray(mean, dtype=dt)
        lo, hi = np.triu_indices(s, 1)
        l0, h0 = 3 + 2 * lo, 3 + 2 * hi
        Dl00, Dl01, Dl11 = cov[l0, l0], cov[l0, l0 + 1], cov[l0 + 1, l0 + 1]
        Dh00, Dh01, Dh11 = cov[h0, h0], cov[h0, h0 + 1], cov[h0 + 1, h0 + 1]
        X00, X01, X10, X11 = cov[l0, h0], cov[l0, h0 + 1], cov[l0 + 1, h0], cov[l0 + 1, h0 + 1]
        c00 = (Dl00 + Dh00) - (X00 + X00)
        s01 = (Dl01 + Dh01) - (X01 + X10)
        s11 = (Dl11 + Dh11) - (X11 + X11)
        f01 = (Dl01 - Dh01) + (X01 - X10)
        f11 = (Dl11 + Dh11) + (X11 + X11)
        da = mean[l0] - mean[h0]
        sd0, sd1 = _remainder(da, dt), mean[l0 + 1] - mean[h0 + 1]
        fd0, fd1 = _remainder(da - dt(math.pi), dt), mean[l0 + 1] + mean[h0 + 1]
        ds = _form(c00, s01, s11, sd0, sd1)
        df = _form(c00, f01, f11, fd0, fd1)
        with np.errstate(invalid="ignore"):
            sm = np.isnan(df) | (ds <= df)
        for a, b in ((lo, hi), (hi, lo)):
            d2[a, b] = np.where(sm, ds, df)
            same[a, b], flipped[a, b] = ds, df
            flip[a, b] = ~sm
            C[a, b] = np.stack([c00, np.where(sm, s01, f01), np.where(sm, s11, f11)], axis=1)
            delta[a, b] = np.stack([np.where(sm, sd0, fd0), np.where(sm, sd1, fd1)], axis=1)
    return dict(d2=d2, same=same, flipped=flipped, flip=flip, C=C, delta=delta, hits=records_of(d2, gate))


def records_of(d2, gate):
    """(first, npass, nearest, d2_first, d2_nearest) per row of a distance matrix: first the lowest index
    with d2 <= gate^2 (a NaN fails), nearest the lowest index at the smallest finite entry."""
    out = []
    g2 = gate * gate
    for row in np.asarray(d2, dtype=np.float64):
        with np.errstate(invalid="ignore"):
            ok = row <= g2
        fin = np.isfinite(row)
        first = int(np.argmax(ok)) if ok.any() else -1
        nearest = int(np.flatnonzero(fin)[np.argmin(row[fin])]) if fin.any() else -1
        out.append((first, int(ok.sum()), nearest, row[first] if first >= 0 else np.nan,
                    row[nearest] if nearest >= 0 else np.nan))
    return out


def margins(ref, gate):
    """How far the reference's decisions are from flipping (relative): the pair nearest gate^2, the
    closest runner-up for `nearest`, the closest call between the two forms."""
    d2 = np.asarray(ref["d2"], dtype=np.float64)
    s = d2.shape[0]
    g2 = gate * gate
    m_gate = m_near = m_form = np.inf
    if s >= 2:
        off = ~np.eye(s, dtype=bool)
        v = d2[off]
        m_gate = float(np.nanmin(np.abs(v - g2) / g2))
        for row in d2:
            f = np.sort(row[np.isfinite(row)])
            if f.size >= 2:
                m_near = min(m_near, float((f[1] - f[0]) / f[0]) if f[0] > 0 else 0.0)
        a, b = np.asarray(ref["same"], dtype=np.float64)[off], np.asarray(ref["flipped"], dtype=np.float64)[off]
        both = ~np.isnan(a) & ~np.isnan(b)
        if both.any():
            m_form = float(np.min(np.abs(a[both] - b[both]) / np.maximum(a[both], b[both])))
    return m_gate, m_near, m_form


def assert_stable(ref, gate, where):
    m_gate, m_near, m_form = margins(ref, gate)
    assert m_gate > 1e-6, (where, "a pair within 1e-6 of the gate", m_gate)
    assert m_near > 1e-9, (where, "a runner-up within 1e-9 of the nearest", m_near)
    assert m_form > 1e-6, (where, "the two forms within 1e-6 of each other", m_form)


# ---------------------------------------------------------------------------------------------
# The test states: a scan_gen world with planted pairs
# ---------------------------------------------------------------------------------------------
# (p, q, kind): landmark q is made a near copy of p (passes, same direction), a flipped copy
# (alpha + pi folded, -r) plus small noise (passes in the flipped form only), or a far copy (fails).
# 15 | 16 is the edge of a 32 x 32-element tile, 5 and 9 share a diagonal tile (both stored orientations),
# 3 and 66 lie in different 64-landmark blocks.
PLANTS = ((3, 66, "near"), (5, 9, "near"), (15, 16, "flip"), (20, 50, "far"), (70, 180, "near"), (100, 129, "flip"))
PLANTS_5 = ((0, 3, "near"), (1, 4, "flip"), (0, 2, "far"))


def planted_world(N, saved, seed=42):
    w = G.make_world(N, active=saved, seed=seed)
    plants = [pl for pl in (PLANTS_5 if saved <= 5 else PLANTS) if pl[1] < saved]
    for p, q, kind in plants:
        if kind == "near":
            w.alpha[q], w.r[q] = w.alpha[p] + 1e-3, w.r[p] - 1e-3
        elif kind == "far":
            w.alpha[q], w.r[q] = w.alpha[p] + 0.05, w.r[p] + 0.05
        else:
            w.alpha[q], w.r[q] = float(G.wrap_pi(w.alpha[p] + np.pi)) + 1e-3, -w.r[p] + 1e-3
    return w, G.initial_state(w), plants


MARGIN_80 = 5      # reset_margin of the N = 80 contexts: 70 + 2 lines stay, 72 + 4 reset the map


def scans_80(w, E=1):
    """Six scans on the N = 80 map (70 saved): four re-observed lines each; scan 2 carries two lines more
    (new landmarks: 72), scan 5 four (76 > 80 - 5: the map is reset), scan 6 starts the new map."""
    rng = np.random.default_rng(11)
    for step in range(1, 7):
        enc, ln, nl = G.make_scan(w, step, instances=E, lines=4)
        extra = {2: 2, 5: 4}.get(step, 0)
        if extra:
            ex = G.random_lines(rng, extra)[None].repeat(E, axis=0)
            ln = np.concatenate([ln, ex], axis=1)
            nl = np.full(E, ln.shape[1], dtype=np.int32)
        yield step, enc, ln, nl


SAVED_200 = (190, 130, 1)


def worlds_200():
    return [planted_world(200, s, seed=42 + k) for k, s in enumerate(SAVED_200)]


def scans_200(worlds, steps=2):
    for step in range(1, steps + 1):
        parts = [G.make_scan(w, step, instances=1, lines=6, first_instance=k) for k, (w, _, _) in enumerate(worlds)]
        yield (step, np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]),
               np.concatenate([p[2] for p in parts]))


def oracle_states(oracle_mod, cap, st, scans, e=0):
    """The dense (cov, mean, saved) of instance e on the oracle: the initial state, then after each scan,
    cut to the saved landmarks as ekf_query_joint returns them."""
    ref = oracle_mod.OracleRobot(cap, mode=oracle_mod.FAST)
    n = ref.n
    P, y = np.zeros((n, n)), np.zeros(n)
    k = st.y.shape[0]
    P[:k, :k], y[:k] = st.dense_P(), st.y
    ref.set_state(P, y, st.saved, st.pose)
    out = []

    def take():
        s = ref.savedLineCount
        q = 3 + 2 * s
        out.append((ref.P_t0[:q, :q].copy(), ref.y[:q].copy(), s))

    take()
    for _step, enc, ln, nl in scans:
        ref.localize(ln[e, :nl[e]], enc[e])
        take()
    return out


def cpu_states(oracle_mod):
    """Every state the GPU tests query, as the oracle computes it: (name, cov, mean, saved)."""
    out = []
    w, st, _ = planted_world(5, 5)
    out += [("N5", *t) for t in oracle_states(oracle_mod, 15, st, [])]
    w, st, _ = planted_world(80, 70)
    # (the oracle's reset margin is the reference's 10: capacity 85 resets where the N = 80 contexts do)
    out += [("N80", *t) for t in oracle_states(oracle_mod, 80 + 10 - MARGIN_80, st, scans_80(w))]
    worlds = worlds_200()
    for e, (w, st, _) in enumerate(worlds):
        out += [(f"N200/{e}", *t) for t in oracle_states(oracle_mod, 200, st, scans_200(worlds), e)]
    return out


# ---------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------
def test_header_declares_the_pairs():
    from tests.test_abi import declared_functions
    names = declared_functions()
    for fn in PAIR_FUNCTIONS:
        assert fn in names, fn
    src = open(os.path.join(ROOT, "include", "slam_ekf.h")).read()
    assert "#define SLAM_EKF_ABI_VERSION 3" in src   # entry points only: the number stays
    assert "typedef struct ekf_pair_hit" in src
    assert "EKF_PH_FLIP_NEAREST = 1, EKF_PH_FLIP_FIRST = 2, EKF_PH_SINGULAR = 4" in src


def test_binding_exports_the_pairs(ekf_mod):
    for fn in PAIR_FUNCTIONS:
        assert fn in ekf_mod.EXPORTED, fn
        assert hasattr(ekf_mod.load_library(), fn), fn
    for name in ("gate_landmarks", "gate_landmarks_device"):
        assert callable(getattr(ekf_mod.Ensemble, name))
    assert callable(ekf_mod.duplicate_clusters)
    assert issubclass(ekf_mod.ekf_pair_hit, ctypes.Structure)
    assert ctypes.sizeof(ekf_mod.EkfPairHit) == 72 == ekf_mod.PAIR_HIT_DTYPE.itemsize
    assert (ekf_mod.PH_FLIP_NEAREST, ekf_mod.PH_FLIP_FIRST, ekf_mod.PH_SINGULAR) == (1, 2, 4)
    from slam_ros_amd import build
    assert "unit_pairs.hip" in build.UNITS


def test_null_context_is_einval(ekf_mod):
    lib = ekf_mod.load_library()
    hits = (ekf_mod.ekf_pair_hit * 4)()
    d2 = (ctypes.c_double * 16)()
    assert lib.ekf_gate_landmarks(None, 0, 0.4, hits, d2) == EINVAL
    assert lib.ekf_gate_landmarks(None, 0, 0.4, None, None) == EINVAL
    assert lib.ekf_gate_landmarks_device(None, 0.4, hits, None) == EINVAL


def test_pairs_driver_builds_and_runs(tmp_path, ekf_mod):
    """tests/cpp/pairs_driver.cpp includes the public header as C++ (-Wall -Werror), holds the structure
    to 72 bytes, and gets EKF_EINVAL for a NULL context from both forms; the binding's structure and
    numpy type have the C structure's field offsets."""
    exe = tmp_path / "pairs_driver"
    libdir = os.path.dirname(ekf_mod.LIB_PATH)
    subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
                    os.path.join(ROOT, "tests", "cpp", "pairs_driver.cpp"), "-o", str(exe),
                    f"-L{libdir}", "-lslam_ekf", f"-Wl,-rpath,{libdir}"], check=True)
    out = subprocess.run([str(exe), "--sizeof"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    c = [int(t) for t in out.stdout.split()]
    H = ekf_mod.ekf_pair_hit
    fields = ("nearest", "first", "npass", "status", "d2_nearest", "d2_first", "C", "delta")
    assert ctypes.sizeof(H) == c[0] == 72
    assert [getattr(H, f).offset for f in fields] == c[1:]
    assert [ekf_mod.PAIR_HIT_DTYPE.fields[f][1] for f in fields] == c[1:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.split() == ["null", "1", "1"], (out.returncode, out.stdout)


def test_duplicate_clusters(ekf_mod):
    """Union-find over the passing pairs: chains join, groups and members ascend; with the matrix every
    passing pair counts, without it the pairs the records name."""
    inf = np.inf
    d2 = np.full((8, 8), 100.0)
    np.fill_diagonal(d2, inf)
    d2[7, :] = d2[:, 7] = inf                      # past savedLineCount
    for a, b, v in ((5, 1, 0.5), (1, 4, 2.0), (2, 6, 1.0), (0, 2, 3.0), (3, 6, 4.0), (0, 3, 5.0)):
        d2[a, b] = d2[b, a] = v
    d2[2, 3] = d2[3, 2] = np.nan                   # a singular pair never passes
    gate = math.sqrt(5.0)
    hits = np.zeros(8, dtype=ekf_mod.PAIR_HIT_DTYPE)
    for a, (first, npass, nearest, df, dn) in enumerate(records_of(d2, gate)):
        hits[a] = (nearest, first, npass, 0, dn, df, (0, 0, 0), (0, 0))
    assert ekf_mod.duplicate_clusters(hits, d2) == [[0, 2, 3, 6], [1, 4, 5]]
    assert ekf_mod.duplicate_clusters(hits) == [[0, 2, 3, 6], [1, 4, 5]]
    # records alone see (a, first) and (a, nearest) only: 2-3 passes, but 2 and 3 name 0 and 1
    d2 = np.full((4, 4), 100.0)
    np.fill_diagonal(d2, inf)
    for a, b, v in ((0, 2, 1.0), (1, 3, 1.0), (2, 3, 2.0)):
        d2[a, b] = d2[b, a] = v
    hits = np.zeros(4, dtype=ekf_mod.PAIR_HIT_DTYPE)
    for a, (first, npass, nearest, df, dn) in enumerate(records_of(d2, gate)):
        hits[a] = (nearest, first, npass, 0, dn, df, (0, 0, 0), (0, 0))
    assert ekf_mod.duplicate_clusters(hits, d2) == [[0, 1, 2, 3]]
    assert ekf_mod.duplicate_clusters(hits) == [[0, 2], [1, 3]]
    assert ekf_mod.duplicate_clusters(np.zeros(0, dtype=ekf_mod.PAIR_HIT_DTYPE)) == []
    none = np.zeros(3, dtype=ekf_mod.PAIR_HIT_DTYPE)
    none["first"] = none["nearest"] = -1
    assert ekf_mod.duplicate_clusters(none) == []


def test_reference_on_a_hand_case():
    """Two independent landmarks with unit covariance: the same-direction distance is |dy|^2 / 2; a
    flipped copy has distance 0 in the flipped form and a large one in the same direction; a fully
    correlated identical pair is NaN in both forms."""
    cov = np.eye(3 + 2 * 4)
    mean = np.array([0, 0, 0, 0.5, 2.0, 0.7, 1.0, 0.5 - math.pi, -2.0, 0.5, 2.0])
    cov[9:11, 3:5] = cov[3:5, 9:11] = np.eye(2)    # landmark 3 == landmark 0, fully correlated
    ref = pairs_ref(cov, mean, 4, GATE)
    assert abs(ref["d2"][0, 1] - (0.2 ** 2 + 1.0 ** 2) / 2) < 1e-14 and not ref["flip"][0, 1]
    assert ref["flip"][0, 2] and ref["flip"][2, 0] and ref["d2"][0, 2] < 1e-30
    assert np.isnan(ref["d2"][0, 3]) and np.isnan(ref["d2"][3, 0])
    assert np.array_equal(ref["d2"], ref["d2"].T, equal_nan=True)
    first, npass, nearest, _, _ = ref["hits"][0]
    assert (first, npass, nearest) == (1, 2, 2)
    assert ref["hits"][3][:3] == (1, 2, 2)         # (its NaN against 0 neither passes nor is nearest)
    assert np.array_equal(ref["C"][0, 1], [2.0, 0.0, 2.0]) and np.array_equal(ref["delta"][2, 0], ref["delta"][0, 2])


def test_reference_spread_and_stable_decisions(oracle_mod):
    """Every state the GPU tests query, on the oracle: the planted pairs come out as planted, the fp64 /
    longdouble spread of d2 is what the comment at the top says, and no decision is near its edge: no
    pair within 1e-6 of gate^2, no runner-up within 1e-9 of a nearest, the two forms never within 1e-6."""
    assert np.finfo(np.longdouble).eps < 2e-19      # (x87 extended: the comparison means something)
    spread, pairs = 0.0, 0
    for name, cov, mean, s in cpu_states(oracle_mod):
        ref = pairs_ref(cov, mean, s, GATE)
        assert_stable(ref, GATE, name)
        if s < 2:
            continue
        ld = pairs_ref(cov, mean, s, GATE, dt=np.longdouble)
        off = ~np.eye(s, dtype=bool)
        a, b = ref["d2"][off], ld["d2"][off]
        assert np.all(np.isfinite(a)) and np.array_equal(ref["flip"], ld["flip"]), name
        spread = max(spread, float(np.max(np.abs(a - b) / b)))
        pairs += a.size // 2
    print(f"{pairs} pairs; fp64 vs longdouble spread of d2 {spread:.3e}")
    assert pairs > 30000
    assert spread <= SPREAD, spread
    # the planted pairs on the initial N = 80 state
    w, st, plants = planted_world(80, 70)
    q = 3 + 2 * st.saved
    ref = pairs_ref(st.dense_P()[:q, :q], st.y[:q], st.saved, GATE)
    check_plants(ref["d2"], ref["flip"], plants, "N80 initial")


def check_plants(d2, flip, plants, where):
    g2 = GATE * GATE
    for p, q, kind in plants:
        if kind == "near":
            assert d2[p, q] <= g2 and not flip[p, q], (where, p, q, d2[p, q])
        elif kind == "flip":
            assert d2[p, q] <= g2 and flip[p, q], (where, p, q, d2[p, q])
        else:
            assert d2[p, q] > g2, (where, p, q, d2[p, q])


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
def make(ekf_mod, N, prec, states, **kw):
    kw.setdefault("max_lines", 8)
    ens = ekf_mod.Ensemble(N, len(states), prec, **kw)
    for e, st in enumerate(states):
        ens.init_lowrank(e, st.diag, st.U, st.y, st.saved, st.pose)
    return ens


def empty_record(h):
    return ((h["first"], h["nearest"], h["npass"], h["status"]) == (-1, -1, 0, 0) and np.isnan(h["d2_first"])
            and np.isnan(h["d2_nearest"]) and not h["C"].any() and not h["delta"].any())


def check_pure(hits, d2, where):
    """The records are a pure function of the matrix: recomputed by numpy, exactly."""
    for a, (first, npass, nearest, df, dn) in enumerate(records_of(d2, GATE)):
        h = hits[a]
        assert (h["first"], h["npass"], h["nearest"]) == (first, npass, nearest), (where, a, h)
        for got, want in ((h["d2_first"], df), (h["d2_nearest"], dn)):
            assert (np.isnan(got) and np.isnan(want)) or got == want, (where, a, h)
    assert np.array_equal(d2, d2.T, equal_nan=True), where          # bit for bit (no -0: d2 >= 0)


def check_values(ens, e, s, where, plants=None):
    """Instance e (s landmarks saved) against pairs_ref on the blocks ekf_query_joint returns now. Returns
    the largest relative error of d2."""
    N = ens.capacity
    hits, d2 = ens.gate_landmarks(e, GATE, want_d2=True)
    only = ens.gate_landmarks(e, GATE)
    assert only.tobytes() == hits.tobytes(), where                  # the same bytes without the matrix
    assert np.all(np.isposinf(d2[s:, :])) and np.all(np.isposinf(d2[:, s:])) and np.all(np.isposinf(np.diag(d2))), where
    check_pure(hits, d2, where)
    for a in range(s if s >= 2 else 0, N):
        assert empty_record(hits[a]), (where, a, hits[a])
    if s < 2:
        assert np.all(np.isposinf(d2)), where
        return 0.0
    cov, mean = ens.query_joint(e, np.arange(s))
    ref = pairs_ref(cov, mean, s, GATE)
    assert_stable(ref, GATE, where)
    off = ~np.eye(s, dtype=bool)
    got, want = d2[:s, :s][off], ref["d2"][off]
    assert np.all(np.isfinite(want)) and np.all(np.isfinite(got)), where
    worst = float(np.max(np.abs(got - want) / want))
    assert worst <= BAR, (where, worst, BAR)
    for a in range(s):
        h = hits[a]
        first, npass, nearest, _, _ = ref["hits"][a]
        assert (h["first"], h["npass"], h["nearest"]) == (first, npass, nearest), (where, a, h, ref["hits"][a])
        st = (PH_FLIP_NEAREST if ref["flip"][a, nearest] else 0) | (PH_FLIP_FIRST if first >= 0 and ref["flip"][a, first] else 0)
        assert h["status"] == st, (where, a, h, st)
        # additions and remainder only: bit for bit
        assert h["C"].tobytes() == ref["C"][a, nearest].tobytes(), (where, a, h["C"], ref["C"][a, nearest])
        assert h["delta"].tobytes() == ref["delta"][a, nearest].tobytes(), (where, a, h["delta"], ref["delta"][a, nearest])
    if plants:
        flip = np.zeros((N, N), dtype=bool)
        for a in range(s):
            if hits[a]["status"] & PH_FLIP_NEAREST:
                flip[a, hits[a]["nearest"]] = True
        check_plants(d2, flip, plants, where)
        for p, q, kind in plants:
            if kind != "far":                                       # each is the other's nearest and only partner
                assert (hits[p]["nearest"], hits[q]["nearest"]) == (q, p), (where, p, q)
                assert hits[p]["npass"] == 1 and hits[q]["npass"] == 1 and hits[q]["first"] == p, (where, p, q)
                want_st = PH_FLIP_NEAREST | PH_FLIP_FIRST if kind == "flip" else 0
                assert hits[p]["status"] == want_st == hits[q]["status"], (where, p, q, hits[p], hits[q])
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [0, 1, 2])
def test_one_partial_block(ekf_mod, prec):
    """N = 5, all saved: one workgroup, five of its 64 lanes and rows; the three planted pairs."""
    w, st, plants = planted_world(5, 5)
    a = make(ekf_mod, 5, prec, [st], flush_interval=4)
    worst = check_values(a, 0, 5, f"N5 prec {prec}", plants)
    print(f"N 5 prec {prec}: worst relative error of d2 {worst:.3e} (bar {BAR:.3e})")
    hits, d2 = a.gate_landmarks(0, GATE, want_d2=True)
    assert ekf_mod.duplicate_clusters(hits, d2) == [[0, 3], [1, 4]] == ekf_mod.duplicate_clusters(hits)


@pytest.mark.gpu
@pytest.mark.parametrize("prec,arith", [(0, 0), (1, 0), (2, 0), (1, 2), (2, 2)])
def test_values_mid_group(ekf_mod, prec, arith):
    """N = 80, 70 saved (two 64-landmark blocks, the tile edge 15 | 16, both stored orientations), T = 4,
    queried at the start and after each of six scans: 1, 2, 3, 0, 1, 2 steps pending, among them one that
    augments (scan 2) and one that resets the map (scan 5), replayed on read. The matrix within the bar of
    pairs_ref on the blocks ekf_query_joint returns at the same moment; first, npass, nearest equal; C and
    delta of nearest bit for bit; the flip bits as planted while the planted map lives.

    Measured on an MI355X, worst relative error of d2 (printed on every run): fp64 storage 4.8e-16, fp32
    4.9e-16, fp16 6.5e-16, F16X3 on fp32 4.3e-16 and on fp16 6.5e-16, against BAR = 5.9e-10."""
    w, st, plants = planted_world(80, 70)
    a = make(ekf_mod, 80, prec, [st], flush_interval=4, arith=arith, reset_margin=MARGIN_80, max_lines=8)
    worst = check_values(a, 0, 70, "initial", plants)
    saved, resets = [], 0
    for step, enc, ln, nl in scans_80(w):
        r = a.localize(enc, ln, nl)[0]
        saved.append(r["saved"])
        resets += r["reset"]
        worst = max(worst, check_values(a, 0, r["saved"], f"prec {prec} arith {arith} scan {step}",
                                        plants if not resets else None))
    print(f"N 80 prec {prec} arith {arith}: saved {saved}; worst relative error of d2 {worst:.3e} (bar {BAR:.3e})")
    assert saved[0] == 70 and saved[1] == 72 and saved[3] == 72 and saved[4] == 0 and saved[5] >= 2 and resets == 1, saved


@pytest.mark.gpu
def test_instances_that_differ(ekf_mod):
    """N = 200, E = 3 with 190, 130 and 1 landmarks saved (four blocks: several I < J workgroups, a
    partial last block, an instance without a pair), fp32, T = 4, two scans pending: the values, the pure
    function, the symmetry per instance; then the device form of all three at once, the same bytes as the
    host forms, with and without the matrix."""
    from tests.hipmem import DeviceArray, hip
    N, E = 200, 3
    worlds = worlds_200()
    a = make(ekf_mod, N, 1, [st for _, st, _ in worlds], flush_interval=4)
    for e in range(E):
        check_values(a, e, SAVED_200[e], f"N200/{e} initial", worlds[e][2])
    for step, enc, ln, nl in scans_200(worlds):
        r = a.localize(enc, ln, nl)
    assert [x["saved"] for x in r] == list(SAVED_200)
    worst = max(check_values(a, e, SAVED_200[e], f"N200/{e} pending 2", worlds[e][2]) for e in range(E))
    print(f"N 200: worst relative error of d2 {worst:.3e} (bar {BAR:.3e})")
    H = ekf_mod.PAIR_HIT_DTYPE
    d_hits = DeviceArray(np.full(E * N * H.itemsize, 0x5a, dtype=np.uint8))
    d_d2 = DeviceArray(np.full((E, N, N), -1.0))
    a.gate_landmarks_device(GATE, d_hits.address, d_d2.address)
    host = [a.gate_landmarks(e, GATE, want_d2=True) for e in range(E)]        # (synchronous, same stream)
    hits = np.zeros((E, N), dtype=H)
    d2 = np.zeros((E, N, N))
    assert hip().hipMemcpy(hits.ctypes.data_as(ctypes.c_void_p), d_hits.ptr, hits.nbytes, 2) == 0
    assert hip().hipMemcpy(d2.ctypes.data_as(ctypes.c_void_p), d_d2.ptr, d2.nbytes, 2) == 0
    for e in range(E):
        assert hits[e].tobytes() == host[e][0].tobytes(), e
        assert d2[e].tobytes() == host[e][1].tobytes(), e
    d_only = DeviceArray(np.full(E * N * H.itemsize, 0x5a, dtype=np.uint8))
    a.gate_landmarks_device(GATE, d_only.address, 0)
    a.sync()
    only = np.zeros((E, N), dtype=H)
    assert hip().hipMemcpy(only.ctypes.data_as(ctypes.c_void_p), d_only.ptr, only.nbytes, 2) == 0
    assert only.tobytes() == hits.tobytes()
    for d in (d_hits, d_d2, d_only):
        d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("prec,arith,pipeline", [(1, 0, False), (1, 0, True), (1, 2, False), (2, 2, False)])
def test_state_untouched(ekf_mod, prec, arith, pipeline):
    """A context queried before and after every scan (host form with and without the matrix, device form)
    and a twin never queried: the same results and matches scan by scan, the same flushes, and P, y, the
    pose and savedLineCount bit for bit at the end. T = 4 over the six scans: under F16X3 a drain of a
    partial group would change the bits."""
    from tests.hipmem import DeviceArray
    w, st, _ = planted_world(80, 70)
    kw = dict(flush_interval=4, arith=arith, reset_margin=MARGIN_80, pipeline=pipeline)
    a = make(ekf_mod, 80, prec, [st, st], **kw)
    c = make(ekf_mod, 80, prec, [st, st], **kw)
    a.profile(1)
    c.profile(1)
    d_hits = DeviceArray(np.zeros(2 * 80 * 72, dtype=np.uint8))
    d_d2 = DeviceArray(np.zeros((2, 80, 80)))
    for step, enc, ln, nl in scans_80(w, 2):
        a.gate_landmarks(step % 2, GATE, want_d2=True)
        a.gate_landmarks_device(GATE, d_hits.address, d_d2.address if step % 2 else 0)
        ra = a.localize(enc, ln, nl)
        rc = c.localize(enc, ln, nl)
        a.gate_landmarks(0, GATE)
        for x, z in zip(ra, rc):
            assert {k: np.asarray(v).tobytes() for k, v in x.items()} == {k: np.asarray(v).tobytes() for k, v in z.items()}, step
    fa = [n for n, _ in a.profile_flushes()]
    fc = [n for n, _ in c.profile_flushes()]
    assert fa == fc == [4], (fa, fc)                      # the call never drained
    for e in range(2):
        Pa, ya, sa, pa = a.download_state(e)
        Pc, yc, sc, pc = c.download_state(e)
        assert np.array_equal(Pa, Pc), (e, np.argwhere(Pa != Pc)[:8].tolist())
        assert np.array_equal(ya, yc) and np.array_equal(pa, pc) and sa == sc
    d_hits.close()
    d_d2.close()


@pytest.mark.gpu
def test_between_predict_and_update(ekf_mod):
    """The predict moves neither the landmark block nor the landmark means: a call between ekf_predict
    and ekf_update returns the bytes the call before the predict returned; the update then changes them."""
    w, st, _ = planted_world(80, 70)
    a = make(ekf_mod, 80, 1, [st], flush_interval=4, reset_margin=MARGIN_80)
    scans = list(scans_80(w))
    for step, enc, ln, nl in scans[:2]:
        a.localize(enc, ln, nl)
    before = a.gate_landmarks(0, GATE, want_d2=True)
    step, enc, ln, nl = scans[2]
    a.predict(enc)
    between = a.gate_landmarks(0, GATE, want_d2=True)
    assert before[0].tobytes() == between[0].tobytes() and before[1].tobytes() == between[1].tobytes()
    r = a.update(ln, nl)[0]
    assert r["matches"] >= 1
    after = a.gate_landmarks(0, GATE, want_d2=True)
    assert after[1].tobytes() != before[1].tobytes()
    check_values(a, 0, r["saved"], "after the update")


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [0, 1])
def test_singular_pair(ekf_mod, prec):
    """Landmarks 0 and 1 uploaded identical and fully correlated (C = 0 in both forms): their pair is NaN,
    EKF_PH_SINGULAR in both records, and it does not pass; landmark 2 is independent and unaffected."""
    N = 16
    n = 3 + 2 * N
    M = np.array([[2.0 ** -10, 2.0 ** -12], [2.0 ** -12, 2.0 ** -10]])      # exact in every storage
    P = np.zeros((n, n))
    P[0, 0] = P[1, 1] = P[2, 2] = 2.0 ** -12
    for i in (0, 1):
        for j in (0, 1):
            P[3 + 2 * i:5 + 2 * i, 3 + 2 * j:5 + 2 * j] = M
    P[7:9, 7:9] = M
    y = np.zeros(n)
    y[3:9] = [0.5, 2.0, 0.5, 2.0, 0.5 + 0.01, 2.0 - 0.01]
    a = ekf_mod.Ensemble(N, 1, prec, max_lines=8, flush_interval=4)
    a.upload_state(0, P, y, 3, np.zeros(3))
    hits, d2 = a.gate_landmarks(0, GATE, want_d2=True)
    assert np.isnan(d2[0, 1]) and np.isnan(d2[1, 0])
    want = ((0.01 ** 2) * (M[0, 0] + M[1, 1] + 2 * M[0, 1]) / (M[0, 0] * M[1, 1] - M[0, 1] ** 2)) / 2
    assert abs(d2[0, 2] - want) <= 1e-9 * want and d2[0, 2] == d2[1, 2] == d2[2, 0] == d2[2, 1]
    for k in (0, 1):
        h = hits[k]
        assert h["status"] == PH_SINGULAR and (h["first"], h["nearest"], h["npass"]) == (2, 2, 1), h
    assert hits[2]["status"] == 0 and (hits[2]["first"], hits[2]["nearest"], hits[2]["npass"]) == (0, 0, 2)
    check_pure(hits, d2, "singular")
    assert a.gate_landmarks(0, GATE).tobytes() == hits.tobytes()
    assert ekf_mod.duplicate_clusters(hits, d2) == [[0, 1, 2]]       # (0-2 and 1-2 pass; 0-1 itself does not)


@pytest.mark.gpu
def test_edges_and_errors(ekf_mod):
    """An empty map and a one-landmark map give empty records and an all-inf matrix; gate = 0 passes
    nothing but keeps nearest; the error returns."""
    N, E = 16, 2
    w, st, _ = planted_world(N, 5)
    one = G.initial_state(G.make_world(N, active=1))
    a = make(ekf_mod, N, 1, [st, one], flush_interval=4)
    b = ekf_mod.Ensemble(N, 1, 1, max_lines=8, flush_interval=4)          # never initialised: empty
    for ens, e in ((b, 0), (a, 1)):
        hits, d2 = ens.gate_landmarks(e, GATE, want_d2=True)
        assert np.all(np.isposinf(d2)) and all(empty_record(h) for h in hits)
        assert ens.gate_landmarks(e, GATE).tobytes() == hits.tobytes()
    h3, d3 = a.gate_landmarks(0, GATE, want_d2=True)
    h0, d0 = a.gate_landmarks(0, 0.0, want_d2=True)
    assert d0.tobytes() == d3.tobytes() and np.array_equal(h0["nearest"], h3["nearest"])
    assert np.all(h0["npass"] == 0) and np.all(h0["first"] == -1) and np.all(np.isnan(h0["d2_first"]))
    assert h3["npass"][:5].tolist() == [1, 1, 0, 1, 1]
    lib, h = ekf_mod.load_library(), a.handle
    H = (ekf_mod.ekf_pair_hit * N)()
    assert lib.ekf_gate_landmarks(h, E, 0.4, H, None) == ERANGE
    assert lib.ekf_gate_landmarks(h, -1, 0.4, H, None) == ERANGE
    assert lib.ekf_gate_landmarks(h, 0, 0.4, None, None) == EINVAL
    for bad in (-0.1, float("nan"), float("inf")):
        assert lib.ekf_gate_landmarks(h, 0, bad, H, None) == EINVAL
        assert lib.ekf_gate_landmarks_device(h, bad, H, None) == EINVAL
    assert lib.ekf_gate_landmarks_device(h, 0.4, None, None) == EINVAL
    assert lib.ekf_gate_landmarks(h, 0, 0.4, H, None) == 0
    s = ekf_mod.Ensemble(64, 1, 1, max_lines=8, flush_interval=4, shard=(0, 1))
    assert lib.ekf_gate_landmarks(s.handle, 0, 0.4, H, None) == EINVAL
    assert lib.ekf_gate_landmarks_device(s.handle, 0.4, H, None) == EINVAL
