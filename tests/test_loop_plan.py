"""The hypothesis loop's device stages on a CPU (slam_ekf.h ekf_gate_candidates_device, ekf_assoc_weights_device,
ekf_resample_plan_device, ekf_resample_device): the header, the binding, the NULL-context returns, and
tests/cpp/loop_driver.cpp, a stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer
that runs the host-callable parts of the kernels:

* resample_pieces (csrc/ekf_resample_plan.h), the table of ekf_resample_device, expanded with a list, is
  resample_plan's table, entry for entry;
* resample_list_code (csrc/ekf_loop_plan.h), the device's check of a list, is resample_check;
* resample_plan_sequential (csrc/ekf_loop_plan.h), the function the plan kernel calls from one lane, is
  ekf.resample_plan where every sum is exact (weights and u multiples of 2^-10) and the sequential
  restatement below on general weights.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

from tests.test_sanitizers import ENV, ROOT, SAN

FUNCTIONS = ("ekf_gate_candidates_device", "ekf_assoc_weights_device", "ekf_resample_plan_device",
             "ekf_resample_device")
EINVAL, ERANGE = 1, 4
RP_INVALID, RP_KEPT = 1, 2
INF = float("inf")

# the issue's named fixtures: weights, u, src
FIXTURES = [
    ([.5, 0, .25, 0, .125, 0, .125, 0], 0.5, [0, 0, 2, 0, 4, 0, 6, 2]),
    ([0, 0, 0, 1, 0, 0, 0, 0], 0.25, [3] * 8),
    ([0.37] * 8, 0.0, list(range(8))),
    ([0, .75, 0, .25, 0], 0.875, [1, 1, 1, 3, 3]),
]


def sequential_plan(w, u, ess_below=INF):
    """The plan as slam_ekf.h states it, in Python floats (IEEE doubles), every sum in ascending order:
    (status, copies, ess, total, src)."""
    E = len(w)
    w = [float(x) for x in w]
    ident = list(range(E))
    total = 0.0
    for x in w:
        total += x
    if any(not (x >= 0.0) or x == INF for x in w) or not (total > 0.0) or total == INF:
        return RP_INVALID, 0, 0.0, total, ident
    q = [x / total for x in w]
    sq = 0.0
    for x in q:
        sq += x * x
    ess = 1.0 / sq
    if not ess < ess_below:
        return RP_KEPT, 0, ess, total, ident
    edges, acc = [], None
    for x in q:
        acc = x if acc is None else acc + x
        edges.append(acc)
    last = max(e for e in range(E) if w[e] > 0.0)
    counts = [0] * E
    for k in range(E):
        p = (u + k) / E
        ub = next((i for i in range(E) if edges[i] > p), E)   # upper_bound
        counts[min(ub, last)] += 1
    src = ident[:]
    surplus = [e for e in range(E) for _ in range(counts[e] - 1)]
    for slot, e in zip([e for e in range(E) if counts[e] == 0], surplus):
        src[slot] = e
    return 0, sum(src[e] != e for e in range(E)), ess, total, src


@pytest.fixture(scope="module")
def loop_driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("loop") / "loop_driver"
    subprocess.run(["g++", "-std=c++17", *SAN, "-Wall", "-Wextra", "-Werror",
                    f"-I{os.path.join(ROOT, 'slam_ros_amd', 'csrc')}",
                    os.path.join(ROOT, "tests", "cpp", "loop_driver.cpp"), "-o", str(exe)], check=True)

    def run(mode, stdin=None):
        out = subprocess.run([str(exe), mode], input=stdin, capture_output=True, text=True, env=ENV, timeout=300)
        assert out.returncode == 0, (out.returncode, out.stdout[-2000:], out.stderr[-4000:])
        assert "runtime error" not in out.stderr and "ERROR: AddressSanitizer" not in out.stderr
        return out.stdout
    return run


def driver_plans(loop_driver, cases):
    """cases: (weights, u, ess_below) -> (status, copies, ess, total, src) per case, from the C++ function."""
    text = "".join(f"{len(w)} {float(u).hex()} {float(b).hex()} " + " ".join(float(x).hex() for x in w) + "\n"
                   for w, u, b in cases)
    out = []
    for line in loop_driver("--plan", text).splitlines():
        t = line.split()
        out.append((int(t[0]), int(t[1]), float.fromhex(t[2]) if "x" in t[2] else float(t[2]),
                    float.fromhex(t[3]) if "x" in t[3] else float(t[3]), [int(x) for x in t[4:]]))
    assert len(out) == len(cases)
    return out


# ---------------------------------------------------------------------------------------------
# the surface
# ---------------------------------------------------------------------------------------------
def test_header_declares_the_loop():
    from tests.test_abi import declared_functions
    names = declared_functions()
    for fn in FUNCTIONS:
        assert fn in names, fn
    src = open(os.path.join(ROOT, "include", "slam_ekf.h")).read()
    assert "#define SLAM_EKF_ABI_VERSION 3" in src   # entry points only: the number stays
    assert "typedef struct ekf_plan_info" in src
    assert "enum { EKF_RP_INVALID = 1, EKF_RP_KEPT = 2 }" in src
    head = src.split("#define SLAM_EKF_ABI_VERSION")[0]
    for fn in FUNCTIONS:
        assert fn in head, fn                        # the "added since" list of the ABI comment


def test_binding_exports_the_loop(ekf_mod):
    for fn in FUNCTIONS:
        assert fn in ekf_mod.EXPORTED, fn
        assert hasattr(ekf_mod.load_library(), fn), fn
    for name in ("gate_candidates_device", "assoc_weights_device", "resample_plan_device", "resample_device"):
        assert callable(getattr(ekf_mod.Ensemble, name))
    assert issubclass(ekf_mod.EkfPlanInfo, ctypes.Structure) and ekf_mod.ekf_plan_info is ekf_mod.EkfPlanInfo
    assert (ekf_mod.RP_INVALID, ekf_mod.RP_KEPT) == (RP_INVALID, RP_KEPT)


def test_null_context_is_einval(ekf_mod):
    """No context: EKF_EINVAL before any HIP call, whatever the other arguments are."""
    lib = ekf_mod.load_library()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.ekf_gate_candidates_device(None, p, p, 3, 0.4, p, p) == EINVAL
    assert lib.ekf_gate_candidates_device(None, None, None, 99, -1.0, None, None) == EINVAL
    assert lib.ekf_assoc_weights_device(None, p, p, 0.0, None, p) == EINVAL
    assert lib.ekf_resample_plan_device(None, p, 0.5, INF, p, None) == EINVAL
    assert lib.ekf_resample_plan_device(None, p, 2.0, INF, p, None) == EINVAL
    assert lib.ekf_resample_device(None, p, None) == EINVAL
    assert lib.ekf_resample_device(None, None, None) == EINVAL


def test_plan_info_layout(ekf_mod, loop_driver):
    c = [int(t) for t in loop_driver("--sizeof").split()]
    H = ekf_mod.EkfPlanInfo
    assert ctypes.sizeof(H) == c[0] == 24
    assert [getattr(H, f).offset for f in ("status", "copies", "ess", "total")] == c[1:]


# ---------------------------------------------------------------------------------------------
# the table and the list check
# ---------------------------------------------------------------------------------------------
def test_pieces_expand_to_the_host_table(loop_driver):
    out = loop_driver("--pieces")
    assert "resample pieces: ok" in out, out


def test_list_check_is_resample_check(loop_driver):
    out = loop_driver("--lists")
    assert "resample lists: ok (1296 lists" in out, out   # 6^4: the 256 lists over [0, 4) and entries outside it


# ---------------------------------------------------------------------------------------------
# the plan function
# ---------------------------------------------------------------------------------------------
def test_plan_fixtures(ekf_mod, loop_driver):
    got = driver_plans(loop_driver, [(w, u, INF) for w, u, _ in FIXTURES])
    for (w, u, want), (status, copies, ess, total, src) in zip(FIXTURES, got):
        assert src == want and status == 0, (w, u, src)
        assert ekf_mod.resample_plan(w, u) == want
        assert sequential_plan(w, u)[4] == want
        assert copies == sum(s != e for e, s in enumerate(src))
        assert all(src[src[e]] == src[e] for e in range(len(src)))


def test_plan_equals_resample_plan_on_exact_sums(ekf_mod, loop_driver):
    """Weights that are multiples of 2^-10 below 2^10 and u a multiple of 2^-10: every sum of weights is
    exact in any order (numpy's pairwise w.sum() too), so the C++ function, the restatement and the
    helper must agree wherever the helper's own arithmetic is the stated one."""
    rng = np.random.default_rng(2024)
    cases = []
    for trial in range(2100):
        E = (1, 2, 3, 8, 13, 64, 200)[trial % 7]
        w = rng.integers(0, 1 << 14, E).astype(np.float64) / 1024.0
        if trial % 3 == 0:
            w[rng.random(E) < 0.5] = 0.0
        if not w.any():
            w[rng.integers(E)] = 1.0
        cases.append((w.tolist(), float(rng.integers(0, 1024)) / 1024.0, INF))
    got = driver_plans(loop_driver, cases)
    for (w, u, _), (status, copies, ess, total, src) in zip(cases, got):
        assert status == 0 and src == ekf_mod.resample_plan(w, u), (w, u, src)
        assert total == float(np.sum(w))
        assert copies == sum(s != e for e, s in enumerate(src))


def test_plan_equals_the_restatement_on_general_weights(loop_driver):
    """src and total exactly, ess to 1e-12 relative (a handful of roundings: the compiler may contract
    q * q into the sum)."""
    rng = np.random.default_rng(7)
    cases = []
    for trial in range(600):
        E = (1, 2, 8, 13, 64, 200)[trial % 6]
        w = rng.random(E) ** 4 * rng.choice([1e-3, 1.0, 40.0])
        w[rng.random(E) < 0.2] = 0.0
        if not w.any():
            w[rng.integers(E)] = 1.0
        cases.append((w.tolist(), float(rng.random()), INF))
    got = driver_plans(loop_driver, cases)
    moved = 0
    for (w, u, _), (status, copies, ess, total, src) in zip(cases, got):
        rs, rc, ress, rtotal, rsrc = sequential_plan(w, u)
        assert (status, copies, src) == (rs, rc, rsrc), (w, u)
        assert total == rtotal
        assert abs(ess - ress) <= 1e-12 * ress
        assert all(src[src[e]] == src[e] for e in range(len(src)))
        moved += copies
    assert moved > 1000


def test_plan_kept_and_invalid(loop_driver):
    w = [0.5, 0.1, 0.1, 0.3]
    ess = sequential_plan(w, 0.5)[2]                   # 1 / (0.25 + 0.01 + 0.01 + 0.09) = 2.78
    nan = float("nan")
    cases = [(w, 0.5, ess * 1.01), (w, 0.5, ess * 0.99), (w, 0.5, INF), (w, 0.5, 0.0), (w, 0.5, -INF),
             ([0.5, -0.1, 0.2], 0.3, INF), ([0.5, nan, 0.2], 0.3, INF), ([0.5, INF, 0.2], 0.3, INF),
             ([0.0, 0.0, 0.0], 0.3, INF), ([-0.0, 0.0], 0.3, INF), ([1e308, 1e308], 0.3, INF)]
    got = driver_plans(loop_driver, cases)
    moved = [0, 0, 2, 3]
    assert got[0][0] == 0 and got[0][4] == moved and got[0][1] == 1
    assert got[1][0] == RP_KEPT and got[1][4] == [0, 1, 2, 3] and got[1][1] == 0
    assert abs(got[1][2] - ess) <= 1e-12 * ess and got[1][3] == sequential_plan(w, 0.5)[3]
    assert got[2][0] == 0 and got[2][4] == moved
    assert got[3][0] == RP_KEPT and got[4][0] == RP_KEPT
    for (w_, _, _), (status, copies, e_, total, src) in zip(cases[5:], got[5:]):
        assert status == RP_INVALID and copies == 0 and e_ == 0.0 and src == list(range(len(w_))), w_
    assert math.isnan(got[6][3]) and got[7][3] == INF and got[8][3] == 0.0 and got[10][3] == INF
