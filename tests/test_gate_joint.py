"""Joint compatibility of line-landmark hypotheses, state untouched (slam_ekf.h ekf_gate_joint /
ekf_gate_joint_device): per hypothesis the stacked innovation's vᵀS⁻¹v and log det S, read on the device
without draining the flush.

CPU: the header, the binding's exports and structure, the NULL-context returns, the C++ driver, and
the bar. GPU: the hits against a numpy evaluation (dense_joint) on the dense state of a twin drained
after every scan, for every storage precision and the split arithmetics; d2_each against
ekf_gate_lines; m = 1 against the gate's 2×2 LU; bit-identity mid-group against a twin flushed after
every step; the state untouched; order independence and host form == device form; the widths up to
2m = 128; predict on read; the device form; the edges; the C++ driver.

The EXACT bars. Under EKF_ARITH_EXACT the blocks the kernel reads are bit for bit the twin's, so the
device and numpy differ only by fp64 evaluation order: summation order, contraction into fma, the
device's sincos and reciprocal, each a few ulps through the same conditioning of S. Measured on the
CPU over the shared trajectory's hypotheses (the oracle's own association of every scan, each of its
single-line sub-hypotheses, one crossed pairing per scan that matches a line: 20 + 67 + 14 cases,
the six scans behind the capacity reset match nothing), the largest |d_fp64 − d_longdouble| /
(1 + d), d = sqrt|d²|, and |logdet_fp64 − logdet_longdouble| / (1 + |logdet|) between dense_joint in
fp64 and in longdouble are SPREAD_D and SPREAD_LOGDET below; the bars are 2^10 times those.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from slam_ros_amd import scan_gen as G
from tests.test_gate import ETA, ST_SINGULAR, dense_gate, dist, make, shared_scans, shared_world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOINT_FUNCTIONS = ("ekf_gate_joint", "ekf_gate_joint_device")
# measured on the CPU: d 2.876e-14, logdet 2.305e-15 (test_the_bar measures them again and holds them to
# these figures), so BAR_D = 2.97e-11 and BAR_LOGDET = 2.46e-12
SPREAD_D = 2.9e-14
SPREAD_LOGDET = 2.4e-15
BAR_D = 2.0 ** 10 * SPREAD_D
BAR_LOGDET = 2.0 ** 10 * SPREAD_LOGDET
EINVAL, ERANGE = 1, 4


# ---------------------------------------------------------------------------------------------
# The reference
# ---------------------------------------------------------------------------------------------
def predicted(P, pose, enc, dt):
    """The dense predict of dense_gate (its expressions): P and the pose a gate with `enc` reads."""
    P = np.asarray(P, dtype=dt)
    pose = np.asarray(pose, dtype=dt)
    if enc is None:
        return P, pose
    enc = np.asarray(enc, dtype=dt)
    u2 = pose[2] - enc[2]
    dX, dY = pose[0] - enc[0], pose[1] - enc[1]
    u0 = np.sqrt(dX * dX + dY * dY)
    xp = np.array([pose[0] + u0 * np.cos(pose[2] + u2 / dt(2)), pose[1] + u0 * np.sin(pose[2] + u2 / dt(2)),
                   pose[2] + u2], dtype=dt)
    c = u2 / dt(2) + pose[2]
    one, zero = dt(1), dt(0)
    F3 = np.array([[one, zero, -u0 * np.sin(c)], [zero, one, u0 * np.cos(c)], [zero, zero, one]], dtype=dt)
    Fu3 = np.array([[np.cos(c), zero, -u0 * np.sin(c) / dt(2)], [np.sin(c), one, u0 * np.cos(c) / dt(2)],
                    [zero, zero, one]], dtype=dt)
    qs = -one / (one + abs(u0)) + one
    en = dt(0.024)
    Q = np.diag(np.array([en * qs, dt(2) * en * qs, en * qs], dtype=dt))
    Pp = P.copy()
    Pp[0:3, 3:] = F3 @ P[0:3, 3:]
    Pp[3:, 0:3] = P[3:, 0:3] @ F3.T
    Pp[0:3, 0:3] = (F3 @ P[0:3, 0:3]) @ F3.T + (Fu3 @ Q) @ Fu3.T
    return Pp, xp


def dense_joint(P, y, saved, pose, enc, lines, assign, r_mode=0, dt=np.float64):
    """One hypothesis on the dense state: dict(m, ok, d2, logdet, S, v, bound, ldbound). The per-pair v
    and the 2×2 S (so R) come from dense_gate, H from its expressions; S = H_J·P·H_Jᵀ + blockdiag(R) is
    factored by Cholesky in dt with v as an extra row (z = L⁻¹v), d2 = Σz², logdet = 2·Σ log L_kk.
    bound = (Σ_a |w_a|·s_a)², w = S⁻¹v, s_a = Σ_k |H_ak|·√P_kk: the gate's first-order bound
    (ekf_gate.h) on the stacked system; ldbound = Σ_ab |S⁻¹_ab|·s_a·s_b, the same for log det S
    (d log det S = tr(S⁻¹·dS), |dS_ab| <= eta·s_a·s_b). A landmark at or past `saved` reads as the zero
    rows the state holds. ok: every pivot positive and finite."""
    lines = np.asarray(lines, dtype=np.float64).reshape(-1, 6)
    assign = np.asarray(assign).reshape(-1)
    act = [i for i in range(len(lines)) if assign[i] >= 0]
    m = len(act)
    if m == 0:
        return dict(m=0, ok=True, d2=dt(0), logdet=dt(0), S=np.zeros((0, 0), dtype=dt), v=np.zeros(0, dtype=dt),
                    bound=0.0, ldbound=0.0)
    n = len(y)
    _, S2, v2, _, _, _ = dense_gate(P, y, (n - 3) // 2, pose, enc, lines, r_mode, dt)
    Pp, xp = predicted(P, pose, enc, dt)
    yy = np.asarray(y, dtype=dt)
    HJ = np.zeros((2 * m, n), dtype=dt)
    v = np.zeros(2 * m, dtype=dt)
    Rb = np.zeros((2 * m, 2 * m), dtype=dt)
    for a, i in enumerate(act):
        j = int(assign[i])
        l0, l1 = 3 + 2 * j, 4 + 2 * j
        ma = yy[l0]
        HJ[2 * a, 2], HJ[2 * a, l0] = -1, 1
        HJ[2 * a + 1, 0], HJ[2 * a + 1, 1] = -np.cos(ma), -np.sin(ma)
        HJ[2 * a + 1, l0], HJ[2 * a + 1, l1] = xp[0] * np.sin(ma) - xp[1] * np.cos(ma), 1
        v[2 * a:2 * a + 2] = v2[i, j]
        R = np.zeros(4, dtype=dt)
        if r_mode == 1:
            if i < 4:
                R[i] = dt(lines[i, 5])
        else:
            R[:] = lines[i, 2:6].astype(dt)
        Rb[2 * a:2 * a + 2, 2 * a:2 * a + 2] = R.reshape(2, 2)
    S = (HJ @ Pp) @ HJ.T + Rb
    for a, i in enumerate(act):   # the diagonal blocks are dense_gate's S of the pair
        blk = S2[i, int(assign[i])].reshape(2, 2)
        assert np.all(np.abs(S[2 * a:2 * a + 2, 2 * a:2 * a + 2] - blk) <= 1e-12 * (1e-300 + np.abs(blk).max()))
    A, z = S.copy(), v.copy()
    logsum, ok = dt(0), True
    for k in range(2 * m):
        piv = A[k, k]
        if not (piv > 0 and np.isfinite(piv)):
            ok = False
            break
        l = np.sqrt(piv)
        logsum = logsum + np.log(l)
        A[k + 1:, k] = A[k + 1:, k] / l
        z[k] = z[k] / l
        A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k + 1:, k])
        z[k + 1:] -= A[k + 1:, k] * z[k]
    out = dict(m=m, ok=ok, S=S, v=v, d2=dt(np.nan), logdet=dt(np.nan), bound=np.nan, ldbound=np.nan)
    if ok:
        out["d2"] = np.sum(z * z)
        out["logdet"] = 2 * logsum
        if dt is np.float64:
            Si = np.linalg.inv(S)
            s = np.abs(HJ) @ np.sqrt(np.abs(np.diag(Pp)))
            out["bound"] = float((np.abs(Si @ v) @ s) ** 2)
            out["ldbound"] = float(s @ np.abs(Si) @ s)
    return out


def hypotheses(match, saved):
    """The cases of one scan from its association `match` (landmark or -1 per line): the association
    itself, each of its single-line sub-hypotheses, and one crossed pairing (the matched lines'
    landmarks rotated by one; a single matched line moved to the next landmark). [(kind, assign)]."""
    match = np.asarray(match, dtype=np.int32)
    on = np.flatnonzero(match >= 0)
    out = [("full", match.copy())]
    for i in on:
        a = np.full_like(match, -1)
        a[i] = match[i]
        out.append(("single", a))
    if len(on) >= 2:
        a = match.copy()
        a[on] = np.roll(match[on], 1)
        out.append(("crossed", a))
    elif len(on) == 1 and saved > 1:
        a = match.copy()
        a[on[0]] = (match[on[0]] + 1) % saved
        out.append(("crossed", a))
    return out


def rel_d(got_d2, want_d2):
    d = float(np.sqrt(abs(want_d2)))
    return abs(float(np.sqrt(abs(got_d2))) - d) / (1 + d)


def rel_ld(got, want):
    return abs(float(got) - float(want)) / (1 + abs(float(want)))


def bits(hit):
    return (hit["m"], hit["status"], np.float64(hit["d2"]).tobytes(), np.float64(hit["logdet"]).tobytes())


# ---------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------
def test_header_declares_the_joint_gate():
    from tests.test_abi import declared_functions
    names = declared_functions()
    for fn in JOINT_FUNCTIONS:
        assert fn in names, fn
    src = open(os.path.join(ROOT, "include", "slam_ekf.h")).read()
    assert "#define SLAM_EKF_ABI_VERSION 3" in src   # entry points only: the number stays
    assert "typedef struct ekf_joint_hit" in src


def test_binding_exports_the_joint_gate(ekf_mod):
    for fn in JOINT_FUNCTIONS:
        assert fn in ekf_mod.EXPORTED, fn
        assert hasattr(ekf_mod.load_library(), fn), fn
    for name in ("gate_joint", "gate_joint_device"):
        assert callable(getattr(ekf_mod.Ensemble, name))
    assert callable(ekf_mod.Robot.gateJoint)
    assert issubclass(ekf_mod.EkfJointHit, ctypes.Structure) and ekf_mod.ekf_joint_hit is ekf_mod.EkfJointHit


def test_null_context_is_einval(ekf_mod):
    lib = ekf_mod.load_library()
    hits = (ekf_mod.EkfJointHit * 2)()
    lines = (ekf_mod.EkfLine * 2)()
    asg = (ctypes.c_int32 * 4)()
    enc = (ctypes.c_double * 3)()
    assert lib.ekf_gate_joint(None, 0, enc, lines, 2, asg, 2, hits, None) == EINVAL
    assert lib.ekf_gate_joint(None, 0, None, None, 0, None, 0, None, None) == EINVAL
    assert lib.ekf_gate_joint_device(None, None, None, None, None, 0, None, None) == EINVAL


def build_joint_driver(tmp_path, ekf_mod):
    exe = tmp_path / "joint_driver"
    libdir = os.path.dirname(ekf_mod.LIB_PATH)
    subprocess.run(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", f"-I{os.path.join(ROOT, 'include')}",
                    f"-I{os.path.join(ROOT, 'slam_ros_amd', 'host')}",
                    os.path.join(ROOT, "tests", "cpp", "joint_driver.cpp"), "-o", str(exe),
                    f"-L{libdir}", "-lslam_ekf", f"-Wl,-rpath,{libdir}"], check=True)
    return exe


def test_joint_driver_compiles_and_structure_size(tmp_path, ekf_mod):
    """BasicRobot::gateJoint compiles against the public header (C++11, -Wall -Werror); the binding's
    structure has the C structure's size and field offsets, taken from the compiled driver."""
    exe = build_joint_driver(tmp_path, ekf_mod)
    out = subprocess.run([str(exe), "--sizeof"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    c = [int(t) for t in out.stdout.split()]
    H = ekf_mod.EkfJointHit
    assert ctypes.sizeof(H) == c[0] == 24
    assert [getattr(H, f).offset for f in ("m", "status", "d2", "logdet")] == c[1:]


def trajectory_cases(oracle_mod):
    """The shared trajectory on the CPU, oracle states: per scan (step, P, y, saved, pose, enc, lines,
    [(kind, assign)]) with the oracle's own association of the scan from that state."""
    N = 64
    w, st = shared_world()
    ref = oracle_mod.OracleRobot(N, mode=oracle_mod.FAST)
    ref.set_state(st.dense_P(), st.y, st.saved, st.pose)
    probe = oracle_mod.OracleRobot(N, mode=oracle_mod.FAST)
    for step, enc, ln, nl in shared_scans(w, 1):
        P, y, s, pose = ref.P_t0.copy(), ref.y.copy(), ref.savedLineCount, np.array(ref.pose, dtype=np.float64)
        lines = ln[0, :nl[0]]
        probe.set_state(P, y, s, pose)
        match = [j if 0 <= j < s else -1 for j in probe.localize(lines, enc[0])]
        yield step, P, y, s, pose, enc[0], lines, hypotheses(match, s)
        ref.localize(lines, enc[0])


def test_the_bar(oracle_mod):
    """The cases mean something and the bars are what the top of this file says: every S of the shared
    trajectory's hypotheses is positive definite (fp64 and longdouble), every scan with a matched line
    has a crossed pairing whose d2 lies above its consistent association's, and the fp64 / longdouble
    spreads of d and logdet are within the pinned figures."""
    sd = sl = 0.0
    kinds = {"full": 0, "single": 0, "crossed": 0}
    for step, P, y, s, pose, enc, lines, hyps in trajectory_cases(oracle_mod):
        d2 = {}
        for kind, asg in hyps:
            r64 = dense_joint(P, y, s, pose, enc, lines, asg)
            rld = dense_joint(P, y, s, pose, enc, lines, asg, dt=np.longdouble)
            assert r64["ok"] and rld["ok"], (step, kind, asg)
            assert r64["m"] == int(np.sum(asg >= 0))
            if r64["m"]:
                assert np.all(np.linalg.eigvalsh(r64["S"]) > 0), (step, kind)
            sd = max(sd, rel_d(r64["d2"], rld["d2"]))
            sl = max(sl, rel_ld(r64["logdet"], rld["logdet"]))
            kinds[kind] += 1
            d2[kind] = float(r64["d2"])
        if "crossed" in d2:
            assert d2["crossed"] > d2["full"], (step, d2)
        else:
            assert not any(k == "single" for k, _ in hyps), step
    print(f"hypotheses {kinds}; fp64 vs longdouble spread: d {sd:.3e}, logdet {sl:.3e}")
    assert kinds == {"full": 20, "single": 67, "crossed": 14}, kinds   # (six scans match no line: after the reset)
    assert np.finfo(np.longdouble).eps < 2e-19      # (x87 extended: the comparison means something)
    assert sd <= SPREAD_D and sl <= SPREAD_LOGDET, (sd, sl)


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
def check_hit(hit, ref, where, eta=0.0):
    """A device hit against dense_joint's: m, status 0, d and logdet within the EXACT bars (eta = 0), or
    d2 within the bar restated for d² plus eta·bound and logdet within its bar plus eta·ldbound (the
    split arithmetics). Returns (|Δd| / (1 + d), |Δlogdet| / (1 + |logdet|))."""
    assert ref["ok"], where
    assert (hit["m"], hit["status"]) == (ref["m"], 0), (where, hit)
    ed, el = rel_d(hit["d2"], ref["d2"]), rel_ld(hit["logdet"], ref["logdet"])
    if eta == 0.0:
        assert ed <= BAR_D, (where, ed, BAR_D)
        assert el <= BAR_LOGDET, (where, el, BAR_LOGDET)
    else:
        d = float(np.sqrt(abs(ref["d2"])))
        # |Δd| <= BAR_D·(1 + d) gives |Δd²| <= 2·BAR_D·(1 + d)² (test_gate.check_against_dense)
        assert abs(hit["d2"] - float(ref["d2"])) <= 2 * BAR_D * (1 + d) ** 2 + eta * ref["bound"], (where, hit, ref["d2"])
        assert abs(hit["logdet"] - float(ref["logdet"])) <= \
            BAR_LOGDET * (1 + abs(float(ref["logdet"]))) + eta * ref["ldbound"], (where, hit, ref["logdet"])
    return ed, el


def run_against_dense(ekf_mod, oracle_mod, prec, T, arith=0, eta=0.0):
    """a (flush interval T) is queried before every scan of the shared trajectory with the hypotheses
    of `hypotheses` (the oracle's association from the twin's state) against dense_joint on the dense
    state of its twin b, which is drained after every scan. No hypothesis is excluded."""
    N = 64
    w, st = shared_world()
    a = make(ekf_mod, N, 1, prec, st, flush_interval=T, arith=arith)
    b = make(ekf_mod, N, 1, prec, st, flush_interval=T, arith=arith)
    probe = oracle_mod.OracleRobot(N, mode=oracle_mod.FAST)
    worst_d = worst_l = 0.0
    cases = {"full": 0, "single": 0, "crossed": 0}
    for step, enc, ln, nl in shared_scans(w, 1):
        Pb, yb, sb, pb = b.download_state(0)          # (drains b)
        lines = ln[0, :nl[0]]
        probe.set_state(Pb, yb, sb, pb)
        match = [j if 0 <= j < sb else -1 for j in probe.localize(lines, enc[0])]
        hyps = hypotheses(match, sb)
        hits = a.gate_joint(0, lines, np.stack([h[1] for h in hyps]), enc[0])
        for (kind, asg), hit in zip(hyps, hits):
            ref = dense_joint(Pb, yb, sb, pb, enc[0], lines, asg)
            ed, el = check_hit(hit, ref, (step, kind, asg.tolist()), eta)
            worst_d, worst_l = max(worst_d, ed), max(worst_l, el)
            cases[kind] += 1
        a.localize(enc, ln, nl)
        b.localize(enc, ln, nl)
    print(f"prec {prec} arith {arith} T {T}: {cases}; worst |dd| / (1 + d) {worst_d:.3e} (EXACT bar {BAR_D:.3e}), "
          f"worst |dlogdet| / (1 + |logdet|) {worst_l:.3e} (EXACT bar {BAR_LOGDET:.3e})")
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [0, 1, 2])
def test_against_the_dense_state(ekf_mod, oracle_mod, prec):
    """EXACT, mid-group (T = 8): d, logdet, m and status 0 of every hypothesis of the shared trajectory
    against dense_joint on the drained twin's dense state, within BAR_D and BAR_LOGDET.

    Measured on an MI355X (printed on every run), worst |Δd| / (1 + d) and |Δlogdet| / (1 + |logdet|):
    fp64 storage 1.8e-16 and 2.1e-16, fp32 2.1e-16 and 2.1e-16, fp16 1.8e-16 and 0, against 2.97e-11
    and 2.46e-12."""
    cases = run_against_dense(ekf_mod, oracle_mod, prec, 8)
    assert cases["full"] == 20 and cases["single"] >= 60 and cases["crossed"] >= 12, cases


@pytest.mark.gpu
@pytest.mark.parametrize("prec,arith,T", [(1, 1, 8), (1, 2, 8), (2, 2, 16)])
def test_split_arithmetics(ekf_mod, oracle_mod, prec, arith, T):
    """The split arithmetics on the same trajectory: |Δd²| within the EXACT bar plus eta·(Σ_a |w_a|·s_a)²,
    eta 2^-16 for fp32 and 2^-8 for fp16 storage (the gate's bound, ekf_gate.h, on the stacked system);
    logdet within its EXACT bar plus eta·Σ_ab |S⁻¹_ab|·s_a·s_b (the same |ΔS_ab| <= eta·s_a·s_b through
    d log det S = tr(S⁻¹·dS)).

    Measured on an MI355X, worst |Δd| / (1 + d) and |Δlogdet| / (1 + |logdet|) (printed on every run):
    BF16X6 fp32 5.6e-9 and 3.8e-9, F16X3 fp32 4.9e-9 and 2.2e-9, F16X3 fp16 9.2e-5 and 3.2e-5."""
    run_against_dense(ekf_mod, oracle_mod, prec, T, arith=arith, eta=ETA[prec])


def gate_walk(ekf_mod, steps, prec=1, T=8):
    """Before every scan of the shared trajectory: (a, step, enc, lines, gate hits, gate d2)."""
    w, st = shared_world()
    a = make(ekf_mod, 64, 1, prec, st, flush_interval=T)
    for step, enc, ln, nl in shared_scans(w, 1, steps=steps):
        lines = ln[0, :nl[0]]
        hg, dg = a.gate_lines(0, lines, enc[0], distances=True)
        yield a, step, enc[0], lines, hg, dg
        a.localize(enc, ln, nl)


@pytest.mark.gpu
def test_d2_each_is_the_gates(ekf_mod):
    """d2_each[h][i] is bit for bit ekf_gate_lines' d2[i][assign[h][i]] on the same context at the same
    point (mid-group), and NaN where the line is unassigned."""
    checked = 0
    for a, step, enc, lines, hg, dg in gate_walk(ekf_mod, 9):
        asg = np.array([[h["first"] for h in hg], [h["nearest"] for h in hg]], dtype=np.int32)
        _, each = a.gate_joint(0, lines, asg, enc, each=True)
        for h in range(2):
            for i in range(len(lines)):
                if asg[h, i] >= 0:
                    assert each[h, i].tobytes() == dg[i, asg[h, i]].tobytes(), (step, h, i)
                    checked += 1
                else:
                    assert np.isnan(each[h, i]), (step, h, i)
    assert checked >= 60


@pytest.mark.gpu
def test_single_line_against_the_gate(ekf_mod):
    """m = 1: d2 of a one-line hypothesis within BAR_D of the gate's d2_first for the same pair
    (Cholesky of the 2×2 S against the gate's LU), and logdet = log det of the hit's S."""
    worst, n = 0.0, 0
    for a, step, enc, lines, hg, dg in gate_walk(ekf_mod, 9):
        on = [i for i, h in enumerate(hg) if h["first"] >= 0]
        if not on:
            continue
        asg = np.full((len(on), len(lines)), -1, dtype=np.int32)
        for k, i in enumerate(on):
            asg[k, i] = hg[i]["first"]
        for k, hit in enumerate(a.gate_joint(0, lines, asg, enc)):
            g = hg[on[k]]
            assert (hit["m"], hit["status"]) == (1, 0)
            err = rel_d(hit["d2"], g["d2_first"])
            assert err <= BAR_D, (step, on[k], err)
            assert rel_ld(hit["logdet"], np.log(np.linalg.det(g["S"]))) <= BAR_LOGDET, (step, on[k])
            worst, n = max(worst, err), n + 1
    print(f"{n} single-line hypotheses: worst |dd| / (1 + d) against the gate {worst:.3e}")
    assert n >= 30


def edge_hypotheses(L, saved_hint=64):
    """Landmarks 15 and 16 (a tile edge) in both line orders, a run of landmarks across that edge, and a
    spread over the whole capacity (at and past savedLineCount among them)."""
    h = np.full((4, L), -1, dtype=np.int32)
    h[0, :2] = (15, 16)
    h[1, :2] = (16, 15)
    h[2] = 13 + np.arange(L)
    h[3] = (7 * np.arange(L) + 1) % saved_hint
    return h


@pytest.mark.gpu
def test_mid_group_identity(ekf_mod):
    """EXACT on fp32 storage, T = 8 against a twin with flush_interval 1, queried before every scan of
    the shared trajectory (0 .. 7 steps pending; groups with augmented rows; the capacity reset inside
    the second group): hits and d2_each bit-identical."""
    w, st = shared_world()
    a = make(ekf_mod, 64, 1, 1, st, flush_interval=8)
    b = make(ekf_mod, 64, 1, 1, st, flush_interval=1)
    pend, after_reset, after_aug = set(), 0, 0
    reset_in_group = aug_in_group = False
    saved, edge_live = st.saved, 0
    for step, enc, ln, nl in shared_scans(w, 1):
        np_ = (step - 1) % 8
        if np_ == 0:
            reset_in_group = aug_in_group = False
        lines = ln[0, :nl[0]]
        asg = edge_hypotheses(len(lines))
        ha, ea = a.gate_joint(0, lines, asg, enc[0], each=True)
        hb, eb = b.gate_joint(0, lines, asg, enc[0], each=True)
        assert [bits(h) for h in ha] == [bits(h) for h in hb], (step, ha, hb)
        assert ea.tobytes() == eb.tobytes(), step
        assert all(h["status"] == 0 and h["m"] == int(np.sum(asg[k] >= 0)) for k, h in enumerate(ha))
        assert bits(ha[0]) != bits(ha[1]) or saved <= 16          # (zero rows give both orders the same S = R)
        pend.add(np_)
        edge_live += saved > 16
        after_reset += reset_in_group
        after_aug += aug_in_group
        ra = a.localize(enc, ln, nl)
        b.localize(enc, ln, nl)
        reset_in_group |= bool(ra[0]["reset"])
        aug_in_group |= ra[0]["new_landmarks"] > 0
        saved = ra[0]["saved"]
    assert {0, 1, 7} <= pend and after_reset >= 1 and after_aug >= 1 and edge_live >= 12, (pend, after_reset, after_aug, edge_live)
    Pa, ya, sa, pa = a.download_state(0)
    Pb, yb, sb, pb = b.download_state(0)
    assert np.array_equal(Pa, Pb) and np.array_equal(ya, yb) and sa == sb


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline,T", [(False, 8), (True, 3)])
def test_state_untouched(ekf_mod, pipeline, T):
    """A context queried before every scan ends bit-identical (P, y, pose, saved) to a twin never
    queried and ran the same flush launches."""
    E = 2
    w, st = shared_world()
    a = make(ekf_mod, 64, E, 1, st, pipeline=pipeline, flush_interval=T)
    c = make(ekf_mod, 64, E, 1, st, pipeline=pipeline, flush_interval=T)
    a.profile(1)
    c.profile(1)
    for step, enc, ln, nl in shared_scans(w, E):
        for e in range(E):
            hits = a.gate_joint(e, ln[e, :nl[e]], edge_hypotheses(int(nl[e])), enc[e])
            assert all(h["status"] == 0 for h in hits)
        a.localize(enc, ln, nl)
        c.localize(enc, ln, nl)
    fa = [n for n, _ in a.profile_flushes()]
    fc = [n for n, _ in c.profile_flushes()]
    assert fa == fc == [T] * (20 // T), (fa, fc)          # the query never drained
    for e in range(E):
        Pa, ya, sa, pa = a.download_state(e)
        Pc, yc, sc, pc = c.download_state(e)
        assert np.array_equal(Pa, Pc), (e, np.argwhere(Pa != Pc)[:8].tolist())
        assert np.array_equal(ya, yc) and np.array_equal(pa, pc) and sa == sc


def device_joint(ekf_mod, a, enc, ln, counts, assign, each=True):
    """ekf_gate_joint_device on (enc [E, 3] or None, ln [E, ML, 6], counts [E], assign [E, H, ML]): the
    hits as dicts [E][H] and d2_each [E, H, ML] (prefilled with -1)."""
    from tests.hipmem import DeviceArray, hip
    E, H, ML = assign.shape
    JH = ekf_mod.EkfJointHit
    bufs = [DeviceArray(ln), DeviceArray(np.asarray(counts, dtype=np.int32)), DeviceArray(assign.astype(np.int32)),
            DeviceArray(np.full(E * H * ctypes.sizeof(JH), 0x5a, dtype=np.uint8)), DeviceArray(np.full((E, H, ML), -1.0))]
    d_enc = DeviceArray(enc) if enc is not None else None
    a.gate_joint_device(d_enc.address if d_enc else 0, bufs[0].address, bufs[1].address, bufs[2].address, H,
                        bufs[3].address, bufs[4].address if each else 0)
    a.sync()
    raw = (JH * (E * H))()
    assert hip().hipMemcpy(ctypes.byref(raw), bufs[3].ptr, ctypes.sizeof(raw), 2) == 0
    d2 = np.zeros((E, H, ML))
    assert hip().hipMemcpy(d2.ctypes.data_as(ctypes.c_void_p), bufs[4].ptr, d2.nbytes, 2) == 0
    for d in bufs + ([d_enc] if d_enc else []):
        d.close()
    return [[a._joint_hit(raw[e * H + h]) for h in range(H)] for e in range(E)], d2


@pytest.mark.gpu
def test_order_independence(ekf_mod):
    """One hypothesis placed first, in the middle and last of a list of H = 37 gives the same bits each
    time, equal to its bits alone; the device form gives the host form's bits for all 37."""
    w, st = shared_world()
    a = make(ekf_mod, 64, 1, 1, st, flush_interval=8)
    scans = list(shared_scans(w, 1, steps=6))
    for step, enc, ln, nl in scans[:5]:
        a.localize(enc, ln, nl)
    step, enc, ln, nl = scans[5]                      # step 6: eight lines, five steps pending
    L = 8
    assert nl[0] == L
    rng = np.random.default_rng(3)
    asg = rng.integers(-1, 52, size=(37, L)).astype(np.int32)
    X = np.array([15, 16, 14, -1, 17, 40, 3, 16], dtype=np.int32)
    asg[0] = asg[17] = asg[36] = X
    hits, each = a.gate_joint(0, ln[0], asg, enc[0], each=True)
    alone, each1 = a.gate_joint(0, ln[0], X[None], enc[0], each=True)
    assert bits(hits[0]) == bits(hits[17]) == bits(hits[36]) == bits(alone[0]), (hits[0], hits[17], hits[36], alone)
    assert each[0].tobytes() == each[17].tobytes() == each[36].tobytes() == each1[0].tobytes()
    assert hits[0]["m"] == 7 and hits[0]["status"] == 0 and len({bits(h) for h in hits}) >= 30
    dh, de = device_joint(ekf_mod, a, enc, ln, nl, asg[None])
    assert [bits(h) for h in dh[0]] == [bits(h) for h in hits]
    assert de[0].tobytes() == each.tobytes()


def lines_of_state(rng, y, pose, landmarks, noise=1e-3):
    """Observations of `landmarks` built from the state itself: z = h(y_j, pose) + noise, R = 1e-4·I."""
    out = G.random_lines(rng, len(landmarks))
    for i, j in enumerate(landmarks):
        al, r = y[3 + 2 * j], y[4 + 2 * j]
        out[i, 0] = G.wrap_pi(al - pose[2]) + noise * rng.normal()
        out[i, 1] = r - (pose[0] * np.cos(al) + pose[1] * np.sin(al)) + noise * rng.normal()
    return out


@pytest.mark.gpu
def test_widths(ekf_mod):
    """N = 96, max_lines = 64, EXACT on fp64 storage, three steps pending: m = 9 (odd), 33 (2m = 66, past
    one wave) and 64 (2m = 128, the LDS limit) distinct landmarks, and m = 64 with one landmark used
    twice, against dense_joint on a drained twin's state; numpy's S is positive definite first."""
    N, ML = 96, 64
    w = G.make_world(N, active=80)
    st = G.initial_state(w)
    ens = []
    for _ in range(2):
        x = ekf_mod.Ensemble(N, 1, 0, max_lines=ML, flush_interval=8)
        x.init_lowrank(0, st.diag, st.U, st.y, st.saved, st.pose)
        ens.append(x)
    a, b = ens
    for step in range(1, 4):
        enc, ln, nl = G.make_scan(w, step, lines=8)
        a.localize(enc, ln, nl)
        b.localize(enc, ln, nl)
    P, y, s, pose = b.download_state(0)
    rng = np.random.default_rng(21)
    perm = rng.choice(s, size=ML, replace=False)
    lines = lines_of_state(rng, y, pose, perm)
    asg = np.full((3, ML), -1, dtype=np.int32)
    for k, m in enumerate((9, 33, 64)):
        asg[k, :m] = perm[:m]
    twice = perm.copy()
    twice[63] = perm[0]
    lines2 = lines_of_state(rng, y, pose, twice)
    cases = [(lines, asg[k], f"m {m}") for k, m in enumerate((9, 33, 64))] + [(lines2, twice.astype(np.int32), "m 64, one twice")]
    refs = []
    for ln_, asg_, name in cases:
        ref = dense_joint(P, y, s, pose, None, ln_, asg_)
        assert ref["ok"] and np.all(np.linalg.eigvalsh(ref["S"]) > 0), name
        refs.append(ref)
    hits = a.gate_joint(0, lines, asg) + a.gate_joint(0, lines2, twice[None])
    for hit, ref, (_, _, name) in zip(hits, refs, cases):
        ed, el = check_hit(hit, ref, name)
        print(f"{name}: d2 {hit['d2']:.6g} logdet {hit['logdet']:.6g}; |dd| / (1 + d) {ed:.3e}, |dlogdet| / (1 + |logdet|) {el:.3e}")
    assert [h["m"] for h in hits] == [9, 33, 64, 64]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", [0, 1])
def test_predict_on_read(ekf_mod, prec):
    """gate_joint(e, lines, assign, enc) on one context equals ekf_predict(enc) then gate_joint with enc
    None on its twin, bit for bit, mid-group; with the predict pending an encoder pose is EKF_EINVAL."""
    E = 2
    w, st = shared_world()
    a = make(ekf_mod, 64, E, prec, st, flush_interval=8)
    b = make(ekf_mod, 64, E, prec, st, flush_interval=8)
    scans = list(shared_scans(w, E, steps=5))
    for step, enc, ln, nl in scans[:4]:
        a.localize(enc, ln, nl)
        b.localize(enc, ln, nl)
    step, enc, ln, nl = scans[4]
    b.predict(enc)
    for e in range(E):
        lines = ln[e, :nl[e]]
        asg = edge_hypotheses(len(lines), 50)
        ha, ea = a.gate_joint(e, lines, asg, enc[e], each=True)
        hb, eb = b.gate_joint(e, lines, asg, None, each=True)
        assert [bits(h) for h in ha] == [bits(h) for h in hb], (e, ha, hb)
        assert ea.tobytes() == eb.tobytes()
        assert all(h["status"] == 0 and h["d2"] > 0 for h in ha)
        with pytest.raises(ekf_mod.EkfError) as err:
            b.gate_joint(e, lines, asg, enc[e])
        assert err.value.code == EINVAL
        # the committed pose with no motion is another question: other bits
        assert [bits(h) for h in a.gate_joint(e, lines, asg, None)] != [bits(h) for h in ha]
    rb = b.update(ln, nl)
    ra = a.localize(enc, ln, nl)
    for e in range(E):
        assert ra[e]["match"] == rb[e]["match"]
        b.gate_joint(e, ln[e, :nl[e]], edge_hypotheses(int(nl[e]), 50), enc[e])          # accepted again
        assert np.array_equal(a.download_state(e)[0], b.download_state(e)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("pipeline,T", [(False, 8), (True, 3)])
def test_device_form(ekf_mod, pipeline, T):
    """ekf_gate_joint_device with E = 3, H = 5, nlines = (8, 0, 3): the hits equal the host form's bit for
    bit; an out-of-range entry gives NaN and EKF_ST_SINGULAR_S for its hypothesis only; entries at and
    past nlines[e] are ignored; asynchronous calls followed at once by a drain and by further groups
    leave the trajectory bit-identical to a twin never queried."""
    from tests.hipmem import DeviceArray
    N, E, H, ML = 64, 3, 5, 8
    w, st = shared_world()
    a = make(ekf_mod, N, E, 1, st, pipeline=pipeline, flush_interval=T)
    c = make(ekf_mod, N, E, 1, st, pipeline=pipeline, flush_interval=T)
    scans = list(shared_scans(w, E, steps=9))
    for step, enc, ln, nl in scans[:5]:
        a.localize(enc, ln, nl)
        c.localize(enc, ln, nl)
    step, enc, ln, nl = scans[5]                      # step 6: eight lines
    assert ln.shape[1] == ML
    counts = np.array([8, 0, 3], dtype=np.int32)
    rng = np.random.default_rng(9)
    asg = rng.integers(-1, 52, size=(E, H, ML)).astype(np.int32)
    asg[0, 1, :2] = (15, 16)
    asg[0, 2, 1] = N                                  # out of range: hypothesis (0, 2)
    asg[2, 1, 0] = -2                                 # ... and (2, 1)
    asg[2, 0, 5] = 1 << 20                            # past nlines[2]: ignored
    asg[2, 3, :3] = -1                                # empty
    bad = {(0, 2), (2, 1)}
    dh, de = device_joint(ekf_mod, a, enc, ln, counts, asg)
    for e in range(E):
        cnt = int(counts[e])
        for h in range(H):
            got = dh[e][h]
            if (e, h) in bad:
                assert got["status"] == ST_SINGULAR and np.isnan(got["d2"]) and np.isnan(got["logdet"]), (e, h, got)
                assert np.all(np.isnan(de[e, h, :cnt]))
            else:
                want, each = a.gate_joint(e, ln[e, :cnt], asg[e, h:h + 1, :cnt], enc[e], each=True)
                assert bits(got) == bits(want[0]), (e, h, got, want)
                assert got["status"] == 0
                assert de[e, h, :cnt].tobytes() == each.tobytes()
            assert np.all(de[e, h, cnt:] == -1.0)     # untouched
    assert dh[1][0]["m"] == 0 and dh[2][3] == dict(m=0, status=0, d2=0.0, logdet=0.0) and dh[0][1]["m"] >= 2
    # asynchronous: a drain right behind a query, then the rest of the trajectory with a query per scan
    bufs = [DeviceArray(enc), DeviceArray(ln), DeviceArray(counts), DeviceArray(asg),
            DeviceArray(np.zeros(E * H * ctypes.sizeof(ekf_mod.EkfJointHit), dtype=np.uint8)), DeviceArray(np.zeros((E, H, ML)))]
    adr = [d.address for d in bufs]
    a.gate_joint_device(adr[0], adr[1], adr[2], adr[3], H, adr[4], 0)
    a.gate_joint_device(0, adr[1], adr[2], adr[3], H, adr[4], adr[5])
    for step, enc, ln, nl in scans[5:]:
        a.localize(enc, ln, nl)
        c.localize(enc, ln, nl)
        a.gate_joint_device(adr[0], adr[1], adr[2], adr[3], H, adr[4], adr[5])
    for e in range(E):
        Pa, ya, sa, _ = a.download_state(e)
        Pc, yc, sc, _ = c.download_state(e)
        assert np.array_equal(Pa, Pc) and np.array_equal(ya, yc) and sa == sc, e
    for d in bufs:
        d.close()


@pytest.mark.gpu
def test_edges(ekf_mod):
    """The empty map (every landmark reads as the zero rows the state holds); H = 0 and L = 0; an all -1 hypothesis;
    the error returns; a singular S (two lines on one landmark of an all-zero state with R = 0) gives
    EKF_ST_SINGULAR_S and NaN without a fault."""
    N, E = 16, 2
    a = ekf_mod.Ensemble(N, E, 1, max_lines=8, flush_interval=4)
    rng = np.random.default_rng(5)
    lines = G.random_lines(rng, 3)
    asg = np.array([[0, -1, 2], [-1, -1, -1], [5, 5, 15]], dtype=np.int32)
    P, y, s, pose = a.download_state(1)
    assert s == 0
    hits, each = a.gate_joint(1, lines, asg, None, each=True)
    for k in (0, 2):
        ed, el = check_hit(hits[k], dense_joint(P, y, s, pose, None, lines, asg[k]), ("empty map", k))
    assert hits[0]["m"] == 2 and hits[2]["m"] == 3
    assert not P[3:, :].any() and P[:3, :3].any()        # (only the pose block: every landmark reads as zero rows)
    assert hits[1] == dict(m=0, status=0, d2=0.0, logdet=0.0) and np.all(np.isnan(each[1]))
    assert np.isnan(each[0, 1]) and np.all(np.isfinite(each[[0, 0, 2, 2, 2], [0, 2, 0, 1, 2]]))
    a.gate_joint(1, lines, asg, [0.01, 0.0, 0.0])                       # with a predict on read
    assert a.gate_joint(0, lines, np.zeros((0, 3), dtype=np.int32)) == []          # H == 0
    assert a.gate_joint(0, np.zeros((0, 6)), np.zeros((3, 0), dtype=np.int32)) == [dict(m=0, status=0, d2=0.0, logdet=0.0)] * 3
    lib, h = ekf_mod.load_library(), a.handle
    JH = (ekf_mod.EkfJointHit * 4)()
    ln = (ekf_mod.EkfLine * 9)()
    enc = (ctypes.c_double * 3)()
    ok = (ctypes.c_int32 * 18)(*([0, 1] * 9))
    assert lib.ekf_gate_joint(h, 0, enc, ln, 2, ok, 2, JH, None) == 0
    assert lib.ekf_gate_joint(h, E, enc, ln, 2, ok, 2, JH, None) == ERANGE
    assert lib.ekf_gate_joint(h, -1, enc, ln, 2, ok, 2, JH, None) == ERANGE
    assert lib.ekf_gate_joint(h, 0, enc, ln, 9, ok, 2, JH, None) == ERANGE
    assert lib.ekf_gate_joint(h, 0, enc, ln, -1, ok, 2, JH, None) == ERANGE
    assert lib.ekf_gate_joint(h, 0, enc, ln, 2, ok, -1, JH, None) == ERANGE
    for badv in (N, -2):
        bad = (ctypes.c_int32 * 4)(0, 1, badv, 1)
        assert lib.ekf_gate_joint(h, 0, enc, ln, 2, bad, 2, JH, None) == ERANGE
    assert lib.ekf_gate_joint(h, 0, enc, None, 2, ok, 2, JH, None) == EINVAL
    assert lib.ekf_gate_joint(h, 0, enc, ln, 2, None, 2, JH, None) == EINVAL
    assert lib.ekf_gate_joint(h, 0, enc, ln, 2, ok, 2, None, None) == EINVAL
    assert lib.ekf_gate_joint(h, 0, None, None, 0, None, 0, None, None) == 0
    assert lib.ekf_gate_joint_device(h, None, None, None, None, 2, None, None) == EINVAL
    assert lib.ekf_gate_joint_device(h, None, ln, ln, ok, -1, JH, None) == ERANGE
    sh = ekf_mod.Ensemble(64, 1, 1, max_lines=8, flush_interval=4, shard=(0, 1))
    assert lib.ekf_gate_joint(sh.handle, 0, enc, ln, 2, ok, 2, JH, None) == EINVAL
    assert lib.ekf_gate_joint_device(sh.handle, None, ln, ln, ok, 2, JH, None) == EINVAL
    # singular
    z = ekf_mod.Ensemble(N, 1, 0, max_lines=8, flush_interval=4)
    n = 3 + 2 * N
    z.upload_state(0, np.zeros((n, n)), np.zeros(n), 1, np.zeros(3))
    flat = np.array([[0.1, 1.0, 0, 0, 0, 0], [0.2, 1.1, 0, 0, 0, 0]])
    hits = z.gate_joint(0, flat, np.array([[0, 0], [-1, -1]], dtype=np.int32))
    assert hits[0]["status"] == ST_SINGULAR and hits[0]["m"] == 2 and np.isnan(hits[0]["d2"]) and np.isnan(hits[0]["logdet"])
    assert hits[1] == dict(m=0, status=0, d2=0.0, logdet=0.0)
    Pz, yz, sz, _ = z.download_state(0)
    assert not Pz.any() and not yz.any() and sz == 1


@pytest.mark.gpu
def test_r_as_written_follows_the_index(ekf_mod):
    """EKF_R_AS_WRITTEN on fp64: R is built from the line's index in the list (Robot.cpp:302-304), so
    the same line on the same landmark at index 0, 1 and 3 gives different hits (index 1's R lands
    above the diagonal, which the lower-only S leaves out: S = H·P·Hᵀ); all against numpy."""
    w, st = shared_world()
    a = ekf_mod.Ensemble(64, 1, 0, max_lines=8, r_mode=1, flush_interval=4)
    a.init_lowrank(0, st.diag, st.U, st.y, st.saved, st.pose)
    enc, ln, nl = G.make_scan(w, 1, lines=6)
    a.localize(enc, ln, nl)
    P, y, s, pose = a.download_state(0)
    enc2, ln2, _ = G.make_scan(w, 2, lines=6)
    lines = ln2[0, :6].copy()
    j = a.gate_lines(0, lines, enc2[0])[0]["nearest"]
    lines[1] = lines[0]
    lines[3] = lines[0]
    asg = np.full((3, 6), -1, dtype=np.int32)
    asg[0, 0] = asg[1, 1] = asg[2, 3] = j
    hits = a.gate_joint(0, lines, asg, enc2[0])
    for k in range(3):
        check_hit(hits[k], dense_joint(P, y, s, pose, enc2[0], lines, asg[k], r_mode=1), ("as written", k))
    assert len({bits(h) for h in hits}) == 3


@pytest.mark.gpu
def test_cpp_driver_against_python(tmp_path, ekf_mod):
    """BasicRobot::gateJoint: the driver's two scans and one hypothesis, and the same through
    Robot.gateJoint: the same hit, bit for bit."""
    exe = build_joint_driver(tmp_path, ekf_mod)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    rows = [r.split() for r in out.stdout.strip().splitlines()]
    obs = [(-2.4, 1.1), (-1.0, 2.3), (0.2, 0.8), (1.3, 3.1), (2.6, 1.9)]
    rob = ekf_mod.Robot(0.0, 0.0, 0.0, capacity=100, precision=0, max_lines=64)
    for k in range(2):
        enc = [0.01 * (k + 1), -0.005 * (k + 1), 0.002 * (k + 1)]
        rob.localize([[a - (enc[2] if k else 0.0), r, 1e-2, 0, 0, 1e-2] for a, r in obs], encoder=enc)
    enc = [0.022, -0.011, 0.0044]
    trial = [[a - enc[2], r, 1e-2, 0, 0, 1e-2] for a, r in obs]
    hit = rob.gateJoint(trial, [[0, 1, 2, -1, 4]], encoder=enc)[0]
    assert rows[-1] == ["saved", str(rob.savedLineCount)] and len(rows) == 2
    r = rows[0]
    assert r[0] == "hit" and [int(t) for t in r[1:3]] == [hit["m"], hit["status"]] == [4, 0], (r, hit)
    assert float(r[3]) == hit["d2"] and float(r[4]) == hit["logdet"], (r, hit)
    assert 0 < hit["d2"] < 1.0
