"""Every association mode (EKF_OPT_SPECULATE 0..3) on the split arithmetics, against the fp64
restatement (oracle/), and the status bits a failed verdict's restart keeps and drops.

On a split-arithmetic context (EKF_ARITH_BF16X6 / EKF_ARITH_F16X3, fp32 or fp16 storage, max_lines
<= 8, EKF_R_INTENDED) with pending steps and EKF_OPT_MFMA_REPLAY != 0 the association kernel replays
the pending steps by MFMA (`mf`, ekf_kernels.hip scan_kernel: "bool mf"), and the restart after a
failed verdict seeds the owned diagonal block from Dd ("const double4 b = Ddr[j]") and re-runs the
kept lines from the speculative pass's cached blocks (sh_cblk). The modes are NOT bit-identical
there, by construction:

  * mode 0 has spec_ok false, hence mf false: it reads every block through pll_block — per pending
    step an fmaf chain INTO the stored block, rounded to storage per step (pll_blocks). Modes 1..3
    read ΔX = Σ_q V_q·V_qᵀ accumulated from zero over all pending steps by plane_replay (the split
    products) or f32_replay (EKF_OPT_MFMA_REPLAY = 2: exact fp32 products, but accumulated from
    zero in the MFMA's k order and subtracted once) — another rounding sequence in either form, so
    also `mfma_replay = 2` is not bit-identical to mode 0: slam_ekf.h claims the EXACT arithmetic's
    precision for it, not its bits.
  * after a restart (modes 2, 3) the columns whose winner was guessed come from the MFMA replay's
    cache (owned_block: sh_cblk), the others from pll_block: neither mode 0's nor mode 1's mix.

What the code does claim bit for bit, and is asserted here:

  * EKF_OPT_MFMA_REPLAY = 0: the staged replay is "per element the same chain as pll_blocks"
    (staged_blocks), so all four modes give the same bits on the split arithmetics too
    (test_per_element_replay_modes_bit_identical);
  * EKF_OPT_SCAN_THREADS ("identical results for every value"): every dot product of either MFMA
    replay has its own accumulator and the same term order whatever the tiling, the guesses and the
    test hooks are per line, not per workgroup: 64 / 128 against 192 landmarks per workgroup within
    every mode, mode 3 included (test_scan_width_bit_identical).

Everything else is held to the project's bars against the restatement, per flush group from
identical inputs (tests/test_bench_config.py run_config's method): ‖ΔP‖_F/‖P‖_F <= P_TOL (fp32
storage 1e-6, fp16 storage 1e-3), ‖Δy‖/‖y‖ <= 1e-8, pose within check_same's 1e-9, saved equal,
association / matches / new landmarks of every scan identical and status 0 — and the per-scan
result tuples equal across the four modes.

The path words (RES_DBG: 8 verdict failed, 512 lines kept, 64 the pending replay took an exact
form, 128 pending reset, 256 foreign plane exponent) prove that the restart under test ran. The
measured group errors and path counts go to spec_modes_parity.json, next to the bench
configurations' record (tests/test_bench_config.py record).

Measured on an MI355X, all 52 cases and four modes: every scan of modes 2 and 3 restarts (16 of
16, lines kept on all 16 in mode 3), none in mode 1, no pending reset and no foreign plane
exponent anywhere (the plane replay proper runs); group error of P 1.8e-7 .. 3.4e-7 on fp32 storage
and 1.5e-4 .. 2.0e-4 on fp16 storage (its floor is the rounding to fp16 once per group), y <=
3.6e-12, pose <= 1.5e-11. Sensitivity: with the restart's diagonal block seeded from the last
flushed block instead of Dd (a mutated build, not kept), modes 2 and 3 of every fp32-storage case
with the MFMA replay miss the bar by 2.8e-4 .. 0.12 (bar 1e-6); on fp16 storage only N = 64, T = 8
does (0.12 and 1.0e-3) — at N >= 256 that error is 3.5e-4 .. 7.3e-4, under the re-stated fp16 bar,
so there the fp32-storage cases of the same kernel path carry the sensitivity.
"""
import hashlib
import json

import numpy as np
import pytest

from slam_ros_amd import scan_gen as G
from tests.test_bench_config import record as bench_record
from tests.test_gpu_parity import P_TOL, Y_TOL, _spec_scans, rel

pytestmark = pytest.mark.gpu

POSE_ATOL = 1e-9     # check_same's (fp32 / fp16 storage)
SCANS = 16           # savedLineCount ends at N − 10 at most: no capacity reset (a reset inside a
#                      group sends it to the exact forms, which is not what this module is about)
MODES = (0, 1, 2, 3)
BF16X6, F16X3 = 1, 2

# (N, T, scan_threads). scan_threads = 0 is the automatic width: the narrowest that fits, 64 at
# these sizes. N = 64: one workgroup; N = 256: four workgroups of 64, two of 192; N = 1000: eight of
# 128 with a partial last one (104 landmarks), six of 192 (40). (64, 8, 0): scan 13 matches
# landmark 44, which scan 9 of the same flush group added (the patch_block / addq path on a matched
# column); at T = 4 the two fall into different groups.
SHAPES = [(64, 4, 0), (256, 8, 0), (256, 8, 64), (1000, 8, 128)]
WIDE = [(64, 8, 0), (256, 8, 192)]
CASES = [(a, p, rep, N, T, nt) for a in (BF16X6, F16X3) for p in (1, 2) for rep in (1, 2)
         for (N, T, nt) in SHAPES + WIDE]
CASES += [(a, 1, 1, 1000, 8, 192) for a in (BF16X6, F16X3)]
# the LDS-staged per-element replay (staged && !mf) under restarts
CASES += [(a, 1, 0, 256, 8, 0) for a in (BF16X6, F16X3)]


def case_id(c):
    a, p, rep, N, T, nt = c
    return f"{'bf16x6' if a == BF16X6 else 'f16x3'}-{'f32' if p == 1 else 'f16'}-rep{rep}-N{N}-T{T}-w{nt}"


def record(key, value):
    bench_record(key, value, name="spec_modes_parity.json")


def digest(a):
    """The bits of an array, −0 folded into +0 (as assert_array_equal compares)."""
    return hashlib.sha256(np.ascontiguousarray(np.asarray(a, dtype=np.float64) + 0.0).tobytes()).hexdigest()


_WORLDS = {}
_RUNS = {}


def world_of(N):
    """World, initial state and the 16 scans of test_speculative_association_identical (shared)."""
    if N not in _WORLDS:
        w = G.make_world(N, active=N - 30)
        _WORLDS[N] = (G.initial_state(w), _spec_scans(w, np.random.default_rng(3), SCANS))
    return _WORLDS[N]


def collect(ekf_mod, oracle_mod, case):
    """One case: the four modes, each on a fresh context with its own restatement re-synced to it
    at every group end. Measures only (no assertion), once per case and session."""
    if case in _RUNS:
        return _RUNS[case]
    arith, prec, rep, N, T, nt = case
    st, scans = world_of(N)
    out = {}
    for mode in MODES:
        ens = ekf_mod.Ensemble(N, 1, prec, max_lines=8, flush_interval=T, arith=arith,
                               options={"speculate": mode, "mfma_replay": rep, "scan_threads": nt})
        ens.init_lowrank(0, st.diag, st.U, st.y, st.saved, st.pose)
        ref = oracle_mod.OracleRobot(N)
        ref.set_state(*ens.download_state(0))        # the GPU's rounded start state
        run = {"gpu": [], "ref": [], "dbg": [], "groups": [], "group_start_saved": []}
        for k, (enc, ln) in enumerate(scans):
            if k % T == 0:
                run["group_start_saved"].append(ref.savedLineCount)
            r = ens.localize(enc, ln[None], [len(ln)])[0]
            m = ref.localize(ln, enc[0])
            run["gpu"].append((r["match"], r["matches"], r["new_landmarks"], r["status"]))
            run["ref"].append((m, sum(x >= 0 for x in m), sum(x < 0 for x in m), ref.status))
            ens.read_results()   # (the full record: a synchronous call mirrors only ekf_result's words)
            run["dbg"].append(int(ens.result_words(0)[9]))
            if (k + 1) % T == 0:                     # the flush has run
                P, y, saved, pose = ens.download_state(0)
                run["groups"].append({"scan": k + 1, "P": float(rel(P, ref.P_t0)), "y": float(rel(y, ref.y)),
                                      "pose": float(np.abs(pose - ref.pose).max()),
                                      "saved": (saved, ref.savedLineCount),
                                      "bits": (digest(P), digest(y), digest(pose), saved)})
                ref.set_state(P, y, saved, pose)     # the next group from identical inputs
                del P
        ens.close()
        out[mode] = run
    _RUNS[case] = out
    return out


def restarts(run, T):
    """Per restarting scan (RES_DBG bit 8): (scan index, pending steps, exact form, an earlier step
    of its group added landmarks, it matched a landmark added earlier in its group)."""
    rows = []
    for k, dw in enumerate(run["dbg"]):
        if not dw & 8:
            continue
        g0 = k - k % T
        added = any(run["ref"][q][2] > 0 for q in range(g0, k))
        in_group = any(x >= run["group_start_saved"][k // T] for x in run["ref"][k][0])
        rows.append((k, k % T, bool(dw & 64), added, in_group))
    return rows


def summary(case, runs):
    T = case[4]
    out = {}
    for mode, run in runs.items():
        rs = restarts(run, T)
        out[str(mode)] = {
            "P_group": max(g["P"] for g in run["groups"]), "y_group": max(g["y"] for g in run["groups"]),
            "pose_group": max(g["pose"] for g in run["groups"]),
            "bits": {str(b): sum(1 for dw in run["dbg"] if dw & b) for b in (8, 512, 16, 64, 128, 256)},
            "restarts_pending_mfma": sum(1 for r in rs if r[1] > 0 and not r[2]),
            "restarts_after_added": sum(1 for r in rs if r[3]),
            "restarts_matching_group_added": sum(1 for r in rs if r[4]),
        }
    return out


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_modes_against_oracle(ekf_mod, oracle_mod, case):
    """Modes 0..3 of one split-arithmetic context against the restatement per flush group, the
    results equal across the modes, and proof from the path words that the failed-verdict restart
    (on MFMA-replay contexts: its Dd seed with pending steps, after steps that added landmarks)
    ran. Bars and their origin: module docstring."""
    arith, prec, rep, N, T, nt = case
    runs = collect(ekf_mod, oracle_mod, case)
    summ = summary(case, runs)
    record(case_id(case), summ)
    print(case_id(case), json.dumps(summ))
    for mode in MODES:
        run = runs[mode]
        for k in range(SCANS):
            assert run["ref"][k][3] == 0, ("restatement status", mode, k)
            assert run["gpu"][k] == run["ref"][k], (mode, k, run["gpu"][k], run["ref"][k])
        assert len(run["groups"]) == SCANS // T
        for g in run["groups"]:
            assert g["P"] <= P_TOL[prec], (mode, g["scan"], "P", g["P"])
            assert g["y"] <= Y_TOL, (mode, g["scan"], "y", g["y"])
            assert g["saved"][0] == g["saved"][1], (mode, g["scan"], g["saved"])
            assert g["pose"] <= POSE_ATOL, (mode, g["scan"], "pose", g["pose"])
        assert run["gpu"] == runs[0]["gpu"], mode
    # the path under test ran (the counts test_speculative_association_identical asserts on these scans)
    bits = {mode: summ[str(mode)]["bits"] for mode in MODES}
    assert bits[1]["8"] == 0, "speculation fell back on ordinary scans"
    assert bits[2]["8"] >= 4, "wrong guesses did not fall back"
    assert bits[3]["8"] >= 2 and bits[3]["512"] >= 1, "wrong late guesses did not keep the lines before them"
    if rep != 0:
        for mode in (2, 3):
            assert summ[str(mode)]["restarts_pending_mfma"] >= 1, (mode, "no restart on the MFMA replay with pending steps")
            assert summ[str(mode)]["restarts_after_added"] >= 1, (mode, "no restart after a step that added landmarks")
        if (N, T) == (64, 8):
            assert summ["2"]["restarts_matching_group_added"] >= 1, "no restart matched a landmark added in its group"
    else:
        # the per-element replay: an exact form on every scan with pending steps
        for mode in MODES:
            assert bits[mode]["64"] == SCANS - SCANS // T, (mode, bits[mode])


def same_bits(a, b, what):
    """P, y, pose and saved of two runs equal bit for bit at every group end, results equal."""
    for ga, gb in zip(a["groups"], b["groups"]):
        for name, xa, xb in zip(("P", "y", "pose", "saved"), ga["bits"], gb["bits"]):
            assert xa == xb, (what, "group ending at scan", ga["scan"], name, "differs; group errors vs the"
                              " restatement", ga["P"], gb["P"])
    assert a["gpu"] == b["gpu"], what


@pytest.mark.parametrize("arith", [BF16X6, F16X3])
def test_per_element_replay_modes_bit_identical(ekf_mod, oracle_mod, arith):
    """EKF_OPT_MFMA_REPLAY = 0 on a split arithmetic: the speculative pass's staged replay is per
    element the chain of pll_blocks (staged_blocks' comment, ekf_kernels.hip), which is what mode 0
    and the restart's uncached columns read, and the flush (the split products) sees the same
    operands in every mode: P, y, pose and saved equal bit for bit at every group end in modes
    0..3. With the MFMA replay they are not (module docstring)."""
    runs = collect(ekf_mod, oracle_mod, (arith, 1, 0, 256, 8, 0))
    for mode in (1, 2, 3):
        same_bits(runs[mode], runs[0], ("mode", mode, "vs 0"))


WIDTH_PAIRS = [(c, c[:5] + (narrow,)) for c in CASES if c[5] == 192
               for narrow in ([64] if c[3] == 256 else [128])]


@pytest.mark.parametrize("wide,narrow", WIDTH_PAIRS, ids=lambda c: case_id(c))
def test_scan_width_bit_identical(ekf_mod, oracle_mod, wide, narrow):
    """EKF_OPT_SCAN_THREADS on MFMA-replay contexts: 64 (N = 256) and 128 (N = 1000, partial last
    workgroup) landmarks per workgroup against 192, bit for bit within every mode — the restarts of
    modes 2 and 3 included, which test_narrow_scan_workgroups_identical does not reach in mode 3."""
    assert narrow in CASES
    a = collect(ekf_mod, oracle_mod, narrow)
    b = collect(ekf_mod, oracle_mod, wide)
    for mode in MODES:
        same_bits(a[mode], b[mode], ("mode", mode, "width", narrow[5], "vs 192"))


# ---- status bits of kept and re-run lines ------------------------------------------------------

SING_N, SING_S, SING_Z = 16, 10, 8
# which landmark each of the 8 lines observes. Landmark 8 has a zero covariance and the lines an
# exact R = 0: its S is singular, GSL_EDOM leaves S⁻¹ = 0 (Robot.cpp:449-457), its distance is 0 and
# it wins the first line that evaluates it — the line observing landmark 9, whose candidates are
# the unmatched landmarks 0..9 in order
SING_SCANS = {
    "kept": [0, 1, 9, 2, 3, 4, 5, 6],      # evaluated by line 2: a kept line of mode 3's restart
    "rerun": [0, 1, 2, 3, 9, 4, 5, 6],     # only by line 4: speculative under a wrong guess, then re-run
    "never": [3, 0, 5, 1, 7, 2, 6, 4],     # every winner below it: never evaluated
}


@pytest.mark.parametrize("arith,prec", [(0, 0), (0, 1), (BF16X6, 1), (F16X3, 1)])
@pytest.mark.parametrize("scan", list(SING_SCANS))
def test_singular_status_of_kept_and_rerun_lines(ekf_mod, oracle_mod, arith, prec, scan):
    """test_singular_status_counts_only_evaluated_candidates on an 8-line scan (mode 3 needs more
    than 3 lines): the restart after a failed verdict takes the kept lines' status from the packed
    per-line words (st_lines(stp, first) | st_lines(rwp, first)) and drops those of the lines it
    re-runs. Ten well-separated landmarks with independent covariances (the robot block is zero, so
    a candidate's S is its own block), landmark 8 singular. EKF_ST_SINGULAR_S must equal the
    restatement's GSL_EDOM bit, the association its list, and the four modes each other: a flag
    leaking from a discarded speculative line, or lost from a kept one, fails here. (The scan ends
    in the reference's map reset, saved > N − 10, in the restatement and the library alike.)"""
    N, s, Z = SING_N, SING_S, SING_Z
    n = 3 + 2 * N
    P = np.zeros((n, n))
    y = np.zeros(n)
    for j in range(s):
        y[3 + 2 * j], y[4 + 2 * j] = -2.5 + 0.5 * j, 1.0 + 0.3 * j
        if j != Z:
            P[3 + 2 * j, 3 + 2 * j], P[4 + 2 * j, 4 + 2 * j] = 0.01, 0.02
    lines = np.array([[y[3 + 2 * j], y[4 + 2 * j], 0.0, 0.0, 0.0, 0.0] for j in SING_SCANS[scan]])
    want_match = [Z if j == 9 else j for j in SING_SCANS[scan]]
    want_sing = 0 if scan == "never" else 1
    got = {}
    for mode in MODES:
        ens = ekf_mod.Ensemble(N, 1, prec, max_lines=8, arith=arith, options={"speculate": mode})
        ens.upload_state(0, P, y, s, [0.0, 0.0, 0.0])
        ref = oracle_mod.OracleRobot(N)
        ref.set_state(*ens.download_state(0))
        res = ens.localize([0.0, 0.0, 0.0], lines[None], [8])[0]
        m = ref.localize(lines, [0.0, 0.0, 0.0])
        ens.read_results()
        dw = int(ens.result_words(0)[9])
        ens.close()
        assert m == want_match and ref.status & 1 == want_sing, (m, ref.status)   # (the scan is what it says)
        assert res["match"] == m, (mode, res["match"], m)
        assert res["status"] & ekf_mod.ST_SINGULAR_S == ref.status & 1, (mode, scan, res["status"])
        got[mode] = (res["match"], res["matches"], res["new_landmarks"], res["status"], res["saved"], res["reset"])
        # the modes ran what they are meant to: no failed verdict in mode 1, one in 2 and 3, lines
        # kept in mode 3 (first = 4: line 4's guess is line 5's winner)
        assert bool(dw & 8) == (mode >= 2), (mode, dw)
        assert bool(dw & 512) == (mode == 3), (mode, dw)
        if mode == 3:
            assert (dw >> 10) & 7 == 4, (mode, dw)
    for mode in (1, 2, 3):
        assert got[mode] == got[0], (mode, got[mode], got[0])
