"""One instance with its landmark block partitioned over two ranks on the product kernels
(DESIGN.md §7): two gloo ranks on the one GPU of the test box, each a partitioned
context (ekf_shard_create) storing its share of the packed tiles, against a single context of the
same library on the same scans. Exact arithmetic: every association, the robot rows, the mean, the
pose and savedLineCount on every rank, and the landmark block — the sum of the ranks' tiles — are
bit-identical, augmentation and the capacity reset included; each rank stores at most 0.55 of the
single context's landmark-block bytes. The per-scan wall time of the two-rank run is recorded.
Both protocols (slam_ekf.h): the speculative one (one exchange of every guessed column, the lines
in one workgroup up to the first wrong guess; the default) and the per-line one (one exchange per
line), with scans whose line 1 repeats line 0, and with every guess wrong (EKF_OPT_SPECULATE = 2:
the run stops at the first line whose winner is not landmark 0 and the per-line protocol finishes
the scan from the state after the lines before it)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from slam_ros_amd import scan_gen as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("prec,N,T,scans,active,extra_every,dup,mode",
                         [(1, 1024, 4, 9, 0, 0, 0, "spec"), (1, 1000, 6, 8, 0, 0, 3, "spec"), (0, 512, 4, 6, 0, 0, 2, "spec"),
                          (1, 1024, 4, 9, 1000, 3, 0, "spec"), (1, 256, 4, 6, 0, 3, 0, "spec"),
                          (0, 480, 4, 7, 400, 2, 3, "wrong"), (1, 1024, 4, 9, 1000, 3, 2, "wrong"),
                          (1, 1024, 4, 9, 1000, 3, 2, "perline"), (0, 512, 4, 6, 0, 0, 0, "perline")])
def test_two_rank_shard_equals_single_context(ekf_mod, oracle_mod, tmp_path, prec, N, T, scans, active, extra_every,
                                              dup, mode):
    """(active, extra_every): every extra_every-th scan carries two unmatched lines — augmented
    landmarks landing on either rank, and (active = N − 10) the capacity reset; dup: line 1 repeats
    line 0 every dup-th scan; mode: the speculative protocol, the same with every guess wrong, or
    the per-line protocol only."""
    run_sharded(ekf_mod, oracle_mod, tmp_path, prec, N, T, scans, active, extra_every, world=2, backend="gloo",
                dup=dup, mode=mode)


@pytest.mark.parametrize("prec,N,T,scans,active,extra_every,dup,mode",
                         [(1, 1024, 4, 9, 1000, 3, 3, "spec"), (0, 512, 4, 6, 0, 0, 0, "wrong"),
                          (1, 1024, 4, 9, 1000, 3, 0, "perline"),
                          (1, 1024, 4, 9, 1000, 3, 3, "native"), (0, 480, 4, 7, 400, 2, 3, "native-wrong"),
                          (1, 512, 4, 6, 0, 0, 2, "native-perline"), (1, 4096, 4, 6, 0, 0, 0, "native"),
                          (1, 8500, 4, 4, 0, 0, 2, "native"), (1, 8500, 4, 3, 0, 0, 0, "native-wrong")])
def test_rccl_device_sum_world1(ekf_mod, oracle_mod, tmp_path, prec, N, T, scans, active, extra_every, dup, mode):
    """The nccl (RCCL) backend's path: the exchange buffers all-reduced in place on the device, on
    the context's stream, with no host staging. One GPU holds one RCCL rank, so this runs a world of
    one (the partition is the whole block); the two-rank protocol itself is covered over gloo.
    native*: the whole scan as one library call (ekf_shard_localize) on the library's own RCCL
    communicator (ekf_shard_attach_rccl), every protocol variant; N = 8500 puts two landmarks on
    each of the run's threads (shard_spec_kernel with K = 2)."""
    run_sharded(ekf_mod, oracle_mod, tmp_path, prec, N, T, scans, active, extra_every, world=1, backend="nccl",
                dup=dup, mode=mode)


def rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def run_sharded(ekf_mod, oracle_mod, tmp_path, prec, N, T, scans, active, extra_every, world, backend, dup=0,
                mode="spec"):
    w = G.make_world(N, active=active or N - 10)
    st = G.initial_state(w)
    one = ekf_mod.Ensemble(N, 1, prec, max_lines=8, flush_interval=T)
    one.init_lowrank(0, st.diag, st.U, st.y, st.saved, st.pose)
    # the restatement (oracle/, fp64) from the same storage-rounded start, on the same scans, never
    # re-synchronised: the partitioned instance is checked against it directly (below)
    ref = oracle_mod.OracleRobot(N, mode=oracle_mod.FAST)
    ref.set_state(*one.download_state(0))
    ref_matches, resets, added = [], 0, 0
    rng = np.random.default_rng(11)
    for step in range(1, scans + 1):
        enc, lines, nl = G.make_scan(w, step, instances=1, lines=6 if extra_every else 8)
        ln = lines[0, :nl[0]]
        if extra_every and step % extra_every == 0:
            ln = np.concatenate([ln, G.random_lines(rng, 2)])
        if dup and step % dup == 0:
            ln = ln.copy()
            ln[1] = ln[0]
        la = np.zeros((1, 8, 6))
        la[0, :len(ln)] = ln
        r = one.localize(enc, la, np.array([len(ln)], dtype=np.int32))
        ref_matches.append(list(r[0]["match"][:len(ln)]) + [-2] * (8 - len(ln)))
        assert ref.localize(ln, enc[0]) == list(r[0]["match"][:len(ln)]), step
        resets += r[0]["reset"]
        added += r[0]["new_landmarks"]
    P, y, saved, pose = one.download_state(0)
    block_bytes = one.landmark_block_bytes()
    one.close()
    if extra_every:
        assert added > 0 or resets > 0
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.join(ROOT, "tests", "rowshard_gpu_worker.py"), "--out", str(tmp_path), "--N", str(N),
           "--T", str(T), "--scans", str(scans), "--precision", str(prec), "--active", str(active),
           "--extra-every", str(extra_every), "--backend", backend, "--dup-every", str(dup)] + \
        {"spec": [], "wrong": ["--wrong-guess"], "perline": ["--per-line"], "native": ["--native"],
         "native-wrong": ["--native", "--wrong-guess"], "native-perline": ["--native", "--per-line"]}[mode]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=110)
    assert out.returncode == 0, out.stderr[-3000:]
    Psum = np.zeros_like(P)
    rows = []
    for r in range(world):
        d = np.load(tmp_path / f"rank{r}.npz")
        assert [list(m) for m in d["matches"]] == ref_matches, r
        np.testing.assert_array_equal(d["P"][:3, :], P[:3, :])      # robot rows: replicated
        np.testing.assert_array_equal(d["y"], y)
        np.testing.assert_array_equal(d["pose"], pose)
        assert int(d["saved"]) == saved
        Psum[3:, 3:] += d["P"][3:, 3:]                                 # the rank's tiles, zero elsewhere
        rows.append(tuple(d["tile_rows"]))
        # ≈1/2 of the packed block per rank; partition boundaries fall on even tile rows, coarse for
        # a small block (N = 256: 16 tile rows)
        if world == 2:
            assert int(d["block_bytes"]) <= (0.55 if N >= 1000 else 0.65) * block_bytes, (r, int(d["block_bytes"]), block_bytes)
        times = d["times"]
        spec_runs = [int(x) for x in d["spec_runs"]]
    if mode == "perline" or mode.startswith("native"):
        assert spec_runs == []   # (the native call does not report its stopping lines)
    else:
        assert len(spec_runs) == scans
        if mode == "wrong":   # guesses of landmark 0: the runs stop early
            assert sum(x < 8 - (extra_every > 0) * 2 for x in spec_runs) >= scans // 2, spec_runs
    np.testing.assert_array_equal(Psum[3:, 3:], P[3:, 3:])
    # the assembled partitioned state against the restatement: a trajectory of `scans` updates
    # never re-synced, so k times the per-scan bar (tests/test_bench_config.py) on P; the state
    # vector within 1e-8 per scan as well
    Pshard = Psum.copy()
    Pshard[:3, :] = d["P"][:3, :]
    Pshard[3:, :3] = d["P"][3:, :3]
    bar = 1e-10 if prec == 0 else 1e-6
    rp, ry = rel(Pshard, ref.P_t0), rel(d["y"], ref.y)
    assert rp <= scans * bar, (rp, scans * bar)
    assert ry <= scans * 1e-8, ry
    assert int(d["saved"]) == ref.savedLineCount
    assert rows[0][0] == 0 and rows[-1][1] == (2 * N + 31) // 32
    assert all(rows[r][1] == rows[r + 1][0] for r in range(world - 1))
    from tests.test_bench_config import record
    record(f"rowshard_{backend}{world}_N{N}_T{T}_p{prec}_{mode}_d{dup}",
           {"scan_ms_median": float(np.median(times)) * 1e3, "spec_runs": spec_runs,
                                            "tile_rows": [[int(a), int(b)] for a, b in rows],
                                            "block_bytes_single": int(block_bytes),
                                            "p_rel_err_vs_oracle": rp, "y_rel_err_vs_oracle": ry})


def test_one_call_scan_in_process(ekf_mod, oracle_mod):
    """ekf_shard_localize straight through the C-ABI, without torch.distributed: its argument
    checks (no communicator attached: EKF_EINVAL; a rank or world other than the context's:
    EKF_EINVAL; more lines than the context takes: EKF_ERANGE), then a world of one attached to
    the library's own RCCL communicator, its scans against one context of the same library
    (bit-identical state and associations) and the restatement (associations). The partitioned
    context is drained after scan 5, so it flushes groups of 4, 1 and 1 steps: an odd group runs the
    wave kernel on one step more (a step that applies nothing), and flush_kernel_name says so."""
    import ctypes
    N, T, scans = 512, 4, 6
    lib = ekf_mod.load_library()
    w = G.make_world(N)
    st = G.initial_state(w)
    one = ekf_mod.Ensemble(N, 1, 1, max_lines=8, flush_interval=T)
    sh = ekf_mod.Ensemble(N, 1, 1, max_lines=8, flush_interval=T, shard=(0, 1))
    for ens in (one, sh):
        ens.init_lowrank(0, st.diag, st.U, st.y, st.saved, st.pose)
    ref = oracle_mod.OracleRobot(N, mode=oracle_mod.FAST)
    ref.set_state(*one.download_state(0))
    res = (ekf_mod.EkfResult * 1)()
    enc0 = np.zeros(3)
    ln0 = np.zeros((8, 6))
    dp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.ekf_shard_localize(sh.handle, dp(enc0), dp(ln0), 1, ctypes.byref(res)) == 1   # no communicator
    assert lib.ekf_shard_localize(one.handle, dp(enc0), dp(ln0), 1, ctypes.byref(res)) == 1  # not partitioned
    uid = (ctypes.c_ubyte * 128)()
    assert lib.ekf_rccl_unique_id(uid) == 0
    assert lib.ekf_shard_attach_rccl(sh.handle, uid, 1, 1) == 1   # rank outside the context's world
    assert lib.ekf_shard_attach_rccl(sh.handle, uid, 0, 2) == 1   # not the context's world
    assert lib.ekf_shard_attach_rccl(sh.handle, uid, 0, 1) == 0
    sh.profile(1)
    big = np.zeros((9, 6))
    assert lib.ekf_shard_localize(sh.handle, dp(enc0), dp(big), 9, ctypes.byref(res)) == 4   # ERANGE
    for step in range(1, scans + 1):
        enc, lines, nl = G.make_scan(w, step, instances=1, lines=8)
        ln = np.ascontiguousarray(lines[0, :nl[0]])
        r1 = one.localize(enc, lines, nl)[0]
        e = np.ascontiguousarray(enc[0])
        assert lib.ekf_shard_localize(sh.handle, dp(e), dp(ln), len(ln), ctypes.byref(res)) == 0
        m = list(res[0].match[: res[0].nlines])
        assert m == list(r1["match"][: len(ln)]), step
        assert ref.localize(ln, enc[0]) == m, step
        if step == 5:
            sh.sync()
    P1, y1, s1, p1 = one.download_state(0)
    P2, y2, s2, p2 = sh.download_state(0)
    assert [n for n, _ in sh.profile_flushes()] == [4, 1, 1]
    assert sh.flush_kernel_name(1) == "flush_f32_wave_kernel<float, 2>"
    assert sh.flush_kernel_name(3) == "flush_f32_wave_kernel<float, 4>"
    assert sh.flush_kernel_name(4) == "flush_f32_wave_kernel<float, 4>"
    np.testing.assert_array_equal(P2, P1)
    np.testing.assert_array_equal(y2, y1)
    assert s1 == s2
    one.close()
    sh.close()
