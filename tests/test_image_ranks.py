"""An ensemble sharded over two ranks resamples as one (dist.resample_global): two gloo
ranks on the one GPU of the test box, 2 + 2 instances fed by lineage, call resample_global part way
through a flush group with weights that force a transfer between the ranks and a local copy. One
context of 4 instances on the same scans calls Ensemble.resample with the concatenated plan. Every
later result and the final dense states are equal bit for bit. Three processes use the GPU: this one
and the two ranks, each rank under its own time limit."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from slam_ros_amd import scan_gen as G
from slam_ros_amd.dist import global_resample_plan
from tests.test_image import feed_pairs, init

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
WEIGHTS, U = [0.8, 0.0, 0.2, 0.0], 0.5       # copies 3, 0, 1, 0: instance 0 fills slot 1 and, on rank 1, slot 3


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("prec,pipeline,T,arith", [(1, 0, 4, 2), (0, 1, 4, 0)])
def test_two_ranks_resample_as_one_context(ekf_mod, tmp_path, prec, pipeline, T, arith):
    N, n, at, more = 64, 2, 6, 6
    local, transfers = global_resample_plan(WEIGHTS, U, [n, n])
    assert transfers == [(0, 0, 1, 1)] and local == [[0, 0], [0, 1]]
    src = [r * n + s for r in range(2) for s in local[r]]
    for sr, se, dr, de in transfers:
        src[dr * n + de] = sr * n + se
    assert src == [0, 0, 2, 0]
    port = free_port()
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "image_ranks_worker.py"), "--out",
                               str(tmp_path), "--rank", str(r), "--world", "2", "--port", str(port), "--N", str(N),
                               "--T", str(T), "--precision", str(prec), "--arith", str(arith), "--pipeline",
                               str(pipeline), "--at", str(at), "--more", str(more), "--weights",
                               ",".join(str(x) for x in WEIGHTS), "--u", str(U)],
                              cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]
    # the single context, while the ranks run
    w = G.make_world(N, active=N - 14)
    st = G.initial_state(w)
    one = ekf_mod.Ensemble(N, 2 * n, prec, max_lines=8, flush_interval=T, arith=arith, pipeline=bool(pipeline))
    for e in range(2 * n):
        init(one, e, e, st)
    for i in range(1, at + 1):
        one.localize(*feed_pairs(w, [(e, i) for e in range(2 * n)]))
    one.resample(src)
    rows = []
    for i in range(at + 1, at + more + 1):
        res = one.localize(*feed_pairs(w, [(l, i) for l in src]))
        rows.append([list(r["pose"]) + [r["matches"], r["new_landmarks"], r["saved"], r["status"], r["reset"]]
                     + list(r["match"]) + [-2] * (8 - len(r["match"])) for r in res])
    rows = np.array(rows, dtype=np.float64)
    states = [one.download_state(e) for e in range(2 * n)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=100))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, p in enumerate(procs):
        assert p.returncode == 0, (r, outs[r][1][-3000:])
    assert rows[:, :, 3].sum() > 0 and rows[:, :, 4].sum() > 0      # matches and new landmarks after the call
    for r in range(2):
        d = np.load(tmp_path / f"rank{r}.npz")
        assert [tuple(t) for t in d["transfers"]] == transfers
        assert list(d["lin"]) == src[r * n: (r + 1) * n]
        assert np.array_equal(d["res"], rows[:, r * n: (r + 1) * n], equal_nan=True), r
        for e in range(n):
            P, y, saved, pose = states[r * n + e]
            assert np.array_equal(d["P"][e], P, equal_nan=True), (r, e, np.argwhere(d["P"][e] != P)[:8].tolist())
            assert np.array_equal(d["y"][e], y) and np.array_equal(d["pose"][e], pose) and int(d["saved"][e]) == saved
