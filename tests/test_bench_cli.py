"""bench.py's command line: a plain run does the timed steps only, --full adds the legs that take
runs of their own, --dump-outputs writes what the last timed step left. Small shapes (N = 256, two
instances, 7 timed steps: a flush group of 4 and a partial one flushed by ekf_sync)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = ["--gpus", "1", "--steps", "7", "--warmup", "2", "--preroll", "0", "--capacity", "256",
          "--instances", "2", "--flush-interval", "4"]
N_STATE = 3 + 2 * 256


def run_bench(extra):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + COMMON + extra,
                         cwd=ROOT, capture_output=True, text=True, timeout=150)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_options_parse(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs == "" and a.steps == 3
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d", "--force-collective", "--no-cpu"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"
    # the parity leg cannot follow the forced collective (its receive groups are retired)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--force-collective"])
    with pytest.raises(SystemExit):
        bench.parse()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--force-collective"])   # a plain run has no parity leg
    assert bench.parse().full is False


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    """One plain run with its dump and final state, shared by the tests below."""
    d = tmp_path_factory.mktemp("plain")
    r = run_bench(["--dump-outputs", str(d / "a"), "--dump-state", str(d / "state")])
    return r, d / "a", d / "state"


@pytest.mark.gpu
def test_plain_run_and_dump_outputs(tmp_path, plain):
    """A plain run: the headline fields, none of the --full legs; its dump is float64
    .npy files within 64 MB, identical from run to run, and equal to the final state that
    --dump-state writes (after a plain run nothing follows the timed steps)."""
    r, a, st = plain
    b = tmp_path / "b"
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in r, key
    assert r["steps"] == 7 and r["warmup"] == 2 and r["all_lines_matched"] is True
    assert r["ms_per_step"] > 0 and abs(r["value"] * r["ms_per_step"] * 1e-3 - 2) < 1e-9   # 2 instances per step
    assert r["cpu_baseline"] is None and "parity" not in r and r["kernel_ms"]["scan"] is None
    # every timed step is in a timed flush: --steps sets their number
    assert sum(f["steps_per_launch"] * f["launches"] for f in r["roofline"]["launch_forms"]) == 7
    run_bench(["--dump-outputs", str(b)])
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and all(n.endswith(".npy") for n in names)
    assert sum(os.path.getsize(a / n) for n in names) <= 64e6
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype in (np.float32, np.float64), (n, x.dtype)
        assert np.array_equal(x, y), n
    rows = np.load(a / "P_row_index.npy").astype(int)
    assert len(rows) == N_STATE                      # the whole of P fits at this size
    P, yv, match = np.load(a / "P_rows.npy"), np.load(a / "y.npy"), np.load(a / "match.npy")
    assert P.shape == (2, N_STATE, N_STATE) and P.dtype == np.float64 and match.shape == (2, 8)
    assert (match >= 0).all() and (np.load(a / "result_counts.npy")[:, 0] == 8).all()
    for e in range(2):
        s = np.load(st / f"state_{e}.npz")
        assert np.array_equal(P[e], s["P"][rows]) and np.array_equal(yv[e], s["y"])
        assert np.array_equal(np.load(a / "P_diag.npy")[e], np.diagonal(s["P"]))
        assert np.array_equal(np.load(a / "pose.npy")[e], s["pose"])
        assert np.load(a / "saved.npy")[e] == int(s["saved"]) == 246


@pytest.mark.gpu
def test_full_run_keeps_its_legs(tmp_path, plain):
    """--full: the association timing, the parity leg (within its bar) and the CPU baseline are in
    the line, and the timed steps leave the same outputs as a plain run's."""
    a, b = tmp_path / "full", plain[1]
    r = run_bench(["--full", "--cpu-seconds", "0.2", "--dump-outputs", str(a)])
    assert r["kernel_ms"]["scan"] > 0
    assert r["parity"]["within_bar"] is True and r["parity"]["association_identical"] is True
    assert r["cpu_baseline"]["value"] > 0 and r["speedup_vs_cpu_baseline"] > 0
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) and "P_rows.npy" in os.listdir(a)
    for n in sorted(os.listdir(a)):
        assert np.array_equal(np.load(a / n), np.load(b / n)), n
