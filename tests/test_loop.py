"""The ensemble's hypothesis loop on the device (slam_ekf.h ekf_gate_candidates_device,
ekf_assoc_weights_device, ekf_resample_plan_device, ekf_resample_device): each stage against its host
form, and the whole chain (gate -> candidates -> joint search -> weights -> plan -> copy) enqueued with no
host read in between against a twin context driven stage by stage on the host.

The copy is tested by the twin scheme of tests/test_resample.py with the list uploaded and the call made
through ekf_resample_device: context `a` runs instances with histories of their own and copies part way
through a flush group, context `b` was set up and fed as the sources from the start and never copies, and
everything `a` returns must equal `b` bit for bit. (The CPU parts are in tests/test_loop_plan.py.)
"""
import ctypes

import numpy as np
import pytest

from slam_ros_amd import scan_gen as G
from tests.hipmem import DeviceArray, hip
from tests.test_associate_joint import CONFIDENCE, GATE_LOOSE, hit_bits
from tests.test_gate import make, shared_scans, shared_world
from tests.test_loop_plan import FIXTURES, INF, RP_INVALID, RP_KEPT, sequential_plan
from tests.test_resample import (FOLLOW, Twin, assert_reads_equal, assert_results_equal, feed, lineage_scan, run_twin,
                                 same)

EINVAL, ERANGE = 1, 4
AS_INVALID, AS_TRUNCATED = 4, 1
LOG_2PI = float(np.log(2.0 * np.pi))


def wait():
    """Everything enqueued so far has run (no drain: ekf_sync would flush the open group)."""
    assert hip().hipDeviceSynchronize() == 0


def junk(nbytes):
    return DeviceArray(np.full(nbytes, 0x5a, dtype=np.uint8))


def fetch(dev, dtype, shape):
    out = np.zeros(shape, dtype=dtype)
    assert out.nbytes <= dev.nbytes
    assert hip().hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), dev.ptr, out.nbytes, 2) == 0
    return out


def fetch_struct(dev, ctype, count):
    raw = (ctype * count)()
    assert hip().hipMemcpy(ctypes.byref(raw), dev.ptr, ctypes.sizeof(raw), 2) == 0
    return raw


# ---------------------------------------------------------------------------------------------
# stage 1: the candidates
# ---------------------------------------------------------------------------------------------
def device_candidates(a, d2, nlines, C, gate):
    """ekf_gate_candidates_device on a host matrix [E, ML, N]: (cand [E, ML, C], count [E, ML])."""
    E, ML, _ = d2.shape
    bufs = [DeviceArray(d2), DeviceArray(np.asarray(nlines, dtype=np.int32)), junk(4 * E * ML * C), junk(4 * E * ML)]
    a.gate_candidates_device(bufs[0].address, bufs[1].address, C, gate, bufs[2].address, bufs[3].address)
    wait()
    cand, count = fetch(bufs[2], np.int32, (E, ML, C)), fetch(bufs[3], np.int32, (E, ML))
    a.gate_candidates_device(bufs[0].address, bufs[1].address, C, gate, bufs[2].address, 0)   # count may be NULL
    wait()
    assert np.array_equal(fetch(bufs[2], np.int32, (E, ML, C)), cand)
    for b in bufs:
        b.close()
    return cand, count


def expected_candidates(ekf_mod, d2, nlines, C, gate):
    E, ML, _ = d2.shape
    cand = np.full((E, ML, C), -1, dtype=np.int32)
    count = np.zeros((E, ML), dtype=np.int32)
    for e in range(E):
        n = int(nlines[e])
        if n > 0:
            cand[e, :n] = ekf_mod.gate_candidates(d2[e, :n], C, gate)
            count[e, :n] = np.count_nonzero(np.sqrt(np.abs(d2[e, :n])) <= gate, axis=1)
    return cand, count


def synthetic_matrix(gate):
    """E = 3, max_lines = 8, N = 300 (no multiple of 64 or 256); nlines = (8, 0, 3)."""
    E, ML, N = 3, 8, 300
    rng = np.random.default_rng(41)
    inside = gate * gate
    d2 = np.full((E, ML, N), np.inf)
    d2[:, :, 250:] = np.nan                                   # tails: NaN, then +inf
    d2[:, :, 280:] = np.inf
    r = d2[0]
    r[0, :200] = 1.0 + rng.random(200)                         # row 0: nothing inside the gate
    for row, n in ((1, 1), (2, 3), (3, 8)):                    # rows 1-3: exactly 1, 3, 8 inside
        r[row, :250] = 1.0 + rng.random(250)
        r[row, rng.choice(300, n, replace=False)] = inside * rng.random(n)
    r[4, :250] = 1.0 + rng.random(250)                         # row 4: 40 inside, in every wave of 64
    js = 3 + 7 * np.arange(40)
    assert js.max() < N and set(js // 64) == {0, 1, 2, 3, 4}
    r[4, js] = inside * rng.random(40) * rng.choice([-1.0, 1.0], 40)
    x = 0.25 * inside                                          # row 5: ties (lower landmark first), -x / +x
    r[5, [7, 71, 263]] = x
    r[5, 100], r[5, 40] = -0.5 * x, 0.5 * x
    r[5, 299], r[5, 0] = 0.75 * x, -0.75 * x
    v = inside                                                 # row 6: sqrt(v) == gate exactly, and the next double
    while np.sqrt(v) > gate:
        v = np.nextafter(v, 0.0)
    while np.sqrt(np.nextafter(v, 1.0)) <= gate:
        v = np.nextafter(v, 1.0)
    assert np.sqrt(v) == gate and np.sqrt(np.nextafter(v, 1.0)) > gate
    r[6, 10], r[6, 11], r[6, 12], r[6, 13] = v, np.nextafter(v, 1.0), -v, -np.nextafter(v, 1.0)
    r[7, 5], r[7, 2], r[7, 270] = -0.0, 0.0, 0.5 * inside      # row 7: zeros of both signs, a member past the NaNs
    r[7, 6] = -np.inf
    d2[1, :, :200] = inside * rng.random((ML, 200))            # nlines 0: members everywhere, never read
    d2[2, :, :200] = 4.0 * inside * rng.random((ML, 200))      # nlines 3: the rows past it are ignored
    return d2, np.array([8, 0, 3], dtype=np.int32)


@pytest.mark.gpu
def test_candidates_are_the_helpers(ekf_mod):
    gate = 0.4
    d2, nlines = synthetic_matrix(gate)
    a = ekf_mod.Ensemble(300, 3, 1, max_lines=8)
    for C in (1, 3, 8):
        cand, count = device_candidates(a, d2, nlines, C, gate)
        want, wcount = expected_candidates(ekf_mod, d2, nlines, C, gate)
        assert np.array_equal(cand, want), (C, np.argwhere(cand != want)[:8].tolist())
        assert np.array_equal(count, wcount), (C, count, wcount)
    assert wcount[0].tolist() == [0, 1, 3, 8, 40, 7, 2, 3] and wcount[1].tolist() == [0] * 8
    assert want[0, 5].tolist() == [40, 100, 0, 299, 7, 71, 263, -1]       # the ties, C = 8
    assert want[0, 6, :3].tolist() == [10, 12, -1] and want[0, 7, :4].tolist() == [2, 5, 270, -1]
    # errors, before any launch
    lib, h = ekf_mod.load_library(), a.handle
    p = ctypes.c_void_p(16)
    for C in (0, 9, -1):
        assert lib.ekf_gate_candidates_device(h, p, p, C, 0.4, p, None) == ERANGE
    for g in (-0.1, float("nan"), INF):
        assert lib.ekf_gate_candidates_device(h, p, p, 3, g, p, None) == EINVAL
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert lib.ekf_gate_candidates_device(h, args[0], args[1], 3, 0.4, args[2], None) == EINVAL


class Chain:
    """The device buffers of one context's loop and the six enqueues."""

    def __init__(self, ekf_mod, ens, N, ML, C):
        self.mod, self.ens, self.E, self.N, self.ML, self.C = ekf_mod, ens, ens.instances, N, ML, C
        E = self.E
        self.sizes = dict(enc=8 * E * 3, lines=48 * E * ML, nlines=4 * E, gate=ctypes.sizeof(ekf_mod.EkfGateHit) * E * ML,
                          d2=8 * E * ML * N, cand=4 * E * ML * C, count=4 * E * ML, bound=8 * (ML + 1),
                          hits=ctypes.sizeof(ekf_mod.EkfAssocHit) * E, weights=8 * E, src=4 * E,
                          info=ctypes.sizeof(ekf_mod.EkfPlanInfo), status=4)
        self.dev = {}

    def put(self, name, host):
        if name in self.dev:
            self.dev[name].close()
        self.dev[name] = DeviceArray(host)
        assert self.dev[name].nbytes == self.sizes[name], name
        return self.dev[name].address

    def adr(self, name):
        if name not in self.dev:
            self.dev[name] = junk(self.sizes[name])
        return self.dev[name].address

    def inputs(self, enc, ln, nl):
        self.put("enc", enc)
        self.put("lines", ln)
        self.put("nlines", np.asarray(nl, dtype=np.int32))
        self.put("bound", self.mod.chi2_bounds(self.ML, CONFIDENCE))

    def gate(self):
        self.ens.gate_lines_device(self.adr("enc"), self.adr("lines"), self.adr("nlines"), self.adr("gate"), self.adr("d2"))

    def candidates(self, gate):
        self.ens.gate_candidates_device(self.adr("d2"), self.adr("nlines"), self.C, gate, self.adr("cand"), self.adr("count"))

    def search(self):
        self.ens.associate_joint_device(self.adr("enc"), self.adr("lines"), self.adr("nlines"), self.adr("cand"), self.C,
                                        self.adr("bound"), self.adr("hits"))

    def weights(self, log_unassigned=0.0, logprior=None):
        d_prior = 0
        if logprior is not None:
            self.prior = DeviceArray(np.asarray(logprior, dtype=np.float64))
            d_prior = self.prior.address
        self.ens.assoc_weights_device(self.adr("hits"), self.adr("nlines"), self.adr("weights"), log_unassigned, d_prior)

    def plan(self, u, ess_below=INF, info=True):
        self.ens.resample_plan_device(self.adr("weights"), u, self.adr("src"), ess_below, self.adr("info") if info else 0)

    def copy(self):
        self.ens.resample_device(self.adr("src"), self.adr("status"))

    def get(self, name):
        E, ML = self.E, self.ML
        if name == "hits":
            return fetch_struct(self.dev[name], self.mod.EkfAssocHit, E)
        if name == "info":
            return fetch_struct(self.dev[name], self.mod.EkfPlanInfo, 1)[0]
        dtype, shape = dict(d2=(np.float64, (E, ML, self.N)), cand=(np.int32, (E, ML, self.C)), count=(np.int32, (E, ML)),
                            weights=(np.float64, (E,)), src=(np.int32, (E,)), status=(np.int32, (1,)))[name]
        return fetch(self.dev[name], dtype, shape)

    def close(self):
        for d in self.dev.values():
            d.close()


@pytest.mark.gpu
def test_candidates_of_the_gates_matrix(ekf_mod):
    """The real thing: ekf_gate_lines_device's matrix on the shared trajectory at N = 64 (finite distances up
    to savedLineCount, +inf past it), with the association's gate 0.4 and the loose gate 30."""
    N, E, ML, C = 64, 2, 8, 3
    w, st = shared_world()
    a = make(ekf_mod, N, E, 1, st, flush_interval=8)
    ch = Chain(ekf_mod, a, N, ML, C)
    inside = {0.4: 0, GATE_LOOSE: 0}
    for step, enc, ln, nl in shared_scans(w, E, steps=6):
        lines = np.zeros((E, ML, 6))
        lines[:, :ln.shape[1]] = ln
        ch.inputs(enc, lines, nl)
        ch.gate()
        for gate in inside:
            ch.candidates(gate)
            wait()
            d2 = ch.get("d2")
            want, wcount = expected_candidates(ekf_mod, d2, nl, C, gate)
            assert np.array_equal(ch.get("cand"), want), (step, gate)
            assert np.array_equal(ch.get("count"), wcount), (step, gate)
            inside[gate] += int(wcount.sum())
        a.localize(enc, ln, nl)
    assert inside[0.4] >= 10 and inside[GATE_LOOSE] > inside[0.4], inside
    ch.close()


# ---------------------------------------------------------------------------------------------
# stage 2: the weights
# ---------------------------------------------------------------------------------------------
def numpy_weights(hits, nlines, log_unassigned=0.0, logprior=None):
    E = len(nlines)
    lw = np.full(E, np.nan)
    for e in range(E):
        h = hits[e]
        v = -(h.d2 + h.logdet) / 2.0 - h.m * LOG_2PI
        if nlines[e] - h.m != 0:
            v += (int(nlines[e]) - h.m) * log_unassigned
        if logprior is not None:
            v += logprior[e]
        if not (h.status & AS_INVALID) and np.isfinite(v):
            lw[e] = v
    if np.all(np.isnan(lw)):
        return np.zeros(E)
    out = np.exp(lw - np.nanmax(lw))
    out[np.isnan(lw)] = 0.0
    return out


def assert_weights(got, ref):
    assert np.all(np.abs(got - ref) <= 1e-10 * ref + 1e-300), (got, ref)
    assert np.array_equal(got == 0.0, ref == 0.0)


@pytest.mark.gpu
def test_weights(ekf_mod):
    N, E, ML, C = 64, 6, 8, 3
    w, st = shared_world()
    a = ekf_mod.Ensemble(N, E, 1, max_lines=ML, flush_interval=8)
    for e in range(E):                                          # instances that differ: their weights do too
        a.init_lowrank(e, st.diag * (1.0 + 0.25 * e), st.U, st.y, st.saved, st.pose)
    ch = Chain(ekf_mod, a, N, ML, C)
    scans = list(shared_scans(w, E, steps=6))
    for step, enc, ln, nl in scans[:5]:
        a.localize(enc, ln, nl)
    step, enc, ln, nl = scans[5]                                # step 6: eight lines
    ch.inputs(enc, ln, nl)
    ch.gate()
    ch.candidates(GATE_LOOSE)
    ch.search()
    ch.weights()
    wait()
    hits = ch.get("hits")
    assert all(hits[e].m >= 1 and hits[e].status == 0 for e in range(E))
    got = ch.get("weights")
    assert_weights(got, numpy_weights(hits, nl))
    assert got.max() == 1.0
    prior = np.log(np.array([0.1, 0.2, 0.3, 0.05, 0.05, 0.3]))
    ch.weights(-2.5, prior)
    wait()
    got = ch.get("weights")
    assert_weights(got, numpy_weights(hits, nl, -2.5, prior))
    assert got.max() == 1.0
    # crafted records: the empty hypothesis, an unusable one, a truncated one, NaN and infinite scores
    H = ekf_mod.EkfAssocHit
    rec = (H * E)()
    for e, (m, status, d2, logdet) in enumerate([(0, 0, 0.0, 0.0), (3, AS_INVALID, 1.0, -20.0), (4, AS_TRUNCATED, 7.5, -31.0),
                                                 (2, 0, float("nan"), -11.0), (5, 0, 90.0, 80.0), (1, 0, 2.0, -INF)]):
        rec[e].m, rec[e].status, rec[e].d2, rec[e].logdet = m, status, d2, logdet
    counts = np.array([0, 8, 6, 2, 5, 4], dtype=np.int32)
    ch.put("hits", np.frombuffer(bytes(rec), dtype=np.uint8))
    ch.put("nlines", counts)
    for lu, pr in ((0.0, None), (-1.75, prior), (-INF, None)):
        ch.weights(lu, pr)
        wait()
        got, ref = ch.get("weights"), numpy_weights(rec, counts, lu, pr)
        assert_weights(got, ref)
        assert got.max() == 1.0 and got[1] == got[3] == got[5] == 0.0, (lu, got)
    assert ref[0] == 1.0 and ref[4] > 0.0                       # log_unassigned -inf: only where no line is left out
    for e in range(E):                                          # every instance out: all zero, which the plan reports
        rec[e].status = AS_INVALID
    ch.put("hits", np.frombuffer(bytes(rec), dtype=np.uint8))
    ch.weights()
    ch.plan(0.5)
    wait()
    assert np.array_equal(ch.get("weights"), np.zeros(E))
    info = ch.get("info")
    assert info.status == RP_INVALID and info.copies == 0 and ch.get("src").tolist() == list(range(E))
    lib, h, p = ekf_mod.load_library(), a.handle, ctypes.c_void_p(16)
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert lib.ekf_assoc_weights_device(h, args[0], args[1], 0.0, None, args[2]) == EINVAL
    ch.close()


# ---------------------------------------------------------------------------------------------
# stage 3: the plan
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_plan(ekf_mod):
    rng = np.random.default_rng(3)
    for E in (8, 5, 1, 70):
        a = ekf_mod.Ensemble(16, E, 0, max_lines=8)
        ch = Chain(ekf_mod, a, 16, 8, 1)
        cases = [(np.asarray(wt, dtype=np.float64), u, INF, src) for wt, u, src in FIXTURES if len(wt) == E]
        for trial in range(6):
            wt = rng.random(E) ** 4 * (40.0 if trial % 2 else 1e-3)
            wt[rng.random(E) < 0.25] = 0.0
            if not wt.any():
                wt[0] = 1.0
            cases.append((wt, float(rng.random()), INF, None))
        wt = rng.random(E) + 0.5
        ess = sequential_plan(wt, 0.25)[2]
        cases += [(wt, 0.25, ess * 1.01, None), (wt, 0.25, ess * 0.99, None), (wt * np.where(np.arange(E) == E - 1, -1.0, 1.0), 0.25, INF, None),
                  (np.zeros(E), 0.25, INF, None), (np.full(E, INF), 0.25, INF, None)]
        for wt, u, below, fixture in cases:
            ch.put("weights", wt)
            ch.plan(u, below)
            wait()
            down = ch.get("weights")                            # the device's own weights, downloaded
            status, copies, ress, total, src = sequential_plan(down.tolist(), u, below)
            got, info = ch.get("src").tolist(), ch.get("info")
            assert got == src and (fixture is None or got == fixture), (E, wt, u, got, src)
            assert (info.status, info.copies) == (status, copies) and same(info.total, total), (E, wt, u)
            assert abs(info.ess - ress) <= 1e-12 * ress
            assert all(got[got[e]] == got[e] for e in range(E))
            ch.put("src", np.full(E, -9, dtype=np.int32))
            ch.plan(u, below, info=False)                       # d_info NULL
            wait()
            assert ch.get("src").tolist() == src
        assert {sequential_plan(c[0].tolist(), c[1], c[2])[0] for c in cases} >= {RP_KEPT, RP_INVALID}
        lib, h, p = ekf_mod.load_library(), a.handle, ctypes.c_void_p(16)
        for u in (1.0, -0.01, float("nan"), 1.5):
            assert lib.ekf_resample_plan_device(h, p, u, INF, p, None) == ERANGE
        assert lib.ekf_resample_plan_device(h, p, 0.5, float("nan"), p, None) == EINVAL
        assert lib.ekf_resample_plan_device(h, None, 0.5, INF, p, None) == EINVAL
        assert lib.ekf_resample_plan_device(h, p, 0.5, INF, None, None) == EINVAL
        ch.close()


# ---------------------------------------------------------------------------------------------
# stage 4: the copy
# ---------------------------------------------------------------------------------------------
def resample_on_device(ens, src, expect=0):
    """ekf_resample_device with `src` uploaded; the status word must be `expect`."""
    bufs = [DeviceArray(np.asarray(src, dtype=np.int32)), junk(4)]
    ens.resample_device(bufs[0].address, bufs[1].address)
    wait()
    status = int(fetch(bufs[1], np.int32, (1,))[0])
    for b in bufs:
        b.close()
    assert status == expect, (src, status)


class DeviceCopies:
    """ekf_mod with Ensemble.resample and copy_instance going through ekf_resample_device, for
    tests.test_resample's Twin and run_twin."""

    def __init__(self, ekf_mod):
        self._mod = ekf_mod

        class Ens(ekf_mod.Ensemble):
            def resample(self, src):
                resample_on_device(self, src)

            def copy_instance(self, dst, frm):
                src = list(range(self.instances))
                src[dst] = frm
                resample_on_device(self, src)

        self.Ensemble = Ens

    def __getattr__(self, name):
        return getattr(self._mod, name)


@pytest.mark.gpu
@pytest.mark.parametrize("prec,pipeline,T,arith", [(0, 0, 4, 0), (1, 1, 3, 0), (1, 0, 16, 2)])
def test_device_copy_equals_twin(ekf_mod, prec, pipeline, T, arith):
    """tests.test_resample.test_resample_equals_twin with the device call: N = 64, src = [0, 0, 2, 0], the
    call after 6 of 16 scans (mid-group; at T = 3 behind a flush in flight), every read entry point right
    after it, FOLLOW scans in which a clone is fed its source's scans, then its own."""
    tw = run_twin(DeviceCopies(ekf_mod), 64, [0, 0, 2, 0], prec, bool(pipeline), T, arith, at=6, more=10)
    assert tw.counts(5, 6, "matches") > 0 and tw.counts(5, 6, "new_landmarks") > 0
    assert tw.counts(7, 16, "matches") > 0 and tw.counts(7, 16, "new_landmarks") > 0


@pytest.mark.gpu
def test_device_copy_exponents_travel(ekf_mod):
    """fp16 storage, EKF_ARITH_F16X3, T = 16, instances at different storage exponents: after the device
    call the host's mirror of the exponents is stale, and ekf_storage_exponent and the ekf_download_state
    that follows must see the source's."""
    N = 64
    w = G.make_world(N, active=N - 14)
    lo = G.initial_state(w, landmark_var=0.1)
    hi = G.initial_state(w, landmark_var=0.1)
    hi.diag = hi.diag * 64.0
    hi.U = hi.U * 8.0
    tw = Twin(DeviceCopies(ekf_mod), N, [0, 0], 2, False, 16, 2, states={0: hi, 1: lo})
    for _ in range(3):
        tw.scan()
    ex = [tw.a.storage_exponent(e) for e in range(2)]
    assert ex[0] < ex[1] == 10, ex
    tw.call("copy_instance")
    assert tw.a.storage_exponent(1) == ex[0] == tw.a.storage_exponent(0)
    trial = lineage_scan(tw.w, 0, 4)[1][:4]
    assert_reads_equal(tw.a, 1, 0, [15, 16, 3], trial, "after the device copy")
    for _ in range(6):
        tw.scan()
    tw.assert_flushes(9)
    tw.assert_final_states_equal()                              # (ekf_download_state unpacks with the exponent)


@pytest.mark.gpu
@pytest.mark.parametrize("N,src,prec,T,at,active", [(200, [1, 1, 2], 1, 8, 5, 170), (37, [1, 1], 0, 4, 3, 25)])
def test_device_copy_many_workgroups_and_partial_tiles(ekf_mod, N, src, prec, T, at, active):
    tw = run_twin(DeviceCopies(ekf_mod), N, src, prec, False, T, 0, at=at, more=5, active=active)
    assert tw.counts(at + 1, at + 5, "matches") > 0


@pytest.mark.gpu
def test_device_copy_nothing_pending(ekf_mod):
    """T = 3, the call after 6 scans: no step is pending, the source's last result record still travels."""
    tw = run_twin(DeviceCopies(ekf_mod), 64, [1, 1], 0, False, 3, 0, at=6, more=6)
    assert tw.counts(7, 12, "matches") > 0


def exports(ens):
    descs, images = ens.export_instances(list(range(ens.instances)))
    return [bytes(d) for d in descs], images


@pytest.mark.gpu
def test_device_copy_untouched_identity_and_export(ekf_mod):
    """EKF_ARITH_F16X3, fp32, T = 16 (where a drain would change every instance's bits). Context a copies
    through the device call, h through ekf_resample with the same list, c never: instances 0 and 2 of a end
    bit-identical to c's, an export of a right after the call equals an export of h (images and
    descriptors), and the identity list changes no byte and flushes nothing."""
    N, E, T, src = 64, 4, 16, [0, 0, 2, 0]
    w = G.make_world(N, active=N - 14)
    st = G.initial_state(w)
    kw = dict(max_lines=8, flush_interval=T, arith=2)
    a, h, c = (ekf_mod.Ensemble(N, E, 1, **kw) for _ in range(3))
    for ens in (a, h, c):
        for e in range(E):
            ens.init_lowrank(e, st.diag * (1.0 + 0.25 * e), st.U, st.y, st.saved, st.pose)
        ens.profile(1)
    own = list(range(E))
    for step in range(1, 17):
        lin = src if 6 < step <= 6 + FOLLOW else own
        ra, rh, rc = (ens.localize(*feed(w, lin, step)) for ens in (a, h, c))
        assert_results_equal([ra[0], ra[2]], [rc[0], rc[2]], step)
        assert_results_equal(ra, rh, step)
        if step == 6:
            resample_on_device(a, src)
            h.resample(src)
            da, ia = exports(a)
            dh, ih = exports(h)
            assert da == dh and np.array_equal(ia, ih)
            assert not np.array_equal(ia, exports(c)[1])
        if step == 10:
            before = exports(a)
            resample_on_device(a, own)
            after = exports(a)
            assert before[0] == after[0] and np.array_equal(before[1], after[1])
    assert [n for n, _ in a.profile_flushes()] == [n for n, _ in c.profile_flushes()] == [T]
    for e in range(E):
        Pa, ya, sa, pa = a.download_state(e)
        for ens in (h,) + ((c,) if e in (0, 2) else ()):
            Pc, yc, sc, pc = ens.download_state(e)
            assert same(Pa, Pc) and same(ya, yc) and same(pa, pc) and sa == sc, e
    assert not same(a.download_state(1, with_P=False)[1], c.download_state(1, with_P=False)[1])


@pytest.mark.gpu
def test_device_copy_refusals(ekf_mod):
    """A list ekf_resample would refuse leaves every byte as it was (the export before == after) and its
    status in d_status; a call between ekf_predict and ekf_update is refused by the host."""
    N, T = 64, 4
    w = G.make_world(N, active=N - 14)
    st = G.initial_state(w)
    for E, bad in ((2, [([1, 0], EINVAL)]), (3, [([1, 2, 2], EINVAL), ([0, 5, 2], ERANGE), ([0, -1, 2], ERANGE),
                                                 ([3, 1, 2], ERANGE), ([1, 2, 0], EINVAL)])):
        a = ekf_mod.Ensemble(N, E, 1, max_lines=8, flush_interval=T)
        for e in range(E):
            a.init_lowrank(e, st.diag * (1.0 + 0.25 * e), st.U, st.y, st.saved, st.pose)
        own = list(range(E))
        for step in (1, 2):
            a.localize(*feed(w, own, step))
        before = exports(a)
        lib = ekf_mod.load_library()
        for src, status in bad:
            assert lib.ekf_resample(a.handle, (ctypes.c_int32 * E)(*src)) == status      # (the host form's answer)
            resample_on_device(a, src, expect=status)
            after = exports(a)
            assert before[0] == after[0] and np.array_equal(before[1], after[1]), src
        d_src = DeviceArray(np.array([0] * E, dtype=np.int32))
        assert lib.ekf_resample_device(a.handle, None, None) == EINVAL
        enc, ln, nl = feed(w, own, 3)
        a.predict(enc)
        assert lib.ekf_resample_device(a.handle, d_src.ptr, None) == EINVAL
        a.update(ln, nl)
        assert lib.ekf_resample_device(a.handle, d_src.ptr, None) == 0                 # d_status NULL
        wait()
        _, y0, s0, p0 = a.download_state(0, with_P=False)
        for e in range(1, E):
            _, ye, se, pe = a.download_state(e, with_P=False)
            assert same(ye, y0) and se == s0 and same(pe, p0)
        d_src.close()
    s = ekf_mod.Ensemble(64, 1, 1, max_lines=8, flush_interval=4, shard=(0, 1))        # a partitioned context
    p = ctypes.c_void_p(16)
    assert lib.ekf_resample_device(s.handle, p, None) == EINVAL
    assert lib.ekf_resample_plan_device(s.handle, p, 0.5, INF, p, None) == EINVAL
    assert lib.ekf_gate_candidates_device(s.handle, p, p, 3, 0.4, p, None) == EINVAL
    assert lib.ekf_assoc_weights_device(s.handle, p, p, 0.0, None, p) == EINVAL


# ---------------------------------------------------------------------------------------------
# the loop, end to end
# ---------------------------------------------------------------------------------------------
def assert_contexts_equal(a, b, lm, trial, where):
    """Every read entry point gives for each instance of a what it gives for that instance of b."""
    assert_results_equal(a.read_results(), b.read_results(), where)
    for e in range(a.instances):
        _, ya, sa, pa = a.download_state(e, with_P=False)
        _, yb, sb, pb = b.download_state(e, with_P=False)
        assert same(ya, yb) and sa == sb and same(pa, pb), (where, "download_state", e)
        assert same(a.pose_cov(e), b.pose_cov(e)) and a.ellipse(e) == b.ellipse(e), (where, "pose_cov", e)
        ca, ma = a.query_joint(e, lm)
        cb, mb = b.query_joint(e, lm)
        assert same(ca, cb) and same(ma, mb), (where, "query_joint", e)
        ha, da = a.gate_lines(e, trial, distances=True)
        hb, db = b.gate_lines(e, trial, distances=True)
        assert same(da, db) and all(same(x[k], y[k]) for x, y in zip(ha, hb) for k in x), (where, "gate_lines", e)
        assert a.storage_exponent(e) == b.storage_exponent(e), (where, "storage_exponent", e)


@pytest.mark.gpu
def test_the_loop_end_to_end(ekf_mod):
    """E = 8, N = 64, fp32 storage, EKF_ARITH_F16X3, T = 16, the lineages of tests/test_resample.py (other
    initial scales, other line counts, extra lines). After 6 scans context a enqueues gate, candidates,
    search, weights, plan and copy for scan 7's lines with no host read in between and waits once. Its twin
    b runs each stage on the host, fed a's output of the stage before: the candidates and the list agree
    exactly, the hits bit for bit, the weights within 1e-10, and after b.resample(a's list) the two contexts
    agree bit for bit in every read and in the scans that follow. Context c runs the read-only stages only
    and ends bit-identical to n, which runs none."""
    N, E, ML, C, T, u = 64, 8, 8, 3, 16, 0.3125
    w = G.make_world(N, active=N - 14)
    st = G.initial_state(w)
    a, b, c, n = (ekf_mod.Ensemble(N, E, 1, max_lines=ML, flush_interval=T, arith=2) for _ in range(4))
    own = list(range(E))
    for ens in (a, b, c, n):
        for e in range(E):
            ens.init_lowrank(e, st.diag * (1.0 + 0.25 * e), st.U, st.y, st.saved, st.pose)
        ens.profile(1)
    for step in range(1, 7):
        for ens in (a, b, c, n):
            ens.localize(*feed(w, own, step))
    enc, ln, nl = feed(w, own, 7)
    prior = np.array([-40.0, -40.0, 0.0, -40.0, -40.0, -0.5, -40.0, -40.0])   # (whatever the scores: some instance dies)
    cha, chc = Chain(ekf_mod, a, N, ML, C), Chain(ekf_mod, c, N, ML, C)
    for ch in (cha, chc):
        ch.inputs(enc, ln, nl)
        ch.gate()
        ch.candidates(GATE_LOOSE)
        ch.search()
        ch.weights(0.0, prior)
        ch.plan(u)
    cha.copy()
    wait()                                                       # the one wait
    # the twin, stage by stage
    d2, cand, hits, weights = cha.get("d2"), cha.get("cand"), cha.get("hits"), cha.get("weights")
    src, info, status = cha.get("src").tolist(), cha.get("info"), int(cha.get("status")[0])
    bound = ekf_mod.chi2_bounds(ML, CONFIDENCE)
    for e in range(E):
        L = int(nl[e])
        _, dg = b.gate_lines(e, ln[e, :L], enc[e], distances=True)
        assert same(dg, d2[e, :L]), e
        assert np.array_equal(cand[e, :L], ekf_mod.gate_candidates(d2[e, :L], C, GATE_LOOSE)), e
        assert np.all(cand[e, L:] == -1)
        hb = b.associate_joint(e, ln[e, :L], cand[e, :L], bound[:L + 1], enc[e])
        assert hit_bits(hb) == hit_bits(a._assoc_hit(hits[e], L)) and hb["status"] == 0, (e, hb)
    ref = numpy_weights(hits, nl, 0.0, prior)
    assert_weights(weights, ref)
    assert weights.max() == 1.0
    rs, rc, ress, rtotal, rsrc = sequential_plan(weights.tolist(), u)
    assert src == rsrc and (info.status, info.copies) == (0, rc) and info.total == rtotal and status == 0
    assert abs(info.ess - ress) <= 1e-12 * ress
    assert info.copies >= 1 and all(src[src[e]] == src[e] for e in range(E)), src
    for name in ("cand", "weights", "src"):                      # c's read-only stages gave the same
        assert same(chc.get(name), cha.get(name)), name
    b.resample(src)
    trial = lineage_scan(w, 0, 7)[1][:4]
    assert_contexts_equal(a, b, [15, 16, 3], trial, "after the loop")
    for step in range(7, 13):                                    # clones follow their sources, then go their own way
        lin = src if step <= 6 + FOLLOW else own
        ra, rb = a.localize(*feed(w, lin, step)), b.localize(*feed(w, lin, step))
        assert_results_equal(ra, rb, step)
        c.localize(*feed(w, own, step))
        n.localize(*feed(w, own, step))
    for x, y in ((a, b), (c, n)):
        assert [k for k, _ in x.profile_flushes()] == [k for k, _ in y.profile_flushes()] == []
        for e in range(E):
            Px, yx, sx, px = x.download_state(e)
            Py, yy, sy, py = y.download_state(e)
            assert same(Px, Py) and same(yx, yy) and same(px, py) and sx == sy, e
    cha.close()
    chc.close()
