"""Instance images (slam_ekf.h ekf_export_instances / ekf_import_instances and their device forms,
dist.global_resample_plan / resample_global): an instance leaves one context as a position-independent
image and enters a slot of another that stands at the same point of its flush group, pending steps
included, without a drain or a flush on either side.

CPU: the header, the binding, the NULL-context returns, the global resampler, a two-rank gloo run of
resample_global over stub ensembles. GPU: twins across contexts. Context `a` runs four instances
(lineages 0..3 of tests/test_resample.py: another initial scale, fewer lines, extra random lines on
some steps). Context `c` runs three others and is one whole flush group ahead of `a`: as many steps
pending, but another step count, other ring slots, another launch epoch and, pipelined, the other
buffer parity. After 6 scans of `a` its instance 2 goes into slot 1 of `c`. In twin `b` slot 1 was
initialised as lineage 2 when `a` was (after b's first group, at a group boundary) and fed as lineage 2
from then on; `b` never imports. From the import on `c` must equal `b` bit for bit in every slot: every
result, every read entry point, the flushes that ran, the final dense states.
"""
import ctypes
import os
import socket

import numpy as np
import pytest

from slam_ros_amd import scan_gen as G
from tests.hipmem import DeviceArray, hip
from tests.test_resample import CONFIGS, assert_reads_equal, assert_results_equal, counts_of, lineage_scan, same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("ekf_instance_image_bytes", "ekf_export_instances", "ekf_import_instances",
             "ekf_export_instances_device", "ekf_import_instances_device")
EINVAL, ERANGE = 1, 4


# ---------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------
def test_header_declares_images():
    from tests.test_abi import declared_functions
    names = declared_functions()
    for fn in FUNCTIONS:
        assert fn in names, fn
    src = open(os.path.join(ROOT, "include", "slam_ekf.h")).read()
    assert "#define SLAM_EKF_ABI_VERSION 3" in src   # entry points only: the number stays
    assert "typedef struct ekf_image_desc" in src


def test_binding_exports_images(ekf_mod):
    for fn in FUNCTIONS:
        assert fn in ekf_mod.EXPORTED, fn
    for m in ("instance_image_bytes", "export_instances", "import_instances", "export_instances_device",
              "import_instances_device"):
        assert callable(getattr(ekf_mod.Ensemble, m)), m
    assert ctypes.sizeof(ekf_mod.EkfImageDesc) == 64 and ekf_mod.EkfImageDesc.bytes.offset == 16
    from slam_ros_amd import dist
    assert callable(dist.global_resample_plan) and callable(dist.resample_global)


def test_null_context_is_einval(ekf_mod):
    """No context: EKF_EINVAL (0 bytes) before any HIP call."""
    lib = ekf_mod.load_library()
    inst = (ctypes.c_int32 * 2)(0, 1)
    buf = (ctypes.c_ubyte * 64)()
    desc = (ekf_mod.EkfImageDesc * 2)()
    assert lib.ekf_instance_image_bytes(None) == 0
    for fn in (lib.ekf_export_instances, lib.ekf_import_instances, lib.ekf_export_instances_device,
               lib.ekf_import_instances_device):
        assert fn(None, inst, 2, buf, desc) == EINVAL
        assert fn(None, None, 0, None, None) == EINVAL
        assert fn(None, inst, -1, buf, desc) == EINVAL


def random_weights(rng, E):
    w = rng.random(E) ** 4
    w[rng.random(E) < 0.25] = 0.0
    if not w.any():
        w[rng.integers(E)] = 1.0
    return w * rng.choice([1e-3, 1.0, 40.0])


def test_global_resample_plan():
    from slam_ros_amd.dist import global_resample_plan
    rng = np.random.default_rng(9)
    layouts = [[2, 2], [4, 4], [3, 5], [1, 7], [4, 0, 4], [0, 6], [8, 8, 8, 8], [5, 1, 2], [1, 1, 1]]
    for trial in range(200):
        counts = layouts[trial % len(layouts)]
        E = sum(counts)
        first = np.concatenate([[0], np.cumsum(counts)])
        w = random_weights(rng, E)
        kind = trial % 5
        if kind == 1:      # all the weight on one rank
            r = [k for k, c in enumerate(counts) if c][trial % sum(1 for c in counts if c)]
            keep = np.zeros(E, dtype=bool)
            keep[first[r]: first[r + 1]] = True
            w = np.where(keep, w + 1e-3, 0.0)
        elif kind == 2:    # a dead rank
            r = [k for k, c in enumerate(counts) if c][0]
            if sum(1 for c in counts if c) > 1:
                w[first[r]: first[r + 1]] = 0.0
                if not w.any():
                    w[-1] = 1.0
        elif kind == 3:    # one instance takes everything
            w = np.zeros(E)
            w[trial % E] = 3.0
        u = float(rng.random())
        local, transfers = global_resample_plan(w, u, counts)
        assert [len(l) for l in local] == counts
        # the copies per instance equal the plain walk along the concatenated weights
        copies = np.zeros(E, dtype=int)
        written = set()
        for r, lst in enumerate(local):
            assert all(0 <= s < counts[r] for s in lst)
            assert all(lst[lst[e]] == lst[e] for e in range(counts[r])), (trial, r, lst)   # resample_check's rule
            for e, s in enumerate(lst):
                copies[first[r] + s] += 1
                if s != e:
                    written.add((r, e))
        for sr, se, dr, de in transfers:
            assert sr != dr and 0 <= se < counts[sr] and 0 <= de < counts[dr]
            assert local[sr][se] == se, "a transfer's source is a survivor that keeps its slot"
            assert local[dr][de] == de, "the slot a transfer fills is left alone by the local list"
            assert (dr, de) not in written, "a slot is written twice"
            written.add((dr, de))
            copies[first[dr] + de] -= 1       # (the local list counted the slot as its own copy)
            copies[first[sr] + se] += 1
        want = counts_of(w, u)
        assert list(copies) == want, (trial, counts, list(copies), want)
        # every source is a fixed point: no written slot is a source
        sources = {(r, s) for r, lst in enumerate(local) for e, s in enumerate(lst) if s != e}
        sources |= {(sr, se) for sr, se, _, _ in transfers}
        dead = {(r, e) for r in range(len(counts)) for e in range(counts[r]) if want[first[r] + e] == 0}
        assert written == dead and not (sources & dead)
        owed = [sum(want[first[r]: first[r + 1]]) for r in range(len(counts))]
        assert len(transfers) == sum(max(0, owed[r] - counts[r]) for r in range(len(counts))), (trial, owed, counts)
    with pytest.raises(ValueError):
        global_resample_plan([0.5, 0.5], 0.3, [3])


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


class StubEnsemble:
    """An instance is a numpy row and its image is the row itself."""

    def __init__(self, rows):
        self.rows = np.array(rows, dtype=np.uint8)
        self.calls = []

    def instance_image_bytes(self):
        return self.rows.shape[1]

    def export_instances(self, inst):
        from slam_ros_amd.ekf import EkfImageDesc
        descs = []
        for e in inst:
            d = EkfImageDesc()
            d.magic, d.bytes, d.storage_exp = 0x474d4945, self.rows.shape[1], int(self.rows[e, 0])
            descs.append(d)
        self.calls.append(("export", list(inst)))
        return descs, self.rows[list(inst)].copy()

    def import_instances(self, inst, images, descs):
        for k, e in enumerate(inst):
            assert descs[k].magic == 0x474d4945 and descs[k].bytes == self.rows.shape[1]
            assert descs[k].storage_exp == int(images[k][0])     # the descriptor travelled with its image
            self.rows[e] = images[k]
        self.calls.append(("import", list(inst)))

    def resample(self, src):
        self.rows = self.rows[list(src)].copy()
        self.calls.append(("resample", list(src)))


GLOO_COUNTS = (3, 5)
GLOO_W = [0.0, 0.0, 0.01, 0.3, 0.0, 0.3, 0.0, 0.39]   # rank 1 is owed more than it holds


def gloo_rows(rank):
    first = sum(GLOO_COUNTS[:rank])
    return [[16 * (first + e) + j for j in range(16)] for e in range(GLOO_COUNTS[rank])]


def gloo_worker(rank, world, port, q):
    import torch.distributed as dist
    from slam_ros_amd import dist as D
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ens = StubEnsemble(gloo_rows(rank))
    first = sum(GLOO_COUNTS[:rank])
    local, transfers = D.resample_global(ens, GLOO_W[first: first + GLOO_COUNTS[rank]], 0.4, dist, rank, world,
                                         host_coll=True)
    q.put((rank, ens.rows.tolist(), local, transfers, ens.calls))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_resample_global_routes_images():
    """resample_global over gloo with stub ensembles: every slot ends as the instance the plan gives it,
    across ranks too, and the calls return."""
    import torch.multiprocessing as mp
    from slam_ros_amd.dist import global_resample_plan
    port = free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=gloo_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=240) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    local, transfers = global_resample_plan(GLOO_W, 0.4, GLOO_COUNTS)
    assert transfers, "the weights force a transfer"
    assert any(s != e for lst in local for e, s in enumerate(lst)), "and a local copy"
    owner = {(r, e): (r, s) for r, lst in enumerate(local) for e, s in enumerate(lst)}
    for sr, se, dr, de in transfers:
        owner[(dr, de)] = (sr, se)
    before = [gloo_rows(0), gloo_rows(1)]
    for rank, rows, loc, tr, calls in got:
        assert loc == local[rank] and [tuple(t) for t in tr] == transfers
        for e in range(GLOO_COUNTS[rank]):
            r0, e0 = owner[(rank, e)]
            assert rows[e] == before[r0][e0], (rank, e, owner[(rank, e)])
        assert calls[-1] == ("resample", local[rank])
    copies = counts_of(GLOO_W, 0.4)
    ends = [tuple(row) for _, rows, _, _, _ in got for row in rows]
    flat = [tuple(row) for rows in before for row in rows]
    assert [ends.count(f) for f in flat] == copies


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
def feed_pairs(w, pairs, max_lines=8):
    """One scan for an ensemble whose slot k runs step pairs[k][1] of lineage pairs[k][0]."""
    E = len(pairs)
    enc, ln, nl = np.zeros((E, 3)), np.zeros((E, max_lines, 6)), np.zeros(E, dtype=np.int32)
    for e, (lin, step) in enumerate(pairs):
        if isinstance(lin, tuple):     # (lineage, rows): a scan given outright
            enc[e], rows = lineage_scan(w, lin[0], step)[0], lin[1]
        else:
            enc[e], rows = lineage_scan(w, lin, step)
        ln[e, :len(rows)] = rows
        nl[e] = len(rows)
    return enc, ln, nl


def init(ens, slot, lin, st, states=None):
    if states is not None:
        s = states.get(lin, states[None])
        ens.init_lowrank(slot, s.diag, s.U, s.y, s.saved, s.pose)
    else:
        ens.init_lowrank(slot, st.diag * (1.0 + 0.25 * lin), st.U, st.y, st.saved, st.pose)


def transfer(src, src_list, dst, dst_list, form):
    """Images of src's instances into dst's slots; returns the image bytes."""
    if form == "host":
        descs, images = src.export_instances(src_list)
        dst.import_instances(dst_list, images, descs)
        return descs, images
    # the device forms order nothing between two contexts, and ekf_sync would drain: both contexts run
    # on one stream (share_stream, set before the first step), so the import follows the export
    assert src.test_stream is dst.test_stream
    buf = DeviceArray(np.full((len(src_list), src.instance_image_bytes()), 0xA5, dtype=np.uint8))
    descs = src.export_instances_device(src_list, buf.address)
    dst.import_instances_device(dst_list, buf.address, descs)
    wait(src.test_stream)
    images = device_bytes(buf, (len(src_list), src.instance_image_bytes()))
    buf.close()
    return descs, images


def share_stream(*ensembles):
    """One HIP stream for all the contexts given (ekf_set_stream drains: call it before the first step)."""
    stream = ctypes.c_void_p()
    assert hip().hipStreamCreate(ctypes.byref(stream)) == 0, "hipStreamCreate"
    for ens in ensembles:
        ens.set_stream(stream.value)
        ens.test_stream = stream
    return stream


def wait(stream):
    """The stream's work is done; no context is drained."""
    hip().hipStreamSynchronize.argtypes = [ctypes.c_void_p]
    assert hip().hipStreamSynchronize(stream) == 0, "hipStreamSynchronize"


def device_bytes(buf, shape):
    out = np.zeros(shape, dtype=np.uint8)
    assert hip().hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), buf.ptr, out.nbytes, 2) == 0, "hipMemcpy"
    return out


def reads(ens, e, lm, trial):
    """What every read entry point gives for instance e (no drain)."""
    res = ens.read_results()[e]
    _, y, saved, pose = ens.download_state(e, with_P=False)
    cov, mean = ens.query_joint(e, lm)
    hits, d2 = ens.gate_lines(e, trial, distances=True)
    assign = [[h["nearest"] for h in hits], [-1] + [h["nearest"] for h in hits][1:]]
    joint, each = ens.gate_joint(e, trial, assign, each=True)
    return dict(res=res, y=y, saved=saved, pose=pose, pose_cov=ens.pose_cov(e), ellipse=ens.ellipse(e), cov=cov,
                mean=mean, hits=hits, d2=d2, joint=joint, each=each, exp=ens.storage_exponent(e))


def assert_same_reads(x, y, where):
    assert_results_equal([x["res"]], [y["res"]], (where, "read_results"))
    for k in ("y", "pose", "pose_cov", "cov", "mean", "d2", "each"):
        assert same(x[k], y[k]), (where, k)
    assert x["saved"] == y["saved"] and x["ellipse"] == y["ellipse"] and x["exp"] == y["exp"], where
    for p, q in zip(x["hits"], y["hits"]):
        assert all(same(p[k], q[k]) for k in p), (where, "gate_lines", p, q)
    for p, q in zip(x["joint"], y["joint"]):
        assert all(same(p[k], q[k]) for k in p), (where, "gate_joint", p, q)


def assert_states_equal(x, ex, y, ey, where):
    Px, yx, sx, px = x.download_state(ex)
    Py, yy, sy, py = y.download_state(ey)
    assert same(Px, Py), (where, np.argwhere(Px != Py)[:8].tolist())
    assert same(yx, yy) and same(px, py) and sx == sy, where


def cross_twin(ekf_mod, N, prec, pipeline, T, arith, form, at=6, more=10, active=None, reset_margin=10, states=None,
               last_rows=None):
    """The scenario of the module docstring; last_rows: the lines of lineage 2's scan `at` (the last
    before the export). Returns (a, b, c, log, at_export) with log[step] = results of c after the import
    and at_export what the read entry points gave for a's instance 2 at the export."""
    w = G.make_world(N, active=N - 14 if active is None else active)
    st = G.initial_state(w)
    kw = dict(max_lines=8, pipeline=bool(pipeline), flush_interval=T, arith=arith, reset_margin=reset_margin)
    a = ekf_mod.Ensemble(N, 4, prec, **kw)
    b = ekf_mod.Ensemble(N, 3, prec, **kw)
    c = ekf_mod.Ensemble(N, 3, prec, **kw)
    if form == "device":
        share_stream(a, c)
    for e in range(4):
        init(a, e, e, st, states)
    for ens in (b, c):
        for e, lin in enumerate((4, 5, 6)):
            init(ens, e, lin, st, states)
        ens.profile(1)
    for j in range(1, T + 1):        # c and b one whole group ahead
        sc = feed_pairs(w, [(4, j), (5, j), (6, j)])
        assert_results_equal(c.localize(*sc), b.localize(*sc), ("lead-in", j))
    init(b, 1, 2, st, states)        # (at a group boundary)

    def lin2(i):
        return ((2, last_rows), i) if (last_rows is not None and i == at) else (2, i)

    for i in range(1, at + 1):
        ra = a.localize(*feed_pairs(w, [(0, i), (1, i), lin2(i), (3, i)]))
        rc = c.localize(*feed_pairs(w, [(4, T + i), (5, T + i), (6, T + i)]))
        rb = b.localize(*feed_pairs(w, [(4, T + i), lin2(i), (6, T + i)]))
        assert_results_equal([ra[2]], [rb[1]], ("the twin's premise", i))
        assert_results_equal([rc[0], rc[2]], [rb[0], rb[2]], ("before the import", i))
    assert not same(c.download_state(1, with_P=False)[1], a.download_state(2, with_P=False)[1])
    nbytes = a.instance_image_bytes()
    assert nbytes == c.instance_image_bytes() and nbytes % 16 == 0
    trial = lineage_scan(w, 2, at + 1)[1][:4]
    lm = [j for j in (15, 16, 3, 16) if j < N]
    at_export = reads(a, 2, lm, trial)
    descs, _ = transfer(a, [2], c, [1], form)
    assert descs[0].bytes == nbytes and descs[0].pending == (at % T if not pipeline or at < T else T + at % T)
    where = ("after the import", N, prec, pipeline, T, arith, form)
    assert_same_reads(reads(c, 1, lm, trial), at_export, where + ("slot 1 against the exported instance",))
    for e in range(3):
        assert_same_reads(reads(c, e, lm, trial), reads(b, e, lm, trial), where + (e,))
    log = {}
    for i in range(at + 1, at + more + 1):
        ra = a.localize(*feed_pairs(w, [(0, i), (1, i), (2, i), (3, i)]))
        sc = feed_pairs(w, [(4, T + i), (2, i), (6, T + i)])
        rc, rb = c.localize(*sc), b.localize(*sc)
        assert_results_equal(rc, rb, (where, i))
        assert_results_equal([rc[1]], [ra[2]], (where, "against the source", i))
        log[i] = rc
    fc = [n for n, _ in c.profile_flushes()]
    fb = [n for n, _ in b.profile_flushes()]
    assert fc == fb == [T] * ((T + at + more) // T), (fc, fb)
    for e in range(3):
        assert_states_equal(c, e, b, e, where + ("final", e))
    assert_states_equal(c, 1, a, 2, where + ("final, against the source",))
    return a, b, c, log, at_export


def form_of(k):
    return ("host", "device")[k % 2]


@pytest.mark.gpu
@pytest.mark.parametrize("k,cfg", list(enumerate(CONFIGS)))
def test_cross_context_twin(ekf_mod, k, cfg):
    """N = 64 over every precision, schedule, flush interval and arithmetic of tests/test_resample.py;
    the host and the device form alternate over the list. Matches and new landmarks are pending at the
    transfer and follow it."""
    prec, pipeline, T, arith = cfg
    _, _, _, log, _ = cross_twin(ekf_mod, 64, prec, pipeline, T, arith, form_of(k))
    assert sum(r[1]["matches"] for r in log.values()) > 0
    assert sum(r[1]["new_landmarks"] for r in log.values()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("prec,pipeline,T,arith", [(1, 0, 4, 2), (0, 1, 4, 0)])
def test_same_context_equals_copy_instance(ekf_mod, form, prec, pipeline, T, arith):
    """Export plus import into a slot of the same context equals ekf_copy_instance, bit for bit."""
    N = 64
    w = G.make_world(N, active=N - 14)
    st = G.initial_state(w)
    kw = dict(max_lines=8, pipeline=bool(pipeline), flush_interval=T, arith=arith)
    p, q = ekf_mod.Ensemble(N, 3, prec, **kw), ekf_mod.Ensemble(N, 3, prec, **kw)
    if form == "device":
        share_stream(p)
    for ens in (p, q):
        for e in range(3):
            init(ens, e, e, st)
    for i in range(1, 7):
        sc = feed_pairs(w, [(0, i), (1, i), (2, i)])
        assert_results_equal(p.localize(*sc), q.localize(*sc), i)
    transfer(p, [2], p, [0], form)
    q.copy_instance(0, 2)
    trial = lineage_scan(w, 2, 7)[1][:4]
    for e in range(3):
        assert_same_reads(reads(p, e, [15, 16, 3], trial), reads(q, e, [15, 16, 3], trial), (form, e))
    assert_reads_equal(p, 0, 2, [15, 16, 3], trial, form)
    for i in range(7, 13):
        sc = feed_pairs(w, [(2, i), (1, i), (2, i)] if i < 10 else [(0, i), (1, i), (2, i)])
        assert_results_equal(p.localize(*sc), q.localize(*sc), i)
    for e in range(3):
        assert_states_equal(p, e, q, e, (form, e))


@pytest.mark.gpu
def test_export_leaves_the_context_untouched(ekf_mod):
    """EKF_ARITH_F16X3, fp32, T = 16 (where a drain would change every instance's bits): a context that
    exported every instance mid-group, in both forms, ends bit-identical to one that never did; the two
    forms give the same bytes, two exports in a row too, and an import of an instance's own image
    changes nothing."""
    N, E, T = 64, 4, 16
    w = G.make_world(N, active=N - 14)
    st = G.initial_state(w)
    kw = dict(max_lines=8, flush_interval=T, arith=2)
    x, y = ekf_mod.Ensemble(N, E, 1, **kw), ekf_mod.Ensemble(N, E, 1, **kw)
    stream = share_stream(x)
    for ens in (x, y):
        for e in range(E):
            init(ens, e, e, st)
        ens.profile(1)
    for i in range(1, 17):
        sc = feed_pairs(w, [(e, i) for e in range(E)])
        assert_results_equal(x.localize(*sc), y.localize(*sc), i)
        if i in (6, 11):
            order = [3, 1, 0, 1]                         # (an export list may repeat an instance; K <= E)
            descs, host = x.export_instances(order)
            _, again = x.export_instances(order)
            buf = DeviceArray(np.full((len(order), x.instance_image_bytes()), 0xA5, dtype=np.uint8))
            ddev = x.export_instances_device(order, buf.address)
            wait(stream)
            dev = device_bytes(buf, host.shape)
            buf.close()
            assert host.shape == dev.shape and np.array_equal(host, again) and np.array_equal(host, dev)
            assert np.array_equal(host[1], host[3]) and not np.array_equal(host[0], host[1])
            assert [bytes(d) for d in descs] == [bytes(d) for d in ddev]
            assert all(d.pending == i and d.has_step == 1 and d.bytes == host.shape[1] for d in descs)
            if i == 11:
                x.import_instances([1], host[1:2], descs[1:2])     # its own image: the same bytes again
    assert [n for n, _ in x.profile_flushes()] == [n for n, _ in y.profile_flushes()] == [T]
    for e in range(E):
        assert_states_equal(x, e, y, e, e)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["host", "device"])
def test_many_workgroups_other_epoch_and_status(ekf_mod, form):
    """N = 200, fp32: an instance spans several association workgroups, whose completion words carry
    the source's launch epoch; the destination is 8 launches ahead. The source's last scan before the
    export overflows the capacity (reset_margin 0, 195 landmarks, 8 unmatched lines: EKF_ST_CAPACITY).
    ekf_read_results on the slot (inside cross_twin's reads) must give the source's status, without
    EKF_ST_SYNC_TIMEOUT."""
    N, T, at = 200, 8, 5
    rows = G.random_lines(np.random.default_rng([5, 5]), 8)
    a, b, c, log, at_export = cross_twin(ekf_mod, N, 1, 0, T, 0, form, at=at, more=5, active=195, reset_margin=0,
                                         last_rows=rows)
    st = at_export["res"]["status"]
    assert st & ekf_mod.ST_CAPACITY and not st & ekf_mod.ST_SYNC_TIMEOUT, st
    # (cross_twin compared read_results of the slot right after the import with exactly this record)


@pytest.mark.gpu
def test_status_travels_with_the_completion_words(ekf_mod):
    """The same transfer looked at directly: right after the import read_results gives the slot the
    source's status bits (EKF_ST_CAPACITY among them) and no EKF_ST_SYNC_TIMEOUT, although every
    completion word in the image carries another context's epoch."""
    N, T = 200, 8
    w = G.make_world(N, active=195)
    st = G.initial_state(w)
    kw = dict(max_lines=8, flush_interval=T, reset_margin=0)
    a, c = ekf_mod.Ensemble(N, 2, 1, **kw), ekf_mod.Ensemble(N, 3, 1, **kw)
    for e in range(2):
        init(a, e, e, st)
    for e in range(3):
        init(c, e, 4 + e, st)
    for j in range(1, T + 1):
        c.localize(*feed_pairs(w, [(4, j), (5, j), (6, j)]))
    rows = G.random_lines(np.random.default_rng([5, 5]), 8)
    for i in range(1, 4):
        ra = a.localize(*feed_pairs(w, [(0, i), ((1, rows), i) if i == 3 else (1, i)]))
        c.localize(*feed_pairs(w, [(4, T + i), (5, T + i), (6, T + i)]))
    assert ra[1]["status"] & ekf_mod.ST_CAPACITY, ra[1]
    descs, images = a.export_instances([1])
    assert descs[0].groups >= 2 and descs[0].epoch == 3
    kept = images.copy()
    c.import_instances([2], images, descs)
    assert np.array_equal(images, kept)        # the re-tag works on a private copy
    rc = c.read_results()
    assert_results_equal([rc[2]], [a.read_results()[1]], "the slot's record")
    assert rc[2]["status"] == ra[1]["status"] and not rc[2]["status"] & ekf_mod.ST_SYNC_TIMEOUT
    assert not any(r["status"] & ekf_mod.ST_SYNC_TIMEOUT for r in rc)


@pytest.mark.gpu
@pytest.mark.parametrize("prec,form", [(0, "host"), (1, "device")])
def test_partial_tile_and_odd_strip(ekf_mod, prec, form):
    """N = 37: M = 74, a partial last tile and an odd strip length (8-byte class pieces)."""
    _, _, _, log, _ = cross_twin(ekf_mod, 37, prec, 0, 4, 0, form, at=3, more=5, active=25)
    assert sum(r[1]["matches"] for r in log.values()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("prec,form", [(0, "device"), (2, "host")])
def test_nothing_pending(ekf_mod, prec, form):
    """The sequential schedule at a group boundary (T = 3, the transfer after 6 scans): no step is
    pending and the source's newest result record travels (read_results inside cross_twin's reads)."""
    _, _, _, log, _ = cross_twin(ekf_mod, 64, prec, 0, 3, 0, form, at=6, more=6)
    assert sum(r[1]["matches"] for r in log.values()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("arith,form", [(2, "host"), (0, "device")])
def test_exponents_travel(ekf_mod, arith, form):
    """fp16 storage: the travelling lineage's variances are 2^6 times the others' (storage exponents
    below 10 and 10), so the storage exponent and its host mirror, and with EKF_ARITH_F16X3 the plane
    exponent and the largest variance, travel with the image; download_state of the slot (the final
    states inside cross_twin) uses the mirrored exponent."""
    N = 64
    w = G.make_world(N, active=N - 14)
    lo = G.initial_state(w, landmark_var=0.1)
    hi = G.initial_state(w, landmark_var=0.1)
    hi.diag = hi.diag * 64.0
    hi.U = hi.U * 8.0
    a, b, c, _, _ = cross_twin(ekf_mod, N, 2, 0, 4, arith, form, at=3, more=6, states={2: hi, None: lo})
    assert a.storage_exponent(2) < a.storage_exponent(0) == 10
    assert c.storage_exponent(1) == a.storage_exponent(2) == b.storage_exponent(1)
    assert c.storage_exponent(0) == c.storage_exponent(2) == 10


@pytest.mark.gpu
def test_errors(ekf_mod):
    """Refused calls leave every byte as it was: both contexts still match their twins after one more
    scan."""
    N, T = 64, 4
    w = G.make_world(N, active=N - 14)
    st = G.initial_state(w)
    base = dict(max_lines=8, flush_interval=T)

    def make(E, lins, n=N, prec=1, **over):
        ww = w if n == N else G.make_world(n, active=n - 14)
        s0 = st if n == N else G.initial_state(ww)
        ens = ekf_mod.Ensemble(n, E, prec, **dict(base, **over))
        for e, lin in enumerate(lins):
            init(ens, e, lin, s0)
        return ens, ww

    (a, _), (a2, _) = make(4, range(4)), make(4, range(4))
    (c, _), (c2, _) = make(3, (4, 5, 6)), make(3, (4, 5, 6))
    for i in (1, 2):
        sa, sc = feed_pairs(w, [(e, i) for e in range(4)]), feed_pairs(w, [(4, i), (5, i), (6, i)])
        for ens, s in ((a, sa), (a2, sa), (c, sc), (c2, sc)):
            ens.localize(*s)
    lib = ekf_mod.load_library()

    def snapshot(ens, E):
        return [(ens.download_state(e, with_P=False)[1:], ens.query_joint(e, [15, 16]), ens.read_results()[e],
                 ens.storage_exponent(e)) for e in range(E)], ens.export_instances(list(range(E)))[1]

    def unchanged(ens, E, before):
        now, img = snapshot(ens, E)
        assert np.array_equal(img, before[1]), "a refused call changed an instance's image"
        for x, y in zip(before[0], now):
            assert same(x[0][0], y[0][0]) and x[0][1] == y[0][1] and same(x[0][2], y[0][2])
            assert same(x[1][0], y[1][0]) and same(x[1][1], y[1][1]) and x[3] == y[3]
            assert_results_equal([x[2]], [y[2]], "refused call")

    def arr(v):
        return (ctypes.c_int32 * len(v))(*v)

    sa, sc = snapshot(a, 4), snapshot(c, 3)
    descs, images = a.export_instances([2, 0])
    darr = (ekf_mod.EkfImageDesc * 2)(*descs)
    dbuf = DeviceArray(images)      # (the device forms get device memory, refused or not)
    hbuf, dptr = images.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(dbuf.address)
    forms = ((lib.ekf_import_instances, hbuf), (lib.ekf_import_instances_device, dptr),
             (lib.ekf_export_instances, hbuf), (lib.ekf_export_instances_device, dptr))
    for fn, buf in forms:
        assert fn(c.handle, arr([0, 3]), 2, buf, darr) == ERANGE
        assert fn(c.handle, arr([0, -1]), 2, buf, darr) == ERANGE
        assert fn(c.handle, arr([0, 1]), -1, buf, darr) == ERANGE
        assert fn(c.handle, arr([0, 1, 2, 0]), 4, buf, darr) == ERANGE      # K > E
        assert fn(c.handle, None, 2, buf, darr) == EINVAL
        assert fn(c.handle, arr([0, 1]), 2, None, darr) == EINVAL
        assert fn(c.handle, arr([0, 1]), 2, buf, None) == EINVAL
        assert fn(c.handle, arr([0, 1]), 0, buf, darr) == 0                 # K == 0: valid, nothing happens
    for fn, buf in forms[:2]:
        assert fn(c.handle, arr([1, 1]), 2, buf, darr) == EINVAL            # a duplicate slot
    # wrong magic, version, bytes, key, pending, has_step, groups
    for field, val in (("magic", 7), ("version", 99), ("bytes", descs[0].bytes + 16), ("key", descs[0].key ^ 1),
                       ("pending", descs[0].pending + 1), ("has_step", 0), ("groups", descs[0].groups + 1)):
        bad = (ekf_mod.EkfImageDesc * 1)(ekf_mod.EkfImageDesc.from_buffer_copy(bytes(descs[0])))
        setattr(bad[0], field, val)
        assert lib.ekf_import_instances(c.handle, arr([1]), 1, hbuf, bad) == EINVAL, field
        assert lib.ekf_import_instances_device(c.handle, arr([1]), 1, dptr, bad) == EINVAL, field
    # descriptors of contexts that differ in N, precision, T, arith or max_lines
    for over in (dict(n=48), dict(prec=2), dict(flush_interval=8), dict(arith=2), dict(max_lines=7),
                 dict(pipeline=True), dict(reset_margin=9), dict(mahalanobis=0.5)):
        o, ow = make(2, (0, 1), **over)
        for i in (1, 2):
            o.localize(*feed_pairs(ow, [(0, i), (1, i)], max_lines=over.get("max_lines", 8)))
        od, oi = o.export_instances([1])
        assert od[0].key != descs[0].key, over
        with pytest.raises(ekf_mod.EkfError) as ei:
            c.import_instances([1], oi, od)
        assert ei.value.code == EINVAL, over
        o.close()
    # the same configuration with another E is congruent (the key does not depend on E) ...
    assert descs[0].key == c.export_instances([0])[0][0].key
    unchanged(a, 4, sa)
    unchanged(c, 3, sc)
    # ... but not one scan ahead: another pending count
    sc3 = feed_pairs(w, [(4, 3), (5, 3), (6, 3)])
    c.localize(*sc3)
    c2.localize(*sc3)
    sc = snapshot(c, 3)
    with pytest.raises(ekf_mod.EkfError) as ei:
        c.import_instances([1], images[:1], descs[:1])
    assert ei.value.code == EINVAL
    unchanged(c, 3, sc)
    # between ekf_predict and ekf_update
    enc, ln, nl = feed_pairs(w, [(e, 3) for e in range(4)])
    a.predict(enc)
    a2.predict(enc)
    for fn, buf in forms:
        assert fn(a.handle, arr([1]), 1, buf, darr) == EINVAL
    assert_results_equal(a.update(ln, nl), a2.update(ln, nl), "update after a refused call")
    # a partitioned context
    s = ekf_mod.Ensemble(64, 1, 1, max_lines=8, flush_interval=4, shard=(0, 1))
    assert s.instance_image_bytes() == 0
    for fn, buf in forms:
        assert fn(s.handle, arr([0]), 1, buf, darr) == EINVAL
    # both contexts still match their twins after one more scan
    s4a, s4c = feed_pairs(w, [(e, 4) for e in range(4)]), feed_pairs(w, [(4, 4), (5, 4), (6, 4)])
    assert_results_equal(a.localize(*s4a), a2.localize(*s4a), "a, one more scan")
    assert_results_equal(c.localize(*s4c), c2.localize(*s4c), "c, one more scan")
    for e in range(4):
        assert_states_equal(a, e, a2, e, ("a", e))
    for e in range(3):
        assert_states_equal(c, e, c2, e, ("c", e))
