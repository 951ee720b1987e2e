"""Ensemble sharding across ranks: one process per GPU, E_total independent EKF
instances split into contiguous slices, the scan stream sent once per step from the sensor rank.

The reference has a single Robot per node (slam_ros/main.cpp:98) fed by one scan topic
(main.cpp:37-56); the ensemble gives every instance the same scan with its own seeded
perturbation. The only data-path collective is the broadcast of each step's payload — all
instances' encoder poses and lines, ≈ E_total × (3 + 6L) doubles — from rank 0 over
RCCL/xGMI (backend "nccl" on ROCm; "gloo" in the CPU tests). The landmark covariances never move.

Payload layout of one step (float64): [encoder (E_total, 3) | lines (E_total, L, 6)], where a line
row is ekf_line {alpha, r, R00, R01, R10, R11} (include/slam_ekf.h).

Resampling is the one step that moves state between ranks: `global_resample_plan` resamples over the
weights of all ranks and `resample_global` carries it out, shipping the instances that change rank as
instance images (slam_ekf.h ekf_export_instances / ekf_import_instances).
"""
from __future__ import annotations

import numpy as np

LINE_FIELDS = 6


def shard(E_total: int, world: int, rank: int) -> tuple[int, int]:
    """(first instance, count) of `rank`: contiguous, sizes differing by at most one."""
    if world < 1 or not 0 <= rank < world:
        raise ValueError("bad rank/world")
    base, extra = divmod(E_total, world)
    first = rank * base + min(rank, extra)
    return first, base + (1 if rank < extra else 0)


def payload_len(E_total: int, L: int) -> int:
    return E_total * 3 + E_total * L * LINE_FIELDS


def pack(encoder: np.ndarray, lines: np.ndarray) -> np.ndarray:
    """encoder (E_total, 3), lines (E_total, L, 6) → flat float64 payload."""
    E = encoder.shape[0]
    if lines.shape[0] != E or lines.shape[2] != LINE_FIELDS:
        raise ValueError("payload shapes")
    return np.concatenate([np.ascontiguousarray(encoder, dtype=np.float64).ravel(),
                           np.ascontiguousarray(lines, dtype=np.float64).ravel()])


def offsets(E_total: int, L: int, first: int) -> tuple[int, int]:
    """Element offsets (not bytes) of a slice's encoder rows and line rows inside a payload."""
    return first * 3, E_total * 3 + first * L * LINE_FIELDS


def unpack_slice(buf, E_total: int, L: int, first: int, count: int):
    """Views of one rank's encoder (count, 3) and lines (count, L, 6) inside a payload (numpy
    array or torch tensor; no copy)."""
    eo, lo = offsets(E_total, L, first)
    enc = buf[eo: eo + count * 3].reshape(count, 3)
    lines = buf[lo: lo + count * L * LINE_FIELDS].reshape(count, L, LINE_FIELDS)
    return enc, lines


def broadcast_step(buf, dist, src: int = 0) -> None:
    """The one exchange of a step: the sensor rank's payload to every rank (in place)."""
    dist.broadcast(buf, src=src)


def broadcast_async(buf, dist, src: int = 0):
    """Same for a group of steps, asynchronously; `.wait()` on the returned work orders the
    caller's current stream after it (NCCL/RCCL) or blocks until it is done (gloo)."""
    return dist.broadcast(buf, src=src, async_op=True)


class GroupedBroadcast:
    """The scan stream of bench.py's multi-rank run: rank `src` holds every step's payload
    (`payload`, shape (steps_total, per_step)); groups of B consecutive steps go out in one
    collective, issued one group ahead of the steps that consume them, into a double-buffered
    receive area. Step s reads row s % B of group s // B:

        gi, k = divmod(s, B)
        k == 0: wait for group gi (NCCL/RCCL: the current stream waits; gloo: blocks), then issue
                group gi + 1 into the other buffer (it overlaps group gi's steps)

    Buffer reuse is ordered by construction: group gi + 1 overwrites the buffer group gi − 1's
    steps read, and those were issued before it (stream order on the GPU; synchronous on CPU).
    `host_coll`: the collective runs on host copies (gloo rehearsal of GPU ranks). `force`: the
    collective path even for a world of one (the RCCL device branch on a one-GPU box)."""

    def __init__(self, payload, B: int, dist, rank: int, world: int, src: int = 0,
                 host_coll: bool = False, sync=None, force: bool = False):
        self.payload, self.B, self.dist = payload, max(1, int(B)), dist
        self.rank, self.world, self.src = rank, world, src
        self.coll = world > 1 or force
        self.steps_total = payload.shape[0]
        self.host_coll, self.sync = host_coll, sync
        self.recv = payload.new_empty((2, self.B, payload.shape[1])) if self.coll else None
        self.inflight = {}
        self.issued = []        # group indices in issue order (tests)

    class _Done:
        def wait(self):
            pass

    def issue(self, gi: int) -> None:
        if not self.coll or gi * self.B >= self.steps_total:
            return
        import torch
        B = self.B
        buf = self.recv[gi & 1]
        cnt = min(B, self.steps_total - gi * B)
        self.issued.append(gi)
        if self.host_coll:
            if self.sync:
                self.sync()     # the previous user of this buffer is done
            hb = (self.payload[gi * B: gi * B + cnt].cpu() if self.rank == self.src
                  else torch.empty((cnt, self.payload.shape[1]), dtype=self.payload.dtype))
            broadcast_step(hb, self.dist, src=self.src)
            buf[:cnt].copy_(hb[:cnt].to(buf.device))
            self.inflight[gi] = self._Done()
            return
        if self.rank == self.src:
            buf[:cnt].copy_(self.payload[gi * B: gi * B + cnt], non_blocking=True)
        self.inflight[gi] = broadcast_async(buf, self.dist, src=self.src)

    def start(self) -> None:
        self.issue(0)

    def step_buffer(self, s: int):
        """The payload row step s consumes (a view into the receive area for world > 1)."""
        if not self.coll:
            return self.payload[s]
        gi, k = divmod(s, self.B)
        if k == 0:
            self.inflight.pop(gi).wait()
            self.issue(gi + 1)
        return self.recv[gi & 1][k]


def global_resample_plan(weights, u: float, counts):
    """Systematic resampling over the concatenated weights of all ranks; counts[r] instances on rank
    r. Returns (local, transfers): local[r] is a src list Ensemble.resample accepts on rank r, and
    transfers a list of (src_rank, src_e, dst_rank, dst_e), local indices, for the instances that
    change rank. The copies per instance are those of ekf.resample_plan on the concatenated weights.
    Every source is a survivor that keeps its slot. The dead slots of a rank take that rank's own
    surplus copies first (ascending slots, ascending survivors), so only the surplus a rank cannot
    place, max(0, c_r - counts[r]) with c_r the copies its sources are owed, crosses ranks: the lower
    bound. A slot a transfer fills keeps itself in the local list (the import writes it)."""
    from .ekf import resample_plan
    counts = [int(c) for c in counts]
    if any(c < 0 for c in counts):
        raise ValueError("global_resample_plan: a negative count")
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    if w.size != sum(counts):
        raise ValueError(f"global_resample_plan: {w.size} weights for {sum(counts)} instances")
    src = resample_plan(w, u)
    copies = np.bincount(np.asarray(src, dtype=np.int64), minlength=w.size)
    local, left, holes = [], [], []
    first = 0
    for r, cnt in enumerate(counts):
        n = copies[first: first + cnt]
        lst = list(range(cnt))
        surplus = [e for e in range(cnt) for _ in range(int(n[e]) - 1)]
        dead = [e for e in range(cnt) if n[e] == 0]
        for slot, e in zip(dead, surplus):
            lst[slot] = e
        k = min(len(dead), len(surplus))
        left += [(r, e) for e in surplus[k:]]
        holes += [(r, e) for e in dead[k:]]
        local.append(lst)
        first += cnt
    assert len(left) == len(holes)   # (the copies sum to the number of instances)
    transfers = [(sr, se, dr, de) for (sr, se), (dr, de) in zip(left, holes)]
    return local, transfers


def resample_global(ens, weights_local, u: float, dist, rank: int, world: int, host_coll: bool = False):
    """One resampling step over the ensemble of all ranks. Every rank calls it at the same point of
    the scan stream (ranks in lockstep are congruent), with the weights of its own instances and the
    same u. The weights are all-gathered and the plan built on every rank; the instances that change
    rank are exported, exchanged with batched isend / irecv in transfer-list order (an image and its
    descriptor per transfer) and imported, and the local list goes to ens.resample. Device tensors on
    nccl; host arrays with host_coll (gloo, as GroupedBroadcast). Sources are never overwritten, so
    export, import and the local copies need no order among themselves beyond send before receive.
    Nothing here drains the context (Ensemble.sync would). On nccl the context must therefore run on
    torch's current stream (Ensemble.set_stream, once, before the first step, as bench.py does): the
    export, the collective, the import and the release of the buffers are then in stream order.
    Returns (local list of this rank, transfers)."""
    import ctypes

    import torch

    from .ekf import EkfImageDesc
    gathered = [None] * world
    dist.all_gather_object(gathered, [float(x) for x in np.asarray(weights_local, dtype=np.float64).reshape(-1)])
    counts = [len(g) for g in gathered]
    local, transfers = global_resample_plan(np.concatenate([np.asarray(g, dtype=np.float64) for g in gathered]), u,
                                            counts)
    out = [t for t in transfers if t[0] == rank]
    inc = [t for t in transfers if t[2] == rank]
    nbytes = int(ens.instance_image_bytes())
    dsz = ctypes.sizeof(EkfImageDesc)
    if host_coll:
        dev = torch.device("cpu")
    else:
        dev = torch.device("cuda", torch.cuda.current_device())
    send_img = recv_img = None
    send_desc = torch.zeros((len(out), dsz), dtype=torch.uint8)
    if out:
        if host_coll:
            descs, images = ens.export_instances([t[1] for t in out])
            send_img = torch.from_numpy(images)
        else:
            send_img = torch.empty((len(out), nbytes), dtype=torch.uint8, device=dev)
            descs = ens.export_instances_device([t[1] for t in out], send_img.data_ptr())
        for k, d in enumerate(descs):
            send_desc[k] = torch.frombuffer(bytearray(bytes(d)), dtype=torch.uint8)
    send_desc = send_desc.to(dev)
    recv_desc = torch.zeros((len(inc), dsz), dtype=torch.uint8, device=dev)
    if inc:
        recv_img = torch.empty((len(inc), nbytes), dtype=torch.uint8, device=dev)
    ops, ko, ki = [], 0, 0
    for sr, _se, dr, _de in transfers:
        if sr == rank:
            ops += [dist.P2POp(dist.isend, send_img[ko], dr), dist.P2POp(dist.isend, send_desc[ko], dr)]
            ko += 1
        elif dr == rank:
            ops += [dist.P2POp(dist.irecv, recv_img[ki], sr), dist.P2POp(dist.irecv, recv_desc[ki], sr)]
            ki += 1
    if ops:
        for req in dist.batch_isend_irecv(ops):
            req.wait()
    if inc:
        raw = recv_desc.cpu().numpy()
        descs = [EkfImageDesc.from_buffer_copy(raw[k].tobytes()) for k in range(len(inc))]
        slots = [t[3] for t in inc]
        if host_coll:
            ens.import_instances(slots, recv_img.numpy(), descs)
        else:
            ens.import_instances_device(slots, recv_img.data_ptr(), descs)
    ens.resample(local[rank])
    return local[rank], transfers
