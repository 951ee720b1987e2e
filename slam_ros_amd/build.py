"""Build the in-tree gfx950 library libslam_ekf.so (hipcc, no torch extension machinery).

The library is the product path: slam_ros_amd/ekf.py loads it with ctypes and fails loudly if
it is missing. Built in-tree so the .so travels to the GPU box with the repository snapshot.
"""
from __future__ import annotations

import hashlib
import json
import os
import shutil
import socket
import subprocess
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
LIB_DIR = os.path.join(HERE, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libslam_ekf.so")
ARCH = "gfx950"


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (ROCm required to build libslam_ekf.so)")


def _file_sha(path: str) -> str:   # (bench.py's lib_sha)
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for blk in iter(lambda: f.read(1 << 20), b""):
            h.update(blk)
    return h.hexdigest()[:16]


def _sha(paths: list[str]) -> str:
    h = hashlib.sha256()
    for p in paths:
        h.update(os.path.basename(p).encode() + b"\0")
        with open(p, "rb") as f:
            for blk in iter(lambda: f.read(1 << 20), b""):
                h.update(blk)
    return h.hexdigest()[:16]


# Build provenance: the library carries a sidecar record of the sources it was
# compiled from (LIB_PATH + ".json": source_sha over the sources, headers and this file, lib_sha of
# the binary). build() reuses the library only when both hashes match — not by file times, which a
# copy of the tree does not keep reliably — and writes what it did to lib/last_build.json
# ("compiled" or "reused", host, time), which bench.py reports as build_mode.
RECORD = LIB_PATH + ".json"
LAST_BUILD = os.path.join(LIB_DIR, "last_build.json")


def _record() -> dict:
    try:
        with open(RECORD) as f:
            return json.load(f)
    except (OSError, ValueError):
        return {}


def last_build() -> dict:
    """The last build() on this copy of the tree, or {"mode": "prebuilt"} when build() never ran
    here (the library as shipped, with its own record)."""
    try:
        with open(LAST_BUILD) as f:
            return json.load(f)
    except (OSError, ValueError):
        rec = _record()
        return {"mode": "prebuilt", "source_sha": rec.get("source_sha"), "lib_sha": rec.get("lib_sha")}


# MFMA accumulators in VGPRs (not AGPRs): the fp16 flush rounds every accumulator after each
# step on the VALU, which cannot read AGPRs, so the AGPR form paid a read + write copy per
# element per step (fp16 flush 0.84 -> 0.72 ms at N=4096, T=8; fp32 unchanged or faster)
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-Wall", "-mllvm", "-amdgpu-mfma-vgpr-form"]
# The compilation units, in link order (the order of the code objects in the library). Each
# unit_*.hip includes the device code its kernels need (the flush units a header per flush family,
# the query unit ekf_device.h alone, the gate unit ekf_gate.h, the joint and search units
# ekf_joint_parts.h above it, the pairs unit ekf_pairs.h, the resample and image units only their tables' headers and the shared
# copy body, the loop unit ekf_loop_plan.h alone, the three scan units the association kernel, ekf_kernels.hip,
# which is not compiled on its own, and unit_shard_pack.hip the partitioned instance's kernels,
# ekf_shard_kernels.h, with ekf_pack.h; those two share ekf_assoc_parts.h)
# and defines the launchers that instantiate them; they compile in parallel with the five host units,
# which define no kernels and share ekf_ctx.h: ekf_api.hip (the context and the schedule), ekf_state.hip
# (state transfers, ellipse), ekf_shard.hip (the partitioned instance, RCCL), ekf_read.hip (queries, gate,
# joint gate, joint search, candidates, weights) and ekf_copy.hip (resample, its plan, images).
UNITS = ["unit_flush_f16x3.hip", "unit_flush_exact.hip", "unit_scan.hip", "unit_scan_nt128.hip",
         "unit_scan_nt64.hip", "unit_flush_2x4.hip", "unit_flush_bf16x6.hip", "unit_shard_pack.hip",
         "unit_flush_quad.hip", "unit_query.hip", "unit_gate.hip", "unit_joint.hip", "unit_assoc.hip",
         "ekf_api.hip", "ekf_state.hip", "ekf_shard.hip", "ekf_read.hip", "ekf_copy.hip",
         "unit_resample.hip", "unit_image.hip", "unit_resample_device.hip", "unit_loop.hip",
         "unit_pairs.hip"]


def source_deps(csrc: str = CSRC) -> list[str]:
    """What the library is built from: every .hip and .h under csrc/, the public header, this file."""
    files = sorted(os.path.join(base, f) for base, _dirs, names in os.walk(csrc)
                   for f in names if f.endswith((".hip", ".h")))
    return files + [os.path.join(ROOT, "include", "slam_ekf.h"), os.path.abspath(__file__)]


def _compile_link(out: str, defines: list[str], verbose: bool = False, csrc: str = CSRC) -> None:
    objdir = out + ".objs"
    os.makedirs(objdir, exist_ok=True)
    procs, objs = [], []
    for src in UNITS:
        obj = os.path.join(objdir, os.path.splitext(src)[0] + ".o")
        cmd = [hipcc(), f"--offload-arch={ARCH}", *FLAGS, *[f"-D{d}" for d in defines],
               "-c", os.path.join(csrc, src), "-o", obj]
        if verbose:
            print(" ".join(cmd))
        procs.append(subprocess.Popen(cmd))
        objs.append(obj)
    if any(p.wait() != 0 for p in procs):
        raise subprocess.CalledProcessError(1, "hipcc (libslam_ekf units)")
    cmd = [hipcc(), f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", out] + objs
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    shutil.rmtree(objdir, ignore_errors=True)


def build_variant(out: str, defines: list[str], csrc: str = CSRC) -> str:
    """An A/B build with extra -D flags, or of a patched copy of csrc/ (scripts only; SLAM_EKF_LIB)."""
    _compile_link(out, defines, csrc=csrc)
    return out


def build(force: bool = False, verbose: bool = False) -> str:
    src = _sha(source_deps())   # (this file among them: the compile flags live here)
    rec = _record()
    reuse = (not force and os.path.exists(LIB_PATH) and rec.get("source_sha") == src
             and rec.get("lib_sha") == _file_sha(LIB_PATH))
    if not reuse:
        os.makedirs(LIB_DIR, exist_ok=True)
        tmp = LIB_PATH + ".tmp"
        _compile_link(tmp, [], verbose)
        os.replace(tmp, LIB_PATH)
        rec = {"source_sha": src, "lib_sha": _file_sha(LIB_PATH), "built_on": socket.gethostname(),
               "built_at": time.strftime("%Y-%m-%dT%H:%M:%S")}
        with open(RECORD, "w") as f:
            json.dump(rec, f)
    last = {"mode": "reused" if reuse else "compiled", "source_sha": src, "lib_sha": rec["lib_sha"],
            "host": socket.gethostname(), "at": time.strftime("%Y-%m-%dT%H:%M:%S")}
    with open(LAST_BUILD, "w") as f:
        json.dump(last, f)
    print(f"libslam_ekf.so: {last['mode']} (source {src}, library {rec['lib_sha']})")
    return LIB_PATH


if __name__ == "__main__":
    print(build(force=True, verbose=True))
