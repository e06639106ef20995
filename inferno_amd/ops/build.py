"""In-tree build of the HIP kernel library for gfx950.

The library is a standalone hipcc shared object with a C ABI (no torch
headers) — loaded via ctypes and driven on torch's current HIP stream with
raw device pointers. Building in-tree (not a JIT cache) is deliberate: the
.so travels with the repo snapshot to GPU boxes.

A second library, the probe build, is the same sources compiled with
-DWVA_CHAIN_PROBE: it adds the chain probe (ops.sweep.run_chain_probe), whose
instantiations would change the code of every other kernel if they shared a
module with them (docs/design/kernels.md, "Chain probe"). Only tests and tools
load it.
"""
from __future__ import annotations

import os
import subprocess
import sys

OPS_DIR = os.path.dirname(os.path.abspath(__file__))
HIP_SRC = os.path.join(OPS_DIR, "hip", "wva_kernels.hip")
# host-only native sources linked into the same .so (C++ runtime pieces:
# the sequential greedy tail of limited mode; the reconcile tick's host
# staging and by-type aggregation)
NATIVE_SRCS = [
    os.path.join(OPS_DIR, "native", "greedy.cpp"),
    os.path.join(OPS_DIR, "native", "stage.cpp"),
]
# files the sources above include (a newer one makes the library stale): the
# context runtime is part of HIP_SRC's translation unit
NATIVE_HDRS = [
    os.path.join(OPS_DIR, "hip", "wva_ctx.inc"),
    os.path.join(OPS_DIR, "hip", "wva_lag.inc"),
    os.path.join(OPS_DIR, "hip", "wva_lag_path.inc"),
    os.path.join(OPS_DIR, "hip", "wva_lag_path_avg.inc"),
    os.path.join(OPS_DIR, "hip", "wva_lag_path_wide.inc"),
    os.path.join(OPS_DIR, "hip", "wva_lag_path_avg_wide.inc"),
    os.path.join(OPS_DIR, "native", "wva_stage.h"),
    os.path.join(OPS_DIR, "native", "wva_arena.h"),
]
LIB_DIR = os.path.join(OPS_DIR, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libwva_hip.so")
PROBE_LIB_PATH = os.path.join(LIB_DIR, "libwva_probe.so")

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = os.environ.get("PYTORCH_ROCM_ARCH", "gfx950")


def _stale(path: str) -> bool:
    if not os.path.exists(path):
        return True
    lib_mtime = os.path.getmtime(path)
    return any(
        os.path.getmtime(src) > lib_mtime for src in [HIP_SRC, *NATIVE_SRCS, *NATIVE_HDRS]
    )


def needs_build() -> bool:
    return _stale(LIB_PATH)


def _command(out: str, defines=()) -> list:
    return [
        HIPCC,
        f"--offload-arch={ARCH}",
        "-O3",
        "-std=c++17",
        "-shared",
        "-fPIC",
        # NOTE: no -ffast-math — the sweep relies on IEEE inf handling
        # (block max init at -inf) and exact within-tolerance comparisons.
        "-fno-gpu-rdc",
        *[f"-D{d}" for d in defines],
        HIP_SRC,
        *NATIVE_SRCS,
        "-o",
        out,
    ]


def build(verbose: bool = True, force: bool = False, probe: bool = False) -> str:
    """Compile the HIP kernels for gfx950 (cross-compiles fine without a GPU).
    ``probe``: the probe build as well; the two compile side by side."""
    jobs = []
    if force or needs_build():
        jobs.append(_command(LIB_PATH))
    if probe and (force or _stale(PROBE_LIB_PATH)):
        jobs.append(_command(PROBE_LIB_PATH, ["WVA_CHAIN_PROBE=1"]))
    if jobs:
        os.makedirs(LIB_DIR, exist_ok=True)
    procs = []
    for cmd in jobs:
        if verbose:
            print(f"[inferno_amd.ops.build] {' '.join(cmd)}", file=sys.stderr)
        procs.append(subprocess.Popen(cmd))
    codes = [p.wait() for p in procs]
    for cmd, code in zip(jobs, codes):
        if code != 0:
            raise subprocess.CalledProcessError(code, cmd)
    return LIB_PATH


def build_probe(verbose: bool = True, force: bool = False) -> str:
    """The probe build alone (the kernel library is left as it is)."""
    if force or _stale(PROBE_LIB_PATH):
        os.makedirs(LIB_DIR, exist_ok=True)
        cmd = _command(PROBE_LIB_PATH, ["WVA_CHAIN_PROBE=1"])
        if verbose:
            print(f"[inferno_amd.ops.build] {' '.join(cmd)}", file=sys.stderr)
        subprocess.run(cmd, check=True)
    return PROBE_LIB_PATH


if __name__ == "__main__":
    build(force="--force" in sys.argv, probe=True)
