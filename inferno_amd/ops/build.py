"""In-tree build of the HIP kernel library for gfx950.

The library is a standalone hipcc shared object with a C ABI (no torch
headers) — loaded via ctypes and driven on torch's current HIP stream with
raw device pointers. Building in-tree (not a JIT cache) is deliberate: the
.so travels with the repo snapshot to GPU boxes.
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
    os.path.join(OPS_DIR, "native", "wva_stage.h"),
    os.path.join(OPS_DIR, "native", "wva_arena.h"),
]
LIB_DIR = os.path.join(OPS_DIR, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libwva_hip.so")

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = os.environ.get("PYTORCH_ROCM_ARCH", "gfx950")


def needs_build() -> bool:
    if not os.path.exists(LIB_PATH):
        return True
    lib_mtime = os.path.getmtime(LIB_PATH)
    return any(
        os.path.getmtime(src) > lib_mtime for src in [HIP_SRC, *NATIVE_SRCS, *NATIVE_HDRS]
    )


def build(verbose: bool = True, force: bool = False) -> str:
    """Compile the HIP kernels for gfx950 (cross-compiles fine without a GPU)."""
    if not force and not needs_build():
        return LIB_PATH
    os.makedirs(LIB_DIR, exist_ok=True)
    cmd = [
        HIPCC,
        f"--offload-arch={ARCH}",
        "-O3",
        "-std=c++17",
        "-shared",
        "-fPIC",
        # NOTE: no -ffast-math — the sweep relies on IEEE inf handling
        # (block max init at -inf) and exact within-tolerance comparisons.
        "-fno-gpu-rdc",
        HIP_SRC,
        *NATIVE_SRCS,
        "-o",
        LIB_PATH,
    ]
    if verbose:
        print(f"[inferno_amd.ops.build] {' '.join(cmd)}", file=sys.stderr)
    subprocess.run(cmd, check=True)
    return LIB_PATH


if __name__ == "__main__":
    build(force="--force" in sys.argv)
