"""ctypes driver for the HIP allocate-sweep kernels.

Loads the in-tree ``lib/libwva_hip.so`` and launches on torch's current HIP
stream with raw device pointers. On a GPU box a missing/failed native library
raises loudly (no silent eager fallback) — the CPU path must be requested
explicitly via the engine's ``backend="cpu"``.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import Optional

from .build import LIB_PATH, build, build_probe, needs_build

# Mirrors of the native library's constants, by their C names. load_library()
# checks every one against wva_abi() once, so a drift fails loudly at load.
_ABI = {
    "WVA_MAX_N": 8192,  # 64KB-LDS limit
    "WVA_XL_MAX_N": 32768,  # XL LDS tier (default)
    "WVA_HUGE_MAX_N": 1 << 22,  # global-memory spill limit
    "WVA_PLAN_MAX_S": 256,  # scenarios per planning pass
    "WVA_N_SMALL": 512,  # N-bucket thresholds (defaults)
    "WVA_N_MED": 2048,
    "WVA_TICK_STALE": 1 << 20,  # wva_ctx_tick: layout stale, nothing launched
    "WVA_DYN_ROWS": 8,  # rows of the dynamic block
    "WVA_REC_ROWS": 10,  # rows of the winner-record block
    "WVA_MAX_BUCKETS": 5,  # buckets a context holds (choose_buckets' regimes)
}
# the lag analysis' constants (ops/hip/wva_lag.inc), checked the same way
_LAG_ABI = {
    "WVA_LAG_MAX_T": 16,  # checkpoints of a lag analysis
    "WVA_LAG_MAX_N": 1117,  # largest N the widest wva_lag_t instantiation holds
    "WVA_LAG_CLASSES": 4,  # wva_lag_t instantiations
    "WVA_LAG_WIDE_MAX_N": 32768,  # largest N of the tiled path (the XL ceiling)
    "WVA_LAG_WIDE_HALO": 768,  # its production halo T, in slots
}
MAX_N = _ABI["WVA_MAX_N"]
# XL LDS tier: fits CDNA4's 160 KiB LDS with the >64KB dynamic-LDS opt-in;
# override to MAX_N to force such cells to GMEM
XL_MAX_N = int(os.environ.get("INFERNO_XL_MAX_N", _ABI["WVA_XL_MAX_N"]))
HUGE_MAX_N = _ABI["WVA_HUGE_MAX_N"]
PLAN_MAX_S = _ABI["WVA_PLAN_MAX_S"]
# N-bucket thresholds: cells are dispatched to 64- and 256-thread blocks by
# batch size — widths picked by A/B measurement on MI355X (see
# choose_buckets); small/medium cells run one barrier-free wave each, large-N
# cells get 4-wave blocks. The env overrides are deliberate (A/B tuning).
N_SMALL = int(os.environ.get("INFERNO_N_SMALL", _ABI["WVA_N_SMALL"]))
N_MED = int(os.environ.get("INFERNO_N_MED", _ABI["WVA_N_MED"]))
# the tick code of wva_ctx_tick for "the bucket layout does not fit the staged
# batch_n, nothing was launched", and the block shapes of ops/native/wva_stage.h
TICK_STALE = _ABI["WVA_TICK_STALE"]
DYN_ROWS = _ABI["WVA_DYN_ROWS"]
REC_ROWS = _ABI["WVA_REC_ROWS"]
MAX_BUCKETS = _ABI["WVA_MAX_BUCKETS"]
LAG_MAX_T = _LAG_ABI["WVA_LAG_MAX_T"]
LAG_MAX_N = _LAG_ABI["WVA_LAG_MAX_N"]
# wva_lag_t<NT, C> instantiations in launch order (widest first): lane l holds C
# states in registers, so a class takes 11 N + 1 <= NT * C
LAG_CLASSES = ((512, 24), (256, 12), (64, 12), (64, 2))
# the tiled path above LAG_MAX_N (wva_lag_tile_t<512, 24>): a tile loads
# LAG_WIDE_W slots, T of them halo on each side, and owns S = W - 2 T
LAG_WIDE_MAX_N = _LAG_ABI["WVA_LAG_WIDE_MAX_N"]
LAG_WIDE_C = 24
LAG_WIDE_W = 512 * LAG_WIDE_C
LAG_WIDE_HALO = _LAG_ABI["WVA_LAG_WIDE_HALO"]
LAG_WIDE_STRIDE = LAG_WIDE_W - 2 * LAG_WIDE_HALO
LAG_SEG_FIRST, LAG_SEG_LAST, LAG_SEG_FINAL = 1, 2, 4


def choose_buckets(batch_n):
    """Partition cells into N-buckets and pick each bucket's block size.

    The natural guess — wide blocks shorten a single cell's latency — is
    WRONG on CDNA4 for this kernel (measured, profiles/REPORT.md): per-eval
    cost is dominated by the redundant per-lane work, which costs
    waves-per-SIMD x instructions, while the serial chain states are cheap
    fp32-LDS FMAs. Narrow blocks therefore win in BOTH regimes.

    Cells with MAX_N < N <= XL_MAX_N use the XL tier: still LDS-resident via
    the 160 KiB dynamic-LDS opt-in (one workgroup per CU, fine for the rare
    huge cells). Cells above XL_MAX_N go to the global-memory bucket: their
    chain geometry lives in a per-block HBM slab instead of LDS (GMEM kernel
    instantiation). Either way the sweep is uncapped like the reference
    (allocation.go:80-86).

    Returns [(nt, cell_idx int32 array or None, bucket_max_n, count, gmem)].
    """
    import numpy as np

    n = len(batch_n)
    masks = [
        (64, batch_n <= N_SMALL),
        (256, (batch_n > N_SMALL) & (batch_n <= N_MED)),
        (1024, (batch_n > N_MED) & (batch_n <= MAX_N)),
        ("xl", (batch_n > MAX_N) & (batch_n <= XL_MAX_N)),
        ("huge", batch_n > XL_MAX_N),
    ]
    out = []
    for base_nt, mask in masks:
        idx = np.nonzero(mask)[0]
        count = len(idx)
        if count == 0:
            continue
        if base_nt == "xl":
            nt = int(os.environ.get("INFERNO_NT_XL", "256"))
            ids = None if count == n else idx.astype(np.int32)
            out.append((nt, ids, int(batch_n[mask].max()), count, False))
            continue
        if base_nt == "huge":
            bmax = int(batch_n[mask].max())
            if bmax > HUGE_MAX_N:
                raise HipKernelError(
                    f"batch size {bmax} exceeds the global-memory sweep limit "
                    f"{HUGE_MAX_N} (per-cell geometry would be "
                    f"{bmax * 4 / 1e6:.0f}+ MB)"
                )
            nt = int(os.environ.get("INFERNO_NT_HUGE", "256"))
            ids = None if count == n else idx.astype(np.int32)
            out.append((nt, ids, bmax, count, True))
            continue
        # Measured on MI355X (profiles/REPORT.md, 512-model fleet A/B): the
        # per-eval cost of a bisection step is dominated by the REDUNDANT
        # per-lane work (log/exp/expm1 of the tail, loop headers) which costs
        # waves-per-SIMD x instructions — 16-wave blocks pay 4x what 4-wave
        # blocks pay — while the serial per-lane chain states are cheap fp32
        # LDS FMAs. So each bucket wants the NARROWEST block whose serial
        # states/lane stay modest (~64): N<=512 -> 64 threads, N<=2048 -> 64
        # (66 states/lane), N<=8192 -> 256 (66 states/lane). 1024-thread
        # blocks lost 25-43% end-to-end in the A/B (ab_large_*/ab2_* runs).
        nt = {64: 64, 256: 64, 1024: 256}[base_nt]
        # measurement override (A/B tuning): INFERNO_NT_SMALL/_MED/_LARGE
        env = os.environ.get(
            {64: "INFERNO_NT_SMALL", 256: "INFERNO_NT_MED", 1024: "INFERNO_NT_LARGE"}[base_nt]
        )
        if env:
            nt = int(env)
        ids = None if count == n else idx.astype(np.int32)
        out.append((nt, ids, int(batch_n[mask].max()), count, False))
    # launch order = descending max_n (most expensive bucket first): ROCm
    # multiplexes streams onto GPU_MAX_HW_QUEUES (default 4) hardware queues,
    # so with 5 buckets the later streams share a queue and serialize —
    # measured: the XL bucket queued behind the large bucket, costing ~250us
    # of lost overlap per reconcile. Put the stragglers on distinct queues
    # and let the cheap buckets share.
    out.sort(key=lambda b: -b[2])
    return out


def alloc_gmem_slabs(n_blocks: int, max_n: int, nt: int, device: str):
    """Allocate the global-memory geometry slabs for a huge-N bucket:
    per-block chunk-transposed fp32 reciprocals + fp64 anchor log-prefixes
    (the same layout the LDS path uses)."""
    import torch

    chunk = (max_n + nt - 1) // nt
    ksub = (chunk + 31) // 32
    g_inv = torch.empty((n_blocks, chunk * nt), dtype=torch.float32, device=device)
    g_anchor = torch.empty((n_blocks, nt * ksub), dtype=torch.float64, device=device)
    return g_inv, g_anchor

def gmem_slab_bytes(max_n: int, nt: int) -> int:
    """Bytes of one block's slabs as alloc_gmem_slabs lays them out."""
    chunk = (max_n + nt - 1) // nt
    ksub = (chunk + 31) // 32
    return chunk * nt * 4 + nt * ksub * 8


def _lag_task_dtype():
    import numpy as np

    return np.dtype([("in_tok", "<i4"), ("out_tok", "<i4"), ("N", "<i4"), ("slot", "<i4"),
                     ("alpha", "<f4"), ("beta", "<f4"), ("gamma", "<f4"), ("delta", "<f4"),
                     ("t_ttft", "<f4"), ("t_itl", "<f4"), ("pad", "<i4", (2,)),
                     ("lam0", "<f8"), ("lam1", "<f8")])


def _lag_wide_dtypes():
    import numpy as np

    return (np.dtype([("Lam", "<f8"), ("slab", "<i8"), ("tile0", "<i4"), ("n_tiles", "<i4"),
                      ("seg0", "<i4"), ("n_seg", "<i4")]),
            np.dtype([("x", "<f8"), ("first", "<i4"), ("count", "<i4"), ("jlo", "<i4"),
                      ("jhi", "<i4"), ("flags", "<i4"), ("j", "<i4")]),
            np.dtype([("task", "<i4"), ("b", "<i4")]))


# one (held cell, scenario) slice of a lag pass: WvaLagTask, 64 bytes
LAG_TASK_DTYPE = _lag_task_dtype()
assert LAG_TASK_DTYPE.itemsize == 64
# the wide path's per-task record, segment and tile: WvaLagWideTask, WvaLagSeg, WvaLagTile
LAG_WIDE_DTYPE, LAG_SEG_DTYPE, LAG_TILE_DTYPE = _lag_wide_dtypes()
assert (LAG_WIDE_DTYPE.itemsize, LAG_SEG_DTYPE.itemsize, LAG_TILE_DTYPE.itemsize) == (32, 32, 8)



def _lag_path_dtypes():
    import numpy as np

    return (np.dtype([("in_tok", "<i4"), ("out_tok", "<i4"), ("N", "<i4"), ("slot", "<i4"),
                      ("alpha", "<f4"), ("beta", "<f4"), ("gamma", "<f4"), ("delta", "<f4"),
                      ("t_ttft", "<f4"), ("t_itl", "<f4"), ("pad", "<i4", (2,)),
                      ("lam0", "<f8"), ("carry", "<i8")]),
            np.dtype([("task", "<i4"), ("tick0", "<i4"), ("n", "<i4"), ("flags", "<i4")]))


# a lag path's run and the ticks of it one launch covers: WvaLagPathTask, WvaLagPathRec
LAG_PATH_TASK_DTYPE, LAG_PATH_REC_DTYPE = _lag_path_dtypes()
assert (LAG_PATH_TASK_DTYPE.itemsize, LAG_PATH_REC_DTYPE.itemsize) == (64, 16)
# WvaLagPathRec.flags: how the vector starts, and whether it is stored at the end
LAG_PATH_STATIONARY, LAG_PATH_EMPTY, LAG_PATH_CARRY, LAG_PATH_STORE = 0, 1, 2, 4
LAG_PATH_SLAB_CAP = 1 << 30  # bytes of carry of one round (WVA_LAG_WIDE_SLAB_CAP)


def _lag_path_wide_dtype():
    import numpy as np

    return np.dtype([("smax", "<f8"), ("slab", "<i8"), ("tile0", "<i4"), ("n_tiles", "<i4"),
                     ("seg0", "<i4"), ("n_seg", "<i4"), ("tick0", "<i4"), ("n_run", "<i4"),
                     ("start", "<i4"), ("pad", "<i4")])


# a wide run beside its LAG_PATH_TASK_DTYPE record: WvaLagPathWideTask, 48 bytes
LAG_PATH_WIDE_DTYPE = _lag_path_wide_dtype()
assert LAG_PATH_WIDE_DTYPE.itemsize == 48

_lib: Optional[ctypes.CDLL] = None


class HipKernelError(RuntimeError):
    pass


def load_library(allow_build: bool = True) -> ctypes.CDLL:
    """dlopen the kernel library (building it first if sources are newer)."""
    global _lib
    if _lib is not None:
        return _lib
    if needs_build():
        if not allow_build:
            raise HipKernelError(
                f"HIP kernel library missing or stale at {LIB_PATH}; "
                "run python -m inferno_amd.ops.build"
            )
        build()
    lib = ctypes.CDLL(LIB_PATH)
    lib.wva_abi.restype = ctypes.c_int
    lib.wva_abi.argtypes = [ctypes.c_char_p]
    for name, mirror in list(_ABI.items()) + list(_LAG_ABI.items()):
        native = lib.wva_abi(name.encode())
        if native != mirror:
            raise HipKernelError(
                f"{name} is {native} in {LIB_PATH} but {mirror} in ops/sweep.py: "
                "the library and the Python package are out of step"
            )
    lib.wva_sweep_launch_bucket.restype = ctypes.c_int
    lib.wva_argmin_launch.restype = ctypes.c_int
    lib.wva_device_count.restype = ctypes.c_int
    lib.wva_ctx_create.restype = ctypes.c_void_p
    lib.wva_ctx_create.argtypes = [ctypes.c_int, ctypes.c_int,
                                   ctypes.POINTER(ctypes.c_void_p)]
    lib.wva_ctx_set_buckets.restype = ctypes.c_int
    lib.wva_ctx_set_buckets.argtypes = [
        ctypes.c_void_p,
        ctypes.c_int,
        ctypes.POINTER(ctypes.c_int),
        ctypes.POINTER(ctypes.c_void_p),
        ctypes.POINTER(ctypes.c_int),
        ctypes.POINTER(ctypes.c_int),
        ctypes.c_int,
        ctypes.c_float,
        ctypes.POINTER(ctypes.c_void_p),  # per-bucket g_inv slabs (huge-N)
        ctypes.POINTER(ctypes.c_void_p),  # per-bucket g_anchor slabs
        ctypes.c_void_p,  # host i32 [n_cells] batch_n the layout was chosen for
    ]
    lib.wva_reconcile.restype = ctypes.c_int
    lib.wva_reconcile.argtypes = [ctypes.c_void_p]
    # the reconcile tick's native prologue (engine/fastpath.py)
    lib.wva_ctx_set_topology.restype = ctypes.c_int
    lib.wva_ctx_set_topology.argtypes = [ctypes.c_void_p] * 6
    lib.wva_ctx_tick.restype = ctypes.c_int
    lib.wva_ctx_tick.argtypes = [ctypes.c_void_p] * 8 + [ctypes.c_int]
    # host-only staging and aggregation (ops/native/stage.cpp)
    lib.wva_stage_dynamic.restype = ctypes.c_int
    lib.wva_stage_dynamic.argtypes = (
        [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 14
        + [ctypes.POINTER(ctypes.c_int)]
    )
    lib.wva_aggregate_by_type.restype = ctypes.c_int
    lib.wva_aggregate_by_type.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 9
    lib.wva_greedy_solve.restype = ctypes.c_int
    lib.wva_ctx_destroy.restype = None
    lib.wva_ctx_destroy.argtypes = [ctypes.c_void_p]
    lib.wva_ctx_memo_stats.restype = ctypes.c_int
    lib.wva_ctx_memo_stats.argtypes = [
        ctypes.c_void_p,
        ctypes.POINTER(ctypes.c_uint),  # hits
        ctypes.POINTER(ctypes.c_uint),  # misses
    ]
    # fused tick diagnostics (engine/native_ctx.py NativeCtx.fused_state)
    lib.wva_ctx_fused_state.restype = ctypes.c_int
    lib.wva_ctx_fused_state.argtypes = [
        ctypes.c_void_p,
        ctypes.POINTER(ctypes.c_int),  # out: info[8]
        ctypes.POINTER(ctypes.c_int),  # out: done[] words that are not 0
    ]
    # scenario planning (engine/fastpath.py FastSweep.plan)
    lib.wva_ctx_plan.restype = ctypes.c_int
    lib.wva_ctx_plan.argtypes = [
        ctypes.c_void_p,
        ctypes.c_int,  # n_scen (1..PLAN_MAX_S)
        ctypes.c_int,  # n_acc
        ctypes.c_void_p,  # host fp32 [n_scen][n_cells] arrival rates
        ctypes.POINTER(ctypes.c_void_p),  # out: pinned fp32 [n_scen][6][n_srv]
        ctypes.POINTER(ctypes.c_void_p),  # out: pinned i32 [n_scen][4][n_srv]
        ctypes.POINTER(ctypes.c_void_p),  # out: pinned u64 [n_scen][n_acc]
    ]
    # SLO planning (engine/fastpath.py FastSweep.plan_slo)
    lib.wva_ctx_plan_slo.restype = ctypes.c_int
    lib.wva_ctx_plan_slo.argtypes = [
        ctypes.c_void_p,
        ctypes.c_int,  # n_tgt
        ctypes.c_int,  # n_scen = n_tgt * n_load (1..PLAN_MAX_S)
        ctypes.c_int,  # n_acc
        ctypes.c_void_p,  # host fp32 [n_load][n_cells] arrival rates
        ctypes.c_void_p,  # host fp32 [n_tgt][n_cells] TTFT targets
        ctypes.c_void_p,  # host fp32 [n_tgt][n_cells] ITL targets
        ctypes.POINTER(ctypes.c_void_p),  # out: pinned fp32 [n_scen][6][n_srv]
        ctypes.POINTER(ctypes.c_void_p),  # out: pinned i32 [n_scen][4][n_srv]
        ctypes.POINTER(ctypes.c_void_p),  # out: pinned u64 [n_scen][n_acc]
    ]
    # percentile planning (engine/fastpath.py FastSweep.plan_tail)
    lib.wva_ctx_plan_tail.restype = ctypes.c_int
    lib.wva_ctx_plan_tail.argtypes = [
        ctypes.c_void_p,
        ctypes.c_int,  # n_q (1..8)
        ctypes.c_int,  # n_scen = n_q * n_load (1..PLAN_MAX_S)
        ctypes.c_int,  # n_acc
        ctypes.c_void_p,  # host fp32 [n_load][n_cells] arrival rates
        ctypes.c_void_p,  # host fp64 [n_q] 1 - q
        ctypes.POINTER(ctypes.c_void_p),  # out: pinned fp32 [n_scen][6][n_srv]
        ctypes.POINTER(ctypes.c_void_p),  # out: pinned i32 [n_scen][4][n_srv]
        ctypes.POINTER(ctypes.c_void_p),  # out: pinned u64 [n_scen][n_acc]
        ctypes.POINTER(ctypes.c_void_p),  # out: pinned fp32 [n_scen][n_srv] wait_tail
    ]
    lib.wva_ctx_plan_tail_cells.restype = ctypes.c_int
    lib.wva_ctx_plan_tail_cells.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.wva_tail_probe_launch.restype = ctypes.c_int
    lib.wva_tail_probe_launch.argtypes = (
        [ctypes.c_int] * 3 + [ctypes.c_void_p] * 11 + [ctypes.c_int] + [ctypes.c_void_p] * 3
        + [ctypes.c_int] + [ctypes.c_void_p] * 5
    )
    # token-mix planning (engine/fastpath.py FastSweep.plan_tokens)
    lib.wva_ctx_plan_tokens.restype = ctypes.c_int
    lib.wva_ctx_plan_tokens.argtypes = [
        ctypes.c_void_p,
        ctypes.c_int,  # n_tok
        ctypes.c_int,  # n_scen = n_tok * n_load (1..PLAN_MAX_S)
        ctypes.c_int,  # n_acc
        ctypes.c_void_p,  # host fp32 [n_load][n_cells] arrival rates
        ctypes.c_void_p,  # host i32 [n_tok][n_cells] in_tok
        ctypes.c_void_p,  # host i32 [n_tok][n_cells] out_tok
        ctypes.c_void_p,  # host i32 [n_tok][n_cells] batch_n
        ctypes.c_int,  # task buckets of the pass
        ctypes.POINTER(ctypes.c_int),  # per bucket: block width
        ctypes.POINTER(ctypes.c_void_p),  # device i32 task ids (null: every task)
        ctypes.POINTER(ctypes.c_int),  # tasks
        ctypes.POINTER(ctypes.c_int),  # largest N
        ctypes.POINTER(ctypes.c_void_p),  # g_inv slabs (huge-N)
        ctypes.POINTER(ctypes.c_void_p),  # g_anchor slabs
        ctypes.POINTER(ctypes.c_int),  # tasks per launch (0: all)
        ctypes.POINTER(ctypes.c_void_p),  # out: pinned fp32 [n_scen][6][n_srv]
        ctypes.POINTER(ctypes.c_void_p),  # out: pinned i32 [n_scen][4][n_srv]
        ctypes.POINTER(ctypes.c_void_p),  # out: pinned u64 [n_scen][n_acc]
    ]
    # forecast rollout (engine/fastpath.py FastSweep.rollout)
    lib.wva_ctx_rollout.restype = ctypes.c_int
    lib.wva_ctx_rollout.argtypes = [
        ctypes.c_void_p,
        ctypes.c_int,  # n_steps (1..PLAN_MAX_S)
        ctypes.c_int,  # n_acc
        ctypes.c_void_p,  # host fp32 [n_steps][n_cells] arrival rates
        ctypes.c_void_p,  # host i32 [n_srv] cur_acc the chain starts from
        ctypes.c_void_p,  # host i32 [n_srv] cur_rep
        ctypes.c_void_p,  # host fp32 [n_srv] cur_cost
        ctypes.POINTER(ctypes.c_void_p),  # out: pinned fp32 [n_steps][6][n_srv]
        ctypes.POINTER(ctypes.c_void_p),  # out: pinned i32 [n_steps][4][n_srv]
        ctypes.POINTER(ctypes.c_void_p),  # out: pinned u64 [n_steps][n_acc]
        ctypes.POINTER(ctypes.c_void_p),  # out: pinned i32 [3][n_srv] final allocation
    ]
    # forecast ensembles (engine/fastpath.py FastSweep.rollout_ensemble)
    lib.wva_ctx_ensemble_pass.restype = ctypes.c_int
    lib.wva_ctx_ensemble_pass.argtypes = [
        ctypes.c_void_p,
        ctypes.c_int,  # paths of the ensemble (1..256)
        ctypes.c_int,  # n_steps (1..PLAN_MAX_S)
        ctypes.c_int,  # quantiles (1..8)
        ctypes.c_int,  # n_acc
        ctypes.c_int,  # first path of this pass
        ctypes.c_int,  # paths of this pass (paths * n_steps <= PLAN_MAX_S)
        ctypes.c_void_p,  # host fp32 [paths * n_steps][n_cells] arrival rates
        ctypes.c_void_p,  # host i32 [n_srv] cur_acc every path starts from
        ctypes.c_void_p,  # host i32 [n_srv] cur_rep
        ctypes.c_void_p,  # host fp32 [n_srv] cur_cost
        ctypes.c_int,  # write and download the pass's records
        ctypes.POINTER(ctypes.c_void_p),  # out: pinned fp32 [paths * n_steps][6][n_srv]
        ctypes.POINTER(ctypes.c_void_p),  # out: pinned i32 [paths * n_steps][4][n_srv]
    ]
    lib.wva_ctx_ensemble_bands.restype = ctypes.c_int
    lib.wva_ctx_ensemble_bands.argtypes = [
        ctypes.c_void_p,
        ctypes.c_void_p,  # host i32 [n_q] ranks
        ctypes.c_int,  # n_q
        ctypes.c_int,  # download the final allocations too
        ctypes.POINTER(ctypes.c_void_p),  # out: ten pinned result buffers
    ]
    # hold analysis (engine/fastpath.py FastSweep.hold)
    lib.wva_ctx_hold.restype = ctypes.c_int
    lib.wva_ctx_hold.argtypes = [
        ctypes.c_void_p,
        ctypes.c_int,  # n_scen (1..PLAN_MAX_S)
        ctypes.c_int,  # n_acc
        ctypes.c_void_p,  # host fp32 [n_scen][n_cells] arrival rates
        ctypes.c_void_p,  # host i32 [n_scen][n_cells] held replicas (-1: not held)
        ctypes.POINTER(ctypes.c_void_p),  # out: pinned fp32 [n_scen][6][n_srv]
        ctypes.POINTER(ctypes.c_void_p),  # out: pinned i32 [n_scen][4][n_srv]
        ctypes.POINTER(ctypes.c_void_p),  # out: pinned u64 [n_scen][6] status counts
        ctypes.POINTER(ctypes.c_void_p),  # out: pinned u64 [n_scen][n_acc] deficits
    ]
    # lag analysis (engine/fastpath.py FastSweep.lag)
    lib.wva_ctx_lag.restype = ctypes.c_int
    lib.wva_ctx_lag.argtypes = [
        ctypes.c_void_p,
        ctypes.c_int,  # n_tasks
        ctypes.c_void_p,  # host LAG_TASK_DTYPE [n_tasks], grouped by class
        ctypes.c_void_p,  # host i32 [4] tasks per class
        ctypes.c_int,  # n_times (1..16)
        ctypes.c_void_p,  # host fp64 [n_times] interval lengths (msec)
        ctypes.c_int,  # n_slots = scenarios * servers
        ctypes.c_int,  # max_steps
        ctypes.POINTER(ctypes.c_void_p),  # out: pinned fp32 [6][n_times][n_slots]
        ctypes.POINTER(ctypes.c_void_p),  # out: pinned u8 [n_times][n_slots] violated
        ctypes.POINTER(ctypes.c_void_p),  # out: pinned i32 [n_slots] steps
    ]
    lib.wva_lag_probe_launch.restype = ctypes.c_int
    lib.wva_lag_probe_launch.argtypes = (
        [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
        + [ctypes.c_void_p] * 5
    )
    # wide lag (FastSweep.lag(max_n=...)): the four tables of lag_wide_schedule,
    # dt, their five lengths and extents, max_steps, stride, halo
    lib.wva_ctx_lag_wide.restype = ctypes.c_int
    lib.wva_ctx_lag_wide.argtypes = (
        [ctypes.c_void_p] * 6 + [ctypes.c_int] * 8 + [ctypes.POINTER(ctypes.c_void_p)] * 3
    )
    lib.wva_lag_wide_probe_launch.restype = ctypes.c_int
    lib.wva_lag_wide_probe_launch.argtypes = (
        [ctypes.c_void_p] * 5 + [ctypes.c_int] * 8 + [ctypes.c_void_p, ctypes.c_void_p,
                                                      ctypes.c_size_t,
                                                      ctypes.POINTER(ctypes.c_size_t),
                                                      ctypes.POINTER(ctypes.c_size_t)]
    )
    # lag paths (FastSweep.lag_path): the four tables of lag_path_schedule, their
    # lengths and extents, max_steps, dt
    lib.wva_ctx_lag_path.restype = ctypes.c_int
    lib.wva_ctx_lag_path.argtypes = (
        [ctypes.c_void_p] * 5 + [ctypes.c_int] * 6 + [ctypes.c_double]
        + [ctypes.POINTER(ctypes.c_void_p)] * 3
    )
    lib.wva_lag_path_probe_launch.restype = ctypes.c_int
    lib.wva_lag_path_probe_launch.argtypes = (
        [ctypes.c_void_p] * 4 + [ctypes.c_int] * 6 + [ctypes.c_double, ctypes.c_void_p,
                                                      ctypes.c_void_p, ctypes.c_size_t,
                                                      ctypes.POINTER(ctypes.c_size_t),
                                                      ctypes.POINTER(ctypes.c_size_t)]
    )
    # lag path averages (FastSweep.lag_path(averages=True)): as above, with the
    # averaged records and verdicts as two more outputs
    lib.wva_ctx_lag_path_avg.restype = ctypes.c_int
    lib.wva_ctx_lag_path_avg.argtypes = (
        list(lib.wva_ctx_lag_path.argtypes) + [ctypes.POINTER(ctypes.c_void_p)] * 2
    )
    lib.wva_lag_path_avg_probe_launch.restype = ctypes.c_int
    lib.wva_lag_path_avg_probe_launch.argtypes = lib.wva_lag_path_probe_launch.argtypes
    # wide lag paths (FastSweep.lag_path(max_n=...)): the four tables of
    # lag_path_wide_schedule, the descriptors, their lengths and extents,
    # max_steps, stride, halo, dt
    lib.wva_ctx_lag_path_wide.restype = ctypes.c_int
    lib.wva_ctx_lag_path_wide.argtypes = (
        [ctypes.c_void_p] * 6 + [ctypes.c_int] * 8 + [ctypes.c_double]
        + [ctypes.POINTER(ctypes.c_void_p)] * 3 + [ctypes.c_void_p]
    )
    lib.wva_lag_path_wide_probe_launch.restype = ctypes.c_int
    lib.wva_lag_path_wide_probe_launch.argtypes = (
        [ctypes.c_void_p] * 5 + [ctypes.c_int] * 8 + [ctypes.c_double, ctypes.c_void_p,
                                                      ctypes.c_void_p, ctypes.c_size_t,
                                                      ctypes.POINTER(ctypes.c_size_t),
                                                      ctypes.POINTER(ctypes.c_size_t)]
    )
    # wide lag path averages (FastSweep.lag_path(max_n=..., averages=True)): as
    # above, with the averaged records and verdicts as two more outputs
    lib.wva_ctx_lag_path_wide_avg.restype = ctypes.c_int
    lib.wva_ctx_lag_path_wide_avg.argtypes = (
        list(lib.wva_ctx_lag_path_wide.argtypes) + [ctypes.POINTER(ctypes.c_void_p)] * 2
    )
    lib.wva_lag_path_avg_wide_probe_launch.restype = ctypes.c_int
    lib.wva_lag_path_avg_wide_probe_launch.argtypes = (
        lib.wva_lag_path_wide_probe_launch.argtypes)
    lib.wva_ctx_plan_cells.restype = ctypes.c_int
    lib.wva_ctx_plan_cells.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
    # capacity-limited planning (FastSweep.plan(capacity=...))
    lib.wva_ctx_set_greedy_static.restype = ctypes.c_int
    lib.wva_ctx_set_greedy_static.argtypes = [
        ctypes.c_void_p,
        ctypes.c_void_p,  # host i32 [n_cells] accelerator-type index per cell
        ctypes.c_void_p,  # host i32 [n_cells] units per replica
        ctypes.c_void_p,  # host i32 [n_srv] priority
    ]
    lib.wva_ctx_plan_limited.restype = ctypes.c_int
    lib.wva_ctx_plan_limited.argtypes = [
        ctypes.c_void_p,
        ctypes.c_int,  # n_scen
        ctypes.c_int,  # n_acc
        ctypes.c_void_p,  # host fp32 [n_scen][n_cells] arrival rates
        ctypes.c_int,  # n_types
        ctypes.c_void_p,  # host i32 [n_scen][n_types] capacity
        ctypes.c_int,  # delayed best-effort
        ctypes.c_int,  # saturation policy 0..3
        ctypes.POINTER(ctypes.c_void_p),  # out: pinned fp32 [n_scen][6][n_srv]
        ctypes.POINTER(ctypes.c_void_p),  # out: pinned i32 [n_scen][4][n_srv]
        ctypes.POINTER(ctypes.c_void_p),  # out: pinned u64 [n_scen][n_acc]
        ctypes.POINTER(ctypes.c_void_p),  # out: pinned i32 [n_scen][2][n_srv]
        ctypes.POINTER(ctypes.c_void_p),  # out: pinned i32 [n_scen][n_types]
    ]
    _lib = lib
    return lib


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


@dataclass
class SweepOutputs:
    feasible: "object"  # torch uint8 [cells]
    zero_empty: "object"
    num_replicas: "object"  # int32
    batch: "object"  # int32
    cost: "object"  # float32
    value: "object"
    itl: "object"
    ttft: "object"
    rho: "object"
    max_rate: "object"


def run_sweep(arrays: dict, device: str = "cuda", analyzer_mode: int = 0,
              cv2: float = 1.0) -> SweepOutputs:
    """Launch the sweep kernel over cell SoA arrays (torch CPU tensors in,
    results copied back to CPU tensors).

    ``arrays`` keys (from engine.snapshot.build_cell_arrays): int32 tensors
    in_tok,out_tok,batch_n,min_replicas,perf_max_batch,cur_replicas,flags and
    float32 tensors alpha,beta,gamma,delta,arrival_rate,t_itl,t_ttft,t_tps,
    acc_cost,cur_cost.
    """
    import torch

    if not torch.cuda.is_available():
        raise HipKernelError("run_sweep requires a GPU (use the CPU engine backend instead)")
    lib = load_library()
    n_cells = int(arrays["in_tok"].shape[0])

    dev = {k: v.to(device, non_blocking=True) for k, v in arrays.items()}
    t = torch
    out = SweepOutputs(
        feasible=t.zeros(n_cells, dtype=t.uint8, device=device),
        zero_empty=t.zeros(n_cells, dtype=t.uint8, device=device),
        num_replicas=t.zeros(n_cells, dtype=t.int32, device=device),
        batch=t.zeros(n_cells, dtype=t.int32, device=device),
        cost=t.zeros(n_cells, dtype=t.float32, device=device),
        value=t.zeros(n_cells, dtype=t.float32, device=device),
        itl=t.zeros(n_cells, dtype=t.float32, device=device),
        ttft=t.zeros(n_cells, dtype=t.float32, device=device),
        rho=t.zeros(n_cells, dtype=t.float32, device=device),
        max_rate=t.zeros(n_cells, dtype=t.float32, device=device),
    )
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    # partition cells into regime-adaptive N-buckets (+ huge-N GMEM spill)
    buckets = []
    for nt, ids, bmax, count, gmem in choose_buckets(arrays["batch_n"].numpy()):
        ids_t = torch.from_numpy(ids).to(device) if ids is not None else None
        slabs = alloc_gmem_slabs(count, bmax, nt, device) if gmem else (None, None)
        buckets.append((nt, ids_t, bmax, slabs))

    # overlap the bucket launches on separate HIP streams: wall time becomes
    # the straggler bucket's latency instead of the sum of all three
    main_stream = torch.cuda.current_stream()
    side = [torch.cuda.Stream() for _ in range(max(len(buckets) - 1, 0))]
    for i, (nt, ids, bmax, slabs) in enumerate(buckets):
        if i == 0:
            cur = main_stream
        else:
            cur = side[i - 1]
            cur.wait_stream(main_stream)  # order after the H2D uploads
        n_blocks = n_cells if ids is None else int(ids.numel())
        rc = lib.wva_sweep_launch_bucket(
            ctypes.c_int(n_blocks),
            ctypes.c_int(max(bmax, 1)),
            ctypes.c_int(nt),
            _ptr(ids) if ids is not None else None,
            ctypes.c_int(int(analyzer_mode)),
            ctypes.c_float(float(cv2)),
            ctypes.c_void_p(cur.cuda_stream),
            _ptr(dev["in_tok"]),
            _ptr(dev["out_tok"]),
            _ptr(dev["batch_n"]),
            _ptr(dev["min_replicas"]),
            _ptr(dev["perf_max_batch"]),
            _ptr(dev["cur_replicas"]),
            _ptr(dev["flags"]),
            _ptr(dev["alpha"]),
            _ptr(dev["beta"]),
            _ptr(dev["gamma"]),
            _ptr(dev["delta"]),
            _ptr(dev["arrival_rate"]),
            _ptr(dev["t_itl"]),
            _ptr(dev["t_ttft"]),
            _ptr(dev["t_tps"]),
            _ptr(dev["acc_cost"]),
            _ptr(dev["cur_cost"]),
            _ptr(out.feasible),
            _ptr(out.zero_empty),
            _ptr(out.num_replicas),
            _ptr(out.batch),
            _ptr(out.cost),
            _ptr(out.value),
            _ptr(out.itl),
            _ptr(out.ttft),
            _ptr(out.rho),
            _ptr(out.max_rate),
            _ptr(slabs[0]) if slabs[0] is not None else None,
            _ptr(slabs[1]) if slabs[1] is not None else None,
        )
        if rc != 0:
            raise HipKernelError(f"wva_sweep_launch_bucket(nt={nt}) failed with hipError {rc}")
    for s in side:
        main_stream.wait_stream(s)
    return out


def run_argmin(value, feasible, seg_start) -> "object":
    """Segmented argmin over sweep outputs (device tensors). Returns winner
    cell index (int32, -1 = no feasible candidate) per server, on device."""
    import torch

    lib = load_library()
    n_servers = int(seg_start.shape[0]) - 1
    winner = torch.full((n_servers,), -1, dtype=torch.int32, device=value.device)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.wva_argmin_launch(
        ctypes.c_int(n_servers),
        stream,
        _ptr(value),
        _ptr(feasible),
        _ptr(seg_start),
        _ptr(winner),
    )
    if rc != 0:
        raise HipKernelError(f"wva_argmin_launch failed with hipError {rc}")
    return winner


def run_tail_probe(arrays: dict, lam, t, quantiles=(), device: str = "cuda"):
    """One-shot probe of the wait-time tail and the percentile TTFT sizing
    (wva_tail_probe_t), for tests and tools.

    ``arrays``: the sweep's per-cell CPU tensors (in_tok, out_tok, batch_n,
    alpha, beta, gamma, delta, t_ttft, t_tps are read). ``lam`` (req/msec) and
    ``t`` (msec): float64 [n_cells, P]. Returns numpy arrays: tail [n_cells, P]
    (NaN where lam is outside (0, s(N))), and for ``quantiles`` [Q] the sized
    lam_ttft [n_cells, Q] (req/msec) with its indicator [n_cells, Q] (-1 below,
    0 within, +1 above the reachable range; -2 degenerate rates). Cells go to
    the block width and geometry tier choose_buckets gives their N."""
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        raise HipKernelError("run_tail_probe requires a GPU")
    lib = load_library()
    n_cells = int(arrays["in_tok"].shape[0])
    lam = np.ascontiguousarray(lam, dtype=np.float64).reshape(n_cells, -1)
    t = np.ascontiguousarray(t, dtype=np.float64).reshape(n_cells, -1)
    if lam.shape != t.shape:
        raise ValueError("lam and t differ in shape")
    q = np.ascontiguousarray(quantiles, dtype=np.float64).reshape(-1)
    if ((q <= 0) | (q >= 1)).any():
        raise ValueError("quantiles must lie in (0, 1)")
    n_pairs, n_q = lam.shape[1], len(q)
    keys = ("in_tok", "out_tok", "batch_n", "alpha", "beta", "gamma", "delta", "t_ttft", "t_tps")
    dev = {k: arrays[k].to(device) for k in keys}
    f64 = dict(dtype=torch.float64, device=device)
    d_lam, d_t = torch.from_numpy(lam).to(device), torch.from_numpy(t).to(device)
    d_y = torch.from_numpy(1.0 - q).to(device)
    d_tail = torch.full((n_cells, max(n_pairs, 1)), float("nan"), **f64)
    d_lamq = torch.full((n_cells, max(n_q, 1)), float("nan"), **f64)
    d_ind = torch.full((n_cells, max(n_q, 1)), -2, dtype=torch.int32, device=device)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    keep = []
    for nt, ids, bmax, count, gmem in choose_buckets(arrays["batch_n"].numpy()):
        ids_t = torch.from_numpy(ids).to(device) if ids is not None else None
        slabs = alloc_gmem_slabs(count, bmax, nt, device) if gmem else (None, None)
        keep.append((ids_t, slabs))
        rc = lib.wva_tail_probe_launch(
            count, max(bmax, 1), nt, _ptr(ids_t) if ids_t is not None else None, stream,
            *[_ptr(dev[k]) for k in keys], n_pairs, _ptr(d_lam), _ptr(d_t), _ptr(d_tail),
            n_q, _ptr(d_y), _ptr(d_lamq), _ptr(d_ind),
            _ptr(slabs[0]) if gmem else None, _ptr(slabs[1]) if gmem else None,
        )
        if rc != 0:
            raise HipKernelError(f"wva_tail_probe_launch(nt={nt}) failed: {rc}")
    torch.cuda.synchronize()
    return (d_tail.cpu().numpy()[:, :n_pairs], d_lamq.cpu().numpy()[:, :n_q],
            d_ind.cpu().numpy()[:, :n_q])


_probe_lib: Optional[ctypes.CDLL] = None


def load_probe_library() -> ctypes.CDLL:
    """dlopen the probe build (ops/build.py): the kernel library's sources with
    the chain probe instantiated, a library of its own so that the kernels the
    engine runs are compiled without it. Built on first use if missing or stale."""
    global _probe_lib
    if _probe_lib is None:
        lib = ctypes.CDLL(build_probe())
        lib.wva_chain_probe_launch.restype = ctypes.c_int
        lib.wva_chain_probe_launch.argtypes = (
            [ctypes.c_int] * 3 + [ctypes.c_void_p] * 10 + [ctypes.c_int] + [ctypes.c_void_p] * 2
            + [ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 8
        )
        _probe_lib = lib
    return _probe_lib


def run_chain_probe(arrays: dict, lam=None, lam_pairs=None, targets=None, nt=None, gmem=None,
                    device: str = "cuda"):
    """One-shot probe of the production chain path (wva_chain_probe_t), for
    tests and tools: chain_eval on the fp32-reciprocal geometry, whole block and
    half-blocks, and the dual bisection with the sizing on top of it.

    ``arrays``: the sweep's per-cell CPU tensors (in_tok, out_tok, batch_n,
    alpha, beta, gamma, delta, t_tps are read). ``lam``: float64 [n_cells, P]
    rates (req/msec) of whole-block evaluations. ``lam_pairs``: float64
    [n_cells, R, 2], one half-block call per pair (half 0 takes [..., 0]).
    ``targets``: float32 [n_cells, T, 2] (TTFT, ITL) target pairs (msec, 0 =
    inactive). Any of the three may be None.

    ``nt`` and ``gmem`` both None: cells go to the block width and geometry tier
    choose_buckets gives their N. Else every cell runs in one launch of ``nt``
    threads (64, 128, 256, 512, 1024; default 256) with the geometry in LDS, or
    with ``gmem`` in global-memory slabs (256 or 1024 threads).

    Returns a dict of numpy arrays: ev1 [n_cells, P, 4] and ev2 [n_cells, R, 2, 4]
    (throughput req/msec, wait msec, serv msec, in_servers; NaN where a rate is
    outside (0, s(N)]), lam_star [n_cells, T, 2] (req/msec), ind [n_cells, T, 2]
    (-1 below, 0 within, +1 above; -2 degenerate rates), verdict [n_cells, T]
    (wva_size_cell's: 1 feasible) and tput [n_cells, T] (req/msec, NaN when
    infeasible)."""
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        raise HipKernelError("run_chain_probe requires a GPU")
    lib = load_probe_library()
    n_cells = int(arrays["in_tok"].shape[0])
    batch_n = arrays["batch_n"].numpy()
    if n_cells < 1 or batch_n.min() < 1:
        raise ValueError("run_chain_probe needs cells with N >= 1")

    def arg(a, dtype, last):
        a = np.zeros((n_cells, 0) + last) if a is None else a
        a = np.ascontiguousarray(a, dtype=dtype)
        if a.ndim != 2 + len(last) or a.shape[0] != n_cells or a.shape[2:] != last:
            raise ValueError(f"expected [{n_cells}, n{''.join(f', {d}' for d in last)}]")
        return a

    lam = arg(lam, np.float64, ())
    pairs = arg(lam_pairs, np.float64, (2,))
    tgt = arg(targets, np.float32, (2,))
    n_lam, n_pair, n_tgt = lam.shape[1], pairs.shape[1], tgt.shape[1]
    if nt is None and gmem is None:
        buckets = choose_buckets(batch_n)
    else:
        nt, gmem = 256 if nt is None else int(nt), bool(gmem)
        if nt not in ((256, 1024) if gmem else (64, 128, 256, 512, 1024)):
            raise ValueError(f"no chain probe of {nt} threads{' with slabs' if gmem else ''}")
        bmax = int(batch_n.max())
        if bmax > (HUGE_MAX_N if gmem else _ABI["WVA_XL_MAX_N"]):
            raise ValueError(f"N = {bmax} does not fit the tier")
        buckets = [(nt, None, bmax, n_cells, gmem)]
    keys = ("in_tok", "out_tok", "batch_n", "alpha", "beta", "gamma", "delta", "t_tps")
    dev = {k: arrays[k].to(device) for k in keys}
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    d_lam, d_la, d_lb = up(lam), up(pairs[:, :, 0]), up(pairs[:, :, 1])
    d_tt, d_ti = up(tgt[:, :, 0]), up(tgt[:, :, 1])
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64,  # noqa: E731
                                    device=device)
    d_ev1, d_ev2 = nan(n_cells, max(n_lam, 1), 4), nan(n_cells, max(n_pair, 1), 2, 4)
    d_star, d_tput = nan(n_cells, max(n_tgt, 1), 2), nan(n_cells, max(n_tgt, 1))
    d_ind = torch.full((n_cells, max(n_tgt, 1), 2), -2, dtype=torch.int32, device=device)
    d_ok = torch.zeros((n_cells, max(n_tgt, 1)), dtype=torch.int32, device=device)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    keep = []
    for b_nt, ids, bmax, count, b_gmem in buckets:
        ids_t = torch.from_numpy(ids).to(device) if ids is not None else None
        slabs = alloc_gmem_slabs(count, bmax, b_nt, device) if b_gmem else (None, None)
        keep.append((ids_t, slabs))
        rc = lib.wva_chain_probe_launch(
            count, bmax, b_nt, _ptr(ids_t) if ids_t is not None else None, stream,
            *[_ptr(dev[k]) for k in keys], n_lam, _ptr(d_lam), _ptr(d_ev1),
            n_pair, _ptr(d_la), _ptr(d_lb), _ptr(d_ev2),
            n_tgt, _ptr(d_tt), _ptr(d_ti), _ptr(d_star), _ptr(d_ind), _ptr(d_ok), _ptr(d_tput),
            _ptr(slabs[0]) if b_gmem else None, _ptr(slabs[1]) if b_gmem else None,
        )
        if rc != 0:
            raise HipKernelError(f"wva_chain_probe_launch(nt={b_nt}) failed: {rc}")
    torch.cuda.synchronize()
    host = lambda t, n: t.cpu().numpy()[:, :n]  # noqa: E731
    return dict(ev1=host(d_ev1, n_lam), ev2=host(d_ev2, n_pair), lam_star=host(d_star, n_tgt),
                ind=host(d_ind, n_tgt), verdict=host(d_ok, n_tgt), tput=host(d_tput, n_tgt))


def lag_task_table(fields: dict, cost):
    """The task table of a lag pass (WvaLagTask records): ``fields`` holds one
    array per LAG_TASK_DTYPE field (``pad`` aside), ``cost`` the tasks' cost
    proxy. Tasks are grouped by the narrowest class that holds their N, classes
    in launch order, and sorted by descending cost within a class. Returns
    (table, int32 [4] tasks per class, the permutation applied)."""
    import numpy as np

    n = np.asarray(fields["N"], dtype=np.int64)
    if len(n) and (n.min() < 1 or n.max() > LAG_MAX_N):
        raise HipKernelError(f"lag tasks must have 1 <= N <= {LAG_MAX_N}")
    cls = np.zeros(len(n), dtype=np.int64)
    for k, (nt, c) in enumerate(LAG_CLASSES):
        cls[11 * n + 1 <= nt * c] = k  # later classes are narrower
    order = np.lexsort((-np.asarray(cost, dtype=np.float64), cls))
    table = np.zeros(len(n), dtype=LAG_TASK_DTYPE)
    for name in LAG_TASK_DTYPE.names:
        if name != "pad":
            table[name] = np.asarray(fields[name])[order]
    counts = np.bincount(cls, minlength=len(LAG_CLASSES)).astype(np.int32)
    return table, counts, order


def lag_intervals(times) -> "object":
    """Interval lengths in msec (float64 [T]) of checkpoint times in seconds."""
    import numpy as np

    t = np.asarray(times, dtype=np.float64)
    return np.ascontiguousarray(np.diff(np.concatenate(([0.0], t))) * 1000.0)


def run_lag_probe(arrays: dict, lam0, lam1, times, max_steps: int = 1 << 22,
                  device: str = "cuda"):
    """One-shot probe of the lag kernel (wva_lag_t), for tests and tools.

    ``arrays``: per-cell CPU tensors or arrays in_tok, out_tok, batch_n, alpha,
    beta, gamma, delta; ``lam0`` / ``lam1`` (req/msec per replica, float64
    [n_cells]) the rates before and during the lag; ``times`` the checkpoints
    in seconds. Every cell is one task, run by the class its N selects.
    Returns (raw float64 [n_cells, T, 5]: blocked, in_servers, in_system, tput,
    wait — before the fp32 rounding of the public outputs; steps int32
    [n_cells], -1 for degenerate rates). A cell above ``max_steps`` has NaN
    functionals and its step count."""
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        raise HipKernelError("run_lag_probe requires a GPU")
    lib = load_library()
    n_cells = len(arrays["batch_n"])
    dt = lag_intervals(times)
    n_times = len(dt)
    if not 1 <= n_times <= LAG_MAX_T or not (dt > 0).all():
        raise ValueError(f"times must be 1..{LAG_MAX_T} strictly increasing positive seconds")
    fields = {k: np.asarray(arrays[k]) for k in ("in_tok", "out_tok", "alpha", "beta", "gamma",
                                                  "delta")}
    fields["N"] = np.asarray(arrays["batch_n"])
    fields["slot"] = np.arange(n_cells, dtype=np.int32)
    fields["t_ttft"] = fields["t_itl"] = np.zeros(n_cells, dtype=np.float32)
    fields["lam0"] = np.asarray(lam0, dtype=np.float64).reshape(n_cells)
    fields["lam1"] = np.asarray(lam1, dtype=np.float64).reshape(n_cells)
    table, counts, order = lag_task_table(fields, fields["N"])
    d_tasks = torch.from_numpy(table.view(np.uint8).reshape(-1)).to(device)
    d_dt = torch.from_numpy(dt).to(device)
    d_f = torch.empty((6, n_times, n_cells), dtype=torch.float32, device=device)
    d_viol = torch.empty((n_times, n_cells), dtype=torch.uint8, device=device)
    d_steps = torch.empty(n_cells, dtype=torch.int32, device=device)
    d_raw = torch.empty((n_cells, n_times, 5), dtype=torch.float64, device=device)
    rc = lib.wva_lag_probe_launch(
        table.ctypes.data, _ptr(d_tasks), counts.ctypes.data, n_times, _ptr(d_dt), n_cells,
        int(max_steps), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), _ptr(d_f),
        _ptr(d_viol), _ptr(d_steps), _ptr(d_raw),
    )
    if rc != 0:
        raise HipKernelError(f"wva_lag_probe_launch failed: {rc}")
    torch.cuda.synchronize()
    raw = np.empty((n_cells, n_times, 5))
    raw[order] = d_raw.cpu().numpy()  # rows are in task order
    return raw, d_steps.cpu().numpy()


def lag_segments(j_lo, j_hi, x, halo: int):
    """The segments of one task: each interval's j_hi steps cut into runs of at
    most ``halo`` steps that never cross a checkpoint. ``j_lo``, ``j_hi``, ``x``
    are per interval (lag_window of x = Lam dt). LAG_SEG_DTYPE records."""
    import numpy as np

    rows = []
    for j, (lo, hi) in enumerate(zip(j_lo, j_hi)):
        lo, hi = int(lo), int(hi)
        for first in range(0, hi, halo):
            count = min(halo, hi - first)
            last = first + count == hi
            flags = ((LAG_SEG_FIRST if first == 0 else 0) | (LAG_SEG_LAST if last else 0)
                     | (LAG_SEG_FINAL if last and j == len(j_hi) - 1 else 0))
            rows.append((float(x[j]), first, count, lo, hi, flags, j))
    return np.array(rows, dtype=LAG_SEG_DTYPE)


def lag_wide_schedule(fields: dict, lam_unif, dt, stride: int = LAG_WIDE_STRIDE,
                      halo: int = LAG_WIDE_HALO):
    """The host schedule of a wide lag pass. ``fields`` as for lag_task_table
    (every N in LAG_MAX_N + 1 .. LAG_WIDE_MAX_N), ``lam_unif`` the tasks'
    uniformization rates, ``dt`` the interval lengths (msec). Tasks are ordered
    by descending segment count, so that launch l (segment l of every task that
    has one) covers a prefix of the tasks and of the tile table. Returns (task
    table, wide table, segments, tiles, the permutation applied)."""
    import numpy as np

    from ..analyzer.lag import lag_window

    n = np.asarray(fields["N"], dtype=np.int64)
    if len(n) == 0 or n.min() <= LAG_MAX_N or n.max() > LAG_WIDE_MAX_N:
        raise HipKernelError(f"wide lag tasks must have {LAG_MAX_N} < N <= {LAG_WIDE_MAX_N}")
    c = LAG_WIDE_C
    if stride % c or halo % c or halo < c or stride < c or stride + 2 * halo > LAG_WIDE_W:
        raise ValueError(f"stride and halo must be multiples of {c} with "
                         f"stride + 2 halo <= {LAG_WIDE_W}")
    lam_unif = np.asarray(lam_unif, dtype=np.float64)
    dt = np.asarray(dt, dtype=np.float64)
    segs = []
    for lam in lam_unif:
        x = lam * dt
        lo, hi = lag_window(x)
        segs.append(lag_segments(lo, hi, x, halo))
    n_seg = np.array([len(s) for s in segs], dtype=np.int64)
    order = np.argsort(-n_seg, kind="stable")
    table = np.zeros(len(n), dtype=LAG_TASK_DTYPE)
    for name in LAG_TASK_DTYPE.names:
        if name != "pad":
            table[name] = np.asarray(fields[name])[order]
    slots = -(-(11 * n[order] + 1) // c) * c
    wide = np.zeros(len(n), dtype=LAG_WIDE_DTYPE)
    wide["Lam"] = lam_unif[order]
    wide["n_tiles"] = -(-slots // stride)
    wide["tile0"] = np.concatenate(([0], np.cumsum(wide["n_tiles"])[:-1]))
    wide["n_seg"] = n_seg[order]
    wide["seg0"] = np.concatenate(([0], np.cumsum(wide["n_seg"])[:-1]))
    tiles = np.zeros(int(wide["n_tiles"].sum()), dtype=LAG_TILE_DTYPE)
    tiles["task"] = np.repeat(np.arange(len(n)), wide["n_tiles"])
    tiles["b"] = np.arange(len(tiles)) - np.repeat(wide["tile0"], wide["n_tiles"])
    return table, wide, np.concatenate([segs[i] for i in order]), tiles, order


def run_lag_wide_probe(arrays: dict, lam0, lam1, times, stride: int = LAG_WIDE_STRIDE,
                       halo: int = LAG_WIDE_HALO, max_steps: int = 1 << 22,
                       device: str = "cuda"):
    """One-shot probe of the tiled lag path (wva_lag_wide_init, wva_lag_tile_t,
    wva_lag_wide_fin), the sibling of run_lag_probe with the tile stride and
    halo as arguments. Every cell (LAG_MAX_N < N <= LAG_WIDE_MAX_N) is one
    task. Returns (raw float64 [n_cells, T, 5], steps int32 [n_cells])."""
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        raise HipKernelError("run_lag_wide_probe requires a GPU")
    lib = load_library()
    n_cells = len(arrays["batch_n"])
    dt = lag_intervals(times)
    n_times = len(dt)
    if not 1 <= n_times <= LAG_MAX_T or not (dt > 0).all():
        raise ValueError(f"times must be 1..{LAG_MAX_T} strictly increasing positive seconds")
    fields = {k: np.asarray(arrays[k]) for k in ("in_tok", "out_tok", "alpha", "beta", "gamma",
                                                  "delta")}
    fields["N"] = np.asarray(arrays["batch_n"])
    fields["slot"] = np.arange(n_cells, dtype=np.int32)
    fields["t_ttft"] = fields["t_itl"] = np.zeros(n_cells, dtype=np.float32)
    fields["lam0"] = np.asarray(lam0, dtype=np.float64).reshape(n_cells)
    fields["lam1"] = np.asarray(lam1, dtype=np.float64).reshape(n_cells)
    lam_unif = fields["lam1"] + np.array([_lag_smax(fields, i) for i in range(n_cells)])
    table, wide, segs, tiles, order = lag_wide_schedule(fields, lam_unif, dt, stride, halo)
    need = ctypes.c_size_t()
    offs = (ctypes.c_size_t * 4)()
    args = (table.ctypes.data, wide.ctypes.data, segs.ctypes.data, tiles.ctypes.data,
            dt.ctypes.data, len(table), len(segs), len(tiles), n_times, n_cells, int(max_steps),
            int(stride), int(halo), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    rc = lib.wva_lag_wide_probe_launch(*args, None, 0, ctypes.byref(need), offs)
    if rc != 0:
        raise HipKernelError(f"wva_lag_wide_probe_launch failed: {rc}")
    dev = torch.empty(need.value, dtype=torch.uint8, device=device)
    rc = lib.wva_lag_wide_probe_launch(*args, _ptr(dev), need.value, ctypes.byref(need), offs)
    if rc != 0:
        raise HipKernelError(f"wva_lag_wide_probe_launch failed: {rc}")
    host = dev[offs[0]:offs[3] + n_cells * n_times * 40].cpu().numpy()
    at = lambda i, n, t: host[offs[i] - offs[0]:offs[i] - offs[0] + n].view(t)  # noqa: E731
    raw = np.empty((n_cells, n_times, 5))
    raw[order] = at(3, n_cells * n_times * 40, np.float64).reshape(n_cells, n_times, 5)
    return raw, at(2, n_cells * 4, np.int32).copy()


def lag_path_schedule(fields: dict, tick0, tick_steps, n_ticks: int, max_steps: int,
                      slab_cap: int = LAG_PATH_SLAB_CAP):
    """The host schedule of a lag-path pass. Task t is one run: ``fields`` holds
    one array per LAG_PATH_TASK_DTYPE field (``pad`` and ``carry`` aside) and
    ``start`` (LAG_PATH_STATIONARY or LAG_PATH_EMPTY); the run covers the ticks
    ``tick0[t]`` .. ``tick0[t] + len(tick_steps[t])`` and ``tick_steps[t]`` are
    their step counts (lag_window), none above ``max_steps``.

    The tick axis is cut into chunks common to all tasks, greedily from the
    left: a chunk ends before the tick that would push any task's step sum in
    it above ``max_steps`` or the chunk beyond LAG_MAX_T ticks, so every block
    stays inside the run time LAG_MAX_STEPS bounds. A task that crosses a chunk
    boundary gets a carry slab (the states of its class, 8 bytes each); tasks
    run in rounds whose slabs fit ``slab_cap`` together. Returns (task table,
    records in launch order, launches int32 [n, 4]: rec0, count, class, round
    by (round, chunk, class) with the records of a launch by descending cost,
    chunk bounds int64 [n_chunks + 1])."""
    import numpy as np

    n = np.asarray(fields["N"], dtype=np.int64)
    n_tasks = len(n)
    if n_tasks == 0 or n.min() < 1 or n.max() > LAG_MAX_N:
        raise HipKernelError(f"lag path tasks must have 1 <= N <= {LAG_MAX_N}")
    tick0 = np.asarray(tick0, dtype=np.int64)
    steps = np.zeros((n_tasks, n_ticks), dtype=np.int64)
    for t, row in enumerate(tick_steps):
        if len(row) < 1 or tick0[t] < 0 or tick0[t] + len(row) > n_ticks:
            raise ValueError("a run lies outside the tick axis")
        steps[t, tick0[t]:tick0[t] + len(row)] = row
    if steps.max() > max_steps:
        raise ValueError("a tick above max_steps cannot be scheduled")
    bounds, run = [0], np.zeros(n_tasks, dtype=np.int64)
    for j in range(n_ticks):
        nxt = run + steps[:, j]
        if j > bounds[-1] and (j - bounds[-1] >= LAG_MAX_T or nxt.max() > max_steps):
            bounds.append(j)
            nxt = steps[:, j]
        run = nxt
    bounds = np.array(bounds + [n_ticks], dtype=np.int64)
    cls = np.zeros(n_tasks, dtype=np.int64)
    for k, (nt, c) in enumerate(LAG_CLASSES):
        cls[11 * n + 1 <= nt * c] = k  # later classes are narrower
    table = np.zeros(n_tasks, dtype=LAG_PATH_TASK_DTYPE)
    for name in LAG_PATH_TASK_DTYPE.names:
        if name not in ("pad", "carry"):
            table[name] = np.asarray(fields[name])
    table["carry"] = -1
    start = np.asarray(fields["start"], dtype=np.int64)
    rows = []  # (round, chunk, class, -cost, task, tick0, n, flags)
    rnd, used = 0, 0
    for t in range(n_tasks):
        t0, t1 = int(tick0[t]), int(tick0[t]) + len(tick_steps[t])
        c0 = int(np.searchsorted(bounds, t0, side="right")) - 1
        c1 = int(np.searchsorted(bounds, t1, side="left"))  # chunks c0 .. c1 - 1
        if c1 - c0 > 1:
            words = LAG_CLASSES[cls[t]][0] * LAG_CLASSES[cls[t]][1]
            if used and (used + words) * 8 > slab_cap:
                rnd, used = rnd + 1, 0
            table["carry"][t] = used
            used += words
        for ch in range(c0, c1):
            a, b = max(t0, int(bounds[ch])), min(t1, int(bounds[ch + 1]))
            flags = (int(start[t]) if a == t0 else LAG_PATH_CARRY) | (LAG_PATH_STORE if b < t1
                                                                        else 0)
            rows.append((rnd, ch, int(cls[t]), -int(n[t]) * int(steps[t, a:b].sum()), t, a,
                         b - a, flags))
    rows.sort()
    recs = np.zeros(len(rows), dtype=LAG_PATH_REC_DTYPE)
    launches = []
    for i, (r, ch, k, _, t, a, cnt, flags) in enumerate(rows):
        recs[i] = (t, a, cnt, flags)
        if i and rows[i - 1][:3] == (r, ch, k):
            launches[-1][1] += 1
        else:
            launches.append([i, 1, k, r])
    return table, recs, np.array(launches, dtype=np.int32).reshape(-1, 4), bounds


def run_lag_path_probe(arrays: dict, start, lam, keep, tick_seconds: float,
                       max_steps: int = 1 << 22, device: str = "cuda", averages: bool = False):
    """One-shot probe of the lag-path kernel (wva_lag_path_t), for tests and
    tools, in the style of run_lag_probe. ``arrays`` as there; every cell is
    one run over all S ticks of ``tick_seconds``: ``start[i]`` is "empty" or
    ("stationary", lam0), ``lam`` and ``keep`` (float64 [n_cells, S]) its
    per-tick rate (req/msec per replica) and scale-out factor. ``max_steps``
    drives the chunking (lag_path_schedule), so a small one sends the state
    through the carry. Returns (raw float64 [n_cells, S, 5] as run_lag_probe,
    steps int32 [n_cells, S], the chunk bounds). ``averages``: run
    wva_lag_path_avg_t instead and return (raw, the raw functionals of the
    time-averaged distribution [n_cells, S, 5], steps, bounds)."""
    import numpy as np
    import torch

    from ..analyzer.lag import lag_window

    if not torch.cuda.is_available():
        raise HipKernelError("run_lag_path_probe requires a GPU")
    lib = load_library()
    n_cells = len(arrays["batch_n"])
    lam = np.ascontiguousarray(lam, dtype=np.float64).reshape(n_cells, -1)
    keep = np.ascontiguousarray(keep, dtype=np.float64).reshape(n_cells, -1)
    n_ticks = lam.shape[1]
    dt = float(tick_seconds) * 1000.0
    if n_ticks < 1 or keep.shape != lam.shape or not dt > 0 or not np.isfinite(dt):
        raise ValueError("lam and keep must be [n_cells, S >= 1], tick_seconds finite and > 0")
    if not ((lam >= 0).all() and (keep >= 0).all() and (keep <= 1).all()):
        raise ValueError("lam must be non-negative and keep in [0, 1]")
    fields = {k: np.asarray(arrays[k]) for k in ("in_tok", "out_tok", "alpha", "beta", "gamma",
                                                  "delta")}
    fields["N"] = np.asarray(arrays["batch_n"])
    fields["slot"] = np.arange(n_cells, dtype=np.int32)
    fields["t_ttft"] = fields["t_itl"] = np.zeros(n_cells, dtype=np.float32)
    fields["lam0"] = np.array([0.0 if isinstance(s, str) else float(s[1]) for s in start])
    fields["start"] = np.array([LAG_PATH_EMPTY if isinstance(s, str) else LAG_PATH_STATIONARY
                                for s in start])
    smax = np.array([_lag_smax(fields, i) for i in range(n_cells)])
    want = lag_window((lam + smax[:, None]) * dt)[1].astype(np.int64)
    table, recs, launches, bounds = lag_path_schedule(
        fields, np.zeros(n_cells, dtype=np.int64), list(want), n_ticks, int(max_steps))
    desc = np.ascontiguousarray(np.stack([lam, keep], axis=2))
    need = ctypes.c_size_t()
    # the offsets the launcher reports: records, violated, steps, (averaged
    # records and verdicts,) raw functionals (and the averaged ones)
    n_off, i_raw = (7, 5) if averages else (4, 3)
    launch = lib.wva_lag_path_avg_probe_launch if averages else lib.wva_lag_path_probe_launch
    offs = (ctypes.c_size_t * n_off)()
    args = (table.ctypes.data, recs.ctypes.data, desc.ctypes.data, launches.ctypes.data,
            len(table), len(recs), len(launches), n_ticks, n_cells, int(max_steps), dt,
            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    rc = launch(*args, None, 0, ctypes.byref(need), offs)
    if rc != 0:
        raise HipKernelError(f"{launch.__name__} failed: {rc}")
    dev = torch.empty(need.value, dtype=torch.uint8, device=device)
    rc = launch(*args, _ptr(dev), need.value, ctypes.byref(need), offs)
    if rc != 0:
        raise HipKernelError(f"{launch.__name__} failed: {rc}")
    cells = n_cells * n_ticks
    host = dev[offs[0]:offs[n_off - 1] + cells * 40].cpu().numpy()
    at = lambda i, n, t: host[offs[i] - offs[0]:offs[i] - offs[0] + n].view(t)  # noqa: E731
    raws = [at(i, cells * 40, np.float64).reshape(n_cells, n_ticks, 5).copy()
            for i in range(i_raw, n_off)]
    return (*raws, at(2, cells * 4, np.int32).reshape(n_ticks, n_cells).T.copy(), bounds)


def lag_path_wide_schedule(fields: dict, tick0, lam, keep, smax, dt: float, n_ticks: int,
                           stride: int = LAG_WIDE_STRIDE, halo: int = LAG_WIDE_HALO,
                           n_slots: Optional[int] = None):
    """The host schedule of a wide lag-path pass. Task t is one run on a cell
    with LAG_MAX_N < N <= LAG_WIDE_MAX_N: ``fields`` as for lag_path_schedule,
    the run covers the ticks ``tick0[t]`` .. ``tick0[t] + len(lam[t])`` at the
    per-replica rates ``lam[t]`` (req/msec) and scale-out factors ``keep[t]``,
    ``smax[t]`` is its largest service rate and ``dt`` the tick in msec. Every
    tick's steps (lag_window of (lam + smax) dt) are cut by lag_segments into
    runs of at most ``halo`` steps, so no segment crosses a tick; a segment's
    ``j`` is its tick. Tasks are ordered by descending segment count, so that
    launch l covers a prefix of the tasks and of the tile table. There are no
    chunks: no block takes more than ``halo`` steps. Returns (task table, wide
    table, segments, tiles, descriptors float64 [n_slots, n_ticks, 2], the
    permutation applied)."""
    import numpy as np

    from ..analyzer.lag import lag_window

    n = np.asarray(fields["N"], dtype=np.int64)
    if len(n) == 0 or n.min() <= LAG_MAX_N or n.max() > LAG_WIDE_MAX_N:
        raise HipKernelError(f"wide lag path tasks must have {LAG_MAX_N} < N <= {LAG_WIDE_MAX_N}")
    c = LAG_WIDE_C
    if stride % c or halo % c or halo < c or stride < c or stride + 2 * halo > LAG_WIDE_W:
        raise ValueError(f"stride and halo must be multiples of {c} with "
                         f"stride + 2 halo <= {LAG_WIDE_W}")
    slot = np.asarray(fields["slot"], dtype=np.int64)
    n_slots = int(slot.max()) + 1 if n_slots is None else int(n_slots)
    tick0 = np.asarray(tick0, dtype=np.int64)
    desc = np.zeros((n_slots, n_ticks, 2))
    desc[:, :, 1] = 1.0
    segs = []
    for t in range(len(n)):
        lam_t = np.asarray(lam[t], dtype=np.float64)
        if len(lam_t) < 1 or tick0[t] < 0 or tick0[t] + len(lam_t) > n_ticks:
            raise ValueError("a run lies outside the tick axis")
        ticks = slice(int(tick0[t]), int(tick0[t]) + len(lam_t))
        desc[slot[t], ticks, 0], desc[slot[t], ticks, 1] = lam_t, keep[t]
        x = (lam_t + float(smax[t])) * dt
        lo, hi = lag_window(x)
        seg = lag_segments(lo, hi, x, halo)
        seg["j"] += int(tick0[t])
        segs.append(seg)
    n_seg = np.array([len(s) for s in segs], dtype=np.int64)
    order = np.argsort(-n_seg, kind="stable")
    table = np.zeros(len(n), dtype=LAG_PATH_TASK_DTYPE)
    for name in LAG_PATH_TASK_DTYPE.names:
        if name not in ("pad", "carry"):
            table[name] = np.asarray(fields[name])[order]
    table["carry"] = -1
    slots = -(-(11 * n[order] + 1) // c) * c
    wide = np.zeros(len(n), dtype=LAG_PATH_WIDE_DTYPE)
    wide["smax"] = np.asarray(smax, dtype=np.float64)[order]
    wide["n_tiles"] = -(-slots // stride)
    wide["tile0"] = np.concatenate(([0], np.cumsum(wide["n_tiles"])[:-1]))
    wide["n_seg"] = n_seg[order]
    wide["seg0"] = np.concatenate(([0], np.cumsum(wide["n_seg"])[:-1]))
    wide["tick0"] = tick0[order]
    wide["n_run"] = [len(lam[t]) for t in order]
    wide["start"] = np.asarray(fields["start"])[order]
    tiles = np.zeros(int(wide["n_tiles"].sum()), dtype=LAG_TILE_DTYPE)
    tiles["task"] = np.repeat(np.arange(len(n)), wide["n_tiles"])
    tiles["b"] = np.arange(len(tiles)) - np.repeat(wide["tile0"], wide["n_tiles"])
    return table, wide, np.concatenate([segs[i] for i in order]), tiles, desc, order


def run_lag_path_wide_probe(arrays: dict, start, lam, keep, tick_seconds: float,
                            stride: int = LAG_WIDE_STRIDE, halo: int = LAG_WIDE_HALO,
                            max_steps: int = 1 << 22, device: str = "cuda",
                            averages: bool = False):
    """One-shot probe of the tiled lag-path kernels (wva_lag_path_wide_init,
    wva_lag_path_tile_t, wva_lag_path_wide_fin), the sibling of
    run_lag_path_probe with the tile stride and halo as arguments. Arguments as
    there; every cell (LAG_MAX_N < N <= LAG_WIDE_MAX_N) is one run over all S
    ticks. Returns (raw float64 [n_cells, S, 5], steps int32 [n_cells, S], the
    segments of every cell int64 [n_cells] in place of the chunk bounds).
    ``averages``: run wva_lag_path_avg_tile_t and wva_lag_path_avg_wide_fin
    instead and return (raw, the raw functionals of the time-averaged
    distribution [n_cells, S, 5], steps, segments)."""
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        raise HipKernelError("run_lag_path_wide_probe requires a GPU")
    lib = load_library()
    n_cells = len(arrays["batch_n"])
    lam = np.ascontiguousarray(lam, dtype=np.float64).reshape(n_cells, -1)
    keep = np.ascontiguousarray(keep, dtype=np.float64).reshape(n_cells, -1)
    n_ticks = lam.shape[1]
    dt = float(tick_seconds) * 1000.0
    if n_ticks < 1 or keep.shape != lam.shape or not dt > 0 or not np.isfinite(dt):
        raise ValueError("lam and keep must be [n_cells, S >= 1], tick_seconds finite and > 0")
    if not ((lam >= 0).all() and (keep >= 0).all() and (keep <= 1).all()):
        raise ValueError("lam must be non-negative and keep in [0, 1]")
    fields = {k: np.asarray(arrays[k]) for k in ("in_tok", "out_tok", "alpha", "beta", "gamma",
                                                  "delta")}
    fields["N"] = np.asarray(arrays["batch_n"])
    fields["slot"] = np.arange(n_cells, dtype=np.int32)
    fields["t_ttft"] = fields["t_itl"] = np.zeros(n_cells, dtype=np.float32)
    fields["lam0"] = np.array([0.0 if isinstance(s, str) else float(s[1]) for s in start])
    fields["start"] = np.array([LAG_PATH_EMPTY if isinstance(s, str) else LAG_PATH_STATIONARY
                                for s in start])
    smax = np.array([_lag_smax(fields, i) for i in range(n_cells)])
    table, wide, segs, tiles, desc, order = lag_path_wide_schedule(
        fields, np.zeros(n_cells, dtype=np.int64), list(lam), list(keep), smax, dt, n_ticks,
        stride, halo, n_cells)
    need = ctypes.c_size_t()
    # the offsets the launcher reports, as in run_lag_path_probe
    n_off, i_raw = (7, 5) if averages else (4, 3)
    launch = (lib.wva_lag_path_avg_wide_probe_launch if averages
              else lib.wva_lag_path_wide_probe_launch)
    offs = (ctypes.c_size_t * n_off)()
    args = (table.ctypes.data, wide.ctypes.data, segs.ctypes.data, tiles.ctypes.data,
            desc.ctypes.data, len(table), len(segs), len(tiles), n_ticks, n_cells, int(max_steps),
            int(stride), int(halo), dt, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    rc = launch(*args, None, 0, ctypes.byref(need), offs)
    if rc != 0:
        raise HipKernelError(f"{launch.__name__} failed: {rc}")
    dev = torch.empty(need.value, dtype=torch.uint8, device=device)
    rc = launch(*args, _ptr(dev), need.value, ctypes.byref(need), offs)
    if rc != 0:
        raise HipKernelError(f"{launch.__name__} failed: {rc}")
    cells = n_cells * n_ticks
    host = dev[offs[0]:offs[n_off - 1] + cells * 40].cpu().numpy()
    at = lambda i, n, t: host[offs[i] - offs[0]:offs[i] - offs[0] + n].view(t)  # noqa: E731
    raws = [at(i, cells * 40, np.float64).reshape(n_cells, n_ticks, 5).copy()
            for i in range(i_raw, n_off)]
    n_seg = np.empty(n_cells, dtype=np.int64)
    n_seg[order] = wide["n_seg"]
    return (*raws, at(2, cells * 4, np.int32).reshape(n_ticks, n_cells).T.copy(), n_seg)


def _lag_smax(fields: dict, i: int) -> float:
    """The largest fp32 service rate of task i of ``fields`` (the analyzer's
    build_service_rates, which wva_rate_exact matches to the bit)."""
    from ..analyzer import (Configuration, DecodeParms, PrefillParms, RequestSize,
                            ServiceParms)
    from ..analyzer.queue import build_service_rates

    n = int(fields["N"][i])
    cfg = Configuration(n, 10 * n, ServiceParms(
        PrefillParms(float(fields["gamma"][i]), float(fields["delta"][i])),
        DecodeParms(float(fields["alpha"][i]), float(fields["beta"][i]))))
    rates = build_service_rates(cfg, RequestSize(int(fields["in_tok"][i]),
                                                 int(fields["out_tok"][i])))
    return float(rates.max())


def run_greedy_native(cand_value, cand_acc_type, cand_units, cand_replicas,
                      seg_start, srv_priority, capacity, delayed: bool,
                      policy: int, allow_build: bool = True):
    """Host-side native greedy solver (C++ in the same .so; no GPU needed).

    All array args are contiguous numpy arrays (value f32, the rest i32);
    ``capacity`` is mutated in place. Returns (winner_cand, winner_replicas)
    int32 arrays per server (-1 = unallocated). Semantics identical to
    solver.greedy.solve_greedy (differential-tested)."""
    import numpy as np

    lib = load_library(allow_build=allow_build)
    n_servers = len(seg_start) - 1
    out_cand = np.full(n_servers, -1, dtype=np.int32)
    out_reps = np.zeros(n_servers, dtype=np.int32)

    def p(a):
        return a.ctypes.data_as(ctypes.c_void_p)

    rc = lib.wva_greedy_solve(
        ctypes.c_int(n_servers), ctypes.c_int(len(capacity)),
        p(cand_value), p(cand_acc_type), p(cand_units), p(cand_replicas),
        p(seg_start), p(srv_priority), p(capacity),
        ctypes.c_int(1 if delayed else 0), ctypes.c_int(int(policy)),
        p(out_cand), p(out_reps),
    )
    if rc != 0:
        raise HipKernelError(f"wva_greedy_solve failed: {rc}")
    return out_cand, out_reps


def run_stage_dynamic(arrival, in_tok, out_tok, cur_acc, cur_rep, cur_cost, cell_server,
                      cell_acc_idx, perf_max_batch_cfg, at_tokens, override,
                      zero_arrival=None, prev_batch_n=None, allow_build: bool = True):
    """Host-only native staging (ops/native/stage.cpp; no GPU needed): the
    six per-server arrays and the static per-cell topology -> the dynamic
    block, an int32 array [8, n_cells] whose rows are in_tok, out_tok,
    batch_n, perf_max_batch, cur_replicas, flags and the bit patterns of the
    fp32 rows arrival_rate, cur_cost (``block[6:].view(np.float32)``).
    ``zero_arrival`` replaces ``arrival`` in the zero-load decision.

    Returns (block, changed): changed says whether batch_n differs from
    ``prev_batch_n`` (always True when that is None)."""
    import numpy as np

    lib = load_library(allow_build=allow_build)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
    srv = [f32(arrival), i32(in_tok), i32(out_tok), i32(cur_acc), i32(cur_rep), f32(cur_cost)]
    topo = [i32(cell_server), i32(cell_acc_idx), i32(perf_max_batch_cfg), i32(at_tokens),
            i32(override)]
    n_srv, n_cells = len(srv[0]), len(topo[0])
    if any(len(a) != n_srv for a in srv) or any(len(a) != n_cells for a in topo):
        raise ValueError("per-server / per-cell arrays differ in length")
    zero = f32(zero_arrival) if zero_arrival is not None else None
    prev = i32(prev_batch_n) if prev_batch_n is not None else None
    if (zero is not None and len(zero) != n_srv) or (prev is not None and len(prev) != n_cells):
        raise ValueError("zero_arrival / prev_batch_n have the wrong length")
    block = np.empty((DYN_ROWS, n_cells), dtype=np.int32)
    changed = ctypes.c_int(0)

    def p(a):
        return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None

    rc = lib.wva_stage_dynamic(
        n_srv, n_cells, *[p(a) for a in srv], p(zero), *[p(a) for a in topo], p(block),
        p(prev), ctypes.byref(changed),
    )
    if rc != 0:
        raise HipKernelError(f"wva_stage_dynamic failed: {rc}")
    return block, bool(changed.value)


def run_aggregate_by_type(acc_idx, num_replicas, cost, valid, inst, mult, type_idx,
                          n_types: int, allow_build: bool = True):
    """Host-only native by-type aggregation (ops/native/stage.cpp): unit
    counts (int64 [n_types]) and fp64 cost sums of the winners with ``valid``
    set and ``acc_idx >= 0``. Servers are added in ascending order, one fp64
    add each — the order np.add.at uses — so the sums carry the same bits as
    the numpy path of ShardedSolver._aggregate_by_type. The unit product
    replicas * inst * mult is formed in int64 where numpy forms it in int32
    and widens: the two differ only where that one silently overflowed."""
    import numpy as np

    lib = load_library(allow_build=allow_build)
    acc_idx = np.ascontiguousarray(acc_idx, dtype=np.int32)
    num_replicas = np.ascontiguousarray(num_replicas, dtype=np.int32)
    cost = np.ascontiguousarray(cost, dtype=np.float32)
    valid = np.ascontiguousarray(valid, dtype=np.bool_)
    inst = np.ascontiguousarray(inst, dtype=np.int32)
    mult = np.ascontiguousarray(mult, dtype=np.int32)
    type_idx = np.ascontiguousarray(type_idx, dtype=np.int32)
    n_srv, n_acc = len(acc_idx), len(mult)
    if inst.shape != (n_srv, n_acc) or len(type_idx) != n_acc or not (
            len(num_replicas) == len(cost) == len(valid) == n_srv):
        raise ValueError("aggregation inputs differ in shape")
    tcount = np.zeros(n_types, dtype=np.int64)
    tcost = np.zeros(n_types, dtype=np.float64)
    rc = lib.wva_aggregate_by_type(
        n_srv, n_acc, n_types, acc_idx.ctypes.data, num_replicas.ctypes.data,
        cost.ctypes.data, valid.ctypes.data, inst.ctypes.data, mult.ctypes.data,
        type_idx.ctypes.data, tcount.ctypes.data, tcost.ctypes.data,
    )
    if rc != 0:
        raise HipKernelError(f"wva_aggregate_by_type failed: {rc}")
    return tcount, tcost


def library_loaded() -> bool:
    return _lib is not None and os.path.exists(LIB_PATH)
