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

from .build import LIB_PATH, build, needs_build

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
    for name, mirror in _ABI.items():
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
