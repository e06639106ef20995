"""NativeCtx — owner of one native reconcile context and of every buffer the
context was handed (ops/hip/wva_ctx.inc).

FastSweep (engine/fastpath.py) holds one as ``_gpu``. It owns the torch device
and pinned buffers, the opaque ctx handle, the bucket cache and what was last
pushed into the context; its methods are the ctypes calls, nothing else. The
context keeps raw pointers into the tensors, so they live here, next to the
handle, and the handle is destroyed first (close()).
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import numpy as np

from ..ops.sweep import (
    DYN_ROWS,
    REC_ROWS,
    TICK_STALE,
    HipKernelError,
    alloc_gmem_slabs,
    choose_buckets,
    gmem_slab_bytes,
    load_library,
)

# Most bytes of global-memory geometry slabs one huge-tier bucket of a
# token-mix plan may hold (NativeCtx.plan_tokens): the tier's tasks grow with
# the number of token sets, so a bucket that needs more runs in consecutive
# slices which share one allocation of at most this size.
# INFERNO_PLAN_TOKENS_SLAB_BYTES replaces it, read when a context is created.
PLAN_TOKENS_SLAB_BYTES = 1 << 30

# The dynamic block (4-byte words, int32 rows then fp32 rows) in row order.
DYN_INT = ("in_tok", "out_tok", "batch_n", "perf_max_batch", "cur_replicas", "flags")
DYN_F32 = ("arrival_rate", "cur_cost")
_BATCH_N_ROW = DYN_INT.index("batch_n")
_STAT_F32 = ("alpha", "beta", "gamma", "delta", "t_itl", "t_ttft", "t_tps", "acc_cost")
# per-cell outputs in WvaCellsOut order, with the dtypes of wva_ctx_plan_cells
CELL_KEYS = ("feasible", "zero_empty", "num_replicas", "batch", "cost", "value", "itl", "ttft",
             "rho", "max_rate")
_CELL_DTYPES = (np.uint8, np.uint8, np.int32, np.int32) + (np.float32,) * 6
# wva_ctx_create's pointer slots, in order, as attribute names of NativeCtx
# (WVA_CTX_SLOTS of them; the order is the C side's and must not change)
CTX_SLOT_NAMES = (
    "dev_dyn", "min_replicas", "alpha", "beta", "gamma", "delta", "t_itl", "t_ttft", "t_tps",
    "acc_cost", "feasible", "zero_empty", "num_replicas", "batch", "cost", "value", "itl", "ttft",
    "rho", "max_rate", "seg", "winner", "cell_acc", "gather", "pin_dyn", "pin_out",
)


def _copy_out(ptr: ctypes.c_void_p, ctype, shape) -> np.ndarray:
    """A numpy copy of one of the context's pinned result buffers."""
    buf = (ctype * int(np.prod(shape))).from_address(ptr.value)
    return np.ctypeslib.as_array(buf).reshape(shape).copy()


class NativeCtx:
    def __init__(self, n_srv: int, stat: dict, cell_server, cell_acc_idx, seg_start,
                 device: str):
        """Upload the static SoA (``stat``: FastSweep._stat) and allocate the
        dynamic block, the per-cell outputs and the winner-record block with
        their pinned mirrors, then create the context on them."""
        import torch

        self._lib = load_library(allow_build=False)
        self.device = device
        self.n_srv = n_srv
        self.n_cells = n = len(cell_server)
        self.ctx = None
        # static topology the native tick stages from (copied by the context)
        self._topo = [
            np.ascontiguousarray(a, dtype=np.int32)
            for a in (cell_server, cell_acc_idx, stat["perf_max_batch_cfg"], stat["at_tokens"],
                      stat["override"])
        ]
        for k in _STAT_F32:
            setattr(self, k, torch.from_numpy(np.ascontiguousarray(stat[k])).to(device))
        self.min_replicas = torch.from_numpy(
            np.ascontiguousarray(stat["min_replicas"], dtype=np.int32)
        ).to(device)
        self.pin_dyn = torch.empty((DYN_ROWS, n), dtype=torch.int32, pin_memory=True)
        self.dev_dyn = torch.empty((DYN_ROWS, n), dtype=torch.int32, device=device)
        self.pin_dyn_np = self.pin_dyn.numpy()
        self.seg = torch.from_numpy(seg_start).to(device)
        self.cell_acc = torch.from_numpy(self._topo[1]).to(device)
        # outputs
        for k, dt in zip(CELL_KEYS, (torch.uint8, torch.uint8, torch.int32, torch.int32)
                         + (torch.float32,) * 6):
            setattr(self, k, torch.zeros(n, dtype=dt, device=device))
        self.winner = torch.full((n_srv,), -1, dtype=torch.int32, device=device)
        # winner records: six fp32 rows (cost, value, itl, ttft, rho, max_rate)
        # then four int32 rows (acc code, num_replicas, batch, winner cell)
        self.gather = torch.empty((REC_ROWS, n_srv), dtype=torch.int32, device=device)
        self.pin_out = torch.empty((REC_ROWS, n_srv), dtype=torch.int32, pin_memory=True)
        self.pin_out_np = self.pin_out.numpy()
        self.tick_stale = False  # did the last tick find the bucket layout stale
        self.stale_ticks = 0
        self.bucket_key = None  # batch_n bytes `buckets` was chosen for
        self.buckets: list = []
        self.greedy_static_key = None  # static greedy inputs last pushed
        # token-mix planning's own bucket cache: the task batch_n bytes
        # `tok_buckets` was chosen for. Apart from bucket_key / buckets, which
        # describe the layout the context holds for its reconciles.
        self.tok_bucket_key = None
        self.tok_buckets: list = []
        env = os.environ.get("INFERNO_PLAN_TOKENS_SLAB_BYTES")
        try:
            self.tok_slab_budget = int(env) if env else PLAN_TOKENS_SLAB_BYTES
        except ValueError:
            raise ValueError(
                f"INFERNO_PLAN_TOKENS_SLAB_BYTES must be an integer, got {env!r}") from None
        if self.tok_slab_budget < 1:
            raise ValueError("INFERNO_PLAN_TOKENS_SLAB_BYTES must be positive")
        self._create_ctx()

    def _create_ctx(self) -> None:
        """Create the native reconcile context (opaque C struct owning the
        HIP streams/events and all registered device/pinned pointers) —
        the whole per-tick pipeline then runs behind ONE C call."""
        lib = self._lib
        n_slots = lib.wva_abi(b"WVA_CTX_SLOTS")
        if len(CTX_SLOT_NAMES) != n_slots:
            raise HipKernelError(
                f"WVA_CTX_SLOTS is {n_slots} in the library but engine/native_ctx.py "
                f"fills {len(CTX_SLOT_NAMES)} slots"
            )
        arr = (ctypes.c_void_p * n_slots)(
            *[ctypes.c_void_p(getattr(self, name).data_ptr()) for name in CTX_SLOT_NAMES]
        )
        ctx = lib.wva_ctx_create(ctypes.c_int(self.n_cells), ctypes.c_int(self.n_srv), arr)
        if not ctx:
            raise HipKernelError("wva_ctx_create failed")
        self.ctx = ctx
        rc = lib.wva_ctx_set_topology(ctx, *[a.ctypes.data for a in self._topo])
        if rc != 0:
            raise HipKernelError(f"wva_ctx_set_topology failed: {rc}")

    def close(self) -> None:
        """Destroy the context (its streams, events and own allocations). The
        tensors it points into are still alive here."""
        ctx, self.ctx = self.ctx, None
        if ctx is not None:
            self._lib.wva_ctx_destroy(ctx)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------
    def buckets_for(self, batch_n: np.ndarray):
        import torch

        key = batch_n.tobytes()
        if self.bucket_key == key:
            return self.buckets
        buckets = []
        for nt, ids, bmax, count, gmem in choose_buckets(batch_n):
            ids_t = torch.from_numpy(ids).to(self.device) if ids is not None else None
            slabs = (
                alloc_gmem_slabs(count, bmax, nt, self.device) if gmem else (None, None)
            )
            buckets.append((nt, ids_t, bmax, count, slabs))
        self.bucket_key = key
        self.buckets = buckets
        return buckets

    def sync_buckets(self, batch_n: np.ndarray, analyzer_mode: int, cv2: float) -> None:
        """Push the bucket layout + analyzer mode into the native context,
        together with the batch_n it was chosen for (called when the context
        reported its layout stale)."""
        buckets = self.buckets_for(batch_n)

        def ptrs(tensors):
            return (ctypes.c_void_p * len(tensors))(
                *[ctypes.c_void_p(t.data_ptr()) if t is not None else None for t in tensors]
            )

        n = len(buckets)
        nts = (ctypes.c_int * n)(*[b[0] for b in buckets])
        nbl = (ctypes.c_int * n)(
            *[int(b[1].numel()) if b[1] is not None else self.n_cells for b in buckets]
        )
        mxn = (ctypes.c_int * n)(*[b[2] for b in buckets])
        batch_n = np.ascontiguousarray(batch_n, dtype=np.int32)
        rc = self._lib.wva_ctx_set_buckets(
            self.ctx, ctypes.c_int(n), nts, ptrs([b[1] for b in buckets]), nbl, mxn,
            ctypes.c_int(analyzer_mode), ctypes.c_float(cv2),
            ptrs([b[4][0] for b in buckets]), ptrs([b[4][1] for b in buckets]),
            batch_n.ctypes.data,
        )
        if rc != 0:
            raise HipKernelError(f"wva_ctx_set_buckets failed: {rc}")

    def sync_greedy_static(self, cell_tidx, units, prio) -> None:
        """Upload the static greedy inputs into the native context (only when
        they changed)."""
        arrs = [np.ascontiguousarray(a, dtype=np.int32) for a in (cell_tidx, units, prio)]
        key = b"".join(a.tobytes() for a in arrs)
        if self.greedy_static_key == key:
            return
        rc = self._lib.wva_ctx_set_greedy_static(
            self.ctx, *[a.ctypes.data_as(ctypes.c_void_p) for a in arrs]
        )
        if rc != 0:
            raise HipKernelError(f"wva_ctx_set_greedy_static failed: {rc}")
        self.greedy_static_key = key

    # ------------------------------------------------------------------
    def tick(self, srv, zero: Optional[np.ndarray], launch: bool) -> bool:
        """wva_ctx_tick on the six contiguous per-server arrays ``srv``
        (arrival, in_tok, out_tok, cur_acc, cur_rep, cur_cost). Returns
        whether the context found its bucket layout stale — it then staged
        the tick but launched nothing; sync_buckets(staged_batch_n(), ...)
        and resume() finish it."""
        rc = self._lib.wva_ctx_tick(
            self.ctx, srv[0].ctypes.data, srv[1].ctypes.data, srv[2].ctypes.data,
            srv[3].ctypes.data, srv[4].ctypes.data, srv[5].ctypes.data,
            zero.ctypes.data if zero is not None else None, 1 if launch else 0,
        )
        self.tick_stale = rc == TICK_STALE
        if rc == TICK_STALE:
            self.stale_ticks += 1
            return True
        if rc != 0:
            raise HipKernelError(f"native reconcile tick failed: {rc}")
        return False

    def staged_batch_n(self) -> np.ndarray:
        return self.pin_dyn_np[_BATCH_N_ROW].copy()

    def resume(self) -> None:
        """Run the already staged tick (wva_reconcile) and synchronise."""
        rc = self._lib.wva_reconcile(self.ctx)
        if rc != 0:
            raise HipKernelError(f"native reconcile tick failed: {rc}")

    def winner_block(self) -> tuple[np.ndarray, np.ndarray]:
        """The last tick's winner records, copied out of the pinned block:
        (fp32 [6, n_srv], int32 [4, n_srv])."""
        blk = self.pin_out_np.copy()
        return blk[:6].view(np.float32), blk[6:]

    def cells(self) -> dict:
        """The last tick's per-cell outputs, downloaded."""
        return {k: getattr(self, k).cpu().numpy() for k in CELL_KEYS}

    def memo_stats(self) -> Optional[tuple[int, int]]:
        """(hits, misses) of the sizing memo, None when the memo is off."""
        hits, misses = ctypes.c_uint(0), ctypes.c_uint(0)
        rc = self._lib.wva_ctx_memo_stats(self.ctx, ctypes.byref(hits), ctypes.byref(misses))
        if rc < 0:
            raise HipKernelError(f"wva_ctx_memo_stats failed: {rc}")
        if rc != 0:
            return None
        return int(hits.value), int(misses.value)

    def fused_state(self) -> dict:
        """Diagnostics of the fused tick (synchronous, never on the hot path):
        ``path`` 0 = bucket launches + wva_winner, 1 = one wva_tick_t launch,
        2 = two; the task counts and LDS sizes of the launches; the CU count of
        the residency rule; ``waves_first`` / ``waves_second``, the launch bound
        (blocks per CU) of the kernel instantiation each launch uses, 0 for a
        launch that does not exist; ``done_nonzero``, how many arrival counters are
        not 0 (-1 when the fused tick is off; 0 after every completed tick)."""
        info = (ctypes.c_int * 8)()
        nz = ctypes.c_int(-1)
        rc = self._lib.wva_ctx_fused_state(self.ctx, info, ctypes.byref(nz))
        if rc != 0:
            raise HipKernelError(f"wva_ctx_fused_state failed: {rc}")
        keys = ("path", "n_tasks", "n_tasks_second", "lds_first", "lds_second", "n_cus",
                "waves_first", "waves_second")
        out = dict(zip(keys, (int(v) for v in info)))
        out["done_nonzero"] = int(nz.value)
        return out

    # ------------------------------------------------------------------
    def plan(self, cell_scen: np.ndarray, n_acc: int, limited=None):
        """wva_ctx_plan on [S, n_cells] fp32 arrivals (the tick is staged and
        the buckets are set): (fp32 [S, 6, n_srv], int32 [S, 4, n_srv], int64
        totals [S, n_acc]). ``limited`` = (int32 capacity [S, n_types],
        delayed, policy code) makes it wva_ctx_plan_limited (after
        sync_greedy_static) and appends int32 [S, 2, n_srv] (pre-cut replicas,
        candidate counts) and the int64 capacity left [S, n_types]."""
        n_scen = cell_scen.shape[0]
        out = [ctypes.c_void_p() for _ in range(3 if limited is None else 5)]
        refs = [ctypes.byref(p) for p in out]
        if limited is None:
            call = "wva_ctx_plan"
            rc = self._lib.wva_ctx_plan(self.ctx, n_scen, n_acc, cell_scen.ctypes.data, *refs)
        else:
            call = "wva_ctx_plan_limited"
            cap, delayed, policy = limited
            rc = self._lib.wva_ctx_plan_limited(
                self.ctx, n_scen, n_acc, cell_scen.ctypes.data, cap.shape[1], cap.ctypes.data,
                1 if delayed else 0, policy, *refs,
            )
        if rc != 0:
            raise HipKernelError(f"{call} failed: {rc}")
        res = (
            _copy_out(out[0], ctypes.c_float, (n_scen, 6, self.n_srv)),
            _copy_out(out[1], ctypes.c_int32, (n_scen, 4, self.n_srv)),
            _copy_out(out[2], ctypes.c_uint64, (n_scen, n_acc)).astype(np.int64),
        )
        if limited is not None:
            res += (_copy_out(out[3], ctypes.c_int32, (n_scen, 2, self.n_srv)),
                    _copy_out(out[4], ctypes.c_int32, cap.shape).astype(np.int64))
        return res

    def plan_slo(self, cell_scen: np.ndarray, cell_ttft: np.ndarray, cell_itl: np.ndarray,
                 n_acc: int):
        """wva_ctx_plan_slo on [S, n_cells] fp32 arrivals and [T, n_cells] fp32
        TTFT / ITL targets (the tick is staged and the buckets are set):
        plan()'s first three arrays with T * S leading, slice t * S + s being
        target set t at arrival rates s."""
        n_load, n_tgt = cell_scen.shape[0], cell_ttft.shape[0]
        n_scen = n_tgt * n_load
        out = [ctypes.c_void_p() for _ in range(3)]
        rc = self._lib.wva_ctx_plan_slo(
            self.ctx, n_tgt, n_scen, n_acc, cell_scen.ctypes.data, cell_ttft.ctypes.data,
            cell_itl.ctypes.data, *[ctypes.byref(p) for p in out],
        )
        if rc != 0:
            raise HipKernelError(f"wva_ctx_plan_slo failed: {rc}")
        return (
            _copy_out(out[0], ctypes.c_float, (n_scen, 6, self.n_srv)),
            _copy_out(out[1], ctypes.c_int32, (n_scen, 4, self.n_srv)),
            _copy_out(out[2], ctypes.c_uint64, (n_scen, n_acc)).astype(np.int64),
        )

    def tok_buckets_for(self, task_n: np.ndarray):
        """Task buckets of a token-mix plan, chosen over the flattened
        [W * n_cells] task batch sizes and cached on their bytes: [(nt, device
        task ids or None, max N, tasks, slabs, tasks per launch)]. A huge-tier
        bucket whose slabs would exceed the budget gets slabs for as many
        tasks as fit and runs in slices of that many (0 = one launch)."""
        import torch

        key = task_n.tobytes()
        if self.tok_bucket_key == key:
            return self.tok_buckets
        self.tok_bucket_key, self.tok_buckets = None, []  # drop the old slabs first
        buckets = []
        for nt, ids, bmax, count, gmem in choose_buckets(task_n):
            slabs, per_launch = (None, None), 0
            if gmem:
                per_task = gmem_slab_bytes(bmax, nt)
                fit = self.tok_slab_budget // per_task
                if fit < 1:
                    raise HipKernelError(
                        f"one token-mix task of batch size {bmax} needs {per_task} bytes of "
                        f"geometry slabs, above the budget of {self.tok_slab_budget} "
                        "(INFERNO_PLAN_TOKENS_SLAB_BYTES)"
                    )
                if fit < count:
                    per_launch = int(fit)
                    if ids is None:  # a slice names its tasks
                        ids = np.arange(count, dtype=np.int32)
                slabs = alloc_gmem_slabs(min(count, fit), bmax, nt, self.device)
            ids_t = torch.from_numpy(ids).to(self.device) if ids is not None else None
            buckets.append((nt, ids_t, bmax, count, slabs, per_launch))
        self.tok_bucket_key, self.tok_buckets = key, buckets
        return buckets

    def plan_tokens(self, cell_scen: np.ndarray, cell_in: np.ndarray, cell_out: np.ndarray,
                    cell_n: np.ndarray, n_acc: int):
        """wva_ctx_plan_tokens on [S, n_cells] fp32 arrivals and [W, n_cells]
        int32 in_tok / out_tok / batch_n (the tick is staged): plan()'s first
        three arrays with W * S leading, slice w * S + s being token set w at
        arrival rates s. The pass runs on task buckets of its own
        (tok_buckets_for); the context's reconcile layout is not touched."""
        n_load, n_tok = cell_scen.shape[0], cell_n.shape[0]
        n_scen = n_tok * n_load
        buckets = self.tok_buckets_for(cell_n.reshape(-1))

        def ptrs(tensors):
            return (ctypes.c_void_p * len(tensors))(
                *[ctypes.c_void_p(t.data_ptr()) if t is not None else None for t in tensors]
            )

        def ints(values):
            return (ctypes.c_int * len(values))(*values)

        out = [ctypes.c_void_p() for _ in range(3)]
        rc = self._lib.wva_ctx_plan_tokens(
            self.ctx, n_tok, n_scen, n_acc, cell_scen.ctypes.data, cell_in.ctypes.data,
            cell_out.ctypes.data, cell_n.ctypes.data, len(buckets),
            ints([b[0] for b in buckets]), ptrs([b[1] for b in buckets]),
            ints([b[3] for b in buckets]), ints([b[2] for b in buckets]),
            ptrs([b[4][0] for b in buckets]), ptrs([b[4][1] for b in buckets]),
            ints([b[5] for b in buckets]), *[ctypes.byref(p) for p in out],
        )
        if rc != 0:
            raise HipKernelError(f"wva_ctx_plan_tokens failed: {rc}")
        return (
            _copy_out(out[0], ctypes.c_float, (n_scen, 6, self.n_srv)),
            _copy_out(out[1], ctypes.c_int32, (n_scen, 4, self.n_srv)),
            _copy_out(out[2], ctypes.c_uint64, (n_scen, n_acc)).astype(np.int64),
        )

    def rollout(self, cell_scen: np.ndarray, n_acc: int, cur):
        """wva_ctx_rollout on [S, n_cells] fp32 arrivals, the rows being
        consecutive ticks, starting from the per-server current allocation
        ``cur`` = (cur_acc i32, cur_rep i32, cur_cost f32), which the tick was
        staged with: plan()'s three arrays, then the allocation after the last
        step as a (cur_acc, cur_rep, cur_cost) triple."""
        n_steps = cell_scen.shape[0]
        cur = (np.ascontiguousarray(cur[0], dtype=np.int32),
               np.ascontiguousarray(cur[1], dtype=np.int32),
               np.ascontiguousarray(cur[2], dtype=np.float32))
        for a in cur:
            if a.shape != (self.n_srv,):
                raise ValueError(
                    f"per-server override has shape {a.shape}, expected ({self.n_srv},)"
                )
        out = [ctypes.c_void_p() for _ in range(4)]
        rc = self._lib.wva_ctx_rollout(
            self.ctx, n_steps, n_acc, cell_scen.ctypes.data, cur[0].ctypes.data,
            cur[1].ctypes.data, cur[2].ctypes.data, *[ctypes.byref(p) for p in out],
        )
        if rc != 0:
            raise HipKernelError(f"wva_ctx_rollout failed: {rc}")
        end = _copy_out(out[3], ctypes.c_int32, (3, self.n_srv))
        return (
            _copy_out(out[0], ctypes.c_float, (n_steps, 6, self.n_srv)),
            _copy_out(out[1], ctypes.c_int32, (n_steps, 4, self.n_srv)),
            _copy_out(out[2], ctypes.c_uint64, (n_steps, n_acc)).astype(np.int64),
            (end[0], end[1], end[2].view(np.float32)),
        )

    def ensemble_pass(self, cell_scen: np.ndarray, dims, path0: int, n_acc: int, cur,
                      full: bool):
        """wva_ctx_ensemble_pass on [P * S, n_cells] fp32 arrivals, row p * S +
        s being tick s of path path0 + p of an ensemble of ``dims`` = (E, S,
        Q), every path starting from ``cur`` (which the tick was staged with).
        The results stay on the device; with ``full`` the pass's records come
        back as rollout()'s first two arrays, else None."""
        n_total, n_steps, n_q = dims
        n_paths = cell_scen.shape[0] // n_steps
        cur = (np.ascontiguousarray(cur[0], dtype=np.int32),
               np.ascontiguousarray(cur[1], dtype=np.int32),
               np.ascontiguousarray(cur[2], dtype=np.float32))
        for a in cur:
            if a.shape != (self.n_srv,):
                raise ValueError(
                    f"per-server override has shape {a.shape}, expected ({self.n_srv},)"
                )
        out = [ctypes.c_void_p() for _ in range(2)]
        rc = self._lib.wva_ctx_ensemble_pass(
            self.ctx, n_total, n_steps, n_q, n_acc, path0, n_paths, cell_scen.ctypes.data,
            cur[0].ctypes.data, cur[1].ctypes.data, cur[2].ctypes.data, 1 if full else 0,
            *[ctypes.byref(p) for p in out],
        )
        if rc != 0:
            raise HipKernelError(f"wva_ctx_ensemble_pass failed: {rc}")
        if not full:
            return None
        rows = n_paths * n_steps
        return (_copy_out(out[0], ctypes.c_float, (rows, 6, self.n_srv)),
                _copy_out(out[1], ctypes.c_int32, (rows, 4, self.n_srv)))

    def ensemble_bands(self, dims, n_acc: int, ranks: np.ndarray, want_final: bool) -> dict:
        """wva_ctx_ensemble_bands after the last pass of an ensemble of
        ``dims`` = (E, S, Q): the per-row aggregates, the bands and the mode
        pair as numpy copies, ``final`` (int32 [E, 3, n_srv]) only with
        ``want_final``."""
        n_total, n_steps, n_q = dims
        rk = np.ascontiguousarray(ranks, dtype=np.int32)
        out = (ctypes.c_void_p * 10)()
        rc = self._lib.wva_ctx_ensemble_bands(self.ctx, rk.ctypes.data, n_q,
                                              1 if want_final else 0, out)
        if rc != 0:
            raise HipKernelError(f"wva_ctx_ensemble_bands failed: {rc}")
        n_srv = self.n_srv
        spec = (
            ("totals", ctypes.c_uint64, (n_total, n_steps, n_acc)),
            ("nowin", ctypes.c_int32, (n_total, n_steps)),
            ("changes", ctypes.c_int32, (n_total, n_steps)),
            ("cost", ctypes.c_double, (n_total, n_steps)),
            ("final", ctypes.c_int32, (n_total, 3, n_srv)),
            ("srv_reps_q", ctypes.c_int32, (n_q, n_steps, n_srv)),
            ("srv_cost_q", ctypes.c_float, (n_q, n_steps, n_srv)),
            ("mode", ctypes.c_int32, (n_steps, n_srv)),
            ("mode_paths", ctypes.c_int32, (n_steps, n_srv)),
            ("fleet_q", ctypes.c_int64, (n_q, n_steps, n_acc + 3)),
        )
        return {
            name: _copy_out(ctypes.c_void_p(out[i]), ctype, shape)
            for i, (name, ctype, shape) in enumerate(spec) if out[i]
        }

    def hold(self, cell_scen: np.ndarray, cell_held: np.ndarray, n_acc: int):
        """wva_ctx_hold on [S, n_cells] fp32 arrivals and int32 held replicas
        (-1: the scenario's allocation is not on the cell; the tick is staged
        and the buckets are set): fp32 [S, 6, n_srv] (itl, ttft, rho, rate,
        slo_rate, cost), int32 [S, 4, n_srv] (status, accelerator, held,
        needed), int64 status counts [S, 6] and int64 deficits [S, n_acc]."""
        n_scen = cell_scen.shape[0]
        if cell_held.shape != cell_scen.shape or cell_held.dtype != np.int32:
            raise ValueError("held replicas must be int32 of the arrivals' shape")
        out = [ctypes.c_void_p() for _ in range(4)]
        rc = self._lib.wva_ctx_hold(
            self.ctx, n_scen, n_acc, cell_scen.ctypes.data, cell_held.ctypes.data,
            *[ctypes.byref(p) for p in out],
        )
        if rc != 0:
            raise HipKernelError(f"wva_ctx_hold failed: {rc}")
        return (
            _copy_out(out[0], ctypes.c_float, (n_scen, 6, self.n_srv)),
            _copy_out(out[1], ctypes.c_int32, (n_scen, 4, self.n_srv)),
            _copy_out(out[2], ctypes.c_uint64, (n_scen, 6)).astype(np.int64),
            _copy_out(out[3], ctypes.c_uint64, (n_scen, n_acc)).astype(np.int64),
        )

    def plan_cells(self, n_scen: int) -> dict:
        """Per-cell outputs [S, n_cells] of the planning pass that just ran."""
        cells = {k: np.empty((n_scen, self.n_cells), dtype=d)
                 for k, d in zip(CELL_KEYS, _CELL_DTYPES)}
        dst = (ctypes.c_void_p * len(CELL_KEYS))(
            *[cells[k].ctypes.data_as(ctypes.c_void_p) for k in CELL_KEYS]
        )
        rc = self._lib.wva_ctx_plan_cells(self.ctx, dst)
        if rc != 0:
            raise HipKernelError(f"wva_ctx_plan_cells failed: {rc}")
        return cells
