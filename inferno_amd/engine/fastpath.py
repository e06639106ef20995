"""FastSweep — the production reconcile hot path.

The full snapshot builder (snapshot.py) loops per cell in Python; at fleet
scale that host time dominates the reconcile (the HIP sweep itself is ~ms).
FastSweep splits the snapshot into:

  * a STATIC cell structure built once per fleet topology (perf parms,
    SLO targets, cell->server segments, accelerator costs), and
  * a DYNAMIC refresh per reconcile (arrival rates, token averages,
    current-allocation penalty inputs): on the GPU path a native loop over
    the cells (ops/native/stage.cpp) behind the tick's one C call, with the
    vectorized numpy version (_refresh_dynamic) as its reference.

Per reconcile it uploads the refreshed SoA, launches wva_sweep + wva_winner,
and materializes ONLY the per-server winner records (not all candidate
cells). The slow path (SweepEngine) remains the oracle and serves greedy
limited mode, which needs the full candidate lists.

FastSweep is the fleet model, the public API with its input validation, and
the CPU golden paths; the device buffers, the native context and the ctypes
calls belong to NativeCtx (engine/native_ctx.py), held as ``_gpu``.
"""
from __future__ import annotations

import contextlib
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np

from ..config import SaturationPolicy
from ..core import create_allocation
from ..core.system import System
from ..ops.sweep import PLAN_MAX_S, run_greedy_native
from .native_ctx import CELL_KEYS, NativeCtx
from .snapshot import FLAG_CUR_EMPTY, FLAG_CUR_SAME, FLAG_HAS_CUR

_INT_KEYS = ("in_tok", "out_tok", "batch_n", "min_replicas", "perf_max_batch",
             "cur_replicas", "flags")
_FLOAT_KEYS = ("alpha", "beta", "gamma", "delta", "arrival_rate", "t_itl", "t_ttft",
               "t_tps", "acc_cost", "cur_cost")


@dataclass
class WinnerRecord:
    """Winner allocation per server (arrays indexed by segment)."""

    acc_idx: np.ndarray  # int32, -1 = none, -2 = zero-load empty
    num_replicas: np.ndarray  # int32
    batch: np.ndarray  # int32
    cost: np.ndarray  # float32
    value: np.ndarray
    itl: np.ndarray
    ttft: np.ndarray
    rho: np.ndarray
    max_rate: np.ndarray


@dataclass
class PlanResult:
    """What-if load plan: the unlimited-mode solution of S arrival-rate
    scenarios of one fleet (FastSweep.plan)."""

    winners: WinnerRecord  # every array [S, n_servers]
    replicas_by_acc: np.ndarray  # int64 [S, n_acc], columns = FastSweep.acc_names
    cost_total: np.ndarray  # float64 [S]: fp64 sum of the winners' fp32 cost
    infeasible_servers: np.ndarray  # int64 [S]: servers with acc_idx == -1
    arrival: np.ndarray  # float32 [S, n_servers]: the scenarios evaluated
    cells: Optional[dict] = None  # reconcile_cells() layout, arrays [S, n_cells]
    # capacity-limited plans only (plan(capacity=...)); None otherwise. The
    # winners are then the limited-mode solution: num_replicas is the granted
    # count, cost and value are scaled by granted/desired.
    desired_replicas: Optional[np.ndarray] = None  # int32 [S, n_servers]: pre-cut count
    unallocated_servers: Optional[np.ndarray] = None  # int64 [S]: candidates but no grant
    partial_servers: Optional[np.ndarray] = None  # int64 [S]: 0 < granted < desired
    capacity_left: Optional[np.ndarray] = None  # int64 [S, n_types]
    capacity_types: Optional[list] = None  # columns of capacity_left


@dataclass
class SloPlanResult:
    """What-if SLO plan: the unlimited-mode solution of T SLO-target sets
    times S arrival-rate scenarios of one fleet (FastSweep.plan_slo)."""

    winners: WinnerRecord  # every array [T, S, n_servers]
    replicas_by_acc: np.ndarray  # int64 [T, S, n_acc], columns = FastSweep.acc_names
    cost_total: np.ndarray  # float64 [T, S]: fp64 sum of the winners' fp32 cost
    infeasible_servers: np.ndarray  # int64 [T, S]: servers with acc_idx == -1
    arrival: np.ndarray  # float32 [S, n_servers]: the load scenarios evaluated
    t_ttft: np.ndarray  # float32 [T, n_servers]: the TTFT targets evaluated (msec, 0 = none)
    t_itl: np.ndarray  # float32 [T, n_servers]: the ITL targets evaluated
    cells: Optional[dict] = None  # reconcile_cells() layout, arrays [T, S, n_cells]


@dataclass
class TokenPlanResult:
    """What-if token-mix plan: the unlimited-mode solution of W sets of
    per-server average input / output token counts times S arrival-rate
    scenarios of one fleet (FastSweep.plan_tokens)."""

    winners: WinnerRecord  # every array [W, S, n_servers]
    replicas_by_acc: np.ndarray  # int64 [W, S, n_acc], columns = FastSweep.acc_names
    cost_total: np.ndarray  # float64 [W, S]: fp64 sum of the winners' fp32 cost
    infeasible_servers: np.ndarray  # int64 [W, S]: servers with acc_idx == -1
    arrival: np.ndarray  # float32 [S, n_servers]: the load scenarios evaluated
    in_tok: np.ndarray  # int32 [W, n_servers]: the average input tokens evaluated
    out_tok: np.ndarray  # int32 [W, n_servers]: the average output tokens evaluated
    cells: Optional[dict] = None  # reconcile_cells() layout, arrays [W, S, n_cells]


@dataclass
class RolloutResult:
    """Forecast rollout: what the controller does over S consecutive ticks of
    an arrival-rate forecast, every tick judged against the allocation the
    tick before it left behind (FastSweep.rollout)."""

    winners: WinnerRecord  # every array [S, n_servers]; row s = tick s
    replicas_by_acc: np.ndarray  # int64 [S, n_acc], columns = FastSweep.acc_names
    cost_total: np.ndarray  # float64 [S]: fp64 sum of the winners' fp32 cost
    infeasible_servers: np.ndarray  # int64 [S]: servers with acc_idx == -1
    arrival: np.ndarray  # float32 [S, n_servers]: the forecast evaluated
    # int64 [S]: servers whose current accelerator after the tick differs from
    # the one before it (empty is an accelerator of its own; from no current
    # allocation to any counts)
    acc_changes: np.ndarray
    # (cur_acc i32, cur_rep i32, cur_cost f32) after the last tick, in the form
    # of FastSweep.cur_override
    final_cur: tuple
    cells: Optional[dict] = None  # reconcile_cells() layout, arrays [S, n_cells]


# Verdict of one (scenario, server) slice of a hold analysis (FastSweep.hold),
# as ops/hip/wva_kernels.hip numbers them (WVA_HOLD_*), in order of precedence
# NOT_HELD, IDLE, INVALID, OVERLOADED, then OK or SLO_VIOLATED.
HOLD_OK = 0  # evaluated; the sizing is feasible and held >= needed replicas
HOLD_SLO_VIOLATED = 1  # evaluated; fewer replicas than the SLO needs, or unreachable SLO
HOLD_OVERLOADED = 2  # no replicas, or the per-replica rate is above the analyzer's range
HOLD_NOT_HELD = 3  # the allocation names no accelerator the server has a cell on
HOLD_IDLE = 4  # no arrivals or no output tokens
HOLD_INVALID = 5  # degenerate service rates: no model of the cell
HOLD_STATUS_NAMES = ("OK", "SLO_VIOLATED", "OVERLOADED", "NOT_HELD", "IDLE", "INVALID")
_HOLD_FLOATS = ("itl", "ttft", "rho", "rate", "slo_rate", "cost")  # device row order
_HOLD_INTS = ("status", "acc_idx", "held_replicas", "needed_replicas")
# wva_ctx_plan_cells' ten arrays under the names a hold pass gives them
_HOLD_CELL_KEYS = ("status", "held", "held_replicas", "needed_replicas", "cost", "slo_rate",
                   "itl", "ttft", "rho", "rate")


@dataclass
class HoldResult:
    """Hold analysis: what users see under S loads when the allocation does
    not move (FastSweep.hold). Arrays are [S, n_servers] unless noted."""

    status: np.ndarray  # int32, one of HOLD_*
    acc_idx: np.ndarray  # int32: the held accelerator, -1 where NOT_HELD
    held_replicas: np.ndarray  # int32: 0 where NOT_HELD
    # int32: ceil(total rate / sized per-replica rate), not raised to
    # min_replicas; 0 where IDLE; -1 where the SLO is unreachable on the held
    # accelerator, and where NOT_HELD or INVALID
    needed_replicas: np.ndarray
    itl: np.ndarray  # float32 msec; +inf where OVERLOADED
    ttft: np.ndarray  # float32 msec; +inf where OVERLOADED
    rho: np.ndarray  # float32; 1 where OVERLOADED
    rate: np.ndarray  # float32 req/s per held replica
    slo_rate: np.ndarray  # float32 req/min the held replicas carry within the SLO
    cost: np.ndarray  # float32: accelerator cost x held replicas
    arrival: np.ndarray  # float32: the loads evaluated
    counts: np.ndarray  # int64 [S, 6]: servers per status
    deficit_by_acc: np.ndarray  # int64 [S, n_acc]: sum of max(needed - held, 0), needed >= 0
    cells: Optional[dict] = None  # per-cell arrays [S, n_cells] of the same, plus cell metadata


# Longest forecast one rollout() takes, and the steps one device pass of it
# holds (at most PLAN_MAX_S): longer forecasts run as consecutive passes, each
# starting from the allocation the one before it ended with.
ROLLOUT_MAX_STEPS = 4096
ROLLOUT_CHUNK = PLAN_MAX_S

_WINNER_FIELDS = ("acc_idx", "num_replicas", "batch", "cost", "value", "itl", "ttft", "rho",
                  "max_rate")

# Forecast ensembles (FastSweep.rollout_ensemble): most paths, most rows (paths
# x ticks) and most quantiles of one call; the rows one device pass holds (at
# most PLAN_MAX_S; a pass holds whole paths, so a forecast of S ticks runs
# ENSEMBLE_PASS_ROWS // S paths per pass; lowered only by tests); and the bytes
# the device arena may take when INFERNO_ENSEMBLE_BYTES does not say.
ENSEMBLE_MAX_PATHS = 256
ENSEMBLE_MAX_ROWS = 4096
ENSEMBLE_MAX_QUANTILES = 8
ENSEMBLE_PASS_ROWS = PLAN_MAX_S
ENSEMBLE_BYTES = 1 << 30


@dataclass
class EnsemblePaths:
    """The per-path records of an ensemble (rollout_ensemble(return_paths=True))."""

    winners: WinnerRecord  # every array [E, S, n_servers]
    final_cur: tuple  # (cur_acc i32, cur_rep i32, cur_cost f32), each [E, n_servers]


@dataclass
class EnsembleResult:
    """Forecast ensemble: E rollouts of S ticks from one start allocation, and
    per tick the order statistics across the paths
    (FastSweep.rollout_ensemble). Q = number of quantiles; band q is the
    rank-``ranks[q]`` value (0 = smallest) among the E paths' values."""

    quantiles: np.ndarray  # float64 [Q]
    ranks: np.ndarray  # int64 [Q]: nearest rank of each quantile, 0-based
    arrival: np.ndarray  # float32 [E, S, n_servers]: the paths evaluated
    # per path and tick: rollout(arrival=arrival[e])'s fields of the same name
    path_replicas_by_acc: np.ndarray  # int64 [E, S, n_acc]
    path_infeasible_servers: np.ndarray  # int64 [E, S]
    path_acc_changes: np.ndarray  # int64 [E, S]
    # float64 [E, S]: the sequential fp64 sum, in server order, of the winners'
    # fp32 cost (rollout().cost_total sums pairwise: last bits may differ)
    path_cost_total: np.ndarray
    # fleet bands: order statistics of the four arrays above across the paths
    replicas_by_acc_q: np.ndarray  # int64 [Q, S, n_acc]
    cost_total_q: np.ndarray  # float64 [Q, S]
    infeasible_q: np.ndarray  # int64 [Q, S]
    acc_changes_q: np.ndarray  # int64 [Q, S]
    # server bands: order statistics of the winners' replicas and cost
    server_replicas_q: np.ndarray  # int32 [Q, S, n_servers]
    server_cost_q: np.ndarray  # float32 [Q, S, n_servers]
    # agreement: the most frequent winner code across the paths (-2 empty, -1
    # none, >= 0 accelerator; the smallest code on ties) and how many chose it
    acc_mode: np.ndarray  # int32 [S, n_servers]
    acc_mode_paths: np.ndarray  # int32 [S, n_servers]
    paths: Optional[EnsemblePaths] = None


def ensemble_ranks(quantiles, n_paths: int) -> np.ndarray:
    """Nearest rank (0-based, ascending order) of every quantile among
    ``n_paths`` values: clamp(ceil(q * E) - 1, 0, E - 1) with q taken as the
    decimal its repr shows, in exact rational arithmetic: 0.9 of 10 is rank 8,
    and 0.07 of 100 rank 6, where binary floating point's 0.07 * 100 lies
    above 7 and would give rank 7."""
    import math
    from fractions import Fraction

    return np.array(
        [min(max(math.ceil(Fraction(repr(float(q))) * n_paths) - 1, 0), n_paths - 1)
         for q in quantiles], dtype=np.int64)


def ensemble_bands(values: np.ndarray, ranks) -> np.ndarray:
    """Order statistics across the leading (path) axis: [E, ...] -> [Q, ...],
    row q holding the rank-``ranks[q]`` value of every column."""
    return np.sort(values, axis=0)[np.asarray(ranks, dtype=np.int64)]


def ensemble_mode(codes: np.ndarray):
    """(mode, count) across the leading (path) axis of integer winner codes
    >= -2: per column the most frequent code, the smallest on ties, and how
    many paths hold it; both int32 of the trailing shape."""
    codes = np.asarray(codes)
    top = int(codes.max()) if codes.size else -2
    # counts[c + 2] = paths that hold code c (a bincount per column)
    counts = np.stack([(codes == c).sum(axis=0) for c in range(-2, top + 1)])
    mode = counts.argmax(axis=0)  # the first, i.e. smallest, code among the most frequent
    return (mode - 2).astype(np.int32), counts.max(axis=0).astype(np.int32)


def ensemble_path_cost(cost: np.ndarray) -> np.ndarray:
    """Sequential fp64 sum over the last (server) axis of fp32 costs, in index
    order from +0.0: what the device's per-row sum computes."""
    cost = np.asarray(cost, dtype=np.float32)
    if cost.shape[-1] == 0:
        return np.zeros(cost.shape[:-1], dtype=np.float64)
    return np.cumsum(cost.astype(np.float64), axis=-1)[..., -1]


def noisy_paths(scales, sigma: float, n_paths: int, seed: int) -> np.ndarray:
    """E sampled load paths around a forecast: [n_paths, S] factors
    scale[s] * exp(sigma * z[e, s]) with z standard normal from
    np.random.Generator(np.random.PCG64(seed)); path 0 is the forecast itself."""
    sc = np.asarray(scales, dtype=np.float64)
    if sc.ndim != 1 or sc.shape[0] < 1:
        raise ValueError(f"scales must be 1-D and non-empty, got shape {sc.shape}")
    if not np.isfinite(sc).all() or (sc < 0).any():
        raise ValueError("scales must be finite and non-negative")
    if not (np.isfinite(sigma) and sigma >= 0):
        raise ValueError(f"sigma must be finite and non-negative, got {sigma}")
    if n_paths < 1:
        raise ValueError(f"n_paths must be at least 1, got {n_paths}")
    z = np.random.Generator(np.random.PCG64(seed)).standard_normal((n_paths, sc.shape[0]))
    z[0] = 0.0
    return sc[None, :] * np.exp(float(sigma) * z)

# the four SaturationPolicy names as ops/native/greedy.cpp numbers them
_POLICY_CODE = {"None": 0, "PriorityExhaustive": 1, "PriorityRoundRobin": 2, "RoundRobin": 3}

# Which solver a capacity-limited GPU plan uses when INFERNO_PLAN_GREEDY does
# not say: "device" (wva_plan_greedy, one wave per scenario) or "host" (the
# native greedy per scenario over the downloaded cells). Both give the same
# bytes. At 16 scenarios of the flagship fleet the device path measured slower
# than the host loop, so the host loop is the default and the kernel is the
# opt-in (docs/design/kernels.md, "Capacity-limited planning").
PLAN_GREEDY_DEFAULT = "host"
# The round-robin policies hand out capacity one unit per step on a single
# lane; above this many units in a scenario's inventory they take the host
# loop, where a step costs nanoseconds.
PLAN_GREEDY_RR_MAX_UNITS = 1 << 18


def greedy_candidates(feasible, zero_empty, value, num_replicas, cell_server, cell_tidx,
                      units, n_srv):
    """Candidate rows of the native greedy (ops/native/greedy.cpp) from
    per-cell sweep outputs: the feasible cells in a stable order by (server,
    float64(value)), so ties keep accelerator-name order exactly like
    sorted(all_allocations.values(), key=value); zero-load cells get type -1
    and drop like the Python accelerator-lookup miss.

    Returns (order, seg_start, cand_value, cand_type, cand_units,
    cand_replicas); order[k] is the cell of candidate row k."""
    idx = np.nonzero(np.asarray(feasible).astype(bool))[0]
    srv_of = np.asarray(cell_server)
    order = idx[np.lexsort((value[idx].astype(np.float64), srv_of[idx]))]
    counts = np.bincount(srv_of[order], minlength=n_srv)
    seg = np.zeros(n_srv + 1, dtype=np.int32)
    np.cumsum(counts, out=seg[1:])
    cand_value = np.ascontiguousarray(value[order], dtype=np.float32)
    cand_tidx = np.where(
        np.asarray(zero_empty)[order].astype(bool), -1, cell_tidx[order]
    ).astype(np.int32)
    cand_units = np.ascontiguousarray(units[order], dtype=np.int32)
    cand_reps = np.ascontiguousarray(num_replicas[order], dtype=np.int32)
    return order, seg, cand_value, cand_tidx, cand_units, cand_reps


class FastSweep:
    def __init__(self, system: System, server_names: Optional[list[str]] = None,
                 backend: str = "gpu", device: str = "cuda"):
        self.system = system
        self.backend = backend
        self.device = device
        self.server_names = (
            list(server_names) if server_names is not None else sorted(system.servers)
        )
        self.acc_names = sorted(system.accelerators)
        self._acc_index = {n: i for i, n in enumerate(self.acc_names)}
        self._build_static()

    # ------------------------------------------------------------------
    def _build_static(self) -> None:
        system = self.system
        cell_server: list[int] = []
        cell_acc_idx: list[int] = []
        stat = {k: [] for k in ("alpha", "beta", "gamma", "delta", "acc_cost",
                                "t_itl", "t_ttft", "t_tps",
                                "perf_max_batch_cfg", "at_tokens", "override",
                                "min_replicas")}
        seg_start = [0]
        self._srv_objs = []
        for seg, name in enumerate(self.server_names):
            server = system.servers[name]
            self._srv_objs.append(server)
            model = system.models.get(server.model_name)
            svc = system.service_classes.get(server.service_class_name)
            target = svc.model_target(server.model_name) if svc is not None else None
            if model is not None and target is not None:
                for acc_name in sorted(server.candidate_accelerators(system)):
                    acc = system.accelerators[acc_name]
                    perf = model.get_perf_data(acc_name)
                    if perf is None:
                        continue
                    cell_server.append(seg)
                    cell_acc_idx.append(self._acc_index[acc_name])
                    stat["alpha"].append(perf.decodeParms.alpha)
                    stat["beta"].append(perf.decodeParms.beta)
                    stat["gamma"].append(perf.prefillParms.gamma)
                    stat["delta"].append(perf.prefillParms.delta)
                    stat["acc_cost"].append(acc.cost * model.get_num_instances(acc_name))
                    stat["t_itl"].append(target.itl)
                    stat["t_ttft"].append(target.ttft)
                    stat["t_tps"].append(target.tps)
                    stat["perf_max_batch_cfg"].append(perf.maxBatchSize)
                    stat["at_tokens"].append(perf.atTokens)
                    stat["override"].append(server.max_batch_size)
                    stat["min_replicas"].append(server.min_num_replicas)
            seg_start.append(len(cell_server))

        self.n_cells = len(cell_server)
        self.cell_server = np.asarray(cell_server, dtype=np.int64)
        self.cell_acc_idx = np.asarray(cell_acc_idx, dtype=np.int32)
        self.seg_start = np.asarray(seg_start, dtype=np.int32)
        self._stat = {
            k: np.asarray(v, dtype=np.float32 if k in
                          ("alpha", "beta", "gamma", "delta", "acc_cost",
                           "t_itl", "t_ttft", "t_tps") else np.int32)
            for k, v in stat.items()
        }

    def greedy_static(self):
        """Static greedy (limited-mode) inputs, cached per fleet topology:
        (type_names, per-cell type index, per-cell units per replica,
        per-server priority). type_names is the sorted union of the
        accelerators' types and system.capacity's keys."""
        cached = getattr(self, "_greedy_static_cache", None)
        if cached is not None:
            return cached
        system = self.system
        type_names = sorted(
            {acc.type for acc in system.accelerators.values()} | set(system.capacity)
        )
        type_index = {t: i for i, t in enumerate(type_names)}
        acc_tidx = np.empty(len(self.acc_names), dtype=np.int32)
        for i, an in enumerate(self.acc_names):
            acc_tidx[i] = type_index[system.accelerators[an].type]
        units = np.empty(self.n_cells, dtype=np.int32)
        for k in range(self.n_cells):
            srv = self._srv_objs[self.cell_server[k]]
            acc_name = self.acc_names[self.cell_acc_idx[k]]
            acc = system.accelerators[acc_name]
            model = system.models[srv.model_name]
            units[k] = model.get_num_instances(acc_name) * acc.multiplicity
        prio = np.array([s.priority(system) for s in self._srv_objs], dtype=np.int32)
        cell_tidx = acc_tidx[self.cell_acc_idx]
        cached = (type_names, cell_tidx, units, prio)
        self._greedy_static_cache = cached
        return cached

    @property
    def capacity_types(self) -> list:
        """Accelerator types in the column order of plan()'s capacity array."""
        return list(self.greedy_static()[0])

    # ------------------------------------------------------------------
    # Array overrides for the steady-state loop: when set, the per-server
    # Python object reads are skipped entirely (the bench/controller can
    # maintain these arrays from winner records between reconciles).
    # load_override = (arrival f32, in_tok i32, out_tok i32) per local server;
    # cur_override = (cur_acc i32 [-3 none, -1 empty, >=0 acc index],
    #                 cur_replicas i32, cur_cost f32).
    load_override = None
    cur_override = None

    def _base_load(self):
        """(arrival f32, in_tok i32, out_tok i32) per server: the load
        override when set, else the server objects."""
        n_srv = len(self.server_names)
        if self.load_override is not None:
            arrival, in_tok, out_tok = self.load_override
            arrival = np.asarray(arrival, dtype=np.float32)
            in_tok = np.asarray(in_tok, dtype=np.int32)
            out_tok = np.asarray(out_tok, dtype=np.int32)
        else:
            arrival = np.empty(n_srv, dtype=np.float32)
            in_tok = np.empty(n_srv, dtype=np.int32)
            out_tok = np.empty(n_srv, dtype=np.int32)
            for i, server in enumerate(self._srv_objs):
                load = server.load
                arrival[i] = load.arrivalRate if load is not None else 0.0
                in_tok[i] = load.avgInTokens if load is not None else 0
                out_tok[i] = load.avgOutTokens if load is not None else 0
        return arrival, in_tok, out_tok

    def _base_cur(self):
        """(cur_acc i32 [-3 none, -1 empty, >= 0 accelerator index],
        cur_replicas i32, cur_cost f32) per server: the current-allocation
        override when set, else the server objects."""
        n_srv = len(self.server_names)
        if self.cur_override is not None:
            cur_acc, cur_rep, cur_cost = self.cur_override
            cur_acc = np.asarray(cur_acc, dtype=np.int32)
            cur_rep = np.asarray(cur_rep, dtype=np.int32)
            cur_cost = np.asarray(cur_cost, dtype=np.float32)
        else:
            cur_acc = np.empty(n_srv, dtype=np.int32)  # -1 empty, -3 no cur
            cur_rep = np.zeros(n_srv, dtype=np.int32)
            cur_cost = np.zeros(n_srv, dtype=np.float32)
            for i, server in enumerate(self._srv_objs):
                cur = server.cur_allocation
                if cur is None:
                    cur_acc[i] = -3
                else:
                    cur_acc[i] = self._acc_index.get(cur.accelerator, -1)
                    cur_rep[i] = cur.num_replicas
                    cur_cost[i] = cur.cost
        return cur_acc, cur_rep, cur_cost

    def _refresh_dynamic(self, plan_arrival: Optional[np.ndarray] = None) -> dict:
        """Gather per-server dynamic state into per-cell arrays (vectorized).

        ``plan_arrival`` ([S, n_servers] fp32, scenario planning) replaces the
        per-server arrival rate by its maximum over the scenarios: a cell then
        counts as zero-load only where no scenario loads it, so every loaded
        cell keeps the batch size a single reconcile of that scenario uses."""
        arrival, in_tok, out_tok = self._base_load()
        if plan_arrival is not None:
            arrival = plan_arrival.max(axis=0).astype(np.float32)
        cur_acc, cur_rep, cur_cost = self._base_cur()

        cs = self.cell_server
        c_out = out_tok[cs]
        # batch sizing depends only on out_tok (and static profile fields);
        # steady-state fleets keep token averages stable, so cache it
        key = out_tok.tobytes()
        cached = getattr(self, "_batch_cache", None)
        if cached is not None and cached[0] == key:
            base_batch, pmb = cached[1], cached[2]
        else:
            safe_k = np.maximum(c_out, 1)
            n_scaled = np.maximum(
                (self._stat["perf_max_batch_cfg"].astype(np.int64)
                 * self._stat["at_tokens"].astype(np.int64)) // safe_k,
                1,
            )
            # uncapped like the reference (allocation.go:80-86); huge-N cells
            # dispatch to the GMEM spill bucket in choose_buckets
            base_batch = np.where(
                self._stat["override"] > 0, self._stat["override"], n_scaled
            ).astype(np.int32)
            pmb = np.where(
                self._stat["override"] > 0, self._stat["override"],
                self._stat["perf_max_batch_cfg"],
            ).astype(np.int32)
            self._batch_cache = (key, base_batch, pmb)
        # zero-load cells take the in-kernel zero path; batch_n is unused
        # there but must stay small so it doesn't inflate the LDS budget
        zero_load = (arrival[cs] == 0) | (c_out == 0)
        batch_n = np.where(zero_load, 1, base_batch).astype(np.int32)

        c_cur_acc = cur_acc[cs]
        flags = np.where(c_cur_acc != -3, FLAG_HAS_CUR, 0).astype(np.int32)
        flags |= np.where(c_cur_acc == self.cell_acc_idx, FLAG_CUR_SAME, 0)
        flags |= np.where(c_cur_acc == -1, FLAG_CUR_EMPTY, 0)

        return {
            "in_tok": in_tok[cs],
            "out_tok": c_out,
            "batch_n": batch_n,
            "min_replicas": self._stat["min_replicas"],
            "perf_max_batch": pmb,
            "cur_replicas": cur_rep[cs],
            "flags": flags,
            "alpha": self._stat["alpha"],
            "beta": self._stat["beta"],
            "gamma": self._stat["gamma"],
            "delta": self._stat["delta"],
            "arrival_rate": arrival[cs],
            "t_itl": self._stat["t_itl"],
            "t_ttft": self._stat["t_ttft"],
            "t_tps": self._stat["t_tps"],
            "acc_cost": self._stat["acc_cost"],
            "cur_cost": cur_cost[cs],
        }

    def cell_arrays(self) -> dict:
        """Torch CPU tensors of the refreshed snapshot (test/inspection API)."""
        import torch

        arrs = self._refresh_dynamic()
        out = {}
        for k in _INT_KEYS:
            out[k] = torch.from_numpy(np.ascontiguousarray(arrs[k], dtype=np.int32))
        for k in _FLOAT_KEYS:
            out[k] = torch.from_numpy(np.ascontiguousarray(arrs[k], dtype=np.float32))
        return out

    # ------------------------------------------------------------------
    def reconcile(self) -> WinnerRecord:
        if self.backend == "gpu":
            return self._reconcile_gpu()
        return self._reconcile_cpu()

    # GPU persistent-state reconcile (NativeCtx): static SoA uploaded once; per
    # step the native library expands the per-server state into ONE pinned
    # dynamic block -> one H2D copy; the bucket layout is kept until the staged
    # batch_n differs from the one it was chosen for; outputs preallocated;
    # winner records selected and gathered ON-DEVICE in one launch and
    # downloaded in a single D2H copy.
    def _tick(self, plan_arrival: Optional[np.ndarray] = None, launch: bool = True,
              cur=None) -> None:
        """One native tick (wva_ctx_tick): the library expands the six
        per-server arrays into the pinned dynamic block — what
        _refresh_dynamic() computes, byte for byte — and, with ``launch``,
        runs the whole device pipeline and synchronises. When the staged
        batch_n no longer fits the context's bucket layout the library
        launches nothing and says so; the layout is then chosen here as
        before and the already staged tick resumed (wva_reconcile).

        ``plan_arrival`` as in _refresh_dynamic; the planning passes stage
        with ``launch=False`` and run their own pipeline afterwards; ``cur``
        (a rollout pass) replaces _base_cur()'s triple. The device state is
        set up on the first call."""
        g = getattr(self, "_gpu", None)
        if g is None:
            g = self._gpu = NativeCtx(len(self.server_names), self._stat, self.cell_server,
                                      self.cell_acc_idx, self.seg_start, self.device)
        arrival, in_tok, out_tok = self._base_load()
        zero = None
        if plan_arrival is not None:
            arrival = plan_arrival.max(axis=0).astype(np.float32)
            zero = arrival
        cur_acc, cur_rep, cur_cost = cur if cur is not None else self._base_cur()
        n_srv = len(self.server_names)
        f32, i32 = np.float32, np.int32
        srv = (
            np.ascontiguousarray(arrival, dtype=f32), np.ascontiguousarray(in_tok, dtype=i32),
            np.ascontiguousarray(out_tok, dtype=i32), np.ascontiguousarray(cur_acc, dtype=i32),
            np.ascontiguousarray(cur_rep, dtype=i32), np.ascontiguousarray(cur_cost, dtype=f32),
        )
        for a in srv:
            if a.shape != (n_srv,):
                raise ValueError(
                    f"per-server override has shape {a.shape}, expected ({n_srv},)"
                )
        if g.tick(srv, zero, launch):  # layout stale: staged, nothing launched
            mode = 1 if getattr(self.system, "analyzer_mode", "mm1k") == "mg1" else 0
            cv2 = float(getattr(self.system, "analyzer_cv2", 1.0))
            g.sync_buckets(g.staged_batch_n(), mode, cv2)
            if launch:
                g.resume()

    def _winner_block(self) -> tuple[np.ndarray, np.ndarray]:
        """The last tick's winner records, copied out of the pinned block:
        (fp32 [6, n_srv], int32 [4, n_srv])."""
        return self._gpu.winner_block()

    def memo_stats(self) -> Optional[tuple[int, int]]:
        """(hits, misses) of the native context's sizing memo since the
        context was created, or None when there is no context yet or the
        memo is off (INFERNO_SIZING_MEMO=0). Synchronous; diagnostics only."""
        g = getattr(self, "_gpu", None)
        return g.memo_stats() if g is not None else None

    def _with_cell_meta(self, cells: dict) -> dict:
        cells["cell_server"] = self.cell_server
        cells["cell_acc_idx"] = self.cell_acc_idx
        cells["seg_start"] = self.seg_start
        return cells

    def reconcile_cells(self) -> Optional[dict]:
        """Run the sweep and return PER-CELL output arrays (numpy) plus the
        cell metadata — the input the greedy limited-mode solver needs (full
        candidate lists, not just argmin winners). GPU backend only; returns
        None on CPU (the slow engine path covers it)."""
        if self.backend != "gpu" or self.n_cells == 0:
            return None
        self._tick()  # fully synced on return
        return self._with_cell_meta(self._gpu.cells())

    def _reconcile_gpu(self) -> WinnerRecord:
        if self.n_cells == 0:
            return _empty_winner(len(self.server_names))
        self._tick()
        return _winner_record(*self._gpu.winner_block())  # one copy; the rows are views of it

    # ------------------------------------------------------------------
    # What-if load planning
    # ------------------------------------------------------------------
    def plan(self, scales=None, arrival=None, return_cells: bool = False, capacity=None,
             saturation_policy: str = "None", delayed_best_effort: bool = False) -> PlanResult:
        """Solve S arrival-rate scenarios of the fleet in one pass.

        Exactly one of ``scales`` (S non-negative factors applied to the base
        arrival rates, as ``float32(base) * float32(scale)``) and ``arrival``
        (explicit [S, n_servers] float32 rates, req/min) is given; 1 <= S <=
        256. Token averages, current allocations and everything else are the
        same in every scenario. Scenario s of the result is what reconcile()
        returns with that scenario's arrival rates as the load.

        On the GPU each cell is sized once (or takes its sizing-memo hit) and
        every scenario is evaluated against that sizing; the memo is shared
        with reconcile(), so planning's hits and misses — one per loaded cell
        and call, not per scenario — show up in memo_stats(). Planning does
        not change what a following reconcile() returns.

        ``capacity`` makes it a limited-mode plan: scenario s is solved by the
        delta-regret greedy (solver/greedy.py) against an inventory of
        accelerator units, with ``saturation_policy`` (a SaturationPolicy
        name) and ``delayed_best_effort`` as in OptimizerSpec. A mapping of
        accelerator type to units applies to every scenario (missing types
        count as 0); an integer array [S, n_types] with columns in
        ``capacity_types`` order sets it per scenario. The winners are then
        the granted allocations (acc_idx -1 where a server got nothing or has
        zero load) and the result's limited-mode fields are filled in. On the
        GPU the scenarios are solved by the native host greedy over the
        downloaded cells; INFERNO_PLAN_GREEDY=device runs one greedy per
        scenario on the device instead (wva_plan_greedy), with the same result.
        """
        scen = self._plan_scenarios(scales, arrival)
        if capacity is not None:
            return self._plan_limited(scen, capacity, saturation_policy, delayed_best_effort,
                                      return_cells)
        if self.backend == "gpu":
            winners, totals, cells = self._plan_gpu(scen, return_cells)
        else:
            winners, totals, cells = self._plan_cpu(scen), None, None
        return self._plan_result(scen, winners, totals, cells)

    def _plan_result(self, scen, winners: WinnerRecord, totals, cells, **limited) -> PlanResult:
        """The PlanResult of a solved plan; ``totals`` None = count the
        winners' replicas here. ``limited``: the limited-mode fields."""
        totals, cost_total, infeasible = self._plan_totals(winners, totals)
        return PlanResult(
            winners=winners,
            replicas_by_acc=totals,
            cost_total=cost_total,
            infeasible_servers=infeasible,
            arrival=scen,
            cells=cells,
            **limited,
        )

    def _plan_totals(self, winners: WinnerRecord, totals):
        """(replicas_by_acc, cost_total, infeasible_servers) of solved winners
        [n_scen, n_servers]; ``totals`` None = count the winners' replicas
        here."""
        n_scen = winners.acc_idx.shape[0]
        has = winners.acc_idx != -1
        if totals is None:
            totals = np.zeros((n_scen, len(self.acc_names)), dtype=np.int64)
            for s in range(n_scen):
                on = winners.acc_idx[s] >= 0
                np.add.at(totals[s], winners.acc_idx[s][on],
                          winners.num_replicas[s][on].astype(np.int64))
        # fp64 sum of the fp32 costs in server order (the device keeps no
        # fp32 running total: its order of additions would not be fixed)
        cost_total = np.array(
            [winners.cost[s][has[s]].astype(np.float64).sum() for s in range(n_scen)],
            dtype=np.float64,
        )
        return totals, cost_total, (~has).sum(axis=1).astype(np.int64)

    def _plan_scenarios(self, scales, arrival, limit: int = PLAN_MAX_S,
                        who: str = "plan()", rows: str = "scenarios") -> np.ndarray:
        """Validate plan()'s input (at most ``limit`` rows; ``who`` and ``rows``
        name the caller in the messages) and return the [S, n_servers] fp32
        rates."""
        if (scales is None) == (arrival is None):
            raise ValueError(f"{who} takes exactly one of scales and arrival")
        n_srv = len(self.server_names)
        if scales is not None:
            try:
                sc = np.asarray(scales, dtype=np.float64)
            except (TypeError, ValueError) as e:
                raise ValueError(f"scales is not numeric: {e}") from None
            if sc.ndim != 1:
                raise ValueError(f"scales must be 1-D, got shape {sc.shape}")
            vals, what = sc, "scales"
        else:
            try:
                arr = np.asarray(arrival, dtype=np.float64)
            except (TypeError, ValueError) as e:
                raise ValueError(f"arrival is not numeric: {e}") from None
            if arr.ndim != 2 or arr.shape[1] != n_srv:
                raise ValueError(
                    f"arrival must have shape [S, {n_srv}], got {arr.shape}"
                )
            vals, what = arr, "arrival"
        n_scen = vals.shape[0]
        if not 1 <= n_scen <= limit:
            raise ValueError(f"{who} takes 1..{limit} {rows}, got {n_scen}")
        if not np.isfinite(vals).all() or (vals < 0).any():
            raise ValueError(f"{what} must be finite and non-negative")
        if scales is not None:
            base = self._base_load()[0]
            scen = base[None, :] * vals.astype(np.float32)[:, None]
        else:
            scen = vals.astype(np.float32)
        scen = np.ascontiguousarray(scen, dtype=np.float32)
        if not np.isfinite(scen).all():
            raise ValueError(f"{what} overflows float32")
        return scen

    def _plan_gpu(self, scen: np.ndarray, return_cells: bool):
        n_scen, n_srv = scen.shape
        n_acc = len(self.acc_names)
        if self.n_cells == 0 or n_acc == 0:
            return _empty_winners(n_scen, n_srv), np.zeros((n_scen, n_acc), dtype=np.int64), None
        self._tick(plan_arrival=scen, launch=False)  # stage + bucket layout
        cell_scen = np.ascontiguousarray(scen[:, self.cell_server], dtype=np.float32)
        of, oi, totals = self._gpu.plan(cell_scen, n_acc)
        cells = self._plan_cells_gpu(n_scen) if return_cells else None
        return _winner_record(of, oi), totals, cells

    def _plan_cells_gpu(self, n_scen: int) -> dict:
        """Per-cell outputs of the planning pass that just ran."""
        return self._with_cell_meta(self._gpu.plan_cells(n_scen))

    # ------------------------------------------------------------------
    # Forecast rollout
    # ------------------------------------------------------------------
    def rollout(self, scales=None, arrival=None, return_cells: bool = False) -> RolloutResult:
        """Replay S consecutive reconciles of an arrival-rate forecast.

        Input as for plan(): exactly one of ``scales`` (S step factors on the
        base arrival rates) and ``arrival`` ([S, n_servers] req/min); 1 <= S
        <= ROLLOUT_MAX_STEPS. The rows are consecutive ticks, not
        alternatives. Tick 0 runs against the current allocation (the
        current-allocation override when set, else the server objects); tick
        s >= 1 against what tick s - 1 left behind: unchanged where it found
        no feasible cell (acc_idx -1), empty after a zero-load empty winner
        (-2), else the winner's accelerator, replicas and cost. Tick s of the
        result is what reconcile() returns with row s as the load and that
        allocation as the current one; with ``return_cells`` the per-cell
        arrays of reconcile_cells() come with it.

        On the GPU the per-cell work is plan()'s pass (each cell sized once,
        the sizing memo shared: one hit or miss per loaded cell and pass) and
        the per-server chain over the ticks runs in one kernel; forecasts
        longer than ROLLOUT_CHUNK ticks run as consecutive passes. A rollout
        changes nothing a following reconcile(), plan() or plan_slo()
        returns, and leaves the server objects as they were."""
        scen = self._plan_scenarios(scales, arrival, ROLLOUT_MAX_STEPS, "rollout()", "steps")
        start = tuple(np.array(a) for a in self._base_cur())
        if self.backend == "gpu":
            winners, totals, cells, final_cur = self._rollout_gpu(scen, start, return_cells)
        else:
            winners, final_cur = self._rollout_cpu(scen, start)
            totals = cells = None
        totals, cost_total, infeasible = self._plan_totals(winners, totals)
        return RolloutResult(
            winners=winners,
            replicas_by_acc=totals,
            cost_total=cost_total,
            infeasible_servers=infeasible,
            arrival=scen,
            acc_changes=_acc_changes(start[0], winners.acc_idx),
            final_cur=final_cur,
            cells=cells,
        )

    def _rollout_gpu(self, scen: np.ndarray, cur, return_cells: bool):
        n_steps, n_srv = scen.shape
        n_acc = len(self.acc_names)
        if self.n_cells == 0 or n_acc == 0:
            return (_empty_winners(n_steps, n_srv), np.zeros((n_steps, n_acc), dtype=np.int64),
                    None, cur)
        chunk = max(1, min(int(ROLLOUT_CHUNK), PLAN_MAX_S))
        pf, pi, tot, cells = [], [], [], []
        for lo in range(0, n_steps, chunk):
            rows = scen[lo:lo + chunk]
            # stage with the allocation the pass starts from; a stale bucket
            # layout (the pass's own zero-load cells) is resynchronised there
            self._tick(plan_arrival=rows, launch=False, cur=cur)
            cell_scen = np.ascontiguousarray(rows[:, self.cell_server], dtype=np.float32)
            of, oi, totals, cur = self._gpu.rollout(cell_scen, n_acc, cur)
            pf.append(of)
            pi.append(oi)
            tot.append(totals)
            if return_cells:
                cells.append(self._gpu.plan_cells(rows.shape[0]))
        all_cells = None
        if return_cells:
            all_cells = self._with_cell_meta(
                {k: np.concatenate([c[k] for c in cells]) for k in CELL_KEYS})
        return (_winner_record(np.concatenate(pf), np.concatenate(pi)), np.concatenate(tot),
                all_cells, cur)

    def _rollout_cpu(self, scen: np.ndarray, cur):
        """Golden path: one _reconcile_cpu per step with the step's arrival
        rates and the fed-back current allocation put on the server objects,
        which are restored afterwards in any case. Step 0 runs against the
        objects' own current allocations unless the override is set."""
        from ..core.allocation import Allocation

        saved = [srv.cur_allocation for srv in self._srv_objs]

        def put_cur(which):
            for i in np.nonzero(which)[0]:
                acc = int(cur[0][i])
                self._srv_objs[i].cur_allocation = None if acc == -3 else Allocation(
                    accelerator=self.acc_names[acc] if acc >= 0 else "",
                    num_replicas=int(cur[1][i]), cost=float(cur[2][i]),
                )

        rows = []
        try:
            with self._scenario_loads() as set_loads:
                if self.cur_override is not None:
                    put_cur(np.ones(len(self._srv_objs), dtype=bool))
                for row in scen:
                    set_loads(row)
                    w = self._reconcile_cpu()
                    rows.append(w)
                    cur = feed_back(cur, w)
                    put_cur(w.acc_idx != -1)  # the others keep what they had
        finally:
            for srv, old in zip(self._srv_objs, saved):
                srv.cur_allocation = old
        winners = WinnerRecord(**{
            f: np.stack([getattr(r, f) for r in rows]) for f in _WINNER_FIELDS
        })
        return winners, cur

    # ------------------------------------------------------------------
    # Forecast ensembles
    # ------------------------------------------------------------------
    def rollout_ensemble(self, scales=None, arrival=None, quantiles=(0.5, 0.9, 1.0),
                         return_paths: bool = False) -> EnsembleResult:
        """Roll out E sampled load paths of S ticks and return, per tick, order
        statistics across the paths.

        Exactly one of ``scales`` ([E, S] factors on the base arrival rates,
        formed as ``float32(base) * float32(scale)`` as plan() does) and
        ``arrival`` ([E, S, n_servers] req/min) is given; 1 <= E <=
        ENSEMBLE_MAX_PATHS, 1 <= S <= PLAN_MAX_S, E * S <= ENSEMBLE_MAX_ROWS.
        Every path starts from the same current allocation, as rollout() does;
        path e is, by definition, ``rollout(arrival=arrival[e])``.

        ``quantiles``: 1 to ENSEMBLE_MAX_QUANTILES values in (0, 1]. Quantile q
        is the nearest-rank order statistic on the ascending order, rank
        ``ensemble_ranks`` (exact rational arithmetic on the decimal q is
        written as: 0.9 of 10 paths is rank 8). A band is that order statistic
        of one number across the E paths; bands of different numbers, or of
        different servers, need not come from the same path.

        ``path_cost_total`` is the sequential fp64 sum, in server order, of the
        winners' fp32 cost (a server without a winner holds 0 and is added). It
        differs from ``rollout().cost_total``, which numpy sums pairwise, in the
        last bits at most. ``acc_mode`` is the winner code most paths chose for
        a (tick, server), ``acc_mode_paths`` how many did; where
        ``acc_mode_paths == E`` the server's replica band is over one
        accelerator and can be read as replicas of that accelerator.

        ``paths`` holds every path's winners and final allocation only with
        ``return_paths``. On the GPU a bands-only call downloads the bands, the
        mode pair and the per-path aggregates and nothing else: the per-cell
        work is plan()'s pass over ENSEMBLE_PASS_ROWS // S paths at a time
        (the sizing memo sees one lookup per loaded cell and pass), the chains
        of all paths of a pass run in one kernel and the selections in another.
        The device arena, about 12 * E * S * n_servers bytes, must not exceed
        INFERNO_ENSEMBLE_BYTES (default 1 GiB, read per call). A call changes
        nothing a following reconcile(), plan(), rollout() or hold() returns
        and leaves the server objects as they were."""
        scen = self._ensemble_scenarios(scales, arrival)
        n_paths, n_steps, n_srv = scen.shape
        qs, ranks = _ensemble_quantiles(quantiles, n_paths)
        n_acc = len(self.acc_names)
        need = _ensemble_arena_bytes(n_paths, n_steps, n_srv, n_acc, len(qs))
        env = os.environ.get("INFERNO_ENSEMBLE_BYTES")
        try:
            limit = int(env) if env else ENSEMBLE_BYTES
        except ValueError:
            raise ValueError(f"INFERNO_ENSEMBLE_BYTES must be an integer, got {env!r}") from None
        if need > limit:
            raise ValueError(
                f"rollout_ensemble() needs a device arena of {need} bytes for {n_paths} paths x "
                f"{n_steps} ticks x {n_srv} servers, above the limit of {limit} "
                "(INFERNO_ENSEMBLE_BYTES)")
        start = tuple(np.array(a) for a in self._base_cur())
        if self.backend == "gpu" and self.n_cells > 0 and n_acc > 0:
            return self._ensemble_gpu(scen, start, qs, ranks, return_paths)
        if self.backend == "gpu":
            rolled = [(_empty_winners(n_steps, n_srv), start)] * n_paths
        else:
            rolled = [self._rollout_cpu(scen[e], start) for e in range(n_paths)]
        winners = WinnerRecord(**{
            f: np.stack([getattr(w, f) for w, _ in rolled]) for f in _WINNER_FIELDS
        })
        final_cur = tuple(np.stack([cur[k] for _, cur in rolled]) for k in range(3))
        totals = np.stack([self._plan_totals(w, None)[0] for w, _ in rolled])
        bands = _ensemble_bands_of(winners, totals, start[0], ranks)
        return EnsembleResult(
            quantiles=qs, ranks=ranks, arrival=scen,
            paths=EnsemblePaths(winners, final_cur) if return_paths else None, **bands)

    def _ensemble_scenarios(self, scales, arrival) -> np.ndarray:
        """Validate rollout_ensemble()'s load input and return the [E, S,
        n_servers] fp32 rates."""
        who = "rollout_ensemble()"
        if (scales is None) == (arrival is None):
            raise ValueError(f"{who} takes exactly one of scales and arrival")
        n_srv = len(self.server_names)
        if scales is not None:
            try:
                vals = np.asarray(scales, dtype=np.float64)
            except (TypeError, ValueError) as e:
                raise ValueError(f"scales is not numeric: {e}") from None
            if vals.ndim != 2:
                raise ValueError(f"scales must have shape [E, S], got {vals.shape}")
            what = "scales"
        else:
            try:
                vals = np.asarray(arrival, dtype=np.float64)
            except (TypeError, ValueError) as e:
                raise ValueError(f"arrival is not numeric: {e}") from None
            if vals.ndim != 3 or vals.shape[2] != n_srv:
                raise ValueError(f"arrival must have shape [E, S, {n_srv}], got {vals.shape}")
            what = "arrival"
        n_paths, n_steps = vals.shape[:2]
        if not 1 <= n_paths <= ENSEMBLE_MAX_PATHS:
            raise ValueError(f"{who} takes 1..{ENSEMBLE_MAX_PATHS} paths, got {n_paths}")
        if not 1 <= n_steps <= PLAN_MAX_S:
            raise ValueError(f"{who} takes 1..{PLAN_MAX_S} steps, got {n_steps}")
        if n_paths * n_steps > ENSEMBLE_MAX_ROWS:
            raise ValueError(
                f"{who} takes at most {ENSEMBLE_MAX_ROWS} paths x steps, got "
                f"{n_paths} x {n_steps} = {n_paths * n_steps}")
        if not np.isfinite(vals).all() or (vals < 0).any():
            raise ValueError(f"{what} must be finite and non-negative")
        with np.errstate(over="ignore"):  # an overflow is reported below
            if scales is not None:
                base = self._base_load()[0]
                scen = base[None, None, :] * vals.astype(np.float32)[:, :, None]
            else:
                scen = vals.astype(np.float32)
        scen = np.ascontiguousarray(scen, dtype=np.float32)
        if not np.isfinite(scen).all():
            raise ValueError(f"{what} overflows float32")
        return scen

    def _ensemble_gpu(self, scen: np.ndarray, start, qs, ranks, return_paths: bool):
        n_paths, n_steps, n_srv = scen.shape
        n_acc = len(self.acc_names)
        dims = (n_paths, n_steps, len(qs))
        per_pass = max(1, min(int(ENSEMBLE_PASS_ROWS), PLAN_MAX_S) // n_steps)
        pf, pi = [], []
        for e0 in range(0, n_paths, per_pass):
            rows = scen[e0:e0 + per_pass].reshape(-1, n_srv)
            # staged exactly as a rollout pass: the pass's own zero-load cells
            # make the bucket layout stale, which is resynchronised there
            self._tick(plan_arrival=rows, launch=False, cur=start)
            cell_scen = np.ascontiguousarray(rows[:, self.cell_server], dtype=np.float32)
            rec = self._gpu.ensemble_pass(cell_scen, dims, e0, n_acc, start, return_paths)
            if return_paths:
                pf.append(rec[0])
                pi.append(rec[1])
        out = self._gpu.ensemble_bands(dims, n_acc, ranks, return_paths)
        paths = None
        if return_paths:
            w = _winner_record(np.concatenate(pf), np.concatenate(pi))
            winners = WinnerRecord(**{
                f: getattr(w, f).reshape(n_paths, n_steps, n_srv) for f in _WINNER_FIELDS
            })
            fin = out["final"]
            paths = EnsemblePaths(winners, (
                np.ascontiguousarray(fin[:, 0]), np.ascontiguousarray(fin[:, 1]),
                np.ascontiguousarray(fin[:, 2]).view(np.float32)))
        fleet = out["fleet_q"]
        return EnsembleResult(
            quantiles=qs, ranks=ranks, arrival=scen,
            path_replicas_by_acc=out["totals"].astype(np.int64),
            path_infeasible_servers=out["nowin"].astype(np.int64),
            path_acc_changes=out["changes"].astype(np.int64),
            path_cost_total=out["cost"],
            replicas_by_acc_q=np.ascontiguousarray(fleet[:, :, :n_acc]),
            cost_total_q=np.ascontiguousarray(fleet[:, :, n_acc + 2]).view(np.float64),
            infeasible_q=np.ascontiguousarray(fleet[:, :, n_acc]),
            acc_changes_q=np.ascontiguousarray(fleet[:, :, n_acc + 1]),
            server_replicas_q=out["srv_reps_q"], server_cost_q=out["srv_cost_q"],
            acc_mode=out["mode"], acc_mode_paths=out["mode_paths"], paths=paths)

    # ------------------------------------------------------------------
    # Hold analysis
    # ------------------------------------------------------------------
    def hold(self, scales=None, arrival=None, allocation=None,
             return_cells: bool = False) -> HoldResult:
        """Evaluate a FIXED allocation under S arrival-rate scenarios in one
        pass: the latency users see when the replicas do not follow the load
        (a capped deployment, an autoscaler that lags a ramp, the headroom of
        today's fleet). Every other pass resizes the fleet per scenario; this
        one pins the replicas.

        Load axis as for plan(): exactly one of ``scales`` and ``arrival``,
        1 <= S <= 256. ``allocation`` None holds the current allocation (the
        current-allocation override when set, else the server objects) in
        every scenario; else it is ``(acc_idx, num_replicas)``, two integer
        arrays of shape [n_servers] or [S, n_servers]. ``acc_idx`` >= 0 indexes
        ``acc_names``; any negative value means "holds nothing", so a
        WinnerRecord's -1 / -2 and a rollout's final_cur -1 / -3 pass straight
        in. ``num_replicas`` >= 0 where an accelerator is named.

        Per (scenario, server) the verdict is, in this order: HOLD_NOT_HELD
        (no accelerator named, or the server has no cell on it), HOLD_IDLE
        (zero arrival or no output tokens; latencies as the zero-load
        allocation reports them), HOLD_INVALID (degenerate service rates),
        HOLD_OVERLOADED (no replicas, or a per-replica rate the analyzer
        refuses: latencies +inf, rho 1), else one analysis at total rate /
        held replicas: HOLD_OK iff the SLO is reachable on the held
        accelerator and held >= needed_replicas, else HOLD_SLO_VIOLATED. The
        verdict compares integers, never latencies with targets.
        ``rollout()`` says what the controller will do over a forecast f;
        ``hold(arrival=f[1:], allocation=(r.winners.acc_idx[:-1],
        r.winners.num_replicas[:-1]))`` says whether the SLO holds while it
        catches up, under one tick of actuation lag.

        On the GPU only the held cell of a server is evaluated, once per
        scenario against one sizing (or its sizing-memo hit: the memo is shared
        with reconcile(), one lookup per held and loaded cell and call). A
        hold changes nothing a following reconcile() or plan returns and
        leaves the server objects as they were."""
        scen = self._plan_scenarios(scales, arrival, who="hold()")
        acc, rep = self._hold_allocation(allocation, scen.shape[0])
        n_scen, n_srv = scen.shape
        n_acc = len(self.acc_names)
        cells = None
        if self.n_cells == 0 or n_acc == 0:
            rec = _empty_hold(n_scen, n_srv)
            counts = deficit = None
        elif self.backend == "gpu":
            self._tick(plan_arrival=scen, launch=False)  # stage + bucket layout
            cs = self.cell_server
            cell_scen = np.ascontiguousarray(scen[:, cs], dtype=np.float32)
            cell_held = np.ascontiguousarray(
                np.where(acc[:, cs] == self.cell_acc_idx[None, :], rep[:, cs], -1), dtype=np.int32)
            hf, hi, counts, deficit = self._gpu.hold(cell_scen, cell_held, n_acc)
            rec = {k: np.ascontiguousarray(hf[:, r]) for r, k in enumerate(_HOLD_FLOATS)}
            rec.update({k: np.ascontiguousarray(hi[:, r]) for r, k in enumerate(_HOLD_INTS)})
            if return_cells:
                raw = self._gpu.plan_cells(n_scen)
                cells = self._with_cell_meta(
                    {new: raw[old] for new, old in zip(_HOLD_CELL_KEYS, CELL_KEYS)})
        else:
            rec = self._hold_cpu(scen, acc, rep)
            counts = deficit = None
        if counts is None:
            counts, deficit = _hold_sums(rec, n_acc)
        return HoldResult(arrival=scen, counts=counts, deficit_by_acc=deficit, cells=cells, **rec)

    def _hold_allocation(self, allocation, n_scen: int):
        """Validate hold()'s allocation and return (acc_idx, num_replicas) as
        int32 [S, n_servers]: acc_idx -1 wherever nothing is held (replicas 0
        there)."""
        n_srv = len(self.server_names)
        if allocation is None:
            cur_acc, cur_rep, _ = self._base_cur()
            raw = [np.asarray(cur_acc), np.asarray(cur_rep)]
        else:
            try:
                a, r = allocation
                raw = [np.asarray(a), np.asarray(r)]
                [x.astype(np.float64) for x in raw]
            except (TypeError, ValueError) as e:
                raise ValueError(
                    "allocation is not an (acc_idx, num_replicas) pair of integer arrays: "
                    f"{e}") from None
        vals = []
        for x, what in zip(raw, ("acc_idx", "num_replicas")):
            v = x.astype(np.float64)
            if v.shape not in ((n_srv,), (n_scen, n_srv)):
                raise ValueError(
                    f"allocation {what} must have shape [{n_srv}] or [{n_scen}, {n_srv}], "
                    f"got {v.shape}")
            if x.dtype.kind not in "iu" and not (np.isfinite(v).all() and (v == np.floor(v)).all()):
                raise ValueError(f"allocation {what} must hold integers")
            vals.append(np.broadcast_to(v, (n_scen, n_srv)))
        acc, rep = vals
        if (acc >= len(self.acc_names)).any():
            raise ValueError(
                f"allocation acc_idx must be below {len(self.acc_names)} (acc_names), "
                f"got {int(acc.max())}")
        on = acc >= 0
        if (rep[on] < 0).any():
            raise ValueError("allocation num_replicas must be non-negative where acc_idx >= 0")
        if (rep[on] > np.iinfo(np.int32).max).any():
            raise ValueError("allocation num_replicas must fit int32")
        return (np.ascontiguousarray(np.where(on, acc, -1), dtype=np.int32),
                np.ascontiguousarray(np.where(on, rep, 0), dtype=np.int32))

    def _hold_cpu(self, scen: np.ndarray, acc: np.ndarray, rep: np.ndarray) -> dict:
        """Golden path: per (scenario, server) the held cell's analyzer built
        as core/allocation.py builds it (M/G/1 mode included), size() for the
        sized rate and the needed replicas, analyze() at total rate / held
        replicas for the latencies, its refusal of the rate mapped to
        OVERLOADED. Reads the server objects and changes none."""
        from ..analyzer import (AnalyzerError, Configuration, DecodeParms, PrefillParms,
                                QueueAnalyzer, RequestSize, ServiceParms, TargetPerf)
        from ..config import MAX_QUEUE_TO_BATCH_RATIO

        system = self.system
        n_scen, n_srv = scen.shape
        rec = _empty_hold(n_scen, n_srv)
        _, in_tok, out_tok = self._base_load()
        targets, _ = self._server_targets()
        cell_of = {(int(self.cell_server[k]), int(self.cell_acc_idx[k])): k
                   for k in range(self.n_cells)}
        st = self._stat
        f32 = np.float32
        sized = {}  # cell -> (analyzer or None, sized rate req/s or None)

        def analyzer(k, i):
            if k in sized:
                return sized[k]
            server = self._srv_objs[i]
            acc_name = self.acc_names[self.cell_acc_idx[k]]
            perf = system.models[server.model_name].get_perf_data(acc_name)
            K = int(out_tok[i])
            N = server.max_batch_size if server.max_batch_size > 0 else max(
                perf.maxBatchSize * perf.atTokens // K, 1)
            cfg = Configuration(
                max_batch_size=N, max_queue_size=N * MAX_QUEUE_TO_BATCH_RATIO,
                service_parms=ServiceParms(
                    prefill=PrefillParms(gamma=perf.prefillParms.gamma,
                                         delta=perf.prefillParms.delta),
                    decode=DecodeParms(alpha=perf.decodeParms.alpha, beta=perf.decodeParms.beta)),
            )
            req = RequestSize(avg_input_tokens=int(in_tok[i]), avg_output_tokens=K)
            qa = rate_star = None
            try:
                if getattr(system, "analyzer_mode", "mm1k") == "mg1":
                    from ..analyzer.mg1 import MG1QueueEvaluator

                    qa = MG1QueueEvaluator(cfg, req, cv2=getattr(system, "analyzer_cv2", 1.0))
                else:
                    qa = QueueAnalyzer(cfg, req)
            except AnalyzerError:
                pass
            if qa is not None:
                t = targets[i]
                try:
                    _, metrics, _ = qa.size(TargetPerf(target_ttft=t.ttft, target_itl=t.itl,
                                                       target_tps=t.tps))
                    rate_star = metrics.throughput
                except AnalyzerError:
                    pass
            sized[k] = (qa, rate_star)
            return sized[k]

        for s in range(n_scen):
            for i in range(n_srv):
                k = cell_of.get((i, int(acc[s, i]))) if acc[s, i] >= 0 else None
                if k is None:
                    continue  # NOT_HELD
                at = (s, i)
                held = int(rep[s, i])
                rec["acc_idx"][at] = acc[s, i]
                rec["held_replicas"][at] = held
                rec["cost"][at] = f32(st["acc_cost"][k]) * f32(held)
                arr, K = float(scen[s, i]), int(out_tok[i])
                if arr == 0 or K == 0:
                    rec["status"][at] = HOLD_IDLE
                    rec["needed_replicas"][at] = 0
                    if st["min_replicas"][k] != 0:
                        rec["itl"][at] = f32(st["alpha"][k]) + f32(st["beta"][k])
                        rec["ttft"][at] = f32(st["gamma"][k]) + f32(st["delta"][k])
                    continue
                qa, rate_star = analyzer(k, i)
                if qa is None:
                    rec["status"][at] = HOLD_INVALID
                    continue
                tps = targets[i].tps
                total_rate = arr / 60.0 if tps == 0 else tps / float(K)
                if rate_star is not None:
                    with np.errstate(all="ignore"):
                        reps_d = np.ceil(np.float64(total_rate) / np.float64(rate_star))
                    reps_d = float(reps_d) if reps_d > 0.0 else 0.0
                    rec["needed_replicas"][at] = int(min(reps_d, 2147483000.0))
                    rec["slo_rate"][at] = f32(rate_star * float(held) * 60.0)
                metrics = None
                if held > 0 and total_rate / float(held) <= qa.rate_max:
                    try:
                        metrics = qa.analyze(total_rate / float(held))
                    except AnalyzerError:
                        pass
                if held > 0:
                    rec["rate"][at] = f32(total_rate / float(held))
                if metrics is None:
                    rec["status"][at] = HOLD_OVERLOADED
                    rec["itl"][at] = rec["ttft"][at] = np.inf
                    rec["rho"][at] = 1.0
                    continue
                rec["itl"][at] = metrics.avg_token_time
                rec["ttft"][at] = metrics.avg_wait_time + metrics.avg_prefill_time
                rec["rho"][at] = metrics.rho
                ok = rate_star is not None and held >= rec["needed_replicas"][at]
                rec["status"][at] = HOLD_OK if ok else HOLD_SLO_VIOLATED
        return rec

    # ------------------------------------------------------------------
    # What-if SLO planning
    # ------------------------------------------------------------------
    def plan_slo(self, slo_scales=None, targets=None, scales=None, arrival=None,
                 return_cells: bool = False) -> SloPlanResult:
        """Solve T SLO-target sets times S arrival-rate scenarios of the fleet
        in one pass: what a tighter or looser SLO costs, at each load.

        Target axis, exactly one of: ``slo_scales`` (T finite factors > 0;
        target set t is ``float32(base) * float32(scale)`` of every server's
        TTFT and ITL target) and ``targets=(ttft, itl)`` (two [T, n_servers]
        arrays in msec, taken as float32, finite and >= 0). A target of 0 is
        "no target"; a zero base target stays zero. The TPS target is the
        server's own in every set. Load axis: ``scales`` or ``arrival`` as in
        plan(); with neither, the base load alone (S = 1). 1 <= T * S <= 256.

        Slice (t, s) of the result is what reconcile() returns on a fresh
        FastSweep of an identical system whose per-server targets are
        ``t_ttft[t]`` / ``t_itl[t]`` and whose arrival rates are
        ``arrival[s]``. Servers that resolve to one Target object (same
        service class and model) cannot be given different targets.

        On the GPU each cell builds its chain geometry once, is sized once
        per target set and every sizing is evaluated at every load. Only a
        target set equal to the targets this FastSweep was built with uses the
        sizing memo (one lookup per loaded cell and call); the others are
        sized from scratch and leave the memo alone, so a following
        reconcile() is neither changed nor slowed. Unlimited mode only."""
        n_srv = len(self.server_names)
        srv_targets, owner = self._server_targets()
        if (slo_scales is None) == (targets is None):
            raise ValueError("plan_slo() takes exactly one of slo_scales and targets")
        if slo_scales is not None:
            try:
                sc = np.asarray(slo_scales, dtype=np.float64)
            except (TypeError, ValueError) as e:
                raise ValueError(f"slo_scales is not numeric: {e}") from None
            if sc.ndim != 1:
                raise ValueError(f"slo_scales must be 1-D, got shape {sc.shape}")
            if not np.isfinite(sc).all() or (sc <= 0).any():
                raise ValueError("slo_scales must be finite and positive")
            f32 = sc.astype(np.float32)
            if (f32 == 0).any():
                raise ValueError("slo_scales underflows float32")
            base_ttft = np.array([0.0 if t is None else t.ttft for t in srv_targets],
                                 dtype=np.float32)
            base_itl = np.array([0.0 if t is None else t.itl for t in srv_targets],
                                dtype=np.float32)
            with np.errstate(over="ignore"):
                t_ttft = base_ttft[None, :] * f32[:, None]
                t_itl = base_itl[None, :] * f32[:, None]
        else:
            try:
                ttft, itl = targets
                t_ttft = np.asarray(ttft, dtype=np.float64)
                t_itl = np.asarray(itl, dtype=np.float64)
            except (TypeError, ValueError) as e:
                raise ValueError(f"targets is not a (ttft, itl) pair of numeric arrays: {e}") \
                    from None
            for a, what in ((t_ttft, "ttft"), (t_itl, "itl")):
                if a.ndim != 2 or a.shape[1] != n_srv:
                    raise ValueError(f"targets {what} must have shape [T, {n_srv}], got {a.shape}")
                if not np.isfinite(a).all() or (a < 0).any():
                    raise ValueError(f"targets {what} must be finite and non-negative")
            if t_ttft.shape != t_itl.shape:
                raise ValueError("targets ttft and itl differ in shape")
            with np.errstate(over="ignore"):
                t_ttft, t_itl = t_ttft.astype(np.float32), t_itl.astype(np.float32)
        t_ttft = np.ascontiguousarray(t_ttft, dtype=np.float32)
        t_itl = np.ascontiguousarray(t_itl, dtype=np.float32)
        if not (np.isfinite(t_ttft).all() and np.isfinite(t_itl).all()):
            raise ValueError("SLO targets overflow float32")
        n_tgt = t_ttft.shape[0]
        if scales is None and arrival is None:
            scen = np.ascontiguousarray(self._base_load()[0][None, :], dtype=np.float32)
        else:
            scen = self._plan_scenarios(scales, arrival)
        n_load = scen.shape[0]
        if not 1 <= n_tgt * n_load <= PLAN_MAX_S:
            raise ValueError(
                f"plan_slo() takes 1..{PLAN_MAX_S} (target set, load) pairs, "
                f"got {n_tgt} x {n_load}"
            )
        # one Target object, one pair of targets per set, on both backends
        # (owner[i]: the first server that resolves to server i's Target)
        split = ((t_ttft != t_ttft[:, owner]) | (t_itl != t_itl[:, owner])).any(axis=0)
        if split.any():
            i = int(np.argmax(split))
            raise ValueError(
                f"servers {self.server_names[owner[i]]} and {self.server_names[i]} share one "
                "service-class target and cannot be given different targets"
            )

        n_acc = len(self.acc_names)
        cells = totals = None
        if self.backend != "gpu":
            rows = []
            with self._scenario_targets(srv_targets) as set_targets:
                for t in range(n_tgt):
                    set_targets(t_ttft[t], t_itl[t])
                    rows.append(self._plan_cpu(scen))
            flat = WinnerRecord(**{
                f: np.concatenate([getattr(r, f) for r in rows]) for f in _WINNER_FIELDS
            })
        elif self.n_cells == 0 or n_acc == 0:
            flat = _empty_winners(n_tgt * n_load, n_srv)
        else:
            self._tick(plan_arrival=scen, launch=False)  # stage + bucket layout
            cs = self.cell_server
            f32 = np.float32
            of, oi, totals = self._gpu.plan_slo(
                np.ascontiguousarray(scen[:, cs], dtype=f32),
                np.ascontiguousarray(t_ttft[:, cs], dtype=f32),
                np.ascontiguousarray(t_itl[:, cs], dtype=f32), n_acc,
            )
            flat = _winner_record(of, oi)
            if return_cells:
                cells = self._plan_cells_gpu(n_tgt * n_load)
                for k in CELL_KEYS:
                    cells[k] = cells[k].reshape(n_tgt, n_load, self.n_cells)
        totals, cost_total, infeasible = self._plan_totals(flat, totals)
        grid = (n_tgt, n_load)
        return SloPlanResult(
            winners=WinnerRecord(**{
                f: getattr(flat, f).reshape(grid + (n_srv,)) for f in _WINNER_FIELDS
            }),
            replicas_by_acc=totals.reshape(grid + (n_acc,)),
            cost_total=cost_total.reshape(grid),
            infeasible_servers=infeasible.reshape(grid),
            arrival=scen,
            t_ttft=t_ttft,
            t_itl=t_itl,
            cells=cells,
        )

    # ------------------------------------------------------------------
    # What-if token-mix planning
    # ------------------------------------------------------------------
    def plan_tokens(self, tokens=None, token_scales=None, scales=None, arrival=None,
                    return_cells: bool = False) -> TokenPlanResult:
        """Solve W sets of average token counts times S arrival-rate scenarios
        of the fleet in one pass: what a change of the request shape costs
        (longer prompts, longer or shorter outputs), at each load.

        Token axis, exactly one of: ``tokens=(in_tok, out_tok)`` (two
        [W, n_servers] integer arrays, every value >= 0 and within int32) and
        ``token_scales`` (W pairs ``(f_in, f_out)`` of finite factors > 0; set
        w is ``floor(float64(base) * f)`` of every server's average input and
        output tokens, where a positive base never drops below 1, so that a
        scale cannot switch a server's load off). Load axis: ``scales`` or
        ``arrival`` as in plan(); with neither, the base load alone (S = 1).
        1 <= W * S <= 256.

        Slice (w, s) of the result is what reconcile() returns on a fresh
        FastSweep of an identical system whose load is ``(arrival[s],
        in_tok[w], out_tok[w])``, with the same current allocation.

        On the GPU nothing of a cell is shared between two token sets: the
        batch size N moves with the output tokens, and with it the chain
        geometry and the block width. Every (set, cell) pair is a block of
        its own, in the bucket and at the width a reconcile under that set
        gives it, and every set is evaluated at every load. The pass brings
        its own bucket layout and stays off the sizing memo, so a following
        reconcile() is neither changed nor slowed and memo_stats() does not
        move. Unlimited mode only."""
        n_srv = len(self.server_names)
        if (tokens is None) == (token_scales is None):
            raise ValueError("plan_tokens() takes exactly one of tokens and token_scales")
        i32 = np.iinfo(np.int32)
        if token_scales is not None:
            try:
                sc = np.asarray(token_scales, dtype=np.float64)
            except (TypeError, ValueError) as e:
                raise ValueError(f"token_scales is not numeric: {e}") from None
            if sc.ndim != 2 or sc.shape[1] != 2:
                raise ValueError(
                    f"token_scales must be W pairs (f_in, f_out), got shape {sc.shape}")
            if not np.isfinite(sc).all() or (sc <= 0).any():
                raise ValueError("token_scales must be finite and positive")
            _, base_in, base_out = self._base_load()
            sets = []
            for base, f in ((base_in, sc[:, 0]), (base_out, sc[:, 1])):
                base = base.astype(np.float64)
                with np.errstate(over="ignore"):
                    v = np.floor(base[None, :] * f[:, None])
                sets.append(np.where(base[None, :] > 0, np.maximum(v, 1.0), v))
        else:
            try:
                t_in, t_out = tokens
                raw = [np.asarray(t_in), np.asarray(t_out)]
                sets = [a.astype(np.float64) for a in raw]
            except (TypeError, ValueError) as e:
                raise ValueError(
                    f"tokens is not an (in_tok, out_tok) pair of integer arrays: {e}") from None
            for a, r, what in zip(sets, raw, ("in_tok", "out_tok")):
                if a.ndim != 2 or a.shape[1] != n_srv:
                    raise ValueError(
                        f"tokens {what} must have shape [W, {n_srv}], got {a.shape}")
                if r.dtype.kind not in "iu" and not (
                        np.isfinite(a).all() and (a == np.floor(a)).all()):
                    raise ValueError(f"tokens {what} must hold integers")
            if sets[0].shape != sets[1].shape:
                raise ValueError("tokens in_tok and out_tok differ in shape")
        for a, what in zip(sets, ("in_tok", "out_tok")):
            if not np.isfinite(a).all() or (a < 0).any() or (a > i32.max).any():
                raise ValueError(f"{what} must be non-negative and fit int32")
        in_tok = np.ascontiguousarray(sets[0], dtype=np.int32)
        out_tok = np.ascontiguousarray(sets[1], dtype=np.int32)
        n_tok = in_tok.shape[0]
        if scales is None and arrival is None:
            scen = np.ascontiguousarray(self._base_load()[0][None, :], dtype=np.float32)
        else:
            scen = self._plan_scenarios(scales, arrival, who="plan_tokens()")
        n_load = scen.shape[0]
        if not 1 <= n_tok * n_load <= PLAN_MAX_S:
            raise ValueError(
                f"plan_tokens() takes 1..{PLAN_MAX_S} (token set, load) pairs, "
                f"got {n_tok} x {n_load}"
            )

        n_acc = len(self.acc_names)
        cells = totals = None
        if self.backend != "gpu":
            rows = []
            with self._scenario_tokens() as set_tokens:
                for w in range(n_tok):
                    set_tokens(in_tok[w], out_tok[w])
                    rows.append(self._plan_cpu(scen))
            flat = WinnerRecord(**{
                f: np.concatenate([getattr(r, f) for r in rows]) for f in _WINNER_FIELDS
            })
        elif self.n_cells == 0 or n_acc == 0:
            flat = _empty_winners(n_tok * n_load, n_srv)
        else:
            self._tick(plan_arrival=scen, launch=False)  # stage the rest of the cell state
            cs = self.cell_server
            of, oi, totals = self._gpu.plan_tokens(
                np.ascontiguousarray(scen[:, cs], dtype=np.float32),
                np.ascontiguousarray(in_tok[:, cs]), np.ascontiguousarray(out_tok[:, cs]),
                self._token_batch_n(scen, out_tok), n_acc,
            )
            flat = _winner_record(of, oi)
            if return_cells:
                cells = self._plan_cells_gpu(n_tok * n_load)
                for k in CELL_KEYS:
                    cells[k] = cells[k].reshape(n_tok, n_load, self.n_cells)
        totals, cost_total, infeasible = self._plan_totals(flat, totals)
        grid = (n_tok, n_load)
        return TokenPlanResult(
            winners=WinnerRecord(**{
                f: getattr(flat, f).reshape(grid + (n_srv,)) for f in _WINNER_FIELDS
            }),
            replicas_by_acc=totals.reshape(grid + (n_acc,)),
            cost_total=cost_total.reshape(grid),
            infeasible_servers=infeasible.reshape(grid),
            arrival=scen,
            in_tok=in_tok,
            out_tok=out_tok,
            cells=cells,
        )

    def _token_batch_n(self, scen: np.ndarray, out_tok: np.ndarray) -> np.ndarray:
        """int32 [W, n_cells]: the batch size N of every cell under every token
        set, by _refresh_dynamic's rule with the plan's zero-load decision: 1
        where no scenario loads the cell or the set's out_tok is 0, else the
        server's override or max(maxBatchSize * atTokens // out_tok, 1)."""
        cs = self.cell_server
        st = self._stat
        c_out = out_tok[:, cs]
        prod = st["perf_max_batch_cfg"].astype(np.int64) * st["at_tokens"].astype(np.int64)
        n_scaled = np.maximum(prod[None, :] // np.maximum(c_out, 1).astype(np.int64), 1)
        base = np.where(st["override"][None, :] > 0, st["override"][None, :],
                        n_scaled).astype(np.int32)
        zero_load = (scen.max(axis=0)[cs] == 0)[None, :] | (c_out == 0)
        return np.ascontiguousarray(np.where(zero_load, 1, base), dtype=np.int32)

    @contextlib.contextmanager
    def _scenario_tokens(self):
        """For the CPU golden path: yields set_tokens(in_row, out_row), which
        puts one token set on the server objects (and into the load override,
        when set, which _scenario_loads copies the tokens from); both are
        restored afterwards in any case."""
        saved_override = self.load_override
        saved = [
            None if srv.load is None else (srv.load.avgInTokens, srv.load.avgOutTokens)
            for srv in self._srv_objs
        ]

        def set_tokens(in_row, out_row):
            for i, srv in enumerate(self._srv_objs):
                if srv.load is not None:
                    srv.load.avgInTokens = int(in_row[i])
                    srv.load.avgOutTokens = int(out_row[i])
            if saved_override is not None:
                self.load_override = (saved_override[0], np.array(in_row, dtype=np.int32),
                                      np.array(out_row, dtype=np.int32))

        try:
            yield set_tokens
        finally:
            self.load_override = saved_override
            for srv, old in zip(self._srv_objs, saved):
                if old is not None:
                    srv.load.avgInTokens, srv.load.avgOutTokens = old

    def _server_targets(self):
        """(targets, owner), cached per fleet topology: the Target object each
        server resolves to (None: no service class or no target for its
        model), as create_allocation resolves it, and per server the index of
        the first server that resolves to the same object (its own index for a
        server without one)."""
        cached = getattr(self, "_server_targets_cache", None)
        if cached is not None:
            return cached
        out, first = [], {}
        owner = np.arange(len(self._srv_objs), dtype=np.int64)
        for i, server in enumerate(self._srv_objs):
            svc = self.system.service_classes.get(server.service_class_name)
            tgt = svc.model_target(server.model_name) if svc is not None else None
            out.append(tgt)
            if tgt is not None:
                owner[i] = first.setdefault(id(tgt), i)
        self._server_targets_cache = (out, owner)
        return self._server_targets_cache

    @contextlib.contextmanager
    def _scenario_targets(self, srv_targets):
        """For the CPU golden path: yields set_targets(ttft_row, itl_row), which
        puts one target set on the servers' Target objects; their targets are
        restored afterwards in any case."""
        saved = {id(t): (t, t.ttft, t.itl) for t in srv_targets if t is not None}

        def set_targets(ttft_row, itl_row):
            for i, t in enumerate(srv_targets):
                if t is not None:
                    t.ttft, t.itl = float(ttft_row[i]), float(itl_row[i])

        try:
            yield set_targets
        finally:
            for t, ttft, itl in saved.values():
                t.ttft, t.itl = ttft, itl

    # ------------------------------------------------------------------
    # Capacity-limited planning
    # ------------------------------------------------------------------
    def _plan_capacity(self, capacity, n_scen: int) -> np.ndarray:
        """Validate plan()'s capacity and return it as int32 [S, n_types]."""
        types = self.capacity_types
        n_types = len(types)
        if hasattr(capacity, "keys"):
            unknown = sorted(set(capacity) - set(types))
            if unknown:
                raise ValueError(f"capacity names unknown accelerator types: {unknown}")
            try:
                row = np.array([capacity.get(t, 0) for t in types], dtype=np.float64)
            except (TypeError, ValueError) as e:
                raise ValueError(f"capacity is not numeric: {e}") from None
            vals = np.repeat(row[None, :], n_scen, axis=0)
        else:
            try:
                vals = np.asarray(capacity, dtype=np.float64)
            except (TypeError, ValueError) as e:
                raise ValueError(f"capacity is not numeric: {e}") from None
            if vals.shape != (n_scen, n_types):
                raise ValueError(
                    f"capacity must be a mapping or have shape [{n_scen}, {n_types}] "
                    f"(columns {types}), got {vals.shape}"
                )
        if not np.isfinite(vals).all():
            raise ValueError("capacity must be finite")
        if (vals < 0).any() or (vals != np.floor(vals)).any():
            raise ValueError("capacity must hold non-negative integers")
        if (vals > np.iinfo(np.int32).max).any():
            raise ValueError("capacity must fit int32")
        return np.ascontiguousarray(vals, dtype=np.int32)

    def _plan_limited(self, scen, capacity, saturation_policy, delayed, return_cells):
        n_scen, n_srv = scen.shape
        cap = self._plan_capacity(capacity, n_scen)
        policy = _POLICY_CODE[SaturationPolicy.parse(saturation_policy).value]
        delayed = bool(delayed)
        cells = None
        if self.n_cells == 0 or not self.acc_names:
            zeros = np.zeros((n_scen, n_srv), dtype=np.int32)
            sol = (_empty_winners(n_scen, n_srv), None, zeros, zeros.copy(), cap.astype(np.int64))
        elif self.backend == "gpu":
            mode = os.environ.get("INFERNO_PLAN_GREEDY", "") or PLAN_GREEDY_DEFAULT
            if mode not in ("host", "device"):
                raise ValueError(f"INFERNO_PLAN_GREEDY must be host or device, got {mode!r}")
            if (policy in (2, 3) and cap.size
                    and int(cap.astype(np.int64).sum(axis=1).max()) > PLAN_GREEDY_RR_MAX_UNITS):
                mode = "host"
            if mode == "device":
                sol = self._plan_limited_device(scen, cap, policy, delayed)
                if return_cells:
                    cells = self._plan_cells_gpu(n_scen)
            else:
                sol, cells = self._plan_limited_host(scen, cap, policy, delayed)
                if not return_cells:
                    cells = None
        else:
            sol = self._plan_limited_cpu(scen, cap, saturation_policy, delayed)
        winners, totals, desired, n_cand, cap_left = sol
        has = winners.acc_idx != -1
        granted = winners.num_replicas
        return self._plan_result(
            scen, winners, totals, cells,
            desired_replicas=desired,
            unallocated_servers=((n_cand > 0) & ~has).sum(axis=1).astype(np.int64),
            partial_servers=((granted > 0) & (granted < desired)).sum(axis=1).astype(np.int64),
            capacity_left=cap_left.astype(np.int64),
            capacity_types=self.capacity_types,
        )

    def _plan_limited_device(self, scen, cap, policy: int, delayed: bool):
        self._tick(plan_arrival=scen, launch=False)  # stage + bucket layout
        g = self._gpu
        g.sync_greedy_static(*self.greedy_static()[1:])
        cell_scen = np.ascontiguousarray(scen[:, self.cell_server], dtype=np.float32)
        of, oi, totals, ox, cap_left = g.plan(cell_scen, len(self.acc_names),
                                              (cap, delayed, policy))
        self._plan_limited_cells = oi[:, 3].copy()  # winning cell index; tests read it
        return _winner_record(of, oi), totals, ox[:, 0].copy(), ox[:, 1].copy(), cap_left

    def _plan_limited_host(self, scen, cap, policy: int, delayed: bool):
        """The host loop: one native greedy (ops/native/greedy.cpp) per
        scenario over the downloaded per-cell outputs."""
        n_scen, n_srv = scen.shape
        _, _, cells = self._plan_gpu(scen, True)
        _, cell_tidx, units, prio = self.greedy_static()
        prio = np.ascontiguousarray(prio, dtype=np.int32)
        win_cells = np.full((n_scen, n_srv), -1, dtype=np.int32)
        granted = np.zeros((n_scen, n_srv), dtype=np.int32)
        cap_left = cap.copy()
        for s in range(n_scen):
            order, seg, c_val, c_type, c_units, c_reps = greedy_candidates(
                cells["feasible"][s], cells["zero_empty"][s], cells["value"][s],
                cells["num_replicas"][s], self.cell_server, cell_tidx, units, n_srv,
            )
            win_cand, win_reps = run_greedy_native(
                c_val, c_type, c_units, c_reps, seg, prio, cap_left[s], delayed, policy,
                allow_build=False,
            )
            got = win_cand >= 0
            win_cells[s, got] = order[win_cand[got]]
            granted[s, got] = win_reps[got]
        # winner records of all scenarios at once
        has = win_cells >= 0
        at = np.where(has, win_cells, 0)

        def pick(key, empty):
            return np.where(has, np.take_along_axis(cells[key], at, axis=1), empty)

        desired = pick("num_replicas", 0).astype(np.int32)
        cut = has & (desired > 0) & (granted != desired)
        factor = np.ones((n_scen, n_srv), dtype=np.float64)
        factor[cut] = granted[cut].astype(np.float64) / desired[cut].astype(np.float64)
        rec = {}
        for f in ("cost", "value"):
            whole = pick(f, np.float32(0.0)).astype(np.float32)
            scaled = (whole.astype(np.float64) * factor).astype(np.float32)
            rec[f] = np.where(cut, scaled, whole)
        for f in ("itl", "ttft", "rho", "max_rate"):
            rec[f] = pick(f, np.float32(0.0)).astype(np.float32)
        winners = WinnerRecord(
            acc_idx=np.where(has, self.cell_acc_idx[at], -1).astype(np.int32),
            num_replicas=granted, batch=pick("batch", 0).astype(np.int32), **rec,
        )
        real = cells["feasible"].astype(bool) & ~cells["zero_empty"].astype(bool)
        run = np.concatenate(
            [np.zeros((n_scen, 1), dtype=np.int32), np.cumsum(real, axis=1, dtype=np.int32)],
            axis=1)
        n_cand = run[:, self.seg_start[1:]] - run[:, self.seg_start[:-1]]
        self._plan_limited_cells = win_cells
        return (winners, None, desired, n_cand, cap_left.astype(np.int64)), cells

    @contextlib.contextmanager
    def _scenario_loads(self):
        """For the CPU golden paths: yields set_loads(row), which puts one
        scenario's arrival rates (and the load override's token averages, when
        set) on the server objects; their loads are restored afterwards in any
        case."""
        _, in_tok, out_tok = self._base_load()
        saved = [
            None if srv.load is None
            else (srv.load.arrivalRate, srv.load.avgInTokens, srv.load.avgOutTokens)
            for srv in self._srv_objs
        ]

        def set_loads(row):
            for i, srv in enumerate(self._srv_objs):
                if srv.load is None:
                    continue  # no load: zero-traffic whatever the scenario says
                srv.load.arrivalRate = float(row[i])
                if self.load_override is not None:
                    srv.load.avgInTokens = int(in_tok[i])
                    srv.load.avgOutTokens = int(out_tok[i])

        try:
            yield set_loads
        finally:
            for srv, old in zip(self._srv_objs, saved):
                if old is not None:
                    (srv.load.arrivalRate, srv.load.avgInTokens,
                     srv.load.avgOutTokens) = old

    def _plan_limited_cpu(self, scen, cap, saturation_policy, delayed: bool):
        """Golden path: per scenario the CPU sweep with the scenario's loads,
        then solver.greedy.solve_greedy with the scenario's capacity. Loads,
        allocations, candidate lists and system.capacity are restored
        afterwards in any case."""
        from ..solver.greedy import solve_greedy
        from .engine import SweepEngine

        system = self.system
        n_scen, n_srv = scen.shape
        types = self.capacity_types
        policy = SaturationPolicy.parse(saturation_policy)
        members = set(self.server_names)
        saved_alloc = {
            name: (srv.allocation, srv.all_allocations, srv.spec.desiredAlloc)
            for name, srv in system.servers.items()
        }
        saved_capacity = system.capacity
        winners = _empty_winners(n_scen, n_srv)
        desired = np.zeros((n_scen, n_srv), dtype=np.int32)
        n_cand = np.zeros((n_scen, n_srv), dtype=np.int32)
        cap_left = cap.astype(np.int64)
        engine = SweepEngine(backend="cpu")
        try:
            with self._scenario_loads() as set_loads:
                for s in range(n_scen):
                    set_loads(scen[s])
                    for name, srv in system.servers.items():
                        if name not in members:
                            srv.all_allocations = {}  # only this sweep's servers compete
                    engine.sweep(system, server_names=self.server_names)
                    want = {}
                    for i, srv in enumerate(self._srv_objs):
                        for alloc in srv.all_allocations.values():
                            want[id(alloc)] = alloc.num_replicas
                            if alloc.accelerator != "":
                                n_cand[s, i] += 1
                    system.capacity = {t: int(cap[s, j]) for j, t in enumerate(types)}
                    solve_greedy(system, delayed_best_effort=delayed, saturation_policy=policy)
                    for i, srv in enumerate(self._srv_objs):
                        alloc = srv.allocation
                        if alloc is None or alloc.accelerator == "":
                            continue
                        acc = system.accelerators[alloc.accelerator]
                        model = system.models[srv.model_name]
                        per = model.get_num_instances(acc.name) * acc.multiplicity
                        cap_left[s, types.index(acc.type)] -= alloc.num_replicas * per
                        desired[s, i] = want.get(id(alloc), alloc.num_replicas)
                        _set_winner(winners, (s, i), alloc, self._acc_index[alloc.accelerator])
        finally:
            for name, (alloc, all_allocs, want_alloc) in saved_alloc.items():
                system.servers[name].allocation = alloc
                system.servers[name].all_allocations = all_allocs
                system.servers[name].spec.desiredAlloc = want_alloc
            system.capacity = saved_capacity
        return winners, None, desired, n_cand, cap_left

    def _plan_cpu(self, scen: np.ndarray) -> WinnerRecord:
        """Golden path: one _reconcile_cpu per scenario with the scenario's
        arrival rate (and the load override's token averages, when set) put
        on the server objects, which are restored afterwards in any case."""
        rows = []
        with self._scenario_loads() as set_loads:
            for row in scen:
                set_loads(row)
                rows.append(self._reconcile_cpu())
        return WinnerRecord(**{
            f: np.stack([getattr(r, f) for r in rows]) for f in _WINNER_FIELDS
        })

    def _reconcile_cpu(self) -> WinnerRecord:
        """Golden scalar path returning the same winner records."""
        n_srv = len(self.server_names)
        rec = _empty_winner(n_srv)
        for seg, name in enumerate(self.server_names):
            server = self.system.servers[name]
            best = None
            for acc_name in sorted(server.candidate_accelerators(self.system)):
                alloc = create_allocation(self.system, name, acc_name)
                if alloc is None:
                    continue
                if server.cur_allocation is not None:
                    alloc.value = server.cur_allocation.transition_penalty(alloc)
                if best is None or alloc.value < best.value:
                    best = alloc
            if best is None:
                continue
            _set_winner(rec, seg, best,
                        -2 if best.accelerator == "" else self._acc_index[best.accelerator])
        return rec


def feed_back(cur, w: WinnerRecord):
    """Desired -> current between two ticks: the (cur_acc, cur_rep, cur_cost)
    triple after a tick that started from ``cur`` and returned the winners
    ``w`` ([n_servers]). A server without a feasible cell (acc_idx -1) keeps
    what it had; a zero-load empty winner (-2) leaves it empty (-1)."""
    pa, pr, pc = cur
    ok = w.acc_idx != -1
    return (
        np.where(ok, np.where(w.acc_idx == -2, -1, w.acc_idx), pa).astype(np.int32),
        np.where(ok, w.num_replicas, pr).astype(np.int32),
        np.where(ok, w.cost, pc).astype(np.float32),
    )


def _acc_changes(start_acc: np.ndarray, acc_idx: np.ndarray) -> np.ndarray:
    """Per step of a rollout, the servers whose current accelerator (-3 none,
    -1 empty, >= 0 index) after the step differs from the one before it;
    ``acc_idx`` is the winners' [S, n_servers], ``start_acc`` the current
    accelerator before step 0."""
    n_steps = acc_idx.shape[0]
    ok = acc_idx != -1
    # the step each server's current accelerator was last set at (-1: never)
    last = np.maximum.accumulate(
        np.where(ok, np.arange(n_steps)[:, None], -1), axis=0)
    new = np.where(acc_idx == -2, -1, acc_idx)
    after = np.where(last >= 0, np.take_along_axis(new, np.maximum(last, 0), axis=0),
                     start_acc[None, :])
    before = np.concatenate([start_acc[None, :], after[:-1]])
    return (after != before).sum(axis=1).astype(np.int64)


def _ensemble_quantiles(quantiles, n_paths: int):
    """Validate rollout_ensemble()'s quantiles: (float64 [Q], int64 ranks)."""
    try:
        qs = np.atleast_1d(np.asarray(quantiles, dtype=np.float64))
    except (TypeError, ValueError) as e:
        raise ValueError(f"quantiles is not numeric: {e}") from None
    if qs.ndim != 1 or not 1 <= qs.shape[0] <= ENSEMBLE_MAX_QUANTILES:
        raise ValueError(
            f"rollout_ensemble() takes 1..{ENSEMBLE_MAX_QUANTILES} quantiles, got shape {qs.shape}")
    if not (np.isfinite(qs).all() and (qs > 0).all() and (qs <= 1).all()):
        raise ValueError("quantiles must lie in (0, 1]")
    return qs, ensemble_ranks(qs, n_paths)


def _ensemble_arena_bytes(n_paths: int, n_steps: int, n_srv: int, n_acc: int, n_q: int) -> int:
    """Bytes of the device arena of an ensemble, as ops/hip/wva_ctx.inc lays it
    out (every segment padded to 256 bytes): the three compact records, the
    per-row aggregates, the final allocations, the bands."""
    rows = n_paths * n_steps
    sizes = [rows * n_srv * 4] * 3 + [rows * n_acc * 8, rows * 4, rows * 4, rows * 8,
                                      n_paths * 3 * n_srv * 4]
    sizes += [n_q * n_steps * n_srv * 4] * 2 + [n_steps * n_srv * 4] * 2
    sizes.append(n_q * n_steps * (n_acc + 3) * 8)
    return sum((b + 255) // 256 * 256 for b in sizes)


def _ensemble_bands_of(winners: WinnerRecord, totals: np.ndarray, start_acc: np.ndarray,
                       ranks: np.ndarray) -> dict:
    """The per-path aggregates, bands and mode pair of an EnsembleResult from
    the paths' winners ([E, S, n_servers] arrays) and replica totals ([E, S,
    n_acc]), all by the module's helpers: the definition the device is checked
    against."""
    acc = winners.acc_idx
    infeasible = (acc == -1).sum(axis=2).astype(np.int64)
    changes = np.stack([_acc_changes(start_acc, a) for a in acc])
    cost = ensemble_path_cost(winners.cost)
    mode, mode_paths = ensemble_mode(acc)
    return dict(
        path_replicas_by_acc=totals, path_infeasible_servers=infeasible,
        path_acc_changes=changes, path_cost_total=cost,
        replicas_by_acc_q=ensemble_bands(totals, ranks),
        cost_total_q=ensemble_bands(cost, ranks),
        infeasible_q=ensemble_bands(infeasible, ranks),
        acc_changes_q=ensemble_bands(changes, ranks),
        server_replicas_q=ensemble_bands(winners.num_replicas, ranks),
        server_cost_q=ensemble_bands(winners.cost, ranks),
        acc_mode=mode, acc_mode_paths=mode_paths)


def _empty_hold(n_scen: int, n_srv: int) -> dict:
    """The per-server arrays of a HoldResult with every slice NOT_HELD."""
    shape = (n_scen, n_srv)
    rec = {k: np.zeros(shape, dtype=np.float32) for k in _HOLD_FLOATS}
    rec["status"] = np.full(shape, HOLD_NOT_HELD, dtype=np.int32)
    rec["acc_idx"] = np.full(shape, -1, dtype=np.int32)
    rec["held_replicas"] = np.zeros(shape, dtype=np.int32)
    rec["needed_replicas"] = np.full(shape, -1, dtype=np.int32)
    return rec


def _hold_sums(rec: dict, n_acc: int):
    """(counts int64 [S, 6], deficit_by_acc int64 [S, n_acc]) of the per-server
    arrays of a hold analysis."""
    n_scen = rec["status"].shape[0]
    counts = np.stack([np.bincount(rec["status"][s], minlength=len(HOLD_STATUS_NAMES))
                       for s in range(n_scen)]).astype(np.int64)
    deficit = np.zeros((n_scen, n_acc), dtype=np.int64)
    need = rec["needed_replicas"].astype(np.int64)
    short = np.maximum(need - rec["held_replicas"].astype(np.int64), 0)
    on = (rec["status"] != HOLD_NOT_HELD) & (need >= 0) & (rec["acc_idx"] >= 0)
    for s in range(n_scen):
        np.add.at(deficit[s], rec["acc_idx"][s][on[s]], short[s][on[s]])
    return counts, deficit


def _empty_winner(n: int) -> WinnerRecord:
    return WinnerRecord(
        acc_idx=np.full(n, -1, dtype=np.int32),
        num_replicas=np.zeros(n, dtype=np.int32),
        batch=np.zeros(n, dtype=np.int32),
        cost=np.zeros(n, dtype=np.float32),
        value=np.zeros(n, dtype=np.float32),
        itl=np.zeros(n, dtype=np.float32),
        ttft=np.zeros(n, dtype=np.float32),
        rho=np.zeros(n, dtype=np.float32),
        max_rate=np.zeros(n, dtype=np.float32),
    )


def _set_winner(rec: WinnerRecord, at, alloc, acc_idx: int) -> None:
    """Put Allocation ``alloc`` into ``rec`` at index ``at`` (the CPU paths)."""
    rec.acc_idx[at] = acc_idx
    rec.num_replicas[at] = alloc.num_replicas
    rec.batch[at] = alloc.batch_size
    rec.cost[at] = alloc.cost
    rec.value[at] = alloc.value
    rec.itl[at] = alloc.itl
    rec.ttft[at] = alloc.ttft
    rec.rho[at] = alloc.rho
    rec.max_rate[at] = alloc.max_arrv_rate_per_replica


def _empty_winners(n_scen: int, n_srv: int) -> WinnerRecord:
    """_empty_winner for every scenario of a plan: arrays [n_scen, n_srv]."""
    w = _empty_winner(n_srv)
    return WinnerRecord(**{
        f: np.repeat(getattr(w, f)[None, :], n_scen, axis=0) for f in _WINNER_FIELDS
    })


def _winner_record(of: np.ndarray, oi: np.ndarray) -> WinnerRecord:
    """The native winner blocks as a WinnerRecord: ``of`` holds the fp32 rows
    (cost, value, itl, ttft, rho, max_rate), ``oi`` the int32 rows (acc code,
    replicas, batch, winner cell). Either the [rows, n_srv] pair of a
    reconcile, whose rows become the fields as they are (views, no copy), or
    the [S, rows, n_srv] pair of a plan, which is first copied rows-major so
    that every field is a contiguous [S, n_srv] array."""
    if of.ndim == 3:
        of = np.ascontiguousarray(of.transpose(1, 0, 2))
        oi = np.ascontiguousarray(oi.transpose(1, 0, 2))
    return WinnerRecord(
        acc_idx=oi[0], num_replicas=oi[1], batch=oi[2],
        cost=of[0], value=of[1], itl=of[2], ttft=of[3], rho=of[4], max_rate=of[5],
    )
