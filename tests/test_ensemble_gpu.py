"""Forecast ensembles on the GPU (FastSweep.rollout_ensemble): every path must be
bit for bit what rollout() computes for it on a second context, and every band
what the CPU helpers (np.sort at the ranks, the cumsum cost, the bincount mode)
give over the downloaded paths.

Every comparison is raw bits. The fleets are those of tests/test_rollout_gpu.py,
built the same way: small, every cell's batch size pinned <= 64 through the
per-cell override row.
"""
import dataclasses

import numpy as np
import pytest

from inferno_amd.core import System
from inferno_amd.engine import (
    FastSweep,
    ensemble_bands,
    ensemble_mode,
    ensemble_path_cost,
    ensemble_ranks,
    fastpath,
)
from tests.fixtures import make_spec

pytestmark = pytest.mark.gpu

CELL_N = (1, 5, 16, 33, 64, 48, 7, 2)
ARRIVAL_SCALE = 6000.0  # req/min: enough load that replica counts move per step
# rises, falls, a zero row, comes back. On the zero row the server with the
# unreachable SLO keeps its load: at zero load its cells would take the zero
# path, which is feasible whatever the SLO.
SCALES = (1.0, 2.3, 3.1, 0.6, 0.0, 0.37, 1.7)
ZERO_STEP = 4
INFEASIBLE_SRV, SCALE_TO_ZERO_SRV, TPS_SRV, NO_CUR_SRV, UNKNOWN_CUR_SRV = 6, 4, 2, 1, 5
IDLE_SRV = 3  # an ordinary server: one path of case 1 never loads it
QUANTILES = (0.2, 0.5, 0.9, 1.0)
WINNER_FLOAT = ("cost", "value", "itl", "ttft", "rho", "max_rate")
RESULT_FIELDS = (
    "quantiles", "ranks", "arrival", "path_replicas_by_acc", "path_infeasible_servers",
    "path_acc_changes", "path_cost_total", "replicas_by_acc_q", "cost_total_q", "infeasible_q",
    "acc_changes_q", "server_replicas_q", "server_cost_q", "acc_mode", "acc_mode_paths")


def pin_batches(fs):
    fs._stat["override"][:] = np.resize(np.asarray(CELL_N, dtype=np.int32), fs.n_cells)


def loads_of(system, fs):
    names = fs.server_names
    arrival = np.array([system.servers[n].load.arrivalRate for n in names], dtype=np.float32)
    in_tok = np.array([system.servers[n].load.avgInTokens for n in names], dtype=np.int32)
    out_tok = np.array([system.servers[n].load.avgOutTokens for n in names], dtype=np.int32)
    assert (arrival > 0).all() and (out_tok > 0).all()
    return arrival, in_tok, out_tok


def oracle_system(analyzer_mode=None):
    """8 servers x 3 accelerators with one server each of: unreachable SLO,
    min_replicas 0, a TPS target."""
    system, _ = System.from_spec(make_spec(n_servers=8, seed=901, arrival_scale=ARRIVAL_SCALE))
    names = sorted(system.servers)

    def target(i):
        srv = system.servers[names[i]]
        return system.service_classes[srv.service_class_name].targets[srv.model_name]

    target(INFEASIBLE_SRV).itl = 1e-3
    target(INFEASIBLE_SRV).ttft = 0.0
    target(TPS_SRV).tps = 2000.0
    system.servers[names[SCALE_TO_ZERO_SRV]].min_num_replicas = 0
    if analyzer_mode is not None:
        system.analyzer_mode = analyzer_mode
    return system


def oracle_cur(fs):
    """The spec's current allocations, with one server that has none and one
    whose accelerator the fleet does not know."""
    cur_acc, cur_rep, cur_cost = (np.array(a) for a in fs._base_cur())
    cur_acc[NO_CUR_SRV], cur_rep[NO_CUR_SRV], cur_cost[NO_CUR_SRV] = -3, 0, 0.0
    cur_acc[UNKNOWN_CUR_SRV], cur_rep[UNKNOWN_CUR_SRV], cur_cost[UNKNOWN_CUR_SRV] = -1, 3, 123.25
    return cur_acc, cur_rep, cur_cost


def oracle_rows(base):
    scen = np.stack([base * np.float32(sc) for sc in SCALES]).astype(np.float32)
    scen[ZERO_STEP, INFEASIBLE_SRV] = base[INFEASIBLE_SRV]
    return scen


def make_pair(build, cur_of=None):
    """The same fleet twice: the one that runs ensembles and the twin whose
    rollout() calls are the reference."""
    out = []
    for _ in range(2):
        system = build()
        fs = FastSweep(system, backend="gpu")
        pin_batches(fs)
        fs.load_override = loads_of(system, fs)
        fs.cur_override = cur_of(fs) if cur_of is not None else tuple(
            np.array(a) for a in fs._base_cur())
        out.append(fs)
    return out


def case1_paths(base):
    rows = oracle_rows(base)
    idle = rows.copy()
    idle[:, IDLE_SRV] = 0.0
    return np.stack([rows, rows[::-1], rows * np.float32(1.6), rows, idle]).astype(np.float32)


def same_bytes(a, b, what):
    assert a.dtype == b.dtype, f"{what}: dtype {a.dtype} != {b.dtype}"
    assert a.shape == b.shape, f"{what}: shape {a.shape} != {b.shape}"
    assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), (
        f"{what} differs")


def assert_path_equals_rollout(res, e, ref):
    what = f"path {e}"
    for f in dataclasses.fields(ref.winners):
        same_bytes(getattr(res.paths.winners, f.name)[e], getattr(ref.winners, f.name),
                   f"{what}: winner {f.name}")
    for k in range(3):
        same_bytes(res.paths.final_cur[k][e], ref.final_cur[k], f"{what}: final_cur[{k}]")
    same_bytes(res.path_replicas_by_acc[e], ref.replicas_by_acc, f"{what}: replicas_by_acc")
    same_bytes(res.path_infeasible_servers[e], ref.infeasible_servers, f"{what}: infeasible")
    same_bytes(res.path_acc_changes[e], ref.acc_changes, f"{what}: acc_changes")


def assert_bands_equal_helpers(res):
    """Every band and the mode pair against the CPU helpers over the
    downloaded paths; the per-path cost against its definition."""
    w = res.paths.winners
    n_paths = w.acc_idx.shape[0]
    same_bytes(res.ranks, ensemble_ranks(res.quantiles, n_paths), "ranks")
    cost = np.cumsum(w.cost.astype(np.float64), axis=2)[:, :, -1]
    same_bytes(res.path_cost_total, cost, "path_cost_total")
    same_bytes(res.path_cost_total, ensemble_path_cost(w.cost), "path_cost_total (helper)")
    same_bytes(res.path_infeasible_servers, (w.acc_idx == -1).sum(axis=2).astype(np.int64),
               "path_infeasible_servers")
    rk = res.ranks
    same_bytes(res.replicas_by_acc_q, ensemble_bands(res.path_replicas_by_acc, rk), "replicas q")
    same_bytes(res.cost_total_q, ensemble_bands(cost, rk), "cost q")
    same_bytes(res.infeasible_q, ensemble_bands(res.path_infeasible_servers, rk), "infeasible q")
    same_bytes(res.acc_changes_q, ensemble_bands(res.path_acc_changes, rk), "changes q")
    same_bytes(res.server_replicas_q, np.sort(w.num_replicas, axis=0)[rk], "server replicas q")
    same_bytes(res.server_cost_q, np.sort(w.cost, axis=0)[rk], "server cost q")
    mode, count = ensemble_mode(w.acc_idx)
    same_bytes(res.acc_mode, mode, "acc_mode")
    same_bytes(res.acc_mode_paths, count, "acc_mode_paths")


def assert_results_identical(a, b, with_paths=True):
    for f in RESULT_FIELDS:
        same_bytes(getattr(a, f), getattr(b, f), f)
    if not with_paths:
        return
    for f in dataclasses.fields(a.paths.winners):
        same_bytes(getattr(a.paths.winners, f.name), getattr(b.paths.winners, f.name), f.name)
    for x, y in zip(a.paths.final_cur, b.paths.final_cur):
        same_bytes(x, y, "final_cur")


_CASE1 = {}


def case1(analyzer_mode=None):
    """(result with paths, its FastSweep, the twin's rollout per path)."""
    if analyzer_mode not in _CASE1:
        fs, twin = make_pair(lambda: oracle_system(analyzer_mode), oracle_cur)
        assert fs.n_cells == 24
        arrival = case1_paths(fs.load_override[0])
        res = fs.rollout_ensemble(arrival=arrival, quantiles=QUANTILES, return_paths=True)
        refs = [twin.rollout(arrival=arrival[e]) for e in range(arrival.shape[0])]
        _CASE1[analyzer_mode] = (res, fs, refs)
    return _CASE1[analyzer_mode]


# -- case 1: E = 5, S = 7 ----------------------------------------------------------
def test_paths_and_bands(monkeypatch):
    monkeypatch.delenv("INFERNO_SIZING_MEMO", raising=False)
    res, fs, refs = case1()
    arrival = case1_paths(fs.load_override[0])
    same_bytes(res.arrival, arrival, "arrival")
    assert res.ranks.tolist() == [0, 2, 4, 4]
    for e, ref in enumerate(refs):
        assert_path_equals_rollout(res, e, ref)
    assert_bands_equal_helpers(res)
    # the idle path stages its server's cells as loaded (the other paths of the
    # pass load them) and still is its stand-alone rollout: checked above; here,
    # that the server really is idle there and sized for its load elsewhere
    assert (res.arrival[4, :, IDLE_SRV] == 0).all() and (res.arrival[0, :3, IDLE_SRV] > 0).all()
    reps = res.paths.winners.num_replicas
    assert (reps[4, :, IDLE_SRV] == reps[4, 0, IDLE_SRV]).all()
    assert (reps[0, :3, IDLE_SRV] > reps[4, :3, IDLE_SRV]).any()
    # the inputs do not degenerate: the paths disagree somewhere, and a band
    # moves with the quantile
    assert (res.acc_mode_paths < 5).any()
    assert (res.server_replicas_q[0] != res.server_replicas_q[3]).any()
    assert (res.cost_total_q[0] != res.cost_total_q[3]).any()
    # paths 0 and 3 are equal keys at every rank
    for f in dataclasses.fields(res.paths.winners):
        same_bytes(getattr(res.paths.winners, f.name)[0], getattr(res.paths.winners, f.name)[3],
                   f.name)


# -- case 2: bands only ------------------------------------------------------------
def test_bands_only_returns_the_same_bytes(monkeypatch):
    monkeypatch.delenv("INFERNO_SIZING_MEMO", raising=False)
    full, fs, _ = case1()
    res = fs.rollout_ensemble(arrival=full.arrival, quantiles=QUANTILES)
    assert res.paths is None
    assert_results_identical(full, res, with_paths=False)


# -- case 3: passes ------------------------------------------------------------------
def test_passes_equal_one_pass(monkeypatch):
    monkeypatch.delenv("INFERNO_SIZING_MEMO", raising=False)
    whole, _, _ = case1()
    fs, _ = make_pair(oracle_system, oracle_cur)
    monkeypatch.setattr(fastpath, "ENSEMBLE_PASS_ROWS", 14)  # two paths per pass, then one
    assert fs.memo_stats() is None
    parts = fs.rollout_ensemble(arrival=whole.arrival, quantiles=QUANTILES, return_paths=True)
    assert_results_identical(whole, parts)
    # one lookup per loaded cell and pass
    out_tok = fs.load_override[2]
    want = 0
    for e0 in (0, 2, 4):
        peak = whole.arrival[e0:e0 + 2].reshape(-1, whole.arrival.shape[2]).max(axis=0)
        want += int(((peak[fs.cell_server] > 0) & (out_tok[fs.cell_server] > 0)).sum())
    hits, misses = fs.memo_stats()
    print("memo lookups:", hits + misses, "loaded cells over the three passes:", want)
    assert want == 3 * fs.n_cells - 3  # the last pass is the idle path alone
    assert hits + misses == want


# -- case 4: widths ------------------------------------------------------------------
_WIDTHS = {}


def width_pair():
    if not _WIDTHS:
        _WIDTHS["pair"] = make_pair(oracle_system, oracle_cur)
    return _WIDTHS["pair"]


@pytest.mark.parametrize("n_paths,n_steps", [(1, 1), (2, 1), (63, 1), (64, 1), (65, 1),
                                             (256, 1), (65, 3)])
def test_widths(monkeypatch, n_paths, n_steps):
    monkeypatch.delenv("INFERNO_SIZING_MEMO", raising=False)
    fs, twin = width_pair()
    rng = np.random.default_rng(1000 * n_paths + n_steps)
    scales = rng.uniform(0.0, 3.0, size=(n_paths, n_steps))
    res = fs.rollout_ensemble(scales=scales, quantiles=QUANTILES, return_paths=True)
    base = fs.load_override[0]
    same_bytes(res.arrival, base[None, None, :] * scales.astype(np.float32)[:, :, None],
               "arrival")
    assert_bands_equal_helpers(res)
    for e in sorted({0, n_paths // 2, n_paths - 1}):
        assert_path_equals_rollout(res, e, twin.rollout(arrival=res.arrival[e]))
    if n_paths == 1:  # the path itself at every quantile
        for q in range(len(QUANTILES)):
            same_bytes(res.server_replicas_q[q], res.paths.winners.num_replicas[0], "replicas")
            same_bytes(res.server_cost_q[q], res.paths.winners.cost[0], "cost")
            same_bytes(res.replicas_by_acc_q[q], res.path_replicas_by_acc[0], "totals")
            same_bytes(res.cost_total_q[q], res.path_cost_total[0], "cost total")
        same_bytes(res.acc_mode, res.paths.winners.acc_idx[0], "mode")
        assert (res.acc_mode_paths == 1).all()


# -- case 5: one accelerator ---------------------------------------------------------
def test_one_accelerator(monkeypatch):
    monkeypatch.delenv("INFERNO_SIZING_MEMO", raising=False)
    fs, twin = make_pair(lambda: System.from_spec(
        make_spec(n_servers=6, seed=31, arrival_scale=ARRIVAL_SCALE, n_accelerators=1))[0])
    assert fs.n_cells == 6 and len(fs.acc_names) == 1
    scales = [[1.0, 2.6, 0.0, 0.45], [0.5, 0.0, 3.0, 1.0], [2.0, 2.0, 0.2, 0.0]]
    res = fs.rollout_ensemble(scales=scales, quantiles=QUANTILES, return_paths=True)
    for e in range(3):
        assert_path_equals_rollout(res, e, twin.rollout(arrival=res.arrival[e]))
    assert_bands_equal_helpers(res)
    assert (res.server_replicas_q[0] != res.server_replicas_q[3]).any()


# -- case 6: the other analyzer mode -------------------------------------------------
def test_mg1_mode(monkeypatch):
    monkeypatch.delenv("INFERNO_SIZING_MEMO", raising=False)
    fs, twin = make_pair(lambda: oracle_system("mg1"), oracle_cur)
    base = fs.load_override[0]
    arrival = case1_paths(base)[[0, 2, 4], :3]
    res = fs.rollout_ensemble(arrival=arrival, quantiles=QUANTILES, return_paths=True)
    for e in range(3):
        assert_path_equals_rollout(res, e, twin.rollout(arrival=arrival[e]))
    assert_bands_equal_helpers(res)


# -- case 7: non-interference ----------------------------------------------------------
def test_ensemble_changes_nothing_around_it(monkeypatch):
    monkeypatch.delenv("INFERNO_SIZING_MEMO", raising=False)
    fs, _ = make_pair(oracle_system, oracle_cur)
    arrival = case1_paths(fs.load_override[0])
    w1 = fs.reconcile()
    r1 = fs.rollout(scales=SCALES)
    e1 = fs.rollout_ensemble(arrival=arrival, quantiles=QUANTILES, return_paths=True)
    assert fs._gpu.fused_state()["done_nonzero"] <= 0
    w2 = fs.reconcile()
    r2 = fs.rollout(scales=SCALES)
    for f in dataclasses.fields(w1):
        same_bytes(getattr(w1, f.name), getattr(w2, f.name), f"reconcile {f.name}")
        same_bytes(getattr(r1.winners, f.name), getattr(r2.winners, f.name), f"rollout {f.name}")
    same_bytes(r1.replicas_by_acc, r2.replicas_by_acc, "rollout totals")
    same_bytes(r1.acc_changes, r2.acc_changes, "rollout changes")
    for x, y in zip(r1.final_cur, r2.final_cur):
        same_bytes(x, y, "rollout final_cur")
    e2 = fs.rollout_ensemble(arrival=arrival, quantiles=QUANTILES, return_paths=True)
    assert_results_identical(e1, e2)
    assert fs.cur_override[0][NO_CUR_SRV] == -3  # the overrides are the caller's
