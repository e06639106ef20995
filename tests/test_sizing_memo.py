"""Sizing memo of the native reconcile context (wva_sweep_t): a memo hit must
replay exactly what the sizing phase computed, and the memo must really be
used.

Fleet: 8 servers x 3 accelerators = 24 cells, batch sizes pinned so the cells
cover one state, the 32-state anchor, the 64-wide and 256-wide blocks and the
XL tier; one server has an unreachable SLO (memo status "infeasible").
Comparisons between a memo-on and a memo-off context are bit for bit — the
memo replays a value the same code produced, so no tolerance applies.
"""
import dataclasses

import numpy as np
import pytest

from inferno_amd.core import System
from inferno_amd.engine import FastSweep
from tests.fixtures import make_spec

pytestmark = pytest.mark.gpu

# per-server pinned batch size N (server i -> PINNED_N[i])
PINNED_N = (1, 33, 512, 513, 2048, 2049, 8193, 2049)
INFEASIBLE_SRV = 7  # N = 2049: the 256-wide block's early exit
ZERO_SRV = 3
TICK_SCALE = (1.0, 1.7, 0.6, 2.3)
ARRIVAL_SCALE = 6000.0  # req/min: enough load that replica counts move per tick
CELL_FLOAT_KEYS = ("cost", "value", "itl", "ttft", "rho", "max_rate")
CELL_EXACT_KEYS = ("feasible", "zero_empty", "num_replicas", "batch")


def build_system(seed=901, analyzer_mode=None):
    system, _ = System.from_spec(make_spec(n_servers=8, seed=seed, arrival_scale=ARRIVAL_SCALE))
    names = sorted(system.servers)
    assert len(names) == len(PINNED_N)
    for i, name in enumerate(names):
        system.servers[name].max_batch_size = PINNED_N[i]
    # unreachable SLO, as in test_gpu_sweep.py::test_infeasible_slo
    srv = system.servers[names[INFEASIBLE_SRV]]
    t = system.service_classes[srv.service_class_name].targets[srv.model_name]
    t.itl = 1e-3
    t.ttft = 0.0
    # with a single state the token time does not move with the rate, so any
    # ITL target lies outside the bounded region; size that server on TTFT
    # alone so the N=1 cells take the sized path too
    srv = system.servers[names[0]]
    system.service_classes[srv.service_class_name].targets[srv.model_name].itl = 0.0
    if analyzer_mode is not None:
        system.analyzer_mode = analyzer_mode
    return system


def base_loads(system):
    names = sorted(system.servers)
    arrival = np.array([system.servers[n].load.arrivalRate for n in names], dtype=np.float32)
    in_tok = np.array([system.servers[n].load.avgInTokens for n in names], dtype=np.int32)
    out_tok = np.array([system.servers[n].load.avgOutTokens for n in names], dtype=np.int32)
    assert (arrival > 0).all() and (out_tok > 0).all()
    return arrival, in_tok, out_tok


def initial_cur(system, fs):
    names = fs.server_names
    cur_acc = np.full(len(names), -3, dtype=np.int32)
    cur_rep = np.zeros(len(names), dtype=np.int32)
    cur_cost = np.zeros(len(names), dtype=np.float32)
    for j, name in enumerate(names):
        cur = system.servers[name].cur_allocation
        if cur is not None:
            cur_acc[j] = fs._acc_index.get(cur.accelerator, -1)
            cur_rep[j] = cur.num_replicas
            cur_cost[j] = cur.cost
    return cur_acc, cur_rep, cur_cost


def feed_back(cur, w):
    """desired -> current between ticks, as the benchmark's steady-state loop"""
    pa, pr, pc = cur
    ok = w.acc_idx != -1
    return (
        np.where(ok, np.where(w.acc_idx == -2, -1, w.acc_idx), pa).astype(np.int32),
        np.where(ok, w.num_replicas, pr).astype(np.int32),
        np.where(ok, w.cost, pc).astype(np.float32),
    )


def tick_arrival(arrival, tick, zero_tick):
    a = (arrival * np.float32(TICK_SCALE[tick])).astype(np.float32)
    if zero_tick is not None and tick == zero_tick:
        a[ZERO_SRV] = 0.0
    return a


def run_ticks(system, n_ticks, zero_tick=None):
    """Drive a fresh FastSweep for n_ticks; per tick return the winner record
    and the per-cell arrays. The first tick reads the per-cell arrays BEFORE
    the winners, so the miss path's per-cell output is what gets compared."""
    fs = FastSweep(system, backend="gpu")
    assert fs.n_cells == 24
    arrival, in_tok, out_tok = base_loads(system)
    cur = initial_cur(system, fs)
    ticks = []
    for tick in range(n_ticks):
        fs.load_override = (tick_arrival(arrival, tick, zero_tick), in_tok, out_tok)
        fs.cur_override = cur
        if tick == 0:
            cells = fs.reconcile_cells()
            winners = fs.reconcile()
        else:
            winners = fs.reconcile()
            cells = fs.reconcile_cells()
        ticks.append((winners, {k: v.copy() for k, v in cells.items()}))
        cur = feed_back(cur, winners)
    return ticks, fs.memo_stats()


def assert_on_equals_off(monkeypatch, n_ticks, zero_tick=None, analyzer_mode=None):
    monkeypatch.setenv("INFERNO_SIZING_MEMO", "0")
    off, off_stats = run_ticks(build_system(analyzer_mode=analyzer_mode), n_ticks, zero_tick)
    monkeypatch.delenv("INFERNO_SIZING_MEMO")
    on, on_stats = run_ticks(build_system(analyzer_mode=analyzer_mode), n_ticks, zero_tick)
    assert off_stats is None, "kill switch did not disable the memo"
    assert on_stats is not None and on_stats[0] > 0, "memo was not used"
    for tick, ((w_off, c_off), (w_on, c_on)) in enumerate(zip(off, on)):
        for f in dataclasses.fields(w_off):
            a, b = getattr(w_off, f.name), getattr(w_on, f.name)
            assert np.array_equal(a, b), f"tick {tick}: winner {f.name} differs"
        for k in CELL_EXACT_KEYS:
            assert np.array_equal(c_off[k], c_on[k]), f"tick {tick}: cell {k} differs"
        feas = c_off["feasible"].astype(bool)
        for k in CELL_FLOAT_KEYS:
            assert np.array_equal(c_off[k][feas], c_on[k][feas]), (
                f"tick {tick}: cell {k} differs"
            )
    return off, on


def test_memo_on_equals_memo_off_bit_for_bit(monkeypatch):
    off, _ = assert_on_equals_off(monkeypatch, n_ticks=4, zero_tick=1)
    # the fixture exercises what it claims to (feasibility as the CPU golden
    # path gives it): the unreachable-SLO server never has a feasible cell,
    # every other cell is sized at its pinned batch size, and the zero-load
    # server takes the zero path on its tick only
    pinned = np.asarray(PINNED_N)
    for tick, (w, c) in enumerate(off):
        srv = c["cell_server"]
        assert np.array_equal(c["feasible"].astype(bool), srv != INFEASIBLE_SRV)
        assert w.acc_idx[INFEASIBLE_SRV] == -1
        sized = (srv != INFEASIBLE_SRV) & ((srv != ZERO_SRV) | (tick != 1))
        assert np.array_equal(c["batch"][sized], pinned[srv[sized]])
        zero = (srv == ZERO_SRV) & (tick == 1)
        assert (c["rho"][zero] == 0).all()


def test_memo_is_used(monkeypatch):
    monkeypatch.delenv("INFERNO_SIZING_MEMO", raising=False)
    system = build_system()
    fs = FastSweep(system, backend="gpu")
    assert fs.memo_stats() is None  # no native context yet
    arrival, in_tok, out_tok = base_loads(system)
    cur = initial_cur(system, fs)
    n_loaded = int(((arrival[fs.cell_server] != 0) & (out_tok[fs.cell_server] != 0)).sum())
    assert n_loaded == fs.n_cells == 24

    def tick(i, in_tok_now):
        nonlocal cur
        fs.load_override = (tick_arrival(arrival, i, None), in_tok_now, out_tok)
        fs.cur_override = cur
        cur = feed_back(cur, fs.reconcile())
        return fs.memo_stats()

    assert tick(0, in_tok) == (0, n_loaded)
    # new arrival rates only: every loaded cell hits, none misses
    assert tick(1, in_tok) == (n_loaded, n_loaded)
    # one server's token average moves: exactly its cells miss...
    changed = 2
    n_changed = int((fs.cell_server == changed).sum())
    assert n_changed == 3
    in_tok2 = in_tok.copy()
    in_tok2[changed] += 1
    assert tick(2, in_tok2) == (2 * n_loaded - n_changed, n_loaded + n_changed)
    # ...and hit again on the following tick
    assert tick(3, in_tok2) == (3 * n_loaded - n_changed, n_loaded + n_changed)


def test_gmem_instantiation(monkeypatch):
    # as test_gpu_sweep.py::test_gmem_cells_match_cpu: the N=8193 cells take
    # the global-memory spill path
    import inferno_amd.ops.sweep as sweep

    monkeypatch.setattr(sweep, "XL_MAX_N", sweep.MAX_N)
    assert_on_equals_off(monkeypatch, n_ticks=2)


def test_mg1_mode(monkeypatch):
    assert_on_equals_off(monkeypatch, n_ticks=2, analyzer_mode="mg1")
