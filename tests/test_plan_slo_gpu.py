"""SLO planning on the GPU (FastSweep.plan_slo): every (target set, load) slice
must be bit for bit what the single-scenario path computes — reconcile_cells /
reconcile on a fresh context of an identical system with that slice's targets
written to its Target objects and that slice's arrival rates as the load.

Fleet: the one of tests/test_plan_gpu.py, 9 servers x 3 accelerators = 27 cells
with batch sizes pinned to 1, 33, 512, 513, 2048, 2049, 8193, 2049, 32769 (one
state, the anchor boundary, both block widths, the XL tier, the global-memory
tier), the unreachable-SLO server, the TTFT-only N = 1 server, the TPS-target
server and the scale-to-zero server. SLO scales (1.0, 0.25, 0.5, 2.0) times load
scales (1.0, 0.0, 1.7): at 0.25 single cells turn infeasible while their server
keeps a candidate, next to feasible target sets of the same cell.

Observed on MI355X for test_gpu_plan_slo_matches_cpu_plan_slo: 0 replica flips of
108 winners.
"""
import dataclasses

import numpy as np
import pytest

from inferno_amd.engine import FastSweep
from tests.test_plan_gpu import (
    CELL_EXACT_KEYS,
    CELL_FLOAT_KEYS,
    INFEASIBLE_SRV,
    PINNED_N,
    SCALE_TO_ZERO_SRV,
    SCALES,
    ZERO_SRV,
    assert_results_identical,
    assert_winners_identical,
    base_loads,
    bits,
    build_system,
    feed_back,
    initial_cur,
    make_planner,
)

pytestmark = pytest.mark.gpu

SLO_SCALES = (1.0, 0.25, 0.5, 2.0)
LOAD_SCALES = (1.0, 0.0, 1.7)
N_LOADED_CELLS = 27
TTFT_OFF_SRV = 5  # explicit targets: TTFT 0 in one target set only
ITL_TIGHT_SRV = 6  # explicit targets: ITL 1e-3 in one target set only
# cells (server, accelerator) a four times tighter SLO makes infeasible while
# the server keeps a candidate (the CPU golden's table, tests/test_plan_slo_cpu.py)
INFEASIBLE_AT_QUARTER = {3: (True, False, True), 4: (True, True, False), 8: (False, True, False)}


def targets_of(system):
    out = []
    for name in sorted(system.servers):
        srv = system.servers[name]
        out.append(system.service_classes[srv.service_class_name].targets[srv.model_name])
    return out


def base_targets():
    t = targets_of(build_system())
    return (np.array([x.ttft for x in t], dtype=np.float32),
            np.array([x.itl for x in t], dtype=np.float32))


def scaled_grid():
    ttft, itl = base_targets()
    arrival, _, _ = base_loads(build_system())
    t_ttft = np.stack([ttft * np.float32(sc) for sc in SLO_SCALES]).astype(np.float32)
    t_itl = np.stack([itl * np.float32(sc) for sc in SLO_SCALES]).astype(np.float32)
    scen = np.stack([arrival * np.float32(sc) for sc in LOAD_SCALES]).astype(np.float32)
    return t_ttft, t_itl, scen


def explicit_grid():
    ttft, itl = base_targets()
    arrival, _, _ = base_loads(build_system())
    t_ttft = np.stack([ttft, ttft, ttft, ttft]).astype(np.float32)
    t_itl = np.stack([itl, itl, itl, itl]).astype(np.float32)
    assert ttft[TTFT_OFF_SRV] > 0 and itl[TTFT_OFF_SRV] > 0 and itl[ITL_TIGHT_SRV] > 1e-3
    t_ttft[1, TTFT_OFF_SRV] = 0.0
    t_itl[2, ITL_TIGHT_SRV] = 1e-3
    t_itl[3, INFEASIBLE_SRV] = 200.0  # reachable, where the server's own target is not
    scen = np.stack([arrival, arrival * np.float32(1.7)]).astype(np.float32)
    scen[1, ZERO_SRV] = 0.0
    return t_ttft, t_itl, scen


def oracle(t_ttft, t_itl, scen, analyzer_mode=None):
    """The single-scenario path: per (t, s) a fresh context on an identical
    system with target set t on its Target objects, per-cell arrays first
    (miss path), then the winners."""
    out = {}
    for t in range(t_ttft.shape[0]):
        for s in range(scen.shape[0]):
            system = build_system(analyzer_mode=analyzer_mode)
            for i, tgt in enumerate(targets_of(system)):
                tgt.ttft, tgt.itl = float(t_ttft[t, i]), float(t_itl[t, i])
            fs = FastSweep(system, backend="gpu")
            assert fs.n_cells == 27
            _, in_tok, out_tok = base_loads(system)
            fs.load_override = (scen[s].copy(), in_tok, out_tok)
            fs.cur_override = initial_cur(system, fs)
            cells = fs.reconcile_cells()
            winners = fs.reconcile()
            out[t, s] = (winners, {k: v.copy() for k, v in cells.items()})
    return out


_ORACLE = {}


def cached_oracle(kind, analyzer_mode=None):
    key = (kind, analyzer_mode)
    if key not in _ORACLE:
        grid = scaled_grid() if kind == "scales" else explicit_grid()
        _ORACLE[key] = (grid, oracle(*grid, analyzer_mode=analyzer_mode))
    return _ORACLE[key]


def slice_winner(w, t, s):
    return type(w)(**{f.name: getattr(w, f.name)[t, s] for f in dataclasses.fields(w)})


def assert_slo_plan_equals_oracle(res, ref, t_index=None):
    """Every slice of res against ref[(t, s)]; t_index maps res's target axis
    to the oracle's (default: identity)."""
    assert res.cells is not None
    n_t, n_s = res.winners.acc_idx.shape[:2]
    for t in range(n_t):
        for s in range(n_s):
            w_ref, c_ref = ref[t if t_index is None else t_index[t], s]
            where = f"slice ({t}, {s})"
            for k in CELL_EXACT_KEYS:
                assert np.array_equal(res.cells[k][t, s], c_ref[k]), f"{where}: cell {k} differs"
            feas = c_ref["feasible"].astype(bool)
            for k in CELL_FLOAT_KEYS:
                assert np.array_equal(bits(res.cells[k][t, s])[feas], bits(c_ref[k])[feas]), (
                    f"{where}: cell {k} differs"
                )
            assert_winners_identical(slice_winner(res.winners, t, s), w_ref, where)


def assert_slo_results_identical(a, b):
    assert_winners_identical(a.winners, b.winners, "plan_slo")
    assert np.array_equal(a.replicas_by_acc, b.replicas_by_acc)
    assert np.array_equal(a.cost_total, b.cost_total)
    assert np.array_equal(a.infeasible_servers, b.infeasible_servers)
    for k in CELL_EXACT_KEYS:
        assert np.array_equal(a.cells[k], b.cells[k]), k
    feas = a.cells["feasible"].astype(bool)
    for k in CELL_FLOAT_KEYS:
        assert np.array_equal(bits(a.cells[k])[feas], bits(b.cells[k])[feas]), k


def assert_totals(fs, res):
    w = res.winners
    n_t, n_s = w.acc_idx.shape[:2]
    assert res.replicas_by_acc.dtype == np.int64
    assert res.replicas_by_acc.shape == (n_t, n_s, len(fs.acc_names))
    for t in range(n_t):
        for s in range(n_s):
            want = np.zeros(len(fs.acc_names), dtype=np.int64)
            on = w.acc_idx[t, s] >= 0
            np.add.at(want, w.acc_idx[t, s][on], w.num_replicas[t, s][on].astype(np.int64))
            assert np.array_equal(res.replicas_by_acc[t, s], want)
            has = w.acc_idx[t, s] != -1
            assert res.cost_total[t, s] == w.cost[t, s][has].astype(np.float64).sum()
            assert res.infeasible_servers[t, s] == int((~has).sum())


def test_fixture_covers_what_it_claims():
    (t_ttft, t_itl, scen), ref = cached_oracle("scales")
    pinned = np.asarray(PINNED_N)
    quarter, one, load = SLO_SCALES.index(0.25), SLO_SCALES.index(1.0), LOAD_SCALES.index(1.0)
    for (t, s), (w, c) in ref.items():
        srv = c["cell_server"]
        if LOAD_SCALES[s] == 0.0:
            assert c["feasible"].all()  # the zero-traffic decision comes first
            assert w.acc_idx[SCALE_TO_ZERO_SRV] == -2
            continue
        assert not c["feasible"][srv == INFEASIBLE_SRV].any()
        assert w.acc_idx[INFEASIBLE_SRV] == -1
        sized = c["feasible"].astype(bool)
        assert np.array_equal(c["batch"][sized], pinned[srv[sized]])
        if t != quarter:
            assert np.array_equal(sized, srv != INFEASIBLE_SRV)
    # 0.25: single cells infeasible while their server keeps a candidate, and
    # the same cells are feasible under the other target sets
    c_q, c_1 = ref[quarter, load][1], ref[one, load][1]
    for srv, want in INFEASIBLE_AT_QUARTER.items():
        at = c_q["cell_server"] == srv
        assert np.array_equal(~c_q["feasible"][at].astype(bool), np.array(want)), srv
        assert c_1["feasible"][at].all()
        assert ref[quarter, load][0].acc_idx[srv] >= 0
    # ...and some server's winner moves to another accelerator
    a_q, a_1 = ref[quarter, load][0].acc_idx, ref[one, load][0].acc_idx
    assert ((a_q != a_1) & (a_q >= 0) & (a_1 >= 0)).any()
    # replicas grow as the targets tighten (2.0 -> 1.0 -> 0.5 -> 0.25)
    order = [SLO_SCALES.index(x) for x in (2.0, 1.0, 0.5, 0.25)]
    for srv in (0, 3, 6, 8):
        for k in np.nonzero(c_1["cell_server"] == srv)[0]:
            col = [int(ref[t, load][1]["num_replicas"][k]) for t in order
                   if ref[t, load][1]["feasible"][k]]
            assert col == sorted(col) and col[0] < col[-1], (srv, k, col)


def test_cold_and_warm_plan_match_single_scenario_path(monkeypatch):
    monkeypatch.delenv("INFERNO_SIZING_MEMO", raising=False)
    (t_ttft, t_itl, scen), ref = cached_oracle("scales")
    fs = make_planner()
    assert fs.memo_stats() is None  # no context yet: plan_slo is its first call
    cold = fs.plan_slo(slo_scales=SLO_SCALES, scales=LOAD_SCALES, return_cells=True)
    assert np.array_equal(cold.arrival, scen)
    assert np.array_equal(bits(cold.t_ttft), bits(t_ttft))
    assert np.array_equal(bits(cold.t_itl), bits(t_itl))
    assert cold.cells["feasible"].shape == (len(SLO_SCALES), len(LOAD_SCALES), 27)
    assert_slo_plan_equals_oracle(cold, ref)
    assert_totals(fs, cold)
    # one lookup per loaded cell, through the base-target set only
    assert fs.memo_stats() == (0, N_LOADED_CELLS)
    warm = fs.plan_slo(slo_scales=SLO_SCALES, scales=LOAD_SCALES, return_cells=True)
    assert fs.memo_stats() == (N_LOADED_CELLS, N_LOADED_CELLS)
    assert_slo_results_identical(cold, warm)
    # no target set at the base targets: the memo is neither read nor written
    part = fs.plan_slo(slo_scales=(0.25, 0.5), scales=LOAD_SCALES)
    assert fs.memo_stats() == (N_LOADED_CELLS, N_LOADED_CELLS)
    for t, t_ref in enumerate((1, 2)):
        for s in range(len(LOAD_SCALES)):
            assert_winners_identical(slice_winner(part.winners, t, s), ref[t_ref, s][0],
                                     f"slice ({t}, {s})")
    # (per-cell arrays on a fresh context: an infeasible cell gets only its two
    # flags written, so its other fields are whatever the buffers held)
    fresh = make_planner()
    part = fresh.plan_slo(slo_scales=(0.25, 0.5), scales=LOAD_SCALES, return_cells=True)
    assert fresh.memo_stats() == (0, 0)
    assert_slo_plan_equals_oracle(part, ref, t_index=(1, 2))


def test_explicit_targets(monkeypatch):
    """TTFT 0 in one target set only, an unreachable ITL for an otherwise
    feasible server in one target set only, one server at zero load in one
    load scenario only; and a reachable ITL in one target set only for the
    server whose own target is unreachable, memo-cold and memo-warm (the warm
    call replays the memo's infeasible verdict for the base set alone)."""
    monkeypatch.delenv("INFERNO_SIZING_MEMO", raising=False)
    (t_ttft, t_itl, scen), ref = cached_oracle("explicit")
    fs = make_planner()
    res = fs.plan_slo(targets=(t_ttft, t_itl), arrival=scen, return_cells=True)
    assert_slo_plan_equals_oracle(res, ref)
    assert_totals(fs, res)
    assert (res.winners.acc_idx[[0, 1, 3], :, ITL_TIGHT_SRV] >= 0).all()
    assert (res.winners.acc_idx[2, :, ITL_TIGHT_SRV] == -1).all()
    assert (res.winners.acc_idx[:3, :, INFEASIBLE_SRV] == -1).all()
    assert (res.winners.acc_idx[3, :, INFEASIBLE_SRV] >= 0).all()
    assert (res.winners.acc_idx[:, :, TTFT_OFF_SRV] >= 0).all()
    off = res.cells["cell_server"] == TTFT_OFF_SRV
    assert (res.cells["num_replicas"][1, 0][off] <= res.cells["num_replicas"][0, 0][off]).all()
    assert (res.winners.acc_idx[:, 1, ZERO_SRV] >= 0).all()  # min_replicas = 1 stays allocated
    assert (res.winners.rho[:, 1, ZERO_SRV] == 0).all()
    # target set 0 is at the base targets: one lookup per cell
    assert fs.memo_stats() == (0, N_LOADED_CELLS)
    warm = fs.plan_slo(targets=(t_ttft, t_itl), arrival=scen, return_cells=True)
    assert fs.memo_stats() == (N_LOADED_CELLS, N_LOADED_CELLS)
    assert_slo_results_identical(res, warm)


def test_reconcile_plan_slo_reconcile(monkeypatch):
    """Planning between two reconciles changes neither and costs the second
    one no memo miss."""
    monkeypatch.delenv("INFERNO_SIZING_MEMO", raising=False)

    def run(with_plan):
        fs = make_planner()
        arrival, in_tok, out_tok = fs.load_override
        cur = fs.cur_override
        w1 = fs.reconcile()
        p = (fs.plan_slo(slo_scales=SLO_SCALES, scales=LOAD_SCALES, return_cells=True)
             if with_plan else None)
        before = fs.memo_stats()
        fs.load_override = ((arrival * np.float32(1.7)).astype(np.float32), in_tok, out_tok)
        fs.cur_override = feed_back(cur, w1)
        w2 = fs.reconcile()
        after = fs.memo_stats()
        return w1, p, w2, (after[0] - before[0], after[1] - before[1])

    w1, p, w2, moved = run(True)
    t1, _, t2, moved_twin = run(False)
    assert_winners_identical(w1, t1, "first reconcile")
    assert_winners_identical(w2, t2, "second reconcile")
    assert moved == moved_twin == (N_LOADED_CELLS, 0)  # every loaded cell hits
    assert SLO_SCALES[0] == 1.0 and LOAD_SCALES[0] == 1.0
    assert_winners_identical(slice_winner(p.winners, 0, 0), w1, "base slice")
    _, ref = cached_oracle("scales")
    assert_slo_plan_equals_oracle(p, ref)


def test_base_targets_equal_load_plan(monkeypatch):
    monkeypatch.delenv("INFERNO_SIZING_MEMO", raising=False)
    a = make_planner().plan_slo(slo_scales=[1.0], scales=SCALES, return_cells=True)
    b = make_planner().plan(scales=SCALES, return_cells=True)
    flat = dataclasses.replace(
        a,
        winners=slice_all(a.winners),
        replicas_by_acc=a.replicas_by_acc[0],
        cost_total=a.cost_total[0],
        cells={k: (v[0] if k in CELL_EXACT_KEYS + CELL_FLOAT_KEYS else v)
               for k, v in a.cells.items()},
    )
    assert_results_identical(flat, b)
    for k in CELL_FLOAT_KEYS:  # all bytes, infeasible cells included
        assert np.array_equal(bits(flat.cells[k]), bits(b.cells[k])), k
    assert np.array_equal(a.infeasible_servers[0], b.infeasible_servers)
    assert np.array_equal(a.arrival, b.arrival)


def slice_all(w):
    return type(w)(**{f.name: getattr(w, f.name)[0] for f in dataclasses.fields(w)})


def test_memo_off(monkeypatch):
    _, ref = cached_oracle("scales")
    monkeypatch.setenv("INFERNO_SIZING_MEMO", "0")
    fs = make_planner()
    res = fs.plan_slo(slo_scales=SLO_SCALES, scales=LOAD_SCALES, return_cells=True)
    assert fs.memo_stats() is None, "kill switch did not disable the memo"
    assert_slo_plan_equals_oracle(res, ref)
    again = fs.plan_slo(slo_scales=SLO_SCALES, scales=LOAD_SCALES, return_cells=True)
    assert_slo_results_identical(res, again)


def test_mg1_mode(monkeypatch):
    monkeypatch.delenv("INFERNO_SIZING_MEMO", raising=False)
    _, ref = cached_oracle("scales", "mg1")
    fs = make_planner(analyzer_mode="mg1")
    cold = fs.plan_slo(slo_scales=SLO_SCALES, scales=LOAD_SCALES, return_cells=True)
    assert_slo_plan_equals_oracle(cold, ref)
    warm = fs.plan_slo(slo_scales=SLO_SCALES, scales=LOAD_SCALES, return_cells=True)
    assert_slo_results_identical(cold, warm)


def test_growing_grid_and_validation(monkeypatch):
    monkeypatch.delenv("INFERNO_SIZING_MEMO", raising=False)
    _, ref = cached_oracle("scales")
    fs = make_planner()
    one = fs.plan_slo(slo_scales=SLO_SCALES[:1], return_cells=True)  # buffers sized for 1 slice
    assert one.winners.acc_idx.shape == (1, 1, 9)
    assert_slo_plan_equals_oracle(one, ref)
    res = fs.plan_slo(slo_scales=SLO_SCALES, scales=LOAD_SCALES, return_cells=True)  # ...12
    assert_slo_plan_equals_oracle(res, ref)
    stats = fs.memo_stats()
    ttft, itl = base_targets()
    for kwargs in (
        {"slo_scales": [1.0] * 257},
        {"slo_scales": [1.0] * 86, "scales": LOAD_SCALES},  # 258 slices
        {"slo_scales": [1.0, 0.0]},
        {"slo_scales": [1.0, -1.0]},
        {"slo_scales": [1.0, float("nan")]},
        {"slo_scales": [1.0], "targets": (ttft[None, :], itl[None, :])},
        {},
        {"targets": (ttft[None, :8], itl[None, :8])},
        {"slo_scales": [1.0], "scales": [1.0, -1.0]},
    ):
        with pytest.raises(ValueError):
            fs.plan_slo(**kwargs)
    assert fs.memo_stats() == stats  # nothing was launched


def test_gpu_plan_slo_matches_cpu_plan_slo():
    """GPU plan_slo against the golden CPU plan_slo under the rule of
    tests/test_plan_gpu.py::test_gpu_plan_matches_cpu_plan: equal accelerators;
    replica counts may differ by one (a ceil boundary inside the bisection
    tolerance) for at most max(1, n // 50) of the n = 108 (server, slice)
    winners; that test's field tolerances for the rest.

    Observed on MI355X: 0 of 108 winners flipped."""
    g = FastSweep(build_system(), backend="gpu").plan_slo(
        slo_scales=SLO_SCALES, scales=LOAD_SCALES).winners
    c = FastSweep(build_system(), backend="cpu").plan_slo(
        slo_scales=SLO_SCALES, scales=LOAD_SCALES).winners
    assert np.array_equal(g.acc_idx, c.acc_idx)
    n = g.acc_idx.size
    assert n == 108
    flips = 0
    for at in np.ndindex(g.acc_idx.shape):
        where = f"(target set, load, server) {at}"
        if c.num_replicas[at] != g.num_replicas[at]:
            flips += 1
            assert abs(int(c.num_replicas[at]) - int(g.num_replicas[at])) <= 1, where
            assert c.cost[at] == pytest.approx(g.cost[at], rel=5e-2), where
            continue
        assert c.batch[at] == g.batch[at], where
        assert c.cost[at] == pytest.approx(g.cost[at], rel=1e-5, abs=1e-4), where
        assert c.value[at] == pytest.approx(g.value[at], rel=1e-4, abs=1e-3), where
        assert c.itl[at] == pytest.approx(g.itl[at], rel=1e-3, abs=1e-4), where
        assert c.ttft[at] == pytest.approx(g.ttft[at], rel=2e-3, abs=1e-3), where
        assert c.rho[at] == pytest.approx(g.rho[at], rel=1e-3, abs=1e-5), where
        assert c.max_rate[at] == pytest.approx(g.max_rate[at], rel=1e-4, abs=1e-9), where
    print(f"replica flips: {flips} of {n}")
    assert flips <= max(1, n // 50)
