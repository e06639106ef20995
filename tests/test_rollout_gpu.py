"""Forecast rollout on the GPU (FastSweep.rollout): step s must be bit for bit
what the single-tick path (reconcile_cells / reconcile on a second context,
with row s as the load and the fed-back allocation as the current one)
computes.

Every comparison is raw bits. The two per-cell flags are compared on every
cell, the other eight per-cell arrays on the feasible cells: an infeasible cell
stores only its two flags, on either path, and keeps whatever an earlier tick
(the tick loop) or nothing (the rollout's buffers) left in the rest.

Fleets are small and every cell's batch size is pinned <= 64 through the
per-cell override row (as tests/test_fused_tick_gpu.py::make_fs does).
"""
import dataclasses

import numpy as np
import pytest

from inferno_amd.config import (
    AcceleratorSpec,
    DecodeParms,
    ModelAcceleratorPerfData,
    PrefillParms,
)
from inferno_amd.core import System
from inferno_amd.engine import FastSweep, feed_back
from inferno_amd.engine import fastpath
from inferno_amd.utils.synthetic import make_fleet_spec
from tests.fixtures import make_spec

pytestmark = pytest.mark.gpu

# cycled over the cells. A one-state cell is sized whatever its ITL target
# (see tests/test_plan_gpu.py), so the period keeps N = 1 off the server with
# the unreachable SLO (cells 18..20 of the oracle fleet).
CELL_N = (1, 5, 16, 33, 64, 48, 7, 2)
ARRIVAL_SCALE = 6000.0  # req/min: enough load that replica counts move per step
# rises, falls, a zero row, comes back. On the zero row the server with the
# unreachable SLO keeps its load (oracle_rows): at zero load its cells would
# take the zero path, which is feasible whatever the SLO.
SCALES = (1.0, 2.3, 3.1, 0.6, 0.0, 0.37, 1.7)
ZERO_STEP = 4
INFEASIBLE_SRV, SCALE_TO_ZERO_SRV, TPS_SRV, NO_CUR_SRV, UNKNOWN_CUR_SRV = 6, 4, 2, 1, 5
CELL_FLAG_KEYS = ("feasible", "zero_empty")
CELL_INT_KEYS = ("num_replicas", "batch")
CELL_FLOAT_KEYS = ("cost", "value", "itl", "ttft", "rho", "max_rate")
WINNER_FLOAT = ("cost", "value", "itl", "ttft", "rho", "max_rate")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


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
    whose accelerator the fleet does not know (empty code, replicas and cost
    kept)."""
    cur_acc, cur_rep, cur_cost = (np.array(a) for a in fs._base_cur())
    cur_acc[NO_CUR_SRV], cur_rep[NO_CUR_SRV], cur_cost[NO_CUR_SRV] = -3, 0, 0.0
    cur_acc[UNKNOWN_CUR_SRV], cur_rep[UNKNOWN_CUR_SRV], cur_cost[UNKNOWN_CUR_SRV] = -1, 3, 123.25
    return cur_acc, cur_rep, cur_cost


def oracle_rows(base):
    scen = np.stack([base * np.float32(sc) for sc in SCALES]).astype(np.float32)
    scen[ZERO_STEP, INFEASIBLE_SRV] = base[INFEASIBLE_SRV]
    return scen


def make_pair(build, cur_of=None):
    """The same fleet twice: the one that rolls out and the one that ticks."""
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


def tick_loop(ref, scen):
    """One reconcile_cells() + reconcile() per row on ``ref``, the winner fed
    back as the current allocation: [(winners, cells, cur after)]."""
    _, in_tok, out_tok = ref.load_override
    cur = ref.cur_override
    saved = (ref.load_override, ref.cur_override)
    out = []
    for s in range(scen.shape[0]):
        ref.load_override = (scen[s].copy(), in_tok, out_tok)
        ref.cur_override = cur
        cells = {k: v.copy() for k, v in ref.reconcile_cells().items()}
        w = ref.reconcile()
        cur = feed_back(cur, w)
        out.append((w, cells, cur))
    ref.load_override, ref.cur_override = saved
    return out


def assert_winner_equal(a, b, what):
    for f in dataclasses.fields(a):
        x, y = getattr(a, f.name), getattr(b, f.name)
        assert x.dtype == y.dtype, f"{what}: winner {f.name} dtype"
        if f.name in WINNER_FLOAT:
            assert np.array_equal(bits(x), bits(y)), f"{what}: winner {f.name} differs"
        else:
            assert np.array_equal(x, y), f"{what}: winner {f.name} differs"


def slice_winner(w, s):
    return type(w)(**{f.name: getattr(w, f.name)[s] for f in dataclasses.fields(w)})


def assert_rollout_equals_loop(res, ref_rows, start_acc):
    assert res.cells is not None
    before = start_acc
    for s, (w, cells, cur) in enumerate(ref_rows):
        what = f"step {s}"
        assert_winner_equal(slice_winner(res.winners, s), w, what)
        for k in CELL_FLAG_KEYS:
            assert np.array_equal(res.cells[k][s], cells[k]), f"{what}: cell {k} differs"
        feas = cells["feasible"].astype(bool)
        for k in CELL_INT_KEYS:
            assert np.array_equal(res.cells[k][s][feas], cells[k][feas]), (
                f"{what}: cell {k} differs")
        for k in CELL_FLOAT_KEYS:
            assert np.array_equal(bits(res.cells[k][s])[feas], bits(cells[k])[feas]), (
                f"{what}: cell {k} differs")
        assert res.acc_changes[s] == int((cur[0] != before).sum()), what
        before = cur[0]
        on = w.acc_idx >= 0
        want = np.zeros(res.replicas_by_acc.shape[1], dtype=np.int64)
        np.add.at(want, w.acc_idx[on], w.num_replicas[on].astype(np.int64))
        assert np.array_equal(res.replicas_by_acc[s], want), what
        has = w.acc_idx != -1
        assert res.cost_total[s] == w.cost[has].astype(np.float64).sum(), what
        assert res.infeasible_servers[s] == int((~has).sum()), what
    for got, want in zip(res.final_cur, ref_rows[-1][2]):
        assert got.dtype == want.dtype
        assert got.tobytes() == want.tobytes(), "final_cur differs"


def assert_results_identical(a, b):
    assert_winner_equal(a.winners, b.winners, "rollout")
    assert np.array_equal(a.replicas_by_acc, b.replicas_by_acc)
    assert np.array_equal(a.cost_total, b.cost_total)
    assert np.array_equal(a.acc_changes, b.acc_changes)
    for x, y in zip(a.final_cur, b.final_cur):
        assert x.tobytes() == y.tobytes()
    for k in CELL_FLAG_KEYS:
        assert np.array_equal(a.cells[k], b.cells[k]), k
    feas = a.cells["feasible"].astype(bool)
    for k in CELL_INT_KEYS:
        assert np.array_equal(a.cells[k][feas], b.cells[k][feas]), k
    for k in CELL_FLOAT_KEYS:
        assert np.array_equal(bits(a.cells[k])[feas], bits(b.cells[k])[feas]), k


_ORACLE = {}


def oracle(analyzer_mode=None):
    """(rollout, its FastSweep, the tick loop's rows, the rows evaluated)."""
    if analyzer_mode not in _ORACLE:
        fs, ref = make_pair(lambda: oracle_system(analyzer_mode), oracle_cur)
        assert fs.n_cells == 24
        res = fs.rollout(arrival=oracle_rows(fs.load_override[0]), return_cells=True)
        _ORACLE[analyzer_mode] = (res, fs, tick_loop(ref, res.arrival))
    return _ORACLE[analyzer_mode]


# -- oracle --------------------------------------------------------------------
@pytest.mark.parametrize("analyzer_mode", [None, "mg1"])
def test_rollout_equals_tick_loop(monkeypatch, analyzer_mode):
    monkeypatch.delenv("INFERNO_SIZING_MEMO", raising=False)
    res, fs, rows = oracle(analyzer_mode)
    assert np.array_equal(res.arrival, oracle_rows(fs.load_override[0]))
    assert_rollout_equals_loop(res, rows, fs.cur_override[0])


def test_fixture_covers_what_it_claims():
    res, fs, rows = oracle()
    acc = res.winners.acc_idx
    zero = SCALES.index(0.0)
    assert zero == ZERO_STEP
    # never a winner: the allocation it started with is the one it ends with
    assert (acc[:, INFEASIBLE_SRV] == -1).all()
    for k in range(3):
        assert res.final_cur[k][INFEASIBLE_SRV] == fs.cur_override[k][INFEASIBLE_SRV]
    assert fs.cur_override[0][INFEASIBLE_SRV] >= 0
    # goes empty on the zero row and comes back from empty
    assert acc[zero, SCALE_TO_ZERO_SRV] == -2 and acc[zero + 1, SCALE_TO_ZERO_SRV] >= 0
    assert rows[zero][2][0][SCALE_TO_ZERO_SRV] == -1
    # the throughput-target server's replica count does not move with the load
    loaded = [s for s, sc in enumerate(SCALES) if sc > 0]
    tps = res.cells["cell_server"] == TPS_SRV
    for s in loaded[1:]:
        assert np.array_equal(res.cells["num_replicas"][s][tps],
                              res.cells["num_replicas"][loaded[0]][tps])
    # no current allocation: step 0's value is the plain cost, on every cell
    none = res.cells["cell_server"] == NO_CUR_SRV
    assert np.array_equal(bits(res.cells["value"][0][none]), bits(res.cells["cost"][0][none]))
    # an unknown current accelerator is a switch whatever wins
    unknown = (res.cells["cell_server"] == UNKNOWN_CUR_SRV) & res.cells["feasible"][0].astype(bool)
    assert unknown.any()
    assert (res.cells["value"][0][unknown]
            > res.cells["cost"][0][unknown] - np.float32(123.25)).all()
    # the rollout is not plan(): step 0 moves servers, so from step 1 on the
    # same rows are judged against another allocation than plan() judges them
    assert res.acc_changes[0] > 0
    plan = fs.plan(arrival=res.arrival, return_cells=True)
    assert_winner_equal(slice_winner(plan.winners, 0), slice_winner(res.winners, 0), "step 0")
    assert (bits(plan.winners.value[1:]) != bits(res.winners.value[1:])).any()
    feas = res.cells["feasible"][1:].astype(bool)
    assert (bits(plan.cells["value"][1:])[feas] != bits(res.cells["value"][1:])[feas]).any()
    print("(step, server) pairs whose accelerator differs from plan():",
          int((plan.winners.acc_idx != acc).sum()))


# -- group shapes ---------------------------------------------------------------
def wide_fleet():
    """3 servers whose candidates are 70 accelerators: segments longer than a
    wave. Costs that fp32 does not hold exactly, so cost - cur_cost rounds."""
    accs = [AcceleratorSpec(name=f"ACC{j:02d}", type=f"T{j % 5}", multiplicity=1,
                            cost=65.37 + 0.73 * j) for j in range(70)]
    rng = np.random.default_rng(12)
    profiles = {}
    for i in range(3):
        base = rng.uniform([6, 0.05, 1, 2e-4], [30, 0.6, 12, 6e-3])
        profiles[f"model-{i:05d}"] = [
            ModelAcceleratorPerfData(
                name=f"model-{i:05d}", acc=a.name, accCount=int(rng.choice([1, 2, 4])),
                maxBatchSize=64, atTokens=1024,
                decodeParms=DecodeParms(alpha=float(base[0] * f), beta=float(base[1] * f)),
                prefillParms=PrefillParms(gamma=float(base[2] * f), delta=float(base[3] * f)),
            )
            for a, f in zip(accs, rng.uniform(0.5, 1.0, size=len(accs)))
        ]
    system, _ = System.from_spec(
        make_fleet_spec(3, seed=12, accelerators=accs, perf_profiles=profiles))
    return system


@pytest.mark.parametrize("name,build,n_cells,group", [
    ("one-accelerator", lambda: System.from_spec(
        make_spec(n_servers=6, seed=31, arrival_scale=ARRIVAL_SCALE, n_accelerators=1))[0], 6, 1),
    ("two-accelerators", lambda: System.from_spec(
        make_spec(n_servers=6, seed=32, arrival_scale=ARRIVAL_SCALE, n_accelerators=2))[0], 12, 2),
    ("five-servers", lambda: System.from_spec(
        make_spec(n_servers=5, seed=33, arrival_scale=ARRIVAL_SCALE))[0], 15, 4),
    ("second-wave", lambda: System.from_spec(
        make_spec(n_servers=17, seed=34, arrival_scale=ARRIVAL_SCALE))[0], 51, 4),
    ("strided", wide_fleet, 210, 64),
])
def test_group_shapes(monkeypatch, name, build, n_cells, group):
    monkeypatch.delenv("INFERNO_SIZING_MEMO", raising=False)
    fs, ref = make_pair(build)
    assert fs.n_cells == n_cells
    longest = int(np.diff(fs.seg_start).max())
    assert group == min(64, 1 << (longest - 1).bit_length())  # the kernel's lanes per server
    scales = (1.0, 2.6, 0.0, 0.45)
    res = fs.rollout(scales=scales, return_cells=True)
    rows = tick_loop(ref, res.arrival)
    assert_rollout_equals_loop(res, rows, fs.cur_override[0])
    if name == "second-wave":  # 17 servers: some of them move
        assert res.acc_changes.sum() > 0


# -- chunking -------------------------------------------------------------------
def test_chunked_equals_unchunked(monkeypatch):
    monkeypatch.delenv("INFERNO_SIZING_MEMO", raising=False)
    whole, _, _ = oracle()
    fs, ref = make_pair(oracle_system, oracle_cur)
    monkeypatch.setattr(fastpath, "ROLLOUT_CHUNK", 3)
    before = fs.memo_stats()
    assert before is None
    parts = fs.rollout(arrival=whole.arrival, return_cells=True)
    assert_results_identical(whole, parts)
    # three passes: at most one lookup per cell and pass
    hits, misses = fs.memo_stats()
    assert 0 < hits + misses <= 3 * fs.n_cells

    # a server that is idle throughout the second pass and loaded in the
    # third: its cells take the zero path in one and are sized in the next,
    # so the bucket layout goes stale at the boundary
    scen = whole.arrival.copy()
    scen[3:6, 0] = 0.0
    assert (scen[6] > 0).all() and (scen[:3] > 0).all()
    stale = fs._gpu.stale_ticks
    parts = fs.rollout(arrival=scen, return_cells=True)
    assert fs._gpu.stale_ticks >= stale + 2
    monkeypatch.setattr(fastpath, "ROLLOUT_CHUNK", fastpath.PLAN_MAX_S)
    whole2 = fs.rollout(arrival=scen, return_cells=True)
    assert_results_identical(whole2, parts)
    assert_rollout_equals_loop(parts, tick_loop(ref, scen), fs.cur_override[0])


# -- neighbours -------------------------------------------------------------------
def test_one_step_equals_reconcile(monkeypatch):
    monkeypatch.delenv("INFERNO_SIZING_MEMO", raising=False)
    fs, ref = make_pair(oracle_system, oracle_cur)
    w = ref.reconcile()
    res = fs.rollout(scales=[1.0])
    assert res.cells is None
    assert_winner_equal(slice_winner(res.winners, 0), w, "one step")
    for got, want in zip(res.final_cur, feed_back(ref.cur_override, w)):
        assert got.tobytes() == want.tobytes()


def test_rollout_changes_nothing_around_it(monkeypatch):
    monkeypatch.delenv("INFERNO_SIZING_MEMO", raising=False)
    fs, _ = make_pair(oracle_system, oracle_cur)
    w1 = fs.reconcile()
    p1 = fs.plan(scales=SCALES, return_cells=True)
    s1 = fs.plan_slo(slo_scales=[0.8, 1.0], scales=[1.0, 2.0])
    stats = fs.memo_stats()
    res = fs.rollout(scales=SCALES)
    hits, misses = fs.memo_stats()
    assert 0 < (hits + misses) - sum(stats) <= fs.n_cells  # one pass, one lookup per cell
    assert fs._gpu.fused_state()["done_nonzero"] <= 0
    w2 = fs.reconcile()
    p2 = fs.plan(scales=SCALES, return_cells=True)
    s2 = fs.plan_slo(slo_scales=[0.8, 1.0], scales=[1.0, 2.0])
    assert fs._gpu.fused_state()["done_nonzero"] <= 0
    assert_winner_equal(w1, w2, "reconcile after the rollout")
    assert_winner_equal(p1.winners, p2.winners, "plan after the rollout")
    assert_winner_equal(s1.winners, s2.winners, "plan_slo after the rollout")
    feas = p1.cells["feasible"].astype(bool)
    assert np.array_equal(p1.cells["feasible"], p2.cells["feasible"])
    assert np.array_equal(bits(p1.cells["value"])[feas], bits(p2.cells["value"])[feas])
    # and the rollout is the same before and after them
    again = fs.rollout(scales=SCALES)
    assert_winner_equal(res.winners, again.winners, "second rollout")
    # the overrides are the caller's
    assert fs.cur_override[0][NO_CUR_SRV] == -3


def test_step_limit_launches_nothing(monkeypatch):
    monkeypatch.delenv("INFERNO_SIZING_MEMO", raising=False)
    fs, _ = make_pair(oracle_system, oracle_cur)
    fs.rollout(scales=[1.0])
    stats = fs.memo_stats()
    with pytest.raises(ValueError):
        fs.rollout(scales=[1.0] * 4097)
    with pytest.raises(ValueError):
        fs.rollout(scales=[1.0, -1.0])
    assert fs.memo_stats() == stats
