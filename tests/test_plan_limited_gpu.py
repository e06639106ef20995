"""Capacity-limited planning on the GPU (wva_plan_greedy): every scenario must
be exactly what the host solver (ops/native/greedy.cpp) gives on the device's
OWN per-cell outputs: plan(return_cells=True) on the same FastSweep, each
scenario slice through the shared candidate preparation and run_greedy_native.
Winning cells, granted replicas, capacity left and replica totals are compared
as integers, the fp32 winner records as bits (the oracle applies the same fp64
granted/desired scaling in numpy).

The GPU's limited plan is deliberately not compared with the CPU backend's:
replica counts may differ at ceil boundaries between the two sweeps, and a
greedy amplifies one flip.

Fleets (batch sizes pinned to 16..64 so the sweep costs nothing):
  a  the 24-server fleet of test_plan_limited_cpu.py (fewer servers than lanes)
  b  70 servers = one wave + 6: the strided loops and their remainder
  c  12 servers with segments of 1 and 3 cells, one server with an unreachable
     SLO and one zero-load server that may scale to zero

The kernel keeps its keys in a global-memory workspace, so there is no cap on
the server count and no cap-crossing run.
"""
import numpy as np
import pytest

from inferno_amd.core import System
from inferno_amd.engine import FastSweep
from inferno_amd.engine.fastpath import _POLICY_CODE, greedy_candidates
from tests.fixtures import make_spec
from tests.test_plan_limited_cpu import POLICIES, build_fleet

pytestmark = pytest.mark.gpu

SCALES = (0.0, 0.5, 1.0, 1.5, 2.0, 4.0, 16.0)
WAVE = 64
INFEASIBLE_SRV = 5
ZERO_SRV = 7
WINNER_INT = ("acc_idx", "num_replicas", "batch")
WINNER_FLOAT = ("cost", "value", "itl", "ttft", "rho", "max_rate")


def pin_batches(system):
    for i, name in enumerate(sorted(system.servers)):
        system.servers[name].max_batch_size = 16 + (i * 7) % 49


def fleet_a():
    return build_fleet(pin_batch=True)


def fleet_b():
    system, _ = System.from_spec(
        make_spec(n_servers=WAVE + 6, seed=31, unlimited=False, priorities=(1, 5, 10)))
    pin_batches(system)
    return system


def fleet_c():
    system, _ = System.from_spec(
        make_spec(n_servers=12, seed=32, unlimited=False, priorities=(1, 5, 10)))
    pin_batches(system)
    names = sorted(system.servers)
    for i in (1, 4, 8, 10):  # keep the accelerator: a one-cell segment
        system.servers[names[i]].keep_accelerator = True
    # unreachable SLO, as in test_plan_gpu.py
    srv = system.servers[names[INFEASIBLE_SRV]]
    t = system.service_classes[srv.service_class_name].targets[srv.model_name]
    t.itl = 1e-3
    t.ttft = 0.0
    system.servers[names[ZERO_SRV]].min_num_replicas = 0
    return system


FLEETS = {"a": fleet_a, "b": fleet_b, "c": fleet_c}
_STATE = {}


def planner(kind):
    """One FastSweep per fleet, its scenarios, and the unlimited plan with the
    per-cell outputs the oracle solves on (computed once, never changed)."""
    if kind not in _STATE:
        system = FLEETS[kind]()
        fs = FastSweep(system, backend="gpu")
        base = np.array([system.servers[n].load.arrivalRate for n in fs.server_names],
                        dtype=np.float32)
        scen = np.stack([base * np.float32(sc) for sc in SCALES]).astype(np.float32)
        if kind == "c":
            scen[:, ZERO_SRV] = 0.0
            seg = np.diff(fs.seg_start)
            assert set(seg.tolist()) == {1, 3}
        free = fs.plan(arrival=scen, return_cells=True)
        _STATE[kind] = (fs, scen, free)
    return _STATE[kind]


def units_at(fs, free, s, only_priority=None):
    """Units per capacity type that the unlimited plan of scenario s uses
    (optionally of one priority group only)."""
    types, cell_tidx, units, prio = fs.greedy_static()
    out = np.zeros(len(types), dtype=np.int64)
    acc_tidx = {int(a): int(t) for a, t in zip(fs.cell_acc_idx, cell_tidx)}
    for i in range(len(fs.server_names)):
        a = int(free.winners.acc_idx[s, i])
        if a < 0 or (only_priority is not None and prio[i] != only_priority):
            continue
        cell = [k for k in range(fs.seg_start[i], fs.seg_start[i + 1])
                if fs.cell_acc_idx[k] == a][0]
        out[acc_tidx[a]] += int(free.winners.num_replicas[s, i]) * int(units[cell])
    return out


def mapping_capacity(fs, free):
    """What the unlimited plan wants at 1x: the fleet starts falling out above it."""
    want = units_at(fs, free, SCALES.index(1.0))
    return {t: int(want[j]) for j, t in enumerate(fs.capacity_types)}


def row_capacity(fs, free):
    """[S, n_types] with rows that differ and the three regimes by construction:
    scenario 0 cannot run out, scenario 1 holds exactly what priority group 1
    takes (so the other two groups fall out whole), the last one has one unit
    per type (fewer units than any group has servers); the rest hold the 1x
    demand."""
    n_types = len(fs.capacity_types)
    rows = np.tile(units_at(fs, free, SCALES.index(1.0)), (len(SCALES), 1))
    rows[0] = 10**4
    rows[1] = units_at(fs, free, 1, only_priority=1)
    rows[-1] = 1
    assert rows.shape == (len(SCALES), n_types)
    return rows


def host_oracle(fs, free, rows, policy, delayed):
    from inferno_amd.ops.sweep import run_greedy_native

    cells = free.cells
    n_scen, n_srv = free.arrival.shape
    n_acc = len(fs.acc_names)
    _, cell_tidx, units, prio = fs.greedy_static()
    prio = np.ascontiguousarray(prio, dtype=np.int32)
    out = {
        "cell": np.full((n_scen, n_srv), -1, np.int32),
        "acc_idx": np.full((n_scen, n_srv), -1, np.int32),
        "num_replicas": np.zeros((n_scen, n_srv), np.int32),
        "batch": np.zeros((n_scen, n_srv), np.int32),
        "desired": np.zeros((n_scen, n_srv), np.int32),
        "cap_left": np.ascontiguousarray(rows, dtype=np.int32).copy(),
        "totals": np.zeros((n_scen, n_acc), np.int64),
        "fell": [],
    }
    for f in WINNER_FLOAT:
        out[f] = np.zeros((n_scen, n_srv), np.float32)
    for s in range(n_scen):
        order, seg, c_val, c_type, c_units, c_reps = greedy_candidates(
            cells["feasible"][s], cells["zero_empty"][s], cells["value"][s],
            cells["num_replicas"][s], fs.cell_server, cell_tidx, units, n_srv)
        win, reps = run_greedy_native(c_val, c_type, c_units, c_reps, seg, prio,
                                      out["cap_left"][s], delayed, _POLICY_CODE[policy])
        real = np.zeros(n_srv, dtype=bool)
        real[fs.cell_server[order[c_type >= 0]]] = True
        out["fell"].append({int(prio[i]) for i in range(n_srv) if real[i] and win[i] < 0})
        for i in np.nonzero(win >= 0)[0]:
            cell = int(order[win[i]])
            want, got = int(cells["num_replicas"][s][cell]), int(reps[i])
            out["cell"][s, i] = cell
            out["acc_idx"][s, i] = fs.cell_acc_idx[cell]
            out["num_replicas"][s, i] = got
            out["batch"][s, i] = cells["batch"][s][cell]
            out["desired"][s, i] = want
            for f in WINNER_FLOAT:
                out[f][s, i] = cells[f][s][cell]
            if want > 0 and got != want:
                factor = float(got) / float(want)
                for f in ("cost", "value"):
                    out[f][s, i] = np.float32(float(cells[f][s][cell]) * factor)
            out["totals"][s, fs.cell_acc_idx[cell]] += got
    return out


def assert_same(res, fs, want):
    np.testing.assert_array_equal(fs._plan_limited_cells, want["cell"])
    for f in WINNER_INT:
        np.testing.assert_array_equal(getattr(res.winners, f), want[f], err_msg=f)
    for f in WINNER_FLOAT:
        np.testing.assert_array_equal(getattr(res.winners, f).view(np.uint32),
                                      want[f].view(np.uint32), err_msg=f)
    np.testing.assert_array_equal(res.desired_replicas, want["desired"])
    np.testing.assert_array_equal(res.capacity_left, want["cap_left"].astype(np.int64))
    np.testing.assert_array_equal(res.replicas_by_acc, want["totals"])
    assert (res.capacity_left >= 0).all()


def run_case(kind, capacity, rows, policy, delayed):
    fs, scen, free = planner(kind)
    want = host_oracle(fs, free, rows, policy, delayed)
    res = fs.plan(arrival=scen, capacity=capacity, saturation_policy=policy,
                  delayed_best_effort=delayed)
    assert_same(res, fs, want)
    return res, want


def as_rows(fs, mapping):
    return np.tile(np.array([mapping[t] for t in fs.capacity_types], dtype=np.int64),
                   (len(SCALES), 1))


@pytest.fixture(autouse=True)
def device_path(monkeypatch):
    monkeypatch.setenv("INFERNO_PLAN_GREEDY", "device")


def test_fallout_precondition():
    """No fall-out, some, and fall-out in every priority group all occur."""
    for kind in FLEETS:
        fs, scen, free = planner(kind)
        want = host_oracle(fs, free, row_capacity(fs, free), "None", False)
        n_groups = [len(f) for f in want["fell"]]
        assert n_groups[0] == 0 and n_groups[-1] == 3, (kind, n_groups)
        assert any(0 < g < 3 for g in n_groups), (kind, n_groups)
    fs, scen, free = planner("a")
    want = host_oracle(fs, free, as_rows(fs, mapping_capacity(fs, free)), "None", False)
    assert len(want["fell"][-1]) == 3  # 16x the load the inventory was sized for


@pytest.mark.parametrize("delayed", [False, True])
@pytest.mark.parametrize("policy", POLICIES)
def test_fleet_a_mapping(policy, delayed):
    fs, scen, free = planner("a")
    cap = mapping_capacity(fs, free)
    res, want = run_case("a", cap, as_rows(fs, cap), policy, delayed)
    if policy == "None":
        assert (res.partial_servers == 0).all()
        assert res.unallocated_servers[-1] > 0


@pytest.mark.parametrize("delayed", [False, True])
@pytest.mark.parametrize("policy", POLICIES)
def test_fleet_a_rows(policy, delayed):
    fs, scen, free = planner("a")
    rows = row_capacity(fs, free)
    assert (rows[0] != rows[1]).any() and (rows[1] != rows[-1]).any()
    run_case("a", rows, rows, policy, delayed)


@pytest.mark.parametrize("policy", ["None", "PriorityRoundRobin"])
@pytest.mark.parametrize("kind", ["b", "c"])
def test_fleets_b_c(kind, policy):
    fs, scen, free = planner(kind)
    rows = row_capacity(fs, free)
    res, want = run_case(kind, rows, rows, policy, False)
    cap = mapping_capacity(fs, free)
    run_case(kind, cap, as_rows(fs, cap), policy, True)
    if kind == "c":
        # no feasible candidate: nothing granted, not counted as unallocated;
        # zero load: dropped by the greedy even with capacity to spare
        # (at scale 0 the unreachable SLO does not bind: minimum replicas)
        assert (free.winners.acc_idx[1:, INFEASIBLE_SRV] == -1).all()
        assert (res.winners.acc_idx[1:, INFEASIBLE_SRV] == -1).all()
        assert (res.winners.acc_idx[:, ZERO_SRV] == -1).all()
        assert (free.winners.acc_idx[:, ZERO_SRV] == -2).all()
        assert res.unallocated_servers[0] == 0


def test_host_path_gives_the_same_bytes(monkeypatch):
    fs, scen, free = planner("a")
    rows = row_capacity(fs, free)
    got = {}
    for mode in ("device", "host"):
        monkeypatch.setenv("INFERNO_PLAN_GREEDY", mode)
        res = fs.plan(arrival=scen, capacity=rows, saturation_policy="PriorityRoundRobin")
        got[mode] = (res, fs._plan_limited_cells.copy())
    dev, host = got["device"], got["host"]
    np.testing.assert_array_equal(dev[1], host[1])
    for f in WINNER_INT + WINNER_FLOAT:
        assert getattr(dev[0].winners, f).tobytes() == getattr(host[0].winners, f).tobytes(), f
    for f in ("replicas_by_acc", "cost_total", "infeasible_servers", "desired_replicas",
              "unallocated_servers", "partial_servers", "capacity_left"):
        a, b = getattr(dev[0], f), getattr(host[0], f)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), f


@pytest.mark.parametrize("kind", ["a", "b"])
def test_global_workspace_path_gives_the_same_bytes(kind, monkeypatch):
    """The kernel keeps its hot state in LDS when it fits the budget read at
    context creation; a budget of 0 forces the global-memory workspace, which
    large fleets take, on a small fleet."""
    fs, scen, free = planner(kind)
    rows = row_capacity(fs, free)
    monkeypatch.setenv("INFERNO_PLAN_GREEDY_LDS", "0")
    spilled = FastSweep(FLEETS[kind](), backend="gpu")
    for policy, delayed in (("None", False), ("PriorityRoundRobin", False),
                            ("PriorityExhaustive", True)):
        want = host_oracle(fs, free, rows, policy, delayed)
        res = spilled.plan(arrival=scen, capacity=rows, saturation_policy=policy,
                           delayed_best_effort=delayed)
        assert_same(res, spilled, want)


def test_limited_pass_leaves_no_state_behind():
    """Limited plan, then plan() without capacity, then reconcile(): what those
    calls return on a context that never planned with capacity."""
    used = FastSweep(fleet_a(), backend="gpu")
    clean = FastSweep(fleet_a(), backend="gpu")
    _, scen, free = planner("a")
    rows = row_capacity(used, free)
    used.plan(arrival=scen, capacity=rows, saturation_policy="RoundRobin")
    a, b = used.plan(arrival=scen), clean.plan(arrival=scen)
    for f in WINNER_INT + WINNER_FLOAT:
        assert getattr(a.winners, f).tobytes() == getattr(b.winners, f).tobytes(), f
    assert a.replicas_by_acc.tobytes() == b.replicas_by_acc.tobytes()
    assert a.capacity_left is None and a.desired_replicas is None
    ra, rb = used.reconcile(), clean.reconcile()
    for f in WINNER_INT + WINNER_FLOAT:
        assert getattr(ra, f).tobytes() == getattr(rb, f).tobytes(), f


def test_arenas_grow_recarve_and_reuse():
    """One context through limited S=2, limited S=5, unlimited S=7, limited S=2
    and a reconcile: the planning arena grows twice, the greedy workspace once,
    both are carved anew and then used below their capacity. Every call must
    give, byte for byte, what it gives on a FastSweep that never did anything
    else."""
    _, scen, free = planner("a")
    used = FastSweep(fleet_a(), backend="gpu")
    assert used.n_cells >= 24 and scen.shape[0] == 7
    rows = row_capacity(used, free)

    def limited(fs, sl):
        res = fs.plan(arrival=scen[sl], capacity=rows[sl], saturation_policy="PriorityRoundRobin")
        return res, fs._plan_limited_cells.copy()

    def same_winners(a, b, what):
        for f in WINNER_INT + WINNER_FLOAT:
            x, y = getattr(a, f), getattr(b, f)
            assert x.dtype == y.dtype and x.shape == y.shape, (what, f)
            assert x.tobytes() == y.tobytes(), (what, f)

    def same_arrays(a, b, what):
        assert a.dtype == b.dtype and a.shape == b.shape, what
        assert a.tobytes() == b.tobytes(), what

    steps = [("limited S=2", slice(0, 2)), ("limited S=5", slice(0, 5)), ("unlimited S=7", None),
             ("limited S=2 again", slice(5, 7))]
    for what, sl in steps:
        fresh = FastSweep(fleet_a(), backend="gpu")
        if sl is None:
            a, b = used.plan(arrival=scen), fresh.plan(arrival=scen)
            assert a.capacity_left is None and a.desired_replicas is None
        else:
            (a, a_cells), (b, b_cells) = limited(used, sl), limited(fresh, sl)
            same_arrays(a_cells, b_cells, what)
            assert a.winners.acc_idx.shape == (sl.stop - sl.start, len(used.server_names))
            for f in ("desired_replicas", "capacity_left"):
                same_arrays(getattr(a, f), getattr(b, f), (what, f))
        same_winners(a.winners, b.winners, what)
        same_arrays(a.replicas_by_acc, b.replicas_by_acc, what)
    same_winners(used.reconcile(), FastSweep(fleet_a(), backend="gpu").reconcile(), "reconcile")
