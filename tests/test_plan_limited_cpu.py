"""Capacity-limited what-if planning on the golden path
(FastSweep.plan(capacity=...), backend="cpu"): scenario s must be what a fresh
system with that scenario's loads gives through SweepEngine(cpu) +
solve_greedy with that scenario's inventory.

Fleet: 24 servers in three priority groups; servers 3, 6 and 9 are exact
copies of server 0 (model, service class, load, current allocation), so equal
ordering keys occur and leftmost re-insertion decides. Two accelerator types
without accelerators are added to system.capacity: one is given 0 units, the
other is left out of the mapping.
"""
import copy
import json
import sys

import numpy as np
import pytest

from inferno_amd import cli
from inferno_amd.config import SaturationPolicy
from inferno_amd.core import System
from inferno_amd.engine import FastSweep, SweepEngine
from inferno_amd.solver.greedy import solve_greedy
from tests.fixtures import make_spec

EXAMPLE = "examples/system.json"
SCALES = (0.0, 0.5, 1.0, 2.0, 4.0)
POLICIES = ("None", "PriorityExhaustive", "PriorityRoundRobin", "RoundRobin")
COPIES = (3, 6, 9)  # copies of server 0; all four are in priority group 0
TYPES = ("AMD-MI300X-192GB", "AMD-MI325X-256GB", "AMD-MI355X-288GB")
EXTRA_ZERO = "AMD-MI250X-128GB"  # no accelerator has it; 0 units in the mapping
EXTRA_MISSING = "AMD-MI210-64GB"  # no accelerator has it; not in the mapping
CAPACITY_SEED = 1665  # 7 / 3 / 2 units: every scale falls out, 4x in every group
ROW_FACTOR = (8, 3, 2, 1, 1)  # array form: scenario s has ROW_FACTOR[s] times the drawn units


def build_fleet(pin_batch=False):
    system, _ = System.from_spec(make_spec(n_servers=24, unlimited=False, priorities=(1, 5, 10)))
    names = sorted(system.servers)
    src = system.servers["srv-0:ns"]
    for i in COPIES:
        srv = system.servers[f"srv-{i}:ns"]
        assert srv.service_class_name == src.service_class_name
        srv.model_name = src.model_name
        srv.load = copy.deepcopy(src.load)
        srv.cur_allocation = copy.deepcopy(src.cur_allocation)
    if pin_batch:
        # GPU tests: batch sizes 16..64 so the sweep costs nothing
        for i, name in enumerate(names):
            system.servers[name].max_batch_size = 16 + (i * 7) % 49
        for i in COPIES:
            system.servers[f"srv-{i}:ns"].max_batch_size = src.max_batch_size
    system.capacity = {EXTRA_ZERO: 7, EXTRA_MISSING: 3}
    return system


def draw_capacity(seed=CAPACITY_SEED):
    """Units per type as tests/test_native_greedy.py draws them, plus the type
    at 0; EXTRA_MISSING stays out of the mapping."""
    rng = np.random.default_rng(seed)
    cap = {t: int(rng.integers(2, 30)) for t in TYPES}
    cap[EXTRA_ZERO] = 0
    return cap


def capacity_rows(fs, cap, n_scen):
    """The [S, n_types] form of a mapping, with rows that differ: scenario s
    has ROW_FACTOR[s] times the mapping's units."""
    types = fs.capacity_types
    rows = np.zeros((n_scen, len(types)), dtype=np.int64)
    for s in range(n_scen):
        for j, t in enumerate(types):
            rows[s, j] = cap.get(t, 0) * ROW_FACTOR[s % len(ROW_FACTOR)]
    return rows


def scenario_rates(system, fs, scales=SCALES):
    base = np.array([system.servers[n].load.arrivalRate for n in fs.server_names],
                    dtype=np.float32)
    return np.stack([base * np.float32(sc) for sc in scales]).astype(np.float32)


def units_per_replica(system, name, acc_name):
    acc = system.accelerators[acc_name]
    return system.models[system.servers[name].model_name].get_num_instances(acc_name) \
        * acc.multiplicity


def golden(scen, cap_rows, types, policy, delayed):
    """Per scenario: fresh system, scenario loads, CPU sweep, Python greedy.
    Returns per scenario {server: allocation or None} and the fall-out
    priorities (servers with a real candidate that got less than desired)."""
    out = []
    for s in range(scen.shape[0]):
        system = build_fleet()
        names = sorted(system.servers)
        for i, n in enumerate(names):
            system.servers[n].load.arrivalRate = float(scen[s, i])
        system.capacity = {t: int(cap_rows[s, j]) for j, t in enumerate(types)}
        SweepEngine(backend="cpu").sweep(system)
        want = {
            n: {k: a.num_replicas for k, a in system.servers[n].all_allocations.items()}
            for n in names
        }
        solve_greedy(system, delayed_best_effort=delayed,
                     saturation_policy=SaturationPolicy.parse(policy))
        fell = set()
        for n in names:
            srv = system.servers[n]
            real = [a for a in srv.all_allocations.values() if a.accelerator != ""]
            short = srv.allocation is None or (
                srv.allocation.num_replicas < want[n][srv.allocation.accelerator])
            if real and short:
                fell.add(srv.priority(system))
        out.append(({n: system.servers[n].allocation for n in names}, fell, system))
    return out


def check_against_golden(res, gold, fs):
    names = fs.server_names
    for s, (allocs, _, _) in enumerate(gold):
        for i, n in enumerate(names):
            a = allocs[n]
            got_acc = int(res.winners.acc_idx[s, i])
            assert (a is None) == (got_acc == -1), (s, n)
            if a is None:
                assert res.winners.num_replicas[s, i] == 0
                continue
            assert fs.acc_names[got_acc] == a.accelerator, (s, n)
            assert int(res.winners.num_replicas[s, i]) == a.num_replicas, (s, n)
            assert float(res.winners.cost[s, i]) == pytest.approx(a.cost, rel=1e-6), (s, n)
            assert float(res.winners.value[s, i]) == pytest.approx(a.value, rel=1e-6), (s, n)


def check_capacity_accounting(res, fs, cap_rows):
    system = fs.system
    types = fs.capacity_types
    assert res.capacity_types == types
    used = np.zeros_like(res.capacity_left)
    for s in range(res.winners.acc_idx.shape[0]):
        for i, n in enumerate(fs.server_names):
            a = int(res.winners.acc_idx[s, i])
            if a < 0:
                continue
            acc_name = fs.acc_names[a]
            used[s, types.index(system.accelerators[acc_name].type)] += (
                int(res.winners.num_replicas[s, i]) * units_per_replica(system, n, acc_name))
    assert (used <= cap_rows).all()
    assert res.capacity_left.dtype == np.int64
    np.testing.assert_array_equal(res.capacity_left, cap_rows - used)


_GOLD = {}


def cached_golden(policy, delayed, rows_differ):
    key = (policy, delayed, rows_differ)
    if key not in _GOLD:
        system = build_fleet()
        fs = FastSweep(system, backend="cpu")
        scen = scenario_rates(system, fs)
        cap = draw_capacity()
        rows = capacity_rows(fs, cap, len(SCALES))
        if not rows_differ:
            rows[:] = rows[0] // ROW_FACTOR[0]  # the mapping itself in every scenario
        _GOLD[key] = (rows, golden(scen, rows, fs.capacity_types, policy, delayed))
    return _GOLD[key]


def test_fallout_precondition():
    """Inputs on which the solvers never run out of capacity show nothing: one
    scenario has no fall-out, one has some, one has it in every priority group."""
    _, gold = cached_golden("None", False, False)
    _, gold_rows = cached_golden("None", False, True)
    n_groups = [len(fell) for _, fell, _ in gold + gold_rows]
    assert 0 in n_groups
    assert any(0 < g < 3 for g in n_groups)
    assert 3 in n_groups


def test_capacity_types():
    fs = FastSweep(build_fleet(), backend="cpu")
    assert fs.capacity_types == sorted(TYPES + (EXTRA_ZERO, EXTRA_MISSING))


@pytest.mark.parametrize("delayed", [False, True])
@pytest.mark.parametrize("policy", POLICIES)
def test_mapping_matches_golden(policy, delayed):
    rows, gold = cached_golden(policy, delayed, False)
    system = build_fleet()
    fs = FastSweep(system, backend="cpu")
    res = fs.plan(scales=SCALES, capacity=draw_capacity(), saturation_policy=policy,
                  delayed_best_effort=delayed)
    check_against_golden(res, gold, fs)
    check_capacity_accounting(res, fs, rows)
    j = fs.capacity_types.index(EXTRA_MISSING)
    assert (res.capacity_left[:, j] == 0).all()  # missing from the mapping counts as 0
    granted, desired = res.winners.num_replicas, res.desired_replicas
    np.testing.assert_array_equal(
        res.partial_servers, ((granted > 0) & (granted < desired)).sum(axis=1))
    for s, (allocs, _, gsys) in enumerate(gold):
        unalloc = sum(
            1 for n in fs.server_names
            if allocs[n] is None and any(
                a.accelerator != "" for a in gsys.servers[n].all_allocations.values())
        )
        assert int(res.unallocated_servers[s]) == unalloc, s


@pytest.mark.parametrize("policy,delayed", [("None", False), ("PriorityRoundRobin", False),
                                            ("RoundRobin", True), ("PriorityExhaustive", True)])
def test_array_form_matches_golden(policy, delayed):
    rows, gold = cached_golden(policy, delayed, True)
    assert (rows[0] != rows[-1]).any()
    system = build_fleet()
    fs = FastSweep(system, backend="cpu")
    res = fs.plan(scales=SCALES, capacity=rows, saturation_policy=policy,
                  delayed_best_effort=delayed)
    check_against_golden(res, gold, fs)
    check_capacity_accounting(res, fs, rows)


def test_fixed_load_varying_inventory():
    """The array form with the same arrival row S times."""
    system = build_fleet()
    fs = FastSweep(system, backend="cpu")
    row = scenario_rates(system, fs, (2.0,))[0]
    scen = np.stack([row] * 3)
    rows = capacity_rows(fs, draw_capacity(), 1)[[0, 0, 0]] // ROW_FACTOR[0] * [[1], [2], [4]]
    res = fs.plan(arrival=scen, capacity=rows, saturation_policy="PriorityExhaustive")
    gold = golden(scen, rows, fs.capacity_types, "PriorityExhaustive", False)
    check_against_golden(res, gold, fs)
    total = res.winners.num_replicas.sum(axis=1)
    assert total[0] <= total[1] <= total[2] and total[0] < total[2]


def test_real_type_at_zero_and_missing():
    system = build_fleet()
    fs = FastSweep(system, backend="cpu")
    res = fs.plan(scales=SCALES, capacity={TYPES[0]: 0, TYPES[2]: 40},
                  saturation_policy="RoundRobin")
    on = res.winners.acc_idx >= 0
    types = np.array([system.accelerators[a].type for a in fs.acc_names])
    assert on.any()
    assert set(types[res.winners.acc_idx[on]]) == {TYPES[2]}


def test_ample_capacity_is_the_unlimited_plan():
    system = build_fleet()
    fs = FastSweep(system, backend="cpu")
    free = fs.plan(scales=SCALES)
    res = fs.plan(scales=SCALES, capacity={t: 10**6 for t in TYPES})
    loaded = free.winners.acc_idx >= 0
    assert loaded.all()  # min_replicas = 1 keeps a replica at scale 0
    np.testing.assert_array_equal(res.winners.acc_idx[loaded], free.winners.acc_idx[loaded])
    np.testing.assert_array_equal(res.winners.num_replicas[loaded],
                                  free.winners.num_replicas[loaded])
    np.testing.assert_array_equal(res.desired_replicas[loaded],
                                  free.winners.num_replicas[loaded])
    assert (res.unallocated_servers == 0).all() and (res.partial_servers == 0).all()
    np.testing.assert_array_equal(res.replicas_by_acc, free.replicas_by_acc)


def test_zero_load_server_is_dropped():
    """A server that may scale to zero has the empty allocation at zero load;
    the greedy drops it, so the limited plan reports -1 where the unlimited
    plan reports -2, and it is not counted as unallocated."""
    system = build_fleet()
    system.servers["srv-1:ns"].min_num_replicas = 0
    fs = FastSweep(system, backend="cpu")
    i = fs.server_names.index("srv-1:ns")
    free = fs.plan(scales=SCALES)
    res = fs.plan(scales=SCALES, capacity={t: 10**6 for t in TYPES})
    assert free.winners.acc_idx[0, i] == -2 and res.winners.acc_idx[0, i] == -1
    assert res.winners.num_replicas[0, i] == 0 and res.desired_replicas[0, i] == 0
    assert (res.winners.acc_idx[1:, i] >= 0).all()
    assert (res.unallocated_servers == 0).all()


def test_without_capacity_nothing_changes():
    fs = FastSweep(build_fleet(), backend="cpu")
    res = fs.plan(scales=SCALES)
    for f in ("desired_replicas", "unallocated_servers", "partial_servers", "capacity_left",
              "capacity_types"):
        assert getattr(res, f) is None


def system_state(system):
    return (
        {n: (None if s.load is None else
             (s.load.arrivalRate, s.load.avgInTokens, s.load.avgOutTokens))
         for n, s in system.servers.items()},
        {n: (id(s.allocation), id(s.all_allocations), dict(s.all_allocations),
             id(s.spec.desiredAlloc)) for n, s in system.servers.items()},
        (id(system.capacity), dict(system.capacity)),
    )


def test_system_is_left_unchanged():
    system = build_fleet()
    SweepEngine(backend="cpu").sweep(system)  # something to lose
    solve_greedy(system)
    before = system_state(system)
    fs = FastSweep(system, backend="cpu")
    fs.plan(scales=SCALES, capacity=draw_capacity(), saturation_policy="RoundRobin")
    assert system_state(system) == before
    with pytest.raises(ValueError):
        fs.plan(scales=SCALES, capacity={"no-such-type": 1})
    assert system_state(system) == before


@pytest.mark.parametrize("bad", [
    {TYPES[0]: -1},
    {TYPES[0]: 2.5},
    {TYPES[0]: float("nan")},
    {TYPES[0]: float("inf")},
    {TYPES[0]: 2**31},
    {TYPES[0]: "many"},
    np.full((len(SCALES), 5), -1),
    np.full((len(SCALES), 5), 0.5),
    np.full((len(SCALES), 5), np.inf),
    np.full((len(SCALES), 5), 2.0**31),
    np.zeros((len(SCALES), 4)),
    np.zeros((len(SCALES) + 1, 5)),
    np.zeros(5),
])
def test_bad_capacity_raises(bad):
    fs = FastSweep(build_fleet(), backend="cpu")
    with pytest.raises(ValueError):
        fs.plan(scales=SCALES, capacity=bad)


def test_int32_max_capacity_is_accepted():
    fs = FastSweep(build_fleet(), backend="cpu")
    res = fs.plan(scales=(1.0,), capacity={TYPES[0]: 2**31 - 1})
    assert res.capacity_left.max() <= 2**31 - 1


def run_cli(monkeypatch, capsys, *argv):
    monkeypatch.setattr(sys, "argv", ["inferno_amd.cli", *argv])
    with pytest.raises(SystemExit) as e:
        cli.main()
    assert e.value.code == 0
    return capsys.readouterr().out


def test_cli_capacity(monkeypatch, capsys):
    system, _ = cli._load_system(EXAMPLE)
    types = FastSweep(system, backend="cpu").capacity_types
    cap = ",".join(f"{t}=3" for t in types)
    doc = json.loads(run_cli(monkeypatch, capsys, "plan", EXAMPLE, "--scales", "0.5,1,4",
                             "--backend", "cpu", "--json", "--capacity", cap,
                             "--saturation-policy", "PriorityExhaustive"))
    assert doc["saturationPolicy"] == "PriorityExhaustive"
    for r in doc["scenarios"]:
        assert {"unallocatedServers", "partialServers", "capacityLeft"} <= set(r)
        assert set(r["capacityLeft"]) == set(types)
        assert all(0 <= v <= 3 for v in r["capacityLeft"].values())
    text = run_cli(monkeypatch, capsys, "plan", EXAMPLE, "--scales", "0.5,1,4",
                   "--backend", "cpu", "--capacity", cap)
    head = text.splitlines()[0]
    assert "unallocated" in head and "partial" in head
    assert all(f"left:{t}" in head for t in types)
    limited = run_cli(monkeypatch, capsys, "plan", EXAMPLE, "--scales", "1", "--backend", "cpu",
                      "--limited")
    assert "unallocated" in limited.splitlines()[0]
    # without the flags the output is the old one
    plain = run_cli(monkeypatch, capsys, "plan", EXAMPLE, "--scales", "0.5,1,4",
                    "--backend", "cpu")
    assert "unallocated" not in plain and "left:" not in plain and "limited" not in plain
    doc = json.loads(run_cli(monkeypatch, capsys, "plan", EXAMPLE, "--scales", "0.5,1,4",
                             "--backend", "cpu", "--json"))
    assert set(doc) == {"backend", "referenceScale", "servers", "scenarios"}
    for r in doc["scenarios"]:
        assert set(r) == {"scale", "totalCost", "replicas", "infeasibleServers",
                          "acceleratorChanges"}
