"""Forecast rollout on the CPU backend: FastSweep.rollout against a
hand-written loop of golden reconciles with the desired allocation fed back as
the current one, the derived arrays, input validation and `plan --rollout`."""
import copy
import dataclasses
import json
import os
import sys

import numpy as np
import pytest

from inferno_amd import cli
from inferno_amd.core import System
from inferno_amd.core.allocation import Allocation
from inferno_amd.engine import ROLLOUT_MAX_STEPS, FastSweep, RolloutResult, feed_back
from tests.fixtures import make_spec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = os.path.join(REPO, "examples", "system.json")
# rises, falls, a zero row, comes back
SCALES = (1.0, 3.0, 0.3, 0.0, 2.0, 0.6, 1.0)
SCALE_TO_ZERO_SRV = 1
FIELDS = ("acc_idx", "num_replicas", "batch", "cost", "value", "itl", "ttft", "rho", "max_rate")


def build_system():
    system, _ = System.from_spec(make_spec(n_servers=6, seed=5, arrival_scale=600.0))
    system.servers[sorted(system.servers)[SCALE_TO_ZERO_SRV]].min_num_replicas = 0
    return system


def object_state(system):
    return [
        (n, s.load.arrivalRate, s.load.avgInTokens, s.load.avgOutTokens, id(s.cur_allocation),
         dataclasses.astuple(s.cur_allocation), id(s.allocation))
        for n, s in sorted(system.servers.items())
    ]


def scenarios(system):
    base = np.array([system.servers[n].load.arrivalRate for n in sorted(system.servers)],
                    dtype=np.float32)
    return np.stack([base * np.float32(sc) for sc in SCALES]).astype(np.float32)


def golden_loop(system, scen):
    """One golden reconcile per step on a private copy of the system; the
    winner becomes the server's current allocation before the next step."""
    twin = copy.deepcopy(system)
    fs = FastSweep(twin, backend="cpu")
    names = fs.server_names
    cur = fs._base_cur()
    rows, curs = [], []
    for s in range(scen.shape[0]):
        for i, name in enumerate(names):
            twin.servers[name].load.arrivalRate = float(scen[s, i])
        w = fs._reconcile_cpu()
        rows.append(w)
        cur = feed_back(cur, w)
        curs.append(cur)
        for i, name in enumerate(names):
            if w.acc_idx[i] == -1:
                continue
            twin.servers[name].cur_allocation = Allocation(
                accelerator="" if w.acc_idx[i] == -2 else fs.acc_names[w.acc_idx[i]],
                num_replicas=int(w.num_replicas[i]), cost=float(w.cost[i]))
    return rows, curs


@pytest.fixture(scope="module")
def rolled():
    system = build_system()
    before = object_state(system)
    fs = FastSweep(system, backend="cpu")
    res = fs.rollout(scales=SCALES)
    scen = scenarios(system)
    rows, curs = golden_loop(system, scen)
    return system, before, fs, res, scen, rows, curs


def test_rollout_equals_golden_loop(rolled):
    system, before, fs, res, scen, rows, _ = rolled
    assert isinstance(res, RolloutResult)
    assert np.array_equal(res.arrival, scen)
    assert {f.name for f in dataclasses.fields(res.winners)} == set(FIELDS)
    for f in FIELDS:
        got = getattr(res.winners, f)
        assert got.shape == (len(SCALES), len(fs.server_names))
        for s, row in enumerate(rows):
            want = getattr(row, f)
            assert got.dtype == want.dtype
            assert np.array_equal(got[s], want), f"step {s}: {f} differs"
    assert res.cells is None  # per-cell arrays are a GPU-backend extra
    # the server objects are as they were: loads, current and desired allocations
    assert object_state(system) == before


def test_fixture_goes_empty_and_comes_back(rolled):
    _, _, _, res, _, _, _ = rolled
    zero = SCALES.index(0.0)
    acc = res.winners.acc_idx
    assert acc[zero, SCALE_TO_ZERO_SRV] == -2
    assert acc[zero + 1, SCALE_TO_ZERO_SRV] >= 0
    # coming back from empty is a switch from the empty allocation at cost 0:
    # 0.1 * (0 + cost) + (cost - 0)
    cost = np.float64(res.winners.cost[zero + 1, SCALE_TO_ZERO_SRV])
    assert res.winners.value[zero + 1, SCALE_TO_ZERO_SRV] == pytest.approx(1.1 * cost, rel=1e-6)


def test_hysteresis_bites(rolled):
    """The rollout is not plan(): somewhere the allocation left behind by the
    step before makes another accelerator win than against the initial one."""
    _, _, fs, res, _, _, _ = rolled
    plan = fs.plan(scales=SCALES)
    assert np.array_equal(res.winners.acc_idx[0], plan.winners.acc_idx[0])
    differs = res.winners.acc_idx[1:] != plan.winners.acc_idx[1:]
    print(f"(step, server) pairs whose accelerator differs from plan(): {int(differs.sum())}")
    assert differs.any()
    # and where the accelerator is the same the value need not be
    assert (res.winners.value[1:] != plan.winners.value[1:]).any()


def test_one_step_equals_reconcile():
    system = build_system()
    for srv in system.servers.values():  # the rates a plan row carries are float32
        srv.load.arrivalRate = float(np.float32(srv.load.arrivalRate))
    fs = FastSweep(system, backend="cpu")
    w = fs.reconcile()
    res = fs.rollout(scales=[1.0])
    for f in FIELDS:
        assert np.array_equal(getattr(res.winners, f)[0], getattr(w, f)), f


def test_final_cur_and_acc_changes(rolled):
    _, _, fs, res, _, rows, curs = rolled
    for got, want in zip(res.final_cur, curs[-1]):
        assert got.dtype == want.dtype
        assert np.array_equal(got, want)
    assert res.acc_changes.dtype == np.int64 and res.acc_changes.shape == (len(SCALES),)
    before = fs._base_cur()[0]
    for s, cur in enumerate(curs):
        assert res.acc_changes[s] == int((cur[0] != before).sum()), f"step {s}"
        before = cur[0]
    assert res.acc_changes.sum() > 0
    # a server without current allocation counts when it gets one
    system = build_system()
    names = sorted(system.servers)
    system.servers[names[0]].cur_allocation = None
    fs0 = FastSweep(system, backend="cpu")
    start = fs0._base_cur()[0]
    assert start[0] == -3
    one = fs0.rollout(scales=[1.0, 1.0])
    assert one.winners.acc_idx[0, 0] >= 0
    others = int((np.where(one.winners.acc_idx[0] == -2, -1, one.winners.acc_idx[0])[1:]
                  != start[1:]).sum())
    assert (one.winners.acc_idx[0] != -1).all()
    assert one.acc_changes[0] == others + 1
    assert system.servers[names[0]].cur_allocation is None


def test_totals_recomputed_from_winners(rolled):
    _, _, fs, res, _, _, _ = rolled
    w = res.winners
    n_acc = len(fs.acc_names)
    assert res.replicas_by_acc.dtype == np.int64
    assert res.replicas_by_acc.shape == (len(SCALES), n_acc)
    assert res.cost_total.dtype == np.float64
    for s in range(len(SCALES)):
        want = np.zeros(n_acc, dtype=np.int64)
        total = np.float64(0.0)
        for i in range(len(fs.server_names)):
            if w.acc_idx[s, i] >= 0:
                want[w.acc_idx[s, i]] += int(w.num_replicas[s, i])
            if w.acc_idx[s, i] != -1:
                total += np.float64(w.cost[s, i])
        assert np.array_equal(res.replicas_by_acc[s], want)
        assert res.cost_total[s] == total
        assert res.infeasible_servers[s] == int((w.acc_idx[s] == -1).sum())


def test_current_allocation_override_is_the_start(rolled):
    """Step 0 runs against cur_override when it is set; the objects come back."""
    system = build_system()
    before = object_state(system)
    fs = FastSweep(system, backend="cpu")
    n = len(fs.server_names)
    fs.cur_override = (np.full(n, -3, dtype=np.int32), np.zeros(n, dtype=np.int32),
                       np.zeros(n, dtype=np.float32))
    res = fs.rollout(scales=SCALES[:2])
    # no current allocation: the value of step 0 is the plain cost
    assert np.array_equal(res.winners.value[0], res.winners.cost[0])
    assert res.acc_changes[0] == n
    assert object_state(system) == before


def test_system_restored_on_exception(monkeypatch):
    system = build_system()
    before = object_state(system)
    fs = FastSweep(system, backend="cpu")
    calls = []

    def boom():
        calls.append(1)
        if len(calls) == 3:
            raise RuntimeError("boom")
        return FastSweep._reconcile_cpu(fs)

    monkeypatch.setattr(fs, "_reconcile_cpu", boom)
    with pytest.raises(RuntimeError):
        fs.rollout(scales=SCALES)
    assert object_state(system) == before


@pytest.mark.parametrize(
    "kwargs",
    [
        {},  # neither
        {"scales": [1.0], "arrival": np.ones((1, 6), dtype=np.float32)},  # both
        {"scales": []},  # S = 0
        {"scales": [1.0] * (ROLLOUT_MAX_STEPS + 1)},  # too many steps
        {"scales": [[1.0, 2.0]]},  # not 1-D
        {"scales": [1.0, float("nan")]},
        {"scales": [float("inf")]},
        {"scales": [1.0, -0.5]},
        {"arrival": np.ones(6, dtype=np.float32)},  # 1-D
        {"arrival": np.ones((2, 5), dtype=np.float32)},  # wrong server count
        {"arrival": np.ones((0, 6), dtype=np.float32)},  # S = 0
        {"arrival": np.ones((ROLLOUT_MAX_STEPS + 1, 6), dtype=np.float32)},
        {"arrival": np.full((1, 6), np.nan, dtype=np.float32)},
        {"arrival": np.full((1, 6), np.inf, dtype=np.float32)},
        {"arrival": np.full((1, 6), -1.0, dtype=np.float32)},
    ],
)
def test_bad_input_raises_value_error(kwargs):
    system = build_system()
    before = object_state(system)
    fs = FastSweep(system, backend="cpu")
    with pytest.raises(ValueError):
        fs.rollout(**kwargs)
    assert object_state(system) == before


def test_step_limit():
    assert ROLLOUT_MAX_STEPS == 4096
    fs = FastSweep(build_system(), backend="cpu")
    with pytest.raises(ValueError, match=r"rollout\(\) takes 1\.\.4096 steps, got 4097"):
        fs.rollout(scales=[1.0] * 4097)
    # more steps than one planning pass holds scenarios are fine
    with pytest.raises(ValueError, match=r"plan\(\) takes 1\.\.256 scenarios, got 257"):
        fs.plan(scales=[1.0] * 257)


def run_cli(monkeypatch, capsys, *argv, code=0):
    monkeypatch.setattr(sys, "argv", ["inferno_amd.cli", *argv])
    with pytest.raises(SystemExit) as e:
        cli.main()
    assert e.value.code == code
    return capsys.readouterr().out


def test_cli_plan_rollout(monkeypatch, capsys):
    scales = [0.5, 1.0, 2.0, 1.0, 0.5]
    out = run_cli(monkeypatch, capsys, "plan", EXAMPLE, "--rollout", "--scales",
                  "0.5,1,2,1,0.5", "--backend", "cpu", "--json")
    doc = json.loads(out)
    rows = doc["rollout"]
    assert [r["scale"] for r in rows] == scales
    assert [r["step"] for r in rows] == list(range(5))
    for r in rows:
        assert set(r) == {"step", "scale", "totalCost", "replicas", "infeasibleServers",
                          "acceleratorChanges"}
    assert doc["acceleratorChangesTotal"] == sum(r["acceleratorChanges"] for r in rows)
    # the document is the API's result
    system, _ = cli._load_system(EXAMPLE)
    fs = FastSweep(system, backend="cpu")
    res = fs.rollout(scales=scales)
    assert doc["servers"] == len(fs.server_names)
    for s, r in enumerate(rows):
        assert r["acceleratorChanges"] == int(res.acc_changes[s])
        assert r["infeasibleServers"] == int(res.infeasible_servers[s])
        assert r["totalCost"] == round(float(res.cost_total[s]), 2)
        assert r["replicas"] == {n: int(res.replicas_by_acc[s, j])
                                 for j, n in enumerate(fs.acc_names)}
    # the table form prints one line per step
    text = run_cli(monkeypatch, capsys, "plan", EXAMPLE, "--rollout", "--scales",
                   "0.5,1,2,1,0.5", "--backend", "cpu")
    lines = [ln.split() for ln in text.splitlines()]
    assert [ln[0] for ln in lines if ln and ln[0].isdigit()] == ["0", "1", "2", "3", "4"]
    # it does not combine with the other planning modes
    for extra in (["--slo-scales", "1,2"], ["--limited"], ["--capacity", "X=1"]):
        monkeypatch.setattr(sys, "argv", ["inferno_amd.cli", "plan", EXAMPLE, "--rollout",
                                          "--scales", "1,2", "--backend", "cpu", *extra])
        with pytest.raises(SystemExit) as e:
            cli.main()
        assert e.value.code not in (0, None)
