"""What-if load planning on the CPU backend: FastSweep.plan against a
hand-written loop over the golden reconcile, the derived totals, input
validation and the `plan` subcommand."""
import collections
import copy
import dataclasses
import json
import os
import sys

import numpy as np
import pytest

from inferno_amd import cli
from inferno_amd.core import System
from inferno_amd.engine import FastSweep, PlanResult
from tests.fixtures import make_spec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = os.path.join(REPO, "examples", "system.json")
SCALES = (1.0, 0.0, 0.37, 2.3)
FIELDS = ("acc_idx", "num_replicas", "batch", "cost", "value", "itl", "ttft", "rho", "max_rate")


def build_system():
    system, _ = System.from_spec(make_spec(n_servers=6, seed=11, arrival_scale=600.0))
    return system


def load_state(system):
    return [
        (n, s.load.arrivalRate, s.load.avgInTokens, s.load.avgOutTokens)
        for n, s in sorted(system.servers.items())
    ]


def base_arrival(system):
    return np.array(
        [system.servers[n].load.arrivalRate for n in sorted(system.servers)], dtype=np.float32
    )


def golden_loop(system, scen):
    """One golden reconcile per scenario on a private copy of the system."""
    rows = []
    for s in range(scen.shape[0]):
        twin = copy.deepcopy(system)
        for i, name in enumerate(sorted(twin.servers)):
            twin.servers[name].load.arrivalRate = float(scen[s, i])
        rows.append(FastSweep(twin, backend="cpu").reconcile())
    return rows


@pytest.fixture(scope="module")
def planned():
    system = build_system()
    before = load_state(system)
    fs = FastSweep(system, backend="cpu")
    res = fs.plan(scales=SCALES)
    return system, before, fs, res


def test_plan_equals_golden_loop(planned):
    system, before, fs, res = planned
    assert isinstance(res, PlanResult)
    base = base_arrival(system)
    scen = np.stack([base * np.float32(sc) for sc in SCALES]).astype(np.float32)
    assert np.array_equal(res.arrival, scen)
    rows = golden_loop(system, scen)
    assert {f.name for f in dataclasses.fields(res.winners)} == set(FIELDS)
    for f in FIELDS:
        got = getattr(res.winners, f)
        assert got.shape == (len(SCALES), len(fs.server_names))
        for s, row in enumerate(rows):
            want = getattr(row, f)
            assert got.dtype == want.dtype
            assert np.array_equal(got[s], want), f"scenario {s}: {f} differs"
    # the fixture moves: replica counts change with the load, and the
    # zero-load scenario is really the zero path
    assert (res.winners.num_replicas[3] > res.winners.num_replicas[0]).any()
    assert (res.winners.rho[1] == 0).all()
    # the caller's system is untouched
    assert load_state(system) == before


def test_system_restored_on_exception(monkeypatch):
    system = build_system()
    before = load_state(system)
    fs = FastSweep(system, backend="cpu")
    calls = []

    def boom():
        calls.append(1)
        if len(calls) == 2:
            raise RuntimeError("boom")
        return FastSweep._reconcile_cpu(fs)

    monkeypatch.setattr(fs, "_reconcile_cpu", boom)
    with pytest.raises(RuntimeError):
        fs.plan(scales=SCALES)
    assert load_state(system) == before


def test_totals_recomputed_from_winners(planned):
    _, _, fs, res = planned
    w = res.winners
    n_scen = len(SCALES)
    n_acc = len(fs.acc_names)
    assert res.replicas_by_acc.dtype == np.int64
    assert res.replicas_by_acc.shape == (n_scen, n_acc)
    assert res.cost_total.dtype == np.float64 and res.cost_total.shape == (n_scen,)
    assert res.infeasible_servers.shape == (n_scen,)
    for s in range(n_scen):
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
    assert res.replicas_by_acc.sum() > 0
    assert res.cells is None  # per-cell arrays are a GPU-backend extra


def test_explicit_arrival_equals_scales(planned):
    system, _, fs, res = planned
    base = base_arrival(system)
    scen = np.stack([base * np.float32(sc) for sc in SCALES])
    res2 = fs.plan(arrival=scen)
    for f in FIELDS:
        assert np.array_equal(getattr(res.winners, f), getattr(res2.winners, f)), f
    assert np.array_equal(res.replicas_by_acc, res2.replicas_by_acc)
    assert np.array_equal(res.cost_total, res2.cost_total)
    assert np.array_equal(res.infeasible_servers, res2.infeasible_servers)


@pytest.mark.parametrize(
    "kwargs",
    [
        {},  # neither
        {"scales": [1.0], "arrival": np.ones((1, 6), dtype=np.float32)},  # both
        {"scales": []},  # S = 0
        {"scales": [1.0] * 257},  # S > 256
        {"scales": [[1.0, 2.0]]},  # not 1-D
        {"scales": [1.0, float("nan")]},
        {"scales": [float("inf")]},
        {"scales": [1.0, -0.5]},
        {"arrival": np.ones(6, dtype=np.float32)},  # 1-D
        {"arrival": np.ones((2, 5), dtype=np.float32)},  # wrong server count
        {"arrival": np.ones((0, 6), dtype=np.float32)},  # S = 0
        {"arrival": np.ones((257, 6), dtype=np.float32)},  # S > 256
        {"arrival": np.full((1, 6), np.nan, dtype=np.float32)},
        {"arrival": np.full((1, 6), np.inf, dtype=np.float32)},
        {"arrival": np.full((1, 6), -1.0, dtype=np.float32)},
    ],
)
def test_bad_input_raises_value_error(kwargs):
    system = build_system()
    before = load_state(system)
    fs = FastSweep(system, backend="cpu")
    with pytest.raises(ValueError):
        fs.plan(**kwargs)
    assert load_state(system) == before


def run_cli(monkeypatch, capsys, *argv):
    monkeypatch.setattr(sys, "argv", ["inferno_amd.cli", *argv])
    with pytest.raises(SystemExit) as e:
        cli.main()
    assert e.value.code == 0
    return capsys.readouterr().out


def test_cli_plan(monkeypatch, capsys):
    out = run_cli(monkeypatch, capsys, "plan", EXAMPLE, "--scales", "0.5,1,2",
                  "--backend", "cpu", "--json")
    doc = json.loads(out)
    rows = doc["scenarios"]
    assert [r["scale"] for r in rows] == [0.5, 1.0, 2.0]
    assert doc["referenceScale"] == 1.0
    for r in rows:
        assert set(r) == {"scale", "totalCost", "replicas", "infeasibleServers",
                          "acceleratorChanges"}
    assert rows[1]["acceleratorChanges"] == 0
    solved = json.loads(run_cli(monkeypatch, capsys, "solve", EXAMPLE, "--backend", "cpu",
                                "--json"))
    want = collections.Counter()
    cost = 0.0
    for d in solved["allocations"].values():
        if d["accelerator"]:
            want[d["accelerator"]] += d["numReplicas"]
        cost += d["cost"]
    got = {k: v for k, v in rows[1]["replicas"].items() if v}
    assert got == dict(want)
    assert rows[1]["totalCost"] == pytest.approx(cost, abs=0.01 * len(solved["allocations"]))
    # more load never needs fewer replicas in total
    tot = [sum(r["replicas"].values()) for r in rows]
    assert tot[0] <= tot[1] <= tot[2]
    # the table form prints one line per scale
    text = run_cli(monkeypatch, capsys, "plan", EXAMPLE, "--scales", "0.5,1,2",
                   "--backend", "cpu")
    assert len([ln for ln in text.splitlines() if ln.strip().startswith(("0.5", "1 ", "2 "))]) == 3
