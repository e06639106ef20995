"""What-if SLO planning on the CPU backend: FastSweep.plan_slo against
reconciles of systems rebuilt with the scaled targets, the facts of the fixture
(which cells a four times tighter SLO makes infeasible, replicas growing as the
targets tighten), equality with plan() at SLO scale 1, restoring the system,
input validation and `plan --slo-scales`.

The fleet is the one of tests/test_plan_gpu.py (9 servers x 3 accelerators)."""
import json
import os
import sys

import numpy as np
import pytest

from inferno_amd import cli
from inferno_amd.core import create_allocation
from inferno_amd.engine import FastSweep, SloPlanResult
from tests.test_plan_gpu import INFEASIBLE_SRV, SCALE_TO_ZERO_SRV, build_system

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = os.path.join(REPO, "examples", "system.json")
SLO_SCALES = (1.0, 0.25, 0.5, 2.0)
LOAD_SCALES = (1.0, 0.0, 1.7)
FIELDS = ("acc_idx", "num_replicas", "batch", "cost", "value", "itl", "ttft", "rho", "max_rate")
# replicas per accelerator at load 1.0 (None = infeasible), per SLO scale
REPLICAS = {
    1.0: {0: (19357, 2089, 4437), 3: (46, 45, 40), 4: (37, 25, 37), 6: (52, 51, 46),
          8: (21, 45, 6)},
    0.25: {0: (65609, 5209, 12612), 3: (None, 95, None), 4: (None, None, 109),
           6: (128, 1318, 55), 8: (52, None, 22)},
    0.5: {0: (34669, 3125, 7147), 3: (70, 54, 62), 4: (76, 40, 47), 6: (64, 74, 49),
          8: (31, 71, 8)},
    2.0: {0: (11737, 1545, 3070), 3: (34, 41, 35), 4: (29, 22, 33), 6: (46, 45, 45),
          8: (16, 37, 6)},
}


def targets_of(system):
    out = []
    for name in sorted(system.servers):
        srv = system.servers[name]
        out.append(system.service_classes[srv.service_class_name].targets[srv.model_name])
    return out


def system_state(system):
    return (
        [(t.ttft, t.itl, t.tps) for t in targets_of(system)],
        [(s.load.arrivalRate, s.load.avgInTokens, s.load.avgOutTokens, s.allocation,
          s.cur_allocation) for _, s in sorted(system.servers.items())],
    )


def rebuilt(slo_scale, load_scale):
    """An identical system with the scaled targets and loads written to it."""
    system = build_system()
    for t in targets_of(system):
        t.ttft = float(np.float32(t.ttft) * np.float32(slo_scale))
        t.itl = float(np.float32(t.itl) * np.float32(slo_scale))
    for _, srv in sorted(system.servers.items()):
        srv.load.arrivalRate = float(np.float32(srv.load.arrivalRate) * np.float32(load_scale))
    return system


@pytest.fixture(scope="module")
def planned():
    system = build_system()
    before = system_state(system)
    fs = FastSweep(system, backend="cpu")
    res = fs.plan_slo(slo_scales=SLO_SCALES, scales=LOAD_SCALES)
    return system, before, fs, res


def test_plan_slo_equals_rebuilt_reconciles(planned):
    system, before, fs, res = planned
    assert isinstance(res, SloPlanResult)
    n_t, n_s, n_srv = len(SLO_SCALES), len(LOAD_SCALES), len(fs.server_names)
    assert res.arrival.shape == (n_s, n_srv) and res.arrival.dtype == np.float32
    assert res.t_ttft.shape == res.t_itl.shape == (n_t, n_srv)
    assert res.t_ttft.dtype == res.t_itl.dtype == np.float32
    assert res.cells is None
    for t, slo in enumerate(SLO_SCALES):
        for s, load in enumerate(LOAD_SCALES):
            twin = rebuilt(slo, load)
            assert [x.ttft for x in targets_of(twin)] == [float(v) for v in res.t_ttft[t]]
            assert [x.itl for x in targets_of(twin)] == [float(v) for v in res.t_itl[t]]
            want = FastSweep(twin, backend="cpu").reconcile()
            for f in FIELDS:
                got = getattr(res.winners, f)
                assert got.shape == (n_t, n_s, n_srv)
                assert got.dtype == getattr(want, f).dtype
                assert np.array_equal(got[t, s], getattr(want, f)), f"slice ({t}, {s}): {f}"
            w_acc, w_rep = res.winners.acc_idx[t, s], res.winners.num_replicas[t, s]
            tot = np.zeros(len(fs.acc_names), dtype=np.int64)
            np.add.at(tot, w_acc[w_acc >= 0], w_rep[w_acc >= 0].astype(np.int64))
            assert np.array_equal(res.replicas_by_acc[t, s], tot)
            has = w_acc != -1
            assert res.cost_total[t, s] == res.winners.cost[t, s][has].astype(np.float64).sum()
            assert res.infeasible_servers[t, s] == int((~has).sum())
    assert res.replicas_by_acc.dtype == np.int64 and res.cost_total.dtype == np.float64
    assert res.cost_total.shape == res.infeasible_servers.shape == (n_t, n_s)
    # a zero base target stays zero, the TPS target is not scaled
    assert (res.t_ttft[:, INFEASIBLE_SRV] == 0).all() and (res.t_itl[:, 0] == 0).all()
    zero = LOAD_SCALES.index(0.0)
    assert (res.winners.acc_idx[:, zero, SCALE_TO_ZERO_SRV] == -2).all()
    assert (res.winners.acc_idx[:, :, INFEASIBLE_SRV][:, [0, 2]] == -1).all()
    assert system_state(system) == before  # the caller's system is untouched


def test_fixture_facts():
    """The table of the SLO-planning fixture: replicas per (server,
    accelerator) at load 1.0 under each SLO scale."""
    for slo, table in REPLICAS.items():
        system = rebuilt(slo, 1.0)
        names = sorted(system.servers)
        for srv, want in table.items():
            got = []
            for acc in sorted(system.accelerators):
                alloc = create_allocation(system, names[srv], acc)
                got.append(None if alloc is None else alloc.num_replicas)
            assert tuple(got) == want, f"SLO scale {slo}, server {srv}"
    # replicas grow on every accelerator as the targets tighten
    order = (2.0, 1.0, 0.5, 0.25)
    for srv in (0, 3, 6, 8):
        for a in range(3):
            col = [REPLICAS[slo][srv][a] for slo in order]
            col = [c for c in col if c is not None]
            assert col == sorted(col) and col[0] < col[-1], (srv, a)
    # 0.25 makes single cells infeasible while their server keeps a candidate
    for srv in (3, 4, 8):
        row = REPLICAS[0.25][srv]
        assert None in row and any(c is not None for c in row)


def test_slo_scale_one_equals_plan(planned):
    _, _, fs, _ = planned
    a = fs.plan_slo(slo_scales=[1.0], scales=LOAD_SCALES)
    b = fs.plan(scales=LOAD_SCALES)
    for f in FIELDS:
        assert np.array_equal(getattr(a.winners, f)[0], getattr(b.winners, f)), f
    assert np.array_equal(a.replicas_by_acc[0], b.replicas_by_acc)
    assert np.array_equal(a.cost_total[0], b.cost_total)
    assert np.array_equal(a.infeasible_servers[0], b.infeasible_servers)
    assert np.array_equal(a.arrival, b.arrival)
    # without a load axis: the base load alone
    c = fs.plan_slo(slo_scales=[1.0])
    assert c.winners.acc_idx.shape == (1, 1, len(fs.server_names))
    for f in FIELDS:
        assert np.array_equal(getattr(c.winners, f)[0, 0], getattr(b.winners, f)[0]), f


def test_explicit_targets_equal_scales(planned):
    _, _, fs, res = planned
    again = fs.plan_slo(targets=(res.t_ttft, res.t_itl), arrival=res.arrival)
    for f in FIELDS:
        assert np.array_equal(getattr(again.winners, f), getattr(res.winners, f)), f
    assert np.array_equal(again.cost_total, res.cost_total)


def test_system_restored_on_exception(monkeypatch):
    system = build_system()
    before = system_state(system)
    fs = FastSweep(system, backend="cpu")
    calls = []

    def boom():
        calls.append(1)
        if len(calls) == 5:  # second target set, second load
            raise RuntimeError("boom")
        return FastSweep._reconcile_cpu(fs)

    monkeypatch.setattr(fs, "_reconcile_cpu", boom)
    with pytest.raises(RuntimeError):
        fs.plan_slo(slo_scales=SLO_SCALES, scales=LOAD_SCALES)
    assert len(calls) == 5
    assert system_state(system) == before


def _ones(t, n=9):
    return np.ones((t, n), dtype=np.float32)


@pytest.mark.parametrize(
    "kwargs",
    [
        {},  # neither target argument
        {"slo_scales": [1.0], "targets": (_ones(1), _ones(1))},  # both
        {"slo_scales": []},  # T = 0
        {"slo_scales": [1.0] * 257},  # T * S = 257
        {"slo_scales": [1.0] * 129, "scales": [1.0, 2.0]},  # T * S = 258
        {"slo_scales": [1.0, 0.0]},
        {"slo_scales": [1.0, -0.5]},
        {"slo_scales": [1.0, float("nan")]},
        {"slo_scales": [float("inf")]},
        {"slo_scales": [[1.0, 2.0]]},  # not 1-D
        {"slo_scales": [1.0], "scales": [1.0], "arrival": _ones(1)},  # both load arguments
        {"slo_scales": [1.0], "scales": [-1.0]},
        {"targets": (_ones(2), _ones(3))},  # shapes differ
        {"targets": (_ones(2, 8), _ones(2, 8))},  # wrong server count
        {"targets": (np.ones(9, dtype=np.float32), np.ones(9, dtype=np.float32))},  # 1-D
        {"targets": (_ones(0), _ones(0))},  # T = 0
        {"targets": (_ones(2), -_ones(2))},
        {"targets": (_ones(2) * np.nan, _ones(2))},
        {"targets": (np.full((2, 9), 1e39), _ones(2))},  # overflows float32
        {"targets": _ones(2)},  # not a pair
    ],
)
def test_bad_input_raises_value_error(kwargs):
    system = build_system()
    before = system_state(system)
    fs = FastSweep(system, backend="cpu")
    with pytest.raises(ValueError):
        fs.plan_slo(**kwargs)
    assert system_state(system) == before


def test_shared_target_needs_equal_targets():
    system = build_system()
    names = sorted(system.servers)
    a, b = system.servers[names[3]], system.servers[names[5]]
    b.service_class_name, b.model_name = a.service_class_name, a.model_name
    fs = FastSweep(system, backend="cpu")
    shared, owner = fs._server_targets()
    assert shared[3] is shared[5] and owner[5] == 3
    ttft, itl = _ones(2) * 500.0, _ones(2) * 50.0
    fs.plan_slo(targets=(ttft, itl))  # equal targets are fine
    itl[1, 5] = 60.0
    before = system_state(system)
    with pytest.raises(ValueError, match="share"):
        fs.plan_slo(targets=(ttft, itl))
    assert system_state(system) == before


def run_cli(monkeypatch, capsys, *argv):
    monkeypatch.setattr(sys, "argv", ["inferno_amd.cli", *argv])
    with pytest.raises(SystemExit) as e:
        cli.main()
    return e.value.code, capsys.readouterr()


def test_cli_plan_slo(monkeypatch, capsys):
    code, io = run_cli(monkeypatch, capsys, "plan", EXAMPLE, "--slo-scales", "0.5,1,2",
                       "--scales", "1,2", "--backend", "cpu", "--json")
    assert code == 0
    doc = json.loads(io.out)
    assert doc["referenceSloScale"] == 1.0 and doc["referenceScale"] == 1.0
    blocks = doc["sloScenarios"]
    assert [b["sloScale"] for b in blocks] == [0.5, 1.0, 2.0]
    for b in blocks:
        assert [r["scale"] for r in b["scenarios"]] == [1.0, 2.0]
        for r in b["scenarios"]:
            assert set(r) == {"scale", "totalCost", "replicas", "infeasibleServers",
                              "acceleratorChanges"}
    assert blocks[1]["scenarios"][0]["acceleratorChanges"] == 0
    # the SLO-scale-1 block is the load plan
    code, io = run_cli(monkeypatch, capsys, "plan", EXAMPLE, "--scales", "1,2", "--backend",
                       "cpu", "--json")
    assert code == 0
    assert json.loads(io.out)["scenarios"] == blocks[1]["scenarios"]
    # a looser SLO never costs more
    cost = [b["scenarios"][0]["totalCost"] for b in blocks if not
            b["scenarios"][0]["infeasibleServers"]]
    assert cost == sorted(cost, reverse=True)
    # the table form prints one block per SLO scale; load scale 1 by default
    code, io = run_cli(monkeypatch, capsys, "plan", EXAMPLE, "--slo-scales", "0.5,1,2",
                       "--backend", "cpu")
    assert code == 0
    assert len([ln for ln in io.out.splitlines() if ln.startswith("SLO scale ")]) == 3
    for extra in (("--capacity", "MI300X=4"), ("--limited",)):
        code, io = run_cli(monkeypatch, capsys, "plan", EXAMPLE, "--slo-scales", "0.5,1",
                           "--backend", "cpu", *extra)
        assert code not in (0, None)
        assert io.out == ""
