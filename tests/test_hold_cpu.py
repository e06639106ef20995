"""Hold analysis on the CPU golden path (FastSweep.hold, backend="cpu"): input
validation, the precedence of the verdicts, the default allocation, the
rollout composition, and the tie to plan(): a fleet held at the plan's own
winners meets its SLO everywhere."""
import copy

import numpy as np
import pytest

from inferno_amd.core import System
from inferno_amd.core.allocation import Allocation
from inferno_amd.engine import (
    HOLD_IDLE,
    HOLD_INVALID,
    HOLD_NOT_HELD,
    HOLD_OK,
    HOLD_OVERLOADED,
    HOLD_SLO_VIOLATED,
    FastSweep,
)
from tests.fixtures import make_spec

SCALES = (1.0, 0.0, 0.5, 2.5)
INFEASIBLE_SRV = 3
INVALID_SRV = 4


def build_system(analyzer_mode=None):
    system, _ = System.from_spec(make_spec(n_servers=6, seed=77, arrival_scale=3000.0))
    names = sorted(system.servers)
    srv = system.servers[names[INFEASIBLE_SRV]]
    t = system.service_classes[srv.service_class_name].targets[srv.model_name]
    t.itl, t.ttft = 1e-3, 0.0  # unreachable, as in tests/test_plan_gpu.py
    if analyzer_mode is not None:
        system.analyzer_mode = analyzer_mode
    return system


def planner(analyzer_mode=None):
    return FastSweep(build_system(analyzer_mode), backend="cpu")


def test_validation():
    fs = planner()
    n = len(fs.server_names)
    acc, rep = np.zeros(n, dtype=np.int32), np.ones(n, dtype=np.int32)
    bad = [
        dict(),  # neither scales nor arrival
        dict(scales=[1.0], arrival=np.ones((1, n))),
        dict(scales=[1.0] * 257),
        dict(scales=[-1.0]),
        dict(scales=[1.0], allocation=(acc,)),
        dict(scales=[1.0], allocation=(acc[:-1], rep[:-1])),
        dict(scales=[1.0, 2.0],
             allocation=(np.zeros((3, n), dtype=int), np.ones((3, n), dtype=int))),
        dict(scales=[1.0], allocation=(acc + 0.5, rep)),
        dict(scales=[1.0], allocation=(acc, rep + 0.25)),
        dict(scales=[1.0], allocation=(["a"] * n, rep)),
        dict(scales=[1.0], allocation=(acc + len(fs.acc_names), rep)),
        dict(scales=[1.0], allocation=(acc, -rep)),
        dict(scales=[1.0], allocation=(acc, rep.astype(np.int64) << 31)),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            fs.hold(**kw)
    # negative replicas are fine where nothing is held; integral floats are integers
    r = fs.hold(scales=[1.0], allocation=(np.full(n, -2.0), -rep))
    assert (r.status == HOLD_NOT_HELD).all()


def test_status_precedence_and_fields():
    fs = planner()
    names = fs.server_names
    n = len(names)
    # server 4: degenerate perf data on accelerator 0
    srv = fs.system.servers[names[INVALID_SRV]]
    bad_acc = fs.acc_names[0]
    perf = fs.system.models[srv.model_name].get_perf_data(bad_acc)
    perf.decodeParms.alpha = perf.decodeParms.beta = 0.0
    perf.prefillParms.gamma = perf.prefillParms.delta = 0.0
    fs = FastSweep(fs.system, backend="cpu")
    p = fs.plan(scales=[1.0]).winners
    acc = np.where(p.acc_idx[0] >= 0, p.acc_idx[0], 0).astype(np.int32)
    rep = np.maximum(p.num_replicas[0], 1).astype(np.int32)
    acc[0] = -1  # holds nothing
    rep[1] = 0  # an accelerator without replicas
    acc[INVALID_SRV] = 0
    rep[INFEASIBLE_SRV] = 1 << 20  # no winner there: enough replicas to be evaluated
    scen = np.repeat(fs._base_load()[0][None, :], 3, axis=0).astype(np.float32)
    scen[1] = 0.0  # IDLE beats INVALID and OVERLOADED, NOT_HELD beats IDLE
    scen[2] *= 1e4  # everything held is overloaded
    r = fs.hold(arrival=scen, allocation=(acc, rep))
    assert r.status.shape == (3, n) and r.status.dtype == np.int32
    assert (r.status[:, 0] == HOLD_NOT_HELD).all()
    assert (r.needed_replicas[:, 0] == -1).all() and (r.cost[:, 0] == 0).all()
    assert (r.status[1, 1:] == HOLD_IDLE).all() and (r.needed_replicas[1, 1:] == 0).all()
    assert r.status[0, 1] == HOLD_OVERLOADED and r.rate[0, 1] == 0
    assert np.isinf(r.itl[0, 1]) and np.isinf(r.ttft[0, 1]) and r.rho[0, 1] == 1
    assert (r.status[[0, 2], INVALID_SRV] == HOLD_INVALID).all()
    assert (r.needed_replicas[[0, 2], INVALID_SRV] == -1).all()
    assert r.status[0, INFEASIBLE_SRV] == HOLD_SLO_VIOLATED  # evaluated, SLO unreachable
    assert r.needed_replicas[0, INFEASIBLE_SRV] == -1 and r.slo_rate[0, INFEASIBLE_SRV] == 0
    assert np.isfinite(r.itl[0, INFEASIBLE_SRV]) and r.itl[0, INFEASIBLE_SRV] > 0
    rest = [i for i in range(n) if i not in (0, 1, INVALID_SRV, INFEASIBLE_SRV)]
    assert (r.status[0, rest] == HOLD_OK).all()
    assert (r.status[2, rest] == HOLD_OVERLOADED).all()
    assert r.status[2, INFEASIBLE_SRV] == HOLD_SLO_VIOLATED
    assert (r.needed_replicas[2, rest] > rep[rest]).all()
    # sums
    for s in range(3):
        assert np.array_equal(r.counts[s], np.bincount(r.status[s], minlength=6))
    want = np.zeros_like(r.deficit_by_acc)
    for s in range(3):
        for i in range(n):
            if r.status[s, i] != HOLD_NOT_HELD and r.needed_replicas[s, i] >= 0:
                want[s, r.acc_idx[s, i]] += max(
                    int(r.needed_replicas[s, i]) - int(r.held_replicas[s, i]), 0)
    assert np.array_equal(r.deficit_by_acc, want) and want[2].sum() > 0
    assert r.counts.dtype == np.int64 and r.deficit_by_acc.dtype == np.int64
    # cost and slo_rate of an evaluated slice
    i = rest[0]
    k = [c for c in range(fs.n_cells)
         if fs.cell_server[c] == i and fs.cell_acc_idx[c] == acc[i]][0]
    assert r.cost[0, i] == np.float32(fs._stat["acc_cost"][k]) * np.float32(rep[i])
    assert r.slo_rate[0, i] > 0
    assert r.rate[0, i] == np.float32(float(scen[0, i]) / 60.0 / rep[i])


def test_default_allocation_is_the_current_one_and_objects_are_restored():
    fs = planner()
    names = fs.server_names
    for j, name in enumerate(names[:4]):
        fs.system.servers[name].cur_allocation = Allocation(
            accelerator=fs.acc_names[j % len(fs.acc_names)], num_replicas=j + 1, cost=1.0)
    fs.system.servers[names[4]].cur_allocation = Allocation()  # empty
    fs.system.servers[names[5]].cur_allocation = None
    before = [(copy.deepcopy(s.load), copy.deepcopy(s.cur_allocation), s.allocation)
              for s in fs._srv_objs]
    cur_acc, cur_rep, _ = fs._base_cur()
    a = fs.hold(scales=SCALES)
    b = fs.hold(scales=SCALES, allocation=(cur_acc, cur_rep))
    for f in ("status", "acc_idx", "held_replicas", "needed_replicas", "itl", "ttft", "rho",
              "rate", "slo_rate", "cost", "counts", "deficit_by_acc"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert (a.status[:, 4:] == HOLD_NOT_HELD).all()
    assert np.array_equal(a.held_replicas[0, :4], [1, 2, 3, 4])
    # the override, when set, is the current allocation
    fs.cur_override = (np.full(len(names), -3, dtype=np.int32), cur_rep, np.zeros(len(names)))
    assert (fs.hold(scales=[1.0]).status == HOLD_NOT_HELD).all()
    fs.cur_override = None
    after = [(s.load, s.cur_allocation, s.allocation) for s in fs._srv_objs]
    for (l0, c0, a0), (l1, c1, a1) in zip(before, after):
        assert l0 == l1 and c0 == c1 and a0 is a1


@pytest.mark.parametrize("mode", [None, "mg1"])
def test_held_at_the_plan_winners_is_ok(mode):
    fs = planner(mode)
    p = fs.plan(scales=SCALES)
    w = p.winners
    r = fs.hold(scales=SCALES, allocation=(w.acc_idx, w.num_replicas))
    held = w.acc_idx >= 0
    assert held.any() and (~held).any()
    assert (r.status[~held] == HOLD_NOT_HELD).all()
    zero = np.asarray(SCALES) == 0.0
    assert (r.status[zero][held[zero]] == HOLD_IDLE).all()
    live = held & ~zero[:, None]
    assert (r.status[live] == HOLD_OK).all()
    min_rep = np.array([s.min_num_replicas for s in fs._srv_objs])[None, :]
    assert np.array_equal(np.maximum(r.needed_replicas, min_rep)[live], w.num_replicas[live])
    for f in ("itl", "ttft", "rho"):
        assert np.array_equal(getattr(r, f)[live], getattr(w, f)[live]), f
    # one replica short where that leaves at least one: never OK
    short = live & (r.needed_replicas >= 2)
    assert short.any()
    r2 = fs.hold(scales=SCALES, allocation=(w.acc_idx, np.where(short, r.needed_replicas - 1,
                                                                w.num_replicas)))
    assert np.isin(r2.status[short], (HOLD_SLO_VIOLATED, HOLD_OVERLOADED)).all()
    assert r2.deficit_by_acc.sum() == short.sum()


def test_rollout_recipe():
    """The SLO verdict of every tick under one tick of actuation lag."""
    fs = planner()
    base = fs._base_load()[0]
    f = np.stack([base * np.float32(x) for x in (1.0, 1.5, 3.0, 0.5)]).astype(np.float32)
    r = fs.rollout(arrival=f)
    h = fs.hold(arrival=f[1:], allocation=(r.winners.acc_idx[:-1], r.winners.num_replicas[:-1]))
    assert h.status.shape == (3, len(fs.server_names))
    # the ramp 1.5x -> 3x is served by the 1.5x fleet: somebody is short
    assert np.isin(h.status[1], (HOLD_SLO_VIOLATED, HOLD_OVERLOADED)).any()
    # the drop 3x -> 0.5x is served by the 3x fleet: nobody held is short
    held = h.status[2] != HOLD_NOT_HELD
    assert (h.status[2][held] == HOLD_OK).all() and h.deficit_by_acc[2].sum() == 0
    # final_cur's codes pass straight in as well
    acc, rep, _ = r.final_cur
    assert fs.hold(arrival=f[-1:], allocation=(acc, rep)).status.shape == (1, len(base))


def run_cli(monkeypatch, capsys, *argv):
    import sys

    from inferno_amd import cli

    monkeypatch.setattr(sys, "argv", ["inferno_amd.cli", *argv])
    with pytest.raises(SystemExit) as e:
        cli.main()
    return e.value.code, capsys.readouterr()


def test_cli_plan_hold(monkeypatch, capsys):
    import json
    import os

    example = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                           "examples", "system.json")
    code, io = run_cli(monkeypatch, capsys, "plan", example, "--hold", "--scales", "0.5,1,4",
                       "--backend", "cpu", "--json")
    assert code == 0
    doc = json.loads(io.out)
    rows = doc["hold"]
    assert [r["scale"] for r in rows] == [0.5, 1.0, 4.0]
    for r in rows:
        assert sum(r["status"].values()) == doc["servers"]
        assert len(r["notOk"]) == doc["servers"] - r["status"]["OK"]
        short = sum(max(b["neededReplicas"] - b["heldReplicas"], 0) for b in r["notOk"]
                    if b["status"] != "NOT_HELD" and b["neededReplicas"] >= 0)
        assert sum(r["deficit"].values()) == short
    # more load on the same replicas: never fewer servers in trouble
    assert rows[2]["status"]["OK"] <= rows[1]["status"]["OK"] <= rows[0]["status"]["OK"]
    code, io = run_cli(monkeypatch, capsys, "plan", example, "--hold", "--scales", "1,4",
                       "--backend", "cpu")
    assert code == 0 and "load scale 4" in io.out and "held at every load scale" in io.out
    for extra in (["--rollout"], ["--limited"], ["--capacity", "X=1"], ["--slo-scales", "1"],
                  ["--token-scales", "1:1"]):
        code, io = run_cli(monkeypatch, capsys, "plan", example, "--hold", "--scales", "1",
                           "--backend", "cpu", *extra)
        assert code not in (0, None) and "--hold" in str(code)
    code, _ = run_cli(monkeypatch, capsys, "plan", example, "--hold", "--backend", "cpu")
    assert "--hold needs --scales" in str(code)
