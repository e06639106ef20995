"""What-if token-mix planning on the CPU backend: FastSweep.plan_tokens against
a loop of plan(arrival=...) calls under load overrides that carry the token
sets, restoring the system, the rounding rule of token_scales, input validation
and `plan --token-scales`.

The fleet is the one of tests/test_plan_gpu.py (9 servers x 3 accelerators)."""
import json
import os
import sys

import numpy as np
import pytest

from inferno_amd import cli
from inferno_amd.engine import FastSweep, TokenPlanResult
from tests.test_plan_gpu import SCALE_TO_ZERO_SRV, base_loads, build_system

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = os.path.join(REPO, "examples", "system.json")
TOKEN_SCALES = ((1.0, 1.0), (4.0, 1.0), (1.0, 0.5), (0.3, 2.5))
LOAD_SCALES = (1.0, 0.0, 1.7)
FIELDS = ("acc_idx", "num_replicas", "batch", "cost", "value", "itl", "ttft", "rho", "max_rate")


def system_state(system):
    return [(s.load.arrivalRate, s.load.avgInTokens, s.load.avgOutTokens, s.allocation,
             s.cur_allocation) for _, s in sorted(system.servers.items())]


def scaled(base, f):
    """floor(float64(base) * f), a positive base never below 1."""
    v = np.floor(base.astype(np.float64) * f)
    return np.where(base > 0, np.maximum(v, 1), v).astype(np.int32)


def token_sets():
    _, in_tok, out_tok = base_loads(build_system())
    return (np.stack([scaled(in_tok, f) for f, _ in TOKEN_SCALES]),
            np.stack([scaled(out_tok, f) for _, f in TOKEN_SCALES]))


def load_scenarios():
    arrival, _, _ = base_loads(build_system())
    return np.stack([arrival * np.float32(sc) for sc in LOAD_SCALES]).astype(np.float32)


def assert_equals_plan_loop(res, t_in, t_out, scen):
    """Set w of res against plan(arrival=scen) on a fresh FastSweep whose load
    override carries set w, field for field."""
    n_w, n_s = t_in.shape[0], scen.shape[0]
    for w in range(n_w):
        twin = FastSweep(build_system(), backend="cpu")
        twin.load_override = (scen[0].copy(), t_in[w].copy(), t_out[w].copy())
        want = twin.plan(arrival=scen)
        for f in FIELDS:
            got = getattr(res.winners, f)
            assert got.shape == (n_w, n_s, 9)
            assert got.dtype == getattr(want.winners, f).dtype
            assert np.array_equal(got[w], getattr(want.winners, f)), f"set {w}: {f}"
        assert np.array_equal(res.replicas_by_acc[w], want.replicas_by_acc)
        assert np.array_equal(res.cost_total[w], want.cost_total)
        assert np.array_equal(res.infeasible_servers[w], want.infeasible_servers)


@pytest.fixture(scope="module")
def planned():
    system = build_system()
    before = system_state(system)
    fs = FastSweep(system, backend="cpu")
    res = fs.plan_tokens(token_scales=TOKEN_SCALES, scales=LOAD_SCALES)
    return system, before, fs, res


def test_plan_tokens_equals_loop_of_plans(planned):
    system, before, fs, res = planned
    assert isinstance(res, TokenPlanResult)
    t_in, t_out = token_sets()
    scen = load_scenarios()
    assert np.array_equal(res.in_tok, t_in) and res.in_tok.dtype == np.int32
    assert np.array_equal(res.out_tok, t_out) and res.out_tok.dtype == np.int32
    assert np.array_equal(res.arrival, scen) and res.arrival.dtype == np.float32
    assert res.cells is None
    assert res.replicas_by_acc.dtype == np.int64 and res.cost_total.dtype == np.float64
    assert res.cost_total.shape == res.infeasible_servers.shape == (4, 3)
    assert_equals_plan_loop(res, t_in, t_out, scen)
    zero = LOAD_SCALES.index(0.0)
    assert (res.winners.acc_idx[:, zero, SCALE_TO_ZERO_SRV] == -2).all()
    # the request shape matters: replicas and some winning accelerator move
    assert (res.winners.num_replicas[1, 0] != res.winners.num_replicas[0, 0]).any()
    acc = res.winners.acc_idx[:, 0]
    assert ((acc != acc[0]) & (acc >= 0) & (acc[0] >= 0)).any()
    assert system_state(system) == before  # the caller's system is untouched
    assert fs.load_override is None


def test_explicit_tokens_equal_scales_and_override_is_kept(planned):
    _, _, fs, res = planned
    again = fs.plan_tokens(tokens=(res.in_tok, res.out_tok), arrival=res.arrival)
    for f in FIELDS:
        assert np.array_equal(getattr(again.winners, f), getattr(res.winners, f)), f
    # with a load override set: its arrival rates are the base load, its tokens
    # the base of token_scales, and it is back in place afterwards
    system = build_system()
    arrival, in_tok, out_tok = base_loads(system)
    over = FastSweep(system, backend="cpu")
    override = ((arrival * np.float32(0.5)).astype(np.float32), in_tok * 2, out_tok + 3)
    over.load_override = override
    before = system_state(system)
    got = over.plan_tokens(token_scales=TOKEN_SCALES[:2])
    assert over.load_override is override
    assert system_state(system) == before
    assert got.winners.acc_idx.shape == (2, 1, 9)
    assert np.array_equal(got.arrival[0], override[0])
    assert np.array_equal(got.in_tok, np.stack([in_tok * 2, in_tok * 8]))
    assert np.array_equal(got.out_tok, np.stack([out_tok + 3, out_tok + 3]))
    assert_equals_plan_loop(got, got.in_tok, got.out_tok, got.arrival)
    # without a load axis and at the base tokens: the load plan at scale 1
    base = over.plan_tokens(token_scales=[(1.0, 1.0)])
    want = over.plan(scales=[1.0]).winners
    for f in FIELDS:
        assert np.array_equal(getattr(base.winners, f)[0], getattr(want, f)), f


def test_token_scales_rounding():
    system = build_system()
    names = sorted(system.servers)
    loads = [system.servers[n].load for n in names]
    loads[0].avgInTokens, loads[0].avgOutTokens = 3, 1
    loads[1].avgInTokens, loads[1].avgOutTokens = 0, 7
    loads[2].avgInTokens, loads[2].avgOutTokens = 1000, 999
    fs = FastSweep(system, backend="cpu")
    res = fs.plan_tokens(token_scales=[(0.5, 0.25), (1.9, 1.001), (1e-6, 1e-6)])
    # floor of the float64 product; a positive base never drops below 1; a zero
    # base stays zero
    assert res.in_tok[:, :3].tolist() == [[1, 0, 500], [5, 0, 1900], [1, 0, 1]]
    assert res.out_tok[:, :3].tolist() == [[1, 1, 249], [1, 7, 999], [1, 1, 1]]
    _, in_tok, out_tok = fs._base_load()
    for w, (f_in, f_out) in enumerate(((0.5, 0.25), (1.9, 1.001), (1e-6, 1e-6))):
        assert np.array_equal(res.in_tok[w], scaled(in_tok, f_in))
        assert np.array_equal(res.out_tok[w], scaled(out_tok, f_out))
    with pytest.raises(ValueError):  # 1000 * 3e6 does not fit int32
        fs.plan_tokens(token_scales=[(3e6, 1.0)])


def test_system_restored_on_exception(monkeypatch):
    system = build_system()
    before = system_state(system)
    fs = FastSweep(system, backend="cpu")
    calls = []

    def boom():
        calls.append(1)
        if len(calls) == 5:  # second token set, second load
            raise RuntimeError("boom")
        return FastSweep._reconcile_cpu(fs)

    monkeypatch.setattr(fs, "_reconcile_cpu", boom)
    with pytest.raises(RuntimeError):
        fs.plan_tokens(token_scales=TOKEN_SCALES, scales=LOAD_SCALES)
    assert len(calls) == 5
    assert system_state(system) == before
    assert fs.load_override is None


def _toks(w, n=9, value=100):
    return np.full((w, n), value, dtype=np.int64)


@pytest.mark.parametrize(
    "kwargs",
    [
        {},  # neither token argument
        {"tokens": (_toks(1), _toks(1)), "token_scales": [(1.0, 1.0)]},  # both
        {"tokens": (_toks(2), _toks(3))},  # shapes differ
        {"tokens": (_toks(2, 8), _toks(2, 8))},  # wrong server count
        {"tokens": (_toks(1)[0], _toks(1)[0])},  # 1-D
        {"tokens": (_toks(0), _toks(0))},  # W = 0
        {"tokens": _toks(2)},  # not a pair
        {"tokens": (_toks(2), -_toks(2))},  # negative
        {"tokens": (_toks(2, value=-1), _toks(2))},
        {"tokens": (_toks(2, value=2 ** 31), _toks(2))},  # outside int32
        {"tokens": (_toks(2) + 0.5, _toks(2))},  # not integers
        {"tokens": (_toks(2) * np.nan, _toks(2))},
        {"tokens": (_toks(257), _toks(257))},  # W * S = 257
        {"tokens": (_toks(129), _toks(129)), "scales": [1.0, 2.0]},  # W * S = 258
        {"token_scales": []},  # W = 0
        {"token_scales": [(1.0, 1.0)] * 257},
        {"token_scales": [(1.0, 0.0)]},
        {"token_scales": [(-0.5, 1.0)]},
        {"token_scales": [(1.0, float("nan"))]},
        {"token_scales": [(float("inf"), 1.0)]},
        {"token_scales": [1.0, 2.0]},  # not pairs
        {"token_scales": [(1.0, 1.0, 1.0)]},
        {"token_scales": [(1.0, 1.0)], "scales": [1.0], "arrival": np.ones((1, 9))},
        {"token_scales": [(1.0, 1.0)], "scales": [-1.0]},
    ],
)
def test_bad_input_raises_value_error(kwargs):
    system = build_system()
    before = system_state(system)
    fs = FastSweep(system, backend="cpu")
    with pytest.raises(ValueError):
        fs.plan_tokens(**kwargs)
    assert system_state(system) == before


def run_cli(monkeypatch, capsys, *argv):
    monkeypatch.setattr(sys, "argv", ["inferno_amd.cli", *argv])
    with pytest.raises(SystemExit) as e:
        cli.main()
    return e.value.code, capsys.readouterr()


def test_cli_plan_tokens(monkeypatch, capsys):
    code, io = run_cli(monkeypatch, capsys, "plan", EXAMPLE, "--token-scales", "1:1,4:1,1:0.5",
                       "--scales", "1,2", "--backend", "cpu", "--json")
    assert code == 0
    doc = json.loads(io.out)
    assert doc["referenceTokenScales"] == [1.0, 1.0] and doc["referenceScale"] == 1.0
    blocks = doc["tokenScenarios"]
    assert [(b["inTokenScale"], b["outTokenScale"]) for b in blocks] == [
        (1.0, 1.0), (4.0, 1.0), (1.0, 0.5)]
    for b in blocks:
        assert [r["scale"] for r in b["scenarios"]] == [1.0, 2.0]
        for r in b["scenarios"]:
            assert set(r) == {"scale", "totalCost", "replicas", "infeasibleServers",
                              "acceleratorChanges"}
    assert blocks[0]["scenarios"][0]["acceleratorChanges"] == 0
    # the 1:1 block is the load plan
    code, io = run_cli(monkeypatch, capsys, "plan", EXAMPLE, "--scales", "1,2", "--backend",
                       "cpu", "--json")
    assert code == 0
    assert json.loads(io.out)["scenarios"] == blocks[0]["scenarios"]
    # longer prompts cost more, shorter outputs less
    cost = [b["scenarios"][0]["totalCost"] for b in blocks]
    assert cost[1] > cost[0] > cost[2]
    # the table form prints one row per (set, load); load scale 1 by default
    code, io = run_cli(monkeypatch, capsys, "plan", EXAMPLE, "--token-scales", "1:1,4:1,1:0.5",
                       "--scales", "1,2", "--backend", "cpu")
    assert code == 0
    lines = io.out.splitlines()
    assert len([ln for ln in lines if ln.startswith("token scales ")]) == 3
    assert len([ln for ln in lines if ln.split()[:1] in (["1"], ["2"])]) == 6
    code, io = run_cli(monkeypatch, capsys, "plan", EXAMPLE, "--token-scales", "2:2",
                       "--backend", "cpu")
    assert code == 0
    assert len([ln for ln in io.out.splitlines() if ln.split()[:1] == ["1"]]) == 1
    for extra in (("--slo-scales", "0.5,1"), ("--rollout", "--scales", "1,2"),
                  ("--capacity", "MI300X=4"), ("--limited",)):
        code, io = run_cli(monkeypatch, capsys, "plan", EXAMPLE, "--token-scales", "1:1,2:1",
                           "--backend", "cpu", *extra)
        assert code not in (0, None)
        assert io.out == ""
    for bad in ("1", "1:x", "", "1:2:3"):
        code, io = run_cli(monkeypatch, capsys, "plan", EXAMPLE, "--token-scales", bad,
                           "--backend", "cpu")
        assert code not in (0, None)
        assert io.out == ""
