"""Forecast ensembles (FastSweep.rollout_ensemble) without a GPU: input
validation, the nearest-rank rule, the CPU golden path against per-path
rollout() calls, the band helpers, noisy_paths and the CLI."""
import dataclasses
import json
import os
import sys

import numpy as np
import pytest

from inferno_amd import cli
from inferno_amd.core import System
from inferno_amd.engine import (
    ENSEMBLE_MAX_PATHS,
    ENSEMBLE_MAX_ROWS,
    FastSweep,
    ensemble_bands,
    ensemble_mode,
    ensemble_path_cost,
    ensemble_ranks,
    noisy_paths,
)
from inferno_amd.ops.sweep import PLAN_MAX_S
from tests.fixtures import make_spec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLE = os.path.join(REPO, "examples", "system.json")
FIELDS = ("acc_idx", "num_replicas", "batch", "cost", "value", "itl", "ttft", "rho", "max_rate")
# E = 3 paths of S = 2 ticks: one rises, one falls to nothing, one stays low
PATHS = ((1.0, 3.0), (2.0, 0.0), (0.4, 0.5))
QUANTILES = (0.2, 0.5, 1.0)


def build_fs():
    system, _ = System.from_spec(make_spec(n_servers=3, seed=5, arrival_scale=600.0))
    system.servers[sorted(system.servers)[1]].min_num_replicas = 0
    return FastSweep(system, backend="cpu")


def object_state(system):
    return [
        (n, s.load.arrivalRate, s.load.avgInTokens, s.load.avgOutTokens, id(s.cur_allocation),
         dataclasses.astuple(s.cur_allocation), id(s.allocation))
        for n, s in sorted(system.servers.items())
    ]


@pytest.fixture(scope="module")
def solved():
    fs = build_fs()
    assert len(fs.server_names) == 3 and len(fs.acc_names) == 3
    before = object_state(fs.system)
    res = fs.rollout_ensemble(scales=PATHS, quantiles=QUANTILES, return_paths=True)
    after = object_state(fs.system)
    refs = [fs.rollout(arrival=res.arrival[e]) for e in range(len(PATHS))]
    return fs, res, refs, before, after


# -- validation -----------------------------------------------------------------
@pytest.mark.parametrize("kwargs,match", [
    ({}, r"rollout_ensemble\(\) takes exactly one of scales and arrival"),
    ({"scales": [[1.0]], "arrival": np.ones((1, 1, 3))}, "exactly one of scales and arrival"),
    ({"scales": [1.0, 2.0]}, r"scales must have shape \[E, S\]"),
    ({"arrival": np.ones((2, 3))}, r"arrival must have shape \[E, S, 3\]"),
    ({"arrival": np.ones((2, 2, 4))}, r"arrival must have shape \[E, S, 3\]"),
    ({"scales": np.ones((0, 2))}, r"rollout_ensemble\(\) takes 1\.\.256 paths, got 0"),
    ({"scales": np.ones((257, 1))}, r"takes 1\.\.256 paths, got 257"),
    ({"scales": np.ones((1, PLAN_MAX_S + 1))}, r"takes 1\.\.256 steps, got 257"),
    ({"scales": np.ones((17, 241))}, r"at most 4096 paths x steps, got 17 x 241 = 4097"),
    ({"scales": [[1.0, -1.0]]}, "scales must be finite and non-negative"),
    ({"scales": [[1.0, float("nan")]]}, "scales must be finite and non-negative"),
    ({"arrival": np.full((1, 1, 3), -1.0)}, "arrival must be finite and non-negative"),
    ({"scales": [[1e38]]}, "scales overflows float32"),
    ({"arrival": np.full((1, 1, 3), 1e39)}, "arrival overflows float32"),
    ({"scales": [["x"]]}, "scales is not numeric"),
    ({"scales": [[1.0]], "quantiles": ()}, r"takes 1\.\.8 quantiles"),
    ({"scales": [[1.0]], "quantiles": [0.1] * 9}, r"takes 1\.\.8 quantiles"),
    ({"scales": [[1.0]], "quantiles": [0.0]}, r"quantiles must lie in \(0, 1\]"),
    ({"scales": [[1.0]], "quantiles": [1.5]}, r"quantiles must lie in \(0, 1\]"),
    ({"scales": [[1.0]], "quantiles": [float("nan")]}, r"quantiles must lie in \(0, 1\]"),
])
def test_bad_input_raises_value_error(kwargs, match):
    fs = build_fs()
    assert ENSEMBLE_MAX_PATHS == 256 and ENSEMBLE_MAX_ROWS == 4096 and PLAN_MAX_S == 256
    with pytest.raises(ValueError, match=match):
        fs.rollout_ensemble(**kwargs)


def test_byte_limit(monkeypatch):
    fs = build_fs()
    # 13 segments padded to 256 bytes each; only the fleet bands (3 quantiles x
    # 2 ticks x 6 columns x 8 bytes = 288) need two such units
    need = 14 * 256
    monkeypatch.setenv("INFERNO_ENSEMBLE_BYTES", str(need - 1))
    with pytest.raises(ValueError, match=rf"arena of {need} bytes .*INFERNO_ENSEMBLE_BYTES"):
        fs.rollout_ensemble(scales=PATHS)
    monkeypatch.setenv("INFERNO_ENSEMBLE_BYTES", str(need))  # read per call
    fs.rollout_ensemble(scales=PATHS)
    monkeypatch.setenv("INFERNO_ENSEMBLE_BYTES", "many")
    with pytest.raises(ValueError, match="must be an integer"):
        fs.rollout_ensemble(scales=PATHS)


# -- the rank rule --------------------------------------------------------------
def test_rank_table():
    # k = clamp(ceil(q * E) - 1, 0, E - 1) on the decimal q
    table = {
        1: {0.01: 0, 0.5: 0, 0.9: 0, 1.0: 0},
        2: {0.01: 0, 0.5: 0, 0.9: 1, 1.0: 1},
        3: {0.01: 0, 0.5: 1, 0.9: 2, 1.0: 2},
        4: {0.01: 0, 0.5: 1, 0.9: 3, 1.0: 3},
        5: {0.01: 0, 0.5: 2, 0.9: 4, 1.0: 4},
        10: {0.01: 0, 0.5: 4, 0.9: 8, 1.0: 9},
    }
    for n, row in table.items():
        got = ensemble_ranks(list(row), n)
        assert got.dtype == np.int64
        assert got.tolist() == list(row.values()), n
    assert ensemble_ranks([0.9], 10).tolist() == [8]
    # where binary floating point says otherwise: 0.07 * 100 rounds above 7
    assert int(np.ceil(0.07 * 100)) - 1 == 7
    assert ensemble_ranks([0.07], 100).tolist() == [6]


# -- the golden path ------------------------------------------------------------
def test_paths_are_rollouts(solved):
    fs, res, refs, _, _ = solved
    base = fs._base_load()[0]
    want = base[None, None, :] * np.asarray(PATHS, dtype=np.float32)[:, :, None]
    assert res.arrival.dtype == np.float32 and res.arrival.tobytes() == want.tobytes()
    assert res.quantiles.tolist() == list(QUANTILES) and res.ranks.tolist() == [0, 1, 2]
    for e, ref in enumerate(refs):
        for f in FIELDS:
            got, exp = getattr(res.paths.winners, f)[e], getattr(ref.winners, f)
            assert got.dtype == exp.dtype and got.tobytes() == exp.tobytes(), (e, f)
        for k in range(3):
            assert res.paths.final_cur[k][e].tobytes() == ref.final_cur[k].tobytes()
        assert np.array_equal(res.path_replicas_by_acc[e], ref.replicas_by_acc)
        assert np.array_equal(res.path_infeasible_servers[e], ref.infeasible_servers)
        assert np.array_equal(res.path_acc_changes[e], ref.acc_changes)
        want_cost = np.cumsum(ref.winners.cost.astype(np.float64), axis=1)[:, -1]
        assert res.path_cost_total[e].tobytes() == want_cost.tobytes()
        assert np.allclose(res.path_cost_total[e], ref.cost_total, rtol=1e-12, atol=0.0)
    for a in (res.path_replicas_by_acc, res.path_infeasible_servers, res.path_acc_changes):
        assert a.dtype == np.int64
    assert res.path_cost_total.dtype == np.float64
    # the paths differ, so the bands are not one path's values
    assert (res.paths.winners.num_replicas[0] != res.paths.winners.num_replicas[1]).any()


def test_bands_are_sorted_paths(solved):
    _, res, refs, _, _ = solved
    rk = res.ranks

    def stack(get):
        return np.stack([get(r) for r in refs])

    cost = stack(lambda r: np.cumsum(r.winners.cost.astype(np.float64), axis=1)[:, -1])
    checks = (
        (res.replicas_by_acc_q, stack(lambda r: r.replicas_by_acc), np.int64),
        (res.cost_total_q, cost, np.float64),
        (res.infeasible_q, stack(lambda r: r.infeasible_servers), np.int64),
        (res.acc_changes_q, stack(lambda r: r.acc_changes), np.int64),
        (res.server_replicas_q, stack(lambda r: r.winners.num_replicas), np.int32),
        (res.server_cost_q, stack(lambda r: r.winners.cost), np.float32),
    )
    for got, per_path, dtype in checks:
        want = np.sort(per_path, axis=0)[rk]
        assert got.dtype == dtype and got.shape == want.shape
        assert got.tobytes() == want.astype(dtype).tobytes()
    codes = stack(lambda r: r.winners.acc_idx)
    mode, count = ensemble_mode(codes)
    assert res.acc_mode.dtype == np.int32 and res.acc_mode_paths.dtype == np.int32
    assert np.array_equal(res.acc_mode, mode) and np.array_equal(res.acc_mode_paths, count)
    for s in range(codes.shape[1]):
        for v in range(codes.shape[2]):
            col = codes[:, s, v]
            assert count[s, v] == (col == mode[s, v]).sum() == max(
                (col == c).sum() for c in col)
    assert res.server_replicas_q.shape == (3, 2, 3) and res.acc_mode.shape == (2, 3)


def test_identical_paths_collapse():
    fs = build_fs()
    one = fs.rollout(scales=PATHS[0])
    res = fs.rollout_ensemble(scales=[PATHS[0]] * 4, quantiles=(0.01, 0.3, 0.75, 1.0))
    assert res.paths is None
    assert res.ranks.tolist() == [0, 1, 2, 3]
    assert (res.acc_mode_paths == 4).all()
    assert np.array_equal(res.acc_mode, one.winners.acc_idx)
    for q in range(4):
        assert np.array_equal(res.server_replicas_q[q], one.winners.num_replicas)
        assert res.server_cost_q[q].tobytes() == one.winners.cost.tobytes()
        assert np.array_equal(res.replicas_by_acc_q[q], one.replicas_by_acc)
        assert np.array_equal(res.infeasible_q[q], one.infeasible_servers)
        assert np.array_equal(res.acc_changes_q[q], one.acc_changes)
        assert res.cost_total_q[q].tobytes() == ensemble_path_cost(one.winners.cost).tobytes()


def test_objects_and_override_unchanged(solved):
    fs, _, _, before, after = solved
    assert before == after
    cur = tuple(np.array(a) for a in fs._base_cur())
    cur[0][0] = -3
    fs.cur_override = cur
    try:
        saved = [a.copy() for a in cur]
        res = fs.rollout_ensemble(scales=PATHS, return_paths=True)
        assert fs.cur_override is cur
        for a, b in zip(cur, saved):
            assert a.tobytes() == b.tobytes()
        ref = fs.rollout(scales=PATHS[2])
        assert np.array_equal(res.paths.winners.acc_idx[2], ref.winners.acc_idx)
        assert np.array_equal(res.path_acc_changes[2], ref.acc_changes)
    finally:
        fs.cur_override = None
    assert object_state(fs.system) == before


# -- helpers ----------------------------------------------------------------------
def test_mode_ties_take_the_smallest_code():
    codes = np.array([[0, 1, -1, 2],
                      [-1, 1, -1, 2],
                      [-2, 0, 0, -2]], dtype=np.int32)
    mode, count = ensemble_mode(codes)
    assert mode.tolist() == [-2, 1, -1, 2] and count.tolist() == [1, 2, 2, 2]
    assert mode.dtype == np.int32 and count.dtype == np.int32


def test_bands_and_cost_helpers():
    vals = np.array([[3.0, 1.0], [1.0, 1.0], [2.0, 5.0]], dtype=np.float32)
    assert ensemble_bands(vals, [0, 2, 2]).tolist() == [[1.0, 1.0], [3.0, 5.0], [3.0, 5.0]]
    cost = np.array([[0.1, 0.2, 0.3], [1e8, 1.0, -1e8]], dtype=np.float32)
    want = [float(np.float32(0.1)) + float(np.float32(0.2)) + float(np.float32(0.3)),
            (1e8 + 1.0) - 1e8]
    assert ensemble_path_cost(cost).tolist() == want
    assert ensemble_path_cost(np.zeros((2, 0), dtype=np.float32)).tolist() == [0.0, 0.0]


def test_noisy_paths_properties():
    scales = [0.5, 1.0, 2.0, 0.0]
    a = noisy_paths(scales, 0.2, 5, seed=7)
    assert a.shape == (5, 4) and a.dtype == np.float64
    assert np.array_equal(a, noisy_paths(scales, 0.2, 5, seed=7))
    assert not np.array_equal(a, noisy_paths(scales, 0.2, 5, seed=8))
    assert a[0].tolist() == scales
    assert (a[:, :3] > 0).all() and (a[:, 3] == 0).all() and np.isfinite(a).all()
    assert np.array_equal(noisy_paths(scales, 0.0, 3, seed=1), np.tile(scales, (3, 1)))
    for bad in ({"scales": [], "sigma": 0.1, "n_paths": 2}, {"scales": [1.0], "sigma": -1.0,
                "n_paths": 2}, {"scales": [1.0], "sigma": 0.1, "n_paths": 0},
                {"scales": [-1.0], "sigma": 0.1, "n_paths": 1}):
        with pytest.raises(ValueError):
            noisy_paths(seed=0, **bad)


# -- CLI ------------------------------------------------------------------------------
def run_cli(monkeypatch, capsys, *argv, code=0):
    monkeypatch.setattr(sys, "argv", ["inferno_amd.cli", *argv])
    with pytest.raises(SystemExit) as e:
        cli.main()
    assert e.value.code == code
    return capsys.readouterr().out


def test_cli_plan_ensemble(monkeypatch, capsys):
    text = "0.5,1,2;0.6,1.2,2.4;0.4,0.9,1.7"
    paths = [[0.5, 1.0, 2.0], [0.6, 1.2, 2.4], [0.4, 0.9, 1.7]]
    out = run_cli(monkeypatch, capsys, "plan", EXAMPLE, "--ensemble-scales", text,
                  "--quantiles", "0.5,1", "--backend", "cpu", "--json")
    doc = json.loads(out)
    rows = doc["ensemble"]
    assert doc["paths"] == 3 and doc["steps"] == 3
    assert [(r["step"], r["quantile"]) for r in rows] == [
        (s, q) for s in range(3) for q in (0.5, 1.0)]
    for r in rows:
        assert set(r) == {"step", "quantile", "rank", "totalCost", "replicas",
                          "infeasibleServers", "acceleratorChanges", "unanimousServers"}
    system, _ = cli._load_system(EXAMPLE)
    fs = FastSweep(system, backend="cpu")
    res = fs.rollout_ensemble(scales=paths, quantiles=(0.5, 1.0))
    assert doc["servers"] == len(fs.server_names)
    for r in rows:
        s, k = r["step"], (0.5, 1.0).index(r["quantile"])
        assert r["rank"] == int(res.ranks[k])
        assert r["totalCost"] == round(float(res.cost_total_q[k, s]), 2)
        assert r["replicas"] == {n: int(res.replicas_by_acc_q[k, s, j])
                                 for j, n in enumerate(fs.acc_names)}
        assert r["infeasibleServers"] == int(res.infeasible_q[k, s])
        assert r["acceleratorChanges"] == int(res.acc_changes_q[k, s])
        assert r["unanimousServers"] == int((res.acc_mode_paths[s] == 3).sum())
    # the table form prints one line per step and quantile (three by default)
    table = run_cli(monkeypatch, capsys, "plan", EXAMPLE, "--ensemble-scales", text,
                    "--backend", "cpu")
    lines = [ln.split() for ln in table.splitlines()]
    assert [ln[0] for ln in lines if ln and ln[0].isdigit()] == [
        str(s) for s in range(3) for _ in range(3)]


def test_cli_ensemble_noise(monkeypatch, capsys):
    out = run_cli(monkeypatch, capsys, "plan", EXAMPLE, "--scales", "0.5,1,2",
                  "--ensemble-noise", "0.2", "--paths", "4", "--seed", "3", "--backend", "cpu",
                  "--json")
    doc = json.loads(out)
    assert doc["paths"] == 4 and doc["steps"] == 3 and len(doc["ensemble"]) == 9
    system, _ = cli._load_system(EXAMPLE)
    fs = FastSweep(system, backend="cpu")
    res = fs.rollout_ensemble(scales=noisy_paths([0.5, 1.0, 2.0], 0.2, 4, 3))
    assert [r["totalCost"] for r in doc["ensemble"]] == [
        round(float(res.cost_total_q[k, s]), 2) for s in range(3) for k in range(3)]


@pytest.mark.parametrize("argv", [
    ["--ensemble-scales", "1,2;2,3", "--rollout"],
    ["--ensemble-scales", "1,2;2,3", "--hold"],
    ["--ensemble-scales", "1,2;2,3", "--slo-scales", "1,2"],
    ["--ensemble-scales", "1,2;2,3", "--token-scales", "1:1"],
    ["--ensemble-scales", "1,2;2,3", "--limited"],
    ["--ensemble-scales", "1,2;2,3", "--capacity", "X=1"],
    ["--ensemble-scales", "1,2;2,3", "--scales", "1,2"],
    ["--ensemble-scales", "1,2;2"],
    ["--ensemble-scales", "1,x"],
    ["--ensemble-noise", "0.2"],
    ["--ensemble-noise", "0.2", "--scales", "1,2", "--rollout"],
])
def test_cli_ensemble_exclusive_flags(monkeypatch, argv):
    monkeypatch.setattr(sys, "argv", ["inferno_amd.cli", "plan", EXAMPLE, "--backend", "cpu",
                                      *argv])
    with pytest.raises(SystemExit) as e:
        cli.main()
    assert isinstance(e.value.code, str) and e.value.code  # a message, not a status
