"""Token-mix planning on the GPU (FastSweep.plan_tokens): every (token set,
load) slice must be bit for bit what the single-scenario path computes —
reconcile_cells / reconcile on a fresh context of an identical system whose
load override is that slice's arrival rates and that set's token averages —
because the same cell function at the same block width produced it.

Fleet: 9 servers x 3 accelerators = 27 cells, batch sizes NOT pinned, so N
follows the output tokens: N = maxBatchSize * atTokens // out_tok. Server 4 may
scale to zero, server 7 has an unreachable SLO. Two loads (the base load; 1.7 x
the base load with server 4 at zero) times five token sets (base; input x 4;
output x 4; output 16 everywhere, which puts N exactly on 2048 .. 32768; output
15 everywhere with one server at (in_tok 0, out_tok 1), N up to 262144, and one
at out_tok 0). The task batch sizes cover all five bucket tiers and both block
widths, and cells change bucket between sets.

Observed on MI355X for test_gpu_plan_tokens_matches_cpu_plan_tokens: 0 replica
flips of 90 winners.
"""
import dataclasses

import numpy as np
import pytest

from inferno_amd.core import System
from inferno_amd.engine import FastSweep
from inferno_amd.ops.sweep import HipKernelError, choose_buckets, gmem_slab_bytes
from tests.fixtures import make_spec
from tests.test_plan_gpu import (
    CELL_EXACT_KEYS,
    CELL_FLOAT_KEYS,
    assert_results_identical,
    assert_winners_identical,
    bits,
    feed_back,
    initial_cur,
)

pytestmark = pytest.mark.gpu

SCALE_TO_ZERO_SRV = 4  # min_replicas = 0, zero arrival in load 1
INFEASIBLE_SRV = 7  # ITL 1e-3, TTFT 0, as in tests/test_plan_gpu.py
DECODE_ONLY_SRV = 1  # set 4: (in_tok 0, out_tok 1)
NO_OUTPUT_SRV = 3  # set 4: out_tok 0
N_LOADED_CELLS = 27
TIERS = (512, 2048, 8192, 32768)  # upper edges of the small, medium, large and XL tiers


def build_system(analyzer_mode=None):
    system, _ = System.from_spec(make_spec(n_servers=9, seed=901, arrival_scale=6000.0))
    names = sorted(system.servers)
    assert len(names) == 9
    system.servers[names[SCALE_TO_ZERO_SRV]].min_num_replicas = 0
    srv = system.servers[names[INFEASIBLE_SRV]]
    t = system.service_classes[srv.service_class_name].targets[srv.model_name]
    t.itl = 1e-3
    t.ttft = 0.0
    if analyzer_mode is not None:
        system.analyzer_mode = analyzer_mode
    return system


def base_loads(system):
    names = sorted(system.servers)
    arrival = np.array([system.servers[n].load.arrivalRate for n in names], dtype=np.float32)
    in_tok = np.array([system.servers[n].load.avgInTokens for n in names], dtype=np.int32)
    out_tok = np.array([system.servers[n].load.avgOutTokens for n in names], dtype=np.int32)
    assert (arrival > 0).all() and (out_tok > 0).all() and (in_tok > 0).all()
    return arrival, in_tok, out_tok


def grid(cpu_comparable=False):
    """(scen [2, 9], in_tok [5, 9], out_tok [5, 9]). ``cpu_comparable`` makes
    set 4 plain out_tok = 15 everywhere."""
    arrival, in_tok, out_tok = base_loads(build_system())
    scen = np.stack([arrival, arrival * np.float32(1.7)]).astype(np.float32)
    scen[1, SCALE_TO_ZERO_SRV] = 0.0
    t_in = np.stack([in_tok, in_tok * 4, in_tok, in_tok, in_tok]).astype(np.int32)
    t_out = np.stack([out_tok, out_tok, out_tok * 4, np.full(9, 16), np.full(9, 15)])
    t_out = t_out.astype(np.int32)
    if not cpu_comparable:
        t_in[4, DECODE_ONLY_SRV], t_out[4, DECODE_ONLY_SRV] = 0, 1
        t_out[4, NO_OUTPUT_SRV] = 0
    return scen, t_in, t_out


def make_planner(analyzer_mode=None):
    system = build_system(analyzer_mode=analyzer_mode)
    fs = FastSweep(system, backend="gpu")
    assert fs.n_cells == 27
    fs.load_override = base_loads(system)
    fs.cur_override = initial_cur(system, fs)
    return fs


def oracle(scen, t_in, t_out, analyzer_mode=None):
    """The single-scenario path: per (w, s) a fresh context on an identical
    system under that slice's load, per-cell arrays first, then the winners."""
    out = {}
    for w in range(t_in.shape[0]):
        for s in range(scen.shape[0]):
            fs = make_planner(analyzer_mode)
            fs.load_override = (scen[s].copy(), t_in[w].copy(), t_out[w].copy())
            cells = fs.reconcile_cells()
            winners = fs.reconcile()
            out[w, s] = (winners, {k: v.copy() for k, v in cells.items()})
    return out


_ORACLE = {}


def cached_oracle(analyzer_mode=None):
    if analyzer_mode not in _ORACLE:
        g = grid()
        _ORACLE[analyzer_mode] = (g, oracle(*g, analyzer_mode=analyzer_mode))
    return _ORACLE[analyzer_mode]


def slice_winner(w, t, s):
    return type(w)(**{f.name: getattr(w, f.name)[t, s] for f in dataclasses.fields(w)})


def assert_token_plan_equals_oracle(res, ref, w_index=None):
    """Every slice of res against ref[(w, s)], as raw bits; w_index maps res's
    token axis to the oracle's (default: identity). An infeasible cell gets
    only its two flags written on either path, so the fp32 fields are compared
    on the feasible cells."""
    assert res.cells is not None
    n_w, n_s = res.winners.acc_idx.shape[:2]
    for w in range(n_w):
        for s in range(n_s):
            w_ref, c_ref = ref[w if w_index is None else w_index[w], s]
            where = f"slice ({w}, {s})"
            for k in CELL_EXACT_KEYS:
                assert np.array_equal(res.cells[k][w, s], c_ref[k]), f"{where}: cell {k} differs"
            feas = c_ref["feasible"].astype(bool)
            for k in CELL_FLOAT_KEYS:
                assert np.array_equal(bits(res.cells[k][w, s])[feas], bits(c_ref[k])[feas]), (
                    f"{where}: cell {k} differs"
                )
            assert_winners_identical(slice_winner(res.winners, w, s), w_ref, where)


def assert_token_results_identical(a, b):
    assert_winners_identical(a.winners, b.winners, "plan_tokens")
    assert np.array_equal(a.replicas_by_acc, b.replicas_by_acc)
    assert np.array_equal(a.cost_total, b.cost_total)
    assert np.array_equal(a.infeasible_servers, b.infeasible_servers)
    for k in CELL_EXACT_KEYS + CELL_FLOAT_KEYS:
        assert a.cells[k].tobytes() == b.cells[k].tobytes(), k


def tier_of(n):
    return int(np.searchsorted(np.asarray(TIERS), n, side="left"))


def test_fixture_covers_what_it_claims():
    (scen, t_in, t_out), ref = cached_oracle()
    fs = make_planner()
    task_n = fs._token_batch_n(scen, t_out)
    assert task_n.shape == (5, 27)
    # all five tiers, the upper edges of three of them exactly, both widths
    tiers = np.array([[tier_of(n) for n in row] for row in task_n])
    assert set(tiers.reshape(-1)) == {0, 1, 2, 3, 4}
    assert {2048, 8192, 32768} <= set(task_n[3])
    assert task_n[3].min() >= 2048 and task_n[3].max() == 32768
    assert task_n[4].max() == 262144 and task_n[4].min() == 1
    widths = {nt for nt, *_ in choose_buckets(task_n.reshape(-1))}
    assert widths == {64, 256}
    # a cell sits in different buckets in two sets
    assert (tiers != tiers[0]).any(axis=0).any()
    # the single-scenario path saw the same N (the batch of a sized cell)
    for (w, s), (_, c) in ref.items():
        sized = c["feasible"].astype(bool) & (c["rho"] > 0)
        assert np.array_equal(c["batch"][sized], task_n[w][sized]), (w, s)
    # some server's winning accelerator differs between two sets
    acc = np.stack([ref[w, 0][0].acc_idx for w in range(5)])
    assert ((acc != acc[0]) & (acc >= 0) & (acc[0] >= 0)).any()
    for (w, s), (win, c) in ref.items():
        srv = c["cell_server"]
        # the unreachable SLO: infeasible wherever the cell is loaded
        assert win.acc_idx[INFEASIBLE_SRV] == -1
        assert not c["feasible"][srv == INFEASIBLE_SRV].any()
        if s == 1:  # the zero-arrival slice of the scale-to-zero server
            assert win.acc_idx[SCALE_TO_ZERO_SRV] == -2
        else:
            assert win.acc_idx[SCALE_TO_ZERO_SRV] >= 0
    for s in range(2):
        win, c = ref[4, s]
        # (in_tok 0, out_tok 1): one decode, no prefill, a sized cell at huge N
        at = c["cell_server"] == DECODE_ONLY_SRV
        sized = at & c["feasible"].astype(bool)
        assert sized.any() and (c["batch"][sized] >= 32768).all()
        assert c["batch"][sized].max() > 32768  # a sized cell of the global-memory tier
        assert win.acc_idx[DECODE_ONLY_SRV] >= 0 and win.rho[DECODE_ONLY_SRV] > 0
        # out_tok 0 is zero traffic: min_replicas at the profile's batch, rho 0
        assert win.acc_idx[NO_OUTPUT_SRV] >= 0 and win.rho[NO_OUTPUT_SRV] == 0
        assert win.num_replicas[NO_OUTPUT_SRV] == 1


def test_every_slice_matches_single_scenario_path(monkeypatch):
    monkeypatch.delenv("INFERNO_SIZING_MEMO", raising=False)
    monkeypatch.delenv("INFERNO_PLAN_TOKENS_SLAB_BYTES", raising=False)
    (scen, t_in, t_out), ref = cached_oracle()
    fs = make_planner()
    first = fs.plan_tokens(tokens=(t_in, t_out), arrival=scen, return_cells=True)
    assert first.cells["feasible"].shape == (5, 2, 27)
    assert np.array_equal(first.arrival, scen)
    assert np.array_equal(first.in_tok, t_in) and first.in_tok.dtype == np.int32
    assert np.array_equal(first.out_tok, t_out) and first.out_tok.dtype == np.int32
    assert_token_plan_equals_oracle(first, ref)
    # totals and sums per slice
    for w in range(5):
        for s in range(2):
            acc, rep = first.winners.acc_idx[w, s], first.winners.num_replicas[w, s]
            want = np.zeros(len(fs.acc_names), dtype=np.int64)
            np.add.at(want, acc[acc >= 0], rep[acc >= 0].astype(np.int64))
            assert np.array_equal(first.replicas_by_acc[w, s], want)
            assert first.infeasible_servers[w, s] == int((acc == -1).sum())
    assert fs.memo_stats() == (0, 0)  # the pass stays off the sizing memo
    # one launch per bucket at the default slab budget
    assert all(b[5] == 0 for b in fs._gpu.tok_buckets)
    second = fs.plan_tokens(tokens=(t_in, t_out), arrival=scen, return_cells=True)
    assert_token_results_identical(first, second)


def test_single_base_set_equals_load_plan(monkeypatch):
    monkeypatch.delenv("INFERNO_SIZING_MEMO", raising=False)
    scen, t_in, t_out = grid()
    a = make_planner().plan_tokens(tokens=(t_in[:1], t_out[:1]), arrival=scen, return_cells=True)
    b = make_planner().plan(arrival=scen, return_cells=True)
    assert a.winners.acc_idx.shape == (1, 2, 9)
    flat = dataclasses.replace(
        a,
        winners=slice_first(a.winners),
        replicas_by_acc=a.replicas_by_acc[0],
        cost_total=a.cost_total[0],
        cells={k: (v[0] if k in CELL_EXACT_KEYS + CELL_FLOAT_KEYS else v)
               for k, v in a.cells.items()},
    )
    assert_results_identical(flat, b)
    for k in CELL_EXACT_KEYS + CELL_FLOAT_KEYS:  # all bytes, infeasible cells included
        assert flat.cells[k].tobytes() == b.cells[k].tobytes(), k
    assert np.array_equal(a.infeasible_servers[0], b.infeasible_servers)
    assert np.array_equal(a.arrival, b.arrival)


def slice_first(w):
    return type(w)(**{f.name: getattr(w, f.name)[0] for f in dataclasses.fields(w)})


def test_reconcile_plan_tokens_reconcile(monkeypatch):
    """A token plan between two reconciles changes neither, moves no memo
    counter, costs the second one no memo miss and leaves the context's
    reconcile layout as it was."""
    monkeypatch.delenv("INFERNO_SIZING_MEMO", raising=False)
    (scen, t_in, t_out), ref = cached_oracle()

    def run(with_plan):
        fs = make_planner()
        arrival, in_tok, out_tok = fs.load_override
        cur = fs.cur_override
        w1 = fs.reconcile()
        p = None
        if with_plan:
            stats, fused, stale = fs.memo_stats(), fs._gpu.fused_state(), fs._gpu.stale_ticks
            key = fs._gpu.bucket_key
            p = fs.plan_tokens(tokens=(t_in, t_out), arrival=scen, return_cells=True)
            assert fs.memo_stats() == stats
            assert fs._gpu.fused_state() == fused
            assert fs._gpu.stale_ticks == stale and fs._gpu.bucket_key == key
        before = fs.memo_stats()
        fs.load_override = ((arrival * np.float32(1.7)).astype(np.float32), in_tok, out_tok)
        fs.cur_override = feed_back(cur, w1)
        w2 = fs.reconcile()
        after = fs.memo_stats()
        return w1, p, w2, (after[0] - before[0], after[1] - before[1]), fs._gpu.stale_ticks

    w1, p, w2, moved, stale = run(True)
    t1, _, t2, moved_twin, stale_twin = run(False)
    assert_winners_identical(w1, t1, "first reconcile")
    assert_winners_identical(w2, t2, "second reconcile")
    assert moved == moved_twin == (N_LOADED_CELLS, 0)  # every loaded cell hits
    assert stale == stale_twin == 1  # only the context's first tick found no layout
    assert_winners_identical(slice_winner(p.winners, 0, 0), w1, "base slice")
    assert_token_plan_equals_oracle(p, ref)


def test_mg1_mode(monkeypatch):
    monkeypatch.delenv("INFERNO_SIZING_MEMO", raising=False)
    (scen, t_in, t_out), ref = cached_oracle("mg1")
    fs = make_planner(analyzer_mode="mg1")
    cold = fs.plan_tokens(tokens=(t_in, t_out), arrival=scen, return_cells=True)
    assert_token_plan_equals_oracle(cold, ref)
    again = fs.plan_tokens(tokens=(t_in, t_out), arrival=scen, return_cells=True)
    assert_token_results_identical(cold, again)


def test_slab_budget_slices_the_huge_bucket(monkeypatch):
    """A budget of two tasks' slabs: the huge tier runs in consecutive slices
    over one allocation, with the same bytes as in one launch."""
    monkeypatch.delenv("INFERNO_SIZING_MEMO", raising=False)
    (scen, t_in, t_out), ref = cached_oracle()
    task_n = make_planner()._token_batch_n(scen, t_out).reshape(-1)
    huge = [b for b in choose_buckets(task_n) if b[4]]
    assert len(huge) == 1
    nt, _, bmax, count, _ = huge[0]
    assert count >= 3 and bmax == 262144
    per_task = gmem_slab_bytes(bmax, nt)
    monkeypatch.setenv("INFERNO_PLAN_TOKENS_SLAB_BYTES", str(2 * per_task + 1))
    fs = make_planner()
    res = fs.plan_tokens(tokens=(t_in, t_out), arrival=scen, return_cells=True)
    sliced = [b for b in fs._gpu.tok_buckets if b[5] > 0]
    assert len(sliced) == 1 and sliced[0][5] == 2 and sliced[0][3] == count
    assert sliced[0][4][0].shape[0] == 2  # slabs for one slice only
    assert_token_plan_equals_oracle(res, ref)
    # a single task above the budget is refused, naming the bytes it needs
    monkeypatch.setenv("INFERNO_PLAN_TOKENS_SLAB_BYTES", str(per_task - 1))
    small = make_planner()
    with pytest.raises(HipKernelError, match=str(per_task)):
        small.plan_tokens(tokens=(t_in, t_out), arrival=scen)
    # ...and the context still plans what fits
    ok = small.plan_tokens(tokens=(t_in[:4], t_out[:4]), arrival=scen, return_cells=True)
    assert_token_plan_equals_oracle(ok, ref)


def test_growing_grid_and_validation(monkeypatch):
    monkeypatch.delenv("INFERNO_SIZING_MEMO", raising=False)
    monkeypatch.delenv("INFERNO_PLAN_TOKENS_SLAB_BYTES", raising=False)
    (scen, t_in, t_out), ref = cached_oracle()
    fs = make_planner()
    one = fs.plan_tokens(tokens=(t_in[3:4], t_out[3:4]), return_cells=True)  # arena for W = 1
    assert one.winners.acc_idx.shape == (1, 1, 9)
    assert_token_plan_equals_oracle(one, ref, w_index=(3,))
    res = fs.plan_tokens(tokens=(t_in, t_out), arrival=scen, return_cells=True)  # ...grown to 5
    assert_token_plan_equals_oracle(res, ref)
    two = fs.plan_tokens(tokens=(t_in[:2], t_out[:2]), arrival=scen, return_cells=True)  # reused
    assert_token_plan_equals_oracle(two, ref, w_index=(0, 1))
    stats, key = fs.memo_stats(), fs._gpu.tok_bucket_key
    calls = []
    monkeypatch.setattr(fs._gpu, "plan_tokens", lambda *a, **k: calls.append(a))
    for kwargs in (
        {},
        {"tokens": (t_in, t_out), "token_scales": [(1.0, 1.0)]},
        {"tokens": (t_in[:, :8], t_out[:, :8])},
        {"tokens": (t_in, t_out[:4])},
        {"tokens": (t_in, -t_out)},
        {"tokens": (np.repeat(t_in, 52, axis=0)[:257], np.repeat(t_out, 52, axis=0)[:257])},
        {"tokens": (np.repeat(t_in, 26, axis=0)[:129], np.repeat(t_out, 26, axis=0)[:129]),
         "arrival": scen},  # 258 slices
        {"token_scales": [(1.0, 0.0)]},
        {"token_scales": [(1.0, float("nan"))]},
        {"token_scales": [(1.0, -2.0)]},
        {"token_scales": [1.0, 2.0]},
        {"tokens": (t_in, t_out), "scales": [1.0, -1.0]},
    ):
        with pytest.raises(ValueError):
            fs.plan_tokens(**kwargs)
    assert calls == []  # nothing was launched
    assert fs.memo_stats() == stats and fs._gpu.tok_bucket_key == key


def test_gpu_plan_tokens_matches_cpu_plan_tokens():
    """GPU plan_tokens against the golden CPU plan_tokens under the rule of
    tests/test_plan_slo_gpu.py::test_gpu_plan_slo_matches_cpu_plan_slo: equal
    accelerators; replica counts may differ by one (a ceil boundary inside the
    bisection tolerance) for at most max(1, n // 50) = 1 of the n = 90 (server,
    slice) winners; that test's field tolerances for the rest. Sets 0-3 and
    out_tok = 15 everywhere: the (in_tok 0, out_tok 1) server, whose N reaches
    262144, stays with the bitwise oracle, since nothing compares the CPU path
    at that size.

    Observed on MI355X: 0 of 90 winners flipped."""
    scen, t_in, t_out = grid(cpu_comparable=True)
    g = make_planner().plan_tokens(tokens=(t_in, t_out), arrival=scen).winners
    cpu_system = build_system()
    cpu = FastSweep(cpu_system, backend="cpu")
    c = cpu.plan_tokens(tokens=(t_in, t_out), arrival=scen).winners
    assert np.array_equal(g.acc_idx, c.acc_idx)
    n = g.acc_idx.size
    assert n == 90
    flips = 0
    for at in np.ndindex(g.acc_idx.shape):
        where = f"(token set, load, server) {at}"
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
