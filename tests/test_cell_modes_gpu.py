"""The planning modes of the sweep cell function (FastSweep.plan, plan_slo) where
the production-tier planning tests do not go: every exit of the cell function,
the degenerate-rate one included, and the override-only block widths.

Every (target set, load) slice must be bit for bit what the single-scenario
path computes: reconcile_cells() then reconcile() of a fresh FastSweep on the
same fleet with that slice's targets on its Target objects and that slice's
arrival rates as the load.

Fleets are the small-tier ones of tests/test_fused_tick_gpu.py: 8 servers x 3
accelerators, batch sizes cycling through 5, 200, 600, 16 and 1500 (one wave,
256 threads, XL, one wave again, global-memory slab).
"""
import numpy as np
import pytest

from tests.test_fused_tick_gpu import (
    DEGENERATE,
    HUGE,
    INFEASIBLE,
    LARGE,
    MED,
    NO_OUT,
    SMALL,
    XL,
    ZERO_EMPTY,
    ZERO_KEEP,
    exits_stat_tweak,
    exits_tweak,
    loads_of,
    make_fs,
    no_cur,
    patch_tiers,
)
from tests.test_plan_gpu import (
    assert_plan_equals_oracle,
    assert_results_identical,
    n_lookup_cells,
)
from tests.test_plan_slo_gpu import (
    assert_slo_plan_equals_oracle,
    assert_slo_results_identical,
    targets_of,
)

pytestmark = pytest.mark.gpu

N_SERVERS = 8
CELL_N = [SMALL, LARGE, XL, MED, HUGE]
LOAD_SCALES = (1.0, 0.0, 1.7)
# 0.125 and not 0.25: by the CPU golden (create_allocation per cell), 0.25 and
# 0.5 only take this fleet's server 6 from two feasible cells to none, while at
# 0.125 servers 4 and 5 each lose cells and keep a candidate (asserted on the
# GPU oracle below)
SLO_SCALES = (1.0, 0.125)
ZERO_ONCE = 5  # explicit arrival: zero in the last load scenario only


def exits_load(system, fs):
    arrival, in_tok, out_tok = loads_of(system, fs)
    arrival, out_tok = arrival.copy(), out_tok.copy()
    arrival[ZERO_KEEP] = 0.0
    arrival[ZERO_EMPTY] = 0.0
    out_tok[NO_OUT] = 0
    return arrival, in_tok, out_tok


def base_targets(system):
    t = targets_of(system)
    return (np.array([x.ttft for x in t], dtype=np.float32),
            np.array([x.itl for x in t], dtype=np.float32))


def oracle_slice(t_ttft, t_itl, load, **kw):
    """The single-scenario path on a fresh context: per-cell arrays first (miss
    path), then the winners."""
    # (the targets go in through the tweak: they are read when the FastSweep is built)
    _, fs = make_fs(N_SERVERS, CELL_N,
                    **dict(kw, tweak=_with_targets(kw.get("tweak"), t_ttft, t_itl)))
    fs.load_override = load
    fs.cur_override = no_cur(fs)
    cells = fs.reconcile_cells()
    winners = fs.reconcile()
    return winners, {k: v.copy() for k, v in cells.items()}


def _with_targets(tweak, t_ttft, t_itl):
    def apply(system):
        if tweak is not None:
            tweak(system)
        for i, tgt in enumerate(targets_of(system)):
            tgt.ttft, tgt.itl = float(t_ttft[i]), float(t_itl[i])
    return apply


def make_planner(load_of, **kw):
    system, fs = make_fs(N_SERVERS, CELL_N, **kw)
    fs.load_override = load_of(system, fs)
    fs.cur_override = no_cur(fs)
    return system, fs


def scaled(v, scales):
    return np.stack([v * np.float32(sc) for sc in scales]).astype(np.float32)


def test_every_exit_in_planning_modes(monkeypatch):
    """Zero-load keep-min, zero-load scale-to-zero, out_tok = 0, unreachable
    SLO, degenerate rates and sized cells, through plan and plan_slo, memo-cold
    and memo-warm."""
    monkeypatch.delenv("INFERNO_SIZING_MEMO", raising=False)
    patch_tiers(monkeypatch)
    kw = dict(tweak=exits_tweak, stat_tweak=exits_stat_tweak)
    system, fs = make_planner(exits_load, **kw)
    arrival, in_tok, out_tok = fs.load_override
    ttft, itl = base_targets(system)
    t_ttft, t_itl = scaled(ttft, SLO_SCALES), scaled(itl, SLO_SCALES)
    scen = scaled(arrival, LOAD_SCALES)
    scen_slo = scen.copy()
    assert scen_slo[2, ZERO_ONCE] > 0
    scen_slo[2, ZERO_ONCE] = 0.0

    # the oracle: target set 0 at the plan's loads, both target sets at plan_slo's
    ref_plan = [oracle_slice(t_ttft[0], t_itl[0], (scen[s].copy(), in_tok, out_tok), **kw)
                for s in range(len(LOAD_SCALES))]
    ref_slo = {}
    for t in range(len(SLO_SCALES)):
        for s in range(len(LOAD_SCALES)):
            if t == 0 and s < 2:
                ref_slo[t, s] = ref_plan[s]  # the same targets and loads
            else:
                ref_slo[t, s] = oracle_slice(t_ttft[t], t_itl[t],
                                             (scen_slo[s].copy(), in_tok, out_tok), **kw)

    # the fixture takes the exits it claims to
    seg = fs.seg_start
    for (t, s), (w, c) in ref_slo.items():
        feas, zero = c["feasible"].astype(bool), c["zero_empty"].astype(bool)
        assert feas[seg[ZERO_KEEP]:seg[ZERO_KEEP + 1]].all()
        assert not zero[seg[ZERO_KEEP]:seg[ZERO_KEEP + 1]].any()
        assert zero[seg[ZERO_EMPTY]:seg[ZERO_EMPTY + 1]].all() and w.acc_idx[ZERO_EMPTY] == -2
        assert feas[seg[NO_OUT]:seg[NO_OUT + 1]].all()
        if LOAD_SCALES[s] == 0.0:
            assert feas.all()  # the zero-traffic decision comes first
            continue
        assert not feas[seg[INFEASIBLE]:seg[INFEASIBLE + 1]].any()
        assert w.acc_idx[INFEASIBLE] == -1
        assert not feas[seg[DEGENERATE] + 1]
        assert (feas & ~zero & (c["rho"] > 0)).any(), "no sized cell"
    once = slice(seg[ZERO_ONCE], seg[ZERO_ONCE + 1])
    assert (ref_slo[0, 2][1]["rho"][once] == 0).all() and (ref_slo[0, 0][1]["rho"][once] > 0).all()
    # the tighter target set: cells infeasible while their server keeps a candidate
    (w_q, c_q), c_1 = ref_slo[1, 0], ref_slo[0, 0][1]
    lost = c_1["feasible"].astype(bool) & ~c_q["feasible"].astype(bool)
    assert (lost & (w_q.acc_idx[fs.cell_server] >= 0)).any()

    n_plan = n_lookup_cells(fs, scen, out_tok)
    n_slo = n_lookup_cells(fs, scen_slo, out_tok)
    assert n_plan == n_slo == 3 * (N_SERVERS - 3)

    assert fs.memo_stats() is None  # no context yet
    cold = fs.plan(scales=LOAD_SCALES, return_cells=True)
    assert np.array_equal(cold.arrival, scen)
    assert_plan_equals_oracle(cold, ref_plan)
    assert fs.memo_stats() == (0, n_plan)
    warm = fs.plan(scales=LOAD_SCALES, return_cells=True)
    assert fs.memo_stats() == (n_plan, n_plan)
    assert_plan_equals_oracle(warm, ref_plan)
    assert_results_identical(cold, warm)

    _, fs = make_planner(exits_load, **kw)
    cold = fs.plan_slo(slo_scales=SLO_SCALES, arrival=scen_slo, return_cells=True)
    assert np.array_equal(cold.arrival, scen_slo)
    assert_slo_plan_equals_oracle(cold, ref_slo)
    assert fs.memo_stats() == (0, n_slo)
    warm = fs.plan_slo(slo_scales=SLO_SCALES, arrival=scen_slo, return_cells=True)
    assert fs.memo_stats() == (n_slo, n_slo)
    assert_slo_plan_equals_oracle(warm, ref_slo)
    assert_slo_results_identical(cold, warm)
    # no target set at the base targets: the memo is neither read nor written
    fs.plan_slo(slo_scales=SLO_SCALES[1:], arrival=scen_slo)
    assert fs.memo_stats() == (n_slo, n_slo)


@pytest.mark.parametrize("env,nt", [
    ("INFERNO_NT_SMALL", 128),
    ("INFERNO_NT_LARGE", 512),
    ("INFERNO_NT_LARGE", 1024),
    ("INFERNO_NT_HUGE", 1024),
])
def test_planning_modes_at_override_widths(monkeypatch, env, nt):
    """The planning kernels at the widths only an override selects, against
    the single-scenario path under the same override (the width is part of the
    memo key and of the reduction order)."""
    monkeypatch.delenv("INFERNO_SIZING_MEMO", raising=False)
    patch_tiers(monkeypatch)
    monkeypatch.setenv(env, str(nt))
    slo_scales, load_scales = (1.0, 0.5), (1.0, 1.7)
    system, fs = make_planner(loads_of)
    arrival, in_tok, out_tok = fs.load_override
    ttft, itl = base_targets(system)
    t_ttft, t_itl = scaled(ttft, slo_scales), scaled(itl, slo_scales)
    scen = scaled(arrival, load_scales)
    ref = {(t, s): oracle_slice(t_ttft[t], t_itl[t], (scen[s].copy(), in_tok, out_tok))
           for t in range(2) for s in range(2)}
    assert any(c["feasible"].any() for _, c in ref.values())

    res = fs.plan_slo(slo_scales=slo_scales, scales=load_scales, return_cells=True)
    assert_slo_plan_equals_oracle(res, ref)
    _, fs = make_planner(loads_of)
    res = fs.plan(scales=load_scales, return_cells=True)
    assert_plan_equals_oracle(res, [ref[0, 0], ref[0, 1]])
