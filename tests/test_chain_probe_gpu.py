"""The production chain path on the GPU (ops.sweep.run_chain_probe: the
fp32-reciprocal geometry, chain_eval<NT, 1>, chain_eval<NT, 2>, dual_bisect<NT>
and wva_size_cell<NT>) against the 60-digit scheme oracle of
tests/test_chain_probe_cpu.py, at every block width and both geometry tiers,
on shapes that reach each unrolled loop of the recurrence, clipped and empty
chunks, the second anchor of a chunk and the reduction scratch of 16 waves.

Tolerance of the evaluations: TOL = max(8 x GOLDEN_MAX_ERR, 1e-13) relative (the
wait as |d wait| / resp): 8 x the fp64 error the CPU golden shows against the
exact chain on the same grid; the device sums the same number of terms in a
different order.

Measured on the MI355X: largest error of an evaluation 1.81e-11 (N = 1023 on 64
threads, at s(N) (1 - 1e-9)); 2.9e-14 at N = 1; TOL is 2.1e-10. The metric at
a sized rate misses its target by at most 5.9e-7 of it (bound 1e-6 + TOL).
"""
import numpy as np
import pytest
import torch

from inferno_amd.ops.sweep import run_chain_probe
from tests.test_chain_probe_cpu import (CELLS, FIELDS, GOLDEN_MAX_ERR, IN_TOK, OUT_TOK, PERF,
                                        WVA_TOL, analyzer, bisect_targets, cell_id, golden_search,
                                        grid_rates, mpf, oracle, rel_errors)

pytestmark = pytest.mark.gpu

TOL = max(8.0 * GOLDEN_MAX_ERR, 1e-13)
TPS_CELLS = ((64, 257, False), (512, 2049, False))  # these size under a TPS target too


def rate_pairs(n):
    """Half-block pairs of a cell: neighbours of the grid in both orders,
    (lam_min, lam_max) in both orders, and every rate against itself."""
    r = grid_rates(n)
    cyc = [(r[i], r[(i + 1) % len(r)]) for i in range(len(r))]
    return cyc + [(b, a) for a, b in cyc] + [(r[0], r[4]), (r[4], r[0])] + [(a, a) for a in r]


_RUN = {}


def probe(cell):
    """One launch per cell, shared by the tests."""
    if cell not in _RUN:
        nt, n, gmem = cell
        i32 = lambda v: torch.full((1,), v, dtype=torch.int32)  # noqa: E731
        f32 = lambda v: torch.full((1,), v, dtype=torch.float32)  # noqa: E731
        arrays = {k: f32(v) for k, v in PERF.items()}
        arrays.update(in_tok=i32(IN_TOK), out_tok=i32(OUT_TOK), batch_n=i32(n),
                      t_tps=f32(100.0 if cell in TPS_CELLS else 0.0))
        _RUN[cell] = run_chain_probe(arrays, lam=[grid_rates(n)], lam_pairs=[rate_pairs(n)],
                                     targets=bisect_targets(n)[None], nt=nt, gmem=gmem)
    return _RUN[cell]


@pytest.mark.parametrize("cell", CELLS, ids=cell_id)
def test_evaluations_match_scheme_oracle(cell):
    nt, n, _ = cell
    out, orc = probe(cell), oracle(n)
    worst = 0.0
    for i, lam in enumerate(grid_rates(n)):
        err = rel_errors(out["ev1"][0, i], orc.solve(lam, nt))
        worst = max(worst, *err)
        assert max(err) <= TOL, ("whole block", lam, dict(zip(FIELDS, err)))
    for i, pair in enumerate(rate_pairs(n)):
        for h, lam in enumerate(pair):
            err = rel_errors(out["ev2"][0, i, h], orc.solve(lam, nt))
            worst = max(worst, *err)
            assert max(err) <= TOL, ("half", h, pair, dict(zip(FIELDS, err)))
    print(f"{cell_id(cell)}: device max error {worst:.3e} (TOL {TOL:.1e})")


@pytest.mark.parametrize("cell", CELLS, ids=cell_id)
def test_halves_agree_bit_for_bit(cell):
    out = probe(cell)
    same = [i for i, (a, b) in enumerate(rate_pairs(cell[1])) if a == b]
    assert len(same) == 7
    ev2 = out["ev2"][0, same]
    assert not np.isnan(ev2).any()
    assert np.array_equal(ev2[:, 0].view(np.uint64), ev2[:, 1].view(np.uint64))


@pytest.mark.parametrize("cell", CELLS, ids=cell_id)
def test_bisection_and_sizing(cell):
    nt, n, _ = cell
    out, orc, qa = probe(cell), oracle(n), analyzer(n)
    lam_max = float(qa.serv_rate[-1]) * (1.0 - 1e-3)
    tg = bisect_targets(n)
    for k in range(len(tg)):
        active = [bool(tg[k, kind] > 0) for kind in (0, 1)]
        for kind in (0, 1):
            lam, ind = float(out["lam_star"][0, k, kind]), int(out["ind"][0, k, kind])
            if not active[kind]:
                assert (lam, ind) == (lam_max, 0)
                continue
            target = float(tg[k, kind])
            assert ind == golden_search(n, kind, target)[1], (k, kind)
            if ind == 0:
                got = orc.metric(kind, lam, nt)
                miss = float(abs(got - mpf(target)))
                print(f"{cell_id(cell)} row {k} kind {kind}: |metric - target| / target = "
                      f"{miss / target:.3e}")
                assert miss <= WVA_TOL * target + TOL * target, (k, kind, lam)
        ok = not any(active[kind] and out["ind"][0, k, kind] < 0 for kind in (0, 1))
        assert bool(out["verdict"][0, k]) == ok, k
        if ok:
            lam_tps = lam_max * (1.0 - 0.1) if cell in TPS_CELLS else lam_max
            lam = min(float(out["lam_star"][0, k, 0]) if active[0] else lam_max,
                      float(out["lam_star"][0, k, 1]) if active[1] else lam_max, lam_tps)
            want = orc.solve(lam, nt)["throughput"]
            assert float(abs(mpf(float(out["tput"][0, k])) - want) / want) <= TOL, k
        else:
            assert np.isnan(out["tput"][0, k])


def test_rates_outside_the_domain_store_nan():
    cell = CELLS[5]
    nt, n, gmem = cell
    s_n = float(analyzer(n).serv_rate[-1])
    arrays = {k: torch.full((1,), v, dtype=torch.float32) for k, v in PERF.items()}
    arrays.update({k: torch.full((1,), v, dtype=torch.int32)
                   for k, v in dict(in_tok=IN_TOK, out_tok=OUT_TOK, batch_n=n).items()},
                  t_tps=torch.zeros(1))
    lam = [[0.0, -1.0, float(np.nextafter(s_n, 1.0)), float("nan"), 0.5 * s_n]]
    pairs = [[(0.5 * s_n, 2.0 * s_n), (0.0, 0.5 * s_n), (0.5 * s_n, 0.25 * s_n)]]
    out = run_chain_probe(arrays, lam=lam, lam_pairs=pairs, nt=nt, gmem=gmem)
    assert np.isnan(out["ev1"][0, :4]).all() and np.isfinite(out["ev1"][0, 4]).all()
    assert np.isnan(out["ev2"][0, :2]).all() and np.isfinite(out["ev2"][0, 2]).all()
    # the default dispatch (choose_buckets) runs this cell at the same width
    auto = run_chain_probe(arrays, lam=lam)
    assert np.array_equal(auto["ev1"][0, 4].view(np.uint64), out["ev1"][0, 4].view(np.uint64))
    # degenerate rates: NaN and indicator -2
    arrays["alpha"] = torch.zeros(1)
    arrays["beta"] = torch.zeros(1)
    arrays["gamma"] = torch.zeros(1)
    arrays["delta"] = torch.zeros(1)
    bad = run_chain_probe(arrays, lam=lam, targets=[[(10.0, 10.0)]], nt=nt)
    assert np.isnan(bad["ev1"]).all() and (bad["ind"] == -2).all() and not bad["verdict"].any()
