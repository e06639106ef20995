"""Percentile TTFT planning, CPU golden: QueueAnalyzer.wait_tail / size_tail and
FastSweep.plan_tail(backend="cpu").

The reference is a 60-digit mpmath evaluation of
    sum_j w[N+j] Q(j+1, x) / (sum w - w[K]),  x = s(N) t,
with w[0] = 1, w[n] = w[n-1] lam / s(min(n, N)) from the exact fp32 rates.
Q(j+1, x) = e^-x sum_{i<=j} x^i / i! is summed in mpmath by the recurrence (a
gammainc call per term takes minutes at N = 2049) and checked against
mpmath.gammainc(j+1, x, inf, regularized=True) at the first, middle and last j
of every grid point.

Largest absolute error of the golden on the grid, measured here: 8.81e-14
(N = 600, lam_max, x = Q/2). GOLDEN_MAX_ERR below is
that figure; the GPU probe's tolerance is 8 x it (tests/test_plan_tail_gpu.py).
"""
import math

import mpmath
import numpy as np
import pytest

from inferno_amd.analyzer import (AnalyzerError, Configuration, DecodeParms, PrefillParms,
                                  QueueAnalyzer, RequestSize, ServiceParms, TargetPerf)
from inferno_amd.core.system import System
from inferno_amd.engine import FastSweep
from inferno_amd.utils.synthetic import make_fleet_spec

mpmath.mp.dps = 60

GRID_N = (1, 2, 33, 64, 600, 2049)
PERF = dict(alpha=8.0, beta=0.05, gamma=5.0, delta=0.02)
IN_TOK, OUT_TOK = 512, 128
GOLDEN_MAX_ERR = 8.9e-14  # measured by test_golden_matches_mpmath (see above)


def analyzer(n):
    cfg = Configuration(n, 10 * n, ServiceParms(PrefillParms(PERF["gamma"], PERF["delta"]),
                                               DecodeParms(PERF["alpha"], PERF["beta"])))
    return QueueAnalyzer(cfg, RequestSize(IN_TOK, OUT_TOK))


def grid_points(qa):
    """(lam, t) of the grid for one analyzer: lam_min, 0.5 s(N), lam_max times
    t < 0, t = 0, x < 1, x = Q/2, x beyond Q plus the window."""
    mu = float(qa.serv_rate[-1])
    q = qa.chain.K - qa.chain.N
    xs = (-1.0, 0.0, 0.5, q / 2.0, q + 40.0 + 12.0 * math.sqrt(q))
    return [(lam, x / mu) for lam in (qa.rate_min / 1000.0, 0.5 * mu, qa.rate_max / 1000.0)
            for x in xs]


def mp_tail(qa, lam, t):
    """The 60-digit reference tail(lam, t)."""
    n, k = qa.chain.N, qa.chain.K
    nq = k - n
    if t < 0:
        return mpmath.mpf(1)
    s = [mpmath.mpf(float(v)) for v in qa.serv_rate]
    lam = mpmath.mpf(lam)
    w = [mpmath.mpf(1)]
    for i in range(1, k + 1):
        w.append(w[-1] * lam / s[min(i, n) - 1])
    x = s[-1] * mpmath.mpf(t)
    pmf = cdf = mpmath.exp(-x)
    total = mpmath.mpf(0)
    check = {0, nq // 2, nq - 1}
    for j in range(nq):
        if j in check:
            assert abs(cdf - mpmath.gammainc(j + 1, x, mpmath.inf, regularized=True)) < 1e-50
        total += w[n + j] * cdf
        pmf = pmf * x / (j + 1)
        cdf += pmf
    return total / (sum(w) - w[k])


_REF = {}


def reference(n):
    """(analyzer, [(lam, t, reference tail)]) of grid size n, computed once."""
    if n not in _REF:
        qa = analyzer(n)
        _REF[n] = (qa, [(lam, t, mp_tail(qa, lam, t)) for lam, t in grid_points(qa)])
    return _REF[n]


@pytest.mark.parametrize("n", GRID_N)
def test_golden_matches_mpmath(n):
    qa, points = reference(n)
    worst = max(float(abs(mpmath.mpf(qa.wait_tail(lam, t)) - ref)) for lam, t, ref in points)
    print(f"N={n}: golden max abs error {worst:.3e}")
    assert worst <= GOLDEN_MAX_ERR


@pytest.mark.parametrize("n", (1, 33, 600))
def test_wait_distribution_properties(n):
    qa = analyzer(n)
    mu = float(qa.serv_rate[-1])
    lams = np.linspace(qa.rate_min / 1000.0, qa.rate_max / 1000.0, 7)
    ts = np.array([-1.0, 0.0, 0.3, 2.0, 10.0 * n, 40.0 * n]) / mu
    grid = np.array([[qa.wait_tail(lam, t) for t in ts] for lam in lams])
    assert (np.diff(grid, axis=1) <= 1e-15).all()  # non-increasing in t
    assert (np.diff(grid, axis=0) >= -1e-15).all()  # non-decreasing in lam
    # the mean of the distribution is the analyzer's avg_wait_time
    # (avg_wait_time is a difference of response and service time: its own
    # rounding is a few ulps of the service time)
    lam = qa.rate_max / 1000.0
    st = qa.chain.solve(lam)
    j = np.arange(qa.chain.K - n)
    mean = np.sum(st.pN * (lam / mu) ** j * (j + 1)) / mu / (1.0 - st.pK)
    assert mean == pytest.approx(st.avg_wait_time, rel=1e-9, abs=1e-13 * st.avg_resp_time)


def test_size_tail_monotone_and_validation():
    qa = analyzer(64)
    targets = TargetPerf(target_ttft=qa.service_parms.prefill.prefill_time(IN_TOK, 64) + 150.0,
                         target_itl=30.0)
    rates = [qa.size_tail(targets, q)[1].throughput for q in (0.5, 0.9, 0.99, 0.999)]
    assert rates == sorted(rates, reverse=True) and rates[0] > rates[-1]
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(AnalyzerError):
            qa.size_tail(targets, bad)
    # a budget that is negative at every rate is infeasible, not "above"
    with pytest.raises(AnalyzerError):
        qa.size_tail(TargetPerf(target_ttft=1.0), 0.5)


def fleet(n_servers=6, seed=11):
    system, _ = System.from_spec(make_fleet_spec(n_servers, seed=seed))
    return system


def test_plan_tail_cpu_is_a_loop_of_size_tail():
    from inferno_amd.core.allocation import create_allocation

    system = fleet()
    fs = FastSweep(system, backend="cpu")
    qs, scales = (0.5, 0.95), (1.0, 2.0)
    res = fs.plan_tail(qs, scales=scales)
    assert res.winners.num_replicas.shape == (2, 2, len(fs.server_names))
    base = {n: system.servers[n].load.arrivalRate for n in fs.server_names}
    for k, q in enumerate(qs):
        for s, sc in enumerate(scales):
            for i, name in enumerate(fs.server_names):
                system.servers[name].load.arrivalRate = float(np.float32(base[name])
                                                              * np.float32(sc))
                allocs = [create_allocation(system, name, a, ttft_quantile=q)
                          for a in sorted(system.servers[name].candidate_accelerators(system))]
                allocs = [a for a in allocs if a is not None]
                system.servers[name].load.arrivalRate = base[name]
                if not allocs:
                    assert res.winners.acc_idx[k, s, i] == -1
                    continue
                best = min(allocs, key=lambda a: a.value)
                assert res.winners.num_replicas[k, s, i] == best.num_replicas
                assert res.wait_tail[k, s, i] == np.float32(best.wait_tail)
                if best.num_replicas > 0:
                    assert best.wait_tail <= (1.0 - q) * (1.0 + 1e-6)
    # more replicas (never fewer) as q rises
    assert (res.winners.num_replicas[1] >= res.winners.num_replicas[0]).all()


def test_plan_tail_validation():
    fs = FastSweep(fleet(), backend="cpu")
    for bad in ((), (0.0,), (1.0,), (0.5, float("nan")), (0.5,) * 9, "x"):
        with pytest.raises(ValueError):
            fs.plan_tail(bad)
    with pytest.raises(ValueError):
        fs.plan_tail((0.5,) * 8, scales=np.linspace(0.5, 2.0, 33))  # 264 pairs
    system = fleet()
    system.analyzer_mode = "mg1"
    with pytest.raises(ValueError):
        FastSweep(system, backend="cpu").plan_tail((0.9,))
