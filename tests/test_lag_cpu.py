"""Lag analysis, CPU golden: analyzer/lag.py and FastSweep.lag(backend="cpu").

The reference is the same uniformization sum in np.longdouble with L = 80 and
Poisson weights normalised over the window (no lgamma), cross-checked against
scipy.linalg.expm of the dense generator at N in {1, 2, 33}.

Largest absolute error of the golden on the grid over blocked, rho and
wait * s(N) / Q, measured here: 7.55e-14 (N = 64, 3 lam_max). GOLDEN_MAX_ERR
is 7.6e-14; the GPU probe's tolerance is max(8 x it, 1e-12)
(tests/test_lag_gpu.py).
"""
import numpy as np
import pytest

from inferno_amd.analyzer import (Configuration, DecodeParms, PrefillParms, QueueAnalyzer,
                                  RequestSize, ServiceParms)
from inferno_amd.analyzer.lag import lag_latency, lag_transient
from inferno_amd.core import System
from inferno_amd.engine import (LAG_BUDGET, LAG_IDLE, LAG_INVALID, LAG_NO_REPLICAS, LAG_NOT_HELD,
                                LAG_OK, LAG_TOO_WIDE, FastSweep)
from tests.fixtures import make_spec

PERF = dict(alpha=8.0, beta=0.05, gamma=5.0, delta=0.02)
IN_TOK, OUT_TOK = 512, 128
GOLDEN_MAX_ERR = 7.6e-14  # measured by test_golden_matches_longdouble (see above)
LD = np.longdouble


def analyzer(n):
    cfg = Configuration(n, 10 * n, ServiceParms(PrefillParms(PERF["gamma"], PERF["delta"]),
                                               DecodeParms(PERF["alpha"], PERF["beta"])))
    return QueueAnalyzer(cfg, RequestSize(IN_TOK, OUT_TOK))


def chain(rates, lam):
    """(up, dn) per state 0..K of the chain at arrival rate lam, longdouble."""
    n = len(rates)
    s = np.concatenate(([0], rates.astype(LD), np.full(10 * n, LD(rates[-1]))))
    up = np.full(11 * n + 1, LD(lam))
    up[-1] = 0
    return up, s


def reference(rates, lam0, lam1, dt_ms, big_l=80.0):
    """[T, 3]: blocked, rho, wait * s(N) / Q in longdouble."""
    n = len(rates)
    k, q = 11 * n, 10 * n
    up0, s = chain(rates, lam0)
    w = np.concatenate(([LD(1)], np.cumprod(up0[:-1] / s[1:]))) if lam0 > 0 else np.eye(1, k + 1)[0]
    v = (w / w.sum()).astype(LD)
    up, _ = chain(rates, lam1)
    unif = LD(lam1) + s.max()
    up, dn = up / unif, s / unif
    stay = 1 - up - dn
    out = []
    for dt in dt_ms:
        x = unif * LD(dt)
        lo = max(int(np.floor(x - np.sqrt(2 * x * big_l))), 0)
        hi = int(np.ceil(x + big_l / 3 + np.sqrt(big_l * big_l / 9 + 2 * x * big_l)))
        js = np.arange(lo, hi + 1).astype(LD)
        log_fact = np.concatenate(([0], np.cumsum(np.log(np.arange(1, hi + 1, dtype=LD)))))
        logw = js * np.log(x) - log_fact[lo:]
        wts = np.exp(logw - logw.max())
        wts /= wts.sum()  # the window holds all but e^-80 of the weight
        acc = np.zeros_like(v)
        for j in range(hi + 1):
            if j >= lo:
                acc += wts[j - lo] * v
            nv = v * stay
            nv[1:] += v[:-1] * up[:-1]
            nv[:-1] += v[1:] * dn[1:]
            v = nv
        v = acc
        wait = np.dot(v[n:k], np.arange(1, q + 1).astype(LD)) / (1 - v[k]) / q
        out.append((v[k], np.dot(v, np.minimum(np.arange(k + 1), n)) / n, wait))
    return np.array(out, dtype=LD)


def normalised(raw, rates):
    n = len(rates)
    return np.stack([raw[:, 0], raw[:, 1] / n, raw[:, 4] * float(rates[-1]) / (10 * n)], axis=1)


GRID = [(n, f0, f1) for n in (1, 2, 33, 64) for f0 in (0.0, 0.5) for f1 in (0.0, 1.5, 3.0)]
DT = (1000.0, 14000.0)  # checkpoints at 1 s and 15 s


@pytest.mark.skipif(not np.finfo(LD).eps < np.finfo(np.float64).eps, reason="no wide longdouble")
@pytest.mark.parametrize("n,f0,f1", GRID)
def test_golden_matches_longdouble(n, f0, f1):
    qa = analyzer(n)
    lmax = qa.rate_max / 1000.0
    got = normalised(lag_transient(qa.serv_rate, f0 * lmax, f1 * lmax, DT), qa.serv_rate)
    ref = reference(qa.serv_rate, f0 * lmax, f1 * lmax, DT)
    worst = float(np.abs(got - ref).max())
    print(f"N={n} lam0={f0} lam1={f1}: golden max abs err {worst:.3g}")
    assert worst <= GOLDEN_MAX_ERR


@pytest.mark.parametrize("n", (1, 2, 33))
def test_reference_matches_expm(n):
    from scipy.linalg import expm

    qa = analyzer(n)
    lmax = qa.rate_max / 1000.0
    up, s = (a.astype(np.float64) for a in chain(qa.serv_rate, 1.5 * lmax))
    gen = np.diag(up[:-1], 1) + np.diag(s[1:], -1)
    gen -= np.diag(gen.sum(axis=1))
    up0, _ = chain(qa.serv_rate, 0.5 * lmax)
    w = np.concatenate(([1.0], np.cumprod((up0[:-1] / s[1:]).astype(np.float64))))
    p = (w / w.sum()) @ expm(gen * 15000.0)
    ref = reference(qa.serv_rate, 0.5 * lmax, 1.5 * lmax, (15000.0,))[0]
    assert abs(p[-1] - float(ref[0])) < 1e-10
    assert abs(np.dot(p, np.minimum(np.arange(11 * n + 1), n)) / n - float(ref[1])) < 1e-10
    wait = np.dot(p[n:11 * n], np.arange(1, 10 * n + 1)) / (1 - p[-1]) / (10 * n)
    assert abs(wait - float(ref[2])) < 1e-10


def test_long_horizon_is_analyze():
    qa = analyzer(33)
    lam = 0.3 * qa.rate_max / 1000.0
    raw = lag_transient(qa.serv_rate, 0.0, lam, [60000.0] * 6)
    assert np.allclose(raw[-1], raw[-2], rtol=1e-12, atol=0)  # the golden has converged
    ttft, itl, rho = lag_latency(raw, qa.service_parms, qa.request_size, 33)
    m = qa.analyze(lam * 1000.0)
    want = (np.float32(m.avg_wait_time) + np.float32(m.avg_prefill_time), m.avg_token_time, m.rho)
    for got, ref in zip((ttft[-1], itl[-1], rho[-1]), want):
        assert abs(float(got) - float(ref)) <= 1e-9 * abs(float(ref))


PINNED_N = (1, 33, 64, 2049, 12, 70)


def small_fleet():
    system, _ = System.from_spec(make_spec(n_servers=6, seed=901, arrival_scale=6000.0))
    names = sorted(system.servers)
    for name, n in zip(names, PINNED_N):
        system.servers[name].max_batch_size = n
    return system


def test_lag_cpu_statuses_and_first_violation():
    fs = FastSweep(small_fleet(), backend="cpu")
    base, _, out_tok = fs._base_load()
    n_srv = len(fs.server_names)
    acc = np.array([int(fs.cell_acc_idx[fs.seg_start[i]]) for i in range(n_srv)])
    rep = np.full(n_srv, 4)
    acc[0] = -1  # NOT_HELD
    rep[4] = 0  # NO_REPLICAS
    scen = np.stack([base * 2, base * 2]).astype(np.float32)
    scen[:, 1] = 0.0  # IDLE with from_arrival 0 there
    frm = base.copy()
    frm[1] = frm[5] = 0.0  # server 5 starts empty: its TTFT climbs through the lag
    times = (1.0, 3.0)
    r = fs.lag(arrival=scen, allocation=(acc, rep), times=times, from_arrival=frm)
    assert r.ttft.shape == (2, 2, n_srv) and r.status.shape == (2, n_srv)
    assert list(r.status[0]) == [LAG_NOT_HELD, LAG_IDLE, LAG_OK, LAG_TOO_WIDE, LAG_NO_REPLICAS,
                                 LAG_OK]
    assert np.isnan(r.ttft[:, :, 3:5]).all() and np.isfinite(r.ttft[:, :, (2, 5)]).all()
    assert (r.steps[:, (2, 5)] > 0).all() and r.counts[0, LAG_OK] == 2
    tight = fs.lag(arrival=scen, allocation=(acc, rep), times=times, from_arrival=frm,
                   max_steps=int(r.steps[0, 5]) - 1)
    assert tight.status[0, 5] == LAG_BUDGET and np.isnan(tight.itl[:, 0, 5]).all()
    assert tight.steps[0, 5] == r.steps[0, 5]
    assert tight.status[0, 2] == (LAG_BUDGET if r.steps[0, 2] >= r.steps[0, 5] else LAG_OK)
    # NOT_HELD and IDLE follow hold()'s conventions
    h = fs.hold(arrival=scen * 0, allocation=(acc, rep))
    for f in ("ttft", "itl", "rho"):
        assert (getattr(r, f)[:, :, :2] == getattr(h, f)[None, :, :2]).all(), f
    assert (r.wait[:, :, :2] == 0).all() and (r.blocked[:, :, :2] == 0).all()
    assert r.acc_idx[0, 0] == -1 and r.first_violation[0, 0] == -1
    # degenerate perf parameters: INVALID
    bad = small_fleet()
    srv = bad.servers[sorted(bad.servers)[2]]
    for perf in bad.models[srv.model_name].perf_data.values():
        perf.decodeParms.alpha = perf.decodeParms.beta = 0.0
        perf.prefillParms.gamma = perf.prefillParms.delta = 0.0
    rb = FastSweep(bad, backend="cpu").lag(arrival=scen, allocation=(acc, rep), times=times)
    assert rb.status[0, 2] == LAG_INVALID
    # targets midway between the reference values at the two checkpoints
    assert r.ttft[1, 0, 5] > r.ttft[0, 0, 5]
    k = int(fs.seg_start[5])
    fs._stat["t_ttft"][k:fs.seg_start[6]] = 0.5 * (r.ttft[0, 0, 5] + r.ttft[1, 0, 5])
    fs._stat["t_itl"][k:fs.seg_start[6]] = 0.0
    mid = fs.lag(arrival=scen, allocation=(acc, rep), times=times, from_arrival=frm)
    assert mid.first_violation[0, 5] == 1 and list(mid.violated[:, 0, 5]) == [False, True]
    assert mid.first_violation[0, 1] == -1
