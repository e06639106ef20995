"""Lag paths, CPU golden: analyzer/lag.py lag_path_transient and
FastSweep.lag_path(backend="cpu").

The reference is the same per-interval uniformization sum in np.longdouble
with L = 80 and Poisson weights normalised over the window, the manner of
tests/test_lag_cpu.py::reference, with the rate changing per interval and the
scale-out mixing at each interval's start.

Largest absolute error of the golden over blocked, rho and wait * s(N) / Q,
measured here: 2.79e-14 (N = 33, empty start). PATH_GOLDEN_MAX_ERR is
2.8e-14; the GPU probe's tolerance is max(8 x it, 1e-12)
(tests/test_lag_path_gpu.py).
"""
import numpy as np
import pytest

from inferno_amd.analyzer.lag import lag_path_transient
from inferno_amd.engine import (LAG_BUDGET, LAG_NO_REPLICAS, LAG_NOT_HELD, LAG_OK, LAG_TOO_WIDE,
                                FastSweep)
from tests.test_lag_cpu import LD, analyzer, chain, normalised, small_fleet

PATH_GOLDEN_MAX_ERR = 2.8e-14  # measured by test_path_golden_matches_longdouble (see above)
STEPS = 600.0  # uniformization steps per tick, about


def path_reference(rates, start, lam, keep, dt, big_l=80.0):
    """[S, 3]: blocked, rho, wait * s(N) / Q at the end of every tick, longdouble."""
    n = len(rates)
    k, q = 11 * n, 10 * n
    v = np.eye(1, k + 1)[0].astype(LD)
    if start != "empty":
        up0, s = chain(rates, start[1])
        w = np.concatenate(([LD(1)], np.cumprod(up0[:-1] / s[1:])))
        v = (w / w.sum()).astype(LD)
    out = []
    for lam_j, keep_j in zip(lam, keep):
        up, s = chain(rates, lam_j)
        unif = LD(lam_j) + s.max()
        up, dn = up / unif, s / unif
        stay = 1 - up - dn
        v = v * LD(keep_j)
        v[0] += 1 - LD(keep_j)
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


@pytest.mark.skipif(not np.finfo(LD).eps < np.finfo(np.float64).eps, reason="no wide longdouble")
@pytest.mark.parametrize("n", (1, 2, 33))
@pytest.mark.parametrize("f0", (None, 0.5))
def test_path_golden_matches_longdouble(n, f0):
    qa = analyzer(n)
    lmax = qa.rate_max / 1000.0
    start = "empty" if f0 is None else ("stationary", f0 * lmax)
    lam = np.array([1.5, 0.0, 0.7]) * lmax
    keep = (1.0, 0.5, 1.0)
    dt = STEPS / (1.5 * lmax + float(qa.serv_rate.max()))
    got = normalised(lag_path_transient(qa.serv_rate, start, lam, keep, dt), qa.serv_rate)
    ref = path_reference(qa.serv_rate, start, lam, keep, dt)
    worst = float(np.abs(got - ref).max())
    print(f"N={n} start={start}: path golden max abs err {worst:.3g}")
    assert ref[0, 1] > ref[2, 1] > 0  # overload, then the halved fleet drains
    assert worst <= PATH_GOLDEN_MAX_ERR


def test_lag_path_cpu_statuses_and_violations():
    fs = FastSweep(small_fleet(), backend="cpu")  # N = 1, 33, 64, 2049, 12, 70
    base = fs._base_load()[0]
    n_srv, n_t = len(fs.server_names), 6
    first = np.array([int(fs.cell_acc_idx[fs.seg_start[i]]) for i in range(n_srv)])
    acc = np.tile(first, (n_t, 1))
    rep = np.full((n_t, n_srv), 4)
    assert fs.seg_start[1] - fs.seg_start[0] >= 2
    acc[3:, 0] = int(fs.cell_acc_idx[fs.seg_start[0] + 1])  # server 0: a second run from tick 3
    rep[2, 1] = 0  # server 1: NO_REPLICAS between two runs
    acc[4, 2] = -1  # server 2: holds nothing in tick 4
    rep[3:, 5] = 8  # server 5: scale-out
    scen = np.tile(base * 2, (n_t, 1)).astype(np.float32)
    scen[2, 4] = base[4] * 200  # server 4: one tick far above the others
    frm = base.copy()
    frm[5] = 0.0  # server 5 starts empty: its TTFT climbs along the path
    kw = dict(arrival=scen, allocation=(acc, rep), delay=0, start_allocation=(first, rep[0]),
              from_arrival=frm, tick_seconds=0.5)
    r = fs.lag_path(**kw)
    assert r.ttft.shape == (n_t, n_srv) and r.counts.shape == (n_t, 7)
    assert (r.status[:, 0] == LAG_OK).all() and (r.status[:, 3] == LAG_TOO_WIDE).all()
    assert list(r.status[:, 1]) == [LAG_OK, LAG_OK, LAG_NO_REPLICAS] + [LAG_OK] * 3
    assert list(r.status[:, 2]) == [LAG_OK] * 4 + [LAG_NOT_HELD, LAG_OK]
    assert r.acc_idx[4, 2] == -1 and r.ttft[4, 2] == 0 and np.isnan(r.ttft[2, 1])
    # a run after a gap or on another accelerator starts empty: fewer in the system
    # than the stationary start had, and than the tick before the gap
    for srv, j in ((0, 3), (1, 3), (2, 5)):
        assert r.in_system[j, srv] < r.in_system[j - 2, srv], (srv, j)
    assert r.in_system[3, 5] < r.in_system[2, 5]  # half of the replicas joined empty
    # a tick over the budget ends its run; every other run is as before
    cap = int(r.steps[r.status == LAG_OK].max()) - 1
    assert r.steps[2, 4] == cap + 1 and (np.delete(r.steps[:, 4], 2) < cap).all()
    tight = fs.lag_path(max_steps=cap, **kw)
    assert list(tight.status[:, 4]) == [LAG_OK] * 2 + [LAG_BUDGET] * 4
    assert np.isnan(tight.ttft[2:, 4]).all() and tight.steps[2, 4] == cap + 1
    others = [0, 1, 2, 3, 5]
    assert np.array_equal(tight.status[:, others], r.status[:, others])
    assert np.array_equal(tight.ttft[:2], r.ttft[:2], equal_nan=True)
    # targets midway between two golden values: violated from the tick the TTFT crosses
    lo, hi = sorted((float(r.ttft[0, 5]), float(r.ttft[1, 5])))
    assert hi > lo
    sl = slice(fs.seg_start[5], fs.seg_start[6])
    fs._stat["t_ttft"][sl] = np.float32(0.5 * (lo + hi))
    fs._stat["t_itl"][:] = 0.0
    mid = fs.lag_path(**kw)
    v = mid.violated
    assert v[:, 5].any() and not v[:, 5].all()
    assert np.array_equal(mid.ticks_violated, v.sum(axis=0))
    assert np.array_equal(mid.first_violation, np.where(v.any(axis=0), v.argmax(axis=0), -1))
    assert np.array_equal(mid.violations, v.sum(axis=1))
