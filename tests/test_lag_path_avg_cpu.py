"""Lag path averages, CPU golden: analyzer/lag.py
lag_path_transient(averages=True).

The reference is the direct sum pbar = (1 / x) sum_{k=0..j_hi} T_k v_k in
np.longdouble with no window: every k from 0 (j_hi at L = 80), T_k = P(Pois(x)
> k) from a longdouble pmf summed from the top, the end state carried as
tests/test_lag_path_cpu.py::path_reference carries it.

Largest absolute error of the golden's averages over blocked, rho and
wait * s(N) / Q, measured here: 2.38e-14 (N = 1, stationary start).
PATH_AVG_GOLDEN_MAX_ERR is 2.4e-14; the GPU probe's tolerance is
max(8 x it, 1e-12) (tests/test_lag_path_avg_gpu.py).
"""
import numpy as np
import pytest

from inferno_amd.analyzer.lag import lag_path_transient
from tests.test_lag_cpu import LD, analyzer, chain, normalised
from tests.test_lag_path_cpu import STEPS

PATH_AVG_GOLDEN_MAX_ERR = 2.4e-14  # measured by test_avg_golden_matches_longdouble (see above)
# overload, scale-out to twice the replicas, drain, moderate load (x lmax)
LAM = np.array([1.5, 0.75, 0.0, 0.7])
KEEP = np.array([1.0, 0.5, 1.0, 1.0])


def avg_reference(rates, start, lam, keep, dt, big_l=80.0):
    """[S, 3]: blocked, rho, wait * s(N) / Q of the distribution averaged over
    every tick, longdouble."""
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
        hi = int(np.ceil(x + big_l / 3 + np.sqrt(big_l * big_l / 9 + 2 * x * big_l)))
        log_fact = np.concatenate(([0], np.cumsum(np.log(np.arange(1, hi + 1, dtype=LD)))))
        logw = np.arange(hi + 1).astype(LD) * np.log(x) - log_fact
        pmf = np.exp(logw - logw.max())
        pmf /= pmf.sum()  # 0..hi holds all but e^-80 of the weight
        tail = np.concatenate((np.cumsum(pmf[::-1])[::-1][1:], [LD(0)]))  # T_k, from the top
        acc, avg = np.zeros_like(v), np.zeros_like(v)
        for j in range(hi + 1):
            acc += pmf[j] * v
            avg += tail[j] * v
            nv = v * stay
            nv[1:] += v[:-1] * up[:-1]
            nv[:-1] += v[1:] * dn[1:]
            v = nv
        v, p = acc, avg / x
        wait = np.dot(p[n:k], np.arange(1, q + 1).astype(LD)) / (1 - p[k]) / q
        out.append((p[k], np.dot(p, np.minimum(np.arange(k + 1), n)) / n, wait))
    return np.array(out, dtype=LD)


def path(n):
    """(analyzer, the two starts, lam [4], tick length in msec) of the test path."""
    qa = analyzer(n)
    lmax = qa.rate_max / 1000.0
    dt = STEPS / (1.5 * lmax + float(qa.serv_rate.max()))
    return qa, [("stationary", 0.5 * lmax), "empty"], LAM * lmax, dt


@pytest.mark.skipif(not np.finfo(LD).eps < np.finfo(np.float64).eps, reason="no wide longdouble")
@pytest.mark.parametrize("n", (1, 2, 33))
@pytest.mark.parametrize("c", (0, 1))
def test_avg_golden_matches_longdouble(n, c):
    qa, starts, lam, dt = path(n)
    end, avg = lag_path_transient(qa.serv_rate, starts[c], lam, KEEP, dt, averages=True)
    # the end-state half is the existing return, to the bit
    assert np.array_equal(end, lag_path_transient(qa.serv_rate, starts[c], lam, KEEP, dt))
    got = normalised(avg, qa.serv_rate)
    worst = float(np.abs(got - avg_reference(qa.serv_rate, starts[c], lam, KEEP, dt)).max())
    print(f"N={n} start={starts[c]}: averaged golden max abs err {worst:.3g}")
    assert worst <= PATH_AVG_GOLDEN_MAX_ERR
    # the drain tick ends emptier than it was on average
    assert avg[2, 1] > end[2, 1]
