"""Lag analysis, CPU golden: the transient distribution p(t) of the
state-dependent M/M/1/K chain by uniformization, in plain numpy fp64.

The chain has states 0..K, K = 11 N, birth rate lam1 below K and death rate
s(min(n, N)) from the fp32 service rates (build_service_rates) widened to
fp64. p(0) is the stationary distribution at lam0 (delta_0 for lam0 = 0; it
exists for every lam0 because K is finite). With Lam = lam1 + max s and
P = I + Q / Lam,

    p(t + dt) = sum_k Pois(Lam dt; k) p(t) P^k,

truncated to the Chernoff window the wait-time tail uses (L = 60: at most
2 e^-60 of the weight is dropped per interval). An interval takes j_hi
applications of P; checkpoints chain. ops/hip/wva_lag.inc is the device form
of exactly this; lag_window() is shared with it to the bit, so both count the
same steps.
"""
from __future__ import annotations

import math

import numpy as np

from .queue import effective_concurrency

LAG_L = 60.0
# raw functionals of one checkpoint, in the order the device probe returns them
LAG_FUNCS = ("blocked", "in_servers", "in_system", "tput", "wait")


def pois_log_pmf(i: float, x: float) -> float:
    """log of e^-x x^i / i! (wva_pois_log_pmf): the plain form below 16, the
    saddle-point form (Loader 2000) above, which has no large cancelling terms."""
    if i < 16.0:
        return i * math.log(x) - x - math.lgamma(i + 1.0)
    v = (x - i) / i
    i2 = 1.0 / (i * i)
    stirlerr = (1.0 / 12.0 - (1.0 / 360.0 - (1.0 / 1260.0 - (1.0 / 1680.0) * i2) * i2) * i2) / i
    return -0.5 * math.log(6.283185307179586477 * i) - stirlerr - i * (v - math.log1p(v))


def lag_window(x):
    """(j_lo, j_hi) of the Poisson window at mean x > 0 (scalars or arrays),
    as floats holding integers. j_hi is also the interval's step count."""
    x = np.asarray(x, dtype=np.float64)
    a = 2.0 * x * LAG_L
    lo = np.maximum(np.floor(x - np.sqrt(a)), 0.0)
    hi = np.ceil(x + LAG_L / 3.0 + np.sqrt(LAG_L * LAG_L / 9.0 + a))
    return lo, hi


def lag_steps(lam_unif, dt_ms) -> np.ndarray:
    """Stencil steps over all intervals ``dt_ms`` [T] at uniformization rates
    ``lam_unif`` [...]: float64 [...], exact integers."""
    x = np.asarray(lam_unif, dtype=np.float64)[..., None] * np.asarray(dt_ms, dtype=np.float64)
    return lag_window(x)[1].sum(axis=-1)


def stationary(rates: np.ndarray, lam0: float) -> np.ndarray:
    """The stationary distribution over 0..11 N at arrival rate lam0 >= 0, in
    log space: prefix of log(lam0 / s(n)) over the head, the geometric tail by
    multiplication, max, exp, one sum."""
    s = np.asarray(rates, dtype=np.float64)
    n_max = len(s)
    k_max = 11 * n_max
    p = np.zeros(k_max + 1)
    if lam0 <= 0.0:
        p[0] = 1.0
        return p
    l0 = math.log(lam0)
    logw = np.empty(k_max + 1)
    logw[0] = 0.0
    logw[1:n_max + 1] = np.cumsum(l0 - np.log(s))
    logw[n_max + 1:] = logw[n_max] + np.arange(1, k_max - n_max + 1) * (l0 - math.log(s[-1]))
    p = np.exp(logw - logw.max())
    return p / p.sum()


def lag_transient(rates: np.ndarray, lam0: float, lam1: float, dt_ms) -> np.ndarray:
    """Raw functionals [T, 5] (LAG_FUNCS) of the chain with fp32 service rates
    ``rates`` [N] (req/msec) at the ends of the intervals ``dt_ms`` (msec),
    from the stationary start at lam0 under arrival rate lam1 (req/msec)."""
    s = np.asarray(rates, dtype=np.float64)
    n_max = len(s)
    k_max = 11 * n_max
    q_len = k_max - n_max
    lam_unif = lam1 + float(s.max())
    s_state = np.concatenate(([0.0], s, np.full(q_len, s[-1])))  # death rate of state n
    dn = s_state / lam_unif
    up = np.full(k_max + 1, lam1 / lam_unif)
    up[k_max] = 0.0
    stay = np.maximum(1.0 - up - dn, 0.0)
    in_srv = np.minimum(np.arange(k_max + 1), n_max).astype(np.float64)
    in_sys = np.arange(k_max + 1, dtype=np.float64)
    departures = np.arange(1, q_len + 1, dtype=np.float64)

    def step(v):
        nv = v * stay
        nv[1:] += v[:-1] * up[:-1]
        nv[:-1] += v[1:] * dn[1:]
        return nv

    v = stationary(rates, lam0)
    out = np.empty((len(dt_ms), len(LAG_FUNCS)))
    for j, dt in enumerate(dt_ms):
        x = lam_unif * float(dt)
        lo, hi = (int(b) for b in lag_window(x))
        for _ in range(lo):
            v = step(v)
        w = math.exp(pois_log_pmf(float(lo), x))
        acc = w * v
        for k in range(lo + 1, hi + 1):
            v = step(v)
            w *= x / k
            acc += w * v
        v = acc
        blocked = float(v[k_max])
        wait = float(np.dot(v[n_max:k_max], departures)) / (1.0 - blocked) / float(s[-1])
        out[j] = (blocked, np.dot(v, in_srv), np.dot(v, in_sys), np.dot(v[1:], s_state[1:]), wait)
    return out


def lag_path_transient(rates: np.ndarray, start, lam, keep, dt_ms: float,
                       averages: bool = False):
    """Raw functionals [S, 5] (LAG_FUNCS) at the ends of S consecutive
    intervals of ``dt_ms`` msec each, interval j under arrival rate ``lam[j]``
    (req/msec). ``start`` is ("stationary", lam0) or "empty" (all mass in
    state 0). At the start of interval j the vector is mixed with the empty
    state, p <- keep[j] p + (1 - keep[j]) e_0 (a scale-out; 1: no change).
    Per interval: lag_transient's uniformization at Lam_j = lam[j] + max s,
    the same window and step count (lag_window), non-negative terms only.
    ops/hip/wva_lag_path.inc is the device form of exactly this.

    ``averages``: return (the above, the same functionals [S, 5] of the TIME
    AVERAGE of the distribution over every interval) instead. With x = Lam_j
    dt and v_k the vector after k steps (v_0 after the mixing),
    pbar = (1 / x) sum_{k=0..j_hi} T_k v_k, T_k = P(Pois(x) > k): 1 below the
    window (to within e^-60), T_k = max(T_{k-1} - w_k, 0) inside it, with the
    weights w_k of the end state's sum. It is what a random arrival of the
    interval meets; ops/hip/wva_lag_path_avg.inc is the device form."""
    s = np.asarray(rates, dtype=np.float64)
    n_max = len(s)
    k_max = 11 * n_max
    q_len = k_max - n_max
    s_max = float(s.max())
    s_state = np.concatenate(([0.0], s, np.full(q_len, s[-1])))  # death rate of state n
    in_srv = np.minimum(np.arange(k_max + 1), n_max).astype(np.float64)
    in_sys = np.arange(k_max + 1, dtype=np.float64)
    departures = np.arange(1, q_len + 1, dtype=np.float64)
    if isinstance(start, str):
        if start != "empty":
            raise ValueError(f"start must be 'empty' or ('stationary', lam0), got {start!r}")
        v = stationary(rates, 0.0)
    else:
        kind, lam0 = start
        if kind != "stationary":
            raise ValueError(f"start must be 'empty' or ('stationary', lam0), got {start!r}")
        v = stationary(rates, float(lam0))
    lam = np.asarray(lam, dtype=np.float64)
    keep = np.asarray(keep, dtype=np.float64)
    out = np.empty((len(lam), len(LAG_FUNCS)))
    out_avg = np.empty_like(out)
    for j in range(len(lam)):
        lam_unif = float(lam[j]) + s_max
        dn = s_state / lam_unif
        up = np.full(k_max + 1, float(lam[j]) / lam_unif)
        up[k_max] = 0.0
        stay = np.maximum(1.0 - up - dn, 0.0)

        def step(v):
            nv = v * stay
            nv[1:] += v[:-1] * up[:-1]
            nv[:-1] += v[1:] * dn[1:]
            return nv

        v = v * float(keep[j])
        v[0] += 1.0 - float(keep[j])
        x = lam_unif * float(dt_ms)
        lo, hi = (int(b) for b in lag_window(x))
        avg = np.zeros_like(v)
        for _ in range(lo):
            if averages:
                avg += v  # T_k = 1 below the window
            v = step(v)
        w = math.exp(pois_log_pmf(float(lo), x))
        acc = w * v
        tail = max(1.0 - w, 0.0)  # T_lo
        if averages:
            avg += tail * v
        for k in range(lo + 1, hi + 1):
            v = step(v)
            w *= x / k
            acc += w * v
            if averages:
                tail = max(tail - w, 0.0)
                avg += tail * v
        v = acc
        blocked = float(v[k_max])
        wait = float(np.dot(v[n_max:k_max], departures)) / (1.0 - blocked) / float(s[-1])
        out[j] = (blocked, np.dot(v, in_srv), np.dot(v, in_sys), np.dot(v[1:], s_state[1:]), wait)
        if averages:
            p = avg / x
            blocked = float(p[k_max])
            wait = float(np.dot(p[n_max:k_max], departures)) / (1.0 - blocked) / float(s[-1])
            out_avg[j] = (blocked, np.dot(p, in_srv), np.dot(p, in_sys),
                          np.dot(p[1:], s_state[1:]), wait)
    return (out, out_avg) if averages else out


def lag_latency(raw: np.ndarray, parms, req, n_max: int):
    """(ttft, itl, rho) per checkpoint from raw functionals [T, 5], with the
    analyzer's definitions: serv = in_servers / tput (0 when nothing departs),
    eff = effective_concurrency(serv), ttft = wait + prefill_time(eff), itl =
    decode_time(eff), each latency term rounded to fp32 as everywhere."""
    ttft = np.empty(len(raw), dtype=np.float32)
    itl = np.empty(len(raw), dtype=np.float32)
    for j, (_, in_servers, _, tput, wait) in enumerate(raw):
        serv = in_servers / tput if tput > 0.0 else 0.0
        eff = effective_concurrency(serv, parms, req, n_max)
        ttft[j] = np.float32(wait) + np.float32(
            parms.prefill.prefill_time(req.avg_input_tokens, eff))
        itl[j] = np.float32(parms.decode.decode_time(eff))
    rho = np.clip(raw[:, 1] / float(n_max), 0.0, 1.0)
    return ttft, itl, rho
