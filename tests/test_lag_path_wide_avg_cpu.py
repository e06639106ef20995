"""Lag path averages for wide cells (N above LAG_MAX_N), the parts that need no
GPU: the averaged golden at the first wide size against the longdouble direct
sum with no window (tests/test_lag_path_avg_cpu.py avg_reference), and
FastSweep.lag_path(max_n=..., averages=True) on the CPU backend.

Largest absolute error of lag_path_transient(averages=True) over blocked, rho
and wait * s(N) / Q at N = 1118 on the 4-tick path of wide_path_case, measured
here: 1.41e-15 from the stationary start, 1.29e-15 from empty (1.36e-15 at
N = 1200; 1.0e-16 on the short ticks whose windows start at j_lo = 0).
WIDE_PATH_AVG_GOLDEN_MAX_ERR is 1.5e-15; the wide GPU probe's tolerance is
max(8 x it, 1e-12) (tests/test_lag_path_wide_avg_gpu.py).
"""
import functools

import numpy as np
import pytest

from inferno_amd.analyzer.lag import lag_path_transient
from inferno_amd.engine import LAG_OK, LAG_WIDE_MAX_N, FastSweep
from tests.test_lag_cpu import LD, normalised, small_fleet
from tests.test_lag_path_avg_cpu import avg_reference
from tests.test_lag_path_wide_cpu import wide_path_case

WIDE_PATH_AVG_GOLDEN_MAX_ERR = 1.5e-15  # measured by test_avg_golden_matches_longdouble_wide


@functools.lru_cache(maxsize=None)
def wide_avg_case(n, short=False):
    """wide_path_case(n) with the longdouble references of the AVERAGED
    distribution for its two starts: (analyzer, lam, keep, tick seconds,
    starts, references). ``short``: ticks of 60 / (largest Lam) msec, so that
    every window starts at j_lo = 0."""
    qa, lam, keep, tick_s, starts, _ = wide_path_case(n)
    if short:
        tick_s = 60.0 / (float(lam.max()) + float(qa.serv_rate.max())) / 1000.0
    refs = tuple(avg_reference(qa.serv_rate, s, lam, keep, tick_s * 1000.0) for s in starts)
    return qa, lam, keep, tick_s, starts, refs


@pytest.mark.skipif(not np.finfo(LD).eps < np.finfo(np.float64).eps, reason="no wide longdouble")
def test_avg_golden_matches_longdouble_wide():
    qa, lam, keep, tick_s, starts, refs = wide_avg_case(1118)
    worst = 0.0
    for start, ref in zip(starts, refs):
        end, avg = lag_path_transient(qa.serv_rate, start, lam, keep, tick_s * 1000.0,
                                      averages=True)
        err = float(np.abs(normalised(avg, qa.serv_rate) - ref).max())
        print(f"N=1118 start={start}: averaged golden max abs err {err:.3g}")
        worst = max(worst, err)
        assert avg[2, 1] > end[2, 1]  # the drain tick ends emptier than it was on average
    assert worst <= WIDE_PATH_AVG_GOLDEN_MAX_ERR


def test_lag_path_cpu_max_n_averages():
    fs = FastSweep(small_fleet(), backend="cpu")  # N = 1, 33, 64, 2049, 12, 70
    base = fs._base_load()[0]
    n_srv, n_t = len(fs.server_names), 3
    first = np.array([int(fs.cell_acc_idx[fs.seg_start[i]]) for i in range(n_srv)])
    kw = dict(arrival=np.tile(base * 2, (n_t, 1)).astype(np.float32),
              allocation=(np.tile(first, (n_t, 1)), np.full((n_t, n_srv), 4)), delay=0,
              start_allocation=(first, np.full(n_srv, 4)), tick_seconds=0.05, averages=True)
    wide = fs.lag_path(max_n=LAG_WIDE_MAX_N, **kw)
    narrow = fs.lag_path(**kw)
    assert (wide.status[:, 3] == LAG_OK).all()
    fields = ("ttft_avg", "itl_avg", "rho_avg", "blocked_avg")
    for f in fields:
        assert np.isfinite(getattr(wide, f)[:, 3]).all(), f
        assert np.isnan(getattr(narrow, f)[:, 3]).all(), f  # LAG_TOO_WIDE there
    assert (wide.blocked_avg[:, 3] >= 0).all() and (wide.rho_avg[:, 3] <= 1).all()
    others = [i for i in range(n_srv) if i != 3]
    for f in fields + ("violated_avg", "ttft", "itl", "status", "violated"):
        a, b = getattr(narrow, f)[:, others], getattr(wide, f)[:, others]
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), f
