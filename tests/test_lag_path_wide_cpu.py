"""Lag paths for wide cells (N above LAG_MAX_N), the parts that need no GPU:
the path golden at the first wide size, the host schedule of the tiled pass,
and FastSweep.lag_path(max_n=...) on the CPU backend.

PATH_GOLDEN_MAX_ERR was measured up to N = 33. Largest absolute error of
lag_path_transient against the longdouble path reference at N = 1118 on the
4-tick path of tests/test_lag_path_gpu.py (overload, keep 0.5, drain, moderate
load; about 600 steps per tick), over blocked, rho and wait * s(N) / Q,
measured here: 2.73e-15 (the stationary start; 2.32e-15 from empty).
WIDE_PATH_GOLDEN_MAX_ERR is 2.8e-15; the wide GPU probe's tolerance is
max(8 x it, 1e-12) (tests/test_lag_path_wide_gpu.py).
"""
import functools

import numpy as np
import pytest

from inferno_amd.analyzer.lag import lag_path_transient, lag_window
from inferno_amd.engine import LAG_OK, LAG_TOO_WIDE, LAG_WIDE_MAX_N, FastSweep
from inferno_amd.ops.sweep import (LAG_PATH_EMPTY, LAG_PATH_STATIONARY, LAG_SEG_FINAL,
                                   LAG_SEG_FIRST, LAG_SEG_LAST, LAG_WIDE_HALO, LAG_WIDE_STRIDE,
                                   lag_path_wide_schedule)
from tests.test_lag_cpu import IN_TOK, LD, OUT_TOK, PERF, analyzer, normalised, small_fleet
from tests.test_lag_path_cpu import STEPS, path_reference

WIDE_PATH_GOLDEN_MAX_ERR = 2.8e-15  # measured by test_path_golden_matches_longdouble_wide
# (N, stride, halo): the first N past the one-block classes, two tiles; the head
# crosses cuts, 17 tiles, several segments per tick, j_lo inside one; the
# smallest halo; 11 N + 1 padded to 12672 = 11 x 1152 slots, the last tile full
TILINGS = [(1118, LAG_WIDE_STRIDE, LAG_WIDE_HALO), (1118, 768, 96), (1200, 1536, 24),
           (1150, 1152, 96)]


@functools.lru_cache(maxsize=None)
def wide_path_case(n):
    """test_path_probe_matches_longdouble's path at N = n: (analyzer, lam [4],
    keep [4], tick seconds, the two starts, their longdouble references)."""
    qa = analyzer(n)
    lmax = qa.rate_max / 1000.0
    lam = np.array([1.5, 0.75, 0.0, 0.7]) * lmax  # overload, scale-out x2, drain, moderate
    keep = np.array([1.0, 0.5, 1.0, 1.0])
    tick_s = STEPS / (1.5 * lmax + float(qa.serv_rate.max())) / 1000.0
    starts = (("stationary", 0.5 * lmax), "empty")
    refs = tuple(path_reference(qa.serv_rate, s, lam, keep, tick_s * 1000.0) for s in starts)
    return qa, lam, keep, tick_s, starts, refs


@pytest.mark.skipif(not np.finfo(LD).eps < np.finfo(np.float64).eps, reason="no wide longdouble")
def test_path_golden_matches_longdouble_wide():
    qa, lam, keep, tick_s, starts, refs = wide_path_case(1118)
    worst = 0.0
    for start, ref in zip(starts, refs):
        got = normalised(lag_path_transient(qa.serv_rate, start, lam, keep, tick_s * 1000.0),
                         qa.serv_rate)
        err = float(np.abs(got - ref).max())
        print(f"N=1118 start={start}: path golden max abs err {err:.3g}")
        worst = max(worst, err)
    assert worst <= WIDE_PATH_GOLDEN_MAX_ERR


@pytest.mark.parametrize("stride,halo", [t[1:] for t in TILINGS])
def test_wide_schedule_partitions_every_tick(stride, halo):
    ns = np.array([1118, 1200, 1150], dtype=np.int32)
    tick0, n_run, n_ticks = [0, 2, 1], [4, 3, 1], 5
    smax = np.array([float(analyzer(int(n)).serv_rate.max()) for n in ns])
    dt = STEPS / smax.max()
    rng = np.random.default_rng(7)
    lam = [rng.uniform(0.0, 1.5, k) * smax[t] for t, k in enumerate(n_run)]
    keep = [rng.uniform(0.3, 1.0, k) for k in n_run]
    fields = {k: np.full(3, v, dtype=np.float32) for k, v in PERF.items()}
    fields.update(in_tok=np.full(3, IN_TOK), out_tok=np.full(3, OUT_TOK), N=ns,
                  slot=np.array([2, 0, 1]), t_ttft=np.zeros(3), t_itl=np.zeros(3),
                  lam0=np.array([0.3, 0.0, 0.0]),
                  start=np.array([LAG_PATH_STATIONARY, LAG_PATH_EMPTY, LAG_PATH_EMPTY]))
    table, wide, segs, tiles, desc, order = lag_path_wide_schedule(
        fields, tick0, lam, keep, smax, dt, n_ticks, stride, halo)
    assert list(wide["n_seg"]) == sorted(wide["n_seg"], reverse=True)  # the launch prefix
    assert (segs["count"] >= 1).all() and (segs["count"] <= halo).all()
    assert desc.shape == (3, n_ticks, 2)
    for row, t in enumerate(order):
        w = wide[row]
        assert (table["N"][row], table["slot"][row]) == (ns[t], fields["slot"][t])
        assert (w["tick0"], w["n_run"], w["start"]) == (tick0[t], n_run[t], fields["start"][t])
        assert w["n_tiles"] == -(-(-(-(11 * int(ns[t]) + 1) // 24) * 24) // stride)
        assert list(tiles["b"][w["tile0"]:w["tile0"] + w["n_tiles"]]) == list(range(w["n_tiles"]))
        assert (tiles["task"][w["tile0"]:w["tile0"] + w["n_tiles"]] == row).all()
        mine = segs[w["seg0"]:w["seg0"] + w["n_seg"]]
        lo, hi = lag_window((lam[t] + smax[t]) * dt)
        assert list(mine["j"]) == sorted(mine["j"])
        for jr in range(n_run[t]):
            j = tick0[t] + jr
            tick = mine[mine["j"] == j]  # consecutive runs from step 0 to j_hi, inside the tick
            assert list(tick["first"]) == list(np.cumsum(tick["count"]) - tick["count"])
            assert tick["count"].sum() == hi[jr] and (tick["jhi"] == hi[jr]).all()
            assert (tick["jlo"] == lo[jr]).all() and (tick["x"] == (lam[t][jr] + smax[t]) * dt).all()
            assert list(tick["flags"] & LAG_SEG_FIRST) == [1] + [0] * (len(tick) - 1)
            assert list(tick["flags"] & LAG_SEG_LAST) == [0] * (len(tick) - 1) + [LAG_SEG_LAST]
            assert tuple(desc[fields["slot"][t], j]) == (lam[t][jr], keep[t][jr])
        assert set(mine["j"]) == set(range(tick0[t], tick0[t] + n_run[t]))
        assert list(np.nonzero(mine["flags"] & LAG_SEG_FINAL)[0]) == [len(mine) - 1]


def test_lag_path_cpu_max_n():
    fs = FastSweep(small_fleet(), backend="cpu")  # N = 1, 33, 64, 2049, 12, 70
    base = fs._base_load()[0]
    n_srv, n_t = len(fs.server_names), 3
    first = np.array([int(fs.cell_acc_idx[fs.seg_start[i]]) for i in range(n_srv)])
    kw = dict(arrival=np.tile(base * 2, (n_t, 1)).astype(np.float32),
              allocation=(np.tile(first, (n_t, 1)), np.full((n_t, n_srv), 4)), delay=0,
              start_allocation=(first, np.full(n_srv, 4)), tick_seconds=0.05)
    wide = fs.lag_path(max_n=LAG_WIDE_MAX_N, **kw)
    assert (wide.status[:, 3] == LAG_OK).all() and np.isfinite(wide.ttft[:, 3]).all()
    assert (wide.steps[:, 3] > 0).all()
    others = [i for i in range(n_srv) if i != 3]
    for r in (fs.lag_path(**kw), fs.lag_path(max_n=2048, **kw)):
        assert (r.status[:, 3] == LAG_TOO_WIDE).all() and np.isnan(r.ttft[:, 3]).all()
        for f in ("status", "steps", "violated", "held_replicas", "acc_idx", "ttft", "itl",
                  "wait", "blocked", "rho", "in_system"):
            assert np.array_equal(getattr(r, f)[:, others], getattr(wide, f)[:, others],
                                  equal_nan=getattr(r, f).dtype.kind == "f"), f
    for bad in (LAG_WIDE_MAX_N + 1, 0):
        with pytest.raises(ValueError):
            fs.lag_path(max_n=bad, **kw)
