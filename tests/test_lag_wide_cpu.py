"""Wide lag (N above LAG_MAX_N), the parts that need no GPU: the golden at
the first wide sizes, the host schedule, and FastSweep.lag(max_n=...) on the
CPU backend.

GOLDEN_MAX_ERR was measured up to N = 64. Largest absolute error of the golden
against the longdouble reference at N in {1118, 1200}, about 600 steps per
interval, over blocked, rho and wait * s(N) / Q, measured here: 7.44e-14
(N = 1200, the start near the full queue into 3 lam_max; 7.42e-14 at N = 1118). WIDE_GOLDEN_MAX_ERR is 7.5e-14; the wide GPU probe's
tolerance is max(8 x it, 1e-12) (tests/test_lag_wide_gpu.py).
"""
import numpy as np
import pytest

from inferno_amd.analyzer.lag import lag_transient, lag_window
from inferno_amd.engine import LAG_OK, LAG_TOO_WIDE, LAG_WIDE_MAX_N, FastSweep
from inferno_amd.ops.sweep import LAG_SEG_FINAL, LAG_SEG_FIRST, LAG_SEG_LAST, lag_segments
from tests.test_lag_cpu import LD, analyzer, normalised, reference, small_fleet

WIDE_GOLDEN_MAX_ERR = 7.5e-14  # measured by test_golden_matches_longdouble_wide (see above)
STEPS = 600.0  # uniformization steps per checkpoint interval, about


def regimes(qa):
    """test_probe_matches_longdouble's three: cold start into overload; a start
    near the full queue into a heavier overload; warm start draining. Each with
    its own two checkpoints of about STEPS steps: (lam0, lam1, dt_ms)."""
    lmax = qa.rate_max / 1000.0
    smax = float(qa.serv_rate.max())
    out = []
    for lam0, lam1 in ((0.0, 1.5 * lmax), (1.05 * lmax, 3.0 * lmax), (0.9 * lmax, 0.0)):
        t1 = STEPS / (lam1 + smax) / 1000.0
        out.append((lam0, lam1, (t1 * 1000.0, (2.0 * t1 - t1) * 1000.0)))
    return out


@pytest.mark.skipif(not np.finfo(LD).eps < np.finfo(np.float64).eps, reason="no wide longdouble")
@pytest.mark.parametrize("n", (1118, 1200))
def test_golden_matches_longdouble_wide(n):
    qa = analyzer(n)
    worst = 0.0
    for c, (lam0, lam1, dt) in enumerate(regimes(qa)):
        got = normalised(lag_transient(qa.serv_rate, lam0, lam1, dt), qa.serv_rate)
        err = float(np.abs(got - reference(qa.serv_rate, lam0, lam1, dt)).max())
        print(f"N={n} regime {c}: golden max abs err {err:.3g}")
        worst = max(worst, err)
    assert worst <= WIDE_GOLDEN_MAX_ERR


# (x per interval, T): j_lo inside a segment, an interval shorter than T, j_lo = 0,
# and an interval that is a whole number of segments
@pytest.mark.parametrize("xs,halo", [((600.0, 600.0), 96), ((40.0, 3000.0), 768),
                                     ((0.5, 5.0), 24), ((700.0,), 1536)])
def test_segments_partition_the_steps(xs, halo):
    lo, hi = lag_window(np.array(xs))
    segs = lag_segments(lo, hi, xs, halo)
    assert (segs["count"] >= 1).all() and (segs["count"] <= halo).all()
    for j in range(len(xs)):
        mine = segs[segs["j"] == j]
        # consecutive runs from step 0 to j_hi: a partition that stays in its interval
        assert list(mine["first"]) == list(np.cumsum(mine["count"]) - mine["count"])
        assert mine["count"].sum() == hi[j] and (mine["jlo"] == lo[j]).all()
        assert (mine["jhi"] == hi[j]).all() and (mine["x"] == xs[j]).all()
        assert list(mine["flags"] & LAG_SEG_FIRST) == [1] + [0] * (len(mine) - 1)
        assert list(mine["flags"] & LAG_SEG_LAST) == [0] * (len(mine) - 1) + [LAG_SEG_LAST]
    assert list(segs["j"]) == sorted(segs["j"])
    assert list(np.nonzero(segs["flags"] & LAG_SEG_FINAL)[0]) == [len(segs) - 1]
    if halo == 96:
        assert ((segs["first"] < segs["jlo"]) & (segs["jlo"] < segs["first"] + segs["count"])).any()


def test_lag_cpu_max_n():
    fs = FastSweep(small_fleet(), backend="cpu")
    base = fs._base_load()[0]
    n_srv = len(fs.server_names)
    acc = np.array([int(fs.cell_acc_idx[fs.seg_start[i]]) for i in range(n_srv)])
    kw = dict(arrival=np.stack([base * 2]).astype(np.float32),
              allocation=(acc, np.full(n_srv, 4)), times=(0.05, 0.1))
    wide = fs.lag(max_n=LAG_WIDE_MAX_N, **kw)
    assert wide.status[0, 3] == LAG_OK and np.isfinite(wide.ttft[:, 0, 3]).all()  # N = 2049
    assert wide.steps[0, 3] > 0
    for r in (fs.lag(**kw), fs.lag(max_n=2048, **kw)):
        assert r.status[0, 3] == LAG_TOO_WIDE and np.isnan(r.ttft[:, 0, 3]).all()
        others = [i for i in range(n_srv) if i != 3]
        assert np.array_equal(r.status[0, others], wide.status[0, others])
        assert np.array_equal(r.ttft[:, 0, others], wide.ttft[:, 0, others], equal_nan=True)
    for bad in (LAG_WIDE_MAX_N + 1, 0):
        with pytest.raises(ValueError):
            fs.lag(max_n=bad, **kw)
