"""Lag path averages on the GPU: wva_lag_path_avg_t through
run_lag_path_probe(averages=True), and FastSweep.lag_path(averages=True)
against the CPU backend.

The probe's averaged functionals are compared with the longdouble direct sum of
tests/test_lag_path_avg_cpu.py (never with the GPU's own output) at the first
and last N of every kernel instantiation, once as one chunk and once cut 2 + 2
through the carry, within max(8 x PATH_AVG_GOLDEN_MAX_ERR, 1e-12) on blocked,
rho and wait * s(N) / Q; the two schedules agree to the bit, and the end-state
half is run_lag_path_probe's without averages to the bit.

Measured on MI355X: largest absolute error 2.40e-14 (N = 1), 1.79e-15 at
N = 1024 and 5.21e-16 there with j_lo = 0; 2639 steps per cell; tolerance 1e-12.
"""
import numpy as np
import pytest

from inferno_amd.analyzer.lag import lag_window
from inferno_amd.engine import LAG_OK, FastSweep
from inferno_amd.ops.sweep import run_lag_path_probe
from tests.test_lag_cpu import IN_TOK, OUT_TOK, PERF, normalised
from tests.test_lag_gpu import lag_system
from tests.test_lag_path_avg_cpu import KEEP, PATH_AVG_GOLDEN_MAX_ERR, avg_reference, path
from tests.test_lag_path_gpu import fleet

pytestmark = pytest.mark.gpu

TOL = max(8 * PATH_AVG_GOLDEN_MAX_ERR, 1e-12)


def probe_args(n, starts, lam, tick_ms):
    arrays = {k: np.full(2, v, dtype=np.float32) for k, v in PERF.items()}
    arrays.update(in_tok=np.full(2, IN_TOK, dtype=np.int32),
                  out_tok=np.full(2, OUT_TOK, dtype=np.int32),
                  batch_n=np.full(2, n, dtype=np.int32))
    return arrays, starts, np.tile(lam, (2, 1)), np.tile(KEEP, (2, 1)), tick_ms / 1000.0


def worst_error(avg, qa, starts, lam, tick_ms):
    return max(float(np.abs(normalised(avg[c], qa.serv_rate)
                            - avg_reference(qa.serv_rate, s, lam, KEEP, tick_ms)).max())
               for c, s in enumerate(starts))


@pytest.mark.parametrize("n", (1, 11, 12, 69, 70, 279, 280, 1024))
def test_avg_probe_matches_longdouble(n):
    qa, starts, lam, tick_ms = path(n)
    args = probe_args(n, starts, lam, tick_ms)
    raw, avg, steps, bounds = run_lag_path_probe(*args, averages=True)
    assert list(bounds) == [0, 4] and (steps > 0).all() and steps.sum(axis=1).max() <= 3000
    cut = int(steps[0, :2].sum())  # the third tick no longer fits: chunks of 2 + 2
    raw2, avg2, steps2, bounds2 = run_lag_path_probe(*args, max_steps=cut, averages=True)
    assert list(bounds2) == [0, 2, 4] and np.array_equal(steps, steps2)
    err = worst_error(avg, qa, starts, lam, tick_ms)
    print(f"N={n}: steps {steps[0].tolist()}, averaged max abs err {err:.3g}")
    assert err <= TOL
    assert np.array_equal(avg, avg2) and np.array_equal(raw, raw2)  # the carry loses nothing
    plain, plain_steps, _ = run_lag_path_probe(*args)
    assert np.array_equal(raw, plain) and np.array_equal(steps, plain_steps)
    assert (avg[:, 2, 1] > raw[:, 2, 1]).all()  # the drain tick: busier on average than at its end


def test_avg_probe_without_a_lower_window():
    # ticks so short that j_lo = 0 in every one: the widest class starts in its
    # window phase, on a zeroed slab
    n = 1024
    qa, starts, lam, _ = path(n)
    tick_ms = 60.0 / (lam.max() + float(qa.serv_rate.max()))
    lo, hi = lag_window((lam + float(qa.serv_rate.max())) * tick_ms)
    assert (lo == 0).all() and (hi > 60).all()
    raw, avg, steps, _ = run_lag_path_probe(*probe_args(n, starts, lam, tick_ms), averages=True)
    assert np.array_equal(steps[0], hi.astype(np.int32))
    err = worst_error(avg, qa, starts, lam, tick_ms)
    print(f"N={n}, j_lo = 0: steps {steps[0].tolist()}, averaged max abs err {err:.3g}")
    assert err <= TOL


def test_gpu_lag_path_averages_match_cpu():
    fs_g, fs_c, kw = fleet()
    # a TTFT target between the averaged TTFTs of the first two ticks where they move
    first = fs_c.lag_path(averages=True, **kw)
    moving = 0
    for i in range(len(fs_c.server_names)):
        lo, hi = sorted((float(first.ttft_avg[0, i]), float(first.ttft_avg[1, i])))
        mid = np.float32(0.5 * (lo + hi)) if hi - lo > 1e-3 * hi else np.float32(0.0)
        moving += mid != 0
        for fs in (fs_g, fs_c):
            sl = slice(fs.seg_start[i], fs.seg_start[i + 1])
            fs._stat["t_ttft"][sl] = mid
            fs._stat["t_itl"][sl] = 0.0
    assert moving >= 3
    cpu, gpu = fs_c.lag_path(averages=True, **kw), fs_g.lag_path(averages=True, **kw)
    ok = cpu.status == LAG_OK
    assert cpu.violated_avg.any() and not cpu.violated_avg[ok].all()
    assert (cpu.violated_avg != cpu.violated).any()
    for f in ("status", "steps", "violated", "violated_avg"):
        assert np.array_equal(getattr(cpu, f), getattr(gpu, f)), f
    for f in ("ttft", "itl", "rho", "blocked", "ttft_avg", "itl_avg", "rho_avg", "blocked_avg"):
        a, b = getattr(cpu, f), getattr(gpu, f)
        assert np.array_equal(np.isnan(a), np.isnan(b)), f
        m = ~np.isnan(a)
        # the bound of test_gpu_lag_path_matches_cpu: TOL relative to the
        # quantity's scale, plus half an fp32 ulp of each side
        bound = TOL * np.maximum(np.abs(a[m]), 1.0) + 0.5 * (np.spacing(np.abs(a[m]))
                                                            + np.spacing(np.abs(b[m])))
        assert (np.abs(a[m].astype(np.float64) - b[m]) <= bound).all(), f
    # the default call is the call without the keyword, to the bit
    plain = fs_g.lag_path(**kw)
    assert plain.ttft_avg is None and plain.violated_avg is None
    for f in ("ttft", "itl", "wait", "blocked", "rho", "in_system"):
        assert np.array_equal(getattr(plain, f).view(np.int32), getattr(gpu, f).view(np.int32)), f


def test_lag_path_averages_change_nothing_else():
    fs, _, kw = fleet(n_t=4)
    w1 = fs.reconcile()
    g = fs._gpu
    before = (fs.memo_stats(), g.fused_state(), g.stale_ticks, g.bucket_key)
    fs.lag_path(averages=True, **kw)
    assert (fs.memo_stats(), g.fused_state(), g.stale_ticks, g.bucket_key) == before
    w2 = fs.reconcile()
    fresh = FastSweep(lag_system(), backend="gpu")
    t1, t2 = fresh.reconcile(), fresh.reconcile()
    for f in ("acc_idx", "num_replicas", "batch", "cost", "value", "itl", "ttft", "rho",
              "max_rate"):
        for a, b in ((w1, t1), (w2, t2)):
            assert np.array_equal(getattr(a, f).view(np.int32), getattr(b, f).view(np.int32)), f
