"""Lag paths on the GPU: wva_lag_path_t through run_lag_path_probe, and
FastSweep.lag_path against the CPU backend.

The probe is compared with the longdouble path reference of
tests/test_lag_path_cpu.py (never with the GPU's own output) at the first and
last N of every kernel instantiation, once as one chunk and once cut 2 + 2 so
that the state goes through the carry, within max(8 x PATH_GOLDEN_MAX_ERR,
1e-12) on blocked, rho and wait * s(N) / Q, which all lie in [0, 1].

Measured on MI355X: largest absolute error 5.13e-14 (N = 11), the same as one
chunk and through the carry; 2639 steps per cell; tolerance 1e-12.
"""
import numpy as np
import pytest

from inferno_amd.engine import LAG_OK, LAG_TOO_WIDE, FastSweep
from inferno_amd.ops.sweep import run_lag_path_probe
from tests.test_lag_cpu import IN_TOK, OUT_TOK, PERF, analyzer, normalised
from tests.test_lag_gpu import lag_system
from tests.test_lag_path_cpu import PATH_GOLDEN_MAX_ERR, STEPS, path_reference

pytestmark = pytest.mark.gpu

TOL = max(8 * PATH_GOLDEN_MAX_ERR, 1e-12)


@pytest.mark.parametrize("n", (1, 11, 12, 69, 70, 279, 280, 1024))
def test_path_probe_matches_longdouble(n):
    qa = analyzer(n)
    lmax = qa.rate_max / 1000.0
    # overload, scale-out to twice the replicas, drain, moderate load
    lam = np.array([1.5, 0.75, 0.0, 0.7]) * lmax
    keep = np.array([1.0, 0.5, 1.0, 1.0])
    tick_s = STEPS / (1.5 * lmax + float(qa.serv_rate.max())) / 1000.0
    starts = [("stationary", 0.5 * lmax), "empty"]  # two cells: one per kind of start
    arrays = {k: np.full(2, v, dtype=np.float32) for k, v in PERF.items()}
    arrays.update(in_tok=np.full(2, IN_TOK, dtype=np.int32),
                  out_tok=np.full(2, OUT_TOK, dtype=np.int32),
                  batch_n=np.full(2, n, dtype=np.int32))
    ref = [path_reference(qa.serv_rate, s, lam, keep, tick_s * 1000.0) for s in starts]
    assert ref[0][0, 1] > ref[0][2, 1]  # busier after the overload than after the drain
    args = (arrays, starts, np.tile(lam, (2, 1)), np.tile(keep, (2, 1)), tick_s)
    raw, steps, bounds = run_lag_path_probe(*args)
    assert list(bounds) == [0, 4] and (steps > 0).all() and steps.sum(axis=1).max() <= 3000
    cut = int(steps[0, :2].sum())  # the third tick no longer fits: chunks of 2 + 2
    raw2, steps2, bounds2 = run_lag_path_probe(*args, max_steps=cut)
    assert list(bounds2) == [0, 2, 4] and np.array_equal(steps, steps2)
    worst = 0.0
    for what, got in (("one chunk", raw), ("2 + 2", raw2)):
        err = max(float(np.abs(normalised(got[c], qa.serv_rate) - ref[c]).max()) for c in range(2))
        print(f"N={n} {what}: steps {steps[0].tolist()}, max abs err {err:.3g}")
        worst = max(worst, err)
    assert worst <= TOL


def fleet(n_t=20):
    fs_g = FastSweep(lag_system(), backend="gpu")
    fs_c = FastSweep(lag_system(), backend="cpu")
    base = fs_c._base_load()[0]
    n_srv = len(fs_c.server_names)
    first = np.array([int(fs_c.cell_acc_idx[fs_c.seg_start[i]]) for i in range(n_srv)])
    acc = np.tile(first, (n_t, 1))
    rep = np.full((n_t, n_srv), 64)
    two = next(i for i in range(n_srv) if fs_c.seg_start[i + 1] - fs_c.seg_start[i] >= 2)
    acc[n_t // 2:, two] = int(fs_c.cell_acc_idx[fs_c.seg_start[two] + 1])  # accelerator change
    rep[n_t // 2 + 2:, (two + 1) % n_srv] = 128  # scale-out
    scen = (base[None, :] * np.linspace(3.0, 0.5, n_t)[:, None]).astype(np.float32)
    kw = dict(arrival=scen, allocation=(acc, rep), delay=1, start_allocation=(first, rep[0]),
              tick_seconds=2.0)
    return fs_g, fs_c, kw


def test_gpu_lag_path_matches_cpu():
    fs_g, fs_c, kw = fleet()
    first = fs_c.lag_path(**kw)
    assert (first.status == LAG_OK).any() and (first.status == LAG_TOO_WIDE).any()
    # TTFT targets midway between the golden's values at the first two ticks; no
    # target (0) where the TTFT does not move by at least 1e-3 relative, so that
    # no verdict sits within rounding of its target
    moving = 0
    for i in range(len(fs_c.server_names)):
        lo, hi = sorted((float(first.ttft[0, i]), float(first.ttft[1, i])))
        mid = np.float32(0.5 * (lo + hi)) if hi - lo > 1e-3 * hi else np.float32(0.0)
        moving += mid != 0
        for fs in (fs_g, fs_c):
            sl = slice(fs.seg_start[i], fs.seg_start[i + 1])
            fs._stat["t_ttft"][sl] = mid
            fs._stat["t_itl"][sl] = 0.0
    assert moving >= 3
    cpu, gpu = fs_c.lag_path(**kw), fs_g.lag_path(**kw)
    assert cpu.violated.any() and not cpu.violated[cpu.status == LAG_OK].all()
    for f in ("status", "steps", "violated", "first_violation", "ticks_violated",
              "held_replicas", "acc_idx"):
        assert np.array_equal(getattr(cpu, f), getattr(gpu, f)), f
    for f in ("ttft", "itl", "wait", "blocked", "rho", "in_system"):
        a, b = getattr(cpu, f), getattr(gpu, f)
        assert np.array_equal(np.isnan(a), np.isnan(b)), f
        m = ~np.isnan(a)
        # TOL is relative to the quantity's scale (the probe's quantities are
        # normalised to [0, 1]), plus half an fp32 ulp of each side
        bound = TOL * np.maximum(np.abs(a[m]), 1.0) + 0.5 * (np.spacing(np.abs(a[m]))
                                                            + np.spacing(np.abs(b[m])))
        assert (np.abs(a[m].astype(np.float64) - b[m]) <= bound).all(), f


def test_lag_path_changes_nothing_else():
    fs, _, kw = fleet(n_t=4)
    w1 = fs.reconcile()
    g = fs._gpu
    before = (fs.memo_stats(), g.fused_state(), g.stale_ticks, g.bucket_key)
    fs.lag_path(**kw)
    assert (fs.memo_stats(), g.fused_state(), g.stale_ticks, g.bucket_key) == before
    w2 = fs.reconcile()
    fresh = FastSweep(lag_system(), backend="gpu")
    t1, t2 = fresh.reconcile(), fresh.reconcile()
    for f in ("acc_idx", "num_replicas", "batch", "cost", "value", "itl", "ttft", "rho",
              "max_rate"):
        for a, b in ((w1, t1), (w2, t2)):
            assert np.array_equal(getattr(a, f).view(np.int32), getattr(b, f).view(np.int32)), f
