"""Lag analysis on the GPU: wva_lag_t through run_lag_probe, and FastSweep.lag
against the CPU backend.

The probe is compared with the longdouble reference of tests/test_lag_cpu.py
(never with the GPU's own output) at the first and last N of every kernel
instantiation, within max(8 x GOLDEN_MAX_ERR, 1e-12) on blocked, rho and
wait * s(N) / Q, which all lie in [0, 1].

Measured on MI355X: largest absolute error 1.14e-13 (N = 1024, start near the
full queue into overload), 1780 steps per task; tolerance 6.08e-13.
"""
import numpy as np
import pytest

from inferno_amd.engine import LAG_OK, LAG_TOO_WIDE, FastSweep
from inferno_amd.ops.sweep import run_lag_probe
from tests.test_lag_cpu import (GOLDEN_MAX_ERR, IN_TOK, OUT_TOK, PERF, analyzer, normalised,
                                reference)
from tests.test_plan_gpu import INFEASIBLE_SRV, build_system

pytestmark = pytest.mark.gpu

TOL = max(8 * GOLDEN_MAX_ERR, 1e-12)
STEPS = 600.0  # uniformization steps per checkpoint interval, about


@pytest.mark.parametrize("n", (1, 11, 12, 69, 70, 279, 280, 1024))
def test_probe_matches_longdouble(n):
    qa = analyzer(n)
    lmax = qa.rate_max / 1000.0
    # cold start into overload; a start already near the full queue into a
    # heavier overload (blocked > 0.1); warm start draining
    regimes = ((0.0, 1.5 * lmax), (1.05 * lmax, 3.0 * lmax), (0.9 * lmax, 0.0))
    lam0 = np.array([r[0] for r in regimes])
    lam1 = np.array([r[1] for r in regimes])
    smax = float(qa.serv_rate.max())
    arrays = {k: np.full(3, v, dtype=np.float32) for k, v in PERF.items()}
    arrays.update(in_tok=np.full(3, IN_TOK, dtype=np.int32),
                  out_tok=np.full(3, OUT_TOK, dtype=np.int32),
                  batch_n=np.full(3, n, dtype=np.int32))
    worst = 0.0
    for c in range(3):  # one probe per regime: each has its own time scale
        t1 = STEPS / (lam1[c] + smax) / 1000.0
        times = (t1, 2.0 * t1)
        one = {k: v[c:c + 1] for k, v in arrays.items()}
        raw, steps = run_lag_probe(one, lam0[c:c + 1], lam1[c:c + 1], times)
        dt = (times[0] * 1000.0, (times[1] - times[0]) * 1000.0)
        ref = reference(qa.serv_rate, lam0[c], lam1[c], dt)
        assert 0 < steps[0] <= 3000
        err = float(np.abs(normalised(raw[0], qa.serv_rate) - ref).max())
        print(f"N={n} regime {c}: steps {steps[0]}, max abs err {err:.3g}")
        worst = max(worst, err)
        if c == 1:
            assert raw[0, 1, 0] > 0.1  # blocked
    assert worst <= TOL


def lag_system():
    """The 27-cell fleet; its second N = 2049 server is pinned to N = 200 here,
    so that a context pass also launches the 256-wide class (the fleet's own
    sizes give 1, 33, 512, 513 and LAG_TOO_WIDE)."""
    system = build_system()
    system.servers[sorted(system.servers)[INFEASIBLE_SRV]].max_batch_size = 200
    return system


def fleet():
    fs_g = FastSweep(lag_system(), backend="gpu")
    fs_c = FastSweep(lag_system(), backend="cpu")
    base = fs_c._base_load()[0]
    n_srv = len(fs_c.server_names)
    acc = np.array([int(fs_c.cell_acc_idx[fs_c.seg_start[i]]) for i in range(n_srv)])
    rep = np.full(n_srv, 64)
    scen = np.stack([base * 3, base * 0, base]).astype(np.float32)
    return fs_g, fs_c, scen, acc, rep


def test_gpu_lag_matches_cpu_lag():
    fs_g, fs_c, scen, acc, rep = fleet()
    kw = dict(arrival=scen, allocation=(acc, rep), times=(0.5, 1.0, 2.0))
    first = fs_c.lag(**kw)
    ok = first.status == LAG_OK
    assert ok.any() and (first.status == LAG_TOO_WIDE).any()
    # TTFT targets midway between the golden's values at the first two
    # checkpoints of the overload scenario; no target (0) where the TTFT does not
    # move by at least 1e-3 relative (the TPS-target server: its rate ignores the
    # scenario), so that no verdict sits within rounding of its target
    moving = 0
    for i in range(len(fs_c.server_names)):
        lo, hi = sorted((float(first.ttft[0, 0, i]), float(first.ttft[1, 0, i])))
        mid = np.float32(0.5 * (lo + hi)) if hi - lo > 1e-3 * hi else np.float32(0.0)
        moving += mid != 0
        for fs in (fs_g, fs_c):
            sl = slice(fs.seg_start[i], fs.seg_start[i + 1])
            fs._stat["t_ttft"][sl] = mid
            fs._stat["t_itl"][sl] = 0.0
    assert moving >= 3
    cpu, gpu = fs_c.lag(**kw), fs_g.lag(**kw)
    assert cpu.violated.any() and not cpu.violated.all(axis=0)[cpu.status == LAG_OK].all()
    for f in ("status", "steps", "first_violation", "violated", "held_replicas", "acc_idx"):
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


def test_lag_changes_nothing_else():
    fs, _, scen, acc, rep = fleet()
    w1 = fs.reconcile()
    g = fs._gpu
    before = (fs.memo_stats(), g.fused_state(), g.stale_ticks, g.bucket_key)
    fs.lag(arrival=scen, allocation=(acc, rep), times=(0.5, 1.0))
    assert (fs.memo_stats(), g.fused_state(), g.stale_ticks, g.bucket_key) == before
    w2 = fs.reconcile()
    fresh = FastSweep(lag_system(), backend="gpu")
    t1, t2 = fresh.reconcile(), fresh.reconcile()
    for f in ("acc_idx", "num_replicas", "batch", "cost", "value", "itl", "ttft", "rho",
              "max_rate"):
        for a, b in ((w1, t1), (w2, t2)):
            assert np.array_equal(getattr(a, f).view(np.int32), getattr(b, f).view(np.int32)), f
