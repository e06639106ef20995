"""Wide lag on the GPU: the tiled kernels through run_lag_wide_probe against the
longdouble reference of tests/test_lag_cpu.py (never against the one-block
kernel or themselves), and FastSweep.lag(max_n=...) against the CPU backend.

Tolerance max(8 x WIDE_GOLDEN_MAX_ERR, 1e-12) = 1e-12 on blocked, rho and
wait * s(N) / Q, the rule of tests/test_lag_gpu.py.

Measured on MI355X: largest absolute error 9.36e-14 (N = 1118, production
stride and halo, the start near the full queue into overload), 1780 steps per
task; the other tiling of N = 1118 gives 9.35e-14.
"""
import numpy as np
import pytest

from inferno_amd.engine import LAG_OK, LAG_TOO_WIDE, LAG_WIDE_MAX_N, FastSweep
from inferno_amd.ops.sweep import LAG_MAX_N, LAG_WIDE_HALO, LAG_WIDE_STRIDE, run_lag_wide_probe
from tests.test_lag_cpu import IN_TOK, OUT_TOK, PERF, analyzer, normalised, reference
from tests.test_lag_wide_cpu import WIDE_GOLDEN_MAX_ERR, regimes
from tests.test_plan_gpu import build_system

pytestmark = pytest.mark.gpu

TOL = max(8 * WIDE_GOLDEN_MAX_ERR, 1e-12)


# the first N the one-block classes refuse, two tiles; the head crosses a cut,
# 17 tiles, several segments per interval, j_lo inside one; the smallest halo,
# one lane; 11 N + 1 padded to 12672 = 11 x 1152 slots: the last tile is full
@pytest.mark.parametrize("n,stride,halo", [(1118, LAG_WIDE_STRIDE, LAG_WIDE_HALO),
                                           (1118, 768, 96), (1200, 1536, 24), (1150, 1152, 96)])
def test_wide_probe_matches_longdouble(n, stride, halo):
    qa = analyzer(n)
    one = {k: np.full(1, v, dtype=np.float32) for k, v in PERF.items()}
    one.update(in_tok=np.full(1, IN_TOK, dtype=np.int32), out_tok=np.full(1, OUT_TOK, dtype=np.int32),
               batch_n=np.full(1, n, dtype=np.int32))
    worst = 0.0
    for c, (lam0, lam1, dt) in enumerate(regimes(qa)):  # one probe per regime
        times = (dt[0] / 1000.0, (dt[0] + dt[1]) / 1000.0)
        raw, steps = run_lag_wide_probe(one, np.array([lam0]), np.array([lam1]), times,
                                        stride=stride, halo=halo)
        dt = (times[0] * 1000.0, (times[1] - times[0]) * 1000.0)  # as the probe forms them
        ref = reference(qa.serv_rate, lam0, lam1, dt)
        assert 0 < steps[0] <= 3000
        err = float(np.abs(normalised(raw[0], qa.serv_rate) - ref).max())
        print(f"N={n} S={stride} T={halo} regime {c}: steps {steps[0]}, max abs err {err:.3g}")
        worst = max(worst, err)
        if c == 1:
            assert raw[0, 1, 0] > 0.1  # blocked
    assert worst <= TOL


def test_gpu_wide_lag_matches_cpu_lag():
    fs_g = FastSweep(build_system(), backend="gpu")
    fs_c = FastSweep(build_system(), backend="cpu")
    base = fs_c._base_load()[0]
    n_srv = len(fs_c.server_names)
    acc = np.array([int(fs_c.cell_acc_idx[fs_c.seg_start[i]]) for i in range(n_srv)])
    kw = dict(arrival=np.stack([base * 3, base * 0, base]).astype(np.float32),
              allocation=(acc, np.full(n_srv, 64)), times=(0.5, 1.0, 2.0))
    fs_g.reconcile()
    g = fs_g._gpu
    before = (fs_g.memo_stats(), g.fused_state(), g.stale_ticks, g.bucket_key)
    narrow = fs_g.lag(**kw)
    gpu = fs_g.lag(max_n=LAG_WIDE_MAX_N, **kw)
    assert (fs_g.memo_stats(), g.fused_state(), g.stale_ticks, g.bucket_key) == before
    cpu = fs_c.lag(max_n=LAG_WIDE_MAX_N, **kw)
    system = build_system()
    n_of = np.array([system.servers[name].max_batch_size for name in sorted(system.servers)])
    wide = (n_of > LAG_MAX_N) & (n_of <= LAG_WIDE_MAX_N)  # 2048, 2049 twice, 8193; not 32769
    assert (n_of[wide] == 2049).sum() == 2 and (n_of > LAG_WIDE_MAX_N).any()
    assert (narrow.status[:, n_of > LAG_MAX_N] == LAG_TOO_WIDE).all()
    assert (cpu.status[:, wide] == LAG_OK).all() and (gpu.status[:, wide] == LAG_OK).all()
    assert np.array_equal(narrow.status[:, ~wide], gpu.status[:, ~wide])
    for f in ("status", "steps", "first_violation", "violated", "held_replicas", "acc_idx"):
        assert np.array_equal(getattr(cpu, f), getattr(gpu, f)), f
    for f in ("ttft", "itl", "wait", "blocked", "rho", "in_system"):
        a, b = getattr(cpu, f), getattr(gpu, f)
        assert np.array_equal(np.isnan(a), np.isnan(b)), f
        m = ~np.isnan(a)
        bound = TOL * np.maximum(np.abs(a[m]), 1.0) + 0.5 * (np.spacing(np.abs(a[m]))
                                                            + np.spacing(np.abs(b[m])))
        assert (np.abs(a[m].astype(np.float64) - b[m]) <= bound).all(), f
