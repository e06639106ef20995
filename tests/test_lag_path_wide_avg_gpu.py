"""Wide lag path averages on the GPU: wva_lag_path_avg_tile_t (two blocks per
tile) through run_lag_path_wide_probe(averages=True) against the longdouble
direct sum (never against the one-block kernel or themselves), and
FastSweep.lag_path(max_n=..., averages=True) against the CPU backend.

Tolerance max(8 x WIDE_PATH_AVG_GOLDEN_MAX_ERR, 1e-12) = 1e-12 on blocked, rho
and wait * s(N) / Q, the rule of tests/test_lag_path_gpu.py.

Measured on MI355X, largest absolute error of the averaged half per tiling
(N, S, T), beside the golden's at that N: (1118, 10752, 768) 1.59e-15 and
(1118, 768, 96) 1.59e-15 (golden 1.41e-15), (1200, 1536, 24) 1.51e-15 (golden
1.36e-15), (1150, 1152, 96) 6.32e-16 (golden 6.32e-16); with j_lo = 0 in every
tick 5.12e-17 at both tilings (golden 1.0e-16). 2639 steps per cell in 5, 29,
112 and 29 segments.
"""
import numpy as np
import pytest

from inferno_amd.engine import LAG_OK, LAG_WIDE_MAX_N, FastSweep
from inferno_amd.ops.sweep import (LAG_MAX_N, LAG_WIDE_HALO, LAG_WIDE_STRIDE,
                                   run_lag_path_wide_probe)
from tests.test_lag_cpu import IN_TOK, OUT_TOK, PERF, normalised
from tests.test_lag_path_wide_avg_cpu import WIDE_PATH_AVG_GOLDEN_MAX_ERR, wide_avg_case
from tests.test_lag_path_wide_cpu import TILINGS
from tests.test_plan_gpu import build_system

pytestmark = pytest.mark.gpu

TOL = max(8 * WIDE_PATH_AVG_GOLDEN_MAX_ERR, 1e-12)
# every window starts at j_lo = 0: no below-window phase, T_0 v_0 seeds the sum
NO_LOWER = [(1118, LAG_WIDE_STRIDE, LAG_WIDE_HALO, True), (1118, 768, 96, True)]


@pytest.mark.parametrize("n,stride,halo,short", [t + (False,) for t in TILINGS] + NO_LOWER)
def test_wide_avg_probe_matches_longdouble(n, stride, halo, short):
    qa, lam, keep, tick_s, starts, refs = wide_avg_case(n, short)
    arrays = {k: np.full(2, v, dtype=np.float32) for k, v in PERF.items()}
    arrays.update(in_tok=np.full(2, IN_TOK, dtype=np.int32),
                  out_tok=np.full(2, OUT_TOK, dtype=np.int32),
                  batch_n=np.full(2, n, dtype=np.int32))
    args = (arrays, list(starts), np.tile(lam, (2, 1)), np.tile(keep, (2, 1)), tick_s)
    raw, avg, steps, n_seg = run_lag_path_wide_probe(*args, stride=stride, halo=halo,
                                                     averages=True)
    end, end_steps, end_seg = run_lag_path_wide_probe(*args, stride=stride, halo=halo)
    # the state blocks are wva_lag_path_tile_t to the bit
    assert np.array_equal(raw.view(np.int64), end.view(np.int64))
    assert np.array_equal(steps, end_steps) and np.array_equal(n_seg, end_seg)
    err = max(float(np.abs(normalised(avg[c], qa.serv_rate) - refs[c]).max()) for c in range(2))
    print(f"N={n} S={stride} T={halo} short={short}: steps {steps[0].tolist()}, segments "
          f"{n_seg[0]}, averaged max abs err {err:.3g}")
    assert err <= TOL
    if not short:
        assert (avg[:, 2, 1] > raw[:, 2, 1]).all()  # the drain tick: busier on average


def test_gpu_wide_lag_path_averages_match_cpu():
    fs_g = FastSweep(build_system(), backend="gpu")
    fs_c = FastSweep(build_system(), backend="cpu")
    system = build_system()
    n_of = np.array([system.servers[name].max_batch_size for name in sorted(system.servers)])
    wide = (n_of > LAG_MAX_N) & (n_of <= LAG_WIDE_MAX_N)  # 2048, 2049 twice, 8193; not 32769
    base = fs_c._base_load()[0]
    n_srv, n_t = len(fs_c.server_names), 6
    first = np.array([int(fs_c.cell_acc_idx[fs_c.seg_start[i]]) for i in range(n_srv)])
    acc = np.tile(first, (n_t, 1))
    rep = np.full((n_t, n_srv), 64)
    two = [i for i in np.nonzero(wide)[0] if fs_c.seg_start[i + 1] - fs_c.seg_start[i] >= 2]
    change, out = two[0], next(i for i in np.nonzero(wide)[0] if i != two[0])
    acc[3:, change] = int(fs_c.cell_acc_idx[fs_c.seg_start[change] + 1])  # a run from empty
    rep[2:, out] = 128  # scale-out mid-path
    scen = (base[None, :] * np.linspace(3.0, 0.5, n_t)[:, None]).astype(np.float32)
    kw = dict(arrival=scen, allocation=(acc, rep), delay=0, start_allocation=(first, rep[0]),
              tick_seconds=8.0)
    probe = fs_c.lag_path(max_n=LAG_WIDE_MAX_N, averages=True, **kw)
    # TTFT targets midway between the golden's averaged values at the first two
    # ticks, none where it moves by less than 1e-3 relative
    moving = 0
    for i in range(n_srv):
        lo, hi = sorted((float(probe.ttft_avg[0, i]), float(probe.ttft_avg[1, i])))
        mid = np.float32(0.5 * (lo + hi)) if hi - lo > 1e-3 * hi else np.float32(0.0)
        moving += mid != 0
        for fs in (fs_g, fs_c):
            sl = slice(fs.seg_start[i], fs.seg_start[i + 1])
            fs._stat["t_ttft"][sl] = mid
            fs._stat["t_itl"][sl] = 0.0
    assert moving >= 3
    fs_g.reconcile()
    g = fs_g._gpu
    before = (fs_g.memo_stats(), g.fused_state(), g.stale_ticks, g.bucket_key)
    plain = fs_g.lag_path(max_n=LAG_WIDE_MAX_N, **kw)
    narrow = fs_g.lag_path(averages=True, **kw)
    gpu = fs_g.lag_path(max_n=LAG_WIDE_MAX_N, averages=True, **kw)
    assert (fs_g.memo_stats(), g.fused_state(), g.stale_ticks, g.bucket_key) == before
    cpu = fs_c.lag_path(max_n=LAG_WIDE_MAX_N, averages=True, **kw)
    assert (gpu.status[:, wide] == LAG_OK).all()
    assert np.array_equal(cpu.violated_avg, gpu.violated_avg)
    assert cpu.violated_avg[:, wide].any() and not cpu.violated_avg[:, wide].all()
    for f in ("status", "steps", "violated", "ttft", "itl", "wait", "blocked", "rho",
              "in_system"):  # the end state is the call without averages, to the bit
        a, b = getattr(plain, f), getattr(gpu, f)
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), f
    for f in ("ttft_avg", "itl_avg", "rho_avg", "blocked_avg"):
        a, b = getattr(cpu, f), getattr(gpu, f)
        assert np.isfinite(b[:, wide]).all(), f
        assert np.array_equal(np.isnan(a), np.isnan(b)), f
        m = ~np.isnan(a)
        bound = TOL * np.maximum(np.abs(a[m]), 1.0) + 0.5 * (np.spacing(np.abs(a[m]))
                                                            + np.spacing(np.abs(b[m])))
        assert (np.abs(a[m].astype(np.float64) - b[m]) <= bound).all(), f
        a, b = getattr(narrow, f)[:, ~wide], b[:, ~wide]  # the one-block pass is untouched
        assert np.array_equal(a, b, equal_nan=True), f
    assert np.array_equal(narrow.violated_avg[:, ~wide], gpu.violated_avg[:, ~wide])
