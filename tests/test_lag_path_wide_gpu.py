"""Wide lag paths on the GPU: the tiled path kernels through
run_lag_path_wide_probe against the longdouble path reference (never against
the one-block kernel or themselves), and FastSweep.lag_path(max_n=...) against
the CPU backend.

Tolerance max(8 x WIDE_PATH_GOLDEN_MAX_ERR, 1e-12) = 1e-12 on blocked, rho and
wait * s(N) / Q, the rule of tests/test_lag_path_gpu.py.

Measured on MI355X: largest absolute error 3.12e-15 (N = 1118, at the
production stride and halo and at S = 768, T = 96 alike; 3.03e-15 at N = 1200,
1.54e-15 at N = 1150), 2639 steps per cell in 5, 29, 112 and 29 segments.
"""
import time

import numpy as np
import pytest

from inferno_amd.engine import LAG_OK, LAG_TOO_WIDE, LAG_WIDE_MAX_N, FastSweep
from inferno_amd.ops.sweep import LAG_MAX_N, run_lag_path_wide_probe
from tests.test_lag_cpu import IN_TOK, OUT_TOK, PERF, normalised
from tests.test_lag_path_wide_cpu import TILINGS, WIDE_PATH_GOLDEN_MAX_ERR, wide_path_case
from tests.test_plan_gpu import build_system

pytestmark = pytest.mark.gpu

TOL = max(8 * WIDE_PATH_GOLDEN_MAX_ERR, 1e-12)


@pytest.mark.parametrize("n,stride,halo", TILINGS)
def test_wide_path_probe_matches_longdouble(n, stride, halo):
    qa, lam, keep, tick_s, starts, refs = wide_path_case(n)
    assert refs[0][0, 1] > refs[0][2, 1]  # busier after the overload than after the drain
    arrays = {k: np.full(2, v, dtype=np.float32) for k, v in PERF.items()}
    arrays.update(in_tok=np.full(2, IN_TOK, dtype=np.int32),
                  out_tok=np.full(2, OUT_TOK, dtype=np.int32),
                  batch_n=np.full(2, n, dtype=np.int32))
    raw, steps, n_seg = run_lag_path_wide_probe(arrays, list(starts), np.tile(lam, (2, 1)),
                                                np.tile(keep, (2, 1)), tick_s, stride=stride,
                                                halo=halo)
    assert (steps > 0).all() and steps.sum(axis=1).max() <= 3000
    assert (n_seg == (-(-steps // halo)).sum(axis=1)).all()  # no segment crosses a tick
    err = max(float(np.abs(normalised(raw[c], qa.serv_rate) - refs[c]).max()) for c in range(2))
    print(f"N={n} S={stride} T={halo}: steps {steps[0].tolist()}, segments {n_seg[0]}, "
          f"max abs err {err:.3g}")
    assert raw[0, 0, 1] > raw[0, 2, 1]  # the path did something
    assert err <= TOL


def test_gpu_wide_lag_path_matches_cpu():
    fs_g = FastSweep(build_system(), backend="gpu")
    fs_c = FastSweep(build_system(), backend="cpu")
    system = build_system()
    n_of = np.array([system.servers[name].max_batch_size for name in sorted(system.servers)])
    wide = (n_of > LAG_MAX_N) & (n_of <= LAG_WIDE_MAX_N)  # 2048, 2049 twice, 8193; not 32769
    assert wide.sum() == 4 and (n_of > LAG_WIDE_MAX_N).any() and (n_of <= LAG_MAX_N).any()
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
    # 8 s ticks: 150 to 860 steps each, so the N = 2049 run with the scale-out has
    # two segments per tick at the production halo. The CPU backend walks every
    # state of every wide run: 1.7 s for this call (measured, printed below)
    t0 = time.perf_counter()
    probe = fs_c.lag_path(max_n=LAG_WIDE_MAX_N, **kw)
    print(f"CPU backend, max_n={LAG_WIDE_MAX_N}: {time.perf_counter() - t0:.2f} s")
    assert (probe.status[:, wide] == LAG_OK).all()
    # TTFT targets midway between the golden's values at the first two ticks, none
    # where the TTFT moves by less than 1e-3 relative: no verdict sits on rounding
    moving = 0
    for i in range(n_srv):
        lo, hi = sorted((float(probe.ttft[0, i]), float(probe.ttft[1, i])))
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
    narrow = fs_g.lag_path(**kw)
    gpu = fs_g.lag_path(max_n=LAG_WIDE_MAX_N, **kw)
    assert (fs_g.memo_stats(), g.fused_state(), g.stale_ticks, g.bucket_key) == before
    cpu = fs_c.lag_path(max_n=LAG_WIDE_MAX_N, **kw)
    assert fs_g.lag_path_pass["wide_tasks"] == 5  # four servers, one of them in two runs
    assert (narrow.status[:, n_of > LAG_MAX_N] == LAG_TOO_WIDE).all()
    assert (gpu.status[:, wide] == LAG_OK).all()
    assert (gpu.status[:, n_of > LAG_WIDE_MAX_N] == LAG_TOO_WIDE).all()
    assert cpu.violated[:, wide].any() and not cpu.violated[:, wide].all()
    assert gpu.in_system[3, change] < gpu.in_system[2, change]  # the new run started empty
    for f in ("status", "steps", "violated", "first_violation", "ticks_violated",
              "held_replicas", "acc_idx"):
        assert np.array_equal(getattr(cpu, f), getattr(gpu, f)), f
    for f in ("status", "steps", "violated", "held_replicas", "acc_idx", "ttft", "itl", "wait",
              "blocked", "rho", "in_system"):  # the default call is the max_n call elsewhere
        a, b = getattr(narrow, f)[:, ~wide], getattr(gpu, f)[:, ~wide]
        assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), f
    for f in ("ttft", "itl", "wait", "blocked", "rho", "in_system"):
        a, b = getattr(cpu, f), getattr(gpu, f)
        assert np.array_equal(np.isnan(a), np.isnan(b)), f
        m = ~np.isnan(a)
        # TOL is relative to the quantity's scale (the probe's quantities are
        # normalised to [0, 1]), plus half an fp32 ulp of each side
        bound = TOL * np.maximum(np.abs(a[m]), 1.0) + 0.5 * (np.spacing(np.abs(a[m]))
                                                            + np.spacing(np.abs(b[m])))
        assert (np.abs(a[m].astype(np.float64) - b[m]) <= bound).all(), f
