"""Percentile TTFT planning on the GPU: the tail evaluator and the percentile
sizing (ops.sweep.run_tail_probe) against the 60-digit mpmath reference of
tests/test_plan_tail_cpu.py, and FastSweep.plan_tail against its own single
slices and against the CPU backend.

Probe cells: N = 1, 2, 33, 64, 600 run as one wave, N = 2049 as a 256-thread
block; the grid clips the window at 0 (x < 1) and at Q - 1 (x beyond Q), and
takes both closed-form branches of the remainder.

Tolerance of the tail values: 8 x the golden's measured maximum error, floor
1e-13 (TAIL_TOL = 7.1e-13).

Measured on the MI355X: largest absolute error of the probe 5.97e-14 (N = 2049;
4.8e-16 at N = 1); 0 replica flips of 96 against the CPU backend.
"""
import mpmath
import numpy as np
import pytest
import torch

from inferno_amd.engine import FastSweep
from inferno_amd.ops.sweep import run_tail_probe
from tests.test_plan_gpu import ZERO_SRV, base_loads, bits, build_system, make_planner
from tests.test_plan_tail_cpu import (GOLDEN_MAX_ERR, GRID_N, IN_TOK, OUT_TOK, PERF, fleet,
                                      mp_tail, reference)

pytestmark = pytest.mark.gpu

WVA_TOL = 1e-6
TAIL_TOL = max(8.0 * GOLDEN_MAX_ERR, 1e-13)
QS = (0.5, 0.9, 0.99)


def probe_arrays(t_ttft):
    n = len(GRID_N)
    i32 = lambda v: torch.full((n,), v, dtype=torch.int32)  # noqa: E731
    f32 = lambda v: torch.full((n,), v, dtype=torch.float32)  # noqa: E731
    arrays = {k: f32(v) for k, v in PERF.items()}
    arrays.update(in_tok=i32(IN_TOK), out_tok=i32(OUT_TOK), t_tps=f32(0.0),
                  batch_n=torch.tensor(GRID_N, dtype=torch.int32),
                  t_ttft=torch.tensor(t_ttft, dtype=torch.float32))
    return arrays


def test_probe_tail_matches_mpmath():
    refs = [reference(n) for n in GRID_N]
    lam = np.array([[p[0] for p in pts] for _, pts in refs])
    t = np.array([[p[1] for p in pts] for _, pts in refs])
    tail, _, _ = run_tail_probe(probe_arrays([0.0] * len(GRID_N)), lam, t)
    for row, (n, (_, pts)) in enumerate(zip(GRID_N, refs)):
        err = [float(abs(mpmath.mpf(float(tail[row, i])) - p[2])) for i, p in enumerate(pts)]
        print(f"N={n}: probe max abs error {max(err):.3e}")
        assert max(err) <= TAIL_TOL, (n, err)


def binding_ttft(qa):
    """A TTFT target inside the reachable range of every quantile of QS: the
    prefill time at full batch plus two departures' time."""
    return float(np.float32(qa.service_parms.prefill.prefill_time(IN_TOK, qa.chain.N)
                            + 2.0 / float(qa.serv_rate[-1])))


def mp_g(qa, lam, t_ttft):
    """g(lam) with the tail in mpmath; the budget as the golden forms it."""
    from inferno_amd.analyzer.queue import effective_concurrency

    st = qa.chain.solve(lam)
    eff = effective_concurrency(st.avg_serv_time, qa.service_parms, qa.request_size, qa.chain.N)
    return mp_tail(qa, lam, t_ttft - qa.service_parms.prefill.prefill_time(IN_TOK, eff))


@pytest.mark.parametrize("kind", ("binding", "below", "above"))
def test_probe_sizing_matches_mpmath(kind):
    qas = [reference(n)[0] for n in GRID_N]
    t_ttft = {"binding": [binding_ttft(qa) for qa in qas],
              "below": [1e-3] * len(qas),  # under the prefill time: g = 1 at every rate
              "above": [1e7] * len(qas)}[kind]
    none = np.zeros((len(qas), 0))
    _, lam_q, ind = run_tail_probe(probe_arrays(t_ttft), none, none, QS)
    if kind != "binding":
        assert (ind == (-1 if kind == "below" else 1)).all()
        return
    assert (ind == 0).all()
    for row, qa in enumerate(qas):
        for k, q in enumerate(QS):
            y = 1.0 - q
            g = float(mp_g(qa, float(lam_q[row, k]), t_ttft[row]))
            print(f"N={qa.chain.N} q={q}: g(lam_ttft)={g:.9e}")
            assert abs(g - y) <= WVA_TOL * y + TAIL_TOL


def tail_fleet():
    """The 27-cell fleet of tests/test_plan_gpu.py (one-wave cells, 256-wide
    cells, the global-memory tier), one server without load in the second
    scenario. Its N = 1 server is TTFT-only, and at lam_min about 1e-3 of its
    requests wait, so its cells are infeasible at the highest quantile only."""
    fs = make_planner()
    arrival, _, _ = base_loads(build_system())
    scen = np.stack([arrival, arrival * np.float32(1.7)]).astype(np.float32)
    scen[1, ZERO_SRV] = 0.0
    return fs, scen


GRID_QS = (0.5, 0.95, 0.99999)


def test_grid_equals_single_slices():
    fs, scen = tail_fleet()
    fs.reconcile()  # a context with a warm memo
    memo = fs.memo_stats()
    res = fs.plan_tail(GRID_QS, arrival=scen, return_cells=True)
    assert fs.memo_stats() == memo
    feas = res.cells["feasible"]
    assert (feas[:2].astype(bool) & ~feas[2].astype(bool)).any(), "no cell turns infeasible"
    assert (res.winners.acc_idx[:, 1, ZERO_SRV] != -1).all()
    assert (res.wait_tail[:, 1, ZERO_SRV] == 0).all()
    for k, q in enumerate(GRID_QS):
        for s in range(scen.shape[0]):
            one = fs.plan_tail([q], arrival=scen[s:s + 1], return_cells=True)
            for f in ("acc_idx", "num_replicas", "batch"):
                assert np.array_equal(getattr(res.winners, f)[k, s], getattr(one.winners, f)[0, 0])
            for f in ("cost", "value", "itl", "ttft", "rho", "max_rate"):
                assert np.array_equal(bits(getattr(res.winners, f)[k, s]),
                                      bits(getattr(one.winners, f)[0, 0])), f
            assert np.array_equal(bits(res.wait_tail[k, s]), bits(one.wait_tail[0, 0]))
            ok = res.cells["feasible"][k, s].astype(bool)
            assert np.array_equal(ok, one.cells["feasible"][0, 0].astype(bool))
            for f in ("num_replicas", "cost", "ttft", "wait_tail"):
                assert np.array_equal(bits(res.cells[f][k, s][ok].astype(np.float32)),
                                      bits(one.cells[f][0, 0][ok].astype(np.float32))), f
            assert np.isnan(res.cells["wait_tail"][k, s][~ok]).all()


def test_gpu_matches_cpu_backend():
    qs, scales = (0.5, 0.95), (40.0, 90.0)  # tens of replicas per server
    gpu = FastSweep(fleet(24, seed=5), backend="gpu").plan_tail(qs, scales=scales)
    cpu = FastSweep(fleet(24, seed=5), backend="cpu").plan_tail(qs, scales=scales)
    assert np.array_equal(gpu.winners.acc_idx == -1, cpu.winners.acc_idx == -1)
    same = gpu.winners.num_replicas == cpu.winners.num_replicas
    flips = ~same
    n = same.size
    print(f"replica flips: {int(flips.sum())} of {n}")
    assert flips.sum() <= max(1, n // 50)
    assert (np.abs(gpu.winners.num_replicas - cpu.winners.num_replicas)[flips] == 1).all()
    on = same & (gpu.winners.acc_idx == cpu.winners.acc_idx) & (gpu.winners.acc_idx >= 0)
    diff = np.abs(gpu.wait_tail[on].astype(np.float64) - cpu.wait_tail[on].astype(np.float64))
    # (both are fp32 outputs: half an ulp of each on top of test 1's tolerance)
    assert (diff <= TAIL_TOL + np.spacing(cpu.wait_tail[on])).all()


def test_sanity_against_mean_sizing():
    system = fleet(24, seed=5)
    fs = FastSweep(system, backend="gpu")
    mean = fs.plan(scales=[60.0])
    # a quantile the mean sizing already implies, picked on the CPU golden: at
    # q = 0.05 its percentile plan needs no more replicas than its mean plan
    cpu = FastSweep(fleet(24, seed=5), backend="cpu")
    q_low = 0.05
    assert (cpu.plan_tail([q_low], scales=[60.0]).winners.num_replicas[0, 0]
            <= cpu.plan(scales=[60.0]).winners.num_replicas[0]).all()
    res = fs.plan_tail([q_low, 0.9, 0.99], scales=[60.0])
    on = res.winners.acc_idx >= 0
    bound = ((1.0 - res.quantiles) * (1.0 + WVA_TOL))[:, None, None]
    assert (res.wait_tail.astype(np.float64) <= bound)[on].all()
    assert (res.winners.num_replicas[0, 0] <= mean.winners.num_replicas[0]).all()
    assert (np.diff(res.winners.num_replicas[:, 0], axis=0) >= 0).all()
