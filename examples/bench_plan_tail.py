"""Measure percentile TTFT planning on the flagship 512-model fleet.

  python examples/bench_plan_tail.py [--reps 5] [--inner 100] [--out FILE]

  tail  one FastSweep.plan_tail(quantiles, scales) call, Q = 4 quantiles
        (0.5, 0.9, 0.95, 0.99) times S = 4 load scales (0.5, 1, 2, 3)
  slo   one FastSweep.plan_slo(slo_scales, scales) call at T = 4 x S = 4 on the
        same build: the same number of sizings, for scale. Its SLO scales are
        moved by 0.1 % so that no target set takes a sizing-memo hit, as no
        quantile does.

There is no earlier way to get plan_tail's answer, so nothing is gated. A
repetition times --inner calls of each job and keeps the median; the jobs
alternate inside a repetition; every timed call ends in a device synchronise.
Also reports x = s(N) * (TTFT target - prefill at full batch), the Poisson mean
that sets the tail evaluator's window, over the fleet's cells. Needs a GPU;
prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

QUANTILES = (0.5, 0.9, 0.95, 0.99)
SLO_SCALES = (0.5005, 0.8008, 1.001, 2.002)
LOAD_SCALES = (0.5, 1.0, 2.0, 3.0)


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--models", type=int, default=512)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--inner", type=int, default=100)
    p.add_argument("--seed", type=int, default=1234)
    p.add_argument("--out", default="")
    args = p.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("bench_plan_tail needs a GPU", file=sys.stderr)
        return 2
    from inferno_amd.core.system import System
    from inferno_amd.engine import FastSweep
    from inferno_amd.utils.synthetic import make_fleet_spec

    system, _ = System.from_spec(make_fleet_spec(args.models, seed=args.seed))
    for acc in system.accelerators.values():
        acc.calculate()
    fs = FastSweep(system, backend="gpu")
    jobs = {
        "tail": lambda: fs.plan_tail(QUANTILES, scales=LOAD_SCALES),
        "slo": lambda: fs.plan_slo(slo_scales=SLO_SCALES, scales=LOAD_SCALES),
    }
    res = jobs["tail"]()  # warm both, and the figures of the result
    jobs["slo"]()
    torch.cuda.synchronize()

    # the window's Poisson mean per cell, from the staged per-cell arrays
    cells = fs.reconcile_cells()
    st = fs._stat
    n = cells["batch"].astype(np.float64)
    on = n > 0
    in_tok, out_tok = fs._base_load()[1:]
    cin = in_tok[fs.cell_server].astype(np.float64)
    cout = out_tok[fs.cell_server].astype(np.float64)
    prefill = st["gamma"] + st["delta"] * cin * n
    mu = n / np.maximum(prefill + np.maximum(cout - 1, 1) * (st["alpha"] + st["beta"] * n), 1e-30)
    x = np.maximum(mu * (st["t_ttft"] - prefill), 0.0)[on]

    medians = {k: [] for k in jobs}
    for _ in range(args.reps):
        times = {k: [] for k in jobs}
        for _ in range(args.inner):
            for k, job in jobs.items():
                t0 = time.perf_counter()
                job()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3)
        for k in jobs:
            medians[k].append(statistics.median(times[k]))
    late = res.wait_tail[res.winners.acc_idx >= 0]
    out = {
        "bench": "plan_tail", "models": args.models, "cells": int(fs.n_cells),
        "grid": [len(QUANTILES), len(LOAD_SCALES)], "reps": args.reps, "inner": args.inner,
        "plan_tail_ms": [round(v, 4) for v in medians["tail"]],
        "plan_slo_ms": [round(v, 4) for v in medians["slo"]],
        "plan_tail_ms_median": round(statistics.median(medians["tail"]), 4),
        "plan_slo_ms_median": round(statistics.median(medians["slo"]), 4),
        "window_x": {"median": round(float(np.median(x)), 2), "max": round(float(x.max()), 2)},
        "replicas_by_quantile": [int(res.winners.num_replicas[k, 1].sum())
                                 for k in range(len(QUANTILES))],
        "max_late_share": float(late.max()) if late.size else 0.0,
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
