"""Measure the forecast rollout against the sequential way of getting the same
answer, on the flagship 512-model fleet.

  python examples/bench_rollout.py [--steps 16,256] [--reps 5] [--inner 100]
                                   [--inner-long 30] [--jobs loop,rollout] [--out FILE]

Two jobs, both producing what the controller does over S consecutive ticks of
a diurnal forecast (a sinusoid between 0.25x and 4x of the base arrival rates,
one period over the horizon):

  loop     S FastSweep.reconcile() calls with load_override, the winner of
           each fed back as cur_override of the next (what a caller had to do
           before FastSweep.rollout existed; on a checkout without rollout()
           only this job runs)
  rollout  one FastSweep.rollout(arrival) call

with the sizing memo warm (the token averages repeat). Before timing, every
step of the rollout is checked to equal the loop's winners byte for byte. A
repetition times --inner calls of each job (--inner-long at horizons above 64
steps) and keeps the median; the jobs alternate inside a repetition, the
repetitions are interleaved. Every timed call ends in a device synchronise.
Needs a GPU; prints one JSON line.
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

FIELDS = ("acc_idx", "num_replicas", "batch", "cost", "value", "itl", "ttft", "rho", "max_rate")


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--models", type=int, default=512)
    p.add_argument("--steps", default="16,256", help="horizons to time, comma-separated")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--inner", type=int, default=100)
    p.add_argument("--inner-long", type=int, default=30)
    p.add_argument("--seed", type=int, default=1234)
    p.add_argument("--jobs", default="loop,rollout", help="which jobs to time (loop,rollout)")
    p.add_argument("--label", default="")
    p.add_argument("--out", default="")
    args = p.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("bench_rollout needs a GPU", file=sys.stderr)
        return 2
    from inferno_amd.core.system import System
    from inferno_amd.engine import FastSweep
    from inferno_amd.utils.synthetic import make_fleet_spec

    system, _ = System.from_spec(make_fleet_spec(args.models, seed=args.seed))
    for acc in system.accelerators.values():
        acc.calculate()
    fs = FastSweep(system, backend="gpu")
    names = fs.server_names
    arrival = np.array([system.servers[n].load.arrivalRate for n in names], dtype=np.float32)
    in_tok = np.array([system.servers[n].load.avgInTokens for n in names], dtype=np.int32)
    out_tok = np.array([system.servers[n].load.avgOutTokens for n in names], dtype=np.int32)
    cur_acc = np.full(len(names), -3, dtype=np.int32)
    cur_rep = np.zeros(len(names), dtype=np.int32)
    cur_cost = np.zeros(len(names), dtype=np.float32)
    for j, n in enumerate(names):
        cur = system.servers[n].cur_allocation
        if cur is not None:
            cur_acc[j] = fs._acc_index.get(cur.accelerator, -1)
            cur_rep[j] = cur.num_replicas
            cur_cost[j] = cur.cost
    start = (cur_acc, cur_rep, cur_cost)
    has_rollout = hasattr(fs, "rollout")

    def forecast(n_steps: int) -> np.ndarray:
        # log-sinusoid: 1x -> 4x -> 1x -> 0.25x -> 1x over the horizon
        phase = 2.0 * np.pi * np.arange(n_steps) / n_steps
        scales = np.exp(np.log(4.0) * np.sin(phase))
        return np.stack([arrival * np.float32(s) for s in scales]).astype(np.float32)

    def job_loop(scen):
        cur = start
        out = []
        for s in range(scen.shape[0]):
            fs.load_override = (scen[s], in_tok, out_tok)
            fs.cur_override = cur
            w = fs.reconcile()
            out.append(w)
            ok = w.acc_idx != -1
            cur = (
                np.where(ok, np.where(w.acc_idx == -2, -1, w.acc_idx), cur[0]).astype(np.int32),
                np.where(ok, w.num_replicas, cur[1]).astype(np.int32),
                np.where(ok, w.cost, cur[2]).astype(np.float32),
            )
        return out

    def job_rollout(scen):
        fs.load_override = (arrival, in_tok, out_tok)
        fs.cur_override = start
        return fs.rollout(arrival=scen)

    jobs = {"loop": job_loop}
    if has_rollout:
        jobs["rollout"] = job_rollout
    jobs = {k: v for k, v in jobs.items() if k in args.jobs.split(",")}

    def timed(fn, scen, inner: int) -> float:
        ts = []
        for _ in range(inner):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(scen)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1000.0)
        return statistics.median(ts)

    horizons = {}
    for n_steps in [int(t) for t in args.steps.split(",") if t.strip()]:
        scen = forecast(n_steps)
        # same answers (checked once, memo warm): every step of the rollout is
        # the loop's reconcile of that step
        ref = job_loop(scen)
        moves = 0
        if "rollout" in jobs:
            res = job_rollout(scen)
            for s, w in enumerate(ref):
                for f in FIELDS:
                    a, b = getattr(res.winners, f)[s], getattr(w, f)
                    assert a.tobytes() == b.tobytes(), f"rollout differs from loop: step {s} {f}"
            moves = int(res.acc_changes.sum())
        inner = args.inner if n_steps <= 64 else args.inner_long
        for fn in jobs.values():  # warm every path the timed window uses
            for _ in range(2):
                fn(scen)
        series = {f"{name}_ms": [] for name in jobs}
        for _ in range(args.reps):
            for name, fn in jobs.items():
                series[f"{name}_ms"].append(round(timed(fn, scen, inner), 4))
        horizons[str(n_steps)] = {
            "steps": n_steps,
            "inner_calls_per_rep": inner,
            "accelerator_changes": moves,
            "series": series,
            "summary": {
                k: {"min": min(v), "median": statistics.median(v), "max": max(v)}
                for k, v in series.items()
            },
        }

    out = {
        "tool": "examples/bench_rollout.py",
        "label": args.label,
        "device": torch.cuda.get_device_name(0),
        "models": args.models,
        "cells": int(fs.n_cells),
        "forecast": "arrival x exp(ln 4 x sin(2 pi s / S)): 0.25x..4x, one period",
        "reps": args.reps,
        "statistic": "median of the inner calls, per repetition; memo warm",
        "memo_stats": fs.memo_stats(),
        "horizons": horizons,
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
