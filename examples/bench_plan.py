"""Measure what-if planning against the sequential way of getting the same
answer, on the flagship 512-model fleet.

  python examples/bench_plan.py [--scenarios 16] [--reps 5] [--inner 100] [--out FILE]
                                [--jobs loop,plan] [--memo both|warm|cold]

Two jobs, both producing the solution of S load scenarios (scales spread
geometrically over 0.25x..4x):

  loop  S FastSweep.reconcile() calls with load_override (what a caller had to
        do before FastSweep.plan existed; on a checkout without plan() only
        this job runs)
  plan  one FastSweep.plan(scales) call

each with the sizing memo warm (the token averages repeat) and cold (every
inner call moves the input token averages by one, so every cell's memo key
changes and every cell is sized again; contexts, buffers and buckets stay
warm). A repetition times --inner calls of each job and keeps the median; the
jobs alternate inside a repetition, the repetitions are interleaved. Every
timed call ends in a device synchronise (reconcile() and plan() return
synchronised). Needs a GPU; prints one JSON line.
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


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--models", type=int, default=512)
    p.add_argument("--scenarios", type=int, default=16)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--inner", type=int, default=100)
    p.add_argument("--seed", type=int, default=1234)
    p.add_argument("--jobs", default="loop,plan", help="which jobs to time (loop,plan)")
    p.add_argument("--memo", choices=["both", "warm", "cold"], default="both")
    p.add_argument("--label", default="")
    p.add_argument("--out", default="")
    args = p.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("bench_plan needs a GPU", file=sys.stderr)
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
    fs.cur_override = (cur_acc, cur_rep, cur_cost)
    scales = np.geomspace(0.25, 4.0, args.scenarios)
    scen = np.stack([arrival * np.float32(s) for s in scales]).astype(np.float32)
    has_plan = hasattr(fs, "plan")
    in_alt = [in_tok, (in_tok + 1).astype(np.int32)]
    flip = [0]

    def tokens(cold: bool):
        if cold:
            flip[0] ^= 1
            return in_alt[flip[0]]
        return in_tok

    def job_loop(cold: bool):
        it = tokens(cold)
        out = []
        for s in range(scen.shape[0]):
            fs.load_override = (scen[s], it, out_tok)
            out.append(fs.reconcile())
        return out

    def job_plan(cold: bool):
        fs.load_override = (arrival, tokens(cold), out_tok)
        return fs.plan(arrival=scen)

    jobs = {"loop": job_loop}
    if has_plan:
        jobs["plan"] = job_plan
    jobs = {k: v for k, v in jobs.items() if k in args.jobs.split(",")}
    memo_states = {"both": (False, True), "warm": (False,), "cold": (True,)}[args.memo]

    # same answers (checked once, memo warm): every slice of the plan is the
    # loop's reconcile of that scenario
    ref = job_loop(False)
    if "plan" in jobs:
        res = job_plan(False)
        for s, w in enumerate(ref):
            for f in ("acc_idx", "num_replicas", "batch", "cost", "value", "itl", "ttft",
                      "rho", "max_rate"):
                a, b = getattr(res.winners, f)[s], getattr(w, f)
                assert a.tobytes() == b.tobytes(), f"plan differs from loop: scenario {s} {f}"

    def timed(fn, cold: bool) -> float:
        ts = []
        for _ in range(args.inner):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(cold)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1000.0)
        return statistics.median(ts)

    for fn in jobs.values():  # warm every path the timed window uses
        for cold in memo_states:
            for _ in range(3):
                fn(cold)

    series = {f"{name}_{'cold' if cold else 'warm'}_ms": []
              for name in jobs for cold in memo_states}
    for _ in range(args.reps):
        for cold in memo_states:
            for name, fn in jobs.items():
                series[f"{name}_{'cold' if cold else 'warm'}_ms"].append(
                    round(timed(fn, cold), 4))

    out = {
        "tool": "examples/bench_plan.py",
        "label": args.label,
        "device": torch.cuda.get_device_name(0),
        "models": args.models,
        "cells": int(fs.n_cells),
        "scenarios": int(args.scenarios),
        "scales": [round(float(s), 4) for s in scales],
        "reps": args.reps,
        "inner_calls_per_rep": args.inner,
        "statistic": "median of the inner calls, per repetition",
        "memo_stats": fs.memo_stats(),
        "series": series,
        "summary": {
            k: {"min": min(v), "median": statistics.median(v), "max": max(v)}
            for k, v in series.items()
        },
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
