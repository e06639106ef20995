"""Measure token-mix what-if planning against the way of getting the same
answer without it, on the flagship 512-model fleet.

  python examples/bench_plan_tokens.py [--reps 5] [--inner 100] [--out FILE]
                                       [--jobs loop,tokens]

Both jobs produce the solution of W = 8 pairs of factors on every server's
average input and output tokens (between 0.25 and 4) times S = 2 load scales
(1, 2):

  loop    one FastSweep; per token set it puts the set's token averages into
          load_override and calls plan(arrival=...): what a caller has to write
          without FastSweep.plan_tokens. Every one of those calls finds the
          bucket layout stale and misses the sizing memo in every cell. (On a
          checkout without plan_tokens only this job runs.)
  tokens  one FastSweep.plan_tokens(token_scales, arrival=...) call

A repetition times --inner calls of each job and keeps the median; the jobs
alternate inside a repetition. Every timed call ends in a device synchronise.
Before timing, every slice of the plan_tokens result is checked byte for byte
against the loop's. Needs a GPU; prints one JSON line.
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

TOKEN_SCALES = ((1.0, 1.0), (0.25, 1.0), (4.0, 1.0), (1.0, 0.25), (1.0, 4.0), (2.0, 2.0),
                (0.5, 0.5), (2.0, 0.5))
LOAD_SCALES = (1.0, 2.0)
FIELDS = ("acc_idx", "num_replicas", "batch", "cost", "value", "itl", "ttft", "rho", "max_rate")


def scaled(base: np.ndarray, f: float) -> np.ndarray:
    """plan_tokens' rule: floor(float64(base) * f), a positive base never
    below 1."""
    v = np.floor(base.astype(np.float64) * f)
    return np.where(base > 0, np.maximum(v, 1), v).astype(np.int32)


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--models", type=int, default=512)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--inner", type=int, default=100)
    p.add_argument("--seed", type=int, default=1234)
    p.add_argument("--jobs", default="loop,tokens", help="which jobs to time (loop,tokens)")
    p.add_argument("--label", default="")
    p.add_argument("--out", default="")
    args = p.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("bench_plan_tokens needs a GPU", file=sys.stderr)
        return 2
    from inferno_amd.core.system import System
    from inferno_amd.engine import FastSweep
    from inferno_amd.utils.synthetic import make_fleet_spec

    def build_sweep():
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
        fs.load_override = (arrival, in_tok, out_tok)
        fs.cur_override = (cur_acc, cur_rep, cur_cost)
        return fs

    looper = build_sweep()
    arrival, in_tok, out_tok = looper.load_override
    scen = np.stack([arrival * np.float32(sc) for sc in LOAD_SCALES]).astype(np.float32)
    sets = [(scaled(in_tok, f_in), scaled(out_tok, f_out)) for f_in, f_out in TOKEN_SCALES]

    def loop():
        out = []
        for t_in, t_out in sets:
            looper.load_override = (arrival, t_in, t_out)
            out.append(looper.plan(arrival=scen))
        return out

    jobs = {"loop": loop}
    planner = build_sweep()
    if hasattr(planner, "plan_tokens"):

        def tokens():
            return planner.plan_tokens(token_scales=TOKEN_SCALES, arrival=scen)

        jobs["tokens"] = tokens

        # same answers, checked once: every slice of plan_tokens is the loop's
        res, ref = tokens(), loop()
        for w, r in enumerate(ref):
            assert res.in_tok[w].tobytes() == sets[w][0].tobytes()
            assert res.out_tok[w].tobytes() == sets[w][1].tobytes()
            for f in FIELDS:
                a, b = getattr(res.winners, f)[w], getattr(r.winners, f)
                assert a.tobytes() == b.tobytes(), f"plan_tokens differs from loop: set {w} {f}"
            assert res.replicas_by_acc[w].tobytes() == r.replicas_by_acc.tobytes()
            assert res.cost_total[w].tobytes() == r.cost_total.tobytes()
    jobs = {k: v for k, v in jobs.items() if k in args.jobs.split(",")}

    def timed(fn) -> float:
        ts = []
        for _ in range(args.inner):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1000.0)
        return statistics.median(ts)

    for fn in jobs.values():  # warm every path the timed window uses
        for _ in range(3):
            fn()

    series = {f"{name}_ms": [] for name in jobs}
    for _ in range(args.reps):
        for name, fn in jobs.items():
            series[f"{name}_ms"].append(round(timed(fn), 4))

    out = {
        "tool": "examples/bench_plan_tokens.py",
        "label": args.label,
        "device": torch.cuda.get_device_name(0),
        "models": args.models,
        "cells": int(planner.n_cells),
        "token_scales": [list(t) for t in TOKEN_SCALES],
        "load_scales": list(LOAD_SCALES),
        "reps": args.reps,
        "inner_calls_per_rep": args.inner,
        "statistic": "median of the inner calls, per repetition",
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
