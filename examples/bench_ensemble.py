"""Measure the forecast ensemble against the loop of rollouts that gives the
same bands, on the flagship 512-model fleet.

  python examples/bench_ensemble.py [--shapes 16x16,64x16] [--reps 5] [--inner 100]
                                    [--inner-long 30] [--jobs loop,bands,paths] [--out FILE]

E load paths of S ticks: the diurnal forecast of examples/bench_rollout.py (a
sinusoid between 0.25x and 4x of the base arrival rates, one period over the
horizon) times lognormal noise, sigma 0.2 per path and tick
(inferno_amd.engine.noisy_paths; path 0 is the forecast itself). Three jobs:

  loop   E FastSweep.rollout(arrival=path) calls and the bands in numpy over
         their records (np.sort at the ranks of the server replicas and costs,
         of the replica totals, the cumsum cost, the infeasible and the change
         counts): what a caller had to do before rollout_ensemble() existed. The
         mode pair is not computed, so the loop does a little less
  bands  one FastSweep.rollout_ensemble(arrival) call
  paths  the same with return_paths=True

with the sizing memo warm. Before timing, every band of the ensemble is checked
to equal numpy's over the loop's rollouts, and every path of the paths job its
rollout, byte for byte. A repetition times --inner calls of each job
(--inner-long for shapes of more than 256 rows) and keeps the median; the jobs
alternate inside a repetition, the repetitions are interleaved. Every timed
call ends in a device synchronise. Needs a GPU; prints one JSON line.
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
QUANTILES = (0.5, 0.9, 1.0)


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--models", type=int, default=512)
    p.add_argument("--shapes", default="16x16,64x16", help="ExS shapes to time, comma-separated")
    p.add_argument("--sigma", type=float, default=0.2)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--inner", type=int, default=100)
    p.add_argument("--inner-long", type=int, default=30)
    p.add_argument("--seed", type=int, default=1234)
    p.add_argument("--jobs", default="loop,bands,paths")
    p.add_argument("--label", default="")
    p.add_argument("--out", default="")
    args = p.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("bench_ensemble needs a GPU", file=sys.stderr)
        return 2
    from inferno_amd.core.system import System
    from inferno_amd.engine import FastSweep, ensemble_ranks, noisy_paths
    from inferno_amd.utils.synthetic import make_fleet_spec

    system, _ = System.from_spec(make_fleet_spec(args.models, seed=args.seed))
    for acc in system.accelerators.values():
        acc.calculate()
    fs = FastSweep(system, backend="gpu")
    names = fs.server_names
    arrival = np.array([system.servers[n].load.arrivalRate for n in names], dtype=np.float32)
    in_tok = np.array([system.servers[n].load.avgInTokens for n in names], dtype=np.int32)
    out_tok = np.array([system.servers[n].load.avgOutTokens for n in names], dtype=np.int32)
    fs.load_override = (arrival, in_tok, out_tok)
    fs.cur_override = tuple(np.array(a) for a in fs._base_cur())

    def paths_of(n_paths: int, n_steps: int) -> np.ndarray:
        phase = 2.0 * np.pi * np.arange(n_steps) / n_steps
        forecast = np.exp(np.log(4.0) * np.sin(phase))
        scales = noisy_paths(forecast, args.sigma, n_paths, args.seed).astype(np.float32)
        return np.ascontiguousarray(arrival[None, None, :] * scales[:, :, None], dtype=np.float32)

    def job_loop(scen):
        ranks = ensemble_ranks(QUANTILES, scen.shape[0])
        rolled = [fs.rollout(arrival=scen[e]) for e in range(scen.shape[0])]

        def band(get):
            return np.sort(np.stack([get(r) for r in rolled]), axis=0)[ranks]

        return rolled, {
            "server_replicas_q": band(lambda r: r.winners.num_replicas),
            "server_cost_q": band(lambda r: r.winners.cost),
            "replicas_by_acc_q": band(lambda r: r.replicas_by_acc),
            "cost_total_q": band(
                lambda r: np.cumsum(r.winners.cost.astype(np.float64), axis=1)[:, -1]),
            "infeasible_q": band(lambda r: r.infeasible_servers),
            "acc_changes_q": band(lambda r: r.acc_changes),
        }

    def job_bands(scen):
        return fs.rollout_ensemble(arrival=scen, quantiles=QUANTILES)

    def job_paths(scen):
        return fs.rollout_ensemble(arrival=scen, quantiles=QUANTILES, return_paths=True)

    jobs = {"loop": job_loop, "bands": job_bands, "paths": job_paths}
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

    shapes = {}
    for shape in [t for t in args.shapes.split(",") if t.strip()]:
        n_paths, n_steps = (int(t) for t in shape.lower().split("x"))
        scen = paths_of(n_paths, n_steps)
        # same answers (checked once, memo warm)
        rolled, want = job_loop(scen)
        res = job_paths(scen)
        only = job_bands(scen)
        for k, v in want.items():
            for got in (getattr(res, k), getattr(only, k)):
                assert got.dtype == v.dtype and got.tobytes() == v.tobytes(), (
                    f"band {k} differs from numpy over the loop's rollouts")
        for e, r in enumerate(rolled):
            for f in FIELDS:
                a, b = getattr(res.paths.winners, f)[e], getattr(r.winners, f)
                assert a.tobytes() == b.tobytes(), f"path {e} differs from its rollout: {f}"
        unanimous = int((only.acc_mode_paths == n_paths).sum())
        inner = args.inner if n_paths * n_steps <= 256 else args.inner_long
        for fn in jobs.values():  # warm every path the timed window uses
            for _ in range(2):
                fn(scen)
        series = {f"{name}_ms": [] for name in jobs}
        for _ in range(args.reps):
            for name, fn in jobs.items():
                series[f"{name}_ms"].append(round(timed(fn, scen, inner), 4))
        summary = {
            k: {"min": min(v), "median": statistics.median(v), "max": max(v)}
            for k, v in series.items()
        }
        entry = {
            "paths": n_paths,
            "steps": n_steps,
            "passes": -(-n_paths // max(1, 256 // n_steps)),
            "inner_calls_per_rep": inner,
            "unanimous_tick_servers": unanimous,
            "tick_servers": n_steps * len(names),
            "series": series,
            "summary": summary,
        }
        if "loop_ms" in summary and "bands_ms" in summary:
            lo, b = summary["loop_ms"], summary["bands_ms"]
            entry["loop_over_bands"] = round(lo["median"] / b["median"], 3)
            # the project's rule: below the loop's fastest repetition by more
            # than three times the loop's own spread
            entry["rule_margin_ms"] = round(lo["min"] - 3.0 * (lo["max"] - lo["min"]), 4)
            entry["rule_met"] = bool(b["median"] < lo["min"] - 3.0 * (lo["max"] - lo["min"]))
        shapes[shape] = entry

    out = {
        "tool": "examples/bench_ensemble.py",
        "label": args.label,
        "device": torch.cuda.get_device_name(0),
        "models": args.models,
        "cells": int(fs.n_cells),
        "paths_model": f"diurnal forecast (0.25x..4x, one period) x exp({args.sigma} z), "
                       "path 0 unperturbed",
        "quantiles": list(QUANTILES),
        "reps": args.reps,
        "statistic": "median of the inner calls, per repetition; memo warm",
        "memo_stats": fs.memo_stats(),
        "shapes": shapes,
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
