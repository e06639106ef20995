"""Measure the hold analysis against the load plan at the same scenario count,
on the flagship 512-model fleet.

  python examples/bench_hold.py [--scenarios 16] [--reps 5] [--inner 100] [--out FILE]
                                [--jobs plan,hold] [--memo both|warm|cold]

Two jobs over S load scenarios (scales spread geometrically over 0.25x..4x):

  plan  one FastSweep.plan(arrival) call: every cell of every server sized and
        evaluated per scenario (on a checkout without hold() only this job runs)
  hold  one FastSweep.hold(arrival, allocation) call with the 1x plan's winners
        as the allocation: one held cell per server evaluated per scenario

each with the sizing memo warm (the token averages repeat) and cold (every
inner call moves the input token averages by one, so every cell's memo key
changes; contexts, buffers and buckets stay warm). A repetition times --inner
calls of each job and keeps the median; the jobs alternate inside a repetition,
the repetitions are interleaved. Every timed call returns synchronised.

Before anything is timed the tool checks the exactness claim on this fleet:
held at the winners of plan(arrival), every loaded slice with a winner has the
plan winner's itl, ttft and rho bit for bit, is HOLD_OK, and
max(needed, min_replicas) is the planned replica count. Needs a GPU; prints one
JSON line.
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
    p.add_argument("--jobs", default="plan,hold", help="which jobs to time (plan,hold)")
    p.add_argument("--memo", choices=["both", "warm", "cold"], default="both")
    p.add_argument("--label", default="")
    p.add_argument("--out", default="")
    args = p.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("bench_hold needs a GPU", file=sys.stderr)
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
    fs.load_override = (arrival, in_tok, out_tok)
    scales = np.geomspace(0.25, 4.0, args.scenarios)
    scen = np.stack([arrival * np.float32(s) for s in scales]).astype(np.float32)
    has_hold = hasattr(fs, "hold")
    in_alt = [in_tok, (in_tok + 1).astype(np.int32)]
    flip = [0]

    def tokens(cold: bool):
        if cold:
            flip[0] ^= 1
            return in_alt[flip[0]]
        return in_tok

    # the held allocation: the winners of the 1x plan
    base = fs.plan(arrival=arrival[None, :]).winners
    held = (base.acc_idx[0].copy(), base.num_replicas[0].copy())

    def job_plan(cold: bool):
        fs.load_override = (arrival, tokens(cold), out_tok)
        return fs.plan(arrival=scen)

    def job_hold(cold: bool):
        fs.load_override = (arrival, tokens(cold), out_tok)
        return fs.hold(arrival=scen, allocation=held)

    jobs = {"plan": job_plan}
    if has_hold:
        jobs["hold"] = job_hold
    jobs = {k: v for k, v in jobs.items() if k in args.jobs.split(",")}
    memo_states = {"both": (False, True), "warm": (False,), "cold": (True,)}[args.memo]

    checked = None
    if has_hold:
        from inferno_amd.engine import HOLD_OK

        pl = job_plan(False)
        w = pl.winners
        h = fs.hold(arrival=scen, allocation=(w.acc_idx, w.num_replicas))
        live = (w.acc_idx >= 0) & (scen != 0)
        for f in ("itl", "ttft", "rho"):
            a = np.ascontiguousarray(getattr(h, f)).view(np.uint32)
            b = np.ascontiguousarray(getattr(w, f)).view(np.uint32)
            assert np.array_equal(a[live], b[live]), f"hold differs from plan in the bits of {f}"
        assert (h.status[live] == HOLD_OK).all(), "a plan-held slice is not HOLD_OK"
        min_rep = np.array([s.min_num_replicas for s in fs._srv_objs])[None, :]
        assert np.array_equal(np.maximum(h.needed_replicas, min_rep)[live],
                              w.num_replicas[live]), "needed replicas differ from the plan's"
        checked = int(live.sum())

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
        "tool": "examples/bench_hold.py",
        "label": args.label,
        "device": torch.cuda.get_device_name(0),
        "models": args.models,
        "cells": int(fs.n_cells),
        "scenarios": int(args.scenarios),
        "scales": [round(float(s), 4) for s in scales],
        "reps": args.reps,
        "inner_calls_per_rep": args.inner,
        "statistic": "median of the inner calls, per repetition",
        "slices_checked_bit_equal": checked,
        "hold_status_counts": (job_hold(False).counts.sum(axis=0).tolist() if "hold" in jobs
                               else None),
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
