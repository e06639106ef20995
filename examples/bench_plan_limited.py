"""Measure capacity-limited what-if planning on the flagship 512-model fleet:
the per-scenario greedy on the device against the host loop over the
downloaded cells.

  python examples/bench_plan_limited.py [--scenarios 16] [--reps 5] [--inner 100]
                                        [--jobs loop,host,device] [--out FILE]

Every job produces the limited-mode solution of S load scenarios (scales
spread geometrically over 0.25x..4x) against one inventory: the units per
accelerator type that the unlimited plan wants at 1x, so the fleet starts
falling out mid-range. Policies: None and PriorityRoundRobin. Sizing memo warm.

  loop    what a caller had to do before plan(capacity=...) existed, written
          here with nothing newer than plan(return_cells=True): download the
          cells, prepare the candidates in numpy and call the native host
          greedy once per scenario (runs on older checkouts too)
  host    FastSweep.plan(capacity=...) with INFERNO_PLAN_GREEDY=host
  device  FastSweep.plan(capacity=...) with INFERNO_PLAN_GREEDY=device
          (wva_plan_greedy, one wave per scenario)

Before anything is timed the jobs' winning cells and granted replicas are
checked for equality, and host and device for byte equality of every result
array. A repetition times --inner calls of each job and keeps the median; the
jobs alternate inside a repetition, the repetitions are interleaved. Every
timed call ends in a device synchronise. Needs a GPU; prints one JSON line.
"""
from __future__ import annotations

import argparse
import inspect
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

POLICIES = {"None": 0, "PriorityRoundRobin": 2}


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--models", type=int, default=512)
    p.add_argument("--scenarios", type=int, default=16)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--inner", type=int, default=100)
    p.add_argument("--seed", type=int, default=1234)
    p.add_argument("--jobs", default="loop,host,device")
    p.add_argument("--label", default="")
    p.add_argument("--out", default="")
    args = p.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("bench_plan_limited needs a GPU", file=sys.stderr)
        return 2
    from inferno_amd.core.system import System
    from inferno_amd.engine import FastSweep
    from inferno_amd.ops.sweep import run_greedy_native
    from inferno_amd.utils.synthetic import make_fleet_spec

    system, _ = System.from_spec(make_fleet_spec(args.models, seed=args.seed))
    for acc in system.accelerators.values():
        acc.calculate()
    fs = FastSweep(system, backend="gpu")
    names = fs.server_names
    n_srv = len(names)
    arrival = np.array([system.servers[n].load.arrivalRate for n in names], dtype=np.float32)
    scales = np.geomspace(0.25, 4.0, args.scenarios)
    scen = np.stack([arrival * np.float32(s) for s in scales]).astype(np.float32)

    # static greedy inputs, as ShardedSolver._greedy_static builds them
    type_names = sorted({a.type for a in system.accelerators.values()} | set(system.capacity))
    acc_tidx = np.array([type_names.index(system.accelerators[a].type) for a in fs.acc_names],
                        dtype=np.int32)
    units = np.empty(fs.n_cells, dtype=np.int32)
    for k in range(fs.n_cells):
        acc_name = fs.acc_names[fs.cell_acc_idx[k]]
        model = system.models[fs._srv_objs[fs.cell_server[k]].model_name]
        units[k] = model.get_num_instances(acc_name) * system.accelerators[acc_name].multiplicity
    cell_tidx = acc_tidx[fs.cell_acc_idx]
    prio = np.array([s.priority(system) for s in fs._srv_objs], dtype=np.int32)

    # inventory: what the unlimited plan wants at 1x
    one = fs.plan(arrival=arrival[None, :], return_cells=True)
    cap0 = np.zeros(len(type_names), dtype=np.int64)
    w = one.cells["feasible"][0].astype(bool)
    for i in range(n_srv):
        a = int(one.winners.acc_idx[0, i])
        if a < 0:
            continue
        seg = np.arange(fs.seg_start[i], fs.seg_start[i + 1])
        cell = seg[(fs.cell_acc_idx[seg] == a) & w[seg]][0]
        cap0[cell_tidx[cell]] += int(one.winners.num_replicas[0, i]) * int(units[cell])
    capacity = {t: int(cap0[j]) for j, t in enumerate(type_names)}

    def job_loop(policy: str):
        cells = fs.plan(arrival=scen, return_cells=True).cells
        srv_of = fs.cell_server
        win_cell = np.full((scen.shape[0], n_srv), -1, dtype=np.int32)
        win_reps = np.zeros((scen.shape[0], n_srv), dtype=np.int32)
        for s in range(scen.shape[0]):
            idx = np.nonzero(cells["feasible"][s].astype(bool))[0]
            value = cells["value"][s]
            order = idx[np.lexsort((value[idx].astype(np.float64), srv_of[idx]))]
            seg = np.zeros(n_srv + 1, dtype=np.int32)
            np.cumsum(np.bincount(srv_of[order], minlength=n_srv), out=seg[1:])
            c_type = np.where(cells["zero_empty"][s][order].astype(bool), -1,
                              cell_tidx[order]).astype(np.int32)
            cand, reps = run_greedy_native(
                np.ascontiguousarray(value[order], dtype=np.float32), c_type,
                np.ascontiguousarray(units[order], dtype=np.int32),
                np.ascontiguousarray(cells["num_replicas"][s][order], dtype=np.int32),
                seg, prio, cap0.astype(np.int32), False, POLICIES[policy], allow_build=False)
            got = cand >= 0
            win_cell[s, got] = order[cand[got]]
            win_reps[s] = reps
        return win_cell, win_reps

    def job_plan(mode: str):
        def run(policy: str):
            os.environ["INFERNO_PLAN_GREEDY"] = mode
            res = fs.plan(arrival=scen, capacity=capacity, saturation_policy=policy)
            return res
        return run

    jobs = {"loop": job_loop}
    if "capacity" in inspect.signature(fs.plan).parameters:
        jobs["host"] = job_plan("host")
        jobs["device"] = job_plan("device")
    jobs = {k: v for k, v in jobs.items() if k in args.jobs.split(",")}

    # same answers, checked before anything is timed
    fallout = {}
    for policy in POLICIES:
        cell, reps = job_loop(policy)
        results = {}
        for name in ("host", "device"):
            if name in jobs:
                res = jobs[name](policy)
                assert np.array_equal(fs._plan_limited_cells, cell), (name, policy, "cells")
                assert np.array_equal(res.winners.num_replicas, reps), (name, policy, "replicas")
                results[name] = res
                fallout[policy] = [int(v) for v in res.unallocated_servers]
        if len(results) == 2:
            a, b = results["host"], results["device"]
            for f in ("acc_idx", "num_replicas", "batch", "cost", "value", "itl", "ttft", "rho",
                      "max_rate"):
                assert getattr(a.winners, f).tobytes() == getattr(b.winners, f).tobytes(), f
            for f in ("replicas_by_acc", "cost_total", "desired_replicas", "capacity_left",
                      "unallocated_servers", "partial_servers"):
                assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f

    def timed(fn, policy: str) -> float:
        ts = []
        for _ in range(args.inner):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(policy)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1000.0)
        return statistics.median(ts)

    for fn in jobs.values():
        for policy in POLICIES:
            for _ in range(3):
                fn(policy)

    series = {f"{name}_{policy}_ms": [] for name in jobs for policy in POLICIES}
    for _ in range(args.reps):
        for policy in POLICIES:
            for name, fn in jobs.items():
                series[f"{name}_{policy}_ms"].append(round(timed(fn, policy), 4))

    out = {
        "tool": "examples/bench_plan_limited.py",
        "label": args.label,
        "device": torch.cuda.get_device_name(0),
        "models": args.models,
        "servers": n_srv,
        "cells": int(fs.n_cells),
        "scenarios": int(args.scenarios),
        "scales": [round(float(s), 4) for s in scales],
        "capacity": capacity,
        "unallocated_servers": fallout,
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
