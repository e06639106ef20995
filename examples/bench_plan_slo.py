"""Measure SLO what-if planning against the way of getting the same answer
without it, on the flagship 512-model fleet.

  python examples/bench_plan_slo.py [--reps 5] [--inner 100] [--out FILE]
                                    [--jobs loop,slo] [--variants kept,adhoc]

Both jobs produce the solution of T = 4 SLO scales (0.5, 0.8, 1, 2 on every
TTFT and ITL target) times S = 4 load scales (0.5, 1, 2, 3):

  loop  T FastSweep objects on systems whose targets were edited, plan(scales)
        on each: what a caller has to write without FastSweep.plan_slo (on a
        checkout without plan_slo only this job runs)
  slo   one FastSweep.plan_slo(slo_scales, scales) call

in two variants:

  kept   the same question again: the loop keeps its T FastSweep objects and
         contexts, so all its sizings are memo hits (its best case); plan_slo
         can take memo hits for its base-target set only and sizes the other
         T - 1 sets on every call
  adhoc  the targets change before every call (the SLO scales alternate
         between the set above and that set times 1.001) and every cell is
         sized again: the loop edits its systems and builds T new FastSweep
         objects and native contexts, plan_slo is called with the other scales
         on its one context (with the input token averages moved by one, so
         that its base-target set misses the memo too)

A repetition times --inner calls of each job and variant and keeps the median;
jobs and variants alternate inside a repetition. Every timed call ends in a
device synchronise. Before timing, every slice of the plan_slo result is
checked byte for byte against the loop's. Needs a GPU; prints one JSON line.
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

SLO_SCALES = (0.5, 0.8, 1.0, 2.0)
LOAD_SCALES = (0.5, 1.0, 2.0, 3.0)
FIELDS = ("acc_idx", "num_replicas", "batch", "cost", "value", "itl", "ttft", "rho", "max_rate")


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--models", type=int, default=512)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--inner", type=int, default=100)
    p.add_argument("--seed", type=int, default=1234)
    p.add_argument("--jobs", default="loop,slo", help="which jobs to time (loop,slo)")
    p.add_argument("--variants", default="kept,adhoc", help="which variants (kept,adhoc)")
    p.add_argument("--label", default="")
    p.add_argument("--out", default="")
    args = p.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("bench_plan_slo needs a GPU", file=sys.stderr)
        return 2
    from inferno_amd.core.system import System
    from inferno_amd.engine import FastSweep
    from inferno_amd.utils.synthetic import make_fleet_spec

    def build_system():
        system, _ = System.from_spec(make_fleet_spec(args.models, seed=args.seed))
        for acc in system.accelerators.values():
            acc.calculate()
        return system

    def targets_of(system):
        seen = {}
        for name in sorted(system.servers):
            srv = system.servers[name]
            svc = system.service_classes.get(srv.service_class_name)
            t = svc.model_target(srv.model_name) if svc is not None else None
            if t is not None:
                seen.setdefault(id(t), t)
        return list(seen.values())

    def overrides(system, fs):
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
        return (arrival, in_tok, out_tok), (cur_acc, cur_rep, cur_cost)

    # the two SLO-scale sets the adhoc variant alternates between; kept uses [0]
    slo_sets = [np.array(SLO_SCALES, dtype=np.float32),
                (np.array(SLO_SCALES, dtype=np.float32) * np.float32(1.001)).astype(np.float32)]

    # loop: one system per target set, its base targets remembered
    loop_systems = [build_system() for _ in SLO_SCALES]
    loop_base = [[(t, np.float32(t.ttft), np.float32(t.itl)) for t in targets_of(s)]
                 for s in loop_systems]

    def edited_sweep(t: int, scale) -> "FastSweep":
        """A new FastSweep (and, at its first call, native context) on system t
        with every target scaled."""
        for tgt, ttft, itl in loop_base[t]:
            tgt.ttft, tgt.itl = float(ttft * np.float32(scale)), float(itl * np.float32(scale))
        system = loop_systems[t]
        fs = FastSweep(system, backend="gpu")
        fs.load_override, fs.cur_override = overrides(system, fs)
        return fs

    kept = [edited_sweep(t, slo_sets[0][t]) for t in range(len(SLO_SCALES))]
    flip = [0, 0]

    def loop_kept():
        return [fs.plan(scales=LOAD_SCALES) for fs in kept]

    def loop_adhoc():
        flip[0] ^= 1
        return [edited_sweep(t, slo_sets[flip[0]][t]).plan(scales=LOAD_SCALES)
                for t in range(len(SLO_SCALES))]

    jobs = {"loop": {"kept": loop_kept, "adhoc": loop_adhoc}}
    base_sys = build_system()
    planner = FastSweep(base_sys, backend="gpu")
    if hasattr(planner, "plan_slo"):
        load, cur = overrides(base_sys, planner)
        planner.load_override, planner.cur_override = load, cur
        in_alt = [load[1], (load[1] + 1).astype(np.int32)]

        def slo_kept():
            planner.load_override = load
            return planner.plan_slo(slo_scales=slo_sets[0], scales=LOAD_SCALES)

        def slo_adhoc():
            flip[1] ^= 1
            planner.load_override = (load[0], in_alt[flip[1]], load[2])
            return planner.plan_slo(slo_scales=slo_sets[flip[1]], scales=LOAD_SCALES)

        jobs["slo"] = {"kept": slo_kept, "adhoc": slo_adhoc}

        # same answers, checked once: every slice of plan_slo is the loop's
        res, ref = slo_kept(), loop_kept()
        for t, r in enumerate(ref):
            for f in FIELDS:
                a, b = getattr(res.winners, f)[t], getattr(r.winners, f)
                assert a.tobytes() == b.tobytes(), f"plan_slo differs from loop: set {t} {f}"
            assert res.replicas_by_acc[t].tobytes() == r.replicas_by_acc.tobytes()
            assert res.cost_total[t].tobytes() == r.cost_total.tobytes()
    jobs = {k: v for k, v in jobs.items() if k in args.jobs.split(",")}
    variants = [v for v in ("kept", "adhoc") if v in args.variants.split(",")]

    def timed(fn) -> float:
        ts = []
        for _ in range(args.inner):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1000.0)
        return statistics.median(ts)

    for fns in jobs.values():  # warm every path the timed window uses
        for v in variants:
            for _ in range(3):
                fns[v]()

    series = {f"{name}_{v}_ms": [] for name in jobs for v in variants}
    for _ in range(args.reps):
        for v in variants:
            for name, fns in jobs.items():
                series[f"{name}_{v}_ms"].append(round(timed(fns[v]), 4))

    out = {
        "tool": "examples/bench_plan_slo.py",
        "label": args.label,
        "device": torch.cuda.get_device_name(0),
        "models": args.models,
        "cells": int(planner.n_cells),
        "slo_scales": list(SLO_SCALES),
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
