"""Measure the lag analysis on the flagship 512-model fleet.

  python examples/bench_lag.py [--reps 5] [--max-n N] [--out profiles/bench_lag.json]

The allocation is the 1x plan's winners; S = 4 load scales spread over 1x..4x;
times = (15, 30, 60) s. Before anything is timed the GPU result is compared with
the CPU golden on a sample of slices. Then it records ms per FastSweep.lag call
(median of --reps calls, each returning synchronised), the host share of a call
(the same call with the device pass replaced by nothing is not available, so
the table building is timed on its own), the status histogram, the total
steps, the state updates per second, and the time of the slowest single task
(run alone through the probe). With --max-n above LAG_MAX_N the cells up to
that N go through the tiled kernels: the sample then also holds the cheapest
wide slices, and the wide tasks, tiles and launches are counted. Needs a GPU;
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


def main() -> int:
    p = argparse.ArgumentParser()
    p.add_argument("--models", type=int, default=512)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--seed", type=int, default=1234)
    p.add_argument("--sample", type=int, default=12)
    p.add_argument("--max-steps", type=int, default=None)
    p.add_argument("--max-n", type=int, default=None)
    p.add_argument("--out", default="")
    args = p.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("bench_lag needs a GPU", file=sys.stderr)
        return 2
    from inferno_amd.core.system import System
    from inferno_amd.engine import LAG_MAX_STEPS, LAG_OK, LAG_STATUS_NAMES, FastSweep
    from inferno_amd.ops.sweep import (LAG_MAX_N, LAG_WIDE_HALO, LAG_WIDE_STRIDE, run_lag_probe,
                                       run_lag_wide_probe)
    from inferno_amd.utils.synthetic import make_fleet_spec

    max_steps = LAG_MAX_STEPS if args.max_steps is None else args.max_steps
    spec = make_fleet_spec(args.models, seed=args.seed)
    fleets = {}
    for backend in ("gpu", "cpu"):
        system, _ = System.from_spec(spec)
        for acc in system.accelerators.values():
            acc.calculate()
        fleets[backend] = FastSweep(system, backend=backend)
    fs = fleets["gpu"]
    plan = fs.plan(scales=[1.0])
    alloc = (plan.winners.acc_idx[0], plan.winners.num_replicas[0])
    scales = [float(s) for s in np.geomspace(1.0, 4.0, 4)]
    times = (15.0, 30.0, 60.0)
    kw = dict(scales=scales, allocation=alloc, times=times, max_steps=max_steps)
    if args.max_n is not None:
        kw["max_n"] = args.max_n

    res = fs.lag(**kw)  # warm: context, buffers
    ok = np.argwhere(res.status == LAG_OK)
    # ---- the GPU against the golden on a sample of slices (cheapest first)
    order = ok[np.argsort(res.steps[ok[:, 0], ok[:, 1]])][:: max(len(ok) // args.sample, 1)]
    n_of = {}
    for s, i in ok:
        k = int(np.nonzero((fs.cell_server == i) & (fs.cell_acc_idx == res.acc_idx[s, i]))[0][0])
        n_of[(s, i)] = (k, int(fs._stat["override"][k]) if fs._stat["override"][k] > 0 else max(
            int(fs._stat["perf_max_batch_cfg"][k]) * int(fs._stat["at_tokens"][k])
            // int(fs._base_load()[2][i]), 1))
    servers = {int(i) for _, i in order[: args.sample]}
    # the wide slices with the fewest state updates: the golden walks every state
    wide = sorted((t for t in n_of if n_of[t][1] > LAG_MAX_N),
                  key=lambda t: int(res.steps[t]) * n_of[t][1])
    servers = sorted(servers | {int(i) for _, i in wide[:2]})
    sub_acc = np.full_like(alloc[0], -1)
    sub_acc[servers] = alloc[0][servers]
    gold = fleets["cpu"].lag(scales=scales, allocation=(sub_acc, alloc[1]), times=times,
                             **{k: kw[k] for k in ("max_steps", "max_n") if k in kw})
    worst = 0.0
    for f in ("ttft", "itl", "wait", "blocked", "rho", "in_system"):
        a, b = getattr(gold, f)[:, :, servers], getattr(res, f)[:, :, servers]
        assert np.array_equal(np.isnan(a), np.isnan(b)), f
        m = ~np.isnan(a)
        worst = max(worst, float((np.abs(a[m] - b[m]) / np.maximum(np.abs(a[m]), 1.0)).max()))
    assert np.array_equal(gold.steps[:, servers], res.steps[:, servers])
    assert worst <= 2e-6, worst  # two fp32 roundings of quantities that agree to 1e-12

    # ---- ms per call
    call_ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        fs.lag(**kw)
        call_ms.append((time.perf_counter() - t0) * 1e3)
    total_steps = int(res.steps[res.status == LAG_OK].sum())
    # state updates: every step moves the K + 1 states of its task
    updates = sum(int(res.steps[s, i]) * (11 * n + 1) for (s, i), (_, n) in n_of.items())

    # ---- the slowest single task, alone on the device through the probe
    (s_max, i_max) = max(n_of, key=lambda t: int(res.steps[t]) * n_of[t][1])
    k, n = n_of[(s_max, i_max)]
    base, in_tok, out_tok = fs._base_load()
    st = fs._stat
    tps = float(st["t_tps"][k])
    held = float(alloc[1][i_max])

    def rate(arr):
        return (float(arr) / 60.0 if tps == 0.0 else tps / float(out_tok[i_max])) / held / 1000.0

    one = {f: np.array([st[f][k]], dtype=np.float32) for f in ("alpha", "beta", "gamma", "delta")}
    one.update(in_tok=np.array([in_tok[i_max]], dtype=np.int32),
               out_tok=np.array([out_tok[i_max]], dtype=np.int32),
               batch_n=np.array([n], dtype=np.int32))
    lam = (np.array([rate(base[i_max])]), np.array([rate(res.arrival[s_max, i_max])]))
    probe = run_lag_wide_probe if n > LAG_MAX_N else run_lag_probe
    probe(one, lam[0], lam[1], times, max_steps=max_steps)
    task_ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        _, probe_steps = probe(one, lam[0], lam[1], times, max_steps=max_steps)
        task_ms.append((time.perf_counter() - t0) * 1e3)
    out = {
        "fleet": f"{args.models} models, {len(fs.server_names)} servers", "scales": scales,
        "times_s": list(times), "max_steps": max_steps,
        "ms_per_call_median": statistics.median(call_ms), "ms_per_call": call_ms,
        "status": {n_: int(res.counts[:, j].sum()) for j, n_ in enumerate(LAG_STATUS_NAMES)},
        "tasks": int(len(ok)), "total_steps": total_steps,
        "state_updates_per_s": updates / (statistics.median(call_ms) * 1e-3),
        "slowest_task": {"N": n, "steps": int(probe_steps[0]),
                         "ms_median_incl_launch_and_copies": statistics.median(task_ms),
                         "us_per_step": statistics.median(task_ms) * 1e3 / int(probe_steps[0])},
        "gpu_vs_golden_max_rel": worst, "golden_sample_servers": len(servers),
    }
    if wide:
        slots = [-(-(11 * n_of[t][1] + 1) // 24) * 24 for t in wide]
        tiles = [-(-g // LAG_WIDE_STRIDE) for g in slots]
        # a task's segments never cross a checkpoint: up to len(times) - 1 more
        seg_launches = max(-(-int(res.steps[t]) // LAG_WIDE_HALO) for t in wide)
        w_updates = sum(int(res.steps[t]) * (11 * n_of[t][1] + 1) for t in wide)
        out["wide"] = {"tasks": len(wide), "tiles": int(sum(tiles)), "halo": LAG_WIDE_HALO,
                       "stride": LAG_WIDE_STRIDE, "step_launches_at_least": int(seg_launches),
                       "state_updates": w_updates}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
