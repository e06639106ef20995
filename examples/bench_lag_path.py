"""Measure the lag path on the flagship 512-model fleet.

  python examples/bench_lag_path.py [--reps 5] [--ticks 32] [--max-n N] [--averages]
                                    [--out profiles/bench_lag_path.json]

The forecast is --ticks ticks of --tick-seconds (a ramp 1x..3x and back), the
allocation the rollout's own winners, one tick late (delay=1). Before anything
is timed the GPU result is compared with the CPU golden on a sample of servers.
Then it records ms per FastSweep.lag_path call (median of --reps calls, each
returning synchronised), the tasks (runs), chunks and launches of the pass, the
total steps, the state updates per second, and the heaviest record of any chunk
(N x steps) run alone through the probe. With --max-n above LAG_MAX_N the wide
runs take part (the tiled path kernels): the golden sample gains the cheapest
wide server, and the wide pass' tasks, tiles, segments, launches and state
updates per second (over the time the call takes beyond a default call, timed
in the same run) are recorded. With --averages the call with averages=True
(wva_lag_path_avg_t) is checked against the golden's averages on the same
sample and timed in alternation with the default call, and the heaviest record
runs through both probes, also in alternation: the cost of the averages per
call and per step. With both, the combined call runs the wide runs through
wva_lag_path_avg_tile_t (two blocks per tile); the wide pass' native call is
timed with and without the averages, beside the bound the schedule gives:
1 + (block-steps of the average blocks) / (all block-steps). Needs a GPU;
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
    p.add_argument("--ticks", type=int, default=32)
    p.add_argument("--tick-seconds", type=float, default=60.0)
    p.add_argument("--sample", type=int, default=8)
    p.add_argument("--max-n", type=int, default=None)
    p.add_argument("--averages", action="store_true")
    p.add_argument("--out", default="")
    args = p.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("bench_lag_path needs a GPU", file=sys.stderr)
        return 2
    from inferno_amd.core.system import System
    from inferno_amd.engine import LAG_MAX_STEPS, LAG_OK, LAG_STATUS_NAMES, FastSweep
    from inferno_amd.analyzer.lag import lag_window
    from inferno_amd.ops.sweep import (LAG_MAX_N, LAG_WIDE_HALO, LAG_WIDE_STRIDE, _lag_smax,
                                       run_lag_path_probe)
    from inferno_amd.utils.synthetic import make_fleet_spec

    spec = make_fleet_spec(args.models, seed=args.seed)
    fleets = {}
    for backend in ("gpu", "cpu"):
        system, _ = System.from_spec(spec)
        for acc in system.accelerators.values():
            acc.calculate()
        fleets[backend] = FastSweep(system, backend=backend)
    fs = fleets["gpu"]
    half = args.ticks // 2
    scales = [float(s) for s in np.concatenate([np.linspace(1.0, 3.0, half),
                                                np.linspace(3.0, 1.0, args.ticks - half)])]
    roll = fs.rollout(scales=scales)
    kw = dict(scales=scales, allocation=(roll.winners.acc_idx, roll.winners.num_replicas),
              delay=1, tick_seconds=args.tick_seconds)
    base_kw = dict(kw)
    if args.max_n is not None:
        kw["max_n"] = args.max_n
    res = fs.lag_path(**kw)  # warm: context, buffers
    shape = fs.lag_path_pass
    ok = res.status == LAG_OK

    # ---- the GPU against the golden on the servers with the fewest state updates
    recs, table = shape["records"], shape["table"]
    n_of = np.zeros(len(fs.server_names), dtype=np.int64)
    n_of[table["slot"]] = table["N"]
    wide_table = shape.get("wide_table")
    if wide_table is not None:
        n_of[wide_table["slot"]] = wide_table["N"]
    work = (res.steps * ok).sum(axis=0) * n_of
    servers = [int(i) for i in np.argsort(np.where(work > 0, work, np.inf))[: args.sample]
               if work[i] > 0]
    if wide_table is not None:  # and the cheapest wide server: the golden walks every state
        w_work = np.where(n_of > LAG_MAX_N, work, 0)
        servers.append(int(np.argmin(np.where(w_work > 0, w_work, np.inf))))
    sub = np.full_like(roll.winners.acc_idx, -1)
    sub[:, servers] = roll.winners.acc_idx[:, servers]
    start = fs._hold_allocation(None, 1)
    start_acc = np.full_like(start[0][0], -1)
    start_acc[servers] = start[0][0][servers]
    gold = fleets["cpu"].lag_path(**{**kw, "allocation": (sub, roll.winners.num_replicas)},
                                  start_allocation=(start_acc, start[1][0]))
    worst = 0.0
    for f in ("ttft", "itl", "wait", "blocked", "rho", "in_system"):
        a, b = getattr(gold, f)[:, servers], getattr(res, f)[:, servers]
        assert np.array_equal(np.isnan(a), np.isnan(b)), f
        m = ~np.isnan(a)
        worst = max(worst, float((np.abs(a[m] - b[m]) / np.maximum(np.abs(a[m]), 1.0)).max()))
    assert np.array_equal(gold.steps[:, servers], res.steps[:, servers])
    assert worst <= 2e-6, worst  # two fp32 roundings of quantities that agree to 1e-12
    worst_avg = 0.0
    if args.averages:
        res_avg = fs.lag_path(averages=True, **kw)  # warm, and against the golden's averages
        gold = fleets["cpu"].lag_path(**{**kw, "allocation": (sub, roll.winners.num_replicas)},
                                      start_allocation=(start_acc, start[1][0]), averages=True)
        for f in ("ttft_avg", "itl_avg", "rho_avg", "blocked_avg"):
            a, b = getattr(gold, f)[:, servers], getattr(res_avg, f)[:, servers]
            assert np.array_equal(np.isnan(a), np.isnan(b)), f
            m = ~np.isnan(a)
            worst_avg = max(worst_avg,
                            float((np.abs(a[m] - b[m]) / np.maximum(np.abs(a[m]), 1.0)).max()))
        assert worst_avg <= 2e-6, worst_avg
        for f in ("ttft", "itl", "wait", "blocked", "rho", "in_system"):  # the end state: the bits
            assert np.array_equal(getattr(res, f).view(np.int32),
                                  getattr(res_avg, f).view(np.int32)), f

    # ---- ms per call (and of the wide pass' native call alone, inside it)
    native_ms, native_avg_ms = [], []
    if wide_table is not None:
        def timed(inner, into):
            def call(*a):
                t0 = time.perf_counter()
                r = inner(*a)
                into.append((time.perf_counter() - t0) * 1e3)
                return r
            return call

        fs._gpu.lag_path_wide = timed(fs._gpu.lag_path_wide, native_ms)
        fs._gpu.lag_path_wide_avg = timed(fs._gpu.lag_path_wide_avg, native_avg_ms)
    call_ms, avg_ms = [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        fs.lag_path(**kw)
        call_ms.append((time.perf_counter() - t0) * 1e3)
        if args.averages:  # in alternation with the default call
            t0 = time.perf_counter()
            fs.lag_path(averages=True, **kw)
            avg_ms.append((time.perf_counter() - t0) * 1e3)
    base_ms = []
    if wide_table is not None:
        fs.lag_path(**base_kw)
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fs.lag_path(**base_kw)
            base_ms.append((time.perf_counter() - t0) * 1e3)
    total_steps = int(res.steps[ok].sum())
    updates = int(((res.steps * ok).sum(axis=0) * (11 * n_of + 1)).sum())

    # ---- the heaviest record of any chunk, alone on the device through the probe
    cost = [int(table["N"][r["task"]]) * int(res.steps[r["tick0"]:r["tick0"] + r["n"],
                                                       table["slot"][r["task"]]].sum())
            for r in recs]
    r = recs[int(np.argmax(cost))]
    t = table[r["task"]]
    i, sl = int(t["slot"]), slice(int(r["tick0"]), int(r["tick0"] + r["n"]))
    one = {f: np.array([t[f]], dtype=np.float32) for f in ("alpha", "beta", "gamma", "delta")}
    one.update(in_tok=np.array([t["in_tok"]], dtype=np.int32),
               out_tok=np.array([t["out_tok"]], dtype=np.int32),
               batch_n=np.array([t["N"]], dtype=np.int32))
    k = int(np.nonzero((fs.cell_server == i) & (fs.cell_acc_idx == res.acc_idx[sl, i][0]))[0][0])
    tps = float(fs._stat["t_tps"][k])
    rate = (res.arrival[sl, i].astype(np.float64) / 60.0 if tps == 0.0
            else np.full(int(r["n"]), tps / float(t["out_tok"])))
    lam = rate / res.held_replicas[sl, i] / 1000.0
    probe = lambda **k: run_lag_path_probe(one, ["empty"], lam[None], np.ones((1, len(lam))),  # noqa: E731
                                           args.tick_seconds, max_steps=LAG_MAX_STEPS, **k)
    probe()
    if args.averages:
        probe(averages=True)
    task_ms, task_avg_ms = [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        _, probe_steps, _ = probe()
        task_ms.append((time.perf_counter() - t0) * 1e3)
        if args.averages:
            t0 = time.perf_counter()
            probe(averages=True)
            task_avg_ms.append((time.perf_counter() - t0) * 1e3)
    assert np.array_equal(probe_steps[0], res.steps[sl, i])
    out = {
        "fleet": f"{args.models} models, {len(fs.server_names)} servers", "ticks": args.ticks,
        "tick_seconds": args.tick_seconds, "delay": 1, "max_steps": LAG_MAX_STEPS,
        "ms_per_call_median": statistics.median(call_ms), "ms_per_call": call_ms,
        "status": {n_: int(res.counts[:, j].sum()) for j, n_ in enumerate(LAG_STATUS_NAMES)},
        "tasks": shape["tasks"], "chunks": shape["chunks"], "launches": shape["launches"],
        "records": len(recs), "total_steps": total_steps,
        "state_updates_per_s": updates / (statistics.median(call_ms) * 1e-3),
        "heaviest_record": {"N": int(t["N"]), "ticks": int(r["n"]),
                            "steps": int(probe_steps.sum()),
                            "ms_median_incl_launch_and_copies": statistics.median(task_ms),
                            "us_per_step": statistics.median(task_ms) * 1e3
                            / int(probe_steps.sum())},
        "gpu_vs_golden_max_rel": worst, "golden_sample_servers": len(servers),
    }
    if args.averages:
        n_steps = int(probe_steps.sum())
        lo, hi = lag_window((lam + _lag_smax({**one, "N": one["batch_n"]}, 0))
                            * args.tick_seconds * 1000.0)
        out["averages"] = {
            "ms_per_call_median": statistics.median(avg_ms), "ms_per_call": avg_ms,
            "over_default": statistics.median(avg_ms) / statistics.median(call_ms),
            "gpu_vs_golden_max_rel": worst_avg,
            "heaviest_record": {
                "ms_median_incl_launch_and_copies": statistics.median(task_avg_ms),
                "us_per_step": statistics.median(task_avg_ms) * 1e3 / n_steps,
                "over_default": statistics.median(task_avg_ms) / statistics.median(task_ms),
                # the steps that also update avg inside the window (the LDS
                # read-modify-write of the widest class), of all steps
                "window_share_of_steps": float((hi - lo).sum()) / n_steps}}
    if wide_table is not None:
        wide_ms = statistics.median(call_ms) - statistics.median(base_ms)
        out["max_n"] = args.max_n
        chain = int((res.steps * ok)[:, n_of > LAG_MAX_N].sum(axis=0).max())
        out["wide"] = {"tasks": shape["wide_tasks"], "tiles": shape["wide_tiles"],
                       "segments": shape["wide_segments"], "launches": shape["wide_launches"],
                       "step_launches": shape["wide_step_launches"],
                       "longest_server_steps": chain,
                       "native_pass_ms_median": statistics.median(native_ms),
                       "us_per_step_of_longest_server": statistics.median(native_ms) * 1e3 / chain,
                       "halo": LAG_WIDE_HALO, "stride": LAG_WIDE_STRIDE,
                       "state_updates": shape["wide_updates"],
                       "default_call_ms_median": statistics.median(base_ms),
                       "wide_part_ms": wide_ms,
                       "state_updates_per_s": shape["wide_updates"] / (wide_ms * 1e-3)}
        if args.averages:
            # the second block of a tile runs on the segments that touch the
            # window (its plain steps again, then the window's); block-steps of
            # the schedule, a segment's steps times its task's tiles
            segs, rows = shape["wide_segs"], shape["wide_rows"]
            tiles_of = np.repeat(rows["n_tiles"].astype(np.int64), rows["n_seg"])
            touches = segs["first"] + segs["count"] > segs["jlo"]
            all_steps = int((segs["count"] * tiles_of).sum())
            avg_steps = int((segs["count"] * tiles_of * touches).sum())
            out["wide"]["averages"] = {
                "native_pass_ms_median": statistics.median(native_avg_ms),
                "over_native_pass": statistics.median(native_avg_ms) / statistics.median(native_ms),
                "block_steps": all_steps, "average_block_steps": avg_steps,
                "bound_from_schedule": 1.0 + avg_steps / all_steps}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
