"""Offline solver CLI: solve a SystemData JSON document (the reference's
pkg/config wire format) and print the allocation solution.

  python -m inferno_amd.cli solve system.json [--backend cpu|gpu] [--json]
  python -m inferno_amd.cli analyze system.json --server NAME:NS
  python -m inferno_amd.cli plan system.json --scales 0.5,1,1.5,2 [--backend ...] [--json]
      [--limited] [--capacity TYPE=N,...] [--saturation-policy P] [--delayed-best-effort]
  python -m inferno_amd.cli plan system.json --slo-scales 0.5,1,2 [--scales ...] [--json]
  python -m inferno_amd.cli plan system.json --rollout --scales 0.5,1,2,1,0.5 [--json]
  python -m inferno_amd.cli plan system.json --hold --scales 0.5,1,2,4 [--json]
  python -m inferno_amd.cli plan system.json --ensemble-scales "0.5,1,2;0.6,1.2,2.4;0.4,0.9,1.7"
      [--quantiles 0.5,0.9,1] [--json]
  python -m inferno_amd.cli plan system.json --scales 0.5,1,2 --ensemble-noise 0.2 --paths 16
      --seed 7 [--quantiles ...] [--json]
"""
from __future__ import annotations

import argparse
import json
import sys


def _load_system(path: str):
    from .config import system_spec_from_json
    from .core.system import System

    with open(path) as f:
        doc = json.load(f)
    spec = system_spec_from_json(doc)
    system, opt = System.from_spec(spec)
    for a in system.accelerators.values():
        a.calculate()
    return system, opt


def cmd_solve(args) -> int:
    from .engine import SweepEngine
    from .parallel import ShardedSolver

    system, opt = _load_system(args.spec)
    solver = ShardedSolver(SweepEngine(backend=args.backend))
    result = solver.solve(system, opt)
    if args.json:
        out = {
            name: {
                "accelerator": d.accelerator,
                "numReplicas": d.numReplicas,
                "maxBatch": d.maxBatch,
                "cost": round(d.cost, 2),
                "itlAverage": round(d.itlAverage, 3),
                "ttftAverage": round(d.ttftAverage, 3),
            }
            for name, d in result.solution.items()
        }
        print(json.dumps({"allocations": out}, indent=2))
    else:
        total = 0.0
        print(f"{'server':<28} {'accelerator':<14} {'replicas':>8} {'cost':>10} "
              f"{'itl(ms)':>9} {'ttft(ms)':>9}")
        for name in sorted(result.solution):
            d = result.solution[name]
            total += d.cost
            print(f"{name:<28} {d.accelerator or '(none)':<14} {d.numReplicas:>8} "
                  f"{d.cost:>10.2f} {d.itlAverage:>9.2f} {d.ttftAverage:>9.2f}")
        by_type = result.allocation_by_type
        print("-" * 82)
        for t in sorted(by_type):
            a = by_type[t]
            lim = f"/{a.limit}" if a.limit else ""
            print(f"{t:<28} {'':<14} {a.count:>8}{lim} {a.cost:>10.2f}")
        print(f"{'TOTAL':<28} {'':<14} {'':>8} {total:>10.2f}")
    return 0


def _parse_scales(text: str, flag: str = "--scales") -> list[float]:
    try:
        scales = [float(t) for t in text.split(",") if t.strip()]
    except ValueError:
        raise SystemExit(f"{flag}: not a comma-separated list of numbers: {text!r}")
    if not scales:
        raise SystemExit(f"{flag}: at least one scale is required")
    return scales


def _parse_token_scales(text: str) -> list[tuple[float, float]]:
    pairs = []
    for item in text.split(","):
        if not item.strip():
            continue
        f_in, sep, f_out = item.partition(":")
        try:
            pairs.append((float(f_in), float(f_out)))
        except ValueError:
            sep = ""
        if not sep:
            raise SystemExit(f"--token-scales: expected IN:OUT[,IN:OUT...], got {item!r}")
    if not pairs:
        raise SystemExit("--token-scales: at least one IN:OUT pair is required")
    return pairs


def _parse_capacity(text: str) -> dict:
    cap = {}
    for item in text.split(","):
        if not item.strip():
            continue
        name, sep, units = item.partition("=")
        try:
            cap[name.strip()] = int(units)
        except ValueError:
            sep = ""
        if not sep or not name.strip():
            raise SystemExit(f"--capacity: expected TYPE=N[,TYPE=N...], got {item!r}")
    return cap


def cmd_plan(args) -> int:
    """What-if load plan: the unlimited-mode solution at each load scale, or
    with --limited / --capacity the capacity-limited one."""
    import numpy as np

    from .engine import FastSweep, SweepEngine

    limited = args.limited or args.capacity is not None
    if args.ensemble_scales is not None or args.ensemble_noise is not None:
        if (limited or args.slo_scales is not None or args.token_scales is not None
                or args.rollout or args.hold):
            raise SystemExit("plan: a forecast ensemble rolls out unlimited-mode reconciles "
                             "over sampled load paths; it does not combine with --rollout, "
                             "--hold, --slo-scales, --token-scales, --limited or --capacity")
        return _cmd_plan_ensemble(args)
    if args.hold:
        if (limited or args.slo_scales is not None or args.token_scales is not None
                or args.rollout):
            raise SystemExit("plan: --hold evaluates the current allocation as it is; it does "
                             "not combine with --slo-scales, --token-scales, --rollout, "
                             "--limited or --capacity")
        return _cmd_plan_hold(args)
    if args.token_scales is not None:
        if limited or args.slo_scales is not None or args.rollout:
            raise SystemExit("plan: --token-scales is an unlimited-mode plan; it does not "
                             "combine with --slo-scales, --rollout, --limited or --capacity")
        return _cmd_plan_tokens(args)
    if args.rollout:
        if limited or args.slo_scales is not None:
            raise SystemExit("plan: --rollout replays consecutive unlimited-mode reconciles; it "
                             "does not combine with --slo-scales, --limited or --capacity")
        return _cmd_plan_rollout(args)
    if args.slo_scales is not None:
        if limited:
            raise SystemExit("plan: --slo-scales is an unlimited-mode plan; it does not "
                             "combine with --limited or --capacity")
        return _cmd_plan_slo(args)
    if args.scales is None:
        raise SystemExit("plan: one of --scales, --slo-scales and --token-scales is required")
    scales = _parse_scales(args.scales)
    system, opt = _load_system(args.spec)
    backend = SweepEngine(backend=args.backend).backend  # resolves "auto"
    fs = FastSweep(system, backend=backend)
    kw = {}
    if limited:
        kw["capacity"] = (_parse_capacity(args.capacity) if args.capacity is not None
                          else dict(system.capacity))
        kw["saturation_policy"] = (args.saturation_policy if args.saturation_policy is not None
                                   else opt.saturationPolicy)
        kw["delayed_best_effort"] = args.delayed_best_effort or bool(opt.delayedBestEffort)
    try:
        res = fs.plan(scales=scales, **kw)
    except ValueError as e:
        print(f"plan: {e}", file=sys.stderr)
        return 2
    # servers whose accelerator differs from the scale-1.0 scenario (the
    # first scale when 1.0 is not among them)
    ref = scales.index(1.0) if 1.0 in scales else 0
    acc = res.winners.acc_idx
    rows = []
    for s, scale in enumerate(scales):
        rows.append({
            "scale": scale,
            "totalCost": round(float(res.cost_total[s]), 2),
            "replicas": {
                name: int(res.replicas_by_acc[s, j]) for j, name in enumerate(fs.acc_names)
            },
            "infeasibleServers": int(res.infeasible_servers[s]),
            "acceleratorChanges": int(np.count_nonzero(acc[s] != acc[ref])),
        })
        if limited:
            rows[-1]["unallocatedServers"] = int(res.unallocated_servers[s])
            rows[-1]["partialServers"] = int(res.partial_servers[s])
            rows[-1]["capacityLeft"] = {
                t: int(res.capacity_left[s, j]) for j, t in enumerate(res.capacity_types)
            }
    if args.json:
        doc = {"backend": backend, "referenceScale": scales[ref],
               "servers": len(fs.server_names), "scenarios": rows}
        if limited:
            doc["saturationPolicy"] = kw["saturation_policy"]
            doc["delayedBestEffort"] = kw["delayed_best_effort"]
        print(json.dumps(doc, indent=2))
        return 0
    names = fs.acc_names
    types = res.capacity_types if limited else []
    print(f"{'scale':>8} {'cost':>12} " + " ".join(f"{n:>10}" for n in names)
          + f" {'infeasible':>10} {'acc-changes':>11}"
          + (f" {'unallocated':>11} {'partial':>7} "
             + " ".join(f"{'left:' + t:>10}" for t in types) if limited else ""))
    for r in rows:
        print(f"{r['scale']:>8g} {r['totalCost']:>12.2f} "
              + " ".join(f"{r['replicas'][n]:>10}" for n in names)
              + f" {r['infeasibleServers']:>10} {r['acceleratorChanges']:>11}"
              + (f" {r['unallocatedServers']:>11} {r['partialServers']:>7} "
                 + " ".join(f"{r['capacityLeft'][t]:>10}" for t in types) if limited else ""))
    print(f"({len(fs.server_names)} servers, backend {backend}; acc-changes are "
          f"relative to scale {scales[ref]:g})")
    if limited:
        print(f"(limited mode: saturation policy {kw['saturation_policy']}, "
              f"delayed best-effort {'on' if kw['delayed_best_effort'] else 'off'})")
    return 0


def _cmd_plan_slo(args) -> int:
    """What-if SLO plan: the unlimited-mode solution at each SLO scale (the
    factor on every TTFT and ITL target) and each load scale."""
    import numpy as np

    from .engine import FastSweep, SweepEngine

    slo_scales = _parse_scales(args.slo_scales, "--slo-scales")
    scales = _parse_scales(args.scales) if args.scales is not None else [1.0]
    system, _ = _load_system(args.spec)
    backend = SweepEngine(backend=args.backend).backend  # resolves "auto"
    fs = FastSweep(system, backend=backend)
    try:
        res = fs.plan_slo(slo_scales=slo_scales, scales=scales)
    except ValueError as e:
        print(f"plan: {e}", file=sys.stderr)
        return 2
    # accelerator changes are relative to SLO scale 1.0 at load scale 1.0 (the
    # first of either when 1.0 is not among them)
    tref = slo_scales.index(1.0) if 1.0 in slo_scales else 0
    sref = scales.index(1.0) if 1.0 in scales else 0
    acc = res.winners.acc_idx
    blocks = []
    for t, slo_scale in enumerate(slo_scales):
        rows = [{
            "scale": scale,
            "totalCost": round(float(res.cost_total[t, s]), 2),
            "replicas": {
                name: int(res.replicas_by_acc[t, s, j]) for j, name in enumerate(fs.acc_names)
            },
            "infeasibleServers": int(res.infeasible_servers[t, s]),
            "acceleratorChanges": int(np.count_nonzero(acc[t, s] != acc[tref, sref])),
        } for s, scale in enumerate(scales)]
        blocks.append({"sloScale": slo_scale, "scenarios": rows})
    if args.json:
        print(json.dumps({"backend": backend, "referenceSloScale": slo_scales[tref],
                          "referenceScale": scales[sref], "servers": len(fs.server_names),
                          "sloScenarios": blocks}, indent=2))
        return 0
    names = fs.acc_names
    for b in blocks:
        print(f"SLO scale {b['sloScale']:g} (TTFT and ITL targets x {b['sloScale']:g})")
        print(f"{'scale':>8} {'cost':>12} " + " ".join(f"{n:>10}" for n in names)
              + f" {'infeasible':>10} {'acc-changes':>11}")
        for r in b["scenarios"]:
            print(f"{r['scale']:>8g} {r['totalCost']:>12.2f} "
                  + " ".join(f"{r['replicas'][n]:>10}" for n in names)
                  + f" {r['infeasibleServers']:>10} {r['acceleratorChanges']:>11}")
    print(f"({len(fs.server_names)} servers, backend {backend}; acc-changes are relative to "
          f"SLO scale {slo_scales[tref]:g} at load scale {scales[sref]:g})")
    return 0


def _cmd_plan_tokens(args) -> int:
    """What-if token-mix plan: the unlimited-mode solution at each pair of
    factors on the average input and output tokens and each load scale."""
    import numpy as np

    from .engine import FastSweep, SweepEngine

    token_scales = _parse_token_scales(args.token_scales)
    scales = _parse_scales(args.scales) if args.scales is not None else [1.0]
    system, _ = _load_system(args.spec)
    backend = SweepEngine(backend=args.backend).backend  # resolves "auto"
    fs = FastSweep(system, backend=backend)
    try:
        res = fs.plan_tokens(token_scales=token_scales, scales=scales)
    except ValueError as e:
        print(f"plan: {e}", file=sys.stderr)
        return 2
    # accelerator changes are relative to token scales 1:1 at load scale 1.0
    # (the first of either when that one is not among them)
    wref = token_scales.index((1.0, 1.0)) if (1.0, 1.0) in token_scales else 0
    sref = scales.index(1.0) if 1.0 in scales else 0
    acc = res.winners.acc_idx
    blocks = []
    for w, (f_in, f_out) in enumerate(token_scales):
        rows = [{
            "scale": scale,
            "totalCost": round(float(res.cost_total[w, s]), 2),
            "replicas": {
                name: int(res.replicas_by_acc[w, s, j]) for j, name in enumerate(fs.acc_names)
            },
            "infeasibleServers": int(res.infeasible_servers[w, s]),
            "acceleratorChanges": int(np.count_nonzero(acc[w, s] != acc[wref, sref])),
        } for s, scale in enumerate(scales)]
        blocks.append({"inTokenScale": f_in, "outTokenScale": f_out, "scenarios": rows})
    if args.json:
        print(json.dumps({"backend": backend,
                          "referenceTokenScales": list(token_scales[wref]),
                          "referenceScale": scales[sref], "servers": len(fs.server_names),
                          "tokenScenarios": blocks}, indent=2))
        return 0
    names = fs.acc_names
    for b in blocks:
        print(f"token scales {b['inTokenScale']:g}:{b['outTokenScale']:g} (average input "
              f"tokens x {b['inTokenScale']:g}, output tokens x {b['outTokenScale']:g})")
        print(f"{'scale':>8} {'cost':>12} " + " ".join(f"{n:>10}" for n in names)
              + f" {'infeasible':>10} {'acc-changes':>11}")
        for r in b["scenarios"]:
            print(f"{r['scale']:>8g} {r['totalCost']:>12.2f} "
                  + " ".join(f"{r['replicas'][n]:>10}" for n in names)
                  + f" {r['infeasibleServers']:>10} {r['acceleratorChanges']:>11}")
    ref_in, ref_out = token_scales[wref]
    print(f"({len(fs.server_names)} servers, backend {backend}; acc-changes are relative to "
          f"token scales {ref_in:g}:{ref_out:g} at load scale {scales[sref]:g})")
    return 0


def _cmd_plan_rollout(args) -> int:
    """Forecast rollout: the scales are consecutive ticks, each reconciled
    against the allocation the tick before it left behind."""
    from .engine import FastSweep, SweepEngine

    if args.scales is None:
        raise SystemExit("plan: --rollout needs --scales (one factor per step)")
    scales = _parse_scales(args.scales)
    system, _ = _load_system(args.spec)
    backend = SweepEngine(backend=args.backend).backend  # resolves "auto"
    fs = FastSweep(system, backend=backend)
    try:
        res = fs.rollout(scales=scales)
    except ValueError as e:
        print(f"plan: {e}", file=sys.stderr)
        return 2
    rows = [{
        "step": s,
        "scale": scale,
        "totalCost": round(float(res.cost_total[s]), 2),
        "replicas": {
            name: int(res.replicas_by_acc[s, j]) for j, name in enumerate(fs.acc_names)
        },
        "infeasibleServers": int(res.infeasible_servers[s]),
        "acceleratorChanges": int(res.acc_changes[s]),
    } for s, scale in enumerate(scales)]
    if args.json:
        print(json.dumps({"backend": backend, "servers": len(fs.server_names), "rollout": rows,
                          "acceleratorChangesTotal": int(res.acc_changes.sum())}, indent=2))
        return 0
    names = fs.acc_names
    print(f"{'step':>5} {'scale':>8} {'cost':>12} " + " ".join(f"{n:>10}" for n in names)
          + f" {'infeasible':>10} {'acc-changes':>11}")
    for r in rows:
        print(f"{r['step']:>5} {r['scale']:>8g} {r['totalCost']:>12.2f} "
              + " ".join(f"{r['replicas'][n]:>10}" for n in names)
              + f" {r['infeasibleServers']:>10} {r['acceleratorChanges']:>11}")
    print(f"({len(fs.server_names)} servers, backend {backend}; consecutive steps, acc-changes "
          f"are relative to the step before; {int(res.acc_changes.sum())} in all)")
    return 0


def _parse_ensemble_scales(text: str) -> list[list[float]]:
    paths = [_parse_scales(p, "--ensemble-scales") for p in text.split(";") if p.strip()]
    if not paths:
        raise SystemExit("--ensemble-scales: at least one path is required")
    if len({len(p) for p in paths}) != 1:
        raise SystemExit("--ensemble-scales: every path needs the same number of ticks, got "
                         + ", ".join(str(len(p)) for p in paths))
    return paths


def _cmd_plan_ensemble(args) -> int:
    """Forecast ensemble: E load paths of consecutive ticks, per tick and
    quantile the order statistics of the fleet across the paths."""
    from .engine import FastSweep, SweepEngine, noisy_paths

    if args.ensemble_scales is not None:
        if args.ensemble_noise is not None or args.scales is not None:
            raise SystemExit("plan: --ensemble-scales names the paths itself; it does not "
                             "combine with --ensemble-noise or --scales")
        paths = _parse_ensemble_scales(args.ensemble_scales)
    else:
        if args.scales is None:
            raise SystemExit("plan: --ensemble-noise needs --scales (the forecast, one factor "
                             "per tick)")
        try:
            paths = noisy_paths(_parse_scales(args.scales), args.ensemble_noise, args.paths,
                                args.seed).tolist()
        except ValueError as e:
            raise SystemExit(f"plan: --ensemble-noise: {e}")
    quantiles = _parse_scales(args.quantiles, "--quantiles")
    system, _ = _load_system(args.spec)
    backend = SweepEngine(backend=args.backend).backend  # resolves "auto"
    fs = FastSweep(system, backend=backend)
    try:
        res = fs.rollout_ensemble(scales=paths, quantiles=quantiles)
    except ValueError as e:
        print(f"plan: {e}", file=sys.stderr)
        return 2
    n_paths = len(paths)
    rows = [{
        "step": s,
        "quantile": float(q),
        "rank": int(res.ranks[k]),
        "totalCost": round(float(res.cost_total_q[k, s]), 2),
        "replicas": {
            name: int(res.replicas_by_acc_q[k, s, j]) for j, name in enumerate(fs.acc_names)
        },
        "infeasibleServers": int(res.infeasible_q[k, s]),
        "acceleratorChanges": int(res.acc_changes_q[k, s]),
        "unanimousServers": int((res.acc_mode_paths[s] == n_paths).sum()),
    } for s in range(len(paths[0])) for k, q in enumerate(res.quantiles)]
    if args.json:
        print(json.dumps({"backend": backend, "servers": len(fs.server_names), "paths": n_paths,
                          "steps": len(paths[0]), "ensemble": rows}, indent=2))
        return 0
    names = fs.acc_names
    print(f"{'step':>5} {'quantile':>8} {'cost':>12} " + " ".join(f"{n:>10}" for n in names)
          + f" {'infeasible':>10} {'acc-changes':>11} {'unanimous':>9}")
    for r in rows:
        print(f"{r['step']:>5} {r['quantile']:>8g} {r['totalCost']:>12.2f} "
              + " ".join(f"{r['replicas'][n]:>10}" for n in names)
              + f" {r['infeasibleServers']:>10} {r['acceleratorChanges']:>11} "
              f"{r['unanimousServers']:>9}")
    print(f"({len(fs.server_names)} servers, backend {backend}; {n_paths} paths of "
          f"{len(paths[0])} consecutive steps; every column is its own order statistic across "
          "the paths; unanimous = servers on which every path chose the same accelerator)")
    return 0


def _cmd_plan_hold(args) -> int:
    """Hold analysis: the current allocation, unchanged, at each load scale."""
    from .engine import HOLD_OK, HOLD_STATUS_NAMES, FastSweep, SweepEngine

    if args.scales is None:
        raise SystemExit("plan: --hold needs --scales")
    scales = _parse_scales(args.scales)
    system, _ = _load_system(args.spec)
    backend = SweepEngine(backend=args.backend).backend  # resolves "auto"
    fs = FastSweep(system, backend=backend)
    try:
        res = fs.hold(scales=scales)
    except ValueError as e:
        print(f"plan: {e}", file=sys.stderr)
        return 2
    rows = []
    for s, scale in enumerate(scales):
        rows.append({
            "scale": scale,
            "status": {n: int(res.counts[s, j]) for j, n in enumerate(HOLD_STATUS_NAMES)},
            "deficit": {n: int(res.deficit_by_acc[s, j]) for j, n in enumerate(fs.acc_names)},
            "notOk": [{
                "server": fs.server_names[i],
                "status": HOLD_STATUS_NAMES[res.status[s, i]],
                "accelerator": fs.acc_names[res.acc_idx[s, i]] if res.acc_idx[s, i] >= 0 else "",
                "heldReplicas": int(res.held_replicas[s, i]),
                "neededReplicas": int(res.needed_replicas[s, i]),
                # +inf (an overloaded server) has no JSON number
                "itl": float(res.itl[s, i]) if res.itl[s, i] != float("inf") else None,
                "ttft": float(res.ttft[s, i]) if res.ttft[s, i] != float("inf") else None,
            } for i in range(len(fs.server_names)) if res.status[s, i] != HOLD_OK],
        })
    if args.json:
        print(json.dumps({"backend": backend, "servers": len(fs.server_names), "hold": rows},
                         indent=2))
        return 0
    for r in rows:
        print(f"load scale {r['scale']:g}: "
              + ", ".join(f"{n} {c}" for n, c in r["status"].items() if c)
              + "; replicas short: "
              + (", ".join(f"{n} {d}" for n, d in r["deficit"].items() if d) or "none"))
        for b in r["notOk"]:
            lat = ("" if b["itl"] is None
                   else f" itl {b['itl']:.2f} ms ttft {b['ttft']:.2f} ms")
            print(f"  {b['server']:<24} {b['status']:<12} {b['accelerator'] or '-':<12} "
                  f"held {b['heldReplicas']} needed {b['neededReplicas']}{lat}")
    print(f"({len(fs.server_names)} servers, backend {backend}; the current allocation is held "
          "at every load scale)")
    return 0


def cmd_analyze(args) -> int:
    from .api import v1alpha1 as api
    from .controller.modelanalyzer import ModelAnalyzer
    from .engine import SweepEngine

    system, _ = _load_system(args.spec)
    name, _, ns = args.server.partition(":")
    va = api.VariantAutoscaling(name=name, namespace=ns or "default")
    resp = ModelAnalyzer(system, SweepEngine(backend=args.backend)).analyze_model(va)
    if not resp.allocations:
        print(f"no feasible allocations for {args.server}", file=sys.stderr)
        return 1
    print(f"{'accelerator':<16} {'replicas':>8} {'batch':>6} {'cost':>10} "
          f"{'value':>10} {'itl(ms)':>9} {'ttft(ms)':>9} {'rho':>6}")
    for acc in sorted(resp.allocations):
        a = resp.allocations[acc].allocation
        print(f"{acc:<16} {a.num_replicas:>8} {a.batch_size:>6} {a.cost:>10.2f} "
              f"{a.value:>10.2f} {a.itl:>9.2f} {a.ttft:>9.2f} {a.rho:>6.3f}")
    return 0


def main() -> None:
    p = argparse.ArgumentParser(prog="inferno_amd.cli")
    sub = p.add_subparsers(dest="cmd", required=True)
    ps = sub.add_parser("solve", help="global cost/SLO solve of a SystemData JSON")
    ps.add_argument("spec")
    ps.add_argument("--backend", choices=["auto", "gpu", "cpu"], default="auto")
    ps.add_argument("--json", action="store_true")
    ps.set_defaults(fn=cmd_solve)
    pp = sub.add_parser("plan", help="what-if plan: the fleet at several load scales")
    pp.add_argument("spec")
    pp.add_argument("--scales", default=None,
                    help="comma-separated load factors, e.g. 0.5,1,1.5,2")
    pp.add_argument("--slo-scales", default=None,
                    help="comma-separated factors on every TTFT and ITL target, e.g. 0.5,1,2: "
                         "one block per SLO scale (load scale 1 unless --scales is given)")
    pp.add_argument("--token-scales", default=None,
                    help="comma-separated IN:OUT factors on every server's average input and "
                         "output tokens, e.g. 1:1,4:1,1:0.5: one block per pair (load scale 1 "
                         "unless --scales is given)")
    pp.add_argument("--backend", choices=["auto", "gpu", "cpu"], default="auto")
    pp.add_argument("--json", action="store_true")
    pp.add_argument("--limited", action="store_true",
                    help="capacity-limited plan: inventory, saturation policy and "
                         "delayed best-effort from the spec")
    pp.add_argument("--capacity", default=None,
                    help="inventory as TYPE=N,...; implies --limited and replaces the spec's")
    pp.add_argument("--saturation-policy", default=None,
                    choices=["None", "PriorityExhaustive", "PriorityRoundRobin", "RoundRobin"])
    pp.add_argument("--delayed-best-effort", action="store_true")
    pp.add_argument("--rollout", action="store_true",
                    help="forecast rollout: --scales are consecutive steps, each reconciled "
                         "against the allocation the step before it left behind")
    pp.add_argument("--hold", action="store_true",
                    help="hold analysis: the current allocation is not resized; per load scale "
                         "the SLO verdict of every server, the replicas short by accelerator")
    pp.add_argument("--ensemble-scales", default=None,
                    help="forecast ensemble: load paths separated by ';', each a comma-separated "
                         "list of consecutive step factors of the same length, e.g. "
                         "'0.5,1,2;0.6,1.2,2.4'; per step and quantile the order statistics "
                         "across the paths")
    pp.add_argument("--quantiles", default="0.5,0.9,1",
                    help="quantiles of a forecast ensemble, each in (0, 1] (nearest rank)")
    pp.add_argument("--ensemble-noise", type=float, default=None, metavar="SIGMA",
                    help="forecast ensemble around --scales: --paths paths scale[s] x "
                         "exp(SIGMA x z), z standard normal; path 0 is the forecast itself")
    pp.add_argument("--paths", type=int, default=16, help="paths of --ensemble-noise")
    pp.add_argument("--seed", type=int, default=0, help="seed of --ensemble-noise")
    pp.set_defaults(fn=cmd_plan)
    pa = sub.add_parser("analyze", help="per-variant candidate allocations")
    pa.add_argument("spec")
    pa.add_argument("--server", required=True, help="name:namespace")
    pa.add_argument("--backend", choices=["auto", "gpu", "cpu"], default="auto")
    pa.set_defaults(fn=cmd_analyze)
    args = p.parse_args()
    sys.exit(args.fn(args))


if __name__ == "__main__":
    main()
