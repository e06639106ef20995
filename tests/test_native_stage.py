"""Host-only pieces of the native reconcile tick (ops/native/stage.cpp) and the
world-size-1 shortcut of ShardedSolver.solve, all on the CPU.

* wva_stage_dynamic against FastSweep._refresh_dynamic, the reference it
  replaces on the hot path: the eight dynamic rows byte for byte.
* wva_aggregate_by_type against the numpy path of
  ShardedSolver._aggregate_by_type: counts equal, fp64 costs equal in bits.
* solve() with the shortcut against solve() forced through the generic
  encode/scatter path.

Comparisons are exact: both sides copy or add the same values in the same
order, so no tolerance applies.
"""
import dataclasses
import os
import shutil

import numpy as np
import pytest

from inferno_amd.core import System
from inferno_amd.engine import FastSweep, SweepEngine
from inferno_amd.ops import sweep as ops_sweep
from inferno_amd.ops.build import HIPCC, LIB_PATH
from inferno_amd.parallel import ShardedSolver
from tests.fixtures import make_spec
from tests.test_sizing_memo import PINNED_N
from tests.test_sizing_memo import build_system as pinned_system

ROWS = ("in_tok", "out_tok", "batch_n", "perf_max_batch", "cur_replicas", "flags",
        "arrival_rate", "cur_cost")
# (name, servers, seed); "pinned" is the 8-server x 3-accelerator fixture of
# test_sizing_memo.py (batch override N = 1, 33, 512, 513, 2048, 2049, 8193)
FLEETS = (("pinned", 8, 901), ("seeded", 8, 11), ("seeded", 23, 12), ("seeded", 40, 13))
CASES = ("base", "arrival_zero", "out_tok_zero", "out_tok_huge", "override_flip", "nan_arrival",
         "plan")


@pytest.fixture(scope="module")
def ops():
    """The loaded native library. Skipped only where there is neither a
    compiler nor a prebuilt library; a failing build, link or symbol lookup
    fails the tests."""
    if shutil.which(HIPCC) is None and not os.path.exists(LIB_PATH):
        pytest.skip(f"no {HIPCC} and no prebuilt {LIB_PATH}")
    ops_sweep.load_library(allow_build=True)
    return ops_sweep


def build_fleet(kind, n_srv, seed, flip_override=False):
    if kind == "pinned":
        system = pinned_system(seed=seed)
        assert len(system.servers) == len(PINNED_N)
    else:
        system, _ = System.from_spec(make_spec(n_servers=n_srv, seed=seed))
    if flip_override:
        # override set <-> unset on every other server (read at construction)
        for i, name in enumerate(sorted(system.servers)):
            if i % 2 == 0:
                srv = system.servers[name]
                srv.max_batch_size = 0 if srv.max_batch_size > 0 else 96 + i
    fs = FastSweep(system, backend="cpu")
    assert fs.n_cells == 3 * len(fs.server_names)
    return fs


def base_inputs(fs, seed):
    """Per-server overrides covering cur_acc's four cases on every fleet:
    none (-3), empty (-1), an accelerator that is one of the server's cells
    (same on that cell, other on the rest)."""
    rng = np.random.default_rng(seed)
    n = len(fs.server_names)
    arrival, in_tok, out_tok = (a.copy() for a in fs._base_load())
    n_acc = len(fs.acc_names)
    cur_acc = np.array([(-3, -1, 0, n_acc - 1, 1)[i % 5] for i in range(n)], dtype=np.int32)
    cur_rep = rng.integers(0, 9, size=n).astype(np.int32)
    cur_cost = rng.uniform(0, 500, size=n).astype(np.float32)
    return [arrival, in_tok, out_tok], [cur_acc, cur_rep, cur_cost]


def apply_case(case, load, n):
    arrival, in_tok, out_tok = load
    plan = None
    if case == "arrival_zero":
        arrival[::3] = 0.0
        arrival[1] = -0.0  # compares equal to 0 like +0
    elif case == "out_tok_zero":
        out_tok[1::3] = 0
    elif case == "out_tok_huge":
        out_tok[::2] = np.iinfo(np.int32).max  # scaled batch clamps to 1
        out_tok[1] = 1 << 20
    elif case == "nan_arrival":
        arrival[0] = np.nan  # not zero-load
        arrival[n - 1] = 0.0
    elif case == "plan":
        # three scenarios; server 0 unloaded in all of them, server 1 in two
        plan = np.stack([arrival * np.float32(f) for f in (0.5, 1.0, 2.5)]).astype(np.float32)
        plan[:, 0] = 0.0
        plan[:2, 1] = 0.0
    return plan


def reference_rows(fs, plan=None):
    arrs = fs._refresh_dynamic(plan_arrival=plan)
    out = []
    for k in ROWS:
        a = np.ascontiguousarray(arrs[k])
        assert a.dtype == (np.float32 if k in ("arrival_rate", "cur_cost") else np.int32), k
        out.append(a.view(np.int32))
    return np.stack(out)


def native_rows(ops, fs, plan=None, prev_batch_n=None, split_zero=False):
    arrival, in_tok, out_tok = fs._base_load()
    zero = None
    if plan is not None:
        zero = plan.max(axis=0).astype(np.float32)
        if not split_zero:
            arrival = zero  # what _refresh_dynamic puts into its arrival row
    cur_acc, cur_rep, cur_cost = fs._base_cur()
    return ops.run_stage_dynamic(
        arrival, in_tok, out_tok, cur_acc, cur_rep, cur_cost, fs.cell_server, fs.cell_acc_idx,
        fs._stat["perf_max_batch_cfg"], fs._stat["at_tokens"], fs._stat["override"],
        zero_arrival=zero, prev_batch_n=prev_batch_n,
    )


@pytest.mark.parametrize("fleet", FLEETS, ids=lambda f: f"{f[0]}{f[1]}")
@pytest.mark.parametrize("case", CASES)
def test_staging_equals_refresh_dynamic(ops, fleet, case):
    fs = build_fleet(*fleet, flip_override=(case == "override_flip"))
    load, cur = base_inputs(fs, fleet[2])
    plan = apply_case(case, load, len(fs.server_names))
    fs.load_override, fs.cur_override = tuple(load), tuple(cur)
    want = reference_rows(fs, plan)
    got, changed = native_rows(ops, fs, plan)
    assert changed  # no previous batch_n given
    assert got.dtype == np.int32 and got.shape == want.shape
    for j, k in enumerate(ROWS):
        assert got[j].tobytes() == want[j].tobytes(), f"row {k} differs"
    flags = want[ROWS.index("flags")]
    assert {0, 4, 5, 6} <= set(flags.tolist()), "fixture misses one of cur_acc's cases"
    if case == "out_tok_huge":
        huge = want[1] == np.iinfo(np.int32).max
        unset = fs._stat["override"] == 0
        assert (want[2][huge & unset] == 1).all()
        # the pinned fixture overrides every server's batch: nothing to clamp there
        assert (huge & unset).any() == (fleet[0] == "seeded")
    if case == "plan":
        # with the zero-load decision split off, only the arrival row changes
        split, _ = native_rows(ops, fs, plan, split_zero=True)
        base = fs._base_load()[0][fs.cell_server]
        for j, k in enumerate(ROWS):
            ref = base.view(np.int32) if k == "arrival_rate" else want[j]
            assert split[j].tobytes() == np.ascontiguousarray(ref).tobytes(), f"row {k}"
        cells0 = fs.cell_server == 0
        assert (want[2][cells0] == 1).all()  # unloaded in every scenario


@pytest.mark.parametrize("fleet", FLEETS, ids=lambda f: f"{f[0]}{f[1]}")
def test_changed_report_tracks_batch_n(ops, fleet):
    fs = build_fleet(*fleet)
    load, cur = base_inputs(fs, fleet[2])
    fs.load_override, fs.cur_override = tuple(load), tuple(cur)
    first, _ = native_rows(ops, fs)
    prev = first[2].copy()
    steps = []
    # same loads; other currents only; a server unloaded; token averages moved; back
    steps.append((load, cur))
    cur2 = [np.roll(cur[0], 1), cur[1] + 1, cur[2] * np.float32(2)]
    steps.append((load, cur2))
    zeroed = [load[0].copy(), load[1], load[2]]
    zeroed[0][2] = 0.0
    steps.append((zeroed, cur2))
    steps.append((zeroed, cur))  # still unloaded: no change against the previous tick
    moved = [load[0], load[1] + 3, (load[2] // 2 + 1).astype(np.int32)]
    steps.append((moved, cur))
    steps.append((load, cur))
    seen = []
    for ld, cu in steps:
        fs.load_override, fs.cur_override = tuple(ld), tuple(cu)
        rows, changed = native_rows(ops, fs, prev_batch_n=prev)
        want = not np.array_equal(rows[2], prev)
        assert changed == want
        assert np.array_equal(rows[2], reference_rows(fs)[2])
        seen.append(changed)
        prev = rows[2].copy()
    assert seen[:2] == [False, False]
    assert any(seen), "no step changed batch_n: the report was never exercised"


def numpy_by_type(acc_idx, num_replicas, cost, valid, inst, mult, type_idx, n_types):
    """The numpy path of ShardedSolver._aggregate_by_type."""
    tcount = np.zeros(n_types, dtype=np.int64)
    tcost = np.zeros(n_types, dtype=np.float64)
    idx = np.nonzero(valid & (acc_idx >= 0))[0]
    if len(idx):
        codes = acc_idx[idx]
        counts = (num_replicas[idx] * inst[idx, codes] * mult[codes]).astype(np.int64)
        np.add.at(tcount, type_idx[codes], counts)
        np.add.at(tcost, type_idx[codes], cost[idx].astype(np.float64))
    return tcount, tcost


@pytest.mark.parametrize("n_acc,n_types", [(3, 2), (5, 3), (8, 4), (8, 2)])
@pytest.mark.parametrize("kind", ["mixed", "all_empty", "all_invalid"])
def test_aggregate_by_type_equals_numpy(ops, n_acc, n_types, kind):
    rng = np.random.default_rng(100 * n_acc + n_types)
    for n_srv in (0, 1, 37, 512):
        acc_idx = rng.integers(-2, n_acc, size=n_srv).astype(np.int32)  # -2, -1 and real
        if kind == "all_empty":
            acc_idx = rng.choice(np.array([-1, -2], dtype=np.int32), size=n_srv)
        num_replicas = rng.integers(0, 400, size=n_srv).astype(np.int32)
        # fp32 costs of very different magnitude: the fp64 sum depends on the order
        cost = (rng.uniform(0, 1, size=n_srv) * 10.0 ** rng.integers(-3, 7, size=n_srv)).astype(
            np.float32)
        valid = rng.random(n_srv) < 0.8
        if kind == "all_invalid":
            valid[:] = False
        inst = rng.integers(0, 9, size=(n_srv, n_acc)).astype(np.int32)
        mult = rng.integers(1, 5, size=n_acc).astype(np.int32)
        type_idx = rng.integers(0, n_types, size=n_acc).astype(np.int32)
        type_idx[:n_types] = np.arange(n_types)  # every type has an accelerator
        args = (acc_idx, num_replicas, cost, valid, inst, mult, type_idx, n_types)
        want_count, want_cost = numpy_by_type(*args)
        got_count, got_cost = ops.run_aggregate_by_type(*args)
        assert got_count.dtype == np.int64 and got_cost.dtype == np.float64
        assert np.array_equal(got_count, want_count)
        assert got_cost.view(np.uint64).tolist() == want_cost.view(np.uint64).tolist()
        if kind != "mixed":
            assert not got_count.any() and not got_cost.any()


def solve_world1(force_generic, native_agg, monkeypatch):
    # the solver aggregates natively exactly when the library is loaded
    monkeypatch.setattr(ops_sweep, "library_loaded", lambda: native_agg)
    spec = make_spec(n_servers=16, seed=314, arrival_scale=600.0, min_num_replicas=0)
    system, opt = System.from_spec(spec)
    # one zero-load server (scales to zero: acc_idx -2) and one without a feasible allocation (-1)
    names = sorted(system.servers)
    system.servers[names[3]].load.arrivalRate = 0.0
    srv = system.servers[names[5]]
    t = system.service_classes[srv.service_class_name].targets[srv.model_name]
    t.itl, t.ttft = 1e-3, 0.0
    solver = ShardedSolver(SweepEngine(backend="cpu"))
    solver.force_generic_gather = force_generic
    return solver.solve(system, opt)


def test_world1_shortcut_equals_generic_path_native_agg(ops, monkeypatch):
    check_world1(solve_world1(False, True, monkeypatch), solve_world1(True, False, monkeypatch))


def test_world1_shortcut_equals_generic_path_numpy_agg(monkeypatch):
    # no native code involved: runs wherever numpy does
    check_world1(solve_world1(False, False, monkeypatch), solve_world1(True, False, monkeypatch))


def check_world1(fast, slow):
    codes = set(fast.winners.acc_idx.tolist())
    assert -2 in codes and -1 in codes and max(codes) >= 0
    for f in dataclasses.fields(fast.winners):
        a, b = getattr(fast.winners, f.name), getattr(slow.winners, f.name)
        if isinstance(a, np.ndarray):
            assert a.dtype == b.dtype and a.shape == b.shape, f.name
            assert a.tobytes() == b.tobytes(), f"winners.{f.name} differs"
        else:
            assert a == b, f.name
    assert fast.winners.valid.dtype == np.bool_ and fast.winners.valid.all()
    assert sorted(fast.allocation_by_type) == sorted(slow.allocation_by_type)
    for t, a in fast.allocation_by_type.items():
        b = slow.allocation_by_type[t]
        assert (a.name, a.count, a.limit) == (b.name, b.count, b.limit)
        assert np.float64(a.cost).view(np.uint64) == np.float64(b.cost).view(np.uint64)
    assert fast.solution == slow.solution
    assert list(fast.solution) == list(slow.solution)


def test_abi_constants_match_the_python_mirrors(ops):
    """What wva_abi() reports is what ops/sweep.py and engine/native_ctx.py
    assume (load_library has already refused a library where it is not), and
    the dead one-shot entry points are gone from the library."""
    import ctypes

    from inferno_amd.engine import native_ctx

    lib = ops.load_library()
    got = {name: lib.wva_abi(name.encode()) for name in ops._ABI}
    assert got == ops._ABI
    assert got == {
        "WVA_MAX_N": ops.MAX_N, "WVA_XL_MAX_N": 32768, "WVA_HUGE_MAX_N": ops.HUGE_MAX_N,
        "WVA_PLAN_MAX_S": ops.PLAN_MAX_S, "WVA_N_SMALL": 512, "WVA_N_MED": 2048,
        "WVA_TICK_STALE": ops.TICK_STALE, "WVA_DYN_ROWS": ops.DYN_ROWS,
        "WVA_REC_ROWS": ops.REC_ROWS, "WVA_MAX_BUCKETS": ops.MAX_BUCKETS,
    }
    assert (ops.MAX_N, ops.HUGE_MAX_N, ops.PLAN_MAX_S) == (8192, 1 << 22, 256)
    assert (ops.TICK_STALE, ops.DYN_ROWS, ops.REC_ROWS, ops.MAX_BUCKETS) == (1 << 20, 8, 10, 5)
    assert lib.wva_abi(b"WVA_CTX_SLOTS") == len(native_ctx.CTX_SLOT_NAMES) == 26
    assert len(set(native_ctx.CTX_SLOT_NAMES)) == 26
    assert ops.DYN_ROWS == len(native_ctx.DYN_INT) + len(native_ctx.DYN_F32)
    assert lib.wva_abi(b"WVA_NO_SUCH_CONSTANT") == -1 and lib.wva_abi(None) == -1
    for gone in ("wva_gather", "wva_sweep_launch"):
        with pytest.raises(AttributeError):
            getattr(ctypes.CDLL(LIB_PATH), gone)
    assert ctypes.CDLL(LIB_PATH).wva_sweep_launch_bucket is not None


def test_abi_mismatch_is_refused_by_name(ops, monkeypatch):
    ops.load_library()
    monkeypatch.setattr(ops, "_lib", None)
    monkeypatch.setitem(ops._ABI, "WVA_REC_ROWS", 11)
    with pytest.raises(ops.HipKernelError, match="WVA_REC_ROWS"):
        ops.load_library(allow_build=False)
