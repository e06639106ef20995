"""The native reconcile tick on the GPU (wva_ctx_tick, the fused wva_winner
kernel, the single dynamic block and the single winner block), on the 24-cell
fixture of test_sizing_memo.py (8 servers x 3 accelerators, pinned batch sizes
1 .. 8193, one server with an unreachable SLO).

Comparisons are bit for bit: the winner kernel only selects and copies what the
sweep wrote, and a tick only stages what _refresh_dynamic() computes.
"""
import dataclasses

import numpy as np
import pytest

from inferno_amd.engine import FastSweep
from tests.test_sizing_memo import (
    INFEASIBLE_SRV,
    ZERO_SRV,
    base_loads,
    build_system,
    feed_back,
    initial_cur,
    tick_arrival,
)

pytestmark = pytest.mark.gpu

RECORD_FLOATS = ("cost", "value", "itl", "ttft", "rho", "max_rate")
SENTINEL = np.int32(-559038737)  # 0xDEADBEEF; as fp32 about -6.26e18, no record holds it


def tie_system():
    """The fixture with ZERO_SRV allowed to scale to zero: unloaded, its three
    cells all hold the same empty allocation, so their values tie."""
    system = build_system()
    names = sorted(system.servers)
    system.servers[names[ZERO_SRV]].min_num_replicas = 0
    return system


def assert_records_equal(a, b, what):
    for f in dataclasses.fields(a):
        x, y = getattr(a, f.name), getattr(b, f.name)
        assert x.dtype == y.dtype and x.shape == y.shape, f"{what}: {f.name}"
        assert x.tobytes() == y.tobytes(), f"{what}: winner {f.name} differs"


def host_records(cells):
    """wva_argmin's rule then wva_gather's record, from per-cell outputs."""
    seg = cells["seg_start"]
    n_srv = len(seg) - 1
    rec = {k: np.zeros(n_srv, dtype=np.float32) for k in RECORD_FLOATS}
    acc = np.full(n_srv, -1, dtype=np.int32)
    reps = np.zeros(n_srv, dtype=np.int32)
    batch = np.zeros(n_srv, dtype=np.int32)
    win = np.full(n_srv, -1, dtype=np.int32)
    for s in range(n_srv):
        best = -1
        for i in range(seg[s], seg[s + 1]):
            if not cells["feasible"][i]:
                continue
            # strict <: the lowest cell index wins a tie
            if best == -1 or cells["value"][i] < cells["value"][best]:
                best = i
        win[s] = best
        if best == -1:
            continue
        acc[s] = -2 if cells["zero_empty"][best] else cells["cell_acc_idx"][best]
        reps[s] = cells["num_replicas"][best]
        batch[s] = cells["batch"][best]
        for k in RECORD_FLOATS:
            rec[k][s] = cells[k][best]
    return acc, reps, batch, rec, win


def test_winner_records_equal_host_argmin_and_gather():
    system = tie_system()
    fs = FastSweep(system, backend="gpu")
    assert fs.n_cells == 24
    arrival, in_tok, out_tok = base_loads(system)
    arrival = arrival.copy()
    arrival[ZERO_SRV] = 0.0
    fs.load_override = (arrival, in_tok, out_tok)
    fs.cur_override = initial_cur(system, fs)
    cells = fs.reconcile_cells()
    w = fs.reconcile()
    acc, reps, batch, rec, win = host_records(cells)

    # the fixture holds what the test is about
    seg = fs.seg_start
    zc = slice(seg[ZERO_SRV], seg[ZERO_SRV + 1])
    assert cells["feasible"][zc].all() and cells["zero_empty"][zc].all()
    assert len(set(cells["value"][zc].view(np.uint32).tolist())) == 1, "no tie on the zero server"
    assert win[ZERO_SRV] == seg[ZERO_SRV] and acc[ZERO_SRV] == -2
    ic = slice(seg[INFEASIBLE_SRV], seg[INFEASIBLE_SRV + 1])
    assert not cells["feasible"][ic].any() and acc[INFEASIBLE_SRV] == -1
    assert (acc >= 0).sum() >= 4, "no ordinary servers"

    assert w.acc_idx.dtype == np.int32 and w.acc_idx.tobytes() == acc.tobytes()
    assert w.num_replicas.tobytes() == reps.tobytes()
    assert w.batch.tobytes() == batch.tobytes()
    for k in RECORD_FLOATS:
        got = getattr(w, k)
        assert got.dtype == np.float32 and got.tobytes() == rec[k].tobytes(), k
    # the winner cell index: row 9 of the record block and the device array
    assert fs._gpu.pin_out_np[9].tobytes() == win.tobytes()
    assert fs._gpu.winner.cpu().numpy().tobytes() == win.tobytes()


DYN_ROWS = ("in_tok", "out_tok", "batch_n", "perf_max_batch", "cur_replicas", "flags",
            "arrival_rate", "cur_cost")


def assert_staged_block(fs, want, what):
    """The pinned dynamic block the context staged against _refresh_dynamic()'s arrays."""
    got = fs._gpu.pin_dyn_np
    assert got.shape == (len(DYN_ROWS), fs.n_cells)
    for j, k in enumerate(DYN_ROWS):
        ref = np.ascontiguousarray(want[k])
        assert ref.dtype.itemsize == 4, k
        assert got[j].tobytes() == ref.tobytes(), f"{what}: staged row {k} differs"


def test_context_stages_what_refresh_dynamic_computes():
    """Through the context, i.e. with the topology arrays as _ensure_ctx hands
    them over. Two servers lose their batch override so that the profile's
    maxBatchSize, atTokens and the override each show in a row of their own."""
    system = tie_system()
    names = sorted(system.servers)
    for i in (1, 4):
        system.servers[names[i]].max_batch_size = 0
    fs = FastSweep(system, backend="gpu")
    ovr = fs._stat["override"]
    assert (ovr > 0).any() and (ovr == 0).any()
    assert (fs._stat["perf_max_batch_cfg"] != fs._stat["at_tokens"]).all()
    arrival, in_tok, out_tok = base_loads(system)
    arrival = arrival.copy()
    arrival[ZERO_SRV] = 0.0
    fs.load_override = (arrival, in_tok, out_tok)
    fs.cur_override = initial_cur(system, fs)
    fs.reconcile()
    assert_staged_block(fs, fs._refresh_dynamic(), "reconcile")
    # planning: zero-load decided by the maximum over the scenarios
    scen = fs._plan_scenarios([0.0, 0.5, 2.0], None)
    scen[:, 2] = 0.0
    fs.plan(arrival=scen)
    assert_staged_block(fs, fs._refresh_dynamic(plan_arrival=scen), "plan")


def one_tick(monkeypatch, load, cur):
    """A fresh context without a sizing memo that sees only this tick."""
    monkeypatch.setenv("INFERNO_SIZING_MEMO", "0")
    system = tie_system()
    fs = FastSweep(system, backend="gpu")
    fs.load_override, fs.cur_override = load, cur
    w = fs.reconcile()
    assert fs._gpu.tick_stale, "a context's first tick must set its buckets"
    assert fs.memo_stats() is None
    monkeypatch.delenv("INFERNO_SIZING_MEMO")
    return w


def test_feedback_loop_across_layout_changes(monkeypatch):
    monkeypatch.delenv("INFERNO_SIZING_MEMO", raising=False)
    system = tie_system()
    fs = FastSweep(system, backend="gpu")
    arrival, in_tok, out_tok = base_loads(system)
    cur = initial_cur(system, fs)
    stale, want_stale, prev_batch = [], [], None
    for tick in range(4):
        # ZERO_SRV unloaded on tick 2 only: the layout goes stale there and on tick 3
        load = (tick_arrival(arrival, tick, 2), in_tok, out_tok)
        fs.load_override, fs.cur_override = load, cur
        batch_n = fs._refresh_dynamic()["batch_n"]
        want_stale.append(prev_batch is None or not np.array_equal(batch_n, prev_batch))
        prev_batch = batch_n.copy()
        w = fs.reconcile()
        stale.append(fs._gpu.tick_stale)
        assert_records_equal(w, one_tick(monkeypatch, load, cur), f"tick {tick}")
        assert (w.acc_idx[ZERO_SRV] == -2) == (tick == 2)
        cur = feed_back(cur, w)
    assert want_stale == [True, False, True, True]
    assert stale == want_stale
    assert fs._gpu.stale_ticks == 3
    hits, _ = fs.memo_stats()
    assert hits > 0, "the long-lived context never took a memo hit"


def test_no_stale_output_survives_a_tick():
    system = tie_system()
    fs = FastSweep(system, backend="gpu")
    arrival, in_tok, out_tok = base_loads(system)
    fs.load_override = (arrival, in_tok, out_tok)
    fs.cur_override = initial_cur(system, fs)
    first = fs.reconcile()
    pin = fs._gpu.pin_out_np
    assert pin.shape == (10, len(fs.server_names))
    pin[:] = SENTINEL
    fs._gpu.pin_dyn_np[:] = SENTINEL  # the staging block is rewritten in full, too
    second = fs.reconcile()
    assert not fs._gpu.tick_stale
    assert not (pin == SENTINEL).any(), "part of the winner block was not written"
    assert not (fs._gpu.pin_dyn_np == SENTINEL).any()
    assert_records_equal(first, second, "same inputs")
    for f in dataclasses.fields(second):
        assert not (getattr(second, f.name).view(np.int32) == SENTINEL).any(), f.name
