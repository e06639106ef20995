"""The fused reconcile tick (wva_tick_t: sweep and winner step in one launch)
against the bucket launches + wva_winner it replaces.

Every comparison is raw bits: the ten winner-record rows, the winner array and
the ten per-cell output arrays of a fused context against those of a second
context created under INFERNO_FUSED_TICK=0, on the same system and the same
sequence of ticks. The fused kernel runs the same cell function at the same
width per cell, so no tolerance applies.

Fleets are small: the tiers are brought down to small N by patching the bucket
thresholds of ops/sweep.py, and every cell gets its own batch size through the
per-cell override row.
"""
import numpy as np
import pytest

from inferno_amd.core import System
from inferno_amd.engine import FastSweep
from inferno_amd.engine.native_ctx import CELL_KEYS
from tests.fixtures import make_spec

pytestmark = pytest.mark.gpu

# tiers at small N: small <= 8 < medium <= 16 (one wave each), large <= 256 and
# XL <= 1024 (256 threads; an XL cell above 768 states needs more LDS than a
# large one or than four narrow slices), huge above (global-memory slab)
THRESHOLDS = {"N_SMALL": 8, "N_MED": 16, "MAX_N": 256, "XL_MAX_N": 1024}
SMALL, MED, LARGE, XL, XL_TOP, HUGE = 5, 16, 200, 600, 1024, 1500
ARRIVAL_SCALE = 6000.0


def patch_tiers(monkeypatch):
    import inferno_amd.ops.sweep as sweep

    for k, v in THRESHOLDS.items():
        monkeypatch.setattr(sweep, k, v)


def make_fs(n_servers, cell_n, seed=77, tweak=None, stat_tweak=None):
    """A FastSweep whose cell k has batch size cell_n[k] (cycled)."""
    system, _ = System.from_spec(
        make_spec(n_servers=n_servers, seed=seed, arrival_scale=ARRIVAL_SCALE))
    if tweak is not None:
        tweak(system)
    fs = FastSweep(system, backend="gpu")
    assert fs.n_cells == 3 * n_servers
    fs._stat["override"][:] = np.resize(np.asarray(cell_n, dtype=np.int32), fs.n_cells)
    if stat_tweak is not None:
        stat_tweak(fs)
    return system, fs


def loads_of(system, fs):
    names = fs.server_names
    arrival = np.array([system.servers[n].load.arrivalRate for n in names], dtype=np.float32)
    in_tok = np.array([system.servers[n].load.avgInTokens for n in names], dtype=np.int32)
    out_tok = np.array([system.servers[n].load.avgOutTokens for n in names], dtype=np.int32)
    return arrival, in_tok, out_tok


def no_cur(fs):
    n = len(fs.server_names)
    return (np.full(n, -3, dtype=np.int32), np.zeros(n, dtype=np.int32),
            np.zeros(n, dtype=np.float32))


def feed_back(cur, w):
    pa, pr, pc = cur
    ok = w.acc_idx != -1
    return (
        np.where(ok, np.where(w.acc_idx == -2, -1, w.acc_idx), pa).astype(np.int32),
        np.where(ok, w.num_replicas, pr).astype(np.int32),
        np.where(ok, w.cost, pc).astype(np.float32),
    )


class Pair:
    """The same fleet twice: a fused context and one under INFERNO_FUSED_TICK=0."""

    def __init__(self, monkeypatch, n_servers, cell_n, **kw):
        self.mp = monkeypatch
        self.system, self.fused = make_fs(n_servers, cell_n, **kw)
        _, self.legacy = make_fs(n_servers, cell_n, **kw)
        self.state = None

    def _run(self, fs, flag, load, cur):
        # the switch is read when the context is created, on the first tick
        self.mp.setenv("INFERNO_FUSED_TICK", flag)
        fs.load_override, fs.cur_override = load, cur
        w = fs.reconcile()
        g = fs._gpu
        cells = g.cells()
        return w, g.pin_out_np.copy(), g.winner.cpu().numpy(), cells, g.fused_state()

    def tick(self, load, cur, what, path=(1, 2)):
        """One tick on both; asserts bit equality and the counter invariant.
        Returns the fused winners, its per-cell arrays and its state."""
        w, rec, win, cells, state = self._run(self.fused, "1", load, cur)
        _, l_rec, l_win, l_cells, l_state = self._run(self.legacy, "0", load, cur)
        assert l_state["path"] == 0 and l_state["done_nonzero"] == -1, what
        assert state["path"] in path, f"{what}: path {state['path']}, expected {path}"
        if state["path"] != 0:
            assert state["done_nonzero"] == 0, f"{what}: arrival counters left non-zero"
        assert rec.tobytes() == l_rec.tobytes(), f"{what}: winner records differ"
        assert win.tobytes() == l_win.tobytes(), f"{what}: winner array differs"
        for k in CELL_KEYS:
            assert cells[k].tobytes() == l_cells[k].tobytes(), f"{what}: cell {k} differs"
        assert self.fused.memo_stats() == self.legacy.memo_stats(), f"{what}: memo counters"
        self.state = state
        return w, cells, state


# -- 1. task packing ----------------------------------------------------------
@pytest.mark.parametrize("name,cell_n,n_wide,n_quads", [
    # 15 narrow cells in two buckets (8 small, 7 medium): both last quads partial
    ("partial-quads", [SMALL, MED] * 7 + [SMALL], 0, 4),
    ("one-narrow", [LARGE] * 14 + [SMALL], 14, 1),
    ("no-narrow", [LARGE, XL, LARGE], 15, 0),
    ("no-wide", [SMALL] * 15, 0, 4),
])
def test_task_packing(monkeypatch, name, cell_n, n_wide, n_quads):
    patch_tiers(monkeypatch)
    pair = Pair(monkeypatch, 5, cell_n)
    load = loads_of(pair.system, pair.fused)
    cur = no_cur(pair.fused)
    for t in range(2):  # the second tick takes the memo hits
        w, cells, state = pair.tick(load, cur, f"{name} tick {t}", path=(1,))
        cur = feed_back(cur, w)
    assert state["n_tasks"] == n_wide + n_quads
    assert cells["feasible"].any()


# -- 2. servers spanning task kinds, one and two launches ---------------------
@pytest.mark.parametrize("xl_n,cus,path", [(XL, None, 1), (XL_TOP, "1", 2)])
def test_servers_spanning_kinds(monkeypatch, xl_n, cus, path):
    """Every server has a small, a large and an XL cell, so its last arriver
    can be a narrow wave or a wide block. With the CU count of the residency
    rule capped to 1 the XL tasks go to the second launch."""
    patch_tiers(monkeypatch)
    if cus is not None:
        monkeypatch.setenv("INFERNO_FUSED_TICK_CUS", cus)
    pair = Pair(monkeypatch, 6, [SMALL, LARGE, xl_n])
    load = loads_of(pair.system, pair.fused)
    cur = no_cur(pair.fused)
    for t in range(3):
        arr = (load[0] * np.float32((1.0, 1.9, 0.4)[t])).astype(np.float32)
        w, cells, state = pair.tick((arr, load[1], load[2]), cur, f"tick {t}", path=(path,))
        cur = feed_back(cur, w)
    assert state["n_tasks"] == 6 + 6 + 2
    assert state["n_tasks_second"] == (6 if path == 2 else 0)
    if path == 2:
        assert state["lds_second"] > state["lds_first"] > 0 and state["n_cus"] == 1
    assert (cells["batch"][cells["feasible"].astype(bool)] > 0).any()


# -- 3. every exit arrives -----------------------------------------------------
ZERO_KEEP, ZERO_EMPTY, NO_OUT, INFEASIBLE, DEGENERATE = 0, 1, 2, 3, 4


def exits_tweak(system):
    names = sorted(system.servers)
    # unloaded and allowed to scale to zero: three equal empty allocations, a tie
    # (as tie_system() of test_native_tick_gpu.py)
    system.servers[names[ZERO_EMPTY]].min_num_replicas = 0
    # unreachable SLO on every cell of the server
    srv = system.servers[names[INFEASIBLE]]
    t = system.service_classes[srv.service_class_name].targets[srv.model_name]
    t.itl = 1e-3
    t.ttft = 0.0


def exits_stat_tweak(fs):
    # one cell with all-zero service times: the degenerate-rate exit
    k = int(fs.seg_start[DEGENERATE]) + 1
    for key in ("alpha", "beta", "gamma", "delta"):
        fs._stat[key][k] = 0.0


def test_every_exit_arrives(monkeypatch):
    patch_tiers(monkeypatch)
    pair = Pair(monkeypatch, 7, [SMALL, LARGE, XL, MED, SMALL, LARGE, XL, MED],
                tweak=exits_tweak, stat_tweak=exits_stat_tweak)
    arrival, in_tok, out_tok = loads_of(pair.system, pair.fused)
    arrival = arrival.copy()
    out_tok = out_tok.copy()
    arrival[ZERO_KEEP] = 0.0
    arrival[ZERO_EMPTY] = 0.0
    out_tok[NO_OUT] = 0
    cur = no_cur(pair.fused)
    seg = pair.fused.seg_start
    for t in range(2):
        w, cells, _ = pair.tick((arrival, in_tok, out_tok), cur, f"tick {t}")
        cur = feed_back(cur, w)
        feas = cells["feasible"].astype(bool)
        zero = cells["zero_empty"].astype(bool)
        # the fixture takes the exits it claims to
        assert feas[seg[ZERO_KEEP]:seg[ZERO_KEEP + 1]].all()
        assert not zero[seg[ZERO_KEEP]:seg[ZERO_KEEP + 1]].any()
        assert zero[seg[ZERO_EMPTY]:seg[ZERO_EMPTY + 1]].all() and w.acc_idx[ZERO_EMPTY] == -2
        assert pair.fused._gpu.pin_out_np[9][ZERO_EMPTY] == seg[ZERO_EMPTY], "tie: lowest cell"
        assert feas[seg[NO_OUT]:seg[NO_OUT + 1]].all()
        assert not feas[seg[INFEASIBLE]:seg[INFEASIBLE + 1]].any()
        assert w.acc_idx[INFEASIBLE] == -1
        assert not feas[seg[DEGENERATE] + 1]
        assert (feas & ~zero & (cells["rho"] > 0)).any(), "no sized cell"
    hits, misses = pair.fused.memo_stats()
    # the second tick replays every loaded cell, the infeasible ones included
    assert hits == misses and hits >= 3 + 1 + 3


# -- 4. counter state across ticks and a layout change -------------------------
def test_counters_stay_zero_across_ticks(monkeypatch):
    patch_tiers(monkeypatch)
    pair = Pair(monkeypatch, 6, [SMALL, LARGE, XL, MED, MED, SMALL, LARGE])
    arrival, in_tok, out_tok = loads_of(pair.system, pair.fused)
    cur = no_cur(pair.fused)
    stale = []
    for t, scale in enumerate((1.0, 1.7, 0.6, 2.3, 0.9, 1.3)):
        arr = (arrival * np.float32(scale)).astype(np.float32)
        if t == 3:
            arr[2] = 0.0  # the server's cells drop to batch_n 1: the layout goes stale
        w, _, _ = pair.tick((arr, in_tok, out_tok), cur, f"tick {t}")
        stale.append(pair.fused._gpu.tick_stale)
        cur = feed_back(cur, w)
    assert stale == [True, False, False, True, True, False]


# -- 5. servers sharing output lines finish far apart ---------------------------
def test_line_sharing_under_uneven_load(monkeypatch):
    """700 servers: neighbours alternate between one-state cells and cells at
    the top of the medium tier (2048 states, default thresholds), so the sixteen
    cells of a 64-byte output line are stored far apart in time and every CU
    runs several winner steps. A regression check for the acquire in front of
    the winner's loads, not a proof of it."""
    for k in ("INFERNO_N_SMALL", "INFERNO_N_MED", "INFERNO_XL_MAX_N"):
        monkeypatch.delenv(k, raising=False)
    cell_n = [1, 1, 1, 2048, 2048, 2048]
    pair = Pair(monkeypatch, 700, cell_n)
    arrival, in_tok, out_tok = loads_of(pair.system, pair.fused)
    cur = no_cur(pair.fused)
    for t, scale in enumerate((1.0, 2.1, 0.5)):
        arr = (arrival * np.float32(scale)).astype(np.float32)
        w, cells, state = pair.tick((arr, in_tok, out_tok), cur, f"tick {t}", path=(1,))
        cur = feed_back(cur, w)
    assert state["n_tasks"] == 2 * ((1050 + 3) // 4)
    assert cells["feasible"].any()


# -- 6. fallback -----------------------------------------------------------------
def test_fallback_other_width(monkeypatch):
    patch_tiers(monkeypatch)
    monkeypatch.setenv("INFERNO_NT_LARGE", "512")
    pair = Pair(monkeypatch, 5, [SMALL, LARGE, XL])
    load = loads_of(pair.system, pair.fused)
    w, cells, state = pair.tick(load, no_cur(pair.fused), "512-wide large bucket", path=(0,))
    assert state["n_tasks"] == 0 and cells["feasible"].any()


def test_fallback_large_grid(monkeypatch):
    """More tasks than one round of blocks (4 per CU): the bucket launches."""
    patch_tiers(monkeypatch)
    n_servers = 342  # 1026 wide tasks; an MI355X has 256 CUs
    pair = Pair(monkeypatch, n_servers, [LARGE])
    load = loads_of(pair.system, pair.fused)
    n_cus = None
    cur = no_cur(pair.fused)
    for t in range(2):
        w, cells, state = pair.tick(load, cur, f"large grid tick {t}", path=(0, 1))
        cur = feed_back(cur, w)
        n_cus = state["n_cus"]
        assert state["path"] == (0 if 3 * n_servers > 4 * n_cus else 1)
    assert n_cus > 0 and cells["feasible"].any()


def test_fallback_huge_tier(monkeypatch):
    patch_tiers(monkeypatch)
    pair = Pair(monkeypatch, 5, [SMALL, LARGE, XL] * 4 + [SMALL, LARGE, HUGE])
    load = loads_of(pair.system, pair.fused)
    cur = no_cur(pair.fused)
    for t in range(2):
        w, cells, state = pair.tick(load, cur, f"huge tier tick {t}", path=(0,))
        cur = feed_back(cur, w)
    assert cells["feasible"].any()
