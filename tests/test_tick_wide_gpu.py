"""The two instantiations of the fused tick kernel (wva_tick_t<2>: 192 VGPRs,
no scratch, for launches whose dynamic LDS holds a CU to two blocks anyway;
wva_tick_t<4>: 128 VGPRs, every other launch) against the bucket launches.

As in test_fused_tick_gpu.py every comparison is raw bits: the winner records,
the winner array and the ten per-cell output arrays of a fused context against
those of a context created under INFERNO_FUSED_TICK=0, over three ticks with
changing loads (the first misses the sizing memo, the others hit it), and the
arrival counters are all zero after each tick. Each fleet is the smallest that
reaches its path; which instantiation a launch took is read from
fused_state().
"""
import numpy as np
import pytest

from inferno_amd.ops.sweep import load_library
from tests.test_fused_tick_gpu import (LARGE, SMALL, Pair, feed_back, loads_of, no_cur,
                                       patch_tiers)

pytestmark = pytest.mark.gpu

# default tiers: an XL cell of 16 384 states needs 69 952 B of LDS (two blocks
# per CU), a large cell of 4096 states and four medium slices of 2048 need less
# than 40 KB (four blocks per CU)
XL_N, LARGE_N, MED_N, SMALL_N = 16384, 4096, 2048, 300
LDS_OPT_IN = 64 * 1024
SCALES = (1.0, 1.9, 0.4)


def bounds():
    lib = load_library()
    return lib.wva_abi(b"WVA_TICK_WIDE_WAVES"), lib.wva_abi(b"WVA_TICK_MAX_WAVES")


def default_tiers(monkeypatch):
    for k in ("INFERNO_N_SMALL", "INFERNO_N_MED", "INFERNO_XL_MAX_N"):
        monkeypatch.delenv(k, raising=False)


def three_ticks(pair, path):
    arrival, in_tok, out_tok = loads_of(pair.system, pair.fused)
    cur = no_cur(pair.fused)
    for t, scale in enumerate(SCALES):
        arr = (arrival * np.float32(scale)).astype(np.float32)
        w, cells, state = pair.tick((arr, in_tok, out_tok), cur, f"tick {t}", path=(path,))
        assert state["done_nonzero"] == 0
        cur = feed_back(cur, w)
    hits, misses = pair.fused.memo_stats()
    assert misses > 0 and hits == 2 * misses, "one miss, then two hits per loaded cell"
    return cells, state


def test_wide_next_to_partial_quad(monkeypatch):
    """One wide task and one narrow quad with two empty slots (small tiers)."""
    patch_tiers(monkeypatch)
    pair = Pair(monkeypatch, 1, [LARGE, SMALL, SMALL])
    cells, state = three_ticks(pair, 1)
    wide, narrow = bounds()
    assert state["n_tasks"] == 2
    assert state["lds_first"] < LDS_OPT_IN and state["waves_first"] == narrow
    assert state["waves_second"] == 0


def test_lds_opt_in_takes_wide_budget(monkeypatch):
    """An XL cell raises the launch's LDS above 64 KB: two blocks per CU fit,
    and the launch runs the two-wave instantiation, wide and narrow tasks alike."""
    default_tiers(monkeypatch)
    pair = Pair(monkeypatch, 2, [XL_N, LARGE_N, SMALL_N])
    cells, state = three_ticks(pair, 1)
    wide, narrow = bounds()
    assert state["n_tasks"] == 2 + 2 + 1
    assert state["lds_first"] > LDS_OPT_IN and 2 * state["lds_first"] <= 160 * 1024
    assert state["waves_first"] == wide and wide < narrow
    assert cells["feasible"].any()


def test_no_xl_layout_keeps_four_blocks(monkeypatch):
    """Without an XL cell the LDS lets four blocks onto a CU: that launch
    keeps the four-wave instantiation."""
    default_tiers(monkeypatch)
    pair = Pair(monkeypatch, 2, [LARGE_N, MED_N, SMALL_N, MED_N, MED_N, MED_N])
    cells, state = three_ticks(pair, 1)
    wide, narrow = bounds()
    assert state["n_tasks"] == 1 + 1 + 1
    assert 4 * state["lds_first"] <= 160 * 1024 < 5 * state["lds_first"]
    assert state["waves_first"] == narrow
    assert cells["feasible"].any()


def test_two_launches_two_instantiations(monkeypatch):
    """The residency rule's CU count capped to 1: the XL tasks go to the second
    launch on the two-wave instantiation, the rest stays on the four-wave one,
    and the arrival counters work across the two."""
    default_tiers(monkeypatch)
    monkeypatch.setenv("INFERNO_FUSED_TICK_CUS", "1")
    pair = Pair(monkeypatch, 3, [XL_N, LARGE_N, SMALL_N])
    cells, state = three_ticks(pair, 2)
    wide, narrow = bounds()
    assert state["n_tasks"] == 3 + 3 + 1 and state["n_tasks_second"] == 3
    assert state["lds_second"] > LDS_OPT_IN > state["lds_first"] > 0
    assert state["waves_second"] == wide and state["waves_first"] == narrow
    assert cells["feasible"].any()
