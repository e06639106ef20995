"""Hold analysis on the GPU (FastSweep.hold): a fixed allocation evaluated under
S loads by wva_hold_t / wva_hold_reduce.

The exactness claim: held at the plan's own winners, every loaded slice has the
plan winner's itl, ttft and rho bit for bit (the same evaluation at the same
per-replica rate and block width), is OK, and needs the replicas the plan gave.

Fleet: the 27 cells of tests/test_plan_gpu.py (9 servers x 3 accelerators,
pinned N = 1, 33, 512, 513, 2048, 2049, 8193, 2049, 32769: one state, the
anchor edge, both block widths, the XL tier and the smallest global-memory
cell; an unreachable-SLO server, the TTFT-only N = 1 server, a TPS-target
server, a scale-to-zero server), built here, under that test's load scales.

Observed on MI355X for test_gpu_hold_matches_cpu_hold: 0 needed flips of 63
slices (8 slices moved off the overload bound); for
test_held_at_the_plan_winners_is_the_plan: 0 of 48 slices differ in the bits of
itl, ttft or rho, in both analyzer modes.
"""
import numpy as np
import pytest

from inferno_amd.core import System
from inferno_amd.engine import (
    HOLD_IDLE,
    HOLD_INVALID,
    HOLD_NOT_HELD,
    HOLD_OK,
    HOLD_OVERLOADED,
    HOLD_SLO_VIOLATED,
    FastSweep,
)
from tests.fixtures import make_spec

pytestmark = pytest.mark.gpu

PINNED_N = (1, 33, 512, 513, 2048, 2049, 8193, 2049, 32769)
INFEASIBLE_SRV = 7
TPS_SRV = 2
SCALE_TO_ZERO_SRV = 4
INVALID_SRV = 5  # used by the fixture check only: degenerate perf data on one accelerator
SCALES = (1.0, 0.0, 0.37, 1.7, 2.3, 0.6, 3.1)
ARRIVAL_SCALE = 6000.0
FLOATS = ("itl", "ttft", "rho", "rate", "slo_rate", "cost")
INTS = ("status", "acc_idx", "held_replicas", "needed_replicas")
CELL_KEYS = ("status", "held", "held_replicas", "needed_replicas", "cost", "slo_rate", "itl",
             "ttft", "rho", "rate")


def build_system(analyzer_mode=None, degenerate=False):
    system, _ = System.from_spec(make_spec(n_servers=9, seed=901, arrival_scale=ARRIVAL_SCALE))
    names = sorted(system.servers)
    assert len(names) == len(PINNED_N)
    for i, name in enumerate(names):
        system.servers[name].max_batch_size = PINNED_N[i]
    srv = system.servers[names[INFEASIBLE_SRV]]
    t = system.service_classes[srv.service_class_name].targets[srv.model_name]
    t.itl, t.ttft = 1e-3, 0.0
    srv = system.servers[names[0]]
    system.service_classes[srv.service_class_name].targets[srv.model_name].itl = 0.0
    srv = system.servers[names[TPS_SRV]]
    system.service_classes[srv.service_class_name].targets[srv.model_name].tps = 2000.0
    system.servers[names[SCALE_TO_ZERO_SRV]].min_num_replicas = 0
    if degenerate:
        srv = system.servers[names[INVALID_SRV]]
        perf = system.models[srv.model_name].get_perf_data(sorted(system.accelerators)[0])
        perf.decodeParms.alpha = perf.decodeParms.beta = 0.0
        perf.prefillParms.gamma = perf.prefillParms.delta = 0.0
    if analyzer_mode is not None:
        system.analyzer_mode = analyzer_mode
    return system


def make(backend="gpu", analyzer_mode=None, degenerate=False):
    fs = FastSweep(build_system(analyzer_mode, degenerate), backend=backend)
    assert fs.n_cells == 27
    return fs


def scenarios(fs):
    base = fs._base_load()[0]
    assert (base > 0).all()
    return np.stack([base * np.float32(sc) for sc in SCALES]).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(a, b, rows=None, what=""):
    """Two HoldResults (row subset ``rows`` of a against all of b), bit for bit."""
    pick = (lambda x: x) if rows is None else (lambda x: x[rows])
    for f in INTS + ("counts", "deficit_by_acc"):
        assert np.array_equal(pick(getattr(a, f)), getattr(b, f)), f"{what}: {f}"
    for f in FLOATS:
        assert np.array_equal(bits(pick(getattr(a, f))), bits(getattr(b, f))), f"{what}: {f}"
    if a.cells is not None and b.cells is not None:
        for k in CELL_KEYS:
            x, y = pick(a.cells[k]), b.cells[k]
            if x.dtype == np.float32:
                x, y = bits(x), bits(y)
            assert np.array_equal(x, y), f"{what}: cell {k}"


_PLAN = {}


def plan_and_hold(analyzer_mode=None):
    """(planner, scenarios, plan at them, hold at the plan's winners), computed
    once per analyzer mode and left unchanged."""
    if analyzer_mode not in _PLAN:
        fs = make(analyzer_mode=analyzer_mode)
        scen = scenarios(fs)
        p = fs.plan(arrival=scen)
        h = fs.hold(arrival=scen, allocation=(p.winners.acc_idx, p.winners.num_replicas),
                    return_cells=True)
        _PLAN[analyzer_mode] = (fs, scen, p, h)
    return _PLAN[analyzer_mode]


def one_short():
    """The plan's winners with one replica less than needed wherever >= 2 are."""
    _, scen, p, h = plan_and_hold()
    short = (h.status == HOLD_OK) & (h.needed_replicas >= 2)
    rep = np.where(short, h.needed_replicas - 1, p.winners.num_replicas).astype(np.int32)
    return scen, p.winners.acc_idx, rep, short


def n_active_cells(scen, acc):
    """Cells that some scenario both holds and loads: the memo lookups of a call."""
    s, i = np.nonzero((acc >= 0) & (scen != 0))
    n = len(set(zip(i.tolist(), acc[s, i].tolist())))
    assert n >= 8  # every server but the unreachable-SLO one
    return n


def test_fixture_covers_what_it_claims():
    fs, scen, p, h = plan_and_hold()
    _, acc, rep, short = one_short()
    assert short.any()
    assert (rep[0] != rep[4]).any()  # an [S, n_srv] allocation that differs between scenarios
    # every status: the plan-held pass has OK, NOT_HELD (unreachable SLO: no winner) and IDLE
    seen = set(np.unique(h.status))
    assert {HOLD_OK, HOLD_NOT_HELD, HOLD_IDLE} <= seen
    d = make(degenerate=True)
    acc2 = np.where(acc >= 0, acc, 0).astype(np.int32)  # the unreachable-SLO server held too
    acc2[:, INVALID_SRV] = 0
    rep2 = np.where(acc >= 0, rep, 1 << 20).astype(np.int32)
    rep2[3, 0] = 0  # an accelerator without replicas
    r = d.hold(arrival=scen, allocation=(acc2, rep2), return_cells=True)
    seen |= set(np.unique(r.status))
    assert seen == {HOLD_OK, HOLD_SLO_VIOLATED, HOLD_OVERLOADED, HOLD_NOT_HELD, HOLD_IDLE,
                    HOLD_INVALID}
    assert (r.status[0::2, INVALID_SRV] == HOLD_INVALID).all()
    assert r.status[3, 0] == HOLD_OVERLOADED and r.rate[3, 0] == 0 and np.isinf(r.itl[3, 0])
    assert r.status[0, INFEASIBLE_SRV] == HOLD_SLO_VIOLATED
    assert r.needed_replicas[0, INFEASIBLE_SRV] == -1 and np.isfinite(r.ttft[0, INFEASIBLE_SRV])
    assert (r.status[1] == HOLD_IDLE).all()
    # held cells in every tier and at both widths
    held_n = np.asarray(PINNED_N)[(r.status[0] != HOLD_NOT_HELD) & (r.status[0] != HOLD_INVALID)]
    for lo, hi in ((1, 512), (513, 2048), (2049, 8192), (8193, 32768), (32769, 1 << 22)):
        assert ((held_n >= lo) & (held_n <= hi)).any(), (lo, hi)
    # the cells agree with the server records
    c = r.cells
    assert c["status"].shape == (len(SCALES), 27) and "cell_server" in c
    assert np.array_equal((c["held"] != 0).sum(axis=1), (r.status != HOLD_NOT_HELD).sum(axis=1))
    for s in range(len(SCALES)):
        for k in np.nonzero(c["held"][s])[0]:
            i = c["cell_server"][k]
            assert c["status"][s, k] == r.status[s, i] and c["cell_acc_idx"][k] == r.acc_idx[s, i]
            assert c["needed_replicas"][s, k] == r.needed_replicas[s, i]


@pytest.mark.parametrize("mode", [None, "mg1"])
def test_held_at_the_plan_winners_is_the_plan(mode):
    """Pinned to the plan: raw bits of itl, ttft, rho; OK; needed == planned."""
    fs, scen, p, h = plan_and_hold(mode)
    w = p.winners
    loaded = (w.acc_idx >= 0) & (scen != 0)
    assert loaded.sum() >= 40
    min_rep = np.array([s.min_num_replicas for s in fs._srv_objs])[None, :]
    for f in ("itl", "ttft", "rho"):
        got, want = bits(getattr(h, f)), bits(getattr(w, f))
        print(f"{f}: {(got != want)[loaded].sum()} of {loaded.sum()} slices differ in bits")
        assert np.array_equal(got[loaded], want[loaded]), f
    assert (h.status[loaded] == HOLD_OK).all()
    assert np.array_equal(np.maximum(h.needed_replicas, min_rep)[loaded], w.num_replicas[loaded])
    assert np.array_equal(h.acc_idx[loaded], w.acc_idx[loaded])
    assert np.array_equal(h.held_replicas[loaded], w.num_replicas[loaded])
    assert np.array_equal(bits(h.cost[loaded]), bits(w.cost[loaded]))


def test_one_replica_short():
    fs, _, _, _ = plan_and_hold()
    scen, acc, rep, short = one_short()
    r = fs.hold(arrival=scen, allocation=(acc, rep))
    assert np.isin(r.status[short], (HOLD_SLO_VIOLATED, HOLD_OVERLOADED)).all()
    want = np.zeros_like(r.deficit_by_acc)
    on = (r.status != HOLD_NOT_HELD) & (r.needed_replicas >= 0)
    for s in range(scen.shape[0]):
        np.add.at(want[s], r.acc_idx[s][on[s]],
                  np.maximum(r.needed_replicas[s][on[s]].astype(np.int64)
                             - r.held_replicas[s][on[s]], 0))
    assert np.array_equal(r.deficit_by_acc, want)
    assert want.sum() == short.sum() > 0
    for s in range(scen.shape[0]):
        assert np.array_equal(r.counts[s], np.bincount(r.status[s], minlength=6))
    assert r.counts.dtype == np.int64 and (r.counts.sum(axis=1) == 9).all()


_RATE_MAX = {}


def golden_rate_max(cpu, i, a):
    """rate_max (req/s) of server i's cell on accelerator a, from the CPU
    golden's analyzer, built as _hold_cpu builds it."""
    if (i, a) not in _RATE_MAX:
        _RATE_MAX[i, a] = _golden_rate_max(cpu, i, a)
    return _RATE_MAX[i, a]


def _golden_rate_max(cpu, i, a):
    from inferno_amd.analyzer import (Configuration, DecodeParms, PrefillParms, QueueAnalyzer,
                                      RequestSize, ServiceParms)
    srv = cpu._srv_objs[i]
    perf = cpu.system.models[srv.model_name].get_perf_data(cpu.acc_names[a])
    n = srv.max_batch_size
    cfg = Configuration(max_batch_size=n, max_queue_size=10 * n, service_parms=ServiceParms(
        prefill=PrefillParms(gamma=perf.prefillParms.gamma, delta=perf.prefillParms.delta),
        decode=DecodeParms(alpha=perf.decodeParms.alpha, beta=perf.decodeParms.beta)))
    _, in_tok, out_tok = cpu._base_load()
    return QueueAnalyzer(cfg, RequestSize(int(in_tok[i]), int(out_tok[i]))).rate_max


def test_overload():
    """1.5x above rate_max * R * 60 is OVERLOADED with +inf latencies, 0.5x of
    it is evaluated: no case within 1 % of the bound."""
    fs, _, p, _ = plan_and_hold()
    cpu = make("cpu")
    servers = [i for i in range(9) if i not in (TPS_SRV, INFEASIBLE_SRV)]
    acc = np.full(9, -1, dtype=np.int32)
    rep = np.zeros(9, dtype=np.int32)
    bound = np.zeros(9)
    for i in servers:
        acc[i] = p.winners.acc_idx[0, i]
        rep[i] = 1 + i % 3
        bound[i] = golden_rate_max(cpu, i, int(acc[i])) * rep[i] * 60.0
    scen = np.stack([bound * 1.5, bound * 0.5]).astype(np.float32)
    r = fs.hold(arrival=scen, allocation=(acc, rep))
    assert (r.status[0, servers] == HOLD_OVERLOADED).all()
    assert np.isinf(r.itl[0, servers]).all() and np.isinf(r.ttft[0, servers]).all()
    assert (r.rho[0, servers] == 1).all() and (r.needed_replicas[0, servers] > rep[servers]).all()
    assert np.isin(r.status[1, servers], (HOLD_OK, HOLD_SLO_VIOLATED)).all()
    assert np.isfinite(r.itl[1, servers]).all() and np.isfinite(r.ttft[1, servers]).all()
    assert np.allclose(r.rate[0, servers], bound[servers] * 1.5 / 60.0 / rep[servers], rtol=1e-6)


def test_slice_independence_memo_and_reconcile(monkeypatch):
    monkeypatch.delenv("INFERNO_SIZING_MEMO", raising=False)
    scen, acc, rep, _ = one_short()
    fs = make()
    assert fs.memo_stats() is None
    cold = fs.hold(arrival=scen, allocation=(acc, rep), return_cells=True)
    active = n_active_cells(scen, acc)
    assert fs.memo_stats() == (0, active)  # once per held-and-loaded cell, not per scenario
    warm = fs.hold(arrival=scen, allocation=(acc, rep), return_cells=True)
    assert fs.memo_stats() == (active, active)
    assert_same(cold, warm, what="cold against warm")
    for s in range(scen.shape[0]):
        one = make()
        a = one.hold(arrival=scen[s:s + 1], allocation=(acc[s], rep[s]), return_cells=True)
        assert_same(cold, a, rows=slice(s, s + 1), what=f"slice {s}, cold")
        b = one.hold(arrival=scen[s:s + 1], allocation=(acc[s:s + 1], rep[s:s + 1]),
                     return_cells=True)
        assert_same(cold, b, rows=slice(s, s + 1), what=f"slice {s}, warm")
    monkeypatch.setenv("INFERNO_SIZING_MEMO", "0")
    off = make()
    res = off.hold(arrival=scen, allocation=(acc, rep), return_cells=True)
    assert off.memo_stats() is None
    assert_same(cold, res, what="memo off")


def test_reconcile_hold_reconcile(monkeypatch):
    """A hold between two reconciles changes neither; each warms the other's
    memo; the fused tick's state and the stale-tick count do not move."""
    monkeypatch.delenv("INFERNO_SIZING_MEMO", raising=False)
    scen, acc, rep, _ = one_short()
    active = n_active_cells(scen, acc)

    def run(with_hold):
        fs = make()
        w1 = fs.reconcile()
        if with_hold:
            g = fs._gpu
            stats, fused, stale, key = fs.memo_stats(), g.fused_state(), g.stale_ticks, g.bucket_key
            fs.hold(arrival=scen, allocation=(acc, rep))
            after = fs.memo_stats()
            # the reconcile sized them
            assert (after[0] - stats[0], after[1] - stats[1]) == (active, 0)
            assert g.fused_state() == fused and g.stale_ticks == stale and g.bucket_key == key
        w2 = fs.reconcile()
        return w1, w2

    (w1, w2), (t1, t2) = run(True), run(False)
    for f in ("acc_idx", "num_replicas", "batch"):
        assert np.array_equal(getattr(w1, f), getattr(t1, f)), f
        assert np.array_equal(getattr(w2, f), getattr(t2, f)), f
    for f in ("cost", "value", "itl", "ttft", "rho", "max_rate"):
        assert np.array_equal(bits(getattr(w1, f)), bits(getattr(t1, f))), f
        assert np.array_equal(bits(getattr(w2, f)), bits(getattr(t2, f))), f
    # hold first: the reconcile after it hits the memo for the cells hold sized
    fs = make()
    fs.hold(arrival=scen, allocation=(acc, rep))
    assert fs.memo_stats() == (0, active)
    w = fs.reconcile()
    assert fs.memo_stats() == (active, 27)  # 27 loaded cells, `active` of them sized by hold
    for f in ("acc_idx", "num_replicas"):
        assert np.array_equal(getattr(w, f), getattr(t1, f)), f
    for f in ("cost", "value", "itl", "ttft", "rho", "max_rate"):
        assert np.array_equal(bits(getattr(w, f)), bits(getattr(t1, f))), f


def test_validation_launches_nothing():
    fs, scen, p, _ = plan_and_hold()
    stats = fs.memo_stats()
    acc, rep = p.winners.acc_idx, p.winners.num_replicas
    for kw in (dict(scales=[1.0] * 257), dict(scales=[1.0, -1.0]),
               dict(arrival=scen, allocation=(acc[:3], rep[:3])),
               dict(arrival=scen, allocation=(acc + 3, rep)),
               dict(arrival=scen, allocation=(np.abs(acc), -np.abs(rep) - 1)),
               dict(arrival=scen, allocation=(acc + 0.5, rep))):
        with pytest.raises(ValueError):
            fs.hold(**kw)
    assert fs.memo_stats() == stats


def test_gpu_hold_matches_cpu_hold():
    """GPU against the CPU golden: statuses and needed_replicas equal except
    for at most max(1, n // 50) slices where needed differs by one (a ceil
    boundary inside the bisection tolerance), which may flip the status between
    OK and SLO_VIOLATED only; itl rel 1e-3, ttft rel 2e-3, rho rel 1e-3, as
    tests/test_plan_slo_gpu.py::test_gpu_plan_slo_matches_cpu_plan_slo.

    The allocation is the one-short one, moved off the overload bound: where
    the golden's own rate_max puts a slice's per-replica rate within 5 % of it,
    the slice holds the first of needed, needed + 1, needed + 2 replicas that
    does not. Checked below on the golden's inputs (1 %)."""
    scen, acc, rep, _ = one_short()
    _, _, _, h = plan_and_hold()
    cpu = make("cpu")
    rep = rep.copy()
    moved = 0
    for s, i in zip(*np.nonzero((acc >= 0) & (scen != 0))):
        rmax = golden_rate_max(cpu, int(i), int(acc[s, i]))
        total = 2000.0 / cpu._base_load()[2][i] if i == TPS_SRV else float(scen[s, i]) / 60.0
        for r in (rep[s, i],) + tuple(int(h.needed_replicas[s, i]) + d for d in (0, 1, 2)):
            if abs(total / r / rmax - 1.0) > 0.05:
                moved += r != rep[s, i]
                rep[s, i] = r
                break
    print(f"slices moved off the overload bound: {moved}")
    c = cpu.hold(arrival=scen, allocation=(acc, rep))
    assert {HOLD_OK, HOLD_SLO_VIOLATED, HOLD_OVERLOADED} <= set(np.unique(c.status))
    g = make().hold(arrival=scen, allocation=(acc, rep))
    # no golden input within 1 % of the analyzer's rate bound
    for s, i in zip(*np.nonzero((c.status != HOLD_NOT_HELD) & (c.status != HOLD_IDLE))):
        rmax = golden_rate_max(cpu, int(i), int(acc[s, i]))
        assert abs(float(c.rate[s, i]) / rmax - 1.0) > 0.01, (s, i)
    n = c.status.size
    flips = 0
    assert np.array_equal(g.acc_idx, c.acc_idx) and np.array_equal(g.held_replicas,
                                                                   c.held_replicas)
    for s in range(c.status.shape[0]):
        for i in range(c.status.shape[1]):
            where = f"scenario {s} server {i}"
            if c.needed_replicas[s, i] != g.needed_replicas[s, i]:
                flips += 1
                assert abs(int(c.needed_replicas[s, i]) - int(g.needed_replicas[s, i])) == 1, where
                if c.status[s, i] != g.status[s, i]:
                    assert {int(c.status[s, i]), int(g.status[s, i])} == {HOLD_OK,
                                                                         HOLD_SLO_VIOLATED}, where
            else:
                assert c.status[s, i] == g.status[s, i], where
            assert c.cost[s, i] == pytest.approx(g.cost[s, i], rel=1e-5, abs=1e-4), where
            assert c.itl[s, i] == pytest.approx(g.itl[s, i], rel=1e-3, abs=1e-4), where
            assert c.ttft[s, i] == pytest.approx(g.ttft[s, i], rel=2e-3, abs=1e-3), where
            assert c.rho[s, i] == pytest.approx(g.rho[s, i], rel=1e-3, abs=1e-5), where
            assert c.rate[s, i] == pytest.approx(g.rate[s, i], rel=1e-5), where
            assert c.slo_rate[s, i] == pytest.approx(g.slo_rate[s, i], rel=1e-4), where
    print(f"needed flips: {flips} of {n}")
    assert flips <= max(1, n // 50)


def test_global_memory_tier_and_arena_growth():
    """S = 1, then S = 7, on one context; the N = 32769 cell is held in both."""
    _, scen, p, ref = plan_and_hold()
    acc, rep = p.winners.acc_idx, p.winners.num_replicas
    assert acc[0, 8] >= 0 and PINNED_N[8] > 32768
    fs = make()
    one = fs.hold(arrival=scen[:1], allocation=(acc[0], rep[0]), return_cells=True)
    assert_same(ref, one, rows=slice(0, 1), what="S = 1")
    assert one.status[0, 8] == HOLD_OK
    full = fs.hold(arrival=scen, allocation=(acc, rep), return_cells=True)
    assert_same(ref, full, what="S = 7")
