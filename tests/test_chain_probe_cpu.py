"""Oracles of the production chain path (ops.sweep.run_chain_probe), checked on
the CPU; tests/test_chain_probe_gpu.py holds the device to them.

Probe cells: alpha = 8, beta = 0.25, gamma = 4, delta = 2^-6, in_tok = 128,
out_tok = 64. The denominator of s(n) is (2032 + 71 n) / 4 and every fp32
intermediate on the way to it is exact up to n = 32768 (asserted below), so the
rates do not depend on whether a compiler contracts multiply-adds.

Exact oracle: mpmath at 60 digits. w(n) = lam^n / prod_{i<=n} s(i) over the
exact values of the fp32 rates for the head n = 0..N, closed-form geometric sums
of ratio lam / s(N) for the 10 N queue states.

Scheme oracle: what the device algorithm defines mathematically on nt threads,
before any fp64 rounding: chunk = ceil(N / nt); the weight at every
chunk-relative index divisible by 32 (an anchor) is exact; between anchors
w(n) = w(n-1) lam inv32(n) with inv32 = float32(1.0 / float64(s32)); the tail
starts from the exact w(N) with ratio lam / s32(N). With nt >= N every state is
an anchor and the scheme is the exact chain.

Both oracles take `flat`: chain_tail_stats (and the golden's solve) replace the
queue sums by their r = 1 values, Q and Q N + Q (Q + 1) / 2, when
Q |log r| < 1e-6. That is an approximation of the algorithm, not a rounding:
its relative error is up to (Q + 1) |log r| / 2 < 5.1e-7, and it is exact at
lam = s(N). On the grid the rate s(N) (1 - 1e-9) takes it at N <= 65. The
oracles mirror it so that the rounding errors measured against them stay
rounding errors; test_flat_branch_error measures the approximation itself. No
rate the kernels evaluate in production reaches the branch: lam <= lam_max
gives Q |log r| >= 1e-2.

Measured here (relative; wait as |d wait| / resp):
  scheme against exact, whole grid: 8.5e-9 at most (N = 32768 on 256 threads;
      0 where the chunk is one state); the derived bound is 2 * 31 * 2^-24 =
      3.7e-6, see test_scheme_error_bound;
  flat branch against the closed form: 9.7e-8 (N = 65, s(N) (1 - 1e-9));
  CPU golden (StateDependentChain.solve) against the exact oracle: 2.52e-11
      (N = 257 at s(N) (1 - 1e-9), where Q |log r| = 2.6e-6 is just past the
      threshold and the numerator of the arithmetico-geometric sum cancels to
      eps / (Q |log r|)); below 3e-14 up to N = 65. GOLDEN_MAX_ERR is that
      figure.
"""
import math
from fractions import Fraction

import mpmath
import numpy as np
import pytest

from inferno_amd.analyzer import (Configuration, DecodeParms, PrefillParms, QueueAnalyzer,
                                  RequestSize, ServiceParms)
from inferno_amd.analyzer.queue import binary_search, within_tolerance
from tests.test_exact_oracle import exact_chain

mpmath.mp.dps = 60
mpf = mpmath.mpf

PERF = dict(alpha=8.0, beta=0.25, gamma=4.0, delta=2.0 ** -6)
IN_TOK, OUT_TOK = 128, 64
WVA_SUB = 32
WVA_TOL = 1e-6
FLAT_THRESHOLD = 1e-6  # chain_tail_stats: Q |log r| below this takes the flat tail

# (nt, N, gmem): the shapes of the GPU test
CELLS = (
    [(64, n, False) for n in (1, 2, 33,  # chunk 1, every state an anchor
                              64, 65,  # chunk 1 -> 2, trailing lanes empty
                              257,  # chunk 5: one 4-wide step
                              576,  # chunk 9: one 8-wide step
                              832,  # chunk 13: 8 + 4
                              1023,  # chunk 16: 8 + 4 + 3 singles, last lane clipped
                              2048,  # chunk 32: a full sub-chunk
                              2113)]  # chunk 34: a second anchor, lane 63 empty
    + [(128, 2049, False), (256, 2049, False),
       (256, 8193, False),  # chunk 33
       (256, 32768, False),  # the XL LDS ceiling
       (512, 2049, False), (512, 8193, False), (1024, 2049, False), (1024, 8193, False),
       (256, 2049, True), (1024, 2049, True)]
)
FIELDS = ("throughput", "wait", "serv", "in_servers")
SCHEME_BOUND = 2 * 31 * 2.0 ** -24
GOLDEN_MAX_ERR = 2.6e-11  # measured by test_golden_matches_exact (see above)


def cell_id(cell):
    nt, n, gmem = cell
    return f"nt{nt}-N{n}" + ("-gmem" if gmem else "")


_QA = {}


def analyzer(n):
    if n not in _QA:
        cfg = Configuration(n, 10 * n, ServiceParms(PrefillParms(PERF["gamma"], PERF["delta"]),
                                                   DecodeParms(PERF["alpha"], PERF["beta"])))
        _QA[n] = QueueAnalyzer(cfg, RequestSize(IN_TOK, OUT_TOK))
    return _QA[n]


def grid_rates(n):
    """The evaluation rates of a cell (float64, req/msec): lam_min, 0.3 / 0.9 /
    0.99 of s(N), lam_max, s(N) (1 - 1e-9) and s(N) itself (log r = 0)."""
    s = analyzer(n).serv_rate
    s1, sn = float(s[0]), float(s[-1])
    return [s1 * 1e-3, 0.3 * sn, 0.9 * sn, 0.99 * sn, sn * (1.0 - 1e-3), sn * (1.0 - 1e-9), sn]


class Oracle:
    """Both oracles of one batch size. w(n) = c(n) lam^n with c independent of
    lam, so an evaluation is two Horner sums over the N + 1 head states."""

    def __init__(self, n):
        self.N = n
        s32 = analyzer(n).serv_rate
        self.s = [mpf(float(v)) for v in s32]
        self.inv32 = [mpf(float(np.float32(1.0 / np.float64(v)))) for v in s32]
        c = [mpf(1)]
        for v in self.s:
            c.append(c[-1] / v)
        self._exact = c
        self._coef = {}
        self._memo = {}

    def coef(self, chunk):
        """(c, n c) of the scheme with `chunk` states per lane; None: exact."""
        if chunk not in self._coef:
            c = self._exact
            if chunk is not None:
                c = [mpf(1)]
                for i in range(1, self.N + 1):
                    anchor = ((i - 1) % chunk) % WVA_SUB == 0
                    c.append(self._exact[i] if anchor else c[-1] * self.inv32[i - 1])
            self._coef[chunk] = (c, [i * v for i, v in enumerate(c)])
        return self._coef[chunk]

    def solve(self, lam, nt=None, flat=True):
        """throughput, wait, serv, in_servers, resp at rate lam (a float64, taken
        exactly) of the exact chain (nt None) or of the scheme on nt threads."""
        chunk = None if nt is None else -(-self.N // nt)
        if chunk == 1:
            chunk = None  # every state an anchor
        key = (float(lam), chunk, flat)
        if key in self._memo:
            return self._memo[key]
        n, q = self.N, 10 * self.N
        lam = mpf(float(lam))
        c, nc = self.coef(chunk)
        head = head_n = mpf(0)
        for i in range(n, -1, -1):
            head = head * lam + c[i]
            head_n = head_n * lam + nc[i]
        w_n = self._exact[n] * lam ** n
        r = lam / self.s[-1]
        if r == 1 or (flat and q * abs(mpmath.log(r)) < FLAT_THRESHOLD):
            g, jg = mpf(q), mpf(q) * (q + 1) / 2
        else:
            g = r * (1 - r ** q) / (1 - r)
            jg = r * (1 - (q + 1) * r ** q + q * r ** (q + 1)) / (1 - r) ** 2
        z = head + w_n * g
        p_k = w_n * r ** q / z
        tput = lam * (1 - p_k)
        in_servers = head_n / z + (1 - head / z) * n
        resp = (head_n + w_n * (n * g + jg)) / z / tput
        serv = in_servers / tput
        out = dict(throughput=tput, wait=resp - serv, serv=serv, in_servers=in_servers, resp=resp)
        self._memo[key] = out
        return out

    def metric(self, kind, lam, nt):
        """eval_metric of the kernels on the scheme: kind 0 TTFT, 1 ITL (msec),
        with the fp32 casts of prefill_time_f / decode_time_f."""
        o = self.solve(lam, nt)
        tokens = OUT_TOK - 1
        num = o["serv"] - (mpf(PERF["gamma"]) + mpf(PERF["alpha"]) * tokens)
        den = mpf(PERF["delta"]) * IN_TOK + mpf(PERF["beta"]) * tokens
        eff = np.float32(float(min(max(num / den, 0), self.N)))
        if kind == 0:
            prefill = np.float32(PERF["gamma"]) + np.float32(PERF["delta"]) * np.float32(IN_TOK) * eff
            return o["wait"] + mpf(float(prefill))
        return mpf(float(np.float32(PERF["alpha"]) + np.float32(PERF["beta"]) * eff))


_ORACLE = {}


def oracle(n):
    if n not in _ORACLE:
        _ORACLE[n] = Oracle(n)
    return _ORACLE[n]


def rel_errors(got, ref):
    """The four errors of `got` (throughput, wait, serv, in_servers) against an
    oracle record: relative, and the wait on the scale of the response time
    (resp - serv cancels at low load, see tests/test_exact_oracle.py)."""
    out = []
    for f, g in zip(FIELDS, got):
        scale = ref["resp"] if f == "wait" else ref[f]
        out.append(float(abs(mpf(g) - ref[f]) / scale) if math.isfinite(float(g)) else math.inf)
    return out


def bisect_targets(n):
    """(TTFT, ITL) target pairs of a cell, float32 [8, 2], from the golden's
    metrics at interior rates: both bind; only TTFT; only ITL; TTFT ends at
    lam_min (phase 0) while ITL bisects; ITL ends at lam_max (phase 1) while
    TTFT bisects; TTFT below the range; ITL above it; TTFT above and ITL below."""
    qa = analyzer(n)
    lo, hi = qa.rate_min / 1000.0, qa.rate_max / 1000.0
    at = lambda f: lo + f * (hi - lo)  # noqa: E731
    ttft, itl = qa._eval_ttft(at(0.6)), qa._eval_itl(at(0.4))
    rows = [(ttft, itl), (ttft, 0.0), (0.0, itl), (qa._eval_ttft(lo), itl),
            (ttft, qa._eval_itl(hi)), (0.5 * qa._eval_ttft(lo), itl),
            (ttft, 2.0 * qa._eval_itl(hi)), (2.0 * qa._eval_ttft(hi), 0.5 * qa._eval_itl(lo))]
    return np.array(rows, dtype=np.float32)


def golden_search(n, kind, target):
    """The golden's binary_search of one target over [lam_min, lam_max]:
    (x_star, indicator, evaluations, final value)."""
    qa = analyzer(n)
    fn = qa._eval_ttft if kind == 0 else qa._eval_itl
    seen = []

    def counted(x):
        seen.append(fn(x))
        return seen[-1]

    x, ind = binary_search(qa.rate_min / 1000.0, qa.rate_max / 1000.0, float(target), counted)
    return x, ind, len(seen), seen[-1]


def test_rate_denominators_are_exact():
    n = np.arange(1, 32769)
    nf = n.astype(np.float32)
    pre = np.float32(PERF["gamma"]) + np.float32(PERF["delta"]) * np.float32(IN_TOK) * nf
    dec = np.float32(OUT_TOK - 1) * (np.float32(PERF["alpha"]) + np.float32(PERF["beta"]) * nf)
    assert pre.dtype == dec.dtype == np.float32
    assert ((pre + dec).astype(np.float64) == (2032 + 71 * n) / 4.0).all()
    assert (pre.astype(np.float64) == 4 + 2 * n).all() and (dec.astype(np.float64)
                                                            == 63 * (8 + 0.25 * n)).all()
    s = analyzer(32768).serv_rate
    assert (s == (nf / (pre + dec)).astype(np.float32)).all()


@pytest.mark.parametrize("n", (1, 2, 33))
def test_oracles_match_fractions(n):
    orc, s32 = oracle(n), analyzer(n).serv_rate
    serv = [Fraction(float(v)) for v in s32]
    for lam in grid_rates(n):
        want = exact_chain(Fraction(lam), serv, 11 * n)
        ref = {f: mpf(want[k].numerator) / mpf(want[k].denominator)
               for f, k in (("throughput", "throughput"), ("wait", "avg_wait_time"),
                            ("serv", "avg_serv_time"), ("in_servers", "avg_num_in_servers"),
                            ("resp", "avg_resp_time"))}
        for nt in (None, 64):  # nt >= N: the scheme is the exact chain
            got = orc.solve(lam, nt, flat=False)
            assert max(rel_errors([got[f] for f in FIELDS], ref)) < 1e-40, (n, lam, nt)


@pytest.mark.parametrize("cell", CELLS, ids=cell_id)
def test_scheme_error_bound(cell):
    """The algorithmic error of the fp32 reciprocals. A weight between anchors
    is the exact one times at most 31 factors inv32(n) s(n), each within
    (1 +- 2^-24) (1 +- 2^-53) of 1, and the statistics are ratios of sums of
    such weights: 2 * 31 * 2^-24 bounds their relative error."""
    nt, n, _ = cell
    orc = oracle(n)
    worst = 0.0
    for lam in grid_rates(n):
        exact, scheme = orc.solve(lam, None, flat=False), orc.solve(lam, nt, flat=False)
        worst = max(worst, *rel_errors([scheme[f] for f in FIELDS], exact))
    print(f"{cell_id(cell)}: scheme max error {worst:.3e}")
    assert worst <= SCHEME_BOUND


def test_flat_branch_error():
    worst, taken = 0.0, []
    for n in sorted({c[1] for c in CELLS}):
        orc = oracle(n)
        for lam in grid_rates(n):
            r = mpf(lam) / orc.s[-1]
            if r == 1 or 10 * n * abs(mpmath.log(r)) >= FLAT_THRESHOLD:
                continue
            taken.append(n)
            flat, closed = orc.solve(lam, None, flat=True), orc.solve(lam, None, flat=False)
            err = max(rel_errors([flat[f] for f in FIELDS], closed))
            worst = max(worst, err)
            assert err <= (10 * n + 1) * float(abs(mpmath.log(r))) / 2 * (1 + 1e-6), (n, lam)
    print(f"flat branch taken at N = {taken}: max error {worst:.3e}")
    assert taken == [1, 2, 33, 64, 65]  # s(N) (1 - 1e-9) at these; none sits near the threshold


@pytest.mark.parametrize("n", sorted({c[1] for c in CELLS}))
def test_golden_matches_exact(n):
    qa, orc = analyzer(n), oracle(n)
    worst = 0.0
    for lam in grid_rates(n):
        st, ref = qa.chain.solve(lam), orc.solve(lam, None)
        got = (st.throughput, st.avg_wait_time, st.avg_serv_time, st.avg_num_in_servers)
        worst = max(worst, *rel_errors(got, ref))
    print(f"N={n}: golden max error {worst:.3e}")
    assert worst <= GOLDEN_MAX_ERR


@pytest.mark.parametrize("n", sorted({c[1] for c in CELLS}))
def test_bisect_targets_end_within_tolerance(n):
    """No search of the GPU test may leave by the fixed-point or the
    100-iteration exit, and from N = 2 on (at N = 1 the ITL does not depend on
    the rate) each row is of the kind bisect_targets names."""
    tg = bisect_targets(n)
    runs = [[golden_search(n, kind, tg[k, kind]) if tg[k, kind] > 0 else None
             for kind in (0, 1)] for k in range(len(tg))]
    for k, row in enumerate(runs):
        for kind, run in enumerate(row):
            if run is not None and run[1] == 0:
                assert run[2] < 2 + 100
                assert within_tolerance(run[3], float(tg[k, kind]), WVA_TOL), (k, kind, run)
    if n == 1:
        return
    ind = [[None if r is None else r[1] for r in row] for row in runs]
    evals = [[None if r is None else r[2] for r in row] for row in runs]
    assert ind == [[0, 0], [0, None], [None, 0], [0, 0], [0, 0], [-1, 0], [0, 1], [1, -1]]
    assert evals[0][0] > 2 and evals[0][1] > 2  # both bisect
    assert evals[3][0] == 1 and evals[3][1] > 2  # TTFT ends in phase 0
    assert evals[4][1] == 2 and evals[4][0] > 2  # ITL ends in phase 1
