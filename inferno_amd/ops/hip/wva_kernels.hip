// wva_kernels.hip — MI355X (gfx950/CDNA4) allocate-sweep + solver kernels.
//
// Replaces the scalar Go hot path of the reference autoscaler
// (pkg/core/allocation.go:27-163 CreateAllocation, pkg/analyzer/
// queueanalyzer.go:99-255 BuildModel/Analyze/Size, pkg/analyzer/
// mm1modelstatedependent.go:70-116 computeProbabilities and
// pkg/solver/solver.go:63-79 SolveUnlimited) with batched device kernels:
//
//   K1 wva_sweep_t<NT>: one block per (server, accelerator[, TP]) cell,
//       templated on block size (64/256/512/1024 instantiated). The host
//       dispatches cells to 64- and 256-thread blocks by batch size N
//       (ops/sweep.py choose_buckets) — widths picked by A/B measurement:
//       per-evaluation cost is dominated by the redundant per-lane
//       transcendental tail, which costs waves-per-SIMD x instructions, so
//       NARROW blocks win (16-wave blocks pay 4x what 4-wave blocks pay).
//       The buckets launch on separate HIP streams so they overlap.
//
//       Per cell (state-dependent M/M/1/K mode, the reference's evaluator):
//       fp32 service rates s(n) (matching the reference's float32 inputs),
//       then a chunked scan builds the chain geometry in LDS — a chunk-
//       TRANSPOSED fp32 1/s(n) table plus the fp64 log-prefix at every
//       32-state anchor. Each chain evaluation is O(N/NT) per lane: within a
//       32-state sub-chunk probabilities advance by the linear-space
//       recurrence w(n+1) = w(n)*lam/s(n+1) (ONE fp64 exp per anchor instead
//       of per state), the 10N saturated queue states fold into an analytic
//       geometric tail (vs the reference's O(11N) sequential recurrence with
//       overflow rescaling), and reductions are __shfl_xor butterflies
//       (hierarchical shfl+LDS above one wave; a 64-thread block runs
//       entirely barrier-free). The TTFT and ITL SLO bisections
//       (pkg/analyzer/utils.go:26-70 semantics: 1e-6 relative tolerance,
//       <=100 iterations, below/within/above indicators) run CONCURRENTLY in
//       the two half-blocks in lock-step (dual_bisect), halving the sizing
//       phase's sequential depth.
//
//       analyzer_mode 1 selects the closed-form M/G/1/K evaluator
//       (mg1_eval: O(1) per evaluation, no chain/LDS — BASELINE config 4).
//
//       Under the native reconcile context the sizing result of each cell
//       is memoized across ticks, keyed on the bits of everything the sizing
//       reads and validated on the device (see "Sizing memo" below): a hit
//       keeps the geometry build and ONE chain evaluation.
//
//   K2 wva_argmin: segmented argmin over the sweep output per server
//       (value = transition-penalty-adjusted cost), deterministic
//       lowest-cell-index tie-break (the one-shot API; the context uses K4b).
//
//   K1 also comes as wva_plan_t<NT>: the same sweep over S arrival-rate
//       scenarios per cell (planning), and as wva_slo_plan_t<NT>: T SLO-target
//       sets times S arrival-rate scenarios per cell (SLO planning).
//
//       And as wva_tok_plan_t<NT>: W sets of token averages times S scenarios
//       (token-mix planning), one block per (set, cell) at the width the cell
//       has under that set.
//
//       And as wva_hold_t<NT>: a FIXED allocation under S scenarios (hold
//       analysis): the replicas are pinned per (cell, scenario), the slice is a
//       verdict with the latencies; K4d wva_hold_reduce picks each server's
//       held cell and sums the verdicts and the replica deficits.
//
//   K4 wva_plan_reduce: per (server, scenario) K2's selection, the winner
//       record and the per-accelerator replica totals, in one launch.
//
//   K4b wva_winner: the reconcile tick's winner step, K4 on one scenario
//       without the totals.
//
//   K5 wva_plan_greedy: the capacity-limited solution of every scenario, one
//       wave per scenario.
//
//   K6 wva_tick_t: the reconcile tick in ONE launch. K1's cell function per
//       cell of a task table (one 256-thread cell or four one-wave cells per
//       block) and K4b's winner step by whichever cell of a server arrives
//       last (agent-scope release / acquire around a per-server counter;
//       nobody waits). The context uses it whenever every bucket is 64 or 256
//       threads wide with its geometry in LDS; K1 + K4b remain for the rest.
//
//   (K3 is unused: the numbers are kept stable for the documents that cite
//   them.)
//
// Built standalone with hipcc (no torch headers); exposed as a C ABI and
// driven from Python via ctypes on torch tensors' device pointers
// (ops/sweep.py one-shot API; engine/native_ctx.py persistent-state hot path,
// whose host side is wva_ctx.inc, included at the end of this file).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <type_traits>

#include "../native/wva_stage.h"  // dynamic-block rows, tick code, host staging ABI

#define WVA_WAVE 64
// max LDS-resident batch size per cell (bounds the LDS chain geometry:
// chunk*NT fp32 reciprocals + NT*ksub fp64 anchors + a 40-double header).
// Cells with N above this spill their chain geometry to a per-block global
// memory slab (GMEM=true instantiation) — the reference's N is uncapped
// (allocation.go:80-86), so no batch size may change the computed allocation.
#define WVA_MAX_N 8192
// XL LDS bucket: 8192 < N <= 32768 still fits the chain geometry in CDNA4's
// 160 KiB LDS (136.6 KiB at NT=256, N=32768) with the >64 KiB dynamic-LDS
// opt-in (hipFuncSetAttribute); beyond that the geometry spills to global
// memory (GMEM instantiation)
#define WVA_XL_MAX_N 32768
// sanity guard for the global-memory spill path (absurd profiles fail loudly
// instead of exhausting HBM: 4M states/cell = ~16 MB geometry per cell)
#define WVA_HUGE_MAX_N (1 << 22)
// N-bucket thresholds (host mirrors these in ops/sweep.py)
#define WVA_N_SMALL 512
#define WVA_N_MED 2048

// bisection constants (ref pkg/analyzer/utils.go:8-9)
#define WVA_TOL 1e-6
#define WVA_MAX_ITERS 100
// ref queueanalyzer.go:8-11
#define WVA_EPSILON 1e-3
#define WVA_STABILITY_FRACTION 0.1
// ref pkg/config/defaults.go:22
#define WVA_ACCEL_PENALTY 0.1f

// ---------------------------------------------------------------------------
// input/output SoA (all device pointers, one entry per cell unless noted)
// ---------------------------------------------------------------------------
struct WvaCellsIn {
  const int *in_tok;
  const int *out_tok;
  const int *batch_n;
  const int *min_replicas;
  const int *perf_max_batch;
  const int *cur_replicas;
  const int *flags;  // bit0: cur acc == this acc; bit1: cur acc empty; bit2: has cur
  const float *alpha;
  const float *beta;
  const float *gamma;
  const float *delta;
  const float *arrival_rate;  // req/min
  const float *t_itl;
  const float *t_ttft;
  const float *t_tps;
  const float *acc_cost;  // accelerator cost * numInstances (per replica)
  const float *cur_cost;
};

struct WvaCellsOut {
  uint8_t *feasible;
  uint8_t *zero_empty;
  int *num_replicas;
  int *batch;
  float *cost;
  float *value;
  float *itl;
  float *ttft;
  float *rho;
  float *max_rate;  // req/msec per replica
};

// ---------------------------------------------------------------------------
// reductions templated on block size and PART (1 = whole block, 2 = the two
// half-blocks reduce independently — used by the concurrent dual bisection).
// scratch is LDS (>= 32 doubles); parts use disjoint scratch regions, and the
// __syncthreads calls are executed uniformly by the whole block (both parts
// run their evaluations in lock-step).
//
// A one-wave cell (NT == 64) takes only the shuffle branches below: no
// barrier, no scratch, no threadIdx.x. The fused tick kernel depends on that:
// the four waves of its narrow blocks run four independent cells and leave at
// different times. The multi-wave branches index by threadIdx.x, which is the
// cell's thread index there because a multi-wave cell always owns its block.
// ---------------------------------------------------------------------------
// true when a part of NT / PART threads reduces by shuffles alone
template <int NT, int PART>
constexpr bool wva_red_barrier_free() {
  return NT / PART <= WVA_WAVE;
}
static_assert(wva_red_barrier_free<WVA_WAVE, 1>() && wva_red_barrier_free<WVA_WAVE, 2>(),
              "one-wave cells must reduce without a barrier (fused tick, narrow blocks)");
template <int NT, int PART>
__device__ __forceinline__ double red_max_p(double v, double *scratch) {
  constexpr int W = NT / PART;  // threads per part
  if constexpr (W < WVA_WAVE) {
    // sub-wave part (NT=64, PART=2): 32-lane butterfly, barrier-free
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, W));
    return v;
  } else {
#pragma unroll
    for (int off = WVA_WAVE / 2; off > 0; off >>= 1)
      v = fmax(v, __shfl_xor(v, off, WVA_WAVE));
    constexpr int NWH = W / WVA_WAVE;  // waves per part
    if constexpr (NWH == 1) {
      return v;
    } else {
      const int tid = threadIdx.x;
      const int part = tid / W;
      const int widx = (tid % W) / WVA_WAVE;
      __syncthreads();  // protect scratch from previous use
      if ((tid & (WVA_WAVE - 1)) == 0) scratch[part * NWH + widx] = v;
      __syncthreads();
      double m = scratch[part * NWH];
#pragma unroll
      for (int i = 1; i < NWH; ++i) m = fmax(m, scratch[part * NWH + i]);
      return m;
    }
  }
}

template <int NT, int PART>
__device__ __forceinline__ void red_sum2_p(double &a, double &b, double *scratch) {
  constexpr int W = NT / PART;
  if constexpr (W < WVA_WAVE) {
#pragma unroll
    for (int off = W / 2; off > 0; off >>= 1) {
      a += __shfl_xor(a, off, W);
      b += __shfl_xor(b, off, W);
    }
  } else {
#pragma unroll
    for (int off = WVA_WAVE / 2; off > 0; off >>= 1) {
      a += __shfl_xor(a, off, WVA_WAVE);
      b += __shfl_xor(b, off, WVA_WAVE);
    }
    constexpr int NWH = W / WVA_WAVE;
    if constexpr (NWH > 1) {
      const int tid = threadIdx.x;
      const int part = tid / W;
      const int widx = (tid % W) / WVA_WAVE;
      __syncthreads();
      if ((tid & (WVA_WAVE - 1)) == 0) {
        scratch[part * 2 * NWH + 2 * widx] = a;
        scratch[part * 2 * NWH + 2 * widx + 1] = b;
      }
      __syncthreads();
      double sa = 0.0, sb = 0.0;
#pragma unroll
      for (int i = 0; i < NWH; ++i) {
        sa += scratch[part * 2 * NWH + 2 * i];
        sb += scratch[part * 2 * NWH + 2 * i + 1];
      }
      a = sa;
      b = sb;
    }
  }
}

// ---------------------------------------------------------------------------
// queueing primitives (fp32 where the reference uses float32)
// ---------------------------------------------------------------------------
__device__ __forceinline__ float prefill_time_f(float gamma, float delta, int in_tok, float b) {
  if (in_tok == 0) return 0.0f;
  return gamma + delta * (float)in_tok * b;
}
__device__ __forceinline__ float decode_time_f(float alpha, float beta, float b) {
  return alpha + beta * b;
}

// ref queueanalyzer.go:288-302
__device__ __forceinline__ double effective_concurrency(double serv_time, float gamma,
                                                        float alpha, float delta, float beta,
                                                        int in_tok, int out_tok, int N) {
  double tokens = (double)(out_tok - 1);
  double num = serv_time - ((double)gamma + (double)alpha * tokens);
  double den = (double)delta * (double)in_tok + (double)beta * tokens;
  double n;
  if (den == 0.0)
    n = (num > 0.0) ? (double)N : 0.0;
  else
    n = num / den;
  return fmin(fmax(n, 0.0), (double)N);
}

struct ChainOut {
  double throughput;  // req/msec
  double wait;        // msec
  double serv;        // msec
  double in_servers;
};

// Chain geometry shared by the setup scan and every evaluation.
// Each lane owns a CONTIGUOUS chunk of states n in [n0, n1]; within the
// chunk, probabilities advance by the linear-space recurrence
// w(n+1) = w(n) * lam / s(n+1) — one fp64 exp per SUB-state anchor instead
// of one per state (the exp is the dominant per-state cost; a 32-state
// sub-chunk product spans at most e^224 relative to its anchor, far inside
// fp64 range, and anchors are pinned <= exp(0) by the anchor max).
// LDS layout: inv_s_t is chunk-TRANSPOSED ([j*NT + lane] holds 1/s(n0+j))
// so the per-step reads are conflict-free; S_anchor holds the log-prefix at
// the anchor states only.
#define WVA_SUB 32

struct ChainGeom {
  const float *inv_s_t;    // [chunk*NT] transposed reciprocal service rates
                           // (fp32: the rates themselves are fp32 per the
                           // reference; one extra rounding per factor is
                           // reset at every 32-state anchor, keeping the
                           // sub-chunk product within ~1e-6 relative — and
                           // it halves the LDS footprint, doubling the
                           // blocks/CU for large-N cells)
  const double *S_anchor;  // [NT*ksub] log-prefix at anchors
  double S_total;          // S[N]
  int chunk;               // states per lane = ceil(N/NT)
  int ksub;                // anchors per lane = ceil(chunk/SUB)
};

// Geometric tail (n = N+1..K, ratio r = lam/s(N)) + final chain statistics
// from the reduced head sums. Pure scalar fp64; factored out so chain_eval
// can run it on one wave per part and broadcast (see epilogue there).
__device__ __forceinline__ ChainOut chain_tail_stats(double lam, double loglam, double logsN,
                                                     double S_total, int N, int K, double m,
                                                     double head_sum, double head_n_sum) {
  const double log_r = loglam - logsN;
  const double r = exp(log_r);
  const double wN = exp((double)N * loglam - S_total - m);
  const int Q = K - N;
  double tail_sum = 0.0, tail_n_sum = 0.0, wK = (Q == 0) ? wN : 0.0;
  if (Q > 0 && wN > 0.0) {
    const double rQ = exp((double)Q * log_r);
    if ((double)Q * fabs(log_r) < 1e-6) {
      // r ~ 1: flat tail; the closed forms cancel catastrophically here
      tail_sum = wN * (double)Q;
      tail_n_sum = wN * ((double)Q * (double)N + (double)Q * (double)(Q + 1) * 0.5);
      wK = wN * rQ;
    } else {
      // expm1-stable: 1-r, 1-r^Q without cancellation; arithmetico-geometric
      // numerator rewritten as (1-r^Q) - Q r^Q (1-r)
      const double omr = -expm1(log_r);
      const double omrQ = -expm1((double)Q * log_r);
      const double gg = r * omrQ / omr;
      const double jg = r * (omrQ - (double)Q * rQ * omr) / (omr * omr);
      tail_sum = wN * gg;
      tail_n_sum = wN * ((double)N * gg + jg);
      wK = wN * rQ;
    }
  }
  const double Z = head_sum + tail_sum;
  const double pK = wK / Z;
  const double avg_n_sys = (head_n_sum + tail_n_sum) / Z;
  const double avg_n_serv = head_n_sum / Z + (1.0 - head_sum / Z) * (double)N;

  ChainOut o;
  o.throughput = lam * (1.0 - pK);
  o.in_servers = avg_n_serv;
  const double resp = avg_n_sys / o.throughput;
  o.serv = avg_n_serv / o.throughput;
  o.wait = fmax(resp - o.serv, 0.0);
  return o;
}

// Solve the state-dependent chain at arrival rate lam. With PART=1 the whole
// block cooperates and every thread returns identical results; with PART=2
// each half-block independently evaluates its own lam (each half covers all
// N states by walking two lane-chunks), enabling the concurrent TTFT/ITL
// bisections.
template <int NT, int PART>
__device__ ChainOut chain_eval(double lam, const ChainGeom &g, double logsN, int N, int K,
                               double *scratch) {
  constexpr int W = NT / PART;
  // the thread's index within its part. W divides 64 for a one-wave cell, so
  // threadIdx.x % W is also right when such a cell is one wave of a wider
  // block (its cell-relative index is threadIdx.x & 63)
  static_assert(NT > WVA_WAVE || WVA_WAVE % W == 0, "one-wave cell: W must divide the wave");
  const int lane = threadIdx.x % W;
  const double loglam = log(lam);

  // pass 1: max over anchor states (plus the n=0 state's t=0)
  double tmax = 0.0;
  for (int c = lane; c < NT; c += W) {
    const int n0c = c * g.chunk + 1;
    const int n1c = min(n0c + g.chunk - 1, N);
    for (int k = 0; k < g.ksub; ++k) {
      int na = n0c + k * WVA_SUB;
      if (na > n1c) break;
      tmax = fmax(tmax, (double)na * loglam - g.S_anchor[c * g.ksub + k]);
    }
  }
  const double m = red_max_p<NT, PART>(tmax, scratch);

  // pass 2: head sums via per-sub-chunk running products
  double head_sum = (lane == 0) ? exp(-m) : 0.0;  // n = 0 state
  double head_n_sum = 0.0;
  for (int c = lane; c < NT; c += W) {
    const int n0c = c * g.chunk + 1;
    const int n1c = min(n0c + g.chunk - 1, N);
    for (int k = 0; k < g.ksub; ++k) {
      const int j0 = k * WVA_SUB;
      const int na = n0c + j0;
      if (na > n1c) break;
      double w = exp((double)na * loglam - g.S_anchor[c * g.ksub + k] - m);
      head_sum += w;
      head_n_sum += (double)na * w;
      const int jend = min(j0 + WVA_SUB - 1, n1c - n0c);
      // batch the LDS reads 4-wide ahead of the dependent w-chain: with the
      // narrow-block dispatch there is often only one wave per SIMD, so an
      // un-batched loop exposes the full LDS latency on every step (PMC:
      // SQ_WAIT_ANY was 50% of wave cycles). Arithmetic order is unchanged
      // (bit-identical results).
      int j = j0 + 1;
      for (; j + 7 <= jend; j += 8) {
        double f[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) f[q] = (double)g.inv_s_t[(j + q) * NT + c];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          w *= lam * f[q];
          head_sum += w;
          head_n_sum += (double)(n0c + j + q) * w;
        }
      }
      for (; j + 3 <= jend; j += 4) {
        const double f0 = (double)g.inv_s_t[j * NT + c];
        const double f1 = (double)g.inv_s_t[(j + 1) * NT + c];
        const double f2 = (double)g.inv_s_t[(j + 2) * NT + c];
        const double f3 = (double)g.inv_s_t[(j + 3) * NT + c];
        w *= lam * f0;
        head_sum += w;
        head_n_sum += (double)(n0c + j) * w;
        w *= lam * f1;
        head_sum += w;
        head_n_sum += (double)(n0c + j + 1) * w;
        w *= lam * f2;
        head_sum += w;
        head_n_sum += (double)(n0c + j + 2) * w;
        w *= lam * f3;
        head_sum += w;
        head_n_sum += (double)(n0c + j + 3) * w;
      }
      for (; j <= jend; ++j) {
        w *= lam * (double)g.inv_s_t[j * NT + c];
        head_sum += w;
        head_n_sum += (double)(n0c + j) * w;
      }
    }
  }
  red_sum2_p<NT, PART>(head_sum, head_n_sum, scratch);

  // tail + final statistics: identical on every lane of the part (the head
  // sums are reduction results), so for multi-wave parts only the FIRST wave
  // computes it and broadcasts through LDS — the transcendental-heavy block
  // (log/exp/expm1) otherwise costs waves-per-part x instructions of VALU
  // throughput (the measured reason narrow blocks beat wide ones; see
  // ops/sweep.py choose_buckets)
  constexpr int NWH_T = (NT / PART) / WVA_WAVE;
  ChainOut o;
  if constexpr (NWH_T > 1) {
    __syncthreads();  // scratch handoff from red_sum2_p
    if (lane < WVA_WAVE) {
      o = chain_tail_stats(lam, loglam, logsN, g.S_total, N, K, m, head_sum, head_n_sum);
      if (lane == 0) {
        const int part = threadIdx.x / W;
        scratch[part * 4 + 0] = o.throughput;
        scratch[part * 4 + 1] = o.wait;
        scratch[part * 4 + 2] = o.serv;
        scratch[part * 4 + 3] = o.in_servers;
      }
    }
    __syncthreads();
    const int part = threadIdx.x / W;
    o.throughput = scratch[part * 4 + 0];
    o.wait = scratch[part * 4 + 1];
    o.serv = scratch[part * 4 + 2];
    o.in_servers = scratch[part * 4 + 3];
  } else {
    // single-wave part: lockstep execution makes the redundancy free (and the
    // one-wave cell stays barrier-free, which the fused tick relies on)
    o = chain_tail_stats(lam, loglam, logsN, g.S_total, N, K, m, head_sum, head_n_sum);
  }
  return o;
}

// ---------------------------------------------------------------------------
// analyzer mode 1: closed-form M/G/1/K (BASELINE config 4's "M/G/1 model").
// mu = s(N) (marginal per-request rate at max batch, req/msec), K = 11N,
// Pollaczek-Khinchine wait factor (1+cv2)/2, utilization-based effective
// concurrency eff = rho*N. O(1) per evaluation — no chain, no LDS.
// ---------------------------------------------------------------------------
struct Mg1Out {
  double throughput;  // req/msec
  double wait;        // msec
  double eff;         // effective concurrency
  double rho;         // clamped utilization
};

__device__ __forceinline__ Mg1Out mg1_eval(double lam, double mu, int K, double cv2, int N) {
  const double rho = lam / mu;
  double p0, pK, avg_n;
  if (fabs(rho - 1.0) < 1e-15) {
    p0 = 1.0 / (double)(K + 1);
    pK = p0;
    avg_n = (double)K * 0.5;
  } else {
    const double rK1 = pow(rho, (double)(K + 1));
    p0 = (1.0 - rho) / (1.0 - rK1);
    pK = p0 * pow(rho, (double)K);
    avg_n = rho / (1.0 - rho) - (double)(K + 1) * rK1 / (1.0 - rK1);
  }
  const double X = lam * (1.0 - pK);
  const double serv = 1.0 / mu;
  const double wait = fmax(avg_n / X - serv, 0.0) * (1.0 + cv2) * 0.5;
  Mg1Out o;
  o.throughput = X;
  o.wait = wait;
  const double rc = fmin(fmax(rho, 0.0), 1.0);
  o.rho = rc;
  o.eff = rc * (double)N;
  return o;
}

// The cell's own scalars, loaded once at the top of the cell function. The
// SLO targets and the arrival rate are not here: they belong to the mode's
// view of the cell (WvaView below).
struct WvaCell {
  int cell;  // index into the per-cell arrays
  int in_tok, out_tok, N;
  float alpha, beta, gamma, delta;
  float t_tps;
  int min_rep;
  float acc_cost, cur_cost;
  int cur_rep;
  bool cur_same, cur_empty, has_cur;
};

// The evaluator's model of the cell: what every evaluation after the geometry
// build reads. Identical on every thread of the cell except tid.
struct WvaModel {
  ChainGeom g;
  double logsN;
  int Kstates;  // maxQueue (10N) + N  (ref allocation.go:87)
  int mode;     // analyzer mode: 0 state-dependent chain, 1 closed-form M/G/1/K
  double cv2d;
  double mu;  // M/G/1 service rate s(N)
  double lam_min, lam_max;  // rate range of the bisections (req/msec)
  double *scratch;  // the cell's LDS header: [0..31] reductions, [32] S_total,
                    // [33..36] the bisections' result slots
  int tid;          // the thread's index within the cell's NT threads
};

// one evaluation at rate lam (req/msec) by the cell's analyzer: throughput
// (req/msec), wait (msec), effective concurrency, utilization
struct WvaEval {
  double tput, wait, eff, rho;
};
template <int NT, int PART>
__device__ __forceinline__ WvaEval wva_evaluate(double lam, const WvaCell &c, const WvaModel &m) {
  WvaEval e;
  if (m.mode == 1) {
    Mg1Out o = mg1_eval(lam, m.mu, m.Kstates, m.cv2d, c.N);
    e.tput = o.throughput;
    e.wait = o.wait;
    e.eff = o.eff;
    e.rho = o.rho;
  } else {
    ChainOut o = chain_eval<NT, PART>(lam, m.g, m.logsN, c.N, m.Kstates, m.scratch);
    e.tput = o.throughput;
    e.wait = o.wait;
    e.eff = effective_concurrency(o.serv, c.gamma, c.alpha, c.delta, c.beta, c.in_tok, c.out_tok,
                                  c.N);
    e.rho = fmin(fmax(o.in_servers / (double)c.N, 0.0), 1.0);
  }
  return e;
}

// kind 0: TTFT, kind 1: ITL at rate lam (msec)
template <int NT, int PART>
__device__ __forceinline__ double eval_metric(int kind, double lam, const WvaCell &c,
                                              const WvaModel &m) {
  const WvaEval e = wva_evaluate<NT, PART>(lam, c, m);
  if (kind == 0)
    return e.wait + (double)prefill_time_f(c.gamma, c.delta, c.in_tok, (float)e.eff);
  return (double)decode_time_f(c.alpha, c.beta, (float)e.eff);
}

__device__ __forceinline__ bool within_tol(double x, double value) {
  if (x == value) return true;
  if (value == 0.0) return false;
  return fabs((x - value) / value) <= WVA_TOL;
}

// Concurrent dual bisection: half-block 0 searches the TTFT target, half 1
// the ITL target, both matching pkg/analyzer/utils.go:26-70 exactly (boundary
// tolerance checks, below/above indicators, <=100 midpoint iterations with
// relative-tolerance early exit). The halves advance in LOCK-STEP — each
// step both halves run exactly one chain evaluation (a finished half keeps
// evaluating its last point as a no-op) so the __syncthreads counts inside
// the partial reductions stay uniform; a block-wide vote ends the loop when
// both halves are done. This halves the sequential depth of the sizing
// phase vs running the two searches back to back.
template <int NT>
__device__ __forceinline__ void dual_bisect(float t_ttft, float t_itl, const WvaCell &c,
                                            const WvaModel &m, double lam_star[2],
                                            int ind_out[2]) {
  constexpr int W = NT / 2;
  // the cell-relative index: threadIdx.x & 63 when the cell is one wave of a
  // wider block (fused tick, narrow blocks), threadIdx.x when it owns its block
  const int tid = m.tid;
  double *const res_slot = m.scratch + 33;  // 4 doubles
  const int h = tid / W;  // 0 = TTFT, 1 = ITL
  const double target = (h == 0) ? (double)t_ttft : (double)t_itl;
  const bool active = target > 0.0;

  double x_min = m.lam_min, x_max = m.lam_max;
  double x_star = m.lam_max;
  double y_lo = 0.0;
  bool increasing = true;
  int ind = 0;
  int phase = active ? 0 : 3;  // 0 eval lo, 1 eval hi, 2 bisect, 3 done
  int iters = 0;

  for (int step = 0; step < WVA_MAX_ITERS + 3; ++step) {
    double x_eval;
    if (phase == 0)
      x_eval = x_min;
    else if (phase == 1)
      x_eval = x_max;
    else if (phase == 2)
      x_eval = 0.5 * (x_min + x_max);
    else
      x_eval = x_max;  // done: dummy evaluation to keep barriers uniform
    const double y = eval_metric<NT, 2>(h, x_eval, c, m);
    if (phase == 0) {
      y_lo = y;
      if (within_tol(y_lo, target)) {
        x_star = x_min;
        phase = 3;
      } else {
        phase = 1;
      }
    } else if (phase == 1) {
      const double y_hi = y;
      if (within_tol(y_hi, target)) {
        x_star = x_max;
        phase = 3;
      } else {
        increasing = y_lo < y_hi;
        if ((increasing && target < y_lo) || (!increasing && target > y_lo)) {
          ind = -1;
          x_star = x_min;
          phase = 3;
        } else if ((increasing && target > y_hi) || (!increasing && target < y_hi)) {
          ind = +1;
          x_star = x_max;
          phase = 3;
        } else {
          phase = 2;
        }
      }
    } else if (phase == 2) {
      x_star = x_eval;
      ++iters;
      // fixed point: the interval has collapsed to <=1 ulp, so the midpoint
      // equals an endpoint and EVERY remaining iteration re-evaluates this
      // same x with the same outcome until the cap — exiting now returns the
      // identical x_star/ind with up to ~45 fewer chain evaluations
      const bool fixed_pt = (x_eval == x_min) || (x_eval == x_max);
      if (within_tol(y, target) || iters >= WVA_MAX_ITERS || fixed_pt) {
        phase = 3;
      } else if ((increasing && target < y) || (!increasing && target > y)) {
        x_max = x_star;
      } else {
        x_min = x_star;
      }
    }
    const bool done = (phase == 3);
    if constexpr (NT == WVA_WAVE) {
      // one-wave cell: a wave vote, no barrier (fused-tick narrow blocks rely
      // on the NT == 64 instantiation executing no barrier at all)
      if (__all(done ? 1 : 0)) break;
    } else {
      if (__syncthreads_and(done ? 1 : 0)) break;
    }
  }

  // publish both halves' results
  if ((tid % W) == 0) {
    res_slot[2 * h] = x_star;
    res_slot[2 * h + 1] = (double)ind;
  }
  if constexpr (NT == WVA_WAVE) {
    __builtin_amdgcn_s_waitcnt(0);  // one-wave cell: barrier-free (see above)
  } else {
    __syncthreads();
  }
  lam_star[0] = res_slot[0];
  ind_out[0] = (int)res_slot[1];
  lam_star[1] = res_slot[2];
  ind_out[1] = (int)res_slot[3];
}

// ---------------------------------------------------------------------------
// Sizing memo: one record per cell, owned by the native reconcile context.
// The SLO sizing phase (dual_bisect + the sized-rate evaluation) reads only
// the fields in the key below — never the arrival rate, the current
// allocation or min_replicas — so while the key repeats from tick to tick
// its fp64 result and feasibility verdict repeat bit for bit. The key is
// compared as raw 32-bit patterns ON THE DEVICE every tick, so a record can
// never be replayed for different inputs. NT is part of the key because the
// reduction order (hence the last bits of tput) depends on the block width.
// ---------------------------------------------------------------------------
#define WVA_MEMO_KEY_WORDS 13
#define WVA_MEMO_EMPTY 0u
#define WVA_MEMO_FEASIBLE 1u
#define WVA_MEMO_INFEASIBLE 2u  // SLO-infeasible or degenerate service rates

struct alignas(16) WvaMemoRec {
  unsigned key[WVA_MEMO_KEY_WORDS];
  unsigned status;  // written last
  double tput;      // tput_at_lam (req/msec); meaningful for status 1 only
};
static_assert(sizeof(WvaMemoRec) == 64, "memo record is one 64-byte line");

struct WvaMemoKey {
  unsigned w[WVA_MEMO_KEY_WORDS];
};

__device__ __forceinline__ WvaMemoKey memo_make_key(int in_tok, int out_tok, int N, float alpha,
                                                    float beta, float gamma, float delta,
                                                    float t_ttft, float t_itl, float t_tps,
                                                    float cv2, int analyzer_mode, int nt) {
  WvaMemoKey k;
  k.w[0] = (unsigned)in_tok;
  k.w[1] = (unsigned)out_tok;
  k.w[2] = (unsigned)N;
  k.w[3] = __float_as_uint(alpha);
  k.w[4] = __float_as_uint(beta);
  k.w[5] = __float_as_uint(gamma);
  k.w[6] = __float_as_uint(delta);
  k.w[7] = __float_as_uint(t_ttft);
  k.w[8] = __float_as_uint(t_itl);
  k.w[9] = __float_as_uint(t_tps);
  k.w[10] = __float_as_uint(cv2);
  k.w[11] = (unsigned)analyzer_mode;
  k.w[12] = (unsigned)nt;
  return k;
}

// called by thread 0 only, on a miss: payload and key first, status last
__device__ __forceinline__ void memo_store(WvaMemoRec *rec, const WvaMemoKey &k, double tput,
                                           unsigned status) {
#pragma unroll
  for (int q = 0; q < WVA_MEMO_KEY_WORDS; ++q) rec->key[q] = k.w[q];
  rec->tput = tput;
  __threadfence();
  rec->status = status;
}

// Zero-traffic result of one cell (ref allocation.go:73-75, 259-288) into
// output slot o: the empty allocation when the server may scale to zero, else
// min_replicas at the profile's max batch. Called by thread 0 only.
template <typename SlotT>
__device__ __forceinline__ void wva_write_zero(const WvaCellsOut &out, SlotT o, const WvaCell &c,
                                               const int *perf_max_batch) {
  if (c.min_rep == 0) {
    out.feasible[o] = 1;
    out.zero_empty[o] = 1;
    out.num_replicas[o] = 0;
    out.batch[o] = 0;
    out.cost[o] = 0.0f;
    out.itl[o] = 0.0f;
    out.ttft[o] = 0.0f;
    out.rho[o] = 0.0f;
    out.max_rate[o] = 0.0f;
    float value = 0.0f;
    if (c.has_cur) {
      if (c.cur_empty)
        value = (c.cur_rep == 0) ? 0.0f : (0.0f - c.cur_cost);
      else
        value = WVA_ACCEL_PENALTY * c.cur_cost + (0.0f - c.cur_cost);
    }
    out.value[o] = value;
  } else {
    int max_batch = perf_max_batch[c.cell];
    float cost = c.acc_cost * (float)c.min_rep;
    float decode1 = c.alpha + c.beta;
    // product rounded before the add in EVERY instantiation: the compiler
    // otherwise fuses it in some (planning) and not in others (it packs this
    // add with decode1's in the single-scenario kernels), and a scenario
    // slice must equal the single-scenario result bit for bit
    float max_decode;
    {
#pragma clang fp contract(off)
      max_decode = c.alpha + c.beta * (float)max_batch;
    }
    float prefill1 = c.gamma + c.delta;
    float max_serv = prefill1 + max_decode;
    out.feasible[o] = 1;
    out.zero_empty[o] = 0;
    out.num_replicas[o] = c.min_rep;
    out.batch[o] = max_batch;
    out.cost[o] = cost;
    out.itl[o] = decode1;
    out.ttft[o] = prefill1;
    out.rho[o] = 0.0f;
    out.max_rate[o] = (max_serv > 0.0f) ? (float)max_batch / max_serv : 0.0f;
    float value = cost;
    if (c.has_cur) {
      if (c.cur_same)
        value = (c.cur_rep == c.min_rep) ? 0.0f : (cost - c.cur_cost);
      else
        value = WVA_ACCEL_PENALTY * (c.cur_cost + cost) + (cost - c.cur_cost);
    }
    out.value[o] = value;
  }
}

// Replicas, cost and the per-replica analysis of one sized cell at arrival
// rate arr (req/min), written to output slot o (ref allocation.go:134-163).
// rate_star is the sized per-replica rate (req/sec). Every thread of the block
// calls this with the same arguments.
template <int NT, typename SlotT>
__device__ __forceinline__ void wva_eval_scenario(const WvaCellsOut &out, SlotT o, float arr,
                                                  double rate_star, const WvaCell &c,
                                                  const WvaModel &m) {
  double total_rate;  // req/sec (ref allocation.go:134-139)
  if (c.t_tps == 0.0f)
    total_rate = (double)arr / 60.0;
  else
    total_rate = (double)c.t_tps / (double)c.out_tok;
  double reps_d = ceil(total_rate / rate_star);
  if (!(reps_d > 0.0)) reps_d = 0.0;
  if (reps_d > 2147483000.0) reps_d = 2147483000.0;
  int num_replicas = (int)reps_d;
  if (num_replicas < c.min_rep) num_replicas = c.min_rep;

  const float cost = c.acc_cost * (float)num_replicas;

  // ---- per-replica analyze (ref allocation.go:148-157) ----
  const double rate = total_rate / (double)num_replicas;
  const WvaEval e = wva_evaluate<NT, 1>(rate / 1000.0, c, m);
  const float prefill_t = prefill_time_f(c.gamma, c.delta, c.in_tok, (float)e.eff);
  const float token_t = decode_time_f(c.alpha, c.beta, (float)e.eff);

  if (m.tid == 0) {
    out.feasible[o] = 1;
    out.zero_empty[o] = 0;
    out.num_replicas[o] = num_replicas;
    out.batch[o] = c.N;
    out.cost[o] = cost;
    out.itl[o] = token_t;
    out.ttft[o] = (float)e.wait + prefill_t;
    out.rho[o] = (float)e.rho;
    out.max_rate[o] = (float)(rate_star / 1000.0);
    float value = cost;
    if (c.has_cur) {
      if (c.cur_same && !c.cur_empty)
        value = (c.cur_rep == num_replicas) ? 0.0f : (cost - c.cur_cost);
      else
        value = WVA_ACCEL_PENALTY * (c.cur_cost + cost) + (cost - c.cur_cost);
    }
    out.value[o] = value;
  }
}

// scenario-planning arguments of the sweep body; the single-scenario
// instantiation takes an empty struct in their place
struct WvaPlanArgs {
  int n_cells;
  int n_scen;
  const float *scen_arrival;  // device, [n_scen][n_cells]
};
struct WvaNoPlan {};
// SLO planning: n_tgt target sets times n_load arrival-rate scenarios of the
// cell; outputs are [n_tgt][n_load][n_cells], target-major
struct WvaSloArgs {
  int n_cells;
  int n_load;
  const float *scen_arrival;  // device, [n_load][n_cells]
  int n_tgt;
  const float *scen_ttft;  // device, [n_tgt][n_cells]
  const float *scen_itl;   // device, [n_tgt][n_cells]
};
// what one launch of the sweep body covers per cell
#define WVA_MODE_SWEEP 0  // the cell's own targets and arrival rate
#define WVA_MODE_PLAN 1   // the cell's own targets, n_scen arrival rates
#define WVA_MODE_SLO 2    // n_tgt target sets x n_load arrival rates
#define WVA_MODE_HOLD 3   // the cell's own targets, n_scen (arrival rate, held replicas) pairs
// Hold analysis: the load plan's arguments plus the replicas the cell holds in
// every scenario. The replica count is pinned, not derived (wva_hold_body).
struct WvaHoldArgs {
  int n_cells;
  int n_scen;
  const float *scen_arrival;  // device, [n_scen][n_cells]
  const int *scen_held;       // device, [n_scen][n_cells]: -1 = not held in this
                              // scenario, >= 0 = held replicas
};
template <int MODE>
using WvaPlanParam = typename std::conditional<
    MODE == WVA_MODE_PLAN, WvaPlanArgs,
    typename std::conditional<
        MODE == WVA_MODE_SLO, WvaSloArgs,
        typename std::conditional<MODE == WVA_MODE_HOLD, WvaHoldArgs, WvaNoPlan>::type>::type>::
    type;

// The SLO sizing of one cell under targets (t_ttft, t_itl): the concurrent
// TTFT+ITL bisections (ref queueanalyzer.go:185-255), the minimum of the sized
// rates and the analysis at that rate (ref allocation.go:126-131). Returns
// false when a target cannot be met; else tput is the throughput at the sized
// rate (req/msec). Every thread of the block calls this with the same
// arguments and gets the same result.
template <int NT>
__device__ __forceinline__ bool wva_size_cell(float t_ttft, float t_itl, const WvaCell &c,
                                              const WvaModel &m, double &tput) {
  const double lam_max = m.lam_max;
  double lam_star[2];
  int inds[2];
  dual_bisect<NT>(t_ttft, t_itl, c, m, lam_star, inds);
  bool feasible = true;
  double lam_ttft = lam_max;
  if (t_ttft > 0.0f) {
    lam_ttft = lam_star[0];
    if (inds[0] < 0) feasible = false;
  }
  double lam_itl = lam_max;
  if (feasible && t_itl > 0.0f) {
    lam_itl = lam_star[1];
    if (inds[1] < 0) feasible = false;
  }
  if (!feasible) return false;
  double lam_tps = (c.t_tps > 0.0f) ? lam_max * (1.0 - WVA_STABILITY_FRACTION) : lam_max;
  double lam = fmin(fmin(lam_ttft, lam_itl), lam_tps);
  tput = wva_evaluate<NT, 1>(lam, c, m).tput;
  return true;
}

// A mode's view of one cell: n_tgt() target sets times n_load() arrival rates,
// the targets of set t, the arrival rate of load s (req/min), the output slot
// of slice (t, s), and memo_tgt(), the target set that owns the cell's memo
// record (-1: none). own_ttft / own_itl are the cell's own targets, which the
// memo key holds. Everything here is uniform over the cell's threads.
//
// A count that is 1 at compile time is returned as the type WvaOne, and
// wva_each(n, f), which is f(0) .. f(n - 1), is then the plain call f(0). A
// `for` over a constant 1 would compute the same, but its back edge survives
// until the loop passes, long after inlining. In the single-scenario kernels
// the zero-traffic exit then rejoins the main path, six of the cell's uniform
// loads and the memo record's land behind its stores as vector loads, and
// scratch grows from 60-68 to 100-128 B/lane (docs/design/kernels.md, "Cell
// function refactor").
using WvaOne = std::integral_constant<int, 1>;
template <typename F>
__device__ __forceinline__ void wva_each(int n, F &&f) {
  for (int i = 0; i < n; ++i) f(i);
}
template <typename F>
__device__ __forceinline__ void wva_each(WvaOne, F &&f) {
  f(0);
}
template <int MODE>
struct WvaView;
template <>
struct WvaView<WVA_MODE_SWEEP> {
  const int cell;
  const float own_ttft, own_itl, own_arrival;
  __device__ WvaView(const WvaCellsIn &in, const WvaNoPlan &, int cell)
      : cell(cell),
        own_ttft(in.t_ttft[cell]),
        own_itl(in.t_itl[cell]),
        own_arrival(in.arrival_rate[cell]) {}
  __device__ static constexpr WvaOne n_tgt() { return {}; }
  __device__ static constexpr WvaOne n_load() { return {}; }
  __device__ float ttft(int) const { return own_ttft; }
  __device__ float itl(int) const { return own_itl; }
  __device__ float arrival(int) const { return own_arrival; }
  __device__ int slot(int, int) const { return cell; }
  __device__ int memo_tgt() const { return 0; }
};
template <>
struct WvaView<WVA_MODE_PLAN> {
  const WvaPlanArgs &p;
  const int cell;
  const float own_ttft, own_itl;
  __device__ WvaView(const WvaCellsIn &in, const WvaPlanArgs &p, int cell)
      : p(p), cell(cell), own_ttft(in.t_ttft[cell]), own_itl(in.t_itl[cell]) {}
  __device__ static constexpr WvaOne n_tgt() { return {}; }
  __device__ int n_load() const { return p.n_scen; }
  __device__ float ttft(int) const { return own_ttft; }
  __device__ float itl(int) const { return own_itl; }
  // output slot s * n_cells + cell (up to 256 scenarios of the fleet)
  __device__ size_t slot(int, int s) const {
    return (size_t)s * (size_t)p.n_cells + (size_t)cell;
  }
  __device__ float arrival(int s) const { return p.scen_arrival[slot(0, s)]; }
  __device__ int memo_tgt() const { return 0; }
};
template <>
struct WvaView<WVA_MODE_SLO> {
  const WvaSloArgs &p;
  const int cell;
  const float own_ttft, own_itl;
  __device__ WvaView(const WvaCellsIn &in, const WvaSloArgs &p, int cell)
      : p(p), cell(cell), own_ttft(in.t_ttft[cell]), own_itl(in.t_itl[cell]) {}
  __device__ int n_tgt() const { return p.n_tgt; }
  __device__ int n_load() const { return p.n_load; }
  __device__ size_t row(int i) const { return (size_t)i * (size_t)p.n_cells + (size_t)cell; }
  __device__ float ttft(int t) const { return p.scen_ttft[row(t)]; }
  __device__ float itl(int t) const { return p.scen_itl[row(t)]; }
  __device__ float arrival(int s) const { return p.scen_arrival[row(s)]; }
  __device__ size_t slot(int t, int s) const {
    return ((size_t)t * (size_t)p.n_load + (size_t)s) * (size_t)p.n_cells + (size_t)cell;
  }
  // the first target set whose two targets are bit-equal to the cell's own.
  // Only that one may use the sizing memo, whose record is keyed on the cell's
  // own targets.
  __device__ int memo_tgt() const {
    int base = -1;
    for (int t = p.n_tgt - 1; t >= 0; --t)
      if (__float_as_uint(ttft(t)) == __float_as_uint(own_ttft) &&
          __float_as_uint(itl(t)) == __float_as_uint(own_itl))
        base = t;
    return base;
  }
};
// Hold analysis: the load plan's view plus held(s), the replicas the cell holds
// under load s (-1: the allocation of scenario s does not name this cell).
template <>
struct WvaView<WVA_MODE_HOLD> {
  const WvaHoldArgs &p;
  const int cell;
  const float own_ttft, own_itl;
  __device__ WvaView(const WvaCellsIn &in, const WvaHoldArgs &p, int cell)
      : p(p), cell(cell), own_ttft(in.t_ttft[cell]), own_itl(in.t_itl[cell]) {}
  __device__ static constexpr WvaOne n_tgt() { return {}; }
  __device__ int n_load() const { return p.n_scen; }
  __device__ float ttft(int) const { return own_ttft; }
  __device__ float itl(int) const { return own_itl; }
  __device__ size_t slot(int, int s) const {
    return (size_t)s * (size_t)p.n_cells + (size_t)cell;
  }
  __device__ float arrival(int s) const { return p.scen_arrival[slot(0, s)]; }
  __device__ int held(int s) const { return p.scen_held[slot(0, s)]; }
  __device__ int memo_tgt() const { return 0; }
};

// (thread 0 only) the "no allocation on this accelerator" verdict of target
// set t: its n_load slices. Per slice the zero-traffic decision still comes
// first, exactly as a single-scenario launch orders it.
template <typename View>
__device__ __forceinline__ void wva_write_infeasible(const WvaCellsOut &out, const View &v, int t,
                                                     const WvaCell &c,
                                                     const int *perf_max_batch) {
  wva_each(v.n_load(), [&](int s) {
    const auto o = v.slot(t, s);
    if (v.arrival(s) == 0.0f) {
      wva_write_zero(out, o, c, perf_max_batch);
    } else {
      out.feasible[o] = 0;
      out.zero_empty[o] = 0;
    }
  });
}

// The cell's region: a 40-double header in LDS (WvaModel::scratch), then the
// chain geometry, in LDS (GMEM=false: hot path, N <= WVA_XL_MAX_N) or in slab
// `slab` of global memory (GMEM=true: g_inv / g_anchor, strided by the
// bucket's max_n) — same algorithm, same arithmetic order, bit-identical
// results; used for the rare huge-N cells so the sweep stays uncapped like the
// reference. The slab layout mirrors the LDS layout (chunk-transposed
// reciprocals), which is also the coalesced global layout.
//
// wva_build_geom fills the geometry: fp32 service rates s(n), the transposed
// 1/s table and the log-prefix at every anchor (chunk loop, scan of the chunk
// totals, anchor fix-up), closed by a wait (one wave) or a barrier, so that
// every thread may read all of it on return. M/G/1 mode builds nothing: its
// evaluations are closed-form. Returns whether one of THIS lane's rates is
// degenerate (not positive and finite).
__device__ __forceinline__ int wva_num_decode(const WvaCell &c) {
  return (c.in_tok == 0 && c.out_tok == 1) ? 1 : c.out_tok - 1;
}
template <int NT, bool GMEM>
__device__ __forceinline__ bool wva_build_geom(const WvaCell &c, int tid, int analyzer_mode,
                                               double *smem, unsigned slab, int max_n,
                                               float *g_inv, double *g_anchor, ChainGeom &geom) {
  double *scratch = smem;
  const int N = c.N;
  const int num_decode = wva_num_decode(c);
  const int chunk = (N + NT - 1) / NT;
  const int ksub = (chunk + WVA_SUB - 1) / WVA_SUB;
  float *inv_s_t;
  double *S_anchor;
  if constexpr (GMEM) {
    // per-block slab in global memory, strided by the bucket's max geometry
    const int chunk_max = (max_n + NT - 1) / NT;
    const int ksub_max = (chunk_max + WVA_SUB - 1) / WVA_SUB;
    inv_s_t = g_inv + (size_t)slab * ((size_t)chunk_max * NT);
    S_anchor = g_anchor + (size_t)slab * ((size_t)NT * ksub_max);
  } else {
    double *S = smem + 40;                // LDS partition behind the header
    inv_s_t = (float *)S;                 // chunk*NT floats
    S_anchor = S + (chunk * NT + 1) / 2;  // NT*ksub doubles (8B aligned)
  }
  double *total_slot = scratch + 32;

  const int n0 = tid * chunk + 1;
  const int n1 = (analyzer_mode == 1) ? 0 : min(n0 + chunk - 1, N);
  double local = 0.0;
  bool bad_rate = false;
  for (int n = n0; n <= n1; ++n) {
    float nf = (float)n;
    float prefill = (c.in_tok == 0) ? 0.0f : (c.gamma + c.delta * (float)c.in_tok * nf);
    float decode = c.alpha + c.beta * nf;
    float s = nf / (prefill + (float)num_decode * decode);  // fp32 like the reference
    bad_rate = bad_rate || !(s > 0.0f) || !isfinite(s);
    local += log((double)s);
    const int j = n - n0;
    inv_s_t[j * NT + tid] = (float)(1.0 / (double)s);
    if ((j % WVA_SUB) == 0) S_anchor[tid * ksub + j / WVA_SUB] = local;  // chunk-local
  }
  // scan of per-thread chunk totals: intra-wave in registers...
  double incl = local;
#pragma unroll
  for (int off = 1; off < WVA_WAVE; off <<= 1) {
    double v = __shfl_up(incl, off, WVA_WAVE);
    if ((tid & (WVA_WAVE - 1)) >= off) incl += v;
  }
  double offset = incl - local;
  if constexpr (NT != WVA_WAVE) {
    // ...then cross-wave carries via scratch
    if ((tid & (WVA_WAVE - 1)) == WVA_WAVE - 1) scratch[tid / WVA_WAVE] = incl;
    __syncthreads();
    double carry = 0.0;
    for (int w = 0; w < tid / WVA_WAVE; ++w) carry += scratch[w];
    offset += carry;
  }
  for (int k = 0; k < ksub && n0 + k * WVA_SUB <= n1; ++k)
    S_anchor[tid * ksub + k] += offset;
  if (tid == NT - 1) *total_slot = offset + local;  // S[N]
  if constexpr (NT == WVA_WAVE) {
    // single wave: order LDS writes before reads. No barrier anywhere in the
    // geometry build of a one-wave cell (the scan above is shuffles only).
    __builtin_amdgcn_s_waitcnt(0);
  } else {
    __syncthreads();
  }
  geom.inv_s_t = inv_s_t;
  geom.S_anchor = S_anchor;
  geom.S_total = *total_slot;
  geom.chunk = chunk;
  geom.ksub = ksub;
  return bad_rate;
}

// ---------------------------------------------------------------------------
// K1: allocate-sweep. wva_cell_body is the computation of ONE cell by NT
// threads, separate from the block that runs it: `cell` is the cell, `tid` the
// thread's index within the cell's NT threads, `smem` the base of the cell's
// LDS region and `slab` the index of its global-memory slab (GMEM only). The
// bucket kernels (wva_sweep_block below) run one cell per block with tid =
// threadIdx.x, the base of dynamic LDS and slab = blockIdx.x; the fused tick
// kernel (wva_tick_t) also runs four one-wave cells side by side in one
// 256-thread block, each with tid = threadIdx.x & 63.
//
// MODE picks the view (WvaView<MODE>) and nothing else; the body is one
// sequence for all three:
//   WVA_MODE_SWEEP  one slice: the cell's own targets and arrival rate, into
//                   output slot `cell`;
//   WVA_MODE_PLAN   the cell's own targets, sized once, evaluated at n_scen
//                   arrival rates into slots s * n_cells + cell;
//   WVA_MODE_SLO    n_tgt target sets (the TPS target stays the cell's own),
//                   each sized and evaluated at n_load arrival rates into slots
//                   (t * n_load + s) * n_cells + cell. The geometry, which
//                   reads no target, is built once.
// Nothing the sizing reads depends on the arrival rate and nothing the
// geometry reads depends on a target (see the memo key), so slice (t, s) is
// bit for bit what a single-scenario launch with those targets and that
// arrival rate writes.
//
// The steps: (1) zero-traffic test over the loads, (2) memo lookup, (3)
// geometry, (4) degenerate-rate guard, (5) per target set: size it or take
// the memo's word, (6) per load: zero-traffic result, infeasible verdict or
// evaluation, in that order of precedence as in a single-scenario launch.
// It returns after (1), (2: memo-infeasible replay, one target set only),
// (4) or (6), every exit uniform over the cell's threads: each condition
// depends on the cell, on (cell, t) or on (cell, s) only, or is a reduction
// result or a value read back from the shared result slots. So every barrier
// inside dual_bisect and chain_eval is executed by all threads of a multi-wave
// cell, and a one-wave cell executes none.
//
// Outputs and memo records are stored by the cell's thread 0 ONLY, at every
// exit: wva_write_zero and wva_write_infeasible are called under `tid == 0`,
// wva_eval_scenario stores under `tid == 0`, and memo_miss_store does too.
// The fused tick's hand-off (release by that one lane) depends on it.
//
// LDS reuse across the sizings and evaluations of one cell. Blocks wider than
// one wave: every write to the reduction scratch (red_max_p, red_sum2_p,
// chain_eval's broadcast) sits behind a barrier that follows the previous
// reads of it, whichever call made them, so the order of calls does not
// matter. The bisection result slots are written at the end of dual_bisect and
// read by all threads right after its closing barrier; the next write to them
// is at the end of the next dual_bisect, whose loop runs at least one step and
// every step ends in a barrier (__syncthreads_and), in both analyzer modes —
// so a barrier separates the reads of target set t from the writes of t + 1,
// also when t ends early on the infeasible verdict. Single-wave cells use no
// scratch at all (their reductions are shuffles), and their result slots are
// written and read by one wave in program order: LDS serves a wave's accesses
// in issue order, and the s_waitcnt in dual_bisect completes the write before
// the reads. Nothing else in LDS is written after the geometry build.
// ---------------------------------------------------------------------------
template <int NT, bool GMEM, int MODE>
__device__ __forceinline__ void wva_cell_body(const WvaCellsIn &in, const WvaCellsOut &out,
                                              const int cell, const int tid, double *smem,
                                              const unsigned slab, int max_n, int analyzer_mode,
                                              float cv2, float *g_inv, double *g_anchor,
                                              WvaMemoRec *memo, unsigned *memo_cnt,
                                              const WvaPlanParam<MODE> &plan) {
  // memo: per-cell sizing records (nullptr = memo off: every cell is sized
  // from scratch and nothing is recorded); memo_cnt: [0] hits, [1] misses
  const int flags = in.flags[cell];
  WvaCell c;
  c.cell = cell;
  c.in_tok = in.in_tok[cell];
  c.out_tok = in.out_tok[cell];
  c.N = in.batch_n[cell];
  c.alpha = in.alpha[cell];
  c.beta = in.beta[cell];
  c.gamma = in.gamma[cell];
  c.delta = in.delta[cell];
  c.t_tps = in.t_tps[cell];
  c.min_rep = in.min_replicas[cell];
  c.acc_cost = in.acc_cost[cell];
  c.cur_cost = in.cur_cost[cell];
  c.cur_rep = in.cur_replicas[cell];
  c.cur_same = flags & 1;
  c.cur_empty = flags & 2;
  c.has_cur = flags & 4;
  const WvaView<MODE> v(in, plan, cell);

  // ---- (1) zero-traffic in EVERY load, hence in every slice: the decision
  // reads no target (ref allocation.go:73-75, 259-288)
  // (two forms of one test. With a single load the test is written as the
  // per-slice tests below are: the general form costs the single-scenario
  // kernels their scalar loads, see wva_each. With several loads, written on
  // `== 0.0f` like that, wva_plan_t reloads about twice as many spilled SGPRs
  // and measured 4-6 % slower; docs/design/kernels.md, "Cell function refactor")
  bool no_load;
  if constexpr (std::is_same<decltype(v.n_load()), WvaOne>::value) {
    no_load = v.arrival(0) == 0.0f || c.out_tok == 0;
  } else {
    bool any_load = false;
    if (c.out_tok != 0)
      wva_each(v.n_load(), [&](int s) { any_load = any_load || (v.arrival(s) != 0.0f); });
    no_load = !any_load;
  }
  if (no_load) {
    if (tid == 0)
      wva_each(v.n_tgt(), [&](int t) {
        wva_each(v.n_load(),
                 [&](int s) { wva_write_zero(out, v.slot(t, s), c, in.perf_max_batch); });
      });
    return;
  }

  // ---- (2) sizing memo lookup: every thread loads the cell's record (same
  // address cell-wide) and compares the key, so the verdict is uniform and
  // every barrier below stays uniform. The only writer is this cell's
  // thread 0 at one of the miss exits, which all lie behind a barrier (or,
  // for the single-wave cell, later in the same wave's program order).
  // The lookup, its counter and the miss store belong to target set memo_t;
  // without one (SLO planning only) the memo is neither read nor written.
  const int memo_t = v.memo_tgt();
  WvaMemoRec *const rec = (memo && memo_t >= 0) ? memo + cell : nullptr;
  const auto memo_key = [&]() {
    return memo_make_key(c.in_tok, c.out_tok, c.N, c.alpha, c.beta, c.gamma, c.delta, v.own_ttft,
                         v.own_itl, c.t_tps, cv2, analyzer_mode, NT);
  };
  unsigned memo_status = WVA_MEMO_EMPTY;
  double memo_tput = 0.0;
  if (rec) {
    const WvaMemoRec r = *rec;
    const WvaMemoKey k = memo_key();
    bool same = r.status == WVA_MEMO_FEASIBLE || r.status == WVA_MEMO_INFEASIBLE;
#pragma unroll
    for (int q = 0; q < WVA_MEMO_KEY_WORDS; ++q) same = same && (r.key[q] == k.w[q]);
    if (same) {
      memo_status = r.status;
      memo_tput = r.tput;
    }
    if (tid == 0) atomicAdd(memo_cnt + (same ? 0 : 1), 1u);
    if constexpr (MODE != WVA_MODE_SLO) {
      if (memo_status == WVA_MEMO_INFEASIBLE) {
        // replay of the infeasible verdict: no geometry, no evaluations
        if (tid == 0) wva_write_infeasible(out, v, 0, c, in.perf_max_batch);
        return;
      }
    }
    // (SLO planning replays it for target set memo_t in the loop below: the
    // other target sets still need the geometry)
  }
  // miss exits (degenerate, infeasible, sized) record their outcome; the key
  // is rebuilt here rather than kept live across the sizing phase.
  // (SLO planning reaches the degenerate exit after a hit too: no store then.
  // The other modes reach a miss exit only on a miss, since the key covers all
  // the geometry reads, so the test is always true there. It is not limited to
  // SLO mode as it once was: that form drops wva_plan_t<256> and <512> to 168
  // VGPRs and occupancy 3, and planning measured 3-6 % slower; this form
  // leaves the override-only wva_plan_t<128> at 164 VGPRs against 162.
  // docs/design/kernels.md, "Cell function refactor")
  auto memo_miss_store = [&](double tput, unsigned status) {
    if (rec && tid == 0 && memo_status == WVA_MEMO_EMPTY)
      memo_store(rec, memo_key(), tput, status);
  };

  // ---- (3) chain geometry
  WvaModel m;
  const bool bad_rate =
      wva_build_geom<NT, GMEM>(c, tid, analyzer_mode, smem, slab, max_n, g_inv, g_anchor, m.g);

  // ---- (4) s(1), s(N) in fp32 (rate-range bounds, ref queueanalyzer.go:117-119)
  const int num_decode = wva_num_decode(c);
  float prefill1 = (c.in_tok == 0) ? 0.0f : (c.gamma + c.delta * (float)c.in_tok);
  float s1 = 1.0f / (prefill1 + (float)num_decode * (c.alpha + c.beta));
  float prefillN = (c.in_tok == 0) ? 0.0f : (c.gamma + c.delta * (float)c.in_tok * (float)c.N);
  float sN = (float)c.N / (prefillN + (float)num_decode * (c.alpha + c.beta * (float)c.N));
  // degenerate perf parameters (zero/negative service times) -> infeasible
  // cell rather than propagating inf/nan through the chain (matches the CPU
  // golden's AnalyzerError guard)
  const double any_bad = red_max_p<NT, 1>(bad_rate ? 1.0 : 0.0, smem);
  if (any_bad > 0.0 || !(s1 > 0.0f) || !(sN > 0.0f) || !isfinite(s1) || !isfinite(sN)) {
    if (tid == 0)
      wva_each(v.n_tgt(),
               [&](int t) { wva_write_infeasible(out, v, t, c, in.perf_max_batch); });
    memo_miss_store(0.0, WVA_MEMO_INFEASIBLE);
    return;
  }
  m.logsN = log((double)sN);
  m.Kstates = 11 * c.N;
  m.mode = analyzer_mode;
  m.cv2d = (double)cv2;
  m.mu = (double)sN;
  m.lam_min = (double)s1 * WVA_EPSILON;
  m.lam_max = (double)sN * (1.0 - WVA_EPSILON);
  m.scratch = smem;
  m.tid = tid;

  wva_each(v.n_tgt(), [&](int t) {
    // ---- (5) size target set t, or take the memo's word for memo_t
    const bool owns_memo = (t == memo_t);
    double tput_at_lam = 0.0;
    bool feasible;
    if (owns_memo && memo_status == WVA_MEMO_FEASIBLE) {
      tput_at_lam = memo_tput;  // memo hit: the sizing would reproduce this value
      feasible = true;
    } else if (owns_memo && memo_status == WVA_MEMO_INFEASIBLE) {
      feasible = false;  // replay of the infeasible verdict, for this t only
    } else {
      feasible = wva_size_cell<NT>(v.ttft(t), v.itl(t), c, m, tput_at_lam);
      if (owns_memo)
        memo_miss_store(tput_at_lam, feasible ? WVA_MEMO_FEASIBLE : WVA_MEMO_INFEASIBLE);
    }
    // ---- (6) per load: zero-traffic result, infeasible verdict or evaluation
    if (!feasible) {
      if (tid == 0) wva_write_infeasible(out, v, t, c, in.perf_max_batch);
    } else {
      const double rate_star = tput_at_lam * 1000.0;  // req/sec
      wva_each(v.n_load(), [&](int s) {
        const float arr = v.arrival(s);
        if (arr == 0.0f) {
          if (tid == 0) wva_write_zero(out, v.slot(t, s), c, in.perf_max_batch);
        } else {
          wva_eval_scenario<NT>(out, v.slot(t, s), arr, rate_star, c, m);
        }
      });
    }
  });
}

// One cell per block: block blockIdx.x of a bucket launch computes cell
// cell_ids[blockIdx.x] with all its threads in the whole of dynamic LDS.
template <int NT, bool GMEM, int MODE>
__device__ __forceinline__ void wva_sweep_block(const WvaCellsIn &in, const WvaCellsOut &out,
                                                int n_blocks, const int *cell_ids, int max_n,
                                                int analyzer_mode, float cv2, float *g_inv,
                                                double *g_anchor, WvaMemoRec *memo,
                                                unsigned *memo_cnt,
                                                const WvaPlanParam<MODE> &plan) {
  extern __shared__ double smem[];
  if ((int)blockIdx.x >= n_blocks) return;
  const int cell = cell_ids ? cell_ids[blockIdx.x] : (int)blockIdx.x;
  wva_cell_body<NT, GMEM, MODE>(in, out, cell, (int)threadIdx.x, smem, blockIdx.x, max_n,
                                analyzer_mode, cv2, g_inv, g_anchor, memo, memo_cnt, plan);
}

template <int NT, bool GMEM>
__global__ void __launch_bounds__(NT, 4) wva_sweep_t(WvaCellsIn in, WvaCellsOut out, int n_blocks,
                                                  const int *cell_ids, int max_n,
                                                  int analyzer_mode, float cv2,
                                                  float *g_inv, double *g_anchor,
                                                  WvaMemoRec *memo, unsigned *memo_cnt) {
  wva_sweep_block<NT, GMEM, WVA_MODE_SWEEP>(in, out, n_blocks, cell_ids, max_n, analyzer_mode, cv2,
                                            g_inv, g_anchor, memo, memo_cnt, WvaNoPlan{});
}

// scenario-planning sweep: out arrays are [n_scen][n_cells]; in.arrival_rate
// is not read. WVA_PLAN_MIN_WAVES is the occupancy the register budget is
// sized for. The reconcile kernels use 4 (128 VGPRs); the scenario loop keeps
// more state live, and at 4 it spills 116-176 B/lane. At 2 it takes 162-175
// VGPRs with no scratch and measured 5-7% faster end to end
// (docs/design/kernels.md, "Scenario planning").
#ifndef WVA_PLAN_MIN_WAVES
#define WVA_PLAN_MIN_WAVES 2
#endif
template <int NT, bool GMEM>
__global__ void __launch_bounds__(NT, WVA_PLAN_MIN_WAVES)
    wva_plan_t(WvaCellsIn in, WvaCellsOut out, int n_blocks, const int *cell_ids, int max_n,
               int analyzer_mode, float cv2, float *g_inv, double *g_anchor, WvaMemoRec *memo,
               unsigned *memo_cnt, WvaPlanArgs plan) {
  wva_sweep_block<NT, GMEM, WVA_MODE_PLAN>(in, out, n_blocks, cell_ids, max_n, analyzer_mode, cv2,
                                           g_inv, g_anchor, memo, memo_cnt, plan);
}

// SLO-planning sweep: out arrays are [n_tgt][n_load][n_cells]; in.arrival_rate
// is not read, in.t_ttft / in.t_itl only to find the target set that may use
// the sizing memo. Built for the planning kernels' register budget
// (docs/design/kernels.md, "SLO planning").
template <int NT, bool GMEM>
__global__ void __launch_bounds__(NT, WVA_PLAN_MIN_WAVES)
    wva_slo_plan_t(WvaCellsIn in, WvaCellsOut out, int n_blocks, const int *cell_ids, int max_n,
                   int analyzer_mode, float cv2, float *g_inv, double *g_anchor, WvaMemoRec *memo,
                   unsigned *memo_cnt, WvaSloArgs plan) {
  wva_sweep_block<NT, GMEM, WVA_MODE_SLO>(in, out, n_blocks, cell_ids, max_n, analyzer_mode, cv2,
                                          g_inv, g_anchor, memo, memo_cnt, plan);
}

// Token-mix planning sweep: n_tok sets of per-cell (in_tok, out_tok, batch_n)
// times n_scen arrival-rate scenarios. Nothing of a cell survives a change of
// tokens (the geometry, N and with N the block width all move), so a set is
// not a loop inside the block: task w * n_cells + cell is a block of its own,
// in the bucket and at the width the single-scenario path gives that cell under
// set w. Block b runs task task_ids[b] (null: task b) as wva_plan_t runs a
// cell, on a view of the arrays shifted to the set: in.in_tok / out_tok /
// batch_n are [n_tok][n_cells] and the block reads row w, the ten outputs are
// [n_tok][n_scen][n_cells] and the block writes slab w of them, the arrivals
// [n_scen][n_cells] are shared, and everything else is the cell's own. The
// cell function runs unchanged on that view.
//
// No sizing memo: the n_tok blocks of one cell would race on its single
// record, and another set's sizing in it would cost the next reconcile a miss.
// The memo arguments are there for the launcher's sake and are not read.
//
// A task outside the grid, or one whose N does not fit the bucket it was put
// in, is skipped (uniformly, before any barrier): the host chose the buckets
// from the same batch_n it uploaded, so this only keeps a broken caller from
// running past the bucket's LDS or slab.
struct WvaTokArgs {
  int n_cells;
  int n_scen;
  const float *scen_arrival;  // device, [n_scen][n_cells]
  int n_tok;
};
template <int NT, bool GMEM>
__global__ void __launch_bounds__(NT, WVA_PLAN_MIN_WAVES)
    wva_tok_plan_t(WvaCellsIn in, WvaCellsOut out, int n_blocks, const int *task_ids, int max_n,
                   int analyzer_mode, float cv2, float *g_inv, double *g_anchor, WvaMemoRec *,
                   unsigned *, WvaTokArgs tok) {
  extern __shared__ double smem[];
  if ((int)blockIdx.x >= n_blocks) return;
  const int task = task_ids ? task_ids[blockIdx.x] : (int)blockIdx.x;
  if (task < 0 || tok.n_cells < 1 || task / tok.n_cells >= tok.n_tok) return;
  const int w = task / tok.n_cells;
  const int cell = task - w * tok.n_cells;
  const size_t row = (size_t)w * (size_t)tok.n_cells;
  const size_t slab = row * (size_t)tok.n_scen;
  in.in_tok += row;
  in.out_tok += row;
  in.batch_n += row;
  const int n = in.batch_n[cell];
  if (n < 1 || n > max_n) return;
  out.feasible += slab;
  out.zero_empty += slab;
  out.num_replicas += slab;
  out.batch += slab;
  out.cost += slab;
  out.value += slab;
  out.itl += slab;
  out.ttft += slab;
  out.rho += slab;
  out.max_rate += slab;
  const WvaPlanArgs plan = {tok.n_cells, tok.n_scen, tok.scen_arrival};
  wva_cell_body<NT, GMEM, WVA_MODE_PLAN>(in, out, cell, (int)threadIdx.x, smem, blockIdx.x, max_n,
                                         analyzer_mode, cv2, g_inv, g_anchor, nullptr, nullptr,
                                         plan);
}

// ---------------------------------------------------------------------------
// Hold analysis, K1 as wva_hold_t<NT>: what latency a FIXED allocation gives
// under n_scen loads. Scenario s pins the cell's replica count to held(s)
// (-1: the allocation of scenario s is not on this cell) where the other modes
// derive it from the sizing, and the slice gets a verdict instead of a
// candidate allocation. The ten output arrays keep their types and take the
// hold meanings:
//   feasible   -> status (WVA_HOLD_*)        zero_empty -> 1 = the cell is held
//   num_replicas -> held replicas            batch      -> needed replicas
//   cost  -> acc_cost * held                 value      -> slo_rate (req/min)
//   itl, ttft, rho                           max_rate   -> rate (req/s per replica)
//
// A sibling of wva_cell_body, not a fourth `if constexpr` arm inside it: the
// sequence differs at every step but the shared ones (wva_build_geom, the
// guard, wva_size_cell, wva_evaluate), and the existing kernels keep their
// registers, scratch and occupancy only if their body is left alone
// (docs/design/kernels.md, "Hold analysis").
//
// Per slice, in this order of precedence:
//   NOT_HELD   held(s) < 0: floats 0, needed -1;
//   IDLE       arrival(s) == 0 or out_tok == 0: itl / ttft / rho as
//              wva_write_zero reports them for the cell, needed 0;
//   INVALID    the degenerate-rate guard fires: no evaluation;
//   OVERLOADED held(s) == 0, or the per-replica rate total_rate / held / 1000
//              is above lam_max (the golden's analyze() refuses it): no
//              evaluation, itl = ttft = +inf, rho = 1;
//   else one wva_evaluate<NT, 1> at that rate, itl / ttft / rho exactly as
//   wva_eval_scenario computes them; OK iff the sizing is feasible and
//   held >= needed = ceil(total_rate / rate_star) (NOT raised to
//   min_replicas; -1 when the sizing is infeasible), else SLO_VIOLATED. The
//   verdict is on integers: the bisection's tolerance never decides it.
//
// The steps: (1) a cell that no scenario both holds and loads writes its
// slices from thread 0 and returns before the memo, the geometry or any
// barrier; (2) memo lookup as plan mode (same key, one counter move per cell
// that gets here), but an infeasible hit does not return: the geometry is
// still needed to evaluate; (3) geometry; (4) guard; (5) wva_size_cell or the
// memo's word, miss stores as in wva_cell_body, so a hold warms the memo for a
// reconcile and a reconcile for a hold; (6) per load the slice above.
//
// Uniformity: held(s) and arrival(s) depend on (cell, s) only, total_rate on
// (cell, s), lam_max and the sizing on the cell, so the early exit, the guard
// exit and every branch of the per-load step are taken by all threads of the
// cell or by none, and the barrier argument of wva_cell_body's plan loop
// carries over: every barrier inside wva_size_cell and wva_evaluate is executed
// by all threads of a multi-wave cell, a one-wave cell executes none. Loop
// bounds are n_scen. No polling, no cross-block traffic. Outputs and the memo
// record are stored by thread 0 only.
// ---------------------------------------------------------------------------
#define WVA_HOLD_OK 0
#define WVA_HOLD_SLO_VIOLATED 1
#define WVA_HOLD_OVERLOADED 2
#define WVA_HOLD_NOT_HELD 3
#define WVA_HOLD_IDLE 4
#define WVA_HOLD_INVALID 5
#define WVA_HOLD_STATUSES 6

// (thread 0 only) one slice record
__device__ __forceinline__ void wva_hold_write(const WvaCellsOut &out, size_t o, int status,
                                               int held, int needed, float cost, float slo_rate,
                                               float itl, float ttft, float rho, float rate) {
  out.feasible[o] = (uint8_t)status;
  out.zero_empty[o] = status != WVA_HOLD_NOT_HELD;
  out.num_replicas[o] = held;
  out.batch[o] = needed;
  out.cost[o] = cost;
  out.value[o] = slo_rate;
  out.itl[o] = itl;
  out.ttft[o] = ttft;
  out.rho[o] = rho;
  out.max_rate[o] = rate;
}

// (thread 0 only) a slice that needs no model of the cell: NOT_HELD, or IDLE
// with wva_write_zero's latencies (none for a server that may scale to zero,
// else the batch-1 decode and prefill times)
__device__ __forceinline__ void wva_hold_write_quiet(const WvaCellsOut &out, size_t o, int held,
                                                     const WvaCell &c) {
  if (held < 0) {
    wva_hold_write(out, o, WVA_HOLD_NOT_HELD, 0, -1, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f);
  } else {
    const bool none = c.min_rep == 0;
    wva_hold_write(out, o, WVA_HOLD_IDLE, held, 0, c.acc_cost * (float)held, 0.0f,
                   none ? 0.0f : c.alpha + c.beta, none ? 0.0f : c.gamma + c.delta, 0.0f, 0.0f);
  }
}

// The verdict and the per-replica analysis of one held, loaded slice: `held`
// replicas (>= 0) at arrival rate arr (req/min, not 0), written to slot o.
// rate_star is the sized per-replica rate (req/sec), meaningful when feasible.
// total_rate, the clamps of `needed`, the per-replica rate and the latency
// arithmetic are wva_eval_scenario's, with the replica count given instead of
// derived. Every thread of the block calls this with the same arguments.
template <int NT, typename SlotT>
__device__ __forceinline__ void wva_hold_scenario(const WvaCellsOut &out, SlotT o, float arr,
                                                  int held, bool feasible, double rate_star,
                                                  const WvaCell &c, const WvaModel &m) {
  double total_rate;  // req/sec (ref allocation.go:134-139)
  if (c.t_tps == 0.0f)
    total_rate = (double)arr / 60.0;
  else
    total_rate = (double)c.t_tps / (double)c.out_tok;
  int needed = -1;
  if (feasible) {
    double reps_d = ceil(total_rate / rate_star);
    if (!(reps_d > 0.0)) reps_d = 0.0;
    if (reps_d > 2147483000.0) reps_d = 2147483000.0;
    needed = (int)reps_d;
  }
  const float cost = c.acc_cost * (float)held;
  const float slo_rate = feasible ? (float)(rate_star * (double)held * 60.0) : 0.0f;

  // ---- per-replica analyze (ref allocation.go:148-157), unless the analyzer
  // refuses the rate (ref queueanalyzer.go:134-140)
  const double rate = total_rate / (double)held;
  if (held == 0 || !(rate / 1000.0 <= m.lam_max)) {  // uniform over the cell
    if (m.tid == 0)
      wva_hold_write(out, o, WVA_HOLD_OVERLOADED, held, needed, cost, slo_rate, INFINITY, INFINITY,
                     1.0f, held == 0 ? 0.0f : (float)rate);
    return;
  }
  const WvaEval e = wva_evaluate<NT, 1>(rate / 1000.0, c, m);
  const float prefill_t = prefill_time_f(c.gamma, c.delta, c.in_tok, (float)e.eff);
  const float token_t = decode_time_f(c.alpha, c.beta, (float)e.eff);
  if (m.tid == 0)
    wva_hold_write(out, o,
                   (feasible && held >= needed) ? WVA_HOLD_OK : WVA_HOLD_SLO_VIOLATED, held,
                   needed, cost, slo_rate, token_t, (float)e.wait + prefill_t, (float)e.rho,
                   (float)rate);
}

template <int NT, bool GMEM>
__device__ __forceinline__ void wva_hold_body(const WvaCellsIn &in, const WvaCellsOut &out,
                                              const int cell, const int tid, double *smem,
                                              const unsigned slab, int max_n, int analyzer_mode,
                                              float cv2, float *g_inv, double *g_anchor,
                                              WvaMemoRec *memo, unsigned *memo_cnt,
                                              const WvaHoldArgs &hold) {
  // the current allocation of the tick is not read: the held one replaces it
  WvaCell c;
  c.cell = cell;
  c.in_tok = in.in_tok[cell];
  c.out_tok = in.out_tok[cell];
  c.N = in.batch_n[cell];
  c.alpha = in.alpha[cell];
  c.beta = in.beta[cell];
  c.gamma = in.gamma[cell];
  c.delta = in.delta[cell];
  c.t_tps = in.t_tps[cell];
  c.min_rep = in.min_replicas[cell];
  c.acc_cost = in.acc_cost[cell];
  c.cur_cost = 0.0f;
  c.cur_rep = 0;
  c.cur_same = c.cur_empty = c.has_cur = false;
  const WvaView<WVA_MODE_HOLD> v(in, hold, cell);
  const int n_scen = v.n_load();

  // ---- (1) no scenario both holds and loads the cell
  bool active = false;
  if (c.out_tok != 0)
    for (int s = 0; s < n_scen; ++s)
      active = active || (v.held(s) >= 0 && v.arrival(s) != 0.0f);
  if (!active) {
    if (tid == 0)
      for (int s = 0; s < n_scen; ++s) wva_hold_write_quiet(out, v.slot(0, s), v.held(s), c);
    return;
  }
  // from here on out_tok != 0: slice s is quiet iff it is not held or not loaded
  const auto quiet = [&](int s) { return v.held(s) < 0 || v.arrival(s) == 0.0f; };

  // ---- (2) sizing memo lookup, as wva_cell_body's: uniform verdict, thread 0
  // of this cell the only writer
  WvaMemoRec *const rec = memo ? memo + cell : nullptr;
  const auto memo_key = [&]() {
    return memo_make_key(c.in_tok, c.out_tok, c.N, c.alpha, c.beta, c.gamma, c.delta, v.own_ttft,
                         v.own_itl, c.t_tps, cv2, analyzer_mode, NT);
  };
  unsigned memo_status = WVA_MEMO_EMPTY;
  double memo_tput = 0.0;
  if (rec) {
    const WvaMemoRec r = *rec;
    const WvaMemoKey k = memo_key();
    bool same = r.status == WVA_MEMO_FEASIBLE || r.status == WVA_MEMO_INFEASIBLE;
#pragma unroll
    for (int q = 0; q < WVA_MEMO_KEY_WORDS; ++q) same = same && (r.key[q] == k.w[q]);
    if (same) {
      memo_status = r.status;
      memo_tput = r.tput;
    }
    if (tid == 0) atomicAdd(memo_cnt + (same ? 0 : 1), 1u);
    // (an infeasible hit goes on: the held replicas are still evaluated)
  }
  auto memo_miss_store = [&](double tput, unsigned status) {
    if (rec && tid == 0 && memo_status == WVA_MEMO_EMPTY)
      memo_store(rec, memo_key(), tput, status);
  };

  // ---- (3) chain geometry
  WvaModel m;
  const bool bad_rate =
      wva_build_geom<NT, GMEM>(c, tid, analyzer_mode, smem, slab, max_n, g_inv, g_anchor, m.g);

  // ---- (4) rate-range bounds and the degenerate-rate guard, as wva_cell_body's
  const int num_decode = wva_num_decode(c);
  float prefill1 = (c.in_tok == 0) ? 0.0f : (c.gamma + c.delta * (float)c.in_tok);
  float s1 = 1.0f / (prefill1 + (float)num_decode * (c.alpha + c.beta));
  float prefillN = (c.in_tok == 0) ? 0.0f : (c.gamma + c.delta * (float)c.in_tok * (float)c.N);
  float sN = (float)c.N / (prefillN + (float)num_decode * (c.alpha + c.beta * (float)c.N));
  const double any_bad = red_max_p<NT, 1>(bad_rate ? 1.0 : 0.0, smem);
  if (any_bad > 0.0 || !(s1 > 0.0f) || !(sN > 0.0f) || !isfinite(s1) || !isfinite(sN)) {
    if (tid == 0)
      for (int s = 0; s < n_scen; ++s) {
        const int held = v.held(s);
        if (quiet(s))
          wva_hold_write_quiet(out, v.slot(0, s), held, c);
        else
          wva_hold_write(out, v.slot(0, s), WVA_HOLD_INVALID, held, -1, c.acc_cost * (float)held,
                         0.0f, 0.0f, 0.0f, 0.0f, 0.0f);
      }
    memo_miss_store(0.0, WVA_MEMO_INFEASIBLE);
    return;
  }
  m.logsN = log((double)sN);
  m.Kstates = 11 * c.N;
  m.mode = analyzer_mode;
  m.cv2d = (double)cv2;
  m.mu = (double)sN;
  m.lam_min = (double)s1 * WVA_EPSILON;
  m.lam_max = (double)sN * (1.0 - WVA_EPSILON);
  m.scratch = smem;
  m.tid = tid;

  // ---- (5) the cell's sizing, or the memo's word
  double tput_at_lam = 0.0;
  bool feasible;
  if (memo_status == WVA_MEMO_FEASIBLE) {
    tput_at_lam = memo_tput;
    feasible = true;
  } else if (memo_status == WVA_MEMO_INFEASIBLE) {
    feasible = false;
  } else {
    feasible = wva_size_cell<NT>(v.own_ttft, v.own_itl, c, m, tput_at_lam);
    memo_miss_store(tput_at_lam, feasible ? WVA_MEMO_FEASIBLE : WVA_MEMO_INFEASIBLE);
  }
  const double rate_star = tput_at_lam * 1000.0;  // req/sec

  // ---- (6) per load: quiet slice, overload verdict or evaluation
  for (int s = 0; s < n_scen; ++s) {
    if (quiet(s)) {
      if (tid == 0) wva_hold_write_quiet(out, v.slot(0, s), v.held(s), c);
    } else {
      wva_hold_scenario<NT>(out, v.slot(0, s), v.arrival(s), v.held(s), feasible, rate_star, c, m);
    }
  }
}

// out arrays are [n_scen][n_cells] with the hold meanings above; in.arrival_rate
// and the tick's current allocation are not read. Built for the planning
// kernels' register budget, one cell per block as wva_plan_t.
template <int NT, bool GMEM>
__global__ void __launch_bounds__(NT, WVA_PLAN_MIN_WAVES)
    wva_hold_t(WvaCellsIn in, WvaCellsOut out, int n_blocks, const int *cell_ids, int max_n,
               int analyzer_mode, float cv2, float *g_inv, double *g_anchor, WvaMemoRec *memo,
               unsigned *memo_cnt, WvaHoldArgs hold) {
  extern __shared__ double smem[];
  if ((int)blockIdx.x >= n_blocks) return;
  const int cell = cell_ids ? cell_ids[blockIdx.x] : (int)blockIdx.x;
  wva_hold_body<NT, GMEM>(in, out, cell, (int)threadIdx.x, smem, blockIdx.x, max_n, analyzer_mode,
                          cv2, g_inv, g_anchor, memo, memo_cnt, hold);
}

// ---------------------------------------------------------------------------
// K2: segmented argmin per server over the sweep output.
// ---------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(WVA_WAVE) wva_argmin(
    const float *value, const uint8_t *feasible, const int *seg_start, int n_servers,
    int *winner) {
  const int srv = blockIdx.x;
  if (srv >= n_servers) return;
  const int lane = threadIdx.x;
  const int beg = seg_start[srv], end = seg_start[srv + 1];
  float best = INFINITY;
  int best_i = -1;
  for (int i = beg + lane; i < end; i += WVA_WAVE) {
    if (!feasible[i]) continue;
    float v = value[i];
    if (best_i == -1 || v < best) {
      best = v;
      best_i = i;
    }
  }
#pragma unroll
  for (int off = WVA_WAVE / 2; off > 0; off >>= 1) {
    float ov = __shfl_down(best, off, WVA_WAVE);
    int oi = __shfl_down(best_i, off, WVA_WAVE);
    if (oi != -1 && (best_i == -1 || ov < best || (ov == best && oi < best_i))) {
      best = ov;
      best_i = oi;
    }
  }
  if (lane == 0) winner[srv] = best_i;
}

// ---------------------------------------------------------------------------
// C ABI launchers
// ---------------------------------------------------------------------------
// runtime (nt, gmem) -> template dispatch. GMEM instantiations exist for the
// two block widths the host's huge-bucket policy uses (256, 1024).
// >64 KiB dynamic-LDS opt-in per kernel instantiation (XL bucket). The
// runtime rejects opting into the full 160 KiB (measured: hipErrorInvalidValue
// above ~the launch-bounds-derived cap), so opt into the exact size needed,
// growing monotonically and caching per func so steady-state launches skip
// the runtime call.
static int wva_optin_lds(const void *func, size_t lds) {
  constexpr size_t kDefaultCap = 64 * 1024;
  if (lds <= kDefaultCap) return 0;
  static const void *funcs[16] = {};
  static size_t sizes[16] = {};
  int slot = -1;
  for (int i = 0; i < 16; ++i) {
    if (funcs[i] == func) {
      if (sizes[i] >= lds) return 0;
      slot = i;
      break;
    }
    if (funcs[i] == nullptr && slot < 0) slot = i;
  }
  int rc = (int)hipFuncSetAttribute(func, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds);
  if (rc != 0) return rc;
  if (slot >= 0) {
    funcs[slot] = func;
    sizes[slot] = lds;
  }
  return 0;
}

// dynamic LDS of one LDS-resident cell of up to max_n states on nt threads:
// header(40) + inv_s floats (chunk*nt/2 doubles, rounded up) + anchors
static size_t wva_cell_lds_bytes(int max_n, int nt) {
  const int chunk = (max_n + nt - 1) / nt;
  const int ksub = (chunk + WVA_SUB - 1) / WVA_SUB;
  return (size_t)(40 + (chunk * nt + 1) / 2 + (size_t)nt * ksub) * sizeof(double);
}

static int wva_sweep_dispatch(int n_blocks, int max_n, int nt, const int *cell_ids,
                              int analyzer_mode, float cv2, hipStream_t s,
                              const WvaCellsIn &in, const WvaCellsOut &out, float *g_inv,
                              double *g_anchor, WvaMemoRec *memo, unsigned *memo_cnt,
                              const WvaPlanArgs *plan = nullptr,
                              const WvaSloArgs *slo = nullptr,
                              const WvaTokArgs *tok = nullptr,
                              const WvaHoldArgs *hold = nullptr) {
  if (n_blocks <= 0) return 0;
  const bool gmem = g_inv != nullptr && g_anchor != nullptr;
  if (max_n < 1) return -2;
  if (!gmem && max_n > WVA_XL_MAX_N) return -2;
  if (gmem && max_n > WVA_HUGE_MAX_N) return -4;
  // the spill path keeps only the header in LDS
  size_t lds = gmem ? (size_t)40 * sizeof(double) : wva_cell_lds_bytes(max_n, nt);
  if (lds > 160 * 1024) return -5;  // exceeds the CU's LDS
  // opt in to the dynamic LDS, then launch; `tail` is the mode's argument
  // struct, if any. The >64 KiB opt-in is per function, so the planning
  // instantiations of a width opt in separately from the reconcile one.
  // (block size nt: WVA_LAUNCH below picks the instantiation with NT == nt)
  auto launch = [&](auto kernel, auto... tail) -> int {
    int rc = wva_optin_lds(reinterpret_cast<const void *>(kernel), lds);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(kernel, dim3(n_blocks), dim3(nt), lds, s, in, out, n_blocks, cell_ids,
                       max_n, analyzer_mode, cv2, g_inv, g_anchor, memo, memo_cnt, tail...);
    return 0;
  };
  int rc = -3;
#define WVA_LAUNCH(NTV, GM)                                        \
  rc = hold != nullptr   ? launch(&wva_hold_t<NTV, GM>, *hold)     \
       : tok != nullptr  ? launch(&wva_tok_plan_t<NTV, GM>, *tok)  \
       : slo != nullptr  ? launch(&wva_slo_plan_t<NTV, GM>, *slo)  \
       : plan != nullptr ? launch(&wva_plan_t<NTV, GM>, *plan)     \
                         : launch(&wva_sweep_t<NTV, GM>)
  if (gmem) {
    switch (nt) {
      case 256: WVA_LAUNCH(256, true); break;
      case 1024: WVA_LAUNCH(1024, true); break;
      default: return -3;
    }
  } else {
    switch (nt) {
      case 64: WVA_LAUNCH(64, false); break;
      case 128: WVA_LAUNCH(128, false); break;
      case 256: WVA_LAUNCH(256, false); break;
      case 512: WVA_LAUNCH(512, false); break;
      case 1024: WVA_LAUNCH(1024, false); break;
      default: return -3;
    }
  }
#undef WVA_LAUNCH
  if (rc != 0) return rc;
  return (int)hipGetLastError();
}

extern "C" int wva_sweep_launch_bucket(
    int n_blocks, int max_n, int nt, const int *cell_ids, int analyzer_mode, float cv2,
    void *stream,
    const int *in_tok, const int *out_tok, const int *batch_n, const int *min_replicas,
    const int *perf_max_batch, const int *cur_replicas, const int *flags,
    const float *alpha, const float *beta, const float *gamma, const float *delta,
    const float *arrival_rate, const float *t_itl, const float *t_ttft, const float *t_tps,
    const float *acc_cost, const float *cur_cost,
    uint8_t *feasible, uint8_t *zero_empty, int *num_replicas, int *batch, float *cost,
    float *value, float *itl, float *ttft, float *rho, float *max_rate,
    void *g_inv, void *g_anchor) {
  WvaCellsIn in = {in_tok, out_tok, batch_n, min_replicas, perf_max_batch, cur_replicas, flags,
                   alpha, beta, gamma, delta, arrival_rate, t_itl, t_ttft, t_tps, acc_cost,
                   cur_cost};
  WvaCellsOut out = {feasible, zero_empty, num_replicas, batch, cost, value, itl, ttft, rho,
                     max_rate};
  return wva_sweep_dispatch(n_blocks, max_n, nt, cell_ids, analyzer_mode, cv2,
                            (hipStream_t)stream, in, out, (float *)g_inv, (double *)g_anchor,
                            nullptr, nullptr);  // one-shot API: no sizing memo
}

extern "C" int wva_argmin_launch(int n_servers, void *stream, const float *value,
                                 const uint8_t *feasible, const int *seg_start, int *winner) {
  if (n_servers <= 0) return 0;
  hipLaunchKernelGGL(wva_argmin, dim3(n_servers), dim3(WVA_WAVE), 0, (hipStream_t)stream, value,
                     feasible, seg_start, n_servers, winner);
  return (int)hipGetLastError();
}

extern "C" int wva_device_count(int *count) { return (int)hipGetDeviceCount(count); }

// ---------------------------------------------------------------------------
// The per-server winner record, which the host reads back from small pinned
// buffers. gf rows: cost, value, itl, ttft, rho, max_rate; gi rows: acc_code
// (-1 none, -2 zero-load empty, else accelerator index), num_replicas,
// batch, winner cell index. K4 and K4b select the winner and write its record
// in one launch.
//
// K4 wva_plan_reduce: winner selection + winner record + per-accelerator
// replica totals for every (server, scenario) of a planning sweep in one
// launch. Grid (n_srv, n_scen), one wave each. The selection is wva_argmin's
// rule on scenario slice s (minimum value over feasible cells, lowest cell
// index on ties), the record is the one above, written into
// pf[n_scen][6][n_srv] / pi[n_scen][4][n_srv]. totals[n_scen][n_acc] must be
// zero on entry; the winner's replica count is added with a 64-bit integer
// atomic (a cell may hold 2 147 483 000 replicas, and integer adds make the
// sum independent of execution order).
// ---------------------------------------------------------------------------
// Shared by wva_plan_reduce and wva_winner: one wave selects server srv's
// winner on scenario slice sc (cell arrays offset by sc * n_cells) and lane 0
// writes the record into gf[6][n_srv] / gi[4][n_srv]. Returns the winner cell
// index on lane 0 (other lanes: unspecified); acc and reps are lane 0's
// record fields.
__device__ __forceinline__ int wva_winner_record(
    const float *value, const uint8_t *feasible, const uint8_t *zero_empty, const int *cell_acc,
    const int *num_replicas, const int *batch, const float *cost, const float *itl,
    const float *ttft, const float *rho, const float *max_rate, const int *seg_start, int n_srv,
    size_t base, int srv, float *gf, int *gi, int &acc, int &reps, const int lane) {
  // lane: the thread's lane in the wave that runs this (threadIdx.x in the
  // one-wave blocks of K4 / K4b; threadIdx.x & 63 in the fused tick kernel)
  const int beg = seg_start[srv], end = seg_start[srv + 1];
  float best = INFINITY;
  int best_i = -1;
  for (int i = beg + lane; i < end; i += WVA_WAVE) {
    if (!feasible[base + i]) continue;
    float v = value[base + i];
    if (best_i == -1 || v < best) {
      best = v;
      best_i = i;
    }
  }
#pragma unroll
  for (int off = WVA_WAVE / 2; off > 0; off >>= 1) {
    float ov = __shfl_down(best, off, WVA_WAVE);
    int oi = __shfl_down(best_i, off, WVA_WAVE);
    if (oi != -1 && (best_i == -1 || ov < best || (ov == best && oi < best_i))) {
      best = ov;
      best_i = oi;
    }
  }
  acc = -1;
  reps = 0;
  if (lane != 0) return -1;
  const int w = best_i;
  const bool has = w >= 0;
  const size_t wc = base + (size_t)(has ? w : 0);
  acc = has ? (zero_empty[wc] ? -2 : cell_acc[w]) : -1;
  reps = has ? num_replicas[wc] : 0;
  gf[0 * n_srv + srv] = has ? cost[wc] : 0.0f;
  gf[1 * n_srv + srv] = has ? value[wc] : 0.0f;
  gf[2 * n_srv + srv] = has ? itl[wc] : 0.0f;
  gf[3 * n_srv + srv] = has ? ttft[wc] : 0.0f;
  gf[4 * n_srv + srv] = has ? rho[wc] : 0.0f;
  gf[5 * n_srv + srv] = has ? max_rate[wc] : 0.0f;
  gi[0 * n_srv + srv] = acc;
  gi[1 * n_srv + srv] = reps;
  gi[2 * n_srv + srv] = has ? batch[wc] : 0;
  gi[3 * n_srv + srv] = w;
  return w;
}

extern "C" __global__ void __launch_bounds__(WVA_WAVE) wva_plan_reduce(
    const float *value, const uint8_t *feasible, const uint8_t *zero_empty, const int *cell_acc,
    const int *num_replicas, const int *batch, const float *cost, const float *itl,
    const float *ttft, const float *rho, const float *max_rate, const int *seg_start, int n_srv,
    int n_cells, int n_scen, int n_acc, float *pf, int *pi, unsigned long long *totals) {
  const int srv = blockIdx.x;
  const int sc = blockIdx.y;
  if (srv >= n_srv || sc >= n_scen) return;
  int acc, reps;
  wva_winner_record(value, feasible, zero_empty, cell_acc, num_replicas, batch, cost, itl, ttft,
                    rho, max_rate, seg_start, n_srv, (size_t)sc * (size_t)n_cells, srv,
                    pf + (size_t)sc * 6 * (size_t)n_srv, pi + (size_t)sc * 4 * (size_t)n_srv, acc,
                    reps, (int)threadIdx.x);
  if (threadIdx.x != 0) return;
  if (acc >= 0 && acc < n_acc && reps > 0)
    atomicAdd(totals + (size_t)sc * (size_t)n_acc + (size_t)acc, (unsigned long long)reps);
}

// ---------------------------------------------------------------------------
// K4c wva_rollout: the winner step of a forecast rollout. The n_steps slices of
// a planning sweep are consecutive ticks: step s is judged against the
// allocation step s - 1 left behind (winner none: unchanged; zero-load empty:
// empty; else the winner's accelerator, replicas and cost). That chain is per
// server and lives in registers: cur_acc (-3 none, -1 empty, >= 0 accelerator
// index), cur_rep, cur_cost, starting from cur[3][n_srv] and written back there
// after the last step.
//
// `group` lanes (a power of two, 1..64) serve one server, 64 / group servers
// share a one-wave block; lane `sub` of a group takes cells beg + sub,
// beg + sub + group, ... of the server's segment. Per step every lane reads its
// cells' slice outputs (none of them depends on the chain), recomputes `value`
// against the chain's current allocation and stores it, the group selects the
// winner by wva_winner_record's rule (minimum value over feasible cells, lowest
// cell index on ties; same shuffle order), the lane that owns the winner writes
// the record into pf[n_steps][6][n_srv] / pi[n_steps][4][n_srv] and adds its
// replicas to totals[n_steps][n_acc] (zero on entry), and all lanes of the
// group take the winner as the new current allocation. No barrier, no LDS.
//
// The value expression is the reconcile kernels' one (wva_sweep_t, wva_tick_t)
// as their machine code has it: cost is the rounded fp32 product the slice
// holds, the sum and the difference are rounded, and only the penalty multiply
// is fused into the final add. It is computed for every step, step 0 included,
// so that no step depends on how the planning kernel happened to contract the
// same source expression.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float wva_rollout_value(bool zero_empty, int reps, float cost,
                                                   int acc, int cur_acc, int cur_rep,
                                                   float cur_cost) {
#pragma clang fp contract(off)
  if (cur_acc == -3) return zero_empty ? 0.0f : cost;
  if (zero_empty) {
    if (cur_acc == -1) return (cur_rep == 0) ? 0.0f : (0.0f - cur_cost);
    return __fmaf_rn(cur_cost, WVA_ACCEL_PENALTY, 0.0f - cur_cost);
  }
  if (cur_acc >= 0 && cur_acc == acc) return (cur_rep == reps) ? 0.0f : (cost - cur_cost);
  return __fmaf_rn(cur_cost + cost, WVA_ACCEL_PENALTY, cost - cur_cost);
}

extern "C" __global__ void __launch_bounds__(WVA_WAVE) wva_rollout(
    float *value, const uint8_t *feasible, const uint8_t *zero_empty, const int *cell_acc,
    const int *num_replicas, const int *batch, const float *cost, const float *itl,
    const float *ttft, const float *rho, const float *max_rate, const int *seg_start, int n_srv,
    int n_cells, int n_steps, int n_acc, int group, float *pf, int *pi,
    unsigned long long *totals, int *cur) {
  const int lane = (int)threadIdx.x;
  const int sub = lane & (group - 1);
  const int srv = (int)blockIdx.x * (WVA_WAVE / group) + lane / group;
  // lanes past the last server keep an empty segment and store nothing, but
  // stay in the loop: the shuffles below are executed by the whole wave
  const bool live = srv < n_srv;
  const int beg = live ? seg_start[srv] : 0;
  const int end = live ? seg_start[srv + 1] : 0;
  int cur_acc = live ? cur[0 * n_srv + srv] : -3;
  int cur_rep = live ? cur[1 * n_srv + srv] : 0;
  float cur_cost = live ? __int_as_float(cur[2 * n_srv + srv]) : 0.0f;

  for (int s = 0; s < n_steps; ++s) {
    const size_t base = (size_t)s * (size_t)n_cells;
    // this lane's best candidate and the fields its record and the chain need
    float best = INFINITY;
    int best_i = -1;
    int b_acc = -1, b_reps = 0, b_batch = 0;
    float b_cost = 0.0f, b_itl = 0.0f, b_ttft = 0.0f, b_rho = 0.0f, b_rate = 0.0f;
    for (int i = beg + sub; i < end; i += group) {
      const size_t o = base + (size_t)i;
      if (!feasible[o]) continue;
      const bool ze = zero_empty[o] != 0;
      const int reps = num_replicas[o];
      const float c = cost[o];
      const int acc = cell_acc[i];
      const float v = wva_rollout_value(ze, reps, c, acc, cur_acc, cur_rep, cur_cost);
      value[o] = v;
      if (best_i == -1 || v < best) {
        best = v;
        best_i = i;
        b_acc = ze ? -2 : acc;
        b_reps = reps;
        b_cost = c;
        b_batch = batch[o];
        b_itl = itl[o];
        b_ttft = ttft[o];
        b_rho = rho[o];
        b_rate = max_rate[o];
      }
    }
    // the group's winner on its lane 0 (wva_winner_record's reduction), then
    // on every lane of the group
    float win = best;
    int w = best_i;
    for (int off = group >> 1; off > 0; off >>= 1) {
      const float ov = __shfl_down(win, off, group);
      const int oi = __shfl_down(w, off, group);
      if (oi != -1 && (w == -1 || ov < win || (ov == win && oi < w))) {
        win = ov;
        w = oi;
      }
    }
    w = __shfl(w, 0, group);
    // the lane whose candidate won holds the winner's fields
    const bool owner = live && w >= 0 && w == best_i;
    if (owner || (live && w < 0 && sub == 0)) {
      float *gf = pf + (size_t)s * 6 * (size_t)n_srv;
      int *gi = pi + (size_t)s * 4 * (size_t)n_srv;
      gf[0 * n_srv + srv] = b_cost;
      gf[1 * n_srv + srv] = owner ? best : 0.0f;
      gf[2 * n_srv + srv] = b_itl;
      gf[3 * n_srv + srv] = b_ttft;
      gf[4 * n_srv + srv] = b_rho;
      gf[5 * n_srv + srv] = b_rate;
      gi[0 * n_srv + srv] = b_acc;
      gi[1 * n_srv + srv] = b_reps;
      gi[2 * n_srv + srv] = b_batch;
      gi[3 * n_srv + srv] = w;
      if (b_acc >= 0 && b_acc < n_acc && b_reps > 0)
        atomicAdd(totals + (size_t)s * (size_t)n_acc + (size_t)b_acc, (unsigned long long)b_reps);
    }
    // desired -> current, on every lane of the group
    const int src = (w >= 0) ? ((w - beg) & (group - 1)) : 0;
    const int n_acc_code = __shfl(b_acc, src, group);
    const int n_reps = __shfl(b_reps, src, group);
    const float n_cost = __shfl(b_cost, src, group);
    if (w >= 0) {
      cur_acc = (n_acc_code == -2) ? -1 : n_acc_code;
      cur_rep = n_reps;
      cur_cost = n_cost;
    }
  }
  if (live && sub == 0) {
    cur[0 * n_srv + srv] = cur_acc;
    cur[1 * n_srv + srv] = cur_rep;
    cur[2 * n_srv + srv] = __float_as_int(cur_cost);
  }
}

// ---------------------------------------------------------------------------
// K4e wva_rollout_paths: wva_rollout for the paths of a forecast ensemble. The
// planning sweep's slices are n_paths paths of n_steps consecutive ticks, slice
// p * n_steps + s being tick s of the pass's p-th path; grid (server groups,
// n_paths), block (x, p) runs wva_rollout's chain for its servers on path p.
// Work split, value expression, selection rule and shuffle order are
// wva_rollout's, written out here so that wva_rollout keeps its registers.
// Every path starts from start[3][n_srv], which nobody writes.
//
// Per (path, tick) = ensemble row gr = (path0 + p) * n_steps + s the lane that
// owns the winner (lane 0 of the group when there is none) writes the compact
// record ens_code / ens_reps / ens_cost [rows][n_srv] (row-major: the stores
// of a wave's servers are consecutive words) and adds the winner's replicas to
// ens_tot[rows][n_acc] with the 64-bit integer atomic; lane 0 of the group
// counts the server into ens_nowin[rows] when the tick has no winner and into
// ens_chg[rows] when the current accelerator after the tick differs from the
// one before (a tick without a winner changes nothing). Integer atomics on
// words that are zero on entry: the sums do not depend on the order. After the
// last tick the path's allocation goes to ens_fin[paths][3][n_srv].
//
// With `full` the pass also writes the pf / pi records of its slices and the
// recomputed per-cell value, as wva_rollout does. No barrier, no LDS, no
// polling; the loop runs n_steps times whatever the data.
// ---------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(WVA_WAVE) wva_rollout_paths(
    float *value, const uint8_t *feasible, const uint8_t *zero_empty, const int *cell_acc,
    const int *num_replicas, const int *batch, const float *cost, const float *itl,
    const float *ttft, const float *rho, const float *max_rate, const int *seg_start, int n_srv,
    int n_cells, int n_steps, int n_paths, int n_acc, int group, int path0, int full, float *pf,
    int *pi, const int *start, int *ens_code, int *ens_reps, float *ens_cost,
    unsigned long long *ens_tot, int *ens_nowin, int *ens_chg, int *ens_fin) {
  const int lane = (int)threadIdx.x;
  const int sub = lane & (group - 1);
  const int srv = (int)blockIdx.x * (WVA_WAVE / group) + lane / group;
  const int p = (int)blockIdx.y;
  if (p >= n_paths) return;  // whole block
  // lanes past the last server keep an empty segment and store nothing, but
  // stay in the loop: the shuffles below are executed by the whole wave
  const bool live = srv < n_srv;
  const int beg = live ? seg_start[srv] : 0;
  const int end = live ? seg_start[srv + 1] : 0;
  int cur_acc = live ? start[0 * n_srv + srv] : -3;
  int cur_rep = live ? start[1 * n_srv + srv] : 0;
  float cur_cost = live ? __int_as_float(start[2 * n_srv + srv]) : 0.0f;

  for (int s = 0; s < n_steps; ++s) {
    const size_t slice = (size_t)p * (size_t)n_steps + (size_t)s;
    const size_t base = slice * (size_t)n_cells;
    float best = INFINITY;
    int best_i = -1;
    int b_acc = -1, b_reps = 0, b_batch = 0;
    float b_cost = 0.0f, b_itl = 0.0f, b_ttft = 0.0f, b_rho = 0.0f, b_rate = 0.0f;
    for (int i = beg + sub; i < end; i += group) {
      const size_t o = base + (size_t)i;
      if (!feasible[o]) continue;
      const bool ze = zero_empty[o] != 0;
      const int reps = num_replicas[o];
      const float c = cost[o];
      const int acc = cell_acc[i];
      const float v = wva_rollout_value(ze, reps, c, acc, cur_acc, cur_rep, cur_cost);
      if (full) value[o] = v;
      if (best_i == -1 || v < best) {
        best = v;
        best_i = i;
        b_acc = ze ? -2 : acc;
        b_reps = reps;
        b_cost = c;
        if (full) {
          b_batch = batch[o];
          b_itl = itl[o];
          b_ttft = ttft[o];
          b_rho = rho[o];
          b_rate = max_rate[o];
        }
      }
    }
    float win = best;
    int w = best_i;
    for (int off = group >> 1; off > 0; off >>= 1) {
      const float ov = __shfl_down(win, off, group);
      const int oi = __shfl_down(w, off, group);
      if (oi != -1 && (w == -1 || ov < win || (ov == win && oi < w))) {
        win = ov;
        w = oi;
      }
    }
    w = __shfl(w, 0, group);
    const size_t gr = ((size_t)path0 + (size_t)p) * (size_t)n_steps + (size_t)s;
    const bool owner = live && w >= 0 && w == best_i;
    if (owner || (live && w < 0 && sub == 0)) {
      const size_t r = gr * (size_t)n_srv + (size_t)srv;
      ens_code[r] = b_acc;
      ens_reps[r] = b_reps;
      ens_cost[r] = b_cost;
      if (b_acc >= 0 && b_acc < n_acc && b_reps > 0)
        atomicAdd(ens_tot + gr * (size_t)n_acc + (size_t)b_acc, (unsigned long long)b_reps);
      if (full) {
        float *gf = pf + slice * 6 * (size_t)n_srv;
        int *gi = pi + slice * 4 * (size_t)n_srv;
        gf[0 * n_srv + srv] = b_cost;
        gf[1 * n_srv + srv] = owner ? best : 0.0f;
        gf[2 * n_srv + srv] = b_itl;
        gf[3 * n_srv + srv] = b_ttft;
        gf[4 * n_srv + srv] = b_rho;
        gf[5 * n_srv + srv] = b_rate;
        gi[0 * n_srv + srv] = b_acc;
        gi[1 * n_srv + srv] = b_reps;
        gi[2 * n_srv + srv] = b_batch;
        gi[3 * n_srv + srv] = w;
      }
    }
    // desired -> current, on every lane of the group
    const int src = (w >= 0) ? ((w - beg) & (group - 1)) : 0;
    const int n_acc_code = __shfl(b_acc, src, group);
    const int n_reps = __shfl(b_reps, src, group);
    const float n_cost = __shfl(b_cost, src, group);
    if (w >= 0) {
      const int new_acc = (n_acc_code == -2) ? -1 : n_acc_code;
      if (live && sub == 0 && new_acc != cur_acc) atomicAdd(ens_chg + gr, 1);
      cur_acc = new_acc;
      cur_rep = n_reps;
      cur_cost = n_cost;
    } else if (live && sub == 0) {
      atomicAdd(ens_nowin + gr, 1);
    }
  }
  if (live && sub == 0) {
    int *fin = ens_fin + ((size_t)path0 + (size_t)p) * 3 * (size_t)n_srv;
    fin[0 * n_srv + srv] = cur_acc;
    fin[1 * n_srv + srv] = cur_rep;
    fin[2 * n_srv + srv] = __float_as_int(cur_cost);
  }
}

// ---------------------------------------------------------------------------
// K4f wva_ensemble_cost: per ensemble row the fp64 sum of the row's compact
// fp32 costs, servers in ascending index from +0.0 (a server without a winner
// holds 0 and is simply added). One lane per row: the n_srv adds of a row
// depend on each other, the rows do not.
// ---------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(WVA_WAVE) wva_ensemble_cost(
    const float *ens_cost, int n_srv, int n_rows, double *row_cost) {
  const int r = (int)blockIdx.x * WVA_WAVE + (int)threadIdx.x;
  if (r >= n_rows) return;
  const float *c = ens_cost + (size_t)r * (size_t)n_srv;
  double sum = 0.0;
  for (int v = 0; v < n_srv; ++v) sum += (double)c[v];
  row_cost[r] = sum;
}

// ---------------------------------------------------------------------------
// K4g wva_ensemble_bands: the order statistics of a forecast ensemble across
// its n_paths <= WVA_ENS_MAX_PATHS paths, one wave per item, grid
// n_steps * (n_srv + n_acc + 3):
//   server item (tick s, server v): the n_q ranks among the paths' winner
//     replicas -> srv_reps_q[n_q][n_steps][n_srv], the same among their costs
//     (compared as floats) -> srv_cost_q, and the most frequent winner code
//     with the number of paths that chose it (smallest code on ties) ->
//     mode[n_steps][n_srv], mode_paths;
//   fleet item (tick s, column c): the n_q ranks among the paths' values of
//     column c < n_acc of the replica totals, n_acc the servers without a
//     winner, n_acc + 1 the accelerator changes (64-bit integer keys), n_acc +
//     2 the row cost (a double key) -> fleet_q[n_q][n_steps][n_acc + 3] 8-byte
//     words, the last column holding doubles.
// Path e's value of tick s is in ensemble row e * n_steps + s.
//
// Selection is rank by counting (wva_ens_select, the one body of every use):
// the wave copies its keys, up to four per lane, into its LDS slice; every
// lane then counts, for each of its keys, the keys that are smaller, or equal
// with a lower path index, reading the same LDS word as the other lanes in
// each step (a broadcast); the count is the key's unique rank, and the key
// whose rank is requested is stored as that quantile. At most n_paths *
// ceil(n_paths / 64) compares per lane. The mode counts equal codes with the
// same loop and takes the (largest count, smallest code) over the wave with
// shuffles, so it does not depend on how many accelerators there are.
//
// One-wave blocks, no barrier: a wave's LDS accesses are served in issue order,
// and the s_waitcnt between the key stores and the counting loop completes the
// stores before the first read (the discipline of the one-wave cell function).
// The three key arrays are separate, so no slice is rewritten while it is read.
// ---------------------------------------------------------------------------
#define WVA_ENS_MAX_PATHS 256
#define WVA_ENS_MAX_Q 8
#define WVA_ENS_KEYS (WVA_ENS_MAX_PATHS / WVA_WAVE)  // keys per lane

struct WvaEnsRanks {
  int k[WVA_ENS_MAX_Q];
};

// cnt[t] = the rank of this lane's key t (path lane + 64 t) among the n keys
// in lds, ties by path index
template <typename K>
__device__ __forceinline__ void wva_ens_rank(const K (&mine)[WVA_ENS_KEYS], K *lds, int n,
                                             int lane, int (&cnt)[WVA_ENS_KEYS]) {
#pragma unroll
  for (int t = 0; t < WVA_ENS_KEYS; ++t) {
    const int e = lane + t * WVA_WAVE;
    if (e < n) lds[e] = mine[t];
    cnt[t] = 0;
  }
  __builtin_amdgcn_s_waitcnt(0);  // one wave: the stores above before the reads below
  for (int j = 0; j < n; ++j) {
    const K kj = lds[j];
#pragma unroll
    for (int t = 0; t < WVA_ENS_KEYS; ++t) {
      const int e = lane + t * WVA_WAVE;
      cnt[t] += (kj < mine[t] || (kj == mine[t] && j < e)) ? 1 : 0;
    }
  }
}

// out[q * stride] = the key of rank ranks.k[q], for every q < n_q
template <typename K, typename O>
__device__ __forceinline__ void wva_ens_select(const K (&mine)[WVA_ENS_KEYS], K *lds, int n,
                                               int lane, const WvaEnsRanks &ranks, int n_q,
                                               O *out, size_t stride) {
  int cnt[WVA_ENS_KEYS];
  wva_ens_rank(mine, lds, n, lane, cnt);
#pragma unroll
  for (int t = 0; t < WVA_ENS_KEYS; ++t) {
    if (lane + t * WVA_WAVE >= n) continue;
    for (int q = 0; q < n_q; ++q)
      if (ranks.k[q] == cnt[t]) out[(size_t)q * stride] = (O)mine[t];
  }
}

extern "C" __global__ void __launch_bounds__(WVA_WAVE) wva_ensemble_bands(
    const int *ens_code, const int *ens_reps, const float *ens_cost,
    const unsigned long long *ens_tot, const int *ens_nowin, const int *ens_chg,
    const double *row_cost, int n_srv, int n_acc, int n_steps, int n_paths, int n_q,
    WvaEnsRanks ranks, int *srv_reps_q, float *srv_cost_q, int *mode, int *mode_paths,
    long long *fleet_q) {
  __shared__ long long lds_i[WVA_ENS_MAX_PATHS];
  __shared__ double lds_d[WVA_ENS_MAX_PATHS];
  __shared__ int lds_c[WVA_ENS_MAX_PATHS];
  const int lane = (int)threadIdx.x;
  const int n_cols = n_acc + 3;
  const int n_srv_items = n_steps * n_srv;
  const int item = (int)blockIdx.x;
  if (n_paths > WVA_ENS_MAX_PATHS || n_q > WVA_ENS_MAX_Q) return;
  if (item >= n_srv_items + n_steps * n_cols) return;
  if (item < n_srv_items) {
    const int s = item / n_srv, v = item - s * n_srv;
    long long kr[WVA_ENS_KEYS];
    double kc[WVA_ENS_KEYS];
    int code[WVA_ENS_KEYS];
#pragma unroll
    for (int t = 0; t < WVA_ENS_KEYS; ++t) {
      const int e = lane + t * WVA_WAVE;
      const size_t r = ((size_t)(e < n_paths ? e : 0) * (size_t)n_steps + (size_t)s) *
                           (size_t)n_srv + (size_t)v;
      kr[t] = (long long)ens_reps[r];
      kc[t] = (double)ens_cost[r];  // exact, and ordered as the floats are
      code[t] = ens_code[r];
    }
    const size_t o = (size_t)s * (size_t)n_srv + (size_t)v;
    const size_t stride = (size_t)n_steps * (size_t)n_srv;
    wva_ens_select(kr, lds_i, n_paths, lane, ranks, n_q, srv_reps_q + o, stride);
    wva_ens_select(kc, lds_d, n_paths, lane, ranks, n_q, srv_cost_q + o, stride);
    // mode: every path counts the paths that hold its code
    int cnt[WVA_ENS_KEYS];
#pragma unroll
    for (int t = 0; t < WVA_ENS_KEYS; ++t) {
      const int e = lane + t * WVA_WAVE;
      if (e < n_paths) lds_c[e] = code[t];
      cnt[t] = 0;
    }
    __builtin_amdgcn_s_waitcnt(0);  // one wave: the stores above before the reads below
    for (int j = 0; j < n_paths; ++j) {
      const int cj = lds_c[j];
#pragma unroll
      for (int t = 0; t < WVA_ENS_KEYS; ++t) cnt[t] += (cj == code[t]) ? 1 : 0;
    }
    int best_n = 0, best_c = 0x7fffffff;
#pragma unroll
    for (int t = 0; t < WVA_ENS_KEYS; ++t) {
      if (lane + t * WVA_WAVE >= n_paths) continue;
      if (cnt[t] > best_n || (cnt[t] == best_n && code[t] < best_c)) {
        best_n = cnt[t];
        best_c = code[t];
      }
    }
    for (int off = WVA_WAVE / 2; off > 0; off >>= 1) {
      const int on = __shfl_xor(best_n, off, WVA_WAVE);
      const int oc = __shfl_xor(best_c, off, WVA_WAVE);
      if (on > best_n || (on == best_n && oc < best_c)) {
        best_n = on;
        best_c = oc;
      }
    }
    if (lane == 0) {
      mode[o] = best_c;
      mode_paths[o] = best_n;
    }
    return;
  }
  const int f = item - n_srv_items;
  const int s = f / n_cols, col = f - s * n_cols;
  long long *out = fleet_q + (size_t)s * (size_t)n_cols + (size_t)col;
  const size_t stride = (size_t)n_steps * (size_t)n_cols;
  if (col == n_acc + 2) {
    double kc[WVA_ENS_KEYS];
#pragma unroll
    for (int t = 0; t < WVA_ENS_KEYS; ++t) {
      const int e = lane + t * WVA_WAVE;
      kc[t] = row_cost[(size_t)(e < n_paths ? e : 0) * (size_t)n_steps + (size_t)s];
    }
    wva_ens_select(kc, lds_d, n_paths, lane, ranks, n_q, (double *)out, stride);
    return;
  }
  long long ki[WVA_ENS_KEYS];
#pragma unroll
  for (int t = 0; t < WVA_ENS_KEYS; ++t) {
    const int e = lane + t * WVA_WAVE;
    const size_t r = (size_t)(e < n_paths ? e : 0) * (size_t)n_steps + (size_t)s;
    ki[t] = col < n_acc      ? (long long)ens_tot[r * (size_t)n_acc + (size_t)col]
            : col == n_acc   ? (long long)ens_nowin[r]
                             : (long long)ens_chg[r];
  }
  wva_ens_select(ki, lds_i, n_paths, lane, ranks, n_q, out, stride);
}

// ---------------------------------------------------------------------------
// K4d wva_hold_reduce: the server records of a hold analysis; it takes
// wva_plan_reduce's place. Nothing is minimised: per (server, scenario) at most
// one cell of the server's segment carries the held flag (the host expands one
// accelerator per server and scenario), and that cell's slice is the server's
// record. Should a broken caller flag several, the lowest cell index is taken.
// A server without a flagged cell (no cells at all included) gets the NOT_HELD
// record: status 3, accelerator -1, held 0, needed -1, floats 0.
//
// Work split as wva_rollout: `group` lanes (a power of two, 1..64) serve one
// server, 64 / group servers share a one-wave block, grid (blocks, n_scen);
// lane `sub` of a group looks at cells beg + sub, beg + sub + group, ... The
// group agrees on the held cell by a minimum over its lanes, the lane that
// found it writes hf[n_scen][6][n_srv] (itl, ttft, rho, rate, slo_rate, cost)
// and hi[n_scen][4][n_srv] (status, accelerator, held, needed). It also adds 1
// to counts[n_scen][6] at the status and max(needed - held, 0), where needed
// >= 0, to deficit[n_scen][n_acc] at the accelerator: 64-bit integer atomics
// (needed may be 2 147 483 000 per server, and integer adds make the sums
// independent of execution order); both arrays must be zero on entry. No
// barrier, no LDS.
// ---------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(WVA_WAVE) wva_hold_reduce(
    const uint8_t *status, const uint8_t *held_flag, const int *cell_acc, const int *held,
    const int *needed, const float *cost, const float *slo_rate, const float *itl,
    const float *ttft, const float *rho, const float *rate, const int *seg_start, int n_srv,
    int n_cells, int n_scen, int n_acc, int group, float *hf, int *hi, unsigned long long *counts,
    unsigned long long *deficit) {
  const int lane = (int)threadIdx.x;
  const int sub = lane & (group - 1);
  const int srv = (int)blockIdx.x * (WVA_WAVE / group) + lane / group;
  const int sc = (int)blockIdx.y;
  if (sc >= n_scen) return;  // whole block
  // lanes past the last server keep an empty segment and store nothing, but
  // take part in the shuffles below
  const bool live = srv < n_srv;
  const int beg = live ? seg_start[srv] : 0;
  const int end = live ? seg_start[srv + 1] : 0;
  const size_t base = (size_t)sc * (size_t)n_cells;
  const int none = 0x7fffffff;
  int mine = none;
  for (int i = beg + sub; i < end; i += group)
    if (held_flag[base + (size_t)i] != 0 && i < mine) mine = i;
  int w = mine;
  for (int off = group >> 1; off > 0; off >>= 1) {
    const int o = __shfl_xor(w, off, group);
    w = o < w ? o : w;
  }
  if (!live) return;
  float *gf = hf + (size_t)sc * 6 * (size_t)n_srv;
  int *gi = hi + (size_t)sc * 4 * (size_t)n_srv;
  unsigned long long *cnt = counts + (size_t)sc * WVA_HOLD_STATUSES;
  if (w == none) {
    if (sub != 0) return;
    for (int r = 0; r < 6; ++r) gf[r * n_srv + srv] = 0.0f;
    gi[0 * n_srv + srv] = WVA_HOLD_NOT_HELD;
    gi[1 * n_srv + srv] = -1;
    gi[2 * n_srv + srv] = 0;
    gi[3 * n_srv + srv] = -1;
    atomicAdd(cnt + WVA_HOLD_NOT_HELD, 1ull);
    return;
  }
  if (mine != w) return;
  const size_t o = base + (size_t)w;
  int st = (int)status[o];
  if (st < 0 || st >= WVA_HOLD_STATUSES) st = WVA_HOLD_INVALID;  // keeps the add in counts[]
  const int acc = cell_acc[w];
  const int reps = held[o];
  const int need = needed[o];
  gf[0 * n_srv + srv] = itl[o];
  gf[1 * n_srv + srv] = ttft[o];
  gf[2 * n_srv + srv] = rho[o];
  gf[3 * n_srv + srv] = rate[o];
  gf[4 * n_srv + srv] = slo_rate[o];
  gf[5 * n_srv + srv] = cost[o];
  gi[0 * n_srv + srv] = st;
  gi[1 * n_srv + srv] = acc;
  gi[2 * n_srv + srv] = reps;
  gi[3 * n_srv + srv] = need;
  atomicAdd(cnt + st, 1ull);
  if (need >= 0 && need > reps && acc >= 0 && acc < n_acc)
    atomicAdd(deficit + (size_t)sc * (size_t)n_acc + (size_t)acc,
              (unsigned long long)(need - reps));
}

// ---------------------------------------------------------------------------
// K4b wva_winner: the reconcile tick's winner step in one launch, one wave
// per server: wva_argmin's selection followed by the winner record, i.e.
// wva_plan_reduce on a single scenario without the totals. rec is the
// 10 x n_srv winner block (six fp32 rows, then four int32 rows); winner[srv]
// gets the winning cell index as wva_argmin leaves it.
// ---------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(WVA_WAVE) wva_winner(
    const float *value, const uint8_t *feasible, const uint8_t *zero_empty, const int *cell_acc,
    const int *num_replicas, const int *batch, const float *cost, const float *itl,
    const float *ttft, const float *rho, const float *max_rate, const int *seg_start, int n_srv,
    void *rec, int *winner) {
  const int srv = blockIdx.x;
  if (srv >= n_srv) return;
  int acc, reps;
  const int w = wva_winner_record(value, feasible, zero_empty, cell_acc, num_replicas, batch, cost,
                                  itl, ttft, rho, max_rate, seg_start, n_srv, 0, srv,
                                  (float *)rec, (int *)rec + (size_t)6 * (size_t)n_srv, acc, reps,
                                  (int)threadIdx.x);
  if (threadIdx.x == 0) winner[srv] = w;
}

// ---------------------------------------------------------------------------
// K6 wva_tick_t: the reconcile tick's sweep AND winner step in one launch.
// 256 threads; block b takes task tasks[task0 + b] of the context's task table
// (wva_ctx_set_buckets builds it), four int32 words:
//   wide   {cell, WVA_TASK_WIDE, -, -}: one cell on the whole block, the
//          NT = 256 cell function in the whole of dynamic LDS (large, XL);
//   narrow {c0, c1, c2, c3}: wave w runs the NT = 64 cell function on cell cw
//          in its own LDS slice (base + w * narrow_stride doubles); -1 = empty
//          slot, that wave does nothing. The one-wave cell function executes
//          no barrier (see the reductions, dual_bisect and the geometry
//          build), so the four waves never wait for each other and may leave
//          at different times.
// NT is the bucket kernels' NT for the same cell, so the reduction order, the
// memo key and every output bit are theirs.
//
// Winner step, last-arriver form. Every cell arrives exactly once per tick at
// done[server of the cell]: after the cell function has returned, by whichever
// exit, the lane that stored the outputs (the cell's thread 0, the only lane
// that stores any) drains its stores, releases at agent scope and adds 1 to
// the counter. The arriver that draws segment length - 1 knows every cell of
// the server has released its outputs: its wave acquires at agent scope,
// writes the server's winner record (wva_winner_record, as K4b) and puts the
// counter back to 0. Nobody polls or waits on a counter, so nothing here
// depends on which blocks are resident or in what order they run; the
// counters also work across two launches of this kernel in one tick.
//
// The acquire is required even though the arriver has not read these outputs
// before: sixteen cells share a 64-byte line of every output array, so this
// CU's L1 can hold a line that a neighbouring server's winner step read
// earlier in the launch, from before this server's cells stored into it. The
// winner's loads of the outputs are plain VECTOR loads behind that acquire:
// the output pointers carry no const __restrict__ here, which would let the
// compiler move them to the scalar cache that the acquire does not cover.
//
// Invariant: after a completed tick every done[] word is 0 (each server's
// last arriver resets it). The host zeroes the array at creation, whenever the
// task table changes and after a failed tick, never per tick.
//
// Register budget. MINW is the kernel's launch bound in waves per SIMD, which
// for these four-wave blocks is blocks per CU. At 4 (128 VGPRs) the kernel
// spills 216 B/lane, which costs a flagship launch 7.5 us whatever its tasks
// are; at WVA_TICK_WIDE_WAVES = 2 it takes 192 VGPRs and no scratch.
// A launch whose dynamic LDS lets at most two blocks onto a CU anyway (an XL
// cell: 69 952 B on the flagship) loses nothing to the wider budget, so the
// host picks the instantiation per launch from the launch's LDS size
// (wva_tick_waves in wva_ctx.inc); every other launch keeps four blocks per CU.
// ---------------------------------------------------------------------------
#define WVA_TASK_WIDE (-2)
#define WVA_TICK_NT 256
#define WVA_TICK_MAX_WAVES 4
#ifndef WVA_TICK_WIDE_WAVES
#define WVA_TICK_WIDE_WAVES 2
#endif

template <int MINW>
__global__ void __launch_bounds__(WVA_TICK_NT, MINW)
    wva_tick_t(WvaCellsIn in, WvaCellsOut out, const int4 *tasks, int task0, int n_tasks,
               int narrow_stride, int analyzer_mode, float cv2, WvaMemoRec *memo,
               unsigned *memo_cnt, const int *cell_server, unsigned *done, const int *seg_start,
               const int *cell_acc, int n_srv, void *rec, int *winner) {
  extern __shared__ double smem[];
  if ((int)blockIdx.x >= n_tasks) return;
  const int4 task = tasks[task0 + (int)blockIdx.x];
  const int lane = (int)threadIdx.x & (WVA_WAVE - 1);
  int cell;
  if (task.y == WVA_TASK_WIDE) {  // block-uniform
    cell = task.x;
    wva_cell_body<WVA_TICK_NT, false, WVA_MODE_SWEEP>(in, out, cell, (int)threadIdx.x, smem, 0, 0,
                                                      analyzer_mode, cv2, nullptr, nullptr, memo,
                                                      memo_cnt, WvaNoPlan{});
    // the cell's thread 0 is in wave 0: that wave arrives, the others are done
    if ((int)threadIdx.x >= WVA_WAVE) return;
  } else {
    const int w = (int)threadIdx.x / WVA_WAVE;  // wave-uniform
    cell = w == 0 ? task.x : w == 1 ? task.y : w == 2 ? task.z : task.w;
    if (cell < 0) return;
    wva_cell_body<WVA_WAVE, false, WVA_MODE_SWEEP>(in, out, cell, lane, smem + w * narrow_stride, 0,
                                                   0, analyzer_mode, cv2, nullptr, nullptr, memo,
                                                   memo_cnt, WvaNoPlan{});
  }
  // ---- arrival: one wave per cell from here on, lane 0 stored the outputs
  const int srv = cell_server[cell];
  unsigned old = 0u;
  if (lane == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    // kept, in this order: the fence's own wait is not guaranteed
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    old = __hip_atomic_fetch_add(done + srv, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  old = __shfl(old, 0, WVA_WAVE);
  const unsigned seg_len = (unsigned)(seg_start[srv + 1] - seg_start[srv]);
  if (old + 1u != seg_len) return;  // wave-uniform: not the server's last cell
  // ---- last arriver: the server's winner step
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  int acc, reps;
  const int win = wva_winner_record(out.value, out.feasible, out.zero_empty, cell_acc,
                                    out.num_replicas, out.batch, out.cost, out.itl, out.ttft,
                                    out.rho, out.max_rate, seg_start, n_srv, 0, srv, (float *)rec,
                                    (int *)rec + (size_t)6 * (size_t)n_srv, acc, reps, lane);
  if (lane == 0) {
    winner[srv] = win;
    __hip_atomic_store(done + srv, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---------------------------------------------------------------------------
// K5 wva_plan_greedy: the capacity-limited ("limited mode") solution of every
// scenario of a planning sweep, one wave per scenario. The reference for every
// detail is ops/native/greedy.cpp; docs/design/kernels.md ("Capacity-limited
// planning") explains the formulation. In short: every server has at most one
// live entry, the host's sorted list is the total order (priority asc, delta
// desc, value desc, stamp asc), "pop front" is a wave-wide argmin over the
// live servers, and leftmost re-insertion among equal keys is a stamp of minus
// the running pop counter (initial stamps are the server index, >= 0).
// Server srv belongs to lane srv % 64: that lane sorts its candidates, keeps
// the front entry among its servers in registers, and performs the pop when
// the wave-wide reduction picks one of them. The best-effort policies run on
// lane 0; the winner records are spread over the lanes.
//
// Per-scenario state. Hot (read or written by every pop): per server delta,
// cnt, cur, stamp, live, priority, segment start, current value, granted cell
// and replicas; per sorted candidate position its cell, type, value and
// replicas * units. It lives in dynamic LDS when use_lds is set (the host
// sets it when wva_greedy_lds_bytes() fits its budget) and otherwise in the
// scenario's rows of the global workspace, in the same layout: wsd
// [n_srv + n_cells] 8-byte words, wsi [15 * n_srv + 3 * n_cells] int32. Cold,
// always in the tail of the wsi row: the fall-out list and the five ticket
// fields. capacity [n_scen][n_types] is consumed in place (through an LDS
// copy when n_types <= WVA_GREEDY_LDS_TYPES) and holds the capacity left on
// exit.
// px [n_scen][2][n_srv]: the granted cell's pre-cut replica count, and the
// server's number of feasible candidates that are not zero-load.
// ---------------------------------------------------------------------------
#define WVA_GREEDY_LDS_TYPES 256
#define WVA_GREEDY_MAXF32 3.4028234663852886e38

struct WvaGreedyScen {
  const float *val;          // scenario slice, [n_cells]
  const uint8_t *zero_empty;
  const int *reps;
  const int *seg_start;
  const int *cell_type;
  const int *cell_units;
  const int *order;
  const int *cnt;
  int *cap;
  int *win_cell;
  int *win_rep;
};

// (priority asc, delta desc, value desc, stamp asc); doubles compare as
// doubles, so -0.0 == 0.0 as on the host
__device__ __forceinline__ bool wva_greedy_before(int pa, double da, double va, int sa, int pb,
                                                  double db, double vb, int sb) {
  if (pa != pb) return pa < pb;
  if (da != db) return da > db;
  if (va != vb) return va > vb;
  return sa < sb;
}

__device__ __forceinline__ int wva_greedy_type(const WvaGreedyScen &g, int cell) {
  return g.zero_empty[cell] ? -1 : g.cell_type[cell];
}

// greedy.cpp allocate_maximally
__device__ void wva_greedy_maximally(const WvaGreedyScen &g, const int *list, int n) {
  for (int j = 0; j < n; ++j) {
    const int srv = list[j];
    const int beg = g.seg_start[srv];
    const int len = g.cnt[srv];
    for (int i = 0; i < len; ++i) {
      const int cell = g.order[beg + i];
      const int t = wva_greedy_type(g, cell);
      if (t < 0) continue;
      const int u = g.cell_units[cell];
      if (u <= 0) continue;
      int max_rep = g.cap[t] / u;
      if (max_rep > g.reps[cell]) max_rep = g.reps[cell];
      if (max_rep > 0) {
        g.win_cell[srv] = cell;
        g.win_rep[srv] = max_rep;
        g.cap[t] -= max_rep * u;
        break;
      }
    }
  }
}

// greedy.cpp allocate_equally. Ticket state: 0 dead, 1 live, 2 live and
// active. Every step on a live ticket either takes at least one capacity unit
// or kills the ticket, so the live steps are bounded by the capacity units
// left plus twice the list length; max_pass bounds the passes the same way.
__device__ void wva_greedy_equally(const WvaGreedyScen &g, const int *list, int n, int *tk_state,
                                   int *tk_type, int *tk_units, int *tk_granted, int *tk_cand,
                                   int n_types) {
  long long max_pass = (long long)n + 1;
  for (int t = 0; t < n_types; ++t) max_pass += (long long)g.cap[t];
  for (int j = 0; j < n; ++j) {
    tk_state[j] = 1;
    tk_granted[j] = 0;
    tk_cand[j] = -1;
  }
  int live = n;
  for (long long pass = 0; live > 0 && pass < max_pass; ++pass) {
    for (int j = 0; j < n; ++j) {
      int st = tk_state[j];
      if (st == 0) continue;
      if (st == 1) {
        const int srv = list[j];
        const int beg = g.seg_start[srv];
        const int len = g.cnt[srv];
        for (int i = 0; i < len; ++i) {
          const int cell = g.order[beg + i];
          const int t = wva_greedy_type(g, cell);
          if (t < 0) continue;
          const int u = g.cell_units[cell];
          if (u > 0 && g.cap[t] >= u) {
            st = 2;
            tk_state[j] = 2;
            tk_type[j] = t;
            tk_units[j] = u;
            tk_cand[j] = cell;
            break;
          }
        }
        if (st != 2) {
          tk_state[j] = 0;
          --live;
          continue;
        }
      }
      const int t = tk_type[j], u = tk_units[j];
      const int avail_rep = g.cap[t] / u;
      const int want = g.reps[tk_cand[j]];
      if ((avail_rep < want ? avail_rep : want) > 0) {
        tk_granted[j] += 1;
        g.cap[t] -= u;
      } else {
        tk_state[j] = 0;
        --live;
      }
    }
  }
  for (int j = 0; j < n; ++j) {
    if (tk_granted[j] > 0) {
      g.win_cell[list[j]] = tk_cand[j];
      g.win_rep[list[j]] = tk_granted[j];
    }
  }
}

// greedy.cpp best_effort; policy: 0 None, 1 PriorityExhaustive,
// 2 PriorityRoundRobin, 3 RoundRobin
__device__ void wva_greedy_best_effort(const WvaGreedyScen &g, const int *list, int n, int policy,
                                       const int *srv_prio, int *tk_state, int *tk_type,
                                       int *tk_units, int *tk_granted, int *tk_cand, int n_types) {
  if (policy == 1) {
    wva_greedy_maximally(g, list, n);
  } else if (policy == 2) {
    int i = 0;
    while (i < n) {
      int j = i + 1;
      const int prio = srv_prio[list[i]];
      while (j < n && srv_prio[list[j]] == prio) ++j;
      wva_greedy_equally(g, list + i, j - i, tk_state, tk_type, tk_units, tk_granted, tk_cand,
                         n_types);
      i = j;
    }
  } else if (policy == 3) {
    wva_greedy_equally(g, list, n, tk_state, tk_type, tk_units, tk_granted, tk_cand, n_types);
  }
}

// bytes of dynamic LDS the per-scenario state takes (0 = keep it in the
// global workspace): 8-byte arrays first, then the 4-byte ones
static size_t wva_greedy_lds_bytes(int n_srv, int n_cells) {
  return ((size_t)n_srv + (size_t)n_cells) * 8 + ((size_t)9 * n_srv + (size_t)3 * n_cells) * 4;
}

// LDS = true: the hot state is the dynamic LDS block (the pointers below are
// then LDS pointers at compile time); false: the global workspace rows
template <bool LDS>
__device__ __forceinline__ void wva_plan_greedy_body(
    const float *value, const uint8_t *feasible, const uint8_t *zero_empty, const int *cell_acc,
    const int *num_replicas, const int *batch, const float *cost, const float *itl,
    const float *ttft, const float *rho, const float *max_rate, const int *seg_start,
    const int *cell_type, const int *cell_units, const int *srv_prio, int n_srv, int n_cells,
    int n_acc, int n_types, int delayed, int policy, int *capacity, int *wsi, double *wsd,
    float *pf, int *pi, int *px, unsigned long long *totals, int *s_cap) {
  extern __shared__ double wva_greedy_lds[];
  const int sc = blockIdx.x;
  const int lane = threadIdx.x;
  const size_t base = (size_t)sc * (size_t)n_cells;
  const float *val = value + base;
  const uint8_t *feas = feasible + base;
  int *gcap = capacity + (size_t)sc * (size_t)n_types;
  float *gf = pf + (size_t)sc * 6 * (size_t)n_srv;
  int *gi = pi + (size_t)sc * 4 * (size_t)n_srv;
  int *gx = px + (size_t)sc * 2 * (size_t)n_srv;
  // Hot state: the same layout in dynamic LDS (use_lds) or in the scenario's
  // rows of the global workspace; the code below does not care which.
  double *hd;
  if constexpr (LDS) hd = wva_greedy_lds;
  else hd = wsd + (size_t)sc * ((size_t)n_srv + (size_t)n_cells);
  double *delta = hd;                                // [n_srv]
  long long *scount = (long long *)(delta + n_srv);  // [n_cells] replicas * units, sorted order
  int *hi;
  if constexpr (LDS) hi = (int *)(scount + n_cells);
  else hi = wsi + (size_t)sc * ((size_t)15 * n_srv + (size_t)3 * n_cells);
  int *order = hi;                      // [n_cells] cell of sorted candidate position
  int *stype = order + n_cells;         // [n_cells] its type, -1 = zero-load
  float *sval = (float *)(stype + n_cells);  // [n_cells] its value
  int *cnt = (int *)(sval + n_cells);   // per server: candidates
  int *cur = cnt + n_srv;               //   current candidate
  int *stamp = cur + n_srv;             //   tie-break stamp
  int *live = stamp + n_srv;            //   entry still in the list
  int *sprio = live + n_srv;            //   priority
  int *sbeg = sprio + n_srv;            //   segment start
  float *curval = (float *)(sbeg + n_srv);  // current candidate's value
  int *win_cell = (int *)(curval + n_srv);  // granted cell, -1 = none
  int *win_rep = win_cell + n_srv;      //   granted replicas, -1 = the cell's own count
  // cold state, always global: fall-out list and tickets
  int *fall = wsi + (size_t)sc * ((size_t)15 * n_srv + (size_t)3 * n_cells) +
              (size_t)9 * n_srv + (size_t)3 * n_cells;
  int *tk_state = fall + n_srv;
  int *tk_type = tk_state + n_srv;
  int *tk_units = tk_type + n_srv;
  int *tk_granted = tk_units + n_srv;
  int *tk_cand = tk_granted + n_srv;
  // capacity counters: LDS when they fit, else the scenario's global row
  const bool cap_lds = n_types <= WVA_GREEDY_LDS_TYPES;
  int *cap = cap_lds ? s_cap : gcap;
  if (cap_lds)
    for (int t = lane; t < n_types; t += WVA_WAVE) s_cap[t] = gcap[t];

  WvaGreedyScen g;
  g.val = val;
  g.zero_empty = zero_empty + base;
  g.reps = num_replicas + base;
  g.seg_start = seg_start;
  g.cell_type = cell_type;
  g.cell_units = cell_units;
  g.order = order;
  g.cnt = cnt;
  g.cap = cap;
  g.win_cell = win_cell;
  g.win_rep = win_rep;

  // 1. per-server candidates: feasible cells by (double)value ascending, ties
  // in cell order (stable insertion sort; segments are short)
  int bound = 0;
  for (int srv = lane; srv < n_srv; srv += WVA_WAVE) {
    const int beg = seg_start[srv], end = seg_start[srv + 1];
    int n = 0, nz = 0;
    for (int i = beg; i < end; ++i) {
      if (!feas[i]) continue;
      const float v = val[i];
      int k = n;
      while (k > 0 && (double)sval[beg + k - 1] > (double)v) {
        order[beg + k] = order[beg + k - 1];
        sval[beg + k] = sval[beg + k - 1];
        --k;
      }
      order[beg + k] = i;
      sval[beg + k] = v;
      ++n;
      if (!g.zero_empty[i]) ++nz;
    }
    for (int k = 0; k < n; ++k) {
      const int cell = order[beg + k];
      stype[beg + k] = wva_greedy_type(g, cell);
      scount[beg + k] = (long long)g.reps[cell] * (long long)cell_units[cell];
    }
    cnt[srv] = n;
    cur[srv] = 0;
    stamp[srv] = srv;
    live[srv] = n > 0 ? 1 : 0;
    sprio[srv] = srv_prio[srv];
    sbeg[srv] = beg;
    curval[srv] = n > 0 ? sval[beg] : 0.0f;
    delta[srv] = n > 1 ? (double)sval[beg + 1] - (double)sval[beg] : WVA_GREEDY_MAXF32;
    win_cell[srv] = -1;
    win_rep[srv] = 0;
    gx[n_srv + srv] = nz;
    bound += n + (n > 0 ? 1 : 0);
  }
#pragma unroll
  for (int off = WVA_WAVE / 2; off > 0; off >>= 1) bound += __shfl_xor(bound, off, WVA_WAVE);
  __syncthreads();

  // 2. pop loop: at most one pop per feasible candidate, bounded by the
  // candidate count plus the entry count whatever the data. Server srv is
  // owned by lane srv % 64: only that lane changes its entry, and it keeps
  // the front entry among the servers it owns in registers, so a pop costs
  // one wave-wide reduction plus a rescan of the owner's servers.
  int lb = -1, lbp = 0, lbs = 0;
  double lbd = 0.0, lbv = 0.0;
  auto rescan = [&]() {
    lb = -1;
#pragma unroll 4
    for (int srv = lane; srv < n_srv; srv += WVA_WAVE) {
      const int lv = live[srv], p = sprio[srv], s = stamp[srv];
      const double d = delta[srv], v = (double)curval[srv];
      if (lv && (lb < 0 || wva_greedy_before(p, d, v, s, lbp, lbd, lbv, lbs))) {
        lb = srv; lbp = p; lbd = d; lbv = v; lbs = s;
      }
    }
  };
  rescan();
  int n_fall = 0, pops = 0, group_prio = 0;
  bool have_group = false;
  for (int it = 0; it < bound; ++it) {
    int b = lb, bp = lbp, bs = lbs;
    double bd = lbd, bv = lbv;
#pragma unroll
    for (int off = WVA_WAVE / 2; off > 0; off >>= 1) {
      const int ob = __shfl_xor(b, off, WVA_WAVE);
      const int op = __shfl_xor(bp, off, WVA_WAVE);
      const int os = __shfl_xor(bs, off, WVA_WAVE);
      const double od = __shfl_xor(bd, off, WVA_WAVE);
      const double ov = __shfl_xor(bv, off, WVA_WAVE);
      if (ob >= 0 && (b < 0 || wva_greedy_before(op, od, ov, os, bp, bd, bv, bs))) {
        b = ob; bp = op; bd = od; bv = ov; bs = os;
      }
    }
    if (b < 0) break;  // uniform: every lane holds the same front entry
    if (!delayed && have_group && bp != group_prio) {
      // the previous priority group is done: its fall-out list goes through
      // best-effort before the first pop of this group
      if (lane == 0)
        wva_greedy_best_effort(g, fall, n_fall, policy, srv_prio, tk_state, tk_type, tk_units,
                               tk_granted, tk_cand, n_types);
      n_fall = 0;
      __syncthreads();
    }
    group_prio = bp;
    have_group = true;
    ++pops;
    const int owner = b & (WVA_WAVE - 1);
    int fell = 0;
    if (lane == owner) {
      const int len = cnt[b];
      int c = cur[b];
      const int pos = sbeg[b] + c;
      const int t = stype[pos];
      if (t < 0) {
        live[b] = 0;  // zero-load empty candidate: the entry is dropped
      } else {
        const long long count = scount[pos];
        if ((long long)cap[t] >= count) {
          cap[t] -= (int)count;
          win_cell[b] = order[pos];
          win_rep[b] = -1;
          live[b] = 0;
        } else {
          c += 1;
          if (c == len) {
            live[b] = 0;
            fall[n_fall] = b;
            fell = 1;
          } else {
            const float nv = sval[pos + 1];
            cur[b] = c;
            curval[b] = nv;
            delta[b] = c + 1 < len ? (double)sval[pos + 2] - (double)nv : WVA_GREEDY_MAXF32;
            stamp[b] = -pops;
          }
        }
      }
      rescan();
    }
    n_fall += __shfl(fell, owner, WVA_WAVE);
    __syncthreads();  // the capacity counters and the fall-out list change hands
  }
  if (lane == 0 && n_fall > 0)
    wva_greedy_best_effort(g, fall, n_fall, policy, srv_prio, tk_state, tk_type, tk_units,
                           tk_granted, tk_cand, n_types);
  __syncthreads();

  // 3. winner records (wva_plan_reduce's layout; cost and value scaled by
  // granted/desired in fp64 and rounded once), replica totals, capacity left
  for (int srv = lane; srv < n_srv; srv += WVA_WAVE) {
    const int w = win_cell[srv];
    const bool has = w >= 0;
    const size_t wc = base + (size_t)(has ? w : 0);
    const int desired = has ? num_replicas[wc] : 0;
    const int granted = has ? (win_rep[srv] < 0 ? desired : win_rep[srv]) : 0;
    float c = has ? cost[wc] : 0.0f;
    float v = has ? value[wc] : 0.0f;
    if (has && desired > 0 && granted != desired) {
      const double f = (double)granted / (double)desired;
      c = (float)((double)c * f);
      v = (float)((double)v * f);
    }
    const int acc = has ? cell_acc[w] : -1;
    gf[0 * n_srv + srv] = c;
    gf[1 * n_srv + srv] = v;
    gf[2 * n_srv + srv] = has ? itl[wc] : 0.0f;
    gf[3 * n_srv + srv] = has ? ttft[wc] : 0.0f;
    gf[4 * n_srv + srv] = has ? rho[wc] : 0.0f;
    gf[5 * n_srv + srv] = has ? max_rate[wc] : 0.0f;
    gi[0 * n_srv + srv] = acc;
    gi[1 * n_srv + srv] = granted;
    gi[2 * n_srv + srv] = has ? batch[wc] : 0;
    gi[3 * n_srv + srv] = w;
    gx[srv] = desired;
    if (acc >= 0 && acc < n_acc && granted > 0)
      atomicAdd(totals + (size_t)sc * (size_t)n_acc + (size_t)acc, (unsigned long long)granted);
  }
  if (cap_lds)
    for (int t = lane; t < n_types; t += WVA_WAVE) gcap[t] = s_cap[t];
}

extern "C" __global__ void __launch_bounds__(WVA_WAVE) wva_plan_greedy(
    const float *value, const uint8_t *feasible, const uint8_t *zero_empty, const int *cell_acc,
    const int *num_replicas, const int *batch, const float *cost, const float *itl,
    const float *ttft, const float *rho, const float *max_rate, const int *seg_start,
    const int *cell_type, const int *cell_units, const int *srv_prio, int n_srv, int n_cells,
    int n_scen, int n_acc, int n_types, int delayed, int policy, int use_lds, int *capacity,
    int *wsi, double *wsd, float *pf, int *pi, int *px, unsigned long long *totals) {
  __shared__ int s_cap[WVA_GREEDY_LDS_TYPES];
  if ((int)blockIdx.x >= n_scen) return;  // whole block
  if (use_lds)
    wva_plan_greedy_body<true>(value, feasible, zero_empty, cell_acc, num_replicas, batch, cost,
                               itl, ttft, rho, max_rate, seg_start, cell_type, cell_units,
                               srv_prio, n_srv, n_cells, n_acc, n_types, delayed, policy,
                               capacity, wsi, wsd, pf, pi, px, totals, s_cap);
  else
    wva_plan_greedy_body<false>(value, feasible, zero_empty, cell_acc, num_replicas, batch, cost,
                                itl, ttft, rho, max_rate, seg_start, cell_type, cell_units,
                                srv_prio, n_srv, n_cells, n_acc, n_types, delayed, policy,
                                capacity, wsi, wsd, pf, pi, px, totals, s_cap);
}

// The native reconcile context (WvaCtx: the per-tick pipeline and the planning
// passes behind the wva_ctx_* C ABI) launches the kernels above; it is host
// code of this translation unit.
#include "wva_ctx.inc"

