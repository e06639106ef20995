// wva_lag.inc — lag analysis: the TRANSIENT distribution of a held cell's
// chain, included by wva_kernels.hip after the steady-state kernels (which it
// does not touch) and before the context runtime.
//
// Every other kernel solves the state-dependent M/M/1/K chain for its
// stationary distribution. Inside an actuation lag that is the wrong question:
// the load has stepped up, the replicas have not, and the finite queue
// (K = 11 N states) fills from where it was at a finite speed. wva_lag_t
// computes p(t) = p(0) exp(Q t) at n_times checkpoints, with p(0) the
// stationary distribution at the rate before the step (lam0) and Q the
// generator at the rate during the lag (lam1); lam1 = 0 (drain) and
// lam1 > s(N) (overload) are ordinary inputs.
//
// Algorithm: uniformization. With Lam = lam1 + max_n s(n), P = I + Q / Lam is
// a non-negative tridiagonal stencil
//   up = lam1 / Lam (0 in state K),  dn(n) = s(min(n, N)) / Lam (0 in state 0),
//   stay(n) = 1 - up - dn(n),
// and over an interval dt, with x = Lam dt,
//   p(t + dt) = sum_k Pois(x; k) p(t) P^k,
// truncated to the Chernoff window [j_lo, j_hi] of chain_wait_tail
// (WVA_TAIL_L = 60: at most 2 e^-60 of the weight is dropped per interval).
// Below j_lo a step only advances the vector, inside the window it also
// accumulates acc += w v with w(k + 1) = w(k) x / (k + 1) from
// exp(wva_pois_log_pmf(j_lo, x)), after j_hi the interval is done and acc is
// the start of the next one (semigroup). Every term is non-negative: nothing
// cancels. An interval takes j_hi steps; the sum over the intervals is
// computed before the first step and compared with max_steps, so every loop
// bound is block-uniform and known up front: no polling, no cross-block
// traffic, no data-dependent exit.
//
// Work split: one block per (held cell, scenario) task — thousands of
// dependent steps each, and the tasks are independent. The host builds the
// task table (only slices that need the device are in it), grouped by
// instantiation and ordered by descending cost within one; a task carries the
// cell's scalars, so the pass reads neither the dynamic block nor anything
// else a reconcile owns, and writes its server's record itself.
//
// State in registers: lane l of wva_lag_t<NT, C, TAB> owns C consecutive states
// as two fully unrolled fp64 register arrays v and acc. The coefficients stay
// and dnr (dn of the right neighbour) are register arrays too in the narrow
// classes; in the widest one they are two uniform constants for the tail
// lanes and an LDS table for the head waves (WvaLagCoef). The states are placed so
// that state K is the LAST state of its lane (pad0 empty states in front of
// state 0): "no birth out of K" is then one per-lane factor on the left halo
// instead of a per-state select, and the padding on both sides stays exactly
// 0 because nothing flows into it. A step is, per state, one multiply and two
// FMAs (three inside the window), plus the two halo values: the left
// neighbour's v[C - 1] and the right neighbour's v[0]. Within a wave they move
// by the DPP wave shifts (gfx950 is a gfx9 part and has them), so a one-wave
// task executes no barrier and touches no LDS per step; across waves the edge
// lanes write to a double-buffered LDS slot, one __syncthreads per step.
//
// p(0) is built in log space: per-lane prefix of log(lam0 / s(n)) over the
// head states, a scan of the lane totals, the geometric tail by
// multiplication, max, exp, one sum. The functionals are one reduction per
// checkpoint, not per step.

#define WVA_LAG_MAX_T 16    // checkpoints per pass
#define WVA_LAG_FUNCS 5     // raw fp64 functionals per checkpoint
#define WVA_LAG_FLOATS 6    // fp32 outputs per checkpoint
#define WVA_LAG_CLASSES 4   // kernel instantiations
#define WVA_LAG_MAX_N 1117  // widest instantiation: 11 N + 1 <= 512 * 24

// One (held cell, scenario) slice. 64 bytes; ops/sweep.py LAG_TASK_DTYPE.
struct WvaLagTask {
  int in_tok, out_tok, N;
  int slot;  // scenario * n_srv + server: where the record goes
  float alpha, beta, gamma, delta;
  float t_ttft, t_itl;  // the server's targets (0: not checked)
  int pad[2];
  double lam0, lam1;  // req/msec per replica before / during the lag
};
static_assert(sizeof(WvaLagTask) == 64, "task record is 64 bytes");

struct WvaLagArgs {
  const WvaLagTask *tasks;  // device
  const double *dt;  // device [n_times]: interval lengths (msec)
  int n_times, n_slots, max_steps;
  float *out_f;       // device [6][n_times][n_slots]: ttft, itl, wait, blocked, rho, in_system
  uint8_t *violated;  // device [n_times][n_slots]
  int *steps;         // device [n_slots]: stencil steps taken, -1 without a model
  double *raw;        // device [tasks][n_times][5] or null: blocked, in_servers, in_system,
                      // tput, wait before any fp32 rounding (the probe)
};

// value of the lane to the left / right within the wave, 0 at the wave's edge
// (wave_shr:1 / wave_shl:1; lanes without a source keep `old` = 0)
__device__ __forceinline__ double wva_lag_from_left(double x) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), 0x138, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), 0x138, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wva_lag_from_right(double x) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), 0x130, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), 0x130, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}

// a block-uniform value the compiler cannot prove uniform (it came through a
// reduction), moved to scalar registers: the step loop keeps its vector
// registers for the state
__device__ __forceinline__ double wva_lag_uniform(double x) {
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(x)),
                          __builtin_amdgcn_readfirstlane(__double2loint(x)));
}

// wva_pois_log_pmf without lgamma, whose library code keeps a stack frame (the
// percentile kernels carry it as scratch): below 16, log i! is a sum of at
// most 14 logs; from 16 on, the saddle-point form as it stands there
__device__ __forceinline__ double wva_lag_pois_log_pmf(double i, double x) {
  if (i >= 16.0) return wva_pois_log_pmf(i, x);
  double log_fact = 0.0;
  for (double m = 2.0; m <= i; m += 1.0) log_fact += log(m);
  return i * log(x) - x - log_fact;
}

// steps of one interval: the window's upper end, and its lower end in *jlo.
// Each operation rounded on its own, in the order the host forms them
// (analyzer/lag.py lag_window), so both sides count the same steps.
__device__ __forceinline__ double wva_lag_window(double x, double *jlo) {
#pragma clang fp contract(off)
  const double a = 2.0 * x * WVA_TAIL_L;
  const double lo = floor(x - sqrt(a));
  *jlo = lo > 0.0 ? lo : 0.0;
  return ceil(x + WVA_TAIL_L / 3.0 + sqrt(WVA_TAIL_L * WVA_TAIL_L / 9.0 + a));
}

// the fp32 latency terms with every operation rounded on its own, as
// PrefillParms.prefill_time / DecodeParms.decode_time round them
__device__ __forceinline__ float wva_lag_prefill(const WvaCell &c, float b) {
#pragma clang fp contract(off)
  if (c.in_tok == 0) return 0.0f;
  const float slope = c.delta * (float)c.in_tok;
  const float var = slope * b;
  return c.gamma + var;
}
__device__ __forceinline__ float wva_lag_decode(const WvaCell &c, float b) {
#pragma clang fp contract(off)
  const float var = c.beta * b;
  return c.alpha + var;
}

// exclusive prefix of x over the block's threads, and the block total
template <int NT>
__device__ __forceinline__ double wva_lag_scan(double x, double *scratch, double *total) {
  constexpr int NW = NT / WVA_WAVE;
  const int lane = threadIdx.x & (WVA_WAVE - 1), wv = threadIdx.x / WVA_WAVE;
  double incl = x;
#pragma unroll
  for (int off = 1; off < WVA_WAVE; off <<= 1) {
    const double o = __shfl_up(incl, off, WVA_WAVE);
    if (lane >= off) incl += o;
  }
  double before = __shfl_up(incl, 1, WVA_WAVE);
  if (lane == 0) before = 0.0;
  if constexpr (NW == 1) {
    *total = __shfl(incl, WVA_WAVE - 1, WVA_WAVE);
  } else {
    __syncthreads();  // the scratch may still be read
    if (lane == WVA_WAVE - 1) scratch[wv] = incl;
    __syncthreads();
    double sum = 0.0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      if (w == wv) before += sum;
      sum += scratch[w];
    }
    *total = sum;
  }
  return before;
}

// Where a lane's stencil coefficients live. Narrow classes (TAB = false) keep
// them in registers: stay[i] and dnr[i] (dn of the right neighbour) per state.
// The widest class holds 24 states per lane, v and acc alone are 96 registers,
// so there (TAB = true) the coefficients follow their structure: they vary only
// in the head n <= N, 1/11 of the states. The waves that hold head states
// ("head waves", at most HL / 64 of them) read their coefficients from an LDS
// table, transposed so that lane t reads word i * HL + t (conflict-free; each
// lane reads only what it wrote, so the table needs no barrier); every other
// wave uses two block-uniform constants and one per-lane value for its last
// state, which differs in the lane that owns state K (no birth out of K).
template <int NT, int C>
constexpr int wva_lag_head_lanes() {
  // lanes of the waves that can hold a state n <= N, N the class' largest
  return (((NT * C - 1) / 11 + C) / (WVA_WAVE * C) + 1) * WVA_WAVE;
}
template <int C, bool TAB, int HL>
struct WvaLagCoef;
template <int C, int HL>
struct WvaLagCoef<C, false, HL> {
  double stay[C], dnr[C];
};
template <int C, int HL>
struct WvaLagCoef<C, true, HL> {
  const double *tab;  // LDS: &table[tid]; stay at i * HL, dnr at (C + i) * HL
  bool head;          // wave-uniform: this wave reads the table
  double stay_t, dn_t;  // tail constants (block-uniform)
  double stay_last;     // stay of the lane's last state in a tail wave
};

// the C states of a lane, given how stay(i) and dnr(i) are read
template <int C, bool ACC, typename S, typename D>
__device__ __forceinline__ void wva_lag_apply(double (&v)[C], double (&acc)[C], double in_left,
                                              double right, double up, double w, S stay, D dnr) {
#pragma unroll
  for (int i = 0; i < C; ++i) {
    const double cur = v[i];
    const double next = i + 1 < C ? v[i + 1] : right;
    const double nv = fma(cur, stay(i), fma(next, dnr(i), in_left));
    v[i] = nv;
    if constexpr (ACC) acc[i] = fma(w, nv, acc[i]);
    in_left = cur * up;
  }
}

// one application of the stencil to the block's vector; with ACC also
// acc += w v on the new vector. `buf` is the halo slot of this step.
template <int NT, int C, bool ACC, bool TAB, int HL>
__device__ __forceinline__ void wva_lag_step(double (&v)[C], double (&acc)[C],
                                             const WvaLagCoef<C, TAB, HL> &k, double up,
                                             double up_left, double w,
                                             double (*halo)[2][NT / WVA_WAVE], int &buf) {
  double left = wva_lag_from_left(v[C - 1]);
  double right = wva_lag_from_right(v[0]);
  if constexpr (NT > WVA_WAVE) {
    constexpr int NW = NT / WVA_WAVE;
    const int lane = threadIdx.x & (WVA_WAVE - 1), wv = threadIdx.x / WVA_WAVE;
    if (lane == WVA_WAVE - 1) halo[buf][0][wv] = v[C - 1];
    if (lane == 0) halo[buf][1][wv] = v[0];
    __syncthreads();
    if (lane == 0 && wv > 0) left = halo[buf][0][wv - 1];
    if (lane == WVA_WAVE - 1 && wv < NW - 1) right = halo[buf][1][wv + 1];
    buf ^= 1;  // the next step writes the other slot: one barrier per step
  }
  const double in_left = left * up_left;
  if constexpr (TAB) {
    if (k.head) {
      wva_lag_apply<C, ACC>(
          v, acc, in_left, right, up, w, [&](int i) { return k.tab[i * HL]; },
          [&](int i) { return k.tab[(C + i) * HL]; });
    } else {
      wva_lag_apply<C, ACC>(
          v, acc, in_left, right, up, w,
          [&](int i) { return i == C - 1 ? k.stay_last : k.stay_t; },
          [&](int) { return k.dn_t; });
    }
  } else {
    wva_lag_apply<C, ACC>(
        v, acc, in_left, right, up, w, [&](int i) { return k.stay[i]; },
        [&](int i) { return k.dnr[i]; });
  }
}

template <int NT, int C, bool TAB>
__global__ void WVA_NO_PK_F32 __launch_bounds__(NT)
    wva_lag_t(WvaLagArgs a, int task0) {
  constexpr int NW = NT / WVA_WAVE;
  constexpr int HL = wva_lag_head_lanes<NT, C>();
  __shared__ double red[64];
  __shared__ double halo[2][2][NW];
  __shared__ double win_w[WVA_LAG_MAX_T];  // per interval: the weight at j_lo,
  __shared__ int win_lo[WVA_LAG_MAX_T];    // j_lo
  __shared__ int win_hi[WVA_LAG_MAX_T];    // and j_hi, its steps
  __shared__ double table[TAB ? 2 * C * HL : 1];
  const int tid = (int)threadIdx.x;
  const int task = task0 + (int)blockIdx.x;
  const WvaLagTask *const tp = a.tasks + task;
  const int n_times = a.n_times, n_slots = a.n_slots, slot = tp->slot;
  const double lam0 = tp->lam0, lam1 = tp->lam1;
  WvaCell c;  // the fields the rate and latency terms read
  c.in_tok = tp->in_tok;
  c.out_tok = tp->out_tok;
  c.N = tp->N;
  c.alpha = tp->alpha;
  c.beta = tp->beta;
  c.gamma = tp->gamma;
  c.delta = tp->delta;
  const int N = c.N, K = 11 * N;
  // the host checked these before the launch (wva_lag_check); uniform
  if (N < 1 || K + 1 > NT * C || slot < 0 || slot >= n_slots || n_times < 1 ||
      n_times > WVA_LAG_MAX_T)
    return;
  const int pad0 = (C - (K + 1) % C) % C;  // state K closes its lane
  const int n_first = tid * C - pad0;       // the state v[0] holds
  const int num_decode = wva_num_decode(c);
// (set-up loops only) finish one unrolled iteration before the next begins:
// the scheduler otherwise interleaves the C logs, exps or divisions of a loop
#define WVA_LAG_SEQ() __builtin_amdgcn_sched_barrier(0)
#define WVA_LAG_VALID(n) ((n) >= 0 && (n) <= K)
#define WVA_LAG_RATE(n) wva_rate_exact(c, num_decode, (n) < 1 ? 1 : ((n) > N ? N : (n)))
// s(min(n, N)) for 1 <= n <= K, else 0
#define WVA_LAG_DEATH(n) ((n) >= 1 && (n) <= K ? (double)WVA_LAG_RATE(n) : 0.0)

  // ---- Lam = lam1 + the largest rate, and the degenerate-rate guard
  bool bad = false;
  float smax_l = 0.0f;
#pragma unroll
  for (int i = 0; i < C; ++i) {
    const int n = n_first + i;
    if (n >= 1 && n <= K) {
      const float r = WVA_LAG_RATE(n);
      bad = bad || !(r > 0.0f) || !isfinite(r);
      smax_l = fmaxf(smax_l, r);
    }
  }
  const double smax =
      wva_lag_uniform(red_max_p<NT, 1>(bad ? (double)INFINITY : (double)smax_l, red));
  const double Lam = lam1 + smax;

  // ---- the window and the steps of every interval, before the first step is
  // taken: thread j has interval j (the Poisson weight costs registers the
  // step loop has none of to spare)
  double mine = 0.0;
  if (tid < n_times) {
    const double x = Lam * a.dt[tid];
    double jlo;
    mine = wva_lag_window(x, &jlo);
    const bool fits = smax < (double)INFINITY && Lam > 0.0 && mine <= (double)a.max_steps;
    win_lo[tid] = fits ? (int)jlo : 0;
    win_hi[tid] = fits ? (int)mine : 0;
    win_w[tid] = fits ? exp(wva_lag_pois_log_pmf(jlo, x)) : 0.0;
  }
  double total = mine, none = 0.0;
  red_sum2_p<NT, 1>(total, none, red);  // integers below 2^53: exact in any order
  total = wva_lag_uniform(total);
  if constexpr (NT == WVA_WAVE) __builtin_amdgcn_wave_barrier();
  const size_t raw0 = (size_t)task * (size_t)n_times * WVA_LAG_FUNCS;
#define WVA_LAG_OUT(f, j) \
  a.out_f[((size_t)(f) * (size_t)n_times + (size_t)(j)) * (size_t)n_slots + (size_t)slot]
  if (!(smax < (double)INFINITY) || !(Lam > 0.0) || !(total <= (double)a.max_steps)) {
    // degenerate rates, or above the step budget: no evaluation (uniform)
    if (tid == 0) {
      a.steps[slot] = smax < (double)INFINITY && total < 2147483000.0 ? (int)total : -1;
      for (int j = 0; j < n_times; ++j) {
        for (int f = 0; f < WVA_LAG_FLOATS; ++f) WVA_LAG_OUT(f, j) = NAN;
        a.violated[(size_t)j * (size_t)n_slots + (size_t)slot] = 0;
        if (a.raw)
          for (int f = 0; f < WVA_LAG_FUNCS; ++f) a.raw[raw0 + (size_t)j * WVA_LAG_FUNCS + f] = NAN;
      }
    }
    return;
  }

  // ---- the stencil's coefficients
  const double sN = (double)wva_rate_exact(c, num_decode, N);
  const double up = lam1 / Lam;
  const double up_left = (n_first - 1 >= 0 && n_first - 1 < K) ? up : 0.0;
  WvaLagCoef<C, TAB, HL> k;
  if constexpr (TAB) {
    // head waves: the waves whose first state is not above N
    const int head_waves = (N + pad0) / (WVA_WAVE * C) + 1;
    k.tab = table + (tid < HL ? tid : 0);
    k.head = __builtin_amdgcn_readfirstlane(tid / WVA_WAVE < head_waves ? 1 : 0) != 0;
    k.dn_t = sN / Lam;
    k.stay_t = fmax(1.0 - up - k.dn_t, 0.0);
    k.stay_last = n_first + C - 1 == K ? fmax(1.0 - k.dn_t, 0.0) : k.stay_t;
    if (head_waves * WVA_WAVE > HL) return;  // cannot happen for an N the class takes; uniform
    if (k.head) {
#pragma unroll
      for (int i = 0; i < C; ++i) {
        const int n = n_first + i;
        const double dn = WVA_LAG_DEATH(n) / Lam;
        table[i * HL + tid] = WVA_LAG_VALID(n) ? fmax(1.0 - (n < K ? up : 0.0) - dn, 0.0) : 0.0;
        table[(C + i) * HL + tid] = WVA_LAG_DEATH(n + 1) / Lam;
        WVA_LAG_SEQ();
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < C; ++i) {
      const int n = n_first + i;
      const double dn = WVA_LAG_DEATH(n) / Lam;
      k.stay[i] = WVA_LAG_VALID(n) ? fmax(1.0 - (n < K ? up : 0.0) - dn, 0.0) : 0.0;
      k.dnr[i] = WVA_LAG_DEATH(n + 1) / Lam;
      WVA_LAG_SEQ();
    }
  }

  // ---- p(0): the stationary distribution at lam0
  double v[C], acc[C];
  if (lam0 > 0.0) {
    const double l0 = log(lam0);
    double run = 0.0;
#pragma unroll
    for (int i = 0; i < C; ++i) {
      const int n = n_first + i;
      if (n >= 1 && n <= N) run += l0 - log((double)WVA_LAG_RATE(n));
      v[i] = run;  // the lane's inclusive prefix of the head terms
      WVA_LAG_SEQ();
    }
    double head;  // log w[N]
    const double before = wva_lag_scan<NT>(run, red, &head);
    const double lr = l0 - log(sN);
    double m = -(double)INFINITY;
#pragma unroll
    for (int i = 0; i < C; ++i) {
      const int n = n_first + i;
      v[i] = !WVA_LAG_VALID(n) ? -(double)INFINITY
             : n <= N  ? before + v[i]
                       : head + (double)(n - N) * lr;
      m = fmax(m, v[i]);
    }
    m = red_max_p<NT, 1>(m, red);
    double sum = 0.0, unused = 0.0;
#pragma unroll
    for (int i = 0; i < C; ++i) {
      v[i] = exp(v[i] - m);
      sum += v[i];
      WVA_LAG_SEQ();
    }
    red_sum2_p<NT, 1>(sum, unused, red);
#pragma unroll
    for (int i = 0; i < C; ++i) {
      v[i] /= sum;
      WVA_LAG_SEQ();
    }
  } else {
#pragma unroll
    for (int i = 0; i < C; ++i) v[i] = n_first + i == 0 ? 1.0 : 0.0;
  }

  // ---- the intervals
  int buf = 0;
  for (int j = 0; j < n_times; ++j) {
    const double x = Lam * a.dt[j];
    const int klo = __builtin_amdgcn_readfirstlane(win_lo[j]);
    const int khi = __builtin_amdgcn_readfirstlane(win_hi[j]);
    for (int s = 0; s < klo; ++s)
      wva_lag_step<NT, C, false, TAB, HL>(v, acc, k, up, up_left, 0.0, halo, buf);
    double w = wva_lag_uniform(win_w[j]);
#pragma unroll
    for (int i = 0; i < C; ++i) acc[i] = w * v[i];
    for (int s = klo + 1; s <= khi; ++s) {
      // w(s) = w(s - 1) x / s with the quotient by two Newton steps on the
      // hardware reciprocal (below an ulp; a full division costs a third of
      // the narrow classes' step)
      const double sd = (double)s;
      double rs = __builtin_amdgcn_rcp(sd);
      rs = fma(fma(-sd, rs, 1.0), rs, rs);
      rs = fma(fma(-sd, rs, 1.0), rs, rs);
      w *= x * rs;
      wva_lag_step<NT, C, true, TAB, HL>(v, acc, k, up, up_left, w, halo, buf);
    }

    // p(t_j) = acc, the start of the next interval; its functionals
    // (the lane's first state through an opaque copy: the per-state factors
    // below are loop-invariant, and hoisted out of the checkpoint loop they
    // would sit in ~70 registers across the step loops)
    int n_base = n_first;
    asm volatile("" : "+v"(n_base));
    double f_blk = 0.0, f_srv = 0.0, f_sys = 0.0, f_tput = 0.0, f_wait = 0.0;
#pragma unroll
    for (int i = 0; i < C; ++i) {
      const int n = n_base + i;
      const double p = acc[i];
      v[i] = p;
      if (WVA_LAG_VALID(n)) {
        f_srv += p * (double)(n < N ? n : N);
        f_sys += p * (double)n;
        if (n >= 1) f_tput += p * (double)WVA_LAG_RATE(n);
        if (n >= N && n < K) f_wait += p * (double)(n - N + 1);
        if (n == K) f_blk = p;
      }
      WVA_LAG_SEQ();
    }
    red_sum2_p<NT, 1>(f_blk, f_srv, red);
    red_sum2_p<NT, 1>(f_sys, f_tput, red);
    double unused = 0.0;
    red_sum2_p<NT, 1>(f_wait, unused, red);
    if (tid == 0) {
      const double wait = f_wait / (1.0 - f_blk) / sN;
      const double serv = f_tput > 0.0 ? f_srv / f_tput : 0.0;
      const double eff =
          effective_concurrency(serv, c.gamma, c.alpha, c.delta, c.beta, c.in_tok, c.out_tok, N);
      const float ttft = (float)wait + wva_lag_prefill(c, (float)eff);
      const float itl = wva_lag_decode(c, (float)eff);
      WVA_LAG_OUT(0, j) = ttft;
      WVA_LAG_OUT(1, j) = itl;
      WVA_LAG_OUT(2, j) = (float)wait;
      WVA_LAG_OUT(3, j) = (float)f_blk;
      WVA_LAG_OUT(4, j) = (float)fmin(fmax(f_srv / (double)N, 0.0), 1.0);
      WVA_LAG_OUT(5, j) = (float)f_sys;
      const float t_ttft = tp->t_ttft, t_itl = tp->t_itl;
      a.violated[(size_t)j * (size_t)n_slots + (size_t)slot] =
          (t_ttft != 0.0f && ttft > t_ttft) || (t_itl != 0.0f && itl > t_itl);
      if (a.raw) {
        double *r = a.raw + raw0 + (size_t)j * WVA_LAG_FUNCS;
        r[0] = f_blk;
        r[1] = f_srv;
        r[2] = f_sys;
        r[3] = f_tput;
        r[4] = wait;
      }
    }
  }
  if (tid == 0) a.steps[slot] = (int)total;
#undef WVA_LAG_SEQ
#undef WVA_LAG_VALID
#undef WVA_LAG_RATE
#undef WVA_LAG_DEATH
#undef WVA_LAG_OUT
}

// ---------------------------------------------------------------------------
// host: the instantiations, widest first (the launch order), and their launch
// ---------------------------------------------------------------------------
static const int wva_lag_class_nt[WVA_LAG_CLASSES] = {512, 256, 64, 64};
static const int wva_lag_class_c[WVA_LAG_CLASSES] = {24, 12, 12, 2};

// the tasks of class `cls` fit it, and every record lands inside the outputs
static int wva_lag_check(const WvaLagTask *tasks, int n, int cls, int n_slots) {
  const int states = wva_lag_class_nt[cls] * wva_lag_class_c[cls];
  for (int i = 0; i < n; ++i) {
    const WvaLagTask &t = tasks[i];
    if (t.N < 1 || t.N > WVA_LAG_MAX_N || 11 * t.N + 1 > states) return -2;
    if (t.slot < 0 || t.slot >= n_slots) return -2;
  }
  return 0;
}

// n tasks of class cls from task0 on
static int wva_lag_dispatch(int cls, int n, int task0, const WvaLagArgs &a, hipStream_t s) {
  if (n <= 0) return 0;
  if (a.n_times < 1 || a.n_times > WVA_LAG_MAX_T || a.n_slots < 1 || a.max_steps < 0) return -2;
  switch (cls) {
    case 0: hipLaunchKernelGGL((wva_lag_t<512, 24, true>), dim3(n), dim3(512), 0, s, a, task0); break;
    case 1: hipLaunchKernelGGL((wva_lag_t<256, 12, false>), dim3(n), dim3(256), 0, s, a, task0); break;
    case 2: hipLaunchKernelGGL((wva_lag_t<64, 12, false>), dim3(n), dim3(64), 0, s, a, task0); break;
    case 3: hipLaunchKernelGGL((wva_lag_t<64, 2, false>), dim3(n), dim3(64), 0, s, a, task0); break;
    default: return -3;
  }
  return (int)hipGetLastError();
}

// One-shot probe for tests and tools: the classes of a task table on one
// stream, into device buffers of the caller. host_tasks is the table the
// caller uploaded to dev_tasks (checked here before anything is launched),
// grouped by class in class order with class_count[] tasks each.
extern "C" int wva_lag_probe_launch(const void *host_tasks, const void *dev_tasks,
                                    const int *class_count, int n_times, const double *dt,
                                    int n_slots, int max_steps, void *stream, float *out_f,
                                    uint8_t *violated, int *steps, double *raw) {
  if (!host_tasks || !dev_tasks || !class_count || !dt || n_times < 1 || n_times > WVA_LAG_MAX_T)
    return -2;
  WvaLagArgs a = {};
  a.tasks = (const WvaLagTask *)dev_tasks;
  a.n_times = n_times;
  a.n_slots = n_slots;
  a.max_steps = max_steps;
  a.dt = dt;
  a.out_f = out_f;
  a.violated = violated;
  a.steps = steps;
  a.raw = raw;
  int at = 0;
  for (int k = 0; k < WVA_LAG_CLASSES; ++k) {
    if (class_count[k] < 0) return -2;
    const int rc = wva_lag_check((const WvaLagTask *)host_tasks + at, class_count[k], k, n_slots);
    if (rc != 0) return rc;
    at += class_count[k];
  }
  at = 0;
  for (int k = 0; k < WVA_LAG_CLASSES; ++k) {
    const int rc = wva_lag_dispatch(k, class_count[k], at, a, (hipStream_t)stream);
    if (rc != 0) return rc;
    at += class_count[k];
  }
  return 0;
}

// ---------------------------------------------------------------------------
// Wide lag: cells above WVA_LAG_MAX_N, whose 11 N + 1 states do not fit one
// block's registers. The chain is cut into tiles and the time axis into
// segments (temporal tiling with overlapped halos): the stencil has dependence
// radius 1 per step, so a block that loads its tile plus T extra slots on each
// side can take up to T steps alone; afterwards exactly those borders are
// wrong and it stores only the S slots it owns. The only synchronisation is
// the kernel boundary: launch l runs segment l of every task that has one.
//
// Slots are numbered g = n + pad0 with wva_lag_t's pad0 (state K closes its
// lane; K + 1 + pad0 is a multiple of C, and so are S and T, so a lane's C
// slots are inside the domain or outside it as one). Tile b loads slots
// [b S - T, b S - T + W), W = NT * C, and owns [b S, (b + 1) S). Per task the
// slab holds v twice (launch l reads copy l & 1 and writes the other:
// neighbours read each other's owned slots) and acc once (owned slots only,
// read and written by the same block). The Poisson weight is carried across
// the segments of a window in a per-task double, double-buffered like v, so
// the weight sequence is wva_lag_t's recurrence.
// ---------------------------------------------------------------------------
#define WVA_LAG_WIDE_MAX_N 32768  // the XL ceiling
#define WVA_LAG_WIDE_NT 512
#define WVA_LAG_WIDE_C 24
#define WVA_LAG_WIDE_HALO 768  // production T; S = W - 2 T (docs/design/kernels.md)
// device bytes of the slabs of one round of wide tasks (3 x 8 x slots each)
#define WVA_LAG_WIDE_SLAB_CAP ((size_t)1 << 30)
#define WVA_LAG_SEG_FIRST 1  // the segment starts its interval
#define WVA_LAG_SEG_LAST 2   // ... ends it: a checkpoint
#define WVA_LAG_SEG_FINAL 4  // ... ends the last one

// per wide task, beside its WvaLagTask; 32 bytes, ops/sweep.py LAG_WIDE_DTYPE
struct WvaLagWideTask {
  double Lam;       // the uniformization rate the host scheduled with
  long long slab;   // first double of the task's slab (filled by wva_lag_wide_plan)
  int tile0, n_tiles;  // its rows of the tile table
  int seg0, n_seg;     // its rows of the segment table
};
// one run of at most T steps inside one interval; 32 bytes, LAG_SEG_DTYPE
struct WvaLagSeg {
  double x;          // Lam dt of the interval
  int first, count;  // steps of the interval taken before, and taken here
  int jlo, jhi;      // the interval's window
  int flags, j;      // WVA_LAG_SEG_*, the interval
};
struct WvaLagTile {
  int task, b;
};
static_assert(sizeof(WvaLagWideTask) == 32 && sizeof(WvaLagSeg) == 32, "32-byte records");

struct WvaLagWideArgs {
  WvaLagArgs a;  // tasks, dt, extents and the outputs, as for wva_lag_t
  const WvaLagWideTask *wide;
  const WvaLagSeg *segs;
  const WvaLagTile *tiles;
  double *slab;    // per task: v[2][G], acc[G], G = K + 1 + pad0
  double *part;    // [tile][5]: a tile's partial functionals
  double *wcarry;  // [task][2]: the Poisson weight between segments
  int *flag;       // [task]: not 0 = no model, the task's launches do nothing
  int stride, halo;  // S, T
};

// wva_lag_step for a tile: the same halo exchange; a head wave reads dn of the
// right neighbour from the LDS table (lane t word i * NT + t) and forms
// stay = max(1 - up - dn, 0) from the dn it read for the state before
template <int NT, int C, bool ACC>
__device__ __forceinline__ void wva_lag_tile_step(double (&v)[C], double (&acc)[C], bool head,
                                                  const double *tab, double dn0, double up,
                                                  double up_last, double up_left, double stay_t,
                                                  double dn_t, double stay_last, double w,
                                                  double (*halo)[2][NT / WVA_WAVE], int &buf) {
  constexpr int NW = NT / WVA_WAVE;
  double left = wva_lag_from_left(v[C - 1]);
  double right = wva_lag_from_right(v[0]);
  const int lane = threadIdx.x & (WVA_WAVE - 1), wv = threadIdx.x / WVA_WAVE;
  if (lane == WVA_WAVE - 1) halo[buf][0][wv] = v[C - 1];
  if (lane == 0) halo[buf][1][wv] = v[0];
  __syncthreads();
  if (lane == 0 && wv > 0) left = halo[buf][0][wv - 1];
  if (lane == WVA_WAVE - 1 && wv < NW - 1) right = halo[buf][1][wv + 1];
  buf ^= 1;  // the next step writes the other slot: one barrier per step
  double in_left = left * up_left;  // a tile's edge lanes at a cut received 0
  if (head) {
    double dn = dn0;
#pragma unroll
    for (int i = 0; i < C; ++i) {
      const double cur = v[i];
      const double next = i + 1 < C ? v[i + 1] : right;
      const double dnr = tab[i * NT];
      const double stay = fmax(1.0 - (i == C - 1 ? up_last : up) - dn, 0.0);
      const double nv = fma(cur, stay, fma(next, dnr, in_left));
      v[i] = nv;
      if constexpr (ACC) acc[i] = fma(w, nv, acc[i]);
      in_left = cur * up;
      dn = dnr;
    }
  } else {
    wva_lag_apply<C, ACC>(
        v, acc, in_left, right, up, w,
        [&](int i) { return i == C - 1 ? stay_last : stay_t; }, [&](int) { return dn_t; });
  }
}

#define WVA_LAG_SEQ() __builtin_amdgcn_sched_barrier(0)
#define WVA_LAG_VALID(n) ((n) >= 0 && (n) <= K)
#define WVA_LAG_RATE(n) wva_rate_exact(c, num_decode, (n) < 1 ? 1 : ((n) > N ? N : (n)))
#define WVA_LAG_DEATH(n) ((n) >= 1 && (n) <= K ? (double)WVA_LAG_RATE(n) : 0.0)
#define WVA_LAG_OUT(f, j) \
  g.a.out_f[((size_t)(f) * (size_t)n_times + (size_t)(j)) * (size_t)n_slots + (size_t)slot]
#define WVA_LAG_CELL(c, tp)  \
  WvaCell c;                 \
  c.in_tok = (tp)->in_tok;   \
  c.out_tok = (tp)->out_tok; \
  c.N = (tp)->N;             \
  c.alpha = (tp)->alpha;     \
  c.beta = (tp)->beta;       \
  c.gamma = (tp)->gamma;     \
  c.delta = (tp)->delta

// One block per (wide task, tile), one segment. The host checked every table
// (wva_lag_wide_plan); all control flow below is block-uniform and comes from
// the segment descriptor.
template <int NT, int C>
__global__ void WVA_NO_PK_F32 __launch_bounds__(NT)
    wva_lag_tile_t(WvaLagWideArgs g, int tile_base, int launch) {
  constexpr int NW = NT / WVA_WAVE;
  extern __shared__ double wva_lag_tab[];  // [C][NT]: dn of the right neighbour (head waves)
  __shared__ double red[64];
  __shared__ double halo[2][2][NW];
  const int tid = (int)threadIdx.x;
  const WvaLagTile tl = g.tiles[tile_base + (int)blockIdx.x];
  const int task = tl.task, b = tl.b;
  if (g.flag[task] != 0) return;
  const WvaLagWideTask wt = g.wide[task];
  if (launch >= wt.n_seg) return;
  const WvaLagSeg sg = g.segs[wt.seg0 + launch];
  const WvaLagTask *const tp = g.a.tasks + task;
  WVA_LAG_CELL(c, tp);
  const int N = c.N, K = 11 * N;
  const int pad0 = (C - (K + 1) % C) % C;
  const int G = K + 1 + pad0;  // slots of the task
  const int S = g.stride, T = g.halo;
  const int g0 = b * S - T + tid * C;  // the slot v[0] holds
  const int n_first = g0 - pad0;
  const bool in_dom = g0 >= 0 && g0 < G;
  const bool owned = in_dom && g0 >= b * S && g0 < (b + 1) * S;
  const int num_decode = wva_num_decode(c);
  const double Lam = wt.Lam, lam1 = tp->lam1;

  // ---- the stencil's coefficients
  const double sN = (double)wva_rate_exact(c, num_decode, N);
  const double up = lam1 / Lam;
  const double up_left = (n_first - 1 >= 0 && n_first - 1 < K) ? up : 0.0;
  const double up_last = n_first + C - 1 == K ? 0.0 : up;
  const double dn_t = sN / Lam;
  const double stay_t = fmax(1.0 - up - dn_t, 0.0);
  const double stay_last = n_first + C - 1 == K ? fmax(1.0 - dn_t, 0.0) : stay_t;
  // head waves: the waves whose first state is not above N (slots in front of
  // state 0 included: nothing may flow into them)
  const int wave_first = b * S - T + (tid / WVA_WAVE) * (WVA_WAVE * C) - pad0;
  const bool head = __builtin_amdgcn_readfirstlane(wave_first <= N ? 1 : 0) != 0;
  const double *const tab = wva_lag_tab + tid;
  double dn0 = 0.0;
  if (head) {
    dn0 = WVA_LAG_DEATH(n_first) / Lam;
#pragma unroll
    for (int i = 0; i < C; ++i) {
      wva_lag_tab[i * NT + tid] = WVA_LAG_DEATH(n_first + i + 1) / Lam;
      WVA_LAG_SEQ();
    }
  }

  // ---- the state: v from the copy this launch reads, acc if the window is open
  const size_t sG = (size_t)G;
  const double *const vin = g.slab + wt.slab + (size_t)(launch & 1) * sG;
  double *const vout = g.slab + wt.slab + (size_t)((launch + 1) & 1) * sG;
  double *const accp = g.slab + wt.slab + 2 * sG;
  const int first = sg.first, count = sg.count, jlo = sg.jlo;
  const bool was_open = first > jlo;                       // acc and w come from before
  const bool opens = first <= jlo && jlo < first + count;  // the window opens in here
  double v[C], acc[C];
#pragma unroll
  for (int i = 0; i < C; i += 2) {
    const double2 t = in_dom ? *(const double2 *)(vin + g0 + i) : make_double2(0.0, 0.0);
    v[i] = t.x;
    v[i + 1] = t.y;
  }
#pragma unroll
  for (int i = 0; i < C; i += 2) {
    const double2 t =
        owned && was_open ? *(const double2 *)(accp + g0 + i) : make_double2(0.0, 0.0);
    acc[i] = t.x;
    acc[i + 1] = t.y;
  }

  // ---- the steps
  const double x = sg.x;
  int plain = jlo - first;
  plain = plain < 0 ? 0 : (plain > count ? count : plain);
  int buf = 0;
  for (int s = 0; s < plain; ++s)
    wva_lag_tile_step<NT, C, false>(v, acc, head, tab, dn0, up, up_last, up_left, stay_t, dn_t,
                                    stay_last, 0.0, halo, buf);
  double w = 0.0;
  if (was_open) w = g.wcarry[2 * task + (launch & 1)];
  if (opens) {
    w = exp(wva_lag_pois_log_pmf((double)jlo, x));
#pragma unroll
    for (int i = 0; i < C; ++i) acc[i] = w * v[i];
  }
  w = wva_lag_uniform(w);
  if (was_open || opens) {
    for (int s = first + plain + 1; s <= first + count; ++s) {
      const double sd = (double)s;
      double rs = __builtin_amdgcn_rcp(sd);
      rs = fma(fma(-sd, rs, 1.0), rs, rs);
      rs = fma(fma(-sd, rs, 1.0), rs, rs);
      w *= x * rs;
      wva_lag_tile_step<NT, C, true>(v, acc, head, tab, dn0, up, up_last, up_left, stay_t, dn_t,
                                     stay_last, w, halo, buf);
    }
    if (b == 0 && tid == 0) g.wcarry[2 * task + ((launch + 1) & 1)] = w;
  }

  // ---- a checkpoint: p(t_j) = acc starts the next interval; the tile's
  // partial functionals over the states it owns
  if (sg.flags & WVA_LAG_SEG_LAST) {
    int n_base = n_first;
    asm volatile("" : "+v"(n_base));
    double f_blk = 0.0, f_srv = 0.0, f_sys = 0.0, f_tput = 0.0, f_wait = 0.0;
#pragma unroll
    for (int i = 0; i < C; ++i) {
      const int n = n_base + i;
      const double p = acc[i];
      v[i] = p;
      if (owned && WVA_LAG_VALID(n)) {
        f_srv += p * (double)(n < N ? n : N);
        f_sys += p * (double)n;
        if (n >= 1) f_tput += p * (double)WVA_LAG_RATE(n);
        if (n >= N && n < K) f_wait += p * (double)(n - N + 1);
        if (n == K) f_blk = p;
      }
      WVA_LAG_SEQ();
    }
    red_sum2_p<NT, 1>(f_blk, f_srv, red);
    red_sum2_p<NT, 1>(f_sys, f_tput, red);
    double unused = 0.0;
    red_sum2_p<NT, 1>(f_wait, unused, red);
    if (tid == 0) {
      double *p = g.part + (size_t)(tile_base + (int)blockIdx.x) * WVA_LAG_FUNCS;
      p[0] = f_blk;
      p[1] = f_srv;
      p[2] = f_sys;
      p[3] = f_tput;
      p[4] = f_wait;
    }
  } else if (owned && (was_open || opens)) {
#pragma unroll
    for (int i = 0; i < C; i += 2) *(double2 *)(accp + g0 + i) = make_double2(acc[i], acc[i + 1]);
  }
  if (owned) {
#pragma unroll
    for (int i = 0; i < C; i += 2) *(double2 *)(vout + g0 + i) = make_double2(v[i], v[i + 1]);
  }
}

// One block per wide task: Lam against the host's, then p(0) at lam0 into copy
// 0 of the task's v, in log space as stationary() builds it.
__global__ void __launch_bounds__(WVA_LAG_WIDE_NT)
    wva_lag_wide_init(WvaLagWideArgs g, int task0) {
  constexpr int NT = WVA_LAG_WIDE_NT, C = WVA_LAG_WIDE_C;
  __shared__ double red[64];
  const int tid = (int)threadIdx.x;
  const int task = task0 + (int)blockIdx.x;
  const WvaLagTask *const tp = g.a.tasks + task;
  const WvaLagWideTask wt = g.wide[task];
  const int n_times = g.a.n_times, n_slots = g.a.n_slots, slot = tp->slot;
  WVA_LAG_CELL(c, tp);
  const int N = c.N, K = 11 * N;
  const int pad0 = (C - (K + 1) % C) % C;
  const int G = K + 1 + pad0;
  const int num_decode = wva_num_decode(c);
  const double lam0 = tp->lam0, lam1 = tp->lam1;
  double *const v = g.slab + wt.slab;

  bool bad = false;
  float smax_l = 0.0f;
  for (int n = 1 + tid; n <= N; n += NT) {
    const float r = wva_rate_exact(c, num_decode, n);
    bad = bad || !(r > 0.0f) || !isfinite(r);
    smax_l = fmaxf(smax_l, r);
  }
  const double smax =
      wva_lag_uniform(red_max_p<NT, 1>(bad ? (double)INFINITY : (double)smax_l, red));
  const double Lam = lam1 + smax;
  if (!(smax < (double)INFINITY) || !(Lam > 0.0) || Lam != wt.Lam) {
    // degenerate rates, or not the Lam the schedule was made for (uniform)
    if (tid == 0) {
      g.flag[task] = 1;
      g.a.steps[slot] = -1;
      for (int j = 0; j < n_times; ++j) {
        for (int f = 0; f < WVA_LAG_FLOATS; ++f) WVA_LAG_OUT(f, j) = NAN;
        g.a.violated[(size_t)j * (size_t)n_slots + (size_t)slot] = 0;
        if (g.a.raw)
          for (int f = 0; f < WVA_LAG_FUNCS; ++f)
            g.a.raw[((size_t)task * (size_t)n_times + (size_t)j) * WVA_LAG_FUNCS + f] = NAN;
      }
    }
    return;
  }
  if (tid == 0) g.flag[task] = 0;
  if (!(lam0 > 0.0)) {
    for (int s = tid; s < G; s += NT) v[s] = s == pad0 ? 1.0 : 0.0;
    return;
  }
  // log prefix over the head 0..N: thread t has a run of consecutive states
  const double l0 = log(lam0);
  const int chunk = (N + NT) / NT;
  const int n_lo = tid * chunk, n_hi = n_lo + chunk < N + 1 ? n_lo + chunk : N + 1;
  double run = 0.0;
  for (int n = n_lo < 1 ? 1 : n_lo; n < n_hi; ++n)
    run += l0 - log((double)wva_rate_exact(c, num_decode, n));
  double log_head;  // log w[N]
  run = wva_lag_scan<NT>(run, red, &log_head);
  log_head = wva_lag_uniform(log_head);
  const double lr = l0 - log((double)wva_rate_exact(c, num_decode, N));
  // the tail is linear in n: its largest term is at one of its ends
  double m = fmax(log_head, fmax(log_head + lr, log_head + (double)(K - N) * lr));
  for (int n = n_lo; n < n_hi; ++n) {
    if (n >= 1) run += l0 - log((double)wva_rate_exact(c, num_decode, n));
    v[pad0 + n] = run;
    m = fmax(m, run);
  }
  m = wva_lag_uniform(red_max_p<NT, 1>(m, red));  // its barriers order the stores above
  double sum = 0.0, unused = 0.0;
  for (int s = tid; s < G; s += NT) {
    const int n = s - pad0;
    const double e = n < 0 ? 0.0 : exp((n <= N ? v[s] : log_head + (double)(n - N) * lr) - m);
    v[s] = e;
    sum += e;
  }
  red_sum2_p<NT, 1>(sum, unused, red);
  for (int s = tid; s < G; s += NT) v[s] /= sum;  // each thread its own slots again
}

// One wave per task of the launch; does something only where segment `launch`
// closed a checkpoint: the tile partials in tile order, then wva_lag_t's
// thread-0 arithmetic.
__global__ void __launch_bounds__(WVA_WAVE)
    wva_lag_wide_fin(WvaLagWideArgs g, int task0, int launch) {
  const int lane = (int)threadIdx.x;
  const int task = task0 + (int)blockIdx.x;
  if (g.flag[task] != 0) return;
  const WvaLagWideTask wt = g.wide[task];
  if (launch >= wt.n_seg) return;
  const WvaLagSeg sg = g.segs[wt.seg0 + launch];
  if (!(sg.flags & WVA_LAG_SEG_LAST)) return;
  const WvaLagTask *const tp = g.a.tasks + task;
  const int n_times = g.a.n_times, n_slots = g.a.n_slots, slot = tp->slot, j = sg.j;
  WVA_LAG_CELL(c, tp);
  const int N = c.N;
  double sum = 0.0;
  if (lane < WVA_LAG_FUNCS)
    for (int t = 0; t < wt.n_tiles; ++t)
      sum += g.part[(size_t)(wt.tile0 + t) * WVA_LAG_FUNCS + lane];
  const double f_blk = __shfl(sum, 0, WVA_WAVE), f_srv = __shfl(sum, 1, WVA_WAVE);
  const double f_sys = __shfl(sum, 2, WVA_WAVE), f_tput = __shfl(sum, 3, WVA_WAVE);
  const double f_wait = __shfl(sum, 4, WVA_WAVE);
  if (lane != 0) return;
  const double sN = (double)wva_rate_exact(c, wva_num_decode(c), N);
  const double wait = f_wait / (1.0 - f_blk) / sN;
  const double serv = f_tput > 0.0 ? f_srv / f_tput : 0.0;
  const double eff =
      effective_concurrency(serv, c.gamma, c.alpha, c.delta, c.beta, c.in_tok, c.out_tok, N);
  const float ttft = (float)wait + wva_lag_prefill(c, (float)eff);
  const float itl = wva_lag_decode(c, (float)eff);
  WVA_LAG_OUT(0, j) = ttft;
  WVA_LAG_OUT(1, j) = itl;
  WVA_LAG_OUT(2, j) = (float)wait;
  WVA_LAG_OUT(3, j) = (float)f_blk;
  WVA_LAG_OUT(4, j) = (float)fmin(fmax(f_srv / (double)N, 0.0), 1.0);
  WVA_LAG_OUT(5, j) = (float)f_sys;
  const float t_ttft = tp->t_ttft, t_itl = tp->t_itl;
  g.a.violated[(size_t)j * (size_t)n_slots + (size_t)slot] =
      (t_ttft != 0.0f && ttft > t_ttft) || (t_itl != 0.0f && itl > t_itl);
  if (g.a.raw) {
    double *r = g.a.raw + ((size_t)task * (size_t)n_times + (size_t)j) * WVA_LAG_FUNCS;
    r[0] = f_blk;
    r[1] = f_srv;
    r[2] = f_sys;
    r[3] = f_tput;
    r[4] = wait;
  }
  if (sg.flags & WVA_LAG_SEG_FINAL) {
    // the device's own count of the steps, as wva_lag_t reports it
    double total = 0.0, jlo;
    for (int i = 0; i < n_times; ++i) total += wva_lag_window(wt.Lam * g.a.dt[i], &jlo);
    g.a.steps[slot] = total < 2147483000.0 ? (int)total : -1;
  }
}
#undef WVA_LAG_SEQ
#undef WVA_LAG_VALID
#undef WVA_LAG_RATE
#undef WVA_LAG_DEATH
#undef WVA_LAG_OUT
#undef WVA_LAG_CELL

// ---------------------------------------------------------------------------
// host: the tables of a wide pass, its device layout and its launches
// ---------------------------------------------------------------------------
#include "../native/wva_arena.h"  // 256-aligned arena layout (host only)

struct WvaLagWideIn {
  const WvaLagTask *tasks;  // host [n_tasks], by descending n_seg
  WvaLagWideTask *wide;     // host [n_tasks]; slab is filled by wva_lag_wide_plan
  const WvaLagSeg *segs;    // host [n_segs]
  const WvaLagTile *tiles;  // host [n_tiles]
  const double *dt;         // host [n_times]
  int n_tasks, n_segs, n_tiles, n_times, n_slots, stride, halo, max_steps;
};

static int wva_lag_wide_slots(int N) {
  const int C = WVA_LAG_WIDE_C, K = 11 * N;
  return K + 1 + (C - (K + 1) % C) % C;
}

// Every index a kernel will form lies inside its table, and the launch-prefix
// rule holds (tasks by descending n_seg, tiles and segments in task order).
// Fills wide[].slab round by round (a round's slabs fit `cap` bytes, a task
// larger than the cap runs alone) and returns the doubles the largest round
// needs in *slab_doubles. -2: a table is inconsistent.
static int wva_lag_wide_plan(const WvaLagWideIn &in, size_t cap, size_t *slab_doubles) {
  const int C = WVA_LAG_WIDE_C, W = WVA_LAG_WIDE_NT * WVA_LAG_WIDE_C;
  const int S = in.stride, T = in.halo;
  if (!in.tasks || !in.wide || !in.segs || !in.tiles || !in.dt) return -2;
  if (in.n_tasks < 1 || in.n_times < 1 || in.n_times > WVA_LAG_MAX_T || in.n_slots < 1) return -2;
  if (S < C || T < C || S % C || T % C || S + 2 * T > W) return -2;
  int tile_at = 0, seg_at = 0;
  size_t round = 0, worst = 0;
  for (int i = 0; i < in.n_tasks; ++i) {
    const WvaLagTask &t = in.tasks[i];
    WvaLagWideTask &w = in.wide[i];
    if (t.N <= WVA_LAG_MAX_N || t.N > WVA_LAG_WIDE_MAX_N) return -2;
    if (t.slot < 0 || t.slot >= in.n_slots) return -2;
    const int G = wva_lag_wide_slots(t.N);
    if (w.tile0 != tile_at || w.n_tiles != (G + S - 1) / S || w.n_tiles > in.n_tiles - tile_at)
      return -2;
    for (int b = 0; b < w.n_tiles; ++b)
      if (in.tiles[tile_at + b].task != i || in.tiles[tile_at + b].b != b) return -2;
    tile_at += w.n_tiles;
    if (w.seg0 != seg_at || w.n_seg < 1 || w.n_seg > in.n_segs - seg_at) return -2;
    if (i > 0 && w.n_seg > in.wide[i - 1].n_seg) return -2;
    int j = 0, done = 0;
    long long total = 0;
    for (int l = 0; l < w.n_seg; ++l) {
      const WvaLagSeg &s = in.segs[seg_at + l];
      if (s.j != j || s.first != done || s.count < 1 || s.count > T) return -2;
      if (s.jlo < 0 || s.jlo >= s.jhi || done + s.count > s.jhi) return -2;
      done += s.count;
      total += s.count;
      const bool last = done == s.jhi;
      const int want = (s.first == 0 ? WVA_LAG_SEG_FIRST : 0) | (last ? WVA_LAG_SEG_LAST : 0) |
                       (last && j == in.n_times - 1 ? WVA_LAG_SEG_FINAL : 0);
      if (s.flags != want) return -2;
      if (last) {
        ++j;
        done = 0;
      }
    }
    if (j != in.n_times || done != 0 || total > (long long)in.max_steps) return -2;
    seg_at += w.n_seg;
    const size_t need = 3 * (size_t)G;
    if (round > 0 && (round + need) * sizeof(double) > cap) round = 0;  // a new round
    w.slab = (long long)round;
    round += need;
    worst = round > worst ? round : worst;
  }
  if (tile_at != in.n_tiles || seg_at != in.n_segs) return -2;
  *slab_doubles = worst;
  return 0;
}

// the device layout of a wide pass: the five tables as one upload, the three
// records (and the probe's raw functionals) as one download, then scratch
enum {
  WVA_LW_TASKS, WVA_LW_WIDE, WVA_LW_SEGS, WVA_LW_TILES, WVA_LW_DT,  // up
  WVA_LW_F, WVA_LW_VIOL, WVA_LW_STEPS, WVA_LW_RAW,                  // down
  WVA_LW_PART, WVA_LW_WCARRY, WVA_LW_FLAG, WVA_LW_SLAB, WVA_LW_N
};
static size_t wva_lag_wide_layout(const WvaLagWideIn &in, size_t slab_doubles, bool raw,
                                  size_t *off) {
  const size_t nt = (size_t)in.n_times, ns = (size_t)in.n_slots, n = (size_t)in.n_tasks;
  const size_t sizes[WVA_LW_N] = {
      n * sizeof(WvaLagTask), n * sizeof(WvaLagWideTask), (size_t)in.n_segs * sizeof(WvaLagSeg),
      (size_t)in.n_tiles * sizeof(WvaLagTile), nt * sizeof(double),
      (size_t)WVA_LAG_FLOATS * nt * ns * sizeof(float), nt * ns, ns * sizeof(int),
      raw ? n * nt * WVA_LAG_FUNCS * sizeof(double) : 0,
      (size_t)in.n_tiles * WVA_LAG_FUNCS * sizeof(double), 2 * n * sizeof(double),
      n * sizeof(int), slab_doubles * sizeof(double)};
  return wva_arena_layout(sizes, WVA_LW_N, off);
}

// copy the tables into `up` (host memory laid out by off[], relative to the
// first table) — one contiguous upload afterwards
static void wva_lag_wide_stage(const WvaLagWideIn &in, const size_t *off, char *up) {
  memcpy(up + off[WVA_LW_TASKS], in.tasks, (size_t)in.n_tasks * sizeof(WvaLagTask));
  memcpy(up + off[WVA_LW_WIDE], in.wide, (size_t)in.n_tasks * sizeof(WvaLagWideTask));
  memcpy(up + off[WVA_LW_SEGS], in.segs, (size_t)in.n_segs * sizeof(WvaLagSeg));
  memcpy(up + off[WVA_LW_TILES], in.tiles, (size_t)in.n_tiles * sizeof(WvaLagTile));
  memcpy(up + off[WVA_LW_DT], in.dt, (size_t)in.n_times * sizeof(double));
}

// the launches of a staged pass, stream-ordered on s: per round one init, then
// per l the step launch over the tiles of the tasks that have a segment l (a
// prefix: tasks are by descending n_seg) and a fin launch if one of them closed
// a checkpoint
static int wva_lag_wide_launch(const WvaLagWideIn &in, const size_t *off, char *d, bool raw,
                               hipStream_t s) {
  constexpr int NT = WVA_LAG_WIDE_NT, C = WVA_LAG_WIDE_C;
  const size_t lds = (size_t)NT * C * sizeof(double);
  int rc = wva_optin_lds((const void *)wva_lag_tile_t<NT, C>, lds);
  if (rc != 0) return rc;
  WvaLagWideArgs g = {};
  g.a.tasks = (const WvaLagTask *)(d + off[WVA_LW_TASKS]);
  g.a.dt = (const double *)(d + off[WVA_LW_DT]);
  g.a.n_times = in.n_times;
  g.a.n_slots = in.n_slots;
  g.a.max_steps = in.max_steps;
  g.a.out_f = (float *)(d + off[WVA_LW_F]);
  g.a.violated = (uint8_t *)(d + off[WVA_LW_VIOL]);
  g.a.steps = (int *)(d + off[WVA_LW_STEPS]);
  g.a.raw = raw ? (double *)(d + off[WVA_LW_RAW]) : nullptr;
  g.wide = (const WvaLagWideTask *)(d + off[WVA_LW_WIDE]);
  g.segs = (const WvaLagSeg *)(d + off[WVA_LW_SEGS]);
  g.tiles = (const WvaLagTile *)(d + off[WVA_LW_TILES]);
  g.part = (double *)(d + off[WVA_LW_PART]);
  g.wcarry = (double *)(d + off[WVA_LW_WCARRY]);
  g.flag = (int *)(d + off[WVA_LW_FLAG]);
  g.slab = (double *)(d + off[WVA_LW_SLAB]);
  g.stride = in.stride;
  g.halo = in.halo;
  for (int t0 = 0; t0 < in.n_tasks;) {
    int t1 = t0 + 1;  // the round: up to the next task whose slab starts over
    while (t1 < in.n_tasks && in.wide[t1].slab != 0) ++t1;
    hipLaunchKernelGGL(wva_lag_wide_init, dim3(t1 - t0), dim3(NT), 0, s, g, t0);
    int live = t1 - t0;  // tasks of the round with a segment l
    for (int l = 0; l < in.wide[t0].n_seg; ++l) {
      while (in.wide[t0 + live - 1].n_seg <= l) --live;
      const WvaLagWideTask &end = in.wide[t0 + live - 1];
      const int tile_base = in.wide[t0].tile0;
      hipLaunchKernelGGL((wva_lag_tile_t<NT, C>), dim3(end.tile0 + end.n_tiles - tile_base),
                         dim3(NT), lds, s, g, tile_base, l);
      bool closes = false;
      for (int i = t0; i < t0 + live && !closes; ++i)
        closes = (in.segs[in.wide[i].seg0 + l].flags & WVA_LAG_SEG_LAST) != 0;
      if (closes) hipLaunchKernelGGL(wva_lag_wide_fin, dim3(live), dim3(WVA_WAVE), 0, s, g, t0, l);
    }
    rc = (int)hipGetLastError();
    if (rc != 0) return rc;
    t0 = t1;
  }
  return 0;
}

// One-shot probe of the wide path for tests and tools, the sibling of
// wva_lag_probe_launch with (stride, halo) as arguments. Call it with dev =
// null to learn the device bytes it needs (*need), then with a device buffer
// of at least that size: it uploads the tables, runs the pass on `stream` and
// synchronises it. off_out[4]: where in dev the fp32 records, violated, steps
// and the raw functionals [task][n_times][5] (table order) lie.
extern "C" int wva_lag_wide_probe_launch(const void *tasks, void *wide, const void *segs,
                                         const void *tiles, const double *dt, int n_tasks,
                                         int n_segs, int n_tiles, int n_times, int n_slots,
                                         int max_steps, int stride, int halo, void *stream,
                                         void *dev, size_t dev_bytes, size_t *need,
                                         size_t *off_out) {
  WvaLagWideIn in = {(const WvaLagTask *)tasks, (WvaLagWideTask *)wide, (const WvaLagSeg *)segs,
                     (const WvaLagTile *)tiles, dt, n_tasks, n_segs, n_tiles, n_times, n_slots,
                     stride, halo, max_steps};
  size_t slab = 0, off[WVA_LW_N];
  int rc = wva_lag_wide_plan(in, WVA_LAG_WIDE_SLAB_CAP, &slab);
  if (rc != 0) return rc;
  const size_t bytes = wva_lag_wide_layout(in, slab, true, off);
  if (need) *need = bytes;
  if (dev == nullptr) return 0;
  if (dev_bytes < bytes || ((uintptr_t)dev & 255) != 0) return -2;
  if (off_out)
    for (int i = 0; i < 4; ++i) off_out[i] = off[WVA_LW_F + i];
  void *up = nullptr;
  if (hipHostMalloc(&up, off[WVA_LW_F], hipHostMallocDefault) != hipSuccess) return -41;
  wva_lag_wide_stage(in, off, (char *)up);
  rc = (int)hipMemcpyAsync(dev, up, off[WVA_LW_F], hipMemcpyHostToDevice, (hipStream_t)stream);
  if (rc == 0) rc = wva_lag_wide_launch(in, off, (char *)dev, true, (hipStream_t)stream);
  const int rs = (int)hipStreamSynchronize((hipStream_t)stream);
  (void)hipHostFree(up);
  return rc != 0 ? rc : rs;
}
