// wva_lag_path_avg.inc — lag path averages: beside the state at the END of
// every tick (wva_lag_path_t), the TIME AVERAGE of the distribution over the
// tick, included by wva_kernels.hip after wva_lag_path.inc (whose kernels it
// does not touch) and before the context runtime.
//
// Arrivals are Poisson at a constant rate inside a tick, so what a random
// arrival of tick j meets is pbar = (1 / dt) int p over the tick. Under
// uniformization, with x = Lam dt and v_k = p_start P^k (p_start after the
// scale-out mixing),
//   pbar = (1 / x) sum_{k = 0..j_hi} T_k v_k,   T_k = P(Pois(x) > k),
// every term non-negative. Below the window T_k = 1 (to within e^-60), inside
// it T_{j_lo - 1} = 1 and T_k = max(T_{k - 1} - w_k, 0) with the weights w_k
// the end state's sum forms anyway. The tick takes the same j_hi steps; the
// functionals are applied to pbar as to the end state.
//
// wva_lag_path_avg_t<NT, C, TAB> is wva_lag_path_t with a third array, avg,
// and differs from it only in where that array lives:
//
// - Register classes (64,2), (64,12), (256,12): avg is a third fp64 register
//   array. Below the window a step adds v to it (acc is not touched there, as
//   before), inside the window one more FMA per state with the block-uniform
//   T_k, which is kept in scalar registers.
// - Widest class (512,24,table): v and acc are 96 of 256 registers and the
//   step needs most of the rest, but below the window acc is dead. Phase 1
//   (k < j_lo) accumulates avg in the registers of acc. At j_lo the lane moves
//   its C doubles to a lane-private slab in dynamic LDS, word i * NT + tid (NT
//   C 8 = 96 KiB, beside the 24 KiB coefficient table, through the > 64 KiB
//   opt-in; a block of this class has its CU to itself anyway), and acc is
//   seeded with w v as before. Phase 2 (the window) is a read-modify-write of
//   the slab per state and step. A lane reads and writes only its own words:
//   program order suffices, no barrier is added, consecutive lanes hit
//   consecutive 8-byte words. A tick with j_lo = 0 has no phase 1.
//
// Record, carry, per-interval rebuild, mixing, the bounds known up front and
// NaN for a chunk the host should not have scheduled are wva_lag_path_t's.
// Outputs: its six floats, violated and raw functionals from the end state,
// and the same three from pbar.

struct WvaLagPathAvgArgs {
  WvaLagPathArgs a;
  float *avg_f;           // [6][n_ticks][n_slots], as a.out_f, of pbar
  uint8_t *avg_violated;  // [n_ticks][n_slots]
  double *avg_raw;        // [n_slots][n_ticks][5] or null (the probe)
};

#define WVA_LAG_SEQ() __builtin_amdgcn_sched_barrier(0)
#define WVA_LAG_VALID(n) ((n) >= 0 && (n) <= K)
#define WVA_LAG_RATE(n) wva_rate_exact(c, num_decode, (n) < 1 ? 1 : ((n) > N ? N : (n)))
#define WVA_LAG_DEATH(n) ((n) >= 1 && (n) <= K ? (double)WVA_LAG_RATE(n) : 0.0)
#define WVA_LAG_AT(j) ((size_t)(tick0 + (j)) * (size_t)n_slots + (size_t)slot)
#define WVA_LAG_OUT(base, f, j) \
  (base)[(size_t)(f) * (size_t)a.n_ticks * (size_t)n_slots + WVA_LAG_AT(j)]
#define WVA_LAG_RAW(base, j) \
  ((base) + ((size_t)slot * (size_t)a.n_ticks + (size_t)(tick0 + (j))) * WVA_LAG_FUNCS)

// the five raw functionals of the block's vector p(i) (state n_base + i of
// this lane), summed over the block: f = blocked, in_servers, in_system, tput
// and the wait sum, the terms and their order as wva_lag_path_t forms them
template <int NT, int C, typename P>
__device__ __forceinline__ void wva_lag_path_funcs(P p_of, int n_base, const WvaCell &c,
                                                   int num_decode, double *red,
                                                   double (&f)[WVA_LAG_FUNCS]) {
  const int N = c.N, K = 11 * N;
  double f_blk = 0.0, f_srv = 0.0, f_sys = 0.0, f_tput = 0.0, f_wait = 0.0;
#pragma unroll
  for (int i = 0; i < C; ++i) {
    const int n = n_base + i;
    const double p = p_of(i);
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
  f[0] = f_blk;
  f[1] = f_srv;
  f[2] = f_sys;
  f[3] = f_tput;
  f[4] = f_wait;
}

// one record from the functionals f of x times a distribution (x = 1: the end
// state): the six floats to out[0..6) (stride elements apart), the verdict,
// and the raw functionals when the probe asked for them
__device__ __forceinline__ void wva_lag_path_record(const double (&f)[WVA_LAG_FUNCS], double x,
                                                    double sN, const WvaCell &c, float t_ttft,
                                                    float t_itl, float *out, size_t stride,
                                                    uint8_t *violated, double *raw) {
  const int N = c.N;
  const double f_blk = f[0] / x, f_srv = f[1] / x, f_sys = f[2] / x, f_tput = f[3] / x;
  const double wait = f[4] / x / (1.0 - f_blk) / sN;
  const double serv = f_tput > 0.0 ? f_srv / f_tput : 0.0;
  const double eff =
      effective_concurrency(serv, c.gamma, c.alpha, c.delta, c.beta, c.in_tok, c.out_tok, N);
  const float ttft = (float)wait + wva_lag_prefill(c, (float)eff);
  const float itl = wva_lag_decode(c, (float)eff);
  out[0] = ttft;
  out[stride] = itl;
  out[2 * stride] = (float)wait;
  out[3 * stride] = (float)f_blk;
  out[4 * stride] = (float)fmin(fmax(f_srv / (double)N, 0.0), 1.0);
  out[5 * stride] = (float)f_sys;
  *violated = (t_ttft != 0.0f && ttft > t_ttft) || (t_itl != 0.0f && itl > t_itl);
  if (raw) {
    raw[0] = f_blk;
    raw[1] = f_srv;
    raw[2] = f_sys;
    raw[3] = f_tput;
    raw[4] = wait;
  }
}

template <int NT, int C, bool TAB>
__global__ void WVA_NO_PK_F32 __launch_bounds__(NT)
    wva_lag_path_avg_t(WvaLagPathAvgArgs g, int rec0) {
  constexpr int NW = NT / WVA_WAVE;
  constexpr int HL = wva_lag_head_lanes<NT, C>();
  __shared__ double red[64];
  __shared__ double halo[2][2][NW];
  __shared__ double win_w[WVA_LAG_MAX_T];  // per interval: the weight at j_lo,
  __shared__ int win_lo[WVA_LAG_MAX_T];    // j_lo
  __shared__ int win_hi[WVA_LAG_MAX_T];    // and j_hi, its steps
  __shared__ double table[TAB ? 2 * C * HL : 1];
  extern __shared__ double wva_lag_avg_lds[];  // TAB: the avg slab, NT * C doubles
  const WvaLagPathArgs &a = g.a;
  const int tid = (int)threadIdx.x;
  const WvaLagPathRec rec = a.recs[rec0 + (int)blockIdx.x];
  const WvaLagPathTask *const tp = a.tasks + rec.task;
  const int n_slots = a.n_slots, slot = tp->slot, tick0 = rec.tick0, n_iv = rec.n;
  WvaCell c;  // the fields the rate and latency terms read
  c.in_tok = tp->in_tok;
  c.out_tok = tp->out_tok;
  c.N = tp->N;
  c.alpha = tp->alpha;
  c.beta = tp->beta;
  c.gamma = tp->gamma;
  c.delta = tp->delta;
  const int N = c.N, K = 11 * N;
  const int start = rec.flags & 3;
  const bool store = (rec.flags & WVA_LAG_PATH_STORE) != 0;
  // the host checked these before the launch (wva_lag_path_plan); uniform
  if (N < 1 || K + 1 > NT * C || slot < 0 || slot >= n_slots || n_iv < 1 ||
      n_iv > WVA_LAG_MAX_T || tick0 < 0 || tick0 > a.n_ticks - n_iv ||
      ((store || start == WVA_LAG_PATH_CARRY) && tp->carry < 0))
    return;
  const int pad0 = (C - (K + 1) % C) % C;  // state K closes its lane
  const int n_first = tid * C - pad0;       // the state v[0] holds
  const int num_decode = wva_num_decode(c);
  const double2 *const desc = a.desc + (size_t)slot * (size_t)a.n_ticks + (size_t)tick0;
  double *const slab = a.carry + (tp->carry < 0 ? 0 : tp->carry) + tid;
  double *const avg_s = wva_lag_avg_lds + tid;  // TAB: word i of this lane at avg_s[i * NT]
  const size_t stride = (size_t)a.n_ticks * (size_t)n_slots;

  // ---- the largest rate, and the degenerate-rate guard
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

  // ---- the window and the steps of every interval of the chunk, before the
  // first step is taken: thread j has interval j
  double mine = 0.0, unfit = 0.0;
  if (tid < n_iv) {
    const double2 d = desc[tid];
    const double x = (d.x + smax) * a.dt;
    double jlo;
    mine = wva_lag_window(x, &jlo);
    const bool fits = smax < (double)INFINITY && d.x >= 0.0 && d.y >= 0.0 && d.y <= 1.0 &&
                      x > 0.0 && mine <= (double)a.max_steps;
    win_lo[tid] = fits ? (int)jlo : 0;
    win_hi[tid] = fits ? (int)mine : 0;
    win_w[tid] = fits ? exp(wva_lag_pois_log_pmf(jlo, x)) : 0.0;
    a.steps[WVA_LAG_AT(tid)] = smax < (double)INFINITY && mine < 2147483000.0 ? (int)mine : -1;
    if (!fits) {
      unfit = 1.0;
      mine = 0.0;
    }
  }
  red_sum2_p<NT, 1>(mine, unfit, red);  // integers below 2^53: exact in any order
  const double total = wva_lag_uniform(mine);
  unfit = wva_lag_uniform(unfit);
  if constexpr (NT == WVA_WAVE) __builtin_amdgcn_wave_barrier();
  if (unfit != 0.0 || !(total <= (double)a.max_steps)) {
    // not the chunk the host scheduled: no evaluation here or downstream (uniform)
    if (tid == 0) {
      for (int j = 0; j < n_iv; ++j) {
        for (int f = 0; f < WVA_LAG_FLOATS; ++f) {
          WVA_LAG_OUT(a.out_f, f, j) = NAN;
          WVA_LAG_OUT(g.avg_f, f, j) = NAN;
        }
        a.violated[WVA_LAG_AT(j)] = 0;
        g.avg_violated[WVA_LAG_AT(j)] = 0;
        if (a.raw)
          for (int f = 0; f < WVA_LAG_FUNCS; ++f) {
            WVA_LAG_RAW(a.raw, j)[f] = NAN;
            WVA_LAG_RAW(g.avg_raw, j)[f] = NAN;
          }
      }
    }
    if (store) {
#pragma unroll
      for (int i = 0; i < C; ++i) slab[i * NT] = NAN;
    }
    return;
  }

  const double sN = (double)wva_rate_exact(c, num_decode, N);
  WvaLagCoef<C, TAB, HL> k;
  if constexpr (TAB) {
    // head waves: the waves whose first state is not above N
    const int head_waves = (N + pad0) / (WVA_WAVE * C) + 1;
    k.tab = table + (tid < HL ? tid : 0);
    k.head = __builtin_amdgcn_readfirstlane(tid / WVA_WAVE < head_waves ? 1 : 0) != 0;
    if (head_waves * WVA_WAVE > HL) return;  // cannot happen for an N the class takes; uniform
  }

  // ---- the start of the chunk
  double v[C], acc[C];
  double avg[TAB ? 1 : C];  // TAB: in acc below the window, in LDS inside it
  if (start == WVA_LAG_PATH_CARRY) {
#pragma unroll
    for (int i = 0; i < C; ++i) v[i] = slab[i * NT];
  } else if (start == WVA_LAG_PATH_STATIONARY && tp->lam0 > 0.0) {
    // the stationary distribution at lam0, in log space as wva_lag_t builds it
    const double l0 = log(tp->lam0);
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
  for (int j = 0; j < n_iv; ++j) {
    const double2 d = desc[j];
    const double lam = d.x, keep = d.y;
    const double Lam = lam + smax;
    const double x = Lam * a.dt;
    // (the lane's first state through an opaque copy: what the set-up below
    // and the functionals derive from it per state is invariant over j, and
    // hoisted out of this loop it would sit in registers across the step loops)
    int n_base = n_first;
    asm volatile("" : "+v"(n_base));

    // scale-out: the replicas that joined are empty
#pragma unroll
    for (int i = 0; i < C; ++i) {
      v[i] *= keep;
      if (n_base + i == 0) v[i] += 1.0 - keep;
    }

    // this interval's stencil
    const double up = lam / Lam;
    const double up_left = (n_base - 1 >= 0 && n_base - 1 < K) ? up : 0.0;
    if constexpr (TAB) {
      k.dn_t = sN / Lam;
      k.stay_t = fmax(1.0 - up - k.dn_t, 0.0);
      k.stay_last = n_base + C - 1 == K ? fmax(1.0 - k.dn_t, 0.0) : k.stay_t;
      if (k.head) {
#pragma unroll
        for (int i = 0; i < C; ++i) {
          const int n = n_base + i;
          const double dn = WVA_LAG_DEATH(n) / Lam;
          table[i * HL + tid] = WVA_LAG_VALID(n) ? fmax(1.0 - (n < K ? up : 0.0) - dn, 0.0) : 0.0;
          table[(C + i) * HL + tid] = WVA_LAG_DEATH(n + 1) / Lam;
          WVA_LAG_SEQ();
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < C; ++i) {
        const int n = n_base + i;
        const double dn = WVA_LAG_DEATH(n) / Lam;
        k.stay[i] = WVA_LAG_VALID(n) ? fmax(1.0 - (n < K ? up : 0.0) - dn, 0.0) : 0.0;
        k.dnr[i] = WVA_LAG_DEATH(n + 1) / Lam;
        WVA_LAG_SEQ();
      }
    }

    const int klo = __builtin_amdgcn_readfirstlane(win_lo[j]);
    const int khi = __builtin_amdgcn_readfirstlane(win_hi[j]);
    // phase 1, k < j_lo: T_k = 1, the sum of v_0 .. v_{j_lo - 1}
#pragma unroll
    for (int i = 0; i < C; ++i) {
      if constexpr (TAB) acc[i] = 0.0;
      else avg[i] = 0.0;
    }
    for (int s = 0; s < klo; ++s) {
#pragma unroll
      for (int i = 0; i < C; ++i) {
        if constexpr (TAB) acc[i] += v[i];
        else avg[i] += v[i];
      }
      wva_lag_step<NT, C, false, TAB, HL>(v, acc, k, up, up_left, 0.0, halo, buf);
    }
    // j_lo: T = 1 - w; the widest class moves avg out of acc's registers
    double w = wva_lag_uniform(win_w[j]);
    double T = wva_lag_uniform(fmax(1.0 - w, 0.0));
#pragma unroll
    for (int i = 0; i < C; ++i) {
      if constexpr (TAB) avg_s[i * NT] = fma(T, v[i], acc[i]);
      else avg[i] = fma(T, v[i], avg[i]);
      acc[i] = w * v[i];
    }
    // phase 2, the window
    for (int s = klo + 1; s <= khi; ++s) {
      // w(s) = w(s - 1) x / s, the quotient as wva_lag_t forms it
      const double sd = (double)s;
      double rs = __builtin_amdgcn_rcp(sd);
      rs = fma(fma(-sd, rs, 1.0), rs, rs);
      rs = fma(fma(-sd, rs, 1.0), rs, rs);
      w *= x * rs;
      wva_lag_step<NT, C, true, TAB, HL>(v, acc, k, up, up_left, w, halo, buf);
      T = wva_lag_uniform(fmax(T - w, 0.0));
#pragma unroll
      for (int i = 0; i < C; ++i) {
        if constexpr (TAB) avg_s[i * NT] = fma(T, v[i], avg_s[i * NT]);
        else avg[i] = fma(T, v[i], avg[i]);
      }
    }

    // p(end of tick j) = acc, the start of the next interval; its functionals,
    // then those of x pbar
    asm volatile("" : "+v"(n_base));
    double f_end[WVA_LAG_FUNCS], f_avg[WVA_LAG_FUNCS];
    wva_lag_path_funcs<NT, C>([&](int i) { return acc[i]; }, n_base, c, num_decode, red, f_end);
#pragma unroll
    for (int i = 0; i < C; ++i) v[i] = acc[i];
    asm volatile("" : "+v"(n_base));
    if constexpr (TAB)
      wva_lag_path_funcs<NT, C>([&](int i) { return avg_s[i * NT]; }, n_base, c, num_decode, red,
                                f_avg);
    else
      wva_lag_path_funcs<NT, C>([&](int i) { return avg[i]; }, n_base, c, num_decode, red, f_avg);
    if (tid == 0) {
      const float t_ttft = tp->t_ttft, t_itl = tp->t_itl;
      wva_lag_path_record(f_end, 1.0, sN, c, t_ttft, t_itl, &WVA_LAG_OUT(a.out_f, 0, j), stride,
                          a.violated + WVA_LAG_AT(j), a.raw ? WVA_LAG_RAW(a.raw, j) : nullptr);
      wva_lag_path_record(f_avg, x, sN, c, t_ttft, t_itl, &WVA_LAG_OUT(g.avg_f, 0, j), stride,
                          g.avg_violated + WVA_LAG_AT(j),
                          a.raw ? WVA_LAG_RAW(g.avg_raw, j) : nullptr);
    }
  }
  if (store) {
#pragma unroll
    for (int i = 0; i < C; ++i) slab[i * NT] = v[i];
  }
}
#undef WVA_LAG_SEQ
#undef WVA_LAG_VALID
#undef WVA_LAG_RATE
#undef WVA_LAG_DEATH
#undef WVA_LAG_AT
#undef WVA_LAG_OUT
#undef WVA_LAG_RAW

// ---------------------------------------------------------------------------
// host: wva_lag_path.inc's tables, plan and launch order; larger output blocks
// ---------------------------------------------------------------------------
// the device layout: the tables as one upload (as WVA_LP_*), the end-state and
// the averaged records (and the probe's raw functionals) as one download, then
// the carry slab
enum {
  WVA_LPA_TASKS, WVA_LPA_RECS, WVA_LPA_DESC,                    // up
  WVA_LPA_F, WVA_LPA_VIOL, WVA_LPA_STEPS, WVA_LPA_AF, WVA_LPA_AVIOL,  // down
  WVA_LPA_RAW, WVA_LPA_ARAW,                                    // down (the probe)
  WVA_LPA_CARRY, WVA_LPA_N
};
static_assert(WVA_LPA_TASKS == WVA_LP_TASKS && WVA_LPA_RECS == WVA_LP_RECS &&
                  WVA_LPA_DESC == WVA_LP_DESC,
              "wva_lag_path_stage fills the upload of both layouts");
static size_t wva_lag_path_avg_layout(const WvaLagPathIn &in, size_t slab_doubles, bool raw,
                                      size_t *off) {
  const size_t cells = (size_t)in.n_ticks * (size_t)in.n_slots;
  const size_t raw_bytes = raw ? cells * WVA_LAG_FUNCS * sizeof(double) : 0;
  const size_t sizes[WVA_LPA_N] = {
      (size_t)in.n_tasks * sizeof(WvaLagPathTask), (size_t)in.n_recs * sizeof(WvaLagPathRec),
      cells * 2 * sizeof(double), WVA_LAG_FLOATS * cells * sizeof(float), cells,
      cells * sizeof(int), WVA_LAG_FLOATS * cells * sizeof(float), cells, raw_bytes, raw_bytes,
      slab_doubles * sizeof(double)};
  return wva_arena_layout(sizes, WVA_LPA_N, off);
}

// dynamic LDS of a class: the avg slab of the table class, nothing elsewhere
static size_t wva_lag_path_avg_lds(int cls) {
  return cls == 0 ? (size_t)wva_lag_class_nt[0] * (size_t)wva_lag_class_c[0] * sizeof(double) : 0;
}

static int wva_lag_path_avg_dispatch(int cls, int n, int rec0, const WvaLagPathAvgArgs &g,
                                     hipStream_t s) {
  const size_t lds = wva_lag_path_avg_lds(cls);
  switch (cls) {
    case 0: {
      const int rc = wva_optin_lds((const void *)wva_lag_path_avg_t<512, 24, true>, lds);
      if (rc != 0) return rc;
      hipLaunchKernelGGL((wva_lag_path_avg_t<512, 24, true>), dim3(n), dim3(512), lds, s, g, rec0);
      break;
    }
    case 1: hipLaunchKernelGGL((wva_lag_path_avg_t<256, 12, false>), dim3(n), dim3(256), 0, s, g, rec0); break;
    case 2: hipLaunchKernelGGL((wva_lag_path_avg_t<64, 12, false>), dim3(n), dim3(64), 0, s, g, rec0); break;
    case 3: hipLaunchKernelGGL((wva_lag_path_avg_t<64, 2, false>), dim3(n), dim3(64), 0, s, g, rec0); break;
    default: return -3;
  }
  return (int)hipGetLastError();
}

// wva_lag_path_launch for the averaged kernels: the same streams, fork/join
// and rounds, the records at the offsets of wva_lag_path_avg_layout
static int wva_lag_path_avg_launch(const WvaLagPathIn &in, const size_t *off, char *d, bool raw,
                                   hipStream_t *stream, hipEvent_t fork, hipEvent_t *join) {
  WvaLagPathAvgArgs g = {};
  g.a.tasks = (const WvaLagPathTask *)(d + off[WVA_LPA_TASKS]);
  g.a.recs = (const WvaLagPathRec *)(d + off[WVA_LPA_RECS]);
  g.a.desc = (const double2 *)(d + off[WVA_LPA_DESC]);
  g.a.carry = (double *)(d + off[WVA_LPA_CARRY]);
  g.a.dt = in.dt;
  g.a.n_ticks = in.n_ticks;
  g.a.n_slots = in.n_slots;
  g.a.max_steps = in.max_steps;
  g.a.out_f = (float *)(d + off[WVA_LPA_F]);
  g.a.violated = (uint8_t *)(d + off[WVA_LPA_VIOL]);
  g.a.steps = (int *)(d + off[WVA_LPA_STEPS]);
  g.a.raw = raw ? (double *)(d + off[WVA_LPA_RAW]) : nullptr;
  g.avg_f = (float *)(d + off[WVA_LPA_AF]);
  g.avg_violated = (uint8_t *)(d + off[WVA_LPA_AVIOL]);
  g.avg_raw = raw ? (double *)(d + off[WVA_LPA_ARAW]) : nullptr;
  return wva_lag_path_rounds(in, stream, fork, join, [&](int cls, int n, int rec0, hipStream_t s) {
    return wva_lag_path_avg_dispatch(cls, n, rec0, g, s);
  });
}

// wva_lag_path_probe_launch with the averages. off_out[7]: where in dev the
// fp32 records, violated, steps, the averaged fp32 records and verdicts, the
// raw functionals [slot][n_ticks][5] and the averaged raw functionals lie.
extern "C" int wva_lag_path_avg_probe_launch(const void *tasks, const void *recs,
                                             const double *desc, const int *launches, int n_tasks,
                                             int n_recs, int n_launches, int n_ticks, int n_slots,
                                             int max_steps, double dt, void *stream, void *dev,
                                             size_t dev_bytes, size_t *need, size_t *off_out) {
  WvaLagPathIn in = {(const WvaLagPathTask *)tasks, (const WvaLagPathRec *)recs, desc,
                     (const WvaLagPathLaunch *)launches, n_tasks, n_recs, n_launches, n_ticks,
                     n_slots, max_steps, dt};
  size_t slab = 0, off[WVA_LPA_N];
  int rc = wva_lag_path_plan(in, WVA_LAG_WIDE_SLAB_CAP, &slab);
  if (rc != 0) return rc;
  const size_t bytes = wva_lag_path_avg_layout(in, slab, true, off);
  if (need) *need = bytes;
  if (dev == nullptr) return 0;
  if (dev_bytes < bytes || ((uintptr_t)dev & 255) != 0) return -2;
  if (off_out)
    for (int i = 0; i < 7; ++i) off_out[i] = off[WVA_LPA_F + i];
  void *up = nullptr;
  if (hipHostMalloc(&up, off[WVA_LPA_F], hipHostMallocDefault) != hipSuccess) return -41;
  wva_lag_path_stage(in, off, (char *)up);
  hipStream_t s[WVA_LAG_CLASSES] = {(hipStream_t)stream, (hipStream_t)stream, (hipStream_t)stream,
                                    (hipStream_t)stream};
  hipEvent_t fork = nullptr;
  rc = hipEventCreateWithFlags(&fork, hipEventDisableTiming) == hipSuccess ? 0 : -10;
  if (rc == 0)
    rc = (int)hipMemcpyAsync(dev, up, off[WVA_LPA_F], hipMemcpyHostToDevice, (hipStream_t)stream);
  if (rc == 0) rc = wva_lag_path_avg_launch(in, off, (char *)dev, true, s, fork, nullptr);
  const int rs = (int)hipStreamSynchronize((hipStream_t)stream);
  if (fork) (void)hipEventDestroy(fork);
  (void)hipHostFree(up);
  return rc != 0 ? rc : rs;
}
