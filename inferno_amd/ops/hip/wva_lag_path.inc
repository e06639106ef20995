// wva_lag_path.inc — lag paths: the transient distribution of a cell's chain
// ALONG a forecast, included by wva_kernels.hip after wva_lag.inc (whose
// kernels it does not touch) and before the context runtime.
//
// wva_lag_t answers one load step under one allocation from a stationary
// start, and its state dies with the launch. wva_lag_path_t walks consecutive
// ticks of one length dt, each at its own per-replica rate, and keeps the
// vector: the queue that filled during tick 3 is there at the start of tick
// 4. A task is one RUN of a server: consecutive ticks on one cell with
// replicas. It is a sibling of wva_lag_t with the same design (one block per
// task, state K closes its lane, v and acc fp64 register arrays, the
// uniformization stencil of wva_lag_step, no barrier and no LDS access per
// step in a one-wave class, one barrier per step in a wider one) and four
// differences:
//
// 1. Per-interval coefficients. Lam_j = lam_j + smax, up_j, stay and dnr
//    change with every tick, so the register classes rebuild their two
//    coefficient arrays at the start of each interval (C divisions against
//    hundreds of steps), and the table class rewrites its LDS table: a head
//    lane rewrites and later reads only its own words, program order suffices,
//    no barrier is added. The rates s(n) are recomputed at each rebuild from
//    an opaque copy of the lane's first state, so that neither they nor the
//    functional factors are kept in registers across the step loops.
// 2. Scale-out mixing. Replicas that join are empty: at an interval's start
//    p <- keep p + (1 - keep) e_0, keep = R_old / R_new (1: no change). Every
//    state is scaled, the lane that owns state 0 adds 1 - keep; the padding
//    stays exactly 0.
// 3. State carry through HBM. A launch covers one chunk of at most
//    WVA_LAG_MAX_T ticks; a per-chunk record says how v starts (stationary at
//    lam0, empty, or the lane's C doubles of carry[task]) and whether the
//    block stores v back at the end. Word i * NT + tid: loads and stores
//    coalesce. A block reads only its own slab and reads before it writes, so
//    one buffer per task is enough and the kernel boundary (stream order: a
//    task never changes class, a class never changes stream) is the only
//    synchronisation.
// 4. The interval descriptors {lam, keep} are a device array [slot][S]; dt is
//    an argument. The windows and step counts of the chunk's intervals are
//    computed before the first step (thread j has interval j), stored per
//    tick, and their sum compared with max_steps: every loop bound is
//    block-uniform and known up front. A chunk the host should not have
//    scheduled writes NaN (to its records and to the carry) and returns.

#define WVA_LAG_PATH_STATIONARY 0  // WvaLagPathRec.flags & 3: v starts stationary at lam0,
#define WVA_LAG_PATH_EMPTY 1       // ... with all mass in state 0,
#define WVA_LAG_PATH_CARRY 2       // ... from carry[task]
#define WVA_LAG_PATH_STORE 4       // the run goes on: store v at the end

// One run of a server. 64 bytes; ops/sweep.py LAG_PATH_TASK_DTYPE.
struct WvaLagPathTask {
  int in_tok, out_tok, N;
  int slot;  // the server: column of the records, row of the descriptors
  float alpha, beta, gamma, delta;
  float t_ttft, t_itl;  // the server's targets (0: not checked)
  int pad[2];
  double lam0;      // req/msec per replica of a stationary start
  long long carry;  // first double of the task's carry slab, -1 without one
};
static_assert(sizeof(WvaLagPathTask) == 64, "task record is 64 bytes");
// The ticks [tick0, tick0 + n) of a task that one launch runs. 16 bytes.
struct WvaLagPathRec {
  int task, tick0, n, flags;
};
struct WvaLagPathArgs {
  const WvaLagPathTask *tasks;
  const WvaLagPathRec *recs;
  const double2 *desc;  // [n_slots][n_ticks]: {lam (req/msec per replica), keep}
  double *carry;
  double dt;  // msec, every tick
  int n_ticks, n_slots, max_steps;
  float *out_f;       // [6][n_ticks][n_slots]: ttft, itl, wait, blocked, rho, in_system
  uint8_t *violated;  // [n_ticks][n_slots]
  int *steps;         // [n_ticks][n_slots]: the tick's stencil steps, -1 without a model
  double *raw;        // [n_slots][n_ticks][5] or null (the probe), as WvaLagArgs.raw
};

#define WVA_LAG_SEQ() __builtin_amdgcn_sched_barrier(0)
#define WVA_LAG_VALID(n) ((n) >= 0 && (n) <= K)
#define WVA_LAG_RATE(n) wva_rate_exact(c, num_decode, (n) < 1 ? 1 : ((n) > N ? N : (n)))
#define WVA_LAG_DEATH(n) ((n) >= 1 && (n) <= K ? (double)WVA_LAG_RATE(n) : 0.0)
#define WVA_LAG_AT(j) ((size_t)(tick0 + (j)) * (size_t)n_slots + (size_t)slot)
#define WVA_LAG_OUT(f, j) \
  a.out_f[(size_t)(f) * (size_t)a.n_ticks * (size_t)n_slots + WVA_LAG_AT(j)]

template <int NT, int C, bool TAB>
__global__ void WVA_NO_PK_F32 __launch_bounds__(NT)
    wva_lag_path_t(WvaLagPathArgs a, int rec0) {
  constexpr int NW = NT / WVA_WAVE;
  constexpr int HL = wva_lag_head_lanes<NT, C>();
  __shared__ double red[64];
  __shared__ double halo[2][2][NW];
  __shared__ double win_w[WVA_LAG_MAX_T];  // per interval: the weight at j_lo,
  __shared__ int win_lo[WVA_LAG_MAX_T];    // j_lo
  __shared__ int win_hi[WVA_LAG_MAX_T];    // and j_hi, its steps
  __shared__ double table[TAB ? 2 * C * HL : 1];
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
        for (int f = 0; f < WVA_LAG_FLOATS; ++f) WVA_LAG_OUT(f, j) = NAN;
        a.violated[WVA_LAG_AT(j)] = 0;
        if (a.raw)
          for (int f = 0; f < WVA_LAG_FUNCS; ++f)
            a.raw[((size_t)slot * (size_t)a.n_ticks + (size_t)(tick0 + j)) * WVA_LAG_FUNCS + f] =
                NAN;
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
    for (int s = 0; s < klo; ++s)
      wva_lag_step<NT, C, false, TAB, HL>(v, acc, k, up, up_left, 0.0, halo, buf);
    double w = wva_lag_uniform(win_w[j]);
#pragma unroll
    for (int i = 0; i < C; ++i) acc[i] = w * v[i];
    for (int s = klo + 1; s <= khi; ++s) {
      // w(s) = w(s - 1) x / s, the quotient as wva_lag_t forms it
      const double sd = (double)s;
      double rs = __builtin_amdgcn_rcp(sd);
      rs = fma(fma(-sd, rs, 1.0), rs, rs);
      rs = fma(fma(-sd, rs, 1.0), rs, rs);
      w *= x * rs;
      wva_lag_step<NT, C, true, TAB, HL>(v, acc, k, up, up_left, w, halo, buf);
    }

    // p(end of tick j) = acc, the start of the next interval; its functionals
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
      a.violated[WVA_LAG_AT(j)] =
          (t_ttft != 0.0f && ttft > t_ttft) || (t_itl != 0.0f && itl > t_itl);
      if (a.raw) {
        double *r =
            a.raw + ((size_t)slot * (size_t)a.n_ticks + (size_t)(tick0 + j)) * WVA_LAG_FUNCS;
        r[0] = f_blk;
        r[1] = f_srv;
        r[2] = f_sys;
        r[3] = f_tput;
        r[4] = wait;
      }
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

// ---------------------------------------------------------------------------
// host: the tables of a path pass (ops/sweep.py lag_path_schedule), their
// check, the device layout and the launches
// ---------------------------------------------------------------------------
// One launch: `count` records from rec0 on, all of class cls. Launches are in
// (round, chunk, class) order; a round is a set of tasks whose carry slabs fit
// the cap together, and the slab is reused from round to round.
struct WvaLagPathLaunch {
  int rec0, count, cls, round;
};
struct WvaLagPathIn {
  const WvaLagPathTask *tasks;       // host [n_tasks]
  const WvaLagPathRec *recs;         // host [n_recs], in launch order
  const double *desc;                // host [n_slots][n_ticks][2]
  const WvaLagPathLaunch *launches;  // host [n_launches]
  int n_tasks, n_recs, n_launches, n_ticks, n_slots, max_steps;
  double dt;
};

// the narrowest class that holds N (the class fixes a task's carry layout)
static int wva_lag_path_class(int N) {
  int cls = 0;
  for (int k = 1; k < WVA_LAG_CLASSES; ++k)
    if (11 * N + 1 <= wva_lag_class_nt[k] * wva_lag_class_c[k]) cls = k;
  return cls;
}

// Every index a kernel will form lies inside its table or the slab; returns
// the doubles of carry the pass needs in *slab_doubles. -2: inconsistent.
static int wva_lag_path_plan(const WvaLagPathIn &in, size_t cap, size_t *slab_doubles) {
  if (!in.tasks || !in.recs || !in.desc || !in.launches) return -2;
  if (in.n_tasks < 1 || in.n_recs < 1 || in.n_launches < 1 || in.n_ticks < 1 || in.n_slots < 1 ||
      in.max_steps < 0 || !(in.dt > 0.0) || !(in.dt < (double)INFINITY))
    return -2;
  for (int i = 0; i < in.n_tasks; ++i) {
    const WvaLagPathTask &t = in.tasks[i];
    if (t.N < 1 || t.N > WVA_LAG_MAX_N || t.slot < 0 || t.slot >= in.n_slots) return -2;
  }
  size_t worst = 0;
  int at = 0;
  for (int l = 0; l < in.n_launches; ++l) {
    const WvaLagPathLaunch &L = in.launches[l];
    if (L.cls < 0 || L.cls >= WVA_LAG_CLASSES || L.rec0 != at || L.count < 1 ||
        L.count > in.n_recs - at || L.round < 0 || (l > 0 && L.round < in.launches[l - 1].round))
      return -2;
    const size_t states = (size_t)wva_lag_class_nt[L.cls] * (size_t)wva_lag_class_c[L.cls];
    for (int r = at; r < at + L.count; ++r) {
      const WvaLagPathRec &rec = in.recs[r];
      if (rec.task < 0 || rec.task >= in.n_tasks) return -2;
      const WvaLagPathTask &t = in.tasks[rec.task];
      if (wva_lag_path_class(t.N) != L.cls) return -2;
      if (rec.n < 1 || rec.n > WVA_LAG_MAX_T || rec.tick0 < 0 || rec.tick0 > in.n_ticks - rec.n)
        return -2;
      if (rec.flags < 0 || rec.flags > 7 || (rec.flags & 3) == 3) return -2;
      if ((rec.flags & WVA_LAG_PATH_STORE) || (rec.flags & 3) == WVA_LAG_PATH_CARRY) {
        if (t.carry < 0 || ((size_t)t.carry + states) * sizeof(double) > cap) return -2;
        worst = (size_t)t.carry + states > worst ? (size_t)t.carry + states : worst;
      }
    }
    at += L.count;
  }
  if (at != in.n_recs) return -2;
  *slab_doubles = worst;
  return 0;
}

// the device layout: three tables as one upload, the three records (and the
// probe's raw functionals) as one download, then the carry slab
enum {
  WVA_LP_TASKS, WVA_LP_RECS, WVA_LP_DESC,         // up
  WVA_LP_F, WVA_LP_VIOL, WVA_LP_STEPS, WVA_LP_RAW,  // down
  WVA_LP_CARRY, WVA_LP_N
};
static size_t wva_lag_path_layout(const WvaLagPathIn &in, size_t slab_doubles, bool raw,
                                  size_t *off) {
  const size_t cells = (size_t)in.n_ticks * (size_t)in.n_slots;
  const size_t sizes[WVA_LP_N] = {
      (size_t)in.n_tasks * sizeof(WvaLagPathTask), (size_t)in.n_recs * sizeof(WvaLagPathRec),
      cells * 2 * sizeof(double), WVA_LAG_FLOATS * cells * sizeof(float), cells,
      cells * sizeof(int), raw ? cells * WVA_LAG_FUNCS * sizeof(double) : 0,
      slab_doubles * sizeof(double)};
  return wva_arena_layout(sizes, WVA_LP_N, off);
}

static void wva_lag_path_stage(const WvaLagPathIn &in, const size_t *off, char *up) {
  memcpy(up + off[WVA_LP_TASKS], in.tasks, (size_t)in.n_tasks * sizeof(WvaLagPathTask));
  memcpy(up + off[WVA_LP_RECS], in.recs, (size_t)in.n_recs * sizeof(WvaLagPathRec));
  memcpy(up + off[WVA_LP_DESC], in.desc,
         (size_t)in.n_ticks * (size_t)in.n_slots * 2 * sizeof(double));
}

static int wva_lag_path_dispatch(int cls, int n, int rec0, const WvaLagPathArgs &a,
                                 hipStream_t s) {
  switch (cls) {
    case 0: hipLaunchKernelGGL((wva_lag_path_t<512, 24, true>), dim3(n), dim3(512), 0, s, a, rec0); break;
    case 1: hipLaunchKernelGGL((wva_lag_path_t<256, 12, false>), dim3(n), dim3(256), 0, s, a, rec0); break;
    case 2: hipLaunchKernelGGL((wva_lag_path_t<64, 12, false>), dim3(n), dim3(64), 0, s, a, rec0); break;
    case 3: hipLaunchKernelGGL((wva_lag_path_t<64, 2, false>), dim3(n), dim3(64), 0, s, a, rec0); break;
    default: return -3;
  }
  return (int)hipGetLastError();
}

// The launches of a staged pass behind whatever `main` holds, each made by
// dispatch(class, count, rec0, stream). Class k runs on
// stream[k] (equal streams are fine: the probe passes one four times), forked
// from and joined back into stream[0] = main with fork / join[k - 1] once per
// round: a task keeps its class, so stream order alone puts its chunks one
// after the other, and only the reuse of the slab by the next round needs all
// classes to have finished.
template <typename Dispatch>
static int wva_lag_path_rounds(const WvaLagPathIn &in, hipStream_t *stream, hipEvent_t fork,
                               hipEvent_t *join, Dispatch dispatch) {
  hipStream_t main = stream[0];
  for (int l0 = 0; l0 < in.n_launches;) {
    int l1 = l0;  // the round's launches
    while (l1 < in.n_launches && in.launches[l1].round == in.launches[l0].round) ++l1;
    bool used[WVA_LAG_CLASSES] = {};
    if (hipEventRecord(fork, main) != hipSuccess) return -10;
    for (int l = l0; l < l1; ++l) {
      const WvaLagPathLaunch &L = in.launches[l];
      hipStream_t s = stream[L.cls];
      if (!used[L.cls] && s != main && hipStreamWaitEvent(s, fork, 0) != hipSuccess) return -11;
      used[L.cls] = true;
      const int rc = dispatch(L.cls, L.count, L.rec0, s);
      if (rc != 0) return rc;
    }
    for (int k = 1; k < WVA_LAG_CLASSES; ++k) {
      if (!used[k] || stream[k] == main) continue;
      if (hipEventRecord(join[k - 1], stream[k]) != hipSuccess) return -12;
      if (hipStreamWaitEvent(main, join[k - 1], 0) != hipSuccess) return -14;
    }
    l0 = l1;
  }
  return 0;
}

static int wva_lag_path_launch(const WvaLagPathIn &in, const size_t *off, char *d, bool raw,
                               hipStream_t *stream, hipEvent_t fork, hipEvent_t *join) {
  WvaLagPathArgs a = {};
  a.tasks = (const WvaLagPathTask *)(d + off[WVA_LP_TASKS]);
  a.recs = (const WvaLagPathRec *)(d + off[WVA_LP_RECS]);
  a.desc = (const double2 *)(d + off[WVA_LP_DESC]);
  a.carry = (double *)(d + off[WVA_LP_CARRY]);
  a.dt = in.dt;
  a.n_ticks = in.n_ticks;
  a.n_slots = in.n_slots;
  a.max_steps = in.max_steps;
  a.out_f = (float *)(d + off[WVA_LP_F]);
  a.violated = (uint8_t *)(d + off[WVA_LP_VIOL]);
  a.steps = (int *)(d + off[WVA_LP_STEPS]);
  a.raw = raw ? (double *)(d + off[WVA_LP_RAW]) : nullptr;
  return wva_lag_path_rounds(in, stream, fork, join, [&](int cls, int n, int rec0, hipStream_t s) {
    return wva_lag_path_dispatch(cls, n, rec0, a, s);
  });
}

// One-shot probe for tests and tools, in the manner of
// wva_lag_wide_probe_launch: dev = null asks for the device bytes (*need),
// then a 256-aligned device buffer of that size runs the pass on `stream` and
// synchronises it. off_out[4]: where in dev the fp32 records, violated, steps
// and the raw functionals [slot][n_ticks][5] lie.
extern "C" int wva_lag_path_probe_launch(const void *tasks, const void *recs, const double *desc,
                                         const int *launches, int n_tasks, int n_recs,
                                         int n_launches, int n_ticks, int n_slots, int max_steps,
                                         double dt, void *stream, void *dev, size_t dev_bytes,
                                         size_t *need, size_t *off_out) {
  WvaLagPathIn in = {(const WvaLagPathTask *)tasks, (const WvaLagPathRec *)recs, desc,
                     (const WvaLagPathLaunch *)launches, n_tasks, n_recs, n_launches, n_ticks,
                     n_slots, max_steps, dt};
  size_t slab = 0, off[WVA_LP_N];
  int rc = wva_lag_path_plan(in, WVA_LAG_WIDE_SLAB_CAP, &slab);
  if (rc != 0) return rc;
  const size_t bytes = wva_lag_path_layout(in, slab, true, off);
  if (need) *need = bytes;
  if (dev == nullptr) return 0;
  if (dev_bytes < bytes || ((uintptr_t)dev & 255) != 0) return -2;
  if (off_out)
    for (int i = 0; i < 4; ++i) off_out[i] = off[WVA_LP_F + i];
  void *up = nullptr;
  if (hipHostMalloc(&up, off[WVA_LP_F], hipHostMallocDefault) != hipSuccess) return -41;
  wva_lag_path_stage(in, off, (char *)up);
  hipStream_t s[WVA_LAG_CLASSES] = {(hipStream_t)stream, (hipStream_t)stream, (hipStream_t)stream,
                                    (hipStream_t)stream};
  hipEvent_t fork = nullptr;
  rc = hipEventCreateWithFlags(&fork, hipEventDisableTiming) == hipSuccess ? 0 : -10;
  if (rc == 0)
    rc = (int)hipMemcpyAsync(dev, up, off[WVA_LP_F], hipMemcpyHostToDevice, (hipStream_t)stream);
  if (rc == 0) rc = wva_lag_path_launch(in, off, (char *)dev, true, s, fork, nullptr);
  const int rs = (int)hipStreamSynchronize((hipStream_t)stream);
  if (fork) (void)hipEventDestroy(fork);
  (void)hipHostFree(up);
  return rc != 0 ? rc : rs;
}
