// wva_lag_path_wide.inc — lag paths for wide cells (WVA_LAG_MAX_N < N <=
// WVA_LAG_WIDE_MAX_N), included by wva_kernels.hip after wva_lag_path.inc and
// before the context runtime. The kernels are siblings of the wide-lag kernels
// of wva_lag.inc ("Wide lag": temporal tiling with overlapped halos), whose
// text they leave alone and whose step, window, weight, scan and reductions
// they call.
//
// A task is one RUN of a server on a wide cell (wva_lag_path.inc): consecutive
// ticks of one length dt, each at its own per-replica rate. The tiling is that
// of wva_lag_tile_t: slots g = n + pad0, tile b loads W = NT * C slots from
// b S - T on and owns [b S, (b + 1) S); v lives in HBM twice (launch l reads
// copy l & 1), acc once, the Poisson weight in a double-buffered per-task
// double written by tile 0; launch l runs segment l of every task that has
// one, and the kernel boundary is the only synchronisation. A segment never
// crosses a tick, so what a path needs falls on segment boundaries:
//
// 1. Per-tick coefficients. The segment names its tick j; {lam_j, keep_j} is
//    word [slot][j] of the descriptor array wva_lag_path_t reads (one 16-byte
//    uniform load per block; the segment record stays the 32-byte WvaLagSeg,
//    and a tick's rate is stored once, not once per segment). Lam_j = lam_j +
//    smax with smax from smax[task], which the init kernel wrote; up, dn_t,
//    stay_t, stay_last and the head waves' LDS table of dn / Lam_j are formed
//    from it at every launch, as wva_lag_tile_t forms them. Each lane reads
//    only the table words it wrote: no barrier.
// 2. Scale-out mixing on load. On a FIRST segment every loaded slot is
//    multiplied by keep_j and the lane that holds slot pad0 (state 0) adds
//    1 - keep_j, halo slots included: the mixing is pointwise, so each tile
//    whose window contains state 0 mixes its own copy. keep = 1 is exact (no
//    branch on it), and the padding stays exactly 0.
// 3. Records per tick. A LAST segment writes the tile's five partial
//    functionals; wva_lag_path_wide_fin sums them in tile order and writes the
//    records at [tick j][slot], with the device's own step count of the tick.
//
// No block runs more than T steps, so the run-time bound that chunking gives
// the one-block path holds by construction and there are no chunks here.

// per wide run, beside its WvaLagPathTask (whose carry is unused: -1); 48
// bytes, ops/sweep.py LAG_PATH_WIDE_DTYPE
struct WvaLagPathWideTask {
  double smax;         // the largest rate the host scheduled with
  long long slab;      // first double of the task's slab (filled by the plan)
  int tile0, n_tiles;  // its rows of the tile table
  int seg0, n_seg;     // its rows of the segment table (WvaLagSeg, j = the tick)
  int tick0, n_run;    // the run: ticks [tick0, tick0 + n_run)
  int start, pad;      // WVA_LAG_PATH_STATIONARY (at lam0) or WVA_LAG_PATH_EMPTY
};
static_assert(sizeof(WvaLagPathWideTask) == 48, "48-byte record");

struct WvaLagPathWideArgs {
  const WvaLagPathTask *tasks;
  const WvaLagPathWideTask *wide;
  const WvaLagSeg *segs;
  const WvaLagTile *tiles;
  const double2 *desc;  // [n_slots][n_ticks]: {lam (req/msec per replica), keep}
  double *slab;         // per task: v[2][G], acc[G], G = K + 1 + pad0
  double *part;         // [tile][5]: a tile's partial functionals
  double *wcarry;       // [task][2]: the Poisson weight between segments
  double *smax;         // [task]: the largest rate, written by the init kernel
  int *flag;            // [task]: not 0 = no model, the task's launches do nothing
  double dt;            // msec, every tick
  int n_ticks, n_slots, stride, halo;
  float *out_f;       // [6][n_ticks][n_slots]: ttft, itl, wait, blocked, rho, in_system
  uint8_t *violated;  // [n_ticks][n_slots]
  int *steps;         // [n_ticks][n_slots]: the tick's stencil steps, -1 without a model
  double *raw;        // [n_slots][n_ticks][5] or null (the probe), as WvaLagPathArgs.raw
};

#define WVA_LAG_SEQ() __builtin_amdgcn_sched_barrier(0)
#define WVA_LAG_VALID(n) ((n) >= 0 && (n) <= K)
#define WVA_LAG_RATE(n) wva_rate_exact(c, num_decode, (n) < 1 ? 1 : ((n) > N ? N : (n)))
#define WVA_LAG_DEATH(n) ((n) >= 1 && (n) <= K ? (double)WVA_LAG_RATE(n) : 0.0)
#define WVA_LAG_AT(j) ((size_t)(j) * (size_t)g.n_slots + (size_t)slot)
#define WVA_LAG_OUT(f, j) g.out_f[(size_t)(f) * (size_t)g.n_ticks * (size_t)g.n_slots + WVA_LAG_AT(j)]
#define WVA_LAG_RAW(j) (g.raw + ((size_t)slot * (size_t)g.n_ticks + (size_t)(j)) * WVA_LAG_FUNCS)
#define WVA_LAG_CELL(c, tp)  \
  WvaCell c;                 \
  c.in_tok = (tp)->in_tok;   \
  c.out_tok = (tp)->out_tok; \
  c.N = (tp)->N;             \
  c.alpha = (tp)->alpha;     \
  c.beta = (tp)->beta;       \
  c.gamma = (tp)->gamma;     \
  c.delta = (tp)->delta

// One block per (wide run, tile), one segment. The host checked every table
// (wva_lag_path_wide_plan); all control flow below is block-uniform and comes
// from the segment record.
template <int NT, int C>
__global__ void WVA_NO_PK_F32 __launch_bounds__(NT)
    wva_lag_path_tile_t(WvaLagPathWideArgs g, int tile_base, int launch) {
  constexpr int NW = NT / WVA_WAVE;
  extern __shared__ double wva_lag_path_tab[];  // [C][NT]: dn of the right neighbour (head waves)
  __shared__ double red[64];
  __shared__ double halo[2][2][NW];
  const int tid = (int)threadIdx.x;
  const WvaLagTile tl = g.tiles[tile_base + (int)blockIdx.x];
  const int task = tl.task, b = tl.b;
  if (g.flag[task] != 0) return;
  const WvaLagPathWideTask wt = g.wide[task];
  if (launch >= wt.n_seg) return;
  const WvaLagSeg sg = g.segs[wt.seg0 + launch];
  const WvaLagPathTask *const tp = g.tasks + task;
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

  // ---- this tick's stencil
  const double2 d = g.desc[(size_t)tp->slot * (size_t)g.n_ticks + (size_t)sg.j];
  const double lam = d.x, keep = d.y;
  const double Lam = lam + g.smax[task];
  const double sN = (double)wva_rate_exact(c, num_decode, N);
  const double up = lam / Lam;
  const double up_left = (n_first - 1 >= 0 && n_first - 1 < K) ? up : 0.0;
  const double up_last = n_first + C - 1 == K ? 0.0 : up;
  const double dn_t = sN / Lam;
  const double stay_t = fmax(1.0 - up - dn_t, 0.0);
  const double stay_last = n_first + C - 1 == K ? fmax(1.0 - dn_t, 0.0) : stay_t;
  // head waves: the waves whose first state is not above N (slots in front of
  // state 0 included: nothing may flow into them)
  const int wave_first = b * S - T + (tid / WVA_WAVE) * (WVA_WAVE * C) - pad0;
  const bool head = __builtin_amdgcn_readfirstlane(wave_first <= N ? 1 : 0) != 0;
  const double *const tab = wva_lag_path_tab + tid;
  double dn0 = 0.0;
  if (head) {
    dn0 = WVA_LAG_DEATH(n_first) / Lam;
#pragma unroll
    for (int i = 0; i < C; ++i) {
      wva_lag_path_tab[i * NT + tid] = WVA_LAG_DEATH(n_first + i + 1) / Lam;
      WVA_LAG_SEQ();
    }
  }

  // ---- the state: v from the copy this launch reads (mixed with the empty
  // replicas that joined, where the tick starts here), acc if the window is open
  const size_t sG = (size_t)G;
  const double *const vin = g.slab + wt.slab + (size_t)(launch & 1) * sG;
  double *const vout = g.slab + wt.slab + (size_t)((launch + 1) & 1) * sG;
  double *const accp = g.slab + wt.slab + 2 * sG;
  const int first = sg.first, count = sg.count, jlo = sg.jlo;
  const bool was_open = first > jlo;                       // acc and w come from before
  const bool opens = first <= jlo && jlo < first + count;  // the window opens in here
  const double mix = (sg.flags & WVA_LAG_SEG_FIRST) ? keep : 1.0;
  double v[C], acc[C];
#pragma unroll
  for (int i = 0; i < C; i += 2) {
    const double2 t = in_dom ? *(const double2 *)(vin + g0 + i) : make_double2(0.0, 0.0);
    v[i] = t.x * mix;
    v[i + 1] = t.y * mix;
    if (n_first + i == 0) v[i] += 1.0 - mix;
    if (n_first + i + 1 == 0) v[i + 1] += 1.0 - mix;
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
      // w(s) = w(s - 1) x / s, the quotient as wva_lag_t forms it
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

  // ---- the end of tick j: p = acc starts the next tick; the tile's partial
  // functionals over the states it owns
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

// One block per wide run: smax against the host's, bit for bit, then the start
// into copy 0 of the task's v: stationary at lam0, in log space as
// wva_lag_wide_init builds it, or all mass in state 0.
__global__ void __launch_bounds__(WVA_LAG_WIDE_NT)
    wva_lag_path_wide_init(WvaLagPathWideArgs g, int task0) {
  constexpr int NT = WVA_LAG_WIDE_NT, C = WVA_LAG_WIDE_C;
  __shared__ double red[64];
  const int tid = (int)threadIdx.x;
  const int task = task0 + (int)blockIdx.x;
  const WvaLagPathTask *const tp = g.tasks + task;
  const WvaLagPathWideTask wt = g.wide[task];
  const int slot = tp->slot;
  WVA_LAG_CELL(c, tp);
  const int N = c.N, K = 11 * N;
  const int pad0 = (C - (K + 1) % C) % C;
  const int G = K + 1 + pad0;
  const int num_decode = wva_num_decode(c);
  const double lam0 = tp->lam0;
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
  if (!(smax < (double)INFINITY) || !(smax > 0.0) || smax != wt.smax) {
    // degenerate rates, or not the smax the schedule was made for (uniform)
    if (tid == 0) g.flag[task] = 1;
    for (int j = wt.tick0 + tid; j < wt.tick0 + wt.n_run; j += NT) {
      for (int f = 0; f < WVA_LAG_FLOATS; ++f) WVA_LAG_OUT(f, j) = NAN;
      g.violated[WVA_LAG_AT(j)] = 0;
      g.steps[WVA_LAG_AT(j)] = -1;
      if (g.raw)
        for (int f = 0; f < WVA_LAG_FUNCS; ++f) WVA_LAG_RAW(j)[f] = NAN;
    }
    return;
  }
  if (tid == 0) {
    g.flag[task] = 0;
    g.smax[task] = smax;
  }
  if (wt.start != WVA_LAG_PATH_STATIONARY || !(lam0 > 0.0)) {
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
// closed a tick: the tile partials in tile order, then wva_lag_t's thread-0
// arithmetic into the records of [tick j][slot].
__global__ void __launch_bounds__(WVA_WAVE)
    wva_lag_path_wide_fin(WvaLagPathWideArgs g, int task0, int launch) {
  const int lane = (int)threadIdx.x;
  const int task = task0 + (int)blockIdx.x;
  if (g.flag[task] != 0) return;
  const WvaLagPathWideTask wt = g.wide[task];
  if (launch >= wt.n_seg) return;
  const WvaLagSeg sg = g.segs[wt.seg0 + launch];
  if (!(sg.flags & WVA_LAG_SEG_LAST)) return;
  const WvaLagPathTask *const tp = g.tasks + task;
  const int slot = tp->slot, j = sg.j;
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
  g.violated[WVA_LAG_AT(j)] = (t_ttft != 0.0f && ttft > t_ttft) || (t_itl != 0.0f && itl > t_itl);
  if (g.raw) {
    double *r = WVA_LAG_RAW(j);
    r[0] = f_blk;
    r[1] = f_srv;
    r[2] = f_sys;
    r[3] = f_tput;
    r[4] = wait;
  }
  // the device's own count of the tick's steps, as wva_lag_path_t reports it
  const double lam = g.desc[(size_t)slot * (size_t)g.n_ticks + (size_t)j].x;
  double jlo;
  const double total = wva_lag_window((lam + g.smax[task]) * g.dt, &jlo);
  g.steps[WVA_LAG_AT(j)] = total < 2147483000.0 ? (int)total : -1;
}
#undef WVA_LAG_SEQ
#undef WVA_LAG_VALID
#undef WVA_LAG_RATE
#undef WVA_LAG_DEATH
#undef WVA_LAG_AT
#undef WVA_LAG_OUT
#undef WVA_LAG_RAW
#undef WVA_LAG_CELL

// ---------------------------------------------------------------------------
// host: the tables of a wide path pass (ops/sweep.py lag_path_wide_schedule),
// their check, the device layout and the launches
// ---------------------------------------------------------------------------
struct WvaLagPathWideIn {
  const WvaLagPathTask *tasks;  // host [n_tasks], by descending n_seg
  WvaLagPathWideTask *wide;     // host [n_tasks]; slab is filled by the plan
  const WvaLagSeg *segs;        // host [n_segs]
  const WvaLagTile *tiles;      // host [n_tiles]
  const double *desc;           // host [n_slots][n_ticks][2]
  int n_tasks, n_segs, n_tiles, n_ticks, n_slots, stride, halo, max_steps;
  double dt;
};

// Every index a kernel will form lies inside its table, the segment chains
// partition each tick's steps, and the launch-prefix rule holds (tasks by
// descending n_seg, tiles and segments in task order). A task's slab is
// `arrays` x G doubles (3: v twice and acc; 4: avg too, wva_lag_path_avg_wide.inc).
// Fills wide[].slab round by round (a round's slabs fit `cap` bytes, a task
// larger than the cap runs alone) and returns the doubles the largest round
// needs in *slab_doubles. -2: a table is inconsistent.
static int wva_lag_path_wide_plan(const WvaLagPathWideIn &in, int arrays, size_t cap,
                                  size_t *slab_doubles) {
  const int C = WVA_LAG_WIDE_C, W = WVA_LAG_WIDE_NT * WVA_LAG_WIDE_C;
  const int S = in.stride, T = in.halo;
  if (!in.tasks || !in.wide || !in.segs || !in.tiles || !in.desc) return -2;
  if (in.n_tasks < 1 || in.n_ticks < 1 || in.n_slots < 1 || in.max_steps < 0 || !(in.dt > 0.0) ||
      !(in.dt < (double)INFINITY))
    return -2;
  if (S < C || T < C || S % C || T % C || S + 2 * T > W) return -2;
  int tile_at = 0, seg_at = 0;
  size_t round = 0, worst = 0;
  for (int i = 0; i < in.n_tasks; ++i) {
    const WvaLagPathTask &t = in.tasks[i];
    WvaLagPathWideTask &w = in.wide[i];
    if (t.N <= WVA_LAG_MAX_N || t.N > WVA_LAG_WIDE_MAX_N) return -2;
    if (t.slot < 0 || t.slot >= in.n_slots) return -2;
    if (w.tick0 < 0 || w.n_run < 1 || w.tick0 > in.n_ticks - w.n_run) return -2;
    if (w.start != WVA_LAG_PATH_STATIONARY && w.start != WVA_LAG_PATH_EMPTY) return -2;
    if (!(w.smax > 0.0) || !(w.smax < (double)INFINITY)) return -2;
    const int G = wva_lag_wide_slots(t.N);
    if (w.tile0 != tile_at || w.n_tiles != (G + S - 1) / S || w.n_tiles > in.n_tiles - tile_at)
      return -2;
    for (int b = 0; b < w.n_tiles; ++b)
      if (in.tiles[tile_at + b].task != i || in.tiles[tile_at + b].b != b) return -2;
    tile_at += w.n_tiles;
    if (w.seg0 != seg_at || w.n_seg < 1 || w.n_seg > in.n_segs - seg_at) return -2;
    if (i > 0 && w.n_seg > in.wide[i - 1].n_seg) return -2;
    const double *const desc = in.desc + ((size_t)t.slot * (size_t)in.n_ticks) * 2;
    int j = w.tick0, done = 0;
    for (int l = 0; l < w.n_seg; ++l) {
      const WvaLagSeg &s = in.segs[seg_at + l];
      if (j >= w.tick0 + w.n_run) return -2;  // segments past the run
      if (s.j != j || s.first != done || s.count < 1 || s.count > T) return -2;
      if (s.jlo < 0 || s.jlo >= s.jhi || s.jhi > in.max_steps || done + s.count > s.jhi)
        return -2;
      const double lam = desc[2 * j], keep = desc[2 * j + 1];
      if (!(lam >= 0.0) || !(lam < (double)INFINITY) || !(keep >= 0.0) || !(keep <= 1.0))
        return -2;
      done += s.count;
      const bool last = done == s.jhi;
      const int want = (s.first == 0 ? WVA_LAG_SEG_FIRST : 0) | (last ? WVA_LAG_SEG_LAST : 0) |
                       (last && j == w.tick0 + w.n_run - 1 ? WVA_LAG_SEG_FINAL : 0);
      if (s.flags != want) return -2;
      if (last) {
        ++j;
        done = 0;
      }
    }
    if (j != w.tick0 + w.n_run || done != 0) return -2;
    seg_at += w.n_seg;
    const size_t need = (size_t)arrays * (size_t)G;
    if (round > 0 && (round + need) * sizeof(double) > cap) round = 0;  // a new round
    w.slab = (long long)round;
    round += need;
    worst = round > worst ? round : worst;
  }
  if (tile_at != in.n_tiles || seg_at != in.n_segs) return -2;
  *slab_doubles = worst;
  return 0;
}

// the device layout: the five tables as one upload, the three records (and the
// probe's raw functionals) as one download, then scratch
enum {
  WVA_LPW_TASKS, WVA_LPW_WIDE, WVA_LPW_SEGS, WVA_LPW_TILES, WVA_LPW_DESC,  // up
  WVA_LPW_F, WVA_LPW_VIOL, WVA_LPW_STEPS, WVA_LPW_RAW,                     // down
  WVA_LPW_PART, WVA_LPW_WCARRY, WVA_LPW_SMAX, WVA_LPW_FLAG, WVA_LPW_SLAB, WVA_LPW_N
};
static size_t wva_lag_path_wide_layout(const WvaLagPathWideIn &in, size_t slab_doubles, bool raw,
                                       size_t *off) {
  const size_t cells = (size_t)in.n_ticks * (size_t)in.n_slots, n = (size_t)in.n_tasks;
  const size_t sizes[WVA_LPW_N] = {
      n * sizeof(WvaLagPathTask), n * sizeof(WvaLagPathWideTask),
      (size_t)in.n_segs * sizeof(WvaLagSeg), (size_t)in.n_tiles * sizeof(WvaLagTile),
      cells * 2 * sizeof(double), WVA_LAG_FLOATS * cells * sizeof(float), cells,
      cells * sizeof(int), raw ? cells * WVA_LAG_FUNCS * sizeof(double) : 0,
      (size_t)in.n_tiles * WVA_LAG_FUNCS * sizeof(double), 2 * n * sizeof(double),
      n * sizeof(double), n * sizeof(int), slab_doubles * sizeof(double)};
  return wva_arena_layout(sizes, WVA_LPW_N, off);
}

static void wva_lag_path_wide_stage(const WvaLagPathWideIn &in, const size_t *off, char *up) {
  memcpy(up + off[WVA_LPW_TASKS], in.tasks, (size_t)in.n_tasks * sizeof(WvaLagPathTask));
  memcpy(up + off[WVA_LPW_WIDE], in.wide, (size_t)in.n_tasks * sizeof(WvaLagPathWideTask));
  memcpy(up + off[WVA_LPW_SEGS], in.segs, (size_t)in.n_segs * sizeof(WvaLagSeg));
  memcpy(up + off[WVA_LPW_TILES], in.tiles, (size_t)in.n_tiles * sizeof(WvaLagTile));
  memcpy(up + off[WVA_LPW_DESC], in.desc,
         (size_t)in.n_ticks * (size_t)in.n_slots * 2 * sizeof(double));
}

// the launch order of a staged pass: per round init(tasks, first task), then
// per l step(tiles, first tile, l) over the tiles of the tasks that have a
// segment l (a prefix: tasks are by descending n_seg) and fin(live tasks, first
// task, l) if one of them closed a tick. launches[3] (or null): init, step and
// fin launches made.
template <typename I, typename S, typename F>
static int wva_lag_path_wide_rounds(const WvaLagPathWideIn &in, int *launches, I init, S step,
                                    F fin) {
  int made[3] = {0, 0, 0};
  for (int t0 = 0; t0 < in.n_tasks;) {
    int t1 = t0 + 1;  // the round: up to the next task whose slab starts over
    while (t1 < in.n_tasks && in.wide[t1].slab != 0) ++t1;
    init(t1 - t0, t0);
    ++made[0];
    int live = t1 - t0;  // tasks of the round with a segment l
    for (int l = 0; l < in.wide[t0].n_seg; ++l) {
      while (in.wide[t0 + live - 1].n_seg <= l) --live;
      const WvaLagPathWideTask &end = in.wide[t0 + live - 1];
      const int tile_base = in.wide[t0].tile0;
      step(end.tile0 + end.n_tiles - tile_base, tile_base, l);
      ++made[1];
      bool closes = false;
      for (int i = t0; i < t0 + live && !closes; ++i)
        closes = (in.segs[in.wide[i].seg0 + l].flags & WVA_LAG_SEG_LAST) != 0;
      if (closes) {
        fin(live, t0, l);
        ++made[2];
      }
    }
    const int rc = (int)hipGetLastError();
    if (rc != 0) return rc;
    t0 = t1;
  }
  if (launches)
    for (int i = 0; i < 3; ++i) launches[i] = made[i];
  return 0;
}

// the launches of a staged pass, stream-ordered on s
static int wva_lag_path_wide_launch(const WvaLagPathWideIn &in, const size_t *off, char *d,
                                    bool raw, hipStream_t s, int *launches) {
  constexpr int NT = WVA_LAG_WIDE_NT, C = WVA_LAG_WIDE_C;
  const size_t lds = (size_t)NT * C * sizeof(double);
  int rc = wva_optin_lds((const void *)wva_lag_path_tile_t<NT, C>, lds);
  if (rc != 0) return rc;
  WvaLagPathWideArgs g = {};
  g.tasks = (const WvaLagPathTask *)(d + off[WVA_LPW_TASKS]);
  g.wide = (const WvaLagPathWideTask *)(d + off[WVA_LPW_WIDE]);
  g.segs = (const WvaLagSeg *)(d + off[WVA_LPW_SEGS]);
  g.tiles = (const WvaLagTile *)(d + off[WVA_LPW_TILES]);
  g.desc = (const double2 *)(d + off[WVA_LPW_DESC]);
  g.slab = (double *)(d + off[WVA_LPW_SLAB]);
  g.part = (double *)(d + off[WVA_LPW_PART]);
  g.wcarry = (double *)(d + off[WVA_LPW_WCARRY]);
  g.smax = (double *)(d + off[WVA_LPW_SMAX]);
  g.flag = (int *)(d + off[WVA_LPW_FLAG]);
  g.dt = in.dt;
  g.n_ticks = in.n_ticks;
  g.n_slots = in.n_slots;
  g.stride = in.stride;
  g.halo = in.halo;
  g.out_f = (float *)(d + off[WVA_LPW_F]);
  g.violated = (uint8_t *)(d + off[WVA_LPW_VIOL]);
  g.steps = (int *)(d + off[WVA_LPW_STEPS]);
  g.raw = raw ? (double *)(d + off[WVA_LPW_RAW]) : nullptr;
  return wva_lag_path_wide_rounds(
      in, launches,
      [&](int n, int t0) {
        hipLaunchKernelGGL(wva_lag_path_wide_init, dim3(n), dim3(NT), 0, s, g, t0);
      },
      [&](int n_tiles, int tile_base, int l) {
        hipLaunchKernelGGL((wva_lag_path_tile_t<NT, C>), dim3(n_tiles), dim3(NT), lds, s, g,
                           tile_base, l);
      },
      [&](int n, int t0, int l) {
        hipLaunchKernelGGL(wva_lag_path_wide_fin, dim3(n), dim3(WVA_WAVE), 0, s, g, t0, l);
      });
}

// One-shot probe of the wide path kernels for tests and tools, the sibling of
// wva_lag_wide_probe_launch with (stride, halo) as arguments: dev = null asks
// for the device bytes (*need), then a 256-aligned device buffer of that size
// runs the pass on `stream` and synchronises it. off_out[4]: where in dev the
// fp32 records, violated, steps and the raw functionals [slot][n_ticks][5] lie.
extern "C" int wva_lag_path_wide_probe_launch(const void *tasks, void *wide, const void *segs,
                                              const void *tiles, const double *desc, int n_tasks,
                                              int n_segs, int n_tiles, int n_ticks, int n_slots,
                                              int max_steps, int stride, int halo, double dt,
                                              void *stream, void *dev, size_t dev_bytes,
                                              size_t *need, size_t *off_out) {
  WvaLagPathWideIn in = {(const WvaLagPathTask *)tasks, (WvaLagPathWideTask *)wide,
                         (const WvaLagSeg *)segs, (const WvaLagTile *)tiles, desc, n_tasks,
                         n_segs, n_tiles, n_ticks, n_slots, stride, halo, max_steps, dt};
  size_t slab = 0, off[WVA_LPW_N];
  int rc = wva_lag_path_wide_plan(in, 3, WVA_LAG_WIDE_SLAB_CAP, &slab);
  if (rc != 0) return rc;
  const size_t bytes = wva_lag_path_wide_layout(in, slab, true, off);
  if (need) *need = bytes;
  if (dev == nullptr) return 0;
  if (dev_bytes < bytes || ((uintptr_t)dev & 255) != 0) return -2;
  if (off_out)
    for (int i = 0; i < 4; ++i) off_out[i] = off[WVA_LPW_F + i];
  void *up = nullptr;
  if (hipHostMalloc(&up, off[WVA_LPW_F], hipHostMallocDefault) != hipSuccess) return -41;
  wva_lag_path_wide_stage(in, off, (char *)up);
  rc = (int)hipMemcpyAsync(dev, up, off[WVA_LPW_F], hipMemcpyHostToDevice, (hipStream_t)stream);
  if (rc == 0)
    rc = wva_lag_path_wide_launch(in, off, (char *)dev, true, (hipStream_t)stream, nullptr);
  const int rs = (int)hipStreamSynchronize((hipStream_t)stream);
  (void)hipHostFree(up);
  return rc != 0 ? rc : rs;
}
