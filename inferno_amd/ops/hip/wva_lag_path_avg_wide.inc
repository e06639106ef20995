// wva_lag_path_avg_wide.inc — lag path averages for wide cells (WVA_LAG_MAX_N
// < N <= WVA_LAG_WIDE_MAX_N): beside the state at the end of every tick
// (wva_lag_path_wide.inc) the TIME AVERAGE of the distribution over the tick
// (wva_lag_path_avg.inc), included by wva_kernels.hip after
// wva_lag_path_wide.inc and before the context runtime. The kernels are
// siblings of the wide path kernels, whose text they leave alone and whose
// step, window, weight, functionals and reductions they call.
//
// The quantity is that of wva_lag_path_avg.inc. With x = Lam_j dt and v_k the
// vector after k steps of tick j (v_0 after the scale-out mixing),
//   pbar = (1 / x) sum_{k = 0..j_hi} T_k v_k,
//   T_k = 1 below the window, T_lo = max(1 - w_lo, 0),
//   T_k = max(T_{k - 1} - w_k, 0) inside it,
// with the weights w_k the end-state sum forms anyway. The functionals and the
// targets are applied to pbar as to the end state, the 1 / x after the sums.
//
// Why a second block. The one-block kernel keeps the sum in the dead acc
// registers below the window and in a 96 KiB lane-private LDS slab inside it.
// The tile kernel <512, 24> already holds a 96 KiB table of dn for its head
// waves (96 + 96 KiB do not fit the CU's 160 KiB), and v and acc are 96 of its
// 238 VGPRs, so a third 48-register array does not fit either. A window
// segment needs two accumulators over the same sequence v_k, so it gets two
// blocks, each with the tile kernel's register budget; below the window acc is
// dead and one block does both jobs.
//
// wva_lag_path_avg_tile_t<512, 24> runs on grid (tiles of the launch, 2) with
// the tables, tiling, launches and 96 KiB table of wva_lag_path_tile_t. A
// task's slab is 4 G doubles: v twice, acc, and avg (owned slots only). Beside
// wcarry[task][2] there is tcarry[task][2], the double-buffered T_k between the
// segments of a window, and beside part[tile][5] there is part_avg[tile][5].
// Per segment exactly one of the two blocks owns the avg slab; which one
// follows from the segment record alone (is first + count <= jlo?), so it is
// block-uniform and no block waits for another.
//
// State block (blockIdx.y == 0). Everything wva_lag_path_tile_t does, to the
// bit: mixing on a FIRST segment, per-tick coefficients and head table, v to
// the other copy, acc and wcarry, the partials at a LAST segment. On a segment
// wholly below the window (first + count <= jlo) acc is dead; there it holds
// the averaged sum: seeded with the mixed v_0 on a FIRST segment, else loaded
// from the avg slab, advanced by the ACC step at weight 1 (v_k enters after
// step k, before step k + 1: the golden's order), stored to the avg slab at
// the end. On a segment that touches the window it leaves the avg slab alone.
//
// Average block (blockIdx.y == 1). Returns at once on a segment wholly below
// the window. On a segment that touches it: the same v copy with the same
// mixing; the avg slab into its acc registers (a FIRST segment seeds v_0, with
// jlo = 0 T_0 v_0); the segment's plain steps again at weight 1 up to jlo; T_lo
// on the vector where the window opens; the window steps as ACC steps at
// weight T_k. w_k advances by the state block's recurrence (hardware
// reciprocal, two Newton steps, w *= x rs) from wcarry[launch & 1], which the
// PREVIOUS launch wrote; T from tcarry[launch & 1]; tile 0 writes
// tcarry[(launch + 1) & 1]. It stores the avg slab (owned slots) and, on a
// LAST segment, the five partial functionals of the sum over its owned slots
// to part_avg. It never writes v, acc, wcarry or part.
// (Where the window opens exactly at a segment's start, jlo = first > 0, the
// vector v_jlo was added by the segment before, at weight 1: for jlo > 0 the
// weight w_lo is below e^-60, so T_lo = max(1 - w_lo, 0) rounds to exactly 1.)
//
// No word is read and written by two blocks of a launch: both read v copy
// launch & 1; the state block writes the other copy, acc, wcarry[(launch + 1)
// & 1] and part; the average block writes avg, tcarry[(launch + 1) & 1] and
// part_avg; on a below-window segment the state block is the only one that
// touches avg. The kernel boundary is the only synchronisation, as before.
//
// wva_lag_path_wide_init is reused as it stands (copy 0 only).
// wva_lag_path_avg_wide_fin forms the end-state records as
// wva_lag_path_wide_fin does, from the same partials in the same order, and
// the averaged records from part_avg in tile order.

struct WvaLagPathWideAvgArgs {
  WvaLagPathWideArgs a;   // slab per task: v[2][G], acc[G], avg[G]
  double *part_avg;       // [tile][5]: a tile's partial functionals of x pbar
  double *tcarry;         // [task][2]: T_k between segments
  float *avg_f;           // [6][n_ticks][n_slots], as a.out_f, of pbar
  uint8_t *avg_violated;  // [n_ticks][n_slots]
  double *avg_raw;        // [n_slots][n_ticks][5] or null (the probe)
};

#define WVA_LAG_SEQ() __builtin_amdgcn_sched_barrier(0)
#define WVA_LAG_RATE(n) wva_rate_exact(c, num_decode, (n) < 1 ? 1 : ((n) > N ? N : (n)))
#define WVA_LAG_DEATH(n) ((n) >= 1 && (n) <= K ? (double)WVA_LAG_RATE(n) : 0.0)
#define WVA_LAG_AT(j) ((size_t)(j) * (size_t)g.n_slots + (size_t)slot)
#define WVA_LAG_RAW(base, j) \
  ((base) + ((size_t)slot * (size_t)g.n_ticks + (size_t)(j)) * WVA_LAG_FUNCS)
#define WVA_LAG_CELL(c, tp)  \
  WvaCell c;                 \
  c.in_tok = (tp)->in_tok;   \
  c.out_tok = (tp)->out_tok; \
  c.N = (tp)->N;             \
  c.alpha = (tp)->alpha;     \
  c.beta = (tp)->beta;       \
  c.gamma = (tp)->gamma;     \
  c.delta = (tp)->delta

// Two blocks per (wide run, tile), one segment. The host checked every table
// (wva_lag_path_wide_plan); all control flow below is block-uniform and comes
// from the segment record and blockIdx.y.
template <int NT, int C>
__global__ void WVA_NO_PK_F32 __launch_bounds__(NT)
    wva_lag_path_avg_tile_t(WvaLagPathWideAvgArgs ga, int tile_base, int launch) {
  constexpr int NW = NT / WVA_WAVE;
  extern __shared__ double wva_lag_path_avg_tab[];  // [C][NT]: dn of the right neighbour (head waves)
  __shared__ double red[64];
  __shared__ double halo[2][2][NW];
  const WvaLagPathWideArgs &g = ga.a;
  const int tid = (int)threadIdx.x;
  const bool avg_blk = blockIdx.y != 0;
  const WvaLagTile tl = g.tiles[tile_base + (int)blockIdx.x];
  const int task = tl.task, b = tl.b;
  if (g.flag[task] != 0) return;
  const WvaLagPathWideTask wt = g.wide[task];
  if (launch >= wt.n_seg) return;
  const WvaLagSeg sg = g.segs[wt.seg0 + launch];
  const int first = sg.first, count = sg.count, jlo = sg.jlo;
  const bool below = first + count <= jlo;  // the segment ends below the window
  if (avg_blk && below) return;             // the state block owns avg here
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

  // ---- this tick's stencil, as wva_lag_path_tile_t forms it
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
  const int wave_first = b * S - T + (tid / WVA_WAVE) * (WVA_WAVE * C) - pad0;
  const bool head = __builtin_amdgcn_readfirstlane(wave_first <= N ? 1 : 0) != 0;
  const double *const tab = wva_lag_path_avg_tab + tid;
  double dn0 = 0.0;
  if (head) {
    dn0 = WVA_LAG_DEATH(n_first) / Lam;
#pragma unroll
    for (int i = 0; i < C; ++i) {
      wva_lag_path_avg_tab[i * NT + tid] = WVA_LAG_DEATH(n_first + i + 1) / Lam;
      WVA_LAG_SEQ();
    }
  }

  // ---- the state: v from the copy this launch reads, mixed where the tick
  // starts here; the second register array holds acc (the state block on a
  // segment that touches the window) or the averaged sum (everywhere else)
  const size_t sG = (size_t)G;
  const double *const vin = g.slab + wt.slab + (size_t)(launch & 1) * sG;
  double *const vout = g.slab + wt.slab + (size_t)((launch + 1) & 1) * sG;
  double *const accp = g.slab + wt.slab + 2 * sG;
  double *const avgp = g.slab + wt.slab + 3 * sG;
  const bool is_first = (sg.flags & WVA_LAG_SEG_FIRST) != 0;
  const bool was_open = first > jlo;                       // acc, w and T come from before
  const bool opens = first <= jlo && jlo < first + count;  // the window opens in here
  const bool holds_avg = avg_blk || below;
  const double mix = is_first ? keep : 1.0;
  double v[C], acc[C];
#pragma unroll
  for (int i = 0; i < C; i += 2) {
    const double2 t = in_dom ? *(const double2 *)(vin + g0 + i) : make_double2(0.0, 0.0);
    v[i] = t.x * mix;
    v[i + 1] = t.y * mix;
    if (n_first + i == 0) v[i] += 1.0 - mix;
    if (n_first + i + 1 == 0) v[i + 1] += 1.0 - mix;
  }
  {
    const double *const src = holds_avg ? avgp : accp;
    const bool load = owned && (holds_avg ? !is_first : was_open);
#pragma unroll
    for (int i = 0; i < C; i += 2) {
      const double2 t = load ? *(const double2 *)(src + g0 + i) : make_double2(0.0, 0.0);
      acc[i] = t.x;
      acc[i + 1] = t.y;
    }
  }
  const double x = sg.x;

  // ---- the steps, in the two loops of wva_lag_path_tile_t. Plain steps: only
  // the state block on a segment that touches the window, up to jlo (its acc
  // is not live yet). Every other step is an ACC step whose block-uniform
  // weight says what the second array sums:
  //   state block, window:        w_s                    (acc, the end state)
  //   state block, below it:      1                      (avg)
  //   average block:              1, T_lo at jlo, T_s    (avg)
  int plain = !holds_avg ? jlo - first : 0;
  plain = plain < 0 ? 0 : plain;
  int buf = 0;
  for (int s = 0; s < plain; ++s)
    wva_lag_tile_step<NT, C, false>(v, acc, head, tab, dn0, up, up_last, up_left, stay_t, dn_t,
                                    stay_last, 0.0, halo, buf);
  double w = 0.0, tk = 1.0;
  if (was_open) {
    w = g.wcarry[2 * task + (launch & 1)];
    if (avg_blk) tk = ga.tcarry[2 * task + (launch & 1)];
  }
  if (opens) w = exp(wva_lag_pois_log_pmf((double)jlo, x));
  if (avg_blk && opens && first == jlo) tk = fmax(1.0 - w, 0.0);  // T_lo of the vector loaded
  // the seed: w_lo v where the state block's window opens; v_0 at the start of
  // the tick for avg (T_0 v_0 with jlo = 0)
  const bool seed = holds_avg ? is_first : opens;
  if (seed) {
    const double sw = !holds_avg ? w : (avg_blk && jlo == 0 ? tk : 1.0);
#pragma unroll
    for (int i = 0; i < C; ++i) acc[i] = sw * v[i];
  }
  w = wva_lag_uniform(w);
  tk = wva_lag_uniform(tk);
  for (int s = first + plain + 1; s <= first + count; ++s) {
    if (s > jlo) {
      // w(s) = w(s - 1) x / s, the quotient as wva_lag_t forms it
      const double sd = (double)s;
      double rs = __builtin_amdgcn_rcp(sd);
      rs = fma(fma(-sd, rs, 1.0), rs, rs);
      rs = fma(fma(-sd, rs, 1.0), rs, rs);
      w *= x * rs;
    }
    // T_s = max(T_{s - 1} - w_s, 0) from jlo on (T = 1 before, w_lo at jlo)
    if (avg_blk && s >= jlo) tk = wva_lag_uniform(fmax(tk - w, 0.0));
    const double wk = avg_blk ? tk : (below ? 1.0 : w);
    wva_lag_tile_step<NT, C, true>(v, acc, head, tab, dn0, up, up_last, up_left, stay_t, dn_t,
                                   stay_last, wk, halo, buf);
  }
  if (!below && b == 0 && tid == 0) {
    if (avg_blk) ga.tcarry[2 * task + ((launch + 1) & 1)] = tk;
    else g.wcarry[2 * task + ((launch + 1) & 1)] = w;
  }

  // ---- the end of tick j (never below the window): the tile's partial
  // functionals over the states it owns, of the end state p = acc, which
  // starts the next tick (state block), or of x pbar (average block)
  if (sg.flags & WVA_LAG_SEG_LAST) {
    int n_base = n_first;
    asm volatile("" : "+v"(n_base));
    double f[WVA_LAG_FUNCS];
    wva_lag_path_funcs<NT, C>([&](int i) { return owned ? acc[i] : 0.0; }, n_base, c, num_decode,
                              red, f);
#pragma unroll
    for (int i = 0; i < C; ++i) v[i] = acc[i];
    if (tid == 0) {
      double *p = (avg_blk ? ga.part_avg : g.part) +
                  (size_t)(tile_base + (int)blockIdx.x) * WVA_LAG_FUNCS;
#pragma unroll
      for (int i = 0; i < WVA_LAG_FUNCS; ++i) p[i] = f[i];
    }
  } else if (owned) {
    double *const dst = holds_avg ? avgp : accp;
#pragma unroll
    for (int i = 0; i < C; i += 2) *(double2 *)(dst + g0 + i) = make_double2(acc[i], acc[i + 1]);
  }
  if (owned && !avg_blk) {
#pragma unroll
    for (int i = 0; i < C; i += 2) *(double2 *)(vout + g0 + i) = make_double2(v[i], v[i + 1]);
  }
}

// One wave per task of the launch; does something only where segment `launch`
// closed a tick: both sets of tile partials in tile order, then the end-state
// record of wva_lag_path_wide_fin and the record of pbar (the sums over x) at
// [tick j][slot]. A task without a model gets NaN averages here, as the init
// kernel gave it NaN end states.
__global__ void __launch_bounds__(WVA_WAVE)
    wva_lag_path_avg_wide_fin(WvaLagPathWideAvgArgs ga, int task0, int launch) {
  const WvaLagPathWideArgs &g = ga.a;
  const int lane = (int)threadIdx.x;
  const int task = task0 + (int)blockIdx.x;
  const WvaLagPathWideTask wt = g.wide[task];
  if (launch >= wt.n_seg) return;
  const WvaLagSeg sg = g.segs[wt.seg0 + launch];
  if (!(sg.flags & WVA_LAG_SEG_LAST)) return;
  const WvaLagPathTask *const tp = g.tasks + task;
  const int slot = tp->slot, j = sg.j;
  const size_t stride = (size_t)g.n_ticks * (size_t)g.n_slots;
  if (g.flag[task] != 0) {
    if (lane == 0) {
      for (int f = 0; f < WVA_LAG_FLOATS; ++f) ga.avg_f[(size_t)f * stride + WVA_LAG_AT(j)] = NAN;
      ga.avg_violated[WVA_LAG_AT(j)] = 0;
      if (ga.avg_raw)
        for (int f = 0; f < WVA_LAG_FUNCS; ++f) WVA_LAG_RAW(ga.avg_raw, j)[f] = NAN;
    }
    return;
  }
  WVA_LAG_CELL(c, tp);
  const int N = c.N;
  double sum = 0.0, sum_a = 0.0;
  if (lane < WVA_LAG_FUNCS)
    for (int t = 0; t < wt.n_tiles; ++t) {
      sum += g.part[(size_t)(wt.tile0 + t) * WVA_LAG_FUNCS + lane];
      sum_a += ga.part_avg[(size_t)(wt.tile0 + t) * WVA_LAG_FUNCS + lane];
    }
  double f_end[WVA_LAG_FUNCS], f_avg[WVA_LAG_FUNCS];
#pragma unroll
  for (int i = 0; i < WVA_LAG_FUNCS; ++i) {
    f_end[i] = __shfl(sum, i, WVA_WAVE);
    f_avg[i] = __shfl(sum_a, i, WVA_WAVE);
  }
  if (lane != 0) return;
  const double sN = (double)wva_rate_exact(c, wva_num_decode(c), N);
  const float t_ttft = tp->t_ttft, t_itl = tp->t_itl;
  wva_lag_path_record(f_end, 1.0, sN, c, t_ttft, t_itl, g.out_f + WVA_LAG_AT(j), stride,
                      g.violated + WVA_LAG_AT(j), g.raw ? WVA_LAG_RAW(g.raw, j) : nullptr);
  wva_lag_path_record(f_avg, sg.x, sN, c, t_ttft, t_itl, ga.avg_f + WVA_LAG_AT(j), stride,
                      ga.avg_violated + WVA_LAG_AT(j),
                      ga.avg_raw ? WVA_LAG_RAW(ga.avg_raw, j) : nullptr);
  // the device's own count of the tick's steps, as wva_lag_path_wide_fin reports it
  const double lam = g.desc[(size_t)slot * (size_t)g.n_ticks + (size_t)j].x;
  double jlo;
  const double total = wva_lag_window((lam + g.smax[task]) * g.dt, &jlo);
  g.steps[WVA_LAG_AT(j)] = total < 2147483000.0 ? (int)total : -1;
}
#undef WVA_LAG_SEQ
#undef WVA_LAG_RATE
#undef WVA_LAG_DEATH
#undef WVA_LAG_AT
#undef WVA_LAG_RAW
#undef WVA_LAG_CELL

// ---------------------------------------------------------------------------
// host: wva_lag_path_wide.inc's tables, plan (at 4 G doubles per task), staging
// and launch order; larger output and scratch blocks
// ---------------------------------------------------------------------------
// the device layout: the five tables as one upload (as WVA_LPW_*), the
// end-state and the averaged records (and the probe's raw functionals) as one
// download, then scratch
enum {
  WVA_LPWA_TASKS, WVA_LPWA_WIDE, WVA_LPWA_SEGS, WVA_LPWA_TILES, WVA_LPWA_DESC,     // up
  WVA_LPWA_F, WVA_LPWA_VIOL, WVA_LPWA_STEPS, WVA_LPWA_AF, WVA_LPWA_AVIOL,          // down
  WVA_LPWA_RAW, WVA_LPWA_ARAW,                                                      // down (the probe)
  WVA_LPWA_PART, WVA_LPWA_APART, WVA_LPWA_WCARRY, WVA_LPWA_TCARRY, WVA_LPWA_SMAX,
  WVA_LPWA_FLAG, WVA_LPWA_SLAB, WVA_LPWA_N
};
static_assert(WVA_LPWA_TASKS == WVA_LPW_TASKS && WVA_LPWA_WIDE == WVA_LPW_WIDE &&
                  WVA_LPWA_SEGS == WVA_LPW_SEGS && WVA_LPWA_TILES == WVA_LPW_TILES &&
                  WVA_LPWA_DESC == WVA_LPW_DESC,
              "wva_lag_path_wide_stage fills the upload of both layouts");
static size_t wva_lag_path_avg_wide_layout(const WvaLagPathWideIn &in, size_t slab_doubles,
                                           bool raw, size_t *off) {
  const size_t cells = (size_t)in.n_ticks * (size_t)in.n_slots, n = (size_t)in.n_tasks;
  const size_t raw_bytes = raw ? cells * WVA_LAG_FUNCS * sizeof(double) : 0;
  const size_t part_bytes = (size_t)in.n_tiles * WVA_LAG_FUNCS * sizeof(double);
  const size_t sizes[WVA_LPWA_N] = {
      n * sizeof(WvaLagPathTask), n * sizeof(WvaLagPathWideTask),
      (size_t)in.n_segs * sizeof(WvaLagSeg), (size_t)in.n_tiles * sizeof(WvaLagTile),
      cells * 2 * sizeof(double), WVA_LAG_FLOATS * cells * sizeof(float), cells,
      cells * sizeof(int), WVA_LAG_FLOATS * cells * sizeof(float), cells, raw_bytes, raw_bytes,
      part_bytes, part_bytes, 2 * n * sizeof(double), 2 * n * sizeof(double), n * sizeof(double),
      n * sizeof(int), slab_doubles * sizeof(double)};
  return wva_arena_layout(sizes, WVA_LPWA_N, off);
}

// wva_lag_path_wide_launch for the averaged kernels: the same rounds and
// launch prefixes, two blocks per tile, the records at the offsets of
// wva_lag_path_avg_wide_layout
static int wva_lag_path_avg_wide_launch(const WvaLagPathWideIn &in, const size_t *off, char *d,
                                        bool raw, hipStream_t s, int *launches) {
  constexpr int NT = WVA_LAG_WIDE_NT, C = WVA_LAG_WIDE_C;
  const size_t lds = (size_t)NT * C * sizeof(double);
  const int rc = wva_optin_lds((const void *)wva_lag_path_avg_tile_t<NT, C>, lds);
  if (rc != 0) return rc;
  WvaLagPathWideAvgArgs g = {};
  g.a.tasks = (const WvaLagPathTask *)(d + off[WVA_LPWA_TASKS]);
  g.a.wide = (const WvaLagPathWideTask *)(d + off[WVA_LPWA_WIDE]);
  g.a.segs = (const WvaLagSeg *)(d + off[WVA_LPWA_SEGS]);
  g.a.tiles = (const WvaLagTile *)(d + off[WVA_LPWA_TILES]);
  g.a.desc = (const double2 *)(d + off[WVA_LPWA_DESC]);
  g.a.slab = (double *)(d + off[WVA_LPWA_SLAB]);
  g.a.part = (double *)(d + off[WVA_LPWA_PART]);
  g.a.wcarry = (double *)(d + off[WVA_LPWA_WCARRY]);
  g.a.smax = (double *)(d + off[WVA_LPWA_SMAX]);
  g.a.flag = (int *)(d + off[WVA_LPWA_FLAG]);
  g.a.dt = in.dt;
  g.a.n_ticks = in.n_ticks;
  g.a.n_slots = in.n_slots;
  g.a.stride = in.stride;
  g.a.halo = in.halo;
  g.a.out_f = (float *)(d + off[WVA_LPWA_F]);
  g.a.violated = (uint8_t *)(d + off[WVA_LPWA_VIOL]);
  g.a.steps = (int *)(d + off[WVA_LPWA_STEPS]);
  g.a.raw = raw ? (double *)(d + off[WVA_LPWA_RAW]) : nullptr;
  g.part_avg = (double *)(d + off[WVA_LPWA_APART]);
  g.tcarry = (double *)(d + off[WVA_LPWA_TCARRY]);
  g.avg_f = (float *)(d + off[WVA_LPWA_AF]);
  g.avg_violated = (uint8_t *)(d + off[WVA_LPWA_AVIOL]);
  g.avg_raw = raw ? (double *)(d + off[WVA_LPWA_ARAW]) : nullptr;
  return wva_lag_path_wide_rounds(
      in, launches,
      [&](int n, int t0) {
        hipLaunchKernelGGL(wva_lag_path_wide_init, dim3(n), dim3(NT), 0, s, g.a, t0);
      },
      [&](int n_tiles, int tile_base, int l) {
        hipLaunchKernelGGL((wva_lag_path_avg_tile_t<NT, C>), dim3(n_tiles, 2), dim3(NT), lds, s, g,
                           tile_base, l);
      },
      [&](int n, int t0, int l) {
        hipLaunchKernelGGL(wva_lag_path_avg_wide_fin, dim3(n), dim3(WVA_WAVE), 0, s, g, t0, l);
      });
}

// wva_lag_path_wide_probe_launch with the averages. off_out[7]: where in dev
// the fp32 records, violated, steps, the averaged fp32 records and verdicts,
// the raw functionals [slot][n_ticks][5] and the averaged raw functionals lie.
extern "C" int wva_lag_path_avg_wide_probe_launch(const void *tasks, void *wide, const void *segs,
                                                  const void *tiles, const double *desc,
                                                  int n_tasks, int n_segs, int n_tiles,
                                                  int n_ticks, int n_slots, int max_steps,
                                                  int stride, int halo, double dt, void *stream,
                                                  void *dev, size_t dev_bytes, size_t *need,
                                                  size_t *off_out) {
  WvaLagPathWideIn in = {(const WvaLagPathTask *)tasks, (WvaLagPathWideTask *)wide,
                         (const WvaLagSeg *)segs, (const WvaLagTile *)tiles, desc, n_tasks,
                         n_segs, n_tiles, n_ticks, n_slots, stride, halo, max_steps, dt};
  size_t slab = 0, off[WVA_LPWA_N];
  int rc = wva_lag_path_wide_plan(in, 4, WVA_LAG_WIDE_SLAB_CAP, &slab);
  if (rc != 0) return rc;
  const size_t bytes = wva_lag_path_avg_wide_layout(in, slab, true, off);
  if (need) *need = bytes;
  if (dev == nullptr) return 0;
  if (dev_bytes < bytes || ((uintptr_t)dev & 255) != 0) return -2;
  if (off_out)
    for (int i = 0; i < 7; ++i) off_out[i] = off[WVA_LPWA_F + i];
  void *up = nullptr;
  if (hipHostMalloc(&up, off[WVA_LPWA_F], hipHostMallocDefault) != hipSuccess) return -41;
  wva_lag_path_wide_stage(in, off, (char *)up);
  rc = (int)hipMemcpyAsync(dev, up, off[WVA_LPWA_F], hipMemcpyHostToDevice, (hipStream_t)stream);
  if (rc == 0)
    rc = wva_lag_path_avg_wide_launch(in, off, (char *)dev, true, (hipStream_t)stream, nullptr);
  const int rs = (int)hipStreamSynchronize((hipStream_t)stream);
  (void)hipHostFree(up);
  return rc != 0 ? rc : rs;
}
