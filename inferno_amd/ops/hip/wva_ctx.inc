// wva_ctx.inc — host side of the native reconcile context, included at the end
// of wva_kernels.hip (one translation unit: the kernels are launched from
// here). The whole per-tick device pipeline behind ONE C call (host staging of
// the per-server state, one H2D copy, the fused tick kernel — or, for layouts
// it does not cover, regime-bucketed sweep launches overlapped via events on
// side streams and the winner kernel —, one D2H copy, sync):
// wva_ctx_tick(ctx, ...); wva_reconcile(ctx) runs an already
// staged tick; the planning passes share the context's arrays and buckets
// (token-mix planning brings a bucket list of its own, over tasks).
#include <vector>

#include "../native/wva_arena.h"  // 256-aligned arena layout (host only)

#define WVA_MAX_BUCKETS 5
#define WVA_PLAN_MAX_S 256  // scenarios per planning pass

struct WvaBucket {
  int nt;
  const int *cell_ids;  // nullptr = identity
  int n_blocks;
  int max_n;
  float *g_inv;      // non-null: global-memory geometry slab (huge-N spill)
  double *g_anchor;
  // blocks per launch: 0 = all n_blocks in one launch; else the bucket runs as
  // consecutive launches of at most this many blocks on its stream, which
  // reuse the first `slice` slabs (token-mix planning's huge tier)
  int slice;
};

// Created with `new WvaCtx()`: every member without an initialiser below
// starts as zero / nullptr.
struct WvaCtx {
  int n_cells;
  int n_srv;
  int analyzer_mode;
  float cv2 = 1.0f;
  // device SoA
  WvaCellsIn in;
  WvaCellsOut out;
  const int *seg_start;
  int *winner;
  const int *cell_acc;
  // dynamic block: WVA_DYN_ROWS x n_cells 4-byte words (six int32 rows, then
  // arrival_rate and cur_cost), one device allocation and its pinned source;
  // `in` points into the device one
  void *dev_dyn;
  void *pin_dyn;
  // winner records: WVA_REC_ROWS x n_srv words (six fp32 rows, then four
  // int32 rows), one device block and its pinned mirror
  void *gather;
  void *pin_out;
  // host-side staging (wva_ctx_tick): the static per-cell topology and the
  // batch_n row the current bucket layout was chosen for (one host
  // allocation, carved up)
  int *topo;  // nullptr until wva_ctx_set_topology
  const int *topo_cell_server, *topo_cell_acc, *topo_cfg, *topo_at_tokens, *topo_override;
  int *bucket_batch_n;
  int bucket_batch_valid;  // 0 until set_buckets recorded a batch_n row
  WvaBucket buckets[WVA_MAX_BUCKETS];
  int n_buckets;
  hipStream_t s0;                           // primary stream
  hipStream_t side[WVA_MAX_BUCKETS - 1];    // overlap streams for buckets 1..
  hipEvent_t e_up;                          // upload-complete
  hipEvent_t e_b[WVA_MAX_BUCKETS - 1];      // side-bucket completion
  // hipGraph capture of the whole per-tick pipeline (H2D copies, bucket
  // kernels on their streams, winner kernel, D2H): replayed as ONE launch
  // per reconcile. State: 0 = not captured, 1 = exec valid, -1 = capture
  // failed once -> stay on the eager path. Invalidated by set_buckets.
  hipGraphExec_t graph_exec;
  int graph_state;
  // sizing memo (one device allocation: n_cells records, then the hit and
  // miss counters). nullptr = memo off (INFERNO_SIZING_MEMO=0 or the
  // allocation failed). Stable for the life of the ctx, so a captured graph
  // stays valid.
  WvaMemoRec *memo;
  unsigned *memo_cnt;
  // fused tick (wva_tick_t): sweep and winner step of a tick in one launch.
  // fused_on: INFERNO_FUSED_TICK is not 0 and the allocations below succeeded
  // (read once at create). fused_path is decided by every wva_ctx_set_buckets:
  // 0 = the bucket launches + wva_winner (a bucket is neither 64 nor 256
  // threads wide, or spills to global memory), 1 = one launch of the task
  // table, 2 = two launches (the widest bucket's tasks [0, n_tasks_b) with
  // lds_b on side[0], the rest with lds_a on s0).
  int fused_on;
  int fused_path;
  int n_cus_dev;         // CUs of the device (hipGetDeviceProperties at create)
  int n_cus;             // CU count of the residency rule: n_cus_dev, or the
                         // test-only INFERNO_FUSED_TICK_CUS
  int *dev_cell_server;  // device [n_cells], uploaded by wva_ctx_set_topology
  // done[n_srv]: arrivals of the current tick per server, an allocation of its
  // own padded to a multiple of 16 bytes and zeroed from its start. Invariant:
  // after a completed tick every word is 0 (the last arriver of each server
  // resets it), so there is no per-tick memset; done_dirty asks for one before
  // the next tick, after a tick that returned non-zero.
  unsigned *done;
  size_t done_bytes;
  int done_dirty;
  int4 *tasks;           // device task table, tasks_cap entries
  int tasks_cap;
  int n_tasks, n_tasks_b;
  int narrow_stride;     // doubles between the LDS slices of a narrow block
  size_t lds_a, lds_b;
  // scenario planning (wva_ctx_plan): buffers allocated on first use, grown
  // to the largest scenario count / accelerator count seen, freed in destroy
  int plan_cap;      // scenarios the buffers hold (0 = not allocated)
  int plan_acc_cap;  // accelerators per totals row the buffers hold
  int plan_s;        // scenario count of the last successful plan (0 = none)
  void *plan_dev;    // one device allocation, carved up below
  void *plan_pin;    // one pinned host allocation, carved up below
  float *plan_scen;  // device [S][n_cells]
  WvaCellsOut plan_out;  // device, each [S][n_cells]
  float *plan_pf;    // device [S][6][n_srv]
  int *plan_pi;      // device [S][4][n_srv]
  unsigned long long *plan_tot;  // device [S][n_acc]
  float *plan_pin_scen;  // pinned mirrors of plan_scen / pf / pi / tot
  float *plan_pin_pf;
  int *plan_pin_pi;
  unsigned long long *plan_pin_tot;
  // SLO planning (wva_ctx_plan_slo): the per-cell target sets, allocated on
  // first use, grown to the largest count seen, freed in destroy
  int slo_cap;       // target sets the buffers hold (0 = not allocated)
  void *slo_dev;     // one device allocation, carved up below
  void *slo_pin;     // one pinned host allocation, carved up below
  float *slo_ttft;   // device [T][n_cells]
  float *slo_itl;    // device [T][n_cells]
  float *slo_pin_ttft;  // pinned mirrors
  float *slo_pin_itl;
  // token-mix planning (wva_ctx_plan_tokens): the per-cell token sets,
  // allocated on first use, grown to the largest count seen, freed in destroy
  int tok_cap;       // token sets the buffers hold (0 = not allocated)
  void *tok_dev;     // one device allocation, carved up below
  void *tok_pin;     // one pinned host allocation, carved up below
  int *tok_in;       // device [W][n_cells]
  int *tok_out;      // device [W][n_cells]
  int *tok_n;        // device [W][n_cells]: the batch size N under set w
  int *tok_pin_in;   // pinned mirrors
  int *tok_pin_out;
  int *tok_pin_n;
  // hold analysis (wva_ctx_hold): the per-cell held replicas of every
  // scenario, allocated on first use, grown to the largest scenario count
  // seen, freed in destroy
  int hold_cap;      // scenarios the buffers hold (0 = not allocated)
  void *hold_dev;    // device i32 [S][n_cells]: -1 not held, >= 0 held replicas
  void *hold_pin;    // its pinned source
  // forecast rollout (wva_ctx_rollout): the per-server current allocation the
  // chain starts from and ends with, three rows of n_srv words (cur_acc,
  // cur_rep, cur_cost). Allocated on first use, freed in destroy.
  int roll_group = 1;  // lanes per server in wva_rollout (wva_ctx_set_topology)
  void *roll_dev;      // device [3][n_srv]
  void *roll_pin;      // its pinned source and mirror
  // forecast ensembles (wva_ctx_ensemble_pass, wva_ctx_ensemble_bands): one
  // device and one pinned allocation, made on first use, grown to the largest
  // ensemble seen and freed in destroy. They are carved up per ensemble
  // (WvaEnsLayout) when its first pass arrives; ens_next counts the paths the
  // passes have delivered since.
  void *ens_dev;
  void *ens_pin;
  size_t ens_dev_cap, ens_pin_cap;  // bytes held (0 = not allocated)
  int ens_paths, ens_steps, ens_acc, ens_q;  // the ensemble under way (ens_paths 0 = none)
  int ens_next;
  // capacity-limited planning (wva_ctx_plan_limited): the static greedy
  // inputs (wva_ctx_set_greedy_static) and the per-scenario workspace, both
  // allocated on first use and freed in destroy
  void *lim_static;     // device: cell_type, cell_units [n_cells], srv_prio [n_srv]
  const int *lim_cell_type;
  const int *lim_cell_units;
  const int *lim_srv_prio;
  int lim_cap;          // scenarios the workspace holds (0 = not allocated)
  int lim_types_cap;    // accelerator types per capacity row it holds
  void *lim_dev;        // one device allocation, carved up below
  void *lim_pin;        // one pinned host allocation, carved up below
  // Dynamic LDS wva_plan_greedy may take for its hot state, in bytes; fleets
  // that need more keep it in the global workspace (same code, same result).
  // INFERNO_PLAN_GREEDY_LDS overrides it (0 = always global), read once at
  // create.
  size_t lim_lds_budget = 120 * 1024;
  double *lim_wsd;      // device [S][n_srv + n_cells] 8-byte words
  int *lim_wsi;         // device [S][15 * n_srv + 3 * n_cells]
  int *lim_capacity;    // device [S][n_types]
  int *lim_px;          // device [S][2][n_srv]
  int *lim_pin_capacity;  // pinned mirrors of lim_capacity / lim_px
  int *lim_pin_px;
};

// pointer-slot order for wva_ctx_create (engine/native_ctx.py builds the
// array from CTX_SLOT_NAMES and checks its length against WVA_CTX_SLOTS):
//  0 dev_dyn (8*n_cells words: in_tok, out_tok, batch_n, perf_max_batch,
//    cur_replicas, flags i32; arrival_rate, cur_cost f32)
//  1 min_replicas            2 alpha  3 beta  4 gamma  5 delta
//  6 t_itl  7 t_ttft  8 t_tps  9 acc_cost
//  10 feasible  11 zero_empty  12 num_replicas  13 batch  14 cost
//  15 value  16 itl  17 ttft  18 rho  19 max_rate
//  20 seg_start  21 winner  22 cell_acc
//  23 gather (10*n_srv words: cost, value, itl, ttft, rho, max_rate f32;
//     acc code, num_replicas, batch, winner cell i32)
//  24 pin_dyn (pinned source of 0)  25 pin_out (pinned mirror of 23)
#define WVA_CTX_SLOTS 26
#define WVA_REC_ROWS 10

// The constants both sides of the C ABI rely on, by name; -1 for an unknown
// name. ops/sweep.py load_library() checks its mirrors against these once.
extern "C" int wva_abi(const char *name) {
#define WVA_ABI(x) {#x, x}
  static const struct {
    const char *name;
    int value;
  } table[] = {WVA_ABI(WVA_MAX_N),      WVA_ABI(WVA_XL_MAX_N),  WVA_ABI(WVA_HUGE_MAX_N),
               WVA_ABI(WVA_PLAN_MAX_S), WVA_ABI(WVA_N_SMALL),   WVA_ABI(WVA_N_MED),
               WVA_ABI(WVA_TICK_STALE), WVA_ABI(WVA_DYN_ROWS),  WVA_ABI(WVA_REC_ROWS),
               WVA_ABI(WVA_CTX_SLOTS),  WVA_ABI(WVA_MAX_BUCKETS), WVA_ABI(WVA_TICK_WIDE_WAVES),
               WVA_ABI(WVA_TICK_MAX_WAVES)};
#undef WVA_ABI
  if (name == nullptr) return -1;
  for (const auto &e : table)
    if (strcmp(name, e.name) == 0) return e.value;
  return -1;
}

// Makes the device that owns dev_ptr current for its scope (allocations must
// land next to the kernels' inputs). Switches only when both device ids are
// known and differ; restores only if it switched.
struct WvaDeviceGuard {
  int prev = -1;
  bool switched = false;
  explicit WvaDeviceGuard(const void *dev_ptr) {
    int dev = -1;
    hipPointerAttribute_t attr;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (hipPointerGetAttributes(&attr, dev_ptr) == hipSuccess) dev = attr.device;
    switched = dev >= 0 && prev >= 0 && dev != prev && hipSetDevice(dev) == hipSuccess;
  }
  ~WvaDeviceGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
  WvaDeviceGuard(const WvaDeviceGuard &) = delete;
  WvaDeviceGuard &operator=(const WvaDeviceGuard &) = delete;
};

extern "C" void *wva_ctx_create(int n_cells, int n_srv, void **p) {
  WvaCtx *c = new WvaCtx();
  c->n_cells = n_cells;
  c->n_srv = n_srv;
  if (const char *lds_env = getenv("INFERNO_PLAN_GREEDY_LDS")) {
    char *end = nullptr;
    const long v = strtol(lds_env, &end, 10);
    if (end != lds_env && *end == '\0' && v >= 0 && v <= 120 * 1024)
      c->lim_lds_budget = (size_t)v;
  }
  char *dd = (char *)p[0];
  size_t cw = (size_t)n_cells * 4;  // one row of the dynamic block
  c->in.in_tok = (const int *)(dd + 0 * cw);
  c->in.out_tok = (const int *)(dd + 1 * cw);
  c->in.batch_n = (const int *)(dd + 2 * cw);
  c->in.perf_max_batch = (const int *)(dd + 3 * cw);
  c->in.cur_replicas = (const int *)(dd + 4 * cw);
  c->in.flags = (const int *)(dd + 5 * cw);
  c->in.arrival_rate = (const float *)(dd + 6 * cw);
  c->in.cur_cost = (const float *)(dd + 7 * cw);
  c->in.min_replicas = (const int *)p[1];
  c->in.alpha = (const float *)p[2];
  c->in.beta = (const float *)p[3];
  c->in.gamma = (const float *)p[4];
  c->in.delta = (const float *)p[5];
  c->in.t_itl = (const float *)p[6];
  c->in.t_ttft = (const float *)p[7];
  c->in.t_tps = (const float *)p[8];
  c->in.acc_cost = (const float *)p[9];
  c->out.feasible = (uint8_t *)p[10];
  c->out.zero_empty = (uint8_t *)p[11];
  c->out.num_replicas = (int *)p[12];
  c->out.batch = (int *)p[13];
  c->out.cost = (float *)p[14];
  c->out.value = (float *)p[15];
  c->out.itl = (float *)p[16];
  c->out.ttft = (float *)p[17];
  c->out.rho = (float *)p[18];
  c->out.max_rate = (float *)p[19];
  c->seg_start = (const int *)p[20];
  c->winner = (int *)p[21];
  c->cell_acc = (const int *)p[22];
  c->gather = p[23];
  c->dev_dyn = p[0];
  c->pin_dyn = p[24];
  c->pin_out = p[25];
  bool ok = hipStreamCreateWithFlags(&c->s0, hipStreamNonBlocking) == hipSuccess &&
            hipEventCreateWithFlags(&c->e_up, hipEventDisableTiming) == hipSuccess;
  for (int i = 0; ok && i < WVA_MAX_BUCKETS - 1; ++i)
    ok = hipStreamCreateWithFlags(&c->side[i], hipStreamNonBlocking) == hipSuccess &&
         hipEventCreateWithFlags(&c->e_b[i], hipEventDisableTiming) == hipSuccess;
  if (!ok) {
    delete c;
    return nullptr;
  }
  // sizing memo: INFERNO_SIZING_MEMO=0 is the kill switch (A/B measurement,
  // tests) — read per call, never cached. Any failure here leaves the memo
  // off; the context itself is still good.
  const char *memo_env = getenv("INFERNO_SIZING_MEMO");
  const bool memo_on = !(memo_env != nullptr && memo_env[0] == '0' && memo_env[1] == '\0');
  if (memo_on && n_cells > 0) {
    WvaDeviceGuard on_dev(c->dev_dyn);
    const size_t bytes = (size_t)n_cells * sizeof(WvaMemoRec) + 2 * sizeof(unsigned);
    void *m = nullptr;
    if (hipMalloc(&m, bytes) == hipSuccess && m != nullptr) {
      if (hipMemsetAsync(m, 0, bytes, c->s0) == hipSuccess) {
        c->memo = (WvaMemoRec *)m;
        c->memo_cnt = (unsigned *)((char *)m + (size_t)n_cells * sizeof(WvaMemoRec));
      } else {
        (void)hipFree(m);
      }
    }
    if (c->memo == nullptr) (void)hipGetLastError();  // clear the non-fatal error
  }
  // fused tick: INFERNO_FUSED_TICK=0 forces the bucket launches (A/B runs,
  // tests). A failure here leaves it off; the context itself is still good.
  // INFERNO_FUSED_TICK_CUS (tests only) replaces the device's CU count in the
  // residency rule (one or two launches), not in the decision to fuse.
  const char *fused_env = getenv("INFERNO_FUSED_TICK");
  const bool fused_req = !(fused_env != nullptr && fused_env[0] == '0' && fused_env[1] == '\0');
  if (fused_req && n_cells > 0 && n_srv > 0) {
    WvaDeviceGuard on_dev(c->dev_dyn);
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
      c->n_cus = c->n_cus_dev = prop.multiProcessorCount;
    if (const char *cus_env = getenv("INFERNO_FUSED_TICK_CUS")) {
      char *end = nullptr;
      const long v = strtol(cus_env, &end, 10);
      if (end != cus_env && *end == '\0' && v >= 1 && v <= (1 << 20)) c->n_cus = (int)v;
    }
    c->done_bytes = (((size_t)n_srv * sizeof(unsigned)) + 15) & ~(size_t)15;
    void *d = nullptr, *cs = nullptr;
    if (c->n_cus > 0 && hipMalloc(&d, c->done_bytes) == hipSuccess && d != nullptr &&
        hipMalloc(&cs, (size_t)n_cells * sizeof(int)) == hipSuccess && cs != nullptr &&
        hipMemsetAsync(d, 0, c->done_bytes, c->s0) == hipSuccess) {
      c->done = (unsigned *)d;
      c->dev_cell_server = (int *)cs;
      c->fused_on = 1;
    } else {
      if (d != nullptr) (void)hipFree(d);
      if (cs != nullptr) (void)hipFree(cs);
      (void)hipGetLastError();
    }
  }
  return c;
}

static int wva_tick_waves(size_t lds);  // below, with the residency rule

// Diagnostics of the fused tick, never on the hot path (synchronous copy).
// info[8]: fused_path (0 bucket launches, 1 one launch, 2 two launches), tasks
// in all, tasks of the second launch, dynamic LDS bytes of the first and of the
// second launch, CU count of the residency rule, launch bound (blocks per CU)
// of the wva_tick_t instantiation of the first and of the second launch (0 =
// no such launch). done_nonzero: how many done[]
// words are not 0 (-1 when the fused tick is off). Either pointer may be null.
extern "C" int wva_ctx_fused_state(void *ctx, int *info, int *done_nonzero) {
  WvaCtx *c = (WvaCtx *)ctx;
  if (c == nullptr) return -1;
  if (info != nullptr) {
    info[0] = c->fused_path;
    info[1] = c->n_tasks;
    info[2] = c->n_tasks_b;
    info[3] = (int)c->lds_a;
    info[4] = (int)c->lds_b;
    info[5] = c->n_cus;
    info[6] = c->fused_path != 0 ? wva_tick_waves(c->lds_a) : 0;
    info[7] = c->fused_path == 2 ? wva_tick_waves(c->lds_b) : 0;
  }
  if (done_nonzero != nullptr) {
    *done_nonzero = -1;
    if (c->done != nullptr) {
      unsigned *h = (unsigned *)malloc(c->done_bytes);
      if (h == nullptr) return -3;
      if (hipStreamSynchronize(c->s0) != hipSuccess ||
          hipMemcpy(h, c->done, c->done_bytes, hipMemcpyDeviceToHost) != hipSuccess) {
        free(h);
        return -2;
      }
      int nz = 0;
      for (size_t i = 0; i < c->done_bytes / sizeof(unsigned); ++i) nz += h[i] != 0u;
      free(h);
      *done_nonzero = nz;
    }
  }
  return 0;
}

// hit/miss counters of the sizing memo since the context was created
// (unsigned, wrapping). Synchronous small D2H — diagnostics only, never on
// the hot path. Returns 1 when the memo is off, <0 on a runtime error.
extern "C" int wva_ctx_memo_stats(void *ctx, unsigned *hits, unsigned *misses) {
  WvaCtx *c = (WvaCtx *)ctx;
  if (c == nullptr || c->memo == nullptr) return 1;
  unsigned h[2] = {0u, 0u};
  if (hipStreamSynchronize(c->s0) != hipSuccess) return -1;
  if (hipMemcpy(h, c->memo_cnt, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return -2;
  if (hits) *hits = h[0];
  if (misses) *misses = h[1];
  return 0;
}

// The static per-cell topology wva_ctx_tick stages from, five host int32
// arrays of n_cells each (copied): the cell's server, its accelerator index,
// the profile's maxBatchSize and atTokens, the server's batch override.
extern "C" int wva_ctx_set_topology(void *ctx, const int *cell_server, const int *cell_acc_idx,
                                    const int *perf_max_batch_cfg, const int *at_tokens,
                                    const int *override_n) {
  WvaCtx *c = (WvaCtx *)ctx;
  if (c == nullptr) return -1;
  const size_t n = (size_t)c->n_cells;
  if (n > 0 && (cell_server == nullptr || cell_acc_idx == nullptr ||
                perf_max_batch_cfg == nullptr || at_tokens == nullptr || override_n == nullptr))
    return -1;
  for (size_t k = 0; k < n; ++k)
    if (cell_server[k] < 0 || cell_server[k] >= c->n_srv) return -2;
  if (c->topo == nullptr) {
    c->topo = (int *)malloc((6 * n + 1) * sizeof(int));
    if (c->topo == nullptr) return -3;
  }
  const int *src[5] = {cell_server, cell_acc_idx, perf_max_batch_cfg, at_tokens, override_n};
  for (int r = 0; r < 5; ++r)
    if (n > 0) memcpy(c->topo + r * n, src[r], n * sizeof(int));
  c->topo_cell_server = c->topo + 0 * n;
  c->topo_cell_acc = c->topo + 1 * n;
  c->topo_cfg = c->topo + 2 * n;
  c->topo_at_tokens = c->topo + 3 * n;
  c->topo_override = c->topo + 4 * n;
  c->bucket_batch_n = c->topo + 5 * n;
  c->bucket_batch_valid = 0;
  // wva_rollout's lanes per server: the smallest power of two that holds the
  // longest segment, at most a wave (longer segments are strided)
  {
    std::vector<int> per_srv((size_t)c->n_srv, 0);
    int longest = 1;
    for (size_t k = 0; k < n; ++k) {
      const int len = ++per_srv[cell_server[k]];
      if (len > longest) longest = len;
    }
    int g = 1;
    while (g < longest && g < WVA_WAVE) g <<= 1;
    c->roll_group = g;
  }
  // the fused tick kernel finds a cell's server on the device. Synchronous
  // upload, off the hot path; the next set_buckets rebuilds the task table.
  c->fused_path = 0;
  if (c->fused_on) {
    if (hipStreamSynchronize(c->s0) != hipSuccess ||
        hipMemcpy(c->dev_cell_server, cell_server, n * sizeof(int), hipMemcpyHostToDevice) !=
            hipSuccess)
      return -4;
  }
  return 0;
}

// The launch bound (blocks per CU) of the wva_tick_t instantiation that a
// launch with `lds` bytes of dynamic LDS uses: the wide budget
// (WVA_TICK_WIDE_WAVES) where the LDS holds the CU to that many blocks anyway,
// otherwise the narrow one (WVA_TICK_MAX_WAVES). So the register bound never
// takes a block off a CU that its LDS would have let on.
static int wva_tick_waves(size_t lds) {
  const size_t per_cu = lds > 0 ? (size_t)(160 * 1024) / lds : WVA_TICK_MAX_WAVES;
  return per_cu <= (size_t)WVA_TICK_WIDE_WAVES ? WVA_TICK_WIDE_WAVES : WVA_TICK_MAX_WAVES;
}
static const void *wva_tick_func(size_t lds) {
  return wva_tick_waves(lds) == WVA_TICK_WIDE_WAVES
             ? reinterpret_cast<const void *>(&wva_tick_t<WVA_TICK_WIDE_WAVES>)
             : reinterpret_cast<const void *>(&wva_tick_t<WVA_TICK_MAX_WAVES>);
}

// Blocks of `lds` bytes of dynamic LDS that are resident at once: per CU what
// fits in its 160 KiB, at most what the launch bound of the instantiation
// chosen for that size asks for.
static long wva_tick_slots(const WvaCtx *c, size_t lds) {
  const size_t bound = (size_t)wva_tick_waves(lds);
  const size_t per_cu = lds > 0 ? (size_t)(160 * 1024) / lds : bound;
  return (long)c->n_cus * (long)(per_cu < bound ? per_cu : bound);
}

// Build and upload the fused tick's task table from the bucket lists just
// recorded, and decide fused_path. Any reason not to fuse leaves fused_path 0
// (the bucket launches) and returns 0; a runtime error returns non-zero.
//   order: wide tasks (256-thread buckets, one cell each) by descending bucket
//   max_n, then narrow quads (64-thread buckets, up to four cells each, per
//   bucket) by descending max_n: the stragglers are dispatched first.
// Off the hot path: the bucket cell lists are copied back synchronously.
static int wva_build_tasks(WvaCtx *c) {
  c->fused_path = 0;
  c->n_tasks = c->n_tasks_b = 0;
  c->lds_a = c->lds_b = 0;
  if (!c->fused_on) return 0;
  // every set_buckets starts the counters from zero (s0 is idle: ticks are
  // synchronous), whichever path the layout takes
  if (hipMemsetAsync(c->done, 0, c->done_bytes, c->s0) != hipSuccess) return -55;
  c->done_dirty = 0;
  if (c->topo == nullptr || c->n_buckets < 1) return 0;
  const int nb = c->n_buckets;
  int order[WVA_MAX_BUCKETS];
  size_t need[WVA_MAX_BUCKETS];
  for (int i = 0; i < nb; ++i) {
    const WvaBucket &b = c->buckets[i];
    // only (64 or 256 threads, geometry in LDS) buckets fuse; anything else
    // (an INFERNO_NT_* override, the huge tier) keeps the whole tick on the
    // bucket launches, which also report a bad bucket as they always did
    if ((b.nt != WVA_WAVE && b.nt != WVA_TICK_NT) || b.g_inv != nullptr ||
        b.g_anchor != nullptr || b.max_n < 1 || b.max_n > WVA_XL_MAX_N || b.n_blocks < 0)
      return 0;
    need[i] = wva_cell_lds_bytes(b.max_n, b.nt);
    order[i] = i;
  }
  // wide before narrow, then descending max_n (insertion sort, stable)
  auto before = [&](int x, int y) {
    const WvaBucket &bx = c->buckets[x], &by = c->buckets[y];
    if (bx.nt != by.nt) return bx.nt > by.nt;
    return bx.max_n > by.max_n;
  };
  for (int i = 1; i < nb; ++i)
    for (int k = i; k > 0 && before(order[k], order[k - 1]); --k) {
      const int t = order[k];
      order[k] = order[k - 1];
      order[k - 1] = t;
    }

  if (hipDeviceSynchronize() != hipSuccess) return -50;
  std::vector<int> seg((size_t)c->n_srv + 1);
  if (hipMemcpy(seg.data(), c->seg_start, seg.size() * sizeof(int), hipMemcpyDeviceToHost) !=
      hipSuccess)
    return -51;
  // the kernel takes a server's cell count from seg_start and a cell's server
  // from cell_server: they must describe the same segments
  for (int k = 0; k < c->n_cells; ++k) {
    const int s = c->topo_cell_server[k];
    if (k < seg[s] || k >= seg[s + 1]) return 0;
  }

  std::vector<int4> tasks;
  std::vector<int> ids;
  std::vector<unsigned char> seen((size_t)c->n_cells, 0);
  size_t narrow_need = 0, wide_top = 0, wide_rest = 0;
  int n_top = 0;  // tasks of the widest (first) wide bucket
  for (int q = 0; q < nb; ++q) {
    const WvaBucket &b = c->buckets[order[q]];
    if (b.n_blocks == 0) continue;
    ids.resize((size_t)b.n_blocks);
    if (b.cell_ids == nullptr) {
      for (int k = 0; k < b.n_blocks; ++k) ids[k] = k;
    } else if (hipMemcpy(ids.data(), b.cell_ids, ids.size() * sizeof(int),
                         hipMemcpyDeviceToHost) != hipSuccess) {
      return -52;
    }
    // every cell exactly once over all buckets, or a server's counter would
    // never (or too early) reach its segment length
    for (int k = 0; k < b.n_blocks; ++k) {
      if (ids[k] < 0 || ids[k] >= c->n_cells || seen[ids[k]]) return 0;
      seen[ids[k]] = 1;
    }
    if (b.nt == WVA_TICK_NT) {
      if (tasks.empty()) {
        wide_top = need[order[q]];
        n_top = b.n_blocks;
      } else if (need[order[q]] > wide_rest) {
        wide_rest = need[order[q]];
      }
      for (int k = 0; k < b.n_blocks; ++k) tasks.push_back(make_int4(ids[k], WVA_TASK_WIDE, 0, 0));
    } else {
      if (need[order[q]] > narrow_need) narrow_need = need[order[q]];
      for (int k = 0; k < b.n_blocks; k += 4) {
        int4 t = make_int4(ids[k], -1, -1, -1);
        if (k + 1 < b.n_blocks) t.y = ids[k + 1];
        if (k + 2 < b.n_blocks) t.z = ids[k + 2];
        if (k + 3 < b.n_blocks) t.w = ids[k + 3];
        tasks.push_back(t);
      }
    }
  }
  for (int k = 0; k < c->n_cells; ++k)
    if (!seen[k]) return 0;
  if (tasks.empty()) return 0;

  // LDS: a wide block takes its bucket's need, a narrow block four slices of
  // the narrow buckets' largest need rounded up to 16 bytes
  const size_t stride = (narrow_need + 15) & ~(size_t)15;
  const size_t rest = wide_rest > 4 * stride ? wide_rest : 4 * stride;
  const size_t all = wide_top > rest ? wide_top : rest;
  const int n_tasks = (int)tasks.size();
  // The fused launch pays where the tick is bound by launches and queues, not
  // by the chip: a grid of at most one round of blocks at the kernel's
  // narrow launch bound (WVA_TICK_MAX_WAVES per CU; a launch on the wide
  // budget holds fewer, and the split rule below counts those). A larger fleet
  // is throughput-bound, and there the bucket launches, with their one-wave
  // blocks, measured faster (config5, 32768 cells: 0.735 ms/step against 1.166).
  if ((long)n_tasks > (long)WVA_TICK_MAX_WAVES * c->n_cus_dev) return 0;
  int path = 1;
  size_t lds_a = all, lds_b = 0;
  // Residency rule. When the widest bucket (the XL tier) alone raises the
  // launch's LDS, its tasks can go to a second launch with their own LDS
  // size, and the rest keeps the smaller one (more blocks per CU). The
  // fork/join of that launch measured 24 us on the flagship, about one round
  // of narrow blocks, so it is taken only when the single launch would need
  // more than one extra round: n_tasks > 2 x the blocks resident at once.
  if (n_top > 0 && n_top < n_tasks && wide_top > rest &&
      (long)n_tasks > 2 * wva_tick_slots(c, all)) {
    path = 2;
    lds_a = rest;
    lds_b = wide_top;
  }
  if (all > (size_t)160 * 1024) return 0;
  // each launch opts in for its own size on the instantiation it will use
  if (wva_optin_lds(wva_tick_func(lds_a), lds_a) != 0 ||
      (path == 2 && wva_optin_lds(wva_tick_func(lds_b), lds_b) != 0)) {
    (void)hipGetLastError();
    return 0;
  }

  // servers without cells never see an arrival: their record is the constant
  // one wva_winner writes for them, stored here once
  for (int s = 0; s < c->n_srv; ++s) {
    if (seg[s + 1] != seg[s]) continue;
    const int none = -1, zero = 0;
    for (int r = 0; r < WVA_REC_ROWS; ++r) {
      const int *v = (r == 6 || r == 9) ? &none : &zero;  // acc code, winner cell
      if (hipMemcpy((int *)c->gather + (size_t)r * c->n_srv + s, v, sizeof(int),
                    hipMemcpyHostToDevice) != hipSuccess)
        return -53;
    }
    if (hipMemcpy(c->winner + s, &none, sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
      return -53;
  }

  if (n_tasks > c->tasks_cap) {
    WvaDeviceGuard on_dev(c->dev_dyn);
    if (c->tasks != nullptr) (void)hipFree(c->tasks);
    c->tasks = nullptr;
    c->tasks_cap = 0;
    void *t = nullptr;
    if (hipMalloc(&t, (size_t)n_tasks * sizeof(int4)) != hipSuccess || t == nullptr) {
      (void)hipGetLastError();
      return 0;
    }
    c->tasks = (int4 *)t;
    c->tasks_cap = n_tasks;
  }
  if (hipMemcpy(c->tasks, tasks.data(), (size_t)n_tasks * sizeof(int4), hipMemcpyHostToDevice) !=
      hipSuccess)
    return -54;
  c->n_tasks = n_tasks;
  c->n_tasks_b = path == 2 ? n_top : 0;
  c->narrow_stride = (int)(stride / sizeof(double));
  c->lds_a = lds_a;
  c->lds_b = lds_b;
  c->fused_path = path;
  return 0;
}

// batch_n (may be null): the host batch_n row [n_cells] the layout was chosen
// for. It is recorded; wva_ctx_tick reports a stale layout when a tick's
// batch_n differs from it (or when none was recorded).
extern "C" int wva_ctx_set_buckets(void *ctx, int n_buckets, const int *nts,
                                   const void **cell_ids, const int *n_blocks,
                                   const int *max_ns, int analyzer_mode, float cv2,
                                   const void **g_invs, const void **g_anchors,
                                   const int *batch_n) {
  WvaCtx *c = (WvaCtx *)ctx;
  if (n_buckets < 0 || n_buckets > WVA_MAX_BUCKETS) return -1;
  c->bucket_batch_valid = 0;
  if (batch_n != nullptr && c->topo != nullptr) {
    if (c->n_cells > 0) memcpy(c->bucket_batch_n, batch_n, (size_t)c->n_cells * sizeof(int));
    c->bucket_batch_valid = 1;
  }
  c->n_buckets = n_buckets;
  for (int i = 0; i < n_buckets; ++i) {
    c->buckets[i].nt = nts[i];
    c->buckets[i].cell_ids = (const int *)cell_ids[i];
    c->buckets[i].n_blocks = n_blocks[i];
    c->buckets[i].max_n = max_ns[i];
    c->buckets[i].g_inv = g_invs ? (float *)g_invs[i] : nullptr;
    c->buckets[i].g_anchor = g_anchors ? (double *)g_anchors[i] : nullptr;
    c->buckets[i].slice = 0;
  }
  c->analyzer_mode = analyzer_mode;
  c->cv2 = cv2;
  // bucket layout / analyzer change: drop the captured pipeline (unless
  // capture already proved unsupported, which is sticky)
  if (c->graph_state == 1) (void)hipGraphExecDestroy(c->graph_exec);
  if (c->graph_state != -1) c->graph_state = 0;
  // the fused tick's task table follows the layout (and zeroes done[])
  return wva_build_tasks(c);
}

// The bucket sweeps of one pass, after the uploads queued on s0: record the
// upload event, launch bucket 0 of `buckets` on s0 and the others on the side
// streams behind that event, then join them back onto s0. `out` receives the
// per-cell results; `plan` (may be null) selects the planning kernels, `slo`
// (may be null) the SLO-planning ones. With `tok` (token-mix planning) the
// buckets hold tasks, `in` is the view with the [W][n_cells] token rows, and
// the sizing memo stays out of it. `hold` (may be null) selects the hold
// kernels on the context's buckets, sizing memo included. Enqueues only —
// no synchronising call, since the reconcile pipeline runs under stream
// capture.
static int wva_run_buckets(WvaCtx *c, const WvaBucket *buckets, int n_buckets,
                           const WvaCellsIn &in, const WvaCellsOut &out, const WvaPlanArgs *plan,
                           const WvaSloArgs *slo = nullptr, const WvaTokArgs *tok = nullptr,
                           const WvaHoldArgs *hold = nullptr) {
  if (n_buckets < 0 || n_buckets > WVA_MAX_BUCKETS) return -1;
  WvaMemoRec *memo = tok != nullptr ? nullptr : c->memo;
  unsigned *memo_cnt = tok != nullptr ? nullptr : c->memo_cnt;
  if (hipEventRecord(c->e_up, c->s0) != hipSuccess) return -10;
  for (int i = 0; i < n_buckets; ++i) {
    hipStream_t s = (i == 0) ? c->s0 : c->side[i - 1];
    if (i > 0 && hipStreamWaitEvent(s, c->e_up, 0) != hipSuccess) return -11;
    const WvaBucket &b = buckets[i];
    // one launch, or consecutive slices on this stream (stream order keeps a
    // slice off the slabs until the one before it is done with them)
    const int step = (b.slice > 0 && b.slice < b.n_blocks) ? b.slice : b.n_blocks;
    if (step < b.n_blocks && b.cell_ids == nullptr) return -2;  // a slice needs its ids
    for (int at = 0; at < b.n_blocks; at += step) {
      const int n = b.n_blocks - at < step ? b.n_blocks - at : step;
      const int rc = wva_sweep_dispatch(n, b.max_n, b.nt, b.cell_ids ? b.cell_ids + at : nullptr,
                                        c->analyzer_mode, c->cv2, s, in, out, b.g_inv,
                                        b.g_anchor, memo, memo_cnt, plan, slo, tok, hold);
      if (rc != 0) return rc;
    }
    if (i > 0 && hipEventRecord(c->e_b[i - 1], s) != hipSuccess) return -12;
  }
  for (int i = 1; i < n_buckets; ++i)
    if (hipStreamWaitEvent(c->s0, c->e_b[i - 1], 0) != hipSuccess) return -14;
  return 0;
}

// n tasks of the fused tick's table from task0 on, `lds` bytes of dynamic LDS
static void wva_tick_launch(WvaCtx *c, int task0, int n, size_t lds, hipStream_t s) {
  if (n <= 0) return;
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(n), dim3(WVA_TICK_NT), lds, s, c->in, c->out, c->tasks, task0,
                       n, c->narrow_stride, c->analyzer_mode, c->cv2, c->memo, c->memo_cnt,
                       c->dev_cell_server, c->done, c->seg_start, c->cell_acc, c->n_srv, c->gather,
                       c->winner);
  };
  if (wva_tick_waves(lds) == WVA_TICK_WIDE_WAVES)
    launch(&wva_tick_t<WVA_TICK_WIDE_WAVES>);
  else
    launch(&wva_tick_t<WVA_TICK_MAX_WAVES>);
}

// enqueue the whole per-tick pipeline on the ctx's streams (used both for
// eager execution and for stream capture into a hipGraph): H2D, then either
// the fused tick's launch(es) or the bucket launches and wva_winner, then D2H
static int wva_enqueue_pipeline(WvaCtx *c) {
  hipError_t err;
  // 1. dynamic H2D (pinned -> device), the whole block in one copy
  err = hipMemcpyAsync(c->dev_dyn, c->pin_dyn, (size_t)WVA_DYN_ROWS * c->n_cells * 4,
                       hipMemcpyHostToDevice, c->s0);
  if (err != hipSuccess) return (int)err;

  if (c->fused_path != 0) {
    // 2+3. sweep and winner records in one launch of the task table (two when
    // the residency rule split off the widest bucket: those tasks go first, on
    // side[0] behind the upload, and are joined before the download)
    if (c->fused_path == 2) {
      if (hipEventRecord(c->e_up, c->s0) != hipSuccess) return -10;
      if (hipStreamWaitEvent(c->side[0], c->e_up, 0) != hipSuccess) return -11;
      wva_tick_launch(c, 0, c->n_tasks_b, c->lds_b, c->side[0]);
      if (hipEventRecord(c->e_b[0], c->side[0]) != hipSuccess) return -12;
    }
    wva_tick_launch(c, c->n_tasks_b, c->n_tasks - c->n_tasks_b, c->lds_a, c->s0);
    if (c->fused_path == 2 && hipStreamWaitEvent(c->s0, c->e_b[0], 0) != hipSuccess) return -14;
    err = hipGetLastError();
    if (err != hipSuccess) return (int)err;
  } else {
    // 2. bucket launches, overlapped on the side streams
    const int rc = wva_run_buckets(c, c->buckets, c->n_buckets, c->in, c->out, nullptr);
    if (rc != 0) return rc;

    // 3. winner selection + winner records on s0, one launch
    hipLaunchKernelGGL(wva_winner, dim3(c->n_srv), dim3(WVA_WAVE), 0, c->s0, c->out.value,
                       c->out.feasible, c->out.zero_empty, c->cell_acc, c->out.num_replicas,
                       c->out.batch, c->out.cost, c->out.itl, c->out.ttft, c->out.rho,
                       c->out.max_rate, c->seg_start, c->n_srv, c->gather, c->winner);
    err = hipGetLastError();
    if (err != hipSuccess) return (int)err;
  }

  // 4. D2H of the winner records, one copy
  err = hipMemcpyAsync(c->pin_out, c->gather, (size_t)WVA_REC_ROWS * c->n_srv * 4,
                       hipMemcpyDeviceToHost, c->s0);
  if (err != hipSuccess) return (int)err;
  return 0;
}

// One reconcile tick behind one call: stage the six per-server arrays
// ([n_srv] each; cur_acc -3 none, -1 empty, >= 0 accelerator index) into the
// pinned dynamic block, then
//   launch != 0: if the tick's batch_n equals the row the bucket layout was
//     set for, run the pipeline and synchronise (returns 0, or a negative /
//     HIP error code); otherwise launch nothing and return WVA_TICK_STALE.
//     The caller then reads batch_n from the pinned block, calls
//     wva_ctx_set_buckets and wva_reconcile, which runs the staged tick.
//   launch == 0: stage only (the planning passes); returns 0 or
//     WVA_TICK_STALE by the same comparison.
// zero_arrival (may be null) replaces arrival in the zero-load decision.
extern "C" int wva_reconcile(void *ctx);
extern "C" int wva_ctx_tick(void *ctx, const float *arrival, const int *in_tok, const int *out_tok,
                            const int *cur_acc, const int *cur_rep, const float *cur_cost,
                            const float *zero_arrival, int launch) {
  WvaCtx *c = (WvaCtx *)ctx;
  if (c == nullptr || c->topo == nullptr) return -41;
  int changed = 1;
  const int rc = wva_stage_dynamic(
      c->n_srv, c->n_cells, arrival, in_tok, out_tok, cur_acc, cur_rep, cur_cost, zero_arrival,
      c->topo_cell_server, c->topo_cell_acc, c->topo_cfg, c->topo_at_tokens, c->topo_override,
      c->pin_dyn, c->bucket_batch_valid ? c->bucket_batch_n : nullptr, &changed);
  if (rc != 0) return -42;
  if (changed) return WVA_TICK_STALE;
  return launch ? wva_reconcile(ctx) : 0;
}

static int wva_reconcile_run(WvaCtx *c);

extern "C" int wva_reconcile(void *ctx) {
  WvaCtx *c = (WvaCtx *)ctx;
  // a tick that failed may have left arrivals in done[]: zero it first. In
  // steady state the last arrivers keep it zero and nothing is queued here.
  if (c->fused_path != 0 && c->done_dirty) {
    if (hipMemsetAsync(c->done, 0, c->done_bytes, c->s0) != hipSuccess) return -56;
    c->done_dirty = 0;
  }
  const int rc = wva_reconcile_run(c);
  if (rc != 0) c->done_dirty = 1;
  return rc;
}

static int wva_reconcile_run(WvaCtx *c) {
  // replay the captured pipeline when available: every buffer pointer and
  // kernel argument is ctx-stable between ticks, so the graph stays valid
  // until the bucket layout changes (set_buckets invalidates)
  if (c->graph_state == 1) {
    if (hipGraphLaunch(c->graph_exec, c->s0) != hipSuccess) {
      (void)hipGraphExecDestroy(c->graph_exec);
      c->graph_state = -1;  // fall back to eager permanently
    } else {
      return (int)hipStreamSynchronize(c->s0);
    }
  }
  if (c->graph_state == 0) {
    // OPT-IN (INFERNO_HIPGRAPH=1): measured SLOWER than eager on MI355X for
    // this pipeline (0.55 vs 0.45 ms/step, same-box x3) — graph replay does
    // not preserve the 4-HW-queue bucket overlap the eager path gets. Kept
    // as an option for launch-bound configurations (many tiny buckets).
    static int enabled = -1;
    if (enabled < 0) enabled = getenv("INFERNO_HIPGRAPH") != nullptr ? 1 : 0;
    if (!enabled) c->graph_state = -1;
  }
  if (c->graph_state == 0) {
    // capture once: the side-stream forks/joins via events become graph
    // dependencies (capture mode relaxed — no other thread uses these
    // streams)
    hipGraph_t graph = nullptr;
    bool ok = hipStreamBeginCapture(c->s0, hipStreamCaptureModeRelaxed) == hipSuccess;
    int rc = ok ? wva_enqueue_pipeline(c) : -20;
    if (ok) {
      if (hipStreamEndCapture(c->s0, &graph) != hipSuccess) ok = false;
    }
    if (ok && rc == 0 && graph != nullptr &&
        hipGraphInstantiate(&c->graph_exec, graph, nullptr, nullptr, 0) == hipSuccess) {
      c->graph_state = 1;
      (void)hipGraphDestroy(graph);
      if (hipGraphLaunch(c->graph_exec, c->s0) == hipSuccess)
        return (int)hipStreamSynchronize(c->s0);
      (void)hipGraphExecDestroy(c->graph_exec);
      c->graph_state = -1;
    } else {
      if (graph != nullptr) (void)hipGraphDestroy(graph);
      c->graph_state = -1;  // capture unsupported here: stay eager
      // a failed capture may have left the stream in capture state; make
      // sure it is usable again
      hipStreamCaptureStatus st;
      if (hipStreamIsCapturing(c->s0, &st) == hipSuccess &&
          st != hipStreamCaptureStatusNone) {
        hipGraph_t dead = nullptr;
        (void)hipStreamEndCapture(c->s0, &dead);
        if (dead != nullptr) (void)hipGraphDestroy(dead);
      }
    }
  }
  int rc = wva_enqueue_pipeline(c);
  if (rc != 0) return rc;
  return (int)hipStreamSynchronize(c->s0);
}

// ---------------------------------------------------------------------------
// Scenario planning: S arrival-rate scenarios of the whole fleet in one pass.
// Shares the context's static arrays, dynamic int arrays, buckets and sizing
// memo with wva_reconcile; owns only the scenario arrivals, the [S][n_cells]
// outputs and the reduce outputs. The hipGraph path is not involved.
// ---------------------------------------------------------------------------

static void wva_arena_free(void *&dev, void *&pin) {
  if (dev != nullptr) (void)hipFree(dev);
  if (pin != nullptr) (void)hipHostFree(pin);
  dev = pin = nullptr;
}

// One device block of dev_bytes (on the device that owns dev_dyn; zero-filled
// on s0 when `zero`) and one pinned host block of pin_bytes. On failure
// nothing is held and the pending HIP error is cleared, so the context stays
// usable for whatever does not need the arena.
static bool wva_arena_alloc(WvaCtx *c, size_t dev_bytes, size_t pin_bytes, bool zero, void **dev,
                            void **pin) {
  void *d = nullptr, *h = nullptr;
  bool ok;
  {
    WvaDeviceGuard on_dev(c->dev_dyn);
    ok = hipMalloc(&d, dev_bytes) == hipSuccess && d != nullptr;
    ok = ok && hipHostMalloc(&h, pin_bytes, hipHostMallocDefault) == hipSuccess && h != nullptr;
    ok = ok && (!zero || hipMemsetAsync(d, 0, dev_bytes, c->s0) == hipSuccess);
  }
  if (!ok) {
    wva_arena_free(d, h);
    (void)hipGetLastError();
    return false;
  }
  *dev = d;
  *pin = h;
  return true;
}

static void wva_plan_release(WvaCtx *c) {
  wva_arena_free(c->plan_dev, c->plan_pin);
  c->plan_cap = c->plan_acc_cap = c->plan_s = 0;
}

// (re)allocate the planning buffers for n_scen scenarios and n_acc
// accelerators; on failure nothing is held and the context is otherwise intact
static int wva_plan_reserve(WvaCtx *c, int n_scen, int n_acc) {
  if (n_scen <= c->plan_cap && n_acc <= c->plan_acc_cap) return 0;
  const int cap = n_scen > c->plan_cap ? n_scen : c->plan_cap;
  const int acap = n_acc > c->plan_acc_cap ? n_acc : c->plan_acc_cap;
  wva_plan_release(c);
  const size_t cells = (size_t)cap * (size_t)c->n_cells;
  const size_t b_w = cells * 4;  // one 4-byte per-cell array
  const size_t b_pf = (size_t)cap * 6 * c->n_srv * sizeof(float);
  const size_t b_pi = (size_t)cap * 4 * c->n_srv * sizeof(int);
  const size_t b_tot = (size_t)cap * acap * sizeof(unsigned long long);
  // device: scenario arrivals, the eight 4-byte and two 1-byte per-cell
  // outputs, pf, pi, totals; pinned: arrivals, pf, pi, totals
  enum { D_SCEN, D_REPS, D_BATCH, D_COST, D_VALUE, D_ITL, D_TTFT, D_RHO, D_RATE, D_FEAS, D_ZERO,
         D_PF, D_PI, D_TOT, D_N };
  enum { H_SCEN, H_PF, H_PI, H_TOT, H_N };
  const size_t d_size[D_N] = {b_w, b_w, b_w, b_w, b_w, b_w, b_w, b_w, b_w, cells, cells,
                              b_pf, b_pi, b_tot};
  const size_t h_size[H_N] = {b_w, b_pf, b_pi, b_tot};
  size_t d_off[D_N], h_off[H_N];
  const size_t dev_bytes = wva_arena_layout(d_size, D_N, d_off);
  const size_t pin_bytes = wva_arena_layout(h_size, H_N, h_off);
  // infeasible cells write only their two flags; start from zeros so the
  // other fields of such cells are defined
  if (!wva_arena_alloc(c, dev_bytes, pin_bytes, true, &c->plan_dev, &c->plan_pin)) return -30;
  c->plan_cap = cap;
  c->plan_acc_cap = acap;
  char *d = (char *)c->plan_dev, *h = (char *)c->plan_pin;
  c->plan_scen = (float *)(d + d_off[D_SCEN]);
  c->plan_out.num_replicas = (int *)(d + d_off[D_REPS]);
  c->plan_out.batch = (int *)(d + d_off[D_BATCH]);
  c->plan_out.cost = (float *)(d + d_off[D_COST]);
  c->plan_out.value = (float *)(d + d_off[D_VALUE]);
  c->plan_out.itl = (float *)(d + d_off[D_ITL]);
  c->plan_out.ttft = (float *)(d + d_off[D_TTFT]);
  c->plan_out.rho = (float *)(d + d_off[D_RHO]);
  c->plan_out.max_rate = (float *)(d + d_off[D_RATE]);
  c->plan_out.feasible = (uint8_t *)(d + d_off[D_FEAS]);
  c->plan_out.zero_empty = (uint8_t *)(d + d_off[D_ZERO]);
  c->plan_pf = (float *)(d + d_off[D_PF]);
  c->plan_pi = (int *)(d + d_off[D_PI]);
  c->plan_tot = (unsigned long long *)(d + d_off[D_TOT]);
  c->plan_pin_scen = (float *)(h + h_off[H_SCEN]);
  c->plan_pin_pf = (float *)(h + h_off[H_PF]);
  c->plan_pin_pi = (int *)(h + h_off[H_PI]);
  c->plan_pin_tot = (unsigned long long *)(h + h_off[H_TOT]);
  return 0;
}

static void wva_slo_release(WvaCtx *c) {
  wva_arena_free(c->slo_dev, c->slo_pin);
  c->slo_cap = 0;
}

// (re)allocate the SLO-planning target arrays for n_tgt target sets; on
// failure nothing is held and reconciles and load plans keep working
static int wva_slo_reserve(WvaCtx *c, int n_tgt) {
  if (n_tgt <= c->slo_cap) return 0;
  wva_slo_release(c);
  const size_t b_t = (size_t)n_tgt * (size_t)c->n_cells * sizeof(float);
  enum { A_TTFT, A_ITL, A_N };  // the same two arrays on the device and pinned
  const size_t size[A_N] = {b_t, b_t};
  size_t off[A_N];
  const size_t bytes = wva_arena_layout(size, A_N, off);
  if (!wva_arena_alloc(c, bytes, bytes, false, &c->slo_dev, &c->slo_pin)) return -36;
  c->slo_cap = n_tgt;
  char *d = (char *)c->slo_dev, *h = (char *)c->slo_pin;
  c->slo_ttft = (float *)(d + off[A_TTFT]);
  c->slo_itl = (float *)(d + off[A_ITL]);
  c->slo_pin_ttft = (float *)(h + off[A_TTFT]);
  c->slo_pin_itl = (float *)(h + off[A_ITL]);
  return 0;
}

static void wva_tok_release(WvaCtx *c) {
  wva_arena_free(c->tok_dev, c->tok_pin);
  c->tok_cap = 0;
}

// (re)allocate the token-mix planning arrays for n_tok token sets; on failure
// nothing is held and reconciles and the other plans keep working
static int wva_tok_reserve(WvaCtx *c, int n_tok) {
  if (n_tok <= c->tok_cap) return 0;
  wva_tok_release(c);
  const size_t b_t = (size_t)n_tok * (size_t)c->n_cells * sizeof(int);
  enum { A_IN, A_OUT, A_N, A_COUNT };  // the same three arrays on the device and pinned
  const size_t size[A_COUNT] = {b_t, b_t, b_t};
  size_t off[A_COUNT];
  const size_t bytes = wva_arena_layout(size, A_COUNT, off);
  if (!wva_arena_alloc(c, bytes, bytes, false, &c->tok_dev, &c->tok_pin)) return -38;
  c->tok_cap = n_tok;
  char *d = (char *)c->tok_dev, *h = (char *)c->tok_pin;
  c->tok_in = (int *)(d + off[A_IN]);
  c->tok_out = (int *)(d + off[A_OUT]);
  c->tok_n = (int *)(d + off[A_N]);
  c->tok_pin_in = (int *)(h + off[A_IN]);
  c->tok_pin_out = (int *)(h + off[A_OUT]);
  c->tok_pin_n = (int *)(h + off[A_N]);
  return 0;
}

static void wva_hold_release(WvaCtx *c) {
  wva_arena_free(c->hold_dev, c->hold_pin);
  c->hold_cap = 0;
}

// (re)allocate the hold analysis' held-replica array for n_scen scenarios; on
// failure nothing is held and reconciles and the other plans keep working
static int wva_hold_reserve(WvaCtx *c, int n_scen) {
  if (n_scen <= c->hold_cap) return 0;
  wva_hold_release(c);
  const size_t bytes = (size_t)n_scen * (size_t)c->n_cells * sizeof(int);
  if (!wva_arena_alloc(c, bytes, bytes, false, &c->hold_dev, &c->hold_pin)) return -39;
  c->hold_cap = n_scen;
  return 0;
}

// the rollout's current-allocation rows; on failure nothing is held and
// reconciles and plans keep working
static int wva_roll_reserve(WvaCtx *c) {
  if (c->roll_dev != nullptr) return 0;
  const size_t bytes = (size_t)3 * (size_t)c->n_srv * sizeof(int);
  if (!wva_arena_alloc(c, bytes, bytes, false, &c->roll_dev, &c->roll_pin)) return -37;
  return 0;
}

static void wva_lim_release(WvaCtx *c) {
  wva_arena_free(c->lim_dev, c->lim_pin);
  c->lim_cap = c->lim_types_cap = 0;
}

// (re)allocate the greedy workspace for n_scen scenarios and n_types
// accelerator types; on failure nothing is held and reconciles and unlimited
// plans keep working
static int wva_lim_reserve(WvaCtx *c, int n_scen, int n_types) {
  if (n_scen <= c->lim_cap && n_types <= c->lim_types_cap) return 0;
  const int cap = n_scen > c->lim_cap ? n_scen : c->lim_cap;
  const int tcap = n_types > c->lim_types_cap ? n_types : c->lim_types_cap;
  wva_lim_release(c);
  const size_t b_cap = (size_t)cap * tcap * sizeof(int);
  const size_t b_px = (size_t)cap * 2 * c->n_srv * sizeof(int);
  // device: wsd, wsi, capacity, px; pinned: capacity, px
  enum { D_WSD, D_WSI, D_CAP, D_PX, D_N };
  enum { H_CAP, H_PX, H_N };
  const size_t d_size[D_N] = {
      (size_t)cap * ((size_t)c->n_srv + (size_t)c->n_cells) * sizeof(double),
      (size_t)cap * ((size_t)15 * c->n_srv + (size_t)3 * c->n_cells) * sizeof(int), b_cap, b_px};
  const size_t h_size[H_N] = {b_cap, b_px};
  size_t d_off[D_N], h_off[H_N];
  const size_t dev_bytes = wva_arena_layout(d_size, D_N, d_off);
  const size_t pin_bytes = wva_arena_layout(h_size, H_N, h_off);
  if (!wva_arena_alloc(c, dev_bytes, pin_bytes, false, &c->lim_dev, &c->lim_pin)) return -34;
  c->lim_cap = cap;
  c->lim_types_cap = tcap;
  char *d = (char *)c->lim_dev, *h = (char *)c->lim_pin;
  c->lim_wsd = (double *)(d + d_off[D_WSD]);
  c->lim_wsi = (int *)(d + d_off[D_WSI]);
  c->lim_capacity = (int *)(d + d_off[D_CAP]);
  c->lim_px = (int *)(d + d_off[D_PX]);
  c->lim_pin_capacity = (int *)(h + h_off[H_CAP]);
  c->lim_pin_px = (int *)(h + h_off[H_PX]);
  return 0;
}

// Static inputs of wva_plan_greedy: host cell_type, cell_units [n_cells] and
// srv_prio [n_srv]. Synchronous upload; the caller repeats it only when one
// of the arrays changed.
extern "C" int wva_ctx_set_greedy_static(void *ctx, const int *cell_type, const int *cell_units,
                                         const int *srv_prio) {
  WvaCtx *c = (WvaCtx *)ctx;
  if (c == nullptr || cell_type == nullptr || cell_units == nullptr || srv_prio == nullptr)
    return -31;
  if (c->n_cells <= 0 || c->n_srv <= 0) return -33;
  const size_t b_c = wva_align256((size_t)c->n_cells * sizeof(int));
  const size_t b_s = wva_align256((size_t)c->n_srv * sizeof(int));
  if (c->lim_static == nullptr) {
    void *d = nullptr;
    bool ok;
    {
      WvaDeviceGuard on_dev(c->dev_dyn);
      ok = hipMalloc(&d, 2 * b_c + b_s) == hipSuccess && d != nullptr;
    }
    if (!ok) {
      (void)hipGetLastError();
      return -34;
    }
    c->lim_static = d;
    c->lim_cell_type = (const int *)d;
    c->lim_cell_units = (const int *)((char *)d + b_c);
    c->lim_srv_prio = (const int *)((char *)d + 2 * b_c);
  }
  if (hipStreamSynchronize(c->s0) != hipSuccess) return -1;
  char *d = (char *)c->lim_static;
  if (hipMemcpy(d, cell_type, (size_t)c->n_cells * sizeof(int), hipMemcpyHostToDevice) !=
          hipSuccess ||
      hipMemcpy(d + b_c, cell_units, (size_t)c->n_cells * sizeof(int), hipMemcpyHostToDevice) !=
          hipSuccess ||
      hipMemcpy(d + 2 * b_c, srv_prio, (size_t)c->n_srv * sizeof(int), hipMemcpyHostToDevice) !=
          hipSuccess)
    return -2;
  return 0;
}

// One planning pass. scen_arrival: host, [n_scen][n_cells] fp32 (req/min).
// The caller has filled the context's pinned dynamic arrays and set the
// buckets, exactly as for wva_reconcile. On success the three out pointers
// name the context's pinned result buffers, valid until the next
// wva_ctx_plan or wva_ctx_destroy: pf [n_scen][6][n_srv] fp32 (cost, value,
// itl, ttft, rho, max_rate), pi [n_scen][4][n_srv] i32 (acc code, replicas,
// batch, winner cell), totals [n_scen][n_acc] u64.
//
// With roll (wva_ctx_rollout) the scenarios are consecutive ticks and step 3
// is wva_rollout; everything else is the same pass.
//
// lim == nullptr is the unlimited plan (wva_ctx_plan). With lim, step 3 is
// wva_plan_greedy instead of wva_plan_reduce and the capacity rows go up and
// come back (wva_ctx_plan_limited); everything else is the same pass.
//
// With slo (wva_ctx_plan_slo) the n_scen slices are n_tgt target sets times
// n_scen / n_tgt arrival-rate scenarios, target-major: scen_arrival holds the
// arrival-rate scenarios only, the target sets go up next to it, and step 2
// launches the SLO-planning kernels; everything else is the same pass.
//
// With tok (wva_ctx_plan_tokens) the n_scen slices are n_tok token sets times
// n_scen / n_tok arrival-rate scenarios, set-major: the token sets go up next
// to the arrivals and step 2 launches the token-mix kernels over the pass's
// own bucket list of tasks; the context's buckets are not read or changed.
//
// With hold (wva_ctx_hold) the held replicas go up next to the arrivals, step
// 2 launches the hold kernels, step 3 is wva_hold_reduce, and the totals block
// holds the status counts and the deficits; everything else is the same pass.
//
// With ens (wva_ctx_ensemble_pass, which also brings roll for the start
// allocation) the slices are whole paths of consecutive ticks, step 3 is
// wva_rollout_paths, whose results stay in the ensemble arena, and step 4
// downloads the pf / pi records only when asked and nothing else.
struct WvaLimArgs {
  int n_types;
  const int *capacity;  // host [n_scen][n_types]
  int delayed;
  int policy;
};
struct WvaSloTargets {
  int n_tgt;
  const float *scen_ttft;  // host [n_tgt][n_cells]
  const float *scen_itl;   // host [n_tgt][n_cells]
};
struct WvaRollArgs {
  const int *cur_acc;     // host [n_srv]: -3 none, -1 empty, >= 0 accelerator index
  const int *cur_rep;     // host [n_srv]
  const float *cur_cost;  // host [n_srv]
};
struct WvaTokSets {
  int n_tok;
  const int *in_tok;   // host [n_tok][n_cells]
  const int *out_tok;  // host [n_tok][n_cells]
  const int *batch_n;  // host [n_tok][n_cells]
  const WvaBucket *buckets;  // the pass's task buckets
  int n_buckets;
};
struct WvaHoldIn {
  const int *scen_held;  // host [n_scen][n_cells]: -1 not held, >= 0 held replicas
};
// The carving of the ensemble arena for one ensemble. Device: the compact
// records, then what the pinned block mirrors at the same distances from its
// start: the per-row aggregates (TOT..RCOST, one download), the final
// allocations, the band outputs (SRQ..FLEET, one download).
struct WvaEnsLayout {
  enum { D_CODE, D_REPS, D_COST, D_TOT, D_NOWIN, D_CHG, D_RCOST, D_FIN, D_SRQ, D_SCQ, D_MODE,
         D_MODEP, D_FLEET, D_N };
  size_t off[D_N];
  size_t dev_bytes, pin_bytes;
  size_t pin(int seg) const { return off[seg] - off[D_TOT]; }  // offset in the pinned block
};
struct WvaEnsArgs {
  int n_paths;  // paths of this pass; the pass's slices are n_paths x n_steps
  int n_steps;
  int path0;    // the pass's first path in the ensemble
  int full;     // write and download the pf / pi records too
  const WvaEnsLayout *lay;
};

static int wva_plan_run(WvaCtx *c, int n_scen, int n_acc, const float *scen_arrival,
                        const WvaLimArgs *lim, const void **out_pf, const void **out_pi,
                        const void **out_totals, const WvaSloTargets *slo = nullptr,
                        const WvaRollArgs *roll = nullptr, const WvaTokSets *tok = nullptr,
                        const WvaHoldIn *hold = nullptr, const WvaEnsArgs *ens = nullptr) {
  if (c == nullptr || scen_arrival == nullptr) return -31;
  if (ens != nullptr && (roll == nullptr || ens->n_paths * ens->n_steps != n_scen)) return -32;
  if (n_scen < 1 || n_scen > WVA_PLAN_MAX_S || n_acc < 1) return -32;
  if (hold != nullptr && (lim != nullptr || slo != nullptr || roll != nullptr || tok != nullptr))
    return -32;
  // words per scenario of the totals block: the replica totals, or a hold's
  // status counts followed (after all scenarios' counts) by its deficits
  const int n_tot = hold != nullptr ? n_acc + WVA_HOLD_STATUSES : n_acc;
  if (slo != nullptr && (slo->n_tgt < 1 || n_scen % slo->n_tgt != 0)) return -32;
  if (tok != nullptr && (slo != nullptr || tok->n_tok < 1 || n_scen % tok->n_tok != 0))
    return -32;
  if (c->n_cells <= 0 || c->n_srv <= 0) return -33;
  c->plan_s = 0;
  int rc = wva_plan_reserve(c, n_scen, n_tot);
  if (rc != 0) return rc;
  if (hold != nullptr) {
    rc = wva_hold_reserve(c, n_scen);
    if (rc != 0) return rc;
  }
  if (slo != nullptr) {
    rc = wva_slo_reserve(c, slo->n_tgt);
    if (rc != 0) return rc;
  }
  if (tok != nullptr) {
    rc = wva_tok_reserve(c, tok->n_tok);
    if (rc != 0) return rc;
  }
  if (lim != nullptr) {
    rc = wva_lim_reserve(c, n_scen, lim->n_types);
    if (rc != 0) return rc;
  }
  if (roll != nullptr) {
    rc = wva_roll_reserve(c);
    if (rc != 0) return rc;
  }
  // arrival-rate scenarios: all n_scen slices, or the load axis of an SLO or
  // token-mix plan
  const int n_load = slo != nullptr   ? n_scen / slo->n_tgt
                     : tok != nullptr ? n_scen / tok->n_tok
                                      : n_scen;
  const size_t cells = (size_t)n_load * (size_t)c->n_cells;
  hipError_t err;

  // 1. uploads: scenario arrivals through the pinned staging buffer, then the
  // dynamic arrays as wva_enqueue_pipeline does
  for (size_t i = 0; i < cells; ++i) c->plan_pin_scen[i] = scen_arrival[i];
  err = hipMemcpyAsync(c->plan_scen, c->plan_pin_scen, cells * sizeof(float),
                       hipMemcpyHostToDevice, c->s0);
  if (err != hipSuccess) return (int)err;
  if (hold != nullptr) {
    memcpy(c->hold_pin, hold->scen_held, cells * sizeof(int));
    err = hipMemcpyAsync(c->hold_dev, c->hold_pin, cells * sizeof(int), hipMemcpyHostToDevice,
                         c->s0);
    if (err != hipSuccess) return (int)err;
  }
  if (slo != nullptr) {
    const size_t tcells = (size_t)slo->n_tgt * (size_t)c->n_cells;
    for (size_t i = 0; i < tcells; ++i) {
      c->slo_pin_ttft[i] = slo->scen_ttft[i];
      c->slo_pin_itl[i] = slo->scen_itl[i];
    }
    err = hipMemcpyAsync(c->slo_ttft, c->slo_pin_ttft, tcells * sizeof(float),
                         hipMemcpyHostToDevice, c->s0);
    if (err != hipSuccess) return (int)err;
    err = hipMemcpyAsync(c->slo_itl, c->slo_pin_itl, tcells * sizeof(float),
                         hipMemcpyHostToDevice, c->s0);
    if (err != hipSuccess) return (int)err;
  }
  if (tok != nullptr) {
    // (one copy per array: the arena pads each to its alignment)
    const size_t tcells = (size_t)tok->n_tok * (size_t)c->n_cells;
    memcpy(c->tok_pin_in, tok->in_tok, tcells * sizeof(int));
    memcpy(c->tok_pin_out, tok->out_tok, tcells * sizeof(int));
    memcpy(c->tok_pin_n, tok->batch_n, tcells * sizeof(int));
    int *const dst[3] = {c->tok_in, c->tok_out, c->tok_n};
    const int *const src[3] = {c->tok_pin_in, c->tok_pin_out, c->tok_pin_n};
    for (int r = 0; r < 3; ++r) {
      err = hipMemcpyAsync(dst[r], src[r], tcells * sizeof(int), hipMemcpyHostToDevice, c->s0);
      if (err != hipSuccess) return (int)err;
    }
  }
  err = hipMemcpyAsync(c->dev_dyn, c->pin_dyn, (size_t)WVA_DYN_ROWS * c->n_cells * 4,
                       hipMemcpyHostToDevice, c->s0);
  if (err != hipSuccess) return (int)err;
  err = hipMemsetAsync(c->plan_tot, 0, (size_t)n_scen * n_tot * sizeof(unsigned long long),
                       c->s0);
  if (err != hipSuccess) return (int)err;
  const size_t b_cur = (size_t)3 * (size_t)c->n_srv * sizeof(int);
  if (roll != nullptr) {
    int *pc = (int *)c->roll_pin;
    for (int i = 0; i < c->n_srv; ++i) {
      pc[i] = roll->cur_acc[i];
      pc[c->n_srv + i] = roll->cur_rep[i];
      memcpy(pc + 2 * (size_t)c->n_srv + i, roll->cur_cost + i, sizeof(float));
    }
    err = hipMemcpyAsync(c->roll_dev, c->roll_pin, b_cur, hipMemcpyHostToDevice, c->s0);
    if (err != hipSuccess) return (int)err;
  }
  const size_t n_capacity = lim != nullptr ? (size_t)n_scen * (size_t)lim->n_types : 0;
  if (lim != nullptr) {
    for (size_t i = 0; i < n_capacity; ++i) c->lim_pin_capacity[i] = lim->capacity[i];
    err = hipMemcpyAsync(c->lim_capacity, c->lim_pin_capacity, n_capacity * sizeof(int),
                         hipMemcpyHostToDevice, c->s0);
    if (err != hipSuccess) return (int)err;
  }

  // 2. planning buckets: same streams, fork/join and order as the reconcile
  if (hold != nullptr) {
    const WvaHoldArgs ha = {c->n_cells, n_scen, c->plan_scen, (const int *)c->hold_dev};
    rc = wva_run_buckets(c, c->buckets, c->n_buckets, c->in, c->plan_out, nullptr, nullptr,
                         nullptr, &ha);
  } else if (tok != nullptr) {
    // the pass's own task buckets on a view of the inputs whose token rows
    // are the [W][n_cells] arrays; the context's layout is left alone
    WvaCellsIn tin = c->in;
    tin.in_tok = c->tok_in;
    tin.out_tok = c->tok_out;
    tin.batch_n = c->tok_n;
    const WvaTokArgs ta = {c->n_cells, n_load, c->plan_scen, tok->n_tok};
    rc = wva_run_buckets(c, tok->buckets, tok->n_buckets, tin, c->plan_out, nullptr, nullptr,
                         &ta);
  } else if (slo != nullptr) {
    const WvaSloArgs sa = {c->n_cells, n_load,       c->plan_scen,
                           slo->n_tgt, c->slo_ttft, c->slo_itl};
    rc = wva_run_buckets(c, c->buckets, c->n_buckets, c->in, c->plan_out, nullptr, &sa);
  } else {
    const WvaPlanArgs pa = {c->n_cells, n_scen, c->plan_scen};
    rc = wva_run_buckets(c, c->buckets, c->n_buckets, c->in, c->plan_out, &pa);
  }
  if (rc != 0) return rc;

  // 3. winners, records and totals for all (server, scenario) pairs; a
  // rollout's scenarios are consecutive steps, chained per server
  if (hold != nullptr) {
    // the held cell's slice per (server, scenario); counts [n_scen][6], then
    // deficit [n_scen][n_acc], in the totals block
    const int per_block = WVA_WAVE / c->roll_group;
    hipLaunchKernelGGL(wva_hold_reduce, dim3((c->n_srv + per_block - 1) / per_block, n_scen),
                       dim3(WVA_WAVE), 0, c->s0, c->plan_out.feasible, c->plan_out.zero_empty,
                       c->cell_acc, c->plan_out.num_replicas, c->plan_out.batch, c->plan_out.cost,
                       c->plan_out.value, c->plan_out.itl, c->plan_out.ttft, c->plan_out.rho,
                       c->plan_out.max_rate, c->seg_start, c->n_srv, c->n_cells, n_scen, n_acc,
                       c->roll_group, c->plan_pf, c->plan_pi, c->plan_tot,
                       c->plan_tot + (size_t)n_scen * WVA_HOLD_STATUSES);
  } else if (ens != nullptr) {
    // the slices are ens->n_paths paths of consecutive ticks, every path
    // chained from the same start allocation
    const int per_block = WVA_WAVE / c->roll_group;
    char *d = (char *)c->ens_dev;
    const size_t *off = ens->lay->off;
    hipLaunchKernelGGL(
        wva_rollout_paths, dim3((c->n_srv + per_block - 1) / per_block, ens->n_paths),
        dim3(WVA_WAVE), 0, c->s0, c->plan_out.value, c->plan_out.feasible, c->plan_out.zero_empty,
        c->cell_acc, c->plan_out.num_replicas, c->plan_out.batch, c->plan_out.cost,
        c->plan_out.itl, c->plan_out.ttft, c->plan_out.rho, c->plan_out.max_rate, c->seg_start,
        c->n_srv, c->n_cells, ens->n_steps, ens->n_paths, n_acc, c->roll_group, ens->path0,
        ens->full, c->plan_pf, c->plan_pi, (const int *)c->roll_dev,
        (int *)(d + off[WvaEnsLayout::D_CODE]), (int *)(d + off[WvaEnsLayout::D_REPS]),
        (float *)(d + off[WvaEnsLayout::D_COST]),
        (unsigned long long *)(d + off[WvaEnsLayout::D_TOT]),
        (int *)(d + off[WvaEnsLayout::D_NOWIN]), (int *)(d + off[WvaEnsLayout::D_CHG]),
        (int *)(d + off[WvaEnsLayout::D_FIN]));
  } else if (roll != nullptr) {
    const int per_block = WVA_WAVE / c->roll_group;
    hipLaunchKernelGGL(wva_rollout, dim3((c->n_srv + per_block - 1) / per_block), dim3(WVA_WAVE),
                       0, c->s0, c->plan_out.value, c->plan_out.feasible, c->plan_out.zero_empty,
                       c->cell_acc, c->plan_out.num_replicas, c->plan_out.batch, c->plan_out.cost,
                       c->plan_out.itl, c->plan_out.ttft, c->plan_out.rho, c->plan_out.max_rate,
                       c->seg_start, c->n_srv, c->n_cells, n_scen, n_acc, c->roll_group,
                       c->plan_pf, c->plan_pi, c->plan_tot, (int *)c->roll_dev);
  } else if (lim == nullptr) {
    hipLaunchKernelGGL(wva_plan_reduce, dim3(c->n_srv, n_scen), dim3(WVA_WAVE), 0, c->s0,
                       c->plan_out.value, c->plan_out.feasible, c->plan_out.zero_empty,
                       c->cell_acc, c->plan_out.num_replicas, c->plan_out.batch, c->plan_out.cost,
                       c->plan_out.itl, c->plan_out.ttft, c->plan_out.rho, c->plan_out.max_rate,
                       c->seg_start, c->n_srv, c->n_cells, n_scen, n_acc, c->plan_pf, c->plan_pi,
                       c->plan_tot);
  } else {
    size_t lds = wva_greedy_lds_bytes(c->n_srv, c->n_cells);
    if (lds > c->lim_lds_budget ||
        wva_optin_lds(reinterpret_cast<const void *>(&wva_plan_greedy), lds) != 0) {
      (void)hipGetLastError();
      lds = 0;  // hot state in the global workspace
    }
    hipLaunchKernelGGL(wva_plan_greedy, dim3(n_scen), dim3(WVA_WAVE), lds, c->s0,
                       c->plan_out.value, c->plan_out.feasible, c->plan_out.zero_empty,
                       c->cell_acc, c->plan_out.num_replicas, c->plan_out.batch, c->plan_out.cost,
                       c->plan_out.itl, c->plan_out.ttft, c->plan_out.rho, c->plan_out.max_rate,
                       c->seg_start, c->lim_cell_type, c->lim_cell_units, c->lim_srv_prio,
                       c->n_srv, c->n_cells, n_scen, n_acc, lim->n_types, lim->delayed,
                       lim->policy, lds > 0 ? 1 : 0, c->lim_capacity, c->lim_wsi, c->lim_wsd, c->plan_pf,
                       c->plan_pi, c->lim_px, c->plan_tot);
  }
  err = hipGetLastError();
  if (err != hipSuccess) return (int)err;
  if (lim != nullptr) {
    err = hipMemcpyAsync(c->lim_pin_capacity, c->lim_capacity, n_capacity * sizeof(int),
                         hipMemcpyDeviceToHost, c->s0);
    if (err != hipSuccess) return (int)err;
    err = hipMemcpyAsync(c->lim_pin_px, c->lim_px, (size_t)n_scen * 2 * c->n_srv * sizeof(int),
                         hipMemcpyDeviceToHost, c->s0);
    if (err != hipSuccess) return (int)err;
  }

  // 4. downloads; an ensemble pass leaves its results in the ensemble arena
  // and downloads the records only when asked
  if (ens != nullptr) {
    if (ens->full) {
      err = hipMemcpyAsync(c->plan_pin_pf, c->plan_pf,
                           (size_t)n_scen * 6 * c->n_srv * sizeof(float), hipMemcpyDeviceToHost,
                           c->s0);
      if (err != hipSuccess) return (int)err;
      err = hipMemcpyAsync(c->plan_pin_pi, c->plan_pi, (size_t)n_scen * 4 * c->n_srv * sizeof(int),
                           hipMemcpyDeviceToHost, c->s0);
      if (err != hipSuccess) return (int)err;
    }
    err = hipStreamSynchronize(c->s0);
    if (err != hipSuccess) return (int)err;
    c->plan_s = n_scen;
    if (out_pf) *out_pf = c->plan_pin_pf;
    if (out_pi) *out_pi = c->plan_pin_pi;
    return 0;
  }
  if (roll != nullptr) {
    err = hipMemcpyAsync(c->roll_pin, c->roll_dev, b_cur, hipMemcpyDeviceToHost, c->s0);
    if (err != hipSuccess) return (int)err;
  }
  err = hipMemcpyAsync(c->plan_pin_pf, c->plan_pf, (size_t)n_scen * 6 * c->n_srv * sizeof(float),
                       hipMemcpyDeviceToHost, c->s0);
  if (err != hipSuccess) return (int)err;
  err = hipMemcpyAsync(c->plan_pin_pi, c->plan_pi, (size_t)n_scen * 4 * c->n_srv * sizeof(int),
                       hipMemcpyDeviceToHost, c->s0);
  if (err != hipSuccess) return (int)err;
  err = hipMemcpyAsync(c->plan_pin_tot, c->plan_tot,
                       (size_t)n_scen * n_tot * sizeof(unsigned long long),
                       hipMemcpyDeviceToHost, c->s0);
  if (err != hipSuccess) return (int)err;
  err = hipStreamSynchronize(c->s0);
  if (err != hipSuccess) return (int)err;
  c->plan_s = n_scen;
  if (out_pf) *out_pf = c->plan_pin_pf;
  if (out_pi) *out_pi = c->plan_pin_pi;
  if (out_totals) *out_totals = c->plan_pin_tot;
  return 0;
}

extern "C" int wva_ctx_plan(void *ctx, int n_scen, int n_acc, const float *scen_arrival,
                            const void **out_pf, const void **out_pi,
                            const void **out_totals) {
  return wva_plan_run((WvaCtx *)ctx, n_scen, n_acc, scen_arrival, nullptr, out_pf, out_pi,
                      out_totals);
}

// One capacity-limited planning pass: wva_ctx_plan's uploads and buckets, then
// one greedy solve per scenario on the device. capacity: host, [n_scen]
// [n_types] int32 units per accelerator type. policy: 0 None,
// 1 PriorityExhaustive, 2 PriorityRoundRobin, 3 RoundRobin. The static inputs
// must have been set (wva_ctx_set_greedy_static). pf, pi and totals are as for
// wva_ctx_plan, holding the limited solution (pi row 0 is the granted
// accelerator or -1, row 1 the granted replicas). out_px: pinned i32 [n_scen]
// [2][n_srv] (the granted cell's pre-cut replicas; the server's feasible
// candidates that are not zero-load). out_capacity: pinned i32 [n_scen]
// [n_types], the capacity left.
extern "C" int wva_ctx_plan_limited(void *ctx, int n_scen, int n_acc, const float *scen_arrival,
                                    int n_types, const int *capacity, int delayed, int policy,
                                    const void **out_pf, const void **out_pi,
                                    const void **out_totals, const void **out_px,
                                    const void **out_capacity) {
  WvaCtx *c = (WvaCtx *)ctx;
  if (c == nullptr || capacity == nullptr) return -31;
  if (n_types < 1 || policy < 0 || policy > 3) return -32;
  if (c->lim_static == nullptr) return -35;
  const WvaLimArgs lim = {n_types, capacity, delayed ? 1 : 0, policy};
  const int rc = wva_plan_run(c, n_scen, n_acc, scen_arrival, &lim, out_pf, out_pi, out_totals);
  if (rc != 0) return rc;
  if (out_px) *out_px = c->lim_pin_px;
  if (out_capacity) *out_capacity = c->lim_pin_capacity;
  return 0;
}

// One SLO-planning pass: n_tgt target sets times n_load = n_scen / n_tgt
// arrival-rate scenarios, n_scen slices in all (1..WVA_PLAN_MAX_S), slice
// t * n_load + s being target set t at arrival rates s. scen_arrival: host
// [n_load][n_cells] fp32 (req/min); scen_ttft, scen_itl: host [n_tgt][n_cells]
// fp32 (msec, 0 = no target). Staging, buckets and the three out pointers
// ([n_scen] leading) are as for wva_ctx_plan; wva_ctx_plan_cells works on the
// result. -36: the target arrays could not be allocated (the context is intact).
extern "C" int wva_ctx_plan_slo(void *ctx, int n_tgt, int n_scen, int n_acc,
                                const float *scen_arrival, const float *scen_ttft,
                                const float *scen_itl, const void **out_pf, const void **out_pi,
                                const void **out_totals) {
  if (scen_ttft == nullptr || scen_itl == nullptr) return -31;
  const WvaSloTargets slo = {n_tgt, scen_ttft, scen_itl};
  return wva_plan_run((WvaCtx *)ctx, n_scen, n_acc, scen_arrival, nullptr, out_pf, out_pi,
                      out_totals, &slo);
}

// One forecast-rollout pass: the n_steps rows of scen_arrival ([n_steps]
// [n_cells] fp32, req/min) are consecutive ticks. wva_ctx_plan's staging,
// uploads and buckets, then wva_rollout instead of wva_plan_reduce: step 0 is
// judged against the per-server current allocation cur_acc / cur_rep / cur_cost
// (host [n_srv]; the caller staged the tick with the same three arrays), step
// s >= 1 against what step s - 1 left behind. pf, pi and totals are as for
// wva_ctx_plan; out_cur names a pinned i32 [3][n_srv] block (cur_acc, cur_rep,
// the bits of cur_cost) holding the allocation after the last step.
// wva_ctx_plan_cells works on the result and returns every step's value
// against that step's own current allocation. -37: the current-allocation
// rows could not be allocated (the context is intact).
extern "C" int wva_ctx_rollout(void *ctx, int n_steps, int n_acc, const float *scen_arrival,
                               const int *cur_acc, const int *cur_rep, const float *cur_cost,
                               const void **out_pf, const void **out_pi, const void **out_totals,
                               const void **out_cur) {
  WvaCtx *c = (WvaCtx *)ctx;
  if (c == nullptr || cur_acc == nullptr || cur_rep == nullptr || cur_cost == nullptr) return -31;
  const WvaRollArgs roll = {cur_acc, cur_rep, cur_cost};
  const int rc = wva_plan_run(c, n_steps, n_acc, scen_arrival, nullptr, out_pf, out_pi,
                              out_totals, nullptr, &roll);
  if (rc != 0) return rc;
  if (out_cur) *out_cur = c->roll_pin;
  return 0;
}

// One token-mix planning pass: n_tok sets of per-cell token averages times
// n_load = n_scen / n_tok arrival-rate scenarios, n_scen slices in all
// (1..WVA_PLAN_MAX_S), slice w * n_load + s being token set w at arrival rates
// s. scen_arrival: host [n_load][n_cells] fp32 (req/min); in_tok, out_tok,
// batch_n: host [n_tok][n_cells] int32, batch_n being the batch size N the
// single-scenario path stages for the cell under set w. The tick is staged as
// for wva_ctx_plan (its token rows are not read). The pass brings its own
// bucket list over the tasks w * n_cells + cell, chosen from batch_n: per
// bucket the block width, the device int32 task ids (null: every task, in
// order), the task count, the largest N, the slabs of a global-memory bucket
// and the tasks per launch (0: all; else the bucket runs in consecutive slices
// of that many tasks, which share slabs for that many blocks). Nothing of the
// context's reconcile layout is read or changed, and the sizing memo is left
// out. The three out pointers ([n_scen] leading) are as for wva_ctx_plan;
// wva_ctx_plan_cells works on the result. -38: the token arrays could not be
// allocated (the context is intact).
extern "C" int wva_ctx_plan_tokens(void *ctx, int n_tok, int n_scen, int n_acc,
                                   const float *scen_arrival, const int *in_tok,
                                   const int *out_tok, const int *batch_n, int n_buckets,
                                   const int *nts, const void **task_ids, const int *n_blocks,
                                   const int *max_ns, const void **g_invs,
                                   const void **g_anchors, const int *slices,
                                   const void **out_pf, const void **out_pi,
                                   const void **out_totals) {
  WvaCtx *c = (WvaCtx *)ctx;
  if (c == nullptr || in_tok == nullptr || out_tok == nullptr || batch_n == nullptr) return -31;
  if (n_buckets < 0 || n_buckets > WVA_MAX_BUCKETS) return -32;
  if (n_buckets > 0 && (nts == nullptr || task_ids == nullptr || n_blocks == nullptr ||
                        max_ns == nullptr))
    return -31;
  if (n_tok < 1 || n_tok > WVA_PLAN_MAX_S) return -32;
  const long n_tasks = (long)n_tok * (long)c->n_cells;
  if (n_tasks > 0x7fffffffL) return -32;
  WvaBucket buckets[WVA_MAX_BUCKETS];
  for (int i = 0; i < n_buckets; ++i) {
    WvaBucket &b = buckets[i];
    b.nt = nts[i];
    b.cell_ids = (const int *)task_ids[i];
    b.n_blocks = n_blocks[i];
    b.max_n = max_ns[i];
    b.g_inv = g_invs ? (float *)g_invs[i] : nullptr;
    b.g_anchor = g_anchors ? (double *)g_anchors[i] : nullptr;
    b.slice = slices ? slices[i] : 0;
    if (b.n_blocks < 0 || (long)b.n_blocks > n_tasks || b.slice < 0) return -32;
    // the identity list names every task; a partial bucket brings its ids
    if (b.cell_ids == nullptr && (long)b.n_blocks != n_tasks) return -32;
  }
  const WvaTokSets tok = {n_tok, in_tok, out_tok, batch_n, buckets, n_buckets};
  return wva_plan_run(c, n_scen, n_acc, scen_arrival, nullptr, out_pf, out_pi, out_totals,
                      nullptr, nullptr, &tok);
}

// One hold-analysis pass: the latency a fixed allocation gives under n_scen
// loads. wva_ctx_plan's staging, uploads, buckets, streams and output arena,
// with wva_hold_t instead of wva_plan_t and wva_hold_reduce instead of
// wva_plan_reduce. scen_arrival: host [n_scen][n_cells] fp32 (req/min);
// scen_held: host [n_scen][n_cells] int32, -1 where the scenario's allocation
// is not on the cell, else the replicas held there (at most one cell per
// server and scenario). The out pointers name pinned buffers valid until the
// next planning pass: hf [n_scen][6][n_srv] fp32 (itl, ttft, rho, rate,
// slo_rate, cost), hi [n_scen][4][n_srv] i32 (status, accelerator, held,
// needed), counts [n_scen][6] u64 (servers per status) and deficit [n_scen]
// [n_acc] u64. wva_ctx_plan_cells works on the result: the ten arrays carry
// the hold meanings (status, held flag, held, needed, cost, slo_rate, itl,
// ttft, rho, rate). The reconcile layout, the fused tick's task table, done[]
// and the captured graph are not touched. -39: the held array could not be
// allocated (the context is intact).
extern "C" int wva_ctx_hold(void *ctx, int n_scen, int n_acc, const float *scen_arrival,
                            const int *scen_held, const void **out_hf, const void **out_hi,
                            const void **out_counts, const void **out_deficit) {
  WvaCtx *c = (WvaCtx *)ctx;
  if (c == nullptr || scen_held == nullptr) return -31;
  const WvaHoldIn hold = {scen_held};
  const void *tot = nullptr;
  const int rc = wva_plan_run(c, n_scen, n_acc, scen_arrival, nullptr, out_hf, out_hi, &tot,
                              nullptr, nullptr, nullptr, &hold);
  if (rc != 0) return rc;
  if (out_counts) *out_counts = tot;
  if (out_deficit)
    *out_deficit = (const unsigned long long *)tot + (size_t)n_scen * WVA_HOLD_STATUSES;
  return 0;
}

// ---------------------------------------------------------------------------
// Forecast ensembles: n_paths rollouts of n_steps ticks from one start
// allocation, delivered in passes of whole paths, then the order statistics
// across the paths. Ensemble row e * n_steps + s is tick s of path e.
// ---------------------------------------------------------------------------
static void wva_ens_layout(const WvaCtx *c, int n_paths, int n_steps, int n_acc, int n_q,
                           WvaEnsLayout *lay) {
  const size_t rows = (size_t)n_paths * (size_t)n_steps;
  const size_t b_rec = rows * (size_t)c->n_srv * 4;
  const size_t b_band = (size_t)n_q * (size_t)n_steps * (size_t)c->n_srv * 4;
  const size_t b_mode = (size_t)n_steps * (size_t)c->n_srv * 4;
  const size_t size[WvaEnsLayout::D_N] = {
      b_rec, b_rec, b_rec, rows * (size_t)n_acc * 8, rows * 4, rows * 4, rows * 8,
      (size_t)n_paths * 3 * (size_t)c->n_srv * 4, b_band, b_band, b_mode, b_mode,
      (size_t)n_q * (size_t)n_steps * (size_t)(n_acc + 3) * 8};
  lay->dev_bytes = wva_arena_layout(size, WvaEnsLayout::D_N, lay->off);
  lay->pin_bytes = lay->dev_bytes - lay->off[WvaEnsLayout::D_TOT];
}

static void wva_ens_release(WvaCtx *c) {
  wva_arena_free(c->ens_dev, c->ens_pin);
  c->ens_dev_cap = c->ens_pin_cap = 0;
  c->ens_paths = c->ens_next = 0;
}

// (re)allocate the ensemble arena for a layout; on failure nothing is held and
// reconciles and the planning calls keep working
static int wva_ens_reserve(WvaCtx *c, const WvaEnsLayout &lay) {
  if (lay.dev_bytes <= c->ens_dev_cap && lay.pin_bytes <= c->ens_pin_cap) return 0;
  const size_t dcap = lay.dev_bytes > c->ens_dev_cap ? lay.dev_bytes : c->ens_dev_cap;
  const size_t pcap = lay.pin_bytes > c->ens_pin_cap ? lay.pin_bytes : c->ens_pin_cap;
  wva_ens_release(c);
  if (!wva_arena_alloc(c, dcap, pcap, false, &c->ens_dev, &c->ens_pin)) return -40;
  c->ens_dev_cap = dcap;
  c->ens_pin_cap = pcap;
  return 0;
}

// One pass of an ensemble of n_total paths x n_steps ticks with n_q quantiles:
// the n_paths paths from path0 on, scen_arrival being their host [n_paths *
// n_steps][n_cells] fp32 arrivals (req/min), n_paths * n_steps <=
// WVA_PLAN_MAX_S. The passes of an ensemble arrive in path order; the one with
// path0 == 0 opens it (the arena is reserved and its sums are zeroed), and
// every pass brings the same start allocation cur_acc / cur_rep / cur_cost
// (host [n_srv]), which the caller staged the tick with. wva_ctx_plan's
// staging, uploads and buckets, then wva_rollout_paths; the results stay in
// the ensemble arena. With full the pass's records are downloaded as by
// wva_ctx_rollout: out_pf [n_paths * n_steps][6][n_srv] fp32, out_pi [..][4]
// [n_srv] i32, pinned, valid until the next planning pass. Ends in a
// synchronise. -40: the arena could not be allocated (the context is intact).
extern "C" int wva_ctx_ensemble_pass(void *ctx, int n_total, int n_steps, int n_q, int n_acc,
                                     int path0, int n_paths, const float *scen_arrival,
                                     const int *cur_acc, const int *cur_rep,
                                     const float *cur_cost, int full, const void **out_pf,
                                     const void **out_pi) {
  WvaCtx *c = (WvaCtx *)ctx;
  if (c == nullptr || cur_acc == nullptr || cur_rep == nullptr || cur_cost == nullptr) return -31;
  if (n_total < 1 || n_total > WVA_ENS_MAX_PATHS || n_steps < 1 || n_steps > WVA_PLAN_MAX_S ||
      n_q < 1 || n_q > WVA_ENS_MAX_Q || n_acc < 1 || n_paths < 1 || path0 < 0 ||
      n_paths > WVA_PLAN_MAX_S / n_steps || path0 > n_total - n_paths)
    return -32;
  if (c->n_cells <= 0 || c->n_srv <= 0) return -33;
  WvaEnsLayout lay;
  wva_ens_layout(c, n_total, n_steps, n_acc, n_q, &lay);
  if (path0 == 0) {
    c->ens_paths = c->ens_next = 0;
    const int rc = wva_ens_reserve(c, lay);
    if (rc != 0) return rc;
    // the integer sums start from zero: TOT, NOWIN and CHG follow each other
    if (hipMemsetAsync((char *)c->ens_dev + lay.off[WvaEnsLayout::D_TOT], 0,
                       lay.off[WvaEnsLayout::D_RCOST] - lay.off[WvaEnsLayout::D_TOT],
                       c->s0) != hipSuccess)
      return -2;
    c->ens_paths = n_total;
    c->ens_steps = n_steps;
    c->ens_acc = n_acc;
    c->ens_q = n_q;
  } else if (c->ens_paths != n_total || c->ens_steps != n_steps || c->ens_acc != n_acc ||
             c->ens_q != n_q || c->ens_next != path0) {
    return -32;  // not the next pass of the ensemble under way
  }
  const WvaRollArgs roll = {cur_acc, cur_rep, cur_cost};
  const WvaEnsArgs ens = {n_paths, n_steps, path0, full ? 1 : 0, &lay};
  const int rc = wva_plan_run(c, n_paths * n_steps, n_acc, scen_arrival, nullptr, out_pf, out_pi,
                              nullptr, nullptr, &roll, nullptr, nullptr, &ens);
  if (rc != 0) {
    c->ens_paths = c->ens_next = 0;  // the ensemble is void
    return rc;
  }
  c->ens_next = path0 + n_paths;
  return 0;
}

// The bands of the ensemble whose last pass has run: the per-row cost sums
// (wva_ensemble_cost), then wva_ensemble_bands with the n_q ranks (0-based,
// below the path count), then the downloads. out[10] names pinned buffers
// valid until the next ensemble call: per-row totals u64 [rows][n_acc],
// servers without a winner i32 [rows], accelerator changes i32 [rows], cost
// f64 [rows]; the final allocations i32 [paths][3][n_srv] (downloaded only
// with want_final, else null); server replica bands i32 [n_q][n_steps][n_srv],
// server cost bands f32 of the same shape, mode and mode_paths i32 [n_steps]
// [n_srv]; fleet bands [n_q][n_steps][n_acc + 3] 8-byte words (i64 replica
// totals per accelerator, servers without a winner, accelerator changes, then
// the f64 cost). Ends in a synchronise.
extern "C" int wva_ctx_ensemble_bands(void *ctx, const int *ranks, int n_q, int want_final,
                                      const void **out) {
  WvaCtx *c = (WvaCtx *)ctx;
  if (c == nullptr || ranks == nullptr || out == nullptr) return -31;
  if (c->ens_paths < 1 || c->ens_next != c->ens_paths || n_q != c->ens_q) return -32;
  WvaEnsRanks rk = {};
  for (int q = 0; q < n_q; ++q) {
    if (ranks[q] < 0 || ranks[q] >= c->ens_paths) return -32;
    rk.k[q] = ranks[q];
  }
  typedef WvaEnsLayout L;
  L lay;
  wva_ens_layout(c, c->ens_paths, c->ens_steps, c->ens_acc, n_q, &lay);
  char *d = (char *)c->ens_dev, *h = (char *)c->ens_pin;
  const int rows = c->ens_paths * c->ens_steps;
  hipLaunchKernelGGL(wva_ensemble_cost, dim3((rows + WVA_WAVE - 1) / WVA_WAVE), dim3(WVA_WAVE), 0,
                     c->s0, (const float *)(d + lay.off[L::D_COST]), c->n_srv, rows,
                     (double *)(d + lay.off[L::D_RCOST]));
  hipLaunchKernelGGL(
      wva_ensemble_bands, dim3(c->ens_steps * (c->n_srv + c->ens_acc + 3)), dim3(WVA_WAVE), 0,
      c->s0, (const int *)(d + lay.off[L::D_CODE]), (const int *)(d + lay.off[L::D_REPS]),
      (const float *)(d + lay.off[L::D_COST]),
      (const unsigned long long *)(d + lay.off[L::D_TOT]), (const int *)(d + lay.off[L::D_NOWIN]),
      (const int *)(d + lay.off[L::D_CHG]), (const double *)(d + lay.off[L::D_RCOST]), c->n_srv,
      c->ens_acc, c->ens_steps, c->ens_paths, n_q, rk, (int *)(d + lay.off[L::D_SRQ]),
      (float *)(d + lay.off[L::D_SCQ]), (int *)(d + lay.off[L::D_MODE]),
      (int *)(d + lay.off[L::D_MODEP]), (long long *)(d + lay.off[L::D_FLEET]));
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return (int)err;
  // the aggregates, the final allocations when asked, the bands
  const int from[3] = {L::D_TOT, L::D_FIN, L::D_SRQ};
  const size_t to[3] = {lay.off[L::D_FIN], lay.off[L::D_SRQ], lay.dev_bytes};
  for (int i = 0; i < 3; ++i) {
    if (i == 1 && !want_final) continue;
    err = hipMemcpyAsync(h + lay.pin(from[i]), d + lay.off[from[i]], to[i] - lay.off[from[i]],
                         hipMemcpyDeviceToHost, c->s0);
    if (err != hipSuccess) return (int)err;
  }
  err = hipStreamSynchronize(c->s0);
  if (err != hipSuccess) return (int)err;
  const int segs[10] = {L::D_TOT, L::D_NOWIN, L::D_CHG,  L::D_RCOST, L::D_FIN,
                        L::D_SRQ, L::D_SCQ,   L::D_MODE, L::D_MODEP, L::D_FLEET};
  for (int i = 0; i < 10; ++i) out[i] = h + lay.pin(segs[i]);
  if (!want_final) out[4] = nullptr;
  return 0;
}

// Per-cell outputs of the last successful wva_ctx_plan, copied into ten host
// arrays of plan_s * n_cells elements each, in WvaCellsOut order (feasible,
// zero_empty: u8; num_replicas, batch: i32; cost, value, itl, ttft, rho,
// max_rate: f32). Synchronous; inspection and tests, not the hot path.
extern "C" int wva_ctx_plan_cells(void *ctx, void **dst) {
  WvaCtx *c = (WvaCtx *)ctx;
  if (c == nullptr || dst == nullptr || c->plan_s < 1) return -31;
  const size_t cells = (size_t)c->plan_s * (size_t)c->n_cells;
  const void *src[10] = {c->plan_out.feasible, c->plan_out.zero_empty, c->plan_out.num_replicas,
                         c->plan_out.batch,    c->plan_out.cost,       c->plan_out.value,
                         c->plan_out.itl,      c->plan_out.ttft,       c->plan_out.rho,
                         c->plan_out.max_rate};
  if (hipStreamSynchronize(c->s0) != hipSuccess) return -1;
  for (int i = 0; i < 10; ++i) {
    const size_t bytes = cells * (i < 2 ? 1 : 4);
    if (hipMemcpy(dst[i], src[i], bytes, hipMemcpyDeviceToHost) != hipSuccess) return -2;
  }
  return 0;
}

extern "C" void wva_ctx_destroy(void *ctx) {
  WvaCtx *c = (WvaCtx *)ctx;
  if (c == nullptr) return;
  if (c->graph_state == 1) (void)hipGraphExecDestroy(c->graph_exec);
  (void)hipStreamDestroy(c->s0);
  (void)hipEventDestroy(c->e_up);
  for (int i = 0; i < WVA_MAX_BUCKETS - 1; ++i) {
    (void)hipStreamDestroy(c->side[i]);
    (void)hipEventDestroy(c->e_b[i]);
  }
  if (c->memo != nullptr) (void)hipFree(c->memo);
  if (c->done != nullptr) (void)hipFree(c->done);
  if (c->dev_cell_server != nullptr) (void)hipFree(c->dev_cell_server);
  if (c->tasks != nullptr) (void)hipFree(c->tasks);
  wva_plan_release(c);
  wva_slo_release(c);
  wva_tok_release(c);
  wva_hold_release(c);
  wva_lim_release(c);
  wva_arena_free(c->roll_dev, c->roll_pin);
  wva_ens_release(c);
  if (c->lim_static != nullptr) (void)hipFree(c->lim_static);
  free(c->topo);
  delete c;
}
