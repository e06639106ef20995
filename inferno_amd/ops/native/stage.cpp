// Host-only prologue and epilogue of the reconcile tick. No HIP in here: both
// functions run without a device context, so they are tested on the CPU and
// under a host sanitizer (ops/native/stage_driver.cpp).
//
//  * wva_stage_dynamic: per-server dynamic state -> the eight dynamic per-cell
//    rows the sweep reads. The reference for every detail is
//    FastSweep._refresh_dynamic (engine/fastpath.py); the rows are equal to its
//    arrays byte for byte.
//  * wva_aggregate_by_type: per-accelerator-type unit counts and costs of the
//    winners (ShardedSolver._aggregate_by_type, parallel/dist.py).
#include "wva_stage.h"

#include <cstddef>

namespace {
// engine/snapshot.py
constexpr int kFlagCurSame = 1;
constexpr int kFlagCurEmpty = 2;
constexpr int kFlagHasCur = 4;
constexpr int kCurNone = -3;   // no current allocation
constexpr int kCurEmpty = -1;  // current allocation on no (known) accelerator
}  // namespace

// Arguments and return codes: wva_stage.h.
extern "C" int wva_stage_dynamic(int n_srv, int n_cells, const float *arrival, const int *in_tok,
                                 const int *out_tok, const int *cur_acc, const int *cur_rep,
                                 const float *cur_cost, const float *zero_arrival,
                                 const int *cell_server, const int *cell_acc_idx,
                                 const int *perf_max_batch_cfg, const int *at_tokens,
                                 const int *override_n, void *out, const int *prev_batch_n,
                                 int *changed) {
  if (n_srv < 0 || n_cells < 0 || out == nullptr) return -1;
  if (n_cells > 0 && (arrival == nullptr || in_tok == nullptr || out_tok == nullptr ||
                      cur_acc == nullptr || cur_rep == nullptr || cur_cost == nullptr ||
                      cell_server == nullptr || cell_acc_idx == nullptr ||
                      perf_max_batch_cfg == nullptr || at_tokens == nullptr ||
                      override_n == nullptr))
    return -1;
  if (zero_arrival == nullptr) zero_arrival = arrival;
  const size_t n = (size_t)n_cells;
  int32_t *oi = static_cast<int32_t *>(out);
  float *of = static_cast<float *>(out);
  int32_t *r_in = oi + WVA_ROW_IN_TOK * n;
  int32_t *r_out = oi + WVA_ROW_OUT_TOK * n;
  int32_t *r_batch = oi + WVA_ROW_BATCH_N * n;
  int32_t *r_pmb = oi + WVA_ROW_PERF_MAX_BATCH * n;
  int32_t *r_rep = oi + WVA_ROW_CUR_REPLICAS * n;
  int32_t *r_flags = oi + WVA_ROW_FLAGS * n;
  float *r_arr = of + WVA_ROW_ARRIVAL * n;
  float *r_cost = of + WVA_ROW_CUR_COST * n;
  bool diff = prev_batch_n == nullptr;
  for (int k = 0; k < n_cells; ++k) {
    const int s = cell_server[k];
    if (s < 0 || s >= n_srv) return -2;
    const int c_out = out_tok[s];
    const int ovr = override_n[k];
    int base;
    if (ovr > 0) {
      base = ovr;
    } else {
      // numpy's // floors and C++'s / truncates; they differ only for a
      // negative product, where both quotients are <= 0 and the max(..., 1)
      // makes either one 1. The int32 cast wraps like .astype(np.int32).
      const int64_t prod = (int64_t)perf_max_batch_cfg[k] * (int64_t)at_tokens[k];
      const int64_t safe_k = c_out > 1 ? (int64_t)c_out : 1;
      int64_t scaled = prod / safe_k;
      if (scaled < 1) scaled = 1;
      base = (int32_t)(uint32_t)(uint64_t)scaled;
    }
    // a NaN rate compares unequal to 0, so it is not zero-load (as in numpy)
    const bool zero_load = (zero_arrival[s] == 0.0f) || (c_out == 0);
    const int32_t batch_n = zero_load ? 1 : base;
    if (!diff && prev_batch_n[k] != batch_n) diff = true;
    const int ca = cur_acc[s];
    int32_t flags = ca != kCurNone ? kFlagHasCur : 0;
    if (ca == cell_acc_idx[k]) flags |= kFlagCurSame;
    if (ca == kCurEmpty) flags |= kFlagCurEmpty;
    r_in[k] = in_tok[s];
    r_out[k] = c_out;
    r_batch[k] = batch_n;
    r_pmb[k] = ovr > 0 ? ovr : perf_max_batch_cfg[k];
    r_rep[k] = cur_rep[s];
    r_flags[k] = flags;
    r_arr[k] = arrival[s];
    r_cost[k] = cur_cost[s];
  }
  if (changed != nullptr) *changed = diff ? 1 : 0;
  return 0;
}

// Per-type accelerator units and cost of the selected winners: a server counts
// when valid[i] != 0 and acc_idx[i] >= 0 (-1 none and -2 zero-load empty do
// not). Servers are visited in ascending order with one fp64 add each, the
// order np.add.at uses, so the cost sums carry the same bits as the numpy
// path. The unit product replicas * inst * mult is formed in int64; the numpy
// path forms it in int32 and widens afterwards, so the two differ only where
// that one overflowed.
// Arguments and return codes: wva_stage.h.
extern "C" int wva_aggregate_by_type(int n_srv, int n_acc, int n_types, const int *acc_idx,
                                     const int *num_replicas, const float *cost,
                                     const uint8_t *valid, const int *inst, const int *mult,
                                     const int *type_idx, int64_t *out_count, double *out_cost) {
  if (n_srv < 0 || n_acc < 0 || n_types < 0) return -1;
  if (n_types > 0 && (out_count == nullptr || out_cost == nullptr)) return -1;
  for (int t = 0; t < n_types; ++t) {
    out_count[t] = 0;
    out_cost[t] = 0.0;
  }
  if (n_srv > 0 && (acc_idx == nullptr || num_replicas == nullptr || cost == nullptr ||
                    valid == nullptr))
    return -1;
  for (int i = 0; i < n_srv; ++i) {
    if (!valid[i]) continue;
    const int a = acc_idx[i];
    if (a < 0) continue;
    if (a >= n_acc || inst == nullptr || mult == nullptr || type_idx == nullptr) return -2;
    const int t = type_idx[a];
    if (t < 0 || t >= n_types) return -2;
    // unsigned arithmetic: wraps instead of overflowing on absurd inputs
    const uint64_t units = (uint64_t)(int64_t)num_replicas[i] *
                           (uint64_t)(int64_t)inst[(size_t)i * (size_t)n_acc + (size_t)a] *
                           (uint64_t)(int64_t)mult[a];
    out_count[t] = (int64_t)((uint64_t)out_count[t] + units);
    out_cost[t] += (double)cost[i];
  }
  return 0;
}
