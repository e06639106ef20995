// Shared by ops/native/stage.cpp, its stand-alone driver and
// ops/hip/wva_kernels.hip: the layout of the dynamic block, the tick code and
// the C ABI of the host-only staging and aggregation. ops/sweep.py mirrors
// WVA_DYN_ROWS (DYN_ROWS) and WVA_TICK_STALE (TICK_STALE); load_library()
// checks both against wva_abi().
#ifndef WVA_STAGE_H
#define WVA_STAGE_H

#include <stdint.h>

// rows of the dynamic block, each n_cells 4-byte words: six int32 rows, then
// two fp32 rows
enum {
  WVA_ROW_IN_TOK = 0,
  WVA_ROW_OUT_TOK = 1,
  WVA_ROW_BATCH_N = 2,
  WVA_ROW_PERF_MAX_BATCH = 3,
  WVA_ROW_CUR_REPLICAS = 4,
  WVA_ROW_FLAGS = 5,
  WVA_ROW_ARRIVAL = 6,
  WVA_ROW_CUR_COST = 7,
  WVA_DYN_ROWS = 8,
};

// wva_ctx_tick: "bucket layout stale, nothing launched". Above every
// hipError_t value, which the tick otherwise passes through.
#define WVA_TICK_STALE (1 << 20)

#ifdef __cplusplus
extern "C" {
#endif

// Per-server inputs [n_srv]: arrival f32, in_tok/out_tok i32, cur_acc i32
// (-3 none, -1 empty, >= 0 accelerator index), cur_rep i32, cur_cost f32.
// zero_arrival (may be null = arrival) is the per-server rate the zero-load
// decision looks at; planning passes the maximum over its scenarios.
// Static per-cell topology [n_cells]: cell_server, cell_acc_idx,
// perf_max_batch_cfg, at_tokens, override_n.
// out: WVA_DYN_ROWS x n_cells words in the row order above.
// prev_batch_n (may be null): a batch_n row to compare against; *changed
// (may be null) is set to 1 when the new row differs from it (or when it is
// null), else 0.
// Returns 0, or -1 for a bad argument, -2 for a cell_server out of range.
int wva_stage_dynamic(int n_srv, int n_cells, const float *arrival, const int *in_tok,
                      const int *out_tok, const int *cur_acc, const int *cur_rep,
                      const float *cur_cost, const float *zero_arrival, const int *cell_server,
                      const int *cell_acc_idx, const int *perf_max_batch_cfg,
                      const int *at_tokens, const int *override_n, void *out,
                      const int *prev_batch_n, int *changed);

// Per-type accelerator units and cost of the selected winners: a server counts
// when valid[i] != 0 and acc_idx[i] >= 0 (-1 none and -2 zero-load empty do
// not). inst [n_srv][n_acc], mult [n_acc], type_idx [n_acc] (each < n_types).
// out_count [n_types] int64 and out_cost [n_types] fp64 are overwritten.
// Returns 0, -1 for a bad argument, -2 for an index out of range.
int wva_aggregate_by_type(int n_srv, int n_acc, int n_types, const int *acc_idx,
                          const int *num_replicas, const float *cost, const uint8_t *valid,
                          const int *inst, const int *mult, const int *type_idx,
                          int64_t *out_count, double *out_cost);

#ifdef __cplusplus
}
#endif

#endif  // WVA_STAGE_H
