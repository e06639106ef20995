// Stand-alone driver for ops/native/stage.cpp, meant to be built together with
// it under a host sanitizer (make asan-stage):
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all
//       stage.cpp stage_driver.cpp -o stage_driver && ./stage_driver
// Random topologies and loads at 0, 1 and a few hundred cells; every output
// buffer is allocated at its exact size so an out-of-bounds access trips the
// sanitizer. Results are checked against a plain restatement of the rules.
// Also checks the arena layout of wva_arena.h (the context's planning and
// greedy buffers). Exits 0 when all is well.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "wva_arena.h"
#include "wva_stage.h"

static int failures = 0;
#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                         \
    }                                                                     \
  } while (0)

struct Fleet {
  int n_srv, n_acc, n_cells;
  std::vector<float> arrival, zero_arrival, cur_cost;
  std::vector<int> in_tok, out_tok, cur_acc, cur_rep;
  std::vector<int> cell_server, cell_acc, cfg, at_tokens, override_n;
};

static Fleet make_fleet(std::mt19937 &rng, int n_srv, int n_acc) {
  Fleet f;
  f.n_srv = n_srv;
  f.n_acc = n_acc;
  auto u = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rng); };
  for (int s = 0; s < n_srv; ++s) {
    const int r = u(0, 9);
    f.arrival.push_back(r == 0 ? 0.0f : r == 1 ? std::nanf("") : (float)u(1, 100000) / 7.0f);
    f.zero_arrival.push_back(u(0, 3) == 0 ? 0.0f : f.arrival.back());
    f.in_tok.push_back(u(0, 4096));
    const int o = u(0, 11);
    f.out_tok.push_back(o == 0 ? 0 : o == 1 ? std::numeric_limits<int>::max()
                                 : o == 2 ? -u(1, 50) : u(1, 2048));
    f.cur_acc.push_back(u(-3, n_acc - 1));
    f.cur_rep.push_back(u(0, 40));
    f.cur_cost.push_back((float)u(0, 90000) / 3.0f);
    // a server has a cell on a random subset of the accelerators
    for (int a = 0; a < n_acc; ++a) {
      if (u(0, 4) == 0) continue;
      f.cell_server.push_back(s);
      f.cell_acc.push_back(a);
      const int c = u(0, 20);
      f.cfg.push_back(c == 0 ? std::numeric_limits<int>::max() : c == 1 ? -u(1, 64) : u(1, 512));
      f.at_tokens.push_back(c == 0 ? std::numeric_limits<int>::max() : u(1, 4096));
      f.override_n.push_back(u(0, 2) == 0 ? u(1, 9000) : 0);
    }
  }
  f.n_cells = (int)f.cell_server.size();
  return f;
}

// the rules, restated cell by cell (FastSweep._refresh_dynamic)
static void expect_rows(const Fleet &f, bool use_zero, std::vector<int32_t> &rows) {
  const size_t n = (size_t)f.n_cells;
  rows.assign(8 * n, 0);
  for (size_t k = 0; k < n; ++k) {
    const int s = f.cell_server[k];
    const int out = f.out_tok[s];
    int64_t base;
    if (f.override_n[k] > 0) {
      base = f.override_n[k];
    } else {
      const int64_t prod = (int64_t)f.cfg[k] * (int64_t)f.at_tokens[k];
      const int64_t div = out > 1 ? out : 1;
      int64_t q = prod / div;  // floor division, as numpy's //
      if (prod % div != 0 && ((prod < 0) != (div < 0))) --q;
      base = q > 1 ? q : 1;
    }
    const float za = use_zero ? f.zero_arrival[s] : f.arrival[s];
    const bool zero = za == 0.0f || out == 0;
    int flags = f.cur_acc[s] != -3 ? 4 : 0;
    if (f.cur_acc[s] == f.cell_acc[k]) flags |= 1;
    if (f.cur_acc[s] == -1) flags |= 2;
    rows[0 * n + k] = f.in_tok[s];
    rows[1 * n + k] = out;
    rows[2 * n + k] = zero ? 1 : (int32_t)(uint32_t)(uint64_t)base;
    rows[3 * n + k] = f.override_n[k] > 0 ? f.override_n[k] : f.cfg[k];
    rows[4 * n + k] = f.cur_rep[s];
    rows[5 * n + k] = flags;
    std::memcpy(&rows[6 * n + k], &f.arrival[s], 4);
    std::memcpy(&rows[7 * n + k], &f.cur_cost[s], 4);
  }
}

static int stage(const Fleet &f, bool use_zero, int32_t *out, const int *prev, int *changed) {
  return wva_stage_dynamic(f.n_srv, f.n_cells, f.arrival.data(), f.in_tok.data(),
                           f.out_tok.data(), f.cur_acc.data(), f.cur_rep.data(),
                           f.cur_cost.data(), use_zero ? f.zero_arrival.data() : nullptr,
                           f.cell_server.data(), f.cell_acc.data(), f.cfg.data(),
                           f.at_tokens.data(), f.override_n.data(), out, prev, changed);
}

static void check_stage(std::mt19937 &rng, int n_srv, int n_acc) {
  Fleet f = make_fleet(rng, n_srv, n_acc);
  const size_t n = (size_t)f.n_cells;
  std::vector<int32_t> want, want2;
  // exact-size heap blocks (never empty vectors' null data for the output)
  int32_t *out = new int32_t[8 * n + (n == 0 ? 1 : 0)];
  int32_t *out2 = new int32_t[8 * n + (n == 0 ? 1 : 0)];
  for (int use_zero = 0; use_zero < 2; ++use_zero) {
    expect_rows(f, use_zero != 0, want);
    int changed = -1;
    CHECK(stage(f, use_zero != 0, out, nullptr, &changed) == 0);
    CHECK(changed == 1);  // nothing to compare against
    CHECK(n == 0 || std::memcmp(out, want.data(), 8 * n * 4) == 0);
    // against its own batch_n: unchanged, same bytes
    changed = -1;
    CHECK(stage(f, use_zero != 0, out2, out + 2 * n, &changed) == 0);
    CHECK(changed == 0);
    CHECK(n == 0 || std::memcmp(out2, want.data(), 8 * n * 4) == 0);
  }
  // next tick: loads move, some token averages too
  std::vector<int32_t> prev(out2 + 2 * n, out2 + 3 * n);
  for (int s = 0; s < f.n_srv; ++s) {
    if (rng() % 3 == 0) f.out_tok[s] = (int)(rng() % 3000);
    if (rng() % 4 == 0) f.arrival[s] = rng() % 2 ? 0.0f : 17.5f;
    f.cur_acc[s] = (int)(rng() % (unsigned)(n_acc + 3)) - 3;
  }
  expect_rows(f, false, want2);
  int changed = -1;
  const int32_t none = 0;  // an empty vector's data() may be null, which means "no previous row"
  CHECK(stage(f, false, out, n != 0 ? prev.data() : &none, &changed) == 0);
  CHECK(n == 0 || std::memcmp(out, want2.data(), 8 * n * 4) == 0);
  const bool differs = n != 0 && std::memcmp(prev.data(), want2.data() + 2 * n, n * 4) != 0;
  CHECK(changed == (differs ? 1 : 0));
  // a cell pointing at a server that does not exist is refused, not read
  if (n > 0) {
    f.cell_server[n / 2] = f.n_srv;
    CHECK(stage(f, false, out, nullptr, &changed) == -2);
  }
  delete[] out;
  delete[] out2;
}

static void check_aggregate(std::mt19937 &rng, int n_srv, int n_acc, int n_types) {
  auto u = [&](int lo, int hi) { return std::uniform_int_distribution<int>(lo, hi)(rng); };
  std::vector<int> acc(n_srv), reps(n_srv), inst((size_t)n_srv * n_acc), mult(n_acc), tidx(n_acc);
  std::vector<float> cost(n_srv);
  std::vector<uint8_t> valid(n_srv);
  for (int a = 0; a < n_acc; ++a) {
    mult[a] = u(1, 8);
    tidx[a] = u(0, n_types - 1);
  }
  for (int i = 0; i < n_srv; ++i) {
    acc[i] = u(-2, n_acc - 1);
    reps[i] = u(0, 3) == 0 ? std::numeric_limits<int>::max() : u(0, 500);
    cost[i] = (float)u(0, 1 << 20) * 0.37f;
    valid[i] = u(0, 5) != 0;
    for (int a = 0; a < n_acc; ++a) inst[(size_t)i * n_acc + a] = u(0, 8);
  }
  std::vector<int64_t> want_count(n_types, 0);
  std::vector<double> want_cost(n_types, 0.0);
  for (int i = 0; i < n_srv; ++i) {
    if (!valid[i] || acc[i] < 0) continue;
    const int t = tidx[acc[i]];
    want_count[t] += (int64_t)reps[i] * inst[(size_t)i * n_acc + acc[i]] * mult[acc[i]];
    want_cost[t] += (double)cost[i];
  }
  int64_t *count = new int64_t[n_types];
  double *csum = new double[n_types];
  CHECK(wva_aggregate_by_type(n_srv, n_acc, n_types, acc.data(), reps.data(), cost.data(),
                              valid.data(), inst.data(), mult.data(), tidx.data(), count,
                              csum) == 0);
  CHECK(std::memcmp(count, want_count.data(), n_types * sizeof(int64_t)) == 0);
  CHECK(std::memcmp(csum, want_cost.data(), n_types * sizeof(double)) == 0);
  if (n_srv > 0) {
    acc[0] = n_acc;  // out of range: refused
    valid[0] = 1;
    CHECK(wva_aggregate_by_type(n_srv, n_acc, n_types, acc.data(), reps.data(), cost.data(),
                                valid.data(), inst.data(), mult.data(), tidx.data(), count,
                                csum) == -2);
  }
  delete[] count;
  delete[] csum;
}

// wva_arena_layout: offsets 256-aligned, segments disjoint and in table
// order, total = the sum of the padded sizes; a zero-sized segment takes no
// room. The table is written into a block of exactly `total` bytes, each
// segment filled with its own index, so an overlap or an overrun shows.
static void check_arena(const std::vector<size_t> &sizes) {
  const int n = (int)sizes.size();
  std::vector<size_t> off((size_t)n + 1, (size_t)-1);  // one spare slot: must stay untouched
  const size_t total = wva_arena_layout(sizes.data(), n, off.data());
  CHECK(off[(size_t)n] == (size_t)-1);
  size_t want = 0;
  for (int i = 0; i < n; ++i) {
    CHECK(off[i] % 256 == 0);
    CHECK(off[i] == want);  // in order, right behind the padded predecessor
    CHECK(off[i] + sizes[i] <= (i + 1 < n ? off[i + 1] : total));  // disjoint
    want += (sizes[i] + 255) / 256 * 256;
  }
  CHECK(total == want);
  CHECK(total % 256 == 0);
  unsigned char *block = new unsigned char[total + (total == 0 ? 1 : 0)];
  for (int i = 0; i < n; ++i) std::memset(block + off[i], i + 1, sizes[i]);
  for (int i = 0; i < n; ++i)
    for (size_t k = 0; k < sizes[i]; ++k)
      if (block[off[i] + k] != (unsigned char)(i + 1)) {
        CHECK(!"segment overwritten by a later one");
        break;
      }
  delete[] block;
}

static void check_arenas(std::mt19937 &rng) {
  CHECK(wva_align256(0) == 0 && wva_align256(1) == 256 && wva_align256(255) == 256);
  CHECK(wva_align256(256) == 256 && wva_align256(257) == 512);
  size_t none = 12345;
  CHECK(wva_arena_layout(nullptr, 0, &none) == 0 && none == 12345);  // empty table
  const size_t edge[] = {0, 1, 255, 256, 257, 4096, 100001};
  for (size_t a : edge) {
    check_arena({a});
    for (size_t b : edge) {
      check_arena({a, b});
      check_arena({a, 0, b, 0});
      check_arena({0, 0, a, b, 1});
    }
  }
  // the planning arena's shape: nine 4-byte and two 1-byte per-cell arrays, three tails
  for (int rep = 0; rep < 50; ++rep) {
    const size_t cells = rng() % 3000, pf = rng() % 5000, tot = rng() % 300;
    std::vector<size_t> t(9, cells * 4);
    t.insert(t.end(), {cells, cells, pf * 6, pf * 4, tot * 8});
    check_arena(t);
  }
}

int main() {
  std::mt19937 rng(20240607u);
  check_arenas(rng);
  const int sizes[] = {0, 1, 2, 7, 64, 130, 300};
  for (int n_srv : sizes)
    for (int n_acc : {1, 3, 8})
      for (int rep = 0; rep < 4; ++rep) {
        check_stage(rng, n_srv, n_acc);
        check_aggregate(rng, n_srv, n_acc, 1 + (int)(rng() % 4));
      }
  if (failures != 0) {
    std::fprintf(stderr, "stage_driver: %d check(s) failed\n", failures);
    return 1;
  }
  std::puts("stage_driver: ok");
  return 0;
}
