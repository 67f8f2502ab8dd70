// lm_sanitize.cpp — the host side of the batched Levenberg-Marquardt step as a program of its own, for the host
// sanitizers: tds_hip_lm_step_host (csrc/tds_lm.hip, host code only) at the edge shapes: p = 1 and 16, m = 1 and 65
// (one entry a tile; a tile and one entry), n_lambda = 1 and 8, a problem without rows, a NaN entry, finite, pinned
// (dlo == dhi == 0), infinite and absent bounds, absent weights, the cost-only mode, and every argument error.  Every
// array is allocated at its exact size, so that an index past what is due is an address the sanitizer knows.  No GPU,
// no Python.  Build and run:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//     -Xarch_host -fno-sanitize-recover=undefined -Iinclude -Itiny-differentiable-simulator_amd/csrc \
//     tools/lm_sanitize.cpp tiny-differentiable-simulator_amd/csrc/tds_lm.hip -o lm_sanitize
//   ./lm_sanitize
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "tds_api_internal.h"

// (the library defines this in tds_api.hip, which this program does not link)
namespace tds_internal {
thread_local char g_err[512] = "";
}  // namespace tds_internal

#define EXPECT(cond)                                                                                 \
  do {                                                                                               \
    if (!(cond)) {                                                                                   \
      fprintf(stderr, "lm_sanitize: line %d: %s  [%s]\n", __LINE__, #cond, tds_internal::g_err);     \
      return 1;                                                                                      \
    }                                                                                                \
  } while (0)

static unsigned long long g_seed = 88172645463325252ull;
static double uniform(double lo, double hi) {  // xorshift64
  g_seed ^= g_seed << 13, g_seed ^= g_seed >> 7, g_seed ^= g_seed << 17;
  return lo + (hi - lo) * (double)(g_seed >> 11) / 9007199254740992.0;
}
static std::vector<double> draw(size_t n, double lo, double hi) {
  std::vector<double> v(n);
  for (double &x : v) x = uniform(lo, hi);
  return v;
}

struct Case {
  int n, rows, m, p, L;
  std::vector<int32_t> row_start;
  std::vector<double> s, s_obs, w, js, dlo, dhi, lambda;
  std::vector<double> cost, g, H, delta, pred;
  std::vector<int32_t> clamped, its, status;
  bool weights = true, bounds = true;

  int run() {
    return tds_hip_lm_step_host(n, rows, m, p, L, row_start.data(), s.data(), s_obs.data(), weights ? w.data() : nullptr,
                                p ? js.data() : nullptr, bounds && p ? dlo.data() : nullptr,
                                bounds && p ? dhi.data() : nullptr, p ? lambda.data() : nullptr, cost.data(),
                                p ? g.data() : nullptr, p ? H.data() : nullptr, p && L ? delta.data() : nullptr,
                                p && L ? pred.data() : nullptr, p && L ? clamped.data() : nullptr,
                                p && L ? its.data() : nullptr, p && L ? status.data() : nullptr);
  }
};

// counts: the rows of each problem; bound kind 0 finite, 1 infinite, 2 pinned, 3 absent
static Case make(const std::vector<int> &counts, int m, int p, int L, int kind) {
  Case c;
  c.n = (int)counts.size(), c.m = m, c.p = p, c.L = L;
  c.row_start.push_back(0);
  for (int k : counts) c.row_start.push_back(c.row_start.back() + k);
  c.rows = c.row_start.back();
  const size_t e = (size_t)c.rows * m;
  c.s = draw(e, -1, 1), c.s_obs = draw(e, -1, 1), c.w = draw(e, 0.5, 1.5), c.js = draw(e * p, -1, 1);
  for (size_t i = 0; i < e; i += 5) c.w[i] = 0.0, c.s_obs[i] = NAN;  // missing measurements
  c.dlo = draw((size_t)c.n * p, -0.01, 0), c.dhi = draw((size_t)c.n * p, 0, 0.01);
  if (kind == 1)
    for (size_t i = 0; i < c.dlo.size(); ++i) c.dlo[i] = -INFINITY, c.dhi[i] = INFINITY;
  if (kind == 2)
    for (size_t i = 0; i < c.dlo.size(); ++i) c.dlo[i] = c.dhi[i] = 0.0;
  c.bounds = kind != 3;
  c.lambda.resize((size_t)c.n * L);
  for (size_t i = 0; i < c.lambda.size(); ++i) c.lambda[i] = pow(10.0, -6.0 + (double)(i % L));
  c.cost.resize(c.n), c.g.resize((size_t)c.n * p), c.H.resize((size_t)c.n * p * p);
  c.delta.resize((size_t)c.n * L * p), c.pred.resize((size_t)c.n * L);
  c.clamped.resize((size_t)c.n * L), c.its.resize((size_t)c.n * L), c.status.resize((size_t)c.n * L);
  return c;
}

static int step(const std::vector<int> &counts, int m, int p, int L, int kind, int nan_problem) {
  Case c = make(counts, m, p, L, kind);
  if (nan_problem >= 0) {
    const size_t e = (size_t)c.row_start[nan_problem] * m + (m - 1);
    c.s[e] = NAN, c.w[e] = 1.0;
  }
  EXPECT(c.run() == TDS_OK);
  for (int i = 0; i < c.n; ++i) {
    const bool empty = counts[i] == 0, bad = i == nan_problem;
    EXPECT(bad ? c.cost[i] == INFINITY : isfinite(c.cost[i]) && (empty ? c.cost[i] == 0.0 : c.cost[i] >= 0.0));
    for (int a = 0; a < p * p; ++a) EXPECT(bad || empty ? c.H[(size_t)i * p * p + a] == 0.0 : isfinite(c.H[(size_t)i * p * p + a]));
    for (int l = 0; l < L; ++l) {
      const size_t il = (size_t)i * L + l;
      EXPECT(c.status[il] == (bad ? 2 : 0));
      EXPECT(bad ? c.pred[il] == 0.0 && c.its[il] == 0 && c.clamped[il] == 0 : c.pred[il] >= 0.0 && c.its[il] >= 1 && c.its[il] <= 100);
      EXPECT(c.clamped[il] >= 0 && c.clamped[il] < (1 << p));
      for (int a = 0; a < p; ++a) {
        const double d = c.delta[il * p + a];
        EXPECT(bad || empty || kind == 2 ? d == 0.0 : isfinite(d));
        if (c.bounds) EXPECT(bad || (d >= c.dlo[(size_t)i * p + a] && d <= c.dhi[(size_t)i * p + a]));
        if (kind == 1 || kind == 3) EXPECT(c.clamped[il] == 0);
      }
    }
  }
  // without weights (the NaN observations then count: put numbers there)
  for (double &v : c.s_obs)
    if (isnan(v)) v = 0.25;
  c.weights = false;
  EXPECT(c.run() == TDS_OK);
  // the cost-only mode prices the same residuals
  std::vector<double> full = c.cost;
  Case o = c;
  o.p = 0;
  EXPECT(o.run() == TDS_OK);
  EXPECT(o.cost == full || nan_problem >= 0);
  o.L = 0;
  EXPECT(o.run() == TDS_OK);
  return 0;
}

static int errors() {
  Case c = make({1, 2}, 9, 3, 2, 0);
  EXPECT(c.run() == TDS_OK);
  Case b = c;
  b.row_start = {1, 2, 3};
  EXPECT(b.run() == TDS_ERR_INVALID_ARG && strstr(tds_internal::g_err, "row_start does not run from 0 to rows"));
  b.row_start = {0, 1, 2};
  EXPECT(b.run() == TDS_ERR_INVALID_ARG && strstr(tds_internal::g_err, "row_start does not run from 0 to rows"));
  b.row_start = {0, 4, 3};
  EXPECT(b.run() == TDS_ERR_INVALID_ARG && strstr(tds_internal::g_err, "row_start decreases"));
  b = c, b.dhi.back() = b.dlo.back() - 1.0;
  EXPECT(b.run() == TDS_ERR_INVALID_ARG && strstr(tds_internal::g_err, "dlo > dhi or a NaN bound"));
  b = c, b.dlo[0] = NAN;
  EXPECT(b.run() == TDS_ERR_INVALID_ARG && strstr(tds_internal::g_err, "dlo > dhi or a NaN bound"));
  for (double bad : {0.0, -1.0, (double)INFINITY, (double)NAN}) {
    b = c, b.lambda.back() = bad;
    EXPECT(b.run() == TDS_ERR_INVALID_ARG && strstr(tds_internal::g_err, "a lambda that is not positive and finite"));
  }
  b = c, b.p = 17;
  EXPECT(b.run() == TDS_ERR_UNSUPPORTED && strstr(tds_internal::g_err, "16 parameters"));
  b = c, b.L = 9;
  EXPECT(b.run() == TDS_ERR_UNSUPPORTED && strstr(tds_internal::g_err, "8 candidates"));
  b = c, b.m = 0;
  EXPECT(b.run() == TDS_ERR_INVALID_ARG && strstr(tds_internal::g_err, "m must be at least 1"));
  b = c, b.n = 0;
  EXPECT(b.run() == TDS_ERR_INVALID_ARG);
  EXPECT(tds_hip_lm_step_host(c.n, c.rows, c.m, c.p, c.L, c.row_start.data(), c.s.data(), c.s_obs.data(), nullptr,
                              c.js.data(), c.dlo.data(), nullptr, c.lambda.data(), c.cost.data(), c.g.data(), c.H.data(),
                              c.delta.data(), c.pred.data(), c.clamped.data(), c.its.data(),
                              c.status.data()) == TDS_ERR_INVALID_ARG);
  EXPECT(strstr(tds_internal::g_err, "dlo and dhi are given together or not at all"));
  EXPECT(tds_hip_lm_step_host(c.n, c.rows, c.m, c.p, c.L, c.row_start.data(), c.s.data(), c.s_obs.data(), nullptr,
                              nullptr, nullptr, nullptr, c.lambda.data(), c.cost.data(), c.g.data(), c.H.data(),
                              c.delta.data(), c.pred.data(), c.clamped.data(), c.its.data(),
                              c.status.data()) == TDS_ERR_INVALID_ARG);
  EXPECT(tds_hip_lm_step(nullptr, c.n, c.rows, c.m, c.p, c.L, c.row_start.data(), c.s.data(), c.s_obs.data(), nullptr,
                         c.js.data(), nullptr, nullptr, c.lambda.data(), c.cost.data(), c.g.data(), c.H.data(),
                         c.delta.data(), c.pred.data(), c.clamped.data(), c.its.data(),
                         c.status.data()) == TDS_ERR_INVALID_ARG);
  return 0;
}

// a candidate whose system is not positive definite in double: two equal directions and a lambda that rounds away
static int singular() {
  Case c = make({1, 1, 1}, 3, 3, 2, 1);
  const size_t r = 1;
  for (int i = 0; i < 3; ++i)
    for (int e = 0; e < 3; ++e) c.js[(r * 3 + i) * 3 + e] = 0.0;
  c.js[(r * 3 + 0) * 3 + 0] = c.js[(r * 3 + 1) * 3 + 0] = 2.0, c.js[(r * 3 + 2) * 3 + 2] = 1.0;
  for (int e = 0; e < 3; ++e) c.w[r * 3 + e] = 1.0, c.s_obs[r * 3 + e] = 0.25;
  c.lambda[r * 2] = 1e-17;
  EXPECT(c.run() == TDS_OK);
  EXPECT(c.status[r * 2] == 1 && c.status[r * 2 + 1] == 0 && c.pred[r * 2] == 0.0 && c.pred[r * 2 + 1] > 0.0);
  for (int a = 0; a < 3; ++a) EXPECT(c.delta[(r * 2) * 3 + a] == 0.0);
  EXPECT(c.status[0] == 0 && c.status[1] == 0 && c.status[4] == 0 && c.status[5] == 0);
  return 0;
}

int main() {
  for (int kind = 0; kind < 4; ++kind) {
    if (step({1}, 1, 1, 1, kind, -1)) return 1;
    if (step({2, 0, 3}, 65, 16, 8, kind, -1)) return 1;
    if (step({1, 2}, 1, 16, 1, kind, -1)) return 1;
    if (step({3, 1}, 65, 1, 8, kind, -1)) return 1;
    if (step({2, 1, 2}, 64, 5, 3, kind, 1)) return 1;
  }
  if (step({0, 0}, 7, 4, 2, 0, -1)) return 1;  // no rows at all
  if (errors() || singular()) return 1;
  printf("lm_sanitize: ok\n");
  return 0;
}
