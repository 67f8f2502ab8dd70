// tds_lm.hip — batched system identification on gfx950: one Levenberg-Marquardt step of n least-squares problems as
// ONE launch.  C ABI tds_hip_lm_step and its _host checker (include/tds_hip.h); the statement is tds_lm.h's.
//
// One wavefront (a workgroup of 64 lanes) per problem.  The problem's (row, entry) sequence is walked in tiles of 64
// entries: lane l requests entry l of the NEXT tile from HBM into registers (its p derivatives, s, s_obs, w: the loads
// of a direction are coalesced along m) before the sums of this tile run, and stores it to LDS after them, so the sums
// do not wait on memory.  The (p + 1)(p + 2) / 2 running sums are owned by lanes, at most three each, in registers
// (arrays of constant extent, walked by unrolled loops: the private segment holds nothing indexed at run time); a lane
// continues its sums over the tile in entry order, so the order of every sum is the host's.  Then H is mirrored, D
// formed, and the candidates run one after the other through the box QP on the workspace that held the tile
// (11416 bytes of LDS at p = 16: below the default bound).  No MFMA, no atomics, no cross-lane operations: every
// decision is formed by every lane from LDS values.
#include <hip/hip_runtime.h>
#include <string.h>

#include <vector>

#include "tds_api_internal.h"
#include "tds_lm.h"

using namespace tds_internal;

namespace {

struct TdsLmArgs {
  int n, rows, m, p, n_lambda;
  const int *row_start;
  const double *s, *s_obs, *w, *js, *dlo, *dhi, *lambda;
  double *cost, *g, *H, *delta, *pred;
  int32_t *clamped, *qp_iterations, *status;
};

struct TdsLmBarrier {
  __device__ void operator()() const { __syncthreads(); }
};
struct TdsLmNoSync {
  void operator()() const {}
};

// problem i of the call: its bounds, candidates and outputs
TDS_HD inline TdsLmProblem tds_lm_problem(const TdsLmArgs &a, size_t i) {
  const size_t p = a.p, L = a.p ? a.n_lambda : 0;
  TdsLmProblem o;
  o.n_lambda = a.n_lambda;
  o.cost = a.cost + i;
  // (p = 0: the offsets are zero, and what may be NULL then is not read)
  o.dlo = a.dlo ? a.dlo + i * p : nullptr, o.dhi = a.dhi ? a.dhi + i * p : nullptr, o.lambda = a.lambda + i * L;
  o.g = a.g + i * p, o.H = a.H + i * p * p, o.delta = a.delta + i * L * p, o.pred = a.pred + i * L;
  o.clamped = a.clamped + i * L, o.qp_iterations = a.qp_iterations + i * L, o.status = a.status + i * L;
  return o;
}

// entry t of the sequence of a problem whose rows begin at r0: its operands (row r0 + t / m, entry t mod m)
struct TdsLmEntry {
  double js[TDS_LM_MAX_P], s, s_obs, w;

  TDS_HD inline __attribute__((always_inline)) void load(const TdsLmArgs &a, size_t r0, size_t t) {
    const size_t m = a.m, row = r0 + t / m, e = t % m;
    s = a.s[row * m + e], s_obs = a.s_obs[row * m + e], w = a.w ? a.w[row * m + e] : 1.0;
#pragma unroll
    for (int i = 0; i < TDS_LM_MAX_P; ++i)
      if (i < a.p) js[i] = a.js[(row * a.p + i) * m + e];
  }
};

__global__ void __launch_bounds__(64) tds_lm_kernel(TdsLmArgs a) {
  extern __shared__ double tds_lm_lds[];
  const int lane = threadIdx.x;
  const size_t i = blockIdx.x;
  const TdsLmWs w = tds_lm_ws(tds_lm_lds, a.p);
  // (a row_start outside [0, rows] is the caller's broken promise: clipped, so that nothing outside the arrays is read)
  int r0 = a.row_start[i], r1 = a.row_start[i + 1];
  r0 = r0 < 0 ? 0 : (r0 > a.rows ? a.rows : r0);
  r1 = r1 < r0 ? r0 : (r1 > a.rows ? a.rows : r1);
  const size_t total = (size_t)(r1 - r0) * a.m, tiles = (total + TDS_LM_TILE - 1) / TDS_LM_TILE;
  TdsLmSums<3> sums;
  sums.init(a.p, lane, 64);
  TdsLmEntry r;
  if ((size_t)lane < total) r.load(a, r0, lane);
  for (size_t t = 0; t < tiles; ++t) {
    const size_t left = total - t * TDS_LM_TILE;
    if ((size_t)lane < left) tds_lm_stage(w, lane, r.w, r.s, r.s_obs, r.js);
    __syncthreads();
    const size_t next = (t + 1) * TDS_LM_TILE + lane;
    if (next < total) r.load(a, r0, next);  // in flight while this tile's sums run
    sums.add(w.tile, left < TDS_LM_TILE ? (int)left : TDS_LM_TILE);
    __syncthreads();
  }
  sums.store(w, lane, 64);
  __syncthreads();
  tds_lm_solve(w, tds_lm_problem(a, i), lane, 64, TdsLmBarrier{});
}

int tds_lm_check_args(const char *fn, const TdsLmArgs &a) {
  const bool no_data = a.rows > 0 && (!a.s || !a.s_obs || (a.p > 0 && !a.js));
  const bool no_out = !a.cost || (a.p > 0 && (!a.g || !a.H)) ||
                      (a.p > 0 && a.n_lambda > 0 &&
                       (!a.lambda || !a.delta || !a.pred || !a.clamped || !a.qp_iterations || !a.status));
  if (a.n < 1 || a.rows < 0 || a.p < 0 || a.n_lambda < 0 || !a.row_start || no_data || no_out)
    return fail(TDS_ERR_INVALID_ARG, fn, ": NULL or empty argument");
  if (a.m < 1) return fail(TDS_ERR_INVALID_ARG, fn, ": m must be at least 1");
  if (!a.dlo != !a.dhi) return fail(TDS_ERR_INVALID_ARG, fn, ": dlo and dhi are given together or not at all");
  if (a.p > TDS_LM_MAX_P) return fail(TDS_ERR_UNSUPPORTED, fn, ": p exceeds the bound of 16 parameters");
  if (a.n_lambda > TDS_LM_MAX_LAMBDA) return fail(TDS_ERR_UNSUPPORTED, fn, ": n_lambda exceeds the bound of 8 candidates");
  return TDS_OK;
}

// the host checker: the kernel's walk with lane 0 of 1
int tds_lm_host(const TdsLmArgs &a) {
  std::vector<double> mem(tds_lm_ws_doubles(a.p));
  const TdsLmWs w = tds_lm_ws(mem.data(), a.p);
  for (size_t i = 0; i < (size_t)a.n; ++i) {
    const size_t r0 = a.row_start[i], total = (size_t)(a.row_start[i + 1] - a.row_start[i]) * a.m;
    TdsLmSums<TDS_LM_MAX_SUMS> sums;
    sums.init(a.p, 0, 1);
    for (size_t t0 = 0; t0 < total; t0 += TDS_LM_TILE) {
      const int cnt = total - t0 < (size_t)TDS_LM_TILE ? (int)(total - t0) : TDS_LM_TILE;
      for (int col = 0; col < cnt; ++col) {
        TdsLmEntry r;
        r.load(a, r0, t0 + col);
        tds_lm_stage(w, col, r.w, r.s, r.s_obs, r.js);
      }
      sums.add(w.tile, cnt);
    }
    sums.store(w, 0, 1);
    tds_lm_solve(w, tds_lm_problem(a, i), 0, 1, TdsLmNoSync{});
  }
  return TDS_OK;
}

}  // namespace

extern "C" {

int tds_hip_lm_step(tds_hip_sim_t *s, int n, int rows, int m, int p, int n_lambda, const void *row_start_dev,
                    const void *s_dev, const void *s_obs_dev, const void *w_dev, const void *js_dev, const void *dlo_dev,
                    const void *dhi_dev, const void *lambda_dev, void *cost_dev, void *g_dev, void *H_dev,
                    void *delta_dev, void *pred_dev, void *clamped_dev, void *qp_iterations_dev, void *status_dev) {
  const TdsLmArgs a = {n, rows, m, p, n_lambda, (const int *)row_start_dev, (const double *)s_dev,
                       (const double *)s_obs_dev, (const double *)w_dev, (const double *)js_dev,
                       (const double *)dlo_dev, (const double *)dhi_dev, (const double *)lambda_dev, (double *)cost_dev,
                       (double *)g_dev, (double *)H_dev, (double *)delta_dev, (double *)pred_dev,
                       (int32_t *)clamped_dev, (int32_t *)qp_iterations_dev, (int32_t *)status_dev};
  if (!s) return fail(TDS_ERR_INVALID_ARG, "tds_hip_lm_step%s", ": NULL or empty argument");
  int rc = tds_lm_check_args("tds_hip_lm_step%s", a);
  if (rc) return rc;
  DeviceGuard guard(s->device);
  hipLaunchKernelGGL(tds_lm_kernel, dim3((unsigned)n), dim3(64), tds_lm_ws_doubles(p) * sizeof(double), s->stream, a);
  TDS_HIP_TRY(hipGetLastError());
  return TDS_OK;
}

int tds_hip_lm_step_host(int n, int rows, int m, int p, int n_lambda, const int32_t *row_start, const double *s,
                         const double *s_obs, const double *w, const double *js, const double *dlo, const double *dhi,
                         const double *lambda, double *cost, double *g, double *H, double *delta, double *pred,
                         int32_t *clamped, int32_t *qp_iterations, int32_t *status) {
  const TdsLmArgs a = {n, rows, m, p, n_lambda, row_start, s, s_obs, w, js, dlo, dhi, lambda, cost, g, H, delta, pred,
                       clamped, qp_iterations, status};
  int rc = tds_lm_check_args("tds_hip_lm_step_host%s", a);
  if (rc) return rc;
  if (row_start[0] != 0 || row_start[n] != rows)
    return fail(TDS_ERR_INVALID_ARG, "tds_hip_lm_step_host: row_start does not run from 0 to rows%s");
  for (int i = 0; i < n; ++i)
    if (row_start[i + 1] < row_start[i])
      return fail(TDS_ERR_INVALID_ARG, "tds_hip_lm_step_host: row_start decreases%s");
  if (p > 0 && dlo)
    for (size_t e = 0; e < (size_t)n * p; ++e)
      if (!(dlo[e] <= dhi[e])) return fail(TDS_ERR_INVALID_ARG, "tds_hip_lm_step_host: dlo > dhi or a NaN bound%s");
  if (p > 0)
    for (size_t e = 0; e < (size_t)n * n_lambda; ++e)
      if (!(lambda[e] > 0.0) || !tds_lm_finite(lambda[e]))
        return fail(TDS_ERR_INVALID_ARG, "tds_hip_lm_step_host: a lambda that is not positive and finite%s");
  return tds_lm_host(a);
}

}  // extern "C"
