// tds_ik.hip — batched inverse kinematics on gfx950 (tds_ik.h over double) and its C ABI: tds_hip_inverse_kinematics,
// tds_hip_inverse_kinematics_host (the checker) and tds_hip_ik_default_options (include/tds_hip.h).
//
// Mapping: that of the dynamics queries (tds_dyn.hip).  One lane per environment, workgroups of W <= 64 lanes narrowed
// so that a small batch still reaches every compute unit, the environment's state (tds_ik_layout) in the handle's work
// buffer laid out [component][lane], records brought in and out through an LDS tile so that global loads and stores
// walk the records in their memory order.  The whole iteration runs inside the one launch: a lane whose environment has
// stopped leaves the loop and waits at its end for the last lane of its wave (the workgroup's barriers are all in the
// record transfers, outside the loop).
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <vector>

#include "tds_diff_classes.h"
#include "tds_ik.h"

using namespace tds_internal;

namespace {

constexpr int kTileC = 64;             // components per LDS tile
constexpr int kTileS = kTileC + 1;     // its row stride in doubles (odd: a lane's row starts on its own bank pair)
constexpr long long kIkLanes = 16384;  // lanes of a launch at most (the work buffer: 16384 states, 140 MB for Laikago's feet)

struct TdsIkArgs {
  const tds_model_t *m;
  int n;
  TdsIkParams o;
  const double *q_init, *targets, *q_ref;
  double *q, *residual;
  int *iterations, *status;
};

// records [e0, e0 + nv)[nc] of `in` -> components off .. off + nc of the workgroup's lanes
__device__ inline void tds_ik_ingest(double *tile, TdsDynMem<double> w, int off, const double *in, int nc, int e0, int nv) {
  const int W = blockDim.x, t = threadIdx.x;
  for (int c0 = 0; c0 < nc; c0 += kTileC) {
    const int tc = nc - c0 < kTileC ? nc - c0 : kTileC;
    for (int idx = t; idx < nv * tc; idx += W) {
      const int e = idx / tc, c = idx - e * tc;
      tile[e * kTileS + c] = in[(size_t)(e0 + e) * nc + c0 + c];
    }
    __syncthreads();
    if (t < nv)
      for (int c = 0; c < tc; ++c) w[off + c0 + c] = tile[t * kTileS + c];
    __syncthreads();
  }
}

// components off .. off + nc of the workgroup's lanes -> records [e0, e0 + nv)[nc] of `out`
__device__ inline void tds_ik_emit(double *tile, TdsDynMem<double> w, int off, double *out, int nc, int e0, int nv) {
  const int W = blockDim.x, t = threadIdx.x;
  for (int c0 = 0; c0 < nc; c0 += kTileC) {
    const int tc = nc - c0 < kTileC ? nc - c0 : kTileC;
    if (t < nv)
      for (int c = 0; c < tc; ++c) tile[t * kTileS + c] = w[off + c0 + c];
    __syncthreads();
    for (int idx = t; idx < nv * tc; idx += W) {
      const int e = idx / tc, c = idx - e * tc;
      out[(size_t)(e0 + e) * nc + c0 + c] = tile[e * kTileS + c];
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(64) tds_ik_kernel(TdsIkArgs a, double *buf, int lanes) {
  __shared__ double tile[64 * kTileS];
  const tds_model_t *m = a.m;
  const TdsIkLayout L = tds_ik_layout(m, a.o.k);
  const int W = blockDim.x, t = threadIdx.x, nq = m->dof_q;
  const TdsDynMem<double> w = {buf + (size_t)blockIdx.x * W + t, (size_t)lanes};
  for (int e0 = blockIdx.x * W; e0 < a.n; e0 += gridDim.x * W) {
    const int nv = a.n - e0 < W ? a.n - e0 : W;
    tds_ik_ingest(tile, w, L.d.q, a.q_init, nq, e0, nv);
    tds_ik_ingest(tile, w, L.tgt, a.targets, 3 * a.o.k, e0, nv);
    if (a.o.have_ref) tds_ik_ingest(tile, w, L.qref, a.q_ref, nq, e0, nv);
    int iterations = 0, status = TDS_IK_FAILED;
    double residual = -1.0;
    if (t < nv) {
      tds_ik_solve(m, w, L, a.o, iterations, status, residual);
      w[L.e] = residual;
    }
    tds_ik_emit(tile, w, L.d.q, a.q, nq, e0, nv);
    if (a.residual) tds_ik_emit(tile, w, L.e, a.residual, 1, e0, nv);
    if (t < nv) {  // 4 B per lane, contiguous
      if (a.iterations) a.iterations[e0 + t] = iterations;
      if (a.status) a.status[e0 + t] = status;
    }
  }
}

// lanes per workgroup: the rule of the dynamics queries (the widest of 64, 32, 16 that still gives every compute unit a
// workgroup; TDS_HIP_DYN_WIDTH overrides it, for measurements)
int tds_ik_width(const tds_hip_sim *s, int n) {
  if (const char *e = getenv("TDS_HIP_DYN_WIDTH")) {
    const int v = atoi(e);
    if (v == 16 || v == 32 || v == 64) return v;
  }
  int W = 64;
  while (W > 16 && (n + W - 1) / W < s->num_cus) W /= 2;
  return W;
}

// the arguments both entry points share, checked and packed
int tds_ik_params(const tds_model_t *m, int k, const int32_t *links, const double *body_points, const tds_ik_options_t *opt,
                  int have_ref, TdsIkParams *p) {
  tds_ik_options_t o;
  tds_hip_ik_default_options(&o);
  if (opt) o = *opt;
  if (k < 1 || k > TDS_IK_MAX_TARGETS) return fail(TDS_ERR_INVALID_ARG, "inverse kinematics: 1 to 4 targets%s");
  if (!links) return fail(TDS_ERR_INVALID_ARG, "inverse kinematics: NULL links%s");
  for (int j = 0; j < k; ++j)
    if (links[j] < 0 || links[j] >= m->num_links) return fail(TDS_ERR_INVALID_ARG, "inverse kinematics: link index out of range%s");
  if (o.max_iterations < 0) return fail(TDS_ERR_INVALID_ARG, "inverse kinematics: negative max_iterations%s");
  if (o.method != TDS_IK_TRANSPOSE && o.method != TDS_IK_PINV && o.method != TDS_IK_DAMPED_LM)
    return fail(TDS_ERR_INVALID_ARG, "inverse kinematics: unknown method%s");
  if (o.method == TDS_IK_DAMPED_LM && !(o.lambda * o.lambda > 0.0))
    return fail(TDS_ERR_INVALID_ARG, "inverse kinematics: damped LM needs lambda != 0%s");
  *p = TdsIkParams{};
  p->method = o.method, p->max_iterations = o.max_iterations, p->k = k, p->have_ref = have_ref;
  p->lambda = o.lambda, p->target_tolerance = o.target_tolerance, p->step_tolerance = o.step_tolerance;
  p->alpha = o.alpha, p->weight_reference = o.weight_reference;
  for (int j = 0; j < k; ++j) {
    p->links[j] = links[j];
    for (int c = 0; c < 3; ++c) p->pts[3 * j + c] = body_points ? body_points[3 * j + c] : 0.0;
  }
  return TDS_OK;
}

}  // namespace

extern "C" {

void tds_hip_ik_default_options(tds_ik_options_t *opt) {
  if (!opt) return;
  opt->method = TDS_IK_PINV;
  opt->max_iterations = 20;
  opt->lambda = 0.02;
  opt->target_tolerance = 1e-3;
  opt->step_tolerance = 1e-8;
  opt->alpha = 5.0;
  opt->weight_reference = 0.2;
}

int tds_hip_inverse_kinematics(tds_hip_sim_t *s, int n, const void *q_init_dev, int k, const int32_t *links,
                               const double *body_points, const void *targets_dev, const void *q_ref_dev,
                               const tds_ik_options_t *opt, void *q_dev, void *iter_dev, void *status_dev,
                               void *residual_dev) {
  if (!s || !q_init_dev || !targets_dev || !q_dev || n < 1)
    return fail(TDS_ERR_INVALID_ARG, "tds_hip_inverse_kinematics: NULL or empty argument%s");
  DeviceGuard guard(s->device);
  int cls, rc = tds_jvp_prepare(s, &cls);
  if (rc) return rc;
  TdsIkArgs a = {};
  if ((rc = tds_ik_params(&s->model, k, links, body_points, opt, q_ref_dev ? 1 : 0, &a.o))) return rc;
  const int W = tds_ik_width(s, n);
  long long blocks = ((long long)n + W - 1) / W;
  if (blocks > kIkLanes / W) blocks = kIkLanes / W;
  const long long lanes = blocks * W;
  const size_t need = ((size_t)lanes * tds_ik_layout(&s->model, k).total * sizeof(double) + 255) & ~(size_t)255;
  if ((rc = tds_jvp_tmp(s, need))) return rc;  // shared with the step derivatives and the dynamics queries
  a.m = (const tds_model_t *)s->d_diff_model;
  a.n = n;
  a.q_init = (const double *)q_init_dev, a.targets = (const double *)targets_dev, a.q_ref = (const double *)q_ref_dev;
  a.q = (double *)q_dev, a.residual = (double *)residual_dev;
  a.iterations = (int *)iter_dev, a.status = (int *)status_dev;
  hipLaunchKernelGGL(tds_ik_kernel, dim3((unsigned)blocks), dim3(W), 0, s->stream, a, (double *)s->d_diff_tmp, (int)lanes);
  TDS_HIP_TRY(hipGetLastError());
  return TDS_OK;
}

int tds_hip_inverse_kinematics_host(const tds_model_t *model, int n, const double *q_init, int k, const int32_t *links,
                                    const double *body_points, const double *targets, const double *q_ref,
                                    const tds_ik_options_t *opt, double *q, int32_t *iterations, int32_t *status,
                                    double *residual) {
  if (!model || !q_init || !targets || !q || n < 1)
    return fail(TDS_ERR_INVALID_ARG, "tds_hip_inverse_kinematics_host: NULL or empty argument%s");
  const char *why = "";
  if (tds_jvp_pick(model, &why) < 0) return fail(TDS_ERR_UNSUPPORTED, "%s", why);
  int rc = tds_hip_model_check(model);
  if (rc) return rc;
  TdsIkParams p;
  if ((rc = tds_ik_params(model, k, links, body_points, opt, q_ref ? 1 : 0, &p))) return rc;
  const TdsIkLayout L = tds_ik_layout(model, k);
  std::vector<double> buf(L.total, 0.0);
  const TdsDynMem<double> w = {buf.data(), 1};
  const int nq = model->dof_q;
  for (int e = 0; e < n; ++e) {
    for (int c = 0; c < nq; ++c) buf[L.d.q + c] = q_init[(size_t)e * nq + c];
    for (int c = 0; c < 3 * k; ++c) buf[L.tgt + c] = targets[(size_t)e * 3 * k + c];
    if (q_ref)
      for (int c = 0; c < nq; ++c) buf[L.qref + c] = q_ref[(size_t)e * nq + c];
    int it, st;
    double res;
    tds_ik_solve(model, w, L, p, it, st, res);
    for (int c = 0; c < nq; ++c) q[(size_t)e * nq + c] = buf[L.d.q + c];
    if (iterations) iterations[e] = it;
    if (status) status[e] = st;
    if (residual) residual[e] = res;
  }
  return TDS_OK;
}

}  // extern "C"
