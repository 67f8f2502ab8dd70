// tds_dyn.hip — batched dynamics queries on gfx950 (tds_dyn.h over double) and their C ABI: tds_hip_dynamics (X_world,
// mass matrix, bias, forward dynamics), tds_hip_inverse_dynamics, tds_hip_point_jacobian and the three _host checkers
// (include/tds_hip.h).
//
// Mapping: one lane per environment, workgroups of W <= 64 lanes (one wavefront, narrowed so that a small batch still
// reaches every compute unit: tds_dyn_width).  An environment's state (tds_dyn_layout: transforms, velocities,
// accelerations, forces, inertias, M, its factor — 17 KB at 22 links) lives in the handle's work buffer laid out
// [component][lane], the lane minor: every access of the recursions is wave-uniform in its component, so a wave reads
// or writes one run of W doubles.  Nothing indexed at run time is kept in the private segment.
// Records in HBM are [environment][component].  A workgroup brings them in and out through an LDS tile of 64 lanes x 64
// components (tds_dyn_ingest / tds_dyn_emit): global loads and stores walk the records in their memory order, so that a
// wave's stores are contiguous runs (512 B of each Ant's M [14][14] at a time; a whole [64][components] block where
// a record has at most 64 components), never a stride of dof_qd^2 doubles per lane.
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <vector>

#include "tds_diff_classes.h"
#include "tds_dyn.h"

using namespace tds_internal;

namespace {

constexpr int kTileC = 64;             // components per LDS tile
constexpr int kTileS = kTileC + 1;     // its row stride in doubles (odd: a lane's row starts on its own bank pair)
constexpr long long kDynLanes = 16384;  // lanes of a launch at most (the work buffer: 16384 states, 280 MB at 22 links)

struct TdsDynArgs {
  const tds_model_t *m;
  int n, what, link, is_local, n_tau;
  const double *q, *qd, *tau, *qdd, *pt;
  double *x_world, *M, *bias, *qdd_out, *jac;
};

// records [e0, e0 + nv)[nc] of `in` -> components off .. off + nc of the workgroup's lanes (in NULL: zeros)
__device__ inline void tds_dyn_ingest(double *tile, TdsDynMem<double> w, int off, const double *in, int nc, int e0, int nv) {
  const int W = blockDim.x, t = threadIdx.x;
  if (!in) {
    if (t < nv)
      for (int c = 0; c < nc; ++c) w[off + c] = 0.0;
    return;
  }
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
__device__ inline void tds_dyn_emit(double *tile, TdsDynMem<double> w, int off, double *out, int nc, int e0, int nv) {
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

__global__ void __launch_bounds__(64) tds_dyn_kernel(TdsDynArgs a, double *buf, int lanes) {
  __shared__ double tile[64 * kTileS];
  const tds_model_t *m = a.m;
  const TdsDynLayout L = tds_dyn_layout(m);
  const int W = blockDim.x, t = threadIdx.x, nq = m->dof_q, nd = m->dof_qd, nl = m->num_links;
  const TdsDynMem<double> w = {buf + (size_t)blockIdx.x * W + t, (size_t)lanes};
  for (int e0 = blockIdx.x * W; e0 < a.n; e0 += gridDim.x * W) {
    const int nv = a.n - e0 < W ? a.n - e0 : W;
    tds_dyn_ingest(tile, w, L.q, a.q, nq, e0, nv);
    tds_dyn_ingest(tile, w, L.qd, a.qd, nd, e0, nv);
    if (a.what & TDS_DYN_QDD) {  // the torques of the actuated dofs behind the base's six zeros
      tds_dyn_ingest(tile, w, L.tau, nullptr, nd - a.n_tau, e0, nv);
      tds_dyn_ingest(tile, w, L.tau + nd - a.n_tau, a.tau, a.n_tau, e0, nv);
    }
    if (a.what & TDS_DYN_ID) tds_dyn_ingest(tile, w, L.qdd, a.qdd, nd, e0, nv);
    if (a.what & TDS_DYN_JAC) tds_dyn_ingest(tile, w, L.pt, a.pt, 3, e0, nv);
    if (t < nv && tds_dyn_eval(m, TdsBlobView{}, w, L, a.what, a.link, a.is_local))
      for (int d = 0; d < nd; ++d) w[L.qdd + d] = __builtin_nan("");  // M not positive definite
    if (a.x_world) tds_dyn_emit(tile, w, L.xw, a.x_world, 12 * nl, e0, nv);
    if (a.M) tds_dyn_emit(tile, w, L.M, a.M, nd * nd, e0, nv);
    if (a.bias) tds_dyn_emit(tile, w, L.bias, a.bias, nd, e0, nv);
    if (a.qdd_out) tds_dyn_emit(tile, w, L.qdd, a.qdd_out, nd, e0, nv);
    if (a.jac) tds_dyn_emit(tile, w, L.jac, a.jac, 3 * nd, e0, nv);
  }
}

// lanes per workgroup: the widest of 64, 32, 16 that still gives every compute unit a workgroup (a lane's recursions
// are one long dependent chain: a batch of 4096 on 64 of 256 compute units takes as long as one four times its size).
// TDS_HIP_DYN_WIDTH (16, 32, 64) overrides the rule, for measurements.
int tds_dyn_width(const tds_hip_sim *s, int n) {
  if (const char *e = getenv("TDS_HIP_DYN_WIDTH")) {
    const int v = atoi(e);
    if (v == 16 || v == 32 || v == 64) return v;
  }
  int W = 64;
  while (W > 16 && (n + W - 1) / W < s->num_cus) W /= 2;
  return W;
}

int tds_dyn_launch(tds_hip_sim *s, TdsDynArgs a) {
  const int W = tds_dyn_width(s, a.n);
  long long blocks = ((long long)a.n + W - 1) / W;
  if (blocks > kDynLanes / W) blocks = kDynLanes / W;
  const long long lanes = blocks * W;
  const size_t need = ((size_t)lanes * tds_dyn_layout(&s->model).total * sizeof(double) + 255) & ~(size_t)255;
  const int rc = tds_jvp_tmp(s, need);  // shared with the step derivatives: calls on the stream use it in turn
  if (rc) return rc;
  a.m = (const tds_model_t *)s->d_diff_model;
  a.n_tau = s->model.dof_qd - (s->model.is_floating ? 6 : 0);
  hipLaunchKernelGGL(tds_dyn_kernel, dim3((unsigned)blocks), dim3(W), 0, s->stream, a, (double *)s->d_diff_tmp, (int)lanes);
  TDS_HIP_TRY(hipGetLastError());
  return TDS_OK;
}

const char kNoFloatingId[] =
    "dynamics queries: bias and inverse dynamics need a fixed base (the reference has no floating-base inverse dynamics)%s";

int tds_dyn_link_check(const tds_model_t *m, int link) {
  if (link < -1 || link >= m->num_links) return fail(TDS_ERR_INVALID_ARG, "dynamics queries: link index out of range%s");
  return TDS_OK;
}

// the host instantiation: one environment at a time in a vector of its own (stride 1)
struct TdsDynHost {
  const tds_model_t *m;
  TdsDynLayout L;
  std::vector<double> buf;
  TdsDynMem<double> w;
  explicit TdsDynHost(const tds_model_t *model) : m(model), L(tds_dyn_layout(model)), buf(L.total, 0.0), w{buf.data(), 1} {}
  void put(int off, const double *src, int nc, int e) {
    for (int c = 0; c < nc; ++c) buf[off + c] = src ? src[(size_t)e * nc + c] : 0.0;
  }
  void get(int off, double *dst, int nc, int e) const {
    if (dst)
      for (int c = 0; c < nc; ++c) dst[(size_t)e * nc + c] = buf[off + c];
  }
};

int tds_dyn_host_check(const tds_model_t *model) {
  const char *why = "";
  if (tds_jvp_pick(model, &why) < 0) return fail(TDS_ERR_UNSUPPORTED, "%s", why);
  return tds_hip_model_check(model);
}

}  // namespace

extern "C" {

int tds_hip_dynamics(tds_hip_sim_t *s, int n, const void *q_dev, const void *qd_dev, const void *tau_dev,
                     const tds_dyn_out_t *out) {
  if (!s || !q_dev || !out || n < 1) return fail(TDS_ERR_INVALID_ARG, "tds_hip_dynamics: NULL or empty argument%s");
  const int what = (out->x_world ? TDS_DYN_XW : 0) | (out->mass_matrix ? TDS_DYN_M : 0) | (out->bias ? TDS_DYN_BIAS : 0) |
                   (out->qdd ? TDS_DYN_QDD : 0);
  if (!what) return fail(TDS_ERR_INVALID_ARG, "tds_hip_dynamics: no output requested%s");
  DeviceGuard guard(s->device);
  int cls, rc = tds_jvp_prepare(s, &cls);
  if (rc) return rc;
  if (out->bias && s->model.is_floating) return fail(TDS_ERR_UNSUPPORTED, kNoFloatingId);
  TdsDynArgs a = {nullptr, n, what, 0, 0, 0, (const double *)q_dev, (const double *)qd_dev, (const double *)tau_dev,
                  nullptr, nullptr, (double *)out->x_world, (double *)out->mass_matrix, (double *)out->bias,
                  (double *)out->qdd, nullptr};
  return tds_dyn_launch(s, a);
}

int tds_hip_inverse_dynamics(tds_hip_sim_t *s, int n, const void *q_dev, const void *qd_dev, const void *qdd_dev,
                             void *tau_dev) {
  if (!s || !q_dev || !tau_dev || n < 1) return fail(TDS_ERR_INVALID_ARG, "tds_hip_inverse_dynamics: NULL or empty argument%s");
  DeviceGuard guard(s->device);
  int cls, rc = tds_jvp_prepare(s, &cls);
  if (rc) return rc;
  if (s->model.is_floating) return fail(TDS_ERR_UNSUPPORTED, kNoFloatingId);
  TdsDynArgs a = {nullptr, n, TDS_DYN_ID, 0, 0, 0, (const double *)q_dev, (const double *)qd_dev, nullptr,
                  (const double *)qdd_dev, nullptr, nullptr, nullptr, (double *)tau_dev, nullptr, nullptr};
  return tds_dyn_launch(s, a);
}

int tds_hip_point_jacobian(tds_hip_sim_t *s, int n, const void *q_dev, int link, const void *point_dev, int is_local,
                           void *jac_dev) {
  if (!s || !q_dev || !point_dev || !jac_dev || n < 1)
    return fail(TDS_ERR_INVALID_ARG, "tds_hip_point_jacobian: NULL or empty argument%s");
  DeviceGuard guard(s->device);
  int cls, rc = tds_jvp_prepare(s, &cls);
  if (rc) return rc;
  if ((rc = tds_dyn_link_check(&s->model, link))) return rc;
  TdsDynArgs a = {nullptr, n, TDS_DYN_JAC, link, is_local ? 1 : 0, 0, (const double *)q_dev, nullptr, nullptr, nullptr,
                  (const double *)point_dev, nullptr, nullptr, nullptr, nullptr, (double *)jac_dev};
  return tds_dyn_launch(s, a);
}

int tds_hip_dynamics_host(const tds_model_t *model, int n, const double *q, const double *qd, const double *tau,
                          const tds_dyn_out_t *out) {
  if (!model || !q || !out || n < 1) return fail(TDS_ERR_INVALID_ARG, "tds_hip_dynamics_host: NULL or empty argument%s");
  const int what = (out->x_world ? TDS_DYN_XW : 0) | (out->mass_matrix ? TDS_DYN_M : 0) | (out->bias ? TDS_DYN_BIAS : 0) |
                   (out->qdd ? TDS_DYN_QDD : 0);
  if (!what) return fail(TDS_ERR_INVALID_ARG, "tds_hip_dynamics_host: no output requested%s");
  int rc = tds_dyn_host_check(model);
  if (rc) return rc;
  if (out->bias && model->is_floating) return fail(TDS_ERR_UNSUPPORTED, kNoFloatingId);
  TdsDynHost h(model);
  const int nd = model->dof_qd, n_tau = nd - (model->is_floating ? 6 : 0);
  int bad = 0;
  for (int e = 0; e < n; ++e) {
    h.put(h.L.q, q, model->dof_q, e);
    h.put(h.L.qd, qd, nd, e);
    h.put(h.L.tau, nullptr, nd - n_tau, 0);
    h.put(h.L.tau + nd - n_tau, tau, n_tau, e);
    if (tds_dyn_eval(model, TdsBlobView{}, h.w, h.L, what, 0, 0)) {
      bad = 1;
      for (int d = 0; d < nd; ++d) h.buf[h.L.qdd + d] = __builtin_nan("");
    }
    h.get(h.L.xw, (double *)out->x_world, 12 * model->num_links, e);
    h.get(h.L.M, (double *)out->mass_matrix, nd * nd, e);
    h.get(h.L.bias, (double *)out->bias, nd, e);
    h.get(h.L.qdd, (double *)out->qdd, nd, e);
  }
  return bad ? fail(TDS_ERR_INVALID_ARG, "dynamics queries: joint-space inertia not positive definite%s") : TDS_OK;
}

int tds_hip_inverse_dynamics_host(const tds_model_t *model, int n, const double *q, const double *qd, const double *qdd,
                                  double *tau) {
  if (!model || !q || !tau || n < 1) return fail(TDS_ERR_INVALID_ARG, "tds_hip_inverse_dynamics_host: NULL or empty argument%s");
  int rc = tds_dyn_host_check(model);
  if (rc) return rc;
  if (model->is_floating) return fail(TDS_ERR_UNSUPPORTED, kNoFloatingId);
  TdsDynHost h(model);
  for (int e = 0; e < n; ++e) {
    h.put(h.L.q, q, model->dof_q, e);
    h.put(h.L.qd, qd, model->dof_qd, e);
    h.put(h.L.qdd, qdd, model->dof_qd, e);
    tds_dyn_eval(model, TdsBlobView{}, h.w, h.L, TDS_DYN_ID, 0, 0);
    h.get(h.L.bias, tau, model->dof_qd, e);
  }
  return TDS_OK;
}

int tds_hip_point_jacobian_host(const tds_model_t *model, int n, const double *q, int link, const double *point,
                                int is_local, double *jac) {
  if (!model || !q || !point || !jac || n < 1)
    return fail(TDS_ERR_INVALID_ARG, "tds_hip_point_jacobian_host: NULL or empty argument%s");
  int rc = tds_dyn_host_check(model);
  if (rc) return rc;
  if ((rc = tds_dyn_link_check(model, link))) return rc;
  TdsDynHost h(model);
  for (int e = 0; e < n; ++e) {
    h.put(h.L.q, q, model->dof_q, e);
    h.put(h.L.pt, point, 3, e);
    tds_dyn_eval(model, TdsBlobView{}, h.w, h.L, TDS_DYN_JAC, link, is_local ? 1 : 0);
    h.get(h.L.jac, jac, 3 * model->dof_qd, e);
  }
  return TDS_OK;
}

}  // extern "C"
