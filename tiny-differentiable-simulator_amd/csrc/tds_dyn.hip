// tds_dyn.hip — batched dynamics queries on gfx950 (tds_dyn.h over double) and their C ABI: tds_hip_dynamics (X_world,
// mass matrix, bias, forward dynamics), tds_hip_inverse_dynamics, tds_hip_point_jacobian and the three _host checkers
// (include/tds_hip.h).
//
// Mapping: tds_query.h's (one lane per environment, the state of tds_dyn_layout in the handle's work buffer laid out
// [component][lane], records through an LDS tile).
#include <hip/hip_runtime.h>

#include "tds_query.h"

namespace {

struct TdsDynArgs {
  const tds_model_t *m;
  int n, what, link, is_local, n_tau;
  const double *q, *qd, *tau, *qdd, *pt;
  double *x_world, *M, *bias, *qdd_out, *jac;
};

__global__ void __launch_bounds__(64) tds_dyn_kernel(TdsDynArgs a, double *buf, int lanes) {
  __shared__ double tile[64 * kTileS];
  const tds_model_t *m = a.m;
  const TdsDynLayout L = tds_dyn_layout(m);
  const int W = blockDim.x, t = threadIdx.x, nq = m->dof_q, nd = m->dof_qd, nl = m->num_links;
  const TdsDynMem<double> w = {buf + (size_t)blockIdx.x * W + t, (size_t)lanes};
  for (int e0 = blockIdx.x * W; e0 < a.n; e0 += gridDim.x * W) {
    const int nv = a.n - e0 < W ? a.n - e0 : W;
    // (<true>: an input that is NULL stands for zeros)
    tds_query_ingest<true>(tile, w, L.q, a.q, nq, e0, nv);
    tds_query_ingest<true>(tile, w, L.qd, a.qd, nd, e0, nv);
    if (a.what & TDS_DYN_QDD) {  // the torques of the actuated dofs behind the base's six zeros
      tds_query_ingest<true>(tile, w, L.tau, nullptr, nd - a.n_tau, e0, nv);
      tds_query_ingest<true>(tile, w, L.tau + nd - a.n_tau, a.tau, a.n_tau, e0, nv);
    }
    if (a.what & TDS_DYN_ID) tds_query_ingest<true>(tile, w, L.qdd, a.qdd, nd, e0, nv);
    if (a.what & TDS_DYN_JAC) tds_query_ingest<true>(tile, w, L.pt, a.pt, 3, e0, nv);
    if (t < nv && tds_dyn_eval(m, TdsBlobView{}, w, L, a.what, a.link, a.is_local))
      for (int d = 0; d < nd; ++d) w[L.qdd + d] = __builtin_nan("");  // M not positive definite
    if (a.x_world) tds_query_emit(tile, w, L.xw, a.x_world, 12 * nl, e0, nv, 0);
    if (a.M) tds_query_emit(tile, w, L.M, a.M, nd * nd, e0, nv, 0);
    if (a.bias) tds_query_emit(tile, w, L.bias, a.bias, nd, e0, nv, 0);
    if (a.qdd_out) tds_query_emit(tile, w, L.qdd, a.qdd_out, nd, e0, nv, 0);
    if (a.jac) tds_query_emit(tile, w, L.jac, a.jac, 3 * nd, e0, nv, 0);
  }
}

int tds_dyn_launch(tds_hip_sim *s, TdsDynArgs a) {
  TdsQueryPlan p;
  const int rc = tds_query_plan(s, a.n, tds_dyn_layout(&s->model).total, &p);
  if (rc) return rc;
  a.m = (const tds_model_t *)s->d_diff_model;
  a.n_tau = s->model.dof_qd - (s->model.is_floating ? 6 : 0);
  hipLaunchKernelGGL(tds_dyn_kernel, dim3((unsigned)p.blocks), dim3(p.W), 0, s->stream, a, (double *)s->d_diff_tmp,
                     (int)p.lanes);
  TDS_HIP_TRY(hipGetLastError());
  return TDS_OK;
}

const char kNoFloatingId[] =
    "dynamics queries: bias and inverse dynamics need a fixed base (the reference has no floating-base inverse dynamics)%s";

int tds_dyn_link_check(const tds_model_t *m, int link) {
  if (link < -1 || link >= m->num_links) return fail(TDS_ERR_INVALID_ARG, "dynamics queries: link index out of range%s");
  return TDS_OK;
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
  int cls, rc = tds_diff_prepare(s, &cls);
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
  int cls, rc = tds_diff_prepare(s, &cls);
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
  int cls, rc = tds_diff_prepare(s, &cls);
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
  int cls, rc = tds_diff_host_check(model, &cls);
  if (rc) return rc;
  if (out->bias && model->is_floating) return fail(TDS_ERR_UNSUPPORTED, kNoFloatingId);
  const TdsDynLayout L = tds_dyn_layout(model);
  TdsQueryHost h(L.total);
  const int nd = model->dof_qd, n_tau = nd - (model->is_floating ? 6 : 0);
  int bad = 0;
  for (int e = 0; e < n; ++e) {
    h.put(L.q, q, model->dof_q, e);
    h.put(L.qd, qd, nd, e);
    h.put(L.tau, nullptr, nd - n_tau, 0);
    h.put(L.tau + nd - n_tau, tau, n_tau, e);
    const int nan = tds_dyn_eval(model, TdsBlobView{}, h.w, L, what, 0, 0);  // M not positive definite
    bad |= nan;
    h.get(L.xw, out->x_world, 12 * model->num_links, e);
    h.get(L.M, out->mass_matrix, nd * nd, e);
    h.get(L.bias, out->bias, nd, e);
    h.get(L.qdd, out->qdd, nd, e, nan);
  }
  return bad ? fail(TDS_ERR_INVALID_ARG, "dynamics queries: joint-space inertia not positive definite%s") : TDS_OK;
}

int tds_hip_inverse_dynamics_host(const tds_model_t *model, int n, const double *q, const double *qd, const double *qdd,
                                  double *tau) {
  if (!model || !q || !tau || n < 1) return fail(TDS_ERR_INVALID_ARG, "tds_hip_inverse_dynamics_host: NULL or empty argument%s");
  int cls, rc = tds_diff_host_check(model, &cls);
  if (rc) return rc;
  if (model->is_floating) return fail(TDS_ERR_UNSUPPORTED, kNoFloatingId);
  const TdsDynLayout L = tds_dyn_layout(model);
  TdsQueryHost h(L.total);
  for (int e = 0; e < n; ++e) {
    h.put(L.q, q, model->dof_q, e);
    h.put(L.qd, qd, model->dof_qd, e);
    h.put(L.qdd, qdd, model->dof_qd, e);
    tds_dyn_eval(model, TdsBlobView{}, h.w, L, TDS_DYN_ID, 0, 0);
    h.get(L.bias, tau, model->dof_qd, e);
  }
  return TDS_OK;
}

int tds_hip_point_jacobian_host(const tds_model_t *model, int n, const double *q, int link, const double *point,
                                int is_local, double *jac) {
  if (!model || !q || !point || !jac || n < 1)
    return fail(TDS_ERR_INVALID_ARG, "tds_hip_point_jacobian_host: NULL or empty argument%s");
  int cls, rc = tds_diff_host_check(model, &cls);
  if (rc) return rc;
  if ((rc = tds_dyn_link_check(model, link))) return rc;
  const TdsDynLayout L = tds_dyn_layout(model);
  TdsQueryHost h(L.total);
  for (int e = 0; e < n; ++e) {
    h.put(L.q, q, model->dof_q, e);
    h.put(L.pt, point, 3, e);
    tds_dyn_eval(model, TdsBlobView{}, h.w, L, TDS_DYN_JAC, link, is_local ? 1 : 0);
    h.get(L.jac, jac, 3 * model->dof_qd, e);
  }
  return TDS_OK;
}

}  // extern "C"
