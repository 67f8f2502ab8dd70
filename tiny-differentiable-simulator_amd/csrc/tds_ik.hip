// tds_ik.hip — batched inverse kinematics on gfx950 (tds_ik.h over double) and its C ABI: tds_hip_inverse_kinematics,
// tds_hip_inverse_kinematics_host (the checker) and tds_hip_ik_default_options (include/tds_hip.h).
//
// Mapping: tds_query.h's, over the state of tds_ik_layout.  The whole iteration runs inside the one launch: a lane whose
// environment has stopped leaves the loop and waits at its end for the last lane of its wave (the workgroup's barriers
// are all in the record transfers, outside the loop).
#include <hip/hip_runtime.h>

#include "tds_ik.h"
#include "tds_query.h"

namespace {

struct TdsIkArgs {
  const tds_model_t *m;
  int n;
  TdsIkParams o;
  const double *q_init, *targets, *q_ref;
  double *q, *residual;
  int *iterations, *status;
};

__global__ void __launch_bounds__(64) tds_ik_kernel(TdsIkArgs a, double *buf, int lanes) {
  __shared__ double tile[64 * kTileS];
  const tds_model_t *m = a.m;
  const TdsIkLayout L = tds_ik_layout(m, a.o.k);
  const int W = blockDim.x, t = threadIdx.x, nq = m->dof_q;
  const TdsDynMem<double> w = {buf + (size_t)blockIdx.x * W + t, (size_t)lanes};
  for (int e0 = blockIdx.x * W; e0 < a.n; e0 += gridDim.x * W) {
    const int nv = a.n - e0 < W ? a.n - e0 : W;
    tds_query_ingest(tile, w, L.d.q, a.q_init, nq, e0, nv);
    tds_query_ingest(tile, w, L.tgt, a.targets, 3 * a.o.k, e0, nv);
    if (a.o.have_ref) tds_query_ingest(tile, w, L.qref, a.q_ref, nq, e0, nv);
    int iterations = 0, status = TDS_IK_FAILED;
    double residual = -1.0;
    if (t < nv) {
      tds_ik_solve(m, w, L, a.o, iterations, status, residual);
      w[L.e] = residual;
    }
    tds_query_emit(tile, w, L.d.q, a.q, nq, e0, nv, 0);
    if (a.residual) tds_query_emit(tile, w, L.e, a.residual, 1, e0, nv, 0);
    if (t < nv) {  // 4 B per lane, contiguous
      if (a.iterations) a.iterations[e0 + t] = iterations;
      if (a.status) a.status[e0 + t] = status;
    }
  }
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
  int cls, rc = tds_diff_prepare(s, &cls);
  if (rc) return rc;
  TdsIkArgs a = {};
  if ((rc = tds_ik_params(&s->model, k, links, body_points, opt, q_ref_dev ? 1 : 0, &a.o))) return rc;
  TdsQueryPlan p;
  if ((rc = tds_query_plan(s, n, tds_ik_layout(&s->model, k).total, &p))) return rc;
  a.m = (const tds_model_t *)s->d_diff_model;
  a.n = n;
  a.q_init = (const double *)q_init_dev, a.targets = (const double *)targets_dev, a.q_ref = (const double *)q_ref_dev;
  a.q = (double *)q_dev, a.residual = (double *)residual_dev;
  a.iterations = (int *)iter_dev, a.status = (int *)status_dev;
  hipLaunchKernelGGL(tds_ik_kernel, dim3((unsigned)p.blocks), dim3(p.W), 0, s->stream, a, (double *)s->d_diff_tmp,
                     (int)p.lanes);
  TDS_HIP_TRY(hipGetLastError());
  return TDS_OK;
}

int tds_hip_inverse_kinematics_host(const tds_model_t *model, int n, const double *q_init, int k, const int32_t *links,
                                    const double *body_points, const double *targets, const double *q_ref,
                                    const tds_ik_options_t *opt, double *q, int32_t *iterations, int32_t *status,
                                    double *residual) {
  if (!model || !q_init || !targets || !q || n < 1)
    return fail(TDS_ERR_INVALID_ARG, "tds_hip_inverse_kinematics_host: NULL or empty argument%s");
  int cls, rc = tds_diff_host_check(model, &cls);
  if (rc) return rc;
  TdsIkParams p;
  if ((rc = tds_ik_params(model, k, links, body_points, opt, q_ref ? 1 : 0, &p))) return rc;
  const TdsIkLayout L = tds_ik_layout(model, k);
  TdsQueryHost h(L.total);
  const int nq = model->dof_q;
  for (int e = 0; e < n; ++e) {
    h.put(L.d.q, q_init, nq, e);
    h.put(L.tgt, targets, 3 * k, e);
    if (q_ref) h.put(L.qref, q_ref, nq, e);
    int it, st;
    double res;
    tds_ik_solve(model, h.w, L, p, it, st, res);
    h.get(L.d.q, q, nq, e);
    if (iterations) iterations[e] = it;
    if (status) status[e] = st;
    if (residual) residual[e] = res;
  }
  return TDS_OK;
}

}  // extern "C"
