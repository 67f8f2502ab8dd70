// tds_contact.hip — the batched contact query on gfx950 (tds_contact.h over double) and its C ABI: tds_hip_contacts,
// the CPU checker tds_hip_contacts_host and tds_hip_contact_layout (include/tds_hip.h).
//
// Mapping: tds_query.h's.  An environment's state is tds_contact_layout's: tds_dyn.h's state, the record x, the contact
// points, their Jacobians, J, W = M^-1 J^T, b, p, u and, only where it is asked for, the Delassus matrix.  A workgroup
// brings x in and every output out through the LDS tile.
#include <hip/hip_runtime.h>

#include "tds_contact.h"
#include "tds_query.h"

namespace {

struct TdsContactArgs {
  const tds_model_t *m;
  int n, what, with_A;
  const double *x;
  double *contacts, *jac, *rows, *rhs, *delassus, *impulse, *force, *qd_pre, *qd_post;
};

__global__ void __launch_bounds__(64) tds_contact_kernel(TdsContactArgs a, double *buf, int lanes) {
  __shared__ double tile[64 * kTileS];
  const tds_model_t *m = a.m;
  const TdsContactLayout L = tds_contact_layout(m, a.with_A);
  const int W = blockDim.x, t = threadIdx.x, nd = m->dof_qd, nc = L.nc, nr = 3 * nc;
  const TdsDynMem<double> w = {buf + (size_t)blockIdx.x * W + t, (size_t)lanes};
  for (int e0 = blockIdx.x * W; e0 < a.n; e0 += gridDim.x * W) {
    const int nv = a.n - e0 < W ? a.n - e0 : W;
    tds_query_ingest(tile, w, L.x, a.x, m->input_dim, e0, nv);
    const int bad = t < nv ? tds_contact_eval(m, TdsBlobView{}, w, L, a.what) : 0;  // M not positive definite
    if (a.contacts && nc) tds_query_emit(tile, w, L.cp, a.contacts, 10 * nc, e0, nv, 0);
    if (a.jac && nc) tds_query_emit(tile, w, L.cjac, a.jac, 3 * nd * nc, e0, nv, 0);
    if (a.rows && nc) tds_query_emit(tile, w, L.J, a.rows, nr * nd, e0, nv, bad);
    if (a.rhs && nc) tds_query_emit(tile, w, L.b, a.rhs, nr, e0, nv, bad);
    if (a.delassus && nc) tds_query_emit(tile, w, L.A, a.delassus, nr * nr, e0, nv, bad);
    if (a.impulse && nc) tds_query_emit(tile, w, L.p, a.impulse, nr, e0, nv, bad);
    if (a.force && nc) tds_query_emit(tile, w, L.force, a.force, nr, e0, nv, bad);
    if (a.qd_pre) tds_query_emit(tile, w, L.qd_pre, a.qd_pre, nd, e0, nv, bad);
    if (a.qd_post) tds_query_emit(tile, w, L.qd_post, a.qd_post, nd, e0, nv, bad);
  }
}

}  // namespace

extern "C" {

int tds_hip_contacts(tds_hip_sim_t *s, int n, const void *x_dev, const tds_contact_out_t *out) {
  if (!s || !x_dev || !out || n < 1) return fail(TDS_ERR_INVALID_ARG, "tds_hip_contacts: NULL or empty argument%s");
  if (!tds_contact_any(out)) return fail(TDS_ERR_INVALID_ARG, "tds_hip_contacts: no output requested%s");
  DeviceGuard guard(s->device);
  int cls, rc = tds_diff_prepare(s, &cls);
  if (rc) return rc;
  const int nc = tds_contact_count(&s->model), what = tds_contact_what(out, nc);
  if (!what) return TDS_OK;  // only outputs without extent (no contact points)
  const int with_A = (what & TDS_CT_DELASSUS) ? 1 : 0;
  TdsQueryPlan p;
  if ((rc = tds_query_plan(s, n, tds_contact_layout(&s->model, with_A).total, &p))) return rc;
  TdsContactArgs a = {(const tds_model_t *)s->d_diff_model, n, what, with_A, (const double *)x_dev,
                      (double *)out->contacts, (double *)out->jac, (double *)out->rows, (double *)out->rhs,
                      (double *)out->delassus, (double *)out->impulse, (double *)out->force, (double *)out->qd_pre,
                      (double *)out->qd_post};
  hipLaunchKernelGGL(tds_contact_kernel, dim3((unsigned)p.blocks), dim3(p.W), 0, s->stream, a, (double *)s->d_diff_tmp,
                     (int)p.lanes);
  TDS_HIP_TRY(hipGetLastError());
  return TDS_OK;
}

int tds_hip_contacts_host(const tds_model_t *model, int n, const double *x, const tds_contact_out_t *out) {
  if (!model || !x || !out || n < 1) return fail(TDS_ERR_INVALID_ARG, "tds_hip_contacts_host: NULL or empty argument%s");
  if (!tds_contact_any(out)) return fail(TDS_ERR_INVALID_ARG, "tds_hip_contacts_host: no output requested%s");
  int cls, rc = tds_diff_host_check(model, &cls);
  if (rc) return rc;
  const int nc = tds_contact_count(model), what = tds_contact_what(out, nc), nd = model->dof_qd, nr = 3 * nc;
  if (!what) return TDS_OK;
  const TdsContactLayout L = tds_contact_layout(model, (what & TDS_CT_DELASSUS) ? 1 : 0);
  TdsQueryHost h(L.total);
  int any_bad = 0;
  for (int e = 0; e < n; ++e) {
    h.put(L.x, x, model->input_dim, e);
    const int bad = tds_contact_eval(model, TdsBlobView{}, h.w, L, what);
    any_bad |= bad;
    h.get(L.cp, out->contacts, 10 * nc, e);
    h.get(L.cjac, out->jac, 3 * nd * nc, e);
    h.get(L.J, out->rows, nr * nd, e, bad);
    h.get(L.b, out->rhs, nr, e, bad);
    h.get(L.A, out->delassus, nr * nr, e, bad);
    h.get(L.p, out->impulse, nr, e, bad);
    h.get(L.force, out->force, nr, e, bad);
    h.get(L.qd_pre, out->qd_pre, nd, e, bad);
    h.get(L.qd_post, out->qd_post, nd, e, bad);
  }
  return any_bad ? fail(TDS_ERR_INVALID_ARG, "contact query: joint-space inertia not positive definite%s") : TDS_OK;
}

int tds_hip_contact_layout(const tds_model_t *model, int32_t *link, int32_t *geom, double *dirs) {
  if (!model) return -fail(TDS_ERR_INVALID_ARG, "tds_hip_contact_layout: NULL model%s");
  int cls;
  if (const int rc = tds_diff_host_check(model, &cls)) return -rc;
  int c = 0;
  if (model->has_plane)
    for (int g = 0; g < model->num_geoms; ++g)
      for (int e = 0; e < tds_contact_points(model->geoms[g].type); ++e, ++c) {
        if (link) link[c] = model->geoms[g].link;
        if (geom) geom[c] = g;
      }
  if (dirs) {
    for (int k = 0; k < 3; ++k) dirs[k] = -model->plane_normal[k];
    tds_d_plane_space(dirs, dirs + 3, dirs + 6);
  }
  return c;
}

}  // extern "C"
