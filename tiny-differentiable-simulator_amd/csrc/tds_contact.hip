// tds_contact.hip — the batched contact query on gfx950 (tds_contact.h over double) and its C ABI: tds_hip_contacts,
// the CPU checker tds_hip_contacts_host and tds_hip_contact_layout (include/tds_hip.h).
//
// Mapping: that of tds_dyn.hip.  One lane per environment, workgroups of W <= 64 lanes (one wavefront, narrowed so
// that a small batch still reaches every compute unit), at most 16 384 lanes per launch and the grid's stride beyond.
// An environment's state (tds_contact_layout: tds_dyn.h's state, the record x, the contact points, their Jacobians,
// J, W = M^-1 J^T, b, p, u and, only where it is asked for, the Delassus matrix) lives in the handle's work buffer
// laid out [component][lane], the lane minor: every access is wave-uniform in its component, so a wave reads or writes
// one run of W doubles.  Nothing indexed at run time is kept in the private segment.
// Records in HBM are [environment][component]; a workgroup brings x in and every output out through an LDS tile of
// 64 lanes x 64 components, so that global loads and stores walk the records in their memory order.
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include <vector>

#include "tds_contact.h"
#include "tds_diff_classes.h"

using namespace tds_internal;

namespace {

constexpr int kTileC = 64;                  // components per LDS tile
constexpr int kTileS = kTileC + 1;          // its row stride in doubles (odd: a lane's row starts on its own bank pair)
constexpr long long kContactLanes = 16384;  // lanes of a launch at most

struct TdsContactArgs {
  const tds_model_t *m;
  int n, what, with_A;
  const double *x;
  double *contacts, *jac, *rows, *rhs, *delassus, *impulse, *force, *qd_pre, *qd_post;
};

// records [e0, e0 + nv)[nc] of `in` -> components off .. off + nc of the workgroup's lanes
__device__ inline void tds_contact_ingest(double *tile, TdsDynMem<double> w, int off, const double *in, int nc, int e0,
                                          int nv) {
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

// components off .. off + nc of the workgroup's lanes -> records [e0, e0 + nv)[nc] of `out`; bad: this lane's
// environment has no valid value (M not positive definite) and its record is NaN
__device__ inline void tds_contact_emit(double *tile, TdsDynMem<double> w, int off, double *out, int nc, int e0, int nv,
                                        int bad) {
  const int W = blockDim.x, t = threadIdx.x;
  for (int c0 = 0; c0 < nc; c0 += kTileC) {
    const int tc = nc - c0 < kTileC ? nc - c0 : kTileC;
    if (t < nv)
      for (int c = 0; c < tc; ++c) tile[t * kTileS + c] = bad ? __builtin_nan("") : w[off + c0 + c];
    __syncthreads();
    for (int idx = t; idx < nv * tc; idx += W) {
      const int e = idx / tc, c = idx - e * tc;
      out[(size_t)(e0 + e) * nc + c0 + c] = tile[e * kTileS + c];
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(64) tds_contact_kernel(TdsContactArgs a, double *buf, int lanes) {
  __shared__ double tile[64 * kTileS];
  const tds_model_t *m = a.m;
  const TdsContactLayout L = tds_contact_layout(m, a.with_A);
  const int W = blockDim.x, t = threadIdx.x, nd = m->dof_qd, nc = L.nc, nr = 3 * nc;
  const TdsDynMem<double> w = {buf + (size_t)blockIdx.x * W + t, (size_t)lanes};
  for (int e0 = blockIdx.x * W; e0 < a.n; e0 += gridDim.x * W) {
    const int nv = a.n - e0 < W ? a.n - e0 : W;
    tds_contact_ingest(tile, w, L.x, a.x, m->input_dim, e0, nv);
    const int bad = t < nv ? tds_contact_eval(m, TdsBlobView{}, w, L, a.what) : 0;
    if (a.contacts && nc) tds_contact_emit(tile, w, L.cp, a.contacts, 10 * nc, e0, nv, 0);
    if (a.jac && nc) tds_contact_emit(tile, w, L.cjac, a.jac, 3 * nd * nc, e0, nv, 0);
    if (a.rows && nc) tds_contact_emit(tile, w, L.J, a.rows, nr * nd, e0, nv, bad);
    if (a.rhs && nc) tds_contact_emit(tile, w, L.b, a.rhs, nr, e0, nv, bad);
    if (a.delassus && nc) tds_contact_emit(tile, w, L.A, a.delassus, nr * nr, e0, nv, bad);
    if (a.impulse && nc) tds_contact_emit(tile, w, L.p, a.impulse, nr, e0, nv, bad);
    if (a.force && nc) tds_contact_emit(tile, w, L.force, a.force, nr, e0, nv, bad);
    if (a.qd_pre) tds_contact_emit(tile, w, L.qd_pre, a.qd_pre, nd, e0, nv, bad);
    if (a.qd_post) tds_contact_emit(tile, w, L.qd_post, a.qd_post, nd, e0, nv, bad);
  }
}

// lanes per workgroup: the rule of the dynamics queries (the widest of 64, 32, 16 that still gives every compute unit
// a workgroup).  TDS_HIP_DYN_WIDTH (16, 32, 64) overrides it, for measurements.
int tds_contact_width(const tds_hip_sim *s, int n) {
  if (const char *e = getenv("TDS_HIP_DYN_WIDTH")) {
    const int v = atoi(e);
    if (v == 16 || v == 32 || v == 64) return v;
  }
  int W = 64;
  while (W > 16 && (n + W - 1) / W < s->num_cus) W /= 2;
  return W;
}

int tds_contact_what(const tds_contact_out_t *o, int nc) {
  int what = (o->qd_pre ? TDS_CT_QD_PRE : 0) | (o->qd_post ? TDS_CT_QD_POST : 0);
  if (nc)
    what |= (o->contacts ? TDS_CT_CONTACTS : 0) | (o->jac ? TDS_CT_JAC : 0) | (o->rows ? TDS_CT_ROWS : 0) |
            (o->rhs ? TDS_CT_RHS : 0) | (o->delassus ? TDS_CT_DELASSUS : 0) | (o->impulse ? TDS_CT_IMPULSE : 0) |
            (o->force ? TDS_CT_FORCE : 0);
  return what;
}

int tds_contact_any(const tds_contact_out_t *o) {
  return o->contacts || o->jac || o->rows || o->rhs || o->delassus || o->impulse || o->force || o->qd_pre || o->qd_post;
}

int tds_contact_host_check(const tds_model_t *model) {
  const char *why = "";
  if (tds_jvp_pick(model, &why) < 0) return fail(TDS_ERR_UNSUPPORTED, "%s", why);
  return tds_hip_model_check(model);
}

}  // namespace

extern "C" {

int tds_hip_contacts(tds_hip_sim_t *s, int n, const void *x_dev, const tds_contact_out_t *out) {
  if (!s || !x_dev || !out || n < 1) return fail(TDS_ERR_INVALID_ARG, "tds_hip_contacts: NULL or empty argument%s");
  if (!tds_contact_any(out)) return fail(TDS_ERR_INVALID_ARG, "tds_hip_contacts: no output requested%s");
  DeviceGuard guard(s->device);
  int cls, rc = tds_jvp_prepare(s, &cls);
  if (rc) return rc;
  const int nc = tds_contact_count(&s->model), what = tds_contact_what(out, nc);
  if (!what) return TDS_OK;  // only outputs without extent (no contact points)
  const int with_A = (what & TDS_CT_DELASSUS) ? 1 : 0;
  const int W = tds_contact_width(s, n);
  long long blocks = ((long long)n + W - 1) / W;
  if (blocks > kContactLanes / W) blocks = kContactLanes / W;
  const long long lanes = blocks * W;
  const size_t need = ((size_t)lanes * tds_contact_layout(&s->model, with_A).total * sizeof(double) + 255) & ~(size_t)255;
  if ((rc = tds_jvp_tmp(s, need))) return rc;  // shared with the step derivatives and the dynamics queries
  TdsContactArgs a = {(const tds_model_t *)s->d_diff_model, n, what, with_A, (const double *)x_dev,
                      (double *)out->contacts, (double *)out->jac, (double *)out->rows, (double *)out->rhs,
                      (double *)out->delassus, (double *)out->impulse, (double *)out->force, (double *)out->qd_pre,
                      (double *)out->qd_post};
  hipLaunchKernelGGL(tds_contact_kernel, dim3((unsigned)blocks), dim3(W), 0, s->stream, a, (double *)s->d_diff_tmp,
                     (int)lanes);
  TDS_HIP_TRY(hipGetLastError());
  return TDS_OK;
}

int tds_hip_contacts_host(const tds_model_t *model, int n, const double *x, const tds_contact_out_t *out) {
  if (!model || !x || !out || n < 1) return fail(TDS_ERR_INVALID_ARG, "tds_hip_contacts_host: NULL or empty argument%s");
  if (!tds_contact_any(out)) return fail(TDS_ERR_INVALID_ARG, "tds_hip_contacts_host: no output requested%s");
  int rc = tds_contact_host_check(model);
  if (rc) return rc;
  const int nc = tds_contact_count(model), what = tds_contact_what(out, nc), nd = model->dof_qd, nr = 3 * nc;
  if (!what) return TDS_OK;
  const TdsContactLayout L = tds_contact_layout(model, (what & TDS_CT_DELASSUS) ? 1 : 0);
  std::vector<double> buf(L.total, 0.0);
  const TdsDynMem<double> w = {buf.data(), 1};
  int any_bad = 0;
  for (int e = 0; e < n; ++e) {
    for (int c = 0; c < model->input_dim; ++c) buf[L.x + c] = x[(size_t)e * model->input_dim + c];
    const int bad = tds_contact_eval(model, TdsBlobView{}, w, L, what);
    any_bad |= bad;
    auto get = [&](int off, void *dst, int width, int nan) {
      if (!dst || !width) return;
      for (int c = 0; c < width; ++c) ((double *)dst)[(size_t)e * width + c] = nan ? __builtin_nan("") : buf[off + c];
    };
    get(L.cp, out->contacts, 10 * nc, 0);
    get(L.cjac, out->jac, 3 * nd * nc, 0);
    get(L.J, out->rows, nr * nd, bad);
    get(L.b, out->rhs, nr, bad);
    get(L.A, out->delassus, nr * nr, bad);
    get(L.p, out->impulse, nr, bad);
    get(L.force, out->force, nr, bad);
    get(L.qd_pre, out->qd_pre, nd, bad);
    get(L.qd_post, out->qd_post, nd, bad);
  }
  return any_bad ? fail(TDS_ERR_INVALID_ARG, "contact query: joint-space inertia not positive definite%s") : TDS_OK;
}

int tds_hip_contact_layout(const tds_model_t *model, int32_t *link, int32_t *geom, double *dirs) {
  if (!model) return -fail(TDS_ERR_INVALID_ARG, "tds_hip_contact_layout: NULL model%s");
  if (const int rc = tds_contact_host_check(model)) return -rc;
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
