// tds_dyn_jvp.hip — forward-mode derivatives of the batched dynamics queries on gfx950 (tds_dyn.h over TdsDual<K> and an
// overlay of parameters) and their C ABI: tds_hip_dynamics_jvp, tds_hip_inverse_dynamics_jvp, their _host checkers and
// tds_hip_dynamics_jvp_tangents (include/tds_hip.h).
//
// The input of a call is z = [q (dof_q) | qd (dof_qd) | u | theta (p)]: u is tau (the actuated dofs) for the dynamics
// call and qdd (dof_qd) for inverse dynamics.  Directions are v [n][k][z], tangents [n][k][...the output's shape...].
//
// The mapping, the launch, the host checkers' loop and the entry points' bodies are tds_query_dual.h's.  This unit
// states what is the dynamics queries' own: how q | qd | pad | u and their columns of v reach tds_dyn_layout's state (an
// input that is NULL stands for zeros), tds_dyn_eval, the table of its four outputs, of which qdd is NaN where M is not
// positive definite, and the refusal of a floating base's bias; once in its kernel, once for the host (TdsDynJvpUnit).
#include <hip/hip_runtime.h>

#include "tds_query_dual.h"

namespace {

enum { kDynXw = 0, kDynM = 1, kDynBias = 2, kDynQdd = 3, kDynOuts = 4 };

struct TdsDynJvpArgs {
  const tds_model_t *m;
  int n, kdirs, p, what;
  int nu, uoff;  // u's entries and the component of the state where they start (L.tau behind the base's six, or L.qdd)
  const double *q, *qd, *u, *theta, *v;
  const tds_param_t *params;
  double *o[kDynOuts], *d[kDynOuts];  // primal outputs; tangents [n][kdirs][shape]  (bias: ID's torques with TDS_DYN_ID)
  // the columns of v before theta and in all
  struct Columns {
    int before, nall;
    TDS_HD int nx() const { return before; }
  };
  TDS_HD Columns columns() const {
    const int nx = m->dof_q + m->dof_qd + nu;
    return {nx, nx + p};
  }
};

// the outputs' components and extents, in the order of TdsDynJvpArgs::o
struct TdsDynJvpOuts {
  int off[kDynOuts], cnt[kDynOuts];
};
TDS_HD inline TdsDynJvpOuts tds_dyn_jvp_outs(const tds_model_t *m, const TdsDynLayout &L) {
  const int nd = m->dof_qd;
  return {{L.xw, L.M, L.bias, L.qdd}, {12 * m->num_links, nd * nd, nd, nd}};
}

template <class B, int K>
__global__ void __launch_bounds__(64) tds_dyn_jvp_kernel(TdsDynJvpArgs a, double *buf,
                                                         TdsParamOverlay<typename TdsContactScalar<K>::type, B> *ovl,
                                                         int lanes) {
  using T = typename TdsQueryScalar<K>::type;
  __shared__ double tile[64 * kTileS];
  const tds_model_t *m = a.m;
  const TdsDynLayout L = tds_dyn_layout(m);
  const TdsDynJvpOuts O = tds_dyn_jvp_outs(m, L);
  const int W = blockDim.x, t = threadIdx.x, nq = m->dof_q, nd = m->dof_qd, nz = nq + nd + a.nu + a.p;
  const int have_u = a.what & (TDS_DYN_QDD | TDS_DYN_ID), upad = (a.what & TDS_DYN_QDD) ? nd - a.nu : 0;
  const TdsQueryJvpLane<K> ln(buf, lanes, W, t);
  const TdsDynMem<T> w = {(T *)buf + ln.lane, (size_t)lanes};
  TdsParamOverlay<T, B> &P = ovl[ln.lane];
  const int chunks = (a.n + W - 1) / W, blocks = a.kdirs > 0 ? (a.kdirs + K - 1) / (K ? K : 1) : 1;
  const long long groups = (long long)chunks * blocks;
  tds_param_seed(m, P);  // the blob's values, all constant: once per lane
  for (long long g = blockIdx.x; g < groups; g += gridDim.x) {
    const int e0 = (int)(g % chunks) * W, d0 = (int)(g / chunks) * K;  // neighbouring workgroups: neighbouring environments
    const int nv = a.n - e0 < W ? a.n - e0 : W, nk = a.kdirs - d0 < K ? a.kdirs - d0 : K;
    // (<true>: an input that is NULL stands for zeros; the base's six torques, upad, are zeros)
    tds_query_ingest<true>(tile, ln.plane(0), L.q, a.q, nq, e0, nv);
    tds_query_ingest<true>(tile, ln.plane(0), L.qd, a.qd, nd, e0, nv);
    if (have_u) {
      tds_query_ingest<true>(tile, ln.plane(0), a.uoff - upad, nullptr, upad, e0, nv);
      tds_query_ingest<true>(tile, ln.plane(0), a.uoff, a.u, a.nu, e0, nv);
    }
    for (int k = 0; k < K; ++k) {
      // direction d0 + k's columns of v, in z's order; directions past kdirs in the last block: zero
      const double *vk = k < nk ? a.v + (size_t)(d0 + k) * nz : nullptr;
      const size_t vs = (size_t)a.kdirs * nz;
      const auto seed = [&](int off, int col, int cnt) {
        if (vk)
          tds_query_ingest_strided(tile, ln.plane(1 + k), off, vk + col, cnt, vs, e0, nv);
        else
          tds_query_ingest<true>(tile, ln.plane(1 + k), off, nullptr, cnt, e0, nv);
      };
      seed(L.q, 0, nq);
      seed(L.qd, nq, nd);
      if (have_u) {
        tds_query_ingest<true>(tile, ln.plane(1 + k), a.uoff - upad, nullptr, upad, e0, nv);
        seed(a.uoff, nq + nd, a.nu);
      }
    }
    int bad = 0;
    if (t < nv) {
      tds_query_jvp_theta(a, P, e0 + t, d0, nk);
      bad = tds_dyn_eval(m, TdsOverlayView<T, B>{&P}, w, L, a.what, 0, 0);  // M not positive definite
    }
    // each output: the primal by the first block's items, then this block's tangents [n][kdirs][cnt]; qdd of an
    // environment whose M is not positive definite is NaN, and so are its tangents
    for (int i = 0; i < kDynOuts; ++i) {
      const int off = O.off[i], cnt = O.cnt[i], nan = i == kDynQdd ? bad : 0;
      if (a.o[i] && d0 == 0) tds_query_emit(tile, ln.plane(0), off, a.o[i], cnt, e0, nv, nan);
      if (a.d[i])
        for (int k = 0; k < nk; ++k)
          tds_query_emit_strided(tile, ln.plane(1 + k), off, a.d[i] + (size_t)(d0 + k) * cnt, cnt, (size_t)a.kdirs * cnt, e0,
                                 nv, nan);
    }
  }
}

// the unit as tds_query_dual.h's host side sees it
struct TdsDynJvpUnit {
  using Args = TdsDynJvpArgs;
  // tangents per work item of a class on the device (the resource table; to be specialised per class)
  template <class B>
  static constexpr int kTangents = 2;
  template <class B, int K>
  static constexpr auto kKernel = tds_dyn_jvp_kernel<B, K>;
  static constexpr const char *kNotPd = "dynamics queries: joint-space inertia not positive definite%s";

  const Args &a;
  const TdsDynLayout L;
  explicit TdsDynJvpUnit(const Args &a) : a(a), L(tds_dyn_layout(a.m)) {}
  int total() const { return L.total; }
  template <class Put>
  void inputs(const Put &put) const {
    const int nq = a.m->dof_q, nd = a.m->dof_qd;
    put(L.q, a.q, 0, nq);
    put(L.qd, a.qd, nq, nd);
    if (a.what & TDS_DYN_QDD) put(L.tau, nullptr, -1, nd - a.nu);  // the base's six torques
    if (a.what & (TDS_DYN_QDD | TDS_DYN_ID)) put(a.uoff, a.u, nq + nd, a.nu);
  }
  template <typename T, class B>
  int eval(TdsOverlayView<T, B> P, TdsDynMem<T> w) const {
    return tds_dyn_eval(a.m, P, w, L, a.what, 0, 0);
  }
  template <class Get>
  void outputs(const Get &get, int bad) const {
    const TdsDynJvpOuts O = tds_dyn_jvp_outs(a.m, L);
    for (int i = 0; i < kDynOuts; ++i) get(a.o[i], a.d[i], O.off[i], O.cnt[i], i == kDynQdd ? bad : 0);
  }
};

// (the primal queries' message, tds_dyn.hip)
const char kNoFloatingId[] =
    "dynamics queries: bias and inverse dynamics need a fixed base (the reference has no floating-base inverse dynamics)%s";

// the arguments of an entry point, checked, as the kernel's and the host loop's.  id: the inverse-dynamics call (u is
// qdd, the torques are out->bias / dout->bias)
int tds_dyn_jvp_args(const char *who, const tds_model_t *model, int id, int n, const void *q, const void *qd, const void *u,
                     int p, const tds_param_t *params, const void *theta, int k, const void *v, const tds_dyn_out_t *out,
                     const tds_dyn_out_t *dout, TdsDynJvpArgs *a) {
  const auto what_of = [](const tds_dyn_out_t *o) {
    return (o->x_world ? TDS_DYN_XW : 0) | (o->mass_matrix ? TDS_DYN_M : 0) | (o->bias ? TDS_DYN_BIAS : 0) |
           (o->qdd ? TDS_DYN_QDD : 0);
  };
  if (const int rc = tds_query_jvp_check(who, n, q, p, params, k, v, out, dout, what_of)) return rc;
  const int what = what_of(out) | what_of(dout);
  if ((what & TDS_DYN_BIAS) && model->is_floating) return fail(TDS_ERR_UNSUPPORTED, kNoFloatingId);
  const TdsDynLayout L = tds_dyn_layout(model);
  const int nd = model->dof_qd, nu = id ? nd : nd - (model->is_floating ? 6 : 0);
  *a = {model, n, k, p, id ? TDS_DYN_ID : what, nu, id ? L.qdd : L.tau + nd - nu, (const double *)q, (const double *)qd,
        (const double *)u, (const double *)theta, (const double *)v, params,
        {(double *)out->x_world, (double *)out->mass_matrix, (double *)out->bias, (double *)out->qdd},
        {(double *)dout->x_world, (double *)dout->mass_matrix, (double *)dout->bias, (double *)dout->qdd}};
  return TDS_OK;
}

int tds_dyn_jvp_device(const char *who, tds_hip_sim_t *s, int id, int n, const void *q, const void *qd, const void *u, int p,
                       const tds_param_t *params_host, const void *theta, int k, const void *v, const tds_dyn_out_t *out,
                       const tds_dyn_out_t *dout) {
  return tds_query_jvp_device<TdsDynJvpUnit>(who, s, p, params_host, k, [&](const tds_model_t *m, TdsDynJvpArgs *a) {
    return tds_dyn_jvp_args(who, m, id, n, q, qd, u, p, params_host, theta, k, v, out, dout, a);
  });
}

int tds_dyn_jvp_host(const char *who, const tds_model_t *model, int id, int n, const double *q, const double *qd,
                     const double *u, int p, const tds_param_t *params, const double *theta, int k, const double *v,
                     const tds_dyn_out_t *out, const tds_dyn_out_t *dout) {
  return tds_query_jvp_host<TdsDynJvpUnit>(who, model, p, params, k, [&](const tds_model_t *m, TdsDynJvpArgs *a) {
    return tds_dyn_jvp_args(who, m, id, n, q, qd, u, p, params, theta, k, v, out, dout, a);
  });
}

// inverse dynamics' torques and their tangents as the `bias` of an output set
tds_dyn_out_t tds_dyn_jvp_id_out(void *tau) { return {nullptr, nullptr, tau, nullptr}; }

}  // namespace

extern "C" {

int tds_hip_dynamics_jvp(tds_hip_sim_t *s, int n, const void *q_dev, const void *qd_dev, const void *tau_dev, int p,
                         const tds_param_t *params_host, const void *theta_dev, int k, const void *v_dev,
                         const tds_dyn_out_t *out, const tds_dyn_out_t *dout) {
  return tds_dyn_jvp_device("tds_hip_dynamics_jvp", s, 0, n, q_dev, qd_dev, tau_dev, p, params_host, theta_dev, k, v_dev,
                            out, dout);
}

int tds_hip_inverse_dynamics_jvp(tds_hip_sim_t *s, int n, const void *q_dev, const void *qd_dev, const void *qdd_dev,
                                 int p, const tds_param_t *params_host, const void *theta_dev, int k, const void *v_dev,
                                 void *tau_dev, void *dtau_dev) {
  const tds_dyn_out_t out = tds_dyn_jvp_id_out(tau_dev), dout = tds_dyn_jvp_id_out(dtau_dev);
  return tds_dyn_jvp_device("tds_hip_inverse_dynamics_jvp", s, 1, n, q_dev, qd_dev, qdd_dev, p, params_host, theta_dev, k,
                            v_dev, &out, &dout);
}

int tds_hip_dynamics_jvp_host(const tds_model_t *model, int n, const double *q, const double *qd, const double *tau,
                              int p, const tds_param_t *params, const double *theta, int k, const double *v,
                              const tds_dyn_out_t *out, const tds_dyn_out_t *dout) {
  return tds_dyn_jvp_host("tds_hip_dynamics_jvp_host", model, 0, n, q, qd, tau, p, params, theta, k, v, out, dout);
}

int tds_hip_inverse_dynamics_jvp_host(const tds_model_t *model, int n, const double *q, const double *qd,
                                      const double *qdd, int p, const tds_param_t *params, const double *theta, int k,
                                      const double *v, double *tau, double *dtau) {
  const tds_dyn_out_t out = tds_dyn_jvp_id_out(tau), dout = tds_dyn_jvp_id_out(dtau);
  return tds_dyn_jvp_host("tds_hip_inverse_dynamics_jvp_host", model, 1, n, q, qd, qdd, p, params, theta, k, v, &out,
                          &dout);
}

int tds_hip_dynamics_jvp_tangents(const tds_model_t *model) {
  return tds_query_jvp_tangents<TdsDynJvpUnit>("tds_hip_dynamics_jvp_tangents", model);
}

}  // extern "C"
