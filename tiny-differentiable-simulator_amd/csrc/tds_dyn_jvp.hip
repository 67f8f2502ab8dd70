// tds_dyn_jvp.hip — forward-mode derivatives of the batched dynamics queries on gfx950 (tds_dyn.h over TdsDual<K> and an
// overlay of parameters) and their C ABI: tds_hip_dynamics_jvp, tds_hip_inverse_dynamics_jvp, their _host checkers and
// tds_hip_dynamics_jvp_tangents (include/tds_hip.h).
//
// The input of a call is z = [q (dof_q) | qd (dof_qd) | u | theta (p)]: u is tau (the actuated dofs) for the dynamics
// call and qdd (dof_qd) for inverse dynamics.  Directions are v [n][k][z], tangents [n][k][...the output's shape...].
//
// Mapping: tds_contact_jvp.hip's.  A work item is (environment, block of K directions); a workgroup of W <= 64 lanes
// takes W neighbouring environments of one block, at most kQueryLanes lanes per launch and the grid's stride beyond.  A
// lane's state is tds_dyn_layout's, every component a TdsDual<K>: [component][lane] of (K + 1) doubles in the handle's
// work buffer.  One value or tangent plane of that state is a TdsDynMem<double> with base offset j and stride
// lanes (K + 1): q, qd, u and the columns of v go in, and the outputs and tangents come out, through tds_query.h's LDS
// tile, plane by plane.  The lane's overlay of parameters (TdsParamOverlay: indexed at run time) lives in the work
// buffer behind the states; nothing indexed at run time is kept in the private segment.
// K = 0 (a call with k = 0): the same kernel over double and an overlay of doubles, the primal at theta.
#include <hip/hip_runtime.h>

#include "tds_dparam.h"
#include "tds_query.h"
#include "tds_query_dual.h"

namespace {

// tangents per work item of each class on the device (the resource table)
template <class B>
struct TdsDynJvpK;
template <>
struct TdsDynJvpK<TdsBoundS> { static constexpr int K = 2; };
template <>
struct TdsDynJvpK<TdsBoundA> { static constexpr int K = 2; };
template <>
struct TdsDynJvpK<TdsBoundL> { static constexpr int K = 2; };

enum { kDynXw = 0, kDynM = 1, kDynBias = 2, kDynQdd = 3, kDynOuts = 4 };

struct TdsDynJvpArgs {
  const tds_model_t *m;
  int n, kdirs, p, what;
  int nu, uoff;  // u's entries and the component of the state where they start (L.tau behind the base's six, or L.qdd)
  const double *q, *qd, *u, *theta, *v;
  const tds_param_t *params;
  double *o[kDynOuts], *d[kDynOuts];  // primal outputs; tangents [n][kdirs][shape]  (bias: ID's torques with TDS_DYN_ID)
};

// theta of environment env and its tangents of directions d0 .. d0 + nk - 1 (zeros past them) into the seeded overlay:
// both slots of each selected scalar (an off-diagonal inertia entry sets its mirror too).  theta NULL: the seed's value
template <int K, typename T, class B>
TDS_HD inline void tds_dyn_jvp_theta(const TdsDynJvpArgs &a, TdsParamOverlay<T, B> &P, int env, int d0, int nk) {
  const int nx = a.m->dof_q + a.m->dof_qd + a.nu, nall = nx + a.p;
  for (int j = 0; j < a.p; ++j)
    for (int mirror = 0; mirror < 2; ++mirror) {
      T *slot = tds_param_slot(P, a.params[j], mirror);
      tds_contact_set_value(*slot, a.theta ? a.theta[(size_t)env * a.p + j] : tds_value(*slot));
      for (int k = 0; k < nk; ++k)
        tds_contact_set_tangent(*slot, k, a.v[((size_t)env * a.kdirs + d0 + k) * nall + nx + j]);
    }
}

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
  using T = typename TdsContactScalar<K>::type;
  static_assert(sizeof(T) == (K + 1) * sizeof(double), "a dual is its value and K tangents, nothing else");
  __shared__ double tile[64 * kTileS];
  const tds_model_t *m = a.m;
  const TdsDynLayout L = tds_dyn_layout(m);
  const TdsDynJvpOuts O = tds_dyn_jvp_outs(m, L);
  const int W = blockDim.x, t = threadIdx.x, nq = m->dof_q, nd = m->dof_qd, nz = nq + nd + a.nu + a.p;
  const int have_u = a.what & (TDS_DYN_QDD | TDS_DYN_ID), upad = (a.what & TDS_DYN_QDD) ? nd - a.nu : 0;
  const size_t lane = (size_t)blockIdx.x * W + t;
  const TdsDynMem<T> w = {(T *)buf + lane, (size_t)lanes};
  // plane j of the state: 0 the values, 1 + k the tangents of the block's direction k
  const auto plane = [&](int j) { return TdsDynMem<double>{buf + lane * (K + 1) + j, (size_t)lanes * (K + 1)}; };
  TdsParamOverlay<T, B> &P = ovl[lane];
  const int chunks = (a.n + W - 1) / W, blocks = a.kdirs > 0 ? (a.kdirs + K - 1) / (K ? K : 1) : 1;
  const long long groups = (long long)chunks * blocks;
  tds_param_seed(m, P);  // the blob's values, all constant: once per lane
  for (long long g = blockIdx.x; g < groups; g += gridDim.x) {
    const int e0 = (int)(g % chunks) * W, d0 = (int)(g / chunks) * K;  // neighbouring workgroups: neighbouring environments
    const int nv = a.n - e0 < W ? a.n - e0 : W, nk = a.kdirs - d0 < K ? a.kdirs - d0 : K;
    // (<true>: an input that is NULL stands for zeros; the base's six torques, upad, are zeros)
    tds_query_ingest<true>(tile, plane(0), L.q, a.q, nq, e0, nv);
    tds_query_ingest<true>(tile, plane(0), L.qd, a.qd, nd, e0, nv);
    if (have_u) {
      tds_query_ingest<true>(tile, plane(0), a.uoff - upad, nullptr, upad, e0, nv);
      tds_query_ingest<true>(tile, plane(0), a.uoff, a.u, a.nu, e0, nv);
    }
    for (int k = 0; k < K; ++k) {
      // direction d0 + k's columns of v, in z's order; directions past kdirs in the last block: zero
      const double *vk = k < nk ? a.v + (size_t)(d0 + k) * nz : nullptr;
      const size_t vs = (size_t)a.kdirs * nz;
      const auto seed = [&](int off, int col, int cnt) {
        if (vk)
          tds_query_ingest_strided(tile, plane(1 + k), off, vk + col, cnt, vs, e0, nv);
        else
          tds_query_ingest<true>(tile, plane(1 + k), off, nullptr, cnt, e0, nv);
      };
      seed(L.q, 0, nq);
      seed(L.qd, nq, nd);
      if (have_u) {
        tds_query_ingest<true>(tile, plane(1 + k), a.uoff - upad, nullptr, upad, e0, nv);
        seed(a.uoff, nq + nd, a.nu);
      }
    }
    int bad = 0;
    if (t < nv) {
      tds_dyn_jvp_theta<K>(a, P, e0 + t, d0, nk);
      bad = tds_dyn_eval(m, TdsOverlayView<T, B>{&P}, w, L, a.what, 0, 0);  // M not positive definite
    }
    // each output: the primal by the first block's items, then this block's tangents [n][kdirs][cnt]; qdd of an
    // environment whose M is not positive definite is NaN, and so are its tangents
    for (int i = 0; i < kDynOuts; ++i) {
      const int off = O.off[i], cnt = O.cnt[i], nan = i == kDynQdd ? bad : 0;
      if (a.o[i] && d0 == 0) tds_query_emit(tile, plane(0), off, a.o[i], cnt, e0, nv, nan);
      if (a.d[i])
        for (int k = 0; k < nk; ++k)
          tds_query_emit_strided(tile, plane(1 + k), off, a.d[i] + (size_t)(d0 + k) * cnt, cnt, (size_t)a.kdirs * cnt, e0,
                                 nv, nan);
    }
  }
}

// a launch over n environments x kdirs directions: tds_query_width's workgroups over the groups of items; the work
// buffer is  states [total][lanes] of T | overlays [lanes] | the selection
struct TdsDynJvpPlan {
  int W;
  long long blocks, lanes;
  size_t states, overlays;
};
template <class B, int K>
TdsDynJvpPlan tds_dyn_jvp_plan(const tds_hip_sim *s, int n, int kdirs, int total) {
  using T = typename TdsContactScalar<K>::type;
  TdsDynJvpPlan p;
  p.W = tds_query_width(s, n);
  p.blocks = (((long long)n + p.W - 1) / p.W) * (kdirs > 0 ? (kdirs + K - 1) / (K ? K : 1) : 1);
  if (p.blocks > kQueryLanes / p.W) p.blocks = kQueryLanes / p.W;
  p.lanes = p.blocks * p.W;
  p.states = ((size_t)p.lanes * total * sizeof(T) + 255) & ~(size_t)255;
  p.overlays = ((size_t)p.lanes * sizeof(TdsParamOverlay<T, B>) + 255) & ~(size_t)255;
  return p;
}

template <class B, int K>
int tds_dyn_jvp_launch(tds_hip_sim *s, TdsDynJvpArgs a, const tds_param_t *params_host) {
  using T = typename TdsContactScalar<K>::type;
  const TdsDynJvpPlan p = tds_dyn_jvp_plan<B, K>(s, a.n, a.kdirs, tds_dyn_layout(&s->model).total);
  const size_t sel = (size_t)a.p * sizeof(tds_param_t);
  if (const int rc = tds_work_buffer(s, p.states + p.overlays + sel)) return rc;
  char *base = (char *)s->d_diff_tmp;
  if (a.p > 0) {  // a blocking copy: earlier calls on the stream may still read the work buffer
    TDS_HIP_TRY(hipStreamSynchronize(s->stream));
    TDS_HIP_TRY(hipMemcpy(base + p.states + p.overlays, params_host, sel, hipMemcpyHostToDevice));
  }
  a.params = (const tds_param_t *)(base + p.states + p.overlays);
  hipLaunchKernelGGL((tds_dyn_jvp_kernel<B, K>), dim3((unsigned)p.blocks), dim3(p.W), 0, s->stream, a, (double *)base,
                     (TdsParamOverlay<T, B> *)(base + p.states), (int)p.lanes);
  TDS_HIP_TRY(hipGetLastError());
  return TDS_OK;
}

// the host instantiation: one environment and block at a time in a state of its own (stride 1)
template <class B, int K>
int tds_dyn_jvp_host_impl(const TdsDynJvpArgs &a) {
  using T = typename TdsContactScalar<K>::type;
  const tds_model_t *m = a.m;
  const TdsDynLayout L = tds_dyn_layout(m);
  const TdsDynJvpOuts O = tds_dyn_jvp_outs(m, L);
  const int nq = m->dof_q, nd = m->dof_qd, nz = nq + nd + a.nu + a.p;
  std::vector<T> buf(L.total);
  std::vector<TdsParamOverlay<T, B>> P(1);
  const TdsDynMem<T> w = {buf.data(), 1};
  tds_param_seed(m, P[0]);
  int any_bad = 0;
  for (int e = 0; e < a.n; ++e)
    for (int d0 = 0; d0 == 0 || d0 < a.kdirs; d0 += K ? K : 1) {
      const int nk = a.kdirs - d0 < K ? a.kdirs - d0 : K;
      // record e of src [.][cnt] (NULL: zeros) and the block's columns col .. of v -> components off ..
      const auto put = [&](int off, const double *src, int col, int cnt) {
        for (int c = 0; c < cnt; ++c) {
          tds_contact_set_value(buf[off + c], src ? src[(size_t)e * cnt + c] : 0.0);
          for (int k = 0; k < nk; ++k)
            tds_contact_set_tangent(buf[off + c], k, a.v[((size_t)e * a.kdirs + d0 + k) * nz + col + c]);
        }
      };
      put(L.q, a.q, 0, nq);
      put(L.qd, a.qd, nq, nd);
      if (a.what & TDS_DYN_QDD)
        for (int c = 0; c < nd - a.nu; ++c) tds_contact_set_value(buf[L.tau + c], 0.0);
      if (a.what & (TDS_DYN_QDD | TDS_DYN_ID)) put(a.uoff, a.u, nq + nd, a.nu);
      tds_dyn_jvp_theta<K>(a, P[0], e, d0, nk);
      const int bad = tds_dyn_eval(m, TdsOverlayView<T, B>{&P[0]}, w, L, a.what, 0, 0);
      any_bad |= bad;
      for (int i = 0; i < kDynOuts; ++i) {
        const double *src = (const double *)(buf.data() + O.off[i]);  // [cnt][K + 1]
        const int cnt = O.cnt[i], nan = i == kDynQdd ? bad : 0;
        if (a.o[i] && d0 == 0)
          for (int c = 0; c < cnt; ++c) a.o[i][(size_t)e * cnt + c] = nan ? __builtin_nan("") : src[c * (K + 1)];
        if (a.d[i])
          for (int k = 0; k < nk; ++k)
            for (int c = 0; c < cnt; ++c)
              a.d[i][((size_t)e * a.kdirs + d0 + k) * cnt + c] = nan ? __builtin_nan("") : src[c * (K + 1) + 1 + k];
      }
    }
  return any_bad ? fail(TDS_ERR_INVALID_ARG, "dynamics queries: joint-space inertia not positive definite%s") : TDS_OK;
}

// (the primal queries' message, tds_dyn.hip)
const char kNoFloatingId[] =
    "dynamics queries: bias and inverse dynamics need a fixed base (the reference has no floating-base inverse dynamics)%s";

// the arguments of an entry point, checked, as the kernel's and the host loop's; out / dout NULL: no output of that
// kind.  id: the inverse-dynamics call (u is qdd, the torques are out->bias / dout->bias)
int tds_dyn_jvp_args(const char *who, const tds_model_t *model, int id, int n, const void *q, const void *qd, const void *u,
                     int p, const tds_param_t *params, const void *theta, int k, const void *v, const tds_dyn_out_t *out,
                     const tds_dyn_out_t *dout, TdsDynJvpArgs *a) {
  static const tds_dyn_out_t none = {};
  if (!out) out = &none;
  if (!dout || k == 0) dout = &none;
  if (!q || n < 1 || k < 0 || p < 0 || (p > 0 && !params) || (k > 0 && !v))
    return fail(TDS_ERR_INVALID_ARG, "%s: NULL or empty argument", who);
  const auto what_of = [](const tds_dyn_out_t *o) {
    return (o->x_world ? TDS_DYN_XW : 0) | (o->mass_matrix ? TDS_DYN_M : 0) | (o->bias ? TDS_DYN_BIAS : 0) |
           (o->qdd ? TDS_DYN_QDD : 0);
  };
  if (!what_of(k > 0 ? dout : out)) return fail(TDS_ERR_INVALID_ARG, "%s: no output requested", who);
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
  if (!s) return fail(TDS_ERR_INVALID_ARG, "%s: NULL or empty argument", who);
  DeviceGuard guard(s->device);
  int cls, rc = tds_diff_prepare(s, &cls);
  if (rc) return rc;
  if ((rc = tds_param_check_sel(&s->model, p, params_host))) return rc;
  TdsDynJvpArgs a;
  if ((rc = tds_dyn_jvp_args(who, &s->model, id, n, q, qd, u, p, params_host, theta, k, v, out, dout, &a))) return rc;
  a.m = (const tds_model_t *)s->d_diff_model;
  return tds_with_bound(cls, [&](auto b) {
    using B = typename decltype(b)::type;
    return k ? tds_dyn_jvp_launch<B, TdsDynJvpK<B>::K>(s, a, params_host) : tds_dyn_jvp_launch<B, 0>(s, a, params_host);
  });
}

int tds_dyn_jvp_host(const char *who, const tds_model_t *model, int id, int n, const double *q, const double *qd,
                     const double *u, int p, const tds_param_t *params, const double *theta, int k, const double *v,
                     const tds_dyn_out_t *out, const tds_dyn_out_t *dout) {
  if (!model) return fail(TDS_ERR_INVALID_ARG, "%s: NULL or empty argument", who);
  int cls, rc = tds_param_host_prepare(model, p, params, &cls);
  if (rc) return rc;
  TdsDynJvpArgs a;
  if ((rc = tds_dyn_jvp_args(who, model, id, n, q, qd, u, p, params, theta, k, v, out, dout, &a))) return rc;
  return tds_with_bound(cls, [&](auto b) {
    using B = typename decltype(b)::type;
    return k ? tds_dyn_jvp_host_impl<B, kHostK>(a) : tds_dyn_jvp_host_impl<B, 0>(a);
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
  if (!model) return -fail(TDS_ERR_INVALID_ARG, "tds_hip_dynamics_jvp_tangents: NULL model%s");
  int cls;
  if (const int rc = tds_diff_host_check(model, &cls)) return -rc;
  return tds_with_bound(cls, [&](auto b) { return TdsDynJvpK<typename decltype(b)::type>::K; });
}

}  // extern "C"
