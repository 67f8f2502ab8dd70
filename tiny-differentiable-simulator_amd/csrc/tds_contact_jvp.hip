// tds_contact_jvp.hip — forward-mode derivatives of the batched contact query in [x | theta] on gfx950 (tds_contact.h
// over TdsDual<K> and an overlay of parameters) and their C ABI: tds_hip_contacts_jvp, the CPU checker
// tds_hip_contacts_jvp_host and tds_hip_contacts_jvp_tangents (include/tds_hip.h).
//
// Mapping.  A work item is (environment, block of K directions): the K tangents of a block share the primal.  A
// workgroup of W <= 64 lanes takes W neighbouring environments of one block (tds_query.h's mapping, a group of items per
// round), at most kQueryLanes lanes per launch and the grid's stride beyond.  A lane's state is tds_contact_layout's,
// every component a TdsDual<K>: [component][lane] of (K + 1) doubles, so that a wave's access to one component is one
// run of 64 (K + 1) 8 B.  One value or tangent plane of that state is a TdsDynMem<double> with base offset j and stride
// lanes (K + 1): the records and the seed go in, and the outputs and tangents come out, through tds_query.h's LDS
// tile, plane by plane.  The lane's overlay of parameters (TdsParamOverlay: indexed at run time) lives in the work
// buffer behind the states, as in tds_dparam.hip; nothing indexed at run time is kept in the private segment.
// K = 0 (tds_hip_contacts_jvp with k = 0): the same kernel over double and an overlay of doubles, the primal at theta.
#include <hip/hip_runtime.h>

#include "tds_contact.h"
#include "tds_dparam.h"
#include "tds_query.h"
#include "tds_query_dual.h"

namespace {

// tangents per work item of each class on the device (the resource table)
template <class B>
struct TdsContactJvpK;
template <>
struct TdsContactJvpK<TdsBoundS> { static constexpr int K = 2; };
template <>
struct TdsContactJvpK<TdsBoundA> { static constexpr int K = 2; };
template <>
struct TdsContactJvpK<TdsBoundL> { static constexpr int K = 2; };

struct TdsContactJvpArgs {
  const tds_model_t *m;
  int n, kdirs, p, what, with_A;
  const double *x, *theta, *v;
  const tds_param_t *params;
  tds_contact_out_t out, dout;  // primal outputs; tangents [n][kdirs][shape]
};

// theta of environment env and its tangents of directions d0 .. d0 + nk - 1 (zeros past them) into the seeded overlay:
// both slots of each selected scalar (an off-diagonal inertia entry sets its mirror too).  theta NULL: the seed's value
template <int K, typename T, class B>
TDS_HD inline void tds_contact_jvp_theta(const TdsContactJvpArgs &a, TdsParamOverlay<T, B> &P, int env, int d0, int nk) {
  const int nall = a.m->input_dim + a.p;
  for (int j = 0; j < a.p; ++j)
    for (int mirror = 0; mirror < 2; ++mirror) {
      T *slot = tds_param_slot(P, a.params[j], mirror);
      tds_contact_set_value(*slot, a.theta ? a.theta[(size_t)env * a.p + j] : tds_value(*slot));
      for (int k = 0; k < nk; ++k)
        tds_contact_set_tangent(*slot, k, a.v[((size_t)env * a.kdirs + d0 + k) * nall + a.m->input_dim + j]);
    }
}

template <class B, int K>
__global__ void __launch_bounds__(64) tds_contact_jvp_kernel(TdsContactJvpArgs a, double *buf,
                                                             TdsParamOverlay<typename TdsContactScalar<K>::type, B> *ovl,
                                                             int lanes) {
  using T = typename TdsContactScalar<K>::type;
  static_assert(sizeof(T) == (K + 1) * sizeof(double), "a dual is its value and K tangents, nothing else");
  __shared__ double tile[64 * kTileS];
  const tds_model_t *m = a.m;
  const TdsContactLayout L = tds_contact_layout(m, a.with_A);
  const int W = blockDim.x, t = threadIdx.x, nin = m->input_dim, nd = m->dof_qd, nc = L.nc, nr = 3 * nc;
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
    tds_query_ingest(tile, plane(0), L.x, a.x, nin, e0, nv);
    for (int k = 0; k < K; ++k)
      if (k < nk) {
        tds_query_ingest_strided(tile, plane(1 + k), L.x, a.v + (size_t)(d0 + k) * (nin + a.p), nin,
                                 (size_t)a.kdirs * (nin + a.p), e0, nv);
      } else if (t < nv) {  // directions past kdirs in the last block: zero
        const TdsDynMem<double> z = plane(1 + k);
        for (int c = 0; c < nin; ++c) z[L.x + c] = 0.0;
      }
    int bad = 0;
    if (t < nv) {
      tds_contact_jvp_theta<K>(a, P, e0 + t, d0, nk);
      bad = tds_contact_eval(m, TdsOverlayView<T, B>{&P}, w, L, a.what);  // M not positive definite
    }
    // output `off` [cnt]: the primal by the first block's items, then this block's tangents [n][kdirs][cnt]
    const auto emit = [&](void *o, void *dto, int off, int cnt, int nan) {
      if (!cnt) return;
      if (o && d0 == 0) tds_query_emit(tile, plane(0), off, (double *)o, cnt, e0, nv, nan);
      if (dto)
        for (int k = 0; k < nk; ++k)
          tds_query_emit_strided(tile, plane(1 + k), off, (double *)dto + (size_t)(d0 + k) * cnt, cnt,
                                 (size_t)a.kdirs * cnt, e0, nv, nan);
    };
    emit(a.out.contacts, a.dout.contacts, L.cp, 10 * nc, 0);
    emit(a.out.jac, a.dout.jac, L.cjac, 3 * nd * nc, 0);
    emit(a.out.rows, a.dout.rows, L.J, nr * nd, bad);
    emit(a.out.rhs, a.dout.rhs, L.b, nr, bad);
    emit(a.out.delassus, a.dout.delassus, L.A, nr * nr, bad);
    emit(a.out.impulse, a.dout.impulse, L.p, nr, bad);
    emit(a.out.force, a.dout.force, L.force, nr, bad);
    emit(a.out.qd_pre, a.dout.qd_pre, L.qd_pre, nd, bad);
    emit(a.out.qd_post, a.dout.qd_post, L.qd_post, nd, bad);
  }
}

// a launch over n environments x kdirs directions: tds_query_plan's workgroups over the groups of items; the work
// buffer is  states [total][lanes] of T | overlays [lanes] | the selection
struct TdsContactJvpPlan {
  int W;
  long long blocks, lanes;
  size_t states, overlays;
};
template <class B, int K>
TdsContactJvpPlan tds_contact_jvp_plan(const tds_hip_sim *s, int n, int kdirs, int total) {
  using T = typename TdsContactScalar<K>::type;
  TdsContactJvpPlan p;
  p.W = tds_query_width(s, n);
  p.blocks = (((long long)n + p.W - 1) / p.W) * (kdirs > 0 ? (kdirs + K - 1) / (K ? K : 1) : 1);
  if (p.blocks > kQueryLanes / p.W) p.blocks = kQueryLanes / p.W;
  p.lanes = p.blocks * p.W;
  p.states = ((size_t)p.lanes * total * sizeof(T) + 255) & ~(size_t)255;
  p.overlays = ((size_t)p.lanes * sizeof(TdsParamOverlay<T, B>) + 255) & ~(size_t)255;
  return p;
}

template <class B, int K>
int tds_contact_jvp_launch(tds_hip_sim *s, TdsContactJvpArgs a, const tds_param_t *params_host) {
  using T = typename TdsContactScalar<K>::type;
  const TdsContactJvpPlan p = tds_contact_jvp_plan<B, K>(s, a.n, a.kdirs, tds_contact_layout(&s->model, a.with_A).total);
  const size_t sel = (size_t)a.p * sizeof(tds_param_t);
  if (const int rc = tds_work_buffer(s, p.states + p.overlays + sel)) return rc;
  char *base = (char *)s->d_diff_tmp;
  if (a.p > 0) {  // a blocking copy: earlier calls on the stream may still read the work buffer
    TDS_HIP_TRY(hipStreamSynchronize(s->stream));
    TDS_HIP_TRY(hipMemcpy(base + p.states + p.overlays, params_host, sel, hipMemcpyHostToDevice));
  }
  a.params = (const tds_param_t *)(base + p.states + p.overlays);
  hipLaunchKernelGGL((tds_contact_jvp_kernel<B, K>), dim3((unsigned)p.blocks), dim3(p.W), 0, s->stream, a,
                     (double *)base, (TdsParamOverlay<T, B> *)(base + p.states), (int)p.lanes);
  TDS_HIP_TRY(hipGetLastError());
  return TDS_OK;
}

// the host instantiation: one environment and block at a time in a state of its own (stride 1)
template <class B, int K>
int tds_contact_jvp_host_impl(const TdsContactJvpArgs &a) {
  using T = typename TdsContactScalar<K>::type;
  const tds_model_t *m = a.m;
  const TdsContactLayout L = tds_contact_layout(m, a.with_A);
  const int nin = m->input_dim, nall = nin + a.p, nd = m->dof_qd, nc = L.nc, nr = 3 * nc;
  std::vector<T> buf(L.total);
  std::vector<TdsParamOverlay<T, B>> P(1);
  const TdsDynMem<T> w = {buf.data(), 1};
  tds_param_seed(m, P[0]);
  int any_bad = 0;
  for (int e = 0; e < a.n; ++e)
    for (int d0 = 0; d0 == 0 || d0 < a.kdirs; d0 += K ? K : 1) {
      const int nk = a.kdirs - d0 < K ? a.kdirs - d0 : K;
      for (int c = 0; c < nin; ++c) {
        tds_contact_set_value(buf[L.x + c], a.x[(size_t)e * nin + c]);
        for (int k = 0; k < nk; ++k)
          tds_contact_set_tangent(buf[L.x + c], k, a.v[((size_t)e * a.kdirs + d0 + k) * nall + c]);
      }
      tds_contact_jvp_theta<K>(a, P[0], e, d0, nk);
      const int bad = tds_contact_eval(m, TdsOverlayView<T, B>{&P[0]}, w, L, a.what);
      any_bad |= bad;
      const auto get = [&](void *o, void *dto, int off, int cnt, int nan) {
        const double *src = (const double *)(buf.data() + off);  // [cnt][K + 1]
        if (o && d0 == 0)
          for (int c = 0; c < cnt; ++c) ((double *)o)[(size_t)e * cnt + c] = nan ? __builtin_nan("") : src[c * (K + 1)];
        if (dto)
          for (int k = 0; k < nk; ++k)
            for (int c = 0; c < cnt; ++c)
              ((double *)dto)[((size_t)e * a.kdirs + d0 + k) * cnt + c] = nan ? __builtin_nan("") : src[c * (K + 1) + 1 + k];
      };
      get(a.out.contacts, a.dout.contacts, L.cp, 10 * nc, 0);
      get(a.out.jac, a.dout.jac, L.cjac, 3 * nd * nc, 0);
      get(a.out.rows, a.dout.rows, L.J, nr * nd, bad);
      get(a.out.rhs, a.dout.rhs, L.b, nr, bad);
      get(a.out.delassus, a.dout.delassus, L.A, nr * nr, bad);
      get(a.out.impulse, a.dout.impulse, L.p, nr, bad);
      get(a.out.force, a.dout.force, L.force, nr, bad);
      get(a.out.qd_pre, a.dout.qd_pre, L.qd_pre, nd, bad);
      get(a.out.qd_post, a.dout.qd_post, L.qd_post, nd, bad);
    }
  return any_bad ? fail(TDS_ERR_INVALID_ARG, "contact query: joint-space inertia not positive definite%s") : TDS_OK;
}

// the arguments of an entry point, checked, as the kernel's and the host loop's (a->what == 0: nothing with extent
// is asked for); out / dout NULL: no output of that kind
int tds_contact_jvp_args(const char *who, const tds_model_t *model, int n, const void *x, int p, const tds_param_t *params,
                         const void *theta, int k, const void *v, const tds_contact_out_t *out,
                         const tds_contact_out_t *dout, TdsContactJvpArgs *a) {
  static const tds_contact_out_t none = {};
  if (!out) out = &none;
  if (!dout || k == 0) dout = &none;
  if (!x || n < 1 || k < 0 || p < 0 || (p > 0 && !params) || (k > 0 && !v))
    return fail(TDS_ERR_INVALID_ARG, "%s: NULL or empty argument", who);
  if (k > 0 ? !tds_contact_any(dout) : !tds_contact_any(out))
    return fail(TDS_ERR_INVALID_ARG, "%s: no output requested", who);
  const int nc = tds_contact_count(model), what = tds_contact_what(out, nc) | tds_contact_what(dout, nc);
  *a = {model, n, k, p, what, (what & TDS_CT_DELASSUS) ? 1 : 0, (const double *)x, (const double *)theta,
        (const double *)v, params, *out, *dout};
  return TDS_OK;
}

}  // namespace

extern "C" {

int tds_hip_contacts_jvp(tds_hip_sim_t *s, int n, const void *x_dev, int p, const tds_param_t *params_host,
                         const void *theta_dev, int k, const void *v_dev, const tds_contact_out_t *out,
                         const tds_contact_out_t *dout) {
  if (!s) return fail(TDS_ERR_INVALID_ARG, "tds_hip_contacts_jvp: NULL or empty argument%s");
  DeviceGuard guard(s->device);
  int cls, rc = tds_diff_prepare(s, &cls);
  if (rc) return rc;
  if ((rc = tds_param_check_sel(&s->model, p, params_host))) return rc;
  TdsContactJvpArgs a;
  if ((rc = tds_contact_jvp_args("tds_hip_contacts_jvp", &s->model, n, x_dev, p, params_host, theta_dev, k, v_dev, out,
                                 dout, &a)))
    return rc;
  if (!a.what) return TDS_OK;  // only outputs without extent (no contact points)
  a.m = (const tds_model_t *)s->d_diff_model;
  return tds_with_bound(cls, [&](auto b) {
    using B = typename decltype(b)::type;
    return k ? tds_contact_jvp_launch<B, TdsContactJvpK<B>::K>(s, a, params_host)
             : tds_contact_jvp_launch<B, 0>(s, a, params_host);
  });
}

int tds_hip_contacts_jvp_host(const tds_model_t *model, int n, const double *x, int p, const tds_param_t *params,
                              const double *theta, int k, const double *v, const tds_contact_out_t *out,
                              const tds_contact_out_t *dout) {
  if (!model) return fail(TDS_ERR_INVALID_ARG, "tds_hip_contacts_jvp_host: NULL or empty argument%s");
  int cls, rc = tds_param_host_prepare(model, p, params, &cls);
  if (rc) return rc;
  TdsContactJvpArgs a;
  if ((rc = tds_contact_jvp_args("tds_hip_contacts_jvp_host", model, n, x, p, params, theta, k, v, out, dout, &a)))
    return rc;
  if (!a.what) return TDS_OK;
  return tds_with_bound(cls, [&](auto b) {
    using B = typename decltype(b)::type;
    return k ? tds_contact_jvp_host_impl<B, kHostK>(a) : tds_contact_jvp_host_impl<B, 0>(a);
  });
}

int tds_hip_contacts_jvp_tangents(const tds_model_t *model) {
  if (!model) return -fail(TDS_ERR_INVALID_ARG, "tds_hip_contacts_jvp_tangents: NULL model%s");
  int cls;
  if (const int rc = tds_diff_host_check(model, &cls)) return -rc;
  return tds_with_bound(cls, [&](auto b) { return TdsContactJvpK<typename decltype(b)::type>::K; });
}

}  // extern "C"
