// tds_query_dual.h — the forward-mode driver of the batched queries' derivatives (tds_contact_jvp.hip, tds_dyn_jvp.hip):
// everything about differentiating a query in [inputs | theta] over TdsDual<K> that does not depend on which query.
//
// MAPPING.  A work item is (environment, block of K directions): the K tangents of a block share the primal.  A
// workgroup of W <= 64 lanes takes W neighbouring environments of one block (tds_query.h's mapping, a group of items per
// round), at most kQueryLanes lanes per launch and the grid's stride beyond.  A lane's state is the unit's layout, every
// component a TdsDual<K>: [component][lane] of (K + 1) doubles in the handle's work buffer, so that a wave's access to
// one component is one run of 64 (K + 1) 8 B.  One value or tangent plane of that state is a TdsDynMem<double> with base
// offset j and stride lanes (K + 1): the inputs and the columns of v go in, and the outputs and tangents come out,
// through tds_query.h's LDS tile, plane by plane.  The lane's overlay of parameters (TdsParamOverlay: indexed at run
// time) lives in the work buffer behind the states, as in tds_dparam.hip; nothing indexed at run time is kept in the
// private segment.  K = 0 (a call with k = 0): the same kernel over double and an overlay of doubles, the primal at
// theta.  The host checkers walk the same items one at a time in a state of their own (TdsQueryDualHost).
//
// Here once: the theta seeding and the plane accessor of the kernels, the launch plan and the launch, the host
// checkers' state and loop, the argument checks and the entry points' bodies.
//
// A UNIT states what is its own in one struct U, built from its arguments:
//   U::Args                the argument struct: the members m, n, kdirs, p, what, theta, v, params in an order of its
//                          own (it is the kernel's first argument), the unit's inputs and output pointers, and
//                          columns(): .nall the columns of v in all, .nx() those before theta
//   U::kTangents<B>        tangents per work item of class B on the device;  U::kKernel<B, K>  its __global__ kernel
//   U::kNotPd              the message of an environment whose M is not positive definite
//   U(a)  .total()         components of a state
//         .inputs(put)     put(off, src, col, cnt) per input: components off .. off + cnt take record `src` [.][cnt]
//                          (NULL: zeros) in value and the columns col .. of v in tangent (col < 0: none)
//         .eval(P, w)      the query over the overlay view P in the state w; nonzero: M not positive definite
//         .outputs(get, bad)  get(primal, tangents, off, cnt, nan) per output
#pragma once
#include "tds_dparam.h"
#include "tds_query.h"

namespace {

// the scalar of K tangents; K = 0: double
template <int K>
struct TdsQueryScalar { using type = TdsDual<K>; };
template <>
struct TdsQueryScalar<0> { using type = double; };
// the same under the name that both kernels' symbols carry (profiles/ and the tools that read them hold those
// symbols): for the kernels' parameter lists only
template <int K>
struct TdsContactScalar : TdsQueryScalar<K> {};

// the value a double or a dual is built from
TDS_HD inline void tds_query_set_value(double &t, double v) { t = v; }
template <int K>
TDS_HD inline void tds_query_set_value(TdsDual<K> &t, double v) {
  t = TdsDual<K>(v);
}
TDS_HD inline void tds_query_set_tangent(double &, int, double) {}
template <int K>
TDS_HD inline void tds_query_set_tangent(TdsDual<K> &t, int k, double d) {
  t.d[k] = d;
}

// theta of environment env and its tangents of directions d0 .. d0 + nk - 1 (zeros past them) into the seeded overlay:
// both slots of each selected scalar (an off-diagonal inertia entry sets its mirror too).  theta NULL: the seed's
// value
template <class A, typename T, class B>
TDS_HD inline void tds_query_jvp_theta(const A &a, TdsParamOverlay<T, B> &P, int env, int d0, int nk) {
  const auto cols = a.columns();
  for (int j = 0; j < a.p; ++j)
    for (int mirror = 0; mirror < 2; ++mirror) {
      T *slot = tds_param_slot(P, a.params[j], mirror);
      tds_query_set_value(*slot, a.theta ? a.theta[(size_t)env * a.p + j] : tds_value(*slot));
      for (int k = 0; k < nk; ++k)
        tds_query_set_tangent(*slot, k, a.v[((size_t)env * a.kdirs + d0 + k) * cols.nall + cols.nx() + j]);
    }
}

// ---------------------------------------------------------------- device
// a lane's slice of the work buffer.  The rest of a kernel's walk (group decoding, ingest-or-zeros, the evaluation,
// the emit pair) is written in each kernel: DESIGN 7b says what sharing each piece did to the kernels' code
template <int K>
struct TdsQueryJvpLane {
  static_assert(sizeof(typename TdsQueryScalar<K>::type) == (K + 1) * sizeof(double),
                "a dual is its value and K tangents, nothing else");
  double *buf;
  int lanes;
  size_t lane;
  __device__ TdsQueryJvpLane(double *buf, int lanes, int W, int t) : buf(buf), lanes(lanes), lane((size_t)blockIdx.x * W + t) {}
  // plane j of the lane's state: 0 the values, 1 + k the tangents of the block's direction k
  __device__ TdsDynMem<double> plane(int j) const { return {buf + lane * (K + 1) + j, (size_t)lanes * (K + 1)}; }
};

// a launch over n environments x kdirs directions: tds_query_width's workgroups over the groups of items; the work
// buffer is  states [total][lanes] of T | overlays [lanes] | the selection
struct TdsQueryJvpPlan {
  int W;
  long long blocks, lanes;
  size_t states, overlays;
};
template <class B, int K>
TdsQueryJvpPlan tds_query_jvp_plan(const tds_hip_sim *s, int n, int kdirs, int total) {
  using T = typename TdsQueryScalar<K>::type;
  TdsQueryJvpPlan p;
  p.W = tds_query_width(s, n);
  p.blocks = (((long long)n + p.W - 1) / p.W) * (kdirs > 0 ? (kdirs + K - 1) / (K ? K : 1) : 1);
  if (p.blocks > kQueryLanes / p.W) p.blocks = kQueryLanes / p.W;
  p.lanes = p.blocks * p.W;
  p.states = ((size_t)p.lanes * total * sizeof(T) + 255) & ~(size_t)255;
  p.overlays = ((size_t)p.lanes * sizeof(TdsParamOverlay<T, B>) + 255) & ~(size_t)255;
  return p;
}

template <class U, class B, int K>
int tds_query_jvp_launch(tds_hip_sim *s, typename U::Args a, int total, const tds_param_t *params_host) {
  using T = typename TdsQueryScalar<K>::type;
  const TdsQueryJvpPlan p = tds_query_jvp_plan<B, K>(s, a.n, a.kdirs, total);
  const size_t sel = (size_t)a.p * sizeof(tds_param_t);
  if (const int rc = tds_work_buffer(s, p.states + p.overlays + sel)) return rc;
  char *base = (char *)s->d_diff_tmp;
  if (a.p > 0) {  // a blocking copy: earlier calls on the stream may still read the work buffer
    TDS_HIP_TRY(hipStreamSynchronize(s->stream));
    TDS_HIP_TRY(hipMemcpy(base + p.states + p.overlays, params_host, sel, hipMemcpyHostToDevice));
  }
  a.params = (const tds_param_t *)(base + p.states + p.overlays);
  hipLaunchKernelGGL((U::template kKernel<B, K>), dim3((unsigned)p.blocks), dim3(p.W), 0, s->stream, a, (double *)base,
                     (TdsParamOverlay<T, B> *)(base + p.states), (int)p.lanes);
  TDS_HIP_TRY(hipGetLastError());
  return TDS_OK;
}

// ---------------------------------------------------------------- host
// the host checkers' state of duals, beside TdsQueryHost: one environment and block of directions at a time in a
// vector of its own (stride 1), the overlay seeded once
template <class B, int K>
struct TdsQueryDualHost {
  using T = typename TdsQueryScalar<K>::type;
  std::vector<T> buf;
  std::vector<TdsParamOverlay<T, B>> P;
  TdsDynMem<T> w;
  const double *v;  // directions [n][kdirs][nz]
  int kdirs, nz;
  int e = 0, d0 = 0, nk = 0;  // the item at hand
  TdsQueryDualHost(const tds_model_t *m, int total, const double *v, int kdirs, int nz)
      : buf(total), P(1), w{buf.data(), 1}, v(v), kdirs(kdirs), nz(nz) {
    tds_param_seed(m, P[0]);
  }
  // record e of src [.][cnt] (NULL: zeros) and the block's columns col .. of v (col < 0: none) -> components off ..
  void put(int off, const double *src, int col, int cnt) {
    for (int c = 0; c < cnt; ++c) {
      tds_query_set_value(buf[off + c], src ? src[(size_t)e * cnt + c] : 0.0);
      for (int k = 0; k < nk && col >= 0; ++k)
        tds_query_set_tangent(buf[off + c], k, v[((size_t)e * kdirs + d0 + k) * nz + col + c]);
    }
  }
  // components off .. [cnt][K + 1] -> record e of o (by the first block) and of dto [n][kdirs][cnt]; NULL: nothing;
  // nan: the records are NaN
  void get(void *o, void *dto, int off, int cnt, int nan) const {
    const double *src = (const double *)(buf.data() + off);
    if (o && d0 == 0)
      for (int c = 0; c < cnt; ++c) ((double *)o)[(size_t)e * cnt + c] = nan ? __builtin_nan("") : src[c * (K + 1)];
    if (dto)
      for (int k = 0; k < nk; ++k)
        for (int c = 0; c < cnt; ++c)
          ((double *)dto)[((size_t)e * kdirs + d0 + k) * cnt + c] = nan ? __builtin_nan("") : src[c * (K + 1) + 1 + k];
  }
};

template <class U, class B, int K>
int tds_query_jvp_host_impl(const typename U::Args &a) {
  using T = typename TdsQueryScalar<K>::type;
  const U u(a);
  TdsQueryDualHost<B, K> h(a.m, u.total(), a.v, a.kdirs, a.columns().nall);
  int any_bad = 0;
  for (h.e = 0; h.e < a.n; ++h.e)
    for (h.d0 = 0; h.d0 == 0 || h.d0 < a.kdirs; h.d0 += K ? K : 1) {
      h.nk = a.kdirs - h.d0 < K ? a.kdirs - h.d0 : K;
      u.inputs([&](int off, const double *src, int col, int cnt) { h.put(off, src, col, cnt); });
      tds_query_jvp_theta(a, h.P[0], h.e, h.d0, h.nk);
      const int bad = u.eval(TdsOverlayView<T, B>{&h.P[0]}, h.w);
      any_bad |= bad;
      u.outputs([&](void *o, void *dto, int off, int cnt, int nan) { h.get(o, dto, off, cnt, nan); }, bad);
    }
  return any_bad ? fail(TDS_ERR_INVALID_ARG, U::kNotPd) : TDS_OK;
}

// ---------------------------------------------------------------- entry points
// the checks every entry point shares, before the unit's own: first the required input of a record; out / dout NULL: no
// output of that kind (none), and no tangents without directions; any(o): whether an output set asks for anything
template <class Out, class Any>
int tds_query_jvp_check(const char *who, int n, const void *first, int p, const tds_param_t *params, int k, const void *v,
                        const Out *&out, const Out *&dout, Any any) {
  static const Out none = {};
  if (!out) out = &none;
  if (!dout || k == 0) dout = &none;
  if (!first || n < 1 || k < 0 || p < 0 || (p > 0 && !params) || (k > 0 && !v))
    return fail(TDS_ERR_INVALID_ARG, "%s: NULL or empty argument", who);
  if (!any(k > 0 ? dout : out)) return fail(TDS_ERR_INVALID_ARG, "%s: no output requested", who);
  return TDS_OK;
}

// a device entry point's body; args(model, &a): the unit's argument check, against the handle's host model.  a.what
// == 0: only outputs without extent are asked for (a contact query without contact points)
template <class U, class ArgsFn>
int tds_query_jvp_device(const char *who, tds_hip_sim_t *s, int p, const tds_param_t *params_host, int k, ArgsFn args) {
  if (!s) return fail(TDS_ERR_INVALID_ARG, "%s: NULL or empty argument", who);
  DeviceGuard guard(s->device);
  int cls, rc = tds_diff_prepare(s, &cls);
  if (rc) return rc;
  if ((rc = tds_param_check_sel(&s->model, p, params_host))) return rc;
  typename U::Args a;
  if ((rc = args(&s->model, &a))) return rc;
  if (!a.what) return TDS_OK;
  const int total = U(a).total();
  a.m = (const tds_model_t *)s->d_diff_model;
  return tds_with_bound(cls, [&](auto b) {
    using B = typename decltype(b)::type;
    return k ? tds_query_jvp_launch<U, B, U::template kTangents<B>>(s, a, total, params_host)
             : tds_query_jvp_launch<U, B, 0>(s, a, total, params_host);
  });
}

// ... and a host checker's
template <class U, class ArgsFn>
int tds_query_jvp_host(const char *who, const tds_model_t *model, int p, const tds_param_t *params, int k, ArgsFn args) {
  if (!model) return fail(TDS_ERR_INVALID_ARG, "%s: NULL or empty argument", who);
  int cls, rc = tds_param_host_prepare(model, p, params, &cls);
  if (rc) return rc;
  typename U::Args a;
  if ((rc = args(model, &a))) return rc;
  if (!a.what) return TDS_OK;
  return tds_with_bound(cls, [&](auto b) {
    using B = typename decltype(b)::type;
    return k ? tds_query_jvp_host_impl<U, B, kHostK>(a) : tds_query_jvp_host_impl<U, B, 0>(a);
  });
}

// ... and a _tangents entry point's: K of the model's class, or minus the error
template <class U>
int tds_query_jvp_tangents(const char *who, const tds_model_t *model) {
  if (!model) return -fail(TDS_ERR_INVALID_ARG, "%s: NULL model", who);
  int cls;
  if (const int rc = tds_diff_host_check(model, &cls)) return -rc;
  return tds_with_bound(cls, [&](auto b) { return U::template kTangents<typename decltype(b)::type>; });
}

}  // namespace
