// tds_dparam.hip — parameter derivatives: the step derivatives in [x | theta] on gfx950, theta the model scalars a
// selection tds_param_t[p] names (include/tds_hip.h), per environment.  C ABI tds_hip_params_get,
// tds_hip_jvp_params, tds_hip_vjp_params and their host checkers.
//
// The step (tds_diff_step_view) reads the selectable parameters through a TdsParamOverlay: T-typed copies of the
// blob's values, the selected entries replaced by active theta.  The overlay is part of the lane's work object, in the
// handle's work buffer (a private-segment work object aborted on its first launch: DESIGN 7a).
//   forward mode: one work item per (environment, block of K directions over [x | theta]), as tds_jvp.hip's kernel;
//   reverse mode: the recording and sweep kernels of tds_vjp_kernels.h over TdsVjpParamLane: theta is variables
//                 input_dim .. input_dim + p - 1, the tape starts after them.
// With p = 0 the device entry points call the plain paths (tds_hip_jvp, tds_hip_vjp); k = 0 in forward mode computes
// y at theta only, with the double step over an overlay of doubles (tds_param_y_kernel).
#include <hip/hip_runtime.h>
#include <string.h>

#include "tds_vjp_param.h"

namespace {

// jv of the directions d0 .. of environment env; `bad`: NaN
template <class B, int K>
TDS_HD inline void tds_jvp_param_store(const TdsJvpParamArgs &a, const TdsJvpParamLane<B, K> &L, int env, int d0,
                                       double bad) {
  const int nout = a.m->output_dim, ny = tds_diff_ny(a.m);
  for (int k = 0; k < K && d0 + k < a.kdirs; ++k) {
    double *o = a.out + ((size_t)env * a.kdirs + d0 + k) * nout;
    for (int i = 0; i < nout; ++i) o[i] = (i < ny ? L.y[i].d[k] : 0.0) + bad;
  }
}

template <class B, int K>
__global__ void __launch_bounds__(64) tds_jvp_param_kernel(TdsJvpParamArgs a, TdsJvpParamLane<B, K> *lanes,
                                                           long long n_lanes) {
  const long long lane = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= n_lanes) return;
  const int blocks = a.kdirs > 0 ? (a.kdirs + K - 1) / K : 1;
  const long long items = (long long)a.n * blocks;
  TdsJvpParamLane<B, K> &L = lanes[lane];
  for (long long it = lane; it < items; it += n_lanes) {
    const int env = (int)(it % a.n), blk = (int)(it / a.n);  // neighbouring lanes: neighbouring environments
    const int rc = tds_jvp_param_eval<B, K>(a, L, env, blk * K);
    const double bad = rc ? __builtin_nan("") : 0.0;  // M not positive definite: the environment's outputs are NaN
    if (a.y && blk == 0) {
      const int nout = a.m->output_dim, ny = tds_diff_ny(a.m);
      double *ye = a.y + (size_t)env * nout;
      for (int i = 0; i < nout; ++i) ye[i] = (i < ny ? L.y[i].v : 0.0) + bad;
    }
    tds_jvp_param_store<B, K>(a, L, env, blk * K, bad);
  }
}

// bytes of the lanes' work objects of a launch over n environments x kdirs directions (kdirs = 0: one block)
template <class B>
size_t tds_jvp_param_ws_bytes(int n, int kdirs) {
  return ((size_t)tds_jvp_lanes<B>(n, kdirs > 0 ? kdirs : 1) * sizeof(TdsJvpParamLane<B, TdsJvpK<B>::K>) + 255) &
         ~(size_t)255;
}

template <class B>
int tds_jvp_param_launch(tds_hip_sim *s, const TdsJvpParamArgs &a, void *ws) {
  constexpr int K = TdsJvpK<B>::K;
  const long long n_lanes = tds_jvp_lanes<B>(a.n, a.kdirs > 0 ? a.kdirs : 1);
  const int threads = 64;
  const unsigned blocks = (unsigned)((n_lanes + threads - 1) / threads);
  hipLaunchKernelGGL((tds_jvp_param_kernel<B, K>), dim3(blocks), dim3(threads), 0, s->stream, a,
                     (TdsJvpParamLane<B, K> *)ws, n_lanes);
  TDS_HIP_TRY(hipGetLastError());
  return TDS_OK;
}

// y of environment env into ye (NaN where M is not positive definite); 0 or the step's -1
template <class B>
TDS_HD inline int tds_param_y_eval(const TdsJvpParamArgs &a, TdsParamYLane<B> &L, int env, double *ye) {
  const tds_model_t *m = a.m;
  const int nout = m->output_dim, ny = tds_diff_ny(m);
  tds_param_seed(m, L.P);
  for (int j = 0; j < a.p; ++j) tds_param_set(L.P, a.params[j], a.theta[(size_t)env * a.p + j]);
  const int rc = tds_diff_step_view(m, TdsOverlayView<double, B>{&L.P}, L.w, a.x + (size_t)env * m->input_dim, L.y);
  const double bad = rc ? __builtin_nan("") : 0.0;
  for (int i = 0; i < nout; ++i) ye[i] = (i < ny ? L.y[i] : 0.0) + bad;
  return rc;
}

// one lane per environment, at most kJvpLanes lanes walking the environments with the grid's stride
template <class B>
__global__ void __launch_bounds__(64) tds_param_y_kernel(TdsJvpParamArgs a, TdsParamYLane<B> *lanes, long long n_lanes) {
  const long long lane = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= n_lanes) return;
  for (long long env = lane; env < a.n; env += n_lanes)
    tds_param_y_eval<B>(a, lanes[lane], (int)env, a.y + (size_t)env * a.m->output_dim);
}

long long tds_param_y_lanes(int n) { return n < kJvpLanes ? n : kJvpLanes; }

template <class B>
size_t tds_param_y_ws_bytes(int n) {
  return ((size_t)tds_param_y_lanes(n) * sizeof(TdsParamYLane<B>) + 255) & ~(size_t)255;
}

template <class B>
int tds_param_y_launch(tds_hip_sim *s, const TdsJvpParamArgs &a, void *ws) {
  const long long n_lanes = tds_param_y_lanes(a.n);
  const unsigned blocks = (unsigned)((n_lanes + 63) / 64);
  hipLaunchKernelGGL((tds_param_y_kernel<B>), dim3(blocks), dim3(64), 0, s->stream, a, (TdsParamYLane<B> *)ws, n_lanes);
  TDS_HIP_TRY(hipGetLastError());
  return TDS_OK;
}

// the host instantiation: y from the double step over an overlay of doubles, jv from TdsDual<kHostK>
template <class B>
int tds_jvp_param_host_impl(const TdsJvpParamArgs &a) {
  const int nout = a.m->output_dim;
  std::vector<TdsJvpParamLane<B, kHostK>> L(1);
  std::vector<TdsParamYLane<B>> Ly(1);
  int bad = 0;
  for (int e = 0; e < a.n; ++e) {
    if (a.y) bad |= tds_param_y_eval<B>(a, Ly[0], e, a.y + (size_t)e * nout) != 0;
    for (int d0 = 0; d0 < a.kdirs; d0 += kHostK) {
      const int rc = tds_jvp_param_eval<B, kHostK>(a, L[0], e, d0);
      bad |= rc != 0;
      tds_jvp_param_store<B, kHostK>(a, L[0], e, d0, rc ? __builtin_nan("") : 0.0);
    }
  }
  return bad ? fail(TDS_ERR_INVALID_ARG, "step Jacobians: joint-space inertia not positive definite%s") : TDS_OK;
}

template <class B>
int tds_vjp_param_launch(tds_hip_sim *s, TdsVjpParamArgs a, const tds_param_t *params_host) {
  const long long n_lanes = tds_vjp_lanes(a.n);
  const size_t sel = (size_t)a.p * sizeof(tds_param_t);
  const TdsVjpLayout<TdsVjpParamLane<B>> lay(n_lanes, s->model.input_dim + a.p, sel);
  int rc = tds_work_buffer(s, lay.total);
  if (rc) return rc;
  // the selection after the overflow flag's slot, copied with a blocking copy: earlier calls on the stream may still
  // read the work buffer
  tds_param_t *d_sel = (tds_param_t *)((char *)s->d_diff_tmp + 256);
  TDS_HIP_TRY(hipStreamSynchronize(s->stream));
  TDS_HIP_TRY(hipMemcpy(d_sel, params_host, sel, hipMemcpyHostToDevice));
  a.params = d_sel;
  return tds_vjp_run(s, a, lay, n_lanes);
}

}  // namespace

extern "C" {

int tds_hip_params_get(const tds_model_t *model, int p, const tds_param_t *params, double *theta) {
  if (!model || (p > 0 && !theta)) return fail(TDS_ERR_INVALID_ARG, "tds_hip_params_get: NULL argument%s");
  int rc = tds_hip_model_check(model);
  if (rc) return rc;
  if ((rc = tds_param_check_sel(model, p, params))) return rc;
  for (int j = 0; j < p; ++j) theta[j] = tds_param_value(model, params[j]);
  return TDS_OK;
}

int tds_hip_jvp_params(tds_hip_sim_t *s, int n, const void *x_dev, int p, const tds_param_t *params_host,
                       const void *theta_dev, int k, const void *v_dev, void *y_dev, void *jv_dev) {
  if (!s || !x_dev || n < 1 || k < 0 || p < 0 || (p > 0 && (!params_host || !theta_dev)) ||
      (k > 0 && (!v_dev || !jv_dev)) || (k == 0 && !y_dev))
    return fail(TDS_ERR_INVALID_ARG, "tds_hip_jvp_params: NULL or empty argument%s");
  if (p == 0 && k > 0) return tds_hip_jvp(s, n, x_dev, k, v_dev, y_dev, jv_dev);  // the plain path
  DeviceGuard guard(s->device);
  int cls, rc = tds_diff_prepare(s, &cls);
  if (rc) return rc;
  if ((rc = tds_param_check_sel(&s->model, p, params_host))) return rc;
  // work buffer: the lanes' work objects (k = 0: of the double step) | the selection
  const size_t ws = tds_with_bound(cls, [&](auto b) {
    using B = typename decltype(b)::type;
    return k ? tds_jvp_param_ws_bytes<B>(n, k) : tds_param_y_ws_bytes<B>(n);
  });
  const size_t sel = (size_t)p * sizeof(tds_param_t);
  if ((rc = tds_work_buffer(s, ws + sel))) return rc;
  tds_param_t *d_sel = (tds_param_t *)((char *)s->d_diff_tmp + ws);
  if (p > 0) {  // a blocking copy: earlier calls on the stream may still read the work buffer
    TDS_HIP_TRY(hipStreamSynchronize(s->stream));
    TDS_HIP_TRY(hipMemcpy(d_sel, params_host, sel, hipMemcpyHostToDevice));
  }
  const TdsJvpParamArgs a = {(const tds_model_t *)s->d_diff_model, n, k, p, (const double *)x_dev,
                             (const double *)theta_dev, (const double *)v_dev, d_sel, (double *)y_dev,
                             (double *)jv_dev};
  if (k == 0)  // y only: the double step
    return tds_with_bound(cls, [&](auto b) {
      return tds_param_y_launch<typename decltype(b)::type>(s, a, s->d_diff_tmp);
    });
  return tds_with_bound(cls, [&](auto b) {
    return tds_jvp_param_launch<typename decltype(b)::type>(s, a, s->d_diff_tmp);
  });
}

int tds_hip_vjp_params(tds_hip_sim_t *s, int n, const void *x_dev, int p, const tds_param_t *params_host,
                       const void *theta_dev, int k, const void *w_dev, void *y_dev, void *wj_dev) {
  if (!s || !x_dev || !w_dev || !wj_dev || n < 1 || k < 1 || p < 0 || (p > 0 && (!params_host || !theta_dev)))
    return fail(TDS_ERR_INVALID_ARG, "tds_hip_vjp_params: NULL or empty argument%s");
  if (p == 0) return tds_hip_vjp(s, n, x_dev, k, w_dev, y_dev, wj_dev);  // the plain path
  DeviceGuard guard(s->device);
  int cls, rc = tds_diff_prepare(s, &cls);
  if (rc) return rc;
  if ((rc = tds_param_check_sel(&s->model, p, params_host))) return rc;
  TdsVjpParamArgs a;
  static_cast<TdsVjpArgs &>(a) = {(const tds_model_t *)s->d_diff_model, n, k, (const double *)x_dev,
                                  (const double *)w_dev, (double *)y_dev, (double *)wj_dev, nullptr};
  a.p = p, a.params = nullptr, a.theta = (const double *)theta_dev;
  return tds_with_bound(cls, [&](auto b) {
    return tds_vjp_param_launch<typename decltype(b)::type>(s, a, params_host);
  });
}

int tds_hip_jvp_params_host(const tds_model_t *model, int n, const double *x, int p, const tds_param_t *params,
                            const double *theta, int k, const double *v, double *y, double *jv) {
  if (!model || !x || n < 1 || k < 0 || p < 0 || (p > 0 && (!params || !theta)) || (k > 0 && (!v || !jv)) ||
      (k == 0 && !y))
    return fail(TDS_ERR_INVALID_ARG, "tds_hip_jvp_params_host: NULL or empty argument%s");
  int cls, rc = tds_param_host_prepare(model, p, params, &cls);
  if (rc) return rc;
  const TdsJvpParamArgs a = {model, n, k, p, x, theta, v, params, y, jv};
  return tds_with_bound(cls, [&](auto b) { return tds_jvp_param_host_impl<typename decltype(b)::type>(a); });
}

int tds_hip_vjp_params_host(const tds_model_t *model, int n, const double *x, int p, const tds_param_t *params,
                            const double *theta, int k, const double *w, double *y, double *wj, int tape_cap,
                            int *tape_len) {
  if (!model || !x || !w || !wj || n < 1 || k < 1 || p < 0 || (p > 0 && (!params || !theta)))
    return fail(TDS_ERR_INVALID_ARG, "tds_hip_vjp_params_host: NULL or empty argument%s");
  int cls, rc = tds_param_host_prepare(model, p, params, &cls);
  if (rc) return rc;
  TdsVjpParamArgs a;
  static_cast<TdsVjpArgs &>(a) = {model, n, k, x, w, y, wj, nullptr};
  a.p = p, a.params = params, a.theta = theta;
  return tds_with_bound(cls, [&](auto b) {
    return tds_vjp_host_run<TdsVjpParamLane<typename decltype(b)::type>>(a, tape_cap, tape_len);
  });
}

}  // extern "C"
