// tds_jvp.hip — step Jacobians: forward-mode tangents of forward_zero (tds_diff_step.h over TdsDual<K>) on gfx950,
// the C ABI tds_hip_jvp / tds_hip_jacobian / tds_hip_jacobian_host (include/tds_hip.h).
//
// Mapping: one work item per (environment, block of K directions).  A lane evaluates the step once over TdsDual<K>:
// the value part is the primal (shared by the block's K tangents), tangent k is J v_k.  The per-lane arrays (the work
// object of tds_diff_step.h, the record in dual form) are indexed at run time; at tens of KB per lane they live in a
// device buffer of kJvpLanes work objects (TdsJvpLane) rather than in the private segment, and a launch of at most
// kJvpLanes lanes walks the items with the grid's stride.  Their size is set by the model class's bound (links, dofs,
// contact points, visuals) and K — see tds_jvp_pick() and DESIGN.md for the figures.
// This is a path of its own: the step kernels (general, 16-, 8-lane, serial chain) carry no tangents.
#include <hip/hip_runtime.h>
#include <string.h>

#include <vector>

#include "tds_diff_classes.h"

using namespace tds_internal;

namespace {

constexpr int kHostK = 8;  // tangents per evaluation on the host

// What a launch computes.  JVP: directions v[n][kdirs][input_dim], out = jv[n][kdirs][output_dim].  Jacobian: unit
// directions e_cols[c] (cols NULL: e_c), out = jac[n][n_rows][n_cols] at rows[r] (rows NULL: r).
struct TdsJvpArgs {
  const tds_model_t *m;
  int n, kdirs;
  const double *x, *v;
  const int *rows, *cols;
  int n_rows, n_cols;
  double *y, *out;
};

// a lane's work object: the record in dual form and the step's state (tens of KB: in a device buffer, not in the
// kernel's private segment)
template <class B, int K>
struct TdsJvpLane {
  TdsDual<K> x[B::NX], y[B::NY];
  TdsDiffWork<TdsDual<K>, B> w;
};

template <class B, int K>
__device__ inline void tds_jvp_item(const TdsJvpArgs &a, TdsJvpLane<B, K> &L, long long item) {
  using D = TdsDual<K>;
  const int env = (int)(item % a.n), blk = (int)(item / a.n);  // neighbouring lanes: neighbouring environments
  const tds_model_t *m = a.m;
  const int nin = m->input_dim, nout = m->output_dim, ny = tds_diff_ny(m);
  D *x = L.x, *y = L.y;
  TdsDiffWork<D, B> &w = L.w;
  const double *xe = a.x + (size_t)env * nin;
  for (int i = 0; i < nin; ++i) x[i] = D(xe[i]);
  for (int k = 0; k < K; ++k) {
    const int dir = blk * K + k;
    if (dir >= a.kdirs) break;
    if (a.v) {
      const double *ve = a.v + ((size_t)env * a.kdirs + dir) * nin;
      for (int i = 0; i < nin; ++i) x[i].d[k] = ve[i];
    } else {
      const int c = a.cols ? a.cols[dir] : dir;
      x[c].d[k] = 1.0;
    }
  }
  const int rc = tds_diff_step(m, w, x, y);
  const double bad = rc ? __builtin_nan("") : 0.0;  // M not positive definite: the environment's outputs are NaN
  if (a.y && blk == 0) {
    double *ye = a.y + (size_t)env * nout;
    for (int i = 0; i < nout; ++i) ye[i] = (i < ny ? y[i].v : 0.0) + bad;
  }
  for (int k = 0; k < K; ++k) {
    const int dir = blk * K + k;
    if (dir >= a.kdirs) break;
    if (a.v) {
      double *o = a.out + ((size_t)env * a.kdirs + dir) * nout;
      for (int i = 0; i < nout; ++i) o[i] = (i < ny ? y[i].d[k] : 0.0) + bad;
    } else {
      double *o = a.out + (size_t)env * a.n_rows * a.n_cols + dir;
      for (int r = 0; r < a.n_rows; ++r) {
        const int row = a.rows ? a.rows[r] : r;
        o[(size_t)r * a.n_cols] = (row < ny ? y[row].d[k] : 0.0) + bad;
      }
    }
  }
}


template <class B, int K>
__global__ void __launch_bounds__(64) tds_jvp_kernel(TdsJvpArgs a, TdsJvpLane<B, K> *lanes, long long n_lanes) {
  const long long lane = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= n_lanes) return;
  const long long items = (long long)a.n * ((a.kdirs + K - 1) / K);
  for (long long it = lane; it < items; it += n_lanes) tds_jvp_item<B, K>(a, lanes[lane], it);
}
// out[j] = sum over environments of per_env[i][j] in environment order (the emitter's host loop,
// cuda_codegen.hpp:218-228), / n for MEAN
__global__ void tds_jac_accumulate(const double *per_env, int n, long long len, int mean, double *out) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= len) return;
  double s = per_env[j];
  for (int i = 1; i < n; ++i) s += per_env[(size_t)i * len + j];
  out[j] = mean ? s / n : s;
}

// bytes of the lanes' work objects of such a launch
template <class B>
size_t tds_jvp_ws_bytes(int n, int kdirs) {
  return ((size_t)tds_jvp_lanes<B>(n, kdirs) * sizeof(TdsJvpLane<B, TdsJvpK<B>::K>) + 255) & ~(size_t)255;
}

template <class B>
int tds_jvp_launch(tds_hip_sim *s, const TdsJvpArgs &a, void *ws) {
  constexpr int K = TdsJvpK<B>::K;
  const long long n_lanes = tds_jvp_lanes<B>(a.n, a.kdirs);
  const int threads = 64;
  const unsigned blocks = (unsigned)((n_lanes + threads - 1) / threads);
  hipLaunchKernelGGL((tds_jvp_kernel<B, K>), dim3(blocks), dim3(threads), 0, s->stream, a, (TdsJvpLane<B, K> *)ws,
                     n_lanes);
  TDS_HIP_TRY(hipGetLastError());
  return TDS_OK;
}

size_t tds_jvp_ws(int cls, int n, int kdirs) {
  return tds_with_bound(cls, [&](auto b) { return tds_jvp_ws_bytes<typename decltype(b)::type>(n, kdirs); });
}

int tds_jvp_dispatch(tds_hip_sim *s, int cls, const TdsJvpArgs &a) {
  void *ws = s->d_diff_tmp;  // the lanes' work objects lie at the front of the work buffer
  return tds_with_bound(cls, [&](auto b) { return tds_jvp_launch<typename decltype(b)::type>(s, a, ws); });
}

int tds_jac_check_sel(const tds_model_t *m, int n_rows, const int *rows, int n_cols, const int *cols) {
  for (int r = 0; rows && r < n_rows; ++r)
    if (rows[r] < 0 || rows[r] >= m->output_dim) return fail(TDS_ERR_INVALID_ARG, "step Jacobians: row index out of range%s");
  for (int c = 0; cols && c < n_cols; ++c)
    if (cols[c] < 0 || cols[c] >= m->input_dim) return fail(TDS_ERR_INVALID_ARG, "step Jacobians: column index out of range%s");
  if (n_rows <= 0 || n_cols <= 0) return fail(TDS_ERR_INVALID_ARG, "step Jacobians: empty row or column selection%s");
  return TDS_OK;
}

// the host instantiation: y (double step) and jac for environments [0, n)
template <class B>
int tds_jac_host_impl(const tds_model_t *m, int n, const double *x, int n_rows, const int *rows, int n_cols,
                      const int *cols, double *y, double *jac /* [n][n_rows][n_cols] */) {
  using D = TdsDual<kHostK>;
  const int nin = m->input_dim, nout = m->output_dim, ny = tds_diff_ny(m);
  std::vector<TdsDiffWork<double, B>> w64(1);
  std::vector<TdsDiffWork<D, B>> wd(1);
  std::vector<double> y64(B::NY);
  std::vector<D> xd(B::NX), yd(B::NY);
  int bad = 0;
  for (int e = 0; e < n; ++e) {
    const double *xe = x + (size_t)e * nin;
    if (y) {
      if (tds_diff_step(m, w64[0], xe, y64.data())) bad = 1;
      for (int i = 0; i < nout; ++i) y[(size_t)e * nout + i] = i < ny ? y64[i] : 0.0;
    }
    for (int c0 = 0; jac && c0 < n_cols; c0 += kHostK) {
      for (int i = 0; i < nin; ++i) xd[i] = D(xe[i]);
      for (int k = 0; k < kHostK && c0 + k < n_cols; ++k) xd[cols ? cols[c0 + k] : c0 + k].d[k] = 1.0;
      if (tds_diff_step(m, wd[0], xd.data(), yd.data())) bad = 1;
      for (int k = 0; k < kHostK && c0 + k < n_cols; ++k)
        for (int r = 0; r < n_rows; ++r) {
          const int row = rows ? rows[r] : r;
          jac[((size_t)e * n_rows + r) * n_cols + c0 + k] = row < ny ? yd[row].d[k] : 0.0;
        }
    }
  }
  return bad ? fail(TDS_ERR_INVALID_ARG, "step Jacobians: joint-space inertia not positive definite%s") : TDS_OK;
}

}  // namespace

namespace tds_internal {

// the work buffer holds at least `need` bytes.  Launches on the handle's stream use it one after the other; only a
// buffer that has to grow is replaced, after the host waits for the earlier calls on the stream.
int tds_work_buffer(tds_hip_sim *s, size_t need) {
  if (need > s->diff_tmp_bytes) {
    TDS_HIP_TRY(hipStreamSynchronize(s->stream));
    if (s->d_diff_tmp) TDS_HIP_TRY(hipFree(s->d_diff_tmp));
    s->d_diff_tmp = nullptr, s->diff_tmp_bytes = 0;
    TDS_HIP_TRY(hipMalloc(&s->d_diff_tmp, need));
    s->diff_tmp_bytes = need;
  }
  return TDS_OK;
}

// the handle's checks and its device copy of the model blob
int tds_diff_prepare(tds_hip_sim *s, int *cls) {
  if (s->dtype != TDS_DTYPE_F64) return fail(TDS_ERR_UNSUPPORTED, "step Jacobians: f64 handles only%s");
  const char *why = "";
  *cls = tds_jvp_pick(&s->model, &why);
  if (*cls < 0) return fail(TDS_ERR_UNSUPPORTED, "%s", why);
  if (!s->d_diff_model) {
    TDS_HIP_TRY(hipMalloc(&s->d_diff_model, sizeof(tds_model_t)));
    TDS_HIP_TRY(hipMemcpy(s->d_diff_model, &s->model, sizeof(tds_model_t), hipMemcpyHostToDevice));
  }
  return TDS_OK;
}

}  // namespace tds_internal

extern "C" {

int tds_hip_jvp(tds_hip_sim_t *s, int n, const void *x_dev, int k, const void *v_dev, void *y_dev, void *jv_dev) {
  if (!s || !x_dev || !v_dev || !jv_dev || n < 1 || k < 1) return fail(TDS_ERR_INVALID_ARG, "tds_hip_jvp: NULL or empty argument%s");
  DeviceGuard guard(s->device);
  int cls, rc = tds_diff_prepare(s, &cls);
  if (rc) return rc;
  if ((rc = tds_work_buffer(s, tds_jvp_ws(cls, n, k)))) return rc;
  TdsJvpArgs a = {(const tds_model_t *)s->d_diff_model, n, k, (const double *)x_dev, (const double *)v_dev,
                  nullptr, nullptr, 0, 0, (double *)y_dev, (double *)jv_dev};
  return tds_jvp_dispatch(s, cls, a);
}

int tds_hip_jacobian(tds_hip_sim_t *s, int n, const void *x_dev, int n_rows, const int *rows_host, int n_cols,
                     const int *cols_host, int accumulate, void *y_dev, void *jac_dev) {
  if (!s || !x_dev || !jac_dev || n < 1) return fail(TDS_ERR_INVALID_ARG, "tds_hip_jacobian: NULL or empty argument%s");
  if (accumulate < TDS_JAC_ACCUMULATE_NONE || accumulate > TDS_JAC_ACCUMULATE_MEAN)
    return fail(TDS_ERR_INVALID_ARG, "tds_hip_jacobian: unknown accumulation method%s");
  DeviceGuard guard(s->device);
  int cls, rc = tds_diff_prepare(s, &cls);
  if (rc) return rc;
  if (!rows_host) n_rows = s->model.output_dim;
  if (!cols_host) n_cols = s->model.input_dim;
  if ((rc = tds_jac_check_sel(&s->model, n_rows, rows_host, n_cols, cols_host))) return rc;
  // work buffer: the lanes' work objects | rows | cols | (accumulated launches) the per-environment Jacobians
  const size_t ws = tds_jvp_ws(cls, n, n_cols);
  const size_t sel_bytes = ((size_t)(n_rows + n_cols) * sizeof(int) + 255) & ~(size_t)255;
  const size_t per_env = (size_t)n * n_rows * n_cols;
  if ((rc = tds_work_buffer(s, ws + sel_bytes + (accumulate ? per_env * sizeof(double) : 0)))) return rc;
  int *d_rows = (int *)((char *)s->d_diff_tmp + ws), *d_cols = d_rows + n_rows;
  // a selection is copied with a blocking copy: earlier calls on the stream may still read the previous one
  if (rows_host || cols_host) TDS_HIP_TRY(hipStreamSynchronize(s->stream));
  if (rows_host) TDS_HIP_TRY(hipMemcpy(d_rows, rows_host, sizeof(int) * n_rows, hipMemcpyHostToDevice));
  if (cols_host) TDS_HIP_TRY(hipMemcpy(d_cols, cols_host, sizeof(int) * n_cols, hipMemcpyHostToDevice));
  double *out = accumulate ? (double *)((char *)s->d_diff_tmp + ws + sel_bytes) : (double *)jac_dev;
  TdsJvpArgs a = {(const tds_model_t *)s->d_diff_model, n, n_cols, (const double *)x_dev, nullptr,
                  rows_host ? d_rows : nullptr, cols_host ? d_cols : nullptr, n_rows, n_cols, (double *)y_dev, out};
  if ((rc = tds_jvp_dispatch(s, cls, a))) return rc;
  if (accumulate) {
    const long long len = (long long)n_rows * n_cols;
    hipLaunchKernelGGL(tds_jac_accumulate, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, s->stream, out, n, len,
                       accumulate == TDS_JAC_ACCUMULATE_MEAN ? 1 : 0, (double *)jac_dev);
    TDS_HIP_TRY(hipGetLastError());
  }
  return TDS_OK;
}

int tds_hip_jacobian_host(const tds_model_t *model, int n, const double *x, int n_rows, const int *rows, int n_cols,
                          const int *cols, int accumulate, double *y, double *jac) {
  if (!model || !x || n < 1 || (!y && !jac)) return fail(TDS_ERR_INVALID_ARG, "tds_hip_jacobian_host: NULL or empty argument%s");
  if (accumulate < TDS_JAC_ACCUMULATE_NONE || accumulate > TDS_JAC_ACCUMULATE_MEAN)
    return fail(TDS_ERR_INVALID_ARG, "tds_hip_jacobian_host: unknown accumulation method%s");
  int cls, rc = tds_diff_host_check(model, &cls);
  if (rc) return rc;
  if (!rows) n_rows = model->output_dim;
  if (!cols) n_cols = model->input_dim;
  if (jac && (rc = tds_jac_check_sel(model, n_rows, rows, n_cols, cols))) return rc;
  std::vector<double> per_env;
  double *dst = jac;
  if (jac && accumulate) {
    per_env.resize((size_t)n * n_rows * n_cols);
    dst = per_env.data();
  }
  rc = tds_with_bound(cls, [&](auto b) {
    return tds_jac_host_impl<typename decltype(b)::type>(model, n, x, n_rows, rows, n_cols, cols, y, dst);
  });
  if (rc || !jac || !accumulate) return rc;
  const size_t len = (size_t)n_rows * n_cols;
  for (size_t j = 0; j < len; ++j) {
    double s = per_env[j];
    for (int i = 1; i < n; ++i) s += per_env[(size_t)i * len + j];
    jac[j] = accumulate == TDS_JAC_ACCUMULATE_MEAN ? s / n : s;
  }
  return TDS_OK;
}

int tds_hip_jacobian_tangents(const tds_model_t *model) {
  const char *why = "";
  const int cls = tds_jvp_pick(model, &why);
  if (cls < 0) return fail(0, "%s", why);
  return tds_with_bound(cls, [](auto b) { return TdsJvpK<typename decltype(b)::type>::K; });
}

}  // extern "C"
