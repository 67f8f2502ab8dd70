// tds_lqr.hip — batched iLQR on gfx950: the Riccati backward pass of n time-varying LQ problems as ONE launch, and the
// closed-loop rollout under time-varying affine feedback around the handle's forward_zero launch.  C ABI
// tds_hip_lqr_backward / tds_hip_feedback_rollout and their _host checkers (include/tds_hip.h); the statement is
// tds_lqr.h's.
//
// Backward pass: one wavefront (a workgroup of 64 lanes) per problem, the whole recursion in its LDS workspace
// (tds_lqr.h: 79248 bytes at nx = 40, nu = 16, two problems per compute unit).  The chain is T dependent steps; what
// step t - 1 reads from HBM (A, B, lxx, lux, luu, lx, lu) is requested into registers before step t's products are
// formed and stored to LDS after them, so no step waits on memory.  The registers are arrays of constant extent, walked
// by unrolled loops: the private segment holds nothing indexed at run time.  Two builds, by the bound of the dimensions
// (28 x 8: the Ant and below; 40 x 16), differ only in those extents.
//
// Feedback rollout: per step one small kernel (a lane per entry of a row's record) that takes s_t from the step's
// output, forms u_t (a lane's sequential sum), assembles the next record and stores s_t, u_t; then the step kernel over
// the records, num_envs rows at a time.  Records and outputs live in the handle's work buffer.
#include <hip/hip_runtime.h>
#include <string.h>

#include <atomic>
#include <vector>

#include "tds_diff_classes.h"
#include "tds_lqr.h"

using namespace tds_internal;

namespace {

struct TdsLqrArgs {
  int n, T, nx, nu;
  const double *A, *B, *lx, *lu, *lxx, *luu, *lux, *mu;
  double *k, *K, *dv;
  int *status;
};
// the box build's: bounds on the step k_t [n][T][nu], the QP's final clamped set and iteration count [n][T]
struct TdsLqrBoxArgs : TdsLqrArgs {
  const double *dlo, *dhi;
  int *clamped, *qp_iterations;
};

struct TdsLqrBarrier {
  __device__ void operator()() const { __syncthreads(); }
};
struct TdsLqrNoSync {
  void operator()() const {}
};

// a step's operands on their way from HBM to LDS: element lane + 64 j of each array in slot j
template <int NXM, int NUM, bool BOX>
struct TdsLqrRegs {
  static constexpr int CA = (NXM * NXM + 63) / 64, CB = (NXM * NUM + 63) / 64, CU = (NUM * NUM + 63) / 64;
  double A[CA], lxx[CA], B[CB], lux[CB], luu[CU], lx, lu;
  double dlo, dhi;  // BOX only

  template <class Args>
  __device__ __attribute__((always_inline)) void load(const Args &a, size_t p, int t, int lane) {
    const int nx = a.nx, nu = a.nu;
    const size_t pt = p * a.T + t;
    const double *Ag = a.A + pt * nx * nx, *Bg = a.B + pt * nx * nu, *lxxg = a.lxx + (p * (a.T + 1) + t) * nx * nx;
    const double *luxg = a.lux + pt * nu * nx, *luug = a.luu + pt * nu * nu;
#pragma unroll
    for (int j = 0; j < CA; ++j) {
      const int e = lane + 64 * j;
      if (e < nx * nx) A[j] = Ag[e], lxx[j] = lxxg[e];
    }
#pragma unroll
    for (int j = 0; j < CB; ++j) {
      const int e = lane + 64 * j;
      if (e < nx * nu) B[j] = Bg[e], lux[j] = luxg[e];
    }
#pragma unroll
    for (int j = 0; j < CU; ++j) {
      const int e = lane + 64 * j;
      if (e < nu * nu) luu[j] = luug[e];
    }
    if (lane < nx) lx = a.lx[(p * (a.T + 1) + t) * nx + lane];
    if (lane < nu) lu = a.lu[pt * nu + lane];
    if constexpr (BOX) {
      if (lane < nu) dlo = a.dlo[pt * nu + lane], dhi = a.dhi[pt * nu + lane];
    }
  }

  __device__ __attribute__((always_inline)) void store(const TdsLqrWs &w, int lane) const {
    const int nx = w.nx, nu = w.nu;
#pragma unroll
    for (int j = 0; j < CA; ++j) {
      const int e = lane + 64 * j;
      if (e < nx * nx) {
        const int r = e / nx, o = r * w.sx + (e - r * nx);
        w.A[o] = A[j], w.Qxx[o] = lxx[j];
      }
    }
#pragma unroll
    for (int j = 0; j < CB; ++j) {
      const int e = lane + 64 * j;
      if (e < nx * nu) {
        const int r = e / nu, c = e - r * nu;  // B [nx][nu]
        w.B[r * w.su + c] = B[j];
        const int a = e / nx, x = e - a * nx;  // lux [nu][nx]
        w.Qux[a * w.sx + x] = lux[j];
      }
    }
#pragma unroll
    for (int j = 0; j < CU; ++j) {
      const int e = lane + 64 * j;
      if (e < nu * nu) {
        const int r = e / nu;
        w.Quu[r * w.su + (e - r * nu)] = luu[j];
      }
    }
    if (lane < nx) w.Qx[lane] = lx;
    if (lane < nu) w.Qu[lane] = lu;
    if constexpr (BOX) {
      if (lane < nu) w.dlo[lane] = dlo, w.dhi[lane] = dhi;
    }
  }
};

template <int NXM, int NUM>
__global__ void __launch_bounds__(64) tds_lqr_kernel(TdsLqrArgs a) {
  extern __shared__ double tds_lqr_lds[];
  const int lane = threadIdx.x, nx = a.nx, nu = a.nu, T = a.T;
  const size_t p = blockIdx.x;
  const TdsLqrWs w = tds_lqr_ws(tds_lqr_lds, nx, nu);
  const double mu = a.mu[p];
  {  // the terminal cost
    const double *lxxT = a.lxx + (p * (T + 1) + T) * nx * nx;
    for (int e = lane; e < nx * nx; e += 64) {
      const int r = e / nx;
      w.V[r * w.sx + (e - r * nx)] = lxxT[e];
    }
    if (lane < nx) w.Vx[lane] = a.lx[(p * (T + 1) + T) * nx + lane];
    if (lane < 2) w.dv[lane] = 0.0;
  }
  TdsLqrRegs<NXM, NUM, false> r;
  r.load(a, p, T - 1, lane);
  r.store(w, lane);
  __syncthreads();
  double *kp = a.k + p * T * nu, *Kp = a.K + p * T * nu * nx;
  int failed = 0;
  for (int t = T - 1; t >= 0; --t) {
    if (t > 0) r.load(a, p, t - 1, lane);  // in flight while this step's products are formed
    if (tds_lqr_step(w, mu, lane, 64, TdsLqrBarrier{})) {
      failed = t + 1;
      break;
    }
    for (int e = lane; e < nu * nx; e += 64) {
      const int c = e / nx;
      Kp[(size_t)t * nu * nx + e] = w.K[c * w.sx + (e - c * nx)];
    }
    if (lane < nu) kp[(size_t)t * nu + lane] = w.k[lane];
    if (t > 0) r.store(w, lane);
    __syncthreads();
  }
  if (failed) {  // the nominal rollout: no gains at any step, nothing expected
    for (size_t e = lane; e < (size_t)T * nu * nx; e += 64) Kp[e] = 0.0;
    for (size_t e = lane; e < (size_t)T * nu; e += 64) kp[e] = 0.0;
  }
  if (lane < 2) a.dv[p * 2 + lane] = failed ? 0.0 : w.dv[lane];
  if (lane == 0) a.status[p] = failed;
}

// The build under control limits: tds_lqr_kernel with the box layout of the workspace, the step's bounds in the
// prefetch, tds_lqr_step<true> (tds_lqr.h: the box QP in place of the unconstrained solve) and the QP's set and
// iteration count stored per step.  (A kernel of its own, not a further parameter of tds_lqr_kernel: the plain
// builds keep their names and, instruction for instruction, their code.)
template <int NXM, int NUM>
__global__ void __launch_bounds__(64) tds_lqr_box_kernel(TdsLqrBoxArgs a) {
  extern __shared__ double tds_lqr_lds[];
  const int lane = threadIdx.x, nx = a.nx, nu = a.nu, T = a.T;
  const size_t p = blockIdx.x;
  const TdsLqrWs w = tds_lqr_ws(tds_lqr_lds, nx, nu, true);
  const double mu = a.mu[p];
  {  // the terminal cost
    const double *lxxT = a.lxx + (p * (T + 1) + T) * nx * nx;
    for (int e = lane; e < nx * nx; e += 64) {
      const int r = e / nx;
      w.V[r * w.sx + (e - r * nx)] = lxxT[e];
    }
    if (lane < nx) w.Vx[lane] = a.lx[(p * (T + 1) + T) * nx + lane];
    if (lane < 2) w.dv[lane] = 0.0;
    if (lane < nu) w.k[lane] = 0.0;  // the QP's start at the last step
  }
  TdsLqrRegs<NXM, NUM, true> r;
  r.load(a, p, T - 1, lane);
  r.store(w, lane);
  __syncthreads();
  double *kp = a.k + p * T * nu, *Kp = a.K + p * T * nu * nx;
  int failed = 0;
  for (int t = T - 1; t >= 0; --t) {
    if (t > 0) r.load(a, p, t - 1, lane);  // in flight while this step's products are formed
    unsigned set = 0;
    int iters = 0;
    if (tds_lqr_step<true>(w, mu, lane, 64, TdsLqrBarrier{}, &set, &iters)) {
      failed = t + 1;
      break;
    }
    if (lane == 0) a.clamped[p * T + t] = (int)set, a.qp_iterations[p * T + t] = iters;
    for (int e = lane; e < nu * nx; e += 64) {
      const int c = e / nx;
      Kp[(size_t)t * nu * nx + e] = w.K[c * w.sx + (e - c * nx)];
    }
    if (lane < nu) kp[(size_t)t * nu + lane] = w.k[lane];
    if (t > 0) r.store(w, lane);
    __syncthreads();
  }
  if (failed) {  // the nominal rollout: no gains at any step, nothing expected
    for (size_t e = lane; e < (size_t)T * nu * nx; e += 64) Kp[e] = 0.0;
    for (size_t e = lane; e < (size_t)T * nu; e += 64) kp[e] = 0.0;
    for (int e = lane; e < T; e += 64) a.clamped[p * T + e] = 0, a.qp_iterations[p * T + e] = 0;
  }
  if (lane < 2) a.dv[p * 2 + lane] = failed ? 0.0 : w.dv[lane];
  if (lane == 0) a.status[p] = failed;
}

int tds_lqr_check_args(const char *fn, int n, int T, int nx, int nu, bool null_arg) {
  if (null_arg || n < 1 || T < 1 || nx < 1 || nu < 1) return fail(TDS_ERR_INVALID_ARG, fn, ": NULL or empty argument");
  if (nx > TDS_LQR_MAX_NX) return fail(TDS_ERR_UNSUPPORTED, fn, ": nx exceeds the bound of 40 state entries");
  if (nu > TDS_LQR_MAX_NU) return fail(TDS_ERR_UNSUPPORTED, fn, ": nu exceeds the bound of 16 controls");
  return TDS_OK;
}

template <int NXM, int NUM, bool BOX, class Args>
int tds_lqr_launch(tds_hip_sim *s, const Args &a) {
  const size_t lds = tds_lqr_ws_doubles(a.nx, a.nu, BOX) * sizeof(double);
  void (*kernel)(Args);
  if constexpr (BOX) kernel = tds_lqr_box_kernel<NXM, NUM>;
  else kernel = tds_lqr_kernel<NXM, NUM>;
  // the build's LDS bound is raised once per device (bit d of `raised`), not per call
  static std::atomic<unsigned long long> raised{0};
  const unsigned long long bit = 1ull << (s->device & 63);
  if (!(raised.load(std::memory_order_acquire) & bit)) {
    TDS_HIP_TRY(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)(tds_lqr_ws_doubles(NXM, NUM, BOX) * sizeof(double))));
    raised.fetch_or(bit, std::memory_order_release);
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)a.n), dim3(64), lds, s->stream, a);
  TDS_HIP_TRY(hipGetLastError());
  return TDS_OK;
}

// the host checker's loop over the problems, plain and box alike
template <bool BOX>
int tds_lqr_host(int n, int T, int nx, int nu, const double *A, const double *B, const double *lx, const double *lu,
                 const double *lxx, const double *luu, const double *lux, const double *mu, const double *dlo,
                 const double *dhi, double *k, double *K, double *dv, int32_t *status, int32_t *clamped,
                 int32_t *qp_iterations) {
  std::vector<double> mem(tds_lqr_ws_doubles(nx, nu, BOX));
  const TdsLqrWs w = tds_lqr_ws(mem.data(), nx, nu, BOX);
  auto rows = [](double *dst, int stride, const double *src, int r, int c) {
    for (int i = 0; i < r; ++i)
      for (int j = 0; j < c; ++j) dst[i * stride + j] = src[(size_t)i * c + j];
  };
  for (size_t p = 0; p < (size_t)n; ++p) {
    rows(w.V, w.sx, lxx + (p * (T + 1) + T) * nx * nx, nx, nx);
    rows(w.Vx, 0, lx + (p * (T + 1) + T) * nx, 1, nx);
    w.dv[0] = w.dv[1] = 0.0;
    if constexpr (BOX)
      for (int c = 0; c < nu; ++c) w.k[c] = 0.0;
    double *kp = k + p * T * nu, *Kp = K + p * T * nu * nx;
    int failed = 0;
    for (int t = T - 1; t >= 0; --t) {
      const size_t pt = p * T + t;
      rows(w.A, w.sx, A + pt * nx * nx, nx, nx);
      rows(w.B, w.su, B + pt * nx * nu, nx, nu);
      rows(w.Qxx, w.sx, lxx + (p * (T + 1) + t) * nx * nx, nx, nx);
      rows(w.Qux, w.sx, lux + pt * nu * nx, nu, nx);
      rows(w.Quu, w.su, luu + pt * nu * nu, nu, nu);
      rows(w.Qx, 0, lx + (p * (T + 1) + t) * nx, 1, nx);
      rows(w.Qu, 0, lu + pt * nu, 1, nu);
      if constexpr (BOX) {
        rows(w.dlo, 0, dlo + pt * nu, 1, nu);
        rows(w.dhi, 0, dhi + pt * nu, 1, nu);
      }
      unsigned set = 0;
      int iters = 0;
      if (tds_lqr_step<BOX>(w, mu[p], 0, 1, TdsLqrNoSync{}, &set, &iters)) {
        failed = t + 1;
        break;
      }
      if constexpr (BOX) clamped[pt] = (int32_t)set, qp_iterations[pt] = iters;
      for (int c = 0; c < nu; ++c)
        for (int j = 0; j < nx; ++j) Kp[((size_t)t * nu + c) * nx + j] = w.K[c * w.sx + j];
      for (int c = 0; c < nu; ++c) kp[(size_t)t * nu + c] = w.k[c];
    }
    if (failed) {
      for (size_t e = 0; e < (size_t)T * nu * nx; ++e) Kp[e] = 0.0;
      for (size_t e = 0; e < (size_t)T * nu; ++e) kp[e] = 0.0;
      if constexpr (BOX)
        for (int t = 0; t < T; ++t) clamped[p * T + t] = qp_iterations[p * T + t] = 0;
    }
    dv[p * 2] = failed ? 0.0 : w.dv[0];
    dv[p * 2 + 1] = failed ? 0.0 : w.dv[1];
    status[p] = failed;
  }
  return TDS_OK;
}

// lo <= hi in every entry (a NaN fails the comparison)
bool tds_bounds_ordered(const double *lo, const double *hi, size_t count) {
  for (size_t e = 0; e < count; ++e)
    if (!(lo[e] <= hi[e])) return false;
  return true;
}

// ---- feedback rollout ------------------------------------------------------------------------------------------

struct TdsFbArgs {
  int rows, T, nin, nout, nsd, nact;
  const double *x0, *s_nom, *u_nom, *k, *K, *alpha;
  const int *problem_of_row;
  double *s_out, *u_out;
  double *xr, *y;  // the records [rows][nin] and the step's outputs [rows][nout]
};
// the clamped rollout's: absolute bounds on the actions [P][T][nact]
struct TdsFbBoxArgs : TdsFbArgs {
  const double *u_lo, *u_hi;
};

// step t of row r, entry i of its record (kernel lanes and the host checker's loops alike): s_t comes from x0 (t = 0)
// or the step's output; t = T stores the last state only.  BOX: u_t is clamped to [u_lo, u_hi] of its problem and step
// before it is stored and before it enters the record
template <bool BOX, class Args>
TDS_HD inline void tds_fb_entry(const Args &a, int t, size_t r, int i) {
  const int nsd = a.nsd, nact = a.nact;
  const double *s = t == 0 ? a.x0 + r * a.nin : a.y + r * a.nout;
  if (i < nsd) {
    a.s_out[(r * (a.T + 1) + t) * nsd + i] = s[i];
    if (t < a.T) a.xr[r * a.nin + i] = s[i];
  } else if (t < a.T) {
    double v;
    if (i < nsd + nact) {
      const int c = i - nsd;
      const size_t p = a.problem_of_row ? (size_t)a.problem_of_row[r] : r, pt = p * a.T + t;
      v = tds_feedback_action(a.u_nom[pt * nact + c], a.alpha[r], a.k[pt * nact + c], a.K + (pt * nact + c) * nsd, s,
                              a.s_nom + (p * (a.T + 1) + t) * nsd, nsd);
      if constexpr (BOX) v = tds_lqr_clamp(v, a.u_lo[pt * nact + c], a.u_hi[pt * nact + c]);
      a.u_out[(r * a.T + t) * nact + c] = v;
    } else {
      v = a.x0[r * a.nin + i];
    }
    a.xr[r * a.nin + i] = v;
  }
}

__global__ void __launch_bounds__(256) tds_fb_kernel(TdsFbArgs a, int t) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (long long)a.rows * a.nin) return;
  const size_t r = (size_t)(g / a.nin);
  tds_fb_entry<false>(a, t, r, (int)(g - (long long)r * a.nin));
}

__global__ void __launch_bounds__(256) tds_fb_box_kernel(TdsFbBoxArgs a, int t) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (long long)a.rows * a.nin) return;
  const size_t r = (size_t)(g / a.nin);
  tds_fb_entry<true>(a, t, r, (int)(g - (long long)r * a.nin));
}

int tds_fb_check_args(const char *fn, int rows, int T, bool null_arg) {
  if (null_arg || rows < 1) return fail(TDS_ERR_INVALID_ARG, fn, ": NULL or empty argument");
  if (T < 1) return fail(TDS_ERR_INVALID_ARG, fn, ": T must be at least 1");
  return TDS_OK;
}

TdsFbArgs tds_fb_args(const tds_model_t *m, int rows, int T, const void *x0, const void *s_nom, const void *u_nom,
                      const void *k, const void *K, const void *alpha, const void *por, void *s_out, void *u_out) {
  TdsFbArgs a;
  a.rows = rows, a.T = T, a.nin = m->input_dim, a.nout = m->output_dim;
  a.nsd = m->dof_q + m->dof_qd;
  a.nact = m->input_dim - a.nsd - (m->step_mode == TDS_STEP_LOCOMOTION ? 3 : 0);
  a.x0 = (const double *)x0, a.s_nom = (const double *)s_nom, a.u_nom = (const double *)u_nom;
  a.k = (const double *)k, a.K = (const double *)K, a.alpha = (const double *)alpha;
  a.problem_of_row = (const int *)por;
  a.s_out = (double *)s_out, a.u_out = (double *)u_out, a.xr = a.y = nullptr;
  return a;
}

// the device rollout, plain (u_lo NULL) and clamped: `fn` names the C ABI function in the argument errors
int tds_fb_device(const char *fn, tds_hip_sim *s, int rows, int T, const void *x0_dev, const void *s_nom_dev,
                  const void *u_nom_dev, const void *k_dev, const void *K_dev, const void *alpha_dev,
                  const void *problem_of_row_dev, const void *u_lo_dev, const void *u_hi_dev, void *s_out_dev,
                  void *u_out_dev) {
  if (!s) return fail(TDS_ERR_INVALID_ARG, fn, ": NULL or empty argument");
  DeviceGuard guard(s->device);
  int cls, rc = tds_diff_prepare(s, &cls);  // (the refusals first: a refused model may have no action slots at all)
  if (rc) return rc;
  if ((rc = tds_fb_check_args(fn, rows, T,
                              !x0_dev || !s_nom_dev || !u_nom_dev || !k_dev || !K_dev || !alpha_dev || !s_out_dev ||
                                  !u_out_dev)))
    return rc;
  if (s->n_variants > 0) return fail(TDS_ERR_UNSUPPORTED, "feedback rollout: not with model variants installed%s");
  TdsFbBoxArgs a;
  static_cast<TdsFbArgs &>(a) = tds_fb_args(&s->model, rows, T, x0_dev, s_nom_dev, u_nom_dev, k_dev, K_dev, alpha_dev,
                                            problem_of_row_dev, s_out_dev, u_out_dev);
  a.u_lo = (const double *)u_lo_dev, a.u_hi = (const double *)u_hi_dev;
  const size_t xr_bytes = ((size_t)rows * a.nin * sizeof(double) + 255) & ~(size_t)255;
  if ((rc = tds_work_buffer(s, xr_bytes + (size_t)rows * a.nout * sizeof(double)))) return rc;
  a.xr = (double *)s->d_diff_tmp;
  a.y = (double *)((char *)s->d_diff_tmp + xr_bytes);
  const unsigned blocks = (unsigned)(((long long)rows * a.nin + 255) / 256);
  for (int t = 0; t <= T; ++t) {
    if (a.u_lo) hipLaunchKernelGGL(tds_fb_box_kernel, dim3(blocks), dim3(256), 0, s->stream, a, t);
    else hipLaunchKernelGGL(tds_fb_kernel, dim3(blocks), dim3(256), 0, s->stream, static_cast<const TdsFbArgs &>(a), t);
    TDS_HIP_TRY(hipGetLastError());
    if (t == T) break;
    for (int r0 = 0; r0 < rows; r0 += s->num_envs) {
      const int nr = rows - r0 < s->num_envs ? rows - r0 : s->num_envs;
      if ((rc = launch(s, a.xr + (size_t)r0 * a.nin, a.y + (size_t)r0 * a.nout, nullptr, nullptr, nullptr, nr, 1,
                       TDS_RESET_NONE, nullptr)))
        return rc;
    }
  }
  return TDS_OK;
}

// the host checker, plain (u_lo NULL) and clamped
int tds_fb_host(const char *fn, const tds_model_t *model, int rows, int T, int num_problems, const double *x0,
                const double *s_nom, const double *u_nom, const double *k, const double *K, const double *alpha,
                const int32_t *problem_of_row, const double *u_lo, const double *u_hi, double *s_out, double *u_out) {
  if (!model) return fail(TDS_ERR_INVALID_ARG, fn, ": NULL or empty argument");
  int cls, rc = tds_diff_host_check(model, &cls);
  if (rc) return rc;
  if ((rc = tds_fb_check_args(fn, rows, T, !x0 || !s_nom || !u_nom || !k || !K || !alpha || !s_out || !u_out)))
    return rc;
  for (int r = 0; r < rows; ++r) {
    const int p = problem_of_row ? problem_of_row[r] : r;
    if (p < 0 || p >= num_problems) return fail(TDS_ERR_INVALID_ARG, fn, ": problem_of_row outside [0, num_problems)");
  }
  TdsFbBoxArgs a;
  static_cast<TdsFbArgs &>(a) = tds_fb_args(model, rows, T, x0, s_nom, u_nom, k, K, alpha, problem_of_row, s_out, u_out);
  a.u_lo = u_lo, a.u_hi = u_hi;
  if (u_lo && !tds_bounds_ordered(u_lo, u_hi, (size_t)num_problems * T * a.nact))
    return fail(TDS_ERR_INVALID_ARG, fn, ": u_lo > u_hi or a NaN bound");
  std::vector<double> xr((size_t)rows * a.nin), y((size_t)rows * a.nout);
  a.xr = xr.data(), a.y = y.data();
  int bad = 0;
  for (int t = 0; t <= T; ++t) {
    for (size_t r = 0; r < (size_t)rows; ++r)
      for (int i = 0; i < a.nin; ++i) {
        if (u_lo) tds_fb_entry<true>(a, t, r, i);
        else tds_fb_entry<false>(a, t, r, i);
      }
    if (t == T) break;
    rc = tds_hip_jacobian_host(model, rows, a.xr, 0, nullptr, 0, nullptr, 0, a.y, nullptr);
    if (rc == TDS_ERR_INVALID_ARG) bad = 1;  // inertia not positive definite somewhere: the outputs are written
    else if (rc) return rc;
  }
  return bad ? fail(TDS_ERR_INVALID_ARG, "step Jacobians: joint-space inertia not positive definite%s") : TDS_OK;
}

}  // namespace

extern "C" {

int tds_hip_lqr_backward(tds_hip_sim_t *s, int n, int T, int nx, int nu, const void *A_dev, const void *B_dev,
                         const void *lx_dev, const void *lu_dev, const void *lxx_dev, const void *luu_dev,
                         const void *lux_dev, const void *mu_dev, void *k_dev, void *K_dev, void *dv_dev,
                         void *status_dev) {
  int rc = tds_lqr_check_args("tds_hip_lqr_backward%s", n, T, nx, nu,
                              !s || !A_dev || !B_dev || !lx_dev || !lu_dev || !lxx_dev || !luu_dev || !lux_dev ||
                                  !mu_dev || !k_dev || !K_dev || !dv_dev || !status_dev);
  if (rc) return rc;
  DeviceGuard guard(s->device);
  const TdsLqrArgs a = {n, T, nx, nu, (const double *)A_dev, (const double *)B_dev, (const double *)lx_dev,
                        (const double *)lu_dev, (const double *)lxx_dev, (const double *)luu_dev,
                        (const double *)lux_dev, (const double *)mu_dev, (double *)k_dev, (double *)K_dev,
                        (double *)dv_dev, (int *)status_dev};
  return nx <= 28 && nu <= 8 ? tds_lqr_launch<28, 8, false>(s, a)
                             : tds_lqr_launch<TDS_LQR_MAX_NX, TDS_LQR_MAX_NU, false>(s, a);
}

int tds_hip_lqr_backward_host(int n, int T, int nx, int nu, const double *A, const double *B, const double *lx,
                              const double *lu, const double *lxx, const double *luu, const double *lux,
                              const double *mu, double *k, double *K, double *dv, int32_t *status) {
  int rc = tds_lqr_check_args("tds_hip_lqr_backward_host%s", n, T, nx, nu,
                              !A || !B || !lx || !lu || !lxx || !luu || !lux || !mu || !k || !K || !dv || !status);
  if (rc) return rc;
  return tds_lqr_host<false>(n, T, nx, nu, A, B, lx, lu, lxx, luu, lux, mu, nullptr, nullptr, k, K, dv, status, nullptr,
                             nullptr);
}

int tds_hip_lqr_backward_box(tds_hip_sim_t *s, int n, int T, int nx, int nu, const void *A_dev, const void *B_dev,
                             const void *lx_dev, const void *lu_dev, const void *lxx_dev, const void *luu_dev,
                             const void *lux_dev, const void *mu_dev, const void *dlo_dev, const void *dhi_dev,
                             void *k_dev, void *K_dev, void *dv_dev, void *status_dev, void *clamped_dev,
                             void *qp_iterations_dev) {
  int rc = tds_lqr_check_args("tds_hip_lqr_backward_box%s", n, T, nx, nu,
                              !s || !A_dev || !B_dev || !lx_dev || !lu_dev || !lxx_dev || !luu_dev || !lux_dev ||
                                  !mu_dev || !dlo_dev || !dhi_dev || !k_dev || !K_dev || !dv_dev || !status_dev ||
                                  !clamped_dev || !qp_iterations_dev);
  if (rc) return rc;
  DeviceGuard guard(s->device);
  const TdsLqrBoxArgs a = {{n, T, nx, nu, (const double *)A_dev, (const double *)B_dev, (const double *)lx_dev,
                            (const double *)lu_dev, (const double *)lxx_dev, (const double *)luu_dev,
                            (const double *)lux_dev, (const double *)mu_dev, (double *)k_dev, (double *)K_dev,
                            (double *)dv_dev, (int *)status_dev},
                           (const double *)dlo_dev, (const double *)dhi_dev, (int *)clamped_dev,
                           (int *)qp_iterations_dev};
  return nx <= 28 && nu <= 8 ? tds_lqr_launch<28, 8, true>(s, a)
                             : tds_lqr_launch<TDS_LQR_MAX_NX, TDS_LQR_MAX_NU, true>(s, a);
}

int tds_hip_lqr_backward_box_host(int n, int T, int nx, int nu, const double *A, const double *B, const double *lx,
                                  const double *lu, const double *lxx, const double *luu, const double *lux,
                                  const double *mu, const double *dlo, const double *dhi, double *k, double *K,
                                  double *dv, int32_t *status, int32_t *clamped, int32_t *qp_iterations) {
  int rc = tds_lqr_check_args("tds_hip_lqr_backward_box_host%s", n, T, nx, nu,
                              !A || !B || !lx || !lu || !lxx || !luu || !lux || !mu || !dlo || !dhi || !k || !K ||
                                  !dv || !status || !clamped || !qp_iterations);
  if (rc) return rc;
  if (!tds_bounds_ordered(dlo, dhi, (size_t)n * T * nu))
    return fail(TDS_ERR_INVALID_ARG, "tds_hip_lqr_backward_box_host: dlo > dhi or a NaN bound%s");
  return tds_lqr_host<true>(n, T, nx, nu, A, B, lx, lu, lxx, luu, lux, mu, dlo, dhi, k, K, dv, status, clamped,
                            qp_iterations);
}

int tds_hip_feedback_rollout(tds_hip_sim_t *s, int rows, int T, const void *x0_dev, const void *s_nom_dev,
                             const void *u_nom_dev, const void *k_dev, const void *K_dev, const void *alpha_dev,
                             const void *problem_of_row_dev, void *s_out_dev, void *u_out_dev) {
  return tds_fb_device("tds_hip_feedback_rollout%s", s, rows, T, x0_dev, s_nom_dev, u_nom_dev, k_dev, K_dev, alpha_dev,
                       problem_of_row_dev, nullptr, nullptr, s_out_dev, u_out_dev);
}

int tds_hip_feedback_rollout_box(tds_hip_sim_t *s, int rows, int T, const void *x0_dev, const void *s_nom_dev,
                                 const void *u_nom_dev, const void *k_dev, const void *K_dev, const void *alpha_dev,
                                 const void *problem_of_row_dev, const void *u_lo_dev, const void *u_hi_dev,
                                 void *s_out_dev, void *u_out_dev) {
  if (!u_lo_dev != !u_hi_dev)
    return fail(TDS_ERR_INVALID_ARG, "tds_hip_feedback_rollout_box: u_lo and u_hi are given together or not at all%s");
  return tds_fb_device("tds_hip_feedback_rollout_box%s", s, rows, T, x0_dev, s_nom_dev, u_nom_dev, k_dev, K_dev,
                       alpha_dev, problem_of_row_dev, u_lo_dev, u_hi_dev, s_out_dev, u_out_dev);
}

int tds_hip_feedback_rollout_host(const tds_model_t *model, int rows, int T, int num_problems, const double *x0,
                                  const double *s_nom, const double *u_nom, const double *k, const double *K,
                                  const double *alpha, const int32_t *problem_of_row, double *s_out, double *u_out) {
  return tds_fb_host("tds_hip_feedback_rollout_host%s", model, rows, T, num_problems, x0, s_nom, u_nom, k, K, alpha,
                     problem_of_row, nullptr, nullptr, s_out, u_out);
}

int tds_hip_feedback_rollout_box_host(const tds_model_t *model, int rows, int T, int num_problems, const double *x0,
                                      const double *s_nom, const double *u_nom, const double *k, const double *K,
                                      const double *alpha, const int32_t *problem_of_row, const double *u_lo,
                                      const double *u_hi, double *s_out, double *u_out) {
  if (!u_lo != !u_hi)
    return fail(TDS_ERR_INVALID_ARG,
                "tds_hip_feedback_rollout_box_host: u_lo and u_hi are given together or not at all%s");
  return tds_fb_host("tds_hip_feedback_rollout_box_host%s", model, rows, T, num_problems, x0, s_nom, u_nom, k, K, alpha,
                     problem_of_row, u_lo, u_hi, s_out, u_out);
}

}  // extern "C"
