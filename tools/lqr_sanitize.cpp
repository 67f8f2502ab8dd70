// lqr_sanitize.cpp — the host side of batched iLQR as a program of its own, for the host sanitizers:
// tds_hip_lqr_backward_host and tds_hip_feedback_rollout_host (csrc/tds_lqr.hip, host code only) at the edge shapes:
// nx = 1 and 40, nu = 1 and 16, T = 1, a problem that is not positive definite between two that are; the rollout with
// and without problem_of_row over a stand-in step; and their control-limited twins tds_hip_lqr_backward_box_host and
// tds_hip_feedback_rollout_box_host at the same shapes with finite, infinite and pinned (dlo == dhi) bounds, a step
// that is not positive definite, and the argument errors.  Every array is allocated at its exact size, so that an index past
// what is due is an address the sanitizer knows.  No GPU, no Python.  Build and run:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//     -Xarch_host -fno-sanitize-recover=undefined -Iinclude -Itiny-differentiable-simulator_amd/csrc \
//     tools/lqr_sanitize.cpp tiny-differentiable-simulator_amd/csrc/tds_lqr.hip -o lqr_sanitize
//   ./lqr_sanitize
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "tds_api_internal.h"

// (the library defines these in tds_api.hip and tds_jvp.hip, which this program does not link)
namespace tds_internal {
thread_local char g_err[512] = "";
int launch(tds_hip_sim *, const void *, void *, const void *, void *, void *, int, int, int, const unsigned char *,
           const Rollout *, int, const LaunchOpts *) {
  return TDS_ERR_NO_DEVICE;
}
int tds_diff_prepare(tds_hip_sim *, int *) { return TDS_ERR_NO_DEVICE; }
int tds_work_buffer(tds_hip_sim *, size_t) { return TDS_ERR_NO_DEVICE; }
}  // namespace tds_internal
extern "C" int tds_hip_model_check(const tds_model_t *) { return TDS_OK; }
// the stand-in step: y = 0.9 [s | u-sum folded into the velocities], enough to move every entry the rollout reads
extern "C" int tds_hip_jacobian_host(const tds_model_t *m, int n, const double *x, int, const int *, int, const int *,
                                     int, double *y, double *) {
  const int nsd = m->dof_q + m->dof_qd;
  for (int e = 0; e < n; ++e)
    for (int i = 0; i < m->output_dim; ++i) {
      double v = i < nsd ? 0.9 * x[(size_t)e * m->input_dim + i] : 0.0;
      if (i < nsd)
        for (int a = nsd; a < m->input_dim; ++a) v += 0.01 * x[(size_t)e * m->input_dim + a];
      y[(size_t)e * m->output_dim + i] = v;
    }
  return TDS_OK;
}

#define EXPECT(cond)                                                                                   \
  do {                                                                                                 \
    if (!(cond)) {                                                                                     \
      fprintf(stderr, "lqr_sanitize: line %d: %s  [%s]\n", __LINE__, #cond, tds_internal::g_err);      \
      return 1;                                                                                        \
    }                                                                                                  \
  } while (0)

static unsigned long long g_seed = 88172645463325252ull;
static double uniform(double lo, double hi) {  // xorshift64
  g_seed ^= g_seed << 13, g_seed ^= g_seed >> 7, g_seed ^= g_seed << 17;
  return lo + (hi - lo) * (double)(g_seed >> 11) / 9007199254740992.0;
}
static std::vector<double> draw(size_t n, double lo, double hi) {
  std::vector<double> v(n);
  for (double &x : v) x = uniform(lo, hi);
  return v;
}
// [count][d][d]: diagonally dominant, symmetric
static std::vector<double> spd(size_t count, int d, double diag) {
  std::vector<double> v(count * d * d);
  for (size_t c = 0; c < count; ++c)
    for (int i = 0; i < d; ++i)
      for (int j = 0; j <= i; ++j) {
        const double x = i == j ? diag : uniform(-0.5, 0.5) / d;
        v[(c * d + i) * d + j] = v[(c * d + j) * d + i] = x;
      }
  return v;
}

static int backward(int n, int T, int nx, int nu, int bad_problem, int bad_step) {
  std::vector<double> A = draw((size_t)n * T * nx * nx, -0.5 / nx, 0.5 / nx), B = draw((size_t)n * T * nx * nu, -1, 1);
  std::vector<double> lx = draw((size_t)n * (T + 1) * nx, -1, 1), lu = draw((size_t)n * T * nu, -1, 1);
  std::vector<double> lxx = spd((size_t)n * (T + 1), nx, 1.5), luu = spd((size_t)n * T, nu, 1.5);
  std::vector<double> lux = draw((size_t)n * T * nu * nx, -0.1, 0.1), mu((size_t)n, 0.25);
  if (bad_problem >= 0)
    for (int a = 0; a < nu; ++a) luu[(((size_t)bad_problem * T + bad_step) * nu + a) * nu + a] = -1e3;
  std::vector<double> k((size_t)n * T * nu), K((size_t)n * T * nu * nx), dv((size_t)n * 2);
  std::vector<int32_t> status((size_t)n);
  EXPECT(tds_hip_lqr_backward_host(n, T, nx, nu, A.data(), B.data(), lx.data(), lu.data(), lxx.data(), luu.data(),
                                   lux.data(), mu.data(), k.data(), K.data(), dv.data(), status.data()) == TDS_OK);
  for (int p = 0; p < n; ++p) {
    EXPECT(status[p] == (p == bad_problem ? bad_step + 1 : 0));
    double top = 0.0;
    for (size_t e = 0; e < (size_t)T * nu * nx; ++e) {
      EXPECT(isfinite(K[(size_t)p * T * nu * nx + e]));
      top = fmax(top, fabs(K[(size_t)p * T * nu * nx + e]));
    }
    for (size_t e = 0; e < (size_t)T * nu; ++e) top = fmax(top, fabs(k[(size_t)p * T * nu + e]));
    EXPECT(p == bad_problem ? top == 0.0 && dv[2 * p] == 0.0 && dv[2 * p + 1] == 0.0 : top > 0.0 && dv[2 * p] < 0.0);
  }
  return 0;
}

// the box pass: kind 0 bounds -U(0, 1) .. U(0, 1), 1 infinite (the outputs are the plain pass's), 2 every control pinned
static int backward_box(int n, int T, int nx, int nu, int kind, int bad_problem, int bad_step) {
  std::vector<double> A = draw((size_t)n * T * nx * nx, -0.5 / nx, 0.5 / nx), B = draw((size_t)n * T * nx * nu, -1, 1);
  std::vector<double> lx = draw((size_t)n * (T + 1) * nx, -1, 1), lu = draw((size_t)n * T * nu, -1, 1);
  std::vector<double> lxx = spd((size_t)n * (T + 1), nx, 1.5), luu = spd((size_t)n * T, nu, 1.5);
  std::vector<double> lux = draw((size_t)n * T * nu * nx, -0.1, 0.1), mu((size_t)n, 0.25);
  std::vector<double> dlo = draw((size_t)n * T * nu, -1, 0), dhi = draw((size_t)n * T * nu, 0, 1);
  if (kind == 1)
    for (size_t e = 0; e < dlo.size(); ++e) dlo[e] = -INFINITY, dhi[e] = INFINITY;
  if (kind == 2) dlo = dhi;
  if (bad_problem >= 0)
    for (int a = 0; a < nu; ++a) {
      const size_t e = ((size_t)bad_problem * T + bad_step) * nu + a;
      luu[e * nu + a] = -1e3, dlo[e] = -INFINITY, dhi[e] = INFINITY;  // (left free: the pivot is met)
    }
  std::vector<double> k((size_t)n * T * nu), K((size_t)n * T * nu * nx), dv((size_t)n * 2);
  std::vector<int32_t> status((size_t)n), clamped((size_t)n * T), its((size_t)n * T);
  EXPECT(tds_hip_lqr_backward_box_host(n, T, nx, nu, A.data(), B.data(), lx.data(), lu.data(), lxx.data(), luu.data(),
                                       lux.data(), mu.data(), dlo.data(), dhi.data(), k.data(), K.data(), dv.data(),
                                       status.data(), clamped.data(), its.data()) == TDS_OK);
  for (int p = 0; p < n; ++p) {
    EXPECT(status[p] == (p == bad_problem ? bad_step + 1 : 0));
    for (size_t e = 0; e < (size_t)T * nu * nx; ++e) EXPECT(isfinite(K[(size_t)p * T * nu * nx + e]));
    for (size_t e = (size_t)p * T * nu; e < (size_t)(p + 1) * T * nu; ++e)
      EXPECT(p == bad_problem ? k[e] == 0.0 : k[e] >= dlo[e] && k[e] <= dhi[e]);
    for (size_t e = (size_t)p * T; e < (size_t)(p + 1) * T; ++e) {
      EXPECT(p == bad_problem ? its[e] == 0 && clamped[e] == 0 : its[e] >= 1 && its[e] <= 100);
      EXPECT(clamped[e] >= 0 && clamped[e] < (1 << nu));
      if (kind == 1 && p != bad_problem) EXPECT(clamped[e] == 0 && its[e] == 2);
      if (kind == 2 && p != bad_problem && bad_problem < 0) EXPECT(its[e] <= 2);
    }
  }
  if (kind == 1) {  // infinite bounds: the plain pass, bit for bit
    std::vector<double> k0(k.size()), K0(K.size()), dv0(dv.size());
    std::vector<int32_t> status0((size_t)n);
    EXPECT(tds_hip_lqr_backward_host(n, T, nx, nu, A.data(), B.data(), lx.data(), lu.data(), lxx.data(), luu.data(),
                                     lux.data(), mu.data(), k0.data(), K0.data(), dv0.data(), status0.data()) == TDS_OK);
    EXPECT(k == k0 && K == K0 && dv == dv0 && status == status0);
  }
  // the argument errors: bounds out of order, a NaN bound
  if (kind == 0) {
    const double keep = dhi.back();
    dhi.back() = dlo.back() - 1.0;
    EXPECT(tds_hip_lqr_backward_box_host(n, T, nx, nu, A.data(), B.data(), lx.data(), lu.data(), lxx.data(), luu.data(),
                                         lux.data(), mu.data(), dlo.data(), dhi.data(), k.data(), K.data(), dv.data(),
                                         status.data(), clamped.data(), its.data()) == TDS_ERR_INVALID_ARG);
    dhi.back() = keep, dlo[0] = NAN;
    EXPECT(tds_hip_lqr_backward_box_host(n, T, nx, nu, A.data(), B.data(), lx.data(), lu.data(), lxx.data(), luu.data(),
                                         lux.data(), mu.data(), dlo.data(), dhi.data(), k.data(), K.data(), dv.data(),
                                         status.data(), clamped.data(), its.data()) == TDS_ERR_INVALID_ARG);
    EXPECT(strstr(tds_internal::g_err, "dlo > dhi or a NaN bound") != nullptr);
  }
  return 0;
}

static int rollout(int rows, int T, int P, bool mapped) {
  tds_model_t m;
  memset(&m, 0, sizeof(m));
  m.dof_q = 3, m.dof_qd = 2, m.is_floating = 1, m.input_dim = 9, m.output_dim = 7;  // (dof_q = dof_qd + 1: floating)
  m.step_mode = TDS_STEP_LOCOMOTION;                                                 // n_act = 9 - 5 - 3 = 1
  const int nsd = 5, nact = 1;
  std::vector<double> x0 = draw((size_t)rows * m.input_dim, -1, 1), s_nom = draw((size_t)P * (T + 1) * nsd, -1, 1);
  std::vector<double> u_nom = draw((size_t)P * T * nact, -1, 1), k = draw((size_t)P * T * nact, -1, 1);
  std::vector<double> K = draw((size_t)P * T * nact * nsd, -1, 1), alpha = draw((size_t)rows, 0, 1);
  std::vector<int32_t> por((size_t)rows);
  for (int r = 0; r < rows; ++r) por[r] = (rows - 1 - r) % P;
  std::vector<double> s((size_t)rows * (T + 1) * nsd), u((size_t)rows * T * nact);
  EXPECT(tds_hip_feedback_rollout_host(&m, rows, T, P, x0.data(), s_nom.data(), u_nom.data(), k.data(), K.data(),
                                       alpha.data(), mapped ? por.data() : nullptr, s.data(), u.data()) == TDS_OK);
  for (double v : s) EXPECT(isfinite(v));
  for (double v : u) EXPECT(isfinite(v));
  // the clamped twin: every action inside its bounds; infinite bounds give the call above; the argument errors
  std::vector<double> lo = draw((size_t)P * T * nact, -0.5, 0), hi = draw((size_t)P * T * nact, 0, 0.5);
  std::vector<double> sb(s.size()), ub(u.size());
  EXPECT(tds_hip_feedback_rollout_box_host(&m, rows, T, P, x0.data(), s_nom.data(), u_nom.data(), k.data(), K.data(),
                                           alpha.data(), mapped ? por.data() : nullptr, lo.data(), hi.data(), sb.data(),
                                           ub.data()) == TDS_OK);
  for (int r = 0; r < rows; ++r)
    for (int e = 0; e < T * nact; ++e) {
      const size_t b = (size_t)(mapped ? por[r] : r) * T * nact + e;
      EXPECT(ub[(size_t)r * T * nact + e] >= lo[b] && ub[(size_t)r * T * nact + e] <= hi[b]);
    }
  for (double v : sb) EXPECT(isfinite(v));
  std::vector<double> ninf(lo.size(), -INFINITY), pinf(lo.size(), INFINITY);
  EXPECT(tds_hip_feedback_rollout_box_host(&m, rows, T, P, x0.data(), s_nom.data(), u_nom.data(), k.data(), K.data(),
                                           alpha.data(), mapped ? por.data() : nullptr, ninf.data(), pinf.data(),
                                           sb.data(), ub.data()) == TDS_OK);
  EXPECT(sb == s && ub == u);
  EXPECT(tds_hip_feedback_rollout_box_host(&m, rows, T, P, x0.data(), s_nom.data(), u_nom.data(), k.data(), K.data(),
                                           alpha.data(), mapped ? por.data() : nullptr, nullptr, nullptr, sb.data(),
                                           ub.data()) == TDS_OK);
  EXPECT(sb == s && ub == u);
  EXPECT(tds_hip_feedback_rollout_box_host(&m, rows, T, P, x0.data(), s_nom.data(), u_nom.data(), k.data(), K.data(),
                                           alpha.data(), mapped ? por.data() : nullptr, lo.data(), nullptr, sb.data(),
                                           ub.data()) == TDS_ERR_INVALID_ARG);
  EXPECT(tds_hip_feedback_rollout_box_host(&m, rows, T, P, x0.data(), s_nom.data(), u_nom.data(), k.data(), K.data(),
                                           alpha.data(), mapped ? por.data() : nullptr, hi.data(), lo.data(), sb.data(),
                                           ub.data()) == TDS_ERR_INVALID_ARG);
  lo.back() = NAN;
  EXPECT(tds_hip_feedback_rollout_box_host(&m, rows, T, P, x0.data(), s_nom.data(), u_nom.data(), k.data(), K.data(),
                                           alpha.data(), mapped ? por.data() : nullptr, lo.data(), hi.data(), sb.data(),
                                           ub.data()) == TDS_ERR_INVALID_ARG);
  EXPECT(strstr(tds_internal::g_err, "u_lo > u_hi or a NaN bound") != nullptr);
  if (mapped) {
    por[rows / 2] = P;
    EXPECT(tds_hip_feedback_rollout_host(&m, rows, T, P, x0.data(), s_nom.data(), u_nom.data(), k.data(), K.data(),
                                         alpha.data(), por.data(), s.data(), u.data()) == TDS_ERR_INVALID_ARG);
  }
  return 0;
}

int main() {
  const int shapes[][4] = {{1, 1, 1, 1}, {3, 1, 40, 16}, {3, 2, 1, 16}, {3, 3, 40, 1}, {2, 4, 28, 8}, {2, 5, 37, 12}};
  for (const auto &sh : shapes)
    if (backward(sh[0], sh[1], sh[2], sh[3], -1, 0)) return 1;
  if (backward(3, 4, 40, 16, 1, 2)) return 1;  // not positive definite at step 2 of the middle problem
  if (backward(3, 1, 5, 3, 1, 0)) return 1;
  for (const auto &sh : shapes)
    for (int kind = 0; kind < 3; ++kind)
      if (backward_box(sh[0], sh[1], sh[2], sh[3], kind, -1, 0)) return 1;
  if (backward_box(3, 4, 40, 16, 0, 1, 2) || backward_box(3, 1, 5, 3, 0, 1, 0) || backward_box(3, 4, 28, 8, 1, 1, 0))
    return 1;
  std::vector<double> none(1);
  std::vector<int32_t> st(1);
  EXPECT(tds_hip_lqr_backward_host(1, 1, 41, 1, none.data(), none.data(), none.data(), none.data(), none.data(),
                                   none.data(), none.data(), none.data(), none.data(), none.data(), none.data(),
                                   st.data()) == TDS_ERR_UNSUPPORTED);
  EXPECT(strstr(tds_internal::g_err, "40 state entries") != nullptr);
  EXPECT(tds_hip_lqr_backward_host(1, 1, 1, 17, none.data(), none.data(), none.data(), none.data(), none.data(),
                                   none.data(), none.data(), none.data(), none.data(), none.data(), none.data(),
                                   st.data()) == TDS_ERR_UNSUPPORTED);
  EXPECT(strstr(tds_internal::g_err, "16 controls") != nullptr);
  EXPECT(tds_hip_lqr_backward_box_host(1, 1, 41, 1, none.data(), none.data(), none.data(), none.data(), none.data(),
                                       none.data(), none.data(), none.data(), none.data(), none.data(), none.data(),
                                       none.data(), none.data(), st.data(), st.data(), st.data()) == TDS_ERR_UNSUPPORTED);
  EXPECT(strstr(tds_internal::g_err, "40 state entries") != nullptr);
  EXPECT(tds_hip_lqr_backward_box_host(1, 1, 1, 17, none.data(), none.data(), none.data(), none.data(), none.data(),
                                       none.data(), none.data(), none.data(), none.data(), none.data(), none.data(),
                                       none.data(), none.data(), st.data(), st.data(), st.data()) == TDS_ERR_UNSUPPORTED);
  EXPECT(strstr(tds_internal::g_err, "16 controls") != nullptr);
  EXPECT(tds_hip_lqr_backward_box_host(1, 1, 1, 1, none.data(), none.data(), none.data(), none.data(), none.data(),
                                       none.data(), none.data(), none.data(), nullptr, none.data(), none.data(),
                                       none.data(), none.data(), st.data(), st.data(), st.data()) == TDS_ERR_INVALID_ARG);
  if (rollout(1, 1, 1, false) || rollout(5, 4, 5, false) || rollout(7, 3, 2, true)) return 1;
  printf("lqr_sanitize: ok\n");
  return 0;
}
