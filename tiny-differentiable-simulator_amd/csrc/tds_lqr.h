// tds_lqr.h — the statement of the batched LQR backward pass and of the feedback law of the closed-loop rollout
// (tds_lqr.hip; C ABI tds_hip_lqr_backward / tds_hip_feedback_rollout and their _host checkers, include/tds_hip.h).
//
// One function, tds_lqr_step, is the device wavefront's step and the host checker's: it walks every phase's elements
// from `lane` with stride `lanes` (the device: 64 lanes of one wavefront over a workspace in LDS; the host: lane 0 of 1
// over a workspace of the same layout in memory) and calls `sync` between the phases.  Every element of every product,
// of the Cholesky factor and of the triangular solves is ONE sequential sum in index order, written once, here; with
// the unit built without FP contraction the device and the host round alike.
#pragma once
#include <math.h>

#include "tds_dual.h"  // TDS_HD
#include "tds_hip.h"

namespace {

// The workspace of one problem, in doubles.  Rows are padded to an odd length (sx, su): a wavefront that walks a
// column (the Cholesky's L[i][k] over i, a solve's K[a][c] over c is a row walk) then touches 64 different LDS banks.
//   V   [nx][sx]   V_xx; rewritten in place at the end of a step
//   A   [nx][sx]   B [nx][su]   the step's dynamics
//   W   [max(nx, nu)][sx]   V_xx A; dead once Q_xx and Q_ux stand, then G = Q_uu K [nu][sx]
//   WB  [nx][su]   V_xx B
//   Qxx [nx][sx]   holds lxx when the step begins;  Qux [nu][sx] (lux),  Quu [nu][su] (luu; stays unregularised)
//   L   [nu][su]   the Cholesky factor of Q_uu + mu I;  K [nu][sx]
//   vectors: Vx [nx], Qx [nx] (lx), Qu [nu] (lu), k [nu], g = Q_uu k [nu], dv [2]
// nx = 40, nu = 16: 4 * 1640 + 2 * 680 + 2 * 656 + 2 * 272 + 2 * 40 + 3 * 16 + 2 = 9906 doubles = 79248 bytes: two
// problems per compute unit of 160 KiB.  nx = 28, nu = 8 (the Ant): 4 * 812 + 2 * 252 + 2 * 232 + 2 * 72 + 82 = 4442
// doubles = 35536 bytes: four.
// The box layout (control limits: tds_lqr_qp below) appends the QP's eight vectors of nu doubles behind dv:
//   dlo, dhi   the bounds on the step;   qx, qhx   the iterate x and H x;   qc, qhc   a candidate and H times it
//   qy   the Newton system's right-hand side, then the Newton point;   qs   spare (keeps the count even)
// 1024 bytes at nu = 16 (80272: still two per compute unit), 512 at nu = 8 (36048: still four).
struct TdsLqrWs {
  int nx, nu, sx, su;
  double *V, *A, *B, *W, *WB, *Qxx, *Qux, *Quu, *L, *K, *Vx, *Qx, *Qu, *k, *g, *dv;
  double *dlo, *dhi, *qx, *qhx, *qc, *qhc, *qy, *qs;  // box layout only
};

TDS_HD inline size_t tds_lqr_ws_doubles(int nx, int nu, bool box = false) {
  const size_t sx = nx | 1, su = nu | 1, mx = nx > nu ? nx : nu;
  return 3 * nx * sx + mx * sx + 2 * nx * su + 2 * nu * sx + 2 * nu * su + 2 * nx + 3 * nu + 2 + (box ? 8 * nu : 0);
}

TDS_HD inline TdsLqrWs tds_lqr_ws(double *p, int nx, int nu, bool box = false) {
  TdsLqrWs w;
  w.nx = nx, w.nu = nu, w.sx = nx | 1, w.su = nu | 1;
  const int mx = nx > nu ? nx : nu;
  w.V = p, p += nx * w.sx;
  w.A = p, p += nx * w.sx;
  w.Qxx = p, p += nx * w.sx;
  w.W = p, p += mx * w.sx;
  w.B = p, p += nx * w.su;
  w.WB = p, p += nx * w.su;
  w.Qux = p, p += nu * w.sx;
  w.K = p, p += nu * w.sx;
  w.Quu = p, p += nu * w.su;
  w.L = p, p += nu * w.su;
  w.Vx = p, p += nx;
  w.Qx = p, p += nx;
  w.Qu = p, p += nu;
  w.k = p, p += nu;
  w.g = p, p += nu;
  w.dv = p, p += 2;
  w.dlo = w.dhi = w.qx = w.qhx = w.qc = w.qhc = w.qy = w.qs = nullptr;
  if (box) {
    w.dlo = p, p += nu;
    w.dhi = p, p += nu;
    w.qx = p, p += nu;
    w.qhx = p, p += nu;
    w.qc = p, p += nu;
    w.qhc = p, p += nu;
    w.qy = p, p += nu;
    w.qs = p;
  }
  return w;
}

// O[i][j] = I[i][j] + sum_k X(k, i) Y(k, j) over i < ni, j < nj (I NULL: the sum starts at 0), with X(k, i) =
// X[k xk + i xi], Y(k, j) = Y[k yk + j yj], O and I row-major with strides os, is.  A lane takes tiles of four rows
// (4 ti ..) and four columns (j, j + q, j + 2 q, j + 3 q with q = ceil(nj / 4), so that the lanes of a wavefront sit
// on consecutive j): sixteen independent sums fed by eight loads per k.  The operands of k + 1 are requested before
// the sums of k run, so the memory's latency lies behind arithmetic.  Each sum is still one lane's, in the order of k.
// Rows and columns past the end repeat the last valid one and are not stored.  O may be I (a lane reads only what it
// wrote itself).
TDS_HD inline __attribute__((always_inline)) void tds_lqr_mac(const double *X, int xk, int xi, const double *Y, int yk, int yj, const double *I, int is,
                               double *O, int os, int ni, int nj, int nk, int lane, int lanes) {
  constexpr int TI = 4, TJ = 4;
  const int q = (nj + TJ - 1) / TJ, tiles = ((ni + TI - 1) / TI) * q;
  for (int t = lane; t < tiles; t += lanes) {
    const int ti = t / q, j0 = t - ti * q;
    int ii[TI], jj[TJ];
#pragma unroll
    for (int r = 0; r < TI; ++r) ii[r] = TI * ti + r < ni ? TI * ti + r : ni - 1;
#pragma unroll
    for (int c = 0; c < TJ; ++c) jj[c] = j0 + c * q < nj ? j0 + c * q : nj - 1;
    double s[TI][TJ];
#pragma unroll
    for (int r = 0; r < TI; ++r)
#pragma unroll
      for (int c = 0; c < TJ; ++c) s[r][c] = I ? I[ii[r] * is + jj[c]] : 0.0;
    const double *xp[TI], *yp[TJ];
#pragma unroll
    for (int r = 0; r < TI; ++r) xp[r] = X + ii[r] * xi;
#pragma unroll
    for (int c = 0; c < TJ; ++c) yp[c] = Y + jj[c] * yj;
    double a[TI], b[TJ];
    if (nk > 0) {
#pragma unroll
      for (int r = 0; r < TI; ++r) a[r] = xp[r][0];
#pragma unroll
      for (int c = 0; c < TJ; ++c) b[c] = yp[c][0];
    }
    for (int k = 0; k < nk; ++k) {
      double ca[TI], cb[TJ];
#pragma unroll
      for (int r = 0; r < TI; ++r) ca[r] = a[r];
#pragma unroll
      for (int c = 0; c < TJ; ++c) cb[c] = b[c];
      if (k + 1 < nk) {
#pragma unroll
        for (int r = 0; r < TI; ++r) a[r] = xp[r][(k + 1) * xk];
#pragma unroll
        for (int c = 0; c < TJ; ++c) b[c] = yp[c][(k + 1) * yk];
      }
#pragma unroll
      for (int r = 0; r < TI; ++r)
#pragma unroll
        for (int c = 0; c < TJ; ++c) s[r][c] += ca[r] * cb[c];
    }
#pragma unroll
    for (int r = 0; r < TI; ++r)
#pragma unroll
      for (int c = 0; c < TJ; ++c)
        if (TI * ti + r < ni && j0 + c * q < nj) O[ii[r] * os + jj[c]] = s[r][c];
  }
}

// Q_uu + mu I = L L^T, a column at a time: every lane forms the pivot (the same sum from the same values), the lanes
// below it their entry of the column.  `clamped` (bit a: control a) replaces those rows and columns by the identity's,
// so that the indexing stays fixed; with no bit set the sums are those of the plain step's phase (3), in the same
// order (the plain step keeps its own loop: routed through this function its builds' code changed).  Returns 1 where a
// pivot is not positive (every lane alike).
template <class Sync>
TDS_HD inline __attribute__((always_inline)) int tds_lqr_factor(const TdsLqrWs &w, double mu, unsigned clamped, int lane, int lanes, Sync sync) {
  const int nu = w.nu, su = w.su;
  for (int j = 0; j < nu; ++j) {
    if (clamped >> j & 1u) {
      for (int i = j + lane; i < nu; i += lanes) w.L[i * su + j] = i == j ? 1.0 : 0.0;
      sync();
      continue;
    }
    double d = w.Quu[j * su + j] + mu;
#pragma unroll 4
    for (int k = 0; k < j; ++k) d -= w.L[j * su + k] * w.L[j * su + k];
    if (!(d > 0.0)) return 1;
    const double ljj = sqrt(d);
    for (int i = j + lane; i < nu; i += lanes) {
      if (i == j) {
        w.L[j * su + j] = ljj;
      } else if (clamped >> i & 1u) {
        w.L[i * su + j] = 0.0;
      } else {
        double s = w.Quu[i * su + j];
#pragma unroll 4
        for (int k = 0; k < j; ++k) s -= w.L[i * su + k] * w.L[j * su + k];
        w.L[i * su + j] = s / ljj;
      }
    }
    sync();
  }
  return 0;
}

// x = (L L^T)^-1 rhs for one column (rhs[a st], a < nu), the column in registers (loops of constant extent, unrolled:
// nothing indexed at run time)
TDS_HD inline __attribute__((always_inline)) void tds_lqr_solve(const TdsLqrWs &w, const double *rhs, int st, double (&x)[TDS_LQR_MAX_NU]) {
  const int nu = w.nu, su = w.su;
#pragma unroll
  for (int a = 0; a < TDS_LQR_MAX_NU; ++a) {
    if (a < nu) {
      double s = rhs[a * st];
#pragma unroll
      for (int b = 0; b < a; ++b) s -= w.L[a * su + b] * x[b];
      x[a] = s / w.L[a * su + a];
    }
  }
#pragma unroll
  for (int a = TDS_LQR_MAX_NU - 1; a >= 0; --a) {
    if (a < nu) {
      double s = x[a];
#pragma unroll
      for (int b = a + 1; b < TDS_LQR_MAX_NU; ++b)
        if (b < nu) s -= w.L[b * su + a] * x[b];
      x[a] = s / w.L[a * su + a];
    }
  }
}

// A decision of the QP loop, formed alike by every lane from the same LDS values: the device reads it from the first
// lane, so that the compiler knows the branch to be the wavefront's
TDS_HD inline int tds_lqr_uniform(int v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_readfirstlane(v);
#else
  return v;
#endif
}

TDS_HD inline double tds_lqr_clamp(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The settings of the box QP (Tassa, Mansard, Todorov: Control-limited differential dynamic programming, ICRA 2014)
constexpr int TDS_LQR_QP_MAX_ITER = 100;
constexpr double TDS_LQR_QP_MIN_GRAD = 1e-8, TDS_LQR_QP_ARMIJO = 0.1, TDS_LQR_QP_STEP_DEC = 0.6, TDS_LQR_QP_MIN_STEP = 1e-22;

// Phases (3) and (4) of a step under control limits: min_x f(x) = x^T H x / 2 + q^T x over dlo <= x <= dhi, with
// H = Q_uu + mu I, q = Q_u, by projected Newton from x = clamp(k of step t + 1) (w.k on entry), then the gains on the
// controls the QP left free.  For i = 1 .. 100:
//   1. g = q + H x; control a is CLAMPED if (x_a == dlo_a and g_a > 0) or (x_a == dhi_a and g_a < 0), else FREE
//   2. no control free: stop (K = 0)
//   3. first iteration, or the clamped set changed: factorise H_ff (tds_lqr_factor); a pivot not positive: return 1
//   4. |g_f|_2 < 1e-8 (the sum of squares in index order): stop
//   5. y_c = x_c, y_f = -H_ff^-1 (q_f + H_fc x_c) (tds_lqr_solve, one lane); sd = (y - x)^T g; sd >= 0: stop
//   6. line search: the candidate at step 1 is clamp(y) ITSELF, at step < 1 clamp(x + step (y - x)); the first with
//      (f(cand) - f(x)) / (step sd) >= 0.1 is taken, else step *= 0.6; step < 1e-22: stop and keep x
//   7. x = cand
// Then k = x, and K = -H_ff^-1 Q_ux,f on the free rows of the last factorisation's set, zero on its clamped rows, zero
// everywhere if the loop stopped with nothing free.  With dlo = -inf, dhi = +inf the first Newton point is the plain
// pass's k, formed by the same sums, and the second iteration's test 4 ends the loop: k and K are the plain pass's bit
// for bit.  Vectors are formed a lane per entry (an entry's sum in index order) and stored to the workspace; every
// decision (the set, the stops, the line search) is then formed by EVERY lane from those values, so the control flow is
// the wavefront's without communication.  H x travels with x (H cand is formed for f(cand) and becomes H x when the
// candidate is taken), so an iteration costs one product per candidate.  *set: the final clamped set; *iters: the
// iterations begun (at most 100).
template <class Sync>
TDS_HD inline __attribute__((always_inline)) int tds_lqr_qp(const TdsLqrWs &w, double mu, int lane, int lanes, Sync sync, unsigned *set, int *iters) {
  const int nx = w.nx, nu = w.nu, sx = w.sx, su = w.su;
  const unsigned full = nu >= 32 ? ~0u : (1u << nu) - 1u;
  double *x = w.qx, *hx = w.qhx, *c = w.qc, *hc = w.qhc;
  // (H v)_a, one lane's sum in index order
  auto times_h = [&](const double *v, int a) {
    double s = 0.0;
    for (int b = 0; b < nu; ++b) s += (a == b ? w.Quu[a * su + b] + mu : w.Quu[a * su + b]) * v[b];
    return s;
  };
  // f(v) given H v
  auto value = [&](const double *v, const double *hv) {
    double s = 0.0;
    for (int a = 0; a < nu; ++a) s += v[a] * (0.5 * hv[a] + w.Qu[a]);
    return s;
  };
  for (int a = lane; a < nu; a += lanes) x[a] = tds_lqr_clamp(w.k[a], w.dlo[a], w.dhi[a]);
  sync();
  for (int a = lane; a < nu; a += lanes) hx[a] = times_h(x, a);
  sync();
  unsigned cl = 0, factored = 0;
  int it = 1, none_free = 0;
  for (; it <= TDS_LQR_QP_MAX_ITER; ++it) {
    // 1.
    cl = 0;
    double gn = 0.0;
    for (int a = 0; a < nu; ++a) {
      const double g = w.Qu[a] + hx[a];
      if ((x[a] == w.dlo[a] && g > 0.0) || (x[a] == w.dhi[a] && g < 0.0)) cl |= 1u << a;
      else gn += g * g;
    }
    cl = (unsigned)tds_lqr_uniform((int)cl);
    // 2.
    if (cl == full) {
      none_free = 1;
      break;
    }
    // 3.
    if (it == 1 || cl != factored) {
      if (tds_lqr_factor(w, mu, cl, lane, lanes, sync)) return 1;
      factored = cl;
    }
    // 4.
    if (tds_lqr_uniform(sqrt(gn) < TDS_LQR_QP_MIN_GRAD)) break;
    // 5.
    for (int a = lane; a < nu; a += lanes) {
      double s = 0.0;
      if (!(cl >> a & 1u)) {
        s = w.Qu[a];
        for (int b = 0; b < nu; ++b)
          if (cl >> b & 1u) s += w.Quu[a * su + b] * x[b];
      }
      w.qy[a] = s;
    }
    sync();
    if (lane == 0) {
      double y[TDS_LQR_MAX_NU];
      tds_lqr_solve(w, w.qy, 1, y);
#pragma unroll
      for (int a = 0; a < TDS_LQR_MAX_NU; ++a)
        if (a < nu) w.qy[a] = (cl >> a & 1u) ? x[a] : -y[a];
    }
    sync();
    double sd = 0.0;
    for (int a = 0; a < nu; ++a) sd += (w.qy[a] - x[a]) * (w.Qu[a] + hx[a]);
    if (tds_lqr_uniform(!(sd < 0.0))) break;
    // 6.
    const double fx = value(x, hx);
    double step = 1.0;
    int taken = 0;
    for (;;) {
      for (int a = lane; a < nu; a += lanes)
        c[a] = tds_lqr_clamp(step == 1.0 ? w.qy[a] : x[a] + step * (w.qy[a] - x[a]), w.dlo[a], w.dhi[a]);
      sync();
      for (int a = lane; a < nu; a += lanes) hc[a] = times_h(c, a);
      sync();
      const double fc = value(c, hc);
      taken = tds_lqr_uniform((fc - fx) / (step * sd) >= TDS_LQR_QP_ARMIJO);
      if (taken) break;
      step *= TDS_LQR_QP_STEP_DEC;
      if (tds_lqr_uniform(step < TDS_LQR_QP_MIN_STEP)) break;
      sync();  // (every lane has read this candidate before the next one is written)
    }
    if (!taken) break;
    // 7.
    double *sw = x;
    x = c, c = sw;
    sw = hx, hx = hc, hc = sw;
  }
  *set = cl;
  *iters = it < TDS_LQR_QP_MAX_ITER ? it : TDS_LQR_QP_MAX_ITER;
  // the gains: a column per lane; k = x
  for (int col = lane; col <= nx; col += lanes) {
    if (col == nx) {
      for (int a = 0; a < nu; ++a) w.k[a] = x[a];
    } else if (none_free) {
      for (int a = 0; a < nu; ++a) w.K[a * sx + col] = 0.0;
    } else {
      double v[TDS_LQR_MAX_NU];
      tds_lqr_solve(w, w.Qux + col, sx, v);
#pragma unroll
      for (int a = 0; a < TDS_LQR_MAX_NU; ++a)
        if (a < nu) w.K[a * sx + col] = (cl >> a & 1u) ? 0.0 : -v[a];
    }
  }
  sync();
  return 0;
}

// One step of the recursion.  On entry the workspace holds V, Vx (of step t + 1), A, B, and lxx, lux, luu, lx, lu in
// Qxx, Qux, Quu, Qx, Qu; on return V, Vx are those of step t, K and k the gains, dv the sums so far.  Returns 0, or 1
// where a pivot of the Cholesky was not positive (every lane returns the same: each forms the pivot itself).  BOX: the
// step under control limits (w.dlo, w.dhi of the box layout; w.k holds k of step t + 1, zero at the last step); *set
// and *iters receive the QP's final clamped set and its iteration count.
template <bool BOX = false, class Sync>
TDS_HD inline __attribute__((always_inline)) int tds_lqr_step(const TdsLqrWs &w, double mu, int lane, int lanes, Sync sync, unsigned *set = nullptr,
                                                              int *iters = nullptr) {
  const int nx = w.nx, nu = w.nu, sx = w.sx, su = w.su;
  // (1) W = V A, WB = V B, Q_x = lx + A^T V_x, Q_u = lu + B^T V_x
  tds_lqr_mac(w.V, 1, sx, w.A, sx, 1, nullptr, 0, w.W, sx, nx, nx, nx, lane, lanes);
  tds_lqr_mac(w.V, 1, sx, w.B, su, 1, nullptr, 0, w.WB, su, nx, nu, nx, lane, lanes);
  tds_lqr_mac(w.A, sx, 1, w.Vx, 1, 0, w.Qx, 1, w.Qx, 1, nx, 1, nx, lane, lanes);
  tds_lqr_mac(w.B, su, 1, w.Vx, 1, 0, w.Qu, 1, w.Qu, 1, nu, 1, nx, lane, lanes);
  sync();
  // (2) Q_xx = lxx + A^T W, Q_ux = lux + B^T W, Q_uu = luu + B^T WB
  tds_lqr_mac(w.A, sx, 1, w.W, sx, 1, w.Qxx, sx, w.Qxx, sx, nx, nx, nx, lane, lanes);
  tds_lqr_mac(w.B, su, 1, w.W, sx, 1, w.Qux, sx, w.Qux, sx, nu, nx, nx, lane, lanes);
  tds_lqr_mac(w.B, su, 1, w.WB, su, 1, w.Quu, su, w.Quu, su, nu, nu, nx, lane, lanes);
  sync();
  if constexpr (BOX) {
    // (3), (4) under control limits: the box QP for k, the gains on its free controls
    if (tds_lqr_qp(w, mu, lane, lanes, sync, set, iters)) return 1;
  } else {
    // (3) Q_uu + mu I = L L^T, a column at a time: every lane forms the pivot (the same sum from the same values), the
    //     lanes below it their entry of the column
    for (int j = 0; j < nu; ++j) {
      double d = w.Quu[j * su + j] + mu;
#pragma unroll 4
      for (int k = 0; k < j; ++k) d -= w.L[j * su + k] * w.L[j * su + k];
      if (!(d > 0.0)) return 1;
      const double ljj = sqrt(d);
      for (int i = j + lane; i < nu; i += lanes) {
        if (i == j) {
          w.L[j * su + j] = ljj;
        } else {
          double s = w.Quu[i * su + j];
#pragma unroll 4
          for (int k = 0; k < j; ++k) s -= w.L[i * su + k] * w.L[j * su + k];
          w.L[i * su + j] = s / ljj;
        }
      }
      sync();
    }
    // (4) K = -(L L^T)^-1 Q_ux, k = -(L L^T)^-1 Q_u: a column per lane
    for (int c = lane; c <= nx; c += lanes) {
      const bool vec = c == nx;
      double *dst = vec ? w.k : w.K + c;
      const double *rhs = vec ? w.Qu : w.Qux + c;
      const int st = vec ? 1 : sx;
      double x[TDS_LQR_MAX_NU];
      tds_lqr_solve(w, rhs, st, x);
#pragma unroll
      for (int a = 0; a < TDS_LQR_MAX_NU; ++a)
        if (a < nu) dst[a * st] = -x[a];
    }
    sync();
  }
  // (5) G = Q_uu K (in W), g = Q_uu k
  tds_lqr_mac(w.Quu, 1, su, w.K, sx, 1, nullptr, 0, w.W, sx, nu, nx, nu, lane, lanes);
  tds_lqr_mac(w.Quu, 1, su, w.k, 1, 0, nullptr, 0, w.g, 1, nu, 1, nu, lane, lanes);
  sync();
  // (6) V_xx = Q_xx + K^T G + K^T Q_ux + Q_ux^T K and V_x = Q_x + K^T g + K^T Q_u + Q_ux^T k: an element's three
  //     sums run one after the other in the same lane; the expected change of the cost
  tds_lqr_mac(w.K, sx, 1, w.W, sx, 1, w.Qxx, sx, w.V, sx, nx, nx, nu, lane, lanes);
  tds_lqr_mac(w.K, sx, 1, w.Qux, sx, 1, w.V, sx, w.V, sx, nx, nx, nu, lane, lanes);
  tds_lqr_mac(w.Qux, sx, 1, w.K, sx, 1, w.V, sx, w.V, sx, nx, nx, nu, lane, lanes);
  tds_lqr_mac(w.K, sx, 1, w.g, 1, 0, w.Qx, 1, w.Vx, 1, nx, 1, nu, lane, lanes);
  tds_lqr_mac(w.K, sx, 1, w.Qu, 1, 0, w.Vx, 1, w.Vx, 1, nx, 1, nu, lane, lanes);
  tds_lqr_mac(w.Qux, sx, 1, w.k, 1, 0, w.Vx, 1, w.Vx, 1, nx, 1, nu, lane, lanes);
  if (lane == lanes - 1) {
    double d1 = 0.0, d2 = 0.0;
    for (int a = 0; a < nu; ++a) d1 += w.k[a] * w.Qu[a];
    for (int a = 0; a < nu; ++a) d2 += w.k[a] * w.g[a];
    w.dv[0] += d1;
    w.dv[1] += 0.5 * d2;
  }
  sync();
  // (7) V_xx <- (V_xx + V_xx^T) / 2: the lane of (i, j), i < j, writes both
  for (int e = lane; e < nx * nx; e += lanes) {
    const int i = e / nx, j = e - i * nx;
    if (i < j) {
      const double m = 0.5 * (w.V[i * sx + j] + w.V[j * sx + i]);
      w.V[i * sx + j] = m;
      w.V[j * sx + i] = m;
    }
  }
  sync();
  return 0;
}

// The feedback law of the closed-loop rollout, one action: (u_nom + alpha k) + K (s - s_nom), the sum in index order
TDS_HD inline double tds_feedback_action(double u_nom, double alpha, double k, const double *K_row, const double *s,
                                         const double *s_nom, int nsd) {
  double d = 0.0;
  for (int j = 0; j < nsd; ++j) d += K_row[j] * (s[j] - s_nom[j]);
  return (u_nom + alpha * k) + d;
}

}  // namespace
