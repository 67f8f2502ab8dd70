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
struct TdsLqrWs {
  int nx, nu, sx, su;
  double *V, *A, *B, *W, *WB, *Qxx, *Qux, *Quu, *L, *K, *Vx, *Qx, *Qu, *k, *g, *dv;
};

TDS_HD inline size_t tds_lqr_ws_doubles(int nx, int nu) {
  const size_t sx = nx | 1, su = nu | 1, mx = nx > nu ? nx : nu;
  return 3 * nx * sx + mx * sx + 2 * nx * su + 2 * nu * sx + 2 * nu * su + 2 * nx + 3 * nu + 2;
}

TDS_HD inline TdsLqrWs tds_lqr_ws(double *p, int nx, int nu) {
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
  w.dv = p;
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

// One step of the recursion.  On entry the workspace holds V, Vx (of step t + 1), A, B, and lxx, lux, luu, lx, lu in
// Qxx, Qux, Quu, Qx, Qu; on return V, Vx are those of step t, K and k the gains, dv the sums so far.  Returns 0, or 1
// where a pivot of the Cholesky was not positive (every lane returns the same: each forms the pivot itself).
template <class Sync>
TDS_HD inline __attribute__((always_inline)) int tds_lqr_step(const TdsLqrWs &w, double mu, int lane, int lanes, Sync sync) {
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
  // (4) K = -(L L^T)^-1 Q_ux, k = -(L L^T)^-1 Q_u: a column per lane, the column in registers (loops of constant
  //     extent, unrolled: nothing indexed at run time)
  for (int c = lane; c <= nx; c += lanes) {
    const bool vec = c == nx;
    double *dst = vec ? w.k : w.K + c;
    const double *rhs = vec ? w.Qu : w.Qux + c;
    const int st = vec ? 1 : sx;
    double x[TDS_LQR_MAX_NU];
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
#pragma unroll
    for (int a = 0; a < TDS_LQR_MAX_NU; ++a)
      if (a < nu) dst[a * st] = -x[a];
  }
  sync();
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
