// tds_lm.h — the statement of the batched Levenberg-Marquardt step of system identification (tds_lm.hip; C ABI
// tds_hip_lm_step and its _host checker, include/tds_hip.h).
//
// Three pieces are the device wavefront's and the host checker's alike: tds_lm_stage (what an entry contributes),
// TdsLmSums (the running sums of cost, g and H over a staged tile) and tds_lm_solve (damping, the box QP per candidate,
// the outputs), each over (lane, lanes) with `sync` between the phases: 64 lanes of one wavefront over a workspace in
// LDS on the device, lane 0 of 1 over a workspace of the same layout in memory on the host.  Every sum is ONE sequential
// sum in the order (row ascending, entry ascending), owned by one lane; with the unit built without FP contraction the
// device and the host round alike.  The box QP, its factorisation and its solves are tds_lqr.h's, called as they stand:
// A = H + lambda diag(D) is written where the QP reads Q_uu, mu = 0, and nx = 0 leaves no gain columns.
#pragma once
#include "tds_lqr.h"

namespace {

// a tile: TDS_LM_TILE consecutive entries of the problem's (row, entry) sequence, p + 1 rows of them: c_0 .. c_{p-1}
// and a.  The rows are TDS_LM_STRIDE doubles apart: the lanes of a wavefront read the SAME entry of different rows, and
// with an odd stride the 17 rows fall on 17 different 8-byte bank slots of a 32-lane half.
constexpr int TDS_LM_TILE = 64, TDS_LM_STRIDE = 65;
constexpr int TDS_LM_MAX_SUMS = (TDS_LM_MAX_P + 1) * (TDS_LM_MAX_P + 2) / 2;  // 153
// Ceres's min_lm_diagonal / max_lm_diagonal
constexpr double TDS_LM_MIN_DIAG = 1e-6, TDS_LM_MAX_DIAG = 1e32;

// The workspace of one problem, in doubles:
//   tile [p + 1][65]   the staged tile; dead once the sums stand, then the box QP's workspace (tds_lqr_ws(0, p, box):
//                      14 p + 2 + 2 p (p | 1) doubles, 770 at p = 16, below the tile's 1105)
//   H [p][su], su = p | 1;   g [p];   D [p];   hd [p] (H delta);   cost [2]
// p = 16: 1105 + 272 + 3 * 16 + 2 = 1427 doubles = 11416 bytes.
struct TdsLmWs {
  int p, su;
  double *tile, *H, *g, *D, *hd, *cost;
  TdsLqrWs qp;
};

TDS_HD inline size_t tds_lm_ws_doubles(int p) {
  return (size_t)(p + 1) * TDS_LM_STRIDE + (size_t)p * (p | 1) + 3 * (size_t)p + 2;
}

TDS_HD inline TdsLmWs tds_lm_ws(double *mem, int p) {
  TdsLmWs w;
  w.p = p, w.su = p | 1;
  w.tile = mem, mem += (p + 1) * TDS_LM_STRIDE;
  w.H = mem, mem += p * w.su;
  w.g = mem, mem += p;
  w.D = mem, mem += p;
  w.hd = mem, mem += p;
  w.cost = mem;
  w.qp = tds_lqr_ws(w.tile, 0, p, true);
  return w;
}

TDS_HD inline bool tds_lm_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// Entry `col` of the tile from one entry of the data: wt == 0 skips it (zeros are staged: a sum that begins at +0 is
// not changed by them), whatever s_obs and js hold there; else a = wt (s - s_obs), c_i = wt js_i.  js: the entry's
// derivatives, in registers on the device (a loop of constant extent, unrolled: nothing indexed at run time).
TDS_HD inline __attribute__((always_inline)) void tds_lm_stage(const TdsLmWs &w, int col, double wt, double s, double s_obs,
                                                              const double (&js)[TDS_LM_MAX_P]) {
  const int p = w.p;
  const bool skip = wt == 0.0;
#pragma unroll
  for (int i = 0; i < TDS_LM_MAX_P; ++i)
    if (i < p) w.tile[i * TDS_LM_STRIDE + col] = skip ? 0.0 : wt * js[i];
  w.tile[p * TDS_LM_STRIDE + col] = skip ? 0.0 : wt * (s - s_obs);
}

// The (p + 1)(p + 2) / 2 running sums over the rows of the tile, sum q = i (i + 1) / 2 + j being row i times row j
// (j <= i; row p is a): H_ij, g_j = (p, j), and the sum of a^2 = (p, p).  Lane `lane` OWNS the sums lane, lane +
// lanes, ..: SLOTS bounds their number (the device: 3 registers at 64 lanes; the host: all 153).  Ownership splits the
// work, never a sum.
template <int SLOTS>
struct TdsLmSums {
  double acc[SLOTS];
  int ri[SLOTS], rj[SLOTS];
  int ns;  // the slots in use, the same in every lane

  TDS_HD inline void init(int p, int lane, int lanes) {
    const int nsums = (p + 1) * (p + 2) / 2;
    ns = (nsums + lanes - 1) / lanes;
#pragma unroll
    for (int k = 0; k < SLOTS; ++k) {
      const int q = lane + k * lanes;
      int i = 0;
      for (int r = 1; r <= TDS_LM_MAX_P; ++r)
        if (q < nsums && r * (r + 1) / 2 <= q) i = r;
      const int j = q < nsums ? q - i * (i + 1) / 2 : 0;
      ri[k] = i * TDS_LM_STRIDE, rj[k] = j * TDS_LM_STRIDE;  // (a slot without a sum reads row 0 and is not stored)
      acc[k] = 0.0;
    }
  }

  // the tile's entries 0 .. cnt - 1, in that order, onto every sum
  template <int NS>
  TDS_HD inline __attribute__((always_inline)) void add_slots(const double *tile, int cnt) {
#pragma unroll 4
    for (int e = 0; e < cnt; ++e) {
#pragma unroll
      for (int k = 0; k < NS; ++k) acc[k] += tile[ri[k] + e] * tile[rj[k] + e];
    }
  }
  TDS_HD inline __attribute__((always_inline)) void add(const double *tile, int cnt) {
    if constexpr (SLOTS == 3) {  // (the device: a loop of constant extent per number of slots in use)
      if (ns == 1) add_slots<1>(tile, cnt);
      else if (ns == 2) add_slots<2>(tile, cnt);
      else add_slots<3>(tile, cnt);
    } else {
      for (int e = 0; e < cnt; ++e)
        for (int k = 0; k < ns; ++k) acc[k] += tile[ri[k] + e] * tile[rj[k] + e];
    }
  }

  // the lower triangle of H, g and cost[0] = the sum of a^2
  TDS_HD inline void store(const TdsLmWs &w, int lane, int lanes) const {
    const int p = w.p, nsums = (p + 1) * (p + 2) / 2;
#pragma unroll
    for (int k = 0; k < SLOTS; ++k) {
      if (lane + k * lanes >= nsums) continue;
      const int i = ri[k] / TDS_LM_STRIDE, j = rj[k] / TDS_LM_STRIDE;
      if (i < p) w.H[i * w.su + j] = acc[k];
      else if (j < p) w.g[j] = acc[k];
      else w.cost[0] = acc[k];
    }
  }
};

// one problem's inputs beside the sums and its outputs, each at the problem's first entry
struct TdsLmProblem {
  int n_lambda;
  const double *dlo, *dhi, *lambda;  // dlo, dhi NULL: no bounds
  double *cost, *g, *H, *delta, *pred;
  int32_t *clamped, *qp_iterations, *status;
};

// From the sums (tds_lm_sums::store, then a sync) to the outputs.  cost = sum a^2 / 2.  A cost or a diagonal entry of H
// that is not finite (a counted entry that is not finite always makes one; so does one whose square overflows) is
// status 2 for every candidate: cost = +inf, everything else zero.  Else D_i = min(max(H_ii, 1e-6), 1e32) and per
// candidate l: A = H + lambda_l diag(D), delta_l = argmin delta^T A delta / 2 + g^T delta over dlo <= delta <= dhi by
// tds_lqr_qp from clamp(0), pred_l = -(g^T delta_l + delta_l^T H delta_l / 2) (the undamped H; every sum in index
// order); a pivot that is not positive: status 1, delta_l = 0, pred_l = 0.  p = 0: the cost alone.
template <class Sync>
TDS_HD inline __attribute__((always_inline)) void tds_lm_solve(const TdsLmWs &w, const TdsLmProblem &o, int lane, int lanes, Sync sync) {
  const int p = w.p, su = w.su, L = o.n_lambda;
  // H's upper triangle from its lower one
  for (int e = lane; e < p * p; e += lanes) {
    const int i = e / p, j = e - i * p;
    if (i < j) w.H[i * su + j] = w.H[j * su + i];
  }
  sync();
  int bad = !tds_lm_finite(w.cost[0]);
  for (int i = 0; i < p; ++i) bad |= !tds_lm_finite(w.H[i * su + i]);
  bad = tds_lqr_uniform(bad);
  if (lane == 0) *o.cost = bad ? INFINITY : 0.5 * w.cost[0];
  if (p == 0) return;
  for (int e = lane; e < p * p; e += lanes) {
    const int i = e / p, j = e - i * p;
    o.H[e] = bad ? 0.0 : w.H[i * su + j];
  }
  for (int i = lane; i < p; i += lanes) o.g[i] = bad ? 0.0 : w.g[i];
  if (bad) {
    for (int e = lane; e < L * p; e += lanes) o.delta[e] = 0.0;
    for (int l = lane; l < L; l += lanes) o.pred[l] = 0.0, o.clamped[l] = 0, o.qp_iterations[l] = 0, o.status[l] = 2;
    return;
  }
  const TdsLqrWs &q = w.qp;
  for (int i = lane; i < p; i += lanes) {
    const double h = w.H[i * su + i];
    w.D[i] = h < TDS_LM_MIN_DIAG ? TDS_LM_MIN_DIAG : (h > TDS_LM_MAX_DIAG ? TDS_LM_MAX_DIAG : h);
    q.dlo[i] = o.dlo ? o.dlo[i] : -INFINITY;
    q.dhi[i] = o.dhi ? o.dhi[i] : INFINITY;
  }
  sync();
  for (int l = 0; l < L; ++l) {
    const double lambda = o.lambda[l];
    for (int e = lane; e < p * p; e += lanes) {
      const int i = e / p, j = e - i * p;
      q.Quu[i * su + j] = i == j ? w.H[i * su + i] + lambda * w.D[i] : w.H[i * su + j];
    }
    for (int i = lane; i < p; i += lanes) q.Qu[i] = w.g[i], q.k[i] = 0.0;
    sync();
    unsigned set = 0;
    int iters = 0;
    const int failed = tds_lqr_qp(q, 0.0, lane, lanes, sync, &set, &iters);
    sync();
    if (failed) {
      for (int i = lane; i < p; i += lanes) o.delta[l * p + i] = 0.0;
      if (lane == 0) o.pred[l] = 0.0, o.clamped[l] = 0, o.qp_iterations[l] = 0, o.status[l] = 1;
    } else {
      for (int i = lane; i < p; i += lanes) {
        double s = 0.0;
        for (int b = 0; b < p; ++b) s += w.H[i * su + b] * q.k[b];
        w.hd[i] = s;
        o.delta[l * p + i] = q.k[i];
      }
      sync();
      if (lane == 0) {
        double d1 = 0.0, d2 = 0.0;
        for (int i = 0; i < p; ++i) d1 += w.g[i] * q.k[i];
        for (int i = 0; i < p; ++i) d2 += q.k[i] * w.hd[i];
        o.pred[l] = -(d1 + 0.5 * d2);
        o.clamped[l] = (int32_t)set, o.qp_iterations[l] = iters, o.status[l] = 0;
      }
    }
    sync();  // (every lane has read this candidate's step before the next one's system is written)
  }
}

}  // namespace
