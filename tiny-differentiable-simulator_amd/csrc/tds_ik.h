// tds_ik.h — one single-source statement of batched inverse kinematics (tds_ik.hip): the reference's
// TinyInverseKinematics::compute (tiny_inverse_kinematics.h:140-247) for one environment, instantiated over double on
// the host (the checker) and on the device.  "ref:" = file:line under the reference's src/.
//
// The kinematics and the point Jacobians are those of tds_dyn.h (tds_dyn_kinematics, tds_dyn_point_jacobian), read only,
// over a layout of IK's own: a TdsDynLayout in which only the offsets those two functions touch are filled (q, pt, xp,
// xw, base, jac), followed by the targets, the reference configuration, the stacked J [3K][dof_qd], A = J J^T [3K][3K],
// a factor of the same size and a few vectors.  Like there, the state is reached through TdsDynMem ([component][lane] on
// the device), every loop is wave-uniform in its component index, and nothing indexed at run time is kept in a local
// array: the 3K x 3K systems and the pivot bookkeeping live in the work buffer.
//
// FRAME.  The reference works in the base frame (links_X_base, base_X_world.apply_inverse); tds_dyn_point_jacobian gives
// world-frame columns, and this statement stays in the world frame: J and e are the reference's rotated by the base
// rotation R, so |e|, J^T e, J^+ e and J^T (J J^T + l^2)^-1 e are the reference's up to round-off.
#pragma once
#include "tds_dyn.h"

struct TdsIkParams {
  int method, max_iterations, k, have_ref;
  double lambda, target_tolerance, step_tolerance, alpha, weight_reference;
  int links[TDS_IK_MAX_TARGETS];
  double pts[3 * TDS_IK_MAX_TARGETS];
};

// entry s k + c of a per-target table held in the kernel arguments, picked with constant indices: a run-time index
// moves the table to the private segment (52 B per lane, measured)
#define TDS_IK_PICK(a, k, s, c) \
  ((k) == 0 ? (a)[c] : (k) == 1 ? (a)[(s) + (c)] : (k) == 2 ? (a)[2 * (s) + (c)] : (a)[3 * (s) + (c)])

// (the 16384 states of a full launch, tds_query.h: 140 MB of the handle's work buffer for Laikago's four feet)
struct TdsIkLayout {
  TdsDynLayout d;  // q, pt, xp, xw, base, jac only
  int tgt, qref, J, A, F, e, z, y, dg, total;
};
static inline TDS_HD TdsIkLayout tds_ik_layout(const tds_model_t *m, int K) {
  const int nl = m->num_links, nd = m->dof_qd, M = 3 * K;
  TdsIkLayout L;
  TdsDynLayout &d = L.d;
  d.qd = d.qdd = d.tau = d.v = d.c = d.a = d.f = d.abi = d.base_v = d.base_f = d.base_abi = d.M = d.L = d.bias = d.rhs = -1;
  int o = 0;
  d.q = o, o += nd + 1;
  d.pt = o, o += 3;
  d.xp = o, o += 12 * nl;
  d.xw = o, o += 12 * nl;
  d.base = o, o += 12;
  d.jac = o, o += 3 * nd;
  d.total = o;
  L.tgt = o, o += M;
  L.qref = o, o += nd + 1;
  L.J = o, o += M * nd;
  L.A = o, o += M * M;  // J J^T; free once it is factored: the triangular T of the pinv route takes its place
  L.F = o, o += M * M;  // the factor
  L.e = o, o += M;
  L.z = o, o += M;
  L.y = o, o += M;
  L.dg = o, o += M;     // the pivoted factorisation's residual diagonal (< 0: row already taken as a pivot)
  L.total = o;
  return L;
}

// M x M at `F` (row stride M): F = C C^T in place, lower triangle, the loop of tds_dyn_solve; then x (M entries at `x`)
// <- F^-1 x, `reps` times.  A pivot <= 0 gives NaN (the caller's finiteness check then fails the environment).
template <typename T>
TDS_HD inline void tds_ik_chol_solve(TdsDynMem<T> w, int F, int M, int r, int x, int reps) {
  for (int i = 0; i < r; ++i)
    for (int j = i; j < r; ++j) {
      T s = w[F + i * M + j];
      for (int k = i - 1; k >= 0; --k) s = s - w[F + i * M + k] * w[F + j * M + k];
      if (i == j)
        w[F + i * M + i] = tds_sqrt(s);
      else
        w[F + j * M + i] = s / w[F + i * M + i];
    }
  for (int rep = 0; rep < reps; ++rep) {
    for (int i = 0; i < r; ++i) {
      T s = w[x + i];
      for (int k = 0; k < i; ++k) s = s - w[F + i * M + k] * w[x + k];
      w[x + i] = s / w[F + i * M + i];
    }
    for (int i = r - 1; i >= 0; --i) {
      T s = w[x + i];
      for (int k = i + 1; k < r; ++k) s = s - w[F + k * M + i] * w[x + k];
      w[x + i] = s / w[F + i * M + i];
    }
  }
}

// z (at L.z) = A^+ e for the symmetric positive semidefinite A = J J^T at L.A, any rank: diagonally pivoted Cholesky
// A = Lf Lf^T with Lf [M][r] (rows in A's own order, so no permutation is applied afterwards), stopped at the first
// pivot <= eps M dof_qd (largest pivot), i.e. the rounding of a dof_qd-term dot product into each entry of A, M times
// over; then, with Lf = U T (U [M][r] with orthonormal columns, T [r][r] upper triangular), A^+ = U T^-T T^-1 U^T: two
// triangular solves with T, whose condition is J's own, so that the answer carries eps cond(J)^2 like a least-squares
// solve, where Lf (Lf^T Lf)^-2 Lf^T through the Gram matrix would carry eps cond(J)^4.  The pivot is each lane's own:
// reads of A's and Lf's row p are gathers from the work buffer (one run where the wave's lanes agree on p).
template <typename T>
TDS_HD inline void tds_ik_psd_pinv_mul(TdsDynMem<T> w, const TdsIkLayout &L, int M, int nd) {
  const int A = L.A, F = L.F, dg = L.dg;
  T big = T(0.0);
  for (int i = 0; i < M; ++i) {
    const T v = w[A + i * M + i];
    w[dg + i] = v;
    if (v > big) big = v;
  }
  const T thr = (2.220446049250313e-16 * (M * nd)) * big;
  int r = 0;
  for (int s = 0; s < M; ++s) {
    T best = T(-1.0);
    int p = 0;
    for (int i = 0; i < M; ++i) {
      const T v = w[dg + i];
      if (v > best) best = v, p = i;
    }
    if (!(best > thr)) break;
    const T piv = tds_sqrt(best);
    for (int i = 0; i < M; ++i) {
      const T v = w[dg + i];
      T l = T(0.0);
      if (i == p) {
        l = piv;
      } else if (!(v < 0.0)) {
        l = w[A + i * M + p];
        for (int t = 0; t < s; ++t) l = l - w[F + i * M + t] * w[F + p * M + t];
        l = l / piv;
        w[dg + i] = v - l * l;
      }
      w[F + i * M + s] = l;
    }
    w[dg + p] = T(-1.0);
    r = s + 1;
  }
  // Lf = U T by modified Gram-Schmidt on its r columns: U (orthonormal columns) takes Lf's place, T [r][r] (upper
  // triangle) A's; y = U^T e on the way
  for (int a = 0; a < r; ++a) {
    for (int b = 0; b < a; ++b) {
      T t = T(0.0);
      for (int i = 0; i < M; ++i) t = t + w[F + i * M + b] * w[F + i * M + a];
      w[A + b * M + a] = t;
      for (int i = 0; i < M; ++i) w[F + i * M + a] = w[F + i * M + a] - t * w[F + i * M + b];
    }
    T nn = T(0.0);
    for (int i = 0; i < M; ++i) nn = nn + w[F + i * M + a] * w[F + i * M + a];
    nn = tds_sqrt(nn);
    w[A + a * M + a] = nn;
    T s = T(0.0);
    for (int i = 0; i < M; ++i) {
      const T u = w[F + i * M + a] / nn;
      w[F + i * M + a] = u;
      s = s + u * w[L.e + i];
    }
    w[L.y + a] = s;
  }
  for (int i = r - 1; i >= 0; --i) {  // T v = y
    T s = w[L.y + i];
    for (int k = i + 1; k < r; ++k) s = s - w[A + i * M + k] * w[L.y + k];
    w[L.y + i] = s / w[A + i * M + i];
  }
  for (int i = 0; i < r; ++i) {  // T^T u = v
    T s = w[L.y + i];
    for (int k = 0; k < i; ++k) s = s - w[A + k * M + i] * w[L.y + k];
    w[L.y + i] = s / w[A + i * M + i];
  }
  for (int i = 0; i < M; ++i) {  // z = U u
    T s = T(0.0);
    for (int a = 0; a < r; ++a) s = s + w[F + i * M + a] * w[L.y + a];
    w[L.z + i] = s;
  }
}

// One environment: q_init at L.d.q, the targets at L.tgt and, with o.have_ref, the reference configuration at L.qref are
// in place; afterwards q is at L.d.q.  ref: tiny_inverse_kinematics.h:140-247.
template <typename T>
TDS_HD inline void tds_ik_solve(const tds_model_t *m, TdsDynMem<T> w, const TdsIkLayout &L, const TdsIkParams &o,
                                int &iterations, int &status, T &residual) {
  const int nd = m->dof_qd, K = o.k, M = 3 * K;
  const int qo = m->is_floating ? 7 : 0, vo = m->is_floating ? 6 : 0;  // :150-151
  int it = 0, st = TDS_IK_FAILED;
  T res = T(-1.0);  // :144
  for (; it < o.max_iterations; ++it) {
    tds_dyn_kinematics(m, TdsBlobView{}, w, L.d, 0);  // :162
    T ss = T(0.0);
    for (int k = 0; k < K; ++k) {
      const int li = TDS_IK_PICK(o.links, k, 1, 0);
      T pt[3] = {T(TDS_IK_PICK(o.pts, k, 3, 0)), T(TDS_IK_PICK(o.pts, k, 3, 1)), T(TDS_IK_PICK(o.pts, k, 3, 2))}, r[3];
      for (int c = 0; c < 3; ++c) w[L.d.pt + c] = pt[c];
      tds_dyn_point_jacobian(m, w, L.d, li, 1);  // :167
      TdsDXf<T> X;
      tds_dyn_ld(w, L.d.xw + 12 * li, X);
      tds_d_mulv(X.r, pt, r);
      for (int c = 0; c < 3 * nd; ++c)  // :169-177 the base's columns zeroed, :181-186
        w[L.J + 3 * k * nd + c] = c % nd < vo ? T(0.0) : w[L.d.jac + c];
      const T d0 = w[L.tgt + 3 * k] - (X.t[0] + r[0]);  // :187
      const T d1 = w[L.tgt + 3 * k + 1] - (X.t[1] + r[1]);
      const T d2 = w[L.tgt + 3 * k + 2] - (X.t[2] + r[2]);
      w[L.e + 3 * k] = d0, w[L.e + 3 * k + 1] = d1, w[L.e + 3 * k + 2] = d2;
      ss = ((ss + d0 * d0) + d1 * d1) + d2 * d2;
    }
    res = tds_sqrt(ss);  // :192
    if (res < o.target_tolerance) {  // :194
      st = TDS_IK_REACHED;
      break;
    }
    int zv = L.e;  // delta = J^T (the vector at zv)
    if (o.method != TDS_IK_TRANSPOSE) {
      for (int i = 0; i < M; ++i)  // A = J J^T, both triangles
        for (int j = 0; j <= i; ++j) {
          T s = T(0.0);
          for (int c = vo; c < nd; ++c) s = s + w[L.J + i * nd + c] * w[L.J + j * nd + c];
          w[L.A + i * M + j] = s, w[L.A + j * M + i] = s;
        }
      zv = L.z;
      if (o.method == TDS_IK_PINV) {  // :206-208
        tds_ik_psd_pinv_mul(w, L, M, nd);
      } else {  // :213-225
        for (int i = 0; i < M; ++i) {
          w[L.A + i * M + i] = w[L.A + i * M + i] + o.lambda * o.lambda;
          w[L.z + i] = w[L.e + i];
        }
        tds_ik_chol_solve(w, L.A, M, M, L.z, 1);
      }
    }
    T sq = T(0.0);
    for (int j = vo; j < nd; ++j) {  // :229-238
      T d = T(0.0);
      for (int i = 0; i < M; ++i) d = d + w[L.J + i * nd + j] * w[zv + i];
      T qi = w[L.d.q + qo + j - vo];
      qi = qi + o.alpha * d;
      if (o.have_ref) qi = qi + o.weight_reference * (w[L.qref + qo + j - vo] - qi);
      w[L.d.q + qo + j - vo] = qi;
      sq = sq + d * d;
    }
    if (!(sq - sq == 0.0)) {  // q is no longer finite: where the reference's loop ends
      it = o.max_iterations;
      break;
    }
    if (sq < o.step_tolerance * o.step_tolerance) {  // :240
      st = TDS_IK_CONVERGED;
      break;
    }
  }
  iterations = it, status = st, residual = res;
}
