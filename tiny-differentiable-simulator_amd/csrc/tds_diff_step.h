// tds_diff_step.h — one single-source, scalar-templated statement of the per-environment step (forward_zero) for the
// step Jacobians.  Instantiated over double (host: the checker against the reference), over TdsDual<K>
// (tds_dual.h; host and device: K directional derivatives per evaluation, tds_jvp.hip) and over TdsRev (tds_rev.h,
// tds_vjp.hip).  The model's selectable parameters are read through a view (TdsBlobView: the blob's values;
// TdsOverlayView: T-typed copies with active theta, the parameter derivatives of tds_dparam.hip).
//
// WHAT THE DERIVATIVE IS.  J = dy/dx of forward_zero per environment, x = the reference record [input_dim] (q, qd,
// actions, and kp, kd, max_force where the record carries them), y = [output_dim].  It is the derivative of the
// algorithm AS EXECUTED — what the reference's TinyDual / CppAD evaluations produce:
//   * clamps (action +-limit, max_force), the PGS projections and friction boxes, and the activation of a contact
//     (distance < 0) follow the branch the primal takes; at a switch the one-sided derivative of the taken branch is
//     returned;
//   * quaternion entries of x are differentiated raw: no projection onto the unit sphere (the reference's
//     quat_to_matrix scales by 2 / |q|^2, so the rotation does not change along q, but integrate_euler's
//     normalisation and the record's raw copy do).
//
// SCOPE.  One articulated body, fixed or floating base, 1-DoF and fixed joints, LOCOMOTION (PD) or TAU actuation,
// plane contacts with spheres, capsules and boxes, any pgs_iterations.  tds_diff_check() refuses the rest (spherical
// joints, worlds of several bodies).  The model is read from the C-ABI blob tds_model_t (include/tds_hip.h) — the
// expanded DevModel of the fast kernels restates a floating base as six pseudo links, which is not the formulation
// the reference differentiates.
//
// The array sizes are template bounds (TdsDiffBounds: links, dofs, contact points, visuals), not TDS_MAX_*: on the
// device the work object is indexed at run time and lives in memory (tds_jvp.hip), so its size is what a lane pays for.
//
// Formulation.  This follows the reference function by function ("ref:" = file:line under the reference's src/), with
// two restatements that change rounding only:
//   * ABI congruence X^T I X in 3x3 blocks instead of dense 6x6 products (forward_dynamics.hpp:187-189,
//     mass_matrix.hpp:45-46);
//   * M^-1 is never formed: M = L L^T (the reference's Cholesky, tiny_matrix_x.h:240-345) and W = M^-1 J^T by two
//     triangular solves; PGS reads A_ij = J_i . W_j + cfm delta_ij through u = W p (mb_constraint_solver.hpp:101-142,
//     :397-410), and the impulse's velocity change is W p (:476-496).
#pragma once
#include "tds_dual.h"
#include "tds_hip.h"

template <int NL_, int ND_, int NC_, int NV_>
struct TdsDiffBounds {
  static constexpr int NL = NL_;      // links
  static constexpr int ND = ND_;      // dof_qd
  static constexpr int NC = NC_;      // plane contact points (sphere 1, capsule 2, box 8)
  static constexpr int NV = NV_;      // visuals
  static constexpr int NR = 3 * NC_;  // constraint rows: normal | friction 1 | friction 2
  static constexpr int NX = 3 * ND_ + 4;            // record x: q | qd | actions (| kp kd max_force)
  static constexpr int NY = 2 * ND_ + 2 + 7 * NV_;  // written part of y: q | qd | visuals | up . z
};

template <typename T>
struct TdsDXf {  // Transform: rotation (row-major), translation
  T r[9], t[3];
};
template <typename T>
struct TdsDSv {  // spatial vector: angular | linear
  T a[3], l[3];
};
template <typename T>
struct TdsDAbi {  // ArticulatedBodyInertia [I H; H^T M]
  T I[9], H[9], M[9];
};

// entries of y the step writes: q | qd | 7 per visual | up . z
static inline TDS_HD int tds_diff_ny(const tds_model_t *m) {
  return m->dof_q + m->dof_qd + (m->pack_visuals ? 7 * m->num_visuals + 1 : 0);
}

template <typename T, class B>
struct TdsDiffWork {
  TdsDXf<T> Xp[B::NL], Xw[B::NL];  // X_parent, X_world
  TdsDSv<T> v[B::NL], c[B::NL], pA[B::NL], U[B::NL];  // (v also holds the accelerations a of the ABA's last pass)
  TdsDAbi<T> abi[B::NL];
  T D[B::NL], u[B::NL];
  TdsDXf<T> base;
  TdsDSv<T> base_v, base_bias;
  TdsDAbi<T> base_abi;
  T q[B::ND + 1], qd[B::ND], qdd[B::ND], tau[B::ND];
  T L[B::ND * B::ND];  // Cholesky factor of the joint-space inertia (lower, row-major)
  int n_c, cp_link[B::NC];
  T cp_b[B::NC][3], cp_dist[B::NC];
  T J[B::NR][B::ND], W[B::NR][B::ND];
  T b[B::NR], p[B::NR], jac[3][B::ND];
};

// 0: the model is in scope and fits bound B; else a nonzero code with `why` filled
template <class B>
static inline int tds_diff_check(const tds_model_t *m, const char **why) {
  int nsph = 0, nc = 0;
  for (int i = 0; i < m->num_links && i < TDS_MAX_LINKS; ++i) nsph += m->links[i].joint_type == TDS_JOINT_SPHERICAL;
  for (int g = 0; m->has_plane && g < m->num_geoms && g < TDS_MAX_GEOMS; ++g)
    nc += m->geoms[g].type == TDS_GEOM_SPHERE ? 1 : m->geoms[g].type == TDS_GEOM_CAPSULE ? 2 : m->geoms[g].type == TDS_GEOM_BOX ? 8 : 0;
  if (m->num_bodies >= 2) return *why = "step Jacobians: worlds of several bodies are not supported", 1;
  if (nsph) return *why = "step Jacobians: spherical joints are not supported", 1;
  if (m->dof_q != m->dof_qd + (m->is_floating ? 1 : 0)) return *why = "step Jacobians: unexpected dof_q", 1;
  if (m->num_links > B::NL || m->dof_qd > B::ND || nc > B::NC || (m->pack_visuals && m->num_visuals > B::NV) ||
      m->input_dim > B::NX || tds_diff_ny(m) > B::NY ||
      m->output_dim < tds_diff_ny(m))
    return *why = "step Jacobians: model exceeds the bound", 2;
  return 0;
}

// ---------------------------------------------------------------- 3x3 helpers
template <typename T>
TDS_HD inline void tds_d_cross(const T *a, const T *b, T *o) {
  T r0 = a[1] * b[2] - a[2] * b[1], r1 = a[2] * b[0] - a[0] * b[2], r2 = a[0] * b[1] - a[1] * b[0];
  o[0] = r0, o[1] = r1, o[2] = r2;
}
template <typename T, typename U>
TDS_HD inline void tds_d_mulv(const U *m, const T *v, T *o) {  // o = m v
  T r[3];
  for (int i = 0; i < 3; ++i) r[i] = m[3 * i] * v[0] + m[3 * i + 1] * v[1] + m[3 * i + 2] * v[2];
  o[0] = r[0], o[1] = r[1], o[2] = r[2];
}
template <typename T, typename U>
TDS_HD inline void tds_d_tmulv(const U *m, const T *v, T *o) {  // o = m^T v
  T r[3];
  for (int i = 0; i < 3; ++i) r[i] = m[i] * v[0] + m[3 + i] * v[1] + m[6 + i] * v[2];
  o[0] = r[0], o[1] = r[1], o[2] = r[2];
}
template <typename T, typename U, typename V>
TDS_HD inline void tds_d_mul(const U *a, const V *b, T *o) {  // o = a b (o may not alias)
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) o[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}
template <typename T>
TDS_HD inline void tds_d_tmul(const T *a, const T *b, T *o) {  // o = a^T b
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) o[3 * i + j] = a[i] * b[j] + a[3 + i] * b[3 + j] + a[6 + i] * b[6 + j];
}
template <typename T>
TDS_HD inline void tds_d_crossm(const T *v, T *m) {  // [v]x
  m[0] = T(0.0), m[1] = -v[2], m[2] = v[1];
  m[3] = v[2], m[4] = T(0.0), m[5] = -v[0];
  m[6] = -v[1], m[7] = v[0], m[8] = T(0.0);
}
// ref: math/tiny/tiny_matrix3x3.h:539-559 (cofactor inverse)
template <typename T>
TDS_HD inline void tds_d_inv3(const T *m, T *o) {
  T c0 = m[4] * m[8] - m[5] * m[7], c1 = m[5] * m[6] - m[3] * m[8], c2 = m[3] * m[7] - m[4] * m[6];
  T s = 1.0 / (m[0] * c0 + m[1] * c1 + m[2] * c2);
  o[0] = c0 * s, o[1] = (m[2] * m[7] - m[1] * m[8]) * s, o[2] = (m[1] * m[5] - m[2] * m[4]) * s;
  o[3] = c1 * s, o[4] = (m[0] * m[8] - m[2] * m[6]) * s, o[5] = (m[2] * m[3] - m[0] * m[5]) * s;
  o[6] = c2 * s, o[7] = (m[1] * m[6] - m[0] * m[7]) * s, o[8] = (m[0] * m[4] - m[1] * m[3]) * s;
}

// ---------------------------------------------------------------- quaternions (x, y, z, w)
// ref: math/tiny/tiny_matrix3x3.h:315-340 (setRotation: scaled by 2 / |q|^2)
template <typename T>
TDS_HD inline void tds_d_quat_to_matrix(const T *q, T *m) {
  T d = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  if (d == 0.0) return;
  T s = 2.0 / d;
  T xs = q[0] * s, ys = q[1] * s, zs = q[2] * s;
  T wx = q[3] * xs, wy = q[3] * ys, wz = q[3] * zs;
  T xx = q[0] * xs, xy = q[0] * ys, xz = q[0] * zs;
  T yy = q[1] * ys, yz = q[1] * zs, zz = q[2] * zs;
  m[0] = 1.0 - (yy + zz), m[1] = xy - wz, m[2] = xz + wy;
  m[3] = xy + wz, m[4] = 1.0 - (xx + zz), m[5] = yz - wx;
  m[6] = xz - wy, m[7] = yz + wx, m[8] = 1.0 - (xx + yy);
}
// ref: math/tiny/tiny_matrix3x3.h:432-465 (getRotation, right-associative: w negated)
template <typename T>
TDS_HD inline void tds_d_matrix_to_quat(const T *m, T *q) {
  T tr = m[0] + m[4] + m[8], e[4];
  if (tr < 0.0) {
    const int i = m[0] < m[4] ? (m[4] < m[8] ? 2 : 1) : (m[0] < m[8] ? 2 : 0);
    const int j = (i + 1) % 3, k = (i + 2) % 3;
    T s = tds_sqrt(((m[4 * i] - m[4 * j]) - m[4 * k]) + 1.0);
    e[i] = s * 0.5;
    s = 0.5 / s;
    e[3] = (m[3 * j + k] - m[3 * k + j]) * s;
    e[j] = (m[3 * i + j] + m[3 * j + i]) * s;
    e[k] = (m[3 * i + k] + m[3 * k + i]) * s;
  } else {
    T s = tds_sqrt(tr + 1.0);
    e[3] = s * 0.5;
    s = 0.5 / s;
    e[0] = (m[5] - m[7]) * s;
    e[1] = (m[6] - m[2]) * s;
    e[2] = (m[1] - m[3]) * s;
  }
  q[0] = e[0], q[1] = e[1], q[2] = e[2], q[3] = -e[3];
}
// ref: math/tiny/tiny_algebra.hpp:219-222
template <typename T>
TDS_HD inline void tds_d_quat_normalize(T *q) {
  T n = tds_sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int k = 0; k < 4; ++k) q[k] = q[k] / n;
}
// ref: math/tiny/tiny_quaternion.h:171-176, 306-345: (q v) q^-1
template <typename T, typename U>
TDS_HD inline void tds_d_quat_rotate(const T *q, const U *v, T *o) {
  T t0 = q[3] * v[0] + q[1] * v[2] - q[2] * v[1], t1 = q[3] * v[1] + q[2] * v[0] - q[0] * v[2];
  T t2 = q[3] * v[2] + q[0] * v[1] - q[1] * v[0], t3 = -q[0] * v[0] - q[1] * v[1] - q[2] * v[2];
  o[0] = -(t3 * q[0]) + t0 * q[3] - t1 * q[2] + t2 * q[1];
  o[1] = -(t3 * q[1]) + t1 * q[3] - t2 * q[0] + t0 * q[2];
  o[2] = -(t3 * q[2]) + t2 * q[3] - t0 * q[1] + t1 * q[0];
}

// ---------------------------------------------------------------- transforms and spatial algebra
// ref: math/transform.hpp:123-131: (A B).t = A.t + A.R B.t, (A B).R = A.R B.R
template <typename T, typename U, typename V>
TDS_HD inline void tds_d_xf_mul(const TdsDXf<T> &a, const U *br, const V *bt, TdsDXf<T> &o) {
  T rt[3];
  for (int i = 0; i < 3; ++i) rt[i] = a.r[3 * i] * bt[0] + a.r[3 * i + 1] * bt[1] + a.r[3 * i + 2] * bt[2];
  for (int k = 0; k < 3; ++k) o.t[k] = a.t[k] + rt[k];
  tds_d_mul(a.r, br, o.r);
}
// ref: math/transform.hpp:210-226: X v = (R^T w, R^T (v - r x w))
template <typename T>
TDS_HD inline void tds_d_apply_motion(const TdsDXf<T> &x, const TdsDSv<T> &in, TdsDSv<T> &o) {
  T rxw[3], d[3];
  tds_d_cross(x.t, in.a, rxw);
  for (int k = 0; k < 3; ++k) d[k] = in.l[k] - rxw[k];
  tds_d_tmulv(x.r, in.a, o.a);
  tds_d_tmulv(x.r, d, o.l);
}
// ref: math/transform.hpp:232-243: X^-1 v = (R w, R v + r x (R w)); `in` is a constant motion axis here
template <typename T>
TDS_HD inline void tds_d_apply_inverse_motion(const TdsDXf<T> &x, const double *S, TdsDSv<T> &o) {
  T c[3];
  for (int i = 0; i < 3; ++i) {
    o.a[i] = x.r[3 * i] * S[0] + x.r[3 * i + 1] * S[1] + x.r[3 * i + 2] * S[2];
    o.l[i] = x.r[3 * i] * S[3] + x.r[3 * i + 1] * S[4] + x.r[3 * i + 2] * S[5];
  }
  tds_d_cross(x.t, o.a, c);
  for (int k = 0; k < 3; ++k) o.l[k] = o.l[k] + c[k];
}
// ref: math/transform.hpp:249-262: X^T f = (R n + r x (R f), R f)
template <typename T>
TDS_HD inline void tds_d_apply_force(const TdsDXf<T> &x, const TdsDSv<T> &in, TdsDSv<T> &o) {
  T c[3], l[3], a[3];
  tds_d_mulv(x.r, in.l, l);
  tds_d_mulv(x.r, in.a, a);
  tds_d_cross(x.t, l, c);
  for (int k = 0; k < 3; ++k) o.a[k] = a[k] + c[k], o.l[k] = l[k];
}
// ref: math/tiny/tiny_algebra.hpp:101-105: v1 x v2 = (w1 x w2, w1 x v2 + v1 x w2)
template <typename T>
TDS_HD inline void tds_d_cross_mm(const TdsDSv<T> &x, const TdsDSv<T> &y, TdsDSv<T> &o) {
  T c1[3], c2[3];
  tds_d_cross(x.a, y.a, o.a);
  tds_d_cross(x.a, y.l, c1);
  tds_d_cross(x.l, y.a, c2);
  for (int k = 0; k < 3; ++k) o.l[k] = c1[k] + c2[k];
}
// ref: math/tiny/tiny_algebra.hpp:112-115: v x* f = (w x n + v x f, w x f)
template <typename T>
TDS_HD inline void tds_d_cross_mf(const TdsDSv<T> &x, const TdsDSv<T> &y, TdsDSv<T> &o) {
  T c1[3], c2[3];
  tds_d_cross(x.a, y.a, c1);
  tds_d_cross(x.l, y.l, c2);
  for (int k = 0; k < 3; ++k) o.a[k] = c1[k] + c2[k];
  tds_d_cross(x.a, y.l, o.l);
}
template <typename T>
TDS_HD inline T tds_d_dot6(const TdsDSv<T> &x, const TdsDSv<T> &y) {
  return (x.a[0] * y.a[0] + x.a[1] * y.a[1] + x.a[2] * y.a[2]) + (x.l[0] * y.l[0] + x.l[1] * y.l[1] + x.l[2] * y.l[2]);
}
template <typename T>
TDS_HD inline T tds_d_dot6c(const double *S, const TdsDSv<T> &y) {  // constant axis . y
  return (S[0] * y.a[0] + S[1] * y.a[1] + S[2] * y.a[2]) + (S[3] * y.l[0] + S[4] * y.l[1] + S[5] * y.l[2]);
}
// ref: math/inertia.hpp:121-130 (ABI of a rigid body: I + m [c]x [c]x^T, H = m [c]x, M = m 1)
template <typename T>
TDS_HD inline void tds_d_abi_rbi(double mass, const double *com, const double *inertia, TdsDAbi<T> &o) {
  const double H[9] = {0.0, -com[2], com[1], com[2], 0.0, -com[0], -com[1], com[0], 0.0};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const double hh = H[3 * i] * H[3 * j] + H[3 * i + 1] * H[3 * j + 1] + H[3 * i + 2] * H[3 * j + 2];
      o.I[3 * i + j] = T(inertia[3 * i + j] + hh * mass);
      o.H[3 * i + j] = T(H[3 * i + j] * mass);
      o.M[3 * i + j] = T(i == j ? mass : 0.0);
    }
}
// ref: math/inertia.hpp:205-210: IA v = (I w + H v, M v + H^T w)
template <typename T>
TDS_HD inline void tds_d_abi_mul(const TdsDAbi<T> &A, const TdsDSv<T> &v, TdsDSv<T> &o) {
  T t1[3], t2[3], t3[3], t4[3];
  tds_d_mulv(A.I, v.a, t1);
  tds_d_mulv(A.H, v.l, t2);
  tds_d_mulv(A.M, v.l, t3);
  tds_d_tmulv(A.H, v.a, t4);
  for (int k = 0; k < 3; ++k) o.a[k] = t1[k] + t2[k], o.l[k] = t3[k] + t4[k];
}
template <typename T>
TDS_HD inline void tds_d_abi_mulc(const TdsDAbi<T> &A, const double *S, TdsDSv<T> &o) {  // IA S, S constant
  for (int i = 0; i < 3; ++i) {
    o.a[i] = (A.I[3 * i] * S[0] + A.I[3 * i + 1] * S[1] + A.I[3 * i + 2] * S[2]) +
             (A.H[3 * i] * S[3] + A.H[3 * i + 1] * S[4] + A.H[3 * i + 2] * S[5]);
    o.l[i] = (A.M[3 * i] * S[3] + A.M[3 * i + 1] * S[4] + A.M[3 * i + 2] * S[5]) +
             (A.H[i] * S[0] + A.H[3 + i] * S[1] + A.H[6 + i] * S[2]);
  }
}
// P += X^T IA X (forward_dynamics.hpp:187-189, mass_matrix.hpp:45-46), in 3x3 blocks: with E = R^T and B = -E [r]x,
// X = [E 0; B E]:  I' = E^T (I E + H B) + B^T (H^T E + M B),  H' = E^T H E + B^T M E,  M' = E^T M E
template <typename T>
TDS_HD inline void tds_d_abi_congruence_add(const TdsDXf<T> &X, const TdsDAbi<T> &A, TdsDAbi<T> &P) {
  T E[9], rx[9], Bm[9], t1[9], t2[9], t3[9], Ht[9], R1[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) E[3 * i + j] = X.r[3 * j + i], Ht[3 * i + j] = A.H[3 * j + i];
  tds_d_crossm(X.t, rx);
  tds_d_mul(E, rx, Bm);
  for (int k = 0; k < 9; ++k) Bm[k] = -Bm[k];
  // I E + H B
  tds_d_mul(A.I, E, t1);
  tds_d_mul(A.H, Bm, t2);
  for (int k = 0; k < 9; ++k) t1[k] = t1[k] + t2[k];
  // H^T E + M B
  tds_d_mul(Ht, E, t2);
  tds_d_mul(A.M, Bm, t3);
  for (int k = 0; k < 9; ++k) t2[k] = t2[k] + t3[k];
  tds_d_tmul(E, t1, R1);
  tds_d_tmul(Bm, t2, t3);
  for (int k = 0; k < 9; ++k) P.I[k] = P.I[k] + (R1[k] + t3[k]);
  // H' = E^T (H E) + B^T (M E)
  tds_d_mul(A.H, E, t1);
  tds_d_tmul(E, t1, R1);
  tds_d_mul(A.M, E, t2);
  tds_d_tmul(Bm, t2, t3);
  for (int k = 0; k < 9; ++k) P.H[k] = P.H[k] + (R1[k] + t3[k]);
  tds_d_tmul(E, t2, R1);
  for (int k = 0; k < 9; ++k) P.M[k] = P.M[k] + R1[k];
}
// ref: math/inertia.hpp:302-329 ArticulatedBodyInertia::inverse() applied to f (the reference takes C = -H for the
// lower-left block, exact while H is skew; restated as is)
template <typename T>
TDS_HD inline void tds_d_abi_inv_mul(const TdsDAbi<T> &A, const TdsDSv<T> &f, TdsDSv<T> &o) {
  T Ainv[9], C[9], t1[9], t2[9], S[9], D[9], ABD[9], I2[9], a[3], b[3];
  tds_d_inv3(A.I, Ainv);
  for (int k = 0; k < 9; ++k) C[k] = -A.H[k];
  tds_d_mul(C, Ainv, t1);
  tds_d_mul(t1, A.H, t2);
  for (int k = 0; k < 9; ++k) S[k] = A.M[k] - t2[k];
  tds_d_inv3(S, D);
  tds_d_mul(Ainv, A.H, t1);
  tds_d_mul(t1, D, ABD);
  tds_d_mul(ABD, C, t1);
  tds_d_mul(t1, Ainv, t2);
  for (int k = 0; k < 9; ++k) I2[k] = Ainv[k] + t2[k];
  // o.a = I2 f.a - ABD f.l ;  o.l = D f.l - ABD^T f.a
  tds_d_mulv(I2, f.a, a);
  tds_d_mulv(ABD, f.l, b);
  for (int k = 0; k < 3; ++k) o.a[k] = a[k] - b[k];
  tds_d_mulv(D, f.l, a);
  tds_d_tmulv(ABD, f.a, b);
  for (int k = 0; k < 3; ++k) o.l[k] = a[k] - b[k];
}

// ---------------------------------------------------------------- parameter views
// Every read of a selectable model parameter (tds_param_t, include/tds_hip.h: masses, COMs, inertias, X_T
// translations, springs, gravity, friction, restitution, and the contact model's cfm, erp and collision shapes: radius,
// capsule length, box extents, X_trans) goes through a view P, passed by value.  TdsBlobView reads
// the blob as double constants: the code of the plain instantiations, tds_diff_step(m, w, x, y).  TdsOverlayView reads
// a TdsParamOverlay<T, B>: T-typed copies seeded from the blob (tds_param_seed), the selected entries replaced by
// active theta (tds_param_set); the overlay lives in the lane's work object (tds_dparam.hip).
// geom_scalar<T>: the type a view's shape reads have (the contact points' offsets are formed in it).
struct TdsBlobView {  // no state: passed by value, it adds nothing to the plain instantiations' code
  template <typename T>
  using geom_scalar = double;
  TDS_HD const double *xt(const tds_model_t *m, int i) const { return m->links[i].X_T_trans; }
  template <typename T>
  TDS_HD void link_rbi(const tds_model_t *m, int i, TdsDAbi<T> &o) const {
    const tds_link_t &l = m->links[i];
    tds_d_abi_rbi(l.mass, l.com, l.inertia, o);
  }
  template <typename T>
  TDS_HD void base_rbi(const tds_model_t *m, TdsDAbi<T> &o) const {
    tds_d_abi_rbi(m->base_mass, m->base_com, m->base_inertia, o);
  }
  TDS_HD const double *base_inertia(const tds_model_t *m) const { return m->base_inertia; }
  TDS_HD double stiffness(const tds_model_t *m, int i) const { return m->links[i].stiffness; }
  TDS_HD double damping(const tds_model_t *m, int i) const { return m->links[i].damping; }
  TDS_HD const double *gravity(const tds_model_t *m) const { return m->gravity; }
  template <typename T>
  TDS_HD T neg_gravity(const tds_model_t *m, int k) const { return T(-m->gravity[k]); }
  TDS_HD double friction(const tds_model_t *m) const { return m->friction; }
  TDS_HD double restitution(const tds_model_t *m) const { return m->restitution; }
  TDS_HD double cfm(const tds_model_t *m) const { return m->cfm; }
  TDS_HD double erp(const tds_model_t *m) const { return m->erp; }
  TDS_HD double geom_radius(const tds_model_t *m, int g) const { return m->geoms[g].radius; }
  TDS_HD double geom_length(const tds_model_t *m, int g) const { return m->geoms[g].length; }
  TDS_HD const double *geom_extents(const tds_model_t *m, int g) const { return m->geoms[g].extents; }
  TDS_HD const double *geom_trans(const tds_model_t *m, int g) const { return m->geoms[g].X_trans; }
};

// the rigid-body ABI of inertia.hpp:121-130 with T-typed mass, COM and inertia (tds_d_abi_rbi's expression order)
template <typename T>
TDS_HD inline void tds_d_abi_rbi_t(const T &mass, const T *com, const T *inertia, TdsDAbi<T> &o) {
  const T z = T(0.0);
  const T H[9] = {z, -com[2], com[1], com[2], z, -com[0], -com[1], com[0], z};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const T hh = H[3 * i] * H[3 * j] + H[3 * i + 1] * H[3 * j + 1] + H[3 * i + 2] * H[3 * j + 2];
      o.I[3 * i + j] = inertia[3 * i + j] + hh * mass;
      o.H[3 * i + j] = H[3 * i + j] * mass;
      o.M[3 * i + j] = i == j ? mass : z;
    }
}

template <typename T, class B>
struct TdsParamOverlay {
  T lxt[B::NL][3], lmass[B::NL], lcom[B::NL][3], linertia[B::NL][9], lstiff[B::NL], ldamp[B::NL];
  T bmass, bcom[3], binertia[9], grav[3], fric, rest;
  // the contact model: solver softness, and the shapes of the geoms that give contact points.  A shape's slot is its
  // rank among the model's spheres, capsules and boxes (gslot; -1: a geom without contact points, and every geom of a
  // model without a plane — nothing reads those).  Each has at least one point, so at most NC slots are in use.
  T cfm, erp, gradius[B::NC], glength[B::NC], gextent[B::NC][3], gtrans[B::NC][3];
  signed char gslot[TDS_MAX_GEOMS];
  T gspare;    // where the theta of a shape that nothing reads goes (tds_param_slot)
  T gnone[3];  // zeros: what the frame of a geom without contact points reads as its translation
};

// the view of an overlay (a pointer to it, passed by value); the model argument is not read
template <typename T, class B>
struct TdsOverlayView {
  const TdsParamOverlay<T, B> *o;
  TDS_HD const T *xt(const tds_model_t *, int i) const { return o->lxt[i]; }
  TDS_HD void link_rbi(const tds_model_t *, int i, TdsDAbi<T> &r) const {
    tds_d_abi_rbi_t(o->lmass[i], o->lcom[i], o->linertia[i], r);
  }
  TDS_HD void base_rbi(const tds_model_t *, TdsDAbi<T> &r) const { tds_d_abi_rbi_t(o->bmass, o->bcom, o->binertia, r); }
  TDS_HD const T *base_inertia(const tds_model_t *) const { return o->binertia; }
  TDS_HD const T &stiffness(const tds_model_t *, int i) const { return o->lstiff[i]; }
  TDS_HD const T &damping(const tds_model_t *, int i) const { return o->ldamp[i]; }
  TDS_HD const T *gravity(const tds_model_t *) const { return o->grav; }
  template <typename U>
  TDS_HD U neg_gravity(const tds_model_t *, int k) const { return -o->grav[k]; }
  TDS_HD const T &friction(const tds_model_t *) const { return o->fric; }
  TDS_HD const T &restitution(const tds_model_t *) const { return o->rest; }
  template <typename U>
  using geom_scalar = T;
  TDS_HD const T &cfm(const tds_model_t *) const { return o->cfm; }
  TDS_HD const T &erp(const tds_model_t *) const { return o->erp; }
  // (radius, length and extents are read for geoms with contact points only: their slots are >= 0.  The frame of a
  //  geom without contact points is formed and dropped, as it always was: its translation reads as 0)
  TDS_HD const T &geom_radius(const tds_model_t *, int g) const { return o->gradius[o->gslot[g]]; }
  TDS_HD const T &geom_length(const tds_model_t *, int g) const { return o->glength[o->gslot[g]]; }
  TDS_HD const T *geom_extents(const tds_model_t *, int g) const { return o->gextent[o->gslot[g]]; }
  TDS_HD const T *geom_trans(const tds_model_t *, int g) const { return o->gslot[g] < 0 ? o->gnone : o->gtrans[o->gslot[g]]; }
};

// whether a geom gives plane contact points (world.hpp:206-282 pairs it with the plane; meshes are ignored)
TDS_HD inline bool tds_geom_has_points(const tds_geom_t &G) {
  return G.type == TDS_GEOM_SPHERE || G.type == TDS_GEOM_CAPSULE || G.type == TDS_GEOM_BOX;
}

// the overlay holds the blob's values, all constant
template <typename T, class B>
TDS_HD inline void tds_param_seed(const tds_model_t *m, TdsParamOverlay<T, B> &o) {
  for (int i = 0; i < m->num_links; ++i) {
    const tds_link_t &l = m->links[i];
    for (int k = 0; k < 3; ++k) o.lxt[i][k] = T(l.X_T_trans[k]), o.lcom[i][k] = T(l.com[k]);
    for (int k = 0; k < 9; ++k) o.linertia[i][k] = T(l.inertia[k]);
    o.lmass[i] = T(l.mass), o.lstiff[i] = T(l.stiffness), o.ldamp[i] = T(l.damping);
  }
  o.bmass = T(m->base_mass);
  for (int k = 0; k < 3; ++k) o.bcom[k] = T(m->base_com[k]), o.grav[k] = T(m->gravity[k]);
  for (int k = 0; k < 9; ++k) o.binertia[k] = T(m->base_inertia[k]);
  o.fric = T(m->friction), o.rest = T(m->restitution);
  o.cfm = T(m->cfm), o.erp = T(m->erp), o.gspare = T(0.0);
  for (int k = 0; k < 3; ++k) o.gnone[k] = T(0.0);
  int ns = 0;
  for (int g = 0; g < m->num_geoms; ++g) {
    const tds_geom_t &G = m->geoms[g];
    o.gslot[g] = -1;
    if (!m->has_plane || !tds_geom_has_points(G) || ns >= B::NC) continue;  // (tds_diff_check: the points fit NC)
    o.gradius[ns] = T(G.radius), o.glength[ns] = T(G.length);
    for (int k = 0; k < 3; ++k) o.gextent[ns][k] = T(G.extents[k]), o.gtrans[ns][k] = T(G.X_trans[k]);
    o.gslot[g] = (signed char)ns++;
  }
}

// inertia entry `comp` (0..5 = xx, yy, zz, xy, xz, yz) of a row-major 3x3: its index and its mirror's
TDS_HD inline int tds_param_inertia_index(int comp, int mirror) {
  if (comp < 3) return 4 * comp;
  const int r = comp == 5 ? 1 : 0, c = comp == 3 ? 1 : 2;
  return mirror ? 3 * c + r : 3 * r + c;
}

// the overlay's entry (entries: an inertia entry and its mirror) of a selection; NULL for a kind it does not know.
// A shape the step does not read (no plane, or no contact points) has no slot of its own: its theta lands in
// o.gspare, which nothing reads, and its derivative is exactly zero.
template <typename T, class B>
TDS_HD inline T *tds_param_slot(TdsParamOverlay<T, B> &o, const tds_param_t &q, int mirror) {
  const int gs = q.kind >= TDS_PARAM_GEOM_RADIUS && q.kind <= TDS_PARAM_GEOM_TRANS ? o.gslot[q.link] : 0;
  if (gs < 0) return &o.gspare;
  switch (q.kind) {
    case TDS_PARAM_LINK_MASS: return &o.lmass[q.link];
    case TDS_PARAM_LINK_COM: return &o.lcom[q.link][q.comp];
    case TDS_PARAM_LINK_INERTIA: return &o.linertia[q.link][tds_param_inertia_index(q.comp, mirror)];
    case TDS_PARAM_LINK_XT_TRANS: return &o.lxt[q.link][q.comp];
    case TDS_PARAM_LINK_STIFFNESS: return &o.lstiff[q.link];
    case TDS_PARAM_LINK_DAMPING: return &o.ldamp[q.link];
    case TDS_PARAM_BASE_MASS: return &o.bmass;
    case TDS_PARAM_BASE_COM: return &o.bcom[q.comp];
    case TDS_PARAM_BASE_INERTIA: return &o.binertia[tds_param_inertia_index(q.comp, mirror)];
    case TDS_PARAM_GRAVITY: return &o.grav[q.comp];
    case TDS_PARAM_FRICTION: return &o.fric;
    case TDS_PARAM_RESTITUTION: return &o.rest;
    case TDS_PARAM_CFM: return &o.cfm;
    case TDS_PARAM_ERP: return &o.erp;
    case TDS_PARAM_GEOM_RADIUS: return &o.gradius[gs];
    case TDS_PARAM_GEOM_LENGTH: return &o.glength[gs];
    case TDS_PARAM_GEOM_EXTENT: return &o.gextent[gs][q.comp];
    case TDS_PARAM_GEOM_TRANS: return &o.gtrans[gs][q.comp];
    default: return nullptr;
  }
}

// selected entry q := t (both mirror entries of an off-diagonal inertia entry: the inertia stays symmetric)
template <typename T, class B>
TDS_HD inline void tds_param_set(TdsParamOverlay<T, B> &o, const tds_param_t &q, const T &t) {
  *tds_param_slot(o, q, 0) = t;
  *tds_param_slot(o, q, 1) = t;
}

// the blob's value of a (checked) selection
inline double tds_param_value(const tds_model_t *m, const tds_param_t &q) {
  const tds_link_t &l = m->links[q.kind <= TDS_PARAM_LINK_DAMPING ? q.link : 0];
  switch (q.kind) {
    case TDS_PARAM_LINK_MASS: return l.mass;
    case TDS_PARAM_LINK_COM: return l.com[q.comp];
    case TDS_PARAM_LINK_INERTIA: return l.inertia[tds_param_inertia_index(q.comp, 0)];
    case TDS_PARAM_LINK_XT_TRANS: return l.X_T_trans[q.comp];
    case TDS_PARAM_LINK_STIFFNESS: return l.stiffness;
    case TDS_PARAM_LINK_DAMPING: return l.damping;
    case TDS_PARAM_BASE_MASS: return m->base_mass;
    case TDS_PARAM_BASE_COM: return m->base_com[q.comp];
    case TDS_PARAM_BASE_INERTIA: return m->base_inertia[tds_param_inertia_index(q.comp, 0)];
    case TDS_PARAM_GRAVITY: return m->gravity[q.comp];
    case TDS_PARAM_FRICTION: return m->friction;
    case TDS_PARAM_CFM: return m->cfm;
    case TDS_PARAM_ERP: return m->erp;
    case TDS_PARAM_GEOM_RADIUS: return m->geoms[q.link].radius;
    case TDS_PARAM_GEOM_LENGTH: return m->geoms[q.link].length;
    case TDS_PARAM_GEOM_EXTENT: return m->geoms[q.link].extents[q.comp];
    case TDS_PARAM_GEOM_TRANS: return m->geoms[q.link].X_trans[q.comp];
    default: return m->restitution;
  }
}

// 0: the selection names p distinct scalars of the model; else why is set
inline int tds_param_check(const tds_model_t *m, int p, const tds_param_t *params, const char **why) {
  if (p < 0 || (p > 0 && !params)) return *why = "parameter derivatives: NULL or negative parameter selection", 1;
  for (int j = 0; j < p; ++j) {
    const tds_param_t &q = params[j];
    if (q.kind < TDS_PARAM_LINK_MASS || q.kind > TDS_PARAM_GEOM_TRANS ||
        (q.kind > TDS_PARAM_RESTITUTION && q.kind < TDS_PARAM_CFM))
      return *why = "parameter derivatives: unknown parameter kind", 1;
    const bool on_link = q.kind <= TDS_PARAM_LINK_DAMPING, on_geom = q.kind >= TDS_PARAM_GEOM_RADIUS;
    const int ncomp = q.kind == TDS_PARAM_LINK_INERTIA || q.kind == TDS_PARAM_BASE_INERTIA ? 6
                      : q.kind == TDS_PARAM_LINK_COM || q.kind == TDS_PARAM_LINK_XT_TRANS || q.kind == TDS_PARAM_BASE_COM ||
                                q.kind == TDS_PARAM_GRAVITY || q.kind == TDS_PARAM_GEOM_EXTENT || q.kind == TDS_PARAM_GEOM_TRANS
                          ? 3
                          : 1;
    if (on_geom) {
      if (q.link < 0 || q.link >= m->num_geoms || q.link >= TDS_MAX_GEOMS)
        return *why = "parameter derivatives: geom index out of range", 1;
      if (q.kind == TDS_PARAM_GEOM_LENGTH && m->geoms[q.link].type != TDS_GEOM_CAPSULE)
        return *why = "parameter derivatives: a length needs a capsule", 1;
      if (q.kind == TDS_PARAM_GEOM_EXTENT && m->geoms[q.link].type != TDS_GEOM_BOX)
        return *why = "parameter derivatives: an extent needs a box", 1;
      if (q.kind == TDS_PARAM_GEOM_RADIUS && !tds_geom_has_points(m->geoms[q.link]))
        return *why = "parameter derivatives: a radius needs a sphere, a capsule or a box", 1;
    } else if (on_link ? (q.link < 0 || q.link >= m->num_links) : q.link != 0) {
      return *why = "parameter derivatives: link index out of range", 1;
    }
    if (q.comp < 0 || q.comp >= ncomp) return *why = "parameter derivatives: component index out of range", 1;
    if (q.kind >= TDS_PARAM_BASE_MASS && q.kind <= TDS_PARAM_BASE_INERTIA && !m->is_floating)
      return *why = "parameter derivatives: base parameters need a floating base", 1;
    for (int i = 0; i < j; ++i)
      if (params[i].kind == q.kind && params[i].link == q.link && params[i].comp == q.comp)
        return *why = "parameter derivatives: duplicate parameter", 1;
  }
  return 0;
}

// ---------------------------------------------------------------- the step
// ref: link.hpp:229-287 (X_J, X_parent) for a 1-DoF or fixed joint
template <typename T, typename X>
TDS_HD inline void tds_d_jcalc(const tds_link_t &l, const X *xt, const T &q, TdsDXf<T> &Xp) {
  T R[9], tj[3] = {T(0.0), T(0.0), T(0.0)};
  for (int k = 0; k < 9; ++k) R[k] = T(k % 4 == 0 ? 1.0 : 0.0);
  switch (l.joint_type) {
    case TDS_JOINT_PRISMATIC_X: tj[0] = q; break;
    case TDS_JOINT_PRISMATIC_Y: tj[1] = q; break;
    case TDS_JOINT_PRISMATIC_Z: tj[2] = q; break;
    case TDS_JOINT_PRISMATIC_AXIS:
      for (int k = 0; k < 3; ++k) tj[k] = l.S[3 + k] * q;
      break;
    case TDS_JOINT_REVOLUTE_X: {  // tiny_matrix3x3.h:218-234
      T c = tds_cos(q), s = tds_sin(q);
      R[4] = c, R[5] = -s, R[7] = s, R[8] = c;
      break;
    }
    case TDS_JOINT_REVOLUTE_Y: {
      T c = tds_cos(q), s = tds_sin(q);
      R[0] = c, R[2] = s, R[6] = -s, R[8] = c;
      break;
    }
    case TDS_JOINT_REVOLUTE_Z: {
      T c = tds_cos(q), s = tds_sin(q);
      R[0] = c, R[1] = -s, R[3] = s, R[4] = c;
      break;
    }
    case TDS_JOINT_REVOLUTE_AXIS: {  // link.hpp:256-261, tiny_quaternion.h:178-183
      const double d = sqrt(l.S[0] * l.S[0] + l.S[1] * l.S[1] + l.S[2] * l.S[2]);
      T sh = tds_sin(q * 0.5) / d, qu[4] = {l.S[0] * sh, l.S[1] * sh, l.S[2] * sh, tds_cos(q * 0.5)};
      tds_d_quat_to_matrix(qu, R);
      break;
    }
    default: break;  // fixed: identity
  }
  // X_parent = X_T X_J (link.hpp:283)
  for (int k = 0; k < 3; ++k)
    Xp.t[k] = xt[k] + (l.X_T_rot[3 * k] * tj[0] + l.X_T_rot[3 * k + 1] * tj[1] + l.X_T_rot[3 * k + 2] * tj[2]);
  tds_d_mul(l.X_T_rot, R, Xp.r);
}

// ref: dynamics/kinematics.hpp:18-148 (fixed and floating base); have_qd = 0: the mass matrix's call (v = 0)
template <typename T, class B, class P>
TDS_HD inline void tds_d_kinematics(const tds_model_t *m, P p, TdsDiffWork<T, B> &w, int have_qd) {
  if (m->is_floating) {  // :35-62
    tds_d_quat_to_matrix(w.q, w.base.r);
    for (int k = 0; k < 3; ++k) {
      w.base.t[k] = w.q[4 + k];
      w.base_v.a[k] = have_qd ? w.qd[k] : T(0.0);
      w.base_v.l[k] = have_qd ? w.qd[3 + k] : T(0.0);
    }
    p.base_rbi(m, w.base_abi);  // :50
    // :52-59 gyroscopic force with the world inertia R I R^T and the base angular velocity (frames as the reference has them)
    T RI[9], Iw[9], Iwv[3];
    tds_d_mul(w.base.r, p.base_inertia(m), RI);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) Iw[3 * i + j] = RI[3 * i] * w.base.r[3 * j] + RI[3 * i + 1] * w.base.r[3 * j + 1] + RI[3 * i + 2] * w.base.r[3 * j + 2];
    tds_d_mulv(Iw, w.base_v.a, Iwv);
    tds_d_cross(w.base_v.a, Iwv, w.base_bias.a);
    for (int k = 0; k < 3; ++k) w.base_bias.l[k] = T(0.0);
  } else {
    for (int k = 0; k < 9; ++k) w.base.r[k] = T(m->base_X_world_rot[k]);
    for (int k = 0; k < 3; ++k) w.base.t[k] = T(m->base_X_world_trans[k]);
  }
  for (int i = 0; i < m->num_links; ++i) {
    const tds_link_t &l = m->links[i];
    const T q = l.q_index >= 0 ? w.q[l.q_index] : T(0.0);  // multi_body.hpp:490-500
    const T qd = (have_qd && l.qd_index >= 0) ? w.qd[l.qd_index] : T(0.0);
    tds_d_jcalc(l, p.xt(m, i), q, w.Xp[i]);
    TdsDSv<T> vJ;  // link.hpp:289-329: S qd
    for (int k = 0; k < 3; ++k) vJ.a[k] = l.S[k] * qd, vJ.l[k] = l.S[3 + k] * qd;
    const TdsDXf<T> &Xpar = l.parent >= 0 ? w.Xw[l.parent] : w.base;
    tds_d_xf_mul(Xpar, w.Xp[i].r, w.Xp[i].t, w.Xw[i]);  // :82 / :92
    if (l.parent >= 0 || m->is_floating) {             // :84-87
      TdsDSv<T> xv;
      tds_d_apply_motion(w.Xp[i], l.parent >= 0 ? w.v[l.parent] : w.base_v, xv);
      for (int k = 0; k < 3; ++k) w.v[i].a[k] = xv.a[k] + vJ.a[k], w.v[i].l[k] = xv.l[k] + vJ.l[k];
    } else {
      w.v[i] = vJ;
    }
    tds_d_cross_mm(w.v[i], vJ, w.c[i]);  // :96-97
    p.link_rbi(m, i, w.abi[i]);  // :99
    TdsDSv<T> Iv;
    tds_d_abi_mul(w.abi[i], w.v[i], Iv);
    tds_d_cross_mf(w.v[i], Iv, w.pA[i]);  // :132
  }
}

// ref: dynamics/forward_dynamics.hpp:11-326 (ABA)
template <typename T, class B, class P>
TDS_HD inline void tds_d_forward_dynamics(const tds_model_t *m, P p, TdsDiffWork<T, B> &w) {
  tds_d_kinematics(m, p, w, 1);
  for (int i = m->num_links - 1; i >= 0; --i) {
    const tds_link_t &l = m->links[i];
    tds_d_abi_mulc(w.abi[i], l.S, w.U[i]);  // :111
    w.D[i] = tds_d_dot6c(l.S, w.U[i]);      // :115
    T tau = l.joint_type != TDS_JOINT_FIXED ? w.tau[l.qd_index] : T(0.0);  // multi_body.hpp:557-570
    const T qv = l.q_index >= 0 ? w.q[l.q_index] : T(0.0), qdv = l.qd_index >= 0 ? w.qd[l.qd_index] : T(0.0);
    tau = tau - p.stiffness(m, i) * qv;  // :122
    tau = tau - p.damping(m, i) * qdv;   // :123
    w.u[i] = tau - tds_d_dot6c(l.S, w.pA[i]);  // :129
    const T invD = l.joint_type == TDS_JOINT_FIXED ? T(0.0) : 1.0 / w.D[i];  // :153
    if (l.parent < 0 && !m->is_floating) continue;
    TdsDAbi<T> Ia;  // :168  IA - U (U invD)^T  (inertia.hpp:333-348)
    TdsDSv<T> Ub, Iac, pa;
    for (int k = 0; k < 3; ++k) Ub.a[k] = w.U[i].a[k] * invD, Ub.l[k] = w.U[i].l[k] * invD;
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        Ia.I[3 * r + c] = w.abi[i].I[3 * r + c] - w.U[i].a[r] * Ub.a[c];
        Ia.H[3 * r + c] = w.abi[i].H[3 * r + c] - w.U[i].a[r] * Ub.l[c];
        Ia.M[3 * r + c] = w.abi[i].M[3 * r + c] - w.U[i].l[r] * Ub.l[c];
      }
    tds_d_abi_mul(Ia, w.c[i], Iac);  // :171
    const T uinvD = w.u[i] * invD;   // :162
    for (int k = 0; k < 3; ++k) {    // :173
      pa.a[k] = w.pA[i].a[k] + Iac.a[k] + w.U[i].a[k] * uinvD;
      pa.l[k] = w.pA[i].l[k] + Iac.l[k] + w.U[i].l[k] * uinvD;
    }
    TdsDSv<T> dpA;
    tds_d_apply_force(w.Xp[i], pa, dpA);  // :181
    TdsDSv<T> &PpA = l.parent >= 0 ? w.pA[l.parent] : w.base_bias;  // :201 / :206
    for (int k = 0; k < 3; ++k) PpA.a[k] = PpA.a[k] + dpA.a[k], PpA.l[k] = PpA.l[k] + dpA.l[k];
    tds_d_abi_congruence_add(w.Xp[i], Ia, l.parent >= 0 ? w.abi[l.parent] : w.base_abi);  // :187-189, :202 / :207
  }
  TdsDSv<T> a_base;
  if (m->is_floating) {  // :232  -base_abi^-1 base_bias
    TdsDSv<T> r;
    tds_d_abi_inv_mul(w.base_abi, w.base_bias, r);
    for (int k = 0; k < 3; ++k) a_base.a[k] = -r.a[k], a_base.l[k] = -r.l[k];
  } else {  // :242  -spatial gravity
    for (int k = 0; k < 3; ++k) a_base.a[k] = T(0.0), a_base.l[k] = p.template neg_gravity<T>(m, k);
  }
  for (int i = 0; i < m->num_links; ++i) {  // :245-302 (a_i into v_i: the velocities are not read any more)
    const tds_link_t &l = m->links[i];
    TdsDSv<T> xa;
    tds_d_apply_motion(w.Xp[i], l.parent >= 0 ? w.v[l.parent] : a_base, xa);
    for (int k = 0; k < 3; ++k) w.v[i].a[k] = xa.a[k] + w.c[i].a[k], w.v[i].l[k] = xa.l[k] + w.c[i].l[k];
    if (l.qd_index >= 0) {
      const T invD = l.joint_type == TDS_JOINT_FIXED ? T(0.0) : 1.0 / w.D[i];
      const T qdd = invD * (w.u[i] - tds_d_dot6(w.U[i], w.v[i]));
      w.qdd[l.qd_index] = qdd;
      for (int k = 0; k < 3; ++k) w.v[i].a[k] = w.v[i].a[k] + l.S[k] * qdd, w.v[i].l[k] = w.v[i].l[k] + l.S[3 + k] * qdd;
    }
  }
  if (m->is_floating)  // :315-319  gravity (world components) added to the base-frame acceleration
    for (int k = 0; k < 3; ++k) w.qdd[k] = a_base.a[k], w.qdd[3 + k] = a_base.l[k] + p.gravity(m)[k];
}

// ref: dynamics/mass_matrix.hpp:13-127 (CRBA) followed by the Cholesky factor of tiny_matrix_x.h:240-345 into w.L.
// Returns 0, or -1 where M is not positive definite (the reference's inverse fails: mb_constraint_solver.hpp:245-246)
template <typename T, class B, class P>
TDS_HD inline int tds_d_mass_matrix(const tds_model_t *m, P p, TdsDiffWork<T, B> &w) {
  const int nd = m->dof_qd;
  T *M = w.L;  // assembled in place, then factored
  tds_d_kinematics(m, p, w, 0);  // :37
  for (int k = 0; k < nd * nd; ++k) M[k] = T(0.0);
  for (int i = m->num_links - 1; i >= 0; --i) {
    const tds_link_t &l = m->links[i];
    if (l.parent >= 0 || m->is_floating)  // :45-53
      tds_d_abi_congruence_add(w.Xp[i], w.abi[i], l.parent >= 0 ? w.abi[l.parent] : w.base_abi);
    if (l.joint_type == TDS_JOINT_FIXED) continue;  // :56
    const int qi = l.qd_index;
    TdsDSv<T> F;
    tds_d_abi_mulc(w.abi[i], l.S, F);  // :87
    M[qi * nd + qi] = tds_d_dot6c(l.S, F);  // :89
    int j = i;
    while (m->links[j].parent != -1) {  // :92-109
      tds_d_apply_force(w.Xp[j], F, F);
      j = m->links[j].parent;
      if (m->links[j].joint_type == TDS_JOINT_FIXED) continue;
      const int qj = m->links[j].qd_index;
      M[qi * nd + qj] = M[qj * nd + qi] = tds_d_dot6c(m->links[j].S, F);
    }
    if (m->is_floating) {  // :111-115
      tds_d_apply_force(w.Xp[j], F, F);
      for (int k = 0; k < 3; ++k) {
        M[k * nd + qi] = M[qi * nd + k] = F.a[k];
        M[(3 + k) * nd + qi] = M[qi * nd + 3 + k] = F.l[k];
      }
    }
  }
  if (m->is_floating)  // :118-125
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        M[r * nd + c] = w.base_abi.I[3 * r + c];
        M[r * nd + 3 + c] = w.base_abi.H[3 * r + c];
        M[(3 + r) * nd + c] = w.base_abi.H[3 * c + r];
        M[(3 + r) * nd + 3 + c] = w.base_abi.M[3 * r + c];
      }
  // L L^T = M, lower triangle in place (tiny_matrix_x.h:240-270)
  for (int i = 0; i < nd; ++i)
    for (int j = i; j < nd; ++j) {
      T s = M[i * nd + j];
      for (int k = i - 1; k >= 0; --k) s = s - M[i * nd + k] * M[j * nd + k];
      if (i == j) {
        if (s <= 0.0) return -1;
        M[i * nd + i] = tds_sqrt(s);
      } else {
        M[j * nd + i] = s / M[i * nd + i];
      }
    }
  return 0;
}

// ref: dynamics/jacobian.hpp:13-83: the world-frame point Jacobian of link `li` at `pt` into w.jac
template <typename T, class B>
TDS_HD inline void tds_d_point_jacobian(const tds_model_t *m, TdsDiffWork<T, B> &w, int li, const T *pt) {
  const int nd = m->dof_qd;
  for (int r = 0; r < 3; ++r)
    for (int d = 0; d < nd; ++d) w.jac[r][d] = T(0.0);
  if (m->is_floating) {  // :39-56  [ [r]x^T | 1 ],  r = point - base position
    T r[3] = {pt[0] - w.base.t[0], pt[1] - w.base.t[1], pt[2] - w.base.t[2]};
    w.jac[0][1] = r[2], w.jac[0][2] = -r[1];
    w.jac[1][0] = -r[2], w.jac[1][2] = r[0];
    w.jac[2][0] = r[1], w.jac[2][1] = -r[0];
    w.jac[0][3] = w.jac[1][4] = w.jac[2][5] = T(1.0);
  }
  for (int i = li; i >= 0; i = m->links[i].parent) {
    const tds_link_t &l = m->links[i];
    if (l.joint_type == TDS_JOINT_FIXED) continue;
    TdsDSv<T> st;
    tds_d_apply_inverse_motion(w.Xw[i], l.S, st);  // :74
    T rxw[3];
    tds_d_cross(pt, st.a, rxw);  // :76
    for (int r = 0; r < 3; ++r) w.jac[r][l.qd_index] = st.l[r] - rxw[r];
  }
}

// ref: world.hpp:206-282 (plane = multi body a, the robot b) and contact_point.hpp:96-198 (plane-sphere / capsule / box)
// The shapes are read through the view.  A box's rad = radius > 1e-2 ? radius : 1e-2 is a branch of the primal: at or
// below 1e-2 the constant is taken and the derivative along the radius is exactly zero.
template <typename T, class B, class P>
TDS_HD inline void tds_d_contacts(const tds_model_t *m, P p, TdsDiffWork<T, B> &w) {
  typedef typename P::template geom_scalar<T> S;
  w.n_c = 0;
  const double *n = m->plane_normal;
  for (int g = 0; g < m->num_geoms; ++g) {
    const tds_geom_t &G = m->geoms[g];
    TdsDXf<T> tr;
    tds_d_xf_mul(G.link >= 0 ? w.Xw[G.link] : w.base, G.X_rot, p.geom_trans(m, g), tr);  // world.hpp:242
    T orn[4];
    tds_d_matrix_to_quat(tr.r, orn);  // world.hpp:244-245
    tds_d_quat_normalize(orn);
    int np = 0;
    S off[8][3], rad = tds_geom_has_points(G) ? p.geom_radius(m, g) : S(0.0);
    if (G.type == TDS_GEOM_SPHERE) {
      np = 1, off[0][0] = off[0][1] = off[0][2] = S(0.0);
    } else if (G.type == TDS_GEOM_CAPSULE) {  // :127-161
      np = 2;
      for (int e = 0; e < 2; ++e)
        off[e][0] = off[e][1] = S(0.0), off[e][2] = (e == 0 ? 0.5 : -0.5) * p.geom_length(m, g);
    } else if (G.type == TDS_GEOM_BOX) {  // :163-198, geometry.hpp:244-259
      np = 8;
      if (!(rad > 1e-2)) rad = S(1e-2);  // rad = radius > 1e-2 ? radius : 1e-2
      const S dx = p.geom_extents(m, g)[0] * 0.5 - rad, dy = p.geom_extents(m, g)[1] * 0.5 - rad,
              dz = p.geom_extents(m, g)[2] * 0.5 - rad;
      for (int c = 0; c < 8; ++c) off[c][0] = (c & 4) ? -dx : dx, off[c][1] = (c & 2) ? -dy : dy, off[c][2] = (c & 1) ? -dz : dz;
    }
    for (int e = 0; e < np; ++e) {
      T pos[3];
      if (G.type == TDS_GEOM_SPHERE) {
        for (int k = 0; k < 3; ++k) pos[k] = tr.t[k];
      } else {
        T ro[3];
        tds_d_quat_rotate(orn, off[e], ro);  // pose.hpp:47-53
        for (int k = 0; k < 3; ++k) pos[k] = tr.t[k] + ro[k];
      }
      // :96-125  t = -(pos . (-n) + constant); point_b = pos - r n; distance = t - r
      const int c = w.n_c++;
      T t = -((pos[0] * -n[0] + pos[1] * -n[1] + pos[2] * -n[2]) + m->plane_constant);
      for (int k = 0; k < 3; ++k) w.cp_b[c][k] = tds_sub_c(pos[k], rad * n[k]);
      w.cp_dist[c] = tds_sub_c(t, rad);
      w.cp_link[c] = G.link;
    }
  }
}

// ref: mb_constraint_solver.hpp:506-520 (incl. its quirks): the friction directions of the (constant) contact normal
static inline TDS_HD void tds_d_plane_space(const double *n, double *p, double *q) {
  const double n_sqr = n[2] * n[2];
  const int gt = n_sqr > 0.5;
  const double a = n[1] * n[1] + (gt ? n_sqr : n[0] * n[0]), k = sqrt(a);
  p[0] = gt ? 0.0 : -n[1] * k;
  p[1] = gt ? -n[2] * k : n[0] * k;
  p[2] = n[1] * k;
  q[0] = gt ? a * k : -n[2] * p[1];
  q[1] = gt ? -n[0] * p[2] : n[2] * p[0];
  q[2] = gt ? n[0] * p[1] : a * k;
}

// ref: mb_constraint_solver.hpp:191-498 (mb_a = plane, mb_b = robot, keep_all_points_), PGS :101-142
template <typename T, class B, class P>
TDS_HD inline int tds_d_resolve(const tds_model_t *m, P p, TdsDiffWork<T, B> &w) {
  const int nc = w.n_c, nd = m->dof_qd, nr = 3 * nc;
  if (nc == 0 || nd == 0) return 0;
  if (tds_d_mass_matrix(m, p, w)) return -1;  // :232-246
  double nrm[3] = {-m->plane_normal[0], -m->plane_normal[1], -m->plane_normal[2]}, f1[3], f2[3];
  tds_d_plane_space(nrm, f1, f2);  // :361
  for (int i = 0; i < nc; ++i) {
    const bool hit = w.cp_dist[i] < 0.0;  // :285 collision = distance < 0
    tds_d_point_jacobian(m, w, w.cp_link[i], w.cp_b[i]);  // :295
    T vel[3];  // :314  jac_b qd
    for (int r = 0; r < 3; ++r) {
      T s = T(0.0);
      for (int d = 0; d < nd; ++d) s = s + w.jac[r][d] * w.qd[d];
      vel[r] = s;
    }
    // rel_vel = -vel (:315); b rows (:321-325, :365-370), J rows (:300-307, :378-384); inactive contacts: zero rows
    const T nrv = -(nrm[0] * vel[0] + nrm[1] * vel[1] + nrm[2] * vel[2]);
    w.b[i] = hit ? (-(1.0 + p.restitution(m)) * nrv - p.erp(m) * w.cp_dist[i] / m->dt) : T(0.0);
    w.b[nc + i] = hit ? (f1[0] * vel[0] + f1[1] * vel[1] + f1[2] * vel[2]) : T(0.0);
    w.b[2 * nc + i] = hit ? (f2[0] * vel[0] + f2[1] * vel[1] + f2[2] * vel[2]) : T(0.0);
    for (int d = 0; d < nd; ++d) {
      w.J[i][d] = hit ? w.jac[0][d] * nrm[0] + w.jac[1][d] * nrm[1] + w.jac[2][d] * nrm[2] : T(0.0);
      w.J[nc + i][d] = hit ? w.jac[0][d] * f1[0] + w.jac[1][d] * f1[1] + w.jac[2][d] * f1[2] : T(0.0);
      w.J[2 * nc + i][d] = hit ? w.jac[0][d] * f2[0] + w.jac[1][d] * f2[1] + w.jac[2][d] * f2[2] : T(0.0);
    }
  }
  // W_r = M^-1 J_r^T: L y = J_r^T, L^T W_r = y
  for (int r = 0; r < nr; ++r) {
    T *x = w.W[r];
    for (int i = 0; i < nd; ++i) {
      T s = w.J[r][i];
      for (int k = 0; k < i; ++k) s = s - w.L[i * nd + k] * x[k];
      x[i] = s / w.L[i * nd + i];
    }
    for (int i = nd - 1; i >= 0; --i) {
      T s = x[i];
      for (int k = i + 1; k < nd; ++k) s = s - w.L[k * nd + i] * x[k];
      x[i] = s / w.L[i * nd + i];
    }
  }
  // PGS (:101-142, :424-440) on A = J M^-1 J^T + cfm 1 through u = W^T p: (A p)_r = J_r . u + cfm p_r
  T u[B::ND];
  for (int d = 0; d < nd; ++d) u[d] = T(0.0);
  for (int r = 0; r < nr; ++r) w.p[r] = T(0.0);
  for (int it = 0; it < m->pgs_iterations; ++it)
    for (int r = 0; r < nr; ++r) {
      T Ju = T(0.0), Arr = T(0.0);
      for (int d = 0; d < nd; ++d) Ju = Ju + w.J[r][d] * u[d], Arr = Arr + w.J[r][d] * w.W[r][d];
      const T delta = Ju - Arr * w.p[r];
      T x = (w.b[r] - delta) / tds_add_c(Arr, p.cfm(m));
      if (r < nc) {  // normal: [0, 1e5]
        x = tds_clamp(x, T(0.0), T(100000.0));
      } else {  // friction: +-mu max(p_normal, 0)
        const T pn = w.p[r % nc], sc = pn < 0.0 ? T(0.0) : pn;
        const T lo = -p.friction(m) * sc, hi = p.friction(m) * sc;
        if (x < lo) x = lo;  // Algebra::max
        if (x > hi) x = hi;  // Algebra::min
      }
      const T dx = x - w.p[r];
      w.p[r] = x;
      for (int d = 0; d < nd; ++d) u[d] = u[d] + w.W[r][d] * dx;
    }
  // :476-496  qd -= M^-1 J^T p
  for (int d = 0; d < nd; ++d) {
    T s = T(0.0);
    for (int r = 0; r < nr; ++r) s = s + w.W[r][d] * w.p[r];
    w.qd[d] = w.qd[d] - s;
  }
  return 0;
}

// forward_zero of one environment: y[0 .. tds_diff_ny(m)) = step(x[input_dim]); the reference record's remaining
// output_dim - tds_diff_ny(m) entries are zero and left to the caller.  ref: examples/environments/
// locomotion_contact_simulation.h:151-304 (LOCOMOTION) and cartpole_environment.h:71-117 (TAU), world.hpp:293-366.
// Returns 0, or -1 where the mass matrix is not positive definite.
// The model's selectable parameters are read through the view p (TdsBlobView: the blob's values).
template <typename T, class B, class P>
TDS_HD inline int tds_diff_step_view(const tds_model_t *m, P p, TdsDiffWork<T, B> &w, const T *x, T *y) {
  const int nq = m->dof_q, nd = m->dof_qd;
  for (int i = 0; i < nq; ++i) w.q[i] = x[i];  // :154-159
  for (int i = 0; i < nd; ++i) w.qd[i] = x[nq + i], w.qdd[i] = T(0.0), w.tau[i] = T(0.0);
  if (m->step_mode == TDS_STEP_LOCOMOTION) {
    const int act = nq + nd, var = nq + nd + m->action_dim;
    const T kp = x[var], kd = x[var + 1], max_force = x[var + 2];  // :164-166
    int pose = 0;
    for (int i = m->pd_start_link; i < m->num_links; ++i) {  // :181-257
      const tds_link_t &l = m->links[i];
      if (l.joint_type == TDS_JOINT_FIXED) continue;
      T a = x[act + pose];
      if (a > m->action_limit) a = T(m->action_limit);  // :235-236
      if (a < -m->action_limit) a = T(-m->action_limit);
      const T q_des = m->initial_poses[pose++] + a;  // :238
      T f = kp * (q_des - w.q[l.q_index]) + kd * (0.0 - w.qd[l.qd_index]);  // :242-245
      if (f < -max_force) f = -max_force;  // :247
      if (f > max_force) f = max_force;
      w.tau[l.qd_index] = f;
    }
  } else {  // TAU: the torques of the actuated dofs (get_tau_for_link, multi_body.hpp:557-570)
    const int off = m->is_floating ? 6 : 0;
    for (int i = 0; i < nd - off; ++i) w.tau[off + i] = x[nq + nd + i];
  }
  tds_d_forward_dynamics(m, p, w);  // :261
  if (m->is_floating)  // integrate_euler_qdd (integrator.hpp:141-182)
    for (int k = 0; k < 6; ++k) w.qd[k] = w.qd[k] + w.qdd[k] * m->dt;
  for (int i = 0; i < m->num_links; ++i)
    if (m->links[i].joint_type != TDS_JOINT_FIXED) {
      const int d = m->links[i].qd_index;
      w.qd[d] = w.qd[d] + w.qdd[d] * m->dt;
    }
  int j = 0;
  // the visuals' poses are taken before the step (:273-303 pack X_world of the dynamics' kinematics); they go into y
  // after q and qd, which are written below
  if (m->pack_visuals) {
    j = nq + nd;
    for (int v = 0; v < m->num_visuals; ++v) {
      const tds_visual_t &V = m->visuals[v];
      TdsDXf<T> vx;
      tds_d_xf_mul(w.Xw[V.link], V.X_rot, V.X_trans, vx);  // :285
      T orn[4];
      tds_d_matrix_to_quat(vx.r, orn);  // :291
      for (int k = 0; k < 3; ++k) y[j++] = vx.t[k];
      for (int k = 0; k < 4; ++k) y[j++] = orn[k];
    }
  }
  if (m->has_plane) {  // world.step (world.hpp:293-366)
    tds_d_contacts(m, p, w);
    if (tds_d_resolve(m, p, w)) return -1;
  }
  if (m->is_floating) {  // integrate_euler (integrator.hpp:23-89): quaternion += quat_velocity(q, omega, dt), normalised
    T *b = w.q;
    const T *om = w.qd;
    const double h = 0.5 * m->dt;
    T ww = (-b[0] * om[0] - b[1] * om[1] - b[2] * om[2]) * h;
    T xx = (b[3] * om[0] + b[2] * om[1] - b[1] * om[2]) * h;
    T yy = (b[3] * om[1] + b[0] * om[2] - b[2] * om[0]) * h;
    T zz = (b[3] * om[2] + b[1] * om[0] - b[0] * om[1]) * h;
    b[0] = b[0] + xx, b[1] = b[1] + yy, b[2] = b[2] + zz, b[3] = b[3] + ww;
    tds_d_quat_normalize(b);
    tds_d_quat_to_matrix(b, w.base.r);  // :83 (the translation of base_X_world is not refreshed)
    for (int k = 0; k < 3; ++k) b[4 + k] = b[4 + k] + w.qd[3 + k] * m->dt;
  }
  for (int i = 0; i < m->num_links; ++i)  // integrator.hpp:126-131
    if (m->links[i].joint_type != TDS_JOINT_FIXED) {
      const tds_link_t &l = m->links[i];
      w.q[l.q_index] = w.q[l.q_index] + w.qd[l.qd_index] * m->dt;
    }
  for (int i = 0; i < nq; ++i) y[i] = w.q[i];  // :273-303
  for (int i = 0; i < nd; ++i) y[nq + i] = w.qd[i];
  if (m->pack_visuals) y[j] = w.base.r[8];  // up . z (:301-303)
  return 0;
}

// the step with the blob's parameters (the plain instantiations: double, TdsDual<K>, TdsRev)
template <typename T, class B>
TDS_HD inline int tds_diff_step(const tds_model_t *m, TdsDiffWork<T, B> &w, const T *x, T *y) {
  return tds_diff_step_view(m, TdsBlobView{}, w, x, y);
}
