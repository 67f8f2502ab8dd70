// tds_dyn.h — one single-source, scalar-templated statement of the batched dynamics queries (tds_dyn.hip): link
// transforms X_world, the joint-space inertia M(q) (CRBA), inverse dynamics tau = ID(q, qd, qdd) (RNEA) and its
// special case bias = ID(q, qd, 0), unconstrained forward dynamics qdd = M^-1 (tau - K q - D qd - bias), and the
// world-frame Jacobian of a point on a link.  Instantiated over double on the host (the checkers) and on the device;
// the scalar is a template parameter so that a dual-number instantiation can follow.
//
// The model is read from the C-ABI blob tds_model_t through a parameter view (TdsBlobView), and the helpers are those
// of tds_diff_step.h (tds_d_jcalc, the transform, spatial-vector and ABI helpers, the X^T I X congruence), read only.
// "ref:" = file:line under the reference's src/.
//
// WHERE THE STATE LIVES.  Unlike TdsDiffWork (a struct per lane), the per-link state is a flat array of components
// reached through TdsDynMem: component i of this environment is p[i * s].  The host passes s = 1 (a vector per
// environment); the device passes p = buffer + lane, s = lanes, so that the buffer is laid out [component][lane] with
// the lane minor and a wave-uniform access to link i's component is one coalesced run.  A link's transform, velocity
// or inertia is loaded into a small local object (constant indices: registers), worked on with the struct helpers, and
// stored back; nothing that is indexed at run time lives in a local array.
//
// SCOPE.  That of the step derivatives (tds_diff_check): one articulated body, 1-DoF and fixed joints.  The public
// bias / inverse dynamics are fixed-base only (the reference's inverse_dynamics asserts on a floating base,
// dynamics/inverse_dynamics.hpp:74); forward dynamics on a floating base uses the internal floating-base recursion of
// tds_dyn_rnea below, arranged as the reference's ABA treats its base (forward_dynamics.hpp:232, :315-319).
#pragma once
#include "tds_diff_step.h"

template <typename T>
struct TdsDynMem {
  T *p;
  size_t s;
  TDS_HD T &operator[](int i) const { return p[(size_t)i * s]; }
};

// component offsets of one environment's state: transforms, velocities, accelerations, forces, inertias, M, its factor
// (17 KB at 22 links: the 16384 states of a full launch, tds_query.h, are 280 MB of the handle's work buffer)
struct TdsDynLayout {
  int q, qd, qdd, tau, pt, xp, xw, v, c, a, f, abi, base, base_v, base_f, base_abi, M, L, bias, rhs, jac, total;
};
static inline TDS_HD TdsDynLayout tds_dyn_layout(const tds_model_t *m) {
  const int nl = m->num_links, nd = m->dof_qd;
  TdsDynLayout L;
  int o = 0;
  L.q = o, o += nd + 1;
  L.qd = o, o += nd;
  L.qdd = o, o += nd;
  L.tau = o, o += nd;
  L.pt = o, o += 3;
  L.xp = o, o += 12 * nl;
  L.xw = o, o += 12 * nl;
  L.v = o, o += 6 * nl;
  L.c = o, o += 6 * nl;
  L.a = o, o += 6 * nl;
  L.f = o, o += 6 * nl;
  L.abi = o, o += 27 * nl;
  L.base = o, o += 12;
  L.base_v = o, o += 6;
  L.base_f = o, o += 6;
  L.base_abi = o, o += 27;
  L.M = o, o += nd * nd;
  L.L = o, o += nd * nd;
  L.bias = o, o += nd;
  L.rhs = o, o += nd;
  L.jac = o, o += 3 * nd;
  L.total = o;
  return L;
}

// ---------------------------------------------------------------- loads and stores of the small objects
template <typename T>
TDS_HD inline void tds_dyn_ld(TdsDynMem<T> w, int o, TdsDXf<T> &x) {
  for (int k = 0; k < 9; ++k) x.r[k] = w[o + k];
  for (int k = 0; k < 3; ++k) x.t[k] = w[o + 9 + k];
}
template <typename T>
TDS_HD inline void tds_dyn_st(TdsDynMem<T> w, int o, const TdsDXf<T> &x) {
  for (int k = 0; k < 9; ++k) w[o + k] = x.r[k];
  for (int k = 0; k < 3; ++k) w[o + 9 + k] = x.t[k];
}
template <typename T>
TDS_HD inline void tds_dyn_ld(TdsDynMem<T> w, int o, TdsDSv<T> &x) {
  for (int k = 0; k < 3; ++k) x.a[k] = w[o + k], x.l[k] = w[o + 3 + k];
}
template <typename T>
TDS_HD inline void tds_dyn_st(TdsDynMem<T> w, int o, const TdsDSv<T> &x) {
  for (int k = 0; k < 3; ++k) w[o + k] = x.a[k], w[o + 3 + k] = x.l[k];
}
template <typename T>
TDS_HD inline void tds_dyn_ld(TdsDynMem<T> w, int o, TdsDAbi<T> &x) {
  for (int k = 0; k < 9; ++k) x.I[k] = w[o + k], x.H[k] = w[o + 9 + k], x.M[k] = w[o + 18 + k];
}
template <typename T>
TDS_HD inline void tds_dyn_st(TdsDynMem<T> w, int o, const TdsDAbi<T> &x) {
  for (int k = 0; k < 9; ++k) w[o + k] = x.I[k], w[o + 9 + k] = x.H[k], w[o + 18 + k] = x.M[k];
}

// ---------------------------------------------------------------- kinematics
// ref: dynamics/kinematics.hpp:18-148.  Reads q (and qd where have_v) at L.q / L.qd; writes X_parent, X_world and, with
// have_v, the link velocities v, the velocity products c = v x vJ and the links' rigid-body inertias (also the base's
// transform, velocity, inertia and gyroscopic force on a floating base).  have_v = 0: transforms only.
template <typename T, class P>
TDS_HD inline void tds_dyn_kinematics(const tds_model_t *m, P p, TdsDynMem<T> w, const TdsDynLayout &L, int have_v) {
  TdsDXf<T> base;
  TdsDSv<T> base_v;
  for (int k = 0; k < 3; ++k) base_v.a[k] = T(0.0), base_v.l[k] = T(0.0);
  if (m->is_floating) {  // :35-62
    T qb[4] = {w[L.q], w[L.q + 1], w[L.q + 2], w[L.q + 3]};
    for (int k = 0; k < 9; ++k) base.r[k] = T(k % 4 == 0 ? 1.0 : 0.0);
    tds_d_quat_to_matrix(qb, base.r);
    for (int k = 0; k < 3; ++k) base.t[k] = w[L.q + 4 + k];
    if (have_v) {
      for (int k = 0; k < 3; ++k) base_v.a[k] = w[L.qd + k], base_v.l[k] = w[L.qd + 3 + k];
      TdsDAbi<T> babi;
      p.base_rbi(m, babi);  // :50
      tds_dyn_st(w, L.base_abi, babi);
      // :52-59 gyroscopic force with the world inertia R I R^T and the base angular velocity (the reference's frames)
      T RI[9], Iw[9], Iwv[3];
      TdsDSv<T> bf;
      tds_d_mul(base.r, p.base_inertia(m), RI);
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
          Iw[3 * i + j] = RI[3 * i] * base.r[3 * j] + RI[3 * i + 1] * base.r[3 * j + 1] + RI[3 * i + 2] * base.r[3 * j + 2];
      tds_d_mulv(Iw, base_v.a, Iwv);
      tds_d_cross(base_v.a, Iwv, bf.a);
      for (int k = 0; k < 3; ++k) bf.l[k] = T(0.0);
      tds_dyn_st(w, L.base_f, bf);
      tds_dyn_st(w, L.base_v, base_v);
    }
  } else {
    for (int k = 0; k < 9; ++k) base.r[k] = T(m->base_X_world_rot[k]);
    for (int k = 0; k < 3; ++k) base.t[k] = T(m->base_X_world_trans[k]);
  }
  tds_dyn_st(w, L.base, base);
  for (int i = 0; i < m->num_links; ++i) {
    const tds_link_t &l = m->links[i];
    const T q = l.q_index >= 0 ? w[L.q + l.q_index] : T(0.0);  // multi_body.hpp:490-500
    TdsDXf<T> Xp, Xpar, Xw;
    tds_d_jcalc(l, p.xt(m, i), q, Xp);
    tds_dyn_st(w, L.xp + 12 * i, Xp);
    if (l.parent >= 0)
      tds_dyn_ld(w, L.xw + 12 * l.parent, Xpar);
    else
      Xpar = base;
    tds_d_xf_mul(Xpar, Xp.r, Xp.t, Xw);  // :82 / :92
    tds_dyn_st(w, L.xw + 12 * i, Xw);
    if (!have_v) continue;
    const T qd = l.qd_index >= 0 ? w[L.qd + l.qd_index] : T(0.0);
    TdsDSv<T> vJ, v, c;  // link.hpp:289-329: S qd
    for (int k = 0; k < 3; ++k) vJ.a[k] = l.S[k] * qd, vJ.l[k] = l.S[3 + k] * qd;
    if (l.parent >= 0 || m->is_floating) {  // :84-87
      TdsDSv<T> vp, xv;
      if (l.parent >= 0)
        tds_dyn_ld(w, L.v + 6 * l.parent, vp);
      else
        vp = base_v;
      tds_d_apply_motion(Xp, vp, xv);
      for (int k = 0; k < 3; ++k) v.a[k] = xv.a[k] + vJ.a[k], v.l[k] = xv.l[k] + vJ.l[k];
    } else {
      v = vJ;
    }
    tds_d_cross_mm(v, vJ, c);  // :96-97
    tds_dyn_st(w, L.v + 6 * i, v);
    tds_dyn_st(w, L.c + 6 * i, c);
    TdsDAbi<T> abi;
    p.link_rbi(m, i, abi);  // :99
    tds_dyn_st(w, L.abi + 27 * i, abi);
  }
}

// ---------------------------------------------------------------- inverse dynamics (RNEA)
// out[dof_qd] (components at `out`) = ID(q, qd, qdd) after tds_dyn_kinematics(have_v = 1) and BEFORE tds_dyn_crba (which
// turns the links' inertias into composite ones).  qdd < 0: zero accelerations.  ref: kinematics.hpp:132-146 (a_i =
// X a_parent + v x vJ, f_i = I a_i + v x* I v) with the joint's own S qdd added (Featherstone, RBDA table 5.1), and
// inverse_dynamics.hpp:54-70 (tau_i = S . f_i, f_parent += X^T f_i).  Springs and dampers are not part of it.
//   fixed base:    the base accelerates with -gravity (inverse_dynamics.hpp:54, forward_dynamics.hpp:242).
//   floating base (internal, the right-hand side of the forward dynamics only): the recursion starts from a resting
//     base and no gravity, and the base's six entries are its gyroscopic force plus the links' forces brought to the
//     base: M qdd = tau - out is then the system the reference's ABA solves (forward_dynamics.hpp:232), which adds
//     gravity to the base's linear acceleration afterwards (:315-319).
template <typename T, class P>
TDS_HD inline void tds_dyn_rnea(const tds_model_t *m, P p, TdsDynMem<T> w, const TdsDynLayout &L, int qdd, int out) {
  TdsDSv<T> a_base;
  for (int k = 0; k < 3; ++k) a_base.a[k] = T(0.0), a_base.l[k] = m->is_floating ? T(0.0) : p.template neg_gravity<T>(m, k);
  for (int i = 0; i < m->num_links; ++i) {
    const tds_link_t &l = m->links[i];
    TdsDXf<T> Xp;
    TdsDSv<T> ap, xa, c, a, v, Iv, Ia, pA;
    TdsDAbi<T> abi;
    tds_dyn_ld(w, L.xp + 12 * i, Xp);
    if (l.parent >= 0)
      tds_dyn_ld(w, L.a + 6 * l.parent, ap);
    else
      ap = a_base;
    tds_d_apply_motion(Xp, ap, xa);
    tds_dyn_ld(w, L.c + 6 * i, c);
    for (int k = 0; k < 3; ++k) a.a[k] = xa.a[k] + c.a[k], a.l[k] = xa.l[k] + c.l[k];
    if (qdd >= 0 && l.qd_index >= 0) {
      const T s = w[qdd + l.qd_index];
      for (int k = 0; k < 3; ++k) a.a[k] = a.a[k] + l.S[k] * s, a.l[k] = a.l[k] + l.S[3 + k] * s;
    }
    tds_dyn_st(w, L.a + 6 * i, a);
    tds_dyn_ld(w, L.abi + 27 * i, abi);
    tds_dyn_ld(w, L.v + 6 * i, v);
    tds_d_abi_mul(abi, v, Iv);
    tds_d_cross_mf(v, Iv, pA);  // kinematics.hpp:132
    tds_d_abi_mul(abi, a, Ia);
    for (int k = 0; k < 3; ++k) Ia.a[k] = Ia.a[k] + pA.a[k], Ia.l[k] = Ia.l[k] + pA.l[k];  // :146
    tds_dyn_st(w, L.f + 6 * i, Ia);
  }
  for (int i = m->num_links - 1; i >= 0; --i) {
    const tds_link_t &l = m->links[i];
    TdsDSv<T> f;
    tds_dyn_ld(w, L.f + 6 * i, f);
    if (l.joint_type != TDS_JOINT_FIXED) w[out + l.qd_index] = tds_d_dot6c(l.S, f);  // inverse_dynamics.hpp:63
    if (l.parent < 0 && !m->is_floating) continue;
    TdsDXf<T> Xp;
    TdsDSv<T> df, fp;
    tds_dyn_ld(w, L.xp + 12 * i, Xp);
    tds_d_apply_force(Xp, f, df);  // :68
    const int po = l.parent >= 0 ? L.f + 6 * l.parent : L.base_f;
    tds_dyn_ld(w, po, fp);
    for (int k = 0; k < 3; ++k) fp.a[k] = fp.a[k] + df.a[k], fp.l[k] = fp.l[k] + df.l[k];
    tds_dyn_st(w, po, fp);
  }
  if (m->is_floating)
    for (int k = 0; k < 6; ++k) w[out + k] = w[L.base_f + k];
}

// ---------------------------------------------------------------- joint-space inertia (CRBA)
// ref: dynamics/mass_matrix.hpp:13-127 after tds_dyn_kinematics(have_v = 1): M [dof_qd][dof_qd] at L.M, both triangles
// written with the same value (symmetric by construction).  The links' inertias at L.abi become composite.
template <typename T, class P>
TDS_HD inline void tds_dyn_crba(const tds_model_t *m, P p, TdsDynMem<T> w, const TdsDynLayout &L) {
  const int nd = m->dof_qd, M = L.M;
  for (int k = 0; k < nd * nd; ++k) w[M + k] = T(0.0);
  for (int i = m->num_links - 1; i >= 0; --i) {
    const tds_link_t &l = m->links[i];
    TdsDAbi<T> abi;
    TdsDXf<T> Xp;
    tds_dyn_ld(w, L.abi + 27 * i, abi);
    if (l.parent >= 0 || m->is_floating) {  // :45-53
      const int po = l.parent >= 0 ? L.abi + 27 * l.parent : L.base_abi;
      TdsDAbi<T> pabi;
      tds_dyn_ld(w, L.xp + 12 * i, Xp);
      tds_dyn_ld(w, po, pabi);
      tds_d_abi_congruence_add(Xp, abi, pabi);
      tds_dyn_st(w, po, pabi);
    }
    if (l.joint_type == TDS_JOINT_FIXED) continue;  // :56
    const int qi = l.qd_index;
    TdsDSv<T> F;
    tds_d_abi_mulc(abi, l.S, F);              // :87
    w[M + qi * nd + qi] = tds_d_dot6c(l.S, F);  // :89
    int j = i;
    while (m->links[j].parent != -1) {  // :92-109
      tds_dyn_ld(w, L.xp + 12 * j, Xp);
      tds_d_apply_force(Xp, F, F);
      j = m->links[j].parent;
      if (m->links[j].joint_type == TDS_JOINT_FIXED) continue;
      const int qj = m->links[j].qd_index;
      const T h = tds_d_dot6c(m->links[j].S, F);
      w[M + qi * nd + qj] = h, w[M + qj * nd + qi] = h;
    }
    if (m->is_floating) {  // :111-115
      tds_dyn_ld(w, L.xp + 12 * j, Xp);
      tds_d_apply_force(Xp, F, F);
      for (int k = 0; k < 3; ++k) {
        w[M + k * nd + qi] = F.a[k], w[M + qi * nd + k] = F.a[k];
        w[M + (3 + k) * nd + qi] = F.l[k], w[M + qi * nd + 3 + k] = F.l[k];
      }
    }
  }
  if (m->is_floating) {  // :118-125
    TdsDAbi<T> b;
    tds_dyn_ld(w, L.base_abi, b);
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) {
        w[M + r * nd + c] = b.I[3 * r + c];
        w[M + r * nd + 3 + c] = b.H[3 * r + c];
        w[M + (3 + r) * nd + c] = b.H[3 * c + r];
        w[M + (3 + r) * nd + 3 + c] = b.M[3 * r + c];
      }
  }
}

// ---------------------------------------------------------------- forward dynamics through M = L L^T
// rhs (at L.rhs) = (tau - K q) - D qd: the spring and damper terms of forward_dynamics.hpp:122-123
template <typename T, class P>
TDS_HD inline void tds_dyn_rhs(const tds_model_t *m, P p, TdsDynMem<T> w, const TdsDynLayout &L) {
  for (int d = 0; d < m->dof_qd; ++d) w[L.rhs + d] = w[L.tau + d];
  for (int i = 0; i < m->num_links; ++i) {
    const tds_link_t &l = m->links[i];
    if (l.joint_type == TDS_JOINT_FIXED) continue;
    T t = w[L.rhs + l.qd_index];
    t = t - p.stiffness(m, i) * w[L.q + l.q_index];  // :122
    t = t - p.damping(m, i) * w[L.qd + l.qd_index];  // :123
    w[L.rhs + l.qd_index] = t;
  }
}

// qdd (at L.qdd) = M^-1 (((tau - K q) - D qd) - b), b at L.bias (tds_dyn_rnea with zero accelerations), as the step's
// contact solve factors and solves (tds_d_mass_matrix, tds_d_resolve: tiny_matrix_x.h:240-345); fixed base.  tau (at
// L.tau) holds dof_qd entries.
// Returns 0, or -1 where M is not positive definite (the caller makes the environment's qdd NaN).
template <typename T, class P>
TDS_HD inline int tds_dyn_solve(const tds_model_t *m, P p, TdsDynMem<T> w, const TdsDynLayout &L) {
  const int nd = m->dof_qd, F = L.L, x = L.qdd;
  for (int k = 0; k < nd * nd; ++k) w[F + k] = w[L.M + k];
  for (int i = 0; i < nd; ++i)  // L L^T = M, lower triangle in place (tiny_matrix_x.h:240-270)
    for (int j = i; j < nd; ++j) {
      T s = w[F + i * nd + j];
      for (int k = i - 1; k >= 0; --k) s = s - w[F + i * nd + k] * w[F + j * nd + k];
      if (i == j) {
        if (s <= 0.0) return -1;
        w[F + i * nd + i] = tds_sqrt(s);
      } else {
        w[F + j * nd + i] = s / w[F + i * nd + i];
      }
    }
  tds_dyn_rhs(m, p, w, L);
  for (int i = 0; i < nd; ++i) {  // L y = rhs - b
    T s = w[L.rhs + i] - w[L.bias + i];
    for (int k = 0; k < i; ++k) s = s - w[F + i * nd + k] * w[x + k];
    w[x + i] = s / w[F + i * nd + i];
  }
  for (int i = nd - 1; i >= 0; --i) {  // L^T qdd = y
    T s = w[x + i];
    for (int k = i + 1; k < nd; ++k) s = s - w[F + k * nd + i] * w[x + k];
    w[x + i] = s / w[F + i * nd + i];
  }
  return 0;
}

// The same on a floating base, where the reference's ABA does not solve M qdd = rhs exactly: it inverts the base's
// articulated inertia [I H; H^T M] with -H in the place of H^T (math/inertia.hpp:302-319, exact only while H is skew,
// which the inertia of a base with links is not), and the links' accelerations follow from that base acceleration.
// To give the reference's values, M is factored with the joints eliminated first (indices reversed: i' = dof_qd - 1 - i,
// M' = L' L'^T by the same loop): the joints' rows are solved forward, what they leave on the base's rows is
// z = -(p0 + B Hjj^-1 (rhs_j - b_j)) and S = Lbb Lbb^T = A - B Hjj^-1 B^T, the base's articulated inertia and bias
// force of forward_dynamics.hpp:187-207; the base's acceleration is the reference's inverse applied to z
// (tds_d_abi_inv_mul, :232), and the joints' rows are solved back with it in place.  base_f and base_abi (free after
// tds_dyn_crba) hold z and S.
template <typename T, class P>
TDS_HD inline int tds_dyn_solve_floating(const tds_model_t *m, P p, TdsDynMem<T> w, const TdsDynLayout &L) {
  const int nd = m->dof_qd, nj = nd - 6, F = L.L, x = L.qdd;
  for (int i = 0; i < nd; ++i)
    for (int j = 0; j < nd; ++j) w[F + i * nd + j] = w[L.M + (nd - 1 - i) * nd + (nd - 1 - j)];
  for (int i = 0; i < nd; ++i)
    for (int j = i; j < nd; ++j) {
      T s = w[F + i * nd + j];
      for (int k = i - 1; k >= 0; --k) s = s - w[F + i * nd + k] * w[F + j * nd + k];
      if (i == j) {
        if (s <= 0.0) return -1;
        w[F + i * nd + i] = tds_sqrt(s);
      } else {
        w[F + j * nd + i] = s / w[F + i * nd + i];
      }
    }
  tds_dyn_rhs(m, p, w, L);
  for (int i = 0; i < nj; ++i) {  // the joints' rows: Ljj y = rhs_j - b_j
    T s = w[L.rhs + nd - 1 - i] - w[L.bias + nd - 1 - i];
    for (int k = 0; k < i; ++k) s = s - w[F + i * nd + k] * w[x + k];
    w[x + i] = s / w[F + i * nd + i];
  }
  for (int b = 0; b < 6; ++b) {  // the base's rows
    const int i = nd - 1 - b;
    T s = w[L.rhs + b] - w[L.bias + b];
    for (int k = 0; k < nj; ++k) s = s - w[F + i * nd + k] * w[x + k];
    w[L.base_f + b] = s;
    for (int c = b; c < 6; ++c) {  // S[b][c], c >= b: i >= j
      const int j = nd - 1 - c;
      T t = T(0.0);
      for (int k = nj; k <= j; ++k) t = t + w[F + i * nd + k] * w[F + j * nd + k];
      if (c < 3) {
        w[L.base_abi + 3 * b + c] = t, w[L.base_abi + 3 * c + b] = t;
      } else if (b < 3) {
        w[L.base_abi + 9 + 3 * b + (c - 3)] = t;
      } else {
        w[L.base_abi + 18 + 3 * (b - 3) + (c - 3)] = t, w[L.base_abi + 18 + 3 * (c - 3) + (b - 3)] = t;
      }
    }
  }
  TdsDAbi<T> S;
  TdsDSv<T> z, a0;
  tds_dyn_ld(w, L.base_abi, S);
  tds_dyn_ld(w, L.base_f, z);
  tds_d_abi_inv_mul(S, z, a0);  // forward_dynamics.hpp:232
  for (int k = 0; k < 3; ++k) w[x + nd - 1 - k] = a0.a[k], w[x + nd - 4 - k] = a0.l[k];
  for (int i = nj - 1; i >= 0; --i) {  // Ljj^T qdd_j = y - Lbj^T a0
    T s = w[x + i];
    for (int k = i + 1; k < nd; ++k) s = s - w[F + k * nd + i] * w[x + k];
    w[x + i] = s / w[F + i * nd + i];
  }
  for (int i = 0; i < nd / 2; ++i) {  // back to the model's order
    const T t = w[x + i];
    w[x + i] = w[x + nd - 1 - i], w[x + nd - 1 - i] = t;
  }
  for (int k = 0; k < 3; ++k)  // :315-319: gravity's world components onto the base's linear acceleration
    w[x + 3 + k] = w[x + 3 + k] + p.gravity(m)[k];
  return 0;
}

// ---------------------------------------------------------------- point Jacobian
// ref: dynamics/jacobian.hpp:13-83 after tds_dyn_kinematics: jac [3][dof_qd] at L.jac, the world-frame Jacobian of the
// point at L.pt on link `li` (-1: the base).  is_local: the point is given in the link's own frame and taken to the
// world with X_world first; the columns are the world-frame ones either way.
template <typename T>
TDS_HD inline void tds_dyn_point_jacobian(const tds_model_t *m, TdsDynMem<T> w, const TdsDynLayout &L, int li,
                                          int is_local) {
  const int nd = m->dof_qd, J = L.jac;
  T pt[3] = {w[L.pt], w[L.pt + 1], w[L.pt + 2]};
  if (is_local) {
    TdsDXf<T> X;
    T r[3];
    tds_dyn_ld(w, li >= 0 ? L.xw + 12 * li : L.base, X);
    tds_d_mulv(X.r, pt, r);
    for (int k = 0; k < 3; ++k) pt[k] = X.t[k] + r[k];
  }
  for (int k = 0; k < 3 * nd; ++k) w[J + k] = T(0.0);
  if (m->is_floating) {  // :39-56  [ [r]x^T | 1 ],  r = point - base position
    const T r0 = pt[0] - w[L.base + 9], r1 = pt[1] - w[L.base + 10], r2 = pt[2] - w[L.base + 11];
    w[J + 1] = r2, w[J + 2] = -r1;
    w[J + nd] = -r2, w[J + nd + 2] = r0;
    w[J + 2 * nd] = r1, w[J + 2 * nd + 1] = -r0;
    w[J + 3] = T(1.0), w[J + nd + 4] = T(1.0), w[J + 2 * nd + 5] = T(1.0);
  }
  for (int i = li; i >= 0; i = m->links[i].parent) {
    const tds_link_t &l = m->links[i];
    if (l.joint_type == TDS_JOINT_FIXED) continue;
    TdsDXf<T> Xw;
    TdsDSv<T> st;
    T rxw[3];
    tds_dyn_ld(w, L.xw + 12 * i, Xw);
    tds_d_apply_inverse_motion(Xw, l.S, st);  // :74
    tds_d_cross(pt, st.a, rxw);               // :76
    for (int r = 0; r < 3; ++r) w[J + r * nd + l.qd_index] = st.l[r] - rxw[r];
  }
}

// ---------------------------------------------------------------- one environment's queries
enum { TDS_DYN_XW = 1, TDS_DYN_M = 2, TDS_DYN_BIAS = 4, TDS_DYN_QDD = 8, TDS_DYN_ID = 16, TDS_DYN_JAC = 32 };

// q, qd, tau (dof_qd entries) or qdd (TDS_DYN_ID) and the point are in place at L.q, L.qd, L.tau, L.qdd, L.pt.
// Afterwards: X_world at L.xw, M at L.M, the bias or ID's torques at L.bias, qdd at L.qdd, the Jacobian at L.jac, as
// `what` asks.  Returns -1 where qdd was asked for and M is not positive definite.
template <typename T, class P>
TDS_HD inline int tds_dyn_eval(const tds_model_t *m, P p, TdsDynMem<T> w, const TdsDynLayout &L, int what, int link,
                               int is_local) {
  const int dyn = what & (TDS_DYN_M | TDS_DYN_BIAS | TDS_DYN_QDD | TDS_DYN_ID);
  tds_dyn_kinematics(m, p, w, L, dyn ? 1 : 0);
  if (what & (TDS_DYN_BIAS | TDS_DYN_QDD | TDS_DYN_ID)) tds_dyn_rnea(m, p, w, L, (what & TDS_DYN_ID) ? L.qdd : -1, L.bias);
  if (what & (TDS_DYN_M | TDS_DYN_QDD)) tds_dyn_crba(m, p, w, L);
  if (what & TDS_DYN_JAC) tds_dyn_point_jacobian(m, w, L, link, is_local);
  if (what & TDS_DYN_QDD) return m->is_floating ? tds_dyn_solve_floating(m, p, w, L) : tds_dyn_solve(m, p, w, L);
  return 0;
}
