// tds_contact.h — one single-source, scalar-templated statement of the batched contact query (tds_contact.hip): what
// the step forward_zero(x) does about its plane contacts — the contact points, their point Jacobians, the constraint
// rows J and right-hand side b, the Delassus matrix A = J M^-1 J^T + cfm 1, the PGS impulses p, the world-frame contact
// forces and the velocities before and after the solve.  Instantiated over double and the blob's view on the host (the
// checker) and on the device (tds_contact.hip), and over TdsDual<K> and an overlay of parameters for the query's
// forward-mode derivatives in [x | theta] (tds_contact_jvp.hip): every selectable scalar of the contact model
// (friction, restitution, cfm, erp, the shapes' radius, length, extents and X_trans) is read through the view P, the
// contact points' offsets are formed in P::geom_scalar<T>; dt, the plane and the shapes' rotations are blob constants.
//
// It is built from tds_dyn.h: the kinematics, CRBA, bias (RNEA), the Cholesky solve for qdd (with tds_dyn.h's
// floating-base arrangement, so that qd_pre is the reference's ABA's) and the point Jacobian, on the state reached
// through TdsDynMem (component i of this environment is p[i * s]: [component][lane] on the device, stride 1 on the
// host).  The helpers of tds_diff_step.h are used read only.  The statement of record for the narrowphase, the rows,
// W = M^-1 J^T by two triangular solves and PGS through u = W^T p is tds_d_contacts / tds_d_resolve there; the
// expressions below are theirs, term for term, over memory components instead of a struct per lane.  Nothing that is
// indexed at run time lives in a local array.  "ref:" = file:line under the reference's src/.
#pragma once
#include "tds_dyn.h"

enum {
  TDS_CT_CONTACTS = 1, TDS_CT_JAC = 2, TDS_CT_ROWS = 4, TDS_CT_RHS = 8, TDS_CT_DELASSUS = 16, TDS_CT_IMPULSE = 32,
  TDS_CT_FORCE = 64, TDS_CT_QD_PRE = 128, TDS_CT_QD_POST = 256
};

// contact points of a geometry against the plane (keep_all_points_: every point of every geometry, contact_point.hpp)
static inline TDS_HD int tds_contact_points(int geom_type) {
  return geom_type == TDS_GEOM_SPHERE ? 1 : geom_type == TDS_GEOM_CAPSULE ? 2 : geom_type == TDS_GEOM_BOX ? 8 : 0;
}
// n_c: a constant of the model (0 without a plane), in the order of tds_d_contacts
static inline TDS_HD int tds_contact_count(const tds_model_t *m) {
  int nc = 0;
  if (m->has_plane)
    for (int g = 0; g < m->num_geoms; ++g) nc += tds_contact_points(m->geoms[g].type);
  return nc;
}

// the outputs a set of pointers asks for (those with extent: without contact points only qd_pre and qd_post)
static inline int tds_contact_what(const tds_contact_out_t *o, int nc) {
  int what = (o->qd_pre ? TDS_CT_QD_PRE : 0) | (o->qd_post ? TDS_CT_QD_POST : 0);
  if (nc)
    what |= (o->contacts ? TDS_CT_CONTACTS : 0) | (o->jac ? TDS_CT_JAC : 0) | (o->rows ? TDS_CT_ROWS : 0) |
            (o->rhs ? TDS_CT_RHS : 0) | (o->delassus ? TDS_CT_DELASSUS : 0) | (o->impulse ? TDS_CT_IMPULSE : 0) |
            (o->force ? TDS_CT_FORCE : 0);
  return what;
}

static inline int tds_contact_any(const tds_contact_out_t *o) {
  return o->contacts || o->jac || o->rows || o->rhs || o->delassus || o->impulse || o->force || o->qd_pre || o->qd_post;
}

// component offsets of one environment's state: tds_dyn.h's, then the record x, then the contact quantities
struct TdsContactLayout {
  TdsDynLayout D;
  int nc, x, cp, cjac, J, W, b, p, u, A, force, qd_pre, qd_post, total;
};
// with_A: whether the Delassus matrix (the largest block, 9 n_c^2) has a place
static inline TDS_HD TdsContactLayout tds_contact_layout(const tds_model_t *m, int with_A) {
  const int nd = m->dof_qd, nc = tds_contact_count(m), nr = 3 * nc;
  TdsContactLayout L;
  L.D = tds_dyn_layout(m);
  L.nc = nc;
  int o = L.D.total;
  L.x = o, o += m->input_dim;
  L.cp = o, o += 10 * nc;
  L.cjac = o, o += 3 * nd * nc;
  L.J = o, o += nr * nd;
  L.W = o, o += nr * nd;
  L.b = o, o += nr;
  L.p = o, o += nr;
  L.u = o, o += nd;
  L.force = o, o += nr;
  L.qd_pre = o, o += nd;
  L.qd_post = o, o += nd;
  L.A = o, o += with_A ? nr * nr : 0;
  L.total = o;
  return L;
}

// ---------------------------------------------------------------- actuation
// q, qd and tau (dof_qd entries) from the record at L.x, as tds_diff_step_view reads them (tds_diff_step.h:874-895).
// ref: examples/environments/locomotion_contact_simulation.h:164-257 (PD), multi_body.hpp:557-570 (torques)
template <typename T>
TDS_HD inline void tds_contact_actuate(const tds_model_t *m, TdsDynMem<T> w, const TdsContactLayout &L) {
  const int nq = m->dof_q, nd = m->dof_qd, x = L.x;
  for (int i = 0; i < nq; ++i) w[L.D.q + i] = w[x + i];
  for (int i = 0; i < nd; ++i) w[L.D.qd + i] = w[x + nq + i], w[L.D.tau + i] = T(0.0);
  if (m->step_mode == TDS_STEP_LOCOMOTION) {
    const int act = nq + nd, var = nq + nd + m->action_dim;
    const T kp = w[x + var], kd = w[x + var + 1], max_force = w[x + var + 2];  // :164-166
    int pose = 0;
    for (int i = m->pd_start_link; i < m->num_links; ++i) {  // :181-257
      const tds_link_t &l = m->links[i];
      if (l.joint_type == TDS_JOINT_FIXED) continue;
      T a = w[x + act + pose];
      if (a > m->action_limit) a = T(m->action_limit);  // :235-236
      if (a < -m->action_limit) a = T(-m->action_limit);
      const T q_des = m->initial_poses[pose++] + a;  // :238
      T f = kp * (q_des - w[L.D.q + l.q_index]) + kd * (0.0 - w[L.D.qd + l.qd_index]);  // :242-245
      if (f < -max_force) f = -max_force;  // :247
      if (f > max_force) f = max_force;
      w[L.D.tau + l.qd_index] = f;
    }
  } else {
    const int off = m->is_floating ? 6 : 0;
    for (int i = 0; i < nd - off; ++i) w[L.D.tau + off + i] = w[x + nq + nd + i];
  }
}

// L L^T = M in the model's order at L.D.L (tiny_matrix_x.h:240-270), as tds_d_mass_matrix factors it: what the step's
// contact solve uses on every base (tds_dyn_solve leaves it there on a fixed base; tds_dyn_solve_floating leaves the
// factor of the reversed order).  Returns -1 where M is not positive definite.
template <typename T>
TDS_HD inline int tds_contact_factor(const tds_model_t *m, TdsDynMem<T> w, const TdsDynLayout &D) {
  const int nd = m->dof_qd, F = D.L;
  for (int k = 0; k < nd * nd; ++k) w[F + k] = w[D.M + k];
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
  return 0;
}

// ---------------------------------------------------------------- rotation -> quaternion with constant indices
// tds_d_matrix_to_quat (tiny_matrix3x3.h:432-465), whose negative-trace branch indexes the matrix and the quaternion
// by the largest diagonal entry at run time (96 + 8 B of private segment per lane on the device).  The same
// expressions, the three cases spelled out over a constant index: registers only.
template <int i, typename T>
TDS_HD inline void tds_contact_quat_case(const T *m, T *e) {
  constexpr int j = (i + 1) % 3, k = (i + 2) % 3;
  T s = tds_sqrt(((m[4 * i] - m[4 * j]) - m[4 * k]) + 1.0);
  e[i] = s * 0.5;
  s = 0.5 / s;
  e[3] = (m[3 * j + k] - m[3 * k + j]) * s;
  e[j] = (m[3 * i + j] + m[3 * j + i]) * s;
  e[k] = (m[3 * i + k] + m[3 * k + i]) * s;
}
template <typename T>
TDS_HD inline void tds_contact_matrix_to_quat(const T *m, T *q) {
  T tr = m[0] + m[4] + m[8], e[4];
  if (tr < 0.0) {
    const int i = m[0] < m[4] ? (m[4] < m[8] ? 2 : 1) : (m[0] < m[8] ? 2 : 0);
    if (i == 0)
      tds_contact_quat_case<0>(m, e);
    else if (i == 1)
      tds_contact_quat_case<1>(m, e);
    else
      tds_contact_quat_case<2>(m, e);
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

// ---------------------------------------------------------------- the shapes' scalars through the view
// radius, capsule length, box extents and X_trans of geometry g (G = m->geoms[g], which the caller holds) as the view
// gives them: p.geom_*(m, g).  The blob's view has overloads that read G itself: the same doubles, and the primal kernel
// keeps its code to the instruction (through the view's own m->geoms[g] the compiler forms the addresses anew:
// tds_contact_kernel 13 815 -> 13 989 instructions, 174 -> 240 SGPR spills).
template <class P>
TDS_HD inline decltype(auto) tds_contact_radius(P p, const tds_model_t *m, int g, const tds_geom_t &) {
  return p.geom_radius(m, g);
}
template <class P>
TDS_HD inline decltype(auto) tds_contact_length(P p, const tds_model_t *m, int g, const tds_geom_t &) {
  return p.geom_length(m, g);
}
template <class P>
TDS_HD inline decltype(auto) tds_contact_extents(P p, const tds_model_t *m, int g, const tds_geom_t &) {
  return p.geom_extents(m, g);
}
template <class P>
TDS_HD inline decltype(auto) tds_contact_trans(P p, const tds_model_t *m, int g, const tds_geom_t &) {
  return p.geom_trans(m, g);
}
TDS_HD inline double tds_contact_radius(TdsBlobView, const tds_model_t *, int, const tds_geom_t &G) { return G.radius; }
TDS_HD inline double tds_contact_length(TdsBlobView, const tds_model_t *, int, const tds_geom_t &G) { return G.length; }
TDS_HD inline const double *tds_contact_extents(TdsBlobView, const tds_model_t *, int, const tds_geom_t &G) {
  return G.extents;
}
TDS_HD inline const double *tds_contact_trans(TdsBlobView, const tds_model_t *, int, const tds_geom_t &G) {
  return G.X_trans;
}

// ---------------------------------------------------------------- narrowphase, point Jacobians, rows
// ref: world.hpp:206-282 (plane = multi body a, the robot b), contact_point.hpp:96-198; per point the ten numbers
// world_normal_on_b | world_point_on_b | world_point_on_a | distance at L.cp, point_jacobian2(robot, link_b,
// world_point_on_b) at L.cjac (jacobian.hpp:13-90) and, with rows, the solver's J rows and b
// (mb_constraint_solver.hpp:278-388) at the velocities at L.qd_pre.  Rows of a separated point are zero.
template <typename T, class P>
TDS_HD inline void tds_contact_points_and_rows(const tds_model_t *m, P p, TdsDynMem<T> w, const TdsContactLayout &L,
                                               int rows) {
  typedef typename P::template geom_scalar<T> S;  // the shapes' scalars: the contact points' offsets are formed in it
  const int nd = m->dof_qd, nc = L.nc;
  const double *n = m->plane_normal;
  double nrm[3] = {-n[0], -n[1], -n[2]}, f1[3], f2[3];
  tds_d_plane_space(nrm, f1, f2);  // :361
  int c = 0;
  for (int g = 0; g < m->num_geoms; ++g) {
    const tds_geom_t &G = m->geoms[g];
    const int np = tds_contact_points(G.type);
    if (!np) continue;
    TdsDXf<T> X, tr;
    tds_dyn_ld(w, G.link >= 0 ? L.D.xw + 12 * G.link : L.D.base, X);
    tds_d_xf_mul(X, G.X_rot, tds_contact_trans(p, m, g, G), tr);  // world.hpp:242
    T orn[4];
    tds_contact_matrix_to_quat(tr.r, orn);  // world.hpp:244-245
    tds_d_quat_normalize(orn);
    S rad = tds_contact_radius(p, m, g, G), dx = S(0.0), dy = S(0.0), dz = S(0.0);
    if (G.type == TDS_GEOM_CAPSULE) {  // contact_point.hpp:127-161
      dz = 0.5 * tds_contact_length(p, m, g, G);
    } else if (G.type == TDS_GEOM_BOX) {  // :163-198, geometry.hpp:244-259; a branch of the primal (tds_d_contacts)
      rad = rad > 1e-2 ? rad : S(1e-2);
      const auto ext = tds_contact_extents(p, m, g, G);
      dx = ext[0] * 0.5 - rad, dy = ext[1] * 0.5 - rad, dz = ext[2] * 0.5 - rad;
    }
    for (int e = 0; e < np; ++e, ++c) {
      T pos[3];
      if (G.type == TDS_GEOM_SPHERE) {
        for (int k = 0; k < 3; ++k) pos[k] = tr.t[k];
      } else {
        S off[3];
        if (G.type == TDS_GEOM_CAPSULE)
          off[0] = S(0.0), off[1] = S(0.0), off[2] = e == 0 ? dz : -dz;
        else
          off[0] = (e & 4) ? -dx : dx, off[1] = (e & 2) ? -dy : dy, off[2] = (e & 1) ? -dz : dz;
        T ro[3];
        tds_d_quat_rotate(orn, off, ro);  // pose.hpp:47-53
        for (int k = 0; k < 3; ++k) pos[k] = tr.t[k] + ro[k];
      }
      // :96-125  t = -(pos . (-n) + constant); point_a = pos + t (-n); point_b = pos - r n; distance = t - r
      const T t = -((pos[0] * -n[0] + pos[1] * -n[1] + pos[2] * -n[2]) + m->plane_constant);
      const T dist = t - rad;
      const int cp = L.cp + 10 * c;
      for (int k = 0; k < 3; ++k) {
        w[cp + k] = T(nrm[k]);
        w[cp + 3 + k] = pos[k] - rad * n[k];
        w[cp + 6 + k] = pos[k] + t * -n[k];
      }
      w[cp + 9] = dist;
      TdsDynLayout Dc = L.D;  // the point and its Jacobian in this contact's own places
      Dc.pt = cp + 3, Dc.jac = L.cjac + 3 * nd * c;
      tds_dyn_point_jacobian(m, w, Dc, G.link, 0);  // :295
      if (!rows) continue;
      const int j = Dc.jac;
      const bool hit = dist < 0.0;  // :285 collision = distance < 0
      T vel[3];                     // :314  jac_b qd
      for (int r = 0; r < 3; ++r) {
        T s = T(0.0);
        for (int d = 0; d < nd; ++d) s = s + w[j + r * nd + d] * w[L.qd_pre + d];
        vel[r] = s;
      }
      // rel_vel = -vel (:315); b rows (:321-325, :365-370), J rows (:300-307, :378-384)
      const T nrv = -(nrm[0] * vel[0] + nrm[1] * vel[1] + nrm[2] * vel[2]);
      w[L.b + c] = hit ? (-(1.0 + p.restitution(m)) * nrv - p.erp(m) * dist / m->dt) : T(0.0);
      w[L.b + nc + c] = hit ? (f1[0] * vel[0] + f1[1] * vel[1] + f1[2] * vel[2]) : T(0.0);
      w[L.b + 2 * nc + c] = hit ? (f2[0] * vel[0] + f2[1] * vel[1] + f2[2] * vel[2]) : T(0.0);
      for (int d = 0; d < nd; ++d) {
        const T j0 = w[j + d], j1 = w[j + nd + d], j2 = w[j + 2 * nd + d];
        w[L.J + c * nd + d] = hit ? j0 * nrm[0] + j1 * nrm[1] + j2 * nrm[2] : T(0.0);
        w[L.J + (nc + c) * nd + d] = hit ? j0 * f1[0] + j1 * f1[1] + j2 * f1[2] : T(0.0);
        w[L.J + (2 * nc + c) * nd + d] = hit ? j0 * f2[0] + j1 * f2[1] + j2 * f2[2] : T(0.0);
      }
    }
  }
}

// ---------------------------------------------------------------- W = M^-1 J^T, A, PGS, forces, qd_post
// ref: mb_constraint_solver.hpp:392-498, solve_pgs :101-142.  W_r by L y = J_r^T, L^T W_r = y (a separated point's
// rows are zero, and so is its W_r: its solves are left out); PGS on A = J M^-1 J^T + cfm 1 through u = W^T p:
// (A p)_r = J_r . u + cfm p_r.
template <typename T, class P>
TDS_HD inline void tds_contact_solve(const tds_model_t *m, P p, TdsDynMem<T> w, const TdsContactLayout &L, int what) {
  const int nd = m->dof_qd, nc = L.nc, nr = 3 * nc, F = L.D.L;
  for (int r = 0; r < nr; ++r) {
    const int x = L.W + r * nd, J = L.J + r * nd;
    if (!(w[L.cp + 10 * (r % nc) + 9] < 0.0)) {
      for (int i = 0; i < nd; ++i) w[x + i] = T(0.0);
      continue;
    }
    for (int i = 0; i < nd; ++i) {
      T s = w[J + i];
      for (int k = 0; k < i; ++k) s = s - w[F + i * nd + k] * w[x + k];
      w[x + i] = s / w[F + i * nd + i];
    }
    for (int i = nd - 1; i >= 0; --i) {
      T s = w[x + i];
      for (int k = i + 1; k < nd; ++k) s = s - w[F + k * nd + i] * w[x + k];
      w[x + i] = s / w[F + i * nd + i];
    }
  }
  if (what & TDS_CT_DELASSUS)  // :392-412: the lower triangle, mirrored
    for (int r = 0; r < nr; ++r)
      for (int s = 0; s <= r; ++s) {
        T a = T(0.0);
        for (int d = 0; d < nd; ++d) a = a + w[L.J + r * nd + d] * w[L.W + s * nd + d];
        if (r == s) a = a + p.cfm(m);
        w[L.A + r * nr + s] = a, w[L.A + s * nr + r] = a;
      }
  if (!(what & (TDS_CT_IMPULSE | TDS_CT_FORCE | TDS_CT_QD_POST))) return;
  for (int d = 0; d < nd; ++d) w[L.u + d] = T(0.0);
  for (int r = 0; r < nr; ++r) w[L.p + r] = T(0.0);
  for (int it = 0; it < m->pgs_iterations; ++it)
    for (int r = 0; r < nr; ++r) {
      T Ju = T(0.0), Arr = T(0.0);
      for (int d = 0; d < nd; ++d) {
        const T j = w[L.J + r * nd + d];
        Ju = Ju + j * w[L.u + d], Arr = Arr + j * w[L.W + r * nd + d];
      }
      const T pr = w[L.p + r];
      const T delta = Ju - Arr * pr;
      T x = (w[L.b + r] - delta) / (Arr + p.cfm(m));
      if (r < nc) {  // normal: [0, 1e5]  (:417-424)
        x = tds_clamp(x, T(0.0), T(100000.0));
      } else {  // friction: +-mu max(p_normal, 0)  (:426-436)
        const T pn = w[L.p + r % nc], sc = pn < 0.0 ? T(0.0) : pn;
        const T lo = -p.friction(m) * sc, hi = p.friction(m) * sc;
        if (x < lo) x = lo;  // Algebra::max
        if (x > hi) x = hi;  // Algebra::min
      }
      const T dx = x - pr;
      w[L.p + r] = x;
      for (int d = 0; d < nd; ++d) w[L.u + d] = w[L.u + d] + w[L.W + r * nd + d] * dx;
    }
  if (what & TDS_CT_FORCE) {  // the force on the robot at world_point_on_b: -(N p_n + t1 p_f1 + t2 p_f2) / dt
    const double *n = m->plane_normal;
    double nrm[3] = {-n[0], -n[1], -n[2]}, f1[3], f2[3];
    tds_d_plane_space(nrm, f1, f2);
    for (int c = 0; c < nc; ++c) {
      const T pn = w[L.p + c], p1 = w[L.p + nc + c], p2 = w[L.p + 2 * nc + c];
      for (int k = 0; k < 3; ++k) w[L.force + 3 * c + k] = -(nrm[k] * pn + f1[k] * p1 + f2[k] * p2) / m->dt;
    }
  }
  for (int d = 0; d < nd; ++d) {  // :476-496  qd -= M^-1 J^T p
    T s = T(0.0);
    for (int r = 0; r < nr; ++r) s = s + w[L.W + r * nd + d] * w[L.p + r];
    w[L.qd_post + d] = w[L.qd_pre + d] - s;
  }
}

// ---------------------------------------------------------------- one environment's query
// The record is in place at L.x.  Afterwards the outputs `what` asks for are at L.cp, L.cjac, L.J, L.b, L.A, L.p,
// L.force, L.qd_pre and L.qd_post.  Returns -1 where M is not positive definite: L.cp and L.cjac are valid then, and
// the caller makes the environment's other outputs NaN.
template <typename T, class P>
TDS_HD inline int tds_contact_eval(const tds_model_t *m, P p, TdsDynMem<T> w, const TdsContactLayout &L, int what) {
  const int nd = m->dof_qd, nc = L.nc;
  const int dyn = what & ~(TDS_CT_CONTACTS | TDS_CT_JAC);
  const int solve = nc > 0 && (what & (TDS_CT_DELASSUS | TDS_CT_IMPULSE | TDS_CT_FORCE | TDS_CT_QD_POST));
  const int rows = nc > 0 && (solve || (what & (TDS_CT_ROWS | TDS_CT_RHS)));
  int bad = 0;
  tds_contact_actuate(m, w, L);
  if (dyn) {
    // forward dynamics (tds_diff_step.h:896) and integrate_euler_qdd (:897-903, integrator.hpp:141-182)
    bad = tds_dyn_eval(m, p, w, L.D, TDS_DYN_M | TDS_DYN_QDD, 0, 0);
    if (!bad && m->is_floating && rows) bad = tds_contact_factor(m, w, L.D);
    for (int d = 0; d < nd; ++d) w[L.qd_pre + d] = w[L.D.qd + d] + w[L.D.qdd + d] * m->dt;
  } else {
    tds_dyn_kinematics(m, p, w, L.D, 0);
  }
  if (nc > 0 && (rows || (what & (TDS_CT_CONTACTS | TDS_CT_JAC)))) tds_contact_points_and_rows(m, p, w, L, rows && !bad);
  if (bad) return -1;
  if (solve)
    tds_contact_solve(m, p, w, L, what);
  else
    for (int d = 0; d < nd; ++d) w[L.qd_post + d] = w[L.qd_pre + d];  // no contact points: the solver does nothing
  return 0;
}
