// tds_rb_step.h — one statement of World::step for worlds of free rigid bodies (tds_rb.hip, tds_rb_diff.hip,
// tds_rb_vjp.hip).
//
// Reference: src/world.hpp:293-366 (step: gravity impulse, pairwise narrowphase, num_solver_iterations sweeps of
// RigidBodyConstraintSolver::resolve_collision over the contacts, integrate), src/rigid_body.hpp:26-123,
// src/rb_constraint_solver.hpp:112-165 (the non-CppAD branch), src/contact_point.hpp:43-198, 405-438, 468-496.
//
// tds_rb_world_steps<T, R>(M, S, steps) is a __host__ __device__ template over the state scalar T and a state
// accessor S; R is the real type of the model table RbDev<R>.  tds_rb_diff.hip instantiates it for T = TdsDual<K> and
// double, tds_rb_vjp.hip for TdsRev (reverse mode) and double, each on the device and on the host.  It is the
// arithmetic of tds_rb_kernel (tds_rb.hip), which keeps its own
// statement: instantiated from this template, the kernel's f64 build compiled to the same code, but its f32 build
// vectorised differently and changed results in the last bits ("Rigid-body rollouts").  The model table,
// its builder and the vector helpers are shared.
// The accessor owns every read of a selectable model scalar (mass, inverse mass, gravity, friction, restitution), so
// that the derivative kernels can make them active; the rest of the model (geometry, dt, erp, inverse inertia) is
// read from M.  Comparisons of T read the value only: a derivative follows the branch the primal takes.
//
// Accessor interface (T the scalar):
//   T get(int b, int c);  void put(int b, int c, const T &x);    c: 0..2 position, 3..5 linear, 6..8 angular velocity,
//                                                                   9..12 orientation quaternion (x, y, z, w)
//   T mass(int b);  T inv_mass(int b);  T grav(int k);  T restitution();  T friction();
#pragma once
#include <math.h>
#include <string.h>

#include "tds_dual.h"
#include "tds_hip.h"

#define RB_NC 13

template <typename T>
struct RbDev {
  int nb, iters;
  T dt, grav[3], restitution, friction, erp;
  T mass[TDS_RB_MAX_BODIES], inv_mass[TDS_RB_MAX_BODIES], inv_in[TDS_RB_MAX_BODIES];
  T radius[TDS_RB_MAX_BODIES];  // of the body's collision spheres (box: max(1e-2, corner radius))
  T pn[TDS_RB_MAX_BODIES][3], pc[TDS_RB_MAX_BODIES];
  int type[TDS_RB_MAX_BODIES];
  int ns[TDS_RB_MAX_BODIES];    // collision spheres of the body: sphere 1, capsule 2, box 8 (plane 0)
  T off[TDS_RB_MAX_BODIES][8][3];  // their centres in body coordinates
};

template <typename T>
__host__ __device__ __forceinline__ void cross3(const T *a, const T *b, T *o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
template <typename T, typename V>
__host__ __device__ __forceinline__ T dot3(const T *a, const V *b) {
  return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}

// q v q^-1 for a unit quaternion (x, y, z, w) — tiny_quaternion.h:171-176
template <typename T, typename V>
__host__ __device__ __forceinline__ void quat_rotate(const T *q, const V *v, T *o) {
  const T t0 = q[3] * v[0] + q[1] * v[2] - q[2] * v[1];
  const T t1 = q[3] * v[1] + q[2] * v[0] - q[0] * v[2];
  const T t2 = q[3] * v[2] + q[0] * v[1] - q[1] * v[0];
  const T t3 = -q[0] * v[0] - q[1] * v[1] - q[2] * v[2];
  const T i0 = -q[0], i1 = -q[1], i2 = -q[2], i3 = q[3];
  o[0] = t3 * i0 + t0 * i3 + t1 * i2 - t2 * i1;
  o[1] = t3 * i1 + t1 * i3 + t2 * i0 - t0 * i2;
  o[2] = t3 * i2 + t2 * i3 + t0 * i1 - t1 * i0;
}

// the device table of a model (host)
template <typename T>
inline void rb_build(const tds_rb_model_t *m, RbDev<T> *d) {
  memset(d, 0, sizeof(*d));
  d->nb = m->num_bodies;
  d->iters = m->solver_iterations;
  d->dt = (T)m->dt;
  for (int k = 0; k < 3; ++k) d->grav[k] = (T)m->gravity[k];
  d->restitution = (T)m->restitution;
  d->friction = (T)m->friction;
  d->erp = (T)m->erp;
  for (int i = 0; i < m->num_bodies; ++i) {
    const tds_rb_body_t &b = m->bodies[i];
    d->mass[i] = (T)b.mass;
    d->inv_mass[i] = b.mass == 0.0 ? T(0) : (T)(1.0 / b.mass);  // rigid_body.hpp:49-53
    d->inv_in[i] = b.mass == 0.0 ? T(0) : T(1);                  // zero33 / eye3
    d->type[i] = b.geom_type;
    double rad = b.radius;
    if (b.geom_type == TDS_GEOM_SPHERE) {
      d->ns[i] = 1;
    } else if (b.geom_type == TDS_GEOM_CAPSULE) {  // contact_point.hpp:143-158
      d->ns[i] = 2;
      d->off[i][0][2] = (T)(0.5 * b.length);
      d->off[i][1][2] = (T)(-0.5 * b.length);
    } else if (b.geom_type == TDS_GEOM_BOX) {      // contact_point.hpp:179-196, geometry.hpp:244-259
      d->ns[i] = 8;
      rad = b.radius > 1e-2 ? b.radius : 1e-2;
      const double dx = b.extents[0] * 0.5 - rad, dy = b.extents[1] * 0.5 - rad, dz = b.extents[2] * 0.5 - rad;
      for (int c = 0; c < 8; ++c) {
        d->off[i][c][0] = (T)((c & 4) ? -dx : dx);
        d->off[i][c][1] = (T)((c & 2) ? -dy : dy);
        d->off[i][c][2] = (T)((c & 1) ? -dz : dz);
      }
    }
    d->radius[i] = (T)rad;
    // Plane's constructor normalises the normal (geometry.hpp:163-168) as v * (1 / |v|) (tiny_algebra.hpp:223); a
    // non-unit normal rounds differently under v / |v|
    double nl = sqrt(b.plane_normal[0] * b.plane_normal[0] + b.plane_normal[1] * b.plane_normal[1] +
                     b.plane_normal[2] * b.plane_normal[2]);
    if (nl == 0.0) nl = 1.0;
    const double inl = 1.0 / nl;
    for (int k = 0; k < 3; ++k) d->pn[i][k] = (T)(b.plane_normal[k] * inl);
    d->pc[i] = (T)b.plane_constant;
  }
}

__host__ __device__ __forceinline__ float rb_sqrt(float x) { return sqrt(x); }
__host__ __device__ __forceinline__ double rb_sqrt(double x) { return sqrt(x); }
template <int K>
__host__ __device__ __forceinline__ TdsDual<K> rb_sqrt(const TdsDual<K> &x) {
  return tds_sqrt(x);
}

// Hooks of a recording scalar type (reverse mode, tds_rb_vjp.hip overloads them for TdsRev): the tape position at the top
// of a collision sphere's narrowphase, and the return to it where the sphere ends without an impulse.  Nothing computed
// since the mark is then read again and no state was written, so what a tape recorded in between is dead.  Every other
// scalar type has no tape: the hooks are empty and compile to nothing.
template <typename T>
__host__ __device__ __forceinline__ int rb_tape_mark(const T *) {
  return 0;
}
template <typename T>
__host__ __device__ __forceinline__ void rb_tape_rewind(const T *, int) {}

// `steps` World::step calls on the world behind S
template <typename T, typename R, typename S>
__host__ __device__ __forceinline__ void tds_rb_world_steps(const RbDev<R> &M, S &s, int steps) {
  const int nb = M.nb;
  const R dt = M.dt;
  for (int st = 0; st < steps; ++st) {
    // apply_gravity + apply_force_impulse + clear_forces (world.hpp:301-310, rigid_body.hpp:81-97)
    for (int b = 0; b < nb; ++b) {
#pragma unroll
      for (int k = 0; k < 3; ++k) s.put(b, 3 + k, s.get(b, 3 + k) + (s.mass(b) * s.grav(k)) * s.inv_mass(b) * dt);
    }
    // num_solver_iterations sweeps over the contacts in pair order i < j (world.hpp:163-191, 336-340)
    for (int it = 0; it < M.iters; ++it) {
      for (int i = 0; i < nb; ++i) {
        for (int j = i + 1; j < nb; ++j) {
          const int ti = M.type[i], tj = M.type[j];  // wave-uniform
          // dispatcher (contact_point.hpp:444-496): P = the plane or the lone sphere, the other body is
          // expanded into its collision spheres; swapped = the reference ran the pair as (j, i)
          int pp, qq, kind;  // kind 0: plane(pp) vs spheres of qq;  1: spheres of pp (capsule / sphere) vs sphere qq
          bool swapped = false;
          const bool jball = tj == TDS_GEOM_SPHERE || tj == TDS_GEOM_CAPSULE || tj == TDS_GEOM_BOX;
          const bool iball = ti == TDS_GEOM_SPHERE || ti == TDS_GEOM_CAPSULE || ti == TDS_GEOM_BOX;
          if (ti == TDS_GEOM_PLANE && jball) {
            pp = i; qq = j; kind = 0;
          } else if (tj == TDS_GEOM_PLANE && iball) {
            pp = j; qq = i; kind = 0; swapped = true;
          } else if ((ti == TDS_GEOM_SPHERE || ti == TDS_GEOM_CAPSULE) && tj == TDS_GEOM_SPHERE) {
            pp = i; qq = j; kind = 1;
          } else if (ti == TDS_GEOM_SPHERE && tj == TDS_GEOM_CAPSULE) {
            pp = j; qq = i; kind = 1; swapped = true;
          } else {
            continue;
          }
          const int eb = kind == 0 ? qq : pp;  // the expanded body
          const T pi[3] = {s.get(i, 0), s.get(i, 1), s.get(i, 2)};
          const T pj[3] = {s.get(j, 0), s.get(j, 1), s.get(j, 2)};
          const T qe[4] = {s.get(eb, 9), s.get(eb, 10), s.get(eb, 11), s.get(eb, 12)};
          const T pe[3] = {s.get(eb, 0), s.get(eb, 1), s.get(eb, 2)};
          const R rad = M.radius[eb];
          for (int sx = 0; sx < M.ns[eb]; ++sx) {
          const int mark = rb_tape_mark((const T *)nullptr);
          T ctr[3];
          if (M.type[eb] == TDS_GEOM_SPHERE) {
            ctr[0] = pe[0]; ctr[1] = pe[1]; ctr[2] = pe[2];
          } else {  // Pose * offset (pose.hpp:47-53)
            const R ov[3] = {M.off[eb][sx][0], M.off[eb][sx][1], M.off[eb][sx][2]};
            T r3[3];
            quat_rotate(qe, ov, r3);
            ctr[0] = pe[0] + r3[0]; ctr[1] = pe[1] + r3[1]; ctr[2] = pe[2] + r3[2];
          }
          T nbv[3], pa[3], pb[3], dist;
          bool got;
          if (kind == 0) {  // contact_plane_sphere (contact_point.hpp:96-125): A = plane, B = sphere at ctr
            const R mn[3] = {-M.pn[pp][0], -M.pn[pp][1], -M.pn[pp][2]};
            const T t = -(dot3(ctr, mn) + M.pc[pp]);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
              pa[k] = ctr[k] + t * mn[k];
              pb[k] = ctr[k] - rad * M.pn[pp][k];
              nbv[k] = T(mn[k]);
            }
            dist = t - rad;
            got = true;
          } else {          // contact_sphere_sphere (contact_point.hpp:43-94): A = sphere at ctr, B = body qq
            const T cq[3] = {s.get(qq, 0), s.get(qq, 1), s.get(qq, 2)};
            const T diff[3] = {ctr[0] - cq[0], ctr[1] - cq[1], ctr[2] - cq[2]};
            const T length = rb_sqrt(dot3(diff, diff));
            dist = length - (rad + M.radius[qq]);
            got = length > R(1) / R(100000);
            const T il = R(1) / length;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
              nbv[k] = il * diff[k];
              pa[k] = ctr[k] - rad * nbv[k];
              pb[k] = pa[k] - dist * nbv[k];
            }
          }
          if (swapped) {  // swap normal and points a, b (contact_point.hpp:484-491)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
              const T t = pa[k];
              pa[k] = pb[k];
              pb[k] = t;
              nbv[k] = -nbv[k];
            }
          }
          // RigidBodyConstraintSolver::resolve_collision (rb_constraint_solver.hpp:112-165)
          if (!(got && dist < R(0))) {
            rb_tape_rewind((const T *)nullptr, mark);
            continue;
          }
          T ra[3], rb[3], wa[3], wb[3], va[3], vb[3], rel[3], t3[3];
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            ra[k] = pa[k] - pi[k];
            rb[k] = pb[k] - pj[k];
            wa[k] = s.get(i, 6 + k);
            wb[k] = s.get(j, 6 + k);
          }
          const T baumgarte = M.erp * dist / dt;
          cross3(wa, ra, t3);
#pragma unroll
          for (int k = 0; k < 3; ++k) va[k] = s.get(i, 3 + k) + t3[k];
          cross3(wb, rb, t3);
#pragma unroll
          for (int k = 0; k < 3; ++k) vb[k] = s.get(j, 3 + k) + t3[k];
#pragma unroll
          for (int k = 0; k < 3; ++k) rel[k] = va[k] - vb[k];
          const T nrv = dot3(nbv, rel);
          if (!(nrv < R(0))) {
            rb_tape_rewind((const T *)nullptr, mark);
            continue;
          }
          T t1[3], t2[3], x1[3], x2[3], sum[3];
          cross3(ra, nbv, t1);
          cross3(rb, nbv, t2);
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            t1[k] = t1[k] * M.inv_in[i];
            t2[k] = t2[k] * M.inv_in[j];
          }
          cross3(t1, ra, x1);
          cross3(t2, rb, x2);
#pragma unroll
          for (int k = 0; k < 3; ++k) sum[k] = x1[k] + x2[k];
          const T ang = dot3(nbv, sum);
          const T denom = s.inv_mass(i) + s.inv_mass(j) + ang;
          const T impulse = (-(R(1) + s.restitution()) * nrv - baumgarte) / denom;
          if (!(impulse > R(0))) {
            rb_tape_rewind((const T *)nullptr, mark);
            continue;
          }
          T iv[3], miv[3];
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            iv[k] = impulse * nbv[k];
            miv[k] = -iv[k];
          }
          // apply_impulse (rigid_body.hpp:103-108)
          cross3(ra, iv, t3);
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            s.put(i, 3 + k, s.get(i, 3 + k) + s.inv_mass(i) * iv[k]);
            s.put(i, 6 + k, s.get(i, 6 + k) + M.inv_in[i] * t3[k]);
          }
          cross3(rb, miv, t3);
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            s.put(j, 3 + k, s.get(j, 3 + k) + s.inv_mass(j) * miv[k]);
            s.put(j, 6 + k, s.get(j, 6 + k) + M.inv_in[j] * t3[k]);
          }
          // Coulomb friction from the PRE-impulse relative velocity
          T lat[3];
#pragma unroll
          for (int k = 0; k < 3; ++k) lat[k] = rel[k] - nrv * nbv[k];
          const T latn = rb_sqrt(dot3(lat, lat));
          const T trial = latn / denom;
          const T fimp = trial < s.friction() * impulse ? trial : s.friction() * impulse;
          if (latn > R(1) / R(10000)) {
            T fa[3], fb[3];
            const T il = R(1) / latn;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
              const T fd = lat[k] * il;
              fa[k] = -fimp * fd;
              fb[k] = fimp * fd;
            }
            cross3(ra, fa, t3);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
              s.put(i, 3 + k, s.get(i, 3 + k) + s.inv_mass(i) * fa[k]);
              s.put(i, 6 + k, s.get(i, 6 + k) + M.inv_in[i] * t3[k]);
            }
            cross3(rb, fb, t3);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
              s.put(j, 3 + k, s.get(j, 3 + k) + s.inv_mass(j) * fb[k]);
              s.put(j, 6 + k, s.get(j, 6 + k) + M.inv_in[j] * t3[k]);
            }
          }
          }  // collision spheres of the expanded body
        }
      }
    }
    // integrate (rigid_body.hpp:116-122, tiny_algebra.hpp:604-614)
    for (int b = 0; b < nb; ++b) {
#pragma unroll
      for (int k = 0; k < 3; ++k) s.put(b, k, s.get(b, k) + s.get(b, 3 + k) * dt);
      {
        const T qx = s.get(b, 9), qy = s.get(b, 10), qz = s.get(b, 11), qw = s.get(b, 12);
        const T w0 = s.get(b, 6), w1 = s.get(b, 7), w2 = s.get(b, 8);
        const R hd = R(0.5) * dt;
        const T ww = (-qx * w0 - qy * w1 - qz * w2) * hd;
        const T xx = (qw * w0 + qz * w1 - qy * w2) * hd;
        const T yy = (qw * w1 + qx * w2 - qz * w0) * hd;
        const T zz = (qw * w2 + qy * w0 - qx * w1) * hd;
        const T nx = qx + xx, ny = qy + yy, nz = qz + zz, nw = qw + ww;
        const T ql = rb_sqrt(nx * nx + ny * ny + nz * nz + nw * nw);
        s.put(b, 9, nx / ql);
        s.put(b, 10, ny / ql);
        s.put(b, 11, nz / ql);
        s.put(b, 12, nw / ql);
      }
    }
  }
}
