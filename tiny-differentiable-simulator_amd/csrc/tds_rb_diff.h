// tds_rb_diff.h — what the derivative units of the rigid-body worlds share (tds_rb_diff.hip: forward mode,
// tds_rb_vjp.hip: reverse mode): the parameter selection and its checks, the model check, the lane's world accessors
// (values in LDS [component][lane], two more components per body for mass and inverse mass), the load of a world with
// its selected scalars made active, and the handle's work buffer.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include "tds_dual.h"
#include "tds_hip.h"
#include "tds_rb_internal.h"
#include "tds_rb_step.h"

#define RB_NCD 15         // components per body in the derivative lane: RB_NC + mass + inverse mass
#define RB_MASS 13
#define RB_INV_MASS 14
#define RB_MAX_SEL 32     // a valid selection has at most 16 masses + 3 gravity + friction + restitution

namespace {

template <int K>
struct RbScalar {
  typedef TdsDual<K> type;
};
template <>
struct RbScalar<0> {
  typedef double type;
};

// the selection, passed by value (kernel argument): kind and body / component per entry
struct RbSel {
  int p;
  int kind[RB_MAX_SEL], idx[RB_MAX_SEL];
};

// HBM offset (position | quaternion | linear | angular velocity) of component c of the step's order
__host__ __device__ __forceinline__ int rb_hbm(int c) { return c < 3 ? c : c < 6 ? c + 4 : c < 9 ? c + 4 : c - 6; }

// a scalar of value x whose tangents are direction d0 + kk's entry at col (col[(d0 + kk) * ld]), 0 past k
template <int K>
__host__ __device__ __forceinline__ typename RbScalar<K>::type rb_seed(double x, const double *col, int ld, int d0,
                                                                      int k) {
  if constexpr (K == 0) {
    return x;
  } else {
    TdsDual<K> r(x);
#pragma unroll
    for (int kk = 0; kk < K; ++kk) r.d[kk] = d0 + kk < k ? col[(size_t)(d0 + kk) * ld] : 0.0;
    return r;
  }
}

// the selectable scalars every accessor carries in registers (compile-time indices only)
template <typename T>
struct RbGlobals {
  T g[3], fr, rs;
};

// world of a device lane: values in LDS [(b * RB_NCD + c) * 64 + lane], tangents at tan[(b * RB_NCD + c) * K + kk) *
// stride] (tan already offset by the lane's item)
template <int K>
struct RbDevWorld : RbGlobals<typename RbScalar<K>::type> {
  typedef typename RbScalar<K>::type T;
  double *sm;
  int lane;
  double *tan;
  size_t stride;
  __device__ __forceinline__ T get(int b, int c) const {
    const int s = b * RB_NCD + c;
    if constexpr (K == 0) {
      return sm[s * 64 + lane];
    } else {
      TdsDual<K> r;
      r.v = sm[s * 64 + lane];
#pragma unroll
      for (int kk = 0; kk < K; ++kk) r.d[kk] = tan[((size_t)s * K + kk) * stride];
      return r;
    }
  }
  __device__ __forceinline__ void put(int b, int c, const T &x) {
    const int s = b * RB_NCD + c;
    if constexpr (K == 0) {
      sm[s * 64 + lane] = x;
    } else {
      sm[s * 64 + lane] = x.v;
#pragma unroll
      for (int kk = 0; kk < K; ++kk) tan[((size_t)s * K + kk) * stride] = x.d[kk];
    }
  }
  __device__ __forceinline__ T mass(int b) const { return get(b, RB_MASS); }
  __device__ __forceinline__ T inv_mass(int b) const { return get(b, RB_INV_MASS); }
  __device__ __forceinline__ T grav(int k) const { return this->g[k]; }
  __device__ __forceinline__ T restitution() const { return this->rs; }
  __device__ __forceinline__ T friction() const { return this->fr; }
};

// world on the host: one array per world
template <typename T>
struct RbHostWorld : RbGlobals<T> {
  T st[TDS_RB_MAX_BODIES * RB_NCD];
  T get(int b, int c) const { return st[b * RB_NCD + c]; }
  void put(int b, int c, const T &x) { st[b * RB_NCD + c] = x; }
  T mass(int b) const { return st[b * RB_NCD + RB_MASS]; }
  T inv_mass(int b) const { return st[b * RB_NCD + RB_INV_MASS]; }
  T grav(int k) const { return this->g[k]; }
  T restitution() const { return this->rs; }
  T friction() const { return this->fr; }
};

// s0 of one world, the model's selectable scalars, theta over the selected ones.  seed(x, col) makes the active scalar
// of value x that is column col of [state in HBM order | theta] (forward mode: its tangents; reverse mode: variable col)
template <typename T, typename W, typename Seed>
__host__ __device__ __forceinline__ void rb_load_seeded(W &w, const RbDev<double> &M, const double *s0w,
                                                        const RbSel &sel, const double *thw, const Seed &seed) {
  const int nb = M.nb;
  for (int b = 0; b < nb; ++b) {
    for (int c = 0; c < RB_NC; ++c) {
      const int h = b * TDS_RB_STATE + rb_hbm(c);
      w.put(b, c, seed(s0w[h], h));
    }
    w.put(b, RB_MASS, T(M.mass[b]));
    w.put(b, RB_INV_MASS, T(M.inv_mass[b]));
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) w.g[c] = T(M.grav[c]);
  w.fr = T(M.friction);
  w.rs = T(M.restitution);
  for (int j = 0; j < sel.p; ++j) {
    const int kind = sel.kind[j], q = sel.idx[j];
    double x0;
    if (kind == TDS_PARAM_LINK_MASS) x0 = M.mass[q];
    else if (kind == TDS_PARAM_GRAVITY) x0 = q == 0 ? M.grav[0] : q == 1 ? M.grav[1] : M.grav[2];
    else if (kind == TDS_PARAM_FRICTION) x0 = M.friction;
    else x0 = M.restitution;
    const T x = seed(thw ? thw[j] : x0, nb * TDS_RB_STATE + j);
    if (kind == TDS_PARAM_LINK_MASS) {
      w.put(q, RB_MASS, x);
      w.put(q, RB_INV_MASS, 1.0 / x);  // rigid_body.hpp:49-53 (dynamic bodies only)
    } else if (kind == TDS_PARAM_GRAVITY) {
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if (q == c) w.g[c] = x;
    } else if (kind == TDS_PARAM_FRICTION) {
      w.fr = x;
    } else {
      w.rs = x;
    }
  }
}

// The forward-mode load keeps its own statement of the same handling: written through rb_load_seeded (a seed functor
// that reads the tangents), tds_rb_jvp_kernel<2> kept its instruction count and resource figures but came out with a
// different register allocation, and tds_rb_jvp measured 2.3 % slower on the billiard scene.
// s0 of one world, the model's selectable scalars, theta over the selected ones; tangents of directions d0.. from
// vw [k][nb * 13 + p] (vw unused when K = 0)
template <int K, typename W>
__host__ __device__ __forceinline__ void rb_load(W &w, const RbDev<double> &M, const double *s0w, const RbSel &sel,
                                                 const double *thw, const double *vw, int k, int d0) {
  typedef typename RbScalar<K>::type T;
  const int nb = M.nb, ld = nb * TDS_RB_STATE + sel.p;
  for (int b = 0; b < nb; ++b) {
    for (int c = 0; c < RB_NC; ++c) {
      const int h = b * TDS_RB_STATE + rb_hbm(c);
      w.put(b, c, rb_seed<K>(s0w[h], vw + h, ld, d0, k));
    }
    w.put(b, RB_MASS, T(M.mass[b]));
    w.put(b, RB_INV_MASS, T(M.inv_mass[b]));
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) w.g[c] = T(M.grav[c]);
  w.fr = T(M.friction);
  w.rs = T(M.restitution);
  for (int j = 0; j < sel.p; ++j) {
    const int kind = sel.kind[j], q = sel.idx[j];
    double x0;
    if (kind == TDS_PARAM_LINK_MASS) x0 = M.mass[q];
    else if (kind == TDS_PARAM_GRAVITY) x0 = q == 0 ? M.grav[0] : q == 1 ? M.grav[1] : M.grav[2];
    else if (kind == TDS_PARAM_FRICTION) x0 = M.friction;
    else x0 = M.restitution;
    const T x = rb_seed<K>(thw ? thw[j] : x0, vw + nb * TDS_RB_STATE + j, ld, d0, k);
    if (kind == TDS_PARAM_LINK_MASS) {
      w.put(q, RB_MASS, x);
      w.put(q, RB_INV_MASS, 1.0 / x);  // rigid_body.hpp:49-53 (dynamic bodies only)
    } else if (kind == TDS_PARAM_GRAVITY) {
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if (q == c) w.g[c] = x;
    } else if (kind == TDS_PARAM_FRICTION) {
      w.fr = x;
    } else {
      w.rs = x;
    }
  }
}

inline int rb_model_check(const tds_rb_model_t *m) {
  if (m->abi_version != TDS_HIP_ABI_VERSION) return tds_rb_fail(TDS_ERR_INVALID_ARG, "model abi_version mismatch");
  if (m->num_bodies < 1 || m->num_bodies > TDS_RB_MAX_BODIES)
    return tds_rb_fail(TDS_ERR_INVALID_ARG, "num_bodies out of range");
  if (m->solver_iterations < 0 || !(m->dt > 0)) return tds_rb_fail(TDS_ERR_INVALID_ARG, "bad solver_iterations / dt");
  for (int i = 0; i < m->num_bodies; ++i)
    if (m->bodies[i].geom_type != TDS_GEOM_SPHERE && m->bodies[i].geom_type != TDS_GEOM_PLANE &&
        m->bodies[i].geom_type != TDS_GEOM_CAPSULE && m->bodies[i].geom_type != TDS_GEOM_BOX)
      return tds_rb_fail(TDS_ERR_UNSUPPORTED, "rigid bodies support sphere, plane, capsule and box geometries");
  return TDS_OK;
}

// checks a selection and fills sel
inline int rb_check_sel(const tds_rb_model_t *m, int p, const tds_param_t *params, RbSel *sel) {
  char msg[160];
  if (p < 0) return tds_rb_fail(TDS_ERR_INVALID_ARG, "p < 0");
  if (p > 0 && !params) return tds_rb_fail(TDS_ERR_INVALID_ARG, "params is NULL");
  sel->p = 0;
  for (int j = 0; j < p; ++j) {
    const tds_param_t &q = params[j];
    int idx;
    if (q.kind == TDS_PARAM_LINK_MASS) {
      if (q.link < 0 || q.link >= m->num_bodies || q.comp != 0) {
        snprintf(msg, sizeof(msg), "params[%d]: body %d out of range (num_bodies %d)", j, q.link, m->num_bodies);
        return tds_rb_fail(TDS_ERR_INVALID_ARG, msg);
      }
      if (m->bodies[q.link].mass == 0.0) {
        snprintf(msg, sizeof(msg), "params[%d]: body %d is static (mass 0): its mass is not selectable", j, q.link);
        return tds_rb_fail(TDS_ERR_INVALID_ARG, msg);
      }
      idx = q.link;
    } else if (q.kind == TDS_PARAM_GRAVITY) {
      if (q.link != 0 || q.comp < 0 || q.comp > 2) {
        snprintf(msg, sizeof(msg), "params[%d]: gravity needs link 0 and comp 0..2", j);
        return tds_rb_fail(TDS_ERR_INVALID_ARG, msg);
      }
      idx = q.comp;
    } else if (q.kind == TDS_PARAM_FRICTION || q.kind == TDS_PARAM_RESTITUTION) {
      if (q.link != 0 || q.comp != 0) {
        snprintf(msg, sizeof(msg), "params[%d]: friction / restitution need link 0 and comp 0", j);
        return tds_rb_fail(TDS_ERR_INVALID_ARG, msg);
      }
      idx = 0;
    } else {
      snprintf(msg, sizeof(msg),
               "params[%d]: kind %d is not selectable for rigid bodies (mass, gravity, friction, restitution)", j,
               q.kind);
      return tds_rb_fail(TDS_ERR_INVALID_ARG, msg);
    }
    for (int i = 0; i < j; ++i)
      if (sel->kind[i] == q.kind && sel->idx[i] == idx) {
        snprintf(msg, sizeof(msg), "params[%d] duplicates params[%d]", j, i);
        return tds_rb_fail(TDS_ERR_INVALID_ARG, msg);
      }
    sel->kind[j] = q.kind;
    sel->idx[j] = idx;
    sel->p = j + 1;
  }
  return TDS_OK;
}

// the handle's work buffer holds at least `need` bytes (kept for the next call; `what` names it in the message)
inline int rb_work_buffer(tds_rb_sim *s, size_t need, const char *what) {
  if (need <= s->work_bytes) return TDS_OK;
  if (s->d_work) (void)hipFree(s->d_work);
  s->d_work = nullptr;
  s->work_bytes = 0;
  if (hipMalloc(&s->d_work, need) != hipSuccess) {
    char msg[128];
    snprintf(msg, sizeof(msg), "hipMalloc of the %zu B %s failed", need, what);
    return tds_rb_fail(TDS_ERR_HIP, msg);
  }
  s->work_bytes = need;
  return TDS_OK;
}

}  // namespace
