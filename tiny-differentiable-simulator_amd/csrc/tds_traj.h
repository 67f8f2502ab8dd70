// tds_traj.h — what the articulated trajectories' forward mode (tds_traj.hip) shares with their reverse mode
// (tds_traj_vjp.hip): the arguments, the lane's work object over TdsDual<K> and double, the item that advances an
// environment through its steps (kernels and host checkers alike), and the argument checks of the entry points.
#pragma once
#include <type_traits>

#include "tds_dparam.h"

namespace {

// steps per launch where TDS_OPT_TRAJ_STEPS is unset (Ant x 4096, one direction block: DESIGN 7a)
constexpr int kTrajStepsDefault = 16;

struct TdsTrajArgs {
  TdsJvpParamArgs a;   // m, n, kdirs, p, x = x0, theta (NULL: the blob's values), v, params; y and out unused
  int steps, every, n_rec, nsd, nact;
  const double *u;     // [n][steps - 1][nact] or NULL
  double *s, *js;      // [n][n_rec][nsd], [n][kdirs][n_rec][nsd]
  double *carry;       // [(nsd (K + 1) + 1)][items]
  long long items;
};

// a lane's work object: the forward-mode lane of tds_dparam.hip (K > 0), or the double lane and its record (K = 0)
template <class B, int K>
struct TdsTrajLane {
  using T = TdsDual<K>;
  TdsJvpParamLane<B, K> l;
  TDS_HD T *x() { return l.x; }
};
template <class B>
struct TdsTrajLane<B, 0> {
  using T = double;
  double xv[B::NX];
  TdsParamYLane<B> l;
  TDS_HD double *x() { return xv; }
};

template <int K>
TDS_HD inline double tds_traj_val(const TdsDual<K> &d) { return d.v; }
TDS_HD inline double tds_traj_val(double d) { return d; }

// doubles of an item's carry: the state's values and K tangents, and the NaN flag
template <int K>
TDS_HD inline int tds_traj_ncarry(int nsd) { return nsd * (K + 1) + 1; }

// advance item `item` (environment item % n, directions (item / n) K ..) from step t0 to t1 (0 <= t0 < t1 <= steps),
// writing the records of steps t0 + 1 .. t1; the state comes from the carry where t0 > 0 and goes back to it where
// t1 < steps.  Returns 1 where the joint-space inertia was not positive definite at some step so far.
template <class B, int K>
TDS_HD inline int tds_traj_advance(const TdsTrajArgs &ta, TdsTrajLane<B, K> &L, long long item, int t0, int t1) {
  using T = typename TdsTrajLane<B, K>::T;
  const TdsJvpParamArgs &a = ta.a;
  const tds_model_t *m = a.m;
  const int env = (int)(item % a.n), blk = (int)(item / a.n), d0 = blk * K;
  const int nin = m->input_dim, nsd = ta.nsd, nact = ta.nact;
  T *x = L.x(), *y = L.l.y;
  // the record, the overlay and the directions, as at step 0
  const double *xe = a.x + (size_t)env * nin;
  for (int i = 0; i < nin; ++i) x[i] = T(xe[i]);
  tds_param_seed(m, L.l.P);
  if (a.theta)
    for (int j = 0; j < a.p; ++j) tds_param_set(L.l.P, a.params[j], T(a.theta[(size_t)env * a.p + j]));
  if constexpr (K > 0) tds_jvp_param_seed_dirs<B, K>(a, L.l, env, d0);
  double bad = 0.0;
  const long long stride = ta.items;
  double *c = ta.carry + item;
  if (t0 > 0) {
    for (int i = 0; i < nsd; ++i) {
      if constexpr (K > 0) {
        x[i].v = c[(long long)i * (K + 1) * stride];
        for (int k = 0; k < K; ++k) x[i].d[k] = c[((long long)i * (K + 1) + 1 + k) * stride];
      } else {
        x[i] = c[(long long)i * stride];
      }
    }
    bad = c[(long long)nsd * (K + 1) * stride];
  }
  for (int t = t0; t < t1; ++t) {
    if (t > 0 && ta.u) {
      const double *ut = ta.u + ((size_t)env * (ta.steps - 1) + (t - 1)) * nact;
      for (int i = 0; i < nact; ++i) x[nsd + i] = T(ut[i]);
    }
    if (bad == 0.0 && tds_diff_step_view(m, TdsOverlayView<T, B>{&L.l.P}, L.l.w, x, y))
      bad = __builtin_nan("");  // M not positive definite: this record and every later one are NaN
    for (int i = 0; i < nsd; ++i) x[i] = y[i];
    if ((t + 1) % ta.every == 0) {
      const int r = (t + 1) / ta.every - 1;
      if (ta.s && blk == 0) {
        double *se = ta.s + ((size_t)env * ta.n_rec + r) * nsd;
        for (int i = 0; i < nsd; ++i) se[i] = tds_traj_val(y[i]) + bad;
      }
      if constexpr (K > 0)
        for (int k = 0; k < K && d0 + k < a.kdirs; ++k) {
          double *o = ta.js + (((size_t)env * a.kdirs + d0 + k) * ta.n_rec + r) * nsd;
          for (int i = 0; i < nsd; ++i) o[i] = y[i].d[k] + bad;
        }
    }
  }
  if (t1 < ta.steps) {
    for (int i = 0; i < nsd; ++i) {
      if constexpr (K > 0) {
        c[(long long)i * (K + 1) * stride] = x[i].v;
        for (int k = 0; k < K; ++k) c[((long long)i * (K + 1) + 1 + k) * stride] = x[i].d[k];
      } else {
        c[(long long)i * stride] = x[i];
      }
    }
    c[(long long)nsd * (K + 1) * stride] = bad;
  }
  return bad != 0.0;
}

// argument checks shared by the entry points (the model's checks follow)
int tds_traj_check_args(const char *fn, int n, int steps, int every, int k, int p, const void *x0, const void *params,
                        const void *v, const void *s, const void *js) {
  if (!x0 || n < 1 || k < 0 || p < 0 || (p > 0 && !params) || (k > 0 && (!v || !js)) || (k == 0 && !s))
    return fail(TDS_ERR_INVALID_ARG, fn, ": NULL or empty argument");
  if (steps < 1) return fail(TDS_ERR_INVALID_ARG, fn, ": steps must be at least 1");
  if (every < 1 || steps % every) return fail(TDS_ERR_INVALID_ARG, fn, ": every must divide steps");
  return TDS_OK;
}

TdsTrajArgs tds_traj_args(const tds_model_t *m, const tds_model_t *m_arg, int n, int steps, int every,
                          const double *x0, const double *u, int p, const double *theta, int k, const double *v,
                          double *s, double *js) {
  TdsTrajArgs ta;
  ta.a = {m_arg, n, k, p, x0, theta, v, nullptr, nullptr, nullptr};
  ta.steps = steps, ta.every = every, ta.n_rec = steps / every;
  ta.nsd = m->dof_q + m->dof_qd;
  ta.nact = m->input_dim - ta.nsd - (m->step_mode == TDS_STEP_LOCOMOTION ? 3 : 0);
  ta.u = u, ta.s = s, ta.js = js, ta.carry = nullptr, ta.items = 0;
  return ta;
}

}  // namespace
