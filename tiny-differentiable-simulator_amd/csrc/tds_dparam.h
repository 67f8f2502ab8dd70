// tds_dparam.h — what the parameter derivatives (tds_dparam.hip) share with the articulated trajectories
// (tds_traj.hip): the forward-mode lane's work object over [x | theta] and its direction seeding, the double lane of y
// at theta, and the selection checks of the entry points.
#pragma once
#include <vector>

#include "tds_diff_classes.h"

namespace {

using namespace tds_internal;

constexpr int kHostK = 8;  // tangents per evaluation on the host

// ---------------------------------------------------------------- forward mode
// directions v[n][kdirs][input_dim + p] -> jv[n][kdirs][output_dim]; kdirs = 0: y only
struct TdsJvpParamArgs {
  const tds_model_t *m;
  int n, kdirs, p;
  const double *x, *theta, *v;
  const tds_param_t *params;
  double *y, *out;
};

template <class B, int K>
struct TdsJvpParamLane {
  TdsDual<K> x[B::NX], y[B::NY];
  TdsParamOverlay<TdsDual<K>, B> P;
  TdsDiffWork<TdsDual<K>, B> w;
};

// the tangents of directions d0 .. d0 + K - 1 (those below kdirs) of environment env: x's from v, and theta's in both
// slots of each selected scalar (an off-diagonal inertia entry sets its mirror too).  tds_jvp_param_eval states the same
// loop in its own body: called from there, this function changes the register allocation of tds_jvp_param_kernel
// (A: 338 -> 340 VGPR spills, private segment 2420 -> 2436 B), whose code stays as measured
template <class B, int K>
TDS_HD inline void tds_jvp_param_seed_dirs(const TdsJvpParamArgs &a, TdsJvpParamLane<B, K> &L, int env, int d0) {
  const int nin = a.m->input_dim, nall = nin + a.p;
  for (int k = 0; k < K && d0 + k < a.kdirs; ++k) {
    const double *ve = a.v + ((size_t)env * a.kdirs + d0 + k) * nall;
    for (int i = 0; i < nin; ++i) L.x[i].d[k] = ve[i];
    for (int j = 0; j < a.p; ++j) {
      tds_param_slot(L.P, a.params[j], 0)->d[k] = ve[nin + j];
      tds_param_slot(L.P, a.params[j], 1)->d[k] = ve[nin + j];
    }
  }
}

// evaluate environment env with directions d0 .. d0 + K - 1 (those below kdirs); 0 or the step's -1
template <class B, int K>
TDS_HD inline int tds_jvp_param_eval(const TdsJvpParamArgs &a, TdsJvpParamLane<B, K> &L, int env, int d0) {
  using D = TdsDual<K>;
  const tds_model_t *m = a.m;
  const int nin = m->input_dim;
  const double *xe = a.x + (size_t)env * nin, *th = a.theta + (size_t)env * a.p;
  for (int i = 0; i < nin; ++i) L.x[i] = D(xe[i]);
  tds_param_seed(m, L.P);
  for (int j = 0; j < a.p; ++j) tds_param_set(L.P, a.params[j], D(th[j]));
  const int nall = nin + a.p;
  for (int k = 0; k < K && d0 + k < a.kdirs; ++k) {
    const double *ve = a.v + ((size_t)env * a.kdirs + d0 + k) * nall;
    for (int i = 0; i < nin; ++i) L.x[i].d[k] = ve[i];
    for (int j = 0; j < a.p; ++j) {
      tds_param_slot(L.P, a.params[j], 0)->d[k] = ve[nin + j];
      tds_param_slot(L.P, a.params[j], 1)->d[k] = ve[nin + j];
    }
  }
  return tds_diff_step_view(m, TdsOverlayView<D, B>{&L.P}, L.w, L.x, L.y);
}

// y only (k = 0): the double step over an overlay of doubles, a lane's work object (no tangents: about a third of the
// dual lane's bytes)
template <class B>
struct TdsParamYLane {
  double y[B::NY];
  TdsParamOverlay<double, B> P;
  TdsDiffWork<double, B> w;
};

// ---------------------------------------------------------------- checks shared by the entry points
inline int tds_param_check_sel(const tds_model_t *m, int p, const tds_param_t *params) {
  const char *why = "";
  if (tds_param_check(m, p, params, &why)) return fail(TDS_ERR_INVALID_ARG, "%s", why);
  return TDS_OK;
}

// the host entry points' model checks: class (refusals as for the Jacobians), blob indices, selection
inline int tds_param_host_prepare(const tds_model_t *m, int p, const tds_param_t *params, int *cls) {
  const int rc = tds_diff_host_check(m, cls);
  return rc ? rc : tds_param_check_sel(m, p, params);
}

}  // namespace
