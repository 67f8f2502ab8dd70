// tds_vjp_param.h — what the parameter derivatives' reverse mode (tds_dparam.hip) shares with the trajectories'
// reverse mode (tds_traj_vjp.hip): the tape bound per class in parameter mode, the arguments and the lane's work
// object over [x | theta] in TdsRev form.
#pragma once
#include "tds_dparam.h"
#include "tds_vjp_kernels.h"

namespace {

// tape entries a lane may record in parameter mode, per class: the longest tape counted with every selectable
// parameter of the model selected, over each model's tests/golden records and the contact sweep of
// tests/diff_states.py (pendulum5_plane 14 248, ant 73 128, laikago 70 355), plus 29 %, 18 % and 16 %
template <class B>
struct TdsVjpParamCap;
template <>
struct TdsVjpParamCap<TdsBoundS> { static constexpr int N = 18432; };
template <>
struct TdsVjpParamCap<TdsBoundA> { static constexpr int N = 86016; };
template <>
struct TdsVjpParamCap<TdsBoundL> { static constexpr int N = 81920; };

// ---------------------------------------------------------------- reverse mode
struct TdsVjpParamArgs : TdsVjpArgs {
  int p;
  const tds_param_t *params;
  const double *theta;
};

// a lane's work object in parameter mode: the record, the overlay and the step's state in TdsRev form
template <class B>
struct TdsVjpParamLane {
  static constexpr int cap = TdsVjpParamCap<B>::N;
  TdsRev x[B::NX], y[B::NY];
  TdsParamOverlay<TdsRev, B> P;
  TdsDiffWork<TdsRev, B> w;
  TDS_HD static int n_extra(const TdsVjpParamArgs &a) { return a.p; }
  // x: variables 0 .. input_dim - 1, theta: input_dim .. input_dim + p - 1
  TDS_HD int record(const TdsVjpParamArgs &a, long long env) {
    const tds_model_t *m = a.m;
    const int nin = m->input_dim;
    const double *xe = a.x + env * nin, *th = a.theta + env * a.p;
    for (int i = 0; i < nin; ++i) x[i] = TdsRev(xe[i], i);
    tds_param_seed(m, P);
    for (int j = 0; j < a.p; ++j) tds_param_set(P, a.params[j], TdsRev(th[j], nin + j));
    tds_rev_cursor(tds_rev_lane()) = 0;
    return tds_diff_step_view(m, TdsOverlayView<TdsRev, B>{&P}, w, x, y);
  }
};

}  // namespace
