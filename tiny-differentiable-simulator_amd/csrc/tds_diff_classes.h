// tds_diff_classes.h — what the seven units beside the step kernels share: the step derivatives (tds_jvp.hip: forward
// mode, tds_vjp.hip: reverse mode, tds_dparam.hip: both in [x | theta], tds_traj.hip: trajectories) and the queries
// (tds_dyn.hip, tds_ik.hip, tds_contact.hip; their own plumbing is tds_query.h's).  The model classes and their bounds,
// the class of a model and the dispatch over it, the forward-mode tangents and lanes per launch, the checks of a handle
// and of a host checker's model, and the handle's work buffer.
#pragma once
#include "tds_api_internal.h"
#include "tds_diff_step.h"

// model classes: the smallest bound a model fits is taken (tds_jvp_pick)
// (links, dofs, contact points, visuals)
using TdsBoundS = TdsDiffBounds<8, 8, 8, 8>;      // cartpole, pendulum5 (+ plane), cube_floating
using TdsBoundA = TdsDiffBounds<14, 14, 17, 9>;   // ant, ant_floating, cartpole_plane (two boxes: 16 points)
using TdsBoundL = TdsDiffBounds<22, 18, 4, 17>;   // laikago, laikago_soft, laikago_floating(_env)

namespace tds_internal {

// 0..2: class S, A, L; -1: refused (why set)
inline int tds_jvp_pick(const tds_model_t *m, const char **why) {
  if (!m) return *why = "NULL model", -1;
  if (tds_diff_check<TdsBoundS>(m, why) == 0) return 0;
  if (tds_diff_check<TdsBoundA>(m, why) == 0) return 1;
  if (tds_diff_check<TdsBoundL>(m, why) == 0) return 2;
  return -1;
}

// f over the bound of class cls (0..2), as a tag: f(b) with `typename decltype(b)::type` TdsBoundS, A or L
template <class B>
struct TdsBoundTag { using type = B; };
template <class F>
auto tds_with_bound(int cls, F &&f) {
  switch (cls) {
    case 0: return f(TdsBoundTag<TdsBoundS>{});
    case 1: return f(TdsBoundTag<TdsBoundA>{});
    default: return f(TdsBoundTag<TdsBoundL>{});
  }
}

// a host checker's model: its class (refusals as tds_jvp_pick words them) and the blob's indices in range (a handle's
// model passed that at creation)
inline int tds_diff_host_check(const tds_model_t *m, int *cls) {
  const char *why = "";
  *cls = tds_jvp_pick(m, &why);
  if (*cls < 0) return fail(TDS_ERR_UNSUPPORTED, "%s", why);
  return tds_hip_model_check(m);
}

// tangents per lane of each class on the device (the lane's work object grows with K + 1)
template <class B>
struct TdsJvpK;
template <>
struct TdsJvpK<TdsBoundS> { static constexpr int K = 4; };
template <>
struct TdsJvpK<TdsBoundA> { static constexpr int K = 2; };
template <>
struct TdsJvpK<TdsBoundL> { static constexpr int K = 2; };

// lanes of one launch: each walks the (environment, direction block) items with the grid's stride.  The cap bounds the
// work buffer (kJvpLanes work objects: 0.9 - 1.2 GB); it also leaves three of four SIMDs without a wave at the kernel's
// occupancy of one
constexpr long long kJvpLanes = 16384;

// lanes of a launch over n environments x kdirs directions: one per item, at most kJvpLanes
template <class B>
long long tds_jvp_lanes(int n, int kdirs) {
  constexpr int K = TdsJvpK<B>::K;
  const long long items = (long long)n * ((kdirs + K - 1) / K);
  return items < kJvpLanes ? items : kJvpLanes;
}

// the handle's checks (f64, a supported model) and its device copy of the model blob
int tds_diff_prepare(tds_hip_sim *s, int *cls);
// the handle's work buffer (d_diff_tmp) holds at least `need` bytes
int tds_work_buffer(tds_hip_sim *s, size_t need);

}  // namespace tds_internal
