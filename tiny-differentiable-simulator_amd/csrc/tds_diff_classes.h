// tds_diff_classes.h — what the two step-derivative translation units share (tds_jvp.hip: forward mode, tds_vjp.hip:
// reverse mode): the model classes and their bounds, the class of a model, the handle's checks and its work buffer.
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

// the handle's checks (f64, a supported model) and its device copy of the model blob
int tds_jvp_prepare(tds_hip_sim *s, int *cls);
// the handle's work buffer (d_diff_tmp) holds at least `need` bytes
int tds_jvp_tmp(tds_hip_sim *s, size_t need);

}  // namespace tds_internal
