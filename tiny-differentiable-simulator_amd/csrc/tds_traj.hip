// tds_traj.hip — forward-mode derivatives of articulated-body trajectories on gfx950: forward_zero chained over
// `steps` steps (tds_diff_step_view, the statement the step derivatives use), with the states recorded every `every`
// steps and their tangents in [x0 | theta].  C ABI tds_hip_trajectory_jvp / tds_hip_trajectory_jvp_host
// (include/tds_hip.h).
//
// Step 0 reads the record x0 as forward_zero reads it.  Step t >= 1 reads [y_{t-1}'s q | qd | u[t-1] | x0's gains]
// (u NULL: x0's action slots every step).  The actions of u are inputs, not differentiated; x0's action slots (u NULL)
// and gains are, through every step.  theta replaces the blob's values of the selection for the whole trajectory.
//
// Mapping: one work item per (environment, block of K directions), K and the 16384-lane cap as in tds_dparam.hip's
// forward-mode kernel, whose lane (TdsJvpParamLane) and direction seeding (tds_jvp_param_seed_dirs) this unit reuses:
// the work objects sit in the handle's work buffer.  No launch runs the whole trajectory: a launch advances every item
// by at most TDS_OPT_TRAJ_STEPS steps, and between launches an item's state duals ((nq + nd) (K + 1) doubles) and
// its NaN flag wait in a carry buffer behind the work objects, item-minor.  A launch re-seeds the record, the overlay
// and the directions from x0, theta and v, then takes the state from the carry: copies only, so the chunking is
// invisible in the results.  k = 0 runs the double step over an overlay of doubles (TdsParamYLane).
//
// One function (tds_traj_advance) is the kernels' item and the host checker's loop, over TdsDual<K> and double.  The
// unit is built without FP contraction (Makefile), so that device and host round alike over many steps.
#include <hip/hip_runtime.h>
#include <string.h>
#include "tds_traj.h"

namespace {

// steps t0 .. t1 of every item, lanes walking the items with the grid's stride
template <class B, int K>
__global__ void __launch_bounds__(64) tds_traj_jvp_kernel(TdsTrajArgs ta, TdsTrajLane<B, K> *lanes, long long n_lanes,
                                                          int t0, int t1) {
  const long long lane = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= n_lanes) return;
  for (long long it = lane; it < ta.items; it += n_lanes) tds_traj_advance<B, K>(ta, lanes[lane], it, t0, t1);
}

// k = 0: the double step, one item per environment
template <class B>
__global__ void __launch_bounds__(64) tds_traj_y_kernel(TdsTrajArgs ta, TdsTrajLane<B, 0> *lanes, long long n_lanes,
                                                        int t0, int t1) {
  const long long lane = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= n_lanes) return;
  for (long long it = lane; it < ta.items; it += n_lanes) tds_traj_advance<B, 0>(ta, lanes[lane], it, t0, t1);
}

// the work buffer: the lanes' work objects | the carry | the selection
struct TdsTrajLayout {
  long long n_lanes;
  size_t lanes_bytes, carry_bytes, total;
};

template <class B, int K>
TdsTrajLayout tds_traj_layout(const TdsTrajArgs &ta, int p) {
  TdsTrajLayout l;
  l.n_lanes = ta.items < kJvpLanes ? ta.items : kJvpLanes;
  l.lanes_bytes = ((size_t)l.n_lanes * sizeof(TdsTrajLane<B, K>) + 255) & ~(size_t)255;
  l.carry_bytes = ta.steps > 1 ? (((size_t)tds_traj_ncarry<K>(ta.nsd) * ta.items * sizeof(double) + 255) & ~(size_t)255)
                               : 0;
  l.total = l.lanes_bytes + l.carry_bytes + (size_t)p * sizeof(tds_param_t);
  return l;
}

template <class B, int K>
int tds_traj_run(tds_hip_sim *s, TdsTrajArgs ta, const tds_param_t *params_host) {
  ta.items = (long long)ta.a.n * (K > 0 ? (ta.a.kdirs + K - 1) / K : 1);
  const TdsTrajLayout lay = tds_traj_layout<B, K>(ta, ta.a.p);
  int rc = tds_work_buffer(s, lay.total);
  if (rc) return rc;
  char *ws = (char *)s->d_diff_tmp;
  ta.carry = (double *)(ws + lay.lanes_bytes);
  tds_param_t *d_sel = (tds_param_t *)(ws + lay.lanes_bytes + lay.carry_bytes);
  if (ta.a.p > 0) {  // a blocking copy: earlier calls on the stream may still read the work buffer
    TDS_HIP_TRY(hipStreamSynchronize(s->stream));
    TDS_HIP_TRY(hipMemcpy(d_sel, params_host, (size_t)ta.a.p * sizeof(tds_param_t), hipMemcpyHostToDevice));
  }
  ta.a.params = d_sel;
  const long long opt = s->opt.get(TDS_OPT_TRAJ_STEPS, kTrajStepsDefault);
  const int chunk = opt < 1 ? 1 : opt > ta.steps ? ta.steps : (int)opt;
  const unsigned blocks = (unsigned)((lay.n_lanes + 63) / 64);
  auto *lanes = (TdsTrajLane<B, K> *)ws;
  for (int t0 = 0; t0 < ta.steps; t0 += chunk) {
    const int t1 = t0 + chunk < ta.steps ? t0 + chunk : ta.steps;
    if constexpr (K > 0)
      hipLaunchKernelGGL((tds_traj_jvp_kernel<B, K>), dim3(blocks), dim3(64), 0, s->stream, ta, lanes, lay.n_lanes, t0,
                         t1);
    else
      hipLaunchKernelGGL((tds_traj_y_kernel<B>), dim3(blocks), dim3(64), 0, s->stream, ta, lanes, lay.n_lanes, t0, t1);
    TDS_HIP_TRY(hipGetLastError());
  }
  return TDS_OK;
}

template <class B>
int tds_traj_dispatch(tds_hip_sim *s, const TdsTrajArgs &ta, const tds_param_t *params_host) {
  return ta.a.kdirs > 0 ? tds_traj_run<B, TdsJvpK<B>::K>(s, ta, params_host) : tds_traj_run<B, 0>(s, ta, params_host);
}

// the host instantiation: s from the double step, js from TdsDual<kHostK>, each item in one pass (no carry)
template <class B>
int tds_traj_host_impl(TdsTrajArgs ta) {
  std::vector<TdsTrajLane<B, kHostK>> L(1);
  std::vector<TdsTrajLane<B, 0>> Ly(1);
  const int kd = ta.a.kdirs, blocks = (kd + kHostK - 1) / kHostK;
  double *s = ta.s;
  int bad = 0;
  for (int e = 0; e < ta.a.n; ++e) {
    ta.items = ta.a.n;
    ta.s = s;
    bad |= tds_traj_advance<B, 0>(ta, Ly[0], e, 0, ta.steps);
    ta.items = (long long)ta.a.n * blocks;
    ta.s = nullptr;
    for (int b = 0; b < blocks; ++b) bad |= tds_traj_advance<B, kHostK>(ta, L[0], (long long)b * ta.a.n + e, 0, ta.steps);
  }
  return bad ? fail(TDS_ERR_INVALID_ARG, "step Jacobians: joint-space inertia not positive definite%s") : TDS_OK;
}

}  // namespace

extern "C" {

int tds_hip_trajectory_jvp(tds_hip_sim_t *s, int n, int steps, int every, const void *x0_dev, const void *u_dev,
                           int p, const tds_param_t *params_host, const void *theta_dev, int k, const void *v_dev,
                           void *s_dev, void *js_dev) {
  if (!s) return fail(TDS_ERR_INVALID_ARG, "tds_hip_trajectory_jvp: NULL or empty argument%s");
  int rc = tds_traj_check_args("tds_hip_trajectory_jvp%s", n, steps, every, k, p, x0_dev, params_host, v_dev, s_dev,
                               js_dev);
  if (rc) return rc;
  DeviceGuard guard(s->device);
  int cls;
  if ((rc = tds_diff_prepare(s, &cls))) return rc;
  if ((rc = tds_param_check_sel(&s->model, p, params_host))) return rc;
  const TdsTrajArgs ta = tds_traj_args(&s->model, (const tds_model_t *)s->d_diff_model, n, steps, every,
                                       (const double *)x0_dev, (const double *)u_dev, p, (const double *)theta_dev, k,
                                       (const double *)v_dev, (double *)s_dev, (double *)js_dev);
  return tds_with_bound(cls, [&](auto b) { return tds_traj_dispatch<typename decltype(b)::type>(s, ta, params_host); });
}

int tds_hip_trajectory_jvp_host(const tds_model_t *model, int n, int steps, int every, const double *x0,
                                const double *u, int p, const tds_param_t *params, const double *theta, int k,
                                const double *v, double *s, double *js) {
  if (!model || !s) return fail(TDS_ERR_INVALID_ARG, "tds_hip_trajectory_jvp_host: NULL or empty argument%s");
  int rc = tds_traj_check_args("tds_hip_trajectory_jvp_host%s", n, steps, every, k, p, x0, params, v, s, js);
  if (rc) return rc;
  int cls;
  if ((rc = tds_param_host_prepare(model, p, params, &cls))) return rc;
  TdsTrajArgs ta = tds_traj_args(model, model, n, steps, every, x0, u, p, theta, k, v, s, js);
  ta.a.params = params;
  return tds_with_bound(cls, [&](auto b) { return tds_traj_host_impl<typename decltype(b)::type>(ta); });
}

}  // extern "C"
