// tds_rb_diff.hip — forward-mode derivatives of rigid-body world rollouts (tds_rb_jvp, tds_rb_jvp_host,
// tds_rb_params_get).
//
// jv = (d s_T / d [s0 | theta]) v: `steps` World::steps from s0, differentiated through tds_rb_world_steps
// (tds_rb_step.h, the statement tds_rb_step runs) over TdsDual<K>.  The derivative is that of the algorithm as executed:
// contact activation, the nrv / impulse tests, the friction clamp and the latn test follow the primal's branch;
// quaternion entries are raw, their tangents pass through integrate's normalisation.
//
// Mapping: one lane per (world, block of RB_JVP_K directions), one wavefront per workgroup; each lane recomputes the
// primal.  Values live in LDS as tds_rb_kernel keeps them, [component][lane], with two more components per body (mass
// and inverse mass, active where selected).  The tangents live in the handle's work buffer as
// [body * RB_NCD + comp][k][item], item minor: a wave-uniform access to body b is one coalesced 512 B run per tangent.
// Neither lives in the private segment.  This TU is built with -ffp-contract=off: the device evaluates the template
// with the host's roundings, so device and host results can be compared to round-off of the compared quantity, not of
// the differing contractions amplified by 300 steps of collisions.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "tds_rb_diff.h"

#ifndef RB_JVP_K
#define RB_JVP_K 2  // directions per lane (kernel-resource-usage table in DESIGN §7a)
#endif
#define RB_CHUNK 262144   // items per launch (tangent buffer <= 16 bodies * 15 * K * 8 B * RB_CHUNK)

namespace {

// s_T [nb * 13] (where sTw) and the tangents of directions d0.. into jvw [k][nb * 13]
template <int K, typename W>
__host__ __device__ __forceinline__ void rb_store(const W &w, int nb, double *sTw, double *jvw, int k, int d0) {
  for (int b = 0; b < nb; ++b) {
    for (int c = 0; c < RB_NC; ++c) {
      const int h = b * TDS_RB_STATE + rb_hbm(c);
      const auto x = w.get(b, c);
      if (sTw) sTw[h] = tds_value(x);
      if constexpr (K > 0) {
#pragma unroll
        for (int kk = 0; kk < K; ++kk)
          if (d0 + kk < k) jvw[(size_t)(d0 + kk) * nb * TDS_RB_STATE + h] = x.d[kk];
      }
    }
  }
}

// items item0 .. item0 + gridDim.x * 64 - 1 of n * ceil(k / K) (K = 0: n), item = block * n + world
template <int K>
__global__ __launch_bounds__(64) void tds_rb_jvp_kernel(const RbDev<double> *__restrict__ Mp, int n, int steps,
                                                        const double *__restrict__ s0, RbSel sel,
                                                        const double *__restrict__ theta, int k,
                                                        const double *__restrict__ v, double *__restrict__ sT,
                                                        double *__restrict__ jv, double *__restrict__ tan,
                                                        long long item0, long long items) {
  const RbDev<double> &M = *Mp;
  extern __shared__ __align__(16) unsigned char rb_smem_raw[];
  const int lane = threadIdx.x;
  const long long local = (long long)blockIdx.x * 64 + lane;
  const long long item = item0 + local;
  const bool valid = item < items;
  const long long it = valid ? item : 0;  // a padding lane runs item 0 and writes nothing
  const int world = (int)(it % n), d0 = (int)(it / n) * K;
  RbDevWorld<K> w;
  w.sm = reinterpret_cast<double *>(rb_smem_raw);
  w.lane = lane;
  w.stride = (size_t)gridDim.x * 64;
  w.tan = tan + local;
  const int nb = M.nb, ns = nb * TDS_RB_STATE;
  rb_load<K>(w, M, s0 + (size_t)world * ns, sel, theta ? theta + (size_t)world * sel.p : nullptr,
             K ? v + (size_t)world * k * (ns + sel.p) : nullptr, k, d0);
  tds_rb_world_steps<typename RbScalar<K>::type>(M, w, steps);
  if (valid)
    rb_store<K>(w, nb, sT && d0 == 0 ? sT + (size_t)world * ns : nullptr, K ? jv + (size_t)world * k * ns : nullptr,
                k, d0);
}

int rb_check_call(int n, int steps, const void *s0, int k, const void *v, const void *sT, const void *jv) {
  if (n < 1) return tds_rb_fail(TDS_ERR_INVALID_ARG, "n < 1");
  if (steps < 1) return tds_rb_fail(TDS_ERR_INVALID_ARG, "steps < 1");
  if (k < 0) return tds_rb_fail(TDS_ERR_INVALID_ARG, "k < 0");
  if (!s0) return tds_rb_fail(TDS_ERR_INVALID_ARG, "s0 is NULL");
  if (k == 0 && !sT) return tds_rb_fail(TDS_ERR_INVALID_ARG, "k = 0 and sT is NULL: nothing to compute");
  if (k > 0 && (!v || !jv)) return tds_rb_fail(TDS_ERR_INVALID_ARG, "k > 0 needs v and jv");
  return TDS_OK;
}

template <int K>
int rb_launch(tds_rb_sim *s, int n, int steps, const double *s0, const RbSel &sel, const double *theta, int k,
              const double *v, double *sT, double *jv) {
  const long long items = K == 0 ? (long long)n : (long long)n * ((k + K - 1) / K);
  const int nb = s->model.num_bodies;
  const size_t lds = (size_t)nb * RB_NCD * 64 * sizeof(double);
  const long long per = items < RB_CHUNK ? (items + 63) / 64 * 64 : RB_CHUNK;  // lanes of one launch
  const size_t need = K == 0 ? 0 : (size_t)nb * RB_NCD * K * per * sizeof(double);
  if (const int rc = rb_work_buffer(s, need, "tangent buffer")) return rc;
  if (hipFuncSetAttribute((const void *)tds_rb_jvp_kernel<K>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) !=
      hipSuccess)
    return tds_rb_fail(TDS_ERR_HIP, "hipFuncSetAttribute (dynamic LDS) failed");
  for (long long i0 = 0; i0 < items; i0 += per) {
    const long long cnt = items - i0 < per ? items - i0 : per;
    hipLaunchKernelGGL(tds_rb_jvp_kernel<K>, dim3((unsigned)((cnt + 63) / 64)), dim3(64), lds, s->stream,
                       (const RbDev<double> *)s->d_model, n, steps, s0, sel, theta, k, v, sT, jv,
                       (double *)s->d_work, i0, items);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
      char msg[160];
      snprintf(msg, sizeof(msg), "tds_rb_jvp_kernel launch failed: %s", hipGetErrorString(e));
      return tds_rb_fail(TDS_ERR_HIP, msg);
    }
  }
  return TDS_OK;
}

template <int K>
void rb_host_world(const RbDev<double> &M, int steps, const double *s0w, const RbSel &sel, const double *thw,
                   const double *vw, int k, int d0, double *sTw, double *jvw) {
  RbHostWorld<typename RbScalar<K>::type> w;
  rb_load<K>(w, M, s0w, sel, thw, vw, k, d0);
  tds_rb_world_steps<typename RbScalar<K>::type>(M, w, steps);
  rb_store<K>(w, M.nb, sTw, jvw, k, d0);
}

}  // namespace

extern "C" {

int tds_rb_params_get(const tds_rb_model_t *model, int p, const tds_param_t *params, double *theta) {
  if (!model || (p > 0 && !theta)) return tds_rb_fail(TDS_ERR_INVALID_ARG, "NULL argument");
  int rc = rb_model_check(model);
  if (rc != TDS_OK) return rc;
  RbSel sel;
  if ((rc = rb_check_sel(model, p, params, &sel)) != TDS_OK) return rc;
  for (int j = 0; j < p; ++j) {
    const int kind = sel.kind[j], q = sel.idx[j];
    theta[j] = kind == TDS_PARAM_LINK_MASS  ? model->bodies[q].mass
               : kind == TDS_PARAM_GRAVITY  ? model->gravity[q]
               : kind == TDS_PARAM_FRICTION ? model->friction
                                            : model->restitution;
  }
  return TDS_OK;
}

int tds_rb_jvp(tds_rb_sim_t *s, int n, int steps, const void *s0_dev, int p, const tds_param_t *params_host,
               const void *theta_dev, int k, const void *v_dev, void *sT_dev, void *jv_dev) {
  if (!s) return tds_rb_fail(TDS_ERR_INVALID_ARG, "sim is NULL");
  if (s->dtype != TDS_DTYPE_F64)
    return tds_rb_fail(TDS_ERR_UNSUPPORTED, "tds_rb_jvp supports f64 handles only (this handle is f32)");
  int rc = rb_check_call(n, steps, s0_dev, k, v_dev, sT_dev, jv_dev);
  if (rc != TDS_OK) return rc;
  RbSel sel;
  if ((rc = rb_check_sel(&s->model, p, params_host, &sel)) != TDS_OK) return rc;
  if (hipSetDevice(s->device) != hipSuccess) return tds_rb_fail(TDS_ERR_HIP, "hipSetDevice failed");
  const double *s0 = (const double *)s0_dev, *th = (const double *)theta_dev, *v = (const double *)v_dev;
  double *sT = (double *)sT_dev, *jv = (double *)jv_dev;
  if (k == 0) return rb_launch<0>(s, n, steps, s0, sel, th, 0, nullptr, sT, nullptr);
  return rb_launch<RB_JVP_K>(s, n, steps, s0, sel, th, k, v, sT, jv);
}

int tds_rb_jvp_host(const tds_rb_model_t *model, int n, int steps, const double *s0, int p, const tds_param_t *params,
                    const double *theta, int k, const double *v, double *sT, double *jv) {
  if (!model) return tds_rb_fail(TDS_ERR_INVALID_ARG, "model is NULL");
  int rc = rb_model_check(model);
  if (rc != TDS_OK) return rc;
  if ((rc = rb_check_call(n, steps, s0, k, v, sT, jv)) != TDS_OK) return rc;
  RbSel sel;
  if ((rc = rb_check_sel(model, p, params, &sel)) != TDS_OK) return rc;
  std::vector<RbDev<double>> Mv(1);
  rb_build<double>(model, Mv.data());
  const RbDev<double> &M = Mv[0];
  const int ns = model->num_bodies * TDS_RB_STATE;
  for (int w = 0; w < n; ++w) {
    const double *s0w = s0 + (size_t)w * ns, *thw = theta ? theta + (size_t)w * p : nullptr;
    double *sTw = sT ? sT + (size_t)w * ns : nullptr;
    if (k == 0) {
      rb_host_world<0>(M, steps, s0w, sel, thw, nullptr, 0, 0, sTw, nullptr);
      continue;
    }
    for (int d0 = 0; d0 < k; d0 += RB_JVP_K)
      rb_host_world<RB_JVP_K>(M, steps, s0w, sel, thw, v + (size_t)w * k * (ns + p), k, d0, d0 == 0 ? sTw : nullptr,
                              jv + (size_t)w * k * ns);
  }
  return TDS_OK;
}

}  // extern "C"
