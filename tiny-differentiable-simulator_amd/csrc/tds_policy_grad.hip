// tds_policy_grad.hip — the policy network between the steps of a closed-loop trajectory on gfx950, forward and
// backward (tds_hip_policy_trajectory_vjp, orchestrated in tds_traj_vjp.hip).  One wavefront per environment, the layout
// of tds_policy_mlp_kernel (tds_api.hip); the arithmetic is tds_policy.h's, which the host checker shares.
//
//   tds_policy_fwd_kernel  u_t = pi_W(obs_t): the observation comes from x0 or from the state store, the actions go to
//                          the action store (t = 0: the action slots of the x0 copy) and to the caller's u.
//   tds_policy_bwd_kernel  after step t's sweep: the layers recomputed with every activation and its derivative in LDS
//                          (2 x 8 x 256 doubles, plus two delta vectors: 36 KB), ubar_t read where the sweep scattered
//                          it, + ga_t, the layers walked down.  Weight and bias gradients are plain read-modify-writes
//                          into gpolicy[env]: an environment belongs to one wavefront.  The unmasked observation
//                          adjoint is added to lambda.
// Built without FP contraction (Makefile), as the other derivative units.
#include <hip/hip_runtime.h>

#include "tds_policy.h"

namespace {

__global__ void __launch_bounds__(64) tds_policy_fwd_kernel(TdsPolicyNet nn, TdsPolicyFwdArgs f) {
  __shared__ double a[kPolicyActs];
  const long long env = blockIdx.x;
  const int lane = threadIdx.x, P = nn.nw + nn.nb, nact = nn.units[nn.n - 1];
  tds_policy_forward(nn, f.policy + env * P, f.obs + env * f.obs_stride, f.raw, a, nullptr);
  const double *const out = a + (nn.n - 1) * TDS_NN_MAX_UNITS;
  for (int i = lane; i < nact; i += 64) {
    const double v = out[i];
    f.dst[env * f.dst_stride + i] = v;
    if (f.out) f.out[env * f.out_stride + i] = v;
  }
}

__global__ void __launch_bounds__(64) tds_policy_bwd_kernel(TdsPolicyNet nn, TdsPolicyBwdArgs b) {
  __shared__ double a[kPolicyActs], d[kPolicyActs], del[2][TDS_NN_MAX_UNITS];
  const long long env = b.e0 + (long long)blockIdx.x;
  if (b.bad[env]) return;  // (the whole wavefront)
  const int lane = threadIdx.x, P = nn.nw + nn.nb, nact = nn.units[nn.n - 1];
  const double *const W = b.policy + env * P;
  tds_policy_forward(nn, W, b.obs + env * b.obs_stride, b.raw, a, d);
  for (int i = lane; i < nact; i += 64) {
    double *const ub = b.ubar + env * b.ubar_stride + i;
    double g = *ub;
    if (b.ga) g += b.ga[env * b.ga_stride + i];
    if (b.zero_ubar) *ub = 0.0;
    del[0][i] = g;
  }
  __syncthreads();
  const double *const gobs = tds_policy_backward(nn, W, a, d, del[0], del[1], b.gpolicy + env * P);
  for (int o = lane; o < nn.units[0]; o += 64)
    if (o >= 2 || b.raw) b.lam[o * b.lam_entry + env * b.lam_env] += gobs[o];
}

__global__ void __launch_bounds__(256) tds_policy_nan_kernel(double *gpolicy, int P, const int *bad, const int *over,
                                                             long long n_items) {
  const long long it = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (it >= n_items) return;
  const long long env = it / P;
  if (bad[env] || over[env]) gpolicy[it] = __builtin_nan("");
}

}  // namespace

int tds_policy_fwd_launch(void *st, const TdsPolicyNet &nn, const TdsPolicyFwdArgs &f) {
  hipLaunchKernelGGL(tds_policy_fwd_kernel, dim3((unsigned)f.n), dim3(64), 0, (hipStream_t)st, nn, f);
  return (int)hipGetLastError();
}

int tds_policy_bwd_launch(void *st, const TdsPolicyNet &nn, const TdsPolicyBwdArgs &b) {
  hipLaunchKernelGGL(tds_policy_bwd_kernel, dim3((unsigned)b.count), dim3(64), 0, (hipStream_t)st, nn, b);
  return (int)hipGetLastError();
}

int tds_policy_nan_launch(void *st, double *gpolicy, int P, const int *bad, const int *over, int n) {
  const long long items = (long long)n * P;
  hipLaunchKernelGGL(tds_policy_nan_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)st,
                     gpolicy, P, bad, over, items);
  return (int)hipGetLastError();
}
