// tds_rollout_vjp.h — what the reverse-mode rollout derivatives share: the trajectory VJP and its closed-loop form
// (tds_traj_vjp.hip) and the rigid-body rollout VJP (tds_rb_vjp.hip).  All three run a primal pass into a state store
// and then, per chunk of environments and per window of W consecutive steps, last window first:
//   recording   the W steps' tapes side by side (a record depends on the primal alone): the unit's own kernel;
//   chained     one wavefront per block of 64 environments walks t from the window's last step down to its first:
//   sweep       zero the ring and the input parts, seed lambda (+ gs at a recorded step), tds_vjp_sweep on tape
//               (t, block), scatter the input adjoints.  lambda [ns][n] lives in the work buffer and so crosses window
//               boundaries.  A sweep leaves every far part it read at zero (tds_vjp_block) and the input parts are
//               zeroed before each sweep, so the one adjoint region of a sweeping wavefront serves all W tapes, and one
//               fill of the adjoints serves all windows and chunks.
// An environment belongs to one lane and t descends, so what a scatter accumulates is a plain read-modify-write.  Only
// copies and lambda cross window and chunk boundaries: the results do not depend on W or the chunk size.
//
// A unit describes its rollout by a problem type P:
//   P::shape()                          TdsRolloutShape: the environments and what the seed reads;
//   P::live(env)                        device: does the environment take part (inside [0, n), primal finite);
//   P::scatter(env, t, adj, as, lam, ls)  the input adjoints of step t's sweep: the state part into lambda (t = 0: into
//                                       the gradient), the rest where the unit accumulates it; entry i at [i * stride].
// The header depends on tds_vjp_sweep.h alone.  The host pieces return hipError_t: the caller reports it its own way.
#pragma once
#include <algorithm>
#include <type_traits>

#include "tds_vjp_sweep.h"

namespace {

struct TdsRolloutShape {
  int n, ns, every, n_rec;  // environments, state entries, a record every `every` steps, steps / every
  const double *gs;         // [n][n_rec][ns]
};

// c into an adjoint's far part / its value (device: as tds_vjp_sweep_kernel seeds and reads them)
TDS_HD inline void tds_rollout_vjp_add(double *p, double c) {
#if defined(__HIP_DEVICE_COMPILE__)
  unsafeAtomicAdd(p, c);
#else
  *p += c;
#endif
}
TDS_HD inline double tds_rollout_vjp_load(const double *p) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  return *p;
#endif
}

// seeds of step t's sweep: adj[y_i] += lambda_i (+ gs_i where step t is recorded), i < ns.  yi: the variable indices
// of the step's ns state outputs, lam: lambda, adj: the lane's adjoints; entry i at [i * stride]
TDS_HD inline void tds_rollout_vjp_seed(const TdsRolloutShape &sh, int env, int t, const int *yi, long long ys,
                                        const double *lam, long long ls, double *adj, long long as) {
  const bool rec = (t + 1) % sh.every == 0;
  const double *g = sh.gs + ((size_t)env * sh.n_rec + (rec ? (t + 1) / sh.every - 1 : 0)) * sh.ns;
  for (int i = 0; i < sh.ns; ++i) {
    const int v = yi[i * ys];
    if (v < 0) continue;  // a constant
    double c = lam[i * ls];
    if (rec) c += g[i];
    tds_rollout_vjp_add(adj + v * as, c);
  }
}

// s [n][n_rec][ns] out of the state store [n][steps][ns]: one lane per (environment, record)
__device__ __forceinline__ void tds_rollout_vjp_select(const double *store, double *s, long long n_items, int steps,
                                                       int every, int n_rec, int ns) {
  const long long it = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (it >= n_items) return;
  const long long env = it / n_rec, r = it % n_rec;
  const double *src = store + (env * steps + (r + 1) * every - 1) * ns;
  double *dst = s + it * ns;
  for (int i = 0; i < ns; ++i) dst[i] = src[i];
}

// the chained sweep of steps t1 - 1 .. t0 for environments e0 + 64 blockIdx.x ..: the tapes of step t at wavefront
// (t - t0) nblk + blockIdx.x of lens, yidx [wavefront][ns][lane], ix and pd (capacity cap, nin inputs)
template <class P>
__device__ __forceinline__ void tds_rollout_vjp_sweep(const P &pr, int e0, int nblk, int t0, int t1, int cap, int nin,
                                                      const int *lens, const int *yidx, TdsRevIdx *ix, TdsRevPart *pd,
                                                      double *adj, double *lam) {
  const TdsRolloutShape sh = pr.shape();
  const int l = threadIdx.x;
  const long long blk = blockIdx.x, env = e0 + blk * 64 + l;
  __shared__ double ring[kVjpRing * 64];  // the near parts of the adjoints, [slot][lane]
  __shared__ int top_s;                   // the wavefront's longest tape of the step
  const bool live = pr.live(env);
  double *adj_w = adj + blk * (long long)(nin + cap) * 64;  // (a variable's index is an int: so is nin + cap)
  double *adj_l = adj_w + l, *ring_l = ring + l, *lam_l = lam + env;
  for (int t = t1 - 1; t >= t0; --t) {
    const long long wave = (long long)(t - t0) * nblk + blk;
    const int len_t = live ? lens[wave * 64 + l] : -1;
    const int len = len_t > 0 ? len_t : 0;  // a lane without a tape sweeps nothing
    __syncthreads();
    if (l == 0) top_s = 0;
    __syncthreads();
    if (len > 0) atomicMax(&top_s, len);
    __syncthreads();
    const int top = top_s;
    const TdsRevTape tp = {ix + wave * cap * 64, pd + wave * cap * 64, adj_w, 64, cap, nin};
    for (int s = 0; s < kVjpRing; ++s) ring_l[s * 64] = 0.0;
    for (int i = 0; i < nin; ++i) adj_l[(long long)i * 64] = 0.0;
    if (len_t >= 0) tds_rollout_vjp_seed(sh, (int)env, t, yidx + wave * sh.ns * 64 + l, 64, lam_l, sh.n, adj_l, 64);
    tds_vjp_sweep(tp, ring_l, l, len, top);
    if (len_t >= 0) pr.scatter((int)env, t, adj_l, 64, lam_l, sh.n);  // (a lane with a tape: env < n)
  }
}

// the host checkers' sweep of step t of one environment, its tape (len entries) recorded last
template <class P>
inline void tds_rollout_vjp_host_step(const P &pr, const TdsRevTape &tp, int len, int env, int t, const int *yi,
                                      double *lam) {
  std::fill(tp.adj, tp.adj + tp.n_in + len, 0.0);
  tds_rollout_vjp_seed(pr.shape(), env, t, yi, 1, lam, 1, tp.adj, 1);
  tds_rev_sweep_host(tp, len);
  pr.scatter(env, t, tp.adj, 1, lam, 1);
}

struct TdsRolloutNoHook {};

#define TDS_ROLLOUT_TRY(expr) \
  if (const hipError_t e_ = (expr); e_ != hipSuccess) return e_

// The backward launches of n environments over `steps` steps in chunks of `chunk` environments (whole wavefronts) and
// windows of W steps, after the one fill of the adjoints (adj_bytes at adj).
//   record(e0, nblk, t0, t1)       launches the recording of steps [t0, t1) of the nblk blocks from environment e0;
//   sweep(e0, nblk, t0, t1, w0)    launches their chained sweep; the tapes begin w0 wavefronts into the window's;
//   after(e0, nblk, t)             optional, follows the sweep of step t: the sweeps then go one step per launch.
// Each returns hipError_t.
template <class Record, class Sweep, class After = TdsRolloutNoHook>
hipError_t tds_rollout_vjp_backward(hipStream_t st, int n, int steps, long long chunk, int W, void *adj,
                                    size_t adj_bytes, Record record, Sweep sweep, After after = {}) {
  TDS_ROLLOUT_TRY(hipMemsetAsync(adj, 0, adj_bytes, st));
  const int n_win = (steps + W - 1) / W, max_blk = (int)(chunk / 64);
  for (long long e0 = 0; e0 < n; e0 += chunk) {
    const long long left = ((long long)n - e0 + 63) / 64;
    const int nblk = left < max_blk ? (int)left : max_blk;
    for (int w = n_win - 1; w >= 0; --w) {
      const int t0 = w * W, t1 = t0 + W < steps ? t0 + W : steps;
      TDS_ROLLOUT_TRY(record(e0, nblk, t0, t1));
      if constexpr (std::is_same_v<After, TdsRolloutNoHook>) {
        TDS_ROLLOUT_TRY(sweep(e0, nblk, t0, t1, 0LL));
      } else {
        for (int t = t1 - 1; t >= t0; --t) {
          TDS_ROLLOUT_TRY(sweep(e0, nblk, t, t + 1, (long long)(t - t0) * nblk));
          TDS_ROLLOUT_TRY(after(e0, nblk, t));
        }
      }
    }
  }
  return hipSuccess;
}

// the call reports an overflow: it reads the flag back and waits for its launches
inline hipError_t tds_rollout_vjp_overflow(hipStream_t st, const int *flag_dev, int *overflow) {
  TDS_ROLLOUT_TRY(hipMemcpyAsync(overflow, flag_dev, sizeof(int), hipMemcpyDeviceToHost, st));
  return hipStreamSynchronize(st);
}

#undef TDS_ROLLOUT_TRY

}  // namespace
