// tds_vjp_kernels.h — the reverse-mode machinery of the step VJPs (tds_vjp.hip: derivatives in x) and of the
// parameter derivatives (tds_dparam.hip: in [x | theta]), written once over the lane's work object: the kernel of the
// sweep (the sweep itself: tds_vjp_sweep.h), a recording kernel, the work buffer's layout, the launches per chunk of environments with the overflow flag,
// and the host instantiation.  The templates take a lane type `Lane`, which supplies:
//   Lane::cap                    tape entries a lane may record (the bound of its model class and mode);
//   Lane::n_extra(a)             active inputs after x (0, or the p parameters): variables input_dim .. + n_extra - 1;
//   lane.record(a, env)          seeds its inputs, sets the lane's cursor to 0 and runs the step over TdsRev (0, or
//                                the step's -1);
//   lane.y                       the step's outputs in TdsRev form;
// and the arguments `A` (TdsVjpArgs or a type derived from it).  The tape's variables 0 .. n_in - 1 are the inputs,
// n_in = input_dim + n_extra; wj is [n][k][n_in].
// tds_vjp.hip launches a recording kernel of its own through tds_vjp_run's `record` argument: instantiated for its
// plain lane, tds_vjp_record_lane_kernel allocates differently (AGPR 186 -> 194, private segment 1056 -> 1680 B, no
// LDS-promoted array: DESIGN 7a), and the plain path keeps its measured figures.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "tds_diff_classes.h"
#include "tds_vjp_sweep.h"

namespace {

using namespace tds_internal;

// lanes of one launch (a multiple of 64).  Ant x 4096: one pass, 4096 x (32 B per entry of the capacity + the work
// object) = 10.9 GB of work buffer
constexpr long long kVjpLanes = 4096;

// w [n][k][output_dim] -> wj [n][k][n_in]; y [n][output_dim] optional
struct TdsVjpArgs {
  const tds_model_t *m;
  int n, k;
  const double *x, *w;
  double *y, *wj;
  int *overflow;  // set where a lane's tape overflows
};

// y (optional) of one recorded environment; `bad` (M not positive definite, or the tape overflowed): NaN, as are
// its k cotangents' wj [k][n_in]
template <class Lane>
TDS_HD inline void tds_vjp_y(const tds_model_t *m, const Lane &L, int n_in, bool bad, int k, double *ye, double *wje) {
  const int nout = m->output_dim, ny = tds_diff_ny(m);
  const double nan = __builtin_nan("");
  if (ye)
    for (int i = 0; i < nout; ++i) ye[i] = (i < ny ? L.y[i].v : 0.0) + (bad ? nan : 0.0);
  if (bad)
    for (int i = 0; i < k * n_in; ++i) wje[i] = nan;
}

// Two kernels per chunk of at most kVjpLanes environments, one lane per environment, one wavefront per workgroup.
// The recording kernel evaluates the step over TdsRev (its register allocation is the step's); the sweep kernel reads
// the tapes back from the work buffer with a register budget of its own.
//
// recording: the lane's tape and y; lens[lane] = the tape's length, -1 where the environment's outputs are NaN
template <class Lane, class A>
__global__ void __launch_bounds__(64) tds_vjp_record_lane_kernel(A a, long long base, Lane *lanes, int *lens,
                                                                 TdsRevIdx *ix, TdsRevPart *pd) {
  constexpr int cap = Lane::cap;
  const int l = threadIdx.x;
  const long long wave = blockIdx.x, lane = wave * 64 + l, env = base + lane;
  const tds_model_t *m = a.m;
  const int nin = m->input_dim + Lane::n_extra(a), nout = m->output_dim;
  if (l == 0) tds_rev_tape() = TdsRevTape{ix + wave * cap * 64, pd + wave * cap * 64, nullptr, 64, cap, nin};
  __syncthreads();
  if (env >= a.n) return;
  Lane &L = lanes[lane];
  const int rc = L.record(a, env);
  const int len = tds_rev_cursor(l);
  const bool bad = rc != 0 || len > cap;
  if (len > cap) *a.overflow = 1;
  lens[lane] = bad ? -1 : len;
  tds_vjp_y(m, L, nin, bad, a.k, a.y ? a.y + env * nout : nullptr, a.wj + env * a.k * nin);
}

// the sweeps: per cotangent, the seeds, the sweep from the wavefront's longest tape down, wj
template <class Lane, class A>
__global__ void __launch_bounds__(64) tds_vjp_sweep_kernel(A a, long long base, const Lane *lanes, const int *lens,
                                                           TdsRevIdx *ix, TdsRevPart *pd, double *adj) {
  constexpr int cap = Lane::cap;
  const int l = threadIdx.x;
  const long long wave = blockIdx.x, lane = wave * 64 + l, env = base + lane;
  const tds_model_t *m = a.m;
  const int nin = m->input_dim + Lane::n_extra(a), nout = m->output_dim, ny = tds_diff_ny(m);
  __shared__ double ring[kVjpRing * 64];  // the near parts of the adjoints, [slot][lane]
  __shared__ int top_s;                   // the wavefront's longest tape: its lanes sweep the same positions together
  const int len = env < a.n ? lens[lane] : -1;
  if (l == 0) top_s = 0;
  __syncthreads();
  if (len > 0) atomicMax(&top_s, len);
  __syncthreads();
  const int top = top_s;
  if (len < 0) return;  // outside [0, n), or NaN outputs written by the recording kernel
  const TdsRevTape t = {ix + wave * cap * 64, pd + wave * cap * 64, adj + wave * (nin + cap) * 64, 64, cap, nin};
  const Lane &L = lanes[lane];
  double *adj_l = t.adj + l, *ring_l = ring + l, *wje = a.wj + env * a.k * nin;
  for (int j = 0; j < a.k; ++j) {
    const double *wv = a.w + (env * a.k + j) * nout;  // entries past ny are not outputs of the step
    for (int s = 0; s < kVjpRing; ++s) ring_l[s * 64] = 0.0;
    for (int i = 0; i < nin; ++i) adj_l[(long long)i * 64] = 0.0;
    for (int i = 0; i < ny; ++i)
      if (L.y[i].i >= 0) unsafeAtomicAdd(adj_l + (long long)L.y[i].i * 64, wv[i]);
    tds_vjp_sweep(t, ring_l, l, len, top);
    for (int i = 0; i < nin; ++i)
      wje[(size_t)j * nin + i] = __hip_atomic_load(adj_l + (long long)i * 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// lanes of a launch over n environments
inline long long tds_vjp_lanes(int n) {
  const long long l = ((long long)n + 63) / 64 * 64;
  return l < kVjpLanes ? l : kVjpLanes;
}

// work buffer: overflow flag | tape lengths | the lanes' work objects | tape indices | tape partials | adjoints
// (`extra` bytes after the overflow flag's slot, before the lengths: what the caller keeps there, e.g. a selection)
template <class Lane>
struct TdsVjpLayout {
  size_t lens, lanes, ix, pd, adj, total;
  TdsVjpLayout(long long n_lanes, int nin, size_t extra = 0) {
    constexpr size_t cap = Lane::cap;
    lens = 256 + tds_vjp_align(extra);
    lanes = lens + tds_vjp_align(n_lanes * sizeof(int));
    ix = lanes + tds_vjp_align(n_lanes * sizeof(Lane));
    pd = ix + tds_vjp_align(n_lanes * cap * sizeof(TdsRevIdx));
    adj = pd + tds_vjp_align(n_lanes * cap * sizeof(TdsRevPart));
    total = adj + tds_vjp_align(n_lanes * (nin + cap) * sizeof(double));
  }
};

// launches tds_vjp_record_lane_kernel (tds_vjp_run's default recording launch)
struct TdsVjpRecordLane {
  template <class Lane, class A>
  void operator()(hipStream_t st, dim3 grid, const A &b, long long base, Lane *lanes, int *lens, TdsRevIdx *ix,
                  TdsRevPart *pd) const {
    hipLaunchKernelGGL((tds_vjp_record_lane_kernel<Lane, A>), grid, dim3(64), 0, st, b, base, lanes, lens, ix, pd);
  }
};

// the launches of a call over a.n environments with n_in inputs; the work buffer already holds lay.total bytes.
// record(stream, grid, args, base, lanes, lens, ix, pd) launches a chunk's recording kernel.
template <class Lane, class A, class Record = TdsVjpRecordLane>
int tds_vjp_run(tds_hip_sim *s, const A &a, const TdsVjpLayout<Lane> &lay, long long n_lanes, Record record = {}) {
  char *ws = (char *)s->d_diff_tmp;
  A b = a;
  b.overflow = (int *)ws;
  TDS_HIP_TRY(hipMemsetAsync(b.overflow, 0, sizeof(int), s->stream));
  Lane *lanes = (Lane *)(ws + lay.lanes);
  int *lens = (int *)(ws + lay.lens);
  TdsRevIdx *ix = (TdsRevIdx *)(ws + lay.ix);
  TdsRevPart *pd = (TdsRevPart *)(ws + lay.pd);
  const dim3 grid((unsigned)(n_lanes / 64));
  // the far parts start at zero; every sweep leaves those of its tape's variables at zero again (inputs: zeroed before
  // each sweep), so one fill serves all chunks of the call
  TDS_HIP_TRY(hipMemsetAsync(ws + lay.adj, 0, lay.total - lay.adj, s->stream));
  for (long long base = 0; base < a.n; base += n_lanes) {  // chunks of n_lanes environments
    record(s->stream, grid, b, base, lanes, lens, ix, pd);
    TDS_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((tds_vjp_sweep_kernel<Lane, A>), grid, dim3(64), 0, s->stream, b, base, lanes, lens, ix, pd,
                       (double *)(ws + lay.adj));
    TDS_HIP_TRY(hipGetLastError());
  }
  int overflow = 0;  // the call reports an overflow: it waits for its launches
  TDS_HIP_TRY(hipMemcpyAsync(&overflow, b.overflow, sizeof(int), hipMemcpyDeviceToHost, s->stream));
  TDS_HIP_TRY(hipStreamSynchronize(s->stream));
  if (overflow)
    return fail(TDS_ERR_UNSUPPORTED, "step VJPs: an environment's tape exceeds the capacity of its model class%s");
  return TDS_OK;
}

// the host instantiation over environments [0, a.n) (a holds host pointers); tape_cap <= 0: the lane's capacity;
// tape_len [n] (optional): entries each environment recorded, -1 where its tape overflowed
template <class Lane, class A>
int tds_vjp_host_run(const A &a, int tape_cap, int *tape_len) {
  const tds_model_t *m = a.m;
  const int nin = m->input_dim + Lane::n_extra(a), nout = m->output_dim, ny = tds_diff_ny(m), n = a.n, k = a.k;
  const int cap = tape_cap > 0 ? tape_cap : Lane::cap;
  std::vector<Lane> L(1);
  std::vector<TdsRevIdx> ix(cap);
  std::vector<TdsRevPart> pd(cap);
  std::vector<double> adj((size_t)nin + cap);
  const TdsRevTape t = {ix.data(), pd.data(), adj.data(), 1, cap, nin};
  tds_rev_tape() = t;
  int bad = 0, over = 0;
  for (int e = 0; e < n; ++e) {
    const int rc = L[0].record(a, e);
    const int len = tds_rev_cursor(0);
    if (tape_len) tape_len[e] = len > cap ? -1 : len;
    bad |= rc != 0, over |= len > cap;
    double *wje = a.wj + (size_t)e * k * nin;
    tds_vjp_y(m, L[0], nin, rc != 0 || len > cap, k, a.y ? a.y + (size_t)e * nout : nullptr, wje);
    if (rc != 0 || len > cap) continue;
    for (int j = 0; j < k; ++j) {
      const double *wv = a.w + ((size_t)e * k + j) * nout;  // entries past ny are not outputs of the step
      std::fill(adj.begin(), adj.begin() + nin + len, 0.0);
      for (int i = 0; i < ny; ++i)
        if (L[0].y[i].i >= 0) adj[L[0].y[i].i] += wv[i];
      tds_rev_sweep_host(t, len);
      std::copy(adj.begin(), adj.begin() + nin, wje + (size_t)j * nin);
    }
  }
  tds_rev_tape() = TdsRevTape{};
  if (over) return fail(TDS_ERR_UNSUPPORTED, "step VJPs: an environment's tape exceeds the capacity%s");
  if (bad) return fail(TDS_ERR_INVALID_ARG, "step VJPs: joint-space inertia not positive definite%s");
  return TDS_OK;
}

}  // namespace
