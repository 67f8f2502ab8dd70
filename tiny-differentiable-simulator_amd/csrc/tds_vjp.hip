// tds_vjp.hip — step VJPs: reverse-mode adjoints of forward_zero (tds_diff_step.h over TdsRev, tds_rev.h) on gfx950,
// the C ABI tds_hip_vjp / tds_hip_vjp_host / tds_hip_vjp_host_tape (include/tds_hip.h).
//
// Mapping: one lane per environment.  A lane evaluates the step once over TdsRev, which records a tape of the
// operations with an active operand (the recording kernel), then sweeps that tape back once per cotangent (the sweep
// kernel): wj_j = w_j^T J.  The lane's work
// object (the record and the step's state in TdsRev form), its tape and its adjoints live in the handle's work buffer,
// not in the private segment.  Tape and adjoints are laid out [wavefront][position][lane]: the lanes of a wavefront
// record in step, and sweep the same positions together.  The environments go through in chunks of at most kVjpLanes,
// one pair of launches per chunk.  The tape capacity per lane is a bound per model class (TdsVjpCap); a lane that
// would exceed it stops recording, its environment's outputs are NaN and the call returns TDS_ERR_UNSUPPORTED.
// This is a path of its own: neither the step kernels nor the forward-mode kernel (tds_jvp.hip) change.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "tds_diff_classes.h"
#include "tds_rev.h"

using namespace tds_internal;

namespace {

// tape entries a lane may record, per class: the longest tape counted for the class's models (golden records, and
// every contact point active), plus 18 - 28 %
template <class B>
struct TdsVjpCap;
template <>
struct TdsVjpCap<TdsBoundS> { static constexpr int N = 16384; };
template <>
struct TdsVjpCap<TdsBoundA> { static constexpr int N = 81920; };
template <>
struct TdsVjpCap<TdsBoundL> { static constexpr int N = 73728; };

// lanes of one launch (a multiple of 64).  Ant x 4096: one pass, 4096 x (32 B per entry of the capacity + the work
// object) = 10.9 GB of work buffer
constexpr long long kVjpLanes = 4096;

// w [n][k][output_dim] -> wj [n][k][input_dim]; y [n][output_dim] optional
struct TdsVjpArgs {
  const tds_model_t *m;
  int n, k;
  const double *x, *w;
  double *y, *wj;
  int *overflow;  // set where a lane's tape overflows
};

// a lane's work object: the record and the step's state in TdsRev form
template <class B>
struct TdsVjpLane {
  TdsRev x[B::NX], y[B::NY];
  TdsDiffWork<TdsRev, B> w;
};

// record one environment's tape (the cursor of the calling lane counts its entries); 0 or the step's -1
template <class B>
TDS_HD inline int tds_vjp_record(const tds_model_t *m, TdsVjpLane<B> &L, const double *xe) {
  for (int i = 0; i < m->input_dim; ++i) L.x[i] = TdsRev(xe[i], i);
  tds_rev_cursor(tds_rev_lane()) = 0;
  return tds_diff_step(m, L.w, L.x, L.y);
}

// y (optional) of one recorded environment; `bad` (M not positive definite, or the tape overflowed): NaN, as are
// its k cotangents' wj
template <class B>
TDS_HD inline void tds_vjp_y(const tds_model_t *m, const TdsVjpLane<B> &L, bool bad, int k, double *ye, double *wje) {
  const int nout = m->output_dim, ny = tds_diff_ny(m);
  const double nan = __builtin_nan("");
  if (ye)
    for (int i = 0; i < nout; ++i) ye[i] = (i < ny ? L.y[i].v : 0.0) + (bad ? nan : 0.0);
  if (bad)
    for (int i = 0; i < k * m->input_dim; ++i) wje[i] = nan;
}

// The device's sweep.  The adjoint of a variable is split in two parts: contributions from entries less than kVjpRing
// positions later (the near part) go to a ring of kVjpRing slots per lane in LDS; the rest (the far part: inputs,
// seeds, long-range uses) go to the lane's adjoints in the work buffer as atomic adds, which the sweep does not wait
// for.  Entries, partials and far parts are loaded a block of kVjpBlock positions ahead of the block being swept:
// every far contribution to a loaded position comes from a position at least kVjpRing later, already swept.  A block
// is swept without data-dependent branches (positions outside the lane's tape contribute zeros), and both parts are
// accumulated by atomic adds without return (LDS; memory, only where some lane has a far contribution): the only wait
// per entry is the LDS read of its own adjoint.  The ring takes 128 KB of the CU's 160 KB of LDS.
constexpr int kVjpRing = 256, kVjpBlock = 8;
static_assert(kVjpRing >= 2 * kVjpBlock, "the far parts of the block loaded ahead are complete when it is loaded");
static_assert((kVjpRing & (kVjpRing - 1)) == 0, "ring slots are taken with a mask");

struct TdsVjpBlk {
  TdsRevIdx e[kVjpBlock];
  TdsRevPart d[kVjpBlock];
  double far[kVjpBlock];
};

// positions p0, p0 - 1, ..., p0 - kVjpBlock + 1 (those below 0 load position 0: they are not swept)
__device__ inline void tds_vjp_load(const TdsRevTape &t, int l, int p0, TdsVjpBlk &b) {
#pragma unroll
  for (int j = 0; j < kVjpBlock; ++j) {
    const long long p = max(p0 - j, 0);
    b.e[j] = t.ix[p * 64 + l];
    b.d[j] = t.pd[p * 64 + l];
    b.far[j] = __hip_atomic_load(t.adj + (t.n_in + p) * 64 + l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// c into the adjoint of v, from the entry whose result is r: the near part (LDS) or the far part (atomic add); the
// other part gets zero
__device__ inline void tds_vjp_add(const TdsRevTape &t, double *ring_l, int l, int v, int r, double c) {
  const bool near = v >= t.n_in && v > r - kVjpRing;
  // LDS atomic add without return: the sweep does not wait for it (LDS keeps a wavefront's operations in order)
  __hip_atomic_fetch_add(ring_l + (v & (kVjpRing - 1)) * 64, near ? c : 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  if (!near && c != 0.0) unsafeAtomicAdd(t.adj + (long long)v * 64 + l, c);  // skipped where no lane has one
}

// sweep positions p0 .. p0 - kVjpBlock + 1 of a lane whose tape has len entries
__device__ inline void tds_vjp_block(const TdsRevTape &t, double *ring_l, int l, int p0, int len, const TdsVjpBlk &b) {
#pragma unroll
  for (int j = 0; j < kVjpBlock; ++j) {
    const int p = p0 - j, r = t.n_in + p;
    const bool valid = p >= 0 && p < len;
    double *slot = ring_l + (r & (kVjpRing - 1)) * 64;
    const double g = *slot + b.far[j];
    *slot = 0.0;  // the slot's next variable, r - kVjpRing, gets its first near contribution after this
    // the far part back to zero for the next sweep (p < 0: no variable of the tape)
    if (p >= 0 && b.far[j] != 0.0)
      __hip_atomic_store(t.adj + (long long)r * 64 + l, 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool two = valid && b.e[j].b >= 0;
    tds_vjp_add(t, ring_l, l, valid ? b.e[j].a : 0, r, valid ? b.d[j].da * g : 0.0);
    tds_vjp_add(t, ring_l, l, two ? b.e[j].b : 0, r, two ? b.d[j].db * g : 0.0);
  }
}

// the sweep of one lane, from the wavefront's longest tape (top) down: the lanes of a wavefront walk the same positions
__device__ inline void tds_vjp_sweep(const TdsRevTape &t, double *ring_l, int l, int len, int top) {
  TdsVjpBlk A, B;
  tds_vjp_load(t, l, top - 1, A);
  for (int p0 = top - 1; p0 >= 0; p0 -= 2 * kVjpBlock) {
    tds_vjp_load(t, l, p0 - kVjpBlock, B);
    tds_vjp_block(t, ring_l, l, p0, len, A);
    tds_vjp_load(t, l, p0 - 2 * kVjpBlock, A);
    tds_vjp_block(t, ring_l, l, p0 - kVjpBlock, len, B);
  }
}

// Two kernels per chunk of at most kVjpLanes environments, one lane per environment, one wavefront per workgroup.
// The recording kernel evaluates the step over TdsRev (its register allocation is the step's); the sweep kernel reads
// the tapes back from the work buffer with a register budget of its own.
//
// recording: the lane's tape and y; lens[lane] = the tape's length, -1 where the environment's outputs are NaN
template <class B>
__global__ void __launch_bounds__(64) tds_vjp_record_kernel(TdsVjpArgs a, long long base, TdsVjpLane<B> *lanes,
                                                            int *lens, TdsRevIdx *ix, TdsRevPart *pd) {
  constexpr int cap = TdsVjpCap<B>::N;
  const int l = threadIdx.x;
  const long long wave = blockIdx.x, lane = wave * 64 + l, env = base + lane;
  const tds_model_t *m = a.m;
  const int nin = m->input_dim, nout = m->output_dim;
  if (l == 0) tds_rev_tape() = TdsRevTape{ix + wave * cap * 64, pd + wave * cap * 64, nullptr, 64, cap, nin};
  __syncthreads();
  if (env >= a.n) return;
  TdsVjpLane<B> &L = lanes[lane];
  const int rc = tds_vjp_record<B>(m, L, a.x + env * nin);
  const int len = tds_rev_cursor(l);
  const bool bad = rc != 0 || len > cap;
  if (len > cap) *a.overflow = 1;
  lens[lane] = bad ? -1 : len;
  tds_vjp_y<B>(m, L, bad, a.k, a.y ? a.y + env * nout : nullptr, a.wj + env * a.k * nin);
}

// the sweeps: per cotangent, the seeds, the sweep from the wavefront's longest tape down, wj
template <class B>
__global__ void __launch_bounds__(64) tds_vjp_sweep_kernel(TdsVjpArgs a, long long base, const TdsVjpLane<B> *lanes,
                                                           const int *lens, TdsRevIdx *ix, TdsRevPart *pd,
                                                           double *adj) {
  constexpr int cap = TdsVjpCap<B>::N;
  const int l = threadIdx.x;
  const long long wave = blockIdx.x, lane = wave * 64 + l, env = base + lane;
  const tds_model_t *m = a.m;
  const int nin = m->input_dim, nout = m->output_dim, ny = tds_diff_ny(m);
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
  const TdsVjpLane<B> &L = lanes[lane];
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
long long tds_vjp_lanes(int n) {
  const long long l = ((long long)n + 63) / 64 * 64;
  return l < kVjpLanes ? l : kVjpLanes;
}

size_t tds_vjp_align(size_t b) { return (b + 255) & ~(size_t)255; }

// work buffer: overflow flag | tape lengths | the lanes' work objects | tape indices | tape partials | adjoints
template <class B>
struct TdsVjpLayout {
  size_t lens, lanes, ix, pd, adj, total;
  TdsVjpLayout(long long n_lanes, int nin) {
    constexpr size_t cap = TdsVjpCap<B>::N;
    lens = 256;
    lanes = lens + tds_vjp_align(n_lanes * sizeof(int));
    ix = lanes + tds_vjp_align(n_lanes * sizeof(TdsVjpLane<B>));
    pd = ix + tds_vjp_align(n_lanes * cap * sizeof(TdsRevIdx));
    adj = pd + tds_vjp_align(n_lanes * cap * sizeof(TdsRevPart));
    total = adj + tds_vjp_align(n_lanes * (nin + cap) * sizeof(double));
  }
};

template <class B>
int tds_vjp_launch(tds_hip_sim *s, const TdsVjpArgs &a) {
  const long long n_lanes = tds_vjp_lanes(a.n);
  const TdsVjpLayout<B> lay(n_lanes, s->model.input_dim);
  int rc = tds_jvp_tmp(s, lay.total);
  if (rc) return rc;
  char *ws = (char *)s->d_diff_tmp;
  TdsVjpArgs b = a;
  b.overflow = (int *)ws;
  TDS_HIP_TRY(hipMemsetAsync(b.overflow, 0, sizeof(int), s->stream));
  TdsVjpLane<B> *lanes = (TdsVjpLane<B> *)(ws + lay.lanes);
  int *lens = (int *)(ws + lay.lens);
  TdsRevIdx *ix = (TdsRevIdx *)(ws + lay.ix);
  TdsRevPart *pd = (TdsRevPart *)(ws + lay.pd);
  const dim3 grid((unsigned)(n_lanes / 64));
  // the far parts start at zero; every sweep leaves those of its tape's variables at zero again (inputs: zeroed before
  // each sweep), so one fill serves all chunks of the call
  TDS_HIP_TRY(hipMemsetAsync(ws + lay.adj, 0, lay.total - lay.adj, s->stream));
  for (long long base = 0; base < a.n; base += n_lanes) {  // chunks of n_lanes environments
    hipLaunchKernelGGL((tds_vjp_record_kernel<B>), grid, dim3(64), 0, s->stream, b, base, lanes, lens, ix, pd);
    TDS_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL((tds_vjp_sweep_kernel<B>), grid, dim3(64), 0, s->stream, b, base, lanes, lens, ix, pd,
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

// the host instantiation over environments [0, n); tape_cap <= 0: the class's capacity; tape_len [n] (optional):
// entries each environment recorded, -1 where its tape overflowed
template <class B>
int tds_vjp_host_impl(const tds_model_t *m, int n, const double *x, int k, const double *w, double *y, double *wj,
                      int tape_cap, int *tape_len) {
  const int nin = m->input_dim, nout = m->output_dim, ny = tds_diff_ny(m);
  const int cap = tape_cap > 0 ? tape_cap : TdsVjpCap<B>::N;
  std::vector<TdsVjpLane<B>> L(1);
  std::vector<TdsRevIdx> ix(cap);
  std::vector<TdsRevPart> pd(cap);
  std::vector<double> adj((size_t)nin + cap);
  const TdsRevTape t = {ix.data(), pd.data(), adj.data(), 1, cap, nin};
  tds_rev_tape() = t;
  int bad = 0, over = 0;
  for (int e = 0; e < n; ++e) {
    const int rc = tds_vjp_record<B>(m, L[0], x + (size_t)e * nin);
    const int len = tds_rev_cursor(0);
    if (tape_len) tape_len[e] = len > cap ? -1 : len;
    bad |= rc != 0, over |= len > cap;
    double *wje = wj + (size_t)e * k * nin;
    tds_vjp_y<B>(m, L[0], rc != 0 || len > cap, k, y ? y + (size_t)e * nout : nullptr, wje);
    if (rc != 0 || len > cap) continue;
    for (int j = 0; j < k; ++j) {
      const double *wv = w + ((size_t)e * k + j) * nout;  // entries past ny are not outputs of the step
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

extern "C" {

int tds_hip_vjp(tds_hip_sim_t *s, int n, const void *x_dev, int k, const void *w_dev, void *y_dev, void *wj_dev) {
  if (!s || !x_dev || !w_dev || !wj_dev || n < 1 || k < 1) return fail(TDS_ERR_INVALID_ARG, "tds_hip_vjp: NULL or empty argument%s");
  DeviceGuard guard(s->device);
  int cls, rc = tds_jvp_prepare(s, &cls);
  if (rc) return rc;
  TdsVjpArgs a = {(const tds_model_t *)s->d_diff_model, n, k, (const double *)x_dev, (const double *)w_dev,
                  (double *)y_dev, (double *)wj_dev, nullptr};
  switch (cls) {
    case 0: return tds_vjp_launch<TdsBoundS>(s, a);
    case 1: return tds_vjp_launch<TdsBoundA>(s, a);
    default: return tds_vjp_launch<TdsBoundL>(s, a);
  }
}

int tds_hip_vjp_host_tape(const tds_model_t *model, int n, const double *x, int k, const double *w, double *y,
                          double *wj, int tape_cap, int *tape_len) {
  if (!model || !x || !w || !wj || n < 1 || k < 1) return fail(TDS_ERR_INVALID_ARG, "tds_hip_vjp_host: NULL or empty argument%s");
  const char *why = "";
  const int cls = tds_jvp_pick(model, &why);
  if (cls < 0) return fail(TDS_ERR_UNSUPPORTED, "%s", why);
  const int rc = tds_hip_model_check(model);  // indices of the blob in range (the handle's model passed it at creation)
  if (rc) return rc;
  switch (cls) {
    case 0: return tds_vjp_host_impl<TdsBoundS>(model, n, x, k, w, y, wj, tape_cap, tape_len);
    case 1: return tds_vjp_host_impl<TdsBoundA>(model, n, x, k, w, y, wj, tape_cap, tape_len);
    default: return tds_vjp_host_impl<TdsBoundL>(model, n, x, k, w, y, wj, tape_cap, tape_len);
  }
}

int tds_hip_vjp_host(const tds_model_t *model, int n, const double *x, int k, const double *w, double *y, double *wj) {
  return tds_hip_vjp_host_tape(model, n, x, k, w, y, wj, 0, nullptr);
}

}  // extern "C"
