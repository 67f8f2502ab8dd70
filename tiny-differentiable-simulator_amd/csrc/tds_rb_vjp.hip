// tds_rb_vjp.hip — reverse-mode derivatives of rigid-body world rollouts on gfx950 (tds_rb_vjp, tds_rb_vjp_host,
// tds_rb_vjp_plan).
//
// The rollout of tds_rb_jvp (`steps` World::steps from s0, tds_rb_world_steps of tds_rb_step.h), the states after every
// `every`-th step recorded, one cotangent gs on the recorded states, and its gradients in s0 and in theta.  The
// derivative is that of the algorithm as executed, as in forward mode: every test of the step reads values only.
//
// The form is that of tds_rollout_vjp.h, which holds the chained sweep, its seed and the launch loop over chunks and
// windows; this unit supplies the kernels that are its own:
//   primal      one lane per world, the double instantiation with the values in LDS [component][lane] as
//               tds_rb_jvp_kernel<0> keeps them; the state after every step goes into a state store [n][steps][nb * 13]
//               in the work buffer, s is copied out of it.
//   then, per chunk of worlds and per window of W consecutive steps, last window first:
//   recording   one lane per (step t of the window, world): the state entering step t from the store seeds variables
//               0 .. nb * 13 - 1, theta variables nb * 13 .. nb * 13 + p - 1 (active where selected; inv_mass = 1 / theta
//               is the tape's first entry), then tds_rb_world_steps<TdsRev>(M, w, 1).  A collision sphere that ends
//               without an impulse leaves no entries (rb_tape_mark / rb_tape_rewind).  The values stay in LDS; the
//               variable indices live in the work buffer [component][lane], lane minor (one coalesced 256 B run per
//               wave-uniform access), as tds_rb_jvp keeps its tangents.  Tape layout [wavefront][position][lane].
//   chained     tds_rollout_vjp_sweep over RbVjpProblem: every world inside [0, n) is live; the scatter's state part
//   sweep       is the next lambda (t = 0: gs0), its theta part accumulates into gtheta.  lambda [nb * 13][n] lives in
//               the work buffer.
//   NaN pass    NaN gradients for the worlds one of whose steps overflowed its tape.
// Only copies and lambda cross window and chunk boundaries, and chunks are whole wavefronts: the results do not depend
// on W or the chunk.  The unit is built without FP contraction (Makefile), as tds_rb_diff.hip: device and host round
// alike.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "tds_rb_diff.h"
#include "tds_rollout_vjp.h"

// found by argument-dependent lookup where tds_rb_world_steps<TdsRev> is instantiated
__host__ __device__ __forceinline__ TdsRev rb_sqrt(const TdsRev &x) { return tds_sqrt(x); }
// the tape hooks of tds_rb_step.h: a collision sphere that ends without an impulse leaves no entries.  (A lane that
// overflowed inside such a stretch is back below the capacity; one that overflowed before it stays at cap + 1.)
__host__ __device__ __forceinline__ int rb_tape_mark(const TdsRev *) { return tds_rev_cursor(tds_rev_lane()); }
__host__ __device__ __forceinline__ void rb_tape_rewind(const TdsRev *, int mark) {
  tds_rev_cursor(tds_rev_lane()) = mark;
}

namespace {

// the default bound of the work buffer: 8 GiB.  The billiard scene x 4096 worlds x 300 steps needs 0.9 GB of state
// store and, at a capacity of 16 384 entries (its longest step records 11 765), 2.1 GB per step of all worlds side by
// side: 8 GiB keeps such a call in one pass with windows of three steps ("Rigid-body rollouts, reverse
// mode")
constexpr size_t kRbVjpBudget = (size_t)8 << 30;
// entries of one narrowphase + solve of one collision sphere (counted on tds_rb_step.h: 83 + 215, rounded up) and of
// one body's gravity impulse + integrate (12 + 47)
constexpr long long kRbVjpContact = 320, kRbVjpBody = 64;

struct RbVjpArgs {
  int n, nb, ns, p, steps, every, n_rec;
  const double *s0, *theta, *gs;  // [n][ns], [n][p] or NULL, [n][n_rec][ns]
  const double *store;            // the state after step t at [n][steps][ns]
  double *gs0, *gtheta;           // [n][ns] or NULL, [n][p] or NULL
  int *overflow;                  // set where a lane's tape overflows
};

// the state entering step t of world w
__host__ __device__ inline const double *rb_vjp_state(const RbVjpArgs &a, long long w, int t) {
  return t > 0 ? a.store + ((size_t)w * a.steps + (t - 1)) * a.ns : a.s0 + (size_t)w * a.ns;
}

// step t of world w over TdsRev on the world behind acc: variable h = entry h of the state in HBM order, ns + j =
// theta_j.  Leaves the lane's cursor at the tape's length (cap + 1: overflowed)
template <typename W>
__host__ __device__ __forceinline__ void rb_vjp_record(const RbVjpArgs &a, const RbDev<double> &M, const RbSel &sel,
                                                       W &acc, long long w, int t) {
  tds_rev_cursor(tds_rev_lane()) = 0;
  rb_load_seeded<TdsRev>(acc, M, rb_vjp_state(a, w, t), sel, a.theta ? a.theta + (size_t)w * a.p : nullptr,
                         [](double x, int col) { return TdsRev(x, col); });
  tds_rb_world_steps<TdsRev>(M, acc, 1);
}

// the rollout as tds_rollout_vjp.h sees it: every world inside [0, n) is live
struct RbVjpProblem {
  const RbVjpArgs &a;
  __host__ __device__ TdsRolloutShape shape() const { return {a.n, a.ns, a.every, a.n_rec, a.gs}; }
  __device__ bool live(long long w) const { return w < a.n; }
  // the input adjoints of step t's sweep: the state part is the next lambda (t = 0: gs0), theta's is added to gtheta
  __host__ __device__ void scatter(int w, int t, const double *adj, long long as, double *lam, long long ls) const {
    if (t > 0) {
      for (int h = 0; h < a.ns; ++h) lam[h * ls] = tds_rollout_vjp_load(adj + h * as);
    } else if (a.gs0) {
      for (int h = 0; h < a.ns; ++h) a.gs0[(size_t)w * a.ns + h] = tds_rollout_vjp_load(adj + h * as);
    }
    if (a.gtheta)
      for (int j = 0; j < a.p; ++j) a.gtheta[(size_t)w * a.p + j] += tds_rollout_vjp_load(adj + (a.ns + j) * as);
  }
};

__host__ __device__ inline void rb_vjp_nan(const RbVjpArgs &a, long long w) {
  const double nan = __builtin_nan("");
  if (a.gs0)
    for (int h = 0; h < a.ns; ++h) a.gs0[(size_t)w * a.ns + h] = nan;
  if (a.gtheta)
    for (int j = 0; j < a.p; ++j) a.gtheta[(size_t)w * a.p + j] = nan;
}

// ---------------------------------------------------------------- the primal
// worlds 64 blockIdx.x ..: every step's state into the store (a padding lane runs world 0 and writes nothing)
__global__ __launch_bounds__(64) void tds_rb_vjp_primal_kernel(const RbDev<double> *__restrict__ Mp, RbVjpArgs a,
                                                               RbSel sel, double *__restrict__ store) {
  const RbDev<double> &M = *Mp;
  extern __shared__ __align__(16) unsigned char rb_smem_raw[];
  const int lane = threadIdx.x;
  const long long world = (long long)blockIdx.x * 64 + lane;
  const bool valid = world < a.n;
  const long long wl = valid ? world : 0;
  RbDevWorld<0> w;
  w.sm = reinterpret_cast<double *>(rb_smem_raw);
  w.lane = lane;
  w.stride = 0;
  w.tan = nullptr;
  rb_load_seeded<double>(w, M, a.s0 + (size_t)wl * a.ns, sel, a.theta ? a.theta + (size_t)wl * a.p : nullptr,
                         [](double x, int) { return x; });
  for (int t = 0; t < a.steps; ++t) {
    tds_rb_world_steps<double>(M, w, 1);
    if (!valid) continue;
    double *dst = store + ((size_t)wl * a.steps + t) * a.ns;
    for (int b = 0; b < a.nb; ++b)
      for (int c = 0; c < RB_NC; ++c) dst[b * TDS_RB_STATE + rb_hbm(c)] = w.get(b, c);
  }
}

// s [n][n_rec][ns] out of the store [n][steps][ns]: one lane per (world, record)
__global__ __launch_bounds__(256) void tds_rb_vjp_select_kernel(const double *__restrict__ store,
                                                                double *__restrict__ s, long long n_items, int steps,
                                                                int every, int n_rec, int ns) {
  tds_rollout_vjp_select(store, s, n_items, steps, every, n_rec, ns);
}

// ---------------------------------------------------------------- recording
// world of a recording lane: values in LDS [(b * RB_NCD + c) * 64 + lane], variable indices at vi[(b * RB_NCD + c) *
// stride] (vi already offset by the lane)
struct RbRevDevWorld : RbGlobals<TdsRev> {
  double *sm;
  int lane;
  int *vi;
  size_t stride;
  __device__ __forceinline__ TdsRev get(int b, int c) const {
    const int s = b * RB_NCD + c;
    return TdsRev(sm[s * 64 + lane], vi[(size_t)s * stride]);
  }
  __device__ __forceinline__ void put(int b, int c, const TdsRev &x) {
    const int s = b * RB_NCD + c;
    sm[s * 64 + lane] = x.v;
    vi[(size_t)s * stride] = x.i;
  }
  __device__ __forceinline__ TdsRev mass(int b) const { return get(b, RB_MASS); }
  __device__ __forceinline__ TdsRev inv_mass(int b) const { return get(b, RB_INV_MASS); }
  __device__ __forceinline__ TdsRev grav(int k) const { return this->g[k]; }
  __device__ __forceinline__ TdsRev restitution() const { return this->rs; }
  __device__ __forceinline__ TdsRev friction() const { return this->fr; }
};

// wavefront blockIdx.x = (step t0 + blockIdx.x / nblk, worlds e0 + 64 (blockIdx.x % nblk) ..): the lane's tape, lens
// [lane] = its length (-1: overflowed, or no world) and yidx [wavefront][ns][lane] = the variables of the step's outputs
__global__ __launch_bounds__(64) void tds_rb_vjp_record_kernel(const RbDev<double> *__restrict__ Mp, RbVjpArgs a,
                                                               RbSel sel, int e0, int nblk, int t0, int cap, int *over,
                                                               int *lens, int *yidx, int *vi, TdsRevIdx *ix,
                                                               TdsRevPart *pd) {
  const RbDev<double> &M = *Mp;
  extern __shared__ __align__(16) unsigned char rb_smem_raw[];
  const int l = threadIdx.x;
  const long long wave = blockIdx.x, lane = wave * 64 + l;
  const int t = t0 + (int)(wave / nblk);
  const long long world = e0 + (wave % nblk) * 64 + l;
  if (l == 0)
    tds_rev_tape() = TdsRevTape{ix + wave * cap * 64, pd + wave * cap * 64, nullptr, 64, cap, a.ns + a.p};
  __syncthreads();
  if (world >= a.n) {
    lens[lane] = -1;
    return;
  }
  RbRevDevWorld w;
  w.sm = reinterpret_cast<double *>(rb_smem_raw);
  w.lane = l;
  w.stride = (size_t)gridDim.x * 64;
  w.vi = vi + lane;
  rb_vjp_record(a, M, sel, w, world, t);
  const int len = tds_rev_cursor(l);
  if (len > cap) *a.overflow = 1, over[world] = 1;
  lens[lane] = len > cap ? -1 : len;
  for (int b = 0; b < a.nb; ++b)
    for (int c = 0; c < RB_NC; ++c)
      yidx[(wave * a.ns + b * TDS_RB_STATE + rb_hbm(c)) * 64 + l] = w.vi[(size_t)(b * RB_NCD + c) * w.stride];
}

// ---------------------------------------------------------------- chained sweep
// steps t1 - 1 .. t0 of worlds e0 + 64 blockIdx.x ..: lambda [ns][n] between them
__global__ __launch_bounds__(64) void tds_rb_vjp_sweep_kernel(RbVjpArgs a, int e0, int nblk, int t0, int t1, int cap,
                                                              const int *lens, const int *yidx, TdsRevIdx *ix,
                                                              TdsRevPart *pd, double *adj, double *lam) {
  tds_rollout_vjp_sweep(RbVjpProblem{a}, e0, nblk, t0, t1, cap, a.ns + a.p, lens, yidx, ix, pd, adj, lam);
}

// the last pass: NaN gradients where a step's tape overflowed
__global__ __launch_bounds__(256) void tds_rb_vjp_nan_kernel(RbVjpArgs a, const int *over) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w < a.n && over[w]) rb_vjp_nan(a, w);
}

// ---------------------------------------------------------------- plan and layout
// entries that hold any step of the model: every collision sphere of every pair the dispatcher accepts in contact in
// every iteration, plus gravity and integrate per body and the selected masses' inverses
int rb_vjp_cap_bound(const tds_rb_model_t *m, int p) {
  long long spheres = 0;
  auto ns_of = [](int t) { return t == TDS_GEOM_SPHERE ? 1 : t == TDS_GEOM_CAPSULE ? 2 : t == TDS_GEOM_BOX ? 8 : 0; };
  for (int i = 0; i < m->num_bodies; ++i)
    for (int j = i + 1; j < m->num_bodies; ++j) {
      const int ti = m->bodies[i].geom_type, tj = m->bodies[j].geom_type;
      if (ti == TDS_GEOM_PLANE && tj != TDS_GEOM_PLANE) spheres += ns_of(tj);
      else if (tj == TDS_GEOM_PLANE && ti != TDS_GEOM_PLANE) spheres += ns_of(ti);
      else if ((ti == TDS_GEOM_SPHERE || ti == TDS_GEOM_CAPSULE) && tj == TDS_GEOM_SPHERE) spheres += ns_of(ti);
      else if (ti == TDS_GEOM_SPHERE && tj == TDS_GEOM_CAPSULE) spheres += ns_of(tj);
    }
  const long long b = spheres * m->solver_iterations * kRbVjpContact + m->num_bodies * kRbVjpBody + p;
  return b > (1 << 30) ? 1 << 30 : (int)b;
}

// the work buffer: overflow flag | state store | over | lambda | lengths | output variables | variable indices | tape
// indices | tape partials | adjoints, for windows of W steps of `chunk` worlds
struct RbVjpLayout {
  size_t store, over, lam, lens, yidx, vi, ix, pd, adj, total;
  RbVjpLayout(int n, int steps, int nb, int p, size_t cap, size_t chunk, size_t W) {
    const size_t ns = (size_t)nb * TDS_RB_STATE, rec = W * chunk;
    store = 256;
    over = store + tds_vjp_align((size_t)n * steps * ns * sizeof(double));
    lam = over + tds_vjp_align((size_t)n * sizeof(int));
    lens = lam + tds_vjp_align((size_t)n * ns * sizeof(double));
    yidx = lens + tds_vjp_align(rec * sizeof(int));
    vi = yidx + tds_vjp_align(rec * ns * sizeof(int));
    ix = vi + tds_vjp_align(rec * nb * RB_NCD * sizeof(int));
    pd = ix + tds_vjp_align(rec * cap * sizeof(TdsRevIdx));
    adj = pd + tds_vjp_align(rec * cap * sizeof(TdsRevPart));
    total = adj + tds_vjp_align(chunk * (ns + p + cap) * sizeof(double));
  }
};

struct RbVjpPlan {
  int cap, W;
  long long chunk;
  size_t total;
};

// capacity, worlds per pass and steps per window of a call within work_bytes (0: the default bound)
int rb_vjp_plan(const tds_rb_model_t *m, int n, int steps, int p, int tape_cap, size_t work_bytes, RbVjpPlan *pl) {
  const int nb = m->num_bodies;
  const size_t budget = work_bytes ? work_bytes : kRbVjpBudget;
  auto total = [&](size_t cap, size_t chunk, size_t W) { return RbVjpLayout(n, steps, nb, p, cap, chunk, W).total; };
  int cap = tape_cap > 0 ? tape_cap : rb_vjp_cap_bound(m, p);
  if (tape_cap <= 0 && total(cap, 64, 1) > budget) {
    // the default capacity is capped by the budget: what one step of 64 worlds leaves room for
    const size_t fixed = total(0, 64, 1) + 3 * 256, per = 64 * (sizeof(TdsRevIdx) + sizeof(TdsRevPart) + sizeof(double));
    cap = budget > fixed + per ? (int)std::min<size_t>((budget - fixed) / per, (size_t)cap) : 0;
  }
  if (cap < 1 || total(cap, 64, 1) > budget) {
    char msg[200];
    snprintf(msg, sizeof(msg), "tds_rb_vjp: work_bytes %zu is too small: one step of 64 worlds needs %zu B", budget,
             total(tape_cap > 0 ? tape_cap : rb_vjp_cap_bound(m, p), 64, 1));
    return tds_rb_fail(TDS_ERR_INVALID_ARG, msg);
  }
  // the largest chunk (whole wavefronts), then the longest window, that fit: the layout grows with both
  long long lo = 1, hi = ((long long)n + 63) / 64;
  while (lo < hi) {
    const long long mid = (lo + hi + 1) / 2;
    if (total(cap, mid * 64, 1) <= budget) lo = mid;
    else hi = mid - 1;
  }
  const long long chunk = lo * 64;
  lo = 1, hi = steps;
  while (lo < hi) {
    const long long mid = (lo + hi + 1) / 2;
    if (total(cap, chunk, mid) <= budget) lo = mid;
    else hi = mid - 1;
  }
  pl->cap = cap, pl->chunk = chunk, pl->W = (int)lo, pl->total = total(cap, chunk, lo);
  return TDS_OK;
}

int rb_vjp_check_call(const char *fn, int n, int steps, int every, const void *s0, const void *gs) {
  char msg[96];
  const char *why = !s0 || !gs || n < 1 ? ": NULL or empty argument"
                    : steps < 1         ? ": steps must be at least 1"
                    : every < 1 || steps % every ? ": every must divide steps"
                                                 : nullptr;
  if (!why) return TDS_OK;
  snprintf(msg, sizeof(msg), "%s%s", fn, why);
  return tds_rb_fail(TDS_ERR_INVALID_ARG, msg);
}

RbVjpArgs rb_vjp_args(int nb, int n, int steps, int every, const double *s0, int p, const double *theta,
                      const double *gs, double *gs0, double *gtheta) {
  RbVjpArgs a;
  a.n = n, a.nb = nb, a.ns = nb * TDS_RB_STATE, a.p = p, a.steps = steps, a.every = every, a.n_rec = steps / every;
  a.s0 = s0, a.theta = theta, a.gs = gs, a.store = nullptr;
  a.gs0 = gs0, a.gtheta = p > 0 ? gtheta : nullptr, a.overflow = nullptr;
  return a;
}

#define RB_VJP_TRY(expr)                                                            \
  do {                                                                              \
    const hipError_t e_ = (expr);                                                   \
    if (e_ != hipSuccess) {                                                         \
      char msg_[200];                                                               \
      snprintf(msg_, sizeof(msg_), "tds_rb_vjp: %s: %s", #expr, hipGetErrorString(e_)); \
      return tds_rb_fail(TDS_ERR_HIP, msg_);                                        \
    }                                                                               \
  } while (0)

int rb_vjp_run(tds_rb_sim *s, RbVjpArgs a, const RbSel &sel, const RbVjpPlan &pl, double *s_out) {
  const int n = a.n, steps = a.steps, nb = a.nb, ns = a.ns, cap = pl.cap;
  const RbVjpLayout lay(n, steps, nb, a.p, cap, pl.chunk, pl.W);
  if (const int rc = rb_work_buffer(s, lay.total, "reverse-mode work buffer")) return rc;
  char *ws = (char *)s->d_work;
  double *store = (double *)(ws + lay.store), *lam = (double *)(ws + lay.lam);
  int *over = (int *)(ws + lay.over);
  a.overflow = (int *)ws;
  a.store = store;
  hipStream_t st = s->stream;
  const RbDev<double> *Mp = (const RbDev<double> *)s->d_model;
  const size_t lds = (size_t)nb * RB_NCD * 64 * sizeof(double);
  RB_VJP_TRY(hipFuncSetAttribute((const void *)tds_rb_vjp_primal_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)lds));
  RB_VJP_TRY(hipFuncSetAttribute((const void *)tds_rb_vjp_record_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)lds));
  RB_VJP_TRY(hipMemsetAsync(a.overflow, 0, sizeof(int), st));
  // over and lambda (they lie side by side) start at zero; so does the accumulated gtheta
  RB_VJP_TRY(hipMemsetAsync(over, 0, lay.lens - lay.over, st));
  if (a.gtheta) RB_VJP_TRY(hipMemsetAsync(a.gtheta, 0, (size_t)n * a.p * sizeof(double), st));

  hipLaunchKernelGGL(tds_rb_vjp_primal_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), lds, st, Mp, a, sel, store);
  RB_VJP_TRY(hipGetLastError());
  if (s_out) {
    const long long items = (long long)n * a.n_rec;
    hipLaunchKernelGGL(tds_rb_vjp_select_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, store, s_out,
                       items, steps, a.every, a.n_rec, ns);
    RB_VJP_TRY(hipGetLastError());
  }

  int *lens = (int *)(ws + lay.lens), *yidx = (int *)(ws + lay.yidx), *vi = (int *)(ws + lay.vi);
  TdsRevIdx *ix = (TdsRevIdx *)(ws + lay.ix);
  TdsRevPart *pd = (TdsRevPart *)(ws + lay.pd);
  double *adj = (double *)(ws + lay.adj);
  auto record = [&](long long e0, int nblk, int t0, int t1) {
    hipLaunchKernelGGL(tds_rb_vjp_record_kernel, dim3((unsigned)((t1 - t0) * nblk)), dim3(64), lds, st, Mp, a, sel,
                       (int)e0, nblk, t0, cap, over, lens, yidx, vi, ix, pd);
    return hipGetLastError();
  };
  auto sweep = [&](long long e0, int nblk, int t0, int t1, long long) {
    hipLaunchKernelGGL(tds_rb_vjp_sweep_kernel, dim3((unsigned)nblk), dim3(64), 0, st, a, (int)e0, nblk, t0, t1, cap,
                       lens, yidx, ix, pd, adj, lam);
    return hipGetLastError();
  };
  RB_VJP_TRY(tds_rollout_vjp_backward(st, n, steps, pl.chunk, pl.W, adj, lay.total - lay.adj, record, sweep));
  hipLaunchKernelGGL(tds_rb_vjp_nan_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, over);
  RB_VJP_TRY(hipGetLastError());
  int overflow = 0;
  RB_VJP_TRY(tds_rollout_vjp_overflow(st, a.overflow, &overflow));
  if (overflow)
    return tds_rb_fail(TDS_ERR_UNSUPPORTED, "tds_rb_vjp: a world's tape exceeds the capacity (tape_cap) of one step");
  return TDS_OK;
}

// the host instantiation: per world the primal into a store, then one tape at a time, t descending
int rb_vjp_host_run(const RbDev<double> &M, RbVjpArgs a, const RbSel &sel, int cap, double *s_out) {
  const int n = a.n, steps = a.steps, nb = a.nb, ns = a.ns, nin = ns + a.p;
  std::vector<double> store((size_t)steps * ns), lam(ns), adj((size_t)nin + cap), s0c(ns);
  std::vector<TdsRevIdx> ix(cap);
  std::vector<TdsRevPart> pd(cap);
  std::vector<int> yi(ns);
  std::vector<RbHostWorld<double>> wd(1);
  std::vector<RbHostWorld<TdsRev>> wr(1);
  const TdsRevTape tp = {ix.data(), pd.data(), adj.data(), 1, cap, nin};
  tds_rev_tape() = tp;
  int over = 0;
  for (int e = 0; e < n; ++e) {
    // this world alone, as world 0 of a one-world call
    RbVjpArgs b = a;
    b.n = 1;
    b.s0 = a.s0 + (size_t)e * ns, b.theta = a.theta ? a.theta + (size_t)e * a.p : nullptr;
    b.gs = a.gs + (size_t)e * a.n_rec * ns, b.store = store.data();
    b.gs0 = a.gs0 ? a.gs0 + (size_t)e * ns : nullptr, b.gtheta = a.gtheta ? a.gtheta + (size_t)e * a.p : nullptr;
    rb_load_seeded<double>(wd[0], M, b.s0, sel, b.theta, [](double x, int) { return x; });
    for (int t = 0; t < steps; ++t) {
      tds_rb_world_steps<double>(M, wd[0], 1);
      for (int bd = 0; bd < nb; ++bd)
        for (int c = 0; c < RB_NC; ++c) store[(size_t)t * ns + bd * TDS_RB_STATE + rb_hbm(c)] = wd[0].get(bd, c);
    }
    if (s_out)
      for (int r = 0; r < a.n_rec; ++r)
        std::copy_n(&store[((size_t)(r + 1) * a.every - 1) * ns], ns, s_out + ((size_t)e * a.n_rec + r) * ns);
    if (b.gtheta) std::fill_n(b.gtheta, a.p, 0.0);
    std::fill(lam.begin(), lam.end(), 0.0);
    int over_e = 0;
    for (int t = steps - 1; t >= 0 && !over_e; --t) {
      rb_vjp_record(b, M, sel, wr[0], 0, t);
      const int len = tds_rev_cursor(0);
      if (len > cap) {
        over_e = 1;
        break;
      }
      for (int bd = 0; bd < nb; ++bd)
        for (int c = 0; c < RB_NC; ++c) yi[bd * TDS_RB_STATE + rb_hbm(c)] = wr[0].get(bd, c).i;
      tds_rollout_vjp_host_step(RbVjpProblem{b}, tp, len, 0, t, yi.data(), lam.data());
    }
    if (over_e) rb_vjp_nan(b, 0);
    over |= over_e;
  }
  tds_rev_tape() = TdsRevTape{};
  if (over)
    return tds_rb_fail(TDS_ERR_UNSUPPORTED, "tds_rb_vjp_host: a world's tape exceeds the capacity (tape_cap) of one step");
  return TDS_OK;
}

}  // namespace

extern "C" {

int tds_rb_vjp_plan(const tds_rb_model_t *model, int n, int steps, int p, int tape_cap, size_t work_bytes,
                    long long *plan) {
  if (!model || !plan) return tds_rb_fail(TDS_ERR_INVALID_ARG, "tds_rb_vjp_plan: NULL or empty argument");
  int rc = rb_model_check(model);
  if (rc != TDS_OK) return rc;
  if (n < 1 || steps < 1 || p < 0 || p > RB_MAX_SEL || tape_cap < 0)
    return tds_rb_fail(TDS_ERR_INVALID_ARG, "tds_rb_vjp_plan: NULL or empty argument");
  RbVjpPlan pl;
  if ((rc = rb_vjp_plan(model, n, steps, p, tape_cap, work_bytes, &pl)) != TDS_OK) return rc;
  plan[0] = pl.cap, plan[1] = pl.chunk, plan[2] = pl.W, plan[3] = (long long)pl.total;
  return TDS_OK;
}

int tds_rb_vjp(tds_rb_sim_t *s, int n, int steps, int every, const void *s0_dev, int p,
               const tds_param_t *params_host, const void *theta_dev, const void *gs_dev, void *s_dev, void *gs0_dev,
               void *gtheta_dev, int tape_cap, size_t work_bytes) {
  if (!s) return tds_rb_fail(TDS_ERR_INVALID_ARG, "sim is NULL");
  if (s->dtype != TDS_DTYPE_F64)
    return tds_rb_fail(TDS_ERR_UNSUPPORTED, "tds_rb_vjp supports f64 handles only (this handle is f32)");
  int rc = rb_vjp_check_call("tds_rb_vjp", n, steps, every, s0_dev, gs_dev);
  if (rc != TDS_OK) return rc;
  if (tape_cap < 0) return tds_rb_fail(TDS_ERR_INVALID_ARG, "tape_cap < 0");
  RbSel sel;
  if ((rc = rb_check_sel(&s->model, p, params_host, &sel)) != TDS_OK) return rc;
  RbVjpPlan pl;
  if ((rc = rb_vjp_plan(&s->model, n, steps, p, tape_cap, work_bytes, &pl)) != TDS_OK) return rc;
  if (hipSetDevice(s->device) != hipSuccess) return tds_rb_fail(TDS_ERR_HIP, "hipSetDevice failed");
  const RbVjpArgs a = rb_vjp_args(s->model.num_bodies, n, steps, every, (const double *)s0_dev, p,
                                  (const double *)theta_dev, (const double *)gs_dev, (double *)gs0_dev,
                                  (double *)gtheta_dev);
  return rb_vjp_run(s, a, sel, pl, (double *)s_dev);
}

int tds_rb_vjp_host(const tds_rb_model_t *model, int n, int steps, int every, const double *s0, int p,
                    const tds_param_t *params, const double *theta, const double *gs, double *s, double *gs0,
                    double *gtheta, int tape_cap) {
  if (!model) return tds_rb_fail(TDS_ERR_INVALID_ARG, "model is NULL");
  int rc = rb_model_check(model);
  if (rc != TDS_OK) return rc;
  if ((rc = rb_vjp_check_call("tds_rb_vjp_host", n, steps, every, s0, gs)) != TDS_OK) return rc;
  if (tape_cap < 0) return tds_rb_fail(TDS_ERR_INVALID_ARG, "tape_cap < 0");
  RbSel sel;
  if ((rc = rb_check_sel(model, p, params, &sel)) != TDS_OK) return rc;
  std::vector<RbDev<double>> Mv(1);
  rb_build<double>(model, Mv.data());
  const RbVjpArgs a = rb_vjp_args(model->num_bodies, n, steps, every, s0, p, theta, gs, gs0, gtheta);
  return rb_vjp_host_run(Mv[0], a, sel, tape_cap > 0 ? tape_cap : rb_vjp_cap_bound(model, p), s);
}

}  // extern "C"
