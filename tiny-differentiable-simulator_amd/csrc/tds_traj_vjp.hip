// tds_traj_vjp.hip — reverse-mode derivatives of articulated-body trajectories on gfx950: the trajectory of
// tds_traj.hip (forward_zero chained over `steps` steps, states recorded every `every` steps), one cotangent gs on the
// recorded states, and its gradients in x0, in the actions u of steps 1 .. and in theta.  C ABI
// tds_hip_trajectory_vjp / tds_hip_trajectory_vjp_host (include/tds_hip.h).  The closed-loop form, every step's action
// taken from a policy network and the gradient in its parameters (tds_hip_policy_trajectory_vjp / _host), runs
// over the same kernels with the policy kernels of tds_policy_grad.hip between them.
//
// Phase 1, the primal: the double item of tds_traj.hip (tds_traj_advance<B, 0>, every = 1) writes the state after every
// step into a state store [n][steps][nsd] in the work buffer; s is copied out of it.
// Phase 2, backward, is the form of tds_rollout_vjp.h, which holds the chained sweep, its seed and the launch loop over
// chunks and windows; this unit supplies what is its own:
//   recording   one wavefront per (step t of the window, block of 64 environments): the lane builds step t's record
//               from the state store (tds_traj_vjp_record) and records it over TdsRev through the parameter-mode lane
//               of tds_dparam.hip; tape layout [wavefront][position][lane], as tds_vjp_kernels.h's;
//   chained     tds_rollout_vjp_sweep over TdsTrajVjpProblem: an environment is live where its primal was finite; the
//   sweep       scatter writes the next lambda and gu and accumulates into gx0 and gtheta.
// A last pass writes NaN gradients for the environments whose primal was NaN or whose tape overflowed.
// There is one device run and one host run: the open loop is the closed loop without a policy (the primal in launches
// of traj_steps steps, one sweep launch per window, nothing between the sweeps).
//
// The unit is built without FP contraction (Makefile), as tds_traj.hip: device and host round alike.
#include <hip/hip_runtime.h>
#include <string.h>

#include "tds_policy.h"
#include "tds_rollout_vjp.h"
#include "tds_traj.h"
#include "tds_vjp_param.h"

namespace {

// lanes of one recording launch where TDS_OPT_TRAJ_VJP_LANES is unset: the work-buffer bound of tds_hip_vjp
constexpr long long kTrajVjpLanesDefault = kVjpLanes, kTrajVjpLanesMax = 16384;

struct TdsTrajVjpArgs {
  const tds_model_t *m;
  int n, p, steps, every, n_rec, nsd, nact;
  const double *x0, *u, *theta, *gs;  // [n][input_dim], [n][steps - 1][nact] or NULL, [n][p] or NULL, [n][n_rec][nsd]
  const tds_param_t *params;
  const double *store;                // the state after step t at [n][steps][nsd]
  double *gx0, *gu, *gtheta;          // [n][input_dim], [n][steps - 1][nact], [n][p]
  int *overflow;                      // set where a lane's tape overflows
};

// step t's record of environment env as the primal read it, in TdsRev form: x variables 0 .. input_dim - 1, theta
// input_dim .. input_dim + p - 1 (theta NULL: the blob's values, still active).  0, or the step's -1
template <class B>
TDS_HD inline int tds_traj_vjp_record(const TdsTrajVjpArgs &a, TdsVjpParamLane<B> &L, int env, int t) {
  const tds_model_t *m = a.m;
  const int nin = m->input_dim, nsd = a.nsd;
  const double *xe = a.x0 + (size_t)env * nin;
  const double *st = t > 0 ? a.store + ((size_t)env * a.steps + (t - 1)) * nsd : xe;
  const double *ut = t > 0 && a.u ? a.u + ((size_t)env * (a.steps - 1) + (t - 1)) * a.nact : xe + nsd;
  for (int i = 0; i < nin; ++i) L.x[i] = TdsRev(i < nsd ? st[i] : i < nsd + a.nact ? ut[i - nsd] : xe[i], i);
  tds_param_seed(m, L.P);
  for (int j = 0; j < a.p; ++j) {
    const double th = a.theta ? a.theta[(size_t)env * a.p + j] : tds_param_slot(L.P, a.params[j], 0)->v;
    tds_param_set(L.P, a.params[j], TdsRev(th, nin + j));
  }
  tds_rev_cursor(tds_rev_lane()) = 0;
  return tds_diff_step_view(m, TdsOverlayView<TdsRev, B>{&L.P}, L.w, L.x, L.y);
}

// the trajectory as tds_rollout_vjp.h sees it (bad: device only)
struct TdsTrajVjpProblem {
  const TdsTrajVjpArgs &a;
  const int *bad;
  TDS_HD TdsRolloutShape shape() const { return {a.n, a.nsd, a.every, a.n_rec, a.gs}; }
  __device__ bool live(long long env) const { return env < a.n && !bad[env < a.n ? env : 0]; }
  // the input adjoints of step t's sweep: the state part is the next lambda (t = 0: gx0's state part); the action part
  // is gu[t - 1] (t = 0, or u NULL: added to gx0's action slots); gains and theta are added to gx0 and gtheta
  TDS_HD void scatter(int env, int t, const double *adj, long long as, double *lam, long long ls) const {
    const int nin = a.m->input_dim, nsd = a.nsd, nact = a.nact;
    double *gx = a.gx0 + (size_t)env * nin;
    for (int i = 0; i < nsd; ++i) {
      const double g = tds_rollout_vjp_load(adj + i * as);
      if (t > 0) lam[i * ls] = g;
      else gx[i] = g;
    }
    if (t > 0 && a.u) {
      double *gut = a.gu + ((size_t)env * (a.steps - 1) + (t - 1)) * nact;
      for (int i = 0; i < nact; ++i) gut[i] = tds_rollout_vjp_load(adj + (nsd + i) * as);
    } else {
      for (int i = nsd; i < nsd + nact; ++i) gx[i] += tds_rollout_vjp_load(adj + i * as);
    }
    for (int i = nsd + nact; i < nin; ++i) gx[i] += tds_rollout_vjp_load(adj + i * as);
    double *gt = a.gtheta + (size_t)env * a.p;
    for (int j = 0; j < a.p; ++j) gt[j] += tds_rollout_vjp_load(adj + (nin + j) * as);
  }
};

// NaN into every gradient of environment env
TDS_HD inline void tds_traj_vjp_nan(const TdsTrajVjpArgs &a, int env) {
  const double nan = __builtin_nan("");
  const int nin = a.m->input_dim;
  for (int i = 0; i < nin; ++i) a.gx0[(size_t)env * nin + i] = nan;
  if (a.u)
    for (long long i = 0; i < (long long)(a.steps - 1) * a.nact; ++i)
      a.gu[(size_t)env * (a.steps - 1) * a.nact + i] = nan;
  for (int j = 0; j < a.p; ++j) a.gtheta[(size_t)env * a.p + j] = nan;
}

// ---------------------------------------------------------------- phase 1
// steps t0 .. t1 of every environment into the state store (ta.s, every = 1); bad[env] once the last step is done
template <class B>
__global__ void __launch_bounds__(64) tds_traj_vjp_primal_kernel(TdsTrajArgs ta, TdsTrajLane<B, 0> *lanes,
                                                                 long long n_lanes, int t0, int t1, int *bad) {
  const long long lane = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= n_lanes) return;
  for (long long it = lane; it < ta.items; it += n_lanes) {
    const int b = tds_traj_advance<B, 0>(ta, lanes[lane], it, t0, t1);
    if (t1 == ta.steps) bad[it] = b;
  }
}

// s [n][n_rec][nsd] out of the store [n][steps][nsd]: one lane per (environment, record)
__global__ void __launch_bounds__(256) tds_traj_vjp_select_kernel(const double *store, double *s, long long n_items,
                                                                  int steps, int every, int n_rec, int nsd) {
  tds_rollout_vjp_select(store, s, n_items, steps, every, n_rec, nsd);
}

// ---------------------------------------------------------------- phase 2
// recording: wavefront blockIdx.x = (step t0 + blockIdx.x / nblk, environments e0 + 64 (blockIdx.x % nblk) ..); the
// lane's tape, lens[lane] = its length (-1: not recorded, or overflowed) and yidx [wavefront][nsd][lane] = the variables
// of y's first nsd entries
template <class B>
__global__ void __launch_bounds__(64) tds_traj_vjp_record_kernel(TdsTrajVjpArgs a, int e0, int nblk, int t0,
                                                                 const int *bad, int *over, TdsVjpParamLane<B> *lanes,
                                                                 int *lens, int *yidx, TdsRevIdx *ix, TdsRevPart *pd) {
  constexpr int cap = TdsVjpParamLane<B>::cap;
  const int l = threadIdx.x;
  const long long wave = blockIdx.x, lane = wave * 64 + l;
  const int t = t0 + (int)(wave / nblk);
  const long long env = e0 + (wave % nblk) * 64 + l;
  if (l == 0)
    tds_rev_tape() = TdsRevTape{ix + wave * cap * 64, pd + wave * cap * 64, nullptr, 64, cap, a.m->input_dim + a.p};
  __syncthreads();
  if (env >= a.n) return;
  if (bad[env]) {
    lens[lane] = -1;
    return;
  }
  TdsVjpParamLane<B> &L = lanes[lane];
  tds_traj_vjp_record<B>(a, L, (int)env, t);  // the primal was positive definite at every step
  const int len = tds_rev_cursor(l);
  if (len > cap) *a.overflow = 1, over[env] = 1;
  lens[lane] = len > cap ? -1 : len;
  for (int i = 0; i < a.nsd; ++i) yidx[(wave * a.nsd + i) * 64 + l] = L.y[i].i;
}

// the chained sweep of steps t1 - 1 .. t0 for environments e0 + 64 blockIdx.x ..: lambda [nsd][n] between them
template <class B>
__global__ void __launch_bounds__(64) tds_traj_vjp_sweep_kernel(TdsTrajVjpArgs a, int e0, int nblk, int t0, int t1,
                                                                const int *bad, const int *lens, const int *yidx,
                                                                TdsRevIdx *ix, TdsRevPart *pd, double *adj,
                                                                double *lam) {
  tds_rollout_vjp_sweep(TdsTrajVjpProblem{a, bad}, e0, nblk, t0, t1, TdsVjpParamLane<B>::cap, a.m->input_dim + a.p,
                        lens, yidx, ix, pd, adj, lam);
}

// the last pass: NaN gradients where the primal was NaN or a tape overflowed
__global__ void __launch_bounds__(256) tds_traj_vjp_nan_kernel(TdsTrajVjpArgs a, const int *bad, const int *over) {
  const int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env < a.n && (bad[env] || over[env])) tds_traj_vjp_nan(a, env);
}

// lanes of a recording launch, environments per chunk and steps per window
struct TdsTrajVjpPlan {
  long long chunk;
  int nblk, W;
};

inline TdsTrajVjpPlan tds_traj_vjp_plan(const tds_hip_sim *s, int n, int steps) {
  long long budget = s->opt.get(TDS_OPT_TRAJ_VJP_LANES, kTrajVjpLanesDefault);
  budget = budget < 64 ? 64 : budget > kTrajVjpLanesMax ? kTrajVjpLanesMax : budget / 64 * 64;
  const long long n64 = ((long long)n + 63) / 64 * 64;
  TdsTrajVjpPlan pl;
  pl.chunk = n64 < budget ? n64 : budget;
  pl.nblk = (int)(pl.chunk / 64);
  long long W = budget / pl.chunk;
  const long long opt = s->opt.get(TDS_OPT_TRAJ_STEPS, kTrajStepsDefault);
  if (W > opt) W = opt;
  if (W > steps) W = steps;
  pl.W = W < 1 ? 1 : (int)W;
  return pl;
}

// the work buffer: overflow flag | selection | state store | bad | over | lambda | then, one after the other in time,
// phase 1's lanes and carry and phase 2's lengths, y variables, lanes, tape indices, tape partials and adjoints
template <class B>
struct TdsTrajVjpLayout {
  size_t store, bad, over, lam, ph;                         // common
  size_t p1_carry, p1_end;                                  // phase 1 (lanes at ph)
  size_t lens, yidx, lanes, ix, pd, adj, total;             // phase 2 (lens at ph)
  long long p1_lanes;
  TdsTrajVjpLayout(const TdsTrajVjpPlan &pl, int n, int steps, int nsd, int nin, int p) {
    using Lane = TdsVjpParamLane<B>;
    constexpr size_t cap = Lane::cap;
    const size_t rec = (size_t)pl.W * pl.chunk;  // lanes of a recording launch
    store = 256 + tds_vjp_align((size_t)p * sizeof(tds_param_t));
    bad = store + tds_vjp_align((size_t)n * steps * nsd * sizeof(double));
    over = bad + tds_vjp_align((size_t)n * sizeof(int));
    lam = over + tds_vjp_align((size_t)n * sizeof(int));
    ph = lam + tds_vjp_align((size_t)n * nsd * sizeof(double));
    p1_lanes = n < kJvpLanes ? n : kJvpLanes;
    p1_carry = ph + tds_vjp_align((size_t)p1_lanes * sizeof(TdsTrajLane<B, 0>));
    p1_end = p1_carry + tds_vjp_align((size_t)tds_traj_ncarry<0>(nsd) * n * sizeof(double));
    lens = ph;
    yidx = lens + tds_vjp_align(rec * sizeof(int));
    lanes = yidx + tds_vjp_align(rec * nsd * sizeof(int));
    ix = lanes + tds_vjp_align(rec * sizeof(Lane));
    pd = ix + tds_vjp_align(rec * cap * sizeof(TdsRevIdx));
    adj = pd + tds_vjp_align(rec * cap * sizeof(TdsRevPart));
    total = adj + tds_vjp_align((size_t)pl.chunk * (nin + p + cap) * sizeof(double));
    if (total < p1_end) total = p1_end;
  }
};

// ---------------------------------------------------------------- closed loop: u_t = pi_W(obs(s_t))
// tds_hip_policy_trajectory_vjp: the trajectory with every step's action taken from the policy network (tds_policy.h)
// on the state that enters the step.  The policy's forward kernel runs in front of every primal step and writes the
// action where the open-loop kernels read it (t = 0: the action slots of a copy of x0; t > 0: row t - 1 of an action
// store), so the primal, recording and sweep kernels see an ordinary trajectory.  Backward, the recording launches stay
// (W steps side by side: a record depends on the primal alone); the sweeps go one step per launch, with the policy's
// backward kernel behind each: it reads ubar_t where the sweep scattered it (gu's row t - 1, or gx0's action slots at
// t = 0, which it then zeroes), adds ga_t, accumulates gpolicy and adds the observation adjoint to lambda (t = 0: to
// gx0's state part).

struct TdsPolicyTrajArgs {
  TdsPolicyNet nn;
  const double *x0, *policy, *ga;  // the caller's x0, [n][P], [n][steps][nact] or NULL
  double *u_out, *gpolicy;         // [n][steps][nact] or NULL, [n][P]
  int flags;
  bool grad;                       // a cotangent was given
};

inline int tds_policy_traj_raw(const TdsPolicyTrajArgs &pa, int t) {
  return ((pa.flags & 2) || ((pa.flags & 1) && t == 0)) ? 1 : 0;
}

// what the closed loop adds to the work buffer, behind the open loop's: the x0 copy, the action store, its adjoints
// and, where only ga is given, a zero gs
struct TdsPolicyTrajExtra {
  size_t xc, us, gu, gz, total;
  TdsPolicyTrajExtra(size_t base, int n, int steps, int n_rec, int nsd, int nin, int nact, bool grad, bool zero_gs) {
    const size_t rows = (size_t)n * (steps > 1 ? steps - 1 : 1) * nact * sizeof(double);
    xc = tds_vjp_align(base);
    us = xc + tds_vjp_align((size_t)n * nin * sizeof(double));
    gu = us + tds_vjp_align(rows);
    gz = gu + (grad ? tds_vjp_align(rows) : 0);
    total = gz + (zero_gs ? tds_vjp_align((size_t)n * n_rec * nsd * sizeof(double)) : 0);
  }
};

// ---------------------------------------------------------------- the device run
// pa NULL: the open loop.  pa given: the closed loop, whose x0 copy, action store and action adjoints stand in for the
// caller's x0, u and gu; without a cotangent (pa->grad false) it returns after the primal without waiting for it
template <class B>
int tds_traj_vjp_run(tds_hip_sim *s, TdsTrajVjpArgs a, const TdsPolicyTrajArgs *pa, const tds_param_t *params_host,
                     double *s_out) {
  using Lane = TdsVjpParamLane<B>;
  constexpr long long cap = Lane::cap;
  const int n = a.n, steps = a.steps, nsd = a.nsd, nact = a.nact, nin = s->model.input_dim;
  const bool grad = !pa || pa->grad, zero_gs = grad && !a.gs;
  const TdsTrajVjpPlan pl = tds_traj_vjp_plan(s, n, steps);
  const TdsTrajVjpLayout<B> lay(pl, n, steps, nsd, nin, a.p);
  const TdsPolicyTrajExtra ex(grad ? lay.total : lay.p1_end, n, steps, a.n_rec, nsd, nin, nact, grad, zero_gs);
  int rc = tds_work_buffer(s, pa ? ex.total : lay.total);
  if (rc) return rc;
  char *ws = (char *)s->d_diff_tmp;
  tds_param_t *d_sel = (tds_param_t *)(ws + 256);
  if (a.p > 0) {  // a blocking copy: earlier calls on the stream may still read the work buffer
    TDS_HIP_TRY(hipStreamSynchronize(s->stream));
    TDS_HIP_TRY(hipMemcpy(d_sel, params_host, (size_t)a.p * sizeof(tds_param_t), hipMemcpyHostToDevice));
  }
  a.params = d_sel;
  a.overflow = (int *)ws;
  double *store = (double *)(ws + lay.store), *lam = (double *)(ws + lay.lam);
  double *xc = (double *)(ws + ex.xc), *us = (double *)(ws + ex.us), *gu = (double *)(ws + ex.gu);  // closed loop
  int *bad = (int *)(ws + lay.bad), *over = (int *)(ws + lay.over);
  const long long urow = (long long)(steps > 1 ? steps - 1 : 1) * nact;  // an environment's doubles of us and gu
  a.store = store;
  hipStream_t st = s->stream;
  TDS_HIP_TRY(hipMemsetAsync(a.overflow, 0, sizeof(int), st));
  TDS_HIP_TRY(hipMemsetAsync(over, 0, lay.ph - lay.over, st));  // over and lambda (they lie side by side)
  if (pa) {
    a.x0 = xc, a.u = steps > 1 ? us : nullptr, a.gu = gu;
    TDS_HIP_TRY(hipMemcpyAsync(xc, pa->x0, (size_t)n * nin * sizeof(double), hipMemcpyDeviceToDevice, st));
  }
  // the observation of step t: the state that enters it
  auto obs = [&](int t) { return t > 0 ? store + (size_t)(t - 1) * nsd : xc; };
  auto obs_stride = [&](int t) { return t > 0 ? (long long)steps * nsd : (long long)nin; };

  // phase 1: the primal, at most traj_steps steps per launch (tds_traj.hip's chunking); closed loop: one step, the
  // policy in front of it
  {
    TdsTrajArgs ta = tds_traj_args(&s->model, a.m, n, steps, 1, a.x0, pa ? us : a.u, a.p, a.theta, 0, nullptr, store,
                                   nullptr);
    ta.a.params = d_sel;
    ta.items = n;
    ta.carry = (double *)(ws + lay.p1_carry);
    const long long opt = s->opt.get(TDS_OPT_TRAJ_STEPS, kTrajStepsDefault);
    const int per = pa || opt < 1 ? 1 : opt > steps ? steps : (int)opt;
    const unsigned blocks = (unsigned)((lay.p1_lanes + 63) / 64);
    for (int t0 = 0; t0 < steps; t0 += per) {
      const int t1 = t0 + per < steps ? t0 + per : steps;
      if (pa) {
        TdsPolicyFwdArgs f;
        f.policy = pa->policy, f.n = n, f.raw = tds_policy_traj_raw(*pa, t0);
        f.obs = obs(t0), f.obs_stride = obs_stride(t0);
        f.dst = t0 > 0 ? us + (size_t)(t0 - 1) * nact : xc + nsd, f.dst_stride = t0 > 0 ? urow : nin;
        f.out = pa->u_out ? pa->u_out + (size_t)t0 * nact : nullptr, f.out_stride = (long long)steps * nact;
        TDS_HIP_TRY((hipError_t)tds_policy_fwd_launch(st, pa->nn, f));
      }
      hipLaunchKernelGGL((tds_traj_vjp_primal_kernel<B>), dim3(blocks), dim3(64), 0, st, ta,
                         (TdsTrajLane<B, 0> *)(ws + lay.ph), lay.p1_lanes, t0, t1, bad);
      TDS_HIP_TRY(hipGetLastError());
    }
    if (s_out) {
      const long long items = (long long)n * a.n_rec;
      hipLaunchKernelGGL(tds_traj_vjp_select_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, store,
                         s_out, items, steps, a.every, a.n_rec, nsd);
      TDS_HIP_TRY(hipGetLastError());
    }
  }
  if (!grad) return TDS_OK;

  // phase 2: the accumulated gradients start at zero
  TDS_HIP_TRY(hipMemsetAsync(a.gx0, 0, (size_t)n * nin * sizeof(double), st));
  if (a.p > 0) TDS_HIP_TRY(hipMemsetAsync(a.gtheta, 0, (size_t)n * a.p * sizeof(double), st));
  const int P = pa ? pa->nn.nw + pa->nn.nb : 0;
  if (pa) {
    TDS_HIP_TRY(hipMemsetAsync(pa->gpolicy, 0, (size_t)n * P * sizeof(double), st));
    TDS_HIP_TRY(hipMemsetAsync(gu, 0, ex.gz - ex.gu, st));
  }
  if (zero_gs) {
    TDS_HIP_TRY(hipMemsetAsync(ws + ex.gz, 0, ex.total - ex.gz, st));
    a.gs = (const double *)(ws + ex.gz);
  }
  Lane *lanes = (Lane *)(ws + lay.lanes);
  int *lens = (int *)(ws + lay.lens), *yidx = (int *)(ws + lay.yidx);
  TdsRevIdx *ix = (TdsRevIdx *)(ws + lay.ix);
  TdsRevPart *pd = (TdsRevPart *)(ws + lay.pd);
  double *adj = (double *)(ws + lay.adj);
  auto record = [&](long long e0, int nblk, int t0, int t1) {
    hipLaunchKernelGGL((tds_traj_vjp_record_kernel<B>), dim3((unsigned)((t1 - t0) * nblk)), dim3(64), 0, st, a, (int)e0,
                       nblk, t0, bad, over, lanes, lens, yidx, ix, pd);
    return hipGetLastError();
  };
  auto sweep = [&](long long e0, int nblk, int t0, int t1, long long w0) {
    hipLaunchKernelGGL((tds_traj_vjp_sweep_kernel<B>), dim3((unsigned)nblk), dim3(64), 0, st, a, (int)e0, nblk, t0, t1,
                       bad, lens + w0 * 64, yidx + w0 * nsd * 64, ix + w0 * cap * 64, pd + w0 * cap * 64, adj, lam);
    return hipGetLastError();
  };
  auto policy_bwd = [&](long long e0, int nblk, int t) {
    const long long envs = (long long)n - e0 < (long long)nblk * 64 ? (long long)n - e0 : (long long)nblk * 64;
    TdsPolicyBwdArgs b;
    b.policy = pa->policy, b.gpolicy = pa->gpolicy, b.bad = bad, b.e0 = (int)e0, b.count = (int)envs;
    b.raw = tds_policy_traj_raw(*pa, t), b.zero_ubar = t == 0;
    b.obs = obs(t), b.obs_stride = obs_stride(t);
    b.ubar = t > 0 ? gu + (size_t)(t - 1) * nact : a.gx0 + nsd, b.ubar_stride = t > 0 ? urow : nin;
    b.ga = pa->ga ? pa->ga + (size_t)t * nact : nullptr, b.ga_stride = (long long)steps * nact;
    b.lam = t > 0 ? lam : a.gx0, b.lam_entry = t > 0 ? n : 1, b.lam_env = t > 0 ? 1 : nin;
    return (hipError_t)tds_policy_bwd_launch(st, pa->nn, b);
  };
  const size_t adj_bytes = lay.total - lay.adj;
  TDS_HIP_TRY(pa ? tds_rollout_vjp_backward(st, n, steps, pl.chunk, pl.W, adj, adj_bytes, record, sweep, policy_bwd)
                 : tds_rollout_vjp_backward(st, n, steps, pl.chunk, pl.W, adj, adj_bytes, record, sweep));
  hipLaunchKernelGGL(tds_traj_vjp_nan_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a, bad, over);
  TDS_HIP_TRY(hipGetLastError());
  if (pa) TDS_HIP_TRY((hipError_t)tds_policy_nan_launch(st, pa->gpolicy, P, bad, over, n));
  int overflow = 0;
  TDS_HIP_TRY(tds_rollout_vjp_overflow(st, a.overflow, &overflow));
  if (overflow)
    return fail(TDS_ERR_UNSUPPORTED,
                "trajectory VJP: an environment's tape exceeds the capacity of its model class%s");
  return TDS_OK;
}

// ---------------------------------------------------------------- the host run
// the host instantiation: per environment the primal into a store (closed loop: step by step, the network in front of
// each, over a carry), then one tape at a time, t descending (closed loop: the network's backward pass behind each
// sweep)
template <class B>
int tds_traj_vjp_host_run(TdsTrajVjpArgs a, const TdsPolicyTrajArgs *pa, double *s_out, int tape_cap, int *tape_len) {
  using Lane = TdsVjpParamLane<B>;
  const tds_model_t *m = a.m;
  const int n = a.n, steps = a.steps, nsd = a.nsd, nact = a.nact, nin = m->input_dim, nall = nin + a.p;
  const bool grad = !pa || pa->grad;
  const int P = pa ? pa->nn.nw + pa->nn.nb : 0;
  const int cap = tape_cap > 0 ? tape_cap : Lane::cap;
  const size_t urow = (size_t)(steps > 1 ? steps - 1 : 1) * nact;
  std::vector<double> store((size_t)n * steps * nsd), lam(nsd), adj(grad ? (size_t)nall + cap : 0);
  std::vector<double> xc, us, gu, carry, gz, act, dact, del;  // closed loop
  std::vector<TdsTrajLane<B, 0>> Ly(1);
  std::vector<Lane> L(grad ? 1 : 0);
  std::vector<TdsRevIdx> ix(grad ? cap : 0);
  std::vector<TdsRevPart> pd(grad ? cap : 0);
  std::vector<int> yi(nsd);
  if (pa) {
    xc.assign(pa->x0, pa->x0 + (size_t)n * nin), us.resize(n * urow), gu.assign(n * urow, 0.0);
    carry.resize((size_t)tds_traj_ncarry<0>(nsd) * n);
    act.resize(kPolicyActs), dact.resize(kPolicyActs), del.resize(2 * TDS_NN_MAX_UNITS);
    if (grad && !a.gs) {
      gz.assign((size_t)n * a.n_rec * nsd, 0.0);
      a.gs = gz.data();
    }
    a.x0 = xc.data(), a.u = steps > 1 ? us.data() : nullptr, a.gu = gu.data();
  }
  a.store = store.data();
  TdsTrajArgs ta = tds_traj_args(m, m, n, steps, 1, a.x0, pa ? us.data() : a.u, a.p, a.theta, 0, nullptr, store.data(),
                                 nullptr);
  ta.a.params = a.params;
  ta.items = n;
  if (pa) ta.carry = carry.data();  // the open loop advances an environment in one go
  const TdsRevTape tp = {ix.data(), pd.data(), adj.data(), 1, cap, nall};
  const TdsTrajVjpProblem pr = {a, nullptr};
  if (grad) tds_rev_tape() = tp;
  auto obs_of = [&](int e, int t) {
    return t > 0 ? store.data() + ((size_t)e * steps + (t - 1)) * nsd : xc.data() + (size_t)e * nin;
  };
  int bad = 0, over = 0;
  for (int e = 0; e < n; ++e) {
    const double *W = pa ? pa->policy + (size_t)e * P : nullptr;
    int bad_e = 0;
    if (!pa) bad_e = tds_traj_advance<B, 0>(ta, Ly[0], e, 0, steps);
    for (int t = 0; pa && t < steps; ++t) {
      tds_policy_forward(pa->nn, W, obs_of(e, t), tds_policy_traj_raw(*pa, t), act.data(), nullptr);
      const double *out = act.data() + (pa->nn.n - 1) * TDS_NN_MAX_UNITS;
      double *dst = t > 0 ? us.data() + e * urow + (size_t)(t - 1) * nact : xc.data() + (size_t)e * nin + nsd;
      std::copy_n(out, nact, dst);
      if (pa->u_out) std::copy_n(out, nact, pa->u_out + ((size_t)e * steps + t) * nact);
      bad_e = tds_traj_advance<B, 0>(ta, Ly[0], e, t, t + 1);
    }
    if (s_out)
      for (int r = 0; r < a.n_rec; ++r)
        std::copy_n(&store[((size_t)e * steps + (size_t)(r + 1) * a.every - 1) * nsd], nsd,
                    s_out + ((size_t)e * a.n_rec + r) * nsd);
    bad |= bad_e;
    if (!grad) continue;
    double *gx = a.gx0 + (size_t)e * nin, *gP = pa ? pa->gpolicy + (size_t)e * P : nullptr;
    std::fill_n(gx, nin, 0.0);
    std::fill_n(a.gtheta + (size_t)e * a.p, a.p, 0.0);
    if (pa) std::fill_n(gP, P, 0.0);
    std::fill(lam.begin(), lam.end(), 0.0);
    int over_e = 0;
    for (int t = steps - 1; t >= 0 && !bad_e; --t) {
      tds_traj_vjp_record<B>(a, L[0], e, t);
      const int len = tds_rev_cursor(0);
      if (tape_len) tape_len[(size_t)e * steps + t] = len > cap ? -1 : len;
      over_e |= len > cap;
      if (over_e) continue;  // the remaining steps are recorded for their lengths only
      for (int i = 0; i < nsd; ++i) yi[i] = L[0].y[i].i;
      tds_rollout_vjp_host_step(pr, tp, len, e, t, yi.data(), lam.data());
      if (!pa) continue;
      // the network at obs_t: ubar_t (+ ga_t) down the layers
      const int raw = tds_policy_traj_raw(*pa, t);
      tds_policy_forward(pa->nn, W, obs_of(e, t), raw, act.data(), dact.data());
      double *ub = t > 0 ? gu.data() + e * urow + (size_t)(t - 1) * nact : gx + nsd;
      for (int i = 0; i < nact; ++i) {
        del[i] = ub[i] + (pa->ga ? pa->ga[((size_t)e * steps + t) * nact + i] : 0.0);
        if (t == 0) ub[i] = 0.0;
      }
      const double *gobs = tds_policy_backward(pa->nn, W, act.data(), dact.data(), del.data(),
                                               del.data() + TDS_NN_MAX_UNITS, gP);
      double *dstl = t > 0 ? lam.data() : gx;
      for (int o = 0; o < nsd; ++o)
        if (o >= 2 || raw) dstl[o] += gobs[o];
    }
    if (bad_e && tape_len) std::fill_n(tape_len + (size_t)e * steps, steps, 0);
    if (bad_e || over_e) {
      tds_traj_vjp_nan(a, e);
      if (pa) std::fill_n(gP, P, __builtin_nan(""));
    }
    over |= over_e;
  }
  if (grad) tds_rev_tape() = TdsRevTape{};
  if (over) return fail(TDS_ERR_UNSUPPORTED, "trajectory VJP: an environment's tape exceeds the capacity%s");
  if (bad) return fail(TDS_ERR_INVALID_ARG, "step Jacobians: joint-space inertia not positive definite%s");
  return TDS_OK;
}

// the checks of tds_traj_check_args and the outputs the call needs
int tds_traj_vjp_check_args(const char *fn, const tds_model_t *m, int n, int steps, int every, int p, const void *x0,
                            const void *u, const void *params, const void *gs, const void *gx0, const void *gu,
                            const void *gtheta) {
  int rc = tds_traj_check_args(fn, n, steps, every, 1, p, x0, params, gs, gx0, gx0);
  if (rc) return rc;
  const int nact = m->input_dim - m->dof_q - m->dof_qd - (m->step_mode == TDS_STEP_LOCOMOTION ? 3 : 0);
  if ((p > 0 && !gtheta) || (u && nact > 0 && steps > 1 && !gu))
    return fail(TDS_ERR_INVALID_ARG, fn, ": NULL or empty argument");
  return TDS_OK;
}

TdsTrajVjpArgs tds_traj_vjp_args(const tds_model_t *m, const tds_model_t *m_arg, int n, int steps, int every,
                                 const double *x0, const double *u, int p, const tds_param_t *params,
                                 const double *theta, const double *gs, double *gx0, double *gu, double *gtheta) {
  TdsTrajVjpArgs a;
  a.m = m_arg, a.n = n, a.p = p, a.steps = steps, a.every = every, a.n_rec = steps / every;
  a.nsd = m->dof_q + m->dof_qd;
  a.nact = m->input_dim - a.nsd - (m->step_mode == TDS_STEP_LOCOMOTION ? 3 : 0);
  // actions that no step reads (steps = 1) or that have no slots are no input of the call
  a.x0 = x0, a.u = steps > 1 && a.nact > 0 ? u : nullptr, a.theta = theta, a.gs = gs, a.params = params;
  a.store = nullptr, a.gx0 = gx0, a.gu = gu, a.gtheta = gtheta, a.overflow = nullptr;
  return a;
}

// the argument checks of both entry points, up to the model's own
int tds_policy_traj_check_args(const char *fn, int n, int steps, int every, int p, const void *x0, const void *policy,
                               const void *params, const void *gs, const void *ga, const void *s, const void *gpolicy,
                               const void *gx0, const void *gtheta) {
  const bool grad = gs || ga;
  int rc = tds_traj_check_args(fn, n, steps, every, grad ? 1 : 0, p, x0, params, grad ? gx0 : nullptr, s,
                               grad ? gpolicy : nullptr);
  if (rc) return rc;
  if (!policy || (grad && p > 0 && !gtheta)) return fail(TDS_ERR_INVALID_ARG, fn, ": NULL or empty argument");
  return TDS_OK;
}

// the model's actions and the network, once the model itself has passed
int tds_policy_traj_net(const char *fn, const tds_model_t *m, int num_layers, const int *layer_sizes,
                        const int *activations, const int *use_bias, int flags, TdsPolicyNet *nn) {
  const int nsd = m->dof_q + m->dof_qd;
  const int nact = m->input_dim - nsd - (m->step_mode == TDS_STEP_LOCOMOTION ? 3 : 0);
  if (m->action_dim < 1 || nact != m->action_dim)
    return fail(TDS_ERR_INVALID_ARG, fn, ": the model has no actions, or its record's action slots are not its actions");
  if (flags & ~3) return fail(TDS_ERR_INVALID_ARG, fn, ": unknown flags");
  if (const char *why = tds_policy_net_make(nsd, m->action_dim, num_layers, layer_sizes, activations, use_bias, nn)) {
    snprintf(tds_internal::g_err, sizeof(tds_internal::g_err), "%s", why);
    return TDS_ERR_INVALID_ARG;
  }
  return TDS_OK;
}

}  // namespace

extern "C" {

int tds_hip_trajectory_vjp(tds_hip_sim_t *s, int n, int steps, int every, const void *x0_dev, const void *u_dev,
                           int p, const tds_param_t *params_host, const void *theta_dev, const void *gs_dev,
                           void *s_dev, void *gx0_dev, void *gu_dev, void *gtheta_dev) {
  if (!s) return fail(TDS_ERR_INVALID_ARG, "tds_hip_trajectory_vjp: NULL or empty argument%s");
  int rc = tds_traj_vjp_check_args("tds_hip_trajectory_vjp%s", &s->model, n, steps, every, p, x0_dev, u_dev,
                                   params_host, gs_dev, gx0_dev, gu_dev, gtheta_dev);
  if (rc) return rc;
  DeviceGuard guard(s->device);
  int cls;
  if ((rc = tds_diff_prepare(s, &cls))) return rc;
  if ((rc = tds_param_check_sel(&s->model, p, params_host))) return rc;
  const TdsTrajVjpArgs a = tds_traj_vjp_args(&s->model, (const tds_model_t *)s->d_diff_model, n, steps, every,
                                             (const double *)x0_dev, (const double *)u_dev, p, nullptr,
                                             (const double *)theta_dev, (const double *)gs_dev, (double *)gx0_dev,
                                             (double *)gu_dev, (double *)gtheta_dev);
  return tds_with_bound(cls, [&](auto b) {
    return tds_traj_vjp_run<typename decltype(b)::type>(s, a, nullptr, params_host, (double *)s_dev);
  });
}

int tds_hip_trajectory_vjp_host(const tds_model_t *model, int n, int steps, int every, const double *x0,
                                const double *u, int p, const tds_param_t *params, const double *theta,
                                const double *gs, double *s, double *gx0, double *gu, double *gtheta, int tape_cap,
                                int *tape_len) {
  if (!model) return fail(TDS_ERR_INVALID_ARG, "tds_hip_trajectory_vjp_host: NULL or empty argument%s");
  int rc = tds_traj_vjp_check_args("tds_hip_trajectory_vjp_host%s", model, n, steps, every, p, x0, u, params, gs, gx0,
                                   gu, gtheta);
  if (rc) return rc;
  int cls;
  if ((rc = tds_param_host_prepare(model, p, params, &cls))) return rc;
  const TdsTrajVjpArgs a = tds_traj_vjp_args(model, model, n, steps, every, x0, u, p, params, theta, gs, gx0, gu, gtheta);
  return tds_with_bound(cls, [&](auto b) {
    return tds_traj_vjp_host_run<typename decltype(b)::type>(a, nullptr, s, tape_cap, tape_len);
  });
}

int tds_hip_policy_trajectory_vjp(tds_hip_sim_t *s, int n, int steps, int every, int flags, const void *x0_dev,
                                  const void *policy_dev, int num_layers, const int *layer_sizes,
                                  const int *activations, const int *use_bias, int p, const tds_param_t *params_host,
                                  const void *theta_dev, const void *gs_dev, const void *ga_dev, void *s_dev,
                                  void *u_dev, void *gpolicy_dev, void *gx0_dev, void *gtheta_dev) {
  const char *fn = "tds_hip_policy_trajectory_vjp%s";
  if (!s) return fail(TDS_ERR_INVALID_ARG, fn, ": NULL or empty argument");
  int rc = tds_policy_traj_check_args(fn, n, steps, every, p, x0_dev, policy_dev, params_host, gs_dev, ga_dev, s_dev,
                                      gpolicy_dev, gx0_dev, gtheta_dev);
  if (rc) return rc;
  DeviceGuard guard(s->device);
  int cls;
  if ((rc = tds_diff_prepare(s, &cls))) return rc;
  if ((rc = tds_param_check_sel(&s->model, p, params_host))) return rc;
  TdsPolicyTrajArgs pa;
  if ((rc = tds_policy_traj_net(fn, &s->model, num_layers, layer_sizes, activations, use_bias, flags, &pa.nn))) return rc;
  pa.x0 = (const double *)x0_dev, pa.policy = (const double *)policy_dev, pa.ga = (const double *)ga_dev;
  pa.u_out = (double *)u_dev, pa.gpolicy = (double *)gpolicy_dev, pa.flags = flags, pa.grad = gs_dev || ga_dev;
  const TdsTrajVjpArgs a = tds_traj_vjp_args(&s->model, (const tds_model_t *)s->d_diff_model, n, steps, every,
                                             (const double *)x0_dev, nullptr, p, nullptr, (const double *)theta_dev,
                                             (const double *)gs_dev, (double *)gx0_dev, nullptr, (double *)gtheta_dev);
  return tds_with_bound(cls, [&](auto b) {
    return tds_traj_vjp_run<typename decltype(b)::type>(s, a, &pa, params_host, (double *)s_dev);
  });
}

int tds_hip_policy_trajectory_vjp_host(const tds_model_t *model, int n, int steps, int every, int flags,
                                       const double *x0, const double *policy, int num_layers, const int *layer_sizes,
                                       const int *activations, const int *use_bias, int p, const tds_param_t *params,
                                       const double *theta, const double *gs, const double *ga, double *s, double *u,
                                       double *gpolicy, double *gx0, double *gtheta, int tape_cap, int *tape_len) {
  const char *fn = "tds_hip_policy_trajectory_vjp_host%s";
  if (!model) return fail(TDS_ERR_INVALID_ARG, fn, ": NULL or empty argument");
  int rc = tds_policy_traj_check_args(fn, n, steps, every, p, x0, policy, params, gs, ga, s, gpolicy, gx0, gtheta);
  if (rc) return rc;
  int cls;
  if ((rc = tds_param_host_prepare(model, p, params, &cls))) return rc;
  TdsPolicyTrajArgs pa;
  if ((rc = tds_policy_traj_net(fn, model, num_layers, layer_sizes, activations, use_bias, flags, &pa.nn))) return rc;
  pa.x0 = x0, pa.policy = policy, pa.ga = ga, pa.u_out = u, pa.gpolicy = gpolicy, pa.flags = flags;
  pa.grad = gs || ga;
  const TdsTrajVjpArgs a = tds_traj_vjp_args(model, model, n, steps, every, x0, nullptr, p, params, theta, gs, gx0,
                                             nullptr, gtheta);
  return tds_with_bound(cls, [&](auto b) {
    return tds_traj_vjp_host_run<typename decltype(b)::type>(a, &pa, s, tape_cap, tape_len);
  });
}

}  // extern "C"
