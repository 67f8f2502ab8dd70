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
// This is a path of its own: neither the step kernels nor the forward-mode kernel (tds_jvp.hip) change.  The sweep, the
// layout, the launches and the host instantiation are tds_vjp_kernels.h's, shared with the parameter derivatives
// (tds_dparam.hip); the recording kernel is this file's own (tds_vjp_kernels.h says why).
#include <hip/hip_runtime.h>
#include <string.h>

#include "tds_vjp_kernels.h"

namespace {

// tape entries a lane may record, per class: the longest tape counted for the class's models (golden records, and
// the contact sweep of tests/diff_states.py, every reachable contact count), plus 18 - 28 %
template <class B>
struct TdsVjpCap;
template <>
struct TdsVjpCap<TdsBoundS> { static constexpr int N = 16384; };
template <>
struct TdsVjpCap<TdsBoundA> { static constexpr int N = 81920; };
template <>
struct TdsVjpCap<TdsBoundL> { static constexpr int N = 73728; };

template <class B>
struct TdsVjpLane;

// record one environment's tape (the cursor of the calling lane counts its entries); 0 or the step's -1
template <class B>
TDS_HD inline int tds_vjp_record(const tds_model_t *m, TdsVjpLane<B> &L, const double *xe) {
  for (int i = 0; i < m->input_dim; ++i) L.x[i] = TdsRev(xe[i], i);
  tds_rev_cursor(tds_rev_lane()) = 0;
  return tds_diff_step(m, L.w, L.x, L.y);
}

// a lane's work object: the record and the step's state in TdsRev form (the lane type of tds_vjp_kernels.h)
template <class B>
struct TdsVjpLane {
  static constexpr int cap = TdsVjpCap<B>::N;
  TdsRev x[B::NX], y[B::NY];
  TdsDiffWork<TdsRev, B> w;
  TDS_HD static int n_extra(const TdsVjpArgs &) { return 0; }
  TDS_HD int record(const TdsVjpArgs &a, long long env) { return tds_vjp_record<B>(a.m, *this, a.x + env * a.m->input_dim); }
};

// the recording kernel of the plain lane: the lane's tape and y; lens[lane] = the tape's length, -1 where the
// environment's outputs are NaN.  It evaluates the step over TdsRev (its register allocation is the step's)
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
  tds_vjp_y(m, L, nin, bad, a.k, a.y ? a.y + env * nout : nullptr, a.wj + env * a.k * nin);
}

struct TdsVjpRecordPlain {
  template <class B>
  void operator()(hipStream_t st, dim3 grid, const TdsVjpArgs &b, long long base, TdsVjpLane<B> *lanes, int *lens,
                  TdsRevIdx *ix, TdsRevPart *pd) const {
    hipLaunchKernelGGL((tds_vjp_record_kernel<B>), grid, dim3(64), 0, st, b, base, lanes, lens, ix, pd);
  }
};

template <class B>
int tds_vjp_launch(tds_hip_sim *s, const TdsVjpArgs &a) {
  const long long n_lanes = tds_vjp_lanes(a.n);
  const TdsVjpLayout<TdsVjpLane<B>> lay(n_lanes, s->model.input_dim);
  int rc = tds_work_buffer(s, lay.total);
  if (rc) return rc;
  return tds_vjp_run(s, a, lay, n_lanes, TdsVjpRecordPlain{});
}

// the host instantiation over environments [0, n); tape_cap <= 0: the class's capacity; tape_len [n] (optional):
// entries each environment recorded, -1 where its tape overflowed
template <class B>
int tds_vjp_host_impl(const tds_model_t *m, int n, const double *x, int k, const double *w, double *y, double *wj,
                      int tape_cap, int *tape_len) {
  const TdsVjpArgs a = {m, n, k, x, w, y, wj, nullptr};
  return tds_vjp_host_run<TdsVjpLane<B>>(a, tape_cap, tape_len);
}

}  // namespace

extern "C" {

int tds_hip_vjp(tds_hip_sim_t *s, int n, const void *x_dev, int k, const void *w_dev, void *y_dev, void *wj_dev) {
  if (!s || !x_dev || !w_dev || !wj_dev || n < 1 || k < 1) return fail(TDS_ERR_INVALID_ARG, "tds_hip_vjp: NULL or empty argument%s");
  DeviceGuard guard(s->device);
  int cls, rc = tds_diff_prepare(s, &cls);
  if (rc) return rc;
  TdsVjpArgs a = {(const tds_model_t *)s->d_diff_model, n, k, (const double *)x_dev, (const double *)w_dev,
                  (double *)y_dev, (double *)wj_dev, nullptr};
  return tds_with_bound(cls, [&](auto b) { return tds_vjp_launch<typename decltype(b)::type>(s, a); });
}

int tds_hip_vjp_host_tape(const tds_model_t *model, int n, const double *x, int k, const double *w, double *y,
                          double *wj, int tape_cap, int *tape_len) {
  if (!model || !x || !w || !wj || n < 1 || k < 1) return fail(TDS_ERR_INVALID_ARG, "tds_hip_vjp_host: NULL or empty argument%s");
  int cls, rc = tds_diff_host_check(model, &cls);
  if (rc) return rc;
  return tds_with_bound(cls, [&](auto b) {
    return tds_vjp_host_impl<typename decltype(b)::type>(model, n, x, k, w, y, wj, tape_cap, tape_len);
  });
}

int tds_hip_vjp_host(const tds_model_t *model, int n, const double *x, int k, const double *w, double *y, double *wj) {
  return tds_hip_vjp_host_tape(model, n, x, k, w, y, wj, 0, nullptr);
}

}  // extern "C"
