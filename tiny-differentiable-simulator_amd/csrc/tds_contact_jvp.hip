// tds_contact_jvp.hip — forward-mode derivatives of the batched contact query in [x | theta] on gfx950 (tds_contact.h
// over TdsDual<K> and an overlay of parameters) and their C ABI: tds_hip_contacts_jvp, the CPU checker
// tds_hip_contacts_jvp_host and tds_hip_contacts_jvp_tangents (include/tds_hip.h).
//
// The mapping, the launch, the host checker's loop and the entry points' bodies are tds_query_dual.h's.  This unit
// states what is the contact query's own: the record x as the one input, tds_contact_layout and tds_contact_eval, and
// its nine outputs, of which rows .. qd_post are NaN where M is not positive definite; once in its kernel, once for the
// host (TdsContactJvpUnit).
#include <hip/hip_runtime.h>

#include "tds_contact.h"
#include "tds_query_dual.h"

namespace {

struct TdsContactJvpArgs {
  const tds_model_t *m;
  int n, kdirs, p, what, with_A;
  const double *x, *theta, *v;
  const tds_param_t *params;
  tds_contact_out_t out, dout;  // primal outputs; tangents [n][kdirs][shape]
  // the columns of v in all and before theta (nx reads the model where it is used)
  struct Columns {
    const tds_model_t *m;
    int nall;
    TDS_HD int nx() const { return m->input_dim; }
  };
  TDS_HD Columns columns() const { return {m, m->input_dim + p}; }
};

template <class B, int K>
__global__ void __launch_bounds__(64) tds_contact_jvp_kernel(TdsContactJvpArgs a, double *buf,
                                                             TdsParamOverlay<typename TdsContactScalar<K>::type, B> *ovl,
                                                             int lanes) {
  using T = typename TdsQueryScalar<K>::type;
  __shared__ double tile[64 * kTileS];
  const tds_model_t *m = a.m;
  const TdsContactLayout L = tds_contact_layout(m, a.with_A);
  const int W = blockDim.x, t = threadIdx.x, nin = m->input_dim, nd = m->dof_qd, nc = L.nc, nr = 3 * nc;
  const TdsQueryJvpLane<K> ln(buf, lanes, W, t);
  const TdsDynMem<T> w = {(T *)buf + ln.lane, (size_t)lanes};
  TdsParamOverlay<T, B> &P = ovl[ln.lane];
  const int chunks = (a.n + W - 1) / W, blocks = a.kdirs > 0 ? (a.kdirs + K - 1) / (K ? K : 1) : 1;
  const long long groups = (long long)chunks * blocks;
  tds_param_seed(m, P);  // the blob's values, all constant: once per lane
  for (long long g = blockIdx.x; g < groups; g += gridDim.x) {
    const int e0 = (int)(g % chunks) * W, d0 = (int)(g / chunks) * K;  // neighbouring workgroups: neighbouring environments
    const int nv = a.n - e0 < W ? a.n - e0 : W, nk = a.kdirs - d0 < K ? a.kdirs - d0 : K;
    tds_query_ingest(tile, ln.plane(0), L.x, a.x, nin, e0, nv);
    for (int k = 0; k < K; ++k)
      if (k < nk) {
        tds_query_ingest_strided(tile, ln.plane(1 + k), L.x, a.v + (size_t)(d0 + k) * (nin + a.p), nin,
                                 (size_t)a.kdirs * (nin + a.p), e0, nv);
      } else if (t < nv) {  // directions past kdirs in the last block: zero
        const TdsDynMem<double> z = ln.plane(1 + k);
        for (int c = 0; c < nin; ++c) z[L.x + c] = 0.0;
      }
    int bad = 0;
    if (t < nv) {
      tds_query_jvp_theta(a, P, e0 + t, d0, nk);
      bad = tds_contact_eval(m, TdsOverlayView<T, B>{&P}, w, L, a.what);  // M not positive definite
    }
    // output `off` [cnt]: the primal by the first block's items, then this block's tangents [n][kdirs][cnt]
    const auto emit = [&](void *o, void *dto, int off, int cnt, int nan) {
      if (!cnt) return;
      if (o && d0 == 0) tds_query_emit(tile, ln.plane(0), off, (double *)o, cnt, e0, nv, nan);
      if (dto)
        for (int k = 0; k < nk; ++k)
          tds_query_emit_strided(tile, ln.plane(1 + k), off, (double *)dto + (size_t)(d0 + k) * cnt, cnt,
                                 (size_t)a.kdirs * cnt, e0, nv, nan);
    };
    emit(a.out.contacts, a.dout.contacts, L.cp, 10 * nc, 0);
    emit(a.out.jac, a.dout.jac, L.cjac, 3 * nd * nc, 0);
    emit(a.out.rows, a.dout.rows, L.J, nr * nd, bad);
    emit(a.out.rhs, a.dout.rhs, L.b, nr, bad);
    emit(a.out.delassus, a.dout.delassus, L.A, nr * nr, bad);
    emit(a.out.impulse, a.dout.impulse, L.p, nr, bad);
    emit(a.out.force, a.dout.force, L.force, nr, bad);
    emit(a.out.qd_pre, a.dout.qd_pre, L.qd_pre, nd, bad);
    emit(a.out.qd_post, a.dout.qd_post, L.qd_post, nd, bad);
  }
}

// the unit as tds_query_dual.h's host side sees it
struct TdsContactJvpUnit {
  using Args = TdsContactJvpArgs;
  // tangents per work item of a class on the device (the resource table; to be specialised per class)
  template <class B>
  static constexpr int kTangents = 2;
  template <class B, int K>
  static constexpr auto kKernel = tds_contact_jvp_kernel<B, K>;
  static constexpr const char *kNotPd = "contact query: joint-space inertia not positive definite%s";

  const Args &a;
  const TdsContactLayout L;
  explicit TdsContactJvpUnit(const Args &a) : a(a), L(tds_contact_layout(a.m, a.with_A)) {}
  int total() const { return L.total; }
  template <class Put>
  void inputs(const Put &put) const {
    put(L.x, a.x, 0, a.m->input_dim);
  }
  template <typename T, class B>
  int eval(TdsOverlayView<T, B> P, TdsDynMem<T> w) const {
    return tds_contact_eval(a.m, P, w, L, a.what);
  }
  template <class Get>
  void outputs(const Get &get, int bad) const {
    const int nd = a.m->dof_qd, nc = L.nc, nr = 3 * nc;
    get(a.out.contacts, a.dout.contacts, L.cp, 10 * nc, 0);
    get(a.out.jac, a.dout.jac, L.cjac, 3 * nd * nc, 0);
    get(a.out.rows, a.dout.rows, L.J, nr * nd, bad);
    get(a.out.rhs, a.dout.rhs, L.b, nr, bad);
    get(a.out.delassus, a.dout.delassus, L.A, nr * nr, bad);
    get(a.out.impulse, a.dout.impulse, L.p, nr, bad);
    get(a.out.force, a.dout.force, L.force, nr, bad);
    get(a.out.qd_pre, a.dout.qd_pre, L.qd_pre, nd, bad);
    get(a.out.qd_post, a.dout.qd_post, L.qd_post, nd, bad);
  }
};

// the arguments of an entry point, checked, as the kernel's and the host loop's (a->what == 0: nothing with extent
// is asked for)
int tds_contact_jvp_args(const char *who, const tds_model_t *model, int n, const void *x, int p, const tds_param_t *params,
                         const void *theta, int k, const void *v, const tds_contact_out_t *out,
                         const tds_contact_out_t *dout, TdsContactJvpArgs *a) {
  if (const int rc = tds_query_jvp_check(who, n, x, p, params, k, v, out, dout, tds_contact_any)) return rc;
  const int nc = tds_contact_count(model), what = tds_contact_what(out, nc) | tds_contact_what(dout, nc);
  *a = {model, n, k, p, what, (what & TDS_CT_DELASSUS) ? 1 : 0, (const double *)x, (const double *)theta,
        (const double *)v, params, *out, *dout};
  return TDS_OK;
}

}  // namespace

extern "C" {

int tds_hip_contacts_jvp(tds_hip_sim_t *s, int n, const void *x_dev, int p, const tds_param_t *params_host,
                         const void *theta_dev, int k, const void *v_dev, const tds_contact_out_t *out,
                         const tds_contact_out_t *dout) {
  const char *who = "tds_hip_contacts_jvp";
  return tds_query_jvp_device<TdsContactJvpUnit>(who, s, p, params_host, k, [&](const tds_model_t *m, TdsContactJvpArgs *a) {
    return tds_contact_jvp_args(who, m, n, x_dev, p, params_host, theta_dev, k, v_dev, out, dout, a);
  });
}

int tds_hip_contacts_jvp_host(const tds_model_t *model, int n, const double *x, int p, const tds_param_t *params,
                              const double *theta, int k, const double *v, const tds_contact_out_t *out,
                              const tds_contact_out_t *dout) {
  const char *who = "tds_hip_contacts_jvp_host";
  return tds_query_jvp_host<TdsContactJvpUnit>(who, model, p, params, k, [&](const tds_model_t *m, TdsContactJvpArgs *a) {
    return tds_contact_jvp_args(who, m, n, x, p, params, theta, k, v, out, dout, a);
  });
}

int tds_hip_contacts_jvp_tangents(const tds_model_t *model) {
  return tds_query_jvp_tangents<TdsContactJvpUnit>("tds_hip_contacts_jvp_tangents", model);
}

}  // extern "C"
