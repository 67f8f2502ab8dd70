// tds_policy.h — the policy network of the rollouts (tds_hip_set_policy_network: NeuralNetwork::compute) for ONE
// environment over f64, forward and backward, stated once for the device kernels of tds_policy_grad.hip (one wavefront
// per environment) and for the host checker of tds_hip_policy_trajectory_vjp_host.
//
// The statement is written over the 64 lanes of a wavefront: TDS_POLICY_LANES(l) { .. } is the body of lane l (device:
// the thread's own lane; host: a loop over 64 lanes), TDS_POLICY_SYNC() separates phases that exchange data through the
// activation arrays (device: LDS).  The summation order of a unit's dot product is fixed here: lane l sums the products
// of the inputs l, l + 64, .. in ascending order, then the 64 partial sums meet in the xor butterfly with distances
// 1, 2, .. 32 (the order of tds_policy_mlp_kernel).  The host walks the same tree, so with FP contraction off (Makefile)
// host and device differ only where their tanh / exp / sin do.
//
// Parameter order as tds_hip_set_policy_network: the weights of layers 1 .., row-major [unit][input], then the biases of
// the layers that have them, the input layer's first.  The default linear policy is the network {obs, act}, identity,
// bias on the output layer.
#pragma once
#include <math.h>

#include "tds_dual.h"
#include "tds_hip.h"

struct TdsPolicyNet {
  int n, units[TDS_NN_MAX_LAYERS], act[TDS_NN_MAX_LAYERS], bias[TDS_NN_MAX_LAYERS], nw, nb;
};

// doubles of an activation array: [layer][TDS_NN_MAX_UNITS]
constexpr int kPolicyActs = TDS_NN_MAX_LAYERS * TDS_NN_MAX_UNITS;

// the checks of tds_hip_set_policy_network; num_layers = 0: the linear policy.  NULL, or what is wrong
inline const char *tds_policy_net_make(int obs_dim, int action_dim, int num_layers, const int *layer_sizes,
                                       const int *activations, const int *use_bias, TdsPolicyNet *nn) {
  *nn = TdsPolicyNet{};
  if (num_layers == 0) {
    nn->n = 2;
    nn->units[0] = obs_dim, nn->units[1] = action_dim;
    nn->act[0] = TDS_NN_ACT_IDENTITY;
    nn->bias[1] = 1;
    nn->nw = obs_dim * action_dim, nn->nb = action_dim;
    return nullptr;
  }
  if (num_layers < 2 || num_layers > TDS_NN_MAX_LAYERS) return "num_layers must be 0 or 2..TDS_NN_MAX_LAYERS";
  if (!layer_sizes || !activations || !use_bias) return "NULL argument";
  if (layer_sizes[0] != obs_dim) return "layer_sizes[0] must be the observation size dof_q + dof_qd";
  if (layer_sizes[num_layers - 1] != action_dim) return "the last layer must have action_dim units";
  for (int i = 0; i < num_layers; ++i) {
    if (layer_sizes[i] < 1 || layer_sizes[i] > TDS_NN_MAX_UNITS) return "layer size out of range (1..TDS_NN_MAX_UNITS)";
    if (i > 0 && (activations[i - 1] < TDS_NN_ACT_IDENTITY || activations[i - 1] > TDS_NN_ACT_SOFTSIGN))
      return "unknown activation";
    if (i > 0) nn->nw += layer_sizes[i - 1] * layer_sizes[i];
    nn->nb += use_bias[i] ? layer_sizes[i] : 0;
    nn->units[i] = layer_sizes[i];
    nn->bias[i] = use_bias[i] ? 1 : 0;
  }
  nn->n = num_layers;
  // (act[i - 1] belongs to layer i, as in the reference's activations_ vector)
  for (int i = 0; i < TDS_NN_MAX_LAYERS; ++i) nn->act[i] = i + 1 < num_layers ? activations[i] : TDS_NN_ACT_IDENTITY;
  return nullptr;
}

#if defined(__HIP_DEVICE_COMPILE__)
#define TDS_POLICY_LANES(l) for (int l = (int)threadIdx.x, once_ = 1; once_; once_ = 0)
#define TDS_POLICY_SYNC() __syncthreads()
#define TDS_POLICY_SLOT(l) 0
constexpr int kPolicyParts = 1;
#else
#define TDS_POLICY_LANES(l) for (int l = 0; l < 64; ++l)
#define TDS_POLICY_SYNC() ((void)0)
#define TDS_POLICY_SLOT(l) (l)
constexpr int kPolicyParts = 64;
#endif

// the xor butterfly over the lanes' partial sums: every lane gets the same sum
TDS_HD inline double tds_policy_tree(double *part) {
#if defined(__HIP_DEVICE_COMPILE__)
  double p = part[0];
  for (int d = 1; d < 64; d <<= 1) p += __shfl_xor(p, d, 64);
  return p;
#else
  double q[64];
  for (int d = 1; d < 64; d <<= 1) {
    for (int l = 0; l < 64; ++l) q[l] = part[l] + part[l ^ d];
    for (int l = 0; l < 64; ++l) part[l] = q[l];
  }
  return part[0];
#endif
}

// activation kind of v, and its derivative at v (a = the activation's value); ReLU and ELU: the primal's branch
TDS_HD inline double tds_policy_act(int kind, double v) {
  switch (kind) {
    case TDS_NN_ACT_TANH: return tanh(v);
    case TDS_NN_ACT_SIN: return sin(v);
    case TDS_NN_ACT_RELU: return v > 0.0 ? v : 0.0;
    case TDS_NN_ACT_SOFT_RELU: return log(1.0 + exp(v));
    case TDS_NN_ACT_ELU: return v >= 0.0 ? v : exp(v) - 1.0;
    case TDS_NN_ACT_SIGMOID: { const double e = exp(v); return e / (e + 1.0); }
    case TDS_NN_ACT_SOFTSIGN: return v / (1.0 + (v < 0.0 ? -v : v));
    default: return v;
  }
}
TDS_HD inline double tds_policy_dact(int kind, double v, double a) {
  switch (kind) {
    case TDS_NN_ACT_TANH: return 1.0 - a * a;
    case TDS_NN_ACT_SIN: return cos(v);
    case TDS_NN_ACT_RELU: return v > 0.0 ? 1.0 : 0.0;
    case TDS_NN_ACT_SOFT_RELU: { const double e = exp(v); return e / (1.0 + e); }
    case TDS_NN_ACT_ELU: return v >= 0.0 ? 1.0 : exp(v);
    case TDS_NN_ACT_SIGMOID: return a * (1.0 - a);
    case TDS_NN_ACT_SOFTSIGN: { const double b = 1.0 + (v < 0.0 ? -v : v); return 1.0 / (b * b); }
    default: return 1.0;
  }
}

// forward: a [layer][TDS_NN_MAX_UNITS] gets every layer's activations (layer 0: the masked observation plus the input
// layer's bias; layer n - 1: the actions), d (optional) the activations' derivatives of layers 1 ..  W: the
// environment's parameters, obs: its [q | qd], raw: obs[0], obs[1] as they are (else zero)
TDS_HD inline void tds_policy_forward(const TdsPolicyNet &nn, const double *W, const double *obs, int raw, double *a,
                                      double *d) {
  const double *const Bs = W + nn.nw;
  int wi = 0, bi = 0;
  TDS_POLICY_LANES(l) {
    for (int o = l; o < nn.units[0]; o += 64) {
      double v = (o < 2 && !raw) ? 0.0 : obs[o];
      if (nn.bias[0]) v += Bs[o];
      a[o] = v;
    }
  }
  if (nn.bias[0]) bi += nn.units[0];
  TDS_POLICY_SYNC();
  for (int i = 1; i < nn.n; ++i) {
    const int P = nn.units[i - 1], Cn = nn.units[i], kind = nn.act[i - 1];
    const double *const prev = a + (i - 1) * TDS_NN_MAX_UNITS;
    double *const out = a + i * TDS_NN_MAX_UNITS;
    for (int ci = 0; ci < Cn; ++ci) {
      double part[kPolicyParts];
      TDS_POLICY_LANES(l) {
        double acc = 0.0;
        for (int pi = l; pi < P; pi += 64) acc += prev[pi] * W[wi + ci * P + pi];
        part[TDS_POLICY_SLOT(l)] = acc;
      }
      const double v = tds_policy_tree(part) + (nn.bias[i] ? Bs[bi + ci] : 0.0);
      TDS_POLICY_LANES(l) {
        if (l == 0) out[ci] = v;
      }
    }
    TDS_POLICY_SYNC();
    TDS_POLICY_LANES(l) {
      for (int ci = l; ci < Cn; ci += 64) {
        const double v = out[ci], av = tds_policy_act(kind, v);
        out[ci] = av;
        if (d) d[i * TDS_NN_MAX_UNITS + ci] = tds_policy_dact(kind, v, av);
      }
    }
    wi += P * Cn;
    if (nn.bias[i]) bi += Cn;
    TDS_POLICY_SYNC();
  }
}

// backward at the activations a and derivatives d of tds_policy_forward: del0 [TDS_NN_MAX_UNITS] holds the cotangent on
// the actions; the parameters' gradients are ADDED into gP (the environment's, parameter order); returns the cotangent
// on layer 0's values (unmasked), in del0 or del1.  Lanes run over the previous layer's units: W and gP rows are read
// and written on consecutive addresses, the sum over a layer's units runs in ascending order
TDS_HD inline double *tds_policy_backward(const TdsPolicyNet &nn, const double *W, const double *a, const double *d,
                                          double *del0, double *del1, double *gP) {
  double *const gB = gP + nn.nw;
  double *del = del0, *deln = del1;
  int wi = nn.nw, bi = nn.nb;
  for (int i = nn.n - 1; i >= 1; --i) {
    const int P = nn.units[i - 1], Cn = nn.units[i];
    wi -= P * Cn;
    if (nn.bias[i]) bi -= Cn;
    TDS_POLICY_LANES(l) {
      for (int ci = l; ci < Cn; ci += 64) {
        const double g = del[ci] * d[i * TDS_NN_MAX_UNITS + ci];
        del[ci] = g;
        if (nn.bias[i]) gB[bi + ci] += g;
      }
    }
    TDS_POLICY_SYNC();
    TDS_POLICY_LANES(l) {
      for (int pi = l; pi < P; pi += 64) {
        const double ap = a[(i - 1) * TDS_NN_MAX_UNITS + pi];
        double acc = 0.0;
        for (int ci = 0; ci < Cn; ++ci) {
          const double g = del[ci];
          gP[wi + ci * P + pi] += g * ap;
          acc += W[wi + ci * P + pi] * g;
        }
        deln[pi] = acc;
      }
    }
    TDS_POLICY_SYNC();
    double *const sw = del;
    del = deln, deln = sw;
  }
  if (nn.bias[0]) {
    TDS_POLICY_LANES(l) {
      for (int o = l; o < nn.units[0]; o += 64) gB[o] += del[o];
    }
  }
  return del;
}

// one policy evaluation of a closed-loop trajectory (tds_traj_vjp.hip): environment env reads its observation at
// obs + env obs_stride and writes its actions to dst + env dst_stride and, where out is given, to out + env out_stride
struct TdsPolicyFwdArgs {
  const double *policy, *obs;
  double *dst, *out;
  long long obs_stride, dst_stride, out_stride;
  int n, raw;
};

// one backward evaluation: the cotangent on the actions is ubar + env ubar_stride (zeroed afterwards where zero_ubar)
// plus ga + env ga_stride (ga may be NULL); gpolicy [n][P] accumulates; the unmasked observation adjoint of entry o is
// added to lam[o lam_entry + env lam_env].  Environments e0 .. e0 + count - 1, those with bad[env] skipped
struct TdsPolicyBwdArgs {
  const double *policy, *obs, *ga;
  double *ubar, *gpolicy, *lam;
  const int *bad;
  long long obs_stride, ubar_stride, ga_stride, lam_entry, lam_env;
  int e0, count, raw, zero_ubar;
};

// launches of tds_policy_grad.hip on stream st (hipError_t as int)
int tds_policy_fwd_launch(void *st, const TdsPolicyNet &nn, const TdsPolicyFwdArgs &f);
int tds_policy_bwd_launch(void *st, const TdsPolicyNet &nn, const TdsPolicyBwdArgs &b);
// NaN into gpolicy of the environments with bad[env] or over[env]
int tds_policy_nan_launch(void *st, double *gpolicy, int P, const int *bad, const int *over, int n);
