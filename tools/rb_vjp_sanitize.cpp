// rb_vjp_sanitize.cpp — the host side of the rigid-body reverse mode as a program of its own, for the host sanitizers:
// tds_rb_vjp_host and tds_rb_vjp_plan (csrc/tds_rb_vjp.hip, host code only) on the tumbling scene (a plane and five
// spheres, tests/test_rigid_bodies.py's make_worlds) and the billiard scene (tests/rb_scenes.py), once with the default
// tape capacity and once with an overflowing one.  No GPU, no Python.  Build and run (tests/test_rb_vjp_cpu.py does
// exactly this):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//     -Xarch_host -fno-sanitize-recover=undefined -Iinclude -Itiny-differentiable-simulator_amd/csrc \
//     tools/rb_vjp_sanitize.cpp tiny-differentiable-simulator_amd/csrc/tds_rb_vjp.hip -o rb_vjp_sanitize
//   ./rb_vjp_sanitize
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "tds_hip.h"

// (the library defines the error texts in tds_api.hip and tds_rb.hip, which this program does not link)
namespace tds_internal {
thread_local char g_err[512] = "";
}
static char g_rb_err[512] = "";
int tds_rb_fail(int code, const char *msg) {
  snprintf(g_rb_err, sizeof(g_rb_err), "%s", msg);
  return code;
}

#define EXPECT(cond)                                                                     \
  do {                                                                                   \
    if (!(cond)) {                                                                       \
      fprintf(stderr, "rb_vjp_sanitize: line %d: %s  [%s]\n", __LINE__, #cond, g_rb_err); \
      return 1;                                                                          \
    }                                                                                    \
  } while (0)

static unsigned long long g_seed = 88172645463325252ull;
static double uniform(double lo, double hi) {  // xorshift64
  g_seed ^= g_seed << 13, g_seed ^= g_seed >> 7, g_seed ^= g_seed << 17;
  return lo + (hi - lo) * (double)(g_seed >> 11) / 9007199254740992.0;
}

static tds_rb_model_t model(int nb, double dt, int iters, double gz, double friction, double restitution) {
  tds_rb_model_t m;
  memset(&m, 0, sizeof(m));
  m.abi_version = TDS_HIP_ABI_VERSION, m.num_bodies = nb, m.solver_iterations = iters, m.dt = dt;
  m.gravity[2] = gz, m.restitution = restitution, m.friction = friction, m.erp = 0.1;
  return m;
}

// runs one scene: default capacity (finite gradients, theta's included), then `small` (NaN gradients, the error)
static int run(const tds_rb_model_t &m, int n, int steps, int every, const std::vector<double> &s0, int p,
               const tds_param_t *sel, int small) {
  const int ns = m.num_bodies * TDS_RB_STATE, n_rec = steps / every;
  std::vector<double> th((size_t)n * p), gs((size_t)n * n_rec * ns), s((size_t)n * n_rec * ns), g0((size_t)n * ns),
      gt((size_t)n * p);
  EXPECT(tds_rb_params_get(&m, p, sel, th.data()) == TDS_OK);
  for (int w = 1; w < n; ++w)
    for (int j = 0; j < p; ++j) th[(size_t)w * p + j] = th[j] * (1.0 + 0.01 * w);
  for (double &g : gs) g = uniform(-1, 1);
  long long plan[4];
  EXPECT(tds_rb_vjp_plan(&m, n, steps, p, 0, 0, plan) == TDS_OK && plan[0] > 0 && plan[1] == 64 && plan[2] >= 1 &&
         plan[2] <= steps);
  EXPECT(tds_rb_vjp_host(&m, n, steps, every, s0.data(), p, sel, th.data(), gs.data(), s.data(), g0.data(), gt.data(),
                         0) == TDS_OK);
  double top = 0.0;
  for (double g : g0) {
    EXPECT(isfinite(g));
    top = fmax(top, fabs(g));
  }
  for (double g : gt) EXPECT(isfinite(g));
  EXPECT(top > 0.0);
  // outputs not wanted
  EXPECT(tds_rb_vjp_host(&m, n, steps, every, s0.data(), p, sel, nullptr, gs.data(), nullptr, nullptr, gt.data(), 0) ==
         TDS_OK);
  EXPECT(tds_rb_vjp_host(&m, n, steps, every, s0.data(), 0, nullptr, nullptr, gs.data(), nullptr, g0.data(), nullptr,
                         0) == TDS_OK);
  // an overflowing capacity
  EXPECT(tds_rb_vjp_host(&m, n, steps, every, s0.data(), p, sel, th.data(), gs.data(), s.data(), g0.data(), gt.data(),
                         small) == TDS_ERR_UNSUPPORTED);
  EXPECT(strstr(g_rb_err, "tape exceeds the capacity") != nullptr);
  for (double g : g0) EXPECT(isnan(g));
  for (double g : gt) EXPECT(isnan(g));
  for (double x : s) EXPECT(isfinite(x));
  return 0;
}

// tds_rb_params_get lives in tds_rb_diff.hip, which this program does not link: the model's values of a selection
int tds_rb_params_get(const tds_rb_model_t *m, int p, const tds_param_t *sel, double *theta) {
  for (int j = 0; j < p; ++j)
    theta[j] = sel[j].kind == TDS_PARAM_LINK_MASS  ? m->bodies[sel[j].link].mass
               : sel[j].kind == TDS_PARAM_GRAVITY  ? m->gravity[sel[j].comp]
               : sel[j].kind == TDS_PARAM_FRICTION ? m->friction
                                                   : m->restitution;
  return TDS_OK;
}

int main() {
  {  // tumbling: a plane and five spheres
    const int n = 3, nb = 6;
    tds_rb_model_t m = model(nb, 1.0 / 60.0, 4, -9.81, 0.6, 0.2);
    m.bodies[0].geom_type = TDS_GEOM_PLANE, m.bodies[0].plane_normal[2] = 1.0;
    const double mass[5] = {0.5, 1.0, 1.5, 2.0, 0.8}, rad[5] = {0.10, 0.15, 0.20, 0.25, 0.12};
    for (int b = 1; b < nb; ++b)
      m.bodies[b].geom_type = TDS_GEOM_SPHERE, m.bodies[b].mass = mass[b - 1], m.bodies[b].radius = rad[b - 1];
    std::vector<double> s0((size_t)n * nb * TDS_RB_STATE, 0.0);
    for (int w = 0; w < n; ++w)
      for (int b = 0; b < nb; ++b) {
        double *x = &s0[((size_t)w * nb + b) * TDS_RB_STATE];
        x[6] = 1.0;
        if (b == 0) continue;
        x[0] = uniform(-0.4, 0.4), x[1] = uniform(-0.4, 0.4), x[2] = uniform(0.1, 0.8);
        for (int k = 0; k < 3; ++k) x[7 + k] = uniform(-1, 1), x[10 + k] = uniform(-2, 2);
      }
    const tds_param_t sel[] = {{TDS_PARAM_LINK_MASS, 2, 0, 0}, {TDS_PARAM_GRAVITY, 0, 2, 0},
                               {TDS_PARAM_FRICTION, 0, 0, 0}, {TDS_PARAM_RESTITUTION, 0, 0, 0}};
    if (run(m, n, 12, 1, s0, 4, sel, 100)) return 1;
    if (run(m, n, 12, 4, s0, 4, sel, 1)) return 1;
  }
  {  // billiards: six balls in the rack, the white ball shot at them
    const int n = 2, nb = 7;
    tds_rb_model_t m = model(nb, 1.0 / 60.0, 50, 0.0, 0.5, 0.0);
    for (int b = 0; b < nb; ++b) m.bodies[b].geom_type = TDS_GEOM_SPHERE, m.bodies[b].mass = 1.0, m.bodies[b].radius = 0.5;
    const double dx = cos(M_PI / 3), dy = sin(M_PI / 3);
    double pos[7][2];
    int k = 0;
    double rx = 0.0, y = 0.0;
    for (int column = 1; column <= 3; ++column, rx -= dx, y += dy)
      for (int i = 0; i < column; ++i, ++k) pos[k][0] = rx + i, pos[k][1] = y;
    pos[6][0] = 0.0, pos[6][1] = -2.0;
    std::vector<double> s0((size_t)n * nb * TDS_RB_STATE, 0.0);
    for (int w = 0; w < n; ++w)
      for (int b = 0; b < nb; ++b) {
        double *x = &s0[((size_t)w * nb + b) * TDS_RB_STATE];
        x[0] = pos[b][0], x[1] = pos[b][1], x[6] = 1.0;
        if (b == 6) x[7] = (10.0 - 30.0 * w) / 60.0, x[8] = 600.0 / 60.0;
      }
    const tds_param_t sel[] = {{TDS_PARAM_LINK_MASS, 6, 0, 0}, {TDS_PARAM_FRICTION, 0, 0, 0}};
    if (run(m, n, 30, 30, s0, 2, sel, 1000)) return 1;
  }
  printf("rb_vjp_sanitize: ok\n");
  return 0;
}
