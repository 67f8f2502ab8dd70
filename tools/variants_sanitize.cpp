// variants_sanitize.cpp — the host side of the per-environment model variants as a program of its own, for the host
// sanitizers: tds_hip_params_apply and tds_hip_model_variants_host (csrc/tds_variants.hip, host code only) on a model
// blob read from a file.  No GPU, no Python.  Build and run (tests/test_variants_cpu.py does exactly this):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//     -Xarch_host -fno-sanitize-recover=undefined -Iinclude -Itiny-differentiable-simulator_amd/csrc \
//     tools/variants_sanitize.cpp tiny-differentiable-simulator_amd/csrc/tds_variants.hip -o variants_sanitize
//   python -c "import sys, ctypes, tds_amd; m = tds_amd.load_model('ant'); \
//              sys.stdout.buffer.write(ctypes.string_at(ctypes.byref(m), ctypes.sizeof(m)))" > ant.blob
//   ./variants_sanitize ant.blob
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "tds_api_internal.h"
#include "tds_variants.h"

// (the library defines the entry points' error text in tds_api.hip, which this program does not link)
namespace tds_internal {
thread_local char g_err[512] = "";
}

#define EXPECT(cond)                                                                                   \
  do {                                                                                                 \
    if (!(cond)) {                                                                                     \
      fprintf(stderr, "variants_sanitize: line %d: %s  [%s]\n", __LINE__, #cond, tds_internal::g_err); \
      return 1;                                                                                        \
    }                                                                                                  \
  } while (0)

int main(int argc, char **argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s <model blob>\n", argv[0]);
    return 2;
  }
  std::vector<tds_model_t> m(3);  // the blob | an applied copy | scratch
  FILE *f = fopen(argv[1], "rb");
  EXPECT(f != nullptr);
  const size_t got = fread(&m[0], 1, sizeof(tds_model_t), f);
  fclose(f);
  EXPECT(got == sizeof(tds_model_t));
  EXPECT(m[0].num_links > 12);  // (the Ant: root chain 0..5, four legs of two links)

  const tds_param_t sel[] = {{TDS_PARAM_LINK_MASS, 7, 0, 0},      {TDS_PARAM_LINK_COM, 8, 1, 0},
                             {TDS_PARAM_LINK_INERTIA, 9, 3, 0},   {TDS_PARAM_LINK_XT_TRANS, 10, 0, 0},
                             {TDS_PARAM_LINK_STIFFNESS, 11, 0, 0}, {TDS_PARAM_LINK_DAMPING, 12, 0, 0},
                             {TDS_PARAM_GRAVITY, 0, 2, 0},        {TDS_PARAM_FRICTION, 0, 0, 0},
                             {TDS_PARAM_RESTITUTION, 0, 0, 0}};
  const int p = (int)(sizeof(sel) / sizeof(sel[0]));
  std::vector<double> base((size_t)p);
  for (int j = 0; j < p; ++j) base[(size_t)j] = tds_param_value(&m[0], sel[j]);

  // ---- apply: round trip, mirror entry, in place, refusals
  std::vector<double> th = base;
  for (int j = 0; j < p; ++j) th[(size_t)j] = base[(size_t)j] * 1.05 + (sel[j].kind == TDS_PARAM_LINK_INERTIA ? 0.0 : 0.01);
  EXPECT(tds_hip_params_apply(&m[0], p, sel, th.data(), &m[1]) == TDS_OK);
  for (int j = 0; j < p; ++j) EXPECT(tds_param_value(&m[1], sel[j]) == th[(size_t)j]);
  EXPECT(m[1].links[9].inertia[1] == m[1].links[9].inertia[3]);
  EXPECT(tds_hip_params_apply(&m[1], p, sel, base.data(), &m[1]) == TDS_OK);  // in place, back to the blob
  EXPECT(memcmp(&m[0], &m[1], sizeof(tds_model_t)) == 0);
  EXPECT(tds_hip_params_apply(&m[0], 0, nullptr, nullptr, &m[2]) == TDS_OK);
  const tds_param_t bad_kind = {12, 0, 0, 0}, bad_link = {TDS_PARAM_LINK_MASS, 14, 0, 0};
  EXPECT(tds_hip_params_apply(&m[0], 1, &bad_kind, th.data(), &m[2]) == TDS_ERR_INVALID_ARG);
  EXPECT(tds_hip_params_apply(&m[0], 1, &bad_link, th.data(), &m[2]) == TDS_ERR_INVALID_ARG);
  EXPECT(tds_hip_params_apply(nullptr, p, sel, th.data(), &m[2]) == TDS_ERR_INVALID_ARG);

  // ---- variants: V = 1, 3, N; both scalar types; maps; a structure-changing variant
  const int n = 70;
  std::vector<int32_t> map((size_t)n);
  for (int V : {1, 3, n}) {
    std::vector<double> theta((size_t)V * p);
    for (int v = 0; v < V; ++v)
      for (int j = 0; j < p; ++j) theta[(size_t)v * p + j] = base[(size_t)j] * (1.0 + 0.04 * ((v * 7 + j * 3) % 11 - 5) / 5.0);
    for (int e = 0; e < n; ++e) map[(size_t)e] = (e * 5 + 1) % V;
    int64_t b64 = 0, b32 = 0;
    EXPECT(tds_hip_model_variants_host(&m[0], TDS_DTYPE_F64, n, V, p, sel, theta.data(), map.data(), &b64) == TDS_OK);
    EXPECT(tds_hip_model_variants_host(&m[0], TDS_DTYPE_F32, n, V, p, sel, theta.data(), map.data(), &b32) == TDS_OK);
    EXPECT(b64 == (int64_t)V * (int64_t)sizeof(DevModel<double>) && b32 == (int64_t)V * (int64_t)sizeof(DevModel<float>));
    EXPECT(tds_hip_model_variants_host(&m[0], TDS_DTYPE_F64_REC32, n, V, p, sel, theta.data(), V == n ? nullptr : map.data(),
                                       nullptr) == TDS_OK);
    if (V > 1) {
      map[(size_t)(n - 1)] = V;  // one past the last variant
      EXPECT(tds_hip_model_variants_host(&m[0], TDS_DTYPE_F64, n, V, p, sel, theta.data(), map.data(), nullptr) ==
             TDS_ERR_INVALID_ARG);
    }
    if (V != n)
      EXPECT(tds_hip_model_variants_host(&m[0], TDS_DTYPE_F64, n, V, p, sel, theta.data(), nullptr, nullptr) ==
             TDS_ERR_INVALID_ARG);
  }
  {
    std::vector<double> theta((size_t)(n + 1) * p, 1.0);
    EXPECT(tds_hip_model_variants_host(&m[0], TDS_DTYPE_F64, n, n + 1, p, sel, theta.data(), map.data(), nullptr) ==
           TDS_ERR_INVALID_ARG);
  }
  {
    const tds_param_t root_mass = {TDS_PARAM_LINK_MASS, 2, 0, 0};  // a mass on a massless link of the root chain
    const double theta[2] = {0.0, 0.25};
    for (int e = 0; e < n; ++e) map[(size_t)e] = e % 2;
    EXPECT(tds_hip_model_variants_host(&m[0], TDS_DTYPE_F64, n, 2, 1, &root_mass, theta, map.data(), nullptr) ==
           TDS_ERR_INVALID_ARG);
    EXPECT(strstr(tds_internal::g_err, "variant 1") != nullptr && strstr(tds_internal::g_err, "root_last") != nullptr);
  }
  // ---- the contact model's kinds: one applied variant each (the Ant: geom 0 the torso's sphere, 1.. the legs' capsules;
  //      the extent on a copy whose torso is a box and which keeps one leg's capsule beside it)
  {
    EXPECT(m[0].num_geoms > 1 && m[0].geoms[0].type == TDS_GEOM_SPHERE && m[0].geoms[1].type == TDS_GEOM_CAPSULE);
    const tds_param_t csel[] = {{TDS_PARAM_CFM, 0, 0, 0},         {TDS_PARAM_ERP, 0, 0, 0},
                                {TDS_PARAM_GEOM_RADIUS, 0, 0, 0}, {TDS_PARAM_GEOM_LENGTH, 1, 0, 0},
                                {TDS_PARAM_GEOM_TRANS, 1, 2, 0},  {TDS_PARAM_GEOM_EXTENT, 0, 1, 0}};
    const double cth[] = {1e-3, 0.3, 0.3, 0.5, 0.05, 0.4};
    for (int e = 0; e < n; ++e) map[(size_t)e] = e % 2;
    for (int j = 0; j < 6; ++j) {
      memcpy(&m[2], &m[0], sizeof(tds_model_t));
      if (csel[j].kind == TDS_PARAM_GEOM_EXTENT) {
        EXPECT(tds_hip_params_apply(&m[2], 1, &csel[j], &cth[j], &m[1]) == TDS_ERR_INVALID_ARG);  // an extent of a sphere
        m[2].geoms[0].type = TDS_GEOM_BOX;
        m[2].num_geoms = 2;  // (the box's 8 points and one leg's 2: within the 17 of the Ant's class)
        for (int k = 0; k < 3; ++k) m[2].geoms[0].extents[k] = 0.5;
      }
      const double theta[2] = {tds_param_value(&m[2], csel[j]), cth[j]};
      EXPECT(tds_hip_params_apply(&m[2], 1, &csel[j], &cth[j], &m[1]) == TDS_OK);
      EXPECT(tds_param_value(&m[1], csel[j]) == cth[j]);
      EXPECT(tds_hip_params_apply(&m[1], 1, &csel[j], &theta[0], &m[1]) == TDS_OK);
      EXPECT(memcmp(&m[2], &m[1], sizeof(tds_model_t)) == 0);
      EXPECT(tds_hip_model_variants_host(&m[2], TDS_DTYPE_F64, n, 2, 1, &csel[j], theta, map.data(), nullptr) == TDS_OK);
      EXPECT(tds_hip_model_variants_host(&m[2], TDS_DTYPE_F32, n, 2, 1, &csel[j], theta, map.data(), nullptr) == TDS_OK);
    }
    const tds_param_t bad_geom = {TDS_PARAM_GEOM_RADIUS, m[0].num_geoms, 0, 0}, bad_len = {TDS_PARAM_GEOM_LENGTH, 0, 0, 0},
                      bad_comp = {TDS_PARAM_GEOM_TRANS, 1, 3, 0}, dup[2] = {csel[0], csel[0]};
    EXPECT(tds_hip_params_apply(&m[0], 1, &bad_geom, cth, &m[1]) == TDS_ERR_INVALID_ARG);
    EXPECT(tds_hip_params_apply(&m[0], 1, &bad_len, cth, &m[1]) == TDS_ERR_INVALID_ARG);
    EXPECT(tds_hip_params_apply(&m[0], 1, &bad_comp, cth, &m[1]) == TDS_ERR_INVALID_ARG);
    EXPECT(tds_hip_params_apply(&m[0], 2, dup, cth, &m[1]) == TDS_ERR_INVALID_ARG);
    for (int kind = 12; kind < 16; ++kind) {
      const tds_param_t unknown = {kind, 0, 0, 0};
      EXPECT(tds_hip_params_apply(&m[0], 1, &unknown, cth, &m[1]) == TDS_ERR_INVALID_ARG);
    }
  }
  printf("variants_sanitize: ok (device model: %zu B double, %zu B float)\n", sizeof(DevModel<double>), sizeof(DevModel<float>));
  return 0;
}
