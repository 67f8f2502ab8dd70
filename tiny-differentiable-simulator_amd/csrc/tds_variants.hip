// tds_variants.hip — per-environment model variants, the entry points that need no device: tds_hip_params_apply (the
// inverse of tds_hip_params_get) and tds_hip_model_variants_host (the checks of tds_hip_set_model_variants on the CPU).
// Host code only — no kernel, no HIP call — so that tools/variants_sanitize.cpp can compile this unit with the host
// sanitizers into a program of its own.  (The device entry point lives with the handle: tds_api.hip.)
#include "tds_variants_api.h"

using namespace tds_internal;

extern "C" {

int tds_hip_params_apply(const tds_model_t *model, int p, const tds_param_t *params, const double *theta,
                         tds_model_t *out_model) {
  if (!model || !out_model || (p > 0 && !theta)) return fail(TDS_ERR_INVALID_ARG, "tds_hip_params_apply: NULL argument%s");
  int rc = tds_variants_model_check(model);
  if (rc) return rc;
  const char *why = "";
  if (tds_param_check(model, p, params, &why)) return fail(TDS_ERR_INVALID_ARG, "%s", why);
  tds_param_apply(model, p, params, theta, out_model);
  return TDS_OK;
}

int tds_hip_model_variants_host(const tds_model_t *model, int dtype, int num_envs, int n_variants, int p,
                                const tds_param_t *params, const double *theta, const int32_t *env_variant,
                                int64_t *bytes) {
  if (!model || (p > 0 && !theta)) return fail(TDS_ERR_INVALID_ARG, "tds_hip_model_variants_host: NULL argument%s");
  if (dtype != TDS_DTYPE_F64 && dtype != TDS_DTYPE_F32 && dtype != TDS_DTYPE_F64_REC32) return fail(TDS_ERR_INVALID_ARG, "unknown dtype");
  if (num_envs <= 0) return fail(TDS_ERR_INVALID_ARG, "num_envs must be positive");
  int rc = tds_variants_prepare(model, num_envs, n_variants, p, params, env_variant);
  if (rc) return rc;
  char why[256];
  rc = dtype == TDS_DTYPE_F32 ? tds_build_variants<float>(model, n_variants, p, params, theta, nullptr, why, sizeof(why))
                              : tds_build_variants<double>(model, n_variants, p, params, theta, nullptr, why, sizeof(why));
  if (rc) return fail(rc, "%s", why);
  if (bytes) *bytes = (int64_t)n_variants * (int64_t)(dtype == TDS_DTYPE_F32 ? sizeof(DevModel<float>) : sizeof(DevModel<double>));
  return TDS_OK;
}

}  // extern "C"
