// tds_variants_api.h — the checks tds_hip_set_model_variants (tds_api.hip) and tds_hip_model_variants_host
// (tds_variants.hip) share, in the entry points' error convention (tds_internal::fail).
#pragma once
#include <new>

#include "tds_diff_classes.h"
#include "tds_variants.h"

namespace tds_internal {

// what tds_hip_model_check checks, stated here so that tds_variants.hip links without tds_api.hip
inline int tds_variants_model_check(const tds_model_t *model) {
  DevModel<double> *d = new (std::nothrow) DevModel<double>;
  if (!d) return fail(TDS_ERR_INVALID_ARG, "out of host memory");
  char why[128];
  const int rc = tds_build_dev_model<double>(model, d, why);
  delete d;
  if (rc != TDS_OK) return fail(rc, "%s", why);
  if (model->num_links > 64) return fail(TDS_ERR_UNSUPPORTED, "more than 64 links");
  return TDS_OK;
}

// model (the classes of the parameter derivatives: spherical joints and worlds of several bodies are refused with their
// message), selection, environment map
inline int tds_variants_prepare(const tds_model_t *model, int num_envs, int n_variants, int p, const tds_param_t *params,
                                const int *env_variant) {
  const char *why = "";
  if (tds_jvp_pick(model, &why) < 0) return fail(TDS_ERR_UNSUPPORTED, "%s", why);
  int rc = tds_variants_model_check(model);
  if (rc) return rc;
  if (tds_param_check(model, p, params, &why)) return fail(TDS_ERR_INVALID_ARG, "%s", why);
  char w[256];
  if ((rc = tds_variants_check_map(num_envs, n_variants, env_variant, w, sizeof(w)))) return fail(rc, "%s", w);
  return TDS_OK;
}

}  // namespace tds_internal
