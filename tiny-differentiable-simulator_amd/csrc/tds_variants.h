// tds_variants.h — per-environment model variants, host side: applying a parameter selection to a blob, building the
// device models of V variants and checking that they share the base model's structure.  Host only, no HIP call: the
// device entry point (tds_api.hip: tds_hip_set_model_variants), its CPU twin (tds_variants.hip:
// tds_hip_model_variants_host) and tools/variants_sanitize.cpp all go through these functions.
//
// "The model of variant v" is tds_param_apply(blob, selection, theta_v) handed to tds_build_dev_model — every derived
// quantity (fixed-link folding, pseudo links of a floating base, the 8-lane kernel's table, ...) is rebuilt, nothing is
// patched in place.  The variant builds of the step kernel (tds_kernels.hip: VAR) read the fields of
// tds_variant_value_fields through the environment's own entry of the array and EVERYTHING ELSE through entry 0, so the
// check here is exactly that: outside those fields a variant's DevModel equals the base's byte for byte.
#pragma once
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "tds_device_model.h"
#include "tds_diff_step.h"

// selected entry q of the blob := t (the inverse of tds_param_value; an off-diagonal inertia entry sets its mirror too)
inline void tds_param_apply_one(tds_model_t *m, const tds_param_t &q, double t) {
  tds_link_t &l = m->links[q.kind <= TDS_PARAM_LINK_DAMPING ? q.link : 0];
  switch (q.kind) {
    case TDS_PARAM_LINK_MASS: l.mass = t; break;
    case TDS_PARAM_LINK_COM: l.com[q.comp] = t; break;
    case TDS_PARAM_LINK_INERTIA:
      l.inertia[tds_param_inertia_index(q.comp, 0)] = t;
      l.inertia[tds_param_inertia_index(q.comp, 1)] = t;
      break;
    case TDS_PARAM_LINK_XT_TRANS: l.X_T_trans[q.comp] = t; break;
    case TDS_PARAM_LINK_STIFFNESS: l.stiffness = t; break;
    case TDS_PARAM_LINK_DAMPING: l.damping = t; break;
    case TDS_PARAM_BASE_MASS: m->base_mass = t; break;
    case TDS_PARAM_BASE_COM: m->base_com[q.comp] = t; break;
    case TDS_PARAM_BASE_INERTIA:
      m->base_inertia[tds_param_inertia_index(q.comp, 0)] = t;
      m->base_inertia[tds_param_inertia_index(q.comp, 1)] = t;
      break;
    case TDS_PARAM_GRAVITY: m->gravity[q.comp] = t; break;
    case TDS_PARAM_FRICTION: m->friction = t; break;
    case TDS_PARAM_RESTITUTION: m->restitution = t; break;
    case TDS_PARAM_CFM: m->cfm = t; break;
    case TDS_PARAM_ERP: m->erp = t; break;
    case TDS_PARAM_GEOM_RADIUS: m->geoms[q.link].radius = t; break;
    case TDS_PARAM_GEOM_LENGTH: m->geoms[q.link].length = t; break;
    case TDS_PARAM_GEOM_EXTENT: m->geoms[q.link].extents[q.comp] = t; break;
    case TDS_PARAM_GEOM_TRANS: m->geoms[q.link].X_trans[q.comp] = t; break;
    default: break;  // (a checked selection has no other kind)
  }
}

// out := the blob with the (checked) selection set to theta [p]
inline void tds_param_apply(const tds_model_t *m, int p, const tds_param_t *params, const double *theta, tds_model_t *out) {
  if (out != m) memcpy(out, m, sizeof(*m));
  for (int j = 0; j < p; ++j) tds_param_apply_one(out, params[j], theta[j]);
}

struct TdsFieldSpan {
  const char *name;
  size_t off, len;
};
#define TDS_SPAN(f) {#f, offsetof(DevModel<T>, f), sizeof(((DevModel<T> *)nullptr)->f)}

// what a variant build reads through the environment's own entry — every field a parameter selection can reach: the
// selectable scalars themselves, and the contact points' / visuals' frames, which folding a fixed link re-bases through
// its X_T.  The contact model's parameters arrive as cfm, erp_over_dt (= erp / dt), cp_radius (a shape's radius; a
// box's clamped one) and cp_local (a shape's X_trans, a capsule's length, a box's extents and radius).
// (oct_tab and gravb are derived from them too; the general kernel's variant builds read neither.)
template <typename T>
inline const std::vector<TdsFieldSpan> &tds_variant_value_fields() {
  static const std::vector<TdsFieldSpan> v = {TDS_SPAN(friction),  TDS_SPAN(restitution), TDS_SPAN(grav),     TDS_SPAN(X_T),
                                              TDS_SPAN(mass),      TDS_SPAN(com),         TDS_SPAN(inertia),  TDS_SPAN(stiffness),
                                              TDS_SPAN(damping),   TDS_SPAN(cp_local),    TDS_SPAN(vis_X),    TDS_SPAN(oct_tab),
                                              TDS_SPAN(gravb),     TDS_SPAN(cfm),         TDS_SPAN(erp_over_dt), TDS_SPAN(cp_radius)};
  return v;
}
// the integer fields, by name (what the message of a refused variant names)
template <typename T>
inline const std::vector<TdsFieldSpan> &tds_variant_int_fields() {
  static const std::vector<TdsFieldSpan> v = {
      TDS_SPAN(num_links),    TDS_SPAN(dof_q),          TDS_SPAN(dof_qd),       TDS_SPAN(num_levels),  TDS_SPAN(num_cp),
      TDS_SPAN(num_visuals),  TDS_SPAN(action_dim),     TDS_SPAN(input_dim),    TDS_SPAN(output_dim),  TDS_SPAN(step_mode),
      TDS_SPAN(has_plane),    TDS_SPAN(pgs_iterations), TDS_SPAN(pack_visuals), TDS_SPAN(num_pairs),   TDS_SPAN(reward_mode),
      TDS_SPAN(settle_steps), TDS_SPAN(reset_obs_raw_xy), TDS_SPAN(is_floating), TDS_SPAN(nj),          TDS_SPAN(num_spherical),
      TDS_SPAN(q_rec),        TDS_SPAN(qd_rec),         TDS_SPAN(dof_rec),      TDS_SPAN(parent),      TDS_SPAN(level),
      TDS_SPAN(joint_type),   TDS_SPAN(q_index),        TDS_SPAN(qd_index),     TDS_SPAN(act_index),   TDS_SPAN(sph_q),
      TDS_SPAN(anc_dofs),     TDS_SPAN(chain_flags),    TDS_SPAN(lc_slot),      TDS_SPAN(num_lc_slots), TDS_SPAN(root_last),
      TDS_SPAN(kin_chain_last), TDS_SPAN(kin_lev0),     TDS_SPAN(euler_root),   TDS_SPAN(leg_len),     TDS_SPAN(dof_identity),
      TDS_SPAN(quad),         TDS_SPAN(oct),            TDS_SPAN(chain),        TDS_SPAN(dof_link),    TDS_SPAN(cp_link),
      TDS_SPAN(vis_link),     TDS_SPAN(pair_i),         TDS_SPAN(pair_j),       TDS_SPAN(num_bodies),  TDS_SPAN(body_dof0),
      TDS_SPAN(body_of_link), TDS_SPAN(num_bpairs),     TDS_SPAN(bpair_a),      TDS_SPAN(bpair_b),     TDS_SPAN(bpair_pc0),
      TDS_SPAN(multi_floating), TDS_SPAN(fb_k),         TDS_SPAN(fb_q),         TDS_SPAN(tau_rec),     TDS_SPAN(dof_body),
      TDS_SPAN(dof_joint0),   TDS_SPAN(dof_base0),      TDS_SPAN(dof_fbq),      TDS_SPAN(num_pc),      TDS_SPAN(pc_link_a),
      TDS_SPAN(pc_link_b),    TDS_SPAN(pc_swap)};
  return v;
}
#undef TDS_SPAN

// NULL: v has the base's structure; else the name of a field that differs (an integer field by its name)
template <typename T>
inline const char *tds_variant_structure_diff(const DevModel<T> &base, const DevModel<T> &v) {
  const unsigned char *a = (const unsigned char *)&base, *b = (const unsigned char *)&v;
  for (const TdsFieldSpan &f : tds_variant_int_fields<T>())
    if (memcmp(a + f.off, b + f.off, f.len) != 0) return f.name;
  // the rest outside the value fields: constants no selection reaches, which the kernel reads from entry 0 for all
  static const std::vector<unsigned char> shared = [] {
    std::vector<unsigned char> m(sizeof(DevModel<T>), 1);
    for (const TdsFieldSpan &f : tds_variant_value_fields<T>()) memset(m.data() + f.off, 0, f.len);
    return m;
  }();
  for (size_t i = 0; i < sizeof(DevModel<T>); ++i)
    if (shared[i] && a[i] != b[i]) return "a constant the variants share";
  return nullptr;
}

// the environment -> variant map of a handle of num_envs environments (NULL: identity, V == num_envs); 0 or why
inline int tds_variants_check_map(int num_envs, int n_variants, const int *env_variant, char *why, size_t cap) {
  if (n_variants < 1 || n_variants > num_envs) {
    snprintf(why, cap, "model variants: %d variants for %d environments (1 .. num_envs)", n_variants, num_envs);
    return TDS_ERR_INVALID_ARG;
  }
  if (!env_variant) {
    if (n_variants == num_envs) return TDS_OK;
    snprintf(why, cap, "model variants: no environment map given for %d variants of %d environments", n_variants, num_envs);
    return TDS_ERR_INVALID_ARG;
  }
  for (int e = 0; e < num_envs; ++e)
    if (env_variant[e] < 0 || env_variant[e] >= n_variants) {
      snprintf(why, cap, "model variants: environment %d maps to variant %d (0 .. %d)", e, env_variant[e], n_variants - 1);
      return TDS_ERR_INVALID_ARG;
    }
  return TDS_OK;
}

// the device models of the variants theta [V][p] of a (checked) model under a (checked) selection; out == NULL: the
// checks only.  A variant the builder refuses, or one whose structure differs from the base's, is
// TDS_ERR_INVALID_ARG with the variant and the field in `why`.
template <typename T>
inline int tds_build_variants(const tds_model_t *m, int n_variants, int p, const tds_param_t *params, const double *theta,
                              std::vector<DevModel<T>> *out, char *why, size_t cap) {
  std::vector<DevModel<T>> one(2);  // base | the variant at hand (heap: a DevModel is tens of KB)
  std::vector<tds_model_t> blob(1);
  char w[128];
  int rc = tds_build_dev_model<T>(m, &one[0], w);
  if (rc != TDS_OK) {
    snprintf(why, cap, "%s", w);
    return rc;
  }
  if (out) out->resize((size_t)n_variants);
  for (int v = 0; v < n_variants; ++v) {
    tds_param_apply(m, p, params, theta + (size_t)v * p, &blob[0]);
    DevModel<T> &d = out ? (*out)[(size_t)v] : one[1];
    rc = tds_build_dev_model<T>(&blob[0], &d, w);
    if (rc != TDS_OK) {
      snprintf(why, cap, "model variants: variant %d is refused: %s", v, w);
      return TDS_ERR_INVALID_ARG;
    }
    if (const char *field = tds_variant_structure_diff<T>(one[0], d)) {
      snprintf(why, cap, "model variants: variant %d differs from the base model in structure (field %s)", v, field);
      return TDS_ERR_INVALID_ARG;
    }
  }
  return TDS_OK;
}
