// tds_launch_plan.h — which step kernel, and which build of it, a launch takes.  The one place that decides it: launch(),
// step_many, the exchange's workgroup count and the shard layer's ring form all read tds_launch_plan, and
// tds_hip_launch_plan_host asks the same function on the CPU.  Host only: it reads the handle's facts and makes no HIP call.
#pragma once
#include "tds_api_internal.h"

// the step kernels (the numbers tds_hip_single_step_kernel reports)
enum TdsKernel { TDS_KERNEL_GENERAL = 0, TDS_KERNEL_QUAD16 = 1, TDS_KERNEL_OCT8 = 2, TDS_KERNEL_CHAIN8 = 3 };
// the general kernel's LDS layouts: tds_hip_sim::lds / lds_w2 / pool_lds
enum TdsLayout { TDS_LAYOUT_LDS = 0, TDS_LAYOUT_W2 = 1, TDS_LAYOUT_POOL = 2 };

// what a launch brings
struct TdsLaunchReq {
  int n = 0;                  // environments in this launch
  int env_total = 0;          // environments resident at the same time (0: n)
  int nsub = 1;               // steps (0: a pure reset launch)
  int reset_mode = TDS_RESET_NONE;
  bool rollout = false;       // policy rollout
  bool rings = false;         // per-step record rings (a step-loop launch)
  bool progress = false;      // ... whose slots carry progress counters
  bool peers = false;         // ... whose records are stored to the peers (peer-store exchange)
  bool pool_states = false;   // done environments take their next state from the reset pool
  bool pool_pass = false;     // a refill pass of the reset pool: its own layout (pool_lds), on the pool stream
  int prof = 0;               // phase stamps: 0 none, 1 room for one wavefront's, 2 room for the two-wavefront form's
};

// what it gets
struct TdsLaunchPlan {
  int kernel;          // TdsKernel
  int kind;            // general kernel: 0 plain, 1 floating base, 2 spherical joints, 3 / 4 worlds of several bodies
  int build;           // the chosen kernel's build — general: gen_build; quad16: wavefronts per workgroup of its step loop (1 or
                       // TDS_QUAD_WIDE_WAVES); oct8: TDS_OCT_*; chain8: TDS_CHAIN_* (the straight-line forms ignore it)
  int gen_build;       // the general kernel's build: TDS_FORM_W2 | TDS_FORM_LOOP_OCC* (what an experiment slot receives)
  int layout;          // TdsLayout of the general kernel
  int envs_per_wg, threads_per_wg, blocks;
  bool refused;        // option loop_occ = 1 asks for a build that does not exist for this launch
  // a request over the handle's environments (step_many):
  bool loop;           // one step-loop launch rather than chained graphs of single steps
  int env_range;       // > 0: the 8-lane kernel's call runs as environment ranges of this size, one after the other
  bool exchange_after; // a ring launch with progress counters: exchange its slots after it completes, without counters
};

inline TdsLaunchPlan tds_launch_plan(const tds_hip_sim &s, const TdsLaunchReq &r) {
  const TdsOptions &o = s.opt;
  const bool c64 = s.compute_f64();
  // Per-environment model variants installed (tds_hip_set_model_variants) are a fact of the handle like option oct = 0:
  // the own kernels are tuned around ONE constant table per workgroup and decline, the general kernel's variant builds
  // exist as one-wavefront workgroups only — the one-wave layout, never the two-wavefront form.
  const bool variants = s.n_variants > 0;
  // (the own kernels of the star-shaped robots and the serial chains exist for double arithmetic only)
  const int quad = (c64 && !variants) ? s.h64.quad : 0, oct = (c64 && !variants) ? s.h64.oct : 0;
  const int chain = (c64 && !variants) ? s.h64.chain : 0;
  const bool floating = c64 ? s.h64.is_floating : s.h32.is_floating;
  const bool spherical = (c64 ? s.h64.num_spherical : s.h32.num_spherical) != 0;
  const bool two = (c64 ? s.h64.num_bodies : s.h32.num_bodies) >= 2;
  const bool multi_floating = (c64 ? s.h64.multi_floating : s.h32.multi_floating) != 0;
  const int ncp = c64 ? s.h64.num_cp : s.h32.num_cp;
  const int in_dim = s.model.input_dim;
  const int n_res = r.env_total > 0 ? r.env_total : r.n;
  const bool one_step = r.nsub == 1 && !r.rings;  // (the kernels' straight-line form)
  TdsLaunchPlan p = {};

  // ---- the general kernel ----
  // two-wavefront workgroups: launches whose whole grid is resident at once (the helper wavefront then fills issue slots
  // that would otherwise idle; beyond that the one-wave form with more workgroups per CU wins) — straight-line launches,
  // and step-loop launches of plain steps, where the helper wavefront loops along and is also the RECORDER of per-step
  // rings (option loop_w2 = 0: the one-wave loop build; = 2: not for launches that take reset states from the pool).
  // A launch whose ring slots are exchanged while it runs (progress counters) takes the SAME two-wavefront build an N = 1
  // launch takes (round 4: every rank of an N > 1 run executes the N = 1 kernel); round 3 dropped such launches to the
  // one-wave loop build — two wavefronts of 256 registers per SIMD leave no register for the exchange's kernels
  // (profiles/r03_ring_exchange_forms.txt) — at 13 % of the step rate (profiles/r04_same_box_ab_and_exchange_forms.txt:
  // two-wavefront build + 256-step launches 14.9 us per step, one-wave build 18.6).  Option exchange_w2 = 0 brings the
  // one-wave build back (bench.py times both forms in its warm-up at N > 1 and keeps the faster one on every rank).
  // Phase stamps: the two-wavefront form only where the caller has room for its stamps.
  const int epw = 64 / s.lanes;
  const long long loop_w2 = o.get(TDS_OPT_LOOP_W2, 1);
  const bool w2_fits = s.w2_max_blocks > 0 && (n_res + epw - 1) / epw <= s.w2_max_blocks && r.reset_mode == TDS_RESET_NONE &&
                       !r.rollout && !r.pool_pass && r.prof != 1 && !variants;
  const bool is_loop = r.nsub > 1 || r.rings;
  const bool exchanged = r.progress && o.get(TDS_OPT_EXCHANGE_W2, 1) == 0;
  const bool two_waves = w2_fits && (!is_loop || (loop_w2 != 0 && !exchanged && (loop_w2 != 2 || !r.pool_states) &&
                                                  s.lds_w2.NDP <= 16));
  const long long occ = r.prof ? 0 : o.get(TDS_OPT_LOOP_OCC, 0);
  p.gen_build = (two_waves ? TDS_FORM_W2 : 0) | (occ == 1 ? TDS_FORM_LOOP_OCC1 : (occ == 2 ? TDS_FORM_LOOP_OCC2 : 0));
  p.layout = r.pool_pass ? TDS_LAYOUT_POOL : (two_waves ? TDS_LAYOUT_W2 : TDS_LAYOUT_LDS);
  p.kind = floating ? 1 : (spherical ? 2 : (two ? (multi_floating ? 4 : 3) : 0));
  // (the one-wavefront-per-SIMD compilation of the step loop does not exist below 24 padded dof: built without
  //  MachineLICM its <double, double, 16, 8> instantiation never terminated — profiles/r04_diag_loop_hang.txt — and the
  //  two-wavefront compilation holds no scratch there; at 14 - 18 dof it paid for the Ant and Laikago at small batches,
  //  which run in kernels of their own since rounds 5 / 6; asked for by option, the launch is refused instead of
  //  falling back silently)
  const TdsLds &L = p.layout == TDS_LAYOUT_POOL ? s.pool_lds : (two_waves ? s.lds_w2 : s.lds);
  p.refused = occ == 1 && L.NDP < 24 && !two_waves && (r.nsub != 1 || r.reset_mode != TDS_RESET_NONE || r.rollout || r.rings);

  // ---- the 16-lane kernel (tds_quad.hip): its step-loop form's wavefronts per workgroup ----
  // 1: one wavefront per workgroup (resident up to six workgroups per compute unit: the constant table costs LDS);
  // TDS_QUAD_WIDE_WAVES: that many wavefronts around one table, a workgroup per compute unit (resident up to 32
  // environments per compute unit: laikago_soft x 8192); 0: neither form has every workgroup resident
  int quad_waves = 0;
  if (quad) {
    const int per_cu = (int)(s.lds_per_cu / (size_t)tds_quad_loop_workgroup_bytes(in_dim, 1));
    const long long wide = o.get(TDS_OPT_QUAD_WIDE, 1);  // 0: never, 1: where the narrow form is not resident, 2: always
    const bool wide_fits = (size_t)tds_quad_loop_workgroup_bytes(in_dim, TDS_QUAD_WIDE_WAVES) <= s.lds_per_cu &&
                           (n_res + 4 * TDS_QUAD_WIDE_WAVES - 1) / (4 * TDS_QUAD_WIDE_WAVES) <= s.num_cus;
    if (wide == 2 && wide_fits) quad_waves = TDS_QUAD_WIDE_WAVES;
    else if ((n_res + 3) / 4 <= s.num_cus * (per_cu < 8 ? per_cu : 8)) quad_waves = 1;
    else quad_waves = (wide != 0 && wide_fits) ? TDS_QUAD_WIDE_WAVES : 0;
  }

  // ---- which kernel ----
  // The own kernels take plain steps — one per launch, or K of them with action replay, record rings and reset-pool
  // entries taken in the loop —: no in-kernel reset, no policy, no phase stamps; the 8-lane kernels the exchange
  // launches of the multi-GPU layer (progress counters / peer stores) as well, the 16-lane kernel not.
  const bool plain_steps = !r.prof && r.nsub >= 1 && r.reset_mode == TDS_RESET_NONE && !r.rollout;
  const int oct_per_cu = oct ? (int)(s.lds_per_cu / (size_t)tds_oct_workgroup_bytes(in_dim)) : 0;
  const long long o2 = o.get(TDS_OPT_OCT_W2, 1);
  if (quad && plain_steps && !r.progress && !r.peers) {
    p.kernel = TDS_KERNEL_QUAD16;
    p.build = quad_waves > 1 ? TDS_QUAD_WIDE_WAVES : 1;
    const bool wide = !one_step && p.build > 1;
    p.envs_per_wg = wide ? 4 * TDS_QUAD_WIDE_WAVES : 4;
    p.threads_per_wg = wide ? 64 * TDS_QUAD_WIDE_WAVES : 64;
  } else if (oct && plain_steps) {
    // its two-wavefront build while every workgroup of the launch is resident with at most two wavefronts per SIMD — four
    // workgroups per compute unit, LDS permitting (Ant: up to 8192 environments); two workgroups per compute unit = one
    // wavefront per SIMD: the build compiled for that (no register limit to spill at).  Option oct_w2 = 3: the
    // two-wavefronts-per-SIMD compilation at any grid size — 256 registers, so that OTHER launches fit beside it on a SIMD:
    // the reset pool's refill passes, see pool_step_many.
    const int blocks = (n_res + 7) / 8;
    p.kernel = TDS_KERNEL_OCT8;
    p.build = TDS_OCT_W1;
    if (o2 != 0 && o2 != 3 && oct_per_cu >= 2 && blocks <= 2 * s.num_cus) p.build = TDS_OCT_W2_OCC1;
    else if (o2 == 2 || o2 == 3 || (o2 != 0 && blocks <= s.num_cus * (oct_per_cu < 4 ? oct_per_cu : 4))) p.build = TDS_OCT_W2;
    // a refill pass of the reset pool while the handle's own chunks are of the one-wavefront-per-SIMD build: the
    // 240-register build, so that the pass runs BESIDE the chunk it was issued next to instead of in its tail
    if (r.pool_pass && o2 != 0 && o2 != 3 && oct_per_cu >= 4 && (s.num_envs + 7) / 8 <= 2 * s.num_cus &&
        o.get(TDS_OPT_POOL_BESIDE, 1) != 0)
      p.build = TDS_OCT_BESIDE;
    p.envs_per_wg = 8;
    p.threads_per_wg = p.build >= TDS_OCT_W2 ? 128 : 64;
  } else if (chain && plain_steps) {
    // the recorder wavefront: step-loop launches that store per-step records, while the launch is resident with at most
    // two wavefronts per SIMD; with the links' constants in registers while it puts at most ONE wavefront on a SIMD
    // (that build holds 276 registers).  Option chain_w2 = 0 / 2: no recorder / a recorder at any grid size.
    const long long cw2 = o.get(TDS_OPT_CHAIN_W2, 1);
    const int blocks = (r.n + 7) / 8, simds = 4 * s.num_cus;
    const bool recorder = r.rings && cw2 != 0 && (blocks <= simds || cw2 == 2);
    p.kernel = TDS_KERNEL_CHAIN8;
    p.build = !recorder ? TDS_CHAIN_W1 : (2 * blocks <= simds ? TDS_CHAIN_W2_CREG : TDS_CHAIN_W2);
    p.envs_per_wg = 8;
    p.threads_per_wg = p.build != TDS_CHAIN_W1 ? 128 : 64;
  } else {
    p.kernel = TDS_KERNEL_GENERAL;
    p.build = p.gen_build;
    p.envs_per_wg = epw;
    p.threads_per_wg = two_waves ? 128 : 64;
  }
  p.blocks = (r.n + p.envs_per_wg - 1) / p.envs_per_wg;

  // ---- step_many: K steps as ONE launch of the step-loop build, or chained graphs of single steps ----
  // The step-loop launch (every step taking its own action block) has no kernel boundaries at all; the state stays in LDS
  // between the steps.  Always for worlds without contact points (pendulums, the cartpole: ~7 us step kernels of which a
  // boundary is a third).  Option step_many_loop = 0 / 1 forbids / forces it.
  if (r.nsub < 2) {
    p.loop = false;
  } else if (o.is_set(TDS_OPT_STEP_MANY_LOOP)) {
    p.loop = o.v[TDS_OPT_STEP_MANY_LOOP] == 1;
  } else if (!(s.model.has_plane && ncp > 0) && !two) {
    p.loop = true;
  } else if (quad) {
    // the star-shaped legged robots (248 VGPR, no scratch in its step-loop form): the step-loop form while EVERY workgroup
    // of the launch is resident at once, the chained graphs beyond that, where the loop form would run its workgroups in
    // two rounds of all the steps each.  laikago_soft (tools/quad_occupancy_sweep.sh, us per step, loop / graphs): x 4096
    // 13.4 / 20.8, x 6144 18.3 / 23.2, x 8192 32.5 / 24.7; with auto-reset: 13.2 / 21.0, 17.8 / 25.8, 30.9 / 27.4.
    p.loop = quad_waves != 0;
  } else if (oct || chain) {
    // the 8-lane kernels: always one launch.  Its straight-line form costs the same table copy and workgroup rounds per
    // step plus a kernel boundary and the state's round trip through HBM, so beyond one round of resident workgroups
    // R rounds of K steps still beat K launches of R rounds
    p.loop = true;
  } else {
    // Worlds with contacts, kernels up to 16 dof (their step-loop builds fit the registers): one launch beats the chained
    // graphs up to three rounds of workgroups (Ant x 2048 / 4096 / 8192: 14.4 / 14.9 / 20.3 us per step against
    // 15.3 / 16.6 / 23.2; x 16384: 39.0 against 36.6).  Wider kernels spill in the loop build and stay with the graphs.
    // With auto-reset on the alternative is not the chained graphs but single steps through the reset pool: the step-loop
    // launches (pool_step_many) win at every batch size.
    const bool plain = !two && !floating && !spherical;
    p.loop = plain && s.lds.NDP <= 16 && ((n_res + epw - 1) / epw <= 3072 || s.auto_reset);
  }
  // The 8-lane kernel beyond one round of resident two-wavefront workgroups (Ant: 8192 environments): the environments are
  // independent, so the call runs as environment ranges of that size ONE AFTER THE OTHER, each a launch of all the steps
  // in the two-wavefront build — instead of one launch of the one-wavefront build in several rounds (x 12288 as 8192 +
  // 4096: 15.7 us per step, as 2 x 6144: 17.5).  The exchange's launches count workgroups per slot and stay whole.
  if (oct && o2 == 1 && !r.progress && !r.peers) {
    const int cap = 8 * s.num_cus * (oct_per_cu < 4 ? oct_per_cu : 4);
    if (cap > 0 && n_res > cap) p.env_range = cap;
  }
  // The ring launch of the shard layer: where it would take the two-wavefront build without progress counters it runs
  // exactly as at N = 1 and its slots are exchanged once it has completed (a wait beside that build gets onto a compute
  // unit only when the launch retires).  (Compares the workgroups of the kernel that takes the launch with the general
  // kernel's w2_max_blocks.)
  p.exchange_after = !variants && o.get(TDS_OPT_EXCHANGE_W2, 1) != 0 && loop_w2 != 0 && s.w2_max_blocks > 0 &&
                     p.blocks <= s.w2_max_blocks && s.lds_w2.NDP <= 16;
  return p;
}

inline const TdsLds &tds_plan_layout(const tds_hip_sim &s, const TdsLaunchPlan &p) {
  return p.layout == TDS_LAYOUT_POOL ? s.pool_lds : (p.layout == TDS_LAYOUT_W2 ? s.lds_w2 : s.lds);
}

// the handle's launch shape, from the model, the options and the device's num_cus / lds_per_cu (set by the caller):
// device model, lanes, LDS layouts, w2_max_blocks.  No HIP call (tds_api.hip).
int tds_shape_handle(tds_hip_sim *s, const tds_model_t *model, int num_envs, int dtype);
