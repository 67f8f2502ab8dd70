// tds_oct.hip — the step kernel of the star-shaped robots with TWO-link legs on 8 lanes per environment (round 6; the
// headline: BASELINE configs 3 and 5, the gym Ant).
//
// The Ant is the same star as Laikago (tds_quad.hip): a root body on the reference's six "virtual" links (prismatic x, y, z,
// revolute x, y, z: tds_device_model.h euler_root) and four legs with nothing between them but the root — here serial
// chains of two links (hip, ankle), every link with a 1-dof joint and a capsule, the root body with a sphere: 17 contact
// points against the plane.  The general kernel gives it a 16-lane group and a dense 14 x 14 register LDL^T; this kernel:
//
//   * 8 lanes per environment = the 8 leg links, one PAIR of lanes per leg (lane = 2 leg + position in the chain); EIGHT
//     environments per wavefront.  The root chain needs no lane: pose, motion axes, velocity and bias acceleration of
//     the root body in closed form on every lane (the formulas of the general kernel's phase C); its rigid inertia
//     redundantly on every lane; the legs' composites reach it by three DPP moves (pair, quad, half-row mirror).
//   * M in LEAVES-FIRST order [leg 0 | leg 1 | leg 2 | leg 3 | root]: four independent 2 x 2 leg blocks, their 6-column
//     couplings to the root, the root's 6 x 6 block.  LDL^T: both lanes of a pair factorise their leg's block (values by
//     quad_perm moves, no LDS), the coupling rows L_c = W D^-1 follow inside the pair, the root's Schur complement
//     S = R - sum_lanes L_c W^T is R in registers (closed form of the six root axes) minus 21 lane-parallel sums over an
//     LDS copy of (L_c | W), factorised redundantly on every lane.  Forward dynamics qdd = M^-1 (tau - C) and the final
//     qd -= M^-1 J^T p are pair-local substitutions plus six 8-lane sums.
//   * a contact's constraint row touches its leg's two dofs and the root's six: z~ = D^-1/2 L^-1 J^T is 8 wide.  The
//     rows are never all in memory: the Gauss-Seidel sweep (mb_constraint_solver.hpp:101-142) visits them in the
//     reference's order — normals, tangents 1, tangents 2, each by contact — in WINDOWS of eight: eight lanes solve the
//     rows of eight consecutive sweep positions (lane == row), the sweep consumes them, the next window follows.  No
//     contact-count cap, no overflow slab: all 17 points of an environment may penetrate at once.
//
// Same arithmetic contract as the general kernel — the reference's env step (locomotion_contact_simulation.h:151-304) to
// round-off, the same quirks (contacts from pre-step transforms with post-integration velocities, plane_space's k,
// unnormalised REVOLUTE_AXIS axes, visual poses that lag q by one step) — pinned by the same tests: a handle takes this
// kernel when its model is such a star (DevModel::oct, tds_device_model.h) and option oct is not 0; option oct = 0 keeps
// the general kernel, and tests/test_oct.py holds the two against each other and against the reference.
//
// Two forms (template parameter LOOP) as in tds_quad.hip: one step per launch, and K steps per launch with the state in
// LDS, a fresh action block per step, per-step record rings, reset-pool entries taken inside the loop and the exchange of
// the multi-GPU layer (tds_shard.hip: progress counters, peer stores).  Four builds of each (template parameter BUILD, see
// oct_body): one wavefront per workgroup of eight environments, and three with TWO — a main wavefront on the step's
// dependent chain and a helper / recorder beside it (narrowphase, visual poses, constraint rows, every record store), the
// form the host grants while every workgroup is resident with at most two wavefronts per SIMD (Ant x 4096: one wavefront
// per SIMD; x 8192: two).  Who does what between which barriers: the comment at "the step" at the end of oct_body.
// In-kernel reset + settle, substeps with one action through a policy and on-device rollouts stay with the general
// kernel.  Reference files as in tds_kernels.hip.
//
// One instantiation is tuned beyond the others: the step-loop form of the build for one wavefront per SIMD (oct_body:
// SOLO) — the benchmark's, Ant x 4096.  There each wavefront has a loop of its own, the main wavefront carries its state and
// the constants of the step's top across the step boundary in registers, the helper sums the Schur complement, stores the
// visual poses in its idle tail, reads the launch's control block once and its rows' operands in batches, and the first
// sweep is specialised for 1 .. 4 contacts.  Where it differs, an `if constexpr (SOLO)` says so and why at the place; the
// other seven instantiations compile the other arm and keep their statement order: reordered statements move the
// register allocation of builds that gain nothing from them (tools/experiments/lds_batching_not_kept.txt).  What was
// measured and lost, so that nobody tries it again: tools/experiments/oct_*_not_kept.txt.
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include "tds_device_model.h"
#include "tds_kernels.h"
#include "tds_lanes.h"
#include "tds_oct_windows.h"
#include "tds_step_shared.h"

// Phase stamps (a build of its own: -DTDS_OCT_PROF, tools/oct_profile.sh): workgroup TDS_OCT_PROF_WG writes the shader clock
// at the phase boundaries of iteration TDS_OCT_PROF_ITER of a step-loop launch into tds_oct_prof_buf
#ifdef TDS_OCT_PROF
#ifndef TDS_OCT_PROF_WG
#define TDS_OCT_PROF_WG 3
#endif
__device__ unsigned long long tds_oct_prof_buf[64];
// (shader clock, 100 MHz real-time clock) at the top of the first 32 iterations of the stamped workgroup's main wavefront: the
// shader clock's frequency step by step (tools/oct_clock_ramp.py)
__device__ unsigned long long tds_oct_prof_clk[64];
// 100 MHz real-time clock of every workgroup (up to 2048) at its first instruction, at the top of its first step and behind its
// last step: how far apart the workgroups of a launch start and end (tools/oct_clock_ramp.py)
__device__ unsigned long long tds_oct_prof_wg[3 * 2048];
__device__ int tds_oct_prof_iter = 500;
#define OCT_STAMP(k, pin)                                                                       \
  do {                                                                                          \
    unsigned long long t_;                                                                      \
    auto p_ = (pin); /* a value of the phase before: computed before the clock is read */       \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_), "+v"(p_)::"memory");        \
    if (prof_on) prof_t[k] = t_;                                                                \
  } while (0)
// a barrier with the clock in front of it and behind it (stamps k, k + 1): who arrives first and how long it waits
// (tools/oct_profile.py); the window barriers behind the first one add their waits up in stamp k + 2
#define OCT_BAR_T(k)       \
  do {                     \
    OCT_STAMP(k, tid);     \
    OCT_BAR();             \
    OCT_STAMP((k) + 1, tid); \
  } while (0)
#define OCT_BAR_W(k, first)                                                                     \
  do {                                                                                          \
    unsigned long long a_, b_;                                                                  \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(a_), "+v"(tid)::"memory");       \
    OCT_BAR();                                                                                  \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(b_), "+v"(tid)::"memory");       \
    if (prof_on && (first)) {                                                                   \
      prof_t[k] = a_;                                                                           \
      prof_t[(k) + 1] = b_;                                                                     \
    } else if (prof_on) {                                                                       \
      prof_t[(k) + 2] += b_ - a_;                                                               \
    }                                                                                           \
  } while (0)
#else
#define OCT_STAMP(k, pin) do { } while (0)
#define OCT_BAR_T(k) OCT_BAR()
#define OCT_BAR_W(k, first) OCT_BAR()
#endif

// -DTDS_OCT_MARKS: "; OCTMARK <name>" comment lines in the assembly at the phase boundaries (tools/oct_isa_phases.py counts the
// instructions between them: on a lone wavefront the instruction count IS the time)
#ifdef TDS_OCT_MARKS
#define OCT_MARK(name) asm volatile("; OCTMARK " name ::: "memory")
#else
#define OCT_MARK(name) do { } while (0)
#endif

namespace {

#define OCT_SYNC()                                             \
  do {                                                         \
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");     \
    __builtin_amdgcn_wave_barrier();                           \
  } while (0)

// ---- DPP moves inside the 8-lane group of an environment (two environments share a 16-lane DPP row) ----
template <int CTRL>
__device__ __forceinline__ double oct_dpp(double v) {
  const int l = __double2loint(v), h = __double2hiint(v);
  const int lo = __builtin_amdgcn_update_dpp(0, l, CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, h, CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
template <int CTRL>
__device__ __forceinline__ float oct_dpp(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
// the other lane of my pair (quad_perm [1, 0, 3, 2])
template <typename T>
__device__ __forceinline__ T pair_other(T v) { return oct_dpp<0xB1>(v); }
// lane K of my pair to both lanes (quad_perm [0, 0, 2, 2] / [1, 1, 3, 3])
template <int K, typename T>
__device__ __forceinline__ T pair_bcast(T v) { return oct_dpp<(K == 0 ? 0xA0 : 0xF5)>(v); }
// sum over the 8 lanes of an environment, every lane receives the SAME bits: pair (a + b and b + a are the same sum),
// pair of pairs, then the mirror image of the half row (lane i <- lane 7 - i: the other quad, whose four lanes agree)
// (the operand is pinned in a register first: a product handed in must be ROUNDED before the first addition — contracted
//  into it, lane i would add its exact product to lane i ^ 1's rounded one and lane i ^ 1 the other way round: the two
//  "same" sums then differ in the last bit, and with them everything that is redundant on every lane behind them; an
//  environment's result would depend on which lane solves which constraint row, i.e. on its wavefront-mates' contacts)
// (PIN = false: for a summand that is NOT a product — a sum, a table value: nothing can contract into the first addition, and
//  the pin costs a copy wherever the summand itself is read again behind the sum)
template <bool PIN = true, typename T>
__device__ __forceinline__ T oct_sum(T v) {
  if constexpr (PIN) asm volatile("" : "+v"(v));
  v += oct_dpp<0xB1>(v);   // quad_perm [1, 0, 3, 2]
  v += oct_dpp<0x4E>(v);   // quad_perm [2, 3, 0, 1]
  v += oct_dpp<0x141>(v);  // row_half_mirror
  return v;
}
// lane K (0..7) of every environment to its 8 lanes: row_newbcast of lane K into the first half of every 16-lane row, of
// lane 8 + K into the second (bank masks: a bank is four lanes)
template <int K>
__device__ __forceinline__ double oct_bcast(double v) {
  const double t = __builtin_amdgcn_update_dpp(0.0, v, 0x150 + K, 0xF, 0x3, false);
  return __builtin_amdgcn_update_dpp(t, v, 0x150 + 8 + K, 0xF, 0xC, false);
}
template <int K>
__device__ __forceinline__ float oct_bcast(float v) {
  const int b = __float_as_int(v);
  const int t = __builtin_amdgcn_update_dpp(0, b, 0x150 + K, 0xF, 0x3, false);
  return __int_as_float(__builtin_amdgcn_update_dpp(t, b, 0x150 + 8 + K, 0xF, 0xC, false));
}

// ---- dot3 / cross3 / sym3_mulv / I s where components of an operand are structural zeros ----
// The root chain is written without the zeros of its axes (A3 = e_x, A4 = (0, cx, sx), P x A3 = (0, Pz, -Py), J3 = (d3, 0, 0)):
// without fast-math the back end keeps every x * 0 and 0 + x.  Only a product with a literal-zero factor, or the addition of
// one, is left out; what remains is rounded as the general form rounds it, so results differ from it in the sign of an exact
// zero at most (profiles/oct_main_diet_bench.txt, tools/experiments/oct_main_diet_not_kept.txt).
// -ffp-contract=on fuses as the source says: x * y + z * w is fma(x, y, rnd(z * w)) — the LEFT product is fused, the right one
// rounded first — so dot3's a0 b0 + a1 b1 + a2 b2 is fma(a2, b2, fma(a0, b0, rnd(a1 b1))), and x * y - z * w is
// fma(x, y, -rnd(z * w)).  With a product 0 what is left must name the SAME product as the rounded one: dot3 without its first
// term is a2 b2 + a1 b1 (not a1 b1 + a2 b2), a cross product's component with one product gone is the other product alone.
template <typename T>
__device__ __forceinline__ T oct_dot3_0(const T *a, const T *b) {  // a[0] b[0] == 0
  return a[2] * b[2] + a[1] * b[1];
}
template <typename T>
__device__ __forceinline__ void oct_cross3_b0(const T *a, const T *b, T *o) {  // a x (0, b1, b2)
  const T x = a[1] * b[2] - a[2] * b[1];
  const T y = -(a[0] * b[2]);
  const T z = a[0] * b[1];
  o[0] = x;
  o[1] = y;
  o[2] = z;
}
template <typename T>
__device__ __forceinline__ void oct_cross3_bx(const T *a, T d, T *o) {  // a x (d, 0, 0)
  o[0] = T(0);
  o[1] = a[2] * d;
  o[2] = -(a[1] * d);
}
template <typename T>
__device__ __forceinline__ void oct_cross3_ax_b0(T d, const T *b, T *o) {  // (d, 0, 0) x (0, b1, b2)
  o[0] = T(0);
  o[1] = -(d * b[2]);
  o[2] = d * b[1];
}
template <typename T>
__device__ __forceinline__ void oct_sym3_mulv_0(const T *s, const T *v, T *o) {  // v[0] == 0
  const T x = s[2] * v[2] + s[1] * v[1];
  const T y = s[4] * v[2] + s[3] * v[1];
  const T z = s[5] * v[2] + s[4] * v[1];
  o[0] = x;
  o[1] = y;
  o[2] = z;
}
// times_inertia (oct_body) of the axis (e_x | 0, p1, p2): F[3] is m * 0 - 0
template <typename T>
__device__ __forceinline__ void oct_times_inertia_ex(const T *I, const T *pl, T *F) {
  T t3[3];
  oct_cross3_b0(I + 6, pl, t3);
  F[0] = I[0] + t3[0];
  F[1] = I[1] + t3[1];
  F[2] = I[2] + t3[2];
  F[3] = T(0);
  F[4] = I[9] * pl[1] - I[8];
  F[5] = I[9] * pl[2] + I[7];
}
// ... of an axis (0, s1, s2 | s3, s4, s5)
template <typename T>
__device__ __forceinline__ void oct_times_inertia_0(const T *I, const T *s, T *F) {
  T t3[3];
  oct_sym3_mulv_0(I, s, F);
  cross3(I + 6, s + 3, t3);
  F[0] += t3[0];
  F[1] += t3[1];
  F[2] += t3[2];
  oct_cross3_b0(I + 6, s, t3);
  F[3] = I[9] * s[3] - t3[0];
  F[4] = I[9] * s[4] - t3[1];
  F[5] = I[9] * s[5] - t3[2];
}

// LDS per environment, offsets in scalars of T
struct OctOff {
  int lcw, legf, swl, qdp, fac, win, xs, cp, stride;
};
struct OctLds {
  static constexpr int LCW = 6;   // [8 lanes][Lc(6)]  (W = Lc D, needed for the Schur sums only, borrows the impulses' slots)
  // a window row: z~ leg (2) | z~ root (6) | 0 | 0 | b | 1 / (G + cfm) | G | hip lane of the contact's leg.  (The two zeros: lane j
  // of the sweep reads root entry j — lanes 6, 7 of an environment read them.)  Every slot is written once per window, with
  // its final value; the first window's root entries are parked in their slots before they are solved (rows_park).
  static constexpr int ZW = 14;
  static constexpr int Z_B = 10, Z_A = 11, Z_G = 12, Z_HL = 13;
  static constexpr int NCP = 17;  // contact points (torso + 2 per leg link), and the stride of the contact list
};
__host__ __device__ inline OctOff oct_layout(int in_dim) {
  OctOff o;
  int at = in_dim + 4;          // x record | x_{t-1} | done | reward | flag / count
  at = (at + 1) & ~1;
  o.lcw = at;  at += 8 * OctLds::LCW;     // L_c of the 8 leg-dof lanes
  o.legf = at; at += 4 * 3;               // per leg: l10 | sqrt(1/d0) | sqrt(1/d1)
  o.swl = at;  at += 8 * 6;               // world motion axis of the 8 leg-dof lanes
  o.qdp = at;  at += 8;                   // leg velocities after integrate_euler_qdd
  o.fac = at;  at += 28;                  // the 21 lane-parallel sums of the Schur complement; then (two-wavefront build) the root
                                          // block's factors for the helper: L_S (15) | sqrt(1/D_S) (6) | root velocities (6)
  o.win = at;  at += 2 * 8 * OctLds::ZW;  // two windows of constraint rows (the second doubles as the hand-over of the links' world
                                          // transforms, 8 x 12, and the root's sines / cosines, 6, from the main wavefront to the helper)
  o.xs = at;   at += 3 * OctLds::NCP + 1; // impulses (before the sweep: W = L_c D of the 8 leg-dof lanes, for the Schur sums)
  o.cp = at;   at += 5 * OctLds::NCP + 1; // contact list: point (3) | distance | owner lane, per slot
  // the environments of a wavefront on different banks: four consecutive ones (half a wavefront) must not meet on an
  // 8-byte bank pair — the stride in 4-byte words a multiple of 8 that is neither 0 nor 32 mod 64
  at = (at + 1) & ~1;
  while ((((at * 2) & 63) % 8) != 0 || ((at * 2) & 63) == 0 || ((at * 2) & 63) == 32) at += 2;
  o.stride = at;
  return o;
}

struct OctKernArgs {
  const void *mdl, *x_in;
  void *y_out;
  const void *actions;
  void *x_feedback, *obs_out;
  TdsStepCtl ctl;
  int n_envs;
  OctOff O;
};
// the constants of the model as the kernel reads them: one table in LDS behind the environments' regions, copied from
// DevModel::oct_tab (laid out by tds_build_oct_table on the host: tds_device_model.h, TDS_OCT_*) at the top of a launch
using TB = TdsOctTab;

// barrier between the two wavefronts of a workgroup (W2: LDS writes done, then s_barrier — neither wavefront waits for its
// outstanding global stores); a compiler-level fence in the one-wave build, where the LDS executes a wavefront's
// instructions in order
#define OCT_BAR()                                                                        \
  do {                                                                                   \
    if constexpr (W2) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");    \
    else OCT_SYNC();                                                                     \
  } while (0)

// LOOP: K steps per launch (state in LDS).  W2: TWO wavefronts per workgroup of eight environments — the MAIN wavefront walks
// the step's dependent chain (PD, kinematics, inertias, LDL^T, forward dynamics, the Gauss-Seidel sweep, integration,
// reward), the HELPER does what hangs off it (narrowphase, visual poses, the constraint rows window by window, every record
// store, the exchange); in the one-wave build the one wavefront plays both roles in the same order.
// BUILD: 1 one wavefront per workgroup; 2 two, compiled for two wavefronts per SIMD (256 registers); 3 two, compiled for one
// wavefront per SIMD (what a launch of at most two workgroups per compute unit gets anyway: Ant x 4096 — no spills)
// BUILD 4: the two-wavefront build for launches that run BESIDE another launch's wavefronts on a SIMD (the reset pool's refill
// passes beside the chunk they top up, tds_api.hip: pool_run): at most 240 registers — a wavefront of the one-wavefront-per-SIMD
// build holds 272 of a SIMD's 512 — every wavefront at the lowest priority.  (The kernel's body is a device function inlined
// into two kernels, because the register limit is an attribute that takes a literal.)
template <typename T, typename TR, bool LOOP, int BUILD>
__device__ __forceinline__ void oct_body(const DevModel<T> *__restrict__ mdl_arg, const TR *x_in, TR *__restrict__ y_out,
                                         const TR *__restrict__ actions, TR *x_feedback /* may alias x_in */,
                                         TR *__restrict__ obs_out, const TdsStepCtl &ctl_arg, int n_envs, const OctOff &O) {
  extern __shared__ __align__(16) unsigned char tds_oct_smem[];
  T *const sm = reinterpret_cast<T *>(tds_oct_smem);
#ifdef TDS_OCT_PROF
  if (threadIdx.x == 0 && blockIdx.x < 2048) {
    unsigned long long c_;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(c_)::"memory");
    tds_oct_prof_wg[3 * blockIdx.x] = c_;
  }
#endif
  constexpr bool W2 = BUILD >= 2;
  // SOLO: the step-loop form compiled for one wavefront per SIMD — the benchmark's instantiation, and the one with registers
  // to spare.  What is confined to it costs registers: the 256-register build would pay with scratch, and the others gain
  // nothing from it (each site says what; profiles/oct_step_boundary_resources.txt, profiles/oct_kernel_resources_lds.txt).
  constexpr bool SOLO = LOOP && BUILD == 3;
  // SD_LATE (main_sweep): a friction row's first use of its normal row's impulse stands behind the row's 8-lane sum — the
  // step-loop forms of builds 2 and 3
  constexpr bool SD_LATE = LOOP && (BUILD == 2 || BUILD == 3);
  constexpr int nq = 14, nd = 14, adim = 8, in_dim = nq + nd + adim + 3, w_obs = nq + nd + 2;
  constexpr int NT = W2 ? 128 : 64;
  T *const CT = sm + 8 * O.stride;  // the constant table
  {
    // ---- the constant table (coalesced copy) and A. x record -> LDS, fresh actions over the action slice
    // (every global load of the prologue is issued before the first of them is waited for: as loops of load -> LDS store the
    //  table copy and the record copy were ten dependent round trips, 4.8 us in front of the first step of every launch —
    //  tools/oct_clock_ramp.py)
    const int t = threadIdx.x;
    constexpr int TN = (TB::TOTAL + NT - 1) / NT, XN = (in_dim + 7) / 8;
    T tv[TN], xv[XN];
#pragma unroll
    for (int k = 0; k < TN; ++k) {
      const int i = t + k * NT;
      tv[k] = i < TB::TOTAL ? mdl_arg->oct_tab[i] : T(0);
    }
    const int lane0 = t & 7, grp0 = (t & 63) >> 3, env0 = blockIdx.x * 8 + grp0;
    const bool valid0 = env0 < n_envs && t < 64;
#pragma unroll
    for (int k = 0; k < XN; ++k) {
      const int i = lane0 + 8 * k;
      const bool act = actions != nullptr && i >= nq + nd && i < nq + nd + adim;
      xv[k] = (!valid0 || i >= in_dim) ? T(0) : act ? (T)actions[(size_t)env0 * adim + (i - nq - nd)] : (T)x_in[(size_t)env0 * in_dim + i];
    }
#pragma unroll
    for (int k = 0; k < TN; ++k) {
      const int i = t + k * NT;
      if (i < TB::TOTAL) CT[i] = tv[k];
    }
    if (t < 64) {
      T *const xr = sm + grp0 * O.stride;
#pragma unroll
      for (int k = 0; k < XN; ++k) {
        const int i = lane0 + 8 * k;
        if (i < in_dim) xr[i] = xv[k];
      }
      if (lane0 < 4) xr[in_dim + lane0] = T(0);
    }
    if constexpr (W2) __syncthreads();
    else OCT_SYNC();
  }
  const int nsteps = LOOP ? ctl_arg.nsub : 1;
  T next_act = T(0);  // (step-loop form, main wavefront: the action of the NEXT step, requested a step ahead)
  // ring positions of the current step, carried along as scalars (a remainder by a run-time divisor per step and ring costs
  // ~100 instructions at the top of the main wavefront's chain): action block of step it + 1, y slot and obs slot of step it
  int act_blk = 0, y_slot = 0, o_slot = 0;
  if constexpr (LOOP) {
    if (ctl_arg.act_pool != nullptr && ctl_arg.act_blocks > 0) act_blk = (ctl_arg.act_first + 1) % ctl_arg.act_blocks;
    if (ctl_arg.y_ring != nullptr && ctl_arg.y_slots > 0) y_slot = ctl_arg.y_first % ctl_arg.y_slots;
    if (ctl_arg.obs_ring != nullptr && ctl_arg.obs_slots > 0) o_slot = ctl_arg.obs_first % ctl_arg.obs_slots;
  }
  // (where my lane's action sits in the record: one register across the steps, against a table read in front of the PD block's
  //  read of the action — two LDS round trips in a row at the top of the main wavefront's step)
  const int act_slot = (int)(CT + (threadIdx.x & 7) * TB::LSTR)[TB::ACT];
  // SOLO: what the main wavefront's integration (main_fin) hands to its next kinematics (main_kin) in registers — its dof's q
  // and qd, the root's six coordinates and six velocities, the very values it stores into the LDS record — so that the top of a
  // step does not read back across barrier (0) what the wavefront wrote itself a phase earlier.  The record is read for the
  // first step of a launch (here: behind the prologue's barrier) and where the reset pool replaced the state of one of the
  // wavefront's environments (main_pool); lanes of an environment past n_envs carry what they stored, as they read it before.
  // (The 256-register build pays for the carried state with 20 B of scratch: profiles/oct_step_boundary_resources.txt.)
  struct Carried { T q, qd, rq[6], rqd[6]; };
  // SOLO: the constants of the PD block, jcalc, the root's frame and velocities — nothing writes them inside a launch: the
  // lane table and the scalar table (written by the prologue, in front of its barrier), kp / kd / max_force of the x record
  // (the reset pool rewrites q | qd only, the helper the action slots only) — requested by the main wavefront in main_fin and
  // held across barrier (0), whose own wait for the LDS takes them in: behind it nothing covers their round trips.  (xt: the
  // translation of X_T; its rotation, read where X_T is not the identity only, stays where it is.  The 256-register build pays
  // for the 33 constants with 64 - 84 B of scratch: the same table.)
  struct TopConsts { T S[6], rotf, nax[3], nn[6], xt[3], ipose, stiff, damp, act_lim, xt_ident, base_t[3], grav[3], kp, kd, max_force; };
  auto carry_load = [&](const T *xr_, int lane_, Carried &c) {
    c.q = xr_[6 + lane_];
    c.qd = xr_[nq + 6 + lane_];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      c.rq[r] = xr_[r];
      c.rqd[r] = xr_[nq + r];
    }
  };
  auto top_request = [&](const T *xr_, const T *CL_, TopConsts &t) {
#pragma unroll
    for (int k = 0; k < 6; ++k) t.S[k] = CL_[TB::S + k];
    t.rotf = CL_[TB::ROTF];
#pragma unroll
    for (int k = 0; k < 3; ++k) t.nax[k] = CL_[TB::NAX + k];
#pragma unroll
    for (int k = 0; k < 6; ++k) t.nn[k] = CL_[TB::NN + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t.xt[k] = CL_[TB::XT + 9 + k];
    t.ipose = CL_[TB::IPOSE];
    t.stiff = CL_[TB::STIFF];
    t.damp = CL_[TB::DAMP];
    t.act_lim = CT[TB::SC + TB::ACTION_LIMIT];
    t.xt_ident = CT[TB::SC + TB::XT_IDENT];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      t.base_t[k] = CT[TB::SC + TB::BASE_T + k];
      t.grav[k] = CT[TB::SC + TB::GRAV + k];
    }
    t.kp = xr_[nq + nd + adim];
    t.kd = xr_[nq + nd + adim + 1];
    t.max_force = xr_[nq + nd + adim + 2];
  };
  Carried car = {};
  TopConsts tc = {};
  // SOLO: the fields of the launch's control block that the helper reads in every step, whatever the launch's form — which
  // rings there are, where they are, whether the step is counted in — read from the kernel-argument segment once per launch and
  // scalars from here on (`hc`, OCT_HC; the helper's loop is its own there, and no other build refers to the copy): through the
  // laundered segment pointer every field is a scalar load of its own in every step, and where one field decides whether the next
  // is read (help_np, help_poses_head, help_rec) a round trip of its own that nothing covers.  What changes from step to step
  // (ring positions, `last`) was never read from there: it follows `it`.  What only an exchange launch reads (the peer table,
  // offsets, flags, epoch) stays a read per step.  The kernel has no SGPRs to spare: the back end parks these sixteen in the lanes of a VGPR in
  // the prologue and fetches a field with one v_readlane where a step uses it — no wait (the whole block held across the loop
  // was 40 parked SGPRs and 69 v_readlane per step; profiles/oct_root_helper_resources.txt).
  struct HelpArgs {
    const void *act_pool;
    void *obs_ring, *y_ring;
    unsigned int *peer_arrive;
    unsigned long long *progress;
    int act_envs, obs_slots, ring_envs, y_stride, obs_envs, ring_flags;
  };
  const HelpArgs hc = {ctl_arg.act_pool, ctl_arg.obs_ring, ctl_arg.y_ring, ctl_arg.peer_arrive, ctl_arg.progress, ctl_arg.act_envs,
                       ctl_arg.obs_slots, ctl_arg.ring_envs, ctl_arg.y_stride, ctl_arg.obs_envs, ctl_arg.ring_flags};
  if constexpr (SOLO) {
    const int lane_ = threadIdx.x & 7;
    const T *const xr_ = sm + ((threadIdx.x & 63) >> 3) * O.stride;
    carry_load(xr_, lane_, car);
    top_request(xr_, CT + lane_ * TB::LSTR, tc);
  }
  // ================================ a step: the body of the step loop ================================
  // ROLE 2: one loop for the whole workgroup, the wavefronts part ways inside the step (`wv`).  ROLE 0 / 1 (SOLO): the
  // main wavefront's / the helper's step, each in a loop of its own — see the loops behind the body.
  auto step_body = [&](auto rolec, const int it) {
  constexpr int ROLE = decltype(rolec)::value;
  // (nothing but `it`, next_act and act_slot lives across an iteration — and, on the main wavefront of the SOLO build,
  //  `car` and `tc` from main_fin to main_kin: lane and kernel-argument segment are laundered)
  const __attribute__((address_space(4))) char *ka_seg = (const __attribute__((address_space(4))) char *)__builtin_amdgcn_kernarg_segment_ptr();
  int tid = threadIdx.x;
  if constexpr (LOOP) asm volatile("" : "+s"(ka_seg), "+v"(tid));
  const int wv = ROLE < 2 ? ROLE : (W2 ? __builtin_amdgcn_readfirstlane(tid >> 6) : 0);
  const bool is_main = !W2 || wv == 0, is_help = !W2 || wv == 1;  // wave-uniform (the profile build's stamps)
  // Two wavefronts per SIMD (BUILD 2): where a main wavefront shares its SIMD with a helper, the main one — the step's
  // instruction stream — issues first (Ant x 8192, same box: 7.93 / 8.09e8 -> 8.42 / 8.37e8 env-steps/s; no effect at one
  // wavefront per SIMD)
  if constexpr (W2) {
    if (BUILD != 4 && wv == 0) __builtin_amdgcn_s_setprio(3);
    else __builtin_amdgcn_s_setprio(0);  // (a helper one step in front of a refill pass's wavefronts on its SIMD: measured, nothing)
  }
  (void)is_main;
  (void)is_help;
#ifdef TDS_OCT_PROF
  unsigned long long prof_t[56] = {};  // 0 .. 14 phases, 24 .. 37 the main wavefront's barriers, 40 .. 53 the helper's
  const bool prof_on = blockIdx.x == TDS_OCT_PROF_WG && it == tds_oct_prof_iter;
  if (it == 0 && tid == 0 && blockIdx.x < 2048) {
    unsigned long long c_;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(c_)::"memory");
    tds_oct_prof_wg[3 * blockIdx.x + 1] = c_;
  }
  if (blockIdx.x == TDS_OCT_PROF_WG && it < 32 && tid == 0) {
    unsigned long long c0_, c1_;
    asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(c0_), "=s"(c1_)::"memory");
    tds_oct_prof_clk[2 * it] = c0_;
    tds_oct_prof_clk[2 * it + 1] = c1_;
  }
#endif
  const int lane = tid & 7;
  const int grp = (tid & 63) >> 3;
  const int env = blockIdx.x * 8 + grp;
  const bool valid = env < n_envs;
  T *const E = sm + grp * O.stride;
  T *const xr = E;
  const int leg = lane >> 1, pos = lane & 1;
  const int dq = 6 + lane;  // my dof in the q / qd records
  const T *const CL = CT + lane * TB::LSTR;  // my lane's constants
  typename TdsCtlRef<LOOP>::type ctl = TdsCtlRef<LOOP>::get(ctl_arg, ka_seg + __builtin_offsetof(OctKernArgs, ctl));
  // (a field of the control block as the helper's phases read it: SOLO, in the helper's own loop — the copy made in front of
  //  that loop; everywhere else the field itself.  The condition is a compile-time constant: one arm only is compiled)
#define OCT_HC(f) ((SOLO && ROLE == 1) ? hc.f : ctl.f)
  const T dt = CT[TB::SC + TB::DT];
  const int pgs_iters = (int)CT[TB::SC + TB::PGS_ITERATIONS];
  const bool last = it == nsteps - 1;
  OCT_STAMP(0, tid);

  // state shared by the phases of a role (main: kinematics .. integration; helper: narrowphase .. records); what crosses from
  // the main wavefront to the helper goes through LDS in the two-wavefront build and stays in these registers otherwise
  T q, qd, tau;
  T Sl[6], R[9], p[3], sw[6], v[6], a0[6];
  T R5[9], P[3], A4[3], A5[3], pA3[3], pA4[3], pA5[3], v5[6], a5[6];
  T Lc[6], l10, id0, id1, sq0, sq1, my_id, my_sq, Ls[15], ids[6], sq_ids[6], qd_new, qdr_new[6];
  T Cb, Cr[6], It[10];  // (main wavefront: bias forces of my dof / the root dofs, the robot's total inertia — across its barriers)
  T u = T(0), urm = T(0);  // u~ = -dt y~ + sum_r z~_r x_r, distributed: my own dof's leg entry | root entry `lane` (lanes 6, 7: zero)
  T u_init = T(0), urm_init = T(0);
  T sw_mu = T(0), sw_rest = T(0), sw_cap = T(0), sw_hip = T(0);  // the sweep's constants (main_sweep_consts)
  int na = 0, NA = 0;

  // the root body's frame and the root's revolute axes from the six sines / cosines (kinematics.hpp:64-97; tds_kernels.hip
  // phase C: same formulas): R5, P, A4, A5 and the linear parts P x A of the three revolute axes (A3 = e_x)
  // (rq, bt: the root's position and the base offset — the record and the table, or the main wavefront's registers: SOLO)
  auto root_frame = [&](const T *rq, const T *bt, T sx, T cx, T sy, T cy, T sz, T cz) {
    R5[0] = cy * cz;                 R5[1] = -cy * sz;                R5[2] = sy;
    R5[3] = sx * sy * cz + cx * sz;  R5[4] = cx * cz - sx * sy * sz;  R5[5] = -sx * cy;
    R5[6] = sx * sz - cx * sy * cz;  R5[7] = cx * sy * sz + sx * cz;  R5[8] = cx * cy;
    P[0] = rq[0] + bt[0];
    P[1] = rq[1] + bt[1];
    P[2] = rq[2] + bt[2];
    A4[0] = T(0); A4[1] = cx; A4[2] = sx;
    A5[0] = sy; A5[1] = -sx * cy; A5[2] = cx * cy;
    pA3[0] = T(0); pA3[1] = P[2]; pA3[2] = -P[1];  // P x e_x
    oct_cross3_b0(P, A4, pA4);
    cross3(P, A5, pA5);
  };
  auto times_inertia = [&](const T *I, const T *s, T *F) {  // (I w + h x v, m v - h x w)
    T t3[3];
    sym3_mulv(I, s, F);
    cross3(I + 6, s + 3, t3);
    F[0] += t3[0];
    F[1] += t3[1];
    F[2] += t3[2];
    cross3(I + 6, s, t3);
    F[3] = I[9] * s[3] - t3[0];
    F[4] = I[9] * s[4] - t3[1];
    F[5] = I[9] * s[5] - t3[2];
  };
  auto dot6 = [&](const T *a, const T *b) -> T { return dot3(a, b) + dot3(a + 3, b + 3); };

  auto main_kin = [&]() {
    // ================================ main: PD, jcalc, kinematics ================================
    OCT_MARK("main_top");
    // (a constant of the top of the step: the register requested in front of barrier (0), SOLO, or the read at its place
    //  of use — the condition is a compile-time constant: one arm only is compiled)
#define OCT_TOP(early, read) (SOLO ? (early) : (read))
    if constexpr (SOLO) {
      q = car.q;
      qd = car.qd;
    } else {
      q = xr[dq];
      qd = xr[nq + dq];
    }
    // ---- PD controller (locomotion_contact_simulation.h:168-258); joint stiffness / damping
    tau = T(0);
    {
      const int act_i = act_slot;
      if (act_i >= 0) {
        const int var = nq + nd + adim;
        const T kp = OCT_TOP(tc.kp, xr[var]), kd = OCT_TOP(tc.kd, xr[var + 1]), max_force = OCT_TOP(tc.max_force, xr[var + 2]);
        const T act_lim = OCT_TOP(tc.act_lim, CT[TB::SC + TB::ACTION_LIMIT]);
        // (the action stays behind barrier (0): the helper writes it during the step)
        T a = xr[nq + nd + act_i];
        a = a < act_lim ? a : act_lim;
        a = a > -act_lim ? a : -act_lim;
        const T q_des = OCT_TOP(tc.ipose, CL[TB::IPOSE]) + a;
        T f = kp * (q_des - q) + kd * (T(0) - qd);
        f = f > -max_force ? f : -max_force;
        f = f < max_force ? f : max_force;
        tau = f;
      }
      tau -= OCT_TOP(tc.stiff, CL[TB::STIFF]) * q + OCT_TOP(tc.damp, CL[TB::DAMP]) * qd;
      // (tau is next read by the forward dynamics, two barriers on: left to itself the back end moves this line down there and
      //  keeps stiffness and damping alive for it — in the 256-register build through scratch, a memory round trip the main
      //  wavefront waited for behind barrier (2))
      asm volatile("" : "+v"(tau));
    }
    // (my root angle: lanes 0, 1, 2 the three angles, the others the first)
    auto root_angle = [&]() -> T {
      if constexpr (SOLO) {
        // (by value first: a conditional between array elements is a conditional between addresses, and `car` a record in scratch)
        const T a3 = car.rq[3], a4 = car.rq[4], a5 = car.rq[5];
        return lane == 1 ? a4 : (lane == 2 ? a5 : a3);
      } else {
        return xr[3 + (lane < 3 ? lane : 0)];
      }
    };
    // (the root angle's sine and cosine, evaluated beside the joint's in one interleaved routine, tds_sincos2: its 17 constants in
    //  registers once per step instead of once per inlined copy — the same bits as two tds_sincos)
    T root_s = T(0), root_c = T(0);
    OCT_MARK("main_jcalc");
    // ---- B. jcalc (link.hpp:229-287)
#pragma unroll
    for (int k = 0; k < 6; ++k) Sl[k] = OCT_TOP(tc.S[k], CL[TB::S + k]);
    T Rp[9], tp[3];
    {
      // the joint transform: R_J = cos I + sin [n]x + (1 - cos) n n^T about the joint's unit axis (table: n, n n^T; a prismatic
      // joint's angle is multiplied by 0), t_J = S_linear q (zero for a revolute joint) — every joint type of link.hpp:229-287
      // without a branch; X_parent = X_T X_J, and where every X_T rotation is the identity (the Ant) no product at all
      T sn, cs;
      tds_sincos2(q * OCT_TOP(tc.rotf, CL[TB::ROTF]), root_angle(), &sn, &cs, &root_s, &root_c);
      const T c1 = T(1) - cs;
      const T nx = OCT_TOP(tc.nax[0], CL[TB::NAX]), ny = OCT_TOP(tc.nax[1], CL[TB::NAX + 1]), nz = OCT_TOP(tc.nax[2], CL[TB::NAX + 2]);
      T RJ[9];
      RJ[0] = cs + c1 * OCT_TOP(tc.nn[0], CL[TB::NN + 0]);
      RJ[1] = c1 * OCT_TOP(tc.nn[1], CL[TB::NN + 1]) - sn * nz;
      RJ[2] = c1 * OCT_TOP(tc.nn[2], CL[TB::NN + 2]) + sn * ny;
      RJ[3] = c1 * OCT_TOP(tc.nn[1], CL[TB::NN + 1]) + sn * nz;
      RJ[4] = cs + c1 * OCT_TOP(tc.nn[3], CL[TB::NN + 3]);
      RJ[5] = c1 * OCT_TOP(tc.nn[4], CL[TB::NN + 4]) - sn * nx;
      RJ[6] = c1 * OCT_TOP(tc.nn[2], CL[TB::NN + 2]) - sn * ny;
      RJ[7] = c1 * OCT_TOP(tc.nn[4], CL[TB::NN + 4]) + sn * nx;
      RJ[8] = cs + c1 * OCT_TOP(tc.nn[5], CL[TB::NN + 5]);
      const T tJ[3] = {Sl[3] * q, Sl[4] * q, Sl[5] * q};
      if (OCT_TOP(tc.xt_ident, CT[TB::SC + TB::XT_IDENT]) != T(0)) {  // wave-uniform
#pragma unroll
        for (int k = 0; k < 9; ++k) Rp[k] = RJ[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) tp[k] = OCT_TOP(tc.xt[k], CL[TB::XT + 9 + k]) + tJ[k];
      } else {
        T RT[9], r[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) RT[k] = CL[TB::XT + k];
        mat3_mul(RT, RJ, Rp);
        mat3_mulv(RT, tJ, r);
#pragma unroll
        for (int k = 0; k < 3; ++k) tp[k] = OCT_TOP(tc.xt[k], CL[TB::XT + 9 + k]) + r[k];
      }
    }
    OCT_MARK("main_rootsincos");
    // ---- C. the root chain in closed form, on every lane.  The three root angles' sines and cosines: lanes 0, 1, 2 of the
    //         environment, broadcast (and, two-wavefront build, handed to the helper behind the links' world transforms)
    {
      const T rs = root_s, rc = root_c;
      const T sx = oct_bcast<0>(rs), cx = oct_bcast<0>(rc);
      const T sy = oct_bcast<1>(rs), cy = oct_bcast<1>(rc);
      const T sz = oct_bcast<2>(rs), cz = oct_bcast<2>(rc);
      if constexpr (W2) {
        if (lane < 3) {
          T *const sc = E + O.win + 8 * OctLds::ZW + 96;
          sc[2 * lane] = rs;
          sc[2 * lane + 1] = rc;
        }
      }
      root_frame(SOLO ? car.rq : xr, SOLO ? tc.base_t : CT + TB::SC + TB::BASE_T, sx, cx, sy, cy, sz, cz);
    }
    OCT_MARK("main_rootvel");
    {
      const T *const rqd = SOLO ? car.rqd : xr + nq;
      const T d0 = rqd[0], d1 = rqd[1], d2 = rqd[2], d3 = rqd[3], d4 = rqd[4], d5 = rqd[5];
      const T U[3] = {d0, d1, d2};
      // J3 = (d3, 0, 0), J4 = (0, cx d4, sx d4).  The general form (tds_kernels.hip phase C) — W4 = J3 + J4, pW4 = P x J3 + P x J4,
      // V3 = U + P x J3, a45 = J3 x J4, l_k = W_k x pJ_k + V_k x J_k, a5 = (a45 + a55 | l3 + l4 + l5 - g) — statement by statement,
      // each without its 0 * x and 0 + x
      const T J4[3] = {T(0), A4[1] * d4, A4[2] * d4}, J5[3] = {A5[0] * d5, A5[1] * d5, A5[2] * d5};
      const T W4[3] = {d3, J4[1], J4[2]};
      const T W5[3] = {W4[0] + J5[0], W4[1] + J5[1], W4[2] + J5[2]};
      T pJ3[3], pJ4[3], pJ5[3];
      oct_cross3_bx(P, d3, pJ3);
      oct_cross3_b0(P, J4, pJ4);
      cross3(P, J5, pJ5);
      const T pW4[3] = {pJ4[0], pJ3[1] + pJ4[1], pJ3[2] + pJ4[2]};
      const T pW5[3] = {pW4[0] + pJ5[0], pW4[1] + pJ5[1], pW4[2] + pJ5[2]};
      const T V3[3] = {U[0], U[1] + pJ3[1], U[2] + pJ3[2]};
      const T V4[3] = {U[0] + pW4[0], U[1] + pW4[1], U[2] + pW4[2]};
      const T V5[3] = {U[0] + pW5[0], U[1] + pW5[1], U[2] + pW5[2]};
      T a45[3], a55[3], t1[3], t2[3], l3[3], l4[3], l5[3];
      oct_cross3_ax_b0(d3, J4, a45);
      cross3(W4, J5, a55);
      oct_cross3_ax_b0(d3, pJ3, t1);
      oct_cross3_bx(V3, d3, t2);
      l3[0] = T(0); l3[1] = t1[1] + t2[1]; l3[2] = t1[2] + t2[2];
      cross3(W4, pJ4, t1);
      oct_cross3_b0(V4, J4, t2);
      l4[0] = t1[0] + t2[0]; l4[1] = t1[1] + t2[1]; l4[2] = t1[2] + t2[2];
      cross3(W5, pJ5, t1);
      cross3(V5, J5, t2);
      l5[0] = t1[0] + t2[0]; l5[1] = t1[1] + t2[1]; l5[2] = t1[2] + t2[2];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        v5[k] = W5[k];
        v5[3 + k] = V5[k];
      }
      a5[0] = a55[0];
      a5[1] = a45[1] + a55[1];
      a5[2] = a45[2] + a55[2];
      a5[3] = (l4[0] + l5[0]) - OCT_TOP(tc.grav[0], CT[TB::SC + TB::GRAV + 0]);
      a5[4] = (l3[1] + l4[1] + l5[1]) - OCT_TOP(tc.grav[1], CT[TB::SC + TB::GRAV + 1]);
      a5[5] = (l3[2] + l4[2] + l5[2]) - OCT_TOP(tc.grav[2], CT[TB::SC + TB::GRAV + 2]);
    }
#undef OCT_TOP
    OCT_MARK("main_legs");
    // ---- the legs: the ankle composes its joint transform with the hip's (one step of a segmented scan along the pair),
    //      the root's pose in front; prefix sums of the joint velocities and of the velocity-product accelerations
    {
      const bool take = pos == 1;
      T Rq[9], pq[3];
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const T sh = pair_bcast<0>(Rp[k]);
        Rq[k] = take ? sh : ((k == 0 || k == 4 || k == 8) ? T(1) : T(0));
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const T sh = pair_bcast<0>(tp[k]);
        pq[k] = take ? sh : T(0);
      }
      T Rl[9], pl[3], r[3];
      mat3_mul(Rq, Rp, Rl);
      mat3_mulv(Rq, tp, r);
#pragma unroll
      for (int k = 0; k < 3; ++k) pl[k] = pq[k] + r[k];
      mat3_mul(R5, Rl, R);
      mat3_mulv(R5, pl, r);
      p[0] = P[0] + r[0];
      p[1] = P[1] + r[1];
      p[2] = P[2] + r[2];
      // s = X_world.apply_inverse(S) = (R w, R v + p x (R w))   (transform.hpp:232-243)
      mat3_mulv(R, Sl, sw);
      mat3_mulv(R, Sl + 3, sw + 3);
      T c[3];
      cross3(p, sw, c);
      sw[3] += c[0];
      sw[4] += c[1];
      sw[5] += c[2];
      T vJ[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) vJ[k] = sw[k] * qd;
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const T sh = pair_bcast<0>(vJ[k]);
        v[k] = v5[k] + (vJ[k] + (take ? sh : T(0)));
      }
      // cb = v x vJ (kinematics.hpp:96-99)
      T cb[6];
      cross3(v, vJ, cb);
      T c1[3], c2[3];
      cross3(v, vJ + 3, c1);
      cross3(v + 3, vJ, c2);
      cb[3] = c1[0] + c2[0];
      cb[4] = c1[1] + c2[1];
      cb[5] = c1[2] + c2[2];
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const T sh = pair_bcast<0>(cb[k]);
        a0[k] = a5[k] + (cb[k] + (take ? sh : T(0)));
      }
    }
    OCT_MARK("main_publish_kin");
    // my world motion axis, for the rows of the contacts (lane-dependent reads in the row windows); two-wavefront build: my
    // link's world transform for the helper's narrowphase and visual poses (the slots of the second row window)
    {
      T *const swl = E + O.swl + lane * 6;
#pragma unroll
      for (int k = 0; k < 6; ++k) swl[k] = sw[k];
      if constexpr (W2) {
        T *const kin = E + O.win + 8 * OctLds::ZW + lane * 12;
#pragma unroll
        for (int k = 0; k < 9; ++k) kin[k] = R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) kin[9 + k] = p[k];
      }
    }
    OCT_MARK("main_kin_end");
    OCT_STAMP(1, sw[5]);
  };

  // where this step's y record goes: the slot of a y ring (every step of a step-loop launch), else the handle's y record
  // (the last step); the last step of a ring launch leaves its record in the handle's y record as well
  const int ystr = OCT_HC(y_stride);
  const int out_dim = (int)CT[TB::SC + TB::OUTPUT_DIM];
  const int nv = (int)CT[TB::SC + TB::NUM_VISUALS];
  // (worked out where a phase stores — three places — from a ring position laundered there: computed once at the top of the
  //  step the two pointers lived across it, in the 256-register build through scratch, reloaded in front of the helper's stores)
  auto y_where = [&](TR *&yo, TR *&yo2, int &yend, int &yend2) {
    int ys = y_slot;
    asm volatile("" : "+s"(ys));
    yo = nullptr;
    yo2 = nullptr;
    yend = ystr;
    yend2 = out_dim;
    if (LOOP && OCT_HC(y_ring) != nullptr) {
      yo = tds_global((TR *)OCT_HC(y_ring)) + ((size_t)ys * OCT_HC(ring_envs) + env) * ystr;
      if (last && y_out != nullptr) yo2 = y_out + (size_t)env * out_dim;
    } else if (last && y_out != nullptr) {
      yo = y_out + (size_t)env * (LOOP ? out_dim : ystr);
      yend = LOOP ? out_dim : ystr;
    }
  };
  // ---- exchange launches of the multi-GPU layer (tds_shard.hip): the records of a step are counted in on the slot's progress
  //      counter (RCCL forms), or on its arrival counters with the flags of every rank raised by the workgroup that
  //      completes the slot (peer-store exchange): tds_step_shared.h.
  // The peer form's count goes in two halves: the first-level atomic (with return) is ISSUED behind barrier (1) — the records of
  // step it - 1 went out a kinematics phase ago — and its result is looked at in front of the visual poses (help_poses): as
  // one piece there, the helper waited for the atomic's round trip to the L2 between barriers (1b) and (2), where the main
  // wavefront waits for the helper
  unsigned sig_tok = 0u;

  auto help_np = [&]() {
    OCT_MARK("help_np");
    // ================================ helper: narrowphase, visual poses ================================
    if constexpr (LOOP) {
      if (it > 0 && OCT_HC(obs_ring) != nullptr && OCT_HC(peer_arrive) != nullptr)  // (wave-uniform; in front of the action request: the wait)
        sig_tok = tds_peer_count_in(ctl, (o_slot == 0 ? OCT_HC(obs_slots) : o_slot) - 1);
      // The NEXT step's action block is requested here, by the helper (a different block per step: tds_hip_step_many), and goes
      // into the record's action slots in front of the visual poses' stores (help_poses) — the slots are dead since the PD
      // block, in front of barrier (1); the next PD block is behind barrier (0).  Requested by the main wavefront and held
      // until the integration, the value crossed the whole step in a register: the 256-register build spilled it to scratch
      // at the top of the step — a wait for the load itself — and reloaded it on the main wavefront's path
      if (OCT_HC(act_pool) != nullptr && it + 1 < nsteps && valid)  // (wave-uniform but for `valid`)
        next_act = (T)tds_global((const TR *)OCT_HC(act_pool))[((size_t)act_blk * OCT_HC(act_envs) + env) * adim + lane];
    }
    if constexpr (W2) {  // my link's world transform and the root's sines / cosines, from the main wavefront
      const T *const kin = E + O.win + 8 * OctLds::ZW + lane * 12;
#pragma unroll
      for (int k = 0; k < 9; ++k) R[k] = kin[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) p[k] = kin[9 + k];
      const T *const sc = E + O.win + 8 * OctLds::ZW + 96;
      root_frame(xr, CT + TB::SC + TB::BASE_T, sc[0], sc[1], sc[2], sc[3], sc[4], sc[5]);
    }
    // ---- I. narrowphase (contact_point.hpp:96-161): my link's capsule = two spheres; the root body's sphere on every lane.
    //         Penetrating points in the reference's order (root, then per link +L/2 end, -L/2 end) into the contact list
    {
      T *const cpx = E + O.cp;
      const T n[3] = {CT[TB::SC + TB::PLANE_N], CT[TB::SC + TB::PLANE_N + 1], CT[TB::SC + TB::PLANE_N + 2]};
      const T pc = CT[TB::SC + TB::PLANE_C];
      auto sphere = [&](const T *Rl, const T *pl, const T *loc, T rad, T *pt, T &dist) {
        T ctr[3];
        mat3_mulv(Rl, loc, ctr);
        ctr[0] += pl[0];
        ctr[1] += pl[1];
        ctr[2] += pl[2];
        const T t = -((-dot3(ctr, n)) + pc);
        dist = t - rad;
        pt[0] = ctr[0] - rad * n[0];
        pt[1] = ctr[1] - rad * n[1];
        pt[2] = ctr[2] - rad * n[2];
      };
      T pt0[3], pt1[3], ptt[3], d0, d1, dtt;
      sphere(R, p, CL + TB::CPL0, CL[TB::CPR0], pt0, d0);
      sphere(R, p, CL + TB::CPL1, CL[TB::CPR1], pt1, d1);
      sphere(R5, P, CT + TB::ROOT + TB::R_CPL, CT[TB::ROOT + TB::R_CPR], ptt, dtt);
      const bool act0 = valid && d0 < T(0), act1 = valid && d1 < T(0), actt = valid && dtt < T(0) && CT[TB::ROOT + TB::R_CPR] >= T(0);
      const unsigned long long b0 = __ballot(act0), b1 = __ballot(act1), bt = __ballot(actt);
      const unsigned m0 = (unsigned)((b0 >> (grp * 8)) & 0xFFull), m1 = (unsigned)((b1 >> (grp * 8)) & 0xFFull);
      const unsigned below = (1u << lane) - 1u;
      const int r0 = (actt ? 1 : 0) + __popc(m0 & below) + __popc(m1 & below);
      const int r1 = r0 + (act0 ? 1 : 0);
      if (act0) {
        cpx[0 * OctLds::NCP + r0] = pt0[0];
        cpx[1 * OctLds::NCP + r0] = pt0[1];
        cpx[2 * OctLds::NCP + r0] = pt0[2];
        cpx[3 * OctLds::NCP + r0] = d0;
        cpx[4 * OctLds::NCP + r0] = (T)lane;
      }
      if (act1) {
        cpx[0 * OctLds::NCP + r1] = pt1[0];
        cpx[1 * OctLds::NCP + r1] = pt1[1];
        cpx[2 * OctLds::NCP + r1] = pt1[2];
        cpx[3 * OctLds::NCP + r1] = d1;
        cpx[4 * OctLds::NCP + r1] = (T)lane;
      }
      if (actt && lane == 0) {
        cpx[0 * OctLds::NCP] = ptt[0];
        cpx[1 * OctLds::NCP] = ptt[1];
        cpx[2 * OctLds::NCP] = ptt[2];
        cpx[3 * OctLds::NCP] = dtt;
        cpx[4 * OctLds::NCP] = T(8);
      }
      na = (actt ? 1 : 0) + __popc(m0) + __popc(m1);
      // the largest count among the wavefront's environments (scalar arithmetic on the three ballots)
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        const int c = __popc((unsigned)((b0 >> (g * 8)) & 0xFFull)) + __popc((unsigned)((b1 >> (g * 8)) & 0xFFull)) + (int)((bt >> (g * 8)) & 1ull);
        NA = c > NA ? c : NA;
      }
      if constexpr (W2) {  // (for the main wavefront's sweep: the spare slot of environment 0's record)
        if ((tid & 63) == 0) sm[in_dim + 3] = (T)NA;
      }
    }
    OCT_STAMP(8, na);
  };
  // (two halves: SOLO takes them apart — the head stays between barriers (1b) and (2), the tail goes behind the helper's last
  //  row window, into its idle tail in front of barrier (0): in one piece the helper idled ~2 k cycles there and was yet the late
  //  one at barrier (2), behind the visual poses; everywhere else help_poses runs them back to back)
  auto help_poses_head = [&]() {
    OCT_MARK("help_signal_poses");
    if constexpr (LOOP) {
      // (loads and stores return through one in-order counter on gfx9: this wait sees the helper's record stores of the step
      //  before, issued a narrowphase and a row stage ago, and nothing of this step)
      if (OCT_HC(act_pool) != nullptr && !last) xr[nq + nd + lane] = next_act;
      // the records of step it - 1 — stored at the end of the iteration before, long acknowledged by now: the wait costs
      // nothing here, in front of this step's first stores — are counted in
      if (it > 0 && OCT_HC(obs_ring) != nullptr) {  // (wave-uniform)
        if (OCT_HC(peer_arrive) != nullptr) tds_peer_finish(ctl, (o_slot == 0 ? OCT_HC(obs_slots) : o_slot) - 1, sig_tok);
        // (SOLO: this guard MIRRORS tds_signal_slot's own check — tds_step_shared.h: without the peer form it acts where there
        //  is a progress counter only — so that a launch without one does not read the two fields per step.  Keep the two in
        //  step: a form added to tds_signal_slot must be added here, or this guard skips it)
        else if (!(SOLO && ROLE == 1) || hc.progress != nullptr) tds_signal_slot(ctl, (o_slot == 0 ? OCT_HC(obs_slots) : o_slot) - 1);
      }
    }
  };
  auto help_poses_tail = [&]() {
    // (SOLO: R, p, R5, P are the helper's registers since help_np — the hand-over slots they came from are row slots of
    //  the later windows by now; the pose slots of the y record are nobody else's: main_pool and help_rec store the state part)
    if constexpr (SOLO) OCT_MARK("help_poses_late");
    // ---- M1. visual poses of y, from the PRE-step X_world (locomotion_contact_simulation.h:281-299): visual 1 + lane is
    //          my link's (DevModel::oct checks the order); visual 0 — the root body's — goes out on lane 7
    TR *yo, *yo2;
    int yend, yend2;
    y_where(yo, yo2, yend, yend2);
    (void)yend;
    (void)yend2;
    if (valid && yo != nullptr && nv > 0) {
      auto pose_out = [&](const T *Rl, const T *pl, const T *vx, int k) {
        T Ro[9], po[3], qo[4];
        mat3_mul(Rl, vx, Ro);
        mat3_mulv(Rl, vx + 9, po);
        matrix_to_quat(Ro, qo);
        TR *o = yo + (nq + nd) + 7 * k;
        o[0] = (TR)(pl[0] + po[0]);
        o[1] = (TR)(pl[1] + po[1]);
        o[2] = (TR)(pl[2] + po[2]);
        o[3] = (TR)qo[0];
        o[4] = (TR)qo[1];
        o[5] = (TR)qo[2];
        o[6] = (TR)qo[3];
        if (yo2 != nullptr) {
          TR *o2 = yo2 + (nq + nd) + 7 * k;
          o2[0] = (TR)(pl[0] + po[0]);
          o2[1] = (TR)(pl[1] + po[1]);
          o2[2] = (TR)(pl[2] + po[2]);
          o2[3] = (TR)qo[0];
          o2[4] = (TR)qo[1];
          o2[5] = (TR)qo[2];
          o2[6] = (TR)qo[3];
        }
      };
      pose_out(R, p, CL + TB::VIS, 1 + lane);
      if (lane == 7) pose_out(R5, P, CT + TB::ROOT + TB::R_VIS, 0);
    }
    OCT_MARK("help_np_end");
    OCT_STAMP(9, na);
  };
  auto help_poses = [&]() {
    help_poses_head();
    help_poses_tail();
  };

  auto main_dyn = [&]() {
    // ================================ main: inertias, LDL^T, forward dynamics ================================
    // ---- D. world-frame rigid inertia and bias force of my link, and (redundantly on every lane) of the root body
    //         (kinematics.hpp:96-132, inertia.hpp:121-130): I = (Isym 6 | h 3 | m), f = I a0 + v x* I v
    auto rigid = [&](const T *Rl, const T *pl, T m, const T *com, const T *Ib, const T *vl, const T *al, T *Ic, T *fc) {
      T cw[3];
      mat3_mulv(Rl, com, cw);
      cw[0] += pl[0];
      cw[1] += pl[1];
      cw[2] += pl[2];
      T RI[9], Iw[9];
      mat3_mul(Rl, Ib, RI);
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) Iw[3 * r + c] = RI[3 * r] * Rl[3 * c] + RI[3 * r + 1] * Rl[3 * c + 1] + RI[3 * r + 2] * Rl[3 * c + 2];
      const T c2 = dot3(cw, cw);
      Ic[0] = Iw[0] + m * (c2 - cw[0] * cw[0]);
      Ic[1] = T(0.5) * (Iw[1] + Iw[3]) - m * cw[0] * cw[1];
      Ic[2] = T(0.5) * (Iw[2] + Iw[6]) - m * cw[0] * cw[2];
      Ic[3] = Iw[4] + m * (c2 - cw[1] * cw[1]);
      Ic[4] = T(0.5) * (Iw[5] + Iw[7]) - m * cw[1] * cw[2];
      Ic[5] = Iw[8] + m * (c2 - cw[2] * cw[2]);
      Ic[6] = m * cw[0];
      Ic[7] = m * cw[1];
      Ic[8] = m * cw[2];
      Ic[9] = m;
      const T *const h = Ic + 6;
      T Iv[6], Ia[6], t3[3];
      sym3_mulv(Ic, vl, Iv);
      cross3(h, vl + 3, t3);
      Iv[0] += t3[0];
      Iv[1] += t3[1];
      Iv[2] += t3[2];
      cross3(h, vl, t3);
      Iv[3] = m * vl[3] - t3[0];
      Iv[4] = m * vl[4] - t3[1];
      Iv[5] = m * vl[5] - t3[2];
      sym3_mulv(Ic, al, Ia);
      cross3(h, al + 3, t3);
      Ia[0] += t3[0];
      Ia[1] += t3[1];
      Ia[2] += t3[2];
      cross3(h, al, t3);
      Ia[3] = m * al[3] - t3[0];
      Ia[4] = m * al[4] - t3[1];
      Ia[5] = m * al[5] - t3[2];
      T u3[3];
      cross3(vl, Iv, fc);
      cross3(vl + 3, Iv + 3, u3);
      fc[0] += u3[0];
      fc[1] += u3[1];
      fc[2] += u3[2];
      cross3(vl, Iv + 3, fc + 3);
#pragma unroll
      for (int k = 0; k < 6; ++k) fc[k] += Ia[k];
    };
    OCT_MARK("main_rigid");
    T Ic[10], fc[6];
    rigid(R, p, CL[TB::MASS], CL + TB::COM, CL + TB::INER, v, a0, Ic, fc);
    // (It, ft) the root body's; below: + the legs' = the whole robot's.  (On the helper, handed over at (1b), it was measured
    //  and not kept — as was the root body's visual pose in the helper's wait at (2): tools/experiments/oct_root_helper_not_kept.txt)
    T ft[6];
    rigid(R5, P, CT[TB::ROOT + TB::R_MASS], CT + TB::ROOT + TB::R_COM, CT + TB::ROOT + TB::R_INER, v5, a5, It, ft);
    OCT_STAMP(2, ft[5]);
    OCT_MARK("main_totals");
    // ---- E. composite inertia / bias force (CRBA, mass_matrix.hpp:39-56): the robot's totals = root + every leg link
    //         (8-lane sums of the rigid values: every lane the same bits); the hip's composite = hip + ankle
    // (Ic[6 .. 8] = m cw are products: pinned.  The others are sums — Ic[0 .. 5], fc — or a table value, Ic[9]: summed without
    //  oct_sum's pinning copy)
    static_for<0, 10>([&](auto kc) {
      constexpr int k = decltype(kc)::value;
      It[k] += oct_sum<(k >= 6 && k <= 8)>(Ic[k]);
    });
#pragma unroll
    for (int k = 0; k < 6; ++k) ft[k] += oct_sum<false>(fc[k]);
    {
      const T recv = pos == 0 ? T(1) : T(0);
#pragma unroll
      for (int k = 0; k < 6; ++k) fc[k] += recv * pair_bcast<1>(fc[k]);
#pragma unroll
      for (int k = 0; k < 10; ++k) Ic[k] += recv * pair_bcast<1>(Ic[k]);
    }
    OCT_MARK("main_FC");
    // F = Ic s, C = s . f of my dof
    T Fc[6];
    times_inertia(Ic, sw, Fc);
    Cb = dot6(sw, fc);
    // the root's revolute axes as (angular | linear): ax3 = (1, 0, 0 | 0, pA3[1], pA3[2]) and ax4 = (0, A4[1], A4[2] | pA4) are
    // written out term by term, without their zeros; the prismatic ones are (0 | e_k)
    const T ax5[6] = {A5[0], A5[1], A5[2], pA5[0], pA5[1], pA5[2]};
    Cr[0] = ft[3];  // bias forces of the root dofs
    Cr[1] = ft[4];
    Cr[2] = ft[5];
    Cr[3] = ft[0] + oct_dot3_0(pA3, ft + 3);
    Cr[4] = oct_dot3_0(A4, ft) + dot3(pA4, ft + 3);
    Cr[5] = dot6(ax5, ft);
    // ---- G. M in leaves-first order.  My row of my leg's 2 x 2 block (M[i][j] = F_i . s_j for j an ancestor of i or i,
    //         mass_matrix.hpp:87-109) and my coupling to the root dofs
    T Bm0, Bm1, Cc[6];
    {
      T s0[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) s0[k] = pair_bcast<0>(sw[k]);
      Bm0 = dot6(Fc, s0);   // hip lane: M_hh; ankle lane: M_ah
      Bm1 = dot6(Fc, sw);   // ankle lane: M_aa
      Cc[0] = Fc[3];
      Cc[1] = Fc[4];
      Cc[2] = Fc[5];
      Cc[3] = Fc[0] + oct_dot3_0(Fc + 3, pA3);
      Cc[4] = oct_dot3_0(Fc, A4) + dot3(Fc + 3, pA4);
      Cc[5] = dot6(Fc, ax5);
    }
    OCT_MARK("main_legldl");
    // ---- H. LDL^T.  The leg block on both lanes of the pair
    {
      const T b00 = pair_bcast<0>(Bm0);
      const T b10 = pair_bcast<1>(Bm0), b11 = pair_bcast<1>(Bm1);
      // (1 / sqrt(d) by the hardware estimate + two Newton steps, 1 / d as its square: what a division AND a square root
      //  per pivot cost — ~25 instructions — for 8)
      sq0 = rsqrt_full<T>(b00);
      id0 = sq0 * sq0;
      l10 = b10 * id0;
      sq1 = rsqrt_full<T>(b11 - l10 * b10);
      id1 = sq1 * sq1;
    }
    my_id = pos == 0 ? id0 : id1;
    my_sq = pos == 0 ? sq0 : sq1;
    // the coupling rows: W_hip = C_hip, W_ankle = C_ankle - l10 W_hip;  L_c = W / d
    {
      T W[6];
      const T m1 = pos == 1 ? l10 : T(0);
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        W[r] = Cc[r] - m1 * pair_bcast<0>(Cc[r]);
        Lc[r] = W[r] * my_id;
      }
      T *const lcw = E + O.lcw + lane * OctLds::LCW;
      T *const wl = E + O.xs + lane * 6;  // (the impulses' slots: free until the sweep)
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        lcw[r] = Lc[r];
        wl[r] = W[r];
      }
      if (pos == 0) {
        T *const lf = E + O.legf + leg * 3;
        lf[0] = l10;
        lf[1] = sq0;
        lf[2] = sq1;
      }
    }
    OCT_STAMP(3, Lc[5]);
  };
  // SOLO: the Schur sums by the helper, directly behind barrier (1b): L_c (O.lcw) and W (O.xs) are in LDS there, and the
  // sums pass through LDS (O.fac) on their way to the 6 x 6 LDL^T anyway.  main_dyn2's table, passes and FMA chains, term by
  // term; the helper has nothing to put across a pass's round trip, so the 48 operands of the three passes are requested in one
  // batch (pass by pass the listing showed 13 exposed round trips).  The other builds sum on the main wavefront, in main_dyn2:
  // batched operands cost build 2 scratch (16-32 B) and the straight-line form of build 3 two more registers, and the
  // one-wavefront build plays both roles in one stream — nothing waits for its main part (profiles/oct_kernel_resources_lds.txt).
  // (The head of the forward dynamics in front of (1c) as well was measured and lost:
  //  tools/experiments/oct_helper_schur_not_kept.txt.)
  auto help_schur = [&]() {
    OCT_MARK("help_schur");
    const T *const lcw = E + O.lcw;
    const T *const wl = E + O.xs;
    T *const Ssum = E + O.fac;
    const int code = (int)CL[TB::SCHUR];
    T la[3][8], wa[3][8];
    int ee[3];
#pragma unroll
    for (int pass = 0; pass < 3; ++pass) {
      const int rc = (code >> (6 * pass)) & 63;
      const int r = rc >> 3, rp = rc & 7;
      ee[pass] = (r * (r + 1)) / 2 + rp;
#pragma unroll
      for (int l = 0; l < 8; ++l) {
        la[pass][l] = lcw[l * OctLds::LCW + r];
        wa[pass][l] = wl[l * 6 + rp];
      }
    }
    __builtin_amdgcn_sched_barrier(0);  // (every request in front of the first sum)
#pragma unroll
    for (int pass = 0; pass < 3; ++pass) {
      T acc = T(0);
#pragma unroll
      for (int l = 0; l < 8; ++l) acc += la[pass][l] * wa[pass][l];
      Ssum[ee[pass]] = acc;
    }
    OCT_MARK("help_schur_end");
    OCT_STAMP(14, na);
  };
  auto main_dyn2 = [&]() {
    OCT_MARK("main_schur");
    // (ax3 = (1, 0, 0 | 0, pA3[1], pA3[2]) is written out term by term, without its zeros; of ax4 = (0, A4[1], A4[2] | pA4) the
    //  zero is never read)
    const T ax4[6] = {A4[0], A4[1], A4[2], pA4[0], pA4[1], pA4[2]}, ax5[6] = {A5[0], A5[1], A5[2], pA5[0], pA5[1], pA5[2]};
    T Sm[21];
    // the root block R[r][r'] = s_r . (It s_r') in registers (packed lower triangle, r (r + 1) / 2 + r'): the prismatic
    // axes are unit vectors, It e_k = (h x e_k | m e_k); then the rows of the three revolute axes
    auto root_block = [&]() {
      T F3[6], F4[6], F5[6];
      const T m = It[9];
      oct_times_inertia_ex(It, pA3, F3);  // (F3[3] = m * 0 - 0 is a structural zero of its own, in the dot products below as well)
      Sm[0] = m;
      Sm[1] = T(0); Sm[2] = m;
      Sm[3] = T(0); Sm[4] = T(0); Sm[5] = m;
      Sm[6] = F3[3]; Sm[7] = F3[4]; Sm[8] = F3[5];
      Sm[9] = F3[0] + oct_dot3_0(pA3, F3 + 3);
      oct_times_inertia_0(It, ax4, F4);
      Sm[10] = F4[3]; Sm[11] = F4[4]; Sm[12] = F4[5];
      Sm[13] = oct_dot3_0(A4, F3) + oct_dot3_0(pA4, F3 + 3);
      Sm[14] = oct_dot3_0(A4, F4) + dot3(pA4, F4 + 3);
      times_inertia(It, ax5, F5);
      Sm[15] = F5[3]; Sm[16] = F5[4]; Sm[17] = F5[5];
      Sm[18] = dot3(A5, F3) + oct_dot3_0(pA5, F3 + 3);
      Sm[19] = dot6(ax5, F4); Sm[20] = dot6(ax5, F5);
    };
    // the sums sum_lanes L_c[r] W[r'] of the Schur complement, entry e = r (r + 1) / 2 + r' on lane e mod 8 (three passes)
    if constexpr (SOLO) {
      // The helper sums (help_schur) while this wavefront does what needs no sum: the root block straight through; barrier (1c):
      // the 21 sums are in O.fac.  Both wavefronts take it once per step, unconditionally.
      // (fences: left to itself the back end moves the root block — arithmetic on registers — up in front of barrier (1b), where
      //  the helper, early there, would wait for it instead of summing beside it; and nothing is to slide behind (1c))
      __builtin_amdgcn_sched_barrier(0);
      root_block();
      __builtin_amdgcn_sched_barrier(0);
      OCT_MARK("main_wait_schur");
      OCT_BAR_T(36);  // (1c)
    } else {
      // (the other builds: this wavefront sums, then computes the root block — why: at help_schur)
      const T *const lcw = E + O.lcw;
      const T *const wl = E + O.xs;  // (W = L_c D in the impulses' slots: every read of it stands here, behind barrier (1b) and in
                                     //  front of barrier (2), in either order of the reads; the sweep's impulses come behind (2))
      T *const Ssum = E + O.fac;
      const int code = (int)CL[TB::SCHUR];  // (which entries this lane sums: table)
#pragma unroll
      for (int pass = 0; pass < 3; ++pass) {
        const int rc = (code >> (6 * pass)) & 63;
        const int r = rc >> 3, rp = rc & 7;
        const int e = (r * (r + 1)) / 2 + rp;
        T acc = T(0);
#pragma unroll
        for (int l = 0; l < 8; ++l) acc += lcw[l * OctLds::LCW + r] * wl[l * 6 + rp];
        Ssum[e] = acc;
      }
    }
    OCT_MARK("main_Rblock");
    if constexpr (!SOLO) root_block();
    OCT_SYNC();  // (the sums of every lane are in LDS, in front of any lane's read of them: a wavefront's LDS operations execute in order)
    OCT_MARK("main_ldl6");
    // ... the Schur complement, factorised redundantly on every lane: Ls (strictly lower, row-major packed), 1 / D
    {
      const T *const Ssum = E + O.fac;
      if constexpr (SOLO) {
        // (the 21 sums requested in one batch: one round trip, not one per pair of them)
        T ss[21];
#pragma unroll
        for (int e = 0; e < 21; ++e) ss[e] = Ssum[e];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int e = 0; e < 21; ++e) Sm[e] -= ss[e];
      } else {
#pragma unroll
        for (int e = 0; e < 21; ++e) Sm[e] -= Ssum[e];
      }
      static_for<0, 6>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        const T rs = rsqrt_full<T>(Sm[(k * (k + 1)) / 2 + k]);
        const T inv = rs * rs;
        sq_ids[k] = rs;
        ids[k] = inv;
        T col[6];
        static_for<k + 1, 6>([&](auto rc) {
          constexpr int r = decltype(rc)::value;
          col[r] = Sm[(r * (r + 1)) / 2 + k];           // S(r, k) before scaling
          Ls[(r * (r - 1)) / 2 + k] = col[r] * inv;     // L(r, k)
        });
        static_for<k + 1, 6>([&](auto rc) {
          constexpr int r = decltype(rc)::value;
          static_for<k + 1, r + 1>([&](auto cc) {
            constexpr int c = decltype(cc)::value;
            Sm[(r * (r + 1)) / 2 + c] -= Ls[(r * (r - 1)) / 2 + k] * col[c];
          });
        });
      });
    }
    OCT_STAMP(4, Ls[14]);
    OCT_MARK("main_fd");
    // two-wavefront build: the root block's factors for the helper's rows
    if constexpr (W2) {
      T *const fac = E + O.fac;  // (the Schur sums are dead: every lane has read them)
      OCT_SYNC();
      if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 15; ++k) fac[k] = Ls[k];
#pragma unroll
        for (int k = 0; k < 6; ++k) fac[15 + k] = sq_ids[k];
      }
    }
    OCT_MARK("main_dyn_end");
  };
  // ---- F. forward dynamics, the forward half (forward_dynamics.hpp:11-326 as qdd = M^-1 (tau - C); integrator.hpp:169-181):
  //      y~ = D^-1/2 L^-1 (tau - C) in the leaves-first system [B C^T; C R] = L D L^T — the leg part on the dof lanes, the root
  //      part on every lane.  The backward half is shared with the contact impulse: the constraint rows' right-hand sides
  //      are formed with the velocities BEFORE the step (rows_geom), and the sweep starts from u~ = -dt y~ instead of 0 —
  //      z~_r . (dt y~) is exactly the J_r (dt qdd) the reference's b_r contains — so that ONE back-substitution at the end
  //      gives  qd_new = qd - L^-T D^-1/2 u~  = qd + dt qdd - M^-1 J^T p  (with no contact: the plain forward dynamics).
  auto main_fd = [&]() {
    OCT_MARK("main_fd");
    T y = tau - Cb;
    y -= (pos == 1 ? l10 : T(0)) * pair_bcast<0>(y);
    T yr[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) yr[r] = -Cr[r] - oct_sum(Lc[r] * y);
    static_for<1, 6>([&](auto rc) {
      constexpr int r = decltype(rc)::value;
      static_for<0, r>([&](auto cc) {
        constexpr int c = decltype(cc)::value;
        yr[r] -= Ls[(r * (r - 1)) / 2 + c] * yr[c];
      });
    });
    u = -dt * (y * my_sq);
    T sel = yr[0] * sq_ids[0];
#pragma unroll
    for (int r = 1; r < 6; ++r) sel = lane == r ? yr[r] * sq_ids[r] : sel;
    urm = lane < 6 ? -dt * sel : T(0);
    u_init = u;
    urm_init = urm;
    OCT_STAMP(5, u);
  };
  // the sweep's constants, once per step, behind the forward dynamics (a scheduling boundary in between: nothing of the
  // forward dynamics is live beside them).  The impulse cap comes from a pinned integer: as a literal it is materialised in
  // every normal row, and a pinned double is canonicalised in front of every minimum.
  auto main_sweep_consts = [&]() {
    OCT_SYNC();
    sw_mu = CT[TB::SC + TB::FRICTION];
    sw_rest = CT[TB::SC + TB::RESTITUTION];
    sw_hip = (T)(lane & ~1);
    int cap = 100000;
    asm volatile("" : "+v"(cap));
    sw_cap = (T)cap;
  };
  // (two-wavefront build, behind barrier (2)) the largest contact count for the main wavefront, the root block's factors for the helper
  auto main_get_count = [&]() { NA = __builtin_amdgcn_readfirstlane((int)sm[in_dim + 3]); };
  auto help_get_factors = [&]() {
    const T *const fac = E + O.fac;
#pragma unroll
    for (int k = 0; k < 15; ++k) Ls[k] = fac[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) sq_ids[k] = fac[15 + k];
  };

  // ---- J, K, L. contacts (wave-uniform: NA = the largest count among the wavefront's environments).  The sweep's order is
  //      the reference's: rows 0 .. NA-1 normals, NA .. 2NA-1 tangents 1, 2NA .. 3NA-1 tangents 2, each by contact (an
  //      environment with fewer contacts has zero rows in its empty slots).  Rows are solved a WINDOW of eight sweep
  //      positions at a time — lane == row, by the helper — and consumed by the main wavefront's sweep; two window buffers:
  //      the helper solves window w + 1 while the main wavefront sweeps window w.
  // A window of the sweep: sweep positions w0 .. w0 + 7 of a Gauss-Seidel iteration, in the row buffer at offset bo (the two
  // buffers take turns); lane == row.  Both wavefronts walk the windows in the same two nested loops (iterations, then w0 in
  // steps of eight up to 3 NA) and carry w0 and bo along: one barrier per window, no division by the run-time window count.
  // Three stages, each as early as its inputs exist (two-wavefront build: all by the helper, beside the main wavefront's chain):
  //   rows_geom  the contact's Jacobian row along the row's direction and the right-hand side c_r from the velocities BEFORE
  //              the step (the kinematics only);
  //   rows_leg   the contact's leg block of z~ = D^-1/2 L^-1 J^T (the leg factors: published at barrier (1b));
  //   rows_root  the root block, G and 1 / (G + cfm) (the root block's factors: barrier (2)).
  // The row's entries of z~ pass from stage to stage in registers (RowRegs), and a slot of the row in LDS is written once, with
  // its final value.  The first window's rows wait for the root block's factors across the visual poses: parked in their own
  // slots of the row (rows_park) and read back in FRONT of barrier (2) (rows_fetch) — behind it the helper reads nothing
  // but the factors.  (SOLO: the poses stand behind the last window, and the first window's rows stay in registers.)
  struct RowRegs {
    T z0, z1, zr[6];
    int hl;
    bool real;
  };
  auto rows_geom = [&](int w0, int bo, RowRegs &rw) {
      OCT_MARK("rows_geom");
      const int nr = 3 * NA;
      T *const row = E + O.win + bo + lane * OctLds::ZW;
      const T *const cpx = E + O.cp;
      const T *const swl = E + O.swl;
      const int s = w0 + lane;
      const int tk = (s >= NA ? 1 : 0) + (s >= 2 * NA ? 1 : 0);
      const int a = s - tk * NA;
      const bool real = s < nr && a < na;
      const int ac = real ? a : 0;
      // (first batch of LDS reads: the contact and the row's direction — n, t1, t2 lie one behind the other in the table —;
      //  every read unconditional, what a padding row reads is masked out at the end: no branch, no wait inside the batch)
      const T Pc[3] = {cpx[0 * OctLds::NCP + ac], cpx[1 * OctLds::NCP + ac], cpx[2 * OctLds::NCP + ac]};
      const T dist = cpx[3 * OctLds::NCP + ac];
      const T owner = cpx[4 * OctLds::NCP + ac];
      const T *const dir = CT + TB::SC + TB::NB + 3 * tk;
      const T e[3] = {dir[0], dir[1], dir[2]};
      // (SOLO: two batches, one per dependent round trip, a scheduling fence behind each — everything that needs no other read
      //  first: the above, the root's velocities, the two constants; then what the owner decides: the leg's axes and velocities.
      //  Left to itself the back end spreads the reads over the arithmetic with a wait in front of every use)
      T rv[6] = {}, c_rest = T(0), c_erp = T(0);
      if constexpr (SOLO) {
#pragma unroll
        for (int k = 0; k < 6; ++k) rv[k] = xr[nq + k];
        c_rest = CT[TB::SC + TB::RESTITUTION];
        c_erp = CT[TB::SC + TB::ERP_OVER_DT];
        __builtin_amdgcn_sched_barrier(0);
      }
#define OCT_GEOM(early, read) (SOLO ? (early) : (read))
      const int ol = real ? (int)owner : 8;    // owner lane; 8: the root body
      const bool on_leg = ol < 8;
      const int hl = on_leg ? (ol & ~1) : 0;   // the hip lane of the contact's leg
      const bool ank = on_leg && (ol & 1);     // the contact sits on the ankle link: both dofs of the leg
      T sh[6], sa[6];
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        sh[c] = swl[hl * 6 + c];
        sa[c] = swl[(hl + 1) * 6 + c];
      }
      const T qh = xr[nq + 6 + hl], qa = xr[nq + 6 + hl + 1];  // velocities before the step
      if constexpr (SOLO) __builtin_amdgcn_sched_barrier(0);
      // column of the point Jacobian along e: e . s_lin + P . (e x s_ang) = e . s_lin + (P x e) . s_ang  (jacobian.hpp:56-72)
      T mo[3];
      cross3(Pc, e, mo);
      const T j0 = dot3(e, sh + 3) + dot3(mo, sh), j1 = dot3(e, sa + 3) + dot3(mo, sa);
      const T z0 = on_leg ? j0 : T(0), z1 = ank ? j1 : T(0);
      T zr[6];
      zr[0] = e[0];
      zr[1] = e[1];
      zr[2] = e[2];
      zr[3] = dot3(e, pA3) + mo[0];
      zr[4] = dot3(e, pA4) + dot3(mo, A4);
      zr[5] = dot3(e, pA5) + dot3(mo, A5);
      const T vrow = ((z0 * qh + z1 * qa) + (zr[0] * OCT_GEOM(rv[0], xr[nq + 0]) + zr[1] * OCT_GEOM(rv[1], xr[nq + 1]))) +
                     ((zr[2] * OCT_GEOM(rv[2], xr[nq + 2]) + zr[3] * OCT_GEOM(rv[3], xr[nq + 3])) +
                      (zr[4] * OCT_GEOM(rv[4], xr[nq + 4]) + zr[5] * OCT_GEOM(rv[5], xr[nq + 5])));
      // rel_vel = vel_a - vel_b = -J qd:  b_n = -(1 + e) n.rel_vel - erp dist / dt,  b_t = -t.rel_vel  (the dt qdd share of
      // the velocity: see main_fd)
      const T crow = tk == 0 ? (T(1) + OCT_GEOM(c_rest, CT[TB::SC + TB::RESTITUTION])) * vrow - OCT_GEOM(c_erp, CT[TB::SC + TB::ERP_OVER_DT]) * dist : vrow;
#undef OCT_GEOM
      rw.z0 = z0;
      rw.z1 = z1;
#pragma unroll
      for (int rr = 0; rr < 6; ++rr) rw.zr[rr] = real ? zr[rr] : T(0);
      rw.hl = hl;  // (a contact of the root body: z0 = z1 = 0, whatever leg rows_leg reads)
      rw.real = real;
      row[8] = T(0);
      row[9] = T(0);
      row[OctLds::Z_B] = real ? crow : T(0);
      row[OctLds::Z_HL] = on_leg ? (T)hl : T(-2);
      OCT_MARK("rows_geom_end");
  };
  auto rows_leg = [&](int bo, RowRegs &rw) {
      OCT_MARK("rows_leg");
      T *const row = E + O.win + bo + lane * OctLds::ZW;
      const T *const lcw = E + O.lcw;
      const T z0 = rw.z0;
      T z1 = rw.z1;
      const int hl = rw.hl;
      T lch[6], lca[6];
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        lch[c] = lcw[hl * OctLds::LCW + c];
        lca[c] = lcw[(hl + 1) * OctLds::LCW + c];
      }
      const T *const lf = E + O.legf + (hl >> 1) * 3;
      const T lf0 = lf[0], lf1 = lf[1], lf2 = lf[2];
      // forward substitution L z = J^T, leaves first: the contact's leg, its share of the root rows; z~_leg = D^-1/2 z
      z1 -= lf0 * z0;
#pragma unroll
      for (int rr = 0; rr < 6; ++rr) rw.zr[rr] = rw.zr[rr] - (lch[rr] * z0 + lca[rr] * z1);
      rw.z0 = z0 * lf1;
      rw.z1 = z1 * lf2;
      row[0] = rw.z0;
      row[1] = rw.z1;
  };
  auto rows_park = [&](const RowRegs &rw) {
      T *const row = E + O.win + lane * OctLds::ZW;
#pragma unroll
      for (int rr = 0; rr < 6; ++rr) row[2 + rr] = rw.zr[rr];
  };
  auto rows_fetch = [&](RowRegs &rw) {
      const T *const row = E + O.win + lane * OctLds::ZW;
      rw.z0 = row[0];
      rw.z1 = row[1];
#pragma unroll
      for (int rr = 0; rr < 6; ++rr) rw.zr[rr] = row[2 + rr];
  };
  auto rows_root = [&](int bo, const RowRegs &rw) {
      OCT_MARK("rows_root");
      T *const row = E + O.win + bo + lane * OctLds::ZW;
      const T z0 = rw.z0, z1 = rw.z1;
      T zr[6];
#pragma unroll
      for (int rr = 0; rr < 6; ++rr) zr[rr] = rw.zr[rr];
      const bool real = rw.real;
      static_for<1, 6>([&](auto rc) {
        constexpr int rr = decltype(rc)::value;
        static_for<0, rr>([&](auto cc) {
          constexpr int c = decltype(cc)::value;
          zr[rr] -= Ls[(rr * (rr - 1)) / 2 + c] * zr[c];
        });
      });
#pragma unroll
      for (int rr = 0; rr < 6; ++rr) zr[rr] *= sq_ids[rr];
      // G = z~ . z~
      const T g = ((z0 * z0 + z1 * z1) + (zr[0] * zr[0] + zr[1] * zr[1])) + ((zr[2] * zr[2] + zr[3] * zr[3]) + (zr[4] * zr[4] + zr[5] * zr[5]));
      const T ai = real ? rcp_full<T>(g + CT[TB::SC + TB::CFM]) : T(0);
#pragma unroll
      for (int rr = 0; rr < 6; ++rr) row[2 + rr] = zr[rr];
      row[OctLds::Z_A] = ai;
      row[OctLds::Z_G] = g;
      OCT_MARK("rows_root_end");
      OCT_STAMP(10, ai);
  };
  // ---- the sweep over a window (mb_constraint_solver.hpp:101-142), by the main wavefront.  A lone wavefront issues an
  //      instruction every ~5 cycles whatever it depends on (tools/ubench/lone_wave_latency.hip): what a row costs is its
  //      instruction count.  u~ = sum_r z~_r x_r is therefore DISTRIBUTED — lane j holds leg entry j (its own dof's) and root
  //      entry j (lanes 6, 7: the row's zero slots) — so that z~_r . u~ is one multiply, one fma and ONE 8-lane sum; the clamp
  //      runs redundantly on every lane; the normal rows and the friction rows of a window are separate loops (no selects on
  //      the row's kind), the first Gauss-Seidel iteration a separate instance (x starts from 0: no G x_old, no read of the
  //      previous impulse).  The window's eight positions are UNROLLED: the row index is a compile-time constant, every row's
  //      LDS addresses are immediate offsets off four base registers per window (the row buffer, my leg entry, my root entry,
  //      the window's impulses), and what is left of the loop is two wave-uniform compares per row — past the window's last
  //      row? a normal row? (normal rows come first in a window).  A row's operands are requested while the row before is
  //      processed (two register sets, taken in turn by the row's parity: no copies); a friction row asks for its normal
  //      row's impulse at its own top, behind the store of the row before (NA = 1: that row IS its normal row).  The model's
  //      constants of the sweep (sw_mu, sw_rest) are read once per step (main_sweep_consts).
  //      The LONG first window (tds_oct_windows.h; two-wavefront builds, first iteration, 8 < 3 NA <= 12: `lw`, wave-uniform):
  //      the chain runs on from position 7 through positions 8 .. 3 NA - 1 — rows of the second buffer, which lies behind
  //      the first: the same immediate offsets off the same bases — instead of returning to the window loop for a window of
  //      one to four rows.  They are second-tangent rows (8 >= 2 NA): the friction arm with xs2 only.  The second window's
  //      barrier is taken in position 7, in front of the request for position 8's operands.
  //      SOLO, NAC = 1 .. 4 (run-time option oct_sweep_na, default 1; the first iteration's sweep from position 0 where it
  //      covers all 3 NA rows — one window, or the long window): NA is a template constant, the rows are straight-line — every row's kind static, no compare, no branch —,
  //      and the normal rows' clamped impulses stay in registers for their friction rows (the stores xw[k] stay: later
  //      iterations read them): no address select, no read, no canonicalising maximum, no wait for the LDS behind the sum.
  //      The long window's second barrier stands where it stands in the generic chain: position 7, in front of position 8's
  //      request.  The same process() as the generic chain: the same expressions, contracted alike.
  auto main_sweep = [&](auto firstc, auto nac, int w0, int bo, bool lw) {
      constexpr bool FIRST = decltype(firstc)::value;
      constexpr int NAC = decltype(nac)::value;
      constexpr int KMAX = (FIRST && W2) ? 12 : 8;
      OCT_MARK("sweep");
      const T *const Zs = E + O.win + bo;
      T *const xw = E + O.xs + w0;  // the window's impulses
      const T my_hip = sw_hip, mu = sw_mu, rest = sw_rest;
      struct Ops { T zs, zm, b, a, g, hl, sd, xo; };
      auto request = [&](auto kc, Ops &o) {
        constexpr int k = decltype(kc)::value;
        const T *const row = Zs + k * OctLds::ZW;
        o.zs = row[pos];        // my dof's leg entry, if the row's contact sits on my leg
        o.zm = row[2 + lane];   // my root entry (lanes 6, 7: zero)
        o.b = row[OctLds::Z_B];
        o.a = row[OctLds::Z_A];
        o.hl = row[OctLds::Z_HL];
        if constexpr (!FIRST) {
          o.g = row[OctLds::Z_G];
          o.xo = xw[k];
        }
      };
      auto process = [&](auto kc, const Ops &o, auto normalc) -> T {
        constexpr int k = decltype(kc)::value;
        constexpr bool NORMAL = decltype(normalc)::value;
        const T zl = o.hl == my_hip ? o.zs : T(0);
        T jw;
        // (a normal row's b_r carries (1 + e) J (dt qdd): the e-fold of z~_r . (dt y~) = -z~_r . u~_init on top of what u~ holds)
        if constexpr (NORMAL) jw = oct_sum(zl * (u + rest * u_init) + o.zm * (urm + rest * urm_init));
        else jw = oct_sum(zl * u + o.zm * urm);
        // (SD_LATE: the normal row's impulse is first used HERE — tied to the sum, behind its last addition.  Left to itself the
        //  back end canonicalises it for the maximum below directly behind its request at the top of the friction arm: a wait
        //  for the whole LDS round trip — and for the next row's five operands — in front of the sum, which does not need it)
        T sd = T(0);
        if constexpr (!NORMAL) {
          sd = o.sd;
          // (NAC > 0: sd is a register of this chain, known to be canonical — pinned, it would be canonicalised again)
          if constexpr (SD_LATE && NAC == 0) asm volatile("" : "+v"(jw), "+v"(sd));
        }
        T xn;
        if constexpr (FIRST) xn = (o.b - jw) * o.a;
        else xn = (o.b - (jw - o.g * o.xo)) * o.a;
        if constexpr (NORMAL) {
          xn = max_t<T>(xn, T(0));
          xn = min_t<T>(xn, sw_cap);
        } else {
          const T hi = mu * max_t<T>(sd, T(0));  // where_lt(s, 0, 0, s)
          xn = max_t<T>(xn, -hi);
          xn = min_t<T>(xn, hi);
        }
        T dx;
        if constexpr (FIRST) dx = xn;
        else dx = xn - o.xo;
        u += zl * dx;
        urm += o.zm * dx;
        xw[k] = xn;  // (every lane the same value to the same slot)
        return xn;
      };
      Ops ops[2];
      if constexpr (NAC > 0) {
        constexpr int NR = 3 * NAC;
        // (the barrier inside the chain — position 7, where a position 8 follows — is the one the host's walk counts)
        static_assert((NR > 8 ? 1 : 0) == tds_oct_sweep_na_inner_barriers(NAC), "tds_oct_windows.h: barriers inside the specialised sweep");
        T xnorm[NAC];  // the normal rows' impulses
        request(std::integral_constant<int, 0>{}, ops[0]);
        static_for<0, NR>([&](auto kc) {
          constexpr int k = decltype(kc)::value;
          Ops &cur = ops[k & 1];
          if constexpr (k + 1 < NR) {
            if constexpr (k == 7) OCT_BAR_W(30, false);  // (the second window's barrier: NR > 8 is the long window)
            request(std::integral_constant<int, k + 1>{}, ops[(k + 1) & 1]);
          }
          // (fences: the next row's requests in front of this row's arithmetic, which covers their round trip, and none of the
          //  next row's arithmetic inside this row — left to itself the back end issues the requests behind this row's store,
          //  folds the next row's product into this row and waits for the round trip at the top of the 8-lane sum; in the
          //  generic chain the branches on the row's kind stand where the fences stand here)
          __builtin_amdgcn_sched_barrier(0);
          if constexpr (k < NAC) {
            xnorm[k] = process(kc, cur, std::true_type{});
          } else {
            cur.sd = xnorm[k < 2 * NAC ? k - NAC : k - 2 * NAC];
            process(kc, cur, std::false_type{});
          }
          __builtin_amdgcn_sched_barrier(0);
        });
        OCT_SYNC();
        OCT_MARK("sweep_end");
      } else {
        // rows 0 .. wn - 1 of the window exist, rows 0 .. k_n - 1 are normal rows, rows k_t2 .. are second tangents (compared with
        // the row index 0 .. 7 only: no clamping)
        const int wn = 3 * NA - w0, k_n = NA - w0, k_t2 = 2 * NA - w0;
        const T *const xs1 = xw - NA, *const xs2 = xw - 2 * NA;  // the impulse of a first / second tangent row's normal row
        auto rows = [&](auto self, auto kc) -> void {
          constexpr int k = decltype(kc)::value;
          if constexpr (k < 8) {
            if (k >= wn) return;
            Ops &cur = ops[k & 1];
            // (the next row's operands in front of the branch on the row's kind: requested inside both arms, the arms' loads
            //  into the same registers cost a wait each)
            if constexpr (k < 7) request(std::integral_constant<int, k + 1>{}, ops[(k + 1) & 1]);
            if (k < k_n) {
              process(kc, cur, std::true_type{});
            } else {
              cur.sd = (k >= k_t2 ? xs2 : xs1)[k];
              if constexpr (k == 7 && KMAX > 8) {
                // (the second window's barrier, in the friction arm: a long window's position 7 is a friction row — 3 NA <= 12,
                //  so k_n = NA <= 4.  Behind the request for the normal row's impulse the barrier's wait for the LDS is the one
                //  this row sits out anyway; it completes the position's own operand reads — the last reads of the first buffer —
                //  in front of the barrier, and position 8's operands then arrive under the whole of this row's arithmetic)
                if (lw) {
                  OCT_BAR_W(30, false);
                  request(std::integral_constant<int, 8>{}, ops[0]);
                }
              }
              process(kc, cur, std::false_type{});
            }
            self(self, std::integral_constant<int, k + 1>{});
          } else if constexpr (k < KMAX) {
            // positions 8 .. 11 of a long first window (position 8 exists whenever the window is long)
            if (k == 8 ? !lw : k >= wn) return;
            Ops &cur = ops[k & 1];
            if constexpr (k + 1 < KMAX) request(std::integral_constant<int, k + 1>{}, ops[(k + 1) & 1]);
            cur.sd = xs2[k];
            process(kc, cur, std::false_type{});
            self(self, std::integral_constant<int, k + 1>{});
          }
        };
        request(std::integral_constant<int, 0>{}, ops[0]);
        rows(rows, std::integral_constant<int, 0>{});
        OCT_SYNC();
        OCT_MARK("sweep_end");
      }
  };

  // (the step's done flag on every lane of the environment, for main_pool: under the Ant's rule it never passes through LDS)
  bool done_reg = false, done_in_reg = false;
  auto main_fin = [&]() {
    // ================================ main: impulse, integration, reward ================================
    OCT_MARK("main_fin");
    OCT_STAMP(6, u);
    {
      // qd_new = qd - L^-T D^-1/2 u~: forward dynamics and contact impulse in one back-substitution (see main_fd;
      // mb_constraint_solver.hpp:476-496: qd_b -= M^-1 J^T p)
      T w = u * my_sq;
      T wr[6];
      static_for<0, 6>([&](auto rc) {
        constexpr int r = decltype(rc)::value;
        wr[r] = oct_bcast<r>(urm) * sq_ids[r];  // (the root part of u~ back onto every lane)
      });
      static_for<0, 5>([&](auto ic) {
        constexpr int r = 4 - decltype(ic)::value;
        static_for<r + 1, 6>([&](auto cc) {
          constexpr int c = decltype(cc)::value;
          wr[r] -= Ls[(c * (c - 1)) / 2 + r] * wr[c];
        });
      });
#pragma unroll
      for (int r = 0; r < 6; ++r) w -= Lc[r] * wr[r];
      w -= (pos == 0 ? l10 : T(0)) * pair_bcast<1>(w);
      qd_new = qd - w;
#pragma unroll
      for (int r = 0; r < 6; ++r) qdr_new[r] = xr[nq + r] - wr[r];
    }
    OCT_MARK("main_integrate");
    // ---- M. integrate_euler: q += qd dt (integrator.hpp:126-131); the new state into the LDS record
    T qn0, qn2, qo0;  // the new base x, z and the old base x: every lane has them — the Ant's reward reads no LDS
    // (the reward rule's two constants requested here: behind the barrier below they were a round trip of their own)
    const int rm = (int)CT[TB::SC + TB::REWARD_MODE];
    const T inv_dt = CT[TB::SC + TB::INV_DT];
    OCT_SYNC();
    {
      // root coordinates: every lane holds the six velocities; lane 0 stores them and the integrated coordinates
      T qn_root[6];
#pragma unroll
      for (int r = 0; r < 6; ++r) qn_root[r] = xr[r] + qdr_new[r] * dt;
      const T q_old0 = xr[0];
      qn0 = qn_root[0];
      qn2 = qn_root[2];
      qo0 = q_old0;
      // (SOLO: the next step's constants, behind the integration's own reads — nothing waits for them in front of barrier
      //  (0), whose wait for the LDS completes them; the prologue's barrier ordered the tables' and the record's writes, and
      //  nothing writes these slots inside a launch)
      if constexpr (SOLO) top_request(xr, CL, tc);
      OCT_SYNC();
      if (lane == 0) {
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          xr[r] = qn_root[r];
          xr[nq + r] = qdr_new[r];
        }
      }
      const T q_new = q + qd_new * dt;
      xr[dq] = q_new;
      xr[nq + dq] = qd_new;
      if constexpr (SOLO) {  // (the stores above stay: the helper's records, the rows and the next launch read the record)
        car.q = q_new;
        car.qd = qd_new;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          car.rq[r] = qn_root[r];
          car.rqd[r] = qdr_new[r];
        }
      }
      if (lane == 0) {
        xr[in_dim] = q_old0;  // x_{t-1} (the Ant's reward reads it)
        xr[in_dim + 3] = T(0);  // "the y state of this step is out already" (set below for an environment the reset pool re-initialises)
      }
    }
    OCT_SYNC();
    OCT_MARK("main_reward");
    // ---- N. reward / done (ant_environment2.h:75-106; laikago_environment2.h:130-171)
    done_in_reg = rm == TDS_REWARD_ANT;
    if (rm == TDS_REWARD_ANT) {  // (wave-uniform) from registers, redundantly on every lane: (x_t - x_{t-1}) / dt, done: z < 0.26
      const T vel_x = (qn0 - qo0) * inv_dt;
      done_reg = qn2 < T(0.26);
      const T reward = done_reg ? T(0) : vel_x;
      if (lane == 0) {
        xr[in_dim + 1] = done_reg ? T(1) : T(0);
        xr[in_dim + 2] = reward;
      }
    } else {
      T rs = T(0), rc = T(1);
      if (rm == TDS_REWARD_LAIKAGO) sincos_t<T>(lane < 3 ? xr[3 + lane] * T(0.5) : T(0), &rs, &rc);  // (wave-uniform branch)
      const T s1 = oct_bcast<1>(rs), c1 = oct_bcast<1>(rc), s2 = oct_bcast<2>(rs), c2 = oct_bcast<2>(rc);
      if (lane == 0) {
        bool done = false;
        T reward = T(0);
        if (rm == TDS_REWARD_LAIKAGO) {
          const T sp = rs, cp = rc, st = s1, ct = c1, ss = s2, cs2 = c2;
          const T qx = sp * ct * cs2 - cp * st * ss;
          const T qy = cp * st * cs2 + sp * ct * ss;
          const T qz = cp * ct * ss - sp * st * cs2;
          const T qw = cp * ct * cs2 + sp * st * ss;
          const T sq = T(2) / (qx * qx + qy * qy + qz * qz + qw * qw);
          const T up = T(1) - (qx * (qx * sq) + qy * (qy * sq));
          done = (up < T(0.6)) || (xr[2] < T(0.2));
          reward = done ? T(0) : xr[0];
        }
        xr[in_dim + 1] = done ? T(1) : T(0);
        xr[in_dim + 2] = reward;
      }
    }
    OCT_SYNC();
  };
  // the state part of a y record — q | qd | (visual poses: M1) | up.z | zero padding — from the LDS record
  // (record stores are plain stores: as non-temporal stores they changed nothing, tools/experiments/r06_not_kept.txt)
  auto y_state = [&](TR *y, int end) {
    {  // (the reads in one batch in front of the stores: as a loop of read -> store every value was an LDS round trip of its own)
      constexpr int NB = (nq + nd + 7) / 8;
      T sv[NB];
#pragma unroll
      for (int k = 0; k < NB; ++k) sv[k] = xr[lane + 8 * k < nq + nd ? lane + 8 * k : 0];
#pragma unroll
      for (int k = 0; k < NB; ++k)
        if (lane + 8 * k < nq + nd) y[lane + 8 * k] = (TR)sv[k];
    }
    int tail = nq + nd;
    if ((int)CT[TB::SC + TB::PACK_VISUALS]) {
      tail += 7 * nv;
      if (lane == 0) y[tail] = (TR)(CT[TB::SC + TB::BASE_R8]);  // up_dot_world_z (fixed base)
      tail += 1;
    }
    for (int i = tail + lane; i < end; i += 8) y[i] = TR(0);
  };
  auto main_pool = [&]() {
    OCT_MARK("main_pool");
    // ---- auto_reset_when_done through the reset pool (ctl.pool; ars_vectorized_environment.h:262-277): a done environment
    //      takes its next pre-settled state — y, reward and done describe the terminal step, the observation and the state
    //      the fresh environment: its y state goes out HERE, before the record is overwritten
    const bool replaced = ctl.pool != nullptr && valid && (done_in_reg ? done_reg : xr[in_dim + 1] != T(0));
    if (replaced) {
      TR *yo, *yo2;
      int yend, yend2;
      y_where(yo, yo2, yend, yend2);
      if (yo != nullptr) {
        y_state(yo, yend);
        if (yo2 != nullptr) y_state(yo2, yend2);
      }
      const unsigned c = ctl.reset_count[env];
      const TR *const src = tds_global((const TR *)ctl.pool) + ((size_t)(c % (unsigned)ctl.pool_depth) * ctl.pool_envs + env) * (nq + nd);
      T v0 = (T)src[lane], v1 = (T)src[lane + 8], v2 = (T)src[lane + 16], v3 = T(0);
      if (lane + 24 < nq + nd) v3 = (T)src[lane + 24];
      OCT_SYNC();
      xr[lane] = v0;
      xr[lane + 8] = v1;
      xr[lane + 16] = v2;
      if (lane + 24 < nq + nd) xr[lane + 24] = v3;
      if (lane == 0) {
        ctl.reset_count[env] = c + 1u;
        xr[in_dim + 3] = T(1);
      }
    }
    if constexpr (SOLO) {
      // (the carried state of a replaced environment is the terminal step's: where any environment of the wavefront was replaced —
      //  wave-uniform, rare — every lane takes its state from the record again; the others read back what they stored)
      if (ctl.pool != nullptr && __any(replaced)) {
        OCT_SYNC();
        carry_load(xr, lane, car);
      }
    }
    OCT_MARK("main_pool_end");
    OCT_STAMP(7, tid);
  };
  auto help_rec = [&]() {
    OCT_MARK("help_rec");
    // ================================ helper: the step's records ================================
    // (two-wavefront build: while the main wavefront starts the next step — it does not write the record before its own
    //  phase M, two barriers from here)
    // ---- y record: q | qd | (visual poses: M1) | up.z | zero padding
    TR *yo, *yo2;
    int yend, yend2;
    y_where(yo, yo2, yend, yend2);
    if (valid && yo != nullptr && xr[in_dim + 3] == T(0)) {
      y_state(yo, yend);
      if (yo2 != nullptr) y_state(yo2, yend2);
    }
    // ---- [obs | reward | done] record (obs[0] = obs[1] = 0, ars_vectorized_environment.h:283-288): the slot of an obs ring
    //      (every step of a step-loop launch; floats on the multi-GPU wire format) and / or the caller's record (last step)
    if constexpr (LOOP) {
      if (OCT_HC(obs_ring) != nullptr) {  // wave-uniform
        const int slot = o_slot;
        const int rf = OCT_HC(ring_flags);
        const bool f32w = (rf & TDS_RING_OBS_F32) != 0 || sizeof(TR) == 4;
        const int np = OCT_HC(peer_arrive) != nullptr ? ctl.n_peers : 0;
        const bool rd_only = (rf & TDS_RING_PEER_REWARD_DONE) != 0;
        if (OCT_HC(peer_arrive) != nullptr && (rf & TDS_RING_WIDE) != 0 && __all(valid)) {
          // Peer-store exchange, the wavefront's eight records as one row of 8-byte units (240 scalars: 960 contiguous bytes
          // on a float wire): every lane takes 8 bytes of the row — read from the environments' LDS records, converted
          // once — and the row goes out with one 8-byte-per-lane store instruction per destination and pass: this rank's
          // own block (device scope, write-through), then every peer's (system scope, over xGMI), the table's pointers by
          // scalar loads (see tds_step_shared.h: tds_obs_store_wide, the same store)
          const int wl = tid & 63;
          const size_t row0 = ((size_t)slot * OCT_HC(obs_envs) + (size_t)blockIdx.x * 8) * (size_t)w_obs;
          const int per_unit = f32w ? 2 : 1;
          const int n_units = (8 * w_obs) / per_unit;
          const unsigned long long *const __attribute__((address_space(4))) *tab =
              (const unsigned long long *const __attribute__((address_space(4))) *)(const __attribute__((address_space(4))) void *)ctl.peer_ring;
          for (int u0 = 0; u0 < n_units; u0 += 64) {
            const int uu = u0 + wl;
            const bool on = uu < n_units;
            unsigned lo = 0u, hi = 0u;
            bool tail = false;  // this unit holds a [reward | done] column
#pragma unroll
            for (int c = 0; c < 2; ++c) {
              if (c < per_unit) {
                const int f = on ? uu * per_unit + c : 0;
                const int e = f / w_obs;
                const int i = f - e * w_obs;
                const int src = i < nq + nd ? i : (i == nq + nd ? in_dim + 2 : in_dim + 1);
                const T vv = i < 2 ? T(0) : sm[e * O.stride + src];
                tail = tail || i >= nq + nd;
                if (f32w) {
                  const unsigned b = (unsigned)__float_as_int((float)vv);
                  if (c == 0) lo = b; else hi = b;
                } else {
                  const double dv = (double)vv;
                  lo = (unsigned)__double2loint(dv);
                  hi = (unsigned)__double2hiint(dv);
                }
              }
            }
            const unsigned long long bits = ((unsigned long long)hi << 32) | (unsigned long long)lo;
            const size_t unit_at = row0 / per_unit + (size_t)uu;  // (row0 is a multiple of per_unit: TDS_RING_WIDE)
            if (on) __hip_atomic_store(tds_global((unsigned long long *)OCT_HC(obs_ring)) + unit_at, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // (reward | done only: a unit travels if ANY of its columns is one of the two — on a float wire they may share a
            //  unit with an observation column)
            const bool to_peers = on && (!rd_only || tail);
            for (int p0 = 0; p0 < np; p0 += 4) {  // (the table is padded to a multiple of four entries)
              const unsigned long long *const b0 = tds_global(tab[p0]), *const b1 = tds_global(tab[p0 + 1]), *const b2 = tds_global(tab[p0 + 2]),
                                       *const b3 = tds_global(tab[p0 + 3]);
              const size_t po = (size_t)ctl.peer_off / 8 + unit_at;
              if (to_peers) {
                using G64 = __attribute__((address_space(1))) unsigned long long;
                __hip_atomic_store((G64 *)((unsigned long long *)b0 + po), bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                if (p0 + 1 < np) __hip_atomic_store((G64 *)((unsigned long long *)b1 + po), bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                if (p0 + 2 < np) __hip_atomic_store((G64 *)((unsigned long long *)b2 + po), bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                if (p0 + 3 < np) __hip_atomic_store((G64 *)((unsigned long long *)b3 + po), bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
              }
            }
          }
        } else if (valid) {
          const size_t at = ((size_t)slot * OCT_HC(obs_envs) + env) * w_obs;
          constexpr int NB = (w_obs + 7) / 8;
          T ov[NB];  // (read in one batch: see y_state)
#pragma unroll
          for (int k = 0; k < NB; ++k) {
            const int i = lane + 8 * k;
            const T rv = xr[i >= w_obs ? 0 : (i < nq + nd ? i : (i == nq + nd ? in_dim + 2 : in_dim + 1))];
            ov[k] = i < 2 ? T(0) : rv;
          }
#pragma unroll
          for (int k = 0; k < NB; ++k) {
            const int i = lane + 8 * k;
            if (i >= w_obs) continue;
            const T vv = ov[k];
            // (TDS_RING_NOFENCE: device-scope write-through stores, visible to the exchange after a plain wait)
            if (rf & TDS_RING_OBS_F32) {
              float *const pp = tds_global((float *)OCT_HC(obs_ring)) + at + i;
              if (rf & TDS_RING_NOFENCE) __hip_atomic_store(pp, (float)vv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              else *pp = (float)vv;
            } else {
              TR *const pp = tds_global((TR *)OCT_HC(obs_ring)) + at + i;
              if (rf & TDS_RING_NOFENCE) __hip_atomic_store(pp, (TR)vv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              else *pp = (TR)vv;
            }
            if (np > 0 && (i >= nq + nd || !rd_only)) {
              for (int pr = 0; pr < np; ++pr) {
                char *const pb = (char *)tds_global(((void *const __attribute__((address_space(4))) *)(const __attribute__((address_space(4))) void *)ctl.peer_ring)[pr]) + ctl.peer_off;
                if (rf & TDS_RING_OBS_F32) __hip_atomic_store((float *)pb + (at + i), (float)vv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                else __hip_atomic_store((TR *)pb + (at + i), (TR)vv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
              }
            }
          }
        }
        // (peer-store exchange: EVERY step is counted in — the last one here, by the wavefront that has just stored it; kernel
        //  completion would tell this rank, not the peers)
        if (last && OCT_HC(peer_arrive) != nullptr) tds_signal_slot(ctl, slot);
      }
    }
    if (valid && last) {
      for (int i = lane; i < nq + nd; i += 8) {
        const TR vv = (TR)xr[i];
        if (obs_out != nullptr) obs_out[(size_t)env * w_obs + i] = i < 2 ? TR(0) : vv;
        if (x_feedback != nullptr) x_feedback[(size_t)env * in_dim + i] = vv;
      }
      if (lane == 0 && obs_out != nullptr) {
        obs_out[(size_t)env * w_obs + nq + nd] = (TR)xr[in_dim + 2];
        obs_out[(size_t)env * w_obs + nq + nd + 1] = (TR)xr[in_dim + 1];
      }
    }
    OCT_MARK("help_rec_end");
    OCT_STAMP(11, tid);
  };

  // ================================ the step ================================
  // Barriers of a two-wavefront workgroup, and who does what between them (main | helper):
  //   (0)  the step's state, reward and done are in the LDS record.
  //        PD, jcalc, kinematics (main_kin) | the records of the step before (help_rec: the main wavefront does not write the
  //        record before its own integration)
  //   (1)  the kinematics are in LDS.
  //        inertias, leg LDL^T, couplings (main_dyn) | narrowphase, the first window's geometry (help_np, rows_geom)
  //   (1b) the leg blocks' factors and couplings are in LDS.
  //        SOLO:   the root block in registers | the 21 Schur sums (help_schur)
  //          (1c)  the sums are in O.fac.
  //                the 6 x 6 LDL^T | the first window's leg stage; the next action, the exchange's count (help_poses_head)
  //        others: the Schur sums, the root block, the 6 x 6 LDL^T (main_dyn2) | the first window's leg stage, its rows parked
  //                in LDS across help_poses_head and the visual poses (help_poses)
  //   (2)  the root block's factors (main wavefront), the contact list and counts (helper) are in LDS.
  //        forward dynamics, then the sweep | the row windows, a window ahead of the sweep — a barrier per window (window wi is
  //        in LDS)
  //        integration, reward, reset pool (main_fin, main_pool) | SOLO: the visual poses (help_poses_tail); others: idle
  // LDS between (1b) and (2), SOLO: W (O.xs) is read by the helper only, in front of (1c) — the sweep's first impulse is written
  // behind the first window barrier; O.fac is written by the helper in front of (1c), read by every main lane behind it, then
  // overwritten by main lane 0 with the factors (behind an OCT_SYNC: every lane's reads are done) and read by the helper behind
  // (2); the helper's next write to it is behind (1b) of the next step.
  if constexpr (W2) {
    if (wv == 0) {
      main_kin();
      OCT_BAR_T(24);  // (1)
      main_dyn();
      OCT_BAR_T(26);  // (1b)
      main_dyn2();
      OCT_BAR_T(28);  // (2)
      main_get_count();
      main_fd();
      main_sweep_consts();
      // (the first window's root stage stays with the helper although the main wavefront holds the factors in registers: doing
      //  it here measured 1.6 k cycles on the chain against 1.1 k of waiting for the helper's)
      // (the window loops of the two wavefronts must agree — a barrier each: pgs_iters is the table's, NA the helper's)
      // (tds_oct_windows.h: the rule both loops follow, case by case)
      const int nr = 3 * NA;
      // (pgs_iters > 0 inside its loop, where alone lw is read: the condition stays on the scalar unit — NA and the launch's flags)
      const bool lw = tds_oct_long_window(NA, 1, ctl.flags & TDS_CTL_OCT_LONG_WINDOW);
      int bo = 0;
      for (int pit = 0; pit < pgs_iters; ++pit) {
        for (int w0 = 0; w0 < nr;) {
          const int nw = tds_oct_main_windows(lw, pit, w0);
          OCT_BAR_W(30, (pit | w0) == 0);
          if ((pit | w0) == 0) OCT_STAMP(12, tid);
          if (pit == 0) {
            // (SOLO: the sweep specialised for NA = 1 .. 4 — wave-uniform; tds_oct_sweep_na: the sweep that starts here covers every
            //  row of the iteration and takes the barriers the generic chain takes — none inside for one window, the long window's
            //  one in position 7.  The other builds do not instantiate the four)
            if (SOLO && tds_oct_sweep_na(NA, w0, nw, ctl.flags & TDS_CTL_OCT_SWEEP_NA)) {
              if constexpr (SOLO) {
                if (NA == 1) main_sweep(std::true_type{}, std::integral_constant<int, 1>{}, 0, 0, false);
                else if (NA == 2) main_sweep(std::true_type{}, std::integral_constant<int, 2>{}, 0, 0, false);
                else if (NA == 3) main_sweep(std::true_type{}, std::integral_constant<int, 3>{}, 0, 0, true);
                else main_sweep(std::true_type{}, std::integral_constant<int, 4>{}, 0, 0, true);
              }
            } else {
              main_sweep(std::true_type{}, std::integral_constant<int, 0>{}, w0, bo, nw == 2);
            }
          } else {
            main_sweep(std::false_type{}, std::integral_constant<int, 0>{}, w0, bo, false);
          }
          if ((pit | w0) == 0) OCT_STAMP(13, u);
          // (a long window took two windows' rows and barriers: the buffers' turn comes out where it was)
          w0 += 8 * nw;
          if (nw == 1) bo = 8 * OctLds::ZW - bo;
        }
      }
      main_fin();
      main_pool();
      OCT_BAR_T(34);  // (0)
    } else {
      OCT_BAR_T(40);  // (1)
      help_np();
      RowRegs rw = {};
      if (NA > 0) rows_geom(0, 0, rw);
      OCT_BAR_T(42);  // (1b)
      if constexpr (SOLO) {
        help_schur();
        OCT_BAR_T(52);  // (1c): once per step, whatever NA, pgs_iters, valid and last are — as the main wavefront's in main_dyn2
        // (nothing stands between the first window's leg stage and its root stage but the barrier: the rows stay in registers)
        if (NA > 0) rows_leg(0, rw);
        help_poses_head();
      } else {
        if (NA > 0) {
          rows_leg(0, rw);
          rows_park(rw);
        }
        help_poses();
        if (NA > 0) rows_fetch(rw);
      }
      OCT_BAR_T(44);  // (2)
      // (the same windows as the main wavefront's two loops, the first one — the stretch the main wavefront waits for: nothing
      //  but the factors' reads, the root stage and the barrier — taken out in front: there is one exactly when NA > 0 and
      //  pgs_iters > 0, as in the main wavefront's loops)
      if (tds_oct_help_has_windows(NA, pgs_iters)) {
        help_get_factors();
        rows_root(0, rw);
        OCT_BAR_W(46, true);
        const int nr = 3 * NA;
        int bo = 8 * OctLds::ZW;
        for (int pit = 0; pit < pgs_iters; ++pit) {
          for (int w0 = tds_oct_help_first_w0(pit); w0 < nr; w0 += 8) {
            rows_geom(w0, bo, rw);
            rows_leg(bo, rw);
            rows_root(bo, rw);
            OCT_BAR_W(46, false);
            bo = 8 * OctLds::ZW - bo;
          }
        }
      }
      // (behind the last row window, or right behind (2) where a step has none: the helper's idle tail)
      if constexpr (SOLO) help_poses_tail();
      OCT_BAR_T(50);  // (0)
      help_rec();
    }
  } else {
    main_kin();
    OCT_SYNC();
    help_np();
    help_poses();
    main_dyn();
    OCT_SYNC();
    main_dyn2();
    main_fd();
    main_sweep_consts();
    const int nr = 3 * NA;
    int bo = 0;
    for (int pit = 0; pit < pgs_iters; ++pit) {
      for (int w0 = 0; w0 < nr; w0 += 8) {
        RowRegs rw;
        rows_geom(w0, bo, rw);
        rows_leg(bo, rw);
        rows_root(bo, rw);
        OCT_SYNC();
        if (pit == 0) main_sweep(std::true_type{}, std::integral_constant<int, 0>{}, w0, bo, false);
        else main_sweep(std::false_type{}, std::integral_constant<int, 0>{}, w0, bo, false);
        bo = 8 * OctLds::ZW - bo;
      }
    }
    main_fin();
    main_pool();
    OCT_SYNC();
    help_rec();
    if constexpr (LOOP) OCT_SYNC();
  }
#ifdef TDS_OCT_PROF
  if (prof_on && (tid & 63) == 0) {
    // (main: stamps 0 .. 7 into buf[0 .. 7]; helper: stamps 8 .. 11 and the window stamp 10 into buf[8 .. 11]; one-wave: all)
    // (barriers: the main wavefront's stamps 24 .. 35, the helper's 40 .. 51 — OCT_BAR_T / OCT_BAR_W; 16 .. 23 the per-row slots
    //  of tools/oct_profile.py's row line, which no build sets at present)
#pragma unroll
    for (int k = 16; k < 24; ++k)
      if (is_main) tds_oct_prof_buf[k] = prof_t[k];
#pragma unroll
    for (int k = 0; k < 14; ++k)
      if (((k < 8 || k >= 12) && is_main) || (k >= 8 && k < 12 && is_help)) tds_oct_prof_buf[k] = prof_t[k];
    if (is_help) tds_oct_prof_buf[15] = (unsigned long long)NA;
    if (is_help) tds_oct_prof_buf[14] = prof_t[14];  // (the helper's Schur sums are stored: help_schur)
    // (barrier (1c): the main wavefront's stamps 36 / 37, the helper's 52 / 53)
#pragma unroll
    for (int k = 24; k < 38; ++k)
      if (is_main) tds_oct_prof_buf[k] = prof_t[k];
#pragma unroll
    for (int k = 40; k < 54; ++k)
      if (is_help) tds_oct_prof_buf[k] = prof_t[k];
  }
#endif
  if constexpr (LOOP) {
    act_blk = act_blk + 1 >= ctl_arg.act_blocks ? 0 : act_blk + 1;
    y_slot = y_slot + 1 >= ctl_arg.y_slots ? 0 : y_slot + 1;
    o_slot = o_slot + 1 >= ctl_arg.obs_slots ? 0 : o_slot + 1;
  }
#undef OCT_HC
  };  // ================================ end of a step ================================
  // ================================ step loop ================================
  // SOLO: each wavefront of the workgroup in a loop of its own.  What the main wavefront carries from one step into the
  // next (`car`, `tc`) is a loop-carried value of ITS loop alone: in the one loop both wavefronts pass through the loop's
  // header, the helper's path had to define the values as well, and the register allocation joined the two paths' registers
  // with up to 140 moves per step at the bottom of the loop (profiles/oct_step_boundary_resources.txt).
  if constexpr (SOLO) {
    if (__builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6) == 0) {
      for (int it = 0; it < nsteps; ++it) step_body(std::integral_constant<int, 0>{}, it);
    } else {
      for (int it = 0; it < nsteps; ++it) step_body(std::integral_constant<int, 1>{}, it);
    }
  } else {
    for (int it = 0; it < nsteps; ++it) step_body(std::integral_constant<int, 2>{}, it);
  }
#ifdef TDS_OCT_PROF
  if (threadIdx.x == 0 && blockIdx.x < 2048) {
    unsigned long long c_;
    asm volatile("s_waitcnt vmcnt(0)\n\ts_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(c_)::"memory");
    tds_oct_prof_wg[3 * blockIdx.x + 2] = c_;
  }
#endif
}

template <typename T, typename TR, bool LOOP, int BUILD>
__global__ __launch_bounds__(BUILD >= 2 ? 128 : 64) __attribute__((amdgpu_waves_per_eu(BUILD == 2 ? 2 : 1, BUILD == 2 ? 2 : 1)))
void tds_oct_kernel(const DevModel<T> *__restrict__ mdl_arg, const TR *x_in, TR *__restrict__ y_out,
                    const TR *__restrict__ actions, TR *x_feedback, TR *__restrict__ obs_out, TdsStepCtl ctl_arg, int n_envs,
                    OctOff O) {
  oct_body<T, TR, LOOP, BUILD>(mdl_arg, x_in, y_out, actions, x_feedback, obs_out, ctl_arg, n_envs, O);
}
// (amdgpu_num_vgpr counts half of the unified register file of gfx90a and later: 120 = 240 registers.  Measured with 128 — the
//  254 registers of BUILD 2, no scratch —: a pass does not start beside a chunk of BUILD 3's 254, the rate falls back to 4.45e8)
template <typename T, typename TR, bool LOOP>
__global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(2, 2), amdgpu_num_vgpr(120)))
void tds_oct_kernel_beside(const DevModel<T> *__restrict__ mdl_arg, const TR *x_in, TR *__restrict__ y_out,
                           const TR *__restrict__ actions, TR *x_feedback, TR *__restrict__ obs_out, TdsStepCtl ctl_arg,
                           int n_envs, OctOff O) {
  oct_body<T, TR, LOOP, 4>(mdl_arg, x_in, y_out, actions, x_feedback, obs_out, ctl_arg, n_envs, O);
}

}  // namespace

#ifdef TDS_OCT_PROF
extern "C" int tds_oct_prof_workgroups(unsigned long long *out, int n_wg) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(tds_oct_prof_wg), (size_t)3 * n_wg * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
extern "C" int tds_oct_prof_clocks(unsigned long long *out64) {
  return hipMemcpyFromSymbol(out64, HIP_SYMBOL(tds_oct_prof_clk), 64 * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
extern "C" int tds_oct_prof_read(unsigned long long *out64, int iter) {  // iter >= 0: which iteration the NEXT launches stamp
  if (out64 && hipMemcpyFromSymbol(out64, HIP_SYMBOL(tds_oct_prof_buf), 64 * sizeof(unsigned long long)) != hipSuccess) return -1;
  if (iter >= 0 && hipMemcpyToSymbol(HIP_SYMBOL(tds_oct_prof_iter), &iter, sizeof(int)) != hipSuccess) return -1;
  return 0;
}
#endif

// LDS bytes of one environment of the 8-lane kernel, and of one workgroup (eight environments + the constant table)
int tds_oct_lds_bytes(int input_dim) { return oct_layout(input_dim).stride * (int)sizeof(double); }
int tds_oct_workgroup_bytes(int input_dim) {
  return (oct_layout(input_dim).stride * 8 + TdsOctTab::TOTAL) * (int)sizeof(double);
}

// build: TDS_OCT_* (tds_kernels.h; which one a launch takes: tds_launch_plan.h)
template <typename T, typename TR>
int tds_launch_oct(const DevModel<T> *d_model, const DevModel<T> &h_model, const TR *x_in, TR *y_out, const TR *actions,
                   TR *x_feedback, TR *obs_out, int n_envs, hipStream_t stream, const TdsStepCtl &ctl, int build) {
  const OctOff O = oct_layout(h_model.input_dim);
  const int blocks = (n_envs + 7) / 8;
  const size_t shmem = ((size_t)O.stride * 8 + TdsOctTab::TOTAL) * sizeof(T);
  // one plain step without rings: the straight-line form; K steps, record rings: the step-loop form
  const bool one_step = ctl.nsub == 1 && ctl.obs_ring == nullptr && ctl.y_ring == nullptr;
#define OCT_LAUNCH(LOOP_, B_)                                                                                                 \
  hipLaunchKernelGGL((tds_oct_kernel<T, TR, LOOP_, B_>), dim3(blocks), dim3(B_ >= 2 ? 128 : 64), shmem, stream, d_model, x_in, \
                     y_out, actions, x_feedback, obs_out, ctl, n_envs, O)
  if (build == 4) {
    if (one_step)
      hipLaunchKernelGGL((tds_oct_kernel_beside<T, TR, false>), dim3(blocks), dim3(128), shmem, stream, d_model, x_in, y_out, actions,
                         x_feedback, obs_out, ctl, n_envs, O);
    else
      hipLaunchKernelGGL((tds_oct_kernel_beside<T, TR, true>), dim3(blocks), dim3(128), shmem, stream, d_model, x_in, y_out, actions,
                         x_feedback, obs_out, ctl, n_envs, O);
  } else if (one_step) {
    if (build == 3) OCT_LAUNCH(false, 3);
    else if (build == 2) OCT_LAUNCH(false, 2);
    else OCT_LAUNCH(false, 1);
  } else {
    if (build == 3) OCT_LAUNCH(true, 3);
    else if (build == 2) OCT_LAUNCH(true, 2);
    else OCT_LAUNCH(true, 1);
  }
#undef OCT_LAUNCH
  return (int)hipGetLastError();
}
template int tds_launch_oct<double, double>(const DevModel<double> *, const DevModel<double> &, const double *, double *,
                                            const double *, double *, double *, int, hipStream_t, const TdsStepCtl &, int);
template int tds_launch_oct<double, float>(const DevModel<double> *, const DevModel<double> &, const float *, float *,
                                           const float *, float *, float *, int, hipStream_t, const TdsStepCtl &, int);
