// tds_step_shared.h — device code that the step kernels share (tds_kernels.hip, tds_oct.hip, tds_chain.hip, tds_quad.hip):
// the small helpers every one of them needs, and the multi-GPU layer's device side (tds_shard.hip) for the kernels that can
// take it from here at no cost: the arrival counting of the peer-store exchange with its flag stores and the progress counters
// of the RCCL forms (8-lane and serial-chain kernel), and the stores of a step's [obs | reward | done] records into the obs
// ring of this rank and of every peer (serial-chain kernel).  What stays local, and why, is said at each piece.  Function templates,
// inlined where a kernel calls them; `ctl` arrives as a template parameter, so that the plain `const TdsStepCtl &` of the
// straight-line builds and the constant-address-space reference of the step-loop builds (TdsCtlRef) pass unchanged.
#pragma once
#include <hip/hip_runtime.h>

#include "tds_kernels.h"

#define TDS_AS4 __attribute__((address_space(4)))

// A pointer that was LOADED (a field of the kernel-argument structs read through the laundered segment pointer, an entry of a
// pointer table) has no address space the compiler could know: its accesses are FLAT instructions — both counters, out of
// order with the DS instructions, and a flat LOAD (the action block requested a step ahead) holds the next LDS wait until it
// has returned from memory.  tds_global() says "global memory" (an assumption `neither LDS nor scratch`, which the
// address-space inference pass turns into address space 1 for every access derived from the pointer).
template <typename P>
__device__ __forceinline__ P *tds_global(P *p) {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_assume(!__builtin_amdgcn_is_shared((const void *)p) && !__builtin_amdgcn_is_private((const void *)p));
#endif
  return p;
}

// A struct of the kernel arguments as the step reads it: the parameter itself in the straight-line builds; in the step-loop
// builds a reference INTO THE KERNEL-ARGUMENT SEGMENT (constant address space: scalar loads that hit the scalar cache), so
// that a field lives from its first use in an iteration to its last instead of across the loop (tds_kernels.hip: TdsKernArgs)
template <bool LOOP, typename S>
struct TdsKaRef {
  using type = const S &;
  static __device__ __forceinline__ type get(const S &param, const TDS_AS4 char *) { return param; }
};
template <typename S>
struct TdsKaRef<true, S> {
  using type = const TDS_AS4 S &;
  static __device__ __forceinline__ type get(const S &, const TDS_AS4 char *at) { return *(const TDS_AS4 S *)at; }
};
template <bool LOOP>
using TdsCtlRef = TdsKaRef<LOOP, TdsStepCtl>;

// sin and cos of a joint angle: Cody-Waite reduction by pi / 2 in two fused steps (exact for |x| < 1e5: the product k * hi is
// formed exactly inside the FMA and cancels against x) and the fdlibm kernels on [-pi/4, pi/4] (__kernel_sin / __kernel_cos:
// < 1 ulp) — ~35 instructions where the library routine takes ~90 with its branch to the Payne-Hanek reduction; angles
// beyond 1e5 rad (no simulation gets there, but a caller may hand in anything) take the library routine
static __device__ __forceinline__ void tds_sincos(double x, double *sn, double *cs) {
  const bool big = !(__builtin_fabs(x) < 1.0e5);
  const double k = __builtin_rint(x * 6.36619772367581382433e-01);
  double r = __builtin_fma(-k, 1.57079632679489655800e+00, x);
  r = __builtin_fma(-k, 6.12323399573676603587e-17, r);
  const int q = (int)k;
  const double z = r * r;
  double ps = __builtin_fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08);
  ps = __builtin_fma(z, ps, 2.75573137070700676789e-06);
  ps = __builtin_fma(z, ps, -1.98412698298579493134e-04);
  ps = __builtin_fma(z, ps, 8.33333333332248946124e-03);
  ps = __builtin_fma(z, ps, -1.66666666666666324348e-01);
  const double s0 = __builtin_fma(z * r, ps, r);
  double pc = __builtin_fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09);
  pc = __builtin_fma(z, pc, -2.75573143513906633035e-07);
  pc = __builtin_fma(z, pc, 2.48015872894767294178e-05);
  pc = __builtin_fma(z, pc, -1.38888888888741095749e-03);
  pc = __builtin_fma(z, pc, 4.16666666666666019037e-02);
  const double c0 = __builtin_fma(z * z, pc, __builtin_fma(z, -0.5, 1.0));
  const bool swap = (q & 1) != 0;
  const double ss = swap ? c0 : s0, cc = swap ? s0 : c0;
  double s_ = (q & 2) ? -ss : ss, c_ = ((q + 1) & 2) ? -cc : cc;
  // (the lanes beyond 1e5 — or NaN — take the library routine; the OTHER lanes of the wavefront keep their own result: an
  //  environment's bits must not depend on a wavefront-mate that has left the finite range)
  if (__builtin_expect(__any(big), 0)) {
    double s2, c2;
    sincos(x, &s2, &c2);
    s_ = big ? s2 : s_;
    c_ = big ? c2 : c_;
  }
  *sn = s_;
  *cs = c_;
}
static __device__ __forceinline__ void tds_sincos(float x, float *sn, float *cs) { sincosf(x, sn, cs); }

// tds_sincos of TWO arguments in one evaluation: per argument the operations of tds_sincos in its order — the same bits —
// the two chains interleaved statement by statement, so that each of the 17 constants is named once in one block (a VOP3 f64
// operand cannot be a 64-bit literal: a constant is two moves into a register pair wherever a copy of the routine stands;
// tds_oct.hip: the joint's angle and the root's, both known at the top of the step).  The fallback keeps its rule per
// argument: a lane beyond 1e5 (or NaN) takes the library routine for THAT argument only.
static __device__ __forceinline__ void tds_sincos2(double xa, double xb, double *sa, double *ca, double *sb, double *cb) {
  const bool biga = !(__builtin_fabs(xa) < 1.0e5), bigb = !(__builtin_fabs(xb) < 1.0e5);
  const double ka = __builtin_rint(xa * 6.36619772367581382433e-01), kb = __builtin_rint(xb * 6.36619772367581382433e-01);
  double ra = __builtin_fma(-ka, 1.57079632679489655800e+00, xa), rb = __builtin_fma(-kb, 1.57079632679489655800e+00, xb);
  ra = __builtin_fma(-ka, 6.12323399573676603587e-17, ra);
  rb = __builtin_fma(-kb, 6.12323399573676603587e-17, rb);
  const int qa = (int)ka, qb = (int)kb;
  const double za = ra * ra, zb = rb * rb;
  double psa = __builtin_fma(za, 1.58969099521155010221e-10, -2.50507602534068634195e-08);
  double psb = __builtin_fma(zb, 1.58969099521155010221e-10, -2.50507602534068634195e-08);
  psa = __builtin_fma(za, psa, 2.75573137070700676789e-06);
  psb = __builtin_fma(zb, psb, 2.75573137070700676789e-06);
  psa = __builtin_fma(za, psa, -1.98412698298579493134e-04);
  psb = __builtin_fma(zb, psb, -1.98412698298579493134e-04);
  psa = __builtin_fma(za, psa, 8.33333333332248946124e-03);
  psb = __builtin_fma(zb, psb, 8.33333333332248946124e-03);
  psa = __builtin_fma(za, psa, -1.66666666666666324348e-01);
  psb = __builtin_fma(zb, psb, -1.66666666666666324348e-01);
  const double s0a = __builtin_fma(za * ra, psa, ra), s0b = __builtin_fma(zb * rb, psb, rb);
  double pca = __builtin_fma(za, -1.13596475577881948265e-11, 2.08757232129817482790e-09);
  double pcb = __builtin_fma(zb, -1.13596475577881948265e-11, 2.08757232129817482790e-09);
  pca = __builtin_fma(za, pca, -2.75573143513906633035e-07);
  pcb = __builtin_fma(zb, pcb, -2.75573143513906633035e-07);
  pca = __builtin_fma(za, pca, 2.48015872894767294178e-05);
  pcb = __builtin_fma(zb, pcb, 2.48015872894767294178e-05);
  pca = __builtin_fma(za, pca, -1.38888888888741095749e-03);
  pcb = __builtin_fma(zb, pcb, -1.38888888888741095749e-03);
  pca = __builtin_fma(za, pca, 4.16666666666666019037e-02);
  pcb = __builtin_fma(zb, pcb, 4.16666666666666019037e-02);
  const double c0a = __builtin_fma(za * za, pca, __builtin_fma(za, -0.5, 1.0));
  const double c0b = __builtin_fma(zb * zb, pcb, __builtin_fma(zb, -0.5, 1.0));
  const bool swapa = (qa & 1) != 0, swapb = (qb & 1) != 0;
  const double ssa = swapa ? c0a : s0a, cca = swapa ? s0a : c0a;
  const double ssb = swapb ? c0b : s0b, ccb = swapb ? s0b : c0b;
  double sa_ = (qa & 2) ? -ssa : ssa, ca_ = ((qa + 1) & 2) ? -cca : cca;
  double sb_ = (qb & 2) ? -ssb : ssb, cb_ = ((qb + 1) & 2) ? -ccb : ccb;
  // (ONE branch behind both chains, the two arguments' own tests inside it: with a branch per argument the back end sinks the
  //  second chain behind the first branch — two blocks, and the constants are moved into registers once per block again)
  if (__builtin_expect(__any(biga || bigb), 0)) {
    if (__any(biga)) {
      double s2, c2;
      sincos(xa, &s2, &c2);
      sa_ = biga ? s2 : sa_;
      ca_ = biga ? c2 : ca_;
    }
    if (__any(bigb)) {
      double s2, c2;
      sincos(xb, &s2, &c2);
      sb_ = bigb ? s2 : sb_;
      cb_ = bigb ? c2 : cb_;
    }
  }
  *sa = sa_;
  *ca = ca_;
  *sb = sb_;
  *cb = cb_;
}
static __device__ __forceinline__ void tds_sincos2(float xa, float xb, float *sa, float *ca, float *sb, float *cb) {
  sincosf(xa, sa, ca);
  sincosf(xb, sb, cb);
}

// ---------------------------------------------------------------------------------------------------------------------------
// A step's records are out: the wavefront that stored them counts its workgroup in.
//
// RCCL forms (TdsStepCtl::progress — what the exchange of the multi-GPU layer polls, tds_shard.hip): one counter PER RING SLOT
// (progress[slot]).  The workgroups of a launch run at their own pace — a wavefront whose environments carry more contacts
// falls steps behind the others over a long launch — so a single running total says nothing about the slowest workgroup; the
// slot's own counter reaches (uses of the slot) x (workgroups) exactly when EVERY workgroup has stored its records of that step.
//
// Peer-store exchange (TdsStepCtl::peer_arrive): this workgroup's records of ring slot `pslot` are out — acknowledged by the
// memory they went to, this rank's and the peers' — so it counts itself in on the slot's arrival counters; the workgroup that
// completes the slot raises the slot's flag of THIS rank on every rank, its own included, to the launch's sequence number.
// Every store of every workgroup was acknowledged before that workgroup's count, and the flag stores are issued after the last
// count returned: a rank that sees the flag sees the records.
// Two levels (tds_kernels.h: TDS_PEER_SUB): workgroup b on first-level counter b mod SUB, whoever completes one on the second
// level; every counter wraps at its own count (atomicInc: never reset) and lives on a line of its own.
//
// In two pieces, because the 8-lane kernel's helper wavefront issues the first-level atomic at one place of its step and looks
// at the result at another (tds_oct.hip: help_np / help_poses); everybody else calls tds_signal_slot.
// Called by the 8-lane and the serial-chain kernel.  The general kernel keeps its own text of the same protocol
// (tds_kernels.hip: peer_signal / signal_progress, with FLAT counter atomics as it always had): with these functions inlined,
// in whichever shape, some of its builds that hold 256 registers spilled more (profiles/step_shared_static_and_ab.txt).
// ---------------------------------------------------------------------------------------------------------------------------
// count in: wait for the stores' acknowledgement, first-level count; returns the token tds_peer_finish wants
template <typename CTL>
__device__ __forceinline__ unsigned tds_peer_count_in(const CTL &ctl, int pslot) {
  __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0): every store of this wavefront acknowledged by the memory it went to
  if ((ctl.ring_flags & TDS_RING_PEER_RELEASE) != 0) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // (A/B switch for the first run on a fabric: tds_kernels.h)
  unsigned tok = 0u;
  if ((threadIdx.x & 63) == 0) {
    constexpr unsigned SUB = TDS_PEER_SUB;
    const unsigned g = gridDim.x, j = blockIdx.x % SUB;
    const unsigned n1 = (g - j + SUB - 1u) / SUB;  // workgroups that count on first-level counter j
    unsigned *const base = tds_global(ctl.peer_arrive) + (size_t)pslot * TDS_PEER_ARRIVE_STRIDE;
    tok = atomicInc(base + j * TDS_PEER_LINE, n1 - 1u);
  }
  return tok;
}
// finish: whoever completed a first-level counter counts on the second level, whoever completes that raises the flags
template <typename CTL>
__device__ __forceinline__ void tds_peer_finish(const CTL &ctl, int pslot, unsigned tok) {
  if ((threadIdx.x & 63) == 0) {
    constexpr unsigned SUB = TDS_PEER_SUB;
    const unsigned g = gridDim.x, j = blockIdx.x % SUB;
    const unsigned n1 = (g - j + SUB - 1u) / SUB;
    const unsigned n2 = g < SUB ? g : SUB;  // first-level counters in use
    unsigned *const base = tds_global(ctl.peer_arrive) + (size_t)pslot * TDS_PEER_ARRIVE_STRIDE;
    if (tok == n1 - 1u) {
      if (atomicInc(base + 32 * TDS_PEER_LINE, n2 - 1u) == n2 - 1u) {
        const size_t fi = (size_t)ctl.peer_flag_off + (size_t)pslot * (size_t)ctl.peer_flag_stride;
        if ((ctl.ring_flags & TDS_RING_PEER_RELEASE) != 0) __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "");
        for (int pr = 0; pr <= ctl.n_peers; ++pr)
          __hip_atomic_store(ctl.peer_flags[pr] + fi, ctl.peer_epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
  }
}
// the records of ring slot `pslot` counted in, whichever form the launch uses (wave-uniform branches: kernel arguments)
template <typename CTL>
__device__ __forceinline__ void tds_signal_slot(const CTL &ctl, int pslot) {
  if (ctl.peer_arrive != nullptr) {
    tds_peer_finish(ctl, pslot, tds_peer_count_in(ctl, pslot));
  } else if (ctl.progress != nullptr) {
    if (ctl.ring_flags & TDS_RING_NOFENCE)
      __builtin_amdgcn_s_waitcnt(0x0f70);  // vmcnt(0): the obs ring's write-through stores have reached the L2 / memory
    else
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    if ((threadIdx.x & 63) == 0)
      __hip_atomic_fetch_add(tds_global(ctl.progress) + pslot, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The [obs | reward | done] records of ring slot `slot`: w = nq + nd + 2 scalars per environment, obs = [q | qd] with
// obs[0] = obs[1] = 0 (ars_vectorized_environment.h:250-289).  The kernel hands in a callable that returns column i from its
// LDS record — columns w - 2 and w - 1 are reward and done, wherever the kernel keeps them: `col(e, i)` of environment e of the
// WAVEFRONT for the wide row, `col(i)` of the lane's own environment for the scalar form.
// Peer-store exchange: the same bits go into the same place of every peer's gathered ring — system-scope write-through stores
// into memory mapped from the other ranks (over xGMI) — by the wavefront that stores the record anyway.  With
// exchange_fields = 1 (TDS_RING_PEER_REWARD_DONE) only reward and done travel: tds_obs_travels.
// Called by the serial-chain kernel.  The general and the 8-lane kernel keep their own text of the same two stores
// (tds_kernels.hip: put_obs / put_obs_wide, tds_oct.hip: help_rec): inlined from here the stores cost the Ant x 4096 lines
// 0.2 - 0.4 % and the general kernel's spilling builds a scratch slot (profiles/step_shared_static_and_ab.txt).
// ---------------------------------------------------------------------------------------------------------------------------
static __device__ __forceinline__ bool tds_obs_travels(int ring_flags, bool reward_or_done) {
  return reward_or_done || (ring_flags & TDS_RING_PEER_REWARD_DONE) == 0;
}

// The whole WAVEFRONT'S records as one burst (TDS_RING_WIDE: every stride of the ring is a multiple of 8 bytes; every
// environment of the wavefront stores).  The EPW environments of a wavefront own consecutive records of a slot: EPW x w scalars
// in a row (Ant, float wire: 960 bytes from 8 environments, 480 from 4).  Lane-per-component stores cut that row into 2 EPW pieces per destination; here every
// lane takes 8 bytes of the row — read from the environments' LDS records, converted once — and the row goes out with ONE
// 8-byte-per-lane store instruction per destination and pass (one pass on a float wire up to 128 scalars per wavefront), whole
// and in order: what a write-through store into another GPU's memory wants to look like on the fabric.  Destinations: this
// rank's own block (device scope), then every peer's (system scope), the table's pointers fetched four at a time.
// wl: the lane's index in its wavefront, as the kernel holds it (the step-loop builds launder theirs per iteration: derived
// from threadIdx.x here, a second copy lives across the loop — 4 VGPRs spilled in the 8-lane kernel's float-record builds).
// W: the record width where the kernel knows it at compile time (unit -> environment is then a division by a constant),
// 0 where it does not (EPW - 1 compares on `w` instead of a division at run time).
template <int EPW, int W, typename TR, typename CTL, typename COL>
__device__ __forceinline__ void tds_obs_store_wide(const CTL &ctl, int slot, int wl, int w_rt, COL col) {
  using T = decltype(col(0, 0));
  const int w = W > 0 ? W : w_rt;
  const int rf = ctl.ring_flags;
  const size_t row0 = ((size_t)slot * ctl.obs_envs + (size_t)blockIdx.x * EPW) * (size_t)w;  // first scalar of the wavefront's row
  const bool f32w = (rf & TDS_RING_OBS_F32) != 0 || sizeof(TR) == 4;
  const int per_unit = f32w ? 2 : 1;  // scalars per 8-byte unit
  const int n_units = (EPW * w) / per_unit;
  const int np = ctl.n_peers;
  // (the pointer table is read through the CONSTANT address space — written once at set-up, uniform index: scalar loads.
  //  As vector loads each pointer was fetched right in front of its store, and the wait for it — loads and stores return
  //  through one in-order counter — was a wait for the acknowledgement of the PREVIOUS peer's row: the seven rows of an
  //  8-GPU run went out one after the other, 2.3 us per step)
  const unsigned long long *const TDS_AS4 *tab = (const unsigned long long *const TDS_AS4 *)(const TDS_AS4 void *)ctl.peer_ring;
  for (int u0 = 0; u0 < n_units; u0 += 64) {
    const int u = u0 + wl;
    const bool on = u < n_units;
    unsigned lo = 0u, hi = 0u;
    bool tail = false;  // this unit holds a [reward | done] column (with exchange_fields = 1 a unit travels if ANY of its
                        // columns is one of the two: on a float wire with an odd record width they share units with
                        // observation columns — floating-base and spherical models)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      if (c < per_unit) {
        const int f = on ? u * per_unit + c : 0;
        int e = 0;
        if constexpr (W > 0) {
          e = f / W;
        } else {
#pragma unroll
          for (int k = 1; k < EPW; ++k) e += f >= k * w ? 1 : 0;
        }
        const int i = f - e * w;
        const T v = i < 2 ? T(0) : col(e, i);
        tail = tail || i >= w - 2;
        if (f32w) {
          const unsigned b = (unsigned)__float_as_int((float)v);
          if (c == 0) lo = b; else hi = b;
        } else {
          const double dv = (double)v;
          lo = (unsigned)__double2loint(dv);
          hi = (unsigned)__double2hiint(dv);
        }
      }
    }
    const unsigned long long bits = ((unsigned long long)hi << 32) | (unsigned long long)lo;
    const size_t unit_at = row0 / per_unit + (size_t)u;  // (row0 is a multiple of per_unit: TDS_RING_WIDE)
    if (on) __hip_atomic_store(tds_global((unsigned long long *)ctl.obs_ring) + unit_at, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool to_peers = on && tds_obs_travels(rf, tail);
    for (int p0 = 0; p0 < np; p0 += 4) {  // (the table is padded to a multiple of four entries)
      const unsigned long long *const b0 = tds_global(tab[p0]), *const b1 = tds_global(tab[p0 + 1]), *const b2 = tds_global(tab[p0 + 2]),
                               *const b3 = tds_global(tab[p0 + 3]);
      const size_t po = (size_t)ctl.peer_off / 8 + unit_at;
      if (to_peers) {
        // (stores through explicitly global pointers: as generic ones they were FLAT stores)
        using G64 = __attribute__((address_space(1))) unsigned long long;
        __hip_atomic_store((G64 *)((unsigned long long *)b0 + po), bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (p0 + 1 < np) __hip_atomic_store((G64 *)((unsigned long long *)b1 + po), bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (p0 + 2 < np) __hip_atomic_store((G64 *)((unsigned long long *)b2 + po), bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (p0 + 3 < np) __hip_atomic_store((G64 *)((unsigned long long *)b3 + po), bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
  }
}

// One scalar per lane and pass, for ragged wavefronts and launches without peers: environment `env` of the launch, stored
// by its G lanes (`lane` = 0 .. G - 1).  Own ring: float or record dtype; a device-scope write-through store that needs no
// cache write-back to become visible to the exchange (TDS_RING_NOFENCE), or the kernel's own kind of plain store,
// `plain(value, pointer)`.  Then the same scalar into every peer's ring.
template <int G, typename TR, typename CTL, typename COL, typename ST>
__device__ __forceinline__ void tds_obs_store_scalar(const CTL &ctl, int slot, int env, int lane, int w, COL col, ST plain) {
  using T = decltype(col(0));
  const size_t at = ((size_t)slot * ctl.obs_envs + env) * w;
  const int rf = ctl.ring_flags;
  const int np = ctl.peer_arrive != nullptr ? ctl.n_peers : 0;  // wave-uniform (kernel arguments)
  for (int i = lane; i < w; i += G) {
    const T v = i < 2 ? T(0) : col(i);
    if (rf & TDS_RING_OBS_F32) {
      float *const p = tds_global((float *)ctl.obs_ring) + at + i;
      if (rf & TDS_RING_NOFENCE) __hip_atomic_store(p, (float)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else plain((float)v, p);
    } else {
      TR *const p = tds_global((TR *)ctl.obs_ring) + at + i;
      if (rf & TDS_RING_NOFENCE) __hip_atomic_store(p, (TR)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      else plain((TR)v, p);
    }
    if (np > 0 && tds_obs_travels(rf, i >= w - 2)) {
      for (int pr = 0; pr < np; ++pr) {
        char *const pb = (char *)tds_global(((void *const TDS_AS4 *)(const TDS_AS4 void *)ctl.peer_ring)[pr]) + ctl.peer_off;  // (scalar loads: see tds_obs_store_wide)
        if (rf & TDS_RING_OBS_F32) __hip_atomic_store((float *)pb + (at + i), (float)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        else __hip_atomic_store((TR *)pb + (at + i), (TR)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
  }
}
