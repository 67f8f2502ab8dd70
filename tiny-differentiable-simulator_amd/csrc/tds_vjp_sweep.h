// tds_vjp_sweep.h — the device's reverse sweep of one tape over TdsRev (tds_rev.h), written once for the step and
// parameter VJPs (tds_vjp_kernels.h) and for the chained sweeps of the rollout VJPs (tds_rollout_vjp.h).  It depends on
// tds_rev.h alone, so both libraries' units can take it.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "tds_rev.h"

namespace {

// The device's sweep.  The adjoint of a variable is split in two parts: contributions from entries less than kVjpRing
// positions later (the near part) go to a ring of kVjpRing slots per lane in LDS; the rest (the far part: inputs,
// seeds, long-range uses) go to the lane's adjoints in the work buffer as atomic adds, which the sweep does not wait
// for.  Entries, partials and far parts are loaded a block of kVjpBlock positions ahead of the block being swept:
// every far contribution to a loaded position comes from a position at least kVjpRing later, already swept.  A block
// is swept without data-dependent branches (positions outside the lane's tape contribute zeros), and both parts are
// accumulated by atomic adds without return (LDS; memory, only where some lane has a far contribution): the only wait
// per entry is the LDS read of its own adjoint.  The ring takes 128 KB of the CU's 160 KB of LDS.
constexpr int kVjpRing = 256, kVjpBlock = 8;
static_assert(kVjpRing >= 2 * kVjpBlock, "the far parts of the block loaded ahead are complete when it is loaded");
static_assert((kVjpRing & (kVjpRing - 1)) == 0, "ring slots are taken with a mask");

struct TdsVjpBlk {
  TdsRevIdx e[kVjpBlock];
  TdsRevPart d[kVjpBlock];
  double far[kVjpBlock];
};

// positions p0, p0 - 1, ..., p0 - kVjpBlock + 1 (those below 0 load position 0: they are not swept)
__device__ inline void tds_vjp_load(const TdsRevTape &t, int l, int p0, TdsVjpBlk &b) {
#pragma unroll
  for (int j = 0; j < kVjpBlock; ++j) {
    const long long p = max(p0 - j, 0);
    b.e[j] = t.ix[p * 64 + l];
    b.d[j] = t.pd[p * 64 + l];
    b.far[j] = __hip_atomic_load(t.adj + (t.n_in + p) * 64 + l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// c into the adjoint of v, from the entry whose result is r: the near part (LDS) or the far part (atomic add); the
// other part gets zero
__device__ inline void tds_vjp_add(const TdsRevTape &t, double *ring_l, int l, int v, int r, double c) {
  const bool near = v >= t.n_in && v > r - kVjpRing;
  // LDS atomic add without return: the sweep does not wait for it (LDS keeps a wavefront's operations in order)
  __hip_atomic_fetch_add(ring_l + (v & (kVjpRing - 1)) * 64, near ? c : 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  if (!near && c != 0.0) unsafeAtomicAdd(t.adj + (long long)v * 64 + l, c);  // skipped where no lane has one
}

// sweep positions p0 .. p0 - kVjpBlock + 1 of a lane whose tape has len entries
__device__ inline void tds_vjp_block(const TdsRevTape &t, double *ring_l, int l, int p0, int len, const TdsVjpBlk &b) {
#pragma unroll
  for (int j = 0; j < kVjpBlock; ++j) {
    const int p = p0 - j, r = t.n_in + p;
    const bool valid = p >= 0 && p < len;
    double *slot = ring_l + (r & (kVjpRing - 1)) * 64;
    const double g = *slot + b.far[j];
    *slot = 0.0;  // the slot's next variable, r - kVjpRing, gets its first near contribution after this
    // the far part back to zero for the next sweep (p < 0: no variable of the tape)
    if (p >= 0 && b.far[j] != 0.0)
      __hip_atomic_store(t.adj + (long long)r * 64 + l, 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool two = valid && b.e[j].b >= 0;
    tds_vjp_add(t, ring_l, l, valid ? b.e[j].a : 0, r, valid ? b.d[j].da * g : 0.0);
    tds_vjp_add(t, ring_l, l, two ? b.e[j].b : 0, r, two ? b.d[j].db * g : 0.0);
  }
}

// the sweep of one lane, from the wavefront's longest tape (top) down: the lanes of a wavefront walk the same positions
__device__ inline void tds_vjp_sweep(const TdsRevTape &t, double *ring_l, int l, int len, int top) {
  TdsVjpBlk A, B;
  tds_vjp_load(t, l, top - 1, A);
  for (int p0 = top - 1; p0 >= 0; p0 -= 2 * kVjpBlock) {
    tds_vjp_load(t, l, p0 - kVjpBlock, B);
    tds_vjp_block(t, ring_l, l, p0, len, A);
    tds_vjp_load(t, l, p0 - 2 * kVjpBlock, A);
    tds_vjp_block(t, ring_l, l, p0 - kVjpBlock, len, B);
  }
}

// the regions of a work buffer start on 256 B
inline size_t tds_vjp_align(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace
