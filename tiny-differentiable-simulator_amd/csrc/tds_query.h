// tds_query.h — what the one-lane-per-environment query units share (tds_dyn.hip: dynamics queries, tds_ik.hip:
// inverse kinematics, tds_contact.hip: the contact query): the mapping, the record transfers of their kernels, the
// launch plan and the host checkers' stride-1 state.  The derivatives of the queries (tds_dyn_jvp.hip,
// tds_contact_jvp.hip) use the transfers and the width rule through their own driver, tds_query_dual.h.
//
// MAPPING.  One lane per environment, workgroups of W <= 64 lanes (one wavefront, narrowed so that a small batch still
// reaches every compute unit: tds_query_width), at most kQueryLanes lanes per launch and the grid's stride beyond.  An
// environment's state (the unit's layout: tds_dyn_layout, tds_ik_layout, tds_contact_layout) lives in the handle's
// work buffer laid out [component][lane], the lane minor (TdsDynMem, tds_dyn.h): every access of the recursions is
// wave-uniform in its component, so a wave reads or writes one run of W doubles.  Nothing indexed at run time is kept
// in the private segment.
// Records in HBM are [environment][component].  A workgroup brings them in and out through an LDS tile of 64 lanes x
// kTileC components (tds_query_ingest / tds_query_emit): global loads and stores walk the records in their memory
// order, so that a wave's stores are contiguous runs (512 B of each Ant's M [14][14] at a time; a whole
// [64][components] block where a record has at most 64 components), never a stride of dof_qd^2 doubles per lane.
#pragma once
#include <stdlib.h>

#include <vector>

#include "tds_diff_classes.h"
#include "tds_dyn.h"

namespace {

using namespace tds_internal;

constexpr int kTileC = 64;                // components per LDS tile
constexpr int kTileS = kTileC + 1;        // its row stride in doubles (odd: a lane's row starts on its own bank pair)
constexpr long long kQueryLanes = 16384;  // lanes of a launch at most (the work buffer: that many states of the layout)

// records [e0, e0 + nv)[nc] of `in` -> components off .. off + nc of the workgroup's lanes.  kNullIsZeros: a NULL `in`
// stands for zeros (the dynamics queries' optional inputs); a unit without such inputs carries no test for it
template <bool kNullIsZeros = false>
__device__ inline void tds_query_ingest(double *tile, TdsDynMem<double> w, int off, const double *in, int nc, int e0,
                                        int nv) {
  const int W = blockDim.x, t = threadIdx.x;
  if constexpr (kNullIsZeros)
    if (!in) {
      if (t < nv)
        for (int c = 0; c < nc; ++c) w[off + c] = 0.0;
      return;
    }
  for (int c0 = 0; c0 < nc; c0 += kTileC) {
    const int tc = nc - c0 < kTileC ? nc - c0 : kTileC;
    for (int idx = t; idx < nv * tc; idx += W) {
      const int e = idx / tc, c = idx - e * tc;
      tile[e * kTileS + c] = in[(size_t)(e0 + e) * nc + c0 + c];
    }
    __syncthreads();
    if (t < nv)
      for (int c = 0; c < tc; ++c) w[off + c0 + c] = tile[t * kTileS + c];
    __syncthreads();
  }
}

// components off .. off + nc of the workgroup's lanes -> records [e0, e0 + nv)[nc] of `out`; bad: this lane's
// environment has no valid value and its record is NaN (a literal 0 where the unit has no such case)
__device__ inline void tds_query_emit(double *tile, TdsDynMem<double> w, int off, double *out, int nc, int e0, int nv,
                                      int bad) {
  const int W = blockDim.x, t = threadIdx.x;
  for (int c0 = 0; c0 < nc; c0 += kTileC) {
    const int tc = nc - c0 < kTileC ? nc - c0 : kTileC;
    if (t < nv)
      for (int c = 0; c < tc; ++c) tile[t * kTileS + c] = bad ? __builtin_nan("") : w[off + c0 + c];
    __syncthreads();
    for (int idx = t; idx < nv * tc; idx += W) {
      const int e = idx / tc, c = idx - e * tc;
      out[(size_t)(e0 + e) * nc + c0 + c] = tile[e * kTileS + c];
    }
    __syncthreads();
  }
}

// The two transfers for records that are `stride` doubles apart in HBM (one direction's [nc] of [n][k][nc], or the
// leading part of a wider record): `in` / `out` point at environment 0's record.  (Functions of their own, so that the
// kernels of the contiguous transfers above keep their code.)
__device__ inline void tds_query_ingest_strided(double *tile, TdsDynMem<double> w, int off, const double *in, int nc,
                                                size_t stride, int e0, int nv) {
  const int W = blockDim.x, t = threadIdx.x;
  for (int c0 = 0; c0 < nc; c0 += kTileC) {
    const int tc = nc - c0 < kTileC ? nc - c0 : kTileC;
    for (int idx = t; idx < nv * tc; idx += W) {
      const int e = idx / tc, c = idx - e * tc;
      tile[e * kTileS + c] = in[(size_t)(e0 + e) * stride + c0 + c];
    }
    __syncthreads();
    if (t < nv)
      for (int c = 0; c < tc; ++c) w[off + c0 + c] = tile[t * kTileS + c];
    __syncthreads();
  }
}
__device__ inline void tds_query_emit_strided(double *tile, TdsDynMem<double> w, int off, double *out, int nc,
                                              size_t stride, int e0, int nv, int bad) {
  const int W = blockDim.x, t = threadIdx.x;
  for (int c0 = 0; c0 < nc; c0 += kTileC) {
    const int tc = nc - c0 < kTileC ? nc - c0 : kTileC;
    if (t < nv)
      for (int c = 0; c < tc; ++c) tile[t * kTileS + c] = bad ? __builtin_nan("") : w[off + c0 + c];
    __syncthreads();
    for (int idx = t; idx < nv * tc; idx += W) {
      const int e = idx / tc, c = idx - e * tc;
      out[(size_t)(e0 + e) * stride + c0 + c] = tile[e * kTileS + c];
    }
    __syncthreads();
  }
}

// lanes per workgroup: the widest of 64, 32, 16 that still gives every compute unit a workgroup (a lane's recursions
// are one long dependent chain: a batch of 4096 on 64 of 256 compute units takes as long as one four times its size).
// TDS_HIP_DYN_WIDTH (16, 32, 64) overrides the rule, for measurements; it is read at every call.
inline int tds_query_width(const tds_hip_sim *s, int n) {
  if (const char *e = getenv("TDS_HIP_DYN_WIDTH")) {
    const int v = atoi(e);
    if (v == 16 || v == 32 || v == 64) return v;
  }
  int W = 64;
  while (W > 16 && (n + W - 1) / W < s->num_cus) W /= 2;
  return W;
}

// a launch over n environments whose state has `total` components: workgroups of W lanes, `blocks` of them, `lanes` =
// blocks W states in the work buffer
struct TdsQueryPlan {
  int W;
  long long blocks, lanes;
};

// plans the launch and grows the handle's work buffer to its lanes' states (shared with the step derivatives: calls on
// the stream use it in turn); the kernel takes (args, (double *)s->d_diff_tmp, (int)lanes)
inline int tds_query_plan(tds_hip_sim *s, int n, int total, TdsQueryPlan *p) {
  p->W = tds_query_width(s, n);
  p->blocks = ((long long)n + p->W - 1) / p->W;
  if (p->blocks > kQueryLanes / p->W) p->blocks = kQueryLanes / p->W;
  p->lanes = p->blocks * p->W;
  return tds_work_buffer(s, ((size_t)p->lanes * total * sizeof(double) + 255) & ~(size_t)255);
}

// the host checkers' state: one environment at a time in a vector of its own (stride 1)
struct TdsQueryHost {
  std::vector<double> buf;
  TdsDynMem<double> w;
  explicit TdsQueryHost(int total) : buf(total, 0.0), w{buf.data(), 1} {}
  // record e of src[.][nc] -> components off .. (src NULL: zeros)
  void put(int off, const double *src, int nc, int e) {
    for (int c = 0; c < nc; ++c) buf[off + c] = src ? src[(size_t)e * nc + c] : 0.0;
  }
  // components off .. -> record e of dst[.][nc] (dst NULL: nothing; nan: the record is NaN)
  void get(int off, void *dst, int nc, int e, int nan = 0) const {
    if (dst)
      for (int c = 0; c < nc; ++c) ((double *)dst)[(size_t)e * nc + c] = nan ? __builtin_nan("") : buf[off + c];
  }
};

}  // namespace
