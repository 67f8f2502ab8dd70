// tds_oct_windows.h — how the two wavefronts of an 8-lane workgroup (tds_oct.hip) walk the row windows of a step's contact
// sweep, and how many window barriers each of them takes on the way.  ONE rule for both sides: a mismatch between the two
// counts is a workgroup that never leaves s_barrier.  Host and device; tds_hip_oct_window_plan_host asks it on the CPU.
//
// The sweep visits the 3 NA constraint rows of a wavefront (NA: the largest contact count among its eight environments,
// wave-uniform) pgs_iters times, in windows of eight sweep positions; window by window the helper solves the rows (lane ==
// row) into one of TWO row buffers that take turns, and the main wavefront sweeps them.  A window barrier says "the rows of
// the next window are in LDS"; because main and helper take the barriers in the same order it also says "the main wavefront
// has read everything it needs of the buffer the helper writes next".
//
// The LONG first window (option oct_long_window, default on; two-wavefront builds, first iteration): with 8 < 3 NA <= 12 the
// second window holds one to four rows, all of them second-tangent rows (positions >= 8 >= 2 NA).  The main wavefront then
// does not return to its window loop behind position 7: its unrolled chain runs on through positions 8 .. 3 NA - 1, which
// lie in the second buffer at the same immediate offsets off the same base (the two buffers are contiguous), and it takes the
// second window's barrier INSIDE the chain, in position 7, in front of the request for position 8's operands.  (Position 7 of
// a long window is a friction row, 3 NA <= 12 means NA <= 4 < 7, and the barrier sits in that row's friction arm: whoever
// widens the condition below must move it.)  It is still one barrier per window for either wavefront; the main wavefront's
// loop advances by two windows.
//
// The cases (M: main wavefront, H: helper; b = a window barrier; nw = ceil(3 NA / 8)):
//   pgs_iters = 0, any NA:    neither loop is entered (H: its first window is guarded by pgs_iters > 0).       M 0 = H 0.
//   NA = 0, any pgs_iters:    3 NA = 0: no window on either side (H: guarded by NA > 0).                       M 0 = H 0.
//   3 NA <= 8:                one window per iteration.  M: b, sweep.  H: rows, b.  Never long.       M = H = pgs_iters.
//   8 < 3 NA <= 12, option on, iteration 0:
//                             M: b, positions 0 .. 6, [in 7, operands read] b, positions 7 .. 3 NA - 1; its loop steps over both
//                             windows (w0 += 16, the buffer offset unchanged).  H as ever: rows(0), b, rows(8), b.   2 = 2.
//                             Later iterations (pgs_iters > 1) are two ordinary windows on both sides.
//                                                                                             M = H = 2 pgs_iters = nw pgs_iters.
//                             H's writes: window 8 goes into buffer 1, which M reads only behind the second barrier.  There
//                             is no third window in iteration 0, so nobody writes buffer 0 during it.  With pgs_iters > 1
//                             H's next write into buffer 0 (iteration 1, window 0) follows the second barrier, and M takes
//                             that barrier behind "s_waitcnt lgkmcnt(0)" (OCT_BAR), i.e. with position 7's operands — its last
//                             reads of buffer 0 — in registers.  H writes buffer 1 again (iteration 1, window 8) behind the
//                             THIRD barrier, which M takes at the top of iteration 1, behind position 3 NA - 1.
//   8 < 3 NA <= 12, option off, and 3 NA > 12 (any option):
//                             ordinary windows, nw per iteration.  M: b, sweep, per window.  H: rows, b, per window; it may
//                             write buffer k & 1 for window k + 2 behind barrier k + 1, which M takes behind its sweep of
//                             window k.                                                                   M = H = nw pgs_iters.
// In every case the count is pgs_iters * ceil(3 NA / 8) for NA > 0, whatever the option.
#pragma once

#include <hip/hip_runtime.h>

// the first window of iteration 0 runs on through the second one's rows (wave-uniform: NA, pgs_iters, opt are)
__host__ __device__ inline bool tds_oct_long_window(int NA, int pgs_iters, int opt) {
  return opt != 0 && pgs_iters > 0 && 3 * NA > 8 && 3 * NA <= 12;
}
// main wavefront: windows (= barriers) covered by the sweep that starts at position w0 of iteration pit
__host__ __device__ inline int tds_oct_main_windows(bool long_window, int pit, int w0) {
  return (long_window && pit == 0 && w0 == 0) ? 2 : 1;
}
// helper: the first window of the first iteration is solved in front of the loops (its stages are spread over the step)
__host__ __device__ inline int tds_oct_help_first_w0(int pit) { return pit == 0 ? 8 : 0; }
__host__ __device__ inline bool tds_oct_help_has_windows(int NA, int pgs_iters) { return NA > 0 && pgs_iters > 0; }

// main wavefront, step-loop build for one wavefront per SIMD (option oct_sweep_na, default on): the first iteration's sweep that
// starts at position w0 and covers nw windows runs in the instantiation specialised for NA (tds_oct.hip: main_sweep, NAC) —
// exactly when that sweep holds ALL 3 NA rows of the iteration: NA = 1, 2 (one window) and NA = 3, 4 as a long window (nw = 2;
// with option oct_long_window off they stay two ordinary windows on the generic chain).  The instantiation takes the barriers
// the generic chain takes for the same (NA, nw): tds_oct_sweep_na_inner_barriers inside the sweep, the one at the window's top
// in the caller's loop — the decision changes no count.
__host__ __device__ inline bool tds_oct_sweep_na(int NA, int w0, int nw, int opt) {
  return opt != 0 && w0 == 0 && NA >= 1 && NA <= 4 && (nw == 2 || 3 * NA <= 8);
}
// (barriers INSIDE the specialised sweep: the long window's second one, in position 7 — rows 3 NA > 8)
__host__ __device__ constexpr int tds_oct_sweep_na_inner_barriers(int NA) { return 3 * NA > 8 ? 1 : 0; }

// the two walks, as the kernel's loops do them: window barriers of one step
inline int tds_oct_main_barriers(int NA, int pgs_iters, int opt) {
  const bool lw = tds_oct_long_window(NA, pgs_iters, opt);
  const int nr = 3 * NA;
  int b = 0;
  for (int pit = 0; pit < pgs_iters; ++pit)
    for (int w0 = 0; w0 < nr;) {
      const int nw = tds_oct_main_windows(lw, pit, w0);
      b += nw;  // one at the top of the window; a long window's second one inside position 7
      w0 += 8 * nw;
    }
  return b;
}
// the main wavefront's walk with the specialised first sweep where it is taken (sweep_na_opt: option oct_sweep_na)
inline int tds_oct_main_barriers_sweep_na(int NA, int pgs_iters, int opt, int sweep_na_opt) {
  const bool lw = tds_oct_long_window(NA, pgs_iters, opt);
  const int nr = 3 * NA;
  int b = 0;
  for (int pit = 0; pit < pgs_iters; ++pit)
    for (int w0 = 0; w0 < nr;) {
      const int nw = tds_oct_main_windows(lw, pit, w0);
      if (pit == 0 && tds_oct_sweep_na(NA, w0, nw, sweep_na_opt)) b += 1 + tds_oct_sweep_na_inner_barriers(NA);  // top + inside
      else b += nw;
      w0 += 8 * nw;
    }
  return b;
}
inline int tds_oct_help_barriers(int NA, int pgs_iters) {
  if (!tds_oct_help_has_windows(NA, pgs_iters)) return 0;
  const int nr = 3 * NA;
  int b = 1;
  for (int pit = 0; pit < pgs_iters; ++pit)
    for (int w0 = tds_oct_help_first_w0(pit); w0 < nr; w0 += 8) ++b;
  return b;
}
