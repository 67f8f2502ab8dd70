// tds_rev.h — reverse-mode scalar for the step VJPs (tds_diff_step.h over TdsRev, tds_vjp.hip).
//
// TdsRev is a value and a variable index (-1: a constant).  Every operation with an active operand appends one tape
// entry: the indices of its (one or two) active arguments and the local partials, taken at record time; the entry's
// result is variable n_in + position.  Inputs are variables 0 .. n_in - 1.  A sum or difference with a double keeps
// its operand's index (the partial is 1) and records nothing.  The value part does the arithmetic of the double
// evaluation, so the primal of a VJP is the double step's result.
//
// Comparisons read the value only, as TdsDual's do: the derivative follows the branch the primal takes.
//
// The tape of the calling lane is reachable from the free operators through one context per lane: on the device a
// file-scope __shared__ descriptor of the workgroup (one wavefront, 64 lanes) plus a __shared__ cursor per lane; on
// the host a thread_local descriptor and cursor.  Entries, adjoints: position p of lane l at [p * stride + l]
// (stride 64 on the device: lanes at the same position store and load contiguously; 1 on the host).  Recording
// stores the entry only: no adjoint is touched, so that the stores cannot alias the step's state.  A lane whose
// tape is full records nothing more; its cursor is left at cap + 1, which the caller reads as an overflow.
#pragma once
#include "tds_dual.h"

struct alignas(8) TdsRevIdx {  // active arguments of an entry (b = -1: one argument)
  int a, b;
};
struct alignas(16) TdsRevPart {  // their local partials
  double da, db;
};

struct TdsRevTape {
  TdsRevIdx *ix;
  TdsRevPart *pd;
  double *adj;        // adjoints of the variables [n_in + cap]
  long long stride;   // elements between neighbouring positions of one lane
  int cap, n_in;
};

#if defined(__HIP_DEVICE_COMPILE__)
__shared__ TdsRevTape tds_rev_tape_s;  // the workgroup's (one wavefront's) tape, at its lane 0
__shared__ int tds_rev_cur_s[64];      // entries each lane has recorded
#else
inline thread_local TdsRevTape tds_rev_tape_h;
inline thread_local int tds_rev_cur_h;
#endif
// the calling lane's tape, the cursor of lane `lane` of its wavefront (host: the calling thread's), its own lane
TDS_HD inline TdsRevTape &tds_rev_tape() {
#if defined(__HIP_DEVICE_COMPILE__)
  return tds_rev_tape_s;
#else
  return tds_rev_tape_h;
#endif
}
TDS_HD inline int tds_rev_lane() {
#if defined(__HIP_DEVICE_COMPILE__)
  return threadIdx.x;
#else
  return 0;
#endif
}
TDS_HD inline int &tds_rev_cursor(int lane) {
#if defined(__HIP_DEVICE_COMPILE__)
  return tds_rev_cur_s[lane];
#else
  return (void)lane, tds_rev_cur_h;
#endif
}

// append an entry; returns its result's variable index, or -1 once the tape is full
TDS_HD inline int tds_rev_push(int a, double da, int b, double db) {
  const TdsRevTape &t = tds_rev_tape();
  const int lane = tds_rev_lane();
  int &cur = tds_rev_cursor(lane);
  const int p = cur;
  if (p >= t.cap) {
    cur = t.cap + 1;
    return -1;
  }
  const long long o = p * t.stride + lane;
#if defined(__HIP_DEVICE_COMPILE__)
  // the tape is global memory: stores through the generic pointers of the __shared__ descriptor would be flat stores,
  // which the next operation's LDS reads (descriptor, cursor) would have to wait for
  typedef __attribute__((address_space(1))) TdsRevIdx GIdx;
  typedef __attribute__((address_space(1))) TdsRevPart GPart;
  ((GIdx *)t.ix)[o] = TdsRevIdx{a, b};
  ((GPart *)t.pd)[o] = TdsRevPart{da, db};
#else
  t.ix[o] = TdsRevIdx{a, b};
  t.pd[o] = TdsRevPart{da, db};
#endif
  cur = p + 1;
  return t.n_in + p;
}

struct TdsRev {
  double v;
  int i;
  TDS_HD TdsRev() : v(0.0), i(-1) {}
  TDS_HD TdsRev(double x) : v(x), i(-1) {}  // a constant
  TDS_HD TdsRev(double x, int idx) : v(x), i(idx) {}

  TDS_HD TdsRev &operator+=(const TdsRev &b) { return *this = *this + b; }
  TDS_HD TdsRev &operator-=(const TdsRev &b) { return *this = *this - b; }
  TDS_HD TdsRev &operator*=(const TdsRev &b) { return *this = *this * b; }
  TDS_HD TdsRev &operator/=(const TdsRev &b) { return *this = *this / b; }

  // r = f(a), df/da = da
  TDS_HD static TdsRev un(double r, const TdsRev &a, double da) {
    return TdsRev(r, a.i < 0 ? -1 : tds_rev_push(a.i, da, -1, 0.0));
  }
  // r = f(a, b)
  TDS_HD static TdsRev bin(double r, const TdsRev &a, double da, const TdsRev &b, double db) {
    if (a.i < 0) return un(r, b, db);
    if (b.i < 0) return un(r, a, da);
    return TdsRev(r, tds_rev_push(a.i, da, b.i, db));
  }

  TDS_HD friend TdsRev operator-(const TdsRev &a) { return un(-a.v, a, -1.0); }
  TDS_HD friend TdsRev operator+(const TdsRev &a, const TdsRev &b) { return bin(a.v + b.v, a, 1.0, b, 1.0); }
  TDS_HD friend TdsRev operator-(const TdsRev &a, const TdsRev &b) { return bin(a.v - b.v, a, 1.0, b, -1.0); }
  TDS_HD friend TdsRev operator*(const TdsRev &a, const TdsRev &b) { return bin(a.v * b.v, a, b.v, b, a.v); }
  TDS_HD friend TdsRev operator/(const TdsRev &a, const TdsRev &b) {
    const double r = a.v / b.v, inv = 1.0 / b.v;
    return bin(r, a, inv, b, -r * inv);
  }
  TDS_HD friend TdsRev operator+(const TdsRev &a, double b) { return TdsRev(a.v + b, a.i); }
  TDS_HD friend TdsRev operator+(double a, const TdsRev &b) { return TdsRev(a + b.v, b.i); }
  TDS_HD friend TdsRev operator-(const TdsRev &a, double b) { return TdsRev(a.v - b, a.i); }
  TDS_HD friend TdsRev operator-(double a, const TdsRev &b) { return un(a - b.v, b, -1.0); }
  TDS_HD friend TdsRev operator*(const TdsRev &a, double b) { return un(a.v * b, a, b); }
  TDS_HD friend TdsRev operator*(double a, const TdsRev &b) { return un(a * b.v, b, a); }
  TDS_HD friend TdsRev operator/(const TdsRev &a, double b) { return un(a.v / b, a, 1.0 / b); }
  TDS_HD friend TdsRev operator/(double a, const TdsRev &b) {
    const double r = a / b.v;
    return un(r, b, -r / b.v);
  }

  // value-only comparisons (the branch of the primal)
  TDS_HD friend bool operator<(const TdsRev &a, const TdsRev &b) { return a.v < b.v; }
  TDS_HD friend bool operator>(const TdsRev &a, const TdsRev &b) { return a.v > b.v; }
  TDS_HD friend bool operator<=(const TdsRev &a, const TdsRev &b) { return a.v <= b.v; }
  TDS_HD friend bool operator>=(const TdsRev &a, const TdsRev &b) { return a.v >= b.v; }
  TDS_HD friend bool operator<(const TdsRev &a, double b) { return a.v < b; }
  TDS_HD friend bool operator>(const TdsRev &a, double b) { return a.v > b; }
  TDS_HD friend bool operator<=(const TdsRev &a, double b) { return a.v <= b; }
  TDS_HD friend bool operator>=(const TdsRev &a, double b) { return a.v >= b; }
  TDS_HD friend bool operator==(const TdsRev &a, double b) { return a.v == b; }
};

TDS_HD inline double tds_value(const TdsRev &x) { return x.v; }
// tds_add_c / tds_sub_c (tds_dual.h): a constant b keeps a's index and records nothing, as a double b does — a
// parameter that is not selected costs the tape no entry
TDS_HD inline TdsRev tds_add_c(const TdsRev &a, const TdsRev &b) { return b.i < 0 ? TdsRev(a.v + b.v, a.i) : a + b; }
TDS_HD inline TdsRev tds_sub_c(const TdsRev &a, const TdsRev &b) { return b.i < 0 ? TdsRev(a.v - b.v, a.i) : a - b; }
TDS_HD inline TdsRev tds_sqrt(const TdsRev &a) {
  const double r = sqrt(a.v);
  return TdsRev::un(r, a, 0.5 / r);
}
TDS_HD inline TdsRev tds_sin(const TdsRev &a) { return TdsRev::un(sin(a.v), a, cos(a.v)); }
TDS_HD inline TdsRev tds_cos(const TdsRev &a) { return TdsRev::un(cos(a.v), a, -sin(a.v)); }

// the reverse sweep of one lane over entries [0, len): adj[ix.a] += da adj[r], adj[ix.b] += db adj[r] (the host's
// form; tds_vjp.hip has the device's).  The caller zeroed the adjoints and seeded the outputs.
inline void tds_rev_sweep_host(const TdsRevTape &t, int len) {
  for (int p = len - 1; p >= 0; --p) {
    const TdsRevIdx e = t.ix[p];
    const TdsRevPart d = t.pd[p];
    const double g = t.adj[t.n_in + p];
    t.adj[e.a] += d.da * g;
    if (e.b >= 0) t.adj[e.b] += d.db * g;
  }
}
