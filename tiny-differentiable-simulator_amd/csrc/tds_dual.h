// tds_dual.h — forward-mode dual numbers for the step Jacobians (tds_diff_step.h, tds_jvp.hip).
//
// TdsDual<K> holds a value and K tangents: x + sum_k d[k] eps_k with eps_j eps_k = 0.  One evaluation of the step over
// TdsDual<K> yields the step's value and K directional derivatives J v_1 .. J v_K at once; the value part does exactly
// the arithmetic of the double evaluation, so the primal of a Jacobian launch is the double step's result.
//
// Comparisons, min / max and clamps look at the value only: a derivative follows the branch the primal takes, as the
// reference's TinyDual does (src/math/tiny/tiny_dual.h: operator<, operator> compare real()).
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TDS_HD __host__ __device__
#else
#define TDS_HD
#endif

template <int K>
struct TdsDual {
  double v;
  double d[K];
  TDS_HD TdsDual() : v(0.0) {
    for (int k = 0; k < K; ++k) d[k] = 0.0;
  }
  TDS_HD TdsDual(double x) : v(x) {  // a constant: no tangents
    for (int k = 0; k < K; ++k) d[k] = 0.0;
  }
  TDS_HD TdsDual &operator+=(const TdsDual &b) {
    v += b.v;
    for (int k = 0; k < K; ++k) d[k] += b.d[k];
    return *this;
  }
  TDS_HD TdsDual &operator-=(const TdsDual &b) {
    v -= b.v;
    for (int k = 0; k < K; ++k) d[k] -= b.d[k];
    return *this;
  }
  TDS_HD TdsDual &operator*=(const TdsDual &b) { return *this = *this * b; }
  TDS_HD TdsDual &operator/=(const TdsDual &b) { return *this = *this / b; }

  TDS_HD friend TdsDual operator-(const TdsDual &a) {
    TdsDual r;
    r.v = -a.v;
    for (int k = 0; k < K; ++k) r.d[k] = -a.d[k];
    return r;
  }
  TDS_HD friend TdsDual operator+(const TdsDual &a, const TdsDual &b) {
    TdsDual r;
    r.v = a.v + b.v;
    for (int k = 0; k < K; ++k) r.d[k] = a.d[k] + b.d[k];
    return r;
  }
  TDS_HD friend TdsDual operator-(const TdsDual &a, const TdsDual &b) {
    TdsDual r;
    r.v = a.v - b.v;
    for (int k = 0; k < K; ++k) r.d[k] = a.d[k] - b.d[k];
    return r;
  }
  TDS_HD friend TdsDual operator*(const TdsDual &a, const TdsDual &b) {
    TdsDual r;
    r.v = a.v * b.v;
    for (int k = 0; k < K; ++k) r.d[k] = a.d[k] * b.v + a.v * b.d[k];
    return r;
  }
  TDS_HD friend TdsDual operator/(const TdsDual &a, const TdsDual &b) {
    TdsDual r;
    r.v = a.v / b.v;
    const double inv = 1.0 / b.v;
    for (int k = 0; k < K; ++k) r.d[k] = (a.d[k] - r.v * b.d[k]) * inv;
    return r;
  }
  // products with a constant: no tangent arithmetic for the constant's side
  TDS_HD friend TdsDual operator*(const TdsDual &a, double b) {
    TdsDual r;
    r.v = a.v * b;
    for (int k = 0; k < K; ++k) r.d[k] = a.d[k] * b;
    return r;
  }
  TDS_HD friend TdsDual operator*(double a, const TdsDual &b) {
    TdsDual r;
    r.v = a * b.v;
    for (int k = 0; k < K; ++k) r.d[k] = a * b.d[k];
    return r;
  }
  TDS_HD friend TdsDual operator+(const TdsDual &a, double b) {
    TdsDual r = a;
    r.v += b;
    return r;
  }
  TDS_HD friend TdsDual operator+(double a, const TdsDual &b) {
    TdsDual r = b;
    r.v = a + b.v;
    return r;
  }
  TDS_HD friend TdsDual operator-(const TdsDual &a, double b) {
    TdsDual r = a;
    r.v -= b;
    return r;
  }
  TDS_HD friend TdsDual operator-(double a, const TdsDual &b) {
    TdsDual r = -b;
    r.v = a - b.v;
    return r;
  }
  TDS_HD friend TdsDual operator/(const TdsDual &a, double b) {
    TdsDual r;
    r.v = a.v / b;
    for (int k = 0; k < K; ++k) r.d[k] = a.d[k] / b;
    return r;
  }
  TDS_HD friend TdsDual operator/(double a, const TdsDual &b) { return TdsDual(a) / b; }

  // value-only comparisons (the branch of the primal)
  TDS_HD friend bool operator<(const TdsDual &a, const TdsDual &b) { return a.v < b.v; }
  TDS_HD friend bool operator>(const TdsDual &a, const TdsDual &b) { return a.v > b.v; }
  TDS_HD friend bool operator<=(const TdsDual &a, const TdsDual &b) { return a.v <= b.v; }
  TDS_HD friend bool operator>=(const TdsDual &a, const TdsDual &b) { return a.v >= b.v; }
  TDS_HD friend bool operator<(const TdsDual &a, double b) { return a.v < b; }
  TDS_HD friend bool operator>(const TdsDual &a, double b) { return a.v > b; }
  TDS_HD friend bool operator<=(const TdsDual &a, double b) { return a.v <= b; }
  TDS_HD friend bool operator>=(const TdsDual &a, double b) { return a.v >= b; }
  TDS_HD friend bool operator==(const TdsDual &a, double b) { return a.v == b; }
};

// value of a scalar of either kind
TDS_HD inline double tds_value(double x) { return x; }
template <int K>
TDS_HD inline double tds_value(const TdsDual<K> &x) {
  return x.v;
}

TDS_HD inline double tds_sqrt(double x) { return sqrt(x); }
TDS_HD inline double tds_sin(double x) { return sin(x); }
TDS_HD inline double tds_cos(double x) { return cos(x); }
template <int K>
TDS_HD inline TdsDual<K> tds_sqrt(const TdsDual<K> &a) {
  TdsDual<K> r;
  r.v = sqrt(a.v);
  const double g = 0.5 / r.v;
  for (int k = 0; k < K; ++k) r.d[k] = a.d[k] * g;
  return r;
}
template <int K>
TDS_HD inline TdsDual<K> tds_sin(const TdsDual<K> &a) {
  TdsDual<K> r;
  r.v = sin(a.v);
  const double c = cos(a.v);
  for (int k = 0; k < K; ++k) r.d[k] = a.d[k] * c;
  return r;
}
template <int K>
TDS_HD inline TdsDual<K> tds_cos(const TdsDual<K> &a) {
  TdsDual<K> r;
  r.v = cos(a.v);
  const double s = -sin(a.v);
  for (int k = 0; k < K; ++k) r.d[k] = a.d[k] * s;
  return r;
}

// a + b, a - b where b is a parameter read through a view (tds_diff_step.h): a double with the blob's view, a T with an
// overlay's.  Plain sums here; TdsRev (tds_rev.h) overloads them so that a constant T records what a double would.
template <typename A, typename Bt>
TDS_HD inline A tds_add_c(const A &a, const Bt &b) {
  return a + b;
}
template <typename A, typename Bt>
TDS_HD inline A tds_sub_c(const A &a, const Bt &b) {
  return a - b;
}

// clamps on the value (Algebra::min / max of the reference pick one operand whole, tangents included)
template <typename T>
TDS_HD inline T tds_clamp(const T &x, const T &lo, const T &hi) {
  if (x < lo) return lo;
  if (x > hi) return hi;
  return x;
}
