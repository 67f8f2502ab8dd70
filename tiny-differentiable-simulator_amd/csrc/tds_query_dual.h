// tds_query_dual.h — what the forward-mode derivatives of the queries (tds_contact_jvp.hip, tds_dyn_jvp.hip) share: the
// scalar of a work item's K tangents and the setters of a value or a tangent that read the same for a double (K = 0)
// and for a dual.
#pragma once
#include "tds_dual.h"

namespace {

// the scalar of K tangents; K = 0: double
template <int K>
struct TdsContactScalar { using type = TdsDual<K>; };
template <>
struct TdsContactScalar<0> { using type = double; };

// the value a double or a dual is built from
TDS_HD inline void tds_contact_set_value(double &t, double v) { t = v; }
template <int K>
TDS_HD inline void tds_contact_set_value(TdsDual<K> &t, double v) {
  t = TdsDual<K>(v);
}
TDS_HD inline void tds_contact_set_tangent(double &, int, double) {}
template <int K>
TDS_HD inline void tds_contact_set_tangent(TdsDual<K> &t, int k, double d) {
  t.d[k] = d;
}

}  // namespace
