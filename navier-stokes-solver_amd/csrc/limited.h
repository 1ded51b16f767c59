// The second-order limited upwind face value of the convection terms (limited.hip), said once:
//
//   a >= 0:  U = q_lo, D = q_hi, UU = q_ll        a < 0:  U = q_hi, D = q_lo, UU = q_hh
//   s = phi(U - UU, D - U) if UU exists, else 0;   F = a * (U + s / 2)
//
// with phi = 0 (donor cell), the minmod or the van Leer (harmonic) slope.  An absent lo or hi is a wall and arrives here
// as the value 0; an absent far value leaves the point donor-cell for that flow direction.  F is continuous across every
// branch (both slopes tend to 0 with p q -> 0+, the two flow directions meet in F = 0 at a = 0).
#pragma once

#include "loop_parts.h"

namespace nss {

typedef int32_t int4v __attribute__((ext_vector_type(4)));

enum Limiter : int { kDonor = 0, kMinmod = 1, kVanLeer = 2 };

template <int LIM>
__device__ __forceinline__ double limited_slope(double p, double q) {
  if constexpr (LIM == kDonor) return 0.0;
  const bool same = p * q > 0.0;
  if constexpr (LIM == kMinmod) return same ? (fabs(p) < fabs(q) ? p : q) : 0.0;
  return same ? 2.0 * p * q / (p + q) : 0.0;
}

// `c`: the stencil row (ll, lo, hi, hh; -1 = absent), the four values gathered whatever the sign of a: the upwind side
// is chosen in registers
template <int LIM>
__device__ __forceinline__ double limited_face(double a, const int4v& c, double q_ll, double q_lo, double q_hi,
                                               double q_hh) {
  const bool pos = a >= 0.0;
  const double up = pos ? q_lo : q_hi, down = pos ? q_hi : q_lo, far = pos ? q_ll : q_hh;
  const double s = (pos ? c.x : c.w) >= 0 ? limited_slope<LIM>(up - far, down - up) : 0.0;
  return a * (up + 0.5 * s);
}

}  // namespace nss
