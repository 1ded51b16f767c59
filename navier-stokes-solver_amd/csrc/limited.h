// The second-order limited upwind face value of the convection terms and the load helpers of the flux kernels
// (flux.hip).  The face value, said once:
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

// ---- the loads of the four flux kernels (flux.hip) ----
// A gather that no branch guards: an absent entry (-1) reads element 0, which exists, and its value is dropped in
// registers.  Guarded by `c >= 0 ? q[c] : 0` every gather sits in a branch of its own, and the wait counts the compiler
// can prove across those branches make the later gathers wait for the earlier ones.
__device__ __forceinline__ int present(int32_t c) { return c < 0 ? 0 : c; }
__device__ __forceinline__ double or_zero(int32_t c, double v) { return c >= 0 ? v : 0.0; }

// All of a lane's loads are in flight before the first value is used.  Left alone the compiler sinks the far gathers
// into the branch behind the sign of a and the presence of the far entry (seen in S1': ll and hh requested after u[r] had
// arrived) -- the dependent second round of loads that DESIGN.md section 2 measured as the cost of the old SpMV.
__device__ __forceinline__ void loads_in_flight(double a, double b, double c, double d, double e, double f = 0.0,
                                                double g = 0.0) {
  asm volatile("" ::"v"(a), "v"(b), "v"(c), "v"(d), "v"(e), "v"(f), "v"(g));
}
// (the scalar forms add the force and the history reads of an extrapolating output: up to nine values)
__device__ __forceinline__ void loads_in_flight(double a, double b, double c, double d, double e, double f, double g,
                                                double h, double i = 0.0) {
  asm volatile("" ::"v"(a), "v"(b), "v"(c), "v"(d), "v"(e), "v"(f), "v"(g), "v"(h), "v"(i));
}

}  // namespace nss
