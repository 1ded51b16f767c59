// Second-order limited forms of the two flux launches of the device-resident time step (F1 of step.hip, S1 of
// scalar.hip): the transported quantity is read through ONE four-point stencil row per flux point (ll, lo, hi, hh; -1 =
// absent) instead of the two-slot copies of avg and diff, and the face value is limited_face (limited.h).
//
//   F1'  flux points : F = a * (U + s / 2), a = I_adv u through the two-slot copy of adv     (step_flux_limited_kernel)
//   S1'  faces       : G = u_r * (U + s / 2) on T;  f_eff = f + w_b ((T_lo + T_hi) / 2 - T_ref)   (scalar_flux_limited_kernel)
//
// Bytes per point: F1' 16 (stencil) + 24 (adv: two columns, two values) + 8 (F) = 48 against 80; S1' 16 + 8 (u) + 8 (G)
// = 32 against 64, buoyant + 24 (w_b, f, f_eff) = 56 against 88.  The limiter is a template argument.
#include "csr_stream.h"
#include "limited.h"

namespace nss {

// F1': one lane per flux point.  The stencil row and the two slots of adv are requested first, then all six gathers of
// u -- the four stencil values whatever the sign of a, so that no load waits for a -- then the selection in registers.
template <int LIM>
__global__ __launch_bounds__(kBlock) void step_flux_limited_kernel(const int32_t* __restrict__ done, int32_t nflux,
                                                                    const int32_t* __restrict__ adv_col,
                                                                    const double* __restrict__ adv_val,
                                                                    const int32_t* __restrict__ stencil,
                                                                    const double* __restrict__ u,
                                                                    double* __restrict__ flux) {
  if (step_done(done)) return;
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t r = int64_t(blockIdx.x) * kBlock + threadIdx.x; r < nflux; r += stride) {
    const int4v c = __builtin_nontemporal_load(reinterpret_cast<const int4v*>(stencil) + r);
    const int2v ca = __builtin_nontemporal_load(reinterpret_cast<const int2v*>(adv_col) + r);
    const dbl2v va = __builtin_nontemporal_load(reinterpret_cast<const dbl2v*>(adv_val) + r);
    const double a0 = u[present(ca.x)], a1 = u[present(ca.y)];
    const double g_ll = u[present(c.x)], g_lo = u[present(c.y)], g_hi = u[present(c.z)], g_hh = u[present(c.w)];
    loads_in_flight(a0, a1, g_ll, g_lo, g_hi, g_hh);
    const double a = two_slot_sum(ca, va, a0, a1);
    NSS_ST(flux[r], limited_face<LIM>(a, c, or_zero(c.x, g_ll), or_zero(c.y, g_lo), or_zero(c.z, g_hi),
                                      or_zero(c.w, g_hh)));
  }
}

// S1': one lane per face; the advecting velocity is the face's own dof
template <int LIM, bool BUOYANT>
__global__ __launch_bounds__(kBlock) void scalar_flux_limited_kernel(const int32_t* __restrict__ done, int32_t nface,
                                                                      const int32_t* __restrict__ stencil,
                                                                      const double* __restrict__ w_b,
                                                                      const double* __restrict__ u,
                                                                      const double* __restrict__ f,
                                                                      const double* __restrict__ T, double t_ref,
                                                                      double* __restrict__ G,
                                                                      double* __restrict__ f_eff) {
  if (step_done(done)) return;
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t r = int64_t(blockIdx.x) * kBlock + threadIdx.x; r < nface; r += stride) {
    const int4v c = __builtin_nontemporal_load(reinterpret_cast<const int4v*>(stencil) + r);
    const double g_ll = T[present(c.x)], g_lo = T[present(c.y)], g_hi = T[present(c.z)], g_hh = T[present(c.w)];
    const double a = u[r];
    double w = 0.0, force = 0.0;
    if constexpr (BUOYANT) w = w_b[r], force = f[r];
    loads_in_flight(a, g_ll, g_lo, g_hi, g_hh, w, force);
    const double q_lo = or_zero(c.y, g_lo), q_hi = or_zero(c.z, g_hi);
    NSS_ST(G[r], limited_face<LIM>(a, c, or_zero(c.x, g_ll), q_lo, q_hi, or_zero(c.w, g_hh)));
    if constexpr (BUOYANT) NSS_ST(f_eff[r], fma(w, 0.5 * (q_lo + q_hi) - t_ref, force));
  }
}

template <int LIM>
static void launch_step_flux_limited(dim3 grid, hipStream_t st, const int32_t* done, const nss_csr_s& adv,
                                     const int32_t* stencil, const double* u, double* flux) {
  hipLaunchKernelGGL(step_flux_limited_kernel<LIM>, grid, dim3(kBlock), 0, st, done, adv.m, adv.fw_col, adv.fw_val,
                     stencil, u, flux);
}

template <int LIM>
static void launch_scalar_flux_limited(dim3 grid, hipStream_t st, const int32_t* done, int32_t nface,
                                       const int32_t* stencil, const double* w_b, const double* u, const double* f,
                                       const double* T, double t_ref, double* G, double* f_eff) {
  if (w_b != nullptr)
    hipLaunchKernelGGL((scalar_flux_limited_kernel<LIM, true>), grid, dim3(kBlock), 0, st, done, nface, stencil, w_b, u, f,
                       T, t_ref, G, f_eff);
  else
    hipLaunchKernelGGL((scalar_flux_limited_kernel<LIM, false>), grid, dim3(kBlock), 0, st, done, nface, stencil, w_b, u,
                       f, T, t_ref, G, f_eff);
}

}  // namespace nss

using namespace nss;

extern "C" {

int nss_step_flux_limited_f64(nss_csr_t adv, const int32_t* stencil, int64_t nflux, int32_t limiter, const double* u,
                              double* flux, const int32_t* done, nss_stream_t stream) {
  return guarded([&] {
    NSS_REQUIRE(adv && stencil && u && flux, "step_flux_limited: NULL argument");
    NSS_REQUIRE(limiter >= kDonor && limiter <= kVanLeer, "step_flux_limited: limiter is 0 (donor), 1 (minmod) or 2 (van Leer)");
    NSS_REQUIRE(nflux == adv->m, "step_flux_limited: nflux is not the row count of adv");
    NSS_REQUIRE(nflux == 0 || adv->n >= 1, "step_flux_limited: adv has no columns");
    NSS_REQUIRE(reinterpret_cast<uintptr_t>(stencil) % 16 == 0, "step_flux_limited: stencil is not 16-byte aligned");
    NSS_REQUIRE(flux != u, "step_flux_limited: flux aliases u");
    require_f64_values(adv, "step_flux_limited");
    if (nflux == 0) return;                                // (no flux points: there is no two-slot copy to build)
    NSS_REQUIRE(fixed_width_copy(*adv), "step_flux_limited: a row of adv has more than two entries");
    const dim3 grid(stream_grid(nflux, kBlock));
    const hipStream_t st = as_stream(stream);
    if (limiter == kDonor) launch_step_flux_limited<kDonor>(grid, st, done, *adv, stencil, u, flux);
    else if (limiter == kMinmod) launch_step_flux_limited<kMinmod>(grid, st, done, *adv, stencil, u, flux);
    else launch_step_flux_limited<kVanLeer>(grid, st, done, *adv, stencil, u, flux);
    NSS_CHECK_LAUNCH();
  });
}

int nss_scalar_flux_limited_f64(const int32_t* stencil, int64_t nface, int32_t limiter, const double* w_b,
                                const double* u, const double* f, const double* T, double t_ref, double* G,
                                double* f_eff, const int32_t* done, nss_stream_t stream) {
  return guarded([&] {
    NSS_REQUIRE(stencil && u && T && G, "scalar_flux_limited: NULL argument");
    NSS_REQUIRE(limiter >= kDonor && limiter <= kVanLeer, "scalar_flux_limited: limiter is 0 (donor), 1 (minmod) or 2 (van Leer)");
    NSS_REQUIRE(nface >= 0 && nface <= INT32_MAX, "scalar_flux_limited: nface out of range");
    NSS_REQUIRE(reinterpret_cast<uintptr_t>(stencil) % 16 == 0, "scalar_flux_limited: stencil is not 16-byte aligned");
    NSS_REQUIRE(w_b == nullptr || (f && f_eff), "scalar_flux_limited: w_b without f or f_eff");
    NSS_REQUIRE(G != T && G != u && f_eff != u && f_eff != T, "scalar_flux_limited: an output aliases an operand");
    if (nface == 0) return;
    const int blocks = stream_grid(nface, kBlock);
    const dim3 grid(blocks < kLimitedScalarBlocks ? blocks : kLimitedScalarBlocks);
    const hipStream_t st = as_stream(stream);
    const int32_t n = int32_t(nface);
    if (limiter == kDonor) launch_scalar_flux_limited<kDonor>(grid, st, done, n, stencil, w_b, u, f, T, t_ref, G, f_eff);
    else if (limiter == kMinmod) launch_scalar_flux_limited<kMinmod>(grid, st, done, n, stencil, w_b, u, f, T, t_ref, G, f_eff);
    else launch_scalar_flux_limited<kVanLeer>(grid, st, done, n, stencil, w_b, u, f, T, t_ref, G, f_eff);
    NSS_CHECK_LAUNCH();
  });
}

}  // extern "C"
