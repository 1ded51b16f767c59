// The flux launches of the second-order IMEX step (CN-AB2; `NavierStokes(time_scheme="cnab2")`): the four flux kernels
// of step.hip, scalar.hip and limited.hip with the two-step extrapolation in their epilogue.  Per point r
//
//   F = the twin's flux (two_slot_sum / donor_flux of loop_parts.h, limited_face of limited.h: the twin's bits)
//   ext[r] = w_new F + w_old prev[r];   prev[r] = F
//
// with (w_new, w_old) = (1, 0) on a quantity's first step and (3/2, -1/2) afterwards.  The buoyant scalar forms carry the
// force the same way: b = w_b (avg T - t_ref), f_eff[r] = f[r] + w_new b + w_old b_prev[r], b_prev[r] = b.  w_old == 0
// is a kernel of its own (HIST = false) that never reads the history: a fresh buffer may hold anything.
//
// Bytes per point: the twin's + 16 (prev read and written; ext takes the place of the twin's output): donor 96, limited
// 64 for the momentum flux; the buoyant scalar forms add another 16 per face for b_prev.  Every load of a lane -- the
// history reads included -- is requested before the first value is used (loads_in_flight, limited.h): the history is a
// read-modify-write stream, and a read left behind the gathers would be a second round trip per point.
#include "csr_stream.h"
#include "limited.h"

namespace nss {

struct Ab2 {
  double w_new, w_old;
};

template <bool HIST>
__device__ __forceinline__ double extrapolated(const Ab2& w, double now, double before) {
  if constexpr (HIST) return fma(w.w_old, before, w.w_new * now);
  return w.w_new * now;
}

struct DonorOps {
  const int32_t *adv_col, *avg_col, *diff_col;
  const double *adv_val, *avg_val, *diff_val;
};

// F1 with the extrapolation: one lane per flux point, the six slots first, then the six gathers of u and the history
template <bool HIST>
__global__ __launch_bounds__(kBlock) void step_flux_ab2_kernel(const int32_t* __restrict__ done, int32_t nflux, DonorOps m,
                                                                const double* __restrict__ u, Ab2 w,
                                                                double* __restrict__ prev, double* __restrict__ ext) {
  if (step_done(done)) return;
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t r = int64_t(blockIdx.x) * kBlock + threadIdx.x; r < nflux; r += stride) {
    const int2v ca = __builtin_nontemporal_load(reinterpret_cast<const int2v*>(m.adv_col) + r);
    const int2v cm = __builtin_nontemporal_load(reinterpret_cast<const int2v*>(m.avg_col) + r);
    const int2v cj = __builtin_nontemporal_load(reinterpret_cast<const int2v*>(m.diff_col) + r);
    const dbl2v va = __builtin_nontemporal_load(reinterpret_cast<const dbl2v*>(m.adv_val) + r);
    const dbl2v vm = __builtin_nontemporal_load(reinterpret_cast<const dbl2v*>(m.avg_val) + r);
    const dbl2v vj = __builtin_nontemporal_load(reinterpret_cast<const dbl2v*>(m.diff_val) + r);
    double before = 0.0;
    if constexpr (HIST) before = prev[r];
    const double a0 = u[present(ca.x)], a1 = u[present(ca.y)];
    const double m0 = u[present(cm.x)], m1 = u[present(cm.y)];
    const double j0 = u[present(cj.x)], j1 = u[present(cj.y)];
    loads_in_flight(a0, a1, m0, m1, j0, j1, before);
    const double F = donor_flux(two_slot_sum(ca, va, a0, a1), two_slot_sum(cm, vm, m0, m1), two_slot_sum(cj, vj, j0, j1));
    NSS_ST(ext[r], extrapolated<HIST>(w, F, before));
    NSS_ST(prev[r], F);
  }
}

// F1' with the extrapolation
template <int LIM, bool HIST>
__global__ __launch_bounds__(kBlock) void step_flux_limited_ab2_kernel(const int32_t* __restrict__ done, int32_t nflux,
                                                                        const int32_t* __restrict__ adv_col,
                                                                        const double* __restrict__ adv_val,
                                                                        const int32_t* __restrict__ stencil,
                                                                        const double* __restrict__ u, Ab2 w,
                                                                        double* __restrict__ prev,
                                                                        double* __restrict__ ext) {
  if (step_done(done)) return;
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t r = int64_t(blockIdx.x) * kBlock + threadIdx.x; r < nflux; r += stride) {
    const int4v c = __builtin_nontemporal_load(reinterpret_cast<const int4v*>(stencil) + r);
    const int2v ca = __builtin_nontemporal_load(reinterpret_cast<const int2v*>(adv_col) + r);
    const dbl2v va = __builtin_nontemporal_load(reinterpret_cast<const dbl2v*>(adv_val) + r);
    double before = 0.0;
    if constexpr (HIST) before = prev[r];
    const double a0 = u[present(ca.x)], a1 = u[present(ca.y)];
    const double g_ll = u[present(c.x)], g_lo = u[present(c.y)], g_hi = u[present(c.z)], g_hh = u[present(c.w)];
    loads_in_flight(a0, a1, g_ll, g_lo, g_hi, g_hh, before);
    const double a = two_slot_sum(ca, va, a0, a1);
    const double F = limited_face<LIM>(a, c, or_zero(c.x, g_ll), or_zero(c.y, g_lo), or_zero(c.z, g_hi),
                                       or_zero(c.w, g_hh));
    NSS_ST(ext[r], extrapolated<HIST>(w, F, before));
    NSS_ST(prev[r], F);
  }
}

struct ScalarHistory {
  double *G_prev, *G_ext, *b_prev, *f_eff;
};

// S1 with the extrapolation: one lane per face
template <bool BUOYANT, bool HIST>
__global__ __launch_bounds__(kBlock) void scalar_flux_ab2_kernel(const int32_t* __restrict__ done, int32_t nface,
                                                                  const int32_t* __restrict__ avg_col,
                                                                  const double* __restrict__ avg_val,
                                                                  const int32_t* __restrict__ diff_col,
                                                                  const double* __restrict__ diff_val,
                                                                  const double* __restrict__ w_b,
                                                                  const double* __restrict__ u,
                                                                  const double* __restrict__ f,
                                                                  const double* __restrict__ T, double t_ref, Ab2 w,
                                                                  ScalarHistory h) {
  if (step_done(done)) return;
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t r = int64_t(blockIdx.x) * kBlock + threadIdx.x; r < nface; r += stride) {
    const int2v cm = __builtin_nontemporal_load(reinterpret_cast<const int2v*>(avg_col) + r);
    const int2v cj = __builtin_nontemporal_load(reinterpret_cast<const int2v*>(diff_col) + r);
    const dbl2v vm = __builtin_nontemporal_load(reinterpret_cast<const dbl2v*>(avg_val) + r);
    const dbl2v vj = __builtin_nontemporal_load(reinterpret_cast<const dbl2v*>(diff_val) + r);
    double before = 0.0, b_before = 0.0, wb = 0.0, force = 0.0;
    if constexpr (HIST) before = h.G_prev[r];
    if constexpr (HIST && BUOYANT) b_before = h.b_prev[r];
    if constexpr (BUOYANT) wb = w_b[r], force = f[r];
    const double adv = u[r];
    const double m0 = T[present(cm.x)], m1 = T[present(cm.y)];
    const double j0 = T[present(cj.x)], j1 = T[present(cj.y)];
    loads_in_flight(adv, m0, m1, j0, j1, wb, force, before, b_before);
    const double avg = two_slot_sum(cm, vm, m0, m1);
    const double G = donor_flux(adv, avg, two_slot_sum(cj, vj, j0, j1));
    NSS_ST(h.G_ext[r], extrapolated<HIST>(w, G, before));
    NSS_ST(h.G_prev[r], G);
    if constexpr (BUOYANT) {
      const double b = wb * (avg - t_ref);
      NSS_ST(h.f_eff[r], force + extrapolated<HIST>(w, b, b_before));
      NSS_ST(h.b_prev[r], b);
    }
  }
}

// S1' with the extrapolation
template <int LIM, bool BUOYANT, bool HIST>
__global__ __launch_bounds__(kBlock) void scalar_flux_limited_ab2_kernel(const int32_t* __restrict__ done, int32_t nface,
                                                                          const int32_t* __restrict__ stencil,
                                                                          const double* __restrict__ w_b,
                                                                          const double* __restrict__ u,
                                                                          const double* __restrict__ f,
                                                                          const double* __restrict__ T, double t_ref,
                                                                          Ab2 w, ScalarHistory h) {
  if (step_done(done)) return;
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t r = int64_t(blockIdx.x) * kBlock + threadIdx.x; r < nface; r += stride) {
    const int4v c = __builtin_nontemporal_load(reinterpret_cast<const int4v*>(stencil) + r);
    double before = 0.0, b_before = 0.0, wb = 0.0, force = 0.0;
    if constexpr (HIST) before = h.G_prev[r];
    if constexpr (HIST && BUOYANT) b_before = h.b_prev[r];
    if constexpr (BUOYANT) wb = w_b[r], force = f[r];
    const double g_ll = T[present(c.x)], g_lo = T[present(c.y)], g_hi = T[present(c.z)], g_hh = T[present(c.w)];
    const double a = u[r];
    loads_in_flight(a, g_ll, g_lo, g_hi, g_hh, wb, force, before, b_before);
    const double q_lo = or_zero(c.y, g_lo), q_hi = or_zero(c.z, g_hi);
    const double G = limited_face<LIM>(a, c, or_zero(c.x, g_ll), q_lo, q_hi, or_zero(c.w, g_hh));
    NSS_ST(h.G_ext[r], extrapolated<HIST>(w, G, before));
    NSS_ST(h.G_prev[r], G);
    if constexpr (BUOYANT) {
      const double b = wb * (0.5 * (q_lo + q_hi) - t_ref);
      NSS_ST(h.f_eff[r], force + extrapolated<HIST>(w, b, b_before));
      NSS_ST(h.b_prev[r], b);
    }
  }
}

// ---- the launches: HIST, BUOYANT and the limiter are chosen on the host ----
template <int LIM>
static void launch_step_limited_ab2(bool hist, dim3 grid, hipStream_t st, const int32_t* done, const nss_csr_s& adv,
                                    const int32_t* stencil, const double* u, Ab2 w, double* prev, double* ext) {
  if (hist)
    hipLaunchKernelGGL((step_flux_limited_ab2_kernel<LIM, true>), grid, dim3(kBlock), 0, st, done, adv.m, adv.fw_col,
                       adv.fw_val, stencil, u, w, prev, ext);
  else
    hipLaunchKernelGGL((step_flux_limited_ab2_kernel<LIM, false>), grid, dim3(kBlock), 0, st, done, adv.m, adv.fw_col,
                       adv.fw_val, stencil, u, w, prev, ext);
}

template <bool BUOYANT, bool HIST>
static void launch_scalar_ab2(dim3 grid, hipStream_t st, const int32_t* done, const nss_csr_s& avg, const nss_csr_s& diff,
                              const double* w_b, const double* u, const double* f, const double* T, double t_ref, Ab2 w,
                              ScalarHistory h) {
  hipLaunchKernelGGL((scalar_flux_ab2_kernel<BUOYANT, HIST>), grid, dim3(kBlock), 0, st, done, avg.m, avg.fw_col,
                     avg.fw_val, diff.fw_col, diff.fw_val, w_b, u, f, T, t_ref, w, h);
}

template <int LIM, bool BUOYANT, bool HIST>
static void launch_scalar_limited_ab2(dim3 grid, hipStream_t st, const int32_t* done, int32_t nface,
                                      const int32_t* stencil, const double* w_b, const double* u, const double* f,
                                      const double* T, double t_ref, Ab2 w, ScalarHistory h) {
  hipLaunchKernelGGL((scalar_flux_limited_ab2_kernel<LIM, BUOYANT, HIST>), grid, dim3(kBlock), 0, st, done, nface,
                     stencil, w_b, u, f, T, t_ref, w, h);
}

template <int LIM, class... Args>
static void pick_scalar_limited_ab2(bool buoyant, bool hist, Args... args) {
  if (buoyant && hist) launch_scalar_limited_ab2<LIM, true, true>(args...);
  else if (buoyant) launch_scalar_limited_ab2<LIM, true, false>(args...);
  else if (hist) launch_scalar_limited_ab2<LIM, false, true>(args...);
  else launch_scalar_limited_ab2<LIM, false, false>(args...);
}

// [a, a + na) and [b, b + nb) share an element
static bool overlap(const double* a, int64_t na, const double* b, int64_t nb) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + uintptr_t(nb) * sizeof(double) && b0 < a0 + uintptr_t(na) * sizeof(double);
}

// the scalar forms' argument rules, `n_T`: the entries of T where the caller knows them (0: only T itself is compared)
static void require_scalar_history(const char* who, int64_t nface, int64_t n_T, const double* w_b, const double* u,
                                   const double* f, const double* T, const ScalarHistory& h) {
  const std::string p = std::string(who) + ": ";
  NSS_REQUIRE(u && T && h.G_prev && h.G_ext, (p + "NULL argument").c_str());
  NSS_REQUIRE(w_b == nullptr || (f && h.f_eff && h.b_prev), (p + "w_b without f, f_eff or b_prev").c_str());
  const double* outs[] = {h.G_prev, h.G_ext, w_b ? h.b_prev : nullptr, w_b ? h.f_eff : nullptr};
  for (int i = 0; i < 4; ++i) {
    if (outs[i] == nullptr) continue;
    NSS_REQUIRE(!overlap(outs[i], nface, u, nface) && !overlap(outs[i], nface, T, n_T > 0 ? n_T : 1),
                (p + "an output aliases u or T").c_str());
    NSS_REQUIRE(w_b == nullptr || (!overlap(outs[i], nface, w_b, nface) && !overlap(outs[i], nface, f, nface)),
                (p + "an output aliases w_b or f").c_str());
    for (int j = 0; j < i; ++j)
      NSS_REQUIRE(outs[j] == nullptr || !overlap(outs[i], nface, outs[j], nface), (p + "two outputs alias").c_str());
  }
}

}  // namespace nss

using namespace nss;

extern "C" {

int nss_step_flux_ab2_f64(nss_csr_t adv, nss_csr_t avg, nss_csr_t diff, const double* u, double w_new, double w_old,
                          double* prev, double* ext, const int32_t* done, nss_stream_t stream) {
  return guarded([&] {
    NSS_REQUIRE(adv && avg && diff && u && prev && ext, "step_flux_ab2: NULL argument");
    NSS_REQUIRE(adv->m == avg->m && adv->m == diff->m && adv->n == avg->n && adv->n == diff->n,
                "step_flux_ab2: adv, avg and diff differ in shape");
    require_f64_values(adv, "step_flux_ab2");
    require_f64_values(avg, "step_flux_ab2");
    require_f64_values(diff, "step_flux_ab2");
    if (adv->m == 0) return;                               // (no flux points: there is no two-slot copy to build)
    NSS_REQUIRE(adv->n >= 1, "step_flux_ab2: adv has no columns");
    NSS_REQUIRE(!overlap(prev, adv->m, ext, adv->m) && !overlap(prev, adv->m, u, adv->n) && !overlap(ext, adv->m, u, adv->n),
                "step_flux_ab2: prev, ext and u alias");
    NSS_REQUIRE(fixed_width_copy(*adv) && fixed_width_copy(*avg) && fixed_width_copy(*diff),
                "step_flux_ab2: a row of adv, avg or diff has more than two entries");
    const DonorOps m{adv->fw_col, avg->fw_col, diff->fw_col, adv->fw_val, avg->fw_val, diff->fw_val};
    const dim3 grid(stream_grid(adv->m, kBlock));
    const Ab2 w{w_new, w_old};
    if (w_old != 0.0)
      hipLaunchKernelGGL(step_flux_ab2_kernel<true>, grid, dim3(kBlock), 0, as_stream(stream), done, adv->m, m, u, w, prev,
                         ext);
    else
      hipLaunchKernelGGL(step_flux_ab2_kernel<false>, grid, dim3(kBlock), 0, as_stream(stream), done, adv->m, m, u, w, prev,
                         ext);
    NSS_CHECK_LAUNCH();
  });
}

int nss_step_flux_limited_ab2_f64(nss_csr_t adv, const int32_t* stencil, int64_t nflux, int32_t limiter, const double* u,
                                  double w_new, double w_old, double* prev, double* ext, const int32_t* done,
                                  nss_stream_t stream) {
  return guarded([&] {
    NSS_REQUIRE(adv && stencil && u && prev && ext, "step_flux_limited_ab2: NULL argument");
    NSS_REQUIRE(limiter >= kDonor && limiter <= kVanLeer,
                "step_flux_limited_ab2: limiter is 0 (donor), 1 (minmod) or 2 (van Leer)");
    NSS_REQUIRE(nflux == adv->m, "step_flux_limited_ab2: nflux is not the row count of adv");
    NSS_REQUIRE(nflux == 0 || adv->n >= 1, "step_flux_limited_ab2: adv has no columns");
    NSS_REQUIRE(reinterpret_cast<uintptr_t>(stencil) % 16 == 0, "step_flux_limited_ab2: stencil is not 16-byte aligned");
    require_f64_values(adv, "step_flux_limited_ab2");
    if (nflux == 0) return;                                // (no flux points: there is no two-slot copy to build)
    NSS_REQUIRE(!overlap(prev, nflux, ext, nflux) && !overlap(prev, nflux, u, adv->n) && !overlap(ext, nflux, u, adv->n),
                "step_flux_limited_ab2: prev, ext and u alias");
    NSS_REQUIRE(fixed_width_copy(*adv), "step_flux_limited_ab2: a row of adv has more than two entries");
    const dim3 grid(stream_grid(nflux, kBlock));
    const hipStream_t st = as_stream(stream);
    const Ab2 w{w_new, w_old};
    const bool hist = w_old != 0.0;
    if (limiter == kDonor) launch_step_limited_ab2<kDonor>(hist, grid, st, done, *adv, stencil, u, w, prev, ext);
    else if (limiter == kMinmod) launch_step_limited_ab2<kMinmod>(hist, grid, st, done, *adv, stencil, u, w, prev, ext);
    else launch_step_limited_ab2<kVanLeer>(hist, grid, st, done, *adv, stencil, u, w, prev, ext);
    NSS_CHECK_LAUNCH();
  });
}

int nss_scalar_flux_ab2_f64(nss_csr_t avg, nss_csr_t diff, const double* w_b, const double* u, const double* f,
                            const double* T, double t_ref, double w_new, double w_old, double* G_prev, double* G_ext,
                            double* b_prev, double* f_eff, const int32_t* done, nss_stream_t stream) {
  return guarded([&] {
    NSS_REQUIRE(avg && diff, "scalar_flux_ab2: NULL argument");
    NSS_REQUIRE(avg->m == diff->m && avg->n == diff->n, "scalar_flux_ab2: avg and diff differ in shape");
    const ScalarHistory h{G_prev, G_ext, b_prev, f_eff};
    require_scalar_history("scalar_flux_ab2", avg->m, avg->n, w_b, u, f, T, h);
    require_f64_values(avg, "scalar_flux_ab2");
    require_f64_values(diff, "scalar_flux_ab2");
    if (avg->m == 0) return;                               // (no faces: there is no two-slot copy to build)
    NSS_REQUIRE(avg->n >= 1, "scalar_flux_ab2: avg has no columns");
    NSS_REQUIRE(fixed_width_copy(*avg) && fixed_width_copy(*diff),
                "scalar_flux_ab2: a row of avg or diff has more than two entries");
    const int blocks = stream_grid(avg->m, kBlock);
    const dim3 grid(blocks < kLimitedScalarBlocks ? blocks : kLimitedScalarBlocks);
    const hipStream_t st = as_stream(stream);
    const Ab2 w{w_new, w_old};
    const bool hist = w_old != 0.0;
    if (w_b != nullptr && hist) launch_scalar_ab2<true, true>(grid, st, done, *avg, *diff, w_b, u, f, T, t_ref, w, h);
    else if (w_b != nullptr) launch_scalar_ab2<true, false>(grid, st, done, *avg, *diff, w_b, u, f, T, t_ref, w, h);
    else if (hist) launch_scalar_ab2<false, true>(grid, st, done, *avg, *diff, w_b, u, f, T, t_ref, w, h);
    else launch_scalar_ab2<false, false>(grid, st, done, *avg, *diff, w_b, u, f, T, t_ref, w, h);
    NSS_CHECK_LAUNCH();
  });
}

int nss_scalar_flux_limited_ab2_f64(const int32_t* stencil, int64_t nface, int32_t limiter, const double* w_b,
                                    const double* u, const double* f, const double* T, double t_ref, double w_new,
                                    double w_old, double* G_prev, double* G_ext, double* b_prev, double* f_eff,
                                    const int32_t* done, nss_stream_t stream) {
  return guarded([&] {
    NSS_REQUIRE(stencil, "scalar_flux_limited_ab2: NULL argument");
    NSS_REQUIRE(limiter >= kDonor && limiter <= kVanLeer,
                "scalar_flux_limited_ab2: limiter is 0 (donor), 1 (minmod) or 2 (van Leer)");
    NSS_REQUIRE(nface >= 0 && nface <= INT32_MAX, "scalar_flux_limited_ab2: nface out of range");
    NSS_REQUIRE(reinterpret_cast<uintptr_t>(stencil) % 16 == 0, "scalar_flux_limited_ab2: stencil is not 16-byte aligned");
    const ScalarHistory h{G_prev, G_ext, b_prev, f_eff};
    require_scalar_history("scalar_flux_limited_ab2", nface, 0, w_b, u, f, T, h);
    if (nface == 0) return;
    const int blocks = stream_grid(nface, kBlock);
    const dim3 grid(blocks < kLimitedScalarBlocks ? blocks : kLimitedScalarBlocks);
    const hipStream_t st = as_stream(stream);
    const int32_t n = int32_t(nface);
    const Ab2 w{w_new, w_old};
    const bool buoyant = w_b != nullptr, hist = w_old != 0.0;
    if (limiter == kDonor) pick_scalar_limited_ab2<kDonor>(buoyant, hist, grid, st, done, n, stencil, w_b, u, f, T, t_ref, w, h);
    else if (limiter == kMinmod) pick_scalar_limited_ab2<kMinmod>(buoyant, hist, grid, st, done, n, stencil, w_b, u, f, T, t_ref, w, h);
    else pick_scalar_limited_ab2<kVanLeer>(buoyant, hist, grid, st, done, n, stencil, w_b, u, f, T, t_ref, w, h);
    NSS_CHECK_LAUNCH();
  });
}

}  // extern "C"
