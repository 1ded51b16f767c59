// The convective flux launches of the device-resident time step (F1 of step.hip, S1 of scalar.hip), one kernel per
// quantity and scheme, each taking what is done with the flux as an output policy:
//
//   F1   flux points : F = adv*avg - |adv| diff / 2, adv = I_adv u, avg = Avg u, diff = Diff u     (step_flux_kernel)
//   F1'  flux points : F = a * (U + s / 2), a = I_adv u, U and s through one stencil row   (step_flux_limited_kernel)
//   S1   faces       : G = u_r (avg T) - |u_r| (diff T) / 2;  the force of avg T - t_ref           (scalar_flux_kernel)
//   S1'  faces       : G = u_r * (U + s / 2) on T;  the force of (T_lo + T_hi) / 2 - t_ref (scalar_flux_limited_kernel)
//
// F1 and S1 read the two-slot copies of their operators; F1' and S1' read the transported quantity through ONE
// four-point stencil row per point (ll, lo, hi, hh; -1 = absent) and limit the face value (limited_face, limited.h;
// the limiter is a template argument).  The output policy is one of
//
//   StoreFlux               flux[r] = F;                                    f_eff[r] = fma(w_b, excess - t_ref, f)
//   ExtrapolateFlux<HIST>   ext[r] = w_new F + w_old prev[r], prev[r] = F;  b = w_b (excess - t_ref),
//                           f_eff[r] = f + w_new b + w_old b_prev[r], b_prev[r] = b
//
// the second being the two-step extrapolation of CN-AB2 (`NavierStokes(time_scheme="cnab2")`) with (w_new, w_old) =
// (1, 0) on a quantity's first step and (3/2, -1/2) afterwards.  w_old == 0 is a policy of its own (HIST = false) that
// never reads the history: a fresh buffer may hold anything.
//
// Bytes per point: F1 80, F1' 16 (stencil) + 24 (adv: two columns, two values) + 8 (F) = 48; S1 64, S1' 16 + 8 (u) + 8
// (G) = 32; buoyant + 24 (w_b, f, f_eff).  Extrapolating adds 16 (prev read and written; ext takes the place of the
// plain output), the buoyant scalar forms another 16 per face for b_prev.  Every load of a lane -- the history reads
// included -- is requested before the first value is used (loads_in_flight, limited.h): the history is a
// read-modify-write stream, and a read left behind the gathers would be a second round trip per point.
#include <type_traits>

#include "csr_stream.h"
#include "limited.h"

namespace nss {

// S1 and S1' run grid-stride over at most this many workgroups (16 per CU): one pass covers 2^20 faces, a 3-D grid of
// n = 64 (774 144 faces) is one-shot
constexpr int kScalarFluxBlocks = 4096;

struct Ab2 {
  double w_new, w_old;
};

template <bool HIST>
__device__ __forceinline__ double extrapolated(const Ab2& w, double now, double before) {
  if constexpr (HIST) return fma(w.w_old, before, w.w_new * now);
  return w.w_new * now;
}

// ---- the output policies: fetch<FORCE>() requests what the lane needs of the history (of the force too: the buoyant
// scalar forms) and its Pre pins those reads with the lane's other loads; flux() stores the flux of point r, force() the
// buoyant force of face r from `excess` = (the face's T) - t_ref ----
struct StoreFlux {
  double* __restrict__ out;
  double* __restrict__ f_eff;                              // (the buoyant scalar forms)
  struct Pre {
    template <class... V>
    __device__ void in_flight_with(V... loads) const { loads_in_flight(loads...); }
  };
  template <bool FORCE>
  __device__ Pre fetch(int64_t) const { return Pre{}; }
  __device__ void flux(int64_t r, double F, const Pre&) const { NSS_ST(out[r], F); }
  __device__ void force(int64_t r, double w_b, double excess, double f, const Pre&) const {
    NSS_ST(f_eff[r], fma(w_b, excess, f));
  }
};

template <bool HIST>
struct ExtrapolateFlux {
  Ab2 w;
  double *prev, *ext;
  double *b_prev, *f_eff;                                  // (the buoyant scalar forms)
  template <bool FORCE>
  struct Pre {
    double before = 0.0, b_before = 0.0;
    template <class... V>
    __device__ void in_flight_with(V... loads) const {
      if constexpr (FORCE) loads_in_flight(loads..., before, b_before);
      else loads_in_flight(loads..., before);
    }
  };
  template <bool FORCE>
  __device__ Pre<FORCE> fetch(int64_t r) const {
    Pre<FORCE> p;
    if constexpr (HIST) p.before = prev[r];
    if constexpr (HIST && FORCE) p.b_before = b_prev[r];
    return p;
  }
  template <bool FORCE>
  __device__ void flux(int64_t r, double F, const Pre<FORCE>& p) const {
    NSS_ST(ext[r], extrapolated<HIST>(w, F, p.before));
    NSS_ST(prev[r], F);
  }
  __device__ void force(int64_t r, double w_b, double excess, double f, const Pre<true>& p) const {
    const double b = w_b * excess;
    NSS_ST(f_eff[r], f + extrapolated<HIST>(w, b, p.b_before));
    NSS_ST(b_prev[r], b);
  }
};

struct DonorOps {
  const int32_t *adv_col, *avg_col, *diff_col;
  const double *adv_val, *avg_val, *diff_val;
};

// F1: one lane per flux point.  The six slots of the three rows are requested first, then the six gathers of u and the
// history, then the arithmetic of upwind_flux_kernel (blas1.hip) on the three row sums.
template <class Out>
__global__ __launch_bounds__(kBlock) void step_flux_kernel(const int32_t* __restrict__ done, int32_t nflux, DonorOps m,
                                                            const double* __restrict__ u, Out out) {
  if (step_done(done)) return;
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t r = int64_t(blockIdx.x) * kBlock + threadIdx.x; r < nflux; r += stride) {
    const int2v ca = __builtin_nontemporal_load(reinterpret_cast<const int2v*>(m.adv_col) + r);
    const int2v cm = __builtin_nontemporal_load(reinterpret_cast<const int2v*>(m.avg_col) + r);
    const int2v cj = __builtin_nontemporal_load(reinterpret_cast<const int2v*>(m.diff_col) + r);
    const dbl2v va = __builtin_nontemporal_load(reinterpret_cast<const dbl2v*>(m.adv_val) + r);
    const dbl2v vm = __builtin_nontemporal_load(reinterpret_cast<const dbl2v*>(m.avg_val) + r);
    const dbl2v vj = __builtin_nontemporal_load(reinterpret_cast<const dbl2v*>(m.diff_val) + r);
    const auto pre = out.template fetch<false>(r);
    const double a0 = u[present(ca.x)], a1 = u[present(ca.y)];
    const double m0 = u[present(cm.x)], m1 = u[present(cm.y)];
    const double j0 = u[present(cj.x)], j1 = u[present(cj.y)];
    pre.in_flight_with(a0, a1, m0, m1, j0, j1);
    out.flux(r, donor_flux(two_slot_sum(ca, va, a0, a1), two_slot_sum(cm, vm, m0, m1), two_slot_sum(cj, vj, j0, j1)),
             pre);
  }
}

// F1': one lane per flux point.  The stencil row and the two slots of adv are requested first, then all six gathers of
// u -- the four stencil values whatever the sign of a, so that no load waits for a -- then the selection in registers.
template <int LIM, class Out>
__global__ __launch_bounds__(kBlock) void step_flux_limited_kernel(const int32_t* __restrict__ done, int32_t nflux,
                                                                    const int32_t* __restrict__ adv_col,
                                                                    const double* __restrict__ adv_val,
                                                                    const int32_t* __restrict__ stencil,
                                                                    const double* __restrict__ u, Out out) {
  if (step_done(done)) return;
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t r = int64_t(blockIdx.x) * kBlock + threadIdx.x; r < nflux; r += stride) {
    const int4v c = __builtin_nontemporal_load(reinterpret_cast<const int4v*>(stencil) + r);
    const int2v ca = __builtin_nontemporal_load(reinterpret_cast<const int2v*>(adv_col) + r);
    const dbl2v va = __builtin_nontemporal_load(reinterpret_cast<const dbl2v*>(adv_val) + r);
    const auto pre = out.template fetch<false>(r);
    const double a0 = u[present(ca.x)], a1 = u[present(ca.y)];
    const double g_ll = u[present(c.x)], g_lo = u[present(c.y)], g_hi = u[present(c.z)], g_hh = u[present(c.w)];
    pre.in_flight_with(a0, a1, g_ll, g_lo, g_hi, g_hh);
    const double a = two_slot_sum(ca, va, a0, a1);
    out.flux(r, limited_face<LIM>(a, c, or_zero(c.x, g_ll), or_zero(c.y, g_lo), or_zero(c.z, g_hi), or_zero(c.w, g_hh)),
             pre);
  }
}

// S1: one lane per face.  The four slots of the two rows are requested first, then the gathers of T together (on a grid
// avg and diff share their columns: the second pair hits the lines of the first), then the arithmetic of
// step_flux_kernel with the face's own velocity as the advecting one.
template <bool BUOYANT, class Out>
__global__ __launch_bounds__(kBlock) void scalar_flux_kernel(const int32_t* __restrict__ done, int32_t nface,
                                                              const int32_t* __restrict__ avg_col,
                                                              const double* __restrict__ avg_val,
                                                              const int32_t* __restrict__ diff_col,
                                                              const double* __restrict__ diff_val,
                                                              const double* __restrict__ w_b,
                                                              const double* __restrict__ u, const double* __restrict__ f,
                                                              const double* __restrict__ T, double t_ref, Out out) {
  if (step_done(done)) return;
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t r = int64_t(blockIdx.x) * kBlock + threadIdx.x; r < nface; r += stride) {
    const int2v cm = __builtin_nontemporal_load(reinterpret_cast<const int2v*>(avg_col) + r);
    const int2v cj = __builtin_nontemporal_load(reinterpret_cast<const int2v*>(diff_col) + r);
    const dbl2v vm = __builtin_nontemporal_load(reinterpret_cast<const dbl2v*>(avg_val) + r);
    const dbl2v vj = __builtin_nontemporal_load(reinterpret_cast<const dbl2v*>(diff_val) + r);
    const auto pre = out.template fetch<BUOYANT>(r);
    double wb = 0.0, force = 0.0;
    if constexpr (BUOYANT) wb = w_b[r], force = f[r];
    const double adv = u[r];
    const double m0 = T[present(cm.x)], m1 = T[present(cm.y)];
    const double j0 = T[present(cj.x)], j1 = T[present(cj.y)];
    pre.in_flight_with(adv, m0, m1, j0, j1, wb, force);
    const double avg = two_slot_sum(cm, vm, m0, m1);
    out.flux(r, donor_flux(adv, avg, two_slot_sum(cj, vj, j0, j1)), pre);
    if constexpr (BUOYANT) out.force(r, wb, avg - t_ref, force, pre);
  }
}

// S1': one lane per face; the advecting velocity is the face's own dof
template <int LIM, bool BUOYANT, class Out>
__global__ __launch_bounds__(kBlock) void scalar_flux_limited_kernel(const int32_t* __restrict__ done, int32_t nface,
                                                                      const int32_t* __restrict__ stencil,
                                                                      const double* __restrict__ w_b,
                                                                      const double* __restrict__ u,
                                                                      const double* __restrict__ f,
                                                                      const double* __restrict__ T, double t_ref,
                                                                      Out out) {
  if (step_done(done)) return;
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t r = int64_t(blockIdx.x) * kBlock + threadIdx.x; r < nface; r += stride) {
    const int4v c = __builtin_nontemporal_load(reinterpret_cast<const int4v*>(stencil) + r);
    const auto pre = out.template fetch<BUOYANT>(r);
    double wb = 0.0, force = 0.0;
    if constexpr (BUOYANT) wb = w_b[r], force = f[r];
    const double g_ll = T[present(c.x)], g_lo = T[present(c.y)], g_hi = T[present(c.z)], g_hh = T[present(c.w)];
    const double a = u[r];
    pre.in_flight_with(a, g_ll, g_lo, g_hi, g_hh, wb, force);
    const double q_lo = or_zero(c.y, g_lo), q_hi = or_zero(c.z, g_hi);
    out.flux(r, limited_face<LIM>(a, c, or_zero(c.x, g_ll), q_lo, q_hi, or_zero(c.w, g_hh)), pre);
    if constexpr (BUOYANT) out.force(r, wb, 0.5 * (q_lo + q_hi) - t_ref, force, pre);
  }
}

// ---- the host side: a runtime value becomes a template argument here and nowhere else ----
template <class Fn>
static void with_flag(bool flag, Fn&& fn) {
  if (flag) fn(std::true_type{});
  else fn(std::false_type{});
}

template <class Fn>
static void with_limiter(int32_t limiter, Fn&& fn) {
  if (limiter == kDonor) fn(std::integral_constant<int, kDonor>{});
  else if (limiter == kMinmod) fn(std::integral_constant<int, kMinmod>{});
  else fn(std::integral_constant<int, kVanLeer>{});
}

// the words of a refusal behind the export's own prefix
struct Who {
  const char* name;
  std::string operator()(const char* what) const { return std::string(name) + ": " + what; }
};

// [a, a + na) and [b, b + nb) share an element
static bool overlap(const double* a, int64_t na, const double* b, int64_t nb) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + uintptr_t(nb) * sizeof(double) && b0 < a0 + uintptr_t(na) * sizeof(double);
}

static void require_limiter(const Who& who, int32_t limiter) {
  NSS_REQUIRE(limiter >= kDonor && limiter <= kVanLeer, who("limiter is 0 (donor), 1 (minmod) or 2 (van Leer)"));
}

static void require_aligned(const Who& who, const int32_t* stencil) {
  NSS_REQUIRE(reinterpret_cast<uintptr_t>(stencil) % 16 == 0, who("stencil is not 16-byte aligned"));
}

// The operators of F1: false when there are no flux points (there is no two-slot copy to build).  With unguarded gathers
// an absent entry reads element 0 of u, so adv must have a column.
static bool donor_momentum_rows(const Who& who, nss_csr_t adv, nss_csr_t avg, nss_csr_t diff) {
  NSS_REQUIRE(adv->m == avg->m && adv->m == diff->m && adv->n == avg->n && adv->n == diff->n,
              who("adv, avg and diff differ in shape"));
  require_f64_values(adv, who.name);
  require_f64_values(avg, who.name);
  require_f64_values(diff, who.name);
  if (adv->m == 0) return false;
  NSS_REQUIRE(adv->n >= 1, who("adv has no columns"));
  return true;
}

template <class Out>
static void launch_step_flux(const Who& who, nss_csr_s& adv, nss_csr_s& avg, nss_csr_s& diff, const double* u,
                             const int32_t* done, nss_stream_t stream, Out out) {
  NSS_REQUIRE(fixed_width_copy(adv) && fixed_width_copy(avg) && fixed_width_copy(diff),
              who("a row of adv, avg or diff has more than two entries"));
  const DonorOps m{adv.fw_col, avg.fw_col, diff.fw_col, adv.fw_val, avg.fw_val, diff.fw_val};
  hipLaunchKernelGGL(step_flux_kernel<Out>, dim3(stream_grid(adv.m, kBlock)), dim3(kBlock), 0, as_stream(stream), done,
                     adv.m, m, u, out);
  NSS_CHECK_LAUNCH();
}

// the operands of F1' that do not depend on the output
static void limited_momentum_rows(const Who& who, nss_csr_t adv, const int32_t* stencil, int64_t nflux,
                                  int32_t limiter) {
  require_limiter(who, limiter);
  NSS_REQUIRE(nflux == adv->m, who("nflux is not the row count of adv"));
  NSS_REQUIRE(nflux == 0 || adv->n >= 1, who("adv has no columns"));
  require_aligned(who, stencil);
}

template <class Out>
static void launch_step_flux_limited(const Who& who, nss_csr_s& adv, const int32_t* stencil, int32_t limiter,
                                     const double* u, const int32_t* done, nss_stream_t stream, Out out) {
  NSS_REQUIRE(fixed_width_copy(adv), who("a row of adv has more than two entries"));
  with_limiter(limiter, [&](auto lim) {
    hipLaunchKernelGGL((step_flux_limited_kernel<lim.value, Out>), dim3(stream_grid(adv.m, kBlock)), dim3(kBlock), 0,
                       as_stream(stream), done, adv.m, adv.fw_col, adv.fw_val, stencil, u, out);
  });
  NSS_CHECK_LAUNCH();
}

static dim3 scalar_grid(int64_t nface) {
  const int blocks = stream_grid(nface, kBlock);
  return dim3(blocks < kScalarFluxBlocks ? blocks : kScalarFluxBlocks);
}

// S1 behind the export's own pointer rules.  With unguarded gathers an absent entry reads element 0 of T, so avg must
// have a column.
template <class Out>
static void launch_scalar_flux(const Who& who, nss_csr_s& avg, nss_csr_s& diff, const double* w_b, const double* u,
                               const double* f, const double* T, double t_ref, const int32_t* done, nss_stream_t stream,
                               Out out) {
  require_f64_values(&avg, who.name);
  require_f64_values(&diff, who.name);
  if (avg.m == 0) return;                                  // (no faces: there is no two-slot copy to build)
  NSS_REQUIRE(avg.n >= 1, who("avg has no columns"));
  NSS_REQUIRE(fixed_width_copy(avg) && fixed_width_copy(diff), who("a row of avg or diff has more than two entries"));
  with_flag(w_b != nullptr, [&](auto buoyant) {
    hipLaunchKernelGGL((scalar_flux_kernel<buoyant.value, Out>), scalar_grid(avg.m), dim3(kBlock), 0, as_stream(stream),
                       done, avg.m, avg.fw_col, avg.fw_val, diff.fw_col, diff.fw_val, w_b, u, f, T, t_ref, out);
  });
  NSS_CHECK_LAUNCH();
}

// S1 as the flux of the linearised convection (loop_parts.h): the passive form on (a, v)
void linear_donor_flux(nss_csr_s& avg, nss_csr_s& diff, const double* a, const double* v, double* F, const int32_t* done,
                       hipStream_t st) {
  launch_scalar_flux(Who{"linear_donor_flux"}, avg, diff, nullptr, a, nullptr, v, 0.0, done, st, StoreFlux{F, nullptr});
}

// the operands of S1' that do not depend on the output
static void limited_scalar_rows(const Who& who, const int32_t* stencil, int64_t nface, int32_t limiter) {
  require_limiter(who, limiter);
  NSS_REQUIRE(nface >= 0 && nface <= INT32_MAX, who("nface out of range"));
  require_aligned(who, stencil);
}

template <class Out>
static void launch_scalar_flux_limited(const int32_t* stencil, int64_t nface, int32_t limiter, const double* w_b,
                                       const double* u, const double* f, const double* T, double t_ref,
                                       const int32_t* done, nss_stream_t stream, Out out) {
  if (nface == 0) return;
  with_limiter(limiter, [&](auto lim) {
    with_flag(w_b != nullptr, [&](auto buoyant) {
      hipLaunchKernelGGL((scalar_flux_limited_kernel<lim.value, buoyant.value, Out>), scalar_grid(nface), dim3(kBlock),
                         0, as_stream(stream), done, int32_t(nface), stencil, w_b, u, f, T, t_ref, out);
    });
  });
  NSS_CHECK_LAUNCH();
}

// the pointer rules of the plain scalar forms
static void require_scalar_plain(const Who& who, const double* w_b, const double* u, const double* f, const double* T,
                                 const double* G, const double* f_eff) {
  NSS_REQUIRE(w_b == nullptr || (f && f_eff), who("w_b without f or f_eff"));
  NSS_REQUIRE(G != T && G != u && f_eff != u && f_eff != T, who("an output aliases an operand"));
}

// the pointer rules of the extrapolating scalar forms, `n_T`: the entries of T where the caller knows them (0: only T
// itself is compared)
static void require_scalar_history(const Who& who, int64_t nface, int64_t n_T, const double* w_b, const double* u,
                                   const double* f, const double* T, double* G_prev, double* G_ext, double* b_prev,
                                   double* f_eff) {
  NSS_REQUIRE(u && T && G_prev && G_ext, who("NULL argument"));
  NSS_REQUIRE(w_b == nullptr || (f && f_eff && b_prev), who("w_b without f, f_eff or b_prev"));
  const double* outs[] = {G_prev, G_ext, w_b ? b_prev : nullptr, w_b ? f_eff : nullptr};
  for (int i = 0; i < 4; ++i) {
    if (outs[i] == nullptr) continue;
    NSS_REQUIRE(!overlap(outs[i], nface, u, nface) && !overlap(outs[i], nface, T, n_T > 0 ? n_T : 1),
                who("an output aliases u or T"));
    NSS_REQUIRE(w_b == nullptr || (!overlap(outs[i], nface, w_b, nface) && !overlap(outs[i], nface, f, nface)),
                who("an output aliases w_b or f"));
    for (int j = 0; j < i; ++j)
      NSS_REQUIRE(outs[j] == nullptr || !overlap(outs[i], nface, outs[j], nface), who("two outputs alias"));
  }
}

}  // namespace nss

using namespace nss;

extern "C" {

int nss_step_flux_f64(nss_csr_t adv, nss_csr_t avg, nss_csr_t diff, const double* u, double* flux, const int32_t* done,
                      nss_stream_t stream) {
  return guarded([&] {
    const Who who{"step_flux"};
    NSS_REQUIRE(adv && avg && diff && u && flux, who("NULL argument"));
    if (!donor_momentum_rows(who, adv, avg, diff)) return;
    launch_step_flux(who, *adv, *avg, *diff, u, done, stream, StoreFlux{flux, nullptr});
  });
}

int nss_step_flux_ab2_f64(nss_csr_t adv, nss_csr_t avg, nss_csr_t diff, const double* u, double w_new, double w_old,
                          double* prev, double* ext, const int32_t* done, nss_stream_t stream) {
  return guarded([&] {
    const Who who{"step_flux_ab2"};
    NSS_REQUIRE(adv && avg && diff && u && prev && ext, who("NULL argument"));
    if (!donor_momentum_rows(who, adv, avg, diff)) return;
    NSS_REQUIRE(!overlap(prev, adv->m, ext, adv->m) && !overlap(prev, adv->m, u, adv->n) && !overlap(ext, adv->m, u, adv->n),
                who("prev, ext and u alias"));
    with_flag(w_old != 0.0, [&](auto hist) {
      launch_step_flux(who, *adv, *avg, *diff, u, done, stream,
                       ExtrapolateFlux<hist.value>{{w_new, w_old}, prev, ext, nullptr, nullptr});
    });
  });
}

int nss_step_flux_limited_f64(nss_csr_t adv, const int32_t* stencil, int64_t nflux, int32_t limiter, const double* u,
                              double* flux, const int32_t* done, nss_stream_t stream) {
  return guarded([&] {
    const Who who{"step_flux_limited"};
    NSS_REQUIRE(adv && stencil && u && flux, who("NULL argument"));
    limited_momentum_rows(who, adv, stencil, nflux, limiter);
    NSS_REQUIRE(flux != u, who("flux aliases u"));
    require_f64_values(adv, who.name);
    if (nflux == 0) return;                                // (no flux points: there is no two-slot copy to build)
    launch_step_flux_limited(who, *adv, stencil, limiter, u, done, stream, StoreFlux{flux, nullptr});
  });
}

int nss_step_flux_limited_ab2_f64(nss_csr_t adv, const int32_t* stencil, int64_t nflux, int32_t limiter, const double* u,
                                  double w_new, double w_old, double* prev, double* ext, const int32_t* done,
                                  nss_stream_t stream) {
  return guarded([&] {
    const Who who{"step_flux_limited_ab2"};
    NSS_REQUIRE(adv && stencil && u && prev && ext, who("NULL argument"));
    limited_momentum_rows(who, adv, stencil, nflux, limiter);
    require_f64_values(adv, who.name);
    if (nflux == 0) return;                                // (no flux points: there is no two-slot copy to build)
    NSS_REQUIRE(!overlap(prev, nflux, ext, nflux) && !overlap(prev, nflux, u, adv->n) && !overlap(ext, nflux, u, adv->n),
                who("prev, ext and u alias"));
    with_flag(w_old != 0.0, [&](auto hist) {
      launch_step_flux_limited(who, *adv, stencil, limiter, u, done, stream,
                               ExtrapolateFlux<hist.value>{{w_new, w_old}, prev, ext, nullptr, nullptr});
    });
  });
}

int nss_scalar_flux_f64(nss_csr_t avg, nss_csr_t diff, const double* w_b, const double* u, const double* f,
                        const double* T, double t_ref, double* G, double* f_eff, const int32_t* done,
                        nss_stream_t stream) {
  return guarded([&] {
    const Who who{"scalar_flux"};
    NSS_REQUIRE(avg && diff && u && T && G, who("NULL argument"));
    NSS_REQUIRE(avg->m == diff->m && avg->n == diff->n, who("avg and diff differ in shape"));
    require_scalar_plain(who, w_b, u, f, T, G, f_eff);
    launch_scalar_flux(who, *avg, *diff, w_b, u, f, T, t_ref, done, stream, StoreFlux{G, f_eff});
  });
}

int nss_scalar_flux_ab2_f64(nss_csr_t avg, nss_csr_t diff, const double* w_b, const double* u, const double* f,
                            const double* T, double t_ref, double w_new, double w_old, double* G_prev, double* G_ext,
                            double* b_prev, double* f_eff, const int32_t* done, nss_stream_t stream) {
  return guarded([&] {
    const Who who{"scalar_flux_ab2"};
    NSS_REQUIRE(avg && diff, who("NULL argument"));
    NSS_REQUIRE(avg->m == diff->m && avg->n == diff->n, who("avg and diff differ in shape"));
    require_scalar_history(who, avg->m, avg->n, w_b, u, f, T, G_prev, G_ext, b_prev, f_eff);
    with_flag(w_old != 0.0, [&](auto hist) {
      launch_scalar_flux(who, *avg, *diff, w_b, u, f, T, t_ref, done, stream,
                         ExtrapolateFlux<hist.value>{{w_new, w_old}, G_prev, G_ext, b_prev, f_eff});
    });
  });
}

int nss_scalar_flux_limited_f64(const int32_t* stencil, int64_t nface, int32_t limiter, const double* w_b,
                                const double* u, const double* f, const double* T, double t_ref, double* G,
                                double* f_eff, const int32_t* done, nss_stream_t stream) {
  return guarded([&] {
    const Who who{"scalar_flux_limited"};
    NSS_REQUIRE(stencil && u && T && G, who("NULL argument"));
    limited_scalar_rows(who, stencil, nface, limiter);
    require_scalar_plain(who, w_b, u, f, T, G, f_eff);
    launch_scalar_flux_limited(stencil, nface, limiter, w_b, u, f, T, t_ref, done, stream, StoreFlux{G, f_eff});
  });
}

int nss_scalar_flux_limited_ab2_f64(const int32_t* stencil, int64_t nface, int32_t limiter, const double* w_b,
                                    const double* u, const double* f, const double* T, double t_ref, double w_new,
                                    double w_old, double* G_prev, double* G_ext, double* b_prev, double* f_eff,
                                    const int32_t* done, nss_stream_t stream) {
  return guarded([&] {
    const Who who{"scalar_flux_limited_ab2"};
    NSS_REQUIRE(stencil, who("NULL argument"));
    limited_scalar_rows(who, stencil, nface, limiter);
    require_scalar_history(who, nface, 0, w_b, u, f, T, G_prev, G_ext, b_prev, f_eff);
    with_flag(w_old != 0.0, [&](auto hist) {
      launch_scalar_flux_limited(stencil, nface, limiter, w_b, u, f, T, t_ref, done, stream,
                                 ExtrapolateFlux<hist.value>{{w_new, w_old}, G_prev, G_ext, b_prev, f_eff});
    });
  });
}

}  // extern "C"
