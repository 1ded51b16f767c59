// Kernels of the scalar (temperature) transport inside the device-resident time step (`NavierStokes.AddScalar` /
// `Advance`): a cell-centred T carried by the face velocities, diffused implicitly, and fed back into the momentum
// equation as a Boussinesq force.  One step adds, around the velocity step of step.hip,
//
//   S1  faces           : G = u (avg T) - |u| (diff T) / 2 written behind T in ONE operand buffer [T | G];
//                         f_eff = f + w_b (avg T - T_ref)                        (scalar_flux_kernel, flux.hip)
//   S2  rows of [K | B] : temp_T = q - [K | B] [T | G]                                     (EpiStepRhs, step.hip)
//   ..  delta = (M_p + tau K)^-1 temp_T                                                    (the fused CG loop, cg.hip)
//   S3  cells           : T += tau delta;  partials of <w, T>                              (scalar_update_kernel)
//   S4  one workgroup   : record[step] = c0 - <w, T>  (the heat entering through a wall)   (scalar_record_kernel)
//
// All fp64, no atomics: the sum is per-workgroup partials added by the fixed tree (fixed_sums_1024).
#include "csr_stream.h"
#include "loop_parts.h"

namespace nss {

// S3: T += tau delta; with w: partials[workgroup] of sum_i w_i T_i over the updated T
__global__ __launch_bounds__(kBlock) void scalar_update_kernel(const int32_t* __restrict__ done, int32_t n, double tau,
                                                                const double* __restrict__ delta, double* __restrict__ T,
                                                                const double* __restrict__ w,
                                                                double* __restrict__ partials) {
  __shared__ double lds[kBlock / kWave];
  if (step_done(done)) return;
  const int stride = gridDim.x * kBlock;
  double acc = 0.0;
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const double t = fma(tau, delta[i], T[i]);
    T[i] = t;
    if (w != nullptr) acc = fma(w[i], t, acc);
  }
  if (w != nullptr) store_block_partial(acc, blockIdx.x, partials, lds);
}

// S4: record[slot] = c0 - sum partials
__global__ __launch_bounds__(kBlock) void scalar_record_kernel(const int32_t* __restrict__ done,
                                                                const double* __restrict__ partials, int n, double c0,
                                                                double* __restrict__ record, int slot) {
  __shared__ double lds[kRedDoubles];
  if (step_done(done)) return;
  const SumPair s = fixed_sums_1024(partials, n, partials, 0, lds);
  if (threadIdx.x == 0) record[slot] = c0 - s.a;
}

static int update_grid(int64_t n) { return stream_grid(n, kBlock); }

}  // namespace nss

using namespace nss;

extern "C" {

int nss_scalar_workspace(int64_t n, int64_t* partials) {
  return guarded([&] {
    NSS_REQUIRE(n >= 0 && n <= INT32_MAX && partials, "scalar_workspace: bad argument");
    *partials = update_grid(n);
  });
}

int nss_scalar_update_f64(int64_t n, double tau, const double* delta, double* T, const double* w, double* partials,
                          int64_t cap, const int32_t* done, nss_stream_t stream) {
  return guarded([&] {
    NSS_REQUIRE(n >= 0 && n <= INT32_MAX && delta && T && delta != T, "scalar_update: bad argument");
    NSS_REQUIRE((w == nullptr) == (partials == nullptr), "scalar_update: w and partials go together");
    NSS_REQUIRE(partials == nullptr || cap >= update_grid(n),
                "scalar_update: partials hold fewer entries than nss_scalar_workspace asks for");
    hipLaunchKernelGGL(scalar_update_kernel, dim3(update_grid(n)), dim3(kBlock), 0, as_stream(stream), done, int32_t(n),
                       tau, delta, T, w, partials);
    NSS_CHECK_LAUNCH();
  });
}

int nss_scalar_record_f64(const double* partials, int64_t n, double c0, double* record, int32_t slot,
                          const int32_t* done, nss_stream_t stream) {
  return guarded([&] {
    NSS_REQUIRE(partials && record && slot >= 0 && n >= 0 && n <= INT32_MAX, "scalar_record: bad argument");
    hipLaunchKernelGGL(scalar_record_kernel, dim3(1), dim3(kBlock), 0, as_stream(stream), done, partials, int(n), c0,
                       record, int(slot));
    NSS_CHECK_LAUNCH();
  });
}

}  // extern "C"
