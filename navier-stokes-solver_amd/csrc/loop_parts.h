// The small parts the device-resident loops (cg, bicgstab, lanczos, minres, bpcg1, bpcg2, step, heat) are put together
// from, said once: the dot-partial finish of a kernel, the sum of such partials by one 1024-thread workgroup, the guarded
// dot kernel, the poll of a loop's control words and the setter of a plan override.
// Three sum trees exist, each with its own bits: fixed_sums_1024 (nss_common.h: minres, bpcg2, bicgstab, step, heat, the
// folded forms of bpcg1 and lanczos), sum_partials_1024 below (cg, the stand-alone sums of lanczos) and the
// one-accumulator, two-input tree of bpcg1_scalar_kernel (bpcg1.hip).
#pragma once

#include "nss_common.h"

namespace nss {

// partials[b] = the workgroup's sum of acc (b < 0: a workgroup without a row block of its own stores nothing)
__device__ __forceinline__ void store_block_partial(double acc, int b, double* partials, double* lds) {
  const double s = block_sum(acc, lds);
  if (threadIdx.x == 0 && b >= 0) partials[b] = s;
}

// Sum of part[0 .. n) by one workgroup of kLoopSum threads, valid in thread 0: two strided accumulators per lane, a
// 64-lane butterfly per wave, the 16 wave sums added in wave order.  `lds`: kLoopSum / kWave doubles.
constexpr int kLoopSum = 1024;
__device__ __forceinline__ double sum_partials_1024(const double* __restrict__ part, int n, double* lds) {
  double a = 0.0, a2 = 0.0;
  int i = threadIdx.x;
  for (; i + kLoopSum < n; i += 2 * kLoopSum) {
    a += part[i];
    a2 += part[i + kLoopSum];
  }
  for (; i < n; i += kLoopSum) a += part[i];
  const double s = wave_sum(a + a2);
  if ((threadIdx.x & (kWave - 1)) == 0) lds[threadIdx.x >> 6] = s;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < kLoopSum / kWave; ++w) t += lds[w];
  return t;
}

// ---- the parts the kernels of the time step share (step.hip, scalar.hip) ----
typedef int32_t int2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ bool step_done(const int32_t* done) { return done != nullptr && *done != 0; }

// the row sum of a two-slot row as csr_direct_kernel forms it: 0 + p0 + p1, products rounded on their own
__device__ __forceinline__ double two_slot_sum(const int2v& c, const dbl2v& v, double x0, double x1) {
  double sum = 0.0;
  if (c.x >= 0) sum += mul_unfused(v.x, x0);
  if (c.y >= 0) sum += mul_unfused(v.y, x1);
  return sum;
}

// the donor-cell flux of the three row sums, as step_flux_kernel and scalar_flux_kernel write it
__device__ __forceinline__ double donor_flux(double adv, double avg, double dif) {
  return fma(adv, avg, -0.5 * (fabs(adv) * dif));
}

// F[r] = donor_flux(a[r], (avg v)_r, (diff v)_r) over the two-slot copies of avg and diff (which the caller has built:
// fixed_width_copy): the scalar flux launch S1 of flux.hip without a force, with the frozen advecting vector `a` in the
// place of the face velocities and `v` in the place of T -- the flux of the linearised convection (bicgstab.hip)
void linear_donor_flux(nss_csr_s& avg, nss_csr_s& diff, const double* a, const double* v, double* F, const int32_t* done,
                       hipStream_t st);
// the entries of the vector an nss_fdmc_t was made for, and nss_fdmc_solve_f64 with a `done` word (device int, may be
// NULL): every pass returns at once when it is non-zero (fdm_components.hip)
int64_t fdmc_rows(const nss_fdmc_s& h);
void fdmc_solve(const nss_fdmc_s& h, double sigma, const double* rhs, double* out, const int32_t* done, hipStream_t st);

// the stop test of a loop that freezes once one control word is set (cg, lanczos)
struct StopWord {
  const int32_t* __restrict__ ctrl;
  int word;
  __device__ bool operator()() const { return ctrl[word] != 0; }
};

// partials[workgroup] of <x, y> behind a preconditioner that is a launch of its own; `stop` (a functor, by value): the
// loop is frozen, nothing is written
template <class Stop>
__global__ __launch_bounds__(kBlock) void dot_partials_kernel(Stop stop, int32_t n, const double* __restrict__ x,
                                                               const double* __restrict__ y,
                                                               double* __restrict__ partials) {
  __shared__ double lds[kBlock / kWave];
  if (stop()) return;
  const int stride = gridDim.x * kBlock;
  double acc = 0.0;
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) acc = fma(x[i], y[i], acc);
  store_block_partial(acc, blockIdx.x, partials, lds);
}

template <class Stop>
inline void launch_dot_partials(Stop stop, int grid, int32_t n, const double* x, const double* y, double* partials,
                                hipStream_t st) {
  hipLaunchKernelGGL((dot_partials_kernel<Stop>), dim3(grid), dim3(kBlock), 0, st, stop, n, x, y, partials);
  NSS_CHECK_LAUNCH();
}

// the four control words of a loop, on the host once everything enqueued on `st` has run
inline void poll_ctrl(const int32_t* ctrl, hipStream_t st, int32_t (&h)[4]) {
  NSS_HIP(hipMemcpyAsync(h, ctrl, sizeof h, hipMemcpyDeviceToHost, st));
  NSS_HIP(hipStreamSynchronize(st));
}

// a plan override (nss_*_fold_mode, nss_*_fuse_mode): `msg` names the values lo .. hi
inline void set_mode(int& g, int32_t mode, int lo, int hi, const char* msg) {
  NSS_REQUIRE(mode >= lo && mode <= hi, msg);
  g = mode;
}

}  // namespace nss
