// Kernels of the device-resident IMEX time step (`NavierStokes.Advance`; the reference's DoTimeStep / Project,
// templates/NavierStokesSIMPLE_iterative.py:424-443).  One step is
//
//   F1  flux points     : F = adv*avg - |adv| diff / 2 with adv = I_adv u, avg = Avg u, diff = Diff u, written behind u
//                         in ONE operand buffer [u | F]                           (step_flux_kernel, flux.hip)
//   F2  rows of [A | D] : temp = f - [A | D] [u | F]  ( = conv(u) + f - A u, conv = -D F )  (EpiStepRhs)
//   ..  raw = mstar^-1 temp, phi = (B M^-1 B^T)^-1 B raw                                    (the fused CG loop, cg.hip)
//   P1  rows of C       : out = raw - C phi;  u += tau out;  partials of <u, M u>           (EpiStepProject)
//   P2  rows of B       : partials of |B u|^2                                               (step_div_kernel, optional)
//   P3  one workgroup   : record[step] = { <u, M u> / 2, |B u| }                            (step_record_kernel)
// and, for a variable step, at the head
//   R1  rows of B       : per workgroup max_r w_r sum_p |B_rp| |u_p|                            (step_cfl_kernel)
//   R2  one workgroup   : rates[step] = the maximum                                             (step_cfl_max_kernel)
//
// All fp64, no atomics: every sum is per-workgroup partials added by the fixed tree (fixed_sums_1024).
#include <cfloat>
#include <cmath>

#include "bpcg2.h"

namespace nss {

// F2: temp = f - (row of [A | D]) . [u | F]
struct EpiStepRhs {
  const int32_t* __restrict__ done;
  const double* __restrict__ f;
  double* __restrict__ out;
  struct Pre { double f = 0.0; };
  __device__ bool skip() const { return step_done(done); }
  __device__ Pre fetch(int r) const { return Pre{f[r]}; }
  __device__ void row(int r, double ax, const Pre& p) const { NSS_ST(out[r], p.f - ax); }
  __device__ void finish(int, double*) const {}
};

// P1: out = raw - C phi (out may be raw itself);  with u: u += tau out;  partials of sum_r m_r e_r^2 over the row block,
// e = the updated u, or out without u (m_r = 1 without mass)
struct EpiStepProject {
  const int32_t* __restrict__ done;
  const double* raw;
  double* out;
  double* u;
  const double* __restrict__ mass;
  double tau;
  double* __restrict__ partials;
  double acc = 0.0;
  struct Pre { double raw = 0.0, u = 0.0, m = 1.0; };
  __device__ bool skip() const { return step_done(done); }
  __device__ Pre fetch(int r) const { return Pre{raw[r], u ? u[r] : 0.0, mass ? mass[r] : 1.0}; }
  __device__ void row(int r, double cphi, const Pre& p) {
    const double t = p.raw - cphi;
    out[r] = t;
    double e = t;
    if (u) {
      e = fma(tau, t, p.u);
      u[r] = e;
    }
    acc = fma(p.m * e, e, acc);
  }
  __device__ void finish(int b, double* lds) {
    if (partials != nullptr) store_block_partial(acc, b, partials, lds);
  }
};

// P2: partials of |B u|^2, one lane per row.  The row is summed entry after entry with products rounded on their own --
// the order of a host CSR product -- because B u of a projected field is what cancellation leaves of terms 1e8 times
// larger: summed in another order the diagnostic could not be checked against a host recomputation beyond a few digits.
__global__ __launch_bounds__(kBlock) void step_div_kernel(const int32_t* __restrict__ done, int32_t m,
                                                           const int32_t* __restrict__ rowptr,
                                                           const int32_t* __restrict__ col, const double* __restrict__ val,
                                                           const double* __restrict__ u, double* __restrict__ partials) {
  __shared__ double lds[kBlock / kWave];
  if (step_done(done)) return;
  const int stride = gridDim.x * kBlock;
  double acc = 0.0;
  for (int r = blockIdx.x * kBlock + threadIdx.x; r < m; r += stride) {
    const int s = rowptr[r], e = rowptr[r + 1];
    double sum = 0.0;
    for (int p = s; p < e; ++p) sum += mul_unfused(val[p], u[col[p]]);
    acc = fma(sum, sum, acc);
  }
  store_block_partial(acc, blockIdx.x, partials, lds);
}

// P3: record[2 slot] = scale * sum pk (the kinetic energy), record[2 slot + 1] = sqrt(sum pd) (NaN without pd)
__global__ __launch_bounds__(kBlock) void step_record_kernel(const int32_t* __restrict__ done,
                                                              const double* __restrict__ pk, int nk,
                                                              const double* __restrict__ pd, int nd, double scale,
                                                              double* __restrict__ record, int slot) {
  __shared__ double lds[kRedDoubles];
  if (step_done(done)) return;
  const SumPair s = fixed_sums_1024(pk, nk, pd ? pd : pk, pd ? nd : 0, lds);
  if (threadIdx.x == 0) {
    record[2 * slot] = scale * s.a;
    record[2 * slot + 1] = pd ? sqrt(s.b) : __builtin_nan("");
  }
}

// Maximum over a kBlock-thread workgroup of values that are not NaN, valid in thread 0.  `lds`: kBlock / kWave doubles.
__device__ __forceinline__ double block_max(double v, double* lds) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, kWave));
  if ((threadIdx.x & (kWave - 1)) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = lds[0];
#pragma unroll
  for (int w = 1; w < kBlock / kWave; ++w) t = fmax(t, lds[w]);
  return t;
}

// the rate of one row, w * sum, with anything that is not finite (NaN included, which fmax would drop) as +inf
__device__ __forceinline__ double cfl_rate(double w, double sum) {
  const double v = mul_unfused(w, sum);
  return v <= DBL_MAX ? v : __builtin_inf();
}

// R1: per workgroup the maximum of w_r sum_p |val_p| |u[col_p]| over the rows of B (w_r = inv_mass[r], or scale), one
// lane per row, summed entry after entry with products rounded on their own like step_div_kernel: the value can be
// compared for equality with a host CSR product.  On the plain grid this is max_cell sum_faces |u_f| / h.
__global__ __launch_bounds__(kBlock) void step_cfl_kernel(const int32_t* __restrict__ done, int32_t m,
                                                           const int32_t* __restrict__ rowptr,
                                                           const int32_t* __restrict__ col, const double* __restrict__ val,
                                                           const double* __restrict__ u,
                                                           const double* __restrict__ inv_mass, double scale,
                                                           double* __restrict__ partials) {
  __shared__ double lds[kBlock / kWave];
  if (step_done(done)) return;
  const int stride = gridDim.x * kBlock;
  double top = 0.0;
  for (int r = blockIdx.x * kBlock + threadIdx.x; r < m; r += stride) {
    const int s = rowptr[r], e = rowptr[r + 1];
    double sum = 0.0;
    for (int p = s; p < e; ++p) sum += mul_unfused(fabs(val[p]), fabs(u[col[p]]));
    top = fmax(top, cfl_rate(inv_mass ? inv_mass[r] : scale, sum));
  }
  top = block_max(top, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = top;
}

// R2: out[slot] = the maximum of the n partials, by one workgroup (the order does not matter for a maximum)
__global__ __launch_bounds__(kBlock) void step_cfl_max_kernel(const int32_t* __restrict__ done,
                                                               const double* __restrict__ partials, int n,
                                                               double* __restrict__ out, int slot) {
  __shared__ double lds[kBlock / kWave];
  if (step_done(done)) return;
  double top = 0.0;
  for (int i = threadIdx.x; i < n; i += kBlock) top = fmax(top, partials[i]);
  top = block_max(top, lds);
  if (threadIdx.x == 0) out[slot] = top;
}

static int div_grid(const nss_csr_s& B) { return stream_grid(B.m, kBlock); }

}  // namespace nss

using namespace nss;

extern "C" {

int nss_step_rhs_f64(nss_csr_t ad, const double* uf, const double* f, double* temp, const int32_t* done,
                     nss_stream_t stream) {
  return guarded([&] {
    NSS_REQUIRE(ad && uf && f && temp, "step_rhs: NULL argument");
    NSS_REQUIRE(temp != uf && temp != f, "step_rhs: temp aliases an operand");
    launch_csr(*ad, uf, EpiStepRhs{done, f, temp}, as_stream(stream));
  });
}

int nss_step_project_f64(nss_csr_t c, const double* phi, const double* raw, double* out, double* u, double tau,
                         const double* mass, double* partials, int64_t cap, const int32_t* done, nss_stream_t stream) {
  return guarded([&] {
    NSS_REQUIRE(c && phi && raw && out, "step_project: NULL argument");
    NSS_REQUIRE(u != out && u != raw, "step_project: u aliases raw / out");
    require_f64_values(c, "step_project");
    if (c->m == 0) return;                                 // (no rows: there is no two-slot copy to build)
    NSS_REQUIRE(fixed_width_copy(*c), "step_project: a row of C has more than two entries");
    NSS_REQUIRE(partials == nullptr || cap >= c->nblk, "step_project: partials hold fewer entries than C has row blocks");
    const EpiStepProject epi{done, raw, out, u, mass, tau, partials};
    hipLaunchKernelGGL((csr_direct_kernel<EpiStepProject>), dim3(nss_csr_s::grid(c->nblk)), dim3(kBlock), 0,
                       as_stream(stream), c->view(0, c->nblk, 0), c->fw_col, c->fw_val, (const uint16_t*)nullptr,
                       (const int32_t*)nullptr, phi, epi);
    NSS_CHECK_LAUNCH();
  });
}

int nss_step_divergence_f64(nss_csr_t b, const double* u, double* partials, int64_t cap, const int32_t* done,
                            nss_stream_t stream) {
  return guarded([&] {
    NSS_REQUIRE(b && u && partials, "step_divergence: NULL argument");
    require_f64_values(b, "step_divergence");
    NSS_REQUIRE(cap >= div_grid(*b), "step_divergence: partials hold fewer entries than nss_step_workspace asks for");
    hipLaunchKernelGGL(step_div_kernel, dim3(div_grid(*b)), dim3(kBlock), 0, as_stream(stream), done, b->m, b->rowptr,
                       b->col, b->val, u, partials);
    NSS_CHECK_LAUNCH();
  });
}

int nss_step_workspace(nss_csr_t c, nss_csr_t b, int64_t* partials_energy, int64_t* partials_div) {
  return guarded([&] {
    NSS_REQUIRE(c && b, "step_workspace: NULL matrix");
    if (partials_energy) *partials_energy = c->nblk;
    if (partials_div) *partials_div = div_grid(*b);
  });
}

int nss_step_cfl_workspace(nss_csr_t b, int64_t* partials) {
  return guarded([&] {
    NSS_REQUIRE(b && partials, "step_cfl_workspace: NULL argument");
    *partials = div_grid(*b);
  });
}

int nss_step_cfl_f64(nss_csr_t b, const double* u, const double* inv_mass, double scale, double* partials, int64_t cap,
                     double* out, int32_t slot, const int32_t* done, nss_stream_t stream) {
  return guarded([&] {
    NSS_REQUIRE(b && u && partials && out && slot >= 0, "step_cfl: NULL argument or a negative slot");
    require_f64_values(b, "step_cfl");
    const int grid = div_grid(*b);
    NSS_REQUIRE(cap >= grid, "step_cfl: partials hold fewer entries than nss_step_cfl_workspace asks for");
    hipLaunchKernelGGL(step_cfl_kernel, dim3(grid), dim3(kBlock), 0, as_stream(stream), done, b->m, b->rowptr, b->col,
                       b->val, u, inv_mass, scale, partials);
    NSS_CHECK_LAUNCH();
    hipLaunchKernelGGL(step_cfl_max_kernel, dim3(1), dim3(kBlock), 0, as_stream(stream), done, partials, grid, out,
                       int(slot));
    NSS_CHECK_LAUNCH();
  });
}

int nss_step_record_f64(const double* partials_energy, int64_t n_energy, const double* partials_div, int64_t n_div,
                        double scale, double* record, int32_t slot, const int32_t* done, nss_stream_t stream) {
  return guarded([&] {
    NSS_REQUIRE(partials_energy && record && slot >= 0 && n_energy >= 0 && n_div >= 0, "step_record: bad argument");
    hipLaunchKernelGGL(step_record_kernel, dim3(1), dim3(kBlock), 0, as_stream(stream), done, partials_energy,
                       int(n_energy), partials_div, int(n_div), scale, record, int(slot));
    NSS_CHECK_LAUNCH();
  });
}

}  // extern "C"
