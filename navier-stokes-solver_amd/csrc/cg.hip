// Fused, device-resident preconditioned conjugate gradients (the reference's inner solver
// `CGSolver`, templates/NavierStokesSIMPLE_iterative.py:92,130; BASELINE config 1).
//
//   C1  rows of A    : q = A p, partial <p, q>      (shifted loop: q = m p + sigma A p, EpiCgShiftQ)
//   S1  one workgroup: <p,q> = sum
//   C2  element-wise : alpha = rz / <p,q>;  x += alpha p;  r -= alpha q;  [z = dinv r, partial <r,z>]
//   [P] block Jacobi / Gauss-Seidel / AMG: z = pre r, then partial <r, z>
//   S2  one workgroup: rz_new = sum
//   C3  element-wise : beta = rz_new / rz;  p = z + beta p;  one lane: history, stop test
#include <cfloat>
#include <cmath>

#include "bpcg2.h"

namespace nss {

enum { G_RZ = 0, G_PQ = 1, G_RZN = 2, G_ERR0 = 3, G_TOL = 4, G_RZ_ODD = 5 };
enum { GC_DONE = 0, GC_ITFINAL = 1, GC_LAST = 2 };
__device__ __forceinline__ int rz_slot(int it) { return (it & 1) ? G_RZ_ODD : G_RZ; }

struct EpiCgQ {
  const int32_t* __restrict__ ctrl;
  const double* __restrict__ p;
  double* __restrict__ q;
  double* __restrict__ partials;
  double acc = 0.0;
  __device__ bool skip() const { return ctrl[GC_DONE] != 0; }
  struct Pre { double p = 0.0; };
  __device__ Pre fetch(int r) const { return Pre{p[r]}; }
  __device__ void row(int r, double ap, const Pre& pre) {
    q[r] = ap;
    acc = fma(pre.p, ap, acc);
  }
  __device__ void finish(int b, double* lds) { store_block_partial(acc, b, partials, lds); }
};

// C1 of a shifted loop: q = m p + sigma (A p) with m_r = mass[r], or m0 without a mass vector (uniform lumped mass) --
// the operator M + sigma A of a time step read from A itself, so that one matrix serves every step size
struct EpiCgShiftQ {
  const int32_t* __restrict__ ctrl;
  const double* __restrict__ p;
  const double* __restrict__ mass;
  double m0, sigma;
  double* __restrict__ q;
  double* __restrict__ partials;
  double acc = 0.0;
  __device__ bool skip() const { return ctrl[GC_DONE] != 0; }
  struct Pre { double p = 0.0, m = 0.0; };
  __device__ Pre fetch(int r) const { return Pre{p[r], mass ? mass[r] : m0}; }
  __device__ void row(int r, double ap, const Pre& pre) {
    const double v = fma(sigma, ap, pre.m * pre.p);
    q[r] = v;
    acc = fma(pre.p, v, acc);
  }
  __device__ void finish(int b, double* lds) { store_block_partial(acc, b, partials, lds); }
};

// dinv = 1 / (m + sigma diag(A)): the point-Jacobi preconditioner of the shifted operator
__global__ __launch_bounds__(kBlock) void cg_shift_jacobi_kernel(int32_t n, const double* __restrict__ mass, double m0,
                                                                 double sigma, const double* __restrict__ diag,
                                                                 double* __restrict__ dinv) {
  const int stride = gridDim.x * kBlock;
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += stride)
    dinv[i] = 1.0 / fma(sigma, diag[i], mass ? mass[i] : m0);
}

__global__ __launch_bounds__(kLoopSum) void cg_sum_kernel(const int32_t* __restrict__ ctrl, int n,
                                                          const double* __restrict__ part, double* __restrict__ scal,
                                                          int slot) {
  __shared__ double lds[kLoopSum / kWave];
  if (ctrl[GC_DONE] != 0) return;
  const double t = sum_partials_1024(part, n, lds);
  if (threadIdx.x == 0) {
    scal[slot] = t;
  }
}

struct CgArgs {
  int32_t* ctrl;
  double* scal;
  double* hist;
  int32_t n, it;
  double *x, *r, *z, *p;
  const double *q, *dinv;
  double* partials;
};

// x += alpha p, r -= alpha q; fused point-Jacobi / identity preconditioner with partial <r, z>
__global__ __launch_bounds__(kBlock) void cg_update_kernel(CgArgs a, int fused_pre) {
  __shared__ double lds[kBlock / kWave];
  if (a.ctrl[GC_DONE] != 0) return;
  const double alpha = a.scal[rz_slot(a.it)] / a.scal[G_PQ];
  const int stride = gridDim.x * kBlock;
  double acc = 0.0;
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < a.n; i += stride) {
    NSS_ST(a.x[i], fma(alpha, a.p[i], a.x[i]));
    const double rn = fma(-alpha, a.q[i], a.r[i]);
    a.r[i] = rn;
    if (fused_pre) {
      const double zn = a.dinv ? a.dinv[i] * rn : rn;
      a.z[i] = zn;
      acc = fma(rn, zn, acc);
    }
  }
  if (fused_pre) store_block_partial(acc, blockIdx.x, a.partials, lds);
}

// p = z + beta p; one lane: history, stop test, rz of the next iteration
__global__ __launch_bounds__(kBlock) void cg_direction_kernel(CgArgs a) {
  if (a.ctrl[GC_DONE] != 0) return;
  const double rz = a.scal[rz_slot(a.it)], rzn = a.scal[G_RZN];
  const double beta = rzn / rz;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    a.scal[rz_slot(a.it + 1)] = rzn;
    const double err = sqrt(fabs(rzn));
    a.hist[a.it] = err;
    a.ctrl[GC_LAST] = a.it;
    if (err < a.scal[G_TOL] * a.scal[G_ERR0]) {
      a.ctrl[GC_ITFINAL] = a.it;
      a.ctrl[GC_DONE] = 1;
    }
  }
  const int stride = gridDim.x * kBlock;
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < a.n; i += stride) a.p[i] = fma(beta, a.p[i], a.z[i]);
}

// Start of a solve from x = 0 on the device (nss_cg_start): x = 0, r = b; with a fused preconditioner also z = dinv r,
// p = z and the partials of <r, z>
__global__ __launch_bounds__(kBlock) void cg_start_kernel(CgArgs a, const double* __restrict__ b, int fused_pre) {
  __shared__ double lds[kBlock / kWave];
  const int stride = gridDim.x * kBlock;
  double acc = 0.0;
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < a.n; i += stride) {
    const double rn = b[i];
    a.x[i] = 0.0;
    a.r[i] = rn;
    if (fused_pre) {
      const double zn = a.dinv ? a.dinv[i] * rn : rn;
      a.z[i] = zn;
      a.p[i] = zn;
      acc = fma(rn, zn, acc);
    }
  }
  if (fused_pre) store_block_partial(acc, blockIdx.x, a.partials, lds);
}

// p = z and the partials of <r, z> behind a preconditioner that is a launch of its own
__global__ __launch_bounds__(kBlock) void cg_start_direction_kernel(CgArgs a) {
  __shared__ double lds[kBlock / kWave];
  const int stride = gridDim.x * kBlock;
  double acc = 0.0;
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < a.n; i += stride) {
    const double zn = a.z[i];
    a.p[i] = zn;
    acc = fma(a.r[i], zn, acc);
  }
  store_block_partial(acc, blockIdx.x, a.partials, lds);
}

// rz = the sum, err0, tol and a cleared control word; a zero right-hand side ends the solve
// before its first iteration (done, it_final = -1: no iterations)
__global__ __launch_bounds__(kLoopSum) void cg_start_sum_kernel(int32_t* __restrict__ ctrl, int n,
                                                                const double* __restrict__ part, double* __restrict__ scal,
                                                                double tol) {
  __shared__ double lds[kLoopSum / kWave];
  const double t = sum_partials_1024(part, n, lds);
  if (threadIdx.x == 0) {
    const double err0 = sqrt(fabs(t));
    scal[G_RZ] = t;
    scal[G_PQ] = 0.0;
    scal[G_RZN] = 0.0;
    scal[G_ERR0] = err0;
    scal[G_TOL] = tol;
    scal[G_RZ_ODD] = 0.0;
    ctrl[GC_DONE] = err0 == 0.0 ? 1 : 0;
    ctrl[GC_ITFINAL] = -1;
    ctrl[GC_LAST] = -1;
  }
}

static int cg_grid(const nss_cg_t& s) { return stream_grid(s.n, kBlock * 4); }

static void cg_check(const nss_cg_t* s) {
  NSS_REQUIRE(s != nullptr && s->A != nullptr, "cg: NULL state / matrix");
  NSS_REQUIRE(s->A->m == s->n && s->A->n == s->n, "cg: matrix does not match n");
  pre_a_check(pre_a_of(*s, s->n), "cg", kPreAOnePartAtMost);
  NSS_REQUIRE(s->x && s->r && s->z && s->p && s->q && s->scal && s->ctrl && s->hist && s->partials_a && s->partials_b,
              "cg: NULL buffer");
  NSS_REQUIRE(s->shift_sigma == 0.0 || (std::isfinite(s->shift_sigma) && !s->pre_bjac && !s->pre_amg),
              "cg: a shifted loop takes a finite sigma and the point-Jacobi preconditioner only");
  const int64_t need[2] = {s->A->nblk, std::max<int64_t>(cg_grid(*s), s->pre_bjac ? bjac_dot_grid(*s->pre_bjac) : 0)};
  const int64_t cap[2] = {s->cap_a, s->cap_b};     // (need = nss_cg_workspace)
  check_plan("cg", plan_stamp({s->A}), s->plan_gen, need, cap, 2);
}

static void cg_iteration(const nss_cg_t& s, int it, hipStream_t st) {
  if (s.shift_sigma == 0.0)
    launch_csr(*s.A, s.p, EpiCgQ{s.ctrl, s.p, s.q, s.partials_a}, st);
  else
    launch_csr<kF32 | kCodes>(*s.A, s.p, EpiCgShiftQ{s.ctrl, s.p, s.shift_mass, s.shift_m0, s.shift_sigma, s.q, s.partials_a},
                              st);      // (every value form of A: a step's operator may be stored in fp32 or as codes)
  hipLaunchKernelGGL(cg_sum_kernel, dim3(1), dim3(kLoopSum), 0, st, s.ctrl, s.A->nblk, s.partials_a, s.scal, int(G_PQ));
  NSS_CHECK_LAUNCH();
  const bool fused_pre = !s.pre_bjac && !s.pre_amg;
  CgArgs a{s.ctrl, s.scal, s.hist, s.n, it, s.x, s.r, s.z, s.p, s.q, s.pre_diag, s.partials_b};
  hipLaunchKernelGGL(cg_update_kernel, dim3(cg_grid(s)), dim3(kBlock), 0, st, a, fused_pre ? 1 : 0);
  NSS_CHECK_LAUNCH();
  int nb = cg_grid(s);
  if (!fused_pre) {
    if (s.pre_bjac && !s.pre_bjac->gs_mat) {   // block Jacobi: <r, z> comes out of the apply kernel
      nb = bjac_apply_dot(*s.pre_bjac, 1.0, s.r, s.z, s.partials_b, s.ctrl, st);
    } else {
      pre_a_apply(pre_a_of(s, s.n), 1.0, s.r, s.z, nullptr, s.ctrl, st);   // Gauss-Seidel sweep as an operator, or V-cycle
      launch_dot_partials(StopWord{s.ctrl, GC_DONE}, nb, s.n, s.r, s.z, s.partials_b, st);
    }
  }
  hipLaunchKernelGGL(cg_sum_kernel, dim3(1), dim3(kLoopSum), 0, st, s.ctrl, nb, s.partials_b, s.scal, int(G_RZN));
  NSS_CHECK_LAUNCH();
  hipLaunchKernelGGL(cg_direction_kernel, dim3(cg_grid(s)), dim3(kBlock), 0, st, a);
  NSS_CHECK_LAUNCH();
}

}  // namespace nss

using namespace nss;

extern "C" {

int nss_cg_workspace(const nss_cg_t* s, int64_t* partials_a, int64_t* partials_b) {
  return guarded([&] {
    NSS_REQUIRE(s && s->A, "cg_workspace: NULL state / matrix");
    if (partials_a) *partials_a = s->A->nblk;
    if (partials_b) *partials_b = std::max<int64_t>(cg_grid(*s), s->pre_bjac ? bjac_dot_grid(*s->pre_bjac) : 0);
  });
}

int nss_cg_start(const nss_cg_t* s, const double* b, double tol, nss_stream_t stream) {
  return guarded([&] {
    cg_check(s);
    NSS_REQUIRE(b != nullptr && b != s->x && b != s->r, "cg_start: NULL right-hand side, or it aliases x / r");
    hipStream_t st = as_stream(stream);
    const bool fused_pre = !s->pre_bjac && !s->pre_amg;
    CgArgs a{s->ctrl, s->scal, s->hist, s->n, 0, s->x, s->r, s->z, s->p, s->q, s->pre_diag, s->partials_b};
    const int nb = cg_grid(*s);
    hipLaunchKernelGGL(cg_start_kernel, dim3(nb), dim3(kBlock), 0, st, a, b, fused_pre ? 1 : 0);
    NSS_CHECK_LAUNCH();
    if (!fused_pre) {
      pre_a_apply(pre_a_of(*s, s->n), 1.0, s->r, s->z, nullptr, nullptr, st);
      hipLaunchKernelGGL(cg_start_direction_kernel, dim3(nb), dim3(kBlock), 0, st, a);
      NSS_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(cg_start_sum_kernel, dim3(1), dim3(kLoopSum), 0, st, s->ctrl, nb, s->partials_b, s->scal, tol);
    NSS_CHECK_LAUNCH();
  });
}

int nss_cg_iterate(const nss_cg_t* s, int32_t it_begin, int32_t it_end, nss_stream_t stream) {
  return guarded([&] {
    cg_check(s);
    for (int it = it_begin; it < it_end; ++it) cg_iteration(*s, it, as_stream(stream));
  });
}

int nss_cg_shift_jacobi_f64(int64_t n, const double* mass, double m0, double sigma, const double* diag, double* dinv,
                            nss_stream_t stream) {
  return guarded([&] {
    NSS_REQUIRE(n >= 0 && n <= INT32_MAX && diag && dinv, "cg_shift_jacobi: NULL argument, or n outside int32");
    if (n == 0) return;
    hipLaunchKernelGGL(cg_shift_jacobi_kernel, dim3(stream_grid(n, kBlock)), dim3(kBlock), 0, as_stream(stream),
                       int32_t(n), mass, m0, sigma, diag, dinv);
    NSS_CHECK_LAUNCH();
  });
}

int nss_cg_poll(const nss_cg_t* s, int32_t* done, int32_t* it_final, int32_t* last_it, nss_stream_t stream) {
  return guarded([&] {
    NSS_REQUIRE(s && s->ctrl, "cg_poll: NULL state");
    int32_t h[4] = {0, 0, 0, 0};
    poll_ctrl(s->ctrl, as_stream(stream), h);
    if (done) *done = h[GC_DONE];
    if (it_final) *it_final = h[GC_ITFINAL];
    if (last_it) *last_it = h[GC_LAST];
  });
}

}  // extern "C"
