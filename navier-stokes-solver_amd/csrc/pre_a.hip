// One check and one apply routine of the velocity preconditioner for the five device loops (pre_a.h).
#include "dist.h"
#include "fdm_inverse.h"

namespace nss {

// r = scale * x - A y  (multiplicative MypreA: the residual between the two sweeps, :379)
struct EpiScaledResidual {
  const int32_t* __restrict__ done;
  double scale;
  const double* __restrict__ x;
  double* __restrict__ r;
  __device__ bool skip() const { return done && *done != 0; }
  struct Pre { double x = 0.0; };
  __device__ Pre fetch(int i) const { return Pre{x[i]}; }
  __device__ void row(int i, double ay, const Pre& p) const { r[i] = fma(scale, p.x, -ay); }
  __device__ void finish(int, double*) const {}
};

__global__ __launch_bounds__(kBlock) void pre_a_zero_kernel(const int32_t* __restrict__ done, int32_t n,
                                                             double* __restrict__ y) {
  if (done && *done != 0) return;
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) y[i] = 0.0;
}

void pre_a_check(const PreA& p, const char* loop, int allows) {
  const std::string who = std::string(loop) + ": ";
  const int terms = int(p.amg != nullptr) + int(p.dist_amg != nullptr) + int(p.dist_aux != nullptr);
  const int parts = int(p.diag != nullptr) + int(p.bjac != nullptr) + terms;
  if (p.fdm) {
    NSS_REQUIRE(parts == 0 && !p.sweep_A,
                who + "pre_fdm (the inverse by fast diagonalisation) is exclusive with pre_diag, pre_bjac and every term");
    NSS_REQUIRE(fdmi_rows(*p.fdm) == p.n && p.ncols == p.n, who + "fast-diagonalisation size mismatch");
    return;
  }
  if (allows & kPreAOnePartAtMost) {
    NSS_REQUIRE(parts <= 1, who + "at most one preconditioner");
  } else {
    NSS_REQUIRE(!(p.diag && p.bjac), who + "pre_diag and pre_bjac are exclusive");
    NSS_REQUIRE(parts >= 1, who + "no preconditioner for the velocity block");
  }
  NSS_REQUIRE(terms <= 1, who + "the row-partitioned terms replace pre_amg and one another");
  NSS_REQUIRE((allows & kPreASlabTerms) || !(p.dist_amg || p.dist_aux), who + "takes no row-partitioned term");
  NSS_REQUIRE(!p.amg || (!p.amg->levels.empty() && p.amg->levels[0].n == p.n), who + "AMG size mismatch");
  NSS_REQUIRE((!p.dist_amg || p.dist_amg->n == p.n) && (!p.dist_aux || p.dist_aux->n_u == p.n),
              who + "row-partitioned term size mismatch");
  NSS_REQUIRE(!p.bjac || p.bjac->n == p.n, who + "block preconditioner size mismatch");
  NSS_REQUIRE((allows & kPreAMultiplicative) || !p.multiplicative(), who + "AMG + Gauss-Seidel mode is not additive");
  NSS_REQUIRE(!p.sweep_A || (p.multiplicative() && p.sweep_A->m == p.n && p.sweep_A->n == p.ncols),
              who + "sweep_A serves the multiplicative preconditioner only, with the rows and the operand layout of A");
  NSS_REQUIRE(!(p.dist_aux && p.multiplicative() && p.residual_A().val32),
              who + "the row-partitioned preconditioner takes fp64 matrix values (its residual too)");
}

// y (+)= term(bscale b)
static void term_apply(const PreA& p, double bscale, const double* b, double* y, bool accumulate, const int32_t* done,
                       hipStream_t st) {
  if (p.dist_aux) dist_aux_apply(*p.dist_aux, bscale, b, y, accumulate, st, done);
  else if (p.dist_amg) dist_amg_apply(*p.dist_amg, bscale, b, y, st, done);      // (additive only: multiplicative())
  else amg_apply(*p.amg, bscale, b, y, st, done, accumulate);
}

void pre_a_apply(const PreA& p, double scale, const double* x, double* y, double* scratch, const int32_t* done,
                 hipStream_t st) {
  if (p.fdm) {
    fdmi_apply(*p.fdm, scale, x, y, done, st);
  } else if (p.multiplicative()) {
    // MypreA with GS=True (:376-381): y = 0; J.Smooth(y, x); r = x - A y; y += M r; J.SmoothBack(y, x), applied to scale x.
    // On slabs the sweeps run inside the slab (additive across slabs); the residual is formed with the matrix of the
    // sweeps (fp32 storage: the handle's fp32 copy of it), which keeps the operator symmetric.
    NSS_REQUIRE(scratch != nullptr, "pre_a_apply: the multiplicative form needs a scratch vector");
    const nss_bjac_s& j = *p.bjac;
    if (j.gs_permuted) {
      bjac_smooth(j, scale, x, y, false, done, st, kGsFromZero);   // colour-major layout: starts from zeros of its own
    } else {
      hipLaunchKernelGGL(pre_a_zero_kernel, dim3(int((p.n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, done, int32_t(p.n), y);
      NSS_CHECK_LAUNCH();
      bjac_smooth(j, scale, x, y, false, done, st);
    }
    if (p.exchange_y) exchange_on(*p.dist_aux->d, p.dist_aux->ch_y, p.dist_aux->halo_y, done, st);
    launch_csr<kF32>(p.residual_A(), y, EpiScaledResidual{done, scale, x, scratch}, st);
    term_apply(p, 1.0, scratch, y, true, done, st);
    bjac_smooth(j, scale, x, y, true, done, st, j.gs_permuted ? kGsKeepX : 0);   // (x again)
  } else if (p.term()) {                             // additive MypreA (:383): term + Jacobi part
    term_apply(p, scale, x, y, false, done, st);
    if (p.bjac) bjac_apply(*p.bjac, scale, x, 1.0, y, done, st);
    if (p.diag) diag_apply(p.n, p.diag, scale, x, 1.0, y, done, st);
  } else if (p.bjac) {                               // block Jacobi, or the symmetric Gauss-Seidel sweep as an operator
    bjac_apply(*p.bjac, scale, x, 0.0, y, done, st);
  } else {
    NSS_REQUIRE(p.diag != nullptr, "pre_a_apply: no preconditioner");
    diag_apply(p.n, p.diag, scale, x, 0.0, y, done, st);
  }
}

}  // namespace nss
