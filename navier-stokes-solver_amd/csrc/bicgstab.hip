// Fused, device-resident BiCGStab for nonsymmetric operators (nss_bicgstab_*): the Krylov loop of the linearly implicit
// (Picard-linearised) convection step, `NavierStokes.SetConvectionTreatment("implicit")`, and of `hipla.BiCGStabSolver`.
// Right-preconditioned, from x = 0, with rhat = r0 = b, p = r0, rho = <rhat, r0>.  One iteration:
//
//   [F]  flux points   : F = a avg(phat) - |a| diff(phat) / 2 behind phat          (form (ii) only; linear_donor_flux)
//   K1   rows of Op    : v = Op phat, partials <rhat, v>                                                       (EpiBiV)
//   S1   one workgroup : alpha = rho / <rhat, v>;  breakdown -> code 1                               (bicg_alpha_kernel)
//   K2   element-wise  : s = r - alpha v (in the place of r);  shat = P s                               (bicg_s_kernel)
//   [F]  flux points   : the same on shat                                                                 (form (ii))
//   K3   rows of Op    : t = Op shat, partials <t, s> and <t, t>                                               (EpiBiT)
//   S2   one workgroup : omega = <t, s> / <t, t>  (<t, t> == 0: omega = 0)                           (bicg_omega_kernel)
//   K4   element-wise  : x += alpha phat + omega shat;  r = s - omega t;  partials <rhat, r> and <r, r>  (bicg_x_kernel)
//   S3   one workgroup : hist[it] = |r|, stop test, breakdowns, beta = (rho'/rho)(alpha/omega), rho = rho'
//                                                                                                     (bicg_beta_kernel)
//   K5   element-wise  : p = r + beta (p - omega v);  phat = P p                                        (bicg_p_kernel)
//
// 8 launches per iteration in form (i), 10 in form (ii); P = identity or the point-Jacobi diagonal rides in K2 and K5,
// P = the direct viscous inverse (nss_fdmc_t) adds its 2 dim launches in front of each of the two applies instead.
// Op, form (i): a square CSR matrix.  Form (ii): y = m v + sigma [L | Dv] [v | F(a; v)], the operator of a time step read
// from the stepper's own [A | D] (or [K | B]) with sigma by value.
// The scalars never leave the device; every sum is per-workgroup partials added by the fixed tree fixed_sums_1024
// (nss_common.h), two sums per launch; no atomics: the same bits every run.  Every launch that writes loop state returns
// before its first load once ctrl[done] is set, the passes of an nss_fdmc_t included (fdmc_solve takes the word).
#include <cmath>

#include "bpcg2.h"

namespace nss {

enum { B_RHO = 0, B_RV = 1, B_ALPHA = 2, B_TS = 3, B_TT = 4, B_OMEGA = 5, B_RHON = 6, B_RR = 7, B_BETA = 8, B_ERR0 = 9,
       B_TOL = 10 };
enum { BC_DONE = 0, BC_ITFINAL = 1, BC_LAST = 2, BC_CODE = 3 };

// the row value of both forms: (i) the row sum itself; (ii) m_r x_r + sigma (row sum)
struct BiShift {
  const double* __restrict__ mass;
  double m0, sigma;
  int form2;
  __device__ double m(int r) const { return form2 ? (mass ? mass[r] : m0) : 0.0; }
  __device__ double value(double ax, double m_r, double x_r) const { return form2 ? fma(sigma, ax, m_r * x_r) : ax; }
};

// K1: v = Op phat, partials <rhat, v>
struct EpiBiV {
  const int32_t* __restrict__ ctrl;
  const double* __restrict__ phat;
  const double* __restrict__ rhat;
  BiShift op;
  double* __restrict__ v;
  double* __restrict__ partials;
  double acc = 0.0;
  __device__ bool skip() const { return ctrl[BC_DONE] != 0; }
  struct Pre { double x = 0.0, m = 0.0, rh = 0.0; };
  __device__ Pre fetch(int r) const { return Pre{op.form2 ? phat[r] : 0.0, op.m(r), rhat[r]}; }
  __device__ void row(int r, double ax, const Pre& pre) {
    const double val = op.value(ax, pre.m, pre.x);
    v[r] = val;
    acc = fma(pre.rh, val, acc);
  }
  __device__ void finish(int b, double* lds) {             // (no partials: the apply alone, nss_bicgstab_apply_f64)
    if (partials != nullptr) store_block_partial(acc, b, partials, lds);
  }
};

// K3: t = Op shat, partials <t, s> (partials[b]) and <t, t> (partials[nblk + b])
struct EpiBiT {
  const int32_t* __restrict__ ctrl;
  const double* __restrict__ shat;
  const double* __restrict__ s;
  BiShift op;
  double* __restrict__ t;
  double* __restrict__ partials;
  int32_t nblk;
  double ts = 0.0, tt = 0.0;
  __device__ bool skip() const { return ctrl[BC_DONE] != 0; }
  struct Pre { double x = 0.0, m = 0.0, s = 0.0; };
  __device__ Pre fetch(int r) const { return Pre{op.form2 ? shat[r] : 0.0, op.m(r), s[r]}; }
  __device__ void row(int r, double ax, const Pre& pre) {
    const double val = op.value(ax, pre.m, pre.x);
    t[r] = val;
    ts = fma(val, pre.s, ts);
    tt = fma(val, val, tt);
  }
  __device__ void finish(int b, double* lds) {
    store_block_partial(ts, b, partials, lds);
    store_block_partial(tt, b, partials + nblk, lds);
  }
};

struct BiArgs {
  int32_t* ctrl;
  double* scal;
  double* hist;
  int32_t n, it;
  double *x, *r, *p, *phat, *shat;
  const double *rhat, *v, *t, *dinv;
  double* partials;          // 2 * grid entries: K4's <rhat, r> in front of <r, r>
  int fused_pre;             // P is the identity or dinv: it rides in K2, K5 and the start
};

__device__ __forceinline__ double bi_pre(const BiArgs& a, int i, double val) { return a.dinv ? a.dinv[i] * val : val; }

// S1: alpha = rho / <rhat, v>.  <rhat, v> zero or not finite, or an alpha that is not finite: code 1 -- nothing of this
// iteration has touched x yet, which stays at its last iterate
__global__ __launch_bounds__(kBlock) void bicg_alpha_kernel(int32_t* __restrict__ ctrl, int it, int n,
                                                             const double* __restrict__ part, double* __restrict__ scal) {
  __shared__ double lds[kRedDoubles];
  if (ctrl[BC_DONE] != 0) return;
  const SumPair s = fixed_sums_1024(part, n, part, 0, lds);
  if (threadIdx.x == 0) {
    const double rv = s.a, alpha = scal[B_RHO] / rv;
    scal[B_RV] = rv;
    scal[B_ALPHA] = alpha;
    if (rv == 0.0 || !isfinite(rv) || !isfinite(alpha)) {
      ctrl[BC_CODE] = 1;
      ctrl[BC_ITFINAL] = it - 1;
      ctrl[BC_DONE] = 1;
    }
  }
}

// K2: s = r - alpha v, written over r;  shat = P s
__global__ __launch_bounds__(kBlock) void bicg_s_kernel(BiArgs a) {
  if (a.ctrl[BC_DONE] != 0) return;
  const double alpha = a.scal[B_ALPHA];
  const int stride = gridDim.x * kBlock;
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < a.n; i += stride) {
    const double s = fma(-alpha, a.v[i], a.r[i]);
    a.r[i] = s;
    if (a.fused_pre) a.shat[i] = bi_pre(a, i, s);
  }
}

// S2: omega = <t, s> / <t, t>; <t, t> == 0 gives omega = 0 (S3 decides whether that is convergence).  An omega that is
// not finite: code 1, before x is touched
__global__ __launch_bounds__(kBlock) void bicg_omega_kernel(int32_t* __restrict__ ctrl, int it, int n,
                                                             const double* __restrict__ part, double* __restrict__ scal) {
  __shared__ double lds[kRedDoubles];
  if (ctrl[BC_DONE] != 0) return;
  const SumPair s = fixed_sums_1024(part, n, part + n, n, lds);
  if (threadIdx.x == 0) {
    const double omega = s.b == 0.0 ? 0.0 : s.a / s.b;
    scal[B_TS] = s.a;
    scal[B_TT] = s.b;
    scal[B_OMEGA] = omega;
    if (!isfinite(omega)) {
      ctrl[BC_CODE] = 1;
      ctrl[BC_ITFINAL] = it - 1;
      ctrl[BC_DONE] = 1;
    }
  }
}

// K4: x += alpha phat + omega shat;  r = s - omega t;  partials <rhat, r> and <r, r>
__global__ __launch_bounds__(kBlock) void bicg_x_kernel(BiArgs a) {
  __shared__ double lds[kBlock / kWave];
  if (a.ctrl[BC_DONE] != 0) return;
  const double alpha = a.scal[B_ALPHA], omega = a.scal[B_OMEGA];
  const int stride = gridDim.x * kBlock;
  double rhr = 0.0, rr = 0.0;
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < a.n; i += stride) {
    a.x[i] = fma(omega, a.shat[i], fma(alpha, a.phat[i], a.x[i]));
    const double rn = fma(-omega, a.t[i], a.r[i]);
    a.r[i] = rn;
    rhr = fma(a.rhat[i], rn, rhr);
    rr = fma(rn, rn, rr);
  }
  store_block_partial(rhr, blockIdx.x, a.partials, lds);
  store_block_partial(rr, blockIdx.x, a.partials + gridDim.x, lds);
}

// S3: the books of iteration `it`: history, stop test, the breakdowns, beta and the new rho
__global__ __launch_bounds__(kBlock) void bicg_beta_kernel(int32_t* __restrict__ ctrl, int it, int n,
                                                            const double* __restrict__ part, double* __restrict__ scal,
                                                            double* __restrict__ hist) {
  __shared__ double lds[kRedDoubles];
  if (ctrl[BC_DONE] != 0) return;
  const SumPair s = fixed_sums_1024(part, n, part + n, n, lds);
  if (threadIdx.x == 0) {
    const double rhon = s.a, rr = s.b, err = sqrt(rr), omega = scal[B_OMEGA];
    scal[B_RHON] = rhon;
    scal[B_RR] = rr;
    hist[it] = err;
    ctrl[BC_LAST] = it;
    int code = -1;                                           // -1: the loop goes on
    if (err < scal[B_TOL] * scal[B_ERR0]) code = 0;
    else if (!isfinite(rr)) code = 1;
    else if (omega == 0.0) code = 2;
    else if (rhon == 0.0 || !isfinite(rhon)) code = 1;
    if (code >= 0) {
      ctrl[BC_CODE] = code;
      ctrl[BC_ITFINAL] = it;
      ctrl[BC_DONE] = 1;
    } else {
      scal[B_BETA] = (rhon / scal[B_RHO]) * (scal[B_ALPHA] / omega);
      scal[B_RHO] = rhon;
    }
  }
}

// K5: p = r + beta (p - omega v);  phat = P p
__global__ __launch_bounds__(kBlock) void bicg_p_kernel(BiArgs a) {
  if (a.ctrl[BC_DONE] != 0) return;
  const double beta = a.scal[B_BETA], omega = a.scal[B_OMEGA];
  const int stride = gridDim.x * kBlock;
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < a.n; i += stride) {
    const double pn = fma(beta, fma(-omega, a.v[i], a.p[i]), a.r[i]);
    a.p[i] = pn;
    if (a.fused_pre) a.phat[i] = bi_pre(a, i, pn);
  }
}

// the start from x = 0: x = 0, r = rhat = p = b, phat = P b, partials <b, b>
__global__ __launch_bounds__(kBlock) void bicg_start_kernel(BiArgs a, double* __restrict__ rhat,
                                                             const double* __restrict__ b) {
  __shared__ double lds[kBlock / kWave];
  const int stride = gridDim.x * kBlock;
  double acc = 0.0;
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < a.n; i += stride) {
    const double bi = b[i];
    a.x[i] = 0.0;
    a.r[i] = bi;
    rhat[i] = bi;
    a.p[i] = bi;
    if (a.fused_pre) a.phat[i] = bi_pre(a, i, bi);
    acc = fma(bi, bi, acc);
  }
  store_block_partial(acc, blockIdx.x, a.partials, lds);
}

// rho = <b, b>, err0 = |b|, tol and a cleared control word; a zero right-hand side ends the solve before its first
// iteration (done, it_final = -1: no iterations)
__global__ __launch_bounds__(kBlock) void bicg_start_sum_kernel(int32_t* __restrict__ ctrl, int n,
                                                                 const double* __restrict__ part,
                                                                 double* __restrict__ scal, double tol) {
  __shared__ double lds[kRedDoubles];
  const SumPair s = fixed_sums_1024(part, n, part, 0, lds);
  if (threadIdx.x == 0) {
    for (int k = 0; k < 16; ++k) scal[k] = 0.0;
    scal[B_RHO] = s.a;
    scal[B_ERR0] = sqrt(s.a);
    scal[B_TOL] = tol;
    ctrl[BC_DONE] = (s.a == 0.0 || !isfinite(s.a)) ? 1 : 0;
    ctrl[BC_ITFINAL] = -1;
    ctrl[BC_LAST] = -1;
    ctrl[BC_CODE] = isfinite(s.a) ? 0 : 1;
  }
}

// dinv_i = 1 / (m_i + sigma (L_ii + sum_p Dv[i, p] (a_p Avg[p, i] - |a_p| Diff[p, i] / 2))): the point-Jacobi diagonal of
// form (ii), one lane per row of [L | Dv] over its CSR row and the two-slot rows of avg and diff
__global__ __launch_bounds__(kBlock) void bicg_jacobi_kernel(int32_t n, const int32_t* __restrict__ rowptr,
                                                              const int32_t* __restrict__ col,
                                                              const double* __restrict__ val,
                                                              const int32_t* __restrict__ avg_col,
                                                              const double* __restrict__ avg_val,
                                                              const int32_t* __restrict__ diff_col,
                                                              const double* __restrict__ diff_val,
                                                              const double* __restrict__ adv,
                                                              const double* __restrict__ mass, double m0, double sigma,
                                                              double* __restrict__ dinv) {
  const int stride = gridDim.x * kBlock;
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    double d = 0.0;
    for (int32_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
      const int32_t c = col[e];
      if (c == i) {
        d += val[e];
      } else if (c >= n) {
        const int32_t p = c - n;
        double avg = 0.0, dif = 0.0;
        for (int k = 0; k < 2; ++k) {
          if (avg_col[2 * p + k] == i) avg += avg_val[2 * p + k];
          if (diff_col[2 * p + k] == i) dif += diff_val[2 * p + k];
        }
        d = fma(val[e], donor_flux(adv[p], avg, dif), d);
      }
    }
    dinv[i] = 1.0 / fma(sigma, d, mass ? mass[i] : m0);
  }
}

static bool bicg_form2(const nss_bicgstab_t& s) { return s.avg != nullptr; }
static int bicg_grid(const nss_bicgstab_t& s) { return stream_grid(s.n, kBlock * 4); }
static BiShift bicg_shift(const nss_bicgstab_t& s) {
  return BiShift{s.shift_mass, s.shift_m0, s.shift_sigma, bicg_form2(s) ? 1 : 0};
}

static void bicg_check(const nss_bicgstab_t* s) {
  NSS_REQUIRE(s != nullptr && s->A != nullptr, "bicgstab: NULL state / matrix");
  NSS_REQUIRE(s->n >= 1 && s->A->m == s->n, "bicgstab: matrix does not match n");
  NSS_REQUIRE((s->avg == nullptr) == (s->diff == nullptr), "bicgstab: avg and diff go together");
  if (bicg_form2(*s)) {
    NSS_REQUIRE(s->nflux >= 0 && s->A->n == s->n + s->nflux, "bicgstab: [L | Dv] has n + nflux columns");
    NSS_REQUIRE(s->avg->m == s->nflux && s->diff->m == s->nflux && s->avg->n == s->n && s->diff->n == s->n,
                "bicgstab: avg and diff are nflux x n");
    NSS_REQUIRE(s->nflux == 0 || s->adv != nullptr, "bicgstab: NULL advecting vector");
    NSS_REQUIRE(std::isfinite(s->shift_sigma) && s->shift_sigma >= 0.0, "bicgstab: sigma is negative or not finite");
  } else {
    NSS_REQUIRE(s->A->n == s->n && s->nflux == 0, "bicgstab: the matrix is not square");
    NSS_REQUIRE(s->pre_fdm == nullptr, "bicgstab: the direct viscous inverse goes with form (ii)");
  }
  NSS_REQUIRE(!(s->pre_diag && s->pre_fdm), "bicgstab: pre_diag and pre_fdm exclude each other");
  NSS_REQUIRE(s->pre_fdm == nullptr || fdmc_rows(*s->pre_fdm) == s->n, "bicgstab: pre_fdm was made for another size");
  NSS_REQUIRE(s->x && s->r && s->rhat && s->p && s->v && s->t && s->phat && s->shat && s->scal && s->ctrl && s->hist &&
                  s->partials_a && s->partials_b,
              "bicgstab: NULL buffer");
  const int64_t need[2] = {2 * int64_t(s->A->nblk), 2 * int64_t(bicg_grid(*s))};     // (= nss_bicgstab_workspace)
  const int64_t cap[2] = {s->cap_a, s->cap_b};
  check_plan("bicgstab", plan_stamp({s->A}), s->plan_gen, need, cap, 2);
}

static BiArgs bicg_args(const nss_bicgstab_t& s, int it) {
  return BiArgs{s.ctrl, s.scal, s.hist, s.n, it, s.x, s.r, s.p, s.phat, s.shat, s.rhat, s.v, s.t, s.pre_diag,
                s.partials_b, s.pre_fdm ? 0 : 1};
}

// out = P src for the preconditioner that is launches of its own, then -- form (ii) -- the flux tail behind `out`
static void bicg_operand(const nss_bicgstab_t& s, const double* src, double* out, hipStream_t st) {
  if (s.pre_fdm) fdmc_solve(*s.pre_fdm, s.shift_sigma, src, out, s.ctrl + BC_DONE, st);
  if (bicg_form2(s) && s.nflux > 0) linear_donor_flux(*s.avg, *s.diff, s.adv, out, out + s.n, s.ctrl + BC_DONE, st);
}

static void bicg_iteration(const nss_bicgstab_t& s, int it, hipStream_t st) {
  const dim3 one(1), block(kBlock), grid(bicg_grid(s));
  const BiArgs a = bicg_args(s, it);
  const BiShift op = bicg_shift(s);
  bicg_operand(s, s.p, s.phat, st);
  launch_csr<kF32 | kCodes>(*s.A, s.phat, EpiBiV{s.ctrl, s.phat, s.rhat, op, s.v, s.partials_a}, st);
  hipLaunchKernelGGL(bicg_alpha_kernel, one, block, 0, st, s.ctrl, it, s.A->nblk, s.partials_a, s.scal);
  NSS_CHECK_LAUNCH();
  hipLaunchKernelGGL(bicg_s_kernel, grid, block, 0, st, a);
  NSS_CHECK_LAUNCH();
  bicg_operand(s, s.r, s.shat, st);
  launch_csr<kF32 | kCodes>(*s.A, s.shat, EpiBiT{s.ctrl, s.shat, s.r, op, s.t, s.partials_a, s.A->nblk}, st);
  hipLaunchKernelGGL(bicg_omega_kernel, one, block, 0, st, s.ctrl, it, s.A->nblk, s.partials_a, s.scal);
  NSS_CHECK_LAUNCH();
  hipLaunchKernelGGL(bicg_x_kernel, grid, block, 0, st, a);
  NSS_CHECK_LAUNCH();
  hipLaunchKernelGGL(bicg_beta_kernel, one, block, 0, st, s.ctrl, it, int(grid.x), s.partials_b, s.scal, s.hist);
  NSS_CHECK_LAUNCH();
  hipLaunchKernelGGL(bicg_p_kernel, grid, block, 0, st, a);
  NSS_CHECK_LAUNCH();
}

}  // namespace nss

using namespace nss;

extern "C" {

int nss_bicgstab_workspace(const nss_bicgstab_t* s, int64_t* partials_a, int64_t* partials_b) {
  return guarded([&] {
    NSS_REQUIRE(s && s->A, "bicgstab_workspace: NULL state / matrix");
    if (partials_a) *partials_a = 2 * int64_t(s->A->nblk);
    if (partials_b) *partials_b = 2 * int64_t(bicg_grid(*s));
  });
}

int nss_bicgstab_start(const nss_bicgstab_t* s, const double* b, double tol, nss_stream_t stream) {
  return guarded([&] {
    bicg_check(s);
    NSS_REQUIRE(b != nullptr && b != s->x && b != s->r && b != s->rhat && b != s->p && b != s->phat,
                "bicgstab_start: NULL right-hand side, or it aliases a buffer of the state");
    hipStream_t st = as_stream(stream);
    const int nb = bicg_grid(*s);
    hipLaunchKernelGGL(bicg_start_kernel, dim3(nb), dim3(kBlock), 0, st, bicg_args(*s, 0), s->rhat, b);
    NSS_CHECK_LAUNCH();
    hipLaunchKernelGGL(bicg_start_sum_kernel, dim3(1), dim3(kBlock), 0, st, s->ctrl, nb, s->partials_b, s->scal, tol);
    NSS_CHECK_LAUNCH();
  });
}

int nss_bicgstab_iterate(const nss_bicgstab_t* s, int32_t it_begin, int32_t it_end, nss_stream_t stream) {
  return guarded([&] {
    bicg_check(s);
    if (bicg_form2(*s) && s->nflux > 0) {                   // (set-up on the first call: the two-slot copies)
      require_f64_values(s->avg, "bicgstab");
      require_f64_values(s->diff, "bicgstab");
      NSS_REQUIRE(fixed_width_copy(*s->avg) && fixed_width_copy(*s->diff),
                  "bicgstab: a row of avg or diff has more than two entries");
    }
    for (int it = it_begin; it < it_end; ++it) bicg_iteration(*s, it, as_stream(stream));
  });
}

int nss_bicgstab_poll(const nss_bicgstab_t* s, int32_t* done, int32_t* it_final, int32_t* last_it, int32_t* code,
                      nss_stream_t stream) {
  return guarded([&] {
    NSS_REQUIRE(s && s->ctrl, "bicgstab_poll: NULL state");
    int32_t h[4] = {0, 0, 0, 0};
    poll_ctrl(s->ctrl, as_stream(stream), h);
    if (done) *done = h[BC_DONE];
    if (it_final) *it_final = h[BC_ITFINAL];
    if (last_it) *last_it = h[BC_LAST];
    if (code) *code = h[BC_CODE];
  });
}

int nss_bicgstab_apply_f64(const nss_bicgstab_t* s, double* operand, double* y, nss_stream_t stream) {
  return guarded([&] {
    NSS_REQUIRE(s && s->A && operand && y && operand != y, "bicgstab_apply: NULL argument, or y aliases the operand");
    NSS_REQUIRE(s->A->m == s->n && s->ctrl, "bicgstab_apply: matrix does not match n, or no control words");
    NSS_REQUIRE((s->avg == nullptr) == (s->diff == nullptr), "bicgstab_apply: avg and diff go together");
    hipStream_t st = as_stream(stream);
    if (bicg_form2(*s)) {
      NSS_REQUIRE(s->A->n == s->n + s->nflux && s->avg->m == s->nflux && s->diff->m == s->nflux && s->avg->n == s->n &&
                      s->diff->n == s->n && (s->nflux == 0 || s->adv),
                  "bicgstab_apply: the shapes of form (ii) do not fit");
      if (s->nflux > 0) {
        require_f64_values(s->avg, "bicgstab_apply");
        require_f64_values(s->diff, "bicgstab_apply");
        NSS_REQUIRE(fixed_width_copy(*s->avg) && fixed_width_copy(*s->diff),
                    "bicgstab_apply: a row of avg or diff has more than two entries");
        linear_donor_flux(*s->avg, *s->diff, s->adv, operand, operand + s->n, s->ctrl + BC_DONE, st);
      }
    } else {
      NSS_REQUIRE(s->A->n == s->n, "bicgstab_apply: the matrix is not square");
    }
    launch_csr<kF32 | kCodes>(*s->A, operand, EpiBiV{s->ctrl, operand, operand, bicg_shift(*s), y, nullptr}, st);
  });
}

int nss_bicgstab_jacobi_f64(const nss_bicgstab_t* s, double* dinv, nss_stream_t stream) {
  return guarded([&] {
    NSS_REQUIRE(s && s->A && dinv, "bicgstab_jacobi: NULL argument");
    NSS_REQUIRE(bicg_form2(*s) && s->diff, "bicgstab_jacobi: the state is not of form (ii)");
    NSS_REQUIRE(s->A->m == s->n && s->A->n == s->n + s->nflux && s->avg->m == s->nflux && s->diff->m == s->nflux &&
                    s->avg->n == s->n && s->diff->n == s->n && (s->nflux == 0 || s->adv),
                "bicgstab_jacobi: the shapes of form (ii) do not fit");
    require_f64_values(s->A, "bicgstab_jacobi");
    const int32_t *ac = nullptr, *dc = nullptr;
    const double *av = nullptr, *dv = nullptr;
    if (s->nflux > 0) {
      require_f64_values(s->avg, "bicgstab_jacobi");
      require_f64_values(s->diff, "bicgstab_jacobi");
      NSS_REQUIRE(fixed_width_copy(*s->avg) && fixed_width_copy(*s->diff),
                  "bicgstab_jacobi: a row of avg or diff has more than two entries");
      ac = s->avg->fw_col, av = s->avg->fw_val, dc = s->diff->fw_col, dv = s->diff->fw_val;
    }
    hipLaunchKernelGGL(bicg_jacobi_kernel, dim3(stream_grid(s->n, kBlock)), dim3(kBlock), 0, as_stream(stream), s->n,
                       s->A->rowptr.get(), s->A->col.get(), s->A->val.get(), ac, av, dc, dv, s->adv, s->shift_mass,
                       s->shift_m0, s->shift_sigma, dinv);
    NSS_CHECK_LAUNCH();
  });
}

}  // extern "C"
