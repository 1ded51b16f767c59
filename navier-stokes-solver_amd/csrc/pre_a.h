// The velocity preconditioner of the fused loops (the reference's MypreA and its parts), said once: what a loop state
// holds of it (PreA), which combinations a loop takes (pre_a_check) and the launches of one apply (pre_a_apply).
#pragma once

#include "amg.h"
#include "precond.h"

struct nss_dist_amg_s;
struct nss_dist_aux_s;
struct nss_fdmi_s;

namespace nss {

// A view of a loop state's preconditioner fields, built on the stack (pre_a_of); owns nothing.
struct PreA {
  int64_t n = 0;                              // velocity rows
  int64_t ncols = 0;                          // columns of A's operand (slabs: [owned | ghosts]; else n)
  const double* diag = nullptr;               // point Jacobi (inverse diagonal)              -- exclusive with bjac
  const nss_bjac_s* bjac = nullptr;           // block Jacobi, or -- gs_mat -- the multicolour Gauss-Seidel sweeps
  const nss_amg_s* amg = nullptr;             // the term: V-cycle / auxiliary-space cycle ...
  const nss_csr_s* A = nullptr;               // the loop's matrix
  const nss_csr_s* sweep_A = nullptr;         // the sweeps' matrix where it is not A: x - A y between them is formed with it
  const nss_dist_amg_s* dist_amg = nullptr;   // ... or the V-cycle on slabs ...
  const nss_dist_aux_s* dist_aux = nullptr;   // ... or the auxiliary-space cycle on slabs (at most one of the three)
  bool exchange_y = false;                    // slabs: the residual reads ghosts of the iterate (dist_aux's halo_y)
  const nss_fdmi_s* fdm = nullptr;            // the exact inverse by fast diagonalisation -- exclusive with everything above
  bool term() const { return amg || dist_amg || dist_aux; }
  // Gauss-Seidel sweeps around the term (GS=True, :376-381) instead of term + Jacobi part (:383)
  bool multiplicative() const { return (amg || dist_aux) && bjac && bjac->gs_mat; }
  const nss_csr_s& residual_A() const { return sweep_A ? *sweep_A : *A; }
};

// the view of a loop state that names its fields pre_diag, pre_bjac, pre_amg and A, with `n` velocity rows (cg, minres,
// bpcg1; lanczos adds its sweep_A; bpcg2 lists its slab fields itself)
// (`fdm` is set by the loops whose state has pre_fdm; the stand-alone CG loop has none: an exact inverse of its own
// operator is no preconditioner to iterate with)
template <class State>
PreA pre_a_of(const State& s, int64_t n) {
  return PreA{.n = n, .ncols = n, .diag = s.pre_diag, .bjac = s.pre_bjac, .amg = s.pre_amg, .A = s.A};
}

// throws "<loop>: ..." for a combination the loop does not take; `allows`: what it takes beyond the additive form
// k (term + Jacobi part) and its parts alone
enum { kPreAAdditiveOnly = 0, kPreAMultiplicative = 1, kPreASlabTerms = 2, kPreAOnePartAtMost = 4 };
void pre_a_check(const PreA& p, const char* loop, int allows);

// y = scale * preA x; every launch returns at once when `done` (device int, may be NULL) is non-zero.
//   multiplicative:  y = 0; J.Smooth(y, scale x); scratch = scale x - A y; y += term(scratch); J.SmoothBack(y, scale x)
//   term, additive:  y = term(scale x) [+ scale J x] [+ scale dinv x]        (`scratch`, n doubles, may be NULL)
//   fdm:             y = scale A^-1 x (the scale in the epilogue of the last forward pass; x != y)
//   else:            y = scale J x  |  y = scale dinv x
void pre_a_apply(const PreA& p, double scale, const double* x, double* y, double* scratch, const int32_t* done,
                 hipStream_t st);

}  // namespace nss
