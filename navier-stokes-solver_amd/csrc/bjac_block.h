// The product of one inverse block-Jacobi block with its slice of a vector, in pieces: every kernel that applies such a
// block -- the three stand-alone apply kernels and the Gauss-Seidel block solve (precond.hip), MINRES' M3, the fused
// Lanczos step, the epilogues of BPCG v1 / v2 -- is put together from these, so that all of them form the same
// products in the same order (same bits) by construction.
#pragma once

#include "csr_stream.h"

namespace nss {

// Run word (nss_bjac_s::run): a block that is a run of consecutive dofs, padding last, as first dof * 32 + length
// (length <= kMaxBs = 16 < 32; first dof < 2^26).
struct BjacRun { int32_t first, len; };
__host__ __device__ __forceinline__ int32_t bjac_pack_run(int32_t first, int32_t len) { return first * 32 + len; }
__host__ __device__ __forceinline__ BjacRun bjac_unpack_run(int32_t w) { return BjacRun{w >> 5, w & 31}; }

// dofs of block b: from its run word (run != NULL: one word per block) or the index table idx[c][b]; -1 = no dof
template <int BS>
__device__ __forceinline__ void bjac_block_dofs(const int32_t* run, const int32_t* idx,
                                                int32_t nb, int b, int32_t (&dof)[BS]) {
  if (run) {
    const BjacRun w = bjac_unpack_run(run[b]);
#pragma unroll
    for (int c = 0; c < BS; ++c) dof[c] = c < w.len ? w.first + c : -1;
  } else {
#pragma unroll
    for (int c = 0; c < BS; ++c) dof[c] = idx[size_t(c) * nb + b];
  }
}

// s = M x for a symmetric block stored as its upper triangle, row-major: m(t) yields stored entry t (from wherever
// the caller keeps it), read once and used for both triangles
template <int BS, class M>
__device__ __forceinline__ void bjac_sym_product(M m, const double (&x)[BS], double (&s)[BS]) {
#pragma unroll
  for (int c = 0; c < BS; ++c) s[c] = 0.0;
  int t = 0;
#pragma unroll
  for (int r = 0; r < BS; ++r) {
#pragma unroll
    for (int c = r; c < BS; ++c, ++t) {
      const double e = m(t);
      s[r] = fma(e, x[c], s[r]);
      if (c > r) s[c] = fma(e, x[r], s[c]);
    }
  }
}

// (M x)[r] for a block stored in full, row-major: m(t) yields entry t = r * BS + c
template <int BS, class M>
__device__ __forceinline__ double bjac_full_row(M m, int r, const double (&x)[BS]) {
  double s = 0.0;
#pragma unroll
  for (int c = 0; c < BS; ++c) s = fma(m(r * BS + c), x[c], s);
  return s;
}

// y[dof] = alpha * s + beta * y[dof] (a dof that exists); returns acc + y[dof] * x, the lane's partial of <y, x>
__device__ __forceinline__ double bjac_store(int32_t dof, double s, double x, double alpha, double beta, double* y,
                                             double acc) {
  if (dof >= 0) {
    double v = alpha * s;
    if (beta != 0.0) v = fma(beta, y[dof], v);
    y[dof] = v;
    acc = fma(v, x, acc);
  }
  return acc;
}

// The blocks of row block b of a matrix planned around the Jacobi blocks (nss_csr_plan_for_blocks: first_of, order),
// one lane per block, length known at run time only: out(dof, (J x)[dof]) for every dof of the block, x from the LDS
// copy of the row block's slice (slot = dof mod kBlockRows), the entries from the packed upper triangles of `bs` rows.
template <class Out>
__device__ __forceinline__ void bjac_rows_from_lds(const int32_t* first_of,
                                                   const int32_t* order,
                                                   const int32_t* run,
                                                   const double* packed, int32_t count, int32_t bs, int b,
                                                   const double* x_lds, Out out) {
  const int j1 = first_of[b + 1];
  for (int pos = first_of[b] + int(threadIdx.x); pos < j1; pos += kBlock) {
    const int jb = order[pos];
    const BjacRun w = bjac_unpack_run(run[jb]);
    for (int i = 0; i < w.len; ++i) {
      double s = 0.0;
      for (int j = 0; j < w.len; ++j) {
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        const int tri = lo * bs - (lo * (lo - 1)) / 2 + (hi - lo);             // upper triangle, row-major
        s = fma(packed[size_t(tri) * count + jb], x_lds[(w.first + j) & (kBlockRows - 1)], s);
      }
      out(w.first + i, s);
    }
  }
}

}  // namespace nss
