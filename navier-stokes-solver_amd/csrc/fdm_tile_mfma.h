// The tile body of the fast-diagonalisation contractions on the fp64 matrix cores: fdm_tile.h's interface and staging
// (64 x 64 outputs per workgroup of 256 lanes, j in steps of 16 through LDS with the next step's tiles in flight in
// registers, guarded loads of zeros and guarded stores for ragged extents, nothing padded), the products by
// v_mfma_f64_16x16x4_f64 instead of scalar FMAs:
//
//   Y(q, i) = sum_j Mop[i][j] X(q, j),     Mop = M (transpose = 0) or M^T,     M row-major n x n
//
// One instruction computes D[m][c] += sum_{k<4} A[m][k] B[k][c] for a 16 x 16 block.  The f64 lane maps are NOT those of
// the f32 forms:
//
//   A, B   one f64 per lane l:  A[m = l & 15][k = l >> 4],  B[k = l >> 4][c = l & 15]
//   C, D   four f64 per lane:   column c = l & 15,  row m = (l >> 4) + 4 * reg      (the f32 forms: 4 * (l >> 4) + reg)
//
// The column of D goes with the lane, so it is given to the direction along which Y is contiguous: q for LINES = false
// (A = Mop, B = X^T: rows i, columns q), i for LINES = true (A = X, B = Mop^T: rows q, columns i).  Either way lane l
// reads row k0 + (l >> 4) of the two LDS tiles at columns (l & 15) + 16 * block.  Each of the four waves holds a 2 x 2
// arrangement of 16 x 16 accumulators (rows 32 (w >> 1) .., columns 32 (w & 1) ..): per four j a lane reads four
// doubles from LDS for four instructions -- 64 FMAs -- where fdm_tile.h reads eight doubles for sixteen FMAs.
//
// Rounding: a matrix instruction adds its four products to the accumulator as one operation, so a sum runs over j in
// groups of four, ascending.  The result is the same bits on every run and from every kernel that calls this body.  It
// is NOT promised to be the bits of fdm_tile.h, whose sums take one FMA per term: how the instruction orders and rounds
// its four additions is not documented for f64.  (Measured on the MI355X the two tiles agreed in every bit of every
// apply, as a chain of four FMAs in ascending k would -- profiles/fdm_stokes.md; no caller relies on it.)  Both obey the
// dot-product bound of n terms.
#pragma once

#include "fdm_tile.h"

namespace nss {

typedef double fdm_acc4 __attribute__((ext_vector_type(4)));

constexpr int kFdmMfmaK = 4;          // j per matrix instruction
constexpr int kFdmMfmaBlk = 16;       // rows and columns of one accumulator
constexpr int kFdmMfmaPer = 2;        // accumulators per wave and direction (2 x 2)

template <bool LINES, class QOffX, class QOffY, class Epilogue>
__device__ __forceinline__ void fdm_tile_mfma(int32_t n, int32_t nq, int32_t q0, int32_t i0, const double* __restrict__ M,
                                              int32_t transpose, const double* __restrict__ X, double* __restrict__ Y,
                                              int64_t sjx, int64_t sjy, QOffX qx, QOffY qy, Epilogue epi) {
  __shared__ double Ms[kFdmStep][kFdmRow];                 // Ms[k][ii] = Mop[i0 + ii][j0 + k]
  __shared__ double Xs[kFdmStep][kFdmRow];                 // Xs[k][qq] = X(q0 + qq, j0 + k)
  const int tid = threadIdx.x;

  // the loads of the two tiles: as fdm_tile.h
  const int k_j = tid & (kFdmStep - 1), r_j = tid >> 4;
  const int r_o = tid & (kFdmTile - 1), k_o = tid >> 6;
  double mreg[kFdmLoads], xreg[kFdmLoads];
  int64_t xoff[kFdmLoads];                                 // qx of the lines this lane loads from (not read past nq)
#pragma unroll
  for (int l = 0; l < kFdmLoads; ++l) xoff[l] = qx(q0 + (LINES ? r_j + 16 * l : r_o));

  auto fetch = [&](int32_t j0) {
#pragma unroll
    for (int l = 0; l < kFdmLoads; ++l) {
      {   // M: rows of M are contiguous along j without transpose, along i with it
        const int k = transpose ? k_o + 4 * l : k_j, ii = transpose ? r_o : r_j + 16 * l;
        const int32_t i = i0 + ii, j = j0 + k;
        const bool in = i < n && j < n;
        mreg[l] = in ? M[transpose ? int64_t(j) * n + i : int64_t(i) * n + j] : 0.0;
      }
      {   // X: contiguous along j for LINES, along q otherwise
        const int k = LINES ? k_j : k_o + 4 * l, qq = LINES ? r_j + 16 * l : r_o;
        const int32_t q = q0 + qq, j = j0 + k;
        const bool in = q < nq && j < n;
        xreg[l] = in ? X[xoff[l] + j * sjx] : 0.0;
      }
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int l = 0; l < kFdmLoads; ++l) {
      Ms[transpose ? k_o + 4 * l : k_j][transpose ? r_o : r_j + 16 * l] = mreg[l];
      Xs[LINES ? k_j : k_o + 4 * l][LINES ? r_j + 16 * l : r_o] = xreg[l];
    }
  };

  // rows of D: i (LINES: q); columns of D, with the lane: q (LINES: i)
  const int lane = tid & (kWave - 1), wave = tid >> 6;
  const int lk = lane >> 4, lc = lane & 15;
  const int row0 = 2 * kFdmMfmaBlk * (wave >> 1), col0 = 2 * kFdmMfmaBlk * (wave & 1);
  const double (*Rows)[kFdmRow] = LINES ? Xs : Ms;
  const double (*Cols)[kFdmRow] = LINES ? Ms : Xs;
  fdm_acc4 acc[kFdmMfmaPer][kFdmMfmaPer];                  // [row block][column block]
#pragma unroll
  for (int a = 0; a < kFdmMfmaPer; ++a)
#pragma unroll
    for (int b = 0; b < kFdmMfmaPer; ++b) acc[a][b] = fdm_acc4{0.0, 0.0, 0.0, 0.0};

  fetch(0);
  for (int32_t j0 = 0; j0 < n; j0 += kFdmStep) {
    __syncthreads();                                       // the previous step's reads of LDS are done
    stage();
    __syncthreads();
    if (j0 + kFdmStep < n) fetch(j0 + kFdmStep);
#pragma unroll
    for (int k0 = 0; k0 < kFdmStep; k0 += kFdmMfmaK) {
      double ra[kFdmMfmaPer], cb[kFdmMfmaPer];
#pragma unroll
      for (int t = 0; t < kFdmMfmaPer; ++t) {
        ra[t] = Rows[k0 + lk][row0 + kFdmMfmaBlk * t + lc];    // A[m = lc][k = lk]
        cb[t] = Cols[k0 + lk][col0 + kFdmMfmaBlk * t + lc];    // B[k = lk][c = lc]
      }
#pragma unroll
      for (int a = 0; a < kFdmMfmaPer; ++a)
#pragma unroll
        for (int b = 0; b < kFdmMfmaPer; ++b)
          acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(ra[a], cb[b], acc[a][b], 0, 0, 0);
    }
  }

  // D: column lc, row lk + 4 * reg of every accumulator
#pragma unroll
  for (int a = 0; a < kFdmMfmaPer; ++a)
#pragma unroll
    for (int b = 0; b < kFdmMfmaPer; ++b) {
      const int c = col0 + kFdmMfmaBlk * b + lc;
      if (LINES) {
        const int32_t i = i0 + c;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int32_t q = q0 + row0 + kFdmMfmaBlk * a + lk + 4 * r;
          if (q < nq && i < n) Y[qy(q) + i * sjy] = epi(q, i, acc[a][b][r]);
        }
      } else {
        const int32_t q = q0 + c;
        if (q >= nq) continue;
        const int64_t yoff = qy(q);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int32_t i = i0 + row0 + kFdmMfmaBlk * a + lk + 4 * r;
          if (i < n) Y[yoff + i * sjy] = epi(q, i, acc[a][b][r]);
        }
      }
    }
}

}  // namespace nss
