// The tile body of the fast-diagonalisation contractions, shared by the contiguous kernel of fdm.hip and the pitched,
// component-batched kernel of fdm_components.hip (the way bjac_block.h shares the block-Jacobi product):
//
//   Y(q, i) = sum_j Mop[i][j] X(q, j),     Mop = M (transpose = 0) or M^T,     M row-major n x n
//
// for one 64 x 64 tile of outputs (q0 .. q0 + 63, i0 .. i0 + 63).  A workgroup of 256 lanes walks j in steps of 16 with
// the M tile and the X tile in LDS (the next step's tiles are in flight, in registers, while this step's are
// multiplied), and every lane keeps a 4 x 4 register tile.  Every sum runs over j ascending, one FMA per term, whatever
// the tiling: the same bits every run, and the same bits from every kernel that calls this body.  Extents that are no
// multiple of the tile are handled by guarded loads of zeros and guarded stores; nothing is padded.
//
// Where the operands live is the caller's: element (q, j) of X is X[qx(q) + j * sjx], element (q, i) of Y is
// Y[qy(q) + i * sjy]; `qx` / `qy` are evaluated once per lane and q, outside the loop over j, so they may divide.
// The value stored is epi(q, i, sum): the identity, or a diagonal scaling that rides on the pass.  Two instantiations:
//
//   LINES = false  q is the direction along which X and Y are contiguous (the caller's qx(q + 1) = qx(q) + 1): loads of
//                  X and stores of Y run along q.  Correct for any nq, coalesced in full from nq >= 64.
//   LINES = true   j and i are the contiguous direction (sjx = sjy = 1, the grid's x axis): loads of X run along j,
//                  stores of Y along i.
#pragma once

#include "nss_common.h"

namespace nss {

constexpr int kFdmTile = 64;      // outputs per workgroup and direction
constexpr int kFdmStep = 16;      // j per K-step
constexpr int kFdmReg = 4;        // register tile per lane and direction: kFdmTile / 16
constexpr int kFdmLoads = kFdmTile * kFdmStep / kBlock;      // elements of one LDS tile per lane: 4
constexpr int kFdmRow = kFdmTile + 1;                        // LDS row stride in doubles (odd: the transposing stores)

template <bool LINES, class QOffX, class QOffY, class Epilogue>
__device__ __forceinline__ void fdm_tile(int32_t n, int32_t nq, int32_t q0, int32_t i0, const double* __restrict__ M,
                                         int32_t transpose, const double* __restrict__ X, double* __restrict__ Y,
                                         int64_t sjx, int64_t sjy, QOffX qx, QOffY qy, Epilogue epi) {
  __shared__ double Ms[kFdmStep][kFdmRow];                 // Ms[k][ii] = Mop[i0 + ii][j0 + k]
  __shared__ double Xs[kFdmStep][kFdmRow];                 // Xs[k][qq] = X(q0 + qq, j0 + k)
  const int tid = threadIdx.x;

  // which elements of the two tiles this lane loads: l = 0 .. kFdmLoads - 1
  //   along j (16 per row of the tile): k = tid % 16, other = tid / 16 + 16 l
  //   along the other direction (64):   other = tid % 64, k = tid / 64 + 4 l
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

  // the register tile: the direction along which Y is contiguous (q, or i for LINES) goes with tid % 16
  const int tx = tid & 15, ty = tid >> 4;
  const int il = LINES ? tx : ty, ql = LINES ? ty : tx;
  double acc[kFdmReg][kFdmReg];                            // [i][q]
#pragma unroll
  for (int a = 0; a < kFdmReg; ++a)
#pragma unroll
    for (int b = 0; b < kFdmReg; ++b) acc[a][b] = 0.0;

  fetch(0);
  for (int32_t j0 = 0; j0 < n; j0 += kFdmStep) {
    __syncthreads();                                       // the previous step's reads of LDS are done
    stage();
    __syncthreads();
    if (j0 + kFdmStep < n) fetch(j0 + kFdmStep);
#pragma unroll
    for (int k = 0; k < kFdmStep; ++k) {
      double mi[kFdmReg], xq[kFdmReg];
#pragma unroll
      for (int t = 0; t < kFdmReg; ++t) {
        mi[t] = Ms[k][il + 16 * t];
        xq[t] = Xs[k][ql + 16 * t];
      }
#pragma unroll
      for (int a = 0; a < kFdmReg; ++a)
#pragma unroll
        for (int b = 0; b < kFdmReg; ++b) acc[a][b] = fma(mi[a], xq[b], acc[a][b]);
    }
  }

#pragma unroll
  for (int b = 0; b < kFdmReg; ++b) {
    const int32_t q = q0 + ql + 16 * b;
    if (q >= nq) continue;
    const int64_t yoff = qy(q);
#pragma unroll
    for (int a = 0; a < kFdmReg; ++a) {
      const int32_t i = i0 + il + 16 * a;
      if (i < n) Y[yoff + i * sjy] = epi(q, i, acc[a][b]);
    }
  }
}

}  // namespace nss
