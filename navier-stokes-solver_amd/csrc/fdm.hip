// Fast diagonalisation of a Kronecker-sum operator (`hipla.FastDiagonalization`; the direct pressure projection of
// `NavierStokes.SetProjection("fdm")`).  With T_a = Q_a diag(lambda_a) Q_a^T per grid axis,
//
//   phi = (Q_0 (x) Q_1 (x) Q_2) [ 1 / (lambda_0[i] + lambda_1[j] + lambda_2[k]) ] (Q_0^T (x) Q_1^T (x) Q_2^T) rhs
//
// is 2 d contractions along one grid axis each:
//
//   Y[o, i, c] = sum_j M[i, j] X[o, j, c]   (transpose = 0)          X, Y: contiguous (outer, n, inner) fp64
//   Y[o, i, c] = sum_j M[j, i] X[o, j, c]   (transpose = 1)          M:    row-major n x n
//
// ONE kernel, a tiled GEMM on plain fp64 FMAs: a workgroup of 256 lanes owns a 64 x 64 tile of outputs, walks j in
// steps of 16 with the M tile and the X tile in LDS (the next step's tiles are in flight, in registers, while this
// step's are multiplied), and every lane keeps a 4 x 4 register tile.  Every sum runs over j ascending, one FMA per
// term, whatever the tiling: the same bits every run.  Extents that are no multiple of the tile are handled by guarded
// loads of zeros and guarded stores; nothing is padded.  Two instantiations:
//
//   LINES = false  the tile is (i, c) of one o; loads of X and stores of Y run along c.  Taken for every inner > 1:
//                  it is correct for any inner, and coalesced in full from inner >= 64.  For 1 < inner < 64 a row of the
//                  X tile is `inner` contiguous doubles and the lanes beyond it idle -- this instantiation is the one
//                  that is correct there, the other one needs inner == 1.
//   LINES = true   inner == 1 (the grid's x axis): the tile is (line o, i); loads of X run along j, stores of Y along i.
//
// The optional epilogue multiplies Y by 1 / (lambda_0[.] + lambda_1[.] + lambda_2[.]) of the cell's multi-index (0
// where |sum| <= null_threshold), computed from the d eigenvalue vectors: it rides on the last forward pass and costs
// neither a launch nor a pass over memory.
//
// Per pass over N = outer n inner cells: 16 N bytes (X read once per tile row of i, i.e. ceil(n / 64) times, the
// re-reads from L2; M from L2) and 2 n N flops.
#include <cmath>
#include <memory>

#include "fdm_tile.h"
#include "nss_common.h"

namespace nss {

// the diagonal scaling of the epilogue; dim == 0: none
struct FdmScale {
  const double* lam[3];
  int32_t ext[3];
  int32_t dim;
  double threshold;
};

// `p`: the cell's index in the grid, last axis fastest (below 2^31)
__device__ __forceinline__ double fdm_multiplier(const FdmScale& sc, uint32_t p) {
  double sum;                                              // (lambda_0 + lambda_1) + lambda_2: the host's order
  if (sc.dim == 3) {
    const uint32_t e1 = uint32_t(sc.ext[1]), e2 = uint32_t(sc.ext[2]);
    const uint32_t t = p / e2;
    sum = sc.lam[0][t / e1] + sc.lam[1][t % e1];
    sum += sc.lam[2][p % e2];
  } else {
    const uint32_t e1 = uint32_t(sc.ext[1]);
    sum = sc.lam[0][p / e1] + sc.lam[1][p % e1];
  }
  return fabs(sum) <= sc.threshold ? 0.0 : 1.0 / sum;
}

// Grid: one dimension, tiles of q fastest, then tiles of i, then o.  q is the tile direction that is not i: the cell
// index c (LINES = false, nq = inner, one o per workgroup) or the line index o (LINES = true, nq = outer).  The tile
// body is fdm_tile.h's.
template <bool LINES>
__global__ __launch_bounds__(kBlock) void fdm_contract_kernel(int32_t n, int32_t nq, int32_t tiles_q, int32_t tiles_i,
                                                               const double* __restrict__ M, int32_t transpose,
                                                               const double* __restrict__ X, double* __restrict__ Y,
                                                               FdmScale sc) {
  const int64_t blk = blockIdx.x;
  const int32_t q0 = int32_t(blk % tiles_q) * kFdmTile;
  const int32_t i0 = int32_t((blk / tiles_q) % tiles_i) * kFdmTile;
  const int64_t o = blk / (int64_t(tiles_q) * tiles_i);    // (0 for LINES)
  // element (q, j) of X and (q, i) of Y: base + q * sq + j * sj
  const int64_t base = LINES ? 0 : o * int64_t(n) * nq;
  const int64_t sq = LINES ? n : 1, sj = LINES ? 1 : nq;
  auto at = [=](int32_t q) { return base + q * sq; };
  fdm_tile<LINES>(n, nq, q0, i0, M, transpose, X, Y, sj, sj, at, at, [&](int32_t q, int32_t i, double v) {
    return sc.dim ? v * fdm_multiplier(sc, uint32_t(base + q * sq + i * sj)) : v;
  });
}

constexpr int64_t kFdmMaxCells = 2147483647;              // 2^31 - 1

// the cells of a shape, after the checks every entry point makes before it launches or allocates
static int64_t fdm_cells(const int64_t* ext, int count, const char* who) {
  int64_t cells = 1;
  for (int a = 0; a < count; ++a) {
    NSS_REQUIRE(ext[a] >= 1, std::string(who) + ": an extent below 1");
    NSS_REQUIRE(ext[a] <= kFdmMaxCells && cells * ext[a] <= kFdmMaxCells,
                std::string(who) + ": more than 2^31 - 1 cells");
    cells *= ext[a];
  }
  return cells;
}

// one pass; the shape has been checked
static void fdm_launch(int64_t outer, int64_t n, int64_t inner, const double* M, int transpose, const double* x,
                       double* y, const FdmScale& sc, hipStream_t st) {
  const bool lines = inner == 1;
  const int64_t nq = lines ? outer : inner;
  const int64_t tiles_q = (nq + kFdmTile - 1) / kFdmTile, tiles_i = (n + kFdmTile - 1) / kFdmTile;
  const int64_t blocks = tiles_q * tiles_i * (lines ? 1 : outer);        // <= the number of cells
  const dim3 grid(static_cast<unsigned>(blocks)), block(kBlock);
  if (lines)
    hipLaunchKernelGGL(fdm_contract_kernel<true>, grid, block, 0, st, int32_t(n), int32_t(nq), int32_t(tiles_q),
                       int32_t(tiles_i), M, int32_t(transpose), x, y, sc);
  else
    hipLaunchKernelGGL(fdm_contract_kernel<false>, grid, block, 0, st, int32_t(n), int32_t(nq), int32_t(tiles_q),
                       int32_t(tiles_i), M, int32_t(transpose), x, y, sc);
  NSS_CHECK_LAUNCH();
}

}  // namespace nss

using namespace nss;

struct nss_fdm_s {
  int dim = 0;
  int64_t ext[3] = {1, 1, 1};
  int64_t cells = 0;
  DeviceBuffer<double> Q[3];                               // device, row-major ext[a] x ext[a]
  DeviceBuffer<double> lam;                                // device, the d eigenvalue vectors one after the other
  DeviceBuffer<double> work[2];                            // device, `cells` doubles each
  FdmScale scale{};                                        // (its lam[] point into `lam`)
};

extern "C" {

int nss_fdm_contract_f64(int64_t outer, int64_t n, int64_t inner, const double* M, int32_t transpose, const double* x,
                         double* y, nss_stream_t stream) {
  return guarded([&] {
    NSS_REQUIRE(M && x && y, "fdm_contract: NULL argument");
    NSS_REQUIRE(x != y, "fdm_contract: y aliases x");
    const int64_t shape[3] = {outer, n, inner};
    fdm_cells(shape, 3, "fdm_contract");
    fdm_launch(outer, n, inner, M, transpose != 0, x, y, FdmScale{}, as_stream(stream));
  });
}

int nss_fdm_contract_scaled_f64(int64_t outer, int64_t n, int64_t inner, const double* M, int32_t transpose,
                                const double* x, double* y, int32_t dim, const int64_t* h_extents, const double* lam,
                                double null_threshold, nss_stream_t stream) {
  return guarded([&] {
    NSS_REQUIRE(M && x && y && h_extents && lam, "fdm_contract_scaled: NULL argument");
    NSS_REQUIRE(x != y, "fdm_contract_scaled: y aliases x");
    NSS_REQUIRE(dim == 2 || dim == 3, "fdm_contract_scaled: dim is 2 or 3");
    const int64_t shape[3] = {outer, n, inner};
    const int64_t cells = fdm_cells(shape, 3, "fdm_contract_scaled");
    NSS_REQUIRE(fdm_cells(h_extents, dim, "fdm_contract_scaled") == cells,
                "fdm_contract_scaled: the extents do not hold outer * n * inner cells");
    FdmScale sc{};
    sc.dim = dim;
    sc.threshold = null_threshold;
    const double* at = lam;
    for (int a = 0; a < dim; ++a) {
      sc.lam[a] = at;
      sc.ext[a] = int32_t(h_extents[a]);
      at += h_extents[a];
    }
    fdm_launch(outer, n, inner, M, transpose != 0, x, y, sc, as_stream(stream));
  });
}

int nss_fdm_create(int32_t dim, const int64_t* h_extents, const double* const* h_Q, const double* const* h_lambda,
                   double null_threshold, nss_fdm_t* out) {
  return guarded([&] {
    NSS_REQUIRE(h_extents && h_Q && h_lambda && out, "fdm_create: NULL argument");
    NSS_REQUIRE(dim == 2 || dim == 3, "fdm_create: dim is 2 or 3");
    const int64_t cells = fdm_cells(h_extents, dim, "fdm_create");
    for (int a = 0; a < dim; ++a) NSS_REQUIRE(h_Q[a] && h_lambda[a], "fdm_create: NULL factor");
    *out = nullptr;
    std::unique_ptr<nss_fdm_s> h(new nss_fdm_s);
    h->dim = dim;
    h->cells = cells;
    int64_t total = 0;
    for (int a = 0; a < dim; ++a) total += (h->ext[a] = h_extents[a]);
    h->lam.alloc(size_t(total));
    h->scale.dim = dim;
    h->scale.threshold = null_threshold;
    int64_t at = 0;
    for (int a = 0; a < dim; ++a) {
      const size_t e = size_t(h->ext[a]);
      h->Q[a].alloc(e * e);
      NSS_HIP(hipMemcpy(h->Q[a], h_Q[a], sizeof(double) * e * e, hipMemcpyHostToDevice));
      NSS_HIP(hipMemcpy(h->lam + at, h_lambda[a], sizeof(double) * e, hipMemcpyHostToDevice));
      h->scale.lam[a] = h->lam + at;
      h->scale.ext[a] = int32_t(e);
      at += int64_t(e);
    }
    for (DeviceBuffer<double>& w : h->work) w.alloc(size_t(cells));
    *out = h.release();
  });
}

int nss_fdm_destroy(nss_fdm_t h) {
  return guarded([&] { delete h; });
}

int nss_fdm_solve_f64(nss_fdm_t h, const double* rhs, double* phi, nss_stream_t stream) {
  return guarded([&] {
    NSS_REQUIRE(h && rhs && phi, "fdm_solve: NULL argument");
    NSS_REQUIRE(rhs != phi, "fdm_solve: phi aliases rhs");
    const int d = h->dim, passes = 2 * d;
    // forward: Q_a^T along every axis, the diagonal scaling on the last of them; backward: Q_a along every axis.
    // rhs -> work0 -> work1 -> work0 -> ... -> phi: pass k reads what pass k - 1 wrote.
    for (int k = 0; k < passes; ++k) {
      const int a = k % d;
      int64_t outer = 1, inner = 1;
      for (int b = 0; b < a; ++b) outer *= h->ext[b];
      for (int b = a + 1; b < d; ++b) inner *= h->ext[b];
      const double* src = k == 0 ? rhs : h->work[(k - 1) % 2];
      double* dst = k == passes - 1 ? phi : h->work[k % 2];
      fdm_launch(outer, h->ext[a], inner, h->Q[a], /*transpose=*/k < d, src, dst,
                 k == d - 1 ? h->scale : FdmScale{}, as_stream(stream));
    }
  });
}

}  // extern "C"
