// The exact inverse of the velocity block by fast diagonalisation, as a preconditioner of the fused Krylov loops
// (`hipla.FastDiagonalizationInverse`; `NavierStokes.SolveInitial(pre="fdm")`).  On the plain
// staggered grid A couples no two velocity components and is a Kronecker sum on each, so
//
//   y_c = scale * Q [ 1 / ((lambda_0[k] + lambda_1[j]) + lambda_2[i]) ] Q^T x_c,        Q = Q_0 (x) Q_1 (x) Q_2,
//
// per component c: 2 dim launches for all components together.  The handle, the addressing of the interleaved vector
// (entry (k, j, i) of component c at base_c + k * pitch + j * e_2 + i) and the argument checks are those of
// fdm_components.hip (fdm_layout.h); there is no mass and no sigma.  Two things are this file's own:
//
//   the loop contract   every launch takes `done` (device int, may be NULL) and returns before its first load when it is
//                       non-zero, and `scale` rides in the epilogue of the last forward pass, v * (scale / sum) with the
//                       sum in the host's order: k * preA costs nothing.
//   the tile            fdm_tile.h's FMA tile or fdm_tile_mfma.h's matrix-core tile (nss_fdmi_set_tile): the same bits
//                       every run with either; that both give the same bits is measured, not promised.
//
// Nothing outside the components is read or written: the two work buffers have the vector's layout, and a pass writes
// the components' entries only.
#include <algorithm>
#include <cmath>
#include <memory>

#include "fdm_inverse.h"
#include "fdm_layout.h"
#include "fdm_tile_mfma.h"
#include "nss_common.h"

namespace nss {

// one component of one pass, by value in the kernel arguments
struct FdmiComp {
  int64_t base;
  int64_t pitch;
  int32_t ext[3];                                          // (E0, E1, E2)
  int32_t pad;
  const double* Q;                                         // device, row-major, of the axis of the pass
  const double* lam[3];                                    // device, per internal axis (lam[1] unused for two axes)
};

struct FdmiPass {
  FdmiComp comp[kFdmcMaxComp];
  uint32_t end[kFdmcMaxComp];                              // running sum of the components' tile counts
  int32_t axis;                                            // internal: 0, 1 or 2
  int32_t transpose, scaled, dim;
  double scale;
};

// the tiles of a pass along `axis` over the extents: (n, nq, workgroups along the outer direction)
struct FdmiTiles {
  int64_t n, nq, outer;
};

__host__ __device__ inline FdmiTiles fdmi_tiles(const int32_t* ext, int axis) {
  const int64_t e0 = ext[0], e1 = ext[1], e2 = ext[2];
  if (axis == 0) return {e0, e1 * e2, 1};                  // q = (j, i) of one slab, contiguous; j steps by the pitch
  if (axis == 1) return {e1, e2, e0};                      // one k per workgroup, q = i, j steps by E2
  return {e2, e0 * e1, 1};                                 // the lines of the grid's x axis
}

template <bool LINES, bool MFMA>                           // LINES <=> axis == 2
__global__ __launch_bounds__(kBlock) void fdmi_pass_kernel(FdmiPass p, const int32_t* __restrict__ done,
                                                            const double* __restrict__ src, double* __restrict__ dst) {
  if (done && *done != 0) return;
  uint32_t blk = blockIdx.x;
  const bool past0 = blk >= p.end[0], past1 = blk >= p.end[1];
  const FdmiComp& d = past1 ? p.comp[2] : past0 ? p.comp[1] : p.comp[0];
  blk -= past1 ? p.end[1] : past0 ? p.end[0] : 0u;
  const int32_t axis = LINES ? 2 : p.axis;
  const int32_t E1 = d.ext[1], E2 = d.ext[2];
  const FdmiTiles t = fdmi_tiles(d.ext, axis);
  const int32_t n = int32_t(t.n), nq = int32_t(t.nq);
  const uint32_t tiles_q = uint32_t((nq + kFdmTile - 1) / kFdmTile), tiles_i = uint32_t((n + kFdmTile - 1) / kFdmTile);
  const int32_t q0 = int32_t(blk % tiles_q) * kFdmTile;
  const int32_t i0 = int32_t((blk / tiles_q) % tiles_i) * kFdmTile;
  const int32_t o = int32_t(blk / (tiles_q * tiles_i));    // the slab k of axis 1; 0 otherwise
  const int64_t pitch = d.pitch, base = d.base;
  // element (q, j) of the source and of the destination: qoff(q) + j * sj
  const int64_t sj = axis == 0 ? pitch : axis == 1 ? E2 : 1;
  auto qoff = [=](int32_t q) -> int64_t {
    return LINES ? base + int64_t(q / E1) * pitch + int64_t(q % E1) * E2 : base + o * pitch + q;
  };
  const double* l0 = d.lam[0];
  const double* l1 = d.lam[1];
  const double* l2 = d.lam[2];
  const double scale = p.scale;
  const int32_t scaled = p.scaled, dim = p.dim;
  auto epi = [=](int32_t q, int32_t i, double v) {
    if (!scaled) return v;
    int32_t c0, c1, c2;                                    // the entry's multi-index (k, j, i) in (E0, E1, E2)
    if (LINES) {
      c0 = q / E1, c1 = q % E1, c2 = i;
    } else if (axis == 0) {
      c0 = i, c1 = q / E2, c2 = q % E2;
    } else {
      c0 = o, c1 = i, c2 = q;
    }
    double sum = l0[c0];                                   // (lambda_0 + lambda_1) + lambda_2: the host's order
    if (dim == 3) sum += l1[c1];
    sum += l2[c2];
    return v * (scale / sum);
  };
  if constexpr (MFMA) fdm_tile_mfma<LINES>(n, nq, q0, i0, d.Q, p.transpose, src, dst, sj, sj, qoff, qoff, epi);
  else fdm_tile<LINES>(n, nq, q0, i0, d.Q, p.transpose, src, dst, sj, sj, qoff, qoff, epi);
}

// Which tile a pass runs, a property of the handle (nss_fdmi_set_tile; NSS_FDM_TILE on the Python side): -1 the library's
// choice, 0 the FMA tile, 1 the matrix-core tile.  Measured (profiles/fdm_stokes.md) the matrix-core tile is faster from
// extent 32 on and within the spread of the windows below, where an apply is its 2 dim launches: there is no extent from
// which the FMA tile wins, so the library's choice is the matrix-core tile from extent 1 on.
constexpr int kFdmiMfmaFromExtent = 1;                     // -1 takes the matrix-core tile from this contracted extent on

static bool fdmi_use_mfma(int tile, int64_t n) { return tile == 1 || (tile == -1 && n >= kFdmiMfmaFromExtent); }

}  // namespace nss

using namespace nss;

struct nss_fdmi_s {
  FdmLayout lay;
  int tile = -1;                                           // nss_fdmi_set_tile
  DeviceBuffer<double> Q[kFdmcMaxComp][3];                 // device, row-major, per internal axis (none for a skipped one)
  DeviceBuffer<double> lam[kFdmcMaxComp];                  // device, a component's eigenvalue vectors one after the other
  const double* lam_at[kFdmcMaxComp][3] = {};              // (point into `lam`)
  DeviceBuffer<double> work[2];                            // device, n_total doubles each, the vector's layout
};

namespace nss {

// one batched pass; the arguments have been checked
static void fdmi_launch(const nss_fdmi_s& h, int axis, int transpose, int scaled, double scale, const double* src,
                        double* dst, const int32_t* done, hipStream_t st) {
  FdmiPass p{};
  p.axis = axis;
  p.transpose = transpose;
  p.scaled = scaled;
  p.dim = h.lay.dim;
  p.scale = scale;
  int64_t blocks = 0, widest = 0;
  for (int c = 0; c < kFdmcMaxComp; ++c) {
    if (c < h.lay.ncomp) {
      FdmiComp& d = p.comp[c];
      d.base = h.lay.base[c];
      d.pitch = h.lay.pitch;
      for (int a = 0; a < 3; ++a) {
        d.ext[a] = h.lay.ext[c][a];
        d.lam[a] = h.lam_at[c][a];
      }
      d.Q = h.Q[c][axis];
      const FdmiTiles t = fdmi_tiles(d.ext, axis);
      blocks += ((t.nq + kFdmTile - 1) / kFdmTile) * ((t.n + kFdmTile - 1) / kFdmTile) * t.outer;   // <= its entries
      widest = std::max(widest, t.n);
    }
    p.end[c] = uint32_t(blocks);                           // (a component that is not there: no tiles)
  }
  const dim3 grid(static_cast<unsigned>(blocks)), block(kBlock);
  const bool mfma = fdmi_use_mfma(h.tile, widest);
  if (axis == 2) {
    if (mfma) hipLaunchKernelGGL((fdmi_pass_kernel<true, true>), grid, block, 0, st, p, done, src, dst);
    else hipLaunchKernelGGL((fdmi_pass_kernel<true, false>), grid, block, 0, st, p, done, src, dst);
  } else {
    if (mfma) hipLaunchKernelGGL((fdmi_pass_kernel<false, true>), grid, block, 0, st, p, done, src, dst);
    else hipLaunchKernelGGL((fdmi_pass_kernel<false, false>), grid, block, 0, st, p, done, src, dst);
  }
  NSS_CHECK_LAUNCH();
}

int64_t fdmi_rows(const nss_fdmi_s& h) { return h.lay.n_total; }

void fdmi_apply(const nss_fdmi_s& h, double scale, const double* x, double* y, const int32_t* done, hipStream_t st) {
  NSS_REQUIRE(x && y, "fdmi_apply: NULL argument");
  NSS_REQUIRE(x != y, "fdmi_apply: y aliases x");
  NSS_REQUIRE(std::isfinite(scale), "fdmi_apply: the scale is not finite");
  const int d = h.lay.dim, passes = 2 * d;
  // forward: Q_a^T along every axis, the scaling on the last of them; backward: Q_a along every axis.
  // x -> work0 -> work1 -> work0 -> ... -> y: pass k reads what pass k - 1 wrote.
  for (int k = 0; k < passes; ++k) {
    const double* src = k == 0 ? x : h.work[(k - 1) % 2];
    double* dst = k == passes - 1 ? y : h.work[k % 2];
    fdmi_launch(h, fdm_internal_axis(d, k % d), /*transpose=*/k < d, /*scaled=*/k == d - 1, scale, src, dst, done, st);
  }
}

}  // namespace nss

extern "C" {

int nss_fdmi_create(int32_t ncomp, int32_t dim, int64_t n_total, const int64_t* h_base, int64_t pitch,
                    const int64_t* h_extents, const double* const* h_Q, const double* const* h_lambda, nss_fdmi_t* out) {
  return guarded([&] {
    NSS_REQUIRE(h_base && h_extents && h_Q && h_lambda && out, "fdmi_create: NULL argument");
    *out = nullptr;
    std::unique_ptr<nss_fdmi_s> h(new nss_fdmi_s);
    h->lay = fdm_layout_checked("fdmi_create", ncomp, dim, n_total, h_base, pitch, h_extents, h_Q, h_lambda);
    // A is definite: every sum of eigenvalues is positive and finite (the host declines before it comes to this)
    for (int c = 0; c < ncomp; ++c) {
      double least = 0.0;
      for (int a = 0; a < dim; ++a) {
        const double* lam = h_lambda[c * dim + a];
        const int64_t e = h_extents[c * dim + a];
        double lo = lam[0];
        for (int64_t i = 0; i < e; ++i) {
          NSS_REQUIRE(std::isfinite(lam[i]),
                      "fdmi_create: component " + std::to_string(c) + ": an eigenvalue is not finite");
          lo = std::min(lo, lam[i]);
        }
        least += lo;
      }
      NSS_REQUIRE(least > 0.0, "fdmi_create: component " + std::to_string(c) +
                                   ": the least sum of eigenvalues is not positive (the operator has no inverse)");
    }
    for (int c = 0; c < ncomp; ++c) {
      int64_t total = 0;
      for (int a = 0; a < dim; ++a) total += h_extents[c * dim + a];
      h->lam[c].alloc(size_t(total));
      int64_t at = 0;
      for (int a = 0; a < dim; ++a) {
        const int ia = fdm_internal_axis(dim, a);
        const size_t e = size_t(h_extents[c * dim + a]);
        h->Q[c][ia].alloc(e * e);
        NSS_HIP(hipMemcpy(h->Q[c][ia], h_Q[c * dim + a], sizeof(double) * e * e, hipMemcpyHostToDevice));
        NSS_HIP(hipMemcpy(h->lam[c] + at, h_lambda[c * dim + a], sizeof(double) * e, hipMemcpyHostToDevice));
        h->lam_at[c][ia] = h->lam[c] + at;
        at += int64_t(e);
      }
    }
    for (DeviceBuffer<double>& w : h->work) w.alloc(size_t(n_total));
    *out = h.release();
  });
}

int nss_fdmi_destroy(nss_fdmi_t h) {
  return guarded([&] { delete h; });
}

int nss_fdmi_apply_f64(nss_fdmi_t h, double scale, const double* x, double* y, const int32_t* done,
                       nss_stream_t stream) {
  return guarded([&] {
    NSS_REQUIRE(h, "fdmi_apply: NULL argument");
    fdmi_apply(*h, scale, x, y, done, as_stream(stream));
  });
}

int nss_fdmi_contract_f64(int64_t n, int64_t nq, int32_t lines, int32_t tile, const double* M, int32_t transpose,
                          const double* x, double* y, const int32_t* done, nss_stream_t stream) {
  return guarded([&] {
    NSS_REQUIRE(M && x && y, "fdmi_contract: NULL argument");
    NSS_REQUIRE(tile >= -1 && tile <= 1,
                "fdmi_contract: the tile is -1 (the library's choice), 0 (FMA) or 1 (matrix cores)");
    NSS_REQUIRE(x != y, "fdmi_contract: y aliases x");
    NSS_REQUIRE(n >= 1 && nq >= 1 && n <= kFdmcMaxTotal / nq, "fdmi_contract: n * nq is not in 1 .. 2^31 - 1");
    // one component over the extents (n, 1, nq) contracted along axis 0 (q contiguous), or (nq, 1, n) along axis 2 (the
    // lines of the x axis): what a pass of the apply launches, without a handle
    FdmiPass p{};
    FdmiComp& d = p.comp[0];
    d.base = 0;
    d.pitch = lines ? n : nq;
    d.ext[0] = int32_t(lines ? nq : n);
    d.ext[1] = 1;
    d.ext[2] = int32_t(lines ? n : nq);
    d.Q = M;
    p.axis = lines ? 2 : 0;
    p.transpose = transpose != 0;
    p.dim = 2;
    p.scale = 1.0;
    const int64_t blocks = ((nq + kFdmTile - 1) / kFdmTile) * ((n + kFdmTile - 1) / kFdmTile);
    p.end[0] = p.end[1] = p.end[2] = uint32_t(blocks);
    const dim3 grid(static_cast<unsigned>(blocks)), block(kBlock);
    hipStream_t st = as_stream(stream);
    const bool mfma = fdmi_use_mfma(tile, n);
    if (lines) {
      if (mfma) hipLaunchKernelGGL((fdmi_pass_kernel<true, true>), grid, block, 0, st, p, done, x, y);
      else hipLaunchKernelGGL((fdmi_pass_kernel<true, false>), grid, block, 0, st, p, done, x, y);
    } else {
      if (mfma) hipLaunchKernelGGL((fdmi_pass_kernel<false, true>), grid, block, 0, st, p, done, x, y);
      else hipLaunchKernelGGL((fdmi_pass_kernel<false, false>), grid, block, 0, st, p, done, x, y);
    }
    NSS_CHECK_LAUNCH();
  });
}

int nss_fdmi_set_tile(nss_fdmi_t h, int32_t mode) {
  return guarded([&] {
    NSS_REQUIRE(h, "fdmi_set_tile: NULL argument");
    NSS_REQUIRE(mode >= -1 && mode <= 1, "fdmi_set_tile: -1 (the library's choice), 0 (FMA tile) or 1 (matrix-core tile)");
    h->tile = mode;
  });
}

}  // extern "C"
