// Fast diagonalisation of a shifted operator on the components of an interleaved vector
// (`hipla.ComponentFastDiagonalization`; the direct velocity and scalar solves of `NavierStokes.SetImplicitSolve("fdm")`,
// DESIGN.md section 17).  The velocity vector of the staggered grid is slab-major with its components interleaved per
// slab: component c is an array over its own extents (e_0, e_1, e_2), and its entry (k, j, i) sits at
//
//   base_c + k * pitch + j * e_2 + i                  (two axes: (k, i) at base_c + k * pitch + i)
//
// -- contiguous inside a slab, strided by `pitch` across slabs.  On every component A_c is a Kronecker sum with factors
// T_a = Q_a diag(lambda_a) Q_a^T and the mass is m_c I, so
//
//   (m_c I + sigma A_c)^-1 = Q [ 1 / (m_c + sigma ((lambda_0[k] + lambda_1[j]) + lambda_2[i])) ] Q^T,   Q = Q_0 (x) Q_1 (x) Q_2,
//
// with the same Q and lambda for every sigma.  One solve is 2 dim launches for ALL components together: a pass
// contracts every component along one of its axes, the grid being the concatenation of the components' tile ranges.  A
// block finds its component with two compares against the running sum of the tile counts and reads that component's
// descriptor from the kernel arguments; its tile is fdm_tile.h's, the arithmetic of fdm.hip's contraction bit for bit.
// What this file adds is the addressing, per axis of the (internally always three) extents (E0, E1, E2), two axes being
// (e_0, 1, e_1):
//
//   axis 0  q = (j, i) of one slab, contiguous;  j steps by the pitch.                                  LINES = false
//   axis 1  one k per workgroup (its offset k * pitch), q = i, j steps by E2.                           LINES = false
//   axis 2  the lines of the grid's x axis: line q = (k, j) starts at base + k * pitch + j * E2.        LINES = true
//
// and the shifted epilogue on the last forward pass.  Nothing outside the components is read or written: the two work
// buffers have the vector's layout, and a pass writes the components' entries only.
#include <algorithm>
#include <cmath>
#include <memory>

#include "fdm_layout.h"
#include "fdm_tile.h"
#include "nss_common.h"

namespace nss {

// one component of one pass, by value in the kernel arguments
struct FdmcComp {
  int64_t base;
  int64_t pitch_src, pitch_dst;                            // of the slowest axis, in the source and in the destination
  int32_t ext[3];                                          // (E0, E1, E2)
  int32_t pad;
  const double* Q;                                         // device, row-major, of the axis of the pass
  const double* lam[3];                                    // device, per internal axis (lam[1] unused for two axes)
  double mass;
};

struct FdmcPass {
  FdmcComp comp[kFdmcMaxComp];
  uint32_t end[kFdmcMaxComp];                              // running sum of the components' tile counts
  int32_t axis;                                            // internal: 0, 1 or 2
  int32_t transpose, scaled, dim;
  double sigma;
  const int32_t* done;                                     // device int (or NULL): non-zero -> the pass returns at once
};

// the tiles of a component in a pass along `axis`: (tiles of q, tiles of i, workgroups along o)
struct FdmcTiles {
  int64_t n, nq, outer;
};

__host__ __device__ inline FdmcTiles fdmc_tiles(const int32_t* ext, int axis) {
  const int64_t e0 = ext[0], e1 = ext[1], e2 = ext[2];
  if (axis == 0) return {e0, e1 * e2, 1};
  if (axis == 1) return {e1, e2, e0};
  return {e2, e0 * e1, 1};
}

template <bool LINES>                                      // LINES <=> axis == 2
__global__ __launch_bounds__(kBlock) void fdmc_pass_kernel(FdmcPass p, const double* __restrict__ src,
                                                            double* __restrict__ dst) {
  if (p.done != nullptr && *p.done != 0) return;           // (a frozen loop: nss::fdmc_solve)
  uint32_t blk = blockIdx.x;
  const bool past0 = blk >= p.end[0], past1 = blk >= p.end[1];
  const FdmcComp& d = past1 ? p.comp[2] : past0 ? p.comp[1] : p.comp[0];
  blk -= past1 ? p.end[1] : past0 ? p.end[0] : 0u;
  const int32_t axis = LINES ? 2 : p.axis;
  const int32_t E1 = d.ext[1], E2 = d.ext[2];
  const FdmcTiles t = fdmc_tiles(d.ext, axis);
  const int32_t n = int32_t(t.n), nq = int32_t(t.nq);
  const uint32_t tiles_q = uint32_t((nq + kFdmTile - 1) / kFdmTile), tiles_i = uint32_t((n + kFdmTile - 1) / kFdmTile);
  const int32_t q0 = int32_t(blk % tiles_q) * kFdmTile;
  const int32_t i0 = int32_t((blk / tiles_q) % tiles_i) * kFdmTile;
  const int32_t o = int32_t(blk / (tiles_q * tiles_i));    // the slab k of axis 1; 0 otherwise
  const int64_t ps = d.pitch_src, pd = d.pitch_dst, base = d.base;
  // element (q, j) of the source: qx(q) + j * sjx; element (q, i) of the destination: qy(q) + i * sjy
  const int64_t sjx = axis == 0 ? ps : axis == 1 ? E2 : 1, sjy = axis == 0 ? pd : axis == 1 ? E2 : 1;
  auto qx = [=](int32_t q) -> int64_t {
    return LINES ? base + int64_t(q / E1) * ps + int64_t(q % E1) * E2 : base + o * ps + q;
  };
  auto qy = [=](int32_t q) -> int64_t {
    return LINES ? base + int64_t(q / E1) * pd + int64_t(q % E1) * E2 : base + o * pd + q;
  };
  const double* l0 = d.lam[0];
  const double* l1 = d.lam[1];
  const double* l2 = d.lam[2];
  const double mass = d.mass, sigma = p.sigma;
  const int32_t scaled = p.scaled, dim = p.dim;
  fdm_tile<LINES>(n, nq, q0, i0, d.Q, p.transpose, src, dst, sjx, sjy, qx, qy, [=](int32_t q, int32_t i, double v) {
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
    return v * (1.0 / __dadd_rn(mass, __dmul_rn(sigma, sum)));       // m + sigma * sum, as the host rounds it
  });
}

}  // namespace nss

using namespace nss;

struct nss_fdmc_s {
  int ncomp = 0, dim = 0;
  int64_t n_total = 0, pitch = 0;
  int64_t base[kFdmcMaxComp] = {0, 0, 0};
  int32_t ext[kFdmcMaxComp][3] = {{1, 1, 1}, {1, 1, 1}, {1, 1, 1}};      // internal: (e_0, 1, e_1) for two axes
  double mass[kFdmcMaxComp] = {0, 0, 0};
  DeviceBuffer<double> Q[kFdmcMaxComp][3];                 // device, row-major, per internal axis (none for a skipped one)
  DeviceBuffer<double> lam[kFdmcMaxComp];                  // device, the eigenvalue vectors of a component one after the other
  const double* lam_at[kFdmcMaxComp][3] = {};              // (point into `lam`)
  DeviceBuffer<double> work[2];                            // device, n_total doubles each, the vector's layout
};

// the internal axis of the caller's axis a
static int fdmc_axis(int dim, int a) { return fdm_internal_axis(dim, a); }

// one batched pass; the arguments have been checked
static void fdmc_launch(const nss_fdmc_s& h, int axis, int transpose, int scaled, double sigma, const double* src,
                        double* dst, hipStream_t st, const int32_t* done = nullptr) {
  FdmcPass p{};
  p.done = done;
  p.axis = axis;
  p.transpose = transpose;
  p.scaled = scaled;
  p.dim = h.dim;
  p.sigma = sigma;
  int64_t blocks = 0;
  for (int c = 0; c < kFdmcMaxComp; ++c) {
    if (c < h.ncomp) {
      FdmcComp& d = p.comp[c];
      d.base = h.base[c];
      d.pitch_src = d.pitch_dst = h.pitch;
      for (int a = 0; a < 3; ++a) {
        d.ext[a] = h.ext[c][a];
        d.lam[a] = h.lam_at[c][a];
      }
      d.Q = h.Q[c][axis];
      d.mass = h.mass[c];
      const FdmcTiles t = fdmc_tiles(d.ext, axis);
      blocks += ((t.nq + kFdmTile - 1) / kFdmTile) * ((t.n + kFdmTile - 1) / kFdmTile) * t.outer;   // <= its entries
    }
    p.end[c] = uint32_t(blocks);                           // (a component that is not there: no tiles)
  }
  const dim3 grid(static_cast<unsigned>(blocks)), block(kBlock);
  if (axis == 2)
    hipLaunchKernelGGL(fdmc_pass_kernel<true>, grid, block, 0, st, p, src, dst);
  else
    hipLaunchKernelGGL(fdmc_pass_kernel<false>, grid, block, 0, st, p, src, dst);
  NSS_CHECK_LAUNCH();
}

namespace nss {

int64_t fdmc_rows(const nss_fdmc_s& h) { return h.n_total; }                 // (loop_parts.h: the BiCGStab loop asks)

// forward: Q_a^T along every axis, the shifted scaling on the last of them; backward: Q_a along every axis.
// rhs -> work0 -> work1 -> work0 -> ... -> out: pass k reads what pass k - 1 wrote.  `done`: see FdmcPass.
void fdmc_solve(const nss_fdmc_s& h, double sigma, const double* rhs, double* out, const int32_t* done, hipStream_t st) {
  NSS_REQUIRE(rhs && out && rhs != out, "fdmc_solve: NULL argument, or out aliases rhs");
  NSS_REQUIRE(std::isfinite(sigma) && sigma >= 0.0, "fdmc_solve: sigma is negative or not finite");
  const int d = h.dim, passes = 2 * d;
  for (int k = 0; k < passes; ++k) {
    const double* src = k == 0 ? rhs : h.work[(k - 1) % 2];
    double* dst = k == passes - 1 ? out : h.work[k % 2];
    fdmc_launch(h, fdmc_axis(d, k % d), /*transpose=*/k < d, /*scaled=*/k == d - 1, sigma, src, dst, st, done);
  }
}

}  // namespace nss

extern "C" {

int nss_fdmc_create(int32_t ncomp, int32_t dim, int64_t n_total, const int64_t* h_base, int64_t pitch,
                    const int64_t* h_extents, const double* const* h_Q, const double* const* h_lambda,
                    const double* h_mass, nss_fdmc_t* out) {
  return guarded([&] {
    NSS_REQUIRE(h_base && h_extents && h_Q && h_lambda && h_mass && out, "fdmc_create: NULL argument");
    *out = nullptr;
    // the layout, its checks and the overlap arithmetic: fdm_layout.h (shared with nss_fdmi_create)
    const FdmLayout lay = fdm_layout_checked("fdmc_create", ncomp, dim, n_total, h_base, pitch, h_extents, h_Q, h_lambda);
    std::unique_ptr<nss_fdmc_s> h(new nss_fdmc_s);
    h->ncomp = ncomp;
    h->dim = dim;
    h->n_total = n_total;
    h->pitch = pitch;
    for (int c = 0; c < ncomp; ++c) {
      NSS_REQUIRE(h_mass[c] > 0.0 && std::isfinite(h_mass[c]),
                  "fdmc_create: component " + std::to_string(c) + ": the mass is not positive and finite");
      h->mass[c] = h_mass[c];
      h->base[c] = lay.base[c];
      for (int a = 0; a < 3; ++a) h->ext[c][a] = lay.ext[c][a];
    }
    for (int c = 0; c < ncomp; ++c) {
      int64_t total = 0;
      for (int a = 0; a < dim; ++a) total += h_extents[c * dim + a];
      h->lam[c].alloc(size_t(total));
      int64_t at = 0;
      for (int a = 0; a < dim; ++a) {
        const int ia = fdmc_axis(dim, a);
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

int nss_fdmc_destroy(nss_fdmc_t h) {
  return guarded([&] { delete h; });
}

int nss_fdmc_pass_f64(nss_fdmc_t h, int32_t axis, int32_t transpose, int32_t scaled, double sigma, const double* src,
                      double* dst, nss_stream_t stream) {
  return guarded([&] {
    NSS_REQUIRE(h && src && dst, "fdmc_pass: NULL argument");
    NSS_REQUIRE(src != dst, "fdmc_pass: dst aliases src");
    NSS_REQUIRE(axis >= 0 && axis < h->dim, "fdmc_pass: the axis is not in 0 .. dim - 1");
    NSS_REQUIRE(!scaled || (std::isfinite(sigma) && sigma >= 0.0), "fdmc_pass: sigma is negative or not finite");
    fdmc_launch(*h, fdmc_axis(h->dim, axis), transpose != 0, scaled != 0, sigma, src, dst, as_stream(stream));
  });
}

int nss_fdmc_solve_f64(nss_fdmc_t h, double sigma, const double* rhs, double* out, nss_stream_t stream) {
  return guarded([&] {
    NSS_REQUIRE(h && rhs && out, "fdmc_solve: NULL argument");
    NSS_REQUIRE(rhs != out, "fdmc_solve: out aliases rhs");
    fdmc_solve(*h, sigma, rhs, out, nullptr, as_stream(stream));
  });
}

}  // extern "C"
