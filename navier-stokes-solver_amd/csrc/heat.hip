// Kernels of the device-resident heat exponential integrator (`heat.evolve`, `hipla.fused.HeatIntegrator`; the
// reference's heat.py:95-142 with orthonormalization.py:5-16).  The operand is a basis of d <= 8 vectors of length n
// stored as PLANES: vector k occupies basis[k * ld .. k * ld + n), ld >= n even, so that every vector is itself a
// contiguous, 16-byte aligned operand of the CG loop, the SpMV and the element-wise kernels.
//
//   nss_mgs_f64           repeated modified Gram-Schmidt, every scalar on the device.  Column j of one pass is the chain
//                           first   (i = 0)      : partials of <b_0, b_j>, <b_0, b_0>               reads b_0, b_j
//                           project (0 < i < j)  : c = <b_{i-1}, b_j> / <b_{i-1}, b_{i-1}> from the previous launch's
//                                                  partials (every workgroup adds them by the fixed tree);
//                                                  b_j -= c b_{i-1};  partials of <b_i, b_j>, <b_i, b_i>
//                                                                                   reads b_{i-1}, b_i, b_j, writes b_j
//                           last                 : the pending update (j > 0); partials of <b_j, b_j>
//                           scale                : b_j *= 1 / sqrt(<b_j, b_j>); norms[pass * d + j] = <b_j, b_j>
//                         j + 2 launches (column 0: 2), none of which waits for the host.  Two sets of partials
//                         alternate: a launch reads the set its predecessor wrote and writes the other one.
//   nss_galerkin_f64      G = V^T (M V) in one pass over the rows of M, one lane per row: the d row products
//                         w_k = sum_c M[r, c] V[c, k] from ONE read of the row, then acc[a][k] += V[r, a] w_k in
//                         registers; per workgroup d^2 partials, added by the fixed tree in a second launch.
//   nss_basis_combine_f64 y = sum_i coeff[i] V_i in one pass.
//
// All fp64, no atomics: every sum is per-workgroup partials added in a fixed order (fixed_sums_1024), the grids depend
// on n alone -- the same bits every run.
#include "csr_stream.h"
#include "loop_parts.h"

namespace nss {

constexpr int kHeatMaxDim = 8;
constexpr int kHeatMaxBlocks = 1024;    // partials per sum: the short form of fixed_sums_1024 (one memory latency)

static int mgs_grid(int64_t n) {         // one lane per PAIR of rows
  const int64_t g = ((n + 1) / 2 + kBlock - 1) / kBlock;
  return int(g < 1 ? 1 : g > kHeatMaxBlocks ? kHeatMaxBlocks : g);
}
static int galerkin_grid(int64_t n) {    // one lane per row
  const int64_t g = (n + kBlock - 1) / kBlock;
  return int(g < 1 ? 1 : g > kHeatMaxBlocks ? kHeatMaxBlocks : g);
}
static int64_t heat_work_doubles(int64_t n, int d) {
  const int64_t mgs = 4 * int64_t(kHeatMaxBlocks), gal = int64_t(d) * d * galerkin_grid(n);
  return mgs > gal ? mgs : gal;
}

// ACC: 0 nothing, 1 partials of <next, b_j> and <next, next>, 2 partials of <b_j, b_j>
template <bool UPDATE, int ACC>
__global__ __launch_bounds__(kBlock) void mgs_kernel(int64_t n, double* bj, const double* __restrict__ prev,
                                                      const double* __restrict__ next,
                                                      const double* __restrict__ pa_in,
                                                      const double* __restrict__ pb_in, int nin,
                                                      double* __restrict__ pa_out, double* __restrict__ pb_out) {
  __shared__ double lds[kRedDoubles];
  double c = 0.0;
  if constexpr (UPDATE) {
    const SumPair s = fixed_sums_1024(pa_in, nin, pb_in, nin, lds);
    c = s.a / s.b;
  }
  double acc_a = 0.0, acc_b = 0.0;
  const int64_t npair = n >> 1, stride = int64_t(gridDim.x) * kBlock;
  for (int64_t p = int64_t(blockIdx.x) * kBlock + threadIdx.x; p < npair; p += stride) {
    double2 x = ld2(bj + 2 * p);
    if constexpr (UPDATE) {
      const double2 q = ld2(prev + 2 * p);
      x.x = fma(-c, q.x, x.x);
      x.y = fma(-c, q.y, x.y);
      st2(bj + 2 * p, x);
    }
    if constexpr (ACC == 1) {
      const double2 y = ld2(next + 2 * p);
      acc_a = fma(y.y, x.y, fma(y.x, x.x, acc_a));
      acc_b = fma(y.y, y.y, fma(y.x, y.x, acc_b));
    } else if constexpr (ACC == 2) {
      acc_a = fma(x.y, x.y, fma(x.x, x.x, acc_a));
    }
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {      // the last row of an odd n
    const int64_t r = n - 1;
    double x = bj[r];
    if constexpr (UPDATE) {
      x = fma(-c, prev[r], x);
      bj[r] = x;
    }
    if constexpr (ACC == 1) {
      const double y = next[r];
      acc_a = fma(y, x, acc_a);
      acc_b = fma(y, y, acc_b);
    } else if constexpr (ACC == 2) {
      acc_a = fma(x, x, acc_a);
    }
  }
  if constexpr (ACC != 0) {
    store_block_partial(acc_a, blockIdx.x, pa_out, lds);
    if constexpr (ACC == 1) store_block_partial(acc_b, blockIdx.x, pb_out, lds);
  }
}

// b_j *= 1 / sqrt(s), s = the sum of the partials of <b_j, b_j>; *norm2 = s
__global__ __launch_bounds__(kBlock) void mgs_scale_kernel(int64_t n, double* __restrict__ bj,
                                                            const double* __restrict__ pa_in, int nin,
                                                            double* __restrict__ norm2) {
  __shared__ double lds[kRedDoubles];
  const double s = fixed_sums_1024(pa_in, nin, pa_in, 0, lds).a;
  if (blockIdx.x == 0 && threadIdx.x == 0) *norm2 = s;
  const double f = 1.0 / sqrt(s);
  const int64_t npair = n >> 1, stride = int64_t(gridDim.x) * kBlock;
  for (int64_t p = int64_t(blockIdx.x) * kBlock + threadIdx.x; p < npair; p += stride) {
    double2 x = ld2(bj + 2 * p);
    x.x *= f;
    x.y *= f;
    st2(bj + 2 * p, x);
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) bj[n - 1] *= f;
}

// One lane per row of M.  partials[(a * D + k) * gridDim.x + block] = the workgroup's part of G[a][k].
template <int D>
__global__ __launch_bounds__(kBlock) void galerkin_kernel(int32_t n, const int32_t* __restrict__ rowptr,
                                                           const int32_t* __restrict__ col,
                                                           const double* __restrict__ val, int64_t ld,
                                                           const double* __restrict__ basis,
                                                           double* __restrict__ partials) {
  __shared__ double lds[kBlock / kWave][D * D];
  double acc[D][D];
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int k = 0; k < D; ++k) acc[a][k] = 0.0;
  const int stride = gridDim.x * kBlock;
  for (int64_t r = int64_t(blockIdx.x) * kBlock + threadIdx.x; r < n; r += stride) {
    const int s = rowptr[r], e = rowptr[r + 1];
    double w[D];
#pragma unroll
    for (int k = 0; k < D; ++k) w[k] = 0.0;
    for (int p = s; p < e; ++p) {
      const double v = val[p];
      const double* x = basis + col[p];
#pragma unroll
      for (int k = 0; k < D; ++k) w[k] = fma(v, x[k * ld], w[k]);
    }
#pragma unroll
    for (int a = 0; a < D; ++a) {
      const double va = basis[a * ld + r];
#pragma unroll
      for (int k = 0; k < D; ++k) acc[a][k] = fma(va, w[k], acc[a][k]);
    }
  }
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const double t = wave_sum(acc[a][k]);
      if (lane == 0) lds[wave][a * D + k] = t;
    }
  __syncthreads();
  if (threadIdx.x < D * D) {
    double t = lds[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kBlock / kWave; ++w) t += lds[w][threadIdx.x];
    partials[int64_t(threadIdx.x) * gridDim.x + blockIdx.x] = t;
  }
}

// workgroup e: G[e] = the sum of partials[e * nblk .. (e + 1) * nblk)
__global__ __launch_bounds__(kBlock) void galerkin_finish_kernel(const double* __restrict__ partials, int nblk,
                                                                  double* __restrict__ g) {
  __shared__ double lds[kRedDoubles];
  const double* p = partials + int64_t(blockIdx.x) * nblk;
  const double s = fixed_sums_1024(p, nblk, p, 0, lds).a;
  if (threadIdx.x == 0) g[blockIdx.x] = s;
}

struct CombineArgs { double c[kHeatMaxDim]; };

// y = sum_i c_i V_i, left to right; y may be V_0 (every lane reads its rows of all planes before it writes)
template <int D>
__global__ __launch_bounds__(kBlock) void combine_kernel(int64_t n, int64_t ld, const double* basis, CombineArgs co,
                                                          double* y) {
  const int64_t npair = n >> 1, stride = int64_t(gridDim.x) * kBlock;
  for (int64_t p = int64_t(blockIdx.x) * kBlock + threadIdx.x; p < npair; p += stride) {
    double2 v[D];
#pragma unroll
    for (int i = 0; i < D; ++i) v[i] = ld2(basis + i * ld + 2 * p);
    double2 s{co.c[0] * v[0].x, co.c[0] * v[0].y};
#pragma unroll
    for (int i = 1; i < D; ++i) {
      s.x = fma(co.c[i], v[i].x, s.x);
      s.y = fma(co.c[i], v[i].y, s.y);
    }
    st2(y + 2 * p, s);
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    const int64_t r = n - 1;
    double v[D];
#pragma unroll
    for (int i = 0; i < D; ++i) v[i] = basis[i * ld + r];
    double s = co.c[0] * v[0];
#pragma unroll
    for (int i = 1; i < D; ++i) s = fma(co.c[i], v[i], s);
    y[r] = s;
  }
}

static void require_basis(const char* who, int64_t n, int32_t d, int64_t ld, const double* basis) {
  const std::string w(who);
  NSS_REQUIRE(d >= 1 && d <= kHeatMaxDim, (w + ": 1 <= d <= 8").c_str());
  NSS_REQUIRE(basis != nullptr, (w + ": NULL basis").c_str());
  NSS_REQUIRE(n >= 1 && ld >= n && (ld & 1) == 0, (w + ": need n >= 1 and an even plane stride ld >= n").c_str());
  NSS_REQUIRE(aligned16(basis), (w + ": the basis is not 16-byte aligned").c_str());
}

#define NSS_HEAT_DISPATCH(d, CALL)            \
  switch (d) {                                \
    case 1: CALL(1) break;                    \
    case 2: CALL(2) break;                    \
    case 3: CALL(3) break;                    \
    case 4: CALL(4) break;                    \
    case 5: CALL(5) break;                    \
    case 6: CALL(6) break;                    \
    case 7: CALL(7) break;                    \
    default: CALL(8) break;                   \
  }

}  // namespace nss

using namespace nss;

extern "C" {

int nss_heat_workspace(int64_t n, int32_t d, int64_t* work_doubles) {
  return guarded([&] {
    NSS_REQUIRE(work_doubles != nullptr, "heat_workspace: NULL argument");
    NSS_REQUIRE(n >= 1 && d >= 1 && d <= kHeatMaxDim, "heat_workspace: need n >= 1 and 1 <= d <= 8");
    *work_doubles = heat_work_doubles(n, d);
  });
}

int nss_mgs_f64(int64_t n, int32_t d, int64_t ld, double* basis, int32_t tries, double* norms, double* work,
                int64_t work_cap, nss_stream_t stream) {
  return guarded([&] {
    require_basis("mgs", n, d, ld, basis);
    NSS_REQUIRE(tries >= 1, "mgs: tries >= 1");
    NSS_REQUIRE(norms != nullptr && work != nullptr, "mgs: NULL norms or work");
    NSS_REQUIRE(work_cap >= heat_work_doubles(n, d), "mgs: work holds fewer doubles than nss_heat_workspace asks for");
    const int grid = mgs_grid(n);
    hipStream_t st = as_stream(stream);
    double* pa[2] = {work, work + 2 * kHeatMaxBlocks};
    double* pb[2] = {work + kHeatMaxBlocks, work + 3 * kHeatMaxBlocks};
    int cur = 0;                                            // the set the NEXT launch writes
    for (int t = 0; t < tries; ++t)
      for (int j = 0; j < d; ++j) {
        double* bj = basis + j * ld;
        for (int i = 0; i < j; ++i) {
          const double* bi = basis + i * ld;
          if (i == 0)
            hipLaunchKernelGGL((mgs_kernel<false, 1>), dim3(grid), dim3(kBlock), 0, st, n, bj, nullptr, bi, nullptr,
                               nullptr, 0, pa[cur], pb[cur]);
          else
            hipLaunchKernelGGL((mgs_kernel<true, 1>), dim3(grid), dim3(kBlock), 0, st, n, bj, bi - ld, bi, pa[cur ^ 1],
                               pb[cur ^ 1], grid, pa[cur], pb[cur]);
          NSS_CHECK_LAUNCH();
          cur ^= 1;
        }
        if (j == 0)
          hipLaunchKernelGGL((mgs_kernel<false, 2>), dim3(grid), dim3(kBlock), 0, st, n, bj, nullptr, nullptr, nullptr,
                             nullptr, 0, pa[cur], pb[cur]);
        else
          hipLaunchKernelGGL((mgs_kernel<true, 2>), dim3(grid), dim3(kBlock), 0, st, n, bj, bj - ld, nullptr,
                             pa[cur ^ 1], pb[cur ^ 1], grid, pa[cur], pb[cur]);
        NSS_CHECK_LAUNCH();
        hipLaunchKernelGGL(mgs_scale_kernel, dim3(grid), dim3(kBlock), 0, st, n, bj, pa[cur], grid,
                           norms + int64_t(t) * d + j);
        NSS_CHECK_LAUNCH();
        cur ^= 1;
      }
  });
}

int nss_galerkin_f64(nss_csr_t m, int32_t d, int64_t ld, const double* basis, double* g, double* work,
                     int64_t work_cap, nss_stream_t stream) {
  return guarded([&] {
    NSS_REQUIRE(m != nullptr, "galerkin: NULL matrix");
    NSS_REQUIRE(m->m == m->n, "galerkin: the matrix is not square");
    require_basis("galerkin", m->m, d, ld, basis);
    NSS_REQUIRE(g != nullptr && work != nullptr, "galerkin: NULL g or work");
    require_f64_values(m, "galerkin");
    NSS_REQUIRE(work_cap >= heat_work_doubles(m->m, d),
                "galerkin: work holds fewer doubles than nss_heat_workspace asks for");
    const int grid = galerkin_grid(m->m);
    hipStream_t st = as_stream(stream);
#define NSS_GALERKIN(D)                                                                                          \
  hipLaunchKernelGGL((galerkin_kernel<D>), dim3(grid), dim3(kBlock), 0, st, m->m, m->rowptr, m->col, m->val, ld, \
                     basis, work);
    NSS_HEAT_DISPATCH(d, NSS_GALERKIN)
#undef NSS_GALERKIN
    NSS_CHECK_LAUNCH();
    hipLaunchKernelGGL(galerkin_finish_kernel, dim3(d * d), dim3(kBlock), 0, st, work, grid, g);
    NSS_CHECK_LAUNCH();
  });
}

int nss_basis_combine_f64(int64_t n, int32_t d, int64_t ld, const double* basis, const double* h_coeff, double* y,
                          nss_stream_t stream) {
  return guarded([&] {
    require_basis("basis_combine", n, d, ld, basis);
    NSS_REQUIRE(h_coeff != nullptr && y != nullptr, "basis_combine: NULL coefficients or y");
    NSS_REQUIRE(aligned16(y), "basis_combine: y is not 16-byte aligned");
    CombineArgs co{};
    for (int i = 0; i < d; ++i) co.c[i] = h_coeff[i];
    const int grid = stream_grid((n + 1) / 2, kBlock);
    hipStream_t st = as_stream(stream);
#define NSS_COMBINE(D) hipLaunchKernelGGL((combine_kernel<D>), dim3(grid), dim3(kBlock), 0, st, n, ld, basis, co, y);
    NSS_HEAT_DISPATCH(d, NSS_COMBINE)
#undef NSS_COMBINE
    NSS_CHECK_LAUNCH();
  });
}

}  // extern "C"
