// The 1-D factors of the fast-diagonalisation solvers, read off a resident matrix (nss_fdm_gather_factors; DESIGN.md
// section 19).  `hipla.fdm.fdm_factors` takes the factor of axis a from the grid line through a component's origin,
// T_a[x, y] = A[line_a[x], line_a[y]]; with the matrix resident as an nss_csr_t that is a gather of e x e entries per
// axis, and only those are downloaded.  The layout is the one of the component handles (fdm_layout.h): entry (k, j, i)
// of component c sits at base_c + k * pitch + j * e_2 + i, so the line along the internal axis a is base_c + x * stride_a
// with the strides (pitch, e_2, 1).
//
// One lane per row of a line.  The lane walks the stored entries of its row and keeps those whose column lies on the
// same line: (column - base) is a multiple of the stride with a quotient below e.  For axis 1 the quotient y < e_1 keeps
// y * e_2 inside the first slab, and for axis 0 the multiples of the pitch are the slab origins: no other point of the
// component has such a column.  Stored zeros are skipped (T is zero on entry), duplicates are not summed.
#include <memory>

#include "csr_stream.h"
#include "fdm_layout.h"
#include "nss_common.h"

namespace nss {

constexpr int kFdmLines = kFdmcMaxComp * 3;

// line l holds the rows base + x * stride, x < e; its factor is e x e row-major from T + at
struct FdmLines {
  int32_t count;
  int32_t base[kFdmLines], stride[kFdmLines], e[kFdmLines];
  int32_t end[kFdmLines];                                  // running sum of e: the lanes of the lines
  int64_t at[kFdmLines];
};

__global__ __launch_bounds__(kBlock) void fdm_gather_kernel(FdmLines ln, const int32_t* __restrict__ rowptr,
                                                             const int32_t* __restrict__ col,
                                                             const double* __restrict__ val, double* __restrict__ T) {
  const int64_t t = int64_t(blockIdx.x) * kBlock + threadIdx.x;
  if (t >= ln.end[ln.count - 1]) return;
  int32_t l = 0;
  while (t >= ln.end[l]) ++l;
  const int32_t x = int32_t(t) - (l ? ln.end[l - 1] : 0);
  const int32_t base = ln.base[l], stride = ln.stride[l], e = ln.e[l];
  const int32_t g = base + x * stride;                     // (inside [0, n_total): fdm_layout_checked)
  double* row = T + ln.at[l] + int64_t(x) * e;
  for (int32_t p = rowptr[g], p1 = rowptr[g + 1]; p < p1; ++p) {
    const int32_t off = col[p] - base;
    const double a = val[p];
    if (off < 0 || a == 0.0) continue;
    const int32_t y = off / stride;
    if (y < e && y * stride == off) row[y] = a;
  }
}

}  // namespace nss

using namespace nss;

extern "C" {

int nss_fdm_gather_factors(nss_csr_t a, int32_t ncomp, int32_t dim, int64_t n_total, const int64_t* h_base, int64_t pitch,
                           const int64_t* h_extents, double* const* h_T_out, nss_stream_t stream) {
  return guarded([&] {
    NSS_REQUIRE(a && h_base && h_extents && h_T_out, "fdm_gather_factors: NULL argument");
    const FdmLayout lay = fdm_layout_checked("fdm_gather_factors", ncomp, dim, n_total, h_base, pitch, h_extents, h_T_out,
                                             h_T_out);
    require_f64_values(a, "fdm_gather_factors");
    NSS_REQUIRE(a->m == n_total && a->n == n_total,
                "fdm_gather_factors: the matrix is not n_total x n_total (" + std::to_string(a->m) + " x " +
                    std::to_string(a->n) + ", n_total " + std::to_string(n_total) + ")");
    FdmLines ln{};
    int64_t total = 0, rows = 0;
    for (int c = 0; c < ncomp; ++c)
      for (int k = 0; k < dim; ++k) {                      // the caller's axes, component-major: the order of h_T_out
        const int ia = fdm_internal_axis(dim, k), l = ln.count++;
        const int64_t e = lay.ext[c][ia];
        rows += e;
        NSS_REQUIRE(rows <= kFdmcMaxTotal, "fdm_gather_factors: the extents add up to more than 2^31 - 1");
        ln.base[l] = int32_t(lay.base[c]);
        ln.stride[l] = ia == 0 ? int32_t(lay.pitch) : ia == 1 ? lay.ext[c][2] : 1;
        ln.e[l] = int32_t(e);
        ln.end[l] = int32_t(rows);
        ln.at[l] = total;
        total += e * e;
      }
    hipStream_t st = as_stream(stream);
    DeviceBuffer<double> T{size_t(total)};
    NSS_HIP(hipMemsetAsync(T, 0, sizeof(double) * size_t(total), st));
    hipLaunchKernelGGL(fdm_gather_kernel, dim3(unsigned((rows + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, ln,
                       a->rowptr, a->col, a->val, T.get());
    NSS_CHECK_LAUNCH();
    NSS_HIP(hipStreamSynchronize(st));
    for (int l = 0; l < ln.count; ++l)
      NSS_HIP(hipMemcpy(h_T_out[l], T + ln.at[l], sizeof(double) * size_t(ln.e[l]) * size_t(ln.e[l]),
                        hipMemcpyDeviceToHost));
  });
}

}  // extern "C"
