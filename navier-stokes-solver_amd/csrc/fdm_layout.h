// The layout of the components of an interleaved vector, as the component handles of the fast diagonalisation take it
// (nss_fdmc_create, nss_fdmi_create): component c is an array over its extents whose entry (k, j, i) sits at
// base_c + k * pitch + j * e_2 + i.  What is said here once: the internal (always three) extents, the argument checks and
// the overlap arithmetic.  Host code in plain C++ -- no HIP call, no allocation -- so that a stand-alone program can run
// it under the host sanitizers (tools/fdm_layout_asan.cpp).  A refused argument throws with the text NSS_REQUIRE gives.
#pragma once

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>

namespace nss {

constexpr int kFdmcMaxComp = 3;
constexpr int64_t kFdmcMaxTotal = 2147483647;             // 2^31 - 1

struct FdmLayout {
  int ncomp = 0, dim = 0;
  int64_t n_total = 0, pitch = 0;
  int64_t base[kFdmcMaxComp] = {0, 0, 0};
  int32_t ext[kFdmcMaxComp][3] = {{1, 1, 1}, {1, 1, 1}, {1, 1, 1}};      // internal: (e_0, 1, e_1) for two axes
};

inline int64_t fdm_floor_div(int64_t a, int64_t b) {      // b > 0
  return a / b - ((a % b != 0) && (a < 0));
}

// the internal axis of the caller's axis a
inline int fdm_internal_axis(int dim, int a) { return dim == 3 ? a : 2 * a; }

inline void fdm_layout_require(bool ok, const std::string& msg) {
  if (!ok) throw std::invalid_argument("invalid argument: " + msg);
}

// The layout of (ncomp, dim, n_total, h_base, pitch, h_extents), checked; h_Q / h_lambda: the ncomp * dim factor
// pointers, checked against NULL only.  `who`: the entry point's name in front of every message.
inline FdmLayout fdm_layout_checked(const std::string& who, int32_t ncomp, int32_t dim, int64_t n_total,
                                    const int64_t* h_base, int64_t pitch, const int64_t* h_extents,
                                    const double* const* h_Q, const double* const* h_lambda) {
  fdm_layout_require(ncomp >= 1 && ncomp <= kFdmcMaxComp, who + ": ncomp is 1, 2 or 3");
  fdm_layout_require(dim == 2 || dim == 3, who + ": dim is 2 or 3");
  fdm_layout_require(n_total >= 1 && n_total <= kFdmcMaxTotal, who + ": n_total is not in 1 .. 2^31 - 1");
  fdm_layout_require(pitch >= 1 && pitch <= kFdmcMaxTotal, who + ": the pitch is not in 1 .. 2^31 - 1");
  FdmLayout h;
  h.ncomp = ncomp;
  h.dim = dim;
  h.n_total = n_total;
  h.pitch = pitch;
  int64_t slab[kFdmcMaxComp] = {0, 0, 0};                  // the entries of a component in one slab
  for (int c = 0; c < ncomp; ++c) {
    const std::string comp = who + ": component " + std::to_string(c);
    for (int a = 0; a < dim; ++a) {
      const int64_t e = h_extents[c * dim + a];
      fdm_layout_require(e >= 1 && e <= n_total, comp + ": an extent is not in 1 .. n_total");
      fdm_layout_require(h_Q[c * dim + a] && h_lambda[c * dim + a], comp + ": NULL factor");
      h.ext[c][fdm_internal_axis(dim, a)] = int32_t(e);
    }
    h.base[c] = h_base[c];
    slab[c] = int64_t(h.ext[c][1]) * h.ext[c][2];          // (below 2^62)
    fdm_layout_require(h.ext[c][0] == 1 || slab[c] <= pitch, comp + ": a slab of it is longer than the pitch");
    fdm_layout_require(h_base[c] >= 0 && slab[c] <= n_total && h_base[c] <= n_total - slab[c] &&
                           (h.ext[c][0] - 1) * pitch <= n_total - slab[c] - h_base[c],
                       comp + " does not fit inside [0, n_total)");
  }
  // two components overlap when slab ka of a and slab kb = ka + m of b do: -slab_b < (base_b - base_a) + m pitch < slab_a
  for (int a = 0; a < ncomp; ++a)
    for (int b = a + 1; b < ncomp; ++b) {
      const int64_t d = h.base[b] - h.base[a];
      const int64_t lo = std::max<int64_t>(-(h.ext[a][0] - 1), -fdm_floor_div(slab[b] - 1 + d, pitch));
      const int64_t hi = std::min<int64_t>(h.ext[b][0] - 1, fdm_floor_div(slab[a] - 1 - d, pitch));
      fdm_layout_require(lo > hi, who + ": components " + std::to_string(a) + " and " + std::to_string(b) + " overlap");
    }
  return h;
}

}  // namespace nss
