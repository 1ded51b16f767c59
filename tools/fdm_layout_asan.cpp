// Stand-alone check of the host code behind nss_fdmi_create and nss_fdmc_create: the argument checks and the overlap
// arithmetic of csrc/fdm_layout.h, meant to be built with the host sanitizers and run on the CPU,
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I navier-stokes-solver_amd/csrc
//       tools/fdm_layout_asan.cpp -o fdm_layout_asan && ./fdm_layout_asan
//
// (with hipcc: -Xarch_host -fsanitize=address,undefined).  The arrays handed in are heap allocations of exactly the
// length the entry points document, so a read past ncomp or ncomp * dim entries is caught; the extents and pitches go
// up to 2^31 - 1, where a careless product would overflow.  Prints "layout checks ok" and returns 0, or says which case
// went wrong and returns 1.
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "fdm_layout.h"

namespace {

struct Case {
  int32_t ncomp, dim;
  int64_t n_total, pitch;
  std::vector<int64_t> base, ext;
  int null_factor = -1;                  // this factor pointer is NULL
};

int failures = 0;

// runs the check on exact-length heap copies; returns the message of the refusal ("" when accepted)
std::string run(const Case& c, nss::FdmLayout* out = nullptr) {
  const size_t nf = size_t(c.ncomp > 0 ? c.ncomp : 0) * size_t(c.dim > 0 ? c.dim : 0);
  std::unique_ptr<int64_t[]> base(new int64_t[c.base.size()]), ext(new int64_t[c.ext.size()]);
  for (size_t i = 0; i < c.base.size(); ++i) base[i] = c.base[i];
  for (size_t i = 0; i < c.ext.size(); ++i) ext[i] = c.ext[i];
  static const double one = 1.0;
  std::unique_ptr<const double*[]> q(new const double*[nf ? nf : 1]), lam(new const double*[nf ? nf : 1]);
  for (size_t i = 0; i < nf; ++i) {
    q[i] = &one;                          // (never dereferenced by the checks)
    lam[i] = int(i) == c.null_factor ? nullptr : &one;
  }
  try {
    const nss::FdmLayout lay = nss::fdm_layout_checked("fdmi_create", c.ncomp, c.dim, c.n_total, base.get(), c.pitch,
                                                       ext.get(), q.get(), lam.get());
    if (out) *out = lay;
    return "";
  } catch (const std::exception& e) {
    return e.what();
  }
}

void accept(const char* name, const Case& c, nss::FdmLayout* out = nullptr) {
  const std::string why = run(c, out);
  if (!why.empty()) {
    std::printf("FAILED %s: refused with \"%s\"\n", name, why.c_str());
    ++failures;
  }
}

void refuse(const char* name, const Case& c, const char* word) {
  const std::string why = run(c);
  if (why.find(word) == std::string::npos || why.find("fdmi_create") == std::string::npos) {
    std::printf("FAILED %s: wanted a refusal with \"%s\", got \"%s\"\n", name, word, why.c_str());
    ++failures;
  }
}

}  // namespace

int main() {
  const int64_t top = nss::kFdmcMaxTotal;
  // the staggered grid in 3-D, n = 4: components (4, 4, 5), (4, 5, 4), (5, 4, 4) interleaved per slab
  Case grid{3, 3, 5 * 60, 60, {0, 20, 40}, {4, 4, 5, 4, 5, 4, 5, 4, 4}};
  grid.n_total = 4 * 60 + 16 + 40;                       // the last component has a fifth slab of 16 entries
  nss::FdmLayout lay;
  accept("3-D grid", grid, &lay);
  if (lay.ext[2][0] != 5 || lay.ext[0][2] != 5 || lay.pitch != 60 || lay.base[1] != 20) {
    std::printf("FAILED 3-D grid: wrong layout\n");
    ++failures;
  }
  Case two{2, 2, 45, 9, {0, 5}, {4, 5, 5, 4}};           // 2-D: (e_0, 1, e_1) internally
  accept("2-D grid", two, &lay);
  if (lay.ext[0][0] != 4 || lay.ext[0][1] != 1 || lay.ext[0][2] != 5) {
    std::printf("FAILED 2-D grid: wrong internal extents\n");
    ++failures;
  }
  accept("one entry", Case{1, 2, 1, 1, {0}, {1, 1}});
  accept("one line at the top", Case{1, 2, top, top, {0}, {1, top}});
  accept("one column at the top", Case{1, 2, top, 1, {0}, {top, 1}});
  accept("two slabs, the widest pitch", Case{1, 2, top, top - 1, {0}, {2, 1}});
  accept("touching components", Case{2, 2, 12, 6, {0, 3}, {2, 3, 2, 3}});
  accept("interleaved behind one another", Case{2, 2, top, top / 2, {0, 1}, {2, 1, 2, 1}});

  refuse("ncomp 0", Case{0, 2, 4, 2, {}, {}}, "ncomp");
  refuse("ncomp 4", Case{4, 2, 64, 2, {0, 1, 2, 3}, {1, 1, 1, 1, 1, 1, 1, 1}}, "ncomp");
  refuse("dim 1", Case{1, 1, 4, 2, {0}, {4}}, "dim");
  refuse("dim 4", Case{1, 4, 16, 2, {0}, {2, 2, 2, 2}}, "dim");
  refuse("n_total 0", Case{1, 2, 0, 2, {0}, {1, 1}}, "n_total");
  refuse("n_total 2^31", Case{1, 2, top + 1, 2, {0}, {1, 1}}, "n_total");
  refuse("pitch 0", Case{1, 2, 4, 0, {0}, {2, 2}}, "pitch");
  refuse("pitch 2^31", Case{1, 2, 4, top + 1, {0}, {2, 2}}, "pitch");
  refuse("extent 0", Case{1, 2, 4, 2, {0}, {0, 2}}, "extent");
  refuse("extent above n_total", Case{1, 2, 4, 2, {0}, {5, 1}}, "extent");
  refuse("extents whose product overflows 32 bits", Case{1, 3, top, top, {0}, {2, 65536, 65536}}, "pitch");
  refuse("slab longer than the pitch", Case{1, 2, 12, 2, {0}, {2, 3}}, "pitch");
  refuse("negative base", Case{1, 2, 4, 2, {-1}, {2, 2}}, "fit");
  refuse("past the end", Case{1, 2, 4, 2, {1}, {2, 2}}, "fit");
  refuse("the last slab past the end", Case{1, 2, top, top - 1, {1}, {2, 2}}, "fit");
  refuse("base near 2^63", Case{1, 2, 4, 2, {INT64_MAX}, {1, 1}}, "fit");
  Case null_factor = two;
  null_factor.null_factor = 3;
  refuse("NULL factor", null_factor, "NULL factor");
  refuse("same place", Case{2, 2, 12, 6, {0, 0}, {2, 3, 2, 3}}, "overlap");
  refuse("overlap by one entry", Case{2, 2, 12, 6, {0, 2}, {2, 3, 2, 3}}, "overlap");
  refuse("overlap in a later slab", Case{2, 2, 20, 6, {0, 7}, {3, 3, 2, 3}}, "overlap");
  refuse("overlap from behind", Case{2, 2, 20, 6, {7, 0}, {2, 3, 3, 3}}, "overlap");
  refuse("overlap of the third with the first", Case{3, 2, 30, 9, {0, 3, 11}, {3, 3, 3, 3, 2, 3}}, "overlap");
  refuse("overlap at the top", Case{2, 2, top, top / 2, {0, top / 2}, {2, 1, 2, 1}}, "overlap");

  if (failures == 0) std::printf("layout checks ok\n");
  return failures == 0 ? 0 : 1;
}
