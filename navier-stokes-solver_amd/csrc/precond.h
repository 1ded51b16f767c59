// Block-Jacobi handle shared by the preconditioner entry points and the fused loops.
#pragma once

#include "bjac_block.h"

#include <string>
#include <type_traits>
#include <vector>

struct nss_bjac_s {
  uint64_t serial = 0;         // unique per handle (matrices planned around its blocks remember it: nss_csr_s::jb_serial)
  int32_t bs = 0, nblocks = 0;
  int64_t n = 0;
  nss::DeviceBuffer<int32_t> idx;       // [bs][nblocks], -1 = padding
  nss::DeviceBuffer<int32_t> run;       // [nblocks]: run words (bjac_pack_run), when every block is a run of
                                        // consecutive dofs (4 bytes per block instead of 4 per dof)
  nss::DeviceBuffer<double> inv;        // [bs*bs][nblocks]
  nss::DeviceBuffer<double> inv_sym;    // [bs*(bs+1)/2][nblocks]: upper triangles, when every inverse block is
                                        // symmetric (A symmetric): the apply kernel then reads ~half the bytes
  // Block codes (nss_bjac_code_blocks): with at most 256 distinct inverse blocks -- compared as the 64-bit patterns
  // of the entries the apply kernel reads -- the apply streams one byte per block and holds the distinct blocks in LDS
  // (bjac_apply_coded_kernel); inv / inv_sym stay for every other reader.  Same doubles, same products.
  nss::DeviceBuffer<uint8_t> code;      // [nblocks]: the block's position in dict
  nss::DeviceBuffer<double> dict;       // [n_codes][dict_doubles]: the distinct blocks, entries ordered as in inv_sym / inv
  int32_t n_codes = 0, dict_doubles = 0;   // dict_doubles = bs (bs + 1) / 2 (inv_sym) or bs * bs (inv)
  nss::DeviceBuffer<int32_t> covered;   // dofs that belong to no block (count: n_uncovered)
  int32_t n_uncovered = 0;
  // multicolour Gauss-Seidel mode (nss_bjac_set_colors): blocks are stored colour-major
  const nss_csr_s* gs_mat = nullptr;      // rows of A permuted block by block, colour-major (the caller's handle)
  std::vector<int32_t> color_ptr;         // ncolors + 1 block offsets (host)
  std::vector<int32_t> color_rowblk;      // ncolors + 1 row-block offsets into gs_mat's launch plan (host)
  std::vector<int32_t> color_row;         // ncolors + 1 row offsets of the colours in the permuted numbering (host)
  nss::DeviceBuffer<int32_t> rowdof;      // device: original dof of permuted row r
  nss::DeviceBuffer<int32_t> ridx;        // device [bs][nblocks]: permuted row of a block entry, -1 = padding
  nss::DeviceBuffer<double> res;          // device: residual of the colour being swept (permuted rows)
  // Colour-major layout INSIDE the sweep (nss_bjac_set_colors_permuted): gs_mat is P A P^T -- rows and columns in the
  // colour-major block order; the dofs that belong to no block (`covered`, ascending) are the trailing columns
  // n_perm .. n_perm + n_uncovered - 1, gathered from y on every entry and never updated or scattered (with every dof
  // covered: one extra column n_perm without entries, 0) -- the iterate
  // and the right-hand side are gathered into that numbering once on entry (yt, xt) and the iterate is scattered back
  // once on exit; a colour is then ONE launch: the rows of the colour with the block solve in the epilogue (every
  // row block of gs_mat holds whole Gauss-Seidel blocks and at most kGsRows rows; the residuals of a row block pass
  // through LDS).  Everything a colour touches of its own is contiguous.
  bool gs_permuted = false;
  int32_t n_perm = 0;
  nss::DeviceBuffer<uint8_t> gpos;        // [n_perm] position of the row inside its block
  nss::DeviceBuffer<uint8_t> glen;        // [n_perm] rows of its block
  nss::DeviceBuffer<double> ginv;         // [bs][n_perm]: ginv[k][r] = (A_bb^-1)(row r, k-th row of the block)
  nss::DeviceBuffer<double> xt, yt;       // [n_perm + max(1, n_uncovered)]
  // Statically condensed form whose MypreA sweeps over the Schur complement S (nss_bjac_set_condensed): the operators
  // the fused BPCG loop folds into the sweep's entry, middle and exit (csrc/bpcg2.hip: the fused condensed forms).
  // cond_key_* = the operators they were made from (the loop uses them only for exactly those); cond_HTp = P H^T (the
  // rows of H^T at the block dofs in the colour-major numbering, original columns); cond_Hp = the rows of H at the
  // dofs outside every block (in `covered` order) with columns renamed into the permuted numbering (n_perm +
  // max(1, n_uncovered) columns); cond_dinner[i] = the diagonal of A_ii^-1 at covered[i].  The six matrices are the
  // caller's handles; only cond_dinner is this handle's memory.
  const nss_csr_s *cond_key_HT = nullptr, *cond_key_H = nullptr, *cond_key_inner = nullptr, *cond_key_S = nullptr;
  const nss_csr_s *cond_HTp = nullptr, *cond_Hp = nullptr;
  nss::DeviceBuffer<double> cond_dinner;
};

namespace nss {

constexpr int kMaxBs = 16;
// Largest dictionary of the coded apply: 160 KiB of LDS per CU over the 8 resident 256-lane workgroups of the uncoded
// kernel, less its static reduction scratch, rounded down to a power of two
constexpr int kBjacDictBytes = 16 << 10;
constexpr int kGsRows = 256;     // rows per row block of the permuted Gauss-Seidel matrix (their residuals: 2 KiB of LDS)

// f(std::integral_constant<int, bs>{}) for 1 <= bs <= kMaxBs: the block size as a template argument of what f launches
template <class F>
void with_block_size(int bs, const char* what, F&& f) {
  switch (bs) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    case 8: return f(std::integral_constant<int, 8>{});
    case 9: return f(std::integral_constant<int, 9>{});
    case 10: return f(std::integral_constant<int, 10>{});
    case 11: return f(std::integral_constant<int, 11>{});
    case 12: return f(std::integral_constant<int, 12>{});
    case 13: return f(std::integral_constant<int, 13>{});
    case 14: return f(std::integral_constant<int, 14>{});
    case 15: return f(std::integral_constant<int, 15>{});
    case 16: return f(std::integral_constant<int, 16>{});
    default: throw Error(std::string(what) + ": unsupported block size");
  }
}
// the same for a flag (the streaming-load argument of the apply kernels)
template <class F>
void with_bool(bool flag, F&& f) {
  if (flag) f(std::true_type{});
  else f(std::false_type{});
}

// y[dofs] = alpha * J x + beta * y[dofs]; returns immediately on the device when
// `done` (device int, may be NULL) is non-zero.
void bjac_apply(const nss_bjac_s& j, double alpha, const double* x, double beta, double* y, const int32_t* done,
                hipStream_t st);
// y = alpha * J x (dofs outside every block: 0) and, from the same registers, the per-workgroup
// partial sums of <y, x> into partials[0 .. bjac_dot_grid(j)); returns that count.  Block-Jacobi
// mode only.  Saves the separate dot pass (two vector reads and a launch) after the apply.
int bjac_dot_grid(const nss_bjac_s& j);
// whether bjac_apply / bjac_apply_dot launch the coded kernel for this handle (nss_bjac_block_code_mode)
bool bjac_coded(const nss_bjac_s& j);
int bjac_apply_dot(const nss_bjac_s& j, double alpha, const double* x, double* y, double* partials, const int32_t* done,
                   hipStream_t st);


// one multicolour block Gauss-Seidel sweep / the symmetric pair as an operator (y = 0 first)
// flags (colour-major layout; ignored by the row-permuted one):
//   kGsFromZero  y is taken to be 0 on entry and need not hold zeros: it is not gathered, and the first colour of the
//                sweep -- whose rows see A y = 0 -- is y_c = D_c^-1 (xscale x_c) without a pass over its rows of A
//   kGsKeepX     x is the vector of the previous call on this handle (its permuted copy is still there): not gathered again
enum { kGsFromZero = 1, kGsKeepX = 2 };
void bjac_smooth(const nss_bjac_s& j, double xscale, const double* x, double* y, bool backward, const int32_t* done,
                 hipStream_t st, int flags = 0);
void bjac_symgs_apply(const nss_bjac_s& j, double xscale, const double* x, double* y, const int32_t* done,
                      hipStream_t st);
// colour-major layout, for callers that fill / drain xt and yt themselves (the fused condensed forms of bpcg2.hip):
// one sweep over the permuted copies as they stand (from_zero: yt holds zeros on the rows, the first colour is solved
// without its pass over P A P^T), and the gather of y at the block dofs only (yt[r] = y[rowdof[r]], xt kept; the
// trailing columns are not gathered -- for callers whose P A P^T has no entries in them)
void bjac_sweep_permuted(const nss_bjac_s& j, double xscale, bool backward, const int32_t* done, hipStream_t st,
                         bool from_zero);
void bjac_gather_rows(const nss_bjac_s& j, const double* y, const int32_t* done, hipStream_t st);

}  // namespace nss
