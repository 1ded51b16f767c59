// CSR-stream SpMV kernel template for gfx950 (fp64 values, int32 indices).
//
// The Stokes blocks have short rows (7 / 6 / 2 non-zeros for A / B / B^T on the MAC
// grid, ~25-84 for HDG-like operators), so a row-per-wave kernel would idle most of
// its 64 lanes.  Instead a 256-thread workgroup owns a contiguous *row block* whose
// non-zeros fit one LDS chunk:
//   phase 1  every lane streams val[] / col[] with unit stride (fully coalesced HBM
//            reads, 8 independent loads in flight per lane), takes x[col] -- from an LDS copy of
//            the row block's operand segments (staged form, below) or by a gather served by
//            L2 / Infinity Cache -- and stages the products in LDS;
//   phase 2  each row is reduced from LDS by RG lanes (RG = 1 ... 64, a power of two chosen from
//            the mean row length) with a __shfl_xor butterfly, in a fixed order -- no
//            atomics, bit-reproducible;
//   epilogue a functor consumes (row, A x) -- plain alpha/beta update or the fused
//            vector updates + dot partials of the Krylov loops -- so y is written once
//            and the extra vectors are read while the row is still in registers.
// Row blocks are precomputed on the host when the matrix is uploaded; one workgroup per row
// block.  The
// blockIdx -> row-block map is XCD-aware: workgroups b and b+8 share an XCD (round-robin
// dispatch), so XCD i walks its own contiguous eighth of the rows and its private 4 MiB
// L2 keeps one window of x instead of all eight L2s caching the same window.
// Host side: launch_csr<FORMS> (one matrix), launch_csr_dual<FORMS> (two matrices in one launch) pick the instantiation
// -- value form, kernel, column form, lanes per row -- for a matrix; every launch of the library goes through them.
// Two further kernel forms serve short rows, one lane per row and no product buffer: csr_direct_kernel (at most two
// entries per row, gathered operand; launch_csr takes it by itself) and csr_slots_kernel (coded matrices with at most
// eight entries per row, staged operand; launch_csr_slots / launch_csr_slots_dual, asked for by two launch sites).
#pragma once

#include <type_traits>
#include <vector>

#include "nss_common.h"
#include "packed_rows.h"

#include <initializer_list>
#include <string>

namespace nss {

// Non-temporal loads for the col/val streams: they are read exactly once, and keeping them
// out of the 4-MiB XCD L2s leaves room for the gathered x window.  Measured on the 1e7-DoF
// case (interleaved A/B, one box): plain A SpMV 0.173 -> 0.163 ms, BPCG iteration +4 %.
#ifndef NSS_STREAM_NT
#define NSS_STREAM_NT 1
#endif

#ifndef NSS_STREAM_PREFETCH
#define NSS_STREAM_PREFETCH 1   // request row bounds + epilogue operands before the matrix stream
#endif

#ifndef NSS_PREFETCH_ROWS
#define NSS_PREFETCH_ROWS 1     // phase-2 rows per lane whose bounds and epilogue operands are requested up front (RG == 1)
#endif

#ifndef NSS_CHUNK
#define NSS_CHUNK 2048
#endif
constexpr int kChunk = NSS_CHUNK;       // products staged per workgroup: 16 KiB of LDS
// (Round 1 staged 4096 products for matrices with >= 32 non-zeros per row: with the gathered operand that was
// worth +5 % at 82 non-zeros per row.  With the staged operand the short chunk wins -- 16 KiB of LDS and ~56
// VGPRs keep 8 workgroups per CU: plain SpMV 0.346 -> 0.309 ms = 6.7 TB/s, C23 -7 % at 82 non-zeros per row,
// profiles/r02_ab_chunk.txt -- and there is one chunk size again.)
constexpr int kMaxRowsPerBlock = 2048;  // bound for blocks of empty / very short rows
constexpr int kXcds = 8;
constexpr int kWindows = 16;          // column windows per row block of the 16-bit index stream
constexpr int kWindowBits = 12;      // 4096 columns per window
#ifndef NSS_DIRECT_ROWS
#define NSS_DIRECT_ROWS 1
#endif
constexpr int kDirectWidth = 2;        // entries per row of the fixed-width copy (csr_direct_kernel)
#ifndef NSS_DIRECT_ROWS_PER_LANE
#define NSS_DIRECT_ROWS_PER_LANE 2
#endif
constexpr int kDirectRows = NSS_DIRECT_ROWS_PER_LANE * 256;   // rows per row block of such a matrix
constexpr int kSlotWidth = 8;          // entries per row of the row-slot copy (csr_slots_kernel)
constexpr unsigned kSlotPad = 0xffffu; // staged position of an unused slot in the 24-byte layout of the copy
static_assert(kChunk <= int(kPackedPosLimit), "the packed row slots hold staged positions of 11 bits");
// Staged operand (nss_csr_s::blkseg): per row block at most kSegMax runs of consecutive columns, together at
// most `chunk` columns (the LDS copy shares the product buffer), copied to LDS by LDS-DMA ahead of the matrix
// stream.
constexpr int kSegMax = 13;
constexpr int kSegWords = 32;        // descriptor: r0, r1, p0, cnt, nseg, total, pre[1..12], off[0..12], spare
constexpr int kSegPre = 6, kSegOff = 18;
constexpr int kSegBlock = 31;        // dispatch-ordered copy of the table: the row block this slot stands for

bool pair_staging_enabled();     // nss_csr_pair_mode (tests, measurements)
bool value_codes_enabled();      // nss_csr_value_code_mode != 0

// Value type of a coded matrix (nss_csr_s::val8): the stream is one byte per entry, the index of the entry's value in
// a dictionary of at most kDictSize doubles that the kernel holds in LDS.  Same doubles, same products.
struct Coded8 {};
constexpr int kDictSize = 256;
// The distinct-pattern collector of the codes (spmv.hip), also run over the block hashes of nss_bjac_code_blocks: the
// ascending distinct 64-bit patterns of val[0 .. n) (false at the 257th), and the position of every entry's pattern
// among them.  Set-up only; both synchronise the stream.
bool collect_patterns(int64_t n, const double* val, std::vector<unsigned long long>& keys, hipStream_t st);
void assign_pattern_codes(int64_t n, const double* val, const std::vector<unsigned long long>& keys, uint8_t* codes,
                          hipStream_t st);

struct CsrView {
  const int32_t* __restrict__ rowblk;
  const int32_t* __restrict__ rowptr;
  const int32_t* __restrict__ col;
  const uint16_t* __restrict__ col16;   // the 16-bit stream of `mode` (window-relative columns or staged positions), or NULL
  const int32_t* __restrict__ blkbase;  // kWindows window bases per row block (mode 1)
  const int32_t* __restrict__ blkseg;   // kSegWords per row block (mode 2)
  const int32_t* __restrict__ blkdisp;  // the same descriptors in DISPATCH order (8 x per_xcd slots, word kSegBlock = the
                                        // row block, -1 in padding slots), or NULL: slot lb is row block blk0 + lb
  const double* __restrict__ val;
  uint32_t gb;      // entries per column group of the 16-bit stream (1: one index per entry)
  uint32_t gstep, sstep;   // kBlock / gb, kBlock % gb: a lane's next entry is kBlock further down the stream
  uint64_t gmagic;  // ceil(2^64 / gb) (gb > 1): p / gb == __umul64hi(p, gmagic) for p < 2^32
  int32_t blk0;     // first row block of this launch (sub-range launches: interior / boundary)
  int32_t nblk;     // row blocks in this launch
  int32_t per_xcd;  // ceil(nblk / 8)
  int32_t mode;     // how the operand is reached: 0 = 4-byte columns, gather; 1 = 16-bit window-relative columns,
                    // gather; 2 = staged (LDS copy of the row block's operand segments, 16-bit positions);
                    // 3 = pair-staged (the segments of TWO vectors, each in one half of the LDS buffer)
  const float* __restrict__ val32;      // the 4-byte value stream of a narrowed matrix (nss_csr_s::val32), else NULL
  const uint8_t* __restrict__ val8;     // the 1-byte value codes of a coded matrix (nss_csr_s::val8), else NULL
  const double* __restrict__ dict;      // ... and its kDictSize values
};

// the value stream of a view as the kernels' value type VT (double: `val`; float: `val32`, widened before the product)
template <class VT>
struct StoredValue { using type = VT; };
template <>
struct StoredValue<Coded8> { using type = uint8_t; };
template <class VT>
__device__ __forceinline__ const typename StoredValue<VT>::type* view_values(const CsrView& a) {
  static_assert(std::is_same<VT, double>::value || std::is_same<VT, float>::value || std::is_same<VT, Coded8>::value,
                "values are fp64, fp32 or codes");
  if constexpr (std::is_same<VT, float>::value) return a.val32;
  else if constexpr (std::is_same<VT, Coded8>::value) return a.val8;
  else return a.val;
}
// a stored value as the double that enters the product (`dict`: the LDS copy of the dictionary, coded form only)
template <class VT>
__device__ __forceinline__ double value_of(typename StoredValue<VT>::type v, const double* dict) {
  if constexpr (std::is_same<VT, Coded8>::value) return dict[v];
  else return double(v);
}
// The LDS copy of the dictionary: static storage of the coded instantiations only (2 KiB beside the 16-KiB product
// buffer: 8 workgroups per CU still fit the 160 KiB).
template <class VT>
struct DictLds {
  static __device__ __forceinline__ double* get() { return nullptr; }
  static __device__ __forceinline__ void request(const CsrView&, double*) {}
};
typedef __attribute__((address_space(3))) void* LdsDst;
typedef const __attribute__((address_space(1))) void* GlobalSrc;
template <>
struct DictLds<Coded8> {
  static __device__ __forceinline__ double* get() {
    __shared__ alignas(16) double dict[kDictSize];         // (destination of 16-byte LDS-DMA)
    return dict;
  }
  // dictionary -> LDS by LDS-DMA (no VGPR destination: nothing for the register allocator to recycle in the middle of
  // the matrix stream): waves 0 and 1 move 64 x 16 bytes each.  Requested AHEAD of the matrix stream; the caller
  // waits for vmcnt(0) and passes a barrier before the first read.
  static __device__ __forceinline__ void request(const CsrView& a, double* dict) {
    const int wave = int(threadIdx.x) / 64, lane = int(threadIdx.x) % 64;
    if (wave < kDictSize / 128)
      __builtin_amdgcn_global_load_lds((GlobalSrc)(a.dict + wave * 128 + 2 * lane), (LdsDst)(dict + wave * 128), 16, 0, 0);
  }
};

}  // namespace nss

struct nss_csr_s {
  int32_t m = 0, n = 0;
  int64_t nnz = 0;
  nss::DeviceBuffer<int32_t> rowptr;
  nss::DeviceBuffer<int32_t> col;
  nss::DeviceBuffer<double> val;
  nss::DeviceBuffer<int32_t> rowblk;
  int32_t nblk = 0;
  int32_t rg = 1;
  int32_t chunk = nss::kChunk;   // products the kernels' LDS buffer holds (the template parameter CH)
  int32_t blk_products = nss::kChunk;   // products per row block the launch plan aims at (<= chunk; nss_csr_plan_for_pairs)
  std::vector<int32_t> cuts;     // row positions no row block spans (kept for re-planning)
  // Launch-plan generation: 0 for the plan made at upload; every re-plan (nss_csr_plan_for_pairs / _for_blocks, the
  // joint AMG cycle of nss_amg_create_auxiliary) takes the next value of ONE process-wide counter, so the largest
  // generation among the matrices of a loop state changes exactly when one of them was re-planned (plan_stamp).
  int64_t plan_gen = 0;
  // Compressed column stream: when the columns of every row block fall into at most 16 aligned
  // windows of 4096 columns (grid operators: a row block touches its own grid plane and the two
  // neighbouring ones -- a few narrow clusters far apart) the kernel streams 2 bytes per entry,
  // 4 bits of window number + 12 bits of offset, decoded through the block's 16 window bases
  // (held in LDS), instead of the 4-byte index: 2 bytes per non-zero less HBM traffic, same
  // products in the same order.  `col` is kept for the set-up kernels and rows longer than a chunk.
  nss::DeviceBuffer<uint16_t> col16;
  nss::DeviceBuffer<int32_t> blkbase;
  // Staged operand (preferred where the kernel's operand is one stored vector).  Measured on gfx950
  // (tools/spmv_probe.py, profiles/r02_gather_probe.txt): what keeps the stream kernel at ~5 TB/s is not the
  // bytes of the x gather but the gather itself, a second round of per-lane loads that can only be issued when
  // the column stream has arrived -- with the operand read from LDS instead, the same kernel streams 6.2 TB/s at
  // 7 and at 82 non-zeros per row.  So: when the columns a row block touches form at most kSegMax runs of
  // consecutive columns (gaps of up to 7 unused columns are bridged) with at most kStageCap columns in total --
  // grid operators: one run per stencil leg; block-structured operators: the block columns of a few block rows
  // -- `blkseg` holds the runs and pos16 holds, per entry, the POSITION of its column in the concatenation of
  // the runs.  The kernel copies the runs from x into LDS by LDS-DMA (global_load_lds_dwordx4: 1 KiB per wave
  // instruction, no VGPR destination), issued BEFORE the matrix stream (the copy does not depend on it), and
  // reads the operand from LDS: no window decode, no dependent gather.  Same products, same order, same results.
  // A matrix is staged only when every one of its row blocks fits.  The window form is kept beside it for
  // kernels whose operand is an expression of two vectors (they gather).
  nss::DeviceBuffer<uint16_t> pos16;
  nss::DeviceBuffer<int32_t> blkseg;
  // Reuse-aware dispatch order (grid operators beyond ~1e7 rows).  XCD i walks its contiguous eighth of the row
  // blocks; the operand runs a block stages besides its own neighbourhood -- the grid planes above and below --
  // are staged again by the blocks P positions further down the walk (P = row blocks per plane).  Up to ~200
  // positions the XCD's 4-MiB L2 still holds them; beyond (5e7 DoF: P ~ 550) every such run comes from HBM a
  // second and a third time (PMC: the dominant launch drew 1.17 x its algorithmic bytes).  `blkdisp` is a copy of
  // the descriptor table in an order that visits the blocks b, b + P, b + 2P, ... of T consecutive planes back to
  // back, then b + 1, b + 1 + P, ...: the re-reads are adjacent in time.  Only the workgroup -> row block map
  // changes: per-row sums and the per-block dot-partial slots, hence all bits, stay.  Built at upload from the run
  // starts (spmv.hip: build_dispatch); full-range launches of the staged forms use it.
  nss::DeviceBuffer<int32_t> blkdisp;
  double disp_period = 0.0;      // P (row blocks), 0: natural order
  int32_t disp_planes = 0;       // T
  // Pair-staged operand: kernels whose operand is an expression of TWO stored vectors (t1 - s0 in the rows of B,
  // beta s1 + w1 in the rows of B^T) copy the segments of both -- the first to the lower half of the LDS buffer, the
  // second to the upper half -- and combine what they read back.  Possible when the segments of every row block hold
  // at most chunk / 2 columns (`pair_ok`); nss_csr_plan_for_pairs re-plans a matrix with shorter row blocks to get there.
  bool pair_ok = false;
  // Grouped column stream (block-structured operators: the facet blocks of the HDG-like spaces, ~84
  // non-zeros per row in runs of 12 consecutive columns): when every row length is a multiple of `gb`
  // and every aligned group of `gb` consecutive entries has consecutive columns, col16 / pos16 hold ONE 16-bit
  // index per group -- 8 + 2/gb bytes per non-zero instead of 10 -- and entry p has column (position)
  // decode(index[p / gb]) + p % gb.  The value order stays CSR (rows contiguous), so the kernel, its
  // reduction order and its results are unchanged.  gb == 1: one index per entry.
  int32_t gb = 1;
  // Fixed-width copy of a large matrix with at most kDirectWidth entries per row (B^T of the staggered grid):
  // kDirectWidth (column, value) slots per row, column -1 in unused slots.  Such a matrix is multiplied by
  // csr_direct_kernel: one lane per row, no LDS staging, every load of a lane's rows requested up front -- the
  // stream kernel spends most of a 2-entry-per-row launch in its per-row phase (1024 rows per workgroup, four
  // passes, the epilogue's loads of each pass behind the previous one's stores).
  nss::DeviceBuffer<int32_t> ell_col;
  nss::DeviceBuffer<double> ell_val;
  // Row blocks planned around the blocks of ONE block-Jacobi handle (nss_csr_plan_for_blocks: every row block holds
  // whole Jacobi blocks and at most kBlockRows rows): a kernel over the rows of this matrix can then apply that
  // preconditioner to its own result in the epilogue -- the row block's results pass through LDS, lanes take one
  // Jacobi block each (the fused BPCG loop: t1 = k J t0 inside C1, no launch of its own and no re-read of t0).
  // jb_order = the Jacobi blocks in row order (callers number them as they like); jb_first[b] = position in jb_order of
  // the first Jacobi block of row block b (nblk + 1 entries); jb_serial = nss_bjac_s::serial of that handle.
  nss::DeviceBuffer<int32_t> jb_first;
  nss::DeviceBuffer<int32_t> jb_order;
  // Fixed-width copy for EPILOGUE use (nss::fixed_width_copy, built on first request): the kDirectWidth (column,
  // value) slots per row of a matrix with at most that many entries per row, whatever its size -- a kernel over the
  // rows of ANOTHER matrix with the same row count can then add this matrix's row product from registers (fused
  // MINRES: B^T z1 inside the rows of A).  fw_col / fw_val are views, not owners: of ell_col / ell_val when those
  // exist, else of fw_own_col / fw_own_val, the handle's own copy.  fw_state: 0 not tried, 1, -1.
  const int32_t* fw_col = nullptr;
  double* fw_val = nullptr;
  nss::DeviceBuffer<int32_t> fw_own_col;
  nss::DeviceBuffer<double> fw_own_val;
  int fw_state = 0;
  // fp32 value storage (nss_csr_narrow_f32): the values rounded once to fp32 and stored 4 bytes wide in `val32`; `val`
  // is then NULL.  Only the kernel paths instantiated for it take such a matrix (launch_csr with kF32, the joint AMG
  // cycle); every other path refuses it (view() without `narrow_ok`, require_f64_values) -- none reads it as doubles.
  nss::DeviceBuffer<float> val32;
  // Value codes (nss_csr_code_values): a matrix with at most kDictSize distinct 64-bit value patterns -- every operator
  // of a uniform grid has a handful -- also holds val8, one byte per entry in CSR order (padded like `val`), and `dict`,
  // the kDictSize doubles the codes index (sorted by bit pattern, unused slots 0).  The kernels instantiated for it
  // (value type Coded8) stream 1 byte per entry instead of 8 and multiply dict[code] * x: the same doubles, the same
  // products in the same order.  `val` STAYS: every set-up path and every kernel without a coded form reads it, and the
  // codes are per entry in CSR order, so re-plans keep them.  ell_code: the two slots' codes of the fixed-width copy,
  // one 16-bit word per row (slot 0 in the low byte), built with ell_col.  Writers of `val` drop the codes.
  nss::DeviceBuffer<uint8_t> val8;
  nss::DeviceBuffer<double> dict;
  nss::DeviceBuffer<uint16_t> ell_code;
  int32_t dict_count = 0;
  // 16-bit columns of the coded fixed-width copy (built with ell_code when EVERY row block's live columns span at most
  // 65534): ell_col16 holds one word per row, both columns as offsets from ell_base[b], the smallest live column of row
  // block b (packed_rows.h).  The coded row-per-lane kernel then streams 6 bytes per row instead of 10; ell_col stays
  // for every other reader.  Belongs to one launch plan (the bases are per row block) and goes with ell_col.
  // ell16_state -1: refused by the caller (nss_csr_narrow_direct_columns), later builds leave the handle alone.
  nss::DeviceBuffer<uint32_t> ell_col16;
  nss::DeviceBuffer<int32_t> ell_base;
  int ell16_state = 0;
  bool direct_col16() const { return ell_col16 != nullptr && ell_base != nullptr && ell_code != nullptr && coded(); }
  // Row slots (nss_csr_plan_row_slots): the eight-slot copy of a coded, staged matrix whose rows hold at most
  // kSlotWidth entries, for the row-per-lane kernel of the staged operand (csr_slots_kernel).  Per row one aligned
  // 16-byte word in slot_pos and one 4-byte word in slot_code, together the packed row of packed_rows.h (slot_packed):
  // eight 11-bit staged positions (the values of pos16, CSR entry order), the row length and the eight value codes, 20
  // bytes per row where the CSR streams take 3 len + 4.  nss_csr_plan_row_slots(3) builds the copy in the 24-byte
  // layout instead (measurements, tests): the 16-byte word holds eight 16-bit positions, kSlotPad in unused slots, and
  // slot_code one 8-byte word of codes per row.  The
  // positions are relative to the operand runs of ONE launch plan: slot_gen is the plan generation the copy was built
  // for, replan() frees it, and a launcher takes it only through row_slots().  slot_state -1: refused by the caller
  // (mode 0), automatic requests leave the handle alone.
  nss::DeviceBuffer<uint16_t> slot_pos;
  nss::DeviceBuffer<uint8_t> slot_code;
  int64_t slot_gen = -1;
  int slot_state = 0;
  bool slot_packed = false;
  uint64_t jb_serial = 0;
  // the kernels with a coded form take it (the grouped column streams have none: nss_csr_code_values refuses such a
  // matrix, and one that a re-plan groups later reads `val` again and reports so)
  bool coded() const { return val8 != nullptr && gb == 1 && nss::value_codes_enabled(); }
  // a copy built for the current launch plan whose codes the kernels may read: the row-slot kernels take the matrix
  bool row_slots() const {
    return slot_pos != nullptr && slot_gen == plan_gen && coded() && blkseg && !ell_col && !val32 && !blkdisp && rg == 1;
  }
  // `stageable`: the kernel's operand functor is one stored vector that can be copied to LDS (XOp::kStageable);
  // `pairable`: it is an expression of two (XOp::kStageablePair)
  int idx_mode(bool stageable = true, bool pairable = false) const {
    if (blkseg && stageable) return 2;
    if (blkseg && pairable && pair_ok && nss::pair_staging_enabled()) return 3;
    return col16 ? 1 : 0;
  }
  // launch view of the row blocks [b0, b1)
  nss::CsrView view(int b0, int b1, int mode, bool narrow_ok = false) const {
    if (val32 && !narrow_ok)
      throw nss::Error("invalid argument: this kernel path has no form for a matrix with fp32 values (nss_csr_narrow_f32)");
    const uint64_t magic = gb > 1 ? ~uint64_t(0) / uint64_t(gb) + 1 : 0;    // ceil(2^64 / gb)
    const bool full = b0 == 0 && b1 == nblk;
    return nss::CsrView{rowblk, rowptr, col, mode >= 2 ? pos16 : (mode == 1 ? col16 : nullptr), blkbase, blkseg,
                        (mode >= 2 && full) ? blkdisp : nullptr, val,
                        uint32_t(gb), uint32_t(nss::kBlock / gb), uint32_t(nss::kBlock % gb), magic, b0, b1 - b0,
                        (b1 - b0 + nss::kXcds - 1) / nss::kXcds, mode, val32, val8, dict};
  }
  // one workgroup per row block, padded to a multiple of the XCD count
  static int grid(int count) { return ((count + nss::kXcds - 1) / nss::kXcds) * nss::kXcds; }
};

namespace nss {

// set-up paths that read the values as doubles (transpose, products, permutations, AMG set-up, block inverses, ...)
inline void require_f64_values(const nss_csr_s* a, const char* who) {
  if (a != nullptr && a->val32 != nullptr)
    throw Error(std::string("invalid argument: ") + who + ": the matrix stores fp32 values (nss_csr_narrow_f32); this path "
                "takes fp64 matrices only");
}

// Build col16 / blkbase of a matrix whose device arrays and launch plan are complete (spmv.hip).
void compress_columns(nss_csr_s& A, hipStream_t st);

bool direct_rows_candidate(int32_t m, const int32_t* rowptr);

// the fixed-width copy of A for epilogue use (see nss_csr_s::fw_col); false when a row has more than kDirectWidth entries
bool fixed_width_copy(nss_csr_s& A);

// New launch plan with at most `products` products per row block (set-up only: synchronises the device and rebuilds
// every derived column stream); per-row sums keep their bits.
void replan_row_blocks(nss_csr_s& A, int products);

// Launch plan of a CSR matrix: lanes per row (*rg_out) and the row-block boundaries (spmv.hip).
// `products`: products per row block to aim at (<= kChunk; the lanes-per-row choice does not depend on it, so the
// per-row sums of a re-planned matrix keep their bits)
// `max_rows` > 0: at most that many rows per row block; `row_pos` (one byte per row, host): a row block may only
// start at a row with row_pos == 0 (rows that belong together -- the dofs of one Gauss-Seidel block -- stay in one
// workgroup)
void plan_row_blocks(int32_t m, int64_t nnz, const int32_t* rowptr, int32_t* rg_out, int32_t* chunk_out,
                     std::vector<int32_t>& blk, const int32_t* cuts = nullptr, int ncuts = 0, int products = kChunk,
                     int max_rows = 0, const uint8_t* row_pos = nullptr);

// Epi interface:
//   __device__ void row(int r, double ax);          // called once per row by one lane
// or, to have the row's read-only operands requested before the matrix stream,
//   struct Pre;  __device__ Pre fetch(int r) const;
//   __device__ void row(int r, double ax, const Pre&);
//   __device__ void finish(int b, double* lds);     // called by all threads at the end; b = row
//                                                   // block of this workgroup (-1: padding), the
//                                                   // slot of its dot partial
//   __device__ bool skip() const;                   // e.g. solver already converged
// optional:
//   __device__ bool prologue(double* lds);          // called by ALL threads of the workgroup before the
//                                                   // stream (lds: 32 doubles): e.g. sum the dot partials of
//                                                   // the previous kernel and derive alpha / beta into the
//                                                   // functor's registers; false -> the workgroup returns
//   struct X;  __device__ X xop(const double* x) const;   // operand functor: X{}(c) = value of the SpMV
//                                                   // operand at column c (default: x[c]); lets a kernel
//                                                   // multiply with a vector that is only defined by a
//                                                   // recurrence, e.g. beta * s[c] + w[c], without a pass
//                                                   // that materialises it first.  X::kStageable says
//                                                   // whether the operand is one stored vector (ptr()) with a
//                                                   // scalar map value(raw) on top: only those can use the
//                                                   // staged form of a matrix; xop() is called before the
//                                                   // prologue for ptr() and after it for value() / ().
template <class E, class = void>
struct EpiPre {
  struct type {};
  static __device__ type fetch(const E&, int) { return type{}; }
  static __device__ void row(E& e, int r, double ax, const type&) { e.row(r, ax); }
};
template <class E>
struct EpiPre<E, std::void_t<typename E::Pre>> {
  using type = typename E::Pre;
  static __device__ type fetch(const E& e, int r) { return e.fetch(r); }
  static __device__ void row(E& e, int r, double ax, const type& p) { e.row(r, ax, p); }
};

struct XPlain {
  const double* __restrict__ x;
  // an operand that is ONE stored vector (times a scalar at most) can be staged: ptr() is copied to LDS as it is
  // and value() applied to what is read back
  static constexpr bool kStageable = true;
  __device__ const double* ptr() const { return x; }
  __device__ double value(double r) const { return r; }
#if defined(NSS_PROBE_GATHER) && NSS_PROBE_GATHER == 1      // timing probes only (tools/spmv_probe.py): wrong results
  __device__ double operator()(int c) const { return 1.0 + 1e-12 * double(c); }   // no operand gather at all
#elif defined(NSS_PROBE_GATHER) && NSS_PROBE_GATHER == 2
  __device__ double operator()(int c) const { return x[c & 1023]; }               // every gather an L1 hit
#else
  __device__ double operator()(int c) const { return x[c]; }
#endif
};
// An operand that is an expression of TWO stored vectors can be pair-staged: ptr() / ptr2() are copied to the two
// halves of the LDS buffer and pair(a, b) is applied to what is read back (X::kStageablePair, X::ptr2, X::pair).
template <class X, class = void>
struct XPairable : std::false_type {};
template <class X>
struct XPairable<X, std::enable_if_t<X::kStageablePair>> : std::true_type {};

template <class E, class = void>
struct EpiX {
  using type = XPlain;
  static __device__ type get(const E&, const double* x) { return XPlain{x}; }
};
template <class E>
struct EpiX<E, std::void_t<typename E::X>> {
  using type = typename E::X;
  static __device__ type get(const E& e, const double* x) { return e.xop(x); }
};
template <class E, class = void>
struct EpiPrologue {
  static __device__ bool run(E&, double*) { return true; }
};
template <class E>
struct EpiPrologue<E, std::void_t<decltype(std::declval<E&>().prologue(static_cast<double*>(nullptr)))>> {
  static __device__ bool run(E& e, double* lds) { return e.prologue(lds); }
};

constexpr int kBlockRows = 512;   // rows per row block of a matrix planned around Jacobi blocks (their results: 4 KiB of LDS)
constexpr int kRedDoubles = 32;   // per-workgroup reduction scratch (block_sum: 4, fixed_sum_1024: 32)

// Phase 1 of one row block for ONE form of the column stream (IDX: 0 = 4-byte columns, 1 = 16-bit
// window-relative columns, 2 = staged positions; GRP: one 16-bit index per group of a.gb entries): request the
// column and value streams, run the epilogue's prologue while they are in flight, take the operand (gather, or
// the LDS copy the caller has requested) and leave the products in `prod`.  Returns false when the prologue ends
// the workgroup.  The kernel selects the form at run time with uniform branches AROUND this function, and every
// form is straight-line code from the first load to the last product: with the branches inside (one loop per
// form, a common tail) hipcc waited for vmcnt(0) at the joins -- the column stream had to arrive before the
// value stream was even requested (seen in the ISA; plain SpMV of B^T +9 %).
template <class Epi, int KPF>
struct RowPrefetch {
  int s[KPF], e[KPF];
  typename EpiPre<Epi>::type pre[KPF];
};

template <class Epi, int CH, int IDX, bool GRP, int KPF, class VT = double>
__device__ __forceinline__ bool csr_phase1(const CsrView& a, const double* __restrict__ x, Epi& epi, int b, int p0,
                                           int cnt, double* prod, double* red, int32_t* window,
                                           RowPrefetch<Epi, KPF>& pf, int rf, int rstep, int r1,
                                           const double* dict = nullptr) {
  constexpr bool kCoded = std::is_same<VT, Coded8>::value;
  using SV = typename StoredValue<VT>::type;
  static_assert(IDX != 0 || !GRP, "grouped column stream needs a 16-bit form");
  using XOp = typename EpiX<Epi>::type;
  constexpr int kPer = CH / kBlock;
  const int tid = threadIdx.x;
  int32_t c[kPer];                                       // column (IDX 0), else position inside the group
  const SV* __restrict__ vals = view_values<VT>(a);
  SV v[kPer];                                            // (fp32: widened to fp64 at the product; codes: looked up there)
  uint16_t c16[kPer];
  if (IDX == 1) {
    if (tid < kWindows) window[tid] = a.blkbase[b * kWindows + tid];
  }
  uint32_t grp = 0, gsub = 0;                            // group of this lane's entry, position inside it
  if (GRP) {
    const uint32_t p = uint32_t(p0 + tid);
    grp = a.gb > 1 ? uint32_t(__umul64hi(uint64_t(p), a.gmagic)) : p;   // one division per lane, then incremental
    gsub = p - grp * a.gb;
  }
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const int i = tid + k * kBlock;
    const bool live = i < cnt;
    if (GRP) {                                           // one index per group of a.gb entries
      c16[k] = live ? a.col16[grp] : uint16_t(0);        // shared by a.gb neighbouring lanes
      c[k] = int32_t(gsub);
      gsub += a.sstep;
      grp += a.gstep + (gsub >= a.gb ? 1u : 0u);
      gsub -= gsub >= a.gb ? a.gb : 0u;
    }
#if NSS_STREAM_NT
    if (IDX != 0 && !GRP) c16[k] = live ? __builtin_nontemporal_load(&a.col16[p0 + i]) : uint16_t(0);
    if (IDX == 0) c[k] = live ? __builtin_nontemporal_load(&a.col[p0 + i]) : 0;
    v[k] = live ? __builtin_nontemporal_load(&vals[p0 + i]) : SV(0);
#else
    if (IDX != 0 && !GRP) c16[k] = live ? a.col16[p0 + i] : uint16_t(0);
    if (IDX == 0) c[k] = live ? a.col[p0 + i] : 0;
    v[k] = live ? vals[p0 + i] : SV(0);
#endif
  }
  // behind the matrix stream and in the same straight-line code (requested in front of it, the register
  // allocator re-used their destination registers for stream addresses and the compiler waited for them in the
  // middle of the stream -- seen in the ISA)
#if NSS_STREAM_PREFETCH
#pragma unroll
  for (int j = 0; j < KPF; ++j) {
    const int rj = rf + j * rstep;
    const bool has = rj < r1;
    pf.s[j] = has ? a.rowptr[rj] : 0;
    pf.e[j] = has ? a.rowptr[rj + 1] : 0;
    pf.pre[j] = has ? EpiPre<Epi>::fetch(epi, rj) : typename EpiPre<Epi>::type{};
  }
#endif
  if (!EpiPrologue<Epi>::run(epi, red)) return false;    // uniform over the workgroup
  const XOp xop = EpiX<Epi>::get(epi, x);
  double xv[kPer];
  if constexpr (IDX == 3) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // (see IDX == 2)
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      const int p = int(c16[k]) + (GRP ? c[k] : 0);
      xv[k] = (tid + k * kBlock < cnt) ? xop.pair(prod[p], prod[CH / 2 + p]) : 0.0;
    }
    __syncthreads();
  } else if constexpr (IDX == 2) {
    // LDS-DMA is tracked by vmcnt and gfx950 does not drain it at s_barrier: every wave waits for its own copies
    // before the barrier that publishes them to the other waves.  (hipcc already placed this wait here -- the
    // matrix stream is consumed right behind the barrier -- the statement pins it against code motion.)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                     // the LDS copy has landed in every wave's part
#pragma unroll
    for (int k = 0; k < kPer; ++k)
      xv[k] = (tid + k * kBlock < cnt) ? xop.value(prod[int(c16[k]) + (GRP ? c[k] : 0)]) : 0.0;
    __syncthreads();                                     // ... and has been read: the buffer takes the products
  } else {
    if (IDX == 1) {
      __syncthreads();                                   // window bases in LDS
#pragma unroll
      for (int k = 0; k < kPer; ++k)
        c[k] = window[c16[k] >> kWindowBits] + int32_t(c16[k] & ((1 << kWindowBits) - 1)) + (GRP ? c[k] : 0);
    }
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
      // columns are non-negative: without the hint the sign extension of a loaded 4-byte column is hoisted to
      // right behind its load, and every column load is followed by a wait (seen in the ISA)
      __builtin_assume(c[k] >= 0);
      xv[k] = (tid + k * kBlock < cnt) ? xop(c[k]) : 0.0;
    }
    if constexpr (kCoded) {
      // the gathering forms have no barrier between the stream and the products: the dictionary's LDS-DMA (requested
      // ahead of the stream) is awaited by its waves and published here, with the gather already in flight
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
  }
  // (coded, staged forms: the wait and the first barrier above have published the dictionary too)
#pragma unroll
  for (int k = 0; k < kPer; ++k)
    if (tid + k * kBlock < cnt) prod[tid + k * kBlock] = value_of<VT>(v[k], dict) * xv[k];
  return true;
}

typedef const int32_t __attribute__((address_space(4))) * ConstI32;   // uniform, invariant reads: scalar loads

// The operand runs of one row block -> LDS, by LDS-DMA (`d`: the block's descriptor, `total`: its word 5): a wave
// instruction moves 64 x 16 bytes = 128 consecutive staged positions to wave-uniform base + 16 * lane; each lane
// supplies the source address of its pair (segments start at even positions and have even lengths: spmv.hip).
// IDX 2: the runs of the operand vector -> buf[0, total); IDX 3 (total <= CH / 2): the first vector's runs ->
// buf[0, CH / 2), the second's -> buf[CH / 2, CH).  ptr() / ptr2() only: the epilogue's prologue has not run yet.  The
// copies are tracked by vmcnt: every wave waits for its own before the barrier that publishes them.  Shared by the
// stream kernel (the buffer then takes the products) and the row-slot kernel.
template <class Epi, int IDX, int CH>
__device__ __forceinline__ void stage_operand_runs(ConstI32 d, int total, const Epi& epi, const double* __restrict__ x,
                                                   double* prod) {
  using XOp = typename EpiX<Epi>::type;
  const int tid = threadIdx.x;
  int32_t seg_pre[kSegMax - 1], seg_off[kSegMax];
#pragma unroll
  for (int s = 0; s < kSegMax - 1; ++s) seg_pre[s] = d[kSegPre + s];
#pragma unroll
  for (int s = 0; s < kSegMax; ++s) seg_off[s] = d[kSegOff + s];
  const int wave = tid / kWave, lane = tid % kWave;
  if constexpr (IDX == 2) {
    const double* __restrict__ src = EpiX<Epi>::get(epi, x).ptr();
#pragma unroll
    for (int j = 0; j < CH / (2 * kBlock); ++j) {
      const int base = j * 2 * kBlock + wave * 2 * kWave;
      const int pos = base + 2 * lane;
      int o = seg_off[0];
#pragma unroll
      for (int s = 1; s < kSegMax; ++s) o = pos >= seg_pre[s - 1] ? seg_off[s] : o;
      if (pos < total) __builtin_amdgcn_global_load_lds((GlobalSrc)(src + pos + o), (LdsDst)(prod + base), 16, 0, 0);
    }
  } else {
    // pair: total <= CH / 2; the first vector's segments -> prod[0, CH/2), the second's -> prod[CH/2, CH)
    const XOp x0 = EpiX<Epi>::get(epi, x);
    const double* __restrict__ src1 = x0.ptr();
    const double* __restrict__ src2 = x0.ptr2();
#pragma unroll
    for (int j = 0; j < CH / (4 * kBlock); ++j) {
      const int base = j * 2 * kBlock + wave * 2 * kWave;
      const int pos = base + 2 * lane;
      int o = seg_off[0];
#pragma unroll
      for (int s = 1; s < kSegMax; ++s) o = pos >= seg_pre[s - 1] ? seg_off[s] : o;
      if (pos < total) {
        __builtin_amdgcn_global_load_lds((GlobalSrc)(src1 + pos + o), (LdsDst)(prod + base), 16, 0, 0);
        __builtin_amdgcn_global_load_lds((GlobalSrc)(src2 + pos + o), (LdsDst)(prod + CH / 2 + base), 16, 0, 0);
      }
    }
  }
}

// One workgroup = one row block: `wg` is the workgroup's index inside this launch's grid part.
// IDX / GRP: the form of the column stream (csr_phase1).  They are template parameters of the kernels: a run-time
// selection inside one kernel was tried (a fifth of the instantiations) and lost 6-10 % on the short-row
// operators -- with alternative paths in one kernel hipcc's wait-count insertion turns conservative at the joins
// and waits for vmcnt(0) in the middle of the matrix stream (seen in the ISA).  The one run-time branch left is
// the staged kernel's fallback for row blocks that do not fit the LDS copy.
template <int RG, class Epi, int IDX, int CH, bool GRP, class VT = double>
__device__ __forceinline__ void csr_stream_body(const CsrView& a, const double* __restrict__ x, Epi& epi, int wg,
                                                double* prod, double* red, int32_t* window) {
  using XOp = typename EpiX<Epi>::type;
  static_assert(IDX != 2 || XOp::kStageable, "staged form with an operand that cannot be copied to LDS");
  static_assert(IDX != 3 || XPairable<XOp>::value, "pair-staged form with an operand that is not a pair of vectors");
  const int tid = threadIdx.x;
  // XCD-aware map: workgroups with equal (index & 7) share an XCD; XCD i owns the i-th
  // contiguous eighth of the row blocks.  One row block per workgroup: a striding
  // (persistent) loop around this body measured 9 % slower on the A SpMV (extra barrier, and
  // the hardware dispatcher balances the tail better).
  const int lb = (wg & (kXcds - 1)) * a.per_xcd + (wg >> 3);
  int b = lb < a.nblk ? a.blk0 + lb : -1;
  if constexpr (IDX >= 2) {
    // reuse-aware dispatch order: slot lb of the dispatch-ordered table names its row block (uniform scalar load)
    if (a.blkdisp != nullptr) b = ((ConstI32)(a.blkdisp + size_t(lb) * kSegWords))[kSegBlock];
  }
  double* const dict = DictLds<VT>::get();
  if (b >= 0) {
    int r0 = 0, r1 = 0, p0 = 0, cnt = 0;
    DictLds<VT>::request(a, dict);                          // (coded form) ahead of everything else
    if constexpr (IDX >= 2) {
      // One descriptor per row block instead of the rowblk -> rowptr chain.  It must arrive through SCALAR loads
      // (the run table then sits in SGPRs); the constant address space makes the loads invariant, and a uniform
      // invariant load is an s_load -- as vector loads (what the compiler emitted in the two-matrix kernel) every
      // use below would wait for vmcnt(0).
      const ConstI32 d = a.blkdisp != nullptr ? (ConstI32)(a.blkdisp + size_t(lb) * kSegWords)
                                              : (ConstI32)(a.blkseg + size_t(b) * kSegWords);
      r0 = d[0];
      r1 = d[1];
      p0 = d[2];
      cnt = d[3];
      const int total = d[5];                              // 0 for a row block that is one over-long row
      // The operand segments of this row block -> LDS (the product buffer, until every lane has taken its
      // values).  Issued BEFORE the matrix stream, on which it does not depend.
      stage_operand_runs<Epi, IDX, CH>(d, total, epi, x, prod);
    } else {
      r0 = a.rowblk[b];
      r1 = a.rowblk[b + 1];
      p0 = a.rowptr[r0];
      cnt = a.rowptr[r1] - p0;
    }
    // Row bounds and epilogue operands of this lane's first phase-2 rows (kPF of them: short-row matrices
    // give a lane several rows): requested inside phase 1, right behind the matrix stream, so that their HBM
    // latency overlaps it instead of following the barrier.
    constexpr int kPF = RG == 1 ? NSS_PREFETCH_ROWS : 1;
    const int rf = r0 + tid / RG;
    RowPrefetch<Epi, kPF> pf;
    if (cnt <= CH) {
      constexpr int kPer = CH / kBlock;
      (void)kPer;
      // ---- phase 1: coalesced stream of (col, val), operand, stage products ------------
      const bool go = csr_phase1<Epi, CH, IDX, GRP, kPF, VT>(a, x, epi, b, p0, cnt, prod, red, window, pf, rf, kBlock / RG, r1, dict);
      if (!go) return;                                     // the prologue ended the workgroup (uniform)
      __syncthreads();
      // ---- phase 2: per-row reduction from LDS -----------------------------------------
      constexpr int kRowsPerPass = kBlock / RG;
      const int sub = tid % RG;
#if NSS_STREAM_PREFETCH
#pragma unroll
      for (int q = 0; q < kPF; ++q) {                      // the prefetched rows
        const int r = rf + q * kRowsPerPass;
        if (r < r1) {
          const int s = pf.s[q] - p0, e = pf.e[q] - p0;
          double sum = 0.0;
          for (int j = s + sub; j < e; j += RG) sum += prod[j];
          if (RG > 1) {
#pragma unroll
            for (int off = RG / 2; off > 0; off >>= 1) sum += __shfl_xor(sum, off, kWave);
          }
          if (sub == 0) EpiPre<Epi>::row(epi, r, sum, pf.pre[q]);
        }
      }
      for (int r = rf + kPF * kRowsPerPass; r < r1; r += kRowsPerPass) {
        const int s = a.rowptr[r] - p0;
        const int e = a.rowptr[r + 1] - p0;
        double sum = 0.0;
        for (int j = s + sub; j < e; j += RG) sum += prod[j];
        if (RG > 1) {
#pragma unroll
          for (int off = RG / 2; off > 0; off >>= 1) sum += __shfl_xor(sum, off, kWave);
        }
        if (sub == 0) EpiPre<Epi>::row(epi, r, sum, EpiPre<Epi>::fetch(epi, r));
      }
#else
      for (int r = r0 + tid / RG; r < r1; r += kRowsPerPass) {
        const int s = a.rowptr[r] - p0;
        const int e = a.rowptr[r + 1] - p0;
        double sum = 0.0;
        for (int j = s + sub; j < e; j += RG) sum += prod[j];
        if (RG > 1) {
#pragma unroll
          for (int off = RG / 2; off > 0; off >>= 1) sum += __shfl_xor(sum, off, kWave);
        }
        if (sub == 0) EpiPre<Epi>::row(epi, r, sum, EpiPre<Epi>::fetch(epi, r));
      }
#endif
    } else {
      // ---- one row longer than the LDS chunk: the whole workgroup reduces it ----------
      if (!EpiPrologue<Epi>::run(epi, red)) return;
      const XOp xop = EpiX<Epi>::get(epi, x);
      double acc = 0.0;
      const typename StoredValue<VT>::type* __restrict__ vals = view_values<VT>(a);
      if constexpr (std::is_same<VT, Coded8>::value) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the dictionary's LDS-DMA, then published
        __syncthreads();
      }
      for (int i = tid; i < cnt; i += kBlock) acc = fma(value_of<VT>(vals[p0 + i], dict), xop(a.col[p0 + i]), acc);
      const double sum = block_sum(acc, red);
      if (tid == 0) EpiPre<Epi>::row(epi, r0, sum, EpiPre<Epi>::fetch(epi, r0));
    }
  }
  epi.finish(b, red);  // one dot partial per row block
}

template <int RG, class Epi, int IDX = 0, int CH = kChunk, bool GRP = false, class VT = double>
__global__ __launch_bounds__(kBlock) void csr_stream_kernel(CsrView a, const double* __restrict__ x, Epi epi) {
  __shared__ double prod[CH];
  __shared__ double red[kRedDoubles];
  __shared__ int32_t window[kWindows];
  if (epi.skip()) return;
  csr_stream_body<RG, Epi, IDX, CH, GRP, VT>(a, x, epi, int(blockIdx.x), prod, red, window);
}

// Two matrices with the same launch-plan parameters in ONE launch: two SpMVs that do not depend on each other
// (the fused BPCG iteration: t2 = A t1 and t3 = B (t1 - s0)) share a kernel boundary.  The two halves may use
// different column streams (IDXA / IDXB).  The workgroups of the SECOND matrix come first in the grid
// (`grid_b` of them, then those of the first): in every use it is the smaller one with the less regular
// operand access (B: gathers over three grid planes), and at the end of the grid its few, slow workgroups
// would be the tail of the launch while the chip drains -- in front they overlap the long uniform stream of A.
#ifndef NSS_DUAL_SECOND_FIRST
#define NSS_DUAL_SECOND_FIRST 1
#endif
template <int RG, class EpiA, class EpiB, int IDXA, int IDXB, int CH, bool GRP, class VT = double>
__global__ __launch_bounds__(kBlock) void csr_stream_dual_kernel(CsrView a, CsrView b, int grid_a, int grid_b,
                                                                  const double* __restrict__ xa,
                                                                  const double* __restrict__ xb, EpiA ea, EpiB eb) {
  __shared__ double prod[CH];
  __shared__ double red[kRedDoubles];
  __shared__ int32_t window[kWindows];
#if NSS_DUAL_SECOND_FIRST
  const bool first = int(blockIdx.x) >= grid_b;
  const int wg = first ? int(blockIdx.x) - grid_b : int(blockIdx.x);
#else
  const bool first = int(blockIdx.x) < grid_a;
  const int wg = first ? int(blockIdx.x) : int(blockIdx.x) - grid_a;
#endif
  if (first) {
    if (ea.skip()) return;
    csr_stream_body<RG, EpiA, IDXA, CH, (GRP && IDXA != 0), VT>(a, xa, ea, wg, prod, red, window);
  } else {
    if (eb.skip()) return;
    csr_stream_body<RG, EpiB, IDXB, CH, (GRP && IDXB != 0), VT>(b, xb, eb, wg, prod, red, window);
  }
}

// The row-per-lane kernel's view of the Pre / fetch interface: an epilogue may keep its up-front operands for that
// kernel alone -- struct DirectPre; fetch_direct(r); row(r, ax, const DirectPre&) -- where the stream kernel is better
// off loading them late (EpiK1c: 12 registers there cost it occupancy).  Without DirectPre: as EpiPre.
template <class E, class = void>
struct EpiDirectPre : EpiPre<E> {};
template <class E>
struct EpiDirectPre<E, std::void_t<typename E::DirectPre>> {
  using type = typename E::DirectPre;
  static __device__ type fetch(const E& e, int r) { return e.fetch_direct(r); }
  static __device__ void row(E& e, int r, double ax, const type& p) { e.row(r, ax, p); }
};

// Row-per-lane kernel for the fixed-width copy (nss_csr_s::ell_col): workgroup = one row block of at most
// kDirectRows rows, lane t takes rows r0 + t and r0 + t + 256 (unit stride across the lanes; giving a lane two
// CONSECUTIVE rows instead makes every per-row access of the epilogue a stride-2 access: C1 +35 %).  The operand is
// gathered (two entries per row: nothing to stage).  The row sum is formed exactly as the stream kernel forms it
// (0 + p0 + p1, products rounded on their own: mul_unfused), so both kernels give identical bits.
// Coded form (VT = Coded8): the row's 16-bit code word (`ecode`) instead of the two 8-byte values, both values from the
// LDS copy of the dictionary -- 10 bytes per row instead of 24.
//
// A workgroup makes THREE dependent memory rounds: (1) column pairs, code words / values and the epilogue's operands of
// both rows, (2) the eight operand gathers, (3) the stores.  For that the rows' code is straight-line from the first
// load to the last gather -- hipcc closes every branch that holds a load (`live ? load : default`, `c >= 0 ? x[c] : 0`)
// with s_waitcnt vmcnt(0), and the earlier form of this kernel made about eleven rounds that way (seen in the ISA,
// profiles/r06_c1_rounds.md):
//  * the row-block bounds come through scalar loads (constant address space, as csr_stream_body reads blkseg);
//  * ONE uniform branch separates full row blocks (all but the last of a matrix: no per-lane predicate at all) from
//    partial ones, whose loads go to a clamped valid row -- only row() is predicated there;
//  * padding slots (column -1) gather from column 0 and the product is discarded by a select: the sum is
//    0 + (p0 or 0) + (p1 or 0), the same bits as skipping the addition (0 + p is never -0, and s + 0 == s then);
//  * the epilogue's prologue runs behind the front loads; its own reads should be scalar loads (EpiK1c);
//  * coded form: the one wait and barrier that publish the dictionary stand behind the gathers, where every load of the
//    workgroup is in flight.
// C16 (coded form only; nss_csr_s::ell_col16): `ecol` holds one 32-bit word per row, the two columns as 16-bit offsets
// from the row block's window base `cbase` (packed_rows.h) -- 6 bytes per row instead of 10.  The base is a scalar
// load beside the row-block bounds; a padding slot gathers from the base column.
// base_first: this call is the row block's first (it requests the dictionary and runs the prologue).
template <bool FULL, class Epi, class VT, bool C16>
__device__ __forceinline__ bool csr_direct_rows(const CsrView& a, const int32_t* __restrict__ ecol,
                                                const double* __restrict__ eval, const uint16_t* __restrict__ ecode,
                                                const double* __restrict__ x, Epi& epi, int base, int r1, bool base_first,
                                                double* red, double* dict, int cbase) {
  using XOp = typename EpiX<Epi>::type;
  using Pre = EpiDirectPre<Epi>;
  constexpr bool kCoded = std::is_same<VT, Coded8>::value;
  static_assert(!C16 || kCoded, "16-bit columns belong to the coded fixed-width copy");
  constexpr int kRows = kDirectRows / kBlock;
  typedef int32_t int2v __attribute__((ext_vector_type(2)));
  const int tid = threadIdx.x;
  int rl[kRows];                                              // the row every load of slot q goes to
#pragma unroll
  for (int q = 0; q < kRows; ++q) {
    const int r = base + tid + q * kBlock;
    rl[q] = FULL ? r : (r < r1 ? r : r1 - 1);
  }
  int2v c[kRows];
  uint32_t cw[kRows];
  dbl2v v[kRows];
  uint16_t code[kRows];
  typename Pre::type pre[kRows];
#pragma unroll
  for (int q = 0; q < kRows; ++q) {
    if constexpr (C16) cw[q] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(ecol) + rl[q]);
    else c[q] = __builtin_nontemporal_load(reinterpret_cast<const int2v*>(ecol) + rl[q]);
  }
#pragma unroll
  for (int q = 0; q < kRows; ++q) {
    if constexpr (kCoded) code[q] = __builtin_nontemporal_load(ecode + rl[q]);
    else v[q] = __builtin_nontemporal_load(reinterpret_cast<const dbl2v*>(eval) + rl[q]);
  }
#pragma unroll
  for (int q = 0; q < kRows; ++q) pre[q] = Pre::fetch(epi, rl[q]);
  // (coded form) the dictionary's copy is requested BEHIND the rows' loads: the request sits in a branch of its own
  // (two of the four waves make it), and in front hipcc made every wave wait for it at the join before the first load
  if (base_first) DictLds<VT>::request(a, dict);
  if (base_first && !EpiPrologue<Epi>::run(epi, red)) return false;   // uniform over the workgroup
  const XOp xop = EpiX<Epi>::get(epi, x);
  double x0[kRows], x1[kRows];
#pragma unroll
  for (int q = 0; q < kRows; ++q) {
    if constexpr (C16) {
      x0[q] = xop(col16_gather_column(cw[q], 0, cbase));
      x1[q] = xop(col16_gather_column(cw[q], 1, cbase));
    } else {
      x0[q] = xop(c[q].x >= 0 ? c[q].x : 0);
      x1[q] = xop(c[q].y >= 0 ? c[q].y : 0);
    }
  }
  if constexpr (kCoded) {
    // the one barrier of the coded form: the dictionary's LDS-DMA is awaited by its waves and published, with
    // every load of the workgroup in flight.  (Reading the two entries as gathers from the 2-KiB table in global
    // memory instead -- no LDS, no barrier -- measured the same: profiles/r06_ab_c1_rounds.txt.)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kRows; ++q) v[q] = dbl2v{dict[code[q] & 0xff], dict[code[q] >> 8]};
  }
#pragma unroll
  for (int q = 0; q < kRows; ++q) {
    const int r = base + tid + q * kBlock;
    const double p0 = mul_unfused(v[q].x, x0[q]), p1 = mul_unfused(v[q].y, x1[q]);
    double sum = 0.0;
    if constexpr (C16) {
      sum += col16_live(cw[q], 0) ? p0 : 0.0;
      sum += col16_live(cw[q], 1) ? p1 : 0.0;
    } else {
      sum += c[q].x >= 0 ? p0 : 0.0;
      sum += c[q].y >= 0 ? p1 : 0.0;
    }
    if (FULL || r < r1) Pre::row(epi, r, sum, pre[q]);
  }
  return true;
}

template <class Epi, class VT = double, bool C16 = false>
__global__ __launch_bounds__(kBlock) void csr_direct_kernel(CsrView a, const int32_t* __restrict__ ecol,
                                                            const double* __restrict__ eval,
                                                            const uint16_t* __restrict__ ecode,
                                                            const int32_t* __restrict__ ebase,
                                                            const double* __restrict__ x, Epi epi) {
  static_assert(kDirectWidth == 2, "csr_direct_kernel is written for two slots per row");
  __shared__ double red[kRedDoubles];
  double* const dict = DictLds<VT>::get();
  if (epi.skip()) return;
  const int wg = int(blockIdx.x);
  const int lb = (wg & (kXcds - 1)) * a.per_xcd + (wg >> 3);
  const int b = lb < a.nblk ? a.blk0 + lb : -1;
  if (b >= 0) {
    const ConstI32 rb = (ConstI32)(a.rowblk + b);             // uniform, invariant: scalar loads
    const int r0 = rb[0], r1 = rb[1];
    int cbase = 0;                                            // window base of the 16-bit columns: a scalar load too
    if constexpr (C16) cbase = ((ConstI32)(ebase + b))[0];
    bool go = true;
    if (r1 - r0 == kDirectRows) {
      go = csr_direct_rows<true, Epi, VT, C16>(a, ecol, eval, ecode, x, epi, r0, r1, true, red, dict, cbase);
    } else if (r1 - r0 < kDirectRows) {
      if (r1 > r0) go = csr_direct_rows<false, Epi, VT, C16>(a, ecol, eval, ecode, x, epi, r0, r1, true, red, dict, cbase);
    } else {
      // (the plan caps the row blocks of such a matrix at kDirectRows rows; a longer one is walked in pieces)
      for (int base = r0; go && base < r1; base += kDirectRows)
        go = csr_direct_rows<false, Epi, VT, C16>(a, ecol, eval, ecode, x, epi, base, r1, base == r0, red, dict, cbase);
    }
    if (!go) return;                                          // the prologue ended the workgroup (uniform)
  }
  epi.finish(b, red);
}

// Row-per-lane kernel with the STAGED operand, for the row-slot copy of a coded matrix (nss_csr_s::slot_pos): the third
// kernel form.  With value codes a row block of 256 rows x 7 entries is 5 KB of matrix beside 9 KB of vectors, and the
// stream form -- sixteen 1- and 2-byte loads per lane, three barriers, every product written to and read back from LDS,
// a dependent per-row LDS loop -- is built for rows of 82 entries.  Here lane t takes rows r0 + t, r0 + t + 256, ...
// one piece of 256 rows after the other (the stream kernel's lane -> row map at one lane per row, so `acc` and the
// block partial are its too), holds the row's eight staged positions and codes in registers (one 16-byte and one
// 4-byte load of the packed row, packed_rows.h: 20 bytes; PK false: 16 + 8 bytes, the layout the form was introduced
// with, kept for tests and measurements), and makes THREE dependent memory rounds: (1) descriptor, LDS-DMA of the operand runs, slot words,
// epilogue operands, dictionary; (2) one wait + one barrier, eight LDS reads of the operand, eight of the dictionary;
// (3) the stores.  Straight-line from the first load to the last product, as csr_direct_rows: one uniform branch between
// full and partial pieces, partial ones load from a clamped valid row and predicate only row(); a padding slot (k at or
// behind the row length; PK false: position kSlotPad) reads LDS position 0 and its product is discarded by a select.
// The packed words are unpacked behind the barrier, where the wave has them anyway.
// Bits: the stream kernel adds prod[s] ... prod[e - 1] in order to 0.0, each a product rounded by its store; here the
// products are rounded by mul_unfused and added in slot order, + 0.0 for an unused slot -- 0 + p is never -0, so
// s + 0.0 == s for every partial sum.
// LDS: the operand copy (CH doubles), the dictionary, `red`; no product buffer, no window table.
typedef uint32_t uint4v __attribute__((ext_vector_type(4)));
typedef uint32_t uint2v __attribute__((ext_vector_type(2)));
// the second word of a row: the eight codes (8 bytes), or, PK, the last word of the packed row (packed_rows.h)
template <bool PK>
struct SlotTail { using type = uint2v; };
template <>
struct SlotTail<true> { using type = uint32_t; };

template <bool FULL, bool PK, class Epi, int IDX, int CH>
__device__ __forceinline__ bool csr_slots_rows(const CsrView& a, const uint4v* __restrict__ spos,
                                               const typename SlotTail<PK>::type* __restrict__ scode,
                                               const double* __restrict__ x, Epi& epi,
                                               int base, int r1, bool base_first, const double* xlds, double* red,
                                               double* dict) {
  using XOp = typename EpiX<Epi>::type;
  using Pre = EpiPre<Epi>;
  static_assert(kSlotWidth == 8, "csr_slots_rows is written for eight slots per row");
  static_assert(!PK || (kSlotWidth == kPackedSlots && CH <= int(kPackedPosLimit)),
                "a staged position must fit the 11 bits of the packed row words");
  const int r = base + int(threadIdx.x);
  const int rl = FULL ? r : (r < r1 ? r : r1 - 1);            // the row every load goes to
  const uint4v pw = __builtin_nontemporal_load(spos + rl);
  const typename SlotTail<PK>::type cw = __builtin_nontemporal_load(scode + rl);
  const typename Pre::type pre = Pre::fetch(epi, rl);
  // behind the rows' loads (csr_direct_rows: in front, every wave waits for the two requesting waves' branch)
  if (base_first) DictLds<Coded8>::request(a, dict);
  if (base_first && !EpiPrologue<Epi>::run(epi, red)) return false;   // uniform over the workgroup
  const XOp xop = EpiX<Epi>::get(epi, x);
  // the one wait and barrier: the LDS-DMA copies (operand runs, dictionary) are awaited by their waves and published
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  bool live[kSlotWidth];
  int q[kSlotWidth];
  uint32_t code[kSlotWidth];
  if constexpr (PK) {
    const uint32_t u[5] = {pw.x, pw.y, pw.z, pw.w, cw};
    const uint32_t len = packed_slot_len(u);
#pragma unroll
    for (int k = 0; k < kSlotWidth; ++k) {
      live[k] = uint32_t(k) < len;
      q[k] = int(packed_slot_pos(u, k));                      // (0 in an unused slot)
      code[k] = packed_slot_code(u, k);
    }
  } else {
    const uint32_t w[4] = {pw.x, pw.y, pw.z, pw.w};
    const uint32_t cws[2] = {cw.x, cw.y};
#pragma unroll
    for (int k = 0; k < kSlotWidth; ++k) {
      const uint32_t p = (w[k / 2] >> (16 * (k % 2))) & 0xffffu;
      live[k] = p != kSlotPad;
      q[k] = live[k] ? int(p) : 0;
      code[k] = (cws[k / 4] >> (8 * (k % 4))) & 0xffu;
    }
  }
  double xv[kSlotWidth], v[kSlotWidth];
#pragma unroll
  for (int k = 0; k < kSlotWidth; ++k) {
    if constexpr (IDX == 3) xv[k] = xop.pair(xlds[q[k]], xlds[CH / 2 + q[k]]);
    else xv[k] = xop.value(xlds[q[k]]);
    v[k] = dict[code[k]];
  }
  double sum = 0.0;
#pragma unroll
  for (int k = 0; k < kSlotWidth; ++k) {
    const double p = mul_unfused(v[k], xv[k]);
    sum += live[k] ? p : 0.0;
  }
  if (FULL || r < r1) Pre::row(epi, r, sum, pre);
  return true;
}

// one workgroup = one row block (`wg`: the workgroup's index inside this launch's grid part; the stream kernel's map)
template <bool PK, class Epi, int IDX, int CH>
__device__ __forceinline__ void csr_slots_body(const CsrView& a, const uint4v* __restrict__ spos,
                                               const typename SlotTail<PK>::type* __restrict__ scode,
                                               const double* __restrict__ x, Epi& epi,
                                               int wg, double* xlds, double* red, double* dict) {
  using XOp = typename EpiX<Epi>::type;
  static_assert(IDX == 2 || IDX == 3, "the row-slot kernel takes the staged forms only");
  static_assert(IDX != 2 || XOp::kStageable, "staged form with an operand that cannot be copied to LDS");
  static_assert(IDX != 3 || XPairable<XOp>::value, "pair-staged form with an operand that is not a pair of vectors");
  const int lb = (wg & (kXcds - 1)) * a.per_xcd + (wg >> 3);
  const int b = lb < a.nblk ? a.blk0 + lb : -1;
  if (b >= 0) {
    const ConstI32 d = (ConstI32)(a.blkseg + size_t(b) * kSegWords);   // scalar loads (see csr_stream_body)
    const int r0 = d[0], r1 = d[1], total = d[5];
    stage_operand_runs<Epi, IDX, CH>(d, total, epi, x, xlds);
    bool go = true;
    if (r1 - r0 == kBlock) {
      go = csr_slots_rows<true, PK, Epi, IDX, CH>(a, spos, scode, x, epi, r0, r1, true, xlds, red, dict);
    } else if (r1 - r0 < kBlock) {
      if (r1 > r0) go = csr_slots_rows<false, PK, Epi, IDX, CH>(a, spos, scode, x, epi, r0, r1, true, xlds, red, dict);
    } else {
      // rows of few entries: a row block of up to kMaxRowsPerBlock rows is walked in pieces (the operand copy stays)
      for (int base = r0; go && base < r1; base += kBlock)
        go = csr_slots_rows<false, PK, Epi, IDX, CH>(a, spos, scode, x, epi, base, r1, base == r0, xlds, red, dict);
    }
    if (!go) return;                                          // the prologue ended the workgroup (uniform)
  }
  epi.finish(b, red);  // one dot partial per row block, in the stream kernel's slot
}

template <class Epi, int IDX, bool PK, int CH = kChunk>
__global__ __launch_bounds__(kBlock) void csr_slots_kernel(CsrView a, const uint4v* __restrict__ spos,
                                                           const typename SlotTail<PK>::type* __restrict__ scode,
                                                           const double* __restrict__ x, Epi epi) {
  __shared__ alignas(16) double xlds[CH];
  __shared__ double red[kRedDoubles];
  double* const dict = DictLds<Coded8>::get();
  if (epi.skip()) return;
  csr_slots_body<PK, Epi, IDX, CH>(a, spos, scode, x, epi, int(blockIdx.x), xlds, red, dict);
}

// two matrices in one launch, the second one's workgroups first (csr_stream_dual_kernel)
template <class EpiA, class EpiB, int IDXA, int IDXB, bool PK, int CH = kChunk>
__global__ __launch_bounds__(kBlock) void csr_slots_dual_kernel(CsrView a, CsrView b, const uint4v* __restrict__ apos,
                                                                const typename SlotTail<PK>::type* __restrict__ acode,
                                                                const uint4v* __restrict__ bpos,
                                                                const typename SlotTail<PK>::type* __restrict__ bcode,
                                                                int grid_a, int grid_b,
                                                                const double* __restrict__ xa,
                                                                const double* __restrict__ xb, EpiA ea, EpiB eb) {
  __shared__ alignas(16) double xlds[CH];
  __shared__ double red[kRedDoubles];
  double* const dict = DictLds<Coded8>::get();
#if NSS_DUAL_SECOND_FIRST
  const bool first = int(blockIdx.x) >= grid_b;
  const int wg = first ? int(blockIdx.x) - grid_b : int(blockIdx.x);
#else
  const bool first = int(blockIdx.x) < grid_a;
  const int wg = first ? int(blockIdx.x) : int(blockIdx.x) - grid_a;
#endif
  if (first) {
    if (ea.skip()) return;
    csr_slots_body<PK, EpiA, IDXA, CH>(a, apos, acode, xa, ea, wg, xlds, red, dict);
  } else {
    if (eb.skip()) return;
    csr_slots_body<PK, EpiB, IDXB, CH>(b, bpos, bcode, xb, eb, wg, xlds, red, dict);
  }
}

// Value forms a launch site instantiates besides fp64 (the FORMS argument of the launchers below).  The value type is a
// template parameter of the kernels, so every form a site asks for adds a full set of instantiations of its epilogue:
// kF32 only where an fp32-storage preconditioner handle launches (the colour launches and residuals of the
// Gauss-Seidel sweep, the single-vector AMG cycle, the residual between the half-sweeps), kCodes only in the launches
// of the flagship loop (C1, C23), both in the plain SpMV.  A matrix in a form its site did not ask for takes the fp64
// path: a coded matrix reads `val`, a narrowed one is refused (view()).
// kCol16 (with kCodes): also the 16-bit-column form of the coded row-per-lane kernel (nss_csr_s::ell_col16) -- only C1 of
// the flagship loop and the plain SpMV ask for it.
enum : unsigned { kF64 = 0, kF32 = 1, kCodes = 2, kCol16 = 4 };

template <int I>
using Idx = std::integral_constant<int, I>;
template <class VT>
struct ValueTag { using type = VT; };
// value types with grouped forms of the 16-bit column streams (a coded matrix is never grouped: nss_csr_s::coded)
template <class VT>
constexpr bool kHasGroupedForms = !std::is_same<VT, Coded8>::value;

// f(Idx<RG>) for the lanes-per-row value RG of the launch plan: one instantiation per value
template <class F>
inline void for_plan_lanes(const nss_csr_s& A, F&& f) {
  switch (A.rg) {
    case 1: f(Idx<1>{}); break;
    case 2: f(Idx<2>{}); break;
    case 4: f(Idx<4>{}); break;
    case 8: f(Idx<8>{}); break;
    case 16: f(Idx<16>{}); break;
    case 32: f(Idx<32>{}); break;
    case 64: f(Idx<64>{}); break;
    default: throw Error("csr_stream: bad lanes-per-row in the launch plan");
  }
}

// the stream kernel over the row blocks [b0, b1) with value type VT (A is not empty and has no fixed-width copy)
template <class VT, class Epi>
inline void launch_csr_stream_kernel(const nss_csr_s& A, const double* x, const Epi& epi, hipStream_t st, int b0, int b1,
                                     size_t dyn_lds) {
  constexpr bool kCanStage = EpiX<Epi>::type::kStageable;
  constexpr bool kCanPair = XPairable<typename EpiX<Epi>::type>::value;
  const int mode = A.idx_mode(kCanStage, kCanPair);
  const bool grp = mode != 0 && A.gb > 1;
  const CsrView v = A.view(b0, b1, mode, std::is_same<VT, float>::value);
  const dim3 grid(nss_csr_s::grid(b1 - b0)), block(kBlock);
  for_plan_lanes(A, [&](auto lanes) {
    const auto go = [&](auto idx) {     // ONE form of the column stream, grouped where the stream is and VT can be
      constexpr int RG = decltype(lanes)::value, IDX = decltype(idx)::value;
      constexpr bool kGrp = IDX != 0 && kHasGroupedForms<VT>;     // (false: both lines name the same instantiation)
      if (kGrp && grp) hipLaunchKernelGGL((csr_stream_kernel<RG, Epi, IDX, kChunk, kGrp, VT>), grid, block, dyn_lds, st, v, x, epi);
      else hipLaunchKernelGGL((csr_stream_kernel<RG, Epi, IDX, kChunk, false, VT>), grid, block, dyn_lds, st, v, x, epi);
    };
    if (mode == 2) { if constexpr (kCanStage) go(Idx<2>{}); }
    else if (mode == 3) { if constexpr (kCanPair) go(Idx<3>{}); }
    else if (mode == 1) go(Idx<1>{});
    else go(Idx<0>{});
  });
  NSS_CHECK_LAUNCH();
}

// A x into `epi` over the rows of the row blocks [b0, b1) (default: all), by the kernel and in the value form that the
// matrix holds and FORMS allows: fp32 values (nss_csr_s::val32) under kF32, value codes (nss_csr_s::coded) under
// kCodes, else fp64; the row-per-lane kernel where the matrix has the fixed-width copy, else the stream kernel.
// DIRECT_ONLY (launch_csr_direct): instantiate the row-per-lane kernel alone.
template <unsigned FORMS = kF64, bool DIRECT_ONLY = false, class Epi>
inline void launch_csr(const nss_csr_s& A, const double* x, const Epi& epi, hipStream_t st, int b0 = 0, int b1 = -1,
                       size_t dyn_lds = 0) {
  constexpr bool kF32Form = (FORMS & kF32) != 0 && !DIRECT_ONLY, kCodedForm = (FORMS & kCodes) != 0;
  constexpr bool kCol16Form = kCodedForm && (FORMS & kCol16) != 0;
  using CodedVT = std::conditional_t<kCodedForm, Coded8, double>;     // (form not asked for: the fp64 kernels either way)
  if (b1 < 0) b1 = A.nblk;
  if (A.m == 0 || b1 <= b0) return;
  if constexpr (kF32Form) {
    if (A.val32) {
      NSS_REQUIRE(!A.ell_col, "csr_stream: a matrix with fp32 values has no fixed-width copy");
      launch_csr_stream_kernel<float>(A, x, epi, st, b0, b1, dyn_lds);
      return;
    }
  }
  if (DIRECT_ONLY && !A.ell_col) throw Error("csr_direct: the matrix has no fixed-width copy");
  if (A.ell_col) {
    const dim3 grid(nss_csr_s::grid(b1 - b0)), block(kBlock);
    const CsrView v = A.view(b0, b1, 0);
    const int32_t* const none = nullptr;
    if (kCol16Form && A.direct_col16())
      hipLaunchKernelGGL((csr_direct_kernel<Epi, CodedVT, kCol16Form>), grid, block, dyn_lds, st, v,
                         reinterpret_cast<const int32_t*>(A.ell_col16.get()), A.ell_val, A.ell_code, A.ell_base, x, epi);
    else if (kCodedForm && A.coded() && A.ell_code)
      hipLaunchKernelGGL((csr_direct_kernel<Epi, CodedVT>), grid, block, dyn_lds, st, v, A.ell_col, A.ell_val, A.ell_code, none, x, epi);
    else
      hipLaunchKernelGGL((csr_direct_kernel<Epi>), grid, block, dyn_lds, st, v, A.ell_col, A.ell_val, (const uint16_t*)nullptr, none, x, epi);
    NSS_CHECK_LAUNCH();
  } else if constexpr (!DIRECT_ONLY) {
    if (kCodedForm && A.coded() && !A.val32) launch_csr_stream_kernel<CodedVT>(A, x, epi, st, b0, b1, dyn_lds);
    else launch_csr_stream_kernel<double>(A, x, epi, st, b0, b1, dyn_lds);
  }
}

// the row-per-lane kernel alone (A must hold the fixed-width copy): for epilogue variants that only exist for it
template <unsigned FORMS = kF64, class Epi>
inline void launch_csr_direct(const nss_csr_s& A, const double* x, const Epi& epi, hipStream_t st, int b0 = 0,
                              int b1 = -1, size_t dyn_lds = 0) {
  launch_csr<FORMS, true>(A, x, epi, st, b0, b1, dyn_lds);
}

// whether launch_csr_dual takes A and B in one launch, and the column-stream forms of the two halves (stage_a, stage_b,
// pair_b: what the operands of the two epilogues admit)
inline bool csr_dual_forms(const nss_csr_s& A, const nss_csr_s& B, bool stage_a, bool stage_b, bool pair_b, int* ma_out,
                           int* mb_out) {
#ifdef NSS_NO_DUAL        // measurements: the two halves as launches of their own
  return false;
#endif
  if (A.m == 0 || B.m == 0 || A.nblk == 0 || B.nblk == 0) return false;
  if (A.ell_col || B.ell_col) return false;               // row-per-lane kernel: a launch of its own
  if (A.val32 || B.val32) return false;                   // fp32 values: the single-matrix launches (or their refusal)
  if (A.rg != B.rg || A.chunk != B.chunk) return false;
  const int ma = A.idx_mode(stage_a);
  int mb = B.idx_mode(stage_b, pair_b);
  if (mb == 3 && ma != 2) mb = B.col16 ? 1 : 0;           // the pair-staged half is only instantiated beside a staged one
  if ((ma == 0) != (mb == 0)) return false;               // a 4-byte stream only pairs with a 4-byte stream
  *ma_out = ma;
  *mb_out = mb;
  return true;
}

// A and B in one launch when their launch plans agree (lanes per row, chunk) and the pair of column streams is
// one of the instantiated ones; returns false (nothing launched) otherwise -- the caller then issues two launches.
// FORMS & kCodes: instantiate the coded form too, taken when BOTH matrices are coded (otherwise both halves read `val`).
template <unsigned FORMS = kF64, class EpiA, class EpiB>
inline bool launch_csr_dual(const nss_csr_s& A, const double* xa, const EpiA& ea, const nss_csr_s& B, const double* xb,
                            const EpiB& eb, hipStream_t st, size_t dyn_lds = 0) {
  constexpr bool kStageA = EpiX<EpiA>::type::kStageable, kStageB = EpiX<EpiB>::type::kStageable;
  constexpr bool kPairB = XPairable<typename EpiX<EpiB>::type>::value;
  int ma = 0, mb = 0;
  if (!csr_dual_forms(A, B, kStageA, kStageB, kPairB, &ma, &mb)) return false;
  const bool grp = ma != 0 && (A.gb > 1 || B.gb > 1);     // the grouped decode also reads a one-per-entry stream (gb == 1)
  const CsrView va = A.view(0, A.nblk, ma), vb = B.view(0, B.nblk, mb);
  const int ga = nss_csr_s::grid(A.nblk), gb = nss_csr_s::grid(B.nblk);
  const dim3 grid(ga + gb), block(kBlock);
  const auto ladder = [&](auto vt) {
    using VT = typename decltype(vt)::type;
    for_plan_lanes(A, [&](auto lanes) {
      const auto go = [&](auto ia, auto ib) {     // ONE pair of column streams, grouped where one is and VT can be
        constexpr int RG = decltype(lanes)::value, IA = decltype(ia)::value, IB = decltype(ib)::value;
        constexpr bool kGrp = IA != 0 && kHasGroupedForms<VT>;
        if (kGrp && grp) hipLaunchKernelGGL((csr_stream_dual_kernel<RG, EpiA, EpiB, IA, IB, kChunk, kGrp, VT>), grid, block, dyn_lds, st, va, vb, ga, gb, xa, xb, ea, eb);
        else hipLaunchKernelGGL((csr_stream_dual_kernel<RG, EpiA, EpiB, IA, IB, kChunk, false, VT>), grid, block, dyn_lds, st, va, vb, ga, gb, xa, xb, ea, eb);
      };
      if (ma == 0) go(Idx<0>{}, Idx<0>{});
      else if (ma == 2 && mb == 2) { if constexpr (kStageA && kStageB) go(Idx<2>{}, Idx<2>{}); }
      else if (ma == 2 && mb == 3) { if constexpr (kStageA && kPairB) go(Idx<2>{}, Idx<3>{}); }
      else if (ma == 2) { if constexpr (kStageA) go(Idx<2>{}, Idx<1>{}); }
      else if (mb == 2) { if constexpr (kStageB) go(Idx<1>{}, Idx<2>{}); }
      else go(Idx<1>{}, Idx<1>{});
    });
    NSS_CHECK_LAUNCH();
    return true;
  };
  constexpr bool kCodedForm = (FORMS & kCodes) != 0;
  if (kCodedForm && A.coded() && B.coded())               // both halves stream value codes
    return ladder(ValueTag<std::conditional_t<kCodedForm, Coded8, double>>{});
  return ladder(ValueTag<double>{});
}

// ---- the row-slot kernels: taken by exactly two launch sites (nss_csr_spmv_f64, C23 of nss_bpcg2_iterate) --------------
// the staged form an epilogue's operand takes in the row-slot kernel: 2 (one stored vector), 3 (a pair), 0 (none)
template <class Epi>
constexpr int slots_idx() {
  return EpiX<Epi>::type::kStageable ? 2 : (XPairable<typename EpiX<Epi>::type>::value ? 3 : 0);
}
// whether a launch of `Epi` over all rows of A goes to the row-slot kernel NOW: a copy valid for the current launch plan
// and codes in force (nss_csr_s::row_slots), and the staged form of this operand in force (pair mode)
template <class Epi>
inline bool takes_row_slots(const nss_csr_s& A) {
  constexpr int IDX = slots_idx<Epi>();
  if (IDX == 0 || A.m == 0 || A.nblk == 0 || !A.row_slots()) return false;
  return A.idx_mode(EpiX<Epi>::type::kStageable, XPairable<typename EpiX<Epi>::type>::value) == IDX;
}
inline const uint4v* slot_positions(const nss_csr_s& A) { return reinterpret_cast<const uint4v*>(A.slot_pos.get()); }
template <bool PK>
inline const typename SlotTail<PK>::type* slot_codes(const nss_csr_s& A) {
  return reinterpret_cast<const typename SlotTail<PK>::type*>(A.slot_code.get());
}
// f(bool_constant<PK>) for the layout of the copy
template <class F>
inline void for_slot_layout(bool packed, F&& f) {
  if (packed) f(std::true_type{});
  else f(std::false_type{});
}

// A x into `epi` by the row-slot kernel; false (nothing launched) when A does not take it
template <class Epi>
inline bool launch_csr_slots(const nss_csr_s& A, const double* x, const Epi& epi, hipStream_t st) {
  constexpr int IDX = slots_idx<Epi>();
  if constexpr (IDX == 0) return false;
  else {
    if (!takes_row_slots<Epi>(A)) return false;
    for_slot_layout(A.slot_packed, [&](auto pk) {
      constexpr bool PK = decltype(pk)::value;
      hipLaunchKernelGGL((csr_slots_kernel<Epi, IDX, PK>), dim3(nss_csr_s::grid(A.nblk)), dim3(kBlock), 0, st,
                         A.view(0, A.nblk, IDX), slot_positions(A), slot_codes<PK>(A), x, epi);
    });
    NSS_CHECK_LAUNCH();
    return true;
  }
}

// A and B in one launch of the row-slot kernels when both take them; false (nothing launched) otherwise
template <class EpiA, class EpiB>
inline bool launch_csr_slots_dual(const nss_csr_s& A, const double* xa, const EpiA& ea, const nss_csr_s& B,
                                  const double* xb, const EpiB& eb, hipStream_t st) {
  constexpr int IA = slots_idx<EpiA>(), IB = slots_idx<EpiB>();
  if constexpr (IA == 0 || IB == 0) return false;
  else {
    if (!takes_row_slots<EpiA>(A) || !takes_row_slots<EpiB>(B)) return false;
    if (A.slot_packed != B.slot_packed) return false;     // (one of the copies in the 24-byte layout: stream kernels)
#ifdef NSS_NO_DUAL        // measurements: the two halves as launches of their own
    return launch_csr_slots(A, xa, ea, st) && launch_csr_slots(B, xb, eb, st);
#else
    const int ga = nss_csr_s::grid(A.nblk), gb = nss_csr_s::grid(B.nblk);
    for_slot_layout(A.slot_packed, [&](auto pk) {
      constexpr bool PK = decltype(pk)::value;
      hipLaunchKernelGGL((csr_slots_dual_kernel<EpiA, EpiB, IA, IB, PK>), dim3(ga + gb), dim3(kBlock), 0, st,
                         A.view(0, A.nblk, IA), B.view(0, B.nblk, IB), slot_positions(A), slot_codes<PK>(A),
                         slot_positions(B), slot_codes<PK>(B), ga, gb, xa, xb, ea, eb);
    });
    NSS_CHECK_LAUNCH();
    return true;
#endif
  }
}

// y = alpha * A x + beta * y
struct EpiAxpby {
  double alpha, beta;
  double* __restrict__ y;
  const int32_t* __restrict__ done = nullptr;   // solver stop flag (device), or NULL
  struct Pre { double y = 0.0; };
  __device__ bool skip() const { return done != nullptr && *done != 0; }
  __device__ Pre fetch(int r) const { return Pre{beta != 0.0 ? y[r] : 0.0}; }
  __device__ void row(int r, double ax, const Pre& p) const {
    double t = alpha * ax;
    if (beta != 0.0) t = fma(beta, p.y, t);
    y[r] = t;
  }
  __device__ void finish(int, double*) const {}
};

}  // namespace nss

namespace nss {

// largest launch-plan generation among `ms` (NULL entries skipped): what a loop state records in `plan_gen` when it
// sizes its dot partials (the host computes the same from nss_csr_plan_generation)
inline int64_t plan_stamp(std::initializer_list<const nss_csr_s*> ms) {
  int64_t g = 0;
  for (const nss_csr_s* m : ms)
    if (m && m->plan_gen > g) g = m->plan_gen;
  return g;
}

// Refuse a loop state before any launch when a matrix of it was re-planned since its partials were sized (its kernels
// and sum launches take the CURRENT row-block counts), or when a partials buffer holds fewer entries than the
// workspace query asks for now.  need / cap: n counts.
inline void check_plan(const char* who, int64_t stamp, int64_t recorded, const int64_t* need, const int64_t* cap, int n) {
  if (stamp != recorded)
    throw Error(std::string("invalid argument: ") + who + ": a matrix of this state was re-planned (plan generation " +
                std::to_string(recorded) + " -> " + std::to_string(stamp) + ": nss_csr_plan_for_pairs, " +
                "nss_csr_plan_for_blocks or nss_amg_create_auxiliary) after its dot partials were sized; query the " +
                "workspace again, re-allocate and record plan_gen / cap_*");
  for (int i = 0; i < n; ++i)
    if (need[i] > cap[i])
      throw Error(std::string("invalid argument: ") + who + ": partials buffer " + char('a' + i) + " holds " +
                  std::to_string(cap[i]) + " entries, the launch plan needs " + std::to_string(need[i]));
}

}  // namespace nss
