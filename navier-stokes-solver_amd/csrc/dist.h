// Shared pieces of the row-partitioned native loops (dist.hip: BPCG v2; minres.hip: MINRES).
#pragma once

#include "bpcg2.h"
#include "p2p.h"

#include <vector>

struct nss_dist_s {
  void* comm = nullptr;
  int nranks = 1, rank = 0;
  hipStream_t xstream = nullptr;
  hipEvent_t ev_ready[3] = {nullptr, nullptr, nullptr};  // operand produced on C
  hipEvent_t ev_halo[3] = {nullptr, nullptr, nullptr};   // ghost tail filled on X
  void* lib = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  // per-phase profile of the native loop (nss_dist_profile_begin / _end): kProfMarks events per iteration
  std::vector<hipEvent_t> prof_ev;
  int prof_cap = 0, prof_iters = 0;
  // mailbox transport (nss_dist_attach_p2p): exchange() and the one-double all-reduces of every native partitioned
  // loop go through peer-mapped memory instead of RCCL (csrc/p2p.h)
  struct nss_p2p_s* p2p = nullptr;
  // condensed form on slabs (nss_dist_set_condensed): the halo of t0, read by the lift E^T t0 on the owned coupling
  // rows, and of the preconditioned vector y (= t1 before the extension), read by E y on the owned interior rows --
  // both in the layout of the loop's A operand
  nss_halo_t cond_lift{};
  nss_halo_t cond_ext{};
  bool has_cond = false;
};


// Smoothed-aggregation V(1,1)-cycle on a row-partitioned operator with REPLICATED coarse levels, applied
// natively inside the partitioned loops (distributed.DistributedAMG is the host-side twin): the finest level
// works on the slab (two halo exchanges of the iterate), the slab's share of the restricted residual is
// all-reduced (one coarse vector) and levels 1.. run redundantly on every rank.
struct nss_dist_amg_s {
  const nss_dist_s* d = nullptr;
  const nss_csr_s* A = nullptr;        // slab rows, columns [owned | ghosts]
  const nss_csr_s* R = nullptr;        // coarse rows x owned columns
  const nss_csr_s* P = nullptr;        // owned rows x coarse columns
  const double* wdinv = nullptr;       // omega / diag(A) on the slab
  const nss_amg_s* coarse = nullptr;   // levels 1.. (replicated)
  nss_halo_t halo{};                   // of the iterate x (ext = x's halo-extended buffer)
  int32_t channel = 0;                 // mailbox transport: the channel of halo's layout (nss_dist_amg_set_channel)
  int32_t n = 0, nc = 0;
  nss::DeviceBuffer<double> res, rc, rc_local, ec;   // work vectors
};

// The auxiliary-space term of MypreA, transform @ V(L) @ transform.T (templates/NavierStokesSIMPLE_iterative.py:336-337,
// 357,380,383), on slabs: the velocity slab's rows of `transform` (columns: this rank's nodal planes + ghosts), the nodal
// slab's rows of its transpose (columns: this rank's velocity dofs + ghosts) and the V-cycle on the stacked nodal
// Laplacian with replicated coarse levels (nss_dist_amg_s).  Per apply: halo exchange of the argument, of the nodal
// correction, the two of the V-cycle, and its coarse all-reduce.
struct nss_dist_aux_s {
  const nss_dist_s* d = nullptr;
  const nss_csr_s* TT = nullptr;       // nodal rows x velocity columns [owned | ghosts]
  const nss_csr_s* T = nullptr;        // velocity rows x nodal columns [owned | ghosts]
  const nss_dist_amg_s* amg = nullptr;
  nss_halo_t halo_x{};                 // of the velocity argument (ext = its halo-extended buffer)
  nss_halo_t halo_e{};                 // of the nodal correction
  nss_halo_t halo_y{};                 // of the loop's iterate t1 as A's operand (multiplicative form: residual x - A y)
  bool has_halo_y = false;
  int32_t ch_x = 0, ch_e = 0, ch_y = 0;   // mailbox transport: the channels of the three halos (nss_dist_aux_set_channels)
  int32_t n_u = 0, n_nodes = 0;
  nss::DeviceBuffer<double> r_aux;     // nodal work vector
};

namespace nss {

// y (+)= scale * T V(L) T^T b on the slab
void dist_aux_apply(const nss_dist_aux_s& a, double scale, const double* b, double* y, bool accumulate, hipStream_t st,
                    const int32_t* done);

// y = scale * V(b) on the slab; every kernel returns at once when *done != 0 (the collectives still run on all
// ranks, on unchanged buffers)
void dist_amg_apply(const nss_dist_amg_s& a, double scale, const double* b, double* y, hipStream_t st,
                    const int32_t* done);

constexpr int kNcclFloat64 = 8;
constexpr int kNcclSum = 0;

void nccl_check(const nss_dist_s& d, int rc, const char* what);
void check_halo(const nss_halo_t* h, const nss_csr_s& mat, const char* name);
// halo exchange of one or two SpMV operands (one grouped send/recv phase) on stream `st`; over the mailbox transport
// (nss_dist_attach_p2p) the first goes through channel 0, the second through channel 1
void exchange(const nss_dist_s& d, const nss_halo_t& h, hipStream_t st, const nss_halo_t* second = nullptr);
// halo exchange of one operand over the channel the caller names: over the mailbox transport p2p_exchange on `channel`
// (skipped on every rank once *done != 0), else exchange(d, h, st)
void exchange_on(const nss_dist_s& d, int channel, const nss_halo_t& h, const int32_t* done, hipStream_t st);
// dst = sum over the ranks of src (n doubles, device); without a communicator (one rank) a copy.  Over the mailbox
// transport n == 1 is the one-double all-reduce and n > 1 needs the transport's vector zone (p2p_allreduce_vec, which
// skips once *done != 0)
void allreduce_sum(const nss_dist_s& d, const double* src, double* dst, size_t n, hipStream_t st,
                   const int32_t* done = nullptr);

}  // namespace nss
