// Peer-to-peer transport of the row-partitioned loops over xGMI without a collective library on the critical path:
// every rank owns a small FINE-GRAINED region (mailbox + halo flags + landing zone) that its peers map through HIP IPC
// and write into with plain remote stores.
//
//   all-reduce of one double   inside the sum kernel that produced the local sum: lanes r < nranks store the value,
//                              split into two 8-byte words (32 bits of payload + the 32-bit sequence number each: an
//                              8-byte store is single-copy atomic, no fence needed), into slot [seq & 1][my rank] of peer
//                              r's mailbox, then spin on their own mailbox until the word pair of rank r carries this
//                              sequence number; thread 0 adds the nranks values IN RANK ORDER -- the same bits on every
//                              rank.  No extra launch, no host involvement; one xGMI store latency + the skew of the ranks.
//   halo exchange              "put": a small kernel copies the boundary runs of the operand straight into the landing
//                              zones of the neighbours (remote stores), fences, and the last workgroup of a segment
//                              raises the neighbour's flag to the sequence number; "wait + copy": every workgroup spins
//                              on the flags of this rank's sources, then moves its share of the landing zone behind the
//                              owned entries of the operand.
// Every spin is bounded (wall clock): a peer that never arrives stops the loop with an error code instead of hanging
// the GPU.  Two mailbox parities suffice: a rank cannot finish all-reduce q + 1 before every rank has entered it, i.e.
// left all-reduce q.  Every landing zone exists TWICE, used alternately by the exchanges of its layout: a neighbour may
// run one exchange ahead (BPCG v1 and MINRES exchange twice in a row without an all-reduce in between: its put of
// exchange e + 1 can arrive before this rank has copied exchange e out -- found by running the native BPCG v1 loop with
// two ranks), never two: its put of exchange e + 2 follows its wait for e + 1, i.e. this rank's put of e + 1, which this
// rank's stream orders behind its copy of e.
//   vector all-reduce          (optional "vector zone", nss_p2p_create_vec): dst[0 .. n) = sum over the ranks of src, added
//                              in rank order.  Every rank q contributes only inside one contiguous range [lo_q, hi_q)
//                              registered at set-up (zero elsewhere; the ranges are the same on every rank); "put" copies
//                              src[lo_q, hi_q) into segment q of every peer's vector zone and raises the peer's vector flag
//                              of q, "wait + add" spins on the flags of all peers, then adds, per entry and in rank order,
//                              the contributions of the ranks whose range covers it (skipping a rank = adding +0.0: no
//                              partial sum is -0.0, so the bits are those of the plain rank-ordered sum).  Per rank this
//                              moves (nranks - 1) (hi_q - lo_q) doubles -- about an all-gather -- instead of
//                              (nranks - 1) n.  The zone exists twice, used alternately: a peer can be at most one vector
//                              all-reduce ahead -- its put of v + 2 follows its wait for v + 1, which needs this rank's
//                              put of v + 1, which this rank's stream orders behind its add of v (the last read of the
//                              zone copy v and v + 2 share).  Once *done is set (the loop's stop flag, flipped by the
//                              same iteration on every rank from all-reduced scalars) both kernels return at once, as the
//                              exchanges of the compact loop do: every rank skips the same calls, nobody waits for a put
//                              that is not coming, and the sequence numbers still advance on the host.
#pragma once

#include "nss_common.h"

#include <vector>

namespace nss {

constexpr int kP2pMaxRanks = 16;
constexpr int kP2pMaxSegments = 8;
constexpr int kP2pMaxChannels = 4;    // operand layouts one handle serves (BPCG v2: t1; MINRES / BPCG v1: A's and B^T's operand)
constexpr unsigned long long kP2pTimeoutTicks = 300000000ull;   // wall_clock64 runs at 100 MHz: 3 s

struct P2pView {                      // what the kernels need (passed by value)
  unsigned long long* mail = nullptr;             // own mailbox: [2][nranks][2] words
  unsigned long long* const* peer_mail = nullptr; // DEVICE array [nranks]: the peers' mailboxes (own entry: `mail`)
  int32_t nranks = 1, rank = 0;
  uint32_t seq = 0;                   // sequence number of THIS collective (host counter, same order on every rank)
  int32_t* error = nullptr;           // device word: set to 1 on a timeout
};

__device__ __forceinline__ unsigned long long p2p_load(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void p2p_store(unsigned long long* p, unsigned long long v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Sum of `local` (taken from thread 0) over the ranks, evaluated by the calling workgroup (>= nranks threads, ALL must
// call); the result is valid in every thread.  A timeout sets the error word (the caller stops the loop).
// `lds`: >= kP2pMaxRanks doubles.
__device__ __forceinline__ double p2p_allreduce_sum(const P2pView& v, double local, double* lds) {
  const int t = threadIdx.x;
  __syncthreads();
  if (t == 0) lds[0] = local;
  __syncthreads();
  const double mine = lds[0];
  __syncthreads();
  const unsigned long long bits = (unsigned long long)__double_as_longlong(mine);
  const unsigned long long tag = (unsigned long long)v.seq << 32;
  const int par = int(v.seq & 1u);
  if (t < v.nranks) {
    unsigned long long* dst = v.peer_mail[t] + (size_t(par) * v.nranks + v.rank) * 2;
    p2p_store(dst, (bits & 0xffffffffull) | tag);
    p2p_store(dst + 1, (bits >> 32) | tag);
    const unsigned long long* src = v.mail + (size_t(par) * v.nranks + t) * 2;
    const unsigned long long t0 = wall_clock64();
    unsigned long long lo = p2p_load(src), hi = p2p_load(src + 1);
    while ((lo >> 32) != v.seq || (hi >> 32) != v.seq) {
      if (wall_clock64() - t0 > kP2pTimeoutTicks) {
        atomicExch(v.error, 1);
        break;
      }
      __builtin_amdgcn_s_sleep(1);
      lo = p2p_load(src);
      hi = p2p_load(src + 1);
    }
    lds[t] = __longlong_as_double((long long)((lo & 0xffffffffull) | (hi << 32)));
  }
  __syncthreads();
  double s = 0.0;
  for (int r = 0; r < v.nranks; ++r) s += lds[r];        // rank order: identical bits on every rank
  return s;
}

}  // namespace nss

// host side of the transport (p2p.hip)
struct nss_p2p_s {
  int32_t nranks = 1, rank = 0;
  char* region = nullptr;                    // own fine-grained region (hipExtMallocWithFlags; nss_p2p_destroy frees it
                                             // after the peers' mappings are closed)
  size_t region_bytes = 0;
  unsigned long long* mail = nullptr;        // region + 0
  std::vector<char*> peer_region;            // mapped peers (own: region), opened and closed by IPC handle: not owned
  nss::DeviceBuffer<unsigned long long*> d_peer_mail;   // device array [nranks]
  nss::DeviceBuffer<int32_t> d_error;
  nss::DeviceBuffer<int32_t> d_ticket;       // [kP2pMaxSegments] workgroup tickets of the put kernel
  uint32_t seq = 0;                          // host counter of collectives issued
  // One CHANNEL per operand layout this handle serves (bound at creation, numbered in the order of nss_p2p_create's
  // halos): its arrival flags (one per source rank), its landing zone, the own receive table and, after connect, where
  // the peers want our segments.  Every exchange names its channel by that index -- not by the identity of the
  // descriptor's host tables, which copies of one descriptor share and which an empty halo does not have (NULL).
  struct Channel {
    int32_t n_owned = 0;
    size_t flags_off = 0, landing_off = 0;   // byte offsets inside the own region (flags_off is the same in every region)
    int64_t landing_doubles = 0;
    size_t zone_bytes = 0;                   // distance of the two copies of the own landing zone
    mutable uint32_t count = 0;              // exchanges of this layout issued so far (host; the same on every rank)
    std::vector<int64_t> peer_zone_bytes;    // per destination rank: the distance of ITS two zones
    std::vector<int64_t> recv_off, recv_cnt; // per source rank: offset into the landing zone / count (0: none)
    std::vector<int64_t> peer_land_off;      // per destination rank: BYTE offset inside ITS region where our segment goes
  };
  std::vector<Channel> channels;
  // the vector zone (nss_p2p_create_vec; vec_n == 0: none): its layout depends only on (n, every rank's range), the
  // same on every rank, so its flags and segments sit at the same byte offsets in every region (nothing in the blob)
  int64_t vec_n = 0;
  std::vector<int64_t> vec_lo, vec_hi, vec_off;   // per rank: contribution range, offset of its segment in the zone
  size_t vec_flags_off = 0, vec_zone_off = 0, vec_zone_bytes = 0;
  uint32_t vec_count = 0;                          // vector all-reduces issued so far (picks the zone copy)
  bool connected = false;
  nss::P2pView view(uint32_t s) const { return nss::P2pView{mail, d_peer_mail, nranks, rank, s, d_error}; }
};

namespace nss {
// halo exchange of `h` (direct sends only) over channel `channel` (the index of its layout at creation) through that
// channel's landing zone: put + wait/copy on stream `st`.  The sequence number and the channel's count advance on every
// call, also when this rank's halo on the channel is empty: every rank issues the same exchanges, so the counters stay
// the same on every rank whatever the neighbourhood.
void p2p_exchange(nss_p2p_s& p, int channel, const nss_halo_t& h, const int32_t* done, hipStream_t st);
// dst[0] = sum over the ranks of src[0], the ranks' values added in rank order (one small launch)
void p2p_allreduce(nss_p2p_s& p, const double* src, double* dst, hipStream_t st);
// dst[0 .. n) = sum over the ranks of src[0 .. n) through the vector zone (n = the zone's size; put + wait/add on `st`).
// The sequence number advances on every call; with *done != 0 both kernels return at once (see the header comment).
void p2p_allreduce_vec(nss_p2p_s& p, const double* src, double* dst, const int32_t* done, hipStream_t st);
}  // namespace nss
