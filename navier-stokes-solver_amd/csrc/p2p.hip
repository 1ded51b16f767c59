// Peer-to-peer transport over xGMI through IPC-mapped mailboxes and landing zones (see p2p.h).
#include "p2p.h"
#include "dist.h"

#include <cstring>
#include <memory>

namespace nss {

struct PutSeg {
  const double* src;            // first entry of the run inside this rank's operand
  double* dst;                  // where it goes: inside the neighbour's landing zone (remote)
  unsigned long long* flag;     // the neighbour's arrival flag of this rank (remote)
  int32_t cnt, wg0, nwg;        // doubles; first workgroup / workgroups of this segment in the launch
};
struct PutArgs {
  PutSeg seg[kP2pMaxSegments];
  int32_t nseg;
  uint32_t seq;
  int32_t* ticket;
  const int32_t* done;
};

constexpr int kPutPerWg = kBlock * 8;

__global__ __launch_bounds__(kBlock) void p2p_put_kernel(PutArgs a) {
  if (a.done && a.done[0] != 0) return;
  int sidx = 0;
  for (int i = 1; i < a.nseg; ++i)
    if (int(blockIdx.x) >= a.seg[i].wg0) sidx = i;
  const PutSeg& g = a.seg[sidx];
  const int base = (int(blockIdx.x) - g.wg0) * kPutPerWg;
  for (int i = base + int(threadIdx.x); i < base + kPutPerWg && i < g.cnt; i += kBlock)
    __builtin_nontemporal_store(g.src[i], g.dst + i);            // remote store over xGMI
  __threadfence_system();                                         // the data before the flag
  __syncthreads();
  if (threadIdx.x == 0) {
    const int t = atomicAdd(a.ticket + sidx, 1);
    if (t == g.nwg - 1) {                                          // last workgroup of this segment
      a.ticket[sidx] = 0;
      p2p_store(g.flag, (unsigned long long)a.seq);
    }
  }
}

struct WaitArgs {
  const unsigned long long* flags;   // own flags, one per source rank
  int32_t src_rank[kP2pMaxSegments];
  int32_t nsrc;
  uint32_t seq;
  const double* landing;
  double* dst;                       // operand + n_owned
  int64_t n;
  int32_t* error;
  const int32_t* done;
};

__global__ __launch_bounds__(kBlock) void p2p_wait_copy_kernel(WaitArgs a) {
  if (a.done && a.done[0] != 0) return;
  if (int(threadIdx.x) < a.nsrc) {
    const unsigned long long* f = a.flags + a.src_rank[threadIdx.x];
    const unsigned long long t0 = wall_clock64();
    while (p2p_load(f) < (unsigned long long)a.seq) {
      if (wall_clock64() - t0 > kP2pTimeoutTicks) {
        atomicExch(a.error, 1);
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
  }
  __threadfence_system();                                         // the flag before the data it announces
  __syncthreads();
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < a.n; i += stride)
    a.dst[i] = __builtin_nontemporal_load(a.landing + i);         // fine-grained memory: not cached
}

void p2p_exchange(nss_p2p_s& p, int channel, const nss_halo_t& h, const int32_t* done, hipStream_t st) {
  if (!p.connected) throw Error("p2p: not connected");
  if (channel < 0 || channel >= int(p.channels.size()))
    throw Error("p2p: no such channel (the halo layout was not registered when the transport was created)");
  if (h.n_send > 0 && !h.direct) throw Error("p2p: the halo must send contiguous runs of the operand (direct)");
  if (h.n_send > kP2pMaxSegments || h.n_recv > kP2pMaxSegments) throw Error("p2p: too many neighbours");
  const nss_p2p_s::Channel* ch = &p.channels[size_t(channel)];
  for (int i = 0; i < h.n_recv; ++i) {              // the halo must have the receive layout the channel was made for
    const int q = h.h_recv_peer[i];
    if (q < 0 || q >= p.nranks || ch->recv_cnt[size_t(q)] != h.h_recv_cnt[i] ||
        ch->recv_off[size_t(q)] != h.h_recv_off[i] - ch->n_owned)
      throw Error("p2p: the halo's receive layout is not the one of channel " + std::to_string(channel));
  }
  // advanced before anything can return: a rank with an empty halo on this channel still takes part in the numbering
  // (its neighbours' all-reduces and later exchanges carry the same sequence numbers)
  const uint32_t seq = ++p.seq;
  const size_t par = size_t(ch->count++ & 1u);                  // which of the two landing zones this exchange uses
  if (h.n_send == 0 && h.n_recv == 0) return;                     // no neighbour on this channel (one rank)
  if (h.n_send > 0) {
    PutArgs a{};
    int wg = 0;
    for (int i = 0; i < h.n_send; ++i) {
      const int peer = h.h_send_peer[i];
      const int64_t cnt = h.h_send_cnt[i];
      if (ch->peer_land_off[size_t(peer)] < 0) throw Error("p2p: a neighbour does not expect our segment");
      char* pr = p.peer_region[size_t(peer)];
      unsigned long long* pflags = reinterpret_cast<unsigned long long*>(pr + ch->flags_off);   // (same offset in every region)
      double* pdst = reinterpret_cast<double*>(pr + ch->peer_land_off[size_t(peer)] +          // byte offset the peer published
                                               par * size_t(ch->peer_zone_bytes[size_t(peer)]));
      a.seg[i] = PutSeg{h.ext + h.h_send_off[i], pdst, pflags + p.rank, int32_t(cnt), wg,
                        int((cnt + kPutPerWg - 1) / kPutPerWg)};
      wg += a.seg[i].nwg;
    }
    a.nseg = h.n_send;
    a.seq = seq;
    a.ticket = p.d_ticket;
    a.done = done;
    hipLaunchKernelGGL(p2p_put_kernel, dim3(wg), dim3(kBlock), 0, st, a);
    NSS_CHECK_LAUNCH();
  }
  if (h.n_recv > 0) {
    WaitArgs w{};
    int64_t total = 0;
    for (int i = 0; i < h.n_recv; ++i) {
      w.src_rank[i] = h.h_recv_peer[i];
      if (h.h_recv_off[i] - ch->n_owned != total) throw Error("p2p: receive segments must fill the ghost tail in order");
      total += h.h_recv_cnt[i];
    }
    if (total > ch->landing_doubles) throw Error("p2p: landing zone too small");
    w.flags = reinterpret_cast<const unsigned long long*>(p.region + ch->flags_off);
    w.nsrc = h.n_recv;
    w.seq = seq;
    w.landing = reinterpret_cast<const double*>(p.region + ch->landing_off + par * ch->zone_bytes);
    w.dst = h.ext + ch->n_owned;
    w.n = total;
    w.error = p.d_error;
    w.done = done;
    hipLaunchKernelGGL(p2p_wait_copy_kernel, dim3(stream_grid(total, kBlock * 4)), dim3(kBlock), 0, st, w);
    NSS_CHECK_LAUNCH();
  }
}

__global__ __launch_bounds__(kBlock) void p2p_allreduce_kernel(P2pView v, const double* src, double* dst) {
  __shared__ double lds[kP2pMaxRanks];
  const double s = p2p_allreduce_sum(v, threadIdx.x == 0 ? src[0] : 0.0, lds);
  if (threadIdx.x == 0) dst[0] = s;
}

void p2p_allreduce(nss_p2p_s& p, const double* src, double* dst, hipStream_t st) {
  if (!p.connected) throw Error("p2p: not connected");
  hipLaunchKernelGGL(p2p_allreduce_kernel, dim3(1), dim3(kBlock), 0, st, p.view(++p.seq), src, dst);
  NSS_CHECK_LAUNCH();
}

struct VecAddArgs {
  const unsigned long long* flags;   // own vector flags, one per source rank
  int64_t lo[kP2pMaxRanks], hi[kP2pMaxRanks], off[kP2pMaxRanks];
  int32_t nranks, rank;
  uint32_t seq;
  const double* zone;                // the zone copy of this call
  const double* src;                 // own contribution (read inside [lo[rank], hi[rank]) only)
  double* dst;
  int64_t n;
  int32_t* error;
  const int32_t* done;
};

__global__ __launch_bounds__(kBlock) void p2p_vec_wait_add_kernel(VecAddArgs a) {
  if (a.done && a.done[0] != 0) return;
  const int t = int(threadIdx.x);
  if (t < a.nranks && t != a.rank) {
    const unsigned long long* f = a.flags + t;
    const unsigned long long t0 = wall_clock64();
    while (p2p_load(f) < (unsigned long long)a.seq) {
      if (wall_clock64() - t0 > kP2pTimeoutTicks) {
        atomicExch(a.error, 1);
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
  }
  __threadfence_system();                                         // the flags before the data they announce
  __syncthreads();
  const int64_t stride = int64_t(gridDim.x) * kBlock;
  for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < a.n; i += stride) {
    double s = 0.0;
    for (int q = 0; q < a.nranks; ++q) {                           // rank order: identical bits on every rank
      if (i < a.lo[q] || i >= a.hi[q]) continue;                   // outside q's range its contribution is zero
      s += q == a.rank ? a.src[i] : __builtin_nontemporal_load(a.zone + a.off[q] + (i - a.lo[q]));
    }
    a.dst[i] = s;
  }
}

void p2p_allreduce_vec(nss_p2p_s& p, const double* src, double* dst, const int32_t* done, hipStream_t st) {
  if (!p.connected) throw Error("p2p: not connected");
  if (p.vec_n <= 0) throw Error("p2p: no vector zone (nss_p2p_create_vec)");
  const uint32_t seq = ++p.seq;                                    // advanced on every rank, in the same order
  const size_t par = size_t(p.vec_count++ & 1u);
  const int me = p.rank;
  const int64_t lo = p.vec_lo[size_t(me)], cnt = p.vec_hi[size_t(me)] - lo;
  // put: segment `me` of every peer's zone copy `par`, then the peer's vector flag of `me` -- also for an empty range
  // (one workgroup that only raises the flag); at most kP2pMaxSegments peers per launch
  std::vector<int> peers;
  for (int q = 0; q < p.nranks; ++q)
    if (q != me) peers.push_back(q);
  const int nwg = int(std::max<int64_t>(1, (cnt + kPutPerWg - 1) / kPutPerWg));
  for (size_t first = 0; first < peers.size(); first += kP2pMaxSegments) {
    PutArgs a{};
    int wg = 0;
    for (size_t i = first; i < peers.size() && i < first + kP2pMaxSegments; ++i) {
      char* pr = p.peer_region[size_t(peers[i])];
      double* pdst = reinterpret_cast<double*>(pr + p.vec_zone_off + par * p.vec_zone_bytes) + p.vec_off[size_t(me)];
      unsigned long long* pflag = reinterpret_cast<unsigned long long*>(pr + p.vec_flags_off) + me;
      a.seg[a.nseg++] = PutSeg{src + lo, pdst, pflag, int32_t(cnt), wg, nwg};
      wg += nwg;
    }
    a.seq = seq;
    a.ticket = p.d_ticket;
    a.done = done;
    hipLaunchKernelGGL(p2p_put_kernel, dim3(wg), dim3(kBlock), 0, st, a);
    NSS_CHECK_LAUNCH();
  }
  VecAddArgs w{};
  w.flags = reinterpret_cast<const unsigned long long*>(p.region + p.vec_flags_off);
  for (int q = 0; q < p.nranks; ++q) {
    w.lo[q] = p.vec_lo[size_t(q)];
    w.hi[q] = p.vec_hi[size_t(q)];
    w.off[q] = p.vec_off[size_t(q)];
  }
  w.nranks = p.nranks;
  w.rank = me;
  w.seq = seq;
  w.zone = reinterpret_cast<const double*>(p.region + p.vec_zone_off + par * p.vec_zone_bytes);
  w.src = src;
  w.dst = dst;
  w.n = p.vec_n;
  w.error = p.d_error;
  w.done = done;
  hipLaunchKernelGGL(p2p_vec_wait_add_kernel, dim3(stream_grid(p.vec_n, kBlock * 4)), dim3(kBlock), 0, st, w);
  NSS_CHECK_LAUNCH();
}

}  // namespace nss

using namespace nss;

namespace {
size_t mail_bytes(int nranks) { return sizeof(unsigned long long) * 2 * size_t(nranks) * 2; }
size_t flags_bytes() { return sizeof(unsigned long long) * size_t(kP2pMaxRanks); }
size_t chan_blob(int nranks) { return size_t(16) * nranks + 8; }   // where[nranks] | count[nranks] | zone_bytes
size_t blob_bytes(int nranks, int nchan) { return 64 + chan_blob(nranks) * nchan; }
}  // namespace

extern "C" {

// blob layout (what every rank publishes): 64 bytes IPC handle | per channel: int64 byte offset (inside the publisher's
// region) where rank q's segment goes, q < nranks (-1: nothing); int64 count from rank q; int64 distance of its two zones
int nss_p2p_blob_bytes(int32_t nranks, int32_t nhalo, int64_t* bytes) {
  return guarded([&] {
    NSS_REQUIRE(nranks >= 1 && nranks <= kP2pMaxRanks && nhalo >= 1 && nhalo <= kP2pMaxChannels && bytes, "p2p_blob_bytes: bad argument");
    *bytes = int64_t(blob_bytes(nranks, nhalo));
  });
}

}  // extern "C"

namespace {
// nss_p2p_create (vec_n == 0: the layout and blob of a transport without vector zone) and nss_p2p_create_vec
int p2p_create(int32_t nranks, int32_t rank, int32_t nhalo, const nss_halo_t* const* halos, const int32_t* n_owned,
               int64_t vec_n, const int64_t* vec_lo, const int64_t* vec_hi, nss_p2p_t* out, void* h_blob) {
  return guarded([&] {
    NSS_REQUIRE(out && h_blob && halos && n_owned, "p2p_create: NULL argument");
    NSS_REQUIRE(nranks >= 1 && nranks <= kP2pMaxRanks && rank >= 0 && rank < nranks, "p2p_create: bad rank / size (at most 16 ranks)");
    NSS_REQUIRE(nhalo >= 1 && nhalo <= kP2pMaxChannels, "p2p_create: 1 .. 4 operand layouts");
    std::unique_ptr<nss_p2p_s, int (*)(nss_p2p_t)> p(new nss_p2p_s, nss_p2p_destroy);   // (unmaps and frees the region)
    p->nranks = nranks;
    p->rank = rank;
    size_t off = mail_bytes(nranks);
    for (int c = 0; c < nhalo; ++c) {
      const nss_halo_t* halo = halos[c];
      NSS_REQUIRE(halo != nullptr, "p2p_create: NULL halo");
      NSS_REQUIRE(halo->direct || halo->n_send == 0, "p2p_create: the halos must send contiguous runs (direct)");
      nss_p2p_s::Channel ch;
      ch.n_owned = n_owned[c];
      ch.recv_off.assign(size_t(nranks), -1);
      ch.recv_cnt.assign(size_t(nranks), 0);
      int64_t total = 0;
      for (int i = 0; i < halo->n_recv; ++i) {
        const int q = halo->h_recv_peer[i];
        NSS_REQUIRE(q >= 0 && q < nranks && q != rank, "p2p_create: bad source rank");
        ch.recv_off[size_t(q)] = halo->h_recv_off[i] - n_owned[c];
        ch.recv_cnt[size_t(q)] = halo->h_recv_cnt[i];
        total += halo->h_recv_cnt[i];
      }
      ch.landing_doubles = std::max<int64_t>(total, 1);
      ch.flags_off = off;
      off += flags_bytes();
      p->channels.push_back(ch);
    }
    if (vec_n > 0) {   // vector zone: flags, then two copies of the segments of all ranks (the same in every region)
      NSS_REQUIRE(vec_lo && vec_hi, "p2p_create: NULL contribution range");
      int64_t total = 0;
      for (int q = 0; q < nranks; ++q) {
        NSS_REQUIRE(0 <= vec_lo[q] && vec_lo[q] <= vec_hi[q] && vec_hi[q] <= vec_n,
                    "p2p_create: contribution range outside [0, n)");
        p->vec_lo.push_back(vec_lo[q]);
        p->vec_hi.push_back(vec_hi[q]);
        p->vec_off.push_back(total);
        total += vec_hi[q] - vec_lo[q];
      }
      p->vec_n = vec_n;
      p->vec_flags_off = off;
      off += flags_bytes();
      off = (off + 255) & ~size_t(255);
      p->vec_zone_off = off;
      p->vec_zone_bytes = (sizeof(double) * size_t(std::max<int64_t>(total, 1)) + 255) & ~size_t(255);
      off += 2 * p->vec_zone_bytes;
    }
    // landing zones behind all flag rows; their sizes differ from rank to rank, so every rank publishes ITS offsets
    // relative to a layout that only depends on (nranks, nhalo): zone c starts at a 256-byte aligned offset that the
    // OWNER computes -- the sender needs the owner's value, which travels in the blob
    for (int c = 0; c < nhalo; ++c) {
      off = (off + 255) & ~size_t(255);
      p->channels[size_t(c)].landing_off = off;
      p->channels[size_t(c)].zone_bytes = (sizeof(double) * size_t(p->channels[size_t(c)].landing_doubles) + 255) & ~size_t(255);
      off += 2 * p->channels[size_t(c)].zone_bytes;
    }
    p->region_bytes = off;
    // fine-grained device memory: remote stores become visible to this GPU's loads without cache maintenance
    void* mem = nullptr;
    NSS_HIP(hipExtMallocWithFlags(&mem, p->region_bytes, hipDeviceMallocFinegrained));
    p->region = static_cast<char*>(mem);
    NSS_HIP(hipMemset(p->region, 0, p->region_bytes));
    p->mail = reinterpret_cast<unsigned long long*>(p->region);
    p->d_error.alloc(1);
    NSS_HIP(hipMemset(p->d_error, 0, sizeof(int32_t)));
    p->d_ticket.alloc(kP2pMaxSegments);
    NSS_HIP(hipMemset(p->d_ticket, 0, sizeof(int32_t) * kP2pMaxSegments));
    NSS_HIP(hipDeviceSynchronize());
    hipIpcMemHandle_t handle;
    NSS_HIP(hipIpcGetMemHandle(&handle, p->region));
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "IPC handle size");
    char* blob = static_cast<char*>(h_blob);
    std::memcpy(blob, &handle, 64);
    for (int c = 0; c < nhalo; ++c) {
      // what the senders need: where (in bytes from the start of MY region) rank q's segment goes, and how long it is
      std::vector<int64_t> where(size_t(nranks), -1);
      for (int q = 0; q < nranks; ++q)
        if (p->channels[size_t(c)].recv_off[size_t(q)] >= 0)
          where[size_t(q)] = int64_t(p->channels[size_t(c)].landing_off) + 8 * p->channels[size_t(c)].recv_off[size_t(q)];
      char* at = blob + 64 + chan_blob(nranks) * c;
      std::memcpy(at, where.data(), sizeof(int64_t) * size_t(nranks));
      std::memcpy(at + 8 * size_t(nranks), p->channels[size_t(c)].recv_cnt.data(), sizeof(int64_t) * size_t(nranks));
      const int64_t zb = int64_t(p->channels[size_t(c)].zone_bytes);
      std::memcpy(at + 16 * size_t(nranks), &zb, sizeof(int64_t));
    }
    *out = p.release();
  });
}
}  // namespace

extern "C" {

int nss_p2p_create(int32_t nranks, int32_t rank, int32_t nhalo, const nss_halo_t* const* halos, const int32_t* n_owned,
                   nss_p2p_t* out, void* h_blob) {
  return p2p_create(nranks, rank, nhalo, halos, n_owned, 0, nullptr, nullptr, out, h_blob);
}

int nss_p2p_create_vec(int32_t nranks, int32_t rank, int32_t nhalo, const nss_halo_t* const* halos, const int32_t* n_owned,
                       int64_t vec_n, const int64_t* vec_lo, const int64_t* vec_hi, nss_p2p_t* out, void* h_blob) {
  if (vec_n < 1) return guarded([] { throw Error("p2p_create_vec: the vector zone needs n >= 1"); });
  return p2p_create(nranks, rank, nhalo, halos, n_owned, vec_n, vec_lo, vec_hi, out, h_blob);
}

int nss_p2p_connect(nss_p2p_t p, const void* h_blobs) {
  return guarded([&] {
    NSS_REQUIRE(p && h_blobs, "p2p_connect: NULL argument");
    NSS_REQUIRE(!p->connected, "p2p_connect: already connected");
    const int nchan = int(p->channels.size());
    const size_t blob = blob_bytes(p->nranks, nchan);
    const char* all = static_cast<const char*>(h_blobs);
    p->peer_region.assign(size_t(p->nranks), nullptr);
    for (nss_p2p_s::Channel& ch : p->channels) {
      ch.peer_land_off.assign(size_t(p->nranks), -1);
      ch.peer_zone_bytes.assign(size_t(p->nranks), 0);
    }
    std::vector<unsigned long long*> mails(size_t(p->nranks), nullptr);
    for (int q = 0; q < p->nranks; ++q) {
      if (q == p->rank) {
        p->peer_region[size_t(q)] = p->region;
      } else {
        hipIpcMemHandle_t handle;
        std::memcpy(&handle, all + blob * size_t(q), 64);
        void* mapped = nullptr;
        NSS_HIP(hipIpcOpenMemHandle(&mapped, handle, hipIpcMemLazyEnablePeerAccess));
        p->peer_region[size_t(q)] = static_cast<char*>(mapped);
        for (int c = 0; c < nchan; ++c) {
          int64_t where = -1;                              // byte offset inside q's region where q wants OUR segment
          const char* at = all + blob * size_t(q) + 64 + chan_blob(p->nranks) * c;
          std::memcpy(&where, at + 8 * size_t(p->rank), sizeof(int64_t));
          int64_t zb = 0;
          std::memcpy(&zb, at + 16 * size_t(p->nranks), sizeof(int64_t));
          p->channels[size_t(c)].peer_land_off[size_t(q)] = where;      // (the zones of different ranks start at different offsets)
          p->channels[size_t(c)].peer_zone_bytes[size_t(q)] = zb;
        }
      }
      mails[size_t(q)] = reinterpret_cast<unsigned long long*>(p->peer_region[size_t(q)]);
    }
    p->d_peer_mail.alloc(size_t(p->nranks));
    NSS_HIP(hipMemcpy(p->d_peer_mail, mails.data(), sizeof(unsigned long long*) * size_t(p->nranks), hipMemcpyHostToDevice));
    p->connected = true;
  });
}

int nss_p2p_destroy(nss_p2p_t p) {
  return guarded([&] {
    if (!p) return;
    (void)hipDeviceSynchronize();
    for (int q = 0; q < int(p->peer_region.size()); ++q)
      if (q != p->rank && p->peer_region[size_t(q)]) (void)hipIpcCloseMemHandle(p->peer_region[size_t(q)]);
    (void)hipFree(p->region);                              // (hipExtMallocWithFlags: not counted by nss_device_memory)
    delete p;
  });
}

int nss_p2p_allreduce_f64(nss_p2p_t p, const double* src, double* dst, nss_stream_t stream) {
  return guarded([&] {
    NSS_REQUIRE(p && src && dst, "p2p_allreduce: bad argument");
    p2p_allreduce(*p, src, dst, as_stream(stream));
  });
}

int nss_p2p_allreduce_vec_f64(nss_p2p_t p, const double* src, double* dst, nss_stream_t stream) {
  return guarded([&] {
    NSS_REQUIRE(p && src && dst, "p2p_allreduce_vec: bad argument");
    p2p_allreduce_vec(*p, src, dst, nullptr, as_stream(stream));
  });
}

int nss_p2p_exchange(nss_p2p_t p, int32_t channel, const nss_halo_t* halo, nss_stream_t stream) {
  return guarded([&] {
    NSS_REQUIRE(p && halo, "p2p_exchange: NULL argument");
    p2p_exchange(*p, channel, *halo, nullptr, as_stream(stream));
  });
}

int nss_p2p_counters(nss_p2p_t p, int64_t* seq, int32_t max_channels, int64_t* counts, int32_t* n_channels) {
  return guarded([&] {
    NSS_REQUIRE(p && seq && n_channels && max_channels >= 0 && (counts || max_channels == 0), "p2p_counters: bad argument");
    *seq = int64_t(p->seq);
    *n_channels = int32_t(p->channels.size());
    for (int c = 0; c < max_channels && c < int(p->channels.size()); ++c) counts[c] = int64_t(p->channels[size_t(c)].count);
  });
}

int nss_p2p_error(nss_p2p_t p, int32_t* timed_out, nss_stream_t stream) {
  return guarded([&] {
    NSS_REQUIRE(p && timed_out, "p2p_error: NULL argument");
    NSS_HIP(hipMemcpyAsync(timed_out, p->d_error, sizeof(int32_t), hipMemcpyDeviceToHost, as_stream(stream)));
    NSS_HIP(hipStreamSynchronize(as_stream(stream)));
  });
}

}  // extern "C"
