// Stand-alone check of nss::DeviceBuffer (csrc/device_buffer.h) on the CPU: the two allocation functions the header
// only declares are supplied here over malloc / free, with live counters and a switch that makes the N-th allocation
// throw.  Built with -fsanitize=address,undefined; at exit the live count is 0, so LeakSanitizer and the counter agree.
#include "device_buffer.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <stdexcept>
#include <utility>

static long g_live = 0, g_allocs = 0, g_fail_at = 0;     // g_fail_at: the allocation (counted from 1) that throws; 0: none

namespace nss {
void* device_alloc(size_t bytes) {
  if (++g_allocs == g_fail_at) throw std::runtime_error("injected allocation failure");
  void* p = std::malloc(bytes);
  if (!p) throw std::runtime_error("out of memory");
  ++g_live;
  return p;
}
void device_free(void* p) noexcept {
  if (!p) return;
  --g_live;
  std::free(p);
}
}  // namespace nss

using nss::DeviceBuffer;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("FAILED line %d: %s (live %ld)\n", __LINE__, #cond, g_live); \
      return 1;                                                            \
    }                                                                      \
  } while (0)

namespace {
struct Handle {                            // like the handle structs: owners, a scalar and a view of one of the owners
  DeviceBuffer<int32_t> a, b;
  DeviceBuffer<double> c, d;
  DeviceBuffer<uint8_t> e;
  int count = 0;
  const double* view = nullptr;            // aliases c or nothing: never freed
  void fill(size_t n) {
    a.alloc(n);
    b.alloc(n);
    c.alloc(n);
    d.alloc(n);
    e.alloc(n);
    count = int(n);
    view = c;
  }
};

void fail_next(long nth) {
  g_allocs = 0;
  g_fail_at = nth;
}

int takes_pointer(const double* p) { return p != nullptr; }
}  // namespace

int main() {
  {  // the buffer on its own
    DeviceBuffer<double> x;
    CHECK(x.get() == nullptr && x.size() == 0 && !x && g_live == 0);
    x.alloc(0);
    CHECK(x.get() == nullptr && x.size() == 0 && g_live == 0);
    x.alloc(8);
    CHECK(x && x.size() == 8 && g_live == 1);
    x[7] = 3.0;                            // (the conversion to double*: all 8 elements are addressable)
    CHECK(takes_pointer(x) == 1);
    double* const first = x;
    x.alloc(16);                           // alloc over a live buffer frees the old one
    CHECK(x.size() == 16 && g_live == 1);
    (void)first;
    x.alloc(0);
    CHECK(!x && g_live == 0);

    x.alloc(4);
    DeviceBuffer<double> y(std::move(x));  // move construction
    CHECK(!x && x.size() == 0 && y && y.size() == 4 && g_live == 1);
    DeviceBuffer<double> z;
    z = std::move(y);                      // move assignment into an empty target
    CHECK(!y && z.size() == 4 && g_live == 1);
    DeviceBuffer<double> w(32);
    CHECK(g_live == 2);
    double* const kept = z;
    w = std::move(z);                      // ... into a live target: what it held is freed
    CHECK(!z && w.get() == kept && w.size() == 4 && g_live == 1);
    DeviceBuffer<double>& self = w;
    w = std::move(self);                   // self-move keeps the allocation
    CHECK(w.get() == kept && w.size() == 4 && g_live == 1);

    double* const raw = w.release();       // release gives up ownership
    CHECK(raw == kept && !w && w.size() == 0 && g_live == 1);
    w.reset();
    CHECK(g_live == 1);
    nss::device_free(raw);
    CHECK(g_live == 0);
    w.reset();                             // (reset of an empty buffer)
    CHECK(g_live == 0);
  }
  CHECK(g_live == 0);

  {  // five buffers, the third allocation throws: the unwinding frees the first two
    bool thrown = false;
    try {
      Handle h;
      fail_next(3);
      h.fill(10);
    } catch (const std::runtime_error&) {
      thrown = true;
    }
    fail_next(0);
    CHECK(thrown && g_live == 0);
  }
  {  // = {} frees everything and clears the scalars
    Handle h;
    h.fill(10);
    CHECK(g_live == 5 && h.view == h.c.get());
    h = {};
    CHECK(g_live == 0 && !h.a && !h.e && h.count == 0 && h.view == nullptr);
    h.fill(3);
    CHECK(g_live == 5);
  }
  CHECK(g_live == 0);
  {  // a unique_ptr to the struct, destroyed on the exception path
    bool thrown = false;
    try {
      std::unique_ptr<Handle> h(new Handle);
      h->fill(6);
      CHECK(g_live == 5);
      fail_next(2);
      h->fill(12);                         // a re-allocated, b throws: both generations go with the handle
    } catch (const std::runtime_error&) {
      thrown = true;
    }
    fail_next(0);
    CHECK(thrown && g_live == 0);
  }
  {  // a view that aliases a buffer member is not freed: the owner frees the allocation exactly once
    Handle h;
    h.fill(5);
    const double* const v = h.view;
    CHECK(v == h.c.get());
    h.view = nullptr;
    CHECK(g_live == 5 && h.c.get() == v);
    h.view = h.c;
    h.c.reset();                           // the owner goes; the (now dangling) view is not touched
    CHECK(g_live == 4);
    h.view = nullptr;
  }
  CHECK(g_live == 0);
  std::printf("device_buffer ok\n");
  return 0;
}
