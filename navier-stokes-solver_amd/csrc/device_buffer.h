// nss::DeviceBuffer<T>: the move-only owner of one device allocation.  Handle structs hold their device arrays as
// members of this type and set-up routines their temporaries as locals, so an array is freed exactly once -- when its
// owner goes, is reset or is assigned to -- on the normal path and on the exception path alike.
//
// The implicit conversion to T* keeps call sites as they are written for a raw pointer: kernel arguments, braced view
// initialisers, `if (A.val8)`, hipMemcpy(A.rowptr, ...), pointer comparisons.  A member that points at memory somebody
// else owns stays a plain pointer, with a comment that names the owner.
//
// No HIP header here: memory comes from the two functions below, defined once in the library (blas1.hip) over
// hipMalloc / hipFree.  They count the live allocations and their bytes (nss_device_memory).  The counts cover what
// goes through these two functions only: not torch's allocations, and not the IPC region of the mailbox transport.
//
// Objects that live as long as the process (scratch(), the ScratchPool) keep raw pointers and are never freed: a static
// object whose destructor calls into the HIP runtime at exit, after the runtime has torn down, can abort the process.
// There is no static DeviceBuffer.
#pragma once

#include <cstddef>

namespace nss {

void* device_alloc(size_t bytes);        // throws nss::Error
void device_free(void* p) noexcept;      // (NULL: nothing)

template <class T>
class DeviceBuffer {
 public:
  DeviceBuffer() = default;
  explicit DeviceBuffer(size_t count) { alloc(count); }
  DeviceBuffer(DeviceBuffer&& o) noexcept : p_(o.p_), n_(o.n_) {
    o.p_ = nullptr;
    o.n_ = 0;
  }
  DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_;
      n_ = o.n_;
      o.p_ = nullptr;
      o.n_ = 0;
    }
    return *this;
  }
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  ~DeviceBuffer() { reset(); }

  // `count` elements, uninitialised; what the buffer held is freed first.  alloc(0) leaves it empty.
  void alloc(size_t count) {
    reset();
    if (count == 0) return;
    p_ = static_cast<T*>(device_alloc(sizeof(T) * count));
    n_ = count;
  }
  void reset() noexcept {
    device_free(p_);
    p_ = nullptr;
    n_ = 0;
  }
  T* get() const { return p_; }
  size_t size() const { return n_; }
  // gives up ownership: the caller frees the allocation with device_free
  T* release() noexcept {
    T* p = p_;
    p_ = nullptr;
    n_ = 0;
    return p;
  }
  operator T*() const { return p_; }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};

}  // namespace nss
