// DeviceBuffer<T>: the one owner of a device allocation in the host layer - move-only, `count` elements of T, freed by its destructor. Everything else that
// holds a device pointer (DeviceScene, the queues, a `take` cut of a block) is a view: it is re-pointed where its buffer is resized and frees nothing.
// Two rules:
//   - No DeviceBuffer at namespace scope or in a `static`: its destructor would run after the HIP runtime has been torn down.
//   - The holder decides which device is current: whoever resizes, resets or destroys a buffer has called hipSetDevice for the device it lives on.
// Host only (no device members), and nothing but the runtime's C API: a plain C++ compiler with -D__HIP_PLATFORM_AMD__ takes it.
#pragma once

#include <hip/hip_runtime_api.h>

#pragma GCC visibility push(hidden)

template <typename T>
class DeviceBuffer {
 public:
  DeviceBuffer() = default;
  DeviceBuffer(const DeviceBuffer&) = delete;
  DeviceBuffer& operator=(const DeviceBuffer&) = delete;
  DeviceBuffer(DeviceBuffer&& o) noexcept : ptr_(o.ptr_), count_(o.count_) { o.ptr_ = nullptr; o.count_ = 0; }
  DeviceBuffer& operator=(DeviceBuffer&& o) noexcept {
    if (this != &o) { reset(); ptr_ = o.ptr_; count_ = o.count_; o.ptr_ = nullptr; o.count_ = 0; }
    return *this;
  }
  ~DeviceBuffer() { reset(); }

  T* get() const { return ptr_; }
  size_t count() const { return count_; }
  explicit operator bool() const { return ptr_ != nullptr; }

  void reset() {
    if (ptr_) (void) hipFree(ptr_);
    ptr_ = nullptr; count_ = 0;
  }
  // Frees, then allocates exactly `count` elements (0: only frees). On failure the buffer is empty. When to call it - on any change of size, or only to
  // grow - is the call site's policy.
  hipError_t resize(size_t count) {
    reset();
    if (count == 0) return hipSuccess;
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, sizeof(T) * count);
    if (e != hipSuccess) return e;
    ptr_ = static_cast<T*>(p); count_ = count;
    return hipSuccess;
  }
  // A device copy of a host array; a null `host` or no elements leave the buffer empty (and succeed).
  hipError_t assign(const T* host, size_t count) {
    const hipError_t e = resize(host ? count : 0);
    return (e != hipSuccess || !ptr_) ? e : hipMemcpy(ptr_, host, sizeof(T) * count, hipMemcpyHostToDevice);
  }

 private:
  T* ptr_ = nullptr;
  size_t count_ = 0;
};

#pragma GCC visibility pop
