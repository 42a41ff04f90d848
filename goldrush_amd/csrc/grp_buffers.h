// Owners of the engine's device buffers, page-locked host buffers and events: each frees what it holds when it goes
// out of scope, so a struct of them needs no hand-written destructor and an early return leaks nothing.  Plain host
// C++ over the HIP runtime API: nothing here knows the engine's context or its error reporting.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstdint>

// Device memory: the pointer and its capacity in elements.  Converts to T* where a kernel argument or a copy wants
// the address; it cannot be copied, so it is never passed to a kernel by value.
template<typename T>
struct DevBuf
{
  T* p = nullptr;
  uint64_t cap = 0; // elements

  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept
    : p(o.p)
    , cap(o.cap)
  {
    o.p = nullptr;
    o.cap = 0;
  }
  DevBuf& operator=(DevBuf&& o) noexcept
  {
    if (this != &o) {
      clear();
      p = o.p;
      cap = o.cap;
      o.p = nullptr;
      o.cap = 0;
    }
    return *this;
  }
  ~DevBuf() { clear(); }

  operator T*() const { return p; }

  void clear()
  {
    if (p) {
      (void)hipFree(p);
    }
    p = nullptr;
    cap = 0;
  }
  // frees, then allocates exactly n elements; empty on failure
  hipError_t reset(uint64_t n)
  {
    clear();
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(T));
    if (e != hipSuccess) {
      p = nullptr;
      return e;
    }
    cap = n;
    return hipSuccess;
  }
  // room for `want` elements; a grow takes a quarter more, so that a slowly rising size does not reallocate every call
  hipError_t ensure(uint64_t want) { return want <= cap ? hipSuccess : reset(want + want / 4 + 64); }
  // hands the memory to somebody else
  T* release()
  {
    T* q = p;
    p = nullptr;
    cap = 0;
    return q;
  }
};

// the buffers of a group that grows together are all freed before the first of them is allocated again
template<typename... B>
void
clear_all(B&... b)
{
  (b.clear(), ...);
}

// Page-locked host memory, same contract; the flags are given at allocation.  With hipHostMallocMapped it also holds
// `dev`, the address the device reads and writes the same memory at.
template<typename T>
struct HostBuf
{
  T* p = nullptr;
  T* dev = nullptr;
  uint64_t cap = 0; // elements

  HostBuf() = default;
  HostBuf(const HostBuf&) = delete;
  HostBuf& operator=(const HostBuf&) = delete;
  HostBuf(HostBuf&& o) noexcept
    : p(o.p)
    , dev(o.dev)
    , cap(o.cap)
  {
    o.release();
  }
  HostBuf& operator=(HostBuf&& o) noexcept
  {
    if (this != &o) {
      clear();
      p = o.p;
      dev = o.dev;
      cap = o.cap;
      o.release();
    }
    return *this;
  }
  ~HostBuf() { clear(); }

  operator T*() const { return p; }

  void clear()
  {
    if (p) {
      (void)hipHostFree(p);
    }
    release();
  }
  hipError_t reset(uint64_t n, unsigned int flags)
  {
    clear();
    hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), n * sizeof(T), flags);
    if (e != hipSuccess) {
      p = nullptr;
      return e;
    }
    if (flags & hipHostMallocMapped) {
      e = hipHostGetDevicePointer(reinterpret_cast<void**>(&dev), p, 0);
      if (e != hipSuccess) {
        clear();
        return e;
      }
    }
    cap = n;
    return hipSuccess;
  }
  T* release()
  {
    T* q = p;
    p = dev = nullptr;
    cap = 0;
    return q;
  }
};

struct Event
{
  hipEvent_t e = nullptr;

  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  Event(Event&& o) noexcept
    : e(o.e)
  {
    o.e = nullptr;
  }
  Event& operator=(Event&& o) noexcept
  {
    if (this != &o) {
      clear();
      e = o.e;
      o.e = nullptr;
    }
    return *this;
  }
  ~Event() { clear(); }

  operator hipEvent_t() const { return e; }

  void clear()
  {
    if (e) {
      (void)hipEventDestroy(e);
    }
    e = nullptr;
  }
  hipError_t create(unsigned int flags)
  {
    clear();
    const hipError_t r = hipEventCreateWithFlags(&e, flags);
    if (r != hipSuccess) {
      e = nullptr;
    }
    return r;
  }
};
