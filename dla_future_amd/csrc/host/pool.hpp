// pool.hpp -- device workspaces: the pool of the eigensolver stages' large temporaries, and the plain allocations
// (dev_alloc, DevBuf) that fall back on it when the device is full.
#pragma once
#include <cstddef>
#include <vector>

#include "runtime.hpp"

namespace dlaf_mi355x {

// ------------------------------------------------------------------------------------------------
// Workspace pool of the widenings (eigensolver stages): the reference takes its device temporaries from Umpire pools
// (src/memory/memory_chunk.cpp, init.cpp:100-140); here hipMalloc / hipFree of the multi-gigabyte temporaries of
// bt_band_to_tridiagonal and the divide & conquer solver cost 0.25-0.5 s per solve on some boxes (measured:
// profiles/r04_eigensolver_alloc_phases.txt), so blocks of 4 MiB and more are kept for the next call instead of going
// back to the driver.  pool_free waits for the device first (what hipFree does implicitly).  DLAF_MI355X_POOL_GB caps
// what is kept (default 64, fractions honoured, 0 = no pool); pool_release() gives everything back (dlaf_finalize).
// Which block a request gets and which ones go when the cap is passed: pool_book.hpp.
hipError_t pool_malloc(void** p, size_t bytes);
hipError_t pool_free(void* p);
void pool_release();
size_t pool_idle_bytes();

// The owner of a function's (or a step's) pool workspaces: get() takes them, release() -- at the latest the destructor --
// gives them back IN THE ORDER THEY WERE TAKEN.  The pool hands out blocks of equal size first-in-first-out, so a
// buffer taken and released at the same position gets the same block on the next call; releasing in reverse order (one
// owner per buffer, destroyed as C++ destroys locals) would swap equal-sized neighbours between calls.  Memory that
// must go early -- to bound the peak, or to place the device synchronisation of pool_free -- gets a scope of its own or
// an explicit release() at that point.
class PoolScope {
public:
  PoolScope() = default;
  PoolScope(const PoolScope&) = delete;
  PoolScope& operator=(const PoolScope&) = delete;
  ~PoolScope() { release(); }
  // `elems` elements (at least one)
  template <class T>
  T* get(size_t elems) {
    void* p = nullptr;
    DLAF_HIP_CHECK(pool_malloc(&p, (elems > 0 ? elems : 1) * sizeof(T)));
    held_.push_back(p);
    return static_cast<T*>(p);
  }
  void release() {
    for (void* p : held_)
      DLAF_HIP_CHECK(pool_free(p));
    held_.clear();
  }

private:
  std::vector<void*> held_;
};

// hipMalloc of `elems` elements (at least one); an allocation that fails releases the workspace pool -- it may be
// holding what this allocation needs -- and is tried once more before it is fatal
template <class T>
T* dev_alloc(size_t elems) {
  T* p = nullptr;
  if (elems == 0)
    elems = 1;
  if (hipMalloc(reinterpret_cast<void**>(&p), elems * sizeof(T)) != hipSuccess) {
    (void) hipGetLastError();
    pool_release();
    DLAF_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&p), elems * sizeof(T)));
  }
  return p;
}

// a device allocation that lives as long as its scope (empty until alloc())
template <class T>
struct DevBuf {
  T* p = nullptr;
  DevBuf() = default;
  explicit DevBuf(size_t elems) { alloc(elems); }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { (void) hipFree(p); }
  void alloc(size_t elems) { p = dev_alloc<T>(elems); }
};

// The scratch stream of a host form or a transfer (uploads, downloads, tile transforms): non-blocking, lives as long as
// its scope.  Declare it BEFORE the matrices it serves: they are destroyed first, the stream after them.  The destructor
// does not wait: the owner calls sync() where the results are needed.
struct ScratchStream {
  hipStream_t s = nullptr;
  ScratchStream() { DLAF_HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); }
  ScratchStream(const ScratchStream&) = delete;
  ScratchStream& operator=(const ScratchStream&) = delete;
  ~ScratchStream() { (void) hipStreamDestroy(s); }
  operator hipStream_t() const { return s; }
  void sync() const { DLAF_HIP_CHECK(hipStreamSynchronize(s)); }
};

}  // namespace dlaf_mi355x
