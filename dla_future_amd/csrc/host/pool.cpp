// pool.cpp -- the workspace pool's side towards the driver: the lock, hipMalloc / hipFree and the device
// synchronisation.  What to hand out and what to evict is PoolBook's answer (pool_book.hpp).
#include "pool.hpp"
#include "pool_book.hpp"

#include <cstdlib>
#include <mutex>

namespace dlaf_mi355x {

namespace {
struct Pool {
  std::mutex mu;
  PoolBook book{PoolBook::parse_cap(std::getenv("DLAF_MI355X_POOL_GB"))};
};
Pool& pool() {
  static Pool p;
  return p;
}
}  // namespace

hipError_t pool_malloc(void** p, size_t bytes) {
  Pool& pl = pool();
  if (!pl.book.pools(bytes))
    return hipMalloc(p, bytes);
  {
    std::lock_guard<std::mutex> lk(pl.mu);
    if ((*p = pl.book.take(bytes)) != nullptr)
      return hipSuccess;
  }
  hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess) {
    // out of memory with blocks kept: give them back and try once more
    (void) hipGetLastError();
    pool_release();
    e = hipMalloc(p, bytes);
  }
  if (e == hipSuccess) {
    std::lock_guard<std::mutex> lk(pl.mu);
    pl.book.record(*p, bytes);
  }
  return e;
}

hipError_t pool_free(void* p) {
  if (p == nullptr)
    return hipSuccess;
  Pool& pl = pool();
  size_t cap = 0;
  {
    std::lock_guard<std::mutex> lk(pl.mu);
    cap = pl.book.release(p);
  }
  if (cap == 0)
    return hipFree(p);
  (void) hipDeviceSynchronize();  // (hipFree's implicit synchronisation: nothing enqueued may still use the block)
  std::vector<void*> drop;
  {
    std::lock_guard<std::mutex> lk(pl.mu);
    drop = pl.book.keep(p, cap);
  }
  for (void* q : drop)
    (void) hipFree(q);
  return hipSuccess;
}

void pool_release() {
  Pool& pl = pool();
  std::vector<void*> drop;
  {
    std::lock_guard<std::mutex> lk(pl.mu);
    drop = pl.book.drop_idle();
  }
  for (void* q : drop)
    (void) hipFree(q);
}

size_t pool_idle_bytes() {
  Pool& pl = pool();
  std::lock_guard<std::mutex> lk(pl.mu);
  return pl.book.idle_bytes();
}

}  // namespace dlaf_mi355x
