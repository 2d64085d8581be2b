// pool_book.hpp -- the bookkeeping of the workspace pool (pool.hpp) without the driver: which idle block a request
// gets, which blocks go back to the driver when the idle bytes pass the cap.  No HIP header and no lock: pool.cpp holds
// the mutex and does what the answers say; tests/pool_book/sweep.cpp replays sequences against a brute-force model.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <iterator>
#include <map>
#include <vector>

namespace dlaf_mi355x {

class PoolBook {
public:
  // the cap in bytes from the text of DLAF_MI355X_POOL_GB (GiB, fractions honoured): unset 64, negative or no number 0
  static size_t parse_cap(const char* gb) {
    return (size_t) ((gb ? std::max(0.0, std::atof(gb)) : 64.0) * (double) ((size_t) 1 << 30));
  }
  explicit PoolBook(size_t cap_bytes) : cap_(cap_bytes) {}
  size_t idle_bytes() const { return idle_bytes_; }
  // requests below 4 MiB, and every request under a cap of 0, are not the pool's business
  bool pools(size_t bytes) const { return bytes >= ((size_t) 4 << 20) && cap_ != 0; }

  // the idle block (now live) of the smallest capacity >= bytes, the one given back FIRST among equal capacities
  // (PoolScope rests on that), if that is no more than bytes + bytes / 4 + 64 MiB; or nullptr
  void* take(size_t bytes) {
    auto it = idle_.lower_bound(bytes);
    if (it == idle_.end() || it->first > bytes + bytes / 4 + ((size_t) 64 << 20))
      return nullptr;
    void* p = it->second;
    live_[p] = it->first;
    idle_bytes_ -= it->first;
    idle_.erase(it);
    return p;
  }
  // a block of `bytes` fresh from the driver, handed out: the pool's from now on
  void record(void* p, size_t bytes) { live_[p] = bytes; }
  // p comes back: its capacity, 0 for a pointer the pool never handed out (the caller frees that one itself)
  size_t release(void* p) {
    auto it = live_.find(p);
    if (it == live_.end())
      return 0;
    const size_t capacity = it->second;
    live_.erase(it);
    return capacity;
  }
  // the released block becomes idle; returns the blocks that leave the pool to stay under the cap, largest first (the
  // one given back last among equals)
  std::vector<void*> keep(void* p, size_t capacity) {
    std::vector<void*> drop;
    idle_.emplace(capacity, p);
    idle_bytes_ += capacity;
    while (idle_bytes_ > cap_ && !idle_.empty()) {
      auto big = std::prev(idle_.end());
      drop.push_back(big->second);
      idle_bytes_ -= big->first;
      idle_.erase(big);
    }
    return drop;
  }
  // every idle block leaves the pool
  std::vector<void*> drop_idle() {
    std::vector<void*> drop;
    for (auto& kv : idle_)
      drop.push_back(kv.second);
    idle_.clear();
    idle_bytes_ = 0;
    return drop;
  }

private:
  const size_t cap_;
  std::map<void*, size_t> live_;       // handed out: pointer -> capacity
  std::multimap<size_t, void*> idle_;  // kept: capacity -> pointer
  size_t idle_bytes_ = 0;
};

}  // namespace dlaf_mi355x
