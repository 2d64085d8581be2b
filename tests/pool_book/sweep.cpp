// Sweep of the workspace pool's bookkeeping (csrc/host/pool_book.hpp) on the host, with fake pointers, against a
// brute-force model written here from the pool's rules, not from the header's containers:
//   * a request below 4 MiB, or any request under a cap of 0, is not pooled;
//   * a request gets the idle block of the smallest capacity >= bytes, among equal capacities the one given back first,
//     and only if capacity <= bytes + bytes / 4 + 64 MiB; otherwise a fresh block, recorded with the bytes asked for;
//   * a block given back becomes idle; while the idle bytes exceed the cap the largest idle block leaves, among equal
//     capacities the one given back last;
//   * a pointer the pool did not hand out is not the pool's.
//   steps     seeded sequences of requests and give-backs played the way pool.cpp plays them: on every step the block
//             handed out, the blocks evicted (in order) and the idle byte count must be the model's;
//   directed  the reuse window's two edges, the 4 MiB threshold, cap 0, first-in-first-out among equals, eviction,
//             unknown pointers;
//   caps      the cap from the text of DLAF_MI355X_POOL_GB.
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "pool_book.hpp"

using dlaf_mi355x::PoolBook;

static long g_steps = 0, g_directed = 0, g_caps = 0, g_failures = 0;
constexpr size_t kMiB = (size_t) 1 << 20, kGiB = (size_t) 1 << 30;

static void fail(const char* what, long x, long y) {
  if (++g_failures <= 20)
    std::fprintf(stderr, "FAIL %s (%ld, %ld)\n", what, x, y);
}

static void* fake_pointer() {
  static uintptr_t next = 0;
  return reinterpret_cast<void*>(++next * 0x1000);
}

// ------------------------------------------------------------------------------------------------ the model
struct ModelBlock {
  void* p;
  size_t capacity;
  long given_back;  // order of the give-backs
};
struct Model {
  size_t cap;
  std::vector<std::pair<void*, size_t>> live;
  std::vector<ModelBlock> idle;
  long clock = 0;

  bool pools(size_t bytes) const { return cap != 0 && bytes >= 4 * kMiB; }
  size_t idle_bytes() const {
    size_t sum = 0;
    for (const ModelBlock& b : idle)
      sum += b.capacity;
    return sum;
  }
  void* take(size_t bytes) {
    int best = -1;
    for (int i = 0; i < (int) idle.size(); ++i) {
      if (idle[i].capacity < bytes)
        continue;
      if (best < 0 || idle[i].capacity < idle[best].capacity ||
          (idle[i].capacity == idle[best].capacity && idle[i].given_back < idle[best].given_back))
        best = i;
    }
    if (best < 0 || idle[best].capacity > bytes + bytes / 4 + 64 * kMiB)
      return nullptr;
    void* p = idle[best].p;
    live.push_back({p, idle[best].capacity});
    idle.erase(idle.begin() + best);
    return p;
  }
  void record(void* p, size_t bytes) { live.push_back({p, bytes}); }
  size_t release(void* p) {
    for (size_t i = 0; i < live.size(); ++i)
      if (live[i].first == p) {
        const size_t capacity = live[i].second;
        live.erase(live.begin() + (long) i);
        return capacity;
      }
    return 0;
  }
  std::vector<void*> keep(void* p, size_t capacity) {
    idle.push_back({p, capacity, clock++});
    std::vector<void*> drop;
    while (idle_bytes() > cap && !idle.empty()) {
      int big = 0;
      for (int i = 1; i < (int) idle.size(); ++i)
        if (idle[i].capacity > idle[big].capacity ||
            (idle[i].capacity == idle[big].capacity && idle[i].given_back > idle[big].given_back))
          big = i;
      drop.push_back(idle[big].p);
      idle.erase(idle.begin() + big);
    }
    return drop;
  }
};

// ------------------------------------------------------------------------------------------------ seeded sequences
struct Rng {
  uint64_t s;
  uint32_t next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t) (s >> 33);
  }
};

static void sweep_sequences(int seeds, int steps_each) {
  // capacities in MiB: below and at the threshold, equal ones, and pairs inside / outside each other's reuse window
  const size_t sizes[] = {1, 3, 4, 5, 8, 8, 8, 16, 64, 84, 85, 100, 150, 200, 512};
  const size_t caps[] = {0, 48 * kMiB, 256 * kMiB, kGiB, 64 * kGiB};
  for (int seed = 0; seed < seeds; ++seed) {
    Rng rng{0x9E3779B97F4A7C15ull * (uint64_t) (seed + 1)};
    const size_t cap = caps[seed % 5];
    PoolBook book(cap);
    Model model{cap};
    std::vector<void*> held;
    for (int step = 0; step < steps_each; ++step) {
      ++g_steps;
      const uint32_t r = rng.next() % 100;
      if (held.empty() || r < 50) {  // pool_malloc
        const size_t bytes = sizes[rng.next() % 15] * kMiB + (rng.next() % 4 == 0 ? rng.next() % 4096 : 0);
        if (book.pools(bytes) != model.pools(bytes))
          fail("pools", seed, step);
        void* p = nullptr;
        if (model.pools(bytes)) {
          p = book.take(bytes);
          if (p != model.take(bytes))
            fail("take", seed, step);
          if (p == nullptr) {
            p = fake_pointer();
            book.record(p, bytes);
            model.record(p, bytes);
          }
        }
        else {
          p = fake_pointer();
        }
        held.push_back(p);
      }
      else {  // pool_free: of a block in hand, now and then of a pointer nobody handed out
        void* p;
        if (r < 55) {
          p = fake_pointer();
        }
        else {
          const size_t i = rng.next() % held.size();
          p = held[i];
          held.erase(held.begin() + (long) i);
        }
        const size_t capacity = book.release(p);
        if (capacity != model.release(p))
          fail("release", seed, step);
        else if (capacity != 0 && book.keep(p, capacity) != model.keep(p, capacity))
          fail("keep", seed, step);
      }
      if (book.idle_bytes() != model.idle_bytes() || book.idle_bytes() > cap)
        fail("idle bytes", seed, step);
    }
    // pool_release
    ++g_steps;
    std::vector<void*> all = book.drop_idle();
    if (all.size() != model.idle.size() || book.idle_bytes() != 0 || book.take(8 * kMiB) != nullptr)
      fail("drop_idle", seed, (long) all.size());
  }
}

// ------------------------------------------------------------------------------------------------ directed cases
static void expect(bool ok, const char* what) {
  ++g_directed;
  if (!ok)
    fail(what, g_directed, 0);
}

// a block of `bytes` that was handed out fresh and has come back
static std::vector<void*> give_back_fresh(PoolBook& book, void* p, size_t bytes) {
  book.record(p, bytes);
  return book.keep(p, book.release(p));
}

static void directed_cases() {
  void *a = fake_pointer(), *b = fake_pointer(), *c = fake_pointer(), *d = fake_pointer();
  {  // the reuse window of a 16 MiB request ends at 16 + 4 + 64 = 84 MiB
    PoolBook book(kGiB);
    give_back_fresh(book, a, 84 * kMiB);
    expect(book.take(84 * kMiB + 1) == nullptr, "a block smaller than the request");
    expect(book.take(16 * kMiB) == a, "a block just inside the reuse window");
    give_back_fresh(book, b, 84 * kMiB + 1);
    expect(book.take(16 * kMiB) == nullptr, "a block just outside the reuse window");
    expect(book.idle_bytes() == 84 * kMiB + 1, "a refused block stays idle");
  }
  {  // below 4 MiB: never pooled
    PoolBook book(kGiB);
    expect(!book.pools(4 * kMiB - 1), "4 MiB - 1 is not pooled");
    expect(book.pools(4 * kMiB), "4 MiB is pooled");
    expect(book.release(a) == 0, "a block that was not recorded is not the pool's");
    expect(book.idle_bytes() == 0, "nothing idle after a small block");
  }
  {  // cap 0: never pools, and keeps nothing
    PoolBook book(0);
    expect(!book.pools(kGiB), "cap 0 pools nothing");
    const std::vector<void*> drop = give_back_fresh(book, a, 8 * kMiB);
    expect(drop.size() == 1 && drop[0] == a, "cap 0 keeps nothing");
    expect(book.idle_bytes() == 0 && book.take(8 * kMiB) == nullptr, "cap 0 has nothing idle");
  }
  {  // three equal blocks given back and retaken come back in the same order, call after call (PoolScope)
    PoolBook book(kGiB);
    give_back_fresh(book, a, 8 * kMiB);
    give_back_fresh(book, b, 8 * kMiB);
    give_back_fresh(book, c, 8 * kMiB);
    for (int call = 0; call < 2; ++call) {
      expect(book.take(8 * kMiB) == a, "first in, first out: first");
      expect(book.take(8 * kMiB) == b, "first in, first out: second");
      expect(book.take(8 * kMiB) == c, "first in, first out: third");
      expect(book.take(8 * kMiB) == nullptr, "no fourth block");
      for (void* p : {a, b, c})
        book.keep(p, book.release(p));
    }
  }
  {  // Eviction.  The idle bytes never exceed the cap between calls and the largest block goes first, so one block
     // always suffices: the block given back if it is the largest, a block at least as large otherwise.
    PoolBook book(20 * kMiB);
    expect(give_back_fresh(book, a, 8 * kMiB).empty() && give_back_fresh(book, b, 6 * kMiB).empty() &&
               give_back_fresh(book, c, 5 * kMiB).empty(),
           "19 MiB under a cap of 20 MiB");
    // 16 MiB more exceed the cap by 15 MiB, more than any one of the blocks kept: the new block alone leaves
    const std::vector<void*> drop = give_back_fresh(book, d, 16 * kMiB);
    expect(drop.size() == 1 && drop[0] == d, "the largest block leaves");
    expect(book.idle_bytes() == 19 * kMiB, "the smaller blocks stay");
    PoolBook equal(20 * kMiB);
    give_back_fresh(equal, a, 10 * kMiB);
    give_back_fresh(equal, b, 10 * kMiB);
    const std::vector<void*> drop2 = give_back_fresh(equal, c, 9 * kMiB);
    expect(drop2.size() == 1 && drop2[0] == b, "among equal largest blocks the one given back last leaves");
    expect(equal.take(10 * kMiB) == a && equal.take(9 * kMiB) == c, "the others stay");
  }
  {  // unknown pointers, and a block given back twice
    PoolBook book(kGiB);
    give_back_fresh(book, a, 8 * kMiB);
    expect(book.release(b) == 0, "a pointer nobody handed out");
    expect(book.release(a) == 0, "an idle block is not live");
    expect(book.idle_bytes() == 8 * kMiB && book.take(8 * kMiB) == a, "the pool is as it was");
  }
}

static void cap_cases() {
  struct Case {
    const char* text;
    size_t want;
  };
  const Case cases[] = {{nullptr, 64 * kGiB}, {"0", 0},    {"0.5", kGiB / 2}, {"1.5", kGiB + kGiB / 2},
                        {"64", 64 * kGiB},    {"-2", 0},   {"lots", 0}};
  for (const Case& c : cases) {
    ++g_caps;
    if (PoolBook::parse_cap(c.text) != c.want)
      fail("parse_cap", g_caps, (long) (PoolBook::parse_cap(c.text) >> 20));
  }
}

int main() {
  sweep_sequences(20, 3000);
  directed_cases();
  cap_cases();
  std::printf("steps %ld directed %ld caps %ld failures %ld\n", g_steps, g_directed, g_caps, g_failures);
  return g_failures == 0 ? 0 : 1;
}
