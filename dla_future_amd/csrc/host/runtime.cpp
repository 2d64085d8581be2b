// runtime.cpp -- device matrix, pool, transports, wait() and the blocking entry points, tile ops; the issue
// order of a factorization is in cholesky.cpp.
// See runtime.hpp for what each piece replaces in the reference.
#include "runtime.hpp"
#include "launch_args.hpp"
#include "tile_matrix.hpp"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <exception>
#include <thread>

namespace dlaf_mi355x {

void fatal(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vfprintf(stderr, fmt, ap);
  va_end(ap);
  std::fflush(stderr);
  std::terminate();  // same failure mode as DLAF_ASSERT (include/dlaf/common/assert.h:58-77)
}

static bool g_initialized = false;

void runtime_init() {
  if (g_initialized)
    return;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0)
    fatal("[dlaf_mi355x] no HIP device available: this library has no CPU fallback\n");
  // one process per GPU: honour LOCAL_RANK the way torch.distributed launchers export it
  int dev = 0;
  if (const char* lr = std::getenv("LOCAL_RANK"))
    dev = std::atoi(lr) % ndev;
  if (const char* d = std::getenv("DLAF_MI355X_DEVICE"))
    dev = std::atoi(d) % ndev;
  DLAF_HIP_CHECK(hipSetDevice(dev));
  device_kernels_init();
  g_initialized = true;
}

void runtime_finalize() {
  if (!g_initialized)
    return;
  (void) hipDeviceSynchronize();
  pool_release();
  g_initialized = false;
}

// =============================================================================== workspace pool
namespace {
struct Pool {
  std::mutex mu;
  std::map<void*, size_t> live;            // handed out: pointer -> capacity
  std::multimap<size_t, void*> idle;       // kept: capacity -> pointer
  size_t idle_bytes = 0;
};
Pool& pool() {
  static Pool p;
  return p;
}
constexpr size_t kPoolMinBytes = (size_t) 4 << 20;
size_t pool_cap_bytes() {
  static const size_t cap = [] {
    const char* e = std::getenv("DLAF_MI355X_POOL_GB");
    return (size_t) (e ? std::max(0.0, std::atof(e)) : 64.0) << 30;
  }();
  return cap;
}
}  // namespace

hipError_t pool_malloc(void** p, size_t bytes) {
  if (bytes < kPoolMinBytes || pool_cap_bytes() == 0)
    return hipMalloc(p, bytes);
  Pool& pl = pool();
  {
    std::lock_guard<std::mutex> lk(pl.mu);
    auto it = pl.idle.lower_bound(bytes);
    if (it != pl.idle.end() && it->first <= bytes + bytes / 4 + ((size_t) 64 << 20)) {
      *p = it->second;
      pl.live[*p] = it->first;
      pl.idle_bytes -= it->first;
      pl.idle.erase(it);
      return hipSuccess;
    }
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
    pl.live[*p] = bytes;
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
    auto it = pl.live.find(p);
    if (it != pl.live.end()) {
      cap = it->second;
      pl.live.erase(it);
    }
  }
  if (cap == 0)
    return hipFree(p);
  (void) hipDeviceSynchronize();  // (hipFree's implicit synchronisation: nothing enqueued may still use the block)
  std::vector<void*> drop;
  {
    std::lock_guard<std::mutex> lk(pl.mu);
    pl.idle.emplace(cap, p);
    pl.idle_bytes += cap;
    while (pl.idle_bytes > pool_cap_bytes() && !pl.idle.empty()) {
      auto big = std::prev(pl.idle.end());
      drop.push_back(big->second);
      pl.idle_bytes -= big->first;
      pl.idle.erase(big);
    }
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
    for (auto& kv : pl.idle)
      drop.push_back(kv.second);
    pl.idle.clear();
    pl.idle_bytes = 0;
  }
  for (void* q : drop)
    (void) hipFree(q);
}

size_t pool_idle_bytes() {
  Pool& pl = pool();
  std::lock_guard<std::mutex> lk(pl.mu);
  return pl.idle_bytes;
}

bool runtime_initialized() {
  return g_initialized;
}

// =============================================================================== host transport
namespace {
class HostTransport final : public Transport {
public:
  HostTransport(dlaf_host_bcast_fn b, dlaf_host_barrier_fn bar, void* user) : bcast_(b), barrier_(bar), user_(user) {}
  ~HostTransport() override {
    if (pinned_)
      (void) hipHostFree(pinned_);
  }
  bool device_side() const override { return false; }
  void bcast(CommAxis axis, int root, int my_index, const void* send, void* recv, size_t bytes,
             hipStream_t stream) override {
    if (bytes == 0)
      return;
    reserve(bytes);
    if (my_index == root)
      DLAF_HIP_CHECK(hipMemcpyAsync(pinned_, send, bytes, hipMemcpyDeviceToHost, stream));
    DLAF_HIP_CHECK(hipStreamSynchronize(stream));
    if (bcast_(user_, (int) axis, root, pinned_, bytes) != 0)
      fatal("[dlaf_mi355x] host broadcast callback failed\n");
    DLAF_HIP_CHECK(hipMemcpyAsync(recv, pinned_, bytes, hipMemcpyHostToDevice, stream));
    DLAF_HIP_CHECK(hipStreamSynchronize(stream));
  }
  void barrier(hipStream_t stream) override {
    DLAF_HIP_CHECK(hipStreamSynchronize(stream));
    if (barrier_ && barrier_(user_) != 0)
      fatal("[dlaf_mi355x] host barrier callback failed\n");
  }
  void allreduce_max(double* v, int n, int nprow, int npcol, int myrow, int mycol) override {
    // with only row/column broadcasts at hand: every member of my row broadcasts in turn, then every
    // member of my column
    std::vector<double> tmp((size_t) n);
    for (int pass = 0; pass < 2; ++pass) {
      const int members = pass == 0 ? npcol : nprow, me = pass == 0 ? mycol : myrow;
      std::vector<double> best(v, v + n);
      for (int root = 0; root < members; ++root) {
        if (me == root)
          std::copy(v, v + n, tmp.begin());
        if (bcast_(user_, pass, root, tmp.data(), sizeof(double) * (size_t) n) != 0)
          fatal("[dlaf_mi355x] host broadcast callback failed\n");
        for (int i = 0; i < n; ++i)
          best[(size_t) i] = std::max(best[(size_t) i], tmp[(size_t) i]);
      }
      std::copy(best.begin(), best.end(), v);
    }
  }

  void allreduce_sum(void* dev, size_t count, char type, char scope, hipStream_t stream) override {
    if (count == 0)
      return;
    const bool dbl = (type == 'd' || type == 'z');
    const size_t nreal = count * ((type == 'c' || type == 'z') ? 2 : 1);
    const size_t bytes = nreal * (dbl ? sizeof(double) : sizeof(float));
    reserve(2 * bytes);
    // (copies on the caller's stream + its synchronisation: the null stream the blocking hipMemcpy would use is not
    //  ordered with the non-blocking stream the consumers of `dev` run on)
    DLAF_HIP_CHECK(hipMemcpyAsync(pinned_, dev, bytes, hipMemcpyDeviceToHost, stream));
    DLAF_HIP_CHECK(hipStreamSynchronize(stream));
    char* mine = static_cast<char*>(pinned_);
    char* tmp = mine + bytes;
    std::vector<char> acc(bytes);
    for (int pass = 0; pass < 2; ++pass) {
      // pass 0: along my process row (axis Row), pass 1: along my process column
      if ((pass == 0 && scope == 'C') || (pass == 1 && scope == 'R'))
        continue;
      const int members = pass == 0 ? npcol : nprow, me = pass == 0 ? mycol : myrow;
      if (members <= 1)
        continue;
      for (int root = 0; root < members; ++root) {
        if (me == root)
          std::memcpy(tmp, mine, bytes);
        if (bcast_(user_, pass, root, tmp, bytes) != 0)
          fatal("[dlaf_mi355x] host broadcast callback failed\n");
        if (root == 0)
          std::memcpy(acc.data(), tmp, bytes);
        else if (dbl) {
          double* a = reinterpret_cast<double*>(acc.data());
          const double* t = reinterpret_cast<const double*>(tmp);
          for (size_t i = 0; i < nreal; ++i)
            a[i] += t[i];
        }
        else {
          float* a = reinterpret_cast<float*>(acc.data());
          const float* t = reinterpret_cast<const float*>(tmp);
          for (size_t i = 0; i < nreal; ++i)
            a[i] += t[i];
        }
      }
      std::memcpy(mine, acc.data(), bytes);
    }
    DLAF_HIP_CHECK(hipMemcpyAsync(dev, mine, bytes, hipMemcpyHostToDevice, stream));
    DLAF_HIP_CHECK(hipStreamSynchronize(stream));
  }

private:
  void reserve(size_t bytes) {
    if (bytes <= cap_)
      return;
    if (pinned_)
      DLAF_HIP_CHECK(hipHostFree(pinned_));
    DLAF_HIP_CHECK(hipHostMalloc(&pinned_, bytes, hipHostMallocDefault));
    cap_ = bytes;
  }
  dlaf_host_bcast_fn bcast_;
  dlaf_host_barrier_fn barrier_;
  void* user_;
  void* pinned_ = nullptr;
  size_t cap_ = 0;
};
}  // namespace

std::unique_ptr<Transport> make_host_transport(dlaf_host_bcast_fn b, dlaf_host_barrier_fn bar, void* user) {
  return std::unique_ptr<Transport>(new HostTransport(b, bar, user));
}

// =============================================================================== recording wrapper
namespace {
class RecordingTransport final : public Transport {
public:
  RecordingTransport(std::unique_ptr<Transport> inner, Grid* g) : inner_(std::move(inner)), g_(g) {}
  bool device_side() const override { return inner_->device_side(); }
  void bcast(CommAxis axis, int root, int my_index, const void* send, void* recv, size_t bytes,
             hipStream_t stream) override {
    if (bytes != 0 && g_->comm_log_on)
      g_->comm_log.push_back({(long) axis, (long) root, (long) bytes, (long) depth_});
    inner_->bcast(axis, root, my_index, send, recv, bytes, stream);
  }
  void group_begin() override {
    ++depth_;
    inner_->group_begin();
  }
  void group_end() override {
    --depth_;
    inner_->group_end();
  }
  void barrier(hipStream_t stream) override {
    if (g_->comm_log_on)
      g_->comm_log.push_back({3, 0, 0, 0});
    inner_->barrier(stream);
  }
  void allreduce_max(double* v, int n, int nprow, int npcol, int myrow, int mycol) override {
    if (g_->comm_log_on)
      g_->comm_log.push_back({4, 0, (long) (n * sizeof(double)), 0});
    inner_->allreduce_max(v, n, nprow, npcol, myrow, mycol);
  }
  void allreduce_sum(void* dev, size_t count, char type, char scope, hipStream_t stream) override {
    if (g_->comm_log_on)
      g_->comm_log.push_back({4, (long) scope, (long) count, 0});
    inner_->nprow = nprow;
    inner_->npcol = npcol;
    inner_->myrow = myrow;
    inner_->mycol = mycol;
    inner_->allreduce_sum(dev, count, type, scope, stream);
  }
  void mark(long step) override {
    if (g_->comm_log_on)
      g_->comm_log.push_back({2, step, 0, 0});
  }
  bool is_recorder() const { return true; }

private:
  std::unique_ptr<Transport> inner_;
  Grid* g_;
  int depth_ = 0;
};
}  // namespace

// the transport of a grid that came with host callbacks: host-staged (default) or, DLAF_MI355X_TRANSPORT=peer, the
// host-driven peer-copy transport whose control messages travel over the same callbacks (transport_peer.cpp)
std::unique_ptr<Transport> make_callback_transport(dlaf_host_bcast_fn b, dlaf_host_barrier_fn bar, void* user) {
  const char* e = std::getenv("DLAF_MI355X_TRANSPORT");
  if (e && std::strcmp(e, "peer") == 0)
    return make_peer_transport(b, bar, user);
  return make_host_transport(b, bar, user);
}

Transport* grid_transport(Grid& g) {
  if (g.nranks > 1 && !g.transport && g.host_bcast)
    g.transport = make_callback_transport(g.host_bcast, g.host_barrier, g.host_user);
  if (g.transport && g.comm_log_on && dynamic_cast<RecordingTransport*>(g.transport.get()) == nullptr)
    g.transport = std::unique_ptr<Transport>(new RecordingTransport(std::move(g.transport), &g));
  if (g.transport) {
    g.transport->nprow = g.nprow;
    g.transport->npcol = g.npcol;
    g.transport->myrow = g.myrow;
    g.transport->mycol = g.mycol;
  }
  return g.transport.get();
}

int agree_on_info(Grid& g, int info) {
  if (g.nranks > 1 && g.transport) {
    // v[0] carries the LAPACK index (MAX of 2^31 - info = MIN of info), v[1] the scheduling failure
    constexpr double kTop = 2147483648.0;
    double v[2] = {info > 0 ? kTop - (double) info : 0.0, info == kInfoSchedulingFailure ? 1.0 : 0.0};
    g.transport->allreduce_max(v, 2, g.nprow, g.npcol, g.myrow, g.mycol);
    info = v[1] > 0 ? kInfoSchedulingFailure : (v[0] > 0 ? (int) (kTop - v[0]) : 0);
  }
  return info;
}

// =============================================================================== DeviceMatrix
static std::vector<hipEvent_t> make_events(size_t n) {
  std::vector<hipEvent_t> v(n);
  for (auto& e : v)
    DLAF_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  return v;
}

template <class T>
void DeviceMatrix<T>::create(Grid* g, char uplo_, long n_, int nb_, int isrc, int jsrc) {
  runtime_init();
  type = TypeInfo<T>::tag;
  grid = g;
  (void) grid_transport(*g);
  uplo = (uplo_ == 'U' || uplo_ == 'u') ? 'U' : 'L';
  transposed = (uplo == 'U');
  n = n_;
  nb = nb_;
  Axis srow{n, nb, g->nprow, g->myrow, isrc};
  Axis scol{n, nb, g->npcol, g->mycol, jsrc};
  rows = transposed ? scol : srow;
  cols = transposed ? srow : scol;
  nt = rows.nt();
  ltr = rows.local_tiles();
  ltc = cols.local_tiles();
  tile_elems = (size_t) nb * nb;

  tiles = dev_alloc<T>((size_t) ltr * ltc * tile_elems);
  winv = dev_alloc<T>(2 * winv_elems());  // alternating by step parity
  const bool dist = g->nranks > 1;
  if (dist) {
    diag_ws = dev_alloc<T>(2 * (tile_elems + winv_elems()));  // alternating by step parity
    for (int b = 0; b < 2; ++b) {
      panel[b] = dev_alloc<T>((size_t) ltr * tile_elems);
      // grouped by root process row: up to rows.P classes of ceil(ltc / classes) tiles each
      panelT[b] = dev_alloc<T>((size_t) (ltc + rows.P) * tile_elems);
    }
  }
  {
    hipDeviceProp_t prop;
    int dev = 0;
    DLAF_HIP_CHECK(hipGetDevice(&dev));
    DLAF_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
    bulk_slots = (long) prop.multiProcessorCount * update_blocks_per_cu<T>();
  }
  DLAF_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&info), sizeof(int)));
  // NOT hipMemset: that call returns before its fill has run, on the null stream, which the streams below do not
  // synchronise with -- the fill could land after the first diagonal tile's POTRF had flagged its pivot, and the
  // factorization of a matrix that is not positive definite came back with info 0 (README, round 4).
  DLAF_HIP_CHECK(zero_device_now(info, sizeof(int)));
  // Flags and counters of the launches that need them: a slice of 16 words (8 dequeue heads + 8 pacing counters)
  // per persistent update launch, then a slice per diagonal tile for the cooperative POTRF.  The whole buffer is
  // zeroed ONCE per factorization and every launch gets a slice of its own: no fill kernel in front of every
  // bulk launch and every tile POTRF.  (Measured A/B on one box, N = 32768 nb = 512: 59.43 against 59.40 TFlop/s --
  // the fill kernels were not on the critical path; kept because it removes ~110 launches per factorization.)
  {
    const size_t nt_ = (size_t) std::max<long>(1, (n + nb - 1) / nb);
    coop_sync_update_slices = 6 * nt_ + 8;
    coop_sync_potrf_words = potrf_coop_sync_words(nb);
    coop_sync_words = 16 * coop_sync_update_slices + coop_sync_potrf_words * nt_;
  }
  DLAF_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&coop_sync), sizeof(unsigned) * coop_sync_words));
  DLAF_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&info_host), sizeof(int), hipHostMallocDefault));
  *info_host = 0;

  // POTRF / TRSM / lookahead column on a high-priority stream, the bulk of the trailing update on a
  // normal one (the reference's priority rule, cholesky/impl.h:172-173, src/init.cpp:70-83)
  int lo = 0, hi = 0;
  DLAF_HIP_CHECK(hipDeviceGetStreamPriorityRange(&lo, &hi));
  DLAF_HIP_CHECK(hipStreamCreateWithPriority(&s_high, hipStreamNonBlocking, hi));
  // Tuning knobs (tune.h analogue): DLAF_MI355X_SERIAL=1 issues everything on one stream (no
  // lookahead); DLAF_MI355X_RESERVED_CUS=R keeps R compute units out of the bulk-update stream so
  // the critical-path kernels (POTRF chain, panel TRSM) never queue behind long update workgroups.
  const char* serial = std::getenv("DLAF_MI355X_SERIAL");
  const char* rcu = std::getenv("DLAF_MI355X_RESERVED_CUS");
  const int reserved = rcu ? std::atoi(rcu) : 0;  // CU-masked streams measured slower on MI355X
  if (serial && std::atoi(serial) != 0) {
    s_low = s_high;
  }
  else if (reserved > 0) {
    hipDeviceProp_t prop;
    int dev = 0;
    DLAF_HIP_CHECK(hipGetDevice(&dev));
    DLAF_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
    const int ncu = prop.multiProcessorCount;
    std::vector<uint32_t> mask((size_t) (ncu + 31) / 32, 0u);
    for (int cu = reserved; cu < ncu; ++cu)
      mask[(size_t) cu / 32] |= 1u << (cu % 32);
    DLAF_HIP_CHECK(hipExtStreamCreateWithCUMask(&s_low, (uint32_t) mask.size(), mask.data()));
  }
  else {
    DLAF_HIP_CHECK(hipStreamCreateWithPriority(&s_low, hipStreamNonBlocking, lo));
  }
  DLAF_HIP_CHECK(hipStreamCreateWithPriority(&s_comm, hipStreamNonBlocking, hi));
  const size_t ne = (size_t) (nt > 0 ? nt : 1);
  ev_panel = make_events(ne);
  ev_done = make_events(1);
  ev_high = make_events(ne);
  ev_diag = make_events(ne);
  ev_bcast = make_events(ne);
  ev_head = make_events(ne);
  ev_headb = make_events(ne);
  ev_start = make_events(2);
}

template <class T>
void DeviceMatrix<T>::destroy() {
  if (!tiles)
    return;
  (void) hipDeviceSynchronize();
  for (auto* v : {&ev_panel, &ev_done, &ev_high, &ev_diag, &ev_bcast, &ev_start, &ev_head, &ev_headb}) {
    for (auto e : *v)
      (void) hipEventDestroy(e);
    v->clear();
  }
  for (auto& ps : prof) {
    for (auto e : ps.start)
      (void) hipEventDestroy(e);
    for (auto e : ps.stop)
      (void) hipEventDestroy(e);
    ps.start.clear();
    ps.stop.clear();
  }
  if (s_low != s_high)
    (void) hipStreamDestroy(s_low);
  (void) hipStreamDestroy(s_high);
  (void) hipStreamDestroy(s_comm);
  (void) hipFree(tiles);
  (void) hipFree(winv);
  if (diag_ws)
    (void) hipFree(diag_ws);
  for (int b = 0; b < 2; ++b) {
    if (panel[b])
      (void) hipFree(panel[b]);
    if (panelT[b])
      (void) hipFree(panelT[b]);
  }
  if (staging)
    (void) hipFree(staging);
  (void) hipFree(info);
  (void) hipFree(coop_sync);
  (void) hipHostFree(info_host);
  tiles = nullptr;
}

template <class T>
static LayoutArgs<T> layout_args(const DeviceMatrix<T>& m, T* cm, long ld_cm) {
  LayoutArgs<T> a;
  a.tiles = m.tiles;
  a.cm = cm;
  a.ld_cm = ld_cm;
  a.ltr = (int) m.ltr;
  a.ltc = (int) m.ltc;
  a.nb = m.nb;
  a.rows = m.rows.local_size();
  a.cols = m.cols.local_size();
  a.pr = m.rows.P;
  a.ri = m.rows.shift();
  a.pc = m.cols.P;
  a.ci = m.cols.shift();
  a.transpose = m.transposed ? 1 : 0;
  return a;
}

// Source (caller-side) local extents: rows/cols of the UNtransposed distribution.
template <class T>
static void source_extents(const DeviceMatrix<T>& m, long& srows, long& scols) {
  srows = m.transposed ? m.cols.local_size() : m.rows.local_size();
  scols = m.transposed ? m.rows.local_size() : m.cols.local_size();
}

template <class T>
static void ensure_staging(DeviceMatrix<T>& m, size_t elems) {
  if (m.staging && m.staging_elems >= elems)
    return;
  if (m.staging)
    DLAF_HIP_CHECK(hipFree(m.staging));
  m.staging = dev_alloc<T>(elems);
  m.staging_elems = elems;
}

// The uplo triangle of the caller's local array as one rectangle per local tile column of the SOURCE:
// f(row0, nrows, col0, ncols) in source element coordinates; diag(row0, col0, rows, cols) for every local
// diagonal tile (whose other half lies inside a rectangle but is not part of the triangle).
template <class T, class F, class D>
static void for_each_triangle_block(const DeviceMatrix<T>& m, F&& f, D&& diag) {
  long srows, scols;
  source_extents(m, srows, scols);
  // source axes: rows of the source are the view's rows (uplo L) or the view's columns (uplo U)
  const Axis& srow_ax = m.transposed ? m.cols : m.rows;
  const Axis& scol_ax = m.transposed ? m.rows : m.cols;
  const long nlc = scol_ax.local_tiles();
  for (long jl = 0; jl < nlc; ++jl) {
    const long gj = scol_ax.global_of(jl);
    const long col0 = jl * m.nb, ncols = std::min<long>(m.nb, scols - col0);
    long row0, row1;
    if (!m.transposed) {  // lower: source tile rows with global index >= gj
      row0 = std::min(srow_ax.next_local(gj) * m.nb, srows);
      row1 = srows;
    }
    else {  // upper: source tile rows with global index <= gj
      row0 = 0;
      row1 = std::min(srow_ax.next_local(gj + 1) * m.nb, srows);
    }
    if (ncols > 0 && row1 > row0)
      f(row0, row1 - row0, col0, ncols);
    if (srow_ax.mine(gj)) {
      const long r0 = srow_ax.local_of(gj) * m.nb;
      diag(r0, col0, std::min<long>(m.nb, srows - r0), ncols);
    }
  }
}

template <class T>
void DeviceMatrix<T>::upload(const T* host, long ld) {
  long srows, scols;
  source_extents(*this, srows, scols);
  if (srows == 0 || scols == 0)
    return;
  const long lds = srows;
  ensure_staging(*this, (size_t) lds * scols);
  // only the uplo triangle crosses PCIe (the relayout never reads the other one); the copies, the relayout and the
  // closing synchronisation share one stream, so the caller's array is free to go when this returns
  for_each_triangle_block(
      *this,
      [&](long r0, long nr, long c0, long nc) {
        DLAF_HIP_CHECK(hipMemcpy2DAsync(staging + r0 + c0 * lds, (size_t) lds * sizeof(T), host + r0 + c0 * ld,
                                        (size_t) ld * sizeof(T), (size_t) nr * sizeof(T), (size_t) nc,
                                        hipMemcpyHostToDevice, s_high));
      },
      [](long, long, long, long) {});
  launch_to_tiles(layout_args(*this, staging, lds), s_high);
  DLAF_HIP_CHECK(hipStreamSynchronize(s_high));
}

template <class T>
void DeviceMatrix<T>::download(T* host, long ld, bool staging_is_current) {
  long srows, scols;
  source_extents(*this, srows, scols);
  if (srows == 0 || scols == 0)
    return;
  const long lds = srows;
  ensure_staging(*this, (size_t) lds * scols);
  // The other half of the diagonal tiles travels back inside the rectangles and must come back unchanged:
  // it is already in the staging copy when that was filled from this very array and no caller code ran in
  // between (the blocking host entry points say so), otherwise the diagonal tiles are staged first.
  if (!staging_is_current) {
    for_each_triangle_block(
        *this, [](long, long, long, long) {},
        [&](long r0, long c0, long nr, long nc) {
          if (nr > 0 && nc > 0)
            DLAF_HIP_CHECK(hipMemcpy2DAsync(staging + r0 + c0 * lds, (size_t) lds * sizeof(T), host + r0 + c0 * ld,
                                            (size_t) ld * sizeof(T), (size_t) nr * sizeof(T), (size_t) nc,
                                            hipMemcpyHostToDevice, s_high));
        });
  }
  launch_from_tiles(layout_args(*this, staging, lds), s_high);
  for_each_triangle_block(
      *this,
      [&](long r0, long nr, long c0, long nc) {
        DLAF_HIP_CHECK(hipMemcpy2DAsync(host + r0 + c0 * ld, (size_t) ld * sizeof(T), staging + r0 + c0 * lds,
                                        (size_t) lds * sizeof(T), (size_t) nr * sizeof(T), (size_t) nc,
                                        hipMemcpyDeviceToHost, s_high));
      },
      [](long, long, long, long) {});
  DLAF_HIP_CHECK(hipStreamSynchronize(s_high));
}

template <class T>
void DeviceMatrix<T>::copy_from(const DeviceMatrix<T>& o) {
  if (o.n != n || o.nb != nb || o.ltr != ltr || o.ltc != ltc || o.transposed != transposed)
    fatal("[dlaf_mi355x] copy_from: matrices differ in shape or distribution\n");
  DLAF_HIP_CHECK(hipMemcpyAsync(tiles, o.tiles, (size_t) ltr * ltc * tile_elems * sizeof(T),
                                hipMemcpyDeviceToDevice, s_high));
  DLAF_HIP_CHECK(hipStreamSynchronize(s_high));
}

template <class T>
void DeviceMatrix<T>::prof_begin(int kind, hipStream_t s) {
  if (!profiling)
    return;
  ProfSlot& p = prof[kind];
  if (p.used == p.start.size()) {
    hipEvent_t a, b;
    DLAF_HIP_CHECK(hipEventCreate(&a));
    DLAF_HIP_CHECK(hipEventCreate(&b));
    p.start.push_back(a);
    p.stop.push_back(b);
  }
  DLAF_HIP_CHECK(hipEventRecord(p.start[p.used], s));
}

template <class T>
void DeviceMatrix<T>::prof_end(int kind, hipStream_t s, double flops, double bytes) {
  if (!profiling)
    return;
  ProfSlot& p = prof[kind];
  DLAF_HIP_CHECK(hipEventRecord(p.stop[p.used], s));
  ++p.used;
  p.flops += flops;
  p.bytes += bytes;
}

// ------------------------------------------------------------------------------- grid self-test
int grid_selftest(Grid& g, size_t bytes) {
  runtime_init();
  Transport* tr = grid_transport(g);
  if (!tr)
    return 0;  // 1x1 grid without communicators
  const size_t words = std::max<size_t>(1, bytes / sizeof(unsigned));
  unsigned *src = nullptr, *dst = nullptr;
  DLAF_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&src), words * sizeof(unsigned)));
  DLAF_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&dst), 2 * words * sizeof(unsigned)));
  std::vector<unsigned> h(words), back(2 * words);
  hipStream_t s = nullptr;
  DLAF_HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  int bad = 0;
  auto pattern = [&](int axis, int root, int fixed, int form, size_t i) {
    return (unsigned) (0x9E3779B1u * (unsigned) (i + 1)) ^ (unsigned) (axis << 28 | form << 24 | root << 12 | fixed);
  };
  for (int axis = 0; axis < 2; ++axis) {
    const CommAxis ax = axis == 0 ? CommAxis::Row : CommAxis::Col;
    const int members = axis == 0 ? g.npcol : g.nprow;
    const int me = axis == 0 ? g.mycol : g.myrow;
    const int fixed = axis == 0 ? g.myrow : g.mycol;
    for (int root = 0; root < members; ++root) {
      // form 0: in place;  form 1: out of place;  form 2: two grouped out-of-place broadcasts
      for (int form = 0; form < 3; ++form) {
        for (size_t i = 0; i < words; ++i)
          h[i] = (me == root) ? pattern(axis, root, fixed, form, i) : 0xDEADBEEFu;
        DLAF_HIP_CHECK(hipMemcpyAsync(src, h.data(), words * sizeof(unsigned), hipMemcpyHostToDevice, s));
        DLAF_HIP_CHECK(hipMemsetAsync(dst, 0, 2 * words * sizeof(unsigned), s));
        const void* send = (me == root) ? src : nullptr;
        if (form == 0)
          tr->bcast(ax, root, me, src, src, words * sizeof(unsigned), s);
        else if (form == 1)
          tr->bcast(ax, root, me, send, dst, words * sizeof(unsigned), s);
        else {
          tr->group_begin();
          tr->bcast(ax, root, me, send, dst, words * sizeof(unsigned), s);
          tr->bcast(ax, root, me, send, dst + words, words * sizeof(unsigned), s);
          tr->group_end();
        }
        DLAF_HIP_CHECK(hipMemcpyAsync(back.data(), form == 0 ? src : dst, (form == 2 ? 2 : 1) * words * sizeof(unsigned),
                                      hipMemcpyDeviceToHost, s));
        DLAF_HIP_CHECK(hipStreamSynchronize(s));
        for (size_t i = 0; i < (form == 2 ? 2 : 1) * words; ++i)
          if (back[i] != pattern(axis, root, fixed, form, i % words)) {
            ++bad;
            break;
          }
      }
    }
  }
  tr->barrier(s);
  double v[2] = {(double) (g.myrow * g.npcol + g.mycol), -(double) (g.myrow * g.npcol + g.mycol)};
  tr->allreduce_max(v, 2, g.nprow, g.npcol, g.myrow, g.mycol);
  if (v[0] != (double) (g.nprow * g.npcol - 1) || v[1] != 0.0)
    ++bad;
  DLAF_HIP_CHECK(hipStreamDestroy(s));
  (void) hipFree(src);
  (void) hipFree(dst);
  return bad;
}

// ------------------------------------------------------------------------------- residual checker
// max|A - L L^H| / max|A| as the reference's miniapp computes it (miniapp_cholesky.cpp:243-443:
// setUpperToZeroForDiagonalTiles, cholesky_diff with row/column broadcasts + reduce, max_norm), on the
// device: the same grouped update kernel subtracts L(:,k) L(:,k)^H column panel by column panel, the
// panels travel exactly like in the factorization, the norms are reduced over the grid with MAX.
template <class T>
void DeviceMatrix<T>::residual_of(DeviceMatrix<T>& L, double* max_diff, double* max_a) {
  if (L.n != n || L.nb != nb || L.ltr != ltr || L.ltc != ltc || L.transposed != transposed)
    fatal("[dlaf_mi355x] residual_of: matrices differ in shape or distribution\n");
  Transport* tr = grid_transport(*grid);
  const bool dist = grid->nranks > 1;
  const CommAxis ax_row = transposed ? CommAxis::Col : CommAxis::Row;
  const CommAxis ax_col = transposed ? CommAxis::Row : CommAxis::Col;
  const size_t tile_bytes = tile_elems * sizeof(T);
  hipStream_t s = s_low;
  double* dnorm = nullptr;
  DLAF_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&dnorm), 2 * sizeof(double)));
  DLAF_HIP_CHECK(hipMemsetAsync(info, 0, sizeof(int), s));
  launch_max_norm(tiles, (int) ltr, (int) ltc, nb, rows.local_size(), cols.local_size(), rows.P, rows.shift(), cols.P,
                  cols.shift(), dnorm + 1, s);
  launch_zero_upper_diag(L.tiles, (int) ltr, (int) ltc, nb, rows.P, rows.shift(), cols.P, cols.shift(), s);
  DLAF_HIP_CHECK(hipStreamSynchronize(s));
  for (long k = 0; k < nt; ++k) {
    const int kb = rows.tile_extent(k);
    const int own_c = cols.owner(k);
    const bool in_col = cols.rank == own_c;
    const long il_f = rows.next_local(k), jl_f = cols.next_local(k);
    const long klc = in_col ? cols.local_of(k) : -1;
    if (il_f >= ltr && !dist)
      continue;
    const T* a_base;
    const T* b_base;
    long b_ts = (long) tile_elems;
    if (cols.P > 1) {
      T* dst = in_col ? L.tile(il_f < ltr ? il_f : 0, klc) : panel[0];
      if (il_f < ltr)
        tr->bcast(ax_row, own_c, cols.rank, dst, dst, (size_t) (ltr - il_f) * tile_bytes, s);
      a_base = dst;
    }
    else {
      a_base = L.tile(il_f < ltr ? il_f : 0, klc);
    }
    int b_period = 1;
    long b_ts2 = 0;
    if (rows.P > 1) {
      bcast_transposed_panel(tr, ax_col, a_base, il_f, jl_f, panelT[0], s, b_period, b_ts2);
      b_base = panelT[0];
    }
    else {
      b_base = a_base + (cols.global_of(jl_f) - il_f) * (long) tile_elems;
      b_ts = (long) tile_elems * cols.P;
    }
    if (il_f >= ltr || jl_f >= ltc)
      continue;
    const long il0 = std::max(il_f, rows.next_local(cols.global_of(jl_f)));
    if (il0 >= ltr)
      continue;
    UpdateArgs<T> ua = update_args(*this, il0, ltr, jl_f, ltc, a_base + (size_t) (il0 - il_f) * tile_elems, b_base, b_ts,
                                   kb, info);
    ua.b_period = b_period;
    ua.b_ts2 = b_ts2;
    ua.b_jl0 = (int) jl_f;
    launch_update(ua, s, 3);
    if (dist)
      DLAF_HIP_CHECK(hipStreamSynchronize(s));  // the single panel workspace is reused by the next step
  }
  launch_max_norm(tiles, (int) ltr, (int) ltc, nb, rows.local_size(), cols.local_size(), rows.P, rows.shift(), cols.P,
                  cols.shift(), dnorm, s);
  DLAF_HIP_CHECK(hipStreamSynchronize(s));
  double h[2];
  DLAF_HIP_CHECK(hipMemcpy(h, dnorm, sizeof(h), hipMemcpyDeviceToHost));
  DLAF_HIP_CHECK(hipFree(dnorm));
  if (dist)
    tr->allreduce_max(h, 2, grid->nprow, grid->npcol, grid->myrow, grid->mycol);
  if (max_diff)
    *max_diff = h[0];
  if (max_a)
    *max_a = h[1];
}

template <class T>
int DeviceMatrix<T>::wait() {
  DLAF_HIP_CHECK(hipStreamSynchronize(s_comm));
  DLAF_HIP_CHECK(hipStreamSynchronize(s_low));
  DLAF_HIP_CHECK(hipStreamSynchronize(s_high));
  DLAF_HIP_CHECK(hipMemcpy(info_host, info, sizeof(int), hipMemcpyDeviceToHost));
  local_info = *info_host;
  // DLAF_MI355X_INFO_VERBOSE=1: this rank's own status word before the grid agrees on one (diagnosis of the
  // intermittent "owner did not report its negative pivot" failure of the six-rank test worker, README status)
  static const bool info_verbose = [] {
    const char* e = std::getenv("DLAF_MI355X_INFO_VERBOSE");
    return e && std::atoi(e) != 0;
  }();
  if (info_verbose)
    std::fprintf(stderr, "[dlaf_mi355x] rank (%d,%d) of %dx%d: local info %d (n %ld nb %d)\n", grid->myrow, grid->mycol,
                 grid->nprow, grid->npcol, *info_host, n, nb);
  // one value for the whole grid (ScaLAPACK's p?potrf contract; the reference aborts every rank,
  // src/cusolver/assert_info.cu:35-45)
  *info_host = agree_on_info(*grid, *info_host);
  if (*info_host == kInfoSchedulingFailure)
    fatal("[dlaf_mi355x] cooperative POTRF: a bounded inter-workgroup wait expired (workgroups not co-resident); "
          "the result is invalid. DLAF_MI355X_POTRF=chain selects the non-cooperative path.\n");
  for (auto& ps : prof) {
    ps.ms = 0;
    ps.launches = (long) ps.used;
    for (size_t i = 0; i < ps.used; ++i) {
      float ms = 0;
      DLAF_HIP_CHECK(hipEventElapsedTime(&ms, ps.start[i], ps.stop[i]));
      ps.ms += ms;
    }
  }
  return *info_host;
}

template <class T>
bool DeviceMatrix<T>::fetch_tile(long gi, long gj, T* host, long ld) {
  // view indices: the device holds the transposed view for uplo == 'U'
  const long vi = transposed ? gj : gi, vj = transposed ? gi : gj;
  if (vi < 0 || vj < 0 || vi >= nt || vj >= nt || !rows.mine(vi) || !cols.mine(vj))
    return false;
  const int r = rows.tile_extent(vi), c = cols.tile_extent(vj);
  const T* src = tile(rows.local_of(vi), cols.local_of(vj));
  DLAF_HIP_CHECK(hipStreamSynchronize(s_low));
  DLAF_HIP_CHECK(hipStreamSynchronize(s_high));
  if (!transposed) {
    DLAF_HIP_CHECK(hipMemcpy2D(host, (size_t) ld * sizeof(T), src, (size_t) nb * sizeof(T), (size_t) r * sizeof(T),
                               (size_t) c, hipMemcpyDeviceToHost));
  }
  else {
    T* tmp = dev_alloc<T>(tile_elems);
    launch_copy2d(tmp, (long) c, src, (long) nb, c, r, 1, 0, s_high);  // caller's tile is c x r
    DLAF_HIP_CHECK(hipStreamSynchronize(s_high));
    DLAF_HIP_CHECK(hipMemcpy2D(host, (size_t) ld * sizeof(T), tmp, (size_t) c * sizeof(T), (size_t) c * sizeof(T),
                               (size_t) r, hipMemcpyDeviceToHost));
    DLAF_HIP_CHECK(hipFree(tmp));
  }
  return true;
}

template <class T>
double DeviceMatrix<T>::trsm_profile(int reps, double* flops, double* bytes) {
  if (flops)
    *flops = 0;
  if (bytes)
    *bytes = 0;
  if (grid->nranks != 1 || nt < 2 || reps < 1)
    return 0.0;
  const long ntiles = ltr - 1;
  T* scratch = dev_alloc<T>((size_t) ntiles * tile_elems);
  T* w = dev_alloc<T>(winv_elems());
  hipStream_t s = s_low;
  DLAF_HIP_CHECK(hipMemsetAsync(info, 0, sizeof(int), s));
  launch_invert_diag_blocks(tile(0, 0), nb, nb, w, info, s, false, false);
  // the panel of step 0 (one process: local row il is global tile il), solved on the copy
  TrsmArgs<T> ta = panel_args<TrsmArgs<T>>(*this, 1, ltr, 0, tile(0, 0), nb);
  ta.b = scratch;
  ta.winv = w;
  ta.info = info;
  hipEvent_t e0, e1;
  DLAF_HIP_CHECK(hipEventCreate(&e0));
  DLAF_HIP_CHECK(hipEventCreate(&e1));
  float total = 0;
  for (int r = -1; r < reps; ++r) {  // r = -1: warm-up
    // a fresh copy of the solved panel each time (X L^-H applied again and again would shrink to nothing)
    DLAF_HIP_CHECK(hipMemcpyAsync(scratch, tile(1, 0), (size_t) ntiles * tile_elems * sizeof(T), hipMemcpyDeviceToDevice, s));
    DLAF_HIP_CHECK(hipEventRecord(e0, s));
    launch_trsm(ta, s);
    DLAF_HIP_CHECK(hipEventRecord(e1, s));
    DLAF_HIP_CHECK(hipStreamSynchronize(s));
    float ms = 0;
    DLAF_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    if (r >= 0)
      total += ms;
  }
  (void) hipEventDestroy(e0);
  (void) hipEventDestroy(e1);
  DLAF_HIP_CHECK(hipFree(scratch));
  DLAF_HIP_CHECK(hipFree(w));
  double fl = 0, by = 0;
  for (long il = 1; il < ltr; ++il) {
    const double mi = rows.tile_extent(rows.global_of(il));
    fl += (TypeInfo<T>::is_complex ? 4.0 : 1.0) * (double) nb * nb * mi;
    by += (0.5 * nb * nb + 2.0 * mi * nb) * sizeof(T);
  }
  if (flops)
    *flops = fl;
  if (bytes)
    *bytes = by;
  return (double) total / reps;
}

template <class T>
int DeviceMatrix<T>::factorize() {
  factorize_async();
  return wait();
}

// View tile column k (rows on/below the diagonal) as a rectangle of the caller's local array.
template <class T>
static bool view_column_rect(const DeviceMatrix<T>& m, long k, long& r0, long& nr, long& c0, long& nc) {
  if (!m.cols.mine(k))
    return false;
  long srows, scols;
  source_extents(m, srows, scols);
  const long jl = m.cols.local_of(k);
  const long first = m.rows.next_local(k) * m.nb;  // first view row (element) on/below the diagonal
  if (!m.transposed) {
    r0 = std::min(first, srows);
    nr = srows - r0;
    c0 = jl * m.nb;
    nc = std::min<long>(m.nb, scols - c0);
  }
  else {  // the view column is a row block of the source
    r0 = jl * m.nb;
    nr = std::min<long>(m.nb, srows - r0);
    c0 = std::min(first, scols);
    nc = scols - c0;
  }
  return nr > 0 && nc > 0;
}

template <class T>
int DeviceMatrix<T>::factorize_and_download(T* host, long ld) {
  long srows, scols;
  source_extents(*this, srows, scols);
  const char* off = std::getenv("DLAF_MI355X_OVERLAP_DOWNLOAD");
  if (srows == 0 || scols == 0 || nt < 3 || (off && std::atoi(off) == 0)) {
    const int r = factorize();
    if (r == 0)
      download(host, ld, true);
    return r;
  }
  const long lds = srows;
  int dev = 0;
  DLAF_HIP_CHECK(hipGetDevice(&dev));
  panels_issued.store(-1, std::memory_order_release);
  std::atomic<bool> stop{false};
  auto fetch_column = [&](long k, hipStream_t s) {
    long r0, nr, c0, nc;
    if (!view_column_rect(*this, k, r0, nr, c0, nc))
      return;
    LayoutArgs<T> la = layout_args(*this, staging, lds);
    la.jl_first = (int) cols.local_of(k);
    la.jl_count = 1;
    launch_from_tiles(la, s);
    DLAF_HIP_CHECK(hipMemcpy2DAsync(host + r0 + c0 * ld, (size_t) ld * sizeof(T), staging + r0 + c0 * lds,
                                    (size_t) lds * sizeof(T), (size_t) nr * sizeof(T), (size_t) nc,
                                    hipMemcpyDeviceToHost, s));
    DLAF_HIP_CHECK(hipStreamSynchronize(s));
  };
  // columns 0 .. nt-2 leave as soon as their panel is solved; the helper never touches a column whose event
  // has not been recorded yet (panels_issued), and the device flag stops it on a failed factorization
  std::thread helper([&] {
    DLAF_HIP_CHECK(hipSetDevice(dev));
    hipStream_t s_dl = nullptr;
    DLAF_HIP_CHECK(hipStreamCreateWithFlags(&s_dl, hipStreamNonBlocking));
    for (long k = 0; k + 1 < nt; ++k) {
      while (panels_issued.load(std::memory_order_acquire) < k && !stop.load(std::memory_order_acquire))
        std::this_thread::yield();
      if (panels_issued.load(std::memory_order_acquire) < k)
        break;
      DLAF_HIP_CHECK(hipStreamWaitEvent(s_dl, ev_panel[k], 0));
      fetch_column(k, s_dl);
    }
    DLAF_HIP_CHECK(hipStreamDestroy(s_dl));
  });
  factorize_async();
  const int r = wait();
  stop.store(true, std::memory_order_release);
  helper.join();
  if (r == 0)
    fetch_column(nt - 1, s_high);
  return r;
}

// =============================================================================== single-tile ops
namespace {
// host (rows x cols, ld) -> dense device buffer in "device orientation" (transposed when tr)
template <class T>
void to_device(T* dst, const T* host, int ld, int rows, int cols, bool tr, T* tmp, hipStream_t s) {
  if (rows == 0 || cols == 0)
    return;
  T* raw = tr ? tmp : dst;
  DLAF_HIP_CHECK(hipMemcpy2DAsync(raw, (size_t) rows * sizeof(T), host, (size_t) ld * sizeof(T),
                                  (size_t) rows * sizeof(T), (size_t) cols, hipMemcpyHostToDevice, s));
  if (tr)
    launch_copy2d(dst, (long) cols, raw, (long) rows, cols, rows, 1, 0, s);
}
}  // namespace

template <class T>
int tile_potrf(char uplo, int n, T* a, int lda) {
  runtime_init();
  if (n == 0)
    return 0;
  const bool tr = (uplo == 'U' || uplo == 'u');
  hipStream_t s = nullptr;
  DevBuf<T> da((size_t) n * n), tmp((size_t) n * n), w((size_t) ((n + kDiagBlock - 1) / kDiagBlock) * kDiagBlock * kDiagBlock);
  DevBuf<int> info(1);
  DevBuf<unsigned> sync(potrf_coop_sync_words(n));
  DLAF_HIP_CHECK(hipMemsetAsync(info.p, 0, sizeof(int), s));
  DLAF_HIP_CHECK(hipMemsetAsync(sync.p, 0, sizeof(unsigned) * potrf_coop_sync_words(n), s));
  // tmp keeps the caller's image (host orientation); da the device orientation
  DLAF_HIP_CHECK(hipMemcpy2DAsync(tmp.p, (size_t) n * sizeof(T), a, (size_t) lda * sizeof(T), (size_t) n * sizeof(T),
                                  (size_t) n, hipMemcpyHostToDevice, s));
  launch_copy2d(da.p, (long) n, tmp.p, (long) n, n, n, tr ? 1 : 0, 0, s);
  potrf_tile(da.p, n, n, w.p, info.p, 0, sync.p, s);
  launch_copy2d(tmp.p, (long) n, da.p, (long) n, n, n, tr ? 1 : 0, tr ? 2 : 1, s);
  DLAF_HIP_CHECK(hipMemcpy2DAsync(a, (size_t) lda * sizeof(T), tmp.p, (size_t) n * sizeof(T), (size_t) n * sizeof(T),
                                  (size_t) n, hipMemcpyDeviceToHost, s));
  int h = 0;
  DLAF_HIP_CHECK(hipMemcpyAsync(&h, info.p, sizeof(int), hipMemcpyDeviceToHost, s));
  DLAF_HIP_CHECK(hipStreamSynchronize(s));
  if (h == kInfoSchedulingFailure)
    fatal("[dlaf_mi355x] cooperative POTRF: a bounded inter-workgroup wait expired; the result is invalid\n");
  return h;
}

// uplo L: B(m x n) <- B A^-H, A n x n lower.   uplo U: B(m x n) <- A^-H B, A m x m upper.
// (the two variants the factorization issues: cholesky/impl.h:56-67 and :110-121)
template <class T>
void tile_trsm(char uplo, int m, int n, const T* a, int lda, T* b, int ldb) {
  runtime_init();
  if (m == 0 || n == 0)
    return;
  const bool tr = (uplo == 'U' || uplo == 'u');
  const int na = tr ? m : n;             // order of the triangular matrix
  const int br = tr ? n : m, bc = na;    // device-orientation extents of B
  hipStream_t s = nullptr;
  const size_t wel = (size_t) ((na + kDiagBlock - 1) / kDiagBlock) * kDiagBlock * kDiagBlock;
  DevBuf<T> da((size_t) na * na), tmpa((size_t) na * na), db((size_t) m * n), tmpb((size_t) m * n), w(wel);
  DevBuf<int> info(1);
  DLAF_HIP_CHECK(hipMemsetAsync(info.p, 0, sizeof(int), s));
  to_device(da.p, a, lda, na, na, tr, tmpa.p, s);
  to_device(db.p, b, ldb, m, n, tr, tmpb.p, s);
  // inverted diagonal blocks of the (already triangular) factor: invert-only mode of the diag kernel
  for (int j0 = 0; j0 < na; j0 += kDiagBlock) {
    const int jb = std::min(kDiagBlock, na - j0);
    launch_potrf_diag(da.p + j0 + (size_t) j0 * na, na, jb, w.p + (size_t) (j0 / kDiagBlock) * kDiagBlock * kDiagBlock,
                      info.p, 0, s, false);
  }
  TrsmArgs<T> ta;
  ta.b = db.p;
  ta.b_ts = 0;
  ta.ldb = br;
  ta.il0 = 0;
  ta.il1 = 1;
  ta.pr = 1;
  ta.ri = 0;
  ta.nb = br;
  ta.nt = 1;
  ta.last_rows = br;
  ta.l = da.p;
  ta.ldl = na;
  ta.winv = w.p;
  ta.n = bc;
  ta.info = info.p;
  launch_trsm(ta, s);
  T* out = tr ? tmpb.p : db.p;
  if (tr)
    launch_copy2d(tmpb.p, (long) m, db.p, (long) br, m, n, 1, 0, s);
  DLAF_HIP_CHECK(hipMemcpy2DAsync(b, (size_t) ldb * sizeof(T), out, (size_t) m * sizeof(T), (size_t) m * sizeof(T),
                                  (size_t) n, hipMemcpyDeviceToHost, s));
  DLAF_HIP_CHECK(hipStreamSynchronize(s));
}

// uplo L: lower(C) -= A A^H, A n x k.   uplo U: upper(C) -= A^H A, A k x n.   (impl.h:70-80, :124-134)
template <class T>
void tile_herk(char uplo, int n, int k, const T* a, int lda, T* c, int ldc) {
  runtime_init();
  if (n == 0)
    return;
  const bool tr = (uplo == 'U' || uplo == 'u');
  hipStream_t s = nullptr;
  const int ar = tr ? k : n, ac = tr ? n : k;  // host extents of A
  DevBuf<T> da((size_t) n * std::max(k, 1)), tmpa((size_t) n * std::max(k, 1)), dc((size_t) n * n), tmpc((size_t) n * n);
  DevBuf<int> info(1);
  DLAF_HIP_CHECK(hipMemsetAsync(info.p, 0, sizeof(int), s));
  to_device(da.p, a, lda, ar, ac, tr, tmpa.p, s);
  DLAF_HIP_CHECK(hipMemcpy2DAsync(tmpc.p, (size_t) n * sizeof(T), c, (size_t) ldc * sizeof(T), (size_t) n * sizeof(T),
                                  (size_t) n, hipMemcpyHostToDevice, s));
  launch_copy2d(dc.p, (long) n, tmpc.p, (long) n, n, n, tr ? 1 : 0, 0, s);
  UpdateArgs<T> ua;
  ua.c = dc.p;
  ua.c_tsr = ua.c_tsc = 0;
  ua.ldc = n;
  ua.a = da.p;
  ua.a_ts = 0;
  ua.lda = n;
  ua.b = da.p;
  ua.b_ts = 0;
  ua.ldb = n;
  ua.il0 = ua.jl0 = 0;
  ua.il1 = ua.jl1 = 1;
  ua.nb = n;
  ua.K = k;
  ua.pr = ua.pc = 1;
  ua.ri = ua.ci = 0;
  ua.nt = 1;
  ua.last_rows = n;
  ua.info = info.p;
  launch_update(ua, s, 2);
  launch_copy2d(tmpc.p, (long) n, dc.p, (long) n, n, n, tr ? 1 : 0, tr ? 2 : 1, s);
  DLAF_HIP_CHECK(hipMemcpy2DAsync(c, (size_t) ldc * sizeof(T), tmpc.p, (size_t) n * sizeof(T), (size_t) n * sizeof(T),
                                  (size_t) n, hipMemcpyDeviceToHost, s));
  DLAF_HIP_CHECK(hipStreamSynchronize(s));
}

// uplo L: C(m x n) -= A B^H, A m x k, B n x k.   uplo U: C -= A^H B, A k x m, B k x n.
// (impl.h:83-94, :137-147)
template <class T>
void tile_gemm(char uplo, int m, int n, int k, const T* a, int lda, const T* b, int ldb, T* c, int ldc) {
  runtime_init();
  if (m == 0 || n == 0)
    return;
  const bool tr = (uplo == 'U' || uplo == 'u');
  hipStream_t s = nullptr;
  // device orientation: C' = C (L) or C^T (U), extents cm x cn; row operand A' (cm x k), column
  // operand B' (cn x k).  For U:  C^T -= B^T conj(A) = B' A'^H with B' = B^T as ROW operand.
  const int cm = tr ? n : m, cn = tr ? m : n;
  const int kk = std::max(k, 1);
  // the update kernel works on square tiles: pad the single tile to sq x sq with zero rows
  const int sq = std::max(cm, cn);
  DevBuf<T> dA((size_t) cm * kk), dB((size_t) cn * kk), tmp((size_t) std::max(m, n) * kk), tmpc((size_t) m * n);
  DevBuf<T> pA((size_t) sq * kk), pB((size_t) sq * kk), pC((size_t) sq * sq);
  DevBuf<int> info(1);
  DLAF_HIP_CHECK(hipMemsetAsync(info.p, 0, sizeof(int), s));
  DLAF_HIP_CHECK(hipMemsetAsync(pA.p, 0, (size_t) sq * kk * sizeof(T), s));
  DLAF_HIP_CHECK(hipMemsetAsync(pB.p, 0, (size_t) sq * kk * sizeof(T), s));
  DLAF_HIP_CHECK(hipMemsetAsync(pC.p, 0, (size_t) sq * sq * sizeof(T), s));
  if (k > 0) {
    if (!tr) {
      to_device(dA.p, a, lda, m, k, false, tmp.p, s);
      to_device(dB.p, b, ldb, n, k, false, tmp.p, s);
    }
    else {
      to_device(dA.p, b, ldb, k, n, true, tmp.p, s);
      DLAF_HIP_CHECK(hipStreamSynchronize(s));  // tmp is reused
      to_device(dB.p, a, lda, k, m, true, tmp.p, s);
    }
    launch_copy2d(pA.p, (long) sq, dA.p, (long) cm, cm, k, 0, 0, s);
    launch_copy2d(pB.p, (long) sq, dB.p, (long) cn, cn, k, 0, 0, s);
  }
  DLAF_HIP_CHECK(hipMemcpy2DAsync(tmpc.p, (size_t) m * sizeof(T), c, (size_t) ldc * sizeof(T), (size_t) m * sizeof(T),
                                  (size_t) n, hipMemcpyHostToDevice, s));
  launch_copy2d(pC.p, (long) sq, tmpc.p, (long) m, cm, cn, tr ? 1 : 0, 0, s);
  // a tile strictly below the diagonal (global index (1,0) of a 3 x 3 tile grid): plain gemm
  UpdateArgs<T> ua;
  ua.c = pC.p;
  ua.c_tsr = ua.c_tsc = 0;
  ua.ldc = sq;
  ua.a = pA.p;
  ua.a_ts = 0;
  ua.lda = sq;
  ua.b = pB.p;
  ua.b_ts = 0;
  ua.ldb = sq;
  ua.il0 = 1;
  ua.il1 = 2;
  ua.jl0 = 0;
  ua.jl1 = 1;
  ua.nb = sq;
  ua.K = k;
  ua.pr = ua.pc = 1;
  ua.ri = ua.ci = 0;
  ua.nt = 3;
  ua.last_rows = sq;
  ua.info = info.p;
  // c_tsr = 0: tile row index does not move the base
  launch_update(ua, s, 2);
  launch_copy2d(tmpc.p, (long) m, pC.p, (long) sq, m, n, tr ? 1 : 0, 0, s);
  DLAF_HIP_CHECK(hipMemcpy2DAsync(c, (size_t) ldc * sizeof(T), tmpc.p, (size_t) m * sizeof(T), (size_t) m * sizeof(T),
                                  (size_t) n, hipMemcpyDeviceToHost, s));
  DLAF_HIP_CHECK(hipStreamSynchronize(s));
}

#define INST(T)                                                                                     \
  template struct DeviceMatrix<T>;                                                                  \
  template int tile_potrf<T>(char, int, T*, int);                                                   \
  template void tile_trsm<T>(char, int, int, const T*, int, T*, int);                               \
  template void tile_herk<T>(char, int, int, const T*, int, T*, int);                               \
  template void tile_gemm<T>(char, int, int, int, const T*, int, const T*, int, T*, int);
INST(float)
INST(double)
INST(cfloat)
INST(cdouble)
#undef INST

}  // namespace dlaf_mi355x
