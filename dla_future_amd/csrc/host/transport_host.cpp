// transport_host.cpp -- the transport over host callbacks (device -> pinned host -> callback -> device), the recording
// wrapper of the communication log, and the grid's own functions: grid_transport, agree_on_info, grid_selftest.
// See transport.hpp for what each piece replaces in the reference.
#include "transport.hpp"
#include "runtime.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace dlaf_mi355x {

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

Transport* checked_transport(Grid& g) {
  runtime_init();
  Transport* tr = grid_transport(g);
  if (g.nranks > 1 && !tr)
    fatal("[dlaf_mi355x] grid with %d ranks has no transport\n", g.nranks);
  return tr;
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

}  // namespace dlaf_mi355x
