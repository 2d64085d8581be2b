// c_api.cpp -- the extern "C" surface, part 1 of 3 (c_api_internal.hpp has the map): the grid registry, and the
// reference's dlaf_c entry points for the Cholesky path (include/dlaf_c/{init,grid,utils}.h,
// include/dlaf_c/factorization/cholesky.h; implemented upstream in src/c_api/{init,grid,utils}.cpp and
// src/c_api/factorization/cholesky.{h,cpp}) with the grid entries of include/dlaf_mi355x/dlaf_mi355x.h.
// (the core never sees <mpi.h>: the MPI-typed prototypes of dlaf_c/grid.h stay out of this translation unit, which
// defines forwarders with a pointer-sized first parameter under the same names)
#define DLAF_MI355X_NO_MPI 1
#include <dlfcn.h>

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <unordered_map>

#include <dlaf_c/factorization/cholesky.h>
#include <dlaf_c/grid.h>
#include <dlaf_c/init.h>
#include <dlaf_mi355x/dlaf_mi355x.h>

#include "c_api_internal.hpp"
#include "device_matrix.hpp"
#include "eigensolver.hpp"
#include "pool.hpp"
#include "tile_matrix.hpp"

using namespace dlaf_mi355x;

namespace {
// grid registry: contexts count down from INT_MAX (reference: src/c_api/grid.cpp:26-31)
std::unordered_map<int, std::unique_ptr<Grid>> g_grids;

// A context is never handed out twice while its grid is alive: the reference numbers them
// INT_MAX - size() (grid.cpp:31) and relies on try_emplace never replacing a live entry; here the
// search simply continues downwards past contexts that are still registered (create A, create B,
// free A, create C must not give C the context of B).
int register_grid(std::unique_ptr<Grid> g) {
  int ctx = INT_MAX - (int) g_grids.size();
  while (g_grids.find(ctx) != g_grids.end())
    --ctx;
  g_grids.emplace(ctx, std::move(g));
  return ctx;
}
}  // namespace

Grid* dlaf_mi355x::find_grid(int ctx) {
  auto it = g_grids.find(ctx);
  return it == g_grids.end() ? nullptr : it->second.get();
}

Grid& dlaf_mi355x::grid_from_context(int ctx) {
  Grid* g = find_grid(ctx);
  if (!g)
    // reference: src/c_api/utils.cpp:55-68 prints this and terminates
    fatal("[ERROR] No DLA-Future grid for context %d. Did you forget to call dlaf_create_grid()?\n", ctx);
  return *g;
}

namespace {

bool coords_from_rank(int rank, int nprow, int npcol, char order, int& myrow, int& mycol) {
  if (in_set(order, "Cc")) {  // reference: common/index2d.h:345-355
    myrow = rank % nprow;
    mycol = rank / nprow;
  }
  else {
    myrow = rank / npcol;
    mycol = rank % npcol;
  }
  return myrow < nprow && mycol < npcol;
}

std::unique_ptr<Grid> make_grid(int nranks, int rank, int nprow, int npcol, char order) {
  if (nprow < 1 || npcol < 1 || nprow * npcol != nranks || rank < 0 || rank >= nranks)
    return nullptr;
  auto g = std::make_unique<Grid>();
  g->nprow = nprow;
  g->npcol = npcol;
  g->rank = rank;
  g->nranks = nranks;
  g->order = in_set(order, "Cc") ? 'C' : 'R';
  coords_from_rank(rank, nprow, npcol, g->order, g->myrow, g->mycol);
  return g;
}

template <class HT>
int cholesky_host(int ctx, char uplo, HT* a, const DLAF_descriptor& d) {
  using DT = typename DevType<HT>::type;
  require_square_desc(d);
  require_uplo(uplo);
  Grid& g = grid_from_context(ctx);
  require_sources(nullptr, g, {&d});
  DeviceMatrix<DT> m;
  m.create(&g, uplo, d.m, d.nb, d.isrc, d.jsrc);
  m.upload(reinterpret_cast<const DT*>(a), d.ld);
  // (a matrix that is not positive definite comes back partially overwritten, as from LAPACK)
  return m.factorize_and_download(reinterpret_cast<DT*>(a), d.ld);
}

template <class HT>
void pxpotrf(char uplo, int n, HT* a, int ia, int ja, const int desca[9], int* info) {
  // reference: src/c_api/factorization/cholesky.h:65-75
  const int ctx = require_scalapack_args({{'A', desca, ia, ja}});
  const int r = cholesky_host<HT>(ctx, uplo, a, make_dlaf_descriptor(n, n, ia, ja, desca));
  if (info)
    *info = r;
}

static void* mpi_shim_handle() {
  static void* handle = []() -> void* {
    Dl_info info;
    std::string path = "libdlaf_mi355x_mpi.so";
    if (dladdr(reinterpret_cast<void*>(&dlaf_free_grid), &info) != 0 && info.dli_fname != nullptr) {
      std::string self = info.dli_fname;
      const size_t slash = self.rfind('/');
      if (slash != std::string::npos)
        path = self.substr(0, slash + 1) + path;
    }
    void* h = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (h == nullptr)
      fatal("[dlaf_mi355x] the MPI-typed grid entry points need %s (built by `make -C dla_future_amd/csrc mpi` when an "
            "MPI is installed): %s\n", path.c_str(), dlerror());
    return h;
  }();
  return handle;
}
template <class F>
static F mpi_shim_symbol(const char* name, F self) {
  F f = reinterpret_cast<F>(dlsym(mpi_shim_handle(), name));
  if (f == nullptr || f == self)
    fatal("[dlaf_mi355x] libdlaf_mi355x_mpi.so does not define %s\n", name);
  return f;
}
}  // namespace

// =================================================================================== dlaf_c
extern "C" {

void dlaf_initialize(int, const char**, int argc_dlaf, const char** argv_dlaf) noexcept {
  const bool first = !runtime_initialized();
  runtime_init();
  // tune parameters (src/init.cpp:211-221: the environment variable first, the command-line option overrides it)
  if (first) {
    if (const char* e = std::getenv("DLAF_EIGENSOLVER_MIN_BAND"))
      set_eigensolver_min_band(std::atoi(e));
    for (int i = 0; argv_dlaf && i < argc_dlaf; ++i) {
      static const char opt[] = "--dlaf:eigensolver-min-band";
      if (!argv_dlaf[i] || std::strncmp(argv_dlaf[i], opt, sizeof(opt) - 1) != 0)
        continue;
      const char* v = argv_dlaf[i] + sizeof(opt) - 1;
      if (*v == '=')
        set_eigensolver_min_band(std::atoi(v + 1));
      else if (*v == 0 && i + 1 < argc_dlaf && argv_dlaf[i + 1])
        set_eigensolver_min_band(std::atoi(argv_dlaf[++i]));
    }
  }
  for (int i = 0; first && argv_dlaf && i < argc_dlaf; ++i)
    if (argv_dlaf[i] && std::strcmp(argv_dlaf[i], "--dlaf:print-config") == 0) {
      int dev = -1;
      (void) hipGetDevice(&dev);
      hipDeviceProp_t p;
      (void) hipGetDeviceProperties(&p, dev);
      std::printf("DLA-Future MI355X build: device %d (%s, %d CUs), diag block %d\n", dev, p.gcnArchName,
                  p.multiProcessorCount, kDiagBlock);
    }
}

void dlaf_finalize(void) noexcept {
  g_grids.clear();
  runtime_finalize();
}

void dlaf_free_grid(int context) noexcept {
  g_grids.erase(context);
}

DLAF_descriptor make_dlaf_descriptor(const int m, const int n, const int i, const int j, const int desc[9]) noexcept {
  if (i != 1 || j != 1)
    fatal("[dlaf_mi355x] make_dlaf_descriptor: i = %d, j = %d must be 1\n", i, j);
  DLAF_descriptor d = {m, n, desc[4], desc[5], desc[6], desc[7], i - 1, j - 1, desc[8]};
  return d;
}

int dlaf_cholesky_factorization_s(const int ctx, const char uplo, float* a, const DLAF_descriptor d) noexcept {
  return cholesky_host<float>(ctx, uplo, a, d);
}
int dlaf_cholesky_factorization_d(const int ctx, const char uplo, double* a, const DLAF_descriptor d) noexcept {
  return cholesky_host<double>(ctx, uplo, a, d);
}
int dlaf_cholesky_factorization_c(const int ctx, const char uplo, dlaf_complex_c* a, const DLAF_descriptor d) noexcept {
  return cholesky_host<std::complex<float>>(ctx, uplo, a, d);
}
int dlaf_cholesky_factorization_z(const int ctx, const char uplo, dlaf_complex_z* a, const DLAF_descriptor d) noexcept {
  return cholesky_host<std::complex<double>>(ctx, uplo, a, d);
}

void dlaf_pspotrf(const char uplo, const int n, float* a, const int ia, const int ja, const int desca[9],
                  int* info) noexcept {
  pxpotrf<float>(uplo, n, a, ia, ja, desca, info);
}
void dlaf_pdpotrf(const char uplo, const int n, double* a, const int ia, const int ja, const int desca[9],
                  int* info) noexcept {
  pxpotrf<double>(uplo, n, a, ia, ja, desca, info);
}
void dlaf_pcpotrf(const char uplo, const int n, dlaf_complex_c* a, const int ia, const int ja, const int desca[9],
                  int* info) noexcept {
  pxpotrf<std::complex<float>>(uplo, n, a, ia, ja, desca, info);
}
void dlaf_pzpotrf(const char uplo, const int n, dlaf_complex_z* a, const int ia, const int ja, const int desca[9],
                  int* info) noexcept {
  pxpotrf<std::complex<double>>(uplo, n, a, ia, ja, desca, info);
}

// =================================================================================== extensions
const char* dlaf_mi355x_version(void) noexcept {
  return "dlaf_mi355x 0.1 gfx950";
}

int dlaf_mi355x_create_grid_single(void) noexcept {
  return register_grid(make_grid(1, 0, 1, 1, 'R'));
}

void dlaf_mi355x_rccl_unique_id(void* out) noexcept {
  runtime_init();
  rccl_get_unique_id(out);
}

int dlaf_mi355x_create_grid_rccl(const void* uid, int nranks, int rank, int nprow, int npcol, char order) noexcept {
  auto g = make_grid(nranks, rank, nprow, npcol, order);
  if (!g)
    return -1;
  runtime_init();
  // a 1-process grid needs no communicator; DLAF_MI355X_RCCL_SINGLE=1 creates them anyway (communicator
  // init / split / teardown exercised on a one-GPU box)
  const char* force = std::getenv("DLAF_MI355X_RCCL_SINGLE");
  if (nranks > 1 || (force && force[0] == '1'))
    g->transport = make_rccl_transport(uid, nranks, rank, nprow, npcol, g->myrow, g->mycol);
  return register_grid(std::move(g));
}

int dlaf_mi355x_create_grid_host(int nranks, int rank, int nprow, int npcol, char order, dlaf_mi355x_bcast_fn bcast,
                                 dlaf_mi355x_barrier_fn barrier, void* user) noexcept {
  auto g = make_grid(nranks, rank, nprow, npcol, order);
  if (!g || (nranks > 1 && !bcast))
    return -1;
  if (nranks > 1) {
    g->host_bcast = bcast;
    g->host_user = user;
    g->host_barrier = barrier;
    // the transport itself (pinned staging buffer, HIP) is created on first use by a matrix
  }
  return register_grid(std::move(g));
}

int dlaf_mi355x_grid_rekey(int ctx, int new_ctx) noexcept {
  auto it = g_grids.find(ctx);
  if (it == g_grids.end())
    return -1;
  if (ctx == new_ctx)
    return 0;
  if (g_grids.find(new_ctx) != g_grids.end())
    return -2;
  std::unique_ptr<Grid> g = std::move(it->second);
  g_grids.erase(it);
  g_grids.emplace(new_ctx, std::move(g));
  return 0;
}

int dlaf_mi355x_grid_on_free(int ctx, void (*fn)(void*), void* user) noexcept {
  Grid* g = find_grid(ctx);
  if (!g)
    return -1;
  g->on_free = fn;
  g->on_free_user = user;
  return 0;
}

int dlaf_mi355x_grid_comm_log(int ctx, int enable) noexcept {
  Grid* g = find_grid(ctx);
  if (!g)
    return -1;
  g->comm_log_on = enable != 0;
  g->comm_log.clear();
  if (g->comm_log_on && runtime_initialized())
    (void) grid_transport(*g);
  return 0;
}

long dlaf_mi355x_grid_comm_log_read(int ctx, long* out, long cap_events) noexcept {
  Grid* g = find_grid(ctx);
  if (!g)
    return -1;
  const auto& log = g->comm_log;
  for (long i = 0; out && i < cap_events && i < (long) log.size(); ++i) {
    out[4 * i + 0] = log[(size_t) i].kind;
    out[4 * i + 1] = log[(size_t) i].root;
    out[4 * i + 2] = log[(size_t) i].bytes;
    out[4 * i + 3] = log[(size_t) i].group;
  }
  return (long) log.size();
}

int dlaf_mi355x_grid_info(int ctx, int* nprow, int* npcol, int* myrow, int* mycol) noexcept {
  Grid* g = find_grid(ctx);
  if (!g)
    return -1;
  if (nprow) *nprow = g->nprow;
  if (npcol) *npcol = g->npcol;
  if (myrow) *myrow = g->myrow;
  if (mycol) *mycol = g->mycol;
  return 0;
}

int dlaf_mi355x_grid_barrier(int ctx) noexcept {
  Grid* g = find_grid(ctx);
  if (!g)
    return -1;
  if (g->transport)
    g->transport->barrier(nullptr);
  else if (g->host_barrier)
    return g->host_barrier(g->host_user);
  else if (runtime_initialized())
    (void) hipDeviceSynchronize();
  return 0;
}

int dlaf_mi355x_grid_selftest(int ctx, size_t bytes) noexcept {
  Grid* g = find_grid(ctx);
  if (!g)
    return -1;
  return grid_selftest(*g, bytes);
}

int dlaf_mi355x_grid_host_bcast(int ctx, int axis, int root, void* host_buf, size_t bytes) noexcept {
  // exercises the grid's broadcast callback with a caller-owned HOST buffer (no GPU involved):
  // lets CPU-only multi-process tests check the row/column communicator wiring of a host grid
  Grid* g = find_grid(ctx);
  if (!g || (axis != 0 && axis != 1))
    return -1;
  if (!g->host_bcast)
    return g->nranks == 1 ? 0 : -2;
  return g->host_bcast(g->host_user, axis, root, host_buf, bytes);
}

// ---- MPI-typed entries of the reference's grid.h (dlaf_create_grid, grid_ordering, dlaf_create_grid_from_blacs) -----
// They live in the optional shim libdlaf_mi355x_mpi.so (mpi_grid.cpp), the only object of this build that sees
// <mpi.h>.  So that a caller of the reference's interface can link -ldlaf_mi355x alone, as it links -ldlaf upstream,
// the core exports forwarders under the same names: the first call loads the shim from this library's directory and
// jumps to its definition.  MPI_Comm is an int (MPICH ABI) or a pointer (Open MPI): either way the first integer
// argument register of the x86-64 psABI, which a forwarder declared with a pointer-sized first parameter passes on
// untouched.  A program that links the shim itself binds to the shim's definitions directly (it comes first in the
// link order) and never gets here.
int dlaf_create_grid(void* comm, int nprow, int npcol, char order) noexcept {
  using fn = int (*)(void*, int, int, char);
  static const fn f = mpi_shim_symbol<fn>("dlaf_create_grid", &dlaf_create_grid);
  return f(comm, nprow, npcol, order);
}
char grid_ordering(void* comm, int nprow, int npcol, int myprow, int mypcol) noexcept {
  using fn = char (*)(void*, int, int, int, int);
  static const fn f = mpi_shim_symbol<fn>("grid_ordering", &grid_ordering);
  return f(comm, nprow, npcol, myprow, mypcol);
}
void dlaf_create_grid_from_blacs(int blacs_ctxt) noexcept {
  using fn = void (*)(int);
  static const fn f = mpi_shim_symbol<fn>("dlaf_create_grid_from_blacs", &dlaf_create_grid_from_blacs);
  f(blacs_ctxt);
}

}  // extern "C"
