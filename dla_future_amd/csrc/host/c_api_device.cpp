// c_api_device.cpp -- the extern "C" surface, part 3 of 3 (c_api_internal.hpp has the map): the device-resident
// matrix / gmatrix handles and the *_device entries over them, the profiles and statistics of the last call, and the
// hooks the tests and bench.py use to reach single kernels and plans (tile_*, *_direct, dist_*, inverse and
// partial-spectrum plans), all declared in include/dlaf_mi355x/dlaf_mi355x.h.
#define DLAF_MI355X_NO_MPI 1  // as in c_api.cpp: no <mpi.h> in the core
#include <algorithm>
#include <complex>
#include <memory>

#include <dlaf_mi355x/dlaf_mi355x.h>

#include "c_api_internal.hpp"
#include "device_matrix.hpp"
#include "direct.hpp"
#include "drivers.hpp"
#include "eigensolver.hpp"
#include "pool.hpp"
#include "red2band.hpp"
#include "tile_matrix.hpp"

using namespace dlaf_mi355x;

namespace dlaf_mi355x {
template <class T>
void set_random_hpd_local(T* a, long ld, long n, int nb, const Axis& rows, const Axis& cols, int nthreads);
}

// the handles: a Hermitian / triangular matrix in the tile layout (type: its letter), and a general one
struct dlaf_mi355x_matrix_s {
  std::unique_ptr<MatrixBase> m;
  char type;
  int ctx;
};
struct dlaf_mi355x_gmatrix_s {
  std::unique_ptr<MatrixBase> m;
  int ctx;
};

namespace {
// dispatch_type (runtime.hpp) on a type letter that comes from the caller: -2 for one that names no type
template <class F>
int dispatch_api_type(char type, F&& f) {
  return dispatch_type(type, f, [] { return -2; });
}
}  // namespace

extern "C" {

int dlaf_mi355x_partial_spectrum_plan(long n, int nb, int npcol, int mycol, int z_jsrc, long begin, long end,
                                      long out[5]) noexcept {
  check_eigenvalues_index("partial_spectrum_plan", n, begin, end);
  const PartialSpectrumPlan p = partial_spectrum_plan(n, nb, npcol, mycol, z_jsrc, begin, end);
  const long v[5] = {p.b0, p.jsrc, p.ncl, p.first, p.pad};
  std::copy(v, v + 5, out);
  return 0;
}
int dlaf_mi355x_eigensolver_profile(double ms[5]) noexcept {
  eigensolver_last_profile(ms);
  return 0;
}

int dlaf_mi355x_red2band_panel_stats(long* blocked, long* fallback) noexcept {
  red2band_last_panels(blocked, fallback);
  return 0;
}
long dlaf_mi355x_workspace_pool_release(void) noexcept {
  const long held = (long) pool_idle_bytes();
  pool_release();
  return held;
}
int dlaf_mi355x_red2band_profile(double* ms, double* flops) noexcept {
  red2band_last_profile(ms, flops);
  return 0;
}

// ---- device-resident operands for the solver ----------------------------------------------------------------
int dlaf_mi355x_gmatrix_create(int ctx, char type, DLAF_descriptor d, dlaf_mi355x_gmatrix_t* out) noexcept {
  Grid* g = out ? find_grid(ctx) : nullptr;
  if (!g)
    return -1;
  if (d.i != 0 || d.j != 0 || d.m < 0 || d.n < 0 || d.mb != d.nb || d.nb < 1)
    return -3;  // square blocks only in this build
  if (!source_in_grid(*g, d))
    return -3;
  MatrixBase* m = general_matrix_create(g, type, d.m, d.n, d.nb, d.isrc, d.jsrc);
  if (!m)
    return -2;
  auto* h = new dlaf_mi355x_gmatrix_s;
  h->m.reset(m);
  h->ctx = ctx;
  *out = h;
  return 0;
}
void dlaf_mi355x_gmatrix_destroy(dlaf_mi355x_gmatrix_t h) noexcept {
  delete h;
}
int dlaf_mi355x_gmatrix_upload(dlaf_mi355x_gmatrix_t h, const void* host, int ld) noexcept {
  if (!h || !h->m)
    return -1;
  general_matrix_transfer(h->m.get(), const_cast<void*>(host), ld, true);
  return 0;
}
int dlaf_mi355x_gmatrix_download(dlaf_mi355x_gmatrix_t h, void* host, int ld) noexcept {
  if (!h || !h->m)
    return -1;
  general_matrix_transfer(h->m.get(), host, ld, false);
  return 0;
}
// how the judgements of api_checks.hpp see a resident operand: a general matrix as stored, and the n x n matrix of the
// caller whose triangle a matrix handle holds (stored: that triangle's letter)
static OperandDesc general_operand(dlaf_mi355x_gmatrix_t h) {
  OperandDesc o{};
  (void) dispatch_api_type(h->m->type, [&](auto* tag) {
    using DT = std::remove_pointer_t<decltype(tag)>;
    const auto& gm = static_cast<GeneralMatrix<DT>&>(*h->m);
    o = OperandDesc{gm.rows_g, gm.cols_g, gm.m.nb, gm.m.nb, gm.isrc, gm.jsrc};
    return 0;
  });
  return o;
}
static OperandDesc triangle_operand(dlaf_mi355x_matrix_t h, char* stored = nullptr) {
  OperandDesc o{};
  (void) dispatch_api_type(h->m->type, [&](auto* tag) {
    using DT = std::remove_pointer_t<decltype(tag)>;
    const auto& dm = static_cast<DeviceMatrix<DT>&>(*h->m);
    const Axis& srow = dm.transposed ? dm.cols : dm.rows;
    const Axis& scol = dm.transposed ? dm.rows : dm.cols;
    o = OperandDesc{dm.n, dm.n, dm.nb, dm.nb, srow.src, scol.src};
    if (stored)
      *stored = dm.uplo;
    return 0;
  });
  return o;
}

int dlaf_mi355x_triangular_solver_device(char side, char uplo, char op, char diag, const void* alpha,
                                         dlaf_mi355x_matrix_t a, dlaf_mi355x_gmatrix_t b) noexcept {
  if (!a || !a->m || !b || !b->m || a->ctx != b->ctx)
    return -1;
  char stored = 0;
  const OperandDesc oa = triangle_operand(a, &stored);
  require_triangular("triangular solver", grid_from_context(a->ctx), side, uplo, op, diag, oa, general_operand(b), stored);
  return triangular_solver_device(side, uplo, op, diag, alpha, a->m.get(), b->m.get());
}
// A X = B from the resident factor (p?potrs without leaving HBM): two solves, nothing crosses PCIe in between
int dlaf_mi355x_potrs_device(char uplo, dlaf_mi355x_matrix_t factor, dlaf_mi355x_gmatrix_t b) noexcept {
  if (!factor || !factor->m || !b || !b->m)
    return -1;
  const bool lower = is_lower(uplo);
  const double one_d[2] = {1.0, 0.0};
  const float one_f[2] = {1.0f, 0.0f};
  const void* one = (factor->type == 's' || factor->type == 'c') ? (const void*) one_f : (const void*) one_d;
  int r = dlaf_mi355x_triangular_solver_device('L', uplo, lower ? 'N' : 'C', 'N', one, factor, b);
  if (r != 0)
    return r;
  return dlaf_mi355x_triangular_solver_device('L', uplo, lower ? 'C' : 'N', 'N', one, factor, b);
}

int dlaf_mi355x_solver_profile(double* ms, double* flops) noexcept {
  solver_last_profile(ms, flops);
  return 0;
}

int dlaf_mi355x_triangular_multiplication_device(char side, char uplo, char op, char diag, const void* alpha,
                                                 dlaf_mi355x_matrix_t a, dlaf_mi355x_gmatrix_t b) noexcept {
  if (!a || !a->m || !b || !b->m || a->ctx != b->ctx)
    return -1;
  char stored = 0;
  const OperandDesc oa = triangle_operand(a, &stored);
  require_triangular("triangular multiplication", grid_from_context(a->ctx), side, uplo, op, diag, oa, general_operand(b),
                     stored);
  return triangular_multiplication_device(side, uplo, op, diag, alpha, a->m.get(), b->m.get());
}

int dlaf_mi355x_hermitian_multiplication_device(char side, char uplo, const void* alpha, dlaf_mi355x_matrix_t a,
                                               dlaf_mi355x_gmatrix_t b, const void* beta,
                                               dlaf_mi355x_gmatrix_t c) noexcept {
  if (!a || !a->m || !b || !b->m || !c || !c->m || a->ctx != b->ctx || a->ctx != c->ctx)
    return -1;
  char stored = 0;
  const OperandDesc oa = triangle_operand(a, &stored);
  require_hermitian_multiplication("hermitian multiplication", grid_from_context(a->ctx), side, uplo, oa,
                                   general_operand(b), general_operand(c), stored);
  return hermitian_multiplication_device(side, uplo, alpha, a->m.get(), b->m.get(), beta, c->m.get());
}

int dlaf_mi355x_general_multiplication_device(char opa, char opb, const void* alpha, dlaf_mi355x_gmatrix_t a,
                                              dlaf_mi355x_gmatrix_t b, const void* beta,
                                              dlaf_mi355x_gmatrix_t c) noexcept {
  const char* who = "general multiplication";
  if (!a || !a->m || !b || !b->m || !c || !c->m || !alpha || !beta)
    return -1;
  if (a->ctx != b->ctx || a->ctx != c->ctx)
    fatal("[dlaf_mi355x] %s: A, B and C live on different contexts (%d, %d, %d)\n", who, a->ctx, b->ctx, c->ctx);
  if (a->m->type != c->m->type || b->m->type != c->m->type)
    fatal("[dlaf_mi355x] %s: operands of different element types ('%c', '%c', '%c')\n", who, a->m->type, b->m->type,
          c->m->type);
  require_general_multiplication(who, grid_from_context(c->ctx), opa, opb, general_operand(a), general_operand(b),
                                 general_operand(c));
  return general_multiplication_device(opa, opb, alpha, a->m.get(), b->m.get(), beta, c->m.get());
}

// b null: rank-k (alpha points to a real), else rank-2k (alpha points to an element); beta points to a real
static int rank_update_device(const char* who, char uplo, char trans, const void* alpha, dlaf_mi355x_gmatrix_t a,
                              dlaf_mi355x_gmatrix_t b, bool her2k, const void* beta, dlaf_mi355x_matrix_t c) {
  if (!a || !a->m || !c || !c->m || !alpha || !beta || (her2k && (!b || !b->m)))
    return -1;
  if (a->ctx != c->ctx || (her2k && b->ctx != c->ctx))
    fatal("[dlaf_mi355x] %s: the operands live on different contexts (A %d, C %d)\n", who, a->ctx, c->ctx);
  if (a->m->type != c->m->type || (her2k && b->m->type != c->m->type))
    fatal("[dlaf_mi355x] %s: operands of different element types (A '%c', C '%c')\n", who, a->m->type, c->m->type);
  char stored = 0;
  const OperandDesc oa = general_operand(a), ob = general_operand(her2k ? b : a), oc = triangle_operand(c, &stored);
  const bool cx = c->m->type == 'c' || c->m->type == 'z';
  require_rank_update(who, grid_from_context(c->ctx), cx, uplo, trans, oa, her2k ? &ob : nullptr, oc, stored);
  return hermitian_rank_update_device(trans, alpha, a->m.get(), her2k ? b->m.get() : nullptr, beta, c->m.get());
}
int dlaf_mi355x_hermitian_rank_k_update_device(char uplo, char trans, const void* alpha, dlaf_mi355x_gmatrix_t a,
                                               const void* beta, dlaf_mi355x_matrix_t c) noexcept {
  return rank_update_device("hermitian rank-k update", uplo, trans, alpha, a, nullptr, false, beta, c);
}
int dlaf_mi355x_hermitian_rank_2k_update_device(char uplo, char trans, const void* alpha, dlaf_mi355x_gmatrix_t a,
                                                dlaf_mi355x_gmatrix_t b, const void* beta,
                                                dlaf_mi355x_matrix_t c) noexcept {
  return rank_update_device("hermitian rank-2k update", uplo, trans, alpha, a, b, true, beta, c);
}
int dlaf_mi355x_hermitian_weighted_rank_k_update_device(char uplo, char trans, const void* alpha, dlaf_mi355x_gmatrix_t a,
                                                        const void* d, const void* beta,
                                                        dlaf_mi355x_matrix_t c) noexcept {
  const char* who = "hermitian weighted rank-k update";
  if (!a || !a->m || !c || !c->m || !alpha || !beta)
    return -1;
  if (a->ctx != c->ctx)
    fatal("[dlaf_mi355x] %s: the operands live on different contexts (A %d, C %d)\n", who, a->ctx, c->ctx);
  if (a->m->type != c->m->type)
    fatal("[dlaf_mi355x] %s: operands of different element types (A '%c', C '%c')\n", who, a->m->type, c->m->type);
  char stored = 0;
  const OperandDesc oa = general_operand(a), oc = triangle_operand(c, &stored);
  const char t = c->m->type;
  const bool cx = t == 'c' || t == 'z';
  const bool alpha_zero = (t == 's' || t == 'c') ? *static_cast<const float*>(alpha) == 0.0f
                                                 : *static_cast<const double*>(alpha) == 0.0;
  require_weighted_rank_update(grid_from_context(c->ctx), cx, uplo, trans, alpha_zero, oa, d, oc, stored);
  // (a null d is the plain update to the driver; it is null only where no weight would be read)
  return hermitian_rank_update_device(trans, alpha, a->m.get(), nullptr, beta, c->m.get(), d);
}

// Functions of a resident Hermitian matrix (matrix_function.cpp): A := f(A) in place
extern "C++" {
template <class DT>
static int function_device(const char* who, dlaf_mi355x_matrix_t a, real_t<DT>* w, SpectralWeights fn, void* self,
                           const long* index_range, const real_t<DT>* value_interval, long* selected) {
  using R = real_t<DT>;
  char stored = 0;
  const OperandDesc oa = triangle_operand(a, &stored);
  require_hermitian_function(who, grid_from_context(a->ctx), stored, oa, index_range != nullptr,
                             value_interval != nullptr);
  SpectralSelection<R> sel(oa.n, index_range, value_interval);
  if (!sel.by_value)
    check_eigenvalues_index(who, oa.n, sel.begin, sel.end);
  const int r = hermitian_function_resident<DT>(static_cast<DeviceMatrix<DT>&>(*a->m), w, sel.by_value ? sel.values : nullptr,
                                                sel.begin, sel.end, fn, self);
  if (selected) {
    selected[0] = sel.begin;
    selected[1] = sel.end;
  }
  return r;
}
}  // extern "C++"
int dlaf_mi355x_hermitian_function_device(dlaf_mi355x_matrix_t a, void* w, void* weights, void* user,
                                          const long* index_range, const void* value_interval,
                                          long* selected) noexcept {
  if (!a || !a->m || !w || !weights)
    return -1;
  return dispatch_api_type(a->type, [&](auto* tag) -> int {
    using DT = std::remove_pointer_t<decltype(tag)>;
    using R = real_t<DT>;
    SpectralWeightsCall<R> call{reinterpret_cast<void (*)(long, const R*, long, long, R*, void*)>(weights), user};
    return function_device<DT>("hermitian function", a, static_cast<R*>(w), &SpectralWeightsCall<R>::call, &call,
                               index_range, static_cast<const R*>(value_interval), selected);
  });
}
int dlaf_mi355x_hermitian_power_device(dlaf_mi355x_matrix_t a, void* w, double exponent, double threshold,
                                       long* n_dropped) noexcept {
  if (!a || !a->m || !w)
    return -1;
  require_power_threshold("hermitian power", threshold);
  return dispatch_api_type(a->type, [&](auto* tag) -> int {
    using DT = std::remove_pointer_t<decltype(tag)>;
    using R = real_t<DT>;
    const R interval[2] = {(R) threshold, std::numeric_limits<R>::infinity()};
    SpectralPower<R> p{exponent};
    long sel[2] = {0, 0};
    const int r = function_device<DT>("hermitian power", a, static_cast<R*>(w), &SpectralPower<R>::call, &p, nullptr,
                                      interval, sel);
    if (n_dropped)
      *n_dropped = sel[0];
    return r;
  });
}

// general_addition / hermitian_complete on resident general matrices, and the conversions between a DeviceMatrix and a
// general matrix (addition.cpp)
int dlaf_mi355x_general_addition_device(char uplo, char op, const void* alpha, dlaf_mi355x_gmatrix_t a, const void* beta,
                                        dlaf_mi355x_gmatrix_t c) noexcept {
  const char* who = "general addition";
  if (!a || !a->m || !c || !c->m || !alpha || !beta)
    return -1;
  if (a->ctx != c->ctx)
    fatal("[dlaf_mi355x] %s: the operands live on different contexts (A %d, C %d)\n", who, a->ctx, c->ctx);
  if (a->m->type != c->m->type)
    fatal("[dlaf_mi355x] %s: operands of different element types (A '%c', C '%c')\n", who, a->m->type, c->m->type);
  require_general_addition(who, grid_from_context(c->ctx), uplo, op, general_operand(a), general_operand(c),
                           a->m.get() == c->m.get());
  return general_addition_device(uplo, op, alpha, a->m.get(), beta, c->m.get());
}
int dlaf_mi355x_hermitian_complete_device(char uplo, char kind, dlaf_mi355x_gmatrix_t a) noexcept {
  if (!a || !a->m)
    return -1;
  require_hermitian_complete("hermitian complete", grid_from_context(a->ctx), uplo, kind, general_operand(a));
  return hermitian_complete_device(uplo, kind, a->m.get());
}
static int matrix_conversion(const char* who, char kind, const char* kinds, dlaf_mi355x_matrix_t m, dlaf_mi355x_gmatrix_t g,
                             bool to_general) {
  if (!m || !m->m || !g || !g->m)
    return -1;
  if (m->ctx != g->ctx)
    fatal("[dlaf_mi355x] %s: the operands live on different contexts (%d, %d)\n", who, m->ctx, g->ctx);
  if (m->m->type != g->m->type)
    fatal("[dlaf_mi355x] %s: operands of different element types ('%c', '%c')\n", who, m->m->type, g->m->type);
  require_matrix_conversion(who, kind, kinds, triangle_operand(m), general_operand(g));
  return to_general ? matrix_to_general(kind, m->m.get(), g->m.get()) : matrix_from_general(m->m.get(), g->m.get());
}
int dlaf_mi355x_matrix_to_general(char kind, dlaf_mi355x_matrix_t m, dlaf_mi355x_gmatrix_t g) noexcept {
  return matrix_conversion("general addition: matrix_to_general", kind, "HhSsTt", m, g, true);
}
int dlaf_mi355x_matrix_from_general(dlaf_mi355x_matrix_t m, dlaf_mi355x_gmatrix_t g) noexcept {
  return matrix_conversion("general addition: matrix_from_general", 0, "", m, g, false);
}
int dlaf_mi355x_addition_profile(double* ms, double* bytes) noexcept {
  addition_last_profile(ms, bytes);
  return 0;
}

int dlaf_mi355x_multiplication_profile(double* ms, double* flops) noexcept {
  multiplication_last_profile(ms, flops);
  return 0;
}

int dlaf_mi355x_matrix_create(int ctx, char type, char uplo, DLAF_descriptor d, dlaf_mi355x_matrix_t* out) noexcept {
  Grid* g = out ? find_grid(ctx) : nullptr;
  if (!g)
    return -1;
  if (d.i != 0 || d.j != 0 || d.m != d.n || d.mb != d.nb || d.nb < 1 || d.m < 0 || !source_in_grid(*g, d))
    return -3;
  if (!is_uplo(uplo))
    return -4;
  auto* h = new dlaf_mi355x_matrix_s;
  h->type = type;
  h->ctx = ctx;
  const int r = dispatch_api_type(type, [&](auto* tag) {
    using DT = std::remove_pointer_t<decltype(tag)>;
    auto m = std::make_unique<DeviceMatrix<DT>>();
    m->create(g, uplo, d.m, d.nb, d.isrc, d.jsrc);
    h->m = std::move(m);
    return 0;
  });
  if (r != 0) {
    delete h;
    return r;
  }
  *out = h;
  return 0;
}

void dlaf_mi355x_matrix_destroy(dlaf_mi355x_matrix_t m) noexcept {
  delete m;
}

#define WITH_MATRIX(handle, body)                                       \
  if (!(handle) || !(handle)->m)                                        \
    return -1;                                                          \
  return dispatch_api_type((handle)->type, [&](auto* tag) -> int {         \
    using DT = std::remove_pointer_t<decltype(tag)>;                    \
    auto& M = static_cast<DeviceMatrix<DT>&>(*(handle)->m);             \
    body                                                                \
  });

int dlaf_mi355x_matrix_upload(dlaf_mi355x_matrix_t h, const void* host, int ld) noexcept {
  WITH_MATRIX(h, M.upload(static_cast<const DT*>(host), ld); return 0;)
}
int dlaf_mi355x_matrix_download(dlaf_mi355x_matrix_t h, void* host, int ld) noexcept {
  WITH_MATRIX(h, M.download(static_cast<DT*>(host), ld); return 0;)
}
int dlaf_mi355x_matrix_copy(dlaf_mi355x_matrix_t dst, dlaf_mi355x_matrix_t src) noexcept {
  if (!src || !dst || src->type != dst->type)
    return -1;
  WITH_MATRIX(dst, M.copy_from(static_cast<DeviceMatrix<DT>&>(*src->m)); return 0;)
}
int dlaf_mi355x_matrix_fetch_tile(dlaf_mi355x_matrix_t h, long gi, long gj, void* host, int ld) noexcept {
  WITH_MATRIX(h, return M.fetch_tile(gi, gj, static_cast<DT*>(host), ld) ? 0 : 1;)
}
int dlaf_mi355x_cholesky_start(dlaf_mi355x_matrix_t h) noexcept {
  WITH_MATRIX(h, M.factorize_async(); return 0;)
}
int dlaf_mi355x_cholesky_wait(dlaf_mi355x_matrix_t h) noexcept {
  WITH_MATRIX(h, return M.wait();)
}
int dlaf_mi355x_cholesky_factorization_device(dlaf_mi355x_matrix_t h) noexcept {
  WITH_MATRIX(h, return M.factorize();)
}
int dlaf_mi355x_matrix_local_info(dlaf_mi355x_matrix_t h) noexcept {
  WITH_MATRIX(h, return M.local_info;)
}
int dlaf_mi355x_update_launch_stats(long* persistent, long* exclusive) noexcept {
  long a = 0, b = 0;
  update_launch_stats(&a, &b);
  if (persistent)
    *persistent = a;
  if (exclusive)
    *exclusive = b;
  return 0;
}
int dlaf_mi355x_potrf_trace(unsigned long long* out) noexcept {
  unsigned long long* tb = potrf_coop_trace_buffer();
  if (tb == nullptr || out == nullptr)
    return 1;
  (void) hipDeviceSynchronize();
  return hipMemcpy(out, tb, 32 * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}

int dlaf_mi355x_cholesky_residual(dlaf_mi355x_matrix_t original, dlaf_mi355x_matrix_t factor, double* max_diff,
                                  double* max_a) noexcept {
  if (!original || !factor || original->type != factor->type)
    return -1;
  WITH_MATRIX(original, M.residual_of(static_cast<DeviceMatrix<DT>&>(*factor->m), max_diff, max_a); return 0;)
}

int dlaf_mi355x_generalized_to_standard_device(dlaf_mi355x_matrix_t a, dlaf_mi355x_matrix_t l) noexcept {
  if (!a || !l || a->type != l->type)
    return -1;
  WITH_MATRIX(a, return gen_to_std_device(M, static_cast<DeviceMatrix<DT>&>(*l->m));)
}

int dlaf_mi355x_triangular_inverse_device(char uplo, char diag, dlaf_mi355x_matrix_t m) noexcept {
  WITH_MATRIX(m, if (is_upper(uplo) != is_upper(M.uplo)) fatal("[dlaf_mi355x] triangular inverse: the resident matrix holds the "
                                                     "'%c' triangle, not '%c'\n", M.uplo, uplo);
              return triangular_inverse_device(diag, M);)
}
int dlaf_mi355x_inverse_from_cholesky_factor_device(char uplo, dlaf_mi355x_matrix_t m) noexcept {
  WITH_MATRIX(m, if (is_upper(uplo) != is_upper(M.uplo)) fatal("[dlaf_mi355x] inverse from the Cholesky factor: the resident "
                                                     "matrix holds the '%c' triangle, not '%c'\n", M.uplo, uplo);
              return inverse_from_cholesky_factor_device(M);)
}
int dlaf_mi355x_inverse_profile(double* ms, double* flops) noexcept {
  inverse_last_profile(ms, flops);
  return 0;
}
int dlaf_mi355x_inverse_plan(long n, int nb, int nprow, int npcol, int myrow, int mycol, int isrc, int jsrc,
                             long out[9]) noexcept {
  const Axis rows{n, nb, nprow, myrow, isrc}, cols{n, nb, npcol, mycol, jsrc};
  const DiagTiles d = local_diag_tiles(rows, cols);
  const long v[9] = {d.count, d.k0, d.kstep, d.il0, d.jl0, d.il_step, d.jl_step, d.last,
                     inverse_workspace_tiles(rows, cols)};
  std::copy(v, v + 9, out);
  return 0;
}
int dlaf_mi355x_inverse_step(long n, int nb, int nprow, int npcol, int myrow, int mycol, int isrc, int jsrc, long k,
                             long out[7]) noexcept {
  const Axis rows{n, nb, nprow, myrow, isrc}, cols{n, nb, npcol, mycol, jsrc};
  const InverseStep st = inverse_step_ranges(rows, cols, k);
  const long v[7] = {st.own_r, st.own_c, st.il_below, st.nrl, st.ncl, st.lr, st.lc};
  std::copy(v, v + 7, out);
  return 0;
}

int dlaf_mi355x_matrix_norm(dlaf_mi355x_matrix_t m, char norm, char structure, char diag, double* value) noexcept {
  if (!value)
    return -6;
  if (norm_kind(norm) == 0)
    return -1;
  if (!in_set(structure, "HhSsTt"))
    return -4;
  if (in_set(structure, "Tt") && !is_diag(diag))
    return -3;
  WITH_MATRIX(m, *value = structured_norm_device(norm, structure, diag, M); return 0;)
}
int dlaf_mi355x_general_matrix_norm(dlaf_mi355x_gmatrix_t m, char norm, double* value) noexcept {
  if (!m || !m->m || !value)
    return -6;
  if (norm_kind(norm) == 0)
    return -1;
  *value = general_norm_device(norm, m->m.get());
  return 0;
}
int dlaf_mi355x_gmatrix_device_tiles(dlaf_mi355x_gmatrix_t m, const void** tiles, size_t* bytes) noexcept {
  if (!m || !m->m || !tiles || !bytes)
    return -6;
  return dispatch_api_type(m->m->type, [&](auto* tag) -> int {
    using DT = std::remove_pointer_t<decltype(tag)>;
    const auto& t = static_cast<GeneralMatrix<DT>&>(*m->m).m;
    *tiles = t.tiles;
    *bytes = (size_t) t.ltr * t.ltc * t.tile_elems * sizeof(DT);
    return 0;
  });
}
int dlaf_mi355x_norm_profile(double* ms, double* bytes) noexcept {
  norm_last_profile(ms, bytes);
  return 0;
}

int dlaf_mi355x_reduction_to_band_device(dlaf_mi355x_matrix_t a, int band, void* taus) noexcept {
  WITH_MATRIX(a, return reduction_to_band_device(M, band, static_cast<DT*>(taus));)
}
int dlaf_mi355x_bt_reduction_to_band_device(int band, dlaf_mi355x_gmatrix_t c, dlaf_mi355x_matrix_t v,
                                            const void* taus) noexcept {
  if (!c || !c->m || !v || !v->m || c->m->type != v->type)
    return -1;
  WITH_MATRIX(v, return bt_reduction_to_band_device(band, static_cast<GeneralMatrix<DT>&>(*c->m).m, M,
                                                    static_cast<const DT*>(taus));)
}

int dlaf_mi355x_matrix_trsm_profile(dlaf_mi355x_matrix_t h, int reps, double* ms, double* flops, double* bytes) noexcept {
  WITH_MATRIX(h, const double t = M.trsm_profile(reps, flops, bytes); if (ms) *ms = t; return 0;)
}

int dlaf_mi355x_matrix_profile(dlaf_mi355x_matrix_t h, int kind, double* ms, long* launches, double* flops,
                               double* bytes) noexcept {
  if (kind < 0 || kind > 3)
    return -2;
  WITH_MATRIX(h, const auto& p = M.prof[kind]; if (ms) *ms = p.ms; if (launches) *launches = p.launches;
              if (flops) *flops = p.flops; if (bytes) *bytes = p.bytes; return 0;)
}

int dlaf_mi355x_set_random_hpd(int ctx, char type, void* host, DLAF_descriptor d, int nthreads) noexcept {
  const Grid* g = find_grid(ctx);
  if (!g)
    return -1;
  if (d.m != d.n || d.mb != d.nb || d.nb < 1)
    return -3;
  Axis rows{d.m, d.nb, g->nprow, g->myrow, d.isrc}, cols{d.n, d.nb, g->npcol, g->mycol, d.jsrc};
  return dispatch_api_type(type, [&](auto* tag) {
    using DT = std::remove_pointer_t<decltype(tag)>;
    using HT = std::conditional_t<TypeInfo<DT>::is_complex, std::complex<real_t<DT>>, DT>;
    set_random_hpd_local(static_cast<HT*>(host), d.ld, d.m, d.nb, rows, cols, nthreads);
    return 0;
  });
}

int dlaf_mi355x_tile_potrf(char type, char uplo, int n, void* a, int lda) noexcept {
  return dispatch_api_type(type, [&](auto* tag) {
    using DT = std::remove_pointer_t<decltype(tag)>;
    return tile_potrf<DT>(uplo, n, static_cast<DT*>(a), lda);
  });
}
int dlaf_mi355x_tile_trsm(char type, char uplo, int m, int n, const void* a, int lda, void* b, int ldb) noexcept {
  return dispatch_api_type(type, [&](auto* tag) {
    using DT = std::remove_pointer_t<decltype(tag)>;
    tile_trsm<DT>(uplo, m, n, static_cast<const DT*>(a), lda, static_cast<DT*>(b), ldb);
    return 0;
  });
}
int dlaf_mi355x_tile_herk(char type, char uplo, int n, int k, const void* a, int lda, void* c, int ldc) noexcept {
  return dispatch_api_type(type, [&](auto* tag) {
    using DT = std::remove_pointer_t<decltype(tag)>;
    tile_herk<DT>(uplo, n, k, static_cast<const DT*>(a), lda, static_cast<DT*>(c), ldc);
    return 0;
  });
}
int dlaf_mi355x_tile_gemm(char type, char uplo, int m, int n, int k, const void* a, int lda, const void* b, int ldb,
                          void* c, int ldc) noexcept {
  return dispatch_api_type(type, [&](auto* tag) {
    using DT = std::remove_pointer_t<decltype(tag)>;
    tile_gemm<DT>(uplo, m, n, k, static_cast<const DT*>(a), lda, static_cast<const DT*>(b), ldb, static_cast<DT*>(c), ldc);
    return 0;
  });
}

#define DLAF_UPDATE_DIRECT(letter, DT)                                                                            \
  int dlaf_mi355x_update_direct_##letter(dlaf_mi355x_update_desc* d, void* c, const void* a, const void* b,         \
                                         const void* a2, const void* b2, void* c_again) noexcept {                \
    if (!d || !c || !a || !b)                                                                                      \
      return -3;                                                                                                   \
    return update_direct<DT>(*d, c, a, b, a2, b2, c_again);                                                        \
  }
DLAF_UPDATE_DIRECT(s, float)
DLAF_UPDATE_DIRECT(d, double)
DLAF_UPDATE_DIRECT(c, cfloat)
DLAF_UPDATE_DIRECT(z, cdouble)
#undef DLAF_UPDATE_DIRECT
#define DLAF_TRSM_DIRECT(letter, DT)                                                                              \
  int dlaf_mi355x_trsm_direct_##letter(dlaf_mi355x_trsm_desc* d, void* b, const void* l, void* winv) noexcept {   \
    if (!d || !b || !l || !winv)                                                                                   \
      return -3;                                                                                                   \
    return trsm_direct<DT>(*d, b, l, winv);                                                                        \
  }
DLAF_TRSM_DIRECT(s, float)
DLAF_TRSM_DIRECT(d, double)
DLAF_TRSM_DIRECT(c, cfloat)
DLAF_TRSM_DIRECT(z, cdouble)
#undef DLAF_TRSM_DIRECT
#define DLAF_POTRF_DIRECT(letter, DT)                                                                             \
  int dlaf_mi355x_potrf_direct_##letter(dlaf_mi355x_potrf_desc* d, void* tile, void* winv) noexcept {             \
    if (!d || !tile || !winv)                                                                                      \
      return -3;                                                                                                   \
    return potrf_direct<DT>(*d, tile, winv);                                                                       \
  }
DLAF_POTRF_DIRECT(s, float)
DLAF_POTRF_DIRECT(d, double)
DLAF_POTRF_DIRECT(c, cfloat)
DLAF_POTRF_DIRECT(z, cdouble)
#undef DLAF_POTRF_DIRECT
long dlaf_mi355x_update_bulk_slots(char type) noexcept {
  long slots = 0;
  const int r = dispatch_api_type(type, [&](auto* tag) {
    using DT = std::remove_pointer_t<decltype(tag)>;
    slots = update_bulk_slots<DT>();
    return 0;
  });
  return r == 0 ? slots : -1;
}

int dlaf_mi355x_dist_owner(long gt, int gs, int src) noexcept {
  return Axis{0, 1, gs, 0, src}.owner(gt);
}
long dlaf_mi355x_dist_local_tile(long gt, int gs, int rank, int src) noexcept {
  return Axis{0, 1, gs, rank, src}.local_of(gt);
}
long dlaf_mi355x_dist_next_local_tile(long gt, int gs, int rank, int src) noexcept {
  return Axis{0, 1, gs, rank, src}.next_local(gt);
}
long dlaf_mi355x_dist_global_tile(long lt, int gs, int rank, int src) noexcept {
  return Axis{0, 1, gs, rank, src}.global_of(lt);
}
long dlaf_mi355x_dist_local_size(long n, int nb, int gs, int rank, int src) noexcept {
  return Axis{n, nb, gs, rank, src}.local_size();
}
long dlaf_mi355x_dist_local_tiles(long n, int nb, int gs, int rank, int src) noexcept {
  return Axis{n, nb, gs, rank, src}.local_tiles();
}


}  // extern "C"
