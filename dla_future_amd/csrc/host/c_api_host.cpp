// c_api_host.cpp -- the extern "C" surface, part 2 of 3 (c_api_internal.hpp has the map): the entries that take
// descriptors or ScaLAPACK argument lists over host memory -- triangular solver and multiplication, Hermitian and
// general multiplication, the Hermitian rank updates, the addition / transposition, p?potrs, generalized to standard, the inverses, the norms, reduction to band and the eigensolver
// stages and drivers (include/dlaf_c/eigensolver/*.h as upstream, include/dlaf_mi355x/dlaf_mi355x.h).  Every argument
// is judged (api_checks.hpp) before anything touches the GPU.
#define DLAF_MI355X_NO_MPI 1  // as in c_api.cpp: no <mpi.h> in the core
#include <algorithm>
#include <complex>
#include <cstring>

#include <dlaf_c/eigensolver/eigensolver.h>
#include <dlaf_c/eigensolver/gen_eigensolver.h>
#include <dlaf_mi355x/dlaf_mi355x.h>

#include "../device/tridiag_api.hpp"
#include "c_api_internal.hpp"
#include "device_matrix.hpp"
#include "drivers.hpp"
#include "eigensolver.hpp"
#include "red2band.hpp"
#include "tile_matrix.hpp"

using namespace dlaf_mi355x;

namespace {
// The two routines over a triangular A, B = the m x n matrix they overwrite: dlaf::triangular_solver
// (include/dlaf/solver/triangular.h:41-177) and dlaf::triangular_multiplication
// (include/dlaf/multiplication/triangular.h), B = alpha op(A) B (side L) / alpha B op(A) (side R).  Same arguments,
// same preconditions (triangular.h:43-48, :57 / :93-98: require_triangular); who names the routine in the messages.
template <class HT>
struct TriangularOp {
  using DT = typename DevType<HT>::type;
  const char* who;
  int (*host)(Grid*, char, char, char, char, DT, HostOperand<const DT>, HostOperand<DT>);
};
template <class HT>
constexpr TriangularOp<HT> kTrsm{"triangular solver", &triangular_solver_host<typename DevType<HT>::type>};
template <class HT>
constexpr TriangularOp<HT> kTrmm{"triangular multiplication",
                                 &triangular_multiplication_host<typename DevType<HT>::type>};

// through descriptors
template <class HT>
int triangular_c(const TriangularOp<HT>& op_, int ctx, char side, char uplo, char op, char diag, const HT* alpha,
                 const HT* a, const DLAF_descriptor& da, HT* b, const DLAF_descriptor& db) {
  using DT = typename DevType<HT>::type;
  if (da.i != 0 || da.j != 0 || db.i != 0 || db.j != 0)
    fatal("[dlaf_mi355x] sub-matrices are not supported: offsets must be 0\n");
  Grid& g = grid_from_context(ctx);
  const auto oa = host_operand(a, da);
  const auto ob = host_operand(b, db);
  require_triangular(op_.who, g, side, uplo, op, diag, oa, ob);
  DT al;
  std::memcpy(&al, alpha, sizeof(DT));
  return op_.host(&g, side, uplo, op, diag, al, oa, ob);
}

// ScaLAPACK p?trsm / p?trmm argument list
template <class HT>
void pxtriangular(const TriangularOp<HT>& op_, char side, char uplo, char op, char diag, int m, int n, const HT* alpha,
                  const HT* a, int ia, int ja, const int desca[9], HT* b, int ib, int jb, const int descb[9]) {
  const int ctx = require_scalapack_args({{'A', desca, ia, ja}, {'B', descb, ib, jb}});
  const int na = is_left(side) ? m : n;
  const DLAF_descriptor da = make_dlaf_descriptor(na, na, ia, ja, desca);
  const DLAF_descriptor db = make_dlaf_descriptor(m, n, ib, jb, descb);
  (void) triangular_c<HT>(op_, ctx, side, uplo, op, diag, alpha, a, da, b, db);
}

// dlaf::hermitian_multiplication through descriptors: C = beta C + alpha A B (side L) / beta C + alpha B A (side R)
template <class HT>
int hermitian_multiplication_c(int ctx, char side, char uplo, const HT* alpha, const HT* a, const DLAF_descriptor& da,
                               const HT* b, const DLAF_descriptor& db, const HT* beta, HT* c, const DLAF_descriptor& dc) {
  using DT = typename DevType<HT>::type;
  const char* who = "hermitian multiplication";
  if (da.i != 0 || da.j != 0 || db.i != 0 || db.j != 0 || dc.i != 0 || dc.j != 0)
    fatal("[dlaf_mi355x] %s: sub-matrices are not supported: offsets must be 0\n", who);
  Grid& g = grid_from_context(ctx);
  const auto oa = host_operand(a, da), ob = host_operand(b, db);
  const auto oc = host_operand(c, dc);
  require_hermitian_multiplication(who, g, side, uplo, oa, ob, oc);
  DT al, be;
  std::memcpy(&al, alpha, sizeof(DT));
  std::memcpy(&be, beta, sizeof(DT));
  return hermitian_multiplication_host<DT>(&g, side, uplo, al, oa, ob, be, oc);
}

// ScaLAPACK p?symm / p?hemm argument list
template <class HT>
void pxhemm(char side, char uplo, int m, int n, const HT* alpha, const HT* a, int ia, int ja, const int desca[9],
            const HT* b, int ib, int jb, const int descb[9], const HT* beta, HT* c, int ic, int jc, const int descc[9]) {
  const int ctx = require_scalapack_args({{'A', desca, ia, ja}, {'B', descb, ib, jb}, {'C', descc, ic, jc}},
                                         "hermitian multiplication");
  const int na = is_left(side) ? m : n;
  const DLAF_descriptor da = make_dlaf_descriptor(na, na, ia, ja, desca);
  const DLAF_descriptor db = make_dlaf_descriptor(m, n, ib, jb, descb);
  const DLAF_descriptor dc = make_dlaf_descriptor(m, n, ic, jc, descc);
  (void) hermitian_multiplication_c<HT>(ctx, side, uplo, alpha, a, da, b, db, beta, c, dc);
}

// dlaf::multiplication::internal::generalMatrix (include/dlaf/multiplication/general.h) through descriptors:
// C = beta C + alpha op(A) op(B), a / b / c described as stored; every argument judged before the GPU is touched
template <class HT>
int general_multiplication_c(int ctx, char opa, char opb, const HT* alpha, const HT* a, const DLAF_descriptor& da,
                             const HT* b, const DLAF_descriptor& db, const HT* beta, HT* c, const DLAF_descriptor& dc) {
  using DT = typename DevType<HT>::type;
  const char* who = "general multiplication";
  if (da.i != 0 || da.j != 0 || db.i != 0 || db.j != 0 || dc.i != 0 || dc.j != 0)
    fatal("[dlaf_mi355x] %s: sub-matrices are not supported: offsets must be 0\n", who);
  Grid& g = grid_from_context(ctx);
  const auto oa = host_operand(a, da), ob = host_operand(b, db);
  const auto oc = host_operand(c, dc);
  require_general_multiplication(who, g, opa, opb, oa, ob, oc);
  DT al, be;
  std::memcpy(&al, alpha, sizeof(DT));
  std::memcpy(&be, beta, sizeof(DT));
  return general_multiplication_host<DT>(&g, opa, opb, al, oa, ob, be, oc);
}

// ScaLAPACK p?gemm argument list
template <class HT>
void pxgemm(char transa, char transb, int m, int n, int k, const HT* alpha, const HT* a, int ia, int ja,
            const int desca[9], const HT* b, int ib, int jb, const int descb[9], const HT* beta, HT* c, int ic, int jc,
            const int descc[9]) {
  const int ctx = require_scalapack_args({{'A', desca, ia, ja}, {'B', descb, ib, jb}, {'C', descc, ic, jc}},
                                         "general multiplication");
  const bool an = is_notrans(transa), bn = is_notrans(transb);
  const DLAF_descriptor da = make_dlaf_descriptor(an ? m : k, an ? k : m, ia, ja, desca);
  const DLAF_descriptor db = make_dlaf_descriptor(bn ? k : n, bn ? n : k, ib, jb, descb);
  const DLAF_descriptor dc = make_dlaf_descriptor(m, n, ic, jc, descc);
  (void) general_multiplication_c<HT>(ctx, transa, transb, alpha, a, da, b, db, beta, c, dc);
}

// Hermitian rank-k (b null) / rank-2k update of the uplo triangle of C through descriptors (rank_update.cpp): a, b as
// stored; alpha an element (rank-k: its real alpha with imaginary part 0), beta real; every argument judged before the
// GPU is touched
template <class HT>
using real_of_t = typename TypeInfo<typename DevType<HT>::type>::real;
template <class HT>
typename DevType<HT>::type element_of_real(real_of_t<HT> v) {
  using DT = typename DevType<HT>::type;
  if constexpr (TypeInfo<DT>::is_complex)
    return DT{v, real_of_t<HT>(0)};
  else
    return v;
}
template <class HT>
int rank_update_c(int ctx, char uplo, char trans, typename DevType<HT>::type alpha, const HT* a, const DLAF_descriptor& da,
                  const HT* b, const DLAF_descriptor* db, real_of_t<HT> beta, HT* c, const DLAF_descriptor& dc) {
  using DT = typename DevType<HT>::type;
  const char* who = db ? "hermitian rank-2k update" : "hermitian rank-k update";
  if (da.i != 0 || da.j != 0 || dc.i != 0 || dc.j != 0 || (db && (db->i != 0 || db->j != 0)))
    fatal("[dlaf_mi355x] %s: sub-matrices are not supported: offsets must be 0\n", who);
  Grid& g = grid_from_context(ctx);
  const auto oa = host_operand(a, da), ob = host_operand(b, db ? *db : da);  // (rank-k: ob is never passed on)
  const auto oc = host_operand(c, dc);
  require_rank_update(who, g, TypeInfo<DT>::is_complex, uplo, trans, oa, db ? &ob : nullptr, oc);
  return hermitian_rank_update_host<DT>(&g, uplo, trans, alpha, oa, db ? &ob : nullptr, beta, oc);
}

// The weighted rank-k update  C = alpha A D A^H + beta C  through descriptors: d the k real weights on the host
template <class HT>
int weighted_rank_update_c(int ctx, char uplo, char trans, real_of_t<HT> alpha, const HT* a, const DLAF_descriptor& da,
                           const real_of_t<HT>* d, real_of_t<HT> beta, HT* c, const DLAF_descriptor& dc) {
  using DT = typename DevType<HT>::type;
  if (da.i != 0 || da.j != 0 || dc.i != 0 || dc.j != 0)
    fatal("[dlaf_mi355x] hermitian weighted rank-k update: sub-matrices are not supported: offsets must be 0\n");
  Grid& g = grid_from_context(ctx);
  const auto oa = host_operand(a, da);
  const auto oc = host_operand(c, dc);
  require_weighted_rank_update(g, TypeInfo<DT>::is_complex, uplo, trans, alpha == real_of_t<HT>(0), oa, d, oc);
  return hermitian_rank_update_host<DT>(&g, uplo, trans, element_of_real<HT>(alpha), oa, nullptr, beta, oc, d);
}

// Functions of a Hermitian matrix through a descriptor (matrix_function.cpp): `fn(…, self)` the untyped weights
// callback; selected (null allowed) receives [begin, end)
template <class HT>
int hermitian_function_c(const char* who, int ctx, char uplo, HT* a, const DLAF_descriptor& da, real_of_t<HT>* w,
                         SpectralWeights fn, void* self, const long* index_range, const real_of_t<HT>* value_interval,
                         long* selected) {
  using DT = typename DevType<HT>::type;
  if (da.i != 0 || da.j != 0)
    fatal("[dlaf_mi355x] %s: sub-matrices are not supported: offsets must be 0\n", who);
  Grid& g = grid_from_context(ctx);
  const auto oa = host_operand(a, da);
  require_hermitian_function(who, g, uplo, oa, index_range != nullptr, value_interval != nullptr);
  if (!w)
    fatal("[dlaf_mi355x] %s: the eigenvalue array w is null\n", who);
  SpectralSelection<real_of_t<HT>> sel(da.m, index_range, value_interval);
  if (!sel.by_value)
    check_eigenvalues_index(who, da.m, sel.begin, sel.end);
  const int r = hermitian_function_host<DT>(&g, uplo, oa, w, sel.by_value ? sel.values : nullptr, sel.begin, sel.end, fn,
                                            self);
  if (selected) {
    selected[0] = sel.begin;
    selected[1] = sel.end;
  }
  return r;
}
template <class HT>
int hermitian_power_c(int ctx, char uplo, HT* a, const DLAF_descriptor& da, real_of_t<HT>* w, double exponent,
                      double threshold, long* n_dropped) {
  using R = real_of_t<HT>;
  require_power_threshold("hermitian power", threshold);
  const R interval[2] = {(R) threshold, std::numeric_limits<R>::infinity()};
  SpectralPower<R> p{exponent};
  long sel[2] = {0, 0};
  const int r = hermitian_function_c<HT>("hermitian power", ctx, uplo, a, da, w, &SpectralPower<R>::call, &p, nullptr,
                                         interval, sel);
  if (n_dropped)
    *n_dropped = sel[0];
  return r;
}

// ScaLAPACK p?syrk / p?herk (b null) and p?syr2k / p?her2k argument lists
template <class HT>
void pxrank_update(char uplo, char trans, int n, int k, typename DevType<HT>::type alpha, const HT* a, int ia, int ja,
                   const int desca[9], const HT* b, int ib, int jb, const int* descb, real_of_t<HT> beta, HT* c, int ic,
                   int jc, const int descc[9]) {
  const bool tn = is_notrans(trans);
  const int ctx = descb ? require_scalapack_args({{'A', desca, ia, ja}, {'B', descb, ib, jb}, {'C', descc, ic, jc}},
                                                 "hermitian rank-2k update")
                        : require_scalapack_args({{'A', desca, ia, ja}, {'C', descc, ic, jc}}, "hermitian rank-k update");
  const DLAF_descriptor da = make_dlaf_descriptor(tn ? n : k, tn ? k : n, ia, ja, desca);
  const DLAF_descriptor dc = make_dlaf_descriptor(n, n, ic, jc, descc);
  DLAF_descriptor db{};
  if (descb)
    db = make_dlaf_descriptor(tn ? n : k, tn ? k : n, ib, jb, descb);
  (void) rank_update_c<HT>(ctx, uplo, trans, alpha, a, da, b, descb ? &db : nullptr, beta, c, dc);
}

// general_addition / hermitian_complete through descriptors (addition.cpp): a, c as stored; every argument judged before
// the GPU is touched
template <class HT>
int general_addition_c(int ctx, char uplo, char op, const HT* alpha, const HT* a, const DLAF_descriptor& da, const HT* beta,
                       HT* c, const DLAF_descriptor& dc) {
  using DT = typename DevType<HT>::type;
  const char* who = "general addition";
  if (da.i != 0 || da.j != 0 || dc.i != 0 || dc.j != 0)
    fatal("[dlaf_mi355x] %s: sub-matrices are not supported: offsets must be 0\n", who);
  Grid& g = grid_from_context(ctx);
  const auto oa = host_operand(a, da);
  const auto oc = host_operand(c, dc);
  require_general_addition(who, g, uplo, op, oa, oc, a == c);
  DT al, be;
  std::memcpy(&al, alpha, sizeof(DT));
  std::memcpy(&be, beta, sizeof(DT));
  return general_addition_host<DT>(&g, uplo, op, al, oa, be, oc);
}
template <class HT>
int hermitian_complete_c(int ctx, char uplo, char kind, HT* a, const DLAF_descriptor& da) {
  using DT = typename DevType<HT>::type;
  const char* who = "hermitian complete";
  if (da.i != 0 || da.j != 0)
    fatal("[dlaf_mi355x] %s: sub-matrices are not supported: offsets must be 0\n", who);
  Grid& g = grid_from_context(ctx);
  const auto oa = host_operand(a, da);
  require_hermitian_complete(who, g, uplo, kind, oa);
  return hermitian_complete_host<DT>(&g, uplo, kind, oa);
}

// PBLAS p?geadd / p?tradd / p?tran* and ScaLAPACK p?lacpy argument lists: C (m x n) = beta C + alpha op(A)
template <class HT>
void pxgeadd(char uplo, char trans, int m, int n, const HT* alpha, const HT* a, int ia, int ja, const int desca[9],
             const HT* beta, HT* c, int ic, int jc, const int descc[9]) {
  const int ctx = require_scalapack_args({{'A', desca, ia, ja}, {'C', descc, ic, jc}}, "general addition");
  const bool tn = is_notrans(trans);
  const DLAF_descriptor da = make_dlaf_descriptor(tn ? m : n, tn ? n : m, ia, ja, desca);
  const DLAF_descriptor dc = make_dlaf_descriptor(m, n, ic, jc, descc);
  (void) general_addition_c<HT>(ctx, uplo, trans, alpha, a, da, beta, c, dc);
}
template <class HT>
void pxlacpy(char uplo, int m, int n, const HT* a, int ia, int ja, const int desca[9], HT* b, int ib, int jb,
             const int descb[9]) {
  const HT one(1), zero(0);
  pxgeadd<HT>(is_uplo(uplo) ? uplo : 'A', 'N', m, n, &one, a, ia, ja, desca, &zero, b, ib, jb, descb);
}

// ScaLAPACK p?potrs: solve A X = B with the factor p?potrf left in a (uplo L: L L^H, uplo U: U^H U)
template <class HT>
void pxpotrs(char uplo, int n, int nrhs, const HT* a, int ia, int ja, const int desca[9], HT* b, int ib, int jb,
             const int descb[9], int* info) {
  const HT one(1);
  const bool lower = is_lower(uplo);
  pxtriangular<HT>(kTrsm<HT>, 'L', uplo, lower ? 'N' : 'C', 'N', n, nrhs, &one, a, ia, ja, desca, b, ib, jb, descb);
  pxtriangular<HT>(kTrsm<HT>, 'L', uplo, lower ? 'C' : 'N', 'N', n, nrhs, &one, a, ia, ja, desca, b, ib, jb, descb);
  if (info)
    *info = 0;
}

// dlaf::eigensolver::internal::generalized_to_standard (include/dlaf/eigensolver/gen_to_std.h:50,:101) through
// descriptors: preconditions of gen_to_std.h:52-60 / :103-113 (square, square blocks, same size and blocks)
template <class HT>
int gen_to_std_c(int ctx, char uplo, HT* a, const DLAF_descriptor& da, const HT* b, const DLAF_descriptor& db) {
  using DT = typename DevType<HT>::type;
  require_square_desc(da);
  require_square_desc(db);
  require_uplo(uplo);
  if (da.m != db.m || da.nb != db.nb || da.isrc != db.isrc || da.jsrc != db.jsrc)
    fatal("[dlaf_mi355x] gen_to_std: A (%d, block %d, source %d,%d) and B (%d, block %d, source %d,%d) must be "
          "distributed alike\n", da.m, da.nb, da.isrc, da.jsrc, db.m, db.nb, db.isrc, db.jsrc);
  Grid& g = grid_from_context(ctx);
  require_sources(nullptr, g, {&da});
  return gen_to_std_host<DT>(&g, uplo, host_operand(a, da), host_operand(b, db));
}

// ScaLAPACK p?sygst / p?hegst argument list (ibtype 1 only: inv(L) A inv(L^H) / inv(U^H) A inv(U))
template <class HT, class RT>
void pxhegst(int ibtype, char uplo, int n, HT* a, int ia, int ja, const int desca[9], const HT* b, int ib, int jb,
             const int descb[9], RT* scale, int* info) {
  if (ibtype != 1)
    fatal("[dlaf_mi355x] p?hegst: only ibtype = 1 is built (got %d)\n", ibtype);
  const int ctx = require_scalapack_args({{'A', desca, ia, ja}, {'B', descb, ib, jb}});
  const int r = gen_to_std_c<HT>(ctx, uplo, a, make_dlaf_descriptor(n, n, ia, ja, desca), b,
                                 make_dlaf_descriptor(n, n, ib, jb, descb));
  if (scale)
    *scale = RT(1);
  if (info)
    *info = r;
}

// dlaf::triangular_inverse / dlaf::inverse_from_cholesky_factor through descriptors (inverse.cpp)
template <class HT>
int inverse_c(int ctx, char uplo, char diag, bool product, HT* a, const DLAF_descriptor& da) {
  using DT = typename DevType<HT>::type;
  require_square_desc(da);
  require_uplo(uplo);
  Grid& g = grid_from_context(ctx);
  require_sources(nullptr, g, {&da});
  if (product)
    return inverse_from_cholesky_factor_host<DT>(&g, uplo, host_operand(a, da));
  return triangular_inverse_host<DT>(&g, uplo, diag, host_operand(a, da));
}

// ScaLAPACK p?trtri / p?potri argument lists
template <class HT>
void pxinverse(char uplo, char diag, bool product, int n, HT* a, int ia, int ja, const int desca[9], int* info) {
  const int ctx = require_scalapack_args({{'A', desca, ia, ja}});
  const int r = inverse_c<HT>(ctx, uplo, diag, product, a, make_dlaf_descriptor(n, n, ia, ja, desca));
  if (info)
    *info = r;
}

// dlaf::auxiliary norms through descriptors (norm.cpp): structure 'G' general, 'H' Hermitian / symmetric, 'T' triangular.
// Every argument is judged before anything touches the GPU; the codes are the header's.
template <class HT>
int norm_c(int ctx, char norm, char structure, char uplo, char diag, const HT* a, const DLAF_descriptor& da,
           double* value) {
  using DT = typename DevType<HT>::type;
  if (!value)
    return -6;
  if (norm_kind(norm) == 0)
    return -1;
  if (structure != 'G' && !is_uplo(uplo))
    return -2;
  if (structure == 'T' && !is_diag(diag))
    return -3;
  if (da.i != 0 || da.j != 0 || da.mb != da.nb || da.nb < 1 || da.m < 0 || da.n < 0 ||
      (structure != 'G' && da.m != da.n))
    return -4;
  Grid* g = find_grid(ctx);
  if (!g)
    return -6;
  if (!source_in_grid(*g, da))
    return -5;
  if (da.m == 0 || da.n == 0) {
    *value = 0.0;
    return 0;
  }
  *value = structure == 'G' ? general_norm_host<DT>(g, norm, host_operand(a, da))
                            : structured_norm_host<DT>(g, norm, structure, uplo, diag, host_operand(a, da));
  return 0;
}

// ScaLAPACK p?lange / p?lansy / p?lanhe / p?lantr argument lists (without work); the value is returned
template <class HT>
double pxnorm(char norm, char structure, char uplo, char diag, int m, int n, const HT* a, int ia, int ja,
              const int desca[9]) {
  const int ctx = require_scalapack_args({{'A', desca, ia, ja}});
  double v = 0.0;
  const int r = norm_c<HT>(ctx, norm, structure, uplo, diag, a, make_dlaf_descriptor(m, n, ia, ja, desca), &v);
  if (r != 0)
    fatal("[dlaf_mi355x] p?lan*: bad argument (code %d; norm '%c', uplo '%c', diag '%c')\n", r, norm, uplo, diag);
  return v;
}

// dlaf::eigensolver::internal::reduction_to_band (include/dlaf/eigensolver/reduction_to_band.h:101-122) through the
// reference's descriptor conventions
template <class HT>
int red2band_c(int ctx, HT* a, const DLAF_descriptor& da, int band, HT* taus) {
  using DT = typename DevType<HT>::type;
  require_square_desc(da);
  Grid& g = grid_from_context(ctx);
  require_sources(nullptr, g, {&da});
  require_band("reduction_to_band", band, da.nb);
  return reduction_to_band_host<DT>(&g, host_operand(a, da), band, reinterpret_cast<DT*>(taus));
}

template <class HT>
int bt_red2band_c(int ctx, int band, HT* c, const DLAF_descriptor& dc, const HT* v, const DLAF_descriptor& dv,
                  const HT* taus) {
  using DT = typename DevType<HT>::type;
  require_square_desc(dv);
  Grid& g = grid_from_context(ctx);
  if (dc.i != 0 || dc.j != 0 || dc.mb != dc.nb || dc.nb != dv.nb || dc.m != dv.m || dc.isrc != dv.isrc)
    fatal("[dlaf_mi355x] bt_reduction_to_band: C (%d x %d, block %d x %d, row source %d) must have V's block size %d, "
          "row count %d and row source %d, and no offsets\n", dc.m, dc.n, dc.mb, dc.nb, dc.isrc, dv.nb, dv.m, dv.isrc);
  require_sources(nullptr, g, {&dc, &dv});  // (C's row source is V's by now)
  require_band("bt_reduction_to_band", band, dv.nb);
  return bt_reduction_to_band_host<DT>(&g, band, host_operand(c, dc), host_operand(v, dv),
                                       reinterpret_cast<const DT*>(taus));
}

// ---- the eigensolver stages and drivers ------------------------------------------------------
template <class HT>
int band_to_tridiag_c(int ctx, const HT* a, const DLAF_descriptor& da, int band, typename RealOf<HT>::type* d,
                      typename RealOf<HT>::type* e, HT* v, int ldv) {
  using DT = typename DevType<HT>::type;
  require_square_desc(da);
  Grid& g = grid_from_context(ctx);
  require_sources(nullptr, g, {&da});
  require_band("band_to_tridiagonal", band, da.nb);
  if (ldv < std::max(1, da.m))
    fatal("[dlaf_mi355x] band_to_tridiagonal: ldv = %d < n = %d\n", ldv, da.m);
  return band_to_tridiag_host<DT>(&g, host_operand(a, da), band, d, e, reinterpret_cast<DT*>(v), ldv);
}

// Eigensolver entry (src/c_api/eigensolver/eigensolver.h:33-75): descriptors of A and of the eigenvector matrix;
// [begin, end): the 0-based range of eigenvalue indices whose eigenvectors are wanted ([0, n): the full entries)
template <class HT>
int eigensolver_c(int ctx, char uplo, HT* a, const DLAF_descriptor& da, typename RealOf<HT>::type* w, HT* z,
                  const DLAF_descriptor& dz, long begin, long end) {
  using DT = typename DevType<HT>::type;
  check_eigenvalues_index("eigensolver", da.m, begin, end);
  require_square_desc(da);
  Grid& g = grid_from_context(ctx);
  require_like("eigensolver", da, {&dz});
  require_sources(nullptr, g, {&da, &dz});
  return hermitian_eigensolver_host<DT>(&g, uplo, host_operand(a, da), w, host_operand(z, dz), begin, end);
}

template <class HT>
int gen_eigensolver_c(int ctx, char uplo, HT* a, const DLAF_descriptor& da, HT* b, const DLAF_descriptor& db,
                      typename RealOf<HT>::type* w, HT* z, const DLAF_descriptor& dz, bool factorized, long begin,
                      long end) {
  using DT = typename DevType<HT>::type;
  check_eigenvalues_index("gen_eigensolver", da.m, begin, end);
  require_square_desc(da);
  require_square_desc(db);
  Grid& g = grid_from_context(ctx);
  require_like("gen_eigensolver", da, {&db, &dz});
  require_sources(nullptr, g, {&da, &db, &dz});
  return hermitian_gen_eigensolver_host<DT>(&g, uplo, host_operand(a, da), host_operand(b, db), w, host_operand(z, dz),
                                            factorized, begin, end);
}

// p?syevd / p?heevd and p?sygvd / p?hegvd argument lists (src/c_api/eigensolver/eigensolver.h:79-124), descb == nullptr
// for the standard problem; il, iu: the 1-based inclusive eigenvalue index range of p?syevx (1, n: the full entries;
// 1, 0: the empty range)
template <class HT>
void pxhegvd(char uplo, int n, HT* a, int ia, int ja, const int desca[9], HT* b, int ib, int jb, const int descb[9],
             typename RealOf<HT>::type* w, HT* z, int iz, int jz, const int descz[9], long il, long iu, int* info,
             bool factorized) {
  const int ctx = descb ? require_scalapack_args({{'A', desca, ia, ja}, {'B', descb, ib, jb}, {'Z', descz, iz, jz}})
                        : require_scalapack_args({{'A', desca, ia, ja}, {'Z', descz, iz, jz}});
  const DLAF_descriptor da = make_dlaf_descriptor(n, n, ia, ja, desca), dz = make_dlaf_descriptor(n, n, iz, jz, descz);
  const int r = descb ? gen_eigensolver_c<HT>(ctx, uplo, a, da, b, make_dlaf_descriptor(n, n, ib, jb, descb), w, z, dz,
                                              factorized, il - 1, iu)
                      : eigensolver_c<HT>(ctx, uplo, a, da, w, z, dz, il - 1, iu);
  if (info)
    *info = r;
}

// ---- eigenvalues only, and the eigenvalue range given by value ----------------------------
template <class HT>
int eigenvalues_c(int ctx, char uplo, const HT* a, const DLAF_descriptor& da, typename RealOf<HT>::type* w, long begin,
                  long end) {
  using DT = typename DevType<HT>::type;
  check_eigenvalues_index("eigenvalues", da.m, begin, end);
  require_square_desc(da);
  Grid& g = grid_from_context(ctx);
  require_sources(nullptr, g, {&da});
  return hermitian_eigenvalues_host<DT>(&g, uplo, host_operand(a, da), w, begin, end);
}

template <class HT>
int gen_eigenvalues_c(int ctx, char uplo, const HT* a, const DLAF_descriptor& da, HT* b, const DLAF_descriptor& db,
                      typename RealOf<HT>::type* w, bool factorized, long begin, long end) {
  using DT = typename DevType<HT>::type;
  check_eigenvalues_index("gen_eigenvalues", da.m, begin, end);
  require_square_desc(da);
  require_square_desc(db);
  Grid& g = grid_from_context(ctx);
  require_like("gen_eigenvalues", da, {&db});
  require_sources(nullptr, g, {&da, &db});
  return hermitian_gen_eigenvalues_host<DT>(&g, uplo, host_operand(a, da), host_operand(b, db), w, factorized, begin,
                                            end);
}

template <class HT>
int eigensolver_by_value_c(int ctx, char uplo, HT* a, const DLAF_descriptor& da, typename RealOf<HT>::type* w, HT* z,
                           const DLAF_descriptor& dz, typename RealOf<HT>::type vl, typename RealOf<HT>::type vu,
                           long* begin, long* end) {
  using DT = typename DevType<HT>::type;
  if (!begin || !end)
    fatal("[dlaf_mi355x] eigensolver: the by-value entries return their index range: begin, end must not be null\n");
  require_square_desc(da);
  Grid& g = grid_from_context(ctx);
  require_like("eigensolver", da, {&dz});
  require_sources(nullptr, g, {&da, &dz});
  return hermitian_eigensolver_by_value_host<DT>(&g, uplo, host_operand(a, da), w, host_operand(z, dz), vl, vu, begin,
                                                 end);
}

template <class HT>
int gen_eigensolver_by_value_c(int ctx, char uplo, HT* a, const DLAF_descriptor& da, HT* b, const DLAF_descriptor& db,
                               typename RealOf<HT>::type* w, HT* z, const DLAF_descriptor& dz, bool factorized,
                               typename RealOf<HT>::type vl, typename RealOf<HT>::type vu, long* begin, long* end) {
  using DT = typename DevType<HT>::type;
  if (!begin || !end)
    fatal("[dlaf_mi355x] gen_eigensolver: the by-value entries return their index range: begin, end must not be null\n");
  require_square_desc(da);
  require_square_desc(db);
  Grid& g = grid_from_context(ctx);
  require_like("gen_eigensolver", da, {&db, &dz});
  require_sources(nullptr, g, {&da, &db, &dz});
  return hermitian_gen_eigensolver_by_value_host<DT>(&g, uplo, host_operand(a, da), host_operand(b, db), w,
                                                     host_operand(z, dz), factorized, vl, vu, begin, end);
}

// the ScaLAPACK-like argument lists: descb == nullptr for the standard problem
template <class HT>
void pxhegvd_eigenvalues(char uplo, int n, const HT* a, int ia, int ja, const int desca[9], HT* b, int ib, int jb,
                         const int descb[9], typename RealOf<HT>::type* w, long il, long iu, int* info, bool factorized) {
  const int ctx = descb ? require_scalapack_args({{'A', desca, ia, ja}, {'B', descb, ib, jb}})
                        : require_scalapack_args({{'A', desca, ia, ja}});
  const DLAF_descriptor da = make_dlaf_descriptor(n, n, ia, ja, desca);
  const int r = descb ? gen_eigenvalues_c<HT>(ctx, uplo, a, da, b, make_dlaf_descriptor(n, n, ib, jb, descb), w,
                                              factorized, il - 1, iu)
                      : eigenvalues_c<HT>(ctx, uplo, a, da, w, il - 1, iu);
  if (info)
    *info = r;
}
template <class HT>
void pxhegvd_by_value(char uplo, int n, HT* a, int ia, int ja, const int desca[9], HT* b, int ib, int jb,
                      const int descb[9], typename RealOf<HT>::type* w, HT* z, int iz, int jz, const int descz[9],
                      typename RealOf<HT>::type vl, typename RealOf<HT>::type vu, int* m, int* info, bool factorized) {
  long begin = 0, end = 0;
  const int ctx = descb ? require_scalapack_args({{'A', desca, ia, ja}, {'B', descb, ib, jb}, {'Z', descz, iz, jz}})
                        : require_scalapack_args({{'A', desca, ia, ja}, {'Z', descz, iz, jz}});
  const DLAF_descriptor da = make_dlaf_descriptor(n, n, ia, ja, desca), dz = make_dlaf_descriptor(n, n, iz, jz, descz);
  const int r = descb ? gen_eigensolver_by_value_c<HT>(ctx, uplo, a, da, b, make_dlaf_descriptor(n, n, ib, jb, descb), w,
                                                       z, dz, factorized, vl, vu, &begin, &end)
                      : eigensolver_by_value_c<HT>(ctx, uplo, a, da, w, z, dz, vl, vu, &begin, &end);
  if (m)
    *m = (int) (end - begin);
  if (info)
    *info = r;
}
}  // namespace

// ===================================================================================================== entries
extern "C" {

// NAME / PNAME / OP: triangular_solver / trsm / kTrsm, triangular_multiplication / trmm / kTrmm
#define DLAF_MI355X_TRIANGULAR_ENTRY(S, HT, CT, NAME, PNAME, OP)                                                 \
  int dlaf_mi355x_##NAME##_##S(int ctx, char side, char uplo, char op, char diag, const CT* alpha, const CT* a,   \
                               DLAF_descriptor desca, CT* b, DLAF_descriptor descb) noexcept {                   \
    return triangular_c<HT>(OP<HT>, ctx, side, uplo, op, diag, reinterpret_cast<const HT*>(alpha),               \
                            reinterpret_cast<const HT*>(a), desca, reinterpret_cast<HT*>(b), descb);             \
  }                                                                                                             \
  void dlaf_mi355x_p##S##PNAME(char side, char uplo, char op, char diag, int m, int n, const CT* alpha, const CT* a, \
                               int ia, int ja, const int desca[9], CT* b, int ib, int jb,                        \
                               const int descb[9]) noexcept {                                                   \
    pxtriangular<HT>(OP<HT>, side, uplo, op, diag, m, n, reinterpret_cast<const HT*>(alpha),                     \
                     reinterpret_cast<const HT*>(a), ia, ja, desca, reinterpret_cast<HT*>(b), ib, jb, descb);    \
  }
#define DLAF_MI355X_TRIANGULAR_ENTRIES(NAME, PNAME, OP)                                  \
  DLAF_MI355X_TRIANGULAR_ENTRY(s, float, float, NAME, PNAME, OP)                         \
  DLAF_MI355X_TRIANGULAR_ENTRY(d, double, double, NAME, PNAME, OP)                       \
  DLAF_MI355X_TRIANGULAR_ENTRY(c, std::complex<float>, dlaf_complex_c, NAME, PNAME, OP)  \
  DLAF_MI355X_TRIANGULAR_ENTRY(z, std::complex<double>, dlaf_complex_z, NAME, PNAME, OP)
DLAF_MI355X_TRIANGULAR_ENTRIES(triangular_multiplication, trmm, kTrmm)
DLAF_MI355X_TRIANGULAR_ENTRIES(triangular_solver, trsm, kTrsm)
#undef DLAF_MI355X_TRIANGULAR_ENTRIES
#undef DLAF_MI355X_TRIANGULAR_ENTRY
#define DLAF_MI355X_HEMM_ENTRY(S, HT, CT, NAME)                                                                  \
  int dlaf_mi355x_hermitian_multiplication_##S(int ctx, char side, char uplo, const CT* alpha, const CT* a,         \
                                               DLAF_descriptor desca, const CT* b, DLAF_descriptor descb,          \
                                               const CT* beta, CT* c, DLAF_descriptor descc) noexcept {            \
    return hermitian_multiplication_c<HT>(ctx, side, uplo, reinterpret_cast<const HT*>(alpha),                     \
                                          reinterpret_cast<const HT*>(a), desca, reinterpret_cast<const HT*>(b),   \
                                          descb, reinterpret_cast<const HT*>(beta), reinterpret_cast<HT*>(c), descc); \
  }                                                                                                             \
  void dlaf_mi355x_p##S##NAME(char side, char uplo, int m, int n, const CT* alpha, const CT* a, int ia, int ja,     \
                              const int desca[9], const CT* b, int ib, int jb, const int descb[9], const CT* beta,  \
                              CT* c, int ic, int jc, const int descc[9]) noexcept {                               \
    pxhemm<HT>(side, uplo, m, n, reinterpret_cast<const HT*>(alpha), reinterpret_cast<const HT*>(a), ia, ja, desca, \
               reinterpret_cast<const HT*>(b), ib, jb, descb, reinterpret_cast<const HT*>(beta),                   \
               reinterpret_cast<HT*>(c), ic, jc, descc);                                                          \
  }
DLAF_MI355X_HEMM_ENTRY(s, float, float, symm)
DLAF_MI355X_HEMM_ENTRY(d, double, double, symm)
DLAF_MI355X_HEMM_ENTRY(c, std::complex<float>, dlaf_complex_c, hemm)
DLAF_MI355X_HEMM_ENTRY(z, std::complex<double>, dlaf_complex_z, hemm)
#undef DLAF_MI355X_HEMM_ENTRY
#define DLAF_MI355X_GEMM_ENTRY(S, HT, CT)                                                                         \
  int dlaf_mi355x_general_multiplication_##S(int ctx, char opa, char opb, const CT* alpha, const CT* a,             \
                                             DLAF_descriptor desca, const CT* b, DLAF_descriptor descb,            \
                                             const CT* beta, CT* c, DLAF_descriptor descc) noexcept {              \
    return general_multiplication_c<HT>(ctx, opa, opb, reinterpret_cast<const HT*>(alpha),                          \
                                        reinterpret_cast<const HT*>(a), desca, reinterpret_cast<const HT*>(b),     \
                                        descb, reinterpret_cast<const HT*>(beta), reinterpret_cast<HT*>(c), descc); \
  }                                                                                                             \
  void dlaf_mi355x_p##S##gemm(char transa, char transb, int m, int n, int k, const CT* alpha, const CT* a, int ia,  \
                              int ja, const int desca[9], const CT* b, int ib, int jb, const int descb[9],          \
                              const CT* beta, CT* c, int ic, int jc, const int descc[9]) noexcept {               \
    pxgemm<HT>(transa, transb, m, n, k, reinterpret_cast<const HT*>(alpha), reinterpret_cast<const HT*>(a), ia, ja, \
               desca, reinterpret_cast<const HT*>(b), ib, jb, descb, reinterpret_cast<const HT*>(beta),            \
               reinterpret_cast<HT*>(c), ic, jc, descc);                                                          \
  }
DLAF_MI355X_GEMM_ENTRY(s, float, float)
DLAF_MI355X_GEMM_ENTRY(d, double, double)
DLAF_MI355X_GEMM_ENTRY(c, std::complex<float>, dlaf_complex_c)
DLAF_MI355X_GEMM_ENTRY(z, std::complex<double>, dlaf_complex_z)
#undef DLAF_MI355X_GEMM_ENTRY
// RT: the real type of alpha (rank-k) and beta; NAME / NAME2: syrk / syr2k or herk / her2k
#define DLAF_MI355X_RANK_UPDATE_ENTRY(S, HT, CT, RT, NAME, NAME2)                                                   \
  int dlaf_mi355x_hermitian_rank_k_update_##S(int ctx, char uplo, char trans, const RT* alpha, const CT* a,           \
                                              DLAF_descriptor desca, const RT* beta, CT* c,                          \
                                              DLAF_descriptor descc) noexcept {                                      \
    return rank_update_c<HT>(ctx, uplo, trans, element_of_real<HT>(*alpha), reinterpret_cast<const HT*>(a), desca,   \
                             nullptr, nullptr, *beta, reinterpret_cast<HT*>(c), descc);                              \
  }                                                                                                                 \
  int dlaf_mi355x_hermitian_rank_2k_update_##S(int ctx, char uplo, char trans, const CT* alpha, const CT* a,          \
                                               DLAF_descriptor desca, const CT* b, DLAF_descriptor descb,            \
                                               const RT* beta, CT* c, DLAF_descriptor descc) noexcept {              \
    DevType<HT>::type al;                                                                                           \
    std::memcpy(&al, alpha, sizeof(al));                                                                            \
    return rank_update_c<HT>(ctx, uplo, trans, al, reinterpret_cast<const HT*>(a), desca,                            \
                             reinterpret_cast<const HT*>(b), &descb, *beta, reinterpret_cast<HT*>(c), descc);        \
  }                                                                                                                 \
  void dlaf_mi355x_p##S##NAME(char uplo, char trans, int n, int k, const RT* alpha, const CT* a, int ia, int ja,      \
                              const int desca[9], const RT* beta, CT* c, int ic, int jc,                             \
                              const int descc[9]) noexcept {                                                         \
    pxrank_update<HT>(uplo, trans, n, k, element_of_real<HT>(*alpha), reinterpret_cast<const HT*>(a), ia, ja, desca, \
                      nullptr, 1, 1, nullptr, *beta, reinterpret_cast<HT*>(c), ic, jc, descc);                       \
  }                                                                                                                 \
  void dlaf_mi355x_p##S##NAME2(char uplo, char trans, int n, int k, const CT* alpha, const CT* a, int ia, int ja,     \
                               const int desca[9], const CT* b, int ib, int jb, const int descb[9], const RT* beta,  \
                               CT* c, int ic, int jc, const int descc[9]) noexcept {                                 \
    DevType<HT>::type al;                                                                                           \
    std::memcpy(&al, alpha, sizeof(al));                                                                            \
    pxrank_update<HT>(uplo, trans, n, k, al, reinterpret_cast<const HT*>(a), ia, ja, desca,                          \
                      reinterpret_cast<const HT*>(b), ib, jb, descb, *beta, reinterpret_cast<HT*>(c), ic, jc, descc); \
  }
DLAF_MI355X_RANK_UPDATE_ENTRY(s, float, float, float, syrk, syr2k)
DLAF_MI355X_RANK_UPDATE_ENTRY(d, double, double, double, syrk, syr2k)
DLAF_MI355X_RANK_UPDATE_ENTRY(c, std::complex<float>, dlaf_complex_c, float, herk, her2k)
DLAF_MI355X_RANK_UPDATE_ENTRY(z, std::complex<double>, dlaf_complex_z, double, herk, her2k)
#undef DLAF_MI355X_RANK_UPDATE_ENTRY
// RS: the letter of the real type (its weights callback)
#define DLAF_MI355X_WEIGHTED_ENTRY(S, HT, CT, RT, RS)                                                                \
  int dlaf_mi355x_hermitian_weighted_rank_k_update_##S(int ctx, char uplo, char trans, const RT* alpha, const CT* a,   \
                                                       DLAF_descriptor desca, const RT* d, const RT* beta, CT* c,     \
                                                       DLAF_descriptor descc) noexcept {                              \
    return weighted_rank_update_c<HT>(ctx, uplo, trans, *alpha, reinterpret_cast<const HT*>(a), desca, d, *beta,      \
                                      reinterpret_cast<HT*>(c), descc);                                              \
  }                                                                                                                 \
  int dlaf_mi355x_hermitian_function_##S(int ctx, char uplo, CT* a, DLAF_descriptor desca, RT* w,                      \
                                         dlaf_mi355x_spectral_weights_##RS weights, void* user,                       \
                                         const long* index_range, const RT* value_interval,                          \
                                         long* selected) noexcept {                                                   \
    if (!weights)                                                                                                   \
      fatal("[dlaf_mi355x] hermitian function: the weights callback is null\n");                                     \
    SpectralWeightsCall<RT> call{weights, user};                                                                    \
    return hermitian_function_c<HT>("hermitian function", ctx, uplo, reinterpret_cast<HT*>(a), desca, w,              \
                                    &SpectralWeightsCall<RT>::call, &call, index_range, value_interval, selected);   \
  }                                                                                                                 \
  int dlaf_mi355x_hermitian_power_##S(int ctx, char uplo, CT* a, DLAF_descriptor desca, RT* w, double exponent,        \
                                      double threshold, long* n_dropped) noexcept {                                   \
    return hermitian_power_c<HT>(ctx, uplo, reinterpret_cast<HT*>(a), desca, w, exponent, threshold, n_dropped);      \
  }
DLAF_MI355X_WEIGHTED_ENTRY(s, float, float, float, s)
DLAF_MI355X_WEIGHTED_ENTRY(d, double, double, double, d)
DLAF_MI355X_WEIGHTED_ENTRY(c, std::complex<float>, dlaf_complex_c, float, s)
DLAF_MI355X_WEIGHTED_ENTRY(z, std::complex<double>, dlaf_complex_z, double, d)
#undef DLAF_MI355X_WEIGHTED_ENTRY
#define DLAF_MI355X_GEADD_ENTRY(S, HT, CT)                                                                            \
  int dlaf_mi355x_general_addition_##S(int ctx, char uplo, char op, const CT* alpha, const CT* a, DLAF_descriptor desca, \
                                       const CT* beta, CT* c, DLAF_descriptor descc) noexcept {                      \
    return general_addition_c<HT>(ctx, uplo, op, reinterpret_cast<const HT*>(alpha), reinterpret_cast<const HT*>(a),  \
                                  desca, reinterpret_cast<const HT*>(beta), reinterpret_cast<HT*>(c), descc);         \
  }                                                                                                                 \
  int dlaf_mi355x_hermitian_complete_##S(int ctx, char uplo, char kind, CT* a, DLAF_descriptor desca) noexcept {       \
    return hermitian_complete_c<HT>(ctx, uplo, kind, reinterpret_cast<HT*>(a), desca);                               \
  }                                                                                                                 \
  void dlaf_mi355x_p##S##geadd(char trans, int m, int n, const CT* alpha, const CT* a, int ia, int ja,                 \
                               const int desca[9], const CT* beta, CT* c, int ic, int jc,                            \
                               const int descc[9]) noexcept {                                                        \
    pxgeadd<HT>('A', trans, m, n, reinterpret_cast<const HT*>(alpha), reinterpret_cast<const HT*>(a), ia, ja, desca,  \
                reinterpret_cast<const HT*>(beta), reinterpret_cast<HT*>(c), ic, jc, descc);                          \
  }                                                                                                                 \
  void dlaf_mi355x_p##S##tradd(char uplo, char trans, int m, int n, const CT* alpha, const CT* a, int ia, int ja,      \
                               const int desca[9], const CT* beta, CT* c, int ic, int jc,                            \
                               const int descc[9]) noexcept {                                                        \
    if (!is_uplo(uplo))                                                                                             \
      fatal("[dlaf_mi355x] general addition: p?tradd: uplo must be 'L' or 'U', got '%c'\n", uplo);                   \
    pxgeadd<HT>(uplo, trans, m, n, reinterpret_cast<const HT*>(alpha), reinterpret_cast<const HT*>(a), ia, ja, desca, \
                reinterpret_cast<const HT*>(beta), reinterpret_cast<HT*>(c), ic, jc, descc);                          \
  }                                                                                                                 \
  void dlaf_mi355x_p##S##lacpy(char uplo, int m, int n, const CT* a, int ia, int ja, const int desca[9], CT* b,        \
                               int ib, int jb, const int descb[9]) noexcept {                                        \
    pxlacpy<HT>(uplo, m, n, reinterpret_cast<const HT*>(a), ia, ja, desca, reinterpret_cast<HT*>(b), ib, jb, descb);  \
  }
DLAF_MI355X_GEADD_ENTRY(s, float, float)
DLAF_MI355X_GEADD_ENTRY(d, double, double)
DLAF_MI355X_GEADD_ENTRY(c, std::complex<float>, dlaf_complex_c)
DLAF_MI355X_GEADD_ENTRY(z, std::complex<double>, dlaf_complex_z)
#undef DLAF_MI355X_GEADD_ENTRY
#define DLAF_MI355X_TRAN_ENTRY(S, NAME, OP, HT, CT)                                                                   \
  void dlaf_mi355x_p##S##NAME(int m, int n, const CT* alpha, const CT* a, int ia, int ja, const int desca[9],          \
                              const CT* beta, CT* c, int ic, int jc, const int descc[9]) noexcept {                  \
    pxgeadd<HT>('A', OP, m, n, reinterpret_cast<const HT*>(alpha), reinterpret_cast<const HT*>(a), ia, ja, desca,     \
                reinterpret_cast<const HT*>(beta), reinterpret_cast<HT*>(c), ic, jc, descc);                          \
  }
DLAF_MI355X_TRAN_ENTRY(s, tran, 'T', float, float)
DLAF_MI355X_TRAN_ENTRY(d, tran, 'T', double, double)
DLAF_MI355X_TRAN_ENTRY(c, tranu, 'T', std::complex<float>, dlaf_complex_c)
DLAF_MI355X_TRAN_ENTRY(c, tranc, 'C', std::complex<float>, dlaf_complex_c)
DLAF_MI355X_TRAN_ENTRY(z, tranu, 'T', std::complex<double>, dlaf_complex_z)
DLAF_MI355X_TRAN_ENTRY(z, tranc, 'C', std::complex<double>, dlaf_complex_z)
#undef DLAF_MI355X_TRAN_ENTRY
#define DLAF_MI355X_POTRS_ENTRY(S, HT, CT)                                                                       \
  void dlaf_mi355x_p##S##potrs(char uplo, int n, int nrhs, const CT* a, int ia, int ja, const int desca[9], CT* b,  \
                               int ib, int jb, const int descb[9], int* info) noexcept {                        \
    pxpotrs<HT>(uplo, n, nrhs, reinterpret_cast<const HT*>(a), ia, ja, desca, reinterpret_cast<HT*>(b), ib, jb,  \
                descb, info);                                                                                   \
  }
DLAF_MI355X_POTRS_ENTRY(s, float, float)
DLAF_MI355X_POTRS_ENTRY(d, double, double)
DLAF_MI355X_POTRS_ENTRY(c, std::complex<float>, dlaf_complex_c)
DLAF_MI355X_POTRS_ENTRY(z, std::complex<double>, dlaf_complex_z)
#undef DLAF_MI355X_POTRS_ENTRY

#define DLAF_MI355X_HEGST_ENTRY(S, HT, CT, RT)                                                                    \
  int dlaf_mi355x_generalized_to_standard_##S(int ctx, char uplo, CT* a, DLAF_descriptor desca, const CT* b,       \
                                              DLAF_descriptor descb) noexcept {                                  \
    return gen_to_std_c<HT>(ctx, uplo, reinterpret_cast<HT*>(a), desca, reinterpret_cast<const HT*>(b), descb);    \
  }                                                                                                              \
  void dlaf_mi355x_p##S##hegst(int ibtype, char uplo, int n, CT* a, int ia, int ja, const int desca[9], const CT* b, \
                               int ib, int jb, const int descb[9], RT* scale, int* info) noexcept {               \
    pxhegst<HT, RT>(ibtype, uplo, n, reinterpret_cast<HT*>(a), ia, ja, desca, reinterpret_cast<const HT*>(b), ib, \
                    jb, descb, scale, info);                                                                     \
  }
DLAF_MI355X_HEGST_ENTRY(s, float, float, float)
DLAF_MI355X_HEGST_ENTRY(d, double, double, double)
DLAF_MI355X_HEGST_ENTRY(c, std::complex<float>, dlaf_complex_c, float)
DLAF_MI355X_HEGST_ENTRY(z, std::complex<double>, dlaf_complex_z, double)
#undef DLAF_MI355X_HEGST_ENTRY

#define DLAF_MI355X_INVERSE_ENTRY(S, HT, CT)                                                                      \
  int dlaf_mi355x_triangular_inverse_##S(int ctx, char uplo, char diag, CT* a, DLAF_descriptor desca) noexcept {     \
    return inverse_c<HT>(ctx, uplo, diag, false, reinterpret_cast<HT*>(a), desca);                                  \
  }                                                                                                                \
  int dlaf_mi355x_inverse_from_cholesky_factor_##S(int ctx, char uplo, CT* a, DLAF_descriptor desca) noexcept {     \
    return inverse_c<HT>(ctx, uplo, 'N', true, reinterpret_cast<HT*>(a), desca);                                    \
  }                                                                                                                \
  void dlaf_mi355x_p##S##trtri(char uplo, char diag, int n, CT* a, int ia, int ja, const int desca[9],              \
                               int* info) noexcept {                                                               \
    pxinverse<HT>(uplo, diag, false, n, reinterpret_cast<HT*>(a), ia, ja, desca, info);                             \
  }                                                                                                                \
  void dlaf_mi355x_p##S##potri(char uplo, int n, CT* a, int ia, int ja, const int desca[9], int* info) noexcept {   \
    pxinverse<HT>(uplo, 'N', true, n, reinterpret_cast<HT*>(a), ia, ja, desca, info);                               \
  }
DLAF_MI355X_INVERSE_ENTRY(s, float, float)
DLAF_MI355X_INVERSE_ENTRY(d, double, double)
DLAF_MI355X_INVERSE_ENTRY(c, std::complex<float>, dlaf_complex_c)
DLAF_MI355X_INVERSE_ENTRY(z, std::complex<double>, dlaf_complex_z)
#undef DLAF_MI355X_INVERSE_ENTRY

#define DLAF_MI355X_NORM_ENTRY(S, HT, CT, RT, HE)                                                                  \
  int dlaf_mi355x_general_norm_##S(int ctx, char norm, const CT* a, DLAF_descriptor desca, double* value) noexcept { \
    return norm_c<HT>(ctx, norm, 'G', 'L', 'N', reinterpret_cast<const HT*>(a), desca, value);                      \
  }                                                                                                                \
  int dlaf_mi355x_hermitian_norm_##S(int ctx, char norm, char uplo, const CT* a, DLAF_descriptor desca,             \
                                     double* value) noexcept {                                                     \
    return norm_c<HT>(ctx, norm, 'H', uplo, 'N', reinterpret_cast<const HT*>(a), desca, value);                     \
  }                                                                                                                \
  int dlaf_mi355x_triangular_norm_##S(int ctx, char norm, char uplo, char diag, const CT* a, DLAF_descriptor desca, \
                                      double* value) noexcept {                                                    \
    return norm_c<HT>(ctx, norm, 'T', uplo, diag, reinterpret_cast<const HT*>(a), desca, value);                    \
  }                                                                                                                \
  RT dlaf_mi355x_p##S##lange(char norm, int m, int n, const CT* a, int ia, int ja, const int desca[9]) noexcept {    \
    return (RT) pxnorm<HT>(norm, 'G', 'L', 'N', m, n, reinterpret_cast<const HT*>(a), ia, ja, desca);               \
  }                                                                                                                \
  RT dlaf_mi355x_p##S##lan##HE(char norm, char uplo, int n, const CT* a, int ia, int ja,                            \
                               const int desca[9]) noexcept {                                                      \
    return (RT) pxnorm<HT>(norm, 'H', uplo, 'N', n, n, reinterpret_cast<const HT*>(a), ia, ja, desca);              \
  }                                                                                                                \
  RT dlaf_mi355x_p##S##lantr(char norm, char uplo, char diag, int n, const CT* a, int ia, int ja,                   \
                             const int desca[9]) noexcept {                                                        \
    return (RT) pxnorm<HT>(norm, 'T', uplo, diag, n, n, reinterpret_cast<const HT*>(a), ia, ja, desca);             \
  }
DLAF_MI355X_NORM_ENTRY(s, float, float, float, sy)
DLAF_MI355X_NORM_ENTRY(d, double, double, double, sy)
DLAF_MI355X_NORM_ENTRY(c, std::complex<float>, dlaf_complex_c, float, he)
DLAF_MI355X_NORM_ENTRY(z, std::complex<double>, dlaf_complex_z, double, he)
#undef DLAF_MI355X_NORM_ENTRY

#define DLAF_MI355X_R2B_ENTRY(S, HT, CT)                                                                          \
  int dlaf_mi355x_reduction_to_band_##S(int ctx, CT* a, DLAF_descriptor desca, int band, CT* taus) noexcept {     \
    return red2band_c<HT>(ctx, reinterpret_cast<HT*>(a), desca, band, reinterpret_cast<HT*>(taus));               \
  }                                                                                                              \
  int dlaf_mi355x_bt_reduction_to_band_##S(int ctx, int band, CT* c, DLAF_descriptor descc, const CT* v,          \
                                           DLAF_descriptor descv, const CT* taus) noexcept {                     \
    return bt_red2band_c<HT>(ctx, band, reinterpret_cast<HT*>(c), descc, reinterpret_cast<const HT*>(v), descv,   \
                             reinterpret_cast<const HT*>(taus));                                                 \
  }
DLAF_MI355X_R2B_ENTRY(s, float, float)
DLAF_MI355X_R2B_ENTRY(d, double, double)
DLAF_MI355X_R2B_ENTRY(c, std::complex<float>, dlaf_complex_c)
DLAF_MI355X_R2B_ENTRY(z, std::complex<double>, dlaf_complex_z)
#undef DLAF_MI355X_R2B_ENTRY


#define DLAF_MI355X_EIG_ENTRY(S, KIND, HT, CT, RT, PEV, PGV)                                                          \
  int dlaf_mi355x_band_to_tridiagonal_##S(int ctx, const CT* a, DLAF_descriptor desca, int band, RT* d, RT* e, CT* v, \
                                          int ldv) noexcept {                                                       \
    return band_to_tridiag_c<HT>(ctx, reinterpret_cast<const HT*>(a), desca, band, d, e, reinterpret_cast<HT*>(v), ldv); \
  }                                                                                                                  \
  int dlaf_mi355x_bt_band_to_tridiagonal_##S(int band, int n, int ncols, const CT* v, int ldv, CT* e, int lde) noexcept { \
    using DT = typename DevType<HT>::type;                                                                           \
    runtime_init();                                                                                                  \
    if (band < 2 || ldv < std::max(1, n) || lde < std::max(1, n))                                                    \
      fatal("[dlaf_mi355x] bt_band_to_tridiagonal: bad band_size / leading dimensions\n");                           \
    return bt_band_to_tridiag_host<DT>(n, band, reinterpret_cast<const DT*>(v), ldv, reinterpret_cast<DT*>(e), lde,   \
                                       ncols);                                                                       \
  }                                                                                                                  \
  int dlaf_##KIND##_eigensolver_##S(const int ctx, const char uplo, CT* a, const DLAF_descriptor desca, RT* w, CT* z, \
                                    const DLAF_descriptor descz) noexcept {                                          \
    return eigensolver_c<HT>(ctx, uplo, reinterpret_cast<HT*>(a), desca, w, reinterpret_cast<HT*>(z), descz, 0,      \
                             desca.m);                                                                               \
  }                                                                                                                  \
  int dlaf_##KIND##_eigensolver_partial_spectrum_##S(const int ctx, const char uplo, CT* a,                           \
                                                     const DLAF_descriptor desca, RT* w, CT* z,                      \
                                                     const DLAF_descriptor descz, const int64_t begin,               \
                                                     const int64_t end) noexcept {                                   \
    return eigensolver_c<HT>(ctx, uplo, reinterpret_cast<HT*>(a), desca, w, reinterpret_cast<HT*>(z), descz, begin,  \
                             end);                                                                                   \
  }                                                                                                                  \
  int dlaf_##KIND##_generalized_eigensolver_##S(const int ctx, const char uplo, CT* a, const DLAF_descriptor desca,   \
                                                CT* b, const DLAF_descriptor descb, RT* w, CT* z,                    \
                                                const DLAF_descriptor descz) noexcept {                              \
    return gen_eigensolver_c<HT>(ctx, uplo, reinterpret_cast<HT*>(a), desca, reinterpret_cast<HT*>(b), descb, w,      \
                                 reinterpret_cast<HT*>(z), descz, false, 0, desca.m);                                \
  }                                                                                                                  \
  int dlaf_##KIND##_generalized_eigensolver_factorized_##S(const int ctx, const char uplo, CT* a,                     \
                                                           const DLAF_descriptor desca, CT* b,                       \
                                                           const DLAF_descriptor descb, RT* w, CT* z,                \
                                                           const DLAF_descriptor descz) noexcept {                   \
    return gen_eigensolver_c<HT>(ctx, uplo, reinterpret_cast<HT*>(a), desca, reinterpret_cast<HT*>(b), descb, w,      \
                                 reinterpret_cast<HT*>(z), descz, true, 0, desca.m);                                 \
  }                                                                                                                  \
  int dlaf_##KIND##_generalized_eigensolver_partial_spectrum_##S(                                                     \
      const int ctx, const char uplo, CT* a, const DLAF_descriptor desca, CT* b, const DLAF_descriptor descb, RT* w,  \
      CT* z, const DLAF_descriptor descz, const int64_t begin, const int64_t end) noexcept {                         \
    return gen_eigensolver_c<HT>(ctx, uplo, reinterpret_cast<HT*>(a), desca, reinterpret_cast<HT*>(b), descb, w,      \
                                 reinterpret_cast<HT*>(z), descz, false, begin, end);                                \
  }                                                                                                                  \
  int dlaf_##KIND##_generalized_eigensolver_factorized_partial_spectrum_##S(                                          \
      const int ctx, const char uplo, CT* a, const DLAF_descriptor desca, CT* b, const DLAF_descriptor descb, RT* w,  \
      CT* z, const DLAF_descriptor descz, const int64_t begin, const int64_t end) noexcept {                         \
    return gen_eigensolver_c<HT>(ctx, uplo, reinterpret_cast<HT*>(a), desca, reinterpret_cast<HT*>(b), descb, w,      \
                                 reinterpret_cast<HT*>(z), descz, true, begin, end);                                 \
  }                                                                                                                  \
  void dlaf_##PEV(const char uplo, const int n, CT* a, const int ia, const int ja, const int desca[9], RT* w, CT* z,  \
                  const int iz, const int jz, const int descz[9], int* info) noexcept {                              \
    pxhegvd<HT>(uplo, n, reinterpret_cast<HT*>(a), ia, ja, desca, nullptr, 1, 1, nullptr, w, reinterpret_cast<HT*>(z), \
                iz, jz, descz, 1, n, info, false);                                                                   \
  }                                                                                                                  \
  void dlaf_##PEV##_partial_spectrum(const char uplo, const int n, CT* a, const int ia, const int ja,                 \
                                     const int desca[9], RT* w, CT* z, const int iz, const int jz,                   \
                                     const int descz[9], const int64_t il, const int64_t iu, int* info) noexcept {   \
    pxhegvd<HT>(uplo, n, reinterpret_cast<HT*>(a), ia, ja, desca, nullptr, 1, 1, nullptr, w, reinterpret_cast<HT*>(z), \
                iz, jz, descz, il, iu, info, false);                                                                 \
  }                                                                                                                  \
  void dlaf_##PGV(const char uplo, const int n, CT* a, const int ia, const int ja, const int desca[9], CT* b,         \
                  const int ib, const int jb, const int descb[9], RT* w, CT* z, const int iz, const int jz,          \
                  const int descz[9], int* info) noexcept {                                                          \
    pxhegvd<HT>(uplo, n, reinterpret_cast<HT*>(a), ia, ja, desca, reinterpret_cast<HT*>(b), ib, jb, descb, w,         \
                reinterpret_cast<HT*>(z), iz, jz, descz, 1, n, info, false);                                         \
  }                                                                                                                  \
  void dlaf_##PGV##_factorized(const char uplo, const int n, CT* a, const int ia, const int ja, const int desca[9],   \
                               CT* b, const int ib, const int jb, const int descb[9], RT* w, CT* z, const int iz,    \
                               const int jz, const int descz[9], int* info) noexcept {                               \
    pxhegvd<HT>(uplo, n, reinterpret_cast<HT*>(a), ia, ja, desca, reinterpret_cast<HT*>(b), ib, jb, descb, w,         \
                reinterpret_cast<HT*>(z), iz, jz, descz, 1, n, info, true);                                          \
  }                                                                                                                  \
  void dlaf_##PGV##_partial_spectrum(const char uplo, const int n, CT* a, const int ia, const int ja,                 \
                                     const int desca[9], CT* b, const int ib, const int jb, const int descb[9],      \
                                     RT* w, CT* z, const int iz, const int jz, const int descz[9], const int64_t il, \
                                     const int64_t iu, int* info) noexcept {                                         \
    pxhegvd<HT>(uplo, n, reinterpret_cast<HT*>(a), ia, ja, desca, reinterpret_cast<HT*>(b), ib, jb, descb, w,         \
                reinterpret_cast<HT*>(z), iz, jz, descz, il, iu, info, false);                                       \
  }                                                                                                                  \
  void dlaf_##PGV##_factorized_partial_spectrum(const char uplo, const int n, CT* a, const int ia, const int ja,      \
                                                const int desca[9], CT* b, const int ib, const int jb,               \
                                                const int descb[9], RT* w, CT* z, const int iz, const int jz,        \
                                                const int descz[9], const int64_t il, const int64_t iu,              \
                                                int* info) noexcept {                                                \
    pxhegvd<HT>(uplo, n, reinterpret_cast<HT*>(a), ia, ja, desca, reinterpret_cast<HT*>(b), ib, jb, descb, w,         \
                reinterpret_cast<HT*>(z), iz, jz, descz, il, iu, info, true);                                        \
  }
DLAF_MI355X_EIG_ENTRY(s, symmetric, float, float, float, pssyevd, pssygvd)
DLAF_MI355X_EIG_ENTRY(d, symmetric, double, double, double, pdsyevd, pdsygvd)
DLAF_MI355X_EIG_ENTRY(c, hermitian, std::complex<float>, dlaf_complex_c, float, pcheevd, pchegvd)
DLAF_MI355X_EIG_ENTRY(z, hermitian, std::complex<double>, dlaf_complex_z, double, pzheevd, pzhegvd)
#undef DLAF_MI355X_EIG_ENTRY

#define DLAF_MI355X_EIGVAL_ENTRY(S, KIND, HT, CT, RT, PEV, PGV)                                                       \
  int dlaf_##KIND##_eigenvalues_##S(const int ctx, const char uplo, const CT* a, const DLAF_descriptor desca, RT* w,  \
                                    const int64_t begin, const int64_t end) noexcept {                               \
    return eigenvalues_c<HT>(ctx, uplo, reinterpret_cast<const HT*>(a), desca, w, begin, end);                       \
  }                                                                                                                  \
  int dlaf_##KIND##_generalized_eigenvalues_##S(const int ctx, const char uplo, const CT* a,                          \
                                                const DLAF_descriptor desca, CT* b, const DLAF_descriptor descb,     \
                                                RT* w, const int64_t begin, const int64_t end) noexcept {            \
    return gen_eigenvalues_c<HT>(ctx, uplo, reinterpret_cast<const HT*>(a), desca, reinterpret_cast<HT*>(b), descb,   \
                                 w, false, begin, end);                                                              \
  }                                                                                                                  \
  int dlaf_##KIND##_generalized_eigenvalues_factorized_##S(const int ctx, const char uplo, const CT* a,               \
                                                           const DLAF_descriptor desca, CT* b,                       \
                                                           const DLAF_descriptor descb, RT* w, const int64_t begin,  \
                                                           const int64_t end) noexcept {                             \
    return gen_eigenvalues_c<HT>(ctx, uplo, reinterpret_cast<const HT*>(a), desca, reinterpret_cast<HT*>(b), descb,   \
                                 w, true, begin, end);                                                               \
  }                                                                                                                  \
  int dlaf_##KIND##_eigensolver_partial_spectrum_by_value_##S(const int ctx, const char uplo, CT* a,                  \
                                                              const DLAF_descriptor desca, RT* w, CT* z,             \
                                                              const DLAF_descriptor descz, const RT vl, const RT vu, \
                                                              long* begin, long* end) noexcept {                     \
    return eigensolver_by_value_c<HT>(ctx, uplo, reinterpret_cast<HT*>(a), desca, w, reinterpret_cast<HT*>(z), descz, \
                                      vl, vu, begin, end);                                                           \
  }                                                                                                                  \
  int dlaf_##KIND##_generalized_eigensolver_partial_spectrum_by_value_##S(                                            \
      const int ctx, const char uplo, CT* a, const DLAF_descriptor desca, CT* b, const DLAF_descriptor descb, RT* w,  \
      CT* z, const DLAF_descriptor descz, const RT vl, const RT vu, long* begin, long* end) noexcept {               \
    return gen_eigensolver_by_value_c<HT>(ctx, uplo, reinterpret_cast<HT*>(a), desca, reinterpret_cast<HT*>(b),       \
                                          descb, w, reinterpret_cast<HT*>(z), descz, false, vl, vu, begin, end);     \
  }                                                                                                                  \
  int dlaf_##KIND##_generalized_eigensolver_factorized_partial_spectrum_by_value_##S(                                 \
      const int ctx, const char uplo, CT* a, const DLAF_descriptor desca, CT* b, const DLAF_descriptor descb, RT* w,  \
      CT* z, const DLAF_descriptor descz, const RT vl, const RT vu, long* begin, long* end) noexcept {               \
    return gen_eigensolver_by_value_c<HT>(ctx, uplo, reinterpret_cast<HT*>(a), desca, reinterpret_cast<HT*>(b),       \
                                          descb, w, reinterpret_cast<HT*>(z), descz, true, vl, vu, begin, end);      \
  }                                                                                                                  \
  void dlaf_##PEV##_eigenvalues(const char uplo, const int n, const CT* a, const int ia, const int ja,                \
                                const int desca[9], RT* w, const int64_t il, const int64_t iu, int* info) noexcept { \
    pxhegvd_eigenvalues<HT>(uplo, n, reinterpret_cast<const HT*>(a), ia, ja, desca, nullptr, 1, 1, nullptr, w, il,    \
                            iu, info, false);                                                                        \
  }                                                                                                                  \
  void dlaf_##PGV##_eigenvalues(const char uplo, const int n, const CT* a, const int ia, const int ja,                \
                                const int desca[9], CT* b, const int ib, const int jb, const int descb[9], RT* w,    \
                                const int64_t il, const int64_t iu, int* info) noexcept {                            \
    pxhegvd_eigenvalues<HT>(uplo, n, reinterpret_cast<const HT*>(a), ia, ja, desca, reinterpret_cast<HT*>(b), ib, jb, \
                            descb, w, il, iu, info, false);                                                          \
  }                                                                                                                  \
  void dlaf_##PGV##_eigenvalues_factorized(const char uplo, const int n, const CT* a, const int ia, const int ja,     \
                                           const int desca[9], CT* b, const int ib, const int jb,                    \
                                           const int descb[9], RT* w, const int64_t il, const int64_t iu,            \
                                           int* info) noexcept {                                                     \
    pxhegvd_eigenvalues<HT>(uplo, n, reinterpret_cast<const HT*>(a), ia, ja, desca, reinterpret_cast<HT*>(b), ib, jb, \
                            descb, w, il, iu, info, true);                                                           \
  }                                                                                                                  \
  void dlaf_##PEV##_partial_spectrum_by_value(const char uplo, const int n, CT* a, const int ia, const int ja,        \
                                              const int desca[9], RT* w, CT* z, const int iz, const int jz,          \
                                              const int descz[9], const RT vl, const RT vu, int* m,                  \
                                              int* info) noexcept {                                                  \
    pxhegvd_by_value<HT>(uplo, n, reinterpret_cast<HT*>(a), ia, ja, desca, nullptr, 1, 1, nullptr, w,                 \
                         reinterpret_cast<HT*>(z), iz, jz, descz, vl, vu, m, info, false);                           \
  }                                                                                                                  \
  void dlaf_##PGV##_partial_spectrum_by_value(const char uplo, const int n, CT* a, const int ia, const int ja,        \
                                              const int desca[9], CT* b, const int ib, const int jb,                 \
                                              const int descb[9], RT* w, CT* z, const int iz, const int jz,          \
                                              const int descz[9], const RT vl, const RT vu, int* m,                  \
                                              int* info) noexcept {                                                  \
    pxhegvd_by_value<HT>(uplo, n, reinterpret_cast<HT*>(a), ia, ja, desca, reinterpret_cast<HT*>(b), ib, jb, descb,   \
                         w, reinterpret_cast<HT*>(z), iz, jz, descz, vl, vu, m, info, false);                        \
  }                                                                                                                  \
  void dlaf_##PGV##_factorized_partial_spectrum_by_value(const char uplo, const int n, CT* a, const int ia,           \
                                                         const int ja, const int desca[9], CT* b, const int ib,      \
                                                         const int jb, const int descb[9], RT* w, CT* z,             \
                                                         const int iz, const int jz, const int descz[9],             \
                                                         const RT vl, const RT vu, int* m, int* info) noexcept {     \
    pxhegvd_by_value<HT>(uplo, n, reinterpret_cast<HT*>(a), ia, ja, desca, reinterpret_cast<HT*>(b), ib, jb, descb,   \
                         w, reinterpret_cast<HT*>(z), iz, jz, descz, vl, vu, m, info, true);                         \
  }
DLAF_MI355X_EIGVAL_ENTRY(s, symmetric, float, float, float, pssyevd, pssygvd)
DLAF_MI355X_EIGVAL_ENTRY(d, symmetric, double, double, double, pdsyevd, pdsygvd)
DLAF_MI355X_EIGVAL_ENTRY(c, hermitian, std::complex<float>, dlaf_complex_c, float, pcheevd, pchegvd)
DLAF_MI355X_EIGVAL_ENTRY(z, hermitian, std::complex<double>, dlaf_complex_z, double, pzheevd, pzhegvd)
#undef DLAF_MI355X_EIGVAL_ENTRY

int dlaf_mi355x_tridiagonal_eigenvalues_s(int n, const float* d, const float* e, float* w, long begin,
                                          long end) noexcept {
  runtime_init();
  return tridiag_eigenvalues_host<float>(n, d, e, w, begin, end);
}
int dlaf_mi355x_tridiagonal_eigenvalues_d(int n, const double* d, const double* e, double* w, long begin,
                                          long end) noexcept {
  runtime_init();
  return tridiag_eigenvalues_host<double>(n, d, e, w, begin, end);
}
int dlaf_mi355x_tridiagonal_sturm_count_s(int n, const float* d, const float* e, long nshifts, const float* shifts,
                                          long* counts) noexcept {
  runtime_init();
  return sturm_count_host<float>(n, d, e, nshifts, shifts, counts);
}
int dlaf_mi355x_tridiagonal_sturm_count_d(int n, const double* d, const double* e, long nshifts, const double* shifts,
                                          long* counts) noexcept {
  runtime_init();
  return sturm_count_host<double>(n, d, e, nshifts, shifts, counts);
}
int dlaf_mi355x_sturm_layout(int out[2]) noexcept {
  out[0] = kSturmChunk;
  out[1] = kSturmThreads;
  return 0;
}

int dlaf_mi355x_tridiagonal_eigensolver_s(int n, int nb, const float* d, const float* e, float* w, float* z,
                                          int ldz) noexcept {
  runtime_init();
  return tridiag_solver_host<float>(n, nb, d, e, w, z, ldz, 0, n);
}
int dlaf_mi355x_tridiagonal_eigensolver_d(int n, int nb, const double* d, const double* e, double* w, double* z,
                                          int ldz) noexcept {
  runtime_init();
  return tridiag_solver_host<double>(n, nb, d, e, w, z, ldz, 0, n);
}
int dlaf_mi355x_tridiagonal_eigensolver_partial_spectrum_s(int n, int nb, const float* d, const float* e, float* w,
                                                           float* z, int ldz, long begin, long end) noexcept {
  check_eigenvalues_index("tridiagonal_eigensolver", n, begin, end);
  runtime_init();
  return tridiag_solver_host<float>(n, nb, d, e, w, z, ldz, begin, end);
}
int dlaf_mi355x_tridiagonal_eigensolver_partial_spectrum_d(int n, int nb, const double* d, const double* e, double* w,
                                                           double* z, int ldz, long begin, long end) noexcept {
  check_eigenvalues_index("tridiagonal_eigensolver", n, begin, end);
  runtime_init();
  return tridiag_solver_host<double>(n, nb, d, e, w, z, ldz, begin, end);
}
int dlaf_mi355x_get_eigensolver_min_band(void) noexcept {
  return eigensolver_min_band();
}
void dlaf_mi355x_set_eigensolver_min_band(int b_min) noexcept {
  set_eigensolver_min_band(b_min);
}
int dlaf_mi355x_get_band_size(int nb) noexcept {
  return get_band_size(nb);
}
}  // extern "C"
