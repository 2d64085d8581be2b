// norm.cpp -- max / one / infinity / Frobenius norm of a general, Hermitian (symmetric) or triangular distributed matrix
// (LAPACK xLANGE, xLANHE / xLANSY, xLANTR; ScaLAPACK p?lange ...; the reference's dlaf::auxiliary::max_norm,
// include/dlaf/auxiliary/norm.h).  Read-only: nothing is written to the operand, host or resident.
//
// One process: pass 1 streams the referenced tiles (kernels_norm.hip), pass 2 folds the partials in a fixed order, a
// handful of doubles comes back.  On a grid the partials meet through the transport:
//   max and the NaN flag     Transport::allreduce_max of two host doubles
//   sum of squares           Transport::allreduce_sum of the three xLASSQ accumulators (type d, scope A)
//   column / row sums        pass 2 writes this process's share of the n-vector at its GLOBAL indices (0 elsewhere);
//                            Transport::allreduce_sum over scope A, then the max of the vector on the device
// Both all-reduces leave the same bits on every rank, so the value is the same on every rank.
// The Hermitian and the triangular structure read the lower triangle of the VIEW (uplo U: the transposed view, as in the
// inverse and the multiplications): for Hermitian matrices the one and the infinity norm coincide, for a triangular
// matrix on a transposed view they trade places here, on the host.
// Special values as in current LAPACK: a NaN anywhere in the referenced part gives NaN, otherwise an Inf gives +Inf.
#include <algorithm>
#include <cmath>
#include <limits>

#include "drivers.hpp"
#include "pool.hpp"
#include "tile_matrix.hpp"

namespace dlaf_mi355x {

namespace {

double g_profile_ms = 0, g_profile_bytes = 0;

// the end of xLASSQ + xNRM2 (LAPACK 3.10): sqrt of the sum of squares from its three scaled accumulators
double combine_squares(double big, double med, double sml) {
  constexpr double kSsml = 0x1p537, kSbig = 0x1p-538;
  double scl, sumsq;
  if (big > 0) {
    if (med > 0 || med != med)
      big += (med * kSbig) * kSbig;
    scl = 1.0 / kSbig;
    sumsq = big;
  }
  else if (sml > 0) {
    if (med > 0 || med != med) {
      const double a = std::sqrt(med), b = std::sqrt(sml) / kSsml;
      const double ymin = std::min(a, b), ymax = std::max(a, b);
      scl = 1.0;
      sumsq = ymax * ymax * (1.0 + (ymin / ymax) * (ymin / ymax));
    }
    else {
      scl = 1.0 / kSsml;
      sumsq = sml;
    }
  }
  else {
    scl = 1.0;
    sumsq = med;
  }
  return scl * std::sqrt(sumsq);
}

// kind: 'M', '1', 'I', 'F' in terms of the VIEW whose local tiles are given; structure 0 / 1 / 2 (norm_split.hpp)
template <class T>
double norm_of_view(Grid& grid, char kind, int structure, bool unit, const T* tiles, const Axis& rows, const Axis& cols,
                    int nb, hipStream_t s) {
  Transport* tr = checked_transport(grid);
  const bool dist = grid.nranks > 1;
  g_profile_ms = 0;
  g_profile_bytes = 0;
  const long ltr = rows.local_tiles(), ltc = cols.local_tiles();
  if (ltr > 65535 || ltc > 65535)
    fatal("[dlaf_mi355x] norm: %ld x %ld local tiles exceed the launch grid\n", ltr, ltc);
  NormArgs<T> a{};
  a.tiles = tiles;
  a.g = NormGeom{(int) ltr, (int) ltc, nb, rows.local_size(), cols.local_size(), rows.P, rows.shift(), cols.P,
                 cols.shift(), structure};
  a.s = norm_split(nb, (int) sizeof(T), norm_aligned16(tiles, nb, (int) sizeof(T)), norm_referenced_tiles(a.g));
  a.unit = unit ? 1 : 0;
  switch (kind) {
    case 'M': a.mode = kNormMax; break;
    case 'F': a.mode = kNormFro; break;
    case '1': a.mode = structure == 1 ? kNormColRow : kNormCol; break;
    default: a.mode = structure == 1 ? kNormColRow : kNormRow; break;
  }
  const bool sums = a.mode == kNormCol || a.mode == kNormRow || a.mode == kNormColRow;
  const long len = !sums ? 0 : (a.mode == kNormRow ? rows.n : cols.n);
  const long units = norm_unit_count(a.g, a.s);
  PoolScope ws;
  double* scal = ws.get<double>((size_t) units * kNormScalars);
  double* colp = ws.get<double>((a.mode & kNormCol) && sums ? (size_t) norm_colp_elems(a.g, a.s) : 0);
  double* rowp = ws.get<double>((a.mode & kNormRow) && sums ? (size_t) norm_rowp_elems(a.g, a.s) : 0);
  double* vec = ws.get<double>((size_t) len);
  double* out = ws.get<double>(8);
  a.scal = scal;
  a.colp = colp;
  a.rowp = rowp;

  double bytes = 0;
  for (int jl = 0; jl < a.g.ltc; ++jl)
    for (int il = 0; il < a.g.ltr; ++il)
      if (norm_tile_referenced(a.g, il, jl))
        bytes += (double) norm_tile_rows(a.g, il) * norm_tile_cols(a.g, jl) * sizeof(T);

  hipEvent_t e0, e1;
  DLAF_HIP_CHECK(hipEventCreate(&e0));
  DLAF_HIP_CHECK(hipEventCreate(&e1));
  DLAF_HIP_CHECK(hipEventRecord(e0, s));
  launch_norm_pass1(a, s);
  launch_norm_scalars(scal, units, out, s);
  if (a.mode == kNormFro && dist)
    tr->allreduce_sum(out + 2, 3, 'd', 'A', s);
  if (sums) {
    launch_norm_vector(a.g, a.s, a.mode, colp, rowp, vec, len, s);
    if (dist)
      tr->allreduce_sum(vec, (size_t) len, 'd', 'A', s);
    launch_norm_vecmax(vec, len, out + kNormScalars, s);
  }
  DLAF_HIP_CHECK(hipEventRecord(e1, s));
  double h[kNormScalars + 1] = {0, 0, 0, 0, 0, 0};
  DLAF_HIP_CHECK(hipMemcpyAsync(h, out, sizeof(h), hipMemcpyDeviceToHost, s));
  DLAF_HIP_CHECK(hipStreamSynchronize(s));
  float ms = 0;
  DLAF_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
  (void) hipEventDestroy(e0);
  (void) hipEventDestroy(e1);
  g_profile_ms = ms;
  g_profile_bytes = bytes;

  double mf[2] = {h[0], h[1]};
  if (dist)
    tr->allreduce_max(mf, 2, grid.nprow, grid.npcol, grid.myrow, grid.mycol);
  double v;
  if (mf[1] > 0)
    v = std::numeric_limits<double>::quiet_NaN();
  else if (a.mode == kNormMax)
    v = mf[0];
  else if (a.mode == kNormFro)
    v = combine_squares(h[2], h[3], h[4]);
  else
    v = h[kNormScalars];
  if (sizeof(real_t<T>) == sizeof(float))
    v = (double) (float) v;  // the value of the s / c routines is a float
  return v;
}

int structure_index(char structure) {
  switch (structure) {
    case 'G': case 'g': return 0;
    case 'H': case 'h': case 'S': case 's': return 1;
    case 'T': case 't': return 2;
    default: fatal("[dlaf_mi355x] norm: structure must be 'G', 'H' or 'T', got '%c'\n", structure);
  }
}

template <class T>
double norm_of_device_matrix(char kind, int structure, bool unit, const DeviceMatrix<T>& A) {
  // work enqueued on the matrix's other streams (a cholesky_start without a wait) must be done before it is read here
  for (hipStream_t ls : {A.s_low, A.s_comm})
    if (ls != nullptr && ls != A.s_high)
      DLAF_HIP_CHECK(hipStreamSynchronize(ls));
  if (structure == 2 && A.transposed && (kind == '1' || kind == 'I'))
    kind = kind == '1' ? 'I' : '1';  // the columns of the view are the caller's rows
  return norm_of_view(*A.grid, kind, structure, unit, A.tiles, A.rows, A.cols, A.nb, A.s_high);
}

template <class T>
double norm_of_tile_matrix(char kind, const TileMatrix<T>& A, hipStream_t s) {
  return norm_of_view(*A.grid, kind, 0, false, A.tiles, A.rows, A.cols, A.nb, s);
}

}  // namespace

char norm_kind(char norm) {
  switch (norm) {
    case 'M': case 'm': return 'M';
    case '1': case 'O': case 'o': return '1';
    case 'I': case 'i': return 'I';
    case 'F': case 'f': case 'E': case 'e': return 'F';
    default: return 0;
  }
}

static char checked_kind(char norm) {
  const char k = norm_kind(norm);
  if (k == 0)
    fatal("[dlaf_mi355x] norm: norm must be one of M, 1, O, I, F, E, got '%c'\n", norm);
  return k;
}
static bool checked_unit(char diag) {
  if (diag == 'U' || diag == 'u')
    return true;
  if (diag != 'N' && diag != 'n')
    fatal("[dlaf_mi355x] norm: diag must be 'N' or 'U', got '%c'\n", diag);
  return false;
}

template <class T>
double general_norm_host(Grid* g, char norm, HostOperand<const T> a) {
  const char kind = checked_kind(norm);
  if (a.m <= 0 || a.n <= 0)
    return 0.0;
  runtime_init();
  ScratchStream s;
  TileMatrix<T> A;
  A.create(g, false, a.m, a.n, a.nb, a.isrc, a.jsrc);
  A.upload(a.p, a.ld, false, false, T{}, s);
  return norm_of_tile_matrix(kind, A, s);
}

template <class T>
double structured_norm_host(Grid* g, char norm, char structure, char uplo, char diag, HostOperand<const T> a) {
  const char kind = checked_kind(norm);
  const int st = structure_index(structure);
  const bool unit = st == 2 && checked_unit(diag);
  if (st == 0)
    return general_norm_host<T>(g, norm, a);
  if (a.n <= 0)
    return 0.0;
  DeviceMatrix<T> A;
  A.create(g, uplo, a.n, a.nb, a.isrc, a.jsrc);
  A.upload(a.p, a.ld);
  return norm_of_device_matrix(kind, st, unit, A);
}

template <class T>
double structured_norm_device(char norm, char structure, char diag, const DeviceMatrix<T>& A) {
  const char kind = checked_kind(norm);
  const int st = structure_index(structure);
  if (st == 0)
    fatal("[dlaf_mi355x] norm: a resident Hermitian / triangular matrix holds one triangle, not a general matrix\n");
  const bool unit = st == 2 && checked_unit(diag);
  if (A.n <= 0)
    return 0.0;
  return norm_of_device_matrix(kind, st, unit, A);
}

double general_norm_device(char norm, MatrixBase* h) {
  const char kind = checked_kind(norm);
  return dispatch_type(h->type, [&](auto* tag) -> double {
    using T = std::remove_pointer_t<decltype(tag)>;
    auto& gm = static_cast<GeneralMatrix<T>&>(*h);
    if (gm.rows_g <= 0 || gm.cols_g <= 0)
      return 0.0;
    ScratchStream s;
    return norm_of_tile_matrix(kind, gm.m, s);
  });
}

void norm_last_profile(double* ms, double* bytes) {
  if (ms)
    *ms = g_profile_ms;
  if (bytes)
    *bytes = g_profile_bytes;
}

#define INST(T)                                                                                                    \
  template double general_norm_host<T>(Grid*, char, HostOperand<const T>);                                         \
  template double structured_norm_host<T>(Grid*, char, char, char, char, HostOperand<const T>);                    \
  template double structured_norm_device<T>(char, char, char, const DeviceMatrix<T>&);
INST(float)
INST(double)
INST(cfloat)
INST(cdouble)
#undef INST

}  // namespace dlaf_mi355x
