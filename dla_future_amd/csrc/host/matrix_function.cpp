// matrix_function.cpp -- functions of a Hermitian matrix: the lower triangle of A becomes that of
//        f(A) = sum_{j selected} g_j z_j z_j^H,      (w, Z) the eigenpairs of A,  g = weights(w)
// -- a density matrix, a spectral projector, S^(-1/2), a square root, an inverse or pseudo-inverse, an exponential.  It is
// the weighted rank-k update (rank_update.cpp: C = alpha A D A^H + beta C) behind the eigensolver (eigensolver.cpp):
//   1. hermitian_eigensolver_resident on A with its selection: all pairs, an index range [begin, end), or a value
//      interval (vl, vu].  Z stays resident, n x (end - b0) on A's row source, b0 = (begin / nb) nb.
//   2. ONE call of the weights callback on the host with all n eigenvalues and the selected range; it fills g[begin, end).
//      Unselected eigenvalues weigh 0 by definition: their eigenvectors were never computed.
//   3. the weighted update, trans N, alpha = 1, beta = 0, k = end - b0, into A's own DeviceMatrix; the padding columns
//      [b0, begin) of Z are zero and get weight 0.  An empty selection: k = 0, a zero triangle.
// Z is never downloaded; the host form downloads the triangle alone.  The eigensolver's status comes back as it is; on a
// non-zero one nothing is synthesised and the host form leaves the caller's array unchanged.  uplo is 'L', as for the
// eigensolver.  Grids: whatever the eigensolver and the trans-N update run on.
#include <memory>
#include <vector>

#include "drivers.hpp"
#include "eigensolver.hpp"
#include "tile_matrix.hpp"
#include "transport.hpp"

namespace dlaf_mi355x {

template <class T>
int hermitian_function_resident(DeviceMatrix<T>& A, real_t<T>* w_host, const real_t<T>* by_value, long& begin, long& end,
                                SpectralWeights weights, void* user) {
  using R = real_t<T>;
  const long n = A.n;
  if (A.transposed)
    fatal("[dlaf_mi355x] hermitian function: the resident matrix holds its 'U' triangle; uplo 'U' is not implemented "
          "(neither by the eigensolver)\n");
  if (n == 0) {
    begin = end = 0;
    return 0;
  }
  std::unique_ptr<MatrixBase> zh;
  PartialSpectrumPlan pl;
  const int info = hermitian_eigensolver_resident(A, w_host, by_value, begin, end, zh, pl);
  if (info != 0)
    return info;
  auto& Z = static_cast<GeneralMatrix<T>&>(*zh);
  std::vector<R> g((size_t) n, R(0));
  const bool any = end > begin;
  if (any)
    weights(n, w_host, begin, end, g.data(), user);
  for (long j = pl.b0; j < begin; ++j)
    g[(size_t) j] = R(0);  // (the padding columns, whatever the callback left there)
  hermitian_weighted_update_resident<T>(A, Z.m, g.data() + pl.b0, any ? end - pl.b0 : 0, make_host_el<T>(1.0), R(0));
  return 0;
}

template <class T>
int hermitian_function_host(Grid* g, char uplo, HostOperand<T> a, real_t<T>* w_host, const real_t<T>* by_value, long& begin,
                            long& end, SpectralWeights weights, void* user) {
  if (a.n == 0) {
    begin = end = 0;
    return 0;
  }
  (void) uplo;  // ('L': the entry has judged it)
  (void) checked_transport(*g);
  DeviceMatrix<T> A;
  A.create(g, 'L', a.n, a.nb, a.isrc, a.jsrc);
  A.upload(a.p, a.ld);
  const int info = hermitian_function_resident<T>(A, w_host, by_value, begin, end, weights, user);
  if (info == 0)
    A.download(a.p, a.ld);
  return info;
}

#define DLAF_MATRIX_FUNCTION_INST(T)                                                                                    \
  template int hermitian_function_resident<T>(DeviceMatrix<T>&, real_t<T>*, const real_t<T>*, long&, long&,            \
                                              SpectralWeights, void*);                                                 \
  template int hermitian_function_host<T>(Grid*, char, HostOperand<T>, real_t<T>*, const real_t<T>*, long&, long&,      \
                                          SpectralWeights, void*);
DLAF_MATRIX_FUNCTION_INST(float)
DLAF_MATRIX_FUNCTION_INST(double)
DLAF_MATRIX_FUNCTION_INST(cfloat)
DLAF_MATRIX_FUNCTION_INST(cdouble)
#undef DLAF_MATRIX_FUNCTION_INST

}  // namespace dlaf_mi355x
