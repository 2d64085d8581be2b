// test_hermitian_rank_update_cpp.cpp -- dlaf::hermitian_rank_k_update / hermitian_rank_2k_update of the facade
// include/dlaf_mi355x/dlaf.hpp on one process: the rank-k update, Lower / NoTrans (double, through the grid overload
// too) and Upper / ConjTrans (complex<double>), and the rank-2k update, Lower / ConjTrans (double) and Upper / NoTrans
// (complex<double>, complex alpha), at n = 150, k = 90, nb = 64, against loop products in this program.  The operands
// are small integers, so the comparison is for equality; the other triangle must keep its value, the diagonal of a
// complex C -- imaginary part 7 on entry -- must come back real.  One process, one GPU.
#include <complex>
#include <cstdio>
#include <vector>

#include <dlaf_mi355x/dlaf.hpp>

using namespace dlaf;

static int failures = 0;
constexpr SizeType n = 150, k = 90, nb = 64;

static double small_int(SizeType i, SizeType j, int salt) {
  return (double) ((int) ((7 * i + 3 * j + salt) % 7) - 3);
}
template <class T>
static T make(SizeType i, SizeType j, int salt) {
  if constexpr (std::is_same_v<T, double>)
    return small_int(i, j, salt);
  else
    return T(small_int(i, j, salt), small_int(j, i, salt + 2));
}
template <class T>
static T conj_of(const T& v) {
  if constexpr (std::is_same_v<T, double>)
    return v;
  else
    return std::conj(v);
}

// form: 0 the local overload, 1 the grid overload
template <class T>
static void run(comm::CommunicatorGrid& grid, bool two, blas::Uplo uplo, blas::Op op, int form, const char* name) {
  const bool tn = op == blas::Op::NoTrans, lower = uplo == blas::Uplo::Lower;
  const SizeType ar = tn ? n : k, ac = tn ? k : n;
  Matrix<T, Device::CPU> a(LocalElementSize(ar, ac), TileElementSize(nb, nb));
  Matrix<T, Device::CPU> b(LocalElementSize(ar, ac), TileElementSize(nb, nb));
  Matrix<T, Device::CPU> c(LocalElementSize(n, n), TileElementSize(nb, nb));
  for (SizeType j = 0; j < ac; ++j)
    for (SizeType i = 0; i < ar; ++i) {
      a(LocalElementIndex(i, j)) = make<T>(i, j, 1);
      b(LocalElementIndex(i, j)) = make<T>(i, j, 4);
    }
  // op(X)(i, l): row i of X (NoTrans) or conj of column i
  auto at = [&](Matrix<T, Device::CPU>& x, SizeType i, SizeType l) {
    return tn ? x(LocalElementIndex(i, l)) : conj_of<T>(x(LocalElementIndex(l, i)));
  };
  const T untouched = make<T>(2, 1, 6) + T(100);
  const BaseType<T> ralpha = 2, beta = -3;
  const T alpha = two ? make<T>(1, 0, 5) : T(ralpha);
  std::vector<T> want((size_t) (n * n));
  for (SizeType j = 0; j < n; ++j)
    for (SizeType i = 0; i < n; ++i) {
      const bool in = lower ? i >= j : i <= j;
      T c0 = make<T>(i, j, 3);
      if constexpr (!std::is_same_v<T, double>)
        if (i == j)
          c0 = T(c0.real(), 7);
      c(LocalElementIndex(i, j)) = in ? c0 : untouched;
      if (!in) {
        want[(size_t) (i + j * n)] = untouched;
        continue;
      }
      if constexpr (!std::is_same_v<T, double>)
        if (i == j)
          c0 = T(c0.real(), 0);
      // C(i, j) = alpha sum op(A)(i, l) conj(op(B)(j, l)) [+ conj(alpha) sum op(B)(i, l) conj(op(A)(j, l))] + beta C
      T s1 = T(0), s2 = T(0);
      for (SizeType l = 0; l < k; ++l) {
        s1 += at(a, i, l) * conj_of<T>(at(two ? b : a, j, l));
        if (two)
          s2 += at(b, i, l) * conj_of<T>(at(a, j, l));
      }
      want[(size_t) (i + j * n)] = alpha * s1 + conj_of<T>(alpha) * s2 + T(beta) * c0;
    }
  if (two && form == 0)
    hermitian_rank_2k_update<Backend::GPU, Device::GPU, T>(uplo, op, alpha, a, b, beta, c);
  else if (two)
    hermitian_rank_2k_update<Backend::GPU, Device::GPU, T>(grid, uplo, op, alpha, a, b, beta, c);
  else if (form == 0)
    hermitian_rank_k_update<Backend::GPU, Device::GPU, T>(uplo, op, ralpha, a, beta, c);
  else
    hermitian_rank_k_update<Backend::GPU, Device::GPU, T>(grid, uplo, op, ralpha, a, beta, c);
  long bad = 0;
  for (SizeType j = 0; j < n; ++j)
    for (SizeType i = 0; i < n; ++i)
      if (!(c(LocalElementIndex(i, j)) == want[(size_t) (i + j * n)]))
        ++bad;
  std::printf("%s: %ld of %ld elements differ\n", name, bad, (long) (n * n));
  if (bad != 0)
    ++failures;
}

int main() {
  dlaf_initialize(0, nullptr, 0, nullptr);
  {
    comm::CommunicatorGrid grid = comm::CommunicatorGrid::single();
    using Z = std::complex<double>;
    run<double>(grid, false, blas::Uplo::Lower, blas::Op::NoTrans, 0, "double rank-k L N");
    run<double>(grid, false, blas::Uplo::Lower, blas::Op::NoTrans, 1, "double rank-k L N (grid overload)");
    run<Z>(grid, false, blas::Uplo::Upper, blas::Op::ConjTrans, 0, "complex<double> rank-k U C");
    run<double>(grid, true, blas::Uplo::Lower, blas::Op::ConjTrans, 0, "double rank-2k L C");
    run<Z>(grid, true, blas::Uplo::Upper, blas::Op::NoTrans, 1, "complex<double> rank-2k U N (grid overload)");
  }
  dlaf_finalize();
  if (failures == 0)
    std::printf("CPP_HERMITIAN_RANK_UPDATE_TEST OK\n");
  return failures == 0 ? 0 : 1;
}
