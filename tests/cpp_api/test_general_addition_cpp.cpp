// test_general_addition_cpp.cpp -- dlaf::general_addition / hermitian_complete of the facade
// include/dlaf_mi355x/dlaf.hpp on one process: one addition and one completion per element type (the four of them cover
// General / Lower / Upper, NoTrans / Trans / ConjTrans, both kinds, the local and the grid overloads) at m = 150, n = 90,
// nb = 64, against loops in this program.  The operands are small integers, so the comparison is for equality; outside
// the part C must keep its value.  One process, one GPU.
#include <complex>
#include <cstdio>
#include <vector>

#include <dlaf_mi355x/dlaf.hpp>

using namespace dlaf;

static int failures = 0;
constexpr SizeType m = 150, n = 90, nb = 64;

static double small_int(SizeType i, SizeType j, int salt) {
  return (double) ((int) ((7 * i + 3 * j + salt) % 7) - 3);
}
template <class T>
static T make(SizeType i, SizeType j, int salt) {
  if constexpr (std::is_floating_point_v<T>)
    return (T) small_int(i, j, salt);
  else
    return T((BaseType<T>) small_int(i, j, salt), (BaseType<T>) small_int(j, i, salt + 2));
}
template <class T>
static T conj_of(const T& v) {
  if constexpr (std::is_floating_point_v<T>)
    return v;
  else
    return std::conj(v);
}
static bool in_part(blas::Uplo uplo, SizeType i, SizeType j) {
  return uplo == blas::Uplo::General || (uplo == blas::Uplo::Lower ? i >= j : i <= j);
}

// form: 0 the local overload, 1 the grid overload
template <class T>
static void run_addition(comm::CommunicatorGrid& grid, blas::Uplo uplo, blas::Op op, int form, const char* name) {
  const bool tn = op == blas::Op::NoTrans;
  const SizeType ar = tn ? m : n, ac = tn ? n : m;
  Matrix<T, Device::CPU> a(LocalElementSize(ar, ac), TileElementSize(nb, nb));
  Matrix<T, Device::CPU> c(LocalElementSize(m, n), TileElementSize(nb, nb));
  for (SizeType j = 0; j < ac; ++j)
    for (SizeType i = 0; i < ar; ++i)
      a(LocalElementIndex(i, j)) = make<T>(i, j, 1);
  const T alpha = make<T>(1, 0, 5), beta = make<T>(0, 2, 6);
  std::vector<T> want((size_t) (m * n));
  for (SizeType j = 0; j < n; ++j)
    for (SizeType i = 0; i < m; ++i) {
      const T c0 = make<T>(i, j, 3);
      c(LocalElementIndex(i, j)) = c0;
      const T s = tn ? a(LocalElementIndex(i, j))
                     : (op == blas::Op::Trans ? a(LocalElementIndex(j, i)) : conj_of<T>(a(LocalElementIndex(j, i))));
      want[(size_t) (i + j * m)] = in_part(uplo, i, j) ? beta * c0 + alpha * s : c0;
    }
  if (form == 0)
    general_addition<Backend::GPU, Device::GPU, T>(uplo, op, alpha, a, beta, c);
  else
    general_addition<Backend::GPU, Device::GPU, T>(grid, uplo, op, alpha, a, beta, c);
  long bad = 0;
  for (SizeType j = 0; j < n; ++j)
    for (SizeType i = 0; i < m; ++i)
      if (!(c(LocalElementIndex(i, j)) == want[(size_t) (i + j * m)]))
        ++bad;
  std::printf("%s: %ld of %ld elements differ\n", name, bad, (long) (m * n));
  if (bad != 0)
    ++failures;
}

template <class T>
static void run_complete(comm::CommunicatorGrid& grid, blas::Uplo uplo, bool conjugate, int form, const char* name) {
  Matrix<T, Device::CPU> a(LocalElementSize(m, m), TileElementSize(nb, nb));
  const T other = T(100);
  std::vector<T> want((size_t) (m * m));
  for (SizeType j = 0; j < m; ++j)
    for (SizeType i = 0; i < m; ++i) {
      const bool stored = in_part(uplo, i, j);
      const T v = stored ? make<T>(i, j, 2) : make<T>(j, i, 2);
      a(LocalElementIndex(i, j)) = stored ? v : other;
      T w = stored ? v : (conjugate ? conj_of<T>(v) : v);
      if constexpr (!std::is_floating_point_v<T>)
        if (conjugate && i == j)
          w = T(w.real(), 0);
      want[(size_t) (i + j * m)] = w;
    }
  if (form == 0)
    hermitian_complete<Backend::GPU, Device::GPU, T>(uplo, conjugate, a);
  else
    hermitian_complete<Backend::GPU, Device::GPU, T>(grid, uplo, conjugate, a);
  long bad = 0;
  for (SizeType j = 0; j < m; ++j)
    for (SizeType i = 0; i < m; ++i)
      if (!(a(LocalElementIndex(i, j)) == want[(size_t) (i + j * m)]))
        ++bad;
  std::printf("%s: %ld of %ld elements differ\n", name, bad, (long) (m * m));
  if (bad != 0)
    ++failures;
}

int main() {
  dlaf_initialize(0, nullptr, 0, nullptr);
  {
    comm::CommunicatorGrid grid = comm::CommunicatorGrid::single();
    using C = std::complex<float>;
    using Z = std::complex<double>;
    run_addition<float>(grid, blas::Uplo::General, blas::Op::Trans, 0, "float addition G T");
    run_addition<double>(grid, blas::Uplo::Lower, blas::Op::NoTrans, 1, "double addition L N (grid overload)");
    run_addition<C>(grid, blas::Uplo::Upper, blas::Op::ConjTrans, 0, "complex<float> addition U C");
    run_addition<Z>(grid, blas::Uplo::General, blas::Op::ConjTrans, 1, "complex<double> addition G C (grid overload)");
    run_complete<float>(grid, blas::Uplo::Lower, false, 0, "float complete L symmetric");
    run_complete<double>(grid, blas::Uplo::Upper, true, 1, "double complete U Hermitian (grid overload)");
    run_complete<C>(grid, blas::Uplo::Lower, true, 1, "complex<float> complete L Hermitian (grid overload)");
    run_complete<Z>(grid, blas::Uplo::Upper, false, 0, "complex<double> complete U symmetric");
    run_complete<Z>(grid, blas::Uplo::Lower, true, 0, "complex<double> complete L Hermitian");
  }
  dlaf_finalize();
  if (failures == 0)
    std::printf("CPP_GENERAL_ADDITION_TEST OK\n");
  return failures == 0 ? 0 : 1;
}
