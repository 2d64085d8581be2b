// test_general_multiplication_cpp.cpp -- dlaf::multiplication::internal::generalMatrix of the facade
// include/dlaf_mi355x/dlaf.hpp on one process: NoTrans x NoTrans (double, through the reference's grid signature too)
// and ConjTrans x NoTrans (complex<double>) at m = 150, n = 70, k = 90, nb = 64, against a loop product in this
// program.  The operands are small integers, so the comparison is for equality.  One process, one GPU.
#include <complex>
#include <cstdio>
#include <vector>

#include <dlaf_mi355x/dlaf.hpp>

using namespace dlaf;

static int failures = 0;
constexpr SizeType m = 150, n = 70, k = 90, nb = 64;

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

// form: 0 local matrices with ops, 1 the grid signature (NoTrans x NoTrans)
template <class T>
static void run(comm::CommunicatorGrid& grid, blas::Op opA, int form, const char* name) {
  const bool an = opA == blas::Op::NoTrans;
  Matrix<T, Device::CPU> a(LocalElementSize(an ? m : k, an ? k : m), TileElementSize(nb, nb));
  Matrix<T, Device::CPU> b(LocalElementSize(k, n), TileElementSize(nb, nb));
  Matrix<T, Device::CPU> c(LocalElementSize(m, n), TileElementSize(nb, nb));
  for (SizeType j = 0; j < (an ? k : m); ++j)
    for (SizeType i = 0; i < (an ? m : k); ++i)
      a(LocalElementIndex(i, j)) = make<T>(i, j, 1);
  for (SizeType j = 0; j < n; ++j)
    for (SizeType i = 0; i < k; ++i)
      b(LocalElementIndex(i, j)) = make<T>(i, j, 2);
  std::vector<T> want((size_t) (m * n));
  const T alpha = make<T>(1, 0, 5), beta = make<T>(0, 2, 1);
  for (SizeType j = 0; j < n; ++j)
    for (SizeType i = 0; i < m; ++i) {
      const T c0 = make<T>(i, j, 3);
      c(LocalElementIndex(i, j)) = c0;
      T sum = T(0);
      for (SizeType l = 0; l < k; ++l) {
        const T av = an ? a(LocalElementIndex(i, l)) : conj_of<T>(a(LocalElementIndex(l, i)));
        sum += av * b(LocalElementIndex(l, j));
      }
      want[(size_t) (i + j * m)] = beta * c0 + alpha * sum;
    }
  if (form == 0)
    multiplication::internal::generalMatrix<Backend::GPU, Device::GPU, T>(opA, blas::Op::NoTrans, alpha, a, b, beta, c);
  else
    multiplication::internal::generalMatrix<Backend::GPU, Device::GPU, T>(grid, alpha, a, b, beta, c);
  long bad = 0;
  for (SizeType j = 0; j < n; ++j)
    for (SizeType i = 0; i < m; ++i)
      if (!(c(LocalElementIndex(i, j)) == want[(size_t) (i + j * m)]))
        ++bad;
  std::printf("%s: %ld of %ld elements differ\n", name, bad, (long) (m * n));
  if (bad != 0)
    ++failures;
}

int main() {
  dlaf_initialize(0, nullptr, 0, nullptr);
  {
    comm::CommunicatorGrid grid = comm::CommunicatorGrid::single();
    run<double>(grid, blas::Op::NoTrans, 0, "double NN");
    run<double>(grid, blas::Op::NoTrans, 1, "double NN (grid signature)");
    run<std::complex<double>>(grid, blas::Op::ConjTrans, 0, "complex<double> CN");
  }
  dlaf_finalize();
  if (failures == 0)
    std::printf("CPP_GENERAL_MULTIPLICATION_TEST OK\n");
  return failures == 0 ? 0 : 1;
}
