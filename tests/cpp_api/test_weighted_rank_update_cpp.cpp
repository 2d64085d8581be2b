// test_weighted_rank_update_cpp.cpp -- dlaf::hermitian_weighted_rank_k_update, hermitian_function and hermitian_power of
// the facade include/dlaf_mi355x/dlaf.hpp on one process.  The update: one case per element type at n = 150, k = 90,
// nb = 64 -- float L / NoTrans, double U / Trans (through the grid overload), complex<float> L / ConjTrans,
// complex<double> U / NoTrans -- against loop products in this program; operands and weights are small integers (zeros
// and negative weights among them), so the comparison is for equality; the other triangle must keep its value, the
// diagonal of a complex C -- imaginary part 7 on entry -- must come back real.  The functions: on the miniapps' random
// Hermitian positive definite matrix (set_random_hermitian_positive_definite: elements in [-1, 1], 2 n more on the diagonal,
// so every eigenvalue lies within Gershgorin's [n, 3 n + 1]), f(A) with f = 1 is the identity (every eigenpair,
// sum z z^H = I) and hermitian_power with exponent 1 gives A back, within the bound of tests/test_gpu_hermitian_function.py,
// n u (max |f| + L lambda_max): n u for f = 1 (L = 0) and n u 2 (3 n + 1) for f = x, u = 1.2e-16.  One process, one GPU.
#include <cmath>
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
  if constexpr (std::is_same_v<T, float> || std::is_same_v<T, double>)
    return (T) small_int(i, j, salt);
  else
    return T((BaseType<T>) small_int(i, j, salt), (BaseType<T>) small_int(j, i, salt + 2));
}
template <class T>
static T conj_of(const T& v) {
  if constexpr (std::is_same_v<T, float> || std::is_same_v<T, double>)
    return v;
  else
    return std::conj(v);
}

template <class T>
static void run_update(comm::CommunicatorGrid& grid, blas::Uplo uplo, blas::Op op, int form, const char* name) {
  using R = BaseType<T>;
  constexpr bool cx = !(std::is_same_v<T, float> || std::is_same_v<T, double>);
  const bool tn = op == blas::Op::NoTrans, lower = uplo == blas::Uplo::Lower;
  const SizeType ar = tn ? n : k, ac = tn ? k : n;
  Matrix<T, Device::CPU> a(LocalElementSize(ar, ac), TileElementSize(nb, nb));
  Matrix<T, Device::CPU> c(LocalElementSize(n, n), TileElementSize(nb, nb));
  for (SizeType j = 0; j < ac; ++j)
    for (SizeType i = 0; i < ar; ++i)
      a(LocalElementIndex(i, j)) = make<T>(i, j, 1);
  std::vector<R> d((size_t) k);
  for (SizeType l = 0; l < k; ++l)
    d[(size_t) l] = (R) ((int) ((5 * l + 2) % 7) - 3);
  auto at = [&](SizeType i, SizeType l) { return tn ? a(LocalElementIndex(i, l)) : conj_of<T>(a(LocalElementIndex(l, i))); };
  const T untouched = make<T>(2, 1, 6) + T(100);
  const R alpha = 2, beta = -3;
  std::vector<T> want((size_t) (n * n));
  for (SizeType j = 0; j < n; ++j)
    for (SizeType i = 0; i < n; ++i) {
      const bool in = lower ? i >= j : i <= j;
      T c0 = make<T>(i, j, 3);
      if constexpr (cx)
        if (i == j)
          c0 = T(c0.real(), 7);
      c(LocalElementIndex(i, j)) = in ? c0 : untouched;
      if (!in) {
        want[(size_t) (i + j * n)] = untouched;
        continue;
      }
      if constexpr (cx)
        if (i == j)
          c0 = T(c0.real(), 0);
      T s = T(0);
      for (SizeType l = 0; l < k; ++l)
        s += at(i, l) * T(d[(size_t) l]) * conj_of<T>(at(j, l));
      want[(size_t) (i + j * n)] = T(alpha) * s + T(beta) * c0;
    }
  if (form == 0)
    hermitian_weighted_rank_k_update<Backend::GPU, Device::GPU, T>(uplo, op, alpha, a, d.data(), beta, c);
  else
    hermitian_weighted_rank_k_update<Backend::GPU, Device::GPU, T>(grid, uplo, op, alpha, a, d.data(), beta, c);
  long bad = 0;
  for (SizeType j = 0; j < n; ++j)
    for (SizeType i = 0; i < n; ++i)
      if (!(c(LocalElementIndex(i, j)) == want[(size_t) (i + j * n)]))
        ++bad;
  std::printf("%s: %ld of %ld elements differ\n", name, bad, (long) (n * n));
  if (bad != 0)
    ++failures;
}

static void run_functions(comm::CommunicatorGrid& grid) {
  Matrix<double, Device::CPU> a(LocalElementSize(n, n), TileElementSize(nb, nb));
  Matrix<double, Device::CPU> a0(LocalElementSize(n, n), TileElementSize(nb, nb));
  matrix::util::set_random_hermitian_positive_definite(grid, a0);
  auto fill = [&] {
    for (SizeType j = 0; j < n; ++j)
      for (SizeType i = 0; i < n; ++i)
        a(LocalElementIndex(i, j)) = i >= j ? a0(LocalElementIndex(i, j)) : -77.0;
  };
  std::vector<double> w((size_t) n);
  // f = 1 on every eigenpair: the identity
  fill();
  SizeType sel[2] = {-1, -1};
  const SpectralWeights<double> ones = [](SizeType, const double*, SizeType b, SizeType e, double* g) {
    for (SizeType j = b; j < e; ++j)
      g[j] = 1.0;
  };
  int r = hermitian_function<Backend::GPU, Device::GPU, double>(grid, blas::Uplo::Lower, a, w.data(), ones, {}, sel);
  double worst = 0;
  bool other = true;
  for (SizeType j = 0; j < n; ++j)
    for (SizeType i = 0; i < n; ++i) {
      if (i >= j)
        worst = std::fmax(worst, std::fabs(a(LocalElementIndex(i, j)) - (i == j ? 1.0 : 0.0)));
      else
        other = other && a(LocalElementIndex(i, j)) == -77.0;
    }
  std::printf("hermitian_function f = 1: status %d, selected [%ld, %ld), max |P - I| %.3e, other triangle %s\n", r,
              (long) sel[0], (long) sel[1], worst, other ? "kept" : "CHANGED");
  if (r != 0 || sel[0] != 0 || sel[1] != n || !(worst <= n * 1.2e-16) || !other)
    ++failures;
  // exponent 1: A itself
  fill();
  SizeType dropped = -1;
  r = hermitian_power<Backend::GPU, Device::GPU, double>(grid, blas::Uplo::Lower, a, w.data(), 1.0, 0.0, &dropped);
  worst = 0;
  for (SizeType j = 0; j < n; ++j)
    for (SizeType i = j; i < n; ++i)
      worst = std::fmax(worst, std::fabs(a(LocalElementIndex(i, j)) - a0(LocalElementIndex(i, j))));
  std::printf("hermitian_power exponent 1: status %d, dropped %ld, max |A^1 - A| %.3e\n", r, (long) dropped, worst);
  if (r != 0 || dropped != 0 || !(worst <= n * 1.2e-16 * 2.0 * (3.0 * n + 1.0)))
    ++failures;
}

int main() {
  dlaf_initialize(0, nullptr, 0, nullptr);
  {
    comm::CommunicatorGrid grid = comm::CommunicatorGrid::single();
    run_update<float>(grid, blas::Uplo::Lower, blas::Op::NoTrans, 0, "float weighted rank-k L N");
    run_update<double>(grid, blas::Uplo::Upper, blas::Op::Trans, 1, "double weighted rank-k U T (grid overload)");
    run_update<std::complex<float>>(grid, blas::Uplo::Lower, blas::Op::ConjTrans, 0, "complex<float> weighted rank-k L C");
    run_update<std::complex<double>>(grid, blas::Uplo::Upper, blas::Op::NoTrans, 1, "complex<double> weighted rank-k U N");
    run_functions(grid);
  }
  dlaf_finalize();
  if (failures == 0)
    std::printf("CPP_WEIGHTED_RANK_UPDATE_TEST OK\n");
  return failures == 0 ? 0 : 1;
}
