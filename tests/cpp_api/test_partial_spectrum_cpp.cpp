// test_partial_spectrum_cpp.cpp -- the partial-spectrum overloads of hermitian_eigensolver and
// hermitian_generalized_eigensolver of the facade include/dlaf_mi355x/dlaf.hpp, once each: n = 34, nb = 8, eigenvalue
// indices [3, 20).  The wanted columns must satisfy test_eigensolver_correctness.h's residual and orthogonality bars
// (m = n) against the input, every other element of the eigenvector matrix must stay as it was.  One process, one GPU.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include <dlaf_mi355x/dlaf.hpp>

using namespace dlaf;

static int failures = 0;
static void fail(const char* what, double got, double bar) {
  std::fprintf(stderr, "%s: %g > %g\n", what, got, bar);
  ++failures;
}

constexpr SizeType n = 34, nb = 8, ib = 3, ie = 20;
constexpr double sentinel = -3.25;
constexpr double error = 2 * std::numeric_limits<double>::epsilon();  // TypeUtilities<double>::error

static double el_a(SizeType i, SizeType j) {
  return std::cos(1.0 + 3.0 * (double) std::min(i, j) + 0.37 * (double) std::max(i, j)) + (i == j ? 0.5 * (double) i : 0.0);
}
static double el_b(SizeType i, SizeType j) {
  return std::exp2(-(double) std::abs((double) (i - j))) + (i == j ? 2.0 : 0.0);  // strictly diagonally dominant: HPD
}

// columns [ib, ie) of z: Z^H B Z == I and A Z == B Z Lambda (B = I for the standard problem); the others untouched
static void check(const char* what, Matrix<double, Device::CPU>& z, const std::vector<double>& w, bool generalized) {
  if ((SizeType) w.size() != n)
    fail(what, (double) w.size(), (double) n);
  for (SizeType i = 0; i + 1 < n; ++i)
    if (!(w[(size_t) i] <= w[(size_t) i + 1]))
      fail("eigenvalues not ascending", w[(size_t) i], w[(size_t) i + 1]);
  for (SizeType j = 0; j < n; ++j)
    for (SizeType i = 0; i < n; ++i)
      if ((j < ib || j >= ie) && z(LocalElementIndex(i, j)) != sentinel)
        fail("element outside the wanted columns was written", z(LocalElementIndex(i, j)), sentinel);
  double bmax = 1, amax = 0, wmax = 0;
  for (SizeType j = 0; j < n; ++j)
    for (SizeType i = 0; i < n; ++i) {
      amax = std::max(amax, std::abs(el_a(i, j)));
      if (generalized)
        bmax = std::max(bmax, std::abs(el_b(i, j)));
    }
  for (double x : w)
    wmax = std::max(wmax, std::abs(x));
  // test_eigensolver_correctness.h: 10 m error and 2 m error; test_gen_eigensolver.cpp's bars for the generalized problem
  const double obar = 10 * n * error * bmax;
  const double rbar = generalized ? 10 * n * error * std::max(1.0, amax * wmax) : 2 * n * error;
  std::vector<double> bz((size_t) n), az((size_t) n);
  for (SizeType j = ib; j < ie; ++j) {
    for (SizeType i = 0; i < n; ++i) {
      double sa = 0, sb = 0;
      for (SizeType k = 0; k < n; ++k) {
        sa += el_a(i, k) * z(LocalElementIndex(k, j));
        sb += (generalized ? el_b(i, k) : (i == k ? 1.0 : 0.0)) * z(LocalElementIndex(k, j));
      }
      az[(size_t) i] = sa;
      bz[(size_t) i] = sb;
    }
    for (SizeType i = 0; i < n; ++i) {
      const double el = bz[(size_t) i] * w[(size_t) j], diff = std::abs(az[(size_t) i] - el);
      if (!(diff <= rbar || diff <= rbar * std::abs(el)))
        fail("residual", diff, rbar);
    }
    for (SizeType c = ib; c < ie; ++c) {
      double g = 0;
      for (SizeType i = 0; i < n; ++i)
        g += z(LocalElementIndex(i, c)) * bz[(size_t) i];
      const double d = std::abs(g - (c == j ? 1.0 : 0.0));
      if (!(d <= obar))
        fail("orthogonality", d, obar);
    }
  }
}

int main() {
  dlaf::initialize();
  {
    comm::CommunicatorGrid grid = comm::CommunicatorGrid::single();
    auto set_a = [](const GlobalElementIndex& x) { return el_a(x.row(), x.col()); };
    auto set_b = [](const GlobalElementIndex& x) { return el_b(x.row(), x.col()); };
    auto set_z = [](const GlobalElementIndex&) { return sentinel; };
    std::vector<double> w;
    {
      Matrix<double, Device::CPU> a(LocalElementSize(n, n), TileElementSize(nb, nb)), z(LocalElementSize(n, n), TileElementSize(nb, nb));
      matrix::util::set(a, set_a);
      matrix::util::set(z, set_z);
      hermitian_eigensolver<Backend::GPU, double>(grid, blas::Uplo::Lower, a, w, z, ib, ie);
      check("hermitian_eigensolver", z, w, false);
    }
    {
      Matrix<double, Device::CPU> a(LocalElementSize(n, n), TileElementSize(nb, nb)), b(LocalElementSize(n, n), TileElementSize(nb, nb)),
          z(LocalElementSize(n, n), TileElementSize(nb, nb));
      matrix::util::set(a, set_a);
      matrix::util::set(b, set_b);
      matrix::util::set(z, set_z);
      hermitian_generalized_eigensolver<Backend::GPU, double>(grid, blas::Uplo::Lower, a, b, w, z, ib, ie);
      check("hermitian_generalized_eigensolver", z, w, true);
    }
  }
  dlaf::finalize();
  std::printf("CPP_PARTIAL_SPECTRUM_TEST %s\n", failures ? "FAILED" : "OK");
  return failures ? 1 : 0;
}
