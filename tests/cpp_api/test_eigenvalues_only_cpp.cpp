// test_eigenvalues_only_cpp.cpp -- the eigenvalues-only functions and the by-value overloads of the facade
// include/dlaf_mi355x/dlaf.hpp, once each: n = 34, nb = 8, a diagonally dominant matrix whose eigenvalues lie within
// Gershgorin discs of radius < 0.5 around 1, 3, 5, ... (disjoint: one eigenvalue each).  hermitian_eigenvalues must agree
// with hermitian_eigensolver's eigenvalues within n error max|w| and write its range alone; the by-value overloads must
// return the index range the discs dictate and write what the index-range overload writes, bit for bit.  One process,
// one GPU.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include <dlaf_mi355x/dlaf.hpp>

using namespace dlaf;

static int failures = 0;
static void fail(const char* what, double got, double bar) {
  std::fprintf(stderr, "%s: %g vs %g\n", what, got, bar);
  ++failures;
}

constexpr SizeType n = 34, nb = 8;
constexpr double sentinel = -3.25;
constexpr double error = 2 * std::numeric_limits<double>::epsilon();  // TypeUtilities<double>::error

static double el_a(SizeType i, SizeType j) {
  return i == j ? 1.0 + 2.0 * (double) i : 0.4 / (double) n * std::cos(1.0 + (double) std::min(i, j) + 0.37 * (double) std::max(i, j));
}
static double el_b(SizeType i, SizeType j) {
  return i == j ? 1.0 : 0.0;  // the identity: the generalized problem keeps the spectrum of A
}

using M = Matrix<double, Device::CPU>;

int main() {
  dlaf::initialize();
  {
    comm::CommunicatorGrid grid = comm::CommunicatorGrid::single();
    auto set_a = [](const GlobalElementIndex& x) { return el_a(x.row(), x.col()); };
    auto set_b = [](const GlobalElementIndex& x) { return el_b(x.row(), x.col()); };
    auto set_z = [](const GlobalElementIndex&) { return sentinel; };
    const LocalElementSize sz(n, n);
    const TileElementSize ts(nb, nb);
    std::vector<double> w_ref, w, wg;
    {
      M a(sz, ts), z(sz, ts);
      matrix::util::set(a, set_a);
      matrix::util::set(z, set_z);
      hermitian_eigensolver<Backend::GPU, double>(grid, blas::Uplo::Lower, a, w_ref, z);
    }
    const double bar = n * error * std::abs(w_ref.back());
    {
      M a(sz, ts), b(sz, ts);
      matrix::util::set(a, set_a);
      matrix::util::set(b, set_b);
      hermitian_eigenvalues<Backend::GPU, double>(grid, blas::Uplo::Lower, a, w);
      hermitian_generalized_eigenvalues<Backend::GPU, double>(grid, blas::Uplo::Lower, a, b, wg);
      for (SizeType i = 0; i < n; ++i) {
        if (a(LocalElementIndex(i, i)) != el_a(i, i))
          fail("hermitian_eigenvalues wrote to its matrix", a(LocalElementIndex(i, i)), el_a(i, i));
        if (!(std::abs(w[(size_t) i] - w_ref[(size_t) i]) <= bar))
          fail("hermitian_eigenvalues", w[(size_t) i], w_ref[(size_t) i]);
        if (!(std::abs(wg[(size_t) i] - w_ref[(size_t) i]) <= bar))
          fail("hermitian_generalized_eigenvalues", wg[(size_t) i], w_ref[(size_t) i]);
      }
      std::vector<double> part((size_t) n, sentinel);
      hermitian_eigenvalues<Backend::GPU, double>(grid, blas::Uplo::Lower, a, part, 5, 20);
      for (SizeType i = 0; i < n; ++i)
        if (part[(size_t) i] != (i >= 5 && i < 20 ? w[(size_t) i] : sentinel))
          fail("hermitian_eigenvalues [5, 20)", part[(size_t) i], w[(size_t) i]);
    }
    // (6, 30.5]: the eigenvalues around 7, 9, ..., 29: indices [3, 15)
    for (int generalized = 0; generalized < 2; ++generalized) {
      M a(sz, ts), b(sz, ts), z(sz, ts), a2(sz, ts), b2(sz, ts), z2(sz, ts);
      for (M* m : {&a, &a2})
        matrix::util::set(*m, set_a);
      for (M* m : {&b, &b2})
        matrix::util::set(*m, set_b);
      for (M* m : {&z, &z2})
        matrix::util::set(*m, set_z);
      std::vector<double> wv, wi;
      std::pair<SizeType, SizeType> found;
      if (generalized) {
        found = hermitian_generalized_eigensolver<Backend::GPU, double>(grid, blas::Uplo::Lower, a, b, wv, z,
                                                                        EigenvaluesValue<double>{6.0, 30.5});
        hermitian_generalized_eigensolver<Backend::GPU, double>(grid, blas::Uplo::Lower, a2, b2, wi, z2, 3, 15);
      }
      else {
        found = hermitian_eigensolver<Backend::GPU, double>(grid, blas::Uplo::Lower, a, wv, z, EigenvaluesValue<double>{6.0, 30.5});
        hermitian_eigensolver<Backend::GPU, double>(grid, blas::Uplo::Lower, a2, wi, z2, 3, 15);
      }
      if (found.first != 3 || found.second != 15)
        fail("by value: index range", (double) found.first, (double) found.second);
      for (SizeType j = 0; j < n; ++j) {
        if (wv[(size_t) j] != wi[(size_t) j])
          fail("by value: eigenvalues differ from the index-range overload", wv[(size_t) j], wi[(size_t) j]);
        for (SizeType i = 0; i < n; ++i) {
          if (z(LocalElementIndex(i, j)) != z2(LocalElementIndex(i, j)))
            fail("by value: eigenvectors differ from the index-range overload", z(LocalElementIndex(i, j)),
                 z2(LocalElementIndex(i, j)));
          if ((j < 3 || j >= 15) && z(LocalElementIndex(i, j)) != sentinel)
            fail("by value: element outside the wanted columns was written", z(LocalElementIndex(i, j)), sentinel);
        }
      }
    }
  }
  dlaf::finalize();
  std::printf("CPP_EIGENVALUES_ONLY_TEST %s\n", failures ? "FAILED" : "OK");
  return failures ? 1 : 0;
}
