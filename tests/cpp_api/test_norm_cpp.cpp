// test_norm_cpp.cpp -- dlaf::auxiliary::max_norm and dlaf::auxiliary::norm of the facade include/dlaf_mi355x/dlaf.hpp
// at n = 333, nb = 100 (double and complex<float>): every overload must return what the C entry it stands for returns,
// on host matrices and on a device-resident one, and max_norm must be the largest modulus of the part it names.
// One process, one GPU.
#include <cmath>
#include <complex>
#include <cstdio>

#include <dlaf_mi355x/dlaf.hpp>

using namespace dlaf;

static int failures = 0;
static void expect(const char* what, double got, double want) {
  if (!(got == want)) {
    std::fprintf(stderr, "%s: %.17g != %.17g\n", what, got, want);
    ++failures;
  }
}

constexpr SizeType n = 333, nb = 100;

static double el(SizeType i, SizeType j) {
  return std::cos(1.0 + 3.0 * (double) i + 0.37 * (double) j) * (1.0 + (double) ((3 * i + j) % 7));
}

template <class T>
static T make(SizeType i, SizeType j) {
  if constexpr (std::is_same_v<T, double>)
    return el(i, j);
  else
    return T((float) el(i, j), (float) el(j, i + 1));
}

template <class T>
static int run(comm::CommunicatorGrid& grid, const char* name) {
  using R = BaseType<T>;
  Matrix<T, Device::CPU> a(LocalElementSize(n, n), TileElementSize(nb, nb));
  R max_all = 0, max_lower = 0, max_upper = 0;
  for (SizeType j = 0; j < n; ++j)
    for (SizeType i = 0; i < n; ++i) {
      const T v = make<T>(i, j);
      a(LocalElementIndex(i, j)) = v;
      const R m = std::abs(v);
      max_all = std::max(max_all, m);
      if (i >= j)
        max_lower = std::max(max_lower, m);
      if (i <= j)
        max_upper = std::max(max_upper, m);
    }
  const DLAF_descriptor desc{(int) n, (int) n, (int) nb, (int) nb, 0, 0, 0, 0, (int) a.ld()};
  const int ctx = grid.context();
  auto c_general = [&](char norm) {
    double v = -1;
    int r;
    if constexpr (std::is_same_v<T, double>)
      r = dlaf_mi355x_general_norm_d(ctx, norm, a.ptr(), desc, &v);
    else
      r = dlaf_mi355x_general_norm_c(ctx, norm, a.ptr(), desc, &v);
    return r == 0 ? v : -1.0;
  };
  auto c_hermitian = [&](char norm, char uplo) {
    double v = -1;
    int r;
    if constexpr (std::is_same_v<T, double>)
      r = dlaf_mi355x_hermitian_norm_d(ctx, norm, uplo, a.ptr(), desc, &v);
    else
      r = dlaf_mi355x_hermitian_norm_c(ctx, norm, uplo, a.ptr(), desc, &v);
    return r == 0 ? v : -1.0;
  };
  auto c_triangular = [&](char norm, char uplo, char diag) {
    double v = -1;
    int r;
    if constexpr (std::is_same_v<T, double>)
      r = dlaf_mi355x_triangular_norm_d(ctx, norm, uplo, diag, a.ptr(), desc, &v);
    else
      r = dlaf_mi355x_triangular_norm_c(ctx, norm, uplo, diag, a.ptr(), desc, &v);
    return r == 0 ? v : -1.0;
  };
  const comm::Index2D rank(0, 0);
  // max_norm with the reference's signature; the complex modulus of the device may differ from std::abs in the last
  // place, so the complex type is compared with the C entry and the real one with the loop above as well
  expect("max_norm General", auxiliary::max_norm<Backend::GPU, Device::CPU, T>(grid, rank, blas::Uplo::General, a),
         c_general('M'));
  expect("max_norm Lower", auxiliary::max_norm<Backend::GPU, Device::CPU, T>(grid, rank, blas::Uplo::Lower, a),
         c_triangular('M', 'L', 'N'));
  expect("max_norm Upper", auxiliary::max_norm<Backend::GPU, Device::CPU, T>(grid, rank, blas::Uplo::Upper, a),
         c_triangular('M', 'U', 'N'));
  if constexpr (std::is_same_v<T, double>) {
    expect("max_norm General against the loop", c_general('M'), max_all);
    expect("max_norm Lower against the loop", c_triangular('M', 'L', 'N'), max_lower);
    expect("max_norm Upper against the loop", c_triangular('M', 'U', 'N'), max_upper);
  }
  const lapack::Norm norms[4] = {lapack::Norm::Max, lapack::Norm::One, lapack::Norm::Inf, lapack::Norm::Fro};
  for (lapack::Norm nm : norms) {
    const char c = (char) nm;
    expect("norm general", auxiliary::norm<Backend::GPU, T>(grid, nm, a), c_general(c));
    for (blas::Uplo uplo : {blas::Uplo::Lower, blas::Uplo::Upper}) {
      expect("norm hermitian", auxiliary::norm<Backend::GPU, T>(grid, nm, uplo, a), c_hermitian(c, (char) uplo));
      for (blas::Diag diag : {blas::Diag::NonUnit, blas::Diag::Unit})
        expect("norm triangular", auxiliary::norm<Backend::GPU, T>(grid, nm, uplo, diag, a),
               c_triangular(c, (char) uplo, (char) diag));
      // the same triangle resident on the device
      {
        matrix::MatrixMirror<T, Device::GPU, Device::CPU> mirror(grid, a, uplo);
        expect("norm hermitian, resident", auxiliary::norm<Backend::GPU, T>(grid, nm, uplo, mirror.get()),
               c_hermitian(c, (char) uplo));
        expect("norm triangular, resident",
               auxiliary::norm<Backend::GPU, T>(grid, nm, uplo, blas::Diag::Unit, mirror.get()),
               c_triangular(c, (char) uplo, 'U'));
        if (nm == lapack::Norm::Max)
          expect("max_norm, resident", auxiliary::max_norm<Backend::GPU, Device::GPU, T>(grid, rank, uplo, mirror.get()),
                 c_triangular('M', (char) uplo, 'N'));
      }
    }
  }
  if (c_general('M') <= 0 || c_general('F') <= c_general('M'))
    expect("norms are not plausible", c_general('F'), c_general('M'));
  std::printf("%s: max %g one %g inf %g fro %g\n", name, c_general('M'), c_general('1'), c_general('I'), c_general('F'));
  return failures;
}

int main() {
  dlaf_initialize(0, nullptr, 0, nullptr);
  {
    comm::CommunicatorGrid grid = comm::CommunicatorGrid::single();
    run<double>(grid, "double");
    run<std::complex<float>>(grid, "complex<float>");
  }
  dlaf_finalize();
  if (failures == 0)
    std::printf("CPP_NORM_TEST OK\n");
  return failures == 0 ? 0 : 1;
}
