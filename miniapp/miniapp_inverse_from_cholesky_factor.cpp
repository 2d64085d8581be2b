// miniapp_inverse_from_cholesky_factor.cpp -- inverse_from_cholesky_factor on the C++ facade, in the mould of
// miniapp_gen_to_std.cpp: same options (--matrix-size --block-size --grid-rows --grid-cols --nruns --nwarmups --type
// --uplo --check-result --csv), same timed window (the operand resident on the device, barrier - call - barrier).
// Input: the Cholesky factor of a random Hermitian positive definite matrix, factored on the device outside the timer.
// Flop model: n^3 / 3 adds + n^3 / 3 muls for the two halves together (LAPACK's counts of xTRTRI + xLAUUM).
// --check-result last | all (one-process grids): LAPACK's xPOT03 ratio on the host from the downloaded triangle and
// the generated A, against the threshold of LAPACK's test programs; on a process grid the check is not implemented.
//   g++ -std=c++17 -O2 -I include miniapp/miniapp_inverse_from_cholesky_factor.cpp -L dla_future_amd/lib -ldlaf_mi355x
#include <chrono>
#include <cmath>
#include <complex>
#include <vector>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <limits>
#include <string>

#include "miniapp_common.hpp"

using namespace dlaf;

struct Options : miniapp::CommonOptions {
  SizeType m = 4096, mb = 256;
  blas::Uplo uplo = blas::Uplo::Lower;
  std::string check = "none";
  bool csv = false;
  std::string info;
};

static Options parse(int argc, char** argv) {
  Options o;
  auto own = [&o](const std::string& a, auto& val) {
    if (a == "--matrix-size")
      o.m = std::stoll(val());
    else if (a == "--block-size")
      o.mb = std::stoll(val());
    else if (a == "--uplo")
      o.uplo = miniapp::upper_initial(val()) == 'U' ? blas::Uplo::Upper : blas::Uplo::Lower;
    else if (a == "--check-result")
      o.check = val();
    else if (a == "--csv")
      o.csv = true;
    else if (a == "--pp-info")
      o.info = val();
    else
      return false;
    return true;
  };
  miniapp::parse_options(argc, argv, o,
                         "miniapp_inverse_from_cholesky_factor --matrix-size N --block-size NB [--grid-rows R --grid-cols C] "
                         "[--nruns K] [--nwarmups W] [--type s|d|c|z] [--uplo L|U] [--check-result none|last|all] [--csv]",
                         own);
  if (o.m < 0 || o.mb < 1 || o.nwarmups < 0 || !o.valid() || (o.check != "none" && o.check != "last" && o.check != "all"))
    miniapp::invalid_option_value();
  return o;
}

template <class T>
static void run(const Options& opts, comm::CommunicatorGrid& comm_grid, int world_rank) {
  using Base = typename std::conditional<std::is_same<T, float>::value || std::is_same<T, std::complex<float>>::value,
                                         float, double>::type;
  GlobalElementSize matrix_size(opts.m, opts.m);
  TileElementSize block_size(opts.mb, opts.mb);
  matrix::Distribution dist(matrix_size, block_size, comm_grid.size(), comm_grid.rank(), comm::Index2D(0, 0));

  // the factor on the device, made once outside the timer; the host keeps A for the check
  Matrix<T, Device::GPU> factor(comm_grid, dist, opts.uplo), matrix(comm_grid, dist, opts.uplo);
  Matrix<T, Device::CPU> host(dist);
  matrix::util::set_random_hermitian_positive_definite(comm_grid, host);
  dlaf_mi355x_matrix_upload(factor.handle(), host.ptr(), (int) host.ld());
  cholesky_factorization<Backend::GPU, Device::GPU, T>(comm_grid, opts.uplo, factor);

  for (int64_t run_index = -opts.nwarmups; run_index < opts.nruns; ++run_index) {
    if (0 == world_rank && run_index >= 0)
      std::cout << "[" << run_index << "]" << std::endl;
    dlaf_mi355x_matrix_copy(matrix.handle(), factor.handle());  // a fresh copy outside the timer
    comm_grid.wait_all_communicators();
    const auto t0 = std::chrono::steady_clock::now();
    const int info = inverse_from_cholesky_factor<Backend::GPU, T>(comm_grid, opts.uplo, matrix);
    comm_grid.wait_all_communicators();
    const double elapsed_time = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (info != 0) {
      std::cerr << "inverse_from_cholesky_factor returned info " << info << std::endl;
      std::exit(1);
    }

    const double n = (double) opts.m;
    const double add_mul = n * n * n / 3;
    const double gigaflops = miniapp::total_ops<T>(add_mul) / elapsed_time / 1e9;
    if (0 == world_rank && run_index >= 0) {
      std::cout << "[" << run_index << "] " << elapsed_time << "s " << gigaflops << "GFlop/s " << opts.type
                << (char) opts.uplo << " (" << opts.m << ", " << opts.m << ") (" << opts.mb << ", " << opts.mb << ") ("
                << comm_grid.size().rows() << ", " << comm_grid.size().cols() << ") 1 GPU" << std::endl;
      if (opts.csv)
        std::cout << "CSVData-2, run, " << run_index << ", time, " << elapsed_time << ", GFlops, " << gigaflops
                  << ", type, " << opts.type << ", uplo, " << (char) opts.uplo << ", matrixsize, " << opts.m
                  << ", blocksize, " << opts.mb << ", comm_rows, " << comm_grid.size().rows() << ", comm_cols, "
                  << comm_grid.size().cols() << ", threads, 1, backend, GPU, " << opts.info << std::endl;
    }
    const bool check = opts.check == "all" || (opts.check == "last" && run_index == opts.nruns - 1);
    if (check && run_index >= 0) {
      if (comm_grid.size().rows() * comm_grid.size().cols() != 1) {
        if (world_rank == 0)
          std::cerr << "Warning! On a process grid result checking is not implemented." << std::endl;
        continue;
      }
      // X from the returned triangle, A from the generator's (Hermitian) host copy
      const SizeType m = opts.m;
      Matrix<T, Device::CPU> x(dist);
      dlaf_mi355x_matrix_download(matrix.handle(), x.ptr(), (int) x.ld());
      const bool lower = opts.uplo == blas::Uplo::Lower;
      auto herm = [&](Matrix<T, Device::CPU>& mat, SizeType i, SizeType j) -> std::complex<double> {
        const bool stored = lower ? i >= j : i <= j;
        const T v = stored ? mat(LocalElementIndex(i, j)) : mat(LocalElementIndex(j, i));
        const std::complex<double> z(v);
        return stored ? z : std::conj(z);
      };
      std::vector<std::complex<double>> xf((size_t) m * m), af((size_t) m * m);
      for (SizeType j = 0; j < m; ++j)
        for (SizeType i = 0; i < m; ++i) {
          xf[(size_t) i * m + j] = herm(x, i, j);     // row-major X
          af[(size_t) j * m + i] = herm(host, i, j);  // column-major A
        }
      // LAPACK's xPOT03 ratio ||I - A X||_1 / (n eps ||A||_1 ||X||_1) against the threshold of LAPACK's own test
      // programs (30); A and X are Hermitian, so the column sums of I - A X are the row sums of X A - I
      const double eps = std::numeric_limits<Base>::epsilon();
      double res1 = 0, a1 = 0, x1 = 0;
      for (SizeType i = 0; i < m; ++i) {
        double rsum = 0, asum = 0, xsum = 0;
        for (SizeType j = 0; j < m; ++j) {
          std::complex<double> sum = (i == j) ? -1.0 : 0.0;
          for (SizeType l = 0; l < m; ++l)
            sum += xf[(size_t) i * m + l] * af[(size_t) j * m + l];
          rsum += std::abs(sum);
          asum += std::abs(af[(size_t) i * m + j]);
          xsum += std::abs(xf[(size_t) i * m + j]);
        }
        res1 = std::max(res1, rsum);
        a1 = std::max(a1, asum);
        x1 = std::max(x1, xsum);
      }
      const double ratio = res1 / ((double) m * eps * a1 * x1);
      std::cout << "Check: ||I - A X||_1 / (n eps ||A||_1 ||X||_1) = " << ratio << (ratio <= 30.0 ? "  PASSED" : "  FAILED")
                << std::endl;
      if (!(ratio <= 30.0))
        std::exit(1);
    }
  }
}

int main(int argc, char** argv) {
  const Options opts = parse(argc, argv);
  return miniapp::run_main(argc, argv, opts, true, [&opts](auto t, comm::CommunicatorGrid& comm_grid, int world_rank, int) {
    run<decltype(t)>(opts, comm_grid, world_rank);
  });
}
