// miniapp_gen_to_std.cpp -- the reference's miniapp/miniapp_gen_to_std.cpp for the MI355X library on the C++ facade:
// same options (--matrix-size --block-size --grid-rows --grid-cols --nruns --nwarmups --type --uplo --csv), same
// timed window (both operands resident on the device, barrier - generalized_to_standard - barrier, :119-140),
// same flop model (n^3/2 adds + n^3/2 muls, :147-151), same result lines; as upstream, --check-result is accepted
// and not implemented (:65-68) -- parity is covered by tests/test_gpu_gen_to_std.py.  Inputs as upstream: A random
// Hermitian, the "factor" = the uplo triangle of a random Hermitian positive definite matrix (:97-110).
//   g++ -std=c++17 -O2 -I include miniapp/miniapp_gen_to_std.cpp -L dla_future_amd/lib -ldlaf_mi355x -o miniapp_gen_to_std
#include <chrono>
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
                         "miniapp_gen_to_std --matrix-size N --block-size NB [--grid-rows R --grid-cols C] [--nruns K] "
                         "[--nwarmups W] [--type s|d|c|z] [--uplo L|U] [--check-result none|last|all] [--csv]",
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

  // reference inputs on the host, then resident copies on the device
  Matrix<T, Device::GPU> matrix_a_ref(comm_grid, dist, opts.uplo), matrix_b_ref(comm_grid, dist, opts.uplo);
  {
    Matrix<T, Device::CPU> host(dist);
    matrix::util::set_random_hermitian_positive_definite(comm_grid, host);
    dlaf_mi355x_matrix_upload(matrix_b_ref.handle(), host.ptr(), (int) host.ld());
    // set_random_hermitian = the same generator without the 2 n on the diagonal (util_matrix.h:460-462, :499-501)
    const LocalElementSize ls = dist.local_size();
    for (SizeType j = 0; j < ls.cols(); ++j)
      for (SizeType i = 0; i < ls.rows(); ++i) {
        const GlobalElementIndex g = dist.global_element_index(LocalElementIndex(i, j));
        if (g.row() == g.col())
          host(LocalElementIndex(i, j)) -= T(2 * (Base) opts.m);
      }
    dlaf_mi355x_matrix_upload(matrix_a_ref.handle(), host.ptr(), (int) host.ld());
  }
  Matrix<T, Device::GPU> matrix_a(comm_grid, dist, opts.uplo), matrix_b(comm_grid, dist, opts.uplo);

  for (int64_t run_index = -opts.nwarmups; run_index < opts.nruns; ++run_index) {
    if (0 == world_rank && run_index >= 0)
      std::cout << "[" << run_index << "]" << std::endl;
    dlaf_mi355x_matrix_copy(matrix_a.handle(), matrix_a_ref.handle());  // fresh copies outside the timer (:112-117)
    dlaf_mi355x_matrix_copy(matrix_b.handle(), matrix_b_ref.handle());
    comm_grid.wait_all_communicators();
    const auto t0 = std::chrono::steady_clock::now();
    eigensolver::internal::generalized_to_standard<Backend::GPU, T>(comm_grid, opts.uplo, matrix_a, matrix_b);
    comm_grid.wait_all_communicators();
    const double elapsed_time = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

    const double n = (double) opts.m;
    const double add_mul = n * n * n / 2;
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
  }
  if (opts.check != "none" && world_rank == 0)
    std::cerr << "Warning! At the moment result checking it is not implemented." << std::endl;
}

int main(int argc, char** argv) {
  const Options opts = parse(argc, argv);
  return miniapp::run_main(argc, argv, opts, true, [&opts](auto t, comm::CommunicatorGrid& comm_grid, int world_rank, int) {
    run<decltype(t)>(opts, comm_grid, world_rank);
  });
}
