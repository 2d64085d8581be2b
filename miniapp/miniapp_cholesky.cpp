// miniapp_cholesky.cpp -- the reference's headline benchmark program (miniapp/miniapp_cholesky.cpp) for the
// MI355X library, written on the C++ facade include/dlaf_mi355x/dlaf.hpp: same options, same timed window
// (device-resident matrix, barrier - factorization - barrier, :133-155), same flop model (n^3/6 adds + n^3/6
// muls, x(2+6)/2 for complex, types.h total_ops), same result lines ("[i] <t>s <GFlop/s>GFlop/s ..." and
// "CSVData-2, ..."), same check ("Max Diff / Max A", Warning above n eps, ERROR above 100 n eps, :408-443) --
// the check runs on the device.
//
//   g++ -std=c++17 -O2 -I include miniapp/miniapp_cholesky.cpp -L dla_future_amd/lib -ldlaf_mi355x -o miniapp_cholesky
//   ./miniapp_cholesky --matrix-size 65536 --block-size 1024 --nruns 3 --check-result last
// Several GPUs (one rank per GPU, LOCAL_RANK or the MPI local rank selects the device): add
//   -DDLAF_MI355X_WITH_MPI -I<mpi>/include -ldlaf_mi355x_mpi -lmpi    and   mpiexec -n 8 ... --grid-rows 2 --grid-cols 4
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
                         "miniapp_cholesky --matrix-size N --block-size NB [--grid-rows R --grid-cols C] [--nruns K] "
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

  // reference input on the host, then one resident copy of it on the device
  Matrix<T, Device::GPU> matrix_ref(comm_grid, dist, opts.uplo);
  {
    Matrix<T, Device::CPU> hermitian_pos_def(dist);
    matrix::util::set_random_hermitian_positive_definite(comm_grid, hermitian_pos_def);
    dlaf_mi355x_matrix_upload(matrix_ref.handle(), hermitian_pos_def.ptr(), (int) hermitian_pos_def.ld());
  }
  Matrix<T, Device::GPU> matrix(comm_grid, dist, opts.uplo);

  for (int64_t run_index = -opts.nwarmups; run_index < opts.nruns; ++run_index) {
    if (0 == world_rank && run_index >= 0)
      std::cout << "[" << run_index << "]" << std::endl;
    dlaf_mi355x_matrix_copy(matrix.handle(), matrix_ref.handle());  // fresh copy outside the timer (:133-141)
    comm_grid.wait_all_communicators();
    const auto t0 = std::chrono::steady_clock::now();
    cholesky_factorization<Backend::GPU, Device::GPU, T>(comm_grid, opts.uplo, matrix);
    comm_grid.wait_all_communicators();
    const double elapsed_time = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

    const double n = (double) opts.m;
    const double add_mul = n * n * n / 6;
    const double gigaflops = miniapp::total_ops<T>(add_mul) / elapsed_time / 1e9;
    if (0 == world_rank && run_index >= 0) {
      std::cout << "[" << run_index << "] " << elapsed_time << "s " << gigaflops << "GFlop/s " << opts.type
                << (char) opts.uplo << " (" << opts.m << ", " << opts.m << ") (" << opts.mb << ", " << opts.mb << ") ("
                << comm_grid.size().rows() << ", " << comm_grid.size().cols() << ") 1 GPU" << std::endl;
      if (opts.csv)
        std::cout << "CSVData-2, run, " << run_index << ", time, " << elapsed_time << ", GFlops, " << gigaflops
                  << ", type, " << opts.type << ", UpLo, " << (char) opts.uplo << ", matrixsize, " << opts.m
                  << ", blocksize, " << opts.mb << ", comm_rows, " << comm_grid.size().rows() << ", comm_cols, "
                  << comm_grid.size().cols() << ", threads, 1, backend, GPU, " << opts.info << std::endl;
    }
    if ((opts.check == "last" && run_index == opts.nruns - 1) || opts.check == "all") {
      // check_cholesky (:408-443) on the device: the original is consumed by the checker, so take a copy
      Matrix<T, Device::GPU> original(comm_grid, dist, opts.uplo);
      dlaf_mi355x_matrix_copy(original.handle(), matrix_ref.handle());
      double norm_diff = 0, norm_a = 0;
      dlaf_mi355x_cholesky_residual(original.handle(), matrix.handle(), &norm_diff, &norm_a);
      if (0 == world_rank) {
        const double eps = std::numeric_limits<Base>::epsilon();
        const double diff_ratio = norm_diff / norm_a;
        if (diff_ratio > 100 * eps * n)
          std::cout << "ERROR: ";
        else if (diff_ratio > eps * n)
          std::cout << "Warning: ";
        std::cout << "Max Diff / Max A: " << diff_ratio << std::endl;
      }
    }
  }
}

int main(int argc, char** argv) {
  const Options opts = parse(argc, argv);
  return miniapp::run_main(argc, argv, opts, true, [&opts](auto t, comm::CommunicatorGrid& comm_grid, int world_rank, int) {
    run<decltype(t)>(opts, comm_grid, world_rank);
  });
}
