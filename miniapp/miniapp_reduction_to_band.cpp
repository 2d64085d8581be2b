// miniapp_reduction_to_band.cpp -- the reference's miniapp/miniapp_reduction_to_band.cpp for the MI355X library on
// the C++ facade: same options (--matrix-size --block-size --band-size --grid-rows --grid-cols --nruns --nwarmups --type
// --csv), same timed window (the matrix resident on the device, barrier - reduction_to_band - barrier, :141-160), same
// flop model (add_mul = 2/3 n^3 - n^2 nb, :163-168), same result lines; as upstream, --check-result is accepted and
// not implemented (:84-87) -- parity is covered by tests/test_gpu_red2band.py.  Input as upstream: a random Hermitian
// matrix (set_random_hermitian, :120-126).
//   g++ -std=c++17 -O2 -I include miniapp/miniapp_reduction_to_band.cpp -L dla_future_amd/lib -ldlaf_mi355x -o miniapp_reduction_to_band
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
  SizeType b = -1;  // --band-size (default: the block size, miniapp_reduction_to_band.cpp:62-63)
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
    else if (a == "--band-size")
      o.b = std::stoll(val());
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
                         "miniapp_reduction_to_band --matrix-size N --block-size NB [--band-size B] [--grid-rows R "
                         "--grid-cols C] [--nruns K] [--nwarmups W] [--type s|d|c|z] [--uplo L|U] "
                         "[--check-result none|last|all] [--csv]",
                         own);
  if (o.b < 0)
    o.b = o.mb;
  if (o.b < 2 || o.mb % o.b != 0) {
    std::cerr << "band size " << o.b << " must be >= 2 and divide the block size " << o.mb << std::endl;
    std::exit(2);
  }
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

  Matrix<T, Device::GPU> matrix_ref(comm_grid, dist, blas::Uplo::Lower);
  {
    Matrix<T, Device::CPU> host(dist);
    // set_random_hermitian = the generator of set_random_hermitian_positive_definite without the 2 n on the diagonal
    // (util_matrix.h:460-462, :499-501)
    matrix::util::set_random_hermitian_positive_definite(comm_grid, host);
    const LocalElementSize ls = dist.local_size();
    for (SizeType j = 0; j < ls.cols(); ++j)
      for (SizeType i = 0; i < ls.rows(); ++i) {
        const GlobalElementIndex g = dist.global_element_index(LocalElementIndex(i, j));
        if (g.row() == g.col())
          host(LocalElementIndex(i, j)) -= T(2 * (Base) opts.m);
      }
    dlaf_mi355x_matrix_upload(matrix_ref.handle(), host.ptr(), (int) host.ld());
  }
  Matrix<T, Device::GPU> matrix(comm_grid, dist, blas::Uplo::Lower);

  for (int64_t run_index = -opts.nwarmups; run_index < opts.nruns; ++run_index) {
    if (0 == world_rank && run_index >= 0)
      std::cout << "[" << run_index << "]" << std::endl;
    dlaf_mi355x_matrix_copy(matrix.handle(), matrix_ref.handle());  // a fresh copy outside the timer (:133-139)
    comm_grid.wait_all_communicators();
    const auto t0 = std::chrono::steady_clock::now();
    auto taus = eigensolver::internal::reduction_to_band<Backend::GPU, T>(comm_grid, matrix, opts.b);
    comm_grid.wait_all_communicators();
    const double elapsed_time = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    (void) taus;

    const double n = (double) opts.m, nbd = (double) opts.mb;
    const double add_mul = 2. / 3. * n * n * n - n * n * nbd;
    const double gigaflops = miniapp::total_ops<T>(add_mul) / elapsed_time / 1e9;
    if (0 == world_rank && run_index >= 0) {
      std::cout << "[" << run_index << "] " << elapsed_time << "s " << gigaflops << "GFlop/s " << opts.type << " ("
                << opts.m << ", " << opts.m << ") (" << opts.mb << ", " << opts.mb << ") " << opts.b << " ("
                << comm_grid.size().rows() << ", " << comm_grid.size().cols() << ") 1 GPU" << std::endl;
      if (opts.csv)
        std::cout << "CSVData-2, run, " << run_index << ", time, " << elapsed_time << ", GFlops, " << gigaflops
                  << ", type, " << opts.type << ", matrixsize, " << opts.m << ", blocksize, " << opts.mb
                  << ", band_size, " << opts.b << ", comm_rows, " << comm_grid.size().rows() << ", comm_cols, "
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
