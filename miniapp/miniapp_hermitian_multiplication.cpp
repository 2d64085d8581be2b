// miniapp_hermitian_multiplication.cpp -- benchmark of dlaf::hermitian_multiplication on the C++ facade of the MI355X
// library (the reference has no miniapp for it), with the options and the result line of the triangular
// multiplication's miniapp (--m --n --mb --nb --side --uplo --grid-rows --grid-cols --nruns --nwarmups --type) plus
// --beta; the variant tag is type, side, uplo (dLL, zRU, ...).  C = beta C + alpha A B (side L) / beta C + alpha B A
// (side R) with alpha = 2, A a random Hermitian matrix of which only the uplo triangle is handed over (the other one
// holds a sentinel); flop model 2 m n k (x4 complex), k = m for side L, n for side R.  The reported time is the device
// time of the sweep (dlaf_mi355x_multiplication_profile), the wall time with PCIe staging is printed next to it.
// --check-result (on one process; anything but "none") checks the last run against a product computed another way:
// C v against beta C_0 v + alpha A (B v) (side L) / beta C_0 v + alpha B (A v) (side R) for a random vector v on the host.
//   g++ -std=c++17 -O2 -I include miniapp/miniapp_hermitian_multiplication.cpp -L dla_future_amd/lib -ldlaf_mi355x -o miniapp_hermitian_multiplication
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "miniapp_common.hpp"

using namespace dlaf;

struct Options : miniapp::CommonOptions {
  SizeType m = 4096, n = 512, mb = 256, nb = 256;
  blas::Side side = blas::Side::Left;
  blas::Uplo uplo = blas::Uplo::Lower;
  double beta = 0.5;
  bool check = true;
};

static Options parse(int argc, char** argv) {
  using miniapp::upper_initial;
  Options o;
  miniapp::parse_options(argc, argv, o, nullptr, [&o](const std::string& a, auto& val) {
    if (a == "--m") o.m = std::stoll(val());
    else if (a == "--n") o.n = std::stoll(val());
    else if (a == "--mb") o.mb = std::stoll(val());
    else if (a == "--nb") o.nb = std::stoll(val());
    else if (a == "--side") o.side = upper_initial(val()) == 'R' ? blas::Side::Right : blas::Side::Left;
    else if (a == "--uplo") o.uplo = upper_initial(val()) == 'U' ? blas::Uplo::Upper : blas::Uplo::Lower;
    else if (a == "--beta") o.beta = std::stod(val());
    else if (a == "--check-result") o.check = val() != "none";
    else if (a == "--op" || a == "--diag") (void) val();
    else if (a != "--csv") return false;
    return true;
  });
  if (o.m <= 0 || o.n <= 0 || o.mb <= 0 || o.nb <= 0 || !o.valid())
    miniapp::invalid_option_value();
  return o;
}

using miniapp::Rand;

template <class T>
static void run(const Options& opts, comm::CommunicatorGrid& grid, int world_rank, int world_size) {
  using Base = decltype(std::abs(T{}));
  constexpr bool complex = !std::is_same<T, Base>::value;
  const bool left = opts.side == blas::Side::Left;
  const bool lower = opts.uplo == blas::Uplo::Lower;
  const SizeType k = left ? opts.m : opts.n;
  const SizeType kb = left ? opts.mb : opts.nb;
  matrix::Distribution da(GlobalElementSize(k, k), TileElementSize(kb, kb), grid.size(), grid.rank(), comm::Index2D(0, 0));
  matrix::Distribution db(GlobalElementSize(opts.m, opts.n), TileElementSize(opts.mb, opts.nb), grid.size(), grid.rank(), comm::Index2D(0, 0));
  Matrix<T, Device::CPU> ah(da), bh(db), c_ref(db), ch(db);
  // per-element generators seeded by the global index: every grid sees the same global matrices.  Element (i, j) of
  // the Hermitian A comes from the key of its lower-triangle twin; the diagonal is real
  auto herm = [k](SizeType i, SizeType j) {
    const SizeType r = std::max(i, j), c = std::min(i, j);
    T v = Rand<T>::make((uint64_t) r * (uint64_t) k + (uint64_t) c);
    if (r == c)
      return T(std::real(v));
    if constexpr (complex)
      return i >= j ? v : std::conj(v);
    else
      return v;
  };
  // only the uplo triangle is handed to the library; the other one holds a sentinel
  matrix::util::set(ah, [&](const GlobalElementIndex& i) {
    const bool stored = lower ? i.row() >= i.col() : i.row() <= i.col();
    return stored ? herm(i.row(), i.col()) : T(-99);
  });
  const uint64_t ncols = (uint64_t) opts.n;
  matrix::util::set(bh, [ncols](const GlobalElementIndex& i) {
    return Rand<T>::make(0x5851F42D4C957F2Dull + (uint64_t) i.row() * ncols + (uint64_t) i.col());
  });
  matrix::util::set(c_ref, [ncols](const GlobalElementIndex& i) {
    return Rand<T>::make(0x2545F4914F6CDD1Dull + (uint64_t) i.row() * ncols + (uint64_t) i.col());
  });
  const T alpha = 2.0, beta = (Base) opts.beta;
  const auto ls = db.local_size();
  for (int64_t run_index = -opts.nwarmups; run_index < opts.nruns; ++run_index) {
    if (0 == world_rank && run_index >= 0)
      std::cout << "[" << run_index << "]" << std::endl;
    for (SizeType j = 0; j < ls.cols(); ++j)
      for (SizeType i = 0; i < ls.rows(); ++i)
        ch(LocalElementIndex(i, j)) = c_ref(LocalElementIndex(i, j));
    grid.wait_all_communicators();
    const auto t0 = std::chrono::steady_clock::now();
    hermitian_multiplication<Backend::GPU, Device::CPU, T>(grid, opts.side, opts.uplo, alpha, ah, bh, beta, ch);
    grid.wait_all_communicators();
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    double ms = 0, fl = 0;
    dlaf_mi355x_multiplication_profile(&ms, &fl);
    const double elapsed_time = ms * 1e-3;
    const double add_mul = (double) opts.n * (double) opts.m * (double) k;
    const double gigaflops = miniapp::total_ops<T>(add_mul) / elapsed_time / 1e9;
    if (0 == world_rank && run_index >= 0)
      std::cout << "[" << run_index << "] " << elapsed_time << "s " << gigaflops << "GFlop/s " << opts.type
                << (char) opts.side << (char) opts.uplo << " (" << opts.m << ", " << opts.n << ") (" << opts.mb << ", "
                << opts.nb << ") (" << grid.size().rows() << ", " << grid.size().cols()
                << ") 1 GPU   [wall with PCIe staging " << wall << "s]" << std::endl;
  }
  if (!opts.check)
    return;
  if (world_size != 1) {
    if (world_rank == 0)
      std::cout << "Check skipped: --check-result needs one process" << std::endl;
    return;
  }
  // check of the last run (one process: local = global indices): C v against beta C_0 v + alpha A (B v) (side L) /
  // beta C_0 v + alpha B (A v) (side R), with the full Hermitian A regenerated on the host
  const SizeType m = opts.m, n = opts.n;
  std::vector<T> v((size_t) n), w((size_t) k, T(0)), want((size_t) m, T(0)), got((size_t) m, T(0));
  for (SizeType j = 0; j < n; ++j)
    v[(size_t) j] = Rand<T>::make(0x9E3779B97F4A7C15ull + (uint64_t) j);
  if (left) {
    for (SizeType j = 0; j < n; ++j)  // w = B v
      for (SizeType i = 0; i < m; ++i)
        w[(size_t) i] += bh(LocalElementIndex(i, j)) * v[(size_t) j];
    for (SizeType j = 0; j < m; ++j)  // want = alpha A w
      for (SizeType i = 0; i < m; ++i)
        want[(size_t) i] += alpha * herm(i, j) * w[(size_t) j];
  }
  else {
    for (SizeType j = 0; j < n; ++j)  // w = A v
      for (SizeType i = 0; i < n; ++i)
        w[(size_t) i] += herm(i, j) * v[(size_t) j];
    for (SizeType j = 0; j < n; ++j)  // want = alpha B w
      for (SizeType i = 0; i < m; ++i)
        want[(size_t) i] += alpha * bh(LocalElementIndex(i, j)) * w[(size_t) j];
  }
  for (SizeType j = 0; j < n; ++j)
    for (SizeType i = 0; i < m; ++i) {
      want[(size_t) i] += beta * c_ref(LocalElementIndex(i, j)) * v[(size_t) j];
      got[(size_t) i] += ch(LocalElementIndex(i, j)) * v[(size_t) j];
    }
  double worst = 0, scale = 0;
  for (SizeType i = 0; i < m; ++i) {
    worst = std::max<double>(worst, std::abs(got[(size_t) i] - want[(size_t) i]));
    scale = std::max<double>(scale, std::abs(want[(size_t) i]));
  }
  std::cout << "Check residual max |C v - (beta C_0 v + alpha A B v)| / max |.| : " << (scale > 0 ? worst / scale : worst)
            << std::endl;
}

int main(int argc, char** argv) {
  const Options opts = parse(argc, argv);
  return miniapp::run_main(argc, argv, opts, false,
                           [&opts](auto t, comm::CommunicatorGrid& grid, int world_rank, int world_size) {
                             run<decltype(t)>(opts, grid, world_rank, world_size);
                           });
}
