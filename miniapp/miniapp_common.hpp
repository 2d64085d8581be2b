// miniapp_common.hpp -- what the miniapps of this directory share: the option tokenizer with its error exits, the options
// every miniapp has, the upstream options that are accepted and ignored, the counter-based random numbers, the flop
// weighting and the main() scaffold (MPI, process-count check, grid, dispatch on the element type).  Each miniapp keeps
// its own options, operands, timed call, result line and check, and includes this header by relative path.
#pragma once

#ifdef DLAF_MI355X_WITH_MPI
#include <mpi.h>
#endif

#include <cctype>
#include <complex>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <type_traits>

#include <dlaf_mi355x/dlaf.hpp>

namespace miniapp {

// --grid-rows --grid-cols --nruns --nwarmups --type
struct CommonOptions {
  int grid_rows = 1, grid_cols = 1;
  int64_t nruns = 1, nwarmups = 1;
  char type = 'd';
  // the part of a miniapp's validation that all of them share (whether a negative --nwarmups is refused differs)
  bool valid() const { return nruns >= 1 && std::strchr("sdcz", type) != nullptr; }
};

[[noreturn]] inline void invalid_option_value() {
  std::cerr << "invalid option value" << std::endl;
  std::exit(2);
}

// Walks `--opt value` / `--opt=value`.  The common options are stored in `o`; --backend (with its value), --local,
// --pika:* and --dlaf:* are upstream's and ignored; everything else goes to own(a, val): it returns false for an option
// it does not know, and calls val() for the value of one it does (also to swallow the value of an option it ignores).
// Exits with status 2 on a missing value or an unknown option; `usage`, if any, follows the unknown option's name.
template <class Own>
void parse_options(int argc, char** argv, CommonOptions& o, const char* usage, Own&& own) {
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i], v;
    const auto eq = a.find('=');
    if (eq != std::string::npos) {
      v = a.substr(eq + 1);
      a = a.substr(0, eq);
    }
    auto val = [&]() -> std::string {
      if (!v.empty())
        return v;
      if (i + 1 >= argc) {
        std::cerr << "missing value for " << a << std::endl;
        std::exit(2);
      }
      return argv[++i];
    };
    if (a == "--grid-rows")
      o.grid_rows = std::stoi(val());
    else if (a == "--grid-cols")
      o.grid_cols = std::stoi(val());
    else if (a == "--nruns")
      o.nruns = std::stoll(val());
    else if (a == "--nwarmups")
      o.nwarmups = std::stoll(val());
    else if (a == "--type")
      o.type = (char) std::tolower(val()[0]);
    else if (a == "--backend")
      (void) val();  // there is one backend
    else if (a == "--local" || a.rfind("--pika:", 0) == 0 || a.rfind("--dlaf:", 0) == 0) {
    }
    else if (!own(a, val)) {
      std::cerr << "unknown option " << a;
      if (usage)
        std::cerr << "\nusage: " << usage;
      std::cerr << std::endl;
      std::exit(2);
    }
  }
}

// the first letter of an option's value, upper case (--uplo l, --side Right, ...)
inline char upper_initial(const std::string& value) { return (char) std::toupper(value[0]); }

// counter-based generator: uniform in [-1, 1) from a hash of the global element index (every grid sees the
// same global matrices; cheap enough for benchmark sizes)
inline double uniform_pm1(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;  // splitmix64
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  x ^= x >> 31;
  return (double) (x >> 11) * (2.0 / 9007199254740992.0) - 1.0;
}
template <class T>
struct Rand {
  static T make(uint64_t key) { return (T) uniform_pm1(key); }
};
template <class R>
struct Rand<std::complex<R>> {
  static std::complex<R> make(uint64_t key) { return {(R) uniform_pm1(2 * key), (R) uniform_pm1(2 * key + 1)}; }
};

// flops of add_mul additions and as many multiplications of T (types.h total_ops: a complex addition is 2, a complex
// multiplication 6)
template <class T>
double total_ops(double add_mul) {
  return std::is_same<T, dlaf::BaseType<T>>::value ? 2 * add_mul : 2 * add_mul + 6 * add_mul;
}

// The body of main(): MPI (when built with DLAF_MI355X_WITH_MPI), the process-count check, initialize, the grid, one call
// run(T{}, grid, world_rank, world_size) for the element type of --type, finalize.  local_rank_from_mpi: export the MPI
// node-local rank as LOCAL_RANK unless the launcher has set it (the library picks its GPU from it).
template <class Run>
int run_main(int argc, char** argv, const CommonOptions& opts, bool local_rank_from_mpi, Run&& run) {
  int world_rank = 0, world_size = 1;
#ifdef DLAF_MI355X_WITH_MPI
  int provided = 0;
  MPI_Init_thread(&argc, &argv, MPI_THREAD_MULTIPLE, &provided);
  MPI_Comm_rank(MPI_COMM_WORLD, &world_rank);
  MPI_Comm_size(MPI_COMM_WORLD, &world_size);
  if (local_rank_from_mpi && std::getenv("LOCAL_RANK") == nullptr) {
    MPI_Comm node;
    MPI_Comm_split_type(MPI_COMM_WORLD, MPI_COMM_TYPE_SHARED, world_rank, MPI_INFO_NULL, &node);
    int local = 0;
    MPI_Comm_rank(node, &local);
    setenv("LOCAL_RANK", std::to_string(local).c_str(), 0);
    MPI_Comm_free(&node);
  }
#else
  (void) argc, (void) argv, (void) local_rank_from_mpi;
#endif
  if (opts.grid_rows * opts.grid_cols != world_size) {
    if (world_rank == 0)
      std::cerr << "grid " << opts.grid_rows << " x " << opts.grid_cols << " needs " << opts.grid_rows * opts.grid_cols
                << " processes, got " << world_size << std::endl;
    return 2;
  }
  dlaf::initialize();
  {
#ifdef DLAF_MI355X_WITH_MPI
    dlaf::comm::CommunicatorGrid grid(MPI_COMM_WORLD, opts.grid_rows, opts.grid_cols, dlaf::common::Ordering::ColumnMajor);
#else
    dlaf::comm::CommunicatorGrid grid = dlaf::comm::CommunicatorGrid::single();
#endif
    switch (opts.type) {
      case 's': run(float{}, grid, world_rank, world_size); break;
      case 'd': run(double{}, grid, world_rank, world_size); break;
      case 'c': run(std::complex<float>{}, grid, world_rank, world_size); break;
      default: run(std::complex<double>{}, grid, world_rank, world_size); break;
    }
  }
  dlaf::finalize();
#ifdef DLAF_MI355X_WITH_MPI
  MPI_Finalize();
#endif
  return 0;
}

}  // namespace miniapp
