/* dlaf.hpp -- header-only C++ facade over the C ABI of libdlaf_mi355x.so with the names of the reference's
 * C++ interface for the Cholesky path, so that code written against DLA-Future reads the same:
 *
 *     dlaf::Matrix<T, Device::CPU> mat_h(distribution);                       // include/dlaf/matrix/matrix.h:86-97
 *     {
 *       dlaf::matrix::MatrixMirror<T, Device::GPU, Device::CPU> mat(grid, mat_h, uplo);  // matrix_mirror.h:137-173
 *       dlaf::cholesky_factorization<Backend::GPU, Device::GPU, T>(grid, uplo, mat.get());
 *     }                                                                       // include/dlaf/factorization/cholesky.h:39-79
 *     dlaf::triangular_solver<Backend::GPU, Device::GPU, T>(grid, side, uplo, op, diag, alpha, a, b);
 *                                                                             // include/dlaf/solver/triangular.h:41-177
 *     dlaf::triangular_multiplication<Backend::GPU, Device::GPU, T>(grid, side, uplo, op, diag, alpha, a, b);
 *                                                                     // include/dlaf/multiplication/triangular.h
 *     dlaf::hermitian_multiplication<Backend::GPU, Device::GPU, T>(grid, side, uplo, alpha, a, b, beta, c);
 *                                                                     // include/dlaf/multiplication/hermitian.h
 *     dlaf::multiplication::internal::generalMatrix<Backend::GPU, Device::GPU, T>(opA, opB, alpha, a, b, beta, c);
 *                                                                     // include/dlaf/multiplication/general.h
 *
 * What differs from the reference, by design: there is no pika runtime (the calls are blocking, no pika::wait),
 * Backend::MC does not exist (the library has no CPU path: static_assert), Matrix<T, Device::CPU> stores its
 * local part column-major with ld = the local row count rounded up to 64 (matrix.h:86-97) or wraps a caller's
 * pointer, Matrix<T, Device::GPU> is the device-resident tile-layout matrix of the library.  Precondition
 * failures terminate, like DLAF_ASSERT.  C++17, depends on the C headers only. */
#pragma once

#include <algorithm>
#include <complex>
#include <cstddef>
#include <cstdio>
#include <exception>
#include <functional>
#include <memory>
#include <type_traits>
#include <utility>
#include <vector>

#include <dlaf_c/desc.h>
#include <dlaf_c/eigensolver/eigensolver.h>
#include <dlaf_c/eigensolver/gen_eigensolver.h>
#include <dlaf_c/factorization/cholesky.h>
#include <dlaf_c/grid.h>
#include <dlaf_c/init.h>
#include <dlaf_mi355x/dlaf_mi355x.h>

namespace dlaf {

using SizeType = std::ptrdiff_t;
// dlaf::BaseType (include/dlaf/types.h): the real type behind an element type
template <class T>
struct BaseTypeOf {
  using type = T;
};
template <class R>
struct BaseTypeOf<std::complex<R>> {
  using type = R;
};
template <class T>
using BaseType = typename BaseTypeOf<T>::type;  // include/dlaf/types.h:25

enum class Backend { MC, GPU, Default = GPU };   // types.h:31-37 (MC has no implementation in this library)
enum class Device { CPU, GPU, Default = GPU };   // types.h:39-45

namespace blas {
enum class Uplo : char { Upper = 'U', Lower = 'L', General = 'G' };
enum class Side : char { Left = 'L', Right = 'R' };
enum class Op : char { NoTrans = 'N', Trans = 'T', ConjTrans = 'C' };
enum class Diag : char { NonUnit = 'N', Unit = 'U' };
}  // namespace blas

namespace common {
enum class Ordering { RowMajor, ColumnMajor };  // common/index2d.h:26
}

namespace internal {
[[noreturn]] inline void fail(const char* what) {
  std::fprintf(stderr, "[dlaf] precondition failed: %s\n", what);
  std::terminate();
}
template <class T>
constexpr char type_tag() {
  if constexpr (std::is_same_v<T, float>)
    return 's';
  else if constexpr (std::is_same_v<T, double>)
    return 'd';
  else if constexpr (std::is_same_v<T, std::complex<float>>)
    return 'c';
  else {
    static_assert(std::is_same_v<T, std::complex<double>>, "element type must be float, double or their complex");
    return 'z';
  }
}
}  // namespace internal

// ---- 2-D index / size helpers (common/index2d.h, matrix/index.h) ---------------------------------------------
template <class Tag>
struct Size2DT {
  SizeType r = 0, c = 0;
  Size2DT() = default;
  Size2DT(SizeType rows_, SizeType cols_) : r(rows_), c(cols_) {}
  SizeType rows() const { return r; }
  SizeType cols() const { return c; }
  bool isEmpty() const { return r == 0 || c == 0; }
};
template <class Tag>
struct Index2DT {
  SizeType r = 0, c = 0;
  Index2DT() = default;
  Index2DT(SizeType row_, SizeType col_) : r(row_), c(col_) {}
  SizeType row() const { return r; }
  SizeType col() const { return c; }
};
struct GlobalElementTag;
struct LocalElementTag;
struct TileElementTag;
struct GridTag;
using GlobalElementSize = Size2DT<GlobalElementTag>;
using LocalElementSize = Size2DT<LocalElementTag>;
using TileElementSize = Size2DT<TileElementTag>;
using GlobalElementIndex = Index2DT<GlobalElementTag>;
using LocalElementIndex = Index2DT<LocalElementTag>;
namespace comm {
using Size2D = Size2DT<GridTag>;
using Index2D = Index2DT<GridTag>;

// communication/communicator_grid.h:37-153.  Owns a grid context of the library.
class CommunicatorGrid {
public:
  // MPI-free constructors (the library's own grid entry points)
  static CommunicatorGrid single() { return CommunicatorGrid(dlaf_mi355x_create_grid_single()); }
  static CommunicatorGrid rccl(const void* unique_id128, int nranks, int rank, int rows, int cols,
                               common::Ordering ordering) {
    return CommunicatorGrid(dlaf_mi355x_create_grid_rccl(unique_id128, nranks, rank, rows, cols,
                                                        ordering == common::Ordering::ColumnMajor ? 'C' : 'R'));
  }
#ifdef DLAF_MI355X_WITH_MPI
  // the reference's constructor (communicator_grid.h:41): needs libdlaf_mi355x_mpi.so
  CommunicatorGrid(MPI_Comm comm, int rows, int cols, common::Ordering ordering)
      : CommunicatorGrid(dlaf_create_grid(comm, rows, cols, ordering == common::Ordering::ColumnMajor ? 'C' : 'R')) {}
#endif
  // adopts an existing context (e.g. from dlaf_create_grid); freed on destruction
  explicit CommunicatorGrid(int context) : ctx_(context) {
    int pr = 0, pc = 0, mr = 0, mc = 0;
    if (context < 0 || dlaf_mi355x_grid_info(context, &pr, &pc, &mr, &mc) != 0)
      internal::fail("valid grid context");
    size_ = Size2D(pr, pc);
    rank_ = Index2D(mr, mc);
  }
  CommunicatorGrid(CommunicatorGrid&& o) noexcept : ctx_(o.ctx_), size_(o.size_), rank_(o.rank_) { o.ctx_ = -1; }
  CommunicatorGrid(const CommunicatorGrid&) = delete;
  CommunicatorGrid& operator=(const CommunicatorGrid&) = delete;
  ~CommunicatorGrid() {
    if (ctx_ >= 0)
      dlaf_free_grid(ctx_);
  }
  Index2D rank() const { return rank_; }
  Size2D size() const { return size_; }
  int context() const { return ctx_; }
  void wait_all_communicators() const { dlaf_mi355x_grid_barrier(ctx_); }

private:
  int ctx_ = -1;
  Size2D size_;
  Index2D rank_;
};
}  // namespace comm

namespace matrix {

// matrix/distribution.h: global size, block size, process grid, this process, source process
class Distribution {
public:
  Distribution() = default;
  Distribution(const LocalElementSize& size, const TileElementSize& block)
      : size_(size.rows(), size.cols()), block_(block), grid_(1, 1), rank_(0, 0), src_(0, 0) {}
  Distribution(const GlobalElementSize& size, const TileElementSize& block, const comm::Size2D& grid_size,
               const comm::Index2D& rank, const comm::Index2D& source_rank)
      : size_(size), block_(block), grid_(grid_size), rank_(rank), src_(source_rank) {
    if (block.rows() < 1 || block.cols() < 1)
      internal::fail("block size >= 1");
  }
  const GlobalElementSize& size() const { return size_; }
  const TileElementSize& block_size() const { return block_; }
  const comm::Size2D& grid_size() const { return grid_; }
  const comm::Index2D& rank_index() const { return rank_; }
  const comm::Index2D& source_rank_index() const { return src_; }
  LocalElementSize local_size() const {
    return LocalElementSize(dlaf_mi355x_dist_local_size(size_.rows(), (int) block_.rows(), (int) grid_.rows(),
                                                        (int) rank_.row(), (int) src_.row()),
                            dlaf_mi355x_dist_local_size(size_.cols(), (int) block_.cols(), (int) grid_.cols(),
                                                        (int) rank_.col(), (int) src_.col()));
  }
  // global element index of local element (i, j) (util_distribution.h:82-196)
  GlobalElementIndex global_element_index(const LocalElementIndex& l) const {
    auto one = [](SizeType li, SizeType nb, SizeType P, SizeType rank, SizeType src) {
      const SizeType lt = li / nb;
      return (lt * P + (rank + P - src) % P) * nb + li % nb;
    };
    return GlobalElementIndex(one(l.row(), block_.rows(), grid_.rows(), rank_.row(), src_.row()),
                              one(l.col(), block_.cols(), grid_.cols(), rank_.col(), src_.col()));
  }

private:
  GlobalElementSize size_;
  TileElementSize block_{1, 1};
  comm::Size2D grid_{1, 1};
  comm::Index2D rank_, src_;
};

}  // namespace matrix

template <class T, Device D>
class Matrix;

// Host matrix: the local part of a block-cyclic matrix, column-major (ScaLAPACK local layout).
template <class T>
class Matrix<T, Device::CPU> {
public:
  using ElementType = T;
  Matrix(const LocalElementSize& size, const TileElementSize& block) : Matrix(matrix::Distribution(size, block)) {}
  explicit Matrix(matrix::Distribution dist) : dist_(std::move(dist)) {
    const LocalElementSize ls = dist_.local_size();
    ld_ = std::max<SizeType>(1, (ls.rows() + 63) / 64 * 64);  // matrix.h:86-97
    own_.assign((std::size_t) ld_ * (std::size_t) std::max<SizeType>(1, ls.cols()), T{});
    ptr_ = own_.data();
  }
  // wraps the caller's memory (matrix.h:137-138: Matrix(distribution, layout, ptr))
  Matrix(matrix::Distribution dist, T* ptr, SizeType ld) : dist_(std::move(dist)), ptr_(ptr), ld_(ld) {}
  const matrix::Distribution& distribution() const { return dist_; }
  GlobalElementSize size() const { return dist_.size(); }
  TileElementSize block_size() const { return dist_.block_size(); }
  T* ptr() { return ptr_; }
  const T* ptr() const { return ptr_; }
  SizeType ld() const { return ld_; }
  T& operator()(const LocalElementIndex& i) { return ptr_[i.row() + i.col() * ld_]; }
  const T& operator()(const LocalElementIndex& i) const { return ptr_[i.row() + i.col() * ld_]; }

private:
  matrix::Distribution dist_;
  std::vector<T> own_;
  T* ptr_ = nullptr;
  SizeType ld_ = 1;
};

// Device matrix: resident in HBM in the library's tile layout (created through a MatrixMirror or empty).
template <class T>
class Matrix<T, Device::GPU> {
public:
  using ElementType = T;
  Matrix(const comm::CommunicatorGrid& grid, matrix::Distribution dist, blas::Uplo uplo)
      : dist_(std::move(dist)), uplo_(uplo), ctx_(grid.context()) {
    const auto sz = dist_.size();
    const auto bs = dist_.block_size();
    if (sz.rows() != sz.cols() || bs.rows() != bs.cols())
      internal::fail("device matrices of this library are square with square blocks");
    DLAF_descriptor d{(int) sz.rows(), (int) sz.cols(), (int) bs.rows(), (int) bs.cols(),
                      (int) dist_.source_rank_index().row(), (int) dist_.source_rank_index().col(), 0, 0, 1};
    if (dlaf_mi355x_matrix_create(ctx_, internal::type_tag<T>(), (char) uplo, d, &h_) != 0)
      internal::fail("dlaf_mi355x_matrix_create");
  }
  Matrix(Matrix&& o) noexcept : dist_(o.dist_), uplo_(o.uplo_), ctx_(o.ctx_), h_(o.h_) { o.h_ = nullptr; }
  Matrix(const Matrix&) = delete;
  ~Matrix() {
    if (h_)
      dlaf_mi355x_matrix_destroy(h_);
  }
  const matrix::Distribution& distribution() const { return dist_; }
  GlobalElementSize size() const { return dist_.size(); }
  TileElementSize block_size() const { return dist_.block_size(); }
  blas::Uplo uplo() const { return uplo_; }
  dlaf_mi355x_matrix_t handle() const { return h_; }
  int context() const { return ctx_; }

private:
  matrix::Distribution dist_;
  blas::Uplo uplo_;
  int ctx_;
  dlaf_mi355x_matrix_t h_ = nullptr;
};

// ---- what every call into the C ABI below shares ----------------------------------------------------------------
namespace internal {
// a host matrix as the C entries take it, next to its pointer
template <class T>
DLAF_descriptor descriptor_of(const Matrix<T, Device::CPU>& m) {
  const auto& d = m.distribution();
  return DLAF_descriptor{(int) d.size().rows(), (int) d.size().cols(), (int) d.block_size().rows(),
                         (int) d.block_size().cols(), (int) d.source_rank_index().row(),
                         (int) d.source_rank_index().col(), 0, 0, (int) m.ld()};
}
// the C entry of a family for the element type T: one of its four functions, chosen when the template is instantiated.
// In C++ dlaf_complex_c / dlaf_complex_z are std::complex<float> / <double>, so the complex entries take T* as it is.
template <class T, auto S, auto D, auto C, auto Z>
constexpr auto c_entry() {
  if constexpr (std::is_same_v<T, float>)
    return S;
  else if constexpr (std::is_same_v<T, double>)
    return D;
  else if constexpr (std::is_same_v<T, std::complex<float>>)
    return C;
  else {
    static_assert(std::is_same_v<T, std::complex<double>>, "element type must be float, double or their complex");
    return Z;
  }
}
}  // namespace internal
// DLAF_MI355X_ENTRY(T, dlaf_mi355x_foo) is dlaf_mi355x_foo_{s,d,c,z}; DLAF_MI355X_EIGEN_ENTRY(T, foo) is
// dlaf_symmetric_foo_{s,d} / dlaf_hermitian_foo_{c,z} (the dlaf_c names).  Both are #undef'd at the end of this header.
#define DLAF_MI355X_ENTRY(T, family) (::dlaf::internal::c_entry<T, family##_s, family##_d, family##_c, family##_z>())
#define DLAF_MI355X_EIGEN_ENTRY(T, family)                                                                 \
  (::dlaf::internal::c_entry<T, dlaf_symmetric_##family##_s, dlaf_symmetric_##family##_d, dlaf_hermitian_##family##_c, \
                             dlaf_hermitian_##family##_z>())

namespace matrix {

// matrix/matrix_mirror.h:137-173: copies the source to the target device on construction and back on
// destruction (copyTargetToSource / copySourceToTarget on demand).  The uplo triangle is what travels, as in
// the Cholesky path; `uplo` must therefore be given (the reference mirrors whole matrices).
template <class T, Device Target, Device Source>
class MatrixMirror;

template <class T>
class MatrixMirror<T, Device::GPU, Device::CPU> {
public:
  MatrixMirror(const comm::CommunicatorGrid& grid, Matrix<T, Device::CPU>& source, blas::Uplo uplo)
      : src_(source), dev_(grid, source.distribution(), uplo) {
    copySourceToTarget();
  }
  ~MatrixMirror() { copyTargetToSource(); }
  Matrix<T, Device::GPU>& get() { return dev_; }
  void copySourceToTarget() {
    if (dlaf_mi355x_matrix_upload(dev_.handle(), src_.ptr(), (int) src_.ld()) != 0)
      internal::fail("dlaf_mi355x_matrix_upload");
  }
  void copyTargetToSource() {
    if (dlaf_mi355x_matrix_download(dev_.handle(), src_.ptr(), (int) src_.ld()) != 0)
      internal::fail("dlaf_mi355x_matrix_download");
  }

private:
  Matrix<T, Device::CPU>& src_;
  Matrix<T, Device::GPU> dev_;
};

namespace util {
// matrix/util_matrix.h:148-160 (set): el(GlobalElementIndex) for every local element
template <class T, class ElementGetter>
void set(Matrix<T, Device::CPU>& m, ElementGetter&& el) {
  const LocalElementSize ls = m.distribution().local_size();
  for (SizeType j = 0; j < ls.cols(); ++j)
    for (SizeType i = 0; i < ls.rows(); ++i)
      m(LocalElementIndex(i, j)) = el(m.distribution().global_element_index(LocalElementIndex(i, j)));
}
// util_matrix.h:498-501
template <class T>
void set_random_hermitian_positive_definite(const comm::CommunicatorGrid& grid, Matrix<T, Device::CPU>& m) {
  if (dlaf_mi355x_set_random_hpd(grid.context(), internal::type_tag<T>(), m.ptr(), internal::descriptor_of(m), 0) != 0)
    internal::fail("square matrix with square blocks");
}
}  // namespace util
}  // namespace matrix

// ---- the algorithms ------------------------------------------------------------------------------------------
// include/dlaf/factorization/cholesky.h:67-79.  Device-resident: factors in HBM, nothing crosses PCIe.
template <Backend B, Device D, class T>
void cholesky_factorization(comm::CommunicatorGrid& grid, blas::Uplo uplo, Matrix<T, Device::GPU>& mat) {
  static_assert(B == Backend::GPU && D == Device::GPU, "this library implements Backend::GPU on Device::GPU only");
  if (uplo != mat.uplo())
    internal::fail("uplo of the call equals the uplo the device matrix was created with");
  if (grid.context() != mat.context())
    internal::fail("matrix::equal_process_grid(mat_a, grid)");
  const int info = dlaf_mi355x_cholesky_factorization_device(mat.handle());
  if (info != 0) {
    // the reference aborts in the tile kernel (lapack/tile.h:374-378, src/cusolver/assert_info.cu:35-45)
    std::fprintf(stderr, "[dlaf] cholesky_factorization: the leading minor of order %d is not positive definite\n", info);
    std::terminate();
  }
}
// Host-resident local part (what the C wrapper does around the template, src/c_api/factorization/cholesky.h:44-55)
template <Backend B, Device D, class T>
void cholesky_factorization(comm::CommunicatorGrid& grid, blas::Uplo uplo, Matrix<T, Device::CPU>& mat) {
  static_assert(B == Backend::GPU, "this library has no CPU backend");
  matrix::MatrixMirror<T, Device::GPU, Device::CPU> mirror(grid, mat, uplo);
  cholesky_factorization<Backend::GPU, Device::GPU, T>(grid, uplo, mirror.get());
}

// include/dlaf/factorization/cholesky.h:39-50: the local (one process) overloads
template <Backend B, Device D, class T>
void cholesky_factorization(blas::Uplo uplo, Matrix<T, Device::CPU>& mat) {
  comm::CommunicatorGrid grid = comm::CommunicatorGrid::single();
  cholesky_factorization<B, D, T>(grid, uplo, mat);
}

// include/dlaf/solver/triangular.h:109-177 (host-resident operands)
template <Backend B, Device D, class T>
void triangular_solver(comm::CommunicatorGrid& grid, blas::Side side, blas::Uplo uplo, blas::Op op, blas::Diag diag,
                       T alpha, Matrix<T, Device::CPU>& mat_a, Matrix<T, Device::CPU>& mat_b) {
  static_assert(B == Backend::GPU, "this library has no CPU backend");
  using internal::descriptor_of;
  if (DLAF_MI355X_ENTRY(T, dlaf_mi355x_triangular_solver)(grid.context(), (char) side, (char) uplo, (char) op, (char) diag,
                                                          &alpha, mat_a.ptr(), descriptor_of(mat_a), mat_b.ptr(),
                                                          descriptor_of(mat_b)) != 0)
    internal::fail("triangular_solver");
}

// include/dlaf/solver/triangular.h:41-107: the local overload
template <Backend B, Device D, class T>
void triangular_solver(blas::Side side, blas::Uplo uplo, blas::Op op, blas::Diag diag, T alpha,
                       Matrix<T, Device::CPU>& mat_a, Matrix<T, Device::CPU>& mat_b) {
  comm::CommunicatorGrid grid = comm::CommunicatorGrid::single();
  triangular_solver<B, D, T>(grid, side, uplo, op, diag, alpha, mat_a, mat_b);
}

// include/dlaf/multiplication/triangular.h: B = alpha op(A) B (Left) / alpha B op(A) (Right), host-resident operands;
// every op on grids too (the reference's distributed version implements NoTrans only)
template <Backend B, Device D, class T>
void triangular_multiplication(comm::CommunicatorGrid& grid, blas::Side side, blas::Uplo uplo, blas::Op op,
                               blas::Diag diag, T alpha, Matrix<T, Device::CPU>& mat_a, Matrix<T, Device::CPU>& mat_b) {
  static_assert(B == Backend::GPU, "this library has no CPU backend");
  using internal::descriptor_of;
  if (DLAF_MI355X_ENTRY(T, dlaf_mi355x_triangular_multiplication)(grid.context(), (char) side, (char) uplo, (char) op,
                                                                  (char) diag, &alpha, mat_a.ptr(), descriptor_of(mat_a),
                                                                  mat_b.ptr(), descriptor_of(mat_b)) != 0)
    internal::fail("triangular_multiplication");
}

// the local overload
template <Backend B, Device D, class T>
void triangular_multiplication(blas::Side side, blas::Uplo uplo, blas::Op op, blas::Diag diag, T alpha,
                               Matrix<T, Device::CPU>& mat_a, Matrix<T, Device::CPU>& mat_b) {
  comm::CommunicatorGrid grid = comm::CommunicatorGrid::single();
  triangular_multiplication<B, D, T>(grid, side, uplo, op, diag, alpha, mat_a, mat_b);
}

// include/dlaf/multiplication/hermitian.h:52, :114: C = beta C + alpha A B (Left) / beta C + alpha B A (Right), A
// Hermitian with only its uplo triangle read; host-resident operands, every side x uplo (the reference implements
// Left / Lower only).  The reference's read-only Matrix<const T, D>& operands are const Matrix<T, D>& here.
template <Backend B, Device D, class T>
void hermitian_multiplication(comm::CommunicatorGrid& grid, blas::Side side, blas::Uplo uplo, const T alpha,
                              const Matrix<T, Device::CPU>& mat_a, const Matrix<T, Device::CPU>& mat_b, const T beta,
                              Matrix<T, Device::CPU>& mat_c) {
  static_assert(B == Backend::GPU, "this library has no CPU backend");
  using internal::descriptor_of;
  if (DLAF_MI355X_ENTRY(T, dlaf_mi355x_hermitian_multiplication)(grid.context(), (char) side, (char) uplo, &alpha, mat_a.ptr(),
                                                                 descriptor_of(mat_a), mat_b.ptr(), descriptor_of(mat_b),
                                                                 &beta, mat_c.ptr(), descriptor_of(mat_c)) != 0)
    internal::fail("hermitian_multiplication");
}

// the local overload
template <Backend B, Device D, class T>
void hermitian_multiplication(blas::Side side, blas::Uplo uplo, const T alpha, const Matrix<T, Device::CPU>& mat_a,
                              const Matrix<T, Device::CPU>& mat_b, const T beta, Matrix<T, Device::CPU>& mat_c) {
  comm::CommunicatorGrid grid = comm::CommunicatorGrid::single();
  hermitian_multiplication<B, D, T>(grid, side, uplo, alpha, mat_a, mat_b, beta, mat_c);
}

// include/dlaf/multiplication/general.h: C = beta C + alpha op(A) op(B) on host-resident operands, under the reference's
// names.  Local matrices: every op pair (the reference: NoTrans x NoTrans).  The grid overload is NoTrans x NoTrans,
// as in the reference.  mat_a and mat_b are the matrices as stored; one square block for the three.
namespace multiplication::internal {
template <Backend B, Device D, class T>
void generalMatrix(comm::CommunicatorGrid& grid, blas::Op opA, blas::Op opB, const T alpha,
                   const Matrix<T, Device::CPU>& mat_a, const Matrix<T, Device::CPU>& mat_b, const T beta,
                   Matrix<T, Device::CPU>& mat_c) {
  static_assert(B == Backend::GPU, "this library has no CPU backend");
  using dlaf::internal::descriptor_of;
  if (DLAF_MI355X_ENTRY(T, dlaf_mi355x_general_multiplication)(grid.context(), (char) opA, (char) opB, &alpha, mat_a.ptr(),
                                                               descriptor_of(mat_a), mat_b.ptr(), descriptor_of(mat_b), &beta,
                                                               mat_c.ptr(), descriptor_of(mat_c)) != 0)
    dlaf::internal::fail("generalMatrix");
}
// the reference's two signatures: local matrices with ops, a grid without (NoTrans x NoTrans)
template <Backend B, Device D, class T>
void generalMatrix(blas::Op opA, blas::Op opB, const T alpha, const Matrix<T, Device::CPU>& mat_a,
                   const Matrix<T, Device::CPU>& mat_b, const T beta, Matrix<T, Device::CPU>& mat_c) {
  comm::CommunicatorGrid grid = comm::CommunicatorGrid::single();
  generalMatrix<B, D, T>(grid, opA, opB, alpha, mat_a, mat_b, beta, mat_c);
}
template <Backend B, Device D, class T>
void generalMatrix(comm::CommunicatorGrid& grid, const T alpha, const Matrix<T, Device::CPU>& mat_a,
                   const Matrix<T, Device::CPU>& mat_b, const T beta, Matrix<T, Device::CPU>& mat_c) {
  generalMatrix<B, D, T>(grid, blas::Op::NoTrans, blas::Op::NoTrans, alpha, mat_a, mat_b, beta, mat_c);
}
}  // namespace multiplication::internal

// BLAS xSYRK / xHERK and xSYR2K / xHER2K on host-resident operands (the reference runs them tile by tile inside its
// algorithms and exposes no such call; the names follow hermitian_multiplication): only the uplo triangle of mat_c is read
// or written, its diagonal comes back real.
//   rank-k : C = alpha A A^H + beta C (NoTrans, A n x k) / alpha A^H A + beta C (ConjTrans, A k x n); alpha, beta real
//   rank-2k: C = alpha A B^H + conj(alpha) B A^H + beta C / alpha A^H B + conj(alpha) B^H A + beta C; beta real
// Real types also take Trans (= ConjTrans); complex types refuse it.  Local matrices: both ops.  A grid of more than one
// process: NoTrans only.  One square block for all operands; mat_b is stored, blocked and distributed like mat_a.
template <Backend B, Device D, class T>
void hermitian_rank_k_update(comm::CommunicatorGrid& grid, blas::Uplo uplo, blas::Op op, const BaseType<T> alpha,
                             const Matrix<T, Device::CPU>& mat_a, const BaseType<T> beta, Matrix<T, Device::CPU>& mat_c) {
  static_assert(B == Backend::GPU, "this library has no CPU backend");
  using internal::descriptor_of;
  if (DLAF_MI355X_ENTRY(T, dlaf_mi355x_hermitian_rank_k_update)(grid.context(), (char) uplo, (char) op, &alpha, mat_a.ptr(),
                                                                descriptor_of(mat_a), &beta, mat_c.ptr(),
                                                                descriptor_of(mat_c)) != 0)
    internal::fail("hermitian_rank_k_update");
}
template <Backend B, Device D, class T>
void hermitian_rank_2k_update(comm::CommunicatorGrid& grid, blas::Uplo uplo, blas::Op op, const T alpha,
                              const Matrix<T, Device::CPU>& mat_a, const Matrix<T, Device::CPU>& mat_b,
                              const BaseType<T> beta, Matrix<T, Device::CPU>& mat_c) {
  static_assert(B == Backend::GPU, "this library has no CPU backend");
  using internal::descriptor_of;
  if (DLAF_MI355X_ENTRY(T, dlaf_mi355x_hermitian_rank_2k_update)(grid.context(), (char) uplo, (char) op, &alpha, mat_a.ptr(),
                                                                 descriptor_of(mat_a), mat_b.ptr(), descriptor_of(mat_b),
                                                                 &beta, mat_c.ptr(), descriptor_of(mat_c)) != 0)
    internal::fail("hermitian_rank_2k_update");
}
// the local overloads
template <Backend B, Device D, class T>
void hermitian_rank_k_update(blas::Uplo uplo, blas::Op op, const BaseType<T> alpha, const Matrix<T, Device::CPU>& mat_a,
                             const BaseType<T> beta, Matrix<T, Device::CPU>& mat_c) {
  comm::CommunicatorGrid grid = comm::CommunicatorGrid::single();
  hermitian_rank_k_update<B, D, T>(grid, uplo, op, alpha, mat_a, beta, mat_c);
}
template <Backend B, Device D, class T>
void hermitian_rank_2k_update(blas::Uplo uplo, blas::Op op, const T alpha, const Matrix<T, Device::CPU>& mat_a,
                              const Matrix<T, Device::CPU>& mat_b, const BaseType<T> beta, Matrix<T, Device::CPU>& mat_c) {
  comm::CommunicatorGrid grid = comm::CommunicatorGrid::single();
  hermitian_rank_2k_update<B, D, T>(grid, uplo, op, alpha, mat_a, mat_b, beta, mat_c);
}

// The weighted rank-k update ("xSYRK / xHERK with weights"): the uplo triangle of mat_c becomes
//   alpha A D A^H + beta C (NoTrans, A n x k) / alpha A^H D A + beta C (ConjTrans, A k x n),  D = diag(d) REAL, any sign;
// d: k reals on the host, the same on every rank.  The weights are multiplied in inside the rank-k kernel: no scaled copy
// of A, the flops of a rank-k update.  Semantics and requirements of hermitian_rank_k_update; a zero weight does NOT
// unreference its column (0 * NaN is NaN).
template <Backend B, Device D, class T>
void hermitian_weighted_rank_k_update(comm::CommunicatorGrid& grid, blas::Uplo uplo, blas::Op op, const BaseType<T> alpha,
                                      const Matrix<T, Device::CPU>& mat_a, const BaseType<T>* d, const BaseType<T> beta,
                                      Matrix<T, Device::CPU>& mat_c) {
  static_assert(B == Backend::GPU, "this library has no CPU backend");
  using internal::descriptor_of;
  if (DLAF_MI355X_ENTRY(T, dlaf_mi355x_hermitian_weighted_rank_k_update)(grid.context(), (char) uplo, (char) op, &alpha,
                                                                         mat_a.ptr(), descriptor_of(mat_a), d, &beta,
                                                                         mat_c.ptr(), descriptor_of(mat_c)) != 0)
    internal::fail("hermitian_weighted_rank_k_update");
}
template <Backend B, Device D, class T>
void hermitian_weighted_rank_k_update(blas::Uplo uplo, blas::Op op, const BaseType<T> alpha,
                                      const Matrix<T, Device::CPU>& mat_a, const BaseType<T>* d, const BaseType<T> beta,
                                      Matrix<T, Device::CPU>& mat_c) {
  comm::CommunicatorGrid grid = comm::CommunicatorGrid::single();
  hermitian_weighted_rank_k_update<B, D, T>(grid, uplo, op, alpha, mat_a, d, beta, mat_c);
}

// Functions of a Hermitian matrix: the Lower triangle of mat_a becomes that of f(A) = sum_j g_j z_j z_j^H over the selected
// eigenpairs, g = weights(w): the eigensolver, ONE call of `weights`, and the weighted rank-k update with the eigenvectors
// still in HBM.  weights(n, w, begin, end, g) writes g[begin, end).  selection: all eigenpairs (default), an index range
// [begin, end), or a value interval (vl, vu]; unselected eigenvalues weigh 0 and their eigenvectors are never computed.
// Returns the eigensolver's status; `eigenvalues` (n reals) receives all eigenvalues, `selected` (null allowed) the
// selected [begin, end).  hermitian_power: x^exponent above `threshold` (>= 0), the rest dropped and counted.
template <class R>
using SpectralWeights = std::function<void(SizeType n, const R* w, SizeType begin, SizeType end, R* g)>;
template <class R>
struct SpectralSelection {
  const SizeType* index_range = nullptr;  // {begin, end}
  const R* value_interval = nullptr;      // {vl, vu}
};
namespace internal {
template <class R>
void spectral_weights_trampoline(long n, const R* w, long begin, long end, R* g, void* user) {
  (*static_cast<const SpectralWeights<R>*>(user))(n, w, begin, end, g);
}
}  // namespace internal
template <Backend B, Device D, class T>
int hermitian_function(comm::CommunicatorGrid& grid, blas::Uplo uplo, Matrix<T, Device::CPU>& mat_a,
                       BaseType<T>* eigenvalues, const SpectralWeights<BaseType<T>>& weights,
                       SpectralSelection<BaseType<T>> selection = {}, SizeType* selected = nullptr) {
  static_assert(B == Backend::GPU, "this library has no CPU backend");
  using R = BaseType<T>;
  void* user = const_cast<SpectralWeights<R>*>(&weights);
  long range[2] = {0, 0}, sel[2] = {0, 0};
  if (selection.index_range) {
    range[0] = (long) selection.index_range[0];
    range[1] = (long) selection.index_range[1];
  }
  const long* ir = selection.index_range ? range : nullptr;
  const int r = DLAF_MI355X_ENTRY(T, dlaf_mi355x_hermitian_function)(
      grid.context(), (char) uplo, mat_a.ptr(), internal::descriptor_of(mat_a), eigenvalues,
      &internal::spectral_weights_trampoline<R>, user, ir, selection.value_interval, sel);
  if (selected) {
    selected[0] = (SizeType) sel[0];
    selected[1] = (SizeType) sel[1];
  }
  return r;
}
template <Backend B, Device D, class T>
int hermitian_power(comm::CommunicatorGrid& grid, blas::Uplo uplo, Matrix<T, Device::CPU>& mat_a, BaseType<T>* eigenvalues,
                    double exponent, double threshold = 0.0, SizeType* n_dropped = nullptr) {
  static_assert(B == Backend::GPU, "this library has no CPU backend");
  long dropped = 0;
  const int r = DLAF_MI355X_ENTRY(T, dlaf_mi355x_hermitian_power)(grid.context(), (char) uplo, mat_a.ptr(),
                                                                  internal::descriptor_of(mat_a), eigenvalues, exponent,
                                                                  threshold, &dropped);
  if (n_dropped)
    *n_dropped = (SizeType) dropped;
  return r;
}

// C = beta C + alpha op(A) on the uplo part of mat_c (PBLAS p?geadd / p?tradd, p?tran / p?tranu / p?tranc; ScaLAPACK
// p?lacpy is alpha 1, beta 0, NoTrans) and the completion of a Hermitian / symmetric matrix from one triangle, on
// host-resident operands.  The reference has no such algorithm (its matrix::copy is the alpha 1, beta 0, NoTrans case);
// the names follow hermitian_rank_k_update.  uplo: blas::Uplo::General (all), Lower (i >= j), Upper (i <= j).  Outside
// the part mat_c keeps its bits; alpha 1, beta 0 with NoTrans / Trans is a bit copy.  Any grid, every op; one square
// block for both; NoTrans needs mat_a on mat_c's source process.  hermitian_complete fills the OTHER triangle of the
// square mat_a from its uplo one: conjugate = true the Hermitian completion (diagonal imaginary parts exactly 0),
// false the symmetric one (diagonal untouched).
template <Backend B, Device D, class T>
void general_addition(comm::CommunicatorGrid& grid, blas::Uplo uplo, blas::Op op, const T alpha,
                      const Matrix<T, Device::CPU>& mat_a, const T beta, Matrix<T, Device::CPU>& mat_c) {
  static_assert(B == Backend::GPU, "this library has no CPU backend");
  const char u = uplo == blas::Uplo::Lower ? 'L' : uplo == blas::Uplo::Upper ? 'U' : 'A';
  if (DLAF_MI355X_ENTRY(T, dlaf_mi355x_general_addition)(grid.context(), u, (char) op, &alpha, mat_a.ptr(),
                                                         internal::descriptor_of(mat_a), &beta, mat_c.ptr(),
                                                         internal::descriptor_of(mat_c)) != 0)
    internal::fail("general_addition");
}
template <Backend B, Device D, class T>
void hermitian_complete(comm::CommunicatorGrid& grid, blas::Uplo uplo, bool conjugate, Matrix<T, Device::CPU>& mat_a) {
  static_assert(B == Backend::GPU, "this library has no CPU backend");
  if (DLAF_MI355X_ENTRY(T, dlaf_mi355x_hermitian_complete)(grid.context(), (char) uplo, conjugate ? 'H' : 'S', mat_a.ptr(),
                                                           internal::descriptor_of(mat_a)) != 0)
    internal::fail("hermitian_complete");
}
// the local overloads
template <Backend B, Device D, class T>
void general_addition(blas::Uplo uplo, blas::Op op, const T alpha, const Matrix<T, Device::CPU>& mat_a, const T beta,
                      Matrix<T, Device::CPU>& mat_c) {
  comm::CommunicatorGrid grid = comm::CommunicatorGrid::single();
  general_addition<B, D, T>(grid, uplo, op, alpha, mat_a, beta, mat_c);
}
template <Backend B, Device D, class T>
void hermitian_complete(blas::Uplo uplo, bool conjugate, Matrix<T, Device::CPU>& mat_a) {
  comm::CommunicatorGrid grid = comm::CommunicatorGrid::single();
  hermitian_complete<B, D, T>(grid, uplo, conjugate, mat_a);
}

// include/dlaf/eigensolver/gen_to_std.h:50, :101: A <- inv(L) A inv(L^H) (Lower) / inv(U^H) A inv(U) (Upper) with
// the Cholesky factor of B in mat_b (host-resident operands; only the uplo triangles are referenced)
namespace eigensolver::internal {
template <Backend B, class T>
void generalized_to_standard(comm::CommunicatorGrid& grid, blas::Uplo uplo, Matrix<T, Device::CPU>& mat_a,
                             Matrix<T, Device::CPU>& mat_b) {
  static_assert(B == Backend::GPU, "this library has no CPU backend");
  using dlaf::internal::descriptor_of;
  if (DLAF_MI355X_ENTRY(T, dlaf_mi355x_generalized_to_standard)(grid.context(), (char) uplo, mat_a.ptr(), descriptor_of(mat_a),
                                                                mat_b.ptr(), descriptor_of(mat_b)) != 0)
    dlaf::internal::fail("generalized_to_standard");
}
// device-resident operands (the reference's miniapp times exactly this: both mirrors on the device,
// miniapp_gen_to_std.cpp:119-140); mat_b holds the Cholesky factor, e.g. straight from cholesky_factorization
template <Backend B, class T>
void generalized_to_standard(comm::CommunicatorGrid& grid, blas::Uplo uplo, Matrix<T, Device::GPU>& mat_a,
                             Matrix<T, Device::GPU>& mat_b) {
  static_assert(B == Backend::GPU, "this library has no CPU backend");
  if (uplo != mat_a.uplo() || uplo != mat_b.uplo())
    dlaf::internal::fail("uplo of the call equals the uplo the device matrices were created with");
  if (grid.context() != mat_a.context() || grid.context() != mat_b.context())
    dlaf::internal::fail("matrix::equal_process_grid(mat_a, grid)");
  if (dlaf_mi355x_generalized_to_standard_device(mat_a.handle(), mat_b.handle()) != 0)
    dlaf::internal::fail("generalized_to_standard");
}
template <Backend B, class T>
void generalized_to_standard(blas::Uplo uplo, Matrix<T, Device::CPU>& mat_a, Matrix<T, Device::CPU>& mat_b) {
  comm::CommunicatorGrid grid = comm::CommunicatorGrid::single();
  generalized_to_standard<B, T>(grid, uplo, mat_a, mat_b);
}
}  // namespace eigensolver::internal

// dlaf::triangular_inverse (LAPACK xTRTRI) and dlaf::inverse_from_cholesky_factor (LAPACK xPOTRI), in place on the uplo
// triangle; local and grid forms, host- and device-resident operands.  They return LAPACK's info (the 1-based index of
// an exactly-zero diagonal element of a non-unit triangular operand, which is then untouched).
namespace internal {
template <class T>
int inverse_host(int ctx, blas::Uplo uplo, blas::Diag diag, bool product, Matrix<T, Device::CPU>& m) {
  const DLAF_descriptor desc = descriptor_of(m);
  return product ? DLAF_MI355X_ENTRY(T, dlaf_mi355x_inverse_from_cholesky_factor)(ctx, (char) uplo, m.ptr(), desc)
                 : DLAF_MI355X_ENTRY(T, dlaf_mi355x_triangular_inverse)(ctx, (char) uplo, (char) diag, m.ptr(), desc);
}
}  // namespace internal
template <Backend B, class T>
int triangular_inverse(comm::CommunicatorGrid& grid, blas::Uplo uplo, blas::Diag diag, Matrix<T, Device::CPU>& mat_a) {
  static_assert(B == Backend::GPU, "this library has no CPU backend");
  return internal::inverse_host<T>(grid.context(), uplo, diag, false, mat_a);
}
template <Backend B, class T>
int triangular_inverse(comm::CommunicatorGrid& grid, blas::Uplo uplo, blas::Diag diag, Matrix<T, Device::GPU>& mat_a) {
  static_assert(B == Backend::GPU, "this library has no CPU backend");
  if (grid.context() != mat_a.context())
    internal::fail("matrix::equal_process_grid(mat_a, grid)");
  return dlaf_mi355x_triangular_inverse_device((char) uplo, (char) diag, mat_a.handle());
}
template <Backend B, class T>
int triangular_inverse(blas::Uplo uplo, blas::Diag diag, Matrix<T, Device::CPU>& mat_a) {
  comm::CommunicatorGrid grid = comm::CommunicatorGrid::single();
  return triangular_inverse<B, T>(grid, uplo, diag, mat_a);
}
template <Backend B, class T>
int inverse_from_cholesky_factor(comm::CommunicatorGrid& grid, blas::Uplo uplo, Matrix<T, Device::CPU>& mat_a) {
  static_assert(B == Backend::GPU, "this library has no CPU backend");
  return internal::inverse_host<T>(grid.context(), uplo, blas::Diag::NonUnit, true, mat_a);
}
template <Backend B, class T>
int inverse_from_cholesky_factor(comm::CommunicatorGrid& grid, blas::Uplo uplo, Matrix<T, Device::GPU>& mat_a) {
  static_assert(B == Backend::GPU, "this library has no CPU backend");
  if (grid.context() != mat_a.context())
    internal::fail("matrix::equal_process_grid(mat_a, grid)");
  return dlaf_mi355x_inverse_from_cholesky_factor_device((char) uplo, mat_a.handle());
}
template <Backend B, class T>
int inverse_from_cholesky_factor(blas::Uplo uplo, Matrix<T, Device::CPU>& mat_a) {
  comm::CommunicatorGrid grid = comm::CommunicatorGrid::single();
  return inverse_from_cholesky_factor<B, T>(grid, uplo, mat_a);
}

// dlaf::auxiliary::max_norm (include/dlaf/auxiliary/norm.h) and its one / infinity / Frobenius siblings (LAPACK xLANGE,
// xLANHE / xLANSY, xLANTR).  The operand is only read.  The value comes back on EVERY rank (the reference defines it on
// `rank` alone), and Upper, which the reference leaves unimplemented, is built.
namespace lapack {
enum class Norm : char { One = '1', Inf = 'I', Fro = 'F', Max = 'M' };
}
namespace auxiliary {
namespace internal {
// structure 'G' / 'H' / 'T'
template <class T>
BaseType<T> norm_host(int ctx, lapack::Norm norm, char structure, blas::Uplo uplo, blas::Diag diag,
                      Matrix<T, Device::CPU>& m) {
  const DLAF_descriptor desc = dlaf::internal::descriptor_of(m);
  double v = 0;
  const char nc = (char) norm, uc = (char) uplo, dc = (char) diag;
  const int r = structure == 'G'   ? DLAF_MI355X_ENTRY(T, dlaf_mi355x_general_norm)(ctx, nc, m.ptr(), desc, &v)
                : structure == 'H' ? DLAF_MI355X_ENTRY(T, dlaf_mi355x_hermitian_norm)(ctx, nc, uc, m.ptr(), desc, &v)
                                   : DLAF_MI355X_ENTRY(T, dlaf_mi355x_triangular_norm)(ctx, nc, uc, dc, m.ptr(), desc, &v);
  if (r != 0)
    dlaf::internal::fail("norm: bad argument");
  return (BaseType<T>) v;
}
template <class T>
BaseType<T> norm_device(comm::CommunicatorGrid& grid, lapack::Norm norm, char structure, blas::Uplo uplo,
                        blas::Diag diag, Matrix<T, Device::GPU>& m) {
  if (grid.context() != m.context())
    dlaf::internal::fail("matrix::equal_process_grid(A, grid)");
  if (uplo != m.uplo())
    dlaf::internal::fail("a device matrix holds the triangle it was created with");
  double v = 0;
  if (dlaf_mi355x_matrix_norm(m.handle(), (char) norm, structure, (char) diag, &v) != 0)
    dlaf::internal::fail("norm: bad argument");
  return (BaseType<T>) v;
}
}  // namespace internal

// general matrix
template <Backend B, class T>
BaseType<T> norm(comm::CommunicatorGrid& grid, lapack::Norm norm_type, Matrix<T, Device::CPU>& A) {
  static_assert(B == Backend::GPU, "this library has no CPU backend");
  return internal::norm_host<T>(grid.context(), norm_type, 'G', blas::Uplo::General, blas::Diag::NonUnit, A);
}
// Hermitian (symmetric) matrix held in its uplo triangle
template <Backend B, class T>
BaseType<T> norm(comm::CommunicatorGrid& grid, lapack::Norm norm_type, blas::Uplo uplo, Matrix<T, Device::CPU>& A) {
  static_assert(B == Backend::GPU, "this library has no CPU backend");
  if (uplo == blas::Uplo::General)
    return norm<B, T>(grid, norm_type, A);
  return internal::norm_host<T>(grid.context(), norm_type, 'H', uplo, blas::Diag::NonUnit, A);
}
template <Backend B, class T>
BaseType<T> norm(comm::CommunicatorGrid& grid, lapack::Norm norm_type, blas::Uplo uplo, Matrix<T, Device::GPU>& A) {
  static_assert(B == Backend::GPU, "this library has no CPU backend");
  return internal::norm_device<T>(grid, norm_type, 'H', uplo, blas::Diag::NonUnit, A);
}
// triangular matrix held in its uplo triangle
template <Backend B, class T>
BaseType<T> norm(comm::CommunicatorGrid& grid, lapack::Norm norm_type, blas::Uplo uplo, blas::Diag diag,
                 Matrix<T, Device::CPU>& A) {
  static_assert(B == Backend::GPU, "this library has no CPU backend");
  return internal::norm_host<T>(grid.context(), norm_type, 'T', uplo, diag, A);
}
template <Backend B, class T>
BaseType<T> norm(comm::CommunicatorGrid& grid, lapack::Norm norm_type, blas::Uplo uplo, blas::Diag diag,
                 Matrix<T, Device::GPU>& A) {
  static_assert(B == Backend::GPU, "this library has no CPU backend");
  return internal::norm_device<T>(grid, norm_type, 'T', uplo, diag, A);
}

// max |a_ij| over the whole matrix (General) or over its uplo triangle (Lower, Upper)
template <Backend B, Device D, class T>
BaseType<T> max_norm(comm::CommunicatorGrid& grid, comm::Index2D /*rank*/, blas::Uplo uplo, Matrix<T, D>& A) {
  static_assert(B == Backend::GPU, "this library has no CPU backend");
  if constexpr (D == Device::CPU) {
    if (uplo == blas::Uplo::General)
      return norm<B, T>(grid, lapack::Norm::Max, A);
  }
  return norm<B, T>(grid, lapack::Norm::Max, uplo, blas::Diag::NonUnit, A);
}
}  // namespace auxiliary

// include/dlaf/eigensolver/reduction_to_band.h:40-122 and bt_reduction_to_band.h (first stage).
// The reference returns the taus as a Matrix<T, Device::CPU> distributed over the process columns; here every
// process gets all n - band_size - 1 of them as a std::vector (entry j belongs to the reflector in global column j).
inline SizeType get_band_size(SizeType nb) { return dlaf_mi355x_get_band_size((int) nb); }

// dlaf::getTuneParameters() (include/dlaf/tune.h:128-160): the parameters this build honours.  The reference's tests
// assign to the field (test/unit/eigensolver/test_eigensolver.cpp:142 `getTuneParameters().eigensolver_min_band = b_min`),
// so the field is a proxy onto the library's value.
struct TuneParameters {
  struct MinBand {
    operator SizeType() const { return dlaf_mi355x_get_eigensolver_min_band(); }
    MinBand& operator=(SizeType b_min) {
      dlaf_mi355x_set_eigensolver_min_band((int) b_min);
      return *this;
    }
  } eigensolver_min_band;
};
inline TuneParameters& getTuneParameters() {
  static TuneParameters params;
  return params;
}
namespace eigensolver::internal {
template <Backend B, class T>
std::vector<T> reduction_to_band(comm::CommunicatorGrid& grid, Matrix<T, Device::GPU>& mat_a, SizeType band_size) {
  static_assert(B == Backend::GPU, "this library has no CPU backend");
  if (mat_a.uplo() != blas::Uplo::Lower)
    dlaf::internal::fail("reduction_to_band references the lower triangle (reduction_to_band.h:66-68)");
  if (grid.context() != mat_a.context())
    dlaf::internal::fail("matrix::equal_process_grid(mat_a, grid)");
  const SizeType n = mat_a.size().rows();
  std::vector<T> taus((size_t) std::max<SizeType>(0, n - band_size - 1));
  if (dlaf_mi355x_reduction_to_band_device(mat_a.handle(), (int) band_size, taus.empty() ? nullptr : taus.data()) != 0)
    dlaf::internal::fail("reduction_to_band");
  return taus;
}
template <Backend B, class T>
std::vector<T> reduction_to_band(comm::CommunicatorGrid& grid, Matrix<T, Device::CPU>& mat_a, SizeType band_size) {
  static_assert(B == Backend::GPU, "this library has no CPU backend");
  std::vector<T> taus((size_t) std::max<SizeType>(0, mat_a.size().rows() - band_size - 1));
  T dummy{};
  T* tp = taus.empty() ? &dummy : taus.data();
  if (DLAF_MI355X_ENTRY(T, dlaf_mi355x_reduction_to_band)(grid.context(), mat_a.ptr(), dlaf::internal::descriptor_of(mat_a),
                                                          (int) band_size, tp) != 0)
    dlaf::internal::fail("reduction_to_band");
  return taus;
}
template <Backend B, class T>
std::vector<T> reduction_to_band(Matrix<T, Device::CPU>& mat_a, SizeType band_size) {
  comm::CommunicatorGrid grid = comm::CommunicatorGrid::single();
  return reduction_to_band<B, T>(grid, mat_a, band_size);
}
// C <- Q C (host-resident operands): mat_v = what reduction_to_band left, taus = what it returned
template <Backend B, class T>
void bt_reduction_to_band(comm::CommunicatorGrid& grid, SizeType band_size, Matrix<T, Device::CPU>& mat_c,
                          Matrix<T, Device::CPU>& mat_v, const std::vector<T>& taus) {
  static_assert(B == Backend::GPU, "this library has no CPU backend");
  using dlaf::internal::descriptor_of;
  T dummy{};
  const T* tp = taus.empty() ? &dummy : taus.data();
  if (DLAF_MI355X_ENTRY(T, dlaf_mi355x_bt_reduction_to_band)(grid.context(), (int) band_size, mat_c.ptr(),
                                                             descriptor_of(mat_c), mat_v.ptr(), descriptor_of(mat_v),
                                                             tp) != 0)
    dlaf::internal::fail("bt_reduction_to_band");
}
}  // namespace eigensolver::internal

// include/dlaf/eigensolver/eigensolver.h:56-190 and gen_eigensolver.h: host-resident matrices, as
// the reference's C entries take them.  eigenvalues: all n on every process (the reference returns a local N x 1 Matrix).
namespace internal {
// What every overload below does around its C call: `eigenvalues` gets its n entries (always_assign: zero-filled on every
// call, as the eigensolvers do; otherwise only when the size differs, as the eigenvalues-only calls do), then
// call(uplo, w) runs with the uplo character ('U' for anything but Lower) and the eigenvalue pointer (never null, n = 0
// included); a non-zero status fails as `what`.
template <class R, class Call>
void eigen_call(const char* what, blas::Uplo uplo, SizeType n, std::vector<R>& eigenvalues, bool always_assign,
                Call&& call) {
  if (always_assign || (SizeType) eigenvalues.size() != n)
    eigenvalues.assign((size_t) n, R(0));
  R dummy{};
  if (call(uplo == blas::Uplo::Lower ? 'L' : 'U', eigenvalues.empty() ? &dummy : eigenvalues.data()) != 0)
    fail(what);
}
}  // namespace internal
template <Backend B, class T>
void hermitian_eigensolver(comm::CommunicatorGrid& grid, blas::Uplo uplo, Matrix<T, Device::CPU>& mat,
                           std::vector<BaseType<T>>& eigenvalues, Matrix<T, Device::CPU>& eigenvectors) {
  static_assert(B == Backend::GPU, "this library has no CPU backend");
  using internal::descriptor_of;
  internal::eigen_call("hermitian_eigensolver", uplo, mat.size().rows(), eigenvalues, true, [&](char u, BaseType<T>* w) {
    return DLAF_MI355X_EIGEN_ENTRY(T, eigensolver)(grid.context(), u, mat.ptr(), descriptor_of(mat), w, eigenvectors.ptr(),
                                                   descriptor_of(eigenvectors));
  });
}
template <Backend B, class T>
void hermitian_generalized_eigensolver(comm::CommunicatorGrid& grid, blas::Uplo uplo, Matrix<T, Device::CPU>& mat_a,
                                       Matrix<T, Device::CPU>& mat_b, std::vector<BaseType<T>>& eigenvalues,
                                       Matrix<T, Device::CPU>& eigenvectors) {
  static_assert(B == Backend::GPU, "this library has no CPU backend");
  using internal::descriptor_of;
  internal::eigen_call("hermitian_generalized_eigensolver", uplo, mat_a.size().rows(), eigenvalues, true,
                       [&](char u, BaseType<T>* w) {
                         return DLAF_MI355X_EIGEN_ENTRY(T, generalized_eigensolver)(
                             grid.context(), u, mat_a.ptr(), descriptor_of(mat_a), mat_b.ptr(), descriptor_of(mat_b), w,
                             eigenvectors.ptr(), descriptor_of(eigenvectors));
                       });
}

// the eigenvectors of the eigenvalues [eigenvalues_index_begin, eigenvalues_index_end) only (0-based, half-open; the
// partial-spectrum overloads of later upstream releases): `eigenvalues` still receives all n, and only the global
// columns of that range are written in `eigenvectors`
template <Backend B, class T>
void hermitian_eigensolver(comm::CommunicatorGrid& grid, blas::Uplo uplo, Matrix<T, Device::CPU>& mat,
                           std::vector<BaseType<T>>& eigenvalues, Matrix<T, Device::CPU>& eigenvectors,
                           SizeType eigenvalues_index_begin, SizeType eigenvalues_index_end) {
  static_assert(B == Backend::GPU, "this library has no CPU backend");
  using internal::descriptor_of;
  const int64_t ib = eigenvalues_index_begin, ie = eigenvalues_index_end;
  internal::eigen_call("hermitian_eigensolver", uplo, mat.size().rows(), eigenvalues, true, [&](char u, BaseType<T>* w) {
    return DLAF_MI355X_EIGEN_ENTRY(T, eigensolver_partial_spectrum)(grid.context(), u, mat.ptr(), descriptor_of(mat), w,
                                                                    eigenvectors.ptr(), descriptor_of(eigenvectors), ib, ie);
  });
}
template <Backend B, class T>
void hermitian_generalized_eigensolver(comm::CommunicatorGrid& grid, blas::Uplo uplo, Matrix<T, Device::CPU>& mat_a,
                                       Matrix<T, Device::CPU>& mat_b, std::vector<BaseType<T>>& eigenvalues,
                                       Matrix<T, Device::CPU>& eigenvectors, SizeType eigenvalues_index_begin,
                                       SizeType eigenvalues_index_end) {
  static_assert(B == Backend::GPU, "this library has no CPU backend");
  using internal::descriptor_of;
  const int64_t ib = eigenvalues_index_begin, ie = eigenvalues_index_end;
  internal::eigen_call("hermitian_generalized_eigensolver", uplo, mat_a.size().rows(), eigenvalues, true,
                       [&](char u, BaseType<T>* w) {
                         return DLAF_MI355X_EIGEN_ENTRY(T, generalized_eigensolver_partial_spectrum)(
                             grid.context(), u, mat_a.ptr(), descriptor_of(mat_a), mat_b.ptr(), descriptor_of(mat_b), w,
                             eigenvectors.ptr(), descriptor_of(eigenvectors), ib, ie);
                       });
}

// the eigenpairs with eigenvalues in (vl, vu] (LAPACK's range = 'V'): the index range is found from two Sturm counts of
// the tridiagonal matrix and returned as {begin, end}; everything else as in the overloads above for that range.  An
// eigenvalue within rounding of vl or vu may fall on either side.
template <class R>
struct EigenvaluesValue {
  R vl, vu;
};
template <Backend B, class T>
std::pair<SizeType, SizeType> hermitian_eigensolver(comm::CommunicatorGrid& grid, blas::Uplo uplo, Matrix<T, Device::CPU>& mat,
                                                    std::vector<BaseType<T>>& eigenvalues,
                                                    Matrix<T, Device::CPU>& eigenvectors,
                                                    EigenvaluesValue<BaseType<T>> eigenvalues_value) {
  static_assert(B == Backend::GPU, "this library has no CPU backend");
  using internal::descriptor_of;
  long ib = 0, ie = 0;
  internal::eigen_call("hermitian_eigensolver", uplo, mat.size().rows(), eigenvalues, true, [&](char u, BaseType<T>* w) {
    return DLAF_MI355X_EIGEN_ENTRY(T, eigensolver_partial_spectrum_by_value)(
        grid.context(), u, mat.ptr(), descriptor_of(mat), w, eigenvectors.ptr(), descriptor_of(eigenvectors),
        eigenvalues_value.vl, eigenvalues_value.vu, &ib, &ie);
  });
  return {(SizeType) ib, (SizeType) ie};
}
template <Backend B, class T>
std::pair<SizeType, SizeType> hermitian_generalized_eigensolver(comm::CommunicatorGrid& grid, blas::Uplo uplo,
                                                                Matrix<T, Device::CPU>& mat_a, Matrix<T, Device::CPU>& mat_b,
                                                                std::vector<BaseType<T>>& eigenvalues,
                                                                Matrix<T, Device::CPU>& eigenvectors,
                                                                EigenvaluesValue<BaseType<T>> eigenvalues_value) {
  static_assert(B == Backend::GPU, "this library has no CPU backend");
  using internal::descriptor_of;
  long ib = 0, ie = 0;
  internal::eigen_call("hermitian_generalized_eigensolver", uplo, mat_a.size().rows(), eigenvalues, true,
                       [&](char u, BaseType<T>* w) {
                         return DLAF_MI355X_EIGEN_ENTRY(T, generalized_eigensolver_partial_spectrum_by_value)(
                             grid.context(), u, mat_a.ptr(), descriptor_of(mat_a), mat_b.ptr(), descriptor_of(mat_b), w,
                             eigenvectors.ptr(), descriptor_of(eigenvectors), eigenvalues_value.vl, eigenvalues_value.vu,
                             &ib, &ie);
                       });
  return {(SizeType) ib, (SizeType) ie};
}

// Eigenvalues only: reduction_to_band, band_to_tridiagonal and bisection on Sturm counts for the eigenvalues
// [eigenvalues_index_begin, eigenvalues_index_end) (0-based, half-open; a negative end: all n).  No eigenvector matrix
// exists anywhere.  `eigenvalues` is resized to n when its size differs (new entries zero) and only the entries of the
// range are written; mat (mat_a) is read only; mat_b ends up holding its Cholesky factor.
template <Backend B, class T>
void hermitian_eigenvalues(comm::CommunicatorGrid& grid, blas::Uplo uplo, const Matrix<T, Device::CPU>& mat,
                           std::vector<BaseType<T>>& eigenvalues, SizeType eigenvalues_index_begin = 0,
                           SizeType eigenvalues_index_end = -1) {
  static_assert(B == Backend::GPU, "this library has no CPU backend");
  const SizeType n = mat.size().rows();
  const int64_t ib = eigenvalues_index_begin, ie = eigenvalues_index_end < 0 ? n : eigenvalues_index_end;
  internal::eigen_call("hermitian_eigenvalues", uplo, n, eigenvalues, false, [&](char u, BaseType<T>* w) {
    return DLAF_MI355X_EIGEN_ENTRY(T, eigenvalues)(grid.context(), u, mat.ptr(), internal::descriptor_of(mat), w, ib, ie);
  });
}
template <Backend B, class T>
void hermitian_generalized_eigenvalues(comm::CommunicatorGrid& grid, blas::Uplo uplo, const Matrix<T, Device::CPU>& mat_a,
                                       Matrix<T, Device::CPU>& mat_b, std::vector<BaseType<T>>& eigenvalues,
                                       SizeType eigenvalues_index_begin = 0, SizeType eigenvalues_index_end = -1) {
  static_assert(B == Backend::GPU, "this library has no CPU backend");
  using internal::descriptor_of;
  const SizeType n = mat_a.size().rows();
  const int64_t ib = eigenvalues_index_begin, ie = eigenvalues_index_end < 0 ? n : eigenvalues_index_end;
  internal::eigen_call("hermitian_generalized_eigenvalues", uplo, n, eigenvalues, false, [&](char u, BaseType<T>* w) {
    return DLAF_MI355X_EIGEN_ENTRY(T, generalized_eigenvalues)(grid.context(), u, mat_a.ptr(), descriptor_of(mat_a),
                                                               mat_b.ptr(), descriptor_of(mat_b), w, ib, ie);
  });
}

// include/dlaf/init.h: the library needs no runtime arguments; initialize / finalize are idempotent
inline void initialize(int argc = 0, const char** argv = nullptr) { dlaf_initialize(argc, argv, 0, nullptr); }
inline void finalize() { dlaf_finalize(); }

}  // namespace dlaf

#undef DLAF_MI355X_ENTRY
#undef DLAF_MI355X_EIGEN_ENTRY
