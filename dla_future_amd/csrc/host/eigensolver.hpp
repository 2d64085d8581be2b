// eigensolver.hpp -- the stages of the Hermitian eigensolver behind reduction_to_band (eigensolver.cpp, tridiag_dc.cpp):
// band -> tridiagonal, tridiagonal eigensolver, back-transformation band <- tridiagonal, and the drivers
// (include/dlaf/eigensolver/eigensolver/impl.h:38-55).
#pragma once
#include <memory>

#include "device_matrix.hpp"
#include "red2band.hpp"
#include "tile_matrix.hpp"

namespace dlaf_mi355x {

// band_to_tridiagonal (include/dlaf/eigensolver/band_to_tridiag.h:74-97, :155-176): A (uplo L, tile layout) holds a
// Hermitian band matrix in its lower band (what reduction_to_band leaves).  Device outputs: d, e (n reals each, e[n-1]
// = 0), v (n x n, ldv): the compact Householder reflectors with tau in the place of the leading 1.  On a process grid
// every rank ends up with the whole result (the band is summed over the grid, the chase runs replicated).
// In the _host drivers of this header a distributed matrix is a HostOperand (host_operand.hpp): this process's local
// column-major part with the matrix's global size, square block and source process, as the entries have judged it
// (c_api_host.cpp); d, e, w and the reflector matrix v are plain arrays.
template <class T>
int band_to_tridiag_device(DeviceMatrix<T>& a, int band, real_t<T>* d, real_t<T>* e, T* v, long ldv);
template <class T>
int band_to_tridiag_host(Grid* g, HostOperand<const T> a, int band, real_t<T>* d, real_t<T>* e, T* v, long ldv);

// bt_band_to_tridiagonal (include/dlaf/eigensolver/bt_band_to_tridiag.h:28-61): E <- Q E on the rows of a
// column-major device array e (n x ncols, lde); v as band_to_tridiag_device left it.
template <class T>
int bt_band_to_tridiag_device(long n, int band, const T* v, long ldv, T* e, long lde, long ncols, hipStream_t s);
template <class T>
int bt_band_to_tridiag_host(long n, int band, const T* v, long ldv, T* e, long lde, long ncols);

// tridiagonal_eigensolver (include/dlaf/eigensolver/tridiag_solver.h:30-60): d, e (device, n; e[n-1] unused) ->
// eigenvalues w (device, n, ascending) and eigenvectors z (device, column-major n x n, ldz).  nb = the leaf size of the
// divide & conquer tree (the block size of the reference's distribution, tridiag_solver/impl.h:198-262).
// [begin, end): the 0-based range of eigenvalue indices whose eigenvectors are wanted; w always receives all n
// eigenvalues, z is n x (end - begin) and column j holds the eigenvector of eigenvalue begin + j.
template <class R>
int tridiag_solver_device(long n, int nb, R* d, R* e, R* w, R* z, long ldz, long begin, long end, hipStream_t s,
                          Transport* tr = nullptr);
template <class R>
int tridiag_solver_host(long n, int nb, const R* d, const R* e, R* w, R* z, long ldz, long begin, long end);

// Hermitian eigensolver, Eigensolver::call (eigensolver/impl.h:38-55, :57-95): a (lower triangle referenced,
// destroyed), eigenvalues w (all n on every rank), eigenvectors z (a general n x n matrix with a's block and its own
// source process, whose row must be a's).  [begin, end): the 0-based range of eigenvalue indices whose eigenvectors
// are computed; global column j of z, j in [begin, end), receives the eigenvector of eigenvalue j and nothing else of
// z is written.
template <class T>
int hermitian_eigensolver_host(Grid* g, char uplo, HostOperand<T> a, real_t<T>* w, HostOperand<T> z, long begin, long end);
// Hermitian generalized eigensolver A x = lambda B x, GenEigensolver::call (gen_eigensolver/impl.h:33-92); a, b and z
// share their source process
template <class T>
int hermitian_gen_eigensolver_host(Grid* g, char uplo, HostOperand<T> a, HostOperand<T> b, real_t<T>* w, HostOperand<T> z,
                                   bool b_factorized, long begin, long end);

// The same with the eigenvalue range given by value, LAPACK's range = 'V': the eigenpairs in (vl, vu].  After
// band_to_tridiagonal the drivers take [begin, end) = [count(vl), count(vu)) from two Sturm counts of the computed
// tridiagonal matrix (vl >= vu: the empty range at count(vl)), return it, and go on exactly as the entries above do
// for that index range.  An eigenvalue within rounding of vl or vu may fall on either side.
template <class T>
int hermitian_eigensolver_by_value_host(Grid* g, char uplo, HostOperand<T> a, real_t<T>* w, HostOperand<T> z, real_t<T> vl,
                                        real_t<T> vu, long* begin, long* end);
template <class T>
int hermitian_gen_eigensolver_by_value_host(Grid* g, char uplo, HostOperand<T> a, HostOperand<T> b, real_t<T>* w,
                                            HostOperand<T> z, bool b_factorized, real_t<T> vl, real_t<T> vu, long* begin,
                                            long* end);

// Eigenvalues only: reduction_to_band, band_to_tridiagonal, bisection for the eigenvalues [begin, end) (0-based,
// half-open).  w[begin, end) is written (the same on every rank) and nothing else; a is read only (its resident copy is
// destroyed); the generalized form leaves the Cholesky factor in b as the eigensolver does.  No divide & conquer, no
// back-transformation, no eigenvector matrix: the replicated memory is the n x n reflector matrix alone.
template <class T>
int hermitian_eigenvalues_host(Grid* g, char uplo, HostOperand<const T> a, real_t<T>* w, long begin, long end);
template <class T>
int hermitian_gen_eigenvalues_host(Grid* g, char uplo, HostOperand<const T> a, HostOperand<T> b, real_t<T>* w,
                                   bool b_factorized, long begin, long end);

// Eigenvalues of the symmetric tridiagonal matrix d (n), e (n - 1) by bisection on Sturm counts (kernels_sturm.hip).
// _device: d, e, w on the device, work = sturm_work_doubles(n) doubles; enqueues on s and returns.  Only w[begin, end)
// is written.  sturm_count: counts[i] = the number of eigenvalues <= shifts[i] (-1 when d or e is not finite); the
// _device form takes d, e on the device and host shifts / counts, and waits for the stream.
template <class R>
void tridiag_eigenvalues_device(long n, const R* d, const R* e, R* w, long begin, long end, double* work, hipStream_t s);
template <class R>
int tridiag_eigenvalues_host(long n, const R* d, const R* e, R* w, long begin, long end);
template <class R>
void sturm_count_device(long n, const R* d, const R* e, const R* shifts_host, long nshifts, long* counts_host,
                        hipStream_t s);
template <class R>
int sturm_count_host(long n, const R* d, const R* e, long nshifts, const R* shifts, long* counts);
// d, e of a host tridiagonal matrix on the device, in workspaces of ws (e padded to n entries); enqueues on s
template <class R>
void upload_tridiag(PoolScope& ws, long n, const R* d, const R* e, R*& dd, R*& de, hipStream_t s);

// Index arithmetic of a partial spectrum.  The drivers hold the eigenvectors of [begin, end) in an internal matrix that
// covers the global columns [b0, end), b0 = (begin / nb) nb: whole tile columns are dropped in front of it, so its local
// columns are a contiguous run of the caller's local columns, and the columns [b0, begin) are zero padding that is
// never written back.
struct PartialSpectrumPlan {
  long b0;          // first global column of the internal matrix
  int jsrc;         // its column source rank
  long ncl;         // this process column's local columns of the internal matrix
  long first;       // the caller's local column its local column 0 corresponds to
  long pad;         // how many of its leading local columns are padding
};
// 0 <= begin <= end <= n, or fatal (before anything touches the GPU)
void check_eigenvalues_index(const char* who, long n, long begin, long end);
PartialSpectrumPlan partial_spectrum_plan(long n, int nb, int npcol, int mycol, int z_jsrc, long begin, long end);

// The eigensolver on a RESIDENT A (an uplo 'L' DeviceMatrix, destroyed): w_host receives all n eigenvalues; zh the
// internal general matrix (n x (end - pl.b0), A's grid, block and row source, resident) whose columns behind the zero
// padding [pl.b0, begin) are the eigenvectors of [begin, end).  by_value = {vl, vu}: the range is found and returned as
// the _by_value_host entries do.  Returns the status agreed over the grid.  (matrix_function.cpp builds on it.)
template <class T>
int hermitian_eigensolver_resident(DeviceMatrix<T>& A, real_t<T>* w_host, const real_t<T>* by_value, long& begin, long& end,
                                   std::unique_ptr<MatrixBase>& zh, PartialSpectrumPlan& pl);

// per-stage device times (ms) of the last eigensolver call on this process:
// 0 reduction_to_band, 1 band_to_tridiagonal, 2 tridiagonal solver (the bisection of an eigenvalues-only call),
// 3 bt_band_to_tridiagonal, 4 bt_reduction_to_band (both 0 after an eigenvalues-only call)
void eigensolver_last_profile(double ms[5]);

}  // namespace dlaf_mi355x
