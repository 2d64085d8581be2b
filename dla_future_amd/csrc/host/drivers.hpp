// drivers.hpp -- what the algorithms on top of the tile kernels export: the triangular solver (solver.cpp), the
// triangular, Hermitian and general multiplications (multiplication.cpp), the rank updates (rank_update.cpp), the addition / transposition (addition.cpp),
// generalized-to-standard (gen_to_std.cpp), the inverses (inverse.cpp) and the norms (norm.cpp), host and
// device-resident forms.  reduction_to_band and the eigensolver stages have headers of their own (red2band.hpp,
// eigensolver.hpp).  A further family is written on three shared pieces: its sweep on sweep.hpp (Sweep, Ring, the
// one-step-ahead StepPipeline, bcast_view_column / bcast_column_and_transposed_panel), its host form on the host scope --
// checked_transport (transport.hpp) after the quick returns, then a ScratchStream (pool.hpp) declared before the
// matrices it serves.
//
// Every matrix of a _host driver is a HostOperand (host_operand.hpp): this process's local column-major part with the
// matrix's global description as stored -- size, blocks, source process.  A driver reads every size from its operands
// (the k of a product is op(A)'s inner extent, the free block of a right-hand side is B's own) and trusts them: the
// entries judge them first, each family with its one require_* function (api_checks.hpp).
#pragma once
#include "device_matrix.hpp"
#include "host_operand.hpp"

namespace dlaf_mi355x {

template <class T>
struct TileMatrix;  // (tile_matrix.hpp)

// op(A) X = alpha B (side L) / X op(A) = alpha B (side R) on the grid, host operands (solver.cpp): a the triangular
// matrix with one square block, b the m x n matrix, overwritten; b's block along the triangular dimension is a's, the
// other one is its own.  The arguments must have passed require_triangular (api_checks.hpp).
template <class T>
int triangular_solver_host(Grid* g, char side, char uplo, char op, char diag, T alpha, HostOperand<const T> a,
                           HostOperand<T> b);

void solver_last_profile(double* ms, double* flops);

// Device-resident operands for the solver (solver.cpp): a general m x n matrix in tile layout behind a MatrixBase
// handle, and dlaf::triangular_solver on a resident triangular matrix (a DeviceMatrix, e.g. the factor p?potrf left
// there) and a resident right-hand side -- no PCIe traffic.
MatrixBase* general_matrix_create(Grid* g, char type, long m, long n, int nb, int isrc, int jsrc);
void general_matrix_transfer(MatrixBase* h, void* host, long ld, bool upload);
int triangular_solver_device(char side, char uplo, char op, char diag, const void* alpha, MatrixBase* a, MatrixBase* b);

// B = alpha op(A) B (side L) / B = alpha B op(A) (side R) on the grid (multiplication.cpp): the arguments and the
// operand mapping of triangular_solver_host (require_triangular too), host and resident forms; device time of the
// last sweep
template <class T>
int triangular_multiplication_host(Grid* g, char side, char uplo, char op, char diag, T alpha, HostOperand<const T> a,
                                   HostOperand<T> b);
int triangular_multiplication_device(char side, char uplo, char op, char diag, const void* alpha, MatrixBase* a,
                                     MatrixBase* b);
// device time and whole-grid flops of the last sweep of ANY multiplication (triangular, Hermitian, general, rank update) on
// this process; set_profile: how a sweep outside multiplication.cpp (rank_update.cpp) reports its own
void multiplication_last_profile(double* ms, double* flops);
void multiplication_set_profile(double ms, double flops);

// C = beta C + alpha A B (side L) / beta C + alpha B A (side R), A Hermitian with only its uplo triangle read
// (multiplication.cpp; dlaf::hermitian_multiplication, every side x uplo).  b and c are described alike; their block
// along A's dimension is a's square block, the other one is their own.  The arguments must have passed
// require_hermitian_multiplication (api_checks.hpp).  Host and resident forms.
template <class T>
int hermitian_multiplication_host(Grid* g, char side, char uplo, T alpha, HostOperand<const T> a, HostOperand<const T> b,
                                  T beta, HostOperand<T> c);
int hermitian_multiplication_device(char side, char uplo, const void* alpha, MatrixBase* a, MatrixBase* b,
                                    const void* beta, MatrixBase* c);

// C = beta C + alpha op(A) op(B) (multiplication.cpp; dlaf::multiplication::internal::generalMatrix, every op pair on
// one process, N x N on a grid).  a, b, c: the matrices as stored (A m x k or k x m, B k x n or n x k), one square block
// nb.  The arguments must have passed require_general_multiplication (api_checks.hpp).  Host and resident forms.
template <class T>
int general_multiplication_host(Grid* g, char opa, char opb, T alpha, HostOperand<const T> a, HostOperand<const T> b,
                                T beta, HostOperand<T> c);
int general_multiplication_device(char opa, char opb, const void* alpha, MatrixBase* a, MatrixBase* b, const void* beta,
                                  MatrixBase* c);

// Hermitian rank-k (b null) / rank-2k update of the uplo triangle of C (rank_update.cpp; xSYRK / xHERK, xSYR2K /
// xHER2K): C = alpha A A^H + beta C (trans N, A n x k) / alpha A^H A + beta C (trans C, A k x n); her2k: alpha A B^H +
// conj(alpha) B A^H + beta C / alpha A^H B + conj(alpha) B^H A + beta C, B stored, blocked and distributed like A.  alpha
// of herk is real (im 0), beta is real.  The other triangle is never referenced; the imaginary part of C's diagonal is
// ignored on entry and 0 on exit; beta == 0: C is not read; alpha == 0 or k == 0: A and B are not referenced, and with
// beta == 1 nothing is touched.  Trans N on any grid, trans C on one process.  The arguments must have passed
// require_rank_update (api_checks.hpp).  Host and resident forms (resident: C a DeviceMatrix whose stored triangle is
// uplo, a / b general matrices, b null for herk; alpha points to a real for herk, to an element for her2k).
// d (herk only; null: the plain update): the weighted update  C = alpha A D A^H + beta C (trans N) / alpha A^H D A + beta C
// (trans C), D = diag(d) REAL of any sign -- a HOST array of k reals, the same on every rank (the caller's duty, as for
// alpha), uploaded once; the kernel multiplies d into one operand between its global load and its LDS image, no scaled
// copy of A exists.  herk's semantics hold; alpha == 0 or k == 0: d is not referenced either.  A zero weight does NOT
// unreference its column (0 * NaN is NaN); non-finite weights are not judged.  The arguments must have passed
// require_weighted_rank_update.
template <class T>
int hermitian_rank_update_host(Grid* g, char uplo, char trans, T alpha, HostOperand<const T> a,
                               const HostOperand<const T>* b, real_t<T> beta, HostOperand<T> c,
                               const real_t<T>* d = nullptr);
int hermitian_rank_update_device(char trans, const void* alpha, MatrixBase* a, MatrixBase* b, const void* beta,
                                 MatrixBase* c, const void* d = nullptr);
// C = alpha A D A^H + beta C on a resident C (stored triangle: its own) and ALL k columns of the resident tile matrix A
// (on C's grid and row source): the synthesis step of matrix_function.cpp
template <class T>
void hermitian_weighted_update_resident(DeviceMatrix<T>& C, TileMatrix<T>& A, const real_t<T>* d_host, long k, T alpha,
                                        real_t<T> beta);

// Functions of a Hermitian matrix (matrix_function.cpp): the uplo ('L': what the eigensolver takes) triangle of the
// resident A becomes that of  sum_{j selected} g_j z_j z_j^H  with (w, Z) A's eigenpairs and g = weights(w): the
// eigensolver on A (hermitian_eigensolver_device: all pairs, the index range [begin, end), or, by_value, the value
// interval (vl, vu]), ONE call of `weights` on the host with all n eigenvalues and the selected range -- it fills
// g[begin, end) --, then the weighted update with trans N, beta = 0 into A itself; Z never leaves HBM.  Unselected
// eigenvalues weigh 0 by definition and their eigenvectors are never computed; an empty selection gives a zero triangle.
// w_host: all n eigenvalues.  Returns the eigensolver's status (agreed over the grid); non-zero: A holds what the
// eigensolver left and the host form leaves the caller's array unchanged.  The host form downloads the triangle alone.
using SpectralWeights = void (*)(long n, const void* w, long begin, long end, void* g, void* user);
template <class T>
int hermitian_function_resident(DeviceMatrix<T>& A, real_t<T>* w_host, const real_t<T>* by_value, long& begin, long& end,
                                SpectralWeights weights, void* user);
template <class T>
int hermitian_function_host(Grid* g, char uplo, HostOperand<T> a, real_t<T>* w_host, const real_t<T>* by_value, long& begin,
                            long& end, SpectralWeights weights, void* user);

// C = beta C + alpha op(A) on the uplo part (A all, L i >= j, U i <= j) of the m x n matrix C (addition.cpp; PBLAS p?geadd /
// p?tradd, p?tran / p?tranu / p?tranc, ScaLAPACK p?lacpy): op N, T, C; A as stored, m x n for N and n x m for T / C, one
// square block nb.  Outside the part C stays bit for bit, the padding rows of ldc too; A is only read; beta == 0: C is
// not read; alpha == 0: A is not referenced, and with beta == 1 nothing is touched; alpha == 1, beta == 0, op N / T: a bit
// copy.  The arguments must have passed require_general_addition (api_checks.hpp).  Host and resident forms (resident:
// two general matrices; the same handle twice is op N in place).
template <class T>
int general_addition_host(Grid* g, char uplo, char op, T alpha, HostOperand<const T> a, T beta, HostOperand<T> c);
int general_addition_device(char uplo, char op, const void* alpha, MatrixBase* a, const void* beta, MatrixBase* c);
// The other triangle of the n x n general matrix A from its uplo one, in place: kind H the conjugated mirror and the
// diagonal's imaginary parts exactly 0, kind S the plain transpose and the diagonal untouched.  The arguments must have
// passed require_hermitian_complete.  Host and resident (a general matrix) forms.
template <class T>
int hermitian_complete_host(Grid* g, char uplo, char kind, HostOperand<T> a);
int hermitian_complete_device(char uplo, char kind, MatrixBase* general_matrix);
// Resident conversions, defined by what download() of either object shows: to_general writes into the general matrix g
// the Hermitian (kind H) / symmetric (S) matrix whose stored triangle m holds, or the triangular one (T: exact zeros in
// the other triangle); from_general takes m's stored triangle from g.  Same grid, order, block and source process (the
// entry checks).
int matrix_to_general(char kind, MatrixBase* m, MatrixBase* g);
int matrix_from_general(MatrixBase* m, MatrixBase* g);
// device time and whole-grid algorithmic bytes (read A + write C, + read C when beta != 0; a completion reads and writes
// half the matrix) of the last of them on this process
void addition_last_profile(double* ms, double* bytes);

// A <- L^-1 A L^-H (uplo L) / U^-H A U^-1 (uplo U) with the Cholesky factor held in the same uplo triangle of
// `l` (gen_to_std.cpp; dlaf::eigensolver::internal::generalized_to_standard); device-resident and host forms (a and l
// square, described alike)
template <class T>
int gen_to_std_device(DeviceMatrix<T>& a, DeviceMatrix<T>& l);
template <class T>
int gen_to_std_host(Grid* g, char uplo, HostOperand<T> a, HostOperand<const T> l);

// A <- A^-1 for the triangular matrix in A's uplo triangle (diag N / U), and the uplo triangle of (L L^H)^-1 /
// (U^H U)^-1 from the Cholesky factor held there (inverse.cpp; LAPACK xTRTRI / xPOTRI), in place; device-resident and
// host forms.  Return LAPACK's info: the 1-based index of the first exactly-zero diagonal element (nothing is written
// then), the same on every rank.
template <class T>
int triangular_inverse_device(char diag, DeviceMatrix<T>& a);
template <class T>
int inverse_from_cholesky_factor_device(DeviceMatrix<T>& a);
template <class T>
int triangular_inverse_host(Grid* g, char uplo, char diag, HostOperand<T> a);
template <class T>
int inverse_from_cholesky_factor_host(Grid* g, char uplo, HostOperand<T> a);
// device time and whole-grid flops (n^3 / 3 per half, x 4 for complex types) of the last of them on this process
void inverse_last_profile(double* ms, double* flops);
// index arithmetic of the two sweeps (exported for the host-logic tests)
struct DiagTiles {
  long count;             // local diagonal tiles: global k0 + m kstep at local (il0 + m il_step, jl0 + m jl_step)
  long k0, kstep;
  long il0, jl0, il_step, jl_step;
  int last;               // extent of the last of them
};
DiagTiles local_diag_tiles(const Axis& rows, const Axis& cols);
struct InverseStep {
  int own_r, own_c;       // owner of the diagonal tile k
  long il_below;          // first local tile row below k
  long nrl, ncl;          // local tile rows / columns before k
  long lr, lc;            // local index of tile row / column k (-1: elsewhere)
};
InverseStep inverse_step_ranges(const Axis& rows, const Axis& cols, long k);
long inverse_workspace_tiles(const Axis& rows, const Axis& cols);

// Max / one / infinity / Frobenius norm (norm.cpp; LAPACK xLANGE, xLANHE / xLANSY, xLANTR): norm letters M, 1 / O, I,
// F / E in either case; structure 'G' general, 'H' Hermitian / symmetric from the uplo triangle, 'T' triangular from the
// uplo triangle with diag N / U.  The operand is only read.  Host forms upload this process's local column-major part
// and write nothing back; the value -- for s / c the float result widened -- is the same bits on every rank.
// norm_kind: the canonical letter (M, 1, I, F) of a norm letter, 0 for any other character.
char norm_kind(char norm);
template <class T>
double general_norm_host(Grid* g, char norm, HostOperand<const T> a);
template <class T>
double structured_norm_host(Grid* g, char norm, char structure, char uplo, char diag, HostOperand<const T> a);
template <class T>
double structured_norm_device(char norm, char structure, char diag, const DeviceMatrix<T>& a);
double general_norm_device(char norm, MatrixBase* general_matrix);
// device time and the bytes of the referenced tiles (diagonal tiles whole) of the last norm on this process
void norm_last_profile(double* ms, double* bytes);

}  // namespace dlaf_mi355x
