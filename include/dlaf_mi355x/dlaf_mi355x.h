/* dlaf_mi355x.h -- extensions of the C interface that the MI355X build adds next to the
 * reference's dlaf_c/ headers.  Plain C ABI: pointers, sizes, chars; no C++ or torch types.
 *
 *   - MPI-free grids over RCCL/xGMI or over caller-supplied host broadcasts,
 *   - a device-resident matrix handle so a driver can time the factorization with the matrix
 *     already in HBM (what the reference's miniapp does with MatrixMirror,
 *     miniapp/miniapp_cholesky.cpp:133-155),
 *   - the synthetic input of the miniapp (include/dlaf/util_matrix.h:498-501),
 *   - the four tile operations with exactly the argument sets the factorization issues
 *     (include/dlaf/factorization/cholesky/impl.h:45-147), for known-answer tests,
 *   - the 2-D block-cyclic index helpers (include/dlaf/matrix/util_distribution.h:82-196).
 *
 * type is one of 's' 'd' 'c' 'z'; uplo 'L' or 'U'.  Functions returning int return 0 on success,
 * a negative value for an invalid argument, or a positive LAPACK info. */
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <dlaf_c/desc.h>
#include <dlaf_c/utils.h>

/* ---- grids --------------------------------------------------------------------------------- */
/* 1x1 grid in this process (no communication).  Returns a context. */
DLAF_EXTERN_C int dlaf_mi355x_create_grid_single(void) DLAF_NOEXCEPT;

/* RCCL: rank 0 calls dlaf_mi355x_rccl_unique_id and ships the 128 bytes to every rank by any
 * means (torch.distributed, MPI, a file); then every rank calls dlaf_mi355x_create_grid_rccl.
 * order 'R': rank = myrow*npcol + mycol, 'C': rank = mycol*nprow + myrow
 * (reference: common/index2d.h:345-355, dlaf_create_grid's order argument). */
#define DLAF_MI355X_UNIQUE_ID_BYTES 128
DLAF_EXTERN_C void dlaf_mi355x_rccl_unique_id(void* out_128_bytes) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_create_grid_rccl(const void* unique_id_128_bytes, int nranks, int rank, int nprow,
                                               int npcol, char order) DLAF_NOEXCEPT;

/* Host-staged transport: the library hands a pinned HOST buffer to `bcast`, which must broadcast
 * it from member `root` of this process's row (axis 0) or column (axis 1) communicator -- root is
 * the process column index for axis 0 and the process row index for axis 1 -- and return 0. */
typedef int (*dlaf_mi355x_bcast_fn)(void* user, int axis, int root, void* host_buf, size_t bytes);
typedef int (*dlaf_mi355x_barrier_fn)(void* user);
DLAF_EXTERN_C int dlaf_mi355x_create_grid_host(int nranks, int rank, int nprow, int npcol, char order,
                                               dlaf_mi355x_bcast_fn bcast, dlaf_mi355x_barrier_fn barrier,
                                               void* user) DLAF_NOEXCEPT;

/* Runs the grid's broadcast callback on a caller-owned HOST buffer (no GPU work): a wiring check of
 * the row (axis 0) / column (axis 1) communicators of a host grid for CPU-only tests. */
DLAF_EXTERN_C int dlaf_mi355x_grid_host_bcast(int context, int axis, int root, void* host_buf, size_t bytes) DLAF_NOEXCEPT;

/* fn(user) is called once when the grid is freed (dlaf_free_grid / dlaf_finalize): the creator of a host
 * grid releases there what its callbacks use (the MPI shim frees its communicators).  -1: unknown context. */
DLAF_EXTERN_C int dlaf_mi355x_grid_on_free(int context, void (*fn)(void*), void* user) DLAF_NOEXCEPT;
/* Moves a registered grid to the context number `new_ctx` (0: done, -1: unknown ctx, -2: new_ctx is taken).  The
 * MPI shim uses it for dlaf_create_grid_from_blacs, whose grids are looked up by the caller's BLACS context
 * (reference: src/c_api/grid.cpp:73-92 registers the grid under blacs_ctxt). */
DLAF_EXTERN_C int dlaf_mi355x_grid_rekey(int ctx, int new_ctx) DLAF_NOEXCEPT;

/* Communication log of a grid (test instrument): while enabled, every broadcast / barrier / all-reduce the
 * library issues on this grid and a marker per factorization step are appended to a per-process list of
 * events {kind, root, bytes, grouped}: kind 0 row broadcast, 1 column broadcast (root = index inside that
 * communicator), 2 step marker (root = step), 3 barrier, 4 all-reduce.  Every member of a communicator must
 * log the same sequence for it -- the property the reference's communicator pipeline enforces
 * (sender/transform_mpi.h:60-75).  enable != 0 clears the list and starts recording.  _read copies up to
 * cap_events events (4 longs each) and returns the number recorded. */
DLAF_EXTERN_C int dlaf_mi355x_grid_comm_log(int context, int enable) DLAF_NOEXCEPT;
DLAF_EXTERN_C long dlaf_mi355x_grid_comm_log_read(int context, long* out_4_longs_per_event,
                                                  long cap_events) DLAF_NOEXCEPT;

/* my coordinates in a grid; returns 0, or -1 for an unknown context */
DLAF_EXTERN_C int dlaf_mi355x_grid_info(int context, int* nprow, int* npcol, int* myrow, int* mycol) DLAF_NOEXCEPT;

/* ---- device-resident matrices -------------------------------------------------------------- */
typedef struct dlaf_mi355x_matrix_s* dlaf_mi355x_matrix_t;

/* desc.ld is ignored here (the device copy is in tile layout) */
DLAF_EXTERN_C int dlaf_mi355x_matrix_create(int context, char type, char uplo, struct DLAF_descriptor desc,
                                            dlaf_mi355x_matrix_t* out) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_matrix_destroy(dlaf_mi355x_matrix_t m) DLAF_NOEXCEPT;
/* host_local: this process's local column-major array with leading dimension ld */
DLAF_EXTERN_C int dlaf_mi355x_matrix_upload(dlaf_mi355x_matrix_t m, const void* host_local, int ld) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_matrix_download(dlaf_mi355x_matrix_t m, void* host_local, int ld) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_matrix_copy(dlaf_mi355x_matrix_t dst, dlaf_mi355x_matrix_t src) DLAF_NOEXCEPT;
/* one global tile (gi, gj) of the device copy into a dense host array (column-major, ld >= tile rows), as the
 * caller's matrix stores it.  Returns 0, 1 when this process does not own the tile, < 0 on a bad handle.
 * Lets a checker sample an N = 65536 factor without moving 32 GiB. */
DLAF_EXTERN_C int dlaf_mi355x_matrix_fetch_tile(dlaf_mi355x_matrix_t m, long gi, long gj, void* host,
                                                int ld) DLAF_NOEXCEPT;
/* enqueue the factorization / wait for it (returns info) / both */
DLAF_EXTERN_C int dlaf_mi355x_cholesky_start(dlaf_mi355x_matrix_t m) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_cholesky_wait(dlaf_mi355x_matrix_t m) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_cholesky_factorization_device(dlaf_mi355x_matrix_t m) DLAF_NOEXCEPT;
/* This process's OWN device status word of the last wait / factorization, before the grid agreed on one value
 * (the reference aborts every rank, src/cusolver/assert_info.cu:35-45; here the smallest positive LAPACK index over
 * the grid is returned everywhere).  A test uses it to assert that the owner of a non-SPD diagonal tile flagged it. */
DLAF_EXTERN_C int dlaf_mi355x_matrix_local_info(dlaf_mi355x_matrix_t m) DLAF_NOEXCEPT;
/* Trailing-update launches of this process so far that ran in persistent form (work items pulled from queues, workgroup
 * slots left to the kernels beside them) and, of those, the ones that vacated exclusive compute units -- lets a test
 * assert that a reservation took the path it was meant to take. */
DLAF_EXTERN_C int dlaf_mi355x_update_launch_stats(long* persistent, long* exclusive) DLAF_NOEXCEPT;
/* Diagnosis hook (DLAF_MI355X_POTRF_TRACE=1): what the first two strips of the last first-diagonal-tile POTRF of
 * this process saw (32 words, kernels_potrf_coop.hip); returns 0, or 1 when tracing is off. */
DLAF_EXTERN_C int dlaf_mi355x_potrf_trace(unsigned long long* out_32_words) DLAF_NOEXCEPT;
/* Residual checker of the miniapp (miniapp/miniapp_cholesky.cpp:408-443 check_cholesky with
 * auxiliary/norm max_norm) on the device: `original` holds the input matrix and is OVERWRITTEN with
 * A - L L^H (uplo triangle); *max_diff = max|A - L L^H|, *max_a = max|A| over the whole grid (MAX-reduced
 * through the grid's transport).  The strict upper part of the factor's diagonal tiles is zeroed on the
 * device (it is never written back to the caller).  Collective. */
DLAF_EXTERN_C int dlaf_mi355x_cholesky_residual(dlaf_mi355x_matrix_t original, dlaf_mi355x_matrix_t factor,
                                                double* max_diff, double* max_a) DLAF_NOEXCEPT;
/* Live timing of the last factorization, measured with HIP events on the stream each launch class
 * runs on.  kind 0: grouped trailing update (herk+gemm of columns > k+1), 1: lookahead-column update,
 * 2: panel TRSM, 3: diagonal-tile POTRF chain.  ms = summed launch durations, flops / bytes = summed
 * ALGORITHMIC work of those launches (BASELINE.md roofline table).  Call after *_wait. */
DLAF_EXTERN_C int dlaf_mi355x_matrix_profile(dlaf_mi355x_matrix_t m, int kind, double* ms, long* launches,
                                             double* flops, double* bytes) DLAF_NOEXCEPT;
/* The panel TRSM of step 0 ALONE on the device: `reps` launches on a copy of the factored first tile column with
 * the factored diagonal tile, timed with HIP events (in the factorization the panel solves run beside the bulk
 * update on a few free workgroup slots; their in-situ durations do not describe the kernel).  One-process grids,
 * after a factorization.  *ms = average per launch, *flops / *bytes = algorithmic work of one launch. */
DLAF_EXTERN_C int dlaf_mi355x_matrix_trsm_profile(dlaf_mi355x_matrix_t m, int reps, double* ms, double* flops,
                                                  double* bytes) DLAF_NOEXCEPT;
/* barrier over the matrix's grid (RCCL all-reduce / host callback) */
DLAF_EXTERN_C int dlaf_mi355x_grid_barrier(int context) DLAF_NOEXCEPT;
/* Collective communication self-test of a grid (what test/unit/communication/test_broadcast*.cpp do for
 * the reference's MPI layer): every member of every row / column communicator broadcasts `bytes` of a
 * coordinate-dependent pattern in place, out of place and grouped, then barrier + max-allreduce.
 * Returns the number of failed checks on this process (0 = good), -1 for an unknown context.
 * DLAF_MI355X_RCCL_SINGLE=1 makes create_grid_rccl build communicators for a 1-process grid too. */
DLAF_EXTERN_C int dlaf_mi355x_grid_selftest(int context, size_t bytes) DLAF_NOEXCEPT;

/* ---- triangular solver ------------------------------------------------------- */
/* dlaf::triangular_solver(grid, side, uplo, op, diag, alpha, A, B), include/dlaf/solver/triangular.h:41-177
 * (the reference has no C entry for it; the p?trsm names take ScaLAPACK's argument list):
 *   side 'L': op(A) X = alpha B,  side 'R': X op(A) = alpha B;  B (m x n) is overwritten by X.
 * A: na x na triangular (na = m for 'L', n for 'R'), only the uplo triangle is read (diag 'U': its diagonal
 * is taken as 1), op in N/T/C, alpha passed by address.  a, b: local column-major parts on the grid of
 * `context`.  Requirements of this build: square blocks, B's block = A's block, no sub-matrix offsets, A and
 * B share the source process along the triangular dimension.  Returns 0; bad arguments terminate like the
 * reference's DLAF_ASSERTs. */
DLAF_EXTERN_C int dlaf_mi355x_triangular_solver_s(int context, char side, char uplo, char op, char diag,
                                                  const float* alpha, const float* a, struct DLAF_descriptor desca,
                                                  float* b, struct DLAF_descriptor descb) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_triangular_solver_d(int context, char side, char uplo, char op, char diag,
                                                  const double* alpha, const double* a, struct DLAF_descriptor desca,
                                                  double* b, struct DLAF_descriptor descb) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_triangular_solver_c(int context, char side, char uplo, char op, char diag,
                                                  const dlaf_complex_c* alpha, const dlaf_complex_c* a,
                                                  struct DLAF_descriptor desca, dlaf_complex_c* b,
                                                  struct DLAF_descriptor descb) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_triangular_solver_z(int context, char side, char uplo, char op, char diag,
                                                  const dlaf_complex_z* alpha, const dlaf_complex_z* a,
                                                  struct DLAF_descriptor desca, dlaf_complex_z* b,
                                                  struct DLAF_descriptor descb) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pstrsm(char side, char uplo, char op, char diag, int m, int n, const float* alpha,
                                      const float* a, int ia, int ja, const int desca[9], float* b, int ib, int jb,
                                      const int descb[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pdtrsm(char side, char uplo, char op, char diag, int m, int n, const double* alpha,
                                      const double* a, int ia, int ja, const int desca[9], double* b, int ib, int jb,
                                      const int descb[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pctrsm(char side, char uplo, char op, char diag, int m, int n,
                                      const dlaf_complex_c* alpha, const dlaf_complex_c* a, int ia, int ja,
                                      const int desca[9], dlaf_complex_c* b, int ib, int jb,
                                      const int descb[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pztrsm(char side, char uplo, char op, char diag, int m, int n,
                                      const dlaf_complex_z* alpha, const dlaf_complex_z* a, int ia, int ja,
                                      const int desca[9], dlaf_complex_z* b, int ib, int jb,
                                      const int descb[9]) DLAF_NOEXCEPT;

/* ---- triangular multiplication ------------------------------------------------------------- */
/* dlaf::triangular_multiplication(grid, side, uplo, op, diag, alpha, A, B), include/dlaf/multiplication/triangular.h
 * (the reference has no C entry for it; the p?trmm names take ScaLAPACK's argument list):
 *   side 'L': B = alpha op(A) B,  side 'R': B = alpha B op(A);  B (m x n) is overwritten.
 * A: na x na triangular (na = m for 'L', n for 'R'), only the uplo triangle is read (diag 'U': its diagonal
 * is taken as 1), op in N/T/C (every op on every grid), alpha passed by address.  a, b: local column-major parts on
 * the grid of `context`.  Requirements of this build, as for the solver: square blocks of A, B's block along the
 * triangular dimension = A's, no sub-matrix offsets, A and B share the source process along the triangular
 * dimension.  Returns 0; bad arguments terminate like the reference's DLAF_ASSERTs, before the GPU is touched. */
DLAF_EXTERN_C int dlaf_mi355x_triangular_multiplication_s(int context, char side, char uplo, char op, char diag,
                                                          const float* alpha, const float* a,
                                                          struct DLAF_descriptor desca, float* b,
                                                          struct DLAF_descriptor descb) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_triangular_multiplication_d(int context, char side, char uplo, char op, char diag,
                                                          const double* alpha, const double* a,
                                                          struct DLAF_descriptor desca, double* b,
                                                          struct DLAF_descriptor descb) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_triangular_multiplication_c(int context, char side, char uplo, char op, char diag,
                                                          const dlaf_complex_c* alpha, const dlaf_complex_c* a,
                                                          struct DLAF_descriptor desca, dlaf_complex_c* b,
                                                          struct DLAF_descriptor descb) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_triangular_multiplication_z(int context, char side, char uplo, char op, char diag,
                                                          const dlaf_complex_z* alpha, const dlaf_complex_z* a,
                                                          struct DLAF_descriptor desca, dlaf_complex_z* b,
                                                          struct DLAF_descriptor descb) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pstrmm(char side, char uplo, char op, char diag, int m, int n, const float* alpha,
                                      const float* a, int ia, int ja, const int desca[9], float* b, int ib, int jb,
                                      const int descb[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pdtrmm(char side, char uplo, char op, char diag, int m, int n, const double* alpha,
                                      const double* a, int ia, int ja, const int desca[9], double* b, int ib, int jb,
                                      const int descb[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pctrmm(char side, char uplo, char op, char diag, int m, int n,
                                      const dlaf_complex_c* alpha, const dlaf_complex_c* a, int ia, int ja,
                                      const int desca[9], dlaf_complex_c* b, int ib, int jb,
                                      const int descb[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pztrmm(char side, char uplo, char op, char diag, int m, int n,
                                      const dlaf_complex_z* alpha, const dlaf_complex_z* a, int ia, int ja,
                                      const int desca[9], dlaf_complex_z* b, int ib, int jb,
                                      const int descb[9]) DLAF_NOEXCEPT;

/* ---- Hermitian multiplication -------------------------------------------------------------- */
/* dlaf::hermitian_multiplication(grid, side, uplo, alpha, A, B, beta, C), include/dlaf/multiplication/hermitian.h
 * (the reference has no C entry for it; the p?symm / p?hemm names take ScaLAPACK's argument list):
 *   side 'L': C = beta C + alpha A B,  side 'R': C = beta C + alpha B A;  C (m x n) is overwritten, A and B are not.
 * A: na x na Hermitian (na = m for 'L', n for 'R'); only its uplo triangle is read and, for complex types, the
 * imaginary part of its diagonal is ignored (xHEMM).  Every side x uplo, on every grid (the reference implements
 * side L / uplo L only).  beta = 0: C is not read.  alpha, beta passed by address; a, b, c: local column-major parts
 * on the grid of `context`; only the m x n elements of c are written.  Requirements of this build, as for the solver:
 * square blocks of A; B and C with the same blocks and source process, their block along A's dimension = A's (the
 * other one is free); no sub-matrix offsets; A shares the source process of B and C along A's dimension.  Returns 0;
 * a violated requirement terminates with a message "hermitian multiplication: ..." before the GPU is touched. */
DLAF_EXTERN_C int dlaf_mi355x_hermitian_multiplication_s(int context, char side, char uplo, const float* alpha,
                                                         const float* a, struct DLAF_descriptor desca, const float* b,
                                                         struct DLAF_descriptor descb, const float* beta, float* c,
                                                         struct DLAF_descriptor descc) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_hermitian_multiplication_d(int context, char side, char uplo, const double* alpha,
                                                         const double* a, struct DLAF_descriptor desca, const double* b,
                                                         struct DLAF_descriptor descb, const double* beta, double* c,
                                                         struct DLAF_descriptor descc) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_hermitian_multiplication_c(int context, char side, char uplo, const dlaf_complex_c* alpha,
                                                         const dlaf_complex_c* a, struct DLAF_descriptor desca,
                                                         const dlaf_complex_c* b, struct DLAF_descriptor descb,
                                                         const dlaf_complex_c* beta, dlaf_complex_c* c,
                                                         struct DLAF_descriptor descc) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_hermitian_multiplication_z(int context, char side, char uplo, const dlaf_complex_z* alpha,
                                                         const dlaf_complex_z* a, struct DLAF_descriptor desca,
                                                         const dlaf_complex_z* b, struct DLAF_descriptor descb,
                                                         const dlaf_complex_z* beta, dlaf_complex_z* c,
                                                         struct DLAF_descriptor descc) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pssymm(char side, char uplo, int m, int n, const float* alpha, const float* a, int ia,
                                      int ja, const int desca[9], const float* b, int ib, int jb, const int descb[9],
                                      const float* beta, float* c, int ic, int jc, const int descc[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pdsymm(char side, char uplo, int m, int n, const double* alpha, const double* a, int ia,
                                      int ja, const int desca[9], const double* b, int ib, int jb, const int descb[9],
                                      const double* beta, double* c, int ic, int jc, const int descc[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pchemm(char side, char uplo, int m, int n, const dlaf_complex_c* alpha,
                                      const dlaf_complex_c* a, int ia, int ja, const int desca[9],
                                      const dlaf_complex_c* b, int ib, int jb, const int descb[9],
                                      const dlaf_complex_c* beta, dlaf_complex_c* c, int ic, int jc,
                                      const int descc[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pzhemm(char side, char uplo, int m, int n, const dlaf_complex_z* alpha,
                                      const dlaf_complex_z* a, int ia, int ja, const int desca[9],
                                      const dlaf_complex_z* b, int ib, int jb, const int descb[9],
                                      const dlaf_complex_z* beta, dlaf_complex_z* c, int ic, int jc,
                                      const int descc[9]) DLAF_NOEXCEPT;

/* ---- General multiplication ---------------------------------------------------------------- */
/* dlaf::multiplication::internal::generalMatrix(opA, opB, alpha, A, B, beta, C), include/dlaf/multiplication/general.h
 * (the reference has no C entry for it; the p?gemm names take ScaLAPACK's argument list):
 *   C = beta C + alpha op(A) op(B),  op(X) = X ('N'), X^T ('T') or X^H ('C');  C (m x n) is overwritten, A and B are not.
 * a, b, c and their descriptors describe the matrices AS STORED: A is m x k ('N') or k x m, B is k x n ('N') or n x k.
 * One process: every op pair.  A grid of more than one process: 'N' 'N' only (the reference's distributed coverage).
 * beta = 0: C is not read.  k = 0 or alpha = 0: C = beta C and A, B are not referenced.  m = 0 or n = 0: returns at
 * once.  alpha, beta passed by address; a, b, c: local column-major parts on the grid of `context`; only the m x n
 * elements of c are written.  Requirements of this build: one square block for A, B and C; no sub-matrix offsets; A
 * starts on C's process row (desca.isrc = descc.isrc) and B on C's process column (descb.jsrc = descc.jsrc).  Returns
 * 0; a violated requirement terminates with a message "general multiplication: ..." before the GPU is touched. */
DLAF_EXTERN_C int dlaf_mi355x_general_multiplication_s(int context, char opa, char opb, const float* alpha,
                                                       const float* a, struct DLAF_descriptor desca, const float* b,
                                                       struct DLAF_descriptor descb, const float* beta, float* c,
                                                       struct DLAF_descriptor descc) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_general_multiplication_d(int context, char opa, char opb, const double* alpha,
                                                       const double* a, struct DLAF_descriptor desca, const double* b,
                                                       struct DLAF_descriptor descb, const double* beta, double* c,
                                                       struct DLAF_descriptor descc) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_general_multiplication_c(int context, char opa, char opb, const dlaf_complex_c* alpha,
                                                       const dlaf_complex_c* a, struct DLAF_descriptor desca, const dlaf_complex_c* b,
                                                       struct DLAF_descriptor descb, const dlaf_complex_c* beta, dlaf_complex_c* c,
                                                       struct DLAF_descriptor descc) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_general_multiplication_z(int context, char opa, char opb, const dlaf_complex_z* alpha,
                                                       const dlaf_complex_z* a, struct DLAF_descriptor desca, const dlaf_complex_z* b,
                                                       struct DLAF_descriptor descb, const dlaf_complex_z* beta, dlaf_complex_z* c,
                                                       struct DLAF_descriptor descc) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_psgemm(char transa, char transb, int m, int n, int k, const float* alpha,
                                      const float* a, int ia, int ja, const int desca[9], const float* b, int ib, int jb,
                                      const int descb[9], const float* beta, float* c, int ic, int jc,
                                      const int descc[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pdgemm(char transa, char transb, int m, int n, int k, const double* alpha,
                                      const double* a, int ia, int ja, const int desca[9], const double* b, int ib, int jb,
                                      const int descb[9], const double* beta, double* c, int ic, int jc,
                                      const int descc[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pcgemm(char transa, char transb, int m, int n, int k, const dlaf_complex_c* alpha,
                                      const dlaf_complex_c* a, int ia, int ja, const int desca[9], const dlaf_complex_c* b, int ib, int jb,
                                      const int descb[9], const dlaf_complex_c* beta, dlaf_complex_c* c, int ic, int jc,
                                      const int descc[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pzgemm(char transa, char transb, int m, int n, int k, const dlaf_complex_z* alpha,
                                      const dlaf_complex_z* a, int ia, int ja, const int desca[9], const dlaf_complex_z* b, int ib, int jb,
                                      const int descb[9], const dlaf_complex_z* beta, dlaf_complex_z* c, int ic, int jc,
                                      const int descc[9]) DLAF_NOEXCEPT;

/* ---- Hermitian rank-k and rank-2k updates ---------------------------------------------------- */
/* BLAS xSYRK / xHERK and xSYR2K / xHER2K on the grid (the reference runs them tile by tile inside its Cholesky and
 * generalized-to-standard algorithms and has no entry for them; the p? names take ScaLAPACK's argument lists).  uplo
 * 'L' or 'U': only that triangle of the n x n matrix C is read or written.
 *   rank-k  (s, d: syrk;  c, z: herk)    alpha and beta are REAL
 *     trans 'N':  C = alpha A A^H + beta C,  A stored n x k        trans 'C':  C = alpha A^H A + beta C,  A stored k x n
 *   rank-2k (s, d: syr2k; c, z: her2k)   alpha is of the element type, beta is REAL; B is stored like A
 *     trans 'N':  C = alpha A B^H + conj(alpha) B A^H + beta C     trans 'C':  C = alpha A^H B + conj(alpha) B^H A + beta C
 * Real types also accept trans 'T', which equals 'C'.  Complex types refuse 'T': that is the complex-symmetric
 * p{c,z}syrk / p{c,z}syr2k, which is not built.
 * Semantics (BLAS):
 *   - the other triangle of C is never referenced: it stays bit for bit, and NaNs in it reach nothing;
 *   - complex types: the imaginary part of C's diagonal is ignored on entry and is exactly 0 on exit, also when only
 *     beta is applied;
 *   - beta = 0: C is not read (NaNs in its triangle do not survive);
 *   - alpha = 0 or k = 0: A (and B) are not referenced and the triangle becomes beta C;
 *   - if, in addition, beta = 1: quick return, C is untouched bit for bit, diagonal imaginary parts included;
 *   - n = 0 returns before the GPU is touched.
 * One process: both trans.  A grid of more than one process: trans 'N' only.  Requirements of this build: one square
 * block for A, B and C; no sub-matrix offsets; B has A's shape, blocks and source process; with trans 'N', A starts on
 * C's process row (desca.isrc = descc.isrc).  Returns 0; a violated requirement terminates with a message "hermitian
 * rank-k update: ..." / "hermitian rank-2k update: ..." before the GPU is touched. */
DLAF_EXTERN_C int dlaf_mi355x_hermitian_rank_k_update_s(int context, char uplo, char trans, const float* alpha,
                                                        const float* a, struct DLAF_descriptor desca, const float* beta,
                                                        float* c, struct DLAF_descriptor descc) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_hermitian_rank_k_update_d(int context, char uplo, char trans, const double* alpha,
                                                        const double* a, struct DLAF_descriptor desca, const double* beta,
                                                        double* c, struct DLAF_descriptor descc) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_hermitian_rank_k_update_c(int context, char uplo, char trans, const float* alpha,
                                                        const dlaf_complex_c* a, struct DLAF_descriptor desca, const float* beta,
                                                        dlaf_complex_c* c, struct DLAF_descriptor descc) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_hermitian_rank_k_update_z(int context, char uplo, char trans, const double* alpha,
                                                        const dlaf_complex_z* a, struct DLAF_descriptor desca, const double* beta,
                                                        dlaf_complex_z* c, struct DLAF_descriptor descc) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_hermitian_rank_2k_update_s(int context, char uplo, char trans, const float* alpha,
                                                         const float* a, struct DLAF_descriptor desca, const float* b,
                                                         struct DLAF_descriptor descb, const float* beta, float* c,
                                                         struct DLAF_descriptor descc) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_hermitian_rank_2k_update_d(int context, char uplo, char trans, const double* alpha,
                                                         const double* a, struct DLAF_descriptor desca, const double* b,
                                                         struct DLAF_descriptor descb, const double* beta, double* c,
                                                         struct DLAF_descriptor descc) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_hermitian_rank_2k_update_c(int context, char uplo, char trans, const dlaf_complex_c* alpha,
                                                         const dlaf_complex_c* a, struct DLAF_descriptor desca, const dlaf_complex_c* b,
                                                         struct DLAF_descriptor descb, const float* beta, dlaf_complex_c* c,
                                                         struct DLAF_descriptor descc) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_hermitian_rank_2k_update_z(int context, char uplo, char trans, const dlaf_complex_z* alpha,
                                                         const dlaf_complex_z* a, struct DLAF_descriptor desca, const dlaf_complex_z* b,
                                                         struct DLAF_descriptor descb, const double* beta, dlaf_complex_z* c,
                                                         struct DLAF_descriptor descc) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pssyrk(char uplo, char trans, int n, int k, const float* alpha, const float* a, int ia,
                                      int ja, const int desca[9], const float* beta, float* c, int ic, int jc,
                                      const int descc[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pdsyrk(char uplo, char trans, int n, int k, const double* alpha, const double* a, int ia,
                                      int ja, const int desca[9], const double* beta, double* c, int ic, int jc,
                                      const int descc[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pcherk(char uplo, char trans, int n, int k, const float* alpha, const dlaf_complex_c* a, int ia,
                                      int ja, const int desca[9], const float* beta, dlaf_complex_c* c, int ic, int jc,
                                      const int descc[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pzherk(char uplo, char trans, int n, int k, const double* alpha, const dlaf_complex_z* a, int ia,
                                      int ja, const int desca[9], const double* beta, dlaf_complex_z* c, int ic, int jc,
                                      const int descc[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pssyr2k(char uplo, char trans, int n, int k, const float* alpha, const float* a,
                                       int ia, int ja, const int desca[9], const float* b, int ib, int jb,
                                       const int descb[9], const float* beta, float* c, int ic, int jc,
                                       const int descc[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pdsyr2k(char uplo, char trans, int n, int k, const double* alpha, const double* a,
                                       int ia, int ja, const int desca[9], const double* b, int ib, int jb,
                                       const int descb[9], const double* beta, double* c, int ic, int jc,
                                       const int descc[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pcher2k(char uplo, char trans, int n, int k, const dlaf_complex_c* alpha, const dlaf_complex_c* a,
                                       int ia, int ja, const int desca[9], const dlaf_complex_c* b, int ib, int jb,
                                       const int descb[9], const float* beta, dlaf_complex_c* c, int ic, int jc,
                                       const int descc[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pzher2k(char uplo, char trans, int n, int k, const dlaf_complex_z* alpha, const dlaf_complex_z* a,
                                       int ia, int ja, const int desca[9], const dlaf_complex_z* b, int ib, int jb,
                                       const int descb[9], const double* beta, dlaf_complex_z* c, int ic, int jc,
                                       const int descc[9]) DLAF_NOEXCEPT;

/* ---- weighted Hermitian rank-k update and functions of a Hermitian matrix -------------------- */
/* "xSYRK / xHERK with weights": the uplo triangle of
 *     trans 'N':  C = alpha A D A^H + beta C,  A stored n x k        trans 'C':  C = alpha A^H D A + beta C,  A stored k x n
 * with D = diag(d) a REAL diagonal of any sign (also the normal-equations product A D A^T); alpha and beta are REAL.  d:
 * k reals in HOST memory, the SAME on every rank of the grid (the caller's duty, as for alpha); they are uploaded once
 * (k reals) and multiplied into one operand inside the rank-k kernel, between its global load and its LDS image: no
 * scaled copy of A is made and the flops are those of a rank-k update, k n (n + 1).  PBLAS has no such routine, hence no
 * p? names.  Real types also accept trans 'T'; complex types refuse it.
 * Semantics are those of the rank-k update above: the other triangle of C is never referenced; the imaginary part of C's
 * diagonal is ignored on entry and exactly 0 on exit; beta = 0: C is not read; alpha = 0 or k = 0: A AND d are not
 * referenced (d may be null then) and the triangle becomes beta C; with beta = 1 on top of that nothing is touched;
 * n = 0 returns before the GPU is touched.  A ZERO weight does NOT unreference its column: 0 * NaN is NaN, as in
 * A diag(d) A^H computed by hand.  Non-finite weights are not judged.
 * One process: both trans.  More than one process: trans 'N' only, A on C's process row.  Requirements of the rank-k
 * update, plus: d non-null while k > 0 and alpha != 0.  A violated one terminates with "hermitian weighted rank-k
 * update: ..." before the GPU is touched. */
DLAF_EXTERN_C int dlaf_mi355x_hermitian_weighted_rank_k_update_s(int context, char uplo, char trans, const float* alpha,
                                                                 const float* a, struct DLAF_descriptor desca,
                                                                 const float* d, const float* beta, float* c,
                                                                 struct DLAF_descriptor descc) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_hermitian_weighted_rank_k_update_d(int context, char uplo, char trans, const double* alpha,
                                                                 const double* a, struct DLAF_descriptor desca,
                                                                 const double* d, const double* beta, double* c,
                                                                 struct DLAF_descriptor descc) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_hermitian_weighted_rank_k_update_c(int context, char uplo, char trans, const float* alpha,
                                                                 const dlaf_complex_c* a, struct DLAF_descriptor desca,
                                                                 const float* d, const float* beta, dlaf_complex_c* c,
                                                                 struct DLAF_descriptor descc) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_hermitian_weighted_rank_k_update_z(int context, char uplo, char trans, const double* alpha,
                                                                 const dlaf_complex_z* a, struct DLAF_descriptor desca,
                                                                 const double* d, const double* beta, dlaf_complex_z* c,
                                                                 struct DLAF_descriptor descc) DLAF_NOEXCEPT;
/* Functions of a Hermitian matrix: the uplo triangle of the n x n matrix A becomes that of
 *     f(A) = sum over the selected j of  g_j z_j z_j^H,    (w, Z) the eigenpairs of A,  g = weights(w)
 * (a density matrix, a spectral projector, S^(-1/2), a square root, an inverse or pseudo-inverse, an exponential): the
 * eigensolver on A, ONE call of `weights` on the host, and the weighted rank-k update above (trans 'N', beta 0) with the
 * eigenvectors still in HBM: Z is never downloaded, only the triangle is.
 *   uplo            'L' (what the eigensolver takes).
 *   w               n reals: all eigenvalues, ascending, as the eigensolver gives them, on every rank.
 *   weights         called once per rank with (n, w, begin, end, g, user): it writes g[j] for begin <= j < end and nothing
 *                   else (g has n entries).  Every rank must compute the same weights.
 *   index_range     null, or {begin, end}: the 0-based half-open range of eigenvalue indices that take part.
 *   value_interval  null, or {vl, vu}: the eigenvalues in (vl, vu] take part (infinite ends allowed).
 *                   Both null: all n.  Both given: refused.  Eigenvalues that are not selected have weight 0 by
 *                   definition, and their eigenvectors are never computed.  An empty selection gives a zero triangle.
 *   selected        null, or two longs that receive the selected [begin, end).
 * Returns the eigensolver's status, agreed over the grid; when it is not 0 the caller's a is unchanged.  The other
 * triangle of a is never touched; the diagonal of a complex result is exactly real.  A violated requirement terminates
 * with "hermitian function: ..." before the GPU is touched.
 * hermitian_power: f = x^exponent on the eigenvalues above `threshold` (>= 0, else refused), the others DROPPED (weight
 * 0: the pseudo-inverse for exponent -1, Loewdin's S^(-1/2) for -1/2).  It is the value interval (threshold, +inf): the
 * dropped eigenvectors are not computed and *n_dropped (null allowed) is the Sturm count of `threshold`. */
typedef void (*dlaf_mi355x_spectral_weights_s)(long n, const float* w, long begin, long end, float* g, void* user);
typedef void (*dlaf_mi355x_spectral_weights_d)(long n, const double* w, long begin, long end, double* g, void* user);
DLAF_EXTERN_C int dlaf_mi355x_hermitian_function_s(int context, char uplo, float* a, struct DLAF_descriptor desca, float* w,
                                                   dlaf_mi355x_spectral_weights_s weights, void* user,
                                                   const long* index_range, const float* value_interval,
                                                   long* selected) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_hermitian_function_d(int context, char uplo, double* a, struct DLAF_descriptor desca, double* w,
                                                   dlaf_mi355x_spectral_weights_d weights, void* user,
                                                   const long* index_range, const double* value_interval,
                                                   long* selected) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_hermitian_function_c(int context, char uplo, dlaf_complex_c* a, struct DLAF_descriptor desca,
                                                   float* w, dlaf_mi355x_spectral_weights_s weights, void* user,
                                                   const long* index_range, const float* value_interval,
                                                   long* selected) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_hermitian_function_z(int context, char uplo, dlaf_complex_z* a, struct DLAF_descriptor desca,
                                                   double* w, dlaf_mi355x_spectral_weights_d weights, void* user,
                                                   const long* index_range, const double* value_interval,
                                                   long* selected) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_hermitian_power_s(int context, char uplo, float* a, struct DLAF_descriptor desca, float* w,
                                                double exponent, double threshold, long* n_dropped) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_hermitian_power_d(int context, char uplo, double* a, struct DLAF_descriptor desca, double* w,
                                                double exponent, double threshold, long* n_dropped) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_hermitian_power_c(int context, char uplo, dlaf_complex_c* a, struct DLAF_descriptor desca,
                                                float* w, double exponent, double threshold,
                                                long* n_dropped) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_hermitian_power_z(int context, char uplo, dlaf_complex_z* a, struct DLAF_descriptor desca,
                                                double* w, double exponent, double threshold,
                                                long* n_dropped) DLAF_NOEXCEPT;

/* general_addition: C = beta C + alpha op(A) on the uplo part of the m x n matrix C -- PBLAS p?geadd (uplo 'A') and
 * p?tradd, the transpositions p?tran / p?tranu / p?tranc (op 'T' / 'C'), ScaLAPACK p?lacpy (alpha 1, beta 0, op 'N').
 *   uplo 'A': every element, 'L': i >= j, 'U': i <= j (for m != n the trapezoids of xLACPY)
 *   op 'N': A stored m x n;  'T' / 'C': A stored n x m (real types: 'C' equals 'T')
 * hermitian_complete: the OTHER triangle of the n x n matrix A from its uplo one, in place; kind 'H': the mirror is
 * conjugated and the imaginary part of the diagonal becomes exactly 0 (the convention of hermitian_rank_k_update), kind
 * 'S': plain transpose, the diagonal untouched bit for bit.
 * Semantics:
 *   - outside the uplo part C stays bit for bit, and so do the padding rows of its leading dimension; A is only read;
 *   - beta = 0: C is not read (NaNs in its part do not survive);
 *   - alpha = 0: A is not referenced (NaNs in it reach nothing), and the part becomes beta C;
 *   - if, in addition, beta = 1: quick return, nothing is touched;
 *   - alpha = 1, beta = 0, op 'N' or 'T': the result is a BIT COPY of the source elements (signed zeros, denormals and
 *     NaN payloads are moved, never multiplied): p?lacpy and a plain transpose are exact;
 *   - m = 0 or n = 0 returns before the GPU is touched.
 * Any grid, every op.  Requirements of this build: one square block for A and C; no sub-matrix offsets; op 'N' needs A
 * on C's source process; A and C being the same array is accepted for op 'N' only; hermitian_complete needs a square
 * matrix.  Returns 0; a violated requirement terminates with a message "general addition: ..." / "hermitian complete:
 * ..." before the GPU is touched. */
DLAF_EXTERN_C int dlaf_mi355x_general_addition_s(int context, char uplo, char op, const float* alpha, const float* a,
                                                  struct DLAF_descriptor desca, const float* beta, float* c,
                                                  struct DLAF_descriptor descc) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_general_addition_d(int context, char uplo, char op, const double* alpha, const double* a,
                                                  struct DLAF_descriptor desca, const double* beta, double* c,
                                                  struct DLAF_descriptor descc) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_general_addition_c(int context, char uplo, char op, const dlaf_complex_c* alpha, const dlaf_complex_c* a,
                                                  struct DLAF_descriptor desca, const dlaf_complex_c* beta, dlaf_complex_c* c,
                                                  struct DLAF_descriptor descc) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_general_addition_z(int context, char uplo, char op, const dlaf_complex_z* alpha, const dlaf_complex_z* a,
                                                  struct DLAF_descriptor desca, const dlaf_complex_z* beta, dlaf_complex_z* c,
                                                  struct DLAF_descriptor descc) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_hermitian_complete_s(int context, char uplo, char kind, float* a,
                                                    struct DLAF_descriptor desca) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_hermitian_complete_d(int context, char uplo, char kind, double* a,
                                                    struct DLAF_descriptor desca) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_hermitian_complete_c(int context, char uplo, char kind, dlaf_complex_c* a,
                                                    struct DLAF_descriptor desca) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_hermitian_complete_z(int context, char uplo, char kind, dlaf_complex_z* a,
                                                    struct DLAF_descriptor desca) DLAF_NOEXCEPT;
/* the ScaLAPACK / PBLAS argument lists (ia = ja = ic = jc = 1); p?lacpy: as in LAPACK, any uplo letter other than 'U' /
 * 'L' means all; p?tran* : C (m x n) = beta C + alpha A^T (tran, tranu) / alpha A^H (tranc), A n x m */
DLAF_EXTERN_C void dlaf_mi355x_psgeadd(char trans, int m, int n, const float* alpha, const float* a, int ia, int ja,
                                       const int desca[9], const float* beta, float* c, int ic, int jc,
                                       const int descc[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pstradd(char uplo, char trans, int m, int n, const float* alpha, const float* a, int ia,
                                       int ja, const int desca[9], const float* beta, float* c, int ic, int jc,
                                       const int descc[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pslacpy(char uplo, int m, int n, const float* a, int ia, int ja, const int desca[9],
                                       float* b, int ib, int jb, const int descb[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pdgeadd(char trans, int m, int n, const double* alpha, const double* a, int ia, int ja,
                                       const int desca[9], const double* beta, double* c, int ic, int jc,
                                       const int descc[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pdtradd(char uplo, char trans, int m, int n, const double* alpha, const double* a, int ia,
                                       int ja, const int desca[9], const double* beta, double* c, int ic, int jc,
                                       const int descc[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pdlacpy(char uplo, int m, int n, const double* a, int ia, int ja, const int desca[9],
                                       double* b, int ib, int jb, const int descb[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pcgeadd(char trans, int m, int n, const dlaf_complex_c* alpha, const dlaf_complex_c* a, int ia, int ja,
                                       const int desca[9], const dlaf_complex_c* beta, dlaf_complex_c* c, int ic, int jc,
                                       const int descc[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pctradd(char uplo, char trans, int m, int n, const dlaf_complex_c* alpha, const dlaf_complex_c* a, int ia,
                                       int ja, const int desca[9], const dlaf_complex_c* beta, dlaf_complex_c* c, int ic, int jc,
                                       const int descc[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pclacpy(char uplo, int m, int n, const dlaf_complex_c* a, int ia, int ja, const int desca[9],
                                       dlaf_complex_c* b, int ib, int jb, const int descb[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pzgeadd(char trans, int m, int n, const dlaf_complex_z* alpha, const dlaf_complex_z* a, int ia, int ja,
                                       const int desca[9], const dlaf_complex_z* beta, dlaf_complex_z* c, int ic, int jc,
                                       const int descc[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pztradd(char uplo, char trans, int m, int n, const dlaf_complex_z* alpha, const dlaf_complex_z* a, int ia,
                                       int ja, const int desca[9], const dlaf_complex_z* beta, dlaf_complex_z* c, int ic, int jc,
                                       const int descc[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pzlacpy(char uplo, int m, int n, const dlaf_complex_z* a, int ia, int ja, const int desca[9],
                                       dlaf_complex_z* b, int ib, int jb, const int descb[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pstran(int m, int n, const float* alpha, const float* a, int ia, int ja,
                                      const int desca[9], const float* beta, float* c, int ic, int jc,
                                      const int descc[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pdtran(int m, int n, const double* alpha, const double* a, int ia, int ja,
                                      const int desca[9], const double* beta, double* c, int ic, int jc,
                                      const int descc[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pctranu(int m, int n, const dlaf_complex_c* alpha, const dlaf_complex_c* a, int ia, int ja,
                                      const int desca[9], const dlaf_complex_c* beta, dlaf_complex_c* c, int ic, int jc,
                                      const int descc[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pctranc(int m, int n, const dlaf_complex_c* alpha, const dlaf_complex_c* a, int ia, int ja,
                                      const int desca[9], const dlaf_complex_c* beta, dlaf_complex_c* c, int ic, int jc,
                                      const int descc[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pztranu(int m, int n, const dlaf_complex_z* alpha, const dlaf_complex_z* a, int ia, int ja,
                                      const int desca[9], const dlaf_complex_z* beta, dlaf_complex_z* c, int ic, int jc,
                                      const int descc[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pztranc(int m, int n, const dlaf_complex_z* alpha, const dlaf_complex_z* a, int ia, int ja,
                                      const int desca[9], const dlaf_complex_z* beta, dlaf_complex_z* c, int ic, int jc,
                                      const int descc[9]) DLAF_NOEXCEPT;

/* ScaLAPACK p?potrs: A X = B with the factor dlaf_p?potrf left in a (two triangular solves; b is overwritten) */
DLAF_EXTERN_C void dlaf_mi355x_pspotrs(char uplo, int n, int nrhs, const float* a, int ia, int ja, const int desca[9],
                                       float* b, int ib, int jb, const int descb[9], int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pdpotrs(char uplo, int n, int nrhs, const double* a, int ia, int ja, const int desca[9],
                                       double* b, int ib, int jb, const int descb[9], int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pcpotrs(char uplo, int n, int nrhs, const dlaf_complex_c* a, int ia, int ja,
                                       const int desca[9], dlaf_complex_c* b, int ib, int jb, const int descb[9],
                                       int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pzpotrs(char uplo, int n, int nrhs, const dlaf_complex_z* a, int ia, int ja,
                                       const int desca[9], dlaf_complex_z* b, int ib, int jb, const int descb[9],
                                       int* info) DLAF_NOEXCEPT;

/* ---- generalized -> standard eigenproblem ------------------------------------------- */
/* dlaf::eigensolver::internal::generalized_to_standard(grid, uplo, A, B), include/dlaf/eigensolver/gen_to_std.h:50,
 * :101 (LAPACK xHEGST itype 1; the reference has no C entry for it):  A <- inv(L) A inv(L^H) (uplo 'L') or
 * inv(U^H) A inv(U) (uplo 'U'), where b holds the Cholesky factor of B in its uplo triangle (dlaf_p?potrf output).
 * Only the uplo triangles are read / written; b is not modified.  A and B must be distributed alike (size, square
 * block, source process).  Returns 0.  The p?hegst names take ScaLAPACK's p?sygst / p?hegst argument list
 * (ibtype must be 1; *scale is set to 1). */
DLAF_EXTERN_C int dlaf_mi355x_generalized_to_standard_s(int context, char uplo, float* a, struct DLAF_descriptor desca,
                                                        const float* b, struct DLAF_descriptor descb) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_generalized_to_standard_d(int context, char uplo, double* a, struct DLAF_descriptor desca,
                                                        const double* b, struct DLAF_descriptor descb) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_generalized_to_standard_c(int context, char uplo, dlaf_complex_c* a,
                                                        struct DLAF_descriptor desca, const dlaf_complex_c* b,
                                                        struct DLAF_descriptor descb) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_generalized_to_standard_z(int context, char uplo, dlaf_complex_z* a,
                                                        struct DLAF_descriptor desca, const dlaf_complex_z* b,
                                                        struct DLAF_descriptor descb) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pshegst(int ibtype, char uplo, int n, float* a, int ia, int ja, const int desca[9],
                                       const float* b, int ib, int jb, const int descb[9], float* scale,
                                       int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pdhegst(int ibtype, char uplo, int n, double* a, int ia, int ja, const int desca[9],
                                       const double* b, int ib, int jb, const int descb[9], double* scale,
                                       int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pchegst(int ibtype, char uplo, int n, dlaf_complex_c* a, int ia, int ja,
                                       const int desca[9], const dlaf_complex_c* b, int ib, int jb,
                                       const int descb[9], float* scale, int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pzhegst(int ibtype, char uplo, int n, dlaf_complex_z* a, int ia, int ja,
                                       const int desca[9], const dlaf_complex_z* b, int ib, int jb,
                                       const int descb[9], double* scale, int* info) DLAF_NOEXCEPT;
/* the same on device-resident matrices (both created with the same uplo on the same grid) */
DLAF_EXTERN_C int dlaf_mi355x_generalized_to_standard_device(dlaf_mi355x_matrix_t a,
                                                             dlaf_mi355x_matrix_t cholesky_factor_of_b) DLAF_NOEXCEPT;

/* ---- reduction to band + back-transformation (first stage of the eigensolver) ----------- */
/* dlaf::eigensolver::internal::reduction_to_band<B, D, T>(grid, mat_a, band_size)
 * (include/dlaf/eigensolver/reduction_to_band.h:40-122; the reference has no C entry for the stage alone):
 * Q^H A Q = B with B Hermitian band (main diagonal + band_size sub-diagonals).  a: this process's local
 * column-major part of the Hermitian matrix; only its LOWER triangle is referenced and overwritten -- with the band
 * and, below it, the Householder reflectors (the layout of reduction_to_band.h:77-96); the strict upper triangle is
 * untouched.  band_size >= 2 must divide the (square) block size.  taus: n - band_size - 1 scalar factors, ALL of
 * them on every process (the reference returns them distributed over the process columns, replicated over the
 * rows; entry j belongs to the reflector in global column j).  Returns 0. */
DLAF_EXTERN_C int dlaf_mi355x_reduction_to_band_s(int context, float* a, struct DLAF_descriptor desca, int band_size,
                                                  float* taus) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_reduction_to_band_d(int context, double* a, struct DLAF_descriptor desca, int band_size,
                                                  double* taus) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_reduction_to_band_c(int context, dlaf_complex_c* a, struct DLAF_descriptor desca,
                                                  int band_size, dlaf_complex_c* taus) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_reduction_to_band_z(int context, dlaf_complex_z* a, struct DLAF_descriptor desca,
                                                  int band_size, dlaf_complex_z* taus) DLAF_NOEXCEPT;
/* the same on a device-resident matrix (created with uplo 'L'); taus: host array as above (may be NULL) */
DLAF_EXTERN_C int dlaf_mi355x_reduction_to_band_device(dlaf_mi355x_matrix_t a, int band_size, void* taus) DLAF_NOEXCEPT;
/* dlaf::eigensolver::internal::bt_reduction_to_band(grid, band_size, mat_c, mat_v, mat_taus)
 * (include/dlaf/eigensolver/bt_reduction_to_band.h): C <- Q C with the reflectors reduction_to_band left in v (lower
 * triangle, below the band) and its taus.  c: n x k general matrix with v's block size and row distribution. */
DLAF_EXTERN_C int dlaf_mi355x_bt_reduction_to_band_s(int context, int band_size, float* c, struct DLAF_descriptor descc,
                                                     const float* v, struct DLAF_descriptor descv,
                                                     const float* taus) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_bt_reduction_to_band_d(int context, int band_size, double* c, struct DLAF_descriptor descc,
                                                     const double* v, struct DLAF_descriptor descv,
                                                     const double* taus) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_bt_reduction_to_band_c(int context, int band_size, dlaf_complex_c* c,
                                                     struct DLAF_descriptor descc, const dlaf_complex_c* v,
                                                     struct DLAF_descriptor descv, const dlaf_complex_c* taus) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_bt_reduction_to_band_z(int context, int band_size, dlaf_complex_z* c,
                                                     struct DLAF_descriptor descc, const dlaf_complex_z* v,
                                                     struct DLAF_descriptor descv, const dlaf_complex_z* taus) DLAF_NOEXCEPT;
/* Panels of this process's last reduction_to_band factored by the blocked path (CholeskyQR2 + Householder
 * reconstruction, csrc/device/kernels_hr.hip) / handed back to the reflector-by-reflector kernel by its gate. */
DLAF_EXTERN_C int dlaf_mi355x_red2band_panel_stats(long* blocked, long* fallback) DLAF_NOEXCEPT;
/* Gives the idle blocks of the workspace pool back to the driver (the stages' temporaries of 4 MiB and more are kept between
 * calls, up to DLAF_MI355X_POOL_GB = 64 GiB; the analogue of the reference's Umpire pools, src/memory/memory_chunk.cpp,
 * which dlaf::finalize releases).  Returns the bytes that were held. */
DLAF_EXTERN_C long dlaf_mi355x_workspace_pool_release(void) DLAF_NOEXCEPT;
/* Tune parameter eigensolver_min_band (include/dlaf/tune.h:71-75,128; default 100).  dlaf_initialize reads
 * DLAF_EIGENSOLVER_MIN_BAND and --dlaf:eigensolver-min-band like src/init.cpp:220; the setter is what the reference's
 * tests do with getTuneParameters().eigensolver_min_band (test/unit/eigensolver/test_eigensolver.cpp:142). b_min >= 2. */
DLAF_EXTERN_C int dlaf_mi355x_get_eigensolver_min_band(void) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_set_eigensolver_min_band(int b_min) DLAF_NOEXCEPT;
/* get_band_size (include/dlaf/eigensolver/internal/get_band_size.h:20-31, tune parameter eigensolver_min_band): the band the
 * reference's eigensolver picks for a block size (128 for nb = 512) */
DLAF_EXTERN_C int dlaf_mi355x_get_band_size(int nb) DLAF_NOEXCEPT;
/* device time (ms, HIP events) and whole-grid flops in the reference miniapps' models (2 (2/3 n^3 - n^2 nb), resp.
 * 2 (n - band)^2 k; x4 complex: miniapp_reduction_to_band.cpp:163-168, miniapp_bt_reduction_to_band.cpp:160-164) of the last
 * reduction_to_band / bt_reduction_to_band on this process */
DLAF_EXTERN_C int dlaf_mi355x_red2band_profile(double* ms, double* flops) DLAF_NOEXCEPT;

/* ---- the eigensolver stages behind reduction_to_band -------------------------------------- */
/* dlaf::eigensolver::internal::band_to_tridiagonal<Backend::MC>(grid, uplo = Lower, band_size, mat_a)
 * (include/dlaf/eigensolver/band_to_tridiag.h:74-97, :155-176; the reference has no C entry for the stage): a holds a
 * Hermitian band matrix in the lower band of its local part (what reduction_to_band leaves; everything below the band
 * is ignored).  d: n diagonal entries, e: n - 1 off-diagonal entries (real), v: n x n (ld ldv) compact Householder
 * reflectors with tau in the place of the leading 1, laid out as band_to_tridiag.h:40-72 says.  The outputs are complete
 * on every process. */
DLAF_EXTERN_C int dlaf_mi355x_band_to_tridiagonal_s(int context, const float* a, struct DLAF_descriptor desca, int band_size,
                                                  float* d, float* e, float* v, int ldv) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_band_to_tridiagonal_d(int context, const double* a, struct DLAF_descriptor desca, int band_size,
                                                  double* d, double* e, double* v, int ldv) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_band_to_tridiagonal_c(int context, const dlaf_complex_c* a, struct DLAF_descriptor desca, int band_size,
                                                  float* d, float* e, dlaf_complex_c* v, int ldv) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_band_to_tridiagonal_z(int context, const dlaf_complex_z* a, struct DLAF_descriptor desca, int band_size,
                                                  double* d, double* e, dlaf_complex_z* v, int ldv) DLAF_NOEXCEPT;
/* dlaf::eigensolver::internal::bt_band_to_tridiagonal(band_size, mat_e, mat_hh)
 * (include/dlaf/eigensolver/bt_band_to_tridiag.h:28-61), local form: e (n x ncols, column-major, ld lde) <- Q e with the
 * reflectors v as band_to_tridiagonal returned them */
DLAF_EXTERN_C int dlaf_mi355x_bt_band_to_tridiagonal_s(int band_size, int n, int ncols, const float* v, int ldv, float* e,
                                                     int lde) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_bt_band_to_tridiagonal_d(int band_size, int n, int ncols, const double* v, int ldv, double* e,
                                                     int lde) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_bt_band_to_tridiagonal_c(int band_size, int n, int ncols, const dlaf_complex_c* v, int ldv, dlaf_complex_c* e,
                                                     int lde) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_bt_band_to_tridiagonal_z(int band_size, int n, int ncols, const dlaf_complex_z* v, int ldv, dlaf_complex_z* e,
                                                     int lde) DLAF_NOEXCEPT;
/* dlaf::eigensolver::internal::tridiagonal_eigensolver (include/dlaf/eigensolver/tridiag_solver.h:30-60), local form:
 * d (n), e (n - 1) -> eigenvalues w (ascending) and eigenvectors z (n x n, column-major, ld ldz) by divide & conquer on
 * the GPU.  nb: the reference's block size (unused by the device algorithm, kept for the call shape). */
DLAF_EXTERN_C int dlaf_mi355x_tridiagonal_eigensolver_s(int n, int nb, const float* d, const float* e, float* w, float* z,
                                                        int ldz) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_tridiagonal_eigensolver_d(int n, int nb, const double* d, const double* e, double* w,
                                                        double* z, int ldz) DLAF_NOEXCEPT;
/* device time (ms) per stage of the last eigensolver call on this process: reduction_to_band, band_to_tridiagonal,
 * tridiagonal_eigensolver, bt_band_to_tridiagonal, bt_reduction_to_band */
DLAF_EXTERN_C int dlaf_mi355x_eigensolver_profile(double ms[5]) DLAF_NOEXCEPT;

/* ---- partial spectrum: the eigenvectors of a range of eigenvalue indices ------------------------------------ */
/* The *_partial_spectrum entries of later DLA-Future releases (they are not in the dlaf_c headers of the snapshot this
 * library models, so they are declared here under upstream's names).  [eigenvalues_index_begin, eigenvalues_index_end)
 * is a 0-based half-open range into the ascending eigenvalues, 0 <= begin <= end <= n.  w receives all n eigenvalues on
 * every rank, the same bits the full entry returns.  z keeps the full entries' description (n x n); its global column
 * j, j in [begin, end), receives the eigenvector of eigenvalue j and every other element of the local array is left
 * as the caller passed it.  begin == end is valid (z may then be a null pointer where the local column range is
 * empty).  A, B and the return value behave as in the full entries.  The p?syevd / p?heevd / p?sygvd / p?hegvd forms
 * take the full entries' argument lists with il, iu in front of info: 1-based and inclusive as in p?syevx (il = 1,
 * iu = 0: the empty range). */
DLAF_EXTERN_C int dlaf_symmetric_eigensolver_partial_spectrum_s(int dlaf_context, char uplo, float* a,
    struct DLAF_descriptor dlaf_desca, float* w, float* z, struct DLAF_descriptor dlaf_descz,
    int64_t eigenvalues_index_begin, int64_t eigenvalues_index_end) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_symmetric_generalized_eigensolver_partial_spectrum_s(int dlaf_context, char uplo, float* a,
    struct DLAF_descriptor dlaf_desca, float* b, struct DLAF_descriptor dlaf_descb, float* w, float* z,
    struct DLAF_descriptor dlaf_descz, int64_t eigenvalues_index_begin, int64_t eigenvalues_index_end) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_symmetric_generalized_eigensolver_factorized_partial_spectrum_s(int dlaf_context, char uplo,
    float* a, struct DLAF_descriptor dlaf_desca, float* b, struct DLAF_descriptor dlaf_descb, float* w, float* z,
    struct DLAF_descriptor dlaf_descz, int64_t eigenvalues_index_begin, int64_t eigenvalues_index_end) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pssyevd_partial_spectrum(char uplo, int n, float* a, int ia, int ja, const int desca[9],
    float* w, float* z, int iz, int jz, const int descz[9], int64_t il, int64_t iu, int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pssygvd_partial_spectrum(char uplo, int n, float* a, int ia, int ja, const int desca[9],
    float* b, int ib, int jb, const int descb[9], float* w, float* z, int iz, int jz, const int descz[9], int64_t il,
    int64_t iu, int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pssygvd_factorized_partial_spectrum(char uplo, int n, float* a, int ia, int ja,
    const int desca[9], float* b, int ib, int jb, const int descb[9], float* w, float* z, int iz, int jz,
    const int descz[9], int64_t il, int64_t iu, int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_symmetric_eigensolver_partial_spectrum_d(int dlaf_context, char uplo, double* a,
    struct DLAF_descriptor dlaf_desca, double* w, double* z, struct DLAF_descriptor dlaf_descz,
    int64_t eigenvalues_index_begin, int64_t eigenvalues_index_end) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_symmetric_generalized_eigensolver_partial_spectrum_d(int dlaf_context, char uplo, double* a,
    struct DLAF_descriptor dlaf_desca, double* b, struct DLAF_descriptor dlaf_descb, double* w, double* z,
    struct DLAF_descriptor dlaf_descz, int64_t eigenvalues_index_begin, int64_t eigenvalues_index_end) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_symmetric_generalized_eigensolver_factorized_partial_spectrum_d(int dlaf_context, char uplo,
    double* a, struct DLAF_descriptor dlaf_desca, double* b, struct DLAF_descriptor dlaf_descb, double* w, double* z,
    struct DLAF_descriptor dlaf_descz, int64_t eigenvalues_index_begin, int64_t eigenvalues_index_end) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pdsyevd_partial_spectrum(char uplo, int n, double* a, int ia, int ja, const int desca[9],
    double* w, double* z, int iz, int jz, const int descz[9], int64_t il, int64_t iu, int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pdsygvd_partial_spectrum(char uplo, int n, double* a, int ia, int ja, const int desca[9],
    double* b, int ib, int jb, const int descb[9], double* w, double* z, int iz, int jz, const int descz[9],
    int64_t il, int64_t iu, int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pdsygvd_factorized_partial_spectrum(char uplo, int n, double* a, int ia, int ja,
    const int desca[9], double* b, int ib, int jb, const int descb[9], double* w, double* z, int iz, int jz,
    const int descz[9], int64_t il, int64_t iu, int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_hermitian_eigensolver_partial_spectrum_c(int dlaf_context, char uplo, dlaf_complex_c* a,
    struct DLAF_descriptor dlaf_desca, float* w, dlaf_complex_c* z, struct DLAF_descriptor dlaf_descz,
    int64_t eigenvalues_index_begin, int64_t eigenvalues_index_end) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_hermitian_generalized_eigensolver_partial_spectrum_c(int dlaf_context, char uplo,
    dlaf_complex_c* a, struct DLAF_descriptor dlaf_desca, dlaf_complex_c* b, struct DLAF_descriptor dlaf_descb,
    float* w, dlaf_complex_c* z, struct DLAF_descriptor dlaf_descz, int64_t eigenvalues_index_begin,
    int64_t eigenvalues_index_end) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_hermitian_generalized_eigensolver_factorized_partial_spectrum_c(int dlaf_context, char uplo,
    dlaf_complex_c* a, struct DLAF_descriptor dlaf_desca, dlaf_complex_c* b, struct DLAF_descriptor dlaf_descb,
    float* w, dlaf_complex_c* z, struct DLAF_descriptor dlaf_descz, int64_t eigenvalues_index_begin,
    int64_t eigenvalues_index_end) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pcheevd_partial_spectrum(char uplo, int n, dlaf_complex_c* a, int ia, int ja,
    const int desca[9], float* w, dlaf_complex_c* z, int iz, int jz, const int descz[9], int64_t il, int64_t iu,
    int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pchegvd_partial_spectrum(char uplo, int n, dlaf_complex_c* a, int ia, int ja,
    const int desca[9], dlaf_complex_c* b, int ib, int jb, const int descb[9], float* w, dlaf_complex_c* z, int iz,
    int jz, const int descz[9], int64_t il, int64_t iu, int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pchegvd_factorized_partial_spectrum(char uplo, int n, dlaf_complex_c* a, int ia, int ja,
    const int desca[9], dlaf_complex_c* b, int ib, int jb, const int descb[9], float* w, dlaf_complex_c* z, int iz,
    int jz, const int descz[9], int64_t il, int64_t iu, int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_hermitian_eigensolver_partial_spectrum_z(int dlaf_context, char uplo, dlaf_complex_z* a,
    struct DLAF_descriptor dlaf_desca, double* w, dlaf_complex_z* z, struct DLAF_descriptor dlaf_descz,
    int64_t eigenvalues_index_begin, int64_t eigenvalues_index_end) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_hermitian_generalized_eigensolver_partial_spectrum_z(int dlaf_context, char uplo,
    dlaf_complex_z* a, struct DLAF_descriptor dlaf_desca, dlaf_complex_z* b, struct DLAF_descriptor dlaf_descb,
    double* w, dlaf_complex_z* z, struct DLAF_descriptor dlaf_descz, int64_t eigenvalues_index_begin,
    int64_t eigenvalues_index_end) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_hermitian_generalized_eigensolver_factorized_partial_spectrum_z(int dlaf_context, char uplo,
    dlaf_complex_z* a, struct DLAF_descriptor dlaf_desca, dlaf_complex_z* b, struct DLAF_descriptor dlaf_descb,
    double* w, dlaf_complex_z* z, struct DLAF_descriptor dlaf_descz, int64_t eigenvalues_index_begin,
    int64_t eigenvalues_index_end) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pzheevd_partial_spectrum(char uplo, int n, dlaf_complex_z* a, int ia, int ja,
    const int desca[9], double* w, dlaf_complex_z* z, int iz, int jz, const int descz[9], int64_t il, int64_t iu,
    int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pzhegvd_partial_spectrum(char uplo, int n, dlaf_complex_z* a, int ia, int ja,
    const int desca[9], dlaf_complex_z* b, int ib, int jb, const int descb[9], double* w, dlaf_complex_z* z, int iz,
    int jz, const int descz[9], int64_t il, int64_t iu, int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pzhegvd_factorized_partial_spectrum(char uplo, int n, dlaf_complex_z* a, int ia, int ja,
    const int desca[9], dlaf_complex_z* b, int ib, int jb, const int descb[9], double* w, dlaf_complex_z* z, int iz,
    int jz, const int descz[9], int64_t il, int64_t iu, int* info) DLAF_NOEXCEPT;
/* the tridiagonal stage alone: z is n x (end - begin), column j the eigenvector of eigenvalue begin + j; w all n */
DLAF_EXTERN_C int dlaf_mi355x_tridiagonal_eigensolver_partial_spectrum_s(int n, int nb, const float* d, const float* e,
    float* w, float* z, int ldz, long begin, long end) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_tridiagonal_eigensolver_partial_spectrum_d(int n, int nb, const double* d, const double* e,
    double* w, double* z, int ldz, long begin, long end) DLAF_NOEXCEPT;
/* index arithmetic of a partial spectrum (no GPU needed).  The drivers keep the wanted eigenvectors in an internal
 * matrix over the global columns [b0, end), b0 = (begin / nb) nb, whose columns [b0, begin) are zero padding.
 * out = {b0, column source rank of the internal matrix, local columns of it on process column mycol, the caller's local
 * column its first local column corresponds to, how many of its leading local columns are padding}. */
DLAF_EXTERN_C int dlaf_mi355x_partial_spectrum_plan(long n, int nb, int npcol, int mycol, int z_jsrc, long begin,
                                                    long end, long out[5]) DLAF_NOEXCEPT;

/* ---- eigenvalues only, and a partial spectrum selected by value ------------------------- */
/* Eigenvalues only.  reduction_to_band, band_to_tridiagonal, then bisection on Sturm counts of the tridiagonal matrix
 * for the eigenvalues [eigenvalues_index_begin, eigenvalues_index_end) (0-based, half-open, ascending): no divide &
 * conquer, no back-transformation, no eigenvector matrix, and per rank the n x n reflector matrix is the only n^2
 * allocation.  w[begin, end) is written -- the same bits on every rank -- and nothing else of w.  a is read only (the
 * uplo = 'L' triangle); the generalized entries leave the Cholesky factor in b as the eigensolver does (the
 * _factorized ones take it there).  The p?syevd / p?heevd / p?sygvd / p?hegvd forms carry the 1-based inclusive il, iu
 * of p?syevx in front of info (il = 1, iu = 0: the empty range).  Stages 3 and 4 of dlaf_mi355x_eigensolver_profile
 * read 0 afterwards and stage 2 holds the bisection.
 *
 * By value, LAPACK's range = 'V'.  The eigenpairs with eigenvalues in (vl, vu]: after band_to_tridiagonal the driver
 * counts the eigenvalues <= vl and <= vu (two Sturm counts of the computed tridiagonal matrix, agreed over the grid),
 * returns [*begin, *end) = [count(vl), count(vu)) and goes on exactly as the *_partial_spectrum entry does for that
 * index range: w receives all n eigenvalues, the global columns [*begin, *end) of z their eigenvectors, and nothing
 * else of z is written.  vl >= vu gives the empty range at count(vl).  The boundary is that of the Sturm counts: an
 * eigenvalue within rounding of vl or vu may fall on either side.  The ScaLAPACK-like forms return m = *end - *begin;
 * the columns written start at the number of eigenvalues not above vl. */
DLAF_EXTERN_C int dlaf_symmetric_eigenvalues_s(int dlaf_context, char uplo, const float* a, struct DLAF_descriptor
    dlaf_desca, float* w, int64_t eigenvalues_index_begin, int64_t eigenvalues_index_end) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_symmetric_generalized_eigenvalues_s(int dlaf_context, char uplo, const float* a, struct
    DLAF_descriptor dlaf_desca, float* b, struct DLAF_descriptor dlaf_descb, float* w, int64_t
    eigenvalues_index_begin, int64_t eigenvalues_index_end) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_symmetric_generalized_eigenvalues_factorized_s(int dlaf_context, char uplo, const float* a,
    struct DLAF_descriptor dlaf_desca, float* b, struct DLAF_descriptor dlaf_descb, float* w, int64_t
    eigenvalues_index_begin, int64_t eigenvalues_index_end) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_symmetric_eigensolver_partial_spectrum_by_value_s(int dlaf_context, char uplo, float* a, struct
    DLAF_descriptor dlaf_desca, float* w, float* z, struct DLAF_descriptor dlaf_descz, float vl, float vu, long*
    begin, long* end) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_symmetric_generalized_eigensolver_partial_spectrum_by_value_s(int dlaf_context, char uplo,
    float* a, struct DLAF_descriptor dlaf_desca, float* b, struct DLAF_descriptor dlaf_descb, float* w, float* z,
    struct DLAF_descriptor dlaf_descz, float vl, float vu, long* begin, long* end) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_symmetric_generalized_eigensolver_factorized_partial_spectrum_by_value_s(int dlaf_context, char
    uplo, float* a, struct DLAF_descriptor dlaf_desca, float* b, struct DLAF_descriptor dlaf_descb, float* w, float*
    z, struct DLAF_descriptor dlaf_descz, float vl, float vu, long* begin, long* end) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pssyevd_eigenvalues(char uplo, int n, const float* a, int ia, int ja, const int desca[9],
    float* w, int64_t il, int64_t iu, int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pssygvd_eigenvalues(char uplo, int n, const float* a, int ia, int ja, const int desca[9],
    float* b, int ib, int jb, const int descb[9], float* w, int64_t il, int64_t iu, int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pssygvd_eigenvalues_factorized(char uplo, int n, const float* a, int ia, int ja, const int
    desca[9], float* b, int ib, int jb, const int descb[9], float* w, int64_t il, int64_t iu, int* info)
    DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pssyevd_partial_spectrum_by_value(char uplo, int n, float* a, int ia, int ja, const int
    desca[9], float* w, float* z, int iz, int jz, const int descz[9], float vl, float vu, int* m, int* info)
    DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pssygvd_partial_spectrum_by_value(char uplo, int n, float* a, int ia, int ja, const int
    desca[9], float* b, int ib, int jb, const int descb[9], float* w, float* z, int iz, int jz, const int descz[9],
    float vl, float vu, int* m, int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pssygvd_factorized_partial_spectrum_by_value(char uplo, int n, float* a, int ia, int ja, const
    int desca[9], float* b, int ib, int jb, const int descb[9], float* w, float* z, int iz, int jz, const int
    descz[9], float vl, float vu, int* m, int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_symmetric_eigenvalues_d(int dlaf_context, char uplo, const double* a, struct DLAF_descriptor
    dlaf_desca, double* w, int64_t eigenvalues_index_begin, int64_t eigenvalues_index_end) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_symmetric_generalized_eigenvalues_d(int dlaf_context, char uplo, const double* a, struct
    DLAF_descriptor dlaf_desca, double* b, struct DLAF_descriptor dlaf_descb, double* w, int64_t
    eigenvalues_index_begin, int64_t eigenvalues_index_end) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_symmetric_generalized_eigenvalues_factorized_d(int dlaf_context, char uplo, const double* a,
    struct DLAF_descriptor dlaf_desca, double* b, struct DLAF_descriptor dlaf_descb, double* w, int64_t
    eigenvalues_index_begin, int64_t eigenvalues_index_end) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_symmetric_eigensolver_partial_spectrum_by_value_d(int dlaf_context, char uplo, double* a,
    struct DLAF_descriptor dlaf_desca, double* w, double* z, struct DLAF_descriptor dlaf_descz, double vl, double vu,
    long* begin, long* end) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_symmetric_generalized_eigensolver_partial_spectrum_by_value_d(int dlaf_context, char uplo,
    double* a, struct DLAF_descriptor dlaf_desca, double* b, struct DLAF_descriptor dlaf_descb, double* w, double* z,
    struct DLAF_descriptor dlaf_descz, double vl, double vu, long* begin, long* end) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_symmetric_generalized_eigensolver_factorized_partial_spectrum_by_value_d(int dlaf_context, char
    uplo, double* a, struct DLAF_descriptor dlaf_desca, double* b, struct DLAF_descriptor dlaf_descb, double* w,
    double* z, struct DLAF_descriptor dlaf_descz, double vl, double vu, long* begin, long* end) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pdsyevd_eigenvalues(char uplo, int n, const double* a, int ia, int ja, const int desca[9],
    double* w, int64_t il, int64_t iu, int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pdsygvd_eigenvalues(char uplo, int n, const double* a, int ia, int ja, const int desca[9],
    double* b, int ib, int jb, const int descb[9], double* w, int64_t il, int64_t iu, int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pdsygvd_eigenvalues_factorized(char uplo, int n, const double* a, int ia, int ja, const int
    desca[9], double* b, int ib, int jb, const int descb[9], double* w, int64_t il, int64_t iu, int* info)
    DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pdsyevd_partial_spectrum_by_value(char uplo, int n, double* a, int ia, int ja, const int
    desca[9], double* w, double* z, int iz, int jz, const int descz[9], double vl, double vu, int* m, int* info)
    DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pdsygvd_partial_spectrum_by_value(char uplo, int n, double* a, int ia, int ja, const int
    desca[9], double* b, int ib, int jb, const int descb[9], double* w, double* z, int iz, int jz, const int descz[9],
    double vl, double vu, int* m, int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pdsygvd_factorized_partial_spectrum_by_value(char uplo, int n, double* a, int ia, int ja,
    const int desca[9], double* b, int ib, int jb, const int descb[9], double* w, double* z, int iz, int jz, const int
    descz[9], double vl, double vu, int* m, int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_hermitian_eigenvalues_c(int dlaf_context, char uplo, const dlaf_complex_c* a, struct
    DLAF_descriptor dlaf_desca, float* w, int64_t eigenvalues_index_begin, int64_t eigenvalues_index_end)
    DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_hermitian_generalized_eigenvalues_c(int dlaf_context, char uplo, const dlaf_complex_c* a,
    struct DLAF_descriptor dlaf_desca, dlaf_complex_c* b, struct DLAF_descriptor dlaf_descb, float* w, int64_t
    eigenvalues_index_begin, int64_t eigenvalues_index_end) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_hermitian_generalized_eigenvalues_factorized_c(int dlaf_context, char uplo, const
    dlaf_complex_c* a, struct DLAF_descriptor dlaf_desca, dlaf_complex_c* b, struct DLAF_descriptor dlaf_descb, float*
    w, int64_t eigenvalues_index_begin, int64_t eigenvalues_index_end) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_hermitian_eigensolver_partial_spectrum_by_value_c(int dlaf_context, char uplo, dlaf_complex_c*
    a, struct DLAF_descriptor dlaf_desca, float* w, dlaf_complex_c* z, struct DLAF_descriptor dlaf_descz, float vl,
    float vu, long* begin, long* end) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_hermitian_generalized_eigensolver_partial_spectrum_by_value_c(int dlaf_context, char uplo,
    dlaf_complex_c* a, struct DLAF_descriptor dlaf_desca, dlaf_complex_c* b, struct DLAF_descriptor dlaf_descb, float*
    w, dlaf_complex_c* z, struct DLAF_descriptor dlaf_descz, float vl, float vu, long* begin, long* end)
    DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_hermitian_generalized_eigensolver_factorized_partial_spectrum_by_value_c(int dlaf_context, char
    uplo, dlaf_complex_c* a, struct DLAF_descriptor dlaf_desca, dlaf_complex_c* b, struct DLAF_descriptor dlaf_descb,
    float* w, dlaf_complex_c* z, struct DLAF_descriptor dlaf_descz, float vl, float vu, long* begin, long* end)
    DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pcheevd_eigenvalues(char uplo, int n, const dlaf_complex_c* a, int ia, int ja, const int
    desca[9], float* w, int64_t il, int64_t iu, int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pchegvd_eigenvalues(char uplo, int n, const dlaf_complex_c* a, int ia, int ja, const int
    desca[9], dlaf_complex_c* b, int ib, int jb, const int descb[9], float* w, int64_t il, int64_t iu, int* info)
    DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pchegvd_eigenvalues_factorized(char uplo, int n, const dlaf_complex_c* a, int ia, int ja,
    const int desca[9], dlaf_complex_c* b, int ib, int jb, const int descb[9], float* w, int64_t il, int64_t iu, int*
    info) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pcheevd_partial_spectrum_by_value(char uplo, int n, dlaf_complex_c* a, int ia, int ja, const
    int desca[9], float* w, dlaf_complex_c* z, int iz, int jz, const int descz[9], float vl, float vu, int* m, int*
    info) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pchegvd_partial_spectrum_by_value(char uplo, int n, dlaf_complex_c* a, int ia, int ja, const
    int desca[9], dlaf_complex_c* b, int ib, int jb, const int descb[9], float* w, dlaf_complex_c* z, int iz, int jz,
    const int descz[9], float vl, float vu, int* m, int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pchegvd_factorized_partial_spectrum_by_value(char uplo, int n, dlaf_complex_c* a, int ia, int
    ja, const int desca[9], dlaf_complex_c* b, int ib, int jb, const int descb[9], float* w, dlaf_complex_c* z, int
    iz, int jz, const int descz[9], float vl, float vu, int* m, int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_hermitian_eigenvalues_z(int dlaf_context, char uplo, const dlaf_complex_z* a, struct
    DLAF_descriptor dlaf_desca, double* w, int64_t eigenvalues_index_begin, int64_t eigenvalues_index_end)
    DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_hermitian_generalized_eigenvalues_z(int dlaf_context, char uplo, const dlaf_complex_z* a,
    struct DLAF_descriptor dlaf_desca, dlaf_complex_z* b, struct DLAF_descriptor dlaf_descb, double* w, int64_t
    eigenvalues_index_begin, int64_t eigenvalues_index_end) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_hermitian_generalized_eigenvalues_factorized_z(int dlaf_context, char uplo, const
    dlaf_complex_z* a, struct DLAF_descriptor dlaf_desca, dlaf_complex_z* b, struct DLAF_descriptor dlaf_descb,
    double* w, int64_t eigenvalues_index_begin, int64_t eigenvalues_index_end) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_hermitian_eigensolver_partial_spectrum_by_value_z(int dlaf_context, char uplo, dlaf_complex_z*
    a, struct DLAF_descriptor dlaf_desca, double* w, dlaf_complex_z* z, struct DLAF_descriptor dlaf_descz, double vl,
    double vu, long* begin, long* end) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_hermitian_generalized_eigensolver_partial_spectrum_by_value_z(int dlaf_context, char uplo,
    dlaf_complex_z* a, struct DLAF_descriptor dlaf_desca, dlaf_complex_z* b, struct DLAF_descriptor dlaf_descb,
    double* w, dlaf_complex_z* z, struct DLAF_descriptor dlaf_descz, double vl, double vu, long* begin, long* end)
    DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_hermitian_generalized_eigensolver_factorized_partial_spectrum_by_value_z(int dlaf_context, char
    uplo, dlaf_complex_z* a, struct DLAF_descriptor dlaf_desca, dlaf_complex_z* b, struct DLAF_descriptor dlaf_descb,
    double* w, dlaf_complex_z* z, struct DLAF_descriptor dlaf_descz, double vl, double vu, long* begin, long* end)
    DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pzheevd_eigenvalues(char uplo, int n, const dlaf_complex_z* a, int ia, int ja, const int
    desca[9], double* w, int64_t il, int64_t iu, int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pzhegvd_eigenvalues(char uplo, int n, const dlaf_complex_z* a, int ia, int ja, const int
    desca[9], dlaf_complex_z* b, int ib, int jb, const int descb[9], double* w, int64_t il, int64_t iu, int* info)
    DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pzhegvd_eigenvalues_factorized(char uplo, int n, const dlaf_complex_z* a, int ia, int ja,
    const int desca[9], dlaf_complex_z* b, int ib, int jb, const int descb[9], double* w, int64_t il, int64_t iu, int*
    info) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pzheevd_partial_spectrum_by_value(char uplo, int n, dlaf_complex_z* a, int ia, int ja, const
    int desca[9], double* w, dlaf_complex_z* z, int iz, int jz, const int descz[9], double vl, double vu, int* m, int*
    info) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pzhegvd_partial_spectrum_by_value(char uplo, int n, dlaf_complex_z* a, int ia, int ja, const
    int desca[9], dlaf_complex_z* b, int ib, int jb, const int descb[9], double* w, dlaf_complex_z* z, int iz, int jz,
    const int descz[9], double vl, double vu, int* m, int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_pzhegvd_factorized_partial_spectrum_by_value(char uplo, int n, dlaf_complex_z* a, int ia, int
    ja, const int desca[9], dlaf_complex_z* b, int ib, int jb, const int descb[9], double* w, dlaf_complex_z* z, int
    iz, int jz, const int descz[9], double vl, double vu, int* m, int* info) DLAF_NOEXCEPT;
/* the tridiagonal level, local: d (n), e (n - 1).  tridiagonal_eigenvalues: w[begin, end) = the eigenvalues [begin,
 * end) by bisection (nothing else of w is written; NaN for every wanted entry when d or e holds a NaN or an Inf).
 * tridiagonal_sturm_count: counts[i] = the number of eigenvalues <= shifts[i], dstebz's convention (-1 for every shift
 * when d or e is not finite).  sturm_layout: out = {pairs staged through LDS at a time, threads per workgroup}. */
DLAF_EXTERN_C int dlaf_mi355x_tridiagonal_eigenvalues_s(int n, const float* d, const float* e, float* w, long begin,
    long end) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_tridiagonal_sturm_count_s(int n, const float* d, const float* e, long nshifts, const
    float* shifts, long* counts) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_tridiagonal_eigenvalues_d(int n, const double* d, const double* e, double* w, long
    begin, long end) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_tridiagonal_sturm_count_d(int n, const double* d, const double* e, long nshifts, const
    double* shifts, long* counts) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_sturm_layout(int out[2]) DLAF_NOEXCEPT;

/* Device-resident operands: a general m x n matrix in HBM (tile layout; square blocks) as the right-hand side,
 * a dlaf_mi355x_matrix_t (the uplo triangle of a resident matrix, e.g. the factor dlaf_mi355x_cholesky_* left there)
 * as the triangular matrix.  b is overwritten by the solution; nothing crosses PCIe.  potrs_device = the two solves of
 * A X = B from the resident Cholesky factor.  Same requirements as the host entry. */
typedef struct dlaf_mi355x_gmatrix_s* dlaf_mi355x_gmatrix_t;
DLAF_EXTERN_C int dlaf_mi355x_gmatrix_create(int context, char type, struct DLAF_descriptor desc,
                                             dlaf_mi355x_gmatrix_t* out) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_gmatrix_destroy(dlaf_mi355x_gmatrix_t m) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_gmatrix_upload(dlaf_mi355x_gmatrix_t m, const void* host_local, int ld) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_gmatrix_download(dlaf_mi355x_gmatrix_t m, void* host_local, int ld) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_triangular_solver_device(char side, char uplo, char op, char diag, const void* alpha,
                                                       dlaf_mi355x_matrix_t a, dlaf_mi355x_gmatrix_t b) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_potrs_device(char uplo, dlaf_mi355x_matrix_t factor, dlaf_mi355x_gmatrix_t b) DLAF_NOEXCEPT;
/* bt_reduction_to_band on resident operands: c (general matrix) <- Q c, reflectors in v (uplo 'L'), taus on the host */
DLAF_EXTERN_C int dlaf_mi355x_bt_reduction_to_band_device(int band_size, dlaf_mi355x_gmatrix_t c, dlaf_mi355x_matrix_t v,
                                                          const void* taus) DLAF_NOEXCEPT;

/* Device time (ms, HIP events on the compute stream) of the sweep of the last triangular solve on this process
 * -- relayout and PCIe staging excluded -- and the whole-grid algorithmic flops it stands for (m n^2 for side
 * R, m^2 n for side L; x4 complex). */
DLAF_EXTERN_C int dlaf_mi355x_solver_profile(double* ms, double* flops) DLAF_NOEXCEPT;

/* triangular_multiplication on resident operands (a: the uplo triangle of a dlaf_mi355x_matrix_t, b: a general
 * resident matrix, overwritten by the product); nothing crosses PCIe.  Same requirements as the host entry. */
DLAF_EXTERN_C int dlaf_mi355x_triangular_multiplication_device(char side, char uplo, char op, char diag,
                                                               const void* alpha, dlaf_mi355x_matrix_t a,
                                                               dlaf_mi355x_gmatrix_t b) DLAF_NOEXCEPT;
/* hermitian_multiplication on resident operands (a: the uplo triangle of a dlaf_mi355x_matrix_t, b and c: general
 * resident matrices of the same size, blocks and source process; only c is written); nothing crosses PCIe.  Same
 * requirements as the host entry, with square blocks for b and c. */
DLAF_EXTERN_C int dlaf_mi355x_hermitian_multiplication_device(char side, char uplo, const void* alpha,
                                                              dlaf_mi355x_matrix_t a, dlaf_mi355x_gmatrix_t b,
                                                              const void* beta, dlaf_mi355x_gmatrix_t c) DLAF_NOEXCEPT;
/* general_multiplication on three resident general matrices of one context and element type (a, b as stored, see the
 * host entry; only c is written); nothing crosses PCIe.  Same requirements as the host entry; a handle or scalar that
 * is null returns -1. */
DLAF_EXTERN_C int dlaf_mi355x_general_multiplication_device(char opa, char opb, const void* alpha,
                                                            dlaf_mi355x_gmatrix_t a, dlaf_mi355x_gmatrix_t b,
                                                            const void* beta, dlaf_mi355x_gmatrix_t c) DLAF_NOEXCEPT;
/* The Hermitian rank-k / rank-2k updates on resident operands: c a dlaf_mi355x_matrix_t created with this uplo (the
 * operand of dlaf_mi355x_matrix_factorize, gen_to_std and the eigensolvers), a and b general resident matrices as stored
 * (n x k for trans 'N', k x n for 'C'); only c's uplo triangle is written, nothing crosses PCIe.  alpha points to a real
 * (rank-k) or to an element (rank-2k), beta to a real, of c's precision.  Semantics and requirements of the host
 * entries; a handle or scalar that is null returns -1. */
DLAF_EXTERN_C int dlaf_mi355x_hermitian_rank_k_update_device(char uplo, char trans, const void* alpha,
                                                             dlaf_mi355x_gmatrix_t a, const void* beta,
                                                             dlaf_mi355x_matrix_t c) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_hermitian_rank_2k_update_device(char uplo, char trans, const void* alpha,
                                                              dlaf_mi355x_gmatrix_t a, dlaf_mi355x_gmatrix_t b,
                                                              const void* beta, dlaf_mi355x_matrix_t c) DLAF_NOEXCEPT;
/* The weighted rank-k update on resident operands: as dlaf_mi355x_hermitian_rank_k_update_device, with d the k real
 * weights of c's precision in HOST memory (null only while k = 0 or alpha = 0). */
DLAF_EXTERN_C int dlaf_mi355x_hermitian_weighted_rank_k_update_device(char uplo, char trans, const void* alpha,
                                                                      dlaf_mi355x_gmatrix_t a, const void* d,
                                                                      const void* beta,
                                                                      dlaf_mi355x_matrix_t c) DLAF_NOEXCEPT;
/* Functions of a resident Hermitian matrix, A := f(A) in place (a created with uplo 'L'): w receives the n eigenvalues
 * (reals of a's precision); weights is a dlaf_mi355x_spectral_weights_s (types s, c) or _d (d, z); value_interval points
 * to two reals of a's precision; exponent and threshold are doubles.  Nothing but w crosses PCIe.  Semantics and
 * requirements of the host entries; a null handle or w returns -1; on a non-zero status a holds what the eigensolver
 * left there. */
DLAF_EXTERN_C int dlaf_mi355x_hermitian_function_device(dlaf_mi355x_matrix_t a, void* w, void* weights, void* user,
                                                        const long* index_range, const void* value_interval,
                                                        long* selected) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_hermitian_power_device(dlaf_mi355x_matrix_t a, void* w, double exponent, double threshold,
                                                     long* n_dropped) DLAF_NOEXCEPT;
/* general_addition / hermitian_complete on resident general matrices of one context and element type (a as stored; only
 * c's uplo part is written; the same handle twice is op 'N' in place), and the resident conversions between a
 * dlaf_mi355x_matrix_t (one triangle) and a general matrix of the same context, type, order, block and source process,
 * defined by what the download of either object shows: matrix_to_general writes into g the Hermitian (kind 'H') /
 * symmetric ('S') matrix whose stored triangle m holds, or the triangular one ('T': exact zeros in the other triangle);
 * matrix_from_general takes m's stored triangle from g.  Nothing crosses PCIe.  Semantics and requirements of the host
 * entries; a handle or scalar that is null returns -1. */
DLAF_EXTERN_C int dlaf_mi355x_general_addition_device(char uplo, char op, const void* alpha, dlaf_mi355x_gmatrix_t a,
                                                      const void* beta, dlaf_mi355x_gmatrix_t c) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_hermitian_complete_device(char uplo, char kind, dlaf_mi355x_gmatrix_t a) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_matrix_to_general(char kind, dlaf_mi355x_matrix_t m, dlaf_mi355x_gmatrix_t g) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_matrix_from_general(dlaf_mi355x_matrix_t m, dlaf_mi355x_gmatrix_t g) DLAF_NOEXCEPT;
/* Device time (ms, HIP events) of the last of them on this process and the whole-grid algorithmic bytes it stands for:
 * read A + write C, + read C when beta != 0, over the uplo part; a completion reads and writes half the matrix. */
DLAF_EXTERN_C int dlaf_mi355x_addition_profile(double* ms, double* bytes) DLAF_NOEXCEPT;
/* Device time (ms, HIP events on the compute stream) of the sweep of the last triangular multiplication on this
 * process -- relayout and PCIe staging excluded -- and the whole-grid algorithmic flops it stands for (m n^2 for
 * side R, m^2 n for side L; x4 complex), as dlaf_mi355x_solver_profile.  The last multiplication of EITHER kind is
 * reported: after a Hermitian multiplication, its sweep and twice those flops (2 m n^2 / 2 m^2 n; x4 complex); after a
 * general multiplication, its sweep and 2 m n k (x4 complex); after a Hermitian rank-k update, its sweep and k n (n + 1)
 * (rank-2k: twice that; x4 complex). */
DLAF_EXTERN_C int dlaf_mi355x_multiplication_profile(double* ms, double* flops) DLAF_NOEXCEPT;

/* ---- synthetic input ------------------------------------------------------------------------ */
/* Fills this process's local array (column-major, ld) of the n x n matrix with the reference's
 * random Hermitian positive definite matrix: per global tile a std::mt19937_64 seeded with the
 * tile's origin, uniform(-1,1) off the diagonal, 2n added on it (util_matrix.h:323-442,498-501).
 * nthreads <= 0: all hardware threads. */
DLAF_EXTERN_C int dlaf_mi355x_set_random_hpd(int context, char type, void* host_local,
                                             struct DLAF_descriptor desc, int nthreads) DLAF_NOEXCEPT;

/* ---- tile operations (host operands, column-major) -------------------------------------------- */
/* potrf: returns LAPACK info (reference: lapack/tile.h:362-378) */
DLAF_EXTERN_C int dlaf_mi355x_tile_potrf(char type, char uplo, int n, void* a, int lda) DLAF_NOEXCEPT;
/* trsm: uplo L: B(m x n) <- B A^-H, A n x n lower;  uplo U: B <- A^-H B, A m x m upper
 * (Right/Lower/ConjTrans and Left/Upper/ConjTrans, NonUnit, alpha 1: impl.h:56-67,:110-121) */
DLAF_EXTERN_C int dlaf_mi355x_tile_trsm(char type, char uplo, int m, int n, const void* a, int lda, void* b,
                                        int ldb) DLAF_NOEXCEPT;
/* herk: uplo L: lower(C) -= A A^H, A n x k;  uplo U: upper(C) -= A^H A, A k x n (impl.h:70-80,:124-134) */
DLAF_EXTERN_C int dlaf_mi355x_tile_herk(char type, char uplo, int n, int k, const void* a, int lda, void* c,
                                        int ldc) DLAF_NOEXCEPT;
/* gemm: uplo L: C(m x n) -= A B^H, A m x k, B n x k;  uplo U: C -= A^H B, A k x m, B k x n
 * (impl.h:83-94,:137-147) */
DLAF_EXTERN_C int dlaf_mi355x_tile_gemm(char type, char uplo, int m, int n, int k, const void* a, int lda,
                                        const void* b, int ldb, void* c, int ldc) DLAF_NOEXCEPT;

/* ---- the grouped update kernel, one launch (host operands) -------------------------------------- */
/* Every field of one launch of the update kernel that a driver sets (the kernel's contract: UpdateArgs in
 * csrc/device/device_api.hpp).  The entry uploads the operands, launches ONCE and downloads C; the tests compare the
 * kernel itself, at any geometry, with a reference.  Strides, leading dimensions and *_elems are in elements of the
 * type; an operand's host array of *_elems elements is placed *_off elements into a fresh device allocation (off = 1:
 * a base that is not 16-byte aligned). */
struct dlaf_mi355x_update_desc {
  long c_elems, a_elems, b_elems, a2_elems, b2_elems;
  long c_off, a_off, b_off, a2_off, b2_off;
  /* tile_layout != 0: C is ltr x ltc local tiles of nb x nb in tile layout and the panels hold nb x K tiles (ld nb);
   * c_tsr / c_tsc / ldc / a_ts / lda / ldb / pr / ri / pc / ci / nt / last_rows / rect / nt_c / last_cols below are
   * then derived from (ltr, nb, pr, ri, pc, ci, nt, last_rows, rect, nt_c, last_cols) the way the drivers derive them */
  int tile_layout, ltr, ltc;
  long c_tsr, c_tsc;
  int ldc;
  long a_ts;
  int lda;
  long b_ts;
  int ldb;
  int b_period;
  long b_ts2;
  int b_jl0;
  int il0, il1, jl0, jl1, nb, K;
  int pr, ri, pc, ci;
  int nt, last_rows;
  int rect, nt_c, last_cols;
  int K1, her2k; /* K1 > 0: a2 / b2 are read */
  int info;      /* value of the device info word the kernel looks at */
  int role;      /* 0 .. 4 */
  long max_blocks; /* 0: one workgroup per work item; > 0: persistent form with at most that many; < 0: this GPU's
                    * workgroup slots for the type (what the drivers pass for the bulk launches) */
  int excl_rounds; /* whole rounds of exclusive compute units (0: none) */
  /* out */
  long persistent, exclusive; /* launches that took the persistent / exclusive form (0 or 1 per launch) */
  long bulk_slots;            /* this GPU's workgroup slots for the type */
  /* in */
  int second_below; /* K1 > 0: a2 / b2 share one device allocation with a / b and lie in front of them, so the second
                     * panel's address is below the first's whatever the allocator does (0: allocations of their own) */
};
/* c (c_elems elements) is updated in place.  c_again != NULL: the launch is repeated on a fresh copy of the original
 * c with the SAME 16 counter words, not zeroed by the caller (counters_are_zero = false), into c_again.
 * Returns 0, -1 for an unknown type / role, -3 when a field would make the kernel touch memory outside an operand. */
DLAF_EXTERN_C int dlaf_mi355x_update_direct_s(struct dlaf_mi355x_update_desc* d, void* c, const void* a, const void* b,
                                              const void* a2, const void* b2, void* c_again) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_update_direct_d(struct dlaf_mi355x_update_desc* d, void* c, const void* a, const void* b,
                                              const void* a2, const void* b2, void* c_again) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_update_direct_c(struct dlaf_mi355x_update_desc* d, void* c, const void* a, const void* b,
                                              const void* a2, const void* b2, void* c_again) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_update_direct_z(struct dlaf_mi355x_update_desc* d, void* c, const void* a, const void* b,
                                              const void* a2, const void* b2, void* c_again) DLAF_NOEXCEPT;
/* this GPU's workgroup slots of the bulk update kernel for the type (initialises the runtime) */
DLAF_EXTERN_C long dlaf_mi355x_update_bulk_slots(char type) DLAF_NOEXCEPT;

/* ---- triangular inverse and inverse from the Cholesky factor (LAPACK xTRTRI / xPOTRI) --------------------- */
/* triangular_inverse: a <- inv(a) for the triangular matrix in a's uplo triangle (diag 'N' / 'U'), in place.  Nothing
 * outside the uplo triangle is read or written, with diag 'U' the stored diagonal neither.
 * inverse_from_cholesky_factor: a's uplo triangle holds the Cholesky factor (dlaf_p?potrf output) and is overwritten
 * by the same triangle of inv(L L^H) (uplo 'L') / inv(U^H U) (uplo 'U'); the diagonal of the result is real.
 * Square matrix, square blocks, offsets 0, any source process.  Return LAPACK's info: 0, or i > 0 when the i-th
 * diagonal element (1-based, global) of a non-unit triangular operand is exactly zero -- the check runs before anything
 * is written, a comes back untouched; the same value on every rank.  The p?trtri / p?potri names take ScaLAPACK's
 * argument lists (ia = ja = 1). */
DLAF_EXTERN_C int dlaf_mi355x_triangular_inverse_s(int context, char uplo, char diag, float* a,
                                                   struct DLAF_descriptor desca) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_inverse_from_cholesky_factor_s(int context, char uplo, float* a,
                                                             struct DLAF_descriptor desca) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pstrtri(char uplo, char diag, int n, float* a, int ia, int ja, const int desca[9],
                                       int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pspotri(char uplo, int n, float* a, int ia, int ja, const int desca[9],
                                       int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_triangular_inverse_d(int context, char uplo, char diag, double* a,
                                                   struct DLAF_descriptor desca) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_inverse_from_cholesky_factor_d(int context, char uplo, double* a,
                                                             struct DLAF_descriptor desca) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pdtrtri(char uplo, char diag, int n, double* a, int ia, int ja, const int desca[9],
                                       int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pdpotri(char uplo, int n, double* a, int ia, int ja, const int desca[9],
                                       int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_triangular_inverse_c(int context, char uplo, char diag, dlaf_complex_c* a,
                                                   struct DLAF_descriptor desca) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_inverse_from_cholesky_factor_c(int context, char uplo, dlaf_complex_c* a,
                                                             struct DLAF_descriptor desca) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pctrtri(char uplo, char diag, int n, dlaf_complex_c* a, int ia, int ja, const int desca[9],
                                       int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pcpotri(char uplo, int n, dlaf_complex_c* a, int ia, int ja, const int desca[9],
                                       int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_triangular_inverse_z(int context, char uplo, char diag, dlaf_complex_z* a,
                                                   struct DLAF_descriptor desca) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_inverse_from_cholesky_factor_z(int context, char uplo, dlaf_complex_z* a,
                                                             struct DLAF_descriptor desca) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pztrtri(char uplo, char diag, int n, dlaf_complex_z* a, int ia, int ja, const int desca[9],
                                       int* info) DLAF_NOEXCEPT;
DLAF_EXTERN_C void dlaf_mi355x_pzpotri(char uplo, int n, dlaf_complex_z* a, int ia, int ja, const int desca[9],
                                       int* info) DLAF_NOEXCEPT;
/* the same on a device-resident matrix (uplo must be the one it was created with) */
DLAF_EXTERN_C int dlaf_mi355x_triangular_inverse_device(char uplo, char diag, dlaf_mi355x_matrix_t m) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_inverse_from_cholesky_factor_device(char uplo, dlaf_mi355x_matrix_t m) DLAF_NOEXCEPT;
/* Device time (ms, HIP events on the compute stream; relayout and PCIe staging excluded) of the last of these calls on
 * this process and the whole-grid flops it stands for: n^3 / 3 for the triangular inverse, as much again for the
 * product (x 4 for complex types). */
DLAF_EXTERN_C int dlaf_mi355x_inverse_profile(double* ms, double* flops) DLAF_NOEXCEPT;
/* index arithmetic of the two sweeps (no GPU needed).  plan: out = {local diagonal tiles, first global one, global
 * step, il0, jl0, il step, jl step, extent of the last, workspace tiles}; step k: out = {owner row, owner column, first
 * local row below k, local rows before k, local columns before k, local row of k or -1, local column of k or -1}. */
DLAF_EXTERN_C int dlaf_mi355x_inverse_plan(long n, int nb, int nprow, int npcol, int myrow, int mycol, int isrc,
                                           int jsrc, long out[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_inverse_step(long n, int nb, int nprow, int npcol, int myrow, int mycol, int isrc,
                                           int jsrc, long k, long out[7]) DLAF_NOEXCEPT;

/* ---- matrix norms (LAPACK xLANGE, xLANHE / xLANSY, xLANTR) --------------------------------------------------- */
/* norm: 'M' max |a_ij|, '1' / 'O' max column sum, 'I' max row sum, 'F' / 'E' Frobenius, either case.
 * general_norm: the m x n matrix.  hermitian_norm: the Hermitian (s, d: symmetric) n x n matrix whose uplo triangle a
 * holds; only the real part of its diagonal is used.  triangular_norm: the triangular matrix in a's uplo triangle;
 * with diag 'U' the stored diagonal is not read and counts as 1.  Nothing outside the referenced part influences the
 * value, and a is only read.  Square blocks, offsets 0, any source process.  *value (for s / c the float result
 * widened) is the same on every rank; any NaN in the referenced part gives NaN, otherwise any Inf gives +Inf; m = 0 or
 * n = 0 gives 0.  Return 0, or -1 bad norm, -2 bad uplo, -3 bad diag, -4 descriptor (offsets, blocks, sizes, square
 * for the Hermitian and the triangular form), -5 source process outside the grid, -6 value or context missing --
 * all decided before the GPU is touched.  The p?lan* names take ScaLAPACK's argument lists without `work`
 * (ia = ja = 1) and return the value. */
DLAF_EXTERN_C int dlaf_mi355x_general_norm_s(int context, char norm, const float* a, struct DLAF_descriptor desca,
                                             double* value) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_general_norm_d(int context, char norm, const double* a, struct DLAF_descriptor desca,
                                             double* value) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_general_norm_c(int context, char norm, const dlaf_complex_c* a,
                                             struct DLAF_descriptor desca, double* value) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_general_norm_z(int context, char norm, const dlaf_complex_z* a,
                                             struct DLAF_descriptor desca, double* value) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_hermitian_norm_s(int context, char norm, char uplo, const float* a,
                                               struct DLAF_descriptor desca, double* value) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_hermitian_norm_d(int context, char norm, char uplo, const double* a,
                                               struct DLAF_descriptor desca, double* value) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_hermitian_norm_c(int context, char norm, char uplo, const dlaf_complex_c* a,
                                               struct DLAF_descriptor desca, double* value) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_hermitian_norm_z(int context, char norm, char uplo, const dlaf_complex_z* a,
                                               struct DLAF_descriptor desca, double* value) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_triangular_norm_s(int context, char norm, char uplo, char diag, const float* a,
                                                struct DLAF_descriptor desca, double* value) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_triangular_norm_d(int context, char norm, char uplo, char diag, const double* a,
                                                struct DLAF_descriptor desca, double* value) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_triangular_norm_c(int context, char norm, char uplo, char diag, const dlaf_complex_c* a,
                                                struct DLAF_descriptor desca, double* value) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_triangular_norm_z(int context, char norm, char uplo, char diag, const dlaf_complex_z* a,
                                                struct DLAF_descriptor desca, double* value) DLAF_NOEXCEPT;
DLAF_EXTERN_C float dlaf_mi355x_pslange(char norm, int m, int n, const float* a, int ia, int ja,
                                        const int desca[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C double dlaf_mi355x_pdlange(char norm, int m, int n, const double* a, int ia, int ja,
                                         const int desca[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C float dlaf_mi355x_pclange(char norm, int m, int n, const dlaf_complex_c* a, int ia, int ja,
                                        const int desca[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C double dlaf_mi355x_pzlange(char norm, int m, int n, const dlaf_complex_z* a, int ia, int ja,
                                         const int desca[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C float dlaf_mi355x_pslansy(char norm, char uplo, int n, const float* a, int ia, int ja,
                                        const int desca[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C double dlaf_mi355x_pdlansy(char norm, char uplo, int n, const double* a, int ia, int ja,
                                         const int desca[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C float dlaf_mi355x_pclanhe(char norm, char uplo, int n, const dlaf_complex_c* a, int ia, int ja,
                                        const int desca[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C double dlaf_mi355x_pzlanhe(char norm, char uplo, int n, const dlaf_complex_z* a, int ia, int ja,
                                         const int desca[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C float dlaf_mi355x_pslantr(char norm, char uplo, char diag, int n, const float* a, int ia, int ja,
                                        const int desca[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C double dlaf_mi355x_pdlantr(char norm, char uplo, char diag, int n, const double* a, int ia, int ja,
                                         const int desca[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C float dlaf_mi355x_pclantr(char norm, char uplo, char diag, int n, const dlaf_complex_c* a, int ia, int ja,
                                        const int desca[9]) DLAF_NOEXCEPT;
DLAF_EXTERN_C double dlaf_mi355x_pzlantr(char norm, char uplo, char diag, int n, const dlaf_complex_z* a, int ia, int ja,
                                         const int desca[9]) DLAF_NOEXCEPT;
/* the same on resident operands: structure 'H' (Hermitian) or 'T' (triangular, diag 'N' / 'U') for the triangle a
 * dlaf_mi355x_matrix_t holds, and the general resident matrix */
DLAF_EXTERN_C int dlaf_mi355x_matrix_norm(dlaf_mi355x_matrix_t m, char norm, char structure, char diag,
                                          double* value) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_general_matrix_norm(dlaf_mi355x_gmatrix_t m, char norm, double* value) DLAF_NOEXCEPT;
/* measurement hook (tools/norm_bench.py): the device allocation that holds the local tiles of a resident general
 * matrix and its size, so that a read-rate yardstick can stream the very allocation the norm reads */
DLAF_EXTERN_C int dlaf_mi355x_gmatrix_device_tiles(dlaf_mi355x_gmatrix_t m, const void** tiles,
                                                   size_t* bytes) DLAF_NOEXCEPT;
/* device time (ms, HIP events on the operand's stream; upload excluded) of the last norm on this process and the bytes
 * of the tiles it referenced (diagonal tiles counted whole) */
DLAF_EXTERN_C int dlaf_mi355x_norm_profile(double* ms, double* bytes) DLAF_NOEXCEPT;

/* ---- the panel TRSM, one launch (host operands) -------------------------------------------------- */
/* Every field of one launch of the panel TRSM (the kernel's contract: TrsmArgs in csrc/device/device_api.hpp) and the
 * preparation of the inverted diagonal blocks that feeds it.  The entry uploads the operands, prepares winv, launches
 * launch_trsm ONCE and downloads the whole B and winv buffers.  Strides, leading dimensions, *_elems and *_off are in
 * elements of the type; an operand's host array of *_elems elements is placed *_off elements into a fresh device
 * allocation (off = 1: a base that is not 16-byte aligned; winv must stay 16-byte aligned). */
struct dlaf_mi355x_trsm_desc {
  long b_elems, l_elems, w_elems;
  long b_off, l_off, w_off;
  long b_ts;
  int ldb;
  int il0, il1, pr, ri;
  int nb, nt, last_rows;
  int ldl, n;
  int upper, prio;
  int info; /* value of the device info word before the launches */
  /* where winv comes from: 0 launch_invert_diag_blocks(l, ldl, n, upper, unit); 1 one launch_potrf_diag(factor = false,
   * upper, unit) per 64 x 64 diagonal block; 2 the caller's winv array as it is */
  int winv_source;
  int unit; /* sources 0 and 1: the diagonal of l is taken as 1 and not read */
  /* out */
  int path;     /* the kernel trsm_path chose: 0 strips, 1 rows-256, 2 rows-128, 3 rows-z */
  int vec;      /* strips: the 16-byte loaders */
  int info_out; /* the device info word after the launches */
};
/* b (b_elems) and winv (w_elems) are overwritten by the device buffers as the launches left them.
 * Returns 0, or -3 when a field would make a kernel touch memory outside an operand (nothing is launched). */
DLAF_EXTERN_C int dlaf_mi355x_trsm_direct_s(struct dlaf_mi355x_trsm_desc* d, void* b, const void* l, void* winv) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_trsm_direct_d(struct dlaf_mi355x_trsm_desc* d, void* b, const void* l, void* winv) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_trsm_direct_c(struct dlaf_mi355x_trsm_desc* d, void* b, const void* l, void* winv) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_trsm_direct_z(struct dlaf_mi355x_trsm_desc* d, void* b, const void* l, void* winv) DLAF_NOEXCEPT;

/* ---- the tile POTRF, one factorization (host operands) --------------------------------------------- */
/* Every field of one factorization of ONE kb x kb diagonal tile (the contract: launch_potrf_coop and launch_potrf_diag in
 * csrc/device/device_api.hpp).  The entry uploads the tile and winv buffers and *info, factors the tile once on the
 * chosen path and downloads both buffers whole.  ld, *_elems and *_off are in elements of the type; a host array of
 * *_elems elements is placed *_off elements into a fresh device allocation (t_off = 1: a tile that is not 16-byte
 * aligned; winv must stay 16-byte aligned).  The *_off elements in front of it are filled with a byte pattern before the
 * launches and looked at again afterwards. */
struct dlaf_mi355x_potrf_desc {
  long t_elems, w_elems;
  long t_off, w_off;
  int kb, ld;
  int info;      /* value of the device info word before the launches */
  int info_base; /* a failing column c reports info_base + c + 1 */
  int path;      /* 0: the cooperative launch; 1: the chain (diagonal block + TRSM + update per 64 columns) */
  /* path 0, who zeroes the hand-off words: 0 the launcher (sync_is_zero = false; the entry fills them with 0xFFFFFFFF
   * first), 1 the entry (sync_is_zero = true) */
  int sync_zeroed_by;
  int count_strips; /* path 0: the strips register in the per-compute-unit table of the bulk update */
  /* out */
  int info_out; /* the device info word after the launches */
  int t_before_changed, w_before_changed; /* bytes in front of the tile / winv buffer that the launches changed */
};
/* tile (t_elems) and winv (w_elems) are overwritten by the device buffers as the launches left them.
 * Returns 0, or -3 when a field would make a kernel touch memory outside a buffer (nothing is launched). */
DLAF_EXTERN_C int dlaf_mi355x_potrf_direct_s(struct dlaf_mi355x_potrf_desc* d, void* tile, void* winv) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_potrf_direct_d(struct dlaf_mi355x_potrf_desc* d, void* tile, void* winv) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_potrf_direct_c(struct dlaf_mi355x_potrf_desc* d, void* tile, void* winv) DLAF_NOEXCEPT;
DLAF_EXTERN_C int dlaf_mi355x_potrf_direct_z(struct dlaf_mi355x_potrf_desc* d, void* tile, void* winv) DLAF_NOEXCEPT;

/* ---- index helpers (no GPU needed) -------------------------------------------------------------- */
DLAF_EXTERN_C int dlaf_mi355x_dist_owner(long global_tile, int grid_size, int src_rank) DLAF_NOEXCEPT;
DLAF_EXTERN_C long dlaf_mi355x_dist_local_tile(long global_tile, int grid_size, int rank, int src_rank) DLAF_NOEXCEPT;
DLAF_EXTERN_C long dlaf_mi355x_dist_next_local_tile(long global_tile, int grid_size, int rank,
                                                    int src_rank) DLAF_NOEXCEPT;
DLAF_EXTERN_C long dlaf_mi355x_dist_global_tile(long local_tile, int grid_size, int rank, int src_rank) DLAF_NOEXCEPT;
DLAF_EXTERN_C long dlaf_mi355x_dist_local_size(long n, int nb, int grid_size, int rank, int src_rank) DLAF_NOEXCEPT;
DLAF_EXTERN_C long dlaf_mi355x_dist_local_tiles(long n, int nb, int grid_size, int rank, int src_rank) DLAF_NOEXCEPT;

/* library identification: "dlaf_mi355x <version> gfx950" */
DLAF_EXTERN_C const char* dlaf_mi355x_version(void) DLAF_NOEXCEPT;
