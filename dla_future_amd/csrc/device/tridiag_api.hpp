// tridiag_api.hpp -- host-callable launchers of the gfx950 kernels of the eigensolver stages behind the reduction to
// band form: band -> tridiagonal (bulge chasing), the tridiagonal divide & conquer
// eigensolver, Sturm counts and bisection on the tridiagonal matrix, and the back-transformation band <- tridiagonal.
// Everything enqueues on the given stream.
//
// Reference: include/dlaf/eigensolver/band_to_tridiag/mc.h (the reference runs this stage on the CPU, one task per
// sweep step, also for GPU matrices), include/dlaf/eigensolver/tridiag_solver/{impl,merge}.h (leaf solver stedc and
// the deflation / secular-equation steps on the CPU, GEMMs on the GPU), include/dlaf/eigensolver/bt_band_to_tridiag/impl.h.
#pragma once
#include <hip/hip_runtime.h>

#include "common.hpp"

namespace dlaf_mi355x {

// ------------------------------------------------------------------------------------------ band storage
// band[c * ldb + o] = A(c + o, c), o in [0, ldb), ldb = 2 * b: the diagonal, the b sub-diagonals and b - 1 rows of
// room for the bulge (BandBlock, band_to_tridiag/mc.h:180-206: ld = 2 b - 1 between columns of the same row).
//
// From the lower tiles of a tile-layout matrix (tile (il, jl) at tiles + (il + jl * ltr) * nb^2, ld nb, global tile
// gi = il * pr + ri, gj = jl * pc + ci): the entries of tiles that are not local are set to zero (a process grid sums
// the images of its ranks).
template <class T>
void launch_band_extract(const T* tiles, long ltr, int nb, int pr, int ri, int pc, int ci, long n, int b, T* band,
                         hipStream_t stream);

// ------------------------------------------------------------------------------------------ band -> tridiagonal
// All sweeps in ONE launch of persistent workgroups: a workgroup draws the next sweep from a counter and runs its
// steps; step t of sweep s waits until sweep s - 1 has finished t + 2 steps (the counting semaphores of
// mc.h:683-709; the register kernel waits for step t and the first column of step t + 1, kernels_tridiag.hip).  Hand-offs between workgroups: write-through stores, sc1 loads, one progress word per sweep.
//   vout (n x n, ldv): the compact reflectors, tau in the place of the leading 1 (band_to_tridiag.h:56-63)
//   sync: b2t_sync_words(n) unsigned words, zeroed by the launcher
// Afterwards d[i] = 2^k Re band[i * ldb], e[i] = 2^k Re band[i * ldb + 1] (launch_tridiag_extract, k of
// launch_band_normalise).
template <class T>
void launch_band_to_tridiag(T* band, long n, int b, T* vout, long ldv, unsigned* sync, int* info, hipStream_t stream);
// (a sweep's progress word has a 128-byte line to itself: pollers and publishers of neighbouring sweeps would
//  otherwise meet in one L2 channel)
constexpr int kB2tProgressStride = 32;
inline size_t b2t_sync_words(long n) {
  return (size_t) n * kB2tProgressStride + 64;
}
// The band copy (n columns) <- 2^-k band copy, 2^k <= max(|Re|, |Im|) < 2^(k + 1), k = 0 for a band that is zero or
// not finite; mx (one 8-byte device word) keeps that max for launch_tridiag_extract.  The reflectors' xLARFG sums
// squares unscaled: in [1, 2) they neither overflow nor underflow for any scale of A, and a power of two is exact, so
// v(2^j A) = v(A) and (d, e)(2^j A) = 2^j (d, e)(A) bit for bit (LAPACK's xLARFG rescales for the same reason).
template <class T>
void launch_band_normalise(T* band, long n, int b, unsigned long long* mx, hipStream_t stream);
template <class T>
void launch_tridiag_extract(const T* band, long n, int b, const unsigned long long* mx, real_t<T>* d, real_t<T>* e,
                            hipStream_t stream);
int b2t_max_band();

// ------------------------------------------------------------------------------------------ band <- tridiagonal
// Block (ib, jb), ib >= jb, of the compact reflector matrix = the reflectors of the sweeps jb b .. jb b + b - 1 at step
// ib - jb (bt_band_to_tridiag.h:64-77).  Its well-formed image: vx + blk * 2 b * b, 2 b x b (ld 2 b), column k with its
// 1 in row k; taus + blk * b.  blk = jb * nblk + ib, nblk = ceil(n / b).  Columns that hold no reflector are zero.
template <class T>
void launch_b2t_expand(const T* vout, long ldv, long n, int b, T* vx, T* taus, hipStream_t stream, bool transposed = false);

// ------------------------------------------------------------------------------------------ eigenvector plumbing
// e[r + cl * lde] = (T) z[r + (gc - pad) * ldz]: the local columns cl of a block-cyclic column axis (pc processes, this
// one at position ci from the source, block nb) out of the replicated real eigenvector matrix z, whose column 0 is the
// axis' column `pad`; the axis' columns gc < pad (the padding in front of a partial spectrum) become zero
template <class R, class T>
void launch_cols_gather_cast(const R* z, long ldz, long n, int nb, int pc, int ci, long ncols_loc, long pad, T* e, long lde,
                             hipStream_t stream);
// the local tile rows (pr processes, position ri) of those columns into a tile-layout matrix of ltr x ltc tiles
template <class T>
void launch_rows_to_tiles(const T* e, long lde, long n, long ncols_loc, int nb, int pr, int ri, long ltr, long ltc, T* tiles,
                          hipStream_t stream);

// ------------------------------------------------------------------------------------------ Sturm counts, bisection
// (kernels_sturm.hip)  work: sturm_work_doubles(n) device doubles, 16-byte aligned: a header of
// kSturmHeader doubles, then the n pairs (2^-k d_i, (2^-k e_{i-1})^2), e_{-1} = 0.
constexpr int kSturmThreads = 64;           // one wave per workgroup, one thread per shift / per eigenvalue index
constexpr int kSturmChunk = 512;            // pairs staged through LDS at a time (two buffers of 8 KiB)
constexpr int kSturmMaxIterations = 1200;   // above any cap a finite matrix can ask for (2^3 / 2^-1074 and change)
constexpr int kSturmHeader = 8;
enum : int { kSturmGl = 0, kSturmGu, kSturmPivmin, kSturmK, kSturmBad, kSturmCap };
inline size_t sturm_work_doubles(long n) {
  return (size_t) kSturmHeader + 2 * (size_t) (n > 0 ? n : 0);
}
// d (n), e (n - 1), device, R = float | double.  Header: the Gershgorin interval [gl, gu] of the scaled matrix, widened
// as dstebz widens it; pivmin = DBL_MIN max(1, max e^2); k (2^k <= max(|d|, |e|) < 2^(k + 1); 0 for a zero or
// non-finite matrix); 1 when d or e holds a NaN or an Inf; the iteration cap of the bisection.
template <class R>
void launch_sturm_prepare(const R* d, const R* e, long n, double* work, hipStream_t stream);
// counts[s] = the number of eigenvalues <= shifts[s] (shifts in the caller's scale; dstebz's convention: pivots
// q <= pivmin); -1 for every shift when the matrix is not finite.  One thread per shift.
template <class R>
void launch_sturm_count(const double* work, long n, const R* shifts, long nshifts, long long* counts, hipStream_t stream);
// w[j], j in [begin, end) = eigenvalue j (0-based, ascending) by bisection on the counts, rounded to R once; nothing
// else of w is written.  NaN for every wanted entry when the matrix is not finite.  One thread per index.
template <class R>
void launch_sturm_bisect(const double* work, long n, long begin, long end, R* w, hipStream_t stream);

// ------------------------------------------------------------------------------------------ tridiagonal D&C
// (kernels of the divide & conquer solver: declared in tridiag_dc.hpp)

}  // namespace dlaf_mi355x
