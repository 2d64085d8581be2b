// device_api.hpp -- host-callable launchers of the gfx950 tile kernels.  Everything here
// enqueues work on the given HIP stream and returns; no allocation, no synchronisation
// (the launchers are hipGraph-capturable).
#pragma once
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "geadd_map.hpp"
#include "norm_split.hpp"

namespace dlaf_mi355x {

// Zero device memory and RETURN ONLY WHEN IT IS ZERO.  On this stack hipMemset -- the "synchronous" entry -- returns
// before its fill kernel has run (measured: 3 us for a call queued behind a 200 ms kernel, tools/memset_sync_probe.hip,
// profiles/r04_memset_sync_probe.txt), and the fill sits on the null stream, which the library's non-blocking streams do
// not synchronise with: a status word "zeroed" that way can be zeroed again AFTER a kernel on another stream has
// written it.  State that kernels on other streams will touch is therefore zeroed with this, or on the stream that
// uses it.
inline hipError_t zero_device_now(void* p, size_t bytes) {
  hipError_t e = hipMemsetAsync(p, 0, bytes, nullptr);
  if (e == hipSuccess)
    e = hipStreamSynchronize(nullptr);
  return e;
}


// Block size of the diagonal factorization / inverted diagonal blocks used by the TRSM.
constexpr int kDiagBlock = 64;
// *info value stored by a kernel whose bounded inter-workgroup wait expired (workgroups of the cooperative
// POTRF not co-scheduled): a runtime failure, never a property of the matrix; the host aborts on it.
constexpr int kInfoSchedulingFailure = -1000000;

// ------------------------------------------------------------------------------------------
// Trailing update (tile::herk + tile::gemm of a whole step in ONE launch):
//   for local tiles (il, jl) in [il0,il1) x [jl0,jl1) with global indices gi = il*pr + ri,
//   gj = jl*pc + ci:   gi > gj:  C(il,jl) -= A(il) * B(jl)^H          (gemm, impl.h:83-94)
//                      gi == gj: lower(C(il,jl)) -= A(il) * B(jl)^H   (herk, impl.h:70-80)
//                      gi < gj:  nothing
// C lives in tile layout (tile (il,jl) at c + il*c_tsr + jl*c_tsc, leading dimension ldc);
// A(il) = a + (il-il0)*a_ts (rows(gi) x K, lda), B(jl) = b + (jl-jl0)*b_ts (rows(gj) x K, ldb).
// rows(g) = nb except for the last global tile g == nt-1 which has last_rows.
template <class T>
struct UpdateArgs {
  T* c;
  long c_tsr, c_tsc;
  int ldc;
  const T* a;
  long a_ts;
  int lda;
  const T* b;
  long b_ts;
  int ldb;
  int il0, il1, jl0, jl1;
  int nb, K;
  int pr, ri, pc, ci;
  int nt, last_rows;
  const int* info;  // device flag: non-zero => a previous POTRF failed, kernels return at once
  // rect != 0: every tile of the rectangle is a gemm (no triangle, no herk); the column axis then has its
  // own tile count / last extent (the triangular solver updates an m x n right-hand side, solver.cpp)
  int rect = 0;
  int nt_c = 0, last_cols = 0;
  // b_period > 1: the transposed panel is stored grouped by the process row that sent it (one broadcast
  // per root instead of one per tile): B(jl) = b + ((jl-jl0) % b_period) * b_ts2 + ((jl-jl0) / b_period) * b_ts
  int b_period = 1;
  long b_ts2 = 0;
  int b_jl0 = -1;  // local tile column that b stands for (-1: jl0)
  // Two-segment product (K1 > 0): columns k < K1 of the operands come from a / b, columns K1 <= k < K from
  // a2 / b2 (same tile strides and leading dimensions): two panels applied in one pass
  //     C -= A1 B1^H + A2 B2^H            (one read-modify-write of C for two steps of the factorization)
  // her2k != 0 (needs K1 > 0): with a = [X | L], b = [L | X] the launch computes C -= X L^H + L X^H; diagonal
  // tiles take their column operand from the column panel again with the segments swapped ([L_j | X_j]) and
  // keep the triangle mask (tile::her2k of gen_to_std).
  int K1 = 0;
  const T* a2 = nullptr;
  const T* b2 = nullptr;
  int her2k = 0;
};
// role: 0 trailing bulk, 1 lookahead column, 2 in-tile POTRF update / single-tile entries, 3 residual checker
// and triangular solver (same code, separate kernel names, so that profiles of the factorization stay clean),
// 4 triangular multiplication: the ADDITIVE form C += A * B^H (its own instantiation; every other role subtracts)
// max_blocks > 0 (with counters = 16 device words of scratch): launch at most that many workgroups and
// let them pull work items (persistent form): what is left of the GPU stays free for kernels that
// must run beside the update.  excl_slots > 0 (persistent form only): the workgroups that land on the first
// compute units of every XCD -- as many whole compute units as hold excl_slots workgroups -- leave at once, so
// max_blocks may cover the whole GPU and the side kernels still find compute units of their own.
template <class T>
void launch_update(const UpdateArgs<T>& args, hipStream_t stream, int role = 0, long max_blocks = 0,
                   unsigned* counters = nullptr, bool counters_are_zero = false, long excl_slots = 0);
template <class T>
int update_blocks_per_cu();
// workgroup slots of one whole round of exclusive compute units -- excl_slots is honoured in multiples of it (0: the
// compute-unit probe found nothing and no launch takes the exclusive form)
template <class T>
long update_exclusive_round();

// ------------------------------------------------------------------------------------------
// Panel TRSM (tile::trsm Right/Lower/ConjTrans/NonUnit of a whole panel in ONE launch,
// impl.h:56-67):   X(il) = B(il) * L^-H for local tiles il in [il0, il1), in place.
// L: n x n lower triangular (ldl); winv: ceil(n/64) inverted diagonal blocks of L, block j is a
// dense 64 x 64 column-major array at winv + j*64*64 (lower triangle valid, rest zero); winv is 16-byte aligned (every
// kernel reads it with 16-byte loads).  Which kernel runs: trsm_path.hpp.
template <class T>
struct TrsmArgs {
  T* b;
  long b_ts;
  int ldb;
  int il0, il1;
  int pr, ri;
  int nb, nt, last_rows;
  const T* l;
  int ldl;
  const T* winv;
  int n;
  const int* info;
  // upper != 0: X(il) = B(il) * U^-H with U = l upper triangular (the 64-column blocks are swept right to
  // left); winv block j then holds inv(U_jj) (upper triangle valid, rest zero)
  int upper = 0;
  // != 0: the waves run at raised priority (a panel solve on the critical path beside the bulk update)
  int prio = 0;
};
template <class T>
void launch_trsm(const TrsmArgs<T>& args, hipStream_t stream);

// ------------------------------------------------------------------------------------------
// Panel TRMM (the diagonal-tile step of triangular_multiplication):  X(il) = B(il) * L^H for local tiles il in
// [il0, il1), in place.  L: n x n (n <= nb, ldl), lower or upper; only its triangle is read, and with unit != 0
// not its diagonal either (taken as 1).  No inverse, no chain: the tiles' row strips are independent.
template <class T>
struct TrmmArgs {
  T* b;
  long b_ts;
  int ldb;
  int il0, il1;
  int pr, ri;
  int nb, nt, last_rows;
  const T* l;
  int ldl;
  int n;
  int upper = 0;
  int unit = 0;
};
template <class T>
void launch_trmm(const TrmmArgs<T>& args, hipStream_t stream);

// ------------------------------------------------------------------------------------------
// One step of the Hermitian multiplication (kernels_hemm.hip):  Y(il, jl) (+)= alpha X(il, l) H(l, j) for every
// local tile of Y in ONE launch, H Hermitian with its LOWER triangle stored.  H(l, j) of local column jl (global
// j = jl pc + ci) is taken from the stored triangle:
//   j > l : the adjoint of the stored tile H(j, l) at hc + (jl - jc0) hc_ts
//   j = l : the Hermitian image of the lower triangle of hd (its diagonal taken as real)
//   j < l : the stored tile H(l, j) as it is, at hr + jl hr_ts
// first != 0: Y = beta Y + ... (beta == 0: Y is not read); else Y += ...  conj_h: the stored tiles hold conj(H).
template <class T>
struct HemmArgs {
  T* y;
  long y_tsr, y_tsc;
  const T* x;
  long x_ts;
  const T* hc;
  long hc_ts;
  const T* hd;
  const T* hr;
  long hr_ts;
  int jc0;
  int l, K;       // the step's global tile column of X = tile row of H, and its extent
  int ltr, ltc;   // local tiles of Y
  int nb;         // tile size = leading dimension of every tile
  int pr, ri, nt_r, last_rows;
  int pc, ci, nt_c, last_cols;
  T alpha, beta;
  int first = 0;
  int conj_h = 0;
};
template <class T>
void launch_hemm(const HemmArgs<T>& args, hipStream_t stream);

// ------------------------------------------------------------------------------------------
// General multiplication (kernels_gemm.hip):  C(il, jl) = [first ? beta : 1] C(il, jl) + alpha sum_t opA(A)(il, t)
// opB(B)(t, jl) over the nk tiles t of the k dimension, for every local tile of C in ONE launch; a block of C stays in
// the accumulators over all of them.  The operands are tiles AS STORED (leading dimension nb), whatever the op:
//   opa N: the m x k tile of (il, t) at a + il a_ts + t a_ks;   T / C: the k x m tile of (t, il) at the same address
//   opb N: the k x n tile of (t, jl) at b + jl b_ts + t b_ks;   T / C: the n x k tile of (jl, t) at the same address
// Every k tile has nb values of k but the last, which has k_last.  nk == 0: C = beta C (first) and a, b are not read.
// first != 0 with beta == 0: C is not read.  (GemmArgs / launch_gemm, band_api.hpp, is the single product of two
// column-major matrices of the eigensolver stages.)
template <class T>
struct GeneralArgs {
  T* c;
  long c_tsr, c_tsc;
  const T* a;
  long a_ts, a_ks;
  const T* b;
  long b_ts, b_ks;
  char opa = 'N', opb = 'N';
  int nk, k_last;
  int ltr, ltc;   // local tiles of C
  int nb;         // tile size = leading dimension of every tile
  int pr, ri, nt_r, last_rows;
  int pc, ci, nt_c, last_cols;
  T alpha, beta;
  int first = 1;
};
template <class T>
void launch_general(const GeneralArgs<T>& args, hipStream_t stream);

// ------------------------------------------------------------------------------------------
// Hermitian rank-k / rank-2k update (kernels_herk.hip; index arithmetic and operand forms: herk_map.hpp) of the local
// tiles of the LOWER triangle of a square view V, in ONE launch, a block of V in the accumulators over all nk k tiles:
//   herk  : V(il, jl) = [first ? beta : 1] V(il, jl) + alpha sum_t x(il, t) y(jl, t)^H
//   her2k : ... + alpha sum_t x(il, t) y2(jl, t)^H + conj(alpha) sum_t x2(il, t) y(jl, t)^H          (x2 != nullptr)
// x / y: the tiles of A (x2 / y2: of B) AS STORED for the local tile rows / columns of V -- trans N the nb x K tile of
// (row, t), trans C the K x nb tile of (t, row) -- tile idx of k tile t at base + herk_panel_offset(idx, period, ts, ts2)
// + t ks; B's panels share A's strides.  conj_view: V holds the plain transpose of an upper-stored C (conj(A), conj(B)
// and conj(alpha) take the place of A, B and alpha).  Tiles above the diagonal, and the elements of a diagonal tile
// above it, are neither read nor written.  On the diagonal the imaginary part of V is ignored and stored as 0.
// first != 0 with beta == 0: V is not read.  nk == 0: V = beta V (first), the operands are not read.
template <class T>
struct RankKArgs {
  T* c;
  long c_tsr, c_tsc;
  const T* x;
  const T* y;
  const T* x2 = nullptr;
  const T* y2 = nullptr;
  long x_ts, x_ts2 = 0, y_ts, y_ts2 = 0, ks;
  int x_period = 1, y_period = 1;
  char trans = 'N';
  int conj_view = 0;
  int nk, k_last;
  int ltr, ltc;   // local tiles of V
  int nb;         // tile size = leading dimension of every tile
  int pr, ri, pc, ci, nt, last;  // block-cyclic geometry; nt tiles per dimension, the last one `last` wide
  T alpha;
  real_t<T> beta;
  int first = 1;
  // the weighted update (launch_rank_k_weighted; x2 == nullptr): x(il, t)[:, k] is multiplied by the real weight
  // kw[t nb + k] on its way into LDS -- kw a device pointer to the weight of k = 0 of k tile 0 of this launch.
  // conj_view leaves the weights alone (they are real).  launch_rank_k never reads it.
  const real_t<T>* kw = nullptr;
};
template <class T>
void launch_rank_k(const RankKArgs<T>& args, hipStream_t stream);
template <class T>
void launch_rank_k_weighted(const RankKArgs<T>& args, hipStream_t stream);

// ------------------------------------------------------------------------------------------
// Addition / transposition (kernels_geadd.hip; index arithmetic: geadd_map.hpp) of the `mask` part of the local tile
// rows [g.il0, g.il0 + g.nil) of D, every local tile column, in ONE launch:
//   D(il, jl) = beta D(il, jl) + alpha op(S(il, jl)),  op = identity (trans 0) or transpose (trans 1), conj on top
// S(il, jl): the source tile at a + geadd_src_tile_offset(...), ld nb like every tile.  arith (geadd_arith) says which of
// the two operands are read at all and whether anything is multiplied: kGeaddCopy moves bits.  diag_real: an element on
// the GLOBAL diagonal is stored with imaginary part 0.  ve: geadd_vector_elems of the two bases.  Elements outside the
// part, outside the local extents and the padding of ragged tiles are never written; nothing outside a tile's nb x nb
// storage is read.  a == c is allowed for trans 0, and for trans 1 when the part of D and the part of S that is USED
// are disjoint up to the diagonal (hermitian_complete): a workgroup reads its source sub-block whole before it writes.
template <class T>
struct GeaddArgs {
  T* c;
  long c_tsr, c_tsc;
  const T* a = nullptr;
  long a_tsi = 0, a_ts = 0, a_ts2 = 0;
  int a_period = 1;
  int trans = 0, conj = 0, mask = kGeaddAll, diag_real = 0;
  int arith = kGeaddCopy;
  int ve = 1;
  GeaddGeom g;
  T alpha, beta;
};
template <class T>
void launch_geadd(const GeaddArgs<T>& args, hipStream_t stream);

// ------------------------------------------------------------------------------------------
// Diagonal-tile work of triangular_inverse / inverse_from_cholesky_factor (kernels_inverse.hip).  A batch of
// `count` lower triangular tiles, tile t at base + t * stride (leading dimension ld), each nb x nb except the last,
// which is last x last.
template <class T>
struct TileBatch {
  T* base;
  long stride;
  int ld;
  int nb, count, last;
};
// N_t = -inv(T_t)^H (upper triangular, whole tile written, zero below the diagonal) at nout + t * nstride (ld as the
// tiles); winv + t * winv_stride: the inverted 64 x 64 diagonal blocks of tile t (launch_invert_diag_blocks, lower).
// Only the strictly lower blocks of T_t are read.
template <class T>
void launch_tile_trtri(const TileBatch<const T>& tiles, const T* winv, long winv_stride, T* nout, long nstride,
                       hipStream_t stream);
// lower(tile t) = lower(Z_t Z_t^H), Z_t = W_t^H upper triangular at z + t * zstride: the self-product W^H W of a lower
// triangular tile (xLAUUM); the diagonal comes out real.
template <class T>
void launch_tile_lauum(const TileBatch<T>& tiles, const T* z, long zstride, hipStream_t stream);
// mode 0: the lower triangle of src tile t into dst tile t (unit: without the diagonal), nothing else of dst touched;
// mode 1: dst tile t = lower(src tile t)^H, the whole tile (zero below the diagonal)
template <class T>
void launch_tri_tile(const TileBatch<T>& dst, const T* src, long sstride, int mode, bool unit, hipStream_t stream);
// *first = min(*first, i + 1) over the exactly-zero diagonal elements i (global index); tile t holds the global tile
// k0 + t * kstep.  The caller presets *first to 0xffffffff.
template <class T>
void launch_diag_zero_scan(const TileBatch<const T>& tiles, long k0, long kstep, unsigned* first, hipStream_t stream);

// ------------------------------------------------------------------------------------------
// Diagonal block factorization + inversion (one workgroup):  a (jb x jb, lda, jb <= 64) is
// overwritten by its lower Cholesky factor (strict upper part untouched); winv_block (64 x 64,
// ld 64) receives inv(L) (lower, zero elsewhere).  On a non-positive pivot at column c the
// kernel stores info_base + c + 1 into *info (first failure wins) and leaves a and winv_block as they were.
// *info != 0 on entry: nothing is read or written (a, winv_block and *info stay as they are).  The diagonal of a is
// taken as real when factoring: its imaginary part is ignored, and the diagonal of the factor is stored with imaginary
// part 0.
// factor == false: a already holds a triangular matrix; only winv_block is produced.  In that mode
// upper: a is upper triangular and winv_block receives inv(a) (upper); unit: the diagonal of a is taken as 1.
template <class T>
void launch_potrf_diag(T* a, int lda, int jb, T* winv_block, int* info, int info_base, hipStream_t stream,
                       bool factor = true, bool upper = false, bool unit = false);

// All ceil(kb/64) diagonal 64 x 64 blocks of one triangular kb x kb tile inverted in ONE launch (the
// triangular solver's per-tile preparation; nothing is factored, the tile is only read).
template <class T>
void launch_invert_diag_blocks(const T* tile, int ld, int kb, T* winv, int* info, hipStream_t stream, bool upper,
                               bool unit);

// Whole diagonal tile (kb x kb, ld) in one resident cooperative launch of ceil(kb/64) workgroups:
// lower Cholesky factor in place + the ceil(kb/64) inverted diagonal blocks in winv.  sync: device
// scratch of at least G + G*G unsigned, G = ceil(kb/64) (zeroed by the launcher on the stream):
// potrf_coop_sync_words(kb).
// Only the lower triangle of tile[0:kb, 0:kb] is read or written (the diagonal is taken as real and comes back with
// imaginary part 0); winv block j has the strict upper triangle and every row and column past the block's extent zero.
// A non-positive or NaN pivot at column c stores info_base + c + 1 into *info (first failure wins): the 64-column
// blocks left of the failing one, and their winv blocks, are final; the rest of the triangle is garbage.
// What an early exit leaves in winv differs between the two forms of the tile POTRF, and callers that broadcast winv
// whatever happened rely on it:
//   * this launch: every strip that leaves without factoring its diagonal block -- *info != 0 on entry (all
//     ceil(kb/64) strips: the tile and *info stay as they are), the failing strip and every strip below it, an expired
//     wait -- fills ITS 64 x 64 block of winv with NaN, real and imaginary parts;
//   * the chain (launch_potrf_diag + launch_trsm + launch_update per 64 columns): those blocks of winv are left as
//     they were; with *info != 0 on entry the tile, winv and *info are all untouched.
template <class T>
void launch_potrf_coop(T* tile, int ld, int kb, T* winv, int* info, int info_base, unsigned* sync,
                       hipStream_t stream, bool sync_is_zero = false, bool count_strips = true);
// count_strips: the strips register in the per-compute-unit table the bulk update kernel consults (the POTRF yield)
// update launches of this process so far in persistent form, and of those with exclusive compute units
void update_launch_stats(long* persistent, long* exclusive);
// diagnosis hook (DLAF_MI355X_POTRF_TRACE=1): 32 device words the launches of a factorization's FIRST diagonal tile
// write what their first two strips saw into (null: off); the caller zeroes them on the stream before the launch
unsigned long long* potrf_coop_trace_buffer();
inline size_t potrf_coop_sync_words(int kb) {
  const size_t g = (size_t) ((kb + kDiagBlock - 1) / kDiagBlock);
  return g + g * g;
}

// ------------------------------------------------------------------------------------------
// Layout kernels between the caller's column-major local array (staged on the device) and the
// tile layout (tile (il,jl) at dst + (il + jl*ltr) * nb*nb, ld = nb).
//   transpose == 0: tile(il,jl)[r][c]  = src[(il*nb + r) + (jl*nb + c)*lds]     (uplo = L)
//   transpose == 1: tile(il,jl)[r][c]  = src[(jl*nb + c) + (il*nb + r)*lds]     (uplo = U seen as
//                   the lower factorization of the transposed view; the view's tile grid is
//                   ltr x ltc with ltr = source tile COLUMNS)
// Only view-tiles with global row index >= global column index are moved (the uplo triangle);
// within diagonal tiles every element is moved to the device and only the triangle is moved back.
template <class T>
struct LayoutArgs {
  T* tiles;
  T* cm;         // column-major local array on the device
  long ld_cm;
  int ltr, ltc;  // local tile rows / cols of the (possibly transposed) VIEW
  int nb;
  long rows, cols;  // local element extents of the VIEW
  int pr, ri, pc, ci;  // global tile index of view-tile: gi = il*pr + ri, gj = jl*pc + ci
  int transpose;
  // general matrices (triangular solver operands): full != 0 moves every tile of the rectangle (no uplo
  // triangle); conj != 0 conjugates on the way (with transpose: the conjugate-transposed view); to-tiles
  // only: scale != 0 multiplies by alpha (the solver's alpha * B)
  int full = 0, conj = 0, scale = 0;
  T alpha{};
  // restrict the move to view tile columns [jl_first, jl_first + jl_count) (jl_count 0: to the last one)
  int jl_first = 0, jl_count = 0;
  // view row r / column c takes source view row rows-1-r / column cols-1-c (the solver turns a backward sweep over an
  // upper triangular matrix into the forward sweep of its reversal)
  int rev_rows = 0, rev_cols = 0;
};
template <class T>
void launch_to_tiles(const LayoutArgs<T>& args, hipStream_t stream);
template <class T>
void launch_from_tiles(const LayoutArgs<T>& args, hipStream_t stream);

template <class T>
void launch_copy2d(T* dst, long ldd, const T* src, long lds, int rows, int cols, int transpose, int mask,
                   hipStream_t stream);

// Batched tile transforms (gen_to_std): tile t at src + t*sstride (rows x cols, lds) -> dst + t*dstride.
//   mode 0: dst = src^H (cols x rows);  mode 1: dst = scale * (full Hermitian image of src's lower triangle);
//   mode 2: lower(dst) = lower(src^H), rest of dst untouched, real diagonal.
template <class T>
void launch_tile_xform(T* dst, long ldd, long dstride, const T* src, long lds, long sstride, int rows, int cols,
                       int count, int mode, double scale, hipStream_t stream);

// dst tile = alpha * op(src tile) for a batch of tiles; op: 0 adjoint, 3 transpose, 4 conjugate, 5 copy
template <class T>
void launch_tile_xform_alpha(T* dst, long ldd, long dstride, const T* src, long lds, long sstride, int rows, int cols,
                             int count, int mode, T alpha, bool use_alpha, hipStream_t stream);

// checker helpers: max |a_ij| over the lower triangle of the local tiles (into *out, device double) and
// zeroing of the strict upper part of the local diagonal tiles
template <class T>
void launch_max_norm(const T* tiles, int ltr, int ltc, int nb, long rows, long cols, int pr, int ri, int pc, int ci,
                     double* out, hipStream_t stream);
template <class T>
void launch_zero_upper_diag(T* tiles, int ltr, int ltc, int nb, int pr, int ri, int pc, int ci, hipStream_t stream);

// ---- matrix norms (kernels_norm.hip; work split and partial-buffer layout: norm_split.hpp) -------------------------
// Pass 1 streams the referenced tiles once and writes, with plain stores and one writer per slot, per-unit scalars
// (max, NaN flag, the big / medium / small accumulators of xLASSQ's sum of squares) and partial column / row sums;
// everything accumulates in fp64.  Only what `mode` needs is computed.  Structure 1 (Hermitian): strictly-lower stored
// elements count for (i, j) and (j, i) -- column AND row sums, weight 2 in the sum of squares --, the diagonal once and
// with its real part only.  Structure 2 (triangular): unit != 0 takes the diagonal as 1 without reading it.
enum NormMode : int { kNormMax = 0, kNormCol = 1, kNormRow = 2, kNormColRow = 3, kNormFro = 4 };
template <class T>
struct NormArgs {
  const T* tiles;
  NormGeom g;
  NormSplit s;
  int unit;
  int mode;
  double* scal;  // norm_unit_count * kNormScalars
  double* colp;  // norm_colp_elems (modes with column sums)
  double* rowp;  // norm_rowp_elems (modes with row sums)
};
template <class T>
void launch_norm_pass1(const NormArgs<T>& a, hipStream_t stream);
// Pass 2, fixed order: out[0 .. kNormScalars) from the scalars of all units (max, flag: max; accumulators: sum)
void launch_norm_scalars(const double* scal, long units, double* out, hipStream_t stream);
// v[x] for the global index x in [0, len): the column sums of global column x (mode & kNormCol) plus the row sums of
// global row x (mode & kNormRow) over this process's live units, 0 where it holds neither
void launch_norm_vector(const NormGeom& g, const NormSplit& s, int mode, const double* colp, const double* rowp,
                        double* v, long len, hipStream_t stream);
// *out = max of v[0 .. len) (0 for len == 0)
void launch_norm_vecmax(const double* v, long len, double* out, hipStream_t stream);

// one-off: opt the kernels into > 64 KiB of dynamic LDS
void device_kernels_init();

}  // namespace dlaf_mi355x
