// kernels_inverse.hip -- the diagonal-tile work of triangular_inverse and inverse_from_cholesky_factor
// (inverse.cpp): every kernel here takes a BATCH of lower triangular kb x kb tiles (tile t at base + t * stride,
// the last one possibly smaller), because no diagonal tile of the matrix depends on another tile's result and all
// of them go in one launch ahead of the sweep.
//
//   tile_trtri_kernel      N = -inv(T)^H (upper triangular) of a whole tile.  inv(T)^H T^H = I, so block ROW j of N
//                          (64 rows) is the forward substitution  N(j, :) T^H = -E_j  that starts at block column j:
//                              Y_i = -[i == j] I - sum_{j <= l < i} N(j, l) T(i, l)^H     (MFMA GEMM of mma_core.hpp)
//                              N(j, i) = Y_i inv(T_ii)^H                                  (MFMA, Y out of the accumulators)
//                          One workgroup per block row; the block rows are independent chains of different lengths
//                          (the longest first), the blocks left of the diagonal are zero and only written as such.
//                          inv(T_ii): the inverted 64 x 64 diagonal blocks of launch_invert_diag_blocks.  The ADJOINT
//                          of the inverse is what comes out because that is the form in which both products are the
//                          core's A B^H; it is also the operand the sweep's panel step multiplies by.
//   tile_lauum_kernel      lower(S) = lower(Z Z^H) for Z = W^H upper triangular (the tile self-product W^H W of one
//                          lower triangular W, xLAUUM): one workgroup per 64 x 64 block (i, j), i >= j, K range =
//                          the columns from 64 i on (what is left of them is zero by triangularity), real diagonal.
//   tri_tile_kernel        masked element moves: the triangle of a tile back into the matrix; Z = lower(W)^H.
//   diag_zero_scan_kernel  LAPACK's info of xTRTRI: the first exactly-zero diagonal element.
// None of them waits for another workgroup.
#include <type_traits>

#include "device_api.hpp"
#include "mma_core.hpp"

namespace dlaf_mi355x {

// 64 x 64 blocks, a wave owns 16 whole rows of the block (the second product feeds Y from the accumulators, as the
// panel TRSM does)
template <class T>
struct InvCfg {
  using type = BlockCfg<T, kDiagBlock, kDiagBlock, 16, kDiagBlock, 16>;
};
template <>
struct InvCfg<cdouble> {
  using type = BlockCfg<cdouble, kDiagBlock, kDiagBlock, 16, kDiagBlock, 8>;
};

template <class T>
constexpr int inv_lds_bytes() {
  using Cfg = typename InvCfg<T>::type;
  constexpr int w = (TypeInfo<T>::is_complex ? 2 : 1) * kDiagBlock * (kDiagBlock + kLdsPad) * (int) sizeof(real_t<T>);
  return Cfg::LDS_BYTES > w ? Cfg::LDS_BYTES : w;
}

template <class T>
__device__ __forceinline__ int batch_extent(const TileBatch<T>& b, int t) {
  return (t == b.count - 1) ? b.last : b.nb;
}

template <class T, bool VEC>
__global__ __launch_bounds__(kThreads) void tile_trtri_kernel(TileBatch<const T> tb, const T* __restrict__ winv,
                                                              long winv_stride, T* __restrict__ nout, long nstride,
                                                              int nblk) {
  using Cfg = typename InvCfg<T>::type;
  using R = real_t<T>;
  using acc_t = typename Mma<R>::acc_t;
  constexpr int JB = kDiagBlock;
  static_assert(Cfg::BM == JB && Cfg::BN == JB && Cfg::WAVES_N == 1 && Cfg::TM == 1, "a wave owns 16 rows of a block");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  R* lds = reinterpret_cast<R*>(lds_raw);

  const int t = blockIdx.x / nblk;
  const int j = nblk - 1 - (int) (blockIdx.x % nblk);  // (block row 0, the longest chain, is dispatched first)
  const int kb = batch_extent(tb, t);
  if (j * JB >= kb)
    return;
  const int ld = tb.ld;
  const T* Tt = tb.base + (long) t * tb.stride;
  const T* Wt = winv + (long) t * winv_stride;
  T* Nj = nout + (long) t * nstride + j * JB;  // block row j of N (ld as the tile)
  const int mrows = min(JB, kb - j * JB);
  const int njb = (kb + JB - 1) / JB;

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave;
  const int g = lane >> 4, c = lane & 15;

  // blocks left of the diagonal: zero
  for (int e = threadIdx.x; e < mrows * j * JB; e += kThreads)
    Nj[e % mrows + (long) (e / mrows) * ld] = zero_el<T>();

  for (int i = j; i < njb; ++i) {
    const int jb = min(JB, kb - i * JB);
    const int K = (i - j) * JB;  // columns [64 j, 64 i) of block row j are done
    const bool full = (mrows == JB) && (jb == JB);
    Acc<Cfg> y;
    y.clear();
    if (K > 0) {
      const T* Xs = Nj + (long) (j * JB) * ld;
      const T* Ti = Tt + i * JB + (long) (j * JB) * ld;
      if (full)
        gemm_nt_block<Cfg, T, VEC, false>(Xs, ld, mrows, Ti, ld, jb, K, lds, y);
      else
        gemm_nt_block<Cfg, T, false, true>(Xs, ld, mrows, Ti, ld, jb, K, lds, y);
    }
    // ---- Y = -[i == j] I - acc  (lane holds m = wm*16 + c, n = j2*16 + irow(g, v)) ---------------------
#pragma unroll
    for (int j2 = 0; j2 < Cfg::TN; ++j2)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int nl = acc_n<Cfg>(j2, g, v);
        const int ml = wm * Cfg::WM + acc_m<Cfg>(0, c);
        y.re[0][j2][v] = ((i == j && ml == nl) ? R(-1) : R(0)) - y.re[0][j2][v];
        if constexpr (Cfg::CX)
          y.im[0][j2][v] = -y.im[0][j2][v];
      }

    // ---- N(j, i) = Y inv(T_ii)^H: the inverted block staged whole into LDS (the K loop is done with it) ----
    const T* Wi = Wt + (long) i * JB * JB;
    constexpr int LDW = JB + kLdsPad;
    constexpr int WPLANE = JB * LDW;
    R* Ws = lds;
    {
      Slab<T, JB, JB, true, LDW> sw;  // dense 64 x 64, 16-byte aligned
      sw.template load<false>(Wi, JB, 0, JB, JB);
      sw.store(Ws);
    }
    __syncthreads();
    T* Nji = Nj + (long) (i * JB) * ld;
#pragma unroll
    for (int jx = 0; jx < Cfg::TN; ++jx) {
      const int j2 = Cfg::TN - 1 - jx;  // inv(T_ii) lower: Y tile ct only feeds N tiles j2 >= ct
      acc_t xre = acc_t{0, 0, 0, 0}, xim = acc_t{0, 0, 0, 0};
#pragma unroll
      for (int ct = 0; ct < Cfg::TN; ++ct) {
        if (ct > j2)
          continue;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int kabs = acc_n<Cfg>(ct, g, v);
          const R w_re = Ws[kabs * LDW + j2 * 16 + c];
          xre = Mma<R>::mma(w_re, y.re[0][ct][v], xre);
          if constexpr (Cfg::CX) {
            const R w_im = Ws[WPLANE + kabs * LDW + j2 * 16 + c];
            // (yr + i yi)(wr - i wi) = (yr wr + yi wi) + i (yi wr - yr wi)
            xre = Mma<R>::mma(w_im, y.im[0][ct][v], xre);
            xim = Mma<R>::mma(w_re, y.im[0][ct][v], xim);
            xim = Mma<R>::mma(-w_im, y.re[0][ct][v], xim);
          }
        }
      }
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int nl = j2 * 16 + Mma<R>::irow(g, v);
        const int ml = wm * Cfg::WM + acc_m<Cfg>(0, c);
        if (ml < mrows && nl < jb) {
          if constexpr (Cfg::CX)
            Nji[ml + (long) nl * ld] = T{xre[v], xim[v]};
          else
            Nji[ml + (long) nl * ld] = xre[v];
        }
      }
    }
    // N(j, i) is read back (through L1/L2) by this workgroup's next K loop, which also refills the LDS
    __syncthreads();
  }
}

// lower(S_t) = lower(Z_t Z_t^H), Z_t upper triangular kb x kb (ld as the tiles); imag(diag) = 0
template <class T, bool VEC>
__global__ __launch_bounds__(kThreads) void tile_lauum_kernel(TileBatch<T> sb, const T* __restrict__ z, long zstride,
                                                              int nblk) {
  using Cfg = typename InvCfg<T>::type;
  using R = real_t<T>;
  constexpr int JB = kDiagBlock;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  R* lds = reinterpret_cast<R*>(lds_raw);

  const int t = blockIdx.z;
  const int i = blockIdx.x, j = blockIdx.y;
  const int kb = batch_extent(sb, t);
  if (i < j || i * JB >= kb)
    return;
  const int ld = sb.ld;
  const T* Z = z + (long) t * zstride;
  T* S = sb.base + (long) t * sb.stride + i * JB + (long) (j * JB) * ld;
  const int mrows = min(JB, kb - i * JB), ncols = min(JB, kb - j * JB);
  const int K = kb - i * JB;
  const T* Zi = Z + i * JB + (long) (i * JB) * ld;
  const T* Zj = Z + j * JB + (long) (i * JB) * ld;
  const bool full = (mrows == JB) && (ncols == JB) && (K % Cfg::BK == 0);
  Acc<Cfg> acc;
  acc.clear();
  if (full)
    gemm_nt_block<Cfg, T, VEC, false>(Zi, ld, mrows, Zj, ld, ncols, K, lds, acc);
  else
    gemm_nt_block<Cfg, T, false, true>(Zi, ld, mrows, Zj, ld, ncols, K, lds, acc);

  const int lane = threadIdx.x & 63, wm = threadIdx.x >> 6;
  const int g = lane >> 4, c = lane & 15;
#pragma unroll
  for (int j2 = 0; j2 < Cfg::TN; ++j2)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int nl = acc_n<Cfg>(j2, g, v);
      const int ml = wm * Cfg::WM + acc_m<Cfg>(0, c);
      if (ml < mrows && nl < ncols && (i > j || ml >= nl)) {
        if constexpr (Cfg::CX)
          S[ml + (long) nl * ld] = T{acc.re[0][j2][v], (i == j && ml == nl) ? R(0) : acc.im[0][j2][v]};
        else
          S[ml + (long) nl * ld] = acc.re[0][j2][v];
      }
    }
}

// mode 0: dst(r, c) = src(r, c) for r > c, and for r == c unless unit -- nothing else of dst is touched
// mode 1: dst = lower(src)^H as a whole tile (zero below the diagonal)
template <class T>
__global__ __launch_bounds__(kThreads) void tri_tile_kernel(TileBatch<T> db, const T* __restrict__ src, long sstride,
                                                            int mode, int unit) {
  const int t = blockIdx.z;
  const int kb = batch_extent(db, t);
  const int ld = db.ld;
  const T* s = src + (long) t * sstride;
  T* d = db.base + (long) t * db.stride;
  const int r = blockIdx.x * 64 + (threadIdx.x & 63);
  const int c0 = blockIdx.y * 64 + (threadIdx.x >> 6) * 16;
  if (r >= kb)
    return;
  for (int c = c0; c < min(c0 + 16, kb); ++c) {
    if (mode == 0) {
      if (r > c || (r == c && !unit))
        d[r + (long) c * ld] = s[r + (long) c * ld];
    }
    else {
      T v = zero_el<T>();
      if (r <= c) {
        v = s[c + (long) r * ld];
        if constexpr (TypeInfo<T>::is_complex)
          v.im = -v.im;
      }
      d[r + (long) c * ld] = v;
    }
  }
}

// *first = min(*first, 1-based global index) over the exactly-zero diagonal elements; tile t holds the global
// elements from (k0 + t * kstep) * nb on
template <class T>
__global__ __launch_bounds__(kThreads) void diag_zero_scan_kernel(TileBatch<const T> tb, long k0, long kstep,
                                                                  unsigned* first) {
  const int t = blockIdx.y;
  const int kb = batch_extent(tb, t);
  const int d = blockIdx.x * kThreads + threadIdx.x;
  if (d >= kb)
    return;
  const T v = tb.base[(long) t * tb.stride + d + (long) d * tb.ld];
  if (re_of(v) == real_t<T>(0) && im_of(v) == real_t<T>(0))
    atomicMin(first, (unsigned) ((k0 + (long) t * kstep) * tb.nb + d + 1));
}

template <class T>
static bool aligned16(const void* ptr, long stride_elems) {
  return (reinterpret_cast<uintptr_t>(ptr) % 16 == 0) && ((stride_elems * (long) sizeof(T)) % 16 == 0);
}

template <class T>
void launch_tile_trtri(const TileBatch<const T>& tiles, const T* winv, long winv_stride, T* nout, long nstride,
                       hipStream_t stream) {
  if (tiles.count <= 0 || tiles.nb <= 0)
    return;
  const int nblk = (tiles.nb + kDiagBlock - 1) / kDiagBlock;
  const bool vec = aligned16<T>(tiles.base, tiles.ld) && aligned16<T>(tiles.base, tiles.stride) &&
                   aligned16<T>(nout, tiles.ld) && aligned16<T>(nout, nstride);
  const dim3 grid((unsigned) (tiles.count * nblk));
  if (vec)
    hipLaunchKernelGGL((tile_trtri_kernel<T, true>), grid, dim3(kThreads), inv_lds_bytes<T>(), stream, tiles, winv,
                       winv_stride, nout, nstride, nblk);
  else
    hipLaunchKernelGGL((tile_trtri_kernel<T, false>), grid, dim3(kThreads), inv_lds_bytes<T>(), stream, tiles, winv,
                       winv_stride, nout, nstride, nblk);
}

template <class T>
void launch_tile_lauum(const TileBatch<T>& tiles, const T* z, long zstride, hipStream_t stream) {
  if (tiles.count <= 0 || tiles.nb <= 0)
    return;
  const int nblk = (tiles.nb + kDiagBlock - 1) / kDiagBlock;
  const bool vec = aligned16<T>(z, tiles.ld) && aligned16<T>(z, zstride);
  const dim3 grid((unsigned) nblk, (unsigned) nblk, (unsigned) tiles.count);
  if (vec)
    hipLaunchKernelGGL((tile_lauum_kernel<T, true>), grid, dim3(kThreads), inv_lds_bytes<T>(), stream, tiles, z, zstride,
                       nblk);
  else
    hipLaunchKernelGGL((tile_lauum_kernel<T, false>), grid, dim3(kThreads), inv_lds_bytes<T>(), stream, tiles, z,
                       zstride, nblk);
}

template <class T>
void launch_tri_tile(const TileBatch<T>& dst, const T* src, long sstride, int mode, bool unit, hipStream_t stream) {
  if (dst.count <= 0 || dst.nb <= 0)
    return;
  const unsigned nblk = (unsigned) ((dst.nb + 63) / 64);
  hipLaunchKernelGGL((tri_tile_kernel<T>), dim3(nblk, nblk, (unsigned) dst.count), dim3(kThreads), 0, stream, dst, src,
                     sstride, mode, unit ? 1 : 0);
}

template <class T>
void launch_diag_zero_scan(const TileBatch<const T>& tiles, long k0, long kstep, unsigned* first, hipStream_t stream) {
  if (tiles.count <= 0 || tiles.nb <= 0)
    return;
  hipLaunchKernelGGL((diag_zero_scan_kernel<T>), dim3((unsigned) ((tiles.nb + kThreads - 1) / kThreads), (unsigned) tiles.count),
                     dim3(kThreads), 0, stream, tiles, k0, kstep, first);
}

template <class T>
static void inverse_init_one() {
#define SET_ONE(K)                                                                              \
  (void) hipFuncSetAttribute(reinterpret_cast<const void*>(&K), hipFuncAttributeMaxDynamicSharedMemorySize, \
                             inv_lds_bytes<T>())
  SET_ONE((tile_trtri_kernel<T, true>) );
  SET_ONE((tile_trtri_kernel<T, false>) );
  SET_ONE((tile_lauum_kernel<T, true>) );
  SET_ONE((tile_lauum_kernel<T, false>) );
#undef SET_ONE
}

void inverse_kernels_init() {
  inverse_init_one<float>();
  inverse_init_one<double>();
  inverse_init_one<cfloat>();
  inverse_init_one<cdouble>();
}

#define INST(T)                                                                                             \
  template void launch_tile_trtri<T>(const TileBatch<const T>&, const T*, long, T*, long, hipStream_t);    \
  template void launch_tile_lauum<T>(const TileBatch<T>&, const T*, long, hipStream_t);                    \
  template void launch_tri_tile<T>(const TileBatch<T>&, const T*, long, int, bool, hipStream_t);           \
  template void launch_diag_zero_scan<T>(const TileBatch<const T>&, long, long, unsigned*, hipStream_t);
INST(float)
INST(double)
INST(cfloat)
INST(cdouble)
#undef INST

}  // namespace dlaf_mi355x
