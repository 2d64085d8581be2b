// kernels_trmm.hip -- panel TRMM  X = B * L^H  in place, for all the local tiles of one tile column in ONE
// launch (the diagonal-tile step of triangular_multiplication, multiplication.cpp).
//
// X(:, c) = sum_{k <= c} B(:, k) conj(L(c, k))  (lower L; k >= c for upper): no chain and no inverse.  Each
// workgroup owns a 128-row strip of one tile and produces its 64-column output blocks right to left (lower) /
// left to right (upper), so that a block is overwritten only after every block that reads it is done.  Block c:
//     acc  = B(:, off-diagonal columns) L(c, off-diagonal columns)^H       (MFMA GEMM of mma_core.hpp)
//     acc += B(:, c) tri(L_cc)^H                                            (same MFMAs, L_cc masked in LDS)
//     B(:, c) = acc
// Only the triangle of L is read; with `unit` its diagonal is taken as 1 and not read.  The strips never exchange
// data: no inter-workgroup synchronisation.  fp64: the strips take the paired-row, direct-to-LDS, 3-stage block
// configuration of the update kernel's fast path (v_mfma_f64_16x16x4f64, L slabs staged global -> LDS by
// global_load_lds) for the off-diagonal GEMM of whole 128-row strips; edges take the register-staged path.
#include <type_traits>

#include "device_api.hpp"
#include "mma_core.hpp"

namespace dlaf_mi355x {

// One wave per SIMD: a launch covers one tile column (m / 128 strips), far fewer workgroups than the GPU holds at
// two, and the GEMM accumulators plus the edge path's register staging do not fit in half the register file.
template <class T>
struct TrmmCfg {
  using type = BlockCfg<T, 128, kDiagBlock, 32, kDiagBlock, 16>;
  static constexpr int min_waves = 1;
};
template <>
struct TrmmCfg<double> {
  using type = BlockCfg<double, 128, kDiagBlock, 32, kDiagBlock, 16, true, 3>;
  static constexpr int min_waves = 1;
};
template <>
struct TrmmCfg<cdouble> {
  using type = BlockCfg<cdouble, 128, kDiagBlock, 32, kDiagBlock, 8>;
  static constexpr int min_waves = 1;
};

// element (r, k) of an LDS slab image [k][ld] (planes re | im, or interleaved (re, im) for CXI)
template <class Cfg, class T>
__device__ __forceinline__ void lds_put(typename Cfg::R* img, int ld, int plane, int r, int k, const T& v) {
  if constexpr (Cfg::CXI) {
    img[2 * (k * ld + r)] = re_of(v);
    img[2 * (k * ld + r) + 1] = im_of(v);
  }
  else {
    img[k * ld + r] = re_of(v);
    if constexpr (Cfg::CX)
      img[plane + k * ld + r] = im_of(v);
  }
}

template <class T, bool VEC, bool UPPER>
__global__ __launch_bounds__(kThreads, TrmmCfg<T>::min_waves) void trmm_kernel(TrmmArgs<T> p, int spt) {
  using Cfg = typename TrmmCfg<T>::type;
  using R = real_t<T>;
  constexpr int JB = kDiagBlock;
  static_assert(Cfg::BN == JB && Cfg::WAVES_N == 1 && JB % Cfg::BK == 0, "a wave owns whole rows of a 64-column block");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  R* lds = reinterpret_cast<R*>(lds_raw);

  const int il = p.il0 + blockIdx.x / spt;
  const int s = blockIdx.x % spt;
  const int gi = il * p.pr + p.ri;
  const int rows_tile = (gi == p.nt - 1) ? p.last_rows : p.nb;
  const int m0 = s * Cfg::BM;
  if (m0 >= rows_tile)
    return;
  const int mrows = min(Cfg::BM, rows_tile - m0);
  T* Bst = p.b + (long) (il - p.il0) * p.b_ts + m0;

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave;  // WAVES_M == 4, WAVES_N == 1
  const int g = lane >> 4, c = lane & 15;
  const int njb = (p.n + JB - 1) / JB;

  for (int jj = 0; jj < njb; ++jj) {
    const int j = UPPER ? jj : njb - 1 - jj;
    const int jb = min(JB, p.n - j * JB);
    // off-diagonal columns of output block j: [0, j JB) for lower L, [(j+1) JB, n) for upper
    const int k0 = UPPER ? (j + 1) * JB : 0;
    const int K = UPPER ? max(0, p.n - k0) : j * JB;
    const bool full = (mrows == Cfg::BM) && (jb == JB) && (K % Cfg::BK == 0);
    Acc<Cfg> acc;
    acc.clear();
    if (K > 0) {
      const T* Bs = Bst + (long) k0 * p.ldb;
      const T* Lj = p.l + j * JB + (long) k0 * p.ldl;
      if (full)
        gemm_nt_block<Cfg, T, VEC, false>(Bs, p.ldb, mrows, Lj, p.ldl, jb, K, lds, acc);
      else
        gemm_nt_block<Cfg, T, false, true>(Bs, p.ldb, mrows, Lj, p.ldl, jb, K, lds, acc);
    }

    // ---- diagonal block: acc += B_j tri(L_jj)^H, BK columns at a time through one LDS slab buffer ------------
    T* Bj = Bst + (long) (j * JB) * p.ldb;
    const T* Ljj = p.l + j * JB + (long) (j * JB) * p.ldl;
    R* As = lds;
    R* Ws = lds + Cfg::A_ELEMS;
    for (int k1 = 0; k1 < jb; k1 += Cfg::BK) {
      __syncthreads();  // nobody reads the slab buffer any more
      for (int e = threadIdx.x; e < Cfg::BM * Cfg::BK; e += Cfg::THREADS) {
        const int r = e % Cfg::BM, kk = e / Cfg::BM;
        T v = zero_el<T>();
        if (r < mrows && k1 + kk < jb)
          v = Bj[r + (long) (k1 + kk) * p.ldb];
        lds_put<Cfg>(As, Cfg::LDA, Cfg::A_PLANE, r, kk, v);
      }
      for (int e = threadIdx.x; e < JB * Cfg::BK; e += Cfg::THREADS) {
        const int r = e % JB, kk = e / JB, k = k1 + kk;  // W(r, k) = L_jj(r, k) inside the triangle, else 0
        T v = zero_el<T>();
        if (r < jb && k < jb) {
          if (r == k)
            v = p.unit ? make_el<T>(R(1), R(0)) : Ljj[r + (long) k * p.ldl];
          else if (UPPER ? (r < k) : (r > k))
            v = Ljj[r + (long) k * p.ldl];
        }
        lds_put<Cfg>(Ws, Cfg::LDB, Cfg::B_PLANE, r, kk, v);
      }
      __syncthreads();
      mma_slab<Cfg>(As, Ws, acc, wm, 0, lane);
    }

    // ---- B_j = acc (every wave has staged its last read of B_j before the barrier above) ----------------------
#pragma unroll
    for (int j2 = 0; j2 < Cfg::TN; ++j2)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int nl = acc_n<Cfg>(j2, g, v);
#pragma unroll
        for (int i = 0; i < Cfg::TM; ++i) {
          const int ml = wm * Cfg::WM + acc_m<Cfg>(i, c);
          if (full || (ml < mrows && nl < jb)) {
            if constexpr (Cfg::CX)
              Bj[ml + (long) nl * p.ldb] = T{acc.re[i][j2][v], acc.im[i][j2][v]};
            else
              Bj[ml + (long) nl * p.ldb] = acc.re[i][j2][v];
          }
        }
      }
    // the next block's GEMM refills the LDS the last slab is still being read from
    __syncthreads();
  }
}

template <class T>
static bool aligned16(const void* ptr, long stride_elems) {
  return (reinterpret_cast<uintptr_t>(ptr) % 16 == 0) && ((stride_elems * (long) sizeof(T)) % 16 == 0);
}

template <class T>
void launch_trmm(const TrmmArgs<T>& a, hipStream_t stream) {
  using Cfg = typename TrmmCfg<T>::type;
  if (a.il1 <= a.il0 || a.n <= 0 || a.nb <= 0)
    return;
  const bool vec = aligned16<T>(a.b, a.ldb) && aligned16<T>(a.b, a.b_ts) && aligned16<T>(a.l, a.ldl);
  const int spt = (a.nb + Cfg::BM - 1) / Cfg::BM;
  const long grid = (long) (a.il1 - a.il0) * spt;
  auto go = [&](auto vtag, auto utag) {
    hipLaunchKernelGGL((trmm_kernel<T, decltype(vtag)::value, decltype(utag)::value>), dim3((unsigned) grid),
                       dim3(kThreads), Cfg::LDS_BYTES, stream, a, spt);
  };
  if (a.upper)
    vec ? go(std::true_type{}, std::true_type{}) : go(std::false_type{}, std::true_type{});
  else
    vec ? go(std::true_type{}, std::false_type{}) : go(std::false_type{}, std::false_type{});
}

template <class T>
static void trmm_init_one() {
  using Cfg = typename TrmmCfg<T>::type;
#define SET_ONE(V, U)                                                                      \
  (void) hipFuncSetAttribute(reinterpret_cast<const void*>(&trmm_kernel<T, V, U>),          \
                             hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::LDS_BYTES)
  SET_ONE(true, false);
  SET_ONE(false, false);
  SET_ONE(true, true);
  SET_ONE(false, true);
#undef SET_ONE
}

void trmm_kernels_init() {
  trmm_init_one<float>();
  trmm_init_one<double>();
  trmm_init_one<cfloat>();
  trmm_init_one<cdouble>();
}

template void launch_trmm<float>(const TrmmArgs<float>&, hipStream_t);
template void launch_trmm<double>(const TrmmArgs<double>&, hipStream_t);
template void launch_trmm<cfloat>(const TrmmArgs<cfloat>&, hipStream_t);
template void launch_trmm<cdouble>(const TrmmArgs<cdouble>&, hipStream_t);

}  // namespace dlaf_mi355x
