// kernels_hemm.hip -- one step of the Hermitian multiplication  Y = beta Y + alpha X H  (multiplication.cpp:
// hermitian_canonical), for ALL the local tiles of Y in one launch:
//        Y(il, jl) (+)= alpha X(il, l) H(l, j)          H Hermitian, only its LOWER triangle stored
// A workgroup owns one BM x BN block of one tile of Y and takes its H operand straight from the stored triangle, in
// one of three fetch modes (uniform over the workgroup; j = the global tile column of jl):
//   1  j > l : H(l, j) = H(j, l)^H -- the stored tile is the B^H operand of the NT product: rows contiguous,
//              16-byte loads along the rows into the [k][n] LDS image                       (OpSlab mode 0)
//   2  j = l : the diagonal tile, mirrored from its lower triangle while it is staged into LDS; the diagonal is taken
//              as real and nothing above it is read                                        (OpDesc::herm)
//   3  j < l : H(l, j) is the stored tile itself: a k-contiguous operand.  16-byte loads along k, stored as loaded
//              into the transposed LDS image [n][BK + 2], which the MFMA fragments read with a row stride of
//              BK + 2 words: neither the store nor the read has a bank conflict (OpSlab::store<TIMG>, gemm_general.hpp)
// Whole, aligned blocks take the vector loaders of their mode; ragged last tiles and unaligned tile sizes take the
// bounds-checked element loader.  All types run the MFMA tiles of the general kernels (GenCfg: v_mfma_f64_16x16x4_f64
// for d and z).  The epilogue applies alpha, and beta in the first step only (beta == 0: Y is not read).
#include <type_traits>

#include "device_api.hpp"
#include "gemm_general.hpp"

namespace dlaf_mi355x {

namespace {

template <class T>
__device__ __forceinline__ T hemm_mul(const T& a, const T& b) {
  if constexpr (TypeInfo<T>::is_complex)
    return T{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
  else
    return a * b;
}
template <class T>
__device__ __forceinline__ T hemm_add(const T& a, const T& b) {
  if constexpr (TypeInfo<T>::is_complex)
    return T{a.re + b.re, a.im + b.im};
  else
    return a + b;
}

}  // namespace

// grid: x = (block inside a tile, il, jl), the blocks of a tile next to each other (they share its X and H tiles)
template <class T, bool VEC>
__global__ __launch_bounds__(GenCfg<T>::type::THREADS, 2) void hemm_kernel(HemmArgs<T> p, int bpr, int bpc) {
  using Cfg = typename GenCfg<T>::type;
  using R = real_t<T>;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  R* lds = reinterpret_cast<R*>(lds_raw);

  const int bpt = bpr * bpc;
  const int blk = (int) (blockIdx.x % (unsigned) bpt);
  const int tile = (int) (blockIdx.x / (unsigned) bpt);
  const int il = tile % p.ltr, jl = tile / p.ltr;
  const int bm = blk % bpr, bn = blk / bpr;
  const int gi = il * p.pr + p.ri, gj = jl * p.pc + p.ci;
  const int rows_tile = (gi == p.nt_r - 1) ? p.last_rows : p.nb;
  const int cols_tile = (gj == p.nt_c - 1) ? p.last_cols : p.nb;
  const int m0 = bm * Cfg::BM, n0 = bn * Cfg::BN;
  if (m0 >= rows_tile || n0 >= cols_tile)
    return;
  const int mrows = min(Cfg::BM, rows_tile - m0), ncols = min(Cfg::BN, cols_tile - n0);
  const int K = p.K;
  const bool whole = VEC && mrows == Cfg::BM && ncols == Cfg::BN && K % Cfg::BK == 0;

  OpDesc<T> da, db;
  da.p = p.x + (long) il * p.x_ts + m0;
  da.rs = 1;
  da.ks = p.nb;
  Acc<Cfg> acc;
  acc.clear();
  if (gj > p.l) {
    // b(n, k) = S(j, l)(n0 + n, k)
    db.p = p.hc + (long) (jl - p.jc0) * p.hc_ts + n0;
    db.rs = 1;
    db.ks = p.nb;
    db.conj = p.conj_h;
    if (whole)
      gemm_acc<Cfg, T, 0, 0>(da, mrows, db, ncols, K, lds, acc);
    else
      gemm_acc<Cfg, T, 2, 2>(da, mrows, db, ncols, K, lds, acc);
  }
  else if (gj < p.l) {
    // b(n, k) = conj(S(l, j)(k, n0 + n))
    db.p = p.hr + (long) jl * p.hr_ts + (long) n0 * p.nb;
    db.rs = p.nb;
    db.ks = 1;
    db.conj = p.conj_h ? 0 : 1;
    if (whole)
      gemm_acc<Cfg, T, 0, 1>(da, mrows, db, ncols, K, lds, acc);
    else
      gemm_acc<Cfg, T, 2, 2>(da, mrows, db, ncols, K, lds, acc);
  }
  else {
    // b(n, k) = the Hermitian image of the diagonal tile's lower triangle at (n0 + n, k)
    db.p = p.hd;
    db.rs = 1;
    db.ks = p.nb;
    db.herm = 1;
    db.roff = n0;
    db.conj = p.conj_h;
    if (whole)
      gemm_acc<Cfg, T, 0, 2>(da, mrows, db, ncols, K, lds, acc);
    else
      gemm_acc<Cfg, T, 2, 2>(da, mrows, db, ncols, K, lds, acc);
  }

  T* yt = p.y + (long) il * p.y_tsr + (long) jl * p.y_tsc + m0 + (long) n0 * p.nb;
  const bool read_y = !p.first || re_of(p.beta) != R(0) || im_of(p.beta) != R(0);
  const T one = make_el<T>(R(1), R(0));
  const T by = p.first ? p.beta : one;
  acc_foreach<Cfg, T>(acc, [&](int m, int n, const T& v) {
    if (m < mrows && n < ncols) {
      T* y = yt + m + (long) n * p.nb;
      T r = hemm_mul(p.alpha, v);
      if (read_y)
        r = hemm_add(r, hemm_mul(by, *y));
      *y = r;
    }
  });
}

template <class T>
void launch_hemm(const HemmArgs<T>& a, hipStream_t stream) {
  using Cfg = typename GenCfg<T>::type;
  if (a.ltr <= 0 || a.ltc <= 0 || a.nb <= 0 || a.K <= 0)
    return;
  auto al16 = [](const void* ptr) { return ptr == nullptr || reinterpret_cast<uintptr_t>(ptr) % 16 == 0; };
  auto st16 = [](long elems) { return (elems * (long) sizeof(T)) % 16 == 0; };
  // every tile origin and every column of a tile on a 16-byte boundary
  const bool vec = al16(a.y) && al16(a.x) && al16(a.hc) && al16(a.hd) && al16(a.hr) && st16(a.nb) && st16(a.x_ts) &&
                   st16(a.hc_ts) && st16(a.hr_ts);
  const int bpr = (a.nb + Cfg::BM - 1) / Cfg::BM, bpc = (a.nb + Cfg::BN - 1) / Cfg::BN;
  const long grid = (long) a.ltr * a.ltc * bpr * bpc;
  if (vec)
    hipLaunchKernelGGL((hemm_kernel<T, true>), dim3((unsigned) grid), dim3(Cfg::THREADS), Cfg::LDS_BYTES, stream, a, bpr,
                       bpc);
  else
    hipLaunchKernelGGL((hemm_kernel<T, false>), dim3((unsigned) grid), dim3(Cfg::THREADS), Cfg::LDS_BYTES, stream, a,
                       bpr, bpc);
}

template <class T>
static void hemm_init_one() {
  using Cfg = typename GenCfg<T>::type;
  (void) hipFuncSetAttribute(reinterpret_cast<const void*>(&hemm_kernel<T, true>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::LDS_BYTES);
  (void) hipFuncSetAttribute(reinterpret_cast<const void*>(&hemm_kernel<T, false>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::LDS_BYTES);
}

void hemm_kernels_init() {
  hemm_init_one<float>();
  hemm_init_one<double>();
  hemm_init_one<cfloat>();
  hemm_init_one<cdouble>();
}

template void launch_hemm<float>(const HemmArgs<float>&, hipStream_t);
template void launch_hemm<double>(const HemmArgs<double>&, hipStream_t);
template void launch_hemm<cfloat>(const HemmArgs<cfloat>&, hipStream_t);
template void launch_hemm<cdouble>(const HemmArgs<cdouble>&, hipStream_t);

}  // namespace dlaf_mi355x
