// kernels_gemm.hip -- the general multiplication  C = beta C + alpha op(A) op(B)  (multiplication.cpp:
// general_canonical), for ALL the local tiles of C in one launch:
//        C(il, jl) = [first ? beta : 1] C(il, jl) + alpha sum_{t < nk} opA(A)(il, t) opB(B)(t, jl)
// A workgroup owns one BM x BN block of one tile of C and keeps it in its MFMA accumulators over all nk tiles of the
// k dimension: one gemm_acc per k tile into the same Acc, one epilogue, C read (at most) once and written once.
// Both operands are read as stored, whatever the ops (gemm_forms.hpp has the mapping): a stored m x k / n x k tile is
// staged along its contiguous rows (OpSlab mode 0), a stored k x m / k x n tile along its contiguous k (mode 1) into
// the transposed LDS image [row][BK + 2] the MFMA fragments read with a row stride (gemm_general.hpp: OpSlab::store<TIMG>)
// -- on the A side too.  A kernel has ONE loader pair, fixed at compile time, for the forms (MA, MB) of its op pair:
// VEC, their vector loaders, or the bounds-checked element loader for the blocks that are ragged or unaligned and for
// a k whose last tile is no whole number of BK slabs; a launch issues both over the same grid (see the k loop).  The
// epilogue applies alpha, and beta in the first launch only (beta == 0: C is not read); nk == 0 is an epilogue-only
// launch (C = beta C, or zero).
#include <type_traits>

#include "device_api.hpp"
#include "gemm_forms.hpp"
#include "gemm_general.hpp"

namespace dlaf_mi355x {

namespace {

template <class T>
__device__ __forceinline__ T gemm_mul(const T& a, const T& b) {
  if constexpr (TypeInfo<T>::is_complex)
    return T{a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
  else
    return a * b;
}
template <class T>
__device__ __forceinline__ T gemm_add(const T& a, const T& b) {
  if constexpr (TypeInfo<T>::is_complex)
    return T{a.re + b.re, a.im + b.im};
  else
    return a + b;
}

template <class T>
__device__ __forceinline__ OpDesc<T> op_desc(const GemmForm& f, const T* tile) {
  OpDesc<T> d;
  d.p = tile + f.off;
  d.rs = f.rs;
  d.ks = f.ks;
  d.conj = f.conj;
  return d;
}

// acc_foreach (gemm_general.hpp) from a thread index the compiler cannot tie to the one gemm_acc used: in the vector
// kernels it would keep the wave's row offset from before the k loop for the epilogue, one register too many in the d
// and c kernels (the element kernel is the other way round: it spills with this and not with acc_foreach)
template <class Cfg, class T, class F>
__device__ __forceinline__ void acc_foreach_fresh(const Acc<Cfg>& acc, F&& f) {
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave % Cfg::WAVES_M, wn = wave / Cfg::WAVES_M;
  const int g = lane >> 4, c = lane & 15;
#pragma unroll
  for (int j = 0; j < Cfg::TN; ++j)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int n = wn * Cfg::WN + acc_n<Cfg>(j, g, v);
#pragma unroll
      for (int i = 0; i < Cfg::TM; ++i) {
        const int m = wm * Cfg::WM + acc_m<Cfg>(i, c);
        if constexpr (Cfg::CX)
          f(m, n, T{acc.re[i][j][v], acc.im[i][j][v]});
        else
          f(m, n, acc.re[i][j][v]);
      }
    }
}

}  // namespace

// grid: x = (block inside a tile, il, jl), the blocks of a tile next to each other (they share its A and B tiles)
// Workgroups per compute unit the kernels are compiled for: two, except the fp64 element kernel.  Held to 256 registers
// its allocator spills 32 bytes per lane around the loops over the k tiles; free, it takes 150 + 128 accumulator
// registers, no scratch, and runs at one workgroup per compute unit.  (The other element kernels fit: 181 (s), 252 (c),
// 234 (z) registers.)
template <class T, bool VEC>
constexpr int kGemmMinBlocks = (!VEC && std::is_same<T, double>::value) ? 1 : 2;

template <class T, int MA, int MB, bool VEC>
__global__ __launch_bounds__(GenCfg<T>::type::THREADS, (kGemmMinBlocks<T, VEC>) ) void general_kernel(GeneralArgs<T> p,
                                                                                                      int bpr, int bpc) {
  using Cfg = typename GenCfg<T>::type;
  using R = real_t<T>;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  R* lds = reinterpret_cast<R*>(lds_raw);

  const int bpt = bpr * bpc;
  const int blk = (int) (blockIdx.x % (unsigned) bpt);
  const int tile = (int) (blockIdx.x / (unsigned) bpt);
  // (hipcc divides on the vector unit: without the readfirstlane every tile address and extent below -- uniform
  // values -- would sit in vector registers beside the accumulators)
  const int il = __builtin_amdgcn_readfirstlane(tile % p.ltr), jl = __builtin_amdgcn_readfirstlane(tile / p.ltr);
  const int bm = __builtin_amdgcn_readfirstlane(blk % bpr), bn = __builtin_amdgcn_readfirstlane(blk / bpr);
  const int gi = il * p.pr + p.ri, gj = jl * p.pc + p.ci;
  const int rows_tile = (gi == p.nt_r - 1) ? p.last_rows : p.nb;
  const int cols_tile = (gj == p.nt_c - 1) ? p.last_cols : p.nb;
  const int m0 = bm * Cfg::BM, n0 = bn * Cfg::BN;
  if (m0 >= rows_tile || n0 >= cols_tile)
    return;
  const int mrows = min(Cfg::BM, rows_tile - m0), ncols = min(Cfg::BN, cols_tile - n0);

  const GemmForm fa = gemm_form_a(p.opa, p.nb, m0), fb = gemm_form_b(p.opb, p.nb, n0);
  const T* at = p.a + (long) il * p.a_ts;
  const T* bt = p.b + (long) jl * p.b_ts;
  T* ct = p.c + (long) il * p.c_tsr + (long) jl * p.c_tsc + m0 + (long) n0 * p.nb;
  Acc<Cfg> acc;
  acc.clear();
  // One loader pair per kernel: VEC, the vector loaders of the forms (MA, MB) for the blocks whose every k tile
  // qualifies (the tiles before the last all have nb values of k and the alignment of the first two, whose addresses
  // differ by the tile stride; the last has k_last); else the element loader for all the other blocks.  launch_general
  // issues both kernels over the same grid and each block runs in exactly one of them.  Both loaders in one kernel --
  // chosen per k tile, or per block around two loops -- cost a copy of the accumulators where the paths join: 80 to
  // 1100 bytes of scratch per lane in the d, c and z kernels.
  auto vec_ok = [&](int t, int K) {
    return gemm_loader_mode<(int) sizeof(T)>(fa, at + (long) t * p.a_ks, p.nb, mrows, Cfg::BM, K, Cfg::BK) != 2 &&
           gemm_loader_mode<(int) sizeof(T)>(fb, bt + (long) t * p.b_ks, p.nb, ncols, Cfg::BN, K, Cfg::BK) != 2;
  };
  const bool vec = p.nk > 0 && vec_ok(p.nk - 1, p.k_last) && (p.nk < 2 || vec_ok(0, p.nb)) && (p.nk < 3 || vec_ok(1, p.nb));
  if (vec != VEC)
    return;
  // (whole blocks in the vector kernel: its row tests fold away)
  const int mr = VEC ? Cfg::BM : mrows, nc = VEC ? Cfg::BN : ncols;
  for (int t = 0; t < p.nk; ++t) {
    OpDesc<T> da = op_desc(fa, at + (long) t * p.a_ks), db = op_desc(fb, bt + (long) t * p.b_ks);
    // The strides do not change from one k tile to the next, and hipcc would compute every lane's slab offsets once,
    // ahead of this loop, and keep them in registers beside the accumulators over all of it: spills.  Opaque per
    // k tile, they are recomputed in gemm_acc's prologue as in a single-tile kernel.
    asm volatile("" : "+s"(da.rs), "+s"(da.ks), "+s"(db.rs), "+s"(db.ks));
    const int K = t == p.nk - 1 ? p.k_last : p.nb;
    if constexpr (VEC)
      gemm_acc<Cfg, T, MA, MB>(da, mr, db, nc, K, lds, acc);
    else
      gemm_acc<Cfg, T, 2, 2>(da, mr, db, nc, K, lds, acc);
  }

  const bool read_c = !p.first || re_of(p.beta) != R(0) || im_of(p.beta) != R(0);
  const bool product = p.nk > 0;
  const T bc = p.first ? p.beta : make_el<T>(R(1), R(0));
  auto store = [&](int m, int n, const T& v) {
    if (m < mr && n < nc) {
      T* c = ct + m + (long) n * p.nb;
      T r = product ? gemm_mul(p.alpha, v) : zero_el<T>();
      if (read_c)
        r = gemm_add(r, gemm_mul(bc, *c));
      *c = r;
    }
  };
  if constexpr (VEC)
    acc_foreach_fresh<Cfg, T>(acc, store);
  else
    acc_foreach<Cfg, T>(acc, store);
}

template <class T, int MA, int MB, bool VEC>
static void launch_gemm_kernel(const GeneralArgs<T>& a, hipStream_t stream) {
  using Cfg = typename GenCfg<T>::type;
  const int bpr = (a.nb + Cfg::BM - 1) / Cfg::BM, bpc = (a.nb + Cfg::BN - 1) / Cfg::BN;
  const long grid = (long) a.ltr * a.ltc * bpr * bpc;
  hipLaunchKernelGGL((general_kernel<T, MA, MB, VEC>), dim3((unsigned) grid), dim3(Cfg::THREADS), Cfg::LDS_BYTES, stream, a,
                     bpr, bpc);
}

template <class T, int MA, int MB>
static void launch_gemm_form(const GeneralArgs<T>& a, hipStream_t stream) {
  using Cfg = typename GenCfg<T>::type;
  // (no block can qualify for the vector kernel when the last k tile is not a whole number of slabs)
  if (a.nk > 0 && a.k_last % Cfg::BK == 0)
    launch_gemm_kernel<T, MA, MB, true>(a, stream);
  launch_gemm_kernel<T, 0, 0, false>(a, stream);  // (one element kernel per type: the forms do not enter it)
}

template <class T>
void launch_general(const GeneralArgs<T>& a, hipStream_t stream) {
  if (a.ltr <= 0 || a.ltc <= 0 || a.nb <= 0 || a.nk < 0)
    return;
  const bool an = gemm_op_is_n(a.opa), bn = gemm_op_is_n(a.opb);
  if (an && bn)
    launch_gemm_form<T, 0, 1>(a, stream);
  else if (an)
    launch_gemm_form<T, 0, 0>(a, stream);
  else if (bn)
    launch_gemm_form<T, 1, 1>(a, stream);
  else
    launch_gemm_form<T, 1, 0>(a, stream);
}

template <class T, int MA, int MB>
static void gemm_init_form() {
  using Cfg = typename GenCfg<T>::type;
  (void) hipFuncSetAttribute(reinterpret_cast<const void*>(&general_kernel<T, MA, MB, true>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::LDS_BYTES);
}
template <class T>
static void gemm_init_one() {
  gemm_init_form<T, 0, 0>();
  gemm_init_form<T, 0, 1>();
  gemm_init_form<T, 1, 0>();
  gemm_init_form<T, 1, 1>();
  (void) hipFuncSetAttribute(reinterpret_cast<const void*>(&general_kernel<T, 0, 0, false>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, GenCfg<T>::type::LDS_BYTES);
}

void gemm_kernels_init() {
  gemm_init_one<float>();
  gemm_init_one<double>();
  gemm_init_one<cfloat>();
  gemm_init_one<cdouble>();
}

template void launch_general<float>(const GeneralArgs<float>&, hipStream_t);
template void launch_general<double>(const GeneralArgs<double>&, hipStream_t);
template void launch_general<cfloat>(const GeneralArgs<cfloat>&, hipStream_t);
template void launch_general<cdouble>(const GeneralArgs<cdouble>&, hipStream_t);

}  // namespace dlaf_mi355x
