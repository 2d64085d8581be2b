// kernels_herk.hip -- the Hermitian rank-k and rank-2k updates (rank_update.cpp: rank_update_canonical) of the local
// tiles of the LOWER triangle of a view V in one launch:
//   herk  : V(il, jl) = [first ? beta : 1] V(il, jl) + alpha sum_{t < nk} x(il, t) y(jl, t)^H
//   her2k : ... + alpha sum_t x(il, t) y2(jl, t)^H + conj(alpha) sum_t x2(il, t) y(jl, t)^H
// A workgroup owns one BM x BN block of one tile and keeps it in its MFMA accumulators over all nk tiles of the k
// dimension, as the general multiplication does (kernels_gemm.hip): one gemm_acc per product and k tile into the same
// Acc, one epilogue, V read (at most) once and written once.  herk_map.hpp decides which blocks run (the tiles on and
// below the diagonal; in a diagonal tile the blocks that reach the triangle), which elements the epilogue stores (global
// row >= column) and which of them are diagonal (imaginary part ignored on entry, stored as 0), and maps trans onto the
// operand forms of gemm_forms.hpp: trans N reads two stored nb x K tiles along their rows (OpSlab mode 0), trans C two
// stored K x nb tiles along k (mode 1, the transposed LDS image).
// As in the general kernel a kernel has ONE loader pair fixed at compile time: VEC, the vector loaders of its trans, or
// the bounds-checked element loader; a launch issues both over the same grid and a block leaves at once from the one
// that is not its own.
// her2k adds two products into the same accumulators.  With a complex alpha they carry different scalars and there is
// no room for a second set of accumulators, so the workgroup makes two passes over k:  V = beta V + alpha acc, clear,
// V += conj(alpha) acc -- the block's extra read and write of V is a 1 / k share of the operand traffic.  Real types
// and Im alpha == 0 take one pass with both products per k tile.
// The weighted update (herk only: V += alpha sum_t x(il, t) D_t y(jl, t)^H, D real diagonal) is the same kernel with WT:
// SlabWeights multiplies the weights into the x slab between its global load and its LDS image (gemm_acc's XW hook).
#include <type_traits>

#include "device_api.hpp"
#include "gemm_general.hpp"
#include "herk_map.hpp"

namespace dlaf_mi355x {

namespace {

template <class T>
__device__ __forceinline__ OpDesc<T> herk_desc(const GemmForm& f, const T* tile) {
  OpDesc<T> d;
  d.p = tile + f.off;
  d.rs = f.rs;
  d.ks = f.ks;
  d.conj = f.conj;
  return d;
}

// acc_foreach (gemm_general.hpp) from a thread index the compiler cannot tie to the one gemm_acc used (see
// kernels_gemm.hip: acc_foreach_fresh)
template <class Cfg, class T, class F>
__device__ __forceinline__ void herk_acc_foreach(const Acc<Cfg>& acc, F&& f) {
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

// The weights of the weighted update for the x slab of one k tile (gemm_acc's XW, gemm_general.hpp): kw points to the
// weight of k = 0 of the tile.  fetch reads the weights of the slab at k0 this thread's registers need next to the slab's
// own global loads, scale multiplies them in just before the registers go to LDS -- both parts of a complex element;
// which weight a register takes is herk_map.hpp's.  Mode 2 reads no weight at or beyond K (the element is zero there).
template <class T, class Cfg>
struct SlabWeights {
  using R = real_t<T>;
  using S = OpSlab<T, Cfg::BM, Cfg::BK, Cfg::LDA, Cfg::THREADS>;
  static constexpr int NMAX = S::PER;  // (mode 2; the slots beyond a mode's own count are never touched)
  // LATE: the complex ELEMENT kernels have no registers to carry the weights over a slab of MFMAs (holding them cost
  // complex float 80 and complex double 12 bytes of scratch per lane): their mode 2 notes the slab in fetch and reads the
  // weights in scale, where they live for one multiply each
  static constexpr bool LATE = TypeInfo<T>::is_complex;
  const R* kw;
  R w[NMAX];
  int k0_late = 0, K_late = 0;

  __device__ __forceinline__ void read(int mode, int k0, int K) {
    const int t = threadIdx.x;
#pragma unroll
    for (int s = 0; s < NMAX; ++s)
      if (s < herk_weight_slots(mode, Cfg::BM, Cfg::BK, S::VE, Cfg::THREADS)) {
        const int k = k0 + herk_weight_k(mode, t, s, Cfg::BM, Cfg::BK, S::VE, Cfg::THREADS);
        w[s] = (mode != 2 || k < K) ? kw[k] : R(0);
      }
  }
  __device__ __forceinline__ void fetch(int mode, int k0, int K) {
    if (LATE && mode == 2) {
      k0_late = k0;
      K_late = K;
    }
    else
      read(mode, k0, K);
  }
  __device__ __forceinline__ void scale(int mode, T (&regs)[S::PER]) {
    if (LATE && mode == 2)
      read(mode, k0_late, K_late);
#pragma unroll
    for (int r = 0; r < S::PER; ++r) {
      const R v = w[herk_weight_slot(mode, r, S::VE)];
      if constexpr (TypeInfo<T>::is_complex)
        regs[r] = T{regs[r].re * v, regs[r].im * v};
      else
        regs[r] = regs[r] * v;
    }
  }
};

}  // namespace

// Workgroups per compute unit, as for the general kernels: two, except the fp64 element kernel (kernels_gemm.hip).
template <class T, bool VEC>
constexpr int kHerkMinBlocks = (!VEC && std::is_same<T, double>::value) ? 1 : 2;

// MODE: the OpSlab mode of both operands (0 trans N, 1 trans C); the element kernel (VEC false) serves both.
// WT: the weighted update -- x(il, t)[:, k] is multiplied by the real p.kw[t nb + k] on its way into LDS (herk only)
template <class T, int MODE, bool VEC, bool WT = false>
__global__ __launch_bounds__(GenCfg<T>::type::THREADS, (kHerkMinBlocks<T, VEC>) ) void rank_k_kernel(RankKArgs<T> p, int bpr,
                                                                                                   int bpc) {
  using Cfg = typename GenCfg<T>::type;
  using R = real_t<T>;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  R* lds = reinterpret_cast<R*>(lds_raw);

  const int bpt = bpr * bpc;
  const int blk = (int) (blockIdx.x % (unsigned) bpt);
  const int tile = (int) (blockIdx.x / (unsigned) bpt);
  const int il = __builtin_amdgcn_readfirstlane(tile % p.ltr), jl = __builtin_amdgcn_readfirstlane(tile / p.ltr);
  const int bm = __builtin_amdgcn_readfirstlane(blk % bpr), bn = __builtin_amdgcn_readfirstlane(blk / bpr);
  const int gi = il * p.pr + p.ri, gj = jl * p.pc + p.ci;
  if (!herk_tile_runs(gi, gj))
    return;
  const int rows_tile = (gi == p.nt - 1) ? p.last : p.nb;
  const int cols_tile = (gj == p.nt - 1) ? p.last : p.nb;
  const int m0 = bm * Cfg::BM, n0 = bn * Cfg::BN;
  if (m0 >= rows_tile || n0 >= cols_tile)
    return;
  const int mrows = min(Cfg::BM, rows_tile - m0), ncols = min(Cfg::BN, cols_tile - n0);
  if (!herk_block_runs(gi, gj, m0, mrows, n0, ncols))
    return;

  const GemmForm fx = herk_form_x(p.trans, p.conj_view, p.nb, m0), fy = herk_form_y(p.trans, p.conj_view, p.nb, n0);
  const long xo = herk_panel_offset(il, p.x_period, p.x_ts, p.x_ts2), yo = herk_panel_offset(jl, p.y_period, p.y_ts, p.y_ts2);
  const bool two = p.x2 != nullptr;
  // One loader pair per kernel (kernels_gemm.hip): the vector loaders when every k tile of every operand qualifies
  auto vec_ok1 = [&](const T* x, const T* y, int t, int K) {
    return gemm_loader_mode<(int) sizeof(T)>(fx, x + xo + (long) t * p.ks, p.nb, mrows, Cfg::BM, K, Cfg::BK) != 2 &&
           gemm_loader_mode<(int) sizeof(T)>(fy, y + yo + (long) t * p.ks, p.nb, ncols, Cfg::BN, K, Cfg::BK) != 2;
  };
  auto vec_ok = [&](int t, int K) { return vec_ok1(p.x, p.y, t, K) && (!two || vec_ok1(p.x2, p.y2, t, K)); };
  const bool vec = p.nk > 0 && vec_ok(p.nk - 1, p.k_last) && (p.nk < 2 || vec_ok(0, p.nb)) && (p.nk < 3 || vec_ok(1, p.nb));
  if (vec != VEC)
    return;
  const int mr = VEC ? Cfg::BM : mrows, nc = VEC ? Cfg::BN : ncols;

  // her2k: product 0 is x y2^H (scalar alpha), product 1 is x2 y^H (scalar conj(alpha)); one pass holds both when the
  // scalars agree, else a pass each
  const bool two_pass = two && im_of(p.alpha) != R(0);
  const int npass = two_pass ? 2 : 1;
  T* ct = p.c + (long) il * p.c_tsr + (long) jl * p.c_tsc + m0 + (long) n0 * p.nb;
  const bool diag_tile = gi == gj;

  for (int pass = 0; pass < npass; ++pass) {
    Acc<Cfg> acc;
    acc.clear();
    const int h0 = two_pass ? pass : 0, h1 = two_pass ? pass + 1 : (two ? 2 : 1);
    // (one loop over the (k tile, product) pairs: a loop over the products inside the one over the k tiles spills)
    const int nh = h1 - h0;
    for (int s = 0; s < p.nk * nh; ++s) {
      const int t = nh == 2 ? s >> 1 : s, h = h0 + (nh == 2 ? s & 1 : 0);
      const int K = t == p.nk - 1 ? p.k_last : p.nb;
      const T* xb = (h == 1) ? p.x2 : p.x;
      const T* yb = (two && h == 0) ? p.y2 : p.y;
      OpDesc<T> dx = herk_desc(fx, xb + xo + (long) t * p.ks), dy = herk_desc(fy, yb + yo + (long) t * p.ks);
      // (opaque per k tile: hipcc would keep every lane's slab offsets in registers over the loop, kernels_gemm.hip)
      asm volatile("" : "+s"(dx.rs), "+s"(dx.ks), "+s"(dy.rs), "+s"(dy.ks));
      if constexpr (WT) {
        SlabWeights<T, Cfg> xw;
        xw.kw = p.kw + (long) t * p.nb;
        if constexpr (VEC)
          gemm_acc<Cfg, T, MODE, MODE>(dx, mr, dy, nc, K, lds, acc, xw);
        else
          gemm_acc<Cfg, T, 2, 2>(dx, mr, dy, nc, K, lds, acc, xw);
      }
      else if constexpr (VEC)
        gemm_acc<Cfg, T, MODE, MODE>(dx, mr, dy, nc, K, lds, acc);
      else
        gemm_acc<Cfg, T, 2, 2>(dx, mr, dy, nc, K, lds, acc);
    }

    // the one epilogue: V = bc V + al acc on the stored elements, the diagonal real
    const bool lead = p.first && pass == 0;
    const bool read_c = !lead || p.beta != R(0);
    const bool product = p.nk > 0;
    const R bc = lead ? p.beta : R(1);
    T al = p.alpha;
    if constexpr (TypeInfo<T>::is_complex)
      if ((pass == 1) != (p.conj_view != 0 && two))
        al.im = -al.im;
    auto store = [&](int m, int n, const T& v) {
      if (m < mr && n < nc && (!diag_tile || herk_element_stored(gi, gj, m0 + m, n0 + n))) {
        T* c = ct + m + (long) n * p.nb;
        const bool dg = diag_tile && herk_element_diagonal(gi, gj, m0 + m, n0 + n);
        T r = zero_el<T>();
        if (product) {
          if constexpr (TypeInfo<T>::is_complex)
            r = T{al.re * v.re - al.im * v.im, al.re * v.im + al.im * v.re};
          else
            r = al * v;
        }
        if (read_c) {
          const T o = *c;
          if constexpr (TypeInfo<T>::is_complex)
            r = T{r.re + bc * o.re, dg ? R(0) : r.im + bc * o.im};
          else
            r = r + bc * o;
        }
        if constexpr (TypeInfo<T>::is_complex)
          if (dg)
            r.im = R(0);
        *c = r;
      }
    };
    // (the fresh thread index: every vector kernel, as in kernels_gemm.hip, and the cfloat element kernel, which spills
    // 108 bytes per lane around the loop over the passes without it)
    if constexpr (VEC || std::is_same<T, cfloat>::value)
      herk_acc_foreach<Cfg, T>(acc, store);
    else
      acc_foreach<Cfg, T>(acc, store);
    // (pass 2 reads what pass 1 stored: the same lanes, the same addresses -- no barrier needed beyond gemm_acc's own)
  }
}

template <class T, int MODE, bool VEC, bool WT = false>
static void launch_rank_k_kernel(const RankKArgs<T>& a, hipStream_t stream) {
  using Cfg = typename GenCfg<T>::type;
  const int bpr = (a.nb + Cfg::BM - 1) / Cfg::BM, bpc = (a.nb + Cfg::BN - 1) / Cfg::BN;
  const long grid = (long) a.ltr * a.ltc * bpr * bpc;
  hipLaunchKernelGGL((rank_k_kernel<T, MODE, VEC, WT>), dim3((unsigned) grid), dim3(Cfg::THREADS), Cfg::LDS_BYTES, stream, a, bpr,
                     bpc);
}

template <class T>
void launch_rank_k(const RankKArgs<T>& a, hipStream_t stream) {
  using Cfg = typename GenCfg<T>::type;
  if (a.ltr <= 0 || a.ltc <= 0 || a.nb <= 0 || a.nk < 0)
    return;
  // (no block can qualify for the vector kernel when the last k tile is not a whole number of slabs)
  if (a.nk > 0 && a.k_last % Cfg::BK == 0) {
    if (herk_vector_mode(a.trans) == 0)
      launch_rank_k_kernel<T, 0, true>(a, stream);
    else
      launch_rank_k_kernel<T, 1, true>(a, stream);
  }
  launch_rank_k_kernel<T, 0, false>(a, stream);  // (one element kernel per type: the forms do not enter it)
}

// The weighted update: the same grids with the WT kernels.  args.kw: the weight of k = 0 of k tile 0 of this launch
// (device memory, nk - 1 whole tiles and k_last more reals); x2 / y2 must be null.  nk == 0: no weight is read.
template <class T>
void launch_rank_k_weighted(const RankKArgs<T>& a, hipStream_t stream) {
  using Cfg = typename GenCfg<T>::type;
  if (a.ltr <= 0 || a.ltc <= 0 || a.nb <= 0 || a.nk < 0)
    return;
  if (a.nk > 0 && a.k_last % Cfg::BK == 0) {
    if (herk_vector_mode(a.trans) == 0)
      launch_rank_k_kernel<T, 0, true, true>(a, stream);
    else
      launch_rank_k_kernel<T, 1, true, true>(a, stream);
  }
  launch_rank_k_kernel<T, 0, false, true>(a, stream);
}

template <class T>
static void herk_init_one() {
  using Cfg = typename GenCfg<T>::type;
  (void) hipFuncSetAttribute(reinterpret_cast<const void*>(&rank_k_kernel<T, 0, true>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::LDS_BYTES);
  (void) hipFuncSetAttribute(reinterpret_cast<const void*>(&rank_k_kernel<T, 1, true>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::LDS_BYTES);
  (void) hipFuncSetAttribute(reinterpret_cast<const void*>(&rank_k_kernel<T, 0, false>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::LDS_BYTES);
  (void) hipFuncSetAttribute(reinterpret_cast<const void*>(&rank_k_kernel<T, 0, true, true>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::LDS_BYTES);
  (void) hipFuncSetAttribute(reinterpret_cast<const void*>(&rank_k_kernel<T, 1, true, true>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::LDS_BYTES);
  (void) hipFuncSetAttribute(reinterpret_cast<const void*>(&rank_k_kernel<T, 0, false, true>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, Cfg::LDS_BYTES);
}

void herk_kernels_init() {
  herk_init_one<float>();
  herk_init_one<double>();
  herk_init_one<cfloat>();
  herk_init_one<cdouble>();
}

template void launch_rank_k<float>(const RankKArgs<float>&, hipStream_t);
template void launch_rank_k<double>(const RankKArgs<double>&, hipStream_t);
template void launch_rank_k<cfloat>(const RankKArgs<cfloat>&, hipStream_t);
template void launch_rank_k<cdouble>(const RankKArgs<cdouble>&, hipStream_t);
template void launch_rank_k_weighted<float>(const RankKArgs<float>&, hipStream_t);
template void launch_rank_k_weighted<double>(const RankKArgs<double>&, hipStream_t);
template void launch_rank_k_weighted<cfloat>(const RankKArgs<cfloat>&, hipStream_t);
template void launch_rank_k_weighted<cdouble>(const RankKArgs<cdouble>&, hipStream_t);

}  // namespace dlaf_mi355x
