// kernels_norm.hip -- max / one / infinity / Frobenius norm of the local part of a general, Hermitian or triangular
// block-cyclic matrix in tile layout (LAPACK xLANGE / xLANHE / xLANSY / xLANTR; the reference has the max norm only:
// include/dlaf/auxiliary/norm/mc.h).  A read-only streaming kernel: the work split and the layout of the partial
// buffers are norm_split.hpp's, the host side is norm.cpp.
//
// Pass 1, one workgroup per work unit (tile, row slab, column chunk): wave w takes the chunk's columns w, w + 4, ...;
// per column a lane loads kNormSlabLoads vectors of 16 bytes (one element on the unaligned path), rows
// (q*64 + lane)*ve + e of the slab, so that a wave instruction reads a 1 KiB run of the column.  What lies outside the
// referenced part -- rows and columns past the tile's extent, the upper part of a diagonal tile, the imaginary part of
// a Hermitian diagonal, a unit diagonal -- is replaced by 0 (or 1) before it reaches any accumulator, and a vector that
// lies wholly above the diagonal is not loaded.  All accumulation is in fp64:
//   max        fmax per lane, wave reduction, then the four waves through LDS: one value per unit
//   NaN        a flag per lane (re or im is NaN), folded like the max; it overrides every result in norm.cpp
//   col sums   per column one lane accumulator over the slab's rows and one wave_sum_fast: slot (il, sl, column)
//   row sums   per lane kNormSlabLoads*ve accumulators over the wave's columns, the four waves summed in wave order
//              through LDS: slot (jl, ch, row)
//   squares    the big / medium / small accumulators of LAPACK 3.10's xLASSQ (Blue's algorithm): |x| > 2^486 is scaled
//              by 2^-538, |x| < 2^-511 by 2^537 before it is squared, so no square overflows or underflows; complex
//              elements add re^2 and im^2.  Wave sums, then the waves in order: three values per unit.
// |z| of a complex element is hypot (no overflow for finite parts; a zero part gives the other part's magnitude
// exactly).  Every order above is fixed by the geometry alone: two runs give the same bits.
// Pass 2 combines the partials of the live units in index order (norm_scalars / norm_vector / norm_vecmax kernels).
// No atomics, no flags, no cooperative launch.
#include "device_api.hpp"
#include "lane_ops.hpp"

namespace dlaf_mi355x {

namespace {

// xLASSQ's thresholds and scalings for fp64 (LAPACK 3.10 la_constants: dtsml, dtbig, dssml, dsbig)
constexpr double kTsml = 0x1p-511, kTbig = 0x1p486, kSsml = 0x1p537, kSbig = 0x1p-538;

// op over the wave, the result in every lane (the exchange sequence of wave_sum_fast)
template <class F>
__device__ __forceinline__ double wave_all(double v, F op) {
  v = op(v, dpp_real<kDppXor1>(v));
  v = op(v, dpp_real<kDppXor2>(v));
  v = op(v, dpp_real<kDppHalfMirror>(v));
  v = op(v, dpp_real<kDppRor8>(v));
  double a = v, b = v;
  swap_real<true>(a, b);
  v = op(a, b);
  a = v;
  b = v;
  swap_real<false>(a, b);
  return op(a, b);
}

template <class T, int VE>
__device__ __forceinline__ void load_vec(const T* __restrict__ p, T (&out)[VE]) {
  if constexpr (VE * sizeof(T) == 16) {
    typedef unsigned int u4 __attribute__((ext_vector_type(4)));
    const u4 raw = *reinterpret_cast<const u4*>(p);
    __builtin_memcpy(&out[0], &raw, 16);
  }
  else {
    static_assert(VE == 1, "the narrow path loads one element");
    out[0] = *p;
  }
}

template <class T, int MODE, bool VEC>
__global__ __launch_bounds__(kThreads) void norm_pass1_kernel(const NormArgs<T> p) {
  constexpr bool CX = TypeInfo<T>::is_complex;
  constexpr int VE = (VEC && sizeof(T) < 16) ? 16 / (int) sizeof(T) : 1;
  constexpr bool COL = MODE == kNormCol || MODE == kNormColRow;
  constexpr bool ROW = MODE == kNormRow || MODE == kNormColRow;
  constexpr bool ABS = COL || ROW || MODE == kNormMax;
  constexpr int SLAB = kNormSlabLoads * kNormLanes * VE;
  static_assert(kThreads == kNormWaves * kNormLanes, "four waves per unit");
  __shared__ double sh_row[ROW ? kNormWaves * SLAB : 1];
  __shared__ double sh_sc[kNormWaves][kNormScalars];

  const NormGeom& g = p.g;
  const NormSplit& s = p.s;
  const int sl = (int) blockIdx.x % s.nsl, ch = (int) blockIdx.x / s.nsl;
  const int il = (int) blockIdx.y, jl = (int) blockIdx.z;
  double* sc = p.scal + norm_unit_index(g, s, il, jl, sl, ch) * kNormScalars;
  if (!norm_unit_live(g, s, il, jl, sl, ch)) {  // (the whole workgroup)
    if (threadIdx.x < kNormScalars)
      sc[threadIdx.x] = 0.0;
    return;
  }
  const int lane = (int) threadIdx.x % kNormLanes, w = (int) threadIdx.x / kNormLanes;
  const int rt = norm_tile_rows(g, il), ct = norm_tile_cols(g, jl);
  const bool dtile = g.structure != 0 && (long) il * g.pr + g.ri == (long) jl * g.pc + g.ci;
  const bool herm = g.structure == 1;
  const bool unit = g.structure == 2 && p.unit != 0;
  const T* __restrict__ tile = p.tiles + ((long) il + (long) jl * g.ltr) * g.nb * g.nb;
  const int r0 = sl * SLAB, c0 = ch * s.cw;
  const int c1 = min(ct, c0 + s.cw);

  double rowacc[kNormSlabLoads][VE];
#pragma unroll
  for (int q = 0; q < kNormSlabLoads; ++q)
#pragma unroll
    for (int e = 0; e < VE; ++e)
      rowacc[q][e] = 0.0;
  double mx = 0.0, big = 0.0, med = 0.0, sml = 0.0;
  bool nan = false;

  for (int c = c0 + w; c < c1; c += kNormWaves) {  // (bounds are the wave's: no lane leaves early)
    const T* __restrict__ col = tile + (long) c * g.nb;
    T v[kNormSlabLoads][VE];
#pragma unroll
    for (int q = 0; q < kNormSlabLoads; ++q) {
      const int r = r0 + (q * kNormLanes + lane) * VE;
      // r + VE <= nb whenever r < rt: the load stays inside the tile; a vector wholly above the diagonal is skipped
      if (r < rt && (!dtile || r + VE - 1 >= c))
        load_vec<T, VE>(col + r, v[q]);
      else {
#pragma unroll
        for (int e = 0; e < VE; ++e)
          v[q][e] = zero_el<T>();
      }
    }
    double colacc = 0.0;
#pragma unroll
    for (int q = 0; q < kNormSlabLoads; ++q) {
#pragma unroll
      for (int e = 0; e < VE; ++e) {
        const int rr = r0 + (q * kNormLanes + lane) * VE + e;
        const bool in = rr < rt && (!dtile || rr >= c);
        const bool dg = dtile && rr == c;
        double re = (double) re_of(v[q][e]);
        double im = CX ? (double) im_of(v[q][e]) : 0.0;
        if (dg && herm)
          im = 0.0;
        if (dg && unit) {
          re = 1.0;
          im = 0.0;
        }
        if (!in) {
          re = 0.0;
          im = 0.0;
        }
        nan = nan || re != re || im != im;
        if constexpr (ABS) {
          double a = fabs(re);
          if constexpr (CX)
            a = im == 0.0 ? fabs(re) : (re == 0.0 ? fabs(im) : hypot(re, im));
          if constexpr (MODE == kNormMax)
            mx = fmax(mx, a);
          if constexpr (COL)
            colacc += a;
          if constexpr (ROW) {
            // Hermitian: the row sum takes the mirrored image (j, i) of the stored element, which the diagonal lacks
            rowacc[q][e] += (herm && dg) ? 0.0 : a;
          }
        }
        if constexpr (MODE == kNormFro) {
          const double wgt = (herm && !dg) ? 2.0 : 1.0;
          auto square = [&](double x) {
            const double ax = fabs(x);
            const bool isb = ax > kTbig, iss = ax < kTsml;
            const double y = ax * (isb ? kSbig : (iss ? kSsml : 1.0));
            const double t = wgt * y * y;
            big += isb ? t : 0.0;
            sml += iss ? t : 0.0;
            med += (isb || iss) ? 0.0 : t;
          };
          square(re);
          if constexpr (CX)
            square(im);
        }
      }
    }
    if constexpr (COL) {
      colacc = wave_sum_fast(colacc);
      if (lane == 0)
        p.colp[norm_colp_slot(g, s, il, sl, jl, c)] = colacc;
    }
  }

  if constexpr (ROW) {
#pragma unroll
    for (int q = 0; q < kNormSlabLoads; ++q)
#pragma unroll
      for (int e = 0; e < VE; ++e)
        sh_row[w * SLAB + (q * kNormLanes + lane) * VE + e] = rowacc[q][e];
    __syncthreads();
    for (int idx = (int) threadIdx.x; idx < SLAB && r0 + idx < rt; idx += kThreads) {
      double t = sh_row[idx];
#pragma unroll
      for (int k = 1; k < kNormWaves; ++k)
        t += sh_row[k * SLAB + idx];
      p.rowp[norm_rowp_slot(g, s, jl, ch, il, r0 + idx)] = t;
    }
  }

  mx = wave_all(mx, [](double a, double b) { return fmax(a, b); });
  const double flag = __any(nan ? 1 : 0) ? 1.0 : 0.0;
  if constexpr (MODE == kNormFro) {
    big = wave_sum_fast(big);
    med = wave_sum_fast(med);
    sml = wave_sum_fast(sml);
  }
  if (lane == 0) {
    sh_sc[w][0] = mx;
    sh_sc[w][1] = flag;
    sh_sc[w][2] = big;
    sh_sc[w][3] = med;
    sh_sc[w][4] = sml;
  }
  __syncthreads();
  if (threadIdx.x < kNormScalars) {
    const int k = (int) threadIdx.x;
    double t = sh_sc[0][k];
#pragma unroll
    for (int ww = 1; ww < kNormWaves; ++ww)
      t = k < 2 ? fmax(t, sh_sc[ww][k]) : t + sh_sc[ww][k];
    sc[k] = t;
  }
}

// one workgroup: thread t folds the units t, t + 256, ... in that order, then a fixed tree over the threads
__global__ __launch_bounds__(kThreads) void norm_scalars_kernel(const double* __restrict__ scal, long units,
                                                                double* __restrict__ out) {
  __shared__ double sh[kThreads][kNormScalars];
  double a[kNormScalars] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (long i = threadIdx.x; i < units; i += kThreads) {
    const double* q = scal + i * kNormScalars;
    a[0] = fmax(a[0], q[0]);
    a[1] = fmax(a[1], q[1]);
    a[2] += q[2];
    a[3] += q[3];
    a[4] += q[4];
  }
#pragma unroll
  for (int k = 0; k < kNormScalars; ++k)
    sh[threadIdx.x][k] = a[k];
  __syncthreads();
  for (int st = kThreads / 2; st > 0; st >>= 1) {
    if ((int) threadIdx.x < st) {
      double* m = sh[threadIdx.x];
      const double* o = sh[threadIdx.x + st];
      m[0] = fmax(m[0], o[0]);
      m[1] = fmax(m[1], o[1]);
      m[2] += o[2];
      m[3] += o[3];
      m[4] += o[4];
    }
    __syncthreads();
  }
  if (threadIdx.x < kNormScalars)
    out[threadIdx.x] = sh[0][threadIdx.x];
}

// one thread per global index x: the partial column sums of column x over (il, sl) in that order, then the partial row
// sums of row x over (jl, ch)
__global__ __launch_bounds__(kThreads) void norm_vector_kernel(NormGeom g, NormSplit s, int mode,
                                                               const double* __restrict__ colp,
                                                               const double* __restrict__ rowp, double* __restrict__ v,
                                                               long len) {
  const long x = (long) blockIdx.x * kThreads + threadIdx.x;
  if (x >= len)
    return;
  const long gt = x / g.nb;
  const int off = (int) (x % g.nb);
  double t = 0.0;
  if ((mode & kNormCol) && gt % g.pc == g.ci && gt / g.pc < g.ltc) {
    const int jl = (int) (gt / g.pc);
    if (off < norm_tile_cols(g, jl)) {
      const int ch = off / s.cw;
      for (int il = 0; il < g.ltr; ++il)
        for (int sl = 0; sl < s.nsl; ++sl)
          if (norm_unit_live(g, s, il, jl, sl, ch))
            t += colp[norm_colp_slot(g, s, il, sl, jl, off)];
    }
  }
  if ((mode & kNormRow) && gt % g.pr == g.ri && gt / g.pr < g.ltr) {
    const int il = (int) (gt / g.pr);
    if (off < norm_tile_rows(g, il)) {
      const int sl = off / s.slab_rows;
      for (int jl = 0; jl < g.ltc; ++jl)
        for (int ch = 0; ch < s.nch; ++ch)
          if (norm_unit_live(g, s, il, jl, sl, ch))
            t += rowp[norm_rowp_slot(g, s, jl, ch, il, off)];
    }
  }
  v[x] = t;
}

__global__ __launch_bounds__(kThreads) void norm_vecmax_kernel(const double* __restrict__ v, long len,
                                                               double* __restrict__ out) {
  __shared__ double sh[kThreads];
  double m = 0.0;
  for (long i = threadIdx.x; i < len; i += kThreads)
    m = fmax(m, v[i]);
  sh[threadIdx.x] = m;
  __syncthreads();
  for (int st = kThreads / 2; st > 0; st >>= 1) {
    if ((int) threadIdx.x < st)
      sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + st]);
    __syncthreads();
  }
  if (threadIdx.x == 0)
    *out = sh[0];
}

template <class T, int MODE>
void launch_pass1_mode(const NormArgs<T>& a, dim3 grid, hipStream_t stream) {
  if (a.s.ve > 1 || sizeof(T) == 16)
    hipLaunchKernelGGL((norm_pass1_kernel<T, MODE, true>), grid, dim3(kThreads), 0, stream, a);
  else
    hipLaunchKernelGGL((norm_pass1_kernel<T, MODE, false>), grid, dim3(kThreads), 0, stream, a);
}

}  // namespace

template <class T>
void launch_norm_pass1(const NormArgs<T>& a, hipStream_t stream) {
  if (a.g.ltr <= 0 || a.g.ltc <= 0)
    return;
  const dim3 grid((unsigned) (a.s.nsl * a.s.nch), (unsigned) a.g.ltr, (unsigned) a.g.ltc);
  switch (a.mode) {
    case kNormMax: launch_pass1_mode<T, kNormMax>(a, grid, stream); break;
    case kNormCol: launch_pass1_mode<T, kNormCol>(a, grid, stream); break;
    case kNormRow: launch_pass1_mode<T, kNormRow>(a, grid, stream); break;
    case kNormColRow: launch_pass1_mode<T, kNormColRow>(a, grid, stream); break;
    default: launch_pass1_mode<T, kNormFro>(a, grid, stream); break;
  }
}

void launch_norm_scalars(const double* scal, long units, double* out, hipStream_t stream) {
  hipLaunchKernelGGL(norm_scalars_kernel, dim3(1), dim3(kThreads), 0, stream, scal, units, out);
}

void launch_norm_vector(const NormGeom& g, const NormSplit& s, int mode, const double* colp, const double* rowp,
                        double* v, long len, hipStream_t stream) {
  if (len <= 0)
    return;
  hipLaunchKernelGGL(norm_vector_kernel, dim3((unsigned) ((len + kThreads - 1) / kThreads)), dim3(kThreads), 0, stream,
                     g, s, mode, colp, rowp, v, len);
}

void launch_norm_vecmax(const double* v, long len, double* out, hipStream_t stream) {
  hipLaunchKernelGGL(norm_vecmax_kernel, dim3(1), dim3(kThreads), 0, stream, v, len, out);
}

#define INST(T) template void launch_norm_pass1<T>(const NormArgs<T>&, hipStream_t);
INST(float)
INST(double)
INST(cfloat)
INST(cdouble)
#undef INST

}  // namespace dlaf_mi355x
