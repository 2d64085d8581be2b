// kernels_geadd.hip -- D = beta D + alpha op(S) on the uplo part of a matrix in tile layout: PBLAS p?geadd / p?tradd,
// p?tran / p?tranu / p?tranc, ScaLAPACK p?lacpy, and the completion of a Hermitian / symmetric matrix from one triangle.
// One memory-bound kernel in two forms; geadd_map.hpp holds every index it uses.
//
//   straight     (op N): every thread moves 16-byte vectors down tile columns, global -> registers -> global.  No LDS.
//   transposing  (op T / C): the source sub-block goes global -> registers -> LDS in ITS column order, a barrier, then
//                LDS -> registers -> global in the destination's column order.  Both global sides are 16-byte accesses in
//                contiguous runs of B elements; only the LDS read is per element.
//
// LDS image (geadd_lds_index): unpadded columns of B elements whose 16-byte slots are XOR-swizzled with the column's slot
// index.  A column is a whole number of bank rows, so the bank of an access is the swizzled slot's alone.  By the bank
// rule (every ds_write and the paired ds_read2: bank (a/4) % 32; ds_read_b64 / b128: (a/4) % 64; lane groups of 8 for a
// 16-byte store, 16 for ds_read2_b64 and ds_read_b128, 32 for ds_read_b32 / b64):
//   store side  a group of 8 lanes writes 8 consecutive slots of one column, permuted inside an aligned 128 bytes:
//               conflict-free for every type
//   load side   the lanes of a group read one source row from columns ve apart, whose slots the swizzle spreads: float
//               (32 lanes over 8 slot positions of 4 banks, 2 of 4 banks used) and double / complex float are 2-way,
//               both as single reads and as the ds_read2st64 pairs the compiler makes of two neighbouring columns;
//               complex double (ds_read_b128, 16 lanes, 16 distinct slots) is conflict-free
// (tests/geadd_map/sweep.cpp counts the same from the rule and prints it).  At HBM rate a compute unit moves about 10
// bytes per clock through an LDS that serves 128 and more: the 2-way reads are not on the critical path.
//
// Every instantiation is plain HIP, holds its vectors in registers and builds without scratch.
#include "device_api.hpp"

namespace dlaf_mi355x {

namespace {

template <class T, int VE>
struct alignas(VE * sizeof(T)) GeaddVec {
  T v[VE];
};

template <class T>
__device__ __forceinline__ T geadd_mul(const T& x, const T& y) {
  if constexpr (TypeInfo<T>::is_complex)
    return T{x.re * y.re - x.im * y.im, x.re * y.im + x.im * y.re};
  else
    return x * y;
}
template <class T>
__device__ __forceinline__ T geadd_add(const T& x, const T& y) {
  if constexpr (TypeInfo<T>::is_complex)
    return T{x.re + y.re, x.im + y.im};
  else
    return x + y;
}

// what is stored for a source value s and the old destination value o
template <class T, int ARITH>
__device__ __forceinline__ T geadd_value(const GeaddArgs<T>& p, T s, const T& o, bool on_diag) {
  T r;
  if constexpr (TypeInfo<T>::is_complex) {
    if (geadd_reads_a(ARITH) && p.conj)
      s.im = -s.im;
  }
  if constexpr (ARITH == kGeaddCopy)
    r = s;
  else if constexpr (ARITH == kGeaddScale)
    r = geadd_mul(p.alpha, s);
  else if constexpr (ARITH == kGeaddAxpby)
    r = geadd_add(geadd_mul(p.beta, o), geadd_mul(p.alpha, s));
  else if constexpr (ARITH == kGeaddScaleC)
    r = geadd_mul(p.beta, o);
  else
    r = zero_el<T>();
  if constexpr (TypeInfo<T>::is_complex) {
    if (p.diag_real && on_diag)
      r.im = real_t<T>(0);
  }
  return r;
}

// the registers, the global accesses and the LDS traffic are raw dwords: 4, 8 or 16 bytes in one native vector
template <int BYTES>
struct GeaddRaw;
template <>
struct GeaddRaw<4> {
  typedef unsigned type;
};
template <>
struct GeaddRaw<8> {
  typedef unsigned type __attribute__((ext_vector_type(2)));
};
template <>
struct GeaddRaw<16> {
  typedef unsigned type __attribute__((ext_vector_type(4)));
};
__device__ __forceinline__ unsigned geadd_dword(unsigned r, int) {
  return r;
}
template <class R>
__device__ __forceinline__ unsigned geadd_dword(const R& r, int k) {
  return r[k];
}
__device__ __forceinline__ void geadd_set_dword(unsigned& r, int, unsigned v) {
  r = v;
}
template <class R>
__device__ __forceinline__ void geadd_set_dword(R& r, int k, unsigned v) {
  r[k] = v;
}

// stores the VE values x of destination rows [r, r + VE) of column c of tile ct (unit u): one 16-byte access when all of
// them are valid and inside the part, element by element otherwise
template <class T, int VE, int ARITH>
__device__ __forceinline__ void geadd_put(const GeaddArgs<T>& p, const GeaddUnit& u, T* ct, int r, int c,
                                          const typename GeaddRaw<VE * sizeof(T)>::type& xr) {
  using V = GeaddVec<T, VE>;
  using Raw = typename GeaddRaw<VE * sizeof(T)>::type;
  const V x = __builtin_bit_cast(V, xr);
  const int rend = u.r0 + u.nr;
  const long gr = u.gr0 + (r - u.r0), gc = u.gc0 + (c - u.c0);
  T* d = ct + r + (long) c * p.g.nb;
  if (geadd_vector_whole(p.mask, u.cls, VE, r, rend, gr, gc)) {
    V o{};
    if constexpr (geadd_reads_c(ARITH))
      o = __builtin_bit_cast(V, *reinterpret_cast<const Raw*>(d));
    V y;
#pragma unroll
    for (int e = 0; e < VE; ++e)
      y.v[e] = geadd_value<T, ARITH>(p, x.v[e], o.v[e], gr + e == gc);
    *reinterpret_cast<Raw*>(d) = __builtin_bit_cast(Raw, y);
  }
  else {
#pragma unroll
    for (int e = 0; e < VE; ++e) {
      if (geadd_element_written(p.mask, u.cls, r, e, rend, gr, gc)) {
        T o = zero_el<T>();
        if constexpr (geadd_reads_c(ARITH))
          o = d[e];
        d[e] = geadd_value<T, ARITH>(p, x.v[e], o, gr + e == gc);
      }
    }
  }
}

// grid: x = sub-block inside a tile (bi + nsb bj), y = il - il0, z = jl
template <class T, int VE, bool TRANS, int ARITH>
__global__ __launch_bounds__(kGeaddThreads) void geadd_kernel(GeaddArgs<T> p) {
  using Raw = typename GeaddRaw<VE * sizeof(T)>::type;
  using RawE = typename GeaddRaw<sizeof(T)>::type;
  constexpr int B = geadd_block((int) sizeof(T));
  constexpr int NQ = B * B / VE / kGeaddThreads;
  constexpr int ND = (int) sizeof(T) / 4;  // dwords of an element
  const int nsb = geadd_sub_blocks(p.g.nb, B);
  const int bi = (int) blockIdx.x % nsb, bj = (int) blockIdx.x / nsb;
  const int il = p.g.il0 + (int) blockIdx.y, jl = (int) blockIdx.z;
  const GeaddUnit u = geadd_unit(p.g, p.mask, B, il, jl, bi, bj);
  if (u.cls == kGeaddDead)
    return;
  T* ct = p.c + (long) il * p.c_tsr + (long) jl * p.c_tsc;
  const T* at = nullptr;
  if constexpr (geadd_reads_a(ARITH))
    at = p.a + geadd_src_tile_offset(p.g, il, jl, p.a_tsi, p.a_period, p.a_ts, p.a_ts2);
  const int tid = (int) threadIdx.x;

  if constexpr (!TRANS) {
    Raw x[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int v = tid + q * kGeaddThreads;
      const int lr = geadd_vec_row(VE, B, v), lc = geadd_vec_col(VE, B, v);
      Raw t = {};
      if constexpr (geadd_reads_a(ARITH))
        if (lr < u.nr && lc < u.nc)
          t = *reinterpret_cast<const Raw*>(at + geadd_src_elem(false, u.r0 + lr, u.c0 + lc, p.g.nb));
      x[q] = t;
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int v = tid + q * kGeaddThreads;
      const int lr = geadd_vec_row(VE, B, v), lc = geadd_vec_col(VE, B, v);
      if (lr < u.nr && lc < u.nc)
        geadd_put<T, VE, ARITH>(p, u, ct, u.r0 + lr, u.c0 + lc, x[q]);
    }
  }
  else {
    __shared__ Raw image[B * B / VE];
    T* lds = reinterpret_cast<T*>(image);
    // the source sub-block: rows = my columns, columns = my rows.  A vector that starts inside the source extent may
    // reach into the tile's padding rows (never past nb: nb and c0 are multiples of VE on the vector path).
    Raw x[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int v = tid + q * kGeaddThreads;
      const int sr = geadd_vec_row(VE, B, v), sc = geadd_vec_col(VE, B, v);
      Raw t = {};
      if (sr < u.nc && sc < u.nr)
        t = *reinterpret_cast<const Raw*>(at + geadd_src_elem(false, u.c0 + sr, u.r0 + sc, p.g.nb));
      x[q] = t;
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int v = tid + q * kGeaddThreads;
      const int sr = geadd_vec_row(VE, B, v), sc = geadd_vec_col(VE, B, v);
      *reinterpret_cast<Raw*>(lds + geadd_lds_index(VE, B, sr, sc)) = x[q];
    }
    // every global read of this workgroup has landed before any of its global writes: what the in-place completion of
    // a diagonal sub-block rests on
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int v = tid + q * kGeaddThreads;
      const int lr = geadd_vec_row(VE, B, v), lc = geadd_vec_col(VE, B, v);
      if (lr < u.nr && lc < u.nc) {
        Raw y = {};
#pragma unroll
        for (int e = 0; e < VE; ++e) {
          // destination (lr + e, lc) = source (lc, lr + e)
          const RawE el = *reinterpret_cast<const RawE*>(lds + geadd_lds_index(VE, B, lc, lr + e));
#pragma unroll
          for (int k = 0; k < ND; ++k)
            geadd_set_dword(y, e * ND + k, geadd_dword(el, k));
        }
        geadd_put<T, VE, ARITH>(p, u, ct, u.r0 + lr, u.c0 + lc, y);
      }
    }
  }
}

template <class T, int VE, bool TRANS, int ARITH>
void launch_one(const GeaddArgs<T>& a, hipStream_t stream) {
  constexpr int B = geadd_block((int) sizeof(T));
  const int nsb = geadd_sub_blocks(a.g.nb, B);
  dim3 grid((unsigned) (nsb * nsb), (unsigned) a.g.nil, (unsigned) a.g.ltc);
  hipLaunchKernelGGL((geadd_kernel<T, VE, TRANS, ARITH>), grid, dim3(kGeaddThreads), 0, stream, a);
}

template <class T, int VE>
void launch_ve(const GeaddArgs<T>& a, hipStream_t stream) {
  if (a.trans) {
    switch (a.arith) {
      case kGeaddCopy: return launch_one<T, VE, true, kGeaddCopy>(a, stream);
      case kGeaddScale: return launch_one<T, VE, true, kGeaddScale>(a, stream);
      case kGeaddAxpby: return launch_one<T, VE, true, kGeaddAxpby>(a, stream);
      default: break;  // (no source: nothing to transpose)
    }
  }
  switch (a.arith) {
    case kGeaddCopy: return launch_one<T, VE, false, kGeaddCopy>(a, stream);
    case kGeaddScale: return launch_one<T, VE, false, kGeaddScale>(a, stream);
    case kGeaddAxpby: return launch_one<T, VE, false, kGeaddAxpby>(a, stream);
    case kGeaddScaleC: return launch_one<T, VE, false, kGeaddScaleC>(a, stream);
    default: return launch_one<T, VE, false, kGeaddZero>(a, stream);
  }
}

}  // namespace

template <class T>
void launch_geadd(const GeaddArgs<T>& a, hipStream_t stream) {
  if (a.g.nil <= 0 || a.g.ltc <= 0 || a.g.nb <= 0)
    return;
  constexpr int kVe = sizeof(T) >= 16 ? 1 : 16 / (int) sizeof(T);
  if (a.ve == kVe)
    launch_ve<T, kVe>(a, stream);
  else
    launch_ve<T, 1>(a, stream);
}

template void launch_geadd<float>(const GeaddArgs<float>&, hipStream_t);
template void launch_geadd<double>(const GeaddArgs<double>&, hipStream_t);
template void launch_geadd<cfloat>(const GeaddArgs<cfloat>&, hipStream_t);
template void launch_geadd<cdouble>(const GeaddArgs<cdouble>&, hipStream_t);

}  // namespace dlaf_mi355x
