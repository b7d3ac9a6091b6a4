// dct_core.hpp -- the arithmetic and the LDS shape the tuned forward-transform kernels share (dct.hip: planes and records;
// dct_pack.hip: the compact stream straight from the transform): the basis tables, the recursive even/odd N-point DCT-II,
// the wave-local LDS ordering and the slab pitches.  One definition, as quant_core.hpp is for the quantiser.
#pragma once

#include "svc_common.hpp"

namespace svc {

#include "dct_tables.inc"

template <int N> struct Basis;
template <> struct Basis<8> {
  static __device__ __forceinline__ double even(int k, int i) { return kDctEven8[k][i]; }
  static __device__ __forceinline__ double odd(int k, int i) { return kDctOdd8[k][i]; }
};
template <> struct Basis<16> {
  static __device__ __forceinline__ double even(int k, int i) { return kDctEven16[k][i]; }
  static __device__ __forceinline__ double odd(int k, int i) { return kDctOdd16[k][i]; }
};

template <int N, int L> struct RecTab;
#define SVC_RECTAB(N_, L_) \
  template <> struct RecTab<N_, L_> { \
    static __device__ __forceinline__ double at(int r, int i) { return kDctRec##N_##_L##L_[r][i]; } \
  }
SVC_RECTAB(8, 0); SVC_RECTAB(8, 1); SVC_RECTAB(8, 2);
SVC_RECTAB(16, 0); SVC_RECTAB(16, 1); SVC_RECTAB(16, 2); SVC_RECTAB(16, 3);
#undef SVC_RECTAB
template <int N> struct RecDc;
template <> struct RecDc<8> { static constexpr double v = kDctRec8_Dc; };
template <> struct RecDc<16> { static constexpr double v = kDctRec16_Dc; };

// N-point orthonormal DCT-II by the even/odd split of the basis, applied recursively: the odd rows
// of a level act on the differences x[i] - x[M-1-i], the even rows are a scaled M/2-point DCT of the
// sums (86 multiplies for 16 points instead of 128, 22 instead of 32 for 8).  x holds the M inputs
// of level L, y the N outputs: level L produces the rows k = 2^L * odd.
// T = int for the row pass: the inputs are bytes, so the sums and differences of every level are integers <= 4080 (byte
// extraction folds into the adds as SDWA operands); each operand of a multiply is widened once (v_cvt_f64_i32).
template <int N, int M, int L, typename T>
__device__ __forceinline__ void dct_level(const T* __restrict__ x, double* __restrict__ y) {
  if constexpr (M == 1) {
    y[0] = RecDc<N>::v * (double)x[0];
  } else {
    constexpr int H = M / 2;
    T s[H];
    double d[H];
#pragma unroll
    for (int i = 0; i < H; ++i) {
      s[i] = x[i] + x[M - 1 - i];
      d[i] = (double)(x[i] - x[M - 1 - i]);
    }
#pragma unroll
    for (int r = 0; r < H; ++r) {
      double o = RecTab<N, L>::at(r, 0) * d[0];
#pragma unroll
      for (int i = 1; i < H; ++i) o = __builtin_fma(RecTab<N, L>::at(r, i), d[i], o);
      y[(1 << L) * (2 * r + 1)] = o;
    }
    dct_level<N, H, L + 1, T>(s, y);
  }
}

template <int N, typename T>
__device__ __forceinline__ void dct1d(const T* __restrict__ x, double* __restrict__ y) {
  dct_level<N, N, 0, T>(x, y);
}

__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

constexpr int kRowPitch = 144;                  // 16 f64 + 16 B pad
constexpr int kSlab8 = 8 * kRowPitch;           // 1152 B  (= 128 mod 256)
constexpr int kSlab16 = 16 * kRowPitch + 128;   // 2432 B  (= 128 mod 256)

}  // namespace svc
