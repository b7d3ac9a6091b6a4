// idct_core.hpp -- the decoder's per-coefficient arithmetic, shared by every kernel that reconstructs tiles (idct.hip from f32
// planes, levels.hip straight from the compact stream): the f64 inverse DCT basis, the 1-D inverse transform and the
// quantise-round-dequantise of DecodeBlock.  One definition, so that both paths produce the same bits.
#pragma once

#include "svc_common.hpp"

namespace svc {

#include "dct_tables.inc"

template <int N> struct IBasis;
template <> struct IBasis<8> {
  static __device__ __forceinline__ double even(int k, int n) { return kDctEven8[k][n]; }
  static __device__ __forceinline__ double odd(int k, int n) { return kDctOdd8[k][n]; }
};
template <> struct IBasis<16> {
  static __device__ __forceinline__ double even(int k, int n) { return kDctEven16[k][n]; }
  static __device__ __forceinline__ double odd(int k, int n) { return kDctOdd16[k][n]; }
};

// x[n] = sum_k C[k][n] y[k]: even-k terms are symmetric, odd-k terms antisymmetric in n <-> N-1-n
template <int N>
__device__ __forceinline__ void idct1d(const double* __restrict__ y, double* __restrict__ x) {
  constexpr int H = N / 2;
#pragma unroll
  for (int n = 0; n < H; ++n) {
    double e = IBasis<N>::even(0, n) * y[0];
    double o = IBasis<N>::odd(0, n) * y[1];
#pragma unroll
    for (int k = 1; k < H; ++k) {
      e = __builtin_fma(IBasis<N>::even(k, n), y[2 * k], e);
      o = __builtin_fma(IBasis<N>::odd(k, n), y[2 * k + 1], o);
    }
    x[n] = e + o;
    x[N - 1 - n] = e - o;
  }
}

__device__ __forceinline__ float requant(float c, float step) {  // libs/decoder.cpp:141-143, IEEE divide
  float q = c / step;
  q = roundf(q);
  return q * step;
}

}  // namespace svc
