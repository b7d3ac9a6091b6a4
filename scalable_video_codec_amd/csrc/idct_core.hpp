// idct_core.hpp -- the decoder's per-coefficient arithmetic, shared by every kernel that reconstructs tiles (idct.hip from f32
// planes, levels.hip straight from the compact stream, entropy.hip from the entropy-coded one, records.hip from the wire records):
// the f64 inverse DCT basis, the 1-D inverse transform and the quantise-round-dequantise of DecodeBlock; and what the stream
// decoders share, the gaze test of a tile, the row and column passes of a tile plane and the store of a thread's pixel column.
// One definition, so that all paths produce the same bits.
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
template <> struct IBasis<4> {  // 4 and 2: the reduced decode's K-point transforms (K = N / reduce)
  static __device__ __forceinline__ double even(int k, int n) { return kDctEven4[k][n]; }
  static __device__ __forceinline__ double odd(int k, int n) { return kDctOdd4[k][n]; }
};
template <> struct IBasis<2> {
  static __device__ __forceinline__ double even(int k, int n) { return kDctEven2[k][n]; }
  static __device__ __forceinline__ double odd(int k, int n) { return kDctOdd2[k][n]; }
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

// The reconstruction of one plane of a tile in the stream decoders.  Thread (t, j) of a workgroup owns row j and then column j of
// the workgroup's tile t; `slab` is the workgroup's f64 LDS slab, one row per (tile, coefficient row) at pitch N + 1 (the column
// reads of a wave then spread over the banks).  invert_row: the tile's dequantised coefficient row `coef` is requantised with the
// decoder's step, inverted and written to the slab.  After a workgroup barrier, invert_column: column j is read back, inverted and
// rounded once to f32.  A second barrier before the slab is written again.  Rows and columns go through idct1d exactly as in
// idct_kernel, so a plane has the bits of svc_hip_decode_frames on the same coefficients.
// (decode_entropy_kernel keeps this text written out: entropy.hip says why.)
template <int N>
__device__ __forceinline__ void invert_row(const float* coef, float step, double* slab, uint32_t t, uint32_t j) {
  double y[N], r[N];
#pragma unroll
  for (int i = 0; i < N; ++i) y[i] = (double)requant(coef[i], step);
  idct1d<N>(y, r);
  double* row = slab + (t * N + j) * (N + 1);
#pragma unroll
  for (int i = 0; i < N; ++i) row[i] = r[i];
}

template <int N>
__device__ __forceinline__ void invert_column(const double* slab, uint32_t t, uint32_t j, float (&out)[N]) {
  double cc[N], xx[N];
#pragma unroll
  for (int v = 0; v < N; ++v) cc[v] = slab[(t * N + v) * (N + 1) + j];
  idct1d<N>(cc, xx);
#pragma unroll
  for (int y = 0; y < N; ++y) out[y] = (float)xx[y];
}

// The reduced decode (svc_hip_decode_levels_reduced_frames): the same two passes on the first K x K coefficients of an N x N tile, with the
// K-point transform and a slab of pitch K + 1; thread (t, j), j < K.  The 1-point transform is the identity.  The column pass scales by
// K / N (a power of two: exact) before its one rounding to f32.
template <int K>
__device__ __forceinline__ void idct1d_reduced(const double* __restrict__ y, double* __restrict__ x) {
  if constexpr (K == 1) x[0] = y[0];
  else idct1d<K>(y, x);
}

template <int K>
__device__ __forceinline__ void invert_row_reduced(const float* coef, float step, double* slab, uint32_t t, uint32_t j) {
  double y[K], r[K];
#pragma unroll
  for (int i = 0; i < K; ++i) y[i] = (double)requant(coef[i], step);
  idct1d_reduced<K>(y, r);
  double* row = slab + (t * K + j) * (K + 1);
#pragma unroll
  for (int i = 0; i < K; ++i) row[i] = r[i];
}

template <int N, int K>
__device__ __forceinline__ void invert_column_reduced(const double* slab, uint32_t t, uint32_t j, float (&out)[K]) {
  double cc[K], xx[K];
#pragma unroll
  for (int v = 0; v < K; ++v) cc[v] = slab[(t * K + v) * (K + 1) + j];
  idct1d_reduced<K>(cc, xx);
#pragma unroll
  for (int y = 0; y < K; ++y) out[y] = (float)(xx[y] * ((double)K / N));
}

// is the tile at (tx, ty) inside frame f's gaze rectangle?  gaze = [n][4] x, y, w, h in padded coordinates, or null (no gaze):
// x <= tx < x + w && y <= ty < y + h, without overflow
__device__ __forceinline__ bool gazed(const uint32_t* gaze, uint32_t f, uint32_t tx, uint32_t ty) {
  if (!gaze) return false;
  const uint32_t* r = gaze + 4ull * f;
  return tx >= r[0] && tx - r[0] < r[2] && ty >= r[1] && ty - r[1] < r[3];
}

// a thread's column of N interleaved B,G,R pixels, from dst down rows of w pixels (the lanes of a wave hold adjacent columns)
template <int N>
__device__ __forceinline__ void store_bgr_column(float* dst, uint32_t w, const float (&out)[3][N]) {
#pragma unroll
  for (int y = 0; y < N; ++y) {
    float* p = dst + (size_t)y * w * 3;
    p[0] = out[0][y]; p[1] = out[1][y]; p[2] = out[2][y];
  }
}

}  // namespace svc
