// quant_core.hpp -- the quantise-round-dequantise of libs/decoder.cpp:141-143 as the transform kernels apply it: the plain
// three lines (quant1) and the two cheaper forms the fused kernels of dct.hip use (quant1_fast, quant2_fast).  One definition,
// so that the test-only translation unit tests/quant_probe/quant_probe.hip runs exactly the functions the kernels inline.
#pragma once

#include "svc_common.hpp"

namespace svc {

// libs/decoder.cpp:141-143: c /= step; c = std::round(c); c *= step  (all f32)
__device__ __forceinline__ float quant1(float c, float step) {
  float q = c / step;  // correctly rounded (hipcc default), as the CPU's divss
  q = roundf(q);
  return q * step;
}

// The same three lines at a fraction of the cost (the IEEE divide expansion + roundf are
// ~60 issue cycles per coefficient on gfx950 and made the fused kernel VALU-bound):
//  - division: q0 = c * inv, r = fma(-q0, step, c), q = fma(r, inv, q0) with inv = RN(1/step)
//    from the host is the correctly rounded quotient (Markstein's correction step) as long
//    as nothing under/overflows -- coefficients here are 0 or 1e-16 < |c| < 4100;
//  - std::round (half away from zero) == trunc(q + copysign(0.5 - 2^-25, q)) for every float.  The sign is taken from c: q has
//    the sign of c, except that the correction chain turns c = -0.0 into q = +0.0 (fma(+0, step, -0) = +0), where c / step is -0.0.
// Both identities are checked bit-for-bit against the oracle by tests/test_gpu_transform_exact.py::test_quant_fast_at_every_tie:
// both functions on every f32 within 3 ulp of every rounding tie (k + 1/2) * step a coefficient can reach, for steps 1 ... 2048
// and a sample of larger ones (the fused kernels' own outputs meet far too few near-ties to show a lost correction step).
__device__ __forceinline__ float quant1_fast(float c, float step, float inv) {
  const float q0 = c * inv;
  const float r = __builtin_fmaf(-q0, step, c);
  float q = __builtin_fmaf(r, inv, q0);
  q = __builtin_truncf(q + __builtin_copysignf(0.49999997f, q0));
  return q * step;
}

// Two coefficients of one tile at a time: the same five steps as v_pk_mul_f32 / v_pk_fma_f32 / v_pk_add_f32, which issue
// like one f32 instruction on gfx950 (copysign and trunc have no packed form) -- 9 instructions per pair instead of 14.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 quant2_fast(f32x2 c, float step, float inv) {
  const f32x2 s2 = {step, step}, i2 = {inv, inv};
  const f32x2 q0 = c * i2;
  const f32x2 r = __builtin_elementwise_fma(-q0, s2, c);
  f32x2 q = __builtin_elementwise_fma(r, i2, q0);
  const f32x2 h = {__builtin_copysignf(0.49999997f, q0.x), __builtin_copysignf(0.49999997f, q0.y)};
  q = q + h;
  q = f32x2{__builtin_truncf(q.x), __builtin_truncf(q.y)};
  return q * s2;
}

// quant2_fast up to its last line: the integer level q itself (an f32 holding an integer, possibly -0.0), for the kernel that
// packs levels instead of storing q * step (dct_pack.hip).  Every level a coefficient can reach here has q * step exact in f32
// (|q * step| <= |c| + step / 2 < 2^24), so std::round((q * step) / step) -- what the pack reads back from the planes -- is q.
__device__ __forceinline__ f32x2 quant2_level(f32x2 c, float step, float inv) {
  const f32x2 s2 = {step, step}, i2 = {inv, inv};
  const f32x2 q0 = c * i2;
  const f32x2 r = __builtin_elementwise_fma(-q0, s2, c);
  f32x2 q = __builtin_elementwise_fma(r, i2, q0);
  const f32x2 h = {__builtin_copysignf(0.49999997f, q0.x), __builtin_copysignf(0.49999997f, q0.y)};
  q = q + h;
  return f32x2{__builtin_truncf(q.x), __builtin_truncf(q.y)};
}

}  // namespace svc
