// encode_geometry.hpp -- what svc::ClipEncoder and svc::StreamEncoder derive from a configuration the same way: the padded frame
// and its motion field, and the RANSAC draws of a run of frame pairs.  tests/test_gpu_stream.py ("stream equals resident, whatever
// the batch size") holds because both drivers take them from here.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "svc_hip.h"

namespace svc {
namespace host __attribute__((visibility("hidden"))) {

// libs/math.hpp:276-283 (ClosestLargerDivisible): smallest value >= dim divisible by both
inline uint32_t ClosestLargerDivisible(uint32_t dim, uint32_t a, uint32_t b) {
  while (dim % a != 0 || dim % b != 0) ++dim;
  return dim;
}

struct EncodeGeometry {
  uint32_t pw = 0, ph = 0;    // padded frame
  uint32_t mfw = 0, mfh = 0;  // its field of MV blocks
  uint32_t blocks = 0;
  uint64_t pyr_stride = 0;    // bytes from one frame's luma pyramid to the next
  uint64_t frame_bytes = 0;   // one padded B,G,R frame
  uint64_t plane_elems = 0;   // one coefficient plane
  EncodeGeometry() = default;
  // the sides must be non-zero, levels in 1..16 (the drivers check their configuration first)
  EncodeGeometry(uint32_t width, uint32_t height, uint32_t levels, uint32_t mv_w, uint32_t mv_h) {
    const uint32_t f = 1u << (levels - 1);
    pw = ClosestLargerDivisible(width, mv_w, f);  // libs/encoder.cpp:164-168
    ph = ClosestLargerDivisible(height, mv_h, f);
    mfw = pw / mv_w; mfh = ph / mv_h; blocks = mfw * mfh;
    pyr_stride = (svc_hip_pyramid_bytes(pw, ph, levels) + 255) / 256 * 256;  // the kernels ask for 16-byte aligned pyramids
    frame_bytes = (uint64_t)pw * ph * 3;
    plane_elems = (uint64_t)pw * ph;
  }
};

inline uint32_t Hash32(uint64_t x) {  // the harness's stateless mixer (scalable_video_codec_amd/synth.py:hash32)
  uint32_t v = (uint32_t)x;
  v ^= v >> 16; v *= 0x7FEB352Du;
  v ^= v >> 15; v *= 0x846CA68Bu;
  v ^= v >> 16;
  return v;
}
constexpr uint64_t kHashStride = 0x9E3779B1ull;  // spreads consecutive indices over Hash32's input

// RANSAC draws of `pairs` consecutive frame pairs from clip-wide pair `first_pair` on: `iters` x `subset_sz` block indices per pair,
// distinct within an iteration, a function of (seed, clip-wide pair, iteration) only -- so a clip encodes the same whatever the
// batch or shard it is cut into.  The Python statement of the same generator is pipeline.ransac_samples.
inline void FillRansacDraws(uint32_t* dst, uint64_t first_pair, size_t pairs, uint32_t iters, uint32_t subset_sz, uint32_t blocks,
                            uint64_t seed) {
  const uint32_t div = std::max<uint32_t>(1, (blocks - 1) / std::max<uint32_t>(1, subset_sz));
  for (size_t q = 0; q < pairs * iters; ++q) {
    const uint64_t idx = first_pair * iters + q;
    const uint32_t first = Hash32(idx * kHashStride + seed) % blocks;
    const uint32_t step = 1 + Hash32(idx * 0x85EBCA6Bull + seed + 1) % div;
    for (uint32_t j = 0; j < subset_sz; ++j) dst[q * subset_sz + j] = (uint32_t)(((uint64_t)first + (uint64_t)step * j) % blocks);
  }
}

}  // namespace host
}  // namespace svc
