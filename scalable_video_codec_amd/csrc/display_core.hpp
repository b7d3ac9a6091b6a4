// display_core.hpp -- the decoder's display pass, shared by every decoder that ends in a picture (levels.hip from the compact
// stream, records.hip from the wire records): the reference's upscaled_frame /= 255, cv::resize(INTER_LINEAR) to the display size and
// imshow's float -> u8 (libs/decoder.cpp:209-210; the statement is in include/svc_hip.h).  One definition, so that both decoders show
// the same bytes.  The kernel has internal linkage: each translation unit that includes this header gets its own copy.
#pragma once

#include "svc_common.hpp"

namespace svc {
namespace {

constexpr uint32_t kDisplayThreads = 256;  // the display pass's workgroup: one display pixel per lane, row blocks of 256 pixels

// source index s and weight a of s + 1 for destination index d (half-pixel centres): fx = (d + 0.5) * n_src / n_dst - 0.5
// = ((2d + 1) n_src - n_dst) / (2 n_dst), >= 0 since n_src >= n_dst; from integers, the weight rounded once to f32
__device__ __forceinline__ void src_coord(uint32_t d, uint32_t n_src, uint32_t n_dst, uint32_t* s, float* a) {
  const uint32_t num = (2 * d + 1) * n_src - n_dst, den = 2 * n_dst;  // < 2^32: sides are at most 32768
  const uint32_t q = num / den;
  if (q >= n_src - 1) { *s = n_src - 1; *a = 0.f; return; }
  *s = q;
  *a = (float)((double)(num - q * den) / (double)den);
}

// display pass: v = rec / 255, bilinear (horizontal, then vertical, f32), saturate_u8(rint(255 v)).  A frame that failed its checks
// is zeros in rec and so zeros here.  Grid (row blocks of 256 pixels, display rows, frames).
__global__ __launch_bounds__(256) void display_kernel(const float* __restrict__ rec, uint8_t* __restrict__ out, uint32_t w, uint32_t h,
                                                      uint32_t dw, uint32_t dh) {
  const uint32_t dx = blockIdx.x * kDisplayThreads + threadIdx.x, dy = blockIdx.y, f = blockIdx.z;
  if (dx >= dw) return;
  uint32_t sx, sy;
  float ax, ay;
  src_coord(dx, w, dw, &sx, &ax);
  src_coord(dy, h, dh, &sy, &ay);
  const uint32_t sx1 = min(sx + 1, w - 1), sy1 = min(sy + 1, h - 1);
  const float* r0 = rec + ((size_t)f * h + sy) * w * 3;
  const float* r1 = rec + ((size_t)f * h + sy1) * w * 3;
  uint8_t* p = out + (((size_t)f * dh + dy) * dw + dx) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v00 = r0[sx * 3 + c] / 255.f, v01 = r0[sx1 * 3 + c] / 255.f;
    const float v10 = r1[sx * 3 + c] / 255.f, v11 = r1[sx1 * 3 + c] / 255.f;
    const float top = v00 * (1.f - ax) + v01 * ax, bot = v10 * (1.f - ax) + v11 * ax;
    const float q = rintf(255.f * (top * (1.f - ay) + bot * ay));
    p[c] = (uint8_t)(q < 0.f ? 0.f : (q > 255.f ? 255.f : q));
  }
}

// The checks and the closing that every decoder with a display pass shares, each with the entry point's name in its message.
// A decoder's steps, then its display size: 0 x 0 = no display pass (*display = false), else within the padded frame (the pass only
// shrinks).
inline int validate_steps_display(const char* what, uint32_t fg_step, uint32_t bg_step, uint32_t dw, uint32_t dh, uint32_t w, uint32_t h,
                                  bool* display) {
  SVC_REQUIRE(fg_step > 0 && bg_step > 0, "%s: quant steps must be positive (libs/decoder.cpp:35-47)", what);
  *display = dw != 0 || dh != 0;
  SVC_REQUIRE(!*display || (dw >= 1 && dw <= w && dh >= 1 && dh <= h), "%s: display %ux%u must lie within 1x1 .. %ux%u (the padded frame)",
              what, dw, dh, w, h);
  return SVC_OK;
}

inline int validate_display_buffer(const char* what, bool display, const uint8_t* d_display) {
  SVC_REQUIRE(display == (d_display != nullptr), "%s: a display buffer goes with a display size, and only with one", what);
  return SVC_OK;
}

// after the launch of a decoder's last pass before the picture: its check, then the display pass if there is one
inline int finish_with_display(const char* what, const char* pass, bool display, const float* d_rec, uint8_t* d_display, uint32_t n_frames,
                               uint32_t w, uint32_t h, uint32_t dw, uint32_t dh, hipStream_t s) {
  const int rc = check_launch(what, pass);
  if (rc || !display) return rc;
  hipLaunchKernelGGL(display_kernel, dim3(div_up(dw, kDisplayThreads), dh, n_frames), dim3(kDisplayThreads), 0, s, d_rec, d_display, w, h,
                     dw, dh);
  return check_launch(what, "display");
}

}  // namespace
}  // namespace svc
