// records.hip -- the headless decoder of the reference's own wire stream: Header + one record per transform tile (libs/codec.hpp:8-17,
// libs/encoder.cpp:222-269), each a u32 type word and 3 x N x N RAW f32 coefficients.  The reference quantises in the decoder
// (libs/decoder.cpp:128-149), so this stream is the gaze-scalable one: inside the frame's gaze rectangle a tile is decoded at step 1.
//
// One kernel from the records in HBM straight to the f32 B,G,R reconstruction at the padded size (DecodeBlock over every tile, the
// arithmetic of idct_core.hpp), then optionally the display pass of display_core.hpp.  No f32 planes in between.
//
// Work split: a workgroup owns a STRETCH = up to kTiles adjacent tiles of one tile row of one frame (2048 coefficients per plane, the
// group size of levels.hip).  A tile row is one contiguous byte range of records, so the stretch is too: it is staged into LDS with
// coalesced dword loads (records are only 4-byte aligned: 772 B per 8x8 record, 3 076 B per 16x16), then thread (t, j) takes row j
// of tile t's coefficients from LDS through the row and column passes of idct_core.hpp with the tile's step and, after the third
// plane, stores its column's interleaved B,G,R pixels.  d_rec has the bits of parsing the records into planes +
// svc_hip_decode_frames with mv_block = block.
#include "display_core.hpp"
#include "idct_core.hpp"

#include <algorithm>

namespace svc {
namespace {

constexpr uint32_t kWireHeaderBytes = 32;  // sizeof(Header), libs/codec.hpp:8-17

template <int N> struct RecGeom {
  static constexpr uint32_t kTiles = 2048 / (N * N);     // tiles per stretch: 32 at 8x8, 8 at 16x16
  static constexpr uint32_t kThreads = kTiles * N;       // one thread per (tile, coefficient row): 256 at 8x8, 128 at 16x16
  static constexpr uint32_t kRecDw = 1 + 3 * N * N;      // dwords per record: the type word, then B, G, R row-major
};

struct RecordsArgs {
  const uint8_t* records;  // frame f at records + f * stride
  uint64_t stride;
  const uint32_t* gaze;    // [n][4] x, y, w, h in padded coordinates, or null
  float* rec;              // [n][h][w][3]
  uint32_t w, h, tiles_x, gx, emit_rows;  // gx = stretches per tile row; emit_rows = tile rows the stream holds
  float fg, bg;            // the decoder's steps
};

// Grid (gx * h / N stretches, frames).  A stretch in a tile row the stream does not hold (emit_frame_h < frame_h) stores zeros.
template <int N>
__global__ __launch_bounds__(RecGeom<N>::kThreads) void decode_records_kernel(RecordsArgs a) {
  using G = RecGeom<N>;
  __shared__ __attribute__((aligned(16))) uint32_t stage[G::kTiles * G::kRecDw];    // 24.1 KiB at 8x8, 24.0 KiB at 16x16
  __shared__ __attribute__((aligned(16))) double rows[G::kTiles * N * (N + 1)];    // the slab of idct_core.hpp's passes
  const uint32_t s = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
  const uint32_t ty = s / a.gx, t0 = (s - ty * a.gx) * G::kTiles;
  const uint32_t nt = min(G::kTiles, a.tiles_x - t0);
  const uint32_t t = tid / N, j = tid - t * N;
  const bool active = t < nt;
  float* dst = a.rec + (((size_t)f * a.h + ty * N) * a.w + (t0 + t) * N + j) * 3;  // a wave stores 64 adjacent pixels per row
  if (ty >= a.emit_rows) {  // uniform over the workgroup
    const float zeros[3][N] = {};
    if (active) store_bgr_column<N>(dst, a.w, zeros);
    return;
  }
  // the stretch: nt whole records, contiguous, 4-byte aligned
  const uint32_t* src = reinterpret_cast<const uint32_t*>(a.records + f * a.stride) + ((size_t)ty * a.tiles_x + t0) * G::kRecDw;
  const uint32_t n_dw = nt * G::kRecDw;
  for (uint32_t i = tid; i < n_dw; i += G::kThreads) stage[i] = src[i];
  __syncthreads();
  float dec = 1.f;
  if (active) {
    const uint32_t type = stage[t * G::kRecDw];  // any non-zero word is foreground (libs/decoder.cpp:130-135, codec.hpp:6)
    dec = gazed(a.gaze, f, (t0 + t) * N, ty * N) ? 1.f : (type == 0 ? a.bg : a.fg);
  }
  float out[3][N];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (active) {
      const float* coef = reinterpret_cast<const float*>(stage + t * G::kRecDw + 1 + c * N * N + j * N);
      invert_row<N>(coef, dec, rows, t, j);
    }
    __syncthreads();
    if (active) invert_column<N>(rows, t, j, out[c]);
    __syncthreads();  // the next plane reuses rows
  }
  if (!active) return;
  store_bgr_column<N>(dst, a.w, out);
}

// what the reconstruction kernel takes, as svc_hip_decode_frames (square 8x8 or 16x16 tiles, whole 16-pixel segments), sides up to
// 32768 for the display pass's u32 coordinates, and the rows of the padded frame the stream holds
int validate_records_geom(uint32_t w, uint32_t h, uint32_t block, uint32_t emit_h) {
  if (block != 8 && block != 16) return fail(SVC_ERR_UNSUPPORTED, "decode_records: transform block %u (supported: 8x8, 16x16)", block);
  SVC_REQUIRE(w > 0 && h > 0 && h % block == 0, "decode_records: frame %ux%u not divisible by block %u", w, h, block);
  if (w % 16 != 0) return fail(SVC_ERR_UNSUPPORTED, "decode_records: frame width %u is not a multiple of 16", w);
  if (w > 32768 || h > 32768) return fail(SVC_ERR_UNSUPPORTED, "decode_records: frame %ux%u above 32768 on a side", w, h);
  SVC_REQUIRE(emit_h >= 1 && emit_h <= h, "decode_records: emit_frame_h %u outside [1, %u]", emit_h, h);
  return SVC_OK;
}

// does a stream of `bytes` hold exactly `count` frames of `frame_bytes` after the header?  (no product: it may overflow u64)
bool holds(uint64_t bytes, uint32_t count, uint64_t frame_bytes) {
  if (bytes < kWireHeaderBytes) return false;
  const uint64_t body = bytes - kWireHeaderBytes;
  if (count == 0 || frame_bytes == 0) return body == 0;
  return body % frame_bytes == 0 && body / frame_bytes == count;
}

}  // namespace
}  // namespace svc

using namespace svc;

extern "C" {

int svc_hip_decode_records_frames(const uint8_t* d_records, uint64_t records_stride_bytes, uint32_t n_frames, uint32_t frame_w,
                                  uint32_t frame_h, uint32_t block, uint32_t emit_frame_h, uint32_t fg_step, uint32_t bg_step,
                                  const uint32_t* d_gaze, float* d_rec, uint8_t* d_display, uint32_t display_w, uint32_t display_h,
                                  void* stream) {
  int rc = validate_records_geom(frame_w, frame_h, block, emit_frame_h);
  if (rc) return rc;
  bool display;
  if ((rc = validate_steps_display("decode_records", fg_step, bg_step, display_w, display_h, frame_w, frame_h, &display))) return rc;
  const uint64_t per = svc_hip_serialized_frame_bytes(frame_w, emit_frame_h, block, block);
  SVC_REQUIRE(records_stride_bytes % 4 == 0 && records_stride_bytes >= per,
              "decode_records: records stride %llu must be a multiple of 4 and at least one frame's %llu B",
              (unsigned long long)records_stride_bytes, (unsigned long long)per);
  if (n_frames > 65535) return fail(SVC_ERR_UNSUPPORTED, "decode_records: more than 65535 frames in one call");
  if (n_frames == 0) return SVC_OK;
  SVC_REQUIRE(d_records && d_rec, "decode_records: null pointer");
  if ((rc = validate_display_buffer("decode_records", display, d_display))) return rc;
  SVC_REQUIRE(aligned(d_records, 4) && aligned(d_rec, 4) && aligned(d_gaze, 4), "decode_records: records, output and gaze must be 4-byte aligned");
  RecordsArgs a;
  a.records = d_records; a.stride = records_stride_bytes; a.gaze = d_gaze; a.rec = d_rec;
  a.w = frame_w; a.h = frame_h; a.tiles_x = frame_w / block; a.emit_rows = div_up(emit_frame_h, block);
  a.fg = (float)fg_step; a.bg = (float)bg_step;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (block == 8) {
    a.gx = div_up(a.tiles_x, RecGeom<8>::kTiles);
    hipLaunchKernelGGL(decode_records_kernel<8>, dim3(a.gx * (frame_h / 8), n_frames), dim3(RecGeom<8>::kThreads), 0, s, a);
  } else {
    a.gx = div_up(a.tiles_x, RecGeom<16>::kTiles);
    hipLaunchKernelGGL(decode_records_kernel<16>, dim3(a.gx * (frame_h / 16), n_frames), dim3(RecGeom<16>::kThreads), 0, s, a);
  }
  return finish_with_display("decode_records", "reconstruction", display, d_rec, d_display, n_frames, frame_w, frame_h, display_w, display_h, s);
}

int svc_hip_wire_layout(const svc_wire_header* hdr, uint64_t stream_bytes, uint32_t* emit_frame_h, uint64_t* frame_bytes) {
  SVC_REQUIRE(hdr && emit_frame_h && frame_bytes, "wire_layout: null pointer");
  const svc_wire_header& h = *hdr;
  SVC_REQUIRE(h.channel_count == 3, "wire_layout: channel_count %u (the stream's records hold B, G, R: 3)", h.channel_count);
  const uint32_t b = h.transform_block_w;
  if (b != h.transform_block_h)
    return fail(SVC_ERR_UNSUPPORTED, "wire_layout: non-square transform blocks %ux%u (supported: 8x8, 16x16)", h.transform_block_w,
                h.transform_block_h);
  if (b != 8 && b != 16) return fail(SVC_ERR_UNSUPPORTED, "wire_layout: transform block %ux%u (supported: 8x8, 16x16)", b, b);
  SVC_REQUIRE(h.frame_w > 0 && h.frame_h > 0, "wire_layout: empty frame %ux%u", h.frame_w, h.frame_h);
  const uint64_t pw64 = (uint64_t)h.frame_w + h.frame_excess_w, ph64 = (uint64_t)h.frame_h + h.frame_excess_h;
  if (pw64 > 32768 || ph64 > 32768)
    return fail(SVC_ERR_UNSUPPORTED, "wire_layout: padded frame %llux%llu above 32768 on a side", (unsigned long long)pw64,
                (unsigned long long)ph64);
  const uint32_t pw = (uint32_t)pw64, ph = (uint32_t)ph64;
  if (pw % 16 != 0 || ph % b != 0)
    return fail(SVC_ERR_UNSUPPORTED, "wire_layout: padded frame %ux%u (the decoder takes widths of whole 16-pixel segments and whole tile rows)",
                pw, ph);
  // the decoder's reading: the padded tile grid (libs/decoder.cpp:185-186); the reference encoder's: its unpadded tile loops
  // (libs/encoder.cpp:647-650), which only differ in the tile rows when the width needs no padding
  const uint64_t dec_bytes = svc_hip_serialized_frame_bytes(pw, ph, b, b);
  const uint64_t enc_bytes = svc_hip_serialized_frame_bytes(h.frame_w, h.frame_h, b, b);
  if (holds(stream_bytes, h.frame_count, dec_bytes)) {
    *emit_frame_h = ph; *frame_bytes = dec_bytes;
    return SVC_OK;
  }
  if (holds(stream_bytes, h.frame_count, enc_bytes)) {
    SVC_REQUIRE(h.frame_excess_w == 0,
                "wire_layout: %llu B = %u frames of the reference encoder's unpadded %ux%u tile loops, but with a padded width "
                "(excess %u) its unpadded row stride (libs/encoder.cpp:258) has scrambled the coefficients: not decodable",
                (unsigned long long)stream_bytes, h.frame_count, h.frame_w, h.frame_h, h.frame_excess_w);
    *emit_frame_h = h.frame_h; *frame_bytes = enc_bytes;
    return SVC_OK;
  }
  return fail(SVC_ERR_INVALID_ARG,
              "wire_layout: a stream of %llu B is truncated or overlong: %u frames take %llu B (the decoder's padded %ux%u grid) or "
              "%llu B (the encoder's unpadded %ux%u loops) after the %u-byte header",
              (unsigned long long)stream_bytes, h.frame_count, (unsigned long long)((uint64_t)h.frame_count * dec_bytes), pw, ph,
              (unsigned long long)((uint64_t)h.frame_count * enc_bytes), h.frame_w, h.frame_h, kWireHeaderBytes);
}

}  // extern "C"
