// stream_format.hpp -- the one native statement of the compact stream's frame formats: "SVCQ" (levels.hip packs, unpacks and
// decodes it) and its lossless coding "SVCE" (entropy.hip).  include/svc_hip.h has the tables; scalable_video_codec_amd/levels.py
// and entropy.py are the independent Python statements the tests compare the kernels against.
//
// The first part is plain C++ (host/stream_decoder.cpp reads the headers it is handed with it).  The second is for the kernel files,
// which include svc_common.hpp first: the checks of an SVCQ frame and of the entry points' arguments, and the wave / workgroup
// primitives both files use.
#pragma once

#include <cstdint>

namespace svc {

constexpr uint32_t kMagicQ = 0x51435653u;  // "SVCQ"
constexpr uint32_t kMagicE = 0x45435653u;  // "SVCE"
constexpr uint32_t kVersion = 1;           // of both
constexpr uint32_t kHeaderBytes = 64;      // 16 x u32, then the types section
constexpr uint32_t kMaxTileCoeffs = 4096;  // a tile fits one group's LDS; the Dct's largest tile is 64 x 64

// header words.  0 .. 11 mean the same in both formats (an SVCE header is its SVCQ frame's with words 0 and 12 .. 15 replaced)
enum : uint32_t {
  kHMagic = 0, kHVersion = 1, kHWidth = 2, kHHeight = 3, kHTileW = 4, kHTileH = 5, kHMvW = 6, kHMvH = 7,
  kHFgStep = 8, kHBgStep = 9,     // the encoder's quant steps
  kHLevels = 10, kHInexact = 11,  // non-zero levels of the frame; coefficients the quantiser did not reproduce exactly
  kHBytes = 12,                   // this frame's bytes, padding included
  kQReserved = 13,                // SVCQ: 13 .. 15 are zero
  kESvcqBytes = 13, kEChunkTiles = 14, kETypesBytes = 15,  // SVCE: the SVCQ frame's bytes, tiles per chunk, the types section's bytes
  kHeaderWords = 16
};

// per-frame status of the unpack / decode (1 .. 7, also the entropy encoder's view of its SVCQ input) and of the entropy decoder; the
// two-layer decode reports its enhancement frame's code as kStEnhancement | code, 11 for one that does not belong to its base frame
enum : uint32_t {
  kStOk = 0, kStRange = 1, kStMagic = 2, kStVersion = 3, kStGeometry = 4, kStSize = 5, kStLevels = 6, kStStrayBits = 7,
  kStIndex = 8, kStChunk = 9, kStSvcqBytes = 10, kStLayer = 11, kStEnhancement = 0x100
};

constexpr uint64_t up16(uint64_t v) { return (v + 15) & ~(uint64_t)15; }  // constexpr: host and device

// One SVCQ frame (little-endian, 16-byte aligned, frames back to back):
//   header 16 x u32 | types [mv blocks] u32 | masks [3][tiles_y][tiles_x][words] u64 | levels [level_count] i16 | zero pad to 16
struct FrameLayout {
  uint32_t mfw, mvb;                 // MV blocks per row, per frame
  uint32_t tiles_x, tiles_y, words;  // words = 64-coefficient mask words per tile
  uint64_t masks_off, levels_off;    // byte offsets inside a frame
  uint64_t max_bytes;                // the frame when every coefficient is a level
};

// for a geometry that passed validate_geom (the sides divide)
inline FrameLayout frame_layout(uint32_t w, uint32_t h, uint32_t bw, uint32_t bh, uint32_t mvbw, uint32_t mvbh) {
  FrameLayout l{};
  l.mfw = w / mvbw; l.mvb = l.mfw * (h / mvbh);
  l.tiles_x = w / bw; l.tiles_y = h / bh;
  l.words = (bw * bh + 63) / 64;
  l.masks_off = kHeaderBytes + 4ull * l.mvb;
  l.levels_off = l.masks_off + 8ull * 3 * l.tiles_x * l.tiles_y * l.words;
  l.max_bytes = up16(l.levels_off + 2ull * 3 * w * h);
  return l;
}

#if defined(__HIPCC__) && defined(SVC_REQUIRE)  // a kernel file: svc_common.hpp (fail, SVC_REQUIRE, hip_runtime.h) came first

constexpr uint32_t kThreads = 256;  // the workgroup of every kernel of the two streams

// ---- arguments of the entry points ------------------------------------------------------------------------------------------------

inline int validate_geom(const char* what, uint32_t w, uint32_t h, uint32_t bw, uint32_t bh, uint32_t mvbw, uint32_t mvbh) {
  SVC_REQUIRE(w > 0 && h > 0 && bw > 0 && bh > 0, "%s: frame and tile sides must be positive", what);
  SVC_REQUIRE(w % bw == 0 && h % bh == 0, "%s: frame %ux%u not divisible by tile %ux%u", what, w, h, bw, bh);
  SVC_REQUIRE(mvbw > 0 && mvbh > 0 && mvbw % bw == 0 && mvbh % bh == 0 && w % mvbw == 0 && h % mvbh == 0,
              "%s: MV block %ux%u must be a multiple of the tile %ux%u and divide the frame", what, mvbw, mvbh, bw, bh);
  return SVC_OK;
}

// what this build's kernels and the formats' fields hold; max_frame_bytes = the caller's worst case (SVCQ's or SVCE's), read only
// for a tile within the limit
inline int validate_limits(const char* what, uint32_t n, uint32_t w, uint32_t h, uint32_t bw, uint32_t bh, uint64_t max_frame_bytes) {
  if ((uint64_t)bw * bh > kMaxTileCoeffs) return fail(SVC_ERR_UNSUPPORTED, "%s: tiles above %u coefficients", what, kMaxTileCoeffs);
  if (n > 65535) return fail(SVC_ERR_UNSUPPORTED, "%s: more than 65535 frames in one call", what);
  if (max_frame_bytes > 0xFFFFFFFFull)
    return fail(SVC_ERR_UNSUPPORTED, "%s: a frame of %ux%u could exceed the u32 frame_bytes field", what, w, h);
  return SVC_OK;
}

// decode: what the reconstruction kernels take (square 8x8 or 16x16 transform blocks and a width of whole 16-pixel segments, as
// svc_hip_decode_frames; sides up to 32768 for the display pass's u32 coordinates), after the format's own geometry
inline int validate_decode_geom(const char* what, uint32_t w, uint32_t h, uint32_t bw, uint32_t bh, uint32_t mvbw, uint32_t mvbh) {
  const int rc = validate_geom(what, w, h, bw, bh, mvbw, mvbh);
  if (rc) return rc;
  if (bw != bh || (bw != 8 && bw != 16))
    return fail(SVC_ERR_UNSUPPORTED, "%s: transform block %ux%u (supported: 8x8, 16x16)", what, bw, bh);
  if (w % 16 != 0) return fail(SVC_ERR_UNSUPPORTED, "%s: frame width %u is not a multiple of 16", what, w);
  if (w > 32768 || h > 32768) return fail(SVC_ERR_UNSUPPORTED, "%s: frame %ux%u above 32768 on a side", what, w, h);
  return SVC_OK;
}

// The drain of a batch of frames to pinned host memory (levels.hip), after the caller's geometry checks: capacity against `need`,
// then pointers, the destination's memory, and the launch.
int drain_to_host(const char* what, const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, void* host_dst,
                  uint64_t capacity, uint64_t need, void* stream);

// ---- device: wave and workgroup primitives ------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  for (uint32_t off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

__device__ __forceinline__ uint32_t wave_exclusive_scan(uint32_t v) {
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t x = v;
  for (uint32_t off = 1; off < 64; off <<= 1) {
    const uint32_t y = __shfl_up(x, off, 64);
    if (lane >= off) x += y;
  }
  return x - v;
}

// exclusive scan of v over the workgroup's 256 threads; *total gets the sum
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* lds4, uint32_t* total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t ex = wave_exclusive_scan(v);
  if (lane == 63) lds4[wave] = ex + v;
  __syncthreads();
  uint32_t base = 0, sum = 0;
  for (uint32_t i = 0; i < kThreads / 64; ++i) {
    const uint32_t s = lds4[i];
    if (i < wave) base += s;
    sum += s;
  }
  __syncthreads();
  *total = sum;
  return base + ex;
}

// a mask word (u64 from two u32: the masks are only 4-byte aligned when the MV block count is odd)
__device__ __forceinline__ uint64_t load_mask(const void* p) {
  const uint32_t* q = static_cast<const uint32_t*>(p);
  return (uint64_t)q[0] | ((uint64_t)q[1] << 32);
}
__device__ __forceinline__ void store_mask(void* p, uint64_t m) {
  uint32_t* q = static_cast<uint32_t*>(p);
  q[0] = (uint32_t)m;
  q[1] = (uint32_t)(m >> 32);
}

// ---- device: is SVCQ frame f well formed for geometry g inside a stream of stream_bytes? ----------------------------------------------
//
// Returns a status (1 .. 5), fills *off and, from the magic on, *hdr; reads nothing outside [o, e).  G = the caller's Geom (w, h, bw,
// bh, mvbw, mvbh, levels_off).  LOSSLESS = false is the unpack's check, before its masks.  LOSSLESS = true adds what a lossless coding
// needs, each where its stage is: reserved words zero (with the geometry, so before the size), the exact size and zero padding.
template <bool LOSSLESS, typename G>
__device__ uint32_t check_svcq(const G& g, const uint8_t* __restrict__ in, uint64_t stream_bytes, const uint64_t* __restrict__ offsets,
                               uint32_t f, uint64_t* off, const uint32_t** hdr) {
  const uint64_t o = offsets[f], e = offsets[f + 1];
  *off = o;
  if (o % 16 != 0 || o > e || e > stream_bytes || e - o < kHeaderBytes) return kStRange;
  const uint32_t* h = reinterpret_cast<const uint32_t*>(in + o);
  *hdr = h;
  if (h[kHMagic] != kMagicQ) return kStMagic;
  if (h[kHVersion] != kVersion) return kStVersion;
  if (h[kHWidth] != g.w || h[kHHeight] != g.h || h[kHTileW] != g.bw || h[kHTileH] != g.bh || h[kHMvW] != g.mvbw || h[kHMvH] != g.mvbh ||
      h[kHFgStep] == 0 || h[kHBgStep] == 0 ||
      (LOSSLESS && (h[kQReserved] != 0 || h[kQReserved + 1] != 0 || h[kQReserved + 2] != 0)))
    return kStGeometry;
  const uint64_t used = g.levels_off + 2ull * h[kHLevels];
  if (h[kHBytes] != e - o || (LOSSLESS ? h[kHBytes] != up16(used) : used > h[kHBytes])) return kStSize;
  if (LOSSLESS)
    for (uint64_t i = used; i < h[kHBytes]; ++i)
      if (in[o + i] != 0) return kStSize;
  return kStOk;
}

#endif  // kernel files

}  // namespace svc
