// stream_format.hpp -- the one native statement of the compact stream's frame formats: "SVCQ" (levels.hip packs, unpacks and
// decodes it) and its lossless coding "SVCE" (entropy.hip).  include/svc_hip.h has the tables; scalable_video_codec_amd/levels.py
// and entropy.py are the independent Python statements the tests compare the kernels against.
//
// The first part is plain C++ (host/stream_decoder.cpp reads the headers it is handed with it).  The second is for the kernel files,
// which include svc_common.hpp first: the checks of an SVCQ frame and of the entry points' arguments, the one statement of a
// workspace (Carver), and the steps every producer and consumer of the stream takes -- the scan of a frame's counts, a frame's offset in
// its batch, a frame's fixed part (header, types, padding), the store of a run of levels, the address of a mask word.
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
// two-layer decode reports its enhancement frame's code as kStEnhancement | code, 11 for one that does not belong to its base frame; the
// union reports its second stream's frame the same way, and 12 for a pair whose masks share a bit
enum : uint32_t {
  kStOk = 0, kStRange = 1, kStMagic = 2, kStVersion = 3, kStGeometry = 4, kStSize = 5, kStLevels = 6, kStStrayBits = 7,
  kStIndex = 8, kStChunk = 9, kStSvcqBytes = 10, kStLayer = 11, kStOverlap = 12, kStEnhancement = 0x100
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

// the two size checks every entry point makes after its limits; which = "output", "base output", "enhancement output", "destination"
inline int require_workspace(const char* what, uint64_t have, uint64_t need) {
  SVC_REQUIRE(have >= need, "%s: workspace of %llu B is smaller than the %llu B needed", what, (unsigned long long)have,
              (unsigned long long)need);
  return SVC_OK;
}
inline int require_capacity(const char* what, const char* which, uint64_t have, uint64_t need) {
  SVC_REQUIRE(have >= need, "%s: %s of %llu B is below the batch's worst case of %llu B", what, which, (unsigned long long)have,
              (unsigned long long)need);
  return SVC_OK;
}

// ---- workspaces ---------------------------------------------------------------------------------------------------------------------
//
// A workspace is stated once, as a function `layout(Carver&, sizes...)` that takes its arrays in order and returns the struct of their
// pointers.  carve() runs it on the caller's d_workspace, layout_bytes() on a null base, where the cursor's end is the size: the size
// an entry point reports and the pointers its kernels store through cannot disagree.
struct Carver {
  uintptr_t at;
  template <typename T>
  T* take(uint64_t count, bool align16 = true) {  // the next `count` T's; the cursor then moves on to a multiple of 16 B, or not
    T* const p = reinterpret_cast<T*>(at);
    at += align16 ? up16(sizeof(T) * count) : sizeof(T) * count;
    return p;
  }
};
template <typename F, typename... A>
auto carve(uint8_t* base, F layout, const A&... sizes) {
  Carver c{reinterpret_cast<uintptr_t>(base)};
  return layout(c, sizes...);
}
template <typename F, typename... A>
uint64_t layout_bytes(F layout, const A&... sizes) {
  Carver c{0};
  (void)layout(c, sizes...);
  return c.at;
}

// The drain of a batch of frames to pinned host memory (levels.hip), after the caller's geometry checks: capacity against `need`,
// then pointers, the destination's memory, and the launch.
int drain_to_host(const char* what, const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, void* host_dst,
                  uint64_t capacity, uint64_t need, void* stream);

// The frame offsets of a batch from its frames' sizes (levels.hip): one launch, a workgroup per job -- offsets[0 .. n] = the running
// sum of bytes[0 .. n), also stored to `copy` where that is not null.  Checked as the launch `what` "offsets".
struct OffsetsJob {
  const uint32_t* bytes;
  uint64_t *offsets, *copy;
};
int enqueue_frame_offsets(const char* what, uint32_t jobs, OffsetsJob job0, OffsetsJob job1, uint32_t n, void* stream);

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

// the first mask word of tile t of tile row `row` = plane * tiles_y + tile row, in the mask section at `section` (as bytes or dwords: a
// mask word is 8 B).  The pointer, not an index: from an index the compiler orders the multiplies of the kernels' address differently.
template <typename P>
__device__ __forceinline__ P* mask_words(P* section, uint64_t row, uint32_t tiles_x, uint64_t t, uint32_t words) {
  return section + (8 / sizeof(P)) * ((row * tiles_x + t) * words);
}

// The scan of count -> scan -> scatter, by a workgroup in trips of kThreads: store(i, carry + the sum of load(j) over j < i) for every
// i < count; returns carry + the sum of all.  The plain form reads src[i] and writes dst[i] (the same array: in place).
template <typename Load, typename Store>
__device__ __forceinline__ uint32_t scan_counts(uint32_t count, uint32_t carry, uint32_t* lds4, Load load, Store store) {
  for (uint32_t base = 0; base < count; base += kThreads) {
    const uint32_t i = base + threadIdx.x;
    uint32_t total;
    const uint32_t ex = block_exclusive_scan(i < count ? load(i) : 0u, lds4, &total);
    if (i < count) store(i, carry + ex);
    carry += total;
  }
  return carry;
}
__device__ __forceinline__ uint32_t scan_counts(const uint32_t* src, uint32_t* dst, uint32_t count, uint32_t carry, uint32_t* lds4) {
  return scan_counts(count, carry, lds4, [&](uint32_t i) { return src[i]; }, [&](uint32_t i, uint32_t v) { dst[i] = v; });
}

// Frame f's offset in its batch = the sizes of the frames before it (a batch is a few dozen frames: no kernel of its own).  Wave 0 sums
// them into *lds; the caller's next barrier hands the value to the workgroup.
__device__ __forceinline__ void frame_offset_to_lds(const uint32_t* frame_bytes, uint32_t f, uint64_t* lds) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (wave != 0) return;
  uint64_t s = 0;
  for (uint32_t i = lane; i < f; i += 64) s += frame_bytes[i];
  for (uint32_t off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
  if (lane == 0) *lds = s;
}

// A frame's header words 2 .. 12, in the header's order; word k of the header they make
struct FrameHead {
  uint32_t w, h, bw, bh, mvbw, mvbh, fg, bg, levels, inexact, bytes;
};
__device__ __forceinline__ uint32_t header_word(const FrameHead& h, uint32_t k) {
  const uint32_t v[kHeaderWords] = {kMagicQ, kVersion, h.w, h.h, h.bw, h.bh, h.mvbw, h.mvbh, h.fg, h.bg, h.levels, h.inexact, h.bytes, 0, 0, 0};
  return v[k];
}

// A frame's fixed part, by a workgroup of `threads`: the header, the types, the zero pad behind the levels and, where `offsets` is not
// null (a frame whose offset its own workgroup summed), offsets[f + 1].
__device__ __forceinline__ void write_frame_edges(uint8_t* frame, const FrameHead& h, const uint32_t* types, uint32_t mvb,
                                                  uint64_t levels_off, uint32_t threads, uint64_t* offsets, uint32_t f, uint64_t frame_off) {
  if (threadIdx.x < kHeaderWords) reinterpret_cast<uint32_t*>(frame)[threadIdx.x] = header_word(h, threadIdx.x);
  uint32_t* tdst = reinterpret_cast<uint32_t*>(frame + kHeaderBytes);
  for (uint32_t i = threadIdx.x; i < mvb; i += threads) tdst[i] = types[i];
  const uint64_t used = levels_off + 2ull * h.levels;
  for (uint64_t i = used + threadIdx.x; i < h.bytes; i += threads) frame[i] = 0;
  if (offsets && threadIdx.x == 0) {
    offsets[f + 1] = frame_off + h.bytes;
    if (f == 0) offsets[0] = 0;
  }
}

// A wave stores a run of cnt int16 levels to dst, a 2-byte aligned place in a frame: aligned dwords, and 16 bits at an odd end, where
// the dword belongs half to the neighbouring run (whose wave stores its own half)
__device__ __forceinline__ void store_level_run(const uint16_t* src, uint32_t cnt, uint16_t* dst) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t head = cnt != 0 && (reinterpret_cast<uintptr_t>(dst) & 2u) ? 1u : 0u, body = (cnt - head) / 2;
  if (head && lane == 0) dst[0] = src[0];
  uint32_t* d32 = reinterpret_cast<uint32_t*>(dst + head);
  for (uint32_t k = lane; k < body; k += 64) d32[k] = (uint32_t)src[head + 2 * k] | ((uint32_t)src[head + 2 * k + 1] << 16);
  if (((cnt - head) & 1u) && lane == 0) dst[cnt - 1] = src[cnt - 1];
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
