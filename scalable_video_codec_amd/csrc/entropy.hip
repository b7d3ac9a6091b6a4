// entropy.hip -- lossless coding of the compact stream: "SVCQ" frames <-> "SVCE" frames (format version 1).
//
// include/svc_hip.h states the format and stream_format.hpp its header words, its statuses and the SVCQ side (layout, frame check);
// scalable_video_codec_amd/entropy.py is its executable statement and writes the same bytes.
// A frame's levels are cut into CHUNKS (one plane, one tile row, up to chunk_tiles adjacent tiles, in the order of SVCQ's levels);
// each chunk is coded on its own, with Exp-Golomb codes whose parameters the encoder picks per chunk, or copied raw when that is
// smaller.  An index of (bytes, levels) per chunk makes every chunk independently decodable.
//
// encode, following the count / scan / scatter of levels.hip:
//   count    one wave per chunk: the popcount of its masks (and mask bits past the tile)
//   scan     one workgroup per frame: the SVCQ frame's checks -> status; chunk level offsets; the types section's size
//   lengths  one wave per chunk, one lane per tile: the code lengths for every k, the choice of k and of raw
//   layout   one workgroup per frame: chunk byte offsets, the frame's size; then the frame offsets (levels.hip: enqueue_frame_offsets)
//   scatter  one wave per chunk: codewords ORed into LDS words, then written out bytewise (coalesced); raw chunks copied
//   frame    one workgroup per frame: header, types section, index, padding (a failed frame: 64 zero bytes)
// decode:
//   check    one workgroup per frame: header and index against each other -> status; chunk byte and level offsets
//   offsets  one workgroup: SVCQ frame offsets (the same kernel)
//   chunks   one lane per chunk: serial Exp-Golomb decoding (a chunk is serial by design), every read clamped to the frame
//   frame    one workgroup per frame: SVCQ header, types, padding, or zeros for a frame that failed
// fused decode (svc_hip_decode_entropy_frames), without the SVCQ frames:
//   check    as above
//   decode   one workgroup per group of tiles of levels.hip's decoder: its chunks into LDS, one lane per chunk, then the reconstruction
//   finish   status; zeros for a frame that failed
// window (svc_hip_window_entropy_frames): an SVCE stream restricted to a window per output frame on its coded bytes -- kept chunks
// copied, dropped chunks a constant, only the chunks a window edge cuts walked and coded again; its kernels are listed at their section
#include "display_core.hpp"
#include "idct_core.hpp"
#include "stream_format.hpp"

#include <algorithm>

namespace svc {
namespace {

constexpr uint32_t kChunkCoeffs = 2048;  // the encoder's chunk: about this many coefficients ...
constexpr uint32_t kMaxChunkTiles = 64;  // ... and at most one tile per lane of a wave
constexpr uint32_t kMaxPrefix = 24;      // a longer Exp-Golomb prefix is malformed (valid values need at most 17)
constexpr uint32_t kWaves = kThreads / 64;

struct Geom {
  uint32_t w, h, bw, bh, mvbw, mvbh, mvb, tx, ty, area, nw;
  uint32_t ct, cx, chunks;  // the encoder's chunk_tiles, chunks per tile row, chunks per frame
  uint32_t max_chunks;      // chunks per frame at chunk_tiles 1 (what the decoder's workspace holds)
  uint32_t max_chunk_bytes; // the largest chunk the encoder writes (its raw size)
  uint64_t masks_off, levels_off;
};

// the SVCQ frame's layout and this file's chunk split
Geom make_geom(uint32_t w, uint32_t h, uint32_t bw, uint32_t bh, uint32_t mvbw, uint32_t mvbh) {
  const FrameLayout l = frame_layout(w, h, bw, bh, mvbw, mvbh);
  Geom g{};
  g.w = w; g.h = h; g.bw = bw; g.bh = bh; g.mvbw = mvbw; g.mvbh = mvbh;
  g.mvb = l.mvb;
  g.tx = l.tiles_x; g.ty = l.tiles_y; g.area = bw * bh; g.nw = l.words;
  g.masks_off = l.masks_off; g.levels_off = l.levels_off;
  g.ct = std::min(kMaxChunkTiles, std::max(1u, kChunkCoeffs / g.area));
  g.cx = div_up(g.tx, g.ct);
  g.chunks = 3 * g.ty * g.cx;
  g.max_chunks = 3 * g.ty * g.tx;
  const uint32_t nt = std::min(g.ct, g.tx);
  g.max_chunk_bytes = 1 + 8 * g.nw * nt + 2 * nt * g.area;
  return g;
}

// the worst SVCE frame: SVCQ's worst case, the types section's mode word, and per chunk its index entry and mode byte
uint64_t svce_max_bytes(const Geom& g) { return up16(g.levels_off + 6ull * g.w * g.h + 4 + 5ull * g.chunks); }

// ---- workspaces ---------------------------------------------------------------------------------------------------------------

struct EncWs {
  uint32_t* cnt;    // [n][chunks] levels (bit 31: mask bits past the tile), then their exclusive prefix
  uint32_t* info;   // [n][chunks] bytes | k_dc << 16 | k_ac << 19 | raw << 22
  uint32_t* coff;   // [n][chunks] byte offset of the chunk's payload inside the frame
  uint32_t* status; // [n]
  uint32_t* types;  // [n][2] types section: bytes, width | raw << 8
  uint32_t* fbytes; // [n] SVCE frame bytes
  uint64_t* foff;   // [n + 1] frame offsets
};
EncWs enc_ws(Carver& c, uint32_t n, const Geom& g) {
  EncWs s;
  s.cnt = c.take<uint32_t>((uint64_t)n * g.chunks);
  s.info = c.take<uint32_t>((uint64_t)n * g.chunks);
  s.coff = c.take<uint32_t>((uint64_t)n * g.chunks);
  s.status = c.take<uint32_t>(n);
  s.types = c.take<uint32_t>(n);  // [n][2] in the room of two arrays of n, each rounded up
  (void)c.take<uint32_t>(n);
  s.fbytes = c.take<uint32_t>(n);
  s.foff = c.take<uint64_t>((uint64_t)n + 1);
  return s;
}

struct DecWs {
  uint32_t* coff;   // [n][max_chunks] byte offset of the chunk's payload inside the frame
  uint32_t* loff;   // [n][max_chunks] its first level
  uint32_t* status; // [n]
  uint32_t* fail;   // [n] set by a chunk that fails
  uint32_t* chunks; // [n] chunk_tiles of the frame's header (0 for a frame that failed its checks)
  uint32_t* qbytes; // [n] SVCQ frame bytes written (the header's, or 64 for a frame that failed its checks)
  uint64_t* qoff;   // [n + 1]
};
DecWs dec_ws(Carver& c, uint32_t n, const Geom& g) {
  DecWs s;
  s.coff = c.take<uint32_t>((uint64_t)n * g.max_chunks);
  s.loff = c.take<uint32_t>((uint64_t)n * g.max_chunks);
  s.status = c.take<uint32_t>(n);
  s.fail = c.take<uint32_t>(n);
  s.chunks = c.take<uint32_t>(n);
  s.qbytes = c.take<uint32_t>(n);
  s.qoff = c.take<uint64_t>((uint64_t)n + 1);
  return s;
}
// what svc_hip_entropy_workspace_bytes reports for both directions, and the fused decode's own: nothing for an empty batch
uint64_t fused_ws_need(uint32_t n, const Geom& g) { return n ? layout_bytes(dec_ws, n, g) : 0; }
uint64_t coder_ws_need(uint32_t n, const Geom& g) { return n ? std::max(layout_bytes(enc_ws, n, g), layout_bytes(dec_ws, n, g)) : 0; }

// ---- device helpers -----------------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t block_max(uint32_t v, uint32_t* lds4) {
  for (uint32_t off = 32; off >= 1; off >>= 1) v = max(v, (uint32_t)__shfl_xor(v, off, 64));
  if ((threadIdx.x & 63u) == 0) lds4[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t m = 0;
  for (uint32_t i = 0; i < kWaves; ++i) m = max(m, lds4[i]);
  __syncthreads();
  return m;
}

__device__ __forceinline__ uint32_t bitlen32(uint32_t x) { return x ? 32u - __clz(x) : 0u; }
__device__ __forceinline__ uint32_t sgn(int32_t v) { return v > 0 ? 2u * (uint32_t)v - 1u : 2u * (uint32_t)(-v); }
__device__ __forceinline__ int32_t unsgn(uint32_t u) { return (u & 1u) ? (int32_t)((u + 1u) >> 1) : -(int32_t)(u >> 1); }
// Exp-Golomb-k code length of u: 2 * floor(log2((u >> k) + 1)) + 1 + k
__device__ __forceinline__ uint32_t eg_len(uint32_t u, uint32_t k) { return 2u * (bitlen32((u >> k) + 1u) - 1u) + 1u + k; }

// ---- encode -------------------------------------------------------------------------------------------------------------------

struct EncArgs {
  Geom g;
  const uint8_t* in;
  uint64_t in_bytes;
  const uint64_t* in_off;
  uint8_t* out;
  uint64_t* out_off;
  uint32_t* d_status;
  EncWs ws;
  uint32_t n;
};

// chunk c of a frame -> its first tile row (plane * ty + tile row), first tile and tile count
__device__ __forceinline__ void chunk_tiles(const Geom& g, uint32_t ct, uint32_t cx, uint32_t c, uint32_t* row, uint32_t* t0, uint32_t* nt) {
  *row = c / cx;
  *t0 = (c - *row * cx) * ct;
  *nt = min(ct, g.tx - *t0);
}

// count: one wave per chunk, a lane per tile
__global__ __launch_bounds__(256) void enc_count_kernel(EncArgs a) {
  const Geom& g = a.g;
  const uint32_t f = blockIdx.y, c = blockIdx.x * kWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (c >= g.chunks) return;
  uint64_t off = 0;
  const uint32_t* hdr = nullptr;
  uint32_t cnt = 0, stray = 0;
  if (check_svcq<true>(g, a.in, a.in_bytes, a.in_off, f, &off, &hdr) == kStOk) {
    uint32_t row, t0, nt;
    chunk_tiles(g, g.ct, g.cx, c, &row, &t0, &nt);
    if (lane < nt) {
      const uint8_t* m = mask_words(a.in + a.in_off[f] + g.masks_off, row, g.tx, (uint64_t)t0 + lane, g.nw);
      for (uint32_t j = 0; j < g.nw; ++j) {
        const uint64_t w = load_mask(m + 8 * j);
        const uint32_t valid = min(64u, g.area - 64 * j);
        const uint64_t keep = valid == 64 ? ~0ull : ((1ull << valid) - 1);
        cnt += __popcll(w & keep);
        stray |= (w & ~keep) != 0;
      }
    }
  }
  cnt = wave_sum(cnt);
  stray = wave_sum(stray);
  if (lane == 0) a.ws.cnt[(size_t)f * g.chunks + c] = cnt | (stray ? 0x80000000u : 0u);
}

// scan: one workgroup per frame
__global__ __launch_bounds__(256) void enc_scan_kernel(EncArgs a) {
  __shared__ uint32_t red[kWaves];
  const Geom& g = a.g;
  const uint32_t f = blockIdx.x;
  uint32_t* cnt = a.ws.cnt + (size_t)f * g.chunks;
  // (scan_counts' loop in its own text, bit 31 masked on the way: through the function this kernel measured 2 % slower,
  // profiles/stream_blocks_refactor.txt)
  uint32_t carry = 0, stray = 0;
  for (uint32_t base = 0; base < g.chunks; base += kThreads) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < g.chunks ? cnt[i] : 0u;
    stray |= v >> 31;
    uint32_t total;
    const uint32_t ex = block_exclusive_scan(v & 0x7FFFFFFFu, red, &total);
    if (i < g.chunks) cnt[i] = carry + ex;
    carry += total;
  }
  uint32_t any_stray;
  (void)block_exclusive_scan(stray, red, &any_stray);
  uint64_t off = 0;
  const uint32_t* hdr = nullptr;
  uint32_t st = check_svcq<true>(g, a.in, a.in_bytes, a.in_off, f, &off, &hdr);
  if (st == kStOk && any_stray) st = kStStrayBits;
  if (st == kStOk && hdr[kHLevels] != carry) st = kStLevels;
  // the types section: a bitmap and fixed-width values, or raw when strictly smaller
  uint32_t nnz = 0, vmax = 0;
  if (st == kStOk) {
    const uint32_t* types = hdr + kHeaderBytes / 4;
    for (uint32_t i = threadIdx.x; i < g.mvb; i += kThreads) {
      const uint32_t t = types[i];
      nnz += t != 0;
      vmax = max(vmax, t);
    }
  }
  uint32_t total_nnz;
  (void)block_exclusive_scan(nnz, red, &total_nnz);
  vmax = block_max(vmax, red);
  if (threadIdx.x == 0) {
    const uint32_t width = total_nnz ? bitlen32(vmax - 1) : 0;
    const uint64_t coded = 4ull * (1 + div_up(g.mvb, 32) + (uint32_t)(((uint64_t)total_nnz * width + 31) / 32));
    const uint64_t raw = 4ull + 4ull * g.mvb;
    a.ws.types[2 * f] = (uint32_t)(raw < coded ? raw : coded);
    a.ws.types[2 * f + 1] = raw < coded ? 1u << 8 : width;
    a.ws.status[f] = st;
    a.d_status[f] = st;
  }
}

// per tile of a chunk (lane = tile): walk its set mask bits in coefficient order; fn(pos, level) for each
template <typename Fn>
__device__ __forceinline__ void for_each_level(const Geom& g, const uint8_t* masks, const int16_t* lev, Fn fn) {
  uint32_t i = 0;
  for (uint32_t j = 0; j < g.nw; ++j) {
    uint64_t w = load_mask(masks + 8 * j);
    while (w) {
      const uint32_t b = __ffsll((unsigned long long)w) - 1;
      w &= w - 1;
      fn(64 * j + b, (int32_t)lev[i++]);
    }
  }
}

__device__ __forceinline__ uint32_t tile_levels(const Geom& g, const uint8_t* masks) {
  uint32_t n = 0;
  for (uint32_t j = 0; j < g.nw; ++j) n += __popcll(load_mask(masks + 8 * j));
  return n;
}

struct TileCtx {
  const uint8_t* masks;
  const int16_t* lev;
  uint32_t nt, row, t0;
};

// the chunk's tile `lane`: its masks and its first level (wave-wide: every lane takes part in the scan)
__device__ __forceinline__ TileCtx tile_ctx(const EncArgs& a, uint32_t f, uint32_t c, uint32_t lane) {
  const Geom& g = a.g;
  TileCtx t;
  chunk_tiles(g, g.ct, g.cx, c, &t.row, &t.t0, &t.nt);
  const uint8_t* frame = a.in + a.in_off[f];
  // (mask_words' address, written out here and in the scatter's raw copy: through it the two heaviest encoder kernels compile to other code)
  t.masks = frame + g.masks_off + 8ull * (((uint64_t)t.row * g.tx + t.t0 + min(lane, t.nt - 1)) * g.nw);
  const uint32_t mine = lane < t.nt ? tile_levels(g, t.masks) : 0u;
  const uint32_t first = a.ws.cnt[(size_t)f * g.chunks + c] + wave_exclusive_scan(mine);
  t.lev = reinterpret_cast<const int16_t*>(frame + g.levels_off) + first;
  return t;
}

// lengths: one wave per chunk, a lane per tile -> bytes, k_dc, k_ac, raw
__global__ __launch_bounds__(256) void enc_lengths_kernel(EncArgs a) {
  const Geom& g = a.g;
  const uint32_t f = blockIdx.y, c = blockIdx.x * kWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (c >= g.chunks || a.ws.status[f] != kStOk) return;
  const TileCtx t = tile_ctx(a, f, c, lane);
  uint32_t dc_bits[8] = {}, ac_bits[8] = {};
  uint32_t fixed = 0, forced = 0, n_lev = 0;
  int32_t dc = 0;
  if (lane < t.nt) {
    uint32_t prev = 0, nac = 0;
    for_each_level(g, t.masks, t.lev, [&](uint32_t pos, int32_t v) {
      ++n_lev;
      forced |= v == 0;
      if (pos == 0) { dc = v; return; }
      ++nac;
      fixed += eg_len(pos - prev - 1, 0);
      prev = pos;
      const uint32_t u = sgn(v);
      for (uint32_t k = 0; k < 8; ++k) ac_bits[k] += eg_len(u, k);
    });
    fixed += eg_len(nac, 0);
  }
  const int32_t left = __shfl_up(dc, 1, 64);
  if (lane < t.nt) {
    const uint32_t u = sgn(dc - (lane == 0 ? 0 : left));
    for (uint32_t k = 0; k < 8; ++k) dc_bits[k] = eg_len(u, k);
  }
  fixed = wave_sum(fixed);
  forced = wave_sum(forced);
  n_lev = wave_sum(n_lev);
  uint32_t best_dc = 0, best_ac = 0, kd = 0, ka = 0;
  for (uint32_t k = 0; k < 8; ++k) {
    const uint32_t d = wave_sum(dc_bits[k]), s = wave_sum(ac_bits[k]);
    if (k == 0 || d < best_dc) { best_dc = d; kd = k; }
    if (k == 0 || s < best_ac) { best_ac = s; ka = k; }
  }
  if (lane == 0) {
    const uint32_t coded = (7 + fixed + best_dc + best_ac + 7) / 8;
    const uint32_t raw = 1 + 8 * g.nw * t.nt + 2 * n_lev;
    const bool use_raw = forced || raw < coded;
    a.ws.info[(size_t)f * g.chunks + c] = (use_raw ? raw : coded) | (kd << 16) | (ka << 19) | ((use_raw ? 1u : 0u) << 22);
  }
}

// layout: one workgroup per frame -> chunk byte offsets, frame bytes
__global__ __launch_bounds__(256) void enc_layout_kernel(EncArgs a) {
  __shared__ uint32_t red[kWaves];
  const Geom& g = a.g;
  const uint32_t f = blockIdx.x;
  if (a.ws.status[f] != kStOk) {
    if (threadIdx.x == 0) a.ws.fbytes[f] = kHeaderBytes;
    return;
  }
  const uint32_t payload = kHeaderBytes + a.ws.types[2 * f] + 4 * g.chunks;
  uint32_t carry = payload;  // (scan_counts' loop in its own text, as in enc_scan_kernel: through the function it measured 1.5 % slower)
  for (uint32_t base = 0; base < g.chunks; base += kThreads) {
    const uint32_t i = base + threadIdx.x;
    const uint32_t v = i < g.chunks ? a.ws.info[(size_t)f * g.chunks + i] & 0xFFFFu : 0u;
    uint32_t total;
    const uint32_t ex = block_exclusive_scan(v, red, &total);
    if (i < g.chunks) a.ws.coff[(size_t)f * g.chunks + i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) a.ws.fbytes[f] = (uint32_t)up16(carry);
}

// LDS bit writer: the field's `bits` low bits of v at bit `pos` of the chunk's words (fields never overlap: OR)
__device__ __forceinline__ void put_bits(uint32_t* words, uint32_t pos, uint64_t v) {
  const uint64_t s = v << (pos & 31u);
  const uint32_t w = pos >> 5;
  if ((uint32_t)s) atomicOr(&words[w], (uint32_t)s);
  if ((uint32_t)(s >> 32)) atomicOr(&words[w + 1], (uint32_t)(s >> 32));
}
// Exp-Golomb-k code of u at bit pos (z zeros, a 1, the low n bits of w = u + 2^k); returns its length
__device__ __forceinline__ uint32_t put_eg(uint32_t* words, uint32_t pos, uint32_t u, uint32_t k) {
  const uint32_t w = u + (1u << k);
  const uint32_t n = bitlen32(w) - 1, z = n - k;
  put_bits(words, pos + z, 1ull | ((uint64_t)(w & ((1u << n) - 1u)) << 1));
  return z + 1 + n;
}

// scatter: one wave per chunk; coded chunks are assembled in LDS (the wave's words), then stored bytewise
__global__ __launch_bounds__(256) void enc_scatter_kernel(EncArgs a, uint32_t lds_words) {
  extern __shared__ uint32_t lds[];
  const Geom& g = a.g;
  const uint32_t f = blockIdx.y, c = blockIdx.x * kWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (c >= g.chunks || a.ws.status[f] != kStOk) return;
  const uint32_t info = a.ws.info[(size_t)f * g.chunks + c];
  const uint32_t size = info & 0xFFFFu, kd = (info >> 16) & 7u, ka = (info >> 19) & 7u;
  uint8_t* dst = a.out + a.ws.foff[f] + a.ws.coff[(size_t)f * g.chunks + c];
  const TileCtx t = tile_ctx(a, f, c, lane);
  if (info >> 22) {  // raw: the mode byte, then the chunk's mask words and levels as they are (both contiguous in SVCQ)
    const uint32_t mbytes = 8 * g.nw * t.nt;
    const uint8_t* m = a.in + a.in_off[f] + g.masks_off + 8ull * ((uint64_t)t.row * g.tx + t.t0) * g.nw;
    const uint8_t* l = reinterpret_cast<const uint8_t*>(__shfl(reinterpret_cast<uintptr_t>(t.lev), 0, 64));
    for (uint32_t i = lane; i < size; i += 64) dst[i] = i == 0 ? 1 : (i <= mbytes ? m[i - 1] : l[i - 1 - mbytes]);
    return;
  }
  uint32_t* words = lds + (threadIdx.x >> 6) * lds_words;
  for (uint32_t i = lane; i < lds_words; i += 64) words[i] = 0;
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  // this tile's DC and code length, then its bit offset in the chunk
  int32_t dc = 0;
  uint32_t len = 0;
  if (lane < t.nt) {
    uint32_t prev = 0, nac = 0;
    for_each_level(g, t.masks, t.lev, [&](uint32_t pos, int32_t v) {
      if (pos == 0) { dc = v; return; }
      ++nac;
      len += eg_len(pos - prev - 1, 0) + eg_len(sgn(v), ka);
      prev = pos;
    });
    len += eg_len(nac, 0);
  }
  const int32_t left = __shfl_up(dc, 1, 64);
  const uint32_t udc = sgn(dc - (lane == 0 ? 0 : left));
  if (lane < t.nt) len += eg_len(udc, kd);
  uint32_t pos = 7 + wave_exclusive_scan(lane < t.nt ? len : 0u);
  if (lane == 0) put_bits(words, 0, (kd << 1) | (ka << 4));
  if (lane < t.nt) {
    pos += put_eg(words, pos, udc, kd);
    uint32_t nac = 0;
    for (uint32_t j = 0; j < g.nw; ++j) nac += __popcll(load_mask(t.masks + 8 * j));
    nac -= (uint32_t)(load_mask(t.masks) & 1u);
    pos += put_eg(words, pos, nac, 0);
    uint32_t prev = 0;
    for_each_level(g, t.masks, t.lev, [&](uint32_t p, int32_t v) {
      if (p == 0) return;
      pos += put_eg(words, pos, p - prev - 1, 0);
      pos += put_eg(words, pos, sgn(v), ka);
      prev = p;
    });
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  const uint8_t* bytes = reinterpret_cast<const uint8_t*>(words);
  for (uint32_t i = lane; i < size; i += 64) dst[i] = bytes[i];
}

// frame: one workgroup per frame -> header, types section, index, padding, or 64 zero bytes for a frame that failed
__global__ __launch_bounds__(256) void enc_frame_kernel(EncArgs a) {
  __shared__ uint32_t red[kWaves];
  __shared__ uint32_t win[kThreads + 2];
  const Geom& g = a.g;
  const uint32_t f = blockIdx.x;
  uint8_t* frame = a.out + a.ws.foff[f];
  uint32_t* fw = reinterpret_cast<uint32_t*>(frame);
  const uint32_t st = a.ws.status[f];
  if (st != kStOk) {
    if (threadIdx.x < 16) fw[threadIdx.x] = 0;
    return;
  }
  const uint32_t* in = reinterpret_cast<const uint32_t*>(a.in + a.in_off[f]);
  const uint32_t tbytes = a.ws.types[2 * f], width = a.ws.types[2 * f + 1] & 0xFFu, raw = a.ws.types[2 * f + 1] >> 8;
  const uint32_t fbytes = a.ws.fbytes[f];
  if (threadIdx.x < 16) {
    uint32_t v = in[threadIdx.x];
    if (threadIdx.x == 0) v = kMagicE;
    if (threadIdx.x == kHBytes) v = fbytes;
    if (threadIdx.x == kESvcqBytes) v = in[kHBytes];
    if (threadIdx.x == kEChunkTiles) v = g.ct;
    if (threadIdx.x == kETypesBytes) v = tbytes;
    fw[threadIdx.x] = v;
  }
  const uint32_t* types = in + kHeaderBytes / 4;
  uint32_t* sec = fw + kHeaderBytes / 4;
  if (raw) {
    if (threadIdx.x == 0) sec[0] = 1;
    for (uint32_t i = threadIdx.x; i < g.mvb; i += kThreads) sec[1 + i] = types[i];
  } else {
    if (threadIdx.x == 0) sec[0] = width << 8;
    const uint32_t bm = div_up(g.mvb, 32);
    uint32_t* vals = sec + 1 + bm;
    // 256 types at a time: the bitmap word of every 32, and the values (type - 1) in `width` bits at rank * width, ORed into an
    // LDS window of words; complete words go out, the partial last one carries into the next window
    uint32_t rank0 = 0, carry = 0;
    for (uint32_t base = 0; base < g.mvb; base += kThreads) {
      const uint32_t i = base + threadIdx.x;
      const uint32_t t = i < g.mvb ? types[i] : 0u;
      const uint64_t b = __ballot(t != 0);
      if ((threadIdx.x & 31u) == 0 && i < g.mvb) sec[1 + (i >> 5)] = (uint32_t)(b >> (threadIdx.x & 32u));
      uint32_t total;
      const uint32_t ex = block_exclusive_scan(t != 0 ? 1u : 0u, red, &total);
      if (width) {
        const uint64_t w0 = ((uint64_t)rank0 * width) >> 5;
        for (uint32_t j = threadIdx.x; j < kThreads + 2; j += kThreads) win[j] = j == 0 ? carry : 0u;
        __syncthreads();
        if (t != 0) {
          const uint32_t bit = (uint32_t)((uint64_t)(rank0 + ex) * width - 32 * w0);
          const uint64_t v = (uint64_t)(t - 1u) << (bit & 31u);
          if ((uint32_t)v) atomicOr(&win[bit >> 5], (uint32_t)v);
          if ((uint32_t)(v >> 32)) atomicOr(&win[(bit >> 5) + 1], (uint32_t)(v >> 32));
        }
        __syncthreads();
        const uint32_t full = (uint32_t)((((uint64_t)(rank0 + total) * width) >> 5) - w0);
        for (uint32_t j = threadIdx.x; j < full; j += kThreads) vals[w0 + j] = win[j];
        carry = win[full];
        __syncthreads();
      }
      rank0 += total;
    }
    const uint64_t end_bit = (uint64_t)rank0 * width;
    if (threadIdx.x == 0 && (end_bit & 31u)) vals[end_bit >> 5] = carry;
  }
  // the index: bytes | levels << 16 per chunk
  const uint32_t level_count = in[kHLevels];
  uint32_t* index = fw + (kHeaderBytes + tbytes) / 4;
  for (uint32_t i = threadIdx.x; i < g.chunks; i += kThreads) {
    const uint32_t lo = a.ws.cnt[(size_t)f * g.chunks + i];
    const uint32_t hi = i + 1 < g.chunks ? a.ws.cnt[(size_t)f * g.chunks + i + 1] : level_count;
    index[i] = (a.ws.info[(size_t)f * g.chunks + i] & 0xFFFFu) | ((hi - lo) << 16);
  }
  // padding: after the last chunk's payload
  const uint32_t last = g.chunks - 1;
  const uint32_t used = a.ws.coff[(size_t)f * g.chunks + last] + (a.ws.info[(size_t)f * g.chunks + last] & 0xFFFFu);
  for (uint32_t i = used + threadIdx.x; i < fbytes; i += kThreads) frame[i] = 0;
}

// ---- decode -------------------------------------------------------------------------------------------------------------------

struct DecArgs {
  Geom g;
  const uint8_t* in;
  uint64_t in_bytes;
  const uint64_t* in_off;
  uint8_t* out;
  uint64_t* out_off;
  uint32_t* d_status;
  DecWs ws;
  uint32_t n;
};

// frame check and index scan, by one workgroup: input frame f (f_ok: it is one of the batch's; else kStRange) into the workspace's entry
// `slot`.  recodable: also refuse (kStGeometry) a chunk_tiles whose raw chunk, 1 + (8 nw + 2 area) min(chunk_tiles, tiles_x) bytes, is
// above the index's u16 -- what the window call must be able to write for any chunk it cuts.
__device__ __forceinline__ void dec_check_frame(const DecArgs& a, uint32_t f, bool f_ok, uint32_t slot, bool recodable, uint32_t* red,
                                                uint32_t* s_st_p) {
  uint32_t& s_st = *s_st_p;
  const Geom& g = a.g;
  const uint64_t o = f_ok ? a.in_off[f] : 0, e = f_ok ? a.in_off[f + 1] : 0;
  uint32_t st = kStOk, ct = 0, cx = 0, chunks = 0;
  const uint32_t* h = nullptr;
  uint64_t payload = 0;
  if (!f_ok || o % 16 != 0 || o > e || e > a.in_bytes || e - o < kHeaderBytes) st = kStRange;
  if (st == kStOk) {
    h = reinterpret_cast<const uint32_t*>(a.in + o);
    if (h[kHMagic] != kMagicE) st = kStMagic;
    else if (h[kHVersion] != kVersion) st = kStVersion;
    else if (h[kHWidth] != g.w || h[kHHeight] != g.h || h[kHTileW] != g.bw || h[kHTileH] != g.bh || h[kHMvW] != g.mvbw ||
             h[kHMvH] != g.mvbh || h[kHFgStep] == 0 || h[kHBgStep] == 0 || h[kEChunkTiles] == 0 ||
             (recodable && 1ull + (8ull * g.nw + 2ull * g.area) * min(h[kEChunkTiles], g.tx) > 0xFFFFull))
      st = kStGeometry;
    else if (h[kHBytes] % 16 != 0 || h[kHBytes] != e - o) st = kStSize;
    else if (h[kHLevels] > 3ull * g.w * g.h || h[kESvcqBytes] != up16(g.levels_off + 2ull * h[kHLevels])) st = kStSvcqBytes;
    else {
      ct = h[kEChunkTiles];
      cx = ct >= g.tx ? 1u : (g.tx + ct - 1) / ct;  // ct may exceed tx (up to 2^32 - 1): then a chunk per tile row
      chunks = 3 * g.ty * cx;
      payload = kHeaderBytes + (uint64_t)h[kETypesBytes] + 4ull * chunks;
      if (h[kETypesBytes] % 4 != 0 || payload > h[kHBytes]) st = kStIndex;
    }
  }
  // the index: chunk byte and level offsets
  uint32_t bytes_total = 0, lev_total = 0;
  if (st == kStOk) {
    const uint32_t* index = h + (kHeaderBytes + h[kETypesBytes]) / 4;
    uint32_t bcarry = 0, lcarry = 0;
    for (uint32_t base = 0; base < chunks; base += kThreads) {
      const uint32_t i = base + threadIdx.x;
      const uint32_t v = i < chunks ? index[i] : 0u;
      uint32_t tb, tl;
      const uint32_t eb = block_exclusive_scan(v & 0xFFFFu, red, &tb);
      const uint32_t el = block_exclusive_scan(v >> 16, red, &tl);
      if (i < chunks) {
        a.ws.coff[(size_t)slot * g.max_chunks + i] = (uint32_t)payload + bcarry + eb;
        a.ws.loff[(size_t)slot * g.max_chunks + i] = lcarry + el;
      }
      bcarry += tb;
      lcarry += tl;
    }
    bytes_total = bcarry;
    lev_total = lcarry;
    if (up16(payload + bytes_total) != h[kHBytes] || lev_total != h[kHLevels]) st = kStIndex;
  }
  // the types section: its mode word and its size against the bitmap's popcount
  if (st == kStOk) {
    const uint32_t* sec = h + kHeaderBytes / 4;
    const uint32_t tbytes = h[kETypesBytes];
    const uint32_t head = tbytes >= 4 ? sec[0] : 0xFFFFFFFFu;
    const uint32_t mode = head & 0xFFu, width = head >> 8;
    const uint32_t bm = div_up(g.mvb, 32);
    uint32_t bad = 0, nnz = 0;
    if (tbytes < 4) bad = 1;
    else if (mode == 1 && width == 0) bad = (uint64_t)tbytes != 4ull + 4ull * g.mvb;
    else if (mode != 0 || width > 32 || (uint64_t)tbytes < 4ull * (1 + bm)) bad = 1;
    else {
      for (uint32_t j = threadIdx.x; j < bm; j += kThreads) {
        uint32_t w = sec[1 + j];
        if (j == bm - 1 && g.mvb % 32) {
          if (w >> (g.mvb % 32)) bad = 1;  // bitmap bits past the MV blocks
          w &= (1u << (g.mvb % 32)) - 1u;
        }
        nnz += __popc(w);
      }
    }
    uint32_t any_bad, total_nnz;
    (void)block_exclusive_scan(bad, red, &any_bad);
    (void)block_exclusive_scan(nnz, red, &total_nnz);
    if (!any_bad && mode == 0 && (uint64_t)tbytes != 4ull * (1 + bm + ((uint64_t)total_nnz * width + 31) / 32)) any_bad = 1;
    if (!any_bad && mode == 0 && width == 32) {  // a stored id - 1 of 2^32 - 1 would decode to the id 2^32, which u32 cannot hold
      uint32_t over = 0;
      for (uint32_t i = threadIdx.x; i < total_nnz; i += kThreads) over |= sec[1 + bm + i] == 0xFFFFFFFFu;
      uint32_t any_over;
      (void)block_exclusive_scan(over, red, &any_over);
      any_bad = any_over;
    }
    if (any_bad) st = kStIndex;
  }
  if (threadIdx.x == 0) s_st = st;
  __syncthreads();
  if (threadIdx.x == 0) {
    a.ws.status[slot] = s_st;
    a.ws.fail[slot] = 0;
    a.ws.chunks[slot] = s_st == kStOk ? ct : 0u;
    a.ws.qbytes[slot] = s_st == kStOk ? h[kESvcqBytes] : kHeaderBytes;
  }
}

__global__ __launch_bounds__(256) void dec_check_kernel(DecArgs a) {
  __shared__ uint32_t red[kWaves];
  __shared__ uint32_t s_st;
  dec_check_frame(a, blockIdx.x, true, blockIdx.x, false, red, &s_st);
}

// a bit reader over one frame: aligned u32 loads, nothing read at or past the frame's end (zeros there).  The bits from the read
// position sit in a 64-bit buffer (33 .. 64 of them after a refill) and the next word is loaded one refill ahead, so a codeword
// usually costs no load of its own; a codeword longer than the buffer holds is read from memory directly.
struct BitReader {
  const uint32_t* w;
  uint32_t nwords;
  uint64_t buf;   // bits [pos, pos + nb) of the frame, the rest zero
  uint32_t nb;
  uint64_t wi;    // the word that follows them
  uint32_t ahead; // word(wi), loaded in advance
  __device__ __forceinline__ uint32_t word(uint64_t i) const { return i < nwords ? w[i] : 0u; }
  __device__ __forceinline__ uint64_t peek(uint64_t pos) const {
    const uint64_t i = pos >> 5;
    const uint32_t s = (uint32_t)(pos & 31u);
    const uint64_t lo = (uint64_t)word(i) | ((uint64_t)word(i + 1) << 32);
    return s ? (lo >> s) | ((uint64_t)word(i + 2) << (64 - s)) : lo;
  }
  __device__ __forceinline__ void seek(uint64_t pos) {
    wi = pos >> 5;
    const uint32_t s = (uint32_t)(pos & 31u);
    buf = (uint64_t)(word(wi) >> s);
    nb = 32 - s;
    ++wi;
    ahead = word(wi);
  }
  __device__ __forceinline__ void refill() {
    while (nb <= 32) {
      buf |= (uint64_t)ahead << nb;
      nb += 32;
      ++wi;
      ahead = word(wi);
    }
  }
};

// one Exp-Golomb-k codeword at *pos (bounded by end): false when malformed
__device__ __forceinline__ bool get_eg(BitReader& r, uint64_t* pos, uint64_t end, uint32_t k, uint32_t* u) {
  r.refill();
  uint64_t v = r.buf;
  uint32_t z = v ? (uint32_t)__builtin_ctzll(v) : 64u;
  const bool slow = z >= r.nb || 2 * z + k + 1 > r.nb;  // the codeword runs past the buffered bits
  if (slow) {
    v = r.peek(*pos);
    z = v ? (uint32_t)__builtin_ctzll(v) : 64u;
  }
  if (z > kMaxPrefix) return false;
  const uint32_t n = z + k, len = z + 1 + n;
  if (*pos + len > end) return false;
  const uint64_t w = (1ull << n) | ((v >> (z + 1)) & ((1ull << n) - 1));
  *u = (uint32_t)(w - (1ull << k));
  *pos += len;
  if (slow) {
    r.seek(*pos);
  } else {
    r.buf >>= len;
    r.nb -= len;
  }
  return true;
}

// chunks: one lane per chunk; decodes the masks and levels of its tiles into the SVCQ frame
__global__ __launch_bounds__(256) void dec_chunks_kernel(DecArgs a) {
  const Geom& g = a.g;
  const uint32_t f = blockIdx.y, c = blockIdx.x * kThreads + threadIdx.x;
  if (c >= g.max_chunks || a.ws.status[f] != kStOk) return;
  const uint32_t ct = a.ws.chunks[f], cx = ct >= g.tx ? 1u : (g.tx + ct - 1) / ct;
  if (c >= 3 * g.ty * cx) return;
  const uint8_t* frame = a.in + a.in_off[f];
  const uint32_t* hdr = reinterpret_cast<const uint32_t*>(frame);
  const uint32_t fbytes = hdr[kHBytes];
  const uint32_t* index = hdr + (kHeaderBytes + hdr[kETypesBytes]) / 4;
  const uint32_t entry = index[c], size = entry & 0xFFFFu, count = entry >> 16;
  const uint32_t start = a.ws.coff[(size_t)f * g.max_chunks + c], lev0 = a.ws.loff[(size_t)f * g.max_chunks + c];
  uint32_t row, t0, nt;
  chunk_tiles(g, ct, cx, c, &row, &t0, &nt);
  uint8_t* q = a.out + a.ws.qoff[f];
  uint8_t* masks = mask_words(q + g.masks_off, row, g.tx, t0, g.nw);
  int16_t* lev = reinterpret_cast<int16_t*>(q + g.levels_off) + lev0;
  bool ok = size != 0;
  if (ok && (frame[start] & 1u)) {  // raw: mask words and levels verbatim
    const uint32_t mbytes = 8 * g.nw * nt;
    ok = (uint64_t)size == 1ull + mbytes + 2ull * count;
    uint32_t got = 0;
    for (uint32_t i = 0; ok && i < nt * g.nw; ++i) {
      const uint8_t* s = frame + start + 1 + 8 * i;
      uint64_t m = 0;
      for (uint32_t b = 0; b < 8; ++b) m |= (uint64_t)s[b] << (8 * b);
      const uint32_t j = i % g.nw;
      const uint32_t valid = min(64u, g.area - 64 * j);
      if (valid < 64 && (m >> valid)) ok = false;
      got += __popcll(m);
      store_mask(masks + 8 * i, m);
    }
    ok = ok && got == count;
    const uint8_t* s = frame + start + 1 + mbytes;
    for (uint32_t i = 0; ok && i < count; ++i) lev[i] = (int16_t)((uint32_t)s[2 * i] | ((uint32_t)s[2 * i + 1] << 8));
  } else if (ok) {
    BitReader r{reinterpret_cast<const uint32_t*>(frame), fbytes / 4, 0, 0, 0, 0};
    const uint64_t end = 8ull * (start + size);
    uint64_t pos = 8ull * start;
    const uint32_t head = (uint32_t)r.peek(pos);
    const uint32_t kd = (head >> 1) & 7u, ka = (head >> 4) & 7u;
    pos += 7;
    r.seek(pos);
    uint32_t written = 0;
    int32_t dcp = 0;
    for (uint32_t t = 0; ok && t < nt; ++t) {
      uint8_t* tm = masks + 8ull * t * g.nw;
      uint32_t u;
      ok = get_eg(r, &pos, end, kd, &u);
      if (!ok) break;
      const int32_t dc = dcp + unsgn(u);
      dcp = dc;
      ok = dc >= -32768 && dc <= 32767;
      uint64_t cur = 0;  // the mask word being filled, word cj of the tile
      uint32_t cj = 0;
      if (ok && dc != 0) {
        ok = written < count;
        if (ok) lev[written++] = (int16_t)dc;
        cur = 1;
      }
      uint32_t nac = 0;
      ok = ok && get_eg(r, &pos, end, 0, &nac) && nac <= g.area - 1;
      uint32_t p = 0;
      for (uint32_t i = 0; ok && i < nac; ++i) {
        uint32_t run, lu;
        ok = get_eg(r, &pos, end, 0, &run) && (uint64_t)p + run + 1 <= g.area - 1;
        if (!ok) break;
        p += run + 1;
        ok = get_eg(r, &pos, end, ka, &lu);
        if (!ok) break;
        const int32_t v = unsgn(lu);
        ok = v >= -32768 && v <= 32767 && written < count;
        if (!ok) break;
        lev[written++] = (int16_t)v;
        for (; cj < (p >> 6); ++cj) {
          store_mask(tm + 8 * cj, cur);
          cur = 0;
        }
        cur |= 1ull << (p & 63u);
      }
      if (!ok) break;
      for (; cj < g.nw; ++cj) {
        store_mask(tm + 8 * cj, cur);
        cur = 0;
      }
    }
    ok = ok && written == count && (pos + 7) / 8 == start + size;
  }
  if (!ok) atomicOr(&a.ws.fail[f], 1u);
}

// frame: SVCQ header, types, padding; a frame that failed is zeros (64 B after a failed check, its svcq_frame_bytes after a chunk)
__global__ __launch_bounds__(256) void dec_frame_kernel(DecArgs a) {
  __shared__ uint32_t red[kWaves];
  const Geom& g = a.g;
  const uint32_t f = blockIdx.x;
  uint8_t* q = a.out + a.ws.qoff[f];
  uint32_t* qw = reinterpret_cast<uint32_t*>(q);
  const uint32_t qbytes = a.ws.qbytes[f];
  uint32_t st = a.ws.status[f];
  if (st == kStOk && a.ws.fail[f]) st = kStChunk;
  if (threadIdx.x == 0) a.d_status[f] = st;
  if (st != kStOk) {
    for (uint32_t i = threadIdx.x; i < qbytes / 4; i += kThreads) qw[i] = 0;
    return;
  }
  const uint32_t* h = reinterpret_cast<const uint32_t*>(a.in + a.in_off[f]);
  if (threadIdx.x < 16) {
    uint32_t v = threadIdx.x < 12 ? h[threadIdx.x] : 0u;
    if (threadIdx.x == 0) v = kMagicQ;
    if (threadIdx.x == kHBytes) v = h[kESvcqBytes];
    qw[threadIdx.x] = v;
  }
  const uint32_t* sec = h + kHeaderBytes / 4;
  uint32_t* types = qw + kHeaderBytes / 4;
  const uint32_t head = sec[0], width = head >> 8;
  if (head == 1) {
    for (uint32_t i = threadIdx.x; i < g.mvb; i += kThreads) types[i] = sec[1 + i];
  } else {
    const uint32_t bm = div_up(g.mvb, 32);
    const uint32_t* bitmap = sec + 1;
    const uint32_t* vals = sec + 1 + bm;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < g.mvb; base += kThreads) {
      const uint32_t i = base + threadIdx.x;
      const uint32_t nz = i < g.mvb ? (bitmap[i >> 5] >> (i & 31u)) & 1u : 0u;
      uint32_t total;
      const uint32_t rank = carry + block_exclusive_scan(nz, red, &total);
      carry += total;
      if (i >= g.mvb) continue;
      uint32_t t = 0;
      if (nz) {
        uint64_t v = 0;
        if (width) {
          const uint64_t bit = (uint64_t)rank * width;
          const uint64_t wi = bit >> 5;
          const uint64_t two = (uint64_t)vals[wi] | (wi + 1 < (uint64_t)(h[kETypesBytes] / 4 - 1 - bm) ? (uint64_t)vals[wi + 1] << 32 : 0ull);
          v = (two >> (bit & 31u)) & ((1ull << width) - 1ull);
        }
        t = (uint32_t)(v + 1);
      }
      types[i] = t;
    }
  }
  const uint64_t used = g.levels_off + 2ull * h[kHLevels];
  for (uint64_t i = used + threadIdx.x; i < qbytes; i += kThreads) q[i] = 0;
}

// ---- fused decode: SVCE frames straight to the decoder's reconstruction ---------------------------------------------------------
//
// The encoder's chunk (g.ct tiles) is the group of tiles one workgroup of levels.hip's decode_body reconstructs, so a
// workgroup decodes the chunks that cover its group (one per plane in the encoder's layout) into dense int16 coefficients in LDS and
// inverts them from there: the SVCQ masks and levels never exist.  Any other chunk_tiles is honoured: a chunk that overlaps the group
// is walked from its first tile to the group's last one, and the group that holds a chunk's last tile walks it to its end and makes
// the end checks, so every chunk is checked exactly once in full.

constexpr uint32_t kCoefBytes = 3 * kChunkCoeffs * 2;  // the group's dense int16 coefficients, three planes
constexpr uint32_t kStageSlots = 3;                    // payloads walked from LDS: the first three walkers (the encoder's layout has three)
// a slot holds the largest chunk the encoder writes for a group (raw: mode byte, 8 B per mask word, 2 B per coefficient) from the
// 4-byte boundary below its first byte
constexpr uint32_t kStageWords = (uint32_t)up16(3 + 1 + 8 * (kChunkCoeffs / 64) + 2 * kChunkCoeffs) / 4;

struct FusedArgs {
  Geom g;
  const uint8_t* in;
  const uint64_t* in_off;
  const uint32_t* gaze;  // [n][4] x, y, w, h in padded coordinates, or null
  float* rec;            // [n][h][w][3]
  uint32_t* d_status;
  DecWs ws;
  float fg, bg;          // the decoder's steps
};

// a coded chunk of `size` bytes from byte sb of the reader's words: its tiles [0, t_end); chunk tile t is the group's tile t + d
// (outside the group while that is negative).  to_end: t_end is the chunk's last tile, and the chunk must end where its index says.
__device__ __forceinline__ bool walk_coded(BitReader r, uint32_t sb, uint32_t size, uint32_t count, uint32_t t_end, bool to_end, int32_t d,
                                           uint32_t area, int16_t* coef) {
  const uint64_t end = 8ull * (sb + size);
  uint64_t pos = 8ull * sb;
  const uint32_t head = (uint32_t)r.peek(pos);
  const uint32_t kd = (head >> 1) & 7u, ka = (head >> 4) & 7u;
  pos += 7;
  r.seek(pos);
  uint32_t written = 0;
  int32_t dcp = 0;
  bool ok = true;
  for (uint32_t t = 0; ok && t < t_end; ++t) {
    const int32_t lt = (int32_t)t + d;
    int16_t* tile = coef + lt * (int32_t)area;  // written only for lt >= 0
    uint32_t u;
    ok = get_eg(r, &pos, end, kd, &u);
    if (!ok) break;
    const int32_t dc = dcp + unsgn(u);
    dcp = dc;
    ok = dc >= -32768 && dc <= 32767;
    if (ok && dc != 0) {
      ok = written < count;
      if (ok) {
        ++written;
        if (lt >= 0) tile[0] = (int16_t)dc;
      }
    }
    uint32_t nac = 0;
    ok = ok && get_eg(r, &pos, end, 0, &nac) && nac <= area - 1;
    uint32_t p = 0;
    for (uint32_t i = 0; ok && i < nac; ++i) {
      uint32_t run, lu;
      ok = get_eg(r, &pos, end, 0, &run) && (uint64_t)p + run + 1 <= area - 1;
      if (!ok) break;
      p += run + 1;
      ok = get_eg(r, &pos, end, ka, &lu);
      if (!ok) break;
      const int32_t v = unsgn(lu);
      ok = v >= -32768 && v <= 32767 && written < count;
      if (!ok) break;
      ++written;
      if (lt >= 0) tile[p] = (int16_t)v;
    }
  }
  if (to_end) ok = ok && written == count && (pos + 7) / 8 == sb + size;
  return ok;
}

// a raw chunk of nt tiles at s (its mode byte): the same walk over its mask words, the levels from behind them
__device__ __forceinline__ bool walk_raw(const uint8_t* s, uint32_t size, uint32_t count, uint32_t nt, uint32_t t_end, bool to_end, int32_t d,
                                         const Geom& g, int16_t* coef) {
  const uint32_t mbytes = 8 * g.nw * nt;
  if ((uint64_t)size != 1ull + mbytes + 2ull * count) return false;
  const uint8_t* lv = s + 1 + mbytes;
  uint32_t got = 0;
  for (uint32_t i = 0; i < t_end * g.nw; ++i) {
    const uint8_t* q = s + 1 + 8 * i;
    uint64_t m = 0;
    for (uint32_t b = 0; b < 8; ++b) m |= (uint64_t)q[b] << (8 * b);
    const uint32_t t = i / g.nw, j = i - t * g.nw;
    const uint32_t valid = min(64u, g.area - 64 * j);
    if (valid < 64 && (m >> valid)) return false;
    const int32_t lt = (int32_t)t + d;
    if (lt < 0) {
      got += __popcll(m);
      continue;
    }
    int16_t* word = coef + lt * (int32_t)g.area + 64 * j;
    while (m) {
      const uint32_t b = __ffsll((unsigned long long)m) - 1;
      m &= m - 1;
      if (got >= count) return false;  // more mask bits than levels: nothing is read past the chunk
      word[b] = (int16_t)((uint32_t)lv[2 * got] | ((uint32_t)lv[2 * got + 1] << 8));
      ++got;
    }
  }
  return !to_end || got == count;
}

// One workgroup per (tile row, group in the row) of a frame, the grid of levels.hip's decode_body<N>.  Walk: per plane and per chunk that
// overlaps the group one lane (walker w = lane * 4 + wave: the encoder's three sit in three waves); the first kStageSlots walkers read
// their payload from LDS, staged by all threads with coalesced loads, a payload above a slot is read in place.  Then thread (t, j)
// dequantises row j of tile t from the dense coefficients and takes it through the row and column passes as idct_core.hpp states
// them, so d_rec has the bits of the two calls.  The payload stage and the f64 row slab are never live together and share their bytes.
// (The passes are written out here: with invert_row / invert_column the 8x8 kernel measured 2.6 % slower, profiles/decode_body_refactor.txt.)
template <int N>
__global__ __launch_bounds__(256) void decode_entropy_kernel(FusedArgs a) {
  constexpr uint32_t kRows = kChunkCoeffs / N;
  constexpr uint32_t kRowBytes = kRows * (N + 1) * 8, kStageBytes = kStageSlots * kStageWords * 4;
  __shared__ __attribute__((aligned(16))) uint8_t smem[kCoefBytes + (kRowBytes > kStageBytes ? kRowBytes : kStageBytes)];
  int16_t* coef = reinterpret_cast<int16_t*>(smem);
  uint32_t* stage = reinterpret_cast<uint32_t*>(smem + kCoefBytes);
  double* rows = reinterpret_cast<double*>(smem + kCoefBytes);  // pitch N + 1, the slab of idct_core.hpp's passes
  const Geom& g = a.g;
  const uint32_t f = blockIdx.y, tid = threadIdx.x;
  if (a.ws.status[f] != kStOk) return;  // the finish kernel zeroes the frame
  const uint32_t row = blockIdx.x / g.cx, gt0 = (blockIdx.x - row * g.cx) * g.ct, gnt = min(g.ct, g.tx - gt0);
  const uint8_t* frame = a.in + a.in_off[f];
  const uint32_t* hdr = reinterpret_cast<const uint32_t*>(frame);
  const uint32_t fwords = hdr[kHBytes] / 4;
  const uint32_t* index = hdr + (kHeaderBytes + hdr[kETypesBytes]) / 4;
  const uint32_t* coff = a.ws.coff + (size_t)f * g.max_chunks;
  const uint32_t ct = a.ws.chunks[f], cx = ct >= g.tx ? 1u : (g.tx + ct - 1) / ct;
  const uint32_t c_first = cx == 1 ? 0u : gt0 / ct, c_last = cx == 1 ? 0u : (gt0 + gnt - 1) / ct;
  const uint32_t nwalk = c_last - c_first + 1;  // per plane: at most the group's tiles

  for (uint32_t i = tid; i < kCoefBytes / 16; i += kThreads) reinterpret_cast<uint4*>(smem)[i] = make_uint4(0, 0, 0, 0);
  for (uint32_t s = 0; s < kStageSlots && s < 3 * nwalk; ++s) {
    const uint32_t c = ((s / nwalk) * g.ty + row) * cx + c_first + s % nwalk;
    const uint32_t start = coff[c], size = index[c] & 0xFFFFu;
    const uint32_t w0 = start >> 2, nwords = ((start & 3u) + size + 3) >> 2;
    if (size == 0 || nwords > kStageWords) continue;
    for (uint32_t i = tid; i < nwords; i += kThreads) stage[s * kStageWords + i] = w0 + i < fwords ? hdr[w0 + i] : 0u;
  }
  __syncthreads();

  const uint32_t w = (tid & 63u) * 4 + (tid >> 6);
  if (w < 3 * nwalk) {
    const uint32_t c = ((w / nwalk) * g.ty + row) * cx + c_first + w % nwalk;
    const uint32_t entry = index[c], size = entry & 0xFFFFu, count = entry >> 16, start = coff[c];
    uint32_t crow, t0, nt;
    chunk_tiles(g, ct, cx, c, &crow, &t0, &nt);
    const uint32_t t_end = min(nt, gt0 + gnt - t0);
    const bool to_end = t_end == nt;
    const int32_t d = (int32_t)t0 - (int32_t)gt0;
    int16_t* plane = coef + (w / nwalk) * kChunkCoeffs;
    const bool staged = w < kStageSlots && ((start & 3u) + size + 3) >> 2 <= kStageWords;
    bool ok = size != 0;
    if (ok && (frame[start] & 1u)) {
      const uint8_t* s = staged ? reinterpret_cast<const uint8_t*>(stage + w * kStageWords) + (start & 3u) : frame + start;
      ok = walk_raw(s, size, count, nt, t_end, to_end, d, g, plane);
    } else if (ok && staged) {
      ok = walk_coded(BitReader{stage + w * kStageWords, ((start & 3u) + size + 3) >> 2, 0, 0, 0, 0}, start & 3u, size, count, t_end, to_end, d,
                      g.area, plane);
    } else if (ok) {
      ok = walk_coded(BitReader{hdr, fwords, 0, 0, 0, 0}, start, size, count, t_end, to_end, d, g.area, plane);
    }
    if (!ok) atomicOr(&a.ws.fail[f], 1u);
  }
  __syncthreads();

  const uint32_t t = tid / N, j = tid - t * N;
  const bool active = t < gnt;
  const uint32_t x0 = (gt0 + t) * N, y0 = row * N;
  float enc = 0.f, dec = 1.f;
  if (active) {
    // only type == 0 or not matters to the steps: the bitmap's bit, or the raw id
    const uint32_t* sec = hdr + kHeaderBytes / 4;
    const uint32_t b = (y0 / g.mvbh) * (g.w / g.mvbw) + x0 / g.mvbw;
    const bool bgnd = sec[0] == 1 ? sec[1 + b] == 0 : ((sec[1 + (b >> 5)] >> (b & 31u)) & 1u) == 0;
    const bool in_gaze = gazed(a.gaze, f, x0, y0);
    enc = (float)(bgnd ? hdr[kHBgStep] : hdr[kHFgStep]);
    dec = in_gaze ? 1.f : (bgnd ? a.bg : a.fg);
  }
  float out[3][N];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (active) {
      const int16_t* lev = coef + c * kChunkCoeffs + t * (N * N) + j * N;
      double y[N], r[N];
#pragma unroll
      for (int i = 0; i < N; ++i) y[i] = (double)requant((float)lev[i] * enc, dec);
      idct1d<N>(y, r);
      double* rw = rows + (t * N + j) * (N + 1);
#pragma unroll
      for (int i = 0; i < N; ++i) rw[i] = r[i];
    }
    __syncthreads();
    if (active) {
      double cc[N], xx[N];
#pragma unroll
      for (int v = 0; v < N; ++v) cc[v] = rows[(t * N + v) * (N + 1) + j];
      idct1d<N>(cc, xx);
#pragma unroll
      for (int y = 0; y < N; ++y) out[c][y] = (float)xx[y];
    }
    __syncthreads();  // the next plane reuses rows
  }
  if (!active) return;
  store_bgr_column<N>(a.rec + (((size_t)f * g.h + y0) * g.w + x0 + j) * 3, g.w, out);
}

// after the fused kernel: the frame's status; a frame that failed (its checks, or a chunk, known only after other groups stored
// their pixels) is zeros in d_rec.  A good frame's workgroups leave at once.
__global__ __launch_bounds__(256) void decode_entropy_finish_kernel(FusedArgs a) {
  const Geom& g = a.g;
  const uint32_t f = blockIdx.y;
  uint32_t st = a.ws.status[f];
  if (st == kStOk && a.ws.fail[f]) st = kStChunk;
  if (blockIdx.x == 0 && threadIdx.x == 0) a.d_status[f] = st;
  if (st == kStOk) return;
  const size_t n = (size_t)g.h * g.w * 3;
  float* r = a.rec + (size_t)f * n;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) r[i] = 0.f;
}

// ---- window: SVCE frames restricted to the tiles of a window, on their coded bytes (svc_hip_window_entropy_frames) -------------------
//
// Output frame i = input frame s (d_src[i], or i) as svc_hip_entropy_encode_frames would write its SVCQ frame restricted to window i,
// on the input's own chunk grid.  A window is a rectangle of tiles, so a chunk (adjacent tiles of one row) is
//   kept     every tile inside: its payload bytes and index entry as they are, never read as codewords
//   dropped  no tile inside: the empty coded chunk, ceil((7 + 2 nt) / 8) bytes of a fixed pattern, the input never read
//   cut      a vertical window edge runs through it: at most two per tile row and plane, each with a SLOT (2 * row + side)
// Only a cut chunk is walked, once, from its first tile to its last KEPT tile: the end-of-chunk checks of the decoder are not made, and
// kept and dropped chunks are not walked at all, so a malformation outside the walked part passes through (copied, or dropped) and the
// decoder of the output flags it.
//   check    one workgroup per frame: the decoder's check of the input frame (dec_check_frame)
//   size     one lane per chunk: the index entries of the kept and the dropped chunks
//   recode   one lane per slot (a chunk is serial by design; the slots of the rows a window crosses are adjacent lanes): the cut
//            chunk's kept tiles decoded once into the slot's slab (mask words, then levels)
//   lengths  one wave per slot, a lane per tile: from the slab the code lengths for every k, the choice of k and of raw as the
//            encoder makes it -> the chunk's index entry
//   layout   one workgroup per frame: chunk byte offsets, the frame's size, levels and final status (over-size: kStSize)
//   offsets  the frame offsets (levels.hip)
//   write    one wave per chunk: kept payloads copied (bytes to the first aligned dword of the destination, then dwords funnelled
//            from the source's two, then bytes: no byte of a neighbouring chunk is touched), the dropped pattern, raw cut chunks
//   place    one wave per slot, a lane per tile: a coded cut chunk's codewords from the slab into LDS words, stored bytewise
//   frame    one workgroup per frame: header, types section, index, padding, or 64 zero bytes for a frame that failed
// Every output byte is stored once, by one thread, from the input and the window alone: two calls write the same bytes.

struct WinWs {
  DecWs in;          // the check's view of output frame i's input frame: chunk byte offsets, status, fail, chunk_tiles
  uint32_t* ent;     // [n][max_chunks] the output chunk's index entry: bytes | levels << 16
  uint32_t* ooff;    // [n][max_chunks] its payload's byte offset inside the output frame
  uint32_t* cut;     // [n][slots] a cut chunk's kept levels (kCutFailed: it failed its walk), then its k_dc | k_ac << 3 | raw << 6
  uint32_t* fbytes;  // [n] output frame bytes
  uint32_t* levels;  // [n] output header word 10
  uint64_t* foff;    // [n + 1] frame offsets
  uint8_t* slab;     // [n][slots][slot_bytes] a cut chunk's kept tiles: their mask words, then their levels
};
// two cut chunks per plane and tile row; a slot holds the kept tiles of the largest chunk the call accepts (raw form within the u16)
uint32_t win_slots(const Geom& g) { return 6 * g.ty; }
uint32_t win_slot_bytes(const Geom& g) { return (uint32_t)up16(std::min<uint64_t>(0xFFFEull, (8ull * g.nw + 2ull * g.area) * g.tx)); }
WinWs win_ws(Carver& c, uint32_t n, const Geom& g) {
  WinWs s;
  s.in = dec_ws(c, n, g);
  s.ent = c.take<uint32_t>((uint64_t)n * g.max_chunks);
  s.ooff = c.take<uint32_t>((uint64_t)n * g.max_chunks);
  s.cut = c.take<uint32_t>((uint64_t)n * win_slots(g));
  s.fbytes = c.take<uint32_t>(n);
  s.levels = c.take<uint32_t>(n);
  s.foff = c.take<uint64_t>((uint64_t)n + 1);
  s.slab = c.take<uint8_t>((uint64_t)n * win_slots(g) * win_slot_bytes(g));
  return s;
}
// the worst canonical frame at chunk_tiles 1 (svce_max_bytes with a chunk per tile): what one output frame may take
uint64_t win_max_bytes(const Geom& g) { return up16(g.levels_off + 6ull * g.w * g.h + 4 + 5ull * g.max_chunks); }

struct WinArgs {
  Geom g;
  const uint8_t* in;
  const uint64_t* in_off;
  const uint32_t* src;     // [n_out] input frame of each output frame, or null: its own index
  const uint32_t* window;  // [n_out][4] x, y, w, h in padded coordinates, or null: every tile is kept
  uint8_t* out;
  uint32_t* d_status;
  WinWs ws;
  uint32_t slots, slot_bytes;
  uint64_t worst;          // win_max_bytes
};

__global__ __launch_bounds__(256) void win_check_kernel(DecArgs a, const uint32_t* src, uint32_t n_in) {
  __shared__ uint32_t red[kWaves];
  __shared__ uint32_t s_st;
  const uint32_t i = blockIdx.x, s = src ? src[i] : i;
  dec_check_frame(a, s, s < n_in, i, true, red, &s_st);
}

// an output frame that passed its check: the input frame and what the kernels read of it
struct WinFrame {
  const uint8_t* frame;
  const uint32_t* hdr;
  const uint32_t* index;
  const uint32_t* coff;  // the input chunks' byte offsets
  uint32_t fwords, ct, cx, chunks;
};
__device__ __forceinline__ WinFrame win_frame(const WinArgs& a, uint32_t i) {
  WinFrame w;
  w.frame = a.in + a.in_off[a.src ? a.src[i] : i];
  w.hdr = reinterpret_cast<const uint32_t*>(w.frame);
  w.index = w.hdr + (kHeaderBytes + w.hdr[kETypesBytes]) / 4;
  w.coff = a.ws.in.coff + (size_t)i * a.g.max_chunks;
  w.fwords = w.hdr[kHBytes] / 4;
  w.ct = a.ws.in.chunks[i];
  w.cx = w.ct >= a.g.tx ? 1u : (a.g.tx + w.ct - 1) / w.ct;
  w.chunks = 3 * a.g.ty * w.cx;
  return w;
}

// the tiles of tile row `row` (plane * ty + tile row) whose origin window i contains: [*first, *last) (the rule of gazed())
__device__ __forceinline__ void kept_span(const WinArgs& a, uint32_t i, uint32_t row, uint32_t* first, uint32_t* last) {
  const Geom& g = a.g;
  *first = 0;
  *last = g.tx;
  if (!a.window) return;
  const uint32_t* r = a.window + 4ull * i;
  const uint32_t oy = (row % g.ty) * g.bh;
  if (!(oy >= r[1] && oy - r[1] < r[3])) {
    *last = 0;
    return;
  }
  const uint64_t f = ((uint64_t)r[0] + g.bw - 1) / g.bw, l = ((uint64_t)r[0] + r[2] + g.bw - 1) / g.bw;  // r[2] == 0: l == f
  *first = f < g.tx ? (uint32_t)f : g.tx;
  *last = l < g.tx ? (uint32_t)l : g.tx;
}
// ... and those of a chunk of nt tiles from tile t0, as chunk tiles [*lo, *hi): kept whole when that is [0, nt), dropped when empty
__device__ __forceinline__ void kept_tiles(uint32_t first, uint32_t last, uint32_t t0, uint32_t nt, uint32_t* lo, uint32_t* hi) {
  const uint32_t a = max(first, t0), b = min(last, t0 + nt);
  *lo = a < b ? a - t0 : 0u;
  *hi = a < b ? b - t0 : 0u;
}
// the slot of a cut chunk: side 0 for the chunk that holds the row's first kept tile, side 1 for the other one (it holds the last)
__device__ __forceinline__ uint32_t slot_of(uint32_t row, uint32_t first, uint32_t t0, uint32_t nt) {
  return 2 * row + (first >= t0 && first < t0 + nt ? 0u : 1u);
}

// size: one lane per chunk
__global__ __launch_bounds__(256) void win_size_kernel(WinArgs a) {
  const Geom& g = a.g;
  const uint32_t i = blockIdx.y, c = blockIdx.x * kThreads + threadIdx.x;
  if (c >= g.max_chunks || a.ws.in.status[i] != kStOk) return;
  const WinFrame w = win_frame(a, i);
  if (c >= w.chunks) return;
  uint32_t row, t0, nt, first, last, lo, hi;
  chunk_tiles(g, w.ct, w.cx, c, &row, &t0, &nt);
  kept_span(a, i, row, &first, &last);
  kept_tiles(first, last, t0, nt, &lo, &hi);
  if (hi - lo == nt) a.ws.ent[(size_t)i * g.max_chunks + c] = w.index[c];
  else if (hi == lo) a.ws.ent[(size_t)i * g.max_chunks + c] = (7 + 2 * nt + 7) / 8;
}

// a slot's cut chunk, if it has one
struct CutChunk {
  uint32_t c, t0, nt, lo, hi;
};
__device__ __forceinline__ bool cut_chunk(const WinArgs& a, const WinFrame& w, uint32_t i, uint32_t sl, CutChunk* k) {
  const Geom& g = a.g;
  const uint32_t row = sl >> 1, side = sl & 1u;
  uint32_t first, last;
  kept_span(a, i, row, &first, &last);
  if (first >= last) return false;
  const uint32_t c0 = w.cx == 1 ? 0u : first / w.ct, c1 = w.cx == 1 ? 0u : (last - 1) / w.ct;
  if (side && c1 == c0) return false;
  uint32_t r;
  k->c = row * w.cx + (side ? c1 : c0);
  chunk_tiles(g, w.ct, w.cx, k->c, &r, &k->t0, &k->nt);
  kept_tiles(first, last, k->t0, k->nt, &k->lo, &k->hi);
  return k->hi - k->lo != k->nt;
}

constexpr uint32_t kCutFailed = 0xFFFFFFFFu;  // in WinWs::cut after the walk: the slot's chunk did not pass it (else: its kept levels)

// recode: one lane per slot
__global__ __launch_bounds__(256) void win_recode_kernel(WinArgs a) {
  const Geom& g = a.g;
  const uint32_t i = blockIdx.y, sl = blockIdx.x * kThreads + threadIdx.x;
  if (sl >= a.slots || a.ws.in.status[i] != kStOk) return;
  const WinFrame w = win_frame(a, i);
  CutChunk k;
  if (!cut_chunk(a, w, i, sl, &k)) return;
  const uint32_t entry = w.index[k.c], size = entry & 0xFFFFu, count = entry >> 16, start = w.coff[k.c];
  const uint8_t* frame = w.frame;
  uint8_t* masks = a.ws.slab + ((size_t)i * a.slots + sl) * a.slot_bytes;
  int16_t* lev = reinterpret_cast<int16_t*>(masks + 8ull * g.nw * (k.hi - k.lo));
  uint32_t kept = 0;  // levels in the slab
  bool ok = size != 0;
  if (ok && (frame[start] & 1u)) {  // raw: the kept tiles' mask words and levels as they are
    const uint32_t mbytes = 8 * g.nw * k.nt;
    ok = (uint64_t)size == 1ull + mbytes + 2ull * count;
    const uint8_t* lv = frame + start + 1 + mbytes;
    uint32_t got = 0;
    for (uint32_t x = 0; ok && x < k.hi * g.nw; ++x) {
      const uint8_t* s = frame + start + 1 + 8 * x;
      uint64_t m = 0;
      for (uint32_t b = 0; b < 8; ++b) m |= (uint64_t)s[b] << (8 * b);
      const uint32_t j = x % g.nw;
      const uint32_t valid = min(64u, g.area - 64 * j);
      if (valid < 64 && (m >> valid)) ok = false;
      const uint32_t pc = (uint32_t)__popcll(m);
      if (ok && got + pc > count) ok = false;  // more mask bits than levels: nothing is read past the chunk
      if (!ok) break;
      if (x >= k.lo * g.nw) {
        store_mask(masks + 8 * (x - k.lo * g.nw), m);
        for (uint32_t e = 0; e < pc; ++e) lev[kept++] = (int16_t)((uint32_t)lv[2 * (got + e)] | ((uint32_t)lv[2 * (got + e) + 1] << 8));
      }
      got += pc;
    }
  } else if (ok) {
    BitReader r{w.hdr, w.fwords, 0, 0, 0, 0};
    const uint64_t end = 8ull * (start + size);
    uint64_t pos = 8ull * start;
    const uint32_t head = (uint32_t)r.peek(pos);
    const uint32_t kd = (head >> 1) & 7u, ka = (head >> 4) & 7u;
    pos += 7;
    r.seek(pos);
    uint32_t written = 0;
    int32_t dcp = 0;
    for (uint32_t t = 0; ok && t < k.hi; ++t) {
      const bool keep = t >= k.lo;
      uint8_t* tm = masks + 8ull * (keep ? t - k.lo : 0u) * g.nw;
      uint32_t u;
      ok = get_eg(r, &pos, end, kd, &u);
      if (!ok) break;
      const int32_t dc = dcp + unsgn(u);
      dcp = dc;
      ok = dc >= -32768 && dc <= 32767;
      uint64_t cur = 0;  // the mask word being filled, word cj of the tile
      uint32_t cj = 0;
      if (ok && dc != 0) {
        ok = written < count;
        if (ok) {
          ++written;
          if (keep) lev[kept++] = (int16_t)dc;
        }
        cur = 1;
      }
      uint32_t nac = 0;
      ok = ok && get_eg(r, &pos, end, 0, &nac) && nac <= g.area - 1;
      uint32_t p = 0;
      for (uint32_t x = 0; ok && x < nac; ++x) {
        uint32_t run, lu;
        ok = get_eg(r, &pos, end, 0, &run) && (uint64_t)p + run + 1 <= g.area - 1;
        if (!ok) break;
        p += run + 1;
        ok = get_eg(r, &pos, end, ka, &lu);
        if (!ok) break;
        const int32_t v = unsgn(lu);
        ok = v >= -32768 && v <= 32767 && written < count;
        if (!ok) break;
        ++written;
        if (!keep) continue;
        lev[kept++] = (int16_t)v;
        for (; cj < (p >> 6); ++cj) {
          store_mask(tm + 8 * cj, cur);
          cur = 0;
        }
        cur |= 1ull << (p & 63u);
      }
      if (!ok || !keep) continue;
      for (; cj < g.nw; ++cj) {
        store_mask(tm + 8 * cj, cur);
        cur = 0;
      }
    }
  }
  if (!ok) {
    atomicOr(&a.ws.in.fail[i], 1u);
    a.ws.cut[(size_t)i * a.slots + sl] = kCutFailed;
    return;
  }
  a.ws.cut[(size_t)i * a.slots + sl] = kept;
}

// the wave's trip over a cut chunk's tiles, 64 at a time, a lane per tile: fn(t, keep, masks, lev) with the tile's mask words and first
// level in the slab for a tile inside the window (keep), nothing to read for one outside it.  Every lane of the wave calls fn.
template <typename Fn>
__device__ __forceinline__ void for_each_cut_tile(const Geom& g, const CutChunk& k, const uint8_t* slab, uint32_t lane, Fn fn) {
  const int16_t* lev = reinterpret_cast<const int16_t*>(slab + 8ull * g.nw * (k.hi - k.lo));
  uint32_t before = 0;  // levels of the tiles of earlier trips
  for (uint32_t base = 0; base < k.nt; base += 64) {
    const uint32_t t = base + lane;
    const bool keep = t >= k.lo && t < k.hi;
    const uint8_t* tm = slab + 8ull * g.nw * (keep ? t - k.lo : 0u);
    const uint32_t mine = keep ? tile_levels(g, tm) : 0u;
    const uint32_t first = before + wave_exclusive_scan(mine);
    before += wave_sum(mine);
    fn(t, keep, tm, lev + first);
  }
}

// lengths: one wave per slot, a lane per tile -> the cut chunk's k_dc, k_ac, raw and index entry, as enc_lengths_kernel chooses them for
// the chunk with every tile outside the window all zero
__global__ __launch_bounds__(64) void win_lengths_kernel(WinArgs a) {
  const Geom& g = a.g;
  const uint32_t i = blockIdx.y, sl = blockIdx.x, lane = threadIdx.x;
  if (a.ws.in.status[i] != kStOk) return;
  const WinFrame w = win_frame(a, i);
  CutChunk k;
  if (!cut_chunk(a, w, i, sl, &k)) return;
  const uint32_t kept = a.ws.cut[(size_t)i * a.slots + sl];
  if (kept == kCutFailed) return;
  const uint8_t* slab = a.ws.slab + ((size_t)i * a.slots + sl) * a.slot_bytes;
  uint32_t dc_bits[8] = {}, ac_bits[8] = {};
  uint32_t fixed = 0, forced = 0;
  int32_t dc_before = 0;  // the DC of the last tile of the trip before
  for_each_cut_tile(g, k, slab, lane, [&](uint32_t t, bool keep, const uint8_t* tm, const int16_t* lev) {
    int32_t dc = 0;
    uint32_t prev = 0, nac = 0;
    if (keep)
      for_each_level(g, tm, lev, [&](uint32_t p, int32_t v) {
        forced |= v == 0;
        if (p == 0) { dc = v; return; }
        ++nac;
        fixed += eg_len(p - prev - 1, 0);
        prev = p;
        const uint32_t u = sgn(v);
        for (uint32_t q = 0; q < 8; ++q) ac_bits[q] += eg_len(u, q);
      });
    const int32_t left = __shfl_up(dc, 1, 64);
    if (t < k.nt) {
      fixed += eg_len(nac, 0);
      const uint32_t u = sgn(dc - (lane == 0 ? dc_before : left));
      for (uint32_t q = 0; q < 8; ++q) dc_bits[q] += eg_len(u, q);
    }
    dc_before = __shfl(dc, 63, 64);
  });
  fixed = wave_sum(fixed);
  forced = wave_sum(forced);
  uint32_t best_dc = 0, best_ac = 0, kd = 0, ka = 0;
  for (uint32_t q = 0; q < 8; ++q) {
    const uint32_t d = wave_sum(dc_bits[q]), s = wave_sum(ac_bits[q]);
    if (q == 0 || d < best_dc) { best_dc = d; kd = q; }
    if (q == 0 || s < best_ac) { best_ac = s; ka = q; }
  }
  if (lane == 0) {
    const uint32_t coded = (7 + fixed + best_dc + best_ac + 7) / 8;
    const uint32_t raw = 1 + 8 * g.nw * k.nt + 2 * kept;
    const bool use_raw = forced || raw < coded;
    a.ws.ent[(size_t)i * g.max_chunks + k.c] = (use_raw ? raw : coded) | (kept << 16);
    a.ws.cut[(size_t)i * a.slots + sl] = kd | (ka << 3) | ((use_raw ? 1u : 0u) << 6);
  }
}

// layout: one workgroup per frame -> chunk byte offsets, the frame's bytes and levels, its final status
__global__ __launch_bounds__(256) void win_layout_kernel(WinArgs a) {
  __shared__ uint32_t red[kWaves];
  const Geom& g = a.g;
  const uint32_t i = blockIdx.x;
  uint32_t st = a.ws.in.status[i];
  if (st == kStOk && a.ws.in.fail[i]) st = kStChunk;
  uint64_t bytes = kHeaderBytes;
  uint32_t lev = 0;
  if (st == kStOk) {
    const WinFrame w = win_frame(a, i);
    const uint32_t* ent = a.ws.ent + (size_t)i * g.max_chunks;
    bytes = kHeaderBytes + (uint64_t)w.hdr[kETypesBytes] + 4ull * w.chunks;  // (64 bits: kept chunks may be of any size)
    for (uint32_t base = 0; base < w.chunks; base += kThreads) {
      const uint32_t c = base + threadIdx.x;
      const uint32_t v = c < w.chunks ? ent[c] : 0u;
      uint32_t tb, tl;
      const uint32_t eb = block_exclusive_scan(v & 0xFFFFu, red, &tb);
      (void)block_exclusive_scan(v >> 16, red, &tl);
      if (c < w.chunks) a.ws.ooff[(size_t)i * g.max_chunks + c] = (uint32_t)(bytes + eb);  // read only for a frame within a.worst
      bytes += tb;
      lev += tl;
    }
    bytes = up16(bytes);
    if (bytes > a.worst) {  // kept chunks above their raw form: nothing of this frame is written
      st = kStSize;
      bytes = kHeaderBytes;
    }
  }
  if (threadIdx.x == 0) {
    a.ws.in.status[i] = st;
    a.d_status[i] = st;
    a.ws.fbytes[i] = (uint32_t)bytes;
    a.ws.levels[i] = lev;
  }
}

// a wave copies `size` bytes from byte sb of the frame's dwords to dst, whatever the two byte phases: single bytes up to dst's first
// aligned dword, then dwords funnelled from the source's two, then single bytes
__device__ __forceinline__ void copy_payload(const WinFrame& w, uint32_t sb, uint32_t size, uint8_t* dst, uint32_t lane) {
  const uint8_t* src = w.frame + sb;
  const uint32_t head = min(size, (4u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u), body = (size - head) / 4;
  if (lane < head) dst[lane] = src[lane];
  uint32_t* d32 = reinterpret_cast<uint32_t*>(dst + head);
  const uint32_t s0 = (sb + head) >> 2, sh = 8 * ((sb + head) & 3u);
  for (uint32_t x = lane; x < body; x += 64) {
    const uint64_t two = (uint64_t)w.hdr[s0 + x] | (sh && s0 + x + 1 < w.fwords ? (uint64_t)w.hdr[s0 + x + 1] << 32 : 0ull);
    d32[x] = (uint32_t)(two >> sh);
  }
  const uint32_t done = head + 4 * body;
  if (lane < size - done) dst[done + lane] = src[done + lane];
}

// write: one wave per chunk
__global__ __launch_bounds__(256) void win_write_kernel(WinArgs a) {
  const Geom& g = a.g;
  const uint32_t i = blockIdx.y, c = blockIdx.x * kWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (c >= g.max_chunks || a.ws.in.status[i] != kStOk) return;
  const WinFrame w = win_frame(a, i);
  if (c >= w.chunks) return;
  uint32_t row, t0, nt, first, last, lo, hi;
  chunk_tiles(g, w.ct, w.cx, c, &row, &t0, &nt);
  kept_span(a, i, row, &first, &last);
  kept_tiles(first, last, t0, nt, &lo, &hi);
  const uint32_t size = a.ws.ent[(size_t)i * g.max_chunks + c] & 0xFFFFu;
  uint8_t* dst = a.out + a.ws.foff[i] + a.ws.ooff[(size_t)i * g.max_chunks + c];
  if (hi - lo == nt) {
    copy_payload(w, w.coff[c], size, dst, lane);
  } else if (hi == lo) {  // coded, k_dc = k_ac = 0, then two 1 bits per tile: bits [7, 7 + 2 nt) set
    for (uint32_t b = lane; b < size; b += 64) {
      const uint32_t from = b == 0 ? 7u : 0u, to = min(8u, 7 + 2 * nt - 8 * b);
      dst[b] = (uint8_t)(((1u << to) - 1u) & ~((1u << from) - 1u));
    }
  } else {
    const uint32_t sl = slot_of(row, first, t0, nt);
    if (!(a.ws.cut[(size_t)i * a.slots + sl] >> 6)) return;  // coded: the place kernel's
    // raw: the mode byte, the chunk's mask words (zero outside the window), the kept levels
    const uint8_t* slab = a.ws.slab + ((size_t)i * a.slots + sl) * a.slot_bytes;
    const uint32_t tb = 8 * g.nw, mbytes = tb * nt, kb = tb * (hi - lo);
    for (uint32_t b = lane; b < size; b += 64) {
      uint8_t v = 1;
      if (b > mbytes) v = slab[kb + (b - 1 - mbytes)];
      else if (b > 0) v = b - 1 >= tb * lo && b - 1 < tb * hi ? slab[b - 1 - tb * lo] : (uint8_t)0;
      dst[b] = v;
    }
  }
}

// place: one wave per slot, a lane per tile -> a coded cut chunk's codewords ORed into the wave's LDS words as enc_scatter_kernel
// places them, then stored bytewise (the chunk shares its first and last dword with its neighbours)
__global__ __launch_bounds__(64) void win_place_kernel(WinArgs a) {
  extern __shared__ uint32_t lds[];
  const Geom& g = a.g;
  const uint32_t i = blockIdx.y, sl = blockIdx.x, lane = threadIdx.x;
  if (a.ws.in.status[i] != kStOk) return;
  const WinFrame w = win_frame(a, i);
  CutChunk k;
  if (!cut_chunk(a, w, i, sl, &k)) return;
  const uint32_t info = a.ws.cut[(size_t)i * a.slots + sl], kd = info & 7u, ka = (info >> 3) & 7u;
  if (info >> 6) return;  // raw: the write kernel's
  const uint32_t size = a.ws.ent[(size_t)i * g.max_chunks + k.c] & 0xFFFFu;
  const uint8_t* slab = a.ws.slab + ((size_t)i * a.slots + sl) * a.slot_bytes;
  for (uint32_t x = lane; x < size / 4 + 1; x += 64) lds[x] = 0;
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  if (lane == 0) put_bits(lds, 0, (kd << 1) | (ka << 4));
  uint32_t bits_before = 7;
  int32_t dc_before = 0;
  for_each_cut_tile(g, k, slab, lane, [&](uint32_t t, bool keep, const uint8_t* tm, const int16_t* lev) {
    int32_t dc = 0;
    uint32_t len = 0, nac = 0, prev = 0;
    if (keep)
      for_each_level(g, tm, lev, [&](uint32_t p, int32_t v) {
        if (p == 0) { dc = v; return; }
        ++nac;
        len += eg_len(p - prev - 1, 0) + eg_len(sgn(v), ka);
        prev = p;
      });
    const int32_t left = __shfl_up(dc, 1, 64);
    const uint32_t udc = sgn(dc - (lane == 0 ? dc_before : left));
    dc_before = __shfl(dc, 63, 64);
    len = t < k.nt ? len + eg_len(nac, 0) + eg_len(udc, kd) : 0u;
    uint32_t pos = bits_before + wave_exclusive_scan(len);
    bits_before += wave_sum(len);
    if (t >= k.nt) return;
    pos += put_eg(lds, pos, udc, kd);
    pos += put_eg(lds, pos, nac, 0);
    if (!keep) return;
    prev = 0;
    for_each_level(g, tm, lev, [&](uint32_t p, int32_t v) {
      if (p == 0) return;
      pos += put_eg(lds, pos, p - prev - 1, 0);
      pos += put_eg(lds, pos, sgn(v), ka);
      prev = p;
    });
  });
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  uint8_t* dst = a.out + a.ws.foff[i] + a.ws.ooff[(size_t)i * g.max_chunks + k.c];
  const uint8_t* bytes = reinterpret_cast<const uint8_t*>(lds);
  for (uint32_t x = lane; x < size; x += 64) dst[x] = bytes[x];
}

// frame: one workgroup per frame -> header, types section, index, padding, or 64 zero bytes for a frame that failed
__global__ __launch_bounds__(256) void win_frame_kernel(WinArgs a) {
  const Geom& g = a.g;
  const uint32_t i = blockIdx.x;
  uint8_t* frame = a.out + a.ws.foff[i];
  uint32_t* fw = reinterpret_cast<uint32_t*>(frame);
  if (a.ws.in.status[i] != kStOk) {
    if (threadIdx.x < kHeaderWords) fw[threadIdx.x] = 0;
    return;
  }
  const WinFrame w = win_frame(a, i);
  const uint32_t fbytes = a.ws.fbytes[i], lev = a.ws.levels[i], twords = w.hdr[kETypesBytes] / 4;
  if (threadIdx.x < kHeaderWords) {
    uint32_t v = w.hdr[threadIdx.x];
    if (threadIdx.x == kHLevels) v = lev;
    if (threadIdx.x == kHBytes) v = fbytes;
    if (threadIdx.x == kESvcqBytes) v = (uint32_t)up16(g.levels_off + 2ull * lev);
    fw[threadIdx.x] = v;
  }
  for (uint32_t x = threadIdx.x; x < twords; x += kThreads) fw[kHeaderWords + x] = w.hdr[kHeaderWords + x];
  const uint32_t* ent = a.ws.ent + (size_t)i * g.max_chunks;
  for (uint32_t c = threadIdx.x; c < w.chunks; c += kThreads) fw[kHeaderWords + twords + c] = ent[c];
  const uint32_t last = w.chunks - 1;
  const uint32_t used = a.ws.ooff[(size_t)i * g.max_chunks + last] + (ent[last] & 0xFFFFu);
  for (uint32_t b = used + threadIdx.x; b < fbytes; b += kThreads) frame[b] = 0;
}

// geometry, then the limits with SVCE's worst case (make_geom divides by the tile area: only for a tile within the limit)
int validate(const char* what, uint32_t n, uint32_t w, uint32_t h, uint32_t bw, uint32_t bh, uint32_t mvbw, uint32_t mvbh) {
  const int rc = validate_geom(what, w, h, bw, bh, mvbw, mvbh);
  if (rc) return rc;
  const bool tile_ok = (uint64_t)bw * bh <= kMaxTileCoeffs;
  return validate_limits(what, n, w, h, bw, bh, tile_ok ? svce_max_bytes(make_geom(w, h, bw, bh, mvbw, mvbh)) : 0);
}

// the fused decode's geometry (what the reconstruction takes), then the limits with SVCE's worst case
int validate_fused(const char* what, uint32_t n, uint32_t w, uint32_t h, uint32_t bw, uint32_t bh, uint32_t mvbw, uint32_t mvbh) {
  const int rc = validate_decode_geom(what, w, h, bw, bh, mvbw, mvbh);
  if (rc) return rc;
  return validate_limits(what, n, w, h, bw, bh, svce_max_bytes(make_geom(w, h, bw, bh, mvbw, mvbh)));
}

// the window call's limits: the entropy coder's, with the window call's own worst frame
int validate_window(const char* what, uint32_t n, uint32_t w, uint32_t h, uint32_t bw, uint32_t bh, uint32_t mvbw, uint32_t mvbh) {
  const int rc = validate_geom(what, w, h, bw, bh, mvbw, mvbh);
  if (rc) return rc;
  const bool tile_ok = (uint64_t)bw * bh <= kMaxTileCoeffs;
  return validate_limits(what, n, w, h, bw, bh, tile_ok ? win_max_bytes(make_geom(w, h, bw, bh, mvbw, mvbh)) : 0);
}

}  // namespace
}  // namespace svc

using namespace svc;

extern "C" {

uint64_t svc_hip_entropy_max_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h, uint32_t block_w, uint32_t block_h,
                                   uint32_t mv_block_w, uint32_t mv_block_h) {
  if (validate("entropy_max_bytes", n_frames, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h)) return 0;
  return n_frames * svce_max_bytes(make_geom(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h));
}

uint64_t svc_hip_entropy_workspace_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h, uint32_t block_w, uint32_t block_h,
                                         uint32_t mv_block_w, uint32_t mv_block_h) {
  if (validate("entropy_workspace_bytes", n_frames, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h)) return 0;
  return coder_ws_need(n_frames, make_geom(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h));
}

// Checked in the order of the SVCQ entry points, for any n_frames: geometry, limits, sizes, then pointers.
int svc_hip_entropy_encode_frames(const uint8_t* d_svcq, uint64_t svcq_bytes, const uint64_t* d_svcq_offsets, uint32_t n_frames,
                                  uint32_t frame_w, uint32_t frame_h, uint32_t block_w, uint32_t block_h, uint32_t mv_block_w,
                                  uint32_t mv_block_h, uint8_t* d_workspace, uint64_t workspace_bytes, uint8_t* d_out,
                                  uint64_t out_capacity, uint64_t* d_out_offsets, uint32_t* d_status, void* stream) {
  int rc = validate("entropy_encode", n_frames, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if (rc) return rc;
  const Geom g = make_geom(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if ((rc = require_workspace("entropy_encode", workspace_bytes, coder_ws_need(n_frames, g)))) return rc;
  if ((rc = require_capacity("entropy_encode", "output", out_capacity, n_frames * svce_max_bytes(g)))) return rc;
  if (n_frames == 0) return SVC_OK;
  SVC_REQUIRE(d_svcq && d_svcq_offsets && d_workspace && d_out && d_out_offsets && d_status, "entropy_encode: null pointer");
  SVC_REQUIRE(aligned(d_svcq, 16) && aligned(d_out, 16) && aligned(d_workspace, 16) && aligned(d_svcq_offsets, 8) &&
                  aligned(d_out_offsets, 8) && aligned(d_status, 4),
              "entropy_encode: frames, output and workspace must be 16-byte aligned, offsets 8-byte, status 4-byte");
  const EncArgs a{g, d_svcq, svcq_bytes, d_svcq_offsets, d_out, d_out_offsets, d_status, carve(d_workspace, enc_ws, n_frames, g), n_frames};
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 chunk_grid(div_up(g.chunks, kWaves), n_frames);
  hipLaunchKernelGGL(enc_count_kernel, chunk_grid, dim3(kThreads), 0, s, a);
  if ((rc = check_launch("entropy_encode count"))) return rc;
  hipLaunchKernelGGL(enc_scan_kernel, dim3(n_frames), dim3(kThreads), 0, s, a);
  if ((rc = check_launch("entropy_encode scan"))) return rc;
  hipLaunchKernelGGL(enc_lengths_kernel, chunk_grid, dim3(kThreads), 0, s, a);
  if ((rc = check_launch("entropy_encode lengths"))) return rc;
  hipLaunchKernelGGL(enc_layout_kernel, dim3(n_frames), dim3(kThreads), 0, s, a);
  if ((rc = check_launch("entropy_encode layout"))) return rc;
  if ((rc = enqueue_frame_offsets("entropy_encode", 1, OffsetsJob{a.ws.fbytes, a.ws.foff, d_out_offsets}, OffsetsJob{}, n_frames, stream))) return rc;
  const uint32_t lds_words = div_up(g.max_chunk_bytes, 4) + 2;
  hipLaunchKernelGGL(enc_scatter_kernel, chunk_grid, dim3(kThreads), kWaves * lds_words * 4, s, a, lds_words);
  if ((rc = check_launch("entropy_encode scatter"))) return rc;
  hipLaunchKernelGGL(enc_frame_kernel, dim3(n_frames), dim3(kThreads), 0, s, a);
  return check_launch("entropy_encode frame");
}

int svc_hip_entropy_decode_frames(const uint8_t* d_svce, uint64_t svce_bytes, const uint64_t* d_offsets, uint32_t n_frames,
                                  uint32_t frame_w, uint32_t frame_h, uint32_t block_w, uint32_t block_h, uint32_t mv_block_w,
                                  uint32_t mv_block_h, uint8_t* d_workspace, uint64_t workspace_bytes, uint8_t* d_svcq_out,
                                  uint64_t capacity, uint64_t* d_svcq_offsets, uint32_t* d_status, void* stream) {
  int rc = validate("entropy_decode", n_frames, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if (rc) return rc;
  const Geom g = make_geom(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if ((rc = require_workspace("entropy_decode", workspace_bytes, coder_ws_need(n_frames, g)))) return rc;
  const uint64_t need = n_frames * frame_layout(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h).max_bytes;
  SVC_REQUIRE(capacity >= need, "entropy_decode: output of %llu B is below the batch's SVCQ worst case of %llu B",
              (unsigned long long)capacity, (unsigned long long)need);
  if (n_frames == 0) return SVC_OK;
  SVC_REQUIRE(d_svce && d_offsets && d_workspace && d_svcq_out && d_svcq_offsets && d_status, "entropy_decode: null pointer");
  SVC_REQUIRE(aligned(d_svce, 16) && aligned(d_svcq_out, 16) && aligned(d_workspace, 16) && aligned(d_offsets, 8) &&
                  aligned(d_svcq_offsets, 8) && aligned(d_status, 4),
              "entropy_decode: frames, output and workspace must be 16-byte aligned, offsets 8-byte, status 4-byte");
  const DecArgs a{g, d_svce, svce_bytes, d_offsets, d_svcq_out, d_svcq_offsets, d_status, carve(d_workspace, dec_ws, n_frames, g), n_frames};
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(dec_check_kernel, dim3(n_frames), dim3(kThreads), 0, s, a);
  if ((rc = check_launch("entropy_decode check"))) return rc;
  if ((rc = enqueue_frame_offsets("entropy_decode", 1, OffsetsJob{a.ws.qbytes, a.ws.qoff, d_svcq_offsets}, OffsetsJob{}, n_frames, stream))) return rc;
  hipLaunchKernelGGL(dec_chunks_kernel, dim3(div_up(g.max_chunks, kThreads), n_frames), dim3(kThreads), 0, s, a);
  if ((rc = check_launch("entropy_decode chunks"))) return rc;
  hipLaunchKernelGGL(dec_frame_kernel, dim3(n_frames), dim3(kThreads), 0, s, a);
  return check_launch("entropy_decode frame");
}

// The drain of levels.hip for SVCE frames, with their worst case as the capacity rule.  Checked as an SVCQ geometry first; SVCE's own
// limit is then reported as svc_hip_entropy_max_bytes reports it (an empty batch needs no room and is not refused for it).
int svc_hip_entropy_drain(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t frame_w,
                          uint32_t frame_h, uint32_t block_w, uint32_t block_h, uint32_t mv_block_w, uint32_t mv_block_h,
                          void* host_dst, uint64_t capacity, void* stream) {
  int rc = validate_geom("entropy_drain", frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if (!rc) rc = validate_limits("entropy_drain", n_frames, frame_w, frame_h, block_w, block_h,
                                frame_layout(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h).max_bytes);
  if (rc) return rc;
  const uint64_t worst = svce_max_bytes(make_geom(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h));
  if ((rc = validate_limits("entropy_max_bytes", n_frames, frame_w, frame_h, block_w, block_h, worst)) && n_frames != 0) return rc;
  return drain_to_host("entropy_drain", d_frames, d_frame_offsets, n_frames, host_dst, capacity, n_frames * worst, stream);
}

uint64_t svc_hip_decode_entropy_workspace_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h, uint32_t block_w, uint32_t block_h,
                                                uint32_t mv_block_w, uint32_t mv_block_h) {
  if (validate_fused("decode_entropy_workspace_bytes", n_frames, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h)) return 0;
  return fused_ws_need(n_frames, make_geom(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h));
}

// Checked in the order of svc_hip_decode_levels_frames, for any n_frames: geometry, steps, display size, limits, workspace, pointers.
int svc_hip_decode_entropy_frames(const uint8_t* d_svce, uint64_t svce_bytes, const uint64_t* d_offsets, uint32_t n_frames,
                                  uint32_t frame_w, uint32_t frame_h, uint32_t block_w, uint32_t block_h, uint32_t mv_block_w,
                                  uint32_t mv_block_h, uint32_t fg_step, uint32_t bg_step, const uint32_t* d_gaze, uint8_t* d_workspace,
                                  uint64_t workspace_bytes, float* d_rec, uint8_t* d_display, uint32_t display_w, uint32_t display_h,
                                  uint32_t* d_status, void* stream) {
  int rc = validate_decode_geom("decode_entropy", frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if (rc) return rc;
  bool display;
  if ((rc = validate_steps_display("decode_entropy", fg_step, bg_step, display_w, display_h, frame_w, frame_h, &display))) return rc;
  if ((rc = validate_fused("decode_entropy", n_frames, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h))) return rc;
  const Geom g = make_geom(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if ((rc = require_workspace("decode_entropy", workspace_bytes, fused_ws_need(n_frames, g)))) return rc;
  if (n_frames == 0) return SVC_OK;
  SVC_REQUIRE(d_svce && d_offsets && d_workspace && d_rec && d_status, "decode_entropy: null pointer");
  if ((rc = validate_display_buffer("decode_entropy", display, d_display))) return rc;
  SVC_REQUIRE(aligned(d_svce, 16) && aligned(d_workspace, 16) && aligned(d_offsets, 8) && aligned(d_rec, 4) && aligned(d_status, 4) &&
                  aligned(d_gaze, 4),
              "decode_entropy: frames and workspace must be 16-byte aligned, offsets 8-byte, output, gaze and status 4-byte");
  const DecWs ws = carve(d_workspace, dec_ws, n_frames, g);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the header, types and index checks and the index scan of svc_hip_entropy_decode_frames (it writes no output)
  const DecArgs c{g, d_svce, svce_bytes, d_offsets, nullptr, nullptr, nullptr, ws, n_frames};
  hipLaunchKernelGGL(dec_check_kernel, dim3(n_frames), dim3(kThreads), 0, s, c);
  if ((rc = check_launch("decode_entropy check"))) return rc;
  const FusedArgs a{g, d_svce, d_offsets, d_gaze, d_rec, d_status, ws, (float)fg_step, (float)bg_step};
  const dim3 grid(g.ty * g.cx, n_frames);
  if (block_w == 8) hipLaunchKernelGGL(decode_entropy_kernel<8>, grid, dim3(kThreads), 0, s, a);
  else hipLaunchKernelGGL(decode_entropy_kernel<16>, grid, dim3(kThreads), 0, s, a);
  if ((rc = check_launch("decode_entropy reconstruction"))) return rc;
  hipLaunchKernelGGL(decode_entropy_finish_kernel, dim3(32, n_frames), dim3(kThreads), 0, s, a);
  return finish_with_display("decode_entropy", "finish", display, d_rec, d_display, n_frames, frame_w, frame_h, display_w, display_h, s);
}

uint64_t svc_hip_window_entropy_max_bytes(uint32_t n_out, uint32_t frame_w, uint32_t frame_h, uint32_t block_w, uint32_t block_h,
                                          uint32_t mv_block_w, uint32_t mv_block_h) {
  if (validate_window("window_entropy_max_bytes", n_out, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h)) return 0;
  return n_out * win_max_bytes(make_geom(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h));
}

uint64_t svc_hip_window_entropy_workspace_bytes(uint32_t n_out, uint32_t frame_w, uint32_t frame_h, uint32_t block_w, uint32_t block_h,
                                                uint32_t mv_block_w, uint32_t mv_block_h) {
  if (validate_window("window_entropy_workspace_bytes", n_out, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h)) return 0;
  return n_out ? layout_bytes(win_ws, n_out, make_geom(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h)) : 0;
}

// Checked in the order of svc_hip_window_levels_frames, for any frame counts: geometry, limits, the d_src rule, sizes, then pointers.
int svc_hip_window_entropy_frames(const uint8_t* d_svce, uint64_t svce_bytes, const uint64_t* d_offsets, uint32_t n_in,
                                  const uint32_t* d_src, uint32_t n_out, uint32_t frame_w, uint32_t frame_h, uint32_t block_w,
                                  uint32_t block_h, uint32_t mv_block_w, uint32_t mv_block_h, const uint32_t* d_window,
                                  uint8_t* d_workspace, uint64_t workspace_bytes, uint8_t* d_out, uint64_t out_capacity,
                                  uint64_t* d_out_offsets, uint32_t* d_status, void* stream) {
  int rc = validate_window("window_entropy", std::max(n_out, n_in), frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if (rc) return rc;
  SVC_REQUIRE(d_src || n_out == n_in, "window_entropy: without d_src output frame i is input frame i, but n_out is %u and n_in %u", n_out,
              n_in);
  const Geom g = make_geom(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if ((rc = require_workspace("window_entropy", workspace_bytes, n_out ? layout_bytes(win_ws, n_out, g) : 0))) return rc;
  if ((rc = require_capacity("window_entropy", "output", out_capacity, n_out * win_max_bytes(g)))) return rc;
  if (n_out == 0) return SVC_OK;
  SVC_REQUIRE(d_svce && d_offsets && d_workspace && d_out && d_out_offsets && d_status, "window_entropy: null pointer");
  SVC_REQUIRE(aligned(d_svce, 16) && aligned(d_out, 16) && aligned(d_workspace, 16) && aligned(d_offsets, 8) && aligned(d_out_offsets, 8) &&
                  aligned(d_src, 4) && aligned(d_window, 4) && aligned(d_status, 4),
              "window_entropy: streams and workspace must be 16-byte aligned, offsets 8-byte, source indices, windows and status 4-byte");
  const WinWs ws = carve(d_workspace, win_ws, n_out, g);
  const DecArgs c{g, d_svce, svce_bytes, d_offsets, nullptr, nullptr, nullptr, ws.in, n_out};
  const WinArgs a{g, d_svce, d_offsets, d_src, d_window, d_out, d_status, ws, win_slots(g), win_slot_bytes(g), win_max_bytes(g)};
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 lanes(div_up(g.max_chunks, kThreads), n_out), slots(div_up(a.slots, kThreads), n_out);
  hipLaunchKernelGGL(win_check_kernel, dim3(n_out), dim3(kThreads), 0, s, c, d_src, n_in);
  if ((rc = check_launch("window_entropy check"))) return rc;
  hipLaunchKernelGGL(win_size_kernel, lanes, dim3(kThreads), 0, s, a);
  if ((rc = check_launch("window_entropy size"))) return rc;
  hipLaunchKernelGGL(win_recode_kernel, slots, dim3(kThreads), 0, s, a);
  if ((rc = check_launch("window_entropy recode"))) return rc;
  hipLaunchKernelGGL(win_lengths_kernel, dim3(a.slots, n_out), dim3(64), 0, s, a);
  if ((rc = check_launch("window_entropy lengths"))) return rc;
  hipLaunchKernelGGL(win_layout_kernel, dim3(n_out), dim3(kThreads), 0, s, a);
  if ((rc = check_launch("window_entropy layout"))) return rc;
  if ((rc = enqueue_frame_offsets("window_entropy", 1, OffsetsJob{ws.fbytes, ws.foff, d_out_offsets}, OffsetsJob{}, n_out, stream))) return rc;
  hipLaunchKernelGGL(win_write_kernel, dim3(div_up(g.max_chunks, kWaves), n_out), dim3(kThreads), 0, s, a);
  if ((rc = check_launch("window_entropy write"))) return rc;
  // the wave's LDS holds the largest coded chunk of this geometry: at most its raw form, at most the index's u16
  const uint32_t place_lds = (uint32_t)std::min<uint64_t>(65536, (1 + (8ull * g.nw + 2ull * g.area) * g.tx) / 4 * 4 + 8);
  hipLaunchKernelGGL(win_place_kernel, dim3(a.slots, n_out), dim3(64), place_lds, s, a);
  if ((rc = check_launch("window_entropy place"))) return rc;
  hipLaunchKernelGGL(win_frame_kernel, dim3(n_out), dim3(kThreads), 0, s, a);
  return check_launch("window_entropy frame");
}

}  // extern "C"
