// levels.hip -- the compact quantised-coefficient stream ("SVCQ", version 1): pack, unpack, drain.
//
// Quantised planes are almost all zeros (a C3 background tile-channel holds about one non-zero level), so a frame is sent as
// a significance mask per tile plus the non-zero levels as int16 -- about 1 MB instead of the 25 MB of f32 planes at 1080p.
// stream_format.hpp states the frame's layout, its header and the check of a frame, and the steps this file shares with dct_pack.hip and
// entropy.hip: a workspace as one layout function (Carver), scan_counts, frame_offset_to_lds, write_frame_edges, store_level_run,
// mask_words.  include/svc_hip.h has the table.
//
// Work split, pack and unpack alike: a workgroup owns a GROUP = one plane, one tile row, up to `tpg` adjacent tiles (about 2048
// coefficients).  It stages the group's rows in LDS with 16-byte loads (the planes are row-major: one 8x8 tile per wave would
// read 32-byte pieces), then one wave per 64-coefficient mask word: the word is a __ballot, a lane's rank among the non-zero
// levels is mbcnt + the popcounts of the earlier words.  The only variable-size section is the levels, so each direction is
//   count   (per group: non-zero levels)  ->  scan (per frame: exclusive scan of the group sums, frame size)  ->  scatter.
// The pack's frame offsets are not scanned by a kernel of their own: the scatter's workgroup sums the frame sizes before its own
// frame (a batch is a few dozen frames).  The window call, the split and entropy.hip, whose frame sizes come from a kernel of their own,
// share frame_offsets_kernel (enqueue_frame_offsets).  Group order = (plane, tile row, group in the row) = the order of the levels.
//
// budgeted pack (rate control): a count per ladder entry, a per-frame choice of steps from a byte budget, then the pack's count,
// scan and scatter with each frame's chosen steps.
//
// decode: unpack's count and scan, then one kernel from the stream straight to the decoder's reconstruction (DecodeBlock with a
// gaze rectangle per frame, the arithmetic of idct_core.hpp), and optionally the display pass of display_core.hpp (/ 255, bilinear
// resize, to u8).
//
// decode of two layers (svc_hip_decode_layers_frames; include/svc_hip.h states them): the count and scan of each stream, a per-frame
// merge of the two statuses, then the same reconstruction with its enhancement compiled in, which inside the gaze adds the enhancement
// frame's residuals.
//
// decode at reduced size (svc_hip_decode_levels_reduced_frames): the decode's count and scan, then a reconstruction from the first K x K
// coefficients of every N x N tile to a picture of 1 / reduce the size (stated at its kernel).
//
// decode of two layers at reduced size (svc_hip_decode_layers_reduced_frames): the two-layer decode's counts, scans and status merge, then
// the reduced reconstruction with the enhancement inside the gaze, a kernel of its own (stated there).
//
// window (svc_hip_window_levels_frames): a stored stream restricted to a window per output frame, without the pixels -- count, scan,
// frame offsets, then one pass that writes every output frame in aligned 16-byte vectors (stated at its kernels).
//
// split (svc_hip_split_levels_frames, svc_hip_split_levels_budget_frames): a stored fine stream -> a base stream at any steps plus its
// enhancement, in integers on the levels -- the window call's count and scan for the input, then count, scan, frame offsets and one
// write pass, each serving both layers (stated at its kernels).
//
// band and union (svc_hip_band_levels_frames, svc_hip_union_levels_frames): a stored stream restricted to a frequency band of every tile
// (and a window), and two streams with disjoint masks joined back -- the window call's count and scan for each input, then count, scan,
// frame offsets and a write pass of the split's shape (stated at their kernels).
//
// delta and undelta (svc_hip_delta_levels_frames, svc_hip_undelta_levels_frames): frames coded against their predecessors as differences
// of levels, and added back up -- the window call's count and scan for the input, then count, scan, frame offsets and write; the undelta's
// waves each carry one group through all frames of the call (stated at their kernels).
//
// decode of a delta stream (svc_hip_decode_delta_levels_frames): the undelta's input and status passes, then one kernel whose workgroups
// each carry a group of tiles in three planes through all frames -- the undelta's add into levels held in LDS and the decode's passes on
// them -- and, for the chain's last frame as an SVCQ frame, a scan and a write pass (stated at its kernels).
//
// temporal layers (svc_hip_delta_levels_temporal_frames, svc_hip_undelta_levels_temporal_frames, svc_hip_decode_delta_levels_temporal_frames):
// the three calls above with frame i coded against frame i - min(lowbit(i), period) -- the delta's body with another frame before, and the two
// kernels that rebuild with one held state per temporal layer; the statuses run down a tree.
//
// decode of a delta stream at reduced size (svc_hip_decode_delta_levels_reduced_frames): the same passes around a kernel of the reduced
// decode's shape that carries only the first K x K levels of every tile through the frames, in registers (stated at its kernel).
//
// decode of a temporal-layer delta stream at reduced size (svc_hip_decode_delta_levels_temporal_reduced_frames, include/svc_hip_temporal_decode.h):
// that kernel with one set of held levels per temporal layer below the odd frames, all in registers (stated at its kernel).
//
// pack of two layers (svc_hip_pack_layers_frames): the pack's count, scan and scatter on raw planes with two quantisations per coefficient,
// the frame offsets from frame_offsets_kernel with a job per layer (stated at its kernels).
//
// wire records <-> SVCQ (svc_hip_records_pack_levels_frames, svc_hip_levels_records_frames): the pack's and the unpack's count, scan and
// scatter with the reference's wire records in place of the planes, stream to stream (stated at their kernels).
#include "budget_core.hpp"
#include "display_core.hpp"
#include "idct_core.hpp"
#include "stream_format.hpp"
#include "svc_hip_temporal_decode.h"

#include <algorithm>
#include <cmath>
#include <type_traits>

namespace svc {
namespace {

constexpr uint32_t kGroupCoeffs = 2048;    // coefficients a workgroup stages
constexpr uint32_t kMaxJobs = 256;         // mask words per group

struct Geom {
  uint32_t w, h, bw, bh, mvbw, mvbh, mfw, mvb;
  uint32_t tiles_x, tiles_y, words, tpg, gx, groups;  // words per tile, tiles per group, groups per tile row, groups per frame
  uint32_t pitch_pad;                                // LDS row pitch = cols + ((pitch_pad - cols) & 63): conflict-free word reads
  uint64_t masks_off, levels_off;                    // byte offsets inside a frame
  bool vec;                                          // rows may be moved as float4
};

// the frame's layout and this file's work split
Geom make_geom(uint32_t w, uint32_t h, uint32_t bw, uint32_t bh, uint32_t mvbw, uint32_t mvbh) {
  const FrameLayout l = frame_layout(w, h, bw, bh, mvbw, mvbh);
  Geom g{};
  g.w = w; g.h = h; g.bw = bw; g.bh = bh; g.mvbw = mvbw; g.mvbh = mvbh;
  g.mfw = l.mfw; g.mvb = l.mvb;
  g.tiles_x = l.tiles_x; g.tiles_y = l.tiles_y; g.words = l.words;
  g.masks_off = l.masks_off; g.levels_off = l.levels_off;
  uint32_t tpg = std::max<uint32_t>(1, kGroupCoeffs / (bw * bh));
  tpg = std::max<uint32_t>(1, std::min<uint32_t>(tpg, kMaxJobs / g.words));  // (tiles above kMaxTileCoeffs are refused)
  if (tpg > 1) tpg &= ~1u;  // even: a group's first column (tile side even) is then a multiple of 4 floats
  g.tpg = std::min(tpg, g.tiles_x);
  g.gx = div_up(g.tiles_x, g.tpg);
  g.groups = 3 * g.tiles_y * g.gx;
  g.pitch_pad = bw & 63;
  g.vec = w % 4 == 0 && (g.tpg * bw) % 4 == 0;  // then every group's first column and every plane are 16-byte aligned
  return g;
}

uint32_t lds_bytes(const Geom& g) {
  const uint32_t cols = g.tpg * g.bw;
  return g.bh * (cols + ((g.pitch_pad - cols) & 63)) * 4;
}

// the workspace: per group a count (then its exclusive prefix) and an inexact count (unpack: mask bits set past the tile area);
// per frame its size, level count, inexact count and unpack status
struct Ws {
  uint32_t *cnt, *inexact, *frame_bytes, *frame_levels, *frame_inexact, *status;
};
Ws stream_ws(Carver& c, uint32_t n, uint32_t groups) {
  Ws s;
  s.cnt = c.take<uint32_t>((uint64_t)n * groups);
  s.inexact = c.take<uint32_t>((uint64_t)n * groups);
  s.frame_bytes = c.take<uint32_t>(n);
  s.frame_levels = c.take<uint32_t>(n);
  s.frame_inexact = c.take<uint32_t>(n);
  s.status = c.take<uint32_t>(n);
  return s;
}

// ---- device helpers ---------------------------------------------------------------------------------------------------------

struct Group {
  uint32_t plane, ty, t0, nt, x0, y0, cols, pitch;
};

__device__ __forceinline__ Group group_of(const Geom& g, uint32_t gi) {
  Group r;
  const uint32_t per_plane = g.tiles_y * g.gx;
  r.plane = gi / per_plane;
  const uint32_t rem = gi - r.plane * per_plane;
  r.ty = rem / g.gx;
  r.t0 = (rem - r.ty * g.gx) * g.tpg;
  r.nt = min(g.tpg, g.tiles_x - r.t0);
  r.x0 = r.t0 * g.bw;
  r.y0 = r.ty * g.bh;
  r.cols = r.nt * g.bw;
  r.pitch = r.cols + ((g.pitch_pad - r.cols) & 63u);
  return r;
}

// the group's first mask word in `plane` (the group's own, or the same tiles of another) of the frame at `frame`, as dwords; a group's
// words are contiguous: [plane][ty][t0 .. t0 + nt)[words]
template <typename B>  // uint8_t or const uint8_t
__device__ __forceinline__ auto group_masks(const Geom& g, B* frame, uint32_t plane, const Group& gr) {
  using W = std::conditional_t<std::is_const_v<B>, const uint32_t, uint32_t>;
  return mask_words(reinterpret_cast<W*>(frame + g.masks_off), (uint64_t)plane * g.tiles_y + gr.ty, g.tiles_x, gr.t0, g.words);
}

// the header of a frame of geometry g
__device__ __forceinline__ FrameHead head_of(const Geom& g, uint32_t fg, uint32_t bg, uint32_t levels, uint32_t inexact, uint32_t bytes) {
  return FrameHead{g.w, g.h, g.bw, g.bh, g.mvbw, g.mvbh, fg, bg, levels, inexact, bytes};
}

// the group's bh rows x cols floats of plane p -> LDS (row pitch gr.pitch)
__device__ __forceinline__ void stage_rows(const Geom& g, const Group& gr, const float* __restrict__ plane, float* lds) {
  if (g.vec && gr.cols % 4 == 0) {
    const uint32_t q = gr.cols / 4, n = q * g.bh;
    for (uint32_t i = threadIdx.x; i < n; i += kThreads) {
      const uint32_t r = i / q, c = (i - r * q) * 4;
      const float4 v = *reinterpret_cast<const float4*>(plane + (size_t)(gr.y0 + r) * g.w + gr.x0 + c);
      float* d = lds + r * gr.pitch + c;
      d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
  } else {
    const uint32_t n = gr.cols * g.bh;
    for (uint32_t i = threadIdx.x; i < n; i += kThreads) {
      const uint32_t r = i / gr.cols, c = i - r * gr.cols;
      lds[r * gr.pitch + c] = plane[(size_t)(gr.y0 + r) * g.w + gr.x0 + c];
    }
  }
}

// LDS -> the group's rows of plane p
__device__ __forceinline__ void store_rows(const Geom& g, const Group& gr, const float* lds, float* __restrict__ plane) {
  if (g.vec && gr.cols % 4 == 0) {
    const uint32_t q = gr.cols / 4, n = q * g.bh;
    for (uint32_t i = threadIdx.x; i < n; i += kThreads) {
      const uint32_t r = i / q, c = (i - r * q) * 4;
      const float* s = lds + r * gr.pitch + c;
      *reinterpret_cast<float4*>(plane + (size_t)(gr.y0 + r) * g.w + gr.x0 + c) = make_float4(s[0], s[1], s[2], s[3]);
    }
  } else {
    const uint32_t n = gr.cols * g.bh;
    for (uint32_t i = threadIdx.x; i < n; i += kThreads) {
      const uint32_t r = i / gr.cols, c = i - r * gr.cols;
      plane[(size_t)(gr.y0 + r) * g.w + gr.x0 + c] = lds[r * gr.pitch + c];
    }
  }
}

// LDS slot of coefficient k of the group's tile t
__device__ __forceinline__ uint32_t lds_index(const Geom& g, const Group& gr, uint32_t t, uint32_t k) {
  const uint32_t r = k / g.bw, c = k - r * g.bw;
  return r * gr.pitch + t * g.bw + c;
}

// region id of the MV block holding the tile origin (the rule of svc_hip_dct_quant_frames)
__device__ __forceinline__ uint32_t tile_type(const Geom& g, const uint32_t* __restrict__ types, const Group& gr, uint32_t t) {
  return types[(gr.y0 / g.mvbh) * g.mfw + (gr.x0 + t * g.bw) / g.mvbw];
}

// std::round(c / step) (the quantiser's level), clamped to int16
__device__ __forceinline__ int32_t level_of(float c, float step) {
  const float q = roundf(c / step);
  return (int32_t)fminf(fmaxf(q, -32768.f), 32767.f);
}

__device__ __forceinline__ uint32_t lane_rank(uint64_t mask) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// ---- pack --------------------------------------------------------------------------------------------------------------------

struct PackArgs {
  Geom g;
  const float* planes;   // [n][3][h][w]
  const uint32_t* types; // [n][mvb]
  uint8_t* out;
  uint64_t* offsets;     // [n + 1]
  Ws ws;
  uint32_t n, fg, bg;
  const uint32_t* steps; // [n][2] fg, bg per frame (the budgeted pack's choice), or null: fg / bg for every frame
};

// SCATTER = false: the group's non-zero count and inexact count.  SCATTER = true: masks and levels at their final place (plus,
// from group 0 of each frame, the header, the types, the zero pad and offsets[f + 1]).
template <bool SCATTER>
__global__ __launch_bounds__(256) void pack_kernel(PackArgs a) {
  extern __shared__ float lds[];
  __shared__ uint64_t job_mask[kMaxJobs];
  __shared__ uint32_t job_base[kMaxJobs];
  __shared__ uint32_t red[kThreads / 64];
  __shared__ uint64_t frame_off;
  const Geom& g = a.g;
  const uint32_t gi = blockIdx.x, f = blockIdx.y, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const Group gr = group_of(g, gi);
  const uint32_t* types = a.types + (size_t)f * g.mvb;
  const uint32_t fg = a.steps ? a.steps[2 * f] : a.fg, bg = a.steps ? a.steps[2 * f + 1] : a.bg;
  stage_rows(g, gr, a.planes + ((size_t)f * 3 + gr.plane) * g.h * g.w, lds);
  if (SCATTER) frame_offset_to_lds(a.ws.frame_bytes, f, &frame_off);
  __syncthreads();

  const uint32_t area = g.bw * g.bh, jobs = gr.nt * g.words;
  uint32_t nz_count = 0, inexact = 0;
  for (uint32_t j = wave; j < jobs; j += kThreads / 64) {
    const uint32_t t = j / g.words, k = (j - t * g.words) * 64 + lane;
    const float step = tile_type(g, types, gr, t) == 0 ? (float)bg : (float)fg;
    int32_t lv = 0;
    if (k < area) {
      const float c = lds[lds_index(g, gr, t, k)];
      lv = level_of(c, step);
      if (!SCATTER) inexact += c != (float)lv * step;
    }
    const uint64_t mask = __ballot(lv != 0);
    if (!SCATTER) nz_count += __popcll(mask);
    else if (lane == 0) job_mask[j] = mask;
  }
  if (!SCATTER) {
    for (uint32_t off = 32; off >= 1; off >>= 1) inexact += __shfl_xor(inexact, off, 64);
    if (lane == 0) red[wave] = inexact;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t s = 0;
      for (uint32_t i = 0; i < kThreads / 64; ++i) s += red[i];
      a.ws.inexact[(size_t)f * g.groups + gi] = s;
    }
    __syncthreads();
    if (lane == 0) red[wave] = nz_count;
    __syncthreads();
    if (threadIdx.x == 0) a.ws.cnt[(size_t)f * g.groups + gi] = red[0] + red[1] + red[2] + red[3];
    return;
  }

  // scatter: exclusive scan of the words' popcounts, in word order
  __syncthreads();
  uint32_t total;
  const uint32_t pc = threadIdx.x < jobs ? (uint32_t)__popcll(job_mask[threadIdx.x]) : 0u;
  const uint32_t ex = block_exclusive_scan(pc, red, &total);
  if (threadIdx.x < jobs) job_base[threadIdx.x] = ex;
  __syncthreads();
  uint8_t* frame = a.out + frame_off;
  int16_t* levels = reinterpret_cast<int16_t*>(frame + g.levels_off) + a.ws.cnt[(size_t)f * g.groups + gi];
  uint32_t* masks = group_masks(g, frame, gr.plane, gr);
  for (uint32_t j = threadIdx.x; j < jobs; j += kThreads) {  // two u32 stores: the masks are 4-byte aligned when mvb is odd
    masks[2 * j] = (uint32_t)job_mask[j];
    masks[2 * j + 1] = (uint32_t)(job_mask[j] >> 32);
  }
  for (uint32_t j = wave; j < jobs; j += kThreads / 64) {
    const uint64_t mask = job_mask[j];
    if (!((mask >> lane) & 1u)) continue;
    const uint32_t t = j / g.words, k = (j - t * g.words) * 64 + lane;
    const float step = tile_type(g, types, gr, t) == 0 ? (float)bg : (float)fg;
    levels[job_base[j] + lane_rank(mask)] = (int16_t)level_of(lds[lds_index(g, gr, t, k)], step);
  }
  if (gi != 0) return;
  // group 0: header, types, pad, offsets
  write_frame_edges(frame, head_of(g, fg, bg, a.ws.frame_levels[f], a.ws.frame_inexact[f], a.ws.frame_bytes[f]), types, g.mvb, g.levels_off,
                    kThreads, a.offsets, f, frame_off);
}

// one workgroup per frame: group counts -> exclusive prefixes (in place), the frame's level count, inexact count and size.
// UNPACK: also the frame's status (header vs geometry, level count vs masks), to ws and d_status.
template <bool UNPACK>
__global__ __launch_bounds__(256) void scan_kernel(Geom g, Ws ws, const uint8_t* in, uint64_t stream_bytes, const uint64_t* offsets,
                                                   uint32_t* d_status) {
  __shared__ uint32_t red[kThreads / 64];
  const uint32_t f = blockIdx.x;
  uint32_t* cnt = ws.cnt + (size_t)f * g.groups;
  uint32_t inexact = 0, t;  // summed on the scan's way: its loads go out with the counts'
  const uint32_t carry = scan_counts(g.groups, 0, red, [&](uint32_t i) { inexact += ws.inexact[(size_t)f * g.groups + i]; return cnt[i]; },
                                     [&](uint32_t i, uint32_t v) { cnt[i] = v; });
  (void)block_exclusive_scan(inexact, red, &t);  // pack: inexact coefficients; unpack: mask bits past the tile area
  if (!UNPACK) {
    if (threadIdx.x == 0) {
      ws.frame_levels[f] = carry;
      ws.frame_inexact[f] = t;
      ws.frame_bytes[f] = (uint32_t)up16(g.levels_off + 2ull * carry);
    }
    return;
  }
  if (threadIdx.x == 0) {
    uint64_t off = 0;
    const uint32_t* hdr = nullptr;
    uint32_t st = check_svcq<false>(g, in, stream_bytes, offsets, f, &off, &hdr);
    if (st == kStOk && t != 0) st = kStStrayBits;
    if (st == kStOk && hdr[kHLevels] != carry) st = kStLevels;
    ws.status[f] = st;
    d_status[f] = st;
  }
}

// ---- budgeted pack: per frame the finest ladder entry whose frame fits its byte budget ------------------------------------------

// (the ladder as the kernels take it, its thresholds, its checks and the choice: budget_core.hpp, shared with dct_pack.hip)

// workspace of the budgeted pack: the pack's own, then per (frame, entry, group) the non-zero levels, per (frame, entry) the frame's
// size, per frame its steps
struct BudgetWs {
  Ws pack;
  uint32_t *nz, *steps;
  uint64_t* bytes;
};
BudgetWs budget_ws(Carver& c, uint32_t n, uint32_t groups, uint32_t len) {
  BudgetWs s;
  s.pack = stream_ws(c, n, groups);
  s.nz = c.take<uint32_t>((uint64_t)n * len * groups);
  s.bytes = c.take<uint64_t>((uint64_t)n * len);
  s.steps = c.take<uint32_t>(2ull * n);
  return s;
}

// One group as pack_kernel splits it.  Per 64-coefficient word (the tile, hence the step class, is the same in every lane):
// entry k keeps a coefficient when |c| >= tau[k]; tau is non-decreasing along the ladder, so the words' ballots for k = 0, 1, ...
// shrink and the loop stops at the first empty one -- a background word at a coarse step costs one ballot.  Lane k holds tau[k] of
// both classes in registers and the loop reads the one it needs with readlane (no memory access in the loop); lane k of each wave
// also sums entry k's popcounts, the four waves add up through LDS and thread k stores nz[f][k][group].
__global__ __launch_bounds__(256) void budget_count_kernel(Geom g, const float* __restrict__ planes, const uint32_t* __restrict__ types_all,
                                                           Ladder lad, uint32_t* __restrict__ nz) {
  extern __shared__ float lds[];
  __shared__ uint32_t part[kThreads / 64][kMaxLadder];
  const uint32_t gi = blockIdx.x, f = blockIdx.y, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const Group gr = group_of(g, gi);
  const uint32_t* types = types_all + (size_t)f * g.mvb;
  const float tau_bg = lane < lad.len ? lad.tau[0][lane] : INFINITY, tau_fg = lane < lad.len ? lad.tau[1][lane] : INFINITY;
  stage_rows(g, gr, planes + ((size_t)f * 3 + gr.plane) * g.h * g.w, lds);
  __syncthreads();
  const uint32_t area = g.bw * g.bh, jobs = gr.nt * g.words;
  uint32_t acc = 0;  // lane k: this wave's non-zero levels at entry k
  for (uint32_t j = wave; j < jobs; j += kThreads / 64) {
    const uint32_t t = j / g.words, k = (j - t * g.words) * 64 + lane;
    const int tau = __float_as_int(tile_type(g, types, gr, t) == 0 ? tau_bg : tau_fg);
    // a NaN quantises to -32768 (fmaxf drops it): kept at every entry, as the pack keeps it
    const float c = k < area ? lds[lds_index(g, gr, t, k)] : 0.f;
    const float m = c != c ? INFINITY : fabsf(c);
    for (uint32_t e = 0; e < lad.len; ++e) {
      const uint64_t mask = __ballot(m >= __int_as_float(__builtin_amdgcn_readlane(tau, e)));
      if (mask == 0) break;
      acc += lane == e ? (uint32_t)__popcll(mask) : 0u;
    }
  }
  part[wave][lane] = acc;
  __syncthreads();
  if (threadIdx.x < lad.len)
    nz[((size_t)f * lad.len + threadIdx.x) * g.groups + gi] =
        part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
}

// One workgroup per (entry, frame): nz_k of the frame = the sum over its groups, as bytes_k = up16(levels_off + 2 nz_k).
__global__ __launch_bounds__(256) void budget_sum_kernel(Geom g, uint32_t len, const uint32_t* __restrict__ nz, uint64_t* __restrict__ bytes) {
  __shared__ uint64_t red[kThreads / 64];
  const uint32_t k = blockIdx.x, f = blockIdx.y, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t* p = nz + ((size_t)f * len + k) * g.groups;
  uint64_t s = 0;
  for (uint32_t i = threadIdx.x; i < g.groups; i += kThreads) s += p[i];
  for (uint32_t off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
  if (lane == 0) red[wave] = s;
  __syncthreads();
  if (threadIdx.x == 0) bytes[(size_t)f * len + k] = up16(g.levels_off + 2 * (red[0] + red[1] + red[2] + red[3]));
}

// One thread per frame: choice = the smallest k with bytes_k <= budget, else the last entry with bit 31 set; that entry's steps go to
// the pack.
__global__ __launch_bounds__(256) void budget_select_kernel(uint32_t n, Ladder lad, const uint64_t* __restrict__ bytes,
                                                            const uint32_t* __restrict__ budget, uint32_t* __restrict__ steps,
                                                            uint32_t* __restrict__ choice) {
  const uint32_t f = blockIdx.x * kThreads + threadIdx.x;
  if (f >= n) return;
  const uint64_t b = budget[f];
  const uint64_t* fb = bytes + (size_t)f * lad.len;
  const uint32_t ch = budget_choice(fb, lad.len, b), pick = ch & 0x7FFFFFFFu;
  choice[f] = ch;
  steps[2 * f] = lad.step[1][pick];
  steps[2 * f + 1] = lad.step[0][pick];
}

// ---- unpack ------------------------------------------------------------------------------------------------------------------

struct UnpackArgs {
  Geom g;
  const uint8_t* in;
  uint64_t stream_bytes;
  const uint64_t* offsets;
  float* planes;
  uint32_t* types;
  Ws ws;
};

// SCATTER = false: the group's popcount over its mask words (0 for a frame that fails its checks).  SCATTER = true: the group's
// rows of the planes (zeros where the mask is 0, everywhere for a bad frame) and, from group 0, the types.
template <bool SCATTER>
__global__ __launch_bounds__(256) void unpack_kernel(UnpackArgs a) {
  extern __shared__ float lds[];
  __shared__ uint32_t red[kThreads / 64];
  __shared__ uint32_t job_base[kMaxJobs];
  __shared__ uint64_t job_mask[kMaxJobs];
  const Geom& g = a.g;
  const uint32_t gi = blockIdx.x, f = blockIdx.y, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const Group gr = group_of(g, gi);
  uint64_t off = 0;
  const uint32_t* hdr = nullptr;
  const uint32_t st = SCATTER ? a.ws.status[f] : check_svcq<false>(g, a.in, a.stream_bytes, a.offsets, f, &off, &hdr);
  if (SCATTER) off = a.offsets[f], hdr = reinterpret_cast<const uint32_t*>(a.in + off);
  const uint8_t* frame = a.in + off;
  const uint32_t jobs = gr.nt * g.words;
  const uint32_t* masks = st != kStOk ? nullptr : group_masks(g, frame, gr.plane, gr);
  const uint32_t j = threadIdx.x;
  const uint64_t m = (masks && j < jobs) ? load_mask(masks + 2 * j) : 0ull;
  const uint32_t area = g.bw * g.bh;
  uint32_t total;
  const uint32_t ex = block_exclusive_scan((uint32_t)__popcll(m), red, &total);
  if (!SCATTER) {
    // the format keeps the bits past the tile area 0: a frame with such bits is refused (status kStStrayBits), not half read
    const uint32_t valid = j < jobs ? area - (j % g.words) * 64 : 64u;
    uint32_t stray;
    (void)block_exclusive_scan(valid < 64 ? (uint32_t)__popcll(m >> valid) : 0u, red, &stray);
    if (threadIdx.x == 0) {
      a.ws.cnt[(size_t)f * g.groups + gi] = total;
      a.ws.inexact[(size_t)f * g.groups + gi] = stray;
    }
    return;
  }
  if (j < jobs) { job_mask[j] = m; job_base[j] = ex; }
  __syncthreads();
  const int16_t* levels = reinterpret_cast<const int16_t*>(frame + g.levels_off) + a.ws.cnt[(size_t)f * g.groups + gi];
  const uint32_t* types = reinterpret_cast<const uint32_t*>(frame + kHeaderBytes);
  const float fg = st == kStOk ? (float)hdr[kHFgStep] : 0.f, bg = st == kStOk ? (float)hdr[kHBgStep] : 0.f;
  for (uint32_t jj = wave; jj < jobs; jj += kThreads / 64) {
    const uint64_t mask = job_mask[jj];
    const uint32_t t = jj / g.words, k = (jj - t * g.words) * 64 + lane;
    if (k >= area) continue;
    float v = 0.f;
    if ((mask >> lane) & 1u) {
      const float step = tile_type(g, types, gr, t) == 0 ? bg : fg;
      v = (float)levels[job_base[jj] + lane_rank(mask)] * step;
    }
    lds[lds_index(g, gr, t, k)] = v;
  }
  __syncthreads();
  store_rows(g, gr, lds, a.planes + ((size_t)f * 3 + gr.plane) * g.h * g.w);
  if (gi == 0) {
    uint32_t* tdst = a.types + (size_t)f * g.mvb;
    for (uint32_t i = threadIdx.x; i < g.mvb; i += kThreads) tdst[i] = st == kStOk ? types[i] : 0u;
  }
}

// ---- decode: one stream, or a base stream and its enhancement -------------------------------------------------------------------

struct DecodeArgs {
  Geom g;
  const uint8_t* in;
  const uint64_t* offsets;
  const uint32_t* gaze;  // [n][4] x, y, w, h in padded coordinates, or null
  float* rec;            // [n][h][w][3]
  Ws ws;
  float fg, bg;          // the decoder's steps
};

struct DecodeLayersArgs {
  DecodeArgs base;              // in / offsets / ws: the base stream's; base.gaze is not null
  const uint8_t* enh;
  const uint64_t* enh_offsets;
  Ws enh_ws;
};

// One thread per frame, after both scans: the frame's status -- the base frame's code, else kStEnhancement | the enhancement frame's,
// else kStEnhancement | kStLayer for an enhancement frame that is not one of this base frame (two steps in its header, or a base step
// that is no multiple of its step) -- to d_status and to the base workspace, where the reconstruction reads it.
__global__ __launch_bounds__(256) void layers_status_kernel(DecodeLayersArgs a, uint32_t n, uint32_t* d_status) {
  const uint32_t f = blockIdx.x * kThreads + threadIdx.x;
  if (f >= n) return;
  uint32_t st = a.base.ws.status[f];
  if (st == kStOk && a.enh_ws.status[f] != kStOk) st = kStEnhancement | a.enh_ws.status[f];
  if (st == kStOk) {  // both passed their checks: their headers are inside their streams, and no step is 0
    const uint32_t* hb = reinterpret_cast<const uint32_t*>(a.base.in + a.base.offsets[f]);
    const uint32_t* he = reinterpret_cast<const uint32_t*>(a.enh + a.enh_offsets[f]);
    const uint32_t e = he[kHFgStep];
    if (he[kHBgStep] != e || hb[kHFgStep] % e != 0 || hb[kHBgStep] % e != 0) st = kStEnhancement | kStLayer;
  }
  a.base.ws.status[f] = st;
  d_status[f] = st;
}

__device__ __forceinline__ const DecodeArgs& base_of(const DecodeArgs& a) { return a; }
__device__ __forceinline__ const DecodeArgs& base_of(const DecodeLayersArgs& a) { return a.base; }

// The reconstruction of both decodes; decode_levels_kernel and decode_layers_kernel are its two forms.  One workgroup per (tile row,
// group in the row) of a frame: the same tiles in all three planes.  Thread (t, j) owns row j of the group's tile t: it gathers that
// coefficient row by rank (the group's level prefix + the popcounts of the earlier mask words + the set bits below it in its own word)
// and dequantises it with the encoder's step; the row and column passes are idct_core.hpp's, with the decoder's step; after the third
// plane the thread stores its column's interleaved B,G,R pixels.  d_rec has the bits of unpack + svc_hip_decode_frames.
//
// ENH, the enhancement (the status read is then the merged one: 0 = both frames may be read): a workgroup whose group holds a gazed
// tile also loads the enhancement frame's mask words of its jobs and scans them, into the caller's enh_mask / enh_base; a thread of a
// gazed tile gathers the residual d by rank beside the base level Lb and decodes (Lb * ratio + d) at the enhancement's step, ratio =
// the tile's base step / that step.  Lb * ratio * enh_step == Lb * base step, so a gazed tile without residuals has the bits of the
// form without ENH; every other tile takes that form's path.  Without ENH none of this is compiled, and the two arrays are null.
//
// (args by value: by reference the compiler spends more instructions on both forms, profiles/decode_body_refactor.txt)
template <int N, bool ENH>
__device__ __forceinline__ void decode_body(const std::conditional_t<ENH, DecodeLayersArgs, DecodeArgs> args, uint64_t* enh_mask,
                                            uint32_t* enh_base) {
  constexpr uint32_t kRows = kGroupCoeffs / N;  // coefficient rows of a group: tpg * N <= 2048 / N
  __shared__ uint64_t job_mask[kMaxJobs];
  __shared__ uint32_t job_base[kMaxJobs];
  __shared__ uint32_t red[kThreads / 64];
  __shared__ double rows[kRows * (N + 1)];  // pitch N + 1: the column reads of a wave spread over the banks
  const DecodeArgs& a = base_of(args);
  const Geom& g = a.g;
  const uint32_t gi0 = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
  const Group gr = group_of(g, gi0);  // plane 0's group; planes 1 and 2 hold the same tiles
  const uint32_t st = a.ws.status[f];
  const uint8_t* frame = a.in + a.offsets[f];  // dereferenced only for a frame that passed its checks
  const uint8_t* eframe = nullptr;
  if constexpr (ENH) eframe = args.enh + (st == kStOk ? args.enh_offsets[f] : 0);
  const uint32_t* hdr = reinterpret_cast<const uint32_t*>(frame);
  const uint32_t t = tid / N, j = tid - t * N;
  const bool active = t < gr.nt;
  float enc = 0.f, dec = 1.f, enh_step = 0.f;
  bool enhanced = false;  // a gazed tile of the form with ENH
  uint32_t ratio = 0;
  if (st == kStOk && active) {
    const uint32_t type = tile_type(g, reinterpret_cast<const uint32_t*>(frame + kHeaderBytes), gr, t);
    const bool in_gaze = gazed(a.gaze, f, gr.x0 + t * N, gr.y0);  // ahead of the header's steps: in this order the code is the measured one
    const uint32_t enc_step = type == 0 ? hdr[kHBgStep] : hdr[kHFgStep];
    enc = (float)enc_step;
    dec = in_gaze ? 1.f : (type == 0 ? a.bg : a.fg);
    if (ENH && in_gaze) {
      const uint32_t e = reinterpret_cast<const uint32_t*>(eframe)[kHFgStep];
      ratio = enc_step / e;
      enh_step = (float)e;
      enhanced = true;
    }
  }
  bool any_enhanced = false;  // the same in every thread: the barriers below depend on it
  if constexpr (ENH) any_enhanced = __syncthreads_or(enhanced) != 0;
  const uint32_t jobs = gr.nt * g.words, per_plane = g.tiles_y * g.gx;
  float out[3][N];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    // (the index, for both frames: with two calls of group_masks the layered form compiles to other code, profiles/stream_blocks_refactor.txt)
    const size_t word0 = 2 * ((((size_t)c * g.tiles_y + gr.ty) * g.tiles_x + gr.t0) * g.words);
    const uint32_t* masks = st != kStOk ? nullptr : reinterpret_cast<const uint32_t*>(frame + g.masks_off) + word0;
    const uint64_t m = (masks && tid < jobs) ? load_mask(masks + 2 * tid) : 0ull;
    uint32_t total;
    const uint32_t ex = block_exclusive_scan((uint32_t)__popcll(m), red, &total);
    if (tid < jobs) { job_mask[tid] = m; job_base[tid] = ex; }
    if (any_enhanced) {  // (then st == kStOk)
      const uint64_t me = tid < jobs ? load_mask(reinterpret_cast<const uint32_t*>(eframe + g.masks_off) + word0 + 2 * tid) : 0ull;
      const uint32_t exe = block_exclusive_scan((uint32_t)__popcll(me), red, &total);
      if (tid < jobs) { enh_mask[tid] = me; enh_base[tid] = exe; }
    }
    __syncthreads();
    if (active) {
      const size_t gi = (size_t)f * g.groups + c * per_plane + gi0;
      const int16_t* levels = reinterpret_cast<const int16_t*>(frame + g.levels_off) + (st == kStOk ? a.ws.cnt[gi] : 0u);
      const int16_t* resid = nullptr;
      if constexpr (ENH) resid = reinterpret_cast<const int16_t*>(eframe + g.levels_off) + (enhanced ? args.enh_ws.cnt[gi] : 0u);
      float v[N];
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const uint32_t k = j * N + i, w = t * g.words + (k >> 6), b = k & 63u;
        const uint64_t mask = job_mask[w], below = (1ull << b) - 1;  // mask: 0 for a frame that failed, no level is read
        v[i] = 0.f;
        if (enhanced) {
          const uint64_t emask = enh_mask[w];
          // unsigned: a stream that breaks the format's bound on a level wraps instead of overflowing
          uint32_t lv = 0;
          if ((mask >> b) & 1u) lv = (uint32_t)(int32_t)levels[job_base[w] + (uint32_t)__popcll(mask & below)] * ratio;
          if ((emask >> b) & 1u) lv += (uint32_t)(int32_t)resid[enh_base[w] + (uint32_t)__popcll(emask & below)];
          v[i] = (float)(int32_t)lv * enh_step;
        } else if ((mask >> b) & 1u) {
          v[i] = (float)levels[job_base[w] + (uint32_t)__popcll(mask & below)] * enc;
        }
      }
      invert_row<N>(v, dec, rows, t, j);
    }
    __syncthreads();
    if (active) invert_column<N>(rows, t, j, out[c]);
    __syncthreads();  // the next plane reuses rows and the job arrays
  }
  if (!active) return;
  // a wave stores 64 adjacent pixels per row
  store_bgr_column<N>(a.rec + (((size_t)f * g.h + gr.y0) * g.w + gr.x0 + t * N + j) * 3, g.w, out);
}

template <int N>
__global__ __launch_bounds__(256) void decode_levels_kernel(DecodeArgs a) {
  decode_body<N, false>(a, nullptr, nullptr);
}

template <int N>
__global__ __launch_bounds__(256) void decode_layers_kernel(DecodeLayersArgs a) {
  __shared__ uint64_t enh_mask[kMaxJobs];
  __shared__ uint32_t enh_base[kMaxJobs];
  decode_body<N, true>(a, enh_mask, enh_base);
}

// ---- decode at reduced size: the first K x K coefficients of every N x N tile ------------------------------------------------------
//
// svc_hip_decode_levels_reduced_frames (include/svc_hip.h states it).  The grid, the rank of a level and the steps are decode_body's;
// the workgroup is only as large as its transform: thread (t, j < K) for the group's tiles, K * tiles threads, at least a wave (N = 8:
// 128, 64, 64; N = 16: 64).  A group has at most 64 mask words, so wave 0 scans each plane's words in registers, and every plane has
// job arrays and an f64 slab of its own: two barriers in all (words -> gather and row passes -> column passes) where decode_body takes
// five per plane.  The thread gathers the K levels of coefficient row j of tile t in each plane, the passes are idct_core.hpp's reduced
// ones on a slab of pitch K + 1, and the thread stores its column of K pixels of the (W K / N) x (H K / N) picture: tile (tx, ty) is the
// K x K pixels at (tx K, ty K).  Only K * K of a tile's levels are read; no f32 plane and no full-size picture is written.
constexpr uint32_t reduced_threads(uint32_t n, uint32_t k) { return std::max<uint32_t>(64, k * (kGroupCoeffs / (n * n))); }

template <int N, int K>
__global__ __launch_bounds__(reduced_threads(N, K)) void decode_reduced_kernel(DecodeArgs a) {
  constexpr uint32_t kTiles = kGroupCoeffs / (N * N), kJobs = kTiles * ((N * N + 63) / 64);  // tiles and mask words of a group
  static_assert(kJobs <= 64, "one wave scans a group's mask words");
  __shared__ uint64_t job_mask[3][kJobs];
  __shared__ uint32_t job_base[3][kJobs];
  __shared__ double rows[3][kTiles * K * (K + 1)];
  const Geom& g = a.g;
  const uint32_t gi0 = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
  const Group gr = group_of(g, gi0);  // plane 0's group; planes 1 and 2 hold the same tiles
  const uint32_t st = a.ws.status[f];
  const uint8_t* frame = a.in + a.offsets[f];  // dereferenced only for a frame that passed its checks
  const uint32_t* hdr = reinterpret_cast<const uint32_t*>(frame);
  const uint32_t t = tid / K, j = tid - t * K;
  const bool active = t < gr.nt;  // (nt <= kTiles)
  const uint32_t jobs = gr.nt * g.words, per_plane = g.tiles_y * g.gx;
  if (tid < 64) {  // wave 0: mask: 0 for a frame that failed and past the group's words, no level is read through it
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const uint64_t m = (st == kStOk && tid < jobs) ? load_mask(group_masks(g, frame, c, gr) + 2 * tid) : 0ull;
      const uint32_t ex = wave_exclusive_scan((uint32_t)__popcll(m));
      if (tid < kJobs) { job_mask[c][tid] = m; job_base[c][tid] = ex; }
    }
  }
  float enc = 0.f, dec = 1.f;
  if (st == kStOk && active) {
    const uint32_t type = tile_type(g, reinterpret_cast<const uint32_t*>(frame + kHeaderBytes), gr, t);
    const bool in_gaze = gazed(a.gaze, f, gr.x0 + t * N, gr.y0);  // the full-size tile origin: one rule for both decoders
    enc = (float)(type == 0 ? hdr[kHBgStep] : hdr[kHFgStep]);
    dec = in_gaze ? 1.f : (type == 0 ? a.bg : a.fg);
  }
  __syncthreads();
  if (active) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const size_t gi = (size_t)f * g.groups + c * per_plane + gi0;
      const int16_t* levels = reinterpret_cast<const int16_t*>(frame + g.levels_off) + (st == kStOk ? a.ws.cnt[gi] : 0u);
      float v[K];
#pragma unroll
      for (int i = 0; i < K; ++i) {
        const uint32_t k = j * N + i, w = t * g.words + (k >> 6), b = k & 63u;
        const uint64_t mask = job_mask[c][w], below = (1ull << b) - 1;
        v[i] = 0.f;
        if ((mask >> b) & 1u) v[i] = (float)levels[job_base[c][w] + (uint32_t)__popcll(mask & below)] * enc;
      }
      invert_row_reduced<K>(v, dec, rows[c], t, j);
    }
  }
  __syncthreads();
  if (!active) return;
  float out[3][K];
#pragma unroll
  for (int c = 0; c < 3; ++c) invert_column_reduced<N, K>(rows[c], t, j, out[c]);
  const uint32_t rw = g.w / N * K;  // the reduced picture's width; adjacent lanes hold adjacent pixels
  store_bgr_column<K>(a.rec + (((size_t)f * (g.h / N * K) + gr.ty * K) * rw + (gr.t0 + t) * K + j) * 3, rw, out);
}

template <int N, int K>
void launch_decode_reduced(dim3 grid, hipStream_t s, const DecodeArgs& a) {
  hipLaunchKernelGGL((decode_reduced_kernel<N, K>), grid, dim3(reduced_threads(N, K)), 0, s, a);
}

// svc_hip_decode_layers_reduced_frames: decode_reduced_kernel with decode_body's enhancement, a kernel of its own so that the one-stream
// form keeps its code.  The status read is the merged one (0 = both frames may be read).  Whether the group holds a gazed tile is
// decided in wave 0 itself (lane l tests tile l, one ballot: the group has at most 32 tiles), which then also scans the enhancement
// frame's words of the three planes into job arrays of their own (3 x 64 x 12 B at most); no barrier depends on it.  A thread of a gazed
// tile gathers the residual d by rank beside the base level Lb, for its K coefficients only, and dequantises (Lb * ratio + d) at the
// enhancement's step; every other thread takes decode_reduced_kernel's path and has its bits.
template <int N, int K>
__global__ __launch_bounds__(reduced_threads(N, K)) void decode_layers_reduced_kernel(DecodeLayersArgs args) {
  constexpr uint32_t kTiles = kGroupCoeffs / (N * N), kJobs = kTiles * ((N * N + 63) / 64);  // tiles and mask words of a group
  static_assert(kJobs <= 64, "one wave scans a group's mask words");
  __shared__ uint64_t job_mask[3][kJobs], enh_mask[3][kJobs];
  __shared__ uint32_t job_base[3][kJobs], enh_base[3][kJobs];
  __shared__ double rows[3][kTiles * K * (K + 1)];
  const DecodeArgs& a = args.base;
  const Geom& g = a.g;
  const uint32_t gi0 = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
  const Group gr = group_of(g, gi0);  // plane 0's group; planes 1 and 2 hold the same tiles
  const uint32_t st = a.ws.status[f];
  const uint8_t* frame = a.in + a.offsets[f];  // both dereferenced only for a frame whose merged status is 0
  const uint8_t* eframe = args.enh + (st == kStOk ? args.enh_offsets[f] : 0);
  const uint32_t* hdr = reinterpret_cast<const uint32_t*>(frame);
  const uint32_t t = tid / K, j = tid - t * K;
  const bool active = t < gr.nt;  // (nt <= kTiles)
  const uint32_t jobs = gr.nt * g.words, per_plane = g.tiles_y * g.gx;
  if (tid < 64) {  // wave 0: mask: 0 for a frame that failed and past the group's words, no level is read through it
    const bool any_gazed = __ballot(st == kStOk && tid < gr.nt && gazed(a.gaze, f, gr.x0 + tid * N, gr.y0)) != 0;  // the same in every lane
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const uint64_t m = (st == kStOk && tid < jobs) ? load_mask(group_masks(g, frame, c, gr) + 2 * tid) : 0ull;
      const uint32_t ex = wave_exclusive_scan((uint32_t)__popcll(m));
      if (tid < kJobs) { job_mask[c][tid] = m; job_base[c][tid] = ex; }
      if (any_gazed) {
        const uint64_t me = tid < jobs ? load_mask(group_masks(g, eframe, c, gr) + 2 * tid) : 0ull;
        const uint32_t exe = wave_exclusive_scan((uint32_t)__popcll(me));
        if (tid < kJobs) { enh_mask[c][tid] = me; enh_base[c][tid] = exe; }
      }
    }
  }
  float enc = 0.f, dec = 1.f, enh_step = 0.f;
  bool enhanced = false;  // a gazed tile: its group's enhancement words are in LDS
  uint32_t ratio = 0;
  if (st == kStOk && active) {
    const uint32_t type = tile_type(g, reinterpret_cast<const uint32_t*>(frame + kHeaderBytes), gr, t);
    const bool in_gaze = gazed(a.gaze, f, gr.x0 + t * N, gr.y0);  // the full-size tile origin: one rule for both decoders
    const uint32_t enc_step = type == 0 ? hdr[kHBgStep] : hdr[kHFgStep];
    enc = (float)enc_step;
    dec = in_gaze ? 1.f : (type == 0 ? a.bg : a.fg);
    if (in_gaze) {
      const uint32_t e = reinterpret_cast<const uint32_t*>(eframe)[kHFgStep];
      ratio = enc_step / e;
      enh_step = (float)e;
      enhanced = true;
    }
  }
  __syncthreads();
  if (active) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const size_t gi = (size_t)f * g.groups + c * per_plane + gi0;
      const int16_t* levels = reinterpret_cast<const int16_t*>(frame + g.levels_off) + (st == kStOk ? a.ws.cnt[gi] : 0u);
      const int16_t* resid = reinterpret_cast<const int16_t*>(eframe + g.levels_off) + (enhanced ? args.enh_ws.cnt[gi] : 0u);
      float v[K];
#pragma unroll
      for (int i = 0; i < K; ++i) {
        const uint32_t k = j * N + i, w = t * g.words + (k >> 6), b = k & 63u;
        const uint64_t mask = job_mask[c][w], below = (1ull << b) - 1;
        v[i] = 0.f;
        if (enhanced) {
          const uint64_t emask = enh_mask[c][w];
          // unsigned: a stream that breaks the format's bound on a level wraps instead of overflowing
          uint32_t lv = 0;
          if ((mask >> b) & 1u) lv = (uint32_t)(int32_t)levels[job_base[c][w] + (uint32_t)__popcll(mask & below)] * ratio;
          if ((emask >> b) & 1u) lv += (uint32_t)(int32_t)resid[enh_base[c][w] + (uint32_t)__popcll(emask & below)];
          v[i] = (float)(int32_t)lv * enh_step;
        } else if ((mask >> b) & 1u) {
          v[i] = (float)levels[job_base[c][w] + (uint32_t)__popcll(mask & below)] * enc;
        }
      }
      invert_row_reduced<K>(v, dec, rows[c], t, j);
    }
  }
  __syncthreads();
  if (!active) return;
  float out[3][K];
#pragma unroll
  for (int c = 0; c < 3; ++c) invert_column_reduced<N, K>(rows[c], t, j, out[c]);
  const uint32_t rw = g.w / N * K;  // the reduced picture's width; adjacent lanes hold adjacent pixels
  store_bgr_column<K>(a.rec + (((size_t)f * (g.h / N * K) + gr.ty * K) * rw + (gr.t0 + t) * K + j) * 3, rw, out);
}

template <int N, int K>
void launch_decode_reduced(dim3 grid, hipStream_t s, const DecodeLayersArgs& a) {
  hipLaunchKernelGGL((decode_layers_reduced_kernel<N, K>), grid, dim3(reduced_threads(N, K)), 0, s, a);
}

// the instantiation for a block of 8 or 16 and a reduce of 2, 4 or 8 (both checked by the caller), of either form
template <typename A>  // DecodeArgs or DecodeLayersArgs
void launch_decode_reduced(uint32_t block, uint32_t reduce, dim3 grid, hipStream_t s, const A& a) {
  if (block == 8) {
    if (reduce == 2) launch_decode_reduced<8, 4>(grid, s, a);
    else if (reduce == 4) launch_decode_reduced<8, 2>(grid, s, a);
    else launch_decode_reduced<8, 1>(grid, s, a);
  } else {
    if (reduce == 2) launch_decode_reduced<16, 8>(grid, s, a);
    else if (reduce == 4) launch_decode_reduced<16, 4>(grid, s, a);
    else launch_decode_reduced<16, 2>(grid, s, a);
  }
}

// ---- window: SVCQ frames restricted to the tiles of a window, stream to stream ---------------------------------------------------
//
// Output frame i = input frame s (d_src[i], or i) with the masks of the tiles outside window i cleared and their levels left out.  The
// levels of a group's kept tiles (the window is a rectangle: adjacent tiles) are one run in the input and one in the output, so per
// output frame
//   count    one wave per group: its levels, its kept levels, its levels before the first kept tile, its stray bits
//   scan     one workgroup per frame: D[group] = kept levels before the group, S[group] = the input index of its run's first level,
//            the frame's status and size
//   offsets  one workgroup: the frame offsets
//   write    one thread per aligned 16 bytes of the output frame, whatever they hold.  Header, types and masks lie at the same byte
//            offsets in both frames: an aligned 16-byte load, patched.  Eight levels inside one run are 4 (even input index) or 5 (odd:
//            funnel-shifted by 16 bits) aligned dwords of the input; vectors that hold a section's or a run's edge, or the padding, are put
//            together level by level.  Every output byte is stored once, by one thread: two calls write the same bytes.

struct WinWs {
  uint32_t *tot, *before, *stray;  // [n][groups]; `before` becomes S
  uint32_t* kept;                  // [n][groups + 1]: becomes D, entry `groups` = the frame's kept levels
  uint32_t *frame_bytes, *status;  // [n]
};
WinWs window_ws(Carver& c, uint32_t n, uint32_t groups) {
  WinWs s;
  s.tot = c.take<uint32_t>((uint64_t)n * groups);
  s.before = c.take<uint32_t>((uint64_t)n * groups);
  s.stray = c.take<uint32_t>((uint64_t)n * groups);
  s.kept = c.take<uint32_t>((uint64_t)n * (groups + 1));
  s.frame_bytes = c.take<uint32_t>(n);
  s.status = c.take<uint32_t>(n);
  return s;
}

struct WindowArgs {
  Geom g;
  const uint8_t* in;
  uint64_t stream_bytes;
  const uint64_t* offsets;  // [n_in + 1]
  uint32_t n_in;
  const uint32_t* src;      // [n_out] input frame of each output frame, or null: its own index
  const uint32_t* window;   // [n_out][4] x, y, w, h in padded coordinates, or null: every tile is kept
  uint8_t* out;
  uint64_t* out_offsets;    // [n_out + 1]
  uint32_t* d_status;       // [n_out]
  WinWs ws;
};

// output frame i's input frame, checked as the unpack checks it before its masks (a frame index past the stream: kStRange)
template <typename A>  // WindowArgs, or the split's SplitArgs
__device__ __forceinline__ uint32_t window_source(const A& a, uint32_t i, uint64_t* off, const uint32_t** hdr) {
  const uint32_t s = a.src ? a.src[i] : i;
  if (s >= a.n_in) return kStRange;
  return check_svcq<false>(a.g, a.in, a.stream_bytes, a.offsets, s, off, hdr);
}

__device__ __forceinline__ bool in_window(const uint32_t* window, uint32_t i, uint32_t ox, uint32_t oy) {
  return !window || gazed(window, i, ox, oy);
}

__global__ __launch_bounds__(256) void window_count_kernel(WindowArgs a) {
  const Geom& g = a.g;
  const uint32_t lane = threadIdx.x & 63u, gi = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6), i = blockIdx.y;
  if (gi >= g.groups) return;  // (the whole wave)
  const Group gr = group_of(g, gi);
  uint64_t off = 0;
  const uint32_t* hdr = nullptr;
  uint32_t tot = 0, kept = 0, before = 0, stray = 0;  // a frame that fails its checks counts nothing: its masks are not read
  if (window_source(a, i, &off, &hdr) == kStOk) {
    const uint32_t* masks = group_masks(g, a.in + off, gr.plane, gr);
    const uint32_t jobs = gr.nt * g.words, area = g.bw * g.bh;
    const uint32_t wx = a.window ? a.window[4ull * i] : 0u;
    for (uint32_t j = lane; j < jobs; j += 64) {
      const uint64_t m = load_mask(masks + 2 * j);
      const uint32_t t = j / g.words, pc = (uint32_t)__popcll(m), ox = gr.x0 + t * g.bw;
      const uint32_t valid = area - (j - t * g.words) * 64;
      tot += pc;
      if (in_window(a.window, i, ox, gr.y0)) kept += pc;
      else if (ox < wx) before += pc;  // left of the window: ahead of the run, if this group has one
      if (valid < 64) stray += (uint32_t)__popcll(m >> valid);
    }
  }
  tot = wave_sum(tot);
  kept = wave_sum(kept);
  before = wave_sum(before);
  stray = wave_sum(stray);
  if (lane == 0) {
    a.ws.tot[(size_t)i * g.groups + gi] = tot;
    a.ws.kept[(size_t)i * (g.groups + 1) + gi] = kept;
    a.ws.before[(size_t)i * g.groups + gi] = before;
    a.ws.stray[(size_t)i * g.groups + gi] = stray;
  }
}

__global__ __launch_bounds__(256) void window_scan_kernel(WindowArgs a) {
  __shared__ uint32_t red[kThreads / 64];
  const Geom& g = a.g;
  const uint32_t i = blockIdx.x;
  const uint32_t* tot = a.ws.tot + (size_t)i * g.groups;
  const uint32_t* strays = a.ws.stray + (size_t)i * g.groups;
  uint32_t* kept = a.ws.kept + (size_t)i * (g.groups + 1);
  uint32_t* run = a.ws.before + (size_t)i * g.groups;
  // S: the levels before the group, then those of its tiles left of the window
  uint32_t stray = 0, stray_bits;  // summed on the first scan's way
  const uint32_t carry_tot = scan_counts(g.groups, 0, red, [&](uint32_t k) { stray += strays[k]; return tot[k]; },
                                         [&](uint32_t k, uint32_t v) { run[k] += v; });
  const uint32_t carry_kept = scan_counts(kept, kept, g.groups, 0, red);
  (void)block_exclusive_scan(stray, red, &stray_bits);
  if (threadIdx.x == 0) {
    kept[g.groups] = carry_kept;
    uint64_t off = 0;
    const uint32_t* hdr = nullptr;
    uint32_t st = window_source(a, i, &off, &hdr);
    if (st == kStOk && stray_bits != 0) st = kStStrayBits;
    if (st == kStOk && hdr[kHLevels] != carry_tot) st = kStLevels;
    a.ws.status[i] = st;
    a.d_status[i] = st;
    a.ws.frame_bytes[i] = st == kStOk ? (uint32_t)up16(g.levels_off + 2ull * carry_kept) : kHeaderBytes;
  }
}

// The batch's frame offsets, for every call whose frames' sizes come from a kernel of their own (enqueue_frame_offsets: the window
// call and the entropy coder have one job, the split a job per layer).  One workgroup per job: a 64-bit inclusive scan of bytes[0 .. n).
__global__ __launch_bounds__(256) void frame_offsets_kernel(OffsetsJob job0, OffsetsJob job1, uint32_t n) {
  __shared__ uint64_t red[kThreads / 64];
  const OffsetsJob& job = blockIdx.x ? job1 : job0;
  const uint32_t* __restrict__ bytes = job.bytes;
  uint64_t* __restrict__ offsets = job.offsets;
  uint64_t* __restrict__ copy = job.copy;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint64_t carry = 0;
  for (uint32_t base = 0; base < n; base += kThreads) {
    const uint32_t k = base + threadIdx.x;
    uint64_t x = k < n ? bytes[k] : 0u;
    for (uint32_t off = 1; off < 64; off <<= 1) {
      const uint64_t y = __shfl_up(x, off, 64);
      if (lane >= off) x += y;
    }
    if (lane == 63) red[wave] = x;
    __syncthreads();
    uint64_t before = 0, sum = 0;
    for (uint32_t w = 0; w < kThreads / 64; ++w) {
      if (w < wave) before += red[w];
      sum += red[w];
    }
    __syncthreads();
    if (k < n) {
      offsets[k + 1] = carry + before + x;
      if (copy) copy[k + 1] = carry + before + x;
    }
    carry += sum;
  }
  if (threadIdx.x == 0) {
    offsets[0] = 0;
    if (copy) copy[0] = 0;
  }
}

// the run that holds kept level e: the last r in [lo, groups) with D[r] <= e (D[lo] <= e < D[groups])
__device__ __forceinline__ uint32_t run_of(const uint32_t* __restrict__ D, uint32_t lo, uint32_t groups, uint32_t e) {
  uint32_t hi = groups;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (D[mid] <= e) lo = mid;
    else hi = mid;
  }
  return lo;
}

// dword wb (< levels_off / 4) of output frame i, from the input frame's dword v at the same place
__device__ __forceinline__ uint32_t window_word(const WindowArgs& a, uint32_t i, const uint32_t* src, uint32_t wb, uint32_t v,
                                                uint32_t kept, uint32_t fbytes) {
  const Geom& g = a.g;
  // the header of a frame with the input's steps and inexact count (its geometry is g: the input frame passed check_svcq with it)
  if (wb < kHeaderWords) return header_word(head_of(g, src[kHFgStep], src[kHBgStep], kept, src[kHInexact], fbytes), wb);
  const uint32_t mw = (uint32_t)(g.masks_off / 4);
  if (wb < mw || !a.window) return v;
  const uint32_t tile = (wb - mw) / (2 * g.words), row = tile / g.tiles_x;  // row = plane * tiles_y + tile row
  return gazed(a.window, i, (tile - row * g.tiles_x) * g.bw, (row % g.tiles_y) * g.bh) ? v : 0u;
}

__global__ __launch_bounds__(256) void window_write_kernel(WindowArgs a) {
  const Geom& g = a.g;
  const uint32_t i = blockIdx.y, fbytes = a.ws.frame_bytes[i], nvec = fbytes / 16, stride = gridDim.x * kThreads;
  uint4* dst = reinterpret_cast<uint4*>(a.out + a.out_offsets[i]);
  uint32_t v = blockIdx.x * kThreads + threadIdx.x;
  if (a.ws.status[i] != kStOk) {  // 64 zero bytes; the input frame is not read
    for (; v < nvec; v += stride) dst[v] = make_uint4(0u, 0u, 0u, 0u);
    return;
  }
  const uint8_t* frame = a.in + a.offsets[a.src ? a.src[i] : i];
  const uint32_t* src32 = reinterpret_cast<const uint32_t*>(frame);
  const uint32_t src_bytes = src32[kHBytes];
  const uint32_t lw = (uint32_t)(g.levels_off / 4);  // the levels' first dword
  const uint32_t* lv32 = src32 + lw;
  const uint16_t* lv16 = reinterpret_cast<const uint16_t*>(lv32);
  const uint32_t* D = a.ws.kept + (size_t)i * (g.groups + 1);
  const uint32_t* S = a.ws.before + (size_t)i * g.groups;
  const uint32_t kept = D[g.groups];
  for (; v < nvec; v += stride) {
    const uint32_t w0 = 4 * v;
    uint32_t o[4];
    if (w0 + 4 <= lw) {  // header, types, masks
      const uint4 x = *reinterpret_cast<const uint4*>(frame + 16ull * v);
      o[0] = window_word(a, i, src32, w0, x.x, kept, fbytes);
      o[1] = window_word(a, i, src32, w0 + 1, x.y, kept, fbytes);
      o[2] = window_word(a, i, src32, w0 + 2, x.z, kept, fbytes);
      o[3] = window_word(a, i, src32, w0 + 3, x.w, kept, fbytes);
    } else {
      const uint32_t e0 = w0 >= lw ? 2 * (w0 - lw) : 0u;  // the vector's first level
      uint32_t r = 0, rend = 0;                           // a run and its end: D[r] <= e < rend for the levels e taken from it
      if (e0 < kept) {
        r = run_of(D, 0, g.groups, e0);
        rend = D[r + 1];
      }
      bool done = false;
      if (w0 >= lw && e0 + 8 <= rend) {  // eight levels of one run
        const uint32_t s = S[r] + (e0 - D[r]), q = s >> 1;
        if (!(s & 1u)) {
          o[0] = lv32[q]; o[1] = lv32[q + 1]; o[2] = lv32[q + 2]; o[3] = lv32[q + 3];
          done = true;
        } else if (g.levels_off + 4ull * (q + 5) <= src_bytes) {  // the fifth dword ends inside the input frame
          const uint32_t x0 = lv32[q], x1 = lv32[q + 1], x2 = lv32[q + 2], x3 = lv32[q + 3], x4 = lv32[q + 4];
          o[0] = (x0 >> 16) | (x1 << 16); o[1] = (x1 >> 16) | (x2 << 16); o[2] = (x2 >> 16) | (x3 << 16); o[3] = (x3 >> 16) | (x4 << 16);
          done = true;
        }
      }
      if (!done) {
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
          const uint32_t wb = w0 + k;
          if (wb < lw) {
            o[k] = window_word(a, i, src32, wb, src32[wb], kept, fbytes);
            continue;
          }
          uint32_t half[2];
#pragma unroll
          for (uint32_t b = 0; b < 2; ++b) {
            const uint32_t e = 2 * (wb - lw) + b;
            half[b] = 0;  // the padding
            if (e < kept) {
              if (e >= rend) {
                r = run_of(D, r, g.groups, e);
                rend = D[r + 1];
              }
              half[b] = lv16[S[r] + (e - D[r])];
            }
          }
          o[k] = half[0] | (half[1] << 16);
        }
      }
    }
    dst[v] = make_uint4(o[0], o[1], o[2], o[3]);
  }
}

// ---- split: a stored fine stream -> a base stream at any steps and its enhancement (svc_hip_split_levels_frames) ---------------------
//
// Input frame s holds the levels Lf at (e, e).  For a tile of class c, r = the class's base step / e, Lb = Lf / r rounded half away
// from zero and d = Lf - Lb * r inside output frame i's window: integers only, per coefficient, so a wave owns a group (a plane, a
// tile row, up to tpg tiles) and walks its mask words with one lane per coefficient.  The lane's Lf is found by rank (mbcnt) from the
// input index S of the group's first level plus the popcounts of the group's earlier words; the new masks are the ballots of Lb != 0
// and d != 0.  Per output frame
//   input    window_count_kernel and window_scan_kernel with no window: S per group and the input frame's status (unpack's code)
//   count    one wave per group: the non-zero levels of both layers
//   scan     one workgroup per frame: both layers' prefixes, level counts and sizes, the final status (kStLayer for a header step that
//            is not e)
//   offsets  frame_offsets_kernel, a workgroup per layer
//   write    one wave per group: both layers' mask words (a lane per word, 8 bytes each) and levels.  The levels are compacted in LDS
//            and stored as aligned dwords; a run that starts or ends at an odd level shares that dword with its neighbour's run and
//            stores its half of it as 16 bits.  The first workgroup of a frame also writes both headers, types and paddings.  Every
//            output byte is stored once: two calls write the same bytes.
// The budgeted form counts, between `input` and `count`, the coefficients every ladder entry keeps (2 |Lf| >= r: an integer compare)
// and picks each frame's pair; the passes after it take the steps per frame.

struct SplitWs {
  WinWs in;                // the input pass: in.before = S, in.status = unpack's code
  uint32_t *nzb, *nze;     // [n][groups] non-zero levels of the base / the enhancement, then their exclusive prefixes
  uint32_t *frame_bytes;   // [2][n] base, enhancement
  uint32_t *frame_levels;  // [2][n]
  uint32_t* steps;         // [n][2] fg, bg of each frame (the budgeted form)
  uint32_t* nz;            // [n][len][groups] (the budgeted form)
};
SplitWs split_ws(Carver& c, uint32_t n, uint32_t groups, uint32_t len) {  // len = 0: the fixed call, no nz
  SplitWs s;
  s.in = window_ws(c, n, groups);
  s.nzb = c.take<uint32_t>((uint64_t)n * groups);
  s.nze = c.take<uint32_t>((uint64_t)n * groups);
  s.frame_bytes = c.take<uint32_t>(2ull * n);
  s.frame_levels = c.take<uint32_t>(2ull * n);
  s.steps = c.take<uint32_t>(2ull * n);
  s.nz = c.take<uint32_t>((uint64_t)n * len * groups);
  return s;
}

struct SplitArgs {
  Geom g;
  const uint8_t* in;
  uint64_t stream_bytes;
  const uint64_t* offsets;  // [n_in + 1]
  uint32_t n_in;
  const uint32_t* src;      // [n_out] or null
  const uint32_t* window;   // [n_out][4] or null: every tile is enhanced
  uint32_t n_out, e, fg, bg;
  const uint32_t* steps;    // [n_out][2] fg, bg per frame (the budgeted form), or null: fg / bg for every frame
  uint8_t *base, *enh;      // enh null: the base only
  uint64_t *base_offsets, *enh_offsets;
  uint32_t* d_status;
  SplitWs ws;
};

// output frame i's input frame; only for a frame whose input pass reported kStOk (its source index and offsets are then in range)
__device__ __forceinline__ const uint8_t* split_frame_ptr(const SplitArgs& a, uint32_t i) {
  return a.in + a.offsets[a.src ? a.src[i] : i];
}

// the frame's status: unpack's code from the input pass, then kStLayer for a frame whose header does not say (e, e)
__device__ __forceinline__ uint32_t split_status(const SplitArgs& a, uint32_t i, const uint8_t** frame) {
  const uint32_t st = a.ws.in.status[i];
  if (st != kStOk) return st;
  *frame = split_frame_ptr(a, i);
  const uint32_t* hdr = reinterpret_cast<const uint32_t*>(*frame);
  return hdr[kHFgStep] == a.e && hdr[kHBgStep] == a.e ? kStOk : kStLayer;
}

// floor(num / den) for num < 2^18 and den < 2^16 with rcp = 1.f / den: the f32 product is within 1 of the quotient
__device__ __forceinline__ uint32_t div_by(uint32_t num, uint32_t den, float rcp) {
  uint32_t q = (uint32_t)((float)num * rcp);
  q -= q * den > num;
  q += (q + 1) * den <= num;
  return q;
}

// Lb = lf / r rounded half away from zero, d = lf - Lb * r; rcp = 1.f / (2 r)
__device__ __forceinline__ void split_level(int32_t lf, uint32_t r, float rcp, int32_t* lb, int32_t* d) {
  const uint32_t q = div_by(2u * (uint32_t)abs(lf) + r, 2u * r, rcp);
  *lb = lf < 0 ? -(int32_t)q : (int32_t)q;
  *d = lf - *lb * (int32_t)r;
}

// The wave's walk over its group's mask words, 64 of them at a time: lane l loads word l's mask and its tile's class and window
// bits, a wave scan of the popcounts gives every word the index of its first level, and the words are then walked with a lane per
// coefficient -- fn(j, fg, win, lf): j the word, fg / win whether its tile is foreground / inside output frame i's window, lf this
// lane's input level (0 where the mask bit is clear).  No load of the walk depends on an earlier one.  s = the input index of the
// group's first level.
template <typename F>
__device__ __forceinline__ void split_walk(const SplitArgs& a, uint32_t i, const Group& gr, const uint8_t* frame, uint32_t s, F&& fn) {
  const Geom& g = a.g;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t* masks = group_masks(g, frame, gr.plane, gr);
  const uint32_t* types = reinterpret_cast<const uint32_t*>(frame + kHeaderBytes);
  const int16_t* lv = reinterpret_cast<const int16_t*>(frame + g.levels_off) + s;
  const uint32_t jobs = gr.nt * g.words;
  for (uint32_t j0 = 0; j0 < jobs; j0 += 64) {
    const uint32_t j = j0 + lane, cnt = min(64u, jobs - j0);
    uint64_t m = 0;
    bool fg = false, win = false;
    if (j < jobs) {
      const uint32_t t = j / g.words;
      m = load_mask(masks + 2 * j);
      fg = tile_type(g, types, gr, t) != 0;
      win = a.enh && in_window(a.window, i, gr.x0 + t * g.bw, gr.y0);
    }
    const uint32_t pc = (uint32_t)__popcll(m), first = wave_exclusive_scan(pc);
    const uint64_t fg_words = __ballot(fg), win_words = __ballot(win);
#pragma unroll 4
    for (uint32_t k = 0; k < cnt; ++k) {
      const uint64_t mk = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)m, k) |
                          ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(m >> 32), k) << 32);
      const uint32_t at = (uint32_t)__builtin_amdgcn_readlane((int)first, k);
      const int32_t lf = (mk >> lane) & 1u ? (int32_t)lv[at + lane_rank(mk)] : 0;
      fn(j0 + k, (uint32_t)(fg_words >> k) & 1u, (win_words >> k) & 1u, lf);
    }
    lv += (uint32_t)__builtin_amdgcn_readlane((int)(first + pc), 63);
  }
}

// a frame's steps as ratios of e: class 0 = background
struct SplitRatios {
  uint32_t fg, bg, r[2];
  float rcp[2];
};
__device__ __forceinline__ SplitRatios split_ratios(const SplitArgs& a, uint32_t i) {
  SplitRatios s;
  s.fg = a.steps ? a.steps[2 * i] : a.fg;
  s.bg = a.steps ? a.steps[2 * i + 1] : a.bg;
  s.r[0] = s.bg / a.e;
  s.r[1] = s.fg / a.e;
  s.rcp[0] = 1.f / (float)(2 * s.r[0]);
  s.rcp[1] = 1.f / (float)(2 * s.r[1]);
  return s;
}

__global__ __launch_bounds__(256) void split_count_kernel(SplitArgs a) {
  const Geom& g = a.g;
  const uint32_t lane = threadIdx.x & 63u, gi = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6), i = blockIdx.y;
  if (gi >= g.groups) return;  // (the whole wave)
  const uint8_t* frame = nullptr;
  uint32_t nzb = 0, nze = 0;  // a frame that fails counts nothing
  if (split_status(a, i, &frame) == kStOk) {
    const Group gr = group_of(g, gi);
    const SplitRatios sr = split_ratios(a, i);
    split_walk(a, i, gr, frame, a.ws.in.before[(size_t)i * g.groups + gi], [&](uint32_t, uint32_t c, bool win, int32_t lf) {
      int32_t lb, d;
      split_level(lf, sr.r[c], sr.rcp[c], &lb, &d);
      nzb += (uint32_t)__popcll(__ballot(lb != 0));
      if (win) nze += (uint32_t)__popcll(__ballot(d != 0));
    });
  }
  if (lane == 0) {
    a.ws.nzb[(size_t)i * g.groups + gi] = nzb;
    a.ws.nze[(size_t)i * g.groups + gi] = nze;
  }
}

__global__ __launch_bounds__(256) void split_scan_kernel(SplitArgs a) {
  __shared__ uint32_t red[kThreads / 64];
  const Geom& g = a.g;
  const uint32_t i = blockIdx.x;
  uint32_t* nzb = a.ws.nzb + (size_t)i * g.groups;
  uint32_t* nze = a.ws.nze + (size_t)i * g.groups;
  // (scan_counts' loop in its own text, both layers in one trip: as two calls this kernel measured 2.3 % slower,
  // profiles/stream_blocks_refactor.txt)
  uint32_t carry_b = 0, carry_e = 0;
  for (uint32_t base = 0; base < g.groups; base += kThreads) {
    const uint32_t k = base + threadIdx.x;
    const bool live = k < g.groups;
    uint32_t sum_b, sum_e;
    const uint32_t ex_b = block_exclusive_scan(live ? nzb[k] : 0u, red, &sum_b);
    const uint32_t ex_e = block_exclusive_scan(live ? nze[k] : 0u, red, &sum_e);
    if (live) {
      nzb[k] = carry_b + ex_b;
      nze[k] = carry_e + ex_e;
    }
    carry_b += sum_b;
    carry_e += sum_e;
  }
  if (threadIdx.x == 0) {
    const uint8_t* frame = nullptr;
    const uint32_t st = split_status(a, i, &frame);
    a.d_status[i] = st;
    a.ws.in.status[i] = st;  // the write pass reads the final code
    a.ws.frame_levels[i] = carry_b;
    a.ws.frame_levels[a.n_out + i] = carry_e;
    a.ws.frame_bytes[i] = st == kStOk ? (uint32_t)up16(g.levels_off + 2ull * carry_b) : kHeaderBytes;
    a.ws.frame_bytes[a.n_out + i] = st == kStOk ? (uint32_t)up16(g.levels_off + 2ull * carry_e) : kHeaderBytes;
  }
}

// what the first workgroup of output frame i writes of one layer: the header (the geometry is the input frame's: it passed check_svcq
// with g; the inexact count is the input's too), the input's types, the padding.  The frame offsets are the offsets kernel's.
__device__ __forceinline__ void split_frame_edges(const Geom& g, const uint8_t* frame, uint8_t* out, uint32_t fg, uint32_t bg,
                                                  uint32_t level_count, uint32_t fbytes) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(frame);
  write_frame_edges(out, head_of(g, fg, bg, level_count, src[kHInexact], fbytes), src + kHeaderWords, g.mvb, g.levels_off, blockDim.x,
                    nullptr, 0, 0);
}

// The write pass's waves per workgroup and its dynamic LDS: per wave the group's coefficients as u16, twice (base, enhancement).  A
// group is tiles of at most kGroupCoeffs coefficients together, or one larger tile of at most kMaxTileCoeffs: 32 KB either way,
// which the assertion below keeps should either constant move.
constexpr uint32_t split_write_waves(uint32_t cap) { return cap > kGroupCoeffs ? 2 : kThreads / 64; }
constexpr uint32_t split_write_lds(uint32_t cap) { return split_write_waves(cap) * 2 * cap * (uint32_t)sizeof(uint16_t); }
static_assert(split_write_lds(kGroupCoeffs) <= 32768 && split_write_lds(kMaxTileCoeffs) <= 32768,
              "the split's write pass stages at most 32 KB per workgroup");

// blockDim.x / 64 waves, a group each; dynamic LDS: split_write_lds(cap), cap = the coefficients of a full group
__global__ __launch_bounds__(256) void split_write_kernel(SplitArgs a, uint32_t cap) {
  extern __shared__ uint16_t stage[];
  const Geom& g = a.g;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, gi = blockIdx.x * (blockDim.x >> 6) + wave, i = blockIdx.y;
  uint8_t* base = a.base + a.base_offsets[i];
  uint8_t* enh = a.enh ? a.enh + a.enh_offsets[i] : nullptr;
  if (a.ws.in.status[i] != kStOk) {  // (the final code) 64 zero bytes in each layer; the input frame is not read
    if (blockIdx.x == 0 && threadIdx.x < kHeaderWords) {
      reinterpret_cast<uint32_t*>(base)[threadIdx.x] = 0;
      if (enh) reinterpret_cast<uint32_t*>(enh)[threadIdx.x] = 0;
    }
    return;
  }
  const uint8_t* frame = split_frame_ptr(a, i);
  const SplitRatios sr = split_ratios(a, i);
  const bool live = gi < g.groups;  // no early return: the barrier below is the workgroup's
  uint16_t* buf_b = stage + (size_t)wave * 2 * cap;
  uint16_t* buf_e = buf_b + cap;
  uint32_t cnt_b = 0, cnt_e = 0;
  if (live) {
    const Group gr = group_of(g, gi);
    uint32_t* masks_b = group_masks(g, base, gr.plane, gr);
    uint32_t* masks_e = enh ? group_masks(g, enh, gr.plane, gr) : nullptr;
    const uint32_t jobs = gr.nt * g.words;
    uint64_t keep_b = 0, keep_e = 0;  // lane l: the new masks of word (j & ~63) + l, stored 64 words at a time
    split_walk(a, i, gr, frame, a.ws.in.before[(size_t)i * g.groups + gi], [&](uint32_t j, uint32_t c, bool win, int32_t lf) {
      int32_t lb, d;
      split_level(lf, sr.r[c], sr.rcp[c], &lb, &d);
      const uint64_t mb = __ballot(lb != 0);
      if (lb != 0) buf_b[cnt_b + lane_rank(mb)] = (uint16_t)lb;
      cnt_b += (uint32_t)__popcll(mb);
      uint64_t me = 0;
      if (win) {
        me = __ballot(d != 0);
        if (d != 0) buf_e[cnt_e + lane_rank(me)] = (uint16_t)d;
        cnt_e += (uint32_t)__popcll(me);
      }
      if (lane == (j & 63u)) keep_b = mb, keep_e = me;
      if ((j & 63u) == 63u || j + 1 == jobs) {
        const uint32_t k = (j & ~63u) + lane;
        if (k <= j) {
          store_mask(masks_b + 2 * k, keep_b);
          if (enh) store_mask(masks_e + 2 * k, keep_e);
        }
      }
    });
  }
  __syncthreads();
  if (live) {
    store_level_run(buf_b, cnt_b, reinterpret_cast<uint16_t*>(base + g.levels_off) + a.ws.nzb[(size_t)i * g.groups + gi]);
    if (enh) store_level_run(buf_e, cnt_e, reinterpret_cast<uint16_t*>(enh + g.levels_off) + a.ws.nze[(size_t)i * g.groups + gi]);
  }
  if (blockIdx.x != 0) return;
  split_frame_edges(g, frame, base, sr.fg, sr.bg, a.ws.frame_levels[i], a.ws.frame_bytes[i]);
  if (enh) split_frame_edges(g, frame, enh, a.e, a.e, a.ws.frame_levels[a.n_out + i], a.ws.frame_bytes[a.n_out + i]);
}

// The budgeted form's count, one wave per group: entry k keeps a coefficient when 2 |Lf| >= r_k of the tile's class (exactly Lb != 0
// there).  r is non-decreasing along the ladder, so a word's ballots shrink and the loop stops at the first empty one.  Lane k holds
// r_k of both classes and sums entry k's popcounts, as budget_count_kernel does with its thresholds.
__global__ __launch_bounds__(256) void split_budget_count_kernel(SplitArgs a, Ladder lad) {
  const Geom& g = a.g;
  const uint32_t lane = threadIdx.x & 63u, gi = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6), i = blockIdx.y;
  if (gi >= g.groups) return;  // (the whole wave)
  const uint8_t* frame = nullptr;
  uint32_t acc = 0;  // lane k: the group's non-zero base levels at entry k; a frame that fails counts nothing
  if (split_status(a, i, &frame) == kStOk) {
    const Group gr = group_of(g, gi);
    const uint32_t r_bg = lane < lad.len ? lad.step[0][lane] / a.e : 0xFFFFFFFFu, r_fg = lane < lad.len ? lad.step[1][lane] / a.e : 0xFFFFFFFFu;
    split_walk(a, i, gr, frame, a.ws.in.before[(size_t)i * g.groups + gi], [&](uint32_t, uint32_t c, bool, int32_t lf) {
      const uint32_t r = c ? r_fg : r_bg, m2 = 2u * (uint32_t)abs(lf);
      for (uint32_t k = 0; k < lad.len; ++k) {
        const uint64_t mask = __ballot(m2 >= (uint32_t)__builtin_amdgcn_readlane((int)r, k));
        if (mask == 0) break;
        acc += lane == k ? (uint32_t)__popcll(mask) : 0u;
      }
    });
  }
  if (lane < lad.len) a.ws.nz[((size_t)i * lad.len + lane) * g.groups + gi] = acc;
}

// One workgroup per frame: bytes_k = up16(levels offset + 2 * the sum of entry k's counts), then the choice (0 for a frame that fails)
// and that entry's steps for the passes after it.
__global__ __launch_bounds__(256) void split_select_kernel(SplitArgs a, Ladder lad, const uint32_t* __restrict__ budget,
                                                           uint32_t* __restrict__ choice) {
  __shared__ uint32_t red[kThreads / 64];
  __shared__ uint64_t bytes[kMaxLadder];
  const Geom& g = a.g;
  const uint32_t i = blockIdx.x;
  for (uint32_t k = 0; k < lad.len; ++k) {
    const uint32_t* p = a.ws.nz + ((size_t)i * lad.len + k) * g.groups;
    uint32_t s = 0, total;
    for (uint32_t j = threadIdx.x; j < g.groups; j += kThreads) s += p[j];
    (void)block_exclusive_scan(s, red, &total);
    if (threadIdx.x == 0) bytes[k] = up16(g.levels_off + 2ull * total);
  }
  if (threadIdx.x != 0) return;
  const uint8_t* frame = nullptr;
  const uint32_t ch = split_status(a, i, &frame) == kStOk ? budget_choice(bytes, lad.len, budget[i]) : 0u, pick = ch & 0x7FFFFFFFu;
  choice[i] = ch;
  a.ws.steps[2 * i] = lad.step[1][pick];
  a.ws.steps[2 * i + 1] = lad.step[0][pick];
}

// ---- pack of two layers from raw planes (svc_hip_pack_layers_frames) ----------------------------------------------------------------
//
// The pack's work split and passes with two quantisations per coefficient: Lb = level_of(c, the tile's base step), Lf = level_of(c, e)
// and d = Lf - Lb * ratio inside the frame's window, 0 outside it -- both from the f32 coefficient the group staged in LDS, so the base
// is the direct quantisation at (fg, bg) for any ratio (the split of a stored fine stream is not, at the ties of an even ratio).
//   count    pack_layers_kernel<false>: per group the non-zero levels of both layers and the base's inexact coefficients
//   scan     one workgroup per frame: both layers' prefixes, level counts and sizes, the base's inexact count
//   offsets  frame_offsets_kernel, a workgroup per layer
//   scatter  pack_layers_kernel<true>: both layers' masks and levels at their final place; group 0 writes both headers, types and
//            paddings.  Every output byte is stored once: two calls write the same bytes.

struct LayersWs {
  uint32_t *nzb, *nze, *inexact;  // [n][groups]; nzb / nze become exclusive prefixes
  uint32_t *frame_bytes;          // [2][n] base, enhancement
  uint32_t *frame_levels;         // [2][n]
  uint32_t *frame_inexact;        // [n] of the base
};
LayersWs layers_ws(Carver& c, uint32_t n, uint32_t groups) {
  LayersWs s;
  s.nzb = c.take<uint32_t>((uint64_t)n * groups);
  s.nze = c.take<uint32_t>((uint64_t)n * groups);
  s.inexact = c.take<uint32_t>((uint64_t)n * groups);
  s.frame_bytes = c.take<uint32_t>(2ull * n);
  s.frame_levels = c.take<uint32_t>(2ull * n);
  s.frame_inexact = c.take<uint32_t>(n);
  return s;
}

struct PackLayersArgs {
  Geom g;
  const float* planes;     // [n][3][h][w]
  const uint32_t* types;   // [n][mvb]
  const uint32_t* window;  // [n][4] or null: every tile is enhanced
  uint8_t *base, *enh;
  uint64_t *base_offsets, *enh_offsets;  // [n + 1], the offsets kernel's
  LayersWs ws;
  uint32_t n, fg, bg, e;
};

// SCATTER = false: the group's counts.  SCATTER = true: both layers' masks and levels and, from group 0 of each frame, their headers,
// types and zero pads.
template <bool SCATTER>
__global__ __launch_bounds__(256) void pack_layers_kernel(PackLayersArgs a) {
  extern __shared__ float lds[];
  __shared__ uint64_t mask_b[kMaxJobs], mask_e[kMaxJobs];
  __shared__ uint32_t at_b[kMaxJobs], at_e[kMaxJobs];
  __shared__ uint32_t red[kThreads / 64];
  const Geom& g = a.g;
  const uint32_t gi = blockIdx.x, f = blockIdx.y, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const Group gr = group_of(g, gi);
  const uint32_t* types = a.types + (size_t)f * g.mvb;
  const float e = (float)a.e;
  stage_rows(g, gr, a.planes + ((size_t)f * 3 + gr.plane) * g.h * g.w, lds);
  __syncthreads();

  const uint32_t area = g.bw * g.bh, jobs = gr.nt * g.words;
  // lane's two levels of word j: the base's Lb and the enhancement's d (0 outside the window and past the tile area)
  auto levels_of = [&](uint32_t j, int32_t* lb, int32_t* d, bool* inexact) {
    const uint32_t t = j / g.words, k = (j - t * g.words) * 64 + lane;
    const uint32_t sb = tile_type(g, types, gr, t) == 0 ? a.bg : a.fg;
    *lb = 0; *d = 0; *inexact = false;
    if (k >= area) return;
    const float c = lds[lds_index(g, gr, t, k)];
    *lb = level_of(c, (float)sb);
    *inexact = c != (float)*lb * (float)sb;
    if (in_window(a.window, f, gr.x0 + t * g.bw, gr.y0)) *d = level_of(c, e) - *lb * (int32_t)(sb / a.e);
  };
  uint32_t nzb = 0, nze = 0, inexact = 0;
  for (uint32_t j = wave; j < jobs; j += kThreads / 64) {
    int32_t lb, d;
    bool ix;
    levels_of(j, &lb, &d, &ix);
    const uint64_t mb = __ballot(lb != 0), me = __ballot(d != 0);
    if (!SCATTER) {
      nzb += (uint32_t)__popcll(mb);
      nze += (uint32_t)__popcll(me);
      inexact += ix;
    } else if (lane == 0) {
      mask_b[j] = mb;
      mask_e[j] = me;
    }
  }
  if (!SCATTER) {
    // (nzb and nze are the same in every lane of a wave: lane 0's value stands for the wave)
    uint32_t total;
    (void)block_exclusive_scan(lane == 0 ? nzb : 0u, red, &total);
    if (threadIdx.x == 0) a.ws.nzb[(size_t)f * g.groups + gi] = total;
    (void)block_exclusive_scan(lane == 0 ? nze : 0u, red, &total);
    if (threadIdx.x == 0) a.ws.nze[(size_t)f * g.groups + gi] = total;
    (void)block_exclusive_scan(inexact, red, &total);
    if (threadIdx.x == 0) a.ws.inexact[(size_t)f * g.groups + gi] = total;
    return;
  }

  // scatter: exclusive scans of the words' popcounts, in word order
  __syncthreads();
  uint32_t total;
  const uint32_t ex_b = block_exclusive_scan(threadIdx.x < jobs ? (uint32_t)__popcll(mask_b[threadIdx.x]) : 0u, red, &total);
  const uint32_t ex_e = block_exclusive_scan(threadIdx.x < jobs ? (uint32_t)__popcll(mask_e[threadIdx.x]) : 0u, red, &total);
  if (threadIdx.x < jobs) { at_b[threadIdx.x] = ex_b; at_e[threadIdx.x] = ex_e; }
  __syncthreads();
  uint8_t* base = a.base + a.base_offsets[f];
  uint8_t* enh = a.enh + a.enh_offsets[f];
  int16_t* lv_b = reinterpret_cast<int16_t*>(base + g.levels_off) + a.ws.nzb[(size_t)f * g.groups + gi];
  int16_t* lv_e = reinterpret_cast<int16_t*>(enh + g.levels_off) + a.ws.nze[(size_t)f * g.groups + gi];
  uint32_t* masks_b = group_masks(g, base, gr.plane, gr);
  uint32_t* masks_e = group_masks(g, enh, gr.plane, gr);
  for (uint32_t j = threadIdx.x; j < jobs; j += kThreads) {  // (kMaxJobs == kThreads: one trip)
    store_mask(masks_b + 2 * j, mask_b[j]);
    store_mask(masks_e + 2 * j, mask_e[j]);
  }
  for (uint32_t j = wave; j < jobs; j += kThreads / 64) {
    const uint64_t mb = mask_b[j], me = mask_e[j];
    if (!(((mb | me) >> lane) & 1u)) continue;
    int32_t lb, d;
    bool ix;
    levels_of(j, &lb, &d, &ix);
    if ((mb >> lane) & 1u) lv_b[at_b[j] + lane_rank(mb)] = (int16_t)lb;
    if ((me >> lane) & 1u) lv_e[at_e[j] + lane_rank(me)] = (int16_t)d;
  }
  if (gi != 0) return;
  write_frame_edges(base, head_of(g, a.fg, a.bg, a.ws.frame_levels[f], a.ws.frame_inexact[f], a.ws.frame_bytes[f]), types, g.mvb,
                    g.levels_off, kThreads, nullptr, 0, 0);
  write_frame_edges(enh, head_of(g, a.e, a.e, a.ws.frame_levels[a.n + f], 0, a.ws.frame_bytes[a.n + f]), types, g.mvb, g.levels_off,
                    kThreads, nullptr, 0, 0);
}

// one workgroup per frame: both layers' group counts -> exclusive prefixes (in place), their level counts and sizes, the base's inexact
// count
__global__ __launch_bounds__(256) void pack_layers_scan_kernel(Geom g, LayersWs ws, uint32_t n) {
  __shared__ uint32_t red[kThreads / 64];
  const uint32_t f = blockIdx.x;
  uint32_t* nzb = ws.nzb + (size_t)f * g.groups;
  uint32_t* nze = ws.nze + (size_t)f * g.groups;
  uint32_t inexact = 0, t;  // summed on the first scan's way
  const uint32_t carry_b = scan_counts(g.groups, 0, red, [&](uint32_t i) { inexact += ws.inexact[(size_t)f * g.groups + i]; return nzb[i]; },
                                       [&](uint32_t i, uint32_t v) { nzb[i] = v; });
  const uint32_t carry_e = scan_counts(nze, nze, g.groups, 0, red);
  (void)block_exclusive_scan(inexact, red, &t);
  if (threadIdx.x == 0) {
    ws.frame_levels[f] = carry_b;
    ws.frame_levels[n + f] = carry_e;
    ws.frame_inexact[f] = t;
    ws.frame_bytes[f] = (uint32_t)up16(g.levels_off + 2ull * carry_b);
    ws.frame_bytes[n + f] = (uint32_t)up16(g.levels_off + 2ull * carry_e);
  }
}

// ---- band: a stored stream restricted to a frequency band (and a window), stream to stream (svc_hip_band_levels_frames) ---------------
//
// Output frame i = input frame s with, of every tile inside window i, only the coefficients (row r, column c) of band i kept:
//   r < hi_h && c < hi_w && !(r < lo_h && c < lo_w)
// -- a plain predicate on u32, so a band is one 64-bit word per mask word of a tile (band_words) and a new mask word is the input's ANDed
// with it.  The selection is inside a tile, so the passes have the split's shape: a wave owns a group, a lane walks each coefficient and
// finds its level by rank.  Per output frame
//   input    window_count_kernel and window_scan_kernel with no window: S per group and the input frame's status (unpack's code)
//   count    one wave per group, a lane per mask word: the kept levels
//   scan     one workgroup per frame: the kept levels' prefixes, the frame's level count and size
//   offsets  frame_offsets_kernel
//   write    one wave per group: the new mask words (a lane per word) and the kept levels, compacted in LDS and stored by store_level_run.
//            The first workgroup of a frame also writes its header, types and padding.  Every output byte is stored once: two calls
//            write the same bytes.

struct BandWs {
  WinWs in;                // the input pass: in.before = S, in.status = unpack's code
  uint32_t* kept;          // [n][groups] kept levels, then their exclusive prefix
  uint32_t *frame_bytes, *frame_levels;  // [n]
};
BandWs band_ws(Carver& c, uint32_t n, uint32_t groups) {
  BandWs s;
  s.in = window_ws(c, n, groups);
  s.kept = c.take<uint32_t>((uint64_t)n * groups);
  s.frame_bytes = c.take<uint32_t>(n);
  s.frame_levels = c.take<uint32_t>(n);
  return s;
}

struct BandArgs {
  WindowArgs w;          // the window call's arguments; w.ws = the input pass's arrays
  const uint32_t* band;  // [n_out][4] lo_w, lo_h, hi_w, hi_h, or null: every coefficient
  uint32_t *kept, *frame_bytes, *frame_levels;
};

__device__ __forceinline__ uint64_t readlane64(uint64_t v, uint32_t k) {
  return (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, k) |
         ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), k) << 32);
}

// lane l (< g.words; the others 0): the bits of a tile's mask word l whose coefficients band i keeps
__device__ __forceinline__ uint64_t band_words(const Geom& g, const uint32_t* __restrict__ band, uint32_t i) {
  const uint32_t lane = threadIdx.x & 63u, area = g.bw * g.bh;
  const uint32_t lo_w = band ? band[4ull * i] : 0u, lo_h = band ? band[4ull * i + 1] : 0u;
  const uint32_t hi_w = band ? band[4ull * i + 2] : 0xFFFFFFFFu, hi_h = band ? band[4ull * i + 3] : 0xFFFFFFFFu;
  uint64_t mine = 0;
  for (uint32_t wi = 0; wi < g.words; ++wi) {
    const uint32_t k = wi * 64 + lane, r = k / g.bw, c = k - r * g.bw;
    const uint64_t word = __ballot(k < area && r < hi_h && c < hi_w && !(r < lo_h && c < lo_w));
    if (lane == wi) mine = word;
  }
  return mine;
}

// lane's view of mask word j of a group of output frame i: the band's bits of the word's place in its tile, 0 outside the window
__device__ __forceinline__ uint64_t band_of_word(const BandArgs& a, uint32_t i, const Group& gr, uint32_t j, uint64_t words) {
  const Geom& g = a.w.g;
  const uint32_t t = j / g.words, wi = j - t * g.words;
  const uint64_t b = __shfl(words, wi, 64);
  return in_window(a.w.window, i, gr.x0 + t * g.bw, gr.y0) ? b : 0ull;
}

__global__ __launch_bounds__(256) void band_count_kernel(BandArgs a) {
  const Geom& g = a.w.g;
  const uint32_t lane = threadIdx.x & 63u, gi = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6), i = blockIdx.y;
  if (gi >= g.groups) return;  // (the whole wave)
  uint32_t kept = 0;           // a frame that fails counts nothing: its masks are not read
  if (a.w.ws.status[i] == kStOk) {
    const Group gr = group_of(g, gi);
    const uint8_t* frame = a.w.in + a.w.offsets[a.w.src ? a.w.src[i] : i];
    const uint32_t* masks = group_masks(g, frame, gr.plane, gr);
    const uint64_t words = band_words(g, a.band, i);
    const uint32_t jobs = gr.nt * g.words;
    for (uint32_t j0 = 0; j0 < jobs; j0 += 64) {  // (the shuffle inside band_of_word is the whole wave's)
      const uint32_t j = min(j0 + lane, jobs - 1);
      const uint64_t b = band_of_word(a, i, gr, j, words);
      if (j0 + lane < jobs) kept += (uint32_t)__popcll(load_mask(masks + 2 * j) & b);
    }
  }
  kept = wave_sum(kept);
  if (lane == 0) a.kept[(size_t)i * g.groups + gi] = kept;
}

__global__ __launch_bounds__(256) void band_scan_kernel(BandArgs a) {
  __shared__ uint32_t red[kThreads / 64];
  const Geom& g = a.w.g;
  const uint32_t i = blockIdx.x;
  uint32_t* kept = a.kept + (size_t)i * g.groups;
  const uint32_t carry = scan_counts(kept, kept, g.groups, 0, red);
  if (threadIdx.x == 0) {
    a.frame_levels[i] = carry;
    a.frame_bytes[i] = a.w.ws.status[i] == kStOk ? (uint32_t)up16(g.levels_off + 2ull * carry) : kHeaderBytes;
  }
}

// The write passes of the band call and the union: kThreads / 64 waves, a group each, each wave's levels staged as u16 -- at most
// the coefficients of a full group
constexpr uint32_t select_write_lds(uint32_t cap) { return (kThreads / 64) * cap * (uint32_t)sizeof(uint16_t); }
static_assert(select_write_lds(kGroupCoeffs) <= 32768 && select_write_lds(kMaxTileCoeffs) <= 32768,
              "the band's and the union's write passes stage at most 32 KB per workgroup");

// dynamic LDS: select_write_lds(cap), cap = the coefficients of a full group
__global__ __launch_bounds__(256) void band_write_kernel(BandArgs a, uint32_t cap) {
  extern __shared__ uint16_t stage[];
  const Geom& g = a.w.g;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, gi = blockIdx.x * (kThreads / 64) + wave, i = blockIdx.y;
  uint8_t* out = a.w.out + a.w.out_offsets[i];
  if (a.w.ws.status[i] != kStOk) {  // 64 zero bytes; the input frame is not read
    if (blockIdx.x == 0 && threadIdx.x < kHeaderWords) reinterpret_cast<uint32_t*>(out)[threadIdx.x] = 0;
    return;
  }
  const uint8_t* frame = a.w.in + a.w.offsets[a.w.src ? a.w.src[i] : i];
  const bool live = gi < g.groups;  // no early return: the barrier below is the workgroup's
  uint16_t* buf = stage + (size_t)wave * cap;
  uint32_t cnt = 0;
  if (live) {
    const Group gr = group_of(g, gi);
    const uint32_t* masks = group_masks(g, frame, gr.plane, gr);
    uint32_t* masks_out = group_masks(g, out, gr.plane, gr);
    const uint16_t* lv = reinterpret_cast<const uint16_t*>(frame + g.levels_off) + a.w.ws.before[(size_t)i * g.groups + gi];
    const uint64_t words = band_words(g, a.band, i);
    const uint32_t jobs = gr.nt * g.words;
    for (uint32_t j0 = 0; j0 < jobs; j0 += 64) {
      const uint32_t j = min(j0 + lane, jobs - 1), n = min(64u, jobs - j0);
      const uint64_t b = band_of_word(a, i, gr, j, words);
      const uint64_t m = j0 + lane < jobs ? load_mask(masks + 2 * j) : 0ull, keep = m & b;
      if (j0 + lane < jobs) store_mask(masks_out + 2 * j, keep);
      const uint32_t pc = (uint32_t)__popcll(m), first = wave_exclusive_scan(pc);
      const uint32_t pk = (uint32_t)__popcll(keep), first_k = wave_exclusive_scan(pk);
      for (uint32_t k = 0; k < n; ++k) {
        const uint64_t kk = readlane64(keep, k);
        if (kk == 0) continue;  // (the whole wave)
        const uint64_t mk = readlane64(m, k);
        const uint32_t at = (uint32_t)__builtin_amdgcn_readlane((int)first, k), to = (uint32_t)__builtin_amdgcn_readlane((int)first_k, k);
        if ((kk >> lane) & 1u) buf[cnt + to + lane_rank(kk)] = lv[at + lane_rank(mk)];
      }
      lv += (uint32_t)__builtin_amdgcn_readlane((int)(first + pc), 63);
      cnt += (uint32_t)__builtin_amdgcn_readlane((int)(first_k + pk), 63);
    }
  }
  __syncthreads();
  if (live) store_level_run(buf, cnt, reinterpret_cast<uint16_t*>(out + g.levels_off) + a.kept[(size_t)i * g.groups + gi]);
  if (blockIdx.x != 0) return;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(frame);
  split_frame_edges(g, frame, out, src[kHFgStep], src[kHBgStep], a.frame_levels[i], a.frame_bytes[i]);
}

// ---- union: two streams of the same frames with disjoint masks -> one (svc_hip_union_levels_frames) -----------------------------------
//
// Output frame i has the masks of frame i of A ORed with those of frame i of B and the levels of both in coefficient order: a lane
// per coefficient picks its level by rank in A's or B's mask word and puts it at its rank in the union's.  Header words 0 .. 9 and 11 and the
// types are A's.  Per frame
//   input    window_count_kernel and window_scan_kernel with no window on each stream: S per group and the frame's unpack code
//   count    one wave per group, a lane per mask word: the union's levels, and whether a bit is set in both
//   scan     one workgroup per frame: the prefixes, the final status (A's code, 0x100 | B's, 0x100 | kStLayer for other steps or types,
//            kStOverlap), the frame's level count and size
//   offsets  frame_offsets_kernel
//   write    as the band's, with two inputs

struct UnionWs {
  WinWs a, b;                                     // the two input passes
  uint32_t *cnt, *overlap;                        // [n][groups] the union's levels (then their prefix); words with a bit in both
  uint32_t *frame_bytes, *frame_levels, *status;  // [n]
};
UnionWs union_ws(Carver& c, uint32_t n, uint32_t groups) {
  UnionWs s;
  s.a = window_ws(c, n, groups);
  s.b = window_ws(c, n, groups);
  s.cnt = c.take<uint32_t>((uint64_t)n * groups);
  s.overlap = c.take<uint32_t>((uint64_t)n * groups);
  s.frame_bytes = c.take<uint32_t>(n);
  s.frame_levels = c.take<uint32_t>(n);
  s.status = c.take<uint32_t>(n);
  return s;
}

struct UnionArgs {
  WindowArgs a, b;  // the two streams as the input pass takes them (no source indices, no window); a.out, a.out_offsets, a.d_status: the call's
  uint32_t *cnt, *overlap, *frame_bytes, *frame_levels, *status;
};

__global__ __launch_bounds__(256) void union_count_kernel(UnionArgs u) {
  const Geom& g = u.a.g;
  const uint32_t lane = threadIdx.x & 63u, gi = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6), i = blockIdx.y;
  if (gi >= g.groups) return;  // (the whole wave)
  uint32_t cnt = 0, both = 0;  // a pair with a frame that fails counts nothing: no masks are read
  if (u.a.ws.status[i] == kStOk && u.b.ws.status[i] == kStOk) {
    const Group gr = group_of(g, gi);
    const uint32_t* ma = group_masks(g, u.a.in + u.a.offsets[i], gr.plane, gr);
    const uint32_t* mb = group_masks(g, u.b.in + u.b.offsets[i], gr.plane, gr);
    const uint32_t jobs = gr.nt * g.words;
    for (uint32_t j = lane; j < jobs; j += 64) {
      const uint64_t x = load_mask(ma + 2 * j), y = load_mask(mb + 2 * j);
      cnt += (uint32_t)__popcll(x | y);
      both += (x & y) != 0;
    }
  }
  cnt = wave_sum(cnt);
  both = wave_sum(both);
  if (lane == 0) {
    u.cnt[(size_t)i * g.groups + gi] = cnt;
    u.overlap[(size_t)i * g.groups + gi] = both;
  }
}

__global__ __launch_bounds__(256) void union_scan_kernel(UnionArgs u) {
  __shared__ uint32_t red[kThreads / 64];
  const Geom& g = u.a.g;
  const uint32_t i = blockIdx.x;
  uint32_t* cnt = u.cnt + (size_t)i * g.groups;
  const uint32_t* overlap = u.overlap + (size_t)i * g.groups;
  uint32_t both = 0, words_both, other = 0, words_other;  // summed on the scan's way
  const uint32_t carry = scan_counts(g.groups, 0, red, [&](uint32_t k) { both += overlap[k]; return cnt[k]; },
                                     [&](uint32_t k, uint32_t v) { cnt[k] = v; });
  (void)block_exclusive_scan(both, red, &words_both);
  const uint32_t sa = u.a.ws.status[i], sb = u.b.ws.status[i];
  if (sa == kStOk && sb == kStOk) {  // (the whole workgroup) does B belong to A: the same steps and types?
    const uint32_t* ha = reinterpret_cast<const uint32_t*>(u.a.in + u.a.offsets[i]);
    const uint32_t* hb = reinterpret_cast<const uint32_t*>(u.b.in + u.b.offsets[i]);
    if (threadIdx.x == 0) other = ha[kHFgStep] != hb[kHFgStep] || ha[kHBgStep] != hb[kHBgStep];
    for (uint32_t k = threadIdx.x; k < g.mvb; k += kThreads) other += ha[kHeaderWords + k] != hb[kHeaderWords + k];
  }
  (void)block_exclusive_scan(other, red, &words_other);
  if (threadIdx.x == 0) {
    uint32_t st = sa;
    if (st == kStOk && sb != kStOk) st = kStEnhancement | sb;
    if (st == kStOk && words_other != 0) st = kStEnhancement | kStLayer;
    if (st == kStOk && words_both != 0) st = kStOverlap;
    u.status[i] = st;
    u.a.d_status[i] = st;
    u.frame_levels[i] = carry;
    u.frame_bytes[i] = st == kStOk ? (uint32_t)up16(g.levels_off + 2ull * carry) : kHeaderBytes;
  }
}

// dynamic LDS: select_write_lds(cap), cap = the coefficients of a full group
__global__ __launch_bounds__(256) void union_write_kernel(UnionArgs u, uint32_t cap) {
  extern __shared__ uint16_t stage[];
  const Geom& g = u.a.g;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, gi = blockIdx.x * (kThreads / 64) + wave, i = blockIdx.y;
  uint8_t* out = u.a.out + u.a.out_offsets[i];
  if (u.status[i] != kStOk) {  // 64 zero bytes; the input frames are not read
    if (blockIdx.x == 0 && threadIdx.x < kHeaderWords) reinterpret_cast<uint32_t*>(out)[threadIdx.x] = 0;
    return;
  }
  const uint8_t* fa = u.a.in + u.a.offsets[i];
  const uint8_t* fb = u.b.in + u.b.offsets[i];
  const bool live = gi < g.groups;  // no early return: the barrier below is the workgroup's
  uint16_t* buf = stage + (size_t)wave * cap;
  uint32_t cnt = 0;
  if (live) {
    const Group gr = group_of(g, gi);
    const uint32_t* masks_a = group_masks(g, fa, gr.plane, gr);
    const uint32_t* masks_b = group_masks(g, fb, gr.plane, gr);
    uint32_t* masks_out = group_masks(g, out, gr.plane, gr);
    const uint16_t* la = reinterpret_cast<const uint16_t*>(fa + g.levels_off) + u.a.ws.before[(size_t)i * g.groups + gi];
    const uint16_t* lb = reinterpret_cast<const uint16_t*>(fb + g.levels_off) + u.b.ws.before[(size_t)i * g.groups + gi];
    const uint32_t jobs = gr.nt * g.words;
    for (uint32_t j0 = 0; j0 < jobs; j0 += 64) {
      const uint32_t j = j0 + lane, n = min(64u, jobs - j0);
      uint64_t x = 0, y = 0;
      if (j < jobs) {
        x = load_mask(masks_a + 2 * j);
        y = load_mask(masks_b + 2 * j);
        store_mask(masks_out + 2 * j, x | y);
      }
      const uint32_t px = (uint32_t)__popcll(x), py = (uint32_t)__popcll(y);  // (disjoint: the union's popcount is their sum)
      const uint32_t first_x = wave_exclusive_scan(px), first_y = wave_exclusive_scan(py);
      for (uint32_t k = 0; k < n; ++k) {
        const uint64_t xk = readlane64(x, k), yk = readlane64(y, k);
        if ((xk | yk) == 0) continue;  // (the whole wave)
        const uint32_t ax = (uint32_t)__builtin_amdgcn_readlane((int)first_x, k), ay = (uint32_t)__builtin_amdgcn_readlane((int)first_y, k);
        uint16_t v = 0;
        if ((xk >> lane) & 1u) v = la[ax + lane_rank(xk)];
        else if ((yk >> lane) & 1u) v = lb[ay + lane_rank(yk)];
        if (((xk | yk) >> lane) & 1u) buf[cnt + ax + ay + lane_rank(xk | yk)] = v;
      }
      const uint32_t tx = (uint32_t)__builtin_amdgcn_readlane((int)(first_x + px), 63);
      const uint32_t ty = (uint32_t)__builtin_amdgcn_readlane((int)(first_y + py), 63);
      la += tx;
      lb += ty;
      cnt += tx + ty;
    }
  }
  __syncthreads();
  if (live) store_level_run(buf, cnt, reinterpret_cast<uint16_t*>(out + g.levels_off) + u.cnt[(size_t)i * g.groups + gi]);
  if (blockIdx.x != 0) return;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(fa);
  split_frame_edges(g, fa, out, src[kHFgStep], src[kHBgStep], u.frame_levels[i], u.frame_bytes[i]);
}

// ---- delta and undelta: frames coded against their predecessors in levels, and back (svc_hip_delta_levels_frames,
// svc_hip_undelta_levels_frames; include/svc_hip.h states them) ---------------------------------------------------------------------------
//
// D = L_cur - L_prev and L = D + L_prev_rec, modulo 2^16, in the tiles both frames code at one step (the others and key frames: D = L_cur),
// a mask bit set iff the result is not 0.  Header and types are copied, so both directions find the predicted tiles in their input stream.
// Both calls share
//   input    window_count_kernel and window_scan_kernel with no window on the stream and on the one frame at d_prev (as a stream of one
//            frame whose offsets delta_prev_kernel writes): S per group and each frame's unpack code
//   status   one wave: every frame's final status -- its own code, else 0x100 | its predecessor's; in the undelta call the predecessor is
//            an output frame, so the wave scans the chain (a frame with a code of its own or a key flag sets the state, any other passes it on)
//   scan     band_scan_kernel on the counts below: the prefixes, the frame's level count and size
//   offsets  frame_offsets_kernel
// The delta call's count and write are delta_kernel, a wave per (group, frame) as the union's: a lane per coefficient picks both levels by
// rank; the count reads the levels too, since it must know which differences are 0.
// The undelta call's are undelta_kernel: frame i needs output frame i - 1, so a wave owns one group through ALL frames of the call and the
// grid does not depend on their number.  It keeps the group's reconstructed levels dense in LDS ([tile][coefficient] u16, at most 4096)
// with their mask words, walks the frames in order and adds each frame's run of levels (found at the input pass's S) into them; a key frame
// and a tile whose step changed start from 0.  A word with no difference and no level held is skipped.  The write walk compacts each
// frame's non-zero levels in LDS and stores them with store_level_run; the first workgroup also writes every frame's header, types and
// padding.  Every output byte is stored once: two calls write the same bytes.

struct DeltaWs {
  WinWs in, prev;          // the input passes of the stream and of d_prev
  uint64_t* prev_offsets;  // [2] 0, prev_bytes
  uint32_t* prev_code;     // [1] d_prev's unpack code, as its input pass reports it
  uint32_t* cnt;           // [n][groups] non-zero results, then their exclusive prefix
  uint32_t *frame_bytes, *frame_levels, *status;  // [n]
};
DeltaWs delta_ws(Carver& c, uint32_t n, uint32_t groups) {
  DeltaWs s;
  s.in = window_ws(c, n, groups);
  const uint32_t one = n ? 1 : 0;  // an empty batch needs no workspace
  s.prev = window_ws(c, one, groups);
  s.prev_offsets = c.take<uint64_t>(2 * one);
  s.prev_code = c.take<uint32_t>(one);
  s.cnt = c.take<uint32_t>((uint64_t)n * groups);
  s.frame_bytes = c.take<uint32_t>(n);
  s.frame_levels = c.take<uint32_t>(n);
  s.status = c.take<uint32_t>(n);
  return s;
}

struct DeltaArgs {
  WindowArgs in;    // the stream as the input pass takes it; in.out, in.out_offsets, in.d_status: the call's
  WindowArgs prev;  // d_prev as a stream of one frame; prev.in null: none
  const uint32_t* key;  // [n] or null
  uint32_t n;
  uint32_t *cnt, *frame_bytes, *frame_levels, *status;
};

__global__ void delta_prev_kernel(uint64_t* offsets, uint64_t prev_bytes) {
  offsets[0] = 0;
  offsets[1] = prev_bytes;
}

__device__ __forceinline__ bool delta_key(const DeltaArgs& a, uint32_t i) {
  return (i == 0 && !a.prev.in) || (a.key && a.key[i] != 0);
}

// The frame that frame i > 0 of a call is coded against (include/svc_hip.h, "Temporal layers"): i - min(lowbit(i), period); period 1,
// the plain delta stream: i - 1.
__device__ __forceinline__ uint32_t temporal_ref(uint32_t i, uint32_t period) {
  return period == 1 ? i - 1 : i - min(i & (0u - i), period);
}

// the input frame before frame i: d_prev for frame 0.  Only for a frame that is not a key frame
__device__ __forceinline__ const uint8_t* delta_before(const DeltaArgs& a, uint32_t i, uint32_t period = 1) {
  return i == 0 ? a.prev.in : a.in.in + a.in.offsets[temporal_ref(i, period)];
}

// the step of the group's tile t in `frame`: the rule of svc_hip_dct_quant_frames on the frame's own header and types
__device__ __forceinline__ uint32_t tile_step(const Geom& g, const uint8_t* frame, const Group& gr, uint32_t t) {
  const uint32_t* h = reinterpret_cast<const uint32_t*>(frame);
  return tile_type(g, h + kHeaderWords, gr, t) == 0 ? h[kHBgStep] : h[kHFgStep];
}

// One wave.  e = the low byte of a frame's final status, the state the next frame inherits unless it is a key frame or has a code of its
// own.  CHAIN (undelta): e runs from frame to frame -- an inclusive scan in which a frame that sets the state overrides what came before it.
// Without CHAIN (delta) the predecessor is an input frame: its own code.
template <bool CHAIN>
__global__ __launch_bounds__(64) void delta_status_kernel(DeltaArgs a) {
  const uint32_t lane = threadIdx.x;
  uint32_t carry = a.prev.in ? a.prev.ws.status[0] & 0xFFu : 0u;  // of the frame before `base`
  for (uint32_t base = 0; base < a.n; base += 64) {
    const uint32_t i = base + lane;
    const bool live = i < a.n;
    const uint32_t own = live ? a.in.ws.status[i] : 0u;
    const bool key = live && delta_key(a, i);
    uint32_t e;
    if (CHAIN) {
      uint32_t sets = own != 0 || key, val = own & 0xFFu;
      for (uint32_t off = 1; off < 64; off <<= 1) {
        const uint32_t s2 = __shfl_up(sets, off, 64), v2 = __shfl_up(val, off, 64);
        if (lane >= off && !sets) sets = s2, val = v2;
      }
      e = sets ? val : carry;
      carry = __shfl(e, 63, 64);
    } else {
      const uint32_t before = i == 0 ? carry : (live ? a.in.ws.status[i - 1] & 0xFFu : 0u);
      e = own != 0 ? own & 0xFFu : (key ? 0u : before);
    }
    if (live) {
      const uint32_t st = own != 0 ? own : (e != 0 ? kStEnhancement | e : (uint32_t)kStOk);
      a.status[i] = st;
      a.in.d_status[i] = st;
    }
  }
}

// WRITE = false: the group's non-zero differences (0 for a frame that fails).  WRITE = true: its mask words and levels and, from the first
// workgroup of a frame, header, types and padding; dynamic LDS: select_write_lds(cap), cap = the coefficients of a full group
// `period`: 1 for svc_hip_delta_levels_frames (a constant there), else the temporal call's: the frame before is frame temporal_ref(i).
template <bool WRITE>
__device__ __forceinline__ void delta_body(const DeltaArgs& a, uint32_t cap, uint32_t period) {
  extern __shared__ uint16_t stage[];
  const Geom& g = a.in.g;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, gi = blockIdx.x * (kThreads / 64) + wave, i = blockIdx.y;
  const bool live = gi < g.groups;  // no early return: the barrier below is the workgroup's
  uint8_t* out = WRITE ? a.in.out + a.in.out_offsets[i] : nullptr;
  if (a.status[i] != kStOk) {  // 64 zero bytes; no frame is read
    if (WRITE) {
      if (blockIdx.x == 0 && threadIdx.x < kHeaderWords) reinterpret_cast<uint32_t*>(out)[threadIdx.x] = 0;
    } else if (live && lane == 0) {
      a.cnt[(size_t)i * g.groups + gi] = 0;
    }
    return;
  }
  const uint8_t* fc = a.in.in + a.in.offsets[i];
  uint16_t* buf = stage + (size_t)wave * cap;
  uint32_t cnt = 0;
  if (live) {
    const Group gr = group_of(g, gi);
    const uint8_t* fp = delta_key(a, i) ? nullptr : delta_before(a, i, period);  // (its own status is 0: this frame's would not be)
    const uint32_t* masks_c = group_masks(g, fc, gr.plane, gr);
    const uint32_t* masks_p = fp ? group_masks(g, fp, gr.plane, gr) : nullptr;
    uint32_t* masks_out = WRITE ? group_masks(g, out, gr.plane, gr) : nullptr;
    const uint16_t* lc = reinterpret_cast<const uint16_t*>(fc + g.levels_off) + a.in.ws.before[(size_t)i * g.groups + gi];
    const uint16_t* lp = nullptr;
    if (fp) lp = reinterpret_cast<const uint16_t*>(fp + g.levels_off) + (i == 0 ? a.prev.ws.before[gi] : a.in.ws.before[(size_t)temporal_ref(i, period) * g.groups + gi]);
    const uint32_t jobs = gr.nt * g.words;
    for (uint32_t j0 = 0; j0 < jobs; j0 += 64) {
      const uint32_t j = j0 + lane, n = min(64u, jobs - j0);
      uint64_t x = 0, y = 0;
      bool predicted = false;
      if (j < jobs) {
        x = load_mask(masks_c + 2 * j);
        if (fp) {
          const uint32_t t = j / g.words;
          y = load_mask(masks_p + 2 * j);
          predicted = tile_step(g, fc, gr, t) == tile_step(g, fp, gr, t);
        }
      }
      const uint32_t px = (uint32_t)__popcll(x), py = (uint32_t)__popcll(y);
      const uint32_t first_x = wave_exclusive_scan(px), first_y = wave_exclusive_scan(py);
      const uint64_t yp = predicted ? y : 0ull;  // the predecessor's levels of any other tile are passed over
      uint64_t keep = 0;                         // lane l: the new mask of word j0 + l
      for (uint32_t k = 0; k < n; ++k) {
        const uint64_t xk = readlane64(x, k), yk = readlane64(yp, k);
        if ((xk | yk) == 0) continue;  // (the whole wave)
        const uint32_t ax = (uint32_t)__builtin_amdgcn_readlane((int)first_x, k), ay = (uint32_t)__builtin_amdgcn_readlane((int)first_y, k);
        const uint16_t c = (xk >> lane) & 1u ? lc[ax + lane_rank(xk)] : (uint16_t)0;
        const uint16_t p = (yk >> lane) & 1u ? lp[ay + lane_rank(yk)] : (uint16_t)0;
        const uint16_t d = (uint16_t)(c - p);
        const uint64_t mk = __ballot(d != 0);
        if (WRITE) {
          if (d != 0) buf[cnt + lane_rank(mk)] = d;
          if (lane == k) keep = mk;
        }
        cnt += (uint32_t)__popcll(mk);
      }
      if (WRITE && j < jobs) store_mask(masks_out + 2 * j, keep);
      lc += (uint32_t)__builtin_amdgcn_readlane((int)(first_x + px), 63);
      if (fp) lp += (uint32_t)__builtin_amdgcn_readlane((int)(first_y + py), 63);
    }
  }
  if (!WRITE) {
    if (live && lane == 0) a.cnt[(size_t)i * g.groups + gi] = cnt;
    return;
  }
  __syncthreads();
  if (live) store_level_run(buf, cnt, reinterpret_cast<uint16_t*>(out + g.levels_off) + a.cnt[(size_t)i * g.groups + gi]);
  if (blockIdx.x != 0) return;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(fc);
  split_frame_edges(g, fc, out, src[kHFgStep], src[kHBgStep], a.frame_levels[i], a.frame_bytes[i]);
}

template <bool WRITE>
__global__ __launch_bounds__(256) void delta_kernel(DeltaArgs a, uint32_t cap) {
  delta_body<WRITE>(a, cap, 1);
}

template <bool WRITE>
__global__ __launch_bounds__(256) void delta_temporal_kernel(DeltaArgs a, uint32_t cap, uint32_t period) {
  delta_body<WRITE>(a, cap, period);
}

// WRITE = false: every frame's count of the group's non-zero levels.  WRITE = true: their mask words and levels and, from the first
// workgroup, every frame's header, types and padding.  blockDim.x / 64 waves, a group each through all frames; waves per workgroup and
// dynamic LDS are the split's write pass's (split_write_waves, split_write_lds(cap), cap = the coefficients of a full group): per wave the
// group's coefficients as u16, twice -- the levels held, and the frame's non-zero ones in order; the held levels' mask words are static
template <bool WRITE>
__global__ __launch_bounds__(256) void undelta_kernel(DeltaArgs a, uint32_t cap) {
  extern __shared__ uint16_t stage[];
  __shared__ uint64_t held_masks[kThreads / 64][kMaxJobs];
  const Geom& g = a.in.g;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, gi = blockIdx.x * (blockDim.x >> 6) + wave;
  const bool live = gi < g.groups;  // no early return: the barriers below are the workgroup's
  const Group gr = group_of(g, live ? gi : 0u);
  const uint32_t jobs = gr.nt * g.words, area = g.bw * g.bh;
  uint16_t* held = stage + (size_t)wave * 2 * cap;  // [tile][coefficient]: != 0 exactly where its bit of held_mask is set
  uint16_t* buf = held + cap;
  uint64_t* held_mask = held_masks[wave];
  for (uint32_t k = lane; k < cap; k += 64) held[k] = 0;
  for (uint32_t j = lane; j < jobs; j += 64) held_mask[j] = 0;
  // frame -1 is d_prev: it is added like a key frame and nothing is written for it.  Every condition on a frame is the workgroup's.
  for (int32_t i = a.prev.in && a.prev.ws.status[0] == kStOk ? -1 : 0; i < (int32_t)a.n; ++i) {
    const bool seed = i < 0;
    uint8_t* out = WRITE && !seed ? a.in.out + a.in.out_offsets[i] : nullptr;
    if (!seed && a.status[i] != kStOk) {  // 64 zero bytes; the frame is not read, and the next frame that passes is a key frame
      if (WRITE) {
        if (blockIdx.x == 0 && threadIdx.x < kHeaderWords) reinterpret_cast<uint32_t*>(out)[threadIdx.x] = 0;
      } else if (live && lane == 0) {
        a.cnt[(size_t)i * g.groups + gi] = 0;
      }
      continue;
    }
    const uint8_t* fc = seed ? a.prev.in : a.in.in + a.in.offsets[i];
    uint32_t cnt = 0;
    if (live) {
      const uint8_t* fp = seed || delta_key(a, (uint32_t)i) ? nullptr : delta_before(a, (uint32_t)i);
      const uint32_t* masks_c = group_masks(g, fc, gr.plane, gr);
      uint32_t* masks_out = out ? group_masks(g, out, gr.plane, gr) : nullptr;
      const uint16_t* lc = reinterpret_cast<const uint16_t*>(fc + g.levels_off) + (seed ? a.prev.ws.before[gi] : a.in.ws.before[(size_t)i * g.groups + gi]);
      for (uint32_t j0 = 0; j0 < jobs; j0 += 64) {
        const uint32_t j = j0 + lane, n = min(64u, jobs - j0);
        uint64_t x = 0, was = 0;
        uint32_t slot0 = 0;  // of the word's first coefficient
        bool predicted = false;
        if (j < jobs) {
          const uint32_t t = j / g.words;
          x = load_mask(masks_c + 2 * j);
          was = held_mask[j];
          slot0 = t * area + (j - t * g.words) * 64;
          if (fp) predicted = tile_step(g, fc, gr, t) == tile_step(g, fp, gr, t);
        }
        const uint32_t px = (uint32_t)__popcll(x), first_x = wave_exclusive_scan(px);
        const uint64_t predicted_words = __ballot(predicted);
        uint64_t keep = 0;  // lane l: the new mask of word j0 + l
        for (uint32_t k = 0; k < n; ++k) {
          const uint64_t xk = readlane64(x, k), wk = readlane64(was, k);
          if ((xk | wk) == 0) continue;  // (the whole wave) nothing to add and nothing held: the word stays 0
          const uint32_t ax = (uint32_t)__builtin_amdgcn_readlane((int)first_x, k);
          const uint32_t slot = (uint32_t)__builtin_amdgcn_readlane((int)slot0, k) + lane;
          const uint16_t d = (xk >> lane) & 1u ? lc[ax + lane_rank(xk)] : (uint16_t)0;
          const uint16_t p = ((predicted_words >> k) & 1u) && ((wk >> lane) & 1u) ? held[slot] : (uint16_t)0;
          const uint16_t lv = (uint16_t)(d + p);
          if (((xk | wk) >> lane) & 1u) held[slot] = lv;  // (no bit is set past the tile's area: such a frame fails)
          const uint64_t mk = __ballot(lv != 0);
          if (lane == k) keep = mk;
          if (WRITE && out && lv != 0) buf[cnt + lane_rank(mk)] = lv;
          cnt += (uint32_t)__popcll(mk);
        }
        if (j < jobs) {
          held_mask[j] = keep;
          if (masks_out) store_mask(masks_out + 2 * j, keep);
        }
        lc += (uint32_t)__builtin_amdgcn_readlane((int)(first_x + px), 63);
      }
    }
    if (seed) continue;
    if (!WRITE) {
      if (live && lane == 0) a.cnt[(size_t)i * g.groups + gi] = cnt;
      continue;
    }
    __syncthreads();
    if (live) store_level_run(buf, cnt, reinterpret_cast<uint16_t*>(out + g.levels_off) + a.cnt[(size_t)i * g.groups + gi]);
    if (blockIdx.x == 0) {
      const uint32_t* src = reinterpret_cast<const uint32_t*>(fc);
      split_frame_edges(g, fc, out, src[kHFgStep], src[kHBgStep], a.frame_levels[i], a.frame_bytes[i]);
    }
    __syncthreads();  // the next frame's levels go to buf again
  }
}

// ---- temporal layers of the delta stream (svc_hip_delta_levels_temporal_frames, svc_hip_undelta_levels_temporal_frames,
// svc_hip_decode_delta_levels_temporal_frames; include/svc_hip.h states them) ------------------------------------------------------------
//
// Frame i is coded against frame temporal_ref(i) = i - min(lowbit(i), period), period 2 or 4 = 2^T (period 1 takes the calls above).  The
// frames of layer 0 (i % period == 0) form a chain of their own, those of layer l hang on a frame of a lower layer, and the odd frames
// (layer T) are referenced by none.  The delta call is delta_kernel's body with that frame before.  The kernels that rebuild keep one
// state per layer below T: a frame of layer l < T is rebuilt INTO state l from the state of its reference's layer, an odd frame from it
// into nothing that lasts.  (State l therefore holds the latest frame of layer l, not the latest multiple of 2^(T - l): a frame reads the
// state of the layer its reference has, which is the same frame, and no frame is stored twice.)  Rebuilt into another state than it reads,
// a coefficient is written wherever the difference, the reference's mask or the destination's old mask has a bit -- else a level of the
// frame overwritten would survive.

__device__ __forceinline__ uint32_t temporal_src_state(uint32_t i, uint32_t period) { return period == 4 && (i & 3u) == 3u ? 1u : 0u; }
// the state frame i is rebuilt into; `none` for an odd frame
__device__ __forceinline__ uint32_t temporal_dst_state(uint32_t i, uint32_t period, uint32_t none) {
  const uint32_t r = i & (period - 1);
  return r == 0 ? 0u : (r == 2 ? 1u : none);
}

// delta_status_kernel for a period of 2 or 4.  One wave.  Without CHAIN (delta) the frame before is an input frame: its own code.  CHAIN
// (undelta, decode): the frames of layer 0 are scanned as delta_status_kernel scans all frames; then, layer by layer, every other frame
// takes the state of its reference, whose final status is in a.status by then -- T steps of independent frames, whatever n.
template <bool CHAIN>
__global__ __launch_bounds__(64) void delta_temporal_status_kernel(DeltaArgs a, uint32_t period) {
  const uint32_t lane = threadIdx.x;
  const uint32_t carry0 = a.prev.in ? a.prev.ws.status[0] & 0xFFu : 0u;
  auto finish = [&](uint32_t i, uint32_t own, uint32_t e) {
    const uint32_t st = own != 0 ? own : (e != 0 ? kStEnhancement | e : (uint32_t)kStOk);
    a.status[i] = st;
    a.in.d_status[i] = st;
  };
  if (!CHAIN) {
    for (uint32_t i = lane; i < a.n; i += 64) {
      const uint32_t own = a.in.ws.status[i];
      const uint32_t before = i == 0 ? carry0 : a.in.ws.status[temporal_ref(i, period)] & 0xFFu;
      finish(i, own, own != 0 ? own & 0xFFu : (delta_key(a, i) ? 0u : before));
    }
    return;
  }
  uint32_t carry = carry0;  // of the layer-0 frame before `base`
  const uint32_t n0 = (a.n + period - 1) / period;
  for (uint32_t base = 0; base < n0; base += 64) {
    const uint32_t i = (base + lane) * period;
    const bool live = base + lane < n0;
    const uint32_t own = live ? a.in.ws.status[i] : 0u;
    uint32_t sets = own != 0 || (live && delta_key(a, i)), val = own & 0xFFu;
    for (uint32_t off = 1; off < 64; off <<= 1) {
      const uint32_t s2 = __shfl_up(sets, off, 64), v2 = __shfl_up(val, off, 64);
      if (lane >= off && !sets) sets = s2, val = v2;
    }
    const uint32_t e = sets ? val : carry;
    carry = __shfl(e, 63, 64);
    if (live) finish(i, own, e);
  }
  for (uint32_t stride = period >> 1; stride >= 1; stride >>= 1) {
    __threadfence();  // the layer below is in a.status
    __syncthreads();
    for (uint32_t i = (2 * lane + 1) * stride; i < a.n; i += 128 * stride) {  // lowbit(i) == stride: its reference is i - stride
      const uint32_t own = a.in.ws.status[i];
      finish(i, own, own != 0 ? own & 0xFFu : (delta_key(a, i) ? 0u : a.status[i - stride] & 0xFFu));
    }
  }
}

// two waves per workgroup, one where a group is a tile above 2048 coefficients; per wave two states and the frame's run of levels
constexpr uint32_t temporal_waves(uint32_t cap) { return cap > kGroupCoeffs ? 1 : 2; }
constexpr uint32_t temporal_lds(uint32_t cap) { return temporal_waves(cap) * 3 * cap * (uint32_t)sizeof(uint16_t); }
static_assert(temporal_lds(kGroupCoeffs) <= 24576 && temporal_lds(kMaxTileCoeffs) <= 24576,
              "the temporal undelta holds at most 24 KB of levels per workgroup, and 8 KB of mask words");

// undelta_kernel for a period of 2 or 4: blockDim.x / 64 waves (temporal_waves), a group each through all frames; dynamic LDS
// temporal_lds(cap): per wave states 0 and 1, [tile][coefficient] u16, then the frame's non-zero levels in order.  Period 2 uses state 0 only.
template <bool WRITE>
__global__ __launch_bounds__(128) void undelta_temporal_kernel(DeltaArgs a, uint32_t cap, uint32_t period) {
  extern __shared__ uint16_t stage[];
  __shared__ uint64_t state_masks[2][2][kMaxJobs];  // [wave][state][word]
  constexpr uint32_t kNone = 2;
  const Geom& g = a.in.g;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, gi = blockIdx.x * (blockDim.x >> 6) + wave;
  const bool live = gi < g.groups;  // no early return: the barriers below are the workgroup's
  const Group gr = group_of(g, live ? gi : 0u);
  const uint32_t jobs = gr.nt * g.words, area = g.bw * g.bh;
  uint16_t* states = stage + (size_t)wave * 3 * cap;  // a level != 0 exactly where its bit of the state's mask is set
  uint16_t* buf = states + 2 * cap;
  for (uint32_t k = lane; k < 2 * cap; k += 64) states[k] = 0;
  for (uint32_t j = lane; j < jobs; j += 64) state_masks[wave][0][j] = 0, state_masks[wave][1][j] = 0;
  // frame -1 is d_prev, the frame at index -period: it goes into state 0 like a key frame and nothing is written for it
  for (int32_t i = a.prev.in && a.prev.ws.status[0] == kStOk ? -1 : 0; i < (int32_t)a.n; ++i) {
    const bool seed = i < 0;
    uint8_t* out = WRITE && !seed ? a.in.out + a.in.out_offsets[i] : nullptr;
    if (!seed && a.status[i] != kStOk) {  // 64 zero bytes; the frame is not read, and no frame that passes hangs on it
      if (WRITE) {
        if (blockIdx.x == 0 && threadIdx.x < kHeaderWords) reinterpret_cast<uint32_t*>(out)[threadIdx.x] = 0;
      } else if (live && lane == 0) {
        a.cnt[(size_t)i * g.groups + gi] = 0;
      }
      continue;
    }
    const uint8_t* fc = seed ? a.prev.in : a.in.in + a.in.offsets[i];
    const uint32_t src = seed ? 0u : temporal_src_state((uint32_t)i, period);
    const uint32_t dst = seed ? 0u : temporal_dst_state((uint32_t)i, period, kNone);
    uint32_t cnt = 0;
    if (live) {
      const uint8_t* fp = seed || delta_key(a, (uint32_t)i) ? nullptr : delta_before(a, (uint32_t)i, period);
      const uint32_t* masks_c = group_masks(g, fc, gr.plane, gr);
      uint32_t* masks_out = out ? group_masks(g, out, gr.plane, gr) : nullptr;
      const uint16_t* lc = reinterpret_cast<const uint16_t*>(fc + g.levels_off) + (seed ? a.prev.ws.before[gi] : a.in.ws.before[(size_t)i * g.groups + gi]);
      const uint16_t* from = states + src * cap;
      uint16_t* into = dst == kNone ? nullptr : states + dst * cap;
      const uint64_t* from_mask = state_masks[wave][src];
      uint64_t* into_mask = dst == kNone ? nullptr : state_masks[wave][dst];
      for (uint32_t j0 = 0; j0 < jobs; j0 += 64) {
        const uint32_t j = j0 + lane, n = min(64u, jobs - j0);
        uint64_t x = 0, ref = 0, old = 0;
        uint32_t slot0 = 0;  // of the word's first coefficient
        bool predicted = false;
        if (j < jobs) {
          const uint32_t t = j / g.words;
          x = load_mask(masks_c + 2 * j);
          ref = from_mask[j];
          if (into_mask) old = into_mask[j];
          slot0 = t * area + (j - t * g.words) * 64;
          if (fp) predicted = tile_step(g, fc, gr, t) == tile_step(g, fp, gr, t);
        }
        const uint32_t px = (uint32_t)__popcll(x), first_x = wave_exclusive_scan(px);
        const uint64_t predicted_words = __ballot(predicted);
        uint64_t keep = 0;  // lane l: the new mask of word j0 + l
        for (uint32_t k = 0; k < n; ++k) {
          const uint64_t xk = readlane64(x, k), rk = readlane64(ref, k), any = xk | rk | readlane64(old, k);
          if (any == 0) continue;  // (the whole wave) nothing to add, nothing to add to and nothing to overwrite: the word stays 0
          const uint32_t ax = (uint32_t)__builtin_amdgcn_readlane((int)first_x, k);
          const uint32_t slot = (uint32_t)__builtin_amdgcn_readlane((int)slot0, k) + lane;
          const uint16_t d = (xk >> lane) & 1u ? lc[ax + lane_rank(xk)] : (uint16_t)0;
          const uint16_t p = ((predicted_words >> k) & 1u) && ((rk >> lane) & 1u) ? from[slot] : (uint16_t)0;
          const uint16_t lv = (uint16_t)(d + p);
          if (into && ((any >> lane) & 1u)) into[slot] = lv;  // (no bit is set past the tile's area: such a frame fails)
          const uint64_t mk = __ballot(lv != 0);
          if (lane == k) keep = mk;
          if (WRITE && out && lv != 0) buf[cnt + lane_rank(mk)] = lv;
          cnt += (uint32_t)__popcll(mk);
        }
        if (j < jobs) {
          if (into_mask) into_mask[j] = keep;
          if (masks_out) store_mask(masks_out + 2 * j, keep);
        }
        lc += (uint32_t)__builtin_amdgcn_readlane((int)(first_x + px), 63);
      }
    }
    if (seed) continue;
    if (!WRITE) {
      if (live && lane == 0) a.cnt[(size_t)i * g.groups + gi] = cnt;
      continue;
    }
    __syncthreads();
    if (live) store_level_run(buf, cnt, reinterpret_cast<uint16_t*>(out + g.levels_off) + a.cnt[(size_t)i * g.groups + gi]);
    if (blockIdx.x == 0) {
      const uint32_t* hdr = reinterpret_cast<const uint32_t*>(fc);
      split_frame_edges(g, fc, out, hdr[kHFgStep], hdr[kHBgStep], a.frame_levels[i], a.frame_bytes[i]);
    }
    __syncthreads();  // the next frame's levels go to buf again
  }
}

// ---- decode of a delta stream: the undelta and the reconstruction in one kernel (svc_hip_decode_delta_levels_frames; include/svc_hip.h
// states it) ------------------------------------------------------------------------------------------------------------------------------
//
// The passes in front are the undelta's (input, status); its count, scan, offsets and write fall away, since no reconstructed stream is
// written.  One workgroup of decode_body's shape -- the same tiles in all three planes, thread (t, j) owns coefficient row j of tile t --
// carries its group through ALL frames of the call.  It holds the three planes' reconstructed levels dense in LDS ([plane][tile][coefficient]
// u16) with their mask words.  Per frame, every wave reads the plane's mask words of the delta frame (a lane per word) and scans their
// popcounts itself, so the add needs no barrier: wave w adds words w, w + 4, .. exactly as undelta_kernel does, a lane per coefficient by
// rank.  After one barrier thread (t, j) reads its row from the held levels -- a plain LDS read where decode_body gathers by rank -- and
// the passes are idct_core.hpp's.  The int16 level of every coefficient is the one decode_body would gather from the undelta's output, so
// d_rec has the bits of svc_hip_undelta_levels_frames + svc_hip_decode_levels_frames.
//
// d_last, the reconstructed SVCQ frame of the call's last frame: the workgroup stores its mask words at their place, its count per plane
// and its non-zero levels as one run per (plane, group) at the group's worst-case place in the workspace; decode_delta_last_scan_kernel
// gives each run its place and the frame its size, decode_delta_last_write_kernel moves the runs (a wave each, store_level_run) and writes
// header, types and padding.  A last frame that failed is 64 zero bytes.  Every output byte is stored once.

struct DecodeDeltaWs {
  WinWs in, prev;          // the input passes of the stream and of d_prev
  uint64_t* prev_offsets;  // [2] 0, prev_bytes
  uint32_t* prev_code;     // [1] d_prev's unpack code, as its input pass reports it
  uint32_t* status;        // [n] the final statuses
  uint32_t *last_cnt, *last_first;  // [groups] the last frame's non-zero levels per group, and their exclusive prefix
  uint32_t* last_head;     // [2] the last frame's level count and size
  uint16_t* last_runs;     // [groups][tpg * bw * bh]
};
DecodeDeltaWs decode_delta_ws(Carver& c, uint32_t n, uint32_t groups, uint32_t cap) {
  DecodeDeltaWs s;
  s.in = window_ws(c, n, groups);
  const uint32_t one = n ? 1 : 0;  // an empty batch needs no workspace
  s.prev = window_ws(c, one, groups);
  s.prev_offsets = c.take<uint64_t>(2 * one);
  s.prev_code = c.take<uint32_t>(one);
  s.status = c.take<uint32_t>(n);
  s.last_cnt = c.take<uint32_t>((uint64_t)one * groups);
  s.last_first = c.take<uint32_t>((uint64_t)one * groups);
  s.last_head = c.take<uint32_t>(2 * one);
  s.last_runs = c.take<uint16_t>((uint64_t)one * groups * cap);
  return s;
}

struct DecodeDeltaArgs {
  DeltaArgs d;           // d.in.out, d.in.out_offsets, d.cnt, d.frame_bytes, d.frame_levels are null: no stream is written
  const uint32_t* gaze;  // [n][4] or null
  float* rec;            // [n][h][w][3]
  float fg, bg;          // the decoder's steps
  uint8_t* last;         // or null: not wanted
  uint64_t* last_bytes;
  uint32_t *last_cnt, *last_first, *last_head;
  uint16_t* last_runs;
  uint32_t cap;          // coefficients of a full group: the pitch of last_runs
};

__device__ __forceinline__ bool bit_of(uint64_t m, uint32_t b) { return (m >> b) & 1u; }

template <int N>
__global__ __launch_bounds__(256) void decode_delta_kernel(DecodeDeltaArgs args) {
  constexpr uint32_t kArea = N * N, kWords = kArea / 64, kJobs = kGroupCoeffs / 64;  // a mask word is 64 adjacent held levels
  constexpr uint32_t kRows = kGroupCoeffs / N;
  constexpr uint32_t kWaves = kThreads / 64;
  __shared__ uint16_t held[3][kGroupCoeffs];  // [plane][tile][coefficient]: != 0 exactly where its bit of held_mask is set
  __shared__ uint64_t held_mask[3][kJobs];
  __shared__ double rows[kRows * (N + 1)];
  const DeltaArgs& a = args.d;
  const Geom& g = a.in.g;
  const uint32_t gi0 = blockIdx.x, tid = threadIdx.x, lane = tid & 63u;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
  const Group gr = group_of(g, gi0);  // plane 0's group; planes 1 and 2 hold the same tiles
  const uint32_t jobs = gr.nt * kWords, per_plane = g.tiles_y * g.gx;
  const uint32_t t = tid / N, j = tid - t * N;
  const bool active = t < gr.nt;  // an idle thread stays in every barrier below
  for (uint32_t k = tid; k < 3 * kGroupCoeffs; k += kThreads) (&held[0][0])[k] = 0;
  for (uint32_t k = tid; k < 3 * kJobs; k += kThreads) (&held_mask[0][0])[k] = 0;
  __syncthreads();
  // frame -1 is d_prev: it is added like a key frame and nothing is decoded for it.  Every condition on a frame is the workgroup's.
  for (int32_t i = a.prev.in && a.prev.ws.status[0] == kStOk ? -1 : 0; i < (int32_t)a.n; ++i) {
    const bool seed = i < 0;
    float* dst = seed ? nullptr : args.rec + (((size_t)i * g.h + gr.y0) * g.w + gr.x0 + t * N + j) * 3;
    if (!seed && a.status[i] != kStOk) {  // zeros; the frame is not read, and the next frame that passes is a key frame
      if (active) {
#pragma unroll
        for (int y = 0; y < N; ++y) {
          float* p = dst + (size_t)y * g.w * 3;
          p[0] = 0.f; p[1] = 0.f; p[2] = 0.f;
        }
      }
      continue;
    }
    const uint8_t* fc = seed ? a.prev.in : a.in.in + a.in.offsets[i];
    const uint8_t* fp = seed || delta_key(a, (uint32_t)i) ? nullptr : delta_before(a, (uint32_t)i);
    const bool same_step = fp && lane < gr.nt && tile_step(g, fc, gr, lane) == tile_step(g, fp, gr, lane);
    const uint64_t predicted_tiles = __ballot(same_step);  // (a group has at most 32 tiles)
    const uint32_t* first_level = seed ? a.prev.ws.before : a.in.ws.before + (size_t)i * g.groups;
#pragma unroll
    for (uint32_t c = 0; c < 3; ++c) {
      const uint32_t* masks = group_masks(g, fc, c, gr);
      const uint16_t* lc = reinterpret_cast<const uint16_t*>(fc + g.levels_off) + first_level[c * per_plane + gi0];
      const uint64_t x = lane < jobs ? load_mask(masks + 2 * lane) : 0ull;
      const uint32_t first_x = wave_exclusive_scan((uint32_t)__popcll(x));
      for (uint32_t k = wave; k < jobs; k += kWaves) {
        const uint64_t xk = readlane64(x, k), wk = readlane64(held_mask[c][k], 0);
        if ((xk | wk) == 0) continue;  // (the whole wave) nothing to add and nothing held: the word stays 0
        const uint32_t ax = (uint32_t)__builtin_amdgcn_readlane((int)first_x, k), slot = k * 64 + lane;
        const uint16_t d = bit_of(xk, lane) ? lc[ax + lane_rank(xk)] : (uint16_t)0;
        const uint16_t p = bit_of(predicted_tiles, k / kWords) && bit_of(wk, lane) ? held[c][slot] : (uint16_t)0;
        const uint16_t lv = (uint16_t)(d + p);
        if (bit_of(xk | wk, lane)) held[c][slot] = lv;  // (no bit is set past the tile's area: such a frame fails)
        const uint64_t mk = __ballot(lv != 0);
        if (lane == 0) held_mask[c][k] = mk;
      }
    }
    __syncthreads();
    if (seed) continue;
    float enc = 0.f, dec = 1.f;
    if (active) {
      const uint32_t* hdr = reinterpret_cast<const uint32_t*>(fc);
      const uint32_t type = tile_type(g, hdr + kHeaderWords, gr, t);
      const bool in_gaze = gazed(args.gaze, (uint32_t)i, gr.x0 + t * N, gr.y0);
      enc = (float)(type == 0 ? hdr[kHBgStep] : hdr[kHFgStep]);
      dec = in_gaze ? 1.f : (type == 0 ? args.bg : args.fg);
    }
    float out[3][N];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (active) {
        const uint16_t* row = &held[c][t * kArea + j * N];
        float v[N];
#pragma unroll
        for (int q = 0; q < N; ++q) v[q] = (float)(int16_t)row[q] * enc;
        invert_row<N>(v, dec, rows, t, j);
      }
      __syncthreads();
      if (active) invert_column<N>(rows, t, j, out[c]);
      if (c < 2) __syncthreads();  // the next plane reuses rows; the next frame writes them only after its own barrier
    }
    if (active) store_bgr_column<N>(dst, g.w, out);
  }
  if (!args.last || a.status[a.n - 1] != kStOk) return;  // (the whole workgroup)
  __syncthreads();
#pragma unroll
  for (uint32_t c = 0; c < 3; ++c) {
    const uint32_t gi = c * per_plane + gi0;
    const uint64_t m = lane < jobs ? held_mask[c][lane] : 0ull;
    const uint32_t pc = (uint32_t)__popcll(m), first = wave_exclusive_scan(pc);
    uint16_t* run = args.last_runs + (size_t)gi * args.cap;
    for (uint32_t k = wave; k < jobs; k += kWaves) {
      const uint64_t mk = readlane64(m, k);
      const uint32_t at = (uint32_t)__builtin_amdgcn_readlane((int)first, k);
      if (bit_of(mk, lane)) run[at + lane_rank(mk)] = held[c][k * 64 + lane];
    }
    if (wave == 0) {
      uint32_t* masks_out = group_masks(g, args.last, c, gr);
      if (lane < jobs) store_mask(masks_out + 2 * lane, m);
      const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)(first + pc), 63);
      if (lane == 0) args.last_cnt[gi] = total;
    }
  }
}

// one workgroup: the last frame's runs get their places, the frame its level count and size; a failed frame is 64 zero bytes
__global__ __launch_bounds__(256) void decode_delta_last_scan_kernel(DecodeDeltaArgs args) {
  __shared__ uint32_t red[kThreads / 64];
  const DeltaArgs& a = args.d;
  const Geom& g = a.in.g;
  if (a.status[a.n - 1] != kStOk) {  // (the whole workgroup)
    if (threadIdx.x < kHeaderWords) reinterpret_cast<uint32_t*>(args.last)[threadIdx.x] = 0;
    if (threadIdx.x == 0) *args.last_bytes = kHeaderBytes;
    return;
  }
  const uint32_t carry = scan_counts(args.last_cnt, args.last_first, g.groups, 0, red);
  if (threadIdx.x == 0) {
    const uint32_t bytes = (uint32_t)up16(g.levels_off + 2ull * carry);
    args.last_head[0] = carry;
    args.last_head[1] = bytes;
    *args.last_bytes = bytes;
  }
}

// a wave per group: its run of levels to its place in d_last; the first workgroup also writes header, types and padding
__global__ __launch_bounds__(256) void decode_delta_last_write_kernel(DecodeDeltaArgs args) {
  const DeltaArgs& a = args.d;
  const Geom& g = a.in.g;
  if (a.status[a.n - 1] != kStOk) return;
  const uint32_t gi = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
  if (gi < g.groups)
    store_level_run(args.last_runs + (size_t)gi * args.cap, args.last_cnt[gi],
                    reinterpret_cast<uint16_t*>(args.last + g.levels_off) + args.last_first[gi]);
  if (blockIdx.x != 0) return;
  const uint8_t* fc = a.in.in + a.in.offsets[a.n - 1];
  const uint32_t* src = reinterpret_cast<const uint32_t*>(fc);
  split_frame_edges(g, fc, args.last, src[kHFgStep], src[kHBgStep], args.last_head[0], args.last_head[1]);
}

// ---- decode of a delta stream with temporal layers (svc_hip_decode_delta_levels_temporal_frames) ----------------------------------------
//
// decode_delta_kernel's workgroup with T + 1 dense states in LDS where that kernel has one: states 0 .. T - 1 are the temporal undelta's
// (the latest rebuilt frame of each layer below T), state T receives the odd frames, which no frame refers to.  Every frame is rebuilt
// from the state of its reference INTO the state of its own layer -- no copy: the add reads one buffer and writes the other, wherever the
// difference, the reference's mask or the destination's old mask has a bit -- and the rows are read from the state just written.
// Static LDS, period 2: 2 x 12.75 KB of states + 18 KB of rows = 43.5 KB, three workgroups (12 waves) per CU; period 4: 3 x 12.75 + 18 =
// 56.25 KB, two workgroups (8 waves) per CU, where decode_delta_kernel's 30.75 KB admits five.
//
// d_last is the frame the next call refers to, period * ((n - 1) / period): state 0 after the last frame.  It goes through
// decode_delta_last_scan_kernel and decode_delta_last_write_kernel, which are handed that frame as the call's last.
template <int N, int T>
__global__ __launch_bounds__(256) void decode_delta_temporal_kernel(DecodeDeltaArgs args, uint32_t last_frame) {
  constexpr uint32_t kArea = N * N, kWords = kArea / 64, kJobs = kGroupCoeffs / 64;  // a mask word is 64 adjacent levels of a state
  constexpr uint32_t kRows = kGroupCoeffs / N;
  constexpr uint32_t kWaves = kThreads / 64;
  constexpr uint32_t kStates = T + 1, kPeriod = 1u << T;
  __shared__ uint16_t state[kStates][3][kGroupCoeffs];  // [state][plane][tile][coefficient]: != 0 exactly where its bit of state_mask is set
  __shared__ uint64_t state_mask[kStates][3][kJobs];
  __shared__ double rows[kRows * (N + 1)];
  const DeltaArgs& a = args.d;
  const Geom& g = a.in.g;
  const uint32_t gi0 = blockIdx.x, tid = threadIdx.x, lane = tid & 63u;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
  const Group gr = group_of(g, gi0);  // plane 0's group; planes 1 and 2 hold the same tiles
  const uint32_t jobs = gr.nt * kWords, per_plane = g.tiles_y * g.gx;
  const uint32_t t = tid / N, j = tid - t * N;
  const bool active = t < gr.nt;  // an idle thread stays in every barrier below
  for (uint32_t k = tid; k < kStates * 3 * kGroupCoeffs; k += kThreads) (&state[0][0][0])[k] = 0;
  for (uint32_t k = tid; k < kStates * 3 * kJobs; k += kThreads) (&state_mask[0][0][0])[k] = 0;
  __syncthreads();
  // frame -1 is d_prev, the frame at index -period: it goes into state 0 like a key frame and nothing is decoded for it
  for (int32_t i = a.prev.in && a.prev.ws.status[0] == kStOk ? -1 : 0; i < (int32_t)a.n; ++i) {
    const bool seed = i < 0;
    float* dst = seed ? nullptr : args.rec + (((size_t)i * g.h + gr.y0) * g.w + gr.x0 + t * N + j) * 3;
    if (!seed && a.status[i] != kStOk) {  // zeros; the frame is not read, and no frame that passes hangs on it
      if (active) {
#pragma unroll
        for (int y = 0; y < N; ++y) {
          float* p = dst + (size_t)y * g.w * 3;
          p[0] = 0.f; p[1] = 0.f; p[2] = 0.f;
        }
      }
      continue;
    }
    const uint8_t* fc = seed ? a.prev.in : a.in.in + a.in.offsets[i];
    const uint8_t* fp = seed || delta_key(a, (uint32_t)i) ? nullptr : delta_before(a, (uint32_t)i, kPeriod);
    const uint32_t from = seed ? 0u : temporal_src_state((uint32_t)i, kPeriod);
    const uint32_t into = seed ? 0u : temporal_dst_state((uint32_t)i, kPeriod, (uint32_t)T);
    const bool same_step = fp && lane < gr.nt && tile_step(g, fc, gr, lane) == tile_step(g, fp, gr, lane);
    const uint64_t predicted_tiles = __ballot(same_step);  // (a group has at most 32 tiles)
    const uint32_t* first_level = seed ? a.prev.ws.before : a.in.ws.before + (size_t)i * g.groups;
#pragma unroll
    for (uint32_t c = 0; c < 3; ++c) {
      const uint32_t* masks = group_masks(g, fc, c, gr);
      const uint16_t* lc = reinterpret_cast<const uint16_t*>(fc + g.levels_off) + first_level[c * per_plane + gi0];
      const uint64_t x = lane < jobs ? load_mask(masks + 2 * lane) : 0ull;
      const uint32_t first_x = wave_exclusive_scan((uint32_t)__popcll(x));
      for (uint32_t k = wave; k < jobs; k += kWaves) {
        const uint64_t xk = readlane64(x, k), rk = readlane64(state_mask[from][c][k], 0);
        const uint64_t any = xk | rk | readlane64(state_mask[into][c][k], 0);
        if (any == 0) continue;  // (the whole wave) nothing to add, nothing to add to and nothing to overwrite: the word stays 0
        const uint32_t ax = (uint32_t)__builtin_amdgcn_readlane((int)first_x, k), slot = k * 64 + lane;
        const uint16_t d = bit_of(xk, lane) ? lc[ax + lane_rank(xk)] : (uint16_t)0;
        const uint16_t p = bit_of(predicted_tiles, k / kWords) && bit_of(rk, lane) ? state[from][c][slot] : (uint16_t)0;
        const uint16_t lv = (uint16_t)(d + p);
        if (bit_of(any, lane)) state[into][c][slot] = lv;  // (no bit is set past the tile's area: such a frame fails)
        const uint64_t mk = __ballot(lv != 0);
        if (lane == 0) state_mask[into][c][k] = mk;
      }
    }
    __syncthreads();
    if (seed) continue;
    float enc = 0.f, dec = 1.f;
    if (active) {
      const uint32_t* hdr = reinterpret_cast<const uint32_t*>(fc);
      const uint32_t type = tile_type(g, hdr + kHeaderWords, gr, t);
      const bool in_gaze = gazed(args.gaze, (uint32_t)i, gr.x0 + t * N, gr.y0);
      enc = (float)(type == 0 ? hdr[kHBgStep] : hdr[kHFgStep]);
      dec = in_gaze ? 1.f : (type == 0 ? args.bg : args.fg);
    }
    float out[3][N];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (active) {
        const uint16_t* row = &state[into][c][t * kArea + j * N];
        float v[N];
#pragma unroll
        for (int q = 0; q < N; ++q) v[q] = (float)(int16_t)row[q] * enc;
        invert_row<N>(v, dec, rows, t, j);
      }
      __syncthreads();
      if (active) invert_column<N>(rows, t, j, out[c]);
      if (c < 2) __syncthreads();  // the next plane reuses rows; the next frame writes them only after its own barrier
    }
    if (active) store_bgr_column<N>(dst, g.w, out);
  }
  if (!args.last || a.status[last_frame] != kStOk) return;  // (the whole workgroup)
  __syncthreads();
#pragma unroll
  for (uint32_t c = 0; c < 3; ++c) {
    const uint32_t gi = c * per_plane + gi0;
    const uint64_t m = lane < jobs ? state_mask[0][c][lane] : 0ull;
    const uint32_t pc = (uint32_t)__popcll(m), first = wave_exclusive_scan(pc);
    uint16_t* run = args.last_runs + (size_t)gi * args.cap;
    for (uint32_t k = wave; k < jobs; k += kWaves) {
      const uint64_t mk = readlane64(m, k);
      const uint32_t at = (uint32_t)__builtin_amdgcn_readlane((int)first, k);
      if (bit_of(mk, lane)) run[at + lane_rank(mk)] = state[0][c][k * 64 + lane];
    }
    if (wave == 0) {
      uint32_t* masks_out = group_masks(g, args.last, c, gr);
      if (lane < jobs) store_mask(masks_out + 2 * lane, m);
      const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)(first + pc), 63);
      if (lane == 0) args.last_cnt[gi] = total;
    }
  }
}

// ---- decode of a delta stream at reduced size (svc_hip_decode_delta_levels_reduced_frames; include/svc_hip.h states it) ------------------
//
// The delta chain is per coefficient, so a decoder of the first K x K coefficients carries only those through time.  The passes in front
// and the workspace are decode_delta_kernel's; the workgroup is decode_reduced_kernel's: thread (t, j < K) for the group's tiles in all
// three planes, and like decode_delta_kernel's it walks ALL frames of the call.  A thread owns the same K coefficients -- row j of tile t
// -- of each plane in every frame, so the held levels are 3 K registers per thread: no level is held in LDS, and no other thread ever
// needs them.  Per frame, wave 0 loads and scans the delta frame's mask words of the three planes (decode_reduced_kernel's first step);
// after a barrier the thread gathers its K differences by rank, adds them modulo 2^16 to what it holds if its own tile is predicted (else
// to 0: a key frame, d_prev, a tile whose step changed), dequantises and runs idct_core.hpp's reduced row pass; after a second barrier,
// the column pass and the store.  Those two barriers also order the job arrays and the slab between frames: wave 0 writes frame i + 1's
// words only after every wave has passed frame i's second barrier, behind its gather.  The held int16 is the level decode_reduced_kernel
// would gather from the undelta's output, so d_rec has the bits of svc_hip_undelta_levels_frames + svc_hip_decode_levels_reduced_frames.
// Levels outside K x K are never read: the frames and d_prev may be their band (0, 0, K, K).
//
// d_last, the band (0, 0, K, K) of the call's last frame as an SVCQ frame, goes through decode_delta_kernel's scan and write passes: the
// threads put their rows' non-zero bits to LDS, wave 0 makes the group's full-size mask words of them (bits only inside K x K), stores
// them and their count, and every thread puts its non-zero levels at their rank in the group's run in the workspace.
// (args.rec: [n][h K / N][w K / N][3])
template <int N, int K>
__global__ __launch_bounds__(reduced_threads(N, K)) void decode_delta_reduced_kernel(DecodeDeltaArgs args) {
  constexpr uint32_t kTiles = kGroupCoeffs / (N * N), kWords = N * N / 64, kJobs = kTiles * kWords;  // tiles and mask words of a group
  constexpr uint32_t kRowsPerWord = 64 / N;  // coefficient rows of a tile in one mask word
  static_assert(kJobs <= 64, "one wave scans a group's mask words");
  __shared__ uint64_t job_mask[3][kJobs];
  __shared__ uint32_t job_base[3][kJobs];
  __shared__ uint32_t row_bits[3][kTiles * K];  // the last frame's non-zero levels of a thread's row, bit i = coefficient i
  __shared__ double rows[3][kTiles * K * (K + 1)];
  const DeltaArgs& a = args.d;
  const Geom& g = a.in.g;
  const uint32_t gi0 = blockIdx.x, tid = threadIdx.x;
  const Group gr = group_of(g, gi0);  // plane 0's group; planes 1 and 2 hold the same tiles
  const uint32_t jobs = gr.nt * kWords, per_plane = g.tiles_y * g.gx;
  const uint32_t t = tid / K, j = tid - t * K;
  const bool active = t < gr.nt;  // (nt <= kTiles) an idle thread stays in every barrier below
  const uint32_t rw = g.w / N * K, rh = g.h / N * K;  // the reduced picture; adjacent lanes hold adjacent pixels
  uint32_t held[3][K];  // the thread's reconstructed levels, as u16
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int q = 0; q < K; ++q) held[c][q] = 0;
  // frame -1 is d_prev: it is added like a key frame and nothing is decoded for it.  Every condition on a frame is the workgroup's.
  for (int32_t i = a.prev.in && a.prev.ws.status[0] == kStOk ? -1 : 0; i < (int32_t)a.n; ++i) {
    const bool seed = i < 0;
    float* dst = seed ? nullptr : args.rec + (((size_t)i * rh + gr.ty * K) * rw + (gr.t0 + t) * K + j) * 3;
    if (!seed && a.status[i] != kStOk) {  // zeros; the frame is not read, and the next frame that passes is a key frame
      if (active) {
#pragma unroll
        for (int y = 0; y < K; ++y) {
          float* p = dst + (size_t)y * rw * 3;
          p[0] = 0.f; p[1] = 0.f; p[2] = 0.f;
        }
      }
      continue;
    }
    const uint8_t* fc = seed ? a.prev.in : a.in.in + a.in.offsets[i];
    const uint8_t* fp = seed || delta_key(a, (uint32_t)i) ? nullptr : delta_before(a, (uint32_t)i);
    const uint32_t* first_level = seed ? a.prev.ws.before : a.in.ws.before + (size_t)i * g.groups;
    if (tid < 64) {  // wave 0: mask 0 past the group's words, no level is read through it
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const uint64_t m = tid < jobs ? load_mask(group_masks(g, fc, c, gr) + 2 * tid) : 0ull;
        const uint32_t ex = wave_exclusive_scan((uint32_t)__popcll(m));
        if (tid < kJobs) { job_mask[c][tid] = m; job_base[c][tid] = ex; }
      }
    }
    bool predicted = false;  // the thread's own tile
    float enc = 0.f, dec = 1.f;
    if (active) {
      const uint32_t* hdr = reinterpret_cast<const uint32_t*>(fc);
      const uint32_t type = tile_type(g, hdr + kHeaderWords, gr, t);
      const uint32_t enc_step = type == 0 ? hdr[kHBgStep] : hdr[kHFgStep];
      predicted = fp && enc_step == tile_step(g, fp, gr, t);
      if (!seed) {
        const bool in_gaze = gazed(args.gaze, (uint32_t)i, gr.x0 + t * N, gr.y0);  // the full-size tile origin: one rule for both decoders
        enc = (float)enc_step;
        dec = in_gaze ? 1.f : (type == 0 ? args.bg : args.fg);
      }
    }
    __syncthreads();
    if (active) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const uint16_t* levels = reinterpret_cast<const uint16_t*>(fc + g.levels_off) + first_level[c * per_plane + gi0];
        float v[K];
#pragma unroll
        for (int q = 0; q < K; ++q) {
          const uint32_t k = j * N + q, w = t * kWords + (k >> 6), b = k & 63u;
          const uint64_t mask = job_mask[c][w], below = (1ull << b) - 1;
          uint32_t lv = predicted ? held[c][q] : 0u;
          if ((mask >> b) & 1u) lv += levels[job_base[c][w] + (uint32_t)__popcll(mask & below)];
          lv &= 0xFFFFu;
          held[c][q] = lv;
          v[q] = (float)(int16_t)lv * enc;
        }
        if (!seed) invert_row_reduced<K>(v, dec, rows[c], t, j);
      }
    }
    __syncthreads();  // (the next frame's words are written behind it; its row passes behind that frame's own first barrier)
    if (seed || !active) continue;
    float out[3][K];
#pragma unroll
    for (int c = 0; c < 3; ++c) invert_column_reduced<N, K>(rows[c], t, j, out[c]);
    store_bgr_column<K>(dst, rw, out);
  }
  if (!args.last || a.status[a.n - 1] != kStOk) return;  // (the whole workgroup)
  if (active) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      uint32_t bits = 0;
#pragma unroll
      for (int q = 0; q < K; ++q) bits |= (held[c][q] != 0 ? 1u : 0u) << q;
      row_bits[c][t * K + j] = bits;
    }
  }
  __syncthreads();  // (also: every wave is past the last frame's gather, the job arrays are free)
  if (tid < 64) {   // wave 0, lane = mask word: the rows of its tile that lie in the word and inside K x K
    const uint32_t wt = tid / kWords, wi = tid - wt * kWords;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      uint64_t m = 0;
      if (tid < jobs) {
#pragma unroll
        for (uint32_t r = 0; r < kRowsPerWord; ++r) {
          const uint32_t row = wi * kRowsPerWord + r;
          if (row < K) m |= (uint64_t)row_bits[c][wt * K + row] << (r * N);
        }
      }
      const uint32_t pc = (uint32_t)__popcll(m), ex = wave_exclusive_scan(pc);
      if (tid < kJobs) { job_mask[c][tid] = m; job_base[c][tid] = ex; }
      if (tid < jobs) store_mask(group_masks(g, args.last, c, gr) + 2 * tid, m);
      const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)(ex + pc), 63);
      if (tid == 0) args.last_cnt[c * per_plane + gi0] = total;
    }
  }
  __syncthreads();
  if (!active) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    uint16_t* run = args.last_runs + (size_t)(c * per_plane + gi0) * args.cap;
#pragma unroll
    for (int q = 0; q < K; ++q) {
      const uint32_t k = j * N + q, w = t * kWords + (k >> 6), b = k & 63u;
      const uint64_t mask = job_mask[c][w], below = (1ull << b) - 1;
      if (held[c][q] != 0) run[job_base[c][w] + (uint32_t)__popcll(mask & below)] = (uint16_t)held[c][q];
    }
  }
}

template <int N, int K>
void launch_decode_delta_reduced(dim3 grid, hipStream_t s, const DecodeDeltaArgs& a) {
  hipLaunchKernelGGL((decode_delta_reduced_kernel<N, K>), grid, dim3(reduced_threads(N, K)), 0, s, a);
}

// the instantiation for a block of 8 or 16 and a reduce of 2, 4 or 8 (both checked by the caller)
void launch_decode_delta_reduced(uint32_t block, uint32_t reduce, dim3 grid, hipStream_t s, const DecodeDeltaArgs& a) {
  if (block == 8) {
    if (reduce == 2) launch_decode_delta_reduced<8, 4>(grid, s, a);
    else if (reduce == 4) launch_decode_delta_reduced<8, 2>(grid, s, a);
    else launch_decode_delta_reduced<8, 1>(grid, s, a);
  } else {
    if (reduce == 2) launch_decode_delta_reduced<16, 8>(grid, s, a);
    else if (reduce == 4) launch_decode_delta_reduced<16, 4>(grid, s, a);
    else launch_decode_delta_reduced<16, 2>(grid, s, a);
  }
}

// ---- decode of a delta stream with temporal layers at reduced size (svc_hip_decode_delta_levels_temporal_reduced_frames;
// include/svc_hip_temporal_decode.h states it) --------------------------------------------------------------------------------------------------
//
// decode_delta_reduced_kernel's workgroup, passes and two barriers per frame, with the temporal undelta's states where that kernel has
// one set of held levels: the thread holds T sets of 3 K levels in registers, set 0 the latest frame of layer 0 and, at period 4 (T = 2),
// set 1 frame 4k + 2.  A frame is rebuilt from the set of its reference (temporal_src_state) and kept in the set of its own layer
// (temporal_dst_state); an odd frame, which no frame refers to, is rebuilt into the temporaries of the row pass alone.  The two sets are
// two named arrays and every index into them is a constant: which one a frame reads and which it writes are conditions on the frame
// number, the same for the whole wave, so each held level costs one v_cndmask to read and one to keep and nothing goes to scratch.  No LDS
// is added to decode_delta_reduced_kernel's.  The tile-predicted predicate reads the reference's header and types as the full-size
// temporal kernel does, and levels outside K x K are never read, so the frames and d_prev may be their band (0, 0, K, K).
//
// d_last is the band (0, 0, K, K) of frame `last_frame` = period * ((n - 1) / period), the frame the next call's frame 0 refers to: set 0
// after the last frame, through decode_delta_reduced_kernel's row_bits -> mask words -> ranked store path and the scan and write kernels,
// which are handed that frame as the call's last.
// (args.rec: [n][h K / N][w K / N][3])
template <int N, int K, int T>
__global__ __launch_bounds__(reduced_threads(N, K)) void decode_delta_temporal_reduced_kernel(DecodeDeltaArgs args, uint32_t last_frame) {
  constexpr uint32_t kTiles = kGroupCoeffs / (N * N), kWords = N * N / 64, kJobs = kTiles * kWords;  // tiles and mask words of a group
  constexpr uint32_t kRowsPerWord = 64 / N;  // coefficient rows of a tile in one mask word
  constexpr uint32_t kPeriod = 1u << T;
  static_assert(T == 1 || T == 2, "period 2 or 4");
  static_assert(kJobs <= 64, "one wave scans a group's mask words");
  __shared__ uint64_t job_mask[3][kJobs];
  __shared__ uint32_t job_base[3][kJobs];
  __shared__ uint32_t row_bits[3][kTiles * K];  // frame last_frame's non-zero levels of a thread's row, bit i = coefficient i
  __shared__ double rows[3][kTiles * K * (K + 1)];
  const DeltaArgs& a = args.d;
  const Geom& g = a.in.g;
  const uint32_t gi0 = blockIdx.x, tid = threadIdx.x;
  const Group gr = group_of(g, gi0);  // plane 0's group; planes 1 and 2 hold the same tiles
  const uint32_t jobs = gr.nt * kWords, per_plane = g.tiles_y * g.gx;
  const uint32_t t = tid / K, j = tid - t * K;
  const bool active = t < gr.nt;  // (nt <= kTiles) an idle thread stays in every barrier below
  const uint32_t rw = g.w / N * K, rh = g.h / N * K;  // the reduced picture; adjacent lanes hold adjacent pixels
  // The thread's levels of layer 0's latest frame, as u16, and (T = 2) of frame 4k + 2.  At K = 8 the second set is packed two levels to
  // a dword: unpacked, the 16 x 16, K = 8, T = 2 instantiation needs 169 VGPRs, one more than three waves per SIMD admit.
  constexpr bool kPacked = K == 8;
  constexpr int kHeld1 = kPacked ? K / 2 : K;
  uint32_t held0[3][K], held1[3][kHeld1];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int q = 0; q < K; ++q) held0[c][q] = 0;
#pragma unroll
    for (int q = 0; q < kHeld1; ++q) held1[c][q] = 0;
  }
  // frame -1 is d_prev, the frame at index -period: it goes into set 0 like a key frame and nothing is decoded for it.  Every condition
  // on a frame is the workgroup's.
  for (int32_t i = a.prev.in && a.prev.ws.status[0] == kStOk ? -1 : 0; i < (int32_t)a.n; ++i) {
    const bool seed = i < 0;
    float* dst = seed ? nullptr : args.rec + (((size_t)i * rh + gr.ty * K) * rw + (gr.t0 + t) * K + j) * 3;
    if (!seed && a.status[i] != kStOk) {  // zeros; the frame is not read, and no frame that passes hangs on it
      if (active) {
#pragma unroll
        for (int y = 0; y < K; ++y) {
          float* p = dst + (size_t)y * rw * 3;
          p[0] = 0.f; p[1] = 0.f; p[2] = 0.f;
        }
      }
      continue;
    }
    const uint8_t* fc = seed ? a.prev.in : a.in.in + a.in.offsets[i];
    const uint8_t* fp = seed || delta_key(a, (uint32_t)i) ? nullptr : delta_before(a, (uint32_t)i, kPeriod);
    const uint32_t from = seed ? 0u : temporal_src_state((uint32_t)i, kPeriod);
    const uint32_t into = seed ? 0u : temporal_dst_state((uint32_t)i, kPeriod, (uint32_t)T);  // T: an odd frame, kept nowhere
    const bool from1 = T == 2 && from == 1u, into0 = into == 0u, into1 = T == 2 && into == 1u;  // (the whole wave)
    const uint32_t* first_level = seed ? a.prev.ws.before : a.in.ws.before + (size_t)i * g.groups;
    if (tid < 64) {  // wave 0: mask 0 past the group's words, no level is read through it
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const uint64_t m = tid < jobs ? load_mask(group_masks(g, fc, c, gr) + 2 * tid) : 0ull;
        const uint32_t ex = wave_exclusive_scan((uint32_t)__popcll(m));
        if (tid < kJobs) { job_mask[c][tid] = m; job_base[c][tid] = ex; }
      }
    }
    bool predicted = false;  // the thread's own tile
    float enc = 0.f, dec = 1.f;
    if (active) {
      const uint32_t* hdr = reinterpret_cast<const uint32_t*>(fc);
      const uint32_t type = tile_type(g, hdr + kHeaderWords, gr, t);
      const uint32_t enc_step = type == 0 ? hdr[kHBgStep] : hdr[kHFgStep];
      predicted = fp && enc_step == tile_step(g, fp, gr, t);
      if (!seed) {
        const bool in_gaze = gazed(args.gaze, (uint32_t)i, gr.x0 + t * N, gr.y0);  // the full-size tile origin: one rule for both decoders
        enc = (float)enc_step;
        dec = in_gaze ? 1.f : (type == 0 ? args.bg : args.fg);
      }
    }
    __syncthreads();
    if (active) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const uint16_t* levels = reinterpret_cast<const uint16_t*>(fc + g.levels_off) + first_level[c * per_plane + gi0];
        float v[K];
#pragma unroll
        for (int q = 0; q < K; ++q) {
          const uint32_t k = j * N + q, w = t * kWords + (k >> 6), b = k & 63u;
          const uint64_t mask = job_mask[c][w], below = (1ull << b) - 1;
          const uint32_t set1 = kPacked ? (held1[c][q / 2] >> (16 * (q & 1))) & 0xFFFFu : held1[c][q % kHeld1];
          uint32_t lv = predicted ? (from1 ? set1 : held0[c][q]) : 0u;
          if ((mask >> b) & 1u) lv += levels[job_base[c][w] + (uint32_t)__popcll(mask & below)];
          lv &= 0xFFFFu;
          if (into0) held0[c][q] = lv;
          if (into1) {
            if (kPacked) held1[c][q / 2] = q & 1 ? (held1[c][q / 2] & 0xFFFFu) | (lv << 16) : (held1[c][q / 2] & 0xFFFF0000u) | lv;
            else held1[c][q % kHeld1] = lv;
          }
          v[q] = (float)(int16_t)lv * enc;
        }
        if (!seed) invert_row_reduced<K>(v, dec, rows[c], t, j);
      }
    }
    __syncthreads();  // (the next frame's words are written behind it; its row passes behind that frame's own first barrier)
    if (seed || !active) continue;
    float out[3][K];
#pragma unroll
    for (int c = 0; c < 3; ++c) invert_column_reduced<N, K>(rows[c], t, j, out[c]);
    store_bgr_column<K>(dst, rw, out);
  }
  if (!args.last || a.status[last_frame] != kStOk) return;  // (the whole workgroup)
  if (active) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      uint32_t bits = 0;
#pragma unroll
      for (int q = 0; q < K; ++q) bits |= (held0[c][q] != 0 ? 1u : 0u) << q;
      row_bits[c][t * K + j] = bits;
    }
  }
  __syncthreads();  // (also: every wave is past the last frame's gather, the job arrays are free)
  if (tid < 64) {   // wave 0, lane = mask word: the rows of its tile that lie in the word and inside K x K
    const uint32_t wt = tid / kWords, wi = tid - wt * kWords;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      uint64_t m = 0;
      if (tid < jobs) {
#pragma unroll
        for (uint32_t r = 0; r < kRowsPerWord; ++r) {
          const uint32_t row = wi * kRowsPerWord + r;
          if (row < K) m |= (uint64_t)row_bits[c][wt * K + row] << (r * N);
        }
      }
      const uint32_t pc = (uint32_t)__popcll(m), ex = wave_exclusive_scan(pc);
      if (tid < kJobs) { job_mask[c][tid] = m; job_base[c][tid] = ex; }
      if (tid < jobs) store_mask(group_masks(g, args.last, c, gr) + 2 * tid, m);
      const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)(ex + pc), 63);
      if (tid == 0) args.last_cnt[c * per_plane + gi0] = total;
    }
  }
  __syncthreads();
  if (!active) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    uint16_t* run = args.last_runs + (size_t)(c * per_plane + gi0) * args.cap;
#pragma unroll
    for (int q = 0; q < K; ++q) {
      const uint32_t k = j * N + q, w = t * kWords + (k >> 6), b = k & 63u;
      const uint64_t mask = job_mask[c][w], below = (1ull << b) - 1;
      if (held0[c][q] != 0) run[job_base[c][w] + (uint32_t)__popcll(mask & below)] = (uint16_t)held0[c][q];
    }
  }
}

template <int N, int K>
void launch_decode_delta_temporal_reduced(uint32_t period, dim3 grid, hipStream_t s, const DecodeDeltaArgs& a, uint32_t last_frame) {
  if (period == 2) hipLaunchKernelGGL((decode_delta_temporal_reduced_kernel<N, K, 1>), grid, dim3(reduced_threads(N, K)), 0, s, a, last_frame);
  else hipLaunchKernelGGL((decode_delta_temporal_reduced_kernel<N, K, 2>), grid, dim3(reduced_threads(N, K)), 0, s, a, last_frame);
}

// the instantiation for a block of 8 or 16, a reduce of 2, 4 or 8 and a period of 2 or 4 (all checked by the caller)
void launch_decode_delta_temporal_reduced(uint32_t block, uint32_t reduce, uint32_t period, dim3 grid, hipStream_t s,
                                          const DecodeDeltaArgs& a, uint32_t last_frame) {
  if (block == 8) {
    if (reduce == 2) launch_decode_delta_temporal_reduced<8, 4>(period, grid, s, a, last_frame);
    else if (reduce == 4) launch_decode_delta_temporal_reduced<8, 2>(period, grid, s, a, last_frame);
    else launch_decode_delta_temporal_reduced<8, 1>(period, grid, s, a, last_frame);
  } else {
    if (reduce == 2) launch_decode_delta_temporal_reduced<16, 8>(period, grid, s, a, last_frame);
    else if (reduce == 4) launch_decode_delta_temporal_reduced<16, 4>(period, grid, s, a, last_frame);
    else launch_decode_delta_temporal_reduced<16, 2>(period, grid, s, a, last_frame);
  }
}

// ---- drain -------------------------------------------------------------------------------------------------------------------

// offsets[n] bytes (a multiple of 16: every frame is padded to 16) from HBM to pinned host memory, 16 B per lane per store
__global__ __launch_bounds__(256) void drain_kernel(const uint4* __restrict__ src, const uint64_t* __restrict__ offsets, uint32_t n,
                                                    uint4* dst, uint64_t capacity) {
  const uint64_t bytes = min(offsets[n], capacity);
  const uint64_t n16 = bytes / 16;
  const uint64_t stride = (uint64_t)gridDim.x * kThreads;
  for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i < n16; i += stride) dst[i] = src[i];
}

// ---- the reference's wire records <-> SVCQ, stream to stream (svc_hip_records_pack_levels_frames, svc_hip_levels_records_frames) --------
//
// A wire frame is one record per tile in tile order, each a u32 type word and 3 x N x N f32 coefficients (wire.hip, records.hip), so
// plane p of a tile is N x N CONTIGUOUS floats at dword 1 + p N N of its record: a 64-coefficient mask word is one coalesced dword load
// (records are only 4-byte aligned: 772 B at 8 x 8) and a __ballot, with no staging of rows.  Both directions keep the pack's and the
// unpack's groups, their order, their counts and their scans, so the bytes are those of the routes through planes.

// the workspace of the pack from records: the pack's own, then per frame the MV blocks' types as the records give them, and per
// (frame, group of plane 0) whether a held record disagrees with its MV block
struct RecordsPackWs {
  Ws pack;
  uint32_t *types, *mismatch;
};
RecordsPackWs records_pack_ws(Carver& c, uint32_t n, uint32_t groups, uint32_t mvb) {
  RecordsPackWs s;
  s.pack = stream_ws(c, n, groups);
  s.types = c.take<uint32_t>((uint64_t)n * mvb);
  s.mismatch = c.take<uint32_t>((uint64_t)n * (groups / 3));
  return s;
}

struct RecordsPackArgs {
  Geom g;
  const uint8_t* records;  // frame f at records + f * stride
  uint64_t stride;
  uint32_t emit_rows, rec_dw;  // tile rows the stream holds; dwords per record
  uint8_t* out;
  uint64_t* offsets;       // [n + 1]
  uint32_t* d_status;      // [n]
  RecordsPackWs ws;
  uint32_t fg, bg;
};

// the type word of the record at the origin of the MV block that holds tile (ty, tx) of a held tile row (the origin's row is then held too)
__device__ __forceinline__ uint32_t origin_type(const RecordsPackArgs& a, const uint32_t* __restrict__ frame_rec, uint32_t ty, uint32_t tx) {
  const Geom& g = a.g;
  const uint32_t oy = (ty * g.bh / g.mvbh) * (g.mvbh / g.bh), ox = (tx * g.bw / g.mvbw) * (g.mvbw / g.bw);
  return frame_rec[((size_t)oy * g.tiles_x + ox) * a.rec_dw];
}

// pack_kernel with the records as its source.  SCATTER = false: the group's non-zero count and inexact count and, from the groups of
// plane 0, the MV blocks' types (the type word of the record at each block's origin; 0 in a tile row the stream does not hold) and
// whether a held record's type word differs from its block's.  SCATTER = true: masks and levels at their final place -- the levels
// compacted in LDS in stream order and stored as one run per wave -- and, from group 0 of each frame, the header, the types, the zero
// pad, offsets[f + 1] and the frame's status.  A tile row the stream does not hold is zero coefficients.
// Dynamic LDS (SCATTER): 2 x cap u16, cap = the group's coefficients, even.
template <bool SCATTER>
__global__ __launch_bounds__(256) void records_pack_kernel(RecordsPackArgs a) {
  extern __shared__ uint16_t lds16[];
  __shared__ uint64_t job_mask[kMaxJobs];
  __shared__ uint32_t job_base[kMaxJobs];
  __shared__ uint32_t red[kThreads / 64];
  __shared__ uint64_t frame_off;
  const Geom& g = a.g;
  const uint32_t gi = blockIdx.x, f = blockIdx.y, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const Group gr = group_of(g, gi);
  const bool held = gr.ty < a.emit_rows;  // the same in every thread
  const uint32_t* frame_rec = reinterpret_cast<const uint32_t*>(a.records + f * a.stride);
  const uint32_t* row_rec = frame_rec + ((size_t)gr.ty * g.tiles_x + gr.t0) * a.rec_dw;  // the group's first record; read only if held
  const uint32_t area = g.bw * g.bh, jobs = gr.nt * g.words, cap = (g.tpg * area + 1) & ~1u;
  uint16_t *raw = lds16, *run = lds16 + cap;
  if (SCATTER) frame_offset_to_lds(a.ws.pack.frame_bytes, f, &frame_off);

  uint32_t nz_count = 0, inexact = 0;
  for (uint32_t j = wave; j < jobs; j += kThreads / 64) {
    const uint32_t t = j / g.words, k = (j - t * g.words) * 64 + lane;
    int32_t lv = 0;
    if (held && k < area) {
      const float step = origin_type(a, frame_rec, gr.ty, gr.t0 + t) == 0 ? (float)a.bg : (float)a.fg;
      const float c = __uint_as_float(row_rec[(size_t)t * a.rec_dw + 1 + gr.plane * area + k]);
      lv = level_of(c, step);
      if (!SCATTER) inexact += c != (float)lv * step;
    }
    if (SCATTER && k < area) raw[t * area + k] = (uint16_t)lv;
    const uint64_t mask = __ballot(lv != 0);
    if (!SCATTER) nz_count += __popcll(mask);
    else if (lane == 0) job_mask[j] = mask;
  }
  if (!SCATTER) {
    inexact = wave_sum(inexact);
    if (lane == 0) red[wave] = inexact;
    __syncthreads();
    if (threadIdx.x == 0) a.ws.pack.inexact[(size_t)f * g.groups + gi] = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    if (lane == 0) red[wave] = nz_count;
    __syncthreads();
    if (threadIdx.x == 0) a.ws.pack.cnt[(size_t)f * g.groups + gi] = red[0] + red[1] + red[2] + red[3];
    if (gr.plane != 0) return;
    // plane 0: thread t looks at the type word of the group's tile t (a group has at most kMaxJobs = kThreads tiles)
    bool differs = false;
    if (threadIdx.x < gr.nt) {
      const uint32_t tx = gr.t0 + threadIdx.x, x = tx * g.bw;
      const uint32_t own = held ? row_rec[(size_t)threadIdx.x * a.rec_dw] : 0u;
      differs = held && own != origin_type(a, frame_rec, gr.ty, tx);
      if (x % g.mvbw == 0 && gr.y0 % g.mvbh == 0) a.ws.types[(size_t)f * g.mvb + (gr.y0 / g.mvbh) * g.mfw + x / g.mvbw] = own;
    }
    const int any = __syncthreads_or(differs);
    if (threadIdx.x == 0) a.ws.mismatch[(size_t)f * (g.groups / 3) + gi] = any != 0;
    return;
  }

  // scatter: exclusive scan of the words' popcounts, in word order; the levels to their ranks in LDS
  __syncthreads();
  uint32_t total;
  const uint32_t pc = threadIdx.x < jobs ? (uint32_t)__popcll(job_mask[threadIdx.x]) : 0u;
  const uint32_t ex = block_exclusive_scan(pc, red, &total);
  if (threadIdx.x < jobs) job_base[threadIdx.x] = ex;
  __syncthreads();
  for (uint32_t j = wave; j < jobs; j += kThreads / 64) {
    const uint64_t mask = job_mask[j];
    if (!((mask >> lane) & 1u)) continue;
    const uint32_t t = j / g.words, k = (j - t * g.words) * 64 + lane;
    run[job_base[j] + lane_rank(mask)] = raw[t * area + k];
  }
  __syncthreads();
  uint8_t* frame = a.out + frame_off;
  uint16_t* levels = reinterpret_cast<uint16_t*>(frame + g.levels_off) + a.ws.pack.cnt[(size_t)f * g.groups + gi];
  uint32_t* masks = group_masks(g, frame, gr.plane, gr);
  for (uint32_t j = threadIdx.x; j < jobs; j += kThreads) {  // two u32 stores: the masks are 4-byte aligned when mvb is odd
    masks[2 * j] = (uint32_t)job_mask[j];
    masks[2 * j + 1] = (uint32_t)(job_mask[j] >> 32);
  }
  // a wave stores a quarter of the group's run, from an even level on
  const uint32_t piece = 2 * div_up(total, 2 * (kThreads / 64)), first = wave * piece;
  if (first < total) store_level_run(run + first, min(piece, total - first), levels + first);
  if (gi != 0) return;
  // group 0: header, types, pad, offsets, status
  const uint32_t* types = a.ws.types + (size_t)f * g.mvb;
  write_frame_edges(frame, head_of(g, a.fg, a.bg, a.ws.pack.frame_levels[f], a.ws.pack.frame_inexact[f], a.ws.pack.frame_bytes[f]), types, g.mvb,
                    g.levels_off, kThreads, a.offsets, f, frame_off);
  bool differs = false;
  for (uint32_t i = threadIdx.x; i < g.groups / 3; i += kThreads) differs |= a.ws.mismatch[(size_t)f * (g.groups / 3) + i] != 0;
  const int any = __syncthreads_or(differs);
  if (threadIdx.x == 0) a.d_status[f] = any ? kStGeometry : kStOk;
}

struct LevelsRecordsArgs {
  UnpackArgs u;      // planes and types are null: none are written
  uint8_t* records;  // frame f at records + f * stride
  uint64_t stride;
  uint32_t rec_dw;   // dwords per record
};

// After the unpack's count and scan.  Grid (groups of plane 0 in the tile rows the stream holds, frames): a workgroup writes the whole
// records of its group's tiles -- the type word (the MV block's id) from thread t for tile t, then plane by plane the unpack's scatter
// with the record as its destination: a wave per mask word, 64 adjacent dwords per store.  A frame that failed its checks is zeros.
__global__ __launch_bounds__(256) void levels_records_kernel(LevelsRecordsArgs a) {
  __shared__ uint32_t red[kThreads / 64];
  __shared__ uint32_t job_base[kMaxJobs];
  __shared__ uint64_t job_mask[kMaxJobs];
  const Geom& g = a.u.g;
  const uint32_t gi0 = blockIdx.x, f = blockIdx.y, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const Group gr = group_of(g, gi0);  // plane 0's group; planes 1 and 2 hold the same tiles
  const uint32_t st = a.u.ws.status[f];
  const uint8_t* frame = a.u.in + (st == kStOk ? a.u.offsets[f] : 0);  // dereferenced only for a frame that passed its checks
  const uint32_t* hdr = reinterpret_cast<const uint32_t*>(frame);
  const uint32_t* types = reinterpret_cast<const uint32_t*>(frame + kHeaderBytes);
  const float fg = st == kStOk ? (float)hdr[kHFgStep] : 0.f, bg = st == kStOk ? (float)hdr[kHBgStep] : 0.f;
  uint32_t* out = reinterpret_cast<uint32_t*>(a.records + f * a.stride) + ((size_t)gr.ty * g.tiles_x + gr.t0) * a.rec_dw;
  const uint32_t area = g.bw * g.bh, jobs = gr.nt * g.words, per_plane = g.tiles_y * g.gx;
  if (tid < gr.nt) out[(size_t)tid * a.rec_dw] = st == kStOk ? tile_type(g, types, gr, tid) : 0u;
  for (uint32_t c = 0; c < 3; ++c) {
    const uint32_t* masks = st != kStOk ? nullptr : group_masks(g, frame, c, gr);
    const uint64_t m = (masks && tid < jobs) ? load_mask(masks + 2 * tid) : 0ull;
    uint32_t total;
    const uint32_t ex = block_exclusive_scan((uint32_t)__popcll(m), red, &total);
    if (tid < jobs) { job_mask[tid] = m; job_base[tid] = ex; }
    __syncthreads();
    const int16_t* levels = reinterpret_cast<const int16_t*>(frame + g.levels_off) +
                            (st == kStOk ? a.u.ws.cnt[(size_t)f * g.groups + c * per_plane + gi0] : 0u);
    for (uint32_t jj = wave; jj < jobs; jj += kThreads / 64) {
      const uint64_t mask = job_mask[jj];
      const uint32_t t = jj / g.words, k = (jj - t * g.words) * 64 + lane;
      if (k >= area) continue;
      float v = 0.f;
      if ((mask >> lane) & 1u) {
        const float step = tile_type(g, types, gr, t) == 0 ? bg : fg;
        v = (float)levels[job_base[jj] + lane_rank(mask)] * step;
      }
      out[(size_t)t * a.rec_dw + 1 + c * area + k] = __float_as_uint(v);
    }
    __syncthreads();  // the next plane reuses the job arrays
  }
}

// ---- the entry points' checks and launch sequences -----------------------------------------------------------------------------------

// the limits with SVCQ's worst case
int validate_limits(const char* what, uint32_t n, uint32_t w, uint32_t h, uint32_t bw, uint32_t bh, uint32_t mvbw, uint32_t mvbh) {
  return svc::validate_limits(what, n, w, h, bw, bh, frame_layout(w, h, bw, bh, mvbw, mvbh).max_bytes);
}

// What the two decodes at reduced size check first, in this order: geometry, steps, reduce, the display size against the reduced picture,
// limits.
int validate_reduced(const char* what, uint32_t n, uint32_t w, uint32_t h, uint32_t bw, uint32_t bh, uint32_t mvbw, uint32_t mvbh, uint32_t fg,
                     uint32_t bg, uint32_t reduce, uint32_t display_w, uint32_t display_h) {
  const int rc = validate_decode_geom(what, w, h, bw, bh, mvbw, mvbh);
  if (rc) return rc;
  SVC_REQUIRE(fg > 0 && bg > 0, "%s: quant steps must be positive (libs/decoder.cpp:35-47)", what);
  SVC_REQUIRE(reduce == 2 || reduce == 4 || reduce == 8, "%s: reduce %u (supported: 2, 4, 8)", what, reduce);
  SVC_REQUIRE((display_w == 0 && display_h == 0) || (display_w >= 1 && display_w <= w / reduce && display_h >= 1 && display_h <= h / reduce),
              "%s: display %ux%u must lie within 1x1 .. %ux%u (the padded frame over reduce)", what, display_w, display_h, w / reduce, h / reduce);
  return validate_limits(what, n, w, h, bw, bh, mvbw, mvbh);
}

// the pack's launches, with a.fg / a.bg or the budgeted pack's per-frame steps
int enqueue_pack(const char* what, const PackArgs& a, hipStream_t s) {
  const Geom& g = a.g;
  const dim3 grid(g.groups, a.n);
  int rc;
  hipLaunchKernelGGL(pack_kernel<false>, grid, dim3(kThreads), lds_bytes(g), s, a);
  if ((rc = check_launch(what, "count"))) return rc;
  hipLaunchKernelGGL(scan_kernel<false>, dim3(a.n), dim3(kThreads), 0, s, g, a.ws, nullptr, 0, nullptr, nullptr);
  if ((rc = check_launch(what, "scan"))) return rc;
  hipLaunchKernelGGL(pack_kernel<true>, grid, dim3(kThreads), lds_bytes(g), s, a);
  return check_launch(what, "scatter");
}

// what the unpack and the decode begin with: the groups' level counts, then their prefixes and every frame's status
int enqueue_unpack_scan(const char* what, const UnpackArgs& u, uint32_t n, uint32_t* d_status, hipStream_t s) {
  hipLaunchKernelGGL(unpack_kernel<false>, dim3(u.g.groups, n), dim3(kThreads), 0, s, u);
  const int rc = check_launch(what, "count");
  if (rc) return rc;
  hipLaunchKernelGGL(scan_kernel<true>, dim3(n), dim3(kThreads), 0, s, u.g, u.ws, u.in, u.stream_bytes, u.offsets, d_status);
  return check_launch(what, "scan");
}


// ---- the split's checks after its steps, and its launches

// a base step pair against the fine step: multiples of it, and ratios whose residuals fit int16
int validate_split_steps(const char* what, uint32_t fine_step, uint32_t fg_step, uint32_t bg_step) {
  SVC_REQUIRE(fg_step % fine_step == 0 && bg_step % fine_step == 0, "%s: the base steps (%u, %u) must be multiples of fine_step %u", what,
              fg_step, bg_step, fine_step);
  if (std::max(fg_step, bg_step) / fine_step > 32766)
    return fail(SVC_ERR_UNSUPPORTED, "%s: residuals of base step %u over fine_step %u could exceed int16", what, std::max(fg_step, bg_step),
                fine_step);
  return SVC_OK;
}

// Both calls after their steps or ladder, in the order of the SVCQ entry points: limits, the d_src rule, workspace, capacities;
// n_out == 0 returns SVC_OK; then pointers; then the launches.  ladder null: the fixed call with a.fg / a.bg.
int split_levels(const char* what, SplitArgs a, const svc_step_pair* ladder, uint32_t ladder_len, const uint32_t* d_budget,
                 uint32_t* d_choice, uint8_t* d_workspace, uint64_t workspace_bytes, uint64_t base_capacity, uint64_t enh_capacity,
                 void* stream) {
  const Geom& g = a.g;
  int rc = validate_limits(what, std::max(a.n_out, a.n_in), g.w, g.h, g.bw, g.bh, g.mvbw, g.mvbh);
  if (rc) return rc;
  SVC_REQUIRE(a.src || a.n_out == a.n_in, "%s: without d_src output frame i is input frame i, but n_out is %u and n_in %u", what, a.n_out,
              a.n_in);
  a.g = make_geom(g.w, g.h, g.bw, g.bh, g.mvbw, g.mvbh);
  const uint32_t len = ladder ? ladder_len : 0;
  if ((rc = require_workspace(what, workspace_bytes, layout_bytes(split_ws, a.n_out, g.groups, len)))) return rc;
  const uint64_t max_bytes = frame_layout(g.w, g.h, g.bw, g.bh, g.mvbw, g.mvbh).max_bytes;
  if ((rc = require_capacity(what, "base output", base_capacity, a.n_out * max_bytes))) return rc;
  if (a.enh && (rc = require_capacity(what, "enhancement output", enh_capacity, a.n_out * max_bytes))) return rc;
  if (a.n_out == 0) return SVC_OK;
  SVC_REQUIRE(a.in && a.offsets && d_workspace && a.base && a.base_offsets && a.d_status && (!a.enh || a.enh_offsets) &&
                  (!ladder || (d_budget && d_choice)),
              "%s: null pointer", what);
  SVC_REQUIRE(aligned(a.in, 16) && aligned(a.base, 16) && aligned(a.enh, 16) && aligned(d_workspace, 16) && aligned(a.offsets, 8) &&
                  aligned(a.base_offsets, 8) && aligned(a.enh_offsets, 8) && aligned(a.src, 4) && aligned(a.window, 4) &&
                  aligned(a.d_status, 4) && aligned(d_budget, 4) && aligned(d_choice, 4),
              "%s: streams and workspace must be 16-byte aligned, offsets 8-byte, source indices, windows, budget, choice and status 4-byte",
              what);
  a.ws = carve(d_workspace, split_ws, a.n_out, g.groups, len);
  if (!a.enh) a.enh_offsets = nullptr, a.window = nullptr;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 waves(div_up(g.groups, kThreads / 64), a.n_out);
  // the input pass: the window call's count and scan with every tile kept
  const WindowArgs in{g, a.in, a.stream_bytes, a.offsets, a.n_in, a.src, nullptr, nullptr, nullptr, a.d_status, a.ws.in};
  hipLaunchKernelGGL(window_count_kernel, waves, dim3(kThreads), 0, s, in);
  if ((rc = check_launch(what, "input count"))) return rc;
  hipLaunchKernelGGL(window_scan_kernel, dim3(a.n_out), dim3(kThreads), 0, s, in);
  if ((rc = check_launch(what, "input scan"))) return rc;
  if (ladder) {
    const Ladder lad = make_ladder(ladder, ladder_len);
    hipLaunchKernelGGL(split_budget_count_kernel, waves, dim3(kThreads), 0, s, a, lad);
    if ((rc = check_launch(what, "count per entry"))) return rc;
    hipLaunchKernelGGL(split_select_kernel, dim3(a.n_out), dim3(kThreads), 0, s, a, lad, d_budget, d_choice);
    if ((rc = check_launch(what, "select"))) return rc;
    a.steps = a.ws.steps;
  }
  hipLaunchKernelGGL(split_count_kernel, waves, dim3(kThreads), 0, s, a);
  if ((rc = check_launch(what, "count"))) return rc;
  hipLaunchKernelGGL(split_scan_kernel, dim3(a.n_out), dim3(kThreads), 0, s, a);
  if ((rc = check_launch(what, "scan"))) return rc;
  if ((rc = enqueue_frame_offsets(what, a.enh ? 2 : 1, OffsetsJob{a.ws.frame_bytes, a.base_offsets, nullptr},
                                  OffsetsJob{a.ws.frame_bytes + a.n_out, a.enh_offsets, nullptr}, a.n_out, stream)))
    return rc;
  // a wave stages its group's levels of both layers in LDS: two waves per workgroup where a group is a tile above 2048 coefficients
  const uint32_t cap = g.tpg * g.bw * g.bh, wpb = split_write_waves(cap);
  hipLaunchKernelGGL(split_write_kernel, dim3(div_up(g.groups, wpb), a.n_out), dim3(64 * wpb), split_write_lds(cap), s, a, cap);
  return check_launch(what, "write");
}

// What the delta call, the undelta call and the decode of a delta stream begin with: the input pass of the stream and of the frame before
// it -- the window call's count and scan with every tile kept (d_status holds the frames' own codes until the status kernel writes the
// final ones) -- then the status kernel, chained for the two calls whose predecessor is a reconstructed frame.  Six launches, three
// without d_prev.
int enqueue_delta_input(const char* what, const DeltaArgs& a, bool chain, uint64_t prev_bytes, hipStream_t s, uint32_t period = 1) {
  int rc;
  const uint32_t wave_blocks = div_up(a.in.g.groups, kThreads / 64);
  if (a.prev.in) {
    hipLaunchKernelGGL(delta_prev_kernel, dim3(1), dim3(1), 0, s, const_cast<uint64_t*>(a.prev.offsets), prev_bytes);
    if ((rc = check_launch(what, "offsets of the frame before"))) return rc;
  }
  for (const WindowArgs* in : {&a.prev, &a.in}) {
    if (!in->in) continue;
    hipLaunchKernelGGL(window_count_kernel, dim3(wave_blocks, in->n_in), dim3(kThreads), 0, s, *in);
    if ((rc = check_launch(what, in == &a.in ? "input count" : "input count of the frame before"))) return rc;
    hipLaunchKernelGGL(window_scan_kernel, dim3(in->n_in), dim3(kThreads), 0, s, *in);
    if ((rc = check_launch(what, "input scan"))) return rc;
  }
  if (period != 1) {  // the temporal calls: a tree of statuses, not a chain
    if (chain) hipLaunchKernelGGL(delta_temporal_status_kernel<true>, dim3(1), dim3(64), 0, s, a, period);
    else hipLaunchKernelGGL(delta_temporal_status_kernel<false>, dim3(1), dim3(64), 0, s, a, period);
  } else if (chain) {
    hipLaunchKernelGGL(delta_status_kernel<true>, dim3(1), dim3(64), 0, s, a);
  } else {
    hipLaunchKernelGGL(delta_status_kernel<false>, dim3(1), dim3(64), 0, s, a);
  }
  return check_launch(what, "status");
}

// the period of the temporal calls, checked right after the geometry
int validate_period(const char* what, uint32_t period) {
  SVC_REQUIRE(period == 1 || period == 2 || period == 4, "%s: period %u (supported: 1, 2, 4)", what, period);
  return SVC_OK;
}

// Both directions of the delta, checked in the window call's order: geometry, limits, workspace, output capacity; n_frames == 0 then
// returns SVC_OK; then pointers.  Ten launches, whatever n_frames (seven without d_prev).  period 1: the plain calls; 2 or 4: the temporal
// calls, which differ in the status kernel and in the count and write kernels alone.
int delta_levels(const char* what, bool undo, uint32_t period, const uint8_t* d_frames, uint64_t stream_bytes, const uint64_t* d_frame_offsets, uint32_t n,
                 const uint8_t* d_prev, uint64_t prev_bytes, const uint32_t* d_key, uint32_t w, uint32_t h, uint32_t bw, uint32_t bh,
                 uint32_t mvbw, uint32_t mvbh, uint8_t* d_workspace, uint64_t workspace_bytes, uint8_t* d_out, uint64_t out_capacity,
                 uint64_t* d_out_offsets, uint32_t* d_status, void* stream) {
  int rc = validate_geom(what, w, h, bw, bh, mvbw, mvbh);
  if (!rc) rc = validate_period(what, period);
  if (!rc) rc = validate_limits(what, n, w, h, bw, bh, mvbw, mvbh);
  if (rc) return rc;
  const Geom g = make_geom(w, h, bw, bh, mvbw, mvbh);
  if ((rc = require_workspace(what, workspace_bytes, layout_bytes(delta_ws, n, g.groups)))) return rc;
  const uint64_t max_bytes = frame_layout(w, h, bw, bh, mvbw, mvbh).max_bytes;
  if ((rc = require_capacity(what, "output", out_capacity, n * max_bytes))) return rc;
  if (n == 0) return SVC_OK;
  SVC_REQUIRE(d_frames && d_frame_offsets && d_workspace && d_out && d_out_offsets && d_status, "%s: null pointer", what);
  SVC_REQUIRE(aligned(d_frames, 16) && aligned(d_prev, 16) && aligned(d_out, 16) && aligned(d_workspace, 16) && aligned(d_frame_offsets, 8) &&
                  aligned(d_out_offsets, 8) && aligned(d_key, 4) && aligned(d_status, 4),
              "%s: streams, the frame before and workspace must be 16-byte aligned, offsets 8-byte, key flags and status 4-byte", what);
  const DeltaWs ws = carve(d_workspace, delta_ws, n, g.groups);
  const DeltaArgs a{{g, d_frames, stream_bytes, d_frame_offsets, n, nullptr, nullptr, d_out, d_out_offsets, d_status, ws.in},
                    {g, d_prev, prev_bytes, ws.prev_offsets, 1, nullptr, nullptr, nullptr, nullptr, ws.prev_code, ws.prev},
                    d_key, n, ws.cnt, ws.frame_bytes, ws.frame_levels, ws.status};
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint32_t wave_blocks = div_up(g.groups, kThreads / 64);
  if ((rc = enqueue_delta_input(what, a, undo, prev_bytes, s, period))) return rc;
  // the scan of the band call on this call's counts and final statuses
  WindowArgs counted = a.in;
  counted.ws.status = ws.status;
  const BandArgs scan{counted, nullptr, ws.cnt, ws.frame_bytes, ws.frame_levels};
  const uint32_t cap = g.tpg * g.bw * g.bh, wpb = split_write_waves(cap);
  const dim3 chains(div_up(g.groups, wpb)), pairs(wave_blocks, n);
  const uint32_t twpb = temporal_waves(cap);
  const dim3 trees(div_up(g.groups, twpb));
  if (period != 1 && undo) hipLaunchKernelGGL(undelta_temporal_kernel<false>, trees, dim3(64 * twpb), temporal_lds(cap), s, a, cap, period);
  else if (period != 1) hipLaunchKernelGGL(delta_temporal_kernel<false>, pairs, dim3(kThreads), 0, s, a, cap, period);
  else if (undo) hipLaunchKernelGGL(undelta_kernel<false>, chains, dim3(64 * wpb), split_write_lds(cap), s, a, cap);
  else hipLaunchKernelGGL(delta_kernel<false>, pairs, dim3(kThreads), 0, s, a, cap);
  if ((rc = check_launch(what, "count"))) return rc;
  hipLaunchKernelGGL(band_scan_kernel, dim3(n), dim3(kThreads), 0, s, scan);
  if ((rc = check_launch(what, "scan"))) return rc;
  if ((rc = enqueue_frame_offsets(what, 1, OffsetsJob{ws.frame_bytes, d_out_offsets, nullptr}, OffsetsJob{}, n, stream))) return rc;
  if (period != 1 && undo) hipLaunchKernelGGL(undelta_temporal_kernel<true>, trees, dim3(64 * twpb), temporal_lds(cap), s, a, cap, period);
  else if (period != 1) hipLaunchKernelGGL(delta_temporal_kernel<true>, pairs, dim3(kThreads), select_write_lds(cap), s, a, cap, period);
  else if (undo) hipLaunchKernelGGL(undelta_kernel<true>, chains, dim3(64 * wpb), split_write_lds(cap), s, a, cap);
  else hipLaunchKernelGGL(delta_kernel<true>, pairs, dim3(kThreads), select_write_lds(cap), s, a, cap);
  return check_launch(what, "write");
}

SplitArgs split_args(const uint8_t* d_frames, uint64_t stream_bytes, const uint64_t* d_frame_offsets, uint32_t n_in, const uint32_t* d_src,
                     uint32_t n_out, uint32_t w, uint32_t h, uint32_t bw, uint32_t bh, uint32_t mvbw, uint32_t mvbh, uint32_t fine_step,
                     const uint32_t* d_window, uint8_t* d_base_out, uint64_t* d_base_offsets, uint8_t* d_enh_out, uint64_t* d_enh_offsets,
                     uint32_t* d_status) {
  SplitArgs a{};
  a.g.w = w; a.g.h = h; a.g.bw = bw; a.g.bh = bh; a.g.mvbw = mvbw; a.g.mvbh = mvbh;  // the rest of g once the limits have passed
  a.in = d_frames; a.stream_bytes = stream_bytes; a.offsets = d_frame_offsets; a.n_in = n_in; a.src = d_src; a.window = d_window;
  a.n_out = n_out; a.e = fine_step;
  a.base = d_base_out; a.enh = d_enh_out; a.base_offsets = d_base_offsets; a.enh_offsets = d_enh_offsets; a.d_status = d_status;
  return a;
}

}  // namespace

int enqueue_frame_offsets(const char* what, uint32_t jobs, OffsetsJob job0, OffsetsJob job1, uint32_t n, void* stream) {
  hipLaunchKernelGGL(frame_offsets_kernel, dim3(jobs), dim3(kThreads), 0, static_cast<hipStream_t>(stream), job0, job1, n);
  return check_launch(what, "offsets");
}

int drain_to_host(const char* what, const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, void* host_dst,
                  uint64_t capacity, uint64_t need, void* stream) {
  const int rc = require_capacity(what, "destination", capacity, need);
  if (rc || n_frames == 0) return rc;
  SVC_REQUIRE(d_frames && d_frame_offsets && host_dst, "%s: null pointer", what);
  SVC_REQUIRE(aligned(d_frames, 16) && aligned(host_dst, 16) && aligned(d_frame_offsets, 8),
              "%s: frames and destination must be 16-byte aligned, offsets 8-byte", what);
  // A kernel that stores to pageable memory faults the GPU: the destination must be pinned / registered host memory, and the
  // WHOLE of [host_dst, host_dst + capacity) must lie inside that one allocation (not run on into a neighbour or a gap).
  hipPointerAttribute_t attr{};
  if (hipPointerGetAttributes(&attr, host_dst) != hipSuccess || attr.type != hipMemoryTypeHost) {
    (void)hipGetLastError();
    return fail(SVC_ERR_INVALID_ARG, "%s: the destination is not pinned or registered host memory", what);
  }
  hipDeviceptr_t start = nullptr;
  size_t size = 0;
  if (hipPointerGetAttribute(&start, HIP_POINTER_ATTRIBUTE_RANGE_START_ADDR, host_dst) != hipSuccess ||
      hipPointerGetAttribute(&size, HIP_POINTER_ATTRIBUTE_RANGE_SIZE, host_dst) != hipSuccess) {
    (void)hipGetLastError();
    return fail(SVC_ERR_INVALID_ARG, "%s: the destination's allocation cannot be resolved", what);
  }
  const uintptr_t lo = reinterpret_cast<uintptr_t>(start), dst = reinterpret_cast<uintptr_t>(host_dst);
  if (dst < lo || dst - lo > size || capacity > size - (dst - lo))
    return fail(SVC_ERR_INVALID_ARG, "%s: %llu B from the destination run past its pinned allocation (%llu B from %p)", what,
                (unsigned long long)capacity, (unsigned long long)size, reinterpret_cast<void*>(lo));
  void* d_dst = nullptr;
  if (hipHostGetDevicePointer(&d_dst, host_dst, 0) != hipSuccess || !d_dst) {
    (void)hipGetLastError();
    return fail(SVC_ERR_INVALID_ARG, "%s: the destination has no device mapping", what);
  }
  SVC_REQUIRE(aligned(d_dst, 16), "%s: the destination's device mapping is not 16-byte aligned", what);
  hipLaunchKernelGGL(drain_kernel, dim3(64), dim3(kThreads), 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const uint4*>(d_frames), d_frame_offsets, n_frames, static_cast<uint4*>(d_dst), capacity);
  return check_launch(what);
}

}  // namespace svc

using namespace svc;

extern "C" {

uint64_t svc_hip_levels_max_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h, uint32_t block_w, uint32_t block_h,
                                  uint32_t mv_block_w, uint32_t mv_block_h) {
  if (validate_geom("levels_max_bytes", frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h) ||
      validate_limits("levels_max_bytes", n_frames, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h))
    return 0;
  return n_frames * frame_layout(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h).max_bytes;
}

uint64_t svc_hip_pack_levels_workspace_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h, uint32_t block_w,
                                             uint32_t block_h) {
  // the MV block does not enter the group split: the whole frame stands in for it
  if (validate_geom("pack_levels_workspace_bytes", frame_w, frame_h, block_w, block_h, frame_w, frame_h) ||
      validate_limits("pack_levels_workspace_bytes", n_frames, frame_w, frame_h, block_w, block_h, frame_w, frame_h))
    return 0;
  return layout_bytes(stream_ws, n_frames, make_geom(frame_w, frame_h, block_w, block_h, frame_w, frame_h).groups);
}

// Every argument is checked in this order, whatever n_frames: geometry, steps, limits, sizes, then pointers (null, alignment,
// and for the drain what memory the destination is).  n_frames == 0 returns SVC_OK after the checks that need no pointer.
int svc_hip_pack_levels_frames(const float* d_planes, const uint32_t* d_block_types, uint32_t n_frames, uint32_t frame_w,
                               uint32_t frame_h, uint32_t block_w, uint32_t block_h, uint32_t mv_block_w, uint32_t mv_block_h,
                               uint32_t fg_step, uint32_t bg_step, uint8_t* d_workspace, uint64_t workspace_bytes, uint8_t* d_out,
                               uint64_t out_capacity, uint64_t* d_frame_offsets, void* stream) {
  int rc = validate_geom("pack_levels", frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if (rc) return rc;
  SVC_REQUIRE(fg_step > 0 && bg_step > 0, "pack_levels: quant steps must be positive");
  // Parseval: no coefficient of an orthonormal DCT of u8 samples exceeds 255 * sqrt(tile area) in magnitude
  if (255.0 * std::sqrt((double)block_w * block_h) / std::min(fg_step, bg_step) > 32767.0)
    return fail(SVC_ERR_UNSUPPORTED, "pack_levels: levels of a %ux%u tile at step %u could exceed int16", block_w, block_h,
                std::min(fg_step, bg_step));
  if ((rc = validate_limits("pack_levels", n_frames, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h))) return rc;
  const Geom g = make_geom(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if ((rc = require_workspace("pack_levels", workspace_bytes, layout_bytes(stream_ws, n_frames, g.groups)))) return rc;
  const uint64_t need = n_frames * frame_layout(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h).max_bytes;
  if ((rc = require_capacity("pack_levels", "output", out_capacity, need))) return rc;
  if (n_frames == 0) return SVC_OK;  // empty batch: nothing to enqueue
  SVC_REQUIRE(d_planes && d_block_types && d_workspace && d_out && d_frame_offsets, "pack_levels: null pointer");
  SVC_REQUIRE(aligned(d_planes, 16) && aligned(d_out, 16) && aligned(d_workspace, 16) && aligned(d_frame_offsets, 8) &&
                  aligned(d_block_types, 4),
              "pack_levels: planes, output and workspace must be 16-byte aligned, offsets 8-byte");
  const PackArgs a{g, d_planes, d_block_types, d_out, d_frame_offsets, carve(d_workspace, stream_ws, n_frames, g.groups), n_frames, fg_step,
                   bg_step, nullptr};
  return enqueue_pack("pack_levels", a, static_cast<hipStream_t>(stream));
}

uint64_t svc_hip_pack_levels_budget_workspace_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h, uint32_t block_w,
                                                    uint32_t block_h, uint32_t ladder_len) {
  if (validate_geom("pack_levels_budget_workspace_bytes", frame_w, frame_h, block_w, block_h, frame_w, frame_h) ||
      validate_limits("pack_levels_budget_workspace_bytes", n_frames, frame_w, frame_h, block_w, block_h, frame_w, frame_h))
    return 0;
  if (ladder_len == 0 || ladder_len > kMaxLadder) {
    (void)fail(SVC_ERR_INVALID_ARG, "pack_levels_budget_workspace_bytes: a ladder of %u entries (1 .. %u)", ladder_len, kMaxLadder);
    return 0;
  }
  return layout_bytes(budget_ws, n_frames, make_geom(frame_w, frame_h, block_w, block_h, frame_w, frame_h).groups, ladder_len);
}

// Checked in the order of svc_hip_pack_levels_frames, the ladder in place of the steps: geometry, ladder, int16 bound on entry 0,
// limits, sizes, then pointers; n_frames == 0 returns SVC_OK after the checks that need no device pointer.
int svc_hip_pack_levels_budget_frames(const float* d_planes, const uint32_t* d_block_types, uint32_t n_frames, uint32_t frame_w,
                                      uint32_t frame_h, uint32_t block_w, uint32_t block_h, uint32_t mv_block_w, uint32_t mv_block_h,
                                      const svc_step_pair* ladder, uint32_t ladder_len, const uint32_t* d_budget, uint8_t* d_workspace,
                                      uint64_t workspace_bytes, uint8_t* d_out, uint64_t out_capacity, uint64_t* d_frame_offsets,
                                      uint32_t* d_choice, void* stream) {
  int rc = validate_geom("pack_levels_budget", frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if (rc) return rc;
  if ((rc = validate_ladder("pack_levels_budget", ladder, ladder_len))) return rc;
  // entry 0 holds the smallest steps: the bound of svc_hip_pack_levels_frames there covers the whole ladder
  const uint32_t smin = std::min(ladder[0].fg_step, ladder[0].bg_step);
  if (255.0 * std::sqrt((double)block_w * block_h) / smin > 32767.0)
    return fail(SVC_ERR_UNSUPPORTED, "pack_levels_budget: levels of a %ux%u tile at step %u could exceed int16", block_w, block_h, smin);
  if ((rc = validate_limits("pack_levels_budget", n_frames, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h))) return rc;
  const Geom g = make_geom(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if ((rc = require_workspace("pack_levels_budget", workspace_bytes, layout_bytes(budget_ws, n_frames, g.groups, ladder_len)))) return rc;
  const uint64_t need = n_frames * frame_layout(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h).max_bytes;
  if ((rc = require_capacity("pack_levels_budget", "output", out_capacity, need))) return rc;
  if (n_frames == 0) return SVC_OK;
  SVC_REQUIRE(d_planes && d_block_types && d_budget && d_workspace && d_out && d_frame_offsets && d_choice, "pack_levels_budget: null pointer");
  SVC_REQUIRE(aligned(d_planes, 16) && aligned(d_out, 16) && aligned(d_workspace, 16) && aligned(d_frame_offsets, 8) &&
                  aligned(d_block_types, 4) && aligned(d_budget, 4) && aligned(d_choice, 4),
              "pack_levels_budget: planes, output and workspace must be 16-byte aligned, offsets 8-byte, types, budget and choice 4-byte");
  const Ladder lad = make_ladder(ladder, ladder_len);
  const BudgetWs bws = carve(d_workspace, budget_ws, n_frames, g.groups, ladder_len);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(g.groups, n_frames);
  hipLaunchKernelGGL(budget_count_kernel, grid, dim3(kThreads), lds_bytes(g), s, g, d_planes, d_block_types, lad, bws.nz);
  if ((rc = check_launch("pack_levels_budget count per entry"))) return rc;
  hipLaunchKernelGGL(budget_sum_kernel, dim3(ladder_len, n_frames), dim3(kThreads), 0, s, g, ladder_len, bws.nz, bws.bytes);
  if ((rc = check_launch("pack_levels_budget sum"))) return rc;
  hipLaunchKernelGGL(budget_select_kernel, dim3(div_up(n_frames, kThreads)), dim3(kThreads), 0, s, n_frames, lad, bws.bytes, d_budget,
                     bws.steps, d_choice);
  if ((rc = check_launch("pack_levels_budget select"))) return rc;
  const PackArgs a{g, d_planes, d_block_types, d_out, d_frame_offsets, bws.pack, n_frames, 0, 0, bws.steps};
  return enqueue_pack("pack_levels_budget", a, s);
}

int svc_hip_unpack_levels_frames(const uint8_t* d_frames, uint64_t stream_bytes, const uint64_t* d_frame_offsets, uint32_t n_frames,
                                 uint32_t frame_w, uint32_t frame_h, uint32_t block_w, uint32_t block_h, uint32_t mv_block_w,
                                 uint32_t mv_block_h, uint8_t* d_workspace, uint64_t workspace_bytes, float* d_planes,
                                 uint32_t* d_block_types, uint32_t* d_status, void* stream) {
  int rc = validate_geom("unpack_levels", frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if (!rc) rc = validate_limits("unpack_levels", n_frames, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if (rc) return rc;
  const Geom g = make_geom(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if ((rc = require_workspace("unpack_levels", workspace_bytes, layout_bytes(stream_ws, n_frames, g.groups)))) return rc;
  if (n_frames == 0) return SVC_OK;
  SVC_REQUIRE(d_frames && d_frame_offsets && d_workspace && d_planes && d_block_types && d_status, "unpack_levels: null pointer");
  SVC_REQUIRE(aligned(d_frames, 16) && aligned(d_planes, 16) && aligned(d_workspace, 16) && aligned(d_frame_offsets, 8) &&
                  aligned(d_block_types, 4) && aligned(d_status, 4),
              "unpack_levels: frames, planes and workspace must be 16-byte aligned, offsets 8-byte");
  const UnpackArgs a{g, d_frames, stream_bytes, d_frame_offsets, d_planes, d_block_types, carve(d_workspace, stream_ws, n_frames, g.groups)};
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((rc = enqueue_unpack_scan("unpack_levels", a, n_frames, d_status, s))) return rc;
  hipLaunchKernelGGL(unpack_kernel<true>, dim3(g.groups, n_frames), dim3(kThreads), lds_bytes(g), s, a);
  return check_launch("unpack_levels scatter");
}

int svc_hip_levels_drain(const uint8_t* d_frames, const uint64_t* d_frame_offsets, uint32_t n_frames, uint32_t frame_w,
                         uint32_t frame_h, uint32_t block_w, uint32_t block_h, uint32_t mv_block_w, uint32_t mv_block_h,
                         void* host_dst, uint64_t capacity, void* stream) {
  int rc = validate_geom("levels_drain", frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if (!rc) rc = validate_limits("levels_drain", n_frames, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if (rc) return rc;
  return drain_to_host("levels_drain", d_frames, d_frame_offsets, n_frames, host_dst, capacity,
                       n_frames * frame_layout(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h).max_bytes, stream);
}

uint64_t svc_hip_decode_levels_workspace_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h, uint32_t block_w,
                                               uint32_t block_h) {
  if (validate_decode_geom("decode_levels_workspace_bytes", frame_w, frame_h, block_w, block_h, frame_w, frame_h) ||
      validate_limits("decode_levels_workspace_bytes", n_frames, frame_w, frame_h, block_w, block_h, frame_w, frame_h))
    return 0;
  return layout_bytes(stream_ws, n_frames, make_geom(frame_w, frame_h, block_w, block_h, frame_w, frame_h).groups);
}

int svc_hip_decode_levels_frames(const uint8_t* d_frames, uint64_t stream_bytes, const uint64_t* d_frame_offsets, uint32_t n_frames,
                                 uint32_t frame_w, uint32_t frame_h, uint32_t block_w, uint32_t block_h, uint32_t mv_block_w,
                                 uint32_t mv_block_h, uint32_t fg_step, uint32_t bg_step, const uint32_t* d_gaze, uint8_t* d_workspace,
                                 uint64_t workspace_bytes, float* d_rec, uint8_t* d_display, uint32_t display_w, uint32_t display_h,
                                 uint32_t* d_status, void* stream) {
  int rc = validate_decode_geom("decode_levels", frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if (rc) return rc;
  bool display;
  if ((rc = validate_steps_display("decode_levels", fg_step, bg_step, display_w, display_h, frame_w, frame_h, &display))) return rc;
  if ((rc = validate_limits("decode_levels", n_frames, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h))) return rc;
  const Geom g = make_geom(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if ((rc = require_workspace("decode_levels", workspace_bytes, layout_bytes(stream_ws, n_frames, g.groups)))) return rc;
  if (n_frames == 0) return SVC_OK;
  SVC_REQUIRE(d_frames && d_frame_offsets && d_workspace && d_rec && d_status, "decode_levels: null pointer");
  if ((rc = validate_display_buffer("decode_levels", display, d_display))) return rc;
  SVC_REQUIRE(aligned(d_frames, 16) && aligned(d_workspace, 16) && aligned(d_frame_offsets, 8) && aligned(d_rec, 4) &&
                  aligned(d_status, 4) && aligned(d_gaze, 4),
              "decode_levels: frames and workspace must be 16-byte aligned, offsets 8-byte, output, gaze and status 4-byte");
  // planes and types null: the count pass writes neither
  const UnpackArgs u{g, d_frames, stream_bytes, d_frame_offsets, nullptr, nullptr, carve(d_workspace, stream_ws, n_frames, g.groups)};
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((rc = enqueue_unpack_scan("decode_levels", u, n_frames, d_status, s))) return rc;
  const DecodeArgs a{g, d_frames, d_frame_offsets, d_gaze, d_rec, u.ws, (float)fg_step, (float)bg_step};
  const dim3 grid(g.tiles_y * g.gx, n_frames);
  if (block_w == 8) hipLaunchKernelGGL(decode_levels_kernel<8>, grid, dim3(kThreads), 0, s, a);
  else hipLaunchKernelGGL(decode_levels_kernel<16>, grid, dim3(kThreads), 0, s, a);
  return finish_with_display("decode_levels", "reconstruction", display, d_rec, d_display, n_frames, frame_w, frame_h, display_w, display_h, s);
}

// Checked in the order of svc_hip_decode_levels_frames, `reduce` after the steps and the display size against the reduced picture.
int svc_hip_decode_levels_reduced_frames(const uint8_t* d_frames, uint64_t stream_bytes, const uint64_t* d_frame_offsets, uint32_t n_frames,
                                         uint32_t frame_w, uint32_t frame_h, uint32_t block_w, uint32_t block_h, uint32_t mv_block_w,
                                         uint32_t mv_block_h, uint32_t fg_step, uint32_t bg_step, uint32_t reduce, const uint32_t* d_gaze,
                                         uint8_t* d_workspace, uint64_t workspace_bytes, float* d_rec, uint8_t* d_display, uint32_t display_w,
                                         uint32_t display_h, uint32_t* d_status, void* stream) {
  const char* what = "decode_levels_reduced";
  int rc = validate_reduced(what, n_frames, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h, fg_step, bg_step, reduce, display_w,
                            display_h);
  if (rc) return rc;
  const uint32_t rw = frame_w / reduce, rh = frame_h / reduce;  // whole: the sides are multiples of the block, the block of `reduce`
  const bool display = display_w != 0 || display_h != 0;
  const Geom g = make_geom(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if ((rc = require_workspace(what, workspace_bytes, layout_bytes(stream_ws, n_frames, g.groups)))) return rc;
  if (n_frames == 0) return SVC_OK;
  SVC_REQUIRE(d_frames && d_frame_offsets && d_workspace && d_rec && d_status, "%s: null pointer", what);
  if ((rc = validate_display_buffer(what, display, d_display))) return rc;
  SVC_REQUIRE(aligned(d_frames, 16) && aligned(d_workspace, 16) && aligned(d_frame_offsets, 8) && aligned(d_rec, 4) &&
                  aligned(d_status, 4) && aligned(d_gaze, 4),
              "%s: frames and workspace must be 16-byte aligned, offsets 8-byte, output, gaze and status 4-byte", what);
  const UnpackArgs u{g, d_frames, stream_bytes, d_frame_offsets, nullptr, nullptr, carve(d_workspace, stream_ws, n_frames, g.groups)};
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((rc = enqueue_unpack_scan(what, u, n_frames, d_status, s))) return rc;
  const DecodeArgs a{g, d_frames, d_frame_offsets, d_gaze, d_rec, u.ws, (float)fg_step, (float)bg_step};
  const dim3 grid(g.tiles_y * g.gx, n_frames);
  launch_decode_reduced(block_w, reduce, grid, s, a);
  return finish_with_display(what, "reconstruction", display, d_rec, d_display, n_frames, rw, rh, display_w, display_h, s);
}

uint64_t svc_hip_decode_layers_workspace_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h, uint32_t block_w,
                                               uint32_t block_h) {
  if (validate_decode_geom("decode_layers_workspace_bytes", frame_w, frame_h, block_w, block_h, frame_w, frame_h) ||
      validate_limits("decode_layers_workspace_bytes", n_frames, frame_w, frame_h, block_w, block_h, frame_w, frame_h))
    return 0;
  // two streams' workspaces back to back: a stream's half is a multiple of 16 B
  return 2 * layout_bytes(stream_ws, n_frames, make_geom(frame_w, frame_h, block_w, block_h, frame_w, frame_h).groups);
}

// Checked in the order of svc_hip_decode_levels_frames.  Without a gaze no tile takes the enhancement: the call is that one on the base.
int svc_hip_decode_layers_frames(const uint8_t* d_base, uint64_t base_bytes, const uint64_t* d_base_offsets, const uint8_t* d_enh,
                                 uint64_t enh_bytes, const uint64_t* d_enh_offsets, uint32_t n_frames, uint32_t frame_w, uint32_t frame_h,
                                 uint32_t block_w, uint32_t block_h, uint32_t mv_block_w, uint32_t mv_block_h, uint32_t fg_step,
                                 uint32_t bg_step, const uint32_t* d_gaze, uint8_t* d_workspace, uint64_t workspace_bytes, float* d_rec,
                                 uint8_t* d_display, uint32_t display_w, uint32_t display_h, uint32_t* d_status, void* stream) {
  int rc = validate_decode_geom("decode_layers", frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if (rc) return rc;
  bool display;
  if ((rc = validate_steps_display("decode_layers", fg_step, bg_step, display_w, display_h, frame_w, frame_h, &display))) return rc;
  if ((rc = validate_limits("decode_layers", n_frames, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h))) return rc;
  const Geom g = make_geom(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  const uint64_t ws_stream = layout_bytes(stream_ws, n_frames, g.groups);
  if ((rc = require_workspace("decode_layers", workspace_bytes, 2 * ws_stream))) return rc;
  if (n_frames == 0) return SVC_OK;
  if (!d_gaze)
    return svc_hip_decode_levels_frames(d_base, base_bytes, d_base_offsets, n_frames, frame_w, frame_h, block_w, block_h, mv_block_w,
                                        mv_block_h, fg_step, bg_step, nullptr, d_workspace, workspace_bytes, d_rec, d_display, display_w,
                                        display_h, d_status, stream);
  SVC_REQUIRE(d_base && d_base_offsets && d_enh && d_enh_offsets && d_workspace && d_rec && d_status, "decode_layers: null pointer");
  if ((rc = validate_display_buffer("decode_layers", display, d_display))) return rc;
  SVC_REQUIRE(aligned(d_base, 16) && aligned(d_enh, 16) && aligned(d_workspace, 16) && aligned(d_base_offsets, 8) && aligned(d_enh_offsets, 8) &&
                  aligned(d_rec, 4) && aligned(d_status, 4) && aligned(d_gaze, 4),
              "decode_layers: frames and workspace must be 16-byte aligned, offsets 8-byte, output, gaze and status 4-byte");
  const UnpackArgs ub{g, d_base, base_bytes, d_base_offsets, nullptr, nullptr, carve(d_workspace, stream_ws, n_frames, g.groups)};
  const UnpackArgs ue{g, d_enh, enh_bytes, d_enh_offsets, nullptr, nullptr, carve(d_workspace + ws_stream, stream_ws, n_frames, g.groups)};
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((rc = enqueue_unpack_scan("decode_layers base", ub, n_frames, d_status, s))) return rc;
  if ((rc = enqueue_unpack_scan("decode_layers enhancement", ue, n_frames, ue.ws.status, s))) return rc;  // its codes stay in its workspace
  const DecodeLayersArgs a{{g, d_base, d_base_offsets, d_gaze, d_rec, ub.ws, (float)fg_step, (float)bg_step}, d_enh, d_enh_offsets, ue.ws};
  hipLaunchKernelGGL(layers_status_kernel, dim3(div_up(n_frames, kThreads)), dim3(kThreads), 0, s, a, n_frames, d_status);
  if ((rc = check_launch("decode_layers status"))) return rc;
  const dim3 grid(g.tiles_y * g.gx, n_frames);
  if (block_w == 8) hipLaunchKernelGGL(decode_layers_kernel<8>, grid, dim3(kThreads), 0, s, a);
  else hipLaunchKernelGGL(decode_layers_kernel<16>, grid, dim3(kThreads), 0, s, a);
  return finish_with_display("decode_layers", "reconstruction", display, d_rec, d_display, n_frames, frame_w, frame_h, display_w, display_h, s);
}

uint64_t svc_hip_decode_layers_reduced_workspace_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h, uint32_t block_w,
                                                       uint32_t block_h) {
  return svc_hip_decode_layers_workspace_bytes(n_frames, frame_w, frame_h, block_w, block_h);
}

// Checked in the order of svc_hip_decode_levels_reduced_frames, with the workspace of svc_hip_decode_layers_frames.  Without a gaze no
// tile takes the enhancement: the call is svc_hip_decode_levels_reduced_frames on the base.
int svc_hip_decode_layers_reduced_frames(const uint8_t* d_base, uint64_t base_bytes, const uint64_t* d_base_offsets, const uint8_t* d_enh,
                                         uint64_t enh_bytes, const uint64_t* d_enh_offsets, uint32_t n_frames, uint32_t frame_w,
                                         uint32_t frame_h, uint32_t block_w, uint32_t block_h, uint32_t mv_block_w, uint32_t mv_block_h,
                                         uint32_t fg_step, uint32_t bg_step, uint32_t reduce, const uint32_t* d_gaze, uint8_t* d_workspace,
                                         uint64_t workspace_bytes, float* d_rec, uint8_t* d_display, uint32_t display_w, uint32_t display_h,
                                         uint32_t* d_status, void* stream) {
  const char* what = "decode_layers_reduced";
  int rc = validate_reduced(what, n_frames, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h, fg_step, bg_step, reduce, display_w,
                            display_h);
  if (rc) return rc;
  const uint32_t rw = frame_w / reduce, rh = frame_h / reduce;  // whole: the sides are multiples of the block, the block of `reduce`
  const bool display = display_w != 0 || display_h != 0;
  const Geom g = make_geom(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  const uint64_t ws_stream = layout_bytes(stream_ws, n_frames, g.groups);
  if ((rc = require_workspace(what, workspace_bytes, 2 * ws_stream))) return rc;
  if (n_frames == 0) return SVC_OK;
  if (!d_gaze)
    return svc_hip_decode_levels_reduced_frames(d_base, base_bytes, d_base_offsets, n_frames, frame_w, frame_h, block_w, block_h, mv_block_w,
                                                mv_block_h, fg_step, bg_step, reduce, nullptr, d_workspace, workspace_bytes, d_rec, d_display,
                                                display_w, display_h, d_status, stream);
  SVC_REQUIRE(d_base && d_base_offsets && d_enh && d_enh_offsets && d_workspace && d_rec && d_status, "%s: null pointer", what);
  if ((rc = validate_display_buffer(what, display, d_display))) return rc;
  SVC_REQUIRE(aligned(d_base, 16) && aligned(d_enh, 16) && aligned(d_workspace, 16) && aligned(d_base_offsets, 8) && aligned(d_enh_offsets, 8) &&
                  aligned(d_rec, 4) && aligned(d_status, 4) && aligned(d_gaze, 4),
              "%s: frames and workspace must be 16-byte aligned, offsets 8-byte, output, gaze and status 4-byte", what);
  const UnpackArgs ub{g, d_base, base_bytes, d_base_offsets, nullptr, nullptr, carve(d_workspace, stream_ws, n_frames, g.groups)};
  const UnpackArgs ue{g, d_enh, enh_bytes, d_enh_offsets, nullptr, nullptr, carve(d_workspace + ws_stream, stream_ws, n_frames, g.groups)};
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((rc = enqueue_unpack_scan("decode_layers_reduced base", ub, n_frames, d_status, s))) return rc;
  if ((rc = enqueue_unpack_scan("decode_layers_reduced enhancement", ue, n_frames, ue.ws.status, s))) return rc;  // its codes stay in its workspace
  const DecodeLayersArgs a{{g, d_base, d_base_offsets, d_gaze, d_rec, ub.ws, (float)fg_step, (float)bg_step}, d_enh, d_enh_offsets, ue.ws};
  hipLaunchKernelGGL(layers_status_kernel, dim3(div_up(n_frames, kThreads)), dim3(kThreads), 0, s, a, n_frames, d_status);
  if ((rc = check_launch("decode_layers_reduced status"))) return rc;
  const dim3 grid(g.tiles_y * g.gx, n_frames);
  launch_decode_reduced(block_w, reduce, grid, s, a);
  return finish_with_display(what, "reconstruction", display, d_rec, d_display, n_frames, rw, rh, display_w, display_h, s);
}

uint64_t svc_hip_window_levels_workspace_bytes(uint32_t n_out, uint32_t frame_w, uint32_t frame_h, uint32_t block_w, uint32_t block_h,
                                               uint32_t mv_block_w, uint32_t mv_block_h) {
  if (validate_geom("window_levels_workspace_bytes", frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h) ||
      validate_limits("window_levels_workspace_bytes", n_out, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h))
    return 0;
  return layout_bytes(window_ws, n_out, make_geom(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h).groups);
}

// Checked in the order of the SVCQ entry points, whatever the frame counts: geometry, limits, the d_src rule, workspace, output
// capacity; n_out == 0 then returns SVC_OK; then pointers.
int svc_hip_window_levels_frames(const uint8_t* d_frames, uint64_t stream_bytes, const uint64_t* d_frame_offsets, uint32_t n_in,
                                 const uint32_t* d_src, uint32_t n_out, uint32_t frame_w, uint32_t frame_h, uint32_t block_w,
                                 uint32_t block_h, uint32_t mv_block_w, uint32_t mv_block_h, const uint32_t* d_window,
                                 uint8_t* d_workspace, uint64_t workspace_bytes, uint8_t* d_out, uint64_t out_capacity,
                                 uint64_t* d_out_offsets, uint32_t* d_status, void* stream) {
  int rc = validate_geom("window_levels", frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if (!rc) rc = validate_limits("window_levels", std::max(n_out, n_in), frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if (rc) return rc;
  SVC_REQUIRE(d_src || n_out == n_in, "window_levels: without d_src output frame i is input frame i, but n_out is %u and n_in %u", n_out,
              n_in);
  const Geom g = make_geom(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if ((rc = require_workspace("window_levels", workspace_bytes, layout_bytes(window_ws, n_out, g.groups)))) return rc;
  const uint64_t max_bytes = frame_layout(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h).max_bytes;
  if ((rc = require_capacity("window_levels", "output", out_capacity, n_out * max_bytes))) return rc;
  if (n_out == 0) return SVC_OK;
  SVC_REQUIRE(d_frames && d_frame_offsets && d_workspace && d_out && d_out_offsets && d_status, "window_levels: null pointer");
  SVC_REQUIRE(aligned(d_frames, 16) && aligned(d_out, 16) && aligned(d_workspace, 16) && aligned(d_frame_offsets, 8) &&
                  aligned(d_out_offsets, 8) && aligned(d_src, 4) && aligned(d_window, 4) && aligned(d_status, 4),
              "window_levels: streams and workspace must be 16-byte aligned, offsets 8-byte, source indices, windows and status 4-byte");
  const WindowArgs a{g, d_frames, stream_bytes, d_frame_offsets, n_in, d_src, d_window, d_out, d_out_offsets, d_status,
                     carve(d_workspace, window_ws, n_out, g.groups)};
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(window_count_kernel, dim3(div_up(g.groups, kThreads / 64), n_out), dim3(kThreads), 0, s, a);
  if ((rc = check_launch("window_levels", "count"))) return rc;
  hipLaunchKernelGGL(window_scan_kernel, dim3(n_out), dim3(kThreads), 0, s, a);
  if ((rc = check_launch("window_levels", "scan"))) return rc;
  if ((rc = enqueue_frame_offsets("window_levels", 1, OffsetsJob{a.ws.frame_bytes, d_out_offsets, nullptr}, OffsetsJob{}, n_out, stream)))
    return rc;
  // a workgroup's pass is 4 KB of an output frame; the grid holds twice the header, types and masks (a window's levels are fewer
  // bytes than its frame's masks), and a frame that keeps more is walked in further passes
  const uint32_t fixed = div_up((uint32_t)(up16(g.levels_off) / 16), kThreads), most = div_up((uint32_t)(max_bytes / 16), kThreads);
  hipLaunchKernelGGL(window_write_kernel, dim3(std::min(2 * fixed, most), n_out), dim3(kThreads), 0, s, a);
  return check_launch("window_levels", "write");
}

uint64_t svc_hip_band_levels_workspace_bytes(uint32_t n_out, uint32_t frame_w, uint32_t frame_h, uint32_t block_w, uint32_t block_h,
                                             uint32_t mv_block_w, uint32_t mv_block_h) {
  if (validate_geom("band_levels_workspace_bytes", frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h) ||
      validate_limits("band_levels_workspace_bytes", n_out, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h))
    return 0;
  return layout_bytes(band_ws, n_out, make_geom(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h).groups);
}

// Checked as svc_hip_window_levels_frames, in its order: geometry, limits, the d_src rule, workspace, output capacity; n_out == 0 then
// returns SVC_OK; then pointers.
int svc_hip_band_levels_frames(const uint8_t* d_frames, uint64_t stream_bytes, const uint64_t* d_frame_offsets, uint32_t n_in,
                               const uint32_t* d_src, uint32_t n_out, uint32_t frame_w, uint32_t frame_h, uint32_t block_w,
                               uint32_t block_h, uint32_t mv_block_w, uint32_t mv_block_h, const uint32_t* d_window, const uint32_t* d_band,
                               uint8_t* d_workspace, uint64_t workspace_bytes, uint8_t* d_out, uint64_t out_capacity,
                               uint64_t* d_out_offsets, uint32_t* d_status, void* stream) {
  int rc = validate_geom("band_levels", frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if (!rc) rc = validate_limits("band_levels", std::max(n_out, n_in), frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if (rc) return rc;
  SVC_REQUIRE(d_src || n_out == n_in, "band_levels: without d_src output frame i is input frame i, but n_out is %u and n_in %u", n_out, n_in);
  const Geom g = make_geom(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if ((rc = require_workspace("band_levels", workspace_bytes, layout_bytes(band_ws, n_out, g.groups)))) return rc;
  const uint64_t max_bytes = frame_layout(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h).max_bytes;
  if ((rc = require_capacity("band_levels", "output", out_capacity, n_out * max_bytes))) return rc;
  if (n_out == 0) return SVC_OK;
  SVC_REQUIRE(d_frames && d_frame_offsets && d_workspace && d_out && d_out_offsets && d_status, "band_levels: null pointer");
  SVC_REQUIRE(aligned(d_frames, 16) && aligned(d_out, 16) && aligned(d_workspace, 16) && aligned(d_frame_offsets, 8) &&
                  aligned(d_out_offsets, 8) && aligned(d_src, 4) && aligned(d_window, 4) && aligned(d_band, 4) && aligned(d_status, 4),
              "band_levels: streams and workspace must be 16-byte aligned, offsets 8-byte, source indices, windows, bands and status 4-byte");
  const BandWs ws = carve(d_workspace, band_ws, n_out, g.groups);
  const BandArgs a{{g, d_frames, stream_bytes, d_frame_offsets, n_in, d_src, d_window, d_out, d_out_offsets, d_status, ws.in},
                   d_band, ws.kept, ws.frame_bytes, ws.frame_levels};
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 waves(div_up(g.groups, kThreads / 64), n_out);
  // the input pass: the window call's count and scan with every tile kept
  WindowArgs in = a.w;
  in.window = nullptr;
  hipLaunchKernelGGL(window_count_kernel, waves, dim3(kThreads), 0, s, in);
  if ((rc = check_launch("band_levels", "input count"))) return rc;
  hipLaunchKernelGGL(window_scan_kernel, dim3(n_out), dim3(kThreads), 0, s, in);
  if ((rc = check_launch("band_levels", "input scan"))) return rc;
  hipLaunchKernelGGL(band_count_kernel, waves, dim3(kThreads), 0, s, a);
  if ((rc = check_launch("band_levels", "count"))) return rc;
  hipLaunchKernelGGL(band_scan_kernel, dim3(n_out), dim3(kThreads), 0, s, a);
  if ((rc = check_launch("band_levels", "scan"))) return rc;
  if ((rc = enqueue_frame_offsets("band_levels", 1, OffsetsJob{ws.frame_bytes, d_out_offsets, nullptr}, OffsetsJob{}, n_out, stream))) return rc;
  const uint32_t cap = g.tpg * g.bw * g.bh;
  hipLaunchKernelGGL(band_write_kernel, waves, dim3(kThreads), select_write_lds(cap), s, a, cap);
  return check_launch("band_levels", "write");
}

uint64_t svc_hip_union_levels_workspace_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h, uint32_t block_w, uint32_t block_h,
                                              uint32_t mv_block_w, uint32_t mv_block_h) {
  if (validate_geom("union_levels_workspace_bytes", frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h) ||
      validate_limits("union_levels_workspace_bytes", n_frames, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h))
    return 0;
  return layout_bytes(union_ws, n_frames, make_geom(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h).groups);
}

// Checked in the window call's order: geometry, limits, workspace, output capacity; n_frames == 0 then returns SVC_OK; then pointers.
int svc_hip_union_levels_frames(const uint8_t* d_a, uint64_t a_bytes, const uint64_t* d_a_offsets, const uint8_t* d_b, uint64_t b_bytes,
                                const uint64_t* d_b_offsets, uint32_t n_frames, uint32_t frame_w, uint32_t frame_h, uint32_t block_w,
                                uint32_t block_h, uint32_t mv_block_w, uint32_t mv_block_h, uint8_t* d_workspace, uint64_t workspace_bytes,
                                uint8_t* d_out, uint64_t out_capacity, uint64_t* d_out_offsets, uint32_t* d_status, void* stream) {
  int rc = validate_geom("union_levels", frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if (!rc) rc = validate_limits("union_levels", n_frames, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if (rc) return rc;
  const Geom g = make_geom(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if ((rc = require_workspace("union_levels", workspace_bytes, layout_bytes(union_ws, n_frames, g.groups)))) return rc;
  const uint64_t max_bytes = frame_layout(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h).max_bytes;
  if ((rc = require_capacity("union_levels", "output", out_capacity, n_frames * max_bytes))) return rc;
  if (n_frames == 0) return SVC_OK;
  SVC_REQUIRE(d_a && d_a_offsets && d_b && d_b_offsets && d_workspace && d_out && d_out_offsets && d_status, "union_levels: null pointer");
  SVC_REQUIRE(aligned(d_a, 16) && aligned(d_b, 16) && aligned(d_out, 16) && aligned(d_workspace, 16) && aligned(d_a_offsets, 8) &&
                  aligned(d_b_offsets, 8) && aligned(d_out_offsets, 8) && aligned(d_status, 4),
              "union_levels: streams and workspace must be 16-byte aligned, offsets 8-byte, status 4-byte");
  const UnionWs ws = carve(d_workspace, union_ws, n_frames, g.groups);
  const UnionArgs u{{g, d_a, a_bytes, d_a_offsets, n_frames, nullptr, nullptr, d_out, d_out_offsets, d_status, ws.a},
                    {g, d_b, b_bytes, d_b_offsets, n_frames, nullptr, nullptr, nullptr, nullptr, d_status, ws.b},
                    ws.cnt, ws.overlap, ws.frame_bytes, ws.frame_levels, ws.status};
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 waves(div_up(g.groups, kThreads / 64), n_frames);
  // the input pass of each stream: the window call's count and scan with every tile kept (d_status holds A's, then B's codes until the
  // scan below writes the pair's)
  for (const WindowArgs* in : {&u.a, &u.b}) {
    const char* which = in == &u.a ? "input count" : "second input count";
    hipLaunchKernelGGL(window_count_kernel, waves, dim3(kThreads), 0, s, *in);
    if ((rc = check_launch("union_levels", which))) return rc;
    hipLaunchKernelGGL(window_scan_kernel, dim3(n_frames), dim3(kThreads), 0, s, *in);
    if ((rc = check_launch("union_levels", "input scan"))) return rc;
  }
  hipLaunchKernelGGL(union_count_kernel, waves, dim3(kThreads), 0, s, u);
  if ((rc = check_launch("union_levels", "count"))) return rc;
  hipLaunchKernelGGL(union_scan_kernel, dim3(n_frames), dim3(kThreads), 0, s, u);
  if ((rc = check_launch("union_levels", "scan"))) return rc;
  if ((rc = enqueue_frame_offsets("union_levels", 1, OffsetsJob{ws.frame_bytes, d_out_offsets, nullptr}, OffsetsJob{}, n_frames, stream)))
    return rc;
  const uint32_t cap = g.tpg * g.bw * g.bh;
  hipLaunchKernelGGL(union_write_kernel, waves, dim3(kThreads), select_write_lds(cap), s, u, cap);
  return check_launch("union_levels", "write");
}

uint64_t svc_hip_delta_levels_workspace_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h, uint32_t block_w, uint32_t block_h,
                                              uint32_t mv_block_w, uint32_t mv_block_h) {
  if (validate_geom("delta_levels_workspace_bytes", frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h) ||
      validate_limits("delta_levels_workspace_bytes", n_frames, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h))
    return 0;
  return layout_bytes(delta_ws, n_frames, make_geom(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h).groups);
}

int svc_hip_delta_levels_frames(const uint8_t* d_frames, uint64_t stream_bytes, const uint64_t* d_frame_offsets, uint32_t n_frames,
                                const uint8_t* d_prev, uint64_t prev_bytes, const uint32_t* d_key, uint32_t frame_w, uint32_t frame_h,
                                uint32_t block_w, uint32_t block_h, uint32_t mv_block_w, uint32_t mv_block_h, uint8_t* d_workspace,
                                uint64_t workspace_bytes, uint8_t* d_out, uint64_t out_capacity, uint64_t* d_out_offsets, uint32_t* d_status,
                                void* stream) {
  return delta_levels("delta_levels", false, 1, d_frames, stream_bytes, d_frame_offsets, n_frames, d_prev, prev_bytes, d_key, frame_w, frame_h,
                      block_w, block_h, mv_block_w, mv_block_h, d_workspace, workspace_bytes, d_out, out_capacity, d_out_offsets, d_status, stream);
}

// (the two directions share one workspace layout)
uint64_t svc_hip_undelta_levels_workspace_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h, uint32_t block_w, uint32_t block_h,
                                                uint32_t mv_block_w, uint32_t mv_block_h) {
  if (validate_geom("undelta_levels_workspace_bytes", frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h) ||
      validate_limits("undelta_levels_workspace_bytes", n_frames, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h))
    return 0;
  return layout_bytes(delta_ws, n_frames, make_geom(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h).groups);
}

int svc_hip_undelta_levels_frames(const uint8_t* d_frames, uint64_t stream_bytes, const uint64_t* d_frame_offsets, uint32_t n_frames,
                                  const uint8_t* d_prev, uint64_t prev_bytes, const uint32_t* d_key, uint32_t frame_w, uint32_t frame_h,
                                  uint32_t block_w, uint32_t block_h, uint32_t mv_block_w, uint32_t mv_block_h, uint8_t* d_workspace,
                                  uint64_t workspace_bytes, uint8_t* d_out, uint64_t out_capacity, uint64_t* d_out_offsets, uint32_t* d_status,
                                  void* stream) {
  return delta_levels("undelta_levels", true, 1, d_frames, stream_bytes, d_frame_offsets, n_frames, d_prev, prev_bytes, d_key, frame_w, frame_h,
                      block_w, block_h, mv_block_w, mv_block_h, d_workspace, workspace_bytes, d_out, out_capacity, d_out_offsets, d_status, stream);
}

uint64_t svc_hip_decode_delta_levels_workspace_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h, uint32_t block_w,
                                                     uint32_t block_h, uint32_t mv_block_w, uint32_t mv_block_h) {
  if (validate_decode_geom("decode_delta_levels_workspace_bytes", frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h) ||
      validate_limits("decode_delta_levels_workspace_bytes", n_frames, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h))
    return 0;
  const Geom g = make_geom(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  return layout_bytes(decode_delta_ws, n_frames, g.groups, g.tpg * block_w * block_h);
}

// Checked in the order of svc_hip_decode_levels_frames, then last_capacity; n_frames == 0 then returns SVC_OK; then pointers.  Four launches
// without d_prev, d_last and display, ten with all three, whatever n_frames.  period 1: svc_hip_decode_delta_levels_frames; 2 or 4: the
// temporal call, which differs in the status kernel, in the reconstruction kernel and in the frame d_last holds.
static int decode_delta_levels(const char* what, uint32_t period, const uint8_t* d_frames, uint64_t stream_bytes,
                               const uint64_t* d_frame_offsets, uint32_t n_frames, const uint8_t* d_prev, uint64_t prev_bytes,
                               const uint32_t* d_key, uint32_t frame_w, uint32_t frame_h, uint32_t block_w, uint32_t block_h,
                               uint32_t mv_block_w, uint32_t mv_block_h, uint32_t fg_step, uint32_t bg_step, const uint32_t* d_gaze,
                               uint8_t* d_workspace, uint64_t workspace_bytes, float* d_rec, uint8_t* d_display, uint32_t display_w,
                               uint32_t display_h, uint8_t* d_last, uint64_t last_capacity, uint64_t* d_last_bytes, uint32_t* d_status,
                               void* stream) {
  int rc = validate_decode_geom(what, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if (rc) return rc;
  if ((rc = validate_period(what, period))) return rc;
  bool display;
  if ((rc = validate_steps_display(what, fg_step, bg_step, display_w, display_h, frame_w, frame_h, &display))) return rc;
  if ((rc = validate_limits(what, n_frames, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h))) return rc;
  const Geom g = make_geom(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  const uint32_t cap = g.tpg * block_w * block_h;
  if ((rc = require_workspace(what, workspace_bytes, layout_bytes(decode_delta_ws, n_frames, g.groups, cap)))) return rc;
  if (d_last && (rc = require_capacity(what, "last frame", last_capacity,
                                       frame_layout(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h).max_bytes)))
    return rc;
  if (n_frames == 0) return SVC_OK;
  SVC_REQUIRE(d_frames && d_frame_offsets && d_workspace && d_rec && d_status, "%s: null pointer", what);
  SVC_REQUIRE((d_last != nullptr) == (d_last_bytes != nullptr), "%s: the last frame and its length go together", what);
  if ((rc = validate_display_buffer(what, display, d_display))) return rc;
  SVC_REQUIRE(aligned(d_frames, 16) && aligned(d_prev, 16) && aligned(d_last, 16) && aligned(d_workspace, 16) && aligned(d_frame_offsets, 8) &&
                  aligned(d_last_bytes, 8) && aligned(d_key, 4) && aligned(d_gaze, 4) && aligned(d_rec, 4) && aligned(d_status, 4),
              "%s: streams, the frame before, the last frame and workspace must be 16-byte aligned, offsets and the last frame's length "
              "8-byte, key flags, gaze, output and status 4-byte",
              what);
  const DecodeDeltaWs ws = carve(d_workspace, decode_delta_ws, n_frames, g.groups, cap);
  const DecodeDeltaArgs a{{{g, d_frames, stream_bytes, d_frame_offsets, n_frames, nullptr, nullptr, nullptr, nullptr, d_status, ws.in},
                           {g, d_prev, prev_bytes, ws.prev_offsets, 1, nullptr, nullptr, nullptr, nullptr, ws.prev_code, ws.prev},
                           d_key, n_frames, nullptr, nullptr, nullptr, ws.status},
                          d_gaze, d_rec, (float)fg_step, (float)bg_step, d_last, d_last_bytes, ws.last_cnt, ws.last_first, ws.last_head,
                          ws.last_runs, cap};
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((rc = enqueue_delta_input(what, a.d, true, prev_bytes, s, period))) return rc;
  const dim3 chains(g.tiles_y * g.gx);
  const uint32_t last_frame = (n_frames - 1) / period * period;  // the frame the next call's frame 0 refers to
  if (period == 1) {
    if (block_w == 8) hipLaunchKernelGGL(decode_delta_kernel<8>, chains, dim3(kThreads), 0, s, a);
    else hipLaunchKernelGGL(decode_delta_kernel<16>, chains, dim3(kThreads), 0, s, a);
  } else if (period == 2) {
    if (block_w == 8) hipLaunchKernelGGL((decode_delta_temporal_kernel<8, 1>), chains, dim3(kThreads), 0, s, a, last_frame);
    else hipLaunchKernelGGL((decode_delta_temporal_kernel<16, 1>), chains, dim3(kThreads), 0, s, a, last_frame);
  } else {
    if (block_w == 8) hipLaunchKernelGGL((decode_delta_temporal_kernel<8, 2>), chains, dim3(kThreads), 0, s, a, last_frame);
    else hipLaunchKernelGGL((decode_delta_temporal_kernel<16, 2>), chains, dim3(kThreads), 0, s, a, last_frame);
  }
  if (d_last) {
    if ((rc = check_launch(what, "reconstruction"))) return rc;
    DecodeDeltaArgs last = a;  // the two kernels take the call's last frame for the one d_last holds
    last.d.n = last_frame + 1;
    hipLaunchKernelGGL(decode_delta_last_scan_kernel, dim3(1), dim3(kThreads), 0, s, last);
    if ((rc = check_launch(what, "scan of the last frame"))) return rc;
    hipLaunchKernelGGL(decode_delta_last_write_kernel, dim3(div_up(g.groups, kThreads / 64)), dim3(kThreads), 0, s, last);
  }
  return finish_with_display(what, d_last ? "write of the last frame" : "reconstruction", display, d_rec, d_display, n_frames, frame_w,
                             frame_h, display_w, display_h, s);
}

int svc_hip_decode_delta_levels_frames(const uint8_t* d_frames, uint64_t stream_bytes, const uint64_t* d_frame_offsets, uint32_t n_frames,
                                       const uint8_t* d_prev, uint64_t prev_bytes, const uint32_t* d_key, uint32_t frame_w, uint32_t frame_h,
                                       uint32_t block_w, uint32_t block_h, uint32_t mv_block_w, uint32_t mv_block_h, uint32_t fg_step,
                                       uint32_t bg_step, const uint32_t* d_gaze, uint8_t* d_workspace, uint64_t workspace_bytes, float* d_rec,
                                       uint8_t* d_display, uint32_t display_w, uint32_t display_h, uint8_t* d_last, uint64_t last_capacity,
                                       uint64_t* d_last_bytes, uint32_t* d_status, void* stream) {
  return decode_delta_levels("decode_delta_levels", 1, d_frames, stream_bytes, d_frame_offsets, n_frames, d_prev, prev_bytes, d_key, frame_w,
                             frame_h, block_w, block_h, mv_block_w, mv_block_h, fg_step, bg_step, d_gaze, d_workspace, workspace_bytes, d_rec,
                             d_display, display_w, display_h, d_last, last_capacity, d_last_bytes, d_status, stream);
}

// ---- temporal layers: the three calls above with a period (the workspaces are their siblings')

uint64_t svc_hip_delta_levels_temporal_workspace_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h, uint32_t block_w,
                                                       uint32_t block_h, uint32_t mv_block_w, uint32_t mv_block_h, uint32_t period) {
  if (validate_geom("delta_levels_temporal_workspace_bytes", frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h) ||
      validate_period("delta_levels_temporal_workspace_bytes", period))
    return 0;
  return svc_hip_delta_levels_workspace_bytes(n_frames, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
}

int svc_hip_delta_levels_temporal_frames(const uint8_t* d_frames, uint64_t stream_bytes, const uint64_t* d_frame_offsets, uint32_t n_frames,
                                         const uint8_t* d_prev, uint64_t prev_bytes, const uint32_t* d_key, uint32_t frame_w,
                                         uint32_t frame_h, uint32_t block_w, uint32_t block_h, uint32_t mv_block_w, uint32_t mv_block_h,
                                         uint8_t* d_workspace, uint64_t workspace_bytes, uint8_t* d_out, uint64_t out_capacity,
                                         uint64_t* d_out_offsets, uint32_t* d_status, void* stream, uint32_t period) {
  return delta_levels("delta_levels_temporal", false, period, d_frames, stream_bytes, d_frame_offsets, n_frames, d_prev, prev_bytes, d_key,
                      frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h, d_workspace, workspace_bytes, d_out, out_capacity,
                      d_out_offsets, d_status, stream);
}

uint64_t svc_hip_undelta_levels_temporal_workspace_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h, uint32_t block_w,
                                                         uint32_t block_h, uint32_t mv_block_w, uint32_t mv_block_h, uint32_t period) {
  if (validate_geom("undelta_levels_temporal_workspace_bytes", frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h) ||
      validate_period("undelta_levels_temporal_workspace_bytes", period))
    return 0;
  return svc_hip_undelta_levels_workspace_bytes(n_frames, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
}

int svc_hip_undelta_levels_temporal_frames(const uint8_t* d_frames, uint64_t stream_bytes, const uint64_t* d_frame_offsets,
                                           uint32_t n_frames, const uint8_t* d_prev, uint64_t prev_bytes, const uint32_t* d_key,
                                           uint32_t frame_w, uint32_t frame_h, uint32_t block_w, uint32_t block_h, uint32_t mv_block_w,
                                           uint32_t mv_block_h, uint8_t* d_workspace, uint64_t workspace_bytes, uint8_t* d_out,
                                           uint64_t out_capacity, uint64_t* d_out_offsets, uint32_t* d_status, void* stream,
                                           uint32_t period) {
  return delta_levels("undelta_levels_temporal", true, period, d_frames, stream_bytes, d_frame_offsets, n_frames, d_prev, prev_bytes, d_key,
                      frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h, d_workspace, workspace_bytes, d_out, out_capacity,
                      d_out_offsets, d_status, stream);
}

uint64_t svc_hip_decode_delta_levels_temporal_workspace_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h, uint32_t block_w,
                                                              uint32_t block_h, uint32_t mv_block_w, uint32_t mv_block_h,
                                                              uint32_t period) {
  if (validate_decode_geom("decode_delta_levels_temporal_workspace_bytes", frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h) ||
      validate_period("decode_delta_levels_temporal_workspace_bytes", period))
    return 0;
  return svc_hip_decode_delta_levels_workspace_bytes(n_frames, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
}

int svc_hip_decode_delta_levels_temporal_frames(const uint8_t* d_frames, uint64_t stream_bytes, const uint64_t* d_frame_offsets,
                                                uint32_t n_frames, const uint8_t* d_prev, uint64_t prev_bytes, const uint32_t* d_key,
                                                uint32_t frame_w, uint32_t frame_h, uint32_t block_w, uint32_t block_h,
                                                uint32_t mv_block_w, uint32_t mv_block_h, uint32_t fg_step, uint32_t bg_step,
                                                const uint32_t* d_gaze, uint8_t* d_workspace, uint64_t workspace_bytes, float* d_rec,
                                                uint8_t* d_display, uint32_t display_w, uint32_t display_h, uint8_t* d_last,
                                                uint64_t last_capacity, uint64_t* d_last_bytes, uint32_t* d_status, void* stream,
                                                uint32_t period) {
  return decode_delta_levels("decode_delta_levels_temporal", period, d_frames, stream_bytes, d_frame_offsets, n_frames, d_prev, prev_bytes,
                             d_key, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h, fg_step, bg_step, d_gaze, d_workspace,
                             workspace_bytes, d_rec, d_display, display_w, display_h, d_last, last_capacity, d_last_bytes, d_status, stream);
}

// (the workspace of svc_hip_decode_delta_levels_frames: a group's run of the last frame is placed at its full-size worst case)
uint64_t svc_hip_decode_delta_levels_reduced_workspace_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h, uint32_t block_w,
                                                             uint32_t block_h, uint32_t mv_block_w, uint32_t mv_block_h) {
  if (validate_decode_geom("decode_delta_levels_reduced_workspace_bytes", frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h) ||
      validate_limits("decode_delta_levels_reduced_workspace_bytes", n_frames, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h))
    return 0;
  const Geom g = make_geom(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  return layout_bytes(decode_delta_ws, n_frames, g.groups, g.tpg * block_w * block_h);
}

// Checked in the order of svc_hip_decode_levels_reduced_frames (the period right after the geometry), then last_capacity; n_frames == 0
// then returns SVC_OK; then pointers.  The launches are those of svc_hip_decode_delta_levels_frames.  period 1:
// svc_hip_decode_delta_levels_reduced_frames; 2 or 4: the temporal call, which differs in the status kernel, in the reconstruction kernel
// and in the frame d_last holds.
static int decode_delta_levels_reduced(const char* what, uint32_t period, const uint8_t* d_frames, uint64_t stream_bytes,
                                       const uint64_t* d_frame_offsets, uint32_t n_frames, const uint8_t* d_prev, uint64_t prev_bytes,
                                       const uint32_t* d_key, uint32_t frame_w, uint32_t frame_h, uint32_t block_w, uint32_t block_h,
                                       uint32_t mv_block_w, uint32_t mv_block_h, uint32_t fg_step, uint32_t bg_step, uint32_t reduce,
                                       const uint32_t* d_gaze, uint8_t* d_workspace, uint64_t workspace_bytes, float* d_rec,
                                       uint8_t* d_display, uint32_t display_w, uint32_t display_h, uint8_t* d_last, uint64_t last_capacity,
                                       uint64_t* d_last_bytes, uint32_t* d_status, void* stream) {
  int rc = validate_decode_geom(what, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if (rc) return rc;
  if ((rc = validate_period(what, period))) return rc;
  if ((rc = validate_reduced(what, n_frames, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h, fg_step, bg_step, reduce, display_w,
                             display_h)))
    return rc;
  const uint32_t rw = frame_w / reduce, rh = frame_h / reduce;  // whole: the sides are multiples of the block, the block of `reduce`
  const bool display = display_w != 0 || display_h != 0;
  const Geom g = make_geom(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  const uint32_t cap = g.tpg * block_w * block_h;
  if ((rc = require_workspace(what, workspace_bytes, layout_bytes(decode_delta_ws, n_frames, g.groups, cap)))) return rc;
  if (d_last && (rc = require_capacity(what, "last frame", last_capacity,
                                       frame_layout(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h).max_bytes)))
    return rc;
  if (n_frames == 0) return SVC_OK;
  SVC_REQUIRE(d_frames && d_frame_offsets && d_workspace && d_rec && d_status, "%s: null pointer", what);
  SVC_REQUIRE((d_last != nullptr) == (d_last_bytes != nullptr), "%s: the last frame and its length go together", what);
  if ((rc = validate_display_buffer(what, display, d_display))) return rc;
  SVC_REQUIRE(aligned(d_frames, 16) && aligned(d_prev, 16) && aligned(d_last, 16) && aligned(d_workspace, 16) && aligned(d_frame_offsets, 8) &&
                  aligned(d_last_bytes, 8) && aligned(d_key, 4) && aligned(d_gaze, 4) && aligned(d_rec, 4) && aligned(d_status, 4),
              "%s: streams, the frame before, the last frame and workspace must be 16-byte aligned, offsets and the last frame's length "
              "8-byte, key flags, gaze, output and status 4-byte",
              what);
  const DecodeDeltaWs ws = carve(d_workspace, decode_delta_ws, n_frames, g.groups, cap);
  const DecodeDeltaArgs a{{{g, d_frames, stream_bytes, d_frame_offsets, n_frames, nullptr, nullptr, nullptr, nullptr, d_status, ws.in},
                           {g, d_prev, prev_bytes, ws.prev_offsets, 1, nullptr, nullptr, nullptr, nullptr, ws.prev_code, ws.prev},
                           d_key, n_frames, nullptr, nullptr, nullptr, ws.status},
                          d_gaze, d_rec, (float)fg_step, (float)bg_step, d_last, d_last_bytes, ws.last_cnt, ws.last_first, ws.last_head,
                          ws.last_runs, cap};
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((rc = enqueue_delta_input(what, a.d, true, prev_bytes, s, period))) return rc;
  const uint32_t last_frame = (n_frames - 1) / period * period;  // the frame the next call's frame 0 refers to
  if (period == 1) launch_decode_delta_reduced(block_w, reduce, dim3(g.tiles_y * g.gx), s, a);
  else launch_decode_delta_temporal_reduced(block_w, reduce, period, dim3(g.tiles_y * g.gx), s, a, last_frame);
  if (d_last) {
    if ((rc = check_launch(what, "reconstruction"))) return rc;
    DecodeDeltaArgs last = a;  // the two kernels take the call's last frame for the one d_last holds
    last.d.n = last_frame + 1;
    hipLaunchKernelGGL(decode_delta_last_scan_kernel, dim3(1), dim3(kThreads), 0, s, last);
    if ((rc = check_launch(what, "scan of the last frame"))) return rc;
    hipLaunchKernelGGL(decode_delta_last_write_kernel, dim3(div_up(g.groups, kThreads / 64)), dim3(kThreads), 0, s, last);
  }
  return finish_with_display(what, d_last ? "write of the last frame" : "reconstruction", display, d_rec, d_display, n_frames, rw, rh,
                             display_w, display_h, s);
}

int svc_hip_decode_delta_levels_reduced_frames(const uint8_t* d_frames, uint64_t stream_bytes, const uint64_t* d_frame_offsets,
                                               uint32_t n_frames, const uint8_t* d_prev, uint64_t prev_bytes, const uint32_t* d_key,
                                               uint32_t frame_w, uint32_t frame_h, uint32_t block_w, uint32_t block_h, uint32_t mv_block_w,
                                               uint32_t mv_block_h, uint32_t fg_step, uint32_t bg_step, uint32_t reduce, const uint32_t* d_gaze,
                                               uint8_t* d_workspace, uint64_t workspace_bytes, float* d_rec, uint8_t* d_display,
                                               uint32_t display_w, uint32_t display_h, uint8_t* d_last, uint64_t last_capacity,
                                               uint64_t* d_last_bytes, uint32_t* d_status, void* stream) {
  return decode_delta_levels_reduced("decode_delta_levels_reduced", 1, d_frames, stream_bytes, d_frame_offsets, n_frames, d_prev, prev_bytes,
                                     d_key, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h, fg_step, bg_step, reduce, d_gaze,
                                     d_workspace, workspace_bytes, d_rec, d_display, display_w, display_h, d_last, last_capacity, d_last_bytes,
                                     d_status, stream);
}

// (include/svc_hip_temporal_decode.h) the workspace is the reduced call's
uint64_t svc_hip_decode_delta_levels_temporal_reduced_workspace_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h, uint32_t block_w,
                                                                      uint32_t block_h, uint32_t mv_block_w, uint32_t mv_block_h,
                                                                      uint32_t period) {
  if (validate_decode_geom("decode_delta_levels_temporal_reduced_workspace_bytes", frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h) ||
      validate_period("decode_delta_levels_temporal_reduced_workspace_bytes", period))
    return 0;
  return svc_hip_decode_delta_levels_reduced_workspace_bytes(n_frames, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
}

int svc_hip_decode_delta_levels_temporal_reduced_frames(const uint8_t* d_frames, uint64_t stream_bytes, const uint64_t* d_frame_offsets,
                                                        uint32_t n_frames, const uint8_t* d_prev, uint64_t prev_bytes, const uint32_t* d_key,
                                                        uint32_t frame_w, uint32_t frame_h, uint32_t block_w, uint32_t block_h,
                                                        uint32_t mv_block_w, uint32_t mv_block_h, uint32_t fg_step, uint32_t bg_step,
                                                        uint32_t reduce, const uint32_t* d_gaze, uint8_t* d_workspace,
                                                        uint64_t workspace_bytes, float* d_rec, uint8_t* d_display, uint32_t display_w,
                                                        uint32_t display_h, uint8_t* d_last, uint64_t last_capacity, uint64_t* d_last_bytes,
                                                        uint32_t* d_status, void* stream, uint32_t period) {
  return decode_delta_levels_reduced("decode_delta_levels_temporal_reduced", period, d_frames, stream_bytes, d_frame_offsets, n_frames, d_prev,
                                     prev_bytes, d_key, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h, fg_step, bg_step, reduce,
                                     d_gaze, d_workspace, workspace_bytes, d_rec, d_display, display_w, display_h, d_last, last_capacity,
                                     d_last_bytes, d_status, stream);
}

uint64_t svc_hip_split_levels_workspace_bytes(uint32_t n_in, uint32_t n_out, uint32_t frame_w, uint32_t frame_h, uint32_t block_w,
                                              uint32_t block_h, uint32_t mv_block_w, uint32_t mv_block_h) {
  if (validate_geom("split_levels_workspace_bytes", frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h) ||
      validate_limits("split_levels_workspace_bytes", std::max(n_in, n_out), frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h))
    return 0;
  return layout_bytes(split_ws, n_out, make_geom(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h).groups, 0u);
}

uint64_t svc_hip_split_levels_budget_workspace_bytes(uint32_t n_in, uint32_t n_out, uint32_t frame_w, uint32_t frame_h, uint32_t block_w,
                                                     uint32_t block_h, uint32_t mv_block_w, uint32_t mv_block_h, uint32_t ladder_len) {
  if (validate_geom("split_levels_budget_workspace_bytes", frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h) ||
      validate_limits("split_levels_budget_workspace_bytes", std::max(n_in, n_out), frame_w, frame_h, block_w, block_h, mv_block_w,
                      mv_block_h))
    return 0;
  if (ladder_len == 0 || ladder_len > kMaxLadder) {
    (void)fail(SVC_ERR_INVALID_ARG, "split_levels_budget_workspace_bytes: a ladder of %u entries (1 .. %u)", ladder_len, kMaxLadder);
    return 0;
  }
  return layout_bytes(split_ws, n_out, make_geom(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h).groups, ladder_len);
}

// Checked in the order of the SVCQ entry points, whatever the frame counts: geometry, steps, limits, the d_src rule, workspace, the two
// capacities; n_out == 0 then returns SVC_OK; then pointers.
int svc_hip_split_levels_frames(const uint8_t* d_frames, uint64_t stream_bytes, const uint64_t* d_frame_offsets, uint32_t n_in,
                                const uint32_t* d_src, uint32_t n_out, uint32_t frame_w, uint32_t frame_h, uint32_t block_w,
                                uint32_t block_h, uint32_t mv_block_w, uint32_t mv_block_h, uint32_t fine_step, uint32_t fg_step,
                                uint32_t bg_step, const uint32_t* d_window, uint8_t* d_workspace, uint64_t workspace_bytes,
                                uint8_t* d_base_out, uint64_t base_capacity, uint64_t* d_base_offsets, uint8_t* d_enh_out,
                                uint64_t enh_capacity, uint64_t* d_enh_offsets, uint32_t* d_status, void* stream) {
  int rc = validate_geom("split_levels", frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if (rc) return rc;
  SVC_REQUIRE(fine_step > 0 && fg_step > 0 && bg_step > 0, "split_levels: quant steps must be positive");
  if ((rc = validate_split_steps("split_levels", fine_step, fg_step, bg_step))) return rc;
  SplitArgs a = split_args(d_frames, stream_bytes, d_frame_offsets, n_in, d_src, n_out, frame_w, frame_h, block_w, block_h, mv_block_w,
                           mv_block_h, fine_step, d_window, d_base_out, d_base_offsets, d_enh_out, d_enh_offsets, d_status);
  a.fg = fg_step;
  a.bg = bg_step;
  return split_levels("split_levels", a, nullptr, 0, nullptr, nullptr, d_workspace, workspace_bytes, base_capacity, enh_capacity, stream);
}

// The same order, the ladder in place of the steps: its own rules, every step a multiple of fine_step, the int16 bound on its last
// (coarsest) entry.
int svc_hip_split_levels_budget_frames(const uint8_t* d_frames, uint64_t stream_bytes, const uint64_t* d_frame_offsets, uint32_t n_in,
                                       const uint32_t* d_src, uint32_t n_out, uint32_t frame_w, uint32_t frame_h, uint32_t block_w,
                                       uint32_t block_h, uint32_t mv_block_w, uint32_t mv_block_h, uint32_t fine_step,
                                       const svc_step_pair* ladder, uint32_t ladder_len, const uint32_t* d_budget,
                                       const uint32_t* d_window, uint8_t* d_workspace, uint64_t workspace_bytes, uint8_t* d_base_out,
                                       uint64_t base_capacity, uint64_t* d_base_offsets, uint8_t* d_enh_out, uint64_t enh_capacity,
                                       uint64_t* d_enh_offsets, uint32_t* d_choice, uint32_t* d_status, void* stream) {
  int rc = validate_geom("split_levels_budget", frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if (rc) return rc;
  SVC_REQUIRE(fine_step > 0, "split_levels_budget: quant steps must be positive");
  if ((rc = validate_ladder("split_levels_budget", ladder, ladder_len))) return rc;
  for (uint32_t k = 0; k < ladder_len; ++k)
    SVC_REQUIRE(ladder[k].fg_step % fine_step == 0 && ladder[k].bg_step % fine_step == 0,
                "split_levels_budget: ladder entry %u (%u, %u) must be multiples of fine_step %u", k, ladder[k].fg_step, ladder[k].bg_step,
                fine_step);
  if ((rc = validate_split_steps("split_levels_budget", fine_step, ladder[ladder_len - 1].fg_step, ladder[ladder_len - 1].bg_step))) return rc;
  const SplitArgs a = split_args(d_frames, stream_bytes, d_frame_offsets, n_in, d_src, n_out, frame_w, frame_h, block_w, block_h,
                                 mv_block_w, mv_block_h, fine_step, d_window, d_base_out, d_base_offsets, d_enh_out, d_enh_offsets, d_status);
  return split_levels("split_levels_budget", a, ladder, ladder_len, d_budget, d_choice, d_workspace, workspace_bytes, base_capacity,
                      enh_capacity, stream);
}

uint64_t svc_hip_pack_layers_workspace_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h, uint32_t block_w, uint32_t block_h) {
  // the MV block does not enter the group split: the whole frame stands in for it
  if (validate_geom("pack_layers_workspace_bytes", frame_w, frame_h, block_w, block_h, frame_w, frame_h) ||
      validate_limits("pack_layers_workspace_bytes", n_frames, frame_w, frame_h, block_w, block_h, frame_w, frame_h))
    return 0;
  return layout_bytes(layers_ws, n_frames, make_geom(frame_w, frame_h, block_w, block_h, frame_w, frame_h).groups);
}

// Checked in the order of svc_hip_dct_pack_layers_frames: geometry, steps, the int16 bounds, limits, workspace, both capacities;
// n_frames == 0 then returns SVC_OK; then pointers.
int svc_hip_pack_layers_frames(const float* d_planes, const uint32_t* d_block_types, uint32_t n_frames, uint32_t frame_w, uint32_t frame_h,
                               uint32_t block_w, uint32_t block_h, uint32_t mv_block_w, uint32_t mv_block_h, uint32_t fg_step,
                               uint32_t bg_step, uint32_t enh_step, const uint32_t* d_window, uint8_t* d_workspace,
                               uint64_t workspace_bytes, uint8_t* d_base_out, uint64_t base_capacity, uint64_t* d_base_offsets,
                               uint8_t* d_enh_out, uint64_t enh_capacity, uint64_t* d_enh_offsets, void* stream) {
  int rc = validate_geom("pack_layers", frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if (rc) return rc;
  SVC_REQUIRE(fg_step > 0 && bg_step > 0 && enh_step > 0, "pack_layers: quant steps must be positive");
  // (a step that divides is not above: this also refuses enh_step > min(fg_step, bg_step))
  SVC_REQUIRE(fg_step % enh_step == 0 && bg_step % enh_step == 0, "pack_layers: fg_step %u and bg_step %u must each be a multiple of enh_step %u",
              fg_step, bg_step, enh_step);
  // the pack's int16 bound (Parseval) on the fine levels; the residuals are within ratio / 2 + 1 of zero
  if (255.0 * std::sqrt((double)block_w * block_h) / enh_step > 32767.0)
    return fail(SVC_ERR_UNSUPPORTED, "pack_layers: levels of a %ux%u tile at step %u could exceed int16", block_w, block_h, enh_step);
  if (std::max(fg_step, bg_step) / enh_step > 32766)
    return fail(SVC_ERR_UNSUPPORTED, "pack_layers: a base step of %u is more than 32766 times enh_step %u: a residual could exceed int16",
                std::max(fg_step, bg_step), enh_step);
  if ((rc = validate_limits("pack_layers", n_frames, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h))) return rc;
  const Geom g = make_geom(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if ((rc = require_workspace("pack_layers", workspace_bytes, layout_bytes(layers_ws, n_frames, g.groups)))) return rc;
  const uint64_t need = n_frames * frame_layout(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h).max_bytes;
  if ((rc = require_capacity("pack_layers", "base output", base_capacity, need))) return rc;
  if ((rc = require_capacity("pack_layers", "enhancement output", enh_capacity, need))) return rc;
  if (n_frames == 0) return SVC_OK;  // empty batch: nothing to enqueue
  SVC_REQUIRE(d_planes && d_block_types && d_workspace && d_base_out && d_base_offsets && d_enh_out && d_enh_offsets, "pack_layers: null pointer");
  SVC_REQUIRE(aligned(d_planes, 16) && aligned(d_base_out, 16) && aligned(d_enh_out, 16) && aligned(d_workspace, 16) &&
                  aligned(d_base_offsets, 8) && aligned(d_enh_offsets, 8) && aligned(d_block_types, 4) && aligned(d_window, 4),
              "pack_layers: planes, outputs and workspace must be 16-byte aligned, offsets 8-byte, types and window 4-byte");
  const PackLayersArgs a{g, d_planes, d_block_types, d_window, d_base_out, d_enh_out, d_base_offsets, d_enh_offsets,
                         carve(d_workspace, layers_ws, n_frames, g.groups), n_frames, fg_step, bg_step, enh_step};
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(g.groups, n_frames);
  hipLaunchKernelGGL(pack_layers_kernel<false>, grid, dim3(kThreads), lds_bytes(g), s, a);
  if ((rc = check_launch("pack_layers", "count"))) return rc;
  hipLaunchKernelGGL(pack_layers_scan_kernel, dim3(n_frames), dim3(kThreads), 0, s, g, a.ws, n_frames);
  if ((rc = check_launch("pack_layers", "scan"))) return rc;
  if ((rc = enqueue_frame_offsets("pack_layers", 2, OffsetsJob{a.ws.frame_bytes, d_base_offsets, nullptr},
                                  OffsetsJob{a.ws.frame_bytes + n_frames, d_enh_offsets, nullptr}, n_frames, stream)))
    return rc;
  hipLaunchKernelGGL(pack_layers_kernel<true>, grid, dim3(kThreads), lds_bytes(g), s, a);
  return check_launch("pack_layers", "scatter");
}

uint64_t svc_hip_records_pack_levels_workspace_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h, uint32_t block,
                                                     uint32_t mv_block_w, uint32_t mv_block_h) {
  if (validate_geom("records_pack_levels_workspace_bytes", frame_w, frame_h, block, block, mv_block_w, mv_block_h) ||
      validate_limits("records_pack_levels_workspace_bytes", n_frames, frame_w, frame_h, block, block, mv_block_w, mv_block_h))
    return 0;
  const Geom g = make_geom(frame_w, frame_h, block, block, mv_block_w, mv_block_h);
  return layout_bytes(records_pack_ws, n_frames, g.groups, g.mvb);
}

// Checked in the order of svc_hip_pack_levels_frames, for any n_frames: geometry (with emit_frame_h), steps, the int16 bound, limits,
// then the records' stride, workspace, output capacity; n_frames == 0 then returns SVC_OK; then pointers.  Three launches.
int svc_hip_records_pack_levels_frames(const uint8_t* d_records, uint64_t records_stride_bytes, uint32_t n_frames, uint32_t frame_w,
                                       uint32_t frame_h, uint32_t block, uint32_t emit_frame_h, uint32_t mv_block_w, uint32_t mv_block_h,
                                       uint32_t fg_step, uint32_t bg_step, uint8_t* d_workspace, uint64_t workspace_bytes, uint8_t* d_out,
                                       uint64_t out_capacity, uint64_t* d_frame_offsets, uint32_t* d_status, void* stream) {
  const char* what = "records_pack_levels";
  int rc = validate_geom(what, frame_w, frame_h, block, block, mv_block_w, mv_block_h);
  if (rc) return rc;
  SVC_REQUIRE(emit_frame_h >= 1 && emit_frame_h <= frame_h, "%s: emit_frame_h %u outside [1, %u]", what, emit_frame_h, frame_h);
  SVC_REQUIRE(fg_step > 0 && bg_step > 0, "%s: quant steps must be positive", what);
  // the pack's bound (Parseval on an orthonormal DCT of u8 samples): a stream of such coefficients then never clamps
  if (255.0 * block / std::min(fg_step, bg_step) > 32767.0)
    return fail(SVC_ERR_UNSUPPORTED, "%s: levels of a %ux%u tile at step %u could exceed int16", what, block, block, std::min(fg_step, bg_step));
  if ((rc = validate_limits(what, n_frames, frame_w, frame_h, block, block, mv_block_w, mv_block_h))) return rc;
  const uint64_t per = svc_hip_serialized_frame_bytes(frame_w, emit_frame_h, block, block);
  SVC_REQUIRE(records_stride_bytes % 4 == 0 && records_stride_bytes >= per,
              "%s: records stride %llu must be a multiple of 4 and at least one frame's %llu B", what,
              (unsigned long long)records_stride_bytes, (unsigned long long)per);
  const Geom g = make_geom(frame_w, frame_h, block, block, mv_block_w, mv_block_h);
  if ((rc = require_workspace(what, workspace_bytes, layout_bytes(records_pack_ws, n_frames, g.groups, g.mvb)))) return rc;
  const uint64_t need = n_frames * frame_layout(frame_w, frame_h, block, block, mv_block_w, mv_block_h).max_bytes;
  if ((rc = require_capacity(what, "output", out_capacity, need))) return rc;
  if (n_frames == 0) return SVC_OK;  // empty batch: nothing to enqueue
  SVC_REQUIRE(d_records && d_workspace && d_out && d_frame_offsets && d_status, "%s: null pointer", what);
  SVC_REQUIRE(aligned(d_records, 4) && aligned(d_out, 16) && aligned(d_workspace, 16) && aligned(d_frame_offsets, 8) && aligned(d_status, 4),
              "%s: output and workspace must be 16-byte aligned, offsets 8-byte, records and status 4-byte", what);
  RecordsPackArgs a{};
  a.g = g; a.records = d_records; a.stride = records_stride_bytes;
  a.emit_rows = div_up(emit_frame_h, block); a.rec_dw = 1 + 3 * block * block;
  a.out = d_out; a.offsets = d_frame_offsets; a.d_status = d_status;
  a.ws = carve(d_workspace, records_pack_ws, n_frames, g.groups, g.mvb);
  a.fg = fg_step; a.bg = bg_step;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(g.groups, n_frames);
  const uint32_t cap = (g.tpg * block * block + 1) & ~1u;  // the group's coefficients, as the kernel splits its LDS
  hipLaunchKernelGGL(records_pack_kernel<false>, grid, dim3(kThreads), 0, s, a);
  if ((rc = check_launch(what, "count"))) return rc;
  hipLaunchKernelGGL(scan_kernel<false>, dim3(n_frames), dim3(kThreads), 0, s, g, a.ws.pack, nullptr, 0, nullptr, nullptr);
  if ((rc = check_launch(what, "scan"))) return rc;
  hipLaunchKernelGGL(records_pack_kernel<true>, grid, dim3(kThreads), 2 * cap * sizeof(uint16_t), s, a);
  return check_launch(what, "scatter");
}

uint64_t svc_hip_levels_records_workspace_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h, uint32_t block_w, uint32_t block_h) {
  return svc_hip_pack_levels_workspace_bytes(n_frames, frame_w, frame_h, block_w, block_h);  // the unpack's count and scan
}

// Checked in the order of svc_hip_unpack_levels_frames, for any n_frames: geometry (with the square tile and emit_frame_h), limits,
// then the records' stride, workspace; n_frames == 0 then returns SVC_OK; then pointers.  Three launches.
int svc_hip_levels_records_frames(const uint8_t* d_frames, uint64_t stream_bytes, const uint64_t* d_frame_offsets, uint32_t n_frames,
                                  uint32_t frame_w, uint32_t frame_h, uint32_t block_w, uint32_t block_h, uint32_t mv_block_w,
                                  uint32_t mv_block_h, uint32_t emit_frame_h, uint8_t* d_workspace, uint64_t workspace_bytes,
                                  uint8_t* d_records, uint64_t records_stride_bytes, uint32_t* d_status, void* stream) {
  const char* what = "levels_records";
  int rc = validate_geom(what, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if (rc) return rc;
  if (block_w != block_h)
    return fail(SVC_ERR_UNSUPPORTED, "%s: non-square tiles %ux%u (a record's rows and columns are those of a square tile)", what, block_w, block_h);
  SVC_REQUIRE(emit_frame_h >= 1 && emit_frame_h <= frame_h, "%s: emit_frame_h %u outside [1, %u]", what, emit_frame_h, frame_h);
  if ((rc = validate_limits(what, n_frames, frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h))) return rc;
  const uint64_t per = svc_hip_serialized_frame_bytes(frame_w, emit_frame_h, block_w, block_h);
  SVC_REQUIRE(records_stride_bytes % 4 == 0 && records_stride_bytes >= per,
              "%s: records stride %llu must be a multiple of 4 and at least one frame's %llu B", what,
              (unsigned long long)records_stride_bytes, (unsigned long long)per);
  const Geom g = make_geom(frame_w, frame_h, block_w, block_h, mv_block_w, mv_block_h);
  if ((rc = require_workspace(what, workspace_bytes, layout_bytes(stream_ws, n_frames, g.groups)))) return rc;
  if (n_frames == 0) return SVC_OK;
  SVC_REQUIRE(d_frames && d_frame_offsets && d_workspace && d_records && d_status, "%s: null pointer", what);
  SVC_REQUIRE(aligned(d_frames, 16) && aligned(d_workspace, 16) && aligned(d_frame_offsets, 8) && aligned(d_records, 4) && aligned(d_status, 4),
              "%s: frames and workspace must be 16-byte aligned, offsets 8-byte, records and status 4-byte", what);
  const LevelsRecordsArgs a{{g, d_frames, stream_bytes, d_frame_offsets, nullptr, nullptr, carve(d_workspace, stream_ws, n_frames, g.groups)},
                            d_records, records_stride_bytes, 1 + 3 * block_w * block_h};
  hipStream_t s = static_cast<hipStream_t>(stream);
  if ((rc = enqueue_unpack_scan(what, a.u, n_frames, d_status, s))) return rc;
  hipLaunchKernelGGL(levels_records_kernel, dim3(div_up(emit_frame_h, block_h) * g.gx, n_frames), dim3(kThreads), 0, s, a);
  return check_launch(what, "records");
}

int svc_hip_gaze_rect(uint32_t cx, uint32_t cy, uint32_t max_w, uint32_t max_h, uint32_t frame_w, uint32_t frame_h, uint32_t padded_w,
                      uint32_t padded_h, uint32_t out_xywh[4]) {
  SVC_REQUIRE(frame_w > 0 && frame_h > 0 && padded_w > 0 && padded_h > 0, "gaze_rect: frame sides must be positive");
  SVC_REQUIRE(cx < frame_w && cy < frame_h, "gaze_rect: centre (%u, %u) outside the %ux%u frame (libs/decoder.cpp:71-75 asserts)", cx,
              cy, frame_w, frame_h);
  SVC_REQUIRE(out_xywh, "gaze_rect: null pointer");
  // CalcWithinFrameRectFromCenter, libs/decoder.cpp:65-100 (unsigned arithmetic, as there)
  uint32_t half_w = (max_w + 1) / 2;
  if (cx + half_w >= frame_w) half_w = frame_w - cx - 1;
  if (cx < half_w) half_w = cx;
  uint32_t half_h = (max_h + 1) / 2;
  if (cy + half_h >= frame_h) half_h = frame_h - cy - 1;
  if (cy < half_h) half_h = cy;
  const uint32_t tl_x = cx - half_w, tl_y = cy - half_h, br_x = cx + half_w, br_y = cy + half_h;
  // to the padded frame: f32 ratios, RoundFloatToInt (libs/decoder.cpp:163-164, :179-183; libs/math.hpp:15-18)
  const float w_ratio = (float)padded_w / (float)frame_w, h_ratio = (float)padded_h / (float)frame_h;
  out_xywh[0] = (uint32_t)(int)std::round((float)tl_x * w_ratio);
  out_xywh[1] = (uint32_t)(int)std::round((float)tl_y * h_ratio);
  out_xywh[2] = (uint32_t)(int)std::round((float)(br_x - tl_x) * w_ratio);
  out_xywh[3] = (uint32_t)(int)std::round((float)(br_y - tl_y) * h_ratio);
  return SVC_OK;
}

}  // extern "C"
