// luma_pyramid.hip -- the step in front of the motion search: luma extraction and
// the Gaussian pyramid, on the device, so a frame crosses PCIe once as BGR u8 and
// its pyramid (also the RCCL halo payload) never leaves HBM.
//
// Stands in for cv::cvtColor(BGR2YUV) + cv::extractChannel + cv::buildPyramid
// (reference libs/encoder.cpp:468-470).  OpenCV is not available offline, so these
// are this repo's own fixed-point definitions (scalable_video_codec_amd/synth.py holds
// the same definitions in torch and is what the parity tests compare with):
//   Y      = (1868 B + 9617 G + 4899 R + 8192) >> 14
//   level+1 = 5x5 [1 4 6 4 1]^2 kernel at even samples, BORDER_REFLECT_101,
//            (sum + 128) >> 8
// Both are HBM-bound byte work: 3 B in / 1 B out, then 1 B in / 0.25 B out.
#include "luma16.hpp"
#include "svc_common.hpp"

namespace svc {

struct LumaArgs {
  const uint8_t* bgr;
  uint64_t frame_stride;
  uint8_t* pyr;
  uint64_t pyr_stride;
  uint32_t groups_per_frame;  // W * H / 16
  uint32_t total_groups;
};

// one lane: 16 pixels = 48 B in (3 x dwordx4), 16 B out (1 x dwordx4)
__global__ __launch_bounds__(256) void luma_kernel(LumaArgs a) {
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g >= a.total_groups) return;
  const uint32_t frame = g / a.groups_per_frame, gi = g - frame * a.groups_per_frame;
  const uint4* src = reinterpret_cast<const uint4*>(a.bgr + (size_t)frame * a.frame_stride + (size_t)gi * 48);
  const uint4 v0 = src[0], v1 = src[1], v2 = src[2];
  const uint32_t w[12] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w};
  uint32_t out[4];
  luma16(w, out);
  uint4* dst = reinterpret_cast<uint4*>(a.pyr + (size_t)frame * a.pyr_stride + (size_t)gi * 16);
  *dst = make_uint4(out[0], out[1], out[2], out[3]);
}

typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

struct PyrDownArgs {
  uint8_t* pyr;
  uint64_t pyr_stride;
  uint64_t src_off, dst_off;  // plane offsets inside a packed pyramid
  uint32_t sw, sh;            // source plane size
  uint32_t dw, dh;            // destination plane size (sw/2, sh/2)
  uint32_t quads_per_row;     // ceil(dw / 4)
  uint32_t total;             // frames * ceil(dh / 2) * quads_per_row
  uint32_t bytewise;          // source or destination rows are not whole dwords (sw % 4 or dw % 4): every quad gathers and
                              // stores byte by byte -- the top level of a 4-level pyramid of a frame 16 mod 32 pixels wide
                              // (PAL's 720 -> 90, 1360 -> 170, QCIF's 176 -> 22), which the reference's default build produces
};

__device__ __forceinline__ int reflect101(int i, int n) {
  i = i < 0 ? -i : i;
  return i >= n ? 2 * (n - 1) - i : i;
}

// One lane: 4 destination pixels of TWO consecutive rows (two dword stores) from a 7 x 11 source
// patch -- the rows share 3 of their 5 source rows, so 7 unaligned dwordx4 loads, all in flight
// together, feed 8 outputs.  Taps 1 4 6 4 of an output are one 4 x u8 dot product over the dword that
// starts at its first tap, the fifth tap rides in as the accumulator.  The first and last quad of a row
// reflect (BORDER_REFLECT_101) and gather their bytes one by one -- 2 lanes in 120 at the level this
// runs on, in the same launch.
__global__ __launch_bounds__(256) void pyr_down_kernel(PyrDownArgs a) {
  // consecutive output rows share source rows: keep them on one XCD's L2
  const uint32_t q = xcd_contiguous_block(blockIdx.x, gridDim.x) * 256u + threadIdx.x;
  if (q >= a.total) return;
  const uint32_t pairs = (a.dh + 1) / 2, per_frame = pairs * a.quads_per_row;
  const uint32_t frame = q / per_frame, rem = q - frame * per_frame;
  const uint32_t dp = rem / a.quads_per_row, dq = rem - dp * a.quads_per_row;
  const uint32_t dy = 2 * dp;
  const uint8_t* src = a.pyr + (size_t)frame * a.pyr_stride + a.src_off;
  const int sx0 = (int)dq * 8;  // source column of the first output's centre
  const bool border = dq == 0 || dq + 1 == a.quads_per_row || a.bytewise != 0;

  uint32_t acc0[4] = {0, 0, 0, 0}, acc1[4] = {0, 0, 0, 0};
  const uint32_t taps[5] = {1, 4, 6, 4, 1};
  const uint8_t* rows[7];
#pragma unroll
  for (int r = 0; r < 7; ++r)  // rows past the plane only feed the (discarded) second output of an odd last pair
    rows[r] = src + (size_t)reflect101(min((int)dy * 2 + r - 2, 2 * (int)a.sh - 2), (int)a.sh) * a.sw;
  constexpr uint32_t kTaps = 1u | (4u << 8) | (6u << 16) | (4u << 24);

  uint32_t h[7][4];
  if (!border) {
    u32x4_a4 w[7];
#pragma unroll
    for (int r = 0; r < 7; ++r) w[r] = *reinterpret_cast<const u32x4_a4*>(rows[r] + sx0 - 4);
#pragma unroll
    for (int r = 0; r < 7; ++r) {
      const uint32_t w0 = w[r].x, w1 = w[r].y, w2 = w[r].z, w3 = w[r].w;  // source columns sx0 - 4 .. sx0 + 11
      h[r][0] = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(w1, w0, 2), kTaps, (w1 >> 16) & 0xFFu, false);
      h[r][1] = __builtin_amdgcn_udot4(w1, kTaps, w2 & 0xFFu, false);
      h[r][2] = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(w2, w1, 2), kTaps, (w2 >> 16) & 0xFFu, false);
      h[r][3] = __builtin_amdgcn_udot4(w2, kTaps, w3 & 0xFFu, false);
    }
  } else {
#pragma unroll
    for (int r = 0; r < 7; ++r) {
      uint32_t px[11];
#pragma unroll
      for (int i = 0; i < 11; ++i)  // (clamped: columns past a partial last quad only feed outputs that are not stored)
        px[i] = rows[r][min(max(reflect101(sx0 - 2 + i, (int)a.sw), 0), (int)a.sw - 1)];
#pragma unroll
      for (int o = 0; o < 4; ++o) h[r][o] = px[2 * o] + 4 * px[2 * o + 1] + 6 * px[2 * o + 2] + 4 * px[2 * o + 3] + px[2 * o + 4];
    }
  }
#pragma unroll
  for (int r = 0; r < 7; ++r)
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      if (r < 5) acc0[o] += taps[r] * h[r][o];
      if (r >= 2) acc1[o] += taps[r - 2] * h[r][o];
    }
  uint32_t out0 = 0, out1 = 0;
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    out0 |= ((acc0[o] + 128u) >> 8) << (8 * o);
    out1 |= ((acc1[o] + 128u) >> 8) << (8 * o);
  }
  uint8_t* dst = a.pyr + (size_t)frame * a.pyr_stride + a.dst_off;
  if (a.bytewise) {  // rows are not whole dwords: the row's last quad may be partial, and no store is dword-aligned
    const uint32_t n = min(4u, a.dw - dq * 4);
    for (uint32_t o = 0; o < n; ++o) {
      dst[(size_t)dy * a.dw + dq * 4 + o] = (uint8_t)(out0 >> (8 * o));
      if (dy + 1 < a.dh) dst[(size_t)(dy + 1) * a.dw + dq * 4 + o] = (uint8_t)(out1 >> (8 * o));
    }
    return;
  }
  *reinterpret_cast<uint32_t*>(dst + (size_t)dy * a.dw + dq * 4) = out0;
  if (dy + 1 < a.dh) *reinterpret_cast<uint32_t*>(dst + (size_t)(dy + 1) * a.dw + dq * 4) = out1;
}

// ---- luma + first pyramid level in one pass over the BGR frame -------------------------
// A workgroup owns a 128 x 32 tile of the luma plane.  (Taller / wider tiles -- 128 x 60, 256 x 60 --
// run no faster and push the tiles in flight per XCD past its L2, so the halo re-reads start to
// miss: FETCH_SIZE 2.37 GB against 1.85 GB with this shape, which is the algorithmic figure.)  Its lanes compute Y for the tile plus
// a 2-pixel halo (reflect-101 at the frame border, exactly what pyr_down_kernel does) into
// LDS, store the interior to the level-0 plane, and then each lane produces 4 level-1 pixels
// from the LDS copy.  Versus luma_kernel + pyr_down_kernel this removes the re-read of the
// whole luma plane and one launch; the halo rows cost 12.5 % more BGR reads, served from L2.
constexpr int kTW = 128, kTH = 32, kOff = 16, kPitch = kTW + 2 * kOff;  // LDS column c <-> x = x0 - kOff + c
static_assert(kPitch % 16 == 0 && kOff % 16 == 0, "LDS rows keep 16-byte alignment for the ds_write_b128");

struct LumaPyr1Args {
  const uint8_t* bgr;  // interleaved frames
  uint64_t frame_stride;
  uint8_t* pyr;
  uint64_t pyr_stride;
  uint64_t src_off;  // unused; kept so that the fields after it keep their kernel-argument offsets
  uint64_t dst_off;  // offset of level 1 inside a packed pyramid (w * h)
  uint32_t w, h;     // the frame
  uint32_t tiles_x, tiles_per_frame, total_tiles;
};

__device__ __forceinline__ uint32_t luma_of(uint32_t b, uint32_t g, uint32_t r) {
  return (1868u * b + 9617u * g + 4899u * r + 8192u) >> 14;
}

// Tile t: luma from the B,G,R frame -> level 0 (stored) -> level 1.
__device__ __forceinline__ void luma_pyr1_tile(const LumaPyr1Args& a, uint32_t t, uint8_t* tile) {
  const uint32_t tid = threadIdx.x;
  const uint32_t frame = t / a.tiles_per_frame, tr = t - frame * a.tiles_per_frame;
  const uint32_t ty = tr / a.tiles_x, tx = tr - ty * a.tiles_x;
  const int x0 = (int)tx * kTW, y0 = (int)ty * kTH;
  const int w = (int)a.w, h = (int)a.h;
  const int segs = min(kTW, w - x0) / 16;  // 16-pixel segments of this tile inside the frame
  const int xe = x0 + segs * 16;           // first column right of the tile's valid part
  const uint8_t* src = a.bgr + (size_t)frame * a.frame_stride;
  uint8_t* y_plane = a.pyr + (size_t)frame * a.pyr_stride;

  // Rows past y = h are never needed (the last output row is centred on h - 2, its taps end at
  // row h) and must not be touched: reflect101 folds once, so a row further out would index
  // outside the frame (short frames: found by tests/test_gpu_misc_property.py).
  const int rows = min(kTH + 4, h - y0 + 3);  // LDS rows 0 .. rows-1 <-> y = y0 - 2 .. min(y0 + 33, h)
  // (a) segment tasks: 16 pixels of one row -> 4 dwords of LDS (+ the level-0 store)
  for (int task = (int)tid; task < rows * segs; task += 256) {
    const int r = task / segs, sgm = task - r * segs;
    const int y = y0 - 2 + r, yr = reflect101(y, h);
    const int x = x0 + sgm * 16;
    const uint4* p = reinterpret_cast<const uint4*>(src + ((size_t)yr * w + x) * 3);
    const uint4 v0 = p[0], v1 = p[1], v2 = p[2];
    const uint32_t wd[12] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, v2.x, v2.y, v2.z, v2.w};
    uint32_t out[4];
    luma16(wd, out);
    const uint4 o4 = make_uint4(out[0], out[1], out[2], out[3]);
    *reinterpret_cast<uint4*>(&tile[r * kPitch + kOff + sgm * 16]) = o4;  // 16-byte aligned (Guideline 17)
    if (r >= 2 && r < kTH + 2 && y < h) *reinterpret_cast<uint4*>(y_plane + (size_t)y * w + x) = o4;
  }
  // (b) halo pixels: two columns on each side of the valid part, every row, three byte loads each.  (By the lanes that hold a row's
  // first / last segment, one more 16-byte load each: 3 - 5 % slower; one unaligned dword per pixel: 2 - 4 % slower at C3,
  // profiles/r06_ab_luma_halo.txt.)
  for (int task = (int)tid; task < rows * 4; task += 256) {
    const int r = task >> 2, k = task & 3;
    const int yr = reflect101(y0 - 2 + r, h);
    const int x = k < 2 ? x0 - 2 + k : xe + (k - 2);
    const uint8_t* p = src + ((size_t)yr * w + reflect101(x, w)) * 3;
    tile[r * kPitch + kOff + (x - x0)] = (uint8_t)luma_of(p[0], p[1], p[2]);
  }
  __syncthreads();

  // (c) level 1 from the tile (LDS column kOff + c <-> x = x0 + c, row r <-> y = y0 - 2 + r): a task = a quad of 4 output columns of one
  // output row.  (Tasks of 2 / 4 output rows that share source rows, on round 5's plane-to-plane pass: 0.266-0.275 / 0.324-0.326 against
  // 0.273-0.282 ms, profiles/r05_ab_plane_rpt.txt: the pass is not bound by its instruction count.)
  constexpr int kQuads = kTW / 8;  // quads of output columns per tile row
  constexpr uint32_t kTaps = 1u | (4u << 8) | (6u << 16) | (4u << 24);
  constexpr int taps[5] = {1, 4, 6, 4, 1};
  for (int task = (int)tid; task < kQuads * (kTH / 2); task += 256) {
    const int q = task % kQuads, oy = task / kQuads;
    const int gx = (x0 >> 1) + 4 * q, gy = (y0 >> 1) + oy;  // output-level coordinates
    if (gx >= (w >> 1) || gy >= (h >> 1)) continue;
    uint32_t acc[4] = {0, 0, 0, 0};
#pragma unroll
    for (int r = 0; r < 5; ++r) {
      // centre of output column 4q + o is LDS column kOff + 8q + 2o; taps span kOff + 8q - 2 .. + 8
      const uint8_t* rowp = &tile[(2 * oy + r) * kPitch + kOff + 8 * q];
      const uint32_t w0 = *reinterpret_cast<const uint32_t*>(rowp - 4);
      const uint2 mid = *reinterpret_cast<const uint2*>(rowp);
      const uint32_t w3 = *reinterpret_cast<const uint32_t*>(rowp + 8);
      // taps 1 4 6 4 of an output are one 4 x u8 dot product over the dword that starts at its first tap;
      // the fifth tap (weight 1) enters as the accumulator
      const uint32_t h0 = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(mid.x, w0, 2), kTaps, (mid.x >> 16) & 0xFFu, false);
      const uint32_t h1 = __builtin_amdgcn_udot4(mid.x, kTaps, mid.y & 0xFFu, false);
      const uint32_t h2 = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(mid.y, mid.x, 2), kTaps, (mid.y >> 16) & 0xFFu, false);
      const uint32_t h3 = __builtin_amdgcn_udot4(mid.y, kTaps, w3 & 0xFFu, false);
      acc[0] += (uint32_t)taps[r] * h0;
      acc[1] += (uint32_t)taps[r] * h1;
      acc[2] += (uint32_t)taps[r] * h2;
      acc[3] += (uint32_t)taps[r] * h3;
    }
    // (a loop of one trip around a row check the `continue` above has already made: in this shape the pass compiles to the instructions
    // that were measured; written straight, the same instructions are scheduled differently)
#pragma unroll
    for (int o = 0; o < 1; ++o) {
      if (gy + o >= (h >> 1)) break;
      uint32_t out = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) out |= ((acc[k] + 128u) >> 8) << (8 * k);
      *reinterpret_cast<uint32_t*>(y_plane + a.dst_off + (size_t)gy * (w >> 1) + gx) = out;
    }
  }
}

// One tile per workgroup (76 500 workgroups at C3).
__global__ __launch_bounds__(256) void luma_pyr1_kernel(LumaPyr1Args a) {
  // (+ 16 bytes that are never touched: the LDS allocation the kernel was measured with)
  __shared__ __attribute__((aligned(16))) uint8_t tile[(kTH + 4) * kPitch + 16];
  const uint32_t t = xcd_contiguous_block(blockIdx.x, gridDim.x);
  if (t < a.total_tiles) luma_pyr1_tile(a, t, tile);
}

// ---- plane -> next level, a wave per column strip, no LDS (round 6) ---------------------------------------------------
// Round 5's LDS-tiled plane pass spent its time on arithmetic and LDS, not on bytes (24 vector instructions per output pixel,
// LDS busy 39 % of a CU's time with 16 M of 41 M cycles bank conflicts: profiles/r05_pmc_C3_sq_tcp_summary.csv).  Here a WAVE owns
// a strip of 512 source columns (lane i: columns 8i .. 8i + 7, one dwordx2 per source row) and walks OB output rows down it:
//   * vertical first, two columns per instruction: a source dword is split once into its even and odd bytes as pairs of u16
//     (E = bytes 0, 2; O = bytes 1, 3) and the 1 4 6 4 1 column sums run on the pairs (<= 4088 each, with the rounding constant
//     folded in as + 8).  Output row oy needs rows 2 oy - 2 .. 2 oy + 2: with S = r[2 oy - 2] + 4 r[2 oy - 1] carried from the
//     previous row, V = S + 6 r[2 oy] + (4 r[2 oy + 1] + r[2 oy + 2]) is four instructions per pair register and no row is kept;
//   * horizontal on the column sums, still in pairs: the two outputs centred on a dword's bytes 0 and 2 are
//     6 E + 4 (O' + O) + (E' + E'') where ' / '' are E, O shifted by one u16 across the neighbouring dword (v_alignbyte) --
//     <= 65 408, so a pair of u16 never carries; the result bytes are bytes 1 and 3 of the sums (the >> 8), picked by one v_perm;
//   * the neighbouring lane's registers arrive by DPP wave shifts; the strip's own neighbours (two column sums left, one right;
//     reflected at the plane's border) come from one more dword per row, loaded by lane 0 and the strip's last lane
//     (lane 0: the dword left of the strip, the strip's last lane: the dword right of it).
// No LDS, no barrier, 2 x 8 + 4 bytes in flight per lane and row.  (Bands of a strip on consecutive waves, 4 / 12 / 16 output rows per
// wave: within 3 %; non-temporal loads and stores: no gain -- profiles/r06_ab_pyr_strip.txt sections 5, 6.)
struct PyrStripArgs {
  uint8_t* pyr;
  uint64_t pyr_stride, src_off, dst_off;
  uint32_t sw, sh;  // source plane; sw % 8 == 0, sh % 2 == 0, sh >= 4
  uint32_t strips, bands, total_waves;
};

typedef uint16_t u16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_mad(uint32_t a, uint16_t k, uint32_t c) {  // v_pk_mad_u16
  return __builtin_bit_cast(uint32_t, (u16x2_t)(__builtin_bit_cast(u16x2_t, a) * k + __builtin_bit_cast(u16x2_t, c)));
}

template <int OB>
__global__ __launch_bounds__(256) void pyr_strip_kernel(PyrStripArgs a, const uint8_t* __restrict__ pyr_in, uint8_t* __restrict__ pyr_out) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wv = __builtin_amdgcn_readfirstlane(xcd_contiguous_block(blockIdx.x, gridDim.x) * 4u + (threadIdx.x >> 6));
  if (wv >= a.total_waves) return;
  // consecutive waves: the strips of one band side by side -- a workgroup's four waves read whole rows of a 1080p plane, one contiguous run
  const uint32_t strip = wv % a.strips, t = wv / a.strips, band = t % a.bands, frame = t / a.bands;
  const int w = (int)a.sw, h = (int)a.sh, dw = w >> 1, dh = h >> 1;
  const int x0 = (int)strip * 512, valid = min(512, w - x0), la = valid / 8 - 1, xe = x0 + valid;
  const int oy0 = (int)band * OB, rows = min(OB, dh - oy0);
  const uint8_t* src = pyr_in + (size_t)frame * a.pyr_stride + a.src_off;  // the source plane is only read, the destination plane only
  uint8_t* dst = pyr_out + (size_t)frame * a.pyr_stride + a.dst_off;       // written, and they do not overlap: __restrict__ holds

  const uint32_t col = (uint32_t)x0 + min(lane, (uint32_t)la) * 8u;
  const bool last = lane == (uint32_t)la;
  // the strip's neighbours as a pair H = (lo, hi) of u16: left of it the columns (x0 - 2, x0 - 1) -- bytes 2, 3 of the dword in front of the
  // strip, reflected (columns 2, 1: bytes 2, 1 of the strip's first dword) at the plane's left border; right of it column xe in lo -- byte 0 of
  // the dword behind the strip, reflected (column w - 2: byte 2 of the plane's last dword) at the right border
  const uint32_t hcol_l = x0 ? (uint32_t)x0 - 4u : 0u, hcol_r = xe < w ? (uint32_t)xe : (uint32_t)w - 4u;
  const uint32_t hsel_l = x0 ? 0x0c030c02u : 0x0c010c02u, hsel_r = xe < w ? 0x0c0c0c00u : 0x0c0c0c02u;  // v_perm selectors; 0x0c = a zero byte
  uint32_t hcol = col, hsel = 0x0c0c0c0cu;
  if (lane == 0) { hcol = hcol_l; hsel = hsel_l; }
  if (last) { hcol = hcol_r; hsel = hsel_r; }

  // a source row -> its pair registers (E = bytes 0, 2; O = bytes 1, 3 of each dword)
  struct Row { uint32_t e0, o0, e1, o1; };
  auto row_offset = [&](int r) { return (uint32_t)reflect101(min(2 * oy0 - 2 + r, h), h) * (uint32_t)w; };  // wave-uniform; a plane is < 4 GB
  auto split = [&](const uint2& v) {
    Row r;
    r.e0 = v.x & 0x00FF00FFu; r.o0 = __builtin_amdgcn_perm(0u, v.x, 0x0c030c01u);
    r.e1 = v.y & 0x00FF00FFu; r.o1 = __builtin_amdgcn_perm(0u, v.y, 0x0c030c01u);
    return r;
  };

  // every source row of the band is requested before the first is used (2 OB + 3 rows in flight: a version that walked the band with two
  // rows of prefetch measured level with the LDS-tiled pass it replaces); straight-line code, so the compiler's waits are exact and rows are
  // consumed as they land
  constexpr int kRows = 2 * OB + 3;
  uint2 rv[kRows];
  // the neighbours' pair per row (lane 0 and the last lane): the extra dword under the exec mask of the two lanes that need it, in one block
  // in front of the rows.  (Loaded by all 64 lanes, or by two scalar loads per row with the column sums on the scalar unit: 0.2180 and
  // 0.2168 against 0.2050 ms alone over a C3-sized clip, profiles/r06_ab_pyr_strip.txt section 9.)
  uint32_t hh[kRows];
#pragma unroll
  for (int r = 0; r < kRows; ++r) hh[r] = 0;
  if (lane == 0 || last) {
#pragma unroll
    for (int r = 0; r < kRows; ++r) hh[r] = *reinterpret_cast<const uint32_t*>(src + row_offset(r) + hcol);
  }
#pragma unroll
  for (int r = 0; r < kRows; ++r) hh[r] = __builtin_amdgcn_perm(0u, hh[r], hsel);
#pragma unroll
  for (int r = 0; r < kRows; ++r)  // rows past the band's last output (and past the plane: clamped) are loaded and not used
    rv[r] = *reinterpret_cast<const uint2*>(src + row_offset(r) + col);

  // column sums, two columns per register: V(oy) = s + 6 e + (4 o + n) with s = r[2 oy - 2] + 4 r[2 oy - 1] + 8 carried, e = r[2 oy],
  // o = r[2 oy + 1], n = r[2 oy + 2] (plain 32-bit adds where no pair can carry: v_add3_u32)
  constexpr uint32_t k8 = 0x00080008u;
  Row s, e;
  uint32_t s_h, e_h;  // the same for the neighbours' pair
  {
    const Row r0 = split(rv[0]), r1 = split(rv[1]);
    e = split(rv[2]);
    s.e0 = (r1.e0 << 2) + r0.e0 + k8; s.o0 = (r1.o0 << 2) + r0.o0 + k8;
    s.e1 = (r1.e1 << 2) + r0.e1 + k8; s.o1 = (r1.o1 << 2) + r0.o1 + k8;
    s_h = (hh[1] << 2) + hh[0] + k8; e_h = hh[2];
  }
  uint8_t* out = dst + (size_t)oy0 * dw + (x0 >> 1) + 4 * lane;
  const bool mine = lane <= (uint32_t)la;
#pragma unroll
  for (int i = 0; i < OB; ++i) {
    const Row o = split(rv[3 + 2 * i]), n = split(rv[4 + 2 * i]);
    Row v;
    { const uint32_t q = o.e0 << 2; v.e0 = pk_mad(e.e0, 6, s.e0) + q + n.e0; s.e0 = q + e.e0 + k8; }
    { const uint32_t q = o.o0 << 2; v.o0 = pk_mad(e.o0, 6, s.o0) + q + n.o0; s.o0 = q + e.o0 + k8; }
    { const uint32_t q = o.e1 << 2; v.e1 = pk_mad(e.e1, 6, s.e1) + q + n.e1; s.e1 = q + e.e1 + k8; }
    { const uint32_t q = o.o1 << 2; v.o1 = pk_mad(e.o1, 6, s.o1) + q + n.o1; s.o1 = q + e.o1 + k8; }
    e = n;
    // the neighbours' column sums: (V[x0 - 2], V[x0 - 1]) for lane 0, (V[xe], -) for the last lane
    uint32_t v_h;
    { const uint32_t q = hh[3 + 2 * i] << 2; v_h = pk_mad(e_h, 6, s_h) + q + hh[4 + 2 * i]; s_h = q + e_h + k8; e_h = hh[4 + 2 * i]; }
    // neighbours: the previous lane's second dword (lane 0: the strip's left neighbours), the next lane's first dword (last lane: the right one)
    const uint32_t pe = __builtin_amdgcn_update_dpp(v_h << 16, v.e1, 0x138, 0xf, 0xf, false);  // wave_shr:1; lane 0 keeps `old`
    const uint32_t po = __builtin_amdgcn_update_dpp(v_h, v.o1, 0x138, 0xf, 0xf, false);
    uint32_t ne = __builtin_amdgcn_update_dpp(v_h, v.e0, 0x130, 0xf, 0xf, false);  // wave_shl:1
    ne = last ? v_h : ne;
    // outputs centred on columns 0, 2 (dword 0) and 4, 6 (dword 1) of the lane
    const uint32_t l2a = __builtin_amdgcn_alignbyte(v.e0, pe, 2), l1a = __builtin_amdgcn_alignbyte(v.o0, po, 2);
    const uint32_t mid = __builtin_amdgcn_alignbyte(v.e1, v.e0, 2), l1b = __builtin_amdgcn_alignbyte(v.o1, v.o0, 2);
    const uint32_t r2b = __builtin_amdgcn_alignbyte(ne, v.e1, 2);
    const uint32_t qa = pk_mad(v.e0, 6, ((l1a + v.o0) << 2) + l2a + mid);
    const uint32_t qb = pk_mad(v.e1, 6, ((l1b + v.o1) << 2) + mid + r2b);
    const uint32_t px = __builtin_amdgcn_perm(qb, qa, 0x07050301u);  // (>> 8) of the four sums
    if (mine && i < rows) *reinterpret_cast<uint32_t*>(out) = px;  // (the plane's last band may be short)
    out += dw;
  }
}

// any frame width: one pixel per lane
__global__ __launch_bounds__(256) void luma_any_kernel(const uint8_t* bgr, uint64_t frame_stride, uint8_t* pyr, uint64_t pyr_stride,
                                                        uint32_t px_per_frame, uint32_t total) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= total) return;
  const uint32_t frame = i / px_per_frame, p = i - frame * px_per_frame;
  const uint8_t* s = bgr + (size_t)frame * frame_stride + (size_t)p * 3;
  pyr[(size_t)frame * pyr_stride + p] = (uint8_t)luma_of(s[0], s[1], s[2]);
}

int launch_luma_pyramid(const uint8_t* d_bgr, uint64_t frame_stride, uint32_t n_frames, uint32_t w,
                        uint32_t h, uint32_t levels, uint8_t* d_pyr, uint64_t pyr_stride,
                        hipStream_t stream) {
  if (n_frames == 0) return SVC_OK;
  if (w % 16 != 0) {
    // Frames that are not whole 16-pixel segments wide (8 x 8 MV blocks pad to multiples of 8: --mv-block-w 8 on a 360-pixel
    // frame): a pixel per lane for the luma plane, then the plane-to-plane kernels.  Not the roofline path.
    const uint64_t px = (uint64_t)w * h, tot = px * n_frames;
    if (tot > 0x7FFFFFFFull) return fail(SVC_ERR_UNSUPPORTED, "luma: too many pixels for one launch");
    hipLaunchKernelGGL(luma_any_kernel, dim3((uint32_t)((tot + 255) / 256)), dim3(256), 0, stream, d_bgr, frame_stride, d_pyr,
                       pyr_stride, (uint32_t)px, (uint32_t)tot);
    int rc0 = check_launch("luma_any_kernel");
    if (rc0) return rc0;
    return launch_pyr_down_levels(d_pyr, pyr_stride, n_frames, w, h, levels, 0, stream);
  }
  LumaArgs la;
  la.bgr = d_bgr;
  la.frame_stride = frame_stride;
  la.pyr = d_pyr;
  la.pyr_stride = pyr_stride;
  la.groups_per_frame = (uint32_t)(((uint64_t)w * h) / 16);
  const uint64_t tg = (uint64_t)la.groups_per_frame * n_frames;
  if (tg > 0x7FFFFFFFull) return fail(SVC_ERR_UNSUPPORTED, "luma: too many pixels for one launch");
  la.total_groups = (uint32_t)tg;
  int rc;
  uint32_t first_plain_level = 0;
  // level-1 width must be a multiple of 4 for the fused kernel's dword stores
  if (levels >= 2 && (w / 2) % 4 == 0 && h % 2 == 0) {
    LumaPyr1Args fa{};
    fa.bgr = d_bgr;
    fa.frame_stride = frame_stride;
    fa.pyr = d_pyr;
    fa.pyr_stride = pyr_stride;
    fa.dst_off = (uint64_t)w * h;
    fa.w = w; fa.h = h;
    fa.tiles_x = div_up(w, kTW);
    fa.tiles_per_frame = fa.tiles_x * div_up(h, kTH);
    const uint64_t tt = (uint64_t)fa.tiles_per_frame * n_frames;
    if (tt > 0x7FFFFFFFull) return fail(SVC_ERR_UNSUPPORTED, "luma: too many tiles for one launch");
    fa.total_tiles = (uint32_t)tt;
    // (the same tile with its B,G,R rows brought in by LDS-DMA -- one wait per workgroup instead of three -- measured level: serial 0.551-0.558
    // against 0.557-0.565 ms, pipelined 0.590-0.600 against 0.575-0.582 at C3, level at C5; profiles/r05_ab_luma_dma.txt; removed)
    hipLaunchKernelGGL(luma_pyr1_kernel, dim3(fa.total_tiles), dim3(256), 0, stream, fa);
    if ((rc = check_launch("luma_pyr1_kernel"))) return rc;
    first_plain_level = 1;
  } else {
    hipLaunchKernelGGL(luma_kernel, dim3(div_up(la.total_groups, 256)), dim3(256), 0, stream, la);
    if ((rc = check_launch("luma_kernel"))) return rc;
  }

  return launch_pyr_down_levels(d_pyr, pyr_stride, n_frames, w, h, levels, first_plain_level, stream);
}

// Levels first_plain_level + 1 .. levels - 1 of n_frames packed pyramids whose levels 0 .. first_plain_level exist
// (cv::buildPyramid from a given level-0 plane is first_plain_level = 0: svc_hip_build_pyramid_host).
int launch_pyr_down_levels(uint8_t* d_pyr, uint64_t pyr_stride, uint32_t n_frames, uint32_t w, uint32_t h, uint32_t levels,
                           uint32_t first_plain_level, hipStream_t stream) {
  int rc;
  uint64_t off = 0;
  for (uint32_t l = 0; l + 1 < levels; ++l) {
    PyrDownArgs pa;
    pa.pyr = d_pyr;
    pa.pyr_stride = pyr_stride;
    pa.sw = w >> l; pa.sh = h >> l;
    pa.dw = pa.sw / 2; pa.dh = pa.sh / 2;
    pa.src_off = off;
    off += (uint64_t)pa.sw * pa.sh;
    pa.dst_off = off;
    pa.quads_per_row = div_up(pa.dw, 4);
    pa.bytewise = (pa.sw % 4 != 0 || pa.dw % 4 != 0) ? 1u : 0u;
    if (l < first_plain_level) continue;  // produced by luma_pyr1_kernel
    // aligned planes (whole dwords of source and destination, at least 4 rows): a wave per 512-column strip
    if (pa.sw % 16 == 0 && pa.sh % 2 == 0 && pa.dw % 4 == 0 && pa.src_off % 16 == 0 && pyr_stride % 16 == 0 &&
        (reinterpret_cast<uintptr_t>(d_pyr) & 15) == 0 && pa.sh >= 4) {
      constexpr int kOB = 8;  // output rows per wave
      PyrStripArgs sa{};
      sa.pyr = d_pyr; sa.pyr_stride = pyr_stride; sa.src_off = pa.src_off; sa.dst_off = pa.dst_off;
      sa.sw = pa.sw; sa.sh = pa.sh;
      sa.strips = div_up(pa.sw, 512);
      sa.bands = div_up(pa.dh, kOB);
      const uint64_t tw = (uint64_t)sa.strips * sa.bands * n_frames;
      if (tw > 0x7FFFFFFFull) return fail(SVC_ERR_UNSUPPORTED, "pyramid: too many strips for one launch");
      sa.total_waves = (uint32_t)tw;
      hipLaunchKernelGGL((pyr_strip_kernel<kOB>), dim3(div_up(sa.total_waves, 4)), dim3(256), 0, stream, sa,
                         static_cast<const uint8_t*>(d_pyr), d_pyr);
      if ((rc = check_launch("pyr_strip_kernel"))) return rc;
      continue;
    }
    if (pa.dw < 1 || pa.dh < 1 || pa.sw < 3 || pa.sh < 3)  // reflect-101 folds once: a source side below 3 cannot be mirrored
      return fail(SVC_ERR_UNSUPPORTED, "pyramid: level %u (%u x %u) is too small to reduce", l, pa.sw, pa.sh);
    const uint64_t tot = (uint64_t)n_frames * ((pa.dh + 1) / 2) * pa.quads_per_row;
    if (tot > 0x7FFFFFFFull) return fail(SVC_ERR_UNSUPPORTED, "pyramid: too many pixels for one launch");
    pa.total = (uint32_t)tot;
    hipLaunchKernelGGL(pyr_down_kernel, dim3(div_up(pa.total, 256)), dim3(256), 0, stream, pa);
    rc = check_launch("pyr_down_kernel");
    if (rc) return rc;
  }
  return SVC_OK;
}

}  // namespace svc
