// dct_pack.hip -- the compact stream ("SVCQ", stream_format.hpp) straight from the transform: B,G,R frames + region ids in, packed
// frames out, byte for byte what svc_hip_dct_quant_frames followed by svc_hip_pack_levels_frames leaves -- without the 12 bytes per
// pixel of f32 planes that route writes once and reads twice.
//
// dct_pack_kernel<N> is the front half of dct_kernel<N, QUANT> (dct.hip; the arithmetic is dct_core.hpp and quant_core.hpp, shared):
// segment columns of 16 pixels x N rows x 3 channels, N lanes per column, 48-byte row loads, integer butterflies, f64 even/odd chains, a
// wave-private LDS slab per column and no workgroup barrier.  Where that kernel stores f32, this one packs:
//   staging  once the column pass of a channel has read the slabs, every lane writes its integer levels (quant2_level: the quantiser's q
//            before the * step) as int16 into TILE IMAGES inside its column's slab -- 128 B per 8x8 tile, 512 B per 16x16 tile,
//            coefficients in the format's row-major order;
//   packing  the wave walks its tiles' 64-coefficient words in the format's order, one 16-bit LDS read per lane: the word's mask is a
//            __ballot, a lane's rank mbcnt, and the base of the word a running popcount sum -- the wave takes its words in order, so the
//            sum is wave-uniform: no scan, no atomics.
// Geometry: a wave's 64 / N segment columns lie in ONE tile row of ONE frame (the last wave of a row may be partly idle), so its tiles are
// consecutive in the format's tile order and a wave's output of one channel is one PIECE = (frame, plane, tile row, wave in the row).
//
// Levels are ordered plane-major within a frame, so a wave cannot know where its levels end up.  The workspace holds, per piece, a slot
// of the worst-case capacity (1024 levels) with the compacted levels and their count -- only the lines touched cost traffic -- and per
// frame the mask words in the format's own order.  Then
//   dct_pack_scan_kernel      one workgroup per frame: piece counts -> exclusive prefixes, the frame's level count and size;
//   dct_pack_assemble_kernel  the frame's offset (the sizes of the frames before it: frame_offset_to_lds, which the pack's scatter calls
//                             too), masks, every piece's levels to levels_off + 2 * prefix (store_level_run), and the frame's edges
//                             (write_frame_edges: header, types, the zero pad, offsets[f + 1]).
//
// Rate control (svc_hip_dct_pack_levels_budget_frames): the rule of the budgeted pack of levels.hip -- per frame the finest pair of a
// ladder whose frame fits a byte budget -- without its planes.  Two launches in front of the three above:
//   dct_count_kernel<N>       the transform up to the column pass's f32 coefficients (the SAME body as dct_pack_kernel<N>: one template,
//                             a flag), then per coefficient e = the number of ladder entries that keep it, |c| >= tau[class][k] (tau is
//                             non-decreasing in k: a binary search over a table in LDS), a histogram of e per wave in LDS, and the
//                             wave's row of it to the workspace;
//   dct_count_sum_kernel      the frame's rows summed in kSumParts interleaved parts (one workgroup per frame took 142 us for the
//                             planes route's counts: profiles/levels_budget_c3.txt);
//   dct_pack_select_kernel    one workgroup per frame: the sum of the parts, nz_k as its suffix sum, bytes_k, the choice
//                             (budget_core.hpp) and the frame's steps, which dct_pack_kernel and the assemble pass then read per frame.
//
// Two layers (svc_hip_dct_pack_layers_frames; include/svc_hip.h states them, scalable_video_codec_amd/layers.py in numpy): a base
// stream at (fg_step, bg_step) and an enhancement stream of residuals d = level(c, enh_step) - level(c, base step) * ratio, from ONE
// transform.  dct_pack_layers_kernel<N> is the third form of the body: each lane quantises its coefficients twice, the wave stages
// and walks the base levels, then stages d into the same images and walks again into a second workspace; the scan and the assemble
// pass then run once per layer.
//
// The delta stream from pixels (svc_hip_dct_pack_delta_frames; include/svc_hip.h states it): the bytes of svc_hip_dct_pack_levels_frames
// followed by svc_hip_delta_levels_frames, without the plain stream in between.  The predecessor of frame i is INPUT frame i - 1, whose
// levels are a function of its pixels, its region ids and the steps alone, so the difference is taken in the transform's registers.
// dct_pack_delta_kernel<N> is the fourth form of the body: a wave owns its piece through a RUN of kDeltaRun consecutive frames.  It
// transforms the frame in front of the run (not where the run starts at a key frame) and keeps that frame's packed levels -- 3 channels
// x 8 dwords -- in registers; then, frame by frame, it transforms, subtracts the kept levels in the two int16 halves of every dword
// where the lane's tile is predicted (a lane's 16 coefficients lie in one tile: a predicate per lane from two type reads), keeps the
// undifferenced levels for the next frame, and stages and walks the differences exactly as the one-layer form does its levels.  A run
// of R frames costs R + 1 transforms and the grid is that of n / R frames; the scan and the assemble pass are the fused pack's.
//
// The same with the key frames chosen by size (svc_hip_dct_pack_delta_auto_frames): a frame is a key frame where its difference holds
// at least as many levels as the frame itself.  dct_delta_count_kernel<N> is the fifth form of the body, TALLY beside DELTA: the delta
// form's runs without its flags (both counts of a frame are a function of two input frames), stopped after quantising; a wave stores the
// two counts of its piece per frame, dct_delta_select_kernel sums them per frame and writes the flags, and the delta form's three
// launches follow with those flags.
//
// Both with temporal layers (svc_hip_dct_pack_delta_temporal_frames, svc_hip_dct_pack_delta_temporal_auto_frames;
// include/svc_hip_temporal.h states them): frame i against INPUT frame i - min(lowbit(i), period), period 2 or 4, the bytes of
// svc_hip_dct_pack_levels_frames followed by svc_hip_delta_levels_temporal_frames.  A run of 8 starts at a frame of layer 0, so every
// reference but that of the run's first frame lies in the run: PERIOD is a template parameter of the DELTA and TALLY forms, the trip in
// front of the run transforms frame run_first - PERIOD, and the kept levels are replaced only at a frame a later one refers to.  The
// other five forms' device code is instruction for instruction what it was (profiles/dct_pack_delta_temporal_c3.txt).
//
// A quality target (svc_hip_dct_pack_levels_quality_frames; include/svc_hip_quality.h states it, layers.distortion_table in numpy): per frame
// the coarsest pair of the ladder whose squared error D_k still meets a target, optionally not finer than the byte budget allows.
// dct_measure_kernel<N> is the sixth form of the body, MEASURE beside COUNT: the counting form, which also keeps |c| of the lane's 48
// coefficients and, per ladder entry, sums e^2, e = rint(256 (|c| - q s)) -- exact integers, so any order gives the same u64.  A wave stores
// its 64 sums as a row beside its row of counts; dct_measure_sum_kernel adds both kinds of rows in kSumParts parts,
// dct_quality_select_kernel chooses and writes the frame's steps (and its row of the table), and the fused pack's three launches follow.
// The other forms' device code is instruction for instruction what it was (profiles/dct_pack_quality_c3.txt).
//
// A byte budget per group of frames (svc_hip_dct_pack_delta_budget_frames; include/svc_hip_delta_budget.h states it,
// layers.delta_ladder_counts / delta_budget_choice in numpy): the delta stream with one pair of a ladder per group, from a key frame up
// to the next.  dct_delta_ladder_kernel<N> is GROUP + TALLY of the body: the delta form's runs with the f32 coefficients of the frame
// before in registers and, per frame and ladder entry, the count of differences that entry would leave -- a row per wave and frame.
// dct_delta_ladder_sum_kernel adds the rows in kSumParts parts, dct_delta_group_select_kernel sums a group's bytes per entry, chooses over
// all entries and writes every frame's steps; dct_pack_delta_group_kernel<N> (GROUP alone) is the delta form with those steps, and the
// fused pack's scan and assemble follow.  The other forms' device code is what it was (profiles/dct_pack_delta_budget_c3.txt).
//
// A distortion target per group of frames (svc_hip_dct_pack_delta_quality_frames; include/svc_hip_delta_quality.h states it,
// layers.delta_quality_choice in numpy): the same stream with the coarsest pair at which every frame of the group meets its target, under
// the group's byte budget where there is one.  dct_delta_measure_kernel<N> is GROUP + TALLY + MEASURE of the body: the ladder tally, which
// adds the measuring form's e^2 from the levels it already has and stores a second row per wave and frame -- both tables from one pass
// over the pixels.  dct_delta_measure_sum_kernel adds both kinds of rows, dct_delta_quality_select_kernel chooses per group over all
// entries and writes every frame's steps; the group form of the pack, scan and assemble follow.  The other forms' device code is what it
// was, and the call built on the two older passes is slower (profiles/dct_pack_delta_quality_c3.txt).
#include <algorithm>
#include <type_traits>

#include "budget_core.hpp"
#include "dct_core.hpp"
#include "quant_core.hpp"
#include "stream_format.hpp"
#include "svc_common.hpp"
#include "svc_hip_delta_budget.h"
#include "svc_hip_delta_quality.h"
#include "svc_hip_quality.h"
#include "svc_hip_temporal.h"

namespace svc {
namespace {

constexpr uint32_t kPieceLevels = 1024;  // 64 / N segment columns x 16 x N coefficients, N = 8 and 16 alike

struct DctPackWs {
  int16_t* slots;        // [n][pieces][kPieceLevels]
  uint32_t* masks;       // [n][mask_dwords] the frame's mask section
  uint32_t* counts;      // [n][pieces] levels of a piece, then (scan) their exclusive prefix
  uint32_t* frame_bytes; // [n]
  uint32_t* frame_levels;// [n]
};

// a frame's steps as the budgeted call's selection leaves them: the pair, and RN(1 / step) of each as the host computes it
struct FrameSteps {
  uint32_t fg, bg;
  float fg_inv, bg_inv;
};

// the budgeted call's workspace: the pack's own, then
constexpr uint32_t kSumParts = 32;  // workgroups that share the sum of a frame's rows
struct BudgetWs {
  DctPackWs pack;
  uint32_t* rows;     // [n][waves of a frame][kMaxLadder]: a wave's coefficients that exactly k + 1 entries keep (the last entry: all)
  uint32_t* parts;    // [n][kSumParts][kMaxLadder]: the rows of a frame summed part by part
  FrameSteps* steps;  // [n]
};

struct PackGeom {
  FrameLayout l;
  uint32_t w, h, n_block, mvbw, mvbh;
  uint32_t segs_per_band;   // w / 16
  uint32_t waves_per_row;   // ceil(segs_per_band / (64 / N))
  uint32_t pieces;          // 3 * tiles_y * waves_per_row, in the order of the levels: plane, tile row, wave
  uint32_t mask_dwords;     // of one frame
};

PackGeom make_pack_geom(uint32_t w, uint32_t h, uint32_t block, uint32_t mvbw, uint32_t mvbh) {
  PackGeom g{};
  g.l = frame_layout(w, h, block, block, mvbw, mvbh);
  g.w = w; g.h = h; g.n_block = block; g.mvbw = mvbw; g.mvbh = mvbh;
  g.segs_per_band = w / 16;
  g.waves_per_row = div_up(g.segs_per_band, 64 / block);
  g.pieces = 3 * g.l.tiles_y * g.waves_per_row;
  g.mask_dwords = (uint32_t)((g.l.levels_off - g.l.masks_off) / 4);
  return g;
}

// a frame's mask section in the workspace: its dwords, rounded up so that every frame's section starts 16-byte aligned
__host__ __device__ inline uint64_t ws_mask_pitch(const PackGeom& g) { return up16(4ull * g.mask_dwords) / 4; }

// (slots, masks, rows and parts are whole multiples of 16 B as they are: taken without rounding)
DctPackWs pack_ws(Carver& c, uint32_t n, const PackGeom& g) {
  DctPackWs s;
  s.slots = c.take<int16_t>((uint64_t)kPieceLevels * n * g.pieces, false);
  s.masks = c.take<uint32_t>(n * ws_mask_pitch(g), false);
  s.counts = c.take<uint32_t>((uint64_t)n * g.pieces);
  s.frame_bytes = c.take<uint32_t>(n);
  s.frame_levels = c.take<uint32_t>(n);
  return s;
}

BudgetWs budget_ws(Carver& c, uint32_t n, const PackGeom& g) {
  BudgetWs s;
  s.pack = pack_ws(c, n, g);
  s.rows = c.take<uint32_t>((uint64_t)kMaxLadder * n * g.l.tiles_y * g.waves_per_row, false);
  s.parts = c.take<uint32_t>((uint64_t)kMaxLadder * n * kSumParts, false);
  s.steps = c.take<FrameSteps>(n);
  return s;
}

// the quality call's workspace: the budgeted call's (so the fixed and the budgeted call run on it too), then the squared errors
struct QualityWs {
  BudgetWs budget;
  uint64_t* drows;   // [n][waves of a frame][kMaxLadder]: a wave's sum of e^2 per ladder entry (0 from the ladder's end on)
  uint64_t* dparts;  // [n][kSumParts][kMaxLadder]: the rows of a frame summed part by part
};
QualityWs quality_ws(Carver& c, uint32_t n, const PackGeom& g) {
  QualityWs s;
  s.budget = budget_ws(c, n, g);
  s.drows = c.take<uint64_t>((uint64_t)kMaxLadder * n * g.l.tiles_y * g.waves_per_row, false);
  s.dparts = c.take<uint64_t>((uint64_t)kMaxLadder * n * kSumParts, false);
  return s;
}

struct DctPackArgs {
  const uint8_t* bgr;
  uint64_t frame_stride;
  PackGeom g;
  uint32_t total_waves;       // frames * tile rows * waves per row
  const uint32_t* types;
  float fg_step, bg_step, fg_inv, bg_inv;  // inv = RN(1 / step), computed on the host
  const FrameSteps* steps;    // [n] each frame's own steps (the budgeted call), or null: the four above for every frame
  DctPackWs ws;
};

// what the counting form takes besides: the ladder, its search depth and where the waves' rows go
struct CountArgs {
  Ladder lad;
  uint32_t probes;  // bit length of lad.len: the probes that find e in 0 .. lad.len
  uint32_t* rows;
};
struct NoCountArgs {};
struct LadderInv {
  float inv[2][kMaxLadder];  // RN(1 / step), computed on the host as the fixed call computes it
};
// what the measuring form takes besides: each entry's RN(1 / step) for the quantiser, and where the waves' rows of squared errors go
struct MeasureArgs : CountArgs {
  LadderInv li;
  uint64_t* drows;
};
// what the two-layer form takes besides: the enhancement's step, each class's base step / enh_step, the frames' windows, and the
// second workspace (a.ws is the base layer's)
struct LayerArgs {
  float enh_step, enh_inv;
  uint32_t fg_ratio, bg_ratio;
  const uint32_t* window;  // [n][4] x, y, w, h in padded coordinates, or null: every tile is enhanced
  DctPackWs enh;
};
// what the delta form takes besides: the frame in front of frame 0 (null: none), the key flags, and how the frames fall into runs
struct DeltaRunArgs {
  const uint8_t* prev_bgr;     // one frame, or null: frame 0 is a key frame
  const uint32_t* prev_types;  // [mv blocks] of that frame
  const uint32_t* key;         // [n] or null
  uint32_t n_frames, run;      // a wave carries frames [r * run, min((r + 1) * run, n_frames))
  uint32_t one_step;           // fg_step == bg_step: every tile of a frame that is not a key frame is predicted
};
// what the delta form's counting takes: the same runs (key is not read), and where a wave leaves the two level counts of its piece
struct DeltaTallyArgs : DeltaRunArgs {
  uint32_t* tally;  // [runs][waves of a frame][run][2] levels of the piece, levels of its difference to the frame before
};
// what the delta form's ladder tally takes: the same runs (key IS read), the ladder with each entry's RN(1 / step) for the quantiser, and
// where a wave leaves its row of counts per frame
struct DeltaLadderArgs : DeltaRunArgs {
  Ladder lad;
  LadderInv li;
  uint32_t* rows;  // [runs][waves of a frame][run][kMaxLadder]: the wave's non-zero differences of the frame at entry k (0 from the ladder's end on)
};
// what the delta form's measuring tally takes besides: where a wave leaves its row of squared errors per frame
struct DeltaMeasureArgs : DeltaLadderArgs {
  uint64_t* drows;  // [runs][waves of a frame][run][kMaxLadder]: the wave's sum of e^2 of the frame at entry k, beside rows
};
// Frames of a run.  {1, 2, 4, 8} measured at C3 and C5, batches of 16 (profiles/dct_pack_delta_c3.txt has all four): 8 is the fastest
// or tied in every row -- at C3 / (1, 640) 0.194, 0.163, 0.152, 0.152 ms; at C5 1.065, 0.897, 0.820, 0.790.
#ifndef SVC_DCT_PACK_DELTA_RUN  // (the probe that measured them builds this file once per value: tools/dct_pack_probe.py delta-encode)
#define SVC_DCT_PACK_DELTA_RUN 8
#endif
constexpr uint32_t kDeltaRun = SVC_DCT_PACK_DELTA_RUN;
static_assert(kDeltaRun >= 1, "a run holds a frame");
// Temporal layers: a run starts at a frame of layer 0, so it holds whole periods (a build that probes another kDeltaRun keeps 8 here).
constexpr uint32_t kTemporalRun = kDeltaRun % 4 == 0 ? kDeltaRun : 8;
// Period 4 needs the levels of frame 4k (for 4k + 1, 4k + 2 and 4k + 4) and of 4k + 2 (for 4k + 3).  0: both are kept, 48 dwords, and the
// kernel has 139 / 147 VGPRs: three workgroups a CU where the delta form has four.  1: one set is kept -- frame 4k + 2's levels replace
// frame 4k's, and frame 4k is transformed a second time in front of frame 4k + 4 (not where that is a key frame): 10 transforms for
// 8 frames at period 2's registers.  Both measured in profiles/dct_pack_delta_temporal_c3.txt (tools/dct_pack_probe.py
// delta-temporal-encode builds this file once per value).
#ifndef SVC_DCT_PACK_TEMPORAL_REDO
#define SVC_DCT_PACK_TEMPORAL_REDO 0
#endif
constexpr bool kTemporalRedo = SVC_DCT_PACK_TEMPORAL_REDO != 0;
// The measuring form takes an entry's sum from the entry before where no lane of the wave has another step there.  1: it does; 0: every
// entry is computed.  Both measured in profiles/dct_pack_quality_c3.txt (tools/dct_pack_probe.py quality-variants builds this file once
// per value).
#ifndef SVC_DCT_PACK_MEASURE_SHARE
#define SVC_DCT_PACK_MEASURE_SHARE 1
#endif
constexpr bool kMeasureShare = SVC_DCT_PACK_MEASURE_SHARE != 0;
// svc_hip_dct_pack_delta_quality_frames takes both tables from one pass over the pixels (dct_delta_measure_kernel).  1: from two, the
// measuring form then the ladder tally, with the same launches after them: the form the fused one was measured against in
// profiles/dct_pack_delta_quality_c3.txt (tools/dct_pack_probe.py delta-quality builds this file once per value).
#ifndef SVC_DCT_PACK_DELTA_QUALITY_TWO_PASS
#define SVC_DCT_PACK_DELTA_QUALITY_TWO_PASS 0
#endif
constexpr bool kDeltaQualityTwoPass = SVC_DCT_PACK_DELTA_QUALITY_TWO_PASS != 0;
constexpr uint32_t kTauTable = 2 * kMaxLadder;  // a class's thresholds, padded with +inf to what 7 probes can reach

__device__ __forceinline__ uint32_t lane_rank(uint64_t mask) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

__device__ __forceinline__ uint32_t pack2(f32x2 q) {  // two levels as int16, the first in the low half
  return ((uint32_t)(int32_t)q.x & 0xFFFFu) | ((uint32_t)(int32_t)q.y << 16);
}

template <typename K>
__device__ __forceinline__ bool k_one_step(const K& k) {
  if constexpr (std::is_base_of_v<DeltaRunArgs, K>) return k.one_step != 0;
  else return false;
}

// the workspace a layer's walk fills: the base's (the only one of the one-layer forms), or the enhancement's
template <typename K>
__device__ __forceinline__ const DctPackWs& layer_ws(const DctPackArgs& a, const K& k, int layer) {
  if constexpr (std::is_same_v<K, LayerArgs>) return layer == 0 ? a.ws : k.enh;
  else return a.ws;
}

// two residuals of the enhancement layer, packed like pack2: fine level - base level * ratio in int32, kept as int16 (|d| <= ratio / 2 + 1)
__device__ __forceinline__ uint32_t residual2(f32x2 fine, f32x2 base, int32_t ratio) {
  const int32_t dx = (int32_t)fine.x - (int32_t)base.x * ratio, dy = (int32_t)fine.y - (int32_t)base.y * ratio;
  return ((uint32_t)dx & 0xFFFFu) | ((uint32_t)dy << 16);
}

// a - b in each int16 half, modulo 2^16: one packed subtract
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t sub2(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(uint32_t, (u16x2)(__builtin_bit_cast(u16x2, a) - __builtin_bit_cast(u16x2, b)));
}

// COUNT = false: the fused pack.  COUNT = true: the same transform, stopped at the column pass's f32 coefficients, which are counted per
// ladder entry instead of quantised: k, and the counting kernel's LDS -- both classes' thresholds, tau_tab[c][i] = tau[c][i] (+inf from
// the ladder's end on), and a histogram per wave (null for the pack).  LAYERS = true (with COUNT = false): the fused pack of two layers,
// the base into a.ws and the residuals of the tiles inside the frame's window into k.enh.  DELTA = true (alone): the fused pack of
// differences; a.total_waves counts runs where the other forms count frames, and the wave goes through its run's frames in turn.
// TALLY = true (with DELTA): the delta form's runs, stopped after quantising: no flag is read, nothing is staged or walked; per frame
// the wave stores the non-zero levels and the non-zero differences of its piece to its own place in k.tally
// (svc_hip_dct_pack_delta_auto_frames sums and chooses by them).
// PERIOD = 2 or 4 (with DELTA, alone or with TALLY): the delta form with temporal layers, frame i against frame i - min(lowbit(i), PERIOD).
// kTemporalRun is a multiple of 4, so a run starts at a frame of layer 0 and every reference but its first frame's lies in the run: the trip
// in front of the run transforms frame run_first - PERIOD, `before` keeps the last frame of layer 0 (2k or 4k: it is replaced only there)
// and, PERIOD = 4, `mid` keeps frame 4k + 2 for frame 4k + 3.  A run still costs R + 1 transforms.  REDO (PERIOD = 4): no `mid`; `before`
// takes frame 4k + 2's levels as well, and a trip in front of frame 4k + 4 puts frame 4k's back (kTemporalRedo above).
// MEASURE = true (with COUNT): the counting form, and per ladder entry k the wave's sum of e^2, e = rint(256 (|c| - q_k s_k)) with q_k the
// level entry k's step of the lane's class gives (include/svc_hip_quality.h states it, layers.distortion_table in numpy).  The lane keeps
// |c| of all three channels and, after the last, goes through the ladder once: 48 quantisations per entry, the lanes' u64 sums added over
// the wave, the total kept by lane k and stored with the wave's row of counts.  An entry at which no lane's step differs from the entry
// before (a ladder of levels.step_ladder moves one class at a time) takes the sum before it: nothing is computed.  The entry is the same
// in every lane, so both classes' step and RN(1 / step) are uniform loads from the arguments and the lane selects by its class: no table.
// GROUP = true (with DELTA, PERIOD 1): the forms of svc_hip_dct_pack_delta_budget_frames (include/svc_hip_delta_budget.h states it,
// layers.delta_ladder_counts in numpy), one pair of steps per group of frames.  Alone: the delta form with each frame's own pair from
// a.steps -- the predicate's fg == bg is then the frame's, not the call's.  With TALLY: the delta form's runs WITH its flags, stopped at
// the column pass's f32 coefficients.  The lane keeps the coefficients of the frame before (48 f32, not levels: a level belongs to one
// step) and, channel by channel, goes through the ladder with the channel's 16 against the kept 16: per entry both are quantised at the
// entry's step of the lane's tile and the levels that differ are counted -- against 0 where the tile is not predicted at that entry, that
// is in a key frame or where the entry gives the tile another step in the frame before (fg_k == bg_k changes along a ladder).  Integer
// counts, so any order of summing gives the same u32.  As in the measuring form, an entry at which no lane's step and no lane's
// predicate differ from the entry before takes that entry's sum.  Lane k keeps entry k's sum over the three channels; the wave stores
// that row per frame to a place of its own (no atomics, as the TALLY form).
// MEASURE = true (with GROUP + TALLY): the form of svc_hip_dct_pack_delta_quality_frames (include/svc_hip_delta_quality.h), the ladder
// tally with the measuring form's squared errors.  From the level q the tally already has of the channel's 16 coefficients at entry k the
// lane adds e^2, e = rint(256 fma(-q, s, c)); the lane's u64 sum and its count go through ONE wave reduction (the count in the bits the
// sum cannot reach), and lane k keeps entry k's two sums over the three channels: a second row per wave and frame, of u64.  The skip rule
// is the union of both parents' -- the tally's already is: an entry is computed where any lane's step or predicate moved.
template <int N, bool COUNT, bool LAYERS = false, bool DELTA = false, bool TALLY = false, int PERIOD = 1, bool REDO = false, bool MEASURE = false,
          bool GROUP = false>
__device__ __forceinline__ void dct_pack_body(
    const DctPackArgs& a,
    const std::conditional_t<MEASURE && TALLY && GROUP, DeltaMeasureArgs,
    std::conditional_t<MEASURE, MeasureArgs,
    std::conditional_t<COUNT, CountArgs,
                             std::conditional_t<LAYERS, LayerArgs,
                                                std::conditional_t<TALLY && GROUP, DeltaLadderArgs,
                                                std::conditional_t<TALLY, DeltaTallyArgs, std::conditional_t<DELTA, DeltaRunArgs, NoCountArgs>>>>>>>& k,
    float (*tau_tab)[kTauTable], uint32_t (*hist_all)[kMaxLadder]) {
  static_assert(!GROUP || (DELTA && PERIOD == 1), "a group's steps: the delta form without temporal layers");
  constexpr bool kLadderTally = GROUP && TALLY;  // the counts of every ladder entry instead of the pack
  static_assert(!MEASURE || COUNT || kLadderTally, "the measuring form is the counting form, or the ladder tally, with the squared errors");
  constexpr bool kTallyMeasure = kLadderTally && MEASURE;  // the ladder tally with every entry's squared error beside its count
  static_assert(!(COUNT && LAYERS), "the counting form has no layers");
  static_assert(!(DELTA && (COUNT || LAYERS)), "the delta form is one layer at fixed steps");
  static_assert(!TALLY || DELTA, "the tally walks the delta form's runs");
  static_assert(PERIOD == 1 || (DELTA && (PERIOD == 2 || PERIOD == 4) && kTemporalRun % PERIOD == 0), "temporal layers: the delta form, whole periods a run");
  static_assert(!REDO || PERIOD == 4, "only period 4 has a second kept frame to trade for a transform");
  constexpr bool kMid = PERIOD == 4 && !REDO;  // frame 4k + 2 is kept in `mid`
  constexpr uint32_t kCols = 64 / N;        // segment columns of a wave
  constexpr uint32_t kColWords = N / 4;     // mask words of a segment column: two 8x8 tiles of one word, or one 16x16 tile of four
  constexpr int kSlab = N == 8 ? kSlab8 : kSlab16;
  // Where word k of the wave's column g starts inside the column's slab.  The slabs are a multiple of 128 B apart, so images at the same
  // place in every slab would put the staging stores of a half-wave's columns on the same banks (8-way at N = 8): each image is skewed
  // by its column -- N = 8: 16 B per tile, the 32 lanes of a half-wave then store to 32 different banks; N = 16: 64 B per odd column.
  // A word's 64 levels stay 128 contiguous bytes, so the walk's reads have no conflicts either way.
  auto image_at = [](uint32_t col, uint32_t k) { return N == 8 ? k * 144 + col * 32 : (col & 1u) * 64 + k * 128; };
  static_assert((N == 8 ? 144 + 7 * 32 + 128 : 64 + 512) <= kSlab, "a column's tile images fit its slab");
  __shared__ __attribute__((aligned(16))) uint8_t lds[(256 / N) * kSlab];

  const PackGeom& gm = a.g;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, sc_local = tid / N, j = tid % N, g = lane / N;
  // the wave's place: (frame, tile row, wave in the row), the same in every lane
  const uint32_t wv = __builtin_amdgcn_readfirstlane(xcd_contiguous_block(blockIdx.x, gridDim.x) * 4u + (tid >> 6));
  if constexpr (COUNT) {
    const uint32_t c = tid / kTauTable, i = tid % kTauTable;  // 256 threads = 2 classes x 128 entries
    tau_tab[c][i] = i < k.lad.len ? k.lad.tau[c][i] : INFINITY;
    hist_all[tid >> 6][lane] = 0;
    __syncthreads();  // the only workgroup barrier, in front of the first exit
  }
  if (wv >= a.total_waves) return;
  const uint32_t row_g = wv / gm.waves_per_row, wr = wv - row_g * gm.waves_per_row;
  const uint32_t frame0 = row_g / gm.l.tiles_y, band = row_g - frame0 * gm.l.tiles_y;  // DELTA: frame0 is the run
  const uint32_t seg0 = wr * kCols, seg = seg0 + g;
  const uint32_t ncols = min(kCols, gm.segs_per_band - seg0);  // the last wave of a row may hold fewer
  const bool active = g < ncols;  // an idle column runs on zeros and is not packed
  const uint32_t y_pix = band * N, x_pix = seg * 16;

  // DELTA: the run's frames in turn, it = -1 for the frame in front of the run, of which only the levels are kept.  The other forms:
  // one trip, it = 0 -- the loop's condition is a constant false there, so their code is what it was without the loop (their symbols'
  // sizes are compared in profiles/dct_pack_delta_c3.txt).  Everything that tells the trips apart is the same in every lane of the wave.
  uint32_t run_first = 0, run_len = 1;
  uint32_t before[3][8] = {};  // DELTA: the undifferenced levels of the frame before, as lv below, and that frame's type of the lane's tile
  uint32_t t_before = 0;
  uint32_t mid[3][8] = {};  // kMid: the same of frame 4k + 2, from there to frame 4k + 3
  bool redo = false;        // REDO: this trip transforms frame 4k again, in front of frame 4k + 4 (`it` stays at 4k + 3)
  uint32_t t_mid = 0;
  uint32_t full = 0;  // COUNT: this lane's coefficients that the whole ladder keeps
  float kept[MEASURE && COUNT ? 3 : 1][16];  // MEASURE: |c| of the lane's coefficients, all three channels, and the lane's class
  uint32_t cls = 0;
  float prior[kLadderTally ? 3 : 1][16] = {};  // kLadderTally: the f32 coefficients of the frame before, all three channels
  uint32_t tally_row = 0;                      // and, in lane k, the frame's count at ladder entry k
  uint64_t measure_row = 0;                    // kTallyMeasure: and the frame's sum of e^2 at that entry
  bool frame_one_step = false;                 // GROUP: the trip's frame has fg == bg
  if constexpr (DELTA) {
    run_first = frame0 * k.run;
    run_len = min(k.run, k.n_frames - run_first);
  }
  int it = DELTA ? -1 : 0;
  do {  // (a trip's statements keep the indentation they have had as the only trip)
  const uint32_t frame = !DELTA ? frame0 : PERIOD > 1 && it < 0 ? run_first - (uint32_t)PERIOD
                                         : REDO && redo     ? run_first + (uint32_t)it - 3u : run_first + (uint32_t)it;
  const bool use_mid = kMid && (it & 3) == 3;  // (it = -1 too: nothing is subtracted in that trip)
  // PERIOD > 1: a trip whose frame is only kept, for the frame after it (asked only in that form's own statements: the others' code stays)
  auto front = [&] { return it < 0 || (REDO && redo); };
  bool key = false;  // DELTA: a key frame is not predicted, and the frame in front of it is not read
  const uint8_t* frame_bgr = nullptr;  // DELTA: the trip's frame and its types
  const uint32_t* frame_types = nullptr;
  if constexpr (DELTA) {
    const uint32_t f = run_first + (uint32_t)max(it, 0);  // the frame whose flag decides this trip
    if constexpr (TALLY && !GROUP) key = f == 0 && !k.prev_bgr;  // no flag is read: the frame in front of a run is always transformed
    else key = (f == 0 && !k.prev_bgr) || (k.key && k.key[f] != 0);
    if (it < 0 && key) continue;  // (`before` is not read)
    const bool outside = it < 0 && run_first == 0;  // the frame in front of frame 0
    frame_bgr = outside ? k.prev_bgr : a.bgr + (size_t)frame * a.frame_stride;
    frame_types = outside ? k.prev_types : a.types + (size_t)frame * gm.l.mvb;
  }

  // 16 BGR pixels of row j of this segment column
  uint32_t wds[12] = {};
  uint32_t t = 0;
  if (active) {
    const uint4* p = reinterpret_cast<const uint4*>((DELTA ? frame_bgr : a.bgr + (size_t)frame * a.frame_stride) + ((size_t)(y_pix + j) * gm.w + x_pix) * 3);
    const uint4 v0 = p[0], v1 = p[1], v2 = p[2];
    wds[0] = v0.x; wds[1] = v0.y; wds[2] = v0.z; wds[3] = v0.w;
    wds[4] = v1.x; wds[5] = v1.y; wds[6] = v1.z; wds[7] = v1.w;
    wds[8] = v2.x; wds[9] = v2.y; wds[10] = v2.z; wds[11] = v2.w;
    // tile type = type of the MV block that holds it; background (0) takes bg_step: the rule of dct_kernel
    const uint32_t col = N == 8 ? x_pix + 2 * j : x_pix + j;
    if constexpr (DELTA) t = frame_types[(y_pix / gm.mvbh) * gm.l.mfw + col / gm.mvbw];
    else t = a.types[(size_t)frame * gm.l.mvb + (y_pix / gm.mvbh) * gm.l.mfw + col / gm.mvbw];
  }
  float step = t == 0 ? a.bg_step : a.fg_step, inv_step = t == 0 ? a.bg_inv : a.fg_inv;
  if (!COUNT && a.steps) {  // the wave's own frame's pair: one workgroup's four waves can belong to four frames
    const FrameSteps fs = a.steps[frame];
    step = (float)(t == 0 ? fs.bg : fs.fg);  // libs/decoder.cpp:141 divides a float by an unsigned
    inv_step = t == 0 ? fs.bg_inv : fs.fg_inv;
    if constexpr (GROUP) frame_one_step = fs.fg == fs.bg;  // (the frame in front of a run: its group's pair, the next frame's unless that is a key frame)
  }
  int32_t ratio = 0;      // LAYERS: the lane's tile's base step / enh_step, and whether the frame's window holds the tile's origin
  bool enhanced = false;  // (the containment rule of the decoders' gaze: w or h of 0 holds nothing)
  if constexpr (LAYERS) {
    ratio = (int32_t)(t == 0 ? k.bg_ratio : k.fg_ratio);
    enhanced = true;
    if (k.window) {
      const uint32_t* r = k.window + 4ull * frame;
      const uint32_t tx = N == 8 ? x_pix + 8 * (j >> 2) : x_pix;
      enhanced = tx >= r[0] && tx - r[0] < r[2] && y_pix >= r[1] && y_pix - r[1] < r[3];
    }
  }

  uint8_t* slab = lds + sc_local * kSlab;
  const uint8_t* wave_slabs = lds + (sc_local - g) * kSlab;
  const uint32_t nwords = ncols * kColWords;                           // mask words of the piece, in the format's order
  const uint32_t word0 = (seg0 * (16 / N)) * gm.l.words;               // the piece's first word within its tile row
  // DELTA: the lane's tile is predicted where both frames code it at one step
  const bool predicted = DELTA && !key && ((GROUP ? frame_one_step : k_one_step(k)) || (t == 0) == ((kMid && use_mid ? t_mid : t_before) == 0));
  uint32_t tally = 0;  // TALLY: this lane's non-zero levels of the frame (at most 48) in the low half, non-zero differences in the high

#pragma unroll
  for (int c = 0; c < 3; ++c) {
    int x[16];
    double r[16];
#pragma unroll
    for (int p = 0; p < 16; ++p) x[p] = (int)((wds[(3 * p + c) >> 2] >> (8 * ((3 * p + c) & 3))) & 0xFFu);
    if (N == 8) {
      dct1d<8, int>(x, r);
      dct1d<8, int>(x + 8, r + 8);
    } else {
      dct1d<16, int>(x, r);
    }
    double2* row = reinterpret_cast<double2*>(slab + j * kRowPitch);
#pragma unroll
    for (int i = 0; i < 8; ++i) row[i] = make_double2(r[2 * i], r[2 * i + 1]);
    wave_lds_sync();

    uint32_t lv[8];  // this lane's levels of the channel, two int16 each
    uint32_t dv[8];  // LAYERS: its residuals, likewise
    float m[16];     // COUNT: |c| of its 16 coefficients instead; kLadderTally: the coefficients themselves
    if (N == 8) {
      // lane j takes columns 2j, 2j+1 of the 16-wide slab (tile j >> 2): lv[v] = row v
      double ca[8], cb[8], ya[8], yb[8];
#pragma unroll
      for (int y = 0; y < 8; ++y) {
        double2 v = *reinterpret_cast<const double2*>(slab + y * kRowPitch + j * 16);
        ca[y] = v.x;
        cb[y] = v.y;
      }
      dct1d<8, double>(ca, ya);
      dct1d<8, double>(cb, yb);
#pragma unroll
      for (int v = 0; v < 8; ++v) {
        if constexpr (COUNT) {
          m[2 * v] = fabsf((float)ya[v]);
          m[2 * v + 1] = fabsf((float)yb[v]);
        } else if constexpr (kLadderTally) {
          m[2 * v] = (float)ya[v];
          m[2 * v + 1] = (float)yb[v];
        } else if constexpr (LAYERS) {
          const f32x2 cf{(float)ya[v], (float)yb[v]}, qb = quant2_level(cf, step, inv_step);
          lv[v] = pack2(qb);
          dv[v] = enhanced ? residual2(quant2_level(cf, k.enh_step, k.enh_inv), qb, ratio) : 0u;
        } else {
          lv[v] = pack2(quant2_level(f32x2{(float)ya[v], (float)yb[v]}, step, inv_step));
        }
      }
    } else {
      // lane j takes column j: lv[v / 2] = rows v, v + 1
      double cc[16], yy[16];
#pragma unroll
      for (int y = 0; y < 16; ++y) cc[y] = *reinterpret_cast<const double*>(slab + y * kRowPitch + j * 8);
      dct1d<16, double>(cc, yy);
#pragma unroll
      for (int v = 0; v < 16; v += 2) {
        if constexpr (COUNT) {
          m[v] = fabsf((float)yy[v]);
          m[v + 1] = fabsf((float)yy[v + 1]);
        } else if constexpr (kLadderTally) {
          m[v] = (float)yy[v];
          m[v + 1] = (float)yy[v + 1];
        } else if constexpr (LAYERS) {
          const f32x2 cf{(float)yy[v], (float)yy[v + 1]}, qb = quant2_level(cf, step, inv_step);
          lv[v / 2] = pack2(qb);
          dv[v / 2] = enhanced ? residual2(quant2_level(cf, k.enh_step, k.enh_inv), qb, ratio) : 0u;
        } else {
          lv[v / 2] = pack2(quant2_level(f32x2{(float)yy[v], (float)yy[v + 1]}, step, inv_step));
        }
      }
    }
    wave_lds_sync();  // every lane of the column has read the slab: it becomes the column's tile images

    if constexpr (COUNT) {
      // e = the entries that keep a coefficient = the thresholds of its class (the lane's: a lane's coefficients lie in one tile) that
      // are <= |c|.  tau is non-decreasing and the table ends in +inf, so e is found bit by bit, highest first: with e' of the earlier
      // probes, bit b is set exactly when tab[e' + 2^b - 1] <= |c|.  Sixteen independent searches per probe keep the LDS reads in flight.
      const float* tab = tau_tab[t == 0 ? 0 : 1];
      uint32_t e[16] = {};
#pragma unroll
      for (int b = 6; b >= 0; --b) {
        if ((uint32_t)b >= k.probes) continue;  // the same in every lane
#pragma unroll
        for (int i = 0; i < 16; ++i) e[i] += m[i] >= tab[e[i] + ((1u << b) - 1u)] ? (1u << b) : 0u;
      }
      // bin e - 1 of the wave's histogram; e = 0 is nobody's level and e = len (every tile's DC, a flat frame's every level) is counted
      // in a register: neither serialises the wave's adds on one bin
      uint32_t* hist = hist_all[tid >> 6];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        full += e[i] == k.lad.len ? 1u : 0u;
        if (e[i] != 0 && e[i] != k.lad.len) atomicAdd(&hist[e[i] - 1], 1u);
      }
      if constexpr (MEASURE) {  // (COUNT: the measuring form)
        cls = t == 0 ? 0u : 1u;
#pragma unroll
        for (int i = 0; i < 16; ++i) kept[c][i] = m[i];
      }
      continue;  // (the slabs are free for the next channel: the sync above)
    }
    if constexpr (kLadderTally) {
      // Entry kk's steps are uniform loads from the arguments (the measuring form's way: no table); the lane selects by its tile's class
      // now and in the frame before.  Where the two steps differ the tile is not predicted at that entry -- the pack's predicate, per entry.
      if (it >= 0) {
        uint32_t total = 0, prev_step = 0;  // (no step is 0: the first entry is always computed)
        uint64_t total_d = 0;               // kTallyMeasure: the entry's sum of e^2 over the wave, this channel
        bool prev_pred = false;
        for (uint32_t kk = 0; kk < k.lad.len; ++kk) {
          const uint32_t s_bg = k.lad.step[0][kk], s_fg = k.lad.step[1][kk];
          const uint32_t s_now = t == 0 ? s_bg : s_fg, s_before = t_before == 0 ? s_bg : s_fg;
          const float inv = t == 0 ? k.li.inv[0][kk] : k.li.inv[1][kk];
          const bool pred = !key && s_now == s_before;
          if (__ballot(s_now != prev_step || pred != prev_pred) != 0) {  // the same in every lane; a lane for which nothing moved computes the count it had
            const float s = (float)s_now;
            uint32_t cnt = 0;
            uint64_t sq = 0;
#pragma unroll
            for (int i = 0; i < 16; i += 2) {
              const f32x2 q = quant2_level(f32x2{m[i], m[i + 1]}, s, inv);
              f32x2 qb = {0.f, 0.f};
              if (pred) qb = quant2_level(f32x2{prior[c][i], prior[c][i + 1]}, s, inv);
              cnt += (q.x != qb.x ? 1u : 0u) + (q.y != qb.y ? 1u : 0u);  // (integers in f32; -0.0 == 0.0, as both pack to level 0)
              if constexpr (kTallyMeasure) {  // the measuring form's e from the same level: the quantiser is odd, so c's sign only flips e's
                const uint32_t e0 = (uint32_t)fabsf(rintf(256.f * __builtin_fmaf(-q.x, s, m[i])));
                const uint32_t e1 = (uint32_t)fabsf(rintf(256.f * __builtin_fmaf(-q.y, s, m[i + 1])));
                sq += (uint64_t)e0 * e0;
                sq += (uint64_t)e1 * e1;
              }
            }
            if constexpr (kTallyMeasure) {
              // One reduction for both: e^2 < 2^41 (the header's bound), a lane's 16 below 2^45 and the wave's below 2^51; the wave's
              // count is at most 64 x 16 = 2^10.  The count rides in bits 52 .. 62 of the same u64.
              uint64_t both = sq | ((uint64_t)cnt << 52);
              for (uint32_t off = 32; off >= 1; off >>= 1) both += __shfl_xor(both, off, 64);
              total = (uint32_t)(both >> 52);
              total_d = both & ((1ull << 52) - 1);
            } else {
              total = wave_sum(cnt);
            }
          }
          prev_step = s_now;
          prev_pred = pred;
          if (lane == kk) tally_row += total;
          if constexpr (kTallyMeasure) {
            if (lane == kk) measure_row += total_d;
          }
        }
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) prior[c][i] = m[i];
      continue;  // (the slabs are free for the next channel: the sync above)
    }
    if constexpr (DELTA && PERIOD > 1) {  // the same against the kept frame of the trip's layer; the levels stay where a later frame refers to them
      // (the same in every lane)  REDO: every even frame is kept, frame 4k + 2 in frame 4k's place
      const bool keep = front() || (it & (REDO ? 1 : PERIOD - 1)) == 0, keep_mid = kMid && (it & 3) == 2;
#pragma unroll
      for (int v = 0; v < 8; ++v) {
        const uint32_t cur = lv[v];
        if (predicted) lv[v] = sub2(cur, kMid && use_mid ? mid[c][v] : before[c][v]);
        if constexpr (TALLY) {
          const uint32_t d = lv[v];
          tally += ((cur & 0xFFFFu) != 0) + ((cur >> 16) != 0) + ((((d & 0xFFFFu) != 0) + ((d >> 16) != 0)) << 16);
        }
        if (keep) before[c][v] = cur;
        if (kMid && keep_mid) mid[c][v] = cur;
      }
      if (front() || TALLY) continue;  // a frame that is only kept is not packed (its tally is not stored); the tally packs nothing
    } else if constexpr (DELTA) {  // the levels stay for the next frame; what is staged and walked is their difference to the frame before
#pragma unroll
      for (int v = 0; v < 8; ++v) {
        const uint32_t cur = lv[v];
        if (predicted) lv[v] = sub2(cur, before[c][v]);
        before[c][v] = cur;
      }
      if (it < 0) continue;  // the frame in front of the run is not packed
      if constexpr (TALLY) {  // (before[c] holds the frame's levels, lv their differences where predicted: the int16 halves that are not 0)
#pragma unroll
        for (int v = 0; v < 8; ++v) {
          const uint32_t cur = before[c][v], d = lv[v];
          tally += ((cur & 0xFFFFu) != 0) + ((cur >> 16) != 0) + ((((d & 0xFFFFu) != 0) + ((d >> 16) != 0)) << 16);
        }
        continue;  // (the slabs are free for the next channel: the sync above)
      }
    }

    // a layer of this channel: the lane's levels q to the column's tile images, then the wave's walk into the layer's workspace.  The
    // second layer's images replace the first's once the walk has read them (the sync that ends a layer)
#pragma unroll
    for (int layer = 0; layer < (LAYERS ? 2 : 1); ++layer) {
      const uint32_t* q = layer == 0 ? lv : dv;
      const DctPackWs& ws = layer_ws(a, k, layer);
      if (N == 8) {
        uint8_t* img = slab + image_at(g, j >> 2) + (j & 3u) * 4;  // coefficient (v, 2 (j & 3)) of tile j >> 2: 2 * (v * 8 + 2 (j & 3)) bytes in
#pragma unroll
        for (int v = 0; v < 8; ++v) *reinterpret_cast<uint32_t*>(img + v * 16) = q[v];
      } else {
        uint8_t* img = slab + image_at(g, 0) + j * 2;  // coefficient (v, j): 2 * (v * 16 + j) bytes in
#pragma unroll
        for (int v = 0; v < 16; v += 2) {
          *reinterpret_cast<uint16_t*>(img + v * 32) = (uint16_t)q[v / 2];
          *reinterpret_cast<uint16_t*>(img + (v + 1) * 32) = (uint16_t)(q[v / 2] >> 16);
        }
      }
      wave_lds_sync();

      // the piece of this channel
      const size_t piece = ((size_t)frame * 3 + c) * gm.l.tiles_y * gm.waves_per_row + (size_t)band * gm.waves_per_row + wr;
      int16_t* slot = ws.slots + piece * kPieceLevels;
      // all 16 words of the wave, idle columns included (their images hold the levels of zero pixels: zeros, so their masks are 0 and
      // nothing of them is stored): no trip count, so the reads go out together and the walk is straight-line code
      constexpr uint32_t kWaveWords = kCols * kColWords;
      int16_t l16[kWaveWords];
#pragma unroll
      for (uint32_t w = 0; w < kWaveWords; ++w)
        l16[w] = *reinterpret_cast<const int16_t*>(wave_slabs + (w / kColWords) * kSlab + image_at(w / kColWords, w % kColWords) + lane * 2);
      uint32_t base = 0;  // levels of the words before this one: wave-uniform
      uint64_t mine = 0;  // lane w keeps word w's mask: one store of the piece's masks at the end
#pragma unroll
      for (uint32_t w = 0; w < kWaveWords; ++w) {
        const uint64_t mask = __ballot(l16[w] != 0);
        if (l16[w] != 0) slot[base + lane_rank(mask)] = l16[w];
        if (lane == w) mine = mask;
        base += (uint32_t)__popcll(mask);
      }
      uint32_t* masks = ws.masks + (size_t)frame * ws_mask_pitch(gm) +
                        2 * ((((size_t)c * gm.l.tiles_y + band) * gm.l.tiles_x) * gm.l.words + word0);
      if (lane < nwords) store_mask(masks + 2 * lane, mine);
      if (lane == 0) ws.counts[piece] = base;
      wave_lds_sync();  // the slabs are rewritten: by the next layer's images, or by the next channel
    }
  }
  if constexpr (kLadderTally) {  // a place per wave and frame: a row of kMaxLadder counts, each at most 64 x 48
    if (it >= 0) k.rows[((size_t)wv * k.run + (uint32_t)it) * kMaxLadder + lane] = tally_row;
    tally_row = 0;
    if constexpr (kTallyMeasure) {
      if (it >= 0) k.drows[((size_t)wv * k.run + (uint32_t)it) * kMaxLadder + lane] = measure_row;
      measure_row = 0;
    }
  } else if constexpr (TALLY) {  // a wave's 64 x 48 coefficients: both sums fit their halves.  A place per wave and frame, no atomics: with
    // 65 280 adds into the one cache line that holds a batch's 32 counters the call took 0.709 ms at C3 (1, 640), with the stores 0.238
    // (profiles/dct_pack_delta_auto_c3.txt)
    if (it >= 0 && !(REDO && redo)) {
      const uint32_t sum = wave_sum(tally);
      if (lane == 0) *reinterpret_cast<uint2*>(k.tally + ((size_t)wv * k.run + (uint32_t)it) * 2) = make_uint2(sum & 0xFFFFu, sum >> 16);
    }
  }
  if constexpr (PERIOD > 1) {
    if (front() || (it & (REDO ? 1 : PERIOD - 1)) == 0) t_before = t;
    if (kMid && (it & 3) == 2) t_mid = t;
  } else {
    t_before = t;
  }
  if constexpr (REDO) {  // after frame 4k + 3, where frame 4k + 4 is in the run and predicted: frame 4k once more, then on
    bool again = !redo && (it & 3) == 3 && it + 1 < (int)run_len;
    if constexpr (!TALLY) again = again && !(k.key && k.key[run_first + (uint32_t)it + 1u] != 0);
    redo = again;
  }
  } while (DELTA && ((REDO && redo) || ++it < (int)run_len));
  if constexpr (MEASURE && COUNT) {
    // x = |c| - q s is exact in one fma and 256 x is exact (the header argues both), so e is an integer below 2^21 whatever the order:
    // e^2 < 2^41, a lane's 48 below 2^47, a wave's below 2^53
    uint64_t mine = 0, total = 0;  // lane k keeps entry k's total
    float prev_step = 0.f;         // (no step is 0: the first entry is always computed)
    for (uint32_t kk = 0; kk < k.lad.len; ++kk) {
      const float2 si = cls ? make_float2((float)k.lad.step[1][kk], k.li.inv[1][kk]) : make_float2((float)k.lad.step[0][kk], k.li.inv[0][kk]);
      if (!kMeasureShare || __ballot(si.x != prev_step) != 0) {  // the same in every lane; a lane whose step stayed computes the sum it had
        uint64_t s = 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
          for (int i = 0; i < 16; i += 2) {
            const f32x2 cf{kept[c][i], kept[c][i + 1]}, q = quant2_level(cf, si.x, si.y);
            const uint32_t e0 = (uint32_t)fabsf(rintf(256.f * __builtin_fmaf(-q.x, si.x, cf.x)));
            const uint32_t e1 = (uint32_t)fabsf(rintf(256.f * __builtin_fmaf(-q.y, si.x, cf.y)));
            s += (uint64_t)e0 * e0;
            s += (uint64_t)e1 * e1;
          }
        }
        for (uint32_t off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
        total = s;
      }
      prev_step = si.x;
      if (lane == kk) mine = total;
    }
    k.drows[(size_t)wv * kMaxLadder + lane] = mine;
  }
  if constexpr (COUNT) {  // the wave's row: bins 0 .. len - 2 as they are, bin len - 1 = the lanes' full counts
    uint32_t* hist = hist_all[tid >> 6];
    if (full) atomicAdd(&hist[k.lad.len - 1], full);
    wave_lds_sync();
    k.rows[(size_t)wv * kMaxLadder + lane] = hist[lane];
  }
}

template <int N>
__global__ __launch_bounds__(256) void dct_pack_kernel(DctPackArgs a) {
  dct_pack_body<N, false>(a, NoCountArgs{}, nullptr, nullptr);
}

template <int N>
__global__ __launch_bounds__(256) void dct_pack_layers_kernel(DctPackArgs a, LayerArgs k) {
  dct_pack_body<N, false, true>(a, k, nullptr, nullptr);
}

template <int N>
__global__ __launch_bounds__(256) void dct_pack_delta_kernel(DctPackArgs a, DeltaRunArgs k) {
  dct_pack_body<N, false, false, true>(a, k, nullptr, nullptr);
}

// the delta form's runs with both level counts of every frame instead of the pack
template <int N>
__global__ __launch_bounds__(256) void dct_delta_count_kernel(DctPackArgs a, DeltaTallyArgs k) {
  dct_pack_body<N, false, false, true, true>(a, k, nullptr, nullptr);
}

// the delta form with each frame's own pair of steps (a.steps), and the delta form's runs with the counts of every ladder entry
template <int N>
__global__ __launch_bounds__(256) void dct_pack_delta_group_kernel(DctPackArgs a, DeltaRunArgs k) {
  dct_pack_body<N, false, false, true, false, 1, false, false, true>(a, k, nullptr, nullptr);
}

template <int N>
__global__ __launch_bounds__(256) void dct_delta_ladder_kernel(DctPackArgs a, DeltaLadderArgs k) {
  dct_pack_body<N, false, false, true, true, 1, false, false, true>(a, k, nullptr, nullptr);
}

// the ladder tally with every entry's squared error beside its count
template <int N>
__global__ __launch_bounds__(256) void dct_delta_measure_kernel(DctPackArgs a, DeltaMeasureArgs k) {
  dct_pack_body<N, false, false, true, true, 1, false, true, true>(a, k, nullptr, nullptr);
}

// both with temporal layers: a frame against frame i - min(lowbit(i), PERIOD)
template <int N, int PERIOD>
__global__ __launch_bounds__(256) void dct_pack_delta_temporal_kernel(DctPackArgs a, DeltaRunArgs k) {
  dct_pack_body<N, false, false, true, false, PERIOD, PERIOD == 4 && kTemporalRedo>(a, k, nullptr, nullptr);
}

template <int N, int PERIOD>
__global__ __launch_bounds__(256) void dct_delta_temporal_count_kernel(DctPackArgs a, DeltaTallyArgs k) {
  dct_pack_body<N, false, false, true, true, PERIOD, PERIOD == 4 && kTemporalRedo>(a, k, nullptr, nullptr);
}

// One workgroup per frame: the waves' counts summed (u32 sums: any order gives the same counts), then the key frame by size,
// key[f] = forced[f] != 0 or (f == 0 and no frame before) or diff >= plain -- a tie is a key frame; the counts to the caller where asked.
struct DeltaSelectArgs {
  const uint32_t* tally;   // as DeltaTallyArgs::tally
  const uint32_t* forced;  // [n] or null
  uint32_t* key;           // [n]
  uint32_t* counts;        // [n][2] or null
  uint32_t waves_per_frame, run, has_prev;
};
__global__ __launch_bounds__(256) void dct_delta_select_kernel(DeltaSelectArgs a) {
  __shared__ uint32_t part[kThreads / 64][2];
  const uint32_t f = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t* mine = a.tally + (((size_t)(f / a.run) * a.waves_per_frame) * a.run + f % a.run) * 2;  // wave 0 of the frame's run, this frame
  uint32_t plain = 0, diff = 0;
  for (uint32_t w = threadIdx.x; w < a.waves_per_frame; w += kThreads) {
    const uint2 v = *reinterpret_cast<const uint2*>(mine + (size_t)w * a.run * 2);
    plain += v.x;
    diff += v.y;
  }
  plain = wave_sum(plain);
  diff = wave_sum(diff);
  if (lane == 0) {
    part[wave][0] = plain;
    part[wave][1] = diff;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  plain = part[0][0] + part[1][0] + part[2][0] + part[3][0];
  diff = part[0][1] + part[1][1] + part[2][1] + part[3][1];
  a.key[f] = ((a.forced && a.forced[f] != 0) || (f == 0 && !a.has_prev) || diff >= plain) ? 1u : 0u;
  if (a.counts) {
    a.counts[2 * (size_t)f] = plain;
    a.counts[2 * (size_t)f + 1] = diff;
  }
}

template <int N>
__global__ __launch_bounds__(256) void dct_count_kernel(DctPackArgs a, CountArgs k) {
  __shared__ float tau_tab[2][kTauTable];
  __shared__ uint32_t hist_all[kThreads / 64][kMaxLadder];
  dct_pack_body<N, true>(a, k, tau_tab, hist_all);
}

// the counting form with every ladder entry's squared error beside the counts
template <int N>
__global__ __launch_bounds__(256) void dct_measure_kernel(DctPackArgs a, MeasureArgs k) {
  __shared__ float tau_tab[2][kTauTable];
  __shared__ uint32_t hist_all[kThreads / 64][kMaxLadder];
  dct_pack_body<N, true, false, false, false, 1, false, true>(a, k, tau_tab, hist_all);
}

// Column `lane` of rows first, first + step, ... below count, summed over the workgroup's four waves: every thread gets its column's sum
// (unsigned sums: any order gives the same bytes).
template <typename T>  // u32 counts, u64 squared errors
__device__ __forceinline__ T sum_rows(const T* __restrict__ rows, uint32_t first, uint32_t step, uint32_t count, T (*part)[kMaxLadder]) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  T s = 0;
#pragma unroll 4
  for (uint32_t r = first + wave * step; r < count; r += (kThreads / 64) * step) s += rows[(size_t)r * kMaxLadder + lane];
  part[wave][lane] = s;
  __syncthreads();
  return part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane];
}

// grid (kSumParts, frames): part p of frame f = the sum of its waves' rows p, p + kSumParts, ...
__global__ __launch_bounds__(256) void dct_count_sum_kernel(uint32_t rows_per_frame, const uint32_t* __restrict__ rows, uint32_t* __restrict__ parts) {
  __shared__ uint32_t part[kThreads / 64][kMaxLadder];
  const uint32_t f = blockIdx.y;
  const uint32_t v = sum_rows(rows + (size_t)f * rows_per_frame * kMaxLadder, blockIdx.x, kSumParts, rows_per_frame, part);
  if (threadIdx.x < kMaxLadder) parts[((size_t)f * kSumParts + blockIdx.x) * kMaxLadder + threadIdx.x] = v;
}

// One workgroup per frame: bin k of the summed rows = the coefficients that exactly k + 1 entries keep (the last entry: all of them), so
// nz_k = the suffix sum from bin k; bytes_k = up16(levels_off + 2 nz_k); the choice, and the chosen pair's steps.
struct SelectArgs {
  uint64_t levels_off;
  const uint32_t* parts;
  const uint32_t* budget;
  FrameSteps* steps;
  uint32_t* choice;
};

__global__ __launch_bounds__(256) void dct_pack_select_kernel(Ladder lad, LadderInv li, SelectArgs a) {
  __shared__ uint32_t part[kThreads / 64][kMaxLadder];
  __shared__ uint64_t bytes[kMaxLadder];
  const uint32_t f = blockIdx.x, lane = threadIdx.x & 63u;
  uint32_t nz = sum_rows(a.parts + (size_t)f * kSumParts * kMaxLadder, 0, 1, kSumParts, part);
  if (threadIdx.x >= 64) return;
  for (uint32_t off = 1; off < 64; off <<= 1) {  // inclusive suffix sum over the lanes
    const uint32_t up = __shfl_down(nz, off, 64);
    if (lane + off < 64) nz += up;
  }
  bytes[lane] = up16(a.levels_off + 2ull * nz);
  wave_lds_sync();
  if (lane != 0) return;
  const uint32_t ch = budget_choice(bytes, lad.len, a.budget[f]), pick = ch & 0x7FFFFFFFu;
  a.choice[f] = ch;
  a.steps[f] = FrameSteps{lad.step[1][pick], lad.step[0][pick], li.inv[1][pick], li.inv[0][pick]};
}

// The quality call's sum: dct_count_sum_kernel on the counts and, in the same launch, on the squared errors.
__global__ __launch_bounds__(256) void dct_measure_sum_kernel(uint32_t rows_per_frame, const uint32_t* __restrict__ rows, uint32_t* __restrict__ parts,
                                                              const uint64_t* __restrict__ drows, uint64_t* __restrict__ dparts) {
  __shared__ uint32_t part[kThreads / 64][kMaxLadder];
  __shared__ uint64_t dpart[kThreads / 64][kMaxLadder];
  const uint32_t f = blockIdx.y;
  const uint32_t v = sum_rows(rows + (size_t)f * rows_per_frame * kMaxLadder, blockIdx.x, kSumParts, rows_per_frame, part);
  const uint64_t d = sum_rows(drows + (size_t)f * rows_per_frame * kMaxLadder, blockIdx.x, kSumParts, rows_per_frame, dpart);
  if (threadIdx.x < kMaxLadder) {
    parts[((size_t)f * kSumParts + blockIdx.x) * kMaxLadder + threadIdx.x] = v;
    dparts[((size_t)f * kSumParts + blockIdx.x) * kMaxLadder + threadIdx.x] = d;
  }
}

// One workgroup per frame: bytes_k as dct_pack_select_kernel has them and D_k = the summed squared errors of entry k; then
//   kq = the largest k with D_k <= target, 0 where there is none (D is not monotone along a ladder);
//   kb = budget_choice on bytes_k, 0 without a budget;
//   choice = max(kq, kb), bit 31 as kb has it, bit 30 where D[choice] > target;
// the chosen pair's steps, and the frame's row of the table where asked.
struct QualitySelectArgs {
  uint64_t levels_off;
  const uint32_t* parts;
  const uint64_t* dparts;
  const uint64_t* target;
  const uint32_t* budget;  // or null
  FrameSteps* steps;
  uint32_t* choice;
  uint64_t* distortion;    // [n][len] or null
};
__global__ __launch_bounds__(256) void dct_quality_select_kernel(Ladder lad, LadderInv li, QualitySelectArgs a) {
  __shared__ uint32_t part[kThreads / 64][kMaxLadder];
  __shared__ uint64_t dpart[kThreads / 64][kMaxLadder];
  __shared__ uint64_t bytes[kMaxLadder], dist[kMaxLadder];
  const uint32_t f = blockIdx.x, lane = threadIdx.x & 63u;
  uint32_t nz = sum_rows(a.parts + (size_t)f * kSumParts * kMaxLadder, 0, 1, kSumParts, part);
  const uint64_t d = sum_rows(a.dparts + (size_t)f * kSumParts * kMaxLadder, 0, 1, kSumParts, dpart);
  if (threadIdx.x >= 64) return;
  for (uint32_t off = 1; off < 64; off <<= 1) {  // inclusive suffix sum over the lanes
    const uint32_t up = __shfl_down(nz, off, 64);
    if (lane + off < 64) nz += up;
  }
  bytes[lane] = up16(a.levels_off + 2ull * nz);
  dist[lane] = d;
  if (a.distortion && lane < lad.len) a.distortion[(size_t)f * lad.len + lane] = d;
  wave_lds_sync();
  if (lane != 0) return;
  const uint64_t target = a.target[f];
  const uint32_t kb = a.budget ? budget_choice(bytes, lad.len, a.budget[f]) : 0u;
  uint32_t kq = 0;
  for (uint32_t i = 0; i < lad.len; ++i) kq = dist[i] <= target ? i : kq;
  const uint32_t pick = max(kq, kb & 0x7FFFFFFFu);
  a.choice[f] = pick | (kb & 0x80000000u) | (dist[pick] > target ? 0x40000000u : 0u);
  a.steps[f] = FrameSteps{lad.step[1][pick], lad.step[0][pick], li.inv[1][pick], li.inv[0][pick]};
}

// The ladder tally's sum.  grid (kSumParts, frames): part p of frame f = the sum of its waves' rows p, p + kSumParts, ...  A wave's rows
// of the frames of its run lie side by side, so the rows of one frame are `run` rows apart.
__global__ __launch_bounds__(256) void dct_delta_ladder_sum_kernel(uint32_t waves_per_frame, uint32_t run, const uint32_t* __restrict__ rows,
                                                                   uint32_t* __restrict__ parts) {
  __shared__ uint32_t part[kThreads / 64][kMaxLadder];
  const uint32_t f = blockIdx.y;
  const uint32_t* mine = rows + (((size_t)(f / run) * waves_per_frame) * run + f % run) * kMaxLadder;  // wave 0 of the frame's run, this frame
  const uint32_t v = sum_rows(mine, blockIdx.x * run, kSumParts * run, waves_per_frame * run, part);
  if (threadIdx.x < kMaxLadder) parts[((size_t)f * kSumParts + blockIdx.x) * kMaxLadder + threadIdx.x] = v;
}

// One workgroup per frame; the one of a frame that starts a group (frame 0, or a set flag) works, the others leave.  Frame by frame up
// to the next start: the parts' sum = count[g][k] in lane k (to the caller's table where asked), bytes_k(g) = up16(levels_off + 2 count)
// and the budget, both summed in 64 bits.  The choice is the first lane whose sum fits, from a ballot over ALL entries: the counts of
// differences are not monotone along a ladder, so nothing of the counting form's suffix sums carries over and no entry is skipped.
// None fits: the last entry, bit 31 set.  Every frame of the group gets the value and the pair's steps.
struct GroupSelectArgs {
  uint64_t levels_off;
  const uint32_t* parts;
  const uint32_t* key;     // [n] or null: one group
  const uint32_t* budget;  // [n]
  FrameSteps* steps;
  uint32_t* choice;
  uint32_t* counts;        // [n][len] or null
  uint32_t n_frames;
};
__global__ __launch_bounds__(256) void dct_delta_group_select_kernel(Ladder lad, LadderInv li, GroupSelectArgs a) {
  __shared__ uint32_t part[kThreads / 64][kMaxLadder];
  const uint32_t first = blockIdx.x, lane = threadIdx.x & 63u;
  if (first != 0 && !(a.key && a.key[first] != 0)) return;  // (the same in every thread, as the loop's trips below)
  uint64_t bytes = 0, allowed = 0;
  uint32_t end = first;
  do {
    const uint32_t nz = sum_rows(a.parts + (size_t)end * kSumParts * kMaxLadder, 0, 1, kSumParts, part);
    bytes += up16(a.levels_off + 2ull * nz);
    allowed += a.budget[end];
    if (a.counts && threadIdx.x < lad.len) a.counts[(size_t)end * lad.len + threadIdx.x] = nz;
    __syncthreads();  // part is rewritten by the next frame's sum
    ++end;
  } while (end < a.n_frames && !(a.key && a.key[end] != 0));
  const uint64_t fits = __ballot(lane < lad.len && bytes <= allowed);  // every wave holds all entries: lane k has entry k
  const uint32_t ch = fits ? (uint32_t)__builtin_ctzll(fits) : ((lad.len - 1) | 0x80000000u), pick = ch & 0x7FFFFFFFu;
  const FrameSteps fs{lad.step[1][pick], lad.step[0][pick], li.inv[1][pick], li.inv[0][pick]};
  for (uint32_t g = first + threadIdx.x; g < end; g += kThreads) {
    a.choice[g] = ch;
    a.steps[g] = fs;
  }
}

// The measuring tally's sum: dct_delta_ladder_sum_kernel on the counts and, in the same launch, on the squared errors, whose rows lie
// the same way (drun == run; the two-pass build's measuring form leaves them frame by frame: drun == 1).
__global__ __launch_bounds__(256) void dct_delta_measure_sum_kernel(uint32_t waves_per_frame, uint32_t run, const uint32_t* __restrict__ rows,
                                                                    uint32_t* __restrict__ parts, uint32_t drun, const uint64_t* __restrict__ drows,
                                                                    uint64_t* __restrict__ dparts) {
  __shared__ uint32_t part[kThreads / 64][kMaxLadder];
  __shared__ uint64_t dpart[kThreads / 64][kMaxLadder];
  const uint32_t f = blockIdx.y;
  const size_t mine = (((size_t)(f / run) * waves_per_frame) * run + f % run) * kMaxLadder;  // wave 0 of the frame's run, this frame
  const uint32_t v = sum_rows(rows + mine, blockIdx.x * run, kSumParts * run, waves_per_frame * run, part);
  const size_t dmine = (((size_t)(f / drun) * waves_per_frame) * drun + f % drun) * kMaxLadder;
  const uint64_t d = sum_rows(drows + dmine, blockIdx.x * drun, kSumParts * drun, waves_per_frame * drun, dpart);
  if (threadIdx.x < kMaxLadder) {
    parts[((size_t)f * kSumParts + blockIdx.x) * kMaxLadder + threadIdx.x] = v;
    dparts[((size_t)f * kSumParts + blockIdx.x) * kMaxLadder + threadIdx.x] = d;
  }
}

// One workgroup per frame; the one of a frame that starts a group works, as in dct_delta_group_select_kernel.  Frame by frame: count and
// D of entry k in lane k (to the caller's tables where asked), the group's bytes and budget summed in 64 bits, and whether every frame so
// far meets its own target at the entry.  Two ballots over ALL entries -- Q, the entries every frame meets its target at, and F, those
// whose bytes fit (every entry without a budget) -- and the choice include/svc_hip_delta_quality.h states: max(Q & F); else min(F), bit 30;
// else the last entry, bit 31, and bit 30 where it is not in Q.  Every frame of the group gets the value and the pair's steps.
struct GroupQualitySelectArgs {
  uint64_t levels_off;
  const uint32_t* parts;
  const uint64_t* dparts;
  const uint32_t* key;      // [n] or null: one group
  const uint64_t* target;   // [n]
  const uint32_t* budget;   // [n] or null: no cap
  FrameSteps* steps;
  uint32_t* choice;
  uint32_t* counts;         // [n][len] or null
  uint64_t* distortion;     // [n][len] or null
  uint32_t n_frames;
};
__global__ __launch_bounds__(256) void dct_delta_quality_select_kernel(Ladder lad, LadderInv li, GroupQualitySelectArgs a) {
  __shared__ uint32_t part[kThreads / 64][kMaxLadder];
  __shared__ uint64_t dpart[kThreads / 64][kMaxLadder];
  const uint32_t first = blockIdx.x, lane = threadIdx.x & 63u;
  if (first != 0 && !(a.key && a.key[first] != 0)) return;  // (the same in every thread, as the loop's trips below)
  uint64_t bytes = 0, allowed = 0;
  bool met = true;
  uint32_t end = first;
  do {
    const uint32_t nz = sum_rows(a.parts + (size_t)end * kSumParts * kMaxLadder, 0, 1, kSumParts, part);
    const uint64_t d = sum_rows(a.dparts + (size_t)end * kSumParts * kMaxLadder, 0, 1, kSumParts, dpart);
    bytes += up16(a.levels_off + 2ull * nz);
    if (a.budget) allowed += a.budget[end];
    met = met && d <= a.target[end];
    if (threadIdx.x < lad.len) {
      if (a.counts) a.counts[(size_t)end * lad.len + threadIdx.x] = nz;
      if (a.distortion) a.distortion[(size_t)end * lad.len + threadIdx.x] = d;
    }
    __syncthreads();  // part and dpart are rewritten by the next frame's sums
    ++end;
  } while (end < a.n_frames && !(a.key && a.key[end] != 0));
  // every wave holds all entries: lane k has entry k
  const uint64_t q = __ballot(lane < lad.len && met), f = __ballot(lane < lad.len && (!a.budget || bytes <= allowed));
  uint32_t ch;
  if (q & f) ch = 63u - (uint32_t)__builtin_clzll(q & f);
  else if (f) ch = (uint32_t)__builtin_ctzll(f) | 0x40000000u;
  else ch = (lad.len - 1) | 0x80000000u | ((q >> (lad.len - 1)) & 1ull ? 0u : 0x40000000u);
  const uint32_t pick = ch & 0x3FFFFFFFu;
  const FrameSteps fs{lad.step[1][pick], lad.step[0][pick], li.inv[1][pick], li.inv[0][pick]};
  for (uint32_t g = first + threadIdx.x; g < end; g += kThreads) {
    a.choice[g] = ch;
    a.steps[g] = fs;
  }
}

// one workgroup per frame: piece counts -> exclusive prefixes (in place), the frame's level count and size
__global__ __launch_bounds__(256) void dct_pack_scan_kernel(uint32_t pieces, uint64_t levels_off, DctPackWs ws) {
  __shared__ uint32_t red[kThreads / 64];
  const uint32_t f = blockIdx.x;
  uint32_t* cnt = ws.counts + (size_t)f * pieces;
  const uint32_t carry = scan_counts(cnt, cnt, pieces, 0, red);
  if (threadIdx.x == 0) {
    ws.frame_levels[f] = carry;
    ws.frame_bytes[f] = (uint32_t)up16(levels_off + 2ull * carry);
  }
}

struct AssembleArgs {
  PackGeom g;
  uint32_t fg, bg;
  const FrameSteps* steps;  // [n] each frame's own pair for its header (the budgeted call), or null: fg / bg
  const uint32_t* types;  // [n][mvb]
  DctPackWs ws;
  uint8_t* out;
  uint64_t* offsets;      // [n + 1]
};

// grid (workgroups per frame, frames): the frame's sections to their final place.  Masks and pieces are dealt over the frame's
// workgroups; workgroup 0 also writes the header, the types, the pad and offsets[f + 1].
__global__ __launch_bounds__(256) void dct_pack_assemble_kernel(AssembleArgs a) {
  __shared__ uint64_t frame_off;
  const PackGeom& g = a.g;
  const uint32_t f = blockIdx.y, wave = threadIdx.x >> 6;
  frame_offset_to_lds(a.ws.frame_bytes, f, &frame_off);
  __syncthreads();
  uint8_t* frame = a.out + frame_off;
  const uint32_t level_count = a.ws.frame_levels[f];

  // masks: u32 copies (the section is only 4-byte aligned when the MV block count is odd)
  const uint32_t* msrc = a.ws.masks + (size_t)f * ws_mask_pitch(g);
  uint32_t* mdst = reinterpret_cast<uint32_t*>(frame + g.l.masks_off);
  for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < g.mask_dwords; i += gridDim.x * kThreads) mdst[i] = msrc[i];

  // levels: a wave per piece, a run at a 2-byte aligned place (the prefix is any number)
  const uint32_t* cnt = a.ws.counts + (size_t)f * g.pieces;
  uint16_t* ldst = reinterpret_cast<uint16_t*>(frame + g.l.levels_off);
  for (uint32_t p = blockIdx.x * (kThreads / 64) + wave; p < g.pieces; p += gridDim.x * (kThreads / 64)) {
    const uint32_t prefix = cnt[p], end = p + 1 < g.pieces ? cnt[p + 1] : level_count;
    store_level_run(reinterpret_cast<const uint16_t*>(a.ws.slots + ((size_t)f * g.pieces + p) * kPieceLevels), end - prefix, ldst + prefix);
  }

  if (blockIdx.x != 0) return;
  // header (inexact = 0: every level reproduces its quantised coefficient), types, pad, offsets
  const uint32_t fg = a.steps ? a.steps[f].fg : a.fg, bg = a.steps ? a.steps[f].bg : a.bg;
  write_frame_edges(frame, FrameHead{g.w, g.h, g.n_block, g.n_block, g.mvbw, g.mvbh, fg, bg, level_count, 0, a.ws.frame_bytes[f]},
                    a.types + (size_t)f * g.l.mvb, g.l.mvb, g.l.levels_off, kThreads, a.offsets, f, frame_off);
}

// the format's geometry, then what the fused kernels take: the tuned transform's blocks on whole 16-pixel segments
int validate_pack_geom(const char* what, uint32_t w, uint32_t h, uint32_t block, uint32_t mvbw, uint32_t mvbh) {
  const int rc = validate_geom(what, w, h, block, block, mvbw, mvbh);
  if (rc) return rc;
  if (block != 8 && block != 16)
    return fail(SVC_ERR_UNSUPPORTED, "%s: transform block %ux%u (supported: 8x8, 16x16; for any other call svc_hip_dct_quant_frames, then "
                                     "svc_hip_pack_levels_frames)", what, block, block);
  if (w % 16 != 0)
    return fail(SVC_ERR_UNSUPPORTED, "%s: frame width %u is not a multiple of 16 (call svc_hip_dct_quant_frames, then svc_hip_pack_levels_frames)",
                what, w);
  return SVC_OK;
}

// the period of the temporal calls, checked right after the geometry (the rule of the temporal calls on streams, csrc/levels.hip)
int validate_pack_period(const char* what, uint32_t period) {
  SVC_REQUIRE(period == 1 || period == 2 || period == 4, "%s: period %u (supported: 1, 2, 4)", what, period);
  return SVC_OK;
}

// the formats' limits with SVCQ's worst case, and one launch's worth of waves
int validate_pack_limits(const char* what, uint32_t n, const PackGeom& g) {
  const int rc = validate_limits(what, n, g.w, g.h, g.n_block, g.n_block, g.l.max_bytes);
  if (rc) return rc;
  if ((uint64_t)n * g.l.tiles_y * g.waves_per_row > 0x7FFFFFFFull) return fail(SVC_ERR_UNSUPPORTED, "%s: too many segment columns for one launch", what);
  return SVC_OK;
}

// what follows the transform, for the layer whose pieces are in ws: the scan and the assemble pass, with fg / bg in the headers or
// each frame's own steps
int enqueue_assemble(const char* what, const DctPackArgs& a, const DctPackWs& ws, uint32_t n_frames, uint32_t fg, uint32_t bg, uint8_t* d_out,
                     uint64_t* d_frame_offsets, hipStream_t s) {
  const PackGeom& g = a.g;
  const dim3 blk(kThreads);
  hipLaunchKernelGGL(dct_pack_scan_kernel, dim3(n_frames), blk, 0, s, g.pieces, g.l.levels_off, ws);
  const int rc = check_launch(what, "scan");
  if (rc) return rc;
  const AssembleArgs as{g, fg, bg, a.steps, a.types, ws, d_out, d_frame_offsets};
  // a wave per piece and trip; enough workgroups per frame to keep a single 4K frame busy, few enough that a batch is not all launch
  const uint32_t per_frame = std::min<uint32_t>(std::max<uint32_t>(div_up(g.pieces, 32), 1), 256);
  hipLaunchKernelGGL(dct_pack_assemble_kernel, dim3(per_frame, n_frames), blk, 0, s, as);
  return check_launch(what, "assemble");
}

// the fused pack's three launches, with a.fg_step / a.bg_step (fg, bg in the headers) or each frame's own steps
int enqueue_dct_pack(const char* what, DctPackArgs& a, uint32_t n_frames, uint32_t fg, uint32_t bg, uint8_t* d_out, uint64_t* d_frame_offsets,
                     hipStream_t s) {
  const dim3 grid(div_up(a.total_waves, 4)), blk(kThreads);
  if (a.g.n_block == 8) hipLaunchKernelGGL(dct_pack_kernel<8>, grid, blk, 0, s, a);
  else hipLaunchKernelGGL(dct_pack_kernel<16>, grid, blk, 0, s, a);
  const int rc = check_launch(what, "transform");
  if (rc) return rc;
  return enqueue_assemble(what, a, a.ws, n_frames, fg, bg, d_out, d_frame_offsets, s);
}

// the delta form's kernel (period 1) or the temporal form's, for a block of 8 or 16 and a period of 1, 2 or 4: the pack, and its counting
void launch_delta_pack(uint32_t block, uint32_t period, dim3 grid, hipStream_t s, const DctPackArgs& a, const DeltaRunArgs& k) {
  const dim3 blk(kThreads);
  if (block == 8) {
    if (period == 1) hipLaunchKernelGGL(dct_pack_delta_kernel<8>, grid, blk, 0, s, a, k);
    else if (period == 2) hipLaunchKernelGGL((dct_pack_delta_temporal_kernel<8, 2>), grid, blk, 0, s, a, k);
    else hipLaunchKernelGGL((dct_pack_delta_temporal_kernel<8, 4>), grid, blk, 0, s, a, k);
  } else {
    if (period == 1) hipLaunchKernelGGL(dct_pack_delta_kernel<16>, grid, blk, 0, s, a, k);
    else if (period == 2) hipLaunchKernelGGL((dct_pack_delta_temporal_kernel<16, 2>), grid, blk, 0, s, a, k);
    else hipLaunchKernelGGL((dct_pack_delta_temporal_kernel<16, 4>), grid, blk, 0, s, a, k);
  }
}
void launch_delta_count(uint32_t block, uint32_t period, dim3 grid, hipStream_t s, const DctPackArgs& a, const DeltaTallyArgs& k) {
  const dim3 blk(kThreads);
  if (block == 8) {
    if (period == 1) hipLaunchKernelGGL(dct_delta_count_kernel<8>, grid, blk, 0, s, a, k);
    else if (period == 2) hipLaunchKernelGGL((dct_delta_temporal_count_kernel<8, 2>), grid, blk, 0, s, a, k);
    else hipLaunchKernelGGL((dct_delta_temporal_count_kernel<8, 4>), grid, blk, 0, s, a, k);
  } else {
    if (period == 1) hipLaunchKernelGGL(dct_delta_count_kernel<16>, grid, blk, 0, s, a, k);
    else if (period == 2) hipLaunchKernelGGL((dct_delta_temporal_count_kernel<16, 2>), grid, blk, 0, s, a, k);
    else hipLaunchKernelGGL((dct_delta_temporal_count_kernel<16, 4>), grid, blk, 0, s, a, k);
  }
}

// the delta form's three launches: a wave per piece and RUN of k.n_frames frames, then the fused pack's scan and assemble
int enqueue_dct_pack_delta(const char* what, DctPackArgs& a, const DeltaRunArgs& k, uint32_t fg, uint32_t bg, uint8_t* d_out,
                           uint64_t* d_frame_offsets, hipStream_t s, uint32_t period = 1) {
  a.total_waves = div_up(k.n_frames, k.run) * a.g.l.tiles_y * a.g.waves_per_row;
  launch_delta_pack(a.g.n_block, period, dim3(div_up(a.total_waves, 4)), s, a, k);
  const int rc = check_launch(what, "transform");
  if (rc) return rc;
  return enqueue_assemble(what, a, a.ws, k.n_frames, fg, bg, d_out, d_frame_offsets, s);
}

// the auto call's workspace: the delta call's, then both level counts of every wave's piece of every frame, whole runs
struct DeltaAutoWs {
  DctPackWs pack;
  uint32_t* tally;  // [runs][waves of a frame][run][2], run = kDeltaRun or kTemporalRun
};
DeltaAutoWs delta_auto_ws(Carver& c, uint32_t n, const PackGeom& g) {
  DeltaAutoWs s;
  s.pack = pack_ws(c, n, g);
  // (whole runs of either length: the two are one number unless a probe build sets another kDeltaRun)
  s.tally = c.take<uint32_t>(2ull * std::max(kDeltaRun * div_up(n, kDeltaRun), kTemporalRun * div_up(n, kTemporalRun)) * g.l.tiles_y * g.waves_per_row);
  return s;
}

// the group-budget call's workspace: the delta call's, then every wave's row of counts per frame (whole runs), their parts and the steps
struct DeltaBudgetWs {
  DctPackWs pack;
  uint32_t* rows;     // as DeltaLadderArgs::rows
  uint32_t* parts;    // [n][kSumParts][kMaxLadder]
  FrameSteps* steps;  // [n]
};
DeltaBudgetWs delta_budget_ws(Carver& c, uint32_t n, const PackGeom& g) {
  DeltaBudgetWs s;
  s.pack = pack_ws(c, n, g);
  s.rows = c.take<uint32_t>((uint64_t)kMaxLadder * kDeltaRun * div_up(n, kDeltaRun) * g.l.tiles_y * g.waves_per_row, false);
  s.parts = c.take<uint32_t>((uint64_t)kMaxLadder * n * kSumParts, false);
  s.steps = c.take<FrameSteps>(n);
  return s;
}

// the group-quality call's workspace: the group-budget call's (so that call and the fixed delta call run on it too), then every wave's
// row of squared errors per frame, laid out as the counts' rows, and their parts
struct DeltaQualityWs {
  DeltaBudgetWs budget;
  uint64_t* drows;   // as DeltaMeasureArgs::drows
  uint64_t* dparts;  // [n][kSumParts][kMaxLadder]
  uint32_t* crows;   // kDeltaQualityTwoPass: [n][waves of a frame][kMaxLadder], the measuring form's rows of counts, which nothing reads
};
DeltaQualityWs delta_quality_ws(Carver& c, uint32_t n, const PackGeom& g) {
  DeltaQualityWs s;
  s.budget = delta_budget_ws(c, n, g);
  s.drows = c.take<uint64_t>((uint64_t)kMaxLadder * kDeltaRun * div_up(n, kDeltaRun) * g.l.tiles_y * g.waves_per_row, false);
  s.dparts = c.take<uint64_t>((uint64_t)kMaxLadder * n * kSumParts, false);
  s.crows = kDeltaQualityTwoPass ? c.take<uint32_t>((uint64_t)kMaxLadder * n * g.l.tiles_y * g.waves_per_row, false) : nullptr;
  return s;
}

}  // namespace
}  // namespace svc

using namespace svc;

extern "C" {

uint64_t svc_hip_dct_pack_levels_workspace_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h, uint32_t block, uint32_t mv_block_w,
                                                 uint32_t mv_block_h) {
  if (validate_pack_geom("dct_pack_levels_workspace_bytes", frame_w, frame_h, block, mv_block_w, mv_block_h)) return 0;
  const PackGeom g = make_pack_geom(frame_w, frame_h, block, mv_block_w, mv_block_h);
  if (validate_pack_limits("dct_pack_levels_workspace_bytes", n_frames, g)) return 0;
  return layout_bytes(pack_ws, n_frames, g);
}

// Checked in the order of the SVCQ entry points, whatever n_frames: geometry, steps, limits, sizes, then pointers.
int svc_hip_dct_pack_levels_frames(const uint8_t* d_bgr, uint64_t frame_stride_bytes, uint32_t n_frames, uint32_t frame_w, uint32_t frame_h,
                                   uint32_t block, const uint32_t* d_block_types, uint32_t mv_block_w, uint32_t mv_block_h, uint32_t fg_step,
                                   uint32_t bg_step, uint8_t* d_workspace, uint64_t workspace_bytes, uint8_t* d_out, uint64_t out_capacity,
                                   uint64_t* d_frame_offsets, void* stream) {
  int rc = validate_pack_geom("dct_pack_levels", frame_w, frame_h, block, mv_block_w, mv_block_h);
  if (rc) return rc;
  SVC_REQUIRE(frame_stride_bytes >= 3ull * frame_w * frame_h && frame_stride_bytes % 16 == 0,
              "dct_pack_levels: a frame stride of %llu B (at least the frame's %llu B, a multiple of 16)", (unsigned long long)frame_stride_bytes,
              3ull * frame_w * frame_h);
  SVC_REQUIRE(fg_step > 0 && bg_step > 0, "dct_pack_levels: quant steps must be positive");
  // (the pack's int16 bound, 255 * sqrt(tile area) / step <= 32767, holds for every step at 8x8 and 16x16: at most 4080)
  const PackGeom g = make_pack_geom(frame_w, frame_h, block, mv_block_w, mv_block_h);
  if ((rc = validate_pack_limits("dct_pack_levels", n_frames, g))) return rc;
  if ((rc = require_workspace("dct_pack_levels", workspace_bytes, layout_bytes(pack_ws, n_frames, g)))) return rc;
  if ((rc = require_capacity("dct_pack_levels", "output", out_capacity, n_frames * g.l.max_bytes))) return rc;
  if (n_frames == 0) return SVC_OK;  // empty batch: nothing to enqueue
  SVC_REQUIRE(d_bgr && d_block_types && d_workspace && d_out && d_frame_offsets, "dct_pack_levels: null pointer");
  SVC_REQUIRE(aligned(d_bgr, 16) && aligned(d_out, 16) && aligned(d_workspace, 16) && aligned(d_frame_offsets, 8) && aligned(d_block_types, 4),
              "dct_pack_levels: frames, output and workspace must be 16-byte aligned, offsets 8-byte");
  hipStream_t s = static_cast<hipStream_t>(stream);
  DctPackArgs a{};
  a.bgr = d_bgr;
  a.frame_stride = frame_stride_bytes;
  a.g = g;
  a.total_waves = n_frames * g.l.tiles_y * g.waves_per_row;
  a.types = d_block_types;
  a.fg_step = (float)fg_step;  // libs/decoder.cpp:141 divides a float by an unsigned
  a.bg_step = (float)bg_step;
  a.fg_inv = 1.0f / a.fg_step;
  a.bg_inv = 1.0f / a.bg_step;
  a.ws = carve(d_workspace, pack_ws, n_frames, g);
  return enqueue_dct_pack("dct_pack_levels", a, n_frames, fg_step, bg_step, d_out, d_frame_offsets, s);
}

uint64_t svc_hip_dct_pack_delta_workspace_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h, uint32_t block, uint32_t mv_block_w,
                                                uint32_t mv_block_h) {
  if (validate_pack_geom("dct_pack_delta_workspace_bytes", frame_w, frame_h, block, mv_block_w, mv_block_h)) return 0;
  const PackGeom g = make_pack_geom(frame_w, frame_h, block, mv_block_w, mv_block_h);
  if (validate_pack_limits("dct_pack_delta_workspace_bytes", n_frames, g)) return 0;
  return layout_bytes(pack_ws, n_frames, g);  // the fused pack's: the frame before lives in registers
}

// Checked in the order of svc_hip_dct_pack_levels_frames: geometry, stride, steps, limits, sizes; n_frames == 0 then returns SVC_OK; then
// pointers, the pairing of d_prev_bgr and d_prev_types among them.
// `period`: 1 for svc_hip_dct_pack_delta_frames, else the temporal call's, checked right after the geometry.
static int dct_pack_delta(const char* what, uint32_t period, const uint8_t* d_bgr, uint64_t frame_stride_bytes, uint32_t n_frames, uint32_t frame_w, uint32_t frame_h,
                                  uint32_t block, const uint32_t* d_block_types, uint32_t mv_block_w, uint32_t mv_block_h, uint32_t fg_step,
                                  uint32_t bg_step, const uint8_t* d_prev_bgr, const uint32_t* d_prev_types, const uint32_t* d_key,
                                  uint8_t* d_workspace, uint64_t workspace_bytes, uint8_t* d_out, uint64_t out_capacity,
                                  uint64_t* d_frame_offsets, void* stream) {
  int rc = validate_pack_geom(what, frame_w, frame_h, block, mv_block_w, mv_block_h);
  if (rc) return rc;
  if ((rc = validate_pack_period(what, period))) return rc;
  SVC_REQUIRE(frame_stride_bytes >= 3ull * frame_w * frame_h && frame_stride_bytes % 16 == 0,
              "%s: a frame stride of %llu B (at least the frame's %llu B, a multiple of 16)", what, (unsigned long long)frame_stride_bytes,
              3ull * frame_w * frame_h);
  SVC_REQUIRE(fg_step > 0 && bg_step > 0, "%s: quant steps must be positive", what);
  // (the pack's int16 bound holds for every step at 8x8 and 16x16, as in svc_hip_dct_pack_levels_frames; a difference wraps by definition)
  const PackGeom g = make_pack_geom(frame_w, frame_h, block, mv_block_w, mv_block_h);
  if ((rc = validate_pack_limits(what, n_frames, g))) return rc;
  if ((rc = require_workspace(what, workspace_bytes, layout_bytes(pack_ws, n_frames, g)))) return rc;
  if ((rc = require_capacity(what, "output", out_capacity, n_frames * g.l.max_bytes))) return rc;
  if (n_frames == 0) return SVC_OK;  // empty batch: nothing to enqueue
  SVC_REQUIRE(d_bgr && d_block_types && d_workspace && d_out && d_frame_offsets, "%s: null pointer", what);
  SVC_REQUIRE((d_prev_bgr == nullptr) == (d_prev_types == nullptr),
              "%s: the frame before frame 0 is its pixels and its types: d_prev_bgr and d_prev_types are given together or not at all", what);
  SVC_REQUIRE(aligned(d_bgr, 16) && aligned(d_prev_bgr, 16) && aligned(d_out, 16) && aligned(d_workspace, 16) && aligned(d_frame_offsets, 8) &&
                  aligned(d_block_types, 4) && aligned(d_prev_types, 4) && aligned(d_key, 4),
              "%s: frames, d_prev_bgr, output and workspace must be 16-byte aligned, offsets 8-byte, types and key flags 4-byte", what);
  hipStream_t s = static_cast<hipStream_t>(stream);
  DctPackArgs a{};
  a.bgr = d_bgr;
  a.frame_stride = frame_stride_bytes;
  a.g = g;
  a.types = d_block_types;
  a.fg_step = (float)fg_step;
  a.bg_step = (float)bg_step;
  a.fg_inv = 1.0f / a.fg_step;
  a.bg_inv = 1.0f / a.bg_step;
  a.ws = carve(d_workspace, pack_ws, n_frames, g);
  const DeltaRunArgs k{d_prev_bgr, d_prev_types, d_key, n_frames, period == 1 ? kDeltaRun : kTemporalRun, fg_step == bg_step ? 1u : 0u};
  return enqueue_dct_pack_delta(what, a, k, fg_step, bg_step, d_out, d_frame_offsets, s, period);
}

int svc_hip_dct_pack_delta_frames(const uint8_t* d_bgr, uint64_t frame_stride_bytes, uint32_t n_frames, uint32_t frame_w, uint32_t frame_h,
                                  uint32_t block, const uint32_t* d_block_types, uint32_t mv_block_w, uint32_t mv_block_h, uint32_t fg_step,
                                  uint32_t bg_step, const uint8_t* d_prev_bgr, const uint32_t* d_prev_types, const uint32_t* d_key,
                                  uint8_t* d_workspace, uint64_t workspace_bytes, uint8_t* d_out, uint64_t out_capacity,
                                  uint64_t* d_frame_offsets, void* stream) {
  return dct_pack_delta("dct_pack_delta", 1, d_bgr, frame_stride_bytes, n_frames, frame_w, frame_h, block, d_block_types, mv_block_w, mv_block_h,
                        fg_step, bg_step, d_prev_bgr, d_prev_types, d_key, d_workspace, workspace_bytes, d_out, out_capacity, d_frame_offsets,
                        stream);
}

uint64_t svc_hip_dct_pack_delta_auto_workspace_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h, uint32_t block, uint32_t mv_block_w,
                                                     uint32_t mv_block_h) {
  if (validate_pack_geom("dct_pack_delta_auto_workspace_bytes", frame_w, frame_h, block, mv_block_w, mv_block_h)) return 0;
  const PackGeom g = make_pack_geom(frame_w, frame_h, block, mv_block_w, mv_block_h);
  if (validate_pack_limits("dct_pack_delta_auto_workspace_bytes", n_frames, g)) return 0;
  return layout_bytes(delta_auto_ws, n_frames, g);
}

// Checked as svc_hip_dct_pack_delta_frames, the new pointers where it checks d_key.  Five launches whatever n_frames: the counting
// kernel, the selection, then that call's own three with d_key_out as their flags.
// `period` as in dct_pack_delta.
static int dct_pack_delta_auto(const char* what, uint32_t period, const uint8_t* d_bgr, uint64_t frame_stride_bytes, uint32_t n_frames, uint32_t frame_w,
                                       uint32_t frame_h, uint32_t block, const uint32_t* d_block_types, uint32_t mv_block_w,
                                       uint32_t mv_block_h, uint32_t fg_step, uint32_t bg_step, const uint8_t* d_prev_bgr,
                                       const uint32_t* d_prev_types, const uint32_t* d_forced, uint8_t* d_workspace, uint64_t workspace_bytes,
                                       uint8_t* d_out, uint64_t out_capacity, uint64_t* d_frame_offsets, uint32_t* d_key_out,
                                       uint32_t* d_level_counts, void* stream) {
  int rc = validate_pack_geom(what, frame_w, frame_h, block, mv_block_w, mv_block_h);
  if (rc) return rc;
  if ((rc = validate_pack_period(what, period))) return rc;
  SVC_REQUIRE(frame_stride_bytes >= 3ull * frame_w * frame_h && frame_stride_bytes % 16 == 0,
              "%s: a frame stride of %llu B (at least the frame's %llu B, a multiple of 16)", what,
              (unsigned long long)frame_stride_bytes, 3ull * frame_w * frame_h);
  SVC_REQUIRE(fg_step > 0 && bg_step > 0, "%s: quant steps must be positive", what);
  const PackGeom g = make_pack_geom(frame_w, frame_h, block, mv_block_w, mv_block_h);
  if ((rc = validate_pack_limits(what, n_frames, g))) return rc;
  if ((rc = require_workspace(what, workspace_bytes, layout_bytes(delta_auto_ws, n_frames, g)))) return rc;
  if ((rc = require_capacity(what, "output", out_capacity, n_frames * g.l.max_bytes))) return rc;
  if (n_frames == 0) return SVC_OK;  // empty batch: nothing to enqueue
  SVC_REQUIRE(d_bgr && d_block_types && d_workspace && d_out && d_frame_offsets && d_key_out, "%s: null pointer", what);
  SVC_REQUIRE((d_prev_bgr == nullptr) == (d_prev_types == nullptr),
              "%s: the frame before frame 0 is its pixels and its types: d_prev_bgr and d_prev_types are given together or "
              "not at all", what);
  SVC_REQUIRE(aligned(d_bgr, 16) && aligned(d_prev_bgr, 16) && aligned(d_out, 16) && aligned(d_workspace, 16) && aligned(d_frame_offsets, 8) &&
                  aligned(d_block_types, 4) && aligned(d_prev_types, 4) && aligned(d_forced, 4) && aligned(d_key_out, 4) &&
                  aligned(d_level_counts, 4),
              "%s: frames, d_prev_bgr, output and workspace must be 16-byte aligned, offsets 8-byte, types, forced flags, key "
              "flags and level counts 4-byte", what);
  hipStream_t s = static_cast<hipStream_t>(stream);
  DctPackArgs a{};
  a.bgr = d_bgr;
  a.frame_stride = frame_stride_bytes;
  a.g = g;
  a.types = d_block_types;
  a.fg_step = (float)fg_step;
  a.bg_step = (float)bg_step;
  a.fg_inv = 1.0f / a.fg_step;
  a.bg_inv = 1.0f / a.bg_step;
  const DeltaAutoWs ws = carve(d_workspace, delta_auto_ws, n_frames, g);
  a.ws = ws.pack;
  const uint32_t run = period == 1 ? kDeltaRun : kTemporalRun;
  a.total_waves = div_up(n_frames, run) * g.l.tiles_y * g.waves_per_row;  // a wave per piece and RUN, as the pack below
  DeltaTallyArgs t{};
  static_cast<DeltaRunArgs&>(t) = DeltaRunArgs{d_prev_bgr, d_prev_types, nullptr, n_frames, run, fg_step == bg_step ? 1u : 0u};
  t.tally = ws.tally;
  launch_delta_count(block, period, dim3(div_up(a.total_waves, 4)), s, a, t);
  if ((rc = check_launch(what, "count"))) return rc;
  const DeltaSelectArgs sel{ws.tally, d_forced, d_key_out, d_level_counts, g.l.tiles_y * g.waves_per_row, run, d_prev_bgr ? 1u : 0u};
  hipLaunchKernelGGL(dct_delta_select_kernel, dim3(n_frames), dim3(kThreads), 0, s, sel);
  if ((rc = check_launch(what, "select"))) return rc;
  const DeltaRunArgs k{d_prev_bgr, d_prev_types, d_key_out, n_frames, run, fg_step == bg_step ? 1u : 0u};
  return enqueue_dct_pack_delta(what, a, k, fg_step, bg_step, d_out, d_frame_offsets, s, period);
}

int svc_hip_dct_pack_delta_auto_frames(const uint8_t* d_bgr, uint64_t frame_stride_bytes, uint32_t n_frames, uint32_t frame_w,
                                       uint32_t frame_h, uint32_t block, const uint32_t* d_block_types, uint32_t mv_block_w,
                                       uint32_t mv_block_h, uint32_t fg_step, uint32_t bg_step, const uint8_t* d_prev_bgr,
                                       const uint32_t* d_prev_types, const uint32_t* d_forced, uint8_t* d_workspace, uint64_t workspace_bytes,
                                       uint8_t* d_out, uint64_t out_capacity, uint64_t* d_frame_offsets, uint32_t* d_key_out,
                                       uint32_t* d_level_counts, void* stream) {
  return dct_pack_delta_auto("dct_pack_delta_auto", 1, d_bgr, frame_stride_bytes, n_frames, frame_w, frame_h, block, d_block_types, mv_block_w,
                             mv_block_h, fg_step, bg_step, d_prev_bgr, d_prev_types, d_forced, d_workspace, workspace_bytes, d_out,
                             out_capacity, d_frame_offsets, d_key_out, d_level_counts, stream);
}

// ---- temporal layers: the two calls above with a period (include/svc_hip_temporal.h; the workspaces are their siblings')

uint64_t svc_hip_dct_pack_delta_temporal_workspace_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h, uint32_t block,
                                                         uint32_t mv_block_w, uint32_t mv_block_h, uint32_t period) {
  if (validate_pack_geom("dct_pack_delta_temporal_workspace_bytes", frame_w, frame_h, block, mv_block_w, mv_block_h) ||
      validate_pack_period("dct_pack_delta_temporal_workspace_bytes", period))
    return 0;
  return svc_hip_dct_pack_delta_workspace_bytes(n_frames, frame_w, frame_h, block, mv_block_w, mv_block_h);
}

int svc_hip_dct_pack_delta_temporal_frames(const uint8_t* d_bgr, uint64_t frame_stride_bytes, uint32_t n_frames, uint32_t frame_w,
                                           uint32_t frame_h, uint32_t block, const uint32_t* d_block_types, uint32_t mv_block_w,
                                           uint32_t mv_block_h, uint32_t fg_step, uint32_t bg_step, const uint8_t* d_prev_bgr,
                                           const uint32_t* d_prev_types, const uint32_t* d_key, uint8_t* d_workspace, uint64_t workspace_bytes,
                                           uint8_t* d_out, uint64_t out_capacity, uint64_t* d_frame_offsets, void* stream, uint32_t period) {
  return dct_pack_delta("dct_pack_delta_temporal", period, d_bgr, frame_stride_bytes, n_frames, frame_w, frame_h, block, d_block_types,
                        mv_block_w, mv_block_h, fg_step, bg_step, d_prev_bgr, d_prev_types, d_key, d_workspace, workspace_bytes, d_out,
                        out_capacity, d_frame_offsets, stream);
}

uint64_t svc_hip_dct_pack_delta_temporal_auto_workspace_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h, uint32_t block,
                                                              uint32_t mv_block_w, uint32_t mv_block_h, uint32_t period) {
  if (validate_pack_geom("dct_pack_delta_temporal_auto_workspace_bytes", frame_w, frame_h, block, mv_block_w, mv_block_h) ||
      validate_pack_period("dct_pack_delta_temporal_auto_workspace_bytes", period))
    return 0;
  return svc_hip_dct_pack_delta_auto_workspace_bytes(n_frames, frame_w, frame_h, block, mv_block_w, mv_block_h);
}

int svc_hip_dct_pack_delta_temporal_auto_frames(const uint8_t* d_bgr, uint64_t frame_stride_bytes, uint32_t n_frames, uint32_t frame_w,
                                                uint32_t frame_h, uint32_t block, const uint32_t* d_block_types, uint32_t mv_block_w,
                                                uint32_t mv_block_h, uint32_t fg_step, uint32_t bg_step, const uint8_t* d_prev_bgr,
                                                const uint32_t* d_prev_types, const uint32_t* d_forced, uint8_t* d_workspace,
                                                uint64_t workspace_bytes, uint8_t* d_out, uint64_t out_capacity, uint64_t* d_frame_offsets,
                                                uint32_t* d_key_out, uint32_t* d_level_counts, void* stream, uint32_t period) {
  return dct_pack_delta_auto("dct_pack_delta_temporal_auto", period, d_bgr, frame_stride_bytes, n_frames, frame_w, frame_h, block,
                             d_block_types, mv_block_w, mv_block_h, fg_step, bg_step, d_prev_bgr, d_prev_types, d_forced, d_workspace,
                             workspace_bytes, d_out, out_capacity, d_frame_offsets, d_key_out, d_level_counts, stream);
}

uint64_t svc_hip_dct_pack_layers_workspace_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h, uint32_t block, uint32_t mv_block_w,
                                                 uint32_t mv_block_h) {
  if (validate_pack_geom("dct_pack_layers_workspace_bytes", frame_w, frame_h, block, mv_block_w, mv_block_h)) return 0;
  const PackGeom g = make_pack_geom(frame_w, frame_h, block, mv_block_w, mv_block_h);
  if (validate_pack_limits("dct_pack_layers_workspace_bytes", n_frames, g)) return 0;
  return 2 * layout_bytes(pack_ws, n_frames, g);  // a layer's workspace is a multiple of 16 B: the second starts aligned
}

// Checked in the order of svc_hip_dct_pack_levels_frames: geometry, stride, steps, the int16 bounds, limits, workspace, both capacities;
// n_frames == 0 then returns SVC_OK; then pointers.
int svc_hip_dct_pack_layers_frames(const uint8_t* d_bgr, uint64_t frame_stride_bytes, uint32_t n_frames, uint32_t frame_w, uint32_t frame_h,
                                   uint32_t block, const uint32_t* d_block_types, uint32_t mv_block_w, uint32_t mv_block_h, uint32_t fg_step,
                                   uint32_t bg_step, uint32_t enh_step, const uint32_t* d_window, uint8_t* d_workspace,
                                   uint64_t workspace_bytes, uint8_t* d_base_out, uint64_t base_capacity, uint64_t* d_base_offsets,
                                   uint8_t* d_enh_out, uint64_t enh_capacity, uint64_t* d_enh_offsets, void* stream) {
  int rc = validate_pack_geom("dct_pack_layers", frame_w, frame_h, block, mv_block_w, mv_block_h);
  if (rc) return rc;
  SVC_REQUIRE(frame_stride_bytes >= 3ull * frame_w * frame_h && frame_stride_bytes % 16 == 0,
              "dct_pack_layers: a frame stride of %llu B (at least the frame's %llu B, a multiple of 16)", (unsigned long long)frame_stride_bytes,
              3ull * frame_w * frame_h);
  SVC_REQUIRE(fg_step > 0 && bg_step > 0 && enh_step > 0, "dct_pack_layers: quant steps must be positive");
  // (a step that divides is not above: this also refuses enh_step > min(fg_step, bg_step))
  SVC_REQUIRE(fg_step % enh_step == 0 && bg_step % enh_step == 0, "dct_pack_layers: fg_step %u and bg_step %u must each be a multiple of enh_step %u",
              fg_step, bg_step, enh_step);
  // the pack's int16 bound (Parseval) on the fine levels; the residuals are within ratio / 2 + 1 of zero
  if (255.0 * block / enh_step > 32767.0)
    return fail(SVC_ERR_UNSUPPORTED, "dct_pack_layers: levels of a %ux%u tile at step %u could exceed int16", block, block, enh_step);
  if (std::max(fg_step, bg_step) / enh_step > 32766)
    return fail(SVC_ERR_UNSUPPORTED, "dct_pack_layers: a base step of %u is more than 32766 times enh_step %u: a residual could exceed int16",
                std::max(fg_step, bg_step), enh_step);
  const PackGeom g = make_pack_geom(frame_w, frame_h, block, mv_block_w, mv_block_h);
  if ((rc = validate_pack_limits("dct_pack_layers", n_frames, g))) return rc;
  const uint64_t ws_layer = layout_bytes(pack_ws, n_frames, g);
  if ((rc = require_workspace("dct_pack_layers", workspace_bytes, 2 * ws_layer))) return rc;
  if ((rc = require_capacity("dct_pack_layers", "base output", base_capacity, n_frames * g.l.max_bytes))) return rc;
  if ((rc = require_capacity("dct_pack_layers", "enhancement output", enh_capacity, n_frames * g.l.max_bytes))) return rc;
  if (n_frames == 0) return SVC_OK;  // empty batch: nothing to enqueue
  SVC_REQUIRE(d_bgr && d_block_types && d_workspace && d_base_out && d_base_offsets && d_enh_out && d_enh_offsets, "dct_pack_layers: null pointer");
  SVC_REQUIRE(aligned(d_bgr, 16) && aligned(d_base_out, 16) && aligned(d_enh_out, 16) && aligned(d_workspace, 16) && aligned(d_base_offsets, 8) &&
                  aligned(d_enh_offsets, 8) && aligned(d_block_types, 4) && aligned(d_window, 4),
              "dct_pack_layers: frames, outputs and workspace must be 16-byte aligned, offsets 8-byte, types and window 4-byte");
  hipStream_t s = static_cast<hipStream_t>(stream);
  DctPackArgs a{};
  a.bgr = d_bgr;
  a.frame_stride = frame_stride_bytes;
  a.g = g;
  a.total_waves = n_frames * g.l.tiles_y * g.waves_per_row;
  a.types = d_block_types;
  a.fg_step = (float)fg_step;
  a.bg_step = (float)bg_step;
  a.fg_inv = 1.0f / a.fg_step;
  a.bg_inv = 1.0f / a.bg_step;
  a.ws = carve(d_workspace, pack_ws, n_frames, g);
  LayerArgs k{};
  k.enh_step = (float)enh_step;
  k.enh_inv = 1.0f / k.enh_step;
  k.fg_ratio = fg_step / enh_step;
  k.bg_ratio = bg_step / enh_step;
  k.window = d_window;
  k.enh = carve(d_workspace + ws_layer, pack_ws, n_frames, g);
  const dim3 grid(div_up(a.total_waves, 4)), blk(kThreads);
  if (block == 8) hipLaunchKernelGGL(dct_pack_layers_kernel<8>, grid, blk, 0, s, a, k);
  else hipLaunchKernelGGL(dct_pack_layers_kernel<16>, grid, blk, 0, s, a, k);
  if ((rc = check_launch("dct_pack_layers", "transform"))) return rc;
  if ((rc = enqueue_assemble("dct_pack_layers base", a, a.ws, n_frames, fg_step, bg_step, d_base_out, d_base_offsets, s))) return rc;
  return enqueue_assemble("dct_pack_layers enhancement", a, k.enh, n_frames, enh_step, enh_step, d_enh_out, d_enh_offsets, s);
}

uint64_t svc_hip_dct_pack_levels_budget_workspace_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h, uint32_t block,
                                                        uint32_t mv_block_w, uint32_t mv_block_h, uint32_t ladder_len) {
  const char* what = "dct_pack_levels_budget_workspace_bytes";
  if (validate_pack_geom(what, frame_w, frame_h, block, mv_block_w, mv_block_h)) return 0;
  if (ladder_len == 0 || ladder_len > kMaxLadder) {
    (void)fail(SVC_ERR_INVALID_ARG, "%s: a ladder of %u entries (1 .. %u)", what, ladder_len, kMaxLadder);
    return 0;
  }
  const PackGeom g = make_pack_geom(frame_w, frame_h, block, mv_block_w, mv_block_h);
  if (validate_pack_limits(what, n_frames, g)) return 0;
  return layout_bytes(budget_ws, n_frames, g);
}

// Checked in the order of svc_hip_dct_pack_levels_frames, the ladder in place of the steps: geometry, stride, ladder, limits, sizes;
// n_frames == 0 then returns SVC_OK; then pointers.
int svc_hip_dct_pack_levels_budget_frames(const uint8_t* d_bgr, uint64_t frame_stride_bytes, uint32_t n_frames, uint32_t frame_w,
                                          uint32_t frame_h, uint32_t block, const uint32_t* d_block_types, uint32_t mv_block_w,
                                          uint32_t mv_block_h, const svc_step_pair* ladder, uint32_t ladder_len, const uint32_t* d_budget,
                                          uint8_t* d_workspace, uint64_t workspace_bytes, uint8_t* d_out, uint64_t out_capacity,
                                          uint64_t* d_frame_offsets, uint32_t* d_choice, void* stream) {
  int rc = validate_pack_geom("dct_pack_levels_budget", frame_w, frame_h, block, mv_block_w, mv_block_h);
  if (rc) return rc;
  SVC_REQUIRE(frame_stride_bytes >= 3ull * frame_w * frame_h && frame_stride_bytes % 16 == 0,
              "dct_pack_levels_budget: a frame stride of %llu B (at least the frame's %llu B, a multiple of 16)",
              (unsigned long long)frame_stride_bytes, 3ull * frame_w * frame_h);
  if ((rc = validate_ladder("dct_pack_levels_budget", ladder, ladder_len))) return rc;
  // (the pack's int16 bound holds for every step at 8x8 and 16x16, as in svc_hip_dct_pack_levels_frames)
  const PackGeom g = make_pack_geom(frame_w, frame_h, block, mv_block_w, mv_block_h);
  if ((rc = validate_pack_limits("dct_pack_levels_budget", n_frames, g))) return rc;
  if ((rc = require_workspace("dct_pack_levels_budget", workspace_bytes, layout_bytes(budget_ws, n_frames, g)))) return rc;
  if ((rc = require_capacity("dct_pack_levels_budget", "output", out_capacity, n_frames * g.l.max_bytes))) return rc;
  if (n_frames == 0) return SVC_OK;  // empty batch: nothing to enqueue
  SVC_REQUIRE(d_bgr && d_block_types && d_budget && d_workspace && d_out && d_frame_offsets && d_choice,
              "dct_pack_levels_budget: null pointer");
  SVC_REQUIRE(aligned(d_bgr, 16) && aligned(d_out, 16) && aligned(d_workspace, 16) && aligned(d_frame_offsets, 8) &&
                  aligned(d_block_types, 4) && aligned(d_budget, 4) && aligned(d_choice, 4),
              "dct_pack_levels_budget: frames, output and workspace must be 16-byte aligned, offsets 8-byte, types, budget and choice 4-byte");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const BudgetWs bws = carve(d_workspace, budget_ws, n_frames, g);
  DctPackArgs a{};
  a.bgr = d_bgr;
  a.frame_stride = frame_stride_bytes;
  a.g = g;
  a.total_waves = n_frames * g.l.tiles_y * g.waves_per_row;
  a.types = d_block_types;
  a.steps = bws.steps;
  a.ws = bws.pack;
  CountArgs k{make_ladder(ladder, ladder_len), 0, bws.rows};
  while ((ladder_len >> k.probes) != 0) ++k.probes;
  LadderInv li{};
  for (uint32_t i = 0; i < ladder_len; ++i) {
    li.inv[0][i] = 1.0f / (float)ladder[i].bg_step;
    li.inv[1][i] = 1.0f / (float)ladder[i].fg_step;
  }
  const dim3 grid(div_up(a.total_waves, 4)), blk(kThreads);
  if (block == 8) hipLaunchKernelGGL(dct_count_kernel<8>, grid, blk, 0, s, a, k);
  else hipLaunchKernelGGL(dct_count_kernel<16>, grid, blk, 0, s, a, k);
  if ((rc = check_launch("dct_pack_levels_budget", "count"))) return rc;
  hipLaunchKernelGGL(dct_count_sum_kernel, dim3(kSumParts, n_frames), blk, 0, s, g.l.tiles_y * g.waves_per_row, bws.rows, bws.parts);
  if ((rc = check_launch("dct_pack_levels_budget", "sum"))) return rc;
  const SelectArgs sel{g.l.levels_off, bws.parts, d_budget, bws.steps, d_choice};
  hipLaunchKernelGGL(dct_pack_select_kernel, dim3(n_frames), blk, 0, s, k.lad, li, sel);
  if ((rc = check_launch("dct_pack_levels_budget", "select"))) return rc;
  return enqueue_dct_pack("dct_pack_levels_budget", a, n_frames, 0, 0, d_out, d_frame_offsets, s);
}

// ---- a quality target in place of the byte budget, or beside it (include/svc_hip_quality.h)

uint64_t svc_hip_dct_pack_levels_quality_workspace_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h, uint32_t block,
                                                         uint32_t mv_block_w, uint32_t mv_block_h, uint32_t ladder_len) {
  const char* what = "dct_pack_levels_quality_workspace_bytes";
  if (validate_pack_geom(what, frame_w, frame_h, block, mv_block_w, mv_block_h)) return 0;
  if (ladder_len == 0 || ladder_len > kMaxLadder) {
    (void)fail(SVC_ERR_INVALID_ARG, "%s: a ladder of %u entries (1 .. %u)", what, ladder_len, kMaxLadder);
    return 0;
  }
  const PackGeom g = make_pack_geom(frame_w, frame_h, block, mv_block_w, mv_block_h);
  if (validate_pack_limits(what, n_frames, g)) return 0;
  return layout_bytes(quality_ws, n_frames, g);
}

// Checked in the order of svc_hip_dct_pack_levels_budget_frames: geometry, stride, ladder, limits (which bound a frame's coefficients
// below 2^31: the u64 sums cannot overflow), sizes; n_frames == 0 then returns SVC_OK; then pointers.  Six launches whatever n_frames.
int svc_hip_dct_pack_levels_quality_frames(const uint8_t* d_bgr, uint64_t frame_stride_bytes, uint32_t n_frames, uint32_t frame_w,
                                           uint32_t frame_h, uint32_t block, const uint32_t* d_block_types, uint32_t mv_block_w,
                                           uint32_t mv_block_h, const svc_step_pair* ladder, uint32_t ladder_len, const uint64_t* d_target,
                                           const uint32_t* d_budget, uint8_t* d_workspace, uint64_t workspace_bytes, uint8_t* d_out,
                                           uint64_t out_capacity, uint64_t* d_frame_offsets, uint32_t* d_choice, uint64_t* d_distortion,
                                           void* stream) {
  const char* what = "dct_pack_levels_quality";
  int rc = validate_pack_geom(what, frame_w, frame_h, block, mv_block_w, mv_block_h);
  if (rc) return rc;
  SVC_REQUIRE(frame_stride_bytes >= 3ull * frame_w * frame_h && frame_stride_bytes % 16 == 0,
              "%s: a frame stride of %llu B (at least the frame's %llu B, a multiple of 16)", what, (unsigned long long)frame_stride_bytes,
              3ull * frame_w * frame_h);
  if ((rc = validate_ladder(what, ladder, ladder_len))) return rc;
  const PackGeom g = make_pack_geom(frame_w, frame_h, block, mv_block_w, mv_block_h);
  if ((rc = validate_pack_limits(what, n_frames, g))) return rc;
  if ((rc = require_workspace(what, workspace_bytes, layout_bytes(quality_ws, n_frames, g)))) return rc;
  if ((rc = require_capacity(what, "output", out_capacity, n_frames * g.l.max_bytes))) return rc;
  if (n_frames == 0) return SVC_OK;  // empty batch: nothing to enqueue
  SVC_REQUIRE(d_bgr && d_block_types && d_target && d_workspace && d_out && d_frame_offsets && d_choice, "%s: null pointer", what);
  SVC_REQUIRE(aligned(d_bgr, 16) && aligned(d_out, 16) && aligned(d_workspace, 16) && aligned(d_frame_offsets, 8) && aligned(d_target, 8) &&
                  aligned(d_distortion, 8) && aligned(d_block_types, 4) && aligned(d_budget, 4) && aligned(d_choice, 4),
              "%s: frames, output and workspace must be 16-byte aligned, offsets, target and distortion 8-byte, types, budget and choice 4-byte",
              what);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const QualityWs qws = carve(d_workspace, quality_ws, n_frames, g);
  DctPackArgs a{};
  a.bgr = d_bgr;
  a.frame_stride = frame_stride_bytes;
  a.g = g;
  a.total_waves = n_frames * g.l.tiles_y * g.waves_per_row;
  a.types = d_block_types;
  a.steps = qws.budget.steps;
  a.ws = qws.budget.pack;
  MeasureArgs k{};
  k.lad = make_ladder(ladder, ladder_len);
  while ((ladder_len >> k.probes) != 0) ++k.probes;
  k.rows = qws.budget.rows;
  for (uint32_t i = 0; i < ladder_len; ++i) {
    k.li.inv[0][i] = 1.0f / (float)ladder[i].bg_step;
    k.li.inv[1][i] = 1.0f / (float)ladder[i].fg_step;
  }
  k.drows = qws.drows;
  const dim3 grid(div_up(a.total_waves, 4)), blk(kThreads);
  if (block == 8) hipLaunchKernelGGL(dct_measure_kernel<8>, grid, blk, 0, s, a, k);
  else hipLaunchKernelGGL(dct_measure_kernel<16>, grid, blk, 0, s, a, k);
  if ((rc = check_launch(what, "measure"))) return rc;
  hipLaunchKernelGGL(dct_measure_sum_kernel, dim3(kSumParts, n_frames), blk, 0, s, g.l.tiles_y * g.waves_per_row, qws.budget.rows,
                     qws.budget.parts, qws.drows, qws.dparts);
  if ((rc = check_launch(what, "sum"))) return rc;
  const QualitySelectArgs sel{g.l.levels_off, qws.budget.parts, qws.dparts, d_target, d_budget, qws.budget.steps, d_choice, d_distortion};
  hipLaunchKernelGGL(dct_quality_select_kernel, dim3(n_frames), blk, 0, s, k.lad, k.li, sel);
  if ((rc = check_launch(what, "select"))) return rc;
  return enqueue_dct_pack(what, a, n_frames, 0, 0, d_out, d_frame_offsets, s);
}

// ---- the delta stream with one pair of steps per group of frames, by a byte budget on the group (include/svc_hip_delta_budget.h)

uint64_t svc_hip_dct_pack_delta_budget_workspace_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h, uint32_t block,
                                                       uint32_t mv_block_w, uint32_t mv_block_h, uint32_t ladder_len) {
  const char* what = "dct_pack_delta_budget_workspace_bytes";
  if (validate_pack_geom(what, frame_w, frame_h, block, mv_block_w, mv_block_h)) return 0;
  if (ladder_len == 0 || ladder_len > kMaxLadder) {
    (void)fail(SVC_ERR_INVALID_ARG, "%s: a ladder of %u entries (1 .. %u)", what, ladder_len, kMaxLadder);
    return 0;
  }
  const PackGeom g = make_pack_geom(frame_w, frame_h, block, mv_block_w, mv_block_h);
  if (validate_pack_limits(what, n_frames, g)) return 0;
  return layout_bytes(delta_budget_ws, n_frames, g);
}

// Checked in the order of svc_hip_dct_pack_levels_budget_frames: geometry, stride, ladder, limits, sizes; n_frames == 0 then returns
// SVC_OK; then pointers.  Six launches whatever n_frames: the ladder tally, its sum, the groups' selection, then the delta form's three
// with each frame's own steps.
int svc_hip_dct_pack_delta_budget_frames(const uint8_t* d_bgr, uint64_t frame_stride_bytes, uint32_t n_frames, uint32_t frame_w,
                                         uint32_t frame_h, uint32_t block, const uint32_t* d_block_types, uint32_t mv_block_w,
                                         uint32_t mv_block_h, const svc_step_pair* ladder, uint32_t ladder_len, const uint32_t* d_key,
                                         const uint32_t* d_budget, uint8_t* d_workspace, uint64_t workspace_bytes, uint8_t* d_out,
                                         uint64_t out_capacity, uint64_t* d_frame_offsets, uint32_t* d_choice, uint32_t* d_level_counts,
                                         void* stream) {
  const char* what = "dct_pack_delta_budget";
  int rc = validate_pack_geom(what, frame_w, frame_h, block, mv_block_w, mv_block_h);
  if (rc) return rc;
  SVC_REQUIRE(frame_stride_bytes >= 3ull * frame_w * frame_h && frame_stride_bytes % 16 == 0,
              "%s: a frame stride of %llu B (at least the frame's %llu B, a multiple of 16)", what, (unsigned long long)frame_stride_bytes,
              3ull * frame_w * frame_h);
  if ((rc = validate_ladder(what, ladder, ladder_len))) return rc;
  // (the pack's int16 bound holds for every step at 8x8 and 16x16, as in svc_hip_dct_pack_levels_frames; a difference wraps by definition)
  const PackGeom g = make_pack_geom(frame_w, frame_h, block, mv_block_w, mv_block_h);
  if ((rc = validate_pack_limits(what, n_frames, g))) return rc;
  if ((rc = require_workspace(what, workspace_bytes, layout_bytes(delta_budget_ws, n_frames, g)))) return rc;
  if ((rc = require_capacity(what, "output", out_capacity, n_frames * g.l.max_bytes))) return rc;
  if (n_frames == 0) return SVC_OK;  // empty batch: nothing to enqueue
  SVC_REQUIRE(d_bgr && d_block_types && d_budget && d_workspace && d_out && d_frame_offsets && d_choice, "%s: null pointer", what);
  SVC_REQUIRE(aligned(d_bgr, 16) && aligned(d_out, 16) && aligned(d_workspace, 16) && aligned(d_frame_offsets, 8) && aligned(d_block_types, 4) &&
                  aligned(d_key, 4) && aligned(d_budget, 4) && aligned(d_choice, 4) && aligned(d_level_counts, 4),
              "%s: frames, output and workspace must be 16-byte aligned, offsets 8-byte, types, key flags, budget, choice and level counts 4-byte",
              what);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const DeltaBudgetWs ws = carve(d_workspace, delta_budget_ws, n_frames, g);
  DctPackArgs a{};
  a.bgr = d_bgr;
  a.frame_stride = frame_stride_bytes;
  a.g = g;
  a.types = d_block_types;
  a.ws = ws.pack;
  a.total_waves = div_up(n_frames, kDeltaRun) * g.l.tiles_y * g.waves_per_row;  // a wave per piece and RUN, as the pack below
  const DeltaRunArgs run{nullptr, nullptr, d_key, n_frames, kDeltaRun, 0u};  // (one_step is each frame's own, from its steps)
  DeltaLadderArgs t{};
  static_cast<DeltaRunArgs&>(t) = run;
  t.lad = make_ladder(ladder, ladder_len);
  for (uint32_t i = 0; i < ladder_len; ++i) {
    t.li.inv[0][i] = 1.0f / (float)ladder[i].bg_step;
    t.li.inv[1][i] = 1.0f / (float)ladder[i].fg_step;
  }
  t.rows = ws.rows;
  const dim3 grid(div_up(a.total_waves, 4)), blk(kThreads);
  if (block == 8) hipLaunchKernelGGL(dct_delta_ladder_kernel<8>, grid, blk, 0, s, a, t);
  else hipLaunchKernelGGL(dct_delta_ladder_kernel<16>, grid, blk, 0, s, a, t);
  if ((rc = check_launch(what, "tally"))) return rc;
  hipLaunchKernelGGL(dct_delta_ladder_sum_kernel, dim3(kSumParts, n_frames), blk, 0, s, g.l.tiles_y * g.waves_per_row, kDeltaRun, ws.rows, ws.parts);
  if ((rc = check_launch(what, "sum"))) return rc;
  const GroupSelectArgs sel{g.l.levels_off, ws.parts, d_key, d_budget, ws.steps, d_choice, d_level_counts, n_frames};
  hipLaunchKernelGGL(dct_delta_group_select_kernel, dim3(n_frames), blk, 0, s, t.lad, t.li, sel);
  if ((rc = check_launch(what, "select"))) return rc;
  a.steps = ws.steps;
  if (block == 8) hipLaunchKernelGGL(dct_pack_delta_group_kernel<8>, grid, blk, 0, s, a, run);
  else hipLaunchKernelGGL(dct_pack_delta_group_kernel<16>, grid, blk, 0, s, a, run);
  if ((rc = check_launch(what, "transform"))) return rc;
  return enqueue_assemble(what, a, a.ws, n_frames, 0, 0, d_out, d_frame_offsets, s);
}

// ---- the same with a distortion target per group, and the byte budget as an optional cap (include/svc_hip_delta_quality.h)

uint64_t svc_hip_dct_pack_delta_quality_workspace_bytes(uint32_t n_frames, uint32_t frame_w, uint32_t frame_h, uint32_t block,
                                                        uint32_t mv_block_w, uint32_t mv_block_h, uint32_t ladder_len) {
  const char* what = "dct_pack_delta_quality_workspace_bytes";
  if (validate_pack_geom(what, frame_w, frame_h, block, mv_block_w, mv_block_h)) return 0;
  if (ladder_len == 0 || ladder_len > kMaxLadder) {
    (void)fail(SVC_ERR_INVALID_ARG, "%s: a ladder of %u entries (1 .. %u)", what, ladder_len, kMaxLadder);
    return 0;
  }
  const PackGeom g = make_pack_geom(frame_w, frame_h, block, mv_block_w, mv_block_h);
  if (validate_pack_limits(what, n_frames, g)) return 0;
  return layout_bytes(delta_quality_ws, n_frames, g);
}

// Checked in the order of svc_hip_dct_pack_delta_budget_frames: geometry, stride, ladder, limits (which bound a frame's coefficients below
// 2^31: the u64 sums cannot overflow), sizes; n_frames == 0 then returns SVC_OK; then pointers.  Six launches whatever n_frames: the
// measuring tally, its sum, the groups' selection, then the delta form's three with each frame's own steps.
int svc_hip_dct_pack_delta_quality_frames(const uint8_t* d_bgr, uint64_t frame_stride_bytes, uint32_t n_frames, uint32_t frame_w,
                                          uint32_t frame_h, uint32_t block, const uint32_t* d_block_types, uint32_t mv_block_w,
                                          uint32_t mv_block_h, const svc_step_pair* ladder, uint32_t ladder_len, const uint32_t* d_key,
                                          const uint64_t* d_target, const uint32_t* d_budget, uint8_t* d_workspace, uint64_t workspace_bytes,
                                          uint8_t* d_out, uint64_t out_capacity, uint64_t* d_frame_offsets, uint32_t* d_choice,
                                          uint32_t* d_level_counts, uint64_t* d_distortion, void* stream) {
  const char* what = "dct_pack_delta_quality";
  int rc = validate_pack_geom(what, frame_w, frame_h, block, mv_block_w, mv_block_h);
  if (rc) return rc;
  SVC_REQUIRE(frame_stride_bytes >= 3ull * frame_w * frame_h && frame_stride_bytes % 16 == 0,
              "%s: a frame stride of %llu B (at least the frame's %llu B, a multiple of 16)", what, (unsigned long long)frame_stride_bytes,
              3ull * frame_w * frame_h);
  if ((rc = validate_ladder(what, ladder, ladder_len))) return rc;
  const PackGeom g = make_pack_geom(frame_w, frame_h, block, mv_block_w, mv_block_h);
  if ((rc = validate_pack_limits(what, n_frames, g))) return rc;
  if ((rc = require_workspace(what, workspace_bytes, layout_bytes(delta_quality_ws, n_frames, g)))) return rc;
  if ((rc = require_capacity(what, "output", out_capacity, n_frames * g.l.max_bytes))) return rc;
  if (n_frames == 0) return SVC_OK;  // empty batch: nothing to enqueue
  SVC_REQUIRE(d_bgr && d_block_types && d_target && d_workspace && d_out && d_frame_offsets && d_choice, "%s: null pointer", what);
  SVC_REQUIRE(aligned(d_bgr, 16) && aligned(d_out, 16) && aligned(d_workspace, 16) && aligned(d_frame_offsets, 8) && aligned(d_target, 8) &&
                  aligned(d_distortion, 8) && aligned(d_block_types, 4) && aligned(d_key, 4) && aligned(d_budget, 4) && aligned(d_choice, 4) &&
                  aligned(d_level_counts, 4),
              "%s: frames, output and workspace must be 16-byte aligned, offsets, target and distortion 8-byte, types, key flags, budget, "
              "choice and level counts 4-byte", what);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const DeltaQualityWs ws = carve(d_workspace, delta_quality_ws, n_frames, g);
  const uint32_t waves_per_frame = g.l.tiles_y * g.waves_per_row;
  DctPackArgs a{};
  a.bgr = d_bgr;
  a.frame_stride = frame_stride_bytes;
  a.g = g;
  a.types = d_block_types;
  a.ws = ws.budget.pack;
  a.total_waves = div_up(n_frames, kDeltaRun) * waves_per_frame;  // a wave per piece and RUN, as the pack below
  const DeltaRunArgs run{nullptr, nullptr, d_key, n_frames, kDeltaRun, 0u};  // (one_step is each frame's own, from its steps)
  DeltaMeasureArgs t{};
  static_cast<DeltaRunArgs&>(t) = run;
  t.lad = make_ladder(ladder, ladder_len);
  for (uint32_t i = 0; i < ladder_len; ++i) {
    t.li.inv[0][i] = 1.0f / (float)ladder[i].bg_step;
    t.li.inv[1][i] = 1.0f / (float)ladder[i].fg_step;
  }
  t.rows = ws.budget.rows;
  t.drows = ws.drows;
  const dim3 grid(div_up(a.total_waves, 4)), blk(kThreads);
  if constexpr (kDeltaQualityTwoPass) {  // the measuring form for D, a frame per wave, then the ladder tally for the counts
    DctPackArgs m = a;
    m.total_waves = n_frames * waves_per_frame;
    MeasureArgs k{};
    k.lad = t.lad;
    while ((ladder_len >> k.probes) != 0) ++k.probes;
    k.rows = ws.crows;
    k.li = t.li;
    k.drows = ws.drows;
    const dim3 mgrid(div_up(m.total_waves, 4));
    if (block == 8) hipLaunchKernelGGL(dct_measure_kernel<8>, mgrid, blk, 0, s, m, k);
    else hipLaunchKernelGGL(dct_measure_kernel<16>, mgrid, blk, 0, s, m, k);
    if ((rc = check_launch(what, "measure"))) return rc;
    if (block == 8) hipLaunchKernelGGL(dct_delta_ladder_kernel<8>, grid, blk, 0, s, a, static_cast<const DeltaLadderArgs&>(t));
    else hipLaunchKernelGGL(dct_delta_ladder_kernel<16>, grid, blk, 0, s, a, static_cast<const DeltaLadderArgs&>(t));
  } else {
    if (block == 8) hipLaunchKernelGGL(dct_delta_measure_kernel<8>, grid, blk, 0, s, a, t);
    else hipLaunchKernelGGL(dct_delta_measure_kernel<16>, grid, blk, 0, s, a, t);
  }
  if ((rc = check_launch(what, "tally"))) return rc;
  hipLaunchKernelGGL(dct_delta_measure_sum_kernel, dim3(kSumParts, n_frames), blk, 0, s, waves_per_frame, kDeltaRun, ws.budget.rows, ws.budget.parts,
                     kDeltaQualityTwoPass ? 1u : kDeltaRun, ws.drows, ws.dparts);
  if ((rc = check_launch(what, "sum"))) return rc;
  const GroupQualitySelectArgs sel{g.l.levels_off, ws.budget.parts, ws.dparts, d_key, d_target, d_budget, ws.budget.steps, d_choice,
                                   d_level_counts, d_distortion, n_frames};
  hipLaunchKernelGGL(dct_delta_quality_select_kernel, dim3(n_frames), blk, 0, s, t.lad, t.li, sel);
  if ((rc = check_launch(what, "select"))) return rc;
  a.steps = ws.budget.steps;
  if (block == 8) hipLaunchKernelGGL(dct_pack_delta_group_kernel<8>, grid, blk, 0, s, a, run);
  else hipLaunchKernelGGL(dct_pack_delta_group_kernel<16>, grid, blk, 0, s, a, run);
  if ((rc = check_launch(what, "transform"))) return rc;
  return enqueue_assemble(what, a, a.ws, n_frames, 0, 0, d_out, d_frame_offsets, s);
}

}  // extern "C"
