// stream_encoder.hpp -- the hot path for a clip that lives in HOST memory, batched and overlapped
// with PCIe: the C++ entry point a host application uses instead of calling the reference's
// one-frame-per-call functions (include/svc/motion.hpp) in a loop.
//
// What it runs per encoded frame is the middle of Encoder::operator() (reference
// libs/encoder.cpp:449-650): pad, luma + pyramid, EstimateMotionHierarchical,
// EstimateGlobalMotionRansac, the segmentation glue -> region ids, Dct (+ the decoder's quant
// lines), optionally SerializeEncodedFrame -- every stage through the C ABI of include/svc_hip.h.
// Frames go pinned -> device on a copy stream while the previous batch is in the kernels and the
// one before is on its way back; the one-frame overlap between batches is copied on the device.
//
// RANSAC's draws (the reference seeds std::random_device, libs/motion.cpp:186-187) and the k-means
// seeds are a deterministic function of `seed` and the frame index, so a clip encodes to the same
// result whatever the batch size.
#ifndef SVC_STREAM_ENCODER_HPP
#define SVC_STREAM_ENCODER_HPP

#include <cstdint>
#include <functional>
#include <memory>
#include <vector>

#include "svc_hip.h"

namespace svc {

struct StreamEncoderConfig {
  uint32_t width = 0, height = 0;  // source frame size; padded as libs/encoder.cpp:164-168 does
  uint32_t levels = 3;             // pyr-lvl-count
  uint32_t mv_block = 16;          // MV block width (and height, unless mv_block_h is set); apps/encoder.cpp:28-58 defaults from here on
  uint32_t search_range = 8;
  uint32_t dct_block = 8;          // transform block width (and height, unless dct_block_h is set): anything the C ABI's Dct takes
  uint32_t mv_block_h = 0;         // non-square blocks (--mv-block-h / --transform-block-h differing from the widths): 0 = square.
  uint32_t dct_block_h = 0;        // Non-square transform blocks with `wire` take the planes + serialiser route (the fused record kernel is square)
  uint32_t fg_step = 1, bg_step = 640;  // apps/decoder.cpp:22-23
  bool wire = false;               // serialised records (libs/encoder.cpp:222-269) instead of planes: RAW
                                   // coefficients, as the reference's encoder emits them (the decoder picks the
                                   // quant step per tile, libs/decoder.cpp:130-135), over the PADDED tile grid its
                                   // decoder parses (libs/decoder.cpp:185-186); fg_step / bg_step apply to planes only
  bool reference_stream = false;   // with `wire`: the records EXACTLY as the reference's ENCODER serialises them
                                   // (libs/encoder.cpp:647-650 hands SerializeEncodedFrame the UNPADDED size: tile loops over it,
                                   // and the unpadded width as the row stride of the padded planes) -- the stream
                                   // apps/encoder.cpp writes to stdout; record_bytes then counts the unpadded tile grid
  uint32_t batch = 16;             // encoded frames per batch
  uint32_t depth = 3;              // batches in flight, >= 3 (H2D, kernels and D2H of three batches overlap)
  uint32_t copy_threads = 4;       // threads that move a source frame into the pinned batch buffer (the caller's included; 1 = the caller alone)
  uint64_t seed = 0;
  svc_ransac_params ransac{1, 7.5f, 0.99f, 0.5f};
  svc_segment_params segment{3, 3, 10, 3, 10, 1.0f, 4};
  bool compact = false;            // the quantised planes leave as the compact stream of include/svc_hip.h ("SVCQ": masks + int16
                                   // levels, ~1 MB instead of 25 MB per 1080p frame): packed on the device, drained by a kernel;
                                   // EncodedBatch::compact instead of coeffs.  Not with `wire`
  uint32_t compact_budget = 0;     // with `compact`: bytes per frame.  Each frame is packed with the finest entry of compact_ladder whose
                                   // frame fits (svc_hip_pack_levels_budget_frames; the transform then leaves RAW planes).  0 = the
                                   // fixed fg_step / bg_step.  SetCompactBudget changes it for a live stream.  With `delta`: a
                                   // group's budget is the sum over its frames (see there)
  std::vector<svc_step_pair> compact_ladder;  // required with a budget: 1 .. 64 (fg_step, bg_step), finest first, non-decreasing
  bool entropy = false;            // with `compact`, not with a budget: every packed frame is coded losslessly on the device ("SVCE",
                                   // svc_hip_entropy_encode_frames) and EncodedBatch::compact carries the SVCE frames; d2h_bytes counts
                                   // the coded bytes.  A budget counts SVCQ bytes, so entropy with compact_budget throws at construction
  uint32_t enh_step = 0;           // with `compact`: two layers (include/svc_hip.h, "Two layers").  EncodedBatch::compact carries the base
                                   // at (fg_step, bg_step), EncodedBatch::enhancement the stream that lifts tiles to enh_step, which
                                   // must divide both.  For every geometry the route is svc_hip_dct_frames (raw planes) then
                                   // svc_hip_pack_layers_frames; with `entropy` both streams are coded.  0 = one layer.  Not with
                                   // `wire`, and not with compact_budget (the budget counts one stream): both throw at construction, as
                                   // do steps the C ABI refuses, with its message
  bool delta = false;              // with `compact`: the DELTA stream (include/svc_hip.h, svc_hip_dct_pack_delta_frames): every frame coded
                                   // against the frame before it in levels, straight from the pixels; EncodedBatch::compact carries it
                                   // (with `entropy`: its SVCE frames) and EncodedBatch::compact_key the key flags.
                                   // svc::StreamDecoder::DecodeDelta plays it.  The chain runs across batches, so the stream does not
                                   // depend on batch or depth; every Encode() starts with a key frame.  Square 8x8 or 16x16 transform
                                   // blocks only; not with `wire` or enh_step: each throws at construction, as does a
                                   // geometry the C ABI refuses, with its message.
                                   // With compact_budget and compact_ladder: a byte budget per GROUP of frames, from a key frame up to
                                   // the next (svc_hip_dct_pack_delta_budget_frames, include/svc_hip_delta_budget.h): the group's frames
                                   // together fit the sum of their budgets at one pair of the ladder, and EncodedBatch::compact_choice
                                   // carries it for every frame.  Accepted exactly when key_interval != 0, batch % key_interval == 0,
                                   // !auto_key, temporal_period == 1 and !entropy -- every batch then holds whole groups and nothing
                                   // is carried across batches; any other combination throws at construction
  double compact_quality = 0;      // with `delta` and compact_ladder: a PSNR in dB that every frame holds, 0 = off
                                   // (svc_hip_dct_pack_delta_quality_frames, include/svc_hip_delta_quality.h).  Per GROUP of frames, from a
                                   // key frame up to the next, the coarsest pair of the ladder at which every frame of the group still
                                   // reaches it; the bytes fall where the content is still.  The target in the units of D is
                                   // floor(255^2 * 3 * padded_w * padded_h * 65536 / 10^(dB / 10)), at most 2^64 - 1.  With compact_budget
                                   // also set the group's budget is a cap, under the rules `delta` states for it.
                                   // EncodedBatch::compact_choice carries each frame's entry (bit 30: the target is not met, bit 31: over
                                   // the cap), compact_distortion its D there.  SetCompactQuality changes it for a live stream.
                                   // Accepted exactly with delta, key_interval != 0, batch % key_interval == 0, !auto_key,
                                   // temporal_period == 1 and no enh_step -- every batch then holds whole groups; `entropy` is allowed (the
                                   // frames are coded unchanged).  Any other combination throws at construction, naming the pair
  uint32_t key_interval = 0;       // with `delta`: the encoded frame with clip index f (as EncodedBatch::first_frame counts: the first
                                   // is 1) is a key frame iff f == 1, or key_interval != 0 and (f - 1) % key_interval == 0
  bool auto_key = false;           // with `delta` (without it the constructor throws): the key frames are chosen by size on the device
                                   // (svc_hip_dct_pack_delta_auto_frames): a frame is a key frame iff the rule above forces it, or its
                                   // difference to the frame before holds at least as many levels as the frame itself -- frame by
                                   // frame the stream is never larger than `compact` alone or `delta` without key frames.
                                   // EncodedBatch::compact_key carries the CHOSEN flags, compact_level_counts what they were chosen
                                   // by.  A frame's choice depends on it and the frame before alone: stream and flags do not
                                   // depend on batch or depth.  With `entropy` the chosen frames are coded unchanged
  uint32_t temporal_period = 1;    // with `delta`: temporal layers (include/svc_hip.h, "Temporal layers").  1, 2 or 4: the encoded frame
                                   // with clip index f has stream index i = f - 1 and is coded against frame i - min(lowbit(i), period), so
                                   // a server thins the stream to 1/2 or 1/4 of the frame rate by dropping frames and their key flags,
                                   // and svc::StreamDecoder::DecodeDeltaTemporal plays it and every thinning.  Above 1 the route is one
                                   // call, svc_hip_dct_pack_delta_temporal_frames (include/svc_hip_temporal.h), straight from the
                                   // pixels as at period 1; the input frame at index -period and its region ids are carried across
                                   // batches on the device, so the stream does not depend on batch or depth.
                                   // The constructor throws for another period, for a period above 1 without `delta` or with auto_key,
                                   // and for a `batch` the period does not divide.  With `entropy` the frames are coded unchanged
  std::function<bool(uint32_t frame, uint32_t xywh[4])> enh_window;  // with enh_step: the window of each encoded frame.  Empty: every
                                   // tile is enhanced (the store-once case: svc_hip_window_levels_frames serves any viewer later).
                                   // Otherwise called on the thread that calls Encode(), while a batch is staged, once per encoded
                                   // frame in clip order; `frame` is the clip index EncodedBatch::first_frame counts in; it fills x, y,
                                   // w, h in padded coordinates (the containment rule of the gaze, on the tile origin); false = an
                                   // empty window
};

// One finished batch; the pointers are pinned host memory owned by the encoder and stay valid
// until depth - 2 more batches have been delivered (a slot is re-staged one iteration before its
// turn to deliver comes again): with the default depth of 3, until the NEXT delivery returns.
struct EncodedBatch {
  uint32_t first_frame = 0;  // clip index of the batch's first encoded frame (frame 0 is tracked-only)
  uint32_t count = 0;
  uint32_t padded_w = 0, padded_h = 0, mv_field_w = 0, mv_field_h = 0;
  const float* mv_xy = nullptr;          // [count][blocks][2]
  const float* global_motion = nullptr;  // [count][2]
  const uint32_t* block_types = nullptr; // [count][blocks], 0 = background
  const float* coeffs = nullptr;         // [count][3][padded_h][padded_w], planes B,G,R (wire == false)
  const uint8_t* records = nullptr;      // [count][record_bytes] (wire == true)
  uint64_t record_bytes = 0;
  const svc_wire_header* header = nullptr;  // wire == true, first batch of a clip only: the 32 bytes that
                                            // open the reference's stream (libs/codec.hpp:8-17, encoder.cpp:360-381)
  const uint8_t* compact = nullptr;           // compact == true: `count` frames of the compact stream back to back (coeffs is null);
                                              // with entropy, its SVCE frames (svc_hip_entropy_decode_frames gives back the SVCQ ones)
  const uint64_t* compact_offsets = nullptr;  // [count + 1]: frame i in [offsets[i], offsets[i + 1])
  uint64_t compact_bytes = 0;                 // = compact_offsets[count]
  const uint32_t* compact_choice = nullptr;   // compact_budget != 0: [count] the ladder entry each frame was packed with, bit 31 set
                                              // when even the last entry is over that frame's budget.  compact_quality != 0: the entry of
                                              // the frame's group in bits 0 .. 29, bit 30 set when the group misses the target there, bit
                                              // 31 when no entry fits the cap
  const uint64_t* compact_distortion = nullptr;  // compact_quality != 0: [count] each frame's D at its chosen entry (include/svc_hip_quality.h;
                                              // PSNR = 10 log10(255^2 * 3 * padded_w * padded_h * 65536 / D))
  const uint32_t* compact_key = nullptr;      // delta == true: [count] != 0 for a key frame, as svc::StreamDecoder::DecodeDelta and
                                              // svc_hip_undelta_levels_frames take them
  const uint32_t* compact_level_counts = nullptr;  // auto_key == true: [count][2] the levels of the frame as a key frame and as a
                                              // difference (equal for a frame without predecessor): svc_hip_dct_pack_delta_auto_frames
  const uint8_t* enhancement = nullptr;           // enh_step != 0: `count` frames of the enhancement stream (SVCQ, or SVCE with entropy),
  const uint64_t* enhancement_offsets = nullptr;  // [count + 1], and
  uint64_t enhancement_bytes = 0;                 // = enhancement_offsets[count]; compact* is then the base.  Lifetime as compact
};

// Where the time of one Encode() went (round 6: the PCIe-inclusive rate explains itself).  Host clocks are wall time of the CALLING thread;
// the three device figures are HIP-event times summed over the batches (the streams overlap: they do not add up to the wall time, the
// largest of them bounds it).
struct EncodeStats {
  uint32_t batches = 0, encoded_frames = 0;
  uint32_t copy_threads = 0;  // threads that stage a source frame into the pinned buffer (the caller's included)
  uint32_t host_cores = 0;    // cores this process may run on (sched_getaffinity)
  double wall_ms = 0;
  double staging_ms = 0;       // host: source frames -> pinned batch buffer (the copy crew), RANSAC draws
  double slot_wait_ms = 0;     // host: waiting for a batch slot whose previous results are still on their way back
  double deliver_wait_ms = 0;  // host: waiting for a batch's results before handing it to the sink
  double sink_ms = 0;          // host: inside the caller's sink
  double h2d_ms = 0, kernels_ms = 0, d2h_ms = 0;  // device, per stream
  uint64_t h2d_bytes = 0, d2h_bytes = 0;  // bytes actually moved (compact: the used bytes of the stream; two layers: of both)
  uint32_t over_budget_frames = 0;        // compact_budget != 0: frames that no ladder entry fit into (compact_choice bit 31)
  uint32_t below_quality_frames = 0;      // compact_quality != 0: frames of groups that miss the target at their entry (compact_choice bit 30)
};

class StreamEncoder {
 public:
  using Sink = std::function<void(const EncodedBatch&)>;
  // Hands out the clip's next source frame (unpadded B,G,R u8, height x width x 3, tightly packed, anywhere in host memory),
  // or nullptr when the clip has ended; the pointer must stay valid until the next call.  May block (a capture queue).
  using Source = std::function<const uint8_t*()>;

  // Allocates every buffer; throws std::runtime_error with the C ABI's message on failure.
  explicit StreamEncoder(const StreamEncoderConfig& config);
  ~StreamEncoder();
  StreamEncoder(const StreamEncoder&) = delete;
  StreamEncoder& operator=(const StreamEncoder&) = delete;

  // Encodes a clip of n_frames >= 2 unpadded B,G,R u8 frames (height x width x 3, tightly packed,
  // anywhere in host memory); sink is called once per batch, in clip order, from this thread.
  void Encode(const uint8_t* bgr, uint32_t n_frames, const Sink& sink);

  // The same for a clip that ARRIVES frame by frame (the reference's reader thread -> queue -> Encoder::operator(),
  // apps/encoder.cpp:125-148): frames are pulled from `next` as the batches need them.  header_frame_count is what the
  // stream's header announces (the reference takes it from the container, libs/encoder.cpp:361-367), not a limit.
  void Encode(const Source& next, uint32_t header_frame_count, const Sink& sink);

  // The byte budget of every frame of each batch STAGED after this returns; a batch already staged keeps the budget it was staged
  // with.  Batches are staged in clip order and batch j + depth - 2 is staged before the sink receives batch j, so a call from inside
  // the sink for batch j applies from batch j + depth - 1 on (with the default depth of 3: j + 2), and a call between Encode() calls
  // applies to the whole next clip.  Safe from any thread.  Throws std::logic_error on an encoder built without a budget, and
  // std::invalid_argument for 0.
  void SetCompactBudget(uint32_t bytes);

  // The same for the quality target, a PSNR in dB: every frame of each batch STAGED after this returns.  Throws std::logic_error on an
  // encoder built without compact_quality, and std::invalid_argument for a value that is not positive and finite.
  void SetCompactQuality(double psnr_db);

  uint32_t padded_width() const;
  uint32_t padded_height() const;
  const EncodeStats& last_stats() const;  // of the last Encode() that returned

 private:
  struct Impl;
  std::unique_ptr<Impl> p_;
};

}  // namespace svc

#endif  // SVC_STREAM_ENCODER_HPP
