// stream_decoder.hpp -- the decoder-side mirror of stream_encoder.hpp: a compact quantised-coefficient stream ("SVCQ", include/svc_hip.h)
// in HOST memory -> the display frames the reference's decoder shows (libs/decoder.cpp:168-210, headless: no window, the gaze centre
// comes from a callback instead of the mouse).
//
// Per frame: the gaze rectangle of svc_hip_gaze_rect around the callback's centre, then svc_hip_decode_levels_frames (DecodeBlock
// over every tile, / 255, bilinear resize, u8).  Batches are staged into pinned memory and copied H2D while the previous batch is
// in the kernels and the one before it is on its way back as u8 display frames.
//
// DecodeWire does the same for the reference's own wire stream (Header + raw-coefficient records, what apps/encoder.cpp writes),
// with svc_hip_wire_layout deciding how the stream is read and svc_hip_decode_records_frames in place of the compact decoder.
#ifndef SVC_STREAM_DECODER_HPP
#define SVC_STREAM_DECODER_HPP

#include <cstdint>
#include <functional>
#include <memory>

#include "svc_hip.h"

namespace svc {

struct StreamDecoderConfig {
  // The size the picture is shown at.  0 x 0 = a default that depends on the stream: Decode (SVCQ) shows the PADDED size, the only
  // size its header holds; DecodeWire shows the header's SOURCE size frame_w x frame_h, what the reference's decoder shows
  // (libs/decoder.cpp:161, :210-211).  Gaze centres are given in display coordinates either way.
  uint32_t display_w = 0, display_h = 0;
  uint32_t fg_step = 1, bg_step = 640;    // the decoder's steps (apps/decoder.cpp:21-26)
  uint32_t max_gaze_w = 64, max_gaze_h = 64;
  uint32_t batch = 16;                    // frames per batch of Decode (a 1080p SVCQ frame is about 1.1 MB)
  // Frames per batch of DecodeWire.  A 1080p wire frame is 25.07 MB of records (23 x the SVCQ frame), and every slot holds a batch of
  // them in pinned AND in device memory: depth x wire_batch x 25 MB = 602 MB pinned at the defaults (1.2 GB at 16).  8 frames are
  // 200 MB per H2D copy, about 4 ms on the link: long enough that the per-batch costs do not show, short enough to keep three
  // batches in flight without pinning a GB.
  uint32_t wire_batch = 8;
  uint32_t depth = 3;                     // batches in flight, >= 3 (H2D, kernels and D2H of three batches overlap)
  // Decode at 1 / reduce of the size from each tile's low frequencies (svc_hip_decode_levels_reduced_frames, for DecodeLayers
  // svc_hip_decode_layers_reduced_frames): 1 = the full decoder, or 2, 4, 8.  Above 1 the picture is the padded size over reduce: a
  // display of 0 x 0 means that size, a larger one throws std::runtime_error at the first Decode or DecodeLayers; gaze centres stay in
  // display coordinates.  Serves Decode and DecodeLayers (SVCQ and SVCE): DecodeWire and DecodeDelta then throw std::runtime_error before
  // any device work, and DecodeDeltaReduced takes only this reduce.
  uint32_t reduce = 1;
};

// One finished batch; the pointers are pinned host memory owned by the decoder and stay valid until depth - 2 more batches have
// been delivered (as for EncodedBatch): with the default depth of 3, until the NEXT delivery returns.
struct DecodedBatch {
  uint32_t first_frame = 0;        // stream index of the batch's first frame
  uint32_t count = 0;
  uint32_t width = 0, height = 0;  // of a display frame
  const uint8_t* bgr = nullptr;    // [count][height][width][3] u8 B,G,R
  const uint32_t* status = nullptr;  // [count]: 0, or svc_hip_unpack_levels_frames's code (the frame is then all zeros); an SVCE
                                    // frame the entropy decoder refuses: svc_hip_entropy_decode_frames's code; DecodeWire: 0;
                                    // DecodeLayers: stated there
};

// Where the time of one Decode() / DecodeWire() went: wall time of the calling thread; per-stream device times summed over the batches (the
// streams overlap); the bytes actually moved each way.
struct DecodeStats {
  uint32_t batches = 0, frames = 0;
  double wall_ms = 0;
  double h2d_ms = 0, kernels_ms = 0, d2h_ms = 0;
  uint64_t h2d_bytes = 0, d2h_bytes = 0;
};

class StreamDecoder {
 public:
  using Sink = std::function<void(const DecodedBatch&)>;
  // Frame index -> gaze centre in display-frame coordinates (where the reference reads the mouse); false = no gaze for that frame.
  using Gaze = std::function<bool(uint32_t frame, uint32_t* x, uint32_t* y)>;

  // Creates the streams; buffers are sized by the first Decode().  Throws std::runtime_error on an invalid configuration.
  explicit StreamDecoder(const StreamDecoderConfig& config);
  ~StreamDecoder();
  StreamDecoder(const StreamDecoder&) = delete;
  StreamDecoder& operator=(const StreamDecoder&) = delete;

  // stream: n_frames SVCQ frames, or SVCE frames (chosen by the first frame's magic: decoded to SVCQ on the device by
  // svc_hip_entropy_decode_frames, then as SVCQ), anywhere in host memory, frame i in [offsets[i], offsets[i + 1]) (offsets: n_frames + 1 values,
  // the shape of EncodedBatch::compact / compact_offsets).  The geometry comes from the first frame's header, which must parse
  // (else std::runtime_error); any later frame that does not match is reported in DecodedBatch::status, not thrown.  gaze may be
  // empty (no gaze).  sink is called once per batch, in stream order, from this thread.
  void Decode(const uint8_t* stream, const uint64_t* offsets, uint32_t n_frames, const Gaze& gaze, const Sink& sink);

  // Two layers (include/svc_hip.h, "Two layers"): a base stream and its enhancement stream, n_frames frames each, the shape of
  // EncodedBatch::compact / enhancement.  Each stream is SVCQ or SVCE by its own first frame's magic (an SVCE stream goes through
  // svc_hip_entropy_decode_frames first); the geometry comes from the base's first header, and the enhancement's first header must parse
  // and name the same geometry (else std::runtime_error).  Schedule, gaze rectangles, display size and statistics as Decode; the device
  // call is svc_hip_decode_layers_frames, with config.reduce above 1 svc_hip_decode_layers_reduced_frames: inside the gaze a tile decodes
  // at the enhancement's step.  With an empty `gaze` the enhancement is not read (it may be null) and the call is Decode on the base
  // (at that reduce); a frame whose callback returns false decodes as the base alone.  DecodedBatch::status: the entropy decoder's code
  // for the base frame if it is not 0, else 0x100 | its code for the enhancement frame, else the code of svc_hip_decode_layers_frames.
  // One decoder serves Decode, DecodeWire and DecodeLayers in any order.
  void DecodeLayers(const uint8_t* base, const uint64_t* base_offsets, const uint8_t* enh, const uint64_t* enh_offsets, uint32_t n_frames,
                    const Gaze& gaze, const Sink& sink);

  // A delta stream (include/svc_hip.h, "A stored SVCQ stream cut by time"): n_frames frames coded against their predecessors by
  // svc_hip_delta_levels_frames, as ONE chain -- frame 0 has no predecessor, frame i > 0 hangs on reconstructed frame i - 1 unless
  // key[i] != 0 (key: n_frames host flags as the delta call took them, or null: only frame 0 is a key frame).  SVCQ or SVCE by the first
  // frame's magic (SVCE goes through svc_hip_entropy_decode_frames first, as in Decode).  Schedule, gaze rectangles, display size and
  // statistics are Decode's.  The device call is svc_hip_decode_delta_levels_frames -- the undelta and the decode in one kernel, which
  // measures faster than the two calls at both densities (README, profiles/decode_delta_c3.txt) -- and two one-frame device buffers carry
  // its d_last of batch b into the d_prev of batch b + 1 on the kernel stream, so the display frames do not depend on the batch size or
  // the depth.  The next batch's call needs the carried frame's length on the host: 8 bytes come back on the kernel stream, and the host
  // waits for batch b's kernels before it enqueues batch b + 1's (its H2D copy is in flight by then).  DecodedBatch::status: the entropy
  // decoder's code if it is not 0, else svc_hip_undelta_levels_frames's (a failure runs down the chain to the next key frame).
  // config.reduce above 1 throws std::runtime_error before any device work (DecodeDeltaReduced is the method for that).  One decoder
  // serves all methods in any order.
  void DecodeDelta(const uint8_t* stream, const uint64_t* offsets, uint32_t n_frames, const uint32_t* key, const Gaze& gaze,
                   const Sink& sink);

  // DecodeDelta at 1 / reduce of the size: the device call is svc_hip_decode_delta_levels_reduced_frames, which carries only the first
  // K x K levels of every tile through time (K = tile side / reduce).  reduce is 2, 4 or 8; the size belongs to the chain, so it is an
  // argument: config.reduce must be 1 or equal to it, and the configured display (0 x 0: the padded frame over reduce) must fit the padded
  // frame over reduce, else std::runtime_error before any device work.  Gaze centres stay in display coordinates, as in Decode under
  // config.reduce.  `stream` is the full delta stream or its band (0, 0, K, K) (svc_hip_band_levels_frames: what a server sends a small
  // viewer), SVCQ or SVCE by the first frame's magic; the display frames are the same for both.  The two chain buffers hold band frames
  // here -- this is the only route that carries a band-sized chain, so the driver uses the fused call whatever it measures against the
  // two calls (README).  Everything else -- key flags, schedule, statuses, statistics -- is DecodeDelta's.
  void DecodeDeltaReduced(const uint8_t* stream, const uint64_t* offsets, uint32_t n_frames, const uint32_t* key, uint32_t reduce,
                          const Gaze& gaze, const Sink& sink);

  // DecodeDelta for a delta stream with temporal layers (include/svc_hip.h, "Temporal layers"; svc::StreamEncoderConfig::temporal_period
  // writes one): frame i hangs on reconstructed frame i - min(lowbit(i), period), period 1, 2 or 4.  The device call is
  // svc_hip_decode_delta_levels_temporal_frames, the undelta and the decode in one kernel (against the two calls: README,
  // profiles/temporal_delta_c3.txt); its d_last, frame period * ((n - 1) / period) of a batch, is the next batch's d_prev, so
  // config.batch must be a multiple of period (else std::runtime_error before any device work, as for another period).  The stream
  // thinned to every 2^s-th frame (frames and key flags copied) plays with period >> s; period 1 forwards to DecodeDelta.  Everything
  // else -- SVCQ or SVCE by magic, key flags, schedule, statistics -- is DecodeDelta's; a failure runs down the tree of references.
  void DecodeDeltaTemporal(const uint8_t* stream, const uint64_t* offsets, uint32_t n_frames, const uint32_t* key, uint32_t period,
                           const Gaze& gaze, const Sink& sink);

  // DecodeDeltaTemporal at 1 / reduce of the size: a temporal-layer delta stream, or its band (0, 0, K, K) (K = tile side / reduce), played
  // small.  The device call is svc_hip_decode_delta_levels_temporal_reduced_frames (include/svc_hip_temporal_decode.h), which carries the first
  // K x K levels of every tile in one set of registers per temporal layer; the two chain buffers hold the band of frame
  // period * ((n - 1) / period) of a batch, the next batch's d_prev.  It is the only route whose chain runs on band-sized frames, so the
  // driver takes it whatever it measures against the undelta and the reduced decode as two calls (README,
  // profiles/decode_delta_temporal_reduced_c3.txt).  Thrown as std::runtime_error before any device work: a period other than 1, 2 or 4;
  // a reduce other than 2, 4 or 8; config.reduce neither 1 nor `reduce`; config.batch not a multiple of period.  period 1 forwards to
  // DecodeDeltaReduced.  The stream thinned to every 2^s-th frame plays with period >> s.  Everything else -- SVCQ or SVCE by magic,
  // key flags, gaze in display coordinates, display size, schedule, statuses, statistics -- is DecodeDeltaReduced's and
  // DecodeDeltaTemporal's.
  void DecodeDeltaTemporalReduced(const uint8_t* stream, const uint64_t* offsets, uint32_t n_frames, const uint32_t* key, uint32_t period,
                                  uint32_t reduce, const Gaze& gaze, const Sink& sink);

  // stream: a whole wire stream of `bytes` bytes in host memory, the 32-byte Header (libs/codec.hpp:8-17) first, then frame_count
  // frames of records.  svc_hip_wire_layout decides how it is read (the decoder's padded tile grid, or the reference encoder's
  // unpadded loops); a stream it refuses throws std::runtime_error with its message.  Batches of config.wire_batch frames, the
  // schedule of Decode; every DecodedBatch::status is 0.  last_stats() is filled as for Decode.
  void DecodeWire(const uint8_t* stream, uint64_t bytes, const Gaze& gaze, const Sink& sink);

  const DecodeStats& last_stats() const;  // of the last Decode() that returned

 private:
  struct Impl;
  std::unique_ptr<Impl> p_;
};

}  // namespace svc

#endif  // SVC_STREAM_DECODER_HPP
