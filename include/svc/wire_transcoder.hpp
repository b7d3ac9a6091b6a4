// wire_transcoder.hpp -- the bridge between the two streams for streams in HOST memory: the reference's wire stream (Header + one
// raw-coefficient record per tile, what apps/encoder.cpp and svc::StreamEncoder{wire = true} write) <-> the compact stream ("SVCQ", or
// entropy-coded "SVCE"; include/svc_hip.h).  Stream to stream on the device (svc_hip_records_pack_levels_frames,
// svc_hip_levels_records_frames): no pixels and no coefficient planes.
//
// The schedule is that of svc::StreamDecoder: batches are staged into pinned memory and copied H2D while the previous batch is in
// the kernels and the one before it is on its way back.
#ifndef SVC_WIRE_TRANSCODER_HPP
#define SVC_WIRE_TRANSCODER_HPP

#include <cstdint>
#include <functional>
#include <memory>

#include "svc_hip.h"

namespace svc {

struct WireTranscoderConfig {
  // ToCompact: the quant steps of the compact stream, and its MV block (the wire header carries none): 0 = the tile, else a
  // multiple of the tile that divides the padded frame.  An MV block's type is the type word of the record at its origin.
  uint32_t fg_step = 1, bg_step = 640;
  uint32_t mv_block_w = 0, mv_block_h = 0;
  bool entropy = false;     // ToCompact delivers SVCE (svc_hip_entropy_encode_frames on the device) instead of SVCQ
  // Frames per batch.  A 1080p wire frame is 25.07 MB of records and every slot holds a batch of them in pinned AND in device memory:
  // depth x wire_batch x 25 MB = 602 MB pinned at the defaults, as StreamDecoderConfig::wire_batch.
  uint32_t wire_batch = 8;
  uint32_t depth = 3;       // batches in flight, >= 3
};

// One finished batch of ToCompact; the pointers are pinned host memory owned by the transcoder and stay valid until depth - 2 more
// batches have been delivered: with the default depth of 3, until the NEXT delivery returns.
struct CompactBatch {
  uint32_t first_frame = 0, count = 0;
  uint32_t frame_w = 0, frame_h = 0, block = 0, mv_block_w = 0, mv_block_h = 0;  // the compact stream's geometry (the padded size)
  bool entropy = false;               // frames are SVCE
  const uint8_t* frames = nullptr;    // frame i of the batch in [offsets[i], offsets[i + 1])
  const uint64_t* offsets = nullptr;  // [count + 1], offsets[0] == 0
  const uint32_t* status = nullptr;   // [count]: 0, or 4 for a frame in which a record's type word differs from its MV block's
};

// One finished batch of ToWire: count frames of records, frame i at records + i * frame_bytes -- what follows the 32-byte Header in
// a wire stream.  The caller writes the Header (svc_hip_wire_header's fields; frame_w + frame_excess_w = frame_w here).
struct WireBatch {
  uint32_t first_frame = 0, count = 0;
  uint32_t frame_w = 0, frame_h = 0, block = 0, emit_frame_h = 0;  // the padded size; the rows of it the records cover
  uint64_t frame_bytes = 0;
  const uint8_t* records = nullptr;
  const uint32_t* status = nullptr;  // [count]: 0, or the code of svc_hip_unpack_levels_frames (the frame is then all-zero records); an
                                     // SVCE frame the entropy decoder refuses: svc_hip_entropy_decode_frames's code
};

struct TranscodeStats {  // of the last call that returned: as svc::DecodeStats
  uint32_t batches = 0, frames = 0;
  double wall_ms = 0;
  double h2d_ms = 0, kernels_ms = 0, d2h_ms = 0;
  uint64_t h2d_bytes = 0, d2h_bytes = 0;
};

class WireTranscoder {
 public:
  using CompactSink = std::function<void(const CompactBatch&)>;
  using WireSink = std::function<void(const WireBatch&)>;

  // Creates the streams; buffers are sized by the first call.  Throws std::runtime_error on an invalid configuration.
  explicit WireTranscoder(const WireTranscoderConfig& config);
  ~WireTranscoder();
  WireTranscoder(const WireTranscoder&) = delete;
  WireTranscoder& operator=(const WireTranscoder&) = delete;

  // stream: a whole wire stream of `bytes` bytes in host memory, the 32-byte Header first.  svc_hip_wire_layout decides how it is read
  // (the decoder's padded tile grid, or the reference encoder's unpadded loops, whose missing tile rows become zero coefficients); a
  // stream it refuses throws std::runtime_error with its message, as does a geometry or a step svc_hip_records_pack_levels_frames
  // refuses.  sink is called once per batch of config.wire_batch frames, in stream order, from this thread.
  void ToCompact(const uint8_t* stream, uint64_t bytes, const CompactSink& sink);

  // compact: n_frames SVCQ or SVCE frames (by the first frame's magic) anywhere in host memory, frame i in [offsets[i], offsets[i + 1]).
  // The geometry comes from the first frame's header, which must parse (else std::runtime_error) and hold square tiles; a later frame
  // that does not match is reported in WireBatch::status.  emit_frame_h: the rows of the padded frame the records cover, 0 = all (the
  // reading of the reference's decoder).
  void ToWire(const uint8_t* compact, const uint64_t* offsets, uint32_t n_frames, uint32_t emit_frame_h, const WireSink& sink);

  const TranscodeStats& last_stats() const;

 private:
  struct Impl;
  std::unique_ptr<Impl> p_;
};

}  // namespace svc

#endif  // SVC_WIRE_TRANSCODER_HPP
