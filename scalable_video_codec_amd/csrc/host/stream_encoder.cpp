// stream_encoder.cpp -- include/svc/stream_encoder.hpp: buffers and what a batch does on each stream of batch_pipe.hpp's schedule.
// No arithmetic of the hot path lives here; every stage is a call into the C ABI.
#include "svc/stream_encoder.hpp"

#include "batch_pipe.hpp"
#include "copy_crew.hpp"
#include "encode_geometry.hpp"
#include "svc_hip_delta_budget.h"
#include "svc_hip_delta_quality.h"
#include "svc_hip_temporal.h"

#include <sched.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

namespace svc {
namespace {

using namespace host;

constexpr Who kWho{"svc::StreamEncoder"};
void Hip(hipError_t e, const char* what) { kWho.Hip(e, what); }
void Abi(int rc, const char* what) { kWho.Abi(rc, what); }

struct Slot {
  DevBuf<uint8_t> bgr, pyr, mask, seg_ws, records, packed, pack_ws, coded, entropy_ws;
  DevBuf<uint64_t> offsets, coded_offsets;
  DevBuf<uint32_t> entropy_status;
  PinBuf<uint32_t> pin_entropy_status;
  PinBuf<uint8_t> pin_packed;
  PinBuf<uint64_t> pin_offsets;
  DevBuf<float> mv, mad, gm, rmse, coeffs;
  DevBuf<uint32_t> count, types, samples, budget, choice;
  PinBuf<uint32_t> pin_samples, pin_budget, pin_choice;
  PinBuf<uint8_t> pin_in, pin_records;
  PinBuf<float> pin_mv, pin_gm, pin_coeffs;
  PinBuf<uint32_t> pin_types;
  // two layers: the enhancement stream's buffers beside the base's (packed, offsets, coded ...), and the frames' windows
  DevBuf<uint8_t> enh_packed, enh_coded;
  DevBuf<uint64_t> enh_offsets, enh_coded_offsets;
  DevBuf<uint32_t> enh_status, window;
  PinBuf<uint8_t> pin_enh;
  PinBuf<uint64_t> pin_enh_offsets;
  PinBuf<uint32_t> pin_enh_status, pin_window;
  // delta: the frames' key flags
  DevBuf<uint32_t> key;
  PinBuf<uint32_t> pin_key;
  // auto_key: the flags the caller's rule forces (key then holds the device's choice), and both level counts of every frame
  DevBuf<uint32_t> forced, level_counts;
  PinBuf<uint32_t> pin_forced, pin_level_counts;
  // temporal_period > 1: the input frame at index -period of the batch's first encoded frame, copied on the device from the slot before
  DevBuf<uint8_t> before_bgr;
  // compact_quality: the frames' targets, the table D[frame][entry] of the batch and, gathered at delivery, each frame's D at its entry
  DevBuf<uint64_t> target, dist_table;
  PinBuf<uint64_t> pin_target, pin_dist_table, pin_distortion;
  uint32_t frames = 0;  // source frames resident in bgr (the last one carries into the next batch)
  uint32_t encoded = 0, first = 0;
};

// layers.distortion_target: the largest D that still reaches psnr_db on a w x h frame, floor(255^2 * 3 w h * 65536 / 10^(dB / 10)), at most
// 2^64 - 1.  In long double: exact wherever 10^(dB / 10) is an integer (the scale of a frame the stream calls take is below 2^64).
uint64_t DistortionTarget(double psnr_db, uint32_t w, uint32_t h) {
  const long double scale = 65025.0L * 3.0L * (long double)w * (long double)h * 65536.0L;
  const long double d = std::floor(scale / std::pow(10.0L, (long double)psnr_db / 10.0L));
  return d >= 18446744073709551615.0L ? ~0ull : (uint64_t)d;
}

}  // namespace

struct StreamEncoder::Impl : EncodeGeometry {
  StreamEncoderConfig c;
  uint32_t iters = 0;
  uint32_t bw = 0, bh = 0, tw = 0, th = 0;  // MV block and transform block sides
  uint64_t record_bytes = 0, seg_ws_bytes = 0;
  uint64_t packed_bytes = 0, pack_ws_bytes = 0;  // compact: worst case of a batch, pack workspace
  uint64_t coded_bytes = 0, entropy_ws_bytes = 0; // entropy: worst case of a coded batch, coder workspace
  bool budgeted = false;                          // compact_budget != 0: rate control
  bool group_budget = false;                      // ... of the delta stream: a budget per group of frames, svc_hip_dct_pack_delta_budget_frames
  bool layered = false;                           // enh_step != 0: a base and an enhancement stream
  bool temporal = false;                          // delta with temporal_period > 1: svc_hip_dct_pack_delta_temporal_frames
  std::atomic<uint32_t> budget{0};                // bytes per frame of the next batch staged (SetCompactBudget)
  bool quality = false;                           // compact_quality != 0: a distortion target per group of frames, svc_hip_dct_pack_delta_quality_frames
  std::atomic<uint64_t> target{0};                // in the units of D, for every frame of the next batch staged (SetCompactQuality)
  std::vector<std::unique_ptr<Slot>> slots;       // the buffers of the pipe's slots
  bool fused_records = false;  // wire: the transform kernel emits the records itself
  std::unique_ptr<CopyCrew> crew;
  std::unique_ptr<BatchPipe> pipe;  // (after the buffers: its streams synchronise before those go)
  EncodeStats stats;
};

StreamEncoder::StreamEncoder(const StreamEncoderConfig& config) : p_(new Impl) {
  Impl& m = *p_;
  m.c = config;
  const StreamEncoderConfig& c = m.c;
  if (!c.width || !c.height || !c.levels || !c.mv_block || c.batch == 0 || c.depth < 3)
    throw std::runtime_error("svc::StreamEncoder: invalid configuration");
  m.bw = c.mv_block; m.bh = c.mv_block_h ? c.mv_block_h : c.mv_block;
  m.tw = c.dct_block; m.th = c.dct_block_h ? c.dct_block_h : c.dct_block;
  if (!m.tw || !m.th) throw std::runtime_error("svc::StreamEncoder: invalid configuration");
  if (c.delta && c.wire) throw std::runtime_error("svc::StreamEncoder: the delta stream is a form of the compact stream, not of the wire records");
  if (c.delta && !c.compact) throw std::runtime_error("svc::StreamEncoder: the delta stream is a form of the compact stream");
  // a quality target: the delta stream's, one pair of steps per group of frames, and a batch must hold whole groups as under a budget
  if (c.compact_quality != 0) {
    auto refuse = [](const std::string& why) { throw std::runtime_error("svc::StreamEncoder: compact_quality " + why); };
    if (!(c.compact_quality > 0) || !std::isfinite(c.compact_quality)) refuse("is a PSNR in dB: positive and finite, or 0 for off");
    if (!c.delta) refuse("holds every frame of the delta stream at a PSNR: not without delta");
    if (c.enh_step) refuse("measures one layer: not with enh_step");
    if (c.temporal_period > 1) refuse("picks one pair of steps per group of consecutive frames: not with temporal_period " + std::to_string(c.temporal_period));
    if (c.auto_key) refuse("needs the groups before it chooses, auto_key the steps before it cuts them: not with auto_key");
    if (c.key_interval == 0 || c.batch % c.key_interval != 0)
      refuse("picks one pair of steps per group of frames, from a key frame up to the next: every batch must hold whole groups (key_interval " +
             std::to_string(c.key_interval) + " must be positive and divide batch " + std::to_string(c.batch) + ")");
  }
  // a byte budget with delta: one pair of steps per group of frames, and a batch must hold whole groups (svc_hip_dct_pack_delta_budget_frames
  // takes no frame before frame 0) -- key frames at a fixed interval that divides the batch, nothing chosen or referred to across them
  if (c.delta && c.compact_budget &&
      !(c.key_interval != 0 && c.batch % c.key_interval == 0 && !c.auto_key && c.temporal_period == 1 && !c.entropy))
    throw std::runtime_error("svc::StreamEncoder: a byte budget picks one pair of steps per group of frames, from a key frame up to the next, and "
                             "a difference needs the steps of the frame before: not with delta unless every batch holds whole groups "
                             "(key_interval != 0 that divides batch, no auto_key, temporal_period 1, no entropy)");
  if (c.auto_key && !c.delta) throw std::runtime_error("svc::StreamEncoder: auto_key chooses the key frames of the delta stream: not without delta");
  if (c.delta && c.enh_step) throw std::runtime_error("svc::StreamEncoder: the delta stream has one layer: not with enh_step");
  if (c.temporal_period != 1 && c.temporal_period != 2 && c.temporal_period != 4)
    throw std::runtime_error("svc::StreamEncoder: temporal_period " + std::to_string(c.temporal_period) + " (supported: 1, 2, 4)");
  if (c.temporal_period > 1 && !c.delta)
    throw std::runtime_error("svc::StreamEncoder: temporal_period chooses the frame each frame of the delta stream is coded against: not without delta");
  if (c.temporal_period > 1 && c.auto_key)
    throw std::runtime_error("svc::StreamEncoder: auto_key weighs a frame against the frame before it, not against its temporal reference: not with temporal_period");
  if (c.batch % c.temporal_period != 0)
    throw std::runtime_error("svc::StreamEncoder: every batch but the last holds a multiple of temporal_period frames: batch " +
                             std::to_string(c.batch) + " is not a multiple of " + std::to_string(c.temporal_period));
  m.temporal = c.delta && c.temporal_period > 1;
  if (c.compact && c.wire) throw std::runtime_error("svc::StreamEncoder: compact is a form of the quantised planes, not of the wire records");
  static_cast<EncodeGeometry&>(m) = EncodeGeometry(c.width, c.height, c.levels, m.bw, m.bh);
  // reference_stream: SerializeEncodedFrame over the UNPADDED size (libs/encoder.cpp:647-650); the transform kernel emits that
  // directly when the padded width IS the frame's width (emit height = the unpadded one); with a padded width the row
  // stride quirk needs the planes first and svc_hip_serialize_frames behind them
  m.record_bytes = !c.wire ? 0 : c.reference_stream ? svc_hip_serialized_frame_bytes(c.width, c.height, m.tw, m.th)
                                                    : svc_hip_serialized_frame_bytes(m.pw, m.ph, m.tw, m.th);
  m.fused_records = c.wire && m.tw == m.th && (!c.reference_stream || m.pw == c.width);
  m.iters = svc_hip_ransac_iter_count(c.ransac);
  m.seg_ws_bytes = svc_hip_segment_workspace_bytes(m.mfw, m.mfh, c.batch, c.segment.attempt_count);
  if (c.compact_budget && !c.compact) throw std::runtime_error("svc::StreamEncoder: a byte budget is a setting of the compact stream");
  m.budgeted = c.compact_budget != 0;
  m.budget.store(c.compact_budget);
  m.quality = c.compact_quality != 0;
  m.group_budget = m.budgeted && c.delta && !m.quality;
  if (m.quality) {  // the call's checks that need neither a device pointer nor a size: geometry, the ladder
    if (m.tw != m.th)
      throw std::runtime_error("svc::StreamEncoder: the delta stream takes square transform blocks (8x8, 16x16), not " + std::to_string(m.tw) + "x" +
                               std::to_string(m.th));
    Abi(svc_hip_dct_pack_delta_quality_frames(nullptr, m.frame_bytes, 0, m.pw, m.ph, m.tw, nullptr, m.bw, m.bh, c.compact_ladder.data(),
                                              (uint32_t)c.compact_ladder.size(), nullptr, nullptr, nullptr, nullptr, ~0ull, nullptr, ~0ull, nullptr,
                                              nullptr, nullptr, nullptr, nullptr), "compact_ladder");
    m.target.store(DistortionTarget(c.compact_quality, m.pw, m.ph));
  } else if (m.group_budget) {  // the call's checks that need neither a device pointer nor a size: geometry, the ladder
    if (m.tw != m.th)
      throw std::runtime_error("svc::StreamEncoder: the delta stream takes square transform blocks (8x8, 16x16), not " + std::to_string(m.tw) + "x" +
                               std::to_string(m.th));
    Abi(svc_hip_dct_pack_delta_budget_frames(nullptr, m.frame_bytes, 0, m.pw, m.ph, m.tw, nullptr, m.bw, m.bh, c.compact_ladder.data(),
                                             (uint32_t)c.compact_ladder.size(), nullptr, nullptr, nullptr, ~0ull, nullptr, ~0ull, nullptr, nullptr,
                                             nullptr, nullptr), "compact_ladder");
  } else if (m.budgeted)  // the budgeted pack's checks that need neither a device pointer nor a size: geometry, the ladder, the int16 bound
    Abi(svc_hip_pack_levels_budget_frames(nullptr, nullptr, 0, m.pw, m.ph, m.tw, m.th, m.bw, m.bh, c.compact_ladder.data(),
                                          (uint32_t)c.compact_ladder.size(), nullptr, nullptr, ~0ull, nullptr, ~0ull, nullptr, nullptr,
                                          nullptr), "compact_ladder");
  if (c.entropy && !c.compact) throw std::runtime_error("svc::StreamEncoder: entropy coding is a form of the compact stream");
  if (c.entropy && c.compact_budget)
    throw std::runtime_error("svc::StreamEncoder: a byte budget counts uncoded compact bytes: not with entropy");
  m.layered = c.enh_step != 0;
  if (m.layered && c.wire) throw std::runtime_error("svc::StreamEncoder: an enhancement layer is a form of the compact stream, not of the wire records");
  if (m.layered && !c.compact) throw std::runtime_error("svc::StreamEncoder: an enhancement layer is a form of the compact stream");
  if (m.layered && c.compact_budget) throw std::runtime_error("svc::StreamEncoder: a byte budget counts one stream: not with enh_step");
  if (m.layered)  // the layered pack's checks that need neither a device pointer nor a size: geometry, the steps, the int16 bounds
    Abi(svc_hip_pack_layers_frames(nullptr, nullptr, 0, m.pw, m.ph, m.tw, m.th, m.bw, m.bh, c.fg_step, c.bg_step, c.enh_step, nullptr, nullptr,
                                   ~0ull, nullptr, ~0ull, nullptr, nullptr, ~0ull, nullptr, nullptr), "enh_step");
  if (c.delta) {  // the call's checks that need neither a device pointer nor a size: geometry (square 8x8 / 16x16 tiles, whole segments), the steps
    if (m.tw != m.th)
      throw std::runtime_error("svc::StreamEncoder: the delta stream takes square transform blocks (8x8, 16x16), not " + std::to_string(m.tw) + "x" +
                               std::to_string(m.th));
    Abi(svc_hip_dct_pack_delta_frames(nullptr, m.frame_bytes, 0, m.pw, m.ph, m.tw, nullptr, m.bw, m.bh, c.fg_step, c.bg_step, nullptr, nullptr,
                                      nullptr, nullptr, ~0ull, nullptr, ~0ull, nullptr, nullptr), "delta");
  }
  if (c.entropy) {
    m.coded_bytes = svc_hip_entropy_max_bytes(c.batch, m.pw, m.ph, m.tw, m.th, m.bw, m.bh);
    m.entropy_ws_bytes = svc_hip_entropy_workspace_bytes(c.batch, m.pw, m.ph, m.tw, m.th, m.bw, m.bh);
    if (!m.coded_bytes || !m.entropy_ws_bytes) throw std::runtime_error("svc::StreamEncoder: no entropy-coded stream for this geometry");
  }
  if (c.compact) {
    m.packed_bytes = svc_hip_levels_max_bytes(c.batch, m.pw, m.ph, m.tw, m.th, m.bw, m.bh);
    m.pack_ws_bytes = m.quality ? svc_hip_dct_pack_delta_quality_workspace_bytes(c.batch, m.pw, m.ph, m.tw, m.bw, m.bh, (uint32_t)c.compact_ladder.size())
                      : m.group_budget ? svc_hip_dct_pack_delta_budget_workspace_bytes(c.batch, m.pw, m.ph, m.tw, m.bw, m.bh, (uint32_t)c.compact_ladder.size())
                      : m.budgeted ? svc_hip_pack_levels_budget_workspace_bytes(c.batch, m.pw, m.ph, m.tw, m.th, (uint32_t)c.compact_ladder.size())
                      : m.layered ? svc_hip_pack_layers_workspace_bytes(c.batch, m.pw, m.ph, m.tw, m.th)
                      : c.auto_key ? svc_hip_dct_pack_delta_auto_workspace_bytes(c.batch, m.pw, m.ph, m.tw, m.bw, m.bh)
                      : m.temporal ? svc_hip_dct_pack_delta_temporal_workspace_bytes(c.batch, m.pw, m.ph, m.tw, m.bw, m.bh, c.temporal_period)
                      : c.delta   ? svc_hip_dct_pack_delta_workspace_bytes(c.batch, m.pw, m.ph, m.tw, m.bw, m.bh)
                                  : svc_hip_pack_levels_workspace_bytes(c.batch, m.pw, m.ph, m.tw, m.th);
    if (!m.packed_bytes || !m.pack_ws_bytes)
      throw std::runtime_error("svc::StreamEncoder: no compact stream for this geometry");
  }
  m.crew.reset(new CopyCrew(std::min<uint32_t>(c.copy_threads ? c.copy_threads - 1 : 0, 15)));
  m.pipe.reset(new BatchPipe(kWho, c.depth));
  const size_t B = c.batch;
  for (uint32_t i = 0; i < c.depth; ++i) {
    std::unique_ptr<Slot> s(new Slot);
    s->bgr.Alloc(kWho, (B + 1) * m.frame_bytes);
    Hip(hipMemset(s->bgr.p, 0, (B + 1) * m.frame_bytes), "hipMemset");  // a short last batch runs the kernels over the whole slot
    s->pyr.Alloc(kWho, (B + 1) * m.pyr_stride);
    s->mv.Alloc(kWho, B * m.blocks * 2); s->mad.Alloc(kWho, B * m.blocks);
    s->gm.Alloc(kWho, B * 2); s->rmse.Alloc(kWho, B);
    s->mask.Alloc(kWho, B * m.blocks); s->count.Alloc(kWho, B); s->types.Alloc(kWho, B * m.blocks);
    s->seg_ws.Alloc(kWho, m.seg_ws_bytes);
    s->pin_in.Alloc(kWho, (B + 1) * m.frame_bytes);
    std::memset(s->pin_in.p, 0, (B + 1) * m.frame_bytes);  // the padding border stays zero (encoder.cpp:459-461)
    s->pin_mv.Alloc(kWho, B * m.blocks * 2); s->pin_gm.Alloc(kWho, B * 2); s->pin_types.Alloc(kWho, B * m.blocks);
    s->samples.Alloc(kWho, B * m.iters * c.ransac.subset_sz); s->pin_samples.Alloc(kWho, B * m.iters * c.ransac.subset_sz);
    Hip(hipMemset(s->samples.p, 0, std::max<size_t>(B * m.iters * c.ransac.subset_sz, 1) * sizeof(uint32_t)), "hipMemset");
    if (c.wire) { s->records.Alloc(kWho, B * m.record_bytes); s->pin_records.Alloc(kWho, B * m.record_bytes); }
    if ((!c.wire || !m.fused_records) && !c.delta) s->coeffs.Alloc(kWho, B * 3 * m.plane_elems);  // (the delta route has no planes)
    if (!c.wire && !c.compact) s->pin_coeffs.Alloc(kWho, B * 3 * m.plane_elems);
    if (c.compact) {
      s->packed.Alloc(kWho, m.packed_bytes); s->pack_ws.Alloc(kWho, m.pack_ws_bytes); s->offsets.Alloc(kWho, B + 1);
      s->pin_packed.Alloc(kWho, c.entropy ? m.coded_bytes : m.packed_bytes); s->pin_offsets.Alloc(kWho, B + 1);
      if (c.entropy) {
        s->coded.Alloc(kWho, m.coded_bytes); s->entropy_ws.Alloc(kWho, m.entropy_ws_bytes); s->coded_offsets.Alloc(kWho, B + 1);
        s->entropy_status.Alloc(kWho, B); s->pin_entropy_status.Alloc(kWho, B);
      }
    }
    if (m.layered) {
      s->enh_packed.Alloc(kWho, m.packed_bytes); s->enh_offsets.Alloc(kWho, B + 1);
      s->pin_enh.Alloc(kWho, c.entropy ? m.coded_bytes : m.packed_bytes); s->pin_enh_offsets.Alloc(kWho, B + 1);
      if (c.entropy) {
        s->enh_coded.Alloc(kWho, m.coded_bytes); s->enh_coded_offsets.Alloc(kWho, B + 1);
        s->enh_status.Alloc(kWho, B); s->pin_enh_status.Alloc(kWho, B);
      }
      if (c.enh_window) { s->window.Alloc(kWho, B * 4); s->pin_window.Alloc(kWho, B * 4); }
    }
    if (c.delta) { s->key.Alloc(kWho, B); s->pin_key.Alloc(kWho, B); }
    if (m.temporal) s->before_bgr.Alloc(kWho, m.frame_bytes);
    if (c.auto_key) {
      s->forced.Alloc(kWho, B); s->pin_forced.Alloc(kWho, B);
      s->level_counts.Alloc(kWho, 2 * B); s->pin_level_counts.Alloc(kWho, 2 * B);
    }
    if (m.budgeted) { s->budget.Alloc(kWho, B); s->pin_budget.Alloc(kWho, B); }
    if (m.budgeted || m.quality) { s->choice.Alloc(kWho, B); s->pin_choice.Alloc(kWho, B); }
    if (m.quality) {
      const size_t L = c.compact_ladder.size();
      s->target.Alloc(kWho, B); s->pin_target.Alloc(kWho, B);
      s->dist_table.Alloc(kWho, B * L); s->pin_dist_table.Alloc(kWho, B * L); s->pin_distortion.Alloc(kWho, B);
    }
    m.slots.push_back(std::move(s));
  }
}

StreamEncoder::~StreamEncoder() = default;
uint32_t StreamEncoder::padded_width() const { return p_->pw; }
uint32_t StreamEncoder::padded_height() const { return p_->ph; }
const EncodeStats& StreamEncoder::last_stats() const { return p_->stats; }

void StreamEncoder::SetCompactBudget(uint32_t bytes) {
  if (!p_->budgeted) throw std::logic_error("svc::StreamEncoder: SetCompactBudget on an encoder built without compact_budget");
  if (bytes == 0) throw std::invalid_argument("svc::StreamEncoder: a byte budget of 0");
  p_->budget.store(bytes);
}

void StreamEncoder::SetCompactQuality(double psnr_db) {
  if (!p_->quality) throw std::logic_error("svc::StreamEncoder: SetCompactQuality on an encoder built without compact_quality");
  if (!(psnr_db > 0) || !std::isfinite(psnr_db)) throw std::invalid_argument("svc::StreamEncoder: a quality target is a PSNR in dB, positive and finite");
  p_->target.store(DistortionTarget(psnr_db, p_->pw, p_->ph));
}

void StreamEncoder::Encode(const uint8_t* bgr, uint32_t n_frames, const Sink& sink) {
  if (!bgr || n_frames < 2) throw std::runtime_error("svc::StreamEncoder: a clip needs at least two frames");
  const size_t frame = (size_t)p_->c.width * p_->c.height * 3;
  uint32_t i = 0;
  Encode([&]() -> const uint8_t* { return i < n_frames ? bgr + (size_t)(i++) * frame : nullptr; }, n_frames, sink);
}

void StreamEncoder::Encode(const Source& next, uint32_t header_frame_count, const Sink& sink) {
  Impl& m = *p_;
  const StreamEncoderConfig& c = m.c;
  if (!next) throw std::runtime_error("svc::StreamEncoder: no frame source");
  const uint32_t B = c.batch;

  svc_wire_header header{};
  if (c.wire)
    Abi(svc_hip_wire_header(std::max<uint32_t>(header_frame_count, 1), c.width, c.height, m.bw, m.bh, c.levels, m.tw,
                            m.th, &header), "svc_hip_wire_header");

  using Clock = std::chrono::steady_clock;
  auto ms_since = [](Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); };
  EncodeStats st;
  st.copy_threads = m.crew->threads();
  {
    cpu_set_t set;
    st.host_cores = sched_getaffinity(0, sizeof(set), &set) == 0 ? (uint32_t)CPU_COUNT(&set) : 0;
  }

  m.pipe->Begin([&](uint32_t slot) {
    Slot& s = *m.slots[slot];
    if (c.compact) st.d2h_bytes += s.pin_offsets.p[s.encoded];  // the drain moved exactly the used bytes
    if (m.layered) st.d2h_bytes += s.pin_enh_offsets.p[s.encoded];
    if (c.entropy)  // the input is the pack's own output: a flagged frame is a bug, not a stream to pass on
      for (uint32_t i = 0; i < s.encoded; ++i) {
        const uint32_t code = s.pin_entropy_status.p[i] ? s.pin_entropy_status.p[i] : m.layered ? s.pin_enh_status.p[i] : 0u;
        if (code)
          throw std::runtime_error("svc::StreamEncoder: svc_hip_entropy_encode_frames flagged frame " + std::to_string(s.first + i) +
                                   " with status " + std::to_string(code));
      }
    if (m.budgeted)
      for (uint32_t i = 0; i < s.encoded; ++i) st.over_budget_frames += s.pin_choice.p[i] >> 31;
    if (m.quality)  // each frame's D at its group's entry, out of the batch's table
      for (uint32_t i = 0; i < s.encoded; ++i) {
        st.below_quality_frames += (s.pin_choice.p[i] >> 30) & 1u;
        s.pin_distortion.p[i] = s.pin_dist_table.p[(size_t)i * c.compact_ladder.size() + (s.pin_choice.p[i] & 0x3FFFFFFFu)];
      }
    st.encoded_frames += s.encoded;
    const Clock::time_point t0 = Clock::now();
    EncodedBatch b;
    b.header = (c.wire && s.first == 1) ? &header : nullptr;
    b.first_frame = s.first; b.count = s.encoded;
    b.padded_w = m.pw; b.padded_h = m.ph; b.mv_field_w = m.mfw; b.mv_field_h = m.mfh;
    b.mv_xy = s.pin_mv.p; b.global_motion = s.pin_gm.p; b.block_types = s.pin_types.p;
    b.coeffs = c.wire || c.compact ? nullptr : s.pin_coeffs.p;
    if (c.compact) {
      b.compact = s.pin_packed.p; b.compact_offsets = s.pin_offsets.p; b.compact_bytes = s.pin_offsets.p[s.encoded];
      b.compact_choice = m.budgeted || m.quality ? s.pin_choice.p : nullptr;
      b.compact_distortion = m.quality ? s.pin_distortion.p : nullptr;
      b.compact_key = c.delta ? s.pin_key.p : nullptr;
      b.compact_level_counts = c.auto_key ? s.pin_level_counts.p : nullptr;
    }
    if (m.layered) {
      b.enhancement = s.pin_enh.p; b.enhancement_offsets = s.pin_enh_offsets.p; b.enhancement_bytes = s.pin_enh_offsets.p[s.encoded];
    }
    b.records = c.wire ? s.pin_records.p : nullptr;
    b.record_bytes = m.record_bytes;
    sink(b);
    st.sink_ms += ms_since(t0);
  });

  const Slot* prev = nullptr;
  uint32_t first = 1;
  bool ended = false;
  while (!ended) {
    const uint32_t slot = m.pipe->Acquire();
    Slot& s = *m.slots[slot];
    const Clock::time_point t_stage = Clock::now();
    const bool carry = prev != nullptr;
    const uint32_t want = carry ? B : B + 1, off = carry ? 1 : 0;
    // source -> pinned, padding each row out to the padded width
    uint32_t n_new = 0;
    for (; n_new < want; ++n_new) {
      const uint8_t* src = next();
      if (!src) { ended = true; break; }
      uint8_t* dst = s.pin_in.p + (size_t)(off + n_new) * m.frame_bytes;
      m.crew->Copy(dst, (size_t)m.pw * 3, src, (size_t)c.width * 3, (size_t)c.width * 3, c.height);
    }
    const uint32_t encoded = carry ? n_new : (n_new ? n_new - 1 : 0);
    if (encoded == 0) break;  // the clip ended on a batch boundary (or had a single frame): nothing left to encode
    const uint32_t g0 = first - 1;  // clip-wide index of the batch's first pair
    if (m.layered && c.enh_window)  // the frames' windows, asked for here: on the caller's thread, in clip order
      for (uint32_t i = 0; i < encoded; ++i) {
        uint32_t* r = s.pin_window.p + 4 * (size_t)i;
        if (!c.enh_window(first + i, r)) r[0] = r[1] = r[2] = r[3] = 0;  // false: an empty window
      }

    auto h2d = [&](hipStream_t si) -> uint64_t {
      Hip(hipMemcpyAsync(s.bgr.p + (size_t)off * m.frame_bytes, s.pin_in.p + (size_t)off * m.frame_bytes,
                         (size_t)n_new * m.frame_bytes, hipMemcpyHostToDevice, si), "hipMemcpyAsync H2D");
      if (carry)  // the previous batch's last frame is this one's first: behind that batch's H2D, which this stream carried too
        Hip(hipMemcpyAsync(s.bgr.p, prev->bgr.p + (size_t)(prev->frames - 1) * m.frame_bytes, m.frame_bytes,
                           hipMemcpyDeviceToDevice, si), "hipMemcpyAsync D2D");
      if (carry && m.temporal)  // and the frame the batch's first encoded frame refers to, `temporal_period` frames before it, the same way
        Hip(hipMemcpyAsync(s.before_bgr.p, prev->bgr.p + (size_t)(prev->frames - c.temporal_period) * m.frame_bytes, m.frame_bytes,
                           hipMemcpyDeviceToDevice, si), "hipMemcpyAsync D2D (temporal reference)");
      FillRansacDraws(s.pin_samples.p, g0, encoded, m.iters, c.ransac.subset_sz, m.blocks, c.seed);
      Hip(hipMemcpyAsync(s.samples.p, s.pin_samples.p, (size_t)encoded * m.iters * c.ransac.subset_sz * sizeof(uint32_t),
                         hipMemcpyHostToDevice, si), "hipMemcpyAsync samples");
      if (m.layered && c.enh_window)
        Hip(hipMemcpyAsync(s.window.p, s.pin_window.p, (size_t)encoded * 4 * sizeof(uint32_t), hipMemcpyHostToDevice, si),
            "hipMemcpyAsync windows");
      if (c.delta) {  // the key flags: a function of the clip index alone, so the stream does not depend on how it falls into batches
        // (auto_key: the flags this rule forces; the device adds its own, a function of a frame and the frame before alone)
        uint32_t* flags = c.auto_key ? s.pin_forced.p : s.pin_key.p;
        for (uint32_t i = 0; i < encoded; ++i) {
          const uint32_t f = first + i;
          flags[i] = (f == 1 || (c.key_interval != 0 && (f - 1) % c.key_interval == 0)) ? 1u : 0u;
        }
        Hip(hipMemcpyAsync(c.auto_key ? s.forced.p : s.key.p, flags, (size_t)encoded * sizeof(uint32_t), hipMemcpyHostToDevice, si),
            "hipMemcpyAsync key flags");
      }
      if (m.budgeted) {  // the budget as it stands now, for every frame of this batch (SetCompactBudget's rule)
        const uint32_t bytes = m.budget.load();
        std::fill(s.pin_budget.p, s.pin_budget.p + encoded, bytes);
        Hip(hipMemcpyAsync(s.budget.p, s.pin_budget.p, (size_t)encoded * sizeof(uint32_t), hipMemcpyHostToDevice, si),
            "hipMemcpyAsync budget");
      }
      if (m.quality) {  // the target as it stands now, for every frame of this batch (SetCompactQuality's rule)
        const uint64_t d = m.target.load();
        std::fill(s.pin_target.p, s.pin_target.p + encoded, d);
        Hip(hipMemcpyAsync(s.target.p, s.pin_target.p, (size_t)encoded * sizeof(uint64_t), hipMemcpyHostToDevice, si),
            "hipMemcpyAsync target");
      }
      st.staging_ms += ms_since(t_stage);
      return (uint64_t)n_new * m.frame_bytes;
    };
    // always B pairs (a short last batch re-encodes stale frames past its end and drops them)
    auto kernels = [&](hipStream_t sk) {
      Abi(svc_hip_luma_pyramid_frames(s.bgr.p, m.frame_bytes, B + 1, m.pw, m.ph, c.levels, s.pyr.p, m.pyr_stride, sk),
          "svc_hip_luma_pyramid_frames");
      Abi(svc_hip_hbma_pairs(s.pyr.p, s.pyr.p + m.pyr_stride, m.pyr_stride, B, c.levels, m.pw, m.ph, c.search_range,
                             m.bw, m.bh, s.mv.p, s.mad.p, SVC_HBMA_AUTO, sk), "svc_hip_hbma_pairs");
      Hip(hipMemsetAsync(s.gm.p, 0, (size_t)B * 2 * sizeof(float), sk), "hipMemsetAsync");
      Abi(svc_hip_ransac_frames(s.mv.p, m.blocks, B, c.ransac, s.samples.p, m.iters,
                                s.gm.p, s.rmse.p, s.mask.p, s.count.p, sk), "svc_hip_ransac_frames");
      Abi(svc_hip_segment_frames(s.mask.p, s.mv.p, m.mfw, m.mfh, B, m.bw, m.bh, c.segment,
                                 c.seed * 1000003ull + g0, s.seg_ws.p, m.seg_ws_bytes, s.types.p, sk),
          "svc_hip_segment_frames");
      const uint8_t* enc_bgr = s.bgr.p + m.frame_bytes;  // encoded frame of pair p is source frame p + 1
      if (c.wire && m.fused_records) {
        Abi(svc_hip_dct_records_frames(enc_bgr, m.frame_bytes, B, m.pw, m.ph, m.tw, s.types.p, m.bw, m.bh,
                                       0, 0, c.reference_stream ? c.height : m.ph, s.records.p, m.record_bytes, sk),  // raw: see the header
            "svc_hip_dct_records_frames");
      } else if (c.wire) {  // the reference encoder's stream on a padded width, or non-square tiles: planes, then the serialiser with the reference's own arguments
        Abi(svc_hip_dct_frames(enc_bgr, m.frame_bytes, B, m.pw, m.ph, m.tw, m.th, s.coeffs.p, sk), "svc_hip_dct_frames");
        const uint32_t sw = c.reference_stream ? c.width : m.pw, sh = c.reference_stream ? c.height : m.ph;
        Abi(svc_hip_serialize_frames(s.coeffs.p, m.plane_elems, B, s.types.p, sw, sh, m.tw, m.th, m.mfw, m.mfh,
                                     m.bw, m.bh, s.records.p, m.record_bytes, sk), "svc_hip_serialize_frames");
      } else if (m.quality) {  // every batch starts at a key frame and holds whole groups: no frame before, nothing carried
        Abi(svc_hip_dct_pack_delta_quality_frames(enc_bgr, m.frame_bytes, encoded, m.pw, m.ph, m.tw, s.types.p, m.bw, m.bh, c.compact_ladder.data(),
                                                  (uint32_t)c.compact_ladder.size(), s.key.p, s.target.p, m.budgeted ? s.budget.p : nullptr,
                                                  s.pack_ws.p, m.pack_ws_bytes, s.packed.p, m.packed_bytes, s.offsets.p, s.choice.p, nullptr,
                                                  s.dist_table.p, sk),
            "svc_hip_dct_pack_delta_quality_frames");
        if (c.entropy)
          Abi(svc_hip_entropy_encode_frames(s.packed.p, m.packed_bytes, s.offsets.p, encoded, m.pw, m.ph, m.tw, m.th, m.bw, m.bh,
                                            s.entropy_ws.p, m.entropy_ws_bytes, s.coded.p, m.coded_bytes, s.coded_offsets.p,
                                            s.entropy_status.p, sk),
              "svc_hip_entropy_encode_frames");
      } else if (m.group_budget) {  // every batch starts at a key frame and holds whole groups: no frame before, nothing carried
        Abi(svc_hip_dct_pack_delta_budget_frames(enc_bgr, m.frame_bytes, encoded, m.pw, m.ph, m.tw, s.types.p, m.bw, m.bh, c.compact_ladder.data(),
                                                 (uint32_t)c.compact_ladder.size(), s.key.p, s.budget.p, s.pack_ws.p, m.pack_ws_bytes, s.packed.p,
                                                 m.packed_bytes, s.offsets.p, s.choice.p, nullptr, sk),
            "svc_hip_dct_pack_delta_budget_frames");
      } else if (m.budgeted) {  // raw planes; the pack picks each frame's steps from its budget
        Abi(svc_hip_dct_frames(enc_bgr, m.frame_bytes, B, m.pw, m.ph, m.tw, m.th, s.coeffs.p, sk), "svc_hip_dct_frames");
        Abi(svc_hip_pack_levels_budget_frames(s.coeffs.p, s.types.p, encoded, m.pw, m.ph, m.tw, m.th, m.bw, m.bh, c.compact_ladder.data(),
                                              (uint32_t)c.compact_ladder.size(), s.budget.p, s.pack_ws.p, m.pack_ws_bytes, s.packed.p,
                                              m.packed_bytes, s.offsets.p, s.choice.p, sk),
            "svc_hip_pack_levels_budget_frames");
      } else if (c.delta) {
        // The frame before this batch's first encoded frame: its pixels are the slot's frame 0 (the previous batch's last frame, copied on
        // the device), its types the previous slot's last encoded row.  That buffer is written by the previous batch's segmentation and
        // next by the batch that takes the slot again, depth - 1 >= 2 batches on -- both on this one stream (batch_pipe.hpp), so the
        // read below lies between them.  The first batch of an Encode() has no frame before: its first frame is a key frame.
        const uint32_t* prev_types = carry ? prev->types.p + (size_t)(prev->encoded - 1) * m.blocks : nullptr;
        if (m.temporal) {
          // The stream index of the encoded frame with clip index f is f - 1, and every batch but the last holds a multiple of the period,
          // so frame i of the batch has an index that is i modulo the period.  The frame at index -period is encoded frame B - period of
          // the batch before: its pixels were copied into this slot behind that batch's H2D (above), its types are that slot's row
          // B - period, read between the two writes named above.  Nothing comes back to the host for it: the stream does not depend on
          // how the clip falls into batches, nor on the depth.
          const uint32_t* before_types = carry ? prev->types.p + (size_t)(prev->encoded - c.temporal_period) * m.blocks : nullptr;
          Abi(svc_hip_dct_pack_delta_temporal_frames(enc_bgr, m.frame_bytes, encoded, m.pw, m.ph, m.tw, s.types.p, m.bw, m.bh, c.fg_step,
                                                     c.bg_step, carry ? s.before_bgr.p : nullptr, before_types, s.key.p, s.pack_ws.p,
                                                     m.pack_ws_bytes, s.packed.p, m.packed_bytes, s.offsets.p, sk, c.temporal_period),
              "svc_hip_dct_pack_delta_temporal_frames");
        } else if (c.auto_key)
          Abi(svc_hip_dct_pack_delta_auto_frames(enc_bgr, m.frame_bytes, encoded, m.pw, m.ph, m.tw, s.types.p, m.bw, m.bh, c.fg_step, c.bg_step,
                                                 carry ? s.bgr.p : nullptr, prev_types, s.forced.p, s.pack_ws.p, m.pack_ws_bytes, s.packed.p,
                                                 m.packed_bytes, s.offsets.p, s.key.p, s.level_counts.p, sk),
              "svc_hip_dct_pack_delta_auto_frames");
        else
          Abi(svc_hip_dct_pack_delta_frames(enc_bgr, m.frame_bytes, encoded, m.pw, m.ph, m.tw, s.types.p, m.bw, m.bh, c.fg_step, c.bg_step,
                                            carry ? s.bgr.p : nullptr, prev_types, s.key.p, s.pack_ws.p, m.pack_ws_bytes, s.packed.p,
                                            m.packed_bytes, s.offsets.p, sk),
              "svc_hip_dct_pack_delta_frames");
        if (c.entropy)
          Abi(svc_hip_entropy_encode_frames(s.packed.p, m.packed_bytes, s.offsets.p, encoded, m.pw, m.ph, m.tw, m.th, m.bw, m.bh,
                                            s.entropy_ws.p, m.entropy_ws_bytes, s.coded.p, m.coded_bytes, s.coded_offsets.p,
                                            s.entropy_status.p, sk),
              "svc_hip_entropy_encode_frames");
      } else if (m.layered) {  // raw planes; both layers quantise them themselves, whatever the geometry
        Abi(svc_hip_dct_frames(enc_bgr, m.frame_bytes, B, m.pw, m.ph, m.tw, m.th, s.coeffs.p, sk), "svc_hip_dct_frames");
        Abi(svc_hip_pack_layers_frames(s.coeffs.p, s.types.p, encoded, m.pw, m.ph, m.tw, m.th, m.bw, m.bh, c.fg_step, c.bg_step, c.enh_step,
                                       c.enh_window ? s.window.p : nullptr, s.pack_ws.p, m.pack_ws_bytes, s.packed.p, m.packed_bytes,
                                       s.offsets.p, s.enh_packed.p, m.packed_bytes, s.enh_offsets.p, sk),
            "svc_hip_pack_layers_frames");
        if (c.entropy) {  // one workspace: the two calls follow each other on this stream
          Abi(svc_hip_entropy_encode_frames(s.packed.p, m.packed_bytes, s.offsets.p, encoded, m.pw, m.ph, m.tw, m.th, m.bw, m.bh,
                                            s.entropy_ws.p, m.entropy_ws_bytes, s.coded.p, m.coded_bytes, s.coded_offsets.p,
                                            s.entropy_status.p, sk),
              "svc_hip_entropy_encode_frames");
          Abi(svc_hip_entropy_encode_frames(s.enh_packed.p, m.packed_bytes, s.enh_offsets.p, encoded, m.pw, m.ph, m.tw, m.th, m.bw, m.bh,
                                            s.entropy_ws.p, m.entropy_ws_bytes, s.enh_coded.p, m.coded_bytes, s.enh_coded_offsets.p,
                                            s.enh_status.p, sk),
              "svc_hip_entropy_encode_frames (enhancement)");
        }
      } else {
        Abi(svc_hip_dct_quant_frames(enc_bgr, m.frame_bytes, B, m.pw, m.ph, m.tw, m.th, s.types.p, m.bw,
                                     m.bh, c.fg_step, c.bg_step, s.coeffs.p, sk), "svc_hip_dct_quant_frames");
        if (c.compact)
          Abi(svc_hip_pack_levels_frames(s.coeffs.p, s.types.p, encoded, m.pw, m.ph, m.tw, m.th, m.bw, m.bh, c.fg_step, c.bg_step,
                                         s.pack_ws.p, m.pack_ws_bytes, s.packed.p, m.packed_bytes, s.offsets.p, sk),
              "svc_hip_pack_levels_frames");
        if (c.entropy)
          Abi(svc_hip_entropy_encode_frames(s.packed.p, m.packed_bytes, s.offsets.p, encoded, m.pw, m.ph, m.tw, m.th, m.bw, m.bh,
                                            s.entropy_ws.p, m.entropy_ws_bytes, s.coded.p, m.coded_bytes, s.coded_offsets.p,
                                            s.entropy_status.p, sk),
              "svc_hip_entropy_encode_frames");
      }
    };
    auto d2h = [&](hipStream_t so) -> uint64_t {
      uint64_t bytes = (uint64_t)encoded * ((uint64_t)m.blocks * 12 + 8 + (c.wire ? m.record_bytes : c.compact ? 0 : 3 * m.plane_elems * sizeof(float)));
      if (c.compact) bytes += (uint64_t)(encoded + 1) * sizeof(uint64_t);  // + the stream's used bytes, known at delivery
      if ((m.budgeted && !m.quality) || c.entropy) bytes += (uint64_t)encoded * sizeof(uint32_t);  // the choices, or the coder's statuses
      if (m.layered) {  // the enhancement stream, moved as the base is (its used bytes are added at delivery)
        bytes += (uint64_t)(encoded + 1) * sizeof(uint64_t) + (c.entropy ? (uint64_t)encoded * sizeof(uint32_t) : 0);
        if (c.entropy) {
          Abi(svc_hip_entropy_drain(s.enh_coded.p, s.enh_coded_offsets.p, encoded, m.pw, m.ph, m.tw, m.th, m.bw, m.bh, s.pin_enh.p,
                                    m.coded_bytes, so), "svc_hip_entropy_drain (enhancement)");
          Hip(hipMemcpyAsync(s.pin_enh_status.p, s.enh_status.p, (size_t)encoded * sizeof(uint32_t), hipMemcpyDeviceToHost, so),
              "D2H enhancement entropy status");
        } else {
          Abi(svc_hip_levels_drain(s.enh_packed.p, s.enh_offsets.p, encoded, m.pw, m.ph, m.tw, m.th, m.bw, m.bh, s.pin_enh.p, m.packed_bytes,
                                   so), "svc_hip_levels_drain (enhancement)");
        }
        Hip(hipMemcpyAsync(s.pin_enh_offsets.p, c.entropy ? s.enh_coded_offsets.p : s.enh_offsets.p, (size_t)(encoded + 1) * sizeof(uint64_t),
                           hipMemcpyDeviceToHost, so), "D2H enhancement offsets");
      }
      if (m.quality) {  // the choices and the batch's table of distortions
        const size_t L = c.compact_ladder.size();
        bytes += (uint64_t)encoded * (sizeof(uint32_t) + L * sizeof(uint64_t));
        Hip(hipMemcpyAsync(s.pin_choice.p, s.choice.p, (size_t)encoded * sizeof(uint32_t), hipMemcpyDeviceToHost, so), "D2H choice");
        Hip(hipMemcpyAsync(s.pin_dist_table.p, s.dist_table.p, (size_t)encoded * L * sizeof(uint64_t), hipMemcpyDeviceToHost, so), "D2H distortion");
      }
      if (c.auto_key) {  // the chosen flags and the counts they were chosen by
        bytes += (uint64_t)encoded * 3 * sizeof(uint32_t);
        Hip(hipMemcpyAsync(s.pin_key.p, s.key.p, (size_t)encoded * sizeof(uint32_t), hipMemcpyDeviceToHost, so), "D2H key flags");
        Hip(hipMemcpyAsync(s.pin_level_counts.p, s.level_counts.p, (size_t)encoded * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, so),
            "D2H level counts");
      }
      Hip(hipMemcpyAsync(s.pin_mv.p, s.mv.p, (size_t)encoded * m.blocks * 2 * sizeof(float), hipMemcpyDeviceToHost, so), "D2H mv");
      Hip(hipMemcpyAsync(s.pin_types.p, s.types.p, (size_t)encoded * m.blocks * sizeof(uint32_t), hipMemcpyDeviceToHost, so), "D2H types");
      Hip(hipMemcpyAsync(s.pin_gm.p, s.gm.p, (size_t)encoded * 2 * sizeof(float), hipMemcpyDeviceToHost, so), "D2H gm");
      if (c.wire)
        Hip(hipMemcpyAsync(s.pin_records.p, s.records.p, (size_t)encoded * m.record_bytes, hipMemcpyDeviceToHost, so), "D2H records");
      else if (c.entropy) {  // the coded frames, drained the same way, their offsets and the coder's statuses
        Abi(svc_hip_entropy_drain(s.coded.p, s.coded_offsets.p, encoded, m.pw, m.ph, m.tw, m.th, m.bw, m.bh, s.pin_packed.p, m.coded_bytes,
                                  so), "svc_hip_entropy_drain");
        Hip(hipMemcpyAsync(s.pin_offsets.p, s.coded_offsets.p, (size_t)(encoded + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, so),
            "D2H offsets");
        Hip(hipMemcpyAsync(s.pin_entropy_status.p, s.entropy_status.p, (size_t)encoded * sizeof(uint32_t), hipMemcpyDeviceToHost, so),
            "D2H entropy status");
      } else if (c.compact) {  // the used bytes only: the count is on the device, the drain kernel reads it there
        Abi(svc_hip_levels_drain(s.packed.p, s.offsets.p, encoded, m.pw, m.ph, m.tw, m.th, m.bw, m.bh, s.pin_packed.p, m.packed_bytes,
                                 so), "svc_hip_levels_drain");
        Hip(hipMemcpyAsync(s.pin_offsets.p, s.offsets.p, (size_t)(encoded + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, so),
            "D2H offsets");
        if (m.budgeted && !m.quality)
          Hip(hipMemcpyAsync(s.pin_choice.p, s.choice.p, (size_t)encoded * sizeof(uint32_t), hipMemcpyDeviceToHost, so), "D2H choice");
      } else
        Hip(hipMemcpyAsync(s.pin_coeffs.p, s.coeffs.p, (size_t)encoded * 3 * m.plane_elems * sizeof(float), hipMemcpyDeviceToHost, so), "D2H coeffs");
      return bytes;
    };
    s.frames = off + n_new; s.encoded = encoded; s.first = first;
    m.pipe->Submit(slot, h2d, kernels, d2h);
    prev = &s; first += encoded;
  }
  const BatchPipe::Totals& t = m.pipe->Finish();
  st.batches = t.batches; st.wall_ms = t.wall_ms;
  st.slot_wait_ms = t.slot_wait_ms; st.deliver_wait_ms = t.deliver_wait_ms;
  st.h2d_ms = t.h2d_ms; st.kernels_ms = t.kernels_ms; st.d2h_ms = t.d2h_ms;
  st.h2d_bytes = t.h2d_bytes; st.d2h_bytes += t.d2h_bytes;
  m.stats = st;
}

}  // namespace svc
