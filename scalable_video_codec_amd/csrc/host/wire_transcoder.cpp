// wire_transcoder.cpp -- include/svc/wire_transcoder.hpp: buffers and the batch schedule of batch_pipe.hpp around the two stream-to-stream
// device calls.  No arithmetic lives here: how a wire stream is read, the transcode, the entropy coder and the drains are calls into
// the C ABI.
#include "svc/wire_transcoder.hpp"

#include "../stream_format.hpp"
#include "batch_pipe.hpp"
#include "copy_crew.hpp"
#include "stage_frames.hpp"

#include <algorithm>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

namespace svc {
namespace {

using namespace host;

constexpr Who kWho{"svc::WireTranscoder"};
void Hip(hipError_t e, const char* what) { kWho.Hip(e, what); }
void Abi(int rc, const char* what) { kWho.Abi(rc, what); }

struct Slot {
  // ToCompact: records in, the batch's frames (SVCQ or SVCE) out through a drain
  // ToWire: staged frames and their offsets in, records out
  PinBuf<uint8_t> pin_in, pin_out;
  DevBuf<uint8_t> in, out;
  PinBuf<uint64_t> pin_off;
  DevBuf<uint64_t> off;
  PinBuf<uint32_t> pin_status, pin_estatus;
  DevBuf<uint32_t> status, estatus;  // estatus: the entropy coder's codes
  uint32_t first = 0, count = 0;
};

}  // namespace

struct WireTranscoder::Impl {
  WireTranscoderConfig c;
  // what the buffers are sized for (mode 0 = none yet, 1 = ToCompact, 2 = ToWire)
  uint32_t mode = 0, pw = 0, ph = 0, b = 0, mbw = 0, mbh = 0, emit_h = 0;
  bool svce = false;
  uint64_t frame_bytes = 0, q_bytes = 0, out_bytes = 0, ws_bytes = 0, ews_bytes = 0;
  DevBuf<uint8_t> ws, ews, q;  // the kernels' stream only, one for all slots: workspaces, and the SVCQ frames beside SVCE ones
  DevBuf<uint64_t> qoff;
  std::vector<std::unique_ptr<Slot>> slots;
  CopyCrew crew{3};
  std::unique_ptr<BatchPipe> pipe;  // (after the buffers: its streams synchronise before those go)
  TranscodeStats stats;

  void Size(uint32_t want_mode, uint32_t w, uint32_t h, uint32_t block, uint32_t mw, uint32_t mh, uint32_t emit, bool entropy) {
    if (mode == want_mode && w == pw && h == ph && block == b && mw == mbw && mh == mbh && emit == emit_h && entropy == svce) return;
    pipe->SyncStreams();
    mode = 0;  // (until every buffer below is there)
    const uint32_t B = c.wire_batch;
    const uint64_t fbytes = svc_hip_serialized_frame_bytes(w, emit, block, block);
    const uint64_t qb = svc_hip_levels_max_bytes(B, w, h, block, block, mw, mh);
    const uint64_t need_ws = want_mode == 1 ? svc_hip_records_pack_levels_workspace_bytes(B, w, h, block, mw, mh)
                                            : svc_hip_levels_records_workspace_bytes(B, w, h, block, block);
    if (!qb || !need_ws) Abi(SVC_ERR_UNSUPPORTED, "no transcoder for this geometry");
    uint64_t eb = 0, ewb = 0;
    if (entropy) {
      eb = svc_hip_entropy_max_bytes(B, w, h, block, block, mw, mh);
      ewb = svc_hip_entropy_workspace_bytes(B, w, h, block, block, mw, mh);
      if (!eb || !ewb) Abi(SVC_ERR_UNSUPPORTED, "no entropy coder for this geometry");
      ews.Alloc(kWho, ewb);
      q.Alloc(kWho, qb); qoff.Alloc(kWho, B + 1);
    }
    ws.Alloc(kWho, need_ws);
    const uint64_t ob = want_mode == 1 ? (entropy ? eb : qb) : B * fbytes;
    for (auto& s : slots) {
      s->out.Alloc(kWho, ob); s->pin_out.Alloc(kWho, ob);
      if (want_mode == 1) { s->in.Alloc(kWho, B * fbytes); s->pin_in.Alloc(kWho, B * fbytes); }
    }
    pw = w; ph = h; b = block; mbw = mw; mbh = mh; emit_h = emit; svce = entropy;
    frame_bytes = fbytes; q_bytes = qb; out_bytes = ob; ws_bytes = need_ws; ews_bytes = ewb;
    mode = want_mode;
  }

  void Finish(TranscodeStats& st) {
    const BatchPipe::Totals& t = pipe->Finish();
    st.batches = t.batches; st.wall_ms = t.wall_ms;
    st.h2d_ms = t.h2d_ms; st.kernels_ms = t.kernels_ms; st.d2h_ms = t.d2h_ms;
    st.h2d_bytes = t.h2d_bytes; st.d2h_bytes += t.d2h_bytes;
    stats = st;
  }
};

WireTranscoder::WireTranscoder(const WireTranscoderConfig& config) : p_(new Impl) {
  Impl& m = *p_;
  m.c = config;
  const WireTranscoderConfig& c = m.c;
  if (c.wire_batch == 0 || c.depth < 3 || !c.fg_step || !c.bg_step || (c.mv_block_w == 0) != (c.mv_block_h == 0))
    throw std::runtime_error("svc::WireTranscoder: invalid configuration");
  m.pipe.reset(new BatchPipe(kWho, c.depth));
  const size_t B = c.wire_batch;
  for (uint32_t i = 0; i < c.depth; ++i) {
    std::unique_ptr<Slot> s(new Slot);
    s->pin_off.Alloc(kWho, B + 1); s->off.Alloc(kWho, B + 1);
    s->pin_status.Alloc(kWho, B); s->status.Alloc(kWho, B);
    s->pin_estatus.Alloc(kWho, B); s->estatus.Alloc(kWho, B);
    m.slots.push_back(std::move(s));
  }
}

WireTranscoder::~WireTranscoder() = default;
const TranscodeStats& WireTranscoder::last_stats() const { return p_->stats; }

void WireTranscoder::ToCompact(const uint8_t* stream, uint64_t bytes, const CompactSink& sink) {
  Impl& m = *p_;
  const WireTranscoderConfig& c = m.c;
  if (!stream || bytes < sizeof(svc_wire_header)) throw std::runtime_error("svc::WireTranscoder: a wire stream opens with a 32-byte header");
  svc_wire_header hdr;
  std::memcpy(&hdr, stream, sizeof(hdr));
  uint32_t emit_h = 0;
  uint64_t fbytes = 0;
  Abi(svc_hip_wire_layout(&hdr, bytes, &emit_h, &fbytes), "svc_hip_wire_layout");
  const uint32_t n_frames = hdr.frame_count;
  if (n_frames == 0) { m.stats = TranscodeStats{}; return; }
  const uint32_t w = hdr.frame_w + hdr.frame_excess_w, h = hdr.frame_h + hdr.frame_excess_h, block = hdr.transform_block_w;
  const uint32_t mw = c.mv_block_w ? c.mv_block_w : block, mh = c.mv_block_h ? c.mv_block_h : block;
  // the call's own checks, without a batch: a geometry or a step it refuses is thrown here with its message
  Abi(svc_hip_records_pack_levels_frames(nullptr, fbytes, 0, w, h, block, emit_h, mw, mh, c.fg_step, c.bg_step, nullptr, 0, nullptr, 0, nullptr,
                                         nullptr, nullptr),
      "svc_hip_records_pack_levels_frames");
  m.Size(1, w, h, block, mw, mh, emit_h, c.entropy);
  const uint8_t* records = stream + sizeof(hdr);
  const uint32_t B = c.wire_batch;

  TranscodeStats st;
  m.pipe->Begin([&](uint32_t slot) {
    Slot& s = *m.slots[slot];
    st.frames += s.count;
    st.d2h_bytes += s.pin_off.p[s.count];  // the drain moved exactly the used bytes
    if (m.svce)  // the coder's input is the pack's own output: a flagged frame is a bug, not a stream to pass on
      for (uint32_t i = 0; i < s.count; ++i)
        if (s.pin_estatus.p[i])
          throw std::runtime_error("svc::WireTranscoder: svc_hip_entropy_encode_frames refused frame " + std::to_string(s.first + i) +
                                   " (status " + std::to_string(s.pin_estatus.p[i]) + ")");
    CompactBatch o;
    o.first_frame = s.first; o.count = s.count;
    o.frame_w = m.pw; o.frame_h = m.ph; o.block = m.b; o.mv_block_w = m.mbw; o.mv_block_h = m.mbh;
    o.entropy = m.svce;
    o.frames = s.pin_out.p; o.offsets = s.pin_off.p; o.status = s.pin_status.p;
    sink(o);
  });
  for (uint32_t first = 0; first < n_frames;) {
    const uint32_t cnt = std::min(B, n_frames - first);
    const uint32_t slot = m.pipe->Acquire();
    Slot& s = *m.slots[slot];
    const uint64_t batch_bytes = (uint64_t)cnt * fbytes;  // whole frames: the stream's length was checked by svc_hip_wire_layout
    m.crew.Copy(s.pin_in.p, records + (uint64_t)first * fbytes, batch_bytes);
    s.first = first; s.count = cnt;
    m.pipe->Submit(
        slot,
        [&](hipStream_t si) -> uint64_t {
          Hip(hipMemcpyAsync(s.in.p, s.pin_in.p, batch_bytes, hipMemcpyHostToDevice, si), "hipMemcpyAsync H2D");
          return batch_bytes;
        },
        [&](hipStream_t sk) {
          uint8_t* packed = m.svce ? m.q.p : s.out.p;
          uint64_t* poff = m.svce ? m.qoff.p : s.off.p;
          Abi(svc_hip_records_pack_levels_frames(s.in.p, fbytes, cnt, m.pw, m.ph, m.b, m.emit_h, m.mbw, m.mbh, c.fg_step, c.bg_step, m.ws.p,
                                                 m.ws_bytes, packed, m.q_bytes, poff, s.status.p, sk),
              "svc_hip_records_pack_levels_frames");
          if (m.svce)
            Abi(svc_hip_entropy_encode_frames(m.q.p, m.q_bytes, m.qoff.p, cnt, m.pw, m.ph, m.b, m.b, m.mbw, m.mbh, m.ews.p, m.ews_bytes, s.out.p,
                                              m.out_bytes, s.off.p, s.estatus.p, sk),
                "svc_hip_entropy_encode_frames");
        },
        [&](hipStream_t so) -> uint64_t {
          if (m.svce) {
            Abi(svc_hip_entropy_drain(s.out.p, s.off.p, cnt, m.pw, m.ph, m.b, m.b, m.mbw, m.mbh, s.pin_out.p, m.out_bytes, so),
                "svc_hip_entropy_drain");
            Hip(hipMemcpyAsync(s.pin_estatus.p, s.estatus.p, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost, so), "hipMemcpyAsync D2H status");
          } else {
            Abi(svc_hip_levels_drain(s.out.p, s.off.p, cnt, m.pw, m.ph, m.b, m.b, m.mbw, m.mbh, s.pin_out.p, m.out_bytes, so),
                "svc_hip_levels_drain");
          }
          Hip(hipMemcpyAsync(s.pin_off.p, s.off.p, (cnt + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, so), "hipMemcpyAsync D2H offsets");
          Hip(hipMemcpyAsync(s.pin_status.p, s.status.p, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost, so), "hipMemcpyAsync D2H status");
          return (cnt + 1) * sizeof(uint64_t) + (m.svce ? 2 : 1) * cnt * sizeof(uint32_t);  // (the drained bytes are added at delivery)
        });
    first += cnt;
  }
  m.Finish(st);
}

void WireTranscoder::ToWire(const uint8_t* compact, const uint64_t* offsets, uint32_t n_frames, uint32_t emit_frame_h, const WireSink& sink) {
  Impl& m = *p_;
  const WireTranscoderConfig& c = m.c;
  if (n_frames == 0) { m.stats = TranscodeStats{}; return; }
  if (!compact || !offsets) throw std::runtime_error("svc::WireTranscoder: null stream");
  const uint64_t total = offsets[n_frames];  // the stream's bytes, from offsets[0] on
  if (offsets[0] % 16 || offsets[0] > total || total - offsets[0] < kHeaderBytes || offsets[1] < offsets[0] + kHeaderBytes)
    throw std::runtime_error("svc::WireTranscoder: the first frame's header is out of range");
  uint32_t hdr[kHeaderWords];
  std::memcpy(hdr, compact + offsets[0], sizeof(hdr));
  if ((hdr[kHMagic] != kMagicQ && hdr[kHMagic] != kMagicE) || hdr[kHVersion] != kVersion)
    throw std::runtime_error("svc::WireTranscoder: the stream does not open with an SVCQ v1 or SVCE v1 header");
  const uint32_t w = hdr[kHWidth], h = hdr[kHHeight], emit = emit_frame_h ? emit_frame_h : h;
  // the call's own checks, without a batch (the square tile and emit_frame_h among them)
  Abi(svc_hip_levels_records_frames(nullptr, 0, nullptr, 0, w, h, hdr[kHTileW], hdr[kHTileH], hdr[kHMvW], hdr[kHMvH], emit, nullptr, 0, nullptr,
                                    svc_hip_serialized_frame_bytes(w, emit, hdr[kHTileW], hdr[kHTileH]), nullptr, nullptr),
      "svc_hip_levels_records_frames");
  m.Size(2, w, h, hdr[kHTileW], hdr[kHMvW], hdr[kHMvH], emit, hdr[kHMagic] == kMagicE);
  const uint32_t B = c.wire_batch;

  TranscodeStats st;
  m.pipe->Begin([&](uint32_t slot) {
    Slot& s = *m.slots[slot];
    st.frames += s.count;
    if (m.svce)  // a frame the entropy decoder refused is zeros to the SVCQ reader (status 2): the decoder's code is reported instead
      for (uint32_t i = 0; i < s.count; ++i)
        if (s.pin_estatus.p[i]) s.pin_status.p[i] = s.pin_estatus.p[i];
    WireBatch o;
    o.first_frame = s.first; o.count = s.count;
    o.frame_w = m.pw; o.frame_h = m.ph; o.block = m.b; o.emit_frame_h = m.emit_h; o.frame_bytes = m.frame_bytes;
    o.records = s.pin_out.p; o.status = s.pin_status.p;
    sink(o);
  });
  for (uint32_t first = 0; first < n_frames;) {
    const uint32_t cnt = std::min(B, n_frames - first);
    const uint32_t slot = m.pipe->Acquire();
    Slot& s = *m.slots[slot];
    const uint64_t bytes = StageFrames(kWho, m.crew, compact, offsets, total, first, cnt, s.pin_in, s.in, s.pin_off.p);
    s.first = first; s.count = cnt;
    m.pipe->Submit(
        slot,
        [&](hipStream_t si) -> uint64_t {
          Hip(hipMemcpyAsync(s.in.p, s.pin_in.p, bytes, hipMemcpyHostToDevice, si), "hipMemcpyAsync H2D");
          Hip(hipMemcpyAsync(s.off.p, s.pin_off.p, (cnt + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, si), "hipMemcpyAsync H2D offsets");
          return bytes + (cnt + 1) * sizeof(uint64_t);
        },
        [&](hipStream_t sk) {
          const uint8_t* qin = s.in.p;
          const uint64_t* qoff = s.off.p;
          uint64_t qbytes = bytes;
          if (m.svce) {  // SVCE -> SVCQ in device scratch, then the SVCQ call unchanged
            Abi(svc_hip_entropy_decode_frames(s.in.p, bytes, s.off.p, cnt, m.pw, m.ph, m.b, m.b, m.mbw, m.mbh, m.ews.p, m.ews_bytes, m.q.p,
                                              m.q_bytes, m.qoff.p, s.estatus.p, sk),
                "svc_hip_entropy_decode_frames");
            qin = m.q.p; qoff = m.qoff.p; qbytes = m.q_bytes;
          }
          Abi(svc_hip_levels_records_frames(qin, qbytes, qoff, cnt, m.pw, m.ph, m.b, m.b, m.mbw, m.mbh, m.emit_h, m.ws.p, m.ws_bytes, s.out.p,
                                            m.frame_bytes, s.status.p, sk),
              "svc_hip_levels_records_frames");
        },
        [&](hipStream_t so) -> uint64_t {
          Hip(hipMemcpyAsync(s.pin_out.p, s.out.p, cnt * m.frame_bytes, hipMemcpyDeviceToHost, so), "hipMemcpyAsync D2H records");
          Hip(hipMemcpyAsync(s.pin_status.p, s.status.p, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost, so), "hipMemcpyAsync D2H status");
          if (m.svce)
            Hip(hipMemcpyAsync(s.pin_estatus.p, s.estatus.p, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost, so), "hipMemcpyAsync D2H status");
          return cnt * (m.frame_bytes + (m.svce ? 2 : 1) * sizeof(uint32_t));
        });
    first += cnt;
  }
  m.Finish(st);
}

}  // namespace svc
