// stream_decoder.cpp -- include/svc/stream_decoder.hpp: buffers and the batch schedule of batch_pipe.hpp, as stream_encoder.cpp, run
// the other way.  No arithmetic of the hot path lives here; the gaze rule and the decode are calls into the C ABI.
#include "svc/stream_decoder.hpp"

#include "svc_hip_temporal_decode.h"

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

constexpr Who kWho{"svc::StreamDecoder"};
void Hip(hipError_t e, const char* what) { kWho.Hip(e, what); }
void Abi(int rc, const char* what) { kWho.Abi(rc, what); }

struct Slot {
  PinBuf<uint8_t> pin_in, pin_disp;
  PinBuf<uint64_t> pin_off;
  PinBuf<uint32_t> pin_gaze, pin_status;
  DevBuf<uint8_t> in, disp;
  DevBuf<uint64_t> off;
  DevBuf<uint32_t> gaze, status, estatus;  // estatus: svc_hip_entropy_decode_frames's codes (SVCE)
  PinBuf<uint32_t> pin_estatus;
  // DecodeLayers: the enhancement stream's batch beside the base's, and the entropy decoder's codes for it
  PinBuf<uint8_t> pin_enh;
  DevBuf<uint8_t> enh;
  PinBuf<uint64_t> pin_enh_off;
  DevBuf<uint64_t> enh_off;
  DevBuf<uint32_t> enh_estatus;
  PinBuf<uint32_t> pin_enh_estatus;
  // DecodeDelta: the batch's key flags
  PinBuf<uint32_t> pin_key;
  DevBuf<uint32_t> key;
  uint32_t first = 0, count = 0;
};

// the first frame's header of a stream of n_frames >= 1 frames, which must open an SVCQ v1 or SVCE v1 frame
void FirstHeader(const uint8_t* stream, const uint64_t* offsets, uint32_t n_frames, const char* which, uint32_t hdr[kHeaderWords]) {
  const uint64_t total = offsets[n_frames];  // the stream's bytes, from offsets[0] on
  if (offsets[0] % 16 || offsets[0] > total || total - offsets[0] < kHeaderBytes || offsets[1] < offsets[0] + kHeaderBytes)
    throw std::runtime_error(std::string("svc::StreamDecoder: the ") + which + "first frame's header is out of range");
  std::memcpy(hdr, stream + offsets[0], kHeaderWords * sizeof(uint32_t));
  if ((hdr[kHMagic] != kMagicQ && hdr[kHMagic] != kMagicE) || hdr[kHVersion] != kVersion)
    throw std::runtime_error(std::string("svc::StreamDecoder: the ") + which + "stream does not open with an SVCQ v1 or SVCE v1 header");
}

// A batch that has landed goes to the sink.  svce_status: a frame the entropy decoder refused is zeros to the SVCQ decoder (status 2),
// so the entropy decoder's code is reported instead.
// enh_svce_status (DecodeLayers): likewise for the enhancement frame, as kStEnhancement | its code, where the base frame's is 0.
void Deliver(Slot& s, uint32_t dw, uint32_t dh, bool svce_status, bool enh_svce_status, DecodeStats& st, const StreamDecoder::Sink& sink) {
  st.frames += s.count;
  for (uint32_t i = 0; i < s.count; ++i) {
    if (svce_status && s.pin_estatus.p[i]) s.pin_status.p[i] = s.pin_estatus.p[i];
    else if (enh_svce_status && s.pin_enh_estatus.p[i]) s.pin_status.p[i] = kStEnhancement | s.pin_enh_estatus.p[i];
  }
  DecodedBatch b;
  b.first_frame = s.first; b.count = s.count; b.width = dw; b.height = dh;
  b.bgr = s.pin_disp.p; b.status = s.pin_status.p;
  sink(b);
}

}  // namespace

struct StreamDecoder::Impl {
  StreamDecoderConfig c;
  // geometry the buffers are sized for (0 = none yet)
  uint32_t pw = 0, ph = 0, bw = 0, bh = 0, mbw = 0, mbh = 0, dw = 0, dh = 0;
  uint64_t disp_bytes = 0, ws_bytes = 0;
  bool wire = false;        // the buffers are sized for DecodeWire
  bool svce = false;        // Decode: the stream is SVCE, decoded to SVCQ in q first
  bool layered = false;     // the buffers are sized for DecodeLayers
  bool enh_svce = false;    // DecodeLayers: the enhancement stream is SVCE, decoded to SVCQ in eq first
  bool delta = false;       // the buffers are sized for DecodeDelta or DecodeDeltaReduced
  uint32_t red = 0;         // the reduce the buffers are sized for (0 = none yet)
  DevBuf<uint8_t> chain[2]; // DecodeDelta: the last reconstructed frame of a batch (DecodeDeltaReduced: its band), the next batch's frame before
  DevBuf<uint64_t> chain_len;     // its length, as the device call writes it ...
  PinBuf<uint64_t> pin_chain_len; // ... and where the host reads it
  uint64_t chain_bytes = 0;
  DevBuf<uint8_t> q, ews;   // SVCE: the batch's SVCQ frames and the coder's workspace (the kernels' stream only)
  DevBuf<uint64_t> qoff;
  DevBuf<uint8_t> eq;       // the same for the enhancement stream (one workspace: the two calls follow each other)
  DevBuf<uint64_t> eqoff;
  uint64_t q_bytes = 0, ews_bytes = 0;
  uint64_t frame_bytes = 0; // DecodeWire: bytes of one frame's records
  DevBuf<float> rec;        // the kernels' stream only: one for all slots
  DevBuf<uint8_t> ws;
  std::vector<std::unique_ptr<Slot>> slots;
  CopyCrew crew{3};
  std::unique_ptr<BatchPipe> pipe;  // (after the buffers: its streams synchronise before those go)
  DecodeStats stats;

  // layers: for DecodeLayers (the workspace of svc_hip_decode_layers_frames, which the reduced call shares; enh_entropy = the enhancement
  // stream is SVCE)
  // chained: for DecodeDelta and DecodeDeltaReduced (the workspace of svc_hip_decode_delta_levels_frames, which the reduced call shares,
  // and the two frames of the chain); reduce: 0 = the configured one, else DecodeDeltaReduced's argument
  void Size(const uint32_t* hdr, bool entropy, bool layers = false, bool enh_entropy = false, bool chained = false, uint32_t reduce = 0) {
    if (!reduce) reduce = c.reduce;
    const uint32_t w = hdr[kHWidth], h = hdr[kHHeight], tw = hdr[kHTileW], th = hdr[kHTileH], mw = hdr[kHMvW], mh = hdr[kHMvH];
    const uint32_t rw = w / reduce, rh = h / reduce;  // the picture the display pass reads
    const uint32_t want_dw = c.display_w ? c.display_w : rw, want_dh = c.display_h ? c.display_h : rh;
    if (!wire && entropy == svce && layers == layered && enh_entropy == enh_svce && chained == delta && reduce == red && w == pw && h == ph && tw == bw && th == bh && mw == mbw && mh == mbh && want_dw == dw && want_dh == dh)
      return;
    pipe->SyncStreams();
    const uint64_t need_ws = chained  ? svc_hip_decode_delta_levels_workspace_bytes(c.batch, w, h, tw, th, mw, mh)
                             : layers ? svc_hip_decode_layers_workspace_bytes(c.batch, w, h, tw, th)
                                      : svc_hip_decode_levels_workspace_bytes(c.batch, w, h, tw, th);
    if (!need_ws) Abi(SVC_ERR_UNSUPPORTED, "no decoder for the first frame's geometry");
    if (want_dw > rw || want_dh > rh)
      throw std::runtime_error(reduce > 1 ? "svc::StreamDecoder: the display size exceeds the padded frame over reduce"
                                          : "svc::StreamDecoder: the display size exceeds the padded frame");
    if (entropy || enh_entropy) {
      q_bytes = svc_hip_levels_max_bytes(c.batch, w, h, tw, th, mw, mh);
      ews_bytes = svc_hip_entropy_workspace_bytes(c.batch, w, h, tw, th, mw, mh);
      if (!q_bytes || !ews_bytes) Abi(SVC_ERR_UNSUPPORTED, "no entropy decoder for the first frame's geometry");
      ews.Alloc(kWho, ews_bytes);
      if (entropy) { q.Alloc(kWho, q_bytes); qoff.Alloc(kWho, c.batch + 1); }
      if (enh_entropy) { eq.Alloc(kWho, q_bytes); eqoff.Alloc(kWho, c.batch + 1); }
    }
    svce = entropy;
    layered = layers;
    enh_svce = enh_entropy;
    delta = chained;
    red = reduce;
    if (chained) {
      chain_bytes = svc_hip_levels_max_bytes(1, w, h, tw, th, mw, mh);
      for (auto& b : chain) b.Alloc(kWho, chain_bytes);
      chain_len.Alloc(kWho, 1); pin_chain_len.Alloc(kWho, 1);
    }
    wire = false;
    pw = w; ph = h; bw = tw; bh = th; mbw = mw; mbh = mh; dw = want_dw; dh = want_dh;
    disp_bytes = (uint64_t)dw * dh * 3;
    ws_bytes = need_ws;
    const size_t B = c.batch;
    rec.Alloc(kWho, B * rw * rh * 3);
    ws.Alloc(kWho, ws_bytes);
    for (auto& s : slots) {
      s->disp.Alloc(kWho, B * disp_bytes); s->pin_disp.Alloc(kWho, B * disp_bytes);
    }
  }

  // DecodeWire: a padded w x h frame of `fbytes` bytes of b x b records, shown at want_dw x want_dh
  void SizeWire(uint32_t w, uint32_t h, uint32_t b, uint64_t fbytes, uint32_t want_dw, uint32_t want_dh) {
    if (wire && w == pw && h == ph && b == bw && fbytes == frame_bytes && want_dw == dw && want_dh == dh) return;
    pipe->SyncStreams();
    if (want_dw > w || want_dh > h) throw std::runtime_error("svc::StreamDecoder: the display size exceeds the padded frame");
    wire = true;
    pw = w; ph = h; bw = bh = b; mbw = mbh = 0; dw = want_dw; dh = want_dh; frame_bytes = fbytes;
    disp_bytes = (uint64_t)dw * dh * 3;
    const size_t B = c.wire_batch;
    rec.Alloc(kWho, B * pw * ph * 3);
    for (auto& s : slots) {
      s->disp.Alloc(kWho, B * disp_bytes); s->pin_disp.Alloc(kWho, B * disp_bytes);
      s->in.Alloc(kWho, B * frame_bytes); s->pin_in.Alloc(kWho, B * frame_bytes);
      std::memset(s->pin_status.p, 0, s->pin_status.n * sizeof(uint32_t));  // the records carry no per-frame status
    }
  }

  // the gaze rectangles of frames first .. first + cnt into the slot's pinned array (no gaze: an empty rectangle)
  void StageGaze(Slot& s, const Gaze& gaze, uint32_t first, uint32_t cnt) {
    for (uint32_t i = 0; i < cnt; ++i) {
      uint32_t x = 0, y = 0, *r = s.pin_gaze.p + 4 * i;
      if (gaze && gaze(first + i, &x, &y))
        Abi(svc_hip_gaze_rect(x, y, c.max_gaze_w, c.max_gaze_h, dw, dh, pw, ph, r), "svc_hip_gaze_rect");
      else
        r[0] = r[1] = r[2] = r[3] = 0;
    }
  }

  void Delta(const uint8_t* stream, const uint64_t* offsets, uint32_t n_frames, const uint32_t* key, uint32_t reduce, uint32_t period, const Gaze& gaze,
             const Sink& sink);

  void Finish(DecodeStats& st) {
    const BatchPipe::Totals& t = pipe->Finish();
    st.batches = t.batches; st.wall_ms = t.wall_ms;
    st.h2d_ms = t.h2d_ms; st.kernels_ms = t.kernels_ms; st.d2h_ms = t.d2h_ms;
    st.h2d_bytes = t.h2d_bytes; st.d2h_bytes = t.d2h_bytes;
    stats = st;
  }
};

StreamDecoder::StreamDecoder(const StreamDecoderConfig& config) : p_(new Impl) {
  Impl& m = *p_;
  m.c = config;
  const StreamDecoderConfig& c = m.c;
  if (c.batch == 0 || c.wire_batch == 0 || c.depth < 3 || !c.fg_step || !c.bg_step || (c.display_w == 0) != (c.display_h == 0) ||
      (c.reduce != 1 && c.reduce != 2 && c.reduce != 4 && c.reduce != 8))
    throw std::runtime_error("svc::StreamDecoder: invalid configuration");
  m.pipe.reset(new BatchPipe(kWho, c.depth));
  const size_t B = std::max(c.batch, c.wire_batch);  // per-frame arrays serve both paths
  for (uint32_t i = 0; i < c.depth; ++i) {
    std::unique_ptr<Slot> s(new Slot);
    s->pin_off.Alloc(kWho, B + 1); s->off.Alloc(kWho, B + 1);
    s->pin_gaze.Alloc(kWho, 4 * B); s->gaze.Alloc(kWho, 4 * B);
    s->pin_status.Alloc(kWho, B); s->status.Alloc(kWho, B);
    s->pin_estatus.Alloc(kWho, B); s->estatus.Alloc(kWho, B);
    s->pin_enh_off.Alloc(kWho, B + 1); s->enh_off.Alloc(kWho, B + 1);
    s->pin_enh_estatus.Alloc(kWho, B); s->enh_estatus.Alloc(kWho, B);
    s->pin_key.Alloc(kWho, B); s->key.Alloc(kWho, B);
    m.slots.push_back(std::move(s));
  }
}

StreamDecoder::~StreamDecoder() = default;
const DecodeStats& StreamDecoder::last_stats() const { return p_->stats; }

void StreamDecoder::Decode(const uint8_t* stream, const uint64_t* offsets, uint32_t n_frames, const Gaze& gaze, const Sink& sink) {
  Impl& m = *p_;
  const StreamDecoderConfig& c = m.c;
  if (n_frames == 0) { m.stats = DecodeStats{}; return; }
  if (!stream || !offsets) throw std::runtime_error("svc::StreamDecoder: null stream");
  const uint64_t total = offsets[n_frames];  // the stream's bytes, from offsets[0] on
  uint32_t hdr[kHeaderWords];
  FirstHeader(stream, offsets, n_frames, "", hdr);
  m.Size(hdr, hdr[kHMagic] == kMagicE);
  const uint32_t B = c.batch;

  DecodeStats st;
  m.pipe->Begin([&](uint32_t slot) { Deliver(*m.slots[slot], m.dw, m.dh, m.svce, false, st, sink); });
  for (uint32_t first = 0; first < n_frames;) {
    const uint32_t cnt = std::min(B, n_frames - first);
    const uint32_t slot = m.pipe->Acquire();
    Slot& s = *m.slots[slot];
    const uint64_t bytes = StageFrames(kWho, m.crew, stream, offsets, total, first, cnt, s.pin_in, s.in, s.pin_off.p);
    m.StageGaze(s, gaze, first, cnt);
    s.first = first; s.count = cnt;
    m.pipe->Submit(
        slot,
        [&](hipStream_t si) -> uint64_t {
          Hip(hipMemcpyAsync(s.in.p, s.pin_in.p, bytes, hipMemcpyHostToDevice, si), "hipMemcpyAsync H2D");
          Hip(hipMemcpyAsync(s.off.p, s.pin_off.p, (cnt + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, si), "hipMemcpyAsync H2D offsets");
          Hip(hipMemcpyAsync(s.gaze.p, s.pin_gaze.p, 4 * cnt * sizeof(uint32_t), hipMemcpyHostToDevice, si), "hipMemcpyAsync H2D gaze");
          return bytes + (cnt + 1) * sizeof(uint64_t) + 4 * cnt * sizeof(uint32_t);
        },
        [&](hipStream_t sk) {
          const uint8_t* qin = s.in.p;
          const uint64_t* qoff = s.off.p;
          uint64_t qbytes = bytes;
          if (m.svce) {  // SVCE -> SVCQ in device scratch, then the SVCQ decoder unchanged
            Abi(svc_hip_entropy_decode_frames(s.in.p, bytes, s.off.p, cnt, m.pw, m.ph, m.bw, m.bh, m.mbw, m.mbh, m.ews.p, m.ews_bytes, m.q.p,
                                              m.q_bytes, m.qoff.p, s.estatus.p, sk),
                "svc_hip_entropy_decode_frames");
            qin = m.q.p; qoff = m.qoff.p; qbytes = m.q_bytes;
          }
          if (c.reduce > 1)
            Abi(svc_hip_decode_levels_reduced_frames(qin, qbytes, qoff, cnt, m.pw, m.ph, m.bw, m.bh, m.mbw, m.mbh, c.fg_step, c.bg_step,
                                                     c.reduce, s.gaze.p, m.ws.p, m.ws_bytes, m.rec.p, s.disp.p, m.dw, m.dh, s.status.p, sk),
                "svc_hip_decode_levels_reduced_frames");
          else
            Abi(svc_hip_decode_levels_frames(qin, qbytes, qoff, cnt, m.pw, m.ph, m.bw, m.bh, m.mbw, m.mbh, c.fg_step, c.bg_step, s.gaze.p,
                                             m.ws.p, m.ws_bytes, m.rec.p, s.disp.p, m.dw, m.dh, s.status.p, sk),
                "svc_hip_decode_levels_frames");
        },
        [&](hipStream_t so) -> uint64_t {
          Hip(hipMemcpyAsync(s.pin_disp.p, s.disp.p, cnt * m.disp_bytes, hipMemcpyDeviceToHost, so), "hipMemcpyAsync D2H display");
          Hip(hipMemcpyAsync(s.pin_status.p, s.status.p, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost, so), "hipMemcpyAsync D2H status");
          if (m.svce)
            Hip(hipMemcpyAsync(s.pin_estatus.p, s.estatus.p, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost, so), "hipMemcpyAsync D2H status");
          return cnt * (m.disp_bytes + (m.svce ? 2 : 1) * sizeof(uint32_t));
        });
    first += cnt;
  }
  m.Finish(st);
}

void StreamDecoder::DecodeLayers(const uint8_t* base, const uint64_t* base_offsets, const uint8_t* enh, const uint64_t* enh_offsets,
                                 uint32_t n_frames, const Gaze& gaze, const Sink& sink) {
  if (!gaze) return Decode(base, base_offsets, n_frames, gaze, sink);  // no tile takes the enhancement: it is not read
  Impl& m = *p_;
  const StreamDecoderConfig& c = m.c;
  if (n_frames == 0) { m.stats = DecodeStats{}; return; }
  if (!base || !base_offsets || !enh || !enh_offsets) throw std::runtime_error("svc::StreamDecoder: null stream");
  const uint64_t total = base_offsets[n_frames], enh_total = enh_offsets[n_frames];
  uint32_t hdr[kHeaderWords], ehdr[kHeaderWords];
  FirstHeader(base, base_offsets, n_frames, "base's ", hdr);
  FirstHeader(enh, enh_offsets, n_frames, "enhancement's ", ehdr);
  for (uint32_t k = kHWidth; k <= kHMvH; ++k)
    if (hdr[k] != ehdr[k]) throw std::runtime_error("svc::StreamDecoder: the enhancement stream's geometry is not the base stream's");
  m.Size(hdr, hdr[kHMagic] == kMagicE, true, ehdr[kHMagic] == kMagicE);
  const uint32_t B = c.batch;

  DecodeStats st;
  m.pipe->Begin([&](uint32_t slot) { Deliver(*m.slots[slot], m.dw, m.dh, m.svce, m.enh_svce, st, sink); });
  for (uint32_t first = 0; first < n_frames;) {
    const uint32_t cnt = std::min(B, n_frames - first);
    const uint32_t slot = m.pipe->Acquire();
    Slot& s = *m.slots[slot];
    const uint64_t bytes = StageFrames(kWho, m.crew, base, base_offsets, total, first, cnt, s.pin_in, s.in, s.pin_off.p);
    const uint64_t ebytes = StageFrames(kWho, m.crew, enh, enh_offsets, enh_total, first, cnt, s.pin_enh, s.enh, s.pin_enh_off.p);
    m.StageGaze(s, gaze, first, cnt);
    s.first = first; s.count = cnt;
    m.pipe->Submit(
        slot,
        [&](hipStream_t si) -> uint64_t {
          Hip(hipMemcpyAsync(s.in.p, s.pin_in.p, bytes, hipMemcpyHostToDevice, si), "hipMemcpyAsync H2D");
          Hip(hipMemcpyAsync(s.enh.p, s.pin_enh.p, ebytes, hipMemcpyHostToDevice, si), "hipMemcpyAsync H2D enhancement");
          Hip(hipMemcpyAsync(s.off.p, s.pin_off.p, (cnt + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, si), "hipMemcpyAsync H2D offsets");
          Hip(hipMemcpyAsync(s.enh_off.p, s.pin_enh_off.p, (cnt + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, si),
              "hipMemcpyAsync H2D enhancement offsets");
          Hip(hipMemcpyAsync(s.gaze.p, s.pin_gaze.p, 4 * cnt * sizeof(uint32_t), hipMemcpyHostToDevice, si), "hipMemcpyAsync H2D gaze");
          return bytes + ebytes + 2 * (cnt + 1) * sizeof(uint64_t) + 4 * cnt * sizeof(uint32_t);
        },
        [&](hipStream_t sk) {
          const uint8_t *qb = s.in.p, *qe = s.enh.p;
          const uint64_t *qboff = s.off.p, *qeoff = s.enh_off.p;
          uint64_t qbbytes = bytes, qebytes = ebytes;
          if (m.svce) {  // SVCE -> SVCQ in device scratch, each stream by its own kind
            Abi(svc_hip_entropy_decode_frames(s.in.p, bytes, s.off.p, cnt, m.pw, m.ph, m.bw, m.bh, m.mbw, m.mbh, m.ews.p, m.ews_bytes, m.q.p,
                                              m.q_bytes, m.qoff.p, s.estatus.p, sk),
                "svc_hip_entropy_decode_frames");
            qb = m.q.p; qboff = m.qoff.p; qbbytes = m.q_bytes;
          }
          if (m.enh_svce) {
            Abi(svc_hip_entropy_decode_frames(s.enh.p, ebytes, s.enh_off.p, cnt, m.pw, m.ph, m.bw, m.bh, m.mbw, m.mbh, m.ews.p, m.ews_bytes,
                                              m.eq.p, m.q_bytes, m.eqoff.p, s.enh_estatus.p, sk),
                "svc_hip_entropy_decode_frames (enhancement)");
            qe = m.eq.p; qeoff = m.eqoff.p; qebytes = m.q_bytes;
          }
          if (c.reduce > 1)
            Abi(svc_hip_decode_layers_reduced_frames(qb, qbbytes, qboff, qe, qebytes, qeoff, cnt, m.pw, m.ph, m.bw, m.bh, m.mbw, m.mbh,
                                                     c.fg_step, c.bg_step, c.reduce, s.gaze.p, m.ws.p, m.ws_bytes, m.rec.p, s.disp.p, m.dw,
                                                     m.dh, s.status.p, sk),
                "svc_hip_decode_layers_reduced_frames");
          else
            Abi(svc_hip_decode_layers_frames(qb, qbbytes, qboff, qe, qebytes, qeoff, cnt, m.pw, m.ph, m.bw, m.bh, m.mbw, m.mbh, c.fg_step,
                                             c.bg_step, s.gaze.p, m.ws.p, m.ws_bytes, m.rec.p, s.disp.p, m.dw, m.dh, s.status.p, sk),
                "svc_hip_decode_layers_frames");
        },
        [&](hipStream_t so) -> uint64_t {
          Hip(hipMemcpyAsync(s.pin_disp.p, s.disp.p, cnt * m.disp_bytes, hipMemcpyDeviceToHost, so), "hipMemcpyAsync D2H display");
          Hip(hipMemcpyAsync(s.pin_status.p, s.status.p, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost, so), "hipMemcpyAsync D2H status");
          if (m.svce)
            Hip(hipMemcpyAsync(s.pin_estatus.p, s.estatus.p, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost, so), "hipMemcpyAsync D2H status");
          if (m.enh_svce)
            Hip(hipMemcpyAsync(s.pin_enh_estatus.p, s.enh_estatus.p, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost, so),
                "hipMemcpyAsync D2H enhancement status");
          return cnt * (m.disp_bytes + (1 + m.svce + m.enh_svce) * sizeof(uint32_t));
        });
    first += cnt;
  }
  m.Finish(st);
}

void StreamDecoder::DecodeDelta(const uint8_t* stream, const uint64_t* offsets, uint32_t n_frames, const uint32_t* key, const Gaze& gaze,
                                const Sink& sink) {
  if (p_->c.reduce != 1) throw std::runtime_error("svc::StreamDecoder: DecodeDelta does not decode at reduced size (reduce must be 1)");
  p_->Delta(stream, offsets, n_frames, key, 1, 1, gaze, sink);
}

void StreamDecoder::DecodeDeltaTemporal(const uint8_t* stream, const uint64_t* offsets, uint32_t n_frames, const uint32_t* key, uint32_t period,
                                        const Gaze& gaze, const Sink& sink) {
  if (period != 1 && period != 2 && period != 4) throw std::runtime_error("svc::StreamDecoder: DecodeDeltaTemporal takes a period of 1, 2 or 4");
  if (p_->c.reduce != 1) throw std::runtime_error("svc::StreamDecoder: DecodeDeltaTemporal does not decode at reduced size (reduce must be 1)");
  if (p_->c.batch % period != 0)
    throw std::runtime_error("svc::StreamDecoder: DecodeDeltaTemporal carries the frame at index -period from batch to batch: config.batch must be a multiple of the period");
  p_->Delta(stream, offsets, n_frames, key, 1, period, gaze, sink);
}

void StreamDecoder::DecodeDeltaReduced(const uint8_t* stream, const uint64_t* offsets, uint32_t n_frames, const uint32_t* key, uint32_t reduce,
                                       const Gaze& gaze, const Sink& sink) {
  if (reduce != 2 && reduce != 4 && reduce != 8) throw std::runtime_error("svc::StreamDecoder: DecodeDeltaReduced takes a reduce of 2, 4 or 8");
  if (p_->c.reduce != 1 && p_->c.reduce != reduce)
    throw std::runtime_error("svc::StreamDecoder: DecodeDeltaReduced's reduce is not the configured one (config.reduce must be 1 or the argument)");
  p_->Delta(stream, offsets, n_frames, key, reduce, 1, gaze, sink);
}

void StreamDecoder::DecodeDeltaTemporalReduced(const uint8_t* stream, const uint64_t* offsets, uint32_t n_frames, const uint32_t* key,
                                               uint32_t period, uint32_t reduce, const Gaze& gaze, const Sink& sink) {
  if (period != 1 && period != 2 && period != 4)
    throw std::runtime_error("svc::StreamDecoder: DecodeDeltaTemporalReduced takes a period of 1, 2 or 4");
  if (reduce != 2 && reduce != 4 && reduce != 8)
    throw std::runtime_error("svc::StreamDecoder: DecodeDeltaTemporalReduced takes a reduce of 2, 4 or 8");
  if (p_->c.reduce != 1 && p_->c.reduce != reduce)
    throw std::runtime_error("svc::StreamDecoder: DecodeDeltaTemporalReduced's reduce is not the configured one (config.reduce must be 1 or the argument)");
  if (p_->c.batch % period != 0)
    throw std::runtime_error("svc::StreamDecoder: DecodeDeltaTemporalReduced carries the frame at index -period from batch to batch: config.batch must be a multiple of the period");
  if (period == 1) return DecodeDeltaReduced(stream, offsets, n_frames, key, reduce, gaze, sink);
  p_->Delta(stream, offsets, n_frames, key, reduce, period, gaze, sink);
}

// DecodeDelta (reduce 1), DecodeDeltaTemporal (reduce 1, a period above 1), DecodeDeltaReduced and DecodeDeltaTemporalReduced (a reduce
// and a period above 1): one chain through the batches, carried
// in the two chain buffers -- whole reconstructed frames at reduce 1, their bands (0, 0, K, K) above; with a period the carried frame is
// the batch's last of layer 0
void StreamDecoder::Impl::Delta(const uint8_t* stream, const uint64_t* offsets, uint32_t n_frames, const uint32_t* key, uint32_t reduce,
                                uint32_t period, const Gaze& gaze, const Sink& sink) {
  Impl& m = *this;
  if (n_frames == 0) { m.stats = DecodeStats{}; return; }
  if (!stream || !offsets) throw std::runtime_error("svc::StreamDecoder: null stream");
  const uint64_t total = offsets[n_frames];  // the stream's bytes, from offsets[0] on
  uint32_t hdr[kHeaderWords];
  FirstHeader(stream, offsets, n_frames, "", hdr);
  m.Size(hdr, hdr[kHMagic] == kMagicE, false, false, true, reduce);
  const uint32_t B = c.batch;

  DecodeStats st;
  m.pipe->Begin([&](uint32_t slot) { Deliver(*m.slots[slot], m.dw, m.dh, m.svce, false, st, sink); });
  uint32_t batch = 0;
  for (uint32_t first = 0; first < n_frames; ++batch) {
    const uint32_t cnt = std::min(B, n_frames - first);
    const uint32_t slot = m.pipe->Acquire();
    Slot& s = *m.slots[slot];
    const uint64_t bytes = StageFrames(kWho, m.crew, stream, offsets, total, first, cnt, s.pin_in, s.in, s.pin_off.p);
    m.StageGaze(s, gaze, first, cnt);
    for (uint32_t i = 0; i < cnt; ++i) s.pin_key.p[i] = key ? key[first + i] : 0u;  // (frame 0 has no frame before it: a key frame)
    s.first = first; s.count = cnt;
    m.pipe->Submit(
        slot,
        [&](hipStream_t si) -> uint64_t {
          Hip(hipMemcpyAsync(s.in.p, s.pin_in.p, bytes, hipMemcpyHostToDevice, si), "hipMemcpyAsync H2D");
          Hip(hipMemcpyAsync(s.off.p, s.pin_off.p, (cnt + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, si), "hipMemcpyAsync H2D offsets");
          Hip(hipMemcpyAsync(s.gaze.p, s.pin_gaze.p, 4 * cnt * sizeof(uint32_t), hipMemcpyHostToDevice, si), "hipMemcpyAsync H2D gaze");
          Hip(hipMemcpyAsync(s.key.p, s.pin_key.p, cnt * sizeof(uint32_t), hipMemcpyHostToDevice, si), "hipMemcpyAsync H2D key flags");
          return bytes + (cnt + 1) * sizeof(uint64_t) + 5 * cnt * sizeof(uint32_t);
        },
        [&](hipStream_t sk) {
          const uint8_t* qin = s.in.p;
          const uint64_t* qoff = s.off.p;
          uint64_t qbytes = bytes;
          if (m.svce) {  // SVCE -> SVCQ in device scratch, then the SVCQ route unchanged
            Abi(svc_hip_entropy_decode_frames(s.in.p, bytes, s.off.p, cnt, m.pw, m.ph, m.bw, m.bh, m.mbw, m.mbh, m.ews.p, m.ews_bytes, m.q.p,
                                              m.q_bytes, m.qoff.p, s.estatus.p, sk),
                "svc_hip_entropy_decode_frames");
            qin = m.q.p; qoff = m.qoff.p; qbytes = m.q_bytes;
          }
          // the frame before this batch: the batch before left it in chain[(batch - 1) % 2], and its length is on its way to the host
          const uint8_t* prev = nullptr;
          uint64_t prev_bytes = 0;
          if (batch > 0) {
            Hip(hipStreamSynchronize(sk), "hipStreamSynchronize");
            prev = m.chain[(batch - 1) % 2].p;
            prev_bytes = m.pin_chain_len.p[0];
          }
          if (reduce > 1 && period > 1)
            Abi(svc_hip_decode_delta_levels_temporal_reduced_frames(qin, qbytes, qoff, cnt, prev, prev_bytes, s.key.p, m.pw, m.ph, m.bw, m.bh,
                                                                    m.mbw, m.mbh, c.fg_step, c.bg_step, reduce, s.gaze.p, m.ws.p, m.ws_bytes,
                                                                    m.rec.p, s.disp.p, m.dw, m.dh, m.chain[batch % 2].p, m.chain_bytes,
                                                                    m.chain_len.p, s.status.p, sk, period),
                "svc_hip_decode_delta_levels_temporal_reduced_frames");
          else if (reduce > 1)
            Abi(svc_hip_decode_delta_levels_reduced_frames(qin, qbytes, qoff, cnt, prev, prev_bytes, s.key.p, m.pw, m.ph, m.bw, m.bh, m.mbw,
                                                           m.mbh, c.fg_step, c.bg_step, reduce, s.gaze.p, m.ws.p, m.ws_bytes, m.rec.p,
                                                           s.disp.p, m.dw, m.dh, m.chain[batch % 2].p, m.chain_bytes, m.chain_len.p,
                                                           s.status.p, sk),
                "svc_hip_decode_delta_levels_reduced_frames");
          else if (period > 1)
            Abi(svc_hip_decode_delta_levels_temporal_frames(qin, qbytes, qoff, cnt, prev, prev_bytes, s.key.p, m.pw, m.ph, m.bw, m.bh, m.mbw,
                                                            m.mbh, c.fg_step, c.bg_step, s.gaze.p, m.ws.p, m.ws_bytes, m.rec.p, s.disp.p, m.dw,
                                                            m.dh, m.chain[batch % 2].p, m.chain_bytes, m.chain_len.p, s.status.p, sk, period),
                "svc_hip_decode_delta_levels_temporal_frames");
          else
            Abi(svc_hip_decode_delta_levels_frames(qin, qbytes, qoff, cnt, prev, prev_bytes, s.key.p, m.pw, m.ph, m.bw, m.bh, m.mbw, m.mbh,
                                                   c.fg_step, c.bg_step, s.gaze.p, m.ws.p, m.ws_bytes, m.rec.p, s.disp.p, m.dw, m.dh,
                                                   m.chain[batch % 2].p, m.chain_bytes, m.chain_len.p, s.status.p, sk),
                "svc_hip_decode_delta_levels_frames");
          if (first + cnt < n_frames)
            Hip(hipMemcpyAsync(m.pin_chain_len.p, m.chain_len.p, sizeof(uint64_t), hipMemcpyDeviceToHost, sk), "hipMemcpyAsync D2H chain length");
        },
        [&](hipStream_t so) -> uint64_t {
          Hip(hipMemcpyAsync(s.pin_disp.p, s.disp.p, cnt * m.disp_bytes, hipMemcpyDeviceToHost, so), "hipMemcpyAsync D2H display");
          Hip(hipMemcpyAsync(s.pin_status.p, s.status.p, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost, so), "hipMemcpyAsync D2H status");
          if (m.svce)
            Hip(hipMemcpyAsync(s.pin_estatus.p, s.estatus.p, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost, so), "hipMemcpyAsync D2H status");
          return cnt * (m.disp_bytes + (m.svce ? 2 : 1) * sizeof(uint32_t));
        });
    first += cnt;
  }
  m.Finish(st);
}

void StreamDecoder::DecodeWire(const uint8_t* stream, uint64_t bytes, const Gaze& gaze, const Sink& sink) {
  Impl& m = *p_;
  const StreamDecoderConfig& c = m.c;
  if (c.reduce != 1) throw std::runtime_error("svc::StreamDecoder: DecodeWire does not decode at reduced size (reduce must be 1)");
  if (!stream || bytes < sizeof(svc_wire_header)) throw std::runtime_error("svc::StreamDecoder: a wire stream opens with a 32-byte header");
  svc_wire_header hdr;
  std::memcpy(&hdr, stream, sizeof(hdr));
  uint32_t emit_h = 0;
  uint64_t fbytes = 0;
  Abi(svc_hip_wire_layout(&hdr, bytes, &emit_h, &fbytes), "svc_hip_wire_layout");
  const uint32_t n_frames = hdr.frame_count;
  if (n_frames == 0) { m.stats = DecodeStats{}; return; }
  m.SizeWire(hdr.frame_w + hdr.frame_excess_w, hdr.frame_h + hdr.frame_excess_h, hdr.transform_block_w, fbytes,
             c.display_w ? c.display_w : hdr.frame_w, c.display_h ? c.display_h : hdr.frame_h);
  const uint8_t* records = stream + sizeof(hdr);
  const uint32_t B = c.wire_batch;

  DecodeStats st;
  m.pipe->Begin([&](uint32_t slot) { Deliver(*m.slots[slot], m.dw, m.dh, false, false, st, sink); });
  for (uint32_t first = 0; first < n_frames;) {
    const uint32_t cnt = std::min(B, n_frames - first);
    const uint32_t slot = m.pipe->Acquire();
    Slot& s = *m.slots[slot];
    const uint64_t batch_bytes = (uint64_t)cnt * fbytes;  // whole frames: the stream's length was checked by svc_hip_wire_layout
    m.crew.Copy(s.pin_in.p, records + (uint64_t)first * fbytes, batch_bytes);
    m.StageGaze(s, gaze, first, cnt);
    s.first = first; s.count = cnt;
    m.pipe->Submit(
        slot,
        [&](hipStream_t si) -> uint64_t {
          Hip(hipMemcpyAsync(s.in.p, s.pin_in.p, batch_bytes, hipMemcpyHostToDevice, si), "hipMemcpyAsync H2D");
          Hip(hipMemcpyAsync(s.gaze.p, s.pin_gaze.p, 4 * cnt * sizeof(uint32_t), hipMemcpyHostToDevice, si), "hipMemcpyAsync H2D gaze");
          return batch_bytes + 4 * cnt * sizeof(uint32_t);
        },
        [&](hipStream_t sk) {
          Abi(svc_hip_decode_records_frames(s.in.p, fbytes, cnt, m.pw, m.ph, m.bw, emit_h, c.fg_step, c.bg_step, s.gaze.p, m.rec.p, s.disp.p,
                                            m.dw, m.dh, sk),
              "svc_hip_decode_records_frames");
        },
        [&](hipStream_t so) -> uint64_t {
          Hip(hipMemcpyAsync(s.pin_disp.p, s.disp.p, cnt * m.disp_bytes, hipMemcpyDeviceToHost, so), "hipMemcpyAsync D2H display");
          return cnt * m.disp_bytes;
        });
    first += cnt;
  }
  m.Finish(st);
}

}  // namespace svc
