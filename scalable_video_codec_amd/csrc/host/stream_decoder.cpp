// stream_decoder.cpp -- include/svc/stream_decoder.hpp: buffers, streams and the batch schedule of stream_encoder.cpp, run the
// other way.  No arithmetic of the hot path lives here; the gaze rule and the decode are calls into the C ABI.
#include "svc/stream_decoder.hpp"

#include "../stream_format.hpp"
#include "copy_crew.hpp"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace svc {
namespace {

void Hip(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string("svc::StreamDecoder: ") + what + ": " + hipGetErrorString(e));
}
void Abi(int rc, const char* what) {
  if (rc) throw std::runtime_error(std::string("svc::StreamDecoder: ") + what + ": " + svc_hip_last_error());
}

template <typename T> struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  void Alloc(size_t count) {
    Free();
    Hip(hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(count, 1) * sizeof(T)), "hipMalloc");
    n = count;
  }
  void Free() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
  ~DevBuf() { Free(); }
};
template <typename T> struct PinBuf {
  T* p = nullptr;
  size_t n = 0;
  void Alloc(size_t count) {
    Free();
    Hip(hipHostMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(count, 1) * sizeof(T), hipHostMallocDefault), "hipHostMalloc");
    n = count;
  }
  void Free() { if (p) (void)hipHostFree(p); p = nullptr; n = 0; }
  ~PinBuf() { Free(); }
};

struct Slot {
  PinBuf<uint8_t> pin_in, pin_disp;
  PinBuf<uint64_t> pin_off;
  PinBuf<uint32_t> pin_gaze, pin_status;
  DevBuf<uint8_t> in, disp;
  DevBuf<uint64_t> off;
  DevBuf<uint32_t> gaze, status, estatus;  // estatus: svc_hip_entropy_decode_frames's codes (SVCE)
  PinBuf<uint32_t> pin_estatus;
  hipEvent_t h2d_done = nullptr, compute_done = nullptr, d2h_done = nullptr;
  hipEvent_t t_in[2] = {}, t_k[2] = {}, t_out[2] = {};
  uint64_t h2d_bytes = 0, d2h_bytes = 0;
  uint32_t first = 0, count = 0;
  bool busy = false;
  ~Slot() {
    for (hipEvent_t e : {h2d_done, compute_done, d2h_done, t_in[0], t_in[1], t_k[0], t_k[1], t_out[0], t_out[1]})
      if (e) (void)hipEventDestroy(e);
  }
};

}  // namespace

struct StreamDecoder::Impl {
  StreamDecoderConfig c;
  // geometry the buffers are sized for (0 = none yet)
  uint32_t pw = 0, ph = 0, bw = 0, bh = 0, mbw = 0, mbh = 0, dw = 0, dh = 0;
  uint64_t disp_bytes = 0, ws_bytes = 0;
  bool wire = false;        // the buffers are sized for DecodeWire
  bool svce = false;        // Decode: the stream is SVCE, decoded to SVCQ in q first
  DevBuf<uint8_t> q, ews;   // SVCE: the batch's SVCQ frames and the coder's workspace (the kernels' stream only)
  DevBuf<uint64_t> qoff;
  uint64_t q_bytes = 0, ews_bytes = 0;
  uint64_t frame_bytes = 0; // DecodeWire: bytes of one frame's records
  DevBuf<float> rec;        // the kernels' stream only: one for all slots
  DevBuf<uint8_t> ws;
  std::vector<std::unique_ptr<Slot>> slots;
  hipStream_t s_in = nullptr, s_compute = nullptr, s_out = nullptr;
  CopyCrew crew{3};
  DecodeStats stats;

  ~Impl() {
    for (hipStream_t s : {s_in, s_compute, s_out})
      if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
  }

  void Size(const uint32_t* hdr, bool entropy) {
    const uint32_t w = hdr[kHWidth], h = hdr[kHHeight], tw = hdr[kHTileW], th = hdr[kHTileH], mw = hdr[kHMvW], mh = hdr[kHMvH];
    const uint32_t want_dw = c.display_w ? c.display_w : w, want_dh = c.display_h ? c.display_h : h;
    if (!wire && entropy == svce && w == pw && h == ph && tw == bw && th == bh && mw == mbw && mh == mbh && want_dw == dw && want_dh == dh)
      return;
    for (hipStream_t s : {s_in, s_compute, s_out}) Hip(hipStreamSynchronize(s), "hipStreamSynchronize");
    const uint64_t need_ws = svc_hip_decode_levels_workspace_bytes(c.batch, w, h, tw, th);
    if (!need_ws) Abi(SVC_ERR_UNSUPPORTED, "no decoder for the first frame's geometry");
    if (want_dw > w || want_dh > h) throw std::runtime_error("svc::StreamDecoder: the display size exceeds the padded frame");
    if (entropy) {
      q_bytes = svc_hip_levels_max_bytes(c.batch, w, h, tw, th, mw, mh);
      ews_bytes = svc_hip_entropy_workspace_bytes(c.batch, w, h, tw, th, mw, mh);
      if (!q_bytes || !ews_bytes) Abi(SVC_ERR_UNSUPPORTED, "no entropy decoder for the first frame's geometry");
      q.Alloc(q_bytes); ews.Alloc(ews_bytes); qoff.Alloc(c.batch + 1);
    }
    svce = entropy;
    wire = false;
    pw = w; ph = h; bw = tw; bh = th; mbw = mw; mbh = mh; dw = want_dw; dh = want_dh;
    disp_bytes = (uint64_t)dw * dh * 3;
    ws_bytes = need_ws;
    const size_t B = c.batch;
    rec.Alloc(B * pw * ph * 3);
    ws.Alloc(ws_bytes);
    for (auto& s : slots) {
      s->disp.Alloc(B * disp_bytes); s->pin_disp.Alloc(B * disp_bytes);
    }
  }

  // DecodeWire: a padded w x h frame of `fbytes` bytes of b x b records, shown at want_dw x want_dh
  void SizeWire(uint32_t w, uint32_t h, uint32_t b, uint64_t fbytes, uint32_t want_dw, uint32_t want_dh) {
    if (wire && w == pw && h == ph && b == bw && fbytes == frame_bytes && want_dw == dw && want_dh == dh) return;
    for (hipStream_t s : {s_in, s_compute, s_out}) Hip(hipStreamSynchronize(s), "hipStreamSynchronize");
    if (want_dw > w || want_dh > h) throw std::runtime_error("svc::StreamDecoder: the display size exceeds the padded frame");
    wire = true;
    pw = w; ph = h; bw = bh = b; mbw = mbh = 0; dw = want_dw; dh = want_dh; frame_bytes = fbytes;
    disp_bytes = (uint64_t)dw * dh * 3;
    const size_t B = c.wire_batch;
    rec.Alloc(B * pw * ph * 3);
    for (auto& s : slots) {
      s->disp.Alloc(B * disp_bytes); s->pin_disp.Alloc(B * disp_bytes);
      s->in.Alloc(B * frame_bytes); s->pin_in.Alloc(B * frame_bytes);
      std::memset(s->pin_status.p, 0, s->pin_status.n * sizeof(uint32_t));  // the records carry no per-frame status
    }
  }
};

StreamDecoder::StreamDecoder(const StreamDecoderConfig& config) : p_(new Impl) {
  Impl& m = *p_;
  m.c = config;
  const StreamDecoderConfig& c = m.c;
  if (c.batch == 0 || c.wire_batch == 0 || c.depth < 3 || !c.fg_step || !c.bg_step || (c.display_w == 0) != (c.display_h == 0))
    throw std::runtime_error("svc::StreamDecoder: invalid configuration");
  Hip(hipStreamCreateWithFlags(&m.s_in, hipStreamNonBlocking), "hipStreamCreate");
  Hip(hipStreamCreateWithFlags(&m.s_compute, hipStreamNonBlocking), "hipStreamCreate");
  Hip(hipStreamCreateWithFlags(&m.s_out, hipStreamNonBlocking), "hipStreamCreate");
  const size_t B = std::max(c.batch, c.wire_batch);  // per-frame arrays serve both paths
  for (uint32_t i = 0; i < c.depth; ++i) {
    std::unique_ptr<Slot> s(new Slot);
    s->pin_off.Alloc(B + 1); s->off.Alloc(B + 1);
    s->pin_gaze.Alloc(4 * B); s->gaze.Alloc(4 * B);
    s->pin_status.Alloc(B); s->status.Alloc(B);
    s->pin_estatus.Alloc(B); s->estatus.Alloc(B);
    Hip(hipEventCreateWithFlags(&s->h2d_done, hipEventDisableTiming), "hipEventCreate");
    Hip(hipEventCreateWithFlags(&s->compute_done, hipEventDisableTiming), "hipEventCreate");
    Hip(hipEventCreateWithFlags(&s->d2h_done, hipEventDisableTiming), "hipEventCreate");
    for (hipEvent_t* e : {&s->t_in[0], &s->t_in[1], &s->t_k[0], &s->t_k[1], &s->t_out[0], &s->t_out[1]}) Hip(hipEventCreate(e), "hipEventCreate");
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
  if (offsets[0] % 16 || offsets[0] > total || total - offsets[0] < kHeaderBytes || offsets[1] < offsets[0] + kHeaderBytes)
    throw std::runtime_error("svc::StreamDecoder: the first frame's header is out of range");
  uint32_t hdr[kHeaderWords];
  std::memcpy(hdr, stream + offsets[0], sizeof(hdr));
  if ((hdr[kHMagic] != kMagicQ && hdr[kHMagic] != kMagicE) || hdr[kHVersion] != kVersion)
    throw std::runtime_error("svc::StreamDecoder: the stream does not open with an SVCQ v1 or SVCE v1 header");
  m.Size(hdr, hdr[kHMagic] == kMagicE);
  const uint32_t B = c.batch;

  using Clock = std::chrono::steady_clock;
  DecodeStats st;
  const Clock::time_point t_start = Clock::now();

  auto deliver = [&](Slot& s) {
    Hip(hipEventSynchronize(s.d2h_done), "hipEventSynchronize");
    float ms = 0;
    Hip(hipEventElapsedTime(&ms, s.t_in[0], s.t_in[1]), "hipEventElapsedTime"); st.h2d_ms += ms;
    Hip(hipEventElapsedTime(&ms, s.t_k[0], s.t_k[1]), "hipEventElapsedTime"); st.kernels_ms += ms;
    Hip(hipEventElapsedTime(&ms, s.t_out[0], s.t_out[1]), "hipEventElapsedTime"); st.d2h_ms += ms;
    st.h2d_bytes += s.h2d_bytes; st.d2h_bytes += s.d2h_bytes;
    ++st.batches; st.frames += s.count;
    if (m.svce)  // a frame the entropy decoder refused is zeros to the SVCQ decoder (status 2): report the entropy decoder's code
      for (uint32_t i = 0; i < s.count; ++i)
        if (s.pin_estatus.p[i]) s.pin_status.p[i] = s.pin_estatus.p[i];
    DecodedBatch b;
    b.first_frame = s.first; b.count = s.count; b.width = m.dw; b.height = m.dh;
    b.bgr = s.pin_disp.p; b.status = s.pin_status.p;
    sink(b);
  };

  std::vector<Slot*> pending;
  for (uint32_t first = 0, k = 0; first < n_frames; ++k) {
    const uint32_t cnt = std::min(B, n_frames - first);
    Slot& s = *m.slots[k % c.depth];
    if (s.busy) { Hip(hipEventSynchronize(s.d2h_done), "hipEventSynchronize"); s.busy = false; }
    // the batch's bytes: from its lowest offset (rounded down to 16: frames stay aligned) to its highest, inside the stream; an
    // offset outside it becomes one the kernels refuse (status 1), so a malformed frame is reported, never read past the copy
    uint64_t lo = total, hi = 0;
    for (uint32_t i = first; i <= first + cnt; ++i) {
      const uint64_t o = std::min(offsets[i], total);
      lo = std::min(lo, o); hi = std::max(hi, o);
    }
    lo &= ~(uint64_t)15;
    const uint64_t bytes = hi - lo;
    if (s.pin_in.n < std::max<uint64_t>(bytes, 16)) {  // grown on demand: a batch of 1080p frames is about 17 MB
      const size_t cap = (size_t)(bytes + bytes / 4 + 4095) & ~(size_t)4095;
      s.pin_in.Alloc(cap); s.in.Alloc(cap);
    }
    m.crew.Copy(s.pin_in.p, stream + lo, bytes);
    for (uint32_t i = 0; i <= cnt; ++i) {
      const uint64_t o = offsets[first + i];
      s.pin_off.p[i] = o <= total ? o - lo : ~(uint64_t)15;
    }
    for (uint32_t i = 0; i < cnt; ++i) {
      uint32_t x = 0, y = 0, *r = s.pin_gaze.p + 4 * i;
      if (gaze && gaze(first + i, &x, &y))
        Abi(svc_hip_gaze_rect(x, y, c.max_gaze_w, c.max_gaze_h, m.dw, m.dh, m.pw, m.ph, r), "svc_hip_gaze_rect");
      else
        r[0] = r[1] = r[2] = r[3] = 0;
    }
    Hip(hipEventRecord(s.t_in[0], m.s_in), "hipEventRecord");
    Hip(hipMemcpyAsync(s.in.p, s.pin_in.p, bytes, hipMemcpyHostToDevice, m.s_in), "hipMemcpyAsync H2D");
    Hip(hipMemcpyAsync(s.off.p, s.pin_off.p, (cnt + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, m.s_in), "hipMemcpyAsync H2D offsets");
    Hip(hipMemcpyAsync(s.gaze.p, s.pin_gaze.p, 4 * cnt * sizeof(uint32_t), hipMemcpyHostToDevice, m.s_in), "hipMemcpyAsync H2D gaze");
    Hip(hipEventRecord(s.t_in[1], m.s_in), "hipEventRecord");
    Hip(hipEventRecord(s.h2d_done, m.s_in), "hipEventRecord");
    s.h2d_bytes = bytes + (cnt + 1) * sizeof(uint64_t) + 4 * cnt * sizeof(uint32_t);

    Hip(hipStreamWaitEvent(m.s_compute, s.h2d_done, 0), "hipStreamWaitEvent");
    Hip(hipEventRecord(s.t_k[0], m.s_compute), "hipEventRecord");
    const uint8_t* qin = s.in.p;
    const uint64_t* qoff = s.off.p;
    uint64_t qbytes = bytes;
    if (m.svce) {  // SVCE -> SVCQ in device scratch, then the SVCQ decoder unchanged
      Abi(svc_hip_entropy_decode_frames(s.in.p, bytes, s.off.p, cnt, m.pw, m.ph, m.bw, m.bh, m.mbw, m.mbh, m.ews.p, m.ews_bytes, m.q.p,
                                        m.q_bytes, m.qoff.p, s.estatus.p, m.s_compute),
          "svc_hip_entropy_decode_frames");
      qin = m.q.p; qoff = m.qoff.p; qbytes = m.q_bytes;
    }
    Abi(svc_hip_decode_levels_frames(qin, qbytes, qoff, cnt, m.pw, m.ph, m.bw, m.bh, m.mbw, m.mbh, c.fg_step, c.bg_step, s.gaze.p,
                                     m.ws.p, m.ws_bytes, m.rec.p, s.disp.p, m.dw, m.dh, s.status.p, m.s_compute),
        "svc_hip_decode_levels_frames");
    Hip(hipEventRecord(s.t_k[1], m.s_compute), "hipEventRecord");
    Hip(hipEventRecord(s.compute_done, m.s_compute), "hipEventRecord");

    Hip(hipStreamWaitEvent(m.s_out, s.compute_done, 0), "hipStreamWaitEvent");
    Hip(hipEventRecord(s.t_out[0], m.s_out), "hipEventRecord");
    Hip(hipMemcpyAsync(s.pin_disp.p, s.disp.p, cnt * m.disp_bytes, hipMemcpyDeviceToHost, m.s_out), "hipMemcpyAsync D2H display");
    Hip(hipMemcpyAsync(s.pin_status.p, s.status.p, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost, m.s_out), "hipMemcpyAsync D2H status");
    if (m.svce)
      Hip(hipMemcpyAsync(s.pin_estatus.p, s.estatus.p, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost, m.s_out), "hipMemcpyAsync D2H status");
    Hip(hipEventRecord(s.t_out[1], m.s_out), "hipEventRecord");
    Hip(hipEventRecord(s.d2h_done, m.s_out), "hipEventRecord");
    s.d2h_bytes = cnt * (m.disp_bytes + (m.svce ? 2 : 1) * sizeof(uint32_t));

    s.busy = true; s.first = first; s.count = cnt;
    pending.push_back(&s);
    first += cnt;
    if (pending.size() >= c.depth - 1) { deliver(*pending.front()); pending.erase(pending.begin()); }
  }
  for (Slot* s : pending) deliver(*s);
  for (auto& s : m.slots) s->busy = false;  // everything delivered and synchronised
  st.wall_ms = std::chrono::duration<double, std::milli>(Clock::now() - t_start).count();
  m.stats = st;
}

void StreamDecoder::DecodeWire(const uint8_t* stream, uint64_t bytes, const Gaze& gaze, const Sink& sink) {
  Impl& m = *p_;
  const StreamDecoderConfig& c = m.c;
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

  using Clock = std::chrono::steady_clock;
  DecodeStats st;
  const Clock::time_point t_start = Clock::now();

  auto deliver = [&](Slot& s) {
    Hip(hipEventSynchronize(s.d2h_done), "hipEventSynchronize");
    float ms = 0;
    Hip(hipEventElapsedTime(&ms, s.t_in[0], s.t_in[1]), "hipEventElapsedTime"); st.h2d_ms += ms;
    Hip(hipEventElapsedTime(&ms, s.t_k[0], s.t_k[1]), "hipEventElapsedTime"); st.kernels_ms += ms;
    Hip(hipEventElapsedTime(&ms, s.t_out[0], s.t_out[1]), "hipEventElapsedTime"); st.d2h_ms += ms;
    st.h2d_bytes += s.h2d_bytes; st.d2h_bytes += s.d2h_bytes;
    ++st.batches; st.frames += s.count;
    DecodedBatch b;
    b.first_frame = s.first; b.count = s.count; b.width = m.dw; b.height = m.dh;
    b.bgr = s.pin_disp.p; b.status = s.pin_status.p;
    sink(b);
  };

  std::vector<Slot*> pending;
  for (uint32_t first = 0, k = 0; first < n_frames; ++k) {
    const uint32_t cnt = std::min(B, n_frames - first);
    Slot& s = *m.slots[k % c.depth];
    if (s.busy) { Hip(hipEventSynchronize(s.d2h_done), "hipEventSynchronize"); s.busy = false; }
    const uint64_t batch_bytes = (uint64_t)cnt * fbytes;  // whole frames: the stream's length was checked by svc_hip_wire_layout
    m.crew.Copy(s.pin_in.p, records + (uint64_t)first * fbytes, batch_bytes);
    for (uint32_t i = 0; i < cnt; ++i) {
      uint32_t x = 0, y = 0, *r = s.pin_gaze.p + 4 * i;
      if (gaze && gaze(first + i, &x, &y))
        Abi(svc_hip_gaze_rect(x, y, c.max_gaze_w, c.max_gaze_h, m.dw, m.dh, m.pw, m.ph, r), "svc_hip_gaze_rect");
      else
        r[0] = r[1] = r[2] = r[3] = 0;
    }
    Hip(hipEventRecord(s.t_in[0], m.s_in), "hipEventRecord");
    Hip(hipMemcpyAsync(s.in.p, s.pin_in.p, batch_bytes, hipMemcpyHostToDevice, m.s_in), "hipMemcpyAsync H2D");
    Hip(hipMemcpyAsync(s.gaze.p, s.pin_gaze.p, 4 * cnt * sizeof(uint32_t), hipMemcpyHostToDevice, m.s_in), "hipMemcpyAsync H2D gaze");
    Hip(hipEventRecord(s.t_in[1], m.s_in), "hipEventRecord");
    Hip(hipEventRecord(s.h2d_done, m.s_in), "hipEventRecord");
    s.h2d_bytes = batch_bytes + 4 * cnt * sizeof(uint32_t);

    Hip(hipStreamWaitEvent(m.s_compute, s.h2d_done, 0), "hipStreamWaitEvent");
    Hip(hipEventRecord(s.t_k[0], m.s_compute), "hipEventRecord");
    Abi(svc_hip_decode_records_frames(s.in.p, fbytes, cnt, m.pw, m.ph, m.bw, emit_h, c.fg_step, c.bg_step, s.gaze.p, m.rec.p, s.disp.p,
                                      m.dw, m.dh, m.s_compute),
        "svc_hip_decode_records_frames");
    Hip(hipEventRecord(s.t_k[1], m.s_compute), "hipEventRecord");
    Hip(hipEventRecord(s.compute_done, m.s_compute), "hipEventRecord");

    Hip(hipStreamWaitEvent(m.s_out, s.compute_done, 0), "hipStreamWaitEvent");
    Hip(hipEventRecord(s.t_out[0], m.s_out), "hipEventRecord");
    Hip(hipMemcpyAsync(s.pin_disp.p, s.disp.p, cnt * m.disp_bytes, hipMemcpyDeviceToHost, m.s_out), "hipMemcpyAsync D2H display");
    Hip(hipEventRecord(s.t_out[1], m.s_out), "hipEventRecord");
    Hip(hipEventRecord(s.d2h_done, m.s_out), "hipEventRecord");
    s.d2h_bytes = cnt * m.disp_bytes;

    s.busy = true; s.first = first; s.count = cnt;
    pending.push_back(&s);
    first += cnt;
    if (pending.size() >= c.depth - 1) { deliver(*pending.front()); pending.erase(pending.begin()); }
  }
  for (Slot* s : pending) deliver(*s);
  for (auto& s : m.slots) s->busy = false;  // everything delivered and synchronised
  st.wall_ms = std::chrono::duration<double, std::milli>(Clock::now() - t_start).count();
  m.stats = st;
}

}  // namespace svc
