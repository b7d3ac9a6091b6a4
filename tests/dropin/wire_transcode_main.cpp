// wire_transcode_main.cpp -- the bridge between the two streams as a filter, written against include/svc/wire_transcoder.hpp only.
//   wire_transcode_main to-compact [--entropy] [--mv-block N] [--foreground-quant-step 1] [--background-quant-step 640] [--batch N]
//     stdin: a whole wire stream (Header + records, what apps/encoder.cpp or svc::StreamEncoder{wire = true} write)
//     stdout: a compact file = u64 frame count n | u64 offsets[n + 1] (from the first frame's first byte) | the n SVCQ frames (SVCE
//     with --entropy).  stderr: one line per frame whose status is not 0.
//   wire_transcode_main to-wire [--source WxH] [--emit-h H] [--batch N]
//     stdin: a compact file; stdout: the wire stream, header included.  The header states the padded size with zero excess, or with
//     --source the source size and the rest as excess (what the reference's decoder shows); --emit-h: the rows of the padded frame the
//     records cover (default all, the reading of the reference's decoder).
//   --rate (either direction): nothing is written; the input is transcoded again and again for a second after a first pass and the
//   PCIe-inclusive rate printed with where its time went.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "svc/wire_transcoder.hpp"

static bool ReadAll(FILE* f, std::vector<uint8_t>* out) {
  out->clear();
  std::vector<uint8_t> buf(1 << 24);
  size_t n;
  while ((n = std::fread(buf.data(), 1, buf.size(), f)) > 0) out->insert(out->end(), buf.begin(), buf.begin() + n);
  return !std::ferror(f);
}

// `pass` transcodes the input once and returns its frames
template <typename Pass> static void Rate(svc::WireTranscoder& tc, const char* what, Pass pass) {
  (void)pass();  // the first pass sizes the buffers
  uint32_t passes = 0, frames = 0;
  svc::TranscodeStats sum;
  const auto t0 = std::chrono::steady_clock::now();
  double s = 0;
  do {
    frames += pass();
    const svc::TranscodeStats& e = tc.last_stats();
    sum.batches += e.batches; sum.wall_ms += e.wall_ms;
    sum.h2d_ms += e.h2d_ms; sum.kernels_ms += e.kernels_ms; sum.d2h_ms += e.d2h_ms;
    sum.h2d_bytes += e.h2d_bytes; sum.d2h_bytes += e.d2h_bytes;
    ++passes;
    s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  } while (s < 1.0 && passes < 256);
  std::printf("%s: %u frames, %.0f frames/s PCIe-inclusive (after a first pass)\n", what, frames, frames / s);
  std::printf("phases {\"passes\": %u, \"batches\": %u, \"seconds\": %.4f, \"wall_ms_per_batch\": %.3f, "
              "\"device_ms_per_batch\": {\"h2d\": %.3f, \"kernels\": %.3f, \"d2h\": %.3f}, \"h2d_GBps\": %.2f, \"d2h_GBps\": %.2f, "
              "\"h2d_bytes_per_frame\": %.0f, \"d2h_bytes_per_frame\": %.0f}\n",
              passes, sum.batches, s, sum.wall_ms / sum.batches, sum.h2d_ms / sum.batches, sum.kernels_ms / sum.batches,
              sum.d2h_ms / sum.batches, sum.h2d_bytes / (sum.h2d_ms * 1e6), sum.d2h_bytes / (sum.d2h_ms * 1e6),
              (double)sum.h2d_bytes / frames, (double)sum.d2h_bytes / frames);
}

static int Usage() {
  std::fprintf(stderr, "usage: wire_transcode_main to-compact|to-wire [options] (see the header comment)\n");
  return 2;
}

int main(int argc, char** argv) {
  if (argc < 2) return Usage();
  const std::string mode = argv[1];
  if (mode != "to-compact" && mode != "to-wire") return Usage();
  svc::WireTranscoderConfig cfg;
  uint32_t src_w = 0, src_h = 0, emit_h = 0;
  bool rate = false;
  for (int i = 2; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--entropy") { cfg.entropy = true; continue; }
    if (a == "--rate") { rate = true; continue; }
    if (i + 1 >= argc) { std::fprintf(stderr, "option %s needs a value\n", a.c_str()); return 2; }
    const char* v = argv[++i];
    if (a == "--mv-block") cfg.mv_block_w = cfg.mv_block_h = (uint32_t)std::strtoul(v, nullptr, 10);
    else if (a == "--foreground-quant-step") cfg.fg_step = (uint32_t)std::strtoul(v, nullptr, 10);
    else if (a == "--background-quant-step") cfg.bg_step = (uint32_t)std::strtoul(v, nullptr, 10);
    else if (a == "--batch") cfg.wire_batch = (uint32_t)std::strtoul(v, nullptr, 10);
    else if (a == "--emit-h") emit_h = (uint32_t)std::strtoul(v, nullptr, 10);
    else if (a == "--source") {
      if (std::sscanf(v, "%ux%u", &src_w, &src_h) != 2) { std::fprintf(stderr, "--source takes WxH\n"); return 2; }
    } else { std::fprintf(stderr, "unknown option %s\n", a.c_str()); return 2; }
  }
  std::vector<uint8_t> in;
  if (!ReadAll(stdin, &in)) { std::fprintf(stderr, "cannot read stdin\n"); return 1; }
  try {
    svc::WireTranscoder tc(cfg);
    uint32_t next = 0;
    if (mode == "to-compact" && rate) {
      Rate(tc, cfg.entropy ? "to-compact --entropy" : "to-compact", [&] {
        uint32_t n = 0;
        tc.ToCompact(in.data(), in.size(), [&](const svc::CompactBatch& b) { n += b.count; });
        return n;
      });
    } else if (mode == "to-compact") {
      std::vector<uint8_t> frames;
      std::vector<uint64_t> offsets{0};
      tc.ToCompact(in.data(), in.size(), [&](const svc::CompactBatch& b) {
        if (b.first_frame != next) { std::fprintf(stderr, "batch out of order: %u, expected %u\n", b.first_frame, next); std::exit(1); }
        next += b.count;
        const uint64_t base = frames.size();
        frames.insert(frames.end(), b.frames, b.frames + b.offsets[b.count]);
        for (uint32_t i = 0; i < b.count; ++i) {
          offsets.push_back(base + b.offsets[i + 1]);
          if (b.status[i]) std::fprintf(stderr, "frame %u: status %u\n", b.first_frame + i, b.status[i]);
        }
      });
      const uint64_t n = next;
      std::fwrite(&n, sizeof(n), 1, stdout);
      std::fwrite(offsets.data(), sizeof(uint64_t), offsets.size(), stdout);
      std::fwrite(frames.data(), 1, frames.size(), stdout);
    } else {
      uint64_t n = 0;
      if (in.size() < sizeof(n)) { std::fprintf(stderr, "a compact file opens with its frame count\n"); return 1; }
      std::memcpy(&n, in.data(), sizeof(n));
      if (n > 0xFFFFFFFFull || in.size() < 8 * (n + 2)) { std::fprintf(stderr, "truncated compact file\n"); return 1; }
      std::vector<uint64_t> offsets(n + 1);
      std::memcpy(offsets.data(), in.data() + 8, 8 * (n + 1));
      const uint8_t* frames = in.data() + 8 * (n + 2);
      if (offsets[n] > in.size() - 8 * (n + 2)) { std::fprintf(stderr, "truncated compact file\n"); return 1; }
      // (n + 2 words is a multiple of 16 bytes only for even n: the frames are copied to an aligned place of their own)
      std::vector<uint8_t> body(frames, frames + offsets[n]);
      bool header_written = false;
      if (rate) {
        Rate(tc, "to-wire", [&] {
          uint32_t m = 0;
          tc.ToWire(body.data(), offsets.data(), (uint32_t)n, emit_h, [&](const svc::WireBatch& b) { m += b.count; });
          return m;
        });
        return 0;
      }
      tc.ToWire(body.data(), offsets.data(), (uint32_t)n, emit_h, [&](const svc::WireBatch& b) {
        if (b.first_frame != next) { std::fprintf(stderr, "batch out of order: %u, expected %u\n", b.first_frame, next); std::exit(1); }
        next += b.count;
        if (!header_written) {
          svc_wire_header h{};
          h.frame_count = (uint32_t)n;
          h.frame_w = src_w ? src_w : b.frame_w; h.frame_h = src_h ? src_h : b.frame_h;
          h.frame_excess_w = b.frame_w - h.frame_w; h.frame_excess_h = b.frame_h - h.frame_h;
          h.transform_block_w = h.transform_block_h = b.block;
          h.channel_count = 3;
          std::fwrite(&h, sizeof(h), 1, stdout);
          header_written = true;
        }
        std::fwrite(b.records, 1, (size_t)b.count * b.frame_bytes, stdout);
        for (uint32_t i = 0; i < b.count; ++i)
          if (b.status[i]) std::fprintf(stderr, "frame %u: status %u\n", b.first_frame + i, b.status[i]);
      });
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return std::fflush(stdout) == 0 ? 0 : 1;
}
