// wire_decode_main.cpp -- a headless apps/decoder.cpp, written against include/svc/stream_decoder.hpp only: the reference's wire
// stream (Header + records, what apps/encoder.cpp or svc::StreamEncoder{wire = true} write) -> the display frames its decoder shows.
//   wire_decode_main [--in FILE] [--out FILE|-] [--gaze FILE] [--foreground-quant-step 1] [--background-quant-step 640]
//                    [--max-gaze-rect-w 64] [--max-gaze-rect-h 64] [--batch N]
// The stream comes from stdin unless --in names a file.  The four quant / gaze options and their defaults are the reference
// decoder's (apps/decoder.cpp:21-26).  --gaze: one line per frame, "x y" (the gaze centre in display = source coordinates, where the
// reference reads the mouse) or "-" (none); without it no frame is gazed.  --out FILE: the display frames back to back (u8 B,G,R,
// the header's frame_w x frame_h).  --out - (the default): no frames are written; the stream is decoded again and again for a
// second and the PCIe-inclusive rate printed with where its time went.  --batch: frames per batch (StreamDecoderConfig::wire_batch).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "svc/stream_decoder.hpp"

static bool ReadAll(FILE* f, std::vector<uint8_t>* out) {
  out->clear();
  std::vector<uint8_t> buf(1 << 24);
  size_t n;
  while ((n = std::fread(buf.data(), 1, buf.size(), f)) > 0) out->insert(out->end(), buf.begin(), buf.begin() + n);
  return !std::ferror(f);
}

int main(int argc, char** argv) {
  std::string in_path, out_path = "-", gaze_path;
  svc::StreamDecoderConfig cfg;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (i + 1 >= argc) { std::fprintf(stderr, "option %s needs a value (usage: see the header comment)\n", a.c_str()); return 2; }
    const char* v = argv[++i];
    if (a == "--in") in_path = v;
    else if (a == "--out") out_path = v;
    else if (a == "--gaze") gaze_path = v;
    else if (a == "--foreground-quant-step") cfg.fg_step = (uint32_t)std::strtoul(v, nullptr, 10);
    else if (a == "--background-quant-step") cfg.bg_step = (uint32_t)std::strtoul(v, nullptr, 10);
    else if (a == "--max-gaze-rect-w") cfg.max_gaze_w = (uint32_t)std::strtoul(v, nullptr, 10);
    else if (a == "--max-gaze-rect-h") cfg.max_gaze_h = (uint32_t)std::strtoul(v, nullptr, 10);
    else if (a == "--batch") cfg.wire_batch = (uint32_t)std::strtoul(v, nullptr, 10);
    else { std::fprintf(stderr, "unknown option %s (usage: see the header comment)\n", a.c_str()); return 2; }
  }

  std::vector<uint8_t> stream;
  FILE* fin = in_path.empty() ? stdin : std::fopen(in_path.c_str(), "rb");
  if (!fin || !ReadAll(fin, &stream)) { std::fprintf(stderr, "cannot read %s\n", in_path.empty() ? "stdin" : in_path.c_str()); return 1; }
  if (fin != stdin) std::fclose(fin);

  std::vector<int64_t> gx, gy;
  if (!gaze_path.empty()) {
    FILE* f = std::fopen(gaze_path.c_str(), "r");
    if (!f) { std::fprintf(stderr, "cannot read %s\n", gaze_path.c_str()); return 1; }
    char line[128];
    while (std::fgets(line, sizeof(line), f)) {
      long x, y;
      const bool ok = std::sscanf(line, "%ld %ld", &x, &y) == 2 && x >= 0 && y >= 0;
      gx.push_back(ok ? x : -1); gy.push_back(ok ? y : -1);
    }
    std::fclose(f);
  }
  const svc::StreamDecoder::Gaze gaze = [&](uint32_t i, uint32_t* x, uint32_t* y) {
    if (i >= gx.size() || gx[i] < 0) return false;
    *x = (uint32_t)gx[i]; *y = (uint32_t)gy[i];
    return true;
  };

  const bool files = out_path != "-";
  FILE* f_out = nullptr;
  if (files && !(f_out = std::fopen(out_path.c_str(), "wb"))) { std::fprintf(stderr, "cannot open %s\n", out_path.c_str()); return 1; }
  try {
    svc::StreamDecoder dec(cfg);
    uint32_t next = 0, total = 0;
    bool dump = files;
    auto sink = [&](const svc::DecodedBatch& b) {
      if (b.first_frame != next) { std::fprintf(stderr, "batch out of order: %u, expected %u\n", b.first_frame, next); std::exit(1); }
      next += b.count; total += b.count;
      if (dump) std::fwrite(b.bgr, 1, (size_t)b.count * b.width * b.height * 3, f_out);
    };
    const auto t_first = std::chrono::steady_clock::now();
    dec.DecodeWire(stream.data(), stream.size(), gaze, sink);
    const double s_first = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_first).count();
    if (files) {
      std::fclose(f_out);
      std::printf("%u frames decoded, %.0f frames/s PCIe-inclusive (first pass, buffers included)\n", total, total / s_first);
      return 0;
    }
    if (total == 0) { std::printf("0 frames in the stream\n"); return 0; }
    dump = false;
    uint32_t passes = 0, frames = 0;
    svc::DecodeStats sum;
    const auto t0 = std::chrono::steady_clock::now();
    double s = 0;
    do {
      next = 0; total = 0;
      dec.DecodeWire(stream.data(), stream.size(), gaze, sink);
      const svc::DecodeStats& e = dec.last_stats();
      sum.batches += e.batches; sum.frames += e.frames; sum.wall_ms += e.wall_ms;
      sum.h2d_ms += e.h2d_ms; sum.kernels_ms += e.kernels_ms; sum.d2h_ms += e.d2h_ms;
      sum.h2d_bytes += e.h2d_bytes; sum.d2h_bytes += e.d2h_bytes;
      ++passes; frames += total;
      s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    } while (s < 1.0 && passes < 256);
    std::printf("%u decoded frames, %.0f frames/s PCIe-inclusive (after a first pass)\n", frames, frames / s);
    std::printf("phases {\"passes\": %u, \"batches\": %u, \"seconds\": %.4f, \"wall_ms_per_batch\": %.3f, "
                "\"device_ms_per_batch\": {\"h2d\": %.3f, \"kernels\": %.3f, \"d2h\": %.3f}, \"h2d_GBps\": %.2f, \"d2h_GBps\": %.2f, "
                "\"h2d_bytes_per_frame\": %.0f, \"d2h_bytes_per_frame\": %.0f}\n",
                passes, sum.batches, s, sum.wall_ms / sum.batches, sum.h2d_ms / sum.batches, sum.kernels_ms / sum.batches,
                sum.d2h_ms / sum.batches, sum.h2d_bytes / (sum.h2d_ms * 1e6), sum.d2h_bytes / (sum.d2h_ms * 1e6),
                (double)sum.h2d_bytes / frames, (double)sum.d2h_bytes / frames);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
