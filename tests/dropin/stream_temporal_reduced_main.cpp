// stream_temporal_reduced_main.cpp -- a host application written against include/svc/stream_decoder.hpp only: decodes a delta stream with
// temporal layers (svc_hip_delta_levels_temporal_frames's output or svc::StreamEncoderConfig::temporal_period's, or its band (0, 0, K, K)
// by svc_hip_band_levels_frames, as <prefix>.big, SVCQ or SVCE, and <prefix>.offsets, its n + 1 u64 frame offsets) to display frames at
// 1 / reduce of the size with svc::StreamDecoder::DecodeDeltaTemporalReduced.  The arguments are stream_delta_reduced_main's and the period:
//   stream_temporal_reduced_main <prefix> <frames> <display_w> <display_h> <gaze_file|-> <key_file|-> <batch> <depth> <reduce> <period> <out|->
// reduce: the method's argument, 2, 4 or 8; "R:C" also sets StreamDecoderConfig::reduce to C (else it stays 1).  period: 1, 2 or 4.
// reduce 0: the route a small viewer had before -- DecodeDeltaTemporal at full size with the display pass at display_w x display_h --
// for tools/decode_probe.py temporal-reduced-rate to measure against.
// display_w / display_h 0: the padded size over reduce.  gaze_file: one line per frame, "x y" (the gaze centre in display coordinates) or "-"
// (none); "-": no gaze.  key_file: one line per frame, 0 or 1 (the key flags the delta call took); "-": none.  out: the display frames
// back to back (u8 B,G,R) and <out>.status (u32 per frame); "-": no output, the clip is decoded again and again for a second and the
// PCIe-inclusive rate printed with where its time went.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "svc/stream_decoder.hpp"

static bool ReadFile(const std::string& path, std::vector<uint8_t>* out) {
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) return false;
  std::fseek(f, 0, SEEK_END);
  const long n = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  out->resize(n > 0 ? (size_t)n : 0);
  const bool ok = out->empty() || std::fread(out->data(), 1, out->size(), f) == out->size();
  std::fclose(f);
  return ok;
}

int main(int argc, char** argv) {
  if (argc != 12) { std::fprintf(stderr, "usage: see the header comment\n"); return 2; }
  const std::string prefix = argv[1], gaze_path = argv[5], key_path = argv[6], out_path = argv[11];
  const uint32_t n = std::atoi(argv[2]);
  svc::StreamDecoderConfig cfg;
  cfg.display_w = std::atoi(argv[3]);
  cfg.display_h = std::atoi(argv[4]);
  cfg.batch = std::atoi(argv[7]);
  cfg.depth = std::atoi(argv[8]);
  const uint32_t reduce = std::atoi(argv[9]);
  if (const char* colon = std::strchr(argv[9], ':')) cfg.reduce = std::atoi(colon + 1);
  const uint32_t period = std::atoi(argv[10]);

  std::vector<uint8_t> big, off_bytes;
  if (!ReadFile(prefix + ".big", &big) || !ReadFile(prefix + ".offsets", &off_bytes)) {
    std::fprintf(stderr, "cannot read %s.big / .offsets\n", prefix.c_str());
    return 1;
  }
  std::vector<uint64_t> offsets(off_bytes.size() / 8);
  std::memcpy(offsets.data(), off_bytes.data(), offsets.size() * 8);
  if (n == 0 || offsets.size() < (size_t)n + 1) { std::fprintf(stderr, "%s.offsets holds fewer than %u frames\n", prefix.c_str(), n); return 1; }

  std::vector<int64_t> gx(n, -1), gy(n, -1);
  if (gaze_path != "-") {
    FILE* f = std::fopen(gaze_path.c_str(), "r");
    if (!f) { std::fprintf(stderr, "cannot read %s\n", gaze_path.c_str()); return 1; }
    char line[128];
    for (uint32_t i = 0; i < n && std::fgets(line, sizeof(line), f); ++i) {
      long x, y;
      if (std::sscanf(line, "%ld %ld", &x, &y) == 2) { gx[i] = x; gy[i] = y; }
    }
    std::fclose(f);
  }
  const svc::StreamDecoder::Gaze gaze = [&](uint32_t i, uint32_t* x, uint32_t* y) {
    if (i >= n || gx[i] < 0) return false;
    *x = (uint32_t)gx[i]; *y = (uint32_t)gy[i];
    return true;
  };
  std::vector<uint32_t> key;
  if (key_path != "-") {
    FILE* f = std::fopen(key_path.c_str(), "r");
    if (!f) { std::fprintf(stderr, "cannot read %s\n", key_path.c_str()); return 1; }
    key.assign(n, 0);
    char line[128];
    for (uint32_t i = 0; i < n && std::fgets(line, sizeof(line), f); ++i) key[i] = std::atoi(line) != 0;
    std::fclose(f);
  }

  const bool files = out_path != "-";
  FILE *f_out = nullptr, *f_st = nullptr;
  if (files) {
    f_out = std::fopen(out_path.c_str(), "wb");
    f_st = std::fopen((out_path + ".status").c_str(), "wb");
    if (!f_out || !f_st) { std::fprintf(stderr, "cannot open %s\n", out_path.c_str()); return 1; }
  }
  try {
    svc::StreamDecoder dec(cfg);
    uint32_t next = 0, total = 0;
    bool dump = files;
    auto sink = [&](const svc::DecodedBatch& b) {
      if (b.first_frame != next) { std::fprintf(stderr, "batch out of order: %u, expected %u\n", b.first_frame, next); std::exit(1); }
      next += b.count; total += b.count;
      if (!dump) return;
      std::fwrite(b.bgr, 1, (size_t)b.count * b.width * b.height * 3, f_out);
      std::fwrite(b.status, sizeof(uint32_t), b.count, f_st);
    };
    const uint32_t* flags = key.empty() ? nullptr : key.data();
    auto play = [&] {
      if (reduce == 0 && !std::strchr(argv[9], ':')) dec.DecodeDeltaTemporal(big.data(), offsets.data(), n, flags, period, gaze, sink);
      else dec.DecodeDeltaTemporalReduced(big.data(), offsets.data(), n, flags, period, reduce, gaze, sink);
    };
    const auto t_first = std::chrono::steady_clock::now();
    play();
    const double s_first = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_first).count();
    if (total != n) { std::fprintf(stderr, "%u decoded frames, expected %u\n", total, n); return 1; }
    if (files) {
      std::fclose(f_out); std::fclose(f_st);
      std::printf("%u frames decoded, %.0f frames/s PCIe-inclusive (first pass, buffers included)\n", n, n / s_first);
      return 0;
    }
    dump = false;
    uint32_t passes = 0, frames = 0;
    svc::DecodeStats sum;
    const auto t0 = std::chrono::steady_clock::now();
    double s = 0;
    do {
      next = 0; total = 0;
      play();
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
