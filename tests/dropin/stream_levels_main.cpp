// stream_levels_main.cpp -- stream_main with the compact output (svc::StreamEncoderConfig::compact): the same command line and
// output files, but <prefix>.big holds the compact quantised-coefficient stream of every batch back to back and <prefix>.offsets
// its n + 1 u64 frame offsets (scalable_video_codec_amd/levels.py iter_frames reads the pair).  tests/test_gpu_levels.py compares
// it with stream_main's planes.
//   stream_levels_main <clip.raw> <w> <h> <frames> <levels> <dct_block> <wire: 0> <batch> <seed> <out_prefix>
// out_prefix "-": no output files, only the PCIe-inclusive rate and the phases.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "svc/stream_encoder.hpp"

int main(int argc, char** argv) {
  if (argc != 11) { std::fprintf(stderr, "usage: see the header comment\n"); return 2; }
  const uint32_t w = std::atoi(argv[2]), h = std::atoi(argv[3]), n = std::atoi(argv[4]);
  svc::StreamEncoderConfig cfg;
  cfg.width = w; cfg.height = h;
  cfg.levels = std::atoi(argv[5]);
  cfg.dct_block = std::atoi(argv[6]);
  cfg.wire = std::atoi(argv[7]) != 0;
  cfg.batch = std::atoi(argv[8]);
  cfg.seed = std::strtoull(argv[9], nullptr, 10);
  cfg.compact = true;
  const std::string prefix = argv[10];

  std::vector<uint8_t> clip((size_t)w * h * 3 * n);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(clip.data(), 1, clip.size(), f) != clip.size()) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
  std::fclose(f);

  const bool files = prefix != "-";
  FILE *f_mv = nullptr, *f_ty = nullptr, *f_gm = nullptr, *f_big = nullptr, *f_off = nullptr;
  if (files) {
    f_mv = std::fopen((prefix + ".mv").c_str(), "wb");
    f_ty = std::fopen((prefix + ".types").c_str(), "wb");
    f_gm = std::fopen((prefix + ".gm").c_str(), "wb");
    f_big = std::fopen((prefix + ".big").c_str(), "wb");
    f_off = std::fopen((prefix + ".offsets").c_str(), "wb");
    if (!f_mv || !f_ty || !f_gm || !f_big || !f_off) { std::fprintf(stderr, "cannot open outputs under %s\n", prefix.c_str()); return 1; }
  }
  try {
    svc::StreamEncoder enc(cfg);
    uint32_t next = 1, total = 0;
    uint64_t base = 0;  // bytes of the stream written so far
    bool dump = files;
    auto sink = [&](const svc::EncodedBatch& b) {
      if (b.first_frame != next) { std::fprintf(stderr, "batch out of order: %u, expected %u\n", b.first_frame, next); std::exit(1); }
      if (b.coeffs || !b.compact || !b.compact_offsets || b.compact_bytes != b.compact_offsets[b.count]) {
        std::fprintf(stderr, "compact batch without its stream\n"); std::exit(1);
      }
      next += b.count; total += b.count;
      if (!dump) return;
      const size_t blocks = (size_t)b.mv_field_w * b.mv_field_h;
      std::fwrite(b.mv_xy, sizeof(float), b.count * blocks * 2, f_mv);
      std::fwrite(b.block_types, sizeof(uint32_t), b.count * blocks, f_ty);
      std::fwrite(b.global_motion, sizeof(float), b.count * 2, f_gm);
      std::fwrite(b.compact, 1, b.compact_bytes, f_big);
      for (uint32_t i = b.first_frame == 1 ? 0 : 1; i <= b.count; ++i) {
        const uint64_t o = base + b.compact_offsets[i];
        std::fwrite(&o, sizeof(o), 1, f_off);
      }
      base += b.compact_bytes;
    };
    enc.Encode(clip.data(), n, sink);
    if (total != n - 1) { std::fprintf(stderr, "%u encoded frames, expected %u\n", total, n - 1); return 1; }
    if (files) {
      std::fclose(f_mv); std::fclose(f_ty); std::fclose(f_gm); std::fclose(f_big); std::fclose(f_off);
      return 0;
    }
    // the same clip again, as often as it takes to fill a second: the PCIe-inclusive rate, and where its time went
    dump = false;
    uint32_t passes = 0, frames = 0;
    svc::EncodeStats sum;
    const auto t0 = std::chrono::steady_clock::now();
    double s = 0;
    do {
      next = 1; total = 0;
      enc.Encode(clip.data(), n, sink);
      const svc::EncodeStats& e = enc.last_stats();
      sum.batches += e.batches; sum.wall_ms += e.wall_ms; sum.staging_ms += e.staging_ms; sum.slot_wait_ms += e.slot_wait_ms;
      sum.deliver_wait_ms += e.deliver_wait_ms; sum.sink_ms += e.sink_ms; sum.h2d_ms += e.h2d_ms; sum.kernels_ms += e.kernels_ms;
      sum.d2h_ms += e.d2h_ms; sum.h2d_bytes += e.h2d_bytes; sum.d2h_bytes += e.d2h_bytes;
      sum.copy_threads = e.copy_threads; sum.host_cores = e.host_cores;
      ++passes; frames += total;
      s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    } while (s < 1.0 && passes < 64);
    std::printf("%u encoded frames, %.0f frames/s PCIe-inclusive (second pass, compact output)\n", frames, frames / s);
    std::printf("phases {\"passes\": %u, \"batches\": %u, \"seconds\": %.4f, \"host_cores\": %u, \"copy_threads\": %u, "
                "\"host_ms_per_batch\": {\"staging\": %.3f, \"slot_wait\": %.3f, \"deliver_wait\": %.3f, \"sink\": %.3f, \"wall\": %.3f}, "
                "\"device_ms_per_batch\": {\"h2d\": %.3f, \"kernels\": %.3f, \"d2h\": %.3f}, \"h2d_GBps\": %.2f, \"d2h_GBps\": %.2f, "
                "\"d2h_bytes_per_frame\": %.0f}\n",
                passes, sum.batches, s, sum.host_cores, sum.copy_threads, sum.staging_ms / sum.batches, sum.slot_wait_ms / sum.batches,
                sum.deliver_wait_ms / sum.batches, sum.sink_ms / sum.batches, sum.wall_ms / sum.batches, sum.h2d_ms / sum.batches,
                sum.kernels_ms / sum.batches, sum.d2h_ms / sum.batches, sum.h2d_bytes / (sum.h2d_ms * 1e6), sum.d2h_bytes / (sum.d2h_ms * 1e6),
                (double)sum.d2h_bytes / frames);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
