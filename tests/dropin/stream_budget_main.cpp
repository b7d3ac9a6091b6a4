// stream_budget_main.cpp -- stream_levels_main with rate control (svc::StreamEncoderConfig::compact_budget): every frame is packed with
// the finest ladder entry whose frame fits the byte budget.  <prefix>.big holds the compact stream of every batch back to back,
// <prefix>.offsets its n + 1 u64 frame offsets and <prefix>.choice one u32 per frame (the entry, bit 31 = over budget).  A second
// budget other than 0 is set from the sink after the first delivery (StreamEncoder::SetCompactBudget): with the default depth of 3 it
// applies from the third batch on.  tests/test_gpu_levels_budget.py compares it with HostStreamEncoder.
//   stream_budget_main <clip.raw> <w> <h> <frames> <levels> <dct_block> <batch> <seed> <budget> <fg:bg,fg:bg,...> <budget2> <out_prefix>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "svc/stream_encoder.hpp"

int main(int argc, char** argv) {
  if (argc != 13) { std::fprintf(stderr, "usage: see the header comment\n"); return 2; }
  const uint32_t w = std::atoi(argv[2]), h = std::atoi(argv[3]), n = std::atoi(argv[4]);
  svc::StreamEncoderConfig cfg;
  cfg.width = w; cfg.height = h;
  cfg.levels = std::atoi(argv[5]);
  cfg.dct_block = std::atoi(argv[6]);
  cfg.batch = std::atoi(argv[7]);
  cfg.seed = std::strtoull(argv[8], nullptr, 10);
  cfg.compact = true;
  cfg.compact_budget = (uint32_t)std::strtoul(argv[9], nullptr, 10);
  for (const char* p = argv[10]; *p;) {
    char* end = nullptr;
    svc_step_pair e;
    e.fg_step = (uint32_t)std::strtoul(p, &end, 10);
    if (*end != ':') { std::fprintf(stderr, "ladder: expected fg:bg pairs separated by commas\n"); return 2; }
    e.bg_step = (uint32_t)std::strtoul(end + 1, &end, 10);
    cfg.compact_ladder.push_back(e);
    p = *end == ',' ? end + 1 : end;
    if (*end && *end != ',') { std::fprintf(stderr, "ladder: expected fg:bg pairs separated by commas\n"); return 2; }
  }
  const uint32_t budget2 = (uint32_t)std::strtoul(argv[11], nullptr, 10);
  const std::string prefix = argv[12];

  std::vector<uint8_t> clip((size_t)w * h * 3 * n);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(clip.data(), 1, clip.size(), f) != clip.size()) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
  std::fclose(f);

  FILE* f_big = std::fopen((prefix + ".big").c_str(), "wb");
  FILE* f_off = std::fopen((prefix + ".offsets").c_str(), "wb");
  FILE* f_ch = std::fopen((prefix + ".choice").c_str(), "wb");
  if (!f_big || !f_off || !f_ch) { std::fprintf(stderr, "cannot open outputs under %s\n", prefix.c_str()); return 1; }
  try {
    svc::StreamEncoder enc(cfg);
    uint32_t next = 1, total = 0, over = 0;
    uint64_t base = 0;  // bytes of the stream written so far
    bool first_delivery = true;
    auto sink = [&](const svc::EncodedBatch& b) {
      if (b.first_frame != next) { std::fprintf(stderr, "batch out of order: %u, expected %u\n", b.first_frame, next); std::exit(1); }
      if (b.coeffs || !b.compact || !b.compact_offsets || !b.compact_choice || b.compact_bytes != b.compact_offsets[b.count]) {
        std::fprintf(stderr, "compact batch without its stream or its choices\n"); std::exit(1);
      }
      next += b.count; total += b.count;
      for (uint32_t i = 0; i < b.count; ++i) over += b.compact_choice[i] >> 31;
      std::fwrite(b.compact, 1, b.compact_bytes, f_big);
      std::fwrite(b.compact_choice, sizeof(uint32_t), b.count, f_ch);
      for (uint32_t i = b.first_frame == 1 ? 0 : 1; i <= b.count; ++i) {
        const uint64_t o = base + b.compact_offsets[i];
        std::fwrite(&o, sizeof(o), 1, f_off);
      }
      base += b.compact_bytes;
      if (first_delivery && budget2) enc.SetCompactBudget(budget2);
      first_delivery = false;
    };
    enc.Encode(clip.data(), n, sink);
    if (total != n - 1) { std::fprintf(stderr, "%u encoded frames, expected %u\n", total, n - 1); return 1; }
    if (enc.last_stats().over_budget_frames != over) {
      std::fprintf(stderr, "over_budget_frames %u, the choices say %u\n", enc.last_stats().over_budget_frames, over);
      return 1;
    }
    std::printf("%u encoded frames, %llu B, %u over budget\n", total, (unsigned long long)base, over);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  std::fclose(f_big); std::fclose(f_off); std::fclose(f_ch);
  return 0;
}
