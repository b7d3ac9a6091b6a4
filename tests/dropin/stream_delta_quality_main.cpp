// stream_delta_quality_main.cpp -- a host application written against include/svc/stream_encoder.hpp only: the delta stream at constant
// quality (svc::StreamEncoderConfig::delta with compact_quality and compact_ladder): every group of frames, from a key frame up to the
// next, is packed with the coarsest ladder entry at which every frame of the group still reaches the PSNR, under the group's byte
// budget where one is set.
//   stream_delta_quality_main <clip.raw> <w> <h> <frames> <levels> <dct_block> <batch> <depth> <seed> <key_interval> <quality_db> <budget>
//                             <fg:bg,fg:bg,...> <quality2_db> <entropy: 0|1> <out_prefix> [auto_key | temporal | enh | nodelta]
// <prefix>.big holds every batch's frames back to back (SVCQ, or SVCE with entropy), <prefix>.offsets their n + 1 u64 frame offsets,
// <prefix>.types the region ids (u32 per MV block), <prefix>.choice one u32 per frame (its group's entry, bit 30 = target not met, bit 31
// = over the cap), <prefix>.distortion one u64 per frame (its D at that entry), <prefix>.key one line per frame, 0 or 1 (the form
// stream_delta_main reads) and <prefix>.batches one line per delivered batch: its first frame's stream index and its count.
// quality_db 0: the quality is off -- the plain delta run of the same configuration, without choices (a budget other than 0 is then the
// budgeted delta run).  A second quality other than 0 is set from the sink after the first delivery (StreamEncoder::SetCompactQuality): it
// applies from some later batch on, never inside one.  The optional last word adds a setting the quality target does not go with; the
// constructor's refusal is printed and the exit status is 1, as for a key_interval of 0 or one that does not divide the batch.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "svc/stream_encoder.hpp"

int main(int argc, char** argv) {
  if (argc != 17 && argc != 18) { std::fprintf(stderr, "usage: see the header comment\n"); return 2; }
  const uint32_t w = std::atoi(argv[2]), h = std::atoi(argv[3]), n = std::atoi(argv[4]);
  svc::StreamEncoderConfig cfg;
  cfg.width = w; cfg.height = h;
  cfg.levels = std::atoi(argv[5]);
  cfg.dct_block = std::atoi(argv[6]);
  cfg.batch = std::atoi(argv[7]);
  cfg.depth = std::atoi(argv[8]);
  cfg.seed = std::strtoull(argv[9], nullptr, 10);
  cfg.compact = true;
  cfg.delta = true;
  cfg.key_interval = std::atoi(argv[10]);
  cfg.compact_quality = std::atof(argv[11]);
  cfg.compact_budget = (uint32_t)std::strtoul(argv[12], nullptr, 10);
  for (const char* p = argv[13]; *p;) {
    char* end = nullptr;
    svc_step_pair e;
    e.fg_step = (uint32_t)std::strtoul(p, &end, 10);
    if (*end != ':') { std::fprintf(stderr, "ladder: expected fg:bg pairs separated by commas\n"); return 2; }
    e.bg_step = (uint32_t)std::strtoul(end + 1, &end, 10);
    cfg.compact_ladder.push_back(e);
    p = *end == ',' ? end + 1 : end;
    if (*end && *end != ',') { std::fprintf(stderr, "ladder: expected fg:bg pairs separated by commas\n"); return 2; }
  }
  const double quality2 = std::atof(argv[14]);
  cfg.entropy = std::atoi(argv[15]) != 0;
  const std::string prefix = argv[16], extra = argc == 18 ? argv[17] : "";
  if (extra == "auto_key") cfg.auto_key = true;
  else if (extra == "temporal") cfg.temporal_period = 2;
  else if (extra == "enh") cfg.enh_step = 1;
  else if (extra == "nodelta") cfg.delta = false;
  else if (!extra.empty()) { std::fprintf(stderr, "unknown setting %s\n", extra.c_str()); return 2; }
  const bool chosen = cfg.compact_quality != 0 || cfg.compact_budget != 0;

  std::vector<uint8_t> clip((size_t)w * h * 3 * n);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(clip.data(), 1, clip.size(), f) != clip.size()) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
  std::fclose(f);

  try {
    svc::StreamEncoder enc(cfg);  // (a refused configuration leaves no files)
    FILE* f_ty = std::fopen((prefix + ".types").c_str(), "wb");
    FILE* f_big = std::fopen((prefix + ".big").c_str(), "wb");
    FILE* f_off = std::fopen((prefix + ".offsets").c_str(), "wb");
    FILE* f_ch = std::fopen((prefix + ".choice").c_str(), "wb");
    FILE* f_d = std::fopen((prefix + ".distortion").c_str(), "wb");
    FILE* f_key = std::fopen((prefix + ".key").c_str(), "w");
    FILE* f_bat = std::fopen((prefix + ".batches").c_str(), "w");
    if (!f_ty || !f_big || !f_off || !f_ch || !f_d || !f_key || !f_bat) { std::fprintf(stderr, "cannot open outputs under %s\n", prefix.c_str()); return 1; }
    uint32_t next = 1, total = 0, over = 0, below = 0;
    uint64_t base = 0;  // bytes of the stream written so far
    bool first_delivery = true;
    auto sink = [&](const svc::EncodedBatch& b) {
      if (b.first_frame != next) { std::fprintf(stderr, "batch out of order: %u, expected %u\n", b.first_frame, next); std::exit(1); }
      if (b.coeffs || !b.compact || !b.compact_offsets || !b.compact_key || b.compact_bytes != b.compact_offsets[b.count] ||
          (b.compact_choice != nullptr) != chosen || (b.compact_distortion != nullptr) != (cfg.compact_quality != 0)) {
        std::fprintf(stderr, "compact batch without its stream or its key flags, or with choices or distortions it should not have\n"); std::exit(1);
      }
      next += b.count; total += b.count;
      std::fwrite(b.block_types, sizeof(uint32_t), (size_t)b.count * b.mv_field_w * b.mv_field_h, f_ty);
      std::fwrite(b.compact, 1, b.compact_bytes, f_big);
      if (b.compact_choice) {
        for (uint32_t i = 0; i < b.count; ++i) { over += b.compact_choice[i] >> 31; below += (b.compact_choice[i] >> 30) & 1u; }
        std::fwrite(b.compact_choice, sizeof(uint32_t), b.count, f_ch);
      }
      if (b.compact_distortion) std::fwrite(b.compact_distortion, sizeof(uint64_t), b.count, f_d);
      for (uint32_t i = b.first_frame == 1 ? 0 : 1; i <= b.count; ++i) {
        const uint64_t o = base + b.compact_offsets[i];
        std::fwrite(&o, sizeof(o), 1, f_off);
      }
      base += b.compact_bytes;
      for (uint32_t i = 0; i < b.count; ++i) std::fprintf(f_key, "%u\n", b.compact_key[i] ? 1u : 0u);
      std::fprintf(f_bat, "%u %u\n", b.first_frame - 1, b.count);
      if (first_delivery && quality2 != 0) enc.SetCompactQuality(quality2);
      first_delivery = false;
    };
    enc.Encode(clip.data(), n, sink);
    if (total != n - 1) { std::fprintf(stderr, "%u encoded frames, expected %u\n", total, n - 1); return 1; }
    if (enc.last_stats().over_budget_frames != over || (cfg.compact_quality != 0 && enc.last_stats().below_quality_frames != below)) {
      std::fprintf(stderr, "over_budget_frames %u and below_quality_frames %u, the choices say %u and %u\n", enc.last_stats().over_budget_frames,
                   enc.last_stats().below_quality_frames, over, below);
      return 1;
    }
    std::printf("%u encoded frames, %llu B, %u over budget, %u below the quality\n", total, (unsigned long long)base, over, below);
    std::fclose(f_ty); std::fclose(f_big); std::fclose(f_off); std::fclose(f_ch); std::fclose(f_d); std::fclose(f_key); std::fclose(f_bat);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
