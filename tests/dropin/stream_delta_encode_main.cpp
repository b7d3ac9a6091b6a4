// stream_delta_encode_main.cpp -- a host application written against include/svc/stream_encoder.hpp only: encodes a raw clip from
// a file with svc::StreamEncoderConfig::delta, the stream svc::StreamDecoder::DecodeDelta plays (tests/dropin/stream_delta_main).
//   stream_delta_encode_main <clip.raw> <w> <h> <frames> <levels> <dct_block> <batch> <depth> <seed> <delta: 0|1> <key_interval>
//                            <entropy: 0|1> <out_prefix> [wire | budget | enh]
// <prefix>.big holds every batch's frames back to back (SVCQ, or SVCE with entropy), <prefix>.offsets their n + 1 u64 frame offsets,
// <prefix>.types the region ids (u32 per MV block) and, with delta, <prefix>.key one line per frame, 0 or 1: the key flags in the form
// stream_delta_main reads.  delta 0: the plain compact stream of the same configuration, for comparison.  The optional last word adds a
// setting the delta stream does not go with (wire records, a byte budget of 1 MB with a one-entry ladder, enh_step 1): the
// constructor's refusal is printed and the exit status is 1.
// out_prefix "-": no output files; the clip is encoded again and again for a second and the PCIe-inclusive rate printed.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "svc/stream_encoder.hpp"

int main(int argc, char** argv) {
  if (argc != 14 && argc != 15) { std::fprintf(stderr, "usage: see the header comment\n"); return 2; }
  const uint32_t w = std::atoi(argv[2]), h = std::atoi(argv[3]), n = std::atoi(argv[4]);
  svc::StreamEncoderConfig cfg;
  cfg.width = w; cfg.height = h;
  cfg.levels = std::atoi(argv[5]);
  cfg.dct_block = std::atoi(argv[6]);
  cfg.batch = std::atoi(argv[7]);
  cfg.depth = std::atoi(argv[8]);
  cfg.seed = std::strtoull(argv[9], nullptr, 10);
  cfg.compact = true;
  cfg.delta = std::atoi(argv[10]) != 0;
  cfg.key_interval = std::atoi(argv[11]);
  cfg.entropy = std::atoi(argv[12]) != 0;
  const std::string prefix = argv[13], extra = argc == 15 ? argv[14] : "";
  if (extra == "wire") cfg.wire = true;
  else if (extra == "budget") { cfg.compact_budget = 1000000; cfg.compact_ladder = {svc_step_pair{cfg.fg_step, cfg.bg_step}}; }
  else if (extra == "enh") cfg.enh_step = 1;
  else if (!extra.empty()) { std::fprintf(stderr, "unknown setting %s\n", extra.c_str()); return 2; }

  std::vector<uint8_t> clip((size_t)w * h * 3 * n);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(clip.data(), 1, clip.size(), f) != clip.size()) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
  std::fclose(f);

  const bool files = prefix != "-";
  FILE *f_ty = nullptr, *f_big = nullptr, *f_off = nullptr, *f_key = nullptr;
  if (files) {
    f_ty = std::fopen((prefix + ".types").c_str(), "wb");
    f_big = std::fopen((prefix + ".big").c_str(), "wb");
    f_off = std::fopen((prefix + ".offsets").c_str(), "wb");
    f_key = cfg.delta ? std::fopen((prefix + ".key").c_str(), "w") : nullptr;
    if (!f_ty || !f_big || !f_off || (cfg.delta && !f_key)) { std::fprintf(stderr, "cannot open outputs under %s\n", prefix.c_str()); return 1; }
  }
  try {
    svc::StreamEncoder enc(cfg);
    uint32_t next = 1, total = 0;
    uint64_t base = 0, bytes = 0;  // bytes of the stream written so far; of the pass
    bool dump = files;
    auto sink = [&](const svc::EncodedBatch& b) {
      if (b.first_frame != next) { std::fprintf(stderr, "batch out of order: %u, expected %u\n", b.first_frame, next); std::exit(1); }
      if (b.coeffs || !b.compact || !b.compact_offsets || b.compact_bytes != b.compact_offsets[b.count] || (cfg.delta != (b.compact_key != nullptr))) {
        std::fprintf(stderr, "compact batch without its stream or its key flags\n"); std::exit(1);
      }
      next += b.count; total += b.count; bytes += b.compact_bytes;
      if (!dump) return;
      std::fwrite(b.block_types, sizeof(uint32_t), (size_t)b.count * b.mv_field_w * b.mv_field_h, f_ty);
      std::fwrite(b.compact, 1, b.compact_bytes, f_big);
      for (uint32_t i = b.first_frame == 1 ? 0 : 1; i <= b.count; ++i) {
        const uint64_t o = base + b.compact_offsets[i];
        std::fwrite(&o, sizeof(o), 1, f_off);
      }
      base += b.compact_bytes;
      if (cfg.delta)
        for (uint32_t i = 0; i < b.count; ++i) std::fprintf(f_key, "%u\n", b.compact_key[i] ? 1u : 0u);
    };
    enc.Encode(clip.data(), n, sink);
    if (total != n - 1) { std::fprintf(stderr, "%u encoded frames, expected %u\n", total, n - 1); return 1; }
    if (files) {
      std::fclose(f_ty); std::fclose(f_big); std::fclose(f_off);
      if (f_key) std::fclose(f_key);
      return 0;
    }
    dump = false;
    uint32_t passes = 0, frames = 0;
    double kernels_ms = 0;
    uint32_t batches = 0;
    const auto t0 = std::chrono::steady_clock::now();
    double s = 0;
    do {
      next = 1; total = 0; bytes = 0;
      enc.Encode(clip.data(), n, sink);
      kernels_ms += enc.last_stats().kernels_ms; batches += enc.last_stats().batches;
      ++passes; frames += total;
      s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    } while (s < 1.0 && passes < 64);
    std::printf("%u encoded frames, %.0f frames/s PCIe-inclusive (%s%s), kernels %.3f ms per batch of %u, %.0f stream bytes per frame\n", frames,
                frames / s, cfg.delta ? "delta" : "compact alone", cfg.entropy ? ", entropy-coded" : "", kernels_ms / batches, cfg.batch,
                (double)bytes / total);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
