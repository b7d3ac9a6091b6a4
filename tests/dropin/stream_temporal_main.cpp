// stream_temporal_main.cpp -- a host application written against include/svc/stream_encoder.hpp and stream_decoder.hpp only: encodes a
// raw clip from a file with svc::StreamEncoderConfig::delta and temporal_period, thins the stream it got on the host by copying every
// 2^s-th frame and key flag, and plays each thinning with svc::StreamDecoder::DecodeDeltaTemporal at the period that remains -- and with
// DecodeDelta where that period is 1.
//   stream_temporal_main <clip.raw> <w> <h> <frames> <levels> <dct_block> <batch> <depth> <seed> <temporal_period> <key_interval>
//                        <entropy: 0|1> <out_prefix> [nodelta | auto_key]
// <prefix>.big holds every batch's frames back to back (SVCQ, or SVCE with entropy), <prefix>.offsets their n + 1 u64 frame offsets,
// <prefix>.types the region ids (u32 per MV block), <prefix>.key one line per frame, 0 or 1.  For every = 1, 2, 4 up to the period:
// <prefix>.display<every> the display frames (u8 B,G,R at the padded size) of frames 0, every, 2 * every, .. as DecodeDeltaTemporal plays
// the thinned stream, <prefix>.display<every>.status a u32 per frame, and where period / every == 1 <prefix>.plain<every>, the same frames
// as DecodeDelta plays them.  The optional last word turns `delta` off or auto_key on: the constructor's refusal is printed and the exit
// status is 1, as for a period or a batch it refuses.
// out_prefix "-": no output files; the clip is encoded again and again for a second and the PCIe-inclusive rate printed, then every
// thinning is played again and again for half a second each and its rate printed.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "svc/stream_decoder.hpp"
#include "svc/stream_encoder.hpp"

static bool WriteFile(const std::string& path, const void* p, size_t bytes) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) return false;
  const bool ok = std::fwrite(p, 1, bytes, f) == bytes;
  return std::fclose(f) == 0 && ok;
}

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
  cfg.delta = true;
  cfg.temporal_period = std::atoi(argv[10]);
  cfg.key_interval = std::atoi(argv[11]);
  cfg.entropy = std::atoi(argv[12]) != 0;
  const std::string prefix = argv[13], extra = argc == 15 ? argv[14] : "";
  if (extra == "nodelta") cfg.delta = false;
  else if (extra == "auto_key") cfg.auto_key = true;
  else if (!extra.empty()) { std::fprintf(stderr, "unknown setting %s\n", extra.c_str()); return 2; }

  std::vector<uint8_t> clip((size_t)w * h * 3 * n);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(clip.data(), 1, clip.size(), f) != clip.size()) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
  std::fclose(f);

  const bool files = prefix != "-";
  try {
    svc::StreamEncoder enc(cfg);
    std::vector<uint8_t> big;
    std::vector<uint64_t> offsets{0};
    std::vector<uint32_t> types, key;
    uint32_t next = 1, total = 0, pw = 0, ph = 0;
    uint64_t bytes = 0;
    bool keep = true;  // the first pass keeps the stream; the timed passes after it do not
    auto sink = [&](const svc::EncodedBatch& b) {
      if (b.first_frame != next) { std::fprintf(stderr, "batch out of order: %u, expected %u\n", b.first_frame, next); std::exit(1); }
      if (b.coeffs || !b.compact || !b.compact_offsets || b.compact_bytes != b.compact_offsets[b.count] || !b.compact_key) {
        std::fprintf(stderr, "delta batch without its stream or its key flags\n"); std::exit(1);
      }
      next += b.count; total += b.count; bytes += b.compact_bytes;
      pw = b.padded_w; ph = b.padded_h;
      if (!keep) return;
      const uint64_t base = big.size();
      big.insert(big.end(), b.compact, b.compact + b.compact_bytes);
      for (uint32_t i = 1; i <= b.count; ++i) offsets.push_back(base + b.compact_offsets[i]);
      types.insert(types.end(), b.block_types, b.block_types + (size_t)b.count * b.mv_field_w * b.mv_field_h);
      for (uint32_t i = 0; i < b.count; ++i) key.push_back(b.compact_key[i] ? 1u : 0u);
    };
    enc.Encode(clip.data(), n, sink);
    if (total != n - 1) { std::fprintf(stderr, "%u encoded frames, expected %u\n", total, n - 1); return 1; }
    if (files) {
      std::string keys_text;
      for (uint32_t k : key) keys_text += k ? "1\n" : "0\n";
      if (!WriteFile(prefix + ".big", big.data(), big.size()) || !WriteFile(prefix + ".offsets", offsets.data(), offsets.size() * 8) ||
          !WriteFile(prefix + ".types", types.data(), types.size() * 4) || !WriteFile(prefix + ".key", keys_text.data(), keys_text.size())) {
        std::fprintf(stderr, "cannot write outputs under %s\n", prefix.c_str());
        return 1;
      }
      svc::StreamDecoderConfig dcfg;
      dcfg.batch = cfg.batch;
      dcfg.depth = cfg.depth;
      svc::StreamDecoder dec(dcfg);  // one decoder plays every thinning
      for (uint32_t every = 1; every <= cfg.temporal_period; every *= 2) {
        // the server's part: every `every`-th frame and its key flag, copied
        std::vector<uint8_t> thin;
        std::vector<uint64_t> thin_offsets{0};
        std::vector<uint32_t> thin_key;
        for (uint32_t i = 0; i < total; i += every) {
          thin.insert(thin.end(), big.begin() + offsets[i], big.begin() + offsets[i + 1]);
          thin_offsets.push_back(thin.size());
          thin_key.push_back(key[i]);
        }
        const uint32_t kept = (uint32_t)thin_key.size(), period = cfg.temporal_period / every;
        for (int plain = 0; plain <= (period == 1 ? 1 : 0); ++plain) {
          std::vector<uint8_t> display;
          std::vector<uint32_t> status;
          auto frames = [&](const svc::DecodedBatch& b) {
            display.insert(display.end(), b.bgr, b.bgr + (size_t)b.count * b.width * b.height * 3);
            status.insert(status.end(), b.status, b.status + b.count);
          };
          if (plain) dec.DecodeDelta(thin.data(), thin_offsets.data(), kept, thin_key.data(), nullptr, frames);
          else dec.DecodeDeltaTemporal(thin.data(), thin_offsets.data(), kept, thin_key.data(), period, nullptr, frames);
          if (display.size() != (size_t)kept * pw * ph * 3 || status.size() != kept) {
            std::fprintf(stderr, "the decoder returned %zu display bytes and %zu statuses for %u frames\n", display.size(), status.size(), kept);
            return 1;
          }
          const std::string name = prefix + (plain ? ".plain" : ".display") + std::to_string(every);
          if (!WriteFile(name, display.data(), display.size()) || (!plain && !WriteFile(name + ".status", status.data(), status.size() * 4))) {
            std::fprintf(stderr, "cannot write outputs under %s\n", prefix.c_str());
            return 1;
          }
        }
      }
      return 0;
    }
    uint32_t passes = 0, frames = 0, batches = 0;
    double kernels_ms = 0;
    keep = false;
    const uint32_t stored = total;
    const auto t0 = std::chrono::steady_clock::now();
    double s = 0;
    do {
      next = 1; total = 0; bytes = 0;
      enc.Encode(clip.data(), n, sink);
      kernels_ms += enc.last_stats().kernels_ms; batches += enc.last_stats().batches;
      ++passes; frames += total;
      s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    } while (s < 1.0 && passes < 64);
    std::printf("%u encoded frames, %.0f frames/s PCIe-inclusive (delta, temporal_period %u%s), kernels %.3f ms per batch of %u, %.0f stream bytes per frame\n",
                frames, frames / s, cfg.temporal_period, cfg.entropy ? ", entropy-coded" : "", kernels_ms / batches, cfg.batch,
                (double)bytes / total);
    svc::StreamDecoderConfig dcfg;
    dcfg.batch = cfg.batch;
    dcfg.depth = cfg.depth;
    svc::StreamDecoder dec(dcfg);
    for (uint32_t every = 1; every <= cfg.temporal_period; every *= 2) {
      std::vector<uint8_t> thin;
      std::vector<uint64_t> thin_offsets{0};
      std::vector<uint32_t> thin_key;
      for (uint32_t i = 0; i < stored; i += every) {
        thin.insert(thin.end(), big.begin() + offsets[i], big.begin() + offsets[i + 1]);
        thin_offsets.push_back(thin.size());
        thin_key.push_back(key[i]);
      }
      const uint32_t kept = (uint32_t)thin_key.size(), period = cfg.temporal_period / every;
      for (int plain = 0; plain <= (period == 1 ? 1 : 0); ++plain) {
        uint32_t shown = 0, failed = 0, rounds = 0;
        auto count = [&](const svc::DecodedBatch& b) {
          shown += b.count;
          for (uint32_t i = 0; i < b.count; ++i) failed += b.status[i] != 0;
        };
        const auto d0 = std::chrono::steady_clock::now();
        double ds = 0;
        do {
          if (plain) dec.DecodeDelta(thin.data(), thin_offsets.data(), kept, thin_key.data(), nullptr, count);
          else dec.DecodeDeltaTemporal(thin.data(), thin_offsets.data(), kept, thin_key.data(), period, nullptr, count);
          ++rounds;
          ds = std::chrono::duration<double>(std::chrono::steady_clock::now() - d0).count();
        } while (ds < 0.5 && rounds < 64);
        std::printf("  every %u%s frame (%u of %u, %.0f stream bytes per kept frame): %s at period %u, %.0f frames/s PCIe-inclusive, %u failed\n", every,
                    every == 1 ? "" : (every == 2 ? "nd" : "th"), kept, stored, (double)thin.size() / kept,
                    plain ? "DecodeDelta" : "DecodeDeltaTemporal", period, shown / ds, failed);
      }
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
