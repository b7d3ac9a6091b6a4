// stream_entropy_main.cpp -- a host application written against include/svc/stream_encoder.hpp and stream_decoder.hpp only: encodes
// a clip with the entropy-coded compact output (svc::StreamEncoderConfig::compact + entropy), writes the SVCE stream, and decodes it
// again with svc::StreamDecoder.
//   stream_entropy_main <clip.raw> <w> <h> <frames> <levels> <dct_block> <batch> <seed> <gaze_file|-> <out_prefix> [compact_budget]
// Writes <prefix>.mv / .types / .gm (as stream_levels_main), <prefix>.big (the SVCE frames back to back) and <prefix>.offsets (n + 1
// u64), then <prefix>.display (the decoded display frames at the padded size, u8 B,G,R) and <prefix>.status (u32 per frame).
// gaze_file: one line per frame, "x y" or "-", as stream_decode_main.  out_prefix "-": no files; the clip is encoded, then its SVCE
// stream decoded, again and again for a second each, and both PCIe-inclusive rates printed.  compact_budget (default 0): a byte
// budget, which svc::StreamEncoder refuses together with entropy (the process then fails with its message).
//   stream_entropy_main reuse <clip.raw> <seed> <out_prefix>
// The slot ring at a depth of 4 and ONE decoder across stream kinds (tests/test_gpu_entropy.py): 11 frames of 96 x 64 are encoded
// three ways (compact, compact + entropy, wire; batch 3, depth 4: a short last batch), then one svc::StreamDecoder (depth 4, batch 2,
// wire_batch 3: more batches than slots) decodes SVCQ, wire, SVCE, SVCQ, a gaze on every other frame, and a fresh default-configured
// decoder decodes each stream once.  Writes <prefix>.{q,e,w}.mv / .types and <prefix>.{reuse,fresh}{0..3}.display / .status.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "svc/stream_decoder.hpp"
#include "svc/stream_encoder.hpp"

namespace {

void Dump(const std::string& path, const void* p, size_t bytes) {
  FILE* o = std::fopen(path.c_str(), "wb");
  if (!o || std::fwrite(p, 1, bytes, o) != bytes) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); std::exit(1); }
  std::fclose(o);
}

struct Coded {  // a clip's stream in host memory, whichever kind
  std::vector<uint8_t> bytes;       // SVCQ / SVCE frames back to back, or the wire header and its records
  std::vector<uint64_t> offsets{0};  // compact kinds only
  std::vector<float> mv;
  std::vector<uint32_t> types;
};

Coded EncodeClip(const std::vector<uint8_t>& clip, uint32_t w, uint32_t h, uint32_t n, uint64_t seed, bool entropy, bool wire) {
  svc::StreamEncoderConfig cfg;
  cfg.width = w; cfg.height = h; cfg.levels = 3; cfg.mv_block = 16; cfg.dct_block = 8;
  cfg.batch = 3; cfg.depth = 4; cfg.seed = seed;
  cfg.wire = wire; cfg.compact = !wire; cfg.entropy = entropy;
  svc::StreamEncoder enc(cfg);
  Coded out;
  uint32_t next = 1;
  enc.Encode(clip.data(), n, [&](const svc::EncodedBatch& b) {
    if (b.first_frame != next) { std::fprintf(stderr, "batch out of order: %u, expected %u\n", b.first_frame, next); std::exit(1); }
    next += b.count;
    const size_t blocks = (size_t)b.mv_field_w * b.mv_field_h;
    out.mv.insert(out.mv.end(), b.mv_xy, b.mv_xy + b.count * blocks * 2);
    out.types.insert(out.types.end(), b.block_types, b.block_types + b.count * blocks);
    if (wire) {
      if (b.header) out.bytes.insert(out.bytes.end(), (const uint8_t*)b.header, (const uint8_t*)b.header + sizeof(*b.header));
      out.bytes.insert(out.bytes.end(), b.records, b.records + b.count * b.record_bytes);
    } else {
      const uint64_t base = out.bytes.size();
      out.bytes.insert(out.bytes.end(), b.compact, b.compact + b.compact_bytes);
      for (uint32_t k = 1; k <= b.count; ++k) out.offsets.push_back(base + b.compact_offsets[k]);
    }
  });
  if (next != n) { std::fprintf(stderr, "%u encoded frames, expected %u\n", next - 1, n - 1); std::exit(1); }
  return out;
}

int Reuse(const char* clip_path, uint64_t seed, const std::string& prefix) {
  const uint32_t w = 96, h = 64, n = 11;
  std::vector<uint8_t> clip((size_t)w * h * 3 * n);
  FILE* f = std::fopen(clip_path, "rb");
  if (!f || std::fread(clip.data(), 1, clip.size(), f) != clip.size()) { std::fprintf(stderr, "cannot read %s\n", clip_path); return 1; }
  std::fclose(f);
  const Coded q = EncodeClip(clip, w, h, n, seed, false, false), e = EncodeClip(clip, w, h, n, seed, true, false),
              wr = EncodeClip(clip, w, h, n, seed, false, true);
  for (const auto& kv : {std::make_pair(".q", &q), std::make_pair(".e", &e), std::make_pair(".w", &wr)}) {
    Dump(prefix + kv.first + ".mv", kv.second->mv.data(), kv.second->mv.size() * sizeof(float));
    Dump(prefix + kv.first + ".types", kv.second->types.data(), kv.second->types.size() * sizeof(uint32_t));
  }
  const svc::StreamDecoder::Gaze gaze = [&](uint32_t i, uint32_t* x, uint32_t* y) {
    if (i % 2) return false;
    *x = (37 * i + 5) % w; *y = (23 * i + 3) % h;
    return true;
  };
  const Coded* order[4] = {&q, &wr, &e, &q};
  auto decode = [&](svc::StreamDecoder& dec, int k, const std::string& name) {
    std::vector<uint8_t> display;
    std::vector<uint32_t> status;
    uint32_t dnext = 0;
    auto sink = [&](const svc::DecodedBatch& b) {
      if (b.first_frame != dnext) { std::fprintf(stderr, "decoded batch out of order: %u, expected %u\n", b.first_frame, dnext); std::exit(1); }
      dnext += b.count;
      display.insert(display.end(), b.bgr, b.bgr + (size_t)b.count * b.width * b.height * 3);
      status.insert(status.end(), b.status, b.status + b.count);
    };
    if (order[k] == &wr) dec.DecodeWire(wr.bytes.data(), wr.bytes.size(), gaze, sink);
    else dec.Decode(order[k]->bytes.data(), order[k]->offsets.data(), n - 1, gaze, sink);
    if (dnext != n - 1) { std::fprintf(stderr, "%u decoded frames, expected %u\n", dnext, n - 1); std::exit(1); }
    Dump(prefix + name + std::to_string(k) + ".display", display.data(), display.size());
    Dump(prefix + name + std::to_string(k) + ".status", status.data(), status.size() * sizeof(uint32_t));
  };
  svc::StreamDecoderConfig dcfg;
  dcfg.depth = 4; dcfg.batch = 2; dcfg.wire_batch = 3;
  svc::StreamDecoder reused(dcfg);
  for (int k = 0; k < 4; ++k) {
    decode(reused, k, ".reuse");
    svc::StreamDecoder fresh{svc::StreamDecoderConfig{}};
    decode(fresh, k, ".fresh");
  }
  std::printf("%u frames encoded three ways, decoded by one decoder and by fresh ones\n", n - 1);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 5 && std::string(argv[1]) == "reuse") {
    try {
      return Reuse(argv[2], std::strtoull(argv[3], nullptr, 10), argv[4]);
    } catch (const std::exception& e) {
      std::fprintf(stderr, "%s\n", e.what());
      return 1;
    }
  }
  if (argc != 11 && argc != 12) { std::fprintf(stderr, "usage: see the header comment\n"); return 2; }
  const uint32_t w = std::atoi(argv[2]), h = std::atoi(argv[3]), n = std::atoi(argv[4]);
  svc::StreamEncoderConfig cfg;
  cfg.width = w; cfg.height = h;
  cfg.levels = std::atoi(argv[5]);
  cfg.dct_block = std::atoi(argv[6]);
  cfg.batch = std::atoi(argv[7]);
  cfg.seed = std::strtoull(argv[8], nullptr, 10);
  cfg.compact = true;
  cfg.entropy = true;
  if (argc == 12 && std::atoi(argv[11]) != 0) {
    cfg.compact_budget = std::atoi(argv[11]);
    cfg.compact_ladder = {{1, 640}};
  }
  const std::string gaze_path = argv[9], prefix = argv[10];

  std::vector<uint8_t> clip((size_t)w * h * 3 * n);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(clip.data(), 1, clip.size(), f) != clip.size()) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
  std::fclose(f);

  std::vector<int64_t> gx(n, -1), gy(n, -1);
  if (gaze_path != "-") {
    FILE* g = std::fopen(gaze_path.c_str(), "r");
    if (!g) { std::fprintf(stderr, "cannot read %s\n", gaze_path.c_str()); return 1; }
    char line[128];
    for (uint32_t i = 0; i < n && std::fgets(line, sizeof(line), g); ++i) {
      long x, y;
      if (std::sscanf(line, "%ld %ld", &x, &y) == 2) { gx[i] = x; gy[i] = y; }
    }
    std::fclose(g);
  }
  const svc::StreamDecoder::Gaze gaze = [&](uint32_t i, uint32_t* x, uint32_t* y) {
    if (i >= n || gx[i] < 0) return false;
    *x = (uint32_t)gx[i]; *y = (uint32_t)gy[i];
    return true;
  };

  const bool files = prefix != "-";
  FILE *f_mv = nullptr, *f_ty = nullptr, *f_gm = nullptr;
  if (files) {
    f_mv = std::fopen((prefix + ".mv").c_str(), "wb");
    f_ty = std::fopen((prefix + ".types").c_str(), "wb");
    f_gm = std::fopen((prefix + ".gm").c_str(), "wb");
    if (!f_mv || !f_ty || !f_gm) { std::fprintf(stderr, "cannot open outputs under %s\n", prefix.c_str()); return 1; }
  }
  try {
    svc::StreamEncoder enc(cfg);
    std::vector<uint8_t> stream;     // the SVCE frames of the whole clip
    std::vector<uint64_t> offsets{0};
    uint32_t next = 1;
    bool keep = true;
    auto sink = [&](const svc::EncodedBatch& b) {
      if (b.first_frame != next) { std::fprintf(stderr, "batch out of order: %u, expected %u\n", b.first_frame, next); std::exit(1); }
      if (b.coeffs || !b.compact || !b.compact_offsets || b.compact_bytes != b.compact_offsets[b.count]) {
        std::fprintf(stderr, "entropy-coded batch without its stream\n"); std::exit(1);
      }
      next += b.count;
      if (!keep) return;
      const uint64_t base = stream.size();
      stream.insert(stream.end(), b.compact, b.compact + b.compact_bytes);
      for (uint32_t i = 1; i <= b.count; ++i) offsets.push_back(base + b.compact_offsets[i]);
      if (!files) return;
      const size_t blocks = (size_t)b.mv_field_w * b.mv_field_h;
      std::fwrite(b.mv_xy, sizeof(float), b.count * blocks * 2, f_mv);
      std::fwrite(b.block_types, sizeof(uint32_t), b.count * blocks, f_ty);
      std::fwrite(b.global_motion, sizeof(float), b.count * 2, f_gm);
    };
    enc.Encode(clip.data(), n, sink);
    const uint32_t coded = (uint32_t)offsets.size() - 1;
    if (coded != n - 1) { std::fprintf(stderr, "%u encoded frames, expected %u\n", coded, n - 1); return 1; }

    svc::StreamDecoderConfig dcfg;
    dcfg.batch = cfg.batch;
    svc::StreamDecoder dec(dcfg);
    std::vector<uint8_t> display;
    std::vector<uint32_t> status;
    uint32_t dnext = 0;
    bool dkeep = true;
    auto dsink = [&](const svc::DecodedBatch& b) {
      if (b.first_frame != dnext) { std::fprintf(stderr, "decoded batch out of order: %u, expected %u\n", b.first_frame, dnext); std::exit(1); }
      dnext += b.count;
      if (!dkeep) return;
      display.insert(display.end(), b.bgr, b.bgr + (size_t)b.count * b.width * b.height * 3);
      status.insert(status.end(), b.status, b.status + b.count);
    };
    dec.Decode(stream.data(), offsets.data(), coded, gaze, dsink);
    if (dnext != coded) { std::fprintf(stderr, "%u decoded frames, expected %u\n", dnext, coded); return 1; }

    if (files) {
      std::fclose(f_mv); std::fclose(f_ty); std::fclose(f_gm);
      auto dump = [&](const std::string& path, const void* p, size_t bytes) {
        FILE* o = std::fopen(path.c_str(), "wb");
        if (!o || std::fwrite(p, 1, bytes, o) != bytes) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); std::exit(1); }
        std::fclose(o);
      };
      dump(prefix + ".big", stream.data(), stream.size());
      dump(prefix + ".offsets", offsets.data(), offsets.size() * sizeof(uint64_t));
      dump(prefix + ".display", display.data(), display.size());
      dump(prefix + ".status", status.data(), status.size() * sizeof(uint32_t));
      std::printf("%u frames encoded to %llu B of SVCE and decoded\n", coded, (unsigned long long)stream.size());
      return 0;
    }
    // rates: the clip encoded again and again for a second, then its SVCE stream decoded again and again for a second
    keep = false;
    dkeep = false;
    uint32_t passes = 0, frames = 0;
    uint64_t d2h = 0;
    auto t0 = std::chrono::steady_clock::now();
    double s = 0;
    do {
      next = 1;
      enc.Encode(clip.data(), n, sink);
      d2h += enc.last_stats().d2h_bytes;
      ++passes; frames += n - 1;
      s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    } while (s < 1.0 && passes < 64);
    std::printf("encode: %u frames, %.0f frames/s PCIe-inclusive (compact + entropy), %.0f d2h bytes per frame, %.4f MB of SVCE per frame\n",
                frames, frames / s, (double)d2h / frames, stream.size() / 1e6 / coded);
    passes = 0; frames = 0;
    t0 = std::chrono::steady_clock::now();
    do {
      dnext = 0;
      dec.Decode(stream.data(), offsets.data(), coded, gaze, dsink);
      ++passes; frames += coded;
      s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    } while (s < 1.0 && passes < 256);
    const svc::DecodeStats& e = dec.last_stats();
    std::printf("decode: %u frames, %.0f frames/s PCIe-inclusive (SVCE), last pass per batch: h2d %.3f ms, kernels %.3f ms, d2h %.3f ms\n",
                frames, frames / s, e.h2d_ms / e.batches, e.kernels_ms / e.batches, e.d2h_ms / e.batches);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
