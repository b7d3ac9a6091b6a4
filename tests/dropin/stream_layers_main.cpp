// stream_layers_main.cpp -- a host application written against include/svc/stream_encoder.hpp and stream_decoder.hpp only: encodes
// a clip as two layers (svc::StreamEncoderConfig::compact + enh_step: a base stream and its enhancement stream, optionally entropy
// coded), writes both, and decodes them again with svc::StreamDecoder::DecodeLayers.
//   stream_layers_main <clip.raw> <w> <h> <frames> <levels> <dct_block> <batch> <depth> <seed> <fg> <bg> <enh> <entropy 0|1>
//                      <window_file|-> <gaze_file|-> <out_prefix> [compact_budget]
// dct_block: one side, or WxH (non-square: dct_block_h).  window_file: one line per frame of the clip, "x y w h" (the frame's window
// in padded coordinates) or "-" (an empty window); "-": no callback, every tile is enhanced.  gaze_file: one line per frame, "x y" or
// "-", as stream_decode_main; "-": no gaze.  Writes <prefix>.base, .base.offsets, .enh, .enh.offsets (n + 1 u64 each), .types, .mv,
// .gm, then <prefix>.display (the display frames at the padded size, u8 B,G,R) and <prefix>.status (u32 per frame) from DecodeLayers on
// what it just encoded.  out_prefix "-": no files; the clip is encoded, then its two streams decoded, again and again for a second
// each, and both PCIe-inclusive rates printed.  compact_budget (default 0): a byte budget, which svc::StreamEncoder refuses together
// with enh_step (the process then fails with its message).
//   stream_layers_main decode <in_prefix> <frames> <batch> <depth> <gaze_file|-> <out_prefix>
// DecodeLayers alone, on <in_prefix>.base / .base.offsets / .enh / .enh.offsets as they are on disk: <out_prefix>.display / .status.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "svc/stream_decoder.hpp"
#include "svc/stream_encoder.hpp"

namespace {

void Dump(const std::string& path, const void* p, size_t bytes) {
  FILE* o = std::fopen(path.c_str(), "wb");
  if (!o || std::fwrite(p, 1, bytes, o) != bytes) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); std::exit(1); }
  std::fclose(o);
}

bool ReadFile(const std::string& path, std::vector<uint8_t>* out) {
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

// one line per frame: `fields` numbers, or anything else = none (row[0] < 0)
std::vector<std::vector<int64_t>> ReadRows(const std::string& path, uint32_t n, int fields) {
  std::vector<std::vector<int64_t>> rows(n, std::vector<int64_t>(4, -1));
  FILE* f = std::fopen(path.c_str(), "r");
  if (!f) { std::fprintf(stderr, "cannot read %s\n", path.c_str()); std::exit(1); }
  char line[128];
  for (uint32_t i = 0; i < n && std::fgets(line, sizeof(line), f); ++i) {
    long long v[4] = {-1, -1, -1, -1};
    if (std::sscanf(line, "%lld %lld %lld %lld", &v[0], &v[1], &v[2], &v[3]) >= fields)
      for (int k = 0; k < 4; ++k) rows[i][k] = v[k];
  }
  std::fclose(f);
  return rows;
}

svc::StreamDecoder::Gaze GazeOf(const std::string& path, uint32_t n) {
  if (path == "-") return {};
  const std::vector<std::vector<int64_t>> rows = ReadRows(path, n, 2);
  return [rows, n](uint32_t i, uint32_t* x, uint32_t* y) {
    if (i >= n || rows[i][0] < 0) return false;
    *x = (uint32_t)rows[i][0]; *y = (uint32_t)rows[i][1];
    return true;
  };
}

struct Layers {  // a clip's two streams in host memory
  std::vector<uint8_t> base, enh;
  std::vector<uint64_t> base_offsets{0}, enh_offsets{0};
};

struct Decoded {
  std::vector<uint8_t> display;
  std::vector<uint32_t> status;
};

// DecodeLayers on the two streams; keep = false: the frames are counted only
uint32_t DecodeClip(svc::StreamDecoder& dec, const Layers& l, uint32_t frames, const svc::StreamDecoder::Gaze& gaze, Decoded* keep) {
  uint32_t next = 0;
  dec.DecodeLayers(l.base.data(), l.base_offsets.data(), l.enh.data(), l.enh_offsets.data(), frames, gaze, [&](const svc::DecodedBatch& b) {
    if (b.first_frame != next) { std::fprintf(stderr, "decoded batch out of order: %u, expected %u\n", b.first_frame, next); std::exit(1); }
    next += b.count;
    if (!keep) return;
    keep->display.insert(keep->display.end(), b.bgr, b.bgr + (size_t)b.count * b.width * b.height * 3);
    keep->status.insert(keep->status.end(), b.status, b.status + b.count);
  });
  if (next != frames) { std::fprintf(stderr, "%u decoded frames, expected %u\n", next, frames); std::exit(1); }
  return next;
}

int DecodeOnly(char** argv) {
  const std::string in = argv[2], out = argv[7];
  const uint32_t n = std::atoi(argv[3]);
  svc::StreamDecoderConfig dcfg;
  dcfg.batch = std::atoi(argv[4]);
  dcfg.depth = std::atoi(argv[5]);
  Layers l;
  std::vector<uint8_t> bo, eo;
  if (!ReadFile(in + ".base", &l.base) || !ReadFile(in + ".base.offsets", &bo) || !ReadFile(in + ".enh", &l.enh) ||
      !ReadFile(in + ".enh.offsets", &eo) || n == 0 || bo.size() < 8 * ((size_t)n + 1) || eo.size() < 8 * ((size_t)n + 1)) {
    std::fprintf(stderr, "cannot read %u frames of %s.base / .enh and their offsets\n", n, in.c_str());
    return 1;
  }
  l.base_offsets.resize(n + 1); l.enh_offsets.resize(n + 1);
  std::memcpy(l.base_offsets.data(), bo.data(), 8 * ((size_t)n + 1));
  std::memcpy(l.enh_offsets.data(), eo.data(), 8 * ((size_t)n + 1));
  svc::StreamDecoder dec(dcfg);
  Decoded d;
  DecodeClip(dec, l, n, GazeOf(argv[6], n), &d);
  Dump(out + ".display", d.display.data(), d.display.size());
  Dump(out + ".status", d.status.data(), d.status.size() * sizeof(uint32_t));
  std::printf("%u frames of two layers decoded\n", n);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  try {
    if (argc == 8 && std::string(argv[1]) == "decode") return DecodeOnly(argv);
    if (argc != 17 && argc != 18) { std::fprintf(stderr, "usage: see the header comment\n"); return 2; }
    const uint32_t w = std::atoi(argv[2]), h = std::atoi(argv[3]), n = std::atoi(argv[4]);
    svc::StreamEncoderConfig cfg;
    cfg.width = w; cfg.height = h;
    cfg.levels = std::atoi(argv[5]);
    unsigned tw = 0, th = 0;
    if (std::sscanf(argv[6], "%ux%u", &tw, &th) == 2) { cfg.dct_block = tw; cfg.dct_block_h = th; }
    else cfg.dct_block = std::atoi(argv[6]);
    cfg.batch = std::atoi(argv[7]);
    cfg.depth = std::atoi(argv[8]);
    cfg.seed = std::strtoull(argv[9], nullptr, 10);
    cfg.fg_step = std::atoi(argv[10]);
    cfg.bg_step = std::atoi(argv[11]);
    cfg.enh_step = std::atoi(argv[12]);
    cfg.compact = true;
    cfg.entropy = std::atoi(argv[13]) != 0;
    if (argc == 18 && std::atoi(argv[17]) != 0) {
      cfg.compact_budget = std::atoi(argv[17]);
      cfg.compact_ladder = {{cfg.fg_step, cfg.bg_step}};
    }
    const std::string window_path = argv[14], gaze_path = argv[15], prefix = argv[16];

    std::vector<uint8_t> clip((size_t)w * h * 3 * n);
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(clip.data(), 1, clip.size(), f) != clip.size()) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
    std::fclose(f);

    uint32_t asked = 0;  // the window callback's calls: once per encoded frame, in clip order
    if (window_path != "-") {
      const std::vector<std::vector<int64_t>> rows = ReadRows(window_path, n, 4);
      cfg.enh_window = [rows, n, &asked](uint32_t frame, uint32_t xywh[4]) {
        if (frame != asked % (n - 1) + 1) { std::fprintf(stderr, "window asked for frame %u, expected %u\n", frame, asked % (n - 1) + 1); std::exit(1); }
        ++asked;
        if (frame >= n || rows[frame][0] < 0) return false;
        for (int k = 0; k < 4; ++k) xywh[k] = (uint32_t)rows[frame][k];
        return true;
      };
    }
    const svc::StreamDecoder::Gaze gaze = GazeOf(gaze_path, n);

    svc::StreamEncoder enc(cfg);
    Layers l;
    std::vector<float> mv, gm;
    std::vector<uint32_t> types;
    uint32_t next = 1;
    bool keep = true;
    auto sink = [&](const svc::EncodedBatch& b) {
      if (b.first_frame != next) { std::fprintf(stderr, "batch out of order: %u, expected %u\n", b.first_frame, next); std::exit(1); }
      if (b.coeffs || !b.compact || !b.compact_offsets || b.compact_bytes != b.compact_offsets[b.count] || !b.enhancement ||
          !b.enhancement_offsets || b.enhancement_bytes != b.enhancement_offsets[b.count]) {
        std::fprintf(stderr, "layered batch without its two streams\n"); std::exit(1);
      }
      next += b.count;
      if (!keep) return;
      const uint64_t base0 = l.base.size(), enh0 = l.enh.size();
      l.base.insert(l.base.end(), b.compact, b.compact + b.compact_bytes);
      l.enh.insert(l.enh.end(), b.enhancement, b.enhancement + b.enhancement_bytes);
      for (uint32_t i = 1; i <= b.count; ++i) {
        l.base_offsets.push_back(base0 + b.compact_offsets[i]);
        l.enh_offsets.push_back(enh0 + b.enhancement_offsets[i]);
      }
      const size_t blocks = (size_t)b.mv_field_w * b.mv_field_h;
      mv.insert(mv.end(), b.mv_xy, b.mv_xy + b.count * blocks * 2);
      types.insert(types.end(), b.block_types, b.block_types + b.count * blocks);
      gm.insert(gm.end(), b.global_motion, b.global_motion + b.count * 2);
    };
    enc.Encode(clip.data(), n, sink);
    const uint32_t coded = (uint32_t)l.base_offsets.size() - 1;
    if (coded != n - 1) { std::fprintf(stderr, "%u encoded frames, expected %u\n", coded, n - 1); return 1; }
    if (cfg.enh_window && asked != coded) { std::fprintf(stderr, "%u window calls for %u frames\n", asked, coded); return 1; }

    const bool files = prefix != "-";
    if (files) {  // the encoder's outputs first: they stand whatever the decoder says of the geometry
      Dump(prefix + ".base", l.base.data(), l.base.size());
      Dump(prefix + ".base.offsets", l.base_offsets.data(), l.base_offsets.size() * sizeof(uint64_t));
      Dump(prefix + ".enh", l.enh.data(), l.enh.size());
      Dump(prefix + ".enh.offsets", l.enh_offsets.data(), l.enh_offsets.size() * sizeof(uint64_t));
      Dump(prefix + ".types", types.data(), types.size() * sizeof(uint32_t));
      Dump(prefix + ".mv", mv.data(), mv.size() * sizeof(float));
      Dump(prefix + ".gm", gm.data(), gm.size() * sizeof(float));
    }

    svc::StreamDecoderConfig dcfg;
    dcfg.batch = cfg.batch;
    dcfg.depth = cfg.depth;
    svc::StreamDecoder dec(dcfg);
    Decoded d;
    DecodeClip(dec, l, coded, gaze, &d);
    if (files) {
      Dump(prefix + ".display", d.display.data(), d.display.size());
      Dump(prefix + ".status", d.status.data(), d.status.size() * sizeof(uint32_t));
      std::printf("%u frames encoded to %llu B of base and %llu B of enhancement, and decoded\n", coded, (unsigned long long)l.base.size(),
                  (unsigned long long)l.enh.size());
      return 0;
    }
    // rates: the clip encoded again and again for a second, then its two streams decoded again and again for a second
    keep = false;
    uint32_t passes = 0, frames = 0;
    svc::EncodeStats es;
    auto t0 = std::chrono::steady_clock::now();
    double s = 0;
    do {
      next = 1;
      enc.Encode(clip.data(), n, sink);
      const svc::EncodeStats& e = enc.last_stats();
      es.batches += e.batches; es.h2d_ms += e.h2d_ms; es.kernels_ms += e.kernels_ms; es.d2h_ms += e.d2h_ms; es.d2h_bytes += e.d2h_bytes;
      ++passes; frames += n - 1;
      s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    } while (s < 1.0 && passes < 64);
    std::printf("encode: %u frames, %.0f frames/s PCIe-inclusive (two layers%s), per batch: h2d %.3f ms, kernels %.3f ms, d2h %.3f ms, "
                "%.0f d2h bytes per frame, %.4f MB of base and %.4f MB of enhancement per frame\n",
                frames, frames / s, cfg.entropy ? ", entropy" : "", es.h2d_ms / es.batches, es.kernels_ms / es.batches, es.d2h_ms / es.batches,
                (double)es.d2h_bytes / frames, l.base.size() / 1e6 / coded, l.enh.size() / 1e6 / coded);
    passes = 0; frames = 0;
    svc::DecodeStats ds;
    t0 = std::chrono::steady_clock::now();
    do {
      frames += DecodeClip(dec, l, coded, gaze, nullptr);
      const svc::DecodeStats& e = dec.last_stats();
      ds.batches += e.batches; ds.h2d_ms += e.h2d_ms; ds.kernels_ms += e.kernels_ms; ds.d2h_ms += e.d2h_ms;
      ++passes;
      s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    } while (s < 1.0 && passes < 256);
    std::printf("decode: %u frames, %.0f frames/s PCIe-inclusive (two layers%s), per batch: h2d %.3f ms, kernels %.3f ms, d2h %.3f ms\n",
                frames, frames / s, cfg.entropy ? ", entropy" : "", ds.h2d_ms / ds.batches, ds.kernels_ms / ds.batches, ds.d2h_ms / ds.batches);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}
