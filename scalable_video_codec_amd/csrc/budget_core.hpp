// budget_core.hpp -- what the two rate controls of the compact stream share (levels.hip: the budgeted pack of raw planes; dct_pack.hip: the
// budgeted form of the fused transform): the ladder as the kernels take it, the threshold below which a step quantises to zero, the
// ladder's argument checks and the per-frame choice.  One definition, as dct_core.hpp is for the transform and quant_core.hpp for the
// quantiser.  For the kernel files: svc_common.hpp comes first.
#pragma once

#include <cmath>

#include "svc_common.hpp"

namespace svc {

constexpr uint32_t kMaxLadder = 64;  // one entry per lane of a wave

// The ladder as the kernels take it (by value: 1 KB of kernel arguments, no copy to the device).  tau[c][k] = the smallest f32
// >= step * (0.5 - 2^-26), class c = 0 background, 1 foreground: with a correctly rounded division, level_of(x, step) != 0
// exactly when |x| >= tau (fl(|x| / step) >= 0.5 under round-to-nearest-even, and std::round sends 0.5 away from zero).
struct Ladder {
  uint32_t len;
  uint32_t step[2][kMaxLadder];
  float tau[2][kMaxLadder];
};

// the smallest f32 >= step * (0.5 - 2^-26) = N / 2^26 with N = step * (2^25 - 1) < 2^57, exactly: every candidate is >= 0.25, so
// candidate * 2^26 is an integer below 2^64 and compares with N without rounding
inline float zero_threshold(uint32_t step) {
  const uint64_t n = (uint64_t)step * ((1u << 25) - 1);
  auto ge = [n](float f) { return (uint64_t)((double)f * 67108864.0) >= n; };
  float f = (float)std::ldexp((double)n, -26);
  while (!ge(f)) f = std::nextafter(f, INFINITY);
  while (ge(std::nextafter(f, 0.f))) f = std::nextafter(f, 0.f);
  return f;
}

// the ladder of an entry point `what`: its length, a null pointer, a zero step, a decreasing fg_step or bg_step
inline int validate_ladder(const char* what, const svc_step_pair* ladder, uint32_t ladder_len) {
  SVC_REQUIRE(ladder_len >= 1 && ladder_len <= kMaxLadder, "%s: a ladder of %u entries (1 .. %u)", what, ladder_len, kMaxLadder);
  SVC_REQUIRE(ladder != nullptr, "%s: null ladder", what);
  for (uint32_t k = 0; k < ladder_len; ++k) {
    SVC_REQUIRE(ladder[k].fg_step > 0 && ladder[k].bg_step > 0, "%s: ladder entry %u: quant steps must be positive", what, k);
    SVC_REQUIRE(k == 0 || (ladder[k].fg_step >= ladder[k - 1].fg_step && ladder[k].bg_step >= ladder[k - 1].bg_step),
                "%s: ladder entry %u (%u, %u) is below entry %u (%u, %u): the ladder must be non-decreasing", what, k,
                ladder[k].fg_step, ladder[k].bg_step, k - 1, ladder[k - 1].fg_step, ladder[k - 1].bg_step);
  }
  return SVC_OK;
}

inline Ladder make_ladder(const svc_step_pair* ladder, uint32_t ladder_len) {
  Ladder lad{};
  lad.len = ladder_len;
  for (uint32_t k = 0; k < ladder_len; ++k) {
    lad.step[0][k] = ladder[k].bg_step; lad.step[1][k] = ladder[k].fg_step;
    lad.tau[0][k] = zero_threshold(ladder[k].bg_step); lad.tau[1][k] = zero_threshold(ladder[k].fg_step);
  }
  return lad;
}

// A frame's choice from its sizes fb[k] = bytes_k: the smallest k with bytes_k <= budget, else the last entry with bit 31 set.
__device__ __forceinline__ uint32_t budget_choice(const uint64_t* __restrict__ fb, uint32_t len, uint64_t b) {
  uint32_t k = 0;
  while (k < len && fb[k] > b) ++k;
  const uint32_t pick = k < len ? k : len - 1;
  return k < len ? k : (pick | 0x80000000u);
}

}  // namespace svc
