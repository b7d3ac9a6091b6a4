// stage_frames.hpp -- how a driver stages a batch of a compact stream (SVCQ or SVCE frames anywhere in host memory, with their
// offsets) into a slot's pinned buffer: shared by stream_decoder.cpp and wire_transcoder.cpp.
#pragma once

#include <algorithm>
#include <cstdint>

#include "copy_crew.hpp"
#include "hip_raii.hpp"

namespace svc {
namespace host __attribute__((visibility("hidden"))) {

// The bytes of frames first .. first + cnt of a stream in host memory -> the slot's pinned buffer, their offsets relative to it:
// from the batch's lowest offset (rounded down to 16: frames stay aligned) to its highest, inside the stream; an offset outside it
// becomes one the kernels refuse (status 1), so a malformed frame is reported, never read past the copy.  -> the bytes staged
inline uint64_t StageFrames(const Who& who, CopyCrew& crew, const uint8_t* stream, const uint64_t* offsets, uint64_t total, uint32_t first,
                            uint32_t cnt, PinBuf<uint8_t>& pin, DevBuf<uint8_t>& dev, uint64_t* pin_off) {
  uint64_t lo = total, hi = 0;
  for (uint32_t i = first; i <= first + cnt; ++i) {
    const uint64_t o = std::min(offsets[i], total);
    lo = std::min(lo, o); hi = std::max(hi, o);
  }
  lo &= ~(uint64_t)15;
  const uint64_t bytes = hi - lo;
  if (pin.n < std::max<uint64_t>(bytes, 16)) {  // grown on demand: a batch of 1080p frames is about 17 MB
    const size_t cap = (size_t)(bytes + bytes / 4 + 4095) & ~(size_t)4095;
    pin.Alloc(who, cap); dev.Alloc(who, cap);
  }
  crew.Copy(pin.p, stream + lo, bytes);
  for (uint32_t i = 0; i <= cnt; ++i) {
    const uint64_t o = offsets[first + i];
    pin_off[i] = o <= total ? o - lo : ~(uint64_t)15;
  }
  return bytes;
}

}  // namespace host
}  // namespace svc
