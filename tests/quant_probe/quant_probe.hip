// quant_probe.hip -- TEST ONLY: the fused kernels' quantiser (csrc/quant_core.hpp: quant1_fast, quant2_fast) applied to an array
// of f32, so that tests/test_gpu_transform_exact.py can feed it every float next to every rounding tie.  Inside dct.hip these
// functions are reachable only behind a transform, whose outputs meet a near-tie a few times per million coefficients.
// Built by scalable_video_codec_amd/build.py into tests/quant_probe/libsvc_quant_probe.so with the product's compiler flags;
// not part of libsvc_hip.so, no public header.
#include <cstdlib>

#include "quant_core.hpp"

namespace {

// form 0: quant1_fast; form 1: quant2_fast with c[i] in the pair's even lane; form 2: ... in its odd lane (the other lane holds
// a neighbouring value of the array, so that both lanes carry live data as in the kernels).  Every element has its own step.
__global__ __launch_bounds__(256) void quant_probe_kernel(const float* __restrict__ in, const float* __restrict__ step,
                                                          const float* __restrict__ inv, float* __restrict__ out, uint64_t n, int form) {
  const uint64_t stride = (uint64_t)gridDim.x * 256;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const float c = in[i], other = in[i + 1 < n ? i + 1 : 0];
    float q;
    if (form == 0) q = svc::quant1_fast(c, step[i], inv[i]);
    else if (form == 1) q = svc::quant2_fast(svc::f32x2{c, other}, step[i], inv[i]).x;
    else q = svc::quant2_fast(svc::f32x2{other, c}, step[i], inv[i]).y;
    out[i] = q;
  }
}

}  // namespace

// host pointers in, host pointers out: out[i] = quant(in[i]) with step[i]; 0 or the hipError_t that stopped it
extern "C" int svc_quant_probe(const float* in, const uint32_t* step, float* out, uint64_t n, int form) {
  if (n == 0) return 0;
  if (form < 0 || form > 2) return (int)hipErrorInvalidValue;
  float* h = static_cast<float*>(malloc(2 * n * sizeof(float)));
  if (!h) return (int)hipErrorOutOfMemory;
  for (uint64_t i = 0; i < n; ++i) {
    if (step[i] == 0) { free(h); return (int)hipErrorInvalidValue; }
    h[i] = (float)step[i];      // as launch_dct computes them: the step as f32 and
    h[n + i] = 1.0f / h[i];     // RN(1 / step) on the host
  }
  float* d = nullptr;  // [in | step | inv | out]
  hipError_t e = hipMalloc(&d, 4 * n * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(d, in, n * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d + n, h, 2 * n * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    const uint64_t want = (n + 255) / 256;
    hipLaunchKernelGGL(quant_probe_kernel, dim3((uint32_t)(want < 4096 ? want : 4096)), dim3(256), 0, nullptr, d, d + n, d + 2 * n,
                       d + 3 * n, n, form);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(out, d + 3 * n, n * sizeof(float), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  free(h);
  return (int)e;
}
