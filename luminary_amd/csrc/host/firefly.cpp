// The host twin of k_firefly_resolve (firefly.hip): firefly.h's firefly_resolve_pixel compiled by the host compiler, no HIP in it. It defines the bytes the kernel
// is held to (lum_core.h lumc_firefly_resolve_host; tests/test_firefly.py, tests/test_firefly_gpu.py).
#define LUM_FIREFLY_HOST_ONLY 1
#include "firefly.h"

extern "C" int lumc_firefly_resolve_host(const float* sums, const uint32_t* counts, uint32_t K, uint32_t pixels, float* image_inout, uint32_t stats[3]) {
  if (!sums || !counts || !image_inout) return 1;
  if (K < lum::kFireflyMinBuckets || K > lum::kFireflyMaxBuckets) return 1;
  lum::FireflyCounts n{};
  bool any = false;
  for (uint32_t b = 0; b < K; b++) { n.n[b] = counts[b]; any = any || counts[b] != 0; }
  if (!any) return 1;  // no bucket has samples: nothing to resolve (lumc_firefly_resolve refuses the same)
  const size_t P = pixels;
  uint32_t st[3] = {0, 0, 0};
  for (size_t p = 0; p < P; p++) {
    float out[3];
    const lum::FireflyPixel px = lum::firefly_resolve_pixel_k(K, [&](uint32_t b, uint32_t ch) { return sums[((size_t) b * 3 + ch) * P + p]; }, n, out);
    if (px.written) { image_inout[p] = out[0]; image_inout[P + p] = out[1]; image_inout[2 * P + p] = out[2]; st[0]++; }
    st[1] += px.trimmed; st[2] += px.nonfinite;
  }
  if (stats) { stats[0] = st[0]; stats[1] = st[1]; stats[2] = st[2]; }
  return 0;
}
