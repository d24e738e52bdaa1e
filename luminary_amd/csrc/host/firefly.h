// Firefly rejection: median-of-means buckets and their Gini-trimmed resolve (lum_core.h lumc_set_firefly_buckets / lumc_firefly_resolve; DESIGN.md section 15;
// Buisine et al., "Firefly Removal in Monte Carlo Rendering with Adaptive Median of meaNs"). The ONE definition of the resolved pixel - firefly_resolve_pixel -,
// compiled twice: by the host compiler into firefly.cpp (lumc_firefly_resolve_host: the twin, no HIP in it) and by the device compiler into firefly.hip
// (k_firefly_resolve), both in binary32, one operation at a time, under -ffp-contract=off with IEEE divide, so that both give the same bytes.
//
// Buckets. Sample id s of a pixel is added to bucket s mod K, per channel: bucket planes [K][3][P]. A bucket's sum is sequential in ascending sample id and starts
// from the stored value, exactly as k_accumulate defines first_moment, so bucket b holds the bits of the first_moment of a render of the ids b, b + K, ... alone.
// counts[b] is the number of ids bucket b has taken - the same for every pixel, so the host keeps it.
//
// Resolve, per pixel, in place on a planar image [3][P]:
//   1. every bucket with counts[b] > 0 has mean_b = B_b / (float) counts[b] per channel; m such buckets.
//   2. a bucket is finite if its three means are; F the set of finite buckets, m' = |F|.
//   3. key_b = max(luminance(mean_b), 0): dev_math.h's luminance, restated below with its coefficients and its order, (a r + b g) + c b. The maximum is written
//      as a comparison (key > 0 ? key : 0), which gives fmaxf's value for every input and leaves no choice between the two zeros.
//   4. rank_b = the number of j in F with key_j < key_b, or key_j == key_b and j < b. No sort and no dynamically indexed array: the K^2 comparisons unroll.
//   5. num = sum (float) (rank_b + 1) * key_b, den = sum key_b, both over F in ascending bucket index, from 0.
//   6. m' >= 4 and den > 0: G = saturate(2 num / ((float) m' den) - (float) (m' + 1) / (float) m') - the Gini coefficient of the keys with 1-based ranks -,
//      c = (uint32_t) (G (float) (m' >> 1)); otherwise c = 0. In real numbers G <= (m' - 1) / m', so c <= (m' >> 1) - 1 and two buckets at least are kept; c is
//      held to that bound, which matters only where num overflows beside a finite den. saturate is written as comparisons too (a NaN gives 0, as fminf(fmaxf()) does).
//   7. c == 0 and m' == m: the pixel is not written.
//   8. otherwise out = (sum of mean_b over F in ascending bucket index with c <= rank_b < m' - c, from 0) / (float) (m' - 2 c), per channel.
//   9. m' == 0 (and m > 0): out = 0.
// Whole buckets are ordered by luminance and trimmed as one: the three channels of an output come from the same buckets, so the pixel keeps its hue (the paper
// trims per channel).
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define LUM_FIREFLY_FN __host__ __device__ __forceinline__
#define LUM_FIREFLY_UNROLL _Pragma("unroll")
#else
#define LUM_FIREFLY_FN inline
#define LUM_FIREFLY_UNROLL
#endif

namespace lum {

constexpr uint32_t kFireflyMinBuckets = 4, kFireflyMaxBuckets = 16;

// what the resolve did to a pixel
struct FireflyPixel {
  uint32_t written;    // steps 8 / 9 applied: out holds the pixel's new value
  uint32_t trimmed;    // buckets left out of the mean: 2 c
  uint32_t nonfinite;  // the pixel has a bucket whose mean is not finite
};

LUM_FIREFLY_FN bool firefly_finite(float f) { uint32_t u; memcpy(&u, &f, 4); return (u & 0x7F800000u) != 0x7F800000u; }

// dev_math.h luminance, operation for operation
LUM_FIREFLY_FN float firefly_luminance(float r, float g, float b) {
  const float tr = 0.212655f * r;
  const float tg = 0.715158f * g;
  const float tb = 0.072187f * b;
  const float s = tr + tg;
  return s + tb;
}

struct FireflyCounts { uint32_t n[kFireflyMaxBuckets]; };

// One pixel. sum(b, channel): the pixel's bucket sums. out is written only where the returned record says so.
template <uint32_t K, typename SumOf>
LUM_FIREFLY_FN FireflyPixel firefly_resolve_pixel(SumOf sum, const FireflyCounts& counts, float out[3]) {
  static_assert(K >= kFireflyMinBuckets && K <= kFireflyMaxBuckets, "4 ... 16 buckets");
  float mr[K], mg[K], mb[K], key[K];
  uint32_t used = 0, finite = 0, m = 0, mf = 0;  // bit b: bucket b has samples / is finite
  LUM_FIREFLY_UNROLL
  for (uint32_t b = 0; b < K; b++) {
    mr[b] = 0.0f; mg[b] = 0.0f; mb[b] = 0.0f; key[b] = 0.0f;
    if (counts.n[b] == 0) continue;
    used |= 1u << b; m++;
    const float n = (float) counts.n[b];
    mr[b] = sum(b, 0u) / n; mg[b] = sum(b, 1u) / n; mb[b] = sum(b, 2u) / n;
    if (!(firefly_finite(mr[b]) && firefly_finite(mg[b]) && firefly_finite(mb[b]))) continue;
    finite |= 1u << b; mf++;
    const float l = firefly_luminance(mr[b], mg[b], mb[b]);
    key[b] = l > 0.0f ? l : 0.0f;
  }
  FireflyPixel px = {0u, 0u, mf != m ? 1u : 0u};
  uint32_t rank[K];
  float num = 0.0f, den = 0.0f;
  LUM_FIREFLY_UNROLL
  for (uint32_t b = 0; b < K; b++) {
    uint32_t r = 0;
    LUM_FIREFLY_UNROLL
    for (uint32_t j = 0; j < K; j++) {
      if (j == b) continue;
      const bool before = key[j] < key[b] || (key[j] == key[b] && j < b);
      r += ((finite >> j) & 1u) && before ? 1u : 0u;
    }
    rank[b] = r;
    if ((finite >> b) & 1u) {
      const float w = (float) (r + 1u);
      const float t = w * key[b];
      num = num + t;
      den = den + key[b];
    }
  }
  uint32_t c = 0;
  if (mf >= 4u && den > 0.0f) {
    const float fm = (float) mf;
    const float t1 = 2.0f * num;
    const float t2 = fm * den;
    const float q = t1 / t2;
    const float r = (float) (mf + 1u) / fm;
    const float d = q - r;
    const float G = d > 0.0f ? (d < 1.0f ? d : 1.0f) : 0.0f;
    const float h = (float) (mf >> 1);
    const float gc = G * h;
    c = (uint32_t) gc;
    if (c > (mf >> 1) - 1u) c = (mf >> 1) - 1u;
  }
  if (c == 0u && mf == m) return px;
  px.written = 1u; px.trimmed = 2u * c;
  if (mf == 0u) { out[0] = 0.0f; out[1] = 0.0f; out[2] = 0.0f; return px; }
  float sr = 0.0f, sg = 0.0f, sb = 0.0f;
  LUM_FIREFLY_UNROLL
  for (uint32_t b = 0; b < K; b++) {
    if (((finite >> b) & 1u) && rank[b] >= c && rank[b] < mf - c) { sr = sr + mr[b]; sg = sg + mg[b]; sb = sb + mb[b]; }
  }
  const float kept = (float) (mf - 2u * c);
  out[0] = sr / kept; out[1] = sg / kept; out[2] = sb / kept;
  return px;
}

// firefly_resolve_pixel<K> for a K known at run time (4 ... 16; the caller checked)
template <typename SumOf>
LUM_FIREFLY_FN FireflyPixel firefly_resolve_pixel_k(uint32_t K, SumOf sum, const FireflyCounts& counts, float out[3]) {
  switch (K) {
    case 4: return firefly_resolve_pixel<4>(sum, counts, out);
    case 5: return firefly_resolve_pixel<5>(sum, counts, out);
    case 6: return firefly_resolve_pixel<6>(sum, counts, out);
    case 7: return firefly_resolve_pixel<7>(sum, counts, out);
    case 8: return firefly_resolve_pixel<8>(sum, counts, out);
    case 9: return firefly_resolve_pixel<9>(sum, counts, out);
    case 10: return firefly_resolve_pixel<10>(sum, counts, out);
    case 11: return firefly_resolve_pixel<11>(sum, counts, out);
    case 12: return firefly_resolve_pixel<12>(sum, counts, out);
    case 13: return firefly_resolve_pixel<13>(sum, counts, out);
    case 14: return firefly_resolve_pixel<14>(sum, counts, out);
    case 15: return firefly_resolve_pixel<15>(sum, counts, out);
    default: return firefly_resolve_pixel<16>(sum, counts, out);
  }
}

}  // namespace lum

#if defined(__HIP_PLATFORM_AMD__) && !defined(LUM_FIREFLY_HOST_ONLY)

#include <hip/hip_runtime_api.h>

#include "device_buffer.h"

#pragma GCC visibility push(hidden)

namespace lum {

// A context's buckets: K * 12 bytes per pixel of its pixel set.
struct FireflyBuckets {
  uint32_t K = 0;                  // 0: off, nothing below is allocated and no kernel of firefly.hip runs
  uint32_t pixels = 0;             // the pixel set the planes were allocated for
  DeviceBuffer<float> planes;      // [K][3][pixels]
  DeviceBuffer<uint32_t> d_stats;  // k_firefly_resolve's three counters
  FireflyCounts counts{};          // ids taken per bucket
  uint64_t resolves = 0;
  bool any() const { for (uint32_t b = 0; b < K; b++) if (counts.n[b]) return true; return false; }
  void take(uint32_t first_sample, uint32_t samples) { for (uint32_t k = 0; k < samples; k++) counts.n[(first_sample + k) % K]++; }
};

// k_bucket_accumulate: a pass's `batch` results per pixel (slot k holds sample id first_sample + k; sample-major results[k * P + p] or pixel-major
// results[p * batch + k]) into the planes. The caller checked that the planes are K * 3 * P floats. Asynchronous, as the two below.
hipError_t firefly_accumulate_launch(const float4* d_results, uint32_t P, uint32_t batch, uint32_t first_sample, uint32_t K, float* d_planes, bool pixel_major, hipStream_t stream);
// k_bucket_accumulate_scatter: result i belongs to frame pixel d_pixels[i] (< frame_pixels, the planes' stride) and is sample id 0: bucket 0.
hipError_t firefly_scatter_launch(const float4* d_results, const uint32_t* d_pixels, uint32_t count, uint32_t frame_pixels, float* d_planes, hipStream_t stream);
// k_firefly_resolve on a planar image [3][P]; d_stats[0 .. 2] += pixels rewritten, buckets trimmed, pixels with a non-finite bucket.
hipError_t firefly_resolve_launch(const float* d_planes, const FireflyCounts& counts, uint32_t K, uint32_t P, float* d_image, uint32_t* d_stats, hipStream_t stream);

}  // namespace lum

#pragma GCC visibility pop
#endif
