// Firefly rejection on the device (lumc_set_firefly_buckets, lumc_firefly_resolve): a pass's results folded into K per-pixel buckets by
// sample id, and the Gini-trimmed mean of the bucket means written over a result image. The arithmetic of the resolve is firefly.h's firefly_resolve_pixel, the
// same source the host twin (firefly.cpp) is compiled from; this unit is compiled without contraction like that one, with IEEE divide: both give the same bytes
// (lumc_firefly_resolve_host, tests/test_firefly_gpu.py). Streaming kernels beside k_accumulate and k_generate_result; none of those is touched.
//
//   k_bucket_accumulate          one thread per pixel, grid-stride. Slot k of a pass holds sample id first + k, which belongs to bucket (first + k) mod K; a
//                                bucket's sum starts from the stored value and takes its ids in ascending order, one float add after the other (k_accumulate's
//                                definition of first_moment). Planes [K][3][P]: consecutive lanes touch consecutive pixels in every plane.
//                                sample-major slots (results[k * P + p]): a lane walks bucket after bucket - load the three sums, add the slots k0, k0 + K, ...,
//                                store -, every result is read once, 16 bytes per lane and contiguous over the wave. No LDS.
//                                pixel-major slots (results[p * batch + k]): a pixel's row is contiguous, the pixels of a wave lie batch x 16 bytes apart. A wave
//                                brings tiles of 64 pixels x 8 slots through LDS in memory order (the shape of k_accumulate's pixel-major path, with its swizzle)
//                                and adds them in slot order to bucket sums that sit in LDS as [bucket][channel][thread] - the bucket of a slot is the same in
//                                every lane, so the index is an address, not a register number. Planes are read and written once per pass.
//   k_bucket_accumulate_scatter  the undersampling preview's first sample: result i is sample id 0 of frame pixel pixels[i], bucket 0.
//   k_firefly_resolve<K>         one thread per pixel, the K^2 comparisons unrolled, no per-thread array that is indexed at run time. 3 K floats read, 3 written
//                                where the definition rewrites the pixel. Three counters, each reduced across the wave and added with one atomic per wave.
#include <hip/hip_runtime.h>

#include "../../../include/lum_core.h"
#include "firefly.h"

namespace lum {
namespace {

constexpr uint32_t kFireflyBlock = 256;
constexpr uint32_t kFireflyMaxGrid = 2048;  // 256 CUs x 8 resident workgroups, grid-stride beyond that (context.h grid_for)
constexpr uint32_t kBucketTile = 8;         // slots per tile row: 8 x 16 = 128 contiguous bytes
// the pixel-major form runs in workgroups of 128: tile 16 KB + sums 3 K x 512 B = 40 KB at K = 16, within the 64 KB every launch may ask for, four workgroups per CU
constexpr uint32_t kBucketPixelMajorBlock = 128;

inline uint32_t firefly_grid(uint32_t n) {
  const uint32_t blocks = (n + kFireflyBlock - 1) / kFireflyBlock;
  return blocks < 1 ? 1 : (blocks > kFireflyMaxGrid ? kFireflyMaxGrid : blocks);
}
inline size_t bucket_lds_bytes(uint32_t K) { return sizeof(float4) * kBucketPixelMajorBlock * kBucketTile + sizeof(float) * 3u * K * kBucketPixelMajorBlock; }

// phase = first_sample mod K: the bucket of slot 0
__device__ __forceinline__ void bucket_accumulate_pixel_major(const float4* __restrict__ results, uint32_t P, uint32_t batch, uint32_t phase, uint32_t K, float* planes, float4* lds) {
  static_assert(kBucketTile == 8u, "the swizzle and the shifts below are written for rows of eight");
  const uint32_t lane = threadIdx.x & 63u, T = blockDim.x;  // T: kBucketPixelMajorBlock
  float4* tile = lds + (threadIdx.x >> 6) * (64u * kBucketTile);
  float* sums = reinterpret_cast<float*>(lds + T * kBucketTile) + threadIdx.x;  // [bucket * 3 + channel][thread]: this thread's column
  const uint32_t touched = batch < K ? batch : K;  // the buckets phase, phase + 1, ... (mod K) get a slot
  const uint32_t rounds = (P + gridDim.x * T - 1u) / (gridDim.x * T);  // whole workgroups go round together: the barriers below
  for (uint32_t round = 0; round < rounds; round++) {
    const uint32_t p = (round * gridDim.x + blockIdx.x) * T + threadIdx.x;
    const uint32_t p0 = p - lane;  // the wave's first pixel
    const bool active = p < P;
    if (active) {
      for (uint32_t i = 0, b = phase; i < touched; i++, b = (b + 1u == K) ? 0u : b + 1u)
        for (uint32_t ch = 0; ch < 3u; ch++) sums[(b * 3u + ch) * T] = planes[(size_t) (b * 3u + ch) * P + p];
    }
    uint32_t b = phase;
    for (uint32_t k0 = 0; k0 < batch; k0 += kBucketTile) {
      const uint32_t kc = min(kBucketTile, batch - k0);
#pragma unroll
      for (uint32_t j = 0; j < kBucketTile; j++) {
        const uint32_t e = j * 64u + lane, row = e >> 3, at = e & 7u;
        if (p0 + row < P && at < kc) tile[row * kBucketTile + (at ^ (row & 7u))] = results[(size_t) (p0 + row) * batch + k0 + at];
      }
      __syncthreads();
      for (uint32_t k = 0; k < kc; k++) {  // (b advances in every lane alike: it stays uniform whether or not the lane has a pixel)
        if (active) {
          const float4 v = tile[lane * kBucketTile + (k ^ (lane & 7u))];
          float* s = sums + b * 3u * T;
          s[0] += v.x; s[T] += v.y; s[2u * T] += v.z;
        }
        b = (b + 1u == K) ? 0u : b + 1u;
      }
      __syncthreads();
    }
    if (active) {
      for (uint32_t i = 0, w = phase; i < touched; i++, w = (w + 1u == K) ? 0u : w + 1u)
        for (uint32_t ch = 0; ch < 3u; ch++) planes[(size_t) (w * 3u + ch) * P + p] = sums[(w * 3u + ch) * T];
    }
  }
}

// pixel_major: the order of the result slots; with it the launch has kBucketPixelMajorBlock threads per workgroup and brings bucket_lds_bytes(K) of dynamic LDS
__global__ __launch_bounds__(kFireflyBlock) void k_bucket_accumulate(const float4* __restrict__ results, uint32_t P, uint32_t batch, uint32_t phase, uint32_t K, float* planes,
                                                                     uint32_t pixel_major) {
  extern __shared__ __attribute__((aligned(16))) float4 bucket_lds[];
  if (pixel_major) { bucket_accumulate_pixel_major(results, P, batch, phase, K, planes, bucket_lds); return; }
  const uint32_t touched = batch < K ? batch : K;
  for (uint32_t p = blockIdx.x * kFireflyBlock + threadIdx.x; p < P; p += gridDim.x * kFireflyBlock) {
    for (uint32_t k0 = 0, b = phase; k0 < touched; k0++, b = (b + 1u == K) ? 0u : b + 1u) {
      float* plane = planes + (size_t) b * 3u * P + p;
      float r = plane[0], g = plane[P], bl = plane[2 * (size_t) P];
      for (uint32_t k = k0; k < batch; k += K) {
        const float4 v = results[(size_t) k * P + p];
        r += v.x; g += v.y; bl += v.z;
      }
      plane[0] = r; plane[P] = g; plane[2 * (size_t) P] = bl;
    }
  }
}

__global__ __launch_bounds__(kFireflyBlock) void k_bucket_accumulate_scatter(const float4* __restrict__ results, const uint32_t* __restrict__ pixels, uint32_t count,
                                                                             uint32_t frame_pixels, float* planes) {
  for (uint32_t i = blockIdx.x * kFireflyBlock + threadIdx.x; i < count; i += gridDim.x * kFireflyBlock) {
    const uint32_t index = pixels[i];
    if (index >= frame_pixels) continue;
    const float4 v = results[i];
    planes[index] += v.x; planes[(size_t) frame_pixels + index] += v.y; planes[2 * (size_t) frame_pixels + index] += v.z;
  }
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (uint32_t d = 32u; d > 0u; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

template <uint32_t K>
__global__ __launch_bounds__(kFireflyBlock) void k_firefly_resolve(const float* __restrict__ planes, FireflyCounts counts, uint32_t P, float* image, uint32_t* stats) {
  const uint32_t p = blockIdx.x * kFireflyBlock + threadIdx.x;  // the grid covers the pixels; every lane stays for the wave's sums
  FireflyPixel px = {0u, 0u, 0u};
  if (p < P) {
    float out[3];
    px = firefly_resolve_pixel<K>([&](uint32_t b, uint32_t ch) { return planes[(size_t) (b * 3u + ch) * P + p]; }, counts, out);
    if (px.written) { image[p] = out[0]; image[(size_t) P + p] = out[1]; image[2 * (size_t) P + p] = out[2]; }
  }
  const uint32_t written = wave_sum(px.written), trimmed = wave_sum(px.trimmed), nonfinite = wave_sum(px.nonfinite);
  if ((threadIdx.x & 63u) == 0u) {
    if (written) atomicAdd(stats + 0, written);
    if (trimmed) atomicAdd(stats + 1, trimmed);
    if (nonfinite) atomicAdd(stats + 2, nonfinite);
  }
}

template <uint32_t K>
void resolve_launch(const float* d_planes, const FireflyCounts& counts, uint32_t P, float* d_image, uint32_t* d_stats, hipStream_t stream) {
  hipLaunchKernelGGL(k_firefly_resolve<K>, dim3((P + kFireflyBlock - 1) / kFireflyBlock), dim3(kFireflyBlock), 0, stream, d_planes, counts, P, d_image, d_stats);
}

}  // namespace

hipError_t firefly_accumulate_launch(const float4* d_results, uint32_t P, uint32_t batch, uint32_t first_sample, uint32_t K, float* d_planes, bool pixel_major, hipStream_t stream) {
  if (P == 0 || batch == 0) return hipSuccess;
  if (!d_results || !d_planes || K < kFireflyMinBuckets || K > kFireflyMaxBuckets || (uint64_t) P * batch > 0x7FFFFFFFull) return hipErrorInvalidValue;
  const uint32_t block = pixel_major ? kBucketPixelMajorBlock : kFireflyBlock;
  const uint32_t blocks = (P + block - 1) / block;
  hipLaunchKernelGGL(k_bucket_accumulate, dim3(blocks > kFireflyMaxGrid ? kFireflyMaxGrid : blocks), dim3(block), pixel_major ? bucket_lds_bytes(K) : 0u, stream, d_results, P, batch,
                     first_sample % K, K, d_planes, pixel_major ? 1u : 0u);
  return hipGetLastError();
}

hipError_t firefly_scatter_launch(const float4* d_results, const uint32_t* d_pixels, uint32_t count, uint32_t frame_pixels, float* d_planes, hipStream_t stream) {
  if (count == 0) return hipSuccess;
  if (!d_results || !d_pixels || !d_planes) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_bucket_accumulate_scatter, dim3(firefly_grid(count)), dim3(kFireflyBlock), 0, stream, d_results, d_pixels, count, frame_pixels, d_planes);
  return hipGetLastError();
}

hipError_t firefly_resolve_launch(const float* d_planes, const FireflyCounts& counts, uint32_t K, uint32_t P, float* d_image, uint32_t* d_stats, hipStream_t stream) {
  if (P == 0) return hipSuccess;
  if (!d_planes || !d_image || !d_stats) return hipErrorInvalidValue;
  switch (K) {
    case 4: resolve_launch<4>(d_planes, counts, P, d_image, d_stats, stream); break;
    case 5: resolve_launch<5>(d_planes, counts, P, d_image, d_stats, stream); break;
    case 6: resolve_launch<6>(d_planes, counts, P, d_image, d_stats, stream); break;
    case 7: resolve_launch<7>(d_planes, counts, P, d_image, d_stats, stream); break;
    case 8: resolve_launch<8>(d_planes, counts, P, d_image, d_stats, stream); break;
    case 9: resolve_launch<9>(d_planes, counts, P, d_image, d_stats, stream); break;
    case 10: resolve_launch<10>(d_planes, counts, P, d_image, d_stats, stream); break;
    case 11: resolve_launch<11>(d_planes, counts, P, d_image, d_stats, stream); break;
    case 12: resolve_launch<12>(d_planes, counts, P, d_image, d_stats, stream); break;
    case 13: resolve_launch<13>(d_planes, counts, P, d_image, d_stats, stream); break;
    case 14: resolve_launch<14>(d_planes, counts, P, d_image, d_stats, stream); break;
    case 15: resolve_launch<15>(d_planes, counts, P, d_image, d_stats, stream); break;
    case 16: resolve_launch<16>(d_planes, counts, P, d_image, d_stats, stream); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace lum
