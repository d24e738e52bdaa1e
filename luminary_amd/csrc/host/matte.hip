// ID mattes on the device (lumc_render_first_hits, lumc_download_mattes, lumc_matte_mask): the first hits of a closest-hit pass folded into
// per-pixel tables of (id, count), the tables ranked by coverage, and the coverage of a list of ids. The definition is matte.h's, the same source the host twin
// (matte.cpp) is compiled from: integers and one IEEE division per output, this unit is compiled like that one without contraction, both give the same bytes
// (lumc_matte_host, tests/test_matte_gpu.py). Streaming kernels beside k_guide; no kernel of the renderer is touched.
//
// Planes [layer][word][pixels], word = slot ids 0 ... 7, slot counts 0 ... 7, dropped: consecutive lanes of a pass are consecutive pixels (one sample id per pass,
// paths in pixel order where the camera made one), so every load below is a run of consecutive words per wave.
//
//   k_matte_accumulate  one thread per path, grid-stride, both layers in one launch. A layer's 17 words are loaded before any is looked at: they are independent and
//                       coalesced, where a slot-by-slot loop with an early exit would wait for up to eight dependent round trips. The slot is picked by unrolled
//                       selects (matte_find), and only what changed goes back: the one (id, count) pair, or the dropped word. A pixel has at most one path per
//                       pass, so plain loads and stores. No LDS, no per-thread array that is indexed at run time.
//   k_matte_resolve     one thread per pixel of one layer: the C^2 comparisons unrolled, R ranks of ids and coverage, dropped and rays written planar; one atomic
//                       per pixel that dropped anything (they are rare: a pixel that saw more than eight ids).
//   k_matte_mask        one thread per pixel of one layer: the counts of the slots whose id is in a list of up to 16 that arrives as a kernel argument.
#include <hip/hip_runtime.h>

#include "matte.h"

namespace lum {
namespace {

constexpr uint32_t kMatteBlock = 256;
constexpr uint32_t kMatteMaxGrid = 2048;  // 256 CUs x 8 resident workgroups, grid-stride beyond that (context.h grid_for)

inline uint32_t matte_grid(uint32_t n) {
  const uint32_t blocks = (n + kMatteBlock - 1) / kMatteBlock;
  return blocks < 1 ? 1 : (blocks > kMatteMaxGrid ? kMatteMaxGrid : blocks);
}

__device__ __forceinline__ MatteTable load_table(const uint32_t* __restrict__ planes, uint32_t n, uint32_t p) {
  MatteTable t;
#pragma unroll
  for (uint32_t k = 0; k < kMatteSlots; k++) t.id[k] = planes[(size_t) k * n + p];
#pragma unroll
  for (uint32_t k = 0; k < kMatteSlots; k++) t.count[k] = planes[(size_t) (kMatteSlots + k) * n + p];
  t.dropped = planes[(size_t) (2u * kMatteSlots) * n + p];
  return t;
}

__device__ __forceinline__ void accumulate_layer(uint32_t* planes, uint32_t n, uint32_t p, uint32_t v) {
  const MatteInsert w = matte_find(load_table(planes, n, p), v);
  if (w.slot < kMatteSlots) {
    planes[(size_t) w.slot * n + p] = w.id;
    planes[(size_t) (kMatteSlots + w.slot) * n + p] = w.count;
  }
  else planes[(size_t) (2u * kMatteSlots) * n + p] = w.count;
}

__global__ __launch_bounds__(kMatteBlock) void k_matte_accumulate(const uint4* __restrict__ hit_id, const uint32_t* __restrict__ hit_scene_tri, const uint32_t* __restrict__ paths_word,
                                                                  const uint4* __restrict__ tri_tex, uint32_t width, uint32_t n, uint32_t* instance_planes,
                                                                  uint32_t* material_planes) {
  const uint32_t paths = *paths_word;
  for (uint32_t i = blockIdx.x * kMatteBlock + threadIdx.x; i < paths; i += gridDim.x * kMatteBlock) {
    const uint4 hid = hit_id[i];
    const uint32_t p = (hid.z & 0xFFFFu) + (hid.z >> 16) * width;  // as k_guide: one sample id per pass, a pixel has at most one path
    if (p >= n) continue;
    const uint32_t c = matte_classify(hid.x);
    if (instance_planes) accumulate_layer(instance_planes, n, p, matte_sample_id(c, hid.x));
    if (material_planes) {
      uint32_t material = 0;
      if (c == kMatteClassTriangle && tri_tex) material = tri_tex[hit_scene_tri[i] & kMatteHitTriMask].w & 0xFFFFu;
      accumulate_layer(material_planes, n, p, matte_sample_id(c, material));
    }
  }
}

__global__ __launch_bounds__(kMatteBlock) void k_matte_resolve(const uint32_t* __restrict__ planes, uint32_t n, uint32_t samples, uint32_t ranks, uint32_t* ids, float* coverage,
                                                               uint32_t* dropped, uint32_t* rays, uint32_t* dropped_pixels) {
  for (uint32_t p = blockIdx.x * kMatteBlock + threadIdx.x; p < n; p += gridDim.x * kMatteBlock) {
    const MatteTable t = load_table(planes, n, p);
    const MatteRanks r = matte_resolve_pixel(t, samples);
#pragma unroll
    for (uint32_t k = 0; k < kMatteSlots; k++) {
      if (k < ranks) {
        if (ids) ids[(size_t) k * n + p] = r.id[k];
        if (coverage) coverage[(size_t) k * n + p] = r.coverage[k];
      }
    }
    if (dropped) dropped[p] = t.dropped;
    if (rays) rays[p] = r.rays;
    if (dropped_pixels && t.dropped > 0u) atomicAdd(dropped_pixels, 1u);
  }
}

__global__ __launch_bounds__(kMatteBlock) void k_matte_mask(const uint32_t* __restrict__ planes, uint32_t n, uint32_t samples, MatteIdList list, float* mask) {
  for (uint32_t p = blockIdx.x * kMatteBlock + threadIdx.x; p < n; p += gridDim.x * kMatteBlock) mask[p] = matte_mask_pixel(load_table(planes, n, p), list, samples);
}

}  // namespace

hipError_t matte_accumulate_launch(const uint4* d_hit_id, const uint32_t* d_hit_scene_tri, const uint32_t* d_paths, const uint4* d_tri_tex, uint32_t width, uint32_t n,
                                   uint32_t* d_instance_planes, uint32_t* d_material_planes, hipStream_t stream) {
  if (n == 0 || (!d_instance_planes && !d_material_planes)) return hipSuccess;
  if (!d_hit_id || !d_hit_scene_tri || !d_paths || width == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_matte_accumulate, dim3(matte_grid(n)), dim3(kMatteBlock), 0, stream, d_hit_id, d_hit_scene_tri, d_paths, d_tri_tex, width, n, d_instance_planes,
                     d_material_planes);
  return hipGetLastError();
}

hipError_t matte_resolve_launch(const uint32_t* d_planes, uint32_t n, uint32_t samples, uint32_t ranks, uint32_t* d_ids, float* d_coverage, uint32_t* d_dropped,
                                uint32_t* d_rays, uint32_t* d_dropped_pixels, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (!d_planes || samples == 0 || samples > kMatteMaxSamples || ranks == 0 || ranks > kMatteSlots) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_matte_resolve, dim3(matte_grid(n)), dim3(kMatteBlock), 0, stream, d_planes, n, samples, ranks, d_ids, d_coverage, d_dropped, d_rays, d_dropped_pixels);
  return hipGetLastError();
}

hipError_t matte_mask_launch(const uint32_t* d_planes, uint32_t n, uint32_t samples, const MatteIdList& ids, float* d_mask, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (!d_planes || !d_mask || samples == 0 || samples > kMatteMaxSamples || ids.count > kMatteMaxMaskIds) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_matte_mask, dim3(matte_grid(n)), dim3(kMatteBlock), 0, stream, d_planes, n, samples, ids, d_mask);
  return hipGetLastError();
}

}  // namespace lum
