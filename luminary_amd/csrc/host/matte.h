// ID mattes: per pixel and layer the ids the first hits of a frame's sample ids saw, ranked by coverage (lum_core.h lumc_render_first_hits / lumc_download_mattes /
// lumc_matte_mask; the idea of Friedman and Jones, "Fully automatic ID mattes with support for motion blur and transparency", SIGGRAPH 2015
// posters - Cryptomatte). The ONE definition of a pixel's table, its ranks and its mask - matte_insert, matte_resolve_pixel, matte_mask_pixel -, compiled twice: by
// the host compiler into matte.cpp (lumc_matte_host, lumc_matte_mask_host_twin: the twin, no HIP in it) and by the device compiler into matte.hip (k_matte_*). The
// arithmetic is integers and one IEEE division per output, so both give the same bytes.
//
// Ids. A sample's id in the instance layer is the first hit's instance id, in the material layer the material id of the hit triangle (the low 16 bits of the
// triangle's texture record, what luminary_host_get_pixel_info reports). A first hit that is no triangle has the same reserved id in both layers: kMatteIdMiss,
// kMatteIdOcean, kMatteIdParticle; the classification is k_guide's (matte_classify). kMatteIdEmpty marks an unused slot or rank and is never a sample's id. A
// sample without a path (a physical camera's ray that did not leave the lens) contributes to nothing.
//
// Table. Per pixel and layer C = 8 slots of (id, count) and one `dropped` counter. Insert of id v, in ascending slot order:
//   1. the first slot with count > 0 and id == v gets count + 1;
//   2. otherwise the first slot with count == 0 becomes (v, 1);
//   3. otherwise dropped + 1.
// Passes run in ascending sample id and a pixel has at most one path per pass, so the table is a function of the pixel's id sequence alone: first come keeps its
// slot, and a ninth distinct id is dropped every time it recurs - also where it ends up the most frequent id of the pixel. dropped says how much of the pixel
// the table does not name. Invariant: sum of counts + dropped = the pixel's samples that had a path (`rays`).
//
// Resolve, per pixel and layer, for R ranks (1 ... 8): over occupied slots rank_j = #{k : count_k > count_j or (count_k == count_j and id_k < id_j)} - a
// permutation of 0 ... occupied - 1, by the C^2 unrolled comparisons, no sort and no dynamically indexed array. For r < R: ids[r] = the id of rank r,
// coverage[r] = (float) count / (float) samples, one division; ranks beyond the occupied slots hold kMatteIdEmpty and +0.
//
// Mask. Given up to 16 ids: (float) (sum of the counts of the slots whose id is listed) / (float) samples, over all C slots. An id listed twice counts once.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define LUM_MATTE_FN __host__ __device__ __forceinline__
#define LUM_MATTE_UNROLL _Pragma("unroll")
#else
#define LUM_MATTE_FN inline
#define LUM_MATTE_UNROLL
#endif

namespace lum {

constexpr uint32_t kMatteSlots = 8, kMatteLayers = 2, kMatteMaxMaskIds = 16, kMatteMaxSamples = 1024;
constexpr uint32_t kMatteWordsPerLayer = 2u * kMatteSlots + 1u;  // planes per layer: ids [8], counts [8], dropped - 68 bytes per pixel
constexpr uint32_t kMatteIdEmpty = 0xFFFFFFFFu, kMatteIdMiss = 0xFFFFFFFEu, kMatteIdOcean = 0xFFFFFFFDu, kMatteIdParticle = 0xFFFFFFFCu;
// the hit words of the device code, restated for the two compilers (dev_ocean.h, dev_particle.h, dev_volume.h, kernels.h, which no host unit includes; tests/test_matte.py reads both and compares)
constexpr uint32_t kMatteHitOcean = 0xFFFFFFFDu, kMatteHitParticleMin = 0x80000000u, kMatteHitParticleMax = 0xEFFFFFFFu, kMatteHitTriangleLimit = 0x7FFFFFFFu;
constexpr uint32_t kMatteHitTriMask = 0x0FFFFFFFu;

enum MatteClass : uint32_t { kMatteClassMiss = 0, kMatteClassOcean = 1, kMatteClassParticle = 2, kMatteClassTriangle = 3 };

// k_guide's order: the ocean, a particle, a triangle, else nothing
LUM_MATTE_FN uint32_t matte_classify(uint32_t hit_instance) {
  if (hit_instance == kMatteHitOcean) return kMatteClassOcean;
  if (hit_instance <= kMatteHitParticleMax && hit_instance >= kMatteHitParticleMin) return kMatteClassParticle;
  if (hit_instance <= kMatteHitTriangleLimit) return kMatteClassTriangle;
  return kMatteClassMiss;
}
// the id of a sample whose first hit is of class `c`; triangle_id: the layer's id of a triangle hit
LUM_MATTE_FN uint32_t matte_sample_id(uint32_t c, uint32_t triangle_id) {
  return c == kMatteClassTriangle ? triangle_id : (c == kMatteClassOcean ? kMatteIdOcean : (c == kMatteClassParticle ? kMatteIdParticle : kMatteIdMiss));
}

struct MatteTable { uint32_t id[kMatteSlots], count[kMatteSlots], dropped; };

// What an insert changes: slot < kMatteSlots becomes (id, count); slot == kMatteSlots: dropped becomes `count`. Nothing else of the table moves, so a caller that
// holds the table in memory writes back these words alone.
struct MatteInsert { uint32_t slot, id, count; };

LUM_MATTE_FN MatteInsert matte_find(const MatteTable& t, uint32_t v) {
  uint32_t match = kMatteSlots, free_slot = kMatteSlots, match_count = 0;
  LUM_MATTE_UNROLL
  for (uint32_t k = kMatteSlots; k-- > 0;) {  // descending, so that the lowest slot is what stays
    const bool used = t.count[k] > 0u;
    if (used && t.id[k] == v) { match = k; match_count = t.count[k]; }
    if (!used) free_slot = k;
  }
  if (match < kMatteSlots) return {match, v, match_count + 1u};
  if (free_slot < kMatteSlots) return {free_slot, v, 1u};
  return {kMatteSlots, v, t.dropped + 1u};
}

LUM_MATTE_FN void matte_insert(MatteTable& t, uint32_t v) {
  const MatteInsert w = matte_find(t, v);
  if (w.slot == kMatteSlots) { t.dropped = w.count; return; }
  LUM_MATTE_UNROLL
  for (uint32_t k = 0; k < kMatteSlots; k++)
    if (k == w.slot) { t.id[k] = w.id; t.count[k] = w.count; }
}

struct MatteRanks { uint32_t id[kMatteSlots]; float coverage[kMatteSlots]; uint32_t rays; };

// All C ranks of a table; the caller keeps the first R. samples >= 1.
LUM_MATTE_FN MatteRanks matte_resolve_pixel(const MatteTable& t, uint32_t samples) {
  MatteRanks out;
  const float n = (float) samples;
  uint32_t sum = t.dropped;
  LUM_MATTE_UNROLL
  for (uint32_t r = 0; r < kMatteSlots; r++) { out.id[r] = kMatteIdEmpty; out.coverage[r] = 0.0f; }
  LUM_MATTE_UNROLL
  for (uint32_t j = 0; j < kMatteSlots; j++) {
    const bool used = t.count[j] > 0u;
    sum += used ? t.count[j] : 0u;
    uint32_t rank = 0;
    LUM_MATTE_UNROLL
    for (uint32_t k = 0; k < kMatteSlots; k++) {
      if (k == j) continue;
      const bool before = t.count[k] > t.count[j] || (t.count[k] == t.count[j] && t.id[k] < t.id[j]);
      rank += (t.count[k] > 0u && before) ? 1u : 0u;
    }
    const float c = (float) t.count[j] / n;
    LUM_MATTE_UNROLL
    for (uint32_t r = 0; r < kMatteSlots; r++)
      if (used && rank == r) { out.id[r] = t.id[j]; out.coverage[r] = c; }
  }
  out.rays = sum;
  return out;
}

struct MatteIdList { uint32_t id[kMatteMaxMaskIds]; uint32_t count; };  // count <= kMatteMaxMaskIds

LUM_MATTE_FN float matte_mask_pixel(const MatteTable& t, const MatteIdList& ids, uint32_t samples) {
  uint32_t sum = 0;
  LUM_MATTE_UNROLL
  for (uint32_t k = 0; k < kMatteSlots; k++) {
    bool listed = false;
    LUM_MATTE_UNROLL
    for (uint32_t i = 0; i < kMatteMaxMaskIds; i++) listed = listed || (i < ids.count && ids.id[i] == t.id[k]);
    sum += (t.count[k] > 0u && listed) ? t.count[k] : 0u;
  }
  return (float) sum / (float) samples;
}

}  // namespace lum

#if defined(__HIP_PLATFORM_AMD__) && !defined(LUM_MATTE_HOST_ONLY)

#include <hip/hip_runtime_api.h>

#include "device_buffer.h"

#pragma GCC visibility push(hidden)

namespace lum {

// A context's mattes: 68 bytes per pixel and layer held, planes [layer held][word][pixels] with word = slot ids 0 ... 7, slot counts 0 ... 7, dropped - a wave's
// accesses to one word are consecutive.
struct Mattes {
  DeviceBuffer<uint32_t> planes;     // allocated at the first matte render, freed by lumc_matte_release and with the context
  DeviceBuffer<uint32_t> d_dropped;  // [kMatteLayers]: pixels with dropped > 0, counted by k_matte_resolve
  uint32_t pixels = 0;               // the frame the planes were allocated for
  uint32_t layers = 0;               // LUMC_MATTE_* bits the planes hold
  uint32_t samples = 0;              // sample ids of the last render
  bool valid = false;                // cleared wherever the denoiser's guides are
  const char* stale = nullptr;       // what made a rendered set invalid (a string literal), null where none was rendered
  double seconds = 0.0;              // the last accumulation, host clock around its passes (synchronised)
  // the planes of `layer` (0 instance, 1 material): null where it is not held
  uint32_t* layer_planes(uint32_t layer) const {
    if (!planes || !((layers >> layer) & 1u)) return nullptr;
    return planes.get() + (size_t) ((layer == 1u && (layers & 1u)) ? 1u : 0u) * kMatteWordsPerLayer * pixels;
  }
};

// k_matte_accumulate: one thread per path of a closest-hit pass over one sample id of every pixel (the first `*d_paths` entries of the queue's planes); the pixel
// from hit_id.z as k_guide takes it, both layers in one launch. A null layer is skipped. n: the frame's pixels, the planes' stride. Asynchronous, as the two below.
hipError_t matte_accumulate_launch(const uint4* d_hit_id, const uint32_t* d_hit_scene_tri, const uint32_t* d_paths, const uint4* d_tri_tex, uint32_t width, uint32_t n,
                                   uint32_t* d_instance_planes, uint32_t* d_material_planes, hipStream_t stream);
// k_matte_resolve: one thread per pixel of one layer; outputs planar [ranks][n] (each may be null); d_dropped_pixels (may be null) += pixels with dropped > 0.
hipError_t matte_resolve_launch(const uint32_t* d_planes, uint32_t n, uint32_t samples, uint32_t ranks, uint32_t* d_ids, float* d_coverage, uint32_t* d_dropped,
                                uint32_t* d_rays, uint32_t* d_dropped_pixels, hipStream_t stream);
// k_matte_mask: one thread per pixel of one layer.
hipError_t matte_mask_launch(const uint32_t* d_planes, uint32_t n, uint32_t samples, const MatteIdList& ids, float* d_mask, hipStream_t stream);

}  // namespace lum

#pragma GCC visibility pop
#endif
