// The two arenas of a pass's work buffers. lay_out_work and lay_out_fused name every array once, with its element type and count; an arena's size is what its
// layout adds up to over a null base (offsets are counted, no pointer is formed), its pointers come from the same function over the allocation: a new array is
// one line here. Host only, no HIP call: a plain C++ compiler takes it (tests/support/work_layout_check.cpp lays both arenas out over host memory).
#pragma once

#include <cstddef>
#include <cstdint>

#include "../device/dev_scene.h"

namespace lum {

// Hands out consecutive arrays of one block, each on a 256-byte boundary of it.
struct ArenaCarver {
  char* base;       // null: only the size is wanted, every array comes out null
  size_t used = 0;  // bytes handed out so far, the rounding of the last array included
  explicit ArenaCarver(char* block) : base(block) {}
  template <typename T> void take(T*& array, size_t count) {
    array = base ? reinterpret_cast<T*>(base + used) : nullptr;
    used += (sizeof(T) * count + 255) & ~(size_t) 255;
  }
};

// Views into the work arena (LumContext::Work owns the block).
struct WorkBuffers {
  uint32_t capacity = 0;      // paths
  uint32_t shadow_kinds = 0;  // visibility-ray kinds per path the arena was laid out for (4, or kVolumeShadowKinds with fog or an ocean)
  PathQueue queue[3]{};       // [2], and every queue's parent plane: the fused arena's, entered by ensure_fused
  NeeQueue nee{};
  float4* results = nullptr;
  ShadowQueue shadow{};
  VolumeQueue volume{};       // with volumes (shadow_kinds > 4), else null
  CloudQueue cloud{};         // the cloud marches of a depth (kernels.h k_clouds_*) when clouds are marched, else null
};
// Views into the fused resolve's arena (FusedResolve, kernels.h; LumContext::Fused owns the block): what it needs beyond the work buffers.
struct FusedBuffers {
  uint32_t capacity = 0;
  PathQueue queue{};                                  // the third path queue
  uint32_t* parent[3] = {nullptr, nullptr, nullptr};  // the parent words of the three queues
  NeeQueue nee{};                                     // the second set of NEE records
  ShadowQueue fallback{};                             // the fallback rays' items
  uint32_t* ended[2] = {nullptr, nullptr};  // a depth's vertices that no entry continues, by the depth's parity (k_shade lists them; the next depth's k_shade resolves them, or k_resolve_ended)
  FusedResolve* records = nullptr;          // six records in device memory: the previous depth's queue (three buffers) and NEE records (two) by depth % 6
};

inline void lay_out_path_queue(ArenaCarver& a, size_t n, PathQueue& q) { a.take(q.origin_t, n); a.take(q.dir_slot, n); a.take(q.aux, n); a.take(q.hit_id, n); a.take(q.hit_scene_tri, n); }
inline void lay_out_nee_records(ArenaCarver& a, size_t n, NeeQueue& e) {
  a.take(e.geo_color_light, n); a.take(e.bsdf_ray_prob, n); a.take(e.bsdf_weight_sum, n); a.take(e.ambient, n); a.take(e.sun, n); a.take(e.amb_path, n);
}

// Per path: two queue entries, the NEE records, the result, up to `shadow_kinds` visibility rays with their answers and a light-query index; with volumes the
// in-scattering records, the scattering-event index and the water-surface factors of the surface vertices; with clouds up to three marches.
inline void lay_out_work(ArenaCarver& a, uint32_t paths, uint32_t shadow_kinds, bool clouds, WorkBuffers& w) {
  const size_t n = paths;
  w = WorkBuffers{};
  for (int k = 0; k < 2; k++) lay_out_path_queue(a, n, w.queue[k]);
  lay_out_nee_records(a, n, w.nee); a.take(w.results, n);
  a.take(w.shadow.origin_dist, shadow_kinds * n); a.take(w.shadow.dir_out, shadow_kinds * n); a.take(w.shadow.ids, shadow_kinds * n); a.take(w.shadow.vis, shadow_kinds * n);
  a.take(w.shadow.light_items, n);
  if (shadow_kinds > 4u) {
    a.take(w.volume.bridge, n); a.take(w.volume.sky, n); a.take(w.volume.weight, n); a.take(w.volume.sun_water, n); a.take(w.volume.amb_t1, n); a.take(w.volume.amb_t2, n);
    a.take(w.volume.items, n); a.take(w.nee.sun_water, n); a.take(w.nee.amb_t1, n); a.take(w.nee.amb_t2, n);
  }
  if (clouds) { a.take(w.cloud.items, 3 * n); a.take(w.cloud.result, 3 * n); a.take(w.cloud.hit_dist, 3 * n); }  // per path up to three marches: list entry, result, distance of the first cloud
  w.capacity = w.shadow.capacity = paths; w.cloud.capacity = clouds ? paths : 0u; w.shadow_kinds = shadow_kinds;
}

// Per path: a third queue entry, three parent words, a second set of NEE records, one fallback ray with its vertex's index and two list entries; then the six records.
inline void lay_out_fused(ArenaCarver& a, uint32_t paths, const WorkBuffers& w, FusedBuffers& f) {
  const size_t n = paths;
  f = FusedBuffers{};
  lay_out_path_queue(a, n, f.queue);
  for (int k = 0; k < 3; k++) a.take(f.parent[k], n);
  lay_out_nee_records(a, n, f.nee);
  a.take(f.fallback.origin_dist, n); a.take(f.fallback.dir_out, n); a.take(f.fallback.ids, n); a.take(f.fallback.light_items, n);
  f.fallback.vis = w.shadow.vis;  // the undecided samples' answers go where the depth's own ambient answers went: kind 2 of the previous depth's words
  a.take(f.ended[0], n); a.take(f.ended[1], n); a.take(f.records, 6);
  f.capacity = paths; f.fallback.capacity = w.shadow.capacity;
}

}  // namespace lum
