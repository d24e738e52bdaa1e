// Stand-alone check of the work buffers' layouts (csrc/host/work_layout.h lay_out_work, lay_out_fused), for a sanitizer build: compiled by
// tests/test_work_layout.py with -fsanitize=address,undefined and run as a program of its own. Exits 0 when every case holds.
// For paths in {1, 255, 256, 257, 65537} x shadow kinds in {4, kVolumeShadowKinds} x clouds off / on, both arenas are laid out over a host block of exactly
// the size their layout derives, and compared with the table of (array, element size, element count) restated below:
//   every array starts on a 256-byte boundary, lies inside the block and overlaps no other; the arrays in order end exactly at the derived size; the arrays
//   that only exist with volumes or clouds are null otherwise; fallback.vis is shadow.vis; the pass over a null base yields only nulls.
// Last, the first and the last element of every array are written: an array that leaves the block is the sanitizer's to report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../luminary_amd/csrc/host/work_layout.h"

using namespace lum;

struct Expected { const char* name; const void* at; size_t element, count; bool exists; };

static int fail(const char* what, const char* array, uint32_t paths, uint32_t kinds, bool clouds) {
  std::fprintf(stderr, "work_layout_check: %s: %s (paths = %u, kinds = %u, clouds = %d)\n", what, array, paths, kinds, (int) clouds);
  return 1;
}

static void path_queue_rows(std::vector<Expected>& t, const char* name, const PathQueue& q, size_t n) {
  t.push_back({name, q.origin_t, 16, n, true}); t.push_back({name, q.dir_slot, 16, n, true}); t.push_back({name, q.aux, 16, n, true});
  t.push_back({name, q.hit_id, 16, n, true}); t.push_back({name, q.hit_scene_tri, 4, n, true});
}
static void nee_rows(std::vector<Expected>& t, const char* name, const NeeQueue& e, size_t n) {
  t.push_back({name, e.geo_color_light, 16, n, true}); t.push_back({name, e.bsdf_ray_prob, 16, n, true}); t.push_back({name, e.bsdf_weight_sum, 16, n, true});
  t.push_back({name, e.ambient, 16, n, true}); t.push_back({name, e.sun, 16, n, true}); t.push_back({name, e.amb_path, 4, n, true});
}

// The arrays in the order of the table, against a block of `size` bytes at `base`.
static int check_arena(const std::vector<Expected>& table, char* base, size_t size, uint32_t paths, uint32_t kinds, bool clouds) {
  if (((uintptr_t) base & 255u) != 0) return fail("the block itself is not aligned", "block", paths, kinds, clouds);
  size_t at = 0;
  for (const Expected& e : table) {
    if (!e.exists) {
      if (e.at) return fail("exists without its feature", e.name, paths, kinds, clouds);
      continue;
    }
    const char* p = (const char*) e.at;
    const size_t bytes = e.element * e.count;
    if (!p) return fail("null", e.name, paths, kinds, clouds);
    if (((uintptr_t) p & 255u) != 0) return fail("not on a 256-byte boundary", e.name, paths, kinds, clouds);
    if (p < base || bytes > size || (size_t) (p - base) > size - bytes) return fail("leaves the block", e.name, paths, kinds, clouds);
    if ((size_t) (p - base) < at) return fail("overlaps the array before it", e.name, paths, kinds, clouds);
    if ((size_t) (p - base) != at) return fail("does not follow the array before it", e.name, paths, kinds, clouds);
    at += (bytes + 255) & ~(size_t) 255;
  }
  if (at != size) return fail("the arrays do not end at the derived size", "block", paths, kinds, clouds);
  for (const Expected& e : table) {  // the sanitizer's part
    if (!e.exists) continue;
    char* p = (char*) e.at;
    std::memset(p, 0xA5, e.element);
    std::memset(p + e.element * (e.count - 1), 0x5A, e.element);
  }
  return 0;
}

static int check(uint32_t paths, uint32_t kinds, bool clouds) {
  const size_t n = paths;
  const bool volumes = kinds > 4u;
  // ---- the work arena ----
  WorkBuffers sized, w;
  ArenaCarver size(nullptr);
  lay_out_work(size, paths, kinds, clouds, sized);
  if (sized.queue[0].origin_t || sized.shadow.vis || sized.results || sized.cloud.items || sized.volume.items) return fail("a pointer from a null base", "work", paths, kinds, clouds);
  char* block = (char*) std::aligned_alloc(256, size.used);
  if (!block) return fail("no host memory", "work", paths, kinds, clouds);
  ArenaCarver arena(block);
  lay_out_work(arena, paths, kinds, clouds, w);
  if (arena.used != size.used) return fail("the two passes disagree", "work", paths, kinds, clouds);
  if (w.capacity != paths || w.shadow_kinds != kinds || w.shadow.capacity != paths || w.cloud.capacity != (clouds ? paths : 0u)) return fail("capacities", "work", paths, kinds, clouds);
  if (w.queue[2].origin_t || w.queue[0].parent || w.queue[1].parent || w.queue[2].parent) return fail("the fused arena's arrays set by the work layout", "work", paths, kinds, clouds);
  std::vector<Expected> t;
  path_queue_rows(t, "queue[0]", w.queue[0], n);
  path_queue_rows(t, "queue[1]", w.queue[1], n);
  nee_rows(t, "nee", w.nee, n);
  t.push_back({"results", w.results, 16, n, true});
  t.push_back({"shadow.origin_dist", w.shadow.origin_dist, 16, kinds * n, true}); t.push_back({"shadow.dir_out", w.shadow.dir_out, 16, kinds * n, true});
  t.push_back({"shadow.ids", w.shadow.ids, 16, kinds * n, true}); t.push_back({"shadow.vis", w.shadow.vis, 16, kinds * n, true});
  t.push_back({"shadow.light_items", w.shadow.light_items, 4, n, true});
  t.push_back({"volume.bridge", w.volume.bridge, 16, n, volumes}); t.push_back({"volume.sky", w.volume.sky, 16, n, volumes}); t.push_back({"volume.weight", w.volume.weight, 16, n, volumes});
  t.push_back({"volume.sun_water", w.volume.sun_water, 16, n, volumes}); t.push_back({"volume.amb_t1", w.volume.amb_t1, 16, n, volumes});
  t.push_back({"volume.amb_t2", w.volume.amb_t2, 16, n, volumes}); t.push_back({"volume.items", w.volume.items, 4, n, volumes});
  t.push_back({"nee.sun_water", w.nee.sun_water, 16, n, volumes}); t.push_back({"nee.amb_t1", w.nee.amb_t1, 16, n, volumes}); t.push_back({"nee.amb_t2", w.nee.amb_t2, 16, n, volumes});
  t.push_back({"cloud.items", w.cloud.items, 4, 3 * n, clouds}); t.push_back({"cloud.result", w.cloud.result, 16, 3 * n, clouds});
  t.push_back({"cloud.hit_dist", w.cloud.hit_dist, 4, 3 * n, clouds});
  int bad = check_arena(t, block, size.used, paths, kinds, clouds);
  // ---- the fused arena, beside it ----
  FusedBuffers fsized, f;
  ArenaCarver fsize(nullptr);
  lay_out_fused(fsize, paths, w, fsized);
  if (!bad && (fsized.queue.origin_t || fsized.parent[0] || fsized.records || fsized.ended[1])) bad = fail("a pointer from a null base", "fused", paths, kinds, clouds);
  char* fblock = (char*) std::aligned_alloc(256, fsize.used);
  if (!fblock) { std::free(block); return fail("no host memory", "fused", paths, kinds, clouds); }
  ArenaCarver farena(fblock);
  lay_out_fused(farena, paths, w, f);
  if (!bad && farena.used != fsize.used) bad = fail("the two passes disagree", "fused", paths, kinds, clouds);
  if (!bad && (f.capacity != paths || f.fallback.capacity != paths)) bad = fail("capacities", "fused", paths, kinds, clouds);
  if (!bad && f.fallback.vis != w.shadow.vis) bad = fail("is not shadow.vis", "fallback.vis", paths, kinds, clouds);
  std::vector<Expected> ft;
  path_queue_rows(ft, "fused.queue", f.queue, n);
  for (int k = 0; k < 3; k++) ft.push_back({"fused.parent", f.parent[k], 4, n, true});
  nee_rows(ft, "fused.nee", f.nee, n);
  ft.push_back({"fallback.origin_dist", f.fallback.origin_dist, 16, n, true}); ft.push_back({"fallback.dir_out", f.fallback.dir_out, 16, n, true});
  ft.push_back({"fallback.ids", f.fallback.ids, 16, n, true}); ft.push_back({"fallback.light_items", f.fallback.light_items, 4, n, true});
  ft.push_back({"fused.ended[0]", f.ended[0], 4, n, true}); ft.push_back({"fused.ended[1]", f.ended[1], 4, n, true});
  ft.push_back({"fused.records", f.records, sizeof(FusedResolve), 6, true});
  if (!bad) bad = check_arena(ft, fblock, fsize.used, paths, kinds, clouds);
  std::free(fblock);
  std::free(block);
  return bad;
}

int main() {
  const uint32_t paths[] = {1u, 255u, 256u, 257u, 65537u}, kinds[] = {4u, kVolumeShadowKinds};
  int cases = 0;
  for (uint32_t p : paths)
    for (uint32_t k : kinds)
      for (int clouds = 0; clouds < 2; clouds++, cases++)
        if (check(p, k, clouds != 0)) return 1;
  std::printf("work_layout_check: ok (%d cases)\n", cases);
  return 0;
}
