// Stand-alone check of what the refit in the resident node array rests on (csrc/host/bvh_build.cpp layout_resident_nodes with its slot map, resident_depth_slots),
// for a sanitizer build: compiled together with bvh_build.cpp by tests/test_resident_refit.py with -fsanitize=address,undefined and run as a program of its own.
// Exits 0 when every case holds. Soups of 1, 2, 7, 300 and 30 000 triangles in 1 to 3 meshes, capacities 1, 5 and 4000:
//   1. the slot map is a bijection onto [C, C + M), mesh_root[m] is the slot of the mesh's node 0
//   2. the depth lists hold every slot of the mesh exactly once
//   3. every inner child sits one depth below its parent
//   4. a host twin of the device's refit - the same loop over the depth lists, deepest first, writing padded child boxes into the laid-out array and exact boxes
//      into a per-slot scratch - equals layout_resident_nodes over refit_bvh4's trees byte for byte
//   5. with 30 000 triangles and C = 4000 one mesh's slots are no range: part of it sits among the tops of all meshes, the rest behind them
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../luminary_amd/csrc/host/bvh_build.h"

using namespace lum;

static uint64_t g_state = 0x2545F4914F6CDD1Dull;
static float uniform(float lo, float hi) {
  g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
  return lo + (hi - lo) * (float) ((g_state >> 40) * (1.0 / 16777216.0));
}
static std::vector<Aabb> soup(uint32_t n, uint64_t seed) {
  g_state = seed * 0x9E3779B97F4A7C15ull + 1;
  std::vector<Aabb> boxes(n);
  const float sizes[3] = {0.05f, 0.5f, 4.0f};
  for (Aabb& b : boxes) {
    const float c[3] = {uniform(-10, 10), uniform(-10, 10), uniform(-10, 10)}, s = sizes[(int) uniform(0, 2.999f)];
    float v[3][3];
    for (auto& p : v) for (int k = 0; k < 3; k++) p[k] = c[k] + s * uniform(-2, 2);
    b = tri_box(v[0], v[1], v[2]);
  }
  return boxes;
}
static int fail(const char* what, size_t scene, uint32_t capacity, uint32_t mesh) {
  std::fprintf(stderr, "resident_refit_check: %s (scene %zu, capacity %u, mesh %u)\n", what, scene, capacity, mesh);
  return 1;
}

static Aabb empty_box() { return Aabb{{FLT_MAX, FLT_MAX, FLT_MAX}, {-FLT_MAX, -FLT_MAX, -FLT_MAX}}; }
static void grow(Aabb& a, const Aabb& b) {
  for (int k = 0; k < 3; k++) { a.lo[k] = std::min(a.lo[k], b.lo[k]); a.hi[k] = std::max(a.hi[k], b.hi[k]); }
}
static void set_child_box(Bvh4Node& n, int k, const Aabb& b) {  // bvh_build.cpp set_child_box, the expression the kernels repeat
  float lo[3], hi[3];
  for (int a = 0; a < 3; a++) {
    const float pad = 1e-5f * std::max(std::max(std::fabs(b.lo[a]), std::fabs(b.hi[a])), 1e-20f) + 1e-30f;
    lo[a] = b.lo[a] - pad; hi[a] = b.hi[a] + pad;
  }
  n.lo_x[k] = lo[0]; n.lo_y[k] = lo[1]; n.lo_z[k] = lo[2];
  n.hi_x[k] = hi[0]; n.hi_y[k] = hi[1]; n.hi_z[k] = hi[2];
}

int main() {
  const std::vector<std::vector<uint32_t>> scenes = {{1}, {2}, {7}, {300}, {30000}, {1, 300}, {7, 2}, {300, 1, 2}, {30000, 300, 7}};
  const uint32_t capacities[] = {1, 5, 4000};
  bool saw_split = false;
  for (size_t s = 0; s < scenes.size(); s++) {
    const uint32_t nm = (uint32_t) scenes[s].size();
    std::vector<std::vector<Aabb>> from(nm), to(nm);
    std::vector<Bvh4> built(nm), refitted(nm);
    std::vector<const Bvh4*> built_ptr(nm), refitted_ptr(nm);
    std::vector<uint32_t> offset(nm + 1, 0);
    for (uint32_t m = 0; m < nm; m++) {
      const uint32_t n = scenes[s][m];
      offset[m + 1] = offset[m] + n;
      from[m] = soup(n, 100 * s + m); to[m] = soup(n, 100 * s + m + 50);
      built[m] = build_bvh4(from[m].data(), n, kBvhLeafMaxTri, 26);
      if (built[m].nodes.empty()) return fail("no tree", s, 0, m);
      refitted[m] = refit_bvh4(built[m], to[m].data(), n);
      if (refitted[m].nodes.empty()) return fail("no refit", s, 0, m);
      built_ptr[m] = &built[m]; refitted_ptr[m] = &refitted[m];
    }
    LumDeviceSceneView v;
    std::memset(&v, 0, sizeof(v));
    v.num_meshes = nm; v.mesh_tri_offset = offset.data();
    for (uint32_t C : capacities) {
      std::vector<Bvh4Node> nodes, want;
      std::vector<uint32_t> mesh_root, want_root;
      std::vector<std::vector<uint32_t>> slots;
      layout_resident_nodes(v, built_ptr.data(), C, nodes, mesh_root, &slots);
      layout_resident_nodes(v, refitted_ptr.data(), C, want, want_root);
      if (nodes.size() != want.size() || mesh_root != want_root || slots.size() != nm || nodes.size() < C) return fail("the two layouts differ in size or roots", s, C, 0);
      const uint32_t M = (uint32_t) nodes.size() - C;
      // 1
      std::vector<uint8_t> taken(M, 0);
      size_t total = 0;
      for (uint32_t m = 0; m < nm; m++) {
        if (slots[m].size() != built[m].nodes.size()) return fail("a slot map of another size than the tree", s, C, m);
        for (uint32_t slot : slots[m]) {
          if (slot < C || slot - C >= M || taken[slot - C]) return fail("a slot outside [C, C + M) or taken twice", s, C, m);
          taken[slot - C] = 1;
        }
        total += slots[m].size();
        if (mesh_root[m] != slots[m][0]) return fail("mesh_root is not the slot of the mesh's root", s, C, m);
      }
      if (total != M) return fail("the slot maps do not cover [C, C + M)", s, C, 0);
      std::vector<Aabb> slot_box(M, empty_box());
      for (uint32_t m = 0; m < nm; m++) {
        // 2
        std::vector<uint32_t> depth_slots, depth_first;
        if (!resident_depth_slots(built[m], scenes[s][m], slots[m], depth_slots, depth_first)) return fail("no depth lists", s, C, m);
        if (depth_slots.size() != slots[m].size() || depth_first.size() < 2 || depth_first.front() != 0 || depth_first.back() != depth_slots.size()) return fail("depth lists of another size", s, C, m);
        std::vector<uint32_t> depth_of(M, UINT32_MAX);
        for (size_t d = 0; d + 1 < depth_first.size(); d++) {
          if (depth_first[d] > depth_first[d + 1]) return fail("depth offsets not monotone", s, C, m);
          for (uint32_t i = depth_first[d]; i < depth_first[d + 1]; i++) {
            const uint32_t slot = depth_slots[i];
            if (slot < C || slot - C >= M || depth_of[slot - C] != UINT32_MAX) return fail("a slot twice in the depth lists", s, C, m);
            depth_of[slot - C] = (uint32_t) d;
          }
        }
        for (uint32_t slot : slots[m]) if (depth_of[slot - C] == UINT32_MAX) return fail("a slot missing from the depth lists", s, C, m);
        if (depth_slots[0] != mesh_root[m] || depth_first[1] != 1) return fail("depth 0 is not the root alone", s, C, m);
        // 3
        for (uint32_t slot : slots[m])
          for (int k = 0; k < 4; k++) {
            const uint32_t c = nodes[slot].child[k];
            if (c == kBvhEmpty || (c & kBvhLeafBit)) continue;
            if (c < C || c - C >= M || depth_of[c - C] != depth_of[slot - C] + 1) return fail("an inner child is not one depth below its parent", s, C, m);
          }
        // 4: the twin of k_refit_tri_boxes' output and k_refit_level_resident's loop
        const uint32_t t0 = offset[m], count = scenes[s][m];
        std::vector<Aabb> prim_box(count);
        for (uint32_t i = 0; i < count; i++) prim_box[i] = to[m][built[m].prims[i]];
        for (size_t d = depth_first.size() - 1; d-- > 0;)
          for (uint32_t i = depth_first[d]; i < depth_first[d + 1]; i++) {
            const uint32_t slot = depth_slots[i];
            Bvh4Node& node = nodes[slot];
            Aabb all = empty_box();
            for (int k = 0; k < 4; k++) {
              const uint32_t c = node.child[k];
              if (c == kBvhEmpty) continue;
              Aabb box;
              if (c & kBvhLeafBit) {
                box = empty_box();
                const uint32_t tri = c & 0x0FFFFFFFu, cnt = ((c >> 28) & 7u) + 1u;
                if (tri < t0 || tri - t0 + cnt > count) return fail("a leaf range outside the mesh's triangles", s, C, m);
                for (uint32_t j = 0; j < cnt; j++) grow(box, prim_box[tri - t0 + j]);
              }
              else box = slot_box[c - C];
              set_child_box(node, k, box);
              grow(all, box);
            }
            slot_box[slot - C] = all;
          }
        // 5
        uint32_t lo = UINT32_MAX, hi = 0;
        for (uint32_t slot : slots[m]) { lo = std::min(lo, slot); hi = std::max(hi, slot); }
        const bool split = (size_t) hi - lo + 1 > slots[m].size();
        if (count == 30000 && nm > 1 && C == 4000) {
          if (!split) return fail("the large mesh's slots are a range: the case this check is for did not occur", s, C, m);
          saw_split = true;
        }
      }
      if (std::memcmp(nodes.data(), want.data(), sizeof(Bvh4Node) * nodes.size()) != 0) return fail("the refit in the laid-out array differs from the layout of the refitted trees", s, C, 0);
    }
  }
  if (!saw_split) return fail("no mesh with split slots was checked", 0, 0, 0);
  std::printf("resident_refit_check: ok\n");
  return 0;
}
