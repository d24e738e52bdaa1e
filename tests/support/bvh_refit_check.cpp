// Stand-alone check of the host refit (csrc/host/bvh_build.cpp refit_bvh4, bvh4_cost, bvh4_valid), for a sanitizer build: compiled together with bvh_build.cpp
// by tests/test_mesh_refit.py with -fsanitize=address,undefined and run as a program of its own. Exits 0 when every case holds.
//   1. identity: a refit to the boxes the tree was built from returns the built nodes byte for byte, cost ratio exactly 1
//   2. hostile motion: unrelated boxes, all boxes collapsed to a point, half of them translated by 1e4 - valid trees, same child words and prims,
//      empty slots untouched
//   4. a tree whose prims do not match the box count cannot be refitted: empty result
#include <cfloat>
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
static int fail(const char* what, uint32_t n) { std::fprintf(stderr, "bvh_refit_check: %s (n = %u)\n", what, n); return 1; }

static int same_topology(const Bvh4& a, const Bvh4& b, uint32_t n) {
  if (a.nodes.size() != b.nodes.size() || a.prims != b.prims || a.max_depth != b.max_depth) return fail("sizes, prims or depth changed", n);
  for (size_t i = 0; i < a.nodes.size(); i++) {
    if (std::memcmp(a.nodes[i].child, b.nodes[i].child, sizeof(a.nodes[i].child)) != 0) return fail("child words changed", n);
    for (int k = 0; k < 4; k++) {
      if (a.nodes[i].child[k] != kBvhEmpty) continue;
      const Bvh4Node& x = b.nodes[i];
      if (x.lo_x[k] != FLT_MAX || x.lo_y[k] != FLT_MAX || x.lo_z[k] != FLT_MAX || x.hi_x[k] != -FLT_MAX || x.hi_y[k] != -FLT_MAX || x.hi_z[k] != -FLT_MAX) return fail("an empty slot was touched", n);
    }
  }
  return 0;
}

int main() {
  const uint32_t sizes[] = {1, 2, 3, 5, 257, 7500};
  for (uint32_t n : sizes) {
    const std::vector<Aabb> boxes = soup(n, n);
    const Bvh4 tree = build_bvh4(boxes.data(), n, kBvhLeafMaxTri, 26);
    if (tree.nodes.empty()) return fail("no tree", n);
    if (!bvh4_valid(tree, boxes.data(), n)) return fail("the built tree is not valid", n);
    // 1
    Aabb root;
    const Bvh4 same = refit_bvh4(tree, boxes.data(), n, &root);
    if (same.nodes.size() != tree.nodes.size() || std::memcmp(same.nodes.data(), tree.nodes.data(), sizeof(Bvh4Node) * tree.nodes.size()) != 0) return fail("identity refit differs from the build", n);
    if (bvh4_cost(same) != bvh4_cost(tree) || !(bvh4_cost(tree) > 0.0)) return fail("identity refit changes the cost", n);
    Aabb all = boxes[0];
    for (const Aabb& b : boxes) for (int k = 0; k < 3; k++) { all.lo[k] = std::min(all.lo[k], b.lo[k]); all.hi[k] = std::max(all.hi[k], b.hi[k]); }
    if (std::memcmp(&all, &root, sizeof(Aabb)) != 0) return fail("the root box is not the union of all boxes", n);
    // 2
    std::vector<Aabb> fresh = soup(n, n + 1000), point(n), half = boxes;
    for (Aabb& b : point) b = Aabb{{1.5f, -2.25f, 3.0f}, {1.5f, -2.25f, 3.0f}};
    for (uint32_t i = 0; i < n; i += 2) for (int k = 0; k < 3; k++) { half[i].lo[k] += 1e4f; half[i].hi[k] += 1e4f; }
    const std::vector<Aabb>* motions[3] = {&fresh, &point, &half};
    for (const std::vector<Aabb>* to : motions) {
      const Bvh4 moved = refit_bvh4(tree, to->data(), n);
      if (moved.nodes.empty()) return fail("refit refused a refittable tree", n);
      if (!bvh4_valid(moved, to->data(), n)) return fail("refitted tree is not valid", n);
      if (same_topology(tree, moved, n)) return 1;
    }
    // 4
    if (!refit_bvh4(tree, boxes.data(), n + 1).nodes.empty()) return fail("a tree with prims.size() != count was refitted", n);
    Bvh4 split = tree;
    split.prims.push_back(0u);  // what a spatial-split tree looks like: more references than primitives
    if (!refit_bvh4(split, boxes.data(), n).nodes.empty()) return fail("a tree with more references than primitives was refitted", n);
  }
  std::printf("bvh_refit_check: ok\n");
  return 0;
}
