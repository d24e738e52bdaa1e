// Host side of the software traversal's trees, which replace the reference's OptiX acceleration structures
// (reference: src/luminary/device/optix_bvh.c:150-684 builds GAS/IAS through optixAccelBuild).
// The builders - binned SAH on the CPU (bvh_build.cpp; the fallback and the particle / light / top-level trees) and LBVH, PLOC and binned SAH on the GPU
// (lbvh.hip; the default for meshes) - all collapse a binary tree into 128-byte 4-wide nodes: the node/triangle layout consumed by the kernels does
// not depend on the builder. Below them, the assembly of the per-mesh trees and the instances into the scene's one node array (bvh_build.cpp; no HIP call).
#pragma once

#include <cstddef>
#include <algorithm>
#include <cstdint>
#include <thread>
#include <vector>

#include "../../../include/lum_core.h"
#include "../device/dev_scene.h"

namespace lum {

struct Aabb { float lo[3], hi[3]; };

struct Bvh4 {
  std::vector<Bvh4Node> nodes;   // nodes[0] is the root and always an inner node
  std::vector<uint32_t> prims;   // primitive ids in leaf order; leaves reference ranges of this array
  uint32_t max_depth = 0;
  // test support (lumc_host_bvh_probe): the cost the collapse plan reports for the root (sum of the surviving binary nodes' half areas), and - for trees of at
  // most 20 binary inner nodes, LUM_BVH_COLLAPSE_BRUTE=1 - the cheapest of ALL valid choices of surviving nodes, found by trying every subset
  double plan_cost = 0.0, brute_cost = -1.0;
};

// Builds a BVH4 over `count` boxes. Leaves hold at most `max_leaf` (<= kBvhLeafMaxTri) primitives. The tree has at most
// `max_depth` BVH4 levels (the kernels' traversal stack is sized for that): a SAH tree that is deeper is rebuilt with median
// splits; if that is still too deep the result is empty (nodes.empty()).
Bvh4 build_bvh4(const Aabb* boxes, uint32_t count, uint32_t max_leaf = kBvhLeafMaxTri, uint32_t max_depth = 20);

// The same tree with spatial splits (Stich, Friedrich, Dietrich: "Spatial Splits in Bounding Volume Hierarchies", HPG 2009): where the best object
// split leaves the children's boxes overlapping, the set is also tried cut by a plane, triangles that straddle it referenced on both sides with their
// boxes clipped to each side. `vertices` = 3 x float4 per triangle (the device scene's layout); `splittable[i] == 0` keeps triangle i in one leaf (a
// visibility ray multiplies the transparency of every triangle reference it crosses, so only opaque triangles may be referenced twice - for those,
// and for closest hits, a second reference changes nothing: same distance, same ids). prims then holds one entry per REFERENCE (prims.size() >= count).
// Opt-in (LUM_BVH_SPATIAL=1): the benchmark meshes are evenly tessellated and gain nothing (tools/bvh_quality.cpp), long thin triangles do.
Bvh4 build_bvh4_triangles(const float* vertices, const Aabb* boxes, const uint8_t* splittable, uint32_t count, uint32_t max_leaf = kBvhLeafMaxTri, uint32_t max_depth = 20);

// Same contract, built on the current HIP device (lbvh.hip): Morton-ordered binary radix tree collapsed to 4-wide nodes. Much faster to
// build, somewhat slower to trace. Returns an empty result when the tree is deeper than `max_depth` or a HIP call fails; the caller
// then falls back to build_bvh4.
Bvh4 build_bvh4_lbvh(const Aabb* boxes, uint32_t count, uint32_t max_leaf = kBvhLeafMaxTri, uint32_t max_depth = 20);
// The same on the device with parallel locally-ordered clustering (bottom-up merges of nearest neighbours in Morton order) instead of the radix
// tree: two to three times the LBVH's build time, trees between its quality and the SAH builder's.
Bvh4 build_bvh4_ploc(const Aabb* boxes, uint32_t count, uint32_t max_leaf = kBvhLeafMaxTri, uint32_t max_depth = 20);

// The host builder's binned SAH, level by level on the device (lbvh.hip): for meshes without degenerate sets the same binary tree and leaf order as
// build_bvh4, in tens of milliseconds. Empty result when the tree is deeper than `max_depth` 4-wide levels or a HIP call fails (the caller falls back).
Bvh4 build_bvh4_sah_gpu(const Aabb* boxes, uint32_t count, uint32_t max_leaf = kBvhLeafMaxTri, uint32_t max_depth = 20);
// Its device-in / device-out core (build_bvh4_sah_gpu is upload + this + download): count >= 2 boxes already on the current device; the nodes are left on the
// device at d_nodes_out[0, *num_nodes) (false, and nothing written, when they are more than node_capacity), the primitive ids in leaf order at d_prims_out[0, count).
// False when the tree is deeper than max_depth or a HIP call fails. Synchronises the device (one counter download per level).
bool build_bvh4_sah_device(const Aabb* d_boxes, uint32_t count, uint32_t max_leaf, uint32_t max_depth, Bvh4Node* d_nodes_out, uint32_t node_capacity, uint32_t* d_prims_out,
                           uint32_t* num_nodes, uint32_t* depth);

// ---- refit: new boxes under an unchanged topology (moved vertices, luminary_ext_set_mesh_positions) ----
// The tree with the same child words, prims and max_depth; every occupied child box = the builders' pad of the exact union (min / max) of the primitive boxes
// below it, empty slots keep their +-FLT_MAX boxes. root_box: the exact union of everything. A tree with prims.size() != count (spatial splits: clipped
// reference boxes are not a function of the primitives' boxes) cannot be refitted: the result is empty and the caller builds. Host twin of bvh_refit.hip.
Bvh4 refit_bvh4(const Bvh4& tree, const Aabb* boxes, uint32_t count, Aabb* root_box = nullptr);
// Sum over all nodes, in node order, and their occupied child slots of the child box's half surface area, in double from the stored (padded) floats: what the
// expected number of node visits of a random ray is proportional to. Defined for any tree; a refit is judged by its growth over the tree as built.
double bvh4_cost(const Bvh4& tree);
// Every primitive of [0, count) sits in exactly one leaf, every child index and leaf range is in bounds, every child box holds what is below it.
bool bvh4_valid(const Bvh4& tree, const Aabb* boxes, uint32_t count);
// The nodes of `tree` by 4-wide level, root first (one breadth-first walk; the GPU builders number nodes through atomics, so levels are not index ranges):
// level l = level_nodes[level_first[l], level_first[l + 1]). False when a child index or a leaf range is out of bounds or a node is reached twice.
bool bvh4_levels(const Bvh4& tree, uint32_t count, std::vector<uint32_t>& level_nodes, std::vector<uint32_t>& level_first);

// ---- the scene's tree (scene upload, core.hip; lumc_scene_tree_probe) ----
// [0, n) in contiguous chunks over the host's cores (per-triangle loops of the scene upload: 10 M triangles are 100 ms each on one core)
template <class F>
void host_parallel_for(size_t n, F&& fn) {
  const unsigned hc = std::thread::hardware_concurrency();
  const unsigned threads = (unsigned) std::min<size_t>(std::min(std::max(hc, 1u), 32u), std::max<size_t>(n / 65536, 1));
  if (threads <= 1) { fn((size_t) 0, n); return; }
  const size_t chunk = (n + threads - 1) / threads;
  std::vector<std::thread> pool;
  for (unsigned t = 1; t < threads; t++) pool.emplace_back([&, t] { const size_t b = std::min(n, t * chunk), e = std::min(n, b + chunk); if (b < e) fn(b, e); });
  fn((size_t) 0, std::min(n, chunk));
  for (auto& th : pool) th.join();
}
Aabb tri_box(const float* a, const float* b, const float* c);
// Traversal triangle of three float4 vertices (12 floats): the edges by the float subtraction the reference's intersection code performs.
inline BvhTri bvh_tri(const float* p, uint32_t id, uint32_t scene_index, uint32_t albedo_tex) {
  BvhTri t;
  for (int k = 0; k < 3; k++) { t.p0[k] = p[k]; t.e1[k] = p[4 + k] - p[k]; t.e2[k] = p[8 + k] - p[k]; }
  t.id = id; t.scene_index = scene_index; t.albedo_tex = albedo_tex;
  return t;
}
// rows[i] = (m_i0, m_i1, m_i2, translation_i) of the world->object map of one instance (8 floats: translation, scale, packed rotation); the world box of an
// object-space box under the inverse of that map (false for a transform that cannot be inverted)
void instance_inverse_rows(const float* transform, float4 rows[3]);
bool instance_world_box(const float4 rows[3], const Aabb& object_box, Aabb& world_box);
// A mesh's `count` triangles (12 floats each): their boxes into tri_boxes (returns the mesh's box); the triangles in the leaf order of the mesh's tree
// (Bvh4::prims) into out[0, count), id = the triangle's index in the mesh, scene_index = first_tri + id.
Aabb mesh_triangle_boxes(const float* vertices, uint32_t count, Aabb* tri_boxes);
void fill_mesh_tris(const float* vertices, uint32_t first_tri, const uint32_t* prims, uint32_t count, BvhTri* out);

struct SceneTree {
  std::vector<Bvh4Node> nodes;      // top level, then every mesh's tree; absolute indices, the most visited nodes first (breadth first across both levels)
  uint32_t tlas_num_nodes = 0;      // nodes that belong to the top level (not a range of `nodes` after the renumbering: bookkeeping and the kernels' leaf test)
  std::vector<float4> tlas_leaves;  // 4 per top-level leaf in traversal order: the instance's rows, then {instance id, root of its mesh, 0, 0}; one record of padding
  std::vector<float4> inv_rows;     // 3 per instance, by instance id (+ 3 of padding)
  std::vector<uint32_t> mesh_root;  // node index of every mesh's root (+ 1 of padding)
  Aabb world;                       // bounds of the top level; the unit cube when nothing can be hit
};
// Top-level tree over the instances of `v` that can be hit (mesh id in range, mesh not empty, invertible transform), concatenated with the per-mesh trees
// (node indices relative to the mesh, leaf ranges relative to its first triangle) and renumbered. Empty (nodes.empty()) when the top level exceeds 16 levels.
SceneTree assemble_scene_tree(const LumDeviceSceneView& v, const Bvh4* const* mesh_bvh, const Aabb* mesh_box);

// The resident layout of the scene's node array (LUMC_DIRTY_INSTANCE_TRANSFORMS, instance_update.hip): slots [0, capacity) are the top level's - empty nodes here -,
// [capacity, capacity + M) hold every mesh's tree with absolute child indices and leaf ranges rebased by mesh_tri_offset, ordered so that the tops of the meshes
// come first (one breadth-first walk from the mesh roots while capacity + nodes stays within the 4096 of assemble_scene_tree, the rest in mesh order).
// mesh_root: num_meshes + 1 absolute indices. mesh_slots (optional): per mesh, the absolute slot of every mesh-relative node id - a mesh's nodes are NOT a range of
// the array: the tops of all meshes come first.
void layout_resident_nodes(const LumDeviceSceneView& v, const Bvh4* const* mesh_bvh, uint32_t capacity, std::vector<Bvh4Node>& nodes, std::vector<uint32_t>& mesh_root,
                           std::vector<std::vector<uint32_t>>* mesh_slots = nullptr);
// A mesh's slots in the resident array by depth below the mesh's root, root first (bvh4_levels through the slot map of layout_resident_nodes): depth d =
// depth_slots[depth_first[d], depth_first[d + 1]). What the refit in the resident array walks, deepest first (bvh_refit.hip k_refit_level_resident). False for a
// tree that cannot be refitted (bvh4_levels) or a slot map of another size.
bool resident_depth_slots(const Bvh4& tree, uint32_t count, const std::vector<uint32_t>& slots, std::vector<uint32_t>& depth_slots, std::vector<uint32_t>& depth_first);

}  // namespace lum
