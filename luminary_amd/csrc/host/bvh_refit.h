// GPU refit of a mesh's tree (bvh_refit.hip): what a context keeps on its device per deformable mesh, and the two calls of the scene update (core.hip).
#pragma once

#include <hip/hip_runtime_api.h>

#include <vector>

#include "bvh_build.h"
#include "device_buffer.h"

#pragma GCC visibility push(hidden)

namespace lum {

// A tree's topology on the device, from the first refit of the mesh on: later refits upload nothing. Owned by one context; the buffers live on its device.
struct RefitPlan {
  DeviceBuffer<Bvh4Node> nodes;        // mesh-relative node array: child words as built, boxes of the last refit
  DeviceBuffer<uint32_t> prims;        // primitive ids in leaf order
  DeviceBuffer<uint32_t> level_nodes;  // node ids by level, root first (bvh4_levels)
  DeviceBuffer<Aabb> node_box;         // scratch: every node's exact box, written by its level's launch and read by the level above
  DeviceBuffer<Aabb> prim_box;         // scratch: the primitives' boxes in leaf order
  std::vector<uint32_t> level_first;   // levels + 1 offsets into level_nodes
  uint32_t num_nodes = 0, count = 0;
  void reset() { nodes.reset(); prims.reset(); level_nodes.reset(); node_box.reset(); prim_box.reset(); level_first.clear(); num_nodes = count = 0; }
};

// Uploads the topology of `tree` (count primitives) to the current device. hipErrorInvalidValue for a tree that cannot be refitted.
hipError_t refit_plan_create(RefitPlan& plan, const Bvh4& tree, uint32_t count);
// One refit on the current device. The primitives' boxes come from d_vertices (the mesh's first vertex in the device scene: 3 float4 per triangle), in which
// case the 9 geometry floats of the mesh's traversal triangles d_tris (leaf order) are rewritten too, or - d_vertices null - from host_boxes (by primitive id).
// out_nodes receives plan.num_nodes refitted nodes, root_box the exact box of everything. Synchronises the device. download_seconds (optional): the host's wall
// clock from the last launch to the end of the copies, i.e. the wait for the kernels and the download.
hipError_t refit_run(RefitPlan& plan, const float4* d_vertices, BvhTri* d_tris, const Aabb* host_boxes, Bvh4Node* out_nodes, Aabb* root_box, double* download_seconds = nullptr);

}  // namespace lum

#pragma GCC visibility pop
