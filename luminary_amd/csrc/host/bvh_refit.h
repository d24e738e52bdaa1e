// GPU refit of a mesh's tree (bvh_refit.hip): what a context keeps on its device per deformable mesh, and the calls of the scene update (scene_device.hip).
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
// out_nodes - host memory, or device memory of the current device - receives plan.num_nodes refitted nodes, root_box the exact box of everything. Synchronises the device. download_seconds (optional): the host's wall
// clock from the last launch to the end of the copies, i.e. the wait for the kernels and the download.
hipError_t refit_run(RefitPlan& plan, const float4* d_vertices, BvhTri* d_tris, const Aabb* host_boxes, Bvh4Node* out_nodes, Aabb* root_box, double* download_seconds = nullptr);

// ---- refit where the nodes live: in the resident node array of instance_update.h (scene_device.hip refit_in_place) ----
constexpr uint32_t kResidentMaxDepths = 27;  // a mesh's tree has at most 26 4-wide levels

// What a context keeps on its device per deformable mesh from the mesh's first refit in the resident array until the layout is dropped. No node copy: the nodes
// are the scene's.
struct ResidentMesh {
  DeviceBuffer<uint32_t> slots;        // the mesh's slots in the resident array by depth below its root, root first (bvh_build.h resident_depth_slots)
  DeviceBuffer<uint32_t> prims;        // primitive ids in leaf order
  DeviceBuffer<Aabb> prim_box;         // scratch: the primitives' boxes in leaf order
  std::vector<uint32_t> depth_first;   // depths + 1 offsets into slots
  uint32_t num_nodes = 0, count = 0;
  void reset() { slots.reset(); prims.reset(); prim_box.reset(); depth_first.clear(); num_nodes = count = 0; }
};
// One moved mesh of an update as the kernels see it; a table of them is the second grid dimension of every launch.
struct ResidentJob {
  const uint32_t* slots;
  const Aabb* prim_box;
  uint32_t depth_first[kResidentMaxDepths + 1];
  uint32_t depths, num_nodes, first_tri, count, mesh, root_slot;
};
struct ResidentResult { Aabb box; double cost; };  // what comes back per moved mesh: the root's exact box and the cost of its nodes as refitted (32 B)

struct ResidentRefit {
  std::vector<std::vector<uint32_t>> mesh_slots;  // host, from the re-layout on: per mesh the slot of every mesh-relative node id (empty: no resident layout)
  uint32_t capacity = 0, mesh_nodes = 0;          // C, M of that layout (instance_update.h)
  std::vector<ResidentMesh> mesh;                 // by mesh; filled on a mesh's first refit in place
  DeviceBuffer<Aabb> slot_box;                    // scratch: the exact box of every node of [C, C + M), indexed by slot - C
  std::vector<uint32_t> batch;                    // the moved meshes the job table below was made for: an animation that moves the same meshes uploads it once
  std::vector<uint32_t> batch_first_tri;          // their first triangles in the scene
  DeviceBuffer<ResidentJob> jobs;
  DeviceBuffer<ResidentResult> results;
  DeviceBuffer<double> partials;                  // cost: one sum per workgroup, partial_stride per job
  uint32_t partial_stride = 0, widest = 0, depths = 0;  // of the batch: workgroups of its largest mesh, nodes of its widest depth, depths of its deepest mesh
  void drop_layout() { capacity = mesh_nodes = 0; mesh_slots.clear(); mesh.clear(); slot_box.reset(); batch.clear(); batch_first_tri.clear(); jobs.reset(); results.reset(); partials.reset(); partial_stride = widest = depths = 0; }
};

// The device side of one mesh (count primitives, first_tri = its first triangle in the scene) whose nodes sit at `slots`. hipErrorInvalidValue for a tree that
// cannot be refitted.
hipError_t resident_mesh_create(ResidentMesh& rm, const Bvh4& tree, uint32_t count, const std::vector<uint32_t>& slots);
// Everything an update of the meshes `moved` (each with a ResidentMesh) allocates and uploads, before any node is written: the slot scratch for mesh_nodes slots,
// the job table, the results. mesh_tri_offset: the host's. A failure leaves the node array as it was.
hipError_t resident_refit_prepare(ResidentRefit& r, const std::vector<uint32_t>& moved, const uint32_t* mesh_tri_offset, uint32_t mesh_nodes);
// The refit of the prepared batch: triangle boxes (and the traversal triangles' geometry) from d_vertices (the scene's first vertex) into d_tris (the scene's first
// traversal triangle), then one launch per depth, deepest first, over all moved meshes together into d_nodes[capacity, capacity + mesh_nodes); every moved mesh's
// root box into d_mesh_box[mesh]; then the cost of every moved mesh's nodes. out: one result per moved mesh, in the batch's order. Synchronises the device.
// launches: kernels launched; seconds[2]: host wall clock of the refit (device synchronised) and of the cost with its download.
hipError_t resident_refit_run(ResidentRefit& r, const float4* d_vertices, BvhTri* d_tris, Bvh4Node* d_nodes, uint32_t capacity, uint32_t mesh_nodes, Aabb* d_mesh_box,
                              uint32_t num_meshes, ResidentResult* out, uint32_t* launches, double seconds[2]);

}  // namespace lum

#pragma GCC visibility pop
