// Moved instances on the device (instance_update.hip): what a context keeps for LUMC_DIRTY_INSTANCE_TRANSFORMS updates, and the calls of the scene update
// (scene_device.hip). The node array itself, the leaf records, the rows and the transforms belong to the scene (SceneArrays::inst).
#pragma once

#include <hip/hip_runtime_api.h>

#include "bvh_build.h"
#include "device_buffer.h"

#pragma GCC visibility push(hidden)

namespace lum {

// The resident layout's bookkeeping and the per-update scratch, sized for one instance count. Owned by one context; the buffers live on its device.
struct InstanceUpdate {
  bool resident = false;                 // sc.bvh_nodes is laid out as [0, C) top level, [C, C + M) mesh trees, and mesh_root names roots in it
  bool prepared = false;                 // the scratch below fits the scene on the device, mesh_box holds its meshes' boxes
  uint32_t capacity = 0, mesh_nodes = 0; // C, M
  uint32_t tlas_nodes = 0;               // T of the top level that is in [0, C) now
  uint32_t num_instances = 0, num_meshes = 0;
  DeviceBuffer<Aabb> mesh_box;           // by mesh, object space
  DeviceBuffer<uint32_t> mesh_root;      // by mesh: absolute index of the root in the resident array
  DeviceBuffer<Aabb> boxes, dense_boxes; // by instance / by rank among the instances that can be hit
  DeviceBuffer<uint32_t> flags, offsets, ids, prims;  // can be hit; exclusive scan of flags; instance id by rank; rank by top-level leaf
  DeviceBuffer<uint32_t> bounds;         // 6 order-encoded floats (lo[3], hi[3]) of the dense boxes' union, then their count
  DeviceBuffer<char> scan_temp;
  size_t scan_bytes = 0;
  void reset() {
    resident = prepared = false; capacity = mesh_nodes = tlas_nodes = num_instances = num_meshes = 0;
    mesh_box.reset(); mesh_root.reset(); boxes.reset(); dense_boxes.reset(); flags.reset(); offsets.reset(); ids.reset(); prims.reset(); bounds.reset(); scan_temp.reset();
    scan_bytes = 0;
  }
};

// The scratch for `num_instances` instances and the meshes' boxes (a host array of num_meshes entries) on the current device.
hipError_t instance_update_prepare(InstanceUpdate& u, uint32_t num_instances, uint32_t num_meshes, const Aabb* mesh_box);
// k_instance_rows_boxes over all instances (rows: 3 float4 per instance, written for every instance), the scan, the compaction into u.dense_boxes / u.ids and the
// bounds. *hittable and world (the unit cube for none) come back to the host: synchronises the device.
hipError_t instance_update_boxes(InstanceUpdate& u, const float4* d_transforms, const uint32_t* d_mesh_ids, const uint32_t* d_mesh_tri_offset, float4* d_rows,
                                 uint32_t* hittable, Aabb* world);
// The leaf records of `leaves` top-level leaves in leaf order (u.prims, u.ids) and one record of padding into d_leaves (room for num_instances + 1 records); empty
// nodes into d_nodes[clear_first, clear_end).
hipError_t instance_update_leaves(InstanceUpdate& u, uint32_t leaves, const float4* d_rows, const uint32_t* d_mesh_ids, float4* d_leaves, Bvh4Node* d_nodes,
                                  uint32_t clear_first, uint32_t clear_end);

}  // namespace lum

#pragma GCC visibility pop
