// Who owns each array of the scene on the device: one typed DeviceBuffer per array, one sub-struct per part that lumc_scene_update replaces as a whole
// (`arrays.lights = {}` frees that part and nothing else). DeviceScene's pointers are views of these buffers (scene_device.hip points them); a write goes
// through the owner's get(). The tables a context generates and keeps across uploads (BSDF and sky tables, cloud noise, baked sky, bridge table) are not here
// but in LumContext. device_buffer.h's two rules hold. Host only: a plain C++ compiler with -D__HIP_PLATFORM_AMD__ takes it.
#pragma once

#include "bvh_build.h"
#include "device_buffer.h"

#pragma GCC visibility push(hidden)

namespace lum {

struct SceneArrays {
  // blas_tris: all meshes, traversal order; it stays where it is when vertices move (the refit and k_tri_opacity write into it)
  struct Mesh { DeviceBuffer<uint32_t> tri_offset; DeviceBuffer<float4> vertices; DeviceBuffer<uint4> tri_tex; DeviceBuffer<BvhTri> blas_tris; } mesh;
  // nodes: top level + every mesh's tree (InstanceUpdate::resident says how it is laid out); a re-layout replaces nodes and tlas_leaves and keeps the rest
  struct Inst { DeviceBuffer<uint32_t> mesh_ids; DeviceBuffer<float4> transforms, rows, tlas_leaves; DeviceBuffer<Bvh4Node> nodes; } inst;
  struct Materials { DeviceBuffer<uint4> materials; } materials;
  struct Lights {
    DeviceBuffer<uint4> tree_root, tree_nodes; DeviceBuffer<float> root_children; DeviceBuffer<uint2> tri_handles;
    DeviceBuffer<float4> tri_table;  // k_light_table's records: allocated with the part, refilled in place by a material or instance edit
    DeviceBuffer<Bvh4Node> bvh_nodes; DeviceBuffer<BvhTri> bvh_tris;
  } lights;
  struct Textures { DeviceBuffer<uint4> table; DeviceBuffer<uint32_t> texels; } textures;
  struct Constants {  // the caller's copies only (cloud noise: shape, detail, weather; sky tables: transmittance, multiscattering): empty where the context renders with its own
    DeviceBuffer<float4> stars; DeviceBuffer<uint32_t> stars_offsets, cloud_noise[3]; DeviceBuffer<float4> sky_lut[2], sky_hdri;
  } constants;
  struct Particles { DeviceBuffer<Bvh4Node> nodes; DeviceBuffer<BvhTri> tris; DeviceBuffer<float4> leaves, normals; } particles;
  DeviceBuffer<uint32_t> bluenoise_2d;  // uploaded once per context
};

}  // namespace lum

#pragma GCC visibility pop
