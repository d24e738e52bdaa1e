// Skinned meshes on the device (lumc_mesh_skin_bind / _pose -> LUMC_DIRTY_MESH_SKIN): from the 48 bytes of every bone to the posed 16-byte
// records of the scene's vertex array, which k_refit_tri_boxes and the shading kernels read - without the host touching a vertex. The arithmetic is mesh_skin.h's
// skin_corner, the same source the host twin (mesh_skin.cpp) is compiled from; this unit is compiled without contraction like that one, IEEE divide and square
// root: both give the same bytes (lumc_skin_host, tests/test_mesh_skin_gpu.py).
//
//   k_skin_mesh  one thread per corner in a grid-stride loop: the palette staged once per workgroup in LDS (3 x 16 B per bone; the ids are a per-lane gather),
//                three 16-byte loads of rest data per corner, each contiguous over the wave, one 16-byte store. Every bone id is checked against the bone count
//                and every corner against the corner count the host passed; a posed coordinate that is not finite and an id out of range set a flag word with
//                a plain atomic, which the update reads back.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../../include/lum_core.h"
#include "mesh_skin.h"

namespace lum {
namespace {

constexpr uint32_t kSkinBlock = 256;
constexpr uint32_t kSkinMaxBlocks = 1024;  // 4 per CU: a 48 KB palette is staged at most that often, whatever the mesh's size

// rest: [3][corners] records (mesh_skin.h MeshSkin); palette: 3 float4 per bone; out: corners records of the scene's vertex array.
__global__ __launch_bounds__(kSkinBlock) void k_skin_mesh(const float4* __restrict__ rest, uint32_t corners, const float4* __restrict__ palette, uint32_t bone_count,
                                                         float4* __restrict__ out, uint32_t* __restrict__ flags) {
  extern __shared__ float4 s_palette[];  // 3 * bone_count
  for (uint32_t k = threadIdx.x; k < 3u * bone_count; k += kSkinBlock) s_palette[k] = palette[k];
  __syncthreads();
  uint32_t flag = 0;
  for (uint32_t c = blockIdx.x * kSkinBlock + threadIdx.x; c < corners; c += gridDim.x * kSkinBlock) {
    const float4 a = rest[c], b = rest[(size_t) corners + c], w4 = rest[2 * (size_t) corners + c];
    const float p[3] = {a.x, a.y, a.z}, n[3] = {a.w, b.x, b.y};
    const uint32_t i01 = __float_as_uint(b.z), i23 = __float_as_uint(b.w);
    uint32_t id[4] = {i01 & 0xFFFFu, i01 >> 16, i23 & 0xFFFFu, i23 >> 16};
    float w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (id[j] >= bone_count) { id[j] = 0; w[j] = 0.0f; flag |= kSkinFlagBadBone; }  // (the bind refuses such ids: never read)
    float op[3], on[3];
    flag |= skin_corner(p, n, w, [&](int j, float m[12]) {
      const float4 r0 = s_palette[3 * id[j]], r1 = s_palette[3 * id[j] + 1], r2 = s_palette[3 * id[j] + 2];
      m[0] = r0.x; m[1] = r0.y; m[2] = r0.z; m[3] = r0.w;
      m[4] = r1.x; m[5] = r1.y; m[6] = r1.z; m[7] = r1.w;
      m[8] = r2.x; m[9] = r2.y; m[10] = r2.z; m[11] = r2.w;
    }, op, on);
    out[c] = make_float4(op[0], op[1], op[2], __uint_as_float(skin_pack_normal(on)));
  }
  if (flag) atomicOr(flags, flag);
}

}  // namespace

hipError_t mesh_skin_upload(MeshSkin& skin, const float* rest_positions, const float* rest_normals, const uint16_t* bone_ids, const float* weights, uint32_t triangle_count,
                            uint32_t bone_count) {
  const size_t corners = 3 * (size_t) triangle_count;
  std::vector<float4> rest(3 * corners);
  for (size_t c = 0; c < corners; c++) {
    const float *p = rest_positions + 3 * c, *n = rest_normals + 3 * c, *w = weights + 4 * c;
    const uint16_t* id = bone_ids + 4 * c;
    rest[c] = make_float4(p[0], p[1], p[2], n[0]);
    rest[corners + c] = make_float4(n[1], n[2], skin_float((uint32_t) id[0] | ((uint32_t) id[1] << 16)), skin_float((uint32_t) id[2] | ((uint32_t) id[3] << 16)));
    rest[2 * corners + c] = make_float4(w[0], w[1], w[2], w[3]);
  }
  skin.triangles = triangle_count; skin.bone_count = bone_count; skin.posed = false; skin.pending.clear();
  hipError_t e = skin.rest.assign(rest.data(), rest.size());
  if (e != hipSuccess) return e;
  return skin.palette.resize(3 * (size_t) bone_count);
}

hipError_t mesh_skin_launch(const MeshSkin& skin, float4* d_vertices, uint32_t* d_flags) {
  const uint32_t corners = 3u * skin.triangles;
  if (corners == 0) return hipSuccess;
  if (!d_vertices || !d_flags || skin.bone_count == 0 || skin.bone_count > kSkinMaxBones || skin.rest.count() != 3 * (size_t) corners ||
      skin.palette.count() != 3 * (size_t) skin.bone_count)
    return hipErrorInvalidValue;
  const uint32_t blocks = std::min<uint32_t>((corners + kSkinBlock - 1) / kSkinBlock, kSkinMaxBlocks);
  hipLaunchKernelGGL(k_skin_mesh, dim3(blocks), dim3(kSkinBlock), sizeof(float4) * 3 * skin.bone_count, 0, (const float4*) skin.rest.get(), corners,
                     (const float4*) skin.palette.get(), skin.bone_count, d_vertices, d_flags);
  return hipGetLastError();
}

}  // namespace lum
