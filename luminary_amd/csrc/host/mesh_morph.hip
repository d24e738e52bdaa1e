// Morphed meshes on the device (lumc_mesh_morph_bind / _weights -> LUMC_DIRTY_MESH_SKIN): from the 4 bytes of every target's weight to the
// blended 16-byte records of the scene's vertex array, which k_refit_tri_boxes and the shading kernels read - without the host touching a vertex. The arithmetic
// is mesh_morph.h's morph_corner (and, for a mesh that is skinned too, mesh_skin.h's skin_corner over its result), the same sources the host twin
// (mesh_morph.cpp) is compiled from; this unit is compiled without contraction like that one, IEEE divide and square root: both give the same bytes
// (lumc_morph_host, tests/test_mesh_morph_gpu.py).
//
//   k_morph_mesh<skin>  one thread per corner in a grid-stride loop. The T weights are staged once per workgroup in LDS (<= 4 KB), with a skin the palette behind
//                       them as k_skin_mesh stages it (<= 48 KB): <= 52 KB, below the 64 KB a workgroup gets without asking. Per corner two 16-byte loads of
//                       the base shape and the row's two bounds, each contiguous over the wave, with a skin its planes 1 and 2 (ids, weights); then the corner's
//                       entries, two 16-byte loads each, in the order the bind laid them out - ascending targets, no atomics, no scatter: the order of the
//                       additions is the layout's. Rows differ in length, so a wave runs as long as its longest row. One 16-byte store. Every row bound is
//                       checked against the entry count, every target id against T, every bone id against the bone count and every corner against the corner
//                       count the host passed; what is out of range and a coordinate that is not finite set a flag word with one plain atomic per thread,
//                       which the update reads back.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../../include/lum_core.h"
#include "mesh_morph.h"

namespace lum {
namespace {

constexpr uint32_t kMorphBlock = 256;
constexpr uint32_t kMorphMaxBlocks = 1024;  // 4 per CU, as k_skin_mesh: a 52 KB stage is filled at most that often, whatever the mesh's size

// base: [2][corners]; row: [corners + 1]; entries: 2 float4 per entry; weights: target_count floats; skin_rest: the skin's [3][corners] planes (mesh_skin.h; planes
// 1 and 2 are read); palette: 3 float4 per bone; out: corners records of the scene's vertex array.
template <bool kSkin>
__global__ __launch_bounds__(kMorphBlock) void k_morph_mesh(const float4* __restrict__ base, const uint32_t* __restrict__ row, const float4* __restrict__ entries,
                                                           uint32_t entry_count, uint32_t corners, const float* __restrict__ weights, uint32_t target_count,
                                                           const float4* __restrict__ skin_rest, const float4* __restrict__ palette, uint32_t bone_count,
                                                           float4* __restrict__ out, uint32_t* __restrict__ flags) {
  extern __shared__ float4 s_stage[];  // (target_count + 3) / 4 words of weights, then 3 * bone_count of palette
  float* s_weights = reinterpret_cast<float*>(s_stage);
  const float4* s_palette = s_stage + (target_count + 3u) / 4u;
  for (uint32_t k = threadIdx.x; k < target_count; k += kMorphBlock) s_weights[k] = weights[k];
  if (kSkin)
    for (uint32_t k = threadIdx.x; k < 3u * bone_count; k += kMorphBlock) s_stage[(target_count + 3u) / 4u + k] = palette[k];
  __syncthreads();
  uint32_t flag = 0;
  for (uint32_t c = blockIdx.x * kMorphBlock + threadIdx.x; c < corners; c += gridDim.x * kMorphBlock) {
    const float4 a = base[c], b = base[(size_t) corners + c];
    uint32_t first = row[c], last = row[c + 1];
    if (first > last || last > entry_count) { first = last = 0; flag |= kMorphFlagBadLayout; }  // (the bind builds the rows itself: never taken)
    const float bn[3] = {a.w, b.x, b.y};
    float p[3] = {a.x, a.y, a.z}, n[3] = {bn[0], bn[1], bn[2]};
    const uint32_t used = morph_corner(p, n, first, last,
                                       [&](uint32_t k, float dp[3], float dn[3]) {
                                         const float4 e0 = entries[2 * (size_t) k], e1 = entries[2 * (size_t) k + 1];
                                         dp[0] = e0.x; dp[1] = e0.y; dp[2] = e0.z; dn[0] = e1.x; dn[1] = e1.y; dn[2] = e1.z;
                                         return __float_as_uint(e0.w);
                                       },
                                       [&](uint32_t t) {
                                         if (t >= target_count) { flag |= kMorphFlagBadLayout; return 0.0f; }  // (the bind writes the ids itself: never taken)
                                         return s_weights[t];
                                       });
    float op[3], on[3];
    if (kSkin) {
      const float4 s1 = skin_rest[(size_t) corners + c], w4 = skin_rest[2 * (size_t) corners + c];
      const uint32_t i01 = __float_as_uint(s1.z), i23 = __float_as_uint(s1.w);
      uint32_t id[4] = {i01 & 0xFFFFu, i01 >> 16, i23 & 0xFFFFu, i23 >> 16};
      float w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (id[j] >= bone_count) { id[j] = 0; w[j] = 0.0f; flag |= kSkinFlagBadBone; }  // (the bind refuses such ids: never read)
      flag |= skin_corner(p, n, w, [&](int j, float m[12]) {
        const float4 r0 = s_palette[3 * id[j]], r1 = s_palette[3 * id[j] + 1], r2 = s_palette[3 * id[j] + 2];
        m[0] = r0.x; m[1] = r0.y; m[2] = r0.z; m[3] = r0.w;
        m[4] = r1.x; m[5] = r1.y; m[6] = r1.z; m[7] = r1.w;
        m[8] = r2.x; m[9] = r2.y; m[10] = r2.z; m[11] = r2.w;
      }, op, on);
    }
    else {
      morph_normal(bn, n, used, on);
      op[0] = p[0]; op[1] = p[1]; op[2] = p[2];
      if (!(skin_finite(p[0]) && skin_finite(p[1]) && skin_finite(p[2]))) flag |= kSkinFlagNotFinite;
    }
    out[c] = make_float4(op[0], op[1], op[2], __uint_as_float(skin_pack_normal(on)));
  }
  if (flag) atomicOr(flags, flag);
}

}  // namespace

hipError_t mesh_morph_upload(MeshMorph& morph, const float* base_positions, const float* base_normals, uint32_t triangle_count, uint32_t target_count, const uint32_t* offsets,
                             const uint32_t* corners, const float* delta_positions, const float* delta_normals) {
  const size_t corner_count = 3 * (size_t) triangle_count;
  std::vector<float4> base(2 * corner_count);
  for (size_t c = 0; c < corner_count; c++) {
    const float *p = base_positions + 3 * c, *n = base_normals + 3 * c;
    base[c] = make_float4(p[0], p[1], p[2], n[0]);
    base[corner_count + c] = make_float4(n[1], n[2], 0.0f, 0.0f);
  }
  MorphCsr csr;
  morph_csr(triangle_count, target_count, offsets, corners, delta_positions, delta_normals, &csr);
  static_assert(sizeof(float4) == 4 * sizeof(float), "an entry is two 16-byte words");
  morph.triangles = triangle_count; morph.target_count = target_count; morph.entry_count = offsets[target_count]; morph.applied = false; morph.pending.clear();
  hipError_t e = morph.base.assign(base.data(), base.size());
  if (e != hipSuccess) return e;
  if ((e = morph.row.assign(csr.row.data(), csr.row.size())) != hipSuccess) return e;
  if ((e = morph.entries.assign(reinterpret_cast<const float4*>(csr.entries.data()), csr.entries.size() / 4)) != hipSuccess) return e;
  const std::vector<float> zero(target_count, 0.0f);
  return morph.weights.assign(zero.data(), zero.size());
}

hipError_t mesh_morph_launch(const MeshMorph& morph, const MeshSkin* skin, float4* d_vertices, uint32_t* d_flags) {
  const uint32_t corners = 3u * morph.triangles;
  if (corners == 0) return hipSuccess;
  if (!d_vertices || !d_flags || morph.target_count == 0 || morph.target_count > kMorphMaxTargets || morph.base.count() != 2 * (size_t) corners ||
      morph.row.count() != (size_t) corners + 1 || morph.entries.count() != 2 * (size_t) morph.entry_count || morph.weights.count() != morph.target_count)
    return hipErrorInvalidValue;
  if (skin && (skin->triangles != morph.triangles || skin->bone_count == 0 || skin->bone_count > kSkinMaxBones || skin->rest.count() != 3 * (size_t) corners ||
               skin->palette.count() != 3 * (size_t) skin->bone_count))
    return hipErrorInvalidValue;
  const uint32_t blocks = std::min<uint32_t>((corners + kMorphBlock - 1) / kMorphBlock, kMorphMaxBlocks);
  const size_t lds = sizeof(float4) * ((morph.target_count + 3u) / 4u + (skin ? 3 * (size_t) skin->bone_count : 0));
  if (skin)
    hipLaunchKernelGGL(k_morph_mesh<true>, dim3(blocks), dim3(kMorphBlock), lds, 0, (const float4*) morph.base.get(), (const uint32_t*) morph.row.get(),
                       (const float4*) morph.entries.get(), morph.entry_count, corners, (const float*) morph.weights.get(), morph.target_count,
                       (const float4*) skin->rest.get(), (const float4*) skin->palette.get(), skin->bone_count, d_vertices, d_flags);
  else
    hipLaunchKernelGGL(k_morph_mesh<false>, dim3(blocks), dim3(kMorphBlock), lds, 0, (const float4*) morph.base.get(), (const uint32_t*) morph.row.get(),
                       (const float4*) morph.entries.get(), morph.entry_count, corners, (const float*) morph.weights.get(), morph.target_count,
                       (const float4*) nullptr, (const float4*) nullptr, 0u, d_vertices, d_flags);
  return hipGetLastError();
}

}  // namespace lum
