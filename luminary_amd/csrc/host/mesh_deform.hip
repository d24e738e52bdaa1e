// Deformed meshes on the device (lumc_mesh_skin_bind / _pose, lumc_mesh_morph_bind / _weights -> LUMC_DIRTY_MESH_SKIN; DESIGN.md sections 11 and 12): from the 48
// bytes of every bone and the 4 bytes of every target's weight to the 16-byte records of the scene's vertex array, which k_refit_tri_boxes and the shading kernels
// read - without the host touching a vertex. The arithmetic is mesh_deform.h's deform_corner, the same source the host twin (mesh_deform.cpp) is compiled from; this
// unit is compiled without contraction like that one, IEEE divide and square root: both give the same bytes (lumc_skin_host, lumc_morph_host,
// tests/test_mesh_skin_gpu.py, tests/test_mesh_morph_gpu.py).
//
//   k_deform_mesh<morph, skin>  one thread per corner in a grid-stride loop; skin only, morph only, or both. Staged once per workgroup in LDS: with a morph the T
//                       weights (<= 4 KB), with a skin the palette behind them (3 x 16 B per bone, <= 48 KB; the ids are a per-lane gather): <= 52 KB, below
//                       the 64 KB a workgroup gets without asking. Per corner two 16-byte loads of the rest shape - the morph's base, or without a morph planes 0
//                       and 1 of the skin's rest data -, each contiguous over the wave; with a morph the row's two bounds, then the corner's entries, two 16-byte
//                       loads each, in the order the bind laid them out - ascending targets, no atomics, no scatter: the order of the additions is the
//                       layout's; rows differ in length, so a wave runs as long as its longest row. With a skin its planes 1 (ids) and 2 (weights) - plane 1 is
//                       the rest shape's second load when there is no morph: three loads in all. One 16-byte store. Every row bound is checked against the
//                       entry count, every target id against T, every bone id against the bone count and every corner against the corner count the host
//                       passed; what is out of range and a coordinate that is not finite set a flag word with one plain atomic per thread, which the update
//                       reads back.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../../include/lum_core.h"
#include "mesh_deform.h"

namespace lum {
namespace {

constexpr uint32_t kDeformBlock = 256;
constexpr uint32_t kDeformMaxBlocks = 1024;  // 4 per CU: a 52 KB stage is filled at most that often, whatever the mesh's size

// base: [2][corners]; row: [corners + 1]; entries: 2 float4 per entry; weights: target_count floats (all four of the morph: unused without one, target_count 0);
// skin_rest: the skin's [3][corners] planes (with a morph planes 1 and 2 are read); palette: 3 float4 per bone; out: corners records of the scene's vertex array.
template <bool kMorph, bool kSkin>
__global__ __launch_bounds__(kDeformBlock) void k_deform_mesh(const float4* __restrict__ base, const uint32_t* __restrict__ row, const float4* __restrict__ entries,
                                                             uint32_t entry_count, uint32_t corners, const float* __restrict__ weights, uint32_t target_count,
                                                             const float4* __restrict__ skin_rest, const float4* __restrict__ palette, uint32_t bone_count,
                                                             float4* __restrict__ out, uint32_t* __restrict__ flags) {
  extern __shared__ float4 s_stage[];  // (target_count + 3) / 4 words of weights, then 3 * bone_count of palette
  const uint32_t palette_at = kMorph ? (target_count + 3u) / 4u : 0u;
  float* s_weights = reinterpret_cast<float*>(s_stage);
  const float4* s_palette = s_stage + palette_at;
  if (kMorph)
    for (uint32_t k = threadIdx.x; k < target_count; k += kDeformBlock) s_weights[k] = weights[k];
  if (kSkin)
    for (uint32_t k = threadIdx.x; k < 3u * bone_count; k += kDeformBlock) s_stage[palette_at + k] = palette[k];
  __syncthreads();
  uint32_t flag = 0;
  for (uint32_t c = blockIdx.x * kDeformBlock + threadIdx.x; c < corners; c += gridDim.x * kDeformBlock) {
    const float4 a = kMorph ? base[c] : skin_rest[c], b = kMorph ? base[(size_t) corners + c] : skin_rest[(size_t) corners + c];
    uint32_t first = 0, last = 0;
    if (kMorph) {
      first = row[c]; last = row[c + 1];
      if (first > last || last > entry_count) { first = last = 0; flag |= kMorphFlagBadLayout; }  // (the bind builds the rows itself: never taken)
    }
    const float p[3] = {a.x, a.y, a.z}, n[3] = {a.w, b.x, b.y};
    float op[3], on[3];
    flag |= deform_corner(p, n, kMorph, first, last,
                          [&](uint32_t k, float dp[3], float dn[3]) {
                            const float4 e0 = entries[2 * (size_t) k], e1 = entries[2 * (size_t) k + 1];
                            dp[0] = e0.x; dp[1] = e0.y; dp[2] = e0.z; dn[0] = e1.x; dn[1] = e1.y; dn[2] = e1.z;
                            return __float_as_uint(e0.w);
                          },
                          [&](uint32_t t) {
                            if (t >= target_count) { flag |= kMorphFlagBadLayout; return 0.0f; }  // (the bind writes the ids itself: never taken)
                            return s_weights[t];
                          },
                          kSkin,
                          [&](uint32_t id[4], float w[4]) {
                            const float4 s1 = kMorph ? skin_rest[(size_t) corners + c] : b, w4 = skin_rest[2 * (size_t) corners + c];
                            const uint32_t i01 = __float_as_uint(s1.z), i23 = __float_as_uint(s1.w);
                            id[0] = i01 & 0xFFFFu; id[1] = i01 >> 16; id[2] = i23 & 0xFFFFu; id[3] = i23 >> 16;
                            w[0] = w4.x; w[1] = w4.y; w[2] = w4.z; w[3] = w4.w;
#pragma unroll
                            for (int j = 0; j < 4; j++)
                              if (id[j] >= bone_count) { id[j] = 0; w[j] = 0.0f; flag |= kSkinFlagBadBone; }  // (the bind refuses such ids: never read)
                          },
                          [&](uint32_t id, float m[12]) {
                            const float4 r0 = s_palette[3 * id], r1 = s_palette[3 * id + 1], r2 = s_palette[3 * id + 2];
                            m[0] = r0.x; m[1] = r0.y; m[2] = r0.z; m[3] = r0.w;
                            m[4] = r1.x; m[5] = r1.y; m[6] = r1.z; m[7] = r1.w;
                            m[8] = r2.x; m[9] = r2.y; m[10] = r2.z; m[11] = r2.w;
                          },
                          op, on);
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

hipError_t mesh_deform_launch(const MeshDeform& d, float4* d_vertices, uint32_t* d_flags) {
  const MeshMorph* morph = d.morph ? &*d.morph : nullptr;
  const MeshSkin* skin = d.skin_writes() ? &*d.skin : nullptr;
  if (!morph && !skin) return hipErrorInvalidValue;
  const uint32_t corners = 3u * (morph ? morph->triangles : skin->triangles);
  if (corners == 0) return hipSuccess;
  if (!d_vertices || !d_flags) return hipErrorInvalidValue;
  if (morph && (morph->target_count == 0 || morph->target_count > kMorphMaxTargets || morph->base.count() != 2 * (size_t) corners ||
                morph->row.count() != (size_t) corners + 1 || morph->entries.count() != 2 * (size_t) morph->entry_count || morph->weights.count() != morph->target_count))
    return hipErrorInvalidValue;
  if (skin && (3u * skin->triangles != corners || skin->bone_count == 0 || skin->bone_count > kSkinMaxBones || skin->rest.count() != 3 * (size_t) corners ||
               skin->palette.count() != 3 * (size_t) skin->bone_count))
    return hipErrorInvalidValue;
  const uint32_t blocks = std::min<uint32_t>((corners + kDeformBlock - 1) / kDeformBlock, kDeformMaxBlocks);
  const uint32_t targets = morph ? morph->target_count : 0u, bones = skin ? skin->bone_count : 0u;
  const size_t lds = sizeof(float4) * ((targets + 3u) / 4u + 3 * (size_t) bones);
  const auto kernel = !morph ? k_deform_mesh<false, true> : skin ? k_deform_mesh<true, true> : k_deform_mesh<true, false>;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kDeformBlock), lds, 0, morph ? (const float4*) morph->base.get() : nullptr, morph ? (const uint32_t*) morph->row.get() : nullptr,
                     morph ? (const float4*) morph->entries.get() : nullptr, morph ? morph->entry_count : 0u, corners, morph ? (const float*) morph->weights.get() : nullptr,
                     targets, skin ? (const float4*) skin->rest.get() : nullptr, skin ? (const float4*) skin->palette.get() : nullptr, bones, d_vertices, d_flags);
  return hipGetLastError();
}

}  // namespace lum
