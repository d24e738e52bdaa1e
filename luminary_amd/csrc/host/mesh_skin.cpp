// The host twin of k_skin_mesh (mesh_skin.hip): mesh_skin.h's skin_corner over a mesh's corners, plain C++ - no HIP, no device. What the host layer materialises
// a posed mesh with, and what every test holds the kernel to, byte for byte (lum_core.h lumc_skin_host).
#define LUM_SKIN_HOST_ONLY 1
#include "mesh_skin.h"

namespace lum {

int skin_host(const float* rest_positions, const float* rest_normals, const uint16_t* bone_ids, const float* weights, uint32_t triangle_count, const float* bones,
              uint32_t bone_count, float* positions, float* normals, uint32_t* packed, uint64_t* not_finite) {
  if (not_finite) *not_finite = 0;
  if (bone_count == 0 || bone_count > kSkinMaxBones || !bones) return 1;
  if (triangle_count && (!rest_positions || !rest_normals || !bone_ids || !weights)) return 1;
  const size_t corners = 3 * (size_t) triangle_count;
  for (size_t i = 0; i < 4 * corners; i++) if (bone_ids[i] >= bone_count) return 1;
  uint64_t bad = 0;
  for (size_t c = 0; c < corners; c++) {
    // (copies: the outputs may be the inputs, as when the host layer poses a mesh whose rest pose it no longer needs)
    const float p[3] = {rest_positions[3 * c], rest_positions[3 * c + 1], rest_positions[3 * c + 2]};
    const float n[3] = {rest_normals[3 * c], rest_normals[3 * c + 1], rest_normals[3 * c + 2]};
    const uint16_t* id = bone_ids + 4 * c;
    float op[3], on[3];
    const uint32_t flag = skin_corner(p, n, weights + 4 * c, [&](int j, float m[12]) { memcpy(m, bones + 12 * (size_t) id[j], sizeof(float) * 12); }, op, on);
    if (flag) bad++;
    if (positions) { positions[3 * c] = op[0]; positions[3 * c + 1] = op[1]; positions[3 * c + 2] = op[2]; }
    if (normals) { normals[3 * c] = on[0]; normals[3 * c + 1] = on[1]; normals[3 * c + 2] = on[2]; }
    if (packed) packed[c] = skin_pack_normal(on);
  }
  if (not_finite) *not_finite = bad;
  return 0;
}

}  // namespace lum

extern "C" int lumc_skin_host(const float* rest_positions, const float* rest_normals, const uint16_t* bone_ids, const float* weights, uint32_t triangle_count,
                              const float* bones, uint32_t bone_count, float* positions, float* normals, uint32_t* packed) {
  return lum::skin_host(rest_positions, rest_normals, bone_ids, weights, triangle_count, bones, bone_count, positions, normals, packed, nullptr);
}
