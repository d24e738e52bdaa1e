// The host twin of k_deform_mesh (mesh_deform.hip): mesh_deform.h's deform_corner over a mesh's corners, plain C++ - no HIP, no device -, and the conversion of the
// caller's target-major lists into the corner-major CSR both walk. What the host layer materialises a posed or morphed mesh with, and what every test holds the
// kernel to, byte for byte (lum_core.h lumc_skin_host, lumc_morph_host).
#define LUM_DEFORM_HOST_ONLY 1
#include "mesh_deform.h"

namespace lum {

const char* morph_check(uint32_t triangle_count, uint32_t target_count, const uint32_t* offsets, const uint32_t* corners, const float* delta_positions, const float* delta_normals) {
  if (target_count == 0 || target_count > kMorphMaxTargets) return "target_count is 1 ... 1024";
  if (!offsets) return "a NULL array";
  if (offsets[0] != 0) return "offsets do not start at 0";
  for (uint32_t t = 0; t < target_count; t++)
    if (offsets[t + 1] < offsets[t]) return "offsets decrease";
  const size_t entries = offsets[target_count], corner_count = 3 * (size_t) triangle_count;
  if (entries > 0x7FFFFFFFu) return "more than 2^31 - 1 entries";
  if (entries && (!corners || !delta_positions)) return "a NULL array";
  for (uint32_t t = 0; t < target_count; t++)
    for (size_t k = offsets[t]; k < offsets[t + 1]; k++) {
      if (corners[k] >= corner_count) return "a corner index is not below 3 * triangle_count";
      if (k > offsets[t] && corners[k] <= corners[k - 1]) return "the corner indices of a target are not strictly increasing";
    }
  for (size_t i = 0; i < 3 * entries; i++)
    if (!skin_finite(delta_positions[i]) || (delta_normals && !skin_finite(delta_normals[i]))) return "a delta is not finite";
  return nullptr;
}

void morph_csr(uint32_t triangle_count, uint32_t target_count, const uint32_t* offsets, const uint32_t* corners, const float* delta_positions, const float* delta_normals,
               MorphCsr* out) {
  const size_t corner_count = 3 * (size_t) triangle_count, entries = offsets[target_count];
  out->row.assign(corner_count + 1, 0);
  out->entries.assign(8 * entries, 0.0f);
  for (size_t k = 0; k < entries; k++) out->row[corners[k] + 1]++;
  for (size_t c = 0; c < corner_count; c++) out->row[c + 1] += out->row[c];
  std::vector<uint32_t> next(out->row.begin(), out->row.end() - 1);
  for (uint32_t t = 0; t < target_count; t++)  // targets ascending: every corner's row fills in target order
    for (size_t k = offsets[t]; k < offsets[t + 1]; k++) {
      float* e = out->entries.data() + 8 * (size_t) next[corners[k]]++;
      e[0] = delta_positions[3 * k]; e[1] = delta_positions[3 * k + 1]; e[2] = delta_positions[3 * k + 2]; e[3] = skin_float(t);
      if (delta_normals) { e[4] = delta_normals[3 * k]; e[5] = delta_normals[3 * k + 1]; e[6] = delta_normals[3 * k + 2]; }
    }
}

void deform_host(const float* rest_positions, const float* rest_normals, const MorphCsr* csr, size_t first_corner, size_t corner_count, const float* morph_weights,
                 const uint16_t* bone_ids, const float* skin_weights, const float* bones, float* positions, float* normals, uint32_t* packed, uint64_t* not_finite) {
  if (!csr && !bones) return;
  uint64_t bad = 0;
  for (size_t c = 0; c < corner_count; c++) {
    // (copies: the outputs may be the inputs, as when the host layer poses a mesh whose rest pose it no longer needs)
    const float p[3] = {rest_positions[3 * c], rest_positions[3 * c + 1], rest_positions[3 * c + 2]};
    const float n[3] = {rest_normals[3 * c], rest_normals[3 * c + 1], rest_normals[3 * c + 2]};
    float op[3], on[3];
    const uint32_t flag = deform_corner(p, n, csr != nullptr, csr ? csr->row[first_corner + c] : 0u, csr ? csr->row[first_corner + c + 1] : 0u,
                                        [&](uint32_t k, float dp[3], float dn[3]) {
                                          const float* e = csr->entries.data() + 8 * (size_t) k;
                                          dp[0] = e[0]; dp[1] = e[1]; dp[2] = e[2]; dn[0] = e[4]; dn[1] = e[5]; dn[2] = e[6];
                                          return skin_bits(e[3]);
                                        },
                                        [&](uint32_t t) { return morph_weights[t]; },
                                        bones != nullptr,
                                        [&](uint32_t id[4], float w[4]) {
                                          for (int j = 0; j < 4; j++) { id[j] = bone_ids[4 * c + j]; w[j] = skin_weights[4 * c + j]; }
                                        },
                                        [&](uint32_t id, float m[12]) { memcpy(m, bones + 12 * (size_t) id, sizeof(float) * 12); },
                                        op, on);
    if (flag) bad++;
    if (positions) { positions[3 * c] = op[0]; positions[3 * c + 1] = op[1]; positions[3 * c + 2] = op[2]; }
    if (normals) { normals[3 * c] = on[0]; normals[3 * c + 1] = on[1]; normals[3 * c + 2] = on[2]; }
    if (packed) packed[c] = skin_pack_normal(on);
  }
  if (not_finite) *not_finite = bad;
}

// null inputs, a bone count outside 1 ... kSkinMaxBones, an id >= bone_count
static bool skin_refused(uint32_t triangle_count, const uint16_t* bone_ids, const float* weights, const float* bones, uint32_t bone_count) {
  if (bone_count == 0 || bone_count > kSkinMaxBones || !bones) return true;
  if (triangle_count && (!bone_ids || !weights)) return true;
  for (size_t i = 0; i < 12 * (size_t) triangle_count; i++) if (bone_ids[i] >= bone_count) return true;
  return false;
}

int skin_host(const float* rest_positions, const float* rest_normals, const uint16_t* bone_ids, const float* weights, uint32_t triangle_count, const float* bones,
              uint32_t bone_count, float* positions, float* normals, uint32_t* packed, uint64_t* not_finite) {
  if (not_finite) *not_finite = 0;
  if ((triangle_count && (!rest_positions || !rest_normals)) || skin_refused(triangle_count, bone_ids, weights, bones, bone_count)) return 1;
  deform_host(rest_positions, rest_normals, nullptr, 0, 3 * (size_t) triangle_count, nullptr, bone_ids, weights, bones, positions, normals, packed, not_finite);
  return 0;
}

void morph_host_csr(const float* base_positions, const float* base_normals, const MorphCsr& csr, size_t first_corner, size_t corner_count, const float* weights,
                    const uint16_t* bone_ids, const float* skin_weights, const float* bones, float* positions, float* normals, uint32_t* packed, uint64_t* not_finite) {
  deform_host(base_positions, base_normals, &csr, first_corner, corner_count, weights, bone_ids, skin_weights, bones, positions, normals, packed, not_finite);
}

int morph_host(const float* base_positions, const float* base_normals, uint32_t triangle_count, uint32_t target_count, const uint32_t* offsets, const uint32_t* corners,
               const float* delta_positions, const float* delta_normals, const float* weights, const uint16_t* bone_ids, const float* skin_weights, const float* bones,
               uint32_t bone_count, float* positions, float* normals, uint32_t* packed, uint64_t* not_finite) {
  if (not_finite) *not_finite = 0;
  if (!weights || (triangle_count && (!base_positions || !base_normals))) return 1;
  if (morph_check(triangle_count, target_count, offsets, corners, delta_positions, delta_normals)) return 1;
  for (uint32_t t = 0; t < target_count; t++) if (!skin_finite(weights[t])) return 1;
  if (bones && skin_refused(triangle_count, bone_ids, skin_weights, bones, bone_count)) return 1;
  MorphCsr csr;
  morph_csr(triangle_count, target_count, offsets, corners, delta_positions, delta_normals, &csr);
  deform_host(base_positions, base_normals, &csr, 0, 3 * (size_t) triangle_count, weights, bone_ids, skin_weights, bones, positions, normals, packed, not_finite);
  return 0;
}

}  // namespace lum

extern "C" int lumc_skin_host(const float* rest_positions, const float* rest_normals, const uint16_t* bone_ids, const float* weights, uint32_t triangle_count,
                              const float* bones, uint32_t bone_count, float* positions, float* normals, uint32_t* packed) {
  return lum::skin_host(rest_positions, rest_normals, bone_ids, weights, triangle_count, bones, bone_count, positions, normals, packed, nullptr);
}

extern "C" int lumc_morph_host(const float* base_positions, const float* base_normals, uint32_t triangle_count, uint32_t target_count, const uint32_t* offsets,
                               const uint32_t* corners, const float* delta_positions, const float* delta_normals, const float* weights, const uint16_t* bone_ids,
                               const float* skin_weights, const float* bones, uint32_t bone_count, float* positions, float* normals, uint32_t* packed) {
  return lum::morph_host(base_positions, base_normals, triangle_count, target_count, offsets, corners, delta_positions, delta_normals, weights, bone_ids, skin_weights, bones,
                         bone_count, positions, normals, packed, nullptr);
}
