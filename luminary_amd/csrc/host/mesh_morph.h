// Morph targets (blend shapes) of a mesh's corners (lum_core.h lumc_mesh_morph_bind / lumc_mesh_morph_weights): the ONE definition of
// morph(base, deltas, weights), compiled twice - by the host compiler into mesh_morph.cpp (morph_host: the twin, no HIP in it) and by the device compiler into
// mesh_morph.hip (k_morph_mesh) - under -ffp-contract=off, so that both give the same bytes, the packed normal word included; what the context keeps per bound
// mesh; and the calls of the scene update (scene_device.hip).
//
// All of it is binary32, one rounding per operation, in this order. Per corner: a base position p and a base normal n, and the corner's entries (target t, dp, dn)
// IN ASCENDING TARGET ORDER. An entry whose weight w_t is 0 (-0 too) is skipped; every other one adds, per row r, p_r = p_r + w_t * dp_r and n_r = n_r + w_t * dn_r
// (a multiply, then an add). Then:
//   no skin, no contributing entry  the record is the base record: position and normal untouched, nothing normalised
//   no skin, contributing entries   len2 = (n.x * n.x + n.y * n.y) + n.z * n.z; a normal with len2 > 0 and finite is n * (1 / sqrtf(len2)), any other keeps the base normal
//   a skin on the same mesh         mesh_skin.h's skin_corner(p, n, w, bones) over the UN-normalised morphed p, n (the skin's own rest pose is not read)
// The device record is {x, y, z, skin_pack_normal(normal)}; a coordinate that is not finite sets kSkinFlagNotFinite.
#pragma once

#include <vector>

#include "mesh_skin.h"

namespace lum {

constexpr uint32_t kMorphMaxTargets = 1024;  // 4 KB of weights in LDS
constexpr uint32_t kMorphFlagBadLayout = 4u;  // next to kSkinFlagNotFinite / kSkinFlagBadBone: a target id beyond the target count or a row outside the entries

// The entries [first, last) of one corner onto p and n, in place. `entry(k, dp, dn)` fills the deltas of entry k and returns its target, `weight(t)` gives w_t.
// Returns the number of entries that contributed.
template <typename EntryOf, typename WeightOf>
LUM_SKIN_FN uint32_t morph_corner(float p[3], float n[3], uint32_t first, uint32_t last, EntryOf entry, WeightOf weight) {
  uint32_t used = 0;
  for (uint32_t k = first; k < last; k++) {
    float dp[3], dn[3];
    const uint32_t t = entry(k, dp, dn);
    const float w = weight(t);
    if (w == 0.0f) continue;  // (-0 too)
    LUM_SKIN_UNROLL
    for (int r = 0; r < 3; r++) {
      p[r] = p[r] + w * dp[r];
      n[r] = n[r] + w * dn[r];
    }
    used++;
  }
  return used;
}

// The normal of a morphed corner without a skin: `n` the morphed sum, `used` what morph_corner returned.
LUM_SKIN_FN void morph_normal(const float base_n[3], const float n[3], uint32_t used, float out_n[3]) {
  out_n[0] = base_n[0]; out_n[1] = base_n[1]; out_n[2] = base_n[2];
  if (used == 0) return;
  const float len2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
  if (len2 > 0.0f && skin_finite(len2)) {
    const float rl = 1.0f / ::sqrtf(len2);
    out_n[0] = n[0] * rl; out_n[1] = n[1] * rl; out_n[2] = n[2] * rl;
  }
}

// The caller's target-major lists - offsets[T + 1] into corners[E] / delta_positions[3E] / delta_normals[3E] (may be null: zero) - as the corner-major CSR both
// compilations walk: row[corners + 1], and per entry 8 floats {dp.x, dp.y, dp.z, target as bits, dn.x, dn.y, dn.z, 0}, a corner's entries in ascending target order.
struct MorphCsr {
  std::vector<uint32_t> row;
  std::vector<float> entries;
};
// Null when the lists can be bound, else what is wrong with them: T outside 1 ... kMorphMaxTargets, offsets that do not start at 0 or decrease, more than 2^31 - 1
// entries, a corner >= 3 * triangle_count, corners of a target not strictly increasing, a delta that is not finite.
const char* morph_check(uint32_t triangle_count, uint32_t target_count, const uint32_t* offsets, const uint32_t* corners, const float* delta_positions, const float* delta_normals);
void morph_csr(uint32_t triangle_count, uint32_t target_count, const uint32_t* offsets, const uint32_t* corners, const float* delta_positions, const float* delta_normals,
               MorphCsr* out);  // (lists morph_check took)

// The host twin (mesh_morph.cpp; no GPU). base_positions / base_normals: 9 floats per triangle; the lists as above; weights: T finite floats. With bones (12 floats
// each, bone_count 1 ... kSkinMaxBones) also bone_ids / skin_weights, 12 per triangle: the combined result. Every output may be null, and may be a base array.
// Returns 0, or 1 for null inputs, lists morph_check refuses, a weight that is not finite, or skin arguments skin_host refuses (nothing is written then);
// *not_finite (optional): corners with a coordinate that is not finite.
int morph_host(const float* base_positions, const float* base_normals, uint32_t triangle_count, uint32_t target_count, const uint32_t* offsets, const uint32_t* corners,
               const float* delta_positions, const float* delta_normals, const float* weights, const uint16_t* bone_ids, const float* skin_weights, const float* bones,
               uint32_t bone_count, float* positions, float* normals, uint32_t* packed, uint64_t* not_finite);
// The same over a CSR that is there already (what the host layer keeps per bound mesh), corners [first_corner, first_corner + corner_count) of it: the arrays other
// than the CSR start at first_corner.
void morph_host_csr(const float* base_positions, const float* base_normals, const MorphCsr& csr, size_t first_corner, size_t corner_count, const float* weights,
                    const uint16_t* bone_ids, const float* skin_weights, const float* bones, float* positions, float* normals, uint32_t* packed, uint64_t* not_finite);

}  // namespace lum

#if defined(__HIP_PLATFORM_AMD__) && !defined(LUM_SKIN_HOST_ONLY)

#pragma GCC visibility push(hidden)

namespace lum {

// A bound mesh on the context's device: the base shape as two planes of 16-byte records over the mesh's corners c - plane 0 {p.x, p.y, p.z, n.x}, plane 1 {n.y, n.z,
// 0, 0} -, the CSR (two 16-byte words per entry: {dp, target as bits}, {dn, 0}) and the T weights. Per corner 32 bytes of base and 8 of row are read and 16 written;
// per entry 32 bytes are read.
struct MeshMorph {
  DeviceBuffer<float4> base;      // [2][corners]
  DeviceBuffer<uint32_t> row;     // [corners + 1]
  DeviceBuffer<float4> entries;   // [2 * entry_count]
  DeviceBuffer<float> weights;    // [target_count]: the last weights that were applied (zero until then; kept for the re-apply after a vertex re-upload)
  std::vector<float> pending;     // the weights lumc_mesh_morph_weights recorded and no update has applied yet (empty: none)
  uint32_t triangles = 0, target_count = 0, entry_count = 0;
  bool applied = false;           // the kernel wrote the scene's vertices of this mesh: the view's are never trusted
};

// Base shape and lists of a mesh into `morph` on the current device (the inputs were validated by the caller: morph_check).
hipError_t mesh_morph_upload(MeshMorph& morph, const float* base_positions, const float* base_normals, uint32_t triangle_count, uint32_t target_count, const uint32_t* offsets,
                             const uint32_t* corners, const float* delta_positions, const float* delta_normals);
// k_morph_mesh over the mesh's corners with morph.weights; `skin` (may be null): the same mesh's skin, whose ids, weights and palette then pose the morphed corners.
// d_vertices = the mesh's first record in the scene's vertex array, room for 3 * morph.triangles records. d_flags[0] gets flag bits ORed in. Asynchronous.
hipError_t mesh_morph_launch(const MeshMorph& morph, const MeshSkin* skin, float4* d_vertices, uint32_t* d_flags);

}  // namespace lum

#pragma GCC visibility pop
#endif
