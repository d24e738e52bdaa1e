// Deformed meshes: linear blend skinning (lum_core.h lumc_mesh_skin_bind / lumc_mesh_skin_pose) and morph targets / blend shapes
// (lumc_mesh_morph_bind / lumc_mesh_morph_weights; section 12) of a mesh's corners. The ONE definition of deform(rest, morph part, skin part) - deform_corner over
// morph_corner, morph_normal and skin_corner -, compiled twice: by the host compiler into mesh_deform.cpp (deform_host: the twin, no HIP in it) and by the device
// compiler into mesh_deform.hip (k_deform_mesh), under -ffp-contract=off, so that both give the same bytes, the packed normal word included; what the context keeps
// per bound mesh; and the calls of the scene update (scene_device.hip).
//
// All of it is binary32, one rounding per operation, in this order.
// Morph. Per corner: a base position p and a base normal n, and the corner's entries (target t, dp, dn) IN ASCENDING TARGET ORDER. An entry whose weight w_t is 0
// (-0 too) is skipped; every other one adds, per row r, p_r = p_r + w_t * dp_r and n_r = n_r + w_t * dn_r (a multiply, then an add).
// Skin. Per corner: a rest position p, a rest normal n, four bone ids and four weights w_j; a bone is a row-major 3 x 4 matrix m. For each slot j with w_j != 0, in
// slot order, per row r: t_r = ((m_r0 * p.x + m_r1 * p.y) + m_r2 * p.z) + m_r3 and acc_r = acc_r + w_j * t_r from +0; the normal likewise with
// u_r = (m_r0 * n.x + m_r1 * n.y) + m_r2 * n.z. The normal goes through the 3 x 3 part AS IT IS, not through its inverse transpose: right for rotations and uniform
// scale, wrong for shear and non-uniform scale (a caller with such bones hands over normals of its own through the host route). Then
// len2 = (a.x * a.x + a.y * a.y) + a.z * a.z; a normal with len2 > 0 and finite is a * (1 / sqrt(len2)), any other keeps the rest normal.
// Together (deform_corner):
//   a morph, no contributing entry  the record is the base record: position and normal untouched, nothing normalised
//   a morph, contributing entries   len2 = (n.x * n.x + n.y * n.y) + n.z * n.z; a normal with len2 > 0 and finite is n * (1 / sqrtf(len2)), any other keeps the base normal
//   a skin                          skin_corner over its rest pose
//   both                            skin_corner over the UN-normalised morphed p, n (the skin's own rest pose is not read)
// The device record is {x, y, z, skin_pack_normal(normal)}, skin_pack_normal as scene.cpp's pack_normal (double arithmetic); a coordinate that is not finite sets
// kSkinFlagNotFinite.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#if defined(__HIPCC__)
#define LUM_DEFORM_FN __host__ __device__ __forceinline__
#define LUM_DEFORM_UNROLL _Pragma("unroll")
#else
#define LUM_DEFORM_FN inline
#define LUM_DEFORM_UNROLL
#endif

namespace lum {

constexpr uint32_t kSkinMaxBones = 1024;  // 48 KB of palette in LDS
constexpr uint32_t kMorphMaxTargets = 1024;  // 4 KB of weights in LDS
constexpr uint32_t kSkinFlagNotFinite = 1u, kSkinFlagBadBone = 2u;
constexpr uint32_t kMorphFlagBadLayout = 4u;  // a target id beyond the target count or a row outside the entries

LUM_DEFORM_FN uint32_t skin_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
LUM_DEFORM_FN float skin_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
LUM_DEFORM_FN bool skin_finite(float f) { return (skin_bits(f) & 0x7F800000u) != 0x7F800000u; }

// scene.cpp pack_normal (device_packing.c:6-35), operation for operation. fmin / fmax return the operand that is a number, on both sides.
LUM_DEFORM_FN uint32_t skin_pack_normal(const float n[3]) {
  double x = n[0], y = n[1], z = n[2];
  const double rn = 1.0 / (::fabs(x) + ::fabs(y) + ::fabs(z));
  x *= rn; y *= rn; z *= rn;
  const double t = ::fmax(::fmin(-z, 1.0), 0.0);
  x += (x >= 0.0) ? t : -t;
  y += (y >= 0.0) ? t : -t;
  x = ::fmax(::fmin(x, 1.0), -1.0);
  y = ::fmax(::fmin(y, 1.0), -1.0);
  x = (x + 1.0) * 0.5; y = (y + 1.0) * 0.5;
  const uint32_t xu = (uint32_t) (x * 0xFFFF + 0.5), yu = (uint32_t) (y * 0xFFFF + 0.5);
  return (yu << 16) | xu;
}

// One corner under its bones. `bone(j, m)` fills m with the 12 floats of the bone of slot j (called only for slots with a weight other than 0). Returns
// kSkinFlagNotFinite when a posed coordinate is not finite, else 0.
template <typename BoneOf>
LUM_DEFORM_FN uint32_t skin_corner(const float p[3], const float n[3], const float w[4], BoneOf bone, float out_p[3], float out_n[3]) {
  float ap[3] = {0.0f, 0.0f, 0.0f}, an[3] = {0.0f, 0.0f, 0.0f};
  LUM_DEFORM_UNROLL
  for (int j = 0; j < 4; j++) {
    if (w[j] == 0.0f) continue;  // (-0 too)
    float m[12];
    bone(j, m);
    LUM_DEFORM_UNROLL
    for (int r = 0; r < 3; r++) {
      const float t = ((m[4 * r] * p[0] + m[4 * r + 1] * p[1]) + m[4 * r + 2] * p[2]) + m[4 * r + 3];
      const float u = (m[4 * r] * n[0] + m[4 * r + 1] * n[1]) + m[4 * r + 2] * n[2];
      ap[r] = ap[r] + w[j] * t;
      an[r] = an[r] + w[j] * u;
    }
  }
  const float len2 = (an[0] * an[0] + an[1] * an[1]) + an[2] * an[2];
  if (len2 > 0.0f && skin_finite(len2)) {
    const float rl = 1.0f / ::sqrtf(len2);
    out_n[0] = an[0] * rl; out_n[1] = an[1] * rl; out_n[2] = an[2] * rl;
  }
  else { out_n[0] = n[0]; out_n[1] = n[1]; out_n[2] = n[2]; }
  out_p[0] = ap[0]; out_p[1] = ap[1]; out_p[2] = ap[2];
  return (skin_finite(ap[0]) && skin_finite(ap[1]) && skin_finite(ap[2])) ? 0u : kSkinFlagNotFinite;
}

// The entries [first, last) of one corner onto p and n, in place. `entry(k, dp, dn)` fills the deltas of entry k and returns its target, `weight(t)` gives w_t.
// Returns the number of entries that contributed.
template <typename EntryOf, typename WeightOf>
LUM_DEFORM_FN uint32_t morph_corner(float p[3], float n[3], uint32_t first, uint32_t last, EntryOf entry, WeightOf weight) {
  uint32_t used = 0;
  for (uint32_t k = first; k < last; k++) {
    float dp[3], dn[3];
    const uint32_t t = entry(k, dp, dn);
    const float w = weight(t);
    if (w == 0.0f) continue;  // (-0 too)
    LUM_DEFORM_UNROLL
    for (int r = 0; r < 3; r++) {
      p[r] = p[r] + w * dp[r];
      n[r] = n[r] + w * dn[r];
    }
    used++;
  }
  return used;
}

// The normal of a morphed corner without a skin: `n` the morphed sum, `used` what morph_corner returned.
LUM_DEFORM_FN void morph_normal(const float base_n[3], const float n[3], uint32_t used, float out_n[3]) {
  out_n[0] = base_n[0]; out_n[1] = base_n[1]; out_n[2] = base_n[2];
  if (used == 0) return;
  const float len2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
  if (len2 > 0.0f && skin_finite(len2)) {
    const float rl = 1.0f / ::sqrtf(len2);
    out_n[0] = n[0] * rl; out_n[1] = n[1] * rl; out_n[2] = n[2] * rl;
  }
}

// One corner under the parts its mesh is bound to - the one place that decides what a morph, a skin and both make of a corner. rest_p / rest_n: the morph's base
// shape with `morph`, else the skin's rest pose. The morph part: the corner's entries [first, last) with morph_corner's accessors. The skin part: `slots(id, w)`
// fills the corner's four bone ids and weights (called once, after the morph), `bone(id, m)` fills m with the 12 floats of a bone (called only for slots with a
// weight other than 0). Neither part's accessors are called when it is absent. Returns kSkinFlagNotFinite when an output coordinate is not finite, else 0.
template <typename EntryOf, typename WeightOf, typename SlotsOf, typename BoneOf>
LUM_DEFORM_FN uint32_t deform_corner(const float rest_p[3], const float rest_n[3], bool morph, uint32_t first, uint32_t last, EntryOf entry, WeightOf weight, bool skin,
                                     SlotsOf slots, BoneOf bone, float out_p[3], float out_n[3]) {
  float p[3] = {rest_p[0], rest_p[1], rest_p[2]}, n[3] = {rest_n[0], rest_n[1], rest_n[2]};
  const uint32_t used = morph ? morph_corner(p, n, first, last, entry, weight) : 0u;
  if (skin) {
    uint32_t id[4];
    float w[4];
    slots(id, w);
    return skin_corner(p, n, w, [&](int j, float m[12]) { bone(id[j], m); }, out_p, out_n);
  }
  morph_normal(rest_n, n, used, out_n);
  out_p[0] = p[0]; out_p[1] = p[1]; out_p[2] = p[2];
  return (skin_finite(p[0]) && skin_finite(p[1]) && skin_finite(p[2])) ? 0u : kSkinFlagNotFinite;
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

// The host twin (mesh_deform.cpp; no GPU): deform_corner over corner_count corners. rest_positions / rest_normals: 3 floats per corner. csr (may be null: no morph)
// with morph_weights, its corners [first_corner, first_corner + corner_count): every other array starts at first_corner. bones (may be null: no skin), 12 floats
// each, with bone_ids / skin_weights, 4 per corner. Every output may be null, and may be a rest array: positions and normals 3 floats per corner, packed one word
// per corner (the w of the device records); *not_finite (optional): corners with a coordinate that is not finite. Checks nothing; with neither part nothing is written.
void deform_host(const float* rest_positions, const float* rest_normals, const MorphCsr* csr, size_t first_corner, size_t corner_count, const float* morph_weights,
                 const uint16_t* bone_ids, const float* skin_weights, const float* bones, float* positions, float* normals, uint32_t* packed, uint64_t* not_finite);
// The entry points that check their arguments. Per triangle 9 rest position floats, 9 rest normal floats, 12 ids, 12 weights. Each returns 0, or 1 and writes nothing.
// skin_host refuses null inputs, a bone count outside 1 ... kSkinMaxBones and an id >= bone_count.
int skin_host(const float* rest_positions, const float* rest_normals, const uint16_t* bone_ids, const float* weights, uint32_t triangle_count, const float* bones,
              uint32_t bone_count, float* positions, float* normals, uint32_t* packed, uint64_t* not_finite);
// morph_host: the lists as above, weights: T finite floats; with bones also bone_ids / skin_weights: the combined result. Refuses null inputs, lists morph_check
// refuses, a weight that is not finite and skin arguments skin_host refuses.
int morph_host(const float* base_positions, const float* base_normals, uint32_t triangle_count, uint32_t target_count, const uint32_t* offsets, const uint32_t* corners,
               const float* delta_positions, const float* delta_normals, const float* weights, const uint16_t* bone_ids, const float* skin_weights, const float* bones,
               uint32_t bone_count, float* positions, float* normals, uint32_t* packed, uint64_t* not_finite);
// The same over a CSR that is there already (what the host layer keeps per bound mesh); nothing is checked.
void morph_host_csr(const float* base_positions, const float* base_normals, const MorphCsr& csr, size_t first_corner, size_t corner_count, const float* weights,
                    const uint16_t* bone_ids, const float* skin_weights, const float* bones, float* positions, float* normals, uint32_t* packed, uint64_t* not_finite);

}  // namespace lum

#if defined(__HIP_PLATFORM_AMD__) && !defined(LUM_DEFORM_HOST_ONLY)
#include <hip/hip_runtime_api.h>

#include <optional>

#include "device_buffer.h"

#pragma GCC visibility push(hidden)

namespace lum {

// A mesh's skin on the context's device. The rest data is three planes of 16-byte records over the mesh's corners c (3 per triangle, in the order of the scene's
// vertex array), so that a wave reads each with one 16-byte load per lane, 1 KB contiguous: plane 0 {p.x, p.y, p.z, n.x}, plane 1 {n.y, n.z, id0 | id1 << 16,
// id2 | id3 << 16}, plane 2 {w0, w1, w2, w3} - 48 bytes read and 16 written per corner.
struct MeshSkin {
  DeviceBuffer<float4> rest;      // [3][corners]
  DeviceBuffer<float4> palette;   // 3 rows per bone: the last pose that was applied (kept for the re-skin after a vertex re-upload)
  std::vector<float> pending;     // the pose lumc_mesh_skin_pose recorded and no update has applied yet (empty: none)
  uint32_t triangles = 0, bone_count = 0;
  bool posed = false;             // a pose was applied: the scene's vertices of this mesh are the kernel's, the view's are never trusted
};

// A mesh's morph on the context's device: the base shape as two planes of 16-byte records over the mesh's corners c - plane 0 {p.x, p.y, p.z, n.x}, plane 1 {n.y, n.z,
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

// What the context keeps per bound mesh: a skin, a morph or both (never neither: the record goes with its last part). The two have rest shapes of their own.
struct MeshDeform {
  std::optional<MeshSkin> skin;
  std::optional<MeshMorph> morph;
  bool empty() const { return !skin && !morph; }
  bool new_pose() const { return skin && !skin->pending.empty(); }
  bool new_weights() const { return morph && !morph->pending.empty(); }
  bool pending() const { return new_pose() || new_weights(); }
  bool skin_writes() const { return skin && (skin->posed || new_pose()); }  // the skin takes part in the next launch (no palette yet: the morph alone writes the mesh)
  bool written_on_device() const { return (skin && skin->posed) || (morph && morph->applied); }  // a kernel wrote this mesh's vertices: the view's are never trusted
};

// Rest data of a mesh into `skin` on the current device (the inputs were validated by the caller).
hipError_t mesh_skin_upload(MeshSkin& skin, const float* rest_positions, const float* rest_normals, const uint16_t* bone_ids, const float* weights, uint32_t triangle_count,
                            uint32_t bone_count);
// Base shape and lists of a mesh into `morph` on the current device (the inputs were validated by the caller: morph_check).
hipError_t mesh_morph_upload(MeshMorph& morph, const float* base_positions, const float* base_normals, uint32_t triangle_count, uint32_t target_count, const uint32_t* offsets,
                             const uint32_t* corners, const float* delta_positions, const float* delta_normals);
// k_deform_mesh over the mesh's corners with the morph's weights, if there is one, and the skin's palette, if d.skin_writes(); one of the two at least. With both,
// the skin's ids, weights and palette pose the morphed corners. d_vertices = the mesh's first record in the scene's vertex array, room for 3 * triangles records.
// d_flags[0] gets flag bits ORed in. Asynchronous.
hipError_t mesh_deform_launch(const MeshDeform& d, float4* d_vertices, uint32_t* d_flags);

}  // namespace lum

#pragma GCC visibility pop
#endif
