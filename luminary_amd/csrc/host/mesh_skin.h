// Linear blend skinning of a mesh's corners (lum_core.h lumc_mesh_skin_bind / lumc_mesh_skin_pose): the ONE definition of skin(rest, ids,
// weights, bones), compiled twice - by the host compiler into mesh_skin.cpp (skin_host: the twin, no HIP in it) and by the device compiler into mesh_skin.hip
// (k_skin_mesh) - under -ffp-contract=off, so that both give the same bytes, the packed normal word included; what the context keeps per bound mesh; and the calls
// of the scene update (scene_device.hip).
//
// All of it is binary32, one rounding per operation, in this order. Per corner: a rest position p, a rest normal n, four bone ids and four weights w_j; a bone is a
// row-major 3 x 4 matrix m. For each slot j with w_j != 0, in slot order, per row r: t_r = ((m_r0 * p.x + m_r1 * p.y) + m_r2 * p.z) + m_r3 and
// acc_r = acc_r + w_j * t_r from +0; the normal likewise with u_r = (m_r0 * n.x + m_r1 * n.y) + m_r2 * n.z. The normal goes through the 3 x 3 part AS IT IS, not
// through its inverse transpose: right for rotations and uniform scale, wrong for shear and non-uniform scale (a caller with such bones hands over normals of
// its own through the host route). Then len2 = (a.x * a.x + a.y * a.y) + a.z * a.z; a normal with len2 > 0 and finite is a * (1 / sqrt(len2)), any other keeps
// the rest normal. The device record is {x, y, z, pack_normal(normal)}, pack_normal as scene.cpp's (double arithmetic).
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define LUM_SKIN_FN __host__ __device__ __forceinline__
#define LUM_SKIN_UNROLL _Pragma("unroll")
#else
#define LUM_SKIN_FN inline
#define LUM_SKIN_UNROLL
#endif

namespace lum {

constexpr uint32_t kSkinMaxBones = 1024;  // 48 KB of palette in LDS
constexpr uint32_t kSkinFlagNotFinite = 1u, kSkinFlagBadBone = 2u;

LUM_SKIN_FN uint32_t skin_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
LUM_SKIN_FN float skin_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
LUM_SKIN_FN bool skin_finite(float f) { return (skin_bits(f) & 0x7F800000u) != 0x7F800000u; }

// scene.cpp pack_normal (device_packing.c:6-35), operation for operation. fmin / fmax return the operand that is a number, on both sides.
LUM_SKIN_FN uint32_t skin_pack_normal(const float n[3]) {
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

// One corner. `bone(j, m)` fills m with the 12 floats of the bone of slot j (called only for slots with a weight other than 0). Returns kSkinFlagNotFinite
// when a posed coordinate is not finite, else 0.
template <typename BoneOf>
LUM_SKIN_FN uint32_t skin_corner(const float p[3], const float n[3], const float w[4], BoneOf bone, float out_p[3], float out_n[3]) {
  float ap[3] = {0.0f, 0.0f, 0.0f}, an[3] = {0.0f, 0.0f, 0.0f};
  LUM_SKIN_UNROLL
  for (int j = 0; j < 4; j++) {
    if (w[j] == 0.0f) continue;  // (-0 too)
    float m[12];
    bone(j, m);
    LUM_SKIN_UNROLL
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

// The host twin (mesh_skin.cpp; no GPU): per triangle 9 rest position floats, 9 rest normal floats, 12 ids, 12 weights; 12 floats per bone. Every output may be
// null: positions and normals 9 floats per triangle, packed 3 words per triangle (the w of the device records). Returns 0, or 1 for null inputs, a bone count
// outside 1 ... kSkinMaxBones or an id >= bone_count (nothing is written then); *not_finite (optional): corners with a posed coordinate that is not finite.
int skin_host(const float* rest_positions, const float* rest_normals, const uint16_t* bone_ids, const float* weights, uint32_t triangle_count, const float* bones,
              uint32_t bone_count, float* positions, float* normals, uint32_t* packed, uint64_t* not_finite);

}  // namespace lum

#if defined(__HIP_PLATFORM_AMD__) && !defined(LUM_SKIN_HOST_ONLY)
#include <hip/hip_runtime_api.h>

#include <vector>

#include "device_buffer.h"

#pragma GCC visibility push(hidden)

namespace lum {

// A bound mesh on the context's device. The rest data is three planes of 16-byte records over the mesh's corners c (3 per triangle, in the order of the scene's
// vertex array), so that a wave reads each with one 16-byte load per lane, 1 KB contiguous: plane 0 {p.x, p.y, p.z, n.x}, plane 1 {n.y, n.z, id0 | id1 << 16,
// id2 | id3 << 16}, plane 2 {w0, w1, w2, w3} - 48 bytes read and 16 written per corner.
struct MeshSkin {
  DeviceBuffer<float4> rest;      // [3][corners]
  DeviceBuffer<float4> palette;   // 3 rows per bone: the last pose that was applied (kept for the re-skin after a vertex re-upload)
  std::vector<float> pending;     // the pose lumc_mesh_skin_pose recorded and no update has applied yet (empty: none)
  uint32_t triangles = 0, bone_count = 0;
  bool posed = false;             // a pose was applied: the scene's vertices of this mesh are the kernel's, the view's are never trusted
};

// Rest data of a mesh into `skin` on the current device (the inputs were validated by the caller).
hipError_t mesh_skin_upload(MeshSkin& skin, const float* rest_positions, const float* rest_normals, const uint16_t* bone_ids, const float* weights, uint32_t triangle_count,
                            uint32_t bone_count);
// k_skin_mesh over the mesh's corners with skin.palette: d_vertices = the mesh's first record in the scene's vertex array, room for 3 * skin.triangles records.
// d_flags[0] gets kSkinFlag* bits ORed in. Asynchronous.
hipError_t mesh_skin_launch(const MeshSkin& skin, float4* d_vertices, uint32_t* d_flags);

}  // namespace lum

#pragma GCC visibility pop
#endif
