// Shutter: a mesh's vertices at a time between two keys (lum_core.h lumc_mesh_shutter_key / lumc_shutter_time -> LUMC_DIRTY_MESH_SHUTTER).
// A key is a copy of the mesh's range of the scene's vertex array - whatever wrote it: an upload, moved vertices, a pose, morph weights -, so one model, linear
// between an open and a close key, covers every route that moves vertices. The ONE definition of the blended record - shutter_record -, compiled twice: by the
// host compiler into mesh_shutter.cpp (lumc_shutter_host: the twin, no HIP in it) and by the device compiler into mesh_shutter.hip (k_shutter_vertices), under
// -ffp-contract=off with IEEE divide and square root, so that both give the same bytes, the packed normal word included; what the context keeps per mesh that
// holds keys; and the calls of the scene update (scene_device.hip).
//
// A record is the scene's 16-byte vertex record {x, y, z, packed normal}. shutter_record(a, b, t), a the open record, b the close record, t in [0, 1]:
//   t == 0     a, bit for bit (-0 and the normal word included); t == 1: b, bit for bit.
//   otherwise  each coordinate is a + t * (b - a) in binary32: a subtract, a multiply, an add, one rounding each. A result that is not finite sets
//              kShutterFlagNotFinite (the record is written as computed).
//   the normal equal words: that word. Otherwise both words are unpacked by the expressions of dev_math.h's normal_unpack, restated here operation by operation in
//              binary32: u = (w & 0xFFFF) * (1 / 65535), v = (w >> 16) * (1 / 65535); x = u * 2 - 1, y = v * 2 - 1, z = (1 - |x|) - |y|; s = min(max(-z, 0), 1);
//              x = x + (x >= 0 ? -s : s), y likewise; len2 = (x x + y y) + z z, n = n * (1 / sqrtf(len2)). The two unpacked normals are blended like the
//              coordinates; a blend with len2 > 0 and finite is normalised the same way and packed with skin_pack_normal (mesh_deform.h); any other blend -
//              opposite normals at t = 0.5, say - takes a's word for t < 0.5 and b's word otherwise.
// The caller guarantees t in [0, 1] (lumc_shutter_host and lumc_shutter_time refuse any other).
#pragma once

#include <math.h>
#include <stdint.h>

#include "mesh_deform.h"

namespace lum {

constexpr uint32_t kShutterFlagNotFinite = 1u;

struct ShutterRecord { float x, y, z; uint32_t n; };

LUM_DEFORM_FN float shutter_lerp(float a, float b, float t) {
  const float d = b - a;
  const float s = t * d;
  return a + s;
}

// dev_math.h normal_unpack, operation for operation.
LUM_DEFORM_FN void shutter_unpack_normal(uint32_t w, float n[3]) {
  float x = (float) (w & 0xFFFFu) * (1.0f / 0xFFFF), y = (float) (w >> 16) * (1.0f / 0xFFFF);
  x = (x * 2.0f) - 1.0f; y = (y * 2.0f) - 1.0f;
  float z = (1.0f - ::fabsf(x)) - ::fabsf(y);
  float s = -z;
  s = s < 0.0f ? 0.0f : (s > 1.0f ? 1.0f : s);
  x = x + ((x >= 0.0f) ? -s : s);
  y = y + ((y >= 0.0f) ? -s : s);
  const float len2 = (x * x + y * y) + z * z;
  const float rl = 1.0f / ::sqrtf(len2);
  n[0] = x * rl; n[1] = y * rl; n[2] = z * rl;
}

// The record at time t between the keys a and b. Returns kShutterFlagNotFinite when a coordinate of the result is not finite, else 0.
LUM_DEFORM_FN uint32_t shutter_record(const ShutterRecord& a, const ShutterRecord& b, float t, ShutterRecord* out) {
  if (t == 0.0f) { *out = a; return 0u; }
  if (t == 1.0f) { *out = b; return 0u; }
  ShutterRecord r;
  r.x = shutter_lerp(a.x, b.x, t); r.y = shutter_lerp(a.y, b.y, t); r.z = shutter_lerp(a.z, b.z, t);
  if (a.n == b.n) r.n = a.n;
  else {
    float na[3], nb[3], n[3];
    shutter_unpack_normal(a.n, na);
    shutter_unpack_normal(b.n, nb);
    n[0] = shutter_lerp(na[0], nb[0], t); n[1] = shutter_lerp(na[1], nb[1], t); n[2] = shutter_lerp(na[2], nb[2], t);
    const float len2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    if (len2 > 0.0f && skin_finite(len2)) {
      const float rl = 1.0f / ::sqrtf(len2);
      n[0] = n[0] * rl; n[1] = n[1] * rl; n[2] = n[2] * rl;
      r.n = skin_pack_normal(n);
    }
    else r.n = (t < 0.5f) ? a.n : b.n;
  }
  *out = r;
  return (skin_finite(r.x) && skin_finite(r.y) && skin_finite(r.z)) ? 0u : kShutterFlagNotFinite;
}

}  // namespace lum

#if defined(__HIP_PLATFORM_AMD__) && !defined(LUM_DEFORM_HOST_ONLY)

#pragma GCC visibility push(hidden)

namespace lum {

// A mesh's keys on the context's device: two planes of 3 * triangles vertex records, each a device-to-device copy of the mesh's range of the scene's vertex array
// at the moment lumc_mesh_shutter_key was called. 32 bytes are read and 16 written per corner.
struct MeshShutter {
  DeviceBuffer<float4> open, close;
  uint32_t triangles = 0;
  bool has_open = false, has_close = false;
  float t = 1.0f;        // the time the scene's vertices of this mesh were last written at (the close key is taken from them: 1)
  bool pending = false;  // lumc_shutter_time recorded a time that no update has applied yet
  bool both() const { return has_open && has_close; }  // the scene's vertices of this mesh are the kernel's: the view's are never trusted
};

// k_shutter_vertices over the mesh's corners at s.t. d_vertices = the mesh's first record in the scene's vertex array, room for `room` records (checked against
// 3 * s.triangles, as the planes' sizes are). d_flags[0] gets kShutterFlag* bits ORed in. Asynchronous.
hipError_t mesh_shutter_launch(const MeshShutter& s, float4* d_vertices, size_t room, uint32_t* d_flags);

}  // namespace lum

#pragma GCC visibility pop
#endif
