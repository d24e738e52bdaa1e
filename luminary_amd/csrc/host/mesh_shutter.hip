// Shutter on the device (lumc_mesh_shutter_key, lumc_shutter_time -> LUMC_DIRTY_MESH_SHUTTER): from a mesh's two keys and one float to the
// 16-byte records of the scene's vertex array, which k_refit_tri_boxes and the shading kernels read - without the host touching a vertex. The arithmetic is
// mesh_shutter.h's shutter_record, the same source the host twin (mesh_shutter.cpp) is compiled from; this unit is compiled without contraction like that one, IEEE
// divide and square root: both give the same bytes (lumc_shutter_host, tests/test_mesh_shutter_gpu.py).
//
//   k_shutter_vertices  one thread per corner. Two 16-byte loads - the open plane and the close plane, each contiguous over the wave: 1 KB per instruction -, one
//                       16-byte store into the mesh's range of the scene's vertex array. No LDS, no loop: the grid covers the corners, the corner is checked
//                       against the count the host passed. A coordinate that is not finite sets a flag word with one plain atomic per thread, which the
//                       update reads back.
#include <hip/hip_runtime.h>

#include "../../../include/lum_core.h"
#include "mesh_shutter.h"

namespace lum {
namespace {

constexpr uint32_t kShutterBlock = 256;

__global__ __launch_bounds__(kShutterBlock) void k_shutter_vertices(const float4* __restrict__ open, const float4* __restrict__ close, uint32_t corners, float t,
                                                                   float4* __restrict__ out, uint32_t* __restrict__ flags) {
  const uint32_t c = blockIdx.x * kShutterBlock + threadIdx.x;
  if (c >= corners) return;
  const float4 a4 = open[c], b4 = close[c];
  const ShutterRecord a = {a4.x, a4.y, a4.z, __float_as_uint(a4.w)}, b = {b4.x, b4.y, b4.z, __float_as_uint(b4.w)};
  ShutterRecord r;
  const uint32_t flag = shutter_record(a, b, t, &r);
  out[c] = make_float4(r.x, r.y, r.z, __uint_as_float(r.n));
  if (flag) atomicOr(flags, flag);
}

}  // namespace

hipError_t mesh_shutter_launch(const MeshShutter& s, float4* d_vertices, size_t room, uint32_t* d_flags) {
  const size_t corners = 3 * (size_t) s.triangles;
  if (corners == 0) return hipSuccess;
  if (!d_vertices || !d_flags || !s.both() || corners > 0xFFFFFFFFu || room < corners || s.open.count() != corners || s.close.count() != corners) return hipErrorInvalidValue;
  if (!(s.t >= 0.0f) || !(s.t <= 1.0f)) return hipErrorInvalidValue;
  const uint32_t blocks = (uint32_t) ((corners + kShutterBlock - 1) / kShutterBlock);
  hipLaunchKernelGGL(k_shutter_vertices, dim3(blocks), dim3(kShutterBlock), 0, 0, (const float4*) s.open.get(), (const float4*) s.close.get(), (uint32_t) corners, s.t,
                     d_vertices, d_flags);
  return hipGetLastError();
}

}  // namespace lum
