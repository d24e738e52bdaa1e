// Moved instances on the device (luminary_ext_set_instance_transforms -> LUMC_DIRTY_INSTANCE_TRANSFORMS): from the 32 bytes of every instance's transform to the
// top-level tree's inputs and leaf records, without the host touching an instance. Host twins, and the checkers of this unit: bvh_build.cpp
// instance_inverse_rows and instance_world_box - the same operations in the same order, float and double, compiled here without contraction like there, IEEE
// divides: both give the same bytes (lumc_instance_boxes_probe, tests/test_instance_update_gpu.py).
//
//   k_instance_rows_boxes  one thread per instance: the world->object rows, the world box of its mesh's box, whether it can be hit
//   hipcub exclusive scan  of the flags: an instance's rank among those that can be hit, in id order (deterministic; no atomics)
//   k_instance_compact     one thread per instance: box and id to their rank; the union of the boxes and their count for the host
//   (lbvh.hip build_bvh4_sah_device builds the top level over the dense boxes)
//   k_tlas_leaves          one thread per top-level leaf in leaf order: rows, instance id, root of its mesh; one more thread writes the padding record
//   k_empty_nodes          slots of the top level's range that the new tree does not use
// Every kernel boundary is the visibility boundary: no in-launch hand-off between workgroups. Every index a kernel forms is checked against a count the host
// passed. The reference has nothing like it: its instance acceleration structure comes out of optixAccelBuild (optix_bvh.c:480-684).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../../include/lum_core.h"
#include "instance_update.h"

namespace lum {
namespace {

constexpr uint32_t kInstBlock = 256;

__host__ __device__ __forceinline__ uint32_t ord_enc(float f) { uint32_t b; memcpy(&b, &f, 4); return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
__host__ __device__ __forceinline__ float ord_dec(uint32_t k) { const uint32_t b = k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu); float f; memcpy(&f, &b, 4); return f; }

// std::min / std::max / std::nextafter of the host code, operand for operand
__device__ __forceinline__ double min_of(double a, double b) { return (b < a) ? b : a; }
__device__ __forceinline__ double max_of(double a, double b) { return (a < b) ? b : a; }
__device__ __forceinline__ float next_after(float x, float to) {
  if (x != x || x == to) return x == to ? to : x;
  uint32_t b = __float_as_uint(x);
  if (x == 0.0f) return __uint_as_float((to < 0.0f ? 0x80000000u : 0u) | 1u);
  b = ((x < to) == (x > 0.0f)) ? b + 1u : b - 1u;
  return __uint_as_float(b);
}

// bvh_build.cpp instance_inverse_rows: p = the 8 floats of a transform
__device__ __forceinline__ void inverse_rows(const float p[8], float4 rows[3]) {
  const uint32_t a = __float_as_uint(p[6]), b = __float_as_uint(p[7]);
  const float ux = 1.0f - ((a & 0xFFFFu) * (1.0f / 0x7FFF)), uy = 1.0f - ((a >> 16) * (1.0f / 0x7FFF));
  const float uz = 1.0f - ((b & 0xFFFFu) * (1.0f / 0x7FFF)), s = ((b >> 16) * (1.0f / 0x7FFF)) - 1.0f;
  const float inv_scale[3] = {1.0f / p[3], 1.0f / p[4], 1.0f / p[5]};
  float col[3][3];
  for (int j = 0; j < 3; j++) {
    const float vx = (j == 0 ? 1.0f : 0.0f) * inv_scale[0], vy = (j == 1 ? 1.0f : 0.0f) * inv_scale[1], vz = (j == 2 ? 1.0f : 0.0f) * inv_scale[2];
    const float duv = ux * vx + uy * vy + uz * vz, duu = ux * ux + uy * uy + uz * uz;
    const float cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
    const float k0 = 2.0f * duv, k1 = s * s - duu, k2 = 2.0f * s;
    col[j][0] = (ux * k0 + vx * k1) + cx * k2;
    col[j][1] = (uy * k0 + vy * k1) + cy * k2;
    col[j][2] = (uz * k0 + vz * k1) + cz * k2;
  }
  for (int i = 0; i < 3; i++) rows[i] = make_float4(col[0][i], col[1][i], col[2][i], p[i]);
}

// bvh_build.cpp instance_world_box
__device__ __forceinline__ bool world_box(const float4 rows[3], const Aabb& ob, Aabb& wb) {
  const double m[3][3] = {{rows[0].x, rows[0].y, rows[0].z}, {rows[1].x, rows[1].y, rows[1].z}, {rows[2].x, rows[2].y, rows[2].z}};
  const double det = m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
                     m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
  if (!(fabs(det) > 0.0) || !isfinite(det)) return false;
  double f[3][3];
  f[0][0] = (m[1][1] * m[2][2] - m[1][2] * m[2][1]) / det; f[0][1] = (m[0][2] * m[2][1] - m[0][1] * m[2][2]) / det; f[0][2] = (m[0][1] * m[1][2] - m[0][2] * m[1][1]) / det;
  f[1][0] = (m[1][2] * m[2][0] - m[1][0] * m[2][2]) / det; f[1][1] = (m[0][0] * m[2][2] - m[0][2] * m[2][0]) / det; f[1][2] = (m[0][2] * m[1][0] - m[0][0] * m[1][2]) / det;
  f[2][0] = (m[1][0] * m[2][1] - m[1][1] * m[2][0]) / det; f[2][1] = (m[0][1] * m[2][0] - m[0][0] * m[2][1]) / det; f[2][2] = (m[0][0] * m[1][1] - m[0][1] * m[1][0]) / det;
  const double t[3] = {rows[0].w, rows[1].w, rows[2].w};
  double lo[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, hi[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
  for (int c = 0; c < 8; c++) {
    const double v[3] = {(c & 1) ? ob.hi[0] : ob.lo[0], (c & 2) ? ob.hi[1] : ob.lo[1], (c & 4) ? ob.hi[2] : ob.lo[2]};
    for (int k = 0; k < 3; k++) {
      const double w = f[k][0] * v[0] + f[k][1] * v[1] + f[k][2] * v[2] + t[k];
      lo[k] = min_of(lo[k], w); hi[k] = max_of(hi[k], w);
    }
  }
  for (int k = 0; k < 3; k++) {
    const double pad = 4e-6 * max_of(fabs(lo[k]), fabs(hi[k])) + 4e-6 * fabs(t[k]) + 1e-6 * (hi[k] - lo[k]) + 1e-30;
    wb.lo[k] = (float) (lo[k] - pad); wb.hi[k] = (float) (hi[k] + pad);
    wb.lo[k] = next_after(wb.lo[k], -FLT_MAX); wb.hi[k] = next_after(wb.hi[k], FLT_MAX);
  }
  return true;
}

// transforms: 2 float4 per instance; rows: 3 float4 per instance; boxes / flags: one per instance (a zero box where the instance cannot be hit).
__global__ __launch_bounds__(kInstBlock) void k_instance_rows_boxes(const float4* __restrict__ transforms, const uint32_t* __restrict__ mesh_ids, uint32_t num_instances,
                                                                    const uint32_t* __restrict__ mesh_tri_offset, const Aabb* __restrict__ mesh_box, uint32_t num_meshes,
                                                                    float4* __restrict__ rows, Aabb* __restrict__ boxes, uint32_t* __restrict__ flags, uint32_t host_nan) {
  const uint32_t i = blockIdx.x * kInstBlock + threadIdx.x;
  if (i >= num_instances) return;
  const float4 t0 = transforms[2 * (size_t) i], t1 = transforms[2 * (size_t) i + 1];
  const float p[8] = {t0.x, t0.y, t0.z, t0.w, t1.x, t1.y, t1.z, t1.w};
  float4 r[3];
  inverse_rows(p, r);
  // A scale of zero makes rows of infinities and NaNs (the instance cannot be hit). Which quiet NaN an invalid operation produces is the processor's choice -
  // IEEE 754 leaves sign and payload open, and the host's differs from this device's: the rows carry the host's, so that they are its bytes there too.
  for (int k = 0; k < 3; k++) {
    if (r[k].x != r[k].x) r[k].x = __uint_as_float(host_nan);
    if (r[k].y != r[k].y) r[k].y = __uint_as_float(host_nan);
    if (r[k].z != r[k].z) r[k].z = __uint_as_float(host_nan);
  }
  for (int k = 0; k < 3; k++) rows[3 * (size_t) i + k] = r[k];
  const uint32_t m = mesh_ids[i];
  Aabb wb{{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
  bool hit = false;
  if (m < num_meshes && mesh_tri_offset[m + 1] != mesh_tri_offset[m]) {
    hit = world_box(r, mesh_box[m], wb);
    if (!hit) wb = Aabb{{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
  }
  boxes[i] = wb;
  flags[i] = hit ? 1u : 0u;
}

// bounds: lo[3] (min), hi[3] (max) as ordered integers, then the number of instances that can be hit.
__global__ __launch_bounds__(kInstBlock) void k_instance_compact(const Aabb* __restrict__ boxes, const uint32_t* __restrict__ flags, const uint32_t* __restrict__ offsets,
                                                                 uint32_t num_instances, Aabb* __restrict__ dense_boxes, uint32_t* __restrict__ ids,
                                                                 uint32_t* __restrict__ bounds) {
  __shared__ uint32_t acc[6];
  if (threadIdx.x < 6) acc[threadIdx.x] = threadIdx.x < 3 ? ord_enc(FLT_MAX) : ord_enc(-FLT_MAX);
  __syncthreads();
  const uint32_t i = blockIdx.x * kInstBlock + threadIdx.x;
  if (i < num_instances) {
    const uint32_t rank = offsets[i];
    if (flags[i] && rank < num_instances) {
      const Aabb b = boxes[i];
      dense_boxes[rank] = b; ids[rank] = i;
      for (int k = 0; k < 3; k++) { atomicMin(&acc[k], ord_enc(b.lo[k])); atomicMax(&acc[3 + k], ord_enc(b.hi[k])); }
    }
    if (i == num_instances - 1u) bounds[6] = rank + (flags[i] ? 1u : 0u);
  }
  __syncthreads();
  if (threadIdx.x < 3) atomicMin(&bounds[threadIdx.x], acc[threadIdx.x]);
  else if (threadIdx.x < 6) atomicMax(&bounds[threadIdx.x], acc[threadIdx.x]);
}

// prims: rank (index into ids) of every top-level leaf; thread `leaves` writes the record of padding.
__global__ __launch_bounds__(kInstBlock) void k_tlas_leaves(const uint32_t* __restrict__ prims, const uint32_t* __restrict__ ids, uint32_t leaves, uint32_t num_instances,
                                                            const float4* __restrict__ rows, const uint32_t* __restrict__ mesh_ids, const uint32_t* __restrict__ mesh_root,
                                                            uint32_t num_meshes, float4* __restrict__ out) {
  const uint32_t i = blockIdx.x * kInstBlock + threadIdx.x;
  if (i > leaves || i > num_instances) return;  // (out holds num_instances + 1 records)
  float4 rec[4] = {make_float4(0.0f, 0.0f, 0.0f, 0.0f), make_float4(0.0f, 0.0f, 0.0f, 0.0f), make_float4(0.0f, 0.0f, 0.0f, 0.0f), make_float4(0.0f, 0.0f, 0.0f, 0.0f)};
  if (i < leaves) {
    const uint32_t rank = prims[i];
    if (rank >= leaves) return;
    const uint32_t inst = ids[rank];
    if (inst >= num_instances) return;
    const uint32_t m = mesh_ids[inst];
    if (m >= num_meshes) return;
    for (int k = 0; k < 3; k++) rec[k] = rows[3 * (size_t) inst + k];
    rec[3] = make_float4(__uint_as_float(inst), __uint_as_float(mesh_root[m]), 0.0f, 0.0f);
  }
  for (int k = 0; k < 4; k++) out[4 * (size_t) i + k] = rec[k];
}

__global__ __launch_bounds__(kInstBlock) void k_empty_nodes(Bvh4Node* __restrict__ nodes, uint32_t first, uint32_t end) {
  const uint32_t i = first + blockIdx.x * kInstBlock + threadIdx.x;
  if (i >= end) return;
  Bvh4Node node;
  for (int k = 0; k < 4; k++) {
    node.child[k] = kBvhEmpty; node.pad[k] = 0;
    node.lo_x[k] = node.lo_y[k] = node.lo_z[k] = FLT_MAX;
    node.hi_x[k] = node.hi_y[k] = node.hi_z[k] = -FLT_MAX;
  }
  nodes[i] = node;
}

inline uint32_t blocks_for(uint32_t n) { return (n + kInstBlock - 1) / kInstBlock; }

// The quiet NaN this host's arithmetic produces for an invalid operation (every NaN of instance_inverse_rows over finite transforms descends from one).
uint32_t host_generated_nan() {
  volatile float inf = INFINITY;
  const float nan = inf - inf;
  uint32_t bits;
  std::memcpy(&bits, &nan, 4);
  return bits;
}

hipError_t launch_rows_boxes(const float4* d_transforms, const uint32_t* d_mesh_ids, uint32_t num_instances, const uint32_t* d_mesh_tri_offset, const Aabb* d_mesh_box,
                             uint32_t num_meshes, float4* d_rows, Aabb* d_boxes, uint32_t* d_flags) {
  if (num_instances == 0) return hipSuccess;
  hipLaunchKernelGGL(k_instance_rows_boxes, dim3(blocks_for(num_instances)), dim3(kInstBlock), 0, 0, d_transforms, d_mesh_ids, num_instances, d_mesh_tri_offset, d_mesh_box,
                     num_meshes, d_rows, d_boxes, d_flags, host_generated_nan());
  return hipGetLastError();
}

}  // namespace

hipError_t instance_update_prepare(InstanceUpdate& u, uint32_t num_instances, uint32_t num_meshes, const Aabb* mesh_box) {
  hipError_t e;
  u.prepared = false;
  u.num_instances = num_instances; u.num_meshes = num_meshes;
  const size_t n = num_instances ? num_instances : 1;
  if ((e = u.mesh_box.assign(mesh_box, num_meshes)) != hipSuccess) return e;
  if ((e = u.boxes.resize(n)) != hipSuccess || (e = u.dense_boxes.resize(n)) != hipSuccess || (e = u.flags.resize(n)) != hipSuccess || (e = u.offsets.resize(n)) != hipSuccess ||
      (e = u.ids.resize(n)) != hipSuccess || (e = u.prims.resize(n)) != hipSuccess || (e = u.bounds.resize(8)) != hipSuccess)
    return e;
  u.scan_bytes = 0;
  if ((e = hipcub::DeviceScan::ExclusiveSum(nullptr, u.scan_bytes, u.flags.get(), u.offsets.get(), (int) n)) != hipSuccess) return e;
  if ((e = u.scan_temp.resize(u.scan_bytes ? u.scan_bytes : 16)) != hipSuccess) return e;
  u.prepared = true;
  return hipSuccess;
}

hipError_t instance_update_boxes(InstanceUpdate& u, const float4* d_transforms, const uint32_t* d_mesh_ids, const uint32_t* d_mesh_tri_offset, float4* d_rows,
                                 uint32_t* hittable, Aabb* world) {
  const uint32_t n = u.num_instances;
  *hittable = 0;
  *world = Aabb{{0.0f, 0.0f, 0.0f}, {1.0f, 1.0f, 1.0f}};
  if (n == 0) return hipSuccess;
  hipError_t e;
  if ((e = launch_rows_boxes(d_transforms, d_mesh_ids, n, d_mesh_tri_offset, u.mesh_box.get(), u.num_meshes, d_rows, u.boxes.get(), u.flags.get())) != hipSuccess) return e;
  size_t bytes = u.scan_bytes;
  if ((e = hipcub::DeviceScan::ExclusiveSum(u.scan_temp.get(), bytes, u.flags.get(), u.offsets.get(), (int) n)) != hipSuccess) return e;
  uint32_t init[7];
  for (int k = 0; k < 3; k++) { init[k] = ord_enc(FLT_MAX); init[3 + k] = ord_enc(-FLT_MAX); }
  init[6] = 0;
  if ((e = hipMemcpy(u.bounds.get(), init, sizeof(init), hipMemcpyHostToDevice)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_instance_compact, dim3(blocks_for(n)), dim3(kInstBlock), 0, 0, (const Aabb*) u.boxes.get(), (const uint32_t*) u.flags.get(),
                     (const uint32_t*) u.offsets.get(), n, u.dense_boxes.get(), u.ids.get(), u.bounds.get());
  if ((e = hipGetLastError()) != hipSuccess) return e;
  uint32_t out[7];
  if ((e = hipMemcpy(out, u.bounds.get(), sizeof(out), hipMemcpyDeviceToHost)) != hipSuccess) return e;  // (waits for the launches)
  if (out[6] > n) return hipErrorUnknown;
  *hittable = out[6];
  if (out[6]) for (int k = 0; k < 3; k++) { world->lo[k] = ord_dec(out[k]); world->hi[k] = ord_dec(out[3 + k]); }
  return hipSuccess;
}

hipError_t instance_update_leaves(InstanceUpdate& u, uint32_t leaves, const float4* d_rows, const uint32_t* d_mesh_ids, float4* d_leaves, Bvh4Node* d_nodes,
                                  uint32_t clear_first, uint32_t clear_end) {
  if (leaves > u.num_instances || clear_end > u.capacity) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_tlas_leaves, dim3(blocks_for(leaves + 1u)), dim3(kInstBlock), 0, 0, (const uint32_t*) u.prims.get(), (const uint32_t*) u.ids.get(), leaves, u.num_instances,
                     d_rows, d_mesh_ids, (const uint32_t*) u.mesh_root.get(), u.num_meshes, d_leaves);
  if (clear_first < clear_end)
    hipLaunchKernelGGL(k_empty_nodes, dim3(blocks_for(clear_end - clear_first)), dim3(kInstBlock), 0, 0, d_nodes, clear_first, clear_end);
  return hipGetLastError();
}

}  // namespace lum

// lum_core.h lumc_instance_boxes_probe
extern "C" int lumc_instance_boxes_probe(const LumDeviceSceneView* v, const float* mesh_boxes, int on_gpu, void* rows, float* boxes, uint32_t* hittable) {
  using namespace lum;
  if (!v || !rows || !boxes || !hittable || (v->num_meshes && !mesh_boxes)) return 1;
  const uint32_t n = v->num_instances, nm = v->num_meshes;
  if (n == 0) return 0;
  static_assert(sizeof(Aabb) == 24, "six floats per box");
  const Aabb* mb = reinterpret_cast<const Aabb*>(mesh_boxes);
  float4* out_rows = static_cast<float4*>(rows);
  Aabb* out_boxes = reinterpret_cast<Aabb*>(boxes);
  if (!on_gpu) {
    for (uint32_t i = 0; i < n; i++) {
      instance_inverse_rows(v->instance_transforms + (size_t) i * 8, out_rows + 3 * (size_t) i);
      const uint32_t m = v->instance_mesh_ids[i];
      Aabb wb{{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
      bool hit = m < nm && v->mesh_tri_offset[m + 1] != v->mesh_tri_offset[m] && instance_world_box(out_rows + 3 * (size_t) i, mb[m], wb);
      if (!hit) wb = Aabb{{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
      out_boxes[i] = wb; hittable[i] = hit ? 1u : 0u;
    }
    return 0;
  }
  DeviceBuffer<float4> d_transforms, d_rows;
  DeviceBuffer<uint32_t> d_mesh_ids, d_offsets, d_flags;
  DeviceBuffer<Aabb> d_mesh_box, d_boxes;
  const uint32_t no_mesh[2] = {0u, 0u};
  const Aabb no_box{{0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
  if (d_transforms.assign(reinterpret_cast<const float4*>(v->instance_transforms), 2 * (size_t) n) != hipSuccess || d_mesh_ids.assign(v->instance_mesh_ids, n) != hipSuccess ||
      d_offsets.assign(nm ? v->mesh_tri_offset : no_mesh, (size_t) nm + 1) != hipSuccess || d_mesh_box.assign(nm ? mb : &no_box, nm ? nm : 1) != hipSuccess ||
      d_rows.resize(3 * (size_t) n) != hipSuccess || d_boxes.resize(n) != hipSuccess || d_flags.resize(n) != hipSuccess)
    return 1;
  if (launch_rows_boxes(d_transforms.get(), d_mesh_ids.get(), n, d_offsets.get(), d_mesh_box.get(), nm, d_rows.get(), d_boxes.get(), d_flags.get()) != hipSuccess) return 1;
  if (hipMemcpy(out_rows, d_rows.get(), sizeof(float4) * 3 * (size_t) n, hipMemcpyDeviceToHost) != hipSuccess) return 1;
  if (hipMemcpy(out_boxes, d_boxes.get(), sizeof(Aabb) * n, hipMemcpyDeviceToHost) != hipSuccess) return 1;
  return hipMemcpy(hittable, d_flags.get(), sizeof(uint32_t) * n, hipMemcpyDeviceToHost) != hipSuccess;
}
