// The light tree's refit on the device (lumc_light_refit_bind -> LUMC_DIRTY_LIGHT_POSITIONS): from the scene's vertex array to the bytes of
// the light tree that hold statistics, without the host touching a light. The arithmetic is light_refit.h's, the same source the host twin (light_refit.cpp) is
// compiled from; this unit is compiled without contraction like that one, IEEE divide and square root: both give the same bytes (lumc_light_refit_host,
// tests/test_light_refit_gpu.py).
//
//   k_light_fragments   one thread per fragment: three 16-byte vertex loads, the fragment's record (5 x 16 B) and the light's three vertices in light-id order -
//                       at once light_bvh_tris and the vertex array the light BVH is refitted from. Every index is checked against the counts the host passed; a
//                       zero area, a value that is not finite and an index out of range set a flag word with a plain atomic, which the update reads back.
//   k_light_slot_stats  one wave per child slot: lane l takes the items first + l, first + l + 64, ... (a range of <= 64 items is one pass), the partials go
//                       through the xor butterfly. Three sweeps - power, mean, variance -, 16-byte loads. The root's slots also leave (power, variance) in the
//                       result buffer the host sums the cost from.
//   k_light_nodes       workgroups of 128: the first is the root's (its 128 slots' statistics staged in LDS, lane c writes child c), every other takes 16 nodes
//                       with 8 lanes each. Only the bytes that hold statistics are written, in place.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../../include/lum_core.h"
#include "light_refit.h"

namespace lum {
namespace {

constexpr uint32_t kLrfBlock = 256, kLrfNodesBlock = 128;
static_assert(sizeof(LrfVec) == sizeof(float4) && sizeof(LumLightFragment) == 32 && sizeof(LumLightTransform) == 40 && sizeof(LumLightSlot) == 8, "record layouts");

__global__ __launch_bounds__(kLrfBlock) void k_light_fragments(const LumLightFragment* __restrict__ fragments, uint32_t count, const LumLightTransform* __restrict__ transforms,
                                                               uint32_t num_transforms, const float4* __restrict__ vertices, const uint32_t* __restrict__ mesh_tri_offset,
                                                               uint32_t num_meshes, uint32_t total_corners, float4* __restrict__ records, float4* __restrict__ tris,
                                                               uint32_t* __restrict__ flags) {
  const uint32_t i = blockIdx.x * kLrfBlock + threadIdx.x;
  if (i >= count) return;
  const LumLightFragment f = fragments[i];
  if (f.mesh >= num_meshes || f.transform >= num_transforms || f.light_id >= count) { atomicOr(flags, kLightRefitFlagBadPlan); return; }  // (the bind refuses such a plan: never taken)
  const uint64_t c0 = 3ull * ((uint64_t) mesh_tri_offset[f.mesh] + f.triangle);
  if (c0 + 3ull > (uint64_t) total_corners) { atomicOr(flags, kLightRefitFlagBadPlan); return; }
  const float4 a = vertices[c0], b = vertices[c0 + 1], c = vertices[c0 + 2];
  const float p[9] = {a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z};
  LrfVec rec[kLightRecordVecs];
  const uint32_t flag = lrf_fragment(f, transforms[f.transform], p, rec);
  for (uint32_t k = 0; k < kLightRecordVecs; k++) records[kLightRecordVecs * (size_t) i + k] = make_float4(rec[k].x, rec[k].y, rec[k].z, rec[k].w);
  for (uint32_t k = 0; k < 3; k++) tris[3 * (size_t) f.light_id + k] = make_float4(rec[k].x, rec[k].y, rec[k].z, rec[k].w);
  if (flag) atomicOr(flags, flag);
}

__device__ __forceinline__ float butterfly(float v) {
#pragma unroll
  for (int k = (int) kLightWave / 2; k >= 1; k >>= 1) v = v + __shfl_xor(v, k, (int) kLightWave);
  return v;
}

// stats: kLightStatFloats per slot; result: 2 floats per root slot
__global__ __launch_bounds__(kLrfBlock) void k_light_slot_stats(const float4* __restrict__ records, uint32_t num_fragments, const LumLightSlot* __restrict__ slots, uint32_t num_slots,
                                                                float4* __restrict__ stats, float2* __restrict__ result) {
  const uint32_t slot = blockIdx.x * (kLrfBlock / kLightWave) + threadIdx.x / kLightWave, lane = threadIdx.x % kLightWave;
  if (slot >= num_slots) return;  // (whole waves leave: the shuffles below see all 64 lanes)
  LumLightSlot s = slots[slot];
  if (s.first > num_fragments || s.count > num_fragments - s.first) s.count = 0;  // (the bind refuses such a plan: never taken)
  const LrfVec* rec = reinterpret_cast<const LrfVec*>(records);
  float power = 0.0f, variance = 0.0f;
  LrfVec mean{0.0f, 0.0f, 0.0f, 0.0f};
  if (s.count) {
    power = butterfly(lrf_lane_power(rec, s.first, s.count, lane));
    const float inv_total = 1.0f / power;
    const LrfVec m = lrf_lane_mean(rec, s.first, s.count, lane, inv_total);
    mean = LrfVec{butterfly(m.x), butterfly(m.y), butterfly(m.z), butterfly(m.w)};
    variance = butterfly(lrf_lane_variance(rec, s.first, s.count, lane, inv_total, mean));
  }
  if (lane == 0) {
    stats[2 * (size_t) slot] = make_float4(power, variance, mean.x, mean.y);
    stats[2 * (size_t) slot + 1] = make_float4(mean.z, mean.w, 0.0f, 0.0f);
    if (slot < kLightRootSlots) result[slot] = make_float2(power, variance);
  }
}

__global__ __launch_bounds__(kLrfNodesBlock) void k_light_nodes(const float* __restrict__ stats, uint32_t num_nodes, uint32_t sections, uint8_t* __restrict__ root,
                                                                float* __restrict__ root_children, uint8_t* __restrict__ nodes, float* __restrict__ scratch_result) {
  __shared__ float s_stats[kLightRootSlots * kLightStatFloats];
  if (blockIdx.x == 0) {
    for (uint32_t k = threadIdx.x; k < kLightRootSlots * kLightStatFloats; k += kLrfNodesBlock) s_stats[k] = stats[k];
    __syncthreads();
    lrf_root_lane(s_stats, threadIdx.x, sections, root, root_children, scratch_result);
    return;
  }
  const uint32_t node = (blockIdx.x - 1u) * (kLrfNodesBlock / kLightNodeSlots) + threadIdx.x / kLightNodeSlots;
  if (node >= num_nodes) return;
  lrf_node_lane(stats + kLightStatFloats * ((size_t) kLightRootSlots + (size_t) kLightNodeSlots * node), threadIdx.x % kLightNodeSlots, nodes + 64 * (size_t) node);
}

}  // namespace

hipError_t light_refit_upload(LightRefit& r, const LumLightRefitPlan& plan, uint32_t sections) {
  const size_t num_slots = kLightRootSlots + (size_t) kLightNodeSlots * plan.num_nodes;
  hipError_t e;
  if ((e = r.fragments.assign(plan.fragments, plan.num_fragments)) != hipSuccess) return e;
  if ((e = r.transforms.assign(plan.transforms, plan.num_transforms)) != hipSuccess) return e;
  if ((e = r.slots.assign(plan.slots, num_slots)) != hipSuccess) return e;
  if ((e = r.records.resize(kLightRecordVecs * (size_t) plan.num_fragments)) != hipSuccess) return e;
  if ((e = r.tris.resize(3 * (size_t) plan.num_fragments)) != hipSuccess) return e;
  if ((e = r.stats.resize(kLightStatFloats * num_slots)) != hipSuccess) return e;
  if ((e = r.result.resize(4 * kLightRootSlots)) != hipSuccess) return e;  // the slots' (power, variance), then k_light_nodes' own copy
  if ((e = r.flags.resize(1)) != hipSuccess) return e;
  if ((e = hipMemset(r.result.get(), 0, sizeof(float) * 4 * kLightRootSlots)) != hipSuccess) return e;
  r.num_fragments = plan.num_fragments; r.num_transforms = plan.num_transforms; r.num_nodes = plan.num_nodes; r.sections = sections; r.root_cost = plan.root_cost;
  return hipSuccess;
}

hipError_t light_refit_fragments(LightRefit& r, const float4* d_vertices, const uint32_t* d_mesh_tri_offset, uint32_t num_meshes, uint32_t total_corners) {
  if (!r.num_fragments || !d_vertices || !d_mesh_tri_offset || r.records.count() != kLightRecordVecs * (size_t) r.num_fragments || r.tris.count() != 3 * (size_t) r.num_fragments)
    return hipErrorInvalidValue;
  hipError_t e;
  if ((e = hipMemsetAsync(r.flags.get(), 0, sizeof(uint32_t), 0)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_light_fragments, dim3((r.num_fragments + kLrfBlock - 1) / kLrfBlock), dim3(kLrfBlock), 0, 0, (const LumLightFragment*) r.fragments.get(),
                     r.num_fragments, (const LumLightTransform*) r.transforms.get(), r.num_transforms, d_vertices, d_mesh_tri_offset, num_meshes, total_corners,
                     r.records.get(), r.tris.get(), r.flags.get());
  return hipGetLastError();
}

hipError_t light_refit_stats(LightRefit& r) {
  const uint32_t num_slots = kLightRootSlots + kLightNodeSlots * r.num_nodes, per_block = kLrfBlock / kLightWave;
  if (r.stats.count() != kLightStatFloats * (size_t) num_slots || r.slots.count() != num_slots) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_light_slot_stats, dim3((num_slots + per_block - 1) / per_block), dim3(kLrfBlock), 0, 0, (const float4*) r.records.get(), r.num_fragments,
                     (const LumLightSlot*) r.slots.get(), num_slots, (float4*) r.stats.get(), (float2*) r.result.get());
  return hipGetLastError();
}

hipError_t light_refit_nodes(LightRefit& r, uint8_t* d_root, float* d_root_children, uint8_t* d_nodes) {
  if (!d_root || !d_root_children || (r.num_nodes && !d_nodes) || r.sections == 0 || r.sections > kLightRootSlots / 8) return hipErrorInvalidValue;
  const uint32_t per_block = kLrfNodesBlock / kLightNodeSlots;
  hipLaunchKernelGGL(k_light_nodes, dim3(1 + (r.num_nodes + per_block - 1) / per_block), dim3(kLrfNodesBlock), 0, 0, (const float*) r.stats.get(), r.num_nodes, r.sections,
                     d_root, d_root_children, d_nodes, r.result.get() + 2 * kLightRootSlots);
  return hipGetLastError();
}

}  // namespace lum
