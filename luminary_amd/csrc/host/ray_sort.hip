// Ray ordering: the sort keys, the sorted permutation and the physical reorder of a path queue (lumc_set_ray_sorting).
#include <algorithm>

#include <hipcub/hipcub.hpp>

#include "context.h"

namespace {

// ---- ray ordering (north star: "ray-sorted wavefront"; the reference sorts its tasks by hit type every depth, cuda/kernels.cuh:391-484) ----
// Key = Morton code of the ray origin's cell in a 64^3 grid over the scene bounds (18 bits) combined with the direction's octant (3 bits).
// Flavour-neutral: the order in which a queue is traced never changes a result (every path owns its slots), it only decides which rays
// share a wave, a CU's L1 and an XCD's L2.
struct SortGrid { float lo[3], scale[3]; uint32_t direction_major; };

__device__ __forceinline__ uint32_t spread6(uint32_t v) {  // 6 bits -> every third bit
  v &= 0x3Fu;
  v = (v | (v << 8)) & 0x300Fu;
  v = (v | (v << 4)) & 0x30C3u;
  v = (v | (v << 2)) & 0x9249u;
  return v;
}

__global__ __launch_bounds__(256) void k_ray_sort_keys(const float4* __restrict__ origin, const float4* __restrict__ dir, const uint32_t* __restrict__ count, uint32_t capacity,
                                                       SortGrid g, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const uint32_t n = min(*count, capacity);
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < capacity; i += gridDim.x * 256u) {
    uint32_t key = 0x200000u;  // beyond the live items: above every live key (21 bits), so they sort to the end whether or not the sort is stable
    if (i < n) {
      const float4 o = origin[i], d = dir[i];
      const uint32_t cx = (uint32_t) fminf(fmaxf((o.x - g.lo[0]) * g.scale[0], 0.0f), 63.0f), cy = (uint32_t) fminf(fmaxf((o.y - g.lo[1]) * g.scale[1], 0.0f), 63.0f),
                     cz = (uint32_t) fminf(fmaxf((o.z - g.lo[2]) * g.scale[2], 0.0f), 63.0f);
      const uint32_t morton = spread6(cx) | (spread6(cy) << 1) | (spread6(cz) << 2);
      const uint32_t octant = (d.x < 0.0f ? 1u : 0u) | (d.y < 0.0f ? 2u : 0u) | (d.z < 0.0f ? 4u : 0u);
      key = g.direction_major ? ((octant << 18) | morton) : ((morton << 3) | octant);
    }
    keys[i] = key;
    vals[i] = i;
  }
}

int ensure_sort(LumContext* ctx, uint32_t items) {
  LumContext::RaySort& s = ctx->sort;
  if (s.d_temp && items <= s.d_keys[0].count()) return 0;
  for (int k = 0; k < 2; k++) { s.d_keys[k].reset(); s.d_vals[k].reset(); }
  s.d_temp.reset();
  for (int k = 0; k < 2; k++) {
    HIP_TRY(ctx, s.d_keys[k].resize(items));
    HIP_TRY(ctx, s.d_vals[k].resize(items));
  }
  hipcub::DoubleBuffer<uint32_t> keys(s.d_keys[0].get(), s.d_keys[1].get()), vals(s.d_vals[0].get(), s.d_vals[1].get());
  HIP_TRY(ctx, hipcub::DeviceRadixSort::SortPairs(nullptr, s.temp_bytes, keys, vals, (int) items, 0, 22, (hipStream_t) 0));
  HIP_TRY(ctx, s.d_temp.resize(std::max<size_t>(s.temp_bytes, 16)));
  return 0;
}

// Mode 3: the path state of the live paths gathered through the sorted permutation into a second set of planes, written in order - the pass every
// later kernel of the depth then reads coherently (trace, shade, and through the order of the appends the visibility rays and the next depth).
__global__ __launch_bounds__(256) void k_permute_queue(PathQueue src, PathQueue dst, const uint32_t* __restrict__ order, const uint32_t* __restrict__ count, uint32_t capacity) {
  const uint32_t n = min(*count, capacity);
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
    const uint32_t j = order[i];
    const float4 o = src.origin_t[j], d = src.dir_slot[j];
    const uint4 a = src.aux[j], h = src.hit_id[j];
    dst.origin_t[i] = o; dst.dir_slot[i] = d; dst.aux[i] = a; dst.hit_id[i] = h;
  }
}

int ensure_sort_queue(LumContext* ctx, uint32_t items) {
  LumContext::RaySort& s = ctx->sort;
  if (items == s.planes[3].count()) return 0;  // (the last of the four: a set that was not completed is allocated again)
  for (auto& plane : s.planes) plane.reset();
  s.queue = PathQueue{};
  for (auto& plane : s.planes) HIP_TRY(ctx, plane.resize(items));
  s.queue.origin_t = s.planes[0].get(); s.queue.dir_slot = s.planes[1].get();
  s.queue.aux = (uint4*) s.planes[2].get(); s.queue.hit_id = (uint4*) s.planes[3].get();
  return 0;
}

}  // namespace

// Sorted order of the first *count items of (origin, dir); returns the permutation (device pointer) or nullptr on failure.
const uint32_t* sort_rays(LumContext* ctx, hipStream_t stream, const float4* origin, const float4* dir, const uint32_t* count, uint32_t capacity) {
  if (ensure_sort(ctx, capacity)) return nullptr;
  SortGrid g;
  for (int k = 0; k < 3; k++) { g.lo[k] = ctx->sort.world_lo[k]; const float e = ctx->sort.world_hi[k] - ctx->sort.world_lo[k]; g.scale[k] = e > 0.0f ? 64.0f / e : 0.0f; }
  g.direction_major = ctx->sort.key == 1 ? 1u : 0u;
  Launch l(ctx, stream, LUMC_KERNEL_SORT);
  const uint32_t blocks = std::min<uint32_t>((capacity + 255u) / 256u, 4096u);
  hipLaunchKernelGGL(k_ray_sort_keys, dim3(blocks ? blocks : 1), dim3(256), 0, stream, origin, dir, count, capacity, g, ctx->sort.d_keys[0].get(), ctx->sort.d_vals[0].get());
  hipcub::DoubleBuffer<uint32_t> keys(ctx->sort.d_keys[0].get(), ctx->sort.d_keys[1].get()), vals(ctx->sort.d_vals[0].get(), ctx->sort.d_vals[1].get());
  size_t bytes = ctx->sort.temp_bytes;
  if (hipcub::DeviceRadixSort::SortPairs(ctx->sort.d_temp.get(), bytes, keys, vals, (int) capacity, 0, 22, stream) != hipSuccess) return nullptr;
  return vals.Current();
}

// Mode 3, the physical reorder: the planes change places, the permutation is spent.
static int reorder_queue(LumContext* ctx, hipStream_t stream, PathQueue& q, const uint32_t* order, uint32_t* ctrl, uint32_t N) {
  if (ensure_sort_queue(ctx, ctx->work.capacity)) return 1;
  Launch l(ctx, stream, LUMC_KERNEL_SORT);
  hipLaunchKernelGGL(k_permute_queue, dim3(std::min<uint32_t>((N + 255u) / 256u, 65536u)), dim3(256), 0, stream, q, ctx->sort.queue, order, ctrl + kCtlPaths, N);
  std::swap(q.origin_t, ctx->sort.queue.origin_t); std::swap(q.dir_slot, ctx->sort.queue.dir_slot);
  std::swap(q.aux, ctx->sort.queue.aux); std::swap(q.hit_id, ctx->sort.queue.hit_id);
  ctx->fused.records_stale = true;  // (the fused resolve does not run with ray sorting; a later pass without it must not read the old planes)
  return 0;
}

// The closest-hit rays of a depth, sorted (modes 1 to 3): *order is the permutation to trace `queue` through, nullptr when the queue itself was reordered.
int sort_closest_rays(LumContext* ctx, hipStream_t stream, PathQueue& queue, uint32_t* ctrl, uint32_t N, const uint32_t** order) {
  *order = sort_rays(ctx, stream, queue.origin_t, queue.dir_slot, ctrl + kCtlPaths, N);
  if (!*order) { ctx->error = "ray sorting failed"; return 1; }
  if (ctx->sort.mode == 3) {
    if (reorder_queue(ctx, stream, queue, *order, ctrl, N)) return 1;
    *order = nullptr;
  }
  return 0;
}

// The buffers of every mode; the settings (mode, key) and the scene's bounds stay.
void free_sort(LumContext* ctx) {
  LumContext::RaySort& s = ctx->sort;
  for (auto& plane : s.planes) plane.reset();
  s.queue = PathQueue{};
  for (int k = 0; k < 2; k++) { s.d_keys[k].reset(); s.d_vals[k].reset(); }
  s.d_temp.reset();
}

extern "C" {

int lumc_set_ray_sorting(LumContext* ctx, int mode) {
  if (!ctx || mode < 0 || mode > 3) { if (ctx) ctx->error = "lumc_set_ray_sorting: 0 (queue order), 1 (closest-hit rays sorted), 2 (visibility rays too), 3 (path queue physically reordered)"; return 1; }
  ctx->sort.mode = mode;
  return 0;
}
int lumc_get_ray_sorting(const LumContext* ctx) { return ctx ? ctx->sort.mode : 0; }

}  // extern "C"
