// The visibility-ray kernel (optix/optix_kernel_shadow.cu:15-100, cuda/optix_anyhit.cuh:49-139) and its query type, in a header of their own because the
// fast flavour compiles the kernel in ITS OWN translation unit (csrc/device/wavefront_fast_shadow.hip) with another instruction scheduler:
// `-mllvm -amdgpu-sched-strategy=max-ilp` takes 3-4 % off k_shadow_rays (hall 180.2 -> 172.4 ms per 3 steps, scan 40.9 -> 39.8, Example-class 26.65 -> 25.8)
// and ADDS 2.4 % to k_shade and 0.8 % to k_trace when applied to the whole flavour (profiles/r05_ab_experiments.txt) - the option is per translation unit.
// LUM_SHADOW_KERNEL_EXTERN=1 (a flavour's main unit: wavefront_fast.hip, wavefront_exact.hip): the kernel is declared here and defined in wavefront_<flavour>_shadow.hip; the
// host stub and the code object come from the defining unit, the launch and hipFuncSetAttribute in wavefront_table_impl.h go through the declaration. The
// scheduler reorders instructions and changes none: the exact flavour's kernel stays bit-identical to the oracle.
#pragma once

#include "dev_trace.h"

#ifndef LUM_SHADOW_KERNEL_EXTERN
#define LUM_SHADOW_KERNEL_EXTERN 0
#endif

LUM_NS_BEGIN

struct ShadowQuery : ShadowState {
  ShadowQueue sq;
  const uint32_t* order;
  uint32_t out;
  LUM_DEV bool load(const DeviceScene&, uint32_t slot, V3& o, V3& d, float& tmax) {
    const uint32_t j = order ? order[slot] : slot;
    const float4 o4 = ld_stream(&sq.origin_dist[j]), d4 = ld_stream(&sq.dir_out[j]);
    begin(ld_stream(&sq.ids[j]), o4.w);
    out = fbits(d4.w);
    o = v3(o4.x, o4.y, o4.z); d = v3(d4.x, d4.y, d4.z); tmax = o4.w;
    return true;
  }
  LUM_DEV void finish(const DeviceScene&, uint32_t) {
    const Col v = result();
#ifdef LUM_PHASE_STATS
    { const uint32_t kind = min(out / sq.capacity, 3u); atomicAdd(&g_vis_stat[2u * kind], 1ull); if (blocked) atomicAdd(&g_vis_stat[2u * kind + 1u], 1ull); }
#endif
    st_stream(&sq.vis[out], make_float4(v.r, v.g, v.b, 0.0f));
  }
};

// Two forms (trace_items, dev_trace.h): the plain kernel walks both levels, the template's one instance <true> a scene of one hittable instance from its mesh
// root; the launcher picks one per launch. Both live in the defining unit, under its scheduler option.
template <bool kSingleLevel>
__global__ LUM_TRACE_BOUNDS void k_shadow_rays(DeviceScene sc, ShadowQueue sq, const uint32_t* order, uint32_t* ctrl, uint64_t* counters, uint32_t lds_nodes);
#if LUM_SHADOW_KERNEL_EXTERN
__global__ LUM_TRACE_BOUNDS void k_shadow_rays(DeviceScene sc, ShadowQueue sq, const uint32_t* order, uint32_t* ctrl, uint64_t* counters, uint32_t lds_nodes);
extern template __global__ void k_shadow_rays<true>(DeviceScene sc, ShadowQueue sq, const uint32_t* order, uint32_t* ctrl, uint64_t* counters, uint32_t lds_nodes);
#else
__global__ LUM_TRACE_BOUNDS void k_shadow_rays(DeviceScene sc, ShadowQueue sq, const uint32_t* order, uint32_t* ctrl, uint64_t* counters, uint32_t lds_nodes) {
  RayStats st{0, 0, 0};
  uint32_t rays = 0;
  ShadowQuery q;
  q.sq = sq;
  q.order = order;
  trace_items(sc, ctrl[kCtlShadowItems], ctrl + kCtlShadowCursor, q, st, rays, lds_nodes);
  flush_stats(counters, st, rays, kCntShadow, kCntNodesShadow, kCntTrisShadow, kCntNodesLdsShadow);
}
template <bool kSingleLevel>
__global__ LUM_TRACE_BOUNDS void k_shadow_rays(DeviceScene sc, ShadowQueue sq, const uint32_t* order, uint32_t* ctrl, uint64_t* counters, uint32_t lds_nodes) {
  static_assert(kSingleLevel, "the two-level form is the plain kernel of this name");
  RayStats st{0, 0, 0};
  uint32_t rays = 0;
  ShadowQuery q;
  q.sq = sq;
  q.order = order;
  trace_items<ShadowQuery, true>(sc, ctrl[kCtlShadowItems], ctrl + kCtlShadowCursor, q, st, rays, lds_nodes);
  flush_stats(counters, st, rays, kCntShadow, kCntNodesShadow, kCntTrisShadow, kCntNodesLdsShadow);
}
template __global__ void k_shadow_rays<true>(DeviceScene sc, ShadowQueue sq, const uint32_t* order, uint32_t* ctrl, uint64_t* counters, uint32_t lds_nodes);
#endif

LUM_NS_END
