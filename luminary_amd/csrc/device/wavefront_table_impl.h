// Defines this translation unit's WavefrontKernels table: the whole of a flavour's main unit (wavefront_exact.hip, wavefront_fast.hip).
#pragma once

#include "dev_adaptive.h"
#include "dev_denoise.h"
#include "wavefront_table.h"

LUM_NS_BEGIN
namespace table {

// The ray kernels by form: the plain kernel walks both levels, the template's instance <true> of the same name is the single-level form (kernels.h, kernel_shadow.h).
typedef void (*TraceKernel)(DeviceScene, PathQueue, const uint32_t*, uint32_t*, uint64_t*, uint32_t);
typedef void (*ShadowKernel)(DeviceScene, ShadowQueue, const uint32_t*, uint32_t*, uint64_t*, uint32_t);
typedef void (*TraceRaysKernel)(DeviceScene, uint32_t, const float*, const float*, const uint32_t*, uint32_t*, uint32_t*, uint64_t*, uint32_t);
// (coherent: the single-level form for waves of rays that walk as one, the template's instance <true, true> - a single-level form, so it follows `single`)
static TraceKernel trace_kernel(bool single, bool coherent = false) { return single ? (coherent ? k_trace<true, true> : k_trace<true>) : static_cast<TraceKernel>(k_trace); }
static ShadowKernel shadow_kernel(bool single) { return single ? k_shadow_rays<true> : static_cast<ShadowKernel>(k_shadow_rays); }
static TraceRaysKernel trace_rays_kernel(bool single, bool coherent = false) {
  return single ? (coherent ? k_trace_rays<true, true> : k_trace_rays<true>) : static_cast<TraceRaysKernel>(k_trace_rays);
}

static int set_ray_kernel_lds(size_t bytes) {
  hipError_t e = hipSuccess;
  for (int single = 0; single < 2 && e == hipSuccess; single++) {
    e = hipFuncSetAttribute((const void*) trace_kernel(single != 0), hipFuncAttributeMaxDynamicSharedMemorySize, (int) bytes);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*) shadow_kernel(single != 0), hipFuncAttributeMaxDynamicSharedMemorySize, (int) bytes);
    if (e == hipSuccess) e = hipFuncSetAttribute((const void*) trace_rays_kernel(single != 0), hipFuncAttributeMaxDynamicSharedMemorySize, (int) bytes);
  }
  if (e == hipSuccess) e = hipFuncSetAttribute((const void*) trace_kernel(true, true), hipFuncAttributeMaxDynamicSharedMemorySize, (int) bytes);
  if (e == hipSuccess) e = hipFuncSetAttribute((const void*) trace_rays_kernel(true, true), hipFuncAttributeMaxDynamicSharedMemorySize, (int) bytes);
  if (e == hipSuccess) e = hipFuncSetAttribute((const void*) k_trace_particles, hipFuncAttributeMaxDynamicSharedMemorySize, (int) bytes);
  return (int) e;
}
static int ray_kernel_registers(bool single_level, uint32_t* trace_regs, uint32_t* light_query_regs) {
  hipFuncAttributes a{};
  hipError_t e = hipFuncGetAttributes(&a, (const void*) trace_kernel(single_level));
  if (e != hipSuccess) return (int) e;
  *trace_regs = (uint32_t) a.numRegs;
  e = hipFuncGetAttributes(&a, (const void*) k_light_query);
  if (e == hipSuccess) *light_query_regs = (uint32_t) a.numRegs;
  return (int) e;
}
static int init_sampler_seeds() { return upload_sampler_seeds(); }
static void sobol_table(hipStream_t s, uint2* table, uint32_t first_sample, uint32_t count, uint32_t stride, uint32_t dims) {
  hipLaunchKernelGGL(k_sobol_table, dim3((dims * stride + 255u) / 256u), dim3(256), 0, s, table, first_sample, count, stride, dims);
}
static void generate(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PassParams& pp, const PathQueue& q, float4* results, uint32_t* count, const DeviceLens& lens,
                     int cam) {
  auto* k = cam == kCamPhysical ? k_generate<kCamPhysical> : cam == kCamPhysicalReflections ? k_generate<kCamPhysicalReflections> : k_generate<kCamThinLens>;
  hipLaunchKernelGGL(k, dim3(grid), dim3(kBlock), 0, s, sc, pp, q, results, count, lens);
}
static void generate_adaptive(uint32_t grid, hipStream_t s, const DeviceScene& sc, const AdaptiveView& a, const AdaptivePass& pass, const PathQueue& q, float4* results,
                              uint32_t* count, const DeviceLens& lens, int cam) {
  auto* k = cam == kCamPhysical ? k_generate_adaptive<kCamPhysical> : cam == kCamPhysicalReflections ? k_generate_adaptive<kCamPhysicalReflections>
                                                                                                     : k_generate_adaptive<kCamThinLens>;
  hipLaunchKernelGGL(k, dim3(grid), dim3(kBlock), 0, s, sc, a, pass, q, results, count, lens);
}
static void camera_rays(uint32_t grid, hipStream_t s, const DeviceScene& sc, const DeviceLens& lens, int cam, const uint32_t* pixels, uint32_t n, uint32_t first_sample,
                        uint32_t samples, float* origin, float* dir, float* weight) {
  auto* k = cam == kCamPhysical ? k_camera_rays<kCamPhysical> : cam == kCamPhysicalReflections ? k_camera_rays<kCamPhysicalReflections> : k_camera_rays<kCamThinLens>;
  hipLaunchKernelGGL(k, dim3(grid), dim3(kBlock), 0, s, sc, lens, pixels, n, first_sample, samples, origin, dir, weight);
}
static void trace(uint32_t grid, size_t lds, hipStream_t s, const DeviceScene& sc, const PathQueue& q, const uint32_t* order, uint32_t* ctrl, uint64_t* counters,
                  uint32_t lds_nodes, bool single_level, bool coherent) {
  hipLaunchKernelGGL(trace_kernel(single_level && single_level_scene(sc), coherent), dim3(grid), dim3(kTraceBlock), lds, s, sc, q, order, ctrl, counters, lds_nodes);
}
static void sky_inscattering(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, float4* results, const uint32_t* ctrl, uint32_t depth_const) {
  hipLaunchKernelGGL(k_sky_inscattering, dim3(grid), dim3(kBlock), 0, s, sc, in, results, ctrl, depth_const);
}
static void shade(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, const PathQueue& out, const NeeQueue& nee, const ShadowQueue& sq, float4* results,
                  uint32_t* ctrl, uint32_t depth_const, uint64_t* counters, uint32_t ambient_reuse, const FusedResolve* fused_dev, uint32_t fused_flags, bool plain_form) {
  auto* k = sc.sky_mode == kSkyDefault ? k_shade<kSkyDefault, false> : sc.sky_mode == kSkyHdri ? k_shade<kSkyHdri, false> : k_shade<kSkyConstantColor, false>;
  if (sc.ocean_active) k = sc.sky_mode == kSkyDefault ? k_shade<kSkyDefault, true> : sc.sky_mode == kSkyHdri ? k_shade<kSkyHdri, true> : k_shade<kSkyConstantColor, true>;
  if (sc.sobol_table) {  // the pass has a Sobol table (dev_sampler.h): the instances that read it instead of hashing
    k = sc.sky_mode == kSkyDefault ? k_shade<kSkyDefault, false, true> : sc.sky_mode == kSkyHdri ? k_shade<kSkyHdri, false, true> : k_shade<kSkyConstantColor, false, true>;
    if (sc.ocean_active) k = sc.sky_mode == kSkyDefault ? k_shade<kSkyDefault, true, true> : sc.sky_mode == kSkyHdri ? k_shade<kSkyHdri, true, true> : k_shade<kSkyConstantColor, true, true>;
  }
  if (plain_form && plain_scene(sc)) {  // the plain form (plain_scene, wavefront_table.h): no ocean, one of these two sky modes
    if (sc.sobol_table) k = sc.sky_mode == kSkyHdri ? k_shade<kSkyHdri, false, true, true> : k_shade<kSkyConstantColor, false, true, true>;
    else k = sc.sky_mode == kSkyHdri ? k_shade<kSkyHdri, false, false, true> : k_shade<kSkyConstantColor, false, false, true>;
  }
  hipLaunchKernelGGL(k, dim3(grid), dim3(kBlock), 0, s, sc, in, out, nee, sq, results, ctrl, depth_const, counters, ambient_reuse, fused_dev, fused_flags);
}
static void shade_debug(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, float4* results, const uint32_t* ctrl) {
  hipLaunchKernelGGL(k_shade_debug, dim3(grid), dim3(kBlock), 0, s, sc, in, results, ctrl);
}
static void sky(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, const ShadowQueue& sq, float4* results, const uint32_t* ctrl, uint32_t depth_const) {
  hipLaunchKernelGGL(k_sky, dim3(grid), dim3(kBlock), 0, s, sc, in, sq, results, ctrl, depth_const);
}
static void light_query(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, const NeeQueue& nee, const ShadowQueue& sq, uint32_t* ctrl, uint32_t depth_const,
                        uint64_t* counters) {
  hipLaunchKernelGGL(k_light_query, dim3(grid), dim3(kBlock), 0, s, sc, in, nee, sq, ctrl, depth_const, counters);
}
static void shadow_rays(uint32_t grid, size_t lds, hipStream_t s, const DeviceScene& sc, const ShadowQueue& sq, const uint32_t* order, uint32_t* ctrl, uint64_t* counters,
                        uint32_t lds_nodes, bool single_level) {
  hipLaunchKernelGGL(shadow_kernel(single_level && single_level_scene(sc)), dim3(grid), dim3(kTraceBlock), lds, s, sc, sq, order, ctrl, counters, lds_nodes);
}
static void resolve(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, const NeeQueue& nee, const ShadowQueue& sq, float4* results, const uint32_t* ctrl) {
  hipLaunchKernelGGL(k_resolve, dim3(grid), dim3(kBlock), 0, s, sc, in, nee, sq, results, ctrl);
}
static void resolve_reuse(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, const PathQueue& next, const NeeQueue& nee, const ShadowQueue& sq, float4* results,
                          uint32_t* ctrl, uint64_t* counters) {
  hipLaunchKernelGGL(k_resolve_reuse, dim3(grid), dim3(kBlock), 0, s, sc, in, next, nee, sq, results, ctrl, counters);
}
static void resolve_listed(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, const NeeQueue& nee, const ShadowQueue& sq, float4* results, const uint32_t* ctrl) {
  hipLaunchKernelGGL(k_resolve_listed, dim3(grid), dim3(kBlock), 0, s, sc, in, nee, sq, results, ctrl);
}
static void resolve_ended(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, const NeeQueue& nee, const ShadowQueue& sq, float4* results, const uint32_t* ctrl,
                          const uint32_t* list) {
  hipLaunchKernelGGL(k_resolve_ended, dim3(grid), dim3(kBlock), 0, s, sc, in, nee, sq, results, ctrl, list);
}
static void volume_inscatter(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, const VolumeQueue& vq, const ShadowQueue& sq, uint32_t* ctrl,
                             uint32_t depth_const) {
  hipLaunchKernelGGL(k_volume_inscatter, dim3(grid), dim3(kBlock), 0, s, sc, in, vq, sq, ctrl, depth_const);
}
static void volume_resolve(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, const VolumeQueue& vq, const ShadowQueue& sq, float4* results,
                           const uint32_t* ctrl) {
  hipLaunchKernelGGL(k_volume_resolve, dim3(grid), dim3(kBlock), 0, s, sc, in, vq, sq, results, ctrl);
}
static void volume_events(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, const VolumeQueue& vq, float4* results, uint32_t* ctrl,
                          uint32_t depth_const) {
  hipLaunchKernelGGL(k_volume_events, dim3(grid), dim3(kBlock), 0, s, sc, in, vq, results, ctrl, depth_const);
}
static void volume_bounce(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, const PathQueue& out, const VolumeQueue& vq, uint32_t* ctrl,
                          uint32_t depth_const) {
  hipLaunchKernelGGL(k_volume_bounce, dim3(grid), dim3(kBlock), 0, s, sc, in, out, vq, ctrl, depth_const);
}
static void trace_particles(uint32_t grid, size_t lds, hipStream_t s, const DeviceScene& particle_tree, const PathQueue& q, uint32_t* ctrl, uint32_t lds_nodes) {
  hipLaunchKernelGGL(k_trace_particles, dim3(grid), dim3(kTraceBlock), lds, s, particle_tree, q, ctrl, lds_nodes);
}
static void particle_shade(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, const PathQueue& out, const NeeQueue& nee, const ShadowQueue& sq,
                           uint32_t* ctrl, uint32_t depth_const) {
  hipLaunchKernelGGL(k_particle_shade, dim3(grid), dim3(kBlock), 0, s, sc, in, out, nee, sq, ctrl, depth_const);
}
static void trace_ocean(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& q, const uint32_t* ctrl) {
  hipLaunchKernelGGL(k_trace_ocean, dim3(grid), dim3(kBlock), 0, s, sc, q, ctrl);
}
static void ocean_shade(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, const PathQueue& out, const NeeQueue& nee, const ShadowQueue& sq,
                        uint32_t* ctrl, uint32_t depth_const) {
  hipLaunchKernelGGL(k_ocean_shade, dim3(grid), dim3(kBlock), 0, s, sc, in, out, nee, sq, ctrl, depth_const);
}
static void clouds_list(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, const CloudQueue& cq, uint32_t* ctrl) {
  hipLaunchKernelGGL(k_clouds_list, dim3(grid), dim3(kBlock), 0, s, sc, in, cq, ctrl);
}
static void clouds_march(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, const CloudQueue& cq, uint32_t* ctrl, uint32_t depth_const) {
  hipLaunchKernelGGL(k_clouds_march, dim3(grid), dim3(kBlock), 0, s, sc, in, cq, ctrl, depth_const);
}
static void clouds(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, const CloudQueue& cq, float4* results, const uint32_t* ctrl, uint32_t depth_const) {
  hipLaunchKernelGGL(k_clouds, dim3(grid), dim3(kBlock), 0, s, sc, in, cq, results, ctrl, depth_const);
}
static void trace_rays(uint32_t grid, size_t lds, hipStream_t s, const DeviceScene& sc, uint32_t n, const float* origins, const float* dirs, const uint32_t* ignore, uint32_t* out,
                       uint32_t* cursor, uint64_t* counters, uint32_t lds_nodes, bool single_level, bool coherent) {
  hipLaunchKernelGGL(trace_rays_kernel(single_level && single_level_scene(sc), coherent), dim3(grid), dim3(kTraceBlock), lds, s, sc, n, origins, dirs, ignore, out, cursor, counters,
                     lds_nodes);
}
static void guide(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, const uint32_t* ctrl, float* planes, uint32_t n) {
  hipLaunchKernelGGL(k_guide, dim3(grid), dim3(kBlock), 0, s, sc, in, ctrl, planes, n);
}
static void guide_normalise(uint32_t grid, hipStream_t s, float* planes, uint32_t n, uint32_t samples) {
  hipLaunchKernelGGL(k_guide_normalise, dim3(grid), dim3(256), 0, s, planes, n, samples);
}
static void denoise_prepare(uint32_t grid, hipStream_t s, const AdaptiveView& a, const DenoiseArgs& p, const float* fm, const float* sm, const float* image, const float* guides,
                            float4* rec_a, uint4* rec_b) {
  hipLaunchKernelGGL(k_denoise_prepare, dim3(grid), dim3(256), 0, s, a, p, fm, sm, image, guides, rec_a, rec_b);
}
static void denoise_atrous(hipStream_t s, const DenoiseArgs& p, const float4* a_in, const uint4* rec_b, float4* a_out, bool lds) {
  const dim3 grid((p.width + kDenoiseTileX - 1u) / kDenoiseTileX, (p.height + kDenoiseTileY - 1u) / kDenoiseTileY);
  if (lds && p.step <= kDenoiseMaxLdsStep) hipLaunchKernelGGL(k_denoise_atrous<true>, grid, dim3(256), 0, s, p, a_in, rec_b, a_out);
  else hipLaunchKernelGGL(k_denoise_atrous<false>, grid, dim3(256), 0, s, p, a_in, rec_b, a_out);
}
static void denoise_finish(uint32_t grid, hipStream_t s, const DenoiseArgs& p, const float4* rec_a, const float* guides, float* image) {
  hipLaunchKernelGGL(k_denoise_finish, dim3(grid), dim3(256), 0, s, p, rec_a, guides, image);
}

// Filled by member name: neighbouring members share a function-pointer type (resolve / resolve_listed, particle_shade / ocean_shade, sky_inscattering / clouds),
// so a positional list with two of them swapped would compile. tests/test_build_units.py checks that no member stays null.
static constexpr WavefrontKernels make_table() {
  WavefrontKernels t{};
  t.flavour = LUM_FLAVOUR_NAME; t.trace_block = (uint32_t) kTraceBlock; t.set_ray_kernel_lds = set_ray_kernel_lds; t.init_sampler_seeds = init_sampler_seeds;
  t.sobol_table = sobol_table; t.generate = generate; t.generate_adaptive = generate_adaptive; t.trace = trace; t.sky_inscattering = sky_inscattering;
  t.shade = shade; t.shade_debug = shade_debug; t.sky = sky; t.light_query = light_query;
  t.shadow_rays = shadow_rays; t.resolve = resolve; t.resolve_reuse = resolve_reuse; t.resolve_listed = resolve_listed; t.resolve_ended = resolve_ended; t.fused_resolve = LUM_FAST != 0;
  t.volume_inscatter = volume_inscatter; t.volume_resolve = volume_resolve; t.volume_events = volume_events; t.volume_bounce = volume_bounce;
  t.trace_particles = trace_particles; t.particle_shade = particle_shade; t.trace_ocean = trace_ocean; t.ocean_shade = ocean_shade;
  t.clouds_list = clouds_list; t.clouds_march = clouds_march; t.clouds = clouds; t.trace_rays = trace_rays;
  t.camera_rays = camera_rays; t.guide = guide;
  t.guide_normalise = guide_normalise; t.denoise_prepare = denoise_prepare; t.denoise_atrous = denoise_atrous; t.denoise_finish = denoise_finish;
  return t;
}
static constexpr WavefrontKernels kTable = make_table();

}  // namespace table
LUM_NS_END

#ifdef LUM_PHASE_STATS
// each flavour's own counter blocks (dev_math.h), read by tools/phase_stats.py
#if LUM_FAST
extern "C" int lumc_debug_phase_stats_fast(uint64_t out[16], int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase), sizeof(uint64_t) * 16) != hipSuccess) return 1;
  if (reset) { const uint64_t zero[16] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_phase), zero, sizeof(zero)) != hipSuccess) return 1; }
  return 0;
}
extern "C" int lumc_debug_phase_times_fast(uint64_t out[16], int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase_time), sizeof(uint64_t) * 16) != hipSuccess) return 1;
  if (reset) { const uint64_t zero[16] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_phase_time), zero, sizeof(zero)) != hipSuccess) return 1; }
  return 0;
}
extern "C" int lumc_debug_vis_stats_fast(uint64_t out[8], int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_vis_stat), sizeof(uint64_t) * 8) != hipSuccess) return 1;
  if (reset) { const uint64_t zero[8] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_vis_stat), zero, sizeof(zero)) != hipSuccess) return 1; }
  return 0;
}
extern "C" int lumc_debug_shade_times_fast(uint64_t out[16], int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_shade_time), sizeof(uint64_t) * 16) != hipSuccess) return 1;
  if (reset) { const uint64_t zero[16] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_shade_time), zero, sizeof(zero)) != hipSuccess) return 1; }
  return 0;
}
#else
extern "C" int lumc_debug_phase_stats(uint64_t out[16], int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_phase), sizeof(uint64_t) * 16) != hipSuccess) return 1;
  if (reset) { const uint64_t zero[16] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_phase), zero, sizeof(zero)) != hipSuccess) return 1; }
  return 0;
}
#endif
#endif

namespace lum {
#if LUM_FAST
const WavefrontKernels* wavefront_kernels_fast() { return &fast::table::kTable; }
int ray_kernel_registers_fast(bool single_level, uint32_t* trace_regs, uint32_t* light_query_regs) { return fast::table::ray_kernel_registers(single_level, trace_regs, light_query_regs); }
#else
int ray_kernel_registers_exact(bool single_level, uint32_t* trace_regs, uint32_t* light_query_regs) { return exact::table::ray_kernel_registers(single_level, trace_regs, light_query_regs); }
const WavefrontKernels* wavefront_kernels_exact() { return &exact::table::kTable; }
#endif
}  // namespace lum
