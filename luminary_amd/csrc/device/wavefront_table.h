// The wavefront kernels as a table of launchers, one table per arithmetic flavour (flavour.h). The host side (csrc/host/core.hip) picks a
// table per context (lumc_set_flavour) and launches through it; everything in the signatures is a plain layout from dev_scene.h.
// Kernels that produce data both flavours must agree on (BSDF / sky tables, panorama bake), bookkeeping (accumulation, adaptive rates) and
// the display chain exist once, in the exact flavour's namespace: kernels_shared.h, compiled in and launched directly by core.hip.
// The tests' probe kernels are no part of that table: WavefrontProbes below, filled by each flavour's probe unit and launched by csrc/host/probes.hip.
#pragma once

#include <hip/hip_runtime.h>

#include "dev_scene.h"

namespace lum {

// The ray kernels have a single-level form for a scene of one hittable instance (trace_items, dev_trace.h): its top level is node 0 with one child and two leaf
// records, the instance's and the padding record. The launchers of trace, shadow_rays and trace_rays ask this at EVERY launch, so a scene update that adds or
// removes instances needs no invalidation; `single_level` in their signatures is the context's switch (lumc_set_single_level), never the decision itself.
inline bool single_level_scene(const DeviceScene& sc) { return sc.tlas_num_nodes == 1u && sc.tlas_num_leaves == 2u; }

// k_shade has a plain form (kernels.h k_shade<.., kPlain>) for a scene without translucent materials, with a flat light tree whose lights are all staged in LDS
// (dev_light.h LUM_LDS_LIGHTS) and untextured, without an ocean, under a constant-colour or HDRI sky: the refraction halves of the BSDF code, the light tree's
// descent, the textured light colour and the lights' reads from memory are not compiled into it. The scene's side of that is DeviceScene::traits, kept by every
// update of the parts it comes from (scene_device.hip scene_traits); the `shade` launcher asks at EVERY launch, `plain_form` in its signature is the context's
// switch (lumc_set_plain_form), never the decision itself.
inline bool plain_scene(const DeviceScene& sc) {
  return (sc.traits & kTraitsPlain) == kTraitsPlain && sc.num_lights <= (uint32_t) LUM_LDS_LIGHTS && !sc.ocean_active &&
         (sc.sky_mode == kSkyConstantColor || sc.sky_mode == kSkyHdri);
}

struct WavefrontKernels {
  const char* flavour;
  uint32_t trace_block;  // threads per workgroup of the persistent ray kernels (one workgroup per CU)
  // dynamic LDS of the persistent ray kernels (the staged tree top); returns a hipError_t
  int (*set_ray_kernel_lds)(size_t bytes);
  // fills this flavour's table of sampler seeds on the current device (dev_sampler.h); returns a hipError_t
  int (*init_sampler_seeds)();
  // the Sobol / Owen pairs of a pass's sample ids for `dims` dimensions, rows of `stride` entries (dev_sampler.h LUM_SOBOL_TABLE)
  void (*sobol_table)(hipStream_t s, uint2* table, uint32_t first_sample, uint32_t count, uint32_t stride, uint32_t dims);
  // the camera paths of a pass; cam: CameraKind (dev_scene.h), `lens` is read by the physical camera only
  void (*generate)(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PassParams& pp, const PathQueue& q, float4* results, uint32_t* count, const DeviceLens& lens,
                   int cam);
  void (*generate_adaptive)(uint32_t grid, hipStream_t s, const DeviceScene& sc, const AdaptiveView& a, const AdaptivePass& pass, const PathQueue& q, float4* results,
                            uint32_t* count, const DeviceLens& lens, int cam);
  void (*trace)(uint32_t grid, size_t lds, hipStream_t s, const DeviceScene& sc, const PathQueue& q, const uint32_t* order, uint32_t* ctrl, uint64_t* counters,
                uint32_t lds_nodes, bool single_level, bool coherent);  // coherent: the waves hold rays that walk as one (trace_items<Q, true, true>; single-level scenes only)
  void (*sky_inscattering)(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, float4* results, const uint32_t* ctrl, uint32_t depth_const);
  void (*shade)(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, const PathQueue& out, const NeeQueue& nee, const ShadowQueue& sq, float4* results,
                uint32_t* ctrl, uint32_t depth_const, uint64_t* counters, uint32_t ambient_reuse, const FusedResolve* fused_dev, uint32_t fused_flags,
                bool plain_form);  // fused_dev: device memory; flags: 1 resolve the entries' parents, 2 announce the survivors' entries; plain_form: the switch (plain_scene above)
  void (*shade_debug)(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, float4* results, const uint32_t* ctrl);
  void (*sky)(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, const ShadowQueue& sq, float4* results, const uint32_t* ctrl, uint32_t depth_const);
  void (*light_query)(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, const NeeQueue& nee, const ShadowQueue& sq, uint32_t* ctrl, uint32_t depth_const,
                      uint64_t* counters);
  void (*shadow_rays)(uint32_t grid, size_t lds, hipStream_t s, const DeviceScene& sc, const ShadowQueue& sq, const uint32_t* order, uint32_t* ctrl, uint64_t* counters,
                      uint32_t lds_nodes, bool single_level);
  void (*resolve)(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, const NeeQueue& nee, const ShadowQueue& sq, float4* results, const uint32_t* ctrl);
  // ambient-visibility reuse (kernels.h, above TraceQuery): the resolve of a depth after the NEXT depth's closest-hit pass over `next`, and of the vertices it listed
  void (*resolve_reuse)(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, const PathQueue& next, const NeeQueue& nee, const ShadowQueue& sq, float4* results,
                        uint32_t* ctrl, uint64_t* counters);
  void (*resolve_listed)(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, const NeeQueue& nee, const ShadowQueue& sq, float4* results, const uint32_t* ctrl);
  void (*resolve_ended)(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, const NeeQueue& nee, const ShadowQueue& sq, float4* results, const uint32_t* ctrl,
                        const uint32_t* list);
  bool fused_resolve;  // k_shade resolves the previous depth's vertices itself when asked to (FusedResolve; the fast flavour only)
  // fog (dev_volume.h): light scattered into the rays of a depth, its summation, the scattering events and their bounce
  void (*volume_inscatter)(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, const VolumeQueue& vq, const ShadowQueue& sq, uint32_t* ctrl,
                           uint32_t depth_const);
  void (*volume_resolve)(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, const VolumeQueue& vq, const ShadowQueue& sq, float4* results,
                         const uint32_t* ctrl);
  void (*volume_events)(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, const VolumeQueue& vq, float4* results, uint32_t* ctrl, uint32_t depth_const);
  void (*volume_bounce)(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, const PathQueue& out, const VolumeQueue& vq, uint32_t* ctrl,
                        uint32_t depth_const);
  // particles (dev_particle.h): the particle pass of the closest-hit kernel (`particle_tree`: the scene with the particle tree in place of the
  // surfaces' tree) and the shading of particle hits
  void (*trace_particles)(uint32_t grid, size_t lds, hipStream_t s, const DeviceScene& particle_tree, const PathQueue& q, uint32_t* ctrl, uint32_t lds_nodes);
  void (*particle_shade)(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, const PathQueue& out, const NeeQueue& nee, const ShadowQueue& sq,
                         uint32_t* ctrl, uint32_t depth_const);
  // ocean (dev_ocean.h, dev_water.h): the height-field pass of the closest-hit kernel and the shading of water-surface hits
  void (*trace_ocean)(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& q, const uint32_t* ctrl);
  void (*ocean_shade)(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, const PathQueue& out, const NeeQueue& nee, const ShadowQueue& sq, uint32_t* ctrl,
                      uint32_t depth_const);
  // clouds (dev_cloud.h, dev_cloud_march.h): the march through the cloud layers, sky mode DEFAULT only
  void (*clouds_list)(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, const CloudQueue& cq, uint32_t* ctrl);
  void (*clouds_march)(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, const CloudQueue& cq, uint32_t* ctrl, uint32_t depth_const);
  void (*clouds)(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, const CloudQueue& cq, float4* results, const uint32_t* ctrl, uint32_t depth_const);
  void (*trace_rays)(uint32_t grid, size_t lds, hipStream_t s, const DeviceScene& sc, uint32_t n, const float* origins, const float* dirs, const uint32_t* ignore, uint32_t* out,
                     uint32_t* cursor, uint64_t* counters, uint32_t lds_nodes, bool single_level, bool coherent);
  // every camera ray of `samples` sample ids of n pixels (device buffers; origin / dir float3, weight float), the invalid ones included (k_camera_rays)
  void (*camera_rays)(uint32_t grid, hipStream_t s, const DeviceScene& sc, const DeviceLens& lens, int cam, const uint32_t* pixels, uint32_t n, uint32_t first_sample,
                      uint32_t samples, float* origin, float* dir, float* weight);
  // denoiser (dev_denoise.h): first-hit guides of the paths of one sample id after a closest-hit pass (`planes`: 9 sum planes of n pixels), their means, and the
  // filter's three stages; `lds`: the a-trous iteration stages its tile and halo in LDS (steps 1 and 2 only)
  void (*guide)(uint32_t grid, hipStream_t s, const DeviceScene& sc, const PathQueue& in, const uint32_t* ctrl, float* planes, uint32_t n);
  void (*guide_normalise)(uint32_t grid, hipStream_t s, float* planes, uint32_t n, uint32_t samples);
  void (*denoise_prepare)(uint32_t grid, hipStream_t s, const AdaptiveView& a, const DenoiseArgs& p, const float* fm, const float* sm, const float* image, const float* guides,
                          float4* rec_a, uint4* rec_b);
  void (*denoise_atrous)(hipStream_t s, const DenoiseArgs& p, const float4* a_in, const uint4* rec_b, float4* a_out, bool lds);
  void (*denoise_finish)(uint32_t grid, hipStream_t s, const DenoiseArgs& p, const float4* rec_a, const float* guides, float* image);
};
// The truth probes: kernels that only the tests launch and whose signatures follow a test's needs (kernels_probe.h; the records' word counts: probe_layout.h). They
// live in units of their own with a table of their own, one per flavour like the kernels': the render's launcher table above keeps its shape when a probe comes or goes.
struct WavefrontProbes {
  // fills the probe unit's own table of sampler seeds on the current device (dev_sampler.h); returns a hipError_t
  int (*init_sampler_seeds)();
  // the light-BVH query of n plain rays, one per thread (k_light_query_probe; device buffers: float3 origins / dirs, uint2 self handles, float randoms)
  void (*light_query_probe)(hipStream_t s, const DeviceScene& sc, uint32_t n, const float* origins, const float* dirs, const uint32_t* self, const float* randoms, uint32_t* out_ids,
                            uint32_t* out_num_hits);
  // sample_light on n_vertices caller-made vertices x `samples` sample ids, one per thread (k_light_sample_probe: kLightProbeVertexWords in per vertex, kLightProbeWords out per thread);
  // form: 0 the general form, 1 the plain form (the caller has asked plain_scene), 2 the general form with no light staged in LDS
  void (*light_sample_probe)(hipStream_t s, const DeviceScene& sc, uint32_t n_vertices, uint32_t samples, uint32_t first_sample, uint32_t form, const uint32_t* vertices,
                             uint32_t* out);
  // sample_bounce and sample_light_direction on the same vertices, one (vertex, sample id) per thread (k_bounce_probe: kBounceProbeWordsPerThread out per thread)
  void (*bounce_probe)(hipStream_t s, const DeviceScene& sc, uint32_t n_vertices, uint32_t samples, uint32_t first_sample, const uint32_t* vertices, uint32_t* out);
  // sky_get_color or sky_trace_inscattering on n caller-made rays, one per thread (k_sky_probe: kSkyProbeRayWords in per ray, kSkyProbeWordsPerThread out per thread)
  void (*sky_probe)(hipStream_t s, const DeviceScene& sc, uint32_t n, const uint32_t* rays, uint32_t* out);
  // sample_sun on the light probe's caller-made vertices, one (vertex, sample id) per thread (k_sun_probe: kSunProbeWordsPerThread out per thread)
  void (*sun_probe)(hipStream_t s, const DeviceScene& sc, uint32_t n_vertices, uint32_t samples, uint32_t first_sample, const uint32_t* vertices, uint32_t* out);
  // v_exp_f32 (op 0), v_sin_f32 (1), v_cos_f32 (2) of n arguments (k_sky_math_probe)
  void (*sky_math_probe)(hipStream_t s, uint32_t n, uint32_t op, const float* x, float* y);
};

const WavefrontKernels* wavefront_kernels_exact();  // csrc/device/wavefront_exact.hip
const WavefrontKernels* wavefront_kernels_fast();   // csrc/device/wavefront_fast.hip
const WavefrontProbes* wavefront_probes_exact();    // csrc/device/wavefront_exact_probes.hip
const WavefrontProbes* wavefront_probes_fast();     // csrc/device/wavefront_fast_probes.hip
// The vector registers per lane (hipFuncGetAttributes numRegs) of a flavour's closest-hit kernel in the given form and of its k_light_query, on the current device:
// what the host asks before it lets the two run side by side (csrc/host/context.h overlap_registers_fit). They return a hipError_t.
int ray_kernel_registers_exact(bool single_level, uint32_t* trace_regs, uint32_t* light_query_regs);
int ray_kernel_registers_fast(bool single_level, uint32_t* trace_regs, uint32_t* light_query_regs);

}  // namespace lum
