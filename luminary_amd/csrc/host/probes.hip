// The entry points of the truth probes (include/lum_core.h lumc_*_probe_host, lumc_light_query_host): host code only. The kernels they launch are the flavours'
// probe units' (csrc/device/kernels_probe.h), reached through WavefrontProbes; each entry point checks its arguments and hands run_probe its launch.
#include <hip/hip_runtime.h>

#include <initializer_list>

#include "../../../include/lum_core.h"
#include "../device/probe_layout.h"
#include "context.h"

namespace {

struct ProbeIn { const void* host; size_t words; };
struct ProbeOut { void* host; size_t words; };

// One probe launch. The input arrays (32-bit words) go up one behind the other into d_in; d_out, as long as the output arrays together and filled with the byte
// `fill`, is what the kernel writes into; launch(d_in, d_out) enqueues the kernel on the null stream; d_out comes down into the output arrays, one behind the other.
template <typename LaunchProbe>
int run_probe(LumContext* ctx, std::initializer_list<ProbeIn> in, std::initializer_list<ProbeOut> out, int fill, LaunchProbe launch) {
  size_t in_words = 0, out_words = 0, at = 0;
  for (const ProbeIn& i : in) in_words += i.words;
  for (const ProbeOut& o : out) out_words += o.words;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  DeviceBuffer<uint32_t> d_in, d_out;
  HIP_TRY(ctx, d_in.resize(in_words));
  for (const ProbeIn& i : in) { HIP_TRY(ctx, hipMemcpy(d_in.get() + at, i.host, sizeof(uint32_t) * i.words, hipMemcpyHostToDevice)); at += i.words; }
  HIP_TRY(ctx, d_out.resize(out_words));
  HIP_TRY(ctx, hipMemset(d_out.get(), fill, sizeof(uint32_t) * out_words));
  launch(d_in.get(), d_out.get());
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipDeviceSynchronize());
  at = 0;
  for (const ProbeOut& o : out) { HIP_TRY(ctx, hipMemcpy(o.host, d_out.get() + at, sizeof(uint32_t) * o.words, hipMemcpyDeviceToHost)); at += o.words; }
  return 0;
}

}  // namespace

extern "C" {

// The light-BVH query of BSDF-sampled directions (light_query, dev_trace.h) on plain rays, in the active flavour: out_ids = the picked light or 0xFFFFFFFF, out_num_hits = the
// number of candidates. A scene without lights answers (0xFFFFFFFF, 0) without a launch.
int lumc_light_query_host(LumContext* ctx, uint32_t n, const float* origins, const float* dirs, const uint32_t* self, const float* randoms, uint32_t* out_ids, uint32_t* out_num_hits) {
  if (!ctx || !ctx->has_scene) { if (ctx) ctx->error = "lumc_light_query_host: no scene"; return 1; }
  if (n == 0) return 0;
  if (!origins || !dirs || !self || !randoms || !out_ids || !out_num_hits) { ctx->error = "lumc_light_query_host: null argument"; return 1; }
  const DeviceScene& sc = ctx->scene;
  if (!sc.num_lights || !sc.light_nodes || !sc.light_tris || !sc.light_tri_handles) {
    for (uint32_t i = 0; i < n; i++) { out_ids[i] = 0xFFFFFFFFu; out_num_hits[i] = 0u; }
    return 0;
  }
  const size_t N = n;
  return run_probe(ctx, {{origins, 3 * N}, {dirs, 3 * N}, {self, 2 * N}, {randoms, N}}, {{out_ids, N}, {out_num_hits, N}}, 0xFF, [&](const uint32_t* d_in, uint32_t* d_out) {
    const float* f = reinterpret_cast<const float*>(d_in);
    probes_of(ctx)->light_query_probe(nullptr, sc, n, f, f + 3 * N, d_in + 6 * N, f + 8 * N, d_out, d_out + N);
  });
}

// sample_light (dev_light.h) on caller-made vertices in the active flavour: num_vertices records of LUMC_LIGHT_PROBE_VERTEX_WORDS words, each sampled with the sample ids
// first_sample .. first_sample + samples - 1; out: LUMC_LIGHT_PROBE_WORDS words per (vertex, sample id), zero where a lane did not get that far (k_light_sample_probe,
// kernels_probe.h). form: LUMC_LIGHT_PROBE_GENERAL, _PLAIN (refused unless the scene is one k_shade's plain form shades and no vertex is translucent), _UNSTAGED.
int lumc_light_sample_probe_host(LumContext* ctx, uint32_t num_vertices, const uint32_t* vertices, uint32_t first_sample, uint32_t samples, int form, uint32_t* out) {
  static_assert(LUMC_LIGHT_PROBE_VERTEX_WORDS == kLightProbeVertexWords && LUMC_LIGHT_PROBE_WORDS == kLightProbeWords, "lum_core.h and probe_layout.h");
  if (!ctx || !ctx->has_scene) { if (ctx) ctx->error = "lumc_light_sample_probe_host: no scene"; return 1; }
  if (num_vertices == 0 || samples == 0) return 0;
  if (!vertices || !out) { ctx->error = "lumc_light_sample_probe_host: null argument"; return 1; }
  if (form < LUMC_LIGHT_PROBE_GENERAL || form > LUMC_LIGHT_PROBE_UNSTAGED) { ctx->error = "lumc_light_sample_probe_host: unknown form"; return 1; }
  const DeviceScene& sc = ctx->scene;
  if (!sc.num_lights || !sc.light_tree_root || !sc.light_root_children || !sc.light_tri_table || !sc.light_tri_handles) { ctx->error = "lumc_light_sample_probe_host: the scene has no lights"; return 1; }
  const size_t n = (size_t) num_vertices * samples;
  if (n > (1u << 24)) { ctx->error = "lumc_light_sample_probe_host: more than 2^24 threads"; return 1; }
  if (form == LUMC_LIGHT_PROBE_PLAIN) {
    if (!plain_scene(sc)) { ctx->error = "lumc_light_sample_probe_host: the plain form does not shade this scene"; return 1; }
    for (uint32_t v = 0; v < num_vertices; v++)
      if (vertices[(size_t) v * kLightProbeVertexWords + 15] & 1u) { ctx->error = "lumc_light_sample_probe_host: a translucent vertex in the plain form"; return 1; }
  }
  return run_probe(ctx, {{vertices, (size_t) num_vertices * kLightProbeVertexWords}}, {{out, n * kLightProbeWords}}, 0, [&](const uint32_t* d_v, uint32_t* d_out) {
    probes_of(ctx)->light_sample_probe(nullptr, sc, num_vertices, samples, first_sample, (uint32_t) form, d_v, d_out);
  });
}

// sample_bounce (dev_bsdf.h) and sample_light_direction (dev_light.h) on the light probe's caller-made vertices in the active flavour, with their stages: out holds
// LUMC_BOUNCE_PROBE_WORDS words per (vertex, sample id), zero where a stage was not reached (k_bounce_probe, kernels_probe.h).
int lumc_bounce_probe_host(LumContext* ctx, uint32_t num_vertices, const uint32_t* vertices, uint32_t first_sample, uint32_t samples, uint32_t* out) {
  static_assert(LUMC_BOUNCE_PROBE_WORDS == kBounceProbeWordsPerThread, "lum_core.h and probe_layout.h");
  static_assert(LUMC_BOUNCE_PROBE_WORDS == LUMC_BOUNCE_PROBE_HEAD_WORDS + 3 * LUMC_BOUNCE_PROBE_TECH_WORDS + LUMC_BOUNCE_PROBE_LIGHT_DIR_WORDS, "lum_core.h");
  if (!ctx || !ctx->has_scene) { if (ctx) ctx->error = "lumc_bounce_probe_host: no scene"; return 1; }
  if (num_vertices == 0 || samples == 0) return 0;
  if (!vertices || !out) { ctx->error = "lumc_bounce_probe_host: null argument"; return 1; }
  const DeviceScene& sc = ctx->scene;
  if (!sc.bluenoise_2d || !sc.lut_conductor || !sc.lut_glossy || !sc.lut_dielectric || !sc.lut_dielectric_inv) { ctx->error = "lumc_bounce_probe_host: the scene has no energy tables"; return 1; }
  const size_t n = (size_t) num_vertices * samples;
  if (n > (1u << 24)) { ctx->error = "lumc_bounce_probe_host: more than 2^24 threads"; return 1; }
  return run_probe(ctx, {{vertices, (size_t) num_vertices * kLightProbeVertexWords}}, {{out, n * kBounceProbeWordsPerThread}}, 0, [&](const uint32_t* d_v, uint32_t* d_out) {
    probes_of(ctx)->bounce_probe(nullptr, sc, num_vertices, samples, first_sample, d_v, d_out);
  });
}

// sky_get_color or sky_trace_inscattering (dev_sky.h) on caller-made rays in the active flavour, with the march's stages: out holds LUMC_SKY_PROBE_WORDS words per
// ray, zero where a stage was not reached (k_sky_probe, kernels_probe.h). The scene is in sky mode DEFAULT or HDRI with the two tables on the device, and has no active clouds.
int lumc_sky_probe_host(LumContext* ctx, uint32_t num_rays, const uint32_t* rays, uint32_t* out) {
  static_assert(LUMC_SKY_PROBE_WORDS == kSkyProbeWordsPerThread && LUMC_SKY_PROBE_RAY_WORDS == kSkyProbeRayWords, "lum_core.h and probe_layout.h");
  static_assert(LUMC_SKY_PROBE_WORDS == LUMC_SKY_PROBE_HEAD_WORDS + LUMC_SKY_PROBE_MAX_STEPS * LUMC_SKY_PROBE_STEP_WORDS, "lum_core.h");
  if (!ctx || !ctx->has_scene) { if (ctx) ctx->error = "lumc_sky_probe_host: no scene"; return 1; }
  if (num_rays == 0) return 0;
  if (!rays || !out) { ctx->error = "lumc_sky_probe_host: null argument"; return 1; }
  const DeviceScene& sc = ctx->scene;
  if (!sc.sky_lut_transmittance || !sc.sky_lut_multiscattering) { ctx->error = "lumc_sky_probe_host: the scene has no sky tables"; return 1; }
  if (sc.cloud_active) { ctx->error = "lumc_sky_probe_host: the probe marches without cloud shadows"; return 1; }
  if (num_rays > (1u << 20)) { ctx->error = "lumc_sky_probe_host: more than 2^20 rays"; return 1; }
  return run_probe(ctx, {{rays, (size_t) num_rays * kSkyProbeRayWords}}, {{out, (size_t) num_rays * kSkyProbeWordsPerThread}}, 0, [&](const uint32_t* d_r, uint32_t* d_out) {
    probes_of(ctx)->sky_probe(nullptr, sc, num_rays, d_r, d_out);
  });
}

// sample_sun (dev_sky.h) on the light probe's caller-made vertices in the active flavour, with its stages: LUMC_SUN_PROBE_WORDS words per (vertex, sample id), zero where
// a stage was not reached (k_sun_probe, kernels_probe.h). The scene has the sky and the energy tables and no active clouds.
int lumc_sun_probe_host(LumContext* ctx, uint32_t num_vertices, const uint32_t* vertices, uint32_t first_sample, uint32_t samples, uint32_t* out) {
  static_assert(LUMC_SUN_PROBE_WORDS == kSunProbeWordsPerThread, "lum_core.h and probe_layout.h");
  if (!ctx || !ctx->has_scene) { if (ctx) ctx->error = "lumc_sun_probe_host: no scene"; return 1; }
  if (num_vertices == 0 || samples == 0) return 0;
  if (!vertices || !out) { ctx->error = "lumc_sun_probe_host: null argument"; return 1; }
  const DeviceScene& sc = ctx->scene;
  if (!sc.bluenoise_2d || !sc.lut_conductor || !sc.lut_glossy || !sc.lut_dielectric || !sc.lut_dielectric_inv) { ctx->error = "lumc_sun_probe_host: the scene has no energy tables"; return 1; }
  if (!sc.sky_lut_transmittance) { ctx->error = "lumc_sun_probe_host: the scene has no sky tables"; return 1; }
  if (sc.cloud_active) { ctx->error = "lumc_sun_probe_host: the probe's scene has no clouds"; return 1; }
  const size_t n = (size_t) num_vertices * samples;
  if (n > (1u << 22)) { ctx->error = "lumc_sun_probe_host: more than 2^22 threads"; return 1; }
  return run_probe(ctx, {{vertices, (size_t) num_vertices * kLightProbeVertexWords}}, {{out, n * kSunProbeWordsPerThread}}, 0, [&](const uint32_t* d_v, uint32_t* d_out) {
    probes_of(ctx)->sun_probe(nullptr, sc, num_vertices, samples, first_sample, d_v, d_out);
  });
}

// The hardware's v_exp_f32 (op 0), v_sin_f32 (1) and v_cos_f32 (2) on caller-made arguments (k_sky_math_probe): what the fast flavour's exp2_det and sincos_det issue,
// so the fast unit's kernel whatever the context's flavour.
int lumc_sky_math_probe_host(LumContext* ctx, uint32_t op, uint32_t count, const float* x, float* y) {
  if (!ctx) return 1;
  if (count == 0) return 0;
  if (!x || !y || op > 2u) { ctx->error = "lumc_sky_math_probe_host: bad argument"; return 1; }
  return run_probe(ctx, {{x, count}}, {{y, count}}, 0, [&](const uint32_t* d_x, uint32_t* d_y) {
    wavefront_probes_fast()->sky_math_probe(nullptr, count, op, reinterpret_cast<const float*>(d_x), reinterpret_cast<float*>(d_y));
  });
}

}  // extern "C"
