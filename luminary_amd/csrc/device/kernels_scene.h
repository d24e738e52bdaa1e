// The scene's kernels: what produces data both flavours must agree on while a scene is uploaded or updated - cloud noise, the sky's and the BSDFs' look-up
// tables, the panorama bake, the per-triangle and per-light records. Flavour-neutral like those of kernels_shared.h: they exist once, in the exact inline
// namespace, and are launched directly by csrc/host/scene_device.hip - the only unit that includes this header, compiled with the exact flavour's flags.
// That unit has its own copy of the sampler's seed table (dev_sampler.h), filled by lumc_context_create through scene_device_init.
#pragma once

#include "dev_sky.h"
#include "dev_cloud_march.h"
#include "dev_wave.h"  // kBlock

LUM_NS_BEGIN

// ---- the clouds' noise textures (cuda/cloud_noise.cuh; the noise functions: dev_cloud.h) ----
__global__ void k_cloud_noise_shape(uint32_t* dst, uint32_t dim) {
  const uint32_t amount = dim * dim * dim;
  const float sc = 1.0f / dim;
  for (uint32_t id = blockIdx.x * blockDim.x + threadIdx.x; id < amount; id += gridDim.x * blockDim.x) {
    const uint32_t z = id / (dim * dim), y = (id - z * (dim * dim)) / dim, x = id - y * dim - z * dim * dim;
    const V3 s = v3(x * sc, y * sc, z * sc);
    const float size_scale = 1.0f;
    float perlin_dilate = perlin_octaves(s, 4.0f * size_scale, 7, true);
    float worley_dilate = worley_octaves(s, 6.0f * size_scale, 3, 0.0f, 0.3f);
    float worley_large = worley_octaves(s, 6.0f * size_scale, 3, 0.0f, 0.3f);
    float worley_medium = worley_octaves(s, 12.0f * size_scale, 3, 0.0f, 0.3f);
    float worley_small = worley_octaves(s, 24.0f * size_scale, 3, 0.0f, 0.3f);
    perlin_dilate = c_remap01(perlin_dilate, 0.3f, 1.4f);
    worley_dilate = c_remap01(worley_dilate, -0.3f, 1.3f);
    worley_large = c_remap01(worley_large, -0.4f, 1.0f);
    worley_medium = c_remap01(worley_medium, -0.4f, 1.0f);
    worley_small = c_remap01(worley_small, -0.4f, 1.0f);
    const float perlin_worley = dilate_perlin_worley(perlin_dilate, worley_dilate, 0.3f);
    dst[id] = cloud_pack(saturate(perlin_worley) * 255.0f, saturate(worley_large) * 255.0f, saturate(worley_medium) * 255.0f, saturate(worley_small) * 255.0f);
  }
}
__global__ void k_cloud_noise_detail(uint32_t* dst, uint32_t dim) {
  const uint32_t amount = dim * dim * dim;
  const float sc = 1.0f / dim;
  for (uint32_t id = blockIdx.x * blockDim.x + threadIdx.x; id < amount; id += gridDim.x * blockDim.x) {
    const uint32_t z = id / (dim * dim), y = (id - z * (dim * dim)) / dim, x = id - y * dim - z * dim * dim;
    const V3 s = v3(x * sc, y * sc, z * sc);
    const float size_scale = 0.5f;
    float worley_large = worley_octaves(s, 10.0f * size_scale, 3, 0.0f, 0.3f);
    float worley_medium = worley_octaves(s, 15.0f * size_scale, 3, 0.0f, 0.3f);
    float worley_small = worley_octaves(s, 20.0f * size_scale, 3, 0.0f, 0.3f);
    worley_large = c_remap01(worley_large, -1.0f, 1.0f);
    worley_medium = c_remap01(worley_medium, -1.0f, 1.0f);
    worley_small = c_remap01(worley_small, -1.0f, 1.0f);
    dst[id] = cloud_pack(saturate(worley_large) * 255.0f, saturate(worley_medium) * 255.0f, saturate(worley_small) * 255.0f, 255.0f);
  }
}
__global__ void k_cloud_noise_weather(uint32_t* dst, uint32_t dim, float seed) {
  const uint32_t amount = dim * dim;
  const float sc = 1.0f / dim;
  for (uint32_t id = blockIdx.x * blockDim.x + threadIdx.x; id < amount; id += gridDim.x * blockDim.x) {
    const uint32_t y = id / dim, x = id - y * dim;
    const float sx = x * sc, sy = y * sc;
    const float size_scale = 3.0f, coverage_perlin_worley_diff = 0.4f, remap_low = 0.5f, remap_high = 1.3f;
    float perlin1 = perlin_octaves(v3(sx, sy, 0.0f), 2.0f * size_scale, 7, true);
    float worley1 = worley_octaves(v3(sx, sy, 0.0f), 3.0f * size_scale, 2, seed, 0.25f);
    float perlin2 = perlin_octaves(v3(sx, sy, 500.0f), 4.0f * size_scale, 7, true);
    float perlin3 = perlin_octaves(v3(sx, sy, 100.0f), 2.0f * size_scale, 7, true);
    float perlin4 = perlin_octaves(v3(sx, sy, 200.0f), 3.0f * size_scale, 7, true);
    perlin1 = c_remap01(perlin1, remap_low, remap_high);
    worley1 = c_remap01(worley1, remap_low, remap_high);
    perlin2 = c_remap01(perlin2, remap_low, remap_high);
    perlin3 = c_remap01(perlin3, remap_low, remap_high);
    perlin4 = c_remap01(perlin4, remap_low, remap_high);
    perlin1 = pow_det(perlin1, 1.0f);
    worley1 = pow_det(worley1, 0.75f);
    perlin2 = pow_det(perlin2, 2.0f);
    perlin3 = pow_det(perlin3, 3.0f);
    perlin4 = pow_det(perlin4, 1.0f);
    perlin1 = saturate(perlin1 * 1.2f) * 0.4f + 0.1f;
    worley1 = saturate(1.0f - worley1 * 2.0f);
    perlin2 = saturate(perlin2) * 0.5f;
    perlin3 = saturate(1.0f - perlin3 * 3.0f);
    perlin4 = saturate(1.0f - perlin4 * 1.5f);
    perlin4 = dilate_perlin_worley(worley1, perlin4, coverage_perlin_worley_diff);
    perlin1 -= perlin4;
    perlin2 -= perlin4 * perlin4;
    perlin1 = c_remap01(2.0f * perlin1, 0.05f, 1.0f);
    dst[id] = cloud_pack(saturate(perlin1) * 255.0f, saturate(perlin2) * 255.0f, saturate(perlin3) * 255.0f, saturate(perlin4) * 255.0f);
  }
}

// ---- the sky's transmittance and multiscattering LUTs (their integrals: dev_sky.h) ----
__global__ __launch_bounds__(64) void k_sky_transmittance_lut(DeviceScene sc, float4* __restrict__ dst) {
  const int id = blockIdx.x * 64 + threadIdx.x;
  if (id >= kSkyTmWidth * kSkyTmHeight) return;
  const SkyView s = sky_view(sc);
  const int y = id / kSkyTmWidth, x = id - y * kSkyTmWidth;
  float fx = ((float) x + 0.5f) / kSkyTmWidth, fy = ((float) y + 0.5f) / kSkyTmHeight;
  fx = sky_sub_to_unit_uv(fx, kSkyTmWidth); fy = sky_sub_to_unit_uv(fy, kSkyTmHeight);
  const float H = sqrtf(kSkyAtmoRadius * kSkyAtmoRadius - kSkyEarthRadius * kSkyEarthRadius);
  const float rho = H * fy;
  const float r = sqrtf(rho * rho + kSkyEarthRadius * kSkyEarthRadius);
  const float d_min = kSkyAtmoRadius - r, d_max = rho + H;
  const float d = d_min + fx * (d_max - d_min);
  float mu = (d == 0.0f) ? 1.0f : (H * H - rho * rho - d * d) / (2.0f * r * d);
  mu = fminf(1.0f, fmaxf(-1.0f, mu));
  const Spectrum t = sp_exp(sp_scale(sky_optical_depth(s, r, mu), -1.0f));
  dst[id] = make_float4(t.v[0], t.v[1], t.v[2], t.v[3]);
  dst[kSkyTmWidth * kSkyTmHeight + id] = make_float4(t.v[4], t.v[5], t.v[6], t.v[7]);
}

// sky_compute_multiscattering_lut, sky.cuh:276-332: one workgroup of 256 directions per texel, shared-memory tree reduction
__global__ __launch_bounds__(256) void k_sky_multiscattering_lut(DeviceScene sc, float4* __restrict__ dst) {
  __shared__ Spectrum lum_shared[kSkyMsIter], ms_shared[kSkyMsIter];
  const SkyView s = sky_view(sc);
  const int x = blockIdx.x, y = blockIdx.y;
  float fx = ((float) x + 0.5f) / kSkyMsSize, fy = ((float) y + 0.5f) / kSkyMsSize;
  fx = sky_sub_to_unit_uv(fx, kSkyMsSize); fy = sky_sub_to_unit_uv(fy, kSkyMsSize);
  const float cos_angle = fx * 2.0f - 1.0f;
  const V3 sun_dir = v3(0.0f, cos_angle, sqrtf(saturate(1.0f - cos_angle * cos_angle)));
  const float height = kSkyEarthRadius + saturate(fy + kSkyHeightOffset) * (kSkyAtmoHeight - kSkyHeightOffset);
  const V3 pos = v3(0.0f, height, 0.0f), sun_pos = sun_dir * kSkySunDistance;
  const float sqrt_sample = (float) kSkyMsBase;
  const float a = (float) (threadIdx.x / kSkyMsBase), b = (float) (threadIdx.x - (threadIdx.x / kSkyMsBase) * kSkyMsBase);
  const V3 ray = sample_ray_sphere(2.0f * (a / sqrt_sample) - 1.0f, b / sqrt_sample);
  const SkyMsResult r = sky_multiscattering_integration(s, pos, ray, sun_pos);
  lum_shared[threadIdx.x] = r.L; ms_shared[threadIdx.x] = r.ms_as_1;
  for (int i = kSkyMsIter >> 1; i > 0; i >>= 1) {
    __syncthreads();
    if ((int) threadIdx.x < i) {
      lum_shared[threadIdx.x] = sp_add(lum_shared[threadIdx.x], lum_shared[threadIdx.x + i]);
      ms_shared[threadIdx.x] = sp_add(ms_shared[threadIdx.x], ms_shared[threadIdx.x + i]);
    }
  }
  if (threadIdx.x > 0) return;
  const Spectrum luminance = sp_scale(lum_shared[0], 1.0f / (sqrt_sample * sqrt_sample));
  const Spectrum multiscattering = sp_scale(ms_shared[0], 1.0f / (sqrt_sample * sqrt_sample));
  const Spectrum contribution = sp_inv(sp_sub(sp_set1(1.0f), multiscattering));
  const Spectrum L = sp_scale(sp_mul(luminance, contribution), s.multiscattering_factor);
  const int id = x + y * kSkyMsSize;
  dst[id] = make_float4(L.v[0], L.v[1], L.v[2], L.v[3]);
  dst[kSkyMsSize * kSkyMsSize + id] = make_float4(L.v[4], L.v[5], L.v[6], L.v[7]);
}

// ---- scene upload: per-triangle opacity word, per-light record ----
// The material word of the traversal triangles (dev_scene.h): the albedo texture's id, or - untextured - whether a visibility ray cannot pass
// (kBvhTriOpaque: the decision of optix_anyhit.cuh:49-139 for alpha 1), taken once per triangle with the kernels' own material decoding; run at
// scene upload and again after a material edit.
__global__ __launch_bounds__(kBlock) void k_tri_opacity(DeviceScene sc, BvhTri* tris, uint32_t count) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= count) return;
  const uint32_t material = sc.tri_tex[tris[i].scene_index].w & 0xFFFFu;
  uint32_t word = kBvhTriNoTexture;
  if (material < sc.num_materials) {
    const Material m = load_material(sc, material);
    word = (m.albedo_tex != kTextureNone) ? m.albedo_tex : ((m.alpha == 1.0f) ? kBvhTriOpaque : kBvhTriNoTexture);  // textured: the texel decides
  }
  tris[i].albedo_tex = word;
}

// The emissive triangles in world space, one record per light id (load_tri_light_table, dev_light.h): light_triangle_init's result
// (light_triangle.cuh:37-72) evaluated once per light at scene upload instead of once per candidate and vertex.
__global__ __launch_bounds__(kBlock) void k_light_table(DeviceScene sc, float4* table) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= sc.num_lights) return;
  const uint2 handle = sc.light_tri_handles[i];
  const TriLight t = load_tri_light(sc, handle.x, handle.y);
  const Material m = load_material(sc, t.material_id);
  const bool textured = m.luminance_tex != kTextureNone || m.albedo_tex != kTextureNone;
  const Col color = textured ? splat(0.0f) : tri_light_color(sc, t, F2{0.0f, 0.0f});  // without textures the colour does not depend on the point
  table[4u * i] = make_float4(t.vertex.x, t.vertex.y, t.vertex.z, bitsf(t.material_id | (t.bidirectional ? 0x10000u : 0u)));
  table[4u * i + 1u] = make_float4(t.edge1.x, t.edge1.y, t.edge1.z, bitsf(t.scene_tri));
  table[4u * i + 2u] = make_float4(t.edge2.x, t.edge2.y, t.edge2.z, tri_light_area(t));
  table[4u * i + 3u] = make_float4(color.r, color.g, color.b, bitsf(textured ? 1u : 0u));
}

// ---- HDRI bake (cuda/sky_hdri.cuh:13-160, device/device_sky.c:283-316): the sky without celestial bodies - and with the clouds, when active - seen from
// `origin`, as an equirectangular dim x dim image. 32 lanes per texel share its samples; their means go through the reference's trimmed mean. ----
__global__ __launch_bounds__(256) void k_sky_hdri(DeviceScene sc, float ox, float oy, float oz, uint32_t dim, uint32_t sample_count, float4* __restrict__ dst) {
  __shared__ float values[256];
  const uint32_t pixel = (blockIdx.x * 256u + threadIdx.x) >> 5, lane = threadIdx.x & 31u;
  const bool in_range = pixel < dim * dim;
  const uint32_t y = in_range ? pixel / dim : 0u, x = in_range ? pixel - y * dim : 0u;
  const SkyView sky = sky_view(sc);
  const float step_size = 1.0f / (float) (dim - 1u);
  Col color = splat(0.0f);
  float alpha = 0.0f;
  uint32_t num_samples = 0;
  const bool clouds = sc.cloud_active && sc.cloud_noise_shape != nullptr;
  if (in_range) {
    for (uint32_t sample_id = lane; sample_id < sample_count; sample_id += 32u) {
      const Sampler smp{sc.bluenoise_2d, x, y, sample_id, 0};
      const F2 jitter = smp.next2(kRndCameraJitter);
      const float u = ((float) x + jitter.x) * step_size, v = 1.0f - ((float) y + jitter.y) * step_size;
      const float altitude = kPi * v - 0.5f * kPi, azimuth = 2.0f * kPi * u - kPi;
      const V3 ray = angles_to_direction(altitude, azimuth);
      Col sky_color = splat(0.0f), transmittance = splat(1.0f);
      float cloud_transmittance = 1.0f;
      V3 sky_origin = world_to_sky(sky, v3(ox, oy, oz));
      if (clouds) {  // sky_hdri.cuh:88-92: the clouds in front, the sky behind them dimmed by their transmittance
        const float offset = clouds_render(sc, sky, smp, sky_origin, ray, kFltMax, sky_color, transmittance, cloud_transmittance);
        sky_origin = sky_origin + ray * offset;
      }
      const Col behind = sky_get_color(sc, sky, sky_origin, ray, kFltMax, false, (int) sky.steps, smp.next1(kRndSkyStepOffset));
      sky_color = sky_color + behind * transmittance;
      color = color + sky_color;
      alpha += cloud_transmittance;
      num_samples++;
    }
  }
  const uint32_t buckets = min(32u, sample_count);
  float* group = values + (threadIdx.x & ~31u);
  float out[4];
  const float mean[4] = {num_samples ? color.r / (float) num_samples : 0.0f, num_samples ? color.g / (float) num_samples : 0.0f, num_samples ? color.b / (float) num_samples : 0.0f,
                         num_samples ? alpha / (float) num_samples : 0.0f};
#pragma unroll
  for (int ch = 0; ch < 4; ch++) {
    __syncthreads();
    values[threadIdx.x] = mean[ch];
    __syncthreads();
    out[ch] = (lane == 0u && in_range) ? sky_hdri_median_of_means(group, buckets) : 0.0f;
  }
  if (lane == 0u && in_range) dst[x + y * dim] = make_float4(out[0], out[1], out[2], out[3]);  // .w: the clouds' own transmittance (the reference's separate shadow texture), 1 without clouds
}

// ---- BSDF energy LUTs (cuda/bsdf_lut.cuh:20-211): pixel (0,0), depth 0, sample id = iteration ----
LUM_DEV uint16_t quantise_energy(float sum) { return (uint16_t) (1 + (uint16_t) (ceilf(saturate(sum) * 0xFFFE))); }

__global__ void k_generate_lut(const uint32_t* bluenoise, int table, uint32_t count, const uint16_t* conductor, uint16_t* dst) {
  const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= count) return;
  uint32_t x, y, z = 0;
  if (table < 2) { y = id / 32; x = id - y * 32; }
  else { z = id / 1024; y = (id - z * 1024) / 32; x = id - y * 32 - z * 1024; }
  const float NdotV = fmaxf(32.0f * kEps, x * (1.0f / 31));
  const float roughness = y * (1.0f / 31);
  const V3 V = normalize(v3(0.0f, sqrtf(1.0f - NdotV * NdotV), NdotV));
  Sampler smp{bluenoise, 0, 0, 0, 0};
  float sum = 0.0f;
  if (table < 2) {
    const Col f0 = col(0.04f, 0.04f, 0.04f);
    for (uint32_t i = 0; i < 0x10000u; i++) {
      smp.sample_id = i;
      const V3 H = sample_vndf_bounded(V, roughness, smp.next2(kRndBsdfReflection));
      const V3 R = reflect(V, H);
      if (R.z > 0.0f) {
        float v = eval_microfacet_over_vndf(V, roughness, R.z, NdotV);
        if (table == 1) v = v * luminance(fresnel_schlick(f0, shadowed_f90(f0), fabsf(dot(H, V))));
        sum += v;
      }
    }
    sum /= 0x10000u;
    if (table == 1) sum /= conductor[id] * (1.0f / 0xFFFF);
  }
  else {
    const float ior_base = 1.0f + z * (1.0f / 31) * 2.0f;
    const float ior = (table == 2) ? 1.0f / ior_base : ior_base;
    for (uint32_t i = 0; i < 0x10000u; i++) {
      smp.sample_id = i;
      bool tot;
      V3 H = sample_vndf_bounded(V, roughness, smp.next2(kRndBsdfReflection));
      const V3 R = reflect(V, H);
      V3 T = refract(V, H, ior, tot);
      float fres = tot ? 1.0f : fresnel_dielectric(H, V, T, ior);
      if (R.z > 0.0f) sum += eval_microfacet_over_vndf(V, roughness, R.z, NdotV) * fres;
      H = sample_vndf_caps(V, roughness, smp.next2(kRndBsdfRefraction));
      T = refract(V, H, ior, tot);
      fres = tot ? ((table == 2) ? 1.0f : 0.0f) : fresnel_dielectric(H, V, T, ior);
      const float NdotR = -T.z;
      if (NdotR > 0.0f) sum += ggx_g2_over_g1(pow4(roughness), NdotR, NdotV) * (1.0f - fres);
    }
    sum /= 0x10000u;
  }
  dst[id] = quantise_energy(sum);
}

LUM_NS_END
