// The flavour-neutral kernels: what produces data both flavours must agree on (BSDF / sky tables, cloud noise, panorama bake, the scene upload's
// per-triangle and per-light records), bookkeeping (accumulation, adaptive rates), the display chain and the helpers of the plain-array entry points.
// They exist once, in the exact inline namespace, and are launched directly by csrc/host/core.hip - the only unit that includes this header, compiled
// with the exact flavour's flags. The wavefront kernels (kernels.h) are not included: they belong to wavefront_exact.hip / wavefront_fast.hip.
// This unit has its own copy of the sampler's seed table (dev_sampler.h), filled by lumc_context_create.
#pragma once

#include "dev_sky.h"
#include "dev_volume.h"
#include "dev_cloud_march.h"
#include "dev_camera.h"
#include "dev_wave.h"  // kBlock
#include "dev_output.h"
#include "dev_adaptive.h"

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

// ---- the display chain (its per-pixel functions: dev_output.h) ----
// generate_final_image, kernels.cuh:503-556 (with accumulation_generate_result's division by the sample count folded in): planar input
// image of (src >> stage) pixels -> planar display-referred RGB of (src >> max(stage, supersampling)) pixels; every output pixel is the
// mean of the output_scale^2 tone-mapped input pixels below it, summed row by row.
__global__ __launch_bounds__(256) void k_final_image(OutputParams p, const float* __restrict__ input, float* __restrict__ frame_output) {
  const uint32_t ui = p.undersampling_stage, uo = max(ui, p.supersampling);
  const uint32_t output_scale = 1u << (uo - ui);
  const uint32_t out_w = p.src_width >> uo, out_h = p.src_height >> uo, in_w = p.src_width >> ui, in_h = p.src_height >> ui;
  const uint32_t n = out_w * out_h, n_in = in_w * in_h;
  const float norm = 1.0f / (output_scale * output_scale);
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const uint32_t y = i / out_w, x = i - y * out_w;
    const uint32_t source_x = x * output_scale, source_y = y * output_scale;
    Col color = splat(0.0f);
    for (uint32_t yi = 0; yi < output_scale; yi++) {
      for (uint32_t xi = 0; xi < output_scale; xi++) {
        const uint32_t px_x = min(source_x + xi, in_w - 1), px_y = min(source_y + yi, in_h - 1);
        const uint32_t index = px_x + px_y * in_w;
        Col px = col(input[index] * p.inv_sample_count, input[n_in + index] * p.inv_sample_count, input[2 * n_in + index] * p.inv_sample_count);
        color = color + display_transform(p, px, px_x, px_y);
      }
    }
    color = color * norm;
    frame_output[i] = color.r; frame_output[n + i] = color.g; frame_output[2 * n + i] = color.b;
  }
}

// accumulation_generate_result_undersampling, accumulation.cuh:192-254: while the first sample is rendered coarse to fine, block (x, y) of
// 2^stage pixels shows the mean of the 4 - iteration pixels of it that exist so far (pattern of kernels.cuh:20-45). Output: compact
// planar image of (width >> stage) x (height >> stage).
__global__ __launch_bounds__(256) void k_result_undersampled(const float* __restrict__ first_moment, uint32_t width, uint32_t height, uint32_t stage, uint32_t iteration,
                                                             float* __restrict__ result) {
  const uint32_t scale = 1u << stage, w = width >> stage, h = height >> stage, n = w * h, frame = width * height;
  const float color_scale = 1.0f / (4 - iteration);
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const uint32_t dst_y = i / w, dst_x = i - dst_y * w;
    const uint32_t base_x = dst_x << stage, base_y = dst_y << stage;
    Col sum = splat(0.0f);
    for (uint32_t id = iteration; id < 4; id++) {
      const uint32_t px = min(base_x + ((id & 1u) ? 0u : scale >> 1), width - 1), py = min(base_y + ((id & 2u) ? 0u : scale >> 1), height - 1);
      const uint32_t index = px + py * width;
      sum = sum + col(first_moment[index], first_moment[frame + index], first_moment[2 * frame + index]);
    }
    sum = sum * color_scale;
    result[i] = sum.r; result[n + i] = sum.g; result[2 * n + i] = sum.b;
  }
}

__global__ __launch_bounds__(256) void k_post_downsample(const float* __restrict__ src, uint32_t sw, uint32_t sh, float* __restrict__ dst, uint32_t tw, uint32_t th) {
  const float scale_x = 1.0f / (tw - 1), scale_y = 1.0f / (th - 1), step_x = 1.0f / (sw - 1), step_y = 1.0f / (sh - 1);
  const uint32_t n = tw * th;
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const uint32_t y = i / tw, x = i - y * tw;
    const float sx = scale_x * x, sy = scale_y * y;
    float p = 0.0f;
    p += sample_plane_border(src, sx - 0.5f * step_x, sy - 0.5f * step_y, sw, sh, 1.0f);
    p += sample_plane_border(src, sx + 0.5f * step_x, sy - 0.5f * step_y, sw, sh, 1.0f);
    p += sample_plane_border(src, sx - 0.5f * step_x, sy + 0.5f * step_y, sw, sh, 1.0f);
    p += sample_plane_border(src, sx + 0.5f * step_x, sy + 0.5f * step_y, sw, sh, 1.0f);
    p += sample_plane_border(src, sx, sy, sw, sh, 1.0f);
    p += sample_plane_border(src, sx, sy - step_y, sw, sh, 0.5f);
    p += sample_plane_border(src, sx - step_x, sy, sw, sh, 0.5f);
    p += sample_plane_border(src, sx + step_x, sy, sw, sh, 0.5f);
    p += sample_plane_border(src, sx, sy + step_y, sw, sh, 0.5f);
    p += sample_plane_border(src, sx - step_x, sy - step_y, sw, sh, 0.25f);
    p += sample_plane_border(src, sx + step_x, sy - step_y, sw, sh, 0.25f);
    p += sample_plane_border(src, sx - step_x, sy + step_y, sw, sh, 0.25f);
    p += sample_plane_border(src, sx + step_x, sy + step_y, sw, sh, 0.25f);
    p *= 1.0f / 8.0f;
    dst[i] = fmaxf(p, 0.0f);  // threshold 0 (device_post.c:82)
  }
}

// dst may be the base image (every thread reads only its own base pixel)
__global__ __launch_bounds__(256) void k_post_upsample(const float* __restrict__ src, uint32_t sw, uint32_t sh, float* dst, uint32_t tw, uint32_t th, float sa, float sb) {
  const float scale_x = 1.0f / (tw - 1), scale_y = 1.0f / (th - 1), step_x = 1.0f / (sw - 1), step_y = 1.0f / (sh - 1);
  const uint32_t n = tw * th;
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const uint32_t y = i / tw, x = i - y * tw;
    const float sx = scale_x * x, sy = scale_y * y;
    float p = sample_plane_border(src, sx - step_x, sy - step_y, sw, sh, 1.0f);
    p += sample_plane_border(src, sx, sy - step_y, sw, sh, 2.0f);
    p += sample_plane_border(src, sx + step_x, sy - step_y, sw, sh, 1.0f);
    p += sample_plane_border(src, sx - step_x, sy, sw, sh, 2.0f);
    p += sample_plane_border(src, sx, sy, sw, sh, 4.0f);
    p += sample_plane_border(src, sx + step_x, sy, sw, sh, 2.0f);
    p += sample_plane_border(src, sx - step_x, sy + step_y, sw, sh, 1.0f);
    p += sample_plane_border(src, sx, sy + step_y, sw, sh, 2.0f);
    p += sample_plane_border(src, sx + step_x, sy + step_y, sw, sh, 1.0f);
    p *= 1.0f / 20.0f;
    p *= sa;
    float base = dst[i];
    base *= sb;
    dst[i] = p + base;
  }
}

// convert_RGBF_to_ARGB8, kernels.cuh:558-644 (bytes b, g, r, a)
__global__ __launch_bounds__(256) void k_to_argb8(OutputParams p, const float* __restrict__ frame_output, const uint16_t* __restrict__ bluenoise_1d,
                                                  uint32_t* __restrict__ dst) {
  const uint32_t uo = max(p.undersampling_stage, p.supersampling), um = uo - p.supersampling;
  const uint32_t nominal_w = p.src_width >> p.supersampling, nominal_h = p.src_height >> p.supersampling;  // the size the frame is rendered for
  const uint32_t mem_w = p.src_width >> uo, mem_h = p.src_height >> uo, ns = mem_w * mem_h;                // the image in memory
  const uint32_t n = p.dst_width * p.dst_height;
  const float scale_x = 1.0f / (p.dst_width - 1), scale_y = 1.0f / (p.dst_height - 1);
  const float mem_scale = 1.0f / (1u << um);
  const bool scaled = p.dst_width != nominal_w || p.dst_height != nominal_h;
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const uint32_t y = i / p.dst_width, x = i - y * p.dst_width;
    Col px;
    if (scaled) {
      const float sx = x * scale_x, sy = y * scale_y;
      px = col(sample_plane(frame_output, sx, sy, nominal_w, nominal_h, mem_scale, ns - 1), sample_plane(frame_output + ns, sx, sy, nominal_w, nominal_h, mem_scale, ns - 1),
               sample_plane(frame_output + 2 * ns, sx, sy, nominal_w, nominal_h, mem_scale, ns - 1));
    }
    else {
      const uint32_t src = min(x >> um, mem_w - 1) + min(y >> um, mem_h - 1) * mem_w;  // the edge repeats where the reference reads past the coarse image
      px = col(frame_output[src], frame_output[ns + src], frame_output[2 * ns + src]);
    }
    px = apply_filter(p, bluenoise_1d, px, x, y);
    const float dither = p.dithering ? dither_mask(bluenoise_1d, x, y) : 0.5f;
    const float r = fmaxf(0.0f, fminf(255.9999f, dither + 255.0f * linear_to_srgb(px.r)));
    const float g = fmaxf(0.0f, fminf(255.9999f, dither + 255.0f * linear_to_srgb(px.g)));
    const float b = fmaxf(0.0f, fminf(255.9999f, dither + 255.0f * linear_to_srgb(px.b)));
    dst[i] = 0xFF000000u | (f2u_sat(r) << 16) | (f2u_sat(g) << 8) | f2u_sat(b);
  }
}

// ---- adaptive sampling: block variance, stage rates, accumulation, the result image (bookkeeping: dev_adaptive.h) ----
// adaptive_sampling_block_reduce_variance (adaptive_sampling.cuh:168-199): 16 lanes per block, four blocks per wave.
__global__ __launch_bounds__(256) void k_adaptive_block_variance(AdaptiveView a, OutputParams op, uint32_t width, uint32_t height, float exposure,
                                                                const float* __restrict__ fm, const float* __restrict__ sm, float* __restrict__ block_variance) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  const uint32_t block = t >> 4;
  float variance = 0.0f;
  if (block < a.num_blocks) {
    const uint32_t by = block / a.blocks_x, bx = block - by * a.blocks_x;
    const uint32_t x = (bx << kAdaptiveBlockLog) + (t & 3u), y = (by << kAdaptiveBlockLog) + ((t >> 2) & 3u);
    if (x < width && y < height) {
      const uint32_t n = adaptive_pixel_samples(a, a.stage_counts[block]);
      const float inv_n = 1.0f / (float) n;
      Col mean;
      variance = adaptive_pixel_variance(fm, sm, width * height, x + y * width, inv_n, mean);
      if (exposure != 0.0f) {
        const float c = adaptive_tonemap_compression(op, mean, exposure);
        variance *= c * c;
      }
    }
  }
#pragma unroll
  for (int off = 8; off > 0; off >>= 1) variance = fmaxf(variance, __shfl_xor(variance, off, 16));
  if ((t & 15u) == 0u && block < a.num_blocks) block_variance[block] = fabsf(variance);
}

// Total of the block variances in a fixed order (see the header): one thread per chunk, then one thread over the chunk sums.
__global__ __launch_bounds__(64) void k_adaptive_sum_chunks(const float* __restrict__ block_variance, uint32_t num_blocks, float* __restrict__ partial) {
  const uint32_t c = blockIdx.x * 64u + threadIdx.x;
  const uint32_t first = c * kAdaptiveSumChunk;
  if (first >= num_blocks) return;
  const uint32_t last = min(first + kAdaptiveSumChunk, num_blocks);
  float s = 0.0f;
  for (uint32_t i = first; i < last; i++) s += block_variance[i];
  partial[c] = s;
}

__global__ void k_adaptive_sum_total(const float* __restrict__ partial, uint32_t num_chunks, float* __restrict__ total) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  float s = 0.0f;
  for (uint32_t i = 0; i < num_chunks; i++) s += partial[i];
  *total = s;
}

// adaptive_sampling_compute_stage_sample_counts (adaptive_sampling.cuh:201-221): the rate of the stage after `current_stage`.
// Also writes the tasks of that stage per block (16 pixels x rate) for the prefix sum.
__global__ __launch_bounds__(256) void k_adaptive_stage_counts(const float* __restrict__ block_variance, const float* __restrict__ total, uint32_t num_blocks,
                                                              uint32_t current_stage, uint32_t max_rate, uint32_t avg_rate, uint32_t* __restrict__ stage_counts,
                                                              uint32_t* __restrict__ block_tasks, const uint8_t* __restrict__ block_mask) {
  const uint32_t block = blockIdx.x * 256u + threadIdx.x;
  if (block >= num_blocks) return;
  const float avg_variance = *total / (float) num_blocks;
  const float variance = block_variance[block];
  uint32_t packed = stage_counts[block];
  packed &= (1u << (current_stage * 8u)) - 1u;  // keep the bytes of the stages already run
  // remap(variance, 0, avg_variance, 0, avg_rate), math.cuh:54-56; a NaN (0/0) converts to 0 as on the reference's hardware
  const float mapped = variance / avg_variance * (float) avg_rate;
  uint32_t rate = f2u_sat(mapped + 0.5f);
  rate = max(rate, 1u);
  rate = min(rate, max_rate);
  packed |= (rate - 1u) << (current_stage * 8u);
  stage_counts[block] = packed;
  // image-tile partition over GPUs: every rank knows every block's rate, but only creates tasks for the blocks it owns
  block_tasks[block] = (!block_mask || block_mask[block]) ? rate << (2u * kAdaptiveBlockLog) : 0u;
}

// Tasks per block of a stage-0 execution under a partition (one sample per pixel of the owned blocks).
__global__ __launch_bounds__(256) void k_adaptive_uniform_tasks(const uint8_t* __restrict__ block_mask, uint32_t num_blocks, uint32_t* __restrict__ block_tasks) {
  const uint32_t block = blockIdx.x * 256u + threadIdx.x;
  if (block < num_blocks) block_tasks[block] = block_mask[block] ? 1u << (2u * kAdaptiveBlockLog) : 0u;
}

// accumulation_collect_results for one adaptive execution: a pixel's samples of this execution are added in sample order.
__global__ __launch_bounds__(256) void k_accumulate_adaptive(AdaptiveView a, AdaptivePass pass, uint32_t width, uint32_t height, const float4* __restrict__ results,
                                                            float* first_moment, float* second_moment) {
  const uint32_t num_pixels = width * height;
  const uint32_t pass_pixels = (pass.block_end - pass.block_begin) << (2u * kAdaptiveBlockLog);
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < pass_pixels; i += gridDim.x * 256u) {
    const uint32_t block = pass.block_begin + (i >> (2u * kAdaptiveBlockLog)), local = i & 15u;
    const uint32_t by = block / a.blocks_x, bx = block - by * a.blocks_x;
    const uint32_t x = (bx << kAdaptiveBlockLog) + (local & 3u), y = (by << kAdaptiveBlockLog) + (local >> kAdaptiveBlockLog);
    if (x >= width || y >= height) continue;
    const uint32_t p = x + y * width;
    const uint32_t packed = a.stage_counts[block];
    const uint32_t per_pixel = adaptive_stage_count(packed, a.stage_id) * pass.executions;
    const uint32_t first_id = adaptive_pixel_samples(a, packed);
    const uint32_t block_begin = block ? a.block_task_end[block - 1u] : 0u;
    if (a.block_task_end[block] == block_begin) continue;  // a block of another GPU's tiles: no tasks here
    const uint32_t base = block_begin * pass.executions - pass.task_begin + local * per_pixel;
    float r = first_moment[p], g = first_moment[num_pixels + p], b = first_moment[2 * num_pixels + p];
    float s = second_moment[p];
    for (uint32_t k = 0; k < per_pixel; k++) {
      if (first_id + k >= kMaxGlobalSamples) break;
      const float4 v = results[base + k];
      r += v.x; g += v.y; b += v.z;
      s += luminance(col(v.x * v.x, v.y * v.y, v.z * v.z));
    }
    first_moment[p] = r; first_moment[num_pixels + p] = g; first_moment[2 * num_pixels + p] = b;
    second_moment[p] = s;
  }
}

__global__ __launch_bounds__(256) void k_generate_result(AdaptiveView a, ResultParams rp, OutputParams op, const float* __restrict__ fm, const float* __restrict__ sm,
                                                        float* __restrict__ frame_result) {
  const uint32_t n = rp.width * rp.height;
  for (uint32_t index = blockIdx.x * 256u + threadIdx.x; index < n; index += gridDim.x * 256u) {
    const uint32_t y = index / rp.width, x = index - y * rp.width;
    const uint32_t samples = result_pixel_samples(a, rp, x, y);
    const float normalization = 1.0f / (float) samples;
    Col result;
    switch (rp.mode) {
      default:
      case 0: {
        if (rp.local_error_minimization) {
          Col center_mean;
          const float center_variance = adaptive_pixel_variance(fm, sm, n, index, normalization, center_mean);
          const float center_error = center_variance * normalization;
          const uint32_t xi_start = max(x, 1u) - 1u, xi_end = min(x, rp.width - 1u) + 1u;
          const uint32_t yi_start = max(y, 1u) - 1u, yi_end = min(y, rp.height - 1u) + 1u;
          Col neighbour_mean = splat(0.0f);
          float neighbour_error = 0.0f;
          for (uint32_t yi = yi_start; yi <= yi_end; yi++) {
            for (uint32_t xi = xi_start; xi <= xi_end; xi++) {
              if (xi == x && yi == y) continue;
              Col m = splat(0.0f);
              float variance = 0.0f, norm = 0.0f;
              // the reference's range runs one past the last row/column; pixels outside the frame contribute zero
              // (adaptive_sampling.cuh:146-151) but still count in the divisor below
              const uint32_t ns = (xi < rp.width && yi < rp.height) ? result_pixel_samples(a, rp, xi, yi) : result_pixel_samples(a, rp, min(xi, rp.width - 1u), min(yi, rp.height - 1u));
              norm = 1.0f / (float) ns;
              if (xi < rp.width && yi < rp.height) variance = adaptive_pixel_variance(fm, sm, n, xi + yi * rp.width, norm, m);
              neighbour_mean = neighbour_mean + m;
              neighbour_error += variance * norm;
            }
          }
          const float neighbour_norm = 1.0f / (float) ((xi_end - xi_start + 1u) * (yi_end - yi_start + 1u) - 1u);
          neighbour_mean = neighbour_mean * neighbour_norm;
          neighbour_error *= neighbour_norm;
          const float t = remap01(center_error, 0.0f, 8.0f * neighbour_error);
          result = col(lerpf(center_mean.r, neighbour_mean.r, t), lerpf(center_mean.g, neighbour_mean.g, t), lerpf(center_mean.b, neighbour_mean.b, t));
        }
        else result = col(fm[index] * normalization, fm[n + index] * normalization, fm[2 * n + index] * normalization);
      } break;
      case 1: {
        Col mean;
        result = splat(128.0f * adaptive_pixel_variance(fm, sm, n, index, normalization, mean));
      } break;
      case 2: {
        Col mean;
        const float variance = adaptive_pixel_variance(fm, sm, n, index, normalization, mean);
        const float compression = adaptive_tonemap_compression(op, mean, rp.exposure);
        const float mse = sqrtf(variance * normalization) * compression;
        const float value = 1024.0f * mse;
        result = col(saturate(2.0f * value), saturate(2.0f * (value - 0.5f)),
                     saturate((value > 0.5f) ? 4.0f * (0.25f - fabsf(value - 1.0f)) : 4.0f * (0.25f - fabsf(value - 0.25f))));
      } break;
      case 3: {
        // adaptive_sampling_get_current_tasks_per_pixel (adaptive_sampling.cuh:107-120)
        uint32_t per_pixel = 1;
        if (a.stage_counts && a.stage_id > 0) per_pixel = adaptive_stage_count(a.stage_counts[adaptive_block_of(a, x, y)], a.stage_id);
        result = splat((float) per_pixel / (float) kAdaptiveMaxRate);
      } break;
    }
    frame_result[index] = result.r; frame_result[n + index] = result.g; frame_result[2 * n + index] = result.b;
  }
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

// ---- accumulation (cuda/accumulation.cuh:63-84): samples of a pixel are added in sample order ----
__global__ __launch_bounds__(kBlock) void k_accumulate(const float4* results, uint32_t num_pixels, uint32_t batch, float* first_moment, float* second_moment) {
  for (uint32_t p = blockIdx.x * kBlock + threadIdx.x; p < num_pixels; p += gridDim.x * kBlock) {
    float r = first_moment[p], g = first_moment[num_pixels + p], b = first_moment[2 * num_pixels + p];
    float s = second_moment ? second_moment[p] : 0.0f;
    for (uint32_t k = 0; k < batch; k++) {
      const float4 v = results[k * num_pixels + p];
      r += v.x; g += v.y; b += v.z;
      s += luminance(col(v.x * v.x, v.y * v.y, v.z * v.z));
    }
    first_moment[p] = r; first_moment[num_pixels + p] = g; first_moment[2 * num_pixels + p] = b;
    if (second_moment) second_moment[p] = s;
  }
}

// One sample of a subset of the frame's pixels (an iteration of the undersampling preview, kernels.cuh:47-95): result p belongs to frame
// pixel pixels[p]. accumulation_collect_results, accumulation.cuh:36-61, with one result per pixel.
__global__ __launch_bounds__(kBlock) void k_accumulate_scatter(const float4* results, const uint32_t* pixels, uint32_t count, uint32_t frame_pixels, float* first_moment,
                                                               float* second_moment) {
  for (uint32_t p = blockIdx.x * kBlock + threadIdx.x; p < count; p += gridDim.x * kBlock) {
    const uint32_t index = pixels[p];
    const float4 v = results[p];
    first_moment[index] += v.x; first_moment[frame_pixels + index] += v.y; first_moment[2 * frame_pixels + index] += v.z;
    if (second_moment) second_moment[index] += luminance(col(v.x * v.x, v.y * v.y, v.z * v.z));
  }
}

// ---- standalone visibility entry (lumc_trace_visibility): plain per-ray arrays into a ShadowQueue whose output index is the ray index, and its answers back ----
__global__ __launch_bounds__(256) void k_visibility_pack(uint32_t n, const float* origins, const float* dirs, const float* dist, const uint32_t* ids, ShadowQueue sq) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  sq.origin_dist[i] = make_float4(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2], dist[i]);
  sq.dir_out[i] = make_float4(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], bitsf(i));
  sq.ids[i] = make_uint4(ids[4 * i], ids[4 * i + 1], ids[4 * i + 2], ids[4 * i + 3]);
}
__global__ __launch_bounds__(256) void k_visibility_unpack(uint32_t n, const float4* vis, float* out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const float4 v = vis[i];
  out[3 * i] = v.x; out[3 * i + 1] = v.y; out[3 * i + 2] = v.z;
}

// ---- camera ray of one pixel (first sample id), for pixel queries; valid[0] = 0: the ray did not leave the lens ----
__global__ void k_pixel_ray(DeviceScene sc, DeviceLens lens, int cam, uint32_t x, uint32_t y, uint32_t sample_id, float* origin, float* dir, uint32_t* valid) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const Sampler smp{sc.bluenoise_2d, x, y, sample_id, 0};
  V3 o, d;
  float w = 1.0f;
  if (cam == kCamThinLens) camera_ray(sc, smp, o, d);
  else if (cam == kCamPhysical) w = camera_sample<kCamPhysical>(sc, lens, smp, o, d);
  else w = camera_sample<kCamPhysicalReflections>(sc, lens, smp, o, d);
  origin[0] = o.x; origin[1] = o.y; origin[2] = o.z;
  dir[0] = d.x; dir[1] = d.y; dir[2] = d.z;
  valid[0] = w > 0.0f ? 1u : 0u;
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
