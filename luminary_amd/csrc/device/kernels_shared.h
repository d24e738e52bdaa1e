// The flavour-neutral kernels of the render schedule's unit: bookkeeping (accumulation, adaptive rates), the display chain and the helpers of the plain-array
// entry points. They exist once, in the exact inline namespace, and are launched directly by csrc/host/core.hip - the only unit that includes this header,
// compiled with the exact flavour's flags. The scene's kernels are kernels_scene.h (scene_device.hip); the wavefront kernels (kernels.h) are not included:
// they belong to wavefront_exact.hip / wavefront_fast.hip. This unit has its own copy of the sampler's seed table (dev_sampler.h), filled by lumc_context_create.
#pragma once

#include "dev_camera.h"
#include "dev_wave.h"  // kBlock
#include "dev_output.h"
#include "dev_adaptive.h"

LUM_NS_BEGIN

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

// ---- accumulation (cuda/accumulation.cuh:63-84): samples of a pixel are added in sample order ----
// Pixel-major result slots (results[p * batch + k], kernels.h): a pixel's samples are neighbours in memory and the pixels of a wave lie `batch` x 16 bytes apart, so
// a lane reading its own pixel's row would touch a cache line per lane and load. Instead a wave brings a tile of 64 pixels x kAccTile samples through LDS - rows of
// kAccTile x 16 = 128 contiguous bytes, the tile's float4s dealt to the lanes in memory order - and every lane then adds its pixel's row from there in sample order,
// one float add after the other: the expressions and their order are the sample-major loop's, so are the bits.
// LDS layout (dynamic: kAccTileBytes per workgroup, none for sample-major slots): float4 `at` of tile row `row` sits at row * kAccTile + (at ^ (row & 7)): the rows
// are 128 bytes apart, and without the swizzle the 64 lanes of a read (same `at`, 64 rows) would meet in the same four banks.
constexpr uint32_t kAccTile = 8;
constexpr uint32_t kAccTileBytes = kBlock * kAccTile * (uint32_t) sizeof(float4);
LUM_DEV void accumulate_pixel_major(const float4* __restrict__ results, uint32_t num_pixels, uint32_t batch, float* first_moment, float* second_moment, float4* tiles) {
  static_assert(kAccTile == 8u, "the swizzle and the shifts below are written for rows of eight");
  const uint32_t lane = threadIdx.x & 63u;
  float4* tile = tiles + (threadIdx.x >> 6) * (64u * kAccTile);
  const uint32_t rounds = (num_pixels + gridDim.x * kBlock - 1u) / (gridDim.x * kBlock);  // whole workgroups go round together: the barriers below
  for (uint32_t round = 0; round < rounds; round++) {
    const uint32_t p = (round * gridDim.x + blockIdx.x) * kBlock + threadIdx.x;
    const uint32_t p0 = p - lane;  // the wave's first pixel
    const bool active = p < num_pixels;
    float r = 0.0f, g = 0.0f, b = 0.0f, s = 0.0f;
    if (active) {
      r = first_moment[p]; g = first_moment[num_pixels + p]; b = first_moment[2 * num_pixels + p];
      s = second_moment ? second_moment[p] : 0.0f;
    }
    for (uint32_t k0 = 0; k0 < batch; k0 += kAccTile) {
      const uint32_t kc = min(kAccTile, batch - k0);
#pragma unroll
      for (uint32_t j = 0; j < kAccTile; j++) {
        const uint32_t e = j * 64u + lane, row = e >> 3, at = e & 7u;
        if (p0 + row < num_pixels && at < kc) tile[row * kAccTile + (at ^ (row & 7u))] = results[(size_t) (p0 + row) * batch + k0 + at];
      }
      __syncthreads();
      if (active) {
        for (uint32_t k = 0; k < kc; k++) {
          const float4 v = tile[lane * kAccTile + (k ^ (lane & 7u))];
          r += v.x; g += v.y; b += v.z;
          s += luminance(col(v.x * v.x, v.y * v.y, v.z * v.z));
        }
      }
      __syncthreads();
    }
    if (active) {
      first_moment[p] = r; first_moment[num_pixels + p] = g; first_moment[2 * num_pixels + p] = b;
      if (second_moment) second_moment[p] = s;
    }
  }
}
// pixel_major: the order of the result slots (PassParams::pixel_major); with it the launch brings kAccTileBytes of dynamic LDS
__global__ __launch_bounds__(kBlock) void k_accumulate(const float4* results, uint32_t num_pixels, uint32_t batch, float* first_moment, float* second_moment, uint32_t pixel_major) {
  extern __shared__ float4 accumulate_tiles[];
  if (pixel_major) { accumulate_pixel_major(results, num_pixels, batch, first_moment, second_moment, accumulate_tiles); return; }
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

LUM_NS_END
