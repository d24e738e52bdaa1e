// Adaptive sampling: per 4x4-pixel block sample rates chosen in up to four refinement stages from the measured
// variance, and the result image with its diagnostic modes.
// Reference: cuda/adaptive_sampling.cuh:9-240 (sample bookkeeping, block variance, stage sample counts),
// device/device_adaptive_sampler.c:60-215 (stage build), device/device_renderer.c:350-375 (when a stage is built),
// cuda/kernels.cuh:195-355 (tasks_create_adaptive_sampling), cuda/accumulation.cuh:86-200 (accumulation_generate_result).
//
// Bookkeeping (DeviceSampleAllocation, device_utils.h:331-338): an *execution* of stage 0 takes one sample of every pixel; an execution
// of stage s >= 1 takes count_s(block) samples of every pixel of a block, count_s - 1 being byte s-1 of stage_counts[block]. A pixel's
// samples are consecutive ids, so the samples it has received so far are also the id of its next one.
//
// What differs from the reference, on purpose: the reference adds the block variances with a float atomicAdd (order unspecified) and
// builds a stage asynchronously (the number of executions per stage depends on timing). Here the sum is a fixed two-level sequential
// order (chunks of 256 blocks, then the chunk sums) and a stage is built exactly after `update_interval << stage` executions, so the
// oracle reproduces every count bit for bit. The reference's task-range machinery (prefix mips, tile block ranges) exists for its
// per-thread task layout and has no counterpart: tasks are addressed through one inclusive prefix sum over blocks.
#pragma once

#include "dev_output.h"
#include "dev_scene.h"

LUM_NS_BEGIN

constexpr uint32_t kAdaptiveBlockLog = 2;        // ADAPTIVE_SAMPLING_BLOCK_SIZE_LOG, device_utils.h:32
constexpr uint32_t kAdaptiveMaxRate = 256;       // ADAPTIVE_SAMPLING_MAX_SAMPLING_RATE, device_utils.h:35
constexpr uint32_t kAdaptiveSumChunk = 256;      // blocks per partial sum of the variance total

// samples per pixel and execution of `stage`: one in stage 0, the block's rate in stages 1..4
LUM_DEV uint32_t adaptive_stage_count(uint32_t packed, uint32_t stage) { return stage ? ((packed >> ((stage - 1u) * 8u)) & 0xFFu) + 1u : 1u; }
// adaptive_sampling.cuh:57-76 / :78-105: samples a pixel of this block has received = id of its next sample
LUM_DEV uint32_t adaptive_pixel_samples(const AdaptiveView& a, uint32_t packed) {
  uint32_t n = a.executions[0];
#pragma unroll
  for (uint32_t s = 1; s <= kAdaptiveStages; s++) n += a.executions[s] * (((packed >> ((s - 1u) * 8u)) & 0xFFu) + 1u);
  return n;
}
LUM_DEV uint32_t adaptive_block_of(const AdaptiveView& a, uint32_t x, uint32_t y) { return (x >> kAdaptiveBlockLog) + (y >> kAdaptiveBlockLog) * a.blocks_x; }

// adaptive_sampling.cuh:122-166
LUM_DEV float adaptive_pixel_variance(const float* __restrict__ fm, const float* __restrict__ sm, uint32_t num_pixels, uint32_t index, float inv_n, Col& mean) {
  const float r1 = fm[index] * inv_n, g1 = fm[num_pixels + index] * inv_n, b1 = fm[2 * num_pixels + index] * inv_n;
  mean = col(r1, g1, b1);
  const float lum2 = sm[index] * inv_n;
  const float lum_sq = luminance(col(r1 * r1, g1 * g1, b1 * b1));
  return fmaxf(lum2 - lum_sq, 0.0f);
}
// adaptive_sampling.cuh:9-18
LUM_DEV float adaptive_tonemap_compression(const OutputParams& op, Col color, float exposure) {
  const Col exposed = color * exposure;
  const Col mapped = tonemap_curve(op, exposed);
  const float ev = luminance(exposed), tv = luminance(mapped);
  return (ev > 0.0f) ? tv / ev : 1.0f;
}

// accumulation_generate_result (cuda/accumulation.cuh:86-200): mean radiance (optionally with local error minimisation) or one of
// the diagnostic images. With a null stage_counts every pixel has `uniform_samples` samples (adaptive sampling off).
struct ResultParams {
  uint32_t width, height;
  uint32_t mode;            // LuminaryAdaptiveSamplingOutputMode: 0 beauty, 1 variance, 2 error, 3 sample distribution
  uint32_t local_error_minimization;
  uint32_t uniform_samples;
  float exposure;           // camera exposure (error mode)
};

LUM_DEV uint32_t result_pixel_samples(const AdaptiveView& a, const ResultParams& rp, uint32_t x, uint32_t y) {
  return a.stage_counts ? adaptive_pixel_samples(a, a.stage_counts[adaptive_block_of(a, x, y)]) : rp.uniform_samples;
}

LUM_NS_END
