// Denoiser: first-hit guide buffers and a variance-guided edge-avoiding a-trous wavelet filter on albedo-demodulated radiance (the filter stage of
// SVGF: Schied et al., "Spatiotemporal Variance-Guided Filtering", HPG 2017; the wavelet of Dammertz et al., "Edge-Avoiding A-Trous Wavelet
// Transform for fast Global Illumination Filtering", HPG 2010). No counterpart in the reference, whose denoiser was OptiX's. Off by default; a path of
// its own between the result image and bloom: no kernel of the renderer is touched.
//
//   k_guide            after one closest-hit pass over one sample id of every pixel: adds albedo, signed shading normal and hit distance into planes
//   k_guide_normalise  sums -> means: planes [albedo r g b | normal x y z | depth], depth -1 where no sample hit anything
//   k_denoise_prepare  per pixel two 16-byte records: A = {demodulated r, g, b, variance of the mean}, B = {octahedral normal, depth, |grad depth|, flags}
//   k_denoise_atrous   one launch per iteration i, taps 2^i apart, A ping-pongs, B stays; kLds: the tile and its halo staged in LDS (steps 1 and 2)
//   k_denoise_finish   times the albedo again, planar RGB; a pixel no iteration changed keeps its bits
// tests/support/denoise_check.c restates prepare, a-trous and finish in plain C; the exact flavour equals it bit for bit.
#pragma once

#include "dev_adaptive.h"
#include "kernels.h"

LUM_NS_BEGIN

// (kGuidePlanes, kGuideSumPlanes, struct DenoiseArgs: dev_scene.h)
constexpr uint32_t kDenoiseTileX = 32, kDenoiseTileY = 8;  // a workgroup of 256: each wave's two rows are 32 consecutive records (512 B per tap)
constexpr uint32_t kDenoiseMaxLdsStep = 2;
constexpr uint32_t kDenoiseLdsRecords = (kDenoiseTileX + 4 * kDenoiseMaxLdsStep) * (kDenoiseTileY + 4 * kDenoiseMaxLdsStep);  // 40 x 16: 20 KB with both records
constexpr float kDenoiseAlbedoFloor = 1e-3f;
constexpr float kDenoiseCutoff = -30.0f;  // taps below 2^-30 of their B3 weight are skipped

// ---- guides ----
__global__ __launch_bounds__(kBlock) void k_guide(DeviceScene sc, PathQueue in, const uint32_t* ctrl, float* planes, uint32_t n) {
  const uint32_t paths = ctrl[kCtlPaths];
  for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < paths; i += gridDim.x * kBlock) {
    const float4 o4 = in.origin_t[i], d4 = in.dir_slot[i];
    const uint4 aux = in.aux[i], hid = in.hit_id[i];
    const V3 origin = v3(o4.x, o4.y, o4.z), ray = v3(d4.x, d4.y, d4.z);
    const uint32_t p = (hid.z & 0xFFFFu) + (hid.z >> 16) * sc.width;  // one sample id per pass: a pixel has at most one path, so plain sums
    if (p >= n) continue;
    Col albedo = splat(1.0f);  // misses, emitters, particles and the ocean surface are not demodulated
    V3 normal = v3(0.0f, 0.0f, 0.0f);
    bool hit = false;
    if (hid.x == kHitOcean) { normal = ocean_get_normal(sc, origin + ray * o4.w); hit = true; }
    else if (particle_is_hit(hid.x)) { normal = particle_context(sc, origin, ray, aux.w, hid.x).normal; hit = true; }
    else if (hid.x <= kHitTriangleLimit) {
      const GeoContext g = build_context(sc, origin + ray * o4.w, ray, aux.w, hid.x, hid.y, in.hit_scene_tri[i] & kHitTriMask, aux.z);
      if (!any_positive(g.params.emission())) albedo = g.params.albedo();
      normal = g.normal; hit = true;
    }
    planes[p] += albedo.r; planes[n + p] += albedo.g; planes[2 * n + p] += albedo.b;
    if (hit) {
      planes[3 * n + p] += normal.x; planes[4 * n + p] += normal.y; planes[5 * n + p] += normal.z;
      planes[6 * n + p] += o4.w;
      planes[7 * n + p] += 1.0f;
    }
    planes[8 * n + p] += 1.0f;
  }
}

// A sample without a path (a physical camera's ray that did not leave the lens) counts as a miss: albedo 1.
__global__ __launch_bounds__(256) void k_guide_normalise(float* planes, uint32_t n, uint32_t samples) {
  const float count = (float) samples;
  for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < n; p += gridDim.x * 256u) {
    const float hits = planes[7 * n + p], missing = count - planes[8 * n + p];
#pragma unroll
    for (uint32_t k = 0; k < 3; k++) planes[k * n + p] = (planes[k * n + p] + missing) / count;
#pragma unroll
    for (uint32_t k = 3; k < 6; k++) planes[k * n + p] = planes[k * n + p] / count;
    planes[6 * n + p] = (hits > 0.0f) ? planes[6 * n + p] / hits : -1.0f;
  }
}

// ---- filter ----
LUM_DEV float denoise_log2(float x) {
#if LUM_FAST
  return __builtin_amdgcn_logf(x);
#else
  return log2_det(x);
#endif
}
LUM_DEV float denoise_exp2(float x) {
#if LUM_FAST
  return __builtin_amdgcn_exp2f(x);
#else
  return exp2_det(x);
#endif
}

// octahedral map of a unit vector, 2 x snorm16
LUM_DEV uint32_t denoise_pack_normal(V3 n) {
  const float s = fabsf(n.x) + fabsf(n.y) + fabsf(n.z);
  float px = n.x / s, py = n.y / s;
  if (n.z < 0.0f) {
    const float qx = (1.0f - fabsf(py)) * ((px >= 0.0f) ? 1.0f : -1.0f), qy = (1.0f - fabsf(px)) * ((py >= 0.0f) ? 1.0f : -1.0f);
    px = qx; py = qy;
  }
  const int ix = (int) rintf(fminf(fmaxf(px, -1.0f), 1.0f) * 32767.0f), iy = (int) rintf(fminf(fmaxf(py, -1.0f), 1.0f) * 32767.0f);
  return ((uint32_t) ix & 0xFFFFu) | ((uint32_t) iy << 16);
}
LUM_DEV V3 denoise_unpack_normal(uint32_t packed) {
  float px = (float) (int) (short) (packed & 0xFFFFu) * (1.0f / 32767.0f), py = (float) ((int) packed >> 16) * (1.0f / 32767.0f);
  const float z = (1.0f - fabsf(px)) - fabsf(py);
  if (z < 0.0f) {
    const float qx = (1.0f - fabsf(py)) * ((px >= 0.0f) ? 1.0f : -1.0f), qy = (1.0f - fabsf(px)) * ((py >= 0.0f) ? 1.0f : -1.0f);
    px = qx; py = qy;
  }
  const float s = 1.0f / sqrtf(px * px + py * py + z * z);
  return v3(px * s, py * s, z * s);
}

__global__ __launch_bounds__(256) void k_denoise_prepare(AdaptiveView a, DenoiseArgs p, const float* __restrict__ fm, const float* __restrict__ sm, const float* __restrict__ image,
                                                        const float* __restrict__ guides, float4* __restrict__ rec_a, uint4* __restrict__ rec_b) {
  const uint32_t n = p.width * p.height;
  for (uint32_t index = blockIdx.x * 256u + threadIdx.x; index < n; index += gridDim.x * 256u) {
    const uint32_t y = index / p.width, x = index - y * p.width;
    const uint32_t samples = a.stage_counts ? adaptive_pixel_samples(a, a.stage_counts[adaptive_block_of(a, x, y)]) : p.uniform_samples;
    const Col albedo = col(fmaxf(guides[index], kDenoiseAlbedoFloor), fmaxf(guides[n + index], kDenoiseAlbedoFloor), fmaxf(guides[2 * n + index], kDenoiseAlbedoFloor));
    // variance of the mean of the luminance, as the variance result image computes it, brought to the demodulated signal's scale
    float variance = 0.0f;
    if (samples > 0u) {
      const float inv_n = 1.0f / (float) samples;
      Col mean;
      const float la = luminance(albedo);
      variance = (adaptive_pixel_variance(fm, sm, n, index, inv_n, mean) * inv_n) / (la * la);
    }
    rec_a[index] = make_float4(image[index] / albedo.r, image[n + index] / albedo.g, image[2 * n + index] / albedo.b, variance);
    const float depth = guides[6 * n + index];
    uint4 b = make_uint4(0u, 0u, 0u, 0u);
    if (depth >= 0.0f) {
      const V3 nrm = v3(guides[3 * n + index], guides[4 * n + index], guides[5 * n + index]);
      const float len2 = dot(nrm, nrm);
      const float inv = (len2 > 0.0f) ? 1.0f / sqrtf(len2) : 0.0f;
      b.x = denoise_pack_normal((len2 > 0.0f) ? v3(nrm.x * inv, nrm.y * inv, nrm.z * inv) : v3(0.0f, 0.0f, 1.0f));
      // central differences over the neighbours inside the frame; a neighbour that missed takes this pixel's depth
      const uint32_t xl = max(x, 1u) - 1u, xr = min(x + 1u, p.width - 1u), yl = max(y, 1u) - 1u, yr = min(y + 1u, p.height - 1u);
      float zl = guides[6 * n + xl + y * p.width], zr = guides[6 * n + xr + y * p.width], zd = guides[6 * n + x + yl * p.width], zu = guides[6 * n + x + yr * p.width];
      zl = (zl >= 0.0f) ? zl : depth; zr = (zr >= 0.0f) ? zr : depth; zd = (zd >= 0.0f) ? zd : depth; zu = (zu >= 0.0f) ? zu : depth;
      const float gx = (xr > xl) ? (zr - zl) / (float) (xr - xl) : 0.0f, gy = (yr > yl) ? (zu - zd) / (float) (yr - yl) : 0.0f;
      b.y = fbits(depth); b.z = fbits(fmaxf(fabsf(gx), fabsf(gy))); b.w = 1u;
    }
    rec_b[index] = b;
  }
}

// May p's filter look at q at all? Never across hit / miss, and not across a fold of 90 degrees or more.
LUM_DEV bool denoise_same_surface(bool hit_p, V3 n_p, const uint4& bq) {
  if (((bq.w & 1u) != 0u) != hit_p) return false;
  return !hit_p || dot(n_p, denoise_unpack_normal(bq.x)) > 0.0f;
}

// One pixel of one iteration; fetch(x, y, A, B) reads the records of a pixel inside the frame.
template <typename Fetch>
LUM_DEV float4 denoise_pixel(const DenoiseArgs& p, uint32_t x, uint32_t y, const Fetch& fetch) {
  float4 ap; uint4 bp;
  fetch(x, y, ap, bp);
  const bool hit = (bp.w & 1u) != 0u;
  const V3 n_p = hit ? denoise_unpack_normal(bp.x) : v3(0.0f, 0.0f, 0.0f);
  const float z_p = bitsf(bp.y), grad_p = bitsf(bp.z);
  // g(var): 3 x 3 Gaussian of the current variance over the adjacent pixels of the same surface
  float gsum = 0.0f, ksum = 0.0f;
#pragma unroll
  for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
    for (int dx = -1; dx <= 1; dx++) {
      const int qx = (int) x + dx, qy = (int) y + dy;
      if (qx < 0 || qy < 0 || qx >= (int) p.width || qy >= (int) p.height) continue;
      const float k = (dx == 0 && dy == 0) ? 0.25f : (dx == 0 || dy == 0) ? 0.125f : 0.0625f;
      float4 aq = ap; uint4 bq = bp;
      if (dx != 0 || dy != 0) {
        fetch((uint32_t) qx, (uint32_t) qy, aq, bq);
        if (!denoise_same_surface(hit, n_p, bq)) continue;
      }
      gsum += k * aq.w; ksum += k;
    }
  }
  const float g = gsum / ksum;
  if (g == 0.0f) return ap;  // nothing to remove here: a converged image passes through bit for bit
  const float l_p = luminance(col(ap.x, ap.y, ap.z));
  const float den_l = p.sigma_luminance * sqrtf(g) + 1e-6f;
  const float fstep = (float) p.step;
  float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f;
#pragma unroll
  for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
    for (int dx = -2; dx <= 2; dx++) {
      const int qx = (int) x + dx * (int) p.step, qy = (int) y + dy * (int) p.step;
      if (qx < 0 || qy < 0 || qx >= (int) p.width || qy >= (int) p.height) continue;
      const float hx = (dx == 0) ? 0.375f : (dx == 1 || dx == -1) ? 0.25f : 0.0625f, hy = (dy == 0) ? 0.375f : (dy == 1 || dy == -1) ? 0.25f : 0.0625f;
      float w = hx * hy;
      float4 aq = ap;
      if (dx != 0 || dy != 0) {
        uint4 bq;
        fetch((uint32_t) qx, (uint32_t) qy, aq, bq);
        if (((bq.w & 1u) != 0u) != hit) continue;
        float e = 0.0f;
        if (hit) {
          const float d = fminf(dot(n_p, denoise_unpack_normal(bq.x)), 1.0f);
          if (!(d > 0.0f)) continue;
          const float len = sqrtf((float) (dx * dx + dy * dy)) * fstep;
          e = p.sigma_normal * denoise_log2(d) - (fabsf(z_p - bitsf(bq.y)) / (p.sigma_depth * grad_p * len + 1e-6f)) * 1.44269504f;
        }
        e = e - (fabsf(l_p - luminance(col(aq.x, aq.y, aq.z))) / den_l) * 1.44269504f;
        if (!(e >= kDenoiseCutoff)) continue;
        w = w * denoise_exp2(e);
      }
      sw += w; sr += w * aq.x; sg += w * aq.y; sb += w * aq.z; sv += (w * w) * aq.w;
    }
  }
  return make_float4(sr / sw, sg / sw, sb / sw, sv / (sw * sw));
}

template <bool kLds>
__global__ __launch_bounds__(256) void k_denoise_atrous(DenoiseArgs p, const float4* __restrict__ a_in, const uint4* __restrict__ rec_b, float4* __restrict__ a_out) {
  const uint32_t tx = threadIdx.x & (kDenoiseTileX - 1u), ty = threadIdx.x / kDenoiseTileX;
  const uint32_t ox = blockIdx.x * kDenoiseTileX, oy = blockIdx.y * kDenoiseTileY;
  const uint32_t x = ox + tx, y = oy + ty;
  if constexpr (kLds) {
    __shared__ float4 lds_a[kDenoiseLdsRecords];
    __shared__ uint4 lds_b[kDenoiseLdsRecords];
    const uint32_t halo = 2u * p.step, stride = kDenoiseTileX + 2u * halo, rows = kDenoiseTileY + 2u * halo;  // step <= kDenoiseMaxLdsStep (the launcher's duty)
    for (uint32_t i = threadIdx.x; i < stride * rows; i += 256u) {
      const uint32_t ly = i / stride, lx = i - ly * stride;
      const int gx = (int) (ox + lx) - (int) halo, gy = (int) (oy + ly) - (int) halo;
      if (gx >= 0 && gy >= 0 && gx < (int) p.width && gy < (int) p.height) {
        lds_a[i] = a_in[(uint32_t) gx + (uint32_t) gy * p.width];
        lds_b[i] = rec_b[(uint32_t) gx + (uint32_t) gy * p.width];
      }
    }
    __syncthreads();
    if (x >= p.width || y >= p.height) return;
    const auto fetch = [&](uint32_t qx, uint32_t qy, float4& aq, uint4& bq) {
      const uint32_t i = (qx + halo - ox) + (qy + halo - oy) * stride;
      aq = lds_a[i]; bq = lds_b[i];
    };
    a_out[x + y * p.width] = denoise_pixel(p, x, y, fetch);
  }
  else {
    if (x >= p.width || y >= p.height) return;
    const auto fetch = [&](uint32_t qx, uint32_t qy, float4& aq, uint4& bq) {
      aq = a_in[qx + qy * p.width]; bq = rec_b[qx + qy * p.width];
    };
    a_out[x + y * p.width] = denoise_pixel(p, x, y, fetch);
  }
}

// `image` still holds the input. A pixel whose record is what prepare wrote was changed by no iteration and keeps its bits (x / a * a is not x).
__global__ __launch_bounds__(256) void k_denoise_finish(DenoiseArgs p, const float4* __restrict__ rec_a, const float* __restrict__ guides, float* __restrict__ image) {
  const uint32_t n = p.width * p.height;
  for (uint32_t index = blockIdx.x * 256u + threadIdx.x; index < n; index += gridDim.x * 256u) {
    const Col albedo = col(fmaxf(guides[index], kDenoiseAlbedoFloor), fmaxf(guides[n + index], kDenoiseAlbedoFloor), fmaxf(guides[2 * n + index], kDenoiseAlbedoFloor));
    const float4 a = rec_a[index];
    const float r = image[index], g = image[n + index], b = image[2 * n + index];
    if (a.x == r / albedo.r && a.y == g / albedo.g && a.z == b / albedo.b) continue;
    image[index] = a.x * albedo.r; image[n + index] = a.y * albedo.g; image[2 * n + index] = a.z * albedo.b;
  }
}

LUM_NS_END
