// Refit of the light tree (lum_core.h lumc_light_refit_*): the ONE definition of what a moved emitter does to the light sampling
// structures, compiled twice - by the host compiler into light_refit.cpp (light_refit_host: the twin, no HIP in it) and by the device compiler into
// light_refit.hip (k_light_fragments, k_light_slot_stats, k_light_nodes) - under -ffp-contract=off with IEEE divide and square root, so that both give the same
// bytes; what the context keeps of a bound plan; and the calls of the scene update (scene_device.hip).
//
// All of it is binary32, one rounding per operation, in this order.
//   Fragment   scene.cpp build_light_tree's own arithmetic: every vertex through rotate_q (and rotate_q_w for the fourth lane), * scale + offset; the area from
//              the cross product in vec128_hsum's order; middle = (a + (b + c)) * (1 / 3), wm likewise; power = (intensity * area) * average_intensity.
//   Slot       a child's statistics are a function of its range [first, first + count) of fragments alone, in a wave-shaped order: lane l of 64 takes the items
//              first + l, first + l + 64, ... in ascending order from +0, the 64 partials are combined by the xor butterfly 32, 16, 8, 4, 2, 1 (p[l] + p[l ^ k]).
//              Power is a plain sum; inv_total = 1 / power; the mean (four lanes) is fma(middle, power_i * inv_total, acc); the variance adds, per item and in
//              vertex order, w * dot4(v_k - mean) with w = ((1 / 3) * power_i) * inv_total and dot4 = (x x + z z) + (y y + w w). The build's rule "take the
//              binned power unless it is tiny" does not exist here: the binned sums cannot be had without the bins.
//   Quantiser  scene.cpp make_quantiser / quantise_child with one difference: the exponent is the exact ceil(log2(x)) of the float x = range * 1.0f / 255.0f, from
//              its exponent and mantissa bits, clamped to -126 ... 126 (libm's log2f is not correctly rounded: within a few ulp above a power of two it can give
//              one less, harmless for the build and not reproducible on a GPU), and 1 / exp2(e) is ldexp(1, -e). Minima and maxima are `b < a ? b : a` chains in
//              slot order.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../../include/lum_core.h"

#if defined(__HIPCC__)
#define LUM_LRF_FN __host__ __device__ __forceinline__
#else
#define LUM_LRF_FN inline
#endif

namespace lum {

constexpr uint32_t kLightRootSlots = 128, kLightNodeSlots = 8, kLightWave = 64;
constexpr uint32_t kLightRecordVecs = 5;  // per fragment: v0 | w0, v1 | w1, v2 | w2, middle | wm, power | 0 0 0
constexpr uint32_t kLightStatFloats = 8;  // per slot: power, variance, mean x y z w, 0, 0
constexpr float kLightMaxValue = 1e10f;   // scene.cpp kMaxValue
constexpr uint32_t kLightRefitFlagBadPlan = 4u;  // beside LUMC_LIGHT_REFIT_*: an index of the plan beyond the scene reached a kernel

struct alignas(16) LrfVec { float x, y, z, w; };

LUM_LRF_FN uint32_t lrf_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
LUM_LRF_FN float lrf_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
LUM_LRF_FN bool lrf_finite(float f) { return (lrf_bits(f) & 0x7F800000u) != 0x7F800000u; }
LUM_LRF_FN float lrf_min(float a, float b) { return b < a ? b : a; }
LUM_LRF_FN float lrf_max(float a, float b) { return a < b ? b : a; }

// scene.cpp rotate_q with rotate_q_w as its fourth lane, then * scale + offset (scale.w = 1, offset.w = 0)
LUM_LRF_FN LrfVec lrf_world(const float a[3], const LumLightTransform& t) {
  const float* q = t.q;
  const float dqa = a[0] * q[0] + a[1] * q[1] + a[2] * q[2], dqq = q[0] * q[0] + q[1] * q[1] + q[2] * q[2];
  const float cr[3] = {q[1] * a[2] - q[2] * a[1], q[2] * a[0] - q[0] * a[2], q[0] * a[1] - q[1] * a[0]};
  float r[3];
  for (int k = 0; k < 3; k++) {
    float v = q[k] * (2.0f * dqa);
    v = v + a[k] * (q[3] * q[3] - dqq);
    v = v + cr[k] * (2.0f * q[3]);
    r[k] = v * t.scale[k] + t.offset[k];
  }
  float w = q[3] * (2.0f * dqa);
  w = w + 0.0f * (q[3] * q[3] - dqq);
  w = w + 0.0f * (2.0f * q[3]);
  return LrfVec{r[0], r[1], r[2], w * 1.0f + 0.0f};
}

// One fragment from its three object-space vertices p[9]: the record (kLightRecordVecs vectors). Returns LUMC_LIGHT_REFIT_* flags.
LUM_LRF_FN uint32_t lrf_fragment(const LumLightFragment& f, const LumLightTransform& t, const float p[9], LrfVec rec[5]) {
  const LrfVec a = lrf_world(p, t), b = lrf_world(p + 3, t), c = lrf_world(p + 6, t);
  const float u[3] = {b.x - a.x, b.y - a.y, b.z - a.z}, v[3] = {c.x - a.x, c.y - a.y, c.z - a.z};
  const float cr[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
  const float area = 0.5f * ::sqrtf((cr[0] * cr[0] + cr[2] * cr[2]) + (cr[1] * cr[1] + 0.0f));
  const float third = 1.0f / 3.0f;
  rec[0] = a; rec[1] = b; rec[2] = c;
  rec[3] = LrfVec{(a.x + (b.x + c.x)) * third, (a.y + (b.y + c.y)) * third, (a.z + (b.z + c.z)) * third, (a.w + (b.w + c.w)) * third};
  const float power = f.intensity * area * f.average_intensity;
  rec[4] = LrfVec{power, 0.0f, 0.0f, 0.0f};
  uint32_t flags = 0;
  bool finite = lrf_finite(power);
  for (int k = 0; k < 9; k++) finite = finite && lrf_finite(p[k]);
  for (int k = 0; k < 4; k++) finite = finite && lrf_finite(rec[k].x) && lrf_finite(rec[k].y) && lrf_finite(rec[k].z) && lrf_finite(rec[k].w);
  if (!finite) flags |= LUMC_LIGHT_REFIT_NOT_FINITE;
  if (area == 0.0f || power == 0.0f) flags |= LUMC_LIGHT_REFIT_ZERO_AREA;  // (a power that underflows to 0 has no place in the tree either)
  return flags;
}

// ---- slot statistics: one lane's share of the range; the callers combine the 64 lanes by the butterfly ----
LUM_LRF_FN float lrf_lane_power(const LrfVec* rec, uint32_t first, uint32_t count, uint32_t lane) {
  float acc = 0.0f;
  for (uint32_t i = lane; i < count; i += kLightWave) acc = acc + rec[kLightRecordVecs * (size_t) (first + i) + 4].x;
  return acc;
}
LUM_LRF_FN LrfVec lrf_lane_mean(const LrfVec* rec, uint32_t first, uint32_t count, uint32_t lane, float inv_total) {
  LrfVec m{0.0f, 0.0f, 0.0f, 0.0f};
  for (uint32_t i = lane; i < count; i += kLightWave) {
    const LrfVec* r = rec + kLightRecordVecs * (size_t) (first + i);
    const LrfVec mid = r[3];
    const float w = r[4].x * inv_total;
    m.x = ::fmaf(mid.x, w, m.x); m.y = ::fmaf(mid.y, w, m.y); m.z = ::fmaf(mid.z, w, m.z); m.w = ::fmaf(mid.w, w, m.w);
  }
  return m;
}
LUM_LRF_FN float lrf_lane_variance(const LrfVec* rec, uint32_t first, uint32_t count, uint32_t lane, float inv_total, LrfVec mean) {
  float var = 0.0f;
  for (uint32_t i = lane; i < count; i += kLightWave) {
    const LrfVec* r = rec + kLightRecordVecs * (size_t) (first + i);
    const float w = (1.0f / 3.0f) * r[4].x * inv_total;
    for (int k = 0; k < 3; k++) {
      const LrfVec v = r[k];
      const float dx = v.x - mean.x, dy = v.y - mean.y, dz = v.z - mean.z, dw = v.w - mean.w;
      var = var + w * ((dx * dx + dz * dz) + (dy * dy + dw * dw));
    }
  }
  return var;
}

// ---- quantiser ----
// ceil(log2(x)) of a finite x > 0, exact
LUM_LRF_FN int lrf_ceil_log2(float x) {
  const uint32_t b = lrf_bits(x), m = b & 0x007FFFFFu;
  const int e = (int) ((b >> 23) & 0xFFu);
  if (e == 0) {  // subnormal: m * 2^-149
    int hi = 0;
    while ((m >> (hi + 1)) != 0u) hi++;
    return (hi - 149) + ((m & (m - 1u)) != 0u ? 1 : 0);
  }
  return (e - 127) + (m != 0u ? 1 : 0);
}
LUM_LRF_FN int lrf_exponent_for(float range) {
  const float x = range * 1.0f / 255.0f;
  if (!(x > 0.0f)) return -126;
  if (!lrf_finite(x)) return 126;
  const int e = lrf_ceil_log2(x);
  return e < -126 ? -126 : (e > 126 ? 126 : e);
}
// scene.cpp pack_float_mode / unpack_float16 (device_packing.c:46-70; mode 0 floor, 1 ceil)
LUM_LRF_FN uint32_t lrf_pack_float(float v, int mode) {
  uint32_t b = lrf_bits(v);
  if (mode == 1) { if (v >= 0.0f) b += (1u << 16) - 1; }
  else { if (v < 0.0f) b += (1u << 16) - 1; }
  return b >> 16;
}
LUM_LRF_FN float lrf_unpack_float(uint32_t v16) { return lrf_float((v16 & 0xFFFFu) << 16); }

struct LrfQuantiser { float min_mean[3], c[4], max_power; int e[4]; uint32_t base[3]; };

// stats: kLightStatFloats per slot; slots with a power of 0 are unused (a used child's power is > 0: every fragment's is)
LUM_LRF_FN LrfQuantiser lrf_make_quantiser(const float* stats, uint32_t slots) {
  float mn[3] = {kLightMaxValue, kLightMaxValue, kLightMaxValue}, mx[3] = {-kLightMaxValue, -kLightMaxValue, -kLightMaxValue};
  float max_variance = 0.0f, max_power = 0.0f;
  for (uint32_t c = 0; c < slots; c++) {
    const float* s = stats + kLightStatFloats * (size_t) c;
    if (!(s[0] > 0.0f)) continue;
    for (int a = 0; a < 3; a++) { mn[a] = lrf_min(mn[a], s[2 + a]); mx[a] = lrf_max(mx[a], s[2 + a]); }
    max_variance = lrf_max(max_variance, s[1]);
    max_power = lrf_max(max_power, s[0]);
  }
  const float max_std_dev = ::sqrtf(max_variance);
  LrfQuantiser q;
  for (int a = 0; a < 3; a++) {
    q.base[a] = lrf_pack_float(mn[a], 0);
    q.min_mean[a] = lrf_unpack_float(q.base[a]);
    q.e[a] = (mx[a] != q.min_mean[a]) ? lrf_exponent_for(mx[a] - q.min_mean[a]) : 0;
  }
  q.e[3] = (max_std_dev > 0.0f) ? lrf_exponent_for(max_std_dev) : 0;
  for (int a = 0; a < 4; a++) q.c[a] = ::ldexpf(1.0f, -q.e[a]);
  q.max_power = max_power;
  return q;
}

struct LrfChild { uint32_t m[3], sd, power; };
LUM_LRF_FN uint32_t lrf_to_byte(float v) { return (uint32_t) (uint8_t) (uint64_t) v; }
LUM_LRF_FN LrfChild lrf_quantise_child(const LrfQuantiser& q, const float* s, uint32_t power_scale) {
  LrfChild o;
  for (int a = 0; a < 3; a++) o.m[a] = lrf_to_byte(::floorf((s[2 + a] - q.min_mean[a]) * q.c[a] + 0.5f));
  uint64_t sd = (uint64_t) (::sqrtf(s[1]) * q.c[3] + 0.5f);
  uint64_t pw = (uint64_t) ::floorf((float) power_scale * s[0] / q.max_power + 0.5f);
  if (sd < 1) sd = 1;
  if (pw < 1) pw = 1;
  o.sd = (uint32_t) (uint8_t) sd; o.power = (uint32_t) pw;
  return o;
}

// ---- nodes: lane c of 8 writes child c's bytes (24 + c, 32 + c, 40 + c, 48 + c, 56 + c), lane 0 the base (0-5) and the exponents (8-11); the counts (12) and the
// pointers (16-23) are not touched. stats: the node's 8 slots. ----
LUM_LRF_FN void lrf_node_lane(const float* stats, uint32_t c, uint8_t* node) {
  const LrfQuantiser q = lrf_make_quantiser(stats, kLightNodeSlots);
  if (c == 0) {
    for (int a = 0; a < 3; a++) { node[2 * a] = (uint8_t) (q.base[a] & 0xFFu); node[2 * a + 1] = (uint8_t) (q.base[a] >> 8); }
    for (int a = 0; a < 4; a++) node[8 + a] = (uint8_t) (int8_t) q.e[a];
  }
  const float* s = stats + kLightStatFloats * (size_t) c;
  if (!(s[0] > 0.0f)) return;
  const LrfChild ch = lrf_quantise_child(q, s, 0xFFu);
  node[24 + c] = (uint8_t) ch.m[0]; node[32 + c] = (uint8_t) ch.m[1]; node[40 + c] = (uint8_t) ch.m[2]; node[48 + c] = (uint8_t) ch.sd; node[56 + c] = (uint8_t) ch.power;
}

// ---- root: lane c of 128 (c < 8 * sections) writes child c's bytes of its section, its 8 floats of the float table (scene_device.hip
// upload_light_root_children: mean = byte * 2^e + base per axis, sigma = byte * 2^e_sigma, the power) and its (power, variance) of `result`; lane 0 the header's
// base (0-5), maximal power (8-9) and exponents (12-15); the light count (6-7) and the section count (10-11) are not touched. An unused slot of the last section
// keeps its zero bytes, so its table entry is the new base. stats: the root's 128 slots. ----
LUM_LRF_FN void lrf_root_lane(const float* stats, uint32_t c, uint32_t sections, uint8_t* root, float* table, float* result) {
  const LrfQuantiser q = lrf_make_quantiser(stats, kLightRootSlots);
  if (c == 0) {
    for (int a = 0; a < 3; a++) { root[2 * a] = (uint8_t) (q.base[a] & 0xFFu); root[2 * a + 1] = (uint8_t) (q.base[a] >> 8); }
    const uint32_t mp = lrf_pack_float(q.max_power, 1);
    root[8] = (uint8_t) (mp & 0xFFu); root[9] = (uint8_t) (mp >> 8);
    for (int a = 0; a < 4; a++) root[12 + a] = (uint8_t) (int8_t) q.e[a];
  }
  if (c >= 8u * sections) return;
  const float* s = stats + kLightStatFloats * (size_t) c;
  const bool used = s[0] > 0.0f;
  LrfChild ch{{0u, 0u, 0u}, 0u, 0u};
  if (used) {
    ch = lrf_quantise_child(q, s, 0xFFFFu);
    uint8_t* sec = root + 16 + 48 * (size_t) (c / 8u);
    const uint32_t k = c % 8u;
    sec[k] = (uint8_t) ch.m[0]; sec[8 + k] = (uint8_t) ch.m[1]; sec[16 + k] = (uint8_t) ch.m[2]; sec[24 + k] = (uint8_t) ch.sd;
    sec[32 + 2 * k] = (uint8_t) (ch.power & 0xFFu); sec[33 + 2 * k] = (uint8_t) ((ch.power >> 8) & 0xFFu);
  }
  float* e = table + 8 * (size_t) c;
  for (int a = 0; a < 3; a++) { const float scaled = (float) ch.m[a] * ::ldexpf(1.0f, (int8_t) q.e[a]); e[a] = scaled + q.min_mean[a]; }
  e[3] = (float) ch.sd * ::ldexpf(1.0f, (int8_t) q.e[3]);
  e[4] = (float) (ch.power & 0xFFFFu);
  result[2 * c] = used ? s[0] : 0.0f; result[2 * c + 1] = used ? s[1] : 0.0f;
}

// The host twin (light_refit.cpp; no GPU), see lum_core.h lumc_light_refit_host.
int light_refit_host(const LumLightRefitPlan* plan, const float* vertices, const uint32_t* mesh_tri_offset, uint8_t* root, float* root_children, uint8_t* nodes,
                     float* light_bvh_tris, float* slot_stats, LumLightRefitReport* report);

}  // namespace lum

#if defined(__HIP_PLATFORM_AMD__) && !defined(LUM_LRF_HOST_ONLY)
#include <hip/hip_runtime_api.h>

#include <vector>

#include "bvh_refit.h"
#include "device_buffer.h"

#pragma GCC visibility push(hidden)

namespace lum {

// A bound plan on the context's device.
struct LightRefit {
  DeviceBuffer<LumLightFragment> fragments;
  DeviceBuffer<LumLightTransform> transforms;
  DeviceBuffer<LumLightSlot> slots;       // 128 + 8 * num_nodes
  DeviceBuffer<float4> records;           // scratch: kLightRecordVecs per fragment
  DeviceBuffer<float4> tris;              // scratch: 3 per light, light-id order - light_bvh_tris, and the vertices the light BVH is refitted from
  DeviceBuffer<float> stats;              // scratch: kLightStatFloats per slot
  DeviceBuffer<float> result;             // the root children's (power, variance), 1 KB, then k_light_nodes' own copy of them
  std::vector<LumLightTransform> pending; // lumc_light_refit_transforms: the table the next refit uploads first (empty: none)
  DeviceBuffer<uint32_t> flags;           // one word
  RefitPlan bvh;                          // the light BVH's topology
  uint32_t num_fragments = 0, num_transforms = 0, num_nodes = 0, sections = 0;
  double root_cost = 0.0;
  bool bound = false;
  void reset() { fragments.reset(); transforms.reset(); slots.reset(); records.reset(); tris.reset(); stats.reset(); result.reset(); flags.reset(); bvh.reset(); pending.clear();
                 num_fragments = num_transforms = num_nodes = sections = 0; root_cost = 0.0; bound = false; }
};

// The plan into `r` on the current device (validated by the caller); sections: of the root it belongs to. r.bvh and r.bound are the caller's.
hipError_t light_refit_upload(LightRefit& r, const LumLightRefitPlan& plan, uint32_t sections);
// k_light_fragments over the plan's fragments: records, tris and the flag word (zeroed first). d_vertices / d_mesh_tri_offset: the scene's; total_corners bounds
// every read. Asynchronous.
hipError_t light_refit_fragments(LightRefit& r, const float4* d_vertices, const uint32_t* d_mesh_tri_offset, uint32_t num_meshes, uint32_t total_corners);
// k_light_slot_stats over every slot; the root's slots' (power, variance) also go to r.result. Asynchronous.
hipError_t light_refit_stats(LightRefit& r);
// k_light_nodes: the statistics' bytes of d_root (16 + 48 * sections bytes), d_root_children and d_nodes in place. Asynchronous.
hipError_t light_refit_nodes(LightRefit& r, uint8_t* d_root, float* d_root_children, uint8_t* d_nodes);

}  // namespace lum

#pragma GCC visibility pop
#endif
