// Image history: the shown frame reprojected into a moved camera and blended with the new accumulation (lum_core.h lumc_set_history / lumc_history_carry /
// lumc_history_blend). The ONE definition of both steps - history_reproject_pixel, history_blend_pixel -, compiled twice: by the host
// compiler into history.cpp (lumc_history_reproject_host, lumc_history_blend_host: the twin, no HIP in it) and by the device compiler into history.hip
// (k_history_reproject, k_history_blend), both in binary32, one operation at a time, under -ffp-contract=off with IEEE divide and square root, so that both give the
// same bytes. Only + - * / sqrt, comparisons, floor and conversions; minima, maxima and clamps are written as comparisons.
//
// State, per pixel p = x + y * width, two 16-byte records: shown[p] = {r, g, b, weight} - the image as it was last shown (after the denoiser, before bloom) and the
// number of samples it stands for - and guide[p] = {normal x, y, z, depth} - the first-hit guides it was shown with (depth < 0: sky). Beside them the key the state
// was shown from: HistoryKey {pos, rotation quaternion (x, y, z, w), fov, width, height}, as the scene view holds them. A carried plane carried[p] = {C r, g, b, W}.
//
// Vectors. dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z. cross(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x).
// rotate(q, v), dev_math.h's qapply: u = (q.x, q.y, q.z), duv = dot(u, v), duu = dot(u, u), cr = cross(u, v), t = 2 duv, k = q.w q.w - duu, m = 2 q.w;
//   per component r = (u t + v k) + cr m. conj(q) = (-q.x, -q.y, -q.z, q.w).
// Frame. step = 2 (fov / (float) width), vfov = (step (float) height) 0.5.
// Centre ray of pixel (px, py) - camera_ray (dev_camera.h) with aperture 0 and jitter (1/2, 1/2) -: sx = fov - step ((float) px + 0.5), sy = step ((float) py + 0.5) - vfov,
//   c = (-sx, -sy, -1), l = sqrt(dot(c, c)), dir = rotate(q, (c.x / l, c.y / l, c.z / l)). The origin is pos.
// Projection of a vector v relative to the camera (X - pos for a point, the direction itself for the sky): dc = rotate(conj(q), v); invalid unless dc.z < 0;
//   fx = (fov - dc.x / dc.z) / step - 0.5, fy = (dc.y / dc.z + vfov) / step - 0.5. The pixel (px, py)'s centre has fx = px, fy = py.
//
// Reproject, pixel (px, py) of the new key, its new guides n_cur, d_cur, the old key and the old state -> carried {C, W} and a class:
//   1. dir from the new key. d_cur >= 0 (surface): X = pos_new + dir d_cur per component, v = X - pos_old, r = sqrt(dot(v, v)). Otherwise (sky, a NaN included): v = dir.
//   2. project v with the old key. Invalid, or not (fx >= -1 and fx < (float) width and fy >= -1 and fy < (float) height) - which a NaN fails -: C = 0, W = 0, class OFF
//      (behind the old camera or off its frame: no tap exists).
//   3. x0 = floor(fx), y0 = floor(fy), tx = fx - x0, ty = fy - y0, ux = 1 - tx, uy = 1 - ty. Taps in this order, with their weights:
//      (x0, y0) ux uy, (x0 + 1, y0) tx uy, (x0, y0 + 1) ux ty, (x0 + 1, y0 + 1) tx ty.
//   4. a tap is valid iff it lies inside the old frame; its shown r, g, b and weight are finite and the weight > 0; sky: the old depth < 0; surface: the old depth >= 0
//      and |depth_old - r| <= depth_tolerance r and dot(n_cur, n_old) >= normal_threshold.
//   5. over the valid taps in tap order, from 0: ws += w, s_c += w shown_c, sw += w weight.
//   6. ws > 0: C_c = s_c / ws, W = min(max_history, sw / ws) ws, class CARRIED. Otherwise C = 0, W = 0, class REJECTED.
//
// Blend, pixel (x, y), N = (float) uniform sample count, cur the planar result image [3][P] after the denoiser, carried {C, W} (none: C = 0, W = 0):
//   1. a cur channel is not finite: shown = cur's bits, weight 0.
//   2. else not W > 0: shown = cur's bits, weight N.
//   3. else c = C; with clamp_sigma > 0, per channel: over the taps (x + dx, y + dy), dy = -1, 0, 1 outermost, dx = -1, 0, 1, that lie inside the frame, in that order,
//      k = their number, s = sum of cur from 0, mean = s / (float) k, then q = sum of (cur - mean)(cur - mean) from 0 in the same order, sigma = sqrt(q / (float) k),
//      lo = mean - clamp_sigma sigma, hi = mean + clamp_sigma sigma, c = c < lo ? lo : (c > hi ? hi : c) (a non-finite neighbour makes both comparisons false: c stays).
//      shown_c = (W c + N cur_c) / (W + N), weight = W + N.
//   The state becomes shown[p] = {shown, weight}, guide[p] = {n_cur, d_cur}; the image takes shown.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define LUM_HISTORY_FN __host__ __device__ __forceinline__
#else
#define LUM_HISTORY_FN inline
#endif

namespace lum {

struct alignas(16) HistoryRec { float x, y, z, w; };
struct HistoryKey { float pos[3]; float rot[4]; float fov; uint32_t width, height; };        // LumHistoryKey (lum_core.h), field for field
struct HistorySettings { uint32_t enabled; float max_history, depth_tolerance, normal_threshold, clamp_sigma; };  // LumHistoryParams, field for field
struct HistoryV3 { float x, y, z; };

enum : uint32_t { kHistoryCarried = 0, kHistoryRejected = 1, kHistoryOff = 2 };
constexpr uint32_t kHistoryTileX = 32, kHistoryTileY = 8;  // a workgroup: each wave holds two rows of 32 pixels
// k_history_reproject's counters: kHistoryStatStripes copies of {carried, rejected, off}, kHistoryStatStride words (a 64-byte line) apart; a workgroup adds to one, the host sums them
constexpr uint32_t kHistoryStatStripes = 32, kHistoryStatStride = 16, kHistoryStatWords = kHistoryStatStripes * kHistoryStatStride;

LUM_HISTORY_FN bool history_finite(float f) { uint32_t u; memcpy(&u, &f, 4); return (u & 0x7F800000u) != 0x7F800000u; }

LUM_HISTORY_FN float history_dot(HistoryV3 a, HistoryV3 b) {
  const float tx = a.x * b.x;
  const float ty = a.y * b.y;
  const float tz = a.z * b.z;
  const float s = tx + ty;
  return s + tz;
}

LUM_HISTORY_FN HistoryV3 history_rotate(float qx, float qy, float qz, float qw, HistoryV3 v) {
  const HistoryV3 u = {qx, qy, qz};
  const float duv = history_dot(u, v), duu = history_dot(u, u);
  const float ax = u.y * v.z, bx = u.z * v.y;
  const float ay = u.z * v.x, by = u.x * v.z;
  const float az = u.x * v.y, bz = u.y * v.x;
  const HistoryV3 cr = {ax - bx, ay - by, az - bz};
  const float t = 2.0f * duv;
  const float ww = qw * qw;
  const float k = ww - duu;
  const float m = 2.0f * qw;
  HistoryV3 r;
  { const float p0 = u.x * t, p1 = v.x * k, p2 = cr.x * m; const float s = p0 + p1; r.x = s + p2; }
  { const float p0 = u.y * t, p1 = v.y * k, p2 = cr.y * m; const float s = p0 + p1; r.y = s + p2; }
  { const float p0 = u.z * t, p1 = v.z * k, p2 = cr.z * m; const float s = p0 + p1; r.z = s + p2; }
  return r;
}

struct HistoryFrame { float step, vfov; };
LUM_HISTORY_FN HistoryFrame history_frame(const HistoryKey& key) {
  const float q = key.fov / (float) key.width;
  const float step = 2.0f * q;
  const float sh = step * (float) key.height;
  return HistoryFrame{step, sh * 0.5f};
}

LUM_HISTORY_FN HistoryV3 history_centre_ray(const HistoryKey& key, uint32_t px, uint32_t py) {
  const HistoryFrame f = history_frame(key);
  const float cx = (float) px + 0.5f, cy = (float) py + 0.5f;
  const float mx = f.step * cx, my = f.step * cy;
  const float sx = key.fov - mx;
  const float sy = my - f.vfov;
  const HistoryV3 c = {-sx, -sy, -1.0f};
  const float l = sqrtf(history_dot(c, c));
  const HistoryV3 n = {c.x / l, c.y / l, c.z / l};
  return history_rotate(key.rot[0], key.rot[1], key.rot[2], key.rot[3], n);
}

// v: relative to the key's camera. False: behind it (or not a number).
LUM_HISTORY_FN bool history_project(const HistoryKey& key, HistoryV3 v, float& fx, float& fy) {
  const HistoryV3 dc = history_rotate(-key.rot[0], -key.rot[1], -key.rot[2], key.rot[3], v);
  fx = 0.0f; fy = 0.0f;
  if (!(dc.z < 0.0f)) return false;
  const HistoryFrame f = history_frame(key);
  const float rx = dc.x / dc.z, ry = dc.y / dc.z;
  const float ax = key.fov - rx;
  const float ay = ry + f.vfov;
  const float bx = ax / f.step, by = ay / f.step;
  fx = bx - 0.5f; fy = by - 0.5f;
  return true;
}

// One pixel of the carried plane. shown_at(x, y) / guide_at(x, y): the old state's records, asked only for taps inside the old frame. Returns the class.
template <typename ShownAt, typename GuideAt>
LUM_HISTORY_FN uint32_t history_reproject_pixel(const HistoryKey& now, const HistoryKey& old, const HistorySettings& st, uint32_t px, uint32_t py, HistoryV3 n_cur, float d_cur,
                                                ShownAt shown_at, GuideAt guide_at, HistoryRec& out) {
  out = HistoryRec{0.0f, 0.0f, 0.0f, 0.0f};
  const HistoryV3 dir = history_centre_ray(now, px, py);
  const bool surface = d_cur >= 0.0f;
  HistoryV3 v = dir;
  float r = 0.0f;
  if (surface) {
    const float ex = dir.x * d_cur, ey = dir.y * d_cur, ez = dir.z * d_cur;
    const float X = now.pos[0] + ex, Y = now.pos[1] + ey, Z = now.pos[2] + ez;
    v = HistoryV3{X - old.pos[0], Y - old.pos[1], Z - old.pos[2]};
    r = sqrtf(history_dot(v, v));
  }
  float fx, fy;
  if (!history_project(old, v, fx, fy)) return kHistoryOff;
  if (!(fx >= -1.0f && fx < (float) old.width && fy >= -1.0f && fy < (float) old.height)) return kHistoryOff;
  const float x0f = floorf(fx), y0f = floorf(fy);
  const int32_t x0 = (int32_t) x0f, y0 = (int32_t) y0f;
  const float tx = fx - x0f, ty = fy - y0f;
  const float ux = 1.0f - tx, uy = 1.0f - ty;
  const float tol = st.depth_tolerance * r;
  float ws = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f;
#if defined(__HIPCC__)
  _Pragma("unroll")
#endif
  for (uint32_t k = 0; k < 4u; k++) {
    const int32_t x = x0 + (int32_t) (k & 1u), y = y0 + (int32_t) (k >> 1);
    const float w = ((k & 1u) ? tx : ux) * ((k >> 1) ? ty : uy);
    if (x < 0 || y < 0 || x >= (int32_t) old.width || y >= (int32_t) old.height) continue;
    const HistoryRec g = guide_at((uint32_t) x, (uint32_t) y);
    if (surface) {
      if (!(g.w >= 0.0f)) continue;
      const float dd = g.w - r;
      const float ad = dd < 0.0f ? -dd : dd;
      if (!(ad <= tol)) continue;
      if (!(history_dot(n_cur, HistoryV3{g.x, g.y, g.z}) >= st.normal_threshold)) continue;
    }
    else if (!(g.w < 0.0f)) continue;
    const HistoryRec s = shown_at((uint32_t) x, (uint32_t) y);
    if (!(history_finite(s.x) && history_finite(s.y) && history_finite(s.z) && history_finite(s.w) && s.w > 0.0f)) continue;
    ws = ws + w;
    const float pr = w * s.x, pg = w * s.y, pb = w * s.z, pw = w * s.w;
    sr = sr + pr; sg = sg + pg; sb = sb + pb; sw = sw + pw;
  }
  if (!(ws > 0.0f)) return kHistoryRejected;
  const float q = sw / ws;
  const float m = q < st.max_history ? q : st.max_history;
  out = HistoryRec{sr / ws, sg / ws, sb / ws, m * ws};
  return kHistoryCarried;
}

// Step 3's clamp of one channel's carried value v to the neighbourhood [xa, xb] x [ya, yb] of cur.
template <typename CurAt>
LUM_HISTORY_FN float history_clamp_channel(float clamp_sigma, uint32_t xa, uint32_t xb, uint32_t ya, uint32_t yb, uint32_t ch, float v, CurAt cur_at) {
  const float k = (float) ((xb - xa + 1u) * (yb - ya + 1u));
  float s = 0.0f;
  for (uint32_t yy = ya; yy <= yb; yy++)
    for (uint32_t xx = xa; xx <= xb; xx++) s = s + cur_at(xx, yy, ch);
  const float mean = s / k;
  float q = 0.0f;
  for (uint32_t yy = ya; yy <= yb; yy++)
    for (uint32_t xx = xa; xx <= xb; xx++) { const float d = cur_at(xx, yy, ch) - mean; const float dd = d * d; q = q + dd; }
  const float sigma = sqrtf(q / k);
  const float e = clamp_sigma * sigma;
  const float lo = mean - e, hi = mean + e;
  return v < lo ? lo : (v > hi ? hi : v);
}

// One pixel of the blend. cur_at(x, y, channel): the result image, asked for (x, y) itself and, with the clamp, for its neighbours inside the frame.
// shown: the pixel's new value and the state's weight. Returns false where the image keeps cur's bits (cases 1 and 2).
template <typename CurAt>
LUM_HISTORY_FN bool history_blend_pixel(const HistorySettings& st, uint32_t width, uint32_t height, uint32_t x, uint32_t y, float N, HistoryRec carried, CurAt cur_at, HistoryRec& shown) {
  const float cr = cur_at(x, y, 0u), cg = cur_at(x, y, 1u), cb = cur_at(x, y, 2u);
  shown = HistoryRec{cr, cg, cb, 0.0f};
  if (!(history_finite(cr) && history_finite(cg) && history_finite(cb))) return false;
  shown.w = N;
  if (!(carried.w > 0.0f)) return false;
  float c0 = carried.x, c1 = carried.y, c2 = carried.z;
  if (st.clamp_sigma > 0.0f) {
    const uint32_t xa = x > 0u ? x - 1u : x, xb = x + 1u < width ? x + 1u : x, ya = y > 0u ? y - 1u : y, yb = y + 1u < height ? y + 1u : y;
    c0 = history_clamp_channel(st.clamp_sigma, xa, xb, ya, yb, 0u, c0, cur_at);
    c1 = history_clamp_channel(st.clamp_sigma, xa, xb, ya, yb, 1u, c1, cur_at);
    c2 = history_clamp_channel(st.clamp_sigma, xa, xb, ya, yb, 2u, c2, cur_at);
  }
  const float W = carried.w;
  const float den = W + N;
  { const float a = W * c0, b = N * cr; const float n = a + b; shown.x = n / den; }
  { const float a = W * c1, b = N * cg; const float n = a + b; shown.y = n / den; }
  { const float a = W * c2, b = N * cb; const float n = a + b; shown.z = n / den; }
  shown.w = den;
  return true;
}

}  // namespace lum

#if defined(__HIP_PLATFORM_AMD__) && !defined(LUM_HISTORY_HOST_ONLY)

#include <hip/hip_runtime_api.h>

#include <vector>

#include "device_buffer.h"

#pragma GCC visibility push(hidden)

namespace lum {

// A context's history: 32 bytes of state and 16 bytes of carried plane per pixel, allocated at the first blend, freed by lumc_history_release and with the context.
struct History {
  HistorySettings settings = {0u, 32.0f, 0.02f, 0.9f, 0.0f};
  DeviceBuffer<HistoryRec> shown, guide;  // the state, one record per pixel each
  DeviceBuffer<HistoryRec> carried;       // {C, W} of the current accumulation
  DeviceBuffer<float> cur;                // with the clamp: the image as it came, whose neighbourhoods the blend reads while it writes the image
  DeviceBuffer<uint32_t> d_stats;         // k_history_reproject's counters, kHistoryStatWords of them
  HistoryKey key{};                       // what the state was shown from
  HistoryKey carried_key{};               // what the carried plane was made for: a blend from another camera is refused
  bool has_state = false, has_carried = false;
  uint64_t carries = 0, blends = 0, drops = 0;
  const char* dropped_why = nullptr;      // the last drop's reason
  // launch stamps of its own under lumc_set_profiling ([0] carry, [1] blend): the context's categories are counted by existing callers
  struct Stamp { hipEvent_t a, b; int what; };
  std::vector<Stamp> stamps;
  double ms[2] = {0.0, 0.0};
  uint32_t launches[2] = {0u, 0u};
  size_t pixels() const { return shown.count(); }
  History() = default;
  History(const History&) = delete;
  History& operator=(const History&) = delete;
  ~History() { for (Stamp& s : stamps) { (void) hipEventDestroy(s.a); (void) hipEventDestroy(s.b); } }
};

// k_history_reproject: the old state into `now`; d_guides are the context's guide planes [albedo 3 | normal 3 | depth] of `now`'s frame. d_stats (kHistoryStatWords,
// zeroed by the caller): stripe k's words 0 .. 2 += pixels carried, rejected, off. Asynchronous, as the one below.
hipError_t history_reproject_launch(const HistoryKey& now, const HistoryKey& old, const HistorySettings& st, const float* d_guides, const HistoryRec* d_shown, const HistoryRec* d_guide,
                                    HistoryRec* d_carried, uint32_t* d_stats, hipStream_t stream);
// k_history_blend on a planar image [3][width * height]; d_cur: where the kernel reads the image it blends (d_image itself without the clamp, a copy of it with
// the clamp); d_carried may be null (nothing carried).
hipError_t history_blend_launch(const HistorySettings& st, uint32_t width, uint32_t height, uint32_t uniform_samples, const float* d_cur, const HistoryRec* d_carried, const float* d_guides,
                                float* d_image, HistoryRec* d_shown, HistoryRec* d_guide, hipStream_t stream);

}  // namespace lum

#pragma GCC visibility pop
#endif
