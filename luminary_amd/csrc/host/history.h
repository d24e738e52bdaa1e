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
//
// Motion (lumc_set_history_motion): the state carried across rigid moves of instances too. Off by default; nothing below exists while it is off.
//
// Owner plane, one uint32 per pixel: the id of the first hit of sample id 0 of the guide render, matte.h's matte_sample_id(matte_classify(hit), hit) - an
//   instance id, or kMatteIdMiss / kMatteIdOcean / kMatteIdParticle (the reserved ids, >= kHistoryOwnerReserved). A pixel without a path holds kMatteIdEmpty,
//   reserved as well. The state holds the plane of the frame it was shown with, the context the current frame's: 4 + 4 bytes per pixel.
//
// Instance motion record, HistoryMotion, 128 bytes (one cache line) per instance, history_motion_record(old8, new8) from the instance's two 8-word transforms
//   as the scene view holds them (dev_math.h Transform: translation 3, scale 3, the quaternion in 4 x 16 bits) - the binary64 part, once per instance:
//   SAME   the eight words are bitwise equal. Every other field of the record is zero.
//   VOID   a translation or scale word of either key is not finite (the two quaternion words are no floats), or the world->object matrix of either key has a
//          determinant that is zero or not finite (instance_world_box's test: such an instance cannot be hit), or an entry of L or NL below is not finite
//          after its rounding. Every other field is zero.
//   MOVED  otherwise: t_new, t_old (the translations), L = Mo^-1 Mn and NL = (Mn^-1 Mo)^T = (L^-1)^T, row-major.
//   M of a key is its world->object matrix as the ray kernels trace with it, bvh_build.cpp's instance_inverse_rows in binary32, operation for operation:
//     u = (1 - lo16(w6) c, 1 - hi16(w6) c, 1 - lo16(w7) c), s = hi16(w7) c - 1 with c = 1.0f / 32767 (the unnormalised conjugate), i = (1 / scale.x, 1 / scale.y, 1 / scale.z);
//     per column j: v = (e_j.x i.x, e_j.y i.y, e_j.z i.z) (products with 0 and 1 as they come), duv = dot(u, v), duu = dot(u, u), cr = cross(u, v), k0 = 2 duv,
//     k1 = s s - duu, k2 = 2 s, col_j = (u k0 + v k1) + cr k2 per component; M[i][j] = col_j[i].
//   In binary64 then, as instance_world_box: det(M) = (m00 (m11 m22 - m12 m21) - m01 (m10 m22 - m12 m20)) + m02 (m10 m21 - m11 m20); the inverse F by cofactors, each
//     over det: F00 = (m11 m22 - m12 m21) / det, F01 = (m02 m21 - m01 m22) / det, F02 = (m01 m12 - m02 m11) / det, F10 = (m12 m20 - m10 m22) / det,
//     F11 = (m00 m22 - m02 m20) / det, F12 = (m02 m10 - m00 m12) / det, F20 = (m10 m21 - m11 m20) / det, F21 = (m01 m20 - m00 m21) / det, F22 = (m00 m11 - m01 m10) / det.
//     A product A B has (A B)[i][j] = (A[i][0] B[0][j] + A[i][1] B[1][j]) + A[i][2] B[2][j]. L = Fo Mn, NL[i][j] = (Fn Mo)[j][i]; each entry rounded once to binary32.
//   The maps are the inverse of what the ray kernels trace with, not xf_point: qapply with the unnormalised quantised quaternion is not the inverse of qapply
//   with its conjugate, and the record has to land where the traced geometry was.
//
// Class of an owner id o, given `count` records: o >= kHistoryOwnerReserved: SAME (nothing of a sky, an ocean or a particle moves with an instance);
//   otherwise o >= count: VOID; otherwise the record's.
//
// Reproject, motion form (history_reproject_pixel_motion): steps 1 to 6 with these changes, o the pixel's owner in the current plane, c its class.
//   0. c is VOID: C = 0, W = 0, class REJECTED; no tap is read.
//   1. c is MOVED and the pixel is a surface: after X = pos_new + dir d_cur, d = X - t_new, Ld_i = (L[i][0] d.x + L[i][1] d.y) + L[i][2] d.z (mat_row_apply's order),
//      X_old = t_old + Ld per component, v = X_old - pos_old, r = sqrt(dot(v, v)). The normal compared with the old guides is m = NL n_cur (the same order) over its
//      length l = sqrt(dot(m, m)), per component; not (l > 0) or l not finite: C = 0, W = 0, class REJECTED. Otherwise (SAME, or no surface): step 1 as it is.
//   4. a tap that passed the tests of step 4 on its guide record is refused all the same when its old owner (the state's plane) differs from o and either of
//      the two owners' classes is MOVED or VOID: a mover's pixel takes nothing from the background it now covers, a background pixel nothing from where the mover
//      was, whatever depth and normal say. Only then is its shown record read.
//   6. the cap is motion_max_history instead of max_history where c is MOVED: a moved object's lighting has changed even where its surface has not.
//   With every record SAME and every owner below count or reserved, this is the form above, bit for bit.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define LUM_HISTORY_FN __host__ __device__ __forceinline__
#define LUM_HISTORY_UNROLL _Pragma("unroll")
#else
#define LUM_HISTORY_FN inline
#define LUM_HISTORY_UNROLL
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

// ---- motion: the record of an instance, the class of an owner, the pixel ----
enum : uint32_t { kHistoryMotionSame = 0, kHistoryMotionMoved = 1, kHistoryMotionVoid = 2 };
constexpr uint32_t kHistoryOwnerReserved = 0xFFFFFFFCu;  // matte.h's kMatteIdParticle, the lowest reserved id (history.cpp asserts it)
struct alignas(128) HistoryMotion { uint32_t cls; float t_new[3], t_old[3], L[9], NL[9]; uint32_t pad[7]; };
// k_history_reproject_motion's two counters beside {carried, rejected, off} in a stripe: pixels whose owner is MOVED, and those of them that carried
constexpr uint32_t kHistoryStatMoved = 3, kHistoryStatMovedCarried = 4;

struct HistoryM3 { double m[3][3]; };
// instance_inverse_rows (bvh_build.cpp) on the 8 words of a transform, in binary32; false: a translation or scale word is not finite
LUM_HISTORY_FN bool history_instance_matrix(const float* p, HistoryM3& out) {
  bool finite = true;
  LUM_HISTORY_UNROLL
  for (uint32_t k = 0; k < 6u; k++) finite = finite && history_finite(p[k]);
  if (!finite) return false;
  uint32_t a, b;
  memcpy(&a, p + 6, 4); memcpy(&b, p + 7, 4);
  const float c = 1.0f / 32767.0f;
  const float ax = (float) (a & 0xFFFFu) * c, ay = (float) (a >> 16) * c, az = (float) (b & 0xFFFFu) * c, aw = (float) (b >> 16) * c;
  const HistoryV3 u = {1.0f - ax, 1.0f - ay, 1.0f - az};
  const float s = aw - 1.0f;
  const float ix = 1.0f / p[3], iy = 1.0f / p[4], iz = 1.0f / p[5];
  const float duu = history_dot(u, u);
  const float ss = s * s;
  const float k1 = ss - duu, k2 = 2.0f * s;
  LUM_HISTORY_UNROLL
  for (uint32_t j = 0; j < 3u; j++) {
    const HistoryV3 v = {(j == 0u ? 1.0f : 0.0f) * ix, (j == 1u ? 1.0f : 0.0f) * iy, (j == 2u ? 1.0f : 0.0f) * iz};
    const float duv = history_dot(u, v);
    const float ax2 = u.y * v.z, bx2 = u.z * v.y;
    const float ay2 = u.z * v.x, by2 = u.x * v.z;
    const float az2 = u.x * v.y, bz2 = u.y * v.x;
    const HistoryV3 cr = {ax2 - bx2, ay2 - by2, az2 - bz2};
    const float k0 = 2.0f * duv;
    { const float p0 = u.x * k0, p1 = v.x * k1, p2 = cr.x * k2; const float t = p0 + p1; out.m[0][j] = (double) (t + p2); }
    { const float p0 = u.y * k0, p1 = v.y * k1, p2 = cr.y * k2; const float t = p0 + p1; out.m[1][j] = (double) (t + p2); }
    { const float p0 = u.z * k0, p1 = v.z * k1, p2 = cr.z * k2; const float t = p0 + p1; out.m[2][j] = (double) (t + p2); }
  }
  return true;
}
LUM_HISTORY_FN double history_sub2(double a, double b, double c, double d) { const double x = a * b, y = c * d; return x - y; }
// the inverse by cofactors over the determinant, instance_world_box's expressions; false: the determinant is zero or not finite
LUM_HISTORY_FN bool history_inverse3(const HistoryM3& A, HistoryM3& F) {
  const double (*m)[3] = A.m;
  const double c0 = history_sub2(m[1][1], m[2][2], m[1][2], m[2][1]), c1 = history_sub2(m[1][0], m[2][2], m[1][2], m[2][0]), c2 = history_sub2(m[1][0], m[2][1], m[1][1], m[2][0]);
  const double d0 = m[0][0] * c0, d1 = m[0][1] * c1, d2 = m[0][2] * c2;
  const double d01 = d0 - d1;
  const double det = d01 + d2;
  const double mag = det < 0.0 ? -det : det;
  if (!(mag > 0.0) || !(mag <= 1.7976931348623157e308)) return false;
  F.m[0][0] = c0 / det;
  F.m[0][1] = history_sub2(m[0][2], m[2][1], m[0][1], m[2][2]) / det;
  F.m[0][2] = history_sub2(m[0][1], m[1][2], m[0][2], m[1][1]) / det;
  F.m[1][0] = history_sub2(m[1][2], m[2][0], m[1][0], m[2][2]) / det;
  F.m[1][1] = history_sub2(m[0][0], m[2][2], m[0][2], m[2][0]) / det;
  F.m[1][2] = history_sub2(m[0][2], m[1][0], m[0][0], m[1][2]) / det;
  F.m[2][0] = c2 / det;
  F.m[2][1] = history_sub2(m[0][1], m[2][0], m[0][0], m[2][1]) / det;
  F.m[2][2] = history_sub2(m[0][0], m[1][1], m[0][1], m[1][0]) / det;
  return true;
}
LUM_HISTORY_FN double history_mul3(const HistoryM3& A, const HistoryM3& B, uint32_t i, uint32_t j) {
  const double x = A.m[i][0] * B.m[0][j], y = A.m[i][1] * B.m[1][j], z = A.m[i][2] * B.m[2][j];
  const double s = x + y;
  return s + z;
}

LUM_HISTORY_FN HistoryMotion history_motion_record(const float* old8, const float* new8) {
  HistoryMotion r = {};
  bool same = true;
  LUM_HISTORY_UNROLL
  for (uint32_t k = 0; k < 8u; k++) { uint32_t a, b; memcpy(&a, old8 + k, 4); memcpy(&b, new8 + k, 4); same = same && a == b; }
  if (same) { r.cls = kHistoryMotionSame; return r; }
  r.cls = kHistoryMotionVoid;
  HistoryM3 Mo, Mn, Fo, Fn;
  if (!history_instance_matrix(old8, Mo) || !history_instance_matrix(new8, Mn)) return r;
  if (!history_inverse3(Mo, Fo) || !history_inverse3(Mn, Fn)) return r;
  float L[9], NL[9];
  bool finite = true;
  LUM_HISTORY_UNROLL
  for (uint32_t i = 0; i < 3u; i++)
    LUM_HISTORY_UNROLL
    for (uint32_t j = 0; j < 3u; j++) {
      L[3u * i + j] = (float) history_mul3(Fo, Mn, i, j);
      NL[3u * i + j] = (float) history_mul3(Fn, Mo, j, i);
      finite = finite && history_finite(L[3u * i + j]) && history_finite(NL[3u * i + j]);
    }
  if (!finite) return r;
  r.cls = kHistoryMotionMoved;
  LUM_HISTORY_UNROLL
  for (uint32_t k = 0; k < 3u; k++) { r.t_new[k] = new8[k]; r.t_old[k] = old8[k]; }
  LUM_HISTORY_UNROLL
  for (uint32_t k = 0; k < 9u; k++) { r.L[k] = L[k]; r.NL[k] = NL[k]; }
  return r;
}

// class_of(id): the class word of record `id`, asked only for id < count
template <typename ClassOf>
LUM_HISTORY_FN uint32_t history_owner_class(uint32_t o, uint32_t count, ClassOf class_of) {
  if (o >= kHistoryOwnerReserved) return kHistoryMotionSame;
  if (o >= count) return kHistoryMotionVoid;
  return class_of(o);
}

LUM_HISTORY_FN float history_row_apply(float a, float b, float c, HistoryV3 v) {
  const float x = a * v.x, y = b * v.y, z = c * v.z;
  const float s = x + y;
  return s + z;
}

// One pixel of the carried plane, motion form. o: the pixel's owner in the current plane; owner_at(x, y): the state's plane; class_of(id), record_of(id): of
// record id < count, the latter asked only where o's class is MOVED. owner_moved: o's class is MOVED. Returns the class.
template <typename ShownAt, typename GuideAt, typename OwnerAt, typename ClassOf, typename RecordOf>
LUM_HISTORY_FN uint32_t history_reproject_pixel_motion(const HistoryKey& now, const HistoryKey& old, const HistorySettings& st, float motion_max_history, uint32_t px, uint32_t py,
                                                       HistoryV3 n_cur, float d_cur, uint32_t o, uint32_t count, ShownAt shown_at, GuideAt guide_at, OwnerAt owner_at, ClassOf class_of,
                                                       RecordOf record_of, HistoryRec& out, bool& owner_moved) {
  out = HistoryRec{0.0f, 0.0f, 0.0f, 0.0f};
  const uint32_t c = history_owner_class(o, count, class_of);
  owner_moved = c == kHistoryMotionMoved;
  if (c == kHistoryMotionVoid) return kHistoryRejected;
  const HistoryV3 dir = history_centre_ray(now, px, py);
  const bool surface = d_cur >= 0.0f;
  HistoryV3 v = dir;
  HistoryV3 n_cmp = n_cur;
  float r = 0.0f;
  if (surface) {
    const float ex = dir.x * d_cur, ey = dir.y * d_cur, ez = dir.z * d_cur;
    float X = now.pos[0] + ex, Y = now.pos[1] + ey, Z = now.pos[2] + ez;
    if (owner_moved) {
      const HistoryMotion m = record_of(o);
      const HistoryV3 d = {X - m.t_new[0], Y - m.t_new[1], Z - m.t_new[2]};
      const float lx = history_row_apply(m.L[0], m.L[1], m.L[2], d), ly = history_row_apply(m.L[3], m.L[4], m.L[5], d), lz = history_row_apply(m.L[6], m.L[7], m.L[8], d);
      X = m.t_old[0] + lx; Y = m.t_old[1] + ly; Z = m.t_old[2] + lz;
      const HistoryV3 nn = {history_row_apply(m.NL[0], m.NL[1], m.NL[2], n_cur), history_row_apply(m.NL[3], m.NL[4], m.NL[5], n_cur), history_row_apply(m.NL[6], m.NL[7], m.NL[8], n_cur)};
      const float l = sqrtf(history_dot(nn, nn));
      if (!(l > 0.0f) || !history_finite(l)) return kHistoryRejected;
      n_cmp = HistoryV3{nn.x / l, nn.y / l, nn.z / l};
    }
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
      if (!(history_dot(n_cmp, HistoryV3{g.x, g.y, g.z}) >= st.normal_threshold)) continue;
    }
    else if (!(g.w < 0.0f)) continue;
    const uint32_t oo = owner_at((uint32_t) x, (uint32_t) y);
    if (oo != o && (c != kHistoryMotionSame || history_owner_class(oo, count, class_of) != kHistoryMotionSame)) continue;
    const HistoryRec s = shown_at((uint32_t) x, (uint32_t) y);
    if (!(history_finite(s.x) && history_finite(s.y) && history_finite(s.z) && history_finite(s.w) && s.w > 0.0f)) continue;
    ws = ws + w;
    const float pr = w * s.x, pg = w * s.y, pb = w * s.z, pw = w * s.w;
    sr = sr + pr; sg = sg + pg; sb = sb + pb; sw = sw + pw;
  }
  if (!(ws > 0.0f)) return kHistoryRejected;
  const float q = sw / ws;
  const float cap = owner_moved ? motion_max_history : st.max_history;
  const float m = q < cap ? q : cap;
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
  // launch stamps of its own under lumc_set_profiling ([0] carry, [1] blend; motion: [2] k_history_owner, [3] k_history_motion, [4] k_history_reproject_motion):
  // the context's categories are counted by existing callers
  struct Stamp { hipEvent_t a, b; int what; };
  std::vector<Stamp> stamps;
  double ms[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  uint32_t launches[5] = {0u, 0u, 0u, 0u, 0u};
  // motion (lumc_set_history_motion): nothing of it is allocated while the switch is off
  struct Motion {
    uint32_t enabled = 0u;
    float max_history = 8.0f;                     // motion_max_history
    DeviceBuffer<uint32_t> owner_state, owner_cur;  // the owner planes: of the frame the state was shown with, of the current guide render
    DeviceBuffer<float4> snapshot;                // the scene's instance transforms as the state was shown with them, 2 per instance
    DeviceBuffer<HistoryMotion> records;          // of the last motion carry
    DeviceBuffer<uint32_t> d_counts;              // k_history_motion's counters {moved, same, void}, a line of their own
    uint32_t snapshot_instances = 0u, record_instances = 0u;
    bool has_snapshot = false, owner_cur_valid = false, last_carry = false;  // last_carry: the last carry took the motion form
    bool state_current = false;  // the state's plane and snapshot are a copy of the current ones: a later blend of the same accumulation copies nothing
    uint64_t carries = 0;
  } motion;
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
// k_history_owner: one thread per path of the closest-hit pass of sample id 0 (the first `*d_paths` entries of hit_id), as k_matte_accumulate reads them;
// d_owner [n] was preset to kMatteIdEmpty by the caller.
hipError_t history_owner_launch(const uint4* d_hit_id, const uint32_t* d_paths, uint32_t width, uint32_t n, uint32_t* d_owner, hipStream_t stream);
// k_history_motion: one thread per instance, old / new transforms (2 float4 each) -> records; d_counts[0 .. 2] (zeroed by the caller) += moved, same, void.
hipError_t history_motion_launch(const float4* d_old, const float4* d_new, uint32_t count, HistoryMotion* d_records, uint32_t* d_counts, hipStream_t stream);
// k_history_reproject_motion: history_reproject_launch with the two owner planes and `count` records; stripe words 3 and 4: kHistoryStatMoved, kHistoryStatMovedCarried.
hipError_t history_reproject_motion_launch(const HistoryKey& now, const HistoryKey& old, const HistorySettings& st, float motion_max_history, const float* d_guides,
                                           const HistoryRec* d_shown, const HistoryRec* d_guide, const uint32_t* d_owner, const uint32_t* d_old_owner, const HistoryMotion* d_records,
                                           uint32_t count, HistoryRec* d_carried, uint32_t* d_stats, hipStream_t stream);

}  // namespace lum

#pragma GCC visibility pop
#endif
