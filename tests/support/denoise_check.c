/* Plain-C restatement of the denoiser's filter (luminary_amd/csrc/device/dev_denoise.h, exact flavour) for tests/test_denoise.py: prepare, a-trous and
 * finish with the same operations in the same order, IEEE float without contraction (built with -ffp-contract=off). log2 and exp2 come from the test
 * oracle (oracle_log2, oracle_exp2), which restates the exact flavour's polynomials. Planes are laid out as on the device: image / first moment
 * [R|G|B], guides [albedo r g b | normal x y z | depth], depth < 0 where nothing was hit. `samples`: one count per pixel. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

float oracle_log2(float x);
float oracle_exp2(float x);

typedef struct { float x, y, z, w; } F4;
typedef struct { uint32_t x, y, z, w; } U4;
typedef struct { float x, y, z; } V;

static uint32_t fbits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float bitsf(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static float lum(float r, float g, float b) { return 0.212655f * r + 0.715158f * g + 0.072187f * b; }
static float dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

static uint32_t pack_normal(V n) {
  const float s = fabsf(n.x) + fabsf(n.y) + fabsf(n.z);
  float px = n.x / s, py = n.y / s;
  if (n.z < 0.0f) {
    const float qx = (1.0f - fabsf(py)) * ((px >= 0.0f) ? 1.0f : -1.0f), qy = (1.0f - fabsf(px)) * ((py >= 0.0f) ? 1.0f : -1.0f);
    px = qx; py = qy;
  }
  const int ix = (int) rintf(fminf(fmaxf(px, -1.0f), 1.0f) * 32767.0f), iy = (int) rintf(fminf(fmaxf(py, -1.0f), 1.0f) * 32767.0f);
  return ((uint32_t) ix & 0xFFFFu) | ((uint32_t) iy << 16);
}
static V unpack_normal(uint32_t packed) {
  float px = (float) (int) (int16_t) (packed & 0xFFFFu) * (1.0f / 32767.0f), py = (float) (int) (int16_t) (packed >> 16) * (1.0f / 32767.0f);
  const float z = (1.0f - fabsf(px)) - fabsf(py);
  if (z < 0.0f) {
    const float qx = (1.0f - fabsf(py)) * ((px >= 0.0f) ? 1.0f : -1.0f), qy = (1.0f - fabsf(px)) * ((py >= 0.0f) ? 1.0f : -1.0f);
    px = qx; py = qy;
  }
  const float s = 1.0f / sqrtf(px * px + py * py + z * z);
  V r = {px * s, py * s, z * s};
  return r;
}

/* for the tests of the packing itself */
void dn_normal_roundtrip(const float in[3], float out[3]) {
  V n = {in[0], in[1], in[2]};
  const V r = unpack_normal(pack_normal(n));
  out[0] = r.x; out[1] = r.y; out[2] = r.z;
}

static float albedo_of(const float* guides, uint32_t n, uint32_t c, uint32_t i) { return fmaxf(guides[c * n + i], 1e-3f); }

static void prepare(uint32_t w, uint32_t h, const float* fm, const float* sm, const uint32_t* samples, const float* image, const float* guides, F4* a, U4* b) {
  const uint32_t n = w * h;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t y = i / w, x = i - y * w;
    const float ar = albedo_of(guides, n, 0, i), ag = albedo_of(guides, n, 1, i), ab = albedo_of(guides, n, 2, i);
    float variance = 0.0f;
    if (samples[i] > 0u) {
      const float inv_n = 1.0f / (float) samples[i];
      const float r1 = fm[i] * inv_n, g1 = fm[n + i] * inv_n, b1 = fm[2 * n + i] * inv_n;
      const float lum2 = sm[i] * inv_n;
      const float lum_sq = lum(r1 * r1, g1 * g1, b1 * b1);
      const float la = lum(ar, ag, ab);
      variance = (fmaxf(lum2 - lum_sq, 0.0f) * inv_n) / (la * la);
    }
    a[i].x = image[i] / ar; a[i].y = image[n + i] / ag; a[i].z = image[2 * n + i] / ab; a[i].w = variance;
    const float depth = guides[6 * n + i];
    U4 rec = {0u, 0u, 0u, 0u};
    if (depth >= 0.0f) {
      V nrm = {guides[3 * n + i], guides[4 * n + i], guides[5 * n + i]};
      const float len2 = dot(nrm, nrm);
      const float inv = (len2 > 0.0f) ? 1.0f / sqrtf(len2) : 0.0f;
      V unit = {0.0f, 0.0f, 1.0f};
      if (len2 > 0.0f) { unit.x = nrm.x * inv; unit.y = nrm.y * inv; unit.z = nrm.z * inv; }
      rec.x = pack_normal(unit);
      const uint32_t xl = (x > 1u ? x : 1u) - 1u, xr = (x + 1u < w - 1u) ? x + 1u : w - 1u, yl = (y > 1u ? y : 1u) - 1u, yr = (y + 1u < h - 1u) ? y + 1u : h - 1u;
      float zl = guides[6 * n + xl + y * w], zr = guides[6 * n + xr + y * w], zd = guides[6 * n + x + yl * w], zu = guides[6 * n + x + yr * w];
      zl = (zl >= 0.0f) ? zl : depth; zr = (zr >= 0.0f) ? zr : depth; zd = (zd >= 0.0f) ? zd : depth; zu = (zu >= 0.0f) ? zu : depth;
      const float gx = (xr > xl) ? (zr - zl) / (float) (xr - xl) : 0.0f, gy = (yr > yl) ? (zu - zd) / (float) (yr - yl) : 0.0f;
      rec.y = fbits(depth); rec.z = fbits(fmaxf(fabsf(gx), fabsf(gy))); rec.w = 1u;
    }
    b[i] = rec;
  }
}

static int same_surface(int hit_p, V n_p, U4 bq) {
  if (((bq.w & 1u) != 0u) != (hit_p != 0)) return 0;
  return !hit_p || dot(n_p, unpack_normal(bq.x)) > 0.0f;
}

static F4 pixel(uint32_t w, uint32_t h, uint32_t step, float sigma_l, float sigma_n, float sigma_z, const F4* a, const U4* b, uint32_t x, uint32_t y) {
  const F4 ap = a[x + y * w];
  const U4 bp = b[x + y * w];
  const int hit = (bp.w & 1u) != 0u;
  V n_p = {0.0f, 0.0f, 0.0f};
  if (hit) n_p = unpack_normal(bp.x);
  const float z_p = bitsf(bp.y), grad_p = bitsf(bp.z);
  float gsum = 0.0f, ksum = 0.0f;
  for (int dy = -1; dy <= 1; dy++)
    for (int dx = -1; dx <= 1; dx++) {
      const int qx = (int) x + dx, qy = (int) y + dy;
      if (qx < 0 || qy < 0 || qx >= (int) w || qy >= (int) h) continue;
      const float k = (dx == 0 && dy == 0) ? 0.25f : (dx == 0 || dy == 0) ? 0.125f : 0.0625f;
      F4 aq = ap;
      if (dx != 0 || dy != 0) {
        aq = a[qx + qy * (int) w];
        if (!same_surface(hit, n_p, b[qx + qy * (int) w])) continue;
      }
      gsum += k * aq.w; ksum += k;
    }
  const float g = gsum / ksum;
  if (g == 0.0f) return ap;
  const float l_p = lum(ap.x, ap.y, ap.z);
  const float den_l = sigma_l * sqrtf(g) + 1e-6f;
  const float fstep = (float) step;
  float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f;
  for (int dy = -2; dy <= 2; dy++)
    for (int dx = -2; dx <= 2; dx++) {
      const int qx = (int) x + dx * (int) step, qy = (int) y + dy * (int) step;
      if (qx < 0 || qy < 0 || qx >= (int) w || qy >= (int) h) continue;
      const float hx = (dx == 0) ? 0.375f : (dx == 1 || dx == -1) ? 0.25f : 0.0625f, hy = (dy == 0) ? 0.375f : (dy == 1 || dy == -1) ? 0.25f : 0.0625f;
      float wt = hx * hy;
      F4 aq = ap;
      if (dx != 0 || dy != 0) {
        aq = a[qx + qy * (int) w];
        const U4 bq = b[qx + qy * (int) w];
        if (((bq.w & 1u) != 0u) != (hit != 0)) continue;
        float e = 0.0f;
        if (hit) {
          const float d = fminf(dot(n_p, unpack_normal(bq.x)), 1.0f);
          if (!(d > 0.0f)) continue;
          const float len = sqrtf((float) (dx * dx + dy * dy)) * fstep;
          e = sigma_n * oracle_log2(d) - (fabsf(z_p - bitsf(bq.y)) / (sigma_z * grad_p * len + 1e-6f)) * 1.44269504f;
        }
        e = e - (fabsf(l_p - lum(aq.x, aq.y, aq.z)) / den_l) * 1.44269504f;
        if (!(e >= -30.0f)) continue;
        wt = wt * oracle_exp2(e);
      }
      sw += wt; sr += wt * aq.x; sg += wt * aq.y; sb += wt * aq.z; sv += (wt * wt) * aq.w;
    }
  F4 out = {sr / sw, sg / sw, sb / sw, sv / (sw * sw)};
  return out;
}

/* image: [3 * w * h], filtered in place. variance_out (may be NULL): the filtered variance plane. Returns 0, or 1 without memory. */
int dn_denoise(uint32_t w, uint32_t h, uint32_t iterations, float sigma_l, float sigma_n, float sigma_z, const float* fm, const float* sm, const uint32_t* samples,
               const float* guides, float* image, float* variance_out) {
  const uint32_t n = w * h;
  F4* a0 = malloc(sizeof(F4) * n);
  F4* a1 = malloc(sizeof(F4) * n);
  U4* b = malloc(sizeof(U4) * n);
  if (!a0 || !a1 || !b) { free(a0); free(a1); free(b); return 1; }
  prepare(w, h, fm, sm, samples, image, guides, a0, b);
  if (iterations > 6u) iterations = 6u;
  F4 *cur = a0, *next = a1;
  for (uint32_t i = 0; i < iterations; i++) {
    for (uint32_t y = 0; y < h; y++)
      for (uint32_t x = 0; x < w; x++) next[x + y * w] = pixel(w, h, 1u << i, sigma_l, sigma_n, sigma_z, cur, b, x, y);
    F4* t = cur; cur = next; next = t;
  }
  for (uint32_t i = 0; i < n; i++) {
    const float ar = albedo_of(guides, n, 0, i), ag = albedo_of(guides, n, 1, i), ab = albedo_of(guides, n, 2, i);
    if (variance_out) variance_out[i] = cur[i].w;
    if (cur[i].x == image[i] / ar && cur[i].y == image[n + i] / ag && cur[i].z == image[2 * n + i] / ab) continue;
    image[i] = cur[i].x * ar; image[n + i] = cur[i].y * ag; image[2 * n + i] = cur[i].z * ab;
  }
  free(a0); free(a1); free(b);
  return 0;
}
