/* Plain-C restatement of the physical camera's ray (luminary_amd/csrc/device/dev_camera.h, exact flavour) for tests/test_physical_camera.py:
 * the same operations in the same order, IEEE float without contraction (built with -ffp-contract=off). Random numbers and sin/cos come from the
 * test oracle (oracle_random_2d, oracle_sincos), which restates the sampler and the exact flavour's polynomials. */
#include <math.h>
#include <stdint.h>
#include <string.h>

void oracle_random_2d(const uint32_t* bn, uint32_t target, uint32_t px, uint32_t py, uint32_t sample, uint32_t depth, uint32_t out[2]);
void oracle_sincos(float x, float out[2]);

/* == LumPhysicalCamera (include/lum_core.h) */
typedef struct {
  float aperture_point, aperture_radius, exit_pupil_point, exit_pupil_radius, image_plane_distance, sensor_width;
  uint32_t allow_reflections, num_interfaces;
  float iface[24][3];  /* radius, vertex, cylindrical radius */
  float media[25][3];  /* design ior, abbe, cylindrical radius */
} Lens;

typedef struct { float x, y, z; } V;
static V v(float x, float y, float z) { V r = {x, y, z}; return r; }
static V add(V a, V b) { return v(a.x + b.x, a.y + b.y, a.z + b.z); }
static V sub(V a, V b) { return v(a.x - b.x, a.y - b.y, a.z - b.z); }
static V scl(V a, float s) { return v(a.x * s, a.y * s, a.z * s); }
static float dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static float len(V a) { return sqrtf(dot(a, a)); }
static V norm(V a) { const float s = 1.0f / sqrtf(dot(a, a)); return v(a.x * s, a.y * s, a.z * s); }
static V cross(V a, V b) { return v(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
static V reflect(V V_, V n) { const float d = dot(V_, n); return norm(sub(scl(n, 2.0f * d), V_)); }
static V refract(V V_, V n, float r, int* tr) {
  if (r < 1.1920928955078125e-7f) { *tr = 0; return scl(V_, -1.0f); }
  const float d = fabsf(dot(n, V_));
  const float b = 1.0f - r * r * (1.0f - d * d);
  *tr = b < 0.0f;
  if (*tr) return reflect(V_, n);
  return norm(sub(scl(n, r * d - sqrtf(b)), scl(V_, r)));
}
static float saturate(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }
static float fresnel(V n, V V_, V refr, float ior) {
  const float NdotV = dot(V_, n), NdotT = -dot(refr, n);
  const float s1 = ior * NdotV, s2 = 1.0f * NdotT, p1 = ior * NdotT, p2 = 1.0f * NdotV;
  float rs = (s1 - s2) / (s1 + s2), rp = (p1 - p2) / (p1 + p2);
  rs *= rs; rp *= rp;
  return saturate(0.5f * (rs + rp));
}
static V qapply(const float q[4], V x) {
  const V u = v(q[0], q[1], q[2]);
  const float s = q[3];
  const float duv = dot(u, x), duu = dot(u, u);
  const V cr = cross(u, x);
  V r = scl(u, 2.0f * duv);
  r = add(r, scl(x, s * s - duu));
  r = add(r, scl(cr, 2.0f * s));
  return r;
}
static float unit_float(uint32_t x) { union { uint32_t u; float f; } c; c.u = 0x3F800000u | (x >> 9); return c.f - 1.0f; }

#define FLT_MAX_ 3.402823466e+38f
static const float kPi = 3.14159265358979323846f, kIorAir = 1.0003f;

static float sphere(V ray, V origin, V p, float r) {
  const V diff = sub(origin, p);
  const float d = dot(diff, ray);
  const float r2 = r * r;
  const float c = dot(diff, diff) - r2;
  const V k = sub(diff, scl(ray, d));
  const float disc = r2 - dot(k, k);
  if (disc < 0.0f) return FLT_MAX_;
  const float sd = sqrtf(disc);
  const float q = -d - copysignf(sd, d);
  const float t0 = c / q;
  if (t0 >= 0.0f) return t0;
  return (q >= 0.0f) ? q : FLT_MAX_;
}
static int aperture_blocks(const Lens* L, V o, V r, float dist) {
  const float t = (L->aperture_point - o.z) / r.z;
  if (t > 0.0f && t < dist) {
    const V h = add(o, scl(r, t));
    if (h.x * h.x + h.y * h.y > L->aperture_radius * L->aperture_radius) return 1;
  }
  return 0;
}
static int medium_cylinder(V* o, V* r, float* w, float dist, float cyl, float medium_ior) {
  if (cyl == FLT_MAX_) return 0;
  V cr = v(r->x, r->y, 0.0f);
  const float cl = len(cr);
  if (cl == 0.0f) return 0;
  cr = scl(cr, 1.0f / cl);
  float cd = sphere(cr, v(o->x, o->y, 0.0f), v(0.0f, 0.0f, 0.0f), cyl);
  cd *= 1.0f / cl;
  if (cd > 0.0f && cd < dist) {
    *o = add(*o, scl(*r, cd));
    const V n = norm(v(-o->x, -o->y, 0.0f));
    const float ior = medium_ior * (1.0f / kIorAir);
    const V V_ = scl(*r, -1.0f);
    int tr;
    const V refr = refract(V_, n, ior, &tr);
    const float f = (tr == 0) ? fresnel(n, V_, refr, ior) : 1.0f;
    *w *= f;
    *r = reflect(V_, n);
    return 1;
  }
  return 0;
}

/* The walk from the sensor (lens space, +z): returns the walk's weight and leaves the end point and direction in o, d (not flipped). */
float pc_lens_walk(const Lens* L, const uint32_t* bn, uint32_t px, uint32_t py, uint32_t sample, float o_io[3], float d_io[3]) {
  V o = v(o_io[0], o_io[1], o_io[2]), d = v(d_io[0], d_io[1], d_io[2]);
  float ior = kIorAir, cyl = FLT_MAX_, weight = 1.0f;
  int forward = 1, reflected = 0;
  const uint32_t n = L->num_interfaces;
  uint32_t it = 0;
  int32_t cur = 0;
  for (; it < 32u; it++) {
    const int32_t id = L->allow_reflections ? cur : (int32_t) it;
    const float* f = L->iface[id];
    const V center = v(0.0f, 0.0f, f[1] - f[0]);
    const float radius = fabsf(f[0]);
    int32_t move = 0;
    float t = sphere(d, o, center, radius);
    if (t == FLT_MAX_ || aperture_blocks(L, o, d, t)) weight = 0.0f;
    else {
      const int inside = len(sub(o, center)) < radius;
      int alive = 1;
      if (medium_cylinder(&o, &d, &weight, t, cyl, ior)) {
        t = sphere(d, o, center, radius);
        if (t == FLT_MAX_ || aperture_blocks(L, o, d, t)) { weight = 0.0f; alive = 0; }
      }
      if (alive) {
        const float* m = L->media[forward ? id + 1 : id];
        o = add(o, scl(d, t));
        if (o.x * o.x + o.y * o.y > f[2] * f[2]) weight = 0.0f;
        else {
          V nrm = norm(sub(o, center));
          if (inside) nrm = scl(nrm, -1.0f);
          const V V_ = scl(d, -1.0f);
          const float eta = ior / m[0];
          int tr;
          const V refr = refract(V_, nrm, eta, &tr);
          const V refl = reflect(V_, nrm);
          int allow_reflection = 0;
          if (L->allow_reflections) allow_reflection = (id != 0 || it != 0) && (!reflected || !forward);
          const int allow_refraction = id != 0 || it == 0;
          float w;
          int refracts;
          if (tr) { w = allow_reflection ? 1.0f : 0.0f; refracts = 0; }
          else {
            const float fr = fresnel(nrm, V_, refr, eta);
            if (allow_refraction && allow_reflection) {
              uint32_t q[2];
              oracle_random_2d(bn, 0u + it, px, py, sample, 0, q);
              w = 1.0f; refracts = unit_float(q[0]) >= fr;
            }
            else if (allow_reflection) { w = fr; refracts = 0; }
            else { w = 1.0f - fr; refracts = 1; }
          }
          weight *= w;
          d = refracts ? refr : refl;
          ior = refracts ? m[0] : ior;
          cyl = refracts ? m[2] : cyl;
          forward = refracts ? forward : !forward;
          reflected = refracts ? reflected : 1;
          move = forward ? 1 : -1;
        }
      }
    }
    cur += move;
    if ((uint32_t) cur >= n || cur < 0 || weight == 0.0f) break;
  }
  if (cur < 0 || (it == 32u && (uint32_t) cur <= n)) weight = 0.0f;
  o_io[0] = o.x; o_io[1] = o.y; o_io[2] = o.z;
  d_io[0] = d.x; d_io[1] = d.y; d_io[2] = d.z;
  return weight;
}

/* Sensor point and exit-pupil direction of a sample (lens space) and the sample's initial weight. */
float pc_sensor_sample(const Lens* L, const uint32_t* bn, uint32_t width, uint32_t height, uint32_t px, uint32_t py, uint32_t sample, float o[3], float d[3]) {
  uint32_t jq[2], rq[2];
  oracle_random_2d(bn, 63u, 0u, 0u, sample, 0u, jq);  /* kRndCameraJitter: the same for every pixel */
  const float jx = unit_float(jq[0]), jy = unit_float(jq[1]);
  const float step = 2.0f * (L->sensor_width / (float) width);
  const float vfov = step * (float) height * 0.5f;
  const V sensor = v(L->sensor_width - step * ((float) px + jx), -vfov + step * ((float) py + jy), -L->image_plane_distance);
  oracle_random_2d(bn, 33u, px, py, sample, 0u, rq);  /* kRndLens */
  const float rx = unit_float(rq[0]), ry = unit_float(rq[1]);
  const float alpha = rx * 2.0f * kPi, beta = sqrtf(ry) * L->exit_pupil_radius;
  float sc[2];
  oracle_sincos(alpha, sc);
  const V diff = sub(v(sc[1] * beta, sc[0] * beta, L->exit_pupil_point), sensor);
  const float dist = len(diff);
  const float area = L->exit_pupil_radius * L->exit_pupil_radius * kPi;
  const V dir = norm(diff);
  o[0] = sensor.x; o[1] = sensor.y; o[2] = sensor.z;
  d[0] = dir.x; d[1] = dir.y; d[2] = dir.z;
  return area * fabsf(dir.z) / (dist * dist);
}

/* Every camera ray of (samples x pixels), sample-major, in world space: what lumc_camera_rays returns. */
void pc_camera_rays(const Lens* L, const uint32_t* bn, uint32_t width, uint32_t height, const float pos[3], const float rot[4], float camera_scale,
                    const uint32_t* pixels, uint32_t n, uint32_t first_sample, uint32_t samples, float* out_o, float* out_d, float* out_w) {
  for (uint32_t s = 0; s < samples; s++)
    for (uint32_t p = 0; p < n; p++) {
      const size_t i = (size_t) s * n + p;
      const uint32_t y = pixels[p] / width, x = pixels[p] - y * width;
      float o[3], d[3];
      const float w0 = pc_sensor_sample(L, bn, width, height, x, y, first_sample + s, o, d);
      const float w = pc_lens_walk(L, bn, x, y, first_sample + s, o, d);
      V wo = v(o[0], o[1], -o[2]), wd = v(d[0], d[1], -d[2]);
      wo = qapply(rot, wo);
      wo = scl(wo, camera_scale * 0.001f);
      wo = add(wo, v(pos[0], pos[1], pos[2]));
      wd = qapply(rot, wd);
      out_o[3 * i] = wo.x; out_o[3 * i + 1] = wo.y; out_o[3 * i + 2] = wo.z;
      out_d[3 * i] = wd.x; out_d[3 * i + 1] = wd.y; out_d[3 * i + 2] = wd.z;
      out_w[i] = w * w0;
    }
}
