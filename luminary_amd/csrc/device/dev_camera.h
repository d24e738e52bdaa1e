// Physical camera: camera rays traced from the sensor through a stack of spherical lens interfaces (cuda/camera_physical.cuh:8-293,
// cuda/camera.cuh:11-38). The lens (DeviceLens, dev_scene.h) is an argument of the camera-ray kernels only: k_generate<kCam>,
// k_generate_adaptive<kCam>, k_camera_rays<kCam>, k_pixel_ray. Non-spectral: every medium has its design index of refraction.
//
// Where the table is read from: without reflections a ray that is still alive is at interface `iteration` - a wave-uniform index - so the
// interface is a scalar load from the kernel argument. With reflections the lanes of a wave stand at different interfaces; the kernels stage
// the table in LDS first (stage_lens) and every lane reads its own entry there.
#pragma once

#include "dev_bsdf.h"
#include "dev_sampler.h"

LUM_NS_BEGIN

constexpr uint32_t kLensMaxIntersections = 32;  // RANDOM_LENS_MAX_INTERSECTIONS (random.cuh:10): steps through the lens before a ray is given up
constexpr float kIorAir = 1.0003f;              // IOR_AIR (device_utils.h:71)
static_assert(kRndLensMethod + kLensMaxIntersections <= kRndLens, "one random dimension per lens step");

// math.cuh:620-641: distance to the first intersection in front of the origin of a ray with a sphere (centre p, radius r), FLT_MAX if none
LUM_DEV float sphere_ray_intersection(V3 ray, V3 origin, V3 p, float r) {
  const V3 diff = origin - p;
  const float d = dot(diff, ray);
  const float r2 = r * r;
  const float c = dot(diff, diff) - r2;
  const V3 k = diff - ray * d;
  const float disc = r2 - dot(k, k);
  if (disc < 0.0f) return kFltMax;
  const float sd = sqrtf(disc);
  const float q = -d - copysignf(sd, d);
  const float t0 = c / q;
  if (t0 >= 0.0f) return t0;
  return (q >= 0.0f) ? q : kFltMax;
}

// camera_simulation_intersect_aperture (camera_physical.cuh:60-75): the segment [origin, origin + dist * ray] crosses the aperture plane outside the stop
LUM_DEV bool lens_aperture_blocks(const DeviceLens& lens, V3 origin, V3 ray, float dist) {
  const float t = (lens.aperture_point - origin.z) / ray.z;
  if (t > 0.0f && t < dist) {
    const V3 h = origin + ray * t;
    const float d2 = h.x * h.x + h.y * h.y;
    if (d2 > lens.aperture_radius * lens.aperture_radius) return true;
  }
  return false;
}

// camera_simulation_intersect_medium_cylinder (camera_physical.cuh:77-117): inside a glass element the ray reflects off the element's cylindrical rim
// if it reaches it before the next interface (Fresnel-weighted, index ratio medium / air)
LUM_DEV bool lens_medium_cylinder(V3& origin, V3& ray, float& weight, float dist, float cylindrical_radius, float medium_ior) {
  if (cylindrical_radius == kFltMax) return false;
  V3 cray = v3(ray.x, ray.y, 0.0f);
  const float clen = length(cray);
  if (clen == 0.0f) return false;
  cray = cray * (1.0f / clen);
  const V3 corigin = v3(origin.x, origin.y, 0.0f);
  float cdist = sphere_ray_intersection(cray, corigin, v3(0.0f, 0.0f, 0.0f), cylindrical_radius);
  cdist *= 1.0f / clen;
  if (cdist > 0.0f && cdist < dist) {
    origin = origin + ray * cdist;
    const V3 n = normalize(v3(-origin.x, -origin.y, 0.0f));
    const float ior = medium_ior * (1.0f / kIorAir);
    const V3 V = ray * -1.0f;
    bool total_reflection;
    const V3 refraction = refract(V, n, ior, total_reflection);
    const float fresnel = (total_reflection == false) ? fresnel_dielectric(n, V, refraction, ior) : 1.0f;
    weight *= fresnel;
    ray = reflect(V, n);
    return true;
  }
  return false;
}

// camera_physical_sample<kReflections, false> + the world transform of camera_sample (camera.cuh:29-35). Returns the ray's weight; 0 = the ray did
// not leave the lens (it then gets no path; origin and ray are what the walk left, for the tests).
template <bool kReflections>
LUM_DEV float camera_sample_physical(const DeviceScene& sc, const DeviceLens& lens, const Sampler& smp, V3& origin_out, V3& ray_out) {
  // sensor point (:8-22), with the thin lens's jitter (camera_utils.cuh:23-27)
  const U2 jq = smp.raw2_at(kRndCameraJitter, 0, 0, 0);
  const float jx = unit_float(jq.x), jy = unit_float(jq.y);
  const float step = 2.0f * (lens.sensor_width / sc.width);
  const float vfov = step * sc.height * 0.5f;
  const V3 sensor = v3(lens.sensor_width - step * (smp.px + jx), -vfov + step * (smp.py + jy), -lens.image_plane_distance);
  // exit-pupil sample (:24-42)
  const F2 r = smp.next2(kRndLens);
  const float alpha = r.x * 2.0f * kPi, beta = sqrtf(r.y) * lens.exit_pupil_radius;
  float sa, ca;
  sincos_det(alpha, sa, ca);
  const V3 diff = v3(ca * beta, sa * beta, lens.exit_pupil_point) - sensor;
  const float dist = length(diff);
  const float area = lens.exit_pupil_radius * lens.exit_pupil_radius * kPi;
  V3 o = sensor, d = normalize(diff);
  const float initial_weight = area * fabsf(d.z) / (dist * dist);

  // the walk through the interfaces (camera_simulation_trace :212-246 over camera_simulation_step :119-210)
  float ior = kIorAir, cylindrical_radius = kFltMax, weight = 1.0f;
  bool forward = true, reflected = false;
  const uint32_t n = lens.num_interfaces;
  uint32_t iteration = 0;
  int32_t current = 0;
  for (; iteration < kLensMaxIntersections; iteration++) {
    const int32_t id = kReflections ? current : (int32_t) iteration;  // (without reflections `current` == `iteration` while the ray lives)
    const LensInterface f = lens.iface[id];
    const V3 center = v3(0.0f, 0.0f, f.vertex - f.radius);
    const float radius = fabsf(f.radius);
    int32_t move = 0;
    float t = sphere_ray_intersection(d, o, center, radius);
    if (t == kFltMax || lens_aperture_blocks(lens, o, d, t)) weight = 0.0f;
    else {
      const bool inside = length(o - center) < radius;  // before the origin moves
      bool alive = true;
      if (lens_medium_cylinder(o, d, weight, t, cylindrical_radius, ior)) {
        t = sphere_ray_intersection(d, o, center, radius);
        if (t == kFltMax || lens_aperture_blocks(lens, o, d, t)) { weight = 0.0f; alive = false; }
      }
      if (alive) {
        const LensMedium m = lens.medium[forward ? id + 1 : id];
        o = o + d * t;
        if (o.x * o.x + o.y * o.y > f.cylindrical_radius * f.cylindrical_radius) weight = 0.0f;  // past the rim of the interface
        else {
          V3 nrm = normalize(o - center);
          if (inside) nrm = nrm * -1.0f;
          const V3 V = d * -1.0f;
          const float eta = ior / m.design_ior;
          bool total_reflection;
          const V3 refraction = refract(V, nrm, eta, total_reflection);
          const V3 reflection = reflect(V, nrm);
          bool allow_reflection = false;
          if constexpr (kReflections) allow_reflection = (id != 0 || iteration != 0) && (!reflected || !forward);  // at most one pair of reflections
          const bool allow_refraction = id != 0 || iteration == 0;
          float w;
          bool refracts;
          if (total_reflection) { w = allow_reflection ? 1.0f : 0.0f; refracts = false; }
          else {
            const float fresnel = fresnel_dielectric(nrm, V, refraction, eta);
            if (allow_refraction && allow_reflection) { w = 1.0f; refracts = smp.next1(kRndLensMethod + iteration) >= fresnel; }
            else if (allow_reflection) { w = fresnel; refracts = false; }
            else { w = 1.0f - fresnel; refracts = true; }
          }
          weight *= w;
          d = refracts ? refraction : reflection;
          ior = refracts ? m.design_ior : ior;
          cylindrical_radius = refracts ? m.cylindrical_radius : cylindrical_radius;
          forward = refracts ? forward : !forward;
          reflected = refracts ? reflected : true;
          move = forward ? 1 : -1;
        }
      }
    }
    current += move;
    if ((uint32_t) current >= n || current < 0 || weight == 0.0f) break;
  }
  if (current < 0 || (iteration == kLensMaxIntersections && (uint32_t) current <= n)) weight = 0.0f;

  // the lens looks along +z, the scene's camera along -z (:288-290); then rotation, scale (mm -> m) and position like the thin lens
  o.z = -o.z; d.z = -d.z;
  const Quat q{sc.cam_rotation[0], sc.cam_rotation[1], sc.cam_rotation[2], sc.cam_rotation[3]};
  o = qapply(q, o);
  o = o * (sc.cam_scale * 0.001f);
  origin_out = o + v3(sc.cam_pos[0], sc.cam_pos[1], sc.cam_pos[2]);
  ray_out = qapply(q, d);
  return weight * initial_weight;
}

// The lens the camera-ray kernels read: with reflections a block-wide copy in LDS (every thread of the block must call this), else the argument itself.
template <int kCam>
LUM_DEV const DeviceLens& stage_lens(const DeviceLens& arg, DeviceLens* lds) {
  if constexpr (kCam == kCamPhysicalReflections) {
    static_assert(sizeof(DeviceLens) % 4 == 0, "copied in words");
    for (uint32_t k = threadIdx.x; k < sizeof(DeviceLens) / 4; k += blockDim.x) reinterpret_cast<uint32_t*>(lds)[k] = reinterpret_cast<const uint32_t*>(&arg)[k];
    __syncthreads();
    return *lds;
  }
  else return arg;
}

// ---- thin-lens camera (cuda/camera_thin_lens.cuh:8-86, cuda/camera.cuh:29-35) ----
LUM_DEV void camera_ray(const DeviceScene& sc, const Sampler& smp, V3& origin, V3& ray) {
  const U2 jq = smp.raw2_at(kRndCameraJitter, 0, 0, 0);  // same jitter for every pixel of a sample (camera_utils.cuh:23-27)
  const float jx = unit_float(jq.x), jy = unit_float(jq.y);
  const float step = 2.0f * (sc.cam_fov / sc.width);
  const float vfov = step * sc.height * 0.5f;
  const V3 sensor = v3(sc.cam_fov - step * (smp.px + jx), -vfov + step * (smp.py + jy), 1.0f);
  const V3 to_focal = normalize(v3(0.0f, 0.0f, 0.0f) - sensor);
  const float focal = fmaxf(sc.cam_object_distance * (1.0f / 0.001f), 0.01f);
  const V3 focal_point = to_focal * (-focal / to_focal.z);
  V3 aperture = v3(0.0f, 0.0f, 0.0f);
  if (sc.cam_aperture_size != 0.0f) {
    const F2 r = smp.next2(kRndLens);
    const float asz = sc.cam_aperture_size * (1.0f / 0.001f);
    if (sc.cam_aperture_shape == 1) {
      const int blade = (int) (smp.next1(kRndLensBlade) * sc.cam_aperture_blade_count);
      const float alpha = sqrtf(r.x), beta = r.y;
      const float u = 1.0f - alpha, v = alpha * beta;
      const float astep = (2.0f * kPi) / sc.cam_aperture_blade_count;
      float s1, c1, s2, c2;
      sincos_det(astep * blade, s1, c1); sincos_det(astep * (blade + 1), s2, c2);
      aperture = v3((s1 * u + s2 * v) * asz, (c1 * u + c2 * v) * asz, 0.0f);
    }
    else {
      const float alpha = r.x * 2.0f * kPi, beta = sqrtf(r.y) * asz;
      float sa, ca; sincos_det(alpha, sa, ca);
      aperture = v3(ca * beta, sa * beta, 0.0f);
    }
  }
  const Quat q{sc.cam_rotation[0], sc.cam_rotation[1], sc.cam_rotation[2], sc.cam_rotation[3]};
  V3 o = qapply(q, aperture);
  o = o * (sc.cam_scale * 0.001f);
  origin = o + v3(sc.cam_pos[0], sc.cam_pos[1], sc.cam_pos[2]);
  ray = qapply(q, normalize(focal_point - aperture));
}

// The camera ray of a sample by camera kind; returns its weight (the thin lens's is 1).
template <int kCam>
LUM_DEV float camera_sample(const DeviceScene& sc, const DeviceLens& lens, const Sampler& smp, V3& o, V3& d) {
  if constexpr (kCam == kCamThinLens) { camera_ray(sc, smp, o, d); return 1.0f; }
  else return camera_sample_physical<kCam == kCamPhysicalReflections>(sc, lens, smp, o, d);
}

LUM_NS_END
