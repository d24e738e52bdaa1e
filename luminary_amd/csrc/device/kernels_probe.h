// The truth probes: kernels that only the tests launch (tests/test_light_query_truth.py, test_light_sample_truth.py, test_bounce_truth.py, test_sky_truth.py), each
// calling device functions of dev_*.h exactly as a render kernel calls them, and below them their launchers and this translation unit's WavefrontProbes table. The
// whole of a flavour's probe unit (wavefront_exact_probes.hip, wavefront_fast_probes.hip): no render kernel is compiled here, and none of this in the render's units,
// so an edit to a probe recompiles neither k_shade nor k_trace. The records' word counts: probe_layout.h.
#pragma once

#include "dev_trace.h"  // light_query; dev_light.h, dev_bsdf.h, dev_sampler.h (this unit's own g_sampler_seeds)
#include "dev_sky.h"
#include "dev_wave.h"  // kBlock
#include "probe_layout.h"
#include "wavefront_table.h"

LUM_NS_BEGIN

static_assert(kLightProbeLanes == kLightTreeOutputs, "probe_layout.h states dev_light.h's lane count for the host");

// ---- standalone light-BVH query for the traversal tests: one ray per thread, light_query exactly as k_light_query calls it ----
__global__ __launch_bounds__(kBlock) void k_light_query_probe(DeviceScene sc, uint32_t n, const float* origins, const float* dirs, const uint32_t* self, const float* randoms,
                                                              uint32_t* out_ids, uint32_t* out_num_hits) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  RayStats st{0, 0, 0};
  uint32_t num_hits = 0;
  const uint32_t id = light_query(sc, v3(origins[3 * i], origins[3 * i + 1], origins[3 * i + 2]), v3(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]), self[2 * i], self[2 * i + 1],
                                  randoms[i], num_hits, st);
  out_ids[i] = id; out_num_hits[i] = num_hits;
}

// ---- standalone light sampling for tests/test_light_sample_truth.py: one thread per (vertex, sample id), sample_light exactly as k_shade calls it ----
// The vertex is caller-made, as the oracle's probe_context makes it: 20 words {position, normal, V, albedo, opacity, roughness, ior ratio, material flags, self instance,
// self triangle, pixel x, pixel y}; state 0, the sampler the unseeded one at depth 0. Every workgroup stages the light lines and handles the way kernel_shade_body.h
// does (`stage` 0: nothing staged, every light is read from memory; kPlain stages them all). Per thread kLightProbeWords words:
//   [0..9)   the LightSample of the one real call: light id, ray, colour, dist, root_sum
//   [9..18)  tree_prepass: the eight cont words, root_sum
//   [18 + 17 lane ..) per lane: TreePick light id, TreePick weight, status, ray[3], solid angle, dist, emitted colour[3], BSDF weight[3], the direction probability
//            handed to mis_base, the MIS weight, the reservoir target
// The per-lane words are a second walk over the loop of light_candidates with the functions that loop calls on the arguments it passes them: shipped code is untouched.
// Words a lane does not reach keep what the caller put there.
enum LightProbeStatus : uint32_t { kLightProbeNoPick = 0, kLightProbeSelf = 1, kLightProbeRefused = 2, kLightProbeMissed = 3, kLightProbeEvaluated = 4 };
template <bool kPlain>
__global__ __launch_bounds__(kBlock) void k_light_sample_probe(DeviceScene sc, uint32_t n, uint32_t samples, uint32_t first_sample, uint32_t stage, const uint32_t* vertices,
                                                               uint32_t* out) {
  StagedLights staged_lights{nullptr, nullptr, 0u};
#if LUM_LDS_LIGHTS
  {
    __shared__ LdsF4 lds_light_table[4u * LUM_LDS_LIGHTS];
    __shared__ unsigned long long lds_light_handles[LUM_LDS_LIGHTS];
    const uint32_t staged = (kPlain || stage) ? min(sc.num_lights, (uint32_t) LUM_LDS_LIGHTS) : 0u;
    for (uint32_t k = threadIdx.x; k < 4u * staged; k += kBlock) { const float4 v = sc.light_tri_table[k]; const LdsF4 t = {v.x, v.y, v.z, v.w}; lds_light_table[k] = t; }
    for (uint32_t k = threadIdx.x; k < staged; k += kBlock) { const uint2 h = sc.light_tri_handles[k]; lds_light_handles[k] = (unsigned long long) h.x | ((unsigned long long) h.y << 32); }
    __syncthreads();
    staged_lights.table = (const __attribute__((address_space(3))) LdsF4*) lds_light_table;
    staged_lights.handles = (const __attribute__((address_space(3))) unsigned long long*) lds_light_handles;
    staged_lights.count = staged;
  }
#endif
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t* vw = vertices + (size_t) (i / samples) * kLightProbeVertexWords;
  uint32_t* o = out + (size_t) i * kLightProbeWords;
  GeoContext g;
  g.instance_id = vw[16]; g.tri_id = vw[17];
  g.position = v3(bitsf(vw[0]), bitsf(vw[1]), bitsf(vw[2]));
  g.normal = normalize(v3(bitsf(vw[3]), bitsf(vw[4]), bitsf(vw[5])));
  g.V = normalize(v3(bitsf(vw[6]), bitsf(vw[7]), bitsf(vw[8])));
  g.face_normal_packed = normal_pack(g.normal);
  g.state = 0;
  g.params.flags = vw[15];
  g.params.set(col(bitsf(vw[9]), bitsf(vw[10]), bitsf(vw[11])), bitsf(vw[12]), bitsf(vw[13]), splat(0.0f), bitsf(vw[14]));
  const SamplerT<false> smp{sc.bluenoise_2d, vw[18], vw[19], first_sample + i % samples, 0u};
  ShadeClock clock;
  clock.start();
  const LightSample ls = sample_light<kPlain>(sc, g, smp, clock, staged_lights);
  o[0] = ls.light_id; o[1] = fbits(ls.ray.x); o[2] = fbits(ls.ray.y); o[3] = fbits(ls.ray.z);
  o[4] = fbits(ls.color.r); o[5] = fbits(ls.color.g); o[6] = fbits(ls.color.b); o[7] = fbits(ls.dist); o[8] = fbits(ls.root_sum);
  // the second walk
  const TreeWork work = tree_prepass(sc, g, smp);
  const Energy energy = energy_terms(sc, g.params, world_ndotv(g));
#pragma unroll
  for (uint32_t l = 0; l < kLightTreeOutputs; l++) o[9 + l] = work.cont[l];
  o[17] = fbits(work.root_sum);
#if LUM_FAST
  const V3 view_local = normalize(qapply(rotation_to_z(g.normal), g.V));
#endif
#pragma nounroll
  for (uint32_t lane = 0; lane < kLightTreeOutputs; lane++) {
    uint32_t* w = o + kLightProbeHeadWords + lane * kLightProbeLaneWords;
    const TreePick pick = tree_postpass<kPlain>(sc, g, smp, lane, work);
    w[0] = pick.light_id; w[1] = fbits(pick.weight); w[2] = kLightProbeNoPick;
    if (pick.light_id == kLightIdInvalid) continue;
#if LUM_LDS_LIGHTS
    uint2 handle;
    const TableLight entry = load_tri_light_table<kPlain>(sc, staged_lights, pick.light_id, handle);
#else
    const uint2 handle = sc.light_tri_handles[pick.light_id];
    const TableLight entry = load_tri_light_table(sc, pick.light_id);
#endif
    const TriLight& tl = entry.tri;
    w[2] = kLightProbeSelf;
    if (handle.x == g.instance_id && handle.y == g.tri_id) continue;
    V3 ray; float sa;
    const F2 pair = smp.next2(kRndLightGeoRay + lane);
    w[2] = kLightProbeRefused;
    if (!sample_tri_solid_angle(g.position, tl, pair, ray, sa)) continue;
    w[3] = fbits(ray.x); w[4] = fbits(ray.y); w[5] = fbits(ray.z); w[6] = fbits(sa);
    F2 uv;
    const float dist = intersect_triangle(tl.vertex, tl.edge1, tl.edge2, g.position, ray, uv);
    w[2] = kLightProbeMissed;
    if (dist == kFltMax) continue;
    w[7] = fbits(dist);
    Col lc = (!kPlain && entry.textured) ? tri_light_color(sc, tl, uv) : entry.color;
    w[8] = fbits(lc.r); w[9] = fbits(lc.g); w[10] = fbits(lc.b);
#if LUM_FAST
    const RayTerms terms = analyze_direction(g.params, g.normal, g.V, ray);
    const Col bw = eval_with_face_normal(energy, g.params, terms, kHintGeneral, ray, normal_unpack(g.face_normal_packed), 1.0f);
    const float dir_prob = light_direction_probability_terms(g.params, view_local, terms);
    const float mis = 1.0f - mis_base(dir_prob, sa, importance(lc) * entry.area, dist * dist, work.root_sum);
#else
    bool is_refraction;
    const Col bw = eval_bsdf(energy, g, ray, kHintGeneral, is_refraction, 1.0f);
    const float dir_prob = light_direction_probability(g, ray);
    const float mis = mis_for_light_sample(g, ray, entry.area, lc, dist, sa, work.root_sum);
#endif
    lc = (lc * bw) * mis;
    w[2] = kLightProbeEvaluated;
    w[11] = fbits(bw.r); w[12] = fbits(bw.g); w[13] = fbits(bw.b); w[14] = fbits(dir_prob); w[15] = fbits(mis); w[16] = fbits(importance(lc));
  }
}

// ---- standalone bounce and BSDF-driven light direction for tests/test_bounce_truth.py: one thread per (vertex, sample id), sample_bounce and sample_light_direction
// exactly as k_shade calls them (dev_bsdf.h, dev_light.h) ----
// The vertex is the light probe's (20 words; self instance and triangle are not read here); state 0, the unseeded sampler at depth 0, set 0. Per thread kBounceProbeWords:
//   [0..3)    transparent_pass, microfacet_based, is_pass_through of the one real call of sample_bounce
//   [3..9)    its ray and weight
//   [9..22)   local_frame: the quaternion, V, the face normal, the energy terms (conductor, glossy, dielectric)
//   [22..29)  the second walk: the opacity draw and its outcome (0 not drawn, 1 stays, 2 passes), the initial pick, weight_sum after each technique, the chosen technique
//             (kBounceProbeNoTechnique on a transparent pass)
//   [29..37)  the second walk's weight, world ray, transparent_pass and microfacet_based
//   [37..44)  the one real call of sample_light_direction: ray, weight, probability
//   [44 + 24 t ..) per technique t (reflection, diffuse, refraction): status, m[3], local ray[3], the terms {fresnel_dielectric, NdotH, NdotL, NdotV, HdotL, HdotV,
//             is_refraction}, eval[3], the own pdf, the two other pdfs (reflection: diffuse, refraction; diffuse: reflection, refraction; refraction: reflection,
//             diffuse), mis, w, prob, pick after the decision
//   [116..143) sample_light_direction's second walk: status, rr, the sampling roughness, m[3], local ray[3], the terms, pdf, the weight before and after 1 / rr,
//             probability, world ray[3]
// The second walks call the functions sample_bounce and sample_light_direction call on the arguments they pass them: shipped code is untouched. Words of a stage that is
// not reached (a technique the material does not take, the pdfs of a refraction without total reflection, everything after a refused roulette) keep the caller's zero.
enum BounceProbeStatus : uint32_t { kBounceProbeNotTaken = 0, kBounceProbeTaken = 1, kBounceProbeTotalReflection = 2 };
enum BounceProbeLightDir : uint32_t { kBounceProbeRefused = 0, kBounceProbeReflection = 1, kBounceProbeRefraction = 2, kBounceProbeRefractionTotal = 3 };
constexpr uint32_t kBounceProbeNoTechnique = 3;
LUM_DEV void probe_put(uint32_t* w, V3 v) { w[0] = fbits(v.x); w[1] = fbits(v.y); w[2] = fbits(v.z); }
LUM_DEV void probe_put(uint32_t* w, Col c) { w[0] = fbits(c.r); w[1] = fbits(c.g); w[2] = fbits(c.b); }
LUM_DEV void probe_put(uint32_t* w, const RayTerms& c) {
  w[0] = fbits(c.fresnel_dielectric); w[1] = fbits(c.NdotH); w[2] = fbits(c.NdotL); w[3] = fbits(c.NdotV); w[4] = fbits(c.HdotL); w[5] = fbits(c.HdotV);
  w[6] = c.is_refraction ? 1u : 0u;
}
__global__ __launch_bounds__(kBlock) void k_bounce_probe(DeviceScene sc, uint32_t n, uint32_t samples, uint32_t first_sample, const uint32_t* vertices, uint32_t* out) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t* vw = vertices + (size_t) (i / samples) * kLightProbeVertexWords;
  uint32_t* o = out + (size_t) i * kBounceProbeWordsPerThread;
  GeoContext g;
  g.instance_id = vw[16]; g.tri_id = vw[17];
  g.position = v3(bitsf(vw[0]), bitsf(vw[1]), bitsf(vw[2]));
  g.normal = normalize(v3(bitsf(vw[3]), bitsf(vw[4]), bitsf(vw[5])));
  g.V = normalize(v3(bitsf(vw[6]), bitsf(vw[7]), bitsf(vw[8])));
  g.face_normal_packed = normal_pack(g.normal);
  g.state = 0;
  g.params.flags = vw[15];
  g.params.set(col(bitsf(vw[9]), bitsf(vw[10]), bitsf(vw[11])), bitsf(vw[12]), bitsf(vw[13]), splat(0.0f), bitsf(vw[14]));
  const SamplerT<false> smp{sc.bluenoise_2d, vw[18], vw[19], first_sample + i % samples, 0u};
  // the real calls
  const LocalFrame lf = local_frame(sc, g);
  const BounceSample bounce = sample_bounce(lf, g, smp, 0);
  const LightDirSample lb = sample_light_direction(lf, g, smp);
  o[0] = bounce.transparent_pass ? 1u : 0u; o[1] = bounce.microfacet_based ? 1u : 0u; o[2] = is_pass_through(g, bounce) ? 1u : 0u;
  probe_put(o + 3, bounce.ray); probe_put(o + 6, bounce.weight);
  o[9] = fbits(lf.to_z.x); o[10] = fbits(lf.to_z.y); o[11] = fbits(lf.to_z.z); o[12] = fbits(lf.to_z.w);
  probe_put(o + 13, lf.V); probe_put(o + 16, lf.face_normal);
  o[19] = fbits(lf.energy.conductor); o[20] = fbits(lf.energy.glossy); o[21] = fbits(lf.energy.dielectric);
  probe_put(o + 37, lb.ray); probe_put(o + 40, lb.weight); o[43] = fbits(lb.probability);
  const MatParams& p = g.params;
  const V3 Vl = lf.V, fnl = lf.face_normal;
  const V3 up = v3(0.0f, 0.0f, 1.0f);
  const float ior = p.ior(), roughness = p.roughness();
  const bool with_refraction = (p.flags & kMatSubstrateMask) == kMatTranslucent;
  // the second walk over sample_bounce
  {
    bool passes = false;
    const float opacity = p.opacity();
    if (opacity < 1.0f) {
      const float draw = smp.next1(kRndBsdfOpacity);
      passes = draw > opacity;
      o[22] = fbits(draw); o[23] = passes ? 2u : 1u;
    }
    if (passes) {
      o[28] = kBounceProbeNoTechnique;
      probe_put(o + 29, (p.flags & kMatColoredTransparency) ? p.albedo() : col(1.0f, 1.0f, 1.0f));
      probe_put(o + 32, g.V * -1.0f);
      o[35] = 1u; o[36] = 0u;
    }
    else {
      const bool with_diffuse = ((p.flags & kMatSubstrateMask) == 0) && ((p.flags & kMatMetallic) == 0);
      float pick = smp.next1(kRndBsdfResampling);
      o[24] = fbits(pick);
      V3 chosen_ray;
      Col chosen_eval;
      float weight_sum;
      uint32_t chosen = 0;
      bool transparent_pass = false, microfacet_based = true;
      {
        uint32_t* w = o + kBounceProbeHeadWords;
        const V3 m = sample_vndf_bounded(Vl, roughness, smp.next2(kRndBsdfReflection));
        const V3 ray = reflect(Vl, m);
        const RayTerms c = sampled_direction_terms(p, up, Vl, m, ray, false);
        const Col eval = eval_with_face_normal(lf.energy, p, c, kHintMicrofacet, ray, fnl, 1.0f);
        const float pdf = pdf_vndf_bounded(Vl, roughness, c.NdotH, c.NdotV);
        const float dp = with_diffuse ? pdf_diffuse(c.NdotL) : 0.0f;
        const float rp = with_refraction ? pdf_refraction(roughness, c.NdotH, c.NdotV, c.HdotV, c.HdotL, ior) : 0.0f;
        const float sum = pdf + dp + rp;
        const float mis = (sum > 0.0f) ? pdf / sum : 0.0f;
        chosen_ray = ray; chosen_eval = eval; weight_sum = importance(eval) * mis;
        w[0] = kBounceProbeTaken; probe_put(w + 1, m); probe_put(w + 4, ray); probe_put(w + 7, c); probe_put(w + 14, eval);
        w[17] = fbits(pdf); w[18] = fbits(dp); w[19] = fbits(rp); w[20] = fbits(mis); w[21] = fbits(weight_sum); w[23] = fbits(pick);
      }
      o[25] = fbits(weight_sum);
      if (with_diffuse) {
        uint32_t* w = o + kBounceProbeHeadWords + kBounceProbeTechWords;
        const F2 r2 = smp.next2(kRndBsdfDiffuse);
        const V3 ray = sample_ray_sphere(r2.x, r2.y);
        const V3 m = normalize(Vl + ray);
        const RayTerms c = sampled_direction_terms(p, up, Vl, m, ray, false);
        const Col eval = eval_with_face_normal(lf.energy, p, c, kHintDiffuse, ray, fnl, 1.0f);
        const float pdf = pdf_diffuse(c.NdotL);
        const float mp = pdf_vndf_bounded(Vl, roughness, c.NdotH, c.NdotV);
        const float rp = with_refraction ? pdf_refraction(roughness, c.NdotH, c.NdotV, c.HdotV, c.HdotL, ior) : 0.0f;
        const float sum = pdf + mp + rp;
        const float mis = (sum > 0.0f) ? pdf / sum : 0.0f;
        const float wt = importance(eval) * mis;
        weight_sum += wt;
        const float prob = wt / weight_sum;
        if (pick < prob) {
          chosen_ray = ray; chosen_eval = eval; transparent_pass = false; microfacet_based = false; chosen = 1;
          pick = clamp_random(pick / prob);
        }
        else pick = clamp_random((pick - prob) / (1.0f - prob));
        w[0] = kBounceProbeTaken; probe_put(w + 1, m); probe_put(w + 4, ray); probe_put(w + 7, c); probe_put(w + 14, eval);
        w[17] = fbits(pdf); w[18] = fbits(mp); w[19] = fbits(rp); w[20] = fbits(mis); w[21] = fbits(wt); w[22] = fbits(prob); w[23] = fbits(pick);
      }
      o[26] = fbits(weight_sum);
      if (with_refraction) {
        uint32_t* w = o + kBounceProbeHeadWords + 2 * kBounceProbeTechWords;
        bool total_reflection;
        const V3 m = sample_vndf_caps(Vl, roughness, smp.next2(kRndBsdfRefraction));
        const V3 ray = refract(Vl, m, ior, total_reflection);
        const RayTerms c = sampled_direction_terms(p, up, Vl, m, ray, !total_reflection);
        const Col eval = eval_with_face_normal(lf.energy, p, c, kHintRefraction, ray, fnl, 1.0f);
        float mis = 1.0f;
        if (total_reflection) {
          const float pdf = pdf_refraction(roughness, c.NdotH, c.NdotV, c.HdotV, c.HdotL, ior);
          const float refl = pdf_vndf_bounded(Vl, roughness, c.NdotH, c.NdotV);
          const float dp = with_diffuse ? pdf_diffuse(c.NdotL) : 0.0f;
          const float sum = pdf + refl + dp;
          mis = (sum > 0.0f) ? pdf / sum : 0.0f;
          w[17] = fbits(pdf); w[18] = fbits(refl); w[19] = fbits(dp);
        }
        const float wt = importance(eval) * mis;
        weight_sum += wt;
        const float prob = wt / weight_sum;
        if (pick < prob) {
          chosen_ray = ray; chosen_eval = eval; transparent_pass = !total_reflection; microfacet_based = true; chosen = 2;
          pick = clamp_random(pick / prob);
        }
        else pick = clamp_random((pick - prob) / (1.0f - prob));
        w[0] = total_reflection ? kBounceProbeTotalReflection : kBounceProbeTaken;
        probe_put(w + 1, m); probe_put(w + 4, ray); probe_put(w + 7, c); probe_put(w + 14, eval);
        w[20] = fbits(mis); w[21] = fbits(wt); w[22] = fbits(prob); w[23] = fbits(pick);
      }
      o[27] = fbits(weight_sum);
      o[28] = chosen;
      probe_put(o + 29, (weight_sum > 0.0f) ? chosen_eval * (weight_sum / importance(chosen_eval)) : col(0.0f, 0.0f, 0.0f));
      probe_put(o + 32, normalize(qapply(qinv(lf.to_z), chosen_ray)));
      o[35] = transparent_pass ? 1u : 0u; o[36] = microfacet_based ? 1u : 0u;
    }
  }
  // the second walk over sample_light_direction
  {
    uint32_t* w = o + kBounceProbeHeadWords + 3 * kBounceProbeTechWords;
    const uint32_t num_tech = with_refraction ? 2 : 1;
    const float refr_prob = with_refraction ? 1.0f / num_tech : 0.0f;
    const uint32_t tech = (uint32_t) (smp.next1(kRndLightBsdfChoice) * num_tech);
    const bool refraction = (tech == 1) && with_refraction;
    const float rr = light_dir_rr(roughness);
    w[0] = kBounceProbeRefused; w[1] = fbits(rr);
    if (smp.next1(kRndLightBsdfRR) >= rr) return;
    const float sr = light_dir_roughness(roughness);
    w[2] = fbits(sr);
    V3 m, ray;
    RayTerms c;
    float pdf, probability;
    bool total_reflection = false;
    if (!refraction) {
      m = sample_vndf_bounded(Vl, sr, smp.next2(kRndLightBsdfDirection));
      ray = reflect(Vl, m);
      c = sampled_direction_terms(p, up, Vl, m, ray, false);
      pdf = pdf_vndf_bounded(Vl, sr, c.NdotH, c.NdotV);
      probability = (1.0f - refr_prob) * pdf;
    }
    else {
      m = sample_vndf_caps(Vl, sr, smp.next2(kRndLightBsdfDirection));
      ray = refract(Vl, m, ior, total_reflection);
      c = sampled_direction_terms(p, up, Vl, m, ray, !total_reflection);
      pdf = pdf_refraction(sr, c.NdotH, c.NdotV, c.HdotV, c.HdotL, ior);
      probability = refr_prob * pdf;
    }
    const Col weight = eval_with_face_normal(lf.energy, p, c, kHintGeneral, ray, fnl, 1.0f / pdf);
    w[0] = !refraction ? kBounceProbeReflection : total_reflection ? kBounceProbeRefractionTotal : kBounceProbeRefraction;
    probe_put(w + 3, m); probe_put(w + 6, ray); probe_put(w + 9, c);
    w[16] = fbits(pdf); probe_put(w + 17, weight); probe_put(w + 20, weight * (1.0f / rr));
    w[23] = fbits(probability * rr);
    probe_put(w + 24, normalize(qapply(qinv(lf.to_z), ray)));
  }
}

// ---- standalone procedural sky for tests/test_sky_truth.py: one thread per caller-made ray, sky_get_color or sky_trace_inscattering exactly as k_sky and
// k_sky_inscattering call them (dev_sky.h), with no sampler: every random number is an input ----
// Per ray kSkyProbeRayWords: origin[3] (sky space, km), direction[3], limit, flags (1 celestials, 2 primary ray, 4 aerial perspective instead of sky_get_color, 8 the panorama: sky_hdri_color, see there),
// steps (aerial perspective: the sky.steps to derive the step count from), random_offset, step_random, 0. Per thread kSkyProbeWordsPerThread:
//   [0..5)    the second walk's path start and distance (sky_compute_path), the distance marched (min with limit - start), the step count, light_angle
//   [5..11)   the one real call: its colour, and the record (0.75, 0.5, 0.25) as sky_trace_inscattering leaves it (untouched by sky_get_color)
//   [11..25)  the second walk: final spectrum, its colour, the record
//   [25..31)  celestials: sun, earth and moon hit distances, the moon point (0 not reached, 1 lit, 2 in the earth's shadow), the star cell (kSkyProbeNoCell: not
//             reached), the sum of the hit stars' intensities
//   [31..39)  the marched segment's transmittance; [39] 0
//   [40 + 49 k ..) per step k < kSkyProbeMaxSteps: reach, height, cos_angle, zenith_cos, u, v, shadow, the Rayleigh and Mie phases, extinction_sun[8], ms_tex[8],
//             step_t[8], result and transmittance after the step [8 + 8]
// The second walk calls the functions sky_compute_atmosphere calls on the arguments it passes them: shipped code is untouched. It marches without cloud shadows, so
// the two walks agree in a scene without active clouds only. Words of steps that were not reached keep the caller's zero.
constexpr uint32_t kSkyProbeNoCell = 0xFFFFFFFFu;
LUM_DEV void probe_put(uint32_t* w, const Spectrum& s) {
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = fbits(s.v[i]);
}
__global__ __launch_bounds__(kBlock) void k_sky_probe(DeviceScene sc, uint32_t n, const uint32_t* rays, uint32_t* out) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= n) return;
  const uint32_t* rw = rays + (size_t) t * kSkyProbeRayWords;
  uint32_t* o = out + (size_t) t * kSkyProbeWordsPerThread;
  SkyView s = sky_view(sc);
  const V3 origin = v3(bitsf(rw[0]), bitsf(rw[1]), bitsf(rw[2])), ray = v3(bitsf(rw[3]), bitsf(rw[4]), bitsf(rw[5]));
  const float limit = bitsf(rw[6]), random_offset = bitsf(rw[9]), step_random = bitsf(rw[10]);
  const bool celestials = (rw[7] & 1u) != 0, primary_ray = (rw[7] & 2u) != 0, aerial = (rw[7] & 4u) != 0;
  const Col record_in = col(0.75f, 0.5f, 0.25f);
  if (rw[7] & 8u) {
    // the panorama: sky_hdri_color on a WORLD-space origin with the path state in word 8, then a second walk over sky_hdri_sample and sky_sun_color:
    //   [0..3) the origin in sky space; [11..15) theta, phi, u, v; [15], [16] the texel; [25] the sun's disk, [26] the earth (0 not asked, 1 hit, 2 missed);
    //   [31..34) the texel's colour; [34..37) the sun's colour, [37], [38] its table coordinates
    const uint32_t state = rw[8];
    probe_put(o + 5, sky_hdri_color(sc, origin, ray, state)); probe_put(o + 8, record_in); probe_put(o + 22, record_in);
    Col c = splat(0.0f);
    if (sc.sky_hdri != nullptr) {
      const float theta = atan2_det(ray.z, ray.x), phi = asin_det(ray.y);
      const float u = (theta + kRefPi) / (2.0f * kRefPi);
      const float v = 1.0f - ((phi + 0.5f * kRefPi) / kRefPi);
      const float dim = (float) sc.sky_hdri_dim;
      const uint32_t x = (uint32_t) ((u - floorf(u)) * dim) % sc.sky_hdri_dim, y = (uint32_t) ((v - floorf(v)) * dim) % sc.sky_hdri_dim;
      const float4 t = sc.sky_hdri[x + (size_t) y * sc.sky_hdri_dim];
      c = col(t.x, t.y, t.z);
      o[11] = fbits(theta); o[12] = fbits(phi); o[13] = fbits(u); o[14] = fbits(v); o[15] = x; o[16] = y;
      probe_put(o + 31, c);
    }
    if (state & (kStCameraDirection | kStAllowEmission)) {
      const V3 sky_origin = world_to_sky(s, origin);
      probe_put(o, sky_origin);
      const bool disk = sphere_hit(ray, sky_origin, s.sun_pos, kSkySunRadius), earth = sph_hit_p0(ray, sky_origin, kSkyEarthRadius);
      o[25] = disk ? 1u : 2u; o[26] = earth ? 1u : 2u;
      if (disk && !earth) {
        const float height = sky_height(sky_origin);
        const float zenith_cos = dot(normalize(sky_origin), ray);
        const F2 uv = sky_transmittance_uv(height, zenith_cos);
        const Spectrum extinction_sun = sp_mul(sp_ident(), sky_lut_fetch(s.tm, kSkyTmWidth, kSkyTmHeight, uv.x, uv.y));
        const Col sun_color = sky_color_from_spectrum(sp_mul(extinction_sun, sp_scale(sky_sun_radiance(), s.sun_strength)));
        o[37] = fbits(uv.x); o[38] = fbits(uv.y);
        probe_put(o + 34, sun_color);
        c = c + sun_color;
      }
    }
    probe_put(o + 19, c);
    return;
  }
  // the real call
  int steps = (int) rw[8];
  Col record = record_in, real;
  if (aerial) {
    s.steps = rw[8];
    real = sky_trace_inscattering(sc, s, origin, ray, limit, record, primary_ray, step_random, random_offset);
    steps = (int) (fminf(fmaxf(0.5f, limit / (primary_ray ? 40.0f : 80.0f)), 2.0f) * (float) (s.steps / 6u) + step_random - 0.5f);
  }
  else real = sky_get_color(sc, s, origin, ray, limit, celestials, steps, random_offset);
  probe_put(o + 5, real); probe_put(o + 8, record);
  // the second walk over sky_compute_atmosphere
  Spectrum result = sp_set1(0.0f);
  const F2 path = sky_compute_path(origin, ray, kSkyEarthRadius, kSkyAtmoRadius);
  const float start = path.x, distance = fminf(path.y, limit - start);
  Spectrum transmittance = aerial ? sp_set1(1.0f) : sp_ident();  // (sky_compute_atmosphere starts at sp_ident and multiplies the caller's 1 by it)
  Spectrum marched = sp_ident();
  o[0] = fbits(start); o[1] = fbits(path.y); o[2] = fbits(distance); o[3] = (uint32_t) steps;
  if (distance > 0.0f) {
    float reach = start;
    const float light_angle = sphere_solid_angle(s.sun_pos, kSkySunRadius, origin);
    o[4] = fbits(light_angle);
    for (int i = 0; i < steps; i++) {
      const float new_reach = start + distance * (i + random_offset) / steps;
      const float step_size = new_reach - reach;
      reach = new_reach;
      const V3 pos = origin + ray * reach;
      const float height = sky_height(pos);
      const V3 ray_scatter = normalize(s.sun_pos - pos);
      const float cos_angle = dot(ray, ray_scatter);
      const float zenith_cos = dot(normalize(pos), ray_scatter);
      const float phase_r = sky_rayleigh_phase(cos_angle), phase_m = sky_mie_phase(s, cos_angle);
      const float shadow = sph_hit_p0(ray_scatter, pos, kSkyEarthRadius) ? 0.0f : 1.0f;
      const F2 uv = sky_transmittance_uv(height, zenith_cos);
      const Spectrum extinction_sun = sky_lut_fetch(s.tm, kSkyTmWidth, kSkyTmHeight, uv.x, uv.y);
      const SkyMedium m = sky_medium(s, height);
      const Spectrum phase_times_scattering = sp_add(sp_scale(m.scattering_rayleigh, phase_r), sp_set1(m.scattering_mie * phase_m));
      const Spectrum ss_radiance = sp_scale(sp_mul(extinction_sun, phase_times_scattering), shadow * light_angle);
      const Spectrum ms_tex = sky_lut_fetch(s.ms, kSkyMsSize, kSkyMsSize, zenith_cos * 0.5f + 0.5f, height / kSkyAtmoHeight);
      const Spectrum S = sp_add(ss_radiance, sp_mul(ms_tex, m.scattering));
      const Spectrum step_t = sp_exp(sp_scale(m.extinction, -step_size));
      const Spectrum s_int = sp_mul(sp_sub(S, sp_mul(S, step_t)), sp_inv(m.extinction));
      result = sp_add(result, sp_mul(s_int, marched));
      marched = sp_mul(marched, step_t);
      if (i < (int) kSkyProbeMaxSteps) {
        uint32_t* w = o + kSkyProbeHeadWords + (uint32_t) i * kSkyProbeStepWords;
        w[0] = fbits(reach); w[1] = fbits(height); w[2] = fbits(cos_angle); w[3] = fbits(zenith_cos); w[4] = fbits(uv.x); w[5] = fbits(uv.y); w[6] = fbits(shadow);
        w[7] = fbits(phase_r); w[8] = fbits(phase_m);
        probe_put(w + 9, extinction_sun); probe_put(w + 17, ms_tex); probe_put(w + 25, step_t); probe_put(w + 33, result); probe_put(w + 41, marched);
      }
    }
    result = sp_mul(result, sp_scale(sky_sun_radiance(), s.sun_strength));
  }
  probe_put(o + 31, marched);
  o[29] = kSkyProbeNoCell;
  if (celestials && !aerial) {
    const float sun_hit = sphere_int(ray, origin, s.sun_pos, kSkySunRadius);
    const float earth_hit = sph_int_p0(ray, origin, kSkyEarthRadius);
    const bool has_moon = s.moon_albedo_tex != 0xFFFFFFFFu;
    const float moon_hit = has_moon ? sphere_int(ray, origin, s.moon_pos, kSkyMoonRadius) : kFltMax;
    o[25] = fbits(sun_hit); o[26] = fbits(earth_hit); o[27] = fbits(moon_hit);
    if (earth_hit > sun_hit && moon_hit > sun_hit) result = sp_add(result, sp_mul(marched, sp_scale(sky_sun_radiance(), s.sun_strength)));
    else if (earth_hit > moon_hit) {
      const V3 moon_point = origin + ray * moon_hit;
      const V3 bounce_ray = normalize(s.sun_pos - moon_point);
      const bool lit = !sphere_hit(bounce_ray, moon_point, v3(0.0f, 0.0f, 0.0f), kSkyEarthRadius);
      o[28] = lit ? 1u : 2u;
      if (lit) {  // the shaded colour, as sky_compute_atmosphere has it (create_basis + transform_vec3, two texture fetches); the truth leaves it out
        V3 normal = normalize(moon_point - s.moon_pos);
        const float tex_u = 0.5f + s.moon_tex_offset + atan2_det(normal.z, normal.x) * (1.0f / (2.0f * kRefPi));
        const float tex_v = 0.5f + asin_det(normal.y) * (1.0f / kRefPi);
        const F2 uv = F2{tex_u, tex_v};
        const float sign = copysignf(1.0f, normal.z);
        const float a = -1.0f / (sign + normal.z);
        const float b = normal.x * normal.y * a;
        const V3 u1 = v3(1.0f + sign * normal.x * normal.x * a, sign * b, -sign * normal.x);
        const V3 u2 = v3(b, sign + normal.y * normal.y * a, -normal.y);
        const float4 nv = texture_load(sc, s.moon_normal_tex, uv, true, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
        const V3 mn = v3(nv.x * 2.0f - 1.0f, nv.y * 2.0f - 1.0f, nv.z * 2.0f - 1.0f);
        normal = normalize(v3(u1.x * mn.x + u2.x * mn.y + normal.x * mn.z, u1.y * mn.x + u2.y * mn.y + normal.y * mn.z, u1.z * mn.x + u2.z * mn.y + normal.z * mn.z));
        const float NdotL = dot(normal, bounce_ray);
        if (NdotL > 0.0f) {
          const float albedo = texture_load(sc, s.moon_albedo_tex, uv, true, make_float4(0.0f, 0.0f, 0.0f, 0.0f)).x;
          const float light_angle = sphere_solid_angle(s.sun_pos, kSkySunRadius, moon_point);
          const float weight = albedo * s.sun_strength * NdotL * light_angle / (2.0f * kRefPi);
          result = sp_add(result, sp_mul(marched, sp_mul(sky_moon_solar_flux(), sp_scale(sky_sun_radiance(), weight))));
        }
      }
    }
    if (s.stars != nullptr && sun_hit == kFltMax && earth_hit == kFltMax && moon_hit == kFltMax) {
      const float ray_altitude = asin_det(ray.y);
      const float ray_azimuth = atan2_det(-ray.z, -ray.x) + kRefPi;
      const uint32_t x = f2u_sat(ray_azimuth * 10.0f), y = f2u_sat((ray_altitude + kRefPi * 0.5f) * 10.0f);
      const uint32_t grid = min(x, 63u) + min(y, 31u) * 64u;
      const uint32_t first = s.stars_offsets[grid], last = s.stars_offsets[grid + 1u];
      float star_sum = 0.0f;
      for (uint32_t i = first; i < last; i++) {
        const float4 star = s.stars[i];
        const V3 star_pos = angles_to_direction(star.x, star.y);
        if (sphere_hit(ray, v3(0.0f, 0.0f, 0.0f), star_pos, star.z)) {
          result = sp_add(result, sp_scale(marched, star.w * s.stars_intensity));
          star_sum += star.w * s.stars_intensity;
        }
      }
      o[29] = grid; o[30] = fbits(star_sum);
    }
  }
  transmittance = sp_mul(transmittance, marched);
  probe_put(o + 11, result);
  const Col walk = sky_color_from_spectrum(result);
  probe_put(o + 19, aerial ? walk * record_in : walk);
  probe_put(o + 22, aerial ? record_in * sky_color_from_spectrum(transmittance) : record_in);
}
// ---- the sun's next-event estimation for the same test: one thread per (vertex, sample id) on the light probe's caller-made vertices, sample_sun exactly as k_shade
// calls it (dev_sky.h), then a second walk over the functions it calls. Per thread kSunProbeWordsPerThread:
//   [0..7)   the real call: returned, light[3], direction[3]
//   [7..14)  sky_pos, the below-horizon and inside-earth flags (0 / 1), the reflection and refraction probabilities
//   [14..21) the shading frame: quaternion, local V
//   [21..27) the sampler's numbers: method, the BSDF pair, the sun pair, resampling
//   [27..35) the BSDF candidate: local ray, technique (0 reflection, 1 refraction, 2 refraction that reflects totally), world direction, the disk (1 hit, 2 missed)
//   [35..41) its sun colour and eval_bsdf (0 where the disk is missed)
//   [41..51) the solid-angle candidate: direction, solid angle, sun colour, eval_bsdf
//   [51..58) sun_bsdf_pdf of the two, the two MIS terms, the two weights, their sum
//   [58..63) the choice (0 none, 1 BSDF, 2 solid angle), the light, returned; [63] 1 where the vertex sees the sun at all
__global__ __launch_bounds__(kBlock) void k_sun_probe(DeviceScene sc, uint32_t n, uint32_t samples, uint32_t first_sample, const uint32_t* vertices, uint32_t* out) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t* vw = vertices + (size_t) (i / samples) * kLightProbeVertexWords;
  uint32_t* o = out + (size_t) i * kSunProbeWordsPerThread;
  GeoContext g;
  g.instance_id = vw[16]; g.tri_id = vw[17];
  g.position = v3(bitsf(vw[0]), bitsf(vw[1]), bitsf(vw[2]));
  g.normal = normalize(v3(bitsf(vw[3]), bitsf(vw[4]), bitsf(vw[5])));
  g.V = normalize(v3(bitsf(vw[6]), bitsf(vw[7]), bitsf(vw[8])));
  g.face_normal_packed = normal_pack(g.normal);
  g.state = 0;
  g.params.flags = vw[15];
  g.params.set(col(bitsf(vw[9]), bitsf(vw[10]), bitsf(vw[11])), bitsf(vw[12]), bitsf(vw[13]), splat(0.0f), bitsf(vw[14]));
  const SamplerT<false> smp{sc.bluenoise_2d, vw[18], vw[19], first_sample + i % samples, 0u};
  const SkyView sky = sky_view(sc);
  const LocalFrame lf = local_frame(sc, g);
  // the real call
  Col real_light = splat(0.0f);
  V3 real_dir = v3(0.0f, 0.0f, 0.0f);
  const bool real = sample_sun(sc, sky, lf, g, smp, real_light, real_dir);
  o[0] = real ? 1u : 0u;
  if (real) { probe_put(o + 1, real_light); probe_put(o + 4, real_dir); }
  // the second walk
  const Energy energy = energy_terms(sc, g.params, world_ndotv(g));
  const V3 sky_pos = world_to_sky(sky, g.position);
  const bool sun_below_horizon = sph_hit_p0(normalize(sky.sun_pos - sky_pos), sky_pos, kSkyEarthRadius);
  const bool inside_earth = length(sky_pos) < kSkyEarthRadius;
  probe_put(o + 7, sky_pos); o[10] = sun_below_horizon ? 1u : 0u; o[11] = inside_earth ? 1u : 0u;
  const MatParams& p = g.params;
  const bool translucent = (p.flags & kMatSubstrateMask) == kMatTranslucent;
  const float w_refl = 1.0f, w_refr = translucent ? 1.0f : 0.0f;
  const float reflection_prob = w_refl / (w_refl + w_refr), refraction_prob = w_refr / (w_refl + w_refr);
  o[12] = fbits(reflection_prob); o[13] = fbits(refraction_prob);
  o[14] = fbits(lf.to_z.x); o[15] = fbits(lf.to_z.y); o[16] = fbits(lf.to_z.z); o[17] = fbits(lf.to_z.w);
  probe_put(o + 18, lf.V);
  if (sun_below_horizon || inside_earth) return;
  o[63] = 1u;
  const float roughness = p.roughness();
  const float method = smp.next1(kRndSunBsdfMethod), resampling = smp.next1(kRndSunResampling);
  const F2 r_bsdf = smp.next2(kRndSunBsdf), r_sun = smp.next2(kRndSunRay);
  o[21] = fbits(method); o[22] = fbits(r_bsdf.x); o[23] = fbits(r_bsdf.y); o[24] = fbits(r_sun.x); o[25] = fbits(r_sun.y); o[26] = fbits(resampling);
  V3 ray_local;
  uint32_t technique = 0;
  if (method < reflection_prob) ray_local = reflect(lf.V, sample_vndf_bounded(lf.V, roughness, r_bsdf));
  else { bool total_reflection; ray_local = refract(lf.V, sample_vndf_caps(lf.V, roughness, r_bsdf), p.ior(), total_reflection); technique = total_reflection ? 2u : 1u; }
  const V3 dir_bsdf = normalize(qapply(qinv(lf.to_z), ray_local));
  probe_put(o + 27, ray_local); o[30] = technique; probe_put(o + 31, dir_bsdf);
  Col light_bsdf = splat(0.0f);
  bool is_refraction;
  const bool disk = sphere_hit(dir_bsdf, sky_pos, sky.sun_pos, kSkySunRadius);
  o[34] = disk ? 1u : 2u;
  if (disk) {
    const Col sun = sky_sun_color(sky, sky_pos, dir_bsdf), ev = eval_bsdf(energy, g, dir_bsdf, kHintGeneral, is_refraction, 1.0f);
    probe_put(o + 35, sun); probe_put(o + 38, ev);
    light_bsdf = sun * ev;
  }
  float solid_angle;
  const V3 dir_sa = sample_sphere(sky.sun_pos, kSkySunRadius, sky_pos, r_sun, solid_angle);
  const Col sun_sa = sky_sun_color(sky, sky_pos, dir_sa), ev_sa = eval_bsdf(energy, g, dir_sa, kHintGeneral, is_refraction, 1.0f);
  const Col light_sa = sun_sa * ev_sa;
  probe_put(o + 41, dir_sa); o[44] = fbits(solid_angle); probe_put(o + 45, sun_sa); probe_put(o + 48, ev_sa);
  const float target_bsdf = importance(light_bsdf), target_sa = importance(light_sa);
  const float pdf_bsdf = sun_bsdf_pdf(g, dir_bsdf, reflection_prob, refraction_prob), pdf_sa = sun_bsdf_pdf(g, dir_sa, reflection_prob, refraction_prob);
  const float mis_bsdf = solid_angle / (pdf_bsdf * solid_angle + 1.0f);
  const float mis_sa = solid_angle / (pdf_sa * solid_angle + 1.0f);
  const float weight_bsdf = target_bsdf * mis_bsdf, weight_sa = target_sa * mis_sa;
  const float sum_weights = weight_bsdf + weight_sa;
  o[51] = fbits(pdf_bsdf); o[52] = fbits(pdf_sa); o[53] = fbits(mis_bsdf); o[54] = fbits(mis_sa); o[55] = fbits(weight_bsdf); o[56] = fbits(weight_sa); o[57] = fbits(sum_weights);
  if (sum_weights == 0.0f) return;
  float target;
  Col light;
  if (resampling * sum_weights < weight_bsdf) { o[58] = 1u; target = target_bsdf; light = light_bsdf; }
  else { o[58] = 2u; target = target_sa; light = light_sa; }
  light = light * (sum_weights / target);
  probe_put(o + 59, light);
  o[62] = (target == 0.0f || importance(light) == 0.0f) ? 0u : 1u;
}
// The hardware's transcendental instructions alone, for the same test: y = v_exp_f32 (op 0), v_sin_f32 (1) or v_cos_f32 (2) of x, whatever the unit's flavour.
__global__ __launch_bounds__(kBlock) void k_sky_math_probe(uint32_t n, uint32_t op, const float* __restrict__ x, float* __restrict__ y) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= n) return;
  const float v = x[t];
  y[t] = (op == 0u) ? __builtin_amdgcn_exp2f(v) : (op == 1u) ? __builtin_amdgcn_sinf(v) : __builtin_amdgcn_cosf(v);
}

namespace table {

static int init_sampler_seeds() { return upload_sampler_seeds(); }
static void light_query_probe(hipStream_t s, const DeviceScene& sc, uint32_t n, const float* origins, const float* dirs, const uint32_t* self, const float* randoms, uint32_t* out_ids,
                              uint32_t* out_num_hits) {
  hipLaunchKernelGGL(k_light_query_probe, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, sc, n, origins, dirs, self, randoms, out_ids, out_num_hits);
}
static void light_sample_probe(hipStream_t s, const DeviceScene& sc, uint32_t n_vertices, uint32_t samples, uint32_t first_sample, uint32_t form, const uint32_t* vertices,
                               uint32_t* out) {
  const uint32_t n = n_vertices * samples;
  if (form == 1u) hipLaunchKernelGGL(k_light_sample_probe<true>, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, sc, n, samples, first_sample, 1u, vertices, out);
  else hipLaunchKernelGGL(k_light_sample_probe<false>, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, sc, n, samples, first_sample, form == 2u ? 0u : 1u, vertices, out);
}
static void bounce_probe(hipStream_t s, const DeviceScene& sc, uint32_t n_vertices, uint32_t samples, uint32_t first_sample, const uint32_t* vertices, uint32_t* out) {
  const uint32_t n = n_vertices * samples;
  hipLaunchKernelGGL(k_bounce_probe, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, sc, n, samples, first_sample, vertices, out);
}
static void sky_probe(hipStream_t s, const DeviceScene& sc, uint32_t n, const uint32_t* rays, uint32_t* out) {
  hipLaunchKernelGGL(k_sky_probe, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, sc, n, rays, out);
}
static void sun_probe(hipStream_t s, const DeviceScene& sc, uint32_t n_vertices, uint32_t samples, uint32_t first_sample, const uint32_t* vertices, uint32_t* out) {
  const uint32_t n = n_vertices * samples;
  hipLaunchKernelGGL(k_sun_probe, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, sc, n, samples, first_sample, vertices, out);
}
static void sky_math_probe(hipStream_t s, uint32_t n, uint32_t op, const float* x, float* y) {
  hipLaunchKernelGGL(k_sky_math_probe, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, n, op, x, y);
}

// Filled by member name, as the render's table is (wavefront_table_impl.h). tests/test_build_units.py checks that no member stays null.
static constexpr WavefrontProbes make_probes() {
  WavefrontProbes p{};
  p.init_sampler_seeds = init_sampler_seeds; p.light_query_probe = light_query_probe; p.light_sample_probe = light_sample_probe; p.bounce_probe = bounce_probe;
  p.sky_probe = sky_probe; p.sun_probe = sun_probe; p.sky_math_probe = sky_math_probe;
  return p;
}
static constexpr WavefrontProbes kProbes = make_probes();

}  // namespace table
LUM_NS_END

#if LUM_FAST
const lum::WavefrontProbes* lum::wavefront_probes_fast() { return &lum::table::kProbes; }
#else
const lum::WavefrontProbes* lum::wavefront_probes_exact() { return &lum::table::kProbes; }
#endif
