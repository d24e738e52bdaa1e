// The host twin of the light tree's refit kernels (light_refit.hip): light_refit.h's functions over a plan, plain C++ - no HIP, no device. The definition of the
// bytes: what every test holds the kernels to (lum_core.h lumc_light_refit_host).
#define LUM_LRF_HOST_ONLY 1
#include "light_refit.h"

#include <vector>

namespace lum {

namespace {

// the 64 lanes' partials through the xor butterfly 32, 16, 8, 4, 2, 1: every lane ends with the same bits (the addition commutes), lane 0's are returned
float butterfly(float p[kLightWave]) {
  for (uint32_t k = kLightWave / 2; k >= 1; k >>= 1) {
    float t[kLightWave];
    for (uint32_t l = 0; l < kLightWave; l++) t[l] = p[l] + p[l ^ k];
    memcpy(p, t, sizeof(t));
  }
  return p[0];
}

void slot_statistics(const LrfVec* rec, LumLightSlot slot, float* s) {
  for (uint32_t k = 0; k < kLightStatFloats; k++) s[k] = 0.0f;
  if (slot.count == 0) return;
  float p[kLightWave], m[4][kLightWave];
  for (uint32_t l = 0; l < kLightWave; l++) p[l] = lrf_lane_power(rec, slot.first, slot.count, l);
  const float power = butterfly(p);
  const float inv_total = 1.0f / power;
  for (uint32_t l = 0; l < kLightWave; l++) {
    const LrfVec v = lrf_lane_mean(rec, slot.first, slot.count, l, inv_total);
    m[0][l] = v.x; m[1][l] = v.y; m[2][l] = v.z; m[3][l] = v.w;
  }
  const LrfVec mean{butterfly(m[0]), butterfly(m[1]), butterfly(m[2]), butterfly(m[3])};
  for (uint32_t l = 0; l < kLightWave; l++) p[l] = lrf_lane_variance(rec, slot.first, slot.count, l, inv_total, mean);
  s[0] = power; s[1] = butterfly(p); s[2] = mean.x; s[3] = mean.y; s[4] = mean.z; s[5] = mean.w;
}

}  // namespace

int light_refit_host(const LumLightRefitPlan* plan, const float* vertices, const uint32_t* mesh_tri_offset, uint8_t* root, float* root_children, uint8_t* nodes,
                     float* light_bvh_tris, float* slot_stats, LumLightRefitReport* report) {
  if (!plan || !report) return 1;
  *report = LumLightRefitReport{};
  const uint32_t n = plan->num_fragments;
  if (n < 2) return 0;  // no lights, or the one-light tree, which is constant
  if (!plan->fragments || !plan->transforms || !plan->slots || !vertices || !mesh_tri_offset || !root || !root_children || !light_bvh_tris) return 1;
  if (plan->num_nodes && !nodes) return 1;
  const uint32_t sections = root[10];
  if (sections == 0 || sections > kLightRootSlots / 8) return 1;
  const size_t num_slots = kLightRootSlots + (size_t) kLightNodeSlots * plan->num_nodes;
  for (uint32_t i = 0; i < n; i++)
    if (plan->fragments[i].transform >= plan->num_transforms || plan->fragments[i].light_id >= n) return 1;
  for (size_t s = 0; s < num_slots; s++)
    if (plan->slots[s].first > n || plan->slots[s].count > n - plan->slots[s].first) return 1;
  for (uint32_t c = 8 * sections; c < kLightRootSlots; c++) if (plan->slots[c].count) return 1;

  std::vector<LrfVec> rec(kLightRecordVecs * (size_t) n);
  std::vector<float> tris(12 * (size_t) n);
  uint32_t flags = 0;
  for (uint32_t i = 0; i < n; i++) {
    const LumLightFragment& f = plan->fragments[i];
    const float* v = vertices + 4 * 3 * ((size_t) mesh_tri_offset[f.mesh] + f.triangle);
    const float p[9] = {v[0], v[1], v[2], v[4], v[5], v[6], v[8], v[9], v[10]};
    LrfVec* r = rec.data() + kLightRecordVecs * (size_t) i;
    flags |= lrf_fragment(f, plan->transforms[f.transform], p, r);
    memcpy(tris.data() + 12 * (size_t) f.light_id, r, 12 * sizeof(float));
  }
  report->flags = flags;
  if (flags) return 0;  // the set of lights changed: nothing is written

  std::vector<float> stats(kLightStatFloats * num_slots);
  for (size_t s = 0; s < num_slots; s++) slot_statistics(rec.data(), plan->slots[s], stats.data() + kLightStatFloats * s);
  if (slot_stats) memcpy(slot_stats, stats.data(), stats.size() * sizeof(float));

  float result[2 * kLightRootSlots] = {};
  for (uint32_t c = 0; c < kLightRootSlots; c++) lrf_root_lane(stats.data(), c, sections, root, root_children, result);
  for (uint32_t j = 0; j < plan->num_nodes; j++)
    for (uint32_t c = 0; c < kLightNodeSlots; c++) lrf_node_lane(stats.data() + kLightStatFloats * (kLightRootSlots + (size_t) kLightNodeSlots * j), c, nodes + 64 * (size_t) j);
  memcpy(light_bvh_tris, tris.data(), tris.size() * sizeof(float));
  double cost = 0.0;
  for (uint32_t c = 0; c < 8 * sections; c++) cost += (double) result[2 * c] * (double) result[2 * c + 1];
  report->refitted = 1; report->cost = cost; report->cost_growth = plan->root_cost > 0.0 ? cost / plan->root_cost : 0.0;
  return 0;
}

}  // namespace lum

extern "C" int lumc_light_refit_host(const LumLightRefitPlan* plan, const float* vertices, const uint32_t* mesh_tri_offset, uint8_t* root, float* root_children,
                                     uint8_t* nodes, float* light_bvh_tris, float* slot_stats, LumLightRefitReport* report) {
  return lum::light_refit_host(plan, vertices, mesh_tri_offset, root, root_children, nodes, light_bvh_tris, slot_stats, report);
}

extern "C" int lumc_light_refit_ceil_log2(float x) { return lum::lrf_ceil_log2(x); }
