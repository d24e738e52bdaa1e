// The host twins of k_history_reproject and k_history_blend (history.hip): history.h's history_reproject_pixel and history_blend_pixel compiled by the host
// compiler, no HIP in it. They define the bytes the kernels are held to (lum_core.h lumc_history_reproject_host, lumc_history_blend_host; tests/test_history.py,
// tests/test_history_gpu.py). The motion form's twins beside them: history_motion_record and history_reproject_pixel_motion (lumc_history_motion_records_host,
// lumc_history_reproject_motion_host; tests/test_history_motion.py, tests/test_history_motion_gpu.py).
#define LUM_HISTORY_HOST_ONLY 1
#include "history.h"
#define LUM_MATTE_HOST_ONLY 1
#include "matte.h"

#include <vector>

#include "../../../include/lum_core.h"

static_assert(sizeof(LumHistoryKey) == sizeof(lum::HistoryKey) && sizeof(LumHistoryParams) == sizeof(lum::HistorySettings), "lum_core.h mirrors history.h field for field");

static_assert(sizeof(LumHistoryMotionRecord) == sizeof(lum::HistoryMotion) && sizeof(lum::HistoryMotion) == 128, "one cache line per instance, lum_core.h mirrors history.h field for field");
static_assert(lum::kHistoryOwnerReserved == lum::kMatteIdParticle && lum::kMatteIdParticle < lum::kMatteIdOcean && lum::kMatteIdOcean < lum::kMatteIdMiss && lum::kMatteIdMiss < lum::kMatteIdEmpty,
              "the reserved owner ids are matte.h's, the particle's the lowest");

namespace {
lum::HistoryKey key_of(const LumHistoryKey* k) { lum::HistoryKey out; memcpy(&out, k, sizeof(out)); return out; }
lum::HistorySettings settings_of(const LumHistoryParams* p) { lum::HistorySettings out; memcpy(&out, p, sizeof(out)); return out; }
bool frame_ok(const lum::HistoryKey& k) { return k.width > 0 && k.height > 0 && k.width <= 0xFFFFu && k.height <= 0xFFFFu; }
}  // namespace

extern "C" void lumc_history_default_params(LumHistoryParams* p) {
  if (!p) return;
  p->enabled = 0u; p->max_history = 32.0f; p->depth_tolerance = 0.02f; p->normal_threshold = 0.9f; p->clamp_sigma = 0.0f;
}

extern "C" int lumc_history_reproject_host(const LumHistoryKey* now_key, const LumHistoryKey* old_key, const LumHistoryParams* params, const float* normal, const float* depth,
                                           const float* old_shown, const float* old_weight, const float* old_normal, const float* old_depth, float* carried, float* carried_weight,
                                           uint32_t stats[3]) {
  if (!now_key || !old_key || !params || !normal || !depth || !old_shown || !old_weight || !old_normal || !old_depth || !carried || !carried_weight) return 1;
  const lum::HistoryKey now = key_of(now_key), old = key_of(old_key);
  if (!frame_ok(now) || !frame_ok(old)) return 1;
  const lum::HistorySettings st = settings_of(params);
  const size_t P = (size_t) now.width * now.height, Q = (size_t) old.width * old.height;
  uint32_t counts[3] = {0, 0, 0};
  for (uint32_t y = 0; y < now.height; y++)
    for (uint32_t x = 0; x < now.width; x++) {
      const size_t p = (size_t) y * now.width + x;
      lum::HistoryRec out;
      const uint32_t cls = lum::history_reproject_pixel(
          now, old, st, x, y, lum::HistoryV3{normal[p], normal[P + p], normal[2 * P + p]}, depth[p],
          [&](uint32_t tx, uint32_t ty) { const size_t q = (size_t) ty * old.width + tx; return lum::HistoryRec{old_shown[q], old_shown[Q + q], old_shown[2 * Q + q], old_weight[q]}; },
          [&](uint32_t tx, uint32_t ty) { const size_t q = (size_t) ty * old.width + tx; return lum::HistoryRec{old_normal[q], old_normal[Q + q], old_normal[2 * Q + q], old_depth[q]}; }, out);
      carried[p] = out.x; carried[P + p] = out.y; carried[2 * P + p] = out.z; carried_weight[p] = out.w;
      counts[cls]++;
    }
  if (stats) { stats[0] = counts[0]; stats[1] = counts[1]; stats[2] = counts[2]; }
  return 0;
}

extern "C" int lumc_history_blend_host(const LumHistoryParams* params, uint32_t width, uint32_t height, uint32_t uniform_samples, float* image_inout, const float* carried,
                                       const float* carried_weight, float* out_shown, float* out_weight) {
  if (!params || !image_inout || width == 0 || height == 0 || width > 0xFFFFu || height > 0xFFFFu || (carried == nullptr) != (carried_weight == nullptr)) return 1;
  const lum::HistorySettings st = settings_of(params);
  const size_t P = (size_t) width * height;
  const std::vector<float> cur(image_inout, image_inout + 3 * P);  // the neighbourhoods are the image's as it came
  const float N = (float) uniform_samples;
  for (uint32_t y = 0; y < height; y++)
    for (uint32_t x = 0; x < width; x++) {
      const size_t p = (size_t) y * width + x;
      const lum::HistoryRec c = carried ? lum::HistoryRec{carried[p], carried[P + p], carried[2 * P + p], carried_weight[p]} : lum::HistoryRec{0.0f, 0.0f, 0.0f, 0.0f};
      lum::HistoryRec shown;
      const bool written = lum::history_blend_pixel(st, width, height, x, y, N, c, [&](uint32_t tx, uint32_t ty, uint32_t ch) { return cur[(size_t) ch * P + (size_t) ty * width + tx]; }, shown);
      if (written) { image_inout[p] = shown.x; image_inout[P + p] = shown.y; image_inout[2 * P + p] = shown.z; }
      if (out_shown) { out_shown[p] = shown.x; out_shown[P + p] = shown.y; out_shown[2 * P + p] = shown.z; }
      if (out_weight) out_weight[p] = shown.w;
    }
  return 0;
}

extern "C" int lumc_history_centre_ray_host(const LumHistoryKey* key, uint32_t px, uint32_t py, float dir[3]) {
  if (!key || !dir) return 1;
  const lum::HistoryV3 d = lum::history_centre_ray(key_of(key), px, py);
  dir[0] = d.x; dir[1] = d.y; dir[2] = d.z;
  return 0;
}

extern "C" int lumc_history_project_host(const LumHistoryKey* key, const float v[3], float* fx, float* fy) {
  if (!key || !v || !fx || !fy) return 1;
  return lum::history_project(key_of(key), lum::HistoryV3{v[0], v[1], v[2]}, *fx, *fy) ? 0 : 2;
}

extern "C" int lumc_history_motion_records_host(const float* old8, const float* new8, uint32_t count, LumHistoryMotionRecord* records, uint32_t stats[3]) {
  if (count && (!old8 || !new8 || !records)) return 1;
  uint32_t counts[3] = {0, 0, 0};  // moved, same, void
  for (uint32_t i = 0; i < count; i++) {
    const lum::HistoryMotion r = lum::history_motion_record(old8 + 8 * (size_t) i, new8 + 8 * (size_t) i);
    memcpy(records + i, &r, sizeof(r));
    counts[r.cls == lum::kHistoryMotionMoved ? 0 : (r.cls == lum::kHistoryMotionSame ? 1 : 2)]++;
  }
  if (stats) { stats[0] = counts[0]; stats[1] = counts[1]; stats[2] = counts[2]; }
  return 0;
}

extern "C" int lumc_history_reproject_motion_host(const LumHistoryKey* now_key, const LumHistoryKey* old_key, const LumHistoryParams* params, float motion_max_history, const float* normal,
                                                  const float* depth, const float* old_shown, const float* old_weight, const float* old_normal, const float* old_depth,
                                                  const uint32_t* owner, const uint32_t* old_owner, const LumHistoryMotionRecord* records, uint32_t count, float* carried,
                                                  float* carried_weight, uint32_t stats[5]) {
  if (!now_key || !old_key || !params || !normal || !depth || !old_shown || !old_weight || !old_normal || !old_depth || !owner || !old_owner || (count && !records) || !carried || !carried_weight)
    return 1;
  if (!(motion_max_history > 0.0f) || !lum::history_finite(motion_max_history)) return 1;
  const lum::HistoryKey now = key_of(now_key), old = key_of(old_key);
  if (!frame_ok(now) || !frame_ok(old)) return 1;
  const lum::HistorySettings st = settings_of(params);
  std::vector<lum::HistoryMotion> rec(count);  // (the caller's array need not be aligned to a line)
  if (count) memcpy(rec.data(), records, sizeof(lum::HistoryMotion) * (size_t) count);
  const size_t P = (size_t) now.width * now.height, Q = (size_t) old.width * old.height;
  uint32_t counts[5] = {0, 0, 0, 0, 0};
  for (uint32_t y = 0; y < now.height; y++)
    for (uint32_t x = 0; x < now.width; x++) {
      const size_t p = (size_t) y * now.width + x;
      lum::HistoryRec out;
      bool moved = false;
      const uint32_t cls = lum::history_reproject_pixel_motion(
          now, old, st, motion_max_history, x, y, lum::HistoryV3{normal[p], normal[P + p], normal[2 * P + p]}, depth[p], owner[p], count,
          [&](uint32_t tx, uint32_t ty) { const size_t q = (size_t) ty * old.width + tx; return lum::HistoryRec{old_shown[q], old_shown[Q + q], old_shown[2 * Q + q], old_weight[q]}; },
          [&](uint32_t tx, uint32_t ty) { const size_t q = (size_t) ty * old.width + tx; return lum::HistoryRec{old_normal[q], old_normal[Q + q], old_normal[2 * Q + q], old_depth[q]}; },
          [&](uint32_t tx, uint32_t ty) { return old_owner[(size_t) ty * old.width + tx]; }, [&](uint32_t id) { return rec[id].cls; }, [&](uint32_t id) { return rec[id]; }, out, moved);
      carried[p] = out.x; carried[P + p] = out.y; carried[2 * P + p] = out.z; carried_weight[p] = out.w;
      counts[cls]++;
      if (moved) { counts[lum::kHistoryStatMoved]++; if (cls == lum::kHistoryCarried) counts[lum::kHistoryStatMovedCarried]++; }
    }
  if (stats) for (int k = 0; k < 5; k++) stats[k] = counts[k];
  return 0;
}
