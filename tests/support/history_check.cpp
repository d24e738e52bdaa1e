// The host twins of the image history (csrc/host/history.cpp) on hostile planes, as a program of its own: tests/test_history.py builds it with
// -fsanitize=address,undefined,float-cast-overflow and runs it. Every float of every plane and key is a random bit pattern part of the time (NaN, infinities,
// denormals, huge values), the frames include 1 x 1 and sizes that are no multiple of anything, and the outputs are allocated exactly: a tap outside the old frame,
// a conversion of a coordinate that is no integer, or a neighbour beyond the image's edge would be reported.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/lum_core.h"

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint32_t next() { state ^= state << 13; state ^= state >> 7; state ^= state << 17; return (uint32_t) (state >> 16); }
static float hostile(float tame) {
  const uint32_t r = next();
  if ((r & 7u) != 0u) return tame * (float) ((r >> 8) & 1023u) / 512.0f;
  const uint32_t bits = next();
  float f;
  std::memcpy(&f, &bits, 4);
  return f;
}
static void fill(std::vector<float>& v, float tame) { for (float& f : v) f = hostile(tame); }

static LumHistoryKey key(uint32_t w, uint32_t h, bool wild) {
  LumHistoryKey k;
  for (float& f : k.pos) f = wild ? hostile(3.0f) : 0.25f;
  k.rotation[0] = wild ? hostile(0.2f) : 0.0f; k.rotation[1] = wild ? hostile(0.2f) : 0.05f; k.rotation[2] = wild ? hostile(0.2f) : 0.0f; k.rotation[3] = wild ? hostile(1.0f) : 0.99875f;
  k.fov = wild ? hostile(0.6f) : 0.6f; k.width = w; k.height = h;
  return k;
}

int main() {
  const uint32_t frames[][2] = {{1, 1}, {2, 1}, {1, 3}, {7, 5}, {33, 9}, {50, 31}};
  int runs = 0;
  for (const auto& now_wh : frames)
    for (const auto& old_wh : frames)
      for (int round = 0; round < 6; round++) {
        const size_t P = (size_t) now_wh[0] * now_wh[1], Q = (size_t) old_wh[0] * old_wh[1];
        const LumHistoryKey now = key(now_wh[0], now_wh[1], round >= 2), old = key(old_wh[0], old_wh[1], round >= 3);
        LumHistoryParams st;
        lumc_history_default_params(&st);
        st.enabled = 1; st.clamp_sigma = (round & 1) ? 1.5f : 0.0f;
        if (round == 5) { st.max_history = hostile(32.0f); st.depth_tolerance = hostile(0.1f); st.normal_threshold = hostile(1.0f); st.clamp_sigma = hostile(2.0f); }
        std::vector<float> normal(3 * P), depth(P), old_shown(3 * Q), old_weight(Q), old_normal(3 * Q), old_depth(Q), carried(3 * P), cw(P), image(3 * P), shown(3 * P), weight(P);
        fill(normal, 1.0f); fill(depth, 8.0f); fill(old_shown, 2.0f); fill(old_weight, 64.0f); fill(old_normal, 1.0f); fill(old_depth, 8.0f); fill(image, 2.0f);
        for (size_t p = 0; p < P; p += 3) depth[p] = -1.0f;
        for (size_t q = 0; q < Q; q += 4) old_depth[q] = -1.0f;
        uint32_t stats[3] = {0, 0, 0};
        if (lumc_history_reproject_host(&now, &old, &st, normal.data(), depth.data(), old_shown.data(), old_weight.data(), old_normal.data(), old_depth.data(), carried.data(), cw.data(), stats)) {
          std::printf("history_check: the reproject twin refused frame %u x %u\n", now_wh[0], now_wh[1]);
          return 1;
        }
        if ((size_t) stats[0] + stats[1] + stats[2] != P) { std::printf("history_check: the classes do not add up to the pixels\n"); return 1; }
        if (lumc_history_blend_host(&st, now_wh[0], now_wh[1], 1u + (uint32_t) round, image.data(), carried.data(), cw.data(), shown.data(), weight.data())) {
          std::printf("history_check: the blend twin refused\n");
          return 1;
        }
        if (lumc_history_blend_host(&st, now_wh[0], now_wh[1], 4u, image.data(), nullptr, nullptr, nullptr, nullptr)) { std::printf("history_check: the blend twin refused optional outputs\n"); return 1; }
        float dir[3], fx, fy;
        if (lumc_history_centre_ray_host(&now, now_wh[0] - 1u, now_wh[1] - 1u, dir) || lumc_history_project_host(&old, dir, &fx, &fy) == 1) { std::printf("history_check: the projection refused\n"); return 1; }
        runs++;
      }
  // refusals: null arrays, empty and oversized frames, half a carried plane
  LumHistoryKey k = key(4, 4, false), bad = key(0, 4, false), big = key(70000, 1, false);
  LumHistoryParams st;
  lumc_history_default_params(&st);
  std::vector<float> a(48, 1.0f), b(16, 1.0f), out3(48, 42.0f), out1(16, 42.0f);
  int refused = 0;
  refused += lumc_history_reproject_host(nullptr, &k, &st, a.data(), b.data(), a.data(), b.data(), a.data(), b.data(), out3.data(), out1.data(), nullptr);
  refused += lumc_history_reproject_host(&k, &k, &st, nullptr, b.data(), a.data(), b.data(), a.data(), b.data(), out3.data(), out1.data(), nullptr);
  refused += lumc_history_reproject_host(&k, &k, &st, a.data(), b.data(), a.data(), b.data(), a.data(), b.data(), nullptr, out1.data(), nullptr);
  refused += lumc_history_reproject_host(&bad, &k, &st, a.data(), b.data(), a.data(), b.data(), a.data(), b.data(), out3.data(), out1.data(), nullptr);
  refused += lumc_history_reproject_host(&k, &big, &st, a.data(), b.data(), a.data(), b.data(), a.data(), b.data(), out3.data(), out1.data(), nullptr);
  refused += lumc_history_blend_host(&st, 0, 4, 1, out3.data(), nullptr, nullptr, nullptr, nullptr);
  refused += lumc_history_blend_host(&st, 4, 4, 1, nullptr, nullptr, nullptr, nullptr, nullptr);
  refused += lumc_history_blend_host(&st, 4, 4, 1, out3.data(), a.data(), nullptr, nullptr, nullptr);
  refused += lumc_history_blend_host(nullptr, 4, 4, 1, out3.data(), nullptr, nullptr, nullptr, nullptr);
  if (refused != 9) { std::printf("history_check: %d of 9 refusals\n", refused); return 1; }
  for (float f : out3) if (f != 42.0f) { std::printf("history_check: a refusal wrote\n"); return 1; }
  for (float f : out1) if (f != 42.0f) { std::printf("history_check: a refusal wrote\n"); return 1; }
  std::printf("history_check: ok (%d runs)\n", runs);
  return 0;
}
