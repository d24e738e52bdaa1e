// The host twins of the image history's motion form (csrc/host/history.cpp lumc_history_motion_records_host, lumc_history_reproject_motion_host) as a program of its
// own: tests/test_history_motion.py builds it with -fsanitize=address,undefined,float-cast-overflow and runs it. Hostile part: every word of every transform, plane
// and key is a random bit pattern part of the time, owner ids lie below, at and far beyond the record count and among the reserved ids, record arrays are allocated
// exactly and handed over unaligned, frames go down to 1 x 1. Hand part: a sticker on a wall moved by three pixels - the disoccluded wall is rejected although its
// depth and normal agree, the sticker takes nothing from the wall, the cap holds for the sticker alone.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/lum_core.h"

static uint64_t state = 0xD1B54A32D192ED03ull;
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
static uint32_t owner_id(uint32_t count) {
  const uint32_t r = next();
  switch (r & 7u) {
    case 0: return 0xFFFFFFFFu - ((r >> 8) & 3u);  // the reserved ids
    case 1: return count + ((r >> 8) & 7u);        // at and beyond the count
    case 2: return next();
    default: return count ? (r >> 8) % count : 0xFFFFFFFEu;
  }
}
static LumHistoryKey key(uint32_t w, uint32_t h, bool wild) {
  LumHistoryKey k;
  for (float& f : k.pos) f = wild ? hostile(3.0f) : 0.25f;
  k.rotation[0] = wild ? hostile(0.2f) : 0.0f; k.rotation[1] = wild ? hostile(0.2f) : 0.05f; k.rotation[2] = wild ? hostile(0.2f) : 0.0f; k.rotation[3] = wild ? hostile(1.0f) : 0.99875f;
  k.fov = wild ? hostile(0.6f) : 0.6f; k.width = w; k.height = h;
  return k;
}
static void transform(float* p, bool wild) {
  for (int k = 0; k < 3; k++) p[k] = wild ? hostile(4.0f) : (float) (next() & 7u);
  for (int k = 3; k < 6; k++) p[k] = wild ? hostile(2.0f) : 0.5f + (float) (next() & 3u);
  for (int k = 6; k < 8; k++) { const uint32_t bits = next() ^ (next() << 16); std::memcpy(p + k, &bits, 4); }
}

static int hostile_runs(int& runs) {
  const uint32_t frames[][2] = {{1, 1}, {2, 1}, {7, 5}, {33, 9}, {50, 31}};
  const uint32_t counts[] = {0, 1, 3, 65, 300};
  for (const auto& now_wh : frames)
    for (const auto& old_wh : frames)
      for (uint32_t count : counts)
        for (int round = 0; round < 4; round++) {
          const size_t P = (size_t) now_wh[0] * now_wh[1], Q = (size_t) old_wh[0] * old_wh[1];
          const LumHistoryKey now = key(now_wh[0], now_wh[1], round >= 2), old = key(old_wh[0], old_wh[1], round >= 3);
          LumHistoryParams st;
          lumc_history_default_params(&st);
          st.enabled = 1;
          if (round == 3) { st.max_history = hostile(32.0f); st.depth_tolerance = hostile(0.1f); st.normal_threshold = hostile(1.0f); }
          std::vector<float> old8(8 * (size_t) count), new8(8 * (size_t) count);
          for (uint32_t i = 0; i < count; i++) {
            transform(old8.data() + 8 * i, round >= 1 && (i & 1u));
            if (i % 3u == 0u) std::memcpy(new8.data() + 8 * i, old8.data() + 8 * i, 32);
            else transform(new8.data() + 8 * i, round >= 1 && (i & 2u));
          }
          std::vector<unsigned char> raw(sizeof(LumHistoryMotionRecord) * (size_t) count + 4);  // four bytes off any alignment the allocator gives
          LumHistoryMotionRecord* records = reinterpret_cast<LumHistoryMotionRecord*>(raw.data() + 4);
          uint32_t by_class[3] = {0, 0, 0};
          if (lumc_history_motion_records_host(old8.data(), new8.data(), count, count ? records : nullptr, by_class)) { std::printf("history_motion_check: the record twin refused\n"); return 1; }
          if (by_class[0] + by_class[1] + by_class[2] != count) { std::printf("history_motion_check: the record classes do not add up\n"); return 1; }
          std::vector<float> normal(3 * P), depth(P), old_shown(3 * Q), old_weight(Q), old_normal(3 * Q), old_depth(Q), carried(3 * P), cw(P);
          std::vector<uint32_t> owner(P), old_owner(Q);
          fill(normal, 1.0f); fill(depth, 8.0f); fill(old_shown, 2.0f); fill(old_weight, 64.0f); fill(old_normal, 1.0f); fill(old_depth, 8.0f);
          for (size_t p = 0; p < P; p += 3) depth[p] = -1.0f;
          for (size_t q = 0; q < Q; q += 4) old_depth[q] = -1.0f;
          for (uint32_t& o : owner) o = owner_id(count);
          for (uint32_t& o : old_owner) o = owner_id(count);
          uint32_t stats[5] = {0, 0, 0, 0, 0};
          if (lumc_history_reproject_motion_host(&now, &old, &st, 8.0f, normal.data(), depth.data(), old_shown.data(), old_weight.data(), old_normal.data(), old_depth.data(), owner.data(),
                                                 old_owner.data(), count ? records : nullptr, count, carried.data(), cw.data(), stats)) {
            std::printf("history_motion_check: the reproject twin refused frame %u x %u\n", now_wh[0], now_wh[1]);
            return 1;
          }
          if ((size_t) stats[0] + stats[1] + stats[2] != P || stats[4] > stats[3] || stats[4] > stats[0]) { std::printf("history_motion_check: the counters do not add up\n"); return 1; }
          runs++;
        }
  return 0;
}

// A wall that fills the frame at depth 5 from a camera without rotation; a sticker of 4 x 4 pixels on it, instance 1, moved by three pixels along +x. A pixel
// centre lands on a pixel centre up to rounding, so a tap beside it may enter with a weight of a few ulp: the exact conditions are on pixels whose every
// neighbour has the same old owner.
static int hand_case() {
  const uint32_t w = 12, h = 6, P = w * h;
  LumHistoryKey k;
  std::memset(&k, 0, sizeof(k));
  k.rotation[3] = 1.0f; k.fov = 0.6f; k.width = w; k.height = h;
  std::vector<float> normal(3 * P, 0.0f), depth(P), shown(3 * P), weight(P, 1000.0f);
  for (uint32_t p = 0; p < P; p++) {
    float dir[3];
    if (lumc_history_centre_ray_host(&k, p % w, p / w, dir)) return 1;
    normal[2 * P + p] = 1.0f;
    depth[p] = -5.0f / dir[2];  // the plane z = -5
  }
  const float pixel = 2.0f * (0.6f / (float) w) * 5.0f;
  float old8[16], new8[16];
  for (int i = 0; i < 2; i++) {
    float* p = old8 + 8 * i;
    p[0] = p[1] = p[2] = 0.0f; p[3] = p[4] = p[5] = 1.0f;
    const uint32_t a = 0x7FFFu | (0x7FFFu << 16), b = 0x7FFFu | (0xFFFEu << 16);  // the identity quaternion
    std::memcpy(p + 6, &a, 4); std::memcpy(p + 7, &b, 4);
  }
  std::memcpy(new8, old8, sizeof(old8));
  new8[8] = 3.0f * pixel;
  LumHistoryMotionRecord rec[2];
  uint32_t by_class[3];
  if (lumc_history_motion_records_host(old8, new8, 2, rec, by_class) || by_class[0] != 1 || by_class[1] != 1 || by_class[2] != 0) { std::printf("history_motion_check: hand records\n"); return 1; }
  if (rec[0].cls != LUMC_HISTORY_MOTION_SAME || rec[1].cls != LUMC_HISTORY_MOTION_MOVED) return 1;
  std::vector<uint32_t> old_owner(P, 0u), owner(P, 0u);
  for (uint32_t y = 1; y < 5; y++)
    for (uint32_t x = 3; x < 7; x++) { old_owner[y * w + x] = 1u; owner[y * w + x + 3] = 1u; }
  for (uint32_t p = 0; p < P; p++) for (int c = 0; c < 3; c++) shown[c * P + p] = old_owner[p] == 1u ? 1.0f : 100.0f;
  LumHistoryParams st;
  lumc_history_default_params(&st);
  st.enabled = 1;
  std::vector<float> carried(3 * P), cw(P);
  uint32_t stats[5];
  if (lumc_history_reproject_motion_host(&k, &k, &st, 8.0f, normal.data(), depth.data(), shown.data(), weight.data(), normal.data(), depth.data(), owner.data(), old_owner.data(), rec, 2,
                                         carried.data(), cw.data(), stats)) return 1;
  for (uint32_t p = 0; p < P; p++) {
    const bool sticker = owner[p] == 1u, was = old_owner[p] == 1u;
    if (sticker) {
      if (!(cw[p] > 0.0f) || carried[p] != 1.0f || !(cw[p] <= 8.0f)) { std::printf("history_motion_check: sticker pixel %u carries %g with weight %g\n", p, carried[p], cw[p]); return 1; }
    }
    else if (was) {  // (column 4, rows 2 and 3: the old sticker all around)
      const bool inner = p % w == 4u && (p / w == 2u || p / w == 3u);
      if (inner ? (cw[p] != 0.0f || carried[p] != 0.0f) : (cw[p] > 0.0f && !(std::fabs(carried[p] - 100.0f) < 1e-3f))) { std::printf("history_motion_check: disoccluded pixel %u carries %g\n", p, carried[p]); return 1; }
    }
    else if (!(std::fabs(carried[p] - 100.0f) < 1e-3f) || !(cw[p] > 8.0f) || !(cw[p] <= 32.0f)) { std::printf("history_motion_check: wall pixel %u carries %g with weight %g\n", p, carried[p], cw[p]); return 1; }
  }
  if (stats[3] != 16 || stats[4] != 16 || stats[1] < 2) { std::printf("history_motion_check: hand counters %u %u %u %u %u\n", stats[0], stats[1], stats[2], stats[3], stats[4]); return 1; }
  return 0;
}

int main() {
  int runs = 0;
  if (hostile_runs(runs) || hand_case()) return 1;
  // refusals
  LumHistoryKey k = key(4, 4, false), bad = key(0, 4, false);
  LumHistoryParams st;
  lumc_history_default_params(&st);
  std::vector<float> a(48, 1.0f), b(16, 1.0f), out3(48, 42.0f), out1(16, 42.0f), t8(8, 1.0f);
  std::vector<uint32_t> o(16, 0u);
  LumHistoryMotionRecord rec;
  int refused = 0;
  refused += lumc_history_motion_records_host(nullptr, t8.data(), 1, &rec, nullptr);
  refused += lumc_history_motion_records_host(t8.data(), t8.data(), 1, nullptr, nullptr);
#define REPROJECT(NOW, CAP, OWNER, OLD_OWNER, REC, COUNT, OUT) \
  lumc_history_reproject_motion_host(NOW, &k, &st, CAP, a.data(), b.data(), a.data(), b.data(), a.data(), b.data(), OWNER, OLD_OWNER, REC, COUNT, OUT, out1.data(), nullptr)
  refused += REPROJECT(&k, 8.0f, nullptr, o.data(), &rec, 1, out3.data());
  refused += REPROJECT(&k, 8.0f, o.data(), nullptr, &rec, 1, out3.data());
  refused += REPROJECT(&k, 8.0f, o.data(), o.data(), nullptr, 1, out3.data());
  refused += REPROJECT(&k, 8.0f, o.data(), o.data(), &rec, 1, nullptr);
  refused += REPROJECT(&bad, 8.0f, o.data(), o.data(), &rec, 1, out3.data());
  refused += REPROJECT(&k, 0.0f, o.data(), o.data(), &rec, 1, out3.data());
  refused += REPROJECT(&k, NAN, o.data(), o.data(), &rec, 1, out3.data());
  refused += REPROJECT(&k, INFINITY, o.data(), o.data(), &rec, 1, out3.data());
  if (refused != 10) { std::printf("history_motion_check: %d of 10 refusals\n", refused); return 1; }
  for (float f : out3) if (f != 42.0f) { std::printf("history_motion_check: a refusal wrote\n"); return 1; }
  for (float f : out1) if (f != 42.0f) { std::printf("history_motion_check: a refusal wrote\n"); return 1; }
  if (lumc_history_motion_records_host(nullptr, nullptr, 0, nullptr, nullptr) != 0) { std::printf("history_motion_check: no instances is no error\n"); return 1; }
  std::printf("history_motion_check: ok (%d runs)\n", runs);
  return 0;
}
