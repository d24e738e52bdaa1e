// The firefly resolve's host twin (csrc/host/firefly.cpp lumc_firefly_resolve_host) as a program of its own, built with the address and undefined-behaviour
// sanitizers by tests/test_firefly.py: every bucket count 4 ... 16 over random bucket sums with outliers, zeros, negative values, NaN and Inf, for counts from the
// ids [0, S) of the suite; equal buckets leave the image alone; one outlier is trimmed into the range of the others; a pixel of non-finite buckets becomes 0; the
// counters add up; what the twin refuses writes nothing.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

extern "C" int lumc_firefly_resolve_host(const float* sums, const uint32_t* counts, uint32_t K, uint32_t pixels, float* image_inout, uint32_t stats[3]);

namespace {
uint32_t g_state = 2463534242u;
uint32_t rnd() { g_state = g_state * 1664525u + 1013904223u; return g_state >> 8; }
float uniform(float lo, float hi) { return lo + (hi - lo) * (float) (rnd() & 0xFFFF) / 65535.0f; }
int g_bad = 0;
void expect(bool ok, const char* what) { if (!ok) { std::printf("firefly_check: %s\n", what); g_bad++; } }
}  // namespace

int main() {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  for (uint32_t K = 4; K <= 16; K++) {
    const uint32_t S[] = {1, 3, K - 1, K, K + 1, 8 * K, 8 * K + 3};
    for (uint32_t s : S) {
      const uint32_t P = 257;
      std::vector<uint32_t> counts(K, 0);
      for (uint32_t id = 0; id < s; id++) counts[id % K]++;
      std::vector<float> sums((size_t) K * 3 * P), image(3 * P), before;
      for (uint32_t p = 0; p < P; p++) {
        const float level = uniform(0.0f, 4.0f);
        for (uint32_t b = 0; b < K; b++)
          for (uint32_t ch = 0; ch < 3; ch++) {
            float v = level * (float) counts[b] * uniform(0.9f, 1.1f);
            if (p % 7 == 1 && b == rnd() % K) v *= 1000.0f;
            if (p % 11 == 2 && b == p % K) v = ch == 1 ? nan : v;
            if (p % 13 == 3 && b == (p + 1) % K) v = inf;
            if (p % 17 == 4) v = 0.0f;
            if (p % 19 == 5) v = -v;
            if (p % 23 == 6) v = nan;
            sums[((size_t) b * 3 + ch) * P + p] = v;
          }
        for (uint32_t ch = 0; ch < 3; ch++) image[(size_t) ch * P + p] = 123.0f + (float) ch;
      }
      before = image;
      uint32_t stats[3] = {9, 9, 9};
      expect(lumc_firefly_resolve_host(sums.data(), counts.data(), K, P, image.data(), stats) == 0, "the twin refused its arguments");
      uint32_t written = 0, m = 0;
      for (uint32_t b = 0; b < K; b++) m += counts[b] ? 1u : 0u;
      for (uint32_t p = 0; p < P; p++) {
        const bool same = image[p] == before[p] && image[P + p] == before[P + p] && image[2 * P + p] == before[2 * P + p];
        written += same ? 0u : 1u;
        if (p % 23 == 6) expect(image[p] == 0.0f && image[P + p] == 0.0f && image[2 * P + p] == 0.0f, "a pixel of non-finite buckets is not 0");
        if (p % 17 == 4 && p % 23 != 6) expect(same, "all-zero buckets were rewritten");
        for (uint32_t ch = 0; ch < 3; ch++) expect(std::isfinite(image[(size_t) ch * P + p]), "an output is not finite");
      }
      expect(written <= stats[0] && stats[0] <= P, "the rewritten counter");  // (a rewritten pixel may by chance get the value it had)
      expect(stats[1] % 2 == 0 && stats[1] <= stats[0] * (m & ~1u), "the trimmed counter");
      if (m < 4) expect(stats[1] == 0, "fewer than four buckets were trimmed");
      expect(stats[2] <= stats[0], "a pixel with a non-finite bucket is always rewritten");
    }
  }
  {  // one outlier among equal buckets is trimmed, and so is the darkest in exchange
    const uint32_t K = 8, P = 1;
    uint32_t counts[K];
    float sums[K * 3], image[3] = {7, 7, 7};
    for (uint32_t b = 0; b < K; b++) { counts[b] = 8; for (uint32_t ch = 0; ch < 3; ch++) sums[b * 3 + ch] = 8.0f * (1.0f + 0.01f * (float) b); }
    for (uint32_t ch = 0; ch < 3; ch++) sums[5 * 3 + ch] = 8.0f * 1000.0f;
    uint32_t stats[3];
    expect(lumc_firefly_resolve_host(sums, counts, K, P, image, stats) == 0 && stats[0] == 1 && stats[1] >= 2 && stats[2] == 0, "the outlier was not trimmed");
    for (uint32_t ch = 0; ch < 3; ch++) expect(image[ch] >= 1.0f && image[ch] <= 1.07f, "the output left the range of the other buckets");
  }
  {  // refusals write nothing
    const uint32_t counts[4] = {1, 1, 1, 1}, none[4] = {0, 0, 0, 0};
    float sums[12] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1}, image[3] = {9, 9, 9};
    uint32_t stats[3] = {42, 42, 42};
    const uint32_t bad_k[] = {0, 1, 3, 17};
    for (uint32_t K : bad_k) expect(lumc_firefly_resolve_host(sums, counts, K, 1, image, stats) == 1, "a bad bucket count is taken");
    expect(lumc_firefly_resolve_host(nullptr, counts, 4, 1, image, stats) == 1 && lumc_firefly_resolve_host(sums, nullptr, 4, 1, image, stats) == 1 &&
           lumc_firefly_resolve_host(sums, counts, 4, 1, nullptr, stats) == 1, "a NULL array is taken");
    expect(lumc_firefly_resolve_host(sums, none, 4, 1, image, stats) == 1, "counts that are all zero are taken");
    expect(image[0] == 9 && image[1] == 9 && image[2] == 9 && stats[0] == 42 && stats[1] == 42 && stats[2] == 42, "a refusal wrote something");
    expect(lumc_firefly_resolve_host(sums, counts, 4, 1, image, nullptr) == 0 && image[0] == 9, "the stats are optional; equal buckets are left alone");
  }
  std::printf(g_bad ? "firefly_check: %d failures\n" : "firefly_check: ok\n", g_bad);
  return g_bad ? 1 : 0;
}
