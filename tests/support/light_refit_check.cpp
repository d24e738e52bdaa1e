// The light refit's host twin (csrc/host/light_refit.cpp) under the sanitizers, stand-alone: plans of several shapes over random soups - a root of two children,
// ranges on either side of a wave, unused slots, a node level, arrays allocated at exactly their sizes so that any byte written past them is seen -, a collapsed
// triangle and a NaN vertex (nothing may be written), and arguments the twin must refuse. Built with -fsanitize=address,undefined and run by
// tests/test_light_refit.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/lum_core.h"

namespace {

struct Case {
  std::vector<LumLightFragment> fragments;
  std::vector<LumLightTransform> transforms;
  std::vector<uint32_t> instances, offsets;
  std::vector<LumLightSlot> slots;
  std::vector<float> vertices, table, tris, stats;
  std::vector<uint8_t> root, nodes;
  LumLightRefitPlan plan{};
};

// root children of the given sizes; the first `node_children` of them are summarised again by one node each (8 slots splitting the range)
Case make(const std::vector<uint32_t>& counts, uint32_t node_children, uint32_t seed) {
  Case c;
  std::mt19937 rng(seed);
  std::uniform_real_distribution<float> u(-5.0f, 5.0f), s(0.5f, 2.0f);
  uint32_t n = 0;
  for (uint32_t k : counts) n += k;
  c.vertices.resize(12 * (size_t) n);
  for (float& v : c.vertices) v = u(rng);
  c.offsets = {0u, n};
  c.transforms.push_back(LumLightTransform{{0.1f, -0.2f, 0.3f, 0.9f}, {1.0f, 1.5f, 0.5f}, {1.0f, 2.0f, 3.0f}});
  c.instances = {0u};
  for (uint32_t i = 0; i < n; i++) c.fragments.push_back(LumLightFragment{0u, 0u, i, n - 1u - i, 0u, s(rng), s(rng), 0u});
  c.slots.assign(128, LumLightSlot{0u, 0u});
  uint32_t first = 0;
  for (size_t k = 0; k < counts.size(); k++) { c.slots[k] = LumLightSlot{first, counts[k]}; first += counts[k]; }
  for (uint32_t j = 0; j < node_children; j++) {
    const LumLightSlot r = c.slots[j];
    for (uint32_t k = 0; k < 8; k++) {
      const uint32_t a = r.first + (uint32_t) ((uint64_t) r.count * k / 8), b = r.first + (uint32_t) ((uint64_t) r.count * (k + 1) / 8);
      c.slots.push_back(LumLightSlot{a, b - a});
    }
  }
  const uint32_t sections = ((uint32_t) counts.size() + 7) / 8;
  c.root.assign(16 + 48 * (size_t) sections, 0);
  c.root[10] = (uint8_t) sections;
  c.nodes.assign(64 * (size_t) node_children, 0xAB);
  c.table.assign((size_t) sections * 64 + 16, 0.0f);
  c.tris.assign(12 * (size_t) n, 0.0f);
  c.stats.assign(8 * c.slots.size(), 0.0f);
  c.plan = LumLightRefitPlan{c.fragments.data(), c.transforms.data(), c.instances.data(), c.slots.data(), n, 1u, node_children, 0u, 1.0};
  return c;
}

int run(Case& c, LumLightRefitReport* report) {
  return lumc_light_refit_host(&c.plan, c.vertices.data(), c.offsets.data(), c.root.data(), c.table.data(), c.nodes.empty() ? nullptr : c.nodes.data(), c.tris.data(), c.stats.data(), report);
}

#define CHECK(cond) do { if (!(cond)) { std::printf("light_refit_check: %s failed at line %d\n", #cond, __LINE__); return 1; } } while (0)

}  // namespace

int main() {
  LumLightRefitReport report;
  const std::vector<std::vector<uint32_t>> shapes = {{1, 1}, {1, 2, 63, 64, 65, 127, 128, 129, 4097}, std::vector<uint32_t>(128, 3), {700, 9, 1, 300}};
  for (size_t k = 0; k < shapes.size(); k++) {
    Case c = make(shapes[k], k == 3 ? 2u : 0u, 7u + (uint32_t) k);
    CHECK(run(c, &report) == 0);
    CHECK(report.refitted == 1 && report.flags == 0 && report.cost > 0.0 && std::isfinite(report.cost_growth));
    for (size_t j = 0; j < c.nodes.size() / 64; j++) {
      const uint8_t* node = c.nodes.data() + 64 * j;
      CHECK(node[12] == 0xAB && node[6] == 0xAB && node[7] == 0xAB);
      for (int b = 13; b < 24; b++) CHECK(node[b] == 0xAB);
      for (int ch = 0; ch < 8; ch++) CHECK(c.slots[128 + 8 * j + ch].count == 0 || node[56 + ch] >= 1);
    }
  }
  {  // a collapsed triangle, a NaN: reported, nothing written
    for (int what = 0; what < 2; what++) {
      Case c = make({5, 60, 200}, 1, 21);
      if (what == 0) for (int v = 1; v < 3; v++) std::memcpy(&c.vertices[12 * 33 + 4 * v], &c.vertices[12 * 33], 3 * sizeof(float));
      else c.vertices[12 * 40 + 5] = std::nanf("");
      const std::vector<uint8_t> root = c.root, nodes = c.nodes;
      CHECK(run(c, &report) == 0);
      CHECK(report.refitted == 0 && report.flags == (what == 0 ? LUMC_LIGHT_REFIT_ZERO_AREA : LUMC_LIGHT_REFIT_NOT_FINITE));
      CHECK(root == c.root && nodes == c.nodes);
      for (float t : c.tris) CHECK(t == 0.0f);
    }
  }
  {  // refused: a slot beyond the fragments, a transform beyond the table, a light id beyond the lights, NULL arrays
    Case c = make({4, 4}, 0, 3);
    c.slots[1].count = 5;
    CHECK(run(c, &report) != 0);
    c.slots[1].count = 4; c.fragments[2].transform = 1;
    CHECK(run(c, &report) != 0);
    c.fragments[2].transform = 0; c.fragments[3].light_id = 8;
    CHECK(run(c, &report) != 0);
    c.fragments[3].light_id = 4;
    CHECK(lumc_light_refit_host(&c.plan, nullptr, c.offsets.data(), c.root.data(), c.table.data(), nullptr, c.tris.data(), nullptr, &report) != 0);
    CHECK(lumc_light_refit_host(nullptr, c.vertices.data(), c.offsets.data(), c.root.data(), c.table.data(), nullptr, c.tris.data(), nullptr, &report) != 0);
  }
  {  // the one-light tree and the empty one: left alone
    Case c = make({1}, 0, 5);
    CHECK(run(c, &report) == 0 && report.refitted == 0 && report.flags == 0);
  }
  for (float x : {1.0f, 1.0000001f, 0.99999994f, 1e-45f, 3e-45f, 3.4e38f, 255.0f, 256.0f})
    CHECK(lumc_light_refit_ceil_log2(x) == (int) std::ceil(std::log2((double) x)));
  std::printf("light_refit_check: ok\n");
  return 0;
}
