// The shutter's host twin (csrc/host/mesh_shutter.cpp lumc_shutter_host) as a program of its own, built with the address and undefined-behaviour sanitizers by
// tests/test_mesh_shutter.py: every corner count and time of the suite over random records with -0, equal normal words, opposite normals and a pair whose
// difference overflows; t = 0 and t = 1 return the keys verbatim; the output may be one of the inputs; what the twin refuses writes nothing.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

extern "C" int lumc_shutter_host(const void* open_records, const void* close_records, uint32_t count, float t, void* out_records, uint32_t* flags);

namespace {
struct Rec { float x, y, z; uint32_t n; };
uint32_t g_state = 12345u;
uint32_t rnd() { g_state = g_state * 1664525u + 1013904223u; return g_state >> 8; }
float uniform(float lo, float hi) { return lo + (hi - lo) * (float) (rnd() & 0xFFFF) / 65535.0f; }
int g_bad = 0;
void expect(bool ok, const char* what) { if (!ok) { std::printf("mesh_shutter_check: %s\n", what); g_bad++; } }
}  // namespace

int main() {
  const uint32_t counts[] = {3, 189, 192, 195, 255, 258, 3000};
  const float times[] = {0.0f, std::ldexp(1.0f, -24), 0.25f, 0.5f, 0.75f, 1.0f - std::ldexp(1.0f, -24), 1.0f};
  for (uint32_t count : counts) {
    std::vector<Rec> a(count), b(count);
    for (uint32_t c = 0; c < count; c++) {
      a[c] = {uniform(-3, 3), uniform(-3, 3), uniform(-3, 3), (rnd() & 0xFFFF) | ((rnd() & 0xFFFF) << 16)};
      b[c] = {uniform(-3, 3), uniform(-3, 3), uniform(-3, 3), (rnd() & 0xFFFF) | ((rnd() & 0xFFFF) << 16)};
      if (c % 5 == 1) { a[c].x = -0.0f; b[c].y = -0.0f; }
      if (c % 5 == 2) b[c].n = a[c].n;
      if (c % 5 == 3) { a[c].n = 0x7FFF7FFFu + 0x00010001u; b[c].n = 0x00000000u; }  // +z and the octahedron's far corner
    }
    a[0].n = 0xFFFF8000u; b[0].n = 0x00008000u;  // +y and -y: all but opposite (no two words unpack to exact opposites), the blend at t = 0.5 is tiny
    for (float t : times) {
      std::vector<Rec> out(count), again(a);
      uint32_t flags = 77;
      expect(lumc_shutter_host(a.data(), b.data(), count, t, out.data(), &flags) == 0 && flags == 0, "the twin refused finite records");
      if (t == 0.0f) expect(std::memcmp(out.data(), a.data(), 16 * (size_t) count) == 0, "t = 0 is not the open key");
      if (t == 1.0f) expect(std::memcmp(out.data(), b.data(), 16 * (size_t) count) == 0, "t = 1 is not the close key");
      for (uint32_t c = 0; c < count; c++)
        if (a[c].n == b[c].n) expect(out[c].n == a[c].n, "equal normal words are not kept");
      expect(lumc_shutter_host(again.data(), b.data(), count, t, again.data(), nullptr) == 0 && std::memcmp(again.data(), out.data(), 16 * (size_t) count) == 0,
             "in place gives other bytes");
    }
  }
  {  // a difference that overflows: the flag, and the record is written as computed
    const float big = std::numeric_limits<float>::max();
    const Rec a = {-big, 1.0f, 2.0f, 0x80008000u}, b = {big, 1.0f, 2.0f, 0x80008000u};
    Rec out = {0, 0, 0, 0};
    uint32_t flags = 0;
    expect(lumc_shutter_host(&a, &b, 1, 0.5f, &out, &flags) == 0 && flags == 1 && std::isinf(out.x) && out.y == 1.0f && out.z == 2.0f && out.n == a.n, "the overflowing pair");
    flags = 5;
    expect(lumc_shutter_host(&a, &b, 1, 1.0f, &out, &flags) == 0 && flags == 0 && std::memcmp(&out, &b, 16) == 0, "t = 1 of the overflowing pair is the close key, no flag");
  }
  {  // refusals write nothing
    const Rec a = {1, 2, 3, 4}, b = {5, 6, 7, 8};
    Rec out = {9, 9, 9, 9};
    const Rec before = out;
    uint32_t flags = 42;
    const float bad_t[] = {-0.25f, 1.5f, std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity()};
    for (float t : bad_t) expect(lumc_shutter_host(&a, &b, 1, t, &out, &flags) == 1, "a bad t is taken");
    expect(lumc_shutter_host(nullptr, &b, 1, 0.5f, &out, &flags) == 1 && lumc_shutter_host(&a, nullptr, 1, 0.5f, &out, &flags) == 1 &&
           lumc_shutter_host(&a, &b, 1, 0.5f, nullptr, &flags) == 1, "a NULL array is taken");
    expect(std::memcmp(&out, &before, 16) == 0 && flags == 42, "a refusal wrote something");
  }
  std::printf(g_bad ? "mesh_shutter_check: %d failures\n" : "mesh_shutter_check: ok\n", g_bad);
  return g_bad ? 1 : 0;
}
