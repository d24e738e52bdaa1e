// The matte kernels' host twins (csrc/host/matte.cpp lumc_matte_host, lumc_matte_mask_host_twin) as a program of its own, built with the address and
// undefined-behaviour sanitizers by tests/test_matte.py: random id streams over alphabets of 1 ... 20 ids with reserved ids and samples without a path, for the
// suite's sample counts and every rank count; the invariant sum of counts + dropped = rays; ranks in non-increasing count with ties in ascending id; optional
// outputs; the mask of a pixel's own ids; what the twins refuse writes nothing. Arrays are sized exactly, so a write past [ranks][pixels] is caught.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

extern "C" int lumc_matte_host(const uint32_t* ids, uint32_t samples, uint32_t pixels, uint32_t ranks, uint32_t* slots_id, uint32_t* slots_count, uint32_t* out_ids,
                               float* out_coverage, uint32_t* dropped, uint32_t* rays);
extern "C" int lumc_matte_mask_host_twin(const uint32_t* slots_id, const uint32_t* slots_count, uint32_t pixels, uint32_t samples, const uint32_t* ids, uint32_t count,
                                         float* mask);

namespace {
constexpr uint32_t kEmpty = 0xFFFFFFFFu, kSlots = 8;
uint32_t g_state = 2463534242u;
uint32_t rnd() { g_state = g_state * 1664525u + 1013904223u; return g_state >> 8; }
int g_bad = 0;
void expect(bool ok, const char* what) { if (!ok) { std::printf("matte_check: %s\n", what); g_bad++; } }
}  // namespace

int main() {
  const uint32_t alphabets[] = {1, 3, 8, 9, 20}, sample_counts[] = {1, 5, 16, 64, 1024};
  const uint32_t reserved[] = {0xFFFFFFFEu, 0xFFFFFFFDu, 0xFFFFFFFCu};
  for (uint32_t A : alphabets)
    for (uint32_t S : sample_counts)
      for (uint32_t R = 1; R <= kSlots; R++) {
        const uint32_t P = 67;
        std::vector<uint32_t> alphabet(A);
        for (uint32_t a = 0; a < A; a++) alphabet[a] = a < 3 && A > 3 ? reserved[a] : rnd() % 1000u;
        std::vector<uint32_t> ids((size_t) S * P), has_path(P, 0);
        for (uint32_t s = 0; s < S; s++)
          for (uint32_t p = 0; p < P; p++) {
            const bool none = p % 5 == 1 ? true : (rnd() % 7 == 0);
            ids[(size_t) s * P + p] = none ? kEmpty : alphabet[rnd() % A];
            has_path[p] += none ? 0u : 1u;
          }
        std::vector<uint32_t> slots_id(kSlots * P, 7), slots_count(kSlots * P, 7), out_ids((size_t) R * P, 7), dropped(P, 7), rays(P, 7);
        std::vector<float> coverage((size_t) R * P, -1.0f);
        expect(lumc_matte_host(ids.data(), S, P, R, slots_id.data(), slots_count.data(), out_ids.data(), coverage.data(), dropped.data(), rays.data()) == 0, "the twin refused its arguments");
        for (uint32_t p = 0; p < P; p++) {
          uint32_t sum = dropped[p], occupied = 0;
          for (uint32_t k = 0; k < kSlots; k++) {
            sum += slots_count[k * P + p];
            occupied += slots_count[k * P + p] ? 1u : 0u;
            if (!slots_count[k * P + p]) expect(slots_id[k * P + p] == kEmpty, "an unused slot does not hold EMPTY");
            else expect(slots_id[k * P + p] != kEmpty, "a used slot holds EMPTY");
          }
          expect(sum == has_path[p] && rays[p] == has_path[p], "sum of counts + dropped is not the number of samples with a path");
          if (A <= kSlots) expect(dropped[p] == 0, "eight ids or fewer dropped a sample");
          for (uint32_t r = 0; r < R; r++) {
            const float c = coverage[(size_t) r * P + p];
            if (r >= occupied) { expect(out_ids[(size_t) r * P + p] == kEmpty && c == 0.0f, "a rank beyond the occupied slots is not EMPTY / 0"); continue; }
            expect(c > 0.0f && c <= 1.0f, "a coverage outside (0, 1]");
            if (r > 0) {
              const float before = coverage[(size_t) (r - 1) * P + p];
              expect(before > c || (before == c && out_ids[(size_t) (r - 1) * P + p] < out_ids[(size_t) r * P + p]), "ranks are not in order");
            }
          }
        }
        // the optional outputs, one at a time, give what the full call gave
        std::vector<uint32_t> again((size_t) R * P, 7);
        expect(lumc_matte_host(ids.data(), S, P, R, nullptr, nullptr, again.data(), nullptr, nullptr, nullptr) == 0 && again == out_ids, "ids alone differ");
        std::vector<uint32_t> rays2(P, 7);
        expect(lumc_matte_host(ids.data(), S, P, R, nullptr, nullptr, nullptr, nullptr, nullptr, rays2.data()) == 0 && rays2 == rays, "rays alone differ");
        // the mask of a pixel's own slot ids, sixteen at most: everything but what was dropped
        std::vector<float> mask(P, -1.0f);
        for (uint32_t p = 0; p < P; p += 13) {
          uint32_t own[16];
          for (uint32_t k = 0; k < 16; k++) own[k] = slots_id[(k % kSlots) * P + p];
          expect(lumc_matte_mask_host_twin(slots_id.data(), slots_count.data(), P, S, own, 16, mask.data()) == 0, "the mask twin refused its arguments");
          expect(mask[p] == (float) (has_path[p] - dropped[p]) / (float) S, "the mask of a pixel's own ids");
        }
        expect(lumc_matte_mask_host_twin(slots_id.data(), slots_count.data(), P, S, nullptr, 0, mask.data()) == 0, "an empty list is refused");
        for (uint32_t p = 0; p < P; p++) expect(mask[p] == 0.0f, "the mask of no ids is not 0");
      }
  {  // refusals write nothing
    const uint32_t ids[4] = {1, 2, 1, 2};
    uint32_t si[16], sc[16], oi[2] = {42, 42}, d[2] = {42, 42}, r[2] = {42, 42};
    float cov[2] = {42.0f, 42.0f}, mask[2] = {42.0f, 42.0f};
    std::memset(si, 0x2A, sizeof(si)); std::memset(sc, 0x2A, sizeof(sc));
    expect(lumc_matte_host(nullptr, 2, 2, 1, si, sc, oi, cov, d, r) == 1, "NULL ids are taken");
    expect(lumc_matte_host(ids, 0, 2, 1, si, sc, oi, cov, d, r) == 1 && lumc_matte_host(ids, 1025, 2, 1, si, sc, oi, cov, d, r) == 1, "a bad sample count is taken");
    expect(lumc_matte_host(ids, 2, 2, 0, si, sc, oi, cov, d, r) == 1 && lumc_matte_host(ids, 2, 2, 9, si, sc, oi, cov, d, r) == 1, "a bad rank count is taken");
    expect(oi[0] == 42 && cov[1] == 42.0f && d[0] == 42 && r[1] == 42 && si[3] == 0x2A2A2A2Au && sc[15] == 0x2A2A2A2Au, "a refusal wrote something");
    uint32_t many[17] = {0};
    expect(lumc_matte_mask_host_twin(si, sc, 2, 2, many, 17, mask) == 1 && lumc_matte_mask_host_twin(nullptr, sc, 2, 2, many, 1, mask) == 1 &&
           lumc_matte_mask_host_twin(si, nullptr, 2, 2, many, 1, mask) == 1 && lumc_matte_mask_host_twin(si, sc, 2, 2, many, 1, nullptr) == 1 &&
           lumc_matte_mask_host_twin(si, sc, 2, 2, nullptr, 1, mask) == 1 && lumc_matte_mask_host_twin(si, sc, 2, 0, many, 1, mask) == 1, "the mask twin takes bad arguments");
    expect(mask[0] == 42.0f && mask[1] == 42.0f, "a refused mask wrote something");
  }
  std::printf(g_bad ? "matte_check: %d failures\n" : "matte_check: ok\n", g_bad);
  return g_bad ? 1 : 0;
}
