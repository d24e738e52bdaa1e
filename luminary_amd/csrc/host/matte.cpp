// The host twin of the matte kernels (matte.hip): matte.h's matte_insert, matte_resolve_pixel and matte_mask_pixel compiled by the host compiler, no HIP in it. It
// defines the bytes the kernels are held to (lum_core.h lumc_matte_host, lumc_matte_mask_host_twin; tests/test_matte.py, tests/test_matte_gpu.py).
#define LUM_MATTE_HOST_ONLY 1
#include "matte.h"

#include <stddef.h>

namespace {

lum::MatteTable load_table(const uint32_t* slots_id, const uint32_t* slots_count, size_t P, size_t p) {
  lum::MatteTable t;
  for (uint32_t k = 0; k < lum::kMatteSlots; k++) { t.id[k] = slots_id[k * P + p]; t.count[k] = slots_count[k * P + p]; }
  t.dropped = 0;
  return t;
}

}  // namespace

// ids [samples][pixels] in ascending sample id, kMatteIdEmpty = the sample has no path. Outputs, each may be NULL: slots_id / slots_count [8][pixels] (an unused slot
// holds kMatteIdEmpty, 0), out_ids / out_coverage [ranks][pixels], dropped / rays [pixels].
extern "C" int lumc_matte_host(const uint32_t* ids, uint32_t samples, uint32_t pixels, uint32_t ranks, uint32_t* slots_id, uint32_t* slots_count, uint32_t* out_ids,
                               float* out_coverage, uint32_t* dropped, uint32_t* rays) {
  if (!ids || samples == 0 || samples > lum::kMatteMaxSamples || ranks == 0 || ranks > lum::kMatteSlots) return 1;
  const size_t P = pixels;
  for (size_t p = 0; p < P; p++) {
    lum::MatteTable t;
    for (uint32_t k = 0; k < lum::kMatteSlots; k++) { t.id[k] = lum::kMatteIdEmpty; t.count[k] = 0; }
    t.dropped = 0;
    for (uint32_t s = 0; s < samples; s++) {
      const uint32_t v = ids[(size_t) s * P + p];
      if (v != lum::kMatteIdEmpty) lum::matte_insert(t, v);
    }
    const lum::MatteRanks r = lum::matte_resolve_pixel(t, samples);
    for (uint32_t k = 0; k < lum::kMatteSlots; k++) {
      if (slots_id) slots_id[k * P + p] = t.id[k];
      if (slots_count) slots_count[k * P + p] = t.count[k];
    }
    for (uint32_t k = 0; k < ranks; k++) {
      if (out_ids) out_ids[k * P + p] = r.id[k];
      if (out_coverage) out_coverage[k * P + p] = r.coverage[k];
    }
    if (dropped) dropped[p] = t.dropped;
    if (rays) rays[p] = r.rays;
  }
  return 0;
}

// slots_id / slots_count [8][pixels], ids [count] (count 0 ... 16), mask [pixels]
extern "C" int lumc_matte_mask_host_twin(const uint32_t* slots_id, const uint32_t* slots_count, uint32_t pixels, uint32_t samples, const uint32_t* ids, uint32_t count,
                                         float* mask) {
  if (!slots_id || !slots_count || !mask || samples == 0 || samples > lum::kMatteMaxSamples || count > lum::kMatteMaxMaskIds || (count && !ids)) return 1;
  lum::MatteIdList list{};
  list.count = count;
  for (uint32_t i = 0; i < count; i++) list.id[i] = ids[i];
  const size_t P = pixels;
  for (size_t p = 0; p < P; p++) mask[p] = lum::matte_mask_pixel(load_table(slots_id, slots_count, P, p), list, samples);
  return 0;
}
