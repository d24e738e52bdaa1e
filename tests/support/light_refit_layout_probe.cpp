// Sizes and field offsets of the light refit's structs (include/lum_core.h) as the compiler lays them out: "name: size offset offset ...", in the order of the
// ctypes mirrors of luminary_amd/core.py. Built and run by tests/test_light_refit.py.
#include <cstddef>
#include <cstdio>

#include "../../include/lum_core.h"

int main() {
  std::printf("LumLightRefitStats: %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(LumLightRefitStats), offsetof(LumLightRefitStats, refits),
              offsetof(LumLightRefitStats, fallbacks), offsetof(LumLightRefitStats, last_launches), offsetof(LumLightRefitStats, last_flags),
              offsetof(LumLightRefitStats, last_bytes_uploaded), offsetof(LumLightRefitStats, last_bytes_downloaded), offsetof(LumLightRefitStats, seconds),
              offsetof(LumLightRefitStats, seconds_fragments), offsetof(LumLightRefitStats, seconds_stats), offsetof(LumLightRefitStats, seconds_nodes),
              offsetof(LumLightRefitStats, seconds_light_bvh), offsetof(LumLightRefitStats, seconds_table), offsetof(LumLightRefitStats, cost_growth));
  std::printf("LumLightRefitReport: %zu %zu %zu %zu %zu\n", sizeof(LumLightRefitReport), offsetof(LumLightRefitReport, refitted), offsetof(LumLightRefitReport, flags),
              offsetof(LumLightRefitReport, cost), offsetof(LumLightRefitReport, cost_growth));
  std::printf("LumLightRefitPlan: %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(LumLightRefitPlan), offsetof(LumLightRefitPlan, fragments), offsetof(LumLightRefitPlan, transforms),
              offsetof(LumLightRefitPlan, transform_instances), offsetof(LumLightRefitPlan, slots), offsetof(LumLightRefitPlan, num_fragments),
              offsetof(LumLightRefitPlan, num_transforms), offsetof(LumLightRefitPlan, num_nodes), offsetof(LumLightRefitPlan, reserved), offsetof(LumLightRefitPlan, root_cost));
  std::printf("LumLightFragment: %zu\nLumLightTransform: %zu\nLumLightSlot: %zu\n", sizeof(LumLightFragment), sizeof(LumLightTransform), sizeof(LumLightSlot));
  return 0;
}
