// plan_update's (csrc/host/update_plan.h) shutter bit, for every input: the twelve dirty bits x lumc_set_mesh_refit_in_place x lumc_set_mesh_refit's mode x
// lumc_set_instance_update's mode x "a pose is pending" x "a light refit plan is bound" x "a shutter time is pending" = 262 144 plans. LUMC_DIRTY_MESH_SHUTTER
// moves something exactly when a time is pending and no new meshes are taken, and then the plan is, field for field, that of a pending pose under
// LUMC_DIRTY_MESH_SKIN - the moved-vertices path without the view's vertices; in every other case the plan is that of the same input without the bit, which
// tests/support/update_plan_check.cpp and light_refit_plan_check.cpp hold to their statements. The defaulted parameter plans nothing.
// Stand-alone: built and run by tests/test_mesh_shutter.py.
#include <cstdio>
#include <cstring>

#include "../../luminary_amd/csrc/host/update_plan.h"

int main() {
  static_assert(LUMC_DIRTY_MESH_SHUTTER == 2048, "the flag's value");
  static_assert((LUMC_DIRTY_ALL & LUMC_DIRTY_MESH_SHUTTER) == 0, "not part of LUMC_DIRTY_ALL");
  int cases = 0, bad = 0;
  for (unsigned dirty = 0; dirty < 4096; dirty++)
    for (uint32_t in_place = 0; in_place < 2; in_place++)
      for (uint32_t refit_mode = 0; refit_mode < 2; refit_mode++)
        for (uint32_t instance_mode = 0; instance_mode < 2; instance_mode++)
          for (int pending = 0; pending < 2; pending++)
            for (int bound = 0; bound < 2; bound++) {
              const unsigned without = dirty & ~(unsigned) LUMC_DIRTY_MESH_SHUTTER;
              const UpdatePlan old = plan_update(without, in_place != 0, refit_mode, instance_mode, pending != 0, bound != 0);
              for (int shutter = 0; shutter < 2; shutter++) {
                const UpdatePlan p = plan_update(dirty, in_place != 0, refit_mode, instance_mode, pending != 0, bound != 0, shutter != 0);
                const bool moves = (dirty & LUMC_DIRTY_MESH_SHUTTER) && shutter && !(dirty & LUMC_DIRTY_MESHES);
                const UpdatePlan want = moves ? plan_update(without | LUMC_DIRTY_MESH_SKIN, in_place != 0, refit_mode, instance_mode, true, bound != 0) : old;
                if (std::memcmp(&want, &p, sizeof(UpdatePlan)) != 0) { std::printf("dirty %u pending %d bound %d shutter %d: another plan than expected\n", dirty, pending, bound, shutter); bad++; }
                if (moves && (!p.positions || (p.upload_view != ((dirty & LUMC_DIRTY_MESH_POSITIONS) != 0)))) { std::printf("dirty %u: the moved-vertices path is not planned as for a pose\n", dirty); bad++; }
                cases++;
              }
              const UpdatePlan defaulted = plan_update(dirty, in_place != 0, refit_mode, instance_mode, pending != 0, bound != 0);
              if (std::memcmp(&defaulted, &old, sizeof(UpdatePlan)) != 0) { std::printf("dirty %u: the bit plans something without a pending time (defaulted parameter)\n", dirty); bad++; }
            }
  std::printf("shutter_plan_check: %d cases, %d disagreements\n", cases, bad);
  return (bad == 0 && cases == 262144) ? 0 : 1;
}
