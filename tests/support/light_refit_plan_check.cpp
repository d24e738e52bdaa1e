// plan_update's (csrc/host/update_plan.h) light-refit bit, for every input: the eleven dirty bits x lumc_set_mesh_refit_in_place x lumc_set_mesh_refit's mode x
// lumc_set_instance_update's mode x "a pose is pending" x "a light refit plan is bound" = 65 536 plans over 32 768 inputs without the binding flag. The bit is
// planned exactly when LUMC_DIRTY_LIGHT_POSITIONS is set, a plan is bound and neither new lights nor new meshes are taken; and it changes no other field: the plan
// of every input equals the plan of the same input without the bit (which tests/support/update_plan_check.cpp holds to the statements the plan replaced).
// Stand-alone: built and run by tests/test_light_refit.py.
#include <cstdio>
#include <cstring>

#include "../../luminary_amd/csrc/host/update_plan.h"

int main() {
  int cases = 0, bad = 0;
  for (unsigned dirty = 0; dirty < 2048; dirty++)
    for (uint32_t in_place = 0; in_place < 2; in_place++)
      for (uint32_t refit_mode = 0; refit_mode < 2; refit_mode++)
        for (uint32_t instance_mode = 0; instance_mode < 2; instance_mode++)
          for (int pending = 0; pending < 2; pending++) {
            for (int bound = 0; bound < 2; bound++) {
              const UpdatePlan p = plan_update(dirty, in_place != 0, refit_mode, instance_mode, pending != 0, bound != 0);
              UpdatePlan old = plan_update(dirty & ~(unsigned) LUMC_DIRTY_LIGHT_POSITIONS, in_place != 0, refit_mode, instance_mode, pending != 0);
              const bool want = (dirty & LUMC_DIRTY_LIGHT_POSITIONS) && bound && !(dirty & LUMC_DIRTY_LIGHTS) && !(dirty & LUMC_DIRTY_MESHES);
              if (p.light_positions != want) { std::printf("dirty %u bound %d: light_positions is %d, expected %d\n", dirty, bound, (int) p.light_positions, (int) want); bad++; }
              if (old.light_positions) { std::printf("dirty %u: the bit is planned without being asked for\n", dirty); bad++; }
              old.light_positions = p.light_positions;
              if (std::memcmp(&old, &p, sizeof(UpdatePlan)) != 0) { std::printf("dirty %u bound %d: the bit changes another field of the plan\n", dirty, bound); bad++; }
            }
            const UpdatePlan defaulted = plan_update(dirty, in_place != 0, refit_mode, instance_mode, pending != 0);
            if (defaulted.light_positions) { std::printf("dirty %u: planned without a binding (defaulted parameter)\n", dirty); bad++; }
            cases++;
          }
  std::printf("light_refit_plan_check: %d cases, %d disagreements\n", cases, bad);
  return (bad == 0 && cases == 32768) ? 0 : 1;
}
