// plan_update (csrc/host/update_plan.h) against the flag statements it replaced, for every input: the ten dirty bits x lumc_set_mesh_refit_in_place x
// lumc_set_mesh_refit's mode x lumc_set_instance_update's mode x "a pose is pending" = 16 384 cases. parent_flags() is the specification: scene_update's
// statements from the LUMC_DIRTY_MESHES mask down to `instances = ...`, and what its two fallback branches assigned, as they stood before the plan, word for
// word (`ctx` is a stand-in with the fields they read). Stand-alone: built with the sanitizers by tests/test_update_plan.py.
#include <cstdio>
#include <map>
#include <vector>

#include "../../luminary_amd/csrc/host/update_plan.h"

namespace {

struct Skin { std::vector<float> pending; };
struct Stats { double seconds = 0.0, seconds_relayout = 0.0, seconds_upload = 0.0, seconds_boxes = 0.0, seconds_build = 0.0, seconds_leaves = 0.0; };
struct Context {
  uint32_t refit_in_place = 0, refit_mode = 0, instance_update_mode = 0;
  std::map<uint32_t, Skin> mesh_skin;
  Stats instance_stats;
};

enum Fallback { kNone, kInPlace, kTopLevel };

struct ParentFlags {
  unsigned dirty;  // as the later consumers read it: update_counts_and_tables, update_constants (dirty == LUMC_DIRTY_ALL), time_lights
  bool upload_view, in_place, instances_moved, moved_by_host, meshes, lights, instances;
};

ParentFlags parent_flags(Context* ctx, unsigned dirty, Fallback fallback) {
  if (dirty & LUMC_DIRTY_MESHES) dirty &= ~(unsigned) (LUMC_DIRTY_MESH_POSITIONS | LUMC_DIRTY_MESH_SKIN);  // a full rebuild of the meshes covers moved vertices
  const bool upload_view = (dirty & LUMC_DIRTY_MESH_POSITIONS) != 0;
  if (dirty & LUMC_DIRTY_MESH_SKIN) {
    bool pending = false;
    for (const auto& kv : ctx->mesh_skin) pending = pending || !kv.second.pending.empty();
    dirty &= ~(unsigned) LUMC_DIRTY_MESH_SKIN;
    if (pending) dirty |= LUMC_DIRTY_MESH_POSITIONS;
  }
  bool in_place = ctx->refit_in_place && (dirty & LUMC_DIRTY_MESH_POSITIONS) && !(dirty & (LUMC_DIRTY_MESHES | LUMC_DIRTY_INSTANCES)) && ctx->refit_mode == 0 && ctx->instance_update_mode == 0;
  const bool instances_moved = (dirty & LUMC_DIRTY_INSTANCE_TRANSFORMS) != 0;
  if (in_place) dirty |= LUMC_DIRTY_INSTANCE_TRANSFORMS;
  else if (dirty & (LUMC_DIRTY_MESHES | LUMC_DIRTY_MESH_POSITIONS)) dirty |= LUMC_DIRTY_INSTANCES;  // the assembled node array holds the per-mesh trees
  if (dirty & LUMC_DIRTY_PARTICLES) dirty |= LUMC_DIRTY_CONSTANTS;
  if (dirty & (LUMC_DIRTY_INSTANCES | LUMC_DIRTY_MESHES)) dirty &= ~(unsigned) LUMC_DIRTY_INSTANCE_TRANSFORMS;  // the instance part covers moved instances
  const bool moved_by_host = (dirty & LUMC_DIRTY_INSTANCE_TRANSFORMS) && ctx->instance_update_mode == 1;  // mode 1: exactly LUMC_DIRTY_INSTANCES; its time is reported
  if (moved_by_host) { dirty = (dirty & ~(unsigned) LUMC_DIRTY_INSTANCE_TRANSFORMS) | LUMC_DIRTY_INSTANCES; ctx->instance_stats.seconds = ctx->instance_stats.seconds_relayout = ctx->instance_stats.seconds_upload = ctx->instance_stats.seconds_boxes = ctx->instance_stats.seconds_build = ctx->instance_stats.seconds_leaves = 0.0; }
  const bool meshes = (dirty & LUMC_DIRTY_MESHES) != 0, lights = (dirty & LUMC_DIRTY_LIGHTS) != 0;
  bool instances = (dirty & LUMC_DIRTY_INSTANCES) != 0;
  if (fallback == kInPlace) {  // refit_in_place fell back: this one update by the other path, as it would have run with the switch off
      in_place = false;
      dirty = (dirty & ~(unsigned) LUMC_DIRTY_INSTANCE_TRANSFORMS) | LUMC_DIRTY_INSTANCES;
      instances = true;
  }
  if (fallback == kTopLevel) {  // update_instance_transforms fell back: the branch ran the host's parts itself and assigned none of these
  }
  return ParentFlags{dirty, upload_view, in_place, instances_moved, moved_by_host, meshes, lights, instances};
}

// Every field of the plan, and update_counts_and_tables' two conditions (either value of `triangles_rewritten`, the bit the parent or-ed into dirty as
// kDirtyTrianglesRewritten = 1 << 30), against the parent's flags. Returns the number of disagreements, each printed.
int compare(const char* where, unsigned dirty, const Context& c, bool pending, const UpdatePlan& p, const ParentFlags& f) {
  int bad = 0;
  auto same = [&](const char* what, bool plan, bool parent) {
    if (plan == parent) return;
    std::printf("%s: dirty %u in_place %u refit_mode %u instance_update_mode %u pending %d: %s is %d, the parent's statements give %d\n", where, dirty, c.refit_in_place, c.refit_mode,
                c.instance_update_mode, (int) pending, what, (int) plan, (int) parent);
    bad++;
  };
  same("meshes", p.meshes, f.meshes);
  same("positions", p.positions, (f.dirty & LUMC_DIRTY_MESH_POSITIONS) != 0);
  same("upload_view", p.upload_view, f.upload_view);
  same("in_place", p.in_place, f.in_place);
  same("instances", p.instances, f.instances);
  same("instances (the bit)", p.instances, (f.dirty & LUMC_DIRTY_INSTANCES) != 0);
  same("transforms_on_device", p.transforms_on_device, (f.dirty & LUMC_DIRTY_INSTANCE_TRANSFORMS) != 0);
  same("instances_moved", p.instances_moved, f.instances_moved);
  same("moved_by_host", p.moved_by_host, f.moved_by_host);
  same("materials", p.materials, (f.dirty & LUMC_DIRTY_MATERIALS) != 0);
  same("lights", p.lights, f.lights);
  same("lights (the bit)", p.lights, (f.dirty & LUMC_DIRTY_LIGHTS) != 0);
  same("textures", p.textures, (f.dirty & LUMC_DIRTY_TEXTURES) != 0);
  same("constants", p.constants, (f.dirty & LUMC_DIRTY_CONSTANTS) != 0);
  same("particles", p.particles, (f.dirty & LUMC_DIRTY_PARTICLES) != 0);
  same("full_upload", p.full_upload, f.dirty == LUMC_DIRTY_ALL);
  same("time_lights", p.time_lights, (f.dirty & LUMC_DIRTY_MESH_POSITIONS) != 0);
  same("no skin bit is left", false, (f.dirty & LUMC_DIRTY_MESH_SKIN) != 0);
  constexpr unsigned kDirtyTrianglesRewritten = 1u << 30;
  for (int rewritten = 0; rewritten < 2; rewritten++) {
    const unsigned d = f.dirty | (rewritten ? kDirtyTrianglesRewritten : 0u);
    same("tri_opacity", p.tri_opacity(rewritten != 0), (d & (LUMC_DIRTY_MESHES | LUMC_DIRTY_MATERIALS | kDirtyTrianglesRewritten)) != 0);
    if (rewritten && (f.dirty & LUMC_DIRTY_MESH_POSITIONS)) same("full_upload beside rewritten triangles", p.full_upload, d == LUMC_DIRTY_ALL);  // (only the moved-vertices path rewrites them)
  }
  same("light_table_inputs", p.light_table_inputs(), (f.dirty & (LUMC_DIRTY_MATERIALS | LUMC_DIRTY_INSTANCES | LUMC_DIRTY_INSTANCE_TRANSFORMS | LUMC_DIRTY_MESHES)) != 0);
  return bad;
}

}  // namespace

int main() {
  int cases = 0, agree = 0;
  for (unsigned dirty = 0; dirty < 1024; dirty++)
    for (uint32_t in_place = 0; in_place < 2; in_place++)
      for (uint32_t refit_mode = 0; refit_mode < 2; refit_mode++)
        for (uint32_t instance_mode = 0; instance_mode < 2; instance_mode++)
          for (int pending = 0; pending < 2; pending++) {
            Context c;
            c.refit_in_place = in_place; c.refit_mode = refit_mode; c.instance_update_mode = instance_mode;
            c.mesh_skin[3] = Skin{};  // a bound mesh without a pose, and one with
            if (pending) c.mesh_skin[7].pending.assign(12, 1.0f);
            const UpdatePlan plan = plan_update(dirty, in_place != 0, refit_mode, instance_mode, pending != 0);
            int bad = compare("plan", dirty, c, pending != 0, plan, parent_flags(&c, dirty, kNone));
            UpdatePlan copies = plan;
            copies.take_copies_path();  // (the parent's branch is reached only with in_place; the statements are held for every input all the same)
            bad += compare("after the in-place fallback", dirty, c, pending != 0, copies, parent_flags(&c, dirty, kInPlace));
            bad += compare("after the top level's fallback", dirty, c, pending != 0, plan, parent_flags(&c, dirty, kTopLevel));
            cases++;
            if (!bad) agree++;
          }
  std::printf("update_plan_check: %d of %d cases agree\n", agree, cases);
  if (agree != cases || cases != 16384) return 1;
  std::printf("update_plan_check: ok\n");
  return 0;
}
