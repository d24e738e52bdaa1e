// What one lumc_scene_update does, decided once from the caller's dirty flags and the context's modes (scene_device.hip scene_update runs the parts in order under
// `if (plan.x)`). Pure and free of HIP: tests/support/update_plan_check.cpp holds every field, for every input, to the flag statements this replaced.
#pragma once

#include <cstdint>

#include "../../../include/lum_core.h"

struct UpdatePlan {
  bool meshes = false;                // new meshes: vertex arrays, trees and traversal triangles are built as by an upload; every skin binding goes
  bool positions = false;             // the moved-vertices path runs: the view's vertices moved, or a pose or a shutter time is pending (never with `meshes`, which covers both)
  bool upload_view = false;           // ... and it takes the view's vertex arrays over (false: poses alone - the view's vertices are not read)
  bool in_place = false;              // ... and refits in the resident node array; the top level follows on the device
  bool instances = false;             // the host assembles the node array and the leaf records (update_instance_arrays, update_scene_tree)
  bool transforms_on_device = false;  // the device rebuilds the top level in the resident layout (never with `instances`)
  bool instances_moved = false;       // the caller said LUMC_DIRTY_INSTANCE_TRANSFORMS: an in-place update has to upload the transforms, too
  bool moved_by_host = false;         // moved instances under lumc_set_instance_update(1): the host's path, timed into the instance stats
  bool materials = false, lights = false, textures = false, constants = false, particles = false;
  bool full_upload = false;           // every part of LUMC_DIRTY_ALL: the BSDF tables are taken from the caller or generated again
  bool light_positions = false;       // the bound light tree is refitted on the device from the final vertices (never with `lights`)
  bool time_lights = false;           // the lights' share of a moved-vertices update is timed (LumMeshRefitStats::seconds_lights)

  // update_counts_and_tables' two conditions: the triangles' material words are derived again; the light table is (always with new lights, else only if there is one)
  bool tri_opacity(bool triangles_rewritten) const { return meshes || materials || triangles_rewritten; }
  bool light_table_inputs() const { return materials || instances || transforms_on_device || meshes; }

  // This in-place update takes the other path, as it would have run with the switch off: copies of the trees are refitted and the host assembles the node array.
  // (A device update of the top level that takes the host's path changes no field: scene_update runs the host's parts there and then, and the light table sees
  // moved instances either way.)
  void take_copies_path() { in_place = false; transforms_on_device = false; instances = true; }
};

// pose_pending: a bound mesh holds a pose that no update has applied yet (LUMC_DIRTY_MESH_SKIN moves something). light_refit_bound: the context holds a light
// refit plan (lumc_light_refit_bind); without one LUMC_DIRTY_LIGHT_POSITIONS plans nothing (scene_update reports that the lights need a rebuild).
// shutter_pending: a mesh that holds both shutter keys has a time no update has applied yet (lumc_shutter_time): LUMC_DIRTY_MESH_SHUTTER moves it as a pose does.
inline UpdatePlan plan_update(unsigned dirty, bool refit_in_place, uint32_t refit_mode, uint32_t instance_update_mode, bool pose_pending, bool light_refit_bound = false,
                              bool shutter_pending = false) {
  auto has = [dirty](unsigned bits) { return (dirty & bits) != 0; };
  UpdatePlan p;
  p.meshes = has(LUMC_DIRTY_MESHES);  // a full rebuild of the meshes covers moved vertices and poses
  p.upload_view = !p.meshes && has(LUMC_DIRTY_MESH_POSITIONS);
  p.positions = p.upload_view || (!p.meshes && has(LUMC_DIRTY_MESH_SKIN) && pose_pending) || (!p.meshes && has(LUMC_DIRTY_MESH_SHUTTER) && shutter_pending);
  // lumc_set_mesh_refit_in_place: moved vertices alone or with moved instances, both modes 0
  p.in_place = refit_in_place && p.positions && !has(LUMC_DIRTY_INSTANCES) && refit_mode == 0 && instance_update_mode == 0;
  p.instances_moved = has(LUMC_DIRTY_INSTANCE_TRANSFORMS);
  const bool assembled = has(LUMC_DIRTY_INSTANCES) || p.meshes || (p.positions && !p.in_place);  // the assembled node array holds the per-mesh trees; the instance part covers moved instances
  p.moved_by_host = !assembled && p.instances_moved && instance_update_mode == 1;  // mode 1: exactly LUMC_DIRTY_INSTANCES; its time is reported
  p.instances = assembled || p.moved_by_host;
  p.transforms_on_device = !p.instances && (p.instances_moved || p.in_place);
  p.materials = has(LUMC_DIRTY_MATERIALS); p.lights = has(LUMC_DIRTY_LIGHTS); p.textures = has(LUMC_DIRTY_TEXTURES);
  p.particles = has(LUMC_DIRTY_PARTICLES);
  p.constants = has(LUMC_DIRTY_CONSTANTS) || p.particles;
  p.full_upload = p.constants && p.materials && p.instances && p.lights && p.meshes && p.textures && p.particles;
  p.light_positions = !p.lights && !p.meshes && light_refit_bound && has(LUMC_DIRTY_LIGHT_POSITIONS);
  p.time_lights = p.positions;
  return p;
}
