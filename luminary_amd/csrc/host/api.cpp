// Implementation of the Luminary C host API (include/luminary_amd.h) on top of the host scene store and the HIP core.
// Reference behaviour: src/luminary/host/host.c (function by function, cited below), src/luminary/luminary.c:7-31,
// src/luminary/path.c, src/luminary/error.c. The reference runs these calls through a Host queue thread and a Device queue
// thread. Here scene edits are applied on the caller's thread under the host's mutex, and rendering happens either
//   * asynchronously, as in the reference: luminary_host_start_new_render starts the host's "Device" worker thread, which renders sample
//     allocation after sample allocation (restarting by itself whenever an edit dirties the integration) and produces the outputs that
//     are due, while the frontend only polls luminary_host_try_await_output / luminary_host_acquire_output (mandarin_duck.c:140-244); or
//   * synchronously inside the additive luminary_ext_render* calls (tests, batch tools), when no render was started.
// (DESIGN.md "Threading".)
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cfloat>
#include <chrono>
#include <condition_variable>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <thread>
#include <type_traits>
#include <string>
#include <vector>

#include "../../../include/lum_core.h"
#include "../../../include/luminary_amd.h"
#include "bvh_build.h"  // host_parallel_for
#include "loaders.h"
#include "scene.h"
#define LUM_DEFORM_HOST_ONLY 1  // the host twin's declaration only: this unit touches no device
#include "light_refit.h"
#include "mesh_deform.h"

extern "C" const unsigned char lum_embedded_bluenoise_2d[];
extern "C" const unsigned char lum_embedded_bluenoise_2d_end[];

#include "output.h"

struct LuminaryPath { std::string value; };

// A bound mesh (luminary_ext_bind_mesh_skin): the rest pose and the corners' bones, the last pose, and who holds it. The serials are values of the host's
// skin_serial counter: a context that has seen the counter at a smaller value gets the binding / the pose before it takes the scene.
// A mesh has ONE rest shape, whichever of the two kinds of binding it holds (luminary_ext_bind_mesh_morph: DESIGN.md section 12): the first binding of either kind
// copies the host mesh, the other kind shares that copy, and the entry lives until the last of the two is unbound.
struct HostSkin {
  std::vector<float> rest_positions, rest_normals, weights;
  std::vector<uint16_t> bone_ids;
  uint32_t bone_count = 0;        // 0: no skin is bound (then a morph is)
  std::vector<float> palette;     // the last pose, 12 floats per bone (empty: none yet)
  uint64_t bind_serial = 0, pose_serial = 0;
  // the morph targets as the caller gave them (what a context is bound to) and as the corner-major rows the host twin walks
  uint32_t target_count = 0;      // 0: no morph is bound
  std::vector<uint32_t> morph_offsets, morph_corners;
  std::vector<float> morph_delta_positions, morph_delta_normals;  // (the normals' empty: zero)
  lum::MorphCsr morph_csr;
  std::vector<float> morph_weights;  // the last weights, target_count floats (zeros until the first call)
  uint64_t morph_bind_serial = 0, morph_weights_serial = 0;  // (weights_serial 0: none set yet)
  bool host_current = true;       // HostMesh::positions / normals hold the last pose (false: brought up to date by the host twin before anything reads them)
  bool view_current = true;       // ... and so do the device scene's vertices of the mesh (the contexts never read those of a posed mesh)
  bool has_skin() const { return bone_count != 0; }
  bool has_morph() const { return target_count != 0; }
  bool posed() const { return has_skin() && !palette.empty(); }
  bool weighted() const { return has_morph() && morph_weights_serial != 0; }
};

// The shutter (luminary_ext_shutter_open ... luminary_ext_render_shutter): what the host remembers of the open key, what was edited since,
// and - once a shutter render has run - what the slices blend between, for as long as nothing is edited.
struct HostShutter {
  struct Pose { LuminaryVec3 position, rotation, scale; };
  bool open = false;            // an open key is held and edits are recorded
  bool synced = false;          // ... and every enabled device held the open scene when it was taken
  bool keyed = false;           // the contexts hold both keys of `meshes`: a shutter render ran and nothing was edited since
  uint32_t edits = 0;           // LUMC_DIRTY_* bits of the edits since the shutter opened (a move's own LUMC_DIRTY_LIGHTS left out: emitter_needs_refit stands for it)
  bool in_move = false;         // the next invalidate belongs to a move of vertices or instances
  bool emitter_needs_refit = false;  // an emitter moved while luminary_ext_set_light_refit is off: the light tree would have to be built per slice
  std::string other;            // the first change since then that the shutter cannot blend (empty: none)
  LuminaryVec3 camera_pos{}, camera_rotation{};  // the open key's
  std::vector<Pose> instances;  // the open key's, by instance
  std::vector<uint32_t> meshes;           // meshes that moved between the keys
  std::vector<uint32_t> moved_instances;  // instances whose position, rotation or scale differs between the keys
  bool camera_moved = false;
  uint32_t slice_dirty = 0;     // what a slice's lumc_scene_update takes
  LuminaryShutterStats stats{};
};

struct LuminaryHost {
  lum::HostScene scene;
  HostShutter shutter;
  std::map<uint32_t, HostSkin> skins;  // by mesh
  uint64_t skin_serial = 0;            // counts binds and poses
  uint64_t core_skin_seen = 0;         // the counter when the main context last took bindings and poses over
  uint64_t host_materialisations = 0;
  lum::DeviceSceneBuffers device_scene;
  // Which parts of the scene edits have touched since the device scene / a device's copy of it was last brought up to date (LUMC_DIRTY_*; the
  // reference keeps such flags per entity, scene.h:42-63, and its device manager uploads by them, device_manager.c:311-320, :424-450): a camera
  // move re-encodes and re-uploads nothing but constants, a material edit the material array, an instance edit the top-level tree.
  uint32_t scene_dirty = LUMC_DIRTY_ALL;  // parts of `device_scene` that are out of date
  uint32_t core_dirty = LUMC_DIRTY_ALL;   // parts the main device's context has not taken over yet
  std::vector<uint32_t> moved_meshes;     // meshes luminary_ext_set_mesh_positions moved since `device_scene` was last brought up to date
  uint32_t refit_mode = 0;                // luminary_ext_set_mesh_refit: handed to every context before it takes a scene
  float refit_max_cost_growth = 0.0f;
  uint32_t instance_update_mode = 0;      // luminary_ext_set_instance_update: likewise
  uint32_t refit_in_place = 0;            // luminary_ext_set_mesh_refit_in_place: likewise
  uint32_t light_refit = 0;               // luminary_ext_set_light_refit: moved emitters refit the light tree on the devices (remembered across uploads)
  float light_refit_max_cost_growth = 0.0f;
  bool view_lights_stale = false;         // the devices refitted their light trees since `device_scene`'s light arrays were made: brought up to date when something reads them
  uint64_t light_rebuilds = 0;            // times a device asked for a rebuild of the light tree and the host built it
  bool device_scene_valid = false;
  bool core_scene_valid = false;
  uint32_t core_width = 0, core_height = 0;  // frame size the main context's pixel set was made for
  LumContext* core = nullptr;        // context of the main device: renders (its tiles) and produces every output
  int device_ordinal = 0;            // HIP ordinal of the main device
  // every visible device (device_manager.c:776-862 creates one Device per masked id); the frame is tiled over the enabled ones
  struct DeviceSlot { int ordinal = 0; bool enabled = false; LumContext* core = nullptr; bool scene_valid = false; uint32_t dirty = LUMC_DIRTY_ALL; uint64_t skin_seen = 0; };
  std::vector<DeviceSlot> devices;
  uint32_t main_slot = 0;
  uint32_t partition_n = 0;          // devices the current accumulation is tiled over (0 or 1: the main device renders every pixel)
  bool comm_ready = false;           // the slots of the current partition share an RCCL communicator
  bool handoff_preview = false;      // the frame's first sample sits on the main device (undersampling preview): the tiles take it over when they are dealt
  std::vector<uint32_t> pixels;  // pixel set of the current accumulation
  bool pixels_all = true;
  uint32_t num_pixels = 0;
  uint32_t accumulated_samples = 0;  // uniform rendering: samples per pixel; adaptive rendering: executions (the reference's sample count)
  bool adaptive_active = false;      // the accumulation is driven by lumc_adaptive_* (luminary_ext_render with adaptive sampling enabled)
  LuminaryDenoiserSettings denoiser = {false, 4u, 5u, 4.0f, 128.0f, 1.0f};  // luminary_ext_set_denoiser
  bool guides_valid = false;         // the main context holds the denoiser's guides of the current accumulation
  bool mattes_valid = false;         // the main context holds ID mattes of the scene as it is (luminary_ext_render_mattes): any edit drops them
  uint64_t matte_renders = 0;
  LuminaryFireflySettings firefly = {false, 8u};  // luminary_ext_set_firefly_rejection
  uint32_t core_firefly = 0;         // buckets the main context holds (sync_firefly): 0 while the switch is off or the frame is tiled over several devices
  uint64_t firefly_resolved = 0, firefly_skipped = 0;  // result images resolved / left alone because adaptive sampling drives the accumulation
  LuminaryHistorySettings history = {false, 32.0f, 0.02f, 0.9f, 0.0f};  // luminary_ext_set_history
  bool history_carry_due = false;      // the integration restarted by camera moves alone since the main context's state was shown: the next output reprojects it
  bool history_camera_move = false;    // luminary_host_set_camera is about to invalidate for a move that carries (camera_change_carries)
  LuminaryHistoryMotionSettings history_motion = {false, 8.0f};  // luminary_ext_set_history_motion
  bool history_carry_instances = false;  // the carry that is due was granted, at least once, for a move of instances: it needs the motion form
  bool history_instance_move = false;  // luminary_ext_set_instance_transforms is about to invalidate for a move that carries (no moved instance emits, motion is on)
  const char* history_cause = nullptr; // what the caller of the next invalidate names as the cause of a drop
  uint64_t history_carried = 0, history_dropped = 0, history_skipped = 0;
  std::string history_last_drop;
  bool hdri_origin_pending = true;   // the next scene build re-bakes the sky panorama from the camera's position (SCENE_DIRTY_FLAG_HDRI)
  lum::OutputStore outputs;
  double render_seconds = 0.0;
  double last_sample_ms = 0.0;  // wall time of the most recent render chunk per sample allocation, in milliseconds (device_sampletime.c)
  std::vector<std::string> log;
  std::mutex mutex;
  // ---- asynchronous rendering: the "Device" queue worker (device_manager.c:127-148, :874) ----
  std::thread worker;
  std::mutex worker_mutex;             // guards the four flags below
  std::condition_variable worker_cv;
  bool worker_started = false, worker_stop = false;
  bool async_active = false;           // a render was started and not stopped
  bool async_failed = false;           // the last iteration failed: wait for the next edit or start instead of spinning
  std::atomic<int> api_waiting{0};     // callers waiting for `mutex`: the worker lets them in between two iterations
  LuminaryThreadStatus* status_host = nullptr;    // queue worker 0 "Host" (edits are applied on the caller's thread: always idle)
  LuminaryThreadStatus* status_device = nullptr;  // queue worker 1 "Device"
};

// Lock of the host's mutex taken by API calls: announces itself so that the render worker, which would otherwise re-take the mutex at
// once, yields between two iterations (std::mutex makes no fairness promise).
struct ApiLock {
  LuminaryHost* h;
  explicit ApiLock(LuminaryHost* host) : h(host) { h->api_waiting.fetch_add(1); h->mutex.lock(); h->api_waiting.fetch_sub(1); }
  ~ApiLock() { h->mutex.unlock(); }
  ApiLock(const ApiLock&) = delete;
  ApiLock& operator=(const ApiLock&) = delete;
};

namespace {

std::vector<uint32_t> embedded_bluenoise() {
  const size_t bytes = (size_t) (lum_embedded_bluenoise_2d_end - lum_embedded_bluenoise_2d);
  std::vector<uint32_t> v(bytes / 4);
  std::memcpy(v.data(), lum_embedded_bluenoise_2d, v.size() * 4);
  return v;
}

// What an edit that moves an emissive triangle marks: the light tree is built again on the host (the default), or - luminary_ext_set_light_refit - refitted on
// the devices.
uint32_t moved_emitter_bit(const LuminaryHost* h) { return h->light_refit ? LUMC_DIRTY_LIGHT_POSITIONS : LUMC_DIRTY_LIGHTS; }

// The contexts' keys go: any edit after a shutter render restarts the integration as it always did.
void shutter_drop_keys(LuminaryHost* h) {
  if (!h->shutter.keyed) return;
  for (uint32_t m : h->shutter.meshes) {
    if (h->core) (void) lumc_mesh_shutter_drop(h->core, m);
    for (uint32_t i = 0; i < h->devices.size(); i++)
      if (i != h->main_slot && h->devices[i].core) (void) lumc_mesh_shutter_drop(h->devices[i].core, m);
  }
  h->shutter.keyed = false;
}
void shutter_cancel(LuminaryHost* h) {
  shutter_drop_keys(h);
  h->shutter.open = false; h->shutter.synced = false; h->shutter.edits = 0; h->shutter.other.clear(); h->shutter.in_move = false; h->shutter.emitter_needs_refit = false;
  h->shutter.meshes.clear(); h->shutter.moved_instances.clear(); h->shutter.camera_moved = false; h->shutter.slice_dirty = 0;
}
void shutter_note_other(LuminaryHost* h, const char* what) {
  if (h->shutter.open && h->shutter.other.empty()) h->shutter.other = what;
}
void shutter_note_mesh(LuminaryHost* h, uint32_t mesh) {
  std::vector<uint32_t>& m = h->shutter.meshes;
  if (h->shutter.open && std::find(m.begin(), m.end(), mesh) == m.end()) m.push_back(mesh);
}

// A move of vertices or instances is about to invalidate: it marks the lights' part whether or not an emitter moved (moved_emitter_bit). Without the light refit a
// moved emitter cannot be blended; a move of something that does not emit leaves the lights as they are in every slice.
void shutter_note_move(LuminaryHost* h, bool emits) {
  if (!h->shutter.open) return;
  h->shutter.in_move = true;
  if (emits && !h->light_refit) h->shutter.emitter_needs_refit = true;
}

// ---- image history (include/luminary_amd.h LuminaryHistorySettings) ----
bool history_held(const LuminaryHost* h) { return h->core && lumc_has_history(h->core); }
// The main context's state and carried plane go, with the reason logged and counted (`why` is a literal: the core keeps the pointer).
void history_drop(LuminaryHost* h, const char* why) {
  h->history_carry_due = false; h->history_carry_instances = false;
  if (!history_held(h)) return;
  (void) lumc_history_drop(h->core, why);
  h->history_dropped++;
  h->history_last_drop = why;
  h->log.push_back(std::string("image history dropped: ") + why);
}
// The guides of the current accumulation, as the denoiser makes them; while the history's motion is on, the owner plane from the same first hits too.
bool history_motion_on(const LuminaryHost* h) { return h->history.enabled && h->history_motion.enabled; }
int render_guides(LuminaryHost* h) {
  LumHistoryMotionParams mp;
  mp.enabled = history_motion_on(h) ? 1u : 0u; mp.motion_max_history = h->history_motion.motion_max_history;
  if (lumc_set_history_motion(h->core, &mp)) return 1;
  if (!mp.enabled) return lumc_render_guides(h->core, h->denoiser.guide_samples, nullptr);
  return lumc_render_first_hits(h->core, h->denoiser.guide_samples, LUMC_FIRST_HIT_GUIDES | LUMC_FIRST_HIT_OWNER, 0u, nullptr);
}
// A restart of the integration: it carries when its caller said that its sole cause is a camera move that does, or - with the motion on - a move of instances
// that does (nothing beside the instance transforms is dirty but the lights' part every move marks, and the shown frame holds the transforms it was shown with),
// and drops otherwise.
void history_restart(LuminaryHost* h, uint32_t dirty) {
  const char* cause = h->history_cause;
  const bool move = h->history_camera_move, instances = h->history_instance_move;
  h->history_cause = nullptr; h->history_camera_move = false; h->history_instance_move = false;
  if (!history_held(h)) return;
  if (move && h->history.enabled) { h->history_carry_due = true; return; }
  // (the physical camera is not reprojected: under it an instance move drops as it always did)
  if (instances && history_motion_on(h) && !h->scene.camera.use_physical_camera &&
      dirty == (LUMC_DIRTY_INSTANCE_TRANSFORMS | (dirty & (LUMC_DIRTY_LIGHTS | LUMC_DIRTY_LIGHT_POSITIONS))) && lumc_has_history_snapshot(h->core)) {
    h->history_carry_due = true; h->history_carry_instances = true;
    return;
  }
  if (!cause) {
    if (dirty == 0) cause = "the device partition or a setting of the accumulation changed";
    else if (dirty == LUMC_DIRTY_ALL) cause = "the scene changed";
    else if (dirty & (LUMC_DIRTY_MESHES | LUMC_DIRTY_MESH_POSITIONS)) cause = "a mesh changed";
    else if (dirty & (LUMC_DIRTY_INSTANCES | LUMC_DIRTY_INSTANCE_TRANSFORMS)) cause = "an instance changed";
    else if (dirty & LUMC_DIRTY_MATERIALS) cause = "a material changed";
    else cause = "the scene changed";
  }
  history_drop(h, cause);
}

void invalidate(LuminaryHost* h, uint32_t dirty = LUMC_DIRTY_ALL) {
  shutter_drop_keys(h);
  history_restart(h, dirty);
  if (h->shutter.open) {
    h->shutter.edits |= h->shutter.in_move ? dirty & ~(uint32_t) LUMC_DIRTY_LIGHTS : dirty;
    h->shutter.in_move = false;
    if (dirty == 0) shutter_note_other(h, "the device partition");
  }
  h->scene_dirty |= dirty; h->core_dirty |= dirty;
  // An adaptive accumulation ends with the edit. The context leaves adaptive mode in lumc_set_pixels only, and an unchanged frame size would keep the
  // pixel set (ensure_core): without this, a uniform render after `enable_adaptive_sampling = false` ran on a context whose result image still
  // normalised by the stale per-block sample counts.
  if (h->adaptive_active) h->num_pixels = 0;
  h->device_scene_valid = false; h->core_scene_valid = false; h->accumulated_samples = 0; h->adaptive_active = false;
  h->guides_valid = false; h->mattes_valid = false;
  for (auto& slot : h->devices) { slot.scene_valid = false; slot.dirty |= dirty; }
  { std::lock_guard<std::mutex> l(h->worker_mutex); h->async_failed = false; }  // the edit may have repaired what failed
  h->worker_cv.notify_all();
}

#define CHECK_NULL(p) do { if (!(p)) return LUMINARY_ERROR_ARGUMENT_NULL; } while (0)

// Does a change of the camera / the renderer settings restart the integration (SCENE_DIRTY_FLAG_INTEGRATION), or does it only change how
// the accumulated frame is shown (SCENE_DIRTY_FLAG_OUTPUT)? camera_check_for_dirty (camera.c:80-147), settings_check_for_dirty
// (settings.c:45-72); checked against both in tests/test_reference_host.py.
bool camera_change_restarts(const LuminaryCamera& in, const LuminaryCamera& old) {
  bool d = in.pos.x != old.pos.x || in.pos.y != old.pos.y || in.pos.z != old.pos.z || in.rotation.x != old.rotation.x || in.rotation.y != old.rotation.y ||
           in.rotation.z != old.rotation.z || in.russian_roulette_threshold != old.russian_roulette_threshold || in.camera_scale != old.camera_scale ||
           in.object_distance != old.object_distance || in.use_physical_camera != old.use_physical_camera || in.aperture_shape != old.aperture_shape;
  if (in.aperture_shape != LUMINARY_APERTURE_ROUND) d = d || in.aperture_blade_count != old.aperture_blade_count;
  if (in.use_physical_camera) {
    const auto& a = in.physical; const auto& b = old.physical;
    d = d || a.allow_reflections != b.allow_reflections || a.use_spectral_rendering != b.use_spectral_rendering || a.focal_length != b.focal_length ||
        a.front_focal_point != b.front_focal_point || a.back_focal_point != b.back_focal_point || a.front_principal_point != b.front_principal_point ||
        a.back_principal_point != b.back_principal_point || a.aperture_point != b.aperture_point || a.aperture_diameter != b.aperture_diameter ||
        a.exit_pupil_point != b.exit_pupil_point || a.exit_pupil_diameter != b.exit_pupil_diameter || a.image_plane_distance != b.image_plane_distance ||
        a.sensor_width != b.sensor_width;
  }
  else d = d || in.thin_lens.fov != old.thin_lens.fov || in.thin_lens.aperture_size != old.thin_lens.aperture_size;
  return d;
}
// Any change of the lens restarts the integration of a physical camera (the lens is part of camera_check_for_dirty's physical block there).
bool lens_change_restarts(const LuminaryCameraLens& in, const LuminaryCameraLens& old) {
  if (in.num_interfaces != old.num_interfaces) return true;
  const uint32_t n = std::min<uint32_t>(in.num_interfaces, LUMINARY_CAMERA_LENS_MAX_INTERFACES);
  for (uint32_t i = 0; i < n; i++) {
    const auto &a = in.interfaces[i], &b = old.interfaces[i];
    if (a.radius != b.radius || a.vertex != b.vertex || a.cylindrical_radius != b.cylindrical_radius) return true;
  }
  for (uint32_t i = 0; i <= n; i++) {
    const auto &a = in.media[i], &b = old.media[i];
    if (a.design_ior != b.design_ior || a.abbe != b.abbe || a.cylindrical_radius != b.cylindrical_radius) return true;
  }
  return false;
}
bool settings_change_restarts(const LuminaryRendererSettings& in, const LuminaryRendererSettings& old) {
  bool d = in.width != old.width || in.height != old.height || in.supersampling != old.supersampling || in.bridge_max_num_vertices != old.bridge_max_num_vertices ||
           in.undersampling != old.undersampling || in.shading_mode != old.shading_mode || in.enable_adaptive_sampling != old.enable_adaptive_sampling ||
           in.region_x != old.region_x || in.region_y != old.region_y || in.region_width != old.region_width || in.region_height != old.region_height;
  if (in.enable_adaptive_sampling)
    d = d || in.adaptive_sampling_max_sampling_rate != old.adaptive_sampling_max_sampling_rate || in.adaptive_sampling_avg_sampling_rate != old.adaptive_sampling_avg_sampling_rate ||
        in.adaptive_sampling_update_interval != old.adaptive_sampling_update_interval || in.adaptive_sampling_exposure_aware != old.adaptive_sampling_exposure_aware;
  if (in.shading_mode == LUMINARY_SHADING_MODE_DEFAULT) d = d || in.max_ray_depth != old.max_ray_depth;
  return d;
}
template <typename T> bool change_restarts(const T&, const T&) { return true; }  // sky, ocean, cloud, fog, particles: every field feeds the integration
inline bool change_restarts(const LuminaryCamera& in, const LuminaryCamera& old) { return camera_change_restarts(in, old); }
inline bool change_restarts(const LuminaryRendererSettings& in, const LuminaryRendererSettings& old) { return settings_change_restarts(in, old); }
// An entity changed while the shutter is open: only the camera's pos and rotation are blended between the keys.
template <typename T> void shutter_note_entity(LuminaryHost* h, const char* name, const T&, const T&) { shutter_note_other(h, name); }
inline void shutter_note_entity(LuminaryHost* h, const char*, const LuminaryCamera& in, const LuminaryCamera& old) {
  LuminaryCamera c = in;
  c.pos = old.pos; c.rotation = old.rotation;
  if (camera_change_restarts(c, old)) shutter_note_other(h, "a camera field other than pos and rotation");
}

// Does this change of the camera restart the integration and keep the image history? Only a move of the thin-lens camera does: nothing differs but pos, rotation,
// thin_lens.fov, thin_lens.aperture_size and object_distance.
bool camera_change_carries(const LuminaryCamera& in, const LuminaryCamera& old) {
  if (!camera_change_restarts(in, old) || in.use_physical_camera || old.use_physical_camera) return false;
  LuminaryCamera c = in;
  c.pos = old.pos; c.rotation = old.rotation; c.thin_lens.fov = old.thin_lens.fov; c.thin_lens.aperture_size = old.thin_lens.aperture_size; c.object_distance = old.object_distance;
  return !camera_change_restarts(c, old);
}
// An entity is about to restart the integration: what the history makes of it (history_restart).
template <typename T> void history_note_entity(LuminaryHost* h, const char* name, const T&, const T&) { h->history_cause = name; }
inline void history_note_entity(LuminaryHost* h, const char*, const LuminaryCamera& in, const LuminaryCamera& old) {
  if (camera_change_carries(in, old)) h->history_camera_move = true;
  else h->history_cause = (in.use_physical_camera || old.use_physical_camera) ? "the physical camera is not reprojected" : "a camera field other than pos, rotation, fov, aperture size and object distance changed";
}
inline void history_note_entity(LuminaryHost* h, const char* name, const LuminaryRendererSettings& in, const LuminaryRendererSettings& old) {
  h->history_cause = (in.width != old.width || in.height != old.height || in.supersampling != old.supersampling) ? "the frame size changed" : name;
}

// ---- skinned and morphed meshes: the lazy host mesh ----
// HostMesh::positions / normals of a posed or morphed mesh from the host twin of the devices' kernel (in place: the pointers luminary_ext_get_mesh handed out
// stay valid): the morph once one is bound, the skin once it has a pose.
void materialise(LuminaryHost* h, uint32_t mesh) {
  const auto it = h->skins.find(mesh);
  if (it == h->skins.end() || it->second.host_current || mesh >= h->scene.meshes.size()) return;
  HostSkin& k = it->second;
  lum::HostMesh& m = h->scene.meshes[mesh];
  lum::host_parallel_for(m.triangle_count(), [&](size_t b, size_t e) {  // (a corner's bytes do not depend on the chunks)
    const bool posed = k.posed();
    lum::deform_host(k.rest_positions.data() + 9 * b, k.rest_normals.data() + 9 * b, k.has_morph() ? &k.morph_csr : nullptr, 3 * b, 3 * (e - b), k.morph_weights.data(),
                     posed ? k.bone_ids.data() + 12 * b : nullptr, posed ? k.weights.data() + 12 * b : nullptr, posed ? k.palette.data() : nullptr,
                     m.positions.data() + 9 * b, m.normals.data() + 9 * b, nullptr, nullptr);
  });
  k.host_current = true;
  h->host_materialisations++;
}
bool mesh_emits(const LuminaryHost* h, uint32_t mesh) {
  for (uint16_t id : h->scene.meshes[mesh].material_ids)
    if (id < h->scene.materials.size() && h->scene.materials[id].emission_active) return true;
  return false;
}

// The view's light arrays and the plan built again from the scene as it stands, the posed and blended emitters brought up to date first (today's path of a moved
// emitter). Nonzero on failure.
int build_view_lights(LuminaryHost* h) {
  for (auto& kv : h->skins)
    if (kv.first < h->scene.meshes.size() && mesh_emits(h, kv.first)) materialise(h, kv.first);
  const std::string err = lum::update_device_scene(h->scene, h->device_scene.bluenoise, LUMC_DIRTY_LIGHTS, &h->device_scene);
  if (!err.empty()) { h->log.push_back(err); return 1; }
  h->view_lights_stale = false;
  return 0;
}

// While the devices refit, the view's light arrays and the plan's transforms are those of the last host build. A context that is about to take the lights' part
// from the view - a new main context, a slot that was just enabled, a pending LUMC_DIRTY_LIGHTS - would get that tree over the moved vertices, so the tree is
// built first from the scene as it stands, and every context takes it: all devices sample with the same tree.
int resolve_stale_lights(LuminaryHost* h, bool partition) {  // partition: the enabled slots are about to render too
  if (!h->view_lights_stale) return 0;
  bool taken = (h->core_dirty & LUMC_DIRTY_LIGHTS) != 0;
  for (uint32_t i = 0; partition && i < h->devices.size(); i++)
    if (i != h->main_slot && h->devices[i].enabled && (!h->devices[i].core || (h->devices[i].dirty & LUMC_DIRTY_LIGHTS))) taken = true;
  if (!taken) return 0;
  if (build_view_lights(h)) return 1;
  h->core_dirty |= LUMC_DIRTY_LIGHTS; h->core_scene_valid = false;
  for (auto& slot : h->devices) { slot.dirty |= LUMC_DIRTY_LIGHTS; slot.scene_valid = false; }
  return 0;
}

// Bindings, poses and weights a context has not seen, before it takes the scene (lumc_scene_update with `dirty`); after an update that rebuilt the meshes - which
// drops the context's bindings - all of them again, and the poses and weights applied in a second, vertex-only update. *seen: the context's mark
// (LuminaryHost::skin_serial then).
int update_context_scene(LuminaryHost* h, LumContext* core, uint32_t dirty, uint64_t* seen) {
  // one mesh's share; `all`: whatever the context has seen. Returns nonzero on failure; *pending: a pose or weights were handed over.
  auto hand_over = [&](uint32_t mesh, const HostSkin& k, bool all, bool* pending) {
    const uint32_t triangles = (uint32_t) (k.rest_positions.size() / 9);
    const bool new_skin = k.has_skin() && (all || k.bind_serial > *seen), new_morph = k.has_morph() && (all || k.morph_bind_serial > *seen);
    if (new_skin && lumc_mesh_skin_bind(core, mesh, k.rest_positions.data(), k.rest_normals.data(), k.bone_ids.data(), k.weights.data(), triangles, k.bone_count)) return 1;
    if (new_morph && lumc_mesh_morph_bind(core, mesh, k.rest_positions.data(), k.rest_normals.data(), triangles, k.target_count, k.morph_offsets.data(), k.morph_corners.data(),
                                          k.morph_delta_positions.data(), k.morph_delta_normals.empty() ? nullptr : k.morph_delta_normals.data()))
      return 1;
    if (k.posed() && (new_skin || k.pose_serial > *seen)) {
      if (lumc_mesh_skin_pose(core, mesh, k.palette.data(), k.bone_count)) return 1;
      *pending = true;
    }
    if (k.weighted() && (new_morph || k.morph_weights_serial > *seen)) {
      if (lumc_mesh_morph_weights(core, mesh, k.morph_weights.data(), k.target_count)) return 1;
      *pending = true;
    }
    return 0;
  };
  const bool rebuilds_meshes = (dirty & LUMC_DIRTY_MESHES) != 0;
  const bool refits_lights = h->light_refit && (dirty & LUMC_DIRTY_LIGHT_POSITIONS) && !(dirty & LUMC_DIRTY_LIGHTS);
  // the plan of the light arrays the context just took, right after an update that took LUMC_DIRTY_LIGHTS
  auto bind_lights = [&]() {
    if (!h->light_refit) return 0;
    const LumLightRefitPlan plan = h->device_scene.light_refit_plan.view();
    return (lumc_set_light_refit(core, h->light_refit_max_cost_growth) || lumc_light_refit_bind(core, &plan)) ? 1 : 0;
  };
  if (refits_lights && (dirty & LUMC_DIRTY_INSTANCE_TRANSFORMS)) {  // 40 bytes per emitting instance
    lum::refresh_light_refit_transforms(h->scene, &h->device_scene.light_refit_plan);
    const auto& t = h->device_scene.light_refit_plan.transforms;
    if (!t.empty() && lumc_light_refit_transforms(core, t.data(), (uint32_t) t.size())) return 1;
  }
  bool pending = false;
  if (!rebuilds_meshes)
    for (const auto& kv : h->skins)
      if (hand_over(kv.first, kv.second, false, &pending)) return 1;
  if (lumc_scene_update(core, &h->device_scene.view, dirty)) return 1;
  if ((dirty & LUMC_DIRTY_LIGHTS) && bind_lights()) return 1;
  // a device that could not refit asked for a rebuild: today's path - the emitters on the host, the tree built again, the lights' part uploaded - for every
  // device, so that all sample with the same tree
  auto rebuild_lights_if_asked = [&]() {
    if (!h->light_refit || !lumc_light_refit_needs_rebuild(core)) return 0;
    if (build_view_lights(h)) return 1;
    h->light_rebuilds++;
    if (core != h->core) { h->core_dirty |= LUMC_DIRTY_LIGHTS; h->core_scene_valid = false; }
    for (auto& slot : h->devices)
      if (slot.core != core) { slot.dirty |= LUMC_DIRTY_LIGHTS; slot.scene_valid = false; }
    return (lumc_scene_update(core, &h->device_scene.view, LUMC_DIRTY_LIGHTS) || bind_lights()) ? 1 : 0;
  };
  if (refits_lights && rebuild_lights_if_asked()) return 1;
  if (rebuilds_meshes) {
    for (const auto& kv : h->skins)
      if (hand_over(kv.first, kv.second, true, &pending)) return 1;
    // (the pose moves an emitter after the tree was uploaded: with the switch on the devices refit for it as for any pose)
    if (pending && lumc_scene_update(core, &h->device_scene.view, LUMC_DIRTY_MESH_SKIN | (h->light_refit ? LUMC_DIRTY_LIGHT_POSITIONS : 0))) return 1;
    if (pending && rebuild_lights_if_asked()) return 1;
  }
  *seen = h->skin_serial;
  return 0;
}

LuminaryResult ensure_device_scene(LuminaryHost* h) {
  if (h->device_scene_valid) return LUMINARY_SUCCESS;
  // what the encoders read of a posed mesh is brought up to date first: every mesh for encode_vertices, the emitters for build_light_tree
  for (auto& kv : h->skins) {
    if (h->scene_dirty & LUMC_DIRTY_MESHES) { materialise(h, kv.first); kv.second.view_current = true; }
    else if ((h->scene_dirty & LUMC_DIRTY_LIGHTS) && kv.first < h->scene.meshes.size() && mesh_emits(h, kv.first)) materialise(h, kv.first);
  }
  if (h->hdri_origin_pending) {  // sky_hdri_update (device/device_sky.c:249-266): the panorama follows the camera only when the sky is dirty
    const LuminaryVec3 p = h->scene.camera.pos;
    h->scene.hdri_origin[0] = p.x; h->scene.hdri_origin[1] = p.y; h->scene.hdri_origin[2] = p.z;
    h->hdri_origin_pending = false;
  }
  static const std::vector<uint32_t> bluenoise = embedded_bluenoise();
  h->device_scene.moved_meshes = std::move(h->moved_meshes);
  h->moved_meshes.clear();
  const std::string err = lum::update_device_scene(h->scene, bluenoise, h->scene_dirty, &h->device_scene);
  if (!err.empty()) { h->log.push_back(err); std::fprintf(stderr, "[luminary_amd] %s\n", err.c_str()); h->scene_dirty = h->core_dirty = LUMC_DIRTY_ALL; return LUMINARY_ERROR_API_EXCEPTION; }
  // what was re-encoded is what the devices have to take over (the encoder may add a part: the texture pool when the sky mode moves the moon in or out)
  h->core_dirty |= h->device_scene.rebuilt;
  for (auto& slot : h->devices) slot.dirty |= h->device_scene.rebuilt;
  if (h->scene_dirty & LUMC_DIRTY_LIGHTS) h->view_lights_stale = false;
  else if (h->scene_dirty & LUMC_DIRTY_LIGHT_POSITIONS) h->view_lights_stale = true;  // the devices refit; the view's light arrays follow when something reads them
  h->scene_dirty = 0;
  h->device_scene_valid = true;
  h->core_scene_valid = false;
  return LUMINARY_SUCCESS;
}

// The camera a context renders with besides its scene: the converted physical camera or the scene's thin lens (lumc_set_physical_camera). Only host
// state of the context: set on every use, so no context of any device slot can miss a camera or lens change.
LuminaryResult set_camera(LuminaryHost* h, LumContext* core) {
  const lum::DeviceSceneBuffers& b = h->device_scene;
  if (lumc_set_physical_camera(core, b.use_physical_camera ? &b.physical_camera : nullptr)) {
    std::fprintf(stderr, "[luminary_amd] %s\n", lumc_last_error(core));
    return LUMINARY_ERROR_API_EXCEPTION;
  }
  return LUMINARY_SUCCESS;
}

// The main context holds the buckets of luminary_ext_set_firefly_rejection while it renders the whole accumulation alone. (The setter refuses a host with several
// enabled devices; one enabled later switches the buckets off here, and post_process then has nothing to resolve.)
int sync_firefly(LuminaryHost* h) {
  uint32_t others = 0;  // (enabled_slots, below: the main slot and every other enabled one)
  for (uint32_t i = 0; i < h->devices.size(); i++) others += (i != h->main_slot && h->devices[i].enabled) ? 1u : 0u;
  const uint32_t want = (h->firefly.enabled && others == 0) ? h->firefly.buckets : 0u;
  if (want == h->core_firefly) return 0;
  if (lumc_set_firefly_buckets(h->core, want)) { std::fprintf(stderr, "[luminary_amd] %s\n", lumc_last_error(h->core)); return 1; }
  h->core_firefly = want;
  return 0;
}

LuminaryResult ensure_core(LuminaryHost* h) {
  if (!h->core) {
    if (lumc_context_create(h->device_ordinal, &h->core)) {
      std::fprintf(stderr, "[luminary_amd] no usable HIP device: %s\n", lumc_last_error(h->core));
      lumc_context_destroy(h->core);
      h->core = nullptr;
      return LUMINARY_ERROR_CUDA;
    }
  }
  const LuminaryResult r = ensure_device_scene(h);
  if (r) return r;
  if (resolve_stale_lights(h, false)) return LUMINARY_ERROR_API_EXCEPTION;
  if (!h->core_scene_valid) {
    lumc_set_mesh_refit(h->core, h->refit_mode, h->refit_max_cost_growth);
    lumc_set_instance_update(h->core, h->instance_update_mode);
    lumc_set_mesh_refit_in_place(h->core, h->refit_in_place);
    lumc_set_light_refit(h->core, h->light_refit_max_cost_growth);
    if (sync_firefly(h)) return LUMINARY_ERROR_CUDA;
    if (update_context_scene(h, h->core, h->core_dirty, &h->core_skin_seen)) { std::fprintf(stderr, "[luminary_amd] %s\n", lumc_last_error(h->core)); h->core_dirty = LUMC_DIRTY_ALL; return LUMINARY_ERROR_CUDA; }
    h->core_dirty = 0;
    h->core_scene_valid = true;
    // The accumulation starts over. With the frame size unchanged the pixel sets of the devices stay as they are and only their accumulators
    // are cleared; a new size makes the render loop set them up again (num_pixels = 0).
    const LumDeviceSceneView& v = h->device_scene.view;
    const bool same_frame = h->num_pixels != 0 && h->core_width == v.width && h->core_height == v.height;
    h->core_width = v.width; h->core_height = v.height;
    if (!same_frame || h->partition_n > 1 || lumc_clear_accumulators(h->core)) h->num_pixels = 0;
  }
  return set_camera(h, h->core);
}

// The enabled devices, main device first. Rendering is tiled over them when the whole frame is rendered uniformly; adaptive sampling, render
// regions / pixel subsets and the undersampling preview run on the main device alone.
std::vector<LuminaryHost::DeviceSlot*> enabled_slots(LuminaryHost* h) {
  std::vector<LuminaryHost::DeviceSlot*> out;
  if (h->main_slot < h->devices.size()) out.push_back(&h->devices[h->main_slot]);
  for (uint32_t i = 0; i < h->devices.size(); i++)
    if (i != h->main_slot && h->devices[i].enabled) out.push_back(&h->devices[i]);
  return out;
}

// Contexts with the current scene on every device of the partition; slot 0 of the result is the main device (h->core).
LuminaryResult ensure_partition_cores(LuminaryHost* h, std::vector<LumContext*>* cores) {
  if (const LuminaryResult rs = ensure_device_scene(h)) return rs;
  if (resolve_stale_lights(h, true)) return LUMINARY_ERROR_API_EXCEPTION;  // (before the main context takes its update: every slot gets the same tree)
  const LuminaryResult r = ensure_core(h);
  if (r) return r;
  cores->clear();
  for (LuminaryHost::DeviceSlot* slot : enabled_slots(h)) {
    if (slot == &h->devices[h->main_slot]) { slot->core = h->core; slot->scene_valid = true; slot->dirty = 0; cores->push_back(h->core); continue; }
    if (!slot->core) {
      if (lumc_context_create(slot->ordinal, &slot->core)) {
        std::fprintf(stderr, "[luminary_amd] device %d: %s\n", slot->ordinal, lumc_last_error(slot->core));
        lumc_context_destroy(slot->core);
        slot->core = nullptr;
        return LUMINARY_ERROR_CUDA;
      }
      lumc_set_flavour(slot->core, lumc_get_flavour(h->core));
      slot->scene_valid = false;
    }
    if (!slot->scene_valid) {
      lumc_set_mesh_refit(slot->core, h->refit_mode, h->refit_max_cost_growth);
      lumc_set_instance_update(slot->core, h->instance_update_mode);
      lumc_set_mesh_refit_in_place(slot->core, h->refit_in_place);
      lumc_set_light_refit(slot->core, h->light_refit_max_cost_growth);
      if (update_context_scene(h, slot->core, slot->dirty, &slot->skin_seen)) { std::fprintf(stderr, "[luminary_amd] device %d: %s\n", slot->ordinal, lumc_last_error(slot->core)); slot->dirty = LUMC_DIRTY_ALL; return LUMINARY_ERROR_CUDA; }
      slot->dirty = 0;
      slot->scene_valid = true;
      h->partition_n = 0;  // the accumulation restarts: the render loop deals the tiles again (which also clears every device's accumulators)
    }
    if (const LuminaryResult rc = set_camera(h, slot->core)) return rc;
    cores->push_back(slot->core);
  }
  return LUMINARY_SUCCESS;
}

}  // namespace

extern "C" {

// ---- error.c ---- (the reference's texts, checked against its own error.c in tests/test_reference_host.py; codes 8 and 9 keep their
// wording for frontends that print or match them, although the errors come from HIP and the BVH builders here)
const char* luminary_result_to_string(LuminaryResult result) {
  switch (result & ~LUMINARY_ERROR_PROPAGATED) {
    case LUMINARY_SUCCESS: return "Success";
    case LUMINARY_ERROR_ARGUMENT_NULL: return "Encountered NULL argument";
    case LUMINARY_ERROR_NOT_IMPLEMENTED: return "Encountered a section that is not implemented";
    case LUMINARY_ERROR_INVALID_API_ARGUMENT: return "Encountered an invalid argument";
    case LUMINARY_ERROR_MEMORY_LEAK: return "Identified a memory leak";
    case LUMINARY_ERROR_OUT_OF_MEMORY: return "Ran out of memory";
    case LUMINARY_ERROR_C_STD: return "Encountered an error in a call to a C stdlib function";
    case LUMINARY_ERROR_API_EXCEPTION: return "Encountered an internal error";
    case LUMINARY_ERROR_CUDA: return "Encountered an error reported by CUDA";
    case LUMINARY_ERROR_OPTIX: return "Encountered an error reported by OptiX";
    case LUMINARY_ERROR_PREVIOUS_ERROR: return "Encountered an unstable state due to a previous error";
    case LUMINARY_ERROR_DEBUG_ASSERT: return "Encountered an invalid state during debugging";
    case LUMINARY_ERROR_MISSING_DATA: return "Missing necessary embedded data";
    case LUMINARY_ERROR_INVALID_DEVICE: return "Specified invalid device";
    default: return "Unknown";
  }
}

// ---- luminary.c:7-31 ----
void luminary_init(void) {}
void luminary_shutdown(void) {}

// ---- path.c ----
LuminaryResult luminary_path_create(LuminaryPath** path) { CHECK_NULL(path); *path = new LuminaryPath(); return LUMINARY_SUCCESS; }
LuminaryResult luminary_path_set_from_string(LuminaryPath* path, const char* string) { CHECK_NULL(path); CHECK_NULL(string); path->value = string; return LUMINARY_SUCCESS; }
LuminaryResult luminary_path_destroy(LuminaryPath** path) { CHECK_NULL(path); CHECK_NULL(*path); delete *path; *path = nullptr; return LUMINARY_SUCCESS; }

// ---- host.c:292-404 ----
LuminaryResult luminary_host_create(LuminaryHost** host, LuminaryHostCreateInfo info) {
  CHECK_NULL(host);
  LuminaryHost* h = new LuminaryHost();
  // one process per GPU: the lowest set bit of the mask selects the ordinal (torch.distributed sets LOCAL_RANK for the launcher)
  int ordinal = 0;
  if (info.device_mask != 0) while (!((info.device_mask >> ordinal) & 1u) && ordinal < 31) ordinal++;
  if (const char* lr = std::getenv("LOCAL_RANK")) { if (info.device_mask == LUMINARY_HOST_CREATE_INFO_DEVICE_MASK_ALL_DEVICES) ordinal = std::atoi(lr); }
  h->device_ordinal = ordinal;
  // One slot per visible device; the mask enables them (device_manager.c:791-822), the lowest enabled one is the main device. Under a
  // one-process-per-GPU launcher (LOCAL_RANK set, default mask) the process drives its own GPU only. LUM_MAX_DEVICES caps the number of
  // devices a host uses; LUM_FAKE_DEVICES=n (tests on a single-GPU box) presents device 0 n times.
  {
    int count = lumc_device_count();
    const char* fake = std::getenv("LUM_FAKE_DEVICES");
    const int fake_n = fake ? std::atoi(fake) : 0;
    if (fake_n > 1 && count >= 1) count = fake_n;
    int cap = 32;
    if (const char* e = std::getenv("LUM_MAX_DEVICES")) cap = std::max(1, std::atoi(e));
    const bool own_gpu_only = std::getenv("LOCAL_RANK") && info.device_mask == LUMINARY_HOST_CREATE_INFO_DEVICE_MASK_ALL_DEVICES;
    int enabled = 0;
    for (int i = 0; i < count && i < 32; i++) {
      LuminaryHost::DeviceSlot slot;
      slot.ordinal = fake_n > 1 ? 0 : i;
      slot.enabled = own_gpu_only ? (i == ordinal) : (((info.device_mask >> i) & 1u) != 0 && enabled < cap);
      if (slot.enabled) enabled++;
      h->devices.push_back(slot);
    }
    if (h->devices.empty()) { LuminaryHost::DeviceSlot slot; slot.ordinal = ordinal; slot.enabled = true; h->devices.push_back(slot); }  // no GPU visible: calls that need one fail later
    h->main_slot = 0;
    bool found = false;
    for (uint32_t i = 0; i < h->devices.size() && !found; i++) if (h->devices[i].enabled) { h->main_slot = i; found = true; }
    if (!found) { h->devices[0].enabled = true; h->main_slot = 0; }
    h->device_ordinal = h->devices[h->main_slot].ordinal;
  }
  // the reference names its queue workers "Host", "Device" and "Worker n" (host.c:318-330, device_manager.c:874)
  if (thread_status_create(&h->status_host) || thread_status_create(&h->status_device)) { delete h; return LUMINARY_ERROR_OUT_OF_MEMORY; }
  thread_status_set_worker_name(h->status_host, "Host");
  thread_status_set_worker_name(h->status_device, "Device");
  *host = h;
  return LUMINARY_SUCCESS;
}

namespace {
LuminaryResult render_locked(LuminaryHost* host, uint32_t num_samples, uint32_t samples_per_pass);
uint32_t pass_size(LuminaryHost* h);
void stop_worker(LuminaryHost* h, bool join) {
  {
    std::lock_guard<std::mutex> l(h->worker_mutex);
    h->async_active = false;
    if (join) h->worker_stop = true;
  }
  h->worker_cv.notify_all();
  if (join && h->worker_started) { h->worker.join(); h->worker_started = false; }
  else { ApiLock wait_for_the_running_iteration(h); }
}

// The "Device" worker: one iteration = the next sample allocations of the running accumulation (luminary_ext_render, which also rebuilds
// the scene after an edit and produces the outputs that are due). Small chunks first, so that the first images of a new accumulation
// appear quickly, then whole wavefront passes of pass_size() sample ids.
void worker_main(LuminaryHost* h) {
  for (;;) {
    {
      std::unique_lock<std::mutex> l(h->worker_mutex);
      h->worker_cv.wait(l, [&] { return h->worker_stop || (h->async_active && !h->async_failed); });
      if (h->worker_stop) break;
    }
    while (h->api_waiting.load() > 0) std::this_thread::yield();  // edits first
    LuminaryResult r = LUMINARY_SUCCESS;
    bool idle = false;
    {
      // One lock from the decision to the last kernel of the iteration: the flag is looked at again under the host's mutex (a stop that set it
      // and then took and released this mutex has been seen by now, so nothing renders after luminary_ext_stop_render returned), and the
      // first sample id is computed under the same lock the passes run under (no start / edit / synchronous render can slip in between).
      ApiLock lock(h);
      bool active;
      { std::lock_guard<std::mutex> l(h->worker_mutex); active = h->async_active && !h->async_failed && !h->worker_stop; }
      if (!active) continue;
      const uint32_t accumulated = h->accumulated_samples;
      if (accumulated >= (1u << 20)) idle = true;  // every sample id is used up (MAX_NUM_GLOBAL_SAMPLES, device_utils.h:39): idle until the next edit
      else {
        thread_status_start(h->status_device, h->core_scene_valid ? "Rendering" : "Updating scene");
        // small allocations first so that the first images of a new accumulation appear quickly, then whole passes (pass_size)
        const uint32_t cap = pass_size(h);
        const uint32_t chunk = accumulated < 1u ? 1u : (accumulated < cap ? accumulated : cap);
        r = render_locked(h, chunk, cap);
      }
    }
    if (idle) {
      std::unique_lock<std::mutex> l(h->worker_mutex);
      h->worker_cv.wait_for(l, std::chrono::milliseconds(50));
      continue;
    }
    thread_status_stop(h->status_device);
    if (r != LUMINARY_SUCCESS) {
      std::fprintf(stderr, "[luminary_amd] render worker: %s; waiting for the next scene edit or luminary_host_start_new_render\n", luminary_result_to_string(r));
      std::lock_guard<std::mutex> l(h->worker_mutex);
      h->async_failed = true;
    }
  }
}
}  // namespace

LuminaryResult luminary_host_destroy(LuminaryHost** host) {
  CHECK_NULL(host); CHECK_NULL(*host);
  stop_worker(*host, true);
  for (uint32_t i = 0; i < (*host)->devices.size(); i++)
    if (i != (*host)->main_slot && (*host)->devices[i].core) lumc_context_destroy((*host)->devices[i].core);
  if ((*host)->core) lumc_context_destroy((*host)->core);
  thread_status_destroy(&(*host)->status_host);
  thread_status_destroy(&(*host)->status_device);
  delete *host;
  *host = nullptr;
  return LUMINARY_SUCCESS;
}

// host.c:406-414: marks the integration dirty, i.e. the accumulation restarts; the reference's Device thread then renders until the host
// is destroyed. Here this call is what starts the "Device" worker (both modes of Mandarin Duck call it before polling for outputs,
// mandarin_duck.c:153, :200).
LuminaryResult luminary_host_start_new_render(LuminaryHost* host) {
  CHECK_NULL(host);
  {
    ApiLock lock(host);
    history_drop(host, "luminary_host_start_new_render");
    host->accumulated_samples = 0;
    host->guides_valid = false;
    host->render_seconds = 0.0;
    host->adaptive_active = false;
    if (host->core && host->num_pixels) lumc_clear_accumulators(host->core);
  }
  {
    std::lock_guard<std::mutex> l(host->worker_mutex);
    host->async_active = true;
    host->async_failed = false;
    if (!host->worker_started) { host->worker_stop = false; host->worker = std::thread(worker_main, host); host->worker_started = true; }
  }
  host->worker_cv.notify_all();
  return LUMINARY_SUCCESS;
}
// Additive: stops the asynchronous rendering started by luminary_host_start_new_render (returns once the running iteration has ended); the
// accumulated frame stays. The luminary_ext_render* calls drive the same loop synchronously afterwards.
LuminaryResult luminary_ext_stop_render(LuminaryHost* host) {
  CHECK_NULL(host);
  stop_worker(host, false);
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_is_rendering(LuminaryHost* host, bool* rendering, uint32_t* accumulated_samples) {
  CHECK_NULL(host);
  { std::lock_guard<std::mutex> l(host->worker_mutex); if (rendering) *rendering = host->async_active && !host->async_failed; }
  if (accumulated_samples) { ApiLock lock(host); *accumulated_samples = host->accumulated_samples; }
  return LUMINARY_SUCCESS;
}

// host.c:416-470, device_manager.c:529-572: the visible devices, which of them render, and the main device (renders its tiles and produces
// every output; re-elected as the lowest enabled device when it is disabled)
LuminaryResult luminary_host_get_device_count(LuminaryHost* host, uint32_t* device_count) {
  CHECK_NULL(host); CHECK_NULL(device_count);
  *device_count = (uint32_t) host->devices.size();
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_host_get_device_info(LuminaryHost* host, uint32_t device_id, LuminaryDeviceInfo* info) {
  CHECK_NULL(host); CHECK_NULL(info);
  if (device_id >= host->devices.size()) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  ApiLock lock(host);
  std::memset(info, 0, sizeof(*info));
  info->is_main_device = device_id == host->main_slot; info->is_enabled = host->devices[device_id].enabled; info->is_unavailable = false;
  char name[200];
  if (lumc_device_name(host->devices[device_id].ordinal, name, sizeof(name))) { std::snprintf(name, sizeof(name), "HIP device %d", host->devices[device_id].ordinal); info->is_unavailable = true; }
  std::snprintf(info->name, sizeof(info->name), "%s", name);
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_host_set_device_enable(LuminaryHost* host, uint32_t device_id, bool enable) {
  CHECK_NULL(host);
  if (device_id >= host->devices.size()) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  ApiLock lock(host);
  if (host->devices[device_id].enabled == enable) return LUMINARY_SUCCESS;
  if (!enable) {
    uint32_t others = 0;
    for (uint32_t i = 0; i < host->devices.size(); i++) if (i != device_id && host->devices[i].enabled) others++;
    if (others == 0) return LUMINARY_ERROR_INVALID_API_ARGUMENT;  // "No device could be selected as the main device" (device_manager.c:44-46)
  }
  host->devices[device_id].enabled = enable;
  if (!enable && device_id == host->main_slot) {  // the main device changes: its context (accumulators, outputs in flight) goes with it
    if (host->core) { lumc_context_destroy(host->core); host->core = nullptr; }
    host->devices[device_id].core = nullptr;
    for (uint32_t i = 0; i < host->devices.size(); i++) if (host->devices[i].enabled) { host->main_slot = i; break; }
    LuminaryHost::DeviceSlot& m = host->devices[host->main_slot];
    host->device_ordinal = m.ordinal;
    if (m.core) { host->core = m.core; }  // its render context becomes the main context
    host->core_scene_valid = false;
    host->core_dirty = LUMC_DIRTY_ALL;  // the new main context takes the whole scene again
    host->num_pixels = 0;
  }
  host->partition_n = 0;
  host->comm_ready = false;
  invalidate(host, 0);  // the integration restarts with the new partition; the scene itself did not change
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_host_start_device(LuminaryHost* host, uint32_t index) { return luminary_host_set_device_enable(host, index, true); }
LuminaryResult luminary_host_shutdown_device(LuminaryHost* host, uint32_t index) { return luminary_host_set_device_enable(host, index, false); }

// host.c:35-100 (+ :472-532)
LuminaryResult luminary_host_load_obj_file(LuminaryHost* host, LuminaryPath* path) {
  CHECK_NULL(host); CHECK_NULL(path);
  ApiLock lock(host);
  lum::HostMesh mesh;
  std::vector<LuminaryMaterial> mats;
  std::vector<std::string> warnings;
  std::string err;
  std::vector<lum::HostTexture> textures;
  if (!lum::load_obj(path->value, lum::ObjLoadArgs(), (uint32_t) host->scene.materials.size(), &mesh, &mats, &warnings, &err, &textures, (uint32_t) host->scene.textures.size())) {
    std::fprintf(stderr, "[luminary_amd] %s\n", err.c_str());
    return LUMINARY_ERROR_API_EXCEPTION;
  }
  for (auto& w : warnings) std::fprintf(stderr, "[luminary_amd] warning: %s\n", w.c_str());
  if (mesh.triangle_count() == 0 && mesh.name.empty()) return LUMINARY_SUCCESS;
  host->scene.materials.insert(host->scene.materials.end(), mats.begin(), mats.end());
  for (auto& t : textures) host->scene.textures.push_back(std::move(t));
  host->scene.meshes.push_back(std::move(mesh));
  invalidate(host, LUMC_DIRTY_MESHES | LUMC_DIRTY_INSTANCES | LUMC_DIRTY_MATERIALS | LUMC_DIRTY_TEXTURES | LUMC_DIRTY_LIGHTS);
  return LUMINARY_SUCCESS;
}

// host.c:534-605
LuminaryResult luminary_host_load_lum_file(LuminaryHost* host, LuminaryPath* path) {
  CHECK_NULL(host); CHECK_NULL(path);
  ApiLock lock(host);
  lum::LumFileContent content;
  lum::default_settings(&content.settings); lum::default_camera(&content.camera); lum::default_ocean(&content.ocean); lum::default_sky(&content.sky);
  lum::default_cloud(&content.cloud); lum::default_fog(&content.fog); lum::default_particles(&content.particles);
  std::vector<std::string> warnings;
  std::string err;
  if (!lum::load_lum_v4(path->value, &content, &warnings, &err)) { std::fprintf(stderr, "[luminary_amd] %s\n", err.c_str()); return LUMINARY_ERROR_API_EXCEPTION; }
  // every mesh file is read before anything is committed: a file that fails to load leaves the host's scene exactly as it was
  std::vector<lum::HostMesh> new_meshes;
  std::vector<LuminaryMaterial> new_materials;
  std::vector<lum::HostTexture> new_textures;
  for (const std::string& obj : content.obj_files) {
    lum::HostMesh mesh;
    std::vector<LuminaryMaterial> mats;
    std::vector<lum::HostTexture> textures;
    if (!lum::load_obj(lum::extend_path(path->value, obj), content.obj_args, (uint32_t) (host->scene.materials.size() + new_materials.size()), &mesh, &mats, &warnings, &err, &textures,
                       (uint32_t) (host->scene.textures.size() + new_textures.size()))) {
      std::fprintf(stderr, "[luminary_amd] %s\n", err.c_str());
      return LUMINARY_ERROR_API_EXCEPTION;
    }
    new_materials.insert(new_materials.end(), mats.begin(), mats.end());
    for (auto& t : textures) new_textures.push_back(std::move(t));
    new_meshes.push_back(std::move(mesh));
  }
  host->scene.materials.insert(host->scene.materials.end(), new_materials.begin(), new_materials.end());
  for (auto& t : new_textures) host->scene.textures.push_back(std::move(t));
  for (auto& m : new_meshes) {
    const uint32_t mesh_id = (uint32_t) host->scene.meshes.size();
    host->scene.meshes.push_back(std::move(m));
    lum::HostInstance inst;
    inst.mesh_id = mesh_id;
    host->scene.instances.push_back(inst);
  }
  for (auto& w : warnings) std::fprintf(stderr, "[luminary_amd] warning: %s\n", w.c_str());
  host->scene.settings = content.settings; host->scene.camera = content.camera; host->scene.ocean = content.ocean; host->scene.sky = content.sky;
  host->scene.cloud = content.cloud; host->scene.fog = content.fog; host->scene.particles = content.particles;
  host->hdri_origin_pending = true;
  invalidate(host);
  return LUMINARY_SUCCESS;
}

// host.c:607-613 -> sample_time_get_time (device_sampletime.c:32-45): with one device, the time its latest sample took (milliseconds; 0 before the first)
LuminaryResult luminary_host_get_current_sample_time(LuminaryHost* host, double* time) { CHECK_NULL(host); CHECK_NULL(time); *time = host->last_sample_ms; return LUMINARY_SUCCESS; }
// host.c:615-703. Two queue workers exist here: 0 "Host" (scene edits are applied on the caller's thread, so it never reports a task) and
// 1 "Device", the render worker, with what it is doing and for how long (thread_status.h). The reference adds 16 "Worker n" threads that
// load mesh files in parallel (host.c:15-20); files are loaded on the caller's thread here.
LuminaryResult luminary_host_get_num_queue_workers(const LuminaryHost* host, uint32_t* n) { CHECK_NULL(host); CHECK_NULL(n); *n = 2; return LUMINARY_SUCCESS; }
static LuminaryThreadStatus* queue_worker_status(const LuminaryHost* host, uint32_t id) { return id == 0 ? host->status_host : id == 1 ? host->status_device : nullptr; }
LuminaryResult luminary_host_get_queue_worker_name(const LuminaryHost* host, uint32_t id, const char** string) {
  CHECK_NULL(host); CHECK_NULL(string);
  LuminaryThreadStatus* st = queue_worker_status(host, id);
  if (!st) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  return thread_status_get_worker_name(st, string);
}
LuminaryResult luminary_host_get_queue_worker_string(const LuminaryHost* host, uint32_t id, const char** string) {
  CHECK_NULL(host); CHECK_NULL(string);
  LuminaryThreadStatus* st = queue_worker_status(host, id);
  if (!st) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  return thread_status_get_string(st, string);
}
LuminaryResult luminary_host_get_queue_worker_time(const LuminaryHost* host, uint32_t id, double* time) {
  CHECK_NULL(host); CHECK_NULL(time);
  LuminaryThreadStatus* st = queue_worker_status(host, id);
  if (!st) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  return thread_status_get_time(st, time);
}

// ---- output chain (host.c:930-1075, host_output_handler.c, device_output.c:178-343) ----
// Rendering is synchronous here (luminary_ext_render_samples), so outputs are produced on the caller's thread right after the pass
// that reaches the sample count they are due at; the handle/promise semantics are the reference's.
LuminaryResult luminary_host_set_output_properties(LuminaryHost* host, LuminaryOutputProperties p) { CHECK_NULL(host); host->outputs.set_properties(p); return LUMINARY_SUCCESS; }
LuminaryResult luminary_host_request_output(LuminaryHost* host, LuminaryOutputRequestProperties p, LuminaryOutputPromiseHandle* handle) {
  CHECK_NULL(host); CHECK_NULL(handle);
  if (p.width < 2 || p.height < 2) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  *handle = host->outputs.add_request(p);
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_host_try_await_output(LuminaryHost* host, LuminaryOutputPromiseHandle handle, LuminaryOutputHandle* out) {
  CHECK_NULL(host); CHECK_NULL(out);
  return host->outputs.acquire_from_promise(handle, out);
}
LuminaryResult luminary_host_acquire_output(LuminaryHost* host, LuminaryOutputHandle* out) { CHECK_NULL(host); CHECK_NULL(out); return host->outputs.acquire_recurring(out); }
LuminaryResult luminary_host_get_image(LuminaryHost* host, LuminaryOutputHandle handle, LuminaryImage* image) { CHECK_NULL(host); CHECK_NULL(image); return host->outputs.get_image(handle, image); }
LuminaryResult luminary_host_release_output(LuminaryHost* host, LuminaryOutputHandle handle) { CHECK_NULL(host); return host->outputs.release(handle); }
// host.c:997-1014. The reference reads a G-buffer that its trace kernel fills during undersampled previews (optix_kernel_raytrace.cu:18-76);
// here the pixel's first-sample camera ray is traced on demand, which gives the same fields at any time.
LuminaryResult luminary_host_get_pixel_info(LuminaryHost* host, uint16_t x, uint16_t y, LuminaryPixelQueryResult* result) {
  CHECK_NULL(host); CHECK_NULL(result);
  ApiLock lock(host);
  std::memset(result, 0, sizeof(*result));
  result->instance_id = 0xFFFFFFFFu; result->material_id = 0xFFFF; result->depth = -1.0f;  // DEPTH_INVALID / MATERIAL_ID_INVALID, utils.h:30-33
  if (ensure_core(host)) return LUMINARY_SUCCESS;  // no device: the query has no data, like a G-buffer that is not ready
  const LumDeviceSceneView& v = host->device_scene.view;
  if (x >= v.width || y >= v.height) return LUMINARY_SUCCESS;
  uint32_t q[6];
  if (lumc_pixel_query(host->core, x, y, 0, q)) return LUMINARY_ERROR_CUDA;
  if (q[0] == 0xFFFFFFFFu) return LUMINARY_SUCCESS;  // the physical camera's ray did not leave the lens: it has no task, like a pixel without a G-buffer entry
  float depth, dir[3];
  std::memcpy(&depth, &q[2], 4); std::memcpy(dir, &q[3], 12);
  result->depth = depth;
  if (q[0] < 0x7FFFFFFFu && q[0] < v.num_instances) {  // HIT_TYPE_TRIANGLE_ID_LIMIT
    const uint32_t mesh = v.instance_mesh_ids[q[0]];
    result->instance_id = q[0];
    result->material_id = (uint16_t) (v.tri_tex[(size_t) (v.mesh_tri_offset[mesh] + q[1]) * 4 + 3] & 0xFFFFu);
  }
  if (depth < FLT_MAX) {  // rel_hit_pos = ray * depth, kept at bfloat16 precision like the G-buffer
    float rel[3] = {dir[0] * depth, dir[1] * depth, dir[2] * depth};
    for (int k = 0; k < 3; k++) { uint32_t b; std::memcpy(&b, &rel[k], 4); b &= 0xFFFF0000u; std::memcpy(&rel[k], &b, 4); }
    result->rel_hit_pos.x = rel[0]; result->rel_hit_pos.y = rel[1]; result->rel_hit_pos.z = rel[2];
  }
  result->pixel_query_is_valid = (result->depth != -1.0f) || (result->instance_id != 0xFFFFFFFFu) || (result->material_id != 0xFFFF);
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_host_save_png(LuminaryHost* host, LuminaryOutputHandle handle, LuminaryPath* path) {
  CHECK_NULL(host); CHECK_NULL(path);
  if (handle == LUMINARY_OUTPUT_HANDLE_INVALID) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  LuminaryResult r = host->outputs.acquire(handle);
  if (r) return r;
  LuminaryImage image;
  r = host->outputs.get_image(handle, &image);
  if (!r) r = lum::write_png(path->value.c_str(), reinterpret_cast<const uint32_t*>(image.buffer), image.width, image.height, image.ld);
  host->outputs.release(handle);
  return r;
}
LuminaryResult luminary_ext_add_texture(LuminaryHost* host, const uint8_t* rgba8, uint32_t width, uint32_t height, float gamma, uint16_t* texture_id) {
  CHECK_NULL(host); CHECK_NULL(rgba8); CHECK_NULL(texture_id);
  if (width == 0 || height == 0 || host->scene.textures.size() >= 0xFFFF) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  ApiLock lock(host);
  lum::HostTexture t;
  t.width = width; t.height = height; t.gamma = gamma;
  t.texels.resize((size_t) width * height);
  std::memcpy(t.texels.data(), rgba8, t.texels.size() * 4);
  host->scene.textures.push_back(std::move(t));
  *texture_id = (uint16_t) (host->scene.textures.size() - 1);
  invalidate(host, LUMC_DIRTY_TEXTURES | LUMC_DIRTY_LIGHTS);  // emissive textures weigh the light tree
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_write_png(const char* path, const uint32_t* argb8, uint32_t width, uint32_t height, size_t ld) { return lum::write_png(path, argb8, width, height, ld); }
// host.c:1077-1084 -> scene_set_hdri_dirty (scene.c:712-722): the panorama is baked again, seen from the camera's current position
LuminaryResult luminary_host_request_sky_hdri_build(LuminaryHost* host) {
  CHECK_NULL(host);
  ApiLock lock(host);
  host->hdri_origin_pending = true;
  shutter_note_other(host, "the sky panorama");
  invalidate(host, LUMC_DIRTY_CONSTANTS);
  return LUMINARY_SUCCESS;
}

// ---- entity getters / setters (host.c:705-900) ----
#define ENTITY_ACCESSORS(NAME, TYPE, FIELD)                                                             \
  LuminaryResult luminary_host_get_##NAME(LuminaryHost* host, TYPE* out) {                              \
    CHECK_NULL(host); CHECK_NULL(out);                                                                  \
    ApiLock lock(host);                                                      \
    *out = host->scene.FIELD;                                                                           \
    return LUMINARY_SUCCESS;                                                                            \
  }                                                                                                     \
  LuminaryResult luminary_host_set_##NAME(LuminaryHost* host, const TYPE* in) {                         \
    CHECK_NULL(host); CHECK_NULL(in);                                                                   \
    ApiLock lock(host);                                                      \
    if (std::memcmp(&host->scene.FIELD, in, sizeof(TYPE)) != 0) {                                       \
      const bool restarts = change_restarts(*in, host->scene.FIELD);                                    \
      if (restarts) shutter_note_entity(host, "the " #NAME, *in, host->scene.FIELD);                     \
      if (restarts) history_note_entity(host, "the " #NAME " changed", *in, host->scene.FIELD);          \
      host->scene.FIELD = *in;                                                                          \
      if (std::is_same<TYPE, LuminarySky>::value) host->hdri_origin_pending = true; /* sky.c:45: every sky change dirties the panorama */ \
      /* these entities reach the kernels as constants (and tables derived from them): no mesh, instance or material array is touched */ \
      if (restarts) invalidate(host, LUMC_DIRTY_CONSTANTS | (std::is_same<TYPE, LuminaryParticles>::value ? LUMC_DIRTY_PARTICLES : 0u)); \
      /* else: only the outputs change; the accumulated frame stays (SCENE_DIRTY_FLAG_OUTPUT) */ \
    }                                                                                                   \
    return LUMINARY_SUCCESS;                                                                            \
  }
ENTITY_ACCESSORS(settings, LuminaryRendererSettings, settings)
ENTITY_ACCESSORS(camera, LuminaryCamera, camera)
ENTITY_ACCESSORS(ocean, LuminaryOcean, ocean)
ENTITY_ACCESSORS(sky, LuminarySky, sky)
ENTITY_ACCESSORS(cloud, LuminaryCloud, cloud)
ENTITY_ACCESSORS(fog, LuminaryFog, fog)
ENTITY_ACCESSORS(particles, LuminaryParticles, particles)

LuminaryResult luminary_host_get_material(LuminaryHost* host, uint16_t id, LuminaryMaterial* material) {
  CHECK_NULL(host); CHECK_NULL(material);
  ApiLock lock(host);
  if (id >= host->scene.materials.size()) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  *material = host->scene.materials[id];
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_host_set_material(LuminaryHost* host, uint16_t id, const LuminaryMaterial* material) {
  CHECK_NULL(host); CHECK_NULL(material);
  ApiLock lock(host);
  if (id >= host->scene.materials.size()) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  host->scene.materials[id] = *material;
  host->scene.materials[id].id = id;
  invalidate(host, LUMC_DIRTY_MATERIALS | LUMC_DIRTY_LIGHTS);  // geometry and acceleration structures stay; emission feeds the light tree
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_host_get_instance(LuminaryHost* host, uint32_t id, LuminaryInstance* instance) {
  CHECK_NULL(host); CHECK_NULL(instance);
  ApiLock lock(host);
  if (id >= host->scene.instances.size()) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  const lum::HostInstance& i = host->scene.instances[id];
  instance->id = id; instance->mesh_id = i.mesh_id; instance->position = i.translation; instance->rotation = i.rotation; instance->scale = i.scale;
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_host_set_instance(LuminaryHost* host, const LuminaryInstance* instance) {
  CHECK_NULL(host); CHECK_NULL(instance);
  ApiLock lock(host);
  if (instance->id >= host->scene.instances.size()) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  lum::HostInstance& i = host->scene.instances[instance->id];
  i.mesh_id = instance->mesh_id; i.translation = instance->position; i.rotation = instance->rotation; i.scale = instance->scale; i.active = true;
  invalidate(host, LUMC_DIRTY_INSTANCES | LUMC_DIRTY_LIGHTS);  // top-level tree and light tree; the per-mesh trees are reused
  return LUMINARY_SUCCESS;
}
// host.c:902-930: writes defaults and the new id back to the caller
LuminaryResult luminary_host_new_instance(LuminaryHost* host, LuminaryInstance* instance) {
  CHECK_NULL(host); CHECK_NULL(instance);
  ApiLock lock(host);
  lum::HostInstance i;
  i.mesh_id = 0;
  host->scene.instances.push_back(i);
  instance->id = (uint32_t) host->scene.instances.size() - 1; instance->mesh_id = i.mesh_id;
  instance->position = i.translation; instance->rotation = i.rotation; instance->scale = i.scale;
  invalidate(host, LUMC_DIRTY_INSTANCES | LUMC_DIRTY_LIGHTS);
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_host_get_num_meshes(LuminaryHost* host, uint32_t* n) { CHECK_NULL(host); CHECK_NULL(n); *n = (uint32_t) host->scene.meshes.size(); return LUMINARY_SUCCESS; }
LuminaryResult luminary_host_get_num_materials(LuminaryHost* host, uint32_t* n) { CHECK_NULL(host); CHECK_NULL(n); *n = (uint32_t) host->scene.materials.size(); return LUMINARY_SUCCESS; }
LuminaryResult luminary_host_get_num_instances(LuminaryHost* host, uint32_t* n) { CHECK_NULL(host); CHECK_NULL(n); *n = (uint32_t) host->scene.instances.size(); return LUMINARY_SUCCESS; }

// ---- additive extension ----
LuminaryResult luminary_ext_add_mesh(LuminaryHost* host, const float* positions, const float* normals, const float* uvs, const uint16_t* material_ids,
                                     uint32_t triangle_count, uint32_t* mesh_id) {
  CHECK_NULL(host); CHECK_NULL(positions); CHECK_NULL(material_ids);
  ApiLock lock(host);
  lum::HostMesh m;
  m.positions.assign(positions, positions + 9 * (size_t) triangle_count);
  m.material_ids.assign(material_ids, material_ids + triangle_count);
  if (uvs) m.uvs.assign(uvs, uvs + 6 * (size_t) triangle_count); else m.uvs.assign(6 * (size_t) triangle_count, 0.0f);
  if (normals) m.normals.assign(normals, normals + 9 * (size_t) triangle_count);
  else {  // face normals, as the .obj path does for files without `vn` (wavefront.c:918-929)
    m.normals.resize(9 * (size_t) triangle_count);
    for (uint32_t t = 0; t < triangle_count; t++) {
      const float* p = positions + 9 * (size_t) t;
      const float e1[3] = {p[3] - p[0], p[4] - p[1], p[5] - p[2]}, e2[3] = {p[6] - p[0], p[7] - p[1], p[8] - p[2]};
      float n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
      const float rl = 1.0f / std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
      if (!std::isnan(rl) && !std::isinf(rl)) { n[0] *= rl; n[1] *= rl; n[2] *= rl; }
      for (int k = 0; k < 3; k++) std::memcpy(&m.normals[9 * (size_t) t + 3 * k], n, sizeof(n));
    }
  }
  host->scene.meshes.push_back(std::move(m));
  if (mesh_id) *mesh_id = (uint32_t) host->scene.meshes.size() - 1;
  invalidate(host, LUMC_DIRTY_MESHES | LUMC_DIRTY_INSTANCES | LUMC_DIRTY_LIGHTS);
  return LUMINARY_SUCCESS;
}
static void face_normals(const float* positions, uint32_t triangle_count, float* normals) {  // as the .obj path does for files without `vn` (wavefront.c:918-929; loaders.cpp)
  for (uint32_t t = 0; t < triangle_count; t++) {
    const float* p = positions + 9 * (size_t) t;
    const float e1[3] = {p[3] - p[0], p[4] - p[1], p[5] - p[2]}, e2[3] = {p[6] - p[0], p[7] - p[1], p[8] - p[2]};
    float n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
    const float rl = 1.0f / std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    if (!std::isnan(rl) && !std::isinf(rl)) { n[0] *= rl; n[1] *= rl; n[2] *= rl; }
    const float rl2 = 1.0f / std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);  // the loader normalises every vertex normal it stores, the face normal included
    if (!std::isnan(rl2) && !std::isinf(rl2)) { n[0] *= rl2; n[1] *= rl2; n[2] *= rl2; }
    for (int k = 0; k < 3; k++) std::memcpy(normals + 9 * (size_t) t + 3 * k, n, sizeof(n));
  }
}
static void mark_moved(LuminaryHost* host, uint32_t mesh_id) {
  shutter_note_mesh(host, mesh_id);
  if (std::find(host->moved_meshes.begin(), host->moved_meshes.end(), mesh_id) == host->moved_meshes.end()) host->moved_meshes.push_back(mesh_id);
}
LuminaryResult luminary_ext_set_mesh_positions(LuminaryHost* host, uint32_t mesh_id, const float* positions, const float* normals, uint32_t triangle_count) {
  CHECK_NULL(host);
  ApiLock lock(host);
  if (!positions || mesh_id >= host->scene.meshes.size() || host->scene.meshes[mesh_id].triangle_count() != triangle_count) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  if (host->skins.count(mesh_id)) return LUMINARY_ERROR_INVALID_API_ARGUMENT;  // a bound mesh moves by its bones (luminary_ext_set_mesh_pose)
  for (size_t i = 0; i < 9 * (size_t) triangle_count; i++) if (!std::isfinite(positions[i])) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  lum::HostMesh& m = host->scene.meshes[mesh_id];
  // in place (std::copy into the vectors as they are): the pointers luminary_ext_get_mesh handed out stay valid. The caller may pass those very pointers.
  if (normals) std::memmove(m.normals.data(), normals, sizeof(float) * 9 * (size_t) triangle_count);
  std::memmove(m.positions.data(), positions, sizeof(float) * 9 * (size_t) triangle_count);
  if (!normals) face_normals(m.positions.data(), triangle_count, m.normals.data());
  mark_moved(host, mesh_id);
  shutter_note_move(host, mesh_emits(host, mesh_id));
  invalidate(host, LUMC_DIRTY_MESH_POSITIONS | moved_emitter_bit(host));  // the vertices and the mesh's tree; the light tree follows moved emitters
  return LUMINARY_SUCCESS;
}
// A bound mesh got a new pose or new weights: the devices write its vertices, the host mesh follows when something reads it.
static void deformed(LuminaryHost* host, uint32_t mesh_id, HostSkin& k) {
  shutter_note_mesh(host, mesh_id);
  k.host_current = false; k.view_current = false;
  uint32_t dirty = LUMC_DIRTY_MESH_SKIN;
  if (mesh_emits(host, mesh_id)) {
    if (host->light_refit) dirty |= LUMC_DIRTY_LIGHT_POSITIONS;  // the devices refit the light tree from the vertices they write: the host mesh stays lazy
    else { materialise(host, mesh_id); dirty |= LUMC_DIRTY_LIGHTS; }  // the light tree is built from the host mesh
  }
  shutter_note_move(host, (dirty & (LUMC_DIRTY_LIGHTS | LUMC_DIRTY_LIGHT_POSITIONS)) != 0);
  invalidate(host, dirty);
}
// One of a mesh's two bindings went, or was replaced, while the other stays, and the one that went had shaped the mesh: the mesh is what the other one makes of the
// shared rest shape. Its pose or weights are handed to every context again (which marks the mesh moved there); with neither, the rest shape itself goes up as moved
// vertices.
static void rebound(LuminaryHost* host, uint32_t mesh_id, HostSkin& k) {
  if (k.posed()) k.pose_serial = ++host->skin_serial;
  if (k.weighted()) k.morph_weights_serial = ++host->skin_serial;
  if (k.posed() || k.weighted()) { deformed(host, mesh_id, k); return; }
  lum::HostMesh& m = host->scene.meshes[mesh_id];
  std::copy(k.rest_positions.begin(), k.rest_positions.end(), m.positions.begin());  // in place: the pointers luminary_ext_get_mesh handed out stay valid
  std::copy(k.rest_normals.begin(), k.rest_normals.end(), m.normals.begin());
  k.host_current = true; k.view_current = true;
  mark_moved(host, mesh_id);
  invalidate(host, LUMC_DIRTY_MESH_POSITIONS | (mesh_emits(host, mesh_id) ? moved_emitter_bit(host) : 0));
}
// The first binding of a mesh, or another of the only kind it holds: the rest shape is the host mesh as it is now (bound before: the current pose).
static HostSkin& bind_fresh(LuminaryHost* host, uint32_t mesh_id) {
  materialise(host, mesh_id);
  const lum::HostMesh& m = host->scene.meshes[mesh_id];
  HostSkin k;
  k.rest_positions = m.positions; k.rest_normals = m.normals;
  const auto old = host->skins.find(mesh_id);
  const bool stale_view = old != host->skins.end() && !old->second.view_current;
  host->skins[mesh_id] = std::move(k);  // (the vertices stay where they are: nothing restarts; the contexts get the binding before their next update)
  if (stale_view) {  // bound and posed before: a context trusts the view's vertices of a mesh until its first pose under the new binding, so they are encoded again
    mark_moved(host, mesh_id);
    invalidate(host, LUMC_DIRTY_MESH_POSITIONS);
  }
  return host->skins[mesh_id];
}
static void unbind_in_contexts(LuminaryHost* host, uint32_t mesh_id, int (*unbind)(LumContext*, uint32_t)) {
  // every context that holds the binding drops it (one that never got it refuses: nothing to drop)
  if (host->core) (void) unbind(host->core, mesh_id);
  for (uint32_t i = 0; i < host->devices.size(); i++)
    if (i != host->main_slot && host->devices[i].core) (void) unbind(host->devices[i].core, mesh_id);
}
// The last of a mesh's bindings goes: the host mesh becomes the current pose, and plain again.
static void unbind_last(LuminaryHost* host, uint32_t mesh_id) {
  materialise(host, mesh_id);
  const auto it = host->skins.find(mesh_id);
  const bool view_current = it->second.view_current;
  host->skins.erase(it);
  if (!view_current) {  // the device scene's vertices of the mesh are re-encoded from the host mesh, as for moved vertices; the devices' are that pose already
    mark_moved(host, mesh_id);
    invalidate(host, LUMC_DIRTY_MESH_POSITIONS);
  }
}

LuminaryResult luminary_ext_bind_mesh_skin(LuminaryHost* host, uint32_t mesh_id, const uint16_t* bone_ids, const float* weights, uint32_t triangle_count, uint32_t bone_count) {
  CHECK_NULL(host);
  ApiLock lock(host);
  if (!bone_ids || !weights || mesh_id >= host->scene.meshes.size() || host->scene.meshes[mesh_id].triangle_count() != triangle_count) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  if (bone_count == 0 || bone_count > lum::kSkinMaxBones) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  for (size_t i = 0; i < 12 * (size_t) triangle_count; i++)
    if (bone_ids[i] >= bone_count || !(weights[i] >= 0.0f) || !std::isfinite(weights[i])) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  const auto old = host->skins.find(mesh_id);
  const bool shares_rest = old != host->skins.end() && old->second.has_morph();  // a morph is bound: its rest shape is the skin's
  const bool was_posed = shares_rest && old->second.posed();
  HostSkin& k = shares_rest ? old->second : bind_fresh(host, mesh_id);
  k.bone_ids.assign(bone_ids, bone_ids + 12 * (size_t) triangle_count);
  k.weights.assign(weights, weights + 12 * (size_t) triangle_count);
  k.bone_count = bone_count;
  k.palette.clear(); k.pose_serial = 0;
  k.bind_serial = ++host->skin_serial;
  if (was_posed) rebound(host, mesh_id, k);
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_set_mesh_pose(LuminaryHost* host, uint32_t mesh_id, const float* bones, uint32_t bone_count) {
  CHECK_NULL(host);
  ApiLock lock(host);
  const auto it = host->skins.find(mesh_id);
  if (!bones || it == host->skins.end() || !it->second.has_skin() || bone_count != it->second.bone_count) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  for (size_t i = 0; i < 12 * (size_t) bone_count; i++) if (!std::isfinite(bones[i])) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  HostSkin& k = it->second;
  k.palette.assign(bones, bones + 12 * (size_t) bone_count);
  k.pose_serial = ++host->skin_serial;
  deformed(host, mesh_id, k);
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_unbind_mesh_skin(LuminaryHost* host, uint32_t mesh_id) {
  CHECK_NULL(host);
  ApiLock lock(host);
  const auto it = host->skins.find(mesh_id);
  if (it == host->skins.end() || !it->second.has_skin()) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  if (!it->second.has_morph()) unbind_last(host, mesh_id);
  unbind_in_contexts(host, mesh_id, lumc_mesh_skin_unbind);
  if (host->skins.count(mesh_id)) {  // the morph stays, over the same rest shape
    HostSkin& k = it->second;
    const bool was_posed = k.posed();
    k.bone_ids.clear(); k.weights.clear(); k.palette.clear();
    k.bone_count = 0; k.bind_serial = k.pose_serial = 0;
    if (was_posed) rebound(host, mesh_id, k);
  }
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_bind_mesh_morph(LuminaryHost* host, uint32_t mesh_id, uint32_t triangle_count, uint32_t target_count, const uint32_t* offsets, const uint32_t* corners,
                                            const float* delta_positions, const float* delta_normals) {
  CHECK_NULL(host);
  ApiLock lock(host);
  if (mesh_id >= host->scene.meshes.size() || host->scene.meshes[mesh_id].triangle_count() != triangle_count) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  if (lum::morph_check(triangle_count, target_count, offsets, corners, delta_positions, delta_normals)) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  const auto old = host->skins.find(mesh_id);
  const bool shares_rest = old != host->skins.end() && old->second.has_skin();  // a skin is bound: its rest pose is the morph's base shape
  const bool was_weighted = shares_rest && old->second.weighted();
  HostSkin& k = shares_rest ? old->second : bind_fresh(host, mesh_id);
  const size_t entries = offsets[target_count];
  k.target_count = target_count;
  k.morph_offsets.assign(offsets, offsets + target_count + 1);
  k.morph_corners.clear(); k.morph_delta_positions.clear(); k.morph_delta_normals.clear();
  if (entries) {
    k.morph_corners.assign(corners, corners + entries);
    k.morph_delta_positions.assign(delta_positions, delta_positions + 3 * entries);
    if (delta_normals) k.morph_delta_normals.assign(delta_normals, delta_normals + 3 * entries);
  }
  lum::morph_csr(triangle_count, target_count, offsets, corners, delta_positions, delta_normals, &k.morph_csr);
  k.morph_weights.assign(target_count, 0.0f); k.morph_weights_serial = 0;
  k.morph_bind_serial = ++host->skin_serial;
  if (was_weighted) rebound(host, mesh_id, k);
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_set_mesh_weights(LuminaryHost* host, uint32_t mesh_id, const float* weights, uint32_t target_count) {
  CHECK_NULL(host);
  ApiLock lock(host);
  const auto it = host->skins.find(mesh_id);
  if (!weights || it == host->skins.end() || !it->second.has_morph() || target_count != it->second.target_count) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  for (uint32_t t = 0; t < target_count; t++) if (!std::isfinite(weights[t])) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  HostSkin& k = it->second;
  k.morph_weights.assign(weights, weights + target_count);
  k.morph_weights_serial = ++host->skin_serial;
  deformed(host, mesh_id, k);
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_unbind_mesh_morph(LuminaryHost* host, uint32_t mesh_id) {
  CHECK_NULL(host);
  ApiLock lock(host);
  const auto it = host->skins.find(mesh_id);
  if (it == host->skins.end() || !it->second.has_morph()) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  if (!it->second.has_skin()) unbind_last(host, mesh_id);
  unbind_in_contexts(host, mesh_id, lumc_mesh_morph_unbind);
  if (host->skins.count(mesh_id)) {  // the skin stays, over the same rest pose
    HostSkin& k = it->second;
    const bool was_weighted = k.weighted();
    k.morph_offsets.clear(); k.morph_corners.clear(); k.morph_delta_positions.clear(); k.morph_delta_normals.clear(); k.morph_weights.clear();
    k.morph_csr = lum::MorphCsr{};
    k.target_count = 0; k.morph_bind_serial = k.morph_weights_serial = 0;
    if (was_weighted) rebound(host, mesh_id, k);
  }
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_get_mesh_morph_stats(LuminaryHost* host, LuminaryMeshMorphStats* out) {
  CHECK_NULL(host); CHECK_NULL(out);
  ApiLock lock(host);
  std::memset(out, 0, sizeof(*out));
  out->host_materialisations = host->host_materialisations;
  if (!host->core) return LUMINARY_SUCCESS;
  LumMeshMorphStats s;
  if (lumc_mesh_morph_stats(host->core, &s)) return LUMINARY_ERROR_API_EXCEPTION;
  static_assert(sizeof(LuminaryMeshMorphStats) == sizeof(LumMeshMorphStats) + sizeof(uint64_t) && offsetof(LuminaryMeshMorphStats, host_materialisations) == sizeof(LumMeshMorphStats),
                "the public struct mirrors the core's, host_materialisations behind it");
  std::memcpy(out, &s, sizeof(s));
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_get_mesh_skin_stats(LuminaryHost* host, LuminaryMeshSkinStats* out) {
  CHECK_NULL(host); CHECK_NULL(out);
  ApiLock lock(host);
  std::memset(out, 0, sizeof(*out));
  out->host_materialisations = host->host_materialisations;
  if (!host->core) return LUMINARY_SUCCESS;
  LumMeshSkinStats s;
  if (lumc_mesh_skin_stats(host->core, &s)) return LUMINARY_ERROR_API_EXCEPTION;
  static_assert(sizeof(LuminaryMeshSkinStats) == sizeof(LumMeshSkinStats) + sizeof(uint64_t) && offsetof(LuminaryMeshSkinStats, host_materialisations) == sizeof(LumMeshSkinStats),
                "the public struct mirrors the core's, host_materialisations behind it");
  std::memcpy(out, &s, sizeof(s));
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_set_mesh_refit(LuminaryHost* host, uint32_t mode, float max_cost_growth) {
  CHECK_NULL(host);
  ApiLock lock(host);
  if (mode > 1 || !(max_cost_growth >= 0.0f) || !std::isfinite(max_cost_growth)) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  host->refit_mode = mode; host->refit_max_cost_growth = max_cost_growth;  // (decides how the next moved mesh is taken over: no restart)
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_get_mesh_refit_stats(LuminaryHost* host, LuminaryMeshRefitStats* out) {
  CHECK_NULL(host); CHECK_NULL(out);
  ApiLock lock(host);
  std::memset(out, 0, sizeof(*out));
  if (!host->core) return LUMINARY_SUCCESS;
  LumMeshRefitStats s;
  if (lumc_mesh_refit_stats(host->core, &s)) return LUMINARY_ERROR_API_EXCEPTION;
  static_assert(sizeof(LuminaryMeshRefitStats) == sizeof(LumMeshRefitStats), "the public struct mirrors the core's");
  std::memcpy(out, &s, sizeof(s));
  return LUMINARY_SUCCESS;
}
// Does this set of new transforms keep the image history (with the motion on)? It does unless an instance whose transform changes has an emissive material:
// the reprojection follows surfaces, not the light they cast. The arguments are valid (luminary_ext_set_instance_transforms checked them).
bool instance_change_carries(const LuminaryHost* host, const LuminaryInstance* instances, uint32_t count) {
  for (uint32_t k = 0; k < count; k++) {
    const lum::HostInstance& i = host->scene.instances[instances[k].id];
    const LuminaryInstance& in = instances[k];
    const bool changed = std::memcmp(&i.translation, &in.position, sizeof(in.position)) != 0 || std::memcmp(&i.rotation, &in.rotation, sizeof(in.rotation)) != 0 ||
                         std::memcmp(&i.scale, &in.scale, sizeof(in.scale)) != 0;
    if (changed && mesh_emits(host, i.mesh_id)) return false;
  }
  return true;
}
LuminaryResult luminary_ext_instance_change_carries_history(LuminaryHost* host, const LuminaryInstance* instances, uint32_t count, bool* carries) {
  CHECK_NULL(host); CHECK_NULL(carries);
  ApiLock lock(host);
  *carries = false;
  if (!instances && count) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  const lum::HostScene& sc = host->scene;
  for (uint32_t k = 0; k < count; k++) {
    const LuminaryInstance& in = instances[k];
    if (in.id >= sc.instances.size()) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
    const lum::HostInstance& i = sc.instances[in.id];
    if (!i.active || i.mesh_id >= sc.meshes.size() || in.mesh_id != i.mesh_id) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  }
  *carries = count > 0 && history_motion_on(host) && !host->scene.camera.use_physical_camera && instance_change_carries(host, instances, count);
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_set_instance_transforms(LuminaryHost* host, const LuminaryInstance* instances, uint32_t count) {
  CHECK_NULL(host);
  ApiLock lock(host);
  if (!instances && count) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  const lum::HostScene& sc = host->scene;
  for (uint32_t k = 0; k < count; k++) {  // all of them before anything changes
    const LuminaryInstance& in = instances[k];
    if (in.id >= sc.instances.size()) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
    const lum::HostInstance& i = sc.instances[in.id];
    if (!i.active || i.mesh_id >= sc.meshes.size() || in.mesh_id != i.mesh_id) return LUMINARY_ERROR_INVALID_API_ARGUMENT;  // (an instance that points at no mesh is inactive: scene.cpp)
    const float f[9] = {in.position.x, in.position.y, in.position.z, in.rotation.x, in.rotation.y, in.rotation.z, in.scale.x, in.scale.y, in.scale.z};
    for (float x : f) if (!std::isfinite(x)) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  }
  if (count == 0) return LUMINARY_SUCCESS;
  bool emitter = false;
  const bool carries = instance_change_carries(host, instances, count);
  for (uint32_t k = 0; k < count; k++) {
    lum::HostInstance& i = host->scene.instances[instances[k].id];
    i.translation = instances[k].position; i.rotation = instances[k].rotation; i.scale = instances[k].scale;
    emitter = emitter || (host->shutter.open && mesh_emits(host, i.mesh_id));
  }
  shutter_note_move(host, emitter);
  if (history_motion_on(host) && !host->scene.camera.use_physical_camera) {
    if (carries) host->history_instance_move = true;
    else host->history_cause = "a moved instance emits";
  }
  invalidate(host, LUMC_DIRTY_INSTANCE_TRANSFORMS | moved_emitter_bit(host));  // the transforms and the top-level tree; the light tree follows moved emitters
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_set_instance_update(LuminaryHost* host, uint32_t mode) {
  CHECK_NULL(host);
  ApiLock lock(host);
  if (mode > 1) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  host->instance_update_mode = mode;  // (decides how the next moved instances are taken over: no restart)
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_get_instance_update_stats(LuminaryHost* host, LuminaryInstanceUpdateStats* out) {
  CHECK_NULL(host); CHECK_NULL(out);
  ApiLock lock(host);
  std::memset(out, 0, sizeof(*out));
  if (!host->core) return LUMINARY_SUCCESS;
  LumInstanceUpdateStats s;
  if (lumc_instance_update_stats(host->core, &s)) return LUMINARY_ERROR_API_EXCEPTION;
  static_assert(sizeof(LuminaryInstanceUpdateStats) == sizeof(LumInstanceUpdateStats), "the public struct mirrors the core's");
  std::memcpy(out, &s, sizeof(s));
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_set_mesh_refit_in_place(LuminaryHost* host, uint32_t on) {
  CHECK_NULL(host);
  ApiLock lock(host);
  if (on > 1) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  host->refit_in_place = on;  // (decides how the next moved vertices are taken over: no restart)
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_get_resident_refit_stats(LuminaryHost* host, LuminaryResidentRefitStats* out) {
  CHECK_NULL(host); CHECK_NULL(out);
  ApiLock lock(host);
  std::memset(out, 0, sizeof(*out));
  if (!host->core) return LUMINARY_SUCCESS;
  LumResidentRefitStats s;
  if (lumc_resident_refit_stats(host->core, &s)) return LUMINARY_ERROR_API_EXCEPTION;
  static_assert(sizeof(LuminaryResidentRefitStats) == sizeof(LumResidentRefitStats), "the public struct mirrors the core's");
  std::memcpy(out, &s, sizeof(s));
  return LUMINARY_SUCCESS;
}
// The host-level mesh as the loaders left it (the reference's Mesh / TriangleGeomData, mesh.h:8-14): borrowed pointers, valid until the mesh list changes. What an
// independent encoder (the test oracle's o_scene.c) starts from.
LuminaryResult luminary_ext_get_mesh(LuminaryHost* host, uint32_t mesh_id, const float** positions, const float** normals, const float** uvs,
                                     const uint16_t** material_ids, uint32_t* triangle_count) {
  CHECK_NULL(host); CHECK_NULL(triangle_count);
  ApiLock lock(host);
  if (mesh_id >= host->scene.meshes.size()) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  materialise(host, mesh_id);  // (a posed mesh: the host mesh is lazy)
  const lum::HostMesh& m = host->scene.meshes[mesh_id];
  if (positions) *positions = m.positions.data();
  if (normals) *normals = m.normals.data();
  if (uvs) *uvs = m.uvs.data();
  if (material_ids) *material_ids = m.material_ids.data();
  *triangle_count = m.triangle_count();
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_add_material(LuminaryHost* host, const LuminaryMaterial* material, uint16_t* material_id) {
  CHECK_NULL(host); CHECK_NULL(material);
  ApiLock lock(host);
  if (host->scene.materials.size() >= 0xFFFF) return LUMINARY_ERROR_API_EXCEPTION;
  host->scene.materials.push_back(*material);
  host->scene.materials.back().id = (uint32_t) host->scene.materials.size() - 1;
  if (material_id) *material_id = (uint16_t) (host->scene.materials.size() - 1);
  invalidate(host, LUMC_DIRTY_MATERIALS | LUMC_DIRTY_LIGHTS);
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_build_device_scene(LuminaryHost* host, const LumDeviceSceneView** view) {
  CHECK_NULL(host); CHECK_NULL(view);
  ApiLock lock(host);
  const LuminaryResult r = ensure_device_scene(host);
  if (r) return r;
  // An independent consumer sees a current view: the vertices of posed meshes, which the contexts never read and the render path therefore leaves stale, are
  // encoded from the materialised host meshes. Nothing the contexts hold changes: no dirty flag, no restart.
  for (auto& kv : host->skins) {
    if (kv.second.view_current) continue;
    materialise(host, kv.first);
    host->device_scene.moved_meshes.push_back(kv.first);
    kv.second.view_current = true;
  }
  if (!host->device_scene.moved_meshes.empty()) {
    const std::string err = lum::update_device_scene(host->scene, host->device_scene.bluenoise, LUMC_DIRTY_MESH_POSITIONS, &host->device_scene);
    if (!err.empty()) return LUMINARY_ERROR_API_EXCEPTION;
  }
  if (host->view_lights_stale) {
    // the view's light arrays as the devices now hold them: the twin of their kernels over the view's vertices; where that reports a fragment that left the set
    // of lights (the devices asked for a rebuild, or will) the tree is built again
    lum::DeviceSceneBuffers& b = host->device_scene;
    lum::refresh_light_refit_transforms(host->scene, &b.light_refit_plan);
    const LumLightRefitPlan plan = b.light_refit_plan.view();
    LumLightRefitReport report{};
    bool refitted = false;
    if (plan.num_fragments >= 2 && !b.light_tree_root.empty()) {
      std::vector<float> table((size_t) b.light_tree_root[10] * 64 + 16, 0.0f);
      refitted = lum::light_refit_host(&plan, b.vertices.data(), b.mesh_tri_offset.data(), b.light_tree_root.data(), table.data(), b.light_tree_nodes.data(), b.light_bvh_tris.data(),
                                       nullptr, &report) == 0 && report.refitted;
    }
    if (!refitted && plan.num_fragments) {
      const std::string err = lum::update_device_scene(host->scene, b.bluenoise, LUMC_DIRTY_LIGHTS, &b);
      if (!err.empty()) return LUMINARY_ERROR_API_EXCEPTION;
      host->core_dirty |= LUMC_DIRTY_LIGHTS; host->core_scene_valid = false;
      for (auto& slot : host->devices) { slot.dirty |= LUMC_DIRTY_LIGHTS; slot.scene_valid = false; }
    }
    host->view_lights_stale = false;
  }
  *view = &host->device_scene.view;
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_set_light_refit(LuminaryHost* host, uint32_t on, float max_cost_growth) {
  CHECK_NULL(host);
  ApiLock lock(host);
  if (on > 1 || !(max_cost_growth >= 0.0f) || !std::isfinite(max_cost_growth)) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  const bool switched = (on != 0) != (host->light_refit != 0);
  host->light_refit = on; host->light_refit_max_cost_growth = max_cost_growth;
  // Switched on: the contexts get the plan with their next LUMC_DIRTY_LIGHTS update, so the lights' part is handed over once more. Switched off: the tree is built
  // from the scene as it stands and every context takes it, which drops its binding - from there on every path is the one without the switch, whatever was refitted
  // or still pending before.
  if (switched) invalidate(host, LUMC_DIRTY_LIGHTS);
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_get_light_refit_stats(LuminaryHost* host, LuminaryLightRefitStats* out) {
  CHECK_NULL(host); CHECK_NULL(out);
  ApiLock lock(host);
  std::memset(out, 0, sizeof(*out));
  out->host_rebuilds = host->light_rebuilds;
  if (!host->core) return LUMINARY_SUCCESS;
  LumLightRefitStats s;
  if (lumc_light_refit_stats(host->core, &s)) return LUMINARY_ERROR_API_EXCEPTION;
  static_assert(sizeof(LuminaryLightRefitStats) == sizeof(LumLightRefitStats) + sizeof(uint64_t) && offsetof(LuminaryLightRefitStats, host_rebuilds) == sizeof(LumLightRefitStats),
                "the public struct mirrors the core's, host_rebuilds behind it");
  std::memcpy(out, &s, sizeof(s));
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_get_light_refit_plan(LuminaryHost* host, LumLightRefitPlan* plan) {
  CHECK_NULL(host); CHECK_NULL(plan);
  ApiLock lock(host);
  const LuminaryResult r = ensure_device_scene(host);
  if (r) return r;
  *plan = host->device_scene.light_refit_plan.view();
  return LUMINARY_SUCCESS;
}
namespace {
// camera / settings -> device-side output state (device_structs.c:40-88: exposure is stored as exp(exposure))
LumOutputParams output_params(const LuminaryHost* h, uint32_t dst_width, uint32_t dst_height) {
  const LuminaryCamera& c = h->scene.camera;
  const LumDeviceSceneView& v = h->device_scene.view;
  LumOutputParams p;
  std::memset(&p, 0, sizeof(p));
  p.src_width = v.width; p.src_height = v.height; p.dst_width = dst_width; p.dst_height = dst_height;
  p.inv_sample_count = 1.0f / (float) h->accumulated_samples;
  p.exposure = std::exp(c.exposure);
  p.tonemap = (uint32_t) c.tonemap; p.filter = (uint32_t) c.filter; p.dithering = c.dithering ? 1u : 0u;
  p.purkinje = (c.purkinje && !c.use_physical_camera) ? 1u : 0u;  // device_structs.c:48: no Purkinje shift behind the physical camera
  p.use_color_correction = c.use_color_correction ? 1u : 0u;
  // tonemap_apply leaves the pixel alone for debug shading modes and for the adaptive-sampling diagnostic images (tonemap.cuh:206-211)
  p.passthrough = (h->scene.settings.shading_mode != LUMINARY_SHADING_MODE_DEFAULT ||
                   h->scene.settings.adaptive_sampling_output_mode != LUMINARY_ADAPTIVE_SAMPLING_OUTPUT_MODE_BEAUTY) ? 1u : 0u;
  p.purkinje_kappa1 = c.purkinje_kappa1; p.purkinje_kappa2 = c.purkinje_kappa2;
  p.cc_h = c.color_correction.r; p.cc_s = c.color_correction.g; p.cc_v = c.color_correction.b;
  p.film_grain = c.film_grain;
  p.agx_slope = c.agx_custom_slope; p.agx_power = c.agx_custom_power; p.agx_saturation = c.agx_custom_saturation;
  p.supersampling = h->scene.settings.supersampling;  // the frame is rendered at output size << supersampling (device_structs.c:20-21)
  return p;
}

// One render iteration of the undersampling preview (device.c:392-420): stage > 0 while the frame's first sample is rendered coarse to fine.
struct PreviewState { uint32_t stage = 0, iteration = 0; };

// device_setup_undersampling, device.c:1281-1310: the preview runs only when somebody watches (recurring outputs), never for render regions.
// Schedule: stage N with iterations 3..0, stages N-1..1 with iterations 2..0.
std::vector<PreviewState> preview_schedule(LuminaryHost* h) {
  std::vector<PreviewState> out;
  const LuminaryRendererSettings& st = h->scene.settings;
  if (!h->outputs.properties().enabled || !(st.region_width >= 1.0f && st.region_height >= 1.0f)) return out;
  // (with several devices the main device renders the coarse-to-fine first sample alone; the tiles then take its sums over: lumc_accumulators_from_frame)
  for (uint32_t stage = st.undersampling & 31u; stage > 0; stage--)
    for (uint32_t it = (stage == (st.undersampling & 31u)) ? 4u : 3u; it-- > 0;) { PreviewState ps; ps.stage = stage; ps.iteration = it; out.push_back(ps); }
  return out;
}

// accumulation_generate_result (accumulation.cuh:86-200) into the core's result image; the output chain then reads that image with a
// sample count of one. Returns the parameters to hand to lumc_generate_output*.
// device_post_apply (device/device_post.c:204-226), run between the result image and the display chain: bloom, for beauty images of
// the whole frame in the default shading mode
// The denoiser on the main context's result image (lumc_denoise). Its guides are rendered once per accumulation: whatever restarts the integration
// drops them (invalidate and the other places that zero accumulated_samples).
int denoise_result(LuminaryHost* h) {
  if (!h->guides_valid || !lumc_has_guides(h->core)) {
    if (render_guides(h)) return 1;
    h->guides_valid = true;
  }
  LumDenoiseParams dp;
  dp.iterations = h->denoiser.iterations; dp.sigma_luminance = h->denoiser.sigma_luminance; dp.sigma_normal = h->denoiser.sigma_normal;
  dp.sigma_depth = h->denoiser.sigma_depth; dp.uniform_samples = h->adaptive_active ? 0u : h->accumulated_samples;
  return lumc_denoise(h->core, &dp, nullptr, nullptr);
}

// The firefly resolve on the main context's result image (lumc_firefly_resolve), where the main context holds buckets (sync_firefly).
int firefly_result(LuminaryHost* h) {
  if (!h->core_firefly || h->partition_n > 1) return 0;
  if (h->adaptive_active) { h->firefly_skipped++; return 0; }  // the adaptive sampler's passes fill no buckets: skipped and counted
  if (lumc_firefly_resolve(h->core, nullptr, nullptr)) return 1;
  h->firefly_resolved++;
  return 0;
}

// The image history on the main context's result image (lumc_history_carry, lumc_history_blend), after the denoiser: the first output of an accumulation that
// camera moves alone restarted reprojects the held frame, every output blends. The guides are the denoiser's, rendered here where it is off.
int history_result(LuminaryHost* h) {
  if (h->adaptive_active) { h->history_skipped++; return 0; }  // every pixel has its own sample count: skipped and counted, as the firefly resolve is
  LumHistoryParams hp;
  hp.enabled = 1u; hp.max_history = h->history.max_history; hp.depth_tolerance = h->history.depth_tolerance; hp.normal_threshold = h->history.normal_threshold;
  hp.clamp_sigma = h->history.clamp_sigma;
  if (lumc_set_history(h->core, &hp)) return 1;
  LumHistoryMotionParams mp;
  mp.enabled = history_motion_on(h) ? 1u : 0u; mp.motion_max_history = h->history_motion.motion_max_history;
  if (lumc_set_history_motion(h->core, &mp)) return 1;
  if (history_motion_on(h) && !lumc_has_history_owner(h->core)) h->guides_valid = false;  // (the guides were made before the motion was switched on: again, with their owner plane)
  if (!h->guides_valid || !lumc_has_guides(h->core)) {
    if (render_guides(h)) return 1;
    h->guides_valid = true;
  }
  if (h->history_carry_due) {
    h->history_carry_due = false; h->history_carry_instances = false;
    if (history_held(h)) {
      if (lumc_history_carry(h->core, nullptr)) return 1;
      h->history_carried++;
    }
  }
  return lumc_history_blend(h->core, h->accumulated_samples, nullptr, nullptr);
}

int post_process(LuminaryHost* h, PreviewState preview) {
  const LuminaryRendererSettings& st = h->scene.settings;
  if (st.shading_mode != LUMINARY_SHADING_MODE_DEFAULT || st.adaptive_sampling_output_mode != LUMINARY_ADAPTIVE_SAMPLING_OUTPUT_MODE_BEAUTY) return 0;
  if (!(st.region_width >= 1.0f && st.region_height >= 1.0f)) return 0;
  if (preview.stage == 0 && firefly_result(h)) return 1;  // result image -> firefly resolve -> denoise -> bloom; never the coarse preview images
  if (h->denoiser.enabled && preview.stage == 0 && denoise_result(h)) return 1;
  if (h->history.enabled && preview.stage == 0 && history_result(h)) return 1;
  const float blend = h->scene.camera.bloom_blend;
  if (!(blend > 0.0f)) return 0;  // device_post_update, device_post.c:186-202
  const LumDeviceSceneView& v = h->device_scene.view;
  return lumc_post_bloom(h->core, nullptr, v.width, v.height, preview.stage, blend, nullptr);
}

int result_image(LuminaryHost* h, LumOutputParams* p, PreviewState preview) {
  if (preview.stage) {  // accumulation_generate_result_undersampling (device_renderer.c:410-420): the coarse image of the pixels that exist so far
    if (lumc_generate_result_undersampled(h->core, preview.stage, preview.iteration, nullptr, nullptr)) return 1;
    p->inv_sample_count = 1.0f;
    p->undersampling_stage = preview.stage;
    return post_process(h, preview);
  }
  const uint32_t mode = (uint32_t) h->scene.settings.adaptive_sampling_output_mode;
  const uint32_t lem = h->scene.camera.use_local_error_minimization ? 1u : 0u;
  if (lumc_generate_result(h->core, mode, lem, h->adaptive_active ? 0u : h->accumulated_samples, p->exposure, p, nullptr, nullptr)) return 1;
  p->inv_sample_count = 1.0f;
  return post_process(h, preview);
}

// device_output_generate_output, device_output.c:203-270: the recurring output if enabled, then every request that is due now
// `preview`: the state of the iteration just rendered (device.c:1509-1536 generates the output before the state advances).
// Tiled render: the moments of all devices on the main device (one grouped RCCL reduce; peer copies without a communicator), which the
// result / output entry points of the main context then read.
LuminaryResult assemble_partition(LuminaryHost* h) {
  if (h->partition_n <= 1) return LUMINARY_SUCCESS;
  std::vector<LumContext*> cores;
  for (LuminaryHost::DeviceSlot* slot : enabled_slots(h)) if (slot->core) cores.push_back(slot->core);
  if (cores.size() != h->partition_n || cores[0] != h->core) return LUMINARY_ERROR_API_EXCEPTION;
  const LumDeviceSceneView& v = h->device_scene.view;
  // uniform tiled rendering: the devices hold the shares of the 32x32 tile deal, so the frame is a gather of their own pixels (1 / n of a reduce's bytes);
  // adaptive rendering keeps full-frame accumulators with a block mask per device: those frames are summed
  const bool gathered = !h->adaptive_active && lumc_frame_gather_all(cores.data(), (int) cores.size(), v.width, v.height, 0, nullptr) == 0;
  if ((!gathered && lumc_frame_assemble_all(cores.data(), (int) cores.size(), v.width * v.height, 0, nullptr)) || lumc_use_assembled_frame(h->core, 1)) {
    std::fprintf(stderr, "[luminary_amd] %s\n", lumc_last_error(h->core));
    return LUMINARY_ERROR_CUDA;
  }
  return LUMINARY_SUCCESS;
}

LuminaryResult produce_outputs(LuminaryHost* h, PreviewState preview = PreviewState()) {
  if (!h->pixels_all || (h->accumulated_samples == 0 && preview.stage == 0)) return LUMINARY_SUCCESS;
  const LuminaryOutputProperties props = h->outputs.properties();
  const bool wanted = (props.enabled && props.width >= 2 && props.height >= 2) || !h->outputs.pending_requests().empty();
  if (wanted) { const LuminaryResult ra = assemble_partition(h); if (ra) return ra; }
  lum::OutputMeta meta;
  meta.sample_count = h->accumulated_samples;
  meta.time = (float) h->render_seconds;
  if (props.enabled && props.width >= 2 && props.height >= 2) {
    meta.width = props.width; meta.height = props.height;
    const uint32_t handle = h->outputs.begin_recurring(meta);
    LumOutputParams p = output_params(h, meta.width, meta.height);
    if (result_image(h, &p, preview) || lumc_generate_output_host(h->core, &p, lumc_result_image(h->core), h->outputs.data(handle), nullptr)) {
      h->outputs.publish(handle);
      return LUMINARY_ERROR_CUDA;
    }
    h->outputs.publish(handle);
  }
  for (const LuminaryOutputRequestProperties& req : h->outputs.pending_requests()) {
    if (req.sample_count > 0 && req.sample_count != h->accumulated_samples) continue;
    meta.width = req.width; meta.height = req.height;
    uint32_t handle;
    if (h->outputs.begin_for_request(meta, &handle)) continue;
    LumOutputParams p = output_params(h, meta.width, meta.height);
    const int rc = result_image(h, &p, preview) || lumc_generate_output_host(h->core, &p, lumc_result_image(h->core), h->outputs.data(handle), nullptr);
    h->outputs.publish(handle);
    if (rc) return LUMINARY_ERROR_CUDA;
  }
  return LUMINARY_SUCCESS;
}
}  // namespace

namespace {
// Sample ids per wavefront pass of the render loop. Deep bounces keep few paths alive, so many ids share a pass to keep 256 CUs busy (hall +5 %,
// Example-class +26 %, scan +35 % from 8 to 32, profiles/r02_ab_experiments.txt) - but a pass is also the latency of the next image, so a frame
// that is being watched (recurring outputs) keeps 8. Round 6: 64 ids for a frame nobody watches (same box, 32 -> 64: hall +2.1 %, Example-class +10.7 %,
// scan +14 % samples/s, profiles/r06_ab_experiments.txt). Bounded by the work buffers: at most 128 M paths (about 64 GB of queues, a fifth of the 288 GB) per pass.
uint32_t pass_size(LuminaryHost* h) {
  const uint32_t want = h->outputs.properties().enabled ? 8u : 64u;
  const LuminaryRendererSettings& st = h->scene.settings;
  const uint64_t pixels = std::max<uint64_t>((uint64_t) (st.width << st.supersampling) * (st.height << st.supersampling), 1u);
  const uint64_t fit = std::max<uint64_t>((128ull << 20) / pixels, 1u);
  return (uint32_t) std::min<uint64_t>(want, fit);
}

// luminary_ext_render_samples with the host's mutex held by the caller
LuminaryResult render_samples_locked(LuminaryHost* host, const uint32_t* pixels, uint32_t num_pixels, uint32_t first_sample, uint32_t num_samples,
                                     uint32_t samples_per_pass) {
  std::vector<LumContext*> cores;
  LuminaryResult r = ensure_partition_cores(host, &cores);
  if (r) return r;
  const bool all = pixels == nullptr;
  // the whole frame is tiled over the enabled devices (32x32 tiles dealt by lumc_tile_owner's lattice, lumc_tile_pixels); pixel subsets stay on the main device
  const uint32_t want_n = (all && cores.size() > 1) ? (uint32_t) cores.size() : 1u;
  bool same = (host->num_pixels != 0) && (all == host->pixels_all) && (host->partition_n == want_n);
  if (same && !all) same = (host->pixels.size() == num_pixels) && std::memcmp(host->pixels.data(), pixels, sizeof(uint32_t) * num_pixels) == 0;
  if (host->adaptive_active) same = false;  // leaving adaptive mode restarts the accumulation
  if (!same) {
    const LumDeviceSceneView& v = host->device_scene.view;
    // the first sample of this frame was rendered on the main device as the preview: its sums go to whoever owns the pixels from now on
    const bool handoff = host->handoff_preview && all && first_sample == 1 && host->accumulated_samples == 1 && host->pixels_all && host->num_pixels == v.width * v.height;
    host->handoff_preview = false;
    if (!handoff) history_drop(host, "the pixel set or the device partition changed");
    if (handoff && lumc_frame_assemble(host->core, v.width * v.height, 0, nullptr, nullptr)) { std::fprintf(stderr, "[luminary_amd] %s\n", lumc_last_error(host->core)); return LUMINARY_ERROR_CUDA; }
    if (want_n > 1) {
      std::vector<uint32_t> tiles;
      for (uint32_t k = 0; k < want_n; k++) {
        uint32_t count = 0;
        lumc_tile_pixels(v.width, v.height, k, want_n, 32, nullptr, &count);
        tiles.resize(count ? count : 1);
        lumc_tile_pixels(v.width, v.height, k, want_n, 32, tiles.data(), &count);
        if (lumc_set_pixels(cores[k], tiles.data(), count)) { std::fprintf(stderr, "[luminary_amd] %s\n", lumc_last_error(cores[k])); return LUMINARY_ERROR_CUDA; }
      }
      if (!host->comm_ready) {  // one RCCL communicator over the partition's GPUs; without one the frame is assembled through peer copies
        if (lumc_comm_init_all(cores.data(), (int) want_n) == 0) host->comm_ready = true;
        else std::fprintf(stderr, "[luminary_amd] no RCCL communicator (%s): frames are assembled through peer copies\n", lumc_last_error(cores[0]));
      }
    }
    else {
      lumc_use_assembled_frame(host->core, 0);
      if (lumc_set_pixels(host->core, pixels, num_pixels)) return LUMINARY_ERROR_CUDA;
    }
    host->partition_n = want_n;
    host->adaptive_active = false;
    host->pixels_all = all;
    if (!all) host->pixels.assign(pixels, pixels + num_pixels);
    host->num_pixels = all ? v.width * v.height : num_pixels;
    host->accumulated_samples = 0;
    host->guides_valid = false;
    if (handoff) {
      for (uint32_t k = 0; k < want_n; k++)
        if (lumc_accumulators_from_frame(cores[k], host->core)) { std::fprintf(stderr, "[luminary_amd] %s\n", lumc_last_error(cores[k])); return LUMINARY_ERROR_CUDA; }
      host->accumulated_samples = 1;
    }
    else host->render_seconds = 0.0;
  }
  // stop at every sample count a pending request is keyed to (device_output.c:160-168), produce the outputs due there, go on
  uint32_t done = 0;
  while (done < num_samples) {
    uint32_t chunk = num_samples - done;
    for (const LuminaryOutputRequestProperties& req : host->outputs.pending_requests())
      if (req.sample_count > host->accumulated_samples && req.sample_count - host->accumulated_samples < chunk) chunk = req.sample_count - host->accumulated_samples;
    const auto t0 = std::chrono::steady_clock::now();
    // every device gets its kernels enqueued before the first one is waited for: the GPUs run side by side
    for (uint32_t k = 0; k < want_n; k++)
      if (lumc_render(cores[k], first_sample + done, chunk, samples_per_pass, nullptr, nullptr, nullptr)) { std::fprintf(stderr, "[luminary_amd] %s\n", lumc_last_error(cores[k])); return LUMINARY_ERROR_CUDA; }
    for (uint32_t k = 0; k < want_n; k++)
      if (lumc_synchronize(cores[k])) { std::fprintf(stderr, "[luminary_amd] %s\n", lumc_last_error(cores[k])); return LUMINARY_ERROR_CUDA; }
    { const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); host->render_seconds += dt; host->last_sample_ms = 1e3 * dt / (chunk ? chunk : 1u); }
    host->accumulated_samples += chunk;
    done += chunk;
    r = produce_outputs(host);
    if (r) return r;
  }
  return LUMINARY_SUCCESS;
}
}  // namespace

LuminaryResult luminary_ext_render_samples(LuminaryHost* host, const uint32_t* pixels, uint32_t num_pixels, uint32_t first_sample, uint32_t num_samples,
                                           uint32_t samples_per_pass) {
  CHECK_NULL(host);
  ApiLock lock(host);
  shutter_cancel(host);  // any other render call ends the shutter
  return render_samples_locked(host, pixels, num_pixels, first_sample, num_samples, samples_per_pass);
}

// ---- shutter (include/luminary_amd.h luminary_ext_shutter_open) ----
namespace {
float shutter_blend(float a, float b, float t) {  // one rounding per operation (this unit is compiled without contraction)
  const float d = b - a;
  const float s = t * d;
  return a + s;
}
LuminaryVec3 shutter_blend3(const LuminaryVec3& a, const LuminaryVec3& b, float t) {
  LuminaryVec3 r = b;
  r.x = shutter_blend(a.x, b.x, t); r.y = shutter_blend(a.y, b.y, t); r.z = shutter_blend(a.z, b.z, t);
  return r;
}
bool same_vec(const LuminaryVec3& a, const LuminaryVec3& b) { return std::memcmp(&a.x, &b.x, 4) == 0 && std::memcmp(&a.y, &b.y, 4) == 0 && std::memcmp(&a.z, &b.z, 4) == 0; }

LuminaryResult shutter_refuse(LuminaryHost* h, const std::string& why, bool cancel) {
  h->log.push_back("luminary_ext_render_shutter: " + why);
  std::fprintf(stderr, "[luminary_amd] luminary_ext_render_shutter: %s\n", why.c_str());
  if (cancel) shutter_cancel(h);
  return LUMINARY_ERROR_INVALID_API_ARGUMENT;
}

// The scene at time t between the keys on every context: the host's camera and moved instances blended (`close`: the close key's own values, verbatim) and
// encoded into the device scene, the moved meshes written by the devices. *rebuild: a device's light refit asked for a rebuild.
int shutter_apply_time(LuminaryHost* h, const std::vector<LumContext*>& cores, float t, bool close, const LuminaryCamera& close_camera,
                       const std::vector<HostShutter::Pose>& close_instances, bool* rebuild) {
  HostShutter& sh = h->shutter;
  if (sh.camera_moved) {
    h->scene.camera.pos = close ? close_camera.pos : shutter_blend3(sh.camera_pos, close_camera.pos, t);
    h->scene.camera.rotation = close ? close_camera.rotation : shutter_blend3(sh.camera_rotation, close_camera.rotation, t);
  }
  for (uint32_t i : sh.moved_instances) {
    lum::HostInstance& inst = h->scene.instances[i];
    const HostShutter::Pose &a = sh.instances[i], &b = close_instances[i];
    inst.translation = close ? b.position : shutter_blend3(a.position, b.position, t);
    inst.rotation = close ? b.rotation : shutter_blend3(a.rotation, b.rotation, t);
    inst.scale = close ? b.scale : shutter_blend3(a.scale, b.scale, t);
  }
  const uint32_t encode = sh.slice_dirty & (LUMC_DIRTY_CONSTANTS | LUMC_DIRTY_INSTANCE_TRANSFORMS);
  if (encode) {
    const std::string err = lum::update_device_scene(h->scene, h->device_scene.bluenoise, encode, &h->device_scene);
    if (!err.empty()) { h->log.push_back(err); std::fprintf(stderr, "[luminary_amd] %s\n", err.c_str()); return 1; }
  }
  if (sh.slice_dirty == LUMC_DIRTY_MESH_SHUTTER && sh.meshes.empty()) return 0;  // nothing moved: the devices hold this scene
  const bool refits_lights = h->light_refit && (sh.slice_dirty & LUMC_DIRTY_LIGHT_POSITIONS);
  if (refits_lights && !sh.moved_instances.empty()) lum::refresh_light_refit_transforms(h->scene, &h->device_scene.light_refit_plan);
  for (LumContext* core : cores) {
    const auto& lt = h->device_scene.light_refit_plan.transforms;
    if (refits_lights && !sh.moved_instances.empty() && !lt.empty() && lumc_light_refit_transforms(core, lt.data(), (uint32_t) lt.size())) return 1;
    if (lumc_shutter_time(core, t) || lumc_scene_update(core, &h->device_scene.view, sh.slice_dirty)) { std::fprintf(stderr, "[luminary_amd] %s\n", lumc_last_error(core)); return 1; }
    if (set_camera(h, core)) return 1;
    if (refits_lights && lumc_light_refit_needs_rebuild(core)) { *rebuild = true; return 1; }
  }
  return 0;
}

LuminaryResult render_shutter_locked(LuminaryHost* h, uint32_t slices, uint32_t samples_per_slice, uint32_t samples_per_pass) {
  HostShutter& sh = h->shutter;
  if (slices == 0 || slices > 1024) return shutter_refuse(h, "slices is 1 ... 1024", false);
  if (samples_per_slice == 0) return shutter_refuse(h, "samples_per_slice is at least 1", false);
  if (h->scene.settings.enable_adaptive_sampling) return shutter_refuse(h, "adaptive sampling does not run under a shutter (settings.enable_adaptive_sampling)", false);
  if (!sh.open && !sh.keyed) return shutter_refuse(h, "no open key (luminary_ext_shutter_open)", false);
  history_drop(h, "a shutter render");
  const auto clock = [] { return std::chrono::steady_clock::now(); };
  const auto since = [&](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(clock() - t0).count(); };
  double seconds_update = 0.0, seconds_render = 0.0;
  std::vector<LumContext*> cores;
  const auto t_keys = clock();
  if (sh.open) {
    if (!sh.other.empty()) return shutter_refuse(h, sh.other + " changed since the shutter opened: only moved vertices, poses, weights, instance transforms and the camera's pos and rotation are blended", true);
    const uint32_t blended = LUMC_DIRTY_CONSTANTS | LUMC_DIRTY_MESH_POSITIONS | LUMC_DIRTY_MESH_SKIN | LUMC_DIRTY_INSTANCE_TRANSFORMS | LUMC_DIRTY_LIGHT_POSITIONS;
    const uint32_t bad = sh.edits & ~(blended | LUMC_DIRTY_LIGHTS);
    if (bad) {
      std::string what;
      const std::pair<uint32_t, const char*> names[] = {{LUMC_DIRTY_MATERIALS, "materials"}, {LUMC_DIRTY_INSTANCES, "the instance list"}, {LUMC_DIRTY_MESHES, "the mesh list"},
                                                        {LUMC_DIRTY_TEXTURES, "textures"}, {LUMC_DIRTY_PARTICLES, "particles"}};
      for (const auto& n : names) if (bad & n.first) what += (what.empty() ? "" : ", ") + std::string(n.second);
      return shutter_refuse(h, what + " changed since the shutter opened: only moved vertices, poses, weights, instance transforms and the camera's pos and rotation are blended", true);
    }
    if (sh.emitter_needs_refit)
      return shutter_refuse(h, "an emitter moved and the light tree would have to be built again per slice (LUMC_DIRTY_LIGHTS): luminary_ext_set_light_refit(host, 1, ...) before the shutter opens lets the devices refit it", true);
    if (sh.edits & LUMC_DIRTY_LIGHTS)
      return shutter_refuse(h, "a rebuild of the light tree is pending (LUMC_DIRTY_LIGHTS; luminary_ext_set_light_refit was switched, or a binding changed) since the shutter opened", true);
    if (!sh.synced || h->scene.instances.size() != sh.instances.size()) {
      shutter_cancel(h);
      std::fprintf(stderr, "[luminary_amd] luminary_ext_render_shutter: the devices did not take the open key\n");
      return LUMINARY_ERROR_CUDA;
    }
    sh.camera_moved = !same_vec(h->scene.camera.pos, sh.camera_pos) || !same_vec(h->scene.camera.rotation, sh.camera_rotation);
    sh.moved_instances.clear();
    for (uint32_t i = 0; i < h->scene.instances.size(); i++) {
      const lum::HostInstance& inst = h->scene.instances[i];
      if (!same_vec(inst.translation, sh.instances[i].position) || !same_vec(inst.rotation, sh.instances[i].rotation) || !same_vec(inst.scale, sh.instances[i].scale)) sh.moved_instances.push_back(i);
    }
    sh.slice_dirty = LUMC_DIRTY_MESH_SHUTTER | (sh.camera_moved ? LUMC_DIRTY_CONSTANTS : 0u) | (sh.moved_instances.empty() ? 0u : LUMC_DIRTY_INSTANCE_TRANSFORMS) |
                     (sh.edits & LUMC_DIRTY_LIGHT_POSITIONS);
    std::sort(sh.meshes.begin(), sh.meshes.end());
    auto fail = [&](LumContext* c) { std::fprintf(stderr, "[luminary_amd] %s\n", lumc_last_error(c)); shutter_cancel(h); return LUMINARY_ERROR_CUDA; };
    // 1. the open keys, from the vertices the devices hold
    for (LuminaryHost::DeviceSlot* slot : enabled_slots(h)) { LumContext* c = slot == &h->devices[h->main_slot] ? h->core : slot->core; if (c) cores.push_back(c); }
    if (cores.empty() && h->core) cores.push_back(h->core);
    for (LumContext* c : cores)
      for (uint32_t m : sh.meshes) if (lumc_mesh_shutter_key(c, m, 0)) return fail(c);
    // 2. the ordinary update: the devices hold the close key (the accumulation starts over exactly when something was edited)
    LuminaryResult r = render_samples_locked(h, nullptr, 0, h->accumulated_samples, 0, 1);
    if (!r) r = ensure_partition_cores(h, &cores);
    if (r) { shutter_cancel(h); return r; }
    // 3. the close keys
    for (LumContext* c : cores)
      for (uint32_t m : sh.meshes) if (lumc_mesh_shutter_key(c, m, 1)) return fail(c);
    sh.open = false; sh.keyed = true; sh.edits = 0;
  }
  else {
    LuminaryResult r = render_samples_locked(h, nullptr, 0, h->accumulated_samples, 0, 1);
    if (!r) r = ensure_partition_cores(h, &cores);
    if (r) return r;
  }
  seconds_update += since(t_keys);
  // 4. the slices
  const LuminaryCamera close_camera = h->scene.camera;
  std::vector<HostShutter::Pose> close_instances(h->scene.instances.size());
  for (size_t i = 0; i < close_instances.size(); i++) close_instances[i] = {h->scene.instances[i].translation, h->scene.instances[i].rotation, h->scene.instances[i].scale};
  const uint32_t first = h->accumulated_samples;
  h->handoff_preview = false;
  bool rebuild = false, failed = false;
  LumContext* failed_core = nullptr;
  for (uint32_t k = 0; k < slices && !failed; k++) {
    const float t = (float) (2 * k + 1) / (float) (2 * slices);
    const auto t_update = clock();
    failed = shutter_apply_time(h, cores, t, false, close_camera, close_instances, &rebuild) != 0;
    seconds_update += since(t_update);
    if (failed) break;
    const auto t_render = clock();
    // every device gets its kernels enqueued before the first one is waited for: the GPUs run side by side
    for (LumContext* c : cores)
      if (!failed && lumc_render(c, first + k * samples_per_slice, samples_per_slice, samples_per_pass, nullptr, nullptr, nullptr)) { failed = true; failed_core = c; }
    for (LumContext* c : cores)
      if (!failed && lumc_synchronize(c)) { failed = true; failed_core = c; }
    const double dt = since(t_render);
    seconds_render += dt; h->render_seconds += dt; h->last_sample_ms = 1e3 * dt / samples_per_slice;
  }
  // 5. time 1 and the close view once more: host and devices agree on the close key
  const auto t_close = clock();
  bool rebuild_close = false;
  if (!failed) failed = shutter_apply_time(h, cores, 1.0f, true, close_camera, close_instances, &rebuild_close) != 0;
  seconds_update += since(t_close);
  if (failed) {  // the host's scene is the close key again; every device takes it whole, and the accumulation starts over
    if (failed_core) std::fprintf(stderr, "[luminary_amd] %s\n", lumc_last_error(failed_core));
    h->scene.camera.pos = close_camera.pos; h->scene.camera.rotation = close_camera.rotation;
    for (uint32_t i : sh.moved_instances) { h->scene.instances[i].translation = close_instances[i].position; h->scene.instances[i].rotation = close_instances[i].rotation; h->scene.instances[i].scale = close_instances[i].scale; }
    shutter_cancel(h);
    invalidate(h);
    if (rebuild || rebuild_close) {
      h->log.push_back("luminary_ext_render_shutter: a slice's light refit asked for a rebuild of the light tree (lumc_light_refit_needs_rebuild); the next render rebuilds it at the close key and the accumulation restarts");
      std::fprintf(stderr, "[luminary_amd] %s\n", h->log.back().c_str());
      return LUMINARY_ERROR_API_EXCEPTION;
    }
    return LUMINARY_ERROR_CUDA;
  }
  h->accumulated_samples += slices * samples_per_slice;
  h->guides_valid = false;
  LuminaryShutterStats& st = sh.stats;
  st.renders++; st.slices += slices;
  st.last_moved_meshes = (uint32_t) sh.meshes.size(); st.last_moved_instances = (uint32_t) sh.moved_instances.size(); st.last_camera_moved = sh.camera_moved ? 1u : 0u; st.last_slices = slices;
  st.seconds_update = seconds_update; st.seconds_render = seconds_render;
  return produce_outputs(h);
}
}  // namespace

LuminaryResult luminary_ext_shutter_open(LuminaryHost* host) {
  CHECK_NULL(host);
  ApiLock lock(host);
  shutter_cancel(host);
  if (const LuminaryResult r = ensure_device_scene(host)) return r;
  host->handoff_preview = false;
  // what a render does before its first pass: every enabled slot takes the scene, the pixels are dealt
  std::vector<LumContext*> cores;
  const LuminaryResult r = host->scene.settings.enable_adaptive_sampling ? ensure_partition_cores(host, &cores)  // (luminary_ext_render_shutter refuses adaptive sampling)
                                                                         : render_samples_locked(host, nullptr, 0, host->accumulated_samples, 0, 1);
  if (r && host->core) return r;  // (no usable device at all: luminary_ext_render_shutter reports it)
  HostShutter& sh = host->shutter;
  sh.open = true; sh.synced = r == LUMINARY_SUCCESS;
  sh.camera_pos = host->scene.camera.pos; sh.camera_rotation = host->scene.camera.rotation;
  sh.instances.resize(host->scene.instances.size());
  for (size_t i = 0; i < sh.instances.size(); i++) sh.instances[i] = {host->scene.instances[i].translation, host->scene.instances[i].rotation, host->scene.instances[i].scale};
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_shutter_cancel(LuminaryHost* host) {
  CHECK_NULL(host);
  ApiLock lock(host);
  shutter_cancel(host);
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_render_shutter(LuminaryHost* host, uint32_t slices, uint32_t samples_per_slice, uint32_t samples_per_pass) {
  CHECK_NULL(host);
  ApiLock lock(host);
  return render_shutter_locked(host, slices, samples_per_slice, samples_per_pass);
}
LuminaryResult luminary_ext_get_shutter_stats(LuminaryHost* host, LuminaryShutterStats* out) {
  CHECK_NULL(host); CHECK_NULL(out);
  ApiLock lock(host);
  *out = host->shutter.stats;
  return LUMINARY_SUCCESS;
}
// The frame's first sample as the undersampling preview: every iteration renders one pixel per block, then the outputs are produced
// from the coarse image; the last iteration completes sample 0 of every pixel. Returns through *ran whether the preview applied.
static LuminaryResult render_first_sample_as_preview(LuminaryHost* host, bool* ran) {
  *ran = false;
  const std::vector<PreviewState> schedule = preview_schedule(host);
  if (schedule.empty() || host->accumulated_samples != 0 || !host->pixels_all) return LUMINARY_SUCCESS;
  for (size_t k = 0; k < schedule.size(); k++) {
    const auto t0 = std::chrono::steady_clock::now();
    if (lumc_render_undersampled(host->core, schedule[k].stage, schedule[k].iteration, nullptr) || lumc_synchronize(host->core)) {
      std::fprintf(stderr, "[luminary_amd] %s\n", lumc_last_error(host->core));
      return LUMINARY_ERROR_CUDA;
    }
    { const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); host->render_seconds += dt; host->last_sample_ms = 1e3 * dt; }
    if (k + 1 == schedule.size()) host->accumulated_samples = 1;  // device_renderer_finish_iteration counts the sample with the last iteration
    const LuminaryResult r = produce_outputs(host, schedule[k]);
    if (r) return r;
  }
  *ran = true;
  return LUMINARY_SUCCESS;
}

namespace {
// luminary_ext_render with the host's mutex held by the caller (the render worker and the API call share it): the first sample id of the
// allocation is read under the same lock the passes run under.
LuminaryResult render_locked(LuminaryHost* host, uint32_t num_samples, uint32_t samples_per_pass) {
  shutter_cancel(host);  // any other render call ends the shutter
  const LuminaryRendererSettings settings = host->scene.settings;
  if (!settings.enable_adaptive_sampling) {
    uint32_t first = host->pixels_all && !host->adaptive_active ? host->accumulated_samples : 0;
    if (first == 0 && num_samples > 0) {  // a new accumulation: its first sample may be due as the undersampling preview
      const LuminaryResult r = ensure_core(host);
      if (r) return r;
      if (!preview_schedule(host).empty()) {
        lumc_use_assembled_frame(host->core, 0);
        if (lumc_set_pixels(host->core, nullptr, 0)) return LUMINARY_ERROR_CUDA;
        host->partition_n = 1;
        host->adaptive_active = false;
        host->pixels_all = true;
        host->num_pixels = host->device_scene.view.width * host->device_scene.view.height;
        host->accumulated_samples = 0;
    host->guides_valid = false;
        host->render_seconds = 0.0;
        bool ran = false;
        const LuminaryResult rp = render_first_sample_as_preview(host, &ran);
        if (rp) return rp;
        if (ran) { first = 1; num_samples--; host->handoff_preview = enabled_slots(host).size() > 1; }
      }
    }
    if (num_samples == 0 && !host->handoff_preview) return LUMINARY_SUCCESS;
    return render_samples_locked(host, nullptr, 0, first, num_samples, samples_per_pass);
  }
  // Adaptive sampling over the enabled devices: the reference's main device computes the rates for all devices (device_adaptive_sampler.c:60-74,
  // :205-213; device_manager.c:452-469). Here every device owns the 4x4 blocks of its 32x32 tiles (lumc_adaptive_set_partition), renders their
  // tasks and, when a stage is due, contributes their variances to ONE all-reduce of 4 bytes per block (lumc_adaptive_exchange_all), after which every
  // device derives the same rates: rates, variances and frame equal the single-device run bit for bit.
  std::vector<LumContext*> cores;
  LuminaryResult r = ensure_partition_cores(host, &cores);
  if (r) return r;
  const uint32_t n = (uint32_t) cores.size();
  auto fail = [&](LumContext* c) { std::fprintf(stderr, "[luminary_amd] %s\n", lumc_last_error(c)); return LUMINARY_ERROR_CUDA; };
  if (!host->adaptive_active || host->partition_n != n) {
    const LumDeviceSceneView& v = host->device_scene.view;
    history_drop(host, "adaptive sampling drives the accumulation");
    lumc_use_assembled_frame(host->core, 0);
    LumAdaptiveParams ap;
    std::memset(&ap, 0, sizeof(ap));
    ap.max_sampling_rate = settings.adaptive_sampling_max_sampling_rate;
    ap.avg_sampling_rate = settings.adaptive_sampling_avg_sampling_rate;
    ap.update_interval = settings.adaptive_sampling_update_interval;
    ap.tone = output_params(host, v.width, v.height);
    ap.exposure = settings.adaptive_sampling_exposure_aware ? ap.tone.exposure : 0.0f;
    const uint32_t blocks_x = (v.width + 3) / 4, blocks_y = (v.height + 3) / 4, tiles_x = (v.width + 31) / 32;
    std::vector<uint8_t> mask((size_t) blocks_x * blocks_y);
    for (uint32_t k = 0; k < n; k++) {
      if (lumc_set_pixels(cores[k], nullptr, 0) || lumc_adaptive_begin(cores[k], &ap)) return fail(cores[k]);
      if (n > 1) {  // the blocks of a tile belong to the tile's device, like the pixels of a uniform tiled render (lumc_tile_owner)
        for (uint32_t by = 0; by < blocks_y; by++)
          for (uint32_t bx = 0; bx < blocks_x; bx++) mask[(size_t) by * blocks_x + bx] = (lumc_tile_owner(bx / 8, by / 8, tiles_x, n) == k) ? 1 : 0;
        if (lumc_adaptive_set_partition(cores[k], mask.data())) return fail(cores[k]);
      }
    }
    if (n > 1 && !host->comm_ready) {
      if (lumc_comm_init_all(cores.data(), (int) n) == 0) host->comm_ready = true;
      else std::fprintf(stderr, "[luminary_amd] no RCCL communicator (%s): block variances and frames go through the host / peer copies\n", lumc_last_error(cores[0]));
    }
    host->partition_n = n;
    host->pixels_all = true;
    host->num_pixels = v.width * v.height;
    host->accumulated_samples = 0;
    host->guides_valid = false;
    host->render_seconds = 0.0;
    host->handoff_preview = false;
    host->adaptive_active = true;
  }
  uint32_t done = 0;
  if (host->accumulated_samples == 0 && num_samples > 0) {  // execution 0 of stage 0 as the undersampling preview, when one is due
    bool ran = false;
    const uint32_t partition = host->partition_n;
    host->partition_n = 1;  // the preview's images come from the main device's own accumulators
    r = render_first_sample_as_preview(host, &ran);
    host->partition_n = partition;
    if (r) return r;
    if (ran) {
      if (n > 1) {  // every device takes over the first sample of the blocks it owns
        if (lumc_frame_assemble(host->core, host->num_pixels, 0, nullptr, nullptr)) return fail(host->core);
        for (uint32_t k = 0; k < n; k++) if (lumc_accumulators_from_frame(cores[k], host->core)) return fail(cores[k]);
      }
      for (uint32_t k = 0; k < n; k++) if (lumc_adaptive_note_first_sample(cores[k], nullptr)) return fail(cores[k]);
      done = 1;
    }
  }
  auto executions_done = [&](LumContext* c, uint32_t* pending) {
    LumAdaptiveInfo info;
    std::memset(&info, 0, sizeof(info));
    lumc_adaptive_info(c, &info);
    uint32_t total = 0;
    for (uint32_t e : info.executions) total += e;
    if (pending) *pending = info.build_pending;
    return total;
  };
  // a stage may be due right away (the preview was its last execution)
  { uint32_t pending = 0; executions_done(cores[0], &pending); if (n > 1 && pending && lumc_adaptive_exchange_all(cores.data(), (int) n)) return fail(cores[0]); }
  while (done < num_samples) {
    uint32_t chunk = num_samples - done;
    for (const LuminaryOutputRequestProperties& req : host->outputs.pending_requests())
      if (req.sample_count > host->accumulated_samples && req.sample_count - host->accumulated_samples < chunk) chunk = req.sample_count - host->accumulated_samples;
    const auto t0 = std::chrono::steady_clock::now();
    uint32_t left = chunk;
    while (left > 0) {  // a partitioned context stops where a stage is due: exchange, go on
      const uint32_t before = executions_done(cores[0], nullptr);
      for (uint32_t k = 0; k < n; k++) if (lumc_adaptive_render(cores[k], left, nullptr)) return fail(cores[k]);
      for (uint32_t k = 0; k < n; k++) if (lumc_synchronize(cores[k])) return fail(cores[k]);
      uint32_t pending = 0;
      const uint32_t ran_now = executions_done(cores[0], &pending) - before;
      if (pending && lumc_adaptive_exchange_all(cores.data(), (int) n)) return fail(cores[0]);
      if (ran_now == 0 && !pending) { std::fprintf(stderr, "[luminary_amd] adaptive rendering made no progress\n"); return LUMINARY_ERROR_API_EXCEPTION; }
      left -= std::min(left, ran_now);
    }
    { const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); host->render_seconds += dt; host->last_sample_ms = 1e3 * dt / (chunk ? chunk : 1u); }
    host->accumulated_samples += chunk;
    done += chunk;
    r = produce_outputs(host);
    if (r) return r;
  }
  return LUMINARY_SUCCESS;
}
}  // namespace

// The reference's render loop for `num_samples` more sample allocations of the whole frame (device_renderer.c:488-575): with
// settings.enable_adaptive_sampling the stage schedule of the adaptive sampler, otherwise one sample id per pixel and allocation.
LuminaryResult luminary_ext_render(LuminaryHost* host, uint32_t num_samples) {
  CHECK_NULL(host);
  ApiLock lock(host);
  return render_locked(host, num_samples, 8);
}
LuminaryResult luminary_ext_get_accumulators(LuminaryHost* host, float* first_moment, float* second_moment, uint32_t* num_pixels) {
  CHECK_NULL(host);
  ApiLock lock(host);
  if (num_pixels) *num_pixels = host->num_pixels;
  if (!host->core || host->num_pixels == 0) return LUMINARY_ERROR_API_EXCEPTION;
  if (host->partition_n > 1) {  // tiled render: the assembled frame
    if (!(first_moment || second_moment)) return LUMINARY_SUCCESS;
    const LuminaryResult ra = assemble_partition(host);
    if (ra) return ra;
    return lumc_frame_download(host->core, host->num_pixels, first_moment, second_moment) ? LUMINARY_ERROR_CUDA : LUMINARY_SUCCESS;
  }
  if ((first_moment || second_moment) && lumc_download_accumulators(host->core, first_moment, second_moment)) return LUMINARY_ERROR_CUDA;
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_get_radiance(LuminaryHost* host, float* rgb, uint32_t* sample_count, uint32_t width, uint32_t height) {
  CHECK_NULL(host); CHECK_NULL(rgb);
  ApiLock lock(host);
  if (!host->core || !host->pixels_all || host->num_pixels == 0) return LUMINARY_ERROR_API_EXCEPTION;
  const LumDeviceSceneView& v = host->device_scene.view;
  if (width != v.width || height != v.height) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  if (host->adaptive_active) {  // every pixel has its own sample count: the beauty result image is the radiance
    if (host->partition_n > 1) { const LuminaryResult ra = assemble_partition(host); if (ra) return ra; }
    std::vector<float> planes(3 * (size_t) host->num_pixels);
    if (lumc_generate_result_host(host->core, 0, 0, 0, 1.0f, nullptr, planes.data())) return LUMINARY_ERROR_CUDA;
    for (size_t p = 0; p < host->num_pixels; p++)
      for (int c = 0; c < 3; c++) rgb[3 * p + c] = planes[(size_t) c * host->num_pixels + p];
    if (sample_count) *sample_count = host->accumulated_samples;
    return LUMINARY_SUCCESS;
  }
  std::vector<float> fm(3 * (size_t) host->num_pixels);
  if (host->partition_n > 1) {
    const LuminaryResult ra = assemble_partition(host);
    if (ra) return ra;
    if (lumc_frame_download(host->core, host->num_pixels, fm.data(), nullptr)) return LUMINARY_ERROR_CUDA;
  }
  else if (lumc_download_accumulators(host->core, fm.data(), nullptr)) return LUMINARY_ERROR_CUDA;
  const float norm = host->accumulated_samples ? 1.0f / host->accumulated_samples : 0.0f;  // accumulation.cuh:149-153
  for (size_t p = 0; p < host->num_pixels; p++)
    for (int c = 0; c < 3; c++) rgb[3 * p + c] = fm[(size_t) c * host->num_pixels + p] * norm;
  if (sample_count) *sample_count = host->accumulated_samples;
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_set_denoiser(LuminaryHost* host, const LuminaryDenoiserSettings* settings) {
  CHECK_NULL(host); CHECK_NULL(settings);
  if (settings->guide_samples == 0 || settings->guide_samples > 1024 || settings->iterations > 6 || !(settings->sigma_luminance > 0.0f) || !(settings->sigma_normal >= 0.0f) ||
      !(settings->sigma_depth > 0.0f))
    return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  ApiLock lock(host);
  if (settings->guide_samples != host->denoiser.guide_samples) host->guides_valid = false;
  host->denoiser = *settings;  // changes how the accumulated frame is shown, like an output-only camera edit: the integration goes on
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_get_denoiser(LuminaryHost* host, LuminaryDenoiserSettings* settings) {
  CHECK_NULL(host); CHECK_NULL(settings);
  ApiLock lock(host);
  *settings = host->denoiser;
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_get_denoised(LuminaryHost* host, float* rgb, uint32_t width, uint32_t height) {
  CHECK_NULL(host); CHECK_NULL(rgb);
  ApiLock lock(host);
  if (!host->core || !host->pixels_all || host->num_pixels == 0 || host->accumulated_samples == 0) return LUMINARY_ERROR_API_EXCEPTION;
  const LumDeviceSceneView& v = host->device_scene.view;
  if (width != v.width || height != v.height) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  if (host->partition_n > 1) { const LuminaryResult ra = assemble_partition(host); if (ra) return ra; }
  if (lumc_generate_result(host->core, 0, 0, host->adaptive_active ? 0u : host->accumulated_samples, 1.0f, nullptr, nullptr, nullptr) || firefly_result(host) || denoise_result(host)) {  // (the outputs' chain up to bloom)
    std::fprintf(stderr, "[luminary_amd] %s\n", lumc_last_error(host->core));
    return LUMINARY_ERROR_CUDA;
  }
  std::vector<float> planes(3 * (size_t) host->num_pixels);
  if (lumc_download_result_image(host->core, planes.data())) return LUMINARY_ERROR_CUDA;
  for (size_t p = 0; p < host->num_pixels; p++)
    for (int c = 0; c < 3; c++) rgb[3 * p + c] = planes[(size_t) c * host->num_pixels + p];
  return LUMINARY_SUCCESS;
}
// ---- firefly rejection (include/luminary_amd.h LuminaryFireflySettings) ----
LuminaryResult luminary_ext_set_firefly_rejection(LuminaryHost* host, const LuminaryFireflySettings* settings) {
  CHECK_NULL(host); CHECK_NULL(settings);
  ApiLock lock(host);
  auto refuse = [&](const std::string& why) {
    host->log.push_back("luminary_ext_set_firefly_rejection: " + why);
    std::fprintf(stderr, "[luminary_amd] %s\n", host->log.back().c_str());
    return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  };
  if (settings->buckets < 4 || settings->buckets > 16) return refuse(std::to_string(settings->buckets) + " buckets (4 ... 16)");
  if (settings->enabled && enabled_slots(host).size() > 1) return refuse("the host renders on more than one device slot, and the gather of a tiled frame carries no bucket planes");
  const bool changed = settings->enabled != host->firefly.enabled || (settings->enabled && settings->buckets != host->firefly.buckets);
  host->firefly = *settings;
  if (changed) {  // the buckets must see every id: the integration restarts, and the render loop sets the pixel set up again
    invalidate(host, 0);
    host->num_pixels = 0;
  }
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_get_firefly_rejection(LuminaryHost* host, LuminaryFireflySettings* settings) {
  CHECK_NULL(host); CHECK_NULL(settings);
  ApiLock lock(host);
  *settings = host->firefly;
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_get_robust_radiance(LuminaryHost* host, float* rgb, uint32_t width, uint32_t height) {
  CHECK_NULL(host); CHECK_NULL(rgb);
  ApiLock lock(host);
  if (!host->core || !host->pixels_all || host->num_pixels == 0 || host->accumulated_samples == 0 || !host->core_firefly || host->partition_n > 1) return LUMINARY_ERROR_API_EXCEPTION;
  const LumDeviceSceneView& v = host->device_scene.view;
  if (width != v.width || height != v.height) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  if (lumc_generate_result(host->core, 0, 0, host->adaptive_active ? 0u : host->accumulated_samples, 1.0f, nullptr, nullptr, nullptr) || firefly_result(host)) {
    std::fprintf(stderr, "[luminary_amd] %s\n", lumc_last_error(host->core));
    return LUMINARY_ERROR_CUDA;
  }
  std::vector<float> planes(3 * (size_t) host->num_pixels);
  if (lumc_download_result_image(host->core, planes.data())) return LUMINARY_ERROR_CUDA;
  for (size_t p = 0; p < host->num_pixels; p++)
    for (int c = 0; c < 3; c++) rgb[3 * p + c] = planes[(size_t) c * host->num_pixels + p];
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_get_firefly_stats(LuminaryHost* host, LuminaryFireflyStats* out) {
  CHECK_NULL(host); CHECK_NULL(out);
  ApiLock lock(host);
  std::memset(out, 0, sizeof(*out));
  out->frames_resolved = host->firefly_resolved; out->frames_skipped = host->firefly_skipped;
  if (host->core && host->core_firefly) {
    LumFireflyStats st;
    if (lumc_firefly_stats(host->core, &st)) return LUMINARY_ERROR_CUDA;
    out->last_rewritten = st.last_rewritten; out->last_trimmed = st.last_trimmed; out->last_nonfinite = st.last_nonfinite;
    out->buckets = st.buckets; out->bytes = st.bytes;
  }
  return LUMINARY_SUCCESS;
}
// ---- image history (include/luminary_amd.h LuminaryHistorySettings; include/lum_core.h lumc_set_history) ----
LuminaryResult luminary_ext_set_history(LuminaryHost* host, const LuminaryHistorySettings* settings) {
  CHECK_NULL(host); CHECK_NULL(settings);
  ApiLock lock(host);
  auto refuse = [&](const std::string& why) {
    host->log.push_back("luminary_ext_set_history: " + why);
    std::fprintf(stderr, "[luminary_amd] %s\n", host->log.back().c_str());
    return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  };
  if (!(settings->max_history > 0.0f) || !std::isfinite(settings->max_history)) return refuse("max_history must be positive and finite");
  if (!(settings->depth_tolerance >= 0.0f) || !std::isfinite(settings->depth_tolerance)) return refuse("depth_tolerance must be >= 0 and finite");
  if (!(settings->normal_threshold >= -1.0f && settings->normal_threshold <= 1.0f)) return refuse("normal_threshold must lie in [-1, 1]");
  if (!(settings->clamp_sigma >= 0.0f) || !std::isfinite(settings->clamp_sigma)) return refuse("clamp_sigma must be >= 0 and finite");
  if (host->history.enabled && !settings->enabled) history_drop(host, "history was switched off");
  host->history = *settings;  // changes how the accumulated frame is shown, like the denoiser's settings: the integration goes on
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_get_history(LuminaryHost* host, LuminaryHistorySettings* settings) {
  CHECK_NULL(host); CHECK_NULL(settings);
  ApiLock lock(host);
  *settings = host->history;
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_get_history_image(LuminaryHost* host, float* rgb, float* weight, uint32_t width, uint32_t height) {
  CHECK_NULL(host);
  ApiLock lock(host);
  if (!host->history.enabled || !history_held(host)) {
    host->log.push_back(std::string("luminary_ext_get_history_image: no shown frame is held") + (host->history_last_drop.empty() ? "" : ": " + host->history_last_drop));
    return LUMINARY_ERROR_API_EXCEPTION;
  }
  LumHistoryKey key;
  if (lumc_history_key(host->core, &key, nullptr)) return LUMINARY_ERROR_API_EXCEPTION;
  if (width != key.width || height != key.height) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  const size_t n = (size_t) width * height;
  std::vector<float> planes(3 * n);
  if (lumc_download_history(host->core, rgb ? planes.data() : nullptr, weight, nullptr, nullptr)) return LUMINARY_ERROR_CUDA;
  if (rgb)
    for (size_t p = 0; p < n; p++)
      for (int c = 0; c < 3; c++) rgb[3 * p + c] = planes[(size_t) c * n + p];
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_get_history_stats(LuminaryHost* host, LuminaryHistoryStats* out) {
  CHECK_NULL(host); CHECK_NULL(out);
  ApiLock lock(host);
  std::memset(out, 0, sizeof(*out));
  out->frames_carried = host->history_carried; out->frames_dropped = host->history_dropped; out->frames_skipped = host->history_skipped;
  std::snprintf(out->last_drop, sizeof(out->last_drop), "%s", host->history_last_drop.c_str());
  if (host->core) {
    LumHistoryStats st;
    if (lumc_history_stats(host->core, &st)) return LUMINARY_ERROR_CUDA;
    out->last_carried = st.last_carried; out->last_rejected = st.last_rejected; out->last_off = st.last_off;
    out->valid = (host->history.enabled && st.has_state) ? 1u : 0u;
    out->bytes = st.bytes;
    out->seconds = 1e-3 * (st.carry_ms + st.blend_ms);  // (the motion form's launches: luminary_ext_get_history_motion_stats)
  }
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_set_history_motion(LuminaryHost* host, const LuminaryHistoryMotionSettings* settings) {
  CHECK_NULL(host); CHECK_NULL(settings);
  ApiLock lock(host);
  if (!(settings->motion_max_history > 0.0f) || !std::isfinite(settings->motion_max_history)) {
    host->log.push_back("luminary_ext_set_history_motion: motion_max_history must be positive and finite");
    std::fprintf(stderr, "[luminary_amd] %s\n", host->log.back().c_str());
    return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  }
  // A carry granted for a move of instances needs the motion form: without it the camera form would leave the mover's old image where it was.
  if (host->history_motion.enabled && !settings->enabled && host->history_carry_due && host->history_carry_instances) history_drop(host, "the history's motion was switched off");
  host->history_motion = *settings;  // (how the next restart is taken and the next frame shown: the integration goes on, nothing is dropped)
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_get_history_motion(LuminaryHost* host, LuminaryHistoryMotionSettings* settings) {
  CHECK_NULL(host); CHECK_NULL(settings);
  ApiLock lock(host);
  *settings = host->history_motion;
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_get_history_motion_stats(LuminaryHost* host, LuminaryHistoryMotionStats* out) {
  CHECK_NULL(host); CHECK_NULL(out);
  ApiLock lock(host);
  std::memset(out, 0, sizeof(*out));
  if (!host->core) return LUMINARY_SUCCESS;
  LumHistoryMotionStats st;
  if (lumc_history_motion_stats(host->core, &st)) return LUMINARY_ERROR_CUDA;
  out->frames_carried = st.motion_carries; out->bytes = st.bytes;
  out->instances_moved = st.instances_moved; out->instances_same = st.instances_same; out->instances_void = st.instances_void;
  out->last_moved_pixels = st.last_moved_pixels; out->last_moved_carried = st.last_moved_carried;
  out->valid = (history_motion_on(host) && st.has_snapshot) ? 1u : 0u;
  out->owner_seconds = 1e-3 * st.owner_ms; out->motion_seconds = 1e-3 * st.motion_ms; out->reproject_seconds = 1e-3 * st.reproject_ms;
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_get_history_owner(LuminaryHost* host, uint32_t* shown_owner, uint32_t* current_owner, uint32_t width, uint32_t height) {
  CHECK_NULL(host);
  ApiLock lock(host);
  if (!history_motion_on(host) || !host->core) return LUMINARY_ERROR_API_EXCEPTION;
  LumHistoryKey key;
  if (lumc_history_key(host->core, nullptr, &key)) return LUMINARY_ERROR_API_EXCEPTION;
  if (width != key.width || height != key.height) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  if (lumc_download_history_owner(host->core, shown_owner, current_owner)) {
    host->log.push_back(std::string("luminary_ext_get_history_owner: ") + lumc_last_error(host->core));
    return LUMINARY_ERROR_API_EXCEPTION;
  }
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_get_history_transforms(LuminaryHost* host, float* shown_transforms, float* current_transforms, uint32_t instances, uint32_t* shown_instances) {
  CHECK_NULL(host);
  ApiLock lock(host);
  if (!history_motion_on(host) || !host->core) return LUMINARY_ERROR_API_EXCEPTION;
  uint32_t held = 0;
  if (lumc_download_history_transforms(host->core, nullptr, nullptr, &held)) return LUMINARY_ERROR_API_EXCEPTION;
  if (shown_instances) *shown_instances = held;
  if ((shown_transforms && held != instances) || (current_transforms && host->device_scene.view.num_instances != instances)) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  if (lumc_download_history_transforms(host->core, shown_transforms, current_transforms, nullptr)) {
    host->log.push_back(std::string("luminary_ext_get_history_transforms: ") + lumc_last_error(host->core));
    return LUMINARY_ERROR_API_EXCEPTION;
  }
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_camera_change_carries_history(const LuminaryCamera* input, const LuminaryCamera* old, bool* carries) {
  CHECK_NULL(input); CHECK_NULL(old); CHECK_NULL(carries);
  *carries = camera_change_carries(*input, *old);
  return LUMINARY_SUCCESS;
}
// ---- ID mattes (include/luminary_amd.h luminary_ext_render_mattes; include/lum_core.h lumc_render_first_hits) ----
namespace {
LuminaryResult matte_refuse(LuminaryHost* host, const char* fn, const std::string& why, LuminaryResult code) {
  host->log.push_back(std::string(fn) + ": " + why);
  std::fprintf(stderr, "[luminary_amd] %s\n", host->log.back().c_str());
  return code;
}
bool one_matte_layer(uint32_t layer) { return layer == LUMINARY_MATTE_LAYER_INSTANCE || layer == LUMINARY_MATTE_LAYER_MATERIAL; }
// the main context holds mattes of the scene as the host has it now
bool mattes_current(const LuminaryHost* host) { return host->core && host->mattes_valid && host->core_scene_valid && lumc_has_mattes(host->core); }
}  // namespace

LuminaryResult luminary_ext_render_mattes(LuminaryHost* host, uint32_t samples, uint32_t layers) {
  CHECK_NULL(host);
  if (samples > 1024 || layers == 0 || (layers & ~(uint32_t) (LUMINARY_MATTE_LAYER_INSTANCE | LUMINARY_MATTE_LAYER_MATERIAL))) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  ApiLock lock(host);
  host->mattes_valid = false;
  if (const LuminaryResult r = ensure_core(host)) return r;
  // The denoiser's guides come from the same first hits: where they are due and want the same sample ids, one set of rays makes both. With another count of
  // guide samples they are rendered on their own, so that the guides are what luminary_ext_set_denoiser asked for.
  const bool guides_due = host->denoiser.enabled && (!host->guides_valid || !lumc_has_guides(host->core));
  const bool shared = guides_due && (samples ? samples : 4u) == host->denoiser.guide_samples;
  LumHistoryMotionParams mp;  // (the guides of an accumulation come with the owner plane while the history's motion is on: render_guides)
  mp.enabled = history_motion_on(host) ? 1u : 0u; mp.motion_max_history = host->history_motion.motion_max_history;
  const uint32_t with_guides = shared ? (uint32_t) LUMC_FIRST_HIT_GUIDES | (mp.enabled ? (uint32_t) LUMC_FIRST_HIT_OWNER : 0u) : 0u;
  if ((shared && lumc_set_history_motion(host->core, &mp)) || lumc_render_first_hits(host->core, samples, LUMC_FIRST_HIT_MATTES | with_guides, layers, nullptr) ||
      (guides_due && !shared && render_guides(host))) {
    std::fprintf(stderr, "[luminary_amd] %s\n", lumc_last_error(host->core));
    return LUMINARY_ERROR_CUDA;
  }
  if (guides_due) host->guides_valid = true;
  host->mattes_valid = true;
  host->matte_renders++;
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_get_matte(LuminaryHost* host, uint32_t layer, uint32_t ranks, uint32_t* ids, float* coverage, uint32_t width, uint32_t height) {
  CHECK_NULL(host);
  if (!ids && !coverage) return LUMINARY_ERROR_ARGUMENT_NULL;
  if (!one_matte_layer(layer) || ranks == 0 || ranks > 8) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  ApiLock lock(host);
  if (!mattes_current(host)) return matte_refuse(host, "luminary_ext_get_matte", "no mattes of the scene as it is (luminary_ext_render_mattes)", LUMINARY_ERROR_API_EXCEPTION);
  const LumDeviceSceneView& v = host->device_scene.view;
  if (width != v.width || height != v.height) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  if (lumc_download_mattes(host->core, layer, ranks, ids, coverage, nullptr, nullptr)) return matte_refuse(host, "luminary_ext_get_matte", lumc_last_error(host->core), LUMINARY_ERROR_API_EXCEPTION);
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_get_matte_mask(LuminaryHost* host, uint32_t layer, const uint32_t* ids, uint32_t count, float* mask, uint32_t width, uint32_t height) {
  CHECK_NULL(host); CHECK_NULL(mask);
  if (count && !ids) return LUMINARY_ERROR_ARGUMENT_NULL;
  if (!one_matte_layer(layer) || count > 16) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  ApiLock lock(host);
  if (!mattes_current(host)) return matte_refuse(host, "luminary_ext_get_matte_mask", "no mattes of the scene as it is (luminary_ext_render_mattes)", LUMINARY_ERROR_API_EXCEPTION);
  const LumDeviceSceneView& v = host->device_scene.view;
  if (width != v.width || height != v.height) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  if (lumc_matte_mask_host(host->core, layer, ids, count, mask)) return matte_refuse(host, "luminary_ext_get_matte_mask", lumc_last_error(host->core), LUMINARY_ERROR_API_EXCEPTION);
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_get_matte_stats(LuminaryHost* host, LuminaryMatteStats* out) {
  CHECK_NULL(host); CHECK_NULL(out);
  ApiLock lock(host);
  std::memset(out, 0, sizeof(*out));
  out->renders = host->matte_renders;
  if (host->core) {
    LumMatteStats st;
    if (lumc_matte_stats(host->core, &st)) return LUMINARY_ERROR_CUDA;
    out->bytes = st.bytes; out->layers = st.layers;
    if (mattes_current(host)) {
      out->valid = 1; out->samples = st.samples; out->seconds = st.seconds;
      out->dropped_pixels[0] = st.dropped_pixels[0]; out->dropped_pixels[1] = st.dropped_pixels[1];
    }
  }
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_get_first_hit_guides(LuminaryHost* host, float* albedo, float* normal, float* depth, uint32_t width, uint32_t height) {
  CHECK_NULL(host);
  if (!albedo && !normal && !depth) return LUMINARY_ERROR_ARGUMENT_NULL;
  ApiLock lock(host);
  if (const LuminaryResult r = ensure_core(host)) return r;
  const LumDeviceSceneView& v = host->device_scene.view;
  if (width != v.width || height != v.height) return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  if (!host->guides_valid || !lumc_has_guides(host->core)) {  // as the denoiser makes them (denoise_result)
    if (render_guides(host)) { std::fprintf(stderr, "[luminary_amd] %s\n", lumc_last_error(host->core)); return LUMINARY_ERROR_CUDA; }
    host->guides_valid = true;
  }
  if (lumc_download_guides(host->core, albedo, normal, depth)) return LUMINARY_ERROR_CUDA;
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_get_ray_counters(LuminaryHost* host, uint64_t out[8]) {
  CHECK_NULL(host); CHECK_NULL(out);
  if (!host->core) return LUMINARY_ERROR_API_EXCEPTION;
  ApiLock lock(host);
  uint64_t all[LUMC_CNT_COUNT] = {0};  // the core keeps more counters than this call returns
  if (lumc_counters(host->core, all)) return LUMINARY_ERROR_CUDA;
  if (host->partition_n > 1)  // rays of every device of the tiled render
    for (LuminaryHost::DeviceSlot* slot : enabled_slots(host)) {
      if (!slot->core || slot->core == host->core) continue;
      uint64_t c[LUMC_CNT_COUNT] = {0};
      if (lumc_counters(slot->core, c)) return LUMINARY_ERROR_CUDA;
      for (int k = 0; k < LUMC_CNT_COUNT; k++) all[k] += c[k];
    }
  for (int k = 0; k < 8; k++) out[k] = all[k];
  return LUMINARY_SUCCESS;
}
// host_math.c:6-21 as the instance transforms use it (exposed so that it can be checked against the reference's own function)
LuminaryResult luminary_ext_euler_to_quaternion(const float rotation[3], float quaternion[4]) {
  CHECK_NULL(rotation); CHECK_NULL(quaternion);
  LuminaryVec3 r; r.x = rotation[0]; r.y = rotation[1]; r.z = rotation[2];
  lum::euler_to_quaternion(r, quaternion);
  return LUMINARY_SUCCESS;
}
// path_extend + path_apply (path.c) as the loaders use it; exposed for the check against the reference
LuminaryResult luminary_ext_path_extend(const char* base_file, const char* name, char* out, size_t out_size) {
  CHECK_NULL(base_file); CHECK_NULL(name); CHECK_NULL(out);
  const std::string r = lum::extend_path(base_file, name);
  if (r.size() + 1 > out_size) return LUMINARY_ERROR_OUT_OF_MEMORY;
  std::memcpy(out, r.c_str(), r.size() + 1);
  return LUMINARY_SUCCESS;
}
// 0: renderer settings, 1: camera. Exposed so that the rule can be checked against the reference's *_check_for_dirty.
LuminaryResult luminary_ext_change_restarts_integration(int entity, const void* input, const void* old, bool* restarts) {
  CHECK_NULL(input); CHECK_NULL(old); CHECK_NULL(restarts);
  if (entity == 0) *restarts = settings_change_restarts(*(const LuminaryRendererSettings*) input, *(const LuminaryRendererSettings*) old);
  else if (entity == 1) *restarts = camera_change_restarts(*(const LuminaryCamera*) input, *(const LuminaryCamera*) old);
  else if (entity == 2) *restarts = lens_change_restarts(*(const LuminaryCameraLens*) input, *(const LuminaryCameraLens*) old);
  else return LUMINARY_ERROR_INVALID_API_ARGUMENT;
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_set_camera_lens(LuminaryHost* host, const LuminaryCameraLens* lens) {
  CHECK_NULL(host); CHECK_NULL(lens);
  const std::string e = lum::validate_camera_lens(*lens);
  if (!e.empty()) { std::fprintf(stderr, "[luminary_amd] %s\n", e.c_str()); return LUMINARY_ERROR_INVALID_API_ARGUMENT; }
  ApiLock lock(host);
  const bool restarts = host->scene.camera.use_physical_camera && lens_change_restarts(*lens, host->scene.lens);
  host->scene.lens = *lens;
  if (restarts) { shutter_note_other(host, "the lens"); host->history_cause = "the lens changed"; invalidate(host, LUMC_DIRTY_CONSTANTS); }
  return LUMINARY_SUCCESS;
}
LuminaryResult luminary_ext_get_camera_lens(LuminaryHost* host, LuminaryCameraLens* lens) {
  CHECK_NULL(host); CHECK_NULL(lens);
  ApiLock lock(host);
  *lens = host->scene.lens;
  return LUMINARY_SUCCESS;
}
void* luminary_ext_get_core_context(LuminaryHost* host) {
  if (!host) return nullptr;
  ApiLock lock(host);
  if (ensure_core(host)) return nullptr;
  return host->core;
}

}  // extern "C"
