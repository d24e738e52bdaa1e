// The host layer's context and the helpers its translation units share. Private to csrc/host: core.hip (the context, the work buffers, the render schedule, the
// adaptive sampler, the output chain, the firefly buckets' entry points and the ray queries, with the flavour-neutral kernels of kernels_shared.h), scene_device.hip (the scene on the device, with the
// kernels of kernels_scene.h), probes.hip (the truth probes' entry points), ray_sort.hip, multi_gpu.hip. The context owns its device memory through DeviceBuffer members (device_buffer.h): deleting it frees them.
// Its other pointers - DeviceScene, the work buffers' arrays (work_layout.h) - are views into those buffers. kernels.h is not included, so a unit that includes
// this header gets none of the flavoured kernels (their device symbols - the sampler's seed table, the phase counters - exist per translation unit).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdio>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../../include/lum_core.h"
#include "../device/dev_scene.h"
#include "../device/wavefront_table.h"
#include "bvh_build.h"
#include "bvh_refit.h"
#include "device_buffer.h"
#include "firefly.h"
#include "history.h"
#include "instance_update.h"
#include "light_refit.h"
#include "matte.h"
#include "mesh_deform.h"
#include "mesh_shutter.h"
#include "scene_arrays.h"
#include "work_layout.h"

using namespace lum;

typedef struct ncclComm* ncclComm_t;  // as rccl.h declares it; only multi_gpu.hip includes that header

// A mesh's bottom-level tree (node indices relative to the mesh, leaf ranges relative to its first triangle). The contexts of one process share them: a host
// with several devices hands every context the same meshes, the first one builds a mesh's tree, the others - and a later upload of the same mesh - take it
// from find_mesh_tree (below), and it is released with the last context that holds it.
struct MeshTree { Bvh4 bvh; bool built_on_gpu = false; };

// What a context keeps per mesh for LUMC_DIRTY_MESH_POSITIONS updates.
struct MeshRefit {
  RefitPlan plan;                  // the held tree's topology on the device, from the mesh's first refit until it is built again
  std::shared_ptr<MeshTree> own;   // the refitted tree (LumContext::mesh_bvh holds the same object): private, never in the process's tree cache
  uint64_t fit_hash[2] = {0, 0};   // of the vertices the held tree was built from or last fitted to (mesh_tree_key)
  double built_cost = 0.0;         // bvh4_cost of the tree as last built (0: not computed yet)
  bool stale = false;              // the mesh was refitted in the resident node array since: the host's nodes hold the boxes of earlier vertices (restore_stale_meshes)
  bool fit_to_pose = false;        // the held tree was last fitted to vertices k_deform_mesh wrote: no host vertices hash to that, fit_hash is not compared
};

struct LumContext {
  int device = 0;
  std::string error;
  const WavefrontKernels* wf = wavefront_kernels_fast();  // flavour of the wavefront kernels (lumc_set_flavour; LUM_FLAVOUR=exact|fast overrides the default)
  int camera = kCamThinLens;  // CameraKind of the camera-ray kernels (lumc_set_physical_camera)
  DeviceLens lens{};          // the physical camera's lens, an argument of those kernels
  SceneArrays arrays;  // the scene's device arrays by the part of it they belong to (lumc_scene_update frees and rebuilds a part at a time); `scene` views them
  // what a partial update needs again: the per-mesh trees (node indices relative to the mesh, leaf ranges relative to its first triangle) and boxes
  std::vector<std::shared_ptr<const MeshTree>> mesh_bvh;
  std::vector<Aabb> mesh_box;
  std::vector<MeshRefit> mesh_refit;         // by mesh, as long as mesh_bvh
  std::vector<uint32_t> mesh_tri_offset;     // the offsets the trees were built for: a LUMC_DIRTY_MESH_POSITIONS update must bring the same
  uint32_t refit_mode = 0;                   // lumc_set_mesh_refit
  float refit_max_cost_growth = 0.0f;
  LumMeshRefitStats refit_stats{};
  // LUMC_DIRTY_INSTANCE_TRANSFORMS updates (instance_update.hip; scene_device.hip instance_boxes, ensure_resident_layout, build_top_level)
  InstanceUpdate instance_update;            // the resident layout's bookkeeping and the device path's scratch
  std::vector<uint32_t> instance_mesh_ids;   // of the scene on the device: such an update must bring the same
  // what DeviceScene::traits is computed from (scene_device.hip scene_traits): the host's words of the parts an update may leave alone
  std::vector<uint16_t> tri_material;        // material id by scene triangle (update_mesh_arrays)
  std::vector<uint16_t> material_words;      // 16 per material, as uploaded (update_materials)
  std::vector<uint32_t> light_handles;       // instance, triangle per light (update_light_tree)
  bool light_tree_flat = true;               // the light tree has no nodes below its root: every root child is a light (update_light_tree)
  uint32_t instance_update_mode = 0;         // lumc_set_instance_update
  LumInstanceUpdateStats instance_stats{};
  // LUMC_DIRTY_MESH_POSITIONS updates in the resident node array (lumc_set_mesh_refit_in_place; bvh_refit.hip, scene_device.hip refit_in_place)
  uint32_t refit_in_place = 0;
  ResidentRefit resident_refit;              // the layout's slot maps, the per-mesh slot lists and the scratch; dropped with the layout
  uint32_t stale_meshes = 0;                 // meshes of mesh_refit marked stale
  LumResidentRefitStats resident_stats{};
  // skinned and morphed meshes (lumc_mesh_skin_*, lumc_mesh_morph_*; mesh_deform.hip, scene_device.hip skin_meshes): a mesh may hold both, then one launch blends and poses it
  std::map<uint32_t, MeshDeform> mesh_deform;  // by mesh, a record while it holds a part; dropped with the meshes
  DeviceBuffer<uint32_t> d_skin_flags;       // one word of kSkinFlag* / kMorphFlag* bits per launch of an update
  LumMeshSkinStats skin_stats{};
  LumMeshMorphStats morph_stats{};
  // shutter keys (lumc_mesh_shutter_*, lumc_shutter_time; mesh_shutter.hip, scene_device.hip shutter_meshes)
  std::map<uint32_t, MeshShutter> mesh_shutter;  // by mesh, a record while it holds a key; dropped with the meshes
  DeviceBuffer<uint32_t> d_shutter_flags;    // one word of kShutterFlag* bits per launch of an update
  LumShutterStats shutter_stats{};
  // the light tree's refit (lumc_light_refit_*; light_refit.hip, scene_device.hip refit_lights)
  LightRefit light_refit;                    // the bound plan; dropped by every update that takes new lights or new meshes
  Bvh4 light_bvh;                            // the light BVH as the last LUMC_DIRTY_LIGHTS update built it: what a bind makes the refit's topology from
  float light_refit_max_cost_growth = 0.0f;  // lumc_set_light_refit (0: never rebuild for quality)
  bool light_refit_needs_rebuild = false;    // the last LUMC_DIRTY_LIGHT_POSITIONS update left the lights alone
  bool lights_refitted = false;              // within an update: refit_lights ran, k_light_table follows
  LumLightRefitStats light_refit_stats{};
  std::vector<uint32_t> sky_lut_key;  // the sky parameters the two sky tables were generated from
  DeviceBuffer<float> d_bridge_lut;   // the bridge sampler's vertex-count table (context-owned: scene.bridge_lut points here while bridges are possible)
  std::vector<float> bridge_lut_host; // its content, to notice a caller that hands over another table
  DeviceBuffer<float4> d_sky_lut[2];
  DeviceScene scene{};
  bool has_scene = false;
  uint64_t bvh_stats[4] = {0, 0, 0, 0};
  int ambient_reuse = -1;         // -1 by flavour (fast: on), 0 off, 1 on (lumc_set_ambient_reuse; LUM_AMBIENT_REUSE)
  int single_level = -1;          // the ray kernels' single-level form on a scene of one hittable instance: -1 auto (on), 0 never, 1 when eligible (lumc_set_single_level; LUM_SINGLE_LEVEL)
  int plain_form = -1;            // k_shade's plain form on a scene that has nothing it leaves out (plain_scene, wavefront_table.h): -1 auto (on), 0 never, 1 when eligible (lumc_set_plain_form; LUM_PLAIN_FORM)
  int pixel_major = -1;           // lumc_render's path slots: -1 auto (kPixelMajorAuto, core.hip), 0 sample-major, 1 pixel-major (lumc_set_pixel_major; LUM_PIXEL_MAJOR)
  int coherent_first_hits = -1;   // the coherent form of the single-level closest-hit kernel for a pass's depth-0 launch: -1 auto (with pixel-major slots), 0 never, 1 when eligible - and then for lumc_trace_closest too (lumc_set_coherent_first_hits; LUM_COHERENT_FIRST_HITS)
  bool first_leaf_identity = false;  // leaf record 0 of the top level maps a ray onto itself (update_scene_tree): see single_level_allowed
  // The overlapped schedule (core.hip wavefront_depths, overlap_allowed): a depth's light queries run on `side_stream` beside the next depth's closest-hit pass.
  int overlap_lq = -1;            // -1 auto (kOverlapAuto), 0 never, 1 when allowed (lumc_set_overlap_light_query; LUM_OVERLAP_LQ)
  hipStream_t side_stream = nullptr;       // non-blocking, lowest priority; made with the context (null: it could not be made, the serial order is kept)
  std::vector<hipEvent_t> overlap_events;  // two per depth: the depth is shaded (recorded on the caller's stream), its light queries are done (on side_stream)
  bool overlap_fits[2][2] = {{false, false}, {false, false}};  // [exact, fast][two-level, single-level]: the register guard's verdict (overlap_registers_fit), read once per context
  uint32_t shade_grid_rounds = 2;  // k_shade's grid as a multiple of its resident set (0: the common 2048-workgroup cap); LUM_SHADE_GRID
  int fused_resolve = 1;          // with the fast flavour's ambient reuse: k_shade resolves the previous depth's vertices itself (lumc_set_fused_resolve; LUM_FUSED_RESOLVE)
  struct Fused : FusedBuffers {   // what that needs beyond the usual work buffers (work_layout.h lay_out_fused)
    DeviceBuffer<char> block;
    bool records_stale = false;     // a queue's planes changed places (ray-sorting mode 3) since the records were written
    uint32_t refused_capacity = 0;  // the capacity its allocation last failed for: not tried again
  } fused;
  DeviceBuffer<uint2> d_sobol;      // the pass's Sobol / Owen table (dev_sampler.h LUM_SOBOL_TABLE; wavefront_depths fills it)
  int sobol_table = 1;              // LUM_SOBOL_TABLE_RT=0: the sampler hashes every number itself
  int fused_ended = 1;  // the vertices that no entry continues (Fused::ended) are resolved by the next depth's k_shade (1) or by k_resolve_ended after the depth's visibility pass (0; LUM_FUSED_ENDED=0)
  int fused_ended_default = 1;  // what lumc_set_fused_resolve(1) goes back to (the environment's choice, if any)
  int bvh_builder = 3;            // 0 binned SAH on the host, 1 LBVH on the GPU, 2 PLOC on the GPU, 3 binned SAH on the GPU (default since round 4: the host builder's trees in a fifth of its time; a mesh it cannot take falls back to 0) (lumc_set_bvh_builder)
  double bvh_build_seconds = 0.0; // bottom-level builds of the last lumc_scene_upload
  uint32_t bvh_meshes_by_builder[2] = {0, 0};  // meshes of the last upload built by SAH / by LBVH
  uint32_t lds_nodes = 0;         // nodes of the tree top every ray-kernel workgroup stages in LDS
  uint32_t trace_blocks = 256;    // persistent grid of the ray kernels
  // LUTs owned by the context when generated here
  DeviceBuffer<uint16_t> d_luts[4];
  // pixels and accumulators
  DeviceBuffer<uint32_t> d_pixels;
  uint32_t num_pixels = 0;
  uint64_t pixels_hash = 0;       // of the pixel list in its order (lumc_set_pixels): the tile gather checks that the set IS the share of the deal it assumes
  DeviceBuffer<float> d_first_moment, d_second_moment;
  FireflyBuckets firefly;  // median-of-means buckets beside the accumulators (lumc_set_firefly_buckets; firefly.hip)
  struct Work : WorkBuffers { DeviceBuffer<char> block; } work;  // the work buffers, laid out for work.capacity paths (work_layout.h lay_out_work)
  uint32_t particle_lds_nodes = 0;
  DeviceBuffer<float> d_frame_output;  // display-referred planes of the output chain [3 * W * H]
  DeviceBuffer<uint16_t> d_bluenoise_1d;
  DeviceBuffer<uint32_t> d_argb8;
  // adaptive sampling (dev_adaptive.h)
  struct Adaptive {
    bool active = false;
    LumAdaptiveParams params{};
    uint32_t blocks_x = 0, blocks_y = 0, num_blocks = 0;
    uint32_t stage_id = 0;
    uint32_t executions[kAdaptiveStages + 1] = {0, 0, 0, 0, 0};
    DeviceBuffer<uint32_t> d_stage_counts, d_block_tasks, d_block_task_end;
    DeviceBuffer<float> d_block_variance;
    DeviceBuffer<float> d_partial;  // chunk sums, then the total in the last element
    DeviceBuffer<char> d_scan_temp;
    size_t scan_temp_bytes = 0;
    std::vector<uint32_t> task_end;  // host copy of d_block_task_end: passes are cut at block boundaries
    float variance_total = 0.0f;
    DeviceBuffer<uint8_t> d_block_mask;  // image-tile partition over GPUs: blocks this context renders (empty = all)
    bool build_pending = false;      // partitioned: a stage is due and waits for the block variances of all ranks
  } adaptive;
  DeviceBuffer<uint32_t> d_cloud_noise[3];  // the clouds' shape / detail / weather textures generated here (kept across scene uploads)
  bool cloud_noise_static = false;  // shape and detail do not depend on the seed
  uint32_t cloud_noise_seed = 0;
  bool cloud_noise_weather_valid = false;
  DeviceBuffer<float4> d_sky_hdri;  // baked sky (lumc_sky_hdri_build): dim x dim equirectangular, rgb + 0
  uint32_t sky_hdri_dim = 0;
  std::vector<DeviceBuffer<float>> bloom_mips;  // mip chain of lumc_post_bloom, level i of (width >> (i + 1)) x (height >> (i + 1))
  uint32_t bloom_width = 0, bloom_height = 0;  // what the chain was allocated for
  DeviceBuffer<uint32_t> d_undersampling_pixels;  // pixel list of the current undersampling iteration (lumc_render_undersampled)
  std::vector<uint32_t> sky_hdri_key;  // what the bake was made from (sky parameters, origin, dim, samples): an unchanged key reuses it
  DeviceBuffer<float> d_frame_result;  // mean radiance planes of lumc_generate_result [3 * W * H]
  // denoiser (dev_denoise.h): the guide planes (9 while they are summed, then albedo[3] normal[3] depth), the filter's records (A twice: ping-pong, B once)
  DeviceBuffer<float> d_guides;
  bool guides_valid = false;
  Mattes mattes;  // ID mattes of the same first-hit passes (lumc_render_first_hits; matte.hip): nothing is allocated until they are asked for
  // the scene, the lens or the camera changed: both were rendered from what was. `why` is what a refused matte download names.
  void drop_first_hit_products(const char* why) { guides_valid = false; history.motion.owner_cur_valid = false; history.motion.state_current = false; if (mattes.valid) { mattes.valid = false; mattes.stale = why; } }
  DeviceBuffer<float4> d_denoise_rec[3];  // one 16-byte record per pixel each
  History history;  // the shown frame carried across camera moves (lumc_set_history; history.hip): nothing is allocated until it is switched on and blends
  int denoise_lds = 1;              // a-trous steps 1 and 2 stage their tile in LDS (lumc_set_denoise_form; LUM_DENOISE_LDS=0|1)
  // ray ordering (N1): keys + permutation, double-buffered for hipcub's radix sort; sized for the visibility items (4 per path)
  struct RaySort {  // ray_sort.hip
    int mode = 0;              // 0 queue order, 1 closest-hit rays of depth >= 1 traced through a sorted permutation, 2 visibility rays too, 3 the path queue physically reordered (lumc_set_ray_sorting, LUM_SORT)
    PathQueue queue{};         // mode 3: the four state planes the reorder pass writes; swapped with the queue's own afterwards
    DeviceBuffer<float4> planes[4];  // what was allocated for them, one 16-byte entry per path (after swaps queue may point into the work block)
    int key = 0;               // 0 position-major (Morton cell | direction octant), 1 direction-major
    DeviceBuffer<uint32_t> d_keys[2], d_vals[2];
    DeviceBuffer<char> d_temp;  // allocated last: with it the keys and values are complete
    size_t temp_bytes = 0;
    float world_lo[3] = {0, 0, 0}, world_hi[3] = {1, 1, 1};  // bounds of the top-level BVH
  } sort;
  bool sync_debug = false;
  // image-tile multi-GPU (lumc_comm_*, lumc_frame_assemble*): this rank's communicator and its [4][frame pixels] assembly buffer
  struct Exchange {  // multi_gpu.hip (free_exchange ends the communicator)
    ncclComm_t comm = nullptr;
    int comm_rank = 0, comm_world = 1;
    DeviceBuffer<float> d_frame;
    uint32_t frame_pixels() const { return (uint32_t) (d_frame.count() / 4); }  // the planes' stride
    // tile gather (lumc_frame_gather*): this rank's padded [4][gather_stride] send buffer; on the root the [world][4][gather_stride] receive buffer and every
    // rank's pixel list [world][gather_stride] (0xFFFFFFFF = padding), keyed by (width, height, world)
    DeviceBuffer<float> d_gather_send, d_gather_recv;
    DeviceBuffer<uint32_t> d_gather_pixels;
    uint32_t gather_stride = 0, gather_key[3] = {0, 0, 0};
    bool use_frame = false;         // the result / output entry points read the assembled frame instead of this context's own accumulators
  } exchange;
  DeviceBuffer<uint32_t> d_ctrl;  // kCtlStride control words per depth (+1 row), zeroed per pass; last row: cursor of lumc_trace_closest
  DeviceBuffer<uint64_t> d_counters;
  // profiling
  bool profiling = false;
  struct Stamp { hipEvent_t a, b; int kernel; };
  std::vector<Stamp> stamps;
  double kernel_ms[LUMC_KERNEL_COUNT] = {};
  uint32_t kernel_launches[LUMC_KERNEL_COUNT] = {};
};

#define HIP_TRY(ctx, expr)                                                                                          \
  do {                                                                                                              \
    const hipError_t e__ = (expr);                                                                                  \
    if (e__ != hipSuccess) {                                                                                        \
      (ctx)->error = std::string(#expr) + " failed: " + hipGetErrorString(e__);                                     \
      return 1;                                                                                                     \
    }                                                                                                               \
  } while (0)

#pragma GCC visibility push(hidden)  // nothing below is part of the library's interface

constexpr uint32_t kLaunchBlock = 256;  // dev_wave.h's kBlock (core.hip asserts it)
inline uint32_t grid_for(uint32_t n) {
  const uint32_t blocks = (n + kLaunchBlock - 1) / kLaunchBlock;
  return blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);  // 256 CUs x 8 resident blocks, grid-stride beyond that
}

// What the launchers of the ray kernels are told besides the scene (single_level_scene, wavefront_table.h): the switch, and in the fast flavour that the one
// instance's world->object map is the identity. The single-level form maps a ray with the expressions of the instance-entry phase, but under the fast flavour's
// -ffp-contract=fast the compiler decides per place which product of a row goes into which fma (it differs between the rows of ONE kernel), so another
// instantiation rounds another way. With rows of 1 and 0 and no translation every product and sum is exact in any arrangement: the outputs keep their bits.
// The exact flavour compiles without contraction and takes every transform.
inline bool single_level_allowed(const LumContext* ctx) {
  return ctx->single_level != 0 && (ctx->wf != wavefront_kernels_fast() || ctx->first_leaf_identity);
}

// The truth probes' table (wavefront_table.h WavefrontProbes) of the context's flavour: the one place that tells it from ctx->wf.
inline const WavefrontProbes* probes_of(const LumContext* ctx) { return ctx->wf == wavefront_kernels_exact() ? wavefront_probes_exact() : wavefront_probes_fast(); }

// The register guard of the overlapped schedule. A SIMD has 512 vector registers per lane, handed out in blocks of 8; the persistent closest-hit kernel keeps four
// waves on it, and one wave of k_light_query must fit beside them or the two kernels only take turns. (The visibility kernel never runs beside the light queries:
// it waits for them, so its count plays no part.)
inline bool overlap_registers_fit(uint32_t ray_kernel_regs, uint32_t light_query_regs) {
  const uint32_t ray = (ray_kernel_regs + 7u) & ~7u, lq = (light_query_regs + 7u) & ~7u;
  return ray_kernel_regs > 0 && light_query_regs > 0 && 4u * ray + lq <= 512u;
}

// Persistent ray kernels: one workgroup per CU (kTraceBlock threads, its own LDS copy of the tree top); waves pull work from a cursor.
inline uint32_t grid_persistent(const LumContext* ctx, uint32_t n) {
  const uint32_t tb = ctx->wf->trace_block;
  const uint32_t blocks = (n + tb - 1) / tb;
  return blocks < 1 ? 1 : (blocks > ctx->trace_blocks ? ctx->trace_blocks : blocks);
}

struct Launch {
  LumContext* ctx;
  hipStream_t stream;
  int kernel;
  size_t idx = (size_t) -1;
  Launch(LumContext* c, hipStream_t s, int k) : ctx(c), stream(s), kernel(k) {
    if (!ctx->profiling) return;
    LumContext::Stamp st;
    st.kernel = k;
    if (hipEventCreate(&st.a) != hipSuccess || hipEventCreate(&st.b) != hipSuccess) return;
    (void) hipEventRecord(st.a, stream);
    ctx->stamps.push_back(st);
    idx = ctx->stamps.size() - 1;
  }
  ~Launch() {
    if (idx != (size_t) -1) (void) hipEventRecord(ctx->stamps[idx].b, stream);
    if (ctx->sync_debug) {  // LUM_SYNC_DEBUG=1: name the launch group a device fault belongs to
      const hipError_t e = hipStreamSynchronize(stream);
      std::fprintf(stderr, "[lum] launch group %d: %s\n", kernel, hipGetErrorString(e));
    }
  }
};

// what the units call of each other
const uint32_t* sort_rays(LumContext* ctx, hipStream_t stream, const float4* origin, const float4* dir, const uint32_t* count, uint32_t capacity);  // ray_sort.hip
int sort_closest_rays(LumContext* ctx, hipStream_t stream, PathQueue& queue, uint32_t* ctrl, uint32_t N, const uint32_t** order);
void free_sort(LumContext* ctx);  // the buffers of every mode; the settings and the scene's bounds stay
void free_exchange(LumContext* ctx);  // multi_gpu.hip
int scene_device_init();  // scene_device.hip: that unit's copy of the sampler's seed table, per device (a hipError_t; lumc_context_create)
int history_owner_begin(LumContext* ctx, const char* fn, uint32_t n, hipStream_t stream);  // history.hip: the current owner plane, preset to "no path", for a guide render with LUMC_FIRST_HIT_OWNER
int history_owner_pass(LumContext* ctx, const uint4* d_hit_id, const uint32_t* d_paths, uint32_t width, uint32_t n, hipStream_t stream);  // k_history_owner on a pass's first hits
extern "C" uint64_t pixel_list_hash(const uint32_t* pixels, uint32_t n);  // core.hip, among the entry points that use it

#pragma GCC visibility pop
extern "C" int adaptive_compute_variance(LumContext* ctx, hipStream_t stream);  // core.hip (adaptive sampling)
extern "C" int adaptive_finish_build(LumContext* ctx, hipStream_t stream);
