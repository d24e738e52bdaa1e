// C ABI of the path-tracing core (include/lum_core.h): context, scene upload, BVH construction, pass scheduling.
// Host-side counterpart of the reference's device layer for the hot path only:
//   device/device.c (context, streams, constant memory), device/device_work_buffers.c:54-117 (task/result buffers),
//   device/device_renderer.c:53-134, :488-575 (per-depth kernel queue), device/device_result_interface.c (moments).
// There is deliberately no CPU fallback: every entry point fails with an error string when HIP is unavailable.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "../../../include/lum_core.h"
#include "../device/kernels_shared.h"  // the flavour-neutral kernels; the wavefront kernels are csrc/device/wavefront_exact.hip and wavefront_fast.hip
#include <hipcub/hipcub.hpp>
#include "context.h"
#include "tiles.h"

static_assert(kLaunchBlock == (uint32_t) kBlock, "grid_for (context.h) counts the kernels' workgroups");

namespace {

// ---- the process's bottom-level trees by what they were built from: the mesh's triangles (two 64-bit hashes of the vertex words, chunk by chunk so that the
// value does not depend on the number of threads), the builder asked for and every LUM_* variable of the environment (the builders' knobs) ----
struct MeshTreeKey {
  uint64_t h0, h1, env;
  uint32_t tris; int builder;
  bool operator<(const MeshTreeKey& o) const { return std::tie(h0, h1, env, tris, builder) < std::tie(o.h0, o.h1, o.env, o.tris, o.builder); }
};
static std::mutex g_mesh_tree_mutex;
static std::map<MeshTreeKey, std::weak_ptr<const MeshTree>> g_mesh_trees;
extern "C" char** environ;

static MeshTreeKey mesh_tree_key(const float* tri_vertices, uint32_t tris, int builder) {
  constexpr size_t kChunk = 65536;  // triangles (12 floats each)
  const size_t chunks = ((size_t) tris + kChunk - 1) / kChunk;
  std::vector<uint64_t> part(2 * chunks);
  host_parallel_for(chunks, [&](size_t b, size_t e) {
    for (size_t c = b; c < e; c++) {
      const size_t first = c * kChunk, last = std::min<size_t>((size_t) tris, first + kChunk);
      uint64_t a = 0x9E3779B97F4A7C15ull ^ c, z = 0xC2B2AE3D27D4EB4Full + c;
      for (size_t w = first * 6; w < last * 6; w++) {
        uint64_t x;
        std::memcpy(&x, reinterpret_cast<const char*>(tri_vertices) + w * 8, 8);
        a = (a ^ x) * 0x100000001B3ull; a ^= a >> 29;
        z = (z + x) * 0xFF51AFD7ED558CCDull; z ^= z >> 32;
      }
      part[2 * c] = a; part[2 * c + 1] = z;
    }
  });
  MeshTreeKey k{0xCBF29CE484222325ull, 0x84222325CBF29CE4ull, 0xCBF29CE484222325ull, tris, builder};
  for (size_t c = 0; c < chunks; c++) { k.h0 = (k.h0 ^ part[2 * c]) * 0x100000001B3ull; k.h1 = (k.h1 + part[2 * c + 1]) * 0xFF51AFD7ED558CCDull; k.h1 ^= k.h1 >> 32; }
  for (char** e = environ; e && *e; e++)
    if (std::strncmp(*e, "LUM_", 4) == 0) for (const char* p = *e; *p; p++) k.env = (k.env ^ (uint8_t) *p) * 0x100000001B3ull;
  return k;
}
static std::shared_ptr<const MeshTree> find_mesh_tree(const MeshTreeKey& k) {
  if (const char* e = getenv("LUM_BVH_SHARE")) if (atoi(e) == 0) return nullptr;  // every upload builds (tools/lbvh_bench.py times the builders this way)
  std::lock_guard<std::mutex> lock(g_mesh_tree_mutex);
  auto it = g_mesh_trees.find(k);
  if (it == g_mesh_trees.end()) return nullptr;
  std::shared_ptr<const MeshTree> t = it->second.lock();
  if (!t) g_mesh_trees.erase(it);
  return t;
}
static void keep_mesh_tree(const MeshTreeKey& k, const std::shared_ptr<const MeshTree>& t) {
  std::lock_guard<std::mutex> lock(g_mesh_tree_mutex);
  for (auto it = g_mesh_trees.begin(); it != g_mesh_trees.end();) it = it->second.expired() ? g_mesh_trees.erase(it) : std::next(it);
  g_mesh_trees[k] = t;
}

constexpr size_t kCloudNoiseTexels[3] = {(size_t) kCloudShapeRes * kCloudShapeRes * kCloudShapeRes, (size_t) kCloudDetailRes * kCloudDetailRes * kCloudDetailRes,
                                         (size_t) kCloudWeatherRes * kCloudWeatherRes};  // shape, detail, weather (RGBA8 each)
constexpr uint32_t kBsdfLutCount[4] = {1024, 1024, 32768, 32768};  // conductor, glossy, dielectric, dielectric_inv

// A scene array on the device, owned by the allocation group it is registered under.
template <typename T>
int upload(LumContext* ctx, int group, const T* host, size_t count, const T** out) {
  *out = nullptr;
  DeviceBuffer<char> d;
  HIP_TRY(ctx, d.assign(reinterpret_cast<const char*>(host), sizeof(T) * count));
  *out = reinterpret_cast<const T*>(d.get());
  if (d) ctx->scene_allocs[group].push_back(std::move(d));
  return 0;
}

void free_scene(LumContext* ctx) {
  for (auto& group : ctx->scene_allocs) group.clear();
  for (auto& t : ctx->d_luts) t.reset();
  for (auto& t : ctx->d_sky_lut) t.reset();
  ctx->sky_lut_key.clear();
  ctx->d_bridge_lut.reset(); ctx->bridge_lut_host.clear();
  ctx->mesh_bvh.clear(); ctx->mesh_box.clear(); ctx->mesh_refit.clear(); ctx->mesh_tri_offset.clear();
  ctx->has_scene = false;
}

void free_work(LumContext* ctx) {
  ctx->work_block.reset();
  ctx->fused_block.reset(); ctx->fused_capacity = 0; ctx->d_fused = nullptr;
  ctx->fused_refused_capacity = 0;  // memory may have been freed since the refusal: the next pass asks again
  ctx->queue[2] = PathQueue{}; ctx->nee2 = NeeQueue{}; ctx->fallback = ShadowQueue{};
  for (int k = 0; k < 3; k++) ctx->queue[k].parent = nullptr;
  ctx->capacity = 0;
  ctx->work_shadow_kinds = 0;
  ctx->cloud = CloudQueue{};
  // the reorder pass's planes (ray-sorting mode 3) trade places with the queues' own: they go with them (and with them the sort's keys, sized by the pass too)
  free_sort(ctx);
  ctx->d_sobol.reset();
}

int ensure_work(LumContext* ctx, uint32_t paths) {
  // in a volume a path can ask for 19 visibility rays in the in-scattering pass (15 bridge segments, sun and ambient in up to two segments each)
  // instead of 4 at a surface (6 with an ocean: the second segments of the sun and ambient samples of a vertex under water)
  const bool volumes = ctx->scene.fog_active || ctx->scene.ocean_active;
  const uint32_t kinds = volumes ? kVolumeShadowKinds : 4u;
  const bool clouds = ctx->scene.cloud_active && ctx->scene.sky_mode == kSkyDefault;
  if (clouds && paths >= (1u << 30)) { ctx->error = "pass too large for the cloud march list (2^30 paths)"; return 1; }
  if (paths <= ctx->capacity && kinds <= ctx->work_shadow_kinds && (!clouds || ctx->cloud.items)) return 0;
  if (paths < ctx->capacity) paths = ctx->capacity;
  free_work(ctx);
  // per path: 2 queues x 68 B + NEE 84 B + result 16 B + up to `kinds` visibility rays x (48 B + 16 B result) + 4 B light-query index
  // (+ the volumes' 96 B of in-scattering records, 4 B scattering-event index and 48 B of water-surface factors of the surface vertices)
  const size_t n = paths;
  const size_t bytes = n * (2 * 68 + 84 + 16 + (size_t) kinds * 64 + 4 + (kinds > 4u ? 100 + 48 : 0) + (clouds ? 3 * (4 + 16 + 4) : 0)) + 56 * 256;
  HIP_TRY(ctx, ctx->work_block.resize(bytes));
  char* p = ctx->work_block.get();
  auto take = [&](size_t sz) { char* r = p; p += (sz + 255) & ~(size_t) 255; return r; };  // keeps every array 256-byte aligned
  for (int k = 0; k < 2; k++) {
    ctx->queue[k].origin_t = (float4*) take(n * 16);
    ctx->queue[k].dir_slot = (float4*) take(n * 16);
    ctx->queue[k].aux      = (uint4*) take(n * 16);
    ctx->queue[k].hit_id   = (uint4*) take(n * 16);
    ctx->queue[k].hit_scene_tri = (uint32_t*) take(n * 4);
  }
  ctx->nee.geo_color_light = (float4*) take(n * 16);
  ctx->nee.bsdf_ray_prob   = (float4*) take(n * 16);
  ctx->nee.bsdf_weight_sum = (float4*) take(n * 16);
  ctx->nee.ambient         = (uint4*) take(n * 16);
  ctx->nee.sun             = (uint4*) take(n * 16);
  ctx->nee.amb_path        = (uint32_t*) take(n * 4);
  ctx->d_results           = (float4*) take(n * 16);
  ctx->shadow.origin_dist  = (float4*) take(kinds * n * 16);
  ctx->shadow.dir_out      = (float4*) take(kinds * n * 16);
  ctx->shadow.ids          = (uint4*) take(kinds * n * 16);
  ctx->shadow.vis          = (float4*) take(kinds * n * 16);
  ctx->shadow.light_items  = (uint32_t*) take(n * 4);
  ctx->shadow.capacity     = paths;
  ctx->volume = VolumeQueue{};
  ctx->nee.sun_water = nullptr; ctx->nee.amb_t1 = nullptr; ctx->nee.amb_t2 = nullptr;
  if (kinds > 4u) {
    ctx->volume.bridge = (float4*) take(n * 16);
    ctx->volume.sky    = (uint4*) take(n * 16);
    ctx->volume.weight = (float4*) take(n * 16);
    ctx->volume.sun_water = (float4*) take(n * 16);
    ctx->volume.amb_t1 = (float4*) take(n * 16);
    ctx->volume.amb_t2 = (float4*) take(n * 16);
    ctx->volume.items  = (uint32_t*) take(n * 4);
    ctx->nee.sun_water = (float4*) take(n * 16);
    ctx->nee.amb_t1    = (float4*) take(n * 16);
    ctx->nee.amb_t2    = (float4*) take(n * 16);
  }
  ctx->cloud = CloudQueue{};
  if (clouds) {  // per path up to three marches: list entry, result, distance of the first cloud
    ctx->cloud.items    = (uint32_t*) take(3 * n * 4);
    ctx->cloud.result   = (float4*) take(3 * n * 16);
    ctx->cloud.hit_dist = (float*) take(3 * n * 4);
    ctx->cloud.capacity = paths;
  }
  ctx->work_shadow_kinds = kinds;
  ctx->capacity = paths;
  return 0;
}

// The fused resolve's own buffers (FusedResolve, kernels.h), sized like the work buffers: per path a third queue entry (68 B), three parent words, a second
// set of NEE records (84 B) and one fallback ray (48 B + its vertex's index).
// The six records k_shade reads the previous depth through (device memory): rewritten whenever a queue's planes move.
int upload_fused_records(LumContext* ctx, hipStream_t stream) {
  FusedResolve by_depth[6];
  for (int d = 0; d < 6; d++) {  // depth d is shaded from queue d % 3 with the records d & 1: the depth before it lives in queue (d + 2) % 3 and the other record set
    by_depth[d].prev = ctx->queue[(d + 2) % 3];
    by_depth[d].nee_prev = (d & 1) ? ctx->nee : ctx->nee2;
    by_depth[d].fallback = ctx->fallback;
    by_depth[d].ended = ctx->d_ended[d & 1];
    by_depth[d].ended_prev = ctx->d_ended[(d & 1) ^ 1];
  }
  HIP_TRY(ctx, hipStreamSynchronize(stream));  // a pass still reading the old records on a non-blocking stream is not ordered against the null-stream copy below
  HIP_TRY(ctx, hipMemcpy(ctx->d_fused, by_depth, sizeof(by_depth), hipMemcpyHostToDevice));
  ctx->fused_records_stale = false;
  return 0;
}
int ensure_fused(LumContext* ctx, hipStream_t stream) {
  if (ctx->fused_block && ctx->fused_capacity == ctx->capacity) return ctx->fused_records_stale ? upload_fused_records(ctx, stream) : 0;
  if (ctx->fused_refused_capacity == ctx->capacity) return 1;
  ctx->fused_capacity = 0;
  const size_t n = ctx->capacity;
  const size_t bytes = n * (68 + 3 * 4 + 84 + 48 + 4 + 2 * 4) + 27 * 256 + 6 * sizeof(FusedResolve);
  if (ctx->fused_block.resize(bytes) != hipSuccess) { ctx->fused_refused_capacity = ctx->capacity; return 1; }
  char* p = ctx->fused_block.get();
  auto take = [&](size_t sz) { char* r = p; p += (sz + 255) & ~(size_t) 255; return r; };
  PathQueue& q = ctx->queue[2];
  q.origin_t = (float4*) take(n * 16); q.dir_slot = (float4*) take(n * 16); q.aux = (uint4*) take(n * 16); q.hit_id = (uint4*) take(n * 16);
  q.hit_scene_tri = (uint32_t*) take(n * 4);
  for (int k = 0; k < 3; k++) ctx->queue[k].parent = (uint32_t*) take(n * 4);
  NeeQueue& e = ctx->nee2;
  e = NeeQueue{};
  e.geo_color_light = (float4*) take(n * 16); e.bsdf_ray_prob = (float4*) take(n * 16); e.bsdf_weight_sum = (float4*) take(n * 16);
  e.ambient = (uint4*) take(n * 16); e.sun = (uint4*) take(n * 16); e.amb_path = (uint32_t*) take(n * 4);
  ShadowQueue& f = ctx->fallback;
  f.origin_dist = (float4*) take(n * 16); f.dir_out = (float4*) take(n * 16); f.ids = (uint4*) take(n * 16);
  f.light_items = (uint32_t*) take(n * 4);
  f.vis = ctx->shadow.vis;  // the undecided samples' answers go where the depth's own ambient answers went: kind 2 of the previous depth's words
  f.capacity = ctx->shadow.capacity;
  ctx->d_ended[0] = (uint32_t*) take(n * 4); ctx->d_ended[1] = (uint32_t*) take(n * 4);
  ctx->d_fused = (FusedResolve*) take(6 * sizeof(FusedResolve));
  ctx->fused_capacity = ctx->capacity;
  return upload_fused_records(ctx, stream);
}

constexpr uint32_t kCtrlRows = 68;  // depths 0..63, one row past the last depth, spare, lumc_trace_closest

// k_shade: its workgroups are grid-stride loops of equal length, three of them resident per CU (3 waves per SIMD). With the common cap of 2048 workgroups that
// was 2.67 rounds of the 768 resident places, paid as 3; the grid is now a whole number of rounds, and eight of them: the shorter a workgroup, the shorter the
// kernel's tail (hall, k_shade per 3 steps: 2048 workgroups 380 ms | 1 round 399 | 2: 383 | 3: 376 | 4: 372 | 6: 369 | 8: 368 | 12: 366 | 24: 371; the Example-class
// scene is best at 6-8). LUM_SHADE_GRID=<rounds> (0: the 2048 cap).
inline uint32_t shade_grid(const LumContext* ctx, uint32_t n) {
  const uint32_t blocks = (n + kBlock - 1) / kBlock;
  const uint32_t resident = ctx->trace_blocks * 3u;  // trace_blocks = the device's CUs (one persistent ray workgroup each)
  // (not with an ocean: k_shade<.., ocean> keeps a scratch frame and its workgroups cost more to start - Example-class scene with an ocean, 8 rounds: shade +2 %)
  // input by cursor (kernels.h): twice the resident set. The second half only starts when the queue is used up and leaves at once; what it buys is that every
  // place is taken from the start (hall, k_shade per 3 steps: fixed shares 345 ms | cursor, 1 x resident 337 | 2 x: 333 | 3 x: 331 | 4 x: 332; the scan and
  // the Example-class scene, whose launches are short, are level at 1-2 x and lose 3-5 % at 3-4 x: profiles/r05_ab_experiments.txt). LUM_SHADE_GRID=<rounds>.
  const uint32_t rounds = ctx->shade_grid_rounds;
  const uint32_t cap = resident * (rounds ? rounds : 1u);
  return blocks < 1 ? 1 : std::min(blocks, cap);
}

int resolve_stamps(LumContext* ctx) {
  for (auto& st : ctx->stamps) {
    float ms = 0.0f;
    if (hipEventSynchronize(st.b) == hipSuccess && hipEventElapsedTime(&ms, st.a, st.b) == hipSuccess) {
      ctx->kernel_ms[st.kernel] += ms;
      ctx->kernel_launches[st.kernel]++;
    }
    (void) hipEventDestroy(st.a);
    (void) hipEventDestroy(st.b);
  }
  ctx->stamps.clear();
  return 0;
}

}  // namespace

extern "C" {

int lumc_context_create(int device_ordinal, LumContext** out) {
  if (!out) return 1;
  *out = nullptr;
  LumContext* ctx = new LumContext();
  ctx->device = device_ordinal;
  if (const char* b = getenv("LUM_BVH_BUILDER")) ctx->bvh_builder = (std::strcmp(b, "lbvh") == 0) ? 1 : (std::strcmp(b, "ploc") == 0) ? 2 : (std::strcmp(b, "sah") == 0 || std::strcmp(b, "host") == 0) ? 0 : 3;
  if (const char* e = getenv("LUM_SORT")) ctx->sort.mode = atoi(e);
  if (const char* e = getenv("LUM_SYNC_DEBUG")) ctx->sync_debug = atoi(e) != 0;
  if (const char* e = getenv("LUM_SORT_KEY")) ctx->sort.key = atoi(e);
  if (const char* e = getenv("LUM_AMBIENT_REUSE")) ctx->ambient_reuse = atoi(e) != 0 ? 1 : 0;
  if (const char* e = getenv("LUM_FUSED_RESOLVE")) ctx->fused_resolve = atoi(e) != 0 ? 1 : 0;
  if (const char* e = getenv("LUM_SHADE_GRID")) ctx->shade_grid_rounds = (uint32_t) atoi(e);
  if (const char* e = getenv("LUM_SOBOL_TABLE_RT")) ctx->sobol_table = atoi(e) != 0 ? 1 : 0;
  if (const char* e = getenv("LUM_FUSED_ENDED")) ctx->fused_ended = ctx->fused_ended_default = atoi(e) != 0 ? 1 : 0;
  if (const char* e = getenv("LUM_DENOISE_LDS")) ctx->denoise_lds = atoi(e) != 0 ? 1 : 0;
  if (const char* f = getenv("LUM_FLAVOUR")) ctx->wf = (std::strcmp(f, "exact") == 0) ? wavefront_kernels_exact() : wavefront_kernels_fast();
  *out = ctx;
  int count = 0;
  HIP_TRY(ctx, hipGetDeviceCount(&count));
  if (device_ordinal < 0 || device_ordinal >= count) { ctx->error = "no such HIP device"; return 1; }
  HIP_TRY(ctx, hipSetDevice(device_ordinal));
  HIP_TRY(ctx, (hipError_t) wavefront_kernels_exact()->init_sampler_seeds());  // per device: module globals live on each GPU
  HIP_TRY(ctx, (hipError_t) wavefront_kernels_fast()->init_sampler_seeds());
  HIP_TRY(ctx, (hipError_t) exact::upload_sampler_seeds());  // this unit's own table: k_sky_hdri, k_generate_lut and k_pixel_ray draw random numbers
  HIP_TRY(ctx, ctx->d_ctrl.resize(kCtlStride * kCtrlRows));
  HIP_TRY(ctx, hipMemset(ctx->d_ctrl.get(), 0, sizeof(uint32_t) * kCtlStride * kCtrlRows));
  HIP_TRY(ctx, ctx->d_counters.resize(LUMC_CNT_COUNT));
  HIP_TRY(ctx, hipMemset(ctx->d_counters.get(), 0, sizeof(uint64_t) * LUMC_CNT_COUNT));
  return 0;
}

void lumc_context_destroy(LumContext* ctx) {
  if (!ctx) return;
  (void) hipSetDevice(ctx->device);
  (void) hipDeviceSynchronize();
  resolve_stamps(ctx);
  free_exchange(ctx);
  delete ctx;
}

const char* lumc_last_error(const LumContext* ctx) { return ctx ? ctx->error.c_str() : "null context"; }
uint32_t lumc_scene_view_sizeof(void) { return (uint32_t) sizeof(LumDeviceSceneView); }

// The clouds' noise textures (device_cloud.c:62-101): shape and detail once per context, the weather map per seed.
static int ensure_cloud_noise(LumContext* ctx, uint32_t seed) {
  for (int k = 0; k < 3; k++)
    if (!ctx->d_cloud_noise[k]) HIP_TRY(ctx, ctx->d_cloud_noise[k].resize(kCloudNoiseTexels[k]));
  if (!ctx->cloud_noise_static) {
    hipLaunchKernelGGL(exact::k_cloud_noise_shape, dim3(2048), dim3(256), 0, 0, ctx->d_cloud_noise[0].get(), (uint32_t) kCloudShapeRes);
    hipLaunchKernelGGL(exact::k_cloud_noise_detail, dim3(128), dim3(256), 0, 0, ctx->d_cloud_noise[1].get(), (uint32_t) kCloudDetailRes);
    HIP_TRY(ctx, hipGetLastError());
    ctx->cloud_noise_static = true;
  }
  if (!ctx->cloud_noise_weather_valid || ctx->cloud_noise_seed != seed) {
    hipLaunchKernelGGL(exact::k_cloud_noise_weather, dim3(2048), dim3(256), 0, 0, ctx->d_cloud_noise[2].get(), (uint32_t) kCloudWeatherRes, (float) seed);
    HIP_TRY(ctx, hipGetLastError());
    ctx->cloud_noise_seed = seed; ctx->cloud_noise_weather_valid = true;
  }
  HIP_TRY(ctx, hipDeviceSynchronize());
  return 0;
}
int lumc_cloud_noise_generate(LumContext* ctx, uint32_t seed, uint32_t* shape, uint32_t* detail, uint32_t* weather) {
  if (!ctx) return 1;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (ensure_cloud_noise(ctx, seed)) return 1;
  uint32_t* out[3] = {shape, detail, weather};
  for (int k = 0; k < 3; k++)
    if (out[k]) HIP_TRY(ctx, hipMemcpy(out[k], ctx->d_cloud_noise[k].get(), sizeof(uint32_t) * kCloudNoiseTexels[k], hipMemcpyDeviceToHost));
  return 0;
}

// The particle tree (device_particle.c:23-131, optix_bvh.c's particle GAS / IAS): one bottom-level tree over the 2 x count triangles of the unit
// cell, and a top level over its 25 x 25 x 25 integer translations, instance id = (xi * 25 + yi) * 25 + zi as the reference numbers them. The
// top-level leaves hold the translation as an exact affine map (rows of the identity), so entering an instance is one subtraction per axis.
static int build_particle_tree(LumContext* ctx, int group, const LumDeviceSceneView* v, DeviceScene& sc) {
  sc.particle_bvh_nodes = nullptr; sc.particle_tris = nullptr; sc.particle_leaves = nullptr; sc.particle_tlas_num_nodes = 0; sc.particle_normals = nullptr;
  if (!sc.particles_active) return 0;
  if (!v->particle_vertices || !v->particle_normals) { ctx->error = "lumc_scene_upload: active particles without particle_vertices / particle_normals"; return 1; }
  const uint32_t nt = 2u * sc.particles_count;
  std::vector<Aabb> tri_boxes(nt);
  Aabb cell{{FLT_MAX, FLT_MAX, FLT_MAX}, {-FLT_MAX, -FLT_MAX, -FLT_MAX}};
  for (uint32_t t = 0; t < nt; t++) {
    const float* p = v->particle_vertices + (size_t) t * 12;
    tri_boxes[t] = tri_box(p, p + 4, p + 8);
    for (int k = 0; k < 3; k++) { cell.lo[k] = std::min(cell.lo[k], tri_boxes[t].lo[k]); cell.hi[k] = std::max(cell.hi[k], tri_boxes[t].hi[k]); }
  }
  constexpr int kDim = 25;  // PARTICLES_BLOCK_DIM
  std::vector<Aabb> boxes((size_t) kDim * kDim * kDim);
  std::vector<float> offsets(3 * boxes.size());
  uint32_t id = 0;
  for (int xi = 0; xi < kDim; xi++)
    for (int yi = 0; yi < kDim; yi++)
      for (int zi = 0; zi < kDim; zi++, id++) {
        const float off[3] = {(float) (xi - (kDim >> 1)), (float) (yi - (kDim >> 1)), (float) (zi - (kDim >> 1))};
        for (int k = 0; k < 3; k++) { offsets[3 * id + k] = off[k]; boxes[id].lo[k] = cell.lo[k] + off[k] - 1e-5f; boxes[id].hi[k] = cell.hi[k] + off[k] + 1e-5f; }
      }
  Bvh4 tlas = build_bvh4(boxes.data(), (uint32_t) boxes.size(), 1, 16);
  Bvh4 blas = build_bvh4(tri_boxes.data(), nt, kBvhLeafMaxTri, 26);
  if (tlas.nodes.empty() || blas.nodes.empty()) { ctx->error = "particle BVH exceeds the traversal's depth limits"; return 1; }
  std::vector<Bvh4Node> nodes = tlas.nodes;
  const uint32_t base = (uint32_t) nodes.size();
  for (Bvh4Node n : blas.nodes) {
    for (int k = 0; k < 4; k++) if (n.child[k] != kBvhEmpty && !(n.child[k] & kBvhLeafBit)) n.child[k] += base;
    nodes.push_back(n);
  }
  std::vector<BvhTri> tris((size_t) nt + 1);
  std::memset(tris.data(), 0, sizeof(BvhTri) * tris.size());
  for (uint32_t i = 0; i < nt; i++) {
    const uint32_t t = blas.prims[i];
    tris[i] = bvh_tri(v->particle_vertices + (size_t) t * 12, t, t, kBvhTriNoTexture);
  }
  std::vector<float4> leaves(4 * tlas.prims.size() + 4);
  for (size_t i = 0; i < tlas.prims.size(); i++) {
    const uint32_t inst = tlas.prims[i];
    leaves[4 * i + 0] = make_float4(1.0f, 0.0f, 0.0f, offsets[3 * inst + 0]);
    leaves[4 * i + 1] = make_float4(0.0f, 1.0f, 0.0f, offsets[3 * inst + 1]);
    leaves[4 * i + 2] = make_float4(0.0f, 0.0f, 1.0f, offsets[3 * inst + 2]);
    const uint32_t words[4] = {inst, base, 0u, 0u};
    std::memcpy(&leaves[4 * i + 3], words, 16);
  }
  if (upload(ctx, group, nodes.data(), nodes.size(), &sc.particle_bvh_nodes)) return 1;
  if (upload(ctx, group, tris.data(), tris.size(), &sc.particle_tris)) return 1;
  if (upload(ctx, group, leaves.data(), leaves.size(), &sc.particle_leaves)) return 1;
  if (upload(ctx, group, (const float4*) v->particle_normals, (size_t) sc.particles_count, &sc.particle_normals)) return 1;
  sc.particle_tlas_num_nodes = (uint32_t) tlas.nodes.size();
  sc.particle_num_leaves = (uint32_t) (leaves.size() / 4);
  ctx->particle_lds_nodes = (uint32_t) std::min<size_t>(ctx->lds_nodes, nodes.size());
  return 0;
}

// ---- the scene on the device, part by part (scene_update below runs the parts in this order). A part frees what it allocated before; a part that is not
// dirty keeps its device arrays and the fields of ctx->scene that point at them. ----
static uint32_t total_triangles(const LumDeviceSceneView* v) { return v->num_meshes ? v->mesh_tri_offset[v->num_meshes] : 0; }

static int update_mesh_arrays(LumContext* ctx, const LumDeviceSceneView* v) {
  DeviceScene& sc = ctx->scene;
  const uint32_t total_tris = total_triangles(v);
  ctx->scene_allocs[LumContext::kGrpMesh].clear();
  if (upload(ctx, LumContext::kGrpMesh, v->mesh_tri_offset, (size_t) v->num_meshes + 1, &sc.mesh_tri_offset)) return 1;
  if (upload(ctx, LumContext::kGrpMesh, (const float4*) v->vertices, (size_t) total_tris * 3, &sc.vertices)) return 1;
  return upload(ctx, LumContext::kGrpMesh, (const uint4*) v->tri_tex, (size_t) total_tris, &sc.tri_tex);
}

// (the scene tree's arrays - update_scene_tree - belong to this group too: whenever the instances are dirty both parts run, this one first)
static int update_instance_arrays(LumContext* ctx, const LumDeviceSceneView* v) {
  DeviceScene& sc = ctx->scene;
  ctx->scene_allocs[LumContext::kGrpInst].clear();
  if (upload(ctx, LumContext::kGrpInst, v->instance_mesh_ids, v->num_instances, &sc.instance_mesh_ids)) return 1;
  return upload(ctx, LumContext::kGrpInst, (const float4*) v->instance_transforms, (size_t) v->num_instances * 2, &sc.instance_transforms);
}

static int update_materials(LumContext* ctx, const LumDeviceSceneView* v) {
  ctx->scene_allocs[LumContext::kGrpMat].clear();
  return upload(ctx, LumContext::kGrpMat, (const uint4*) v->materials, (size_t) v->num_materials * 2, &ctx->scene.materials);
}

// The light tree's root children as floats (dev_light.h tree_prepass): mean = byte * 2^e + base per axis, sigma = byte * 2^e_sigma, power = the 16-bit
// integer - the operations the kernels used to perform per vertex (cuda/light_tree.cuh:133-161, :203-205), every one exact or a single
// binary32 rounding, so the table holds the same bits (this translation unit is compiled without contraction).
static int upload_light_root_children(LumContext* ctx, const LumDeviceSceneView* v, uint32_t sections) {
  const uint32_t* h = (const uint32_t*) v->light_tree_root;
  auto bf = [](uint32_t v16) { const uint32_t b = (v16 & 0xFFFFu) << 16; float f; std::memcpy(&f, &b, 4); return f; };
  const float base[3] = {bf(h[0]), bf(h[0] >> 16), bf(h[1])};
  const float ex[3] = {std::ldexp(1.0f, (int8_t) (h[3] & 0xFF)), std::ldexp(1.0f, (int8_t) ((h[3] >> 8) & 0xFF)), std::ldexp(1.0f, (int8_t) ((h[3] >> 16) & 0xFF))};
  const float ev = std::ldexp(1.0f, (int8_t) (h[3] >> 24));
  std::vector<float> table((size_t) sections * 8 * 8 + 16, 0.0f);  // + one pair of zeros: the pass reads two children per step
  for (uint32_t s = 0; s < sections; s++) {
    const uint8_t* sec = (const uint8_t*) (h + 4 + 12 * s);  // 8 x rel mean x, y, z, rel std dev, then 8 x u16 power
    for (uint32_t c = 0; c < 8; c++) {
      float* e = &table[((size_t) s * 8 + c) * 8];
      for (int a = 0; a < 3; a++) { const float q = (float) sec[8 * a + c]; const float scaled = q * ex[a]; e[a] = scaled + base[a]; }
      e[3] = (float) sec[24 + c] * ev;
      uint16_t pw; std::memcpy(&pw, sec + 32 + 2 * c, 2);
      e[4] = (float) pw;
    }
  }
  return upload(ctx, LumContext::kGrpLight, table.data(), table.size(), &ctx->scene.light_root_children);
}

// (the light BVH and k_light_table's records - update_light_bvh, update_counts_and_tables - belong to this group too and run whenever this part does)
static int update_light_tree(LumContext* ctx, const LumDeviceSceneView* v) {
  DeviceScene& sc = ctx->scene;
  ctx->scene_allocs[LumContext::kGrpLight].clear();
  sc.light_tree_root = nullptr; sc.light_root_children = nullptr; sc.light_tree_nodes = nullptr; sc.light_tri_handles = nullptr; sc.light_tri_table = nullptr;
  sc.light_nodes = nullptr; sc.light_tris = nullptr; sc.light_num_nodes = 0;
  if (!v->light_tree_root || !v->num_lights) return 0;
  const uint32_t sections = v->light_tree_root[10];
  if (upload(ctx, LumContext::kGrpLight, (const uint4*) v->light_tree_root, (size_t) 1 + 3 * sections, &sc.light_tree_root)) return 1;
  if (upload_light_root_children(ctx, v, sections)) return 1;
  if (upload(ctx, LumContext::kGrpLight, (const uint4*) v->light_tree_nodes, (size_t) v->num_light_tree_nodes * 4, &sc.light_tree_nodes)) return 1;
  return upload(ctx, LumContext::kGrpLight, (const uint2*) v->light_tri_handles, v->num_lights, &sc.light_tri_handles);
}

static int update_textures(LumContext* ctx, const LumDeviceSceneView* v) {
  DeviceScene& sc = ctx->scene;
  ctx->scene_allocs[LumContext::kGrpTex].clear();
  sc.num_textures = 0; sc.texture_table = nullptr; sc.texels = nullptr;
  if (!v->num_textures || !v->texture_table || !v->texels) return 0;
  size_t texel_count = 0;
  for (uint32_t t = 0; t < v->num_textures; t++)
    texel_count = std::max(texel_count, (size_t) v->texture_table[4 * t] + (size_t) v->texture_table[4 * t + 1] * v->texture_table[4 * t + 2]);
  if (upload(ctx, LumContext::kGrpTex, (const uint4*) v->texture_table, v->num_textures, &sc.texture_table)) return 1;
  if (upload(ctx, LumContext::kGrpTex, v->texels, texel_count, &sc.texels)) return 1;
  sc.num_textures = v->num_textures;
  return 0;
}

// A mesh's tree from the process's cache, else built by the context's builder and entered there; null (ctx->error set) for a mesh no builder can take.
static std::shared_ptr<const MeshTree> cached_or_built_mesh_tree(LumContext* ctx, const MeshTreeKey& key, const Aabb* tri_boxes, uint32_t nt) {
  std::shared_ptr<const MeshTree> tree = find_mesh_tree(key);
  if (tree) return tree;
  auto built = std::make_shared<MeshTree>();
  if (ctx->bvh_builder == 1) built->bvh = build_bvh4_lbvh(tri_boxes, nt, kBvhLeafMaxTri, 26);
  else if (ctx->bvh_builder == 2) built->bvh = build_bvh4_ploc(tri_boxes, nt, kBvhLeafMaxTri, 26);
  else if (ctx->bvh_builder == 3) built->bvh = build_bvh4_sah_gpu(tri_boxes, nt, kBvhLeafMaxTri, 26);
  built->built_on_gpu = !built->bvh.nodes.empty();
  if (!built->built_on_gpu) built->bvh = build_bvh4(tri_boxes, nt, kBvhLeafMaxTri, 26);  // the host builder: asked for, or the fallback for a mesh the GPU builders cannot take
  if (built->bvh.nodes.empty()) { ctx->error = "mesh BVH exceeds 26 levels"; return nullptr; }
  tree = built;
  keep_mesh_tree(key, tree);
  return tree;
}

// Every mesh's box, tree (from the process's cache, else built) and traversal triangles: the only part of an upload that takes long; an instance edit skips it.
static int build_mesh_trees(LumContext* ctx, const LumDeviceSceneView* v, std::vector<BvhTri>& blas_tris) {
  ctx->bvh_build_seconds = 0.0;
  ctx->bvh_meshes_by_builder[0] = ctx->bvh_meshes_by_builder[1] = 0;
  ctx->mesh_bvh.assign(v->num_meshes, nullptr);
  ctx->mesh_box.assign(v->num_meshes, Aabb{});
  ctx->mesh_refit.clear(); ctx->mesh_refit.resize(v->num_meshes);
  ctx->mesh_tri_offset.assign(v->mesh_tri_offset, v->mesh_tri_offset + v->num_meshes + 1);
  blas_tris.assign((size_t) total_triangles(v) + 1, BvhTri{});
  for (uint32_t m = 0; m < v->num_meshes; m++) {
    const uint32_t t0 = v->mesh_tri_offset[m], nt = v->mesh_tri_offset[m + 1] - t0;
    const float* vertices = v->vertices + (size_t) t0 * 12;
    std::vector<Aabb> tri_boxes(nt);
    ctx->mesh_box[m] = mesh_triangle_boxes(vertices, nt, tri_boxes.data());
    const auto t_build = std::chrono::steady_clock::now();
    const MeshTreeKey key = mesh_tree_key(vertices, nt, ctx->bvh_builder);
    std::shared_ptr<const MeshTree> tree = cached_or_built_mesh_tree(ctx, key, tri_boxes.data(), nt);
    if (!tree) return 1;
    ctx->bvh_meshes_by_builder[tree->built_on_gpu ? 1 : 0]++;
    ctx->bvh_build_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_build).count();
    fill_mesh_tris(vertices, t0, tree->bvh.prims.data(), nt, blas_tris.data() + t0);
    ctx->mesh_bvh[m] = std::move(tree);
    ctx->mesh_refit[m].fit_hash[0] = key.h0; ctx->mesh_refit[m].fit_hash[1] = key.h1;
  }
  return 0;
}

// LUMC_DIRTY_MESH_POSITIONS: the vertex arrays of the same meshes again - the traversal triangles stay on the device (update_mesh_arrays frees its group) -, then
// every mesh whose vertices differ from those its held tree was fitted to gets a tree for them: refitted on the device (bvh_refit.hip; the tree becomes
// private to this context, the shared one it came from is not touched and the cache never sees the refitted one) or, where the mode, the cost's growth or a
// tree that cannot be refitted says so, from the cache / the builder like an upload. *rebuilt: a mesh's traversal triangles were written anew (k_tri_opacity).
static int refit_mesh_trees(LumContext* ctx, const LumDeviceSceneView* v, bool* rebuilt) {
  using clock = std::chrono::steady_clock;
  auto since = [](clock::time_point t) { return std::chrono::duration<double>(clock::now() - t).count(); };
  DeviceScene& sc = ctx->scene;
  LumMeshRefitStats& st = ctx->refit_stats;
  st.last_refits = st.last_rebuilds = 0; st.max_cost_growth = st.seconds = st.seconds_upload = st.seconds_refit = st.seconds_rebuild = st.seconds_assemble = 0.0;
  st.seconds_hash = st.seconds_download = st.seconds_lights = 0.0;
  *rebuilt = false;
  if (ctx->mesh_bvh.size() != v->num_meshes || ctx->mesh_refit.size() != v->num_meshes || ctx->mesh_tri_offset.size() != (size_t) v->num_meshes + 1 ||
      std::memcmp(ctx->mesh_tri_offset.data(), v->mesh_tri_offset, sizeof(uint32_t) * ((size_t) v->num_meshes + 1)) != 0) {
    ctx->error = "lumc_scene_update: LUMC_DIRTY_MESH_POSITIONS with other meshes or triangle counts than the scene on the device";
    return 1;
  }
  const auto t_all = clock::now();
  auto& group = ctx->scene_allocs[LumContext::kGrpMesh];
  DeviceBuffer<char> tris_buffer;
  for (auto& b : group) if (b.get() == reinterpret_cast<const char*>(sc.blas_tris)) tris_buffer = std::move(b);
  if (!tris_buffer) { ctx->error = "lumc_scene_update: the scene on the device has no traversal triangles"; return 1; }
  BvhTri* d_tris = reinterpret_cast<BvhTri*>(tris_buffer.get());
  const int failed = update_mesh_arrays(ctx, v);
  group.push_back(std::move(tris_buffer));
  if (failed) return 1;
  HIP_TRY(ctx, hipDeviceSynchronize());
  st.seconds_upload = since(t_all);
  for (uint32_t m = 0; m < v->num_meshes; m++) {
    const uint32_t t0 = v->mesh_tri_offset[m], nt = v->mesh_tri_offset[m + 1] - t0;
    if (nt == 0) continue;
    const float* vertices = v->vertices + (size_t) t0 * 12;
    MeshRefit& mr = ctx->mesh_refit[m];
    const auto t_hash = clock::now();
    const MeshTreeKey key = mesh_tree_key(vertices, nt, ctx->bvh_builder);
    st.seconds_hash += since(t_hash);
    if (key.h0 == mr.fit_hash[0] && key.h1 == mr.fit_hash[1]) continue;  // the held tree fits these vertices
    bool build = ctx->refit_mode == 1;
    if (!build) {
      const auto t_refit = clock::now();
      if (mr.built_cost == 0.0) mr.built_cost = bvh4_cost(ctx->mesh_bvh[m]->bvh);  // (no refit yet: the held tree is the built one)
      if (!mr.plan.nodes) {
        const hipError_t e = refit_plan_create(mr.plan, ctx->mesh_bvh[m]->bvh, nt);
        if (e == hipErrorInvalidValue) build = true;  // spatial splits: more references than triangles
        else HIP_TRY(ctx, e);
      }
      if (!build) {
        if (!mr.own) {
          mr.own = std::make_shared<MeshTree>();
          mr.own->bvh.prims = ctx->mesh_bvh[m]->bvh.prims; mr.own->bvh.max_depth = ctx->mesh_bvh[m]->bvh.max_depth; mr.own->built_on_gpu = ctx->mesh_bvh[m]->built_on_gpu;
          mr.own->bvh.nodes.resize(mr.plan.num_nodes);
        }
        Aabb box;
        double download = 0.0;
        HIP_TRY(ctx, refit_run(mr.plan, sc.vertices + 3 * (size_t) t0, d_tris + t0, nullptr, mr.own->bvh.nodes.data(), &box, &download));
        st.seconds_download += download;
        const double growth = mr.built_cost > 0.0 ? bvh4_cost(mr.own->bvh) / mr.built_cost : 1.0;
        st.max_cost_growth = std::max(st.max_cost_growth, growth);
        if (ctx->refit_max_cost_growth > 0.0f && growth > (double) ctx->refit_max_cost_growth) build = true;
        else { ctx->mesh_bvh[m] = mr.own; ctx->mesh_box[m] = box; st.refits++; st.last_refits++; }
      }
      st.seconds_refit += since(t_refit);
    }
    if (build) {
      const auto t_build = clock::now();
      std::vector<Aabb> tri_boxes(nt);
      ctx->mesh_box[m] = mesh_triangle_boxes(vertices, nt, tri_boxes.data());
      std::shared_ptr<const MeshTree> tree = cached_or_built_mesh_tree(ctx, key, tri_boxes.data(), nt);
      if (!tree) return 1;
      std::vector<BvhTri> tris(nt);
      fill_mesh_tris(vertices, t0, tree->bvh.prims.data(), nt, tris.data());
      HIP_TRY(ctx, hipMemcpy(d_tris + t0, tris.data(), sizeof(BvhTri) * nt, hipMemcpyHostToDevice));
      mr.plan.reset(); mr.own.reset();
      mr.built_cost = bvh4_cost(tree->bvh);
      ctx->mesh_bvh[m] = std::move(tree);
      *rebuilt = true;
      st.rebuilds++; st.last_rebuilds++;
      st.seconds_rebuild += since(t_build);
    }
    mr.fit_hash[0] = key.h0; mr.fit_hash[1] = key.h1;
  }
  st.seconds = since(t_all);
  return 0;
}

// Top level + every mesh's tree in ONE node array (bvh_build.cpp assemble_scene_tree), in the instances' group; the traversal triangles in the meshes'.
static int update_scene_tree(LumContext* ctx, const LumDeviceSceneView* v, bool dirty_meshes, size_t* num_nodes) {
  DeviceScene& sc = ctx->scene;
  std::vector<BvhTri> blas_tris;
  if (dirty_meshes && build_mesh_trees(ctx, v, blas_tris)) return 1;
  if (ctx->mesh_box.size() != v->num_meshes || ctx->mesh_bvh.size() != v->num_meshes) { ctx->error = "lumc_scene_update: the meshes changed but LUMC_DIRTY_MESHES is not set"; return 1; }
  std::vector<const Bvh4*> mesh_bvh(v->num_meshes);
  for (uint32_t m = 0; m < v->num_meshes; m++) mesh_bvh[m] = &ctx->mesh_bvh[m]->bvh;
  const SceneTree tree = assemble_scene_tree(*v, mesh_bvh.data(), ctx->mesh_box.data());
  if (tree.nodes.empty()) { ctx->error = "top-level BVH exceeds 16 levels"; return 1; }
  if (total_triangles(v) >= (1u << 28) || tree.nodes.size() >= (1u << 25)) { ctx->error = "scene too large for 28-bit leaf ranges / 32-bit node offsets"; return 1; }
  // by instance id: the exact flavour's ambient reuse re-tests a ray against a hit's triangle (k_resolve_reuse)
  if (upload(ctx, LumContext::kGrpInst, tree.inv_rows.data(), tree.inv_rows.size(), &sc.instance_rows)) return 1;
  if (upload(ctx, LumContext::kGrpInst, tree.nodes.data(), tree.nodes.size(), &sc.bvh_nodes)) return 1;
  if (dirty_meshes && upload(ctx, LumContext::kGrpMesh, blas_tris.data(), blas_tris.size(), &sc.blas_tris)) return 1;
  if (upload(ctx, LumContext::kGrpInst, tree.tlas_leaves.data(), tree.tlas_leaves.size(), &sc.tlas_leaves)) return 1;
  sc.tlas_num_nodes = tree.tlas_num_nodes;
  sc.tlas_num_leaves = (uint32_t) (tree.tlas_leaves.size() / 4);  // records that exist (one of padding included): what a workgroup may stage in LDS
  std::memcpy(ctx->sort.world_lo, tree.world.lo, sizeof(ctx->sort.world_lo)); std::memcpy(ctx->sort.world_hi, tree.world.hi, sizeof(ctx->sort.world_hi));
  ctx->bvh_stats[0] = tree.nodes.size() - tree.tlas_num_nodes;
  ctx->bvh_stats[2] = tree.tlas_num_nodes;
  *num_nodes = tree.nodes.size();
  return 0;
}

// How many nodes of the scene tree's top every ray-kernel workgroup stages in LDS, and the kernels' dynamic LDS.
static int update_ray_kernel_lds(LumContext* ctx, size_t num_nodes) {
  // resident workgroups per CU share the LDS: what the device offers minus a margin, 128 B per node
  hipDeviceProp_t prop;
  HIP_TRY(ctx, hipGetDeviceProperties(&prop, ctx->device));
  size_t lds_bytes = prop.maxSharedMemoryPerMultiProcessor ? prop.maxSharedMemoryPerMultiProcessor : prop.sharedMemPerBlock;
  // the ray kernels are compiled for 128 VGPRs: 4 waves per SIMD = 16 waves per CU = one workgroup of kTraceBlock = 1024 threads (both flavours since round 4)
  lds_bytes = std::min<size_t>(lds_bytes, 160 * 1024);
  lds_bytes = lds_bytes > 16384 ? lds_bytes - 8192 : 0;  // margin: the ray kernels' static LDS (the staged top-level leaf records) and the runtime's own
  lds_bytes = lds_bytes > LUM_LDS_STACK_BYTES ? lds_bytes - LUM_LDS_STACK_BYTES : 0;  // the stacks' share (dev_trace.h, TraversalStack)
  ctx->lds_nodes = (uint32_t) std::min<size_t>(lds_bytes / kNodeBytes, num_nodes);
  if (const char* e = getenv("LUM_LDS_NODES")) ctx->lds_nodes = std::min<uint32_t>((uint32_t) atoi(e), ctx->lds_nodes);
  ctx->trace_blocks = (uint32_t) prop.multiProcessorCount;  // one workgroup of kTraceBlock threads per CU
  // The attribute is a property of the kernel, not of a context: it is set to what the largest scene may ask for (the whole budget computed
  // above), never to this scene's need - a second context with a small scene must not lower the cap a first one launches with.
  const size_t dyn = lds_bytes + LUM_LDS_STACK_BYTES;
  HIP_TRY(ctx, (hipError_t) wavefront_kernels_exact()->set_ray_kernel_lds(dyn));
  HIP_TRY(ctx, (hipError_t) wavefront_kernels_fast()->set_ray_kernel_lds(dyn));
  return 0;
}

// Light-only BVH (world-space triangles; reference: optix_bvh.c:382-478), in the light tree's group.
static int update_light_bvh(LumContext* ctx, const LumDeviceSceneView* v) {
  DeviceScene& sc = ctx->scene;
  const uint32_t nl = (v->light_tree_root && v->light_bvh_tris) ? v->num_lights : 0;
  std::vector<Aabb> boxes(nl);
  for (uint32_t l = 0; l < nl; l++) { const float* p = v->light_bvh_tris + (size_t) l * 12; boxes[l] = tri_box(p, p + 4, p + 8); }
  Bvh4 lb = build_bvh4(boxes.data(), nl, kBvhLeafMaxTri, 40);
  if (lb.nodes.empty()) { ctx->error = "light BVH exceeds 40 levels"; return 1; }
  std::vector<BvhTri> tris(nl ? nl : 1, BvhTri{});
  for (uint32_t i = 0; i < nl; i++) tris[i] = bvh_tri(v->light_bvh_tris + (size_t) lb.prims[i] * 12, lb.prims[i], 0u, 0u);
  if (upload(ctx, LumContext::kGrpLight, lb.nodes.data(), lb.nodes.size(), &sc.light_nodes)) return 1;
  if (upload(ctx, LumContext::kGrpLight, tris.data(), tris.size(), &sc.light_tris)) return 1;
  sc.light_num_nodes = (uint32_t) lb.nodes.size();
  ctx->bvh_stats[3] = lb.nodes.size();
  return 0;
}

constexpr unsigned kDirtyTrianglesRewritten = 1u << 30;  // scene_update's own: a LUMC_DIRTY_MESH_POSITIONS update built a mesh again, its traversal triangles are new

// The counts, then what two kernels derive from the arrays above: k_tri_opacity (needs the materials and blas_tris), k_light_table (needs the counts).
static int update_counts_and_tables(LumContext* ctx, const LumDeviceSceneView* v, unsigned dirty) {
  DeviceScene& sc = ctx->scene;
  const uint32_t total_tris = total_triangles(v);
  const bool dirty_lights = (dirty & LUMC_DIRTY_LIGHTS) != 0;
  ctx->bvh_stats[1] = total_tris;
  sc.num_meshes = v->num_meshes; sc.num_instances = v->num_instances; sc.num_materials = v->num_materials; sc.num_lights = v->num_lights;  // (num_textures: update_textures)
  if (total_tris && (dirty & (LUMC_DIRTY_MESHES | LUMC_DIRTY_MATERIALS | kDirtyTrianglesRewritten))) {  // the triangles' material words: texture id, or whether they stop a visibility ray on their own
    hipLaunchKernelGGL(k_tri_opacity, dim3((total_tris + kBlock - 1) / kBlock), dim3(kBlock), 0, 0, sc, const_cast<BvhTri*>(sc.blas_tris), total_tris);
    HIP_TRY(ctx, hipGetLastError());
  }
  if ((dirty_lights || ((dirty & (LUMC_DIRTY_MATERIALS | LUMC_DIRTY_INSTANCES | LUMC_DIRTY_MESHES)) && sc.light_tri_table)) && sc.light_tree_root && sc.num_lights) {  // the emissive triangles in world space with what their material says, one record per light (load_tri_light_table)
    float4* table = const_cast<float4*>(sc.light_tri_table);  // a material edit alone refills the table in place (same lights)
    if (dirty_lights) {
      DeviceBuffer<char> records;
      HIP_TRY(ctx, records.resize(sizeof(float4) * 4 * (size_t) sc.num_lights));
      table = (float4*) records.get();
      ctx->scene_allocs[LumContext::kGrpLight].push_back(std::move(records));
    }
    hipLaunchKernelGGL(k_light_table, dim3((sc.num_lights + kBlock - 1) / kBlock), dim3(kBlock), 0, 0, sc, table);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipDeviceSynchronize());
    sc.light_tri_table = table;
  }
  return 0;
}

// The scalar fields of the constants' part, with the pointers of that part reset (the functions after this one fill them in again).
static int copy_constants(LumContext* ctx, const LumDeviceSceneView* v) {
  DeviceScene& sc = ctx->scene;
  sc.width = v->width; sc.height = v->height; sc.max_ray_depth = v->max_ray_depth; sc.shading_mode = v->shading_mode;
  std::memcpy(sc.cam_pos, v->cam_pos, sizeof(sc.cam_pos));
  std::memcpy(sc.cam_rotation, v->cam_rotation, sizeof(sc.cam_rotation));
  sc.cam_fov = v->cam_fov; sc.cam_aperture_size = v->cam_aperture_size; sc.cam_object_distance = v->cam_object_distance;
  sc.cam_scale = v->cam_scale; sc.cam_rr_threshold = v->cam_rr_threshold;
  sc.cam_aperture_shape = v->cam_aperture_shape; sc.cam_aperture_blade_count = v->cam_aperture_blade_count;
  sc.sky_mode = v->sky_mode;
  std::memcpy(sc.sky_constant_color, v->sky_constant_color, sizeof(sc.sky_constant_color));
  sc.sky_steps = v->sky_steps; sc.sky_ozone_absorption = v->sky_ozone_absorption;
  std::memcpy(sc.sky_geometry_offset, v->sky_geometry_offset, sizeof(sc.sky_geometry_offset));
  sc.sky_sun_strength = v->sky_sun_strength; sc.sky_base_density = v->sky_base_density; sc.sky_rayleigh_density = v->sky_rayleigh_density;
  sc.sky_mie_density = v->sky_mie_density; sc.sky_ozone_density = v->sky_ozone_density; sc.sky_rayleigh_falloff = v->sky_rayleigh_falloff;
  sc.sky_mie_falloff = v->sky_mie_falloff; sc.sky_ground_visibility = v->sky_ground_visibility; sc.sky_ozone_layer_thickness = v->sky_ozone_layer_thickness;
  sc.sky_multiscattering_factor = v->sky_multiscattering_factor;
  std::memcpy(sc.sky_sun_pos, v->sky_sun_pos, sizeof(sc.sky_sun_pos));
  std::memcpy(sc.sky_mie_phase, v->sky_mie_phase, sizeof(sc.sky_mie_phase));
  std::memcpy(sc.sky_moon_pos, v->sky_moon_pos, sizeof(sc.sky_moon_pos));
  sc.sky_moon_tex_offset = v->sky_moon_tex_offset; sc.sky_stars_intensity = v->sky_stars_intensity;
  sc.sky_moon_albedo_tex = v->sky_moon_albedo_tex; sc.sky_moon_normal_tex = v->sky_moon_normal_tex;
  sc.sky_stars_count = 0; sc.sky_stars = nullptr; sc.sky_stars_offsets = nullptr;
  sc.sky_lut_transmittance = nullptr; sc.sky_lut_multiscattering = nullptr;
  sc.sky_hdri = nullptr; sc.sky_hdri_dim = 0;
  sc.sky_aerial_perspective = v->sky_aerial_perspective;
  // ---- fog ----
  sc.fog_active = v->fog_active ? 1u : 0u;
  sc.fog_density = v->fog_density; sc.fog_dist = v->fog_dist; sc.fog_height = v->fog_height;
  std::memcpy(sc.fog_phase, v->fog_phase, sizeof(sc.fog_phase));
  sc.bridge_max_num_vertices = v->bridge_max_num_vertices;
  if (sc.fog_active && !(sc.fog_density > 0.0f)) { ctx->error = "lumc_scene_upload: fog needs a positive density"; return 1; }
  // ---- ocean ----
  sc.ocean_active = v->ocean_active ? 1u : 0u;
  sc.ocean_height = v->ocean_height; sc.ocean_amplitude = v->ocean_amplitude; sc.ocean_frequency = v->ocean_frequency;
  sc.ocean_refractive_index = v->ocean_refractive_index;
  std::memcpy(sc.ocean_scattering, v->ocean_scattering, sizeof(sc.ocean_scattering));
  std::memcpy(sc.ocean_absorption, v->ocean_absorption, sizeof(sc.ocean_absorption));
  sc.ocean_molecular_weight = v->ocean_molecular_weight;
  sc.ocean_caustics_active = v->ocean_caustics_active ? 1u : 0u;
  sc.ocean_caustics_ris_sample_count = v->ocean_caustics_ris_sample_count;
  sc.ocean_caustics_domain_scale = v->ocean_caustics_domain_scale;
  sc.ocean_multiscattering = v->ocean_multiscattering ? 1u : 0u;
  sc.ocean_triangle_light_contribution = v->ocean_triangle_light_contribution ? 1u : 0u;
  if (sc.ocean_active && !(sc.ocean_refractive_index >= 1.0f)) { ctx->error = "lumc_scene_upload: the ocean needs a refractive index of at least 1"; return 1; }
  // ---- clouds ----
  sc.cloud_active = v->cloud_active ? 1u : 0u;
  sc.cloud_atmosphere_scattering = v->cloud_atmosphere_scattering ? 1u : 0u;
  sc.cloud_steps = v->cloud_steps & 0x3FFu; sc.cloud_shadow_steps = v->cloud_shadow_steps & 0x3FFu; sc.cloud_octaves = v->cloud_octaves & 0xFu;  // DeviceCloud's bit fields
  sc.cloud_offset_x = v->cloud_offset_x; sc.cloud_offset_z = v->cloud_offset_z; sc.cloud_density = v->cloud_density;
  sc.cloud_noise_shape_scale = v->cloud_noise_shape_scale; sc.cloud_noise_detail_scale = v->cloud_noise_detail_scale; sc.cloud_noise_weather_scale = v->cloud_noise_weather_scale;
  std::memcpy(sc.cloud_phase, v->cloud_phase, sizeof(sc.cloud_phase));
  std::memcpy(sc.cloud_layers, v->cloud_layers, sizeof(sc.cloud_layers));
  sc.cloud_noise_shape = nullptr; sc.cloud_noise_detail = nullptr; sc.cloud_noise_weather = nullptr;
  if (sc.cloud_active && (sc.cloud_steps == 0 || sc.cloud_shadow_steps == 0)) { ctx->error = "lumc_scene_upload: clouds need positive step counts"; return 1; }
  // ---- particles ----
  sc.particles_active = (v->particles_active && v->particles_count) ? 1u : 0u;
  sc.particles_count = sc.particles_active ? v->particles_count : 0u;
  sc.particles_scale = v->particles_scale; sc.particles_speed = v->particles_speed;
  std::memcpy(sc.particles_albedo, v->particles_albedo, sizeof(sc.particles_albedo));
  std::memcpy(sc.particles_direction, v->particles_direction, sizeof(sc.particles_direction));
  std::memcpy(sc.particles_phase, v->particles_phase, sizeof(sc.particles_phase));
  return 0;
}

static int update_stars(LumContext* ctx, const LumDeviceSceneView* v) {
  DeviceScene& sc = ctx->scene;
  if (!v->sky_stars || !v->sky_stars_offsets || !v->sky_stars_count) return 0;
  if (upload(ctx, LumContext::kGrpConst, (const float4*) v->sky_stars, (size_t) v->sky_stars_count, &sc.sky_stars)) return 1;
  if (upload(ctx, LumContext::kGrpConst, v->sky_stars_offsets, (size_t) 64 * 32 + 1, &sc.sky_stars_offsets)) return 1;
  sc.sky_stars_count = v->sky_stars_count;
  return 0;
}

// The clouds' noise textures: the caller's three, or the context's own (ensure_cloud_noise).
static int update_cloud_noise(LumContext* ctx, const LumDeviceSceneView* v) {
  DeviceScene& sc = ctx->scene;
  if (!sc.cloud_active) return 0;
  if (v->cloud_noise_shape && v->cloud_noise_detail && v->cloud_noise_weather) {
    if (upload(ctx, LumContext::kGrpConst, (const uint32_t*) v->cloud_noise_shape, kCloudNoiseTexels[0], &sc.cloud_noise_shape)) return 1;
    if (upload(ctx, LumContext::kGrpConst, (const uint32_t*) v->cloud_noise_detail, kCloudNoiseTexels[1], &sc.cloud_noise_detail)) return 1;
    return upload(ctx, LumContext::kGrpConst, (const uint32_t*) v->cloud_noise_weather, kCloudNoiseTexels[2], &sc.cloud_noise_weather);
  }
  if (ensure_cloud_noise(ctx, v->cloud_seed)) return 1;
  sc.cloud_noise_shape = ctx->d_cloud_noise[0].get(); sc.cloud_noise_detail = ctx->d_cloud_noise[1].get(); sc.cloud_noise_weather = ctx->d_cloud_noise[2].get();
  return 0;
}

static int update_particles(LumContext* ctx, const LumDeviceSceneView* v) {
  ctx->scene_allocs[LumContext::kGrpPart].clear();
  return build_particle_tree(ctx, LumContext::kGrpPart, v, ctx->scene);
}

// Sky look-up tables: the caller's or generated here (device/device_sky.c:64-200); not for a constant sky (HDRI mode bakes from them and samples the sun through them).
static int update_sky_tables(LumContext* ctx, const LumDeviceSceneView* v) {
  DeviceScene& sc = ctx->scene;
  if (sc.sky_mode == kSkyConstantColor) return 0;
  const size_t tm_texels = 2 * (size_t) kSkyTmWidth * kSkyTmHeight, ms_texels = 2 * (size_t) kSkyMsSize * kSkyMsSize;
  if (v->sky_lut_transmittance && v->sky_lut_multiscattering) {
    if (upload(ctx, LumContext::kGrpConst, (const float4*) v->sky_lut_transmittance, tm_texels, &sc.sky_lut_transmittance)) return 1;
    if (upload(ctx, LumContext::kGrpConst, (const float4*) v->sky_lut_multiscattering, ms_texels, &sc.sky_lut_multiscattering)) return 1;
    ctx->sky_lut_key.clear();
    return 0;
  }
  // the two tables are functions of the atmosphere's parameters alone (sky.cuh:110-176, :186-332): a camera move or a sun move keeps them
  std::vector<uint32_t> key;
  auto put = [&](const void* p, size_t bytes) { const size_t at = key.size(); key.resize(at + (bytes + 3) / 4, 0u); std::memcpy(key.data() + at, p, bytes); };
  put(&sc.sky_ozone_absorption, sizeof(sc.sky_ozone_absorption));
  const float params[] = {sc.sky_base_density, sc.sky_rayleigh_density, sc.sky_mie_density, sc.sky_ozone_density, sc.sky_rayleigh_falloff, sc.sky_mie_falloff,
                          sc.sky_ground_visibility, sc.sky_ozone_layer_thickness, sc.sky_multiscattering_factor, sc.sky_sun_strength};
  put(params, sizeof(params)); put(sc.sky_mie_phase, sizeof(sc.sky_mie_phase)); put(sc.sky_sun_pos, sizeof(sc.sky_sun_pos)); put(sc.sky_geometry_offset, sizeof(sc.sky_geometry_offset));
  if (!ctx->d_sky_lut[0]) {
    HIP_TRY(ctx, ctx->d_sky_lut[0].resize(tm_texels));
    HIP_TRY(ctx, ctx->d_sky_lut[1].resize(ms_texels));
    ctx->sky_lut_key.clear();
  }
  if (key != ctx->sky_lut_key) {
    hipLaunchKernelGGL(k_sky_transmittance_lut, dim3((kSkyTmWidth * kSkyTmHeight + 63) / 64), dim3(64), 0, 0, sc, ctx->d_sky_lut[0].get());
    sc.sky_lut_transmittance = ctx->d_sky_lut[0].get();  // the multiscattering integration reads the finished transmittance table
    hipLaunchKernelGGL(k_sky_multiscattering_lut, dim3(kSkyMsSize, kSkyMsSize), dim3(kSkyMsIter), 0, 0, sc, ctx->d_sky_lut[1].get());
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipDeviceSynchronize());
    ctx->sky_lut_key = key;
  }
  sc.sky_lut_transmittance = ctx->d_sky_lut[0].get();
  sc.sky_lut_multiscattering = ctx->d_sky_lut[1].get();
  return 0;
}

// BSDF energy tables: taken from the caller or generated here (device/device_bsdf.c:64-130).
static int update_bsdf_tables(LumContext* ctx, const LumDeviceSceneView* v, bool full_upload) {
  DeviceScene& sc = ctx->scene;
  const uint16_t* host_luts[4] = {v->lut_conductor, v->lut_glossy, v->lut_dielectric, v->lut_dielectric_inv};
  const bool have_luts = bool(ctx->d_luts[0]);
  for (int t = 0; t < 4 && !have_luts; t++) HIP_TRY(ctx, ctx->d_luts[t].resize(kBsdfLutCount[t]));
  if (have_luts && !full_upload) { /* a partial update keeps the tables the context renders with */ }
  else if (host_luts[0] && host_luts[1] && host_luts[2] && host_luts[3]) {
    for (int t = 0; t < 4; t++) HIP_TRY(ctx, hipMemcpy(ctx->d_luts[t].get(), host_luts[t], sizeof(uint16_t) * kBsdfLutCount[t], hipMemcpyHostToDevice));
  }
  else {
    // The tables are a function of the embedded blue-noise mask alone (65 536 samples per texel, one thread per texel: 0.29 s of GPU time):
    // generated once per process, every later upload copies them.
    static std::mutex lut_mutex;
    static std::vector<uint16_t> lut_cache[4];
    static std::vector<uint32_t> lut_cache_mask;
    std::lock_guard<std::mutex> lock(lut_mutex);
    const bool cached = !lut_cache[0].empty() && lut_cache_mask.size() == 65536 && std::memcmp(lut_cache_mask.data(), v->bluenoise_2d, sizeof(uint32_t) * 65536) == 0;
    if (cached) {
      for (int t = 0; t < 4; t++) HIP_TRY(ctx, hipMemcpy(ctx->d_luts[t].get(), lut_cache[t].data(), sizeof(uint16_t) * kBsdfLutCount[t], hipMemcpyHostToDevice));
    }
    else {
      // the two big tables and the conductor table are independent: side by side on three streams; the glossy table divides by the conductor's
      hipStream_t streams[3];
      for (auto& st : streams) HIP_TRY(ctx, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
      const int first_wave[3] = {0, 2, 3};
      for (int k = 0; k < 3; k++) {
        const int t = first_wave[k];
        hipLaunchKernelGGL(k_generate_lut, dim3((kBsdfLutCount[t] + 63) / 64), dim3(64), 0, streams[k], sc.bluenoise_2d, t, kBsdfLutCount[t], ctx->d_luts[0].get(), ctx->d_luts[t].get());
      }
      hipLaunchKernelGGL(k_generate_lut, dim3((kBsdfLutCount[1] + 63) / 64), dim3(64), 0, streams[0], sc.bluenoise_2d, 1, kBsdfLutCount[1], ctx->d_luts[0].get(), ctx->d_luts[1].get());
      HIP_TRY(ctx, hipGetLastError());
      for (auto& st : streams) { HIP_TRY(ctx, hipStreamSynchronize(st)); (void) hipStreamDestroy(st); }
      for (int t = 0; t < 4; t++) {
        lut_cache[t].resize(kBsdfLutCount[t]);
        HIP_TRY(ctx, hipMemcpy(lut_cache[t].data(), ctx->d_luts[t].get(), sizeof(uint16_t) * kBsdfLutCount[t], hipMemcpyDeviceToHost));
      }
      lut_cache_mask.assign(v->bluenoise_2d, v->bluenoise_2d + 65536);
    }
  }
  sc.lut_conductor = ctx->d_luts[0].get(); sc.lut_glossy = ctx->d_luts[1].get(); sc.lut_dielectric = ctx->d_luts[2].get(); sc.lut_dielectric_inv = ctx->d_luts[3].get();
  return 0;
}

// Sky panorama (HDRI mode): the caller's, or baked here from the procedural sky as the reference's device manager does when the sky changes
// (device_manager.c:351-366, device_sky.c:249-366); lumc_sky_hdri_build re-bakes on request.
static int update_sky_panorama(LumContext* ctx, const LumDeviceSceneView* v) {
  DeviceScene& sc = ctx->scene;
  if (sc.sky_mode != kSkyHdri) return 0;
  if (v->sky_hdri && v->sky_hdri_dim) {
    if (upload(ctx, LumContext::kGrpConst, (const float4*) v->sky_hdri, (size_t) v->sky_hdri_dim * v->sky_hdri_dim, &sc.sky_hdri)) return 1;
    sc.sky_hdri_dim = v->sky_hdri_dim;
    return 0;
  }
  ctx->has_scene = true;  // the bake renders this scene's sky
  if (lumc_sky_hdri_build(ctx, v->sky_hdri_origin, v->sky_hdri_dim, v->sky_hdri_samples ? v->sky_hdri_samples : 1u)) { ctx->has_scene = false; return 1; }
  return 0;
}

// Camera, settings, sky, fog, ocean, clouds, particles: the kernels' scalar arguments and the tables derived from them.
static int update_constants(LumContext* ctx, const LumDeviceSceneView* v, unsigned dirty) {
  ctx->scene_allocs[LumContext::kGrpConst].clear();
  if (copy_constants(ctx, v)) return 1;
  if (update_stars(ctx, v)) return 1;
  if (update_cloud_noise(ctx, v)) return 1;
  if ((dirty & LUMC_DIRTY_PARTICLES) && update_particles(ctx, v)) return 1;
  if (update_sky_tables(ctx, v)) return 1;
  if (update_bsdf_tables(ctx, v, dirty == LUMC_DIRTY_ALL)) return 1;
  return update_sky_panorama(ctx, v);
}

// Bridges to emissive triangles (fog, or an ocean with triangle_light_contribution): the vertex-count table. Decided after EVERY update, not only when
// the constants are dirty: a material that becomes emissive (MATERIALS | LIGHTS) gives a fogged scene its first light, and bridges_vertex_count_importance
// reads the table without a check. The table lives in the context (5 KB, uploaded once per content).
static int update_bridge_table(LumContext* ctx, const LumDeviceSceneView* v) {
  DeviceScene& sc = ctx->scene;
  sc.bridge_lut = nullptr;
  if (!((sc.fog_active || (sc.ocean_active && sc.ocean_triangle_light_contribution)) && sc.num_lights > 0 && sc.light_tree_root)) return 0;
  if (!v->bridge_lut) { ctx->error = sc.fog_active ? "lumc_scene_upload: fog with emissive triangles needs bridge_lut" : "lumc_scene_upload: an ocean lit by emissive triangles needs bridge_lut"; return 1; }
  if (sc.bridge_max_num_vertices == 0) { ctx->error = "lumc_scene_upload: bridge_max_num_vertices must be at least 1"; return 1; }
  const size_t n = (size_t) 64 * 21;
  if (!ctx->d_bridge_lut || ctx->bridge_lut_host.size() != n || std::memcmp(ctx->bridge_lut_host.data(), v->bridge_lut, n * sizeof(float)) != 0) {
    if (!ctx->d_bridge_lut) HIP_TRY(ctx, ctx->d_bridge_lut.resize(n));
    HIP_TRY(ctx, hipMemcpy(ctx->d_bridge_lut.get(), v->bridge_lut, n * sizeof(float), hipMemcpyHostToDevice));
    ctx->bridge_lut_host.assign(v->bridge_lut, v->bridge_lut + n);
  }
  sc.bridge_lut = ctx->d_bridge_lut.get();
  return 0;
}

// The scene on the device: the dirty parts, in the order their kernels and uploads depend on. Until the update has gone through the context has no scene.
static int scene_update(LumContext* ctx, const LumDeviceSceneView* v, unsigned dirty) {
  ctx->guides_valid = false;  // the denoiser's guides were rendered from the scene as it was
  DeviceScene& sc = ctx->scene;
  if (!v->bluenoise_2d) { ctx->error = "scene has no blue-noise mask"; return 1; }
  if (v->max_ray_depth > 63) { ctx->error = "max_ray_depth exceeds 63 (6-bit field, device_structs.h:9)"; return 1; }
  if (dirty & LUMC_DIRTY_MESHES) dirty &= ~(unsigned) LUMC_DIRTY_MESH_POSITIONS;  // a full rebuild of the meshes covers moved vertices
  if (dirty & (LUMC_DIRTY_MESHES | LUMC_DIRTY_MESH_POSITIONS)) dirty |= LUMC_DIRTY_INSTANCES;  // the assembled node array holds the per-mesh trees
  if (dirty & LUMC_DIRTY_PARTICLES) dirty |= LUMC_DIRTY_CONSTANTS;
  const bool meshes = (dirty & LUMC_DIRTY_MESHES) != 0, instances = (dirty & LUMC_DIRTY_INSTANCES) != 0, lights = (dirty & LUMC_DIRTY_LIGHTS) != 0;
  ctx->has_scene = false;
  if (meshes && update_mesh_arrays(ctx, v)) return 1;
  if (dirty & LUMC_DIRTY_MESH_POSITIONS) {
    bool rebuilt = false;
    if (refit_mesh_trees(ctx, v, &rebuilt)) return 1;
    if (rebuilt) dirty |= kDirtyTrianglesRewritten;
  }
  if (instances && update_instance_arrays(ctx, v)) return 1;
  if ((dirty & LUMC_DIRTY_MATERIALS) && update_materials(ctx, v)) return 1;
  const bool time_lights = (dirty & LUMC_DIRTY_MESH_POSITIONS) != 0;
  auto lights_since = [&](std::chrono::steady_clock::time_point t) { if (time_lights) ctx->refit_stats.seconds_lights += std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count(); };
  auto t_lights = std::chrono::steady_clock::now();
  if (lights && update_light_tree(ctx, v)) return 1;
  lights_since(t_lights);
  if (!sc.bluenoise_2d && upload(ctx, LumContext::kGrpOnce, v->bluenoise_2d, 65536, &sc.bluenoise_2d)) return 1;
  if ((dirty & LUMC_DIRTY_TEXTURES) && update_textures(ctx, v)) return 1;
  size_t num_nodes = 0;
  const auto t_assemble = std::chrono::steady_clock::now();
  if (instances && (update_scene_tree(ctx, v, meshes, &num_nodes) || update_ray_kernel_lds(ctx, num_nodes))) return 1;
  if (dirty & LUMC_DIRTY_MESH_POSITIONS) ctx->refit_stats.seconds_assemble = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_assemble).count();
  t_lights = std::chrono::steady_clock::now();
  if (lights && update_light_bvh(ctx, v)) return 1;
  if (update_counts_and_tables(ctx, v, dirty)) return 1;
  lights_since(t_lights);
  if ((dirty & LUMC_DIRTY_CONSTANTS) && update_constants(ctx, v, dirty)) return 1;
  if (update_bridge_table(ctx, v)) return 1;
  // the moon's texture ids follow the texture pool (the host layer appends the two moon textures behind the scene's own): an added texture moves them
  sc.sky_moon_albedo_tex = v->sky_moon_albedo_tex; sc.sky_moon_normal_tex = v->sky_moon_normal_tex;
  ctx->has_scene = true;
  return 0;
}

int lumc_scene_upload(LumContext* ctx, const LumDeviceSceneView* v) {
  if (!ctx || !v) return 1;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  free_scene(ctx);
  std::memset(&ctx->scene, 0, sizeof(ctx->scene));
  return scene_update(ctx, v, LUMC_DIRTY_ALL);
}

int lumc_scene_update(LumContext* ctx, const LumDeviceSceneView* v, unsigned int dirty) {
  if (!ctx || !v) return 1;
  if (!ctx->has_scene || (dirty & LUMC_DIRTY_ALL) == LUMC_DIRTY_ALL) return lumc_scene_upload(ctx, v);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipDeviceSynchronize());  // nothing renders from the arrays that are about to be freed
  if (scene_update(ctx, v, dirty & (LUMC_DIRTY_ALL | LUMC_DIRTY_MESH_POSITIONS))) { free_scene(ctx); return 1; }  // a failed partial update leaves no half-updated scene behind
  return 0;
}

int lumc_set_mesh_refit(LumContext* ctx, uint32_t mode, float max_cost_growth) {
  if (!ctx) return 1;
  if (mode > 1 || !(max_cost_growth >= 0.0f) || !std::isfinite(max_cost_growth)) { ctx->error = "lumc_set_mesh_refit: mode is 0 or 1, max_cost_growth >= 0"; return 1; }
  ctx->refit_mode = mode; ctx->refit_max_cost_growth = max_cost_growth;
  return 0;
}

int lumc_mesh_refit_stats(const LumContext* ctx, LumMeshRefitStats* out) {
  if (!ctx || !out) return 1;
  *out = ctx->refit_stats;
  return 0;
}

int lumc_download_luts(LumContext* ctx, uint16_t* conductor, uint16_t* glossy, uint16_t* dielectric, uint16_t* dielectric_inv) {
  if (!ctx || !ctx->has_scene) return 1;
  uint16_t* dst[4] = {conductor, glossy, dielectric, dielectric_inv};
  for (int t = 0; t < 4; t++)
    if (dst[t]) HIP_TRY(ctx, hipMemcpy(dst[t], ctx->d_luts[t].get(), sizeof(uint16_t) * kBsdfLutCount[t], hipMemcpyDeviceToHost));
  return 0;
}

int lumc_download_sky_luts(LumContext* ctx, float* transmittance, float* multiscattering) {
  if (!ctx || !ctx->has_scene || !ctx->scene.sky_lut_transmittance) { if (ctx) ctx->error = "lumc_download_sky_luts: the scene has no procedural sky"; return 1; }
  if (transmittance) HIP_TRY(ctx, hipMemcpy(transmittance, ctx->scene.sky_lut_transmittance, sizeof(float4) * 2 * kSkyTmWidth * kSkyTmHeight, hipMemcpyDeviceToHost));
  if (multiscattering) HIP_TRY(ctx, hipMemcpy(multiscattering, ctx->scene.sky_lut_multiscattering, sizeof(float4) * 2 * kSkyMsSize * kSkyMsSize, hipMemcpyDeviceToHost));
  return 0;
}

// Everything the bake reads: the sky's parameters (not its tables: they are functions of the parameters), the star field's size, the moon.
static std::vector<uint32_t> sky_hdri_key(const DeviceScene& sc, uint32_t ctx_cloud_seed, const float origin[3], uint32_t dim, uint32_t samples) {
  std::vector<uint32_t> key;
  auto put = [&](const void* p, size_t bytes) { const size_t at = key.size(); key.resize(at + (bytes + 3) / 4, 0u); std::memcpy(key.data() + at, p, bytes); };
  put(&sc.sky_steps, sizeof(sc.sky_steps)); put(&sc.sky_ozone_absorption, sizeof(sc.sky_ozone_absorption));
  put(sc.sky_geometry_offset, sizeof(sc.sky_geometry_offset));
  const float params[] = {sc.sky_sun_strength, sc.sky_base_density, sc.sky_rayleigh_density, sc.sky_mie_density, sc.sky_ozone_density, sc.sky_rayleigh_falloff, sc.sky_mie_falloff,
                          sc.sky_ground_visibility, sc.sky_ozone_layer_thickness, sc.sky_multiscattering_factor, sc.sky_moon_tex_offset, sc.sky_stars_intensity};
  put(params, sizeof(params));
  put(sc.sky_sun_pos, sizeof(sc.sky_sun_pos)); put(sc.sky_mie_phase, sizeof(sc.sky_mie_phase)); put(sc.sky_moon_pos, sizeof(sc.sky_moon_pos));
  put(&sc.sky_stars_count, sizeof(sc.sky_stars_count));
  put(&sc.cloud_active, sizeof(sc.cloud_active));
  if (sc.cloud_active) {  // the clouds are baked in (sky_hdri.cuh:88-92)
    const uint32_t ints[] = {sc.cloud_atmosphere_scattering, sc.cloud_steps, sc.cloud_shadow_steps, sc.cloud_octaves};
    const float floats[] = {sc.cloud_offset_x, sc.cloud_offset_z, sc.cloud_density, sc.cloud_noise_shape_scale, sc.cloud_noise_detail_scale, sc.cloud_noise_weather_scale};
    put(ints, sizeof(ints)); put(floats, sizeof(floats)); put(sc.cloud_phase, sizeof(sc.cloud_phase)); put(sc.cloud_layers, sizeof(sc.cloud_layers));
    const uint64_t tex[] = {(uint64_t) (uintptr_t) sc.cloud_noise_shape, (uint64_t) (uintptr_t) sc.cloud_noise_weather, (uint64_t) ctx_cloud_seed};
    put(tex, sizeof(tex));
  }
  put(origin, 3 * sizeof(float)); put(&dim, sizeof(dim)); put(&samples, sizeof(samples));
  return key;
}

int lumc_sky_hdri_build(LumContext* ctx, const float origin[3], uint32_t dim, uint32_t samples) {
  if (!ctx || !origin || !ctx->has_scene || !ctx->scene.sky_lut_transmittance) { if (ctx) ctx->error = "lumc_sky_hdri_build: the scene has no atmosphere (constant-colour sky)"; return 1; }
  if (dim < 2 || dim > 16384 || samples == 0) { ctx->error = "lumc_sky_hdri_build: dim must be in [2, 16384] and samples positive"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::vector<uint32_t> key = sky_hdri_key(ctx->scene, ctx->cloud_noise_seed, origin, dim, samples);
  if (ctx->d_sky_hdri && key == ctx->sky_hdri_key) {
    if (ctx->scene.sky_mode == kSkyHdri) { ctx->scene.sky_hdri = ctx->d_sky_hdri.get(); ctx->scene.sky_hdri_dim = dim; }
    return 0;
  }
  ctx->sky_hdri_key.clear();
  if (ctx->d_sky_hdri.count() != (size_t) dim * dim) HIP_TRY(ctx, ctx->d_sky_hdri.resize((size_t) dim * dim));
  ctx->sky_hdri_dim = dim;
  const uint64_t threads = (uint64_t) dim * dim * 32u;
  hipLaunchKernelGGL(k_sky_hdri, dim3((uint32_t) ((threads + 255) / 256)), dim3(256), 0, 0, ctx->scene, origin[0], origin[1], origin[2], dim, samples, ctx->d_sky_hdri.get());
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipDeviceSynchronize());
  ctx->sky_hdri_key = std::move(key);
  if (ctx->scene.sky_mode == kSkyHdri) { ctx->scene.sky_hdri = ctx->d_sky_hdri.get(); ctx->scene.sky_hdri_dim = dim; }
  return 0;
}

int lumc_sky_hdri_download(LumContext* ctx, float* rgba, uint32_t* dim) {
  if (!ctx || !ctx->d_sky_hdri) { if (ctx) ctx->error = "lumc_sky_hdri_download: no baked sky"; return 1; }
  if (dim) *dim = ctx->sky_hdri_dim;
  if (rgba) HIP_TRY(ctx, hipMemcpy(rgba, ctx->d_sky_hdri.get(), sizeof(float4) * (size_t) ctx->sky_hdri_dim * ctx->sky_hdri_dim, hipMemcpyDeviceToHost));
  return 0;
}

// FNV-1a over a pixel list (null: 0, 1, 2 ... n - 1): the identity of a context's pixel set and of its ORDER
uint64_t pixel_list_hash(const uint32_t* pixels, uint32_t n) {
  uint64_t h = 1469598103934665603ull;
  for (uint32_t i = 0; i < n; i++) { h ^= pixels ? pixels[i] : i; h *= 1099511628211ull; }
  return h;
}

int lumc_set_pixels(LumContext* ctx, const uint32_t* pixels, uint32_t num_pixels) {
  if (!ctx || !ctx->has_scene) { if (ctx) ctx->error = "lumc_set_pixels: no scene"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!pixels) num_pixels = ctx->scene.width * ctx->scene.height;
  ctx->adaptive = LumContext::Adaptive();
  ctx->d_pixels.reset(); ctx->d_first_moment.reset(); ctx->d_second_moment.reset();
  ctx->num_pixels = num_pixels;
  ctx->pixels_hash = pixel_list_hash(pixels, num_pixels);  // what lumc_frame_gather checks the set against (a null list = the frame in row-major order)
  if (num_pixels == 0) return 0;
  HIP_TRY(ctx, ctx->d_pixels.assign(pixels, num_pixels));  // (no list: the frame in row-major order, and no buffer)
  HIP_TRY(ctx, ctx->d_first_moment.resize(3 * (size_t) num_pixels));
  HIP_TRY(ctx, ctx->d_second_moment.resize(num_pixels));
  return lumc_clear_accumulators(ctx);
}

int lumc_clear_accumulators(LumContext* ctx) {
  if (!ctx || !ctx->d_first_moment) return 1;
  HIP_TRY(ctx, hipMemset(ctx->d_first_moment.get(), 0, sizeof(float) * 3 * (size_t) ctx->num_pixels));
  HIP_TRY(ctx, hipMemset(ctx->d_second_moment.get(), 0, sizeof(float) * (size_t) ctx->num_pixels));
  return 0;
}

// The particle pass of the closest-hit kernel: the same traversal on the particle tree (the scene copy carries it in place of the surfaces' tree).
static void trace_particles(LumContext* ctx, hipStream_t stream, const PathQueue& q, uint32_t* ctrl, uint32_t N) {
  DeviceScene tree = ctx->scene;
  tree.bvh_nodes = tree.particle_bvh_nodes; tree.blas_tris = tree.particle_tris; tree.tlas_leaves = tree.particle_leaves; tree.tlas_num_nodes = tree.particle_tlas_num_nodes; tree.tlas_num_leaves = tree.particle_num_leaves;
  Launch l(ctx, stream, LUMC_KERNEL_TRACE);
  ctx->wf->trace_particles(grid_persistent(ctx, N), (size_t) ctx->particle_lds_nodes * kNodeBytes + LUM_LDS_STACK_BYTES, stream, tree, q, ctrl, ctx->particle_lds_nodes);
}

// Does the next pass reuse the closest-hit rays for the ambient visibility (lumc_set_ambient_reuse)? Plain scenes only: with fog the vertex's ambient term
// is dimmed along the packed direction, an ocean ends the ambient ray at the water surface, particles and the ocean replace closest hits after the
// pass that would answer, clouds and the procedural sky have no ambient sample; the reorder of sort mode 3 does not move hit_scene_tri.
static bool ambient_reuse_active(const LumContext* ctx) {
  const DeviceScene& sc = ctx->scene;
  // -1: by flavour. The fast flavour: on. The exact flavour: off - asked for (1), it takes only the answers it can prove for the ambient ray itself
  // (k_resolve_reuse re-tests that ray against the hit's triangle) and stays bit-identical to the oracle, but the proof's gathers cost more than the
  // cheap rays they save (hall: visibility kernel -29 ms, resolve +61 ms per step), so it is not its default.
  const bool wanted = ctx->ambient_reuse < 0 ? (ctx->wf == wavefront_kernels_fast()) : ctx->ambient_reuse != 0;
  return wanted && ctx->has_scene && sc.sky_mode != kSkyDefault && !sc.fog_active && !sc.ocean_active && !sc.particles_active && !sc.cloud_active &&
         !sc.sky_aerial_perspective && ctx->sort.mode == 0 && sc.shading_mode == 0u;
}

// The Sobol / Owen pairs of this pass's sample ids for every dimension k_shade can ask for (dev_sampler.h LUM_SOBOL_TABLE): 1.3 MB at 32 ids and 8 bounces
static void prepare_sobol_table(LumContext* ctx, hipStream_t stream, DeviceScene& sc, uint32_t first_sample, uint32_t sample_count) {
  sc.sobol_table = nullptr;
  if (!(ctx->sobol_table && sample_count > 0 && sample_count <= kSobolTableMaxSamples && sc.shading_mode == 0u)) return;
  const uint32_t stride = (sample_count + 15u) & ~15u, dims = (sc.max_ray_depth + 1u) * kRndTargetCount;
  const size_t entries = (size_t) stride * dims;
  if (ctx->d_sobol.count() < entries && ctx->d_sobol.resize(entries) != hipSuccess) (void) hipGetLastError();  // no room: the sampler hashes
  if (ctx->d_sobol) {
    ctx->wf->sobol_table(stream, ctx->d_sobol.get(), first_sample, sample_count, stride, dims);
    sc.sobol_table = ctx->d_sobol.get(); sc.sobol_first = first_sample; sc.sobol_count = sample_count; sc.sobol_stride = stride;
  }
}

static size_t ray_kernel_lds(const LumContext* ctx) { return (size_t) ctx->lds_nodes * kNodeBytes + LUM_LDS_STACK_BYTES; }
static bool render_volumes(const DeviceScene& sc) { return sc.fog_active || sc.ocean_active; }  // device_manager.c:478

// Debug shading modes: one closest-hit pass and a colour per path (device_renderer.c:136-181)
static void debug_pass(LumContext* ctx, hipStream_t stream, const DeviceScene& sc, uint32_t N) {
  const WavefrontKernels& wf = *ctx->wf;
  {
    Launch l(ctx, stream, LUMC_KERNEL_TRACE);
    wf.trace(grid_persistent(ctx, N), ray_kernel_lds(ctx), stream, sc, ctx->queue[0], nullptr, ctx->d_ctrl.get(), ctx->d_counters.get(), ctx->lds_nodes);
  }
  if (sc.particles_active) trace_particles(ctx, stream, ctx->queue[0], ctx->d_ctrl.get(), N);
  if (sc.ocean_active) {
    Launch l(ctx, stream, LUMC_KERNEL_TRACE);
    wf.trace_ocean(grid_for(N), stream, sc, ctx->queue[0], (const uint32_t*) ctx->d_ctrl.get());
  }
  if (render_volumes(sc)) {  // the debug queue keeps volume_process_events (device_renderer.c:145-147)
    Launch l(ctx, stream, LUMC_KERNEL_VOLUME);
    wf.volume_events(grid_for(N), stream, sc, ctx->queue[0], ctx->volume, ctx->d_results, ctx->d_ctrl.get(), 0u);
  }
  if (sc.sky_aerial_perspective && sc.sky_mode != kSkyConstantColor) {  // the debug queue keeps the in-scattering events (device_renderer.c:150-154)
    Launch l(ctx, stream, LUMC_KERNEL_SKY);
    wf.sky_inscattering(grid_for(N), stream, sc, ctx->queue[0], ctx->d_results, (const uint32_t*) ctx->d_ctrl.get(), 0u);
  }
  Launch l(ctx, stream, LUMC_KERNEL_SHADE);
  wf.shade_debug(grid_for(N), stream, sc, ctx->queue[0], ctx->d_results, (const uint32_t*) ctx->d_ctrl.get());
}

// How the vertices of a depth get their sums (the visibility answers applied to the NEE records):
//   kResolvePlain: k_resolve after the depth's visibility pass.
//   kResolveReuse - ambient-visibility reuse (lumc_set_ambient_reuse; AmbientReuse in kernels.h): the vertices of depth d leave their ambient sample to the
//     closest-hit pass of depth d + 1, which is followed by a second, small visibility pass (what the closest hit could not decide) and only then by the resolve
//     of depth d - still before k_shade of depth d + 1 touches the result slots, so the order of the sums is the usual one.
//   kResolveFused - fused resolve (FusedResolve, kernels.h): with the fast flavour's reuse the resolve of depth d is done by k_shade of depth d + 1 for the
//     vertices an entry continues, by k_resolve_ended for the others; the queues rotate through three buffers and the NEE records through two, so that depth d
//     is intact while depth d + 1 is shaded. The exact flavour's (provable) reuse keeps its own kernel: its sums must land in the reference's order.
enum ResolveScheme { kResolvePlain, kResolveReuse, kResolveFused };

// What one depth reads and writes. Only depth_buffers knows how the queues and record sets rotate.
struct DepthBuffers {
  PathQueue& cur;        // the depth's paths
  PathQueue& next;       // where its shading kernels append the next depth's
  PathQueue& prev;       // the depth before (kResolveReuse, kResolveFused: not yet resolved when this depth is traced)
  NeeQueue& nee;         // the depth's NEE records
  NeeQueue& nee_before;  // the depth before's (kResolveFused)
  uint32_t* ctrl;        // the depth's control words; the depth before's are ctrl - kCtlStride
  const FusedResolve* fused_records;  // kResolveFused: the device record k_shade reads the depth before through
  uint32_t* ended;       // kResolveFused: the list of the depth's vertices that no entry continues
  uint32_t depth, depth_const;
  bool last;             // depth == max_ray_depth
};

static DepthBuffers depth_buffers(LumContext* ctx, ResolveScheme scheme, uint32_t depth, uint32_t max_depth) {
  // (cur == depth % 3 and the record set == depth & 1 below: what the six device records assume)
  const bool fused = scheme == kResolveFused;
  const int cur = fused ? (int) (depth % 3u) : (int) (depth & 1u);
  const int next_q = fused ? (cur + 1) % 3 : (cur ^ 1), prev_q = fused ? (cur + 2) % 3 : (cur ^ 1);
  const bool second_set = fused && (depth & 1u);
  // the sampler's depth constant is not advanced before the last pass (device_renderer.c:126-130)
  const uint32_t depth_const = (depth == max_depth && depth > 0) ? depth - 1 : depth;
  return DepthBuffers{ctx->queue[cur], ctx->queue[next_q], ctx->queue[prev_q], second_set ? ctx->nee2 : ctx->nee, second_set ? ctx->nee : ctx->nee2,
                      ctx->d_ctrl.get() + kCtlStride * depth, fused ? ctx->d_fused + depth % 6u : nullptr, fused ? ctx->d_ended[depth & 1u] : nullptr, depth, depth_const,
                      depth == max_depth};
}

// The closest hits of a depth; with kResolveReuse they also answer the ambient samples of the depth before, which is resolved here.
static int closest_hits(LumContext* ctx, hipStream_t stream, const DeviceScene& sc, ResolveScheme scheme, const DepthBuffers& d, uint32_t N) {
  const WavefrontKernels& wf = *ctx->wf;
  // camera rays leave k_generate in pixel order, which is as coherent as rays get; later depths are sorted on request
  const uint32_t* order = nullptr;
  if (ctx->sort.mode >= 1 && d.depth >= 1 && sort_closest_rays(ctx, stream, d.cur, d.ctrl, N, &order)) return 1;
  {
    Launch l(ctx, stream, LUMC_KERNEL_TRACE);
    wf.trace(grid_persistent(ctx, N), ray_kernel_lds(ctx), stream, sc, d.cur, order, d.ctrl, ctx->d_counters.get(), ctx->lds_nodes);
  }
  if (scheme == kResolveReuse && d.depth > 0) {  // the previous depth's resolve: ambient samples answered by the pass above; what it cannot answer is traced (the control words of the fog's visibility pass: no fog here) and resolved after
    uint32_t* prev = d.ctrl - kCtlStride;
    {
      Launch l(ctx, stream, LUMC_KERNEL_RESOLVE);
      wf.resolve_reuse(grid_for(N), stream, sc, d.prev, d.cur, d.nee, ctx->shadow, ctx->d_results, prev, ctx->d_counters.get());
    }
    {
      Launch l(ctx, stream, LUMC_KERNEL_SHADOW);
      wf.shadow_rays(ctx->trace_blocks, ray_kernel_lds(ctx), stream, sc, ctx->shadow, nullptr, prev + kCtlVolumeShift, ctx->d_counters.get(), ctx->lds_nodes);
    }
    Launch l(ctx, stream, LUMC_KERNEL_RESOLVE);
    wf.resolve_listed(std::min<uint32_t>(grid_for(N), 1024u), stream, sc, d.prev, d.nee, ctx->shadow, ctx->d_results, (const uint32_t*) prev);
  }
  return 0;
}

// What lies between the surfaces: particles, ocean, volumes, clouds, aerial perspective.
static void media_passes(LumContext* ctx, hipStream_t stream, const DeviceScene& sc, const DepthBuffers& d, uint32_t N) {
  const WavefrontKernels& wf = *ctx->wf;
  if (sc.particles_active) trace_particles(ctx, stream, d.cur, d.ctrl, N);  // optix_kernel_raytrace.cu:171
  if (sc.ocean_active) {  // optix_kernel_raytrace.cu:134-144, :172
    Launch l(ctx, stream, LUMC_KERNEL_TRACE);
    wf.trace_ocean(grid_for(N), stream, sc, d.cur, (const uint32_t*) d.ctrl);
  }
  if (render_volumes(sc)) {  // device_renderer.c:64-76: in-scattering with its own visibility pass, then the scattering events
    {
      Launch l(ctx, stream, LUMC_KERNEL_VOLUME);
      wf.volume_inscatter(grid_for(N), stream, sc, d.cur, ctx->volume, ctx->shadow, d.ctrl, d.depth_const);
    }
    {
      Launch l(ctx, stream, LUMC_KERNEL_SHADOW);
      wf.shadow_rays(grid_persistent(ctx, N), ray_kernel_lds(ctx), stream, sc, ctx->shadow, nullptr, d.ctrl + kCtlVolumeShift, ctx->d_counters.get(), ctx->lds_nodes);
    }
    Launch l(ctx, stream, LUMC_KERNEL_VOLUME);
    wf.volume_resolve(grid_for(N), stream, sc, d.cur, ctx->volume, ctx->shadow, ctx->d_results, (const uint32_t*) d.ctrl);
    wf.volume_events(grid_for(N), stream, sc, d.cur, ctx->volume, ctx->d_results, d.ctrl, d.depth_const);
  }
  if (sc.cloud_active && sc.sky_mode == kSkyDefault && sc.cloud_noise_shape) {  // device_manager.c:474, device_renderer.c:78-82
    Launch l(ctx, stream, LUMC_KERNEL_SKY);
    wf.clouds_list(grid_for(N), stream, sc, d.cur, ctx->cloud, d.ctrl);
    wf.clouds_march(ctx->trace_blocks * 4u, stream, sc, d.cur, ctx->cloud, d.ctrl, d.depth_const);  // persistent: 4 workgroups of 256 per CU
    wf.clouds(grid_for(N), stream, sc, d.cur, ctx->cloud, ctx->d_results, (const uint32_t*) d.ctrl, d.depth_const);
  }
  if (sc.sky_aerial_perspective && sc.sky_mode != kSkyConstantColor) {  // device_manager.c:475, device_renderer.c:84-88
    Launch l(ctx, stream, LUMC_KERNEL_SKY);
    wf.sky_inscattering(grid_for(N), stream, sc, d.cur, ctx->d_results, (const uint32_t*) d.ctrl, d.depth_const);
  }
}

// k_shade; with kResolveFused it resolves the depth before, and what it could not is finished here.
static void shade_depth(LumContext* ctx, hipStream_t stream, const DeviceScene& sc, ResolveScheme scheme, const DepthBuffers& d, uint32_t N) {
  const WavefrontKernels& wf = *ctx->wf;
  const bool fused = scheme == kResolveFused;
  {
    Launch l(ctx, stream, LUMC_KERNEL_SHADE);
    wf.shade(shade_grid(ctx, N), stream, sc, d.cur, d.next, d.nee, ctx->shadow, ctx->d_results, d.ctrl, d.depth_const, ctx->d_counters.get(),
             (scheme != kResolvePlain && !d.last) ? 1u : 0u, d.fused_records,
             fused ? ((d.depth > 0 ? 1u : 0u) | (!d.last ? 2u : 0u) | (ctx->fused_ended ? 4u : 0u)) : 0u);
  }
  if (fused && d.depth > 0) {  // the samples of depth - 1 their paths' closest hits could not decide: traced now, their vertices resolved (before this depth's visibility pass reuses the words)
    {
      Launch l(ctx, stream, LUMC_KERNEL_SHADOW);
      wf.shadow_rays(ctx->trace_blocks, ray_kernel_lds(ctx), stream, sc, ctx->fallback, nullptr, d.ctrl + kCtlVolumeShift, ctx->d_counters.get(), ctx->lds_nodes);
    }
    Launch l(ctx, stream, LUMC_KERNEL_RESOLVE);
    wf.resolve_listed(std::min<uint32_t>(grid_for(N), 1024u), stream, sc, d.prev, d.nee_before, ctx->fallback, ctx->d_results, (const uint32_t*) d.ctrl);
  }
}

// The shading of what k_shade leaves to others: particle hits, water-surface hits, paths that left into the procedural sky.
static void feature_shading(LumContext* ctx, hipStream_t stream, const DeviceScene& sc, const DepthBuffers& d, uint32_t N) {
  const WavefrontKernels& wf = *ctx->wf;
  if (sc.particles_active) {  // device_renderer.c:99-103
    Launch l(ctx, stream, LUMC_KERNEL_SHADE);
    wf.particle_shade(grid_for(N), stream, sc, d.cur, d.next, d.nee, ctx->shadow, d.ctrl, d.depth_const);
  }
  if (sc.ocean_active) {  // device_renderer.c:104-108
    Launch l(ctx, stream, LUMC_KERNEL_SHADE);
    wf.ocean_shade(grid_for(N), stream, sc, d.cur, d.next, d.nee, ctx->shadow, d.ctrl, d.depth_const);
  }
  if (sc.sky_mode == kSkyDefault) {  // paths that left the scene into the procedural sky (listed by k_shade)
    Launch l(ctx, stream, LUMC_KERNEL_SKY);
    wf.sky(grid_for(N), stream, sc, d.cur, ctx->shadow, ctx->d_results, (const uint32_t*) d.ctrl, d.depth_const);
  }
}

// Light query, visibility rays, and the depth's resolve where the scheme does it at this point.
static int visibility_and_resolve(LumContext* ctx, hipStream_t stream, const DeviceScene& sc, ResolveScheme scheme, const DepthBuffers& d, uint32_t N) {
  const WavefrontKernels& wf = *ctx->wf;
  {
    Launch l(ctx, stream, LUMC_KERNEL_LIGHT_QUERY);
    // (one resident round of its workgroups - four per CU: the kernel's workgroups are dear to start (a 1 KB stack per lane in scratch); 2 rounds, the common cap:
    //  Example-class 4.6 -> 4.0 ms per 3 steps, scan 3.9 -> 3.6, hall equal; 4 / 8 / 16 rounds on the hall: 30.2 / 32.8 / 44.5 ms against 29.9)
    wf.light_query(std::min<uint32_t>(grid_for(N), ctx->trace_blocks * 4u), stream, sc, d.cur, d.nee, ctx->shadow, d.ctrl, d.depth_const, ctx->d_counters.get());
  }
  const uint32_t* shadow_order = nullptr;
  if (ctx->sort.mode == 2) {
    shadow_order = sort_rays(ctx, stream, ctx->shadow.origin_dist, ctx->shadow.dir_out, d.ctrl + kCtlShadowItems,
                             (sc.ocean_active ? kSurfaceShadowKindsWater : 4u) * (ctx->shadow.capacity < N ? ctx->shadow.capacity : N));
    if (!shadow_order) { ctx->error = "ray sorting failed"; return 1; }
  }
  {
    Launch l(ctx, stream, LUMC_KERNEL_SHADOW);
    wf.shadow_rays(grid_persistent(ctx, N), ray_kernel_lds(ctx), stream, sc, ctx->shadow, shadow_order, d.ctrl, ctx->d_counters.get(), ctx->lds_nodes);
  }
  if (d.last || scheme == kResolvePlain) {
    Launch l(ctx, stream, LUMC_KERNEL_RESOLVE);
    wf.resolve(grid_for(N), stream, sc, d.cur, d.nee, ctx->shadow, ctx->d_results, (const uint32_t*) d.ctrl);
  }
  else if (scheme == kResolveFused) {  // the vertices no entry of the next depth continues; the others are resolved by those entries, in k_shade - and so are these, as its last input (fused_flags & 4)
    if (!ctx->fused_ended) {
      Launch l(ctx, stream, LUMC_KERNEL_RESOLVE);
      wf.resolve_ended(std::min<uint32_t>(grid_for(N), 4096u), stream, sc, d.cur, d.nee, ctx->shadow, ctx->d_results, (const uint32_t*) d.ctrl, d.ended);
    }
  }
  // (kResolveReuse: the depth's resolve waits for the next depth's closest-hit pass, closest_hits)
  return 0;
}

static void volume_bounce(LumContext* ctx, hipStream_t stream, const DeviceScene& sc, const DepthBuffers& d, uint32_t N) {
  if (render_volumes(sc) && !d.last) {  // device_renderer.c:114-118
    Launch l(ctx, stream, LUMC_KERNEL_VOLUME);
    ctx->wf->volume_bounce(grid_for(N), stream, sc, d.cur, d.next, ctx->volume, d.ctrl, d.depth_const);
  }
}

// The depth loop of one wavefront pass over the paths k_generate* left in queue[0] (at most N of them, counted on the device).
// `first_sample`, `sample_count`: the pass's sample ids when they are one contiguous range for every pixel (lumc_render), 0 otherwise.
static int wavefront_depths(LumContext* ctx, hipStream_t stream, uint32_t N, uint32_t first_sample = 0, uint32_t sample_count = 0) {
  DeviceScene sc = ctx->scene;
  const uint32_t max_depth = sc.max_ray_depth;
  prepare_sobol_table(ctx, stream, sc, first_sample, sample_count);
  if (sc.shading_mode != 0u) { debug_pass(ctx, stream, sc, N); return 0; }
  ResolveScheme scheme = ambient_reuse_active(ctx) ? kResolveReuse : kResolvePlain;
  if (scheme == kResolveReuse && ctx->wf->fused_resolve && ctx->fused_resolve != 0 && ctx->wf == wavefront_kernels_fast() && max_depth > 0) {
    if (ensure_fused(ctx, stream) == 0) scheme = kResolveFused;
    else {  // no room for its buffers (a third of the work buffers again): the separate resolve kernel does the same sums
      (void) hipGetLastError();
      ctx->error.clear();
    }
  }
  for (uint32_t depth = 0; depth <= max_depth; depth++) {
    const DepthBuffers d = depth_buffers(ctx, scheme, depth, max_depth);
    if (closest_hits(ctx, stream, sc, scheme, d, N)) return 1;
    media_passes(ctx, stream, sc, d, N);
    shade_depth(ctx, stream, sc, scheme, d, N);
    feature_shading(ctx, stream, sc, d, N);
    if (visibility_and_resolve(ctx, stream, sc, scheme, d, N)) return 1;
    volume_bounce(ctx, stream, sc, d, N);
  }
  return 0;
}

int lumc_render(LumContext* ctx, uint32_t first_sample, uint32_t num_samples, uint32_t samples_per_pass, float* d_fm, float* d_sm, void* stream_) {
  if (!ctx || !ctx->has_scene) { if (ctx) ctx->error = "lumc_render: no scene"; return 1; }
  if (ctx->num_pixels == 0) return 0;
  hipStream_t stream = (hipStream_t) stream_;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!d_fm) { d_fm = ctx->d_first_moment.get(); d_sm = ctx->d_second_moment.get(); }
  if (samples_per_pass == 0) samples_per_pass = 1;
  // sample ids beyond 2^20 would duplicate earlier ones (cuda/kernels.cuh:103-105)
  if (first_sample >= kMaxGlobalSamples) return 0;
  if (first_sample + (uint64_t) num_samples > kMaxGlobalSamples) num_samples = kMaxGlobalSamples - first_sample;
  const uint32_t P = ctx->num_pixels;
  const uint64_t want = (uint64_t) P * samples_per_pass;
  if (want > 0x7FFFFFFFull) { ctx->error = "pass too large"; return 1; }
  if (ensure_work(ctx, (uint32_t) want)) return 1;
  const DeviceScene& sc = ctx->scene;
  const uint32_t max_depth = sc.max_ray_depth;

  for (uint32_t done = 0; done < num_samples; done += samples_per_pass) {
    const uint32_t batch = std::min(samples_per_pass, num_samples - done);
    const uint32_t N = P * batch;
    PassParams pp{ctx->d_pixels.get(), P, batch, first_sample + done};
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_ctrl.get(), 0, sizeof(uint32_t) * kCtlStride * (max_depth + 2), stream));
    {
      Launch l(ctx, stream, LUMC_KERNEL_GENERATE);
      ctx->wf->generate(grid_for(N), stream, sc, pp, ctx->queue[0], ctx->d_results, ctx->d_ctrl.get() + kCtlPaths, ctx->lens, ctx->camera);
    }
    if (wavefront_depths(ctx, stream, N, first_sample + done, batch)) return 1;
    {
      Launch l(ctx, stream, LUMC_KERNEL_ACCUMULATE);
      hipLaunchKernelGGL(k_accumulate, dim3(grid_for(P)), dim3(kBlock), 0, stream, (const float4*) ctx->d_results, P, batch, d_fm, d_sm);
    }
    HIP_TRY(ctx, hipGetLastError());
  }
  return 0;
}

int lumc_render_undersampled(LumContext* ctx, uint32_t stage, uint32_t iteration, void* stream_) {
  if (!ctx || !ctx->has_scene || !ctx->d_first_moment || ctx->d_pixels || ctx->num_pixels != ctx->scene.width * ctx->scene.height) {
    if (ctx) ctx->error = "lumc_render_undersampled: needs the full-frame accumulators";
    return 1;
  }
  if (stage == 0 || stage > 15 || iteration > 3) { ctx->error = "lumc_render_undersampled: stage in [1, 15], iteration in [0, 3]"; return 1; }
  hipStream_t stream = (hipStream_t) stream_;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const DeviceScene& sc = ctx->scene;
  const std::vector<uint32_t> px = undersampling_pixels(sc.width, sc.height, stage, iteration);
  const uint32_t n = (uint32_t) px.size();
  if (n == 0) return 0;
  if (ctx->d_undersampling_pixels.count() < n) HIP_TRY(ctx, ctx->d_undersampling_pixels.resize(n));
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_undersampling_pixels.get(), px.data(), sizeof(uint32_t) * (size_t) n, hipMemcpyHostToDevice, stream));
  HIP_TRY(ctx, hipStreamSynchronize(stream));  // the list leaves scope
  if (ensure_work(ctx, n)) return 1;
  PassParams pp{ctx->d_undersampling_pixels.get(), n, 1u, 0u};  // every pixel's first sample
  HIP_TRY(ctx, hipMemsetAsync(ctx->d_ctrl.get(), 0, sizeof(uint32_t) * kCtlStride * (sc.max_ray_depth + 2), stream));
  {
    Launch l(ctx, stream, LUMC_KERNEL_GENERATE);
    ctx->wf->generate(grid_for(n), stream, sc, pp, ctx->queue[0], ctx->d_results, ctx->d_ctrl.get() + kCtlPaths, ctx->lens, ctx->camera);
  }
  if (wavefront_depths(ctx, stream, n)) return 1;
  {
    Launch l(ctx, stream, LUMC_KERNEL_ACCUMULATE);
    hipLaunchKernelGGL(k_accumulate_scatter, dim3(grid_for(n)), dim3(kBlock), 0, stream, (const float4*) ctx->d_results, (const uint32_t*) ctx->d_undersampling_pixels.get(), n,
                       ctx->num_pixels, ctx->d_first_moment.get(), ctx->d_second_moment.get());
  }
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

// ---- adaptive sampling ----
namespace {

AdaptiveView adaptive_view(const LumContext* ctx) {
  const LumContext::Adaptive& a = ctx->adaptive;
  AdaptiveView v;
  v.stage_counts = a.d_stage_counts.get(); v.block_task_end = a.d_block_task_end.get();
  v.blocks_x = a.blocks_x; v.blocks_y = a.blocks_y; v.num_blocks = a.num_blocks;
  for (uint32_t s = 0; s <= kAdaptiveStages; s++) v.executions[s] = a.executions[s];
  v.stage_id = a.stage_id;
  return v;
}

OutputParams tone_params(const LumOutputParams* p) {
  OutputParams op;
  std::memset(&op, 0, sizeof(op));
  if (p) std::memcpy(&op, p, sizeof(op));
  return op;
}

// adaptive_sampler_compute_next_stage (device_adaptive_sampler.c:105-215) in two halves: the block variances measured so far, then the
// rates of stage `stage_id + 1` from them. Between the halves a partitioned render exchanges the variances of the ranks' blocks.
int adaptive_compute_variance(LumContext* ctx, hipStream_t stream) {
  LumContext::Adaptive& a = ctx->adaptive;
  const DeviceScene& sc = ctx->scene;
  const AdaptiveView view = adaptive_view(ctx);
  const OutputParams op = tone_params(&a.params.tone);
  hipLaunchKernelGGL(k_adaptive_block_variance, dim3((a.num_blocks * 16 + 255) / 256), dim3(256), 0, stream, view, op, sc.width, sc.height, a.params.exposure,
                     (const float*) ctx->d_first_moment.get(), (const float*) ctx->d_second_moment.get(), a.d_block_variance.get());
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

// Inclusive prefix over d_block_tasks and its host copy (passes are cut at block boundaries).
int adaptive_task_prefix(LumContext* ctx, hipStream_t stream) {
  LumContext::Adaptive& a = ctx->adaptive;
  const uint32_t nb = a.num_blocks;
  HIP_TRY(ctx, hipcub::DeviceScan::InclusiveSum(a.d_scan_temp.get(), a.scan_temp_bytes, a.d_block_tasks.get(), a.d_block_task_end.get(), (int) nb, stream));
  a.task_end.resize(nb);
  HIP_TRY(ctx, hipMemcpyAsync(a.task_end.data(), a.d_block_task_end.get(), sizeof(uint32_t) * nb, hipMemcpyDeviceToHost, stream));
  HIP_TRY(ctx, hipStreamSynchronize(stream));
  return 0;
}

int adaptive_finish_build(LumContext* ctx, hipStream_t stream) {
  LumContext::Adaptive& a = ctx->adaptive;
  const uint32_t nb = a.num_blocks, chunks = (nb + kAdaptiveSumChunk - 1) / kAdaptiveSumChunk;
  hipLaunchKernelGGL(k_adaptive_sum_chunks, dim3((chunks + 63) / 64), dim3(64), 0, stream, (const float*) a.d_block_variance.get(), nb, a.d_partial.get());
  hipLaunchKernelGGL(k_adaptive_sum_total, dim3(1), dim3(1), 0, stream, (const float*) a.d_partial.get(), chunks, a.d_partial.get() + chunks);
  hipLaunchKernelGGL(k_adaptive_stage_counts, dim3((nb + 255) / 256), dim3(256), 0, stream, (const float*) a.d_block_variance.get(), (const float*) (a.d_partial.get() + chunks), nb,
                     a.stage_id, a.params.max_sampling_rate, a.params.avg_sampling_rate, a.d_stage_counts.get(), a.d_block_tasks.get(), (const uint8_t*) a.d_block_mask.get());
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(&a.variance_total, a.d_partial.get() + chunks, sizeof(float), hipMemcpyDeviceToHost, stream));
  if (adaptive_task_prefix(ctx, stream)) return 1;
  a.stage_id++;
  a.build_pending = false;
  return 0;
}

int adaptive_build_stage(LumContext* ctx, hipStream_t stream) {
  if (adaptive_compute_variance(ctx, stream)) return 1;
  return adaptive_finish_build(ctx, stream);
}

// `merged` consecutive executions of stage >= 1 as one set of passes of whole blocks (tasks_create_adaptive_sampling + the usual depth
// loop + accumulation). Merging keeps the passes large enough to fill the GPU when the rates are low.
constexpr uint32_t kAdaptiveTasksPerPass = 16u << 20;

int adaptive_execute(LumContext* ctx, hipStream_t stream, uint32_t merged) {
  LumContext::Adaptive& a = ctx->adaptive;
  const DeviceScene& sc = ctx->scene;
  const uint32_t nb = a.num_blocks;
  const AdaptiveView view = adaptive_view(ctx);
  uint32_t block = 0;
  while (block < nb) {
    AdaptivePass pass;
    pass.executions = merged;
    pass.block_begin = block;
    pass.task_begin = (block ? a.task_end[block - 1] : 0u) * merged;
    // as many whole blocks as fit the pass (a single block has at most 16 * 256 tasks per execution)
    const uint32_t limit = (pass.task_begin + kAdaptiveTasksPerPass) / merged;
    uint32_t end = (uint32_t) (std::upper_bound(a.task_end.begin() + block, a.task_end.end(), limit) - a.task_end.begin());
    if (end == block) end = block + 1;
    pass.block_end = end;
    pass.task_end = a.task_end[end - 1] * merged;
    const uint32_t N = pass.task_end - pass.task_begin;
    if (ensure_work(ctx, N)) return 1;
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_ctrl.get(), 0, sizeof(uint32_t) * kCtlStride * (sc.max_ray_depth + 2), stream));
    {
      Launch l(ctx, stream, LUMC_KERNEL_GENERATE);
      ctx->wf->generate_adaptive(grid_for(N), stream, sc, view, pass, ctx->queue[0], ctx->d_results, ctx->d_ctrl.get() + kCtlPaths, ctx->lens, ctx->camera);
    }
    if (wavefront_depths(ctx, stream, N)) return 1;
    {
      Launch l(ctx, stream, LUMC_KERNEL_ACCUMULATE);
      hipLaunchKernelGGL(k_accumulate_adaptive, dim3(grid_for((end - block) * 16)), dim3(kBlock), 0, stream, view, pass, sc.width, sc.height, (const float4*) ctx->d_results,
                         ctx->d_first_moment.get(), ctx->d_second_moment.get());
    }
    HIP_TRY(ctx, hipGetLastError());
    block = end;
  }
  a.executions[a.stage_id] += merged;
  return 0;
}

}  // namespace

int lumc_adaptive_begin(LumContext* ctx, const LumAdaptiveParams* params) {
  if (!ctx || !params) { if (ctx) ctx->error = "lumc_adaptive_begin: null argument"; return 1; }
  if (!ctx->has_scene || ctx->d_pixels || ctx->num_pixels != ctx->scene.width * ctx->scene.height || ctx->num_pixels == 0) {
    ctx->error = "lumc_adaptive_begin: needs a scene and the full-frame pixel set (lumc_set_pixels(ctx, NULL, 0))";
    return 1;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  ctx->adaptive = LumContext::Adaptive();
  LumContext::Adaptive& a = ctx->adaptive;
  a.params = *params;
  // adaptive_sampler_setup, device_adaptive_sampler.c:40-58
  a.params.max_sampling_rate = std::min(std::max(params->max_sampling_rate, 1u), kAdaptiveMaxRate);
  a.params.avg_sampling_rate = std::min(std::max(params->avg_sampling_rate, 1u), a.params.max_sampling_rate);
  a.params.update_interval = std::max(params->update_interval, 1u);
  a.blocks_x = (ctx->scene.width + 3u) >> kAdaptiveBlockLog;
  a.blocks_y = (ctx->scene.height + 3u) >> kAdaptiveBlockLog;
  a.num_blocks = a.blocks_x * a.blocks_y;
  const uint32_t nb = a.num_blocks, chunks = (nb + kAdaptiveSumChunk - 1) / kAdaptiveSumChunk;
  HIP_TRY(ctx, a.d_stage_counts.resize(nb));
  HIP_TRY(ctx, a.d_block_tasks.resize(nb));
  HIP_TRY(ctx, a.d_block_task_end.resize(nb));
  HIP_TRY(ctx, a.d_block_variance.resize(nb));
  HIP_TRY(ctx, a.d_partial.resize(chunks + 1));
  HIP_TRY(ctx, hipMemset(a.d_stage_counts.get(), 0, sizeof(uint32_t) * nb));
  HIP_TRY(ctx, hipMemset(a.d_block_variance.get(), 0, sizeof(float) * nb));
  HIP_TRY(ctx, hipcub::DeviceScan::InclusiveSum(nullptr, a.scan_temp_bytes, a.d_block_tasks.get(), a.d_block_task_end.get(), (int) nb, (hipStream_t) 0));
  HIP_TRY(ctx, a.d_scan_temp.resize(std::max<size_t>(a.scan_temp_bytes, 16)));
  a.active = true;
  return lumc_clear_accumulators(ctx);
}

int lumc_adaptive_render(LumContext* ctx, uint32_t executions, void* stream_) {
  if (!ctx || !ctx->adaptive.active) { if (ctx) ctx->error = "lumc_adaptive_render: call lumc_adaptive_begin first"; return 1; }
  hipStream_t stream = (hipStream_t) stream_;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  LumContext::Adaptive& a = ctx->adaptive;
  if (a.build_pending) { ctx->error = "lumc_adaptive_render: a stage build is pending (lumc_adaptive_variance / lumc_adaptive_build_from)"; return 1; }
  while (executions > 0) {
    const uint32_t s = a.stage_id;
    // stage s lasts update_interval << s executions (device_renderer.c:364-371); the last stage never ends
    uint32_t run = executions;
    if (s < kAdaptiveStages) {
      const uint64_t due = (uint64_t) a.params.update_interval << s;
      run = (uint32_t) std::min<uint64_t>(run, due > a.executions[s] ? due - a.executions[s] : 0);
    }
    if (s == 0 && !a.d_block_mask) {
      // one sample id for every pixel per execution: the uniform wavefront pass, several executions per pass
      if (run && lumc_render(ctx, a.executions[0], run, std::min(run, 8u), nullptr, nullptr, stream_)) return 1;
      a.executions[0] += run;
    }
    else {
      // merge executions while a merged pass stays within the usual pass size
      const uint32_t per_execution = std::max(a.task_end.empty() ? 1u : a.task_end.back(), 1u);
      const uint32_t merge_max = std::max(1u, std::min(kAdaptiveTasksPerPass / per_execution, 64u));
      for (uint32_t e = 0; e < run;) {
        const uint32_t merged = std::min(merge_max, run - e);
        if (adaptive_execute(ctx, stream, merged)) return 1;
        e += merged;
      }
    }
    executions -= run;
    if (s < kAdaptiveStages && a.executions[s] >= ((uint64_t) a.params.update_interval << s)) {
      // partitioned: the rates need the block variances of every rank; stop here and let the caller exchange them. The exchange entry
      // points (lumc_adaptive_variance / _build_from) work on the null stream: everything queued on the caller's stream is finished first.
      if (a.d_block_mask) { a.build_pending = true; HIP_TRY(ctx, hipStreamSynchronize(stream)); return 0; }
      if (adaptive_build_stage(ctx, stream)) return 1;
    }
  }
  return 0;
}

int lumc_adaptive_note_first_sample(LumContext* ctx, void* stream_) {
  if (!ctx || !ctx->adaptive.active) { if (ctx) ctx->error = "lumc_adaptive_note_first_sample: call lumc_adaptive_begin first"; return 1; }
  LumContext::Adaptive& a = ctx->adaptive;
  if (a.stage_id != 0 || a.executions[0] != 0) { ctx->error = "lumc_adaptive_note_first_sample: the first execution is already done"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  a.executions[0] = 1;
  if (a.executions[0] >= (uint64_t) a.params.update_interval) {
    if (a.d_block_mask) { a.build_pending = true; HIP_TRY(ctx, hipStreamSynchronize((hipStream_t) stream_)); return 0; }
    if (adaptive_build_stage(ctx, (hipStream_t) stream_)) return 1;
  }
  return 0;
}

int lumc_adaptive_set_partition(LumContext* ctx, const uint8_t* block_mask) {
  if (!ctx || !ctx->adaptive.active || !block_mask) { if (ctx) ctx->error = "lumc_adaptive_set_partition: adaptive mode is not active or null mask"; return 1; }
  LumContext::Adaptive& a = ctx->adaptive;
  for (uint32_t s = 0; s <= kAdaptiveStages; s++)
    if (a.executions[s]) { ctx->error = "lumc_adaptive_set_partition: call it before the first execution"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!a.d_block_mask) HIP_TRY(ctx, a.d_block_mask.resize(a.num_blocks));
  HIP_TRY(ctx, hipMemcpy(a.d_block_mask.get(), block_mask, a.num_blocks, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_adaptive_uniform_tasks, dim3((a.num_blocks + 255) / 256), dim3(256), 0, 0, (const uint8_t*) a.d_block_mask.get(), a.num_blocks, a.d_block_tasks.get());
  HIP_TRY(ctx, hipGetLastError());
  return adaptive_task_prefix(ctx, (hipStream_t) 0);
}

int lumc_adaptive_variance(LumContext* ctx, float* block_variance) {
  if (!ctx || !ctx->adaptive.active || !block_variance) { if (ctx) ctx->error = "lumc_adaptive_variance: adaptive mode is not active or null buffer"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (adaptive_compute_variance(ctx, (hipStream_t) 0)) return 1;
  HIP_TRY(ctx, hipMemcpy(block_variance, ctx->adaptive.d_block_variance.get(), sizeof(float) * ctx->adaptive.num_blocks, hipMemcpyDeviceToHost));
  return 0;
}

int lumc_adaptive_build_from(LumContext* ctx, const float* block_variance) {
  if (!ctx || !ctx->adaptive.active || !block_variance) { if (ctx) ctx->error = "lumc_adaptive_build_from: adaptive mode is not active or null buffer"; return 1; }
  LumContext::Adaptive& a = ctx->adaptive;
  if (a.stage_id >= kAdaptiveStages) { ctx->error = "lumc_adaptive_build_from: the last stage is already running"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipMemcpy(a.d_block_variance.get(), block_variance, sizeof(float) * a.num_blocks, hipMemcpyHostToDevice));
  return adaptive_finish_build(ctx, (hipStream_t) 0);
}

int lumc_adaptive_info(LumContext* ctx, LumAdaptiveInfo* out) {
  if (!ctx || !out || !ctx->adaptive.active) { if (ctx) ctx->error = "lumc_adaptive_info: adaptive mode is not active"; return 1; }
  const LumContext::Adaptive& a = ctx->adaptive;
  out->stage_id = a.stage_id;
  for (uint32_t s = 0; s <= kAdaptiveStages; s++) out->executions[s] = a.executions[s];
  out->num_blocks = a.num_blocks; out->blocks_x = a.blocks_x; out->blocks_y = a.blocks_y;
  out->tasks_per_execution = a.task_end.empty() ? a.num_blocks * 16u : a.task_end.back();
  out->variance_total = a.variance_total;
  out->build_pending = a.build_pending ? 1u : 0u;
  return 0;
}

int lumc_adaptive_download(LumContext* ctx, uint32_t* stage_counts, float* block_variance) {
  if (!ctx || !ctx->adaptive.active) { if (ctx) ctx->error = "lumc_adaptive_download: adaptive mode is not active"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipDeviceSynchronize());
  const LumContext::Adaptive& a = ctx->adaptive;
  if (stage_counts) HIP_TRY(ctx, hipMemcpy(stage_counts, a.d_stage_counts.get(), sizeof(uint32_t) * a.num_blocks, hipMemcpyDeviceToHost));
  if (block_variance) HIP_TRY(ctx, hipMemcpy(block_variance, a.d_block_variance.get(), sizeof(float) * a.num_blocks, hipMemcpyDeviceToHost));
  return 0;
}

int lumc_adaptive_end(LumContext* ctx) {
  if (!ctx) return 1;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipDeviceSynchronize());
  ctx->adaptive = LumContext::Adaptive();
  return 0;
}

// The context's result image of n pixels: what lumc_generate_result* write when the caller passes no image of its own.
static int result_image(LumContext* ctx, uint32_t n, float** out) {
  if (ctx->d_frame_result.count() != 3 * (size_t) n) HIP_TRY(ctx, ctx->d_frame_result.resize(3 * (size_t) n));
  *out = ctx->d_frame_result.get();
  return 0;
}

int lumc_generate_result(LumContext* ctx, uint32_t mode, uint32_t local_error_minimization, uint32_t uniform_samples, float exposure, const LumOutputParams* tone,
                         float* d_result, void* stream_) {
  const bool framed = ctx && ctx->exchange.use_frame && ctx->exchange.d_frame && ctx->has_scene && ctx->exchange.frame_pixels() == ctx->scene.width * ctx->scene.height;
  if (!ctx || !ctx->has_scene || (!framed && (!ctx->d_first_moment || ctx->d_pixels || ctx->num_pixels != ctx->scene.width * ctx->scene.height))) {
    if (ctx) ctx->error = "lumc_generate_result: needs the full-frame accumulators";
    return 1;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t stream = (hipStream_t) stream_;
  const uint32_t n = ctx->scene.width * ctx->scene.height;
  const float* src_fm = framed ? ctx->exchange.d_frame.get() : ctx->d_first_moment.get();
  const float* src_sm = framed ? ctx->exchange.d_frame.get() + 3 * (size_t) n : ctx->d_second_moment.get();
  if (!d_result && result_image(ctx, n, &d_result)) return 1;
  AdaptiveView view;
  std::memset(&view, 0, sizeof(view));
  if (ctx->adaptive.active) view = adaptive_view(ctx);
  else { view.blocks_x = (ctx->scene.width + 3u) >> kAdaptiveBlockLog; view.blocks_y = (ctx->scene.height + 3u) >> kAdaptiveBlockLog; view.num_blocks = view.blocks_x * view.blocks_y; }
  if (!ctx->adaptive.active && uniform_samples == 0) { ctx->error = "lumc_generate_result: no samples"; return 1; }
  ResultParams rp{ctx->scene.width, ctx->scene.height, mode, local_error_minimization, uniform_samples, exposure};
  const OutputParams op = tone_params(tone);
  {
    Launch l(ctx, stream, LUMC_KERNEL_OUTPUT);
    hipLaunchKernelGGL(k_generate_result, dim3(grid_for(n)), dim3(256), 0, stream, view, rp, op, src_fm, src_sm, d_result);
  }
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

int lumc_generate_result_host(LumContext* ctx, uint32_t mode, uint32_t local_error_minimization, uint32_t uniform_samples, float exposure, const LumOutputParams* tone,
                              float* result) {
  if (!ctx || !result) { if (ctx) ctx->error = "lumc_generate_result_host: null argument"; return 1; }
  if (lumc_generate_result(ctx, mode, local_error_minimization, uniform_samples, exposure, tone, nullptr, nullptr)) return 1;
  HIP_TRY(ctx, hipDeviceSynchronize());
  HIP_TRY(ctx, hipMemcpy(result, ctx->d_frame_result.get(), sizeof(float) * 3 * (size_t) ctx->scene.width * ctx->scene.height, hipMemcpyDeviceToHost));
  return 0;
}

int lumc_generate_result_undersampled(LumContext* ctx, uint32_t stage, uint32_t iteration, float* d_result, void* stream_) {
  if (!ctx || !ctx->has_scene || !ctx->d_first_moment || ctx->d_pixels || ctx->num_pixels != ctx->scene.width * ctx->scene.height) {
    if (ctx) ctx->error = "lumc_generate_result_undersampled: needs the full-frame accumulators";
    return 1;
  }
  if (stage == 0 || stage > 15 || iteration > 3) { ctx->error = "lumc_generate_result_undersampled: stage in [1, 15], iteration in [0, 3]"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t stream = (hipStream_t) stream_;
  const uint32_t n = ctx->num_pixels;
  if (!d_result && result_image(ctx, n, &d_result)) return 1;
  const uint32_t compact = (ctx->scene.width >> stage) * (ctx->scene.height >> stage);
  if (compact == 0) return 0;
  {
    Launch l(ctx, stream, LUMC_KERNEL_OUTPUT);
    hipLaunchKernelGGL(k_result_undersampled, dim3(grid_for(compact)), dim3(256), 0, stream, (const float*) ctx->d_first_moment.get(), ctx->scene.width, ctx->scene.height, stage, iteration,
                       d_result);
  }
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

int lumc_generate_result_undersampled_host(LumContext* ctx, uint32_t stage, uint32_t iteration, float* result) {
  if (!ctx || !result) { if (ctx) ctx->error = "lumc_generate_result_undersampled_host: null argument"; return 1; }
  if (lumc_generate_result_undersampled(ctx, stage, iteration, nullptr, nullptr)) return 1;
  HIP_TRY(ctx, hipDeviceSynchronize());
  const size_t compact = (size_t) (ctx->scene.width >> stage) * (ctx->scene.height >> stage);
  HIP_TRY(ctx, hipMemcpy(result, ctx->d_frame_result.get(), sizeof(float) * 3 * compact, hipMemcpyDeviceToHost));
  return 0;
}

int lumc_download_result_image(LumContext* ctx, float* result) {
  if (!ctx || !result || !ctx->d_frame_result || !ctx->has_scene || ctx->d_frame_result.count() != 3 * (size_t) (ctx->scene.width * ctx->scene.height)) { if (ctx) ctx->error = "lumc_download_result_image: no result image"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipDeviceSynchronize());
  HIP_TRY(ctx, hipMemcpy(result, ctx->d_frame_result.get(), sizeof(float) * ctx->d_frame_result.count(), hipMemcpyDeviceToHost));
  return 0;
}
const float* lumc_result_image(LumContext* ctx) { return ctx ? ctx->d_frame_result.get() : nullptr; }

// _device_post_bloom_apply, device/device_post.c:56-139
int lumc_post_bloom(LumContext* ctx, float* d_image, uint32_t full_width, uint32_t full_height, uint32_t undersampling_stage, float blend, void* stream_) {
  if (!ctx) return 1;
  if (!d_image) d_image = ctx->d_frame_result.get();
  if (!d_image || full_width == 0 || full_height == 0) { ctx->error = "lumc_post_bloom: no image"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t stream = (hipStream_t) stream_;
  uint32_t chain = 0;  // _device_post_bloom_mip_count: floor(log2(min dimension))
  for (uint32_t m = std::min(full_width, full_height); m > 1; m >>= 1) chain++;
  if (undersampling_stage + 1 >= chain) return 0;  // too coarse for a mip chain (device_post.c:62-64)
  if (ctx->bloom_width != full_width || ctx->bloom_height != full_height) {
    ctx->bloom_mips.clear(); ctx->bloom_width = ctx->bloom_height = 0;
    for (uint32_t i = 0; i < chain; i++) {
      DeviceBuffer<float> m;
      HIP_TRY(ctx, m.resize((size_t) (full_width >> (i + 1)) * (full_height >> (i + 1))));
      ctx->bloom_mips.push_back(std::move(m));
    }
    ctx->bloom_width = full_width; ctx->bloom_height = full_height;
  }
  const uint32_t width = full_width >> undersampling_stage, height = full_height >> undersampling_stage, mips = chain - undersampling_stage;
  const size_t plane = (size_t) width * height;
  Launch l(ctx, stream, LUMC_KERNEL_OUTPUT);
  for (uint32_t c = 0; c < 3; c++) {
    float* image = d_image + c * plane;
    const std::vector<DeviceBuffer<float>>& mip = ctx->bloom_mips;
    hipLaunchKernelGGL(k_post_downsample, dim3(grid_for((width >> 1) * (height >> 1))), dim3(256), 0, stream, (const float*) image, width, height, mip[0].get(), width >> 1, height >> 1);
    for (uint32_t i = 0; i + 1 < mips; i++)
      hipLaunchKernelGGL(k_post_downsample, dim3(grid_for((width >> (i + 2)) * (height >> (i + 2)))), dim3(256), 0, stream, (const float*) mip[i].get(), width >> (i + 1), height >> (i + 1),
                         mip[i + 1].get(), width >> (i + 2), height >> (i + 2));
    for (uint32_t i = mips - 1; i > 0; i--)
      hipLaunchKernelGGL(k_post_upsample, dim3(grid_for((width >> i) * (height >> i))), dim3(256), 0, stream, (const float*) mip[i].get(), width >> (i + 1), height >> (i + 1), mip[i - 1].get(),
                         width >> i, height >> i, 1.0f, 1.0f);
    hipLaunchKernelGGL(k_post_upsample, dim3(grid_for(width * height)), dim3(256), 0, stream, (const float*) mip[0].get(), width >> 1, height >> 1, image, width, height, blend / mips,
                       1.0f - blend);
  }
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

int lumc_post_bloom_host(LumContext* ctx, float* image, uint32_t full_width, uint32_t full_height, uint32_t undersampling_stage, float blend) {
  if (!ctx || !image) { if (ctx) ctx->error = "lumc_post_bloom_host: null argument"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t count = 3 * (size_t) (full_width >> undersampling_stage) * (full_height >> undersampling_stage);
  DeviceBuffer<float> d;
  HIP_TRY(ctx, d.assign(image, count));
  if (lumc_post_bloom(ctx, d.get(), full_width, full_height, undersampling_stage, blend, nullptr)) return 1;
  HIP_TRY(ctx, hipDeviceSynchronize());
  HIP_TRY(ctx, hipMemcpy(image, d.get(), sizeof(float) * count, hipMemcpyDeviceToHost));
  return 0;
}

// ---- denoiser (dev_denoise.h) ----
static size_t guide_pixels(const LumContext* ctx) { return ctx->d_guides.count() / kGuideSumPlanes; }  // the frame the guide planes were allocated for

int lumc_render_guides(LumContext* ctx, uint32_t num_samples, void* stream_) {
  if (!ctx || !ctx->has_scene) { if (ctx) ctx->error = "lumc_render_guides: no scene"; return 1; }
  if (num_samples == 0) num_samples = 4;
  if (num_samples > 1024u) { ctx->error = "lumc_render_guides: at most 1024 guide samples"; return 1; }
  hipStream_t stream = (hipStream_t) stream_;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  DeviceScene sc = ctx->scene;
  sc.sobol_table = nullptr;
  const uint32_t n = sc.width * sc.height;
  if (n == 0 || sc.width > 0xFFFFu || sc.height > 0xFFFFu) { ctx->error = "lumc_render_guides: frame size"; return 1; }
  ctx->guides_valid = false;
  if (guide_pixels(ctx) != n) HIP_TRY(ctx, ctx->d_guides.resize(kGuideSumPlanes * (size_t) n));
  if (ensure_work(ctx, n)) return 1;
  HIP_TRY(ctx, hipMemsetAsync(ctx->d_guides.get(), 0, sizeof(float) * kGuideSumPlanes * (size_t) n, stream));
  const WavefrontKernels& wf = *ctx->wf;
  // one sample id of every pixel per pass: the closest-hit pass of the debug shading modes (wavefront_depths), then k_guide adds into the planes
  for (uint32_t s = 0; s < num_samples; s++) {
    PassParams pp{nullptr, n, 1u, s};
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_ctrl.get(), 0, sizeof(uint32_t) * kCtlStride * (sc.max_ray_depth + 2), stream));
    {
      Launch l(ctx, stream, LUMC_KERNEL_GENERATE);
      wf.generate(grid_for(n), stream, sc, pp, ctx->queue[0], ctx->d_results, ctx->d_ctrl.get() + kCtlPaths, ctx->lens, ctx->camera);
    }
    {
      Launch l(ctx, stream, LUMC_KERNEL_TRACE);
      wf.trace(grid_persistent(ctx, n), ray_kernel_lds(ctx), stream, sc, ctx->queue[0], nullptr, ctx->d_ctrl.get(), ctx->d_counters.get(), ctx->lds_nodes);
    }
    if (sc.particles_active) trace_particles(ctx, stream, ctx->queue[0], ctx->d_ctrl.get(), n);
    if (sc.ocean_active) {
      Launch l(ctx, stream, LUMC_KERNEL_TRACE);
      wf.trace_ocean(grid_for(n), stream, sc, ctx->queue[0], (const uint32_t*) ctx->d_ctrl.get());
    }
    Launch l(ctx, stream, LUMC_KERNEL_OUTPUT);
    wf.guide(grid_for(n), stream, sc, ctx->queue[0], (const uint32_t*) ctx->d_ctrl.get(), ctx->d_guides.get(), n);
  }
  {
    Launch l(ctx, stream, LUMC_KERNEL_OUTPUT);
    wf.guide_normalise(grid_for(n), stream, ctx->d_guides.get(), n, num_samples);
  }
  HIP_TRY(ctx, hipGetLastError());
  ctx->guides_valid = true;
  return 0;
}

int lumc_download_guides(LumContext* ctx, float* albedo, float* normal, float* depth) {
  if (!ctx || !ctx->guides_valid) { if (ctx) ctx->error = "lumc_download_guides: no guides (lumc_render_guides)"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipDeviceSynchronize());
  const size_t n = guide_pixels(ctx);
  if (albedo) HIP_TRY(ctx, hipMemcpy(albedo, ctx->d_guides.get(), sizeof(float) * 3 * n, hipMemcpyDeviceToHost));
  if (normal) HIP_TRY(ctx, hipMemcpy(normal, ctx->d_guides.get() + 3 * n, sizeof(float) * 3 * n, hipMemcpyDeviceToHost));
  if (depth) HIP_TRY(ctx, hipMemcpy(depth, ctx->d_guides.get() + 6 * n, sizeof(float) * n, hipMemcpyDeviceToHost));
  return 0;
}

int lumc_has_guides(const LumContext* ctx) { return (ctx && ctx->guides_valid) ? 1 : 0; }

void lumc_denoise_default_params(LumDenoiseParams* p) {
  if (!p) return;
  p->iterations = 5; p->sigma_luminance = 4.0f; p->sigma_normal = 128.0f; p->sigma_depth = 1.0f; p->uniform_samples = 0;
}

int lumc_set_denoise_form(LumContext* ctx, int lds) {
  if (!ctx) return 1;
  ctx->denoise_lds = lds != 0 ? 1 : 0;
  return 0;
}

int lumc_denoise(LumContext* ctx, const LumDenoiseParams* params, float* d_image, void* stream_) {
  if (!ctx || !params || !ctx->has_scene) { if (ctx) ctx->error = "lumc_denoise: no scene or null argument"; return 1; }
  const uint32_t n = ctx->scene.width * ctx->scene.height;
  if (!ctx->guides_valid || guide_pixels(ctx) != n) { ctx->error = "lumc_denoise: no guides for this frame (lumc_render_guides)"; return 1; }
  const bool framed = ctx->exchange.use_frame && ctx->exchange.d_frame && ctx->exchange.frame_pixels() == n;
  if (!framed && (!ctx->d_first_moment || ctx->d_pixels || ctx->num_pixels != n)) { ctx->error = "lumc_denoise: needs the full-frame accumulators"; return 1; }
  if (!d_image) d_image = (ctx->d_frame_result.count() == 3 * (size_t) n) ? ctx->d_frame_result.get() : nullptr;
  if (!d_image) { ctx->error = "lumc_denoise: no image"; return 1; }
  if (!ctx->adaptive.active && params->uniform_samples == 0) { ctx->error = "lumc_denoise: no samples"; return 1; }
  if (!(params->sigma_luminance > 0.0f) || !(params->sigma_normal >= 0.0f) || !(params->sigma_depth > 0.0f)) { ctx->error = "lumc_denoise: sigmas must be positive"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t stream = (hipStream_t) stream_;
  if (ctx->d_denoise_rec[2].count() != n) {  // (the last of the three: a set that was not completed is allocated again)
    for (auto& r : ctx->d_denoise_rec) r.reset();
    for (auto& r : ctx->d_denoise_rec) HIP_TRY(ctx, r.resize(n));
  }
  const float* src_fm = framed ? ctx->exchange.d_frame.get() : ctx->d_first_moment.get();
  const float* src_sm = framed ? ctx->exchange.d_frame.get() + 3 * (size_t) n : ctx->d_second_moment.get();
  AdaptiveView view;
  std::memset(&view, 0, sizeof(view));
  if (ctx->adaptive.active) view = adaptive_view(ctx);
  DenoiseArgs args{ctx->scene.width, ctx->scene.height, 1u, params->uniform_samples, params->sigma_luminance, params->sigma_normal, params->sigma_depth};
  const uint32_t iterations = std::min(params->iterations, 6u);
  float4* rec_a[2] = {ctx->d_denoise_rec[0].get(), ctx->d_denoise_rec[1].get()};
  uint4* rec_b = (uint4*) ctx->d_denoise_rec[2].get();
  const WavefrontKernels& wf = *ctx->wf;
  Launch l(ctx, stream, LUMC_KERNEL_OUTPUT);
  wf.denoise_prepare(grid_for(n), stream, view, args, src_fm, src_sm, d_image, ctx->d_guides.get(), rec_a[0], rec_b);
  uint32_t cur = 0;
  for (uint32_t i = 0; i < iterations; i++, cur ^= 1u) {
    args.step = 1u << i;
    wf.denoise_atrous(stream, args, rec_a[cur], rec_b, rec_a[cur ^ 1u], ctx->denoise_lds != 0);
  }
  wf.denoise_finish(grid_for(n), stream, args, rec_a[cur], ctx->d_guides.get(), d_image);
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

int lumc_denoise_host(LumContext* ctx, const LumDenoiseParams* params, float* image) {
  if (!ctx || !image || !ctx->has_scene) { if (ctx) ctx->error = "lumc_denoise_host: null argument"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t count = 3 * (size_t) ctx->scene.width * ctx->scene.height;
  DeviceBuffer<float> d;
  HIP_TRY(ctx, d.assign(image, count));
  if (lumc_denoise(ctx, params, d.get(), nullptr)) return 1;
  HIP_TRY(ctx, hipDeviceSynchronize());
  HIP_TRY(ctx, hipMemcpy(image, d.get(), sizeof(float) * count, hipMemcpyDeviceToHost));
  return 0;
}

int lumc_synchronize(LumContext* ctx) {
  if (!ctx) return 1;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipDeviceSynchronize());
  return resolve_stamps(ctx);
}

int lumc_download_accumulators(LumContext* ctx, float* first_moment, float* second_moment) {
  if (!ctx || !ctx->d_first_moment) return 1;
  HIP_TRY(ctx, hipDeviceSynchronize());
  if (first_moment) HIP_TRY(ctx, hipMemcpy(first_moment, ctx->d_first_moment.get(), sizeof(float) * 3 * (size_t) ctx->num_pixels, hipMemcpyDeviceToHost));
  if (second_moment) HIP_TRY(ctx, hipMemcpy(second_moment, ctx->d_second_moment.get(), sizeof(float) * (size_t) ctx->num_pixels, hipMemcpyDeviceToHost));
  return 0;
}

int lumc_counters(LumContext* ctx, uint64_t out[LUMC_CNT_COUNT]) {
  if (!ctx) return 1;
  HIP_TRY(ctx, hipDeviceSynchronize());
  HIP_TRY(ctx, hipMemcpy(out, ctx->d_counters.get(), sizeof(uint64_t) * LUMC_CNT_COUNT, hipMemcpyDeviceToHost));
  return 0;
}
int lumc_reset_counters(LumContext* ctx) {
  if (!ctx) return 1;
  HIP_TRY(ctx, hipMemset(ctx->d_counters.get(), 0, sizeof(uint64_t) * LUMC_CNT_COUNT));
  return 0;
}
int lumc_set_profiling(LumContext* ctx, int enabled) {
  if (!ctx) return 1;
  ctx->profiling = enabled != 0;
  for (int k = 0; k < LUMC_KERNEL_COUNT; k++) { ctx->kernel_ms[k] = 0.0; ctx->kernel_launches[k] = 0; }
  return 0;
}
int lumc_kernel_times(LumContext* ctx, double total_ms[LUMC_KERNEL_COUNT], uint32_t launches[LUMC_KERNEL_COUNT]) {
  if (!ctx) return 1;
  if (lumc_synchronize(ctx)) return 1;
  for (int k = 0; k < LUMC_KERNEL_COUNT; k++) { total_ms[k] = ctx->kernel_ms[k]; launches[k] = ctx->kernel_launches[k]; }
  return 0;
}

extern "C" const unsigned char lum_embedded_bluenoise_1d[];
extern "C" const unsigned char lum_embedded_bluenoise_1d_end[];

int lumc_generate_output(LumContext* ctx, const LumOutputParams* params, const float* d_first_moment, uint32_t* d_argb8, void* stream_) {
  if (!ctx || !params || !d_argb8) { if (ctx) ctx->error = "lumc_generate_output: null argument"; return 1; }
  static_assert(sizeof(LumOutputParams) == sizeof(OutputParams), "output parameter structs must match");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t stream = (hipStream_t) stream_;
  OutputParams p;
  std::memcpy(&p, params, sizeof(p));
  if (p.src_width == 0 || p.src_height == 0 || p.dst_width < 2 || p.dst_height < 2) { ctx->error = "lumc_generate_output: image sizes must be at least 2x2"; return 1; }
  if (p.supersampling > 3 || p.undersampling_stage > 15) { ctx->error = "lumc_generate_output: supersampling at most 3, undersampling stage at most 15"; return 1; }
  const uint32_t ns = p.src_width * p.src_height;
  const uint32_t uo = std::max(p.undersampling_stage, p.supersampling);
  const uint32_t n_out = (p.src_width >> uo) * (p.src_height >> uo);
  if (n_out == 0) { ctx->error = "lumc_generate_output: the frame is smaller than one output pixel"; return 1; }
  if (!d_first_moment) {
    if (p.undersampling_stage) { ctx->error = "lumc_generate_output: an undersampled image must be passed explicitly (lumc_result_image)"; return 1; }
    if (!ctx->d_first_moment || ctx->d_pixels || ctx->num_pixels != ns) { ctx->error = "lumc_generate_output: the context does not hold a full frame of this size"; return 1; }
    d_first_moment = ctx->d_first_moment.get();
  }
  if (!ctx->d_bluenoise_1d) {
    const size_t bytes = (size_t) (lum_embedded_bluenoise_1d_end - lum_embedded_bluenoise_1d);
    if (bytes != 65536 * sizeof(uint16_t)) { ctx->error = "embedded 1D blue-noise mask has the wrong size"; return 1; }
    HIP_TRY(ctx, ctx->d_bluenoise_1d.assign((const uint16_t*) lum_embedded_bluenoise_1d, 65536));
  }
  if (ctx->d_frame_output.count() < 3 * (size_t) ns) HIP_TRY(ctx, ctx->d_frame_output.resize(3 * (size_t) ns));
  {
    Launch l(ctx, stream, LUMC_KERNEL_OUTPUT);
    hipLaunchKernelGGL(k_final_image, dim3(grid_for(n_out)), dim3(256), 0, stream, p, d_first_moment, ctx->d_frame_output.get());
    hipLaunchKernelGGL(k_to_argb8, dim3(grid_for(p.dst_width * p.dst_height)), dim3(256), 0, stream, p, (const float*) ctx->d_frame_output.get(),
                       (const uint16_t*) ctx->d_bluenoise_1d.get(), d_argb8);
  }
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

int lumc_generate_output_host(LumContext* ctx, const LumOutputParams* params, const float* d_first_moment, uint32_t* argb8, float* frame_output) {
  if (!ctx || !params || !argb8) { if (ctx) ctx->error = "lumc_generate_output_host: null argument"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const uint32_t n = params->dst_width * params->dst_height;
  if (ctx->d_argb8.count() < n) HIP_TRY(ctx, ctx->d_argb8.resize(n));
  if (lumc_generate_output(ctx, params, d_first_moment, ctx->d_argb8.get(), nullptr)) return 1;
  HIP_TRY(ctx, hipDeviceSynchronize());
  HIP_TRY(ctx, hipMemcpy(argb8, ctx->d_argb8.get(), sizeof(uint32_t) * (size_t) n, hipMemcpyDeviceToHost));
  if (frame_output) {
    const uint32_t uo = std::max(params->undersampling_stage, params->supersampling);
    HIP_TRY(ctx, hipMemcpy(frame_output, ctx->d_frame_output.get(), sizeof(float) * 3 * (size_t) (params->src_width >> uo) * (params->src_height >> uo), hipMemcpyDeviceToHost));
  }
  return 0;
}

int lumc_generate_output_from_host(LumContext* ctx, const LumOutputParams* params, const float* first_moment, uint32_t* argb8, float* frame_output) {
  if (!ctx || !params || !first_moment || !argb8) { if (ctx) ctx->error = "lumc_generate_output_from_host: null argument"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  DeviceBuffer<float> d;
  HIP_TRY(ctx, d.assign(first_moment, 3 * (size_t) (params->src_width >> params->undersampling_stage) * (params->src_height >> params->undersampling_stage)));
  return lumc_generate_output_host(ctx, params, d.get(), argb8, frame_output);
}

int lumc_trace_closest(LumContext* ctx, uint32_t n, const float* d_origins, const float* d_dirs, const uint32_t* d_ignore, uint32_t* d_out, void* stream_) {
  if (!ctx || !ctx->has_scene) { if (ctx) ctx->error = "lumc_trace_closest: no scene"; return 1; }
  if (n == 0) return 0;
  hipStream_t stream = (hipStream_t) stream_;
  uint32_t* cursor = ctx->d_ctrl.get() + kCtlStride * (kCtrlRows - 1);
  HIP_TRY(ctx, hipMemsetAsync(cursor, 0, sizeof(uint32_t), stream));  // the work cursor of trace_items (dev_trace.h)
  Launch l(ctx, stream, LUMC_KERNEL_TRACE);
  ctx->wf->trace_rays(grid_persistent(ctx, n), ray_kernel_lds(ctx), stream, ctx->scene, n, d_origins, d_dirs, d_ignore, d_out, cursor, ctx->d_counters.get(),
                      ctx->lds_nodes);
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

int lumc_trace_closest_host(LumContext* ctx, uint32_t n, const float* origins, const float* dirs, const uint32_t* ignore, uint32_t* out) {
  if (!ctx || !ctx->has_scene) { if (ctx) ctx->error = "lumc_trace_closest_host: no scene"; return 1; }
  if (n == 0) return 0;
  DeviceBuffer<float> d_o, d_d;
  DeviceBuffer<uint32_t> d_i, d_out;
  HIP_TRY(ctx, d_o.assign(origins, 3 * (size_t) n));
  HIP_TRY(ctx, d_d.assign(dirs, 3 * (size_t) n));
  HIP_TRY(ctx, d_out.resize(3 * (size_t) n));
  HIP_TRY(ctx, d_i.assign(ignore, 2 * (size_t) n));
  if (lumc_trace_closest(ctx, n, d_o.get(), d_d.get(), d_i.get(), d_out.get(), nullptr)) return 1;
  HIP_TRY(ctx, hipMemcpy(out, d_out.get(), sizeof(uint32_t) * 3 * (size_t) n, hipMemcpyDeviceToHost));
  return 0;
}

// Visibility rays through the render's own kernel: a temporary ShadowQueue whose output index is the ray index, the item count and the work cursor in the spare
// control row, the active flavour's k_shadow_rays with the render's grid, LDS size and staged nodes. The answers start as a NaN pattern, so a ray that nobody
// answered shows. Synchronises the stream (the temporaries are freed before the call returns).
int lumc_trace_visibility(LumContext* ctx, uint32_t n, const float* d_origins, const float* d_dirs, const float* d_dist, const uint32_t* d_ids, const uint32_t* d_order, float* d_out,
                          void* stream_) {
  if (!ctx || !ctx->has_scene) { if (ctx) ctx->error = "lumc_trace_visibility: no scene"; return 1; }
  if (n == 0) return 0;
  if (!d_origins || !d_dirs || !d_dist || !d_ids || !d_out) { ctx->error = "lumc_trace_visibility: null argument"; return 1; }
  hipStream_t stream = (hipStream_t) stream_;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  DeviceBuffer<float4> buffer;  // origin_dist | dir_out | ids | vis, n entries of 16 bytes each
  HIP_TRY(ctx, buffer.resize(4 * (size_t) n));
  float4* items = buffer.get();
  ShadowQueue sq{};
  sq.origin_dist = items; sq.dir_out = items + n; sq.ids = reinterpret_cast<uint4*>(items + 2 * (size_t) n); sq.vis = items + 3 * (size_t) n;
  sq.capacity = n;
  uint32_t* ctrl = ctx->d_ctrl.get() + kCtlStride * (kCtrlRows - 2);
  const uint32_t blocks = (n + 255u) / 256u;
  HIP_TRY(ctx, hipMemsetAsync(sq.vis, 0xFF, sizeof(float4) * (size_t) n, stream));
  HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t) (ctrl + kCtlShadowItems), (int) n, 1, stream));
  HIP_TRY(ctx, hipMemsetAsync(ctrl + kCtlShadowCursor, 0, sizeof(uint32_t), stream));
  hipLaunchKernelGGL(k_visibility_pack, dim3(blocks), dim3(256), 0, stream, n, d_origins, d_dirs, d_dist, d_ids, sq);
  {
    Launch l(ctx, stream, LUMC_KERNEL_SHADOW);
    ctx->wf->shadow_rays(grid_persistent(ctx, n), ray_kernel_lds(ctx), stream, ctx->scene, sq, d_order, ctrl, ctx->d_counters.get(), ctx->lds_nodes);
  }
  hipLaunchKernelGGL(k_visibility_unpack, dim3(blocks), dim3(256), 0, stream, n, sq.vis, d_out);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipStreamSynchronize(stream));
  return 0;
}

int lumc_trace_visibility_host(LumContext* ctx, uint32_t n, const float* origins, const float* dirs, const float* dist, const uint32_t* ids, const uint32_t* order, float* out) {
  if (!ctx || !ctx->has_scene) { if (ctx) ctx->error = "lumc_trace_visibility_host: no scene"; return 1; }
  if (n == 0) return 0;
  if (!origins || !dirs || !dist || !ids || !out) { ctx->error = "lumc_trace_visibility_host: null argument"; return 1; }
  if (order) {  // a slot that names no ray would read outside the queue
    for (uint32_t i = 0; i < n; i++) if (order[i] >= n) { ctx->error = "lumc_trace_visibility_host: order entry out of range"; return 1; }
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  DeviceBuffer<float> d_o, d_d, d_t, d_out;
  DeviceBuffer<uint32_t> d_i, d_ord;
  HIP_TRY(ctx, d_o.assign(origins, 3 * (size_t) n));
  HIP_TRY(ctx, d_d.assign(dirs, 3 * (size_t) n));
  HIP_TRY(ctx, d_t.assign(dist, n));
  HIP_TRY(ctx, d_i.assign(ids, 4 * (size_t) n));
  HIP_TRY(ctx, d_ord.assign(order, n));
  HIP_TRY(ctx, d_out.resize(3 * (size_t) n));
  if (lumc_trace_visibility(ctx, n, d_o.get(), d_d.get(), d_t.get(), d_i.get(), d_ord.get(), d_out.get(), nullptr)) return 1;
  HIP_TRY(ctx, hipMemcpy(out, d_out.get(), sizeof(float) * 3 * (size_t) n, hipMemcpyDeviceToHost));
  return 0;
}

// The light-BVH query of BSDF-sampled directions (light_query, dev_trace.h) on plain rays, in the active flavour: out_ids = the picked light or 0xFFFFFFFF, out_num_hits = the
// number of candidates. A scene without lights answers (0xFFFFFFFF, 0) without a launch.
int lumc_light_query_host(LumContext* ctx, uint32_t n, const float* origins, const float* dirs, const uint32_t* self, const float* randoms, uint32_t* out_ids, uint32_t* out_num_hits) {
  if (!ctx || !ctx->has_scene) { if (ctx) ctx->error = "lumc_light_query_host: no scene"; return 1; }
  if (n == 0) return 0;
  if (!origins || !dirs || !self || !randoms || !out_ids || !out_num_hits) { ctx->error = "lumc_light_query_host: null argument"; return 1; }
  const DeviceScene& sc = ctx->scene;
  if (!sc.num_lights || !sc.light_nodes || !sc.light_tris || !sc.light_tri_handles) {
    for (uint32_t i = 0; i < n; i++) { out_ids[i] = 0xFFFFFFFFu; out_num_hits[i] = 0u; }
    return 0;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  DeviceBuffer<float> d_o, d_d, d_r;
  DeviceBuffer<uint32_t> d_s, d_out;
  HIP_TRY(ctx, d_o.assign(origins, 3 * (size_t) n));
  HIP_TRY(ctx, d_d.assign(dirs, 3 * (size_t) n));
  HIP_TRY(ctx, d_s.assign(self, 2 * (size_t) n));
  HIP_TRY(ctx, d_r.assign(randoms, n));
  HIP_TRY(ctx, d_out.resize(2 * (size_t) n));
  HIP_TRY(ctx, hipMemset(d_out.get(), 0xFF, sizeof(uint32_t) * 2 * (size_t) n));
  ctx->wf->light_query_probe(nullptr, sc, n, d_o.get(), d_d.get(), d_s.get(), d_r.get(), d_out.get(), d_out.get() + n);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipDeviceSynchronize());
  HIP_TRY(ctx, hipMemcpy(out_ids, d_out.get(), sizeof(uint32_t) * (size_t) n, hipMemcpyDeviceToHost));
  HIP_TRY(ctx, hipMemcpy(out_num_hits, d_out.get() + n, sizeof(uint32_t) * (size_t) n, hipMemcpyDeviceToHost));
  return 0;
}

int lumc_pixel_query(LumContext* ctx, uint32_t x, uint32_t y, uint32_t sample_id, uint32_t out[6]) {
  if (!ctx || !ctx->has_scene || !out) { if (ctx) ctx->error = "lumc_pixel_query: no scene"; return 1; }
  if (x >= ctx->scene.width || y >= ctx->scene.height) { ctx->error = "lumc_pixel_query: pixel outside the frame"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  DeviceBuffer<float> buffer;  // origin[3] direction[3] hit[3] valid
  HIP_TRY(ctx, buffer.resize(10));
  float* d = buffer.get();
  hipLaunchKernelGGL(k_pixel_ray, dim3(1), dim3(64), 0, 0, ctx->scene, ctx->lens, ctx->camera, x, y, sample_id, d, d + 3, (uint32_t*) (d + 9));
  uint32_t valid = 0;
  HIP_TRY(ctx, hipMemcpy(&valid, d + 9, 4, hipMemcpyDeviceToHost));
  if (valid && lumc_trace_closest(ctx, 1, d, d + 3, nullptr, (uint32_t*) (d + 6), nullptr)) return 1;
  HIP_TRY(ctx, hipDeviceSynchronize());
  if (valid) HIP_TRY(ctx, hipMemcpy(out, d + 6, 12, hipMemcpyDeviceToHost));
  else { out[0] = 0xFFFFFFFFu; out[1] = 0u; std::memcpy(&out[2], &kFltMax, 4); }  // the ray did not leave the lens: nothing is hit
  HIP_TRY(ctx, hipMemcpy(out + 3, d + 3, 12, hipMemcpyDeviceToHost));
  return 0;
}

int lumc_set_physical_camera(LumContext* ctx, const LumPhysicalCamera* c) {
  if (!ctx) return 1;
  ctx->guides_valid = false;
  if (!c) { ctx->camera = kCamThinLens; return 0; }
  if (c->num_interfaces == 0 || c->num_interfaces > LUMC_LENS_MAX_INTERFACES) { ctx->error = "lumc_set_physical_camera: 1 ... 24 interfaces"; return 1; }
  const uint32_t n = c->num_interfaces;
  bool finite = std::isfinite(c->aperture_point) && std::isfinite(c->aperture_radius) && std::isfinite(c->exit_pupil_point) && std::isfinite(c->exit_pupil_radius) &&
                std::isfinite(c->image_plane_distance) && std::isfinite(c->sensor_width);
  bool ior_ok = true;
  for (uint32_t i = 0; i < n; i++) {
    const LumLensInterface& f = c->interfaces[i];
    finite = finite && std::isfinite(f.radius) && std::isfinite(f.vertex) && std::isfinite(f.cylindrical_radius);
  }
  for (uint32_t i = 0; i <= n; i++) {
    const LumLensMedium& m = c->media[i];
    finite = finite && std::isfinite(m.design_ior) && std::isfinite(m.abbe) && std::isfinite(m.cylindrical_radius);
    ior_ok = ior_ok && m.design_ior > 0.0f;
  }
  if (!finite) { ctx->error = "lumc_set_physical_camera: non-finite parameter"; return 1; }
  if (!(c->exit_pupil_radius > 0.0f) || !(c->aperture_radius > 0.0f)) { ctx->error = "lumc_set_physical_camera: exit pupil and aperture must be larger than 0"; return 1; }
  if (!ior_ok) { ctx->error = "lumc_set_physical_camera: index of refraction <= 0"; return 1; }
  static_assert(sizeof(LumLensInterface) == sizeof(LensInterface) && sizeof(LumLensMedium) == sizeof(LensMedium), "lens tables: one layout");
  DeviceLens l{};
  l.aperture_point = c->aperture_point; l.aperture_radius = c->aperture_radius; l.exit_pupil_point = c->exit_pupil_point; l.exit_pupil_radius = c->exit_pupil_radius;
  l.image_plane_distance = c->image_plane_distance; l.sensor_width = c->sensor_width; l.num_interfaces = n;
  std::memcpy(l.iface, c->interfaces, sizeof(LensInterface) * n);
  std::memcpy(l.medium, c->media, sizeof(LensMedium) * (n + 1));
  ctx->lens = l;
  ctx->camera = c->allow_reflections ? kCamPhysicalReflections : kCamPhysical;
  return 0;
}

int lumc_camera_rays(LumContext* ctx, const uint32_t* pixels, uint32_t n, uint32_t first_sample, uint32_t samples, float* out_origin, float* out_dir, float* out_weight) {
  if (!ctx || !ctx->has_scene || !pixels || !out_origin || !out_dir || !out_weight) { if (ctx) ctx->error = "lumc_camera_rays: no scene or null argument"; return 1; }
  const uint64_t total = (uint64_t) n * samples;
  if (total == 0) return 0;
  if (total > 0x7FFFFFFFull) { ctx->error = "lumc_camera_rays: too many rays"; return 1; }
  for (uint32_t p = 0; p < n; p++)
    if (pixels[p] >= ctx->scene.width * ctx->scene.height) { ctx->error = "lumc_camera_rays: pixel outside the frame"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  DeviceBuffer<uint32_t> d_px;
  DeviceBuffer<float> rays;  // origin[3 * total] direction[3 * total] weight[total]
  HIP_TRY(ctx, d_px.resize(n));
  HIP_TRY(ctx, rays.resize(7 * (size_t) total));
  HIP_TRY(ctx, hipMemcpy(d_px.get(), pixels, sizeof(uint32_t) * (size_t) n, hipMemcpyHostToDevice));
  float* d = rays.get();
  ctx->wf->camera_rays(grid_for((uint32_t) total), 0, ctx->scene, ctx->lens, ctx->camera, d_px.get(), n, first_sample, samples, d, d + 3 * total, d + 6 * total);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipDeviceSynchronize());
  HIP_TRY(ctx, hipMemcpy(out_origin, d, sizeof(float) * 3 * total, hipMemcpyDeviceToHost));
  HIP_TRY(ctx, hipMemcpy(out_dir, d + 3 * total, sizeof(float) * 3 * total, hipMemcpyDeviceToHost));
  HIP_TRY(ctx, hipMemcpy(out_weight, d + 6 * total, sizeof(float) * total, hipMemcpyDeviceToHost));
  return 0;
}

int lumc_device_name(int ordinal, char* out, size_t size) {
  if (!out || size == 0) return 1;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, ordinal) != hipSuccess) { out[0] = 0; return 1; }
  std::snprintf(out, size, "%s", prop.name);
  return 0;
}

int lumc_set_flavour(LumContext* ctx, int flavour) {
  if (!ctx || flavour < 0 || flavour > 1) { if (ctx) ctx->error = "lumc_set_flavour: 0 (exact) or 1 (fast)"; return 1; }
  ctx->wf = flavour == LUMC_FLAVOUR_FAST ? wavefront_kernels_fast() : wavefront_kernels_exact();
  return 0;
}
int lumc_set_fused_resolve(LumContext* ctx, int on) {
  if (!ctx) return 1;
  ctx->fused_resolve = on != 0 ? 1 : 0;
  ctx->fused_ended = on == 2 ? 0 : ctx->fused_ended_default;  // 2: the vertices whose path ended keep their own kernel (k_resolve_ended) - for comparison; 1: the context's default (LUM_FUSED_ENDED)
  return 0;
}
int lumc_set_sobol_table(LumContext* ctx, int on) {
  if (!ctx) return 1;
  ctx->sobol_table = on != 0 ? 1 : 0;
  return 0;
}
int lumc_set_ambient_reuse(LumContext* ctx, int mode) {
  if (!ctx || mode < -1 || mode > 1) { if (ctx) ctx->error = "lumc_set_ambient_reuse: -1 (by flavour), 0 (off) or 1 (on)"; return 1; }
  ctx->ambient_reuse = mode;
  return 0;
}
int lumc_get_ambient_reuse(const LumContext* ctx) { return (ctx && ambient_reuse_active(ctx)) ? 1 : 0; }
int lumc_get_flavour(const LumContext* ctx) { return (ctx && ctx->wf == wavefront_kernels_exact()) ? LUMC_FLAVOUR_EXACT : LUMC_FLAVOUR_FAST; }

unsigned int lumc_lds_stack_bytes(void) { return LUM_LDS_STACK_BYTES; }

int lumc_set_bvh_builder(LumContext* ctx, int builder) {
  if (!ctx || builder < 0 || builder > 3) { if (ctx) ctx->error = "lumc_set_bvh_builder: 0 (SAH, host), 1 (LBVH, GPU), 2 (PLOC, GPU) or 3 (SAH, GPU)"; return 1; }
  ctx->bvh_builder = builder;
  return 0;
}
double lumc_bvh_build_seconds(const LumContext* ctx) { return ctx ? ctx->bvh_build_seconds : 0.0; }
int lumc_bvh_meshes_by_builder(const LumContext* ctx, uint32_t out[2]) {
  if (!ctx || !out) return 1;
  out[0] = ctx->bvh_meshes_by_builder[0]; out[1] = ctx->bvh_meshes_by_builder[1];
  return 0;
}

int lumc_bvh_stats(LumContext* ctx, uint64_t out[4]) {
  if (!ctx) return 1;
  for (int k = 0; k < 4; k++) out[k] = ctx->bvh_stats[k];
  return 0;
}

}  // extern "C"
