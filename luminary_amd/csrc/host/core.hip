// C ABI of the path-tracing core (include/lum_core.h): the context, the work buffers, the render schedule, the adaptive sampler, the result / output / bloom /
// denoise entry points, the ray queries and the setters. The scene on the device is scene_device.hip, the ray sort ray_sort.hip, the multi-GPU exchange multi_gpu.hip.
// Host-side counterpart of the reference's device layer for the hot path only:
//   device/device.c (context, streams, constant memory), device/device_work_buffers.c:54-117 (task/result buffers),
//   device/device_renderer.c:53-134, :488-575 (per-depth kernel queue), device/device_result_interface.c (moments).
// There is deliberately no CPU fallback: every entry point fails with an error string when HIP is unavailable.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/lum_core.h"
#include "../device/kernels_shared.h"  // the flavour-neutral kernels; the wavefront kernels are csrc/device/wavefront_exact.hip and wavefront_fast.hip
#include <hipcub/hipcub.hpp>
#include "context.h"
#include "tiles.h"

static_assert(kLaunchBlock == (uint32_t) kBlock, "grid_for (context.h) counts the kernels' workgroups");

namespace {

void free_work(LumContext* ctx) {
  ctx->work = LumContext::Work{};
  ctx->fused = LumContext::Fused{};  // (its refusal too: memory may have been freed since, the next pass asks again)
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
  if (paths <= ctx->work.capacity && kinds <= ctx->work.shadow_kinds && (!clouds || ctx->work.cloud.items)) return 0;
  if (paths < ctx->work.capacity) paths = ctx->work.capacity;
  free_work(ctx);
  WorkBuffers sized;
  ArenaCarver size(nullptr);  // the first pass counts, the second points into the block
  lay_out_work(size, paths, kinds, clouds, sized);
  HIP_TRY(ctx, ctx->work.block.resize(size.used));
  ArenaCarver arena(ctx->work.block.get());
  lay_out_work(arena, paths, kinds, clouds, ctx->work);
  return 0;
}

// The six records k_shade reads the previous depth through (device memory): rewritten whenever a queue's planes move.
int upload_fused_records(LumContext* ctx, hipStream_t stream) {
  FusedResolve by_depth[6];
  for (int d = 0; d < 6; d++) {  // depth d is shaded from queue d % 3 with the records d & 1: the depth before it lives in queue (d + 2) % 3 and the other record set
    by_depth[d].prev = ctx->work.queue[(d + 2) % 3];
    by_depth[d].nee_prev = (d & 1) ? ctx->work.nee : ctx->fused.nee;
    by_depth[d].fallback = ctx->fused.fallback;
    by_depth[d].ended = ctx->fused.ended[d & 1];
    by_depth[d].ended_prev = ctx->fused.ended[(d & 1) ^ 1];
  }
  HIP_TRY(ctx, hipStreamSynchronize(stream));  // a pass still reading the old records on a non-blocking stream is not ordered against the null-stream copy below
  HIP_TRY(ctx, hipMemcpy(ctx->fused.records, by_depth, sizeof(by_depth), hipMemcpyHostToDevice));
  ctx->fused.records_stale = false;
  return 0;
}
// The fused resolve's own buffers (lay_out_fused), for as many paths as the work buffers.
int ensure_fused(LumContext* ctx, hipStream_t stream) {
  LumContext::Fused& f = ctx->fused;
  const uint32_t paths = ctx->work.capacity;
  if (f.block && f.capacity == paths) return f.records_stale ? upload_fused_records(ctx, stream) : 0;
  if (f.refused_capacity == paths) return 1;
  FusedBuffers sized;
  ArenaCarver size(nullptr);
  lay_out_fused(size, paths, ctx->work, sized);
  if (f.block.resize(size.used) != hipSuccess) { f.refused_capacity = paths; return 1; }
  ArenaCarver arena(f.block.get());
  lay_out_fused(arena, paths, ctx->work, f);
  ctx->work.queue[2] = f.queue;
  for (int k = 0; k < 3; k++) ctx->work.queue[k].parent = f.parent[k];
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

// The overlapped schedule's side stream and the register guard's verdicts (context.h; overlap_allowed below). A failure here is no error: the passes keep the serial order.
void prepare_overlap(LumContext* ctx) {
  int least = 0, greatest = 0;
  if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) least = 0;
  // the lowest priority: the ray kernel's workgroups, one per CU, get their CUs before the light queries spread over them
  if (hipStreamCreateWithPriority(&ctx->side_stream, hipStreamNonBlocking, least) != hipSuccess) ctx->side_stream = nullptr;
  for (int fast = 0; fast < 2; fast++)
    for (int single = 0; single < 2; single++) {
      uint32_t trace_regs = 0, light_query_regs = 0;
      const int e = fast ? ray_kernel_registers_fast(single != 0, &trace_regs, &light_query_regs) : ray_kernel_registers_exact(single != 0, &trace_regs, &light_query_regs);
      ctx->overlap_fits[fast][single] = e == 0 && overlap_registers_fit(trace_regs, light_query_regs);
    }
  (void) hipGetLastError();
}

// The events of the overlapped schedule, two per depth, made once and used again by every pass.
int ensure_overlap_events(LumContext* ctx, uint32_t depths) {
  while (ctx->overlap_events.size() < 2u * (size_t) depths) {
    hipEvent_t e;
    HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    ctx->overlap_events.push_back(e);
  }
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
  if (const char* e = getenv("LUM_SINGLE_LEVEL")) ctx->single_level = atoi(e) != 0 ? 1 : 0;
  if (const char* e = getenv("LUM_PLAIN_FORM")) ctx->plain_form = atoi(e) != 0 ? 1 : 0;
  if (const char* e = getenv("LUM_OVERLAP_LQ")) ctx->overlap_lq = atoi(e) != 0 ? 1 : 0;
  if (const char* e = getenv("LUM_PIXEL_MAJOR")) ctx->pixel_major = atoi(e) != 0 ? 1 : 0;
  if (const char* e = getenv("LUM_COHERENT_FIRST_HITS")) ctx->coherent_first_hits = atoi(e) != 0 ? 1 : 0;
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
  HIP_TRY(ctx, (hipError_t) wavefront_probes_exact()->init_sampler_seeds());  // the probe units' own tables (kernels_probe.h)
  HIP_TRY(ctx, (hipError_t) wavefront_probes_fast()->init_sampler_seeds());
  HIP_TRY(ctx, (hipError_t) exact::upload_sampler_seeds());  // this unit's own table: k_pixel_ray draws random numbers
  HIP_TRY(ctx, (hipError_t) scene_device_init());
  HIP_TRY(ctx, ctx->d_ctrl.resize(kCtlStride * kCtrlRows));
  HIP_TRY(ctx, hipMemset(ctx->d_ctrl.get(), 0, sizeof(uint32_t) * kCtlStride * kCtrlRows));
  HIP_TRY(ctx, ctx->d_counters.resize(LUMC_CNT_COUNT));
  HIP_TRY(ctx, hipMemset(ctx->d_counters.get(), 0, sizeof(uint64_t) * LUMC_CNT_COUNT));
  prepare_overlap(ctx);
  return 0;
}

void lumc_context_destroy(LumContext* ctx) {
  if (!ctx) return;
  (void) hipSetDevice(ctx->device);
  (void) hipDeviceSynchronize();
  resolve_stamps(ctx);
  for (hipEvent_t e : ctx->overlap_events) (void) hipEventDestroy(e);
  if (ctx->side_stream) (void) hipStreamDestroy(ctx->side_stream);
  free_exchange(ctx);
  delete ctx;
}

const char* lumc_last_error(const LumContext* ctx) { return ctx ? ctx->error.c_str() : "null context"; }
uint32_t lumc_scene_view_sizeof(void) { return (uint32_t) sizeof(LumDeviceSceneView); }

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
  ctx->firefly.planes.reset(); ctx->firefly.pixels = 0; ctx->firefly.counts = FireflyCounts{};
  ctx->num_pixels = num_pixels;
  ctx->pixels_hash = pixel_list_hash(pixels, num_pixels);  // what lumc_frame_gather checks the set against (a null list = the frame in row-major order)
  if (num_pixels == 0) return 0;
  HIP_TRY(ctx, ctx->d_pixels.assign(pixels, num_pixels));  // (no list: the frame in row-major order, and no buffer)
  HIP_TRY(ctx, ctx->d_first_moment.resize(3 * (size_t) num_pixels));
  HIP_TRY(ctx, ctx->d_second_moment.resize(num_pixels));
  if (ctx->firefly.K) {  // the buckets follow the pixel set
    ctx->firefly.pixels = num_pixels;
    HIP_TRY(ctx, ctx->firefly.planes.resize((size_t) ctx->firefly.K * 3 * num_pixels));
  }
  return lumc_clear_accumulators(ctx);
}

int lumc_clear_accumulators(LumContext* ctx) {
  if (!ctx || !ctx->d_first_moment) return 1;
  HIP_TRY(ctx, hipMemset(ctx->d_first_moment.get(), 0, sizeof(float) * 3 * (size_t) ctx->num_pixels));
  HIP_TRY(ctx, hipMemset(ctx->d_second_moment.get(), 0, sizeof(float) * (size_t) ctx->num_pixels));
  if (ctx->firefly.planes) HIP_TRY(ctx, hipMemset(ctx->firefly.planes.get(), 0, sizeof(float) * ctx->firefly.planes.count()));
  ctx->firefly.counts = FireflyCounts{};
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

// The first hits of the camera rays in queue[0], where nothing else happens between the passes (the depth loop has closest_hits and media_passes): surfaces, particles, ocean.
static void first_hits(LumContext* ctx, hipStream_t stream, const DeviceScene& sc, uint32_t N) {
  const WavefrontKernels& wf = *ctx->wf;
  {
    Launch l(ctx, stream, LUMC_KERNEL_TRACE);
    wf.trace(grid_persistent(ctx, N), ray_kernel_lds(ctx), stream, sc, ctx->work.queue[0], nullptr, ctx->d_ctrl.get(), ctx->d_counters.get(), ctx->lds_nodes, single_level_allowed(ctx), false);
  }
  if (sc.particles_active) trace_particles(ctx, stream, ctx->work.queue[0], ctx->d_ctrl.get(), N);
  if (sc.ocean_active) {
    Launch l(ctx, stream, LUMC_KERNEL_TRACE);
    wf.trace_ocean(grid_for(N), stream, sc, ctx->work.queue[0], (const uint32_t*) ctx->d_ctrl.get());
  }
}

// Debug shading modes: one closest-hit pass and a colour per path (device_renderer.c:136-181)
static void debug_pass(LumContext* ctx, hipStream_t stream, const DeviceScene& sc, uint32_t N) {
  const WavefrontKernels& wf = *ctx->wf;
  first_hits(ctx, stream, sc, N);
  if (render_volumes(sc)) {  // the debug queue keeps volume_process_events (device_renderer.c:145-147)
    Launch l(ctx, stream, LUMC_KERNEL_VOLUME);
    wf.volume_events(grid_for(N), stream, sc, ctx->work.queue[0], ctx->work.volume, ctx->work.results, ctx->d_ctrl.get(), 0u);
  }
  if (sc.sky_aerial_perspective && sc.sky_mode != kSkyConstantColor) {  // the debug queue keeps the in-scattering events (device_renderer.c:150-154)
    Launch l(ctx, stream, LUMC_KERNEL_SKY);
    wf.sky_inscattering(grid_for(N), stream, sc, ctx->work.queue[0], ctx->work.results, (const uint32_t*) ctx->d_ctrl.get(), 0u);
  }
  Launch l(ctx, stream, LUMC_KERNEL_SHADE);
  wf.shade_debug(grid_for(N), stream, sc, ctx->work.queue[0], ctx->work.results, (const uint32_t*) ctx->d_ctrl.get());
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

// The scheme the next pass asks for (kResolveFused still needs its buffers: wavefront_depths).
static ResolveScheme wanted_scheme(const LumContext* ctx) {
  if (!ambient_reuse_active(ctx)) return kResolvePlain;
  return (ctx->wf->fused_resolve && ctx->fused_resolve != 0 && ctx->wf == wavefront_kernels_fast() && ctx->scene.max_ray_depth > 0) ? kResolveFused : kResolveReuse;
}

// The overlapped schedule (wavefront_depths): k_light_query of depth d runs on the context's side stream while the caller's stream traces depth d + 1.
//   The dependency is not there: the closest-hit pass of depth d + 1 reads and writes the next queue's planes and the control words of depth d + 1, which k_shade
//   of depth d has finished; the light queries read depth d's queue and NEE records, write nee.bsdf_weight_sum and append to depth d's visibility items. The
//   depth's visibility pass needs the light queries and nothing of the next depth's hits: it runs after both. Both kernels add to the counters atomically.
//   kResolveReuse keeps the serial order (its closest_hits also resolves depth d, which needs depth d's visibility pass first), and so does everything that
//   puts a pass between the closest hits and the shading (media_passes), the ray sort (its keys and the reorder pass are ordered on one stream) and a debug mode.
//   The registers must be there (context.h overlap_registers_fit): today they are for the single-level ray kernels (4 x 96 + 112 = 496 of 512) and not for
//   the two-level ones (4 x 120 + 112), which keep the serial order launch for launch.
// kOverlapAuto: what mode -1 means - decided by measurement (profiles/overlap_lq_ab.txt, docs/HISTORY.md): hall +1.5 % samples/s against a spread of 0.2 %, k_light_query
// 2.1 -> 7.7 ms per launch but off the critical path, k_trace 13.4 -> 14.7 ms beside it.
constexpr bool kOverlapAuto = true;
static bool overlap_allowed(const LumContext* ctx, ResolveScheme scheme) {
  const DeviceScene& sc = ctx->scene;
  const bool wanted = ctx->overlap_lq < 0 ? kOverlapAuto : ctx->overlap_lq != 0;
  if (!wanted || !ctx->has_scene || !ctx->side_stream || scheme == kResolveReuse || ctx->sort.mode != 0 || sc.shading_mode != 0u || sc.max_ray_depth == 0u) return false;
  if (sc.fog_active || sc.ocean_active || sc.particles_active || sc.cloud_active || sc.sky_aerial_perspective) return false;
  return ctx->overlap_fits[ctx->wf == wavefront_kernels_fast() ? 1 : 0][(single_level_allowed(ctx) && single_level_scene(sc)) ? 1 : 0];
}

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
  return DepthBuffers{ctx->work.queue[cur], ctx->work.queue[next_q], ctx->work.queue[prev_q], second_set ? ctx->fused.nee : ctx->work.nee, second_set ? ctx->work.nee : ctx->fused.nee,
                      ctx->d_ctrl.get() + kCtlStride * depth, fused ? ctx->fused.records + depth % 6u : nullptr, fused ? ctx->fused.ended[depth & 1u] : nullptr, depth, depth_const,
                      depth == max_depth};
}

// The closest-hit launch of a depth, alone: the overlapped schedule issues it a depth early.
static void trace_depth(LumContext* ctx, hipStream_t stream, const DeviceScene& sc, const DepthBuffers& d, const uint32_t* order, uint32_t N, bool coherent = false) {
  Launch l(ctx, stream, LUMC_KERNEL_TRACE);
  ctx->wf->trace(grid_persistent(ctx, N), ray_kernel_lds(ctx), stream, sc, d.cur, order, d.ctrl, ctx->d_counters.get(), ctx->lds_nodes, single_level_allowed(ctx), coherent);
}

// The pass's slot order (lumc_render says what it is; the adaptive and the undersampling passes have their own) and, from it, the form of the depth-0 closest-hit
// launch. Pixel-major slots (kernels.h, top) put the sample ids of a pixel side by side, so that a wave of that launch holds the camera rays of one pixel (at 64 ids
// per pass) instead of one ray of 64 pixels; the coherent form of the single-level kernel (dev_trace.h trace_items<Q, true, true>) lets such a wave visit a node as
// one. A path's arithmetic does not depend on its slot, every result slot has one writer, the coherent form visits what the plain one visits: the frame moments and
// the counters keep their bits. kPixelMajorAuto, kCoherentAuto: what mode -1 means - decided by measurement (profiles/first_depth_ab.txt).
constexpr bool kPixelMajorAuto = true, kCoherentAuto = true;
static bool pixel_major_wanted(const LumContext* ctx) { return ctx->pixel_major < 0 ? kPixelMajorAuto : ctx->pixel_major != 0; }
// `forced`: asked for by name (mode 1), whatever the slot order - what lumc_trace_closest goes by, whose rays are the caller's
static bool coherent_eligible(const LumContext* ctx) { return ctx->has_scene && single_level_allowed(ctx) && single_level_scene(ctx->scene); }
static bool coherent_forced(const LumContext* ctx) { return ctx->coherent_first_hits == 1 && coherent_eligible(ctx); }
// Auto takes the form only where a wave's 64 slots ARE one pixel's rays: pixel-major slots, the thin lens (the physical camera appends only the rays that left the
// lens, so its queue is compacted and its waves straddle pixels - there a wave that waits for all its lanes before it refills has little to gain and stragglers to
// wait for). The default rests on one scene, the hall; nothing else of one instance was measured.
static bool coherent_first_hits(const LumContext* ctx, bool pixel_major) {
  return coherent_forced(ctx) || (ctx->coherent_first_hits < 0 && kCoherentAuto && pixel_major && ctx->camera == kCamThinLens && coherent_eligible(ctx));
}

// The closest hits of a depth; with kResolveReuse they also answer the ambient samples of the depth before, which is resolved here.
static int closest_hits(LumContext* ctx, hipStream_t stream, const DeviceScene& sc, ResolveScheme scheme, const DepthBuffers& d, uint32_t N, bool coherent_depth0 = false) {
  const WavefrontKernels& wf = *ctx->wf;
  // camera rays leave k_generate in pixel order, which is as coherent as rays get; later depths are sorted on request
  const uint32_t* order = nullptr;
  if (ctx->sort.mode >= 1 && d.depth >= 1 && sort_closest_rays(ctx, stream, d.cur, d.ctrl, N, &order)) return 1;
  trace_depth(ctx, stream, sc, d, order, N, coherent_depth0 && d.depth == 0u && order == nullptr);
  if (scheme == kResolveReuse && d.depth > 0) {  // the previous depth's resolve: ambient samples answered by the pass above; what it cannot answer is traced (the control words of the fog's visibility pass: no fog here) and resolved after
    uint32_t* prev = d.ctrl - kCtlStride;
    {
      Launch l(ctx, stream, LUMC_KERNEL_RESOLVE);
      wf.resolve_reuse(grid_for(N), stream, sc, d.prev, d.cur, d.nee, ctx->work.shadow, ctx->work.results, prev, ctx->d_counters.get());
    }
    {
      Launch l(ctx, stream, LUMC_KERNEL_SHADOW);
      wf.shadow_rays(ctx->trace_blocks, ray_kernel_lds(ctx), stream, sc, ctx->work.shadow, nullptr, prev + kCtlVolumeShift, ctx->d_counters.get(), ctx->lds_nodes, single_level_allowed(ctx));
    }
    Launch l(ctx, stream, LUMC_KERNEL_RESOLVE);
    wf.resolve_listed(std::min<uint32_t>(grid_for(N), 1024u), stream, sc, d.prev, d.nee, ctx->work.shadow, ctx->work.results, (const uint32_t*) prev);
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
      wf.volume_inscatter(grid_for(N), stream, sc, d.cur, ctx->work.volume, ctx->work.shadow, d.ctrl, d.depth_const);
    }
    {
      Launch l(ctx, stream, LUMC_KERNEL_SHADOW);
      wf.shadow_rays(grid_persistent(ctx, N), ray_kernel_lds(ctx), stream, sc, ctx->work.shadow, nullptr, d.ctrl + kCtlVolumeShift, ctx->d_counters.get(), ctx->lds_nodes, single_level_allowed(ctx));
    }
    Launch l(ctx, stream, LUMC_KERNEL_VOLUME);
    wf.volume_resolve(grid_for(N), stream, sc, d.cur, ctx->work.volume, ctx->work.shadow, ctx->work.results, (const uint32_t*) d.ctrl);
    wf.volume_events(grid_for(N), stream, sc, d.cur, ctx->work.volume, ctx->work.results, d.ctrl, d.depth_const);
  }
  if (sc.cloud_active && sc.sky_mode == kSkyDefault && sc.cloud_noise_shape) {  // device_manager.c:474, device_renderer.c:78-82
    Launch l(ctx, stream, LUMC_KERNEL_SKY);
    wf.clouds_list(grid_for(N), stream, sc, d.cur, ctx->work.cloud, d.ctrl);
    wf.clouds_march(ctx->trace_blocks * 4u, stream, sc, d.cur, ctx->work.cloud, d.ctrl, d.depth_const);  // persistent: 4 workgroups of 256 per CU
    wf.clouds(grid_for(N), stream, sc, d.cur, ctx->work.cloud, ctx->work.results, (const uint32_t*) d.ctrl, d.depth_const);
  }
  if (sc.sky_aerial_perspective && sc.sky_mode != kSkyConstantColor) {  // device_manager.c:475, device_renderer.c:84-88
    Launch l(ctx, stream, LUMC_KERNEL_SKY);
    wf.sky_inscattering(grid_for(N), stream, sc, d.cur, ctx->work.results, (const uint32_t*) d.ctrl, d.depth_const);
  }
}

// k_shade; with kResolveFused it resolves the depth before, and what it could not is finished here.
static void shade_depth(LumContext* ctx, hipStream_t stream, const DeviceScene& sc, ResolveScheme scheme, const DepthBuffers& d, uint32_t N) {
  const WavefrontKernels& wf = *ctx->wf;
  const bool fused = scheme == kResolveFused;
  {
    Launch l(ctx, stream, LUMC_KERNEL_SHADE);
    wf.shade(shade_grid(ctx, N), stream, sc, d.cur, d.next, d.nee, ctx->work.shadow, ctx->work.results, d.ctrl, d.depth_const, ctx->d_counters.get(),
             (scheme != kResolvePlain && !d.last) ? 1u : 0u, d.fused_records,
             fused ? ((d.depth > 0 ? 1u : 0u) | (!d.last ? 2u : 0u) | (ctx->fused_ended ? 4u : 0u)) : 0u, ctx->plain_form != 0);
  }
  if (fused && d.depth > 0) {  // the samples of depth - 1 their paths' closest hits could not decide: traced now, their vertices resolved (before this depth's visibility pass reuses the words)
    {
      Launch l(ctx, stream, LUMC_KERNEL_SHADOW);
      wf.shadow_rays(ctx->trace_blocks, ray_kernel_lds(ctx), stream, sc, ctx->fused.fallback, nullptr, d.ctrl + kCtlVolumeShift, ctx->d_counters.get(), ctx->lds_nodes, single_level_allowed(ctx));
    }
    Launch l(ctx, stream, LUMC_KERNEL_RESOLVE);
    wf.resolve_listed(std::min<uint32_t>(grid_for(N), 1024u), stream, sc, d.prev, d.nee_before, ctx->fused.fallback, ctx->work.results, (const uint32_t*) d.ctrl);
  }
}

// The shading of what k_shade leaves to others: particle hits, water-surface hits, paths that left into the procedural sky.
static void feature_shading(LumContext* ctx, hipStream_t stream, const DeviceScene& sc, const DepthBuffers& d, uint32_t N) {
  const WavefrontKernels& wf = *ctx->wf;
  if (sc.particles_active) {  // device_renderer.c:99-103
    Launch l(ctx, stream, LUMC_KERNEL_SHADE);
    wf.particle_shade(grid_for(N), stream, sc, d.cur, d.next, d.nee, ctx->work.shadow, d.ctrl, d.depth_const);
  }
  if (sc.ocean_active) {  // device_renderer.c:104-108
    Launch l(ctx, stream, LUMC_KERNEL_SHADE);
    wf.ocean_shade(grid_for(N), stream, sc, d.cur, d.next, d.nee, ctx->work.shadow, d.ctrl, d.depth_const);
  }
  if (sc.sky_mode == kSkyDefault) {  // paths that left the scene into the procedural sky (listed by k_shade)
    Launch l(ctx, stream, LUMC_KERNEL_SKY);
    wf.sky(grid_for(N), stream, sc, d.cur, ctx->work.shadow, ctx->work.results, (const uint32_t*) d.ctrl, d.depth_const);
  }
}

// The depth's light queries. `beside_trace`: on the side stream, next to the persistent closest-hit kernel of the next depth (the overlapped schedule).
static void light_queries(LumContext* ctx, hipStream_t stream, const DeviceScene& sc, const DepthBuffers& d, uint32_t N, bool beside_trace) {
  Launch l(ctx, stream, LUMC_KERNEL_LIGHT_QUERY);
  // (one resident round of its workgroups - four per CU: the kernel's workgroups are dear to start (a 1 KB stack per lane in scratch); 2 rounds, the common cap:
  //  Example-class 4.6 -> 4.0 ms per 3 steps, scan 3.9 -> 3.6, hall equal; 4 / 8 / 16 rounds on the hall: 30.2 / 32.8 / 44.5 ms against 29.9)
  // Beside the ray kernel: one workgroup per CU, one wave per SIMD - what the registers leave room for; four per CU could take a CU before the ray kernel's
  // workgroup arrives and put the two in sequence again. The kernel loops over its rounds. (Two per CU measure the same: profiles/overlap_lq_ab.txt.)
  const uint32_t per_cu = beside_trace ? 1u : 4u;
  ctx->wf->light_query(std::min<uint32_t>(grid_for(N), ctx->trace_blocks * per_cu), stream, sc, d.cur, d.nee, ctx->work.shadow, d.ctrl, d.depth_const, ctx->d_counters.get());
}

// Visibility rays, and the depth's resolve where the scheme does it at this point.
static int visibility_and_resolve(LumContext* ctx, hipStream_t stream, const DeviceScene& sc, ResolveScheme scheme, const DepthBuffers& d, uint32_t N) {
  const WavefrontKernels& wf = *ctx->wf;
  const uint32_t* shadow_order = nullptr;
  if (ctx->sort.mode == 2) {
    shadow_order = sort_rays(ctx, stream, ctx->work.shadow.origin_dist, ctx->work.shadow.dir_out, d.ctrl + kCtlShadowItems,
                             (sc.ocean_active ? kSurfaceShadowKindsWater : 4u) * (ctx->work.shadow.capacity < N ? ctx->work.shadow.capacity : N));
    if (!shadow_order) { ctx->error = "ray sorting failed"; return 1; }
  }
  {
    Launch l(ctx, stream, LUMC_KERNEL_SHADOW);
    wf.shadow_rays(grid_persistent(ctx, N), ray_kernel_lds(ctx), stream, sc, ctx->work.shadow, shadow_order, d.ctrl, ctx->d_counters.get(), ctx->lds_nodes, single_level_allowed(ctx));
  }
  if (d.last || scheme == kResolvePlain) {
    Launch l(ctx, stream, LUMC_KERNEL_RESOLVE);
    wf.resolve(grid_for(N), stream, sc, d.cur, d.nee, ctx->work.shadow, ctx->work.results, (const uint32_t*) d.ctrl);
  }
  else if (scheme == kResolveFused) {  // the vertices no entry of the next depth continues; the others are resolved by those entries, in k_shade - and so are these, as its last input (fused_flags & 4)
    if (!ctx->fused_ended) {
      Launch l(ctx, stream, LUMC_KERNEL_RESOLVE);
      wf.resolve_ended(std::min<uint32_t>(grid_for(N), 4096u), stream, sc, d.cur, d.nee, ctx->work.shadow, ctx->work.results, (const uint32_t*) d.ctrl, d.ended);
    }
  }
  // (kResolveReuse: the depth's resolve waits for the next depth's closest-hit pass, closest_hits)
  return 0;
}

static void volume_bounce(LumContext* ctx, hipStream_t stream, const DeviceScene& sc, const DepthBuffers& d, uint32_t N) {
  if (render_volumes(sc) && !d.last) {  // device_renderer.c:114-118
    Launch l(ctx, stream, LUMC_KERNEL_VOLUME);
    ctx->wf->volume_bounce(grid_for(N), stream, sc, d.cur, d.next, ctx->work.volume, d.ctrl, d.depth_const);
  }
}

// The depth loop of one wavefront pass over the paths k_generate* left in queue[0] (at most N of them, counted on the device).
// `first_sample`, `sample_count`: the pass's sample ids when they are one contiguous range for every pixel (lumc_render), 0 otherwise.
// `coherent`: the depth-0 closest-hit launch takes the coherent form (coherent_first_hits).
static int wavefront_depths(LumContext* ctx, hipStream_t stream, uint32_t N, uint32_t first_sample = 0, uint32_t sample_count = 0, bool coherent = false) {
  DeviceScene sc = ctx->scene;
  const uint32_t max_depth = sc.max_ray_depth;
  prepare_sobol_table(ctx, stream, sc, first_sample, sample_count);
  if (sc.shading_mode != 0u) { debug_pass(ctx, stream, sc, N); return 0; }
  ResolveScheme scheme = wanted_scheme(ctx);
  if (scheme == kResolveFused && ensure_fused(ctx, stream) != 0) {  // no room for its buffers (a third of the work buffers again): the separate resolve kernel does the same sums
    (void) hipGetLastError();
    ctx->error.clear();
    scheme = kResolveReuse;
  }
  // The overlapped order (overlap_allowed), chosen per pass: after a depth is shaded its light queries go to the side stream and the caller's stream traces the
  // next depth meanwhile, then waits for them before the depth's visibility pass. Depth 0's closest hits and the last depth's light queries stay on the caller's
  // stream. Every launch on the side stream is followed by a wait on the caller's, so the pass ends - for the accumulate kernel, for lumc_synchronize, for whatever
  // the caller puts on its stream next - where the serial order ends.
  const bool overlap = overlap_allowed(ctx, scheme) && ensure_overlap_events(ctx, max_depth) == 0;
  hipStream_t side = ctx->side_stream;
  bool traced = false;  // this depth's closest-hit launch was issued with the depth before
  for (uint32_t depth = 0; depth <= max_depth; depth++) {
    const DepthBuffers d = depth_buffers(ctx, scheme, depth, max_depth);
    if (!traced && closest_hits(ctx, stream, sc, scheme, d, N, coherent)) return 1;  // (overlapped: kResolvePlain or kResolveFused, no sort - closest_hits is that one launch)
    traced = false;
    media_passes(ctx, stream, sc, d, N);
    shade_depth(ctx, stream, sc, scheme, d, N);
    feature_shading(ctx, stream, sc, d, N);
    if (overlap && !d.last) {
      hipEvent_t shaded = ctx->overlap_events[2u * depth], queried = ctx->overlap_events[2u * depth + 1u];
      HIP_TRY(ctx, hipEventRecord(shaded, stream));
      HIP_TRY(ctx, hipStreamWaitEvent(side, shaded, 0));
      light_queries(ctx, side, sc, d, N, true);
      const hipError_t recorded = hipEventRecord(queried, side);
      if (recorded != hipSuccess) (void) hipStreamSynchronize(side);  // no event to wait for: the host joins the side stream before it reports the error
      HIP_TRY(ctx, recorded);
      trace_depth(ctx, stream, sc, depth_buffers(ctx, scheme, depth + 1u, max_depth), nullptr, N);
      traced = true;
      HIP_TRY(ctx, hipStreamWaitEvent(stream, queried, 0));
    }
    else light_queries(ctx, stream, sc, d, N, false);
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
  const bool buckets = !d_fm && !ctx->adaptive.active && ctx->firefly.K && ctx->firefly.planes && ctx->firefly.pixels == ctx->num_pixels;  // the context's own accumulators: its buckets too
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
    const bool pixel_major = pixel_major_wanted(ctx);
    PassParams pp{ctx->d_pixels.get(), P, batch, first_sample + done, pixel_major ? 1u : 0u};
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_ctrl.get(), 0, sizeof(uint32_t) * kCtlStride * (max_depth + 2), stream));
    {
      Launch l(ctx, stream, LUMC_KERNEL_GENERATE);
      ctx->wf->generate(grid_for(N), stream, sc, pp, ctx->work.queue[0], ctx->work.results, ctx->d_ctrl.get() + kCtlPaths, ctx->lens, ctx->camera);
    }
    // (a wave of the depth-0 launch takes 64 consecutive slots: one pixel's where the batch is a multiple of 64)
    if (wavefront_depths(ctx, stream, N, first_sample + done, batch, coherent_first_hits(ctx, pixel_major && batch % 64u == 0u))) return 1;
    {
      Launch l(ctx, stream, LUMC_KERNEL_ACCUMULATE);
      hipLaunchKernelGGL(k_accumulate, dim3(grid_for(P)), dim3(kBlock), pixel_major ? kAccTileBytes : 0u, stream, (const float4*) ctx->work.results, P, batch, d_fm, d_sm, pixel_major ? 1u : 0u);
      if (buckets) {
        HIP_TRY(ctx, firefly_accumulate_launch((const float4*) ctx->work.results, P, batch, first_sample + done, ctx->firefly.K, ctx->firefly.planes.get(), pixel_major, stream));
        ctx->firefly.take(first_sample + done, batch);
      }
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
    ctx->wf->generate(grid_for(n), stream, sc, pp, ctx->work.queue[0], ctx->work.results, ctx->d_ctrl.get() + kCtlPaths, ctx->lens, ctx->camera);
  }
  if (wavefront_depths(ctx, stream, n)) return 1;
  {
    Launch l(ctx, stream, LUMC_KERNEL_ACCUMULATE);
    hipLaunchKernelGGL(k_accumulate_scatter, dim3(grid_for(n)), dim3(kBlock), 0, stream, (const float4*) ctx->work.results, (const uint32_t*) ctx->d_undersampling_pixels.get(), n,
                       ctx->num_pixels, ctx->d_first_moment.get(), ctx->d_second_moment.get());
    if (ctx->firefly.K && ctx->firefly.planes && ctx->firefly.pixels == ctx->num_pixels) {
      HIP_TRY(ctx, firefly_scatter_launch((const float4*) ctx->work.results, (const uint32_t*) ctx->d_undersampling_pixels.get(), n, ctx->num_pixels, ctx->firefly.planes.get(), stream));
      if (stage == 1 && iteration == 0) ctx->firefly.counts.n[0]++;  // the schedule's last step: every pixel has its id 0 now
    }
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
      ctx->wf->generate_adaptive(grid_for(N), stream, sc, view, pass, ctx->work.queue[0], ctx->work.results, ctx->d_ctrl.get() + kCtlPaths, ctx->lens, ctx->camera);
    }
    if (wavefront_depths(ctx, stream, N)) return 1;
    {
      Launch l(ctx, stream, LUMC_KERNEL_ACCUMULATE);
      hipLaunchKernelGGL(k_accumulate_adaptive, dim3(grid_for((end - block) * 16)), dim3(kBlock), 0, stream, view, pass, sc.width, sc.height, (const float4*) ctx->work.results,
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

// What the result and the denoiser read: the full frame's moments - the assembled frame's (multi_gpu.hip) or this context's own accumulators - and the
// adaptive sampler's bookkeeping (none: zeros). usable: there is such a frame of n = width * height pixels.
struct FrameMoments { bool usable; const float* first; const float* second; AdaptiveView view; };
static FrameMoments frame_moments(const LumContext* ctx, uint32_t n) {
  const bool framed = ctx->exchange.use_frame && ctx->exchange.d_frame && ctx->exchange.frame_pixels() == n;
  FrameMoments m{framed || (ctx->d_first_moment && !ctx->d_pixels && ctx->num_pixels == n), framed ? ctx->exchange.d_frame.get() : ctx->d_first_moment.get(),
                 framed ? ctx->exchange.d_frame.get() + 3 * (size_t) n : ctx->d_second_moment.get(), {}};
  std::memset(&m.view, 0, sizeof(m.view));
  if (ctx->adaptive.active) m.view = adaptive_view(ctx);
  return m;
}

// The context's result image of n pixels: what lumc_generate_result* write when the caller passes no image of its own.
static int result_image(LumContext* ctx, uint32_t n, float** out) {
  if (ctx->d_frame_result.count() != 3 * (size_t) n) HIP_TRY(ctx, ctx->d_frame_result.resize(3 * (size_t) n));
  *out = ctx->d_frame_result.get();
  return 0;
}

int lumc_generate_result(LumContext* ctx, uint32_t mode, uint32_t local_error_minimization, uint32_t uniform_samples, float exposure, const LumOutputParams* tone,
                         float* d_result, void* stream_) {
  const uint32_t n = (ctx && ctx->has_scene) ? ctx->scene.width * ctx->scene.height : 0u;
  FrameMoments src{};
  if (n) src = frame_moments(ctx, n);
  if (!src.usable) {
    if (ctx) ctx->error = "lumc_generate_result: needs the full-frame accumulators";
    return 1;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t stream = (hipStream_t) stream_;
  if (!d_result && result_image(ctx, n, &d_result)) return 1;
  AdaptiveView view = src.view;
  if (!ctx->adaptive.active) { view.blocks_x = (ctx->scene.width + 3u) >> kAdaptiveBlockLog; view.blocks_y = (ctx->scene.height + 3u) >> kAdaptiveBlockLog; view.num_blocks = view.blocks_x * view.blocks_y; }
  if (!ctx->adaptive.active && uniform_samples == 0) { ctx->error = "lumc_generate_result: no samples"; return 1; }
  ResultParams rp{ctx->scene.width, ctx->scene.height, mode, local_error_minimization, uniform_samples, exposure};
  const OutputParams op = tone_params(tone);
  {
    Launch l(ctx, stream, LUMC_KERNEL_OUTPUT);
    hipLaunchKernelGGL(k_generate_result, dim3(grid_for(n)), dim3(256), 0, stream, view, rp, op, src.first, src.second, d_result);
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

static double now_seconds() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// The matte planes for a frame of n pixels and the layers asked for, every table empty: slot ids kMatteIdEmpty, counts and dropped 0.
static int begin_mattes(LumContext* ctx, const char* fn, uint32_t n, uint32_t layers, hipStream_t stream) {
  Mattes& m = ctx->mattes;
  m.valid = false; m.stale = nullptr;
  if (m.pixels != n || m.layers != layers || !m.planes) {
    m.planes.reset(); m.pixels = 0; m.layers = 0;
    const uint32_t held = (layers & 1u) + ((layers >> 1) & 1u);
    const size_t words = (size_t) held * kMatteWordsPerLayer * n;
    hipError_t e = m.planes.resize(words);
    if (e == hipSuccess && !m.d_dropped) e = m.d_dropped.resize(kMatteLayers);
    if (e != hipSuccess) {
      (void) hipGetLastError();
      m.planes.reset();
      ctx->error = std::string(fn) + ": no room for " + std::to_string(words * sizeof(uint32_t)) + " bytes of matte planes: " + hipGetErrorString(e);
      return 1;
    }
    m.pixels = n; m.layers = layers;
  }
  for (uint32_t layer = 0; layer < kMatteLayers; layer++) {
    uint32_t* planes = m.layer_planes(layer);
    if (!planes) continue;
    HIP_TRY(ctx, hipMemsetAsync(planes, 0xFF, sizeof(uint32_t) * kMatteSlots * (size_t) n, stream));
    HIP_TRY(ctx, hipMemsetAsync(planes + kMatteSlots * (size_t) n, 0, sizeof(uint32_t) * (kMatteSlots + 1u) * (size_t) n, stream));
  }
  return 0;
}

// One closest-hit pass per sample id over every pixel of the frame, and what is made of its first hits: the denoiser's guides (k_guide), the ID mattes
// (k_matte_accumulate), or both from the same rays. With guides alone this is lumc_render_guides as it always was: the same launches in the same order.
static int render_first_hits(LumContext* ctx, const char* fn, uint32_t num_samples, uint32_t what, uint32_t layers, hipStream_t stream) {
  const std::string name(fn);
  if (!ctx->has_scene) { ctx->error = name + ": no scene"; return 1; }
  if (num_samples == 0) num_samples = 4;
  if (num_samples > 1024u) { ctx->error = name + ": at most 1024 guide samples"; return 1; }
  const bool guides = (what & LUMC_FIRST_HIT_GUIDES) != 0, mattes = (what & LUMC_FIRST_HIT_MATTES) != 0, owner = (what & LUMC_FIRST_HIT_OWNER) != 0;
  if (!what || (what & ~(uint32_t) (LUMC_FIRST_HIT_GUIDES | LUMC_FIRST_HIT_MATTES | LUMC_FIRST_HIT_OWNER))) { ctx->error = name + ": what is LUMC_FIRST_HIT_GUIDES | LUMC_FIRST_HIT_MATTES | LUMC_FIRST_HIT_OWNER"; return 1; }
  if (owner && !guides) { ctx->error = name + ": LUMC_FIRST_HIT_OWNER is the owner plane of a guide render: it goes with LUMC_FIRST_HIT_GUIDES"; return 1; }
  if (mattes && (!layers || (layers & ~(uint32_t) (LUMC_MATTE_INSTANCE | LUMC_MATTE_MATERIAL)))) { ctx->error = name + ": layers is LUMC_MATTE_INSTANCE | LUMC_MATTE_MATERIAL"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  DeviceScene sc = ctx->scene;
  sc.sobol_table = nullptr;
  const uint32_t n = sc.width * sc.height;
  if (n == 0 || sc.width > 0xFFFFu || sc.height > 0xFFFFu) { ctx->error = name + ": frame size"; return 1; }
  if (guides) {
    ctx->guides_valid = false;
    ctx->history.motion.owner_cur_valid = false;  // (the plane of an earlier guide render is not this one's)
    if (guide_pixels(ctx) != n) HIP_TRY(ctx, ctx->d_guides.resize(kGuideSumPlanes * (size_t) n));
  }
  if (ensure_work(ctx, n)) return 1;
  if (guides) HIP_TRY(ctx, hipMemsetAsync(ctx->d_guides.get(), 0, sizeof(float) * kGuideSumPlanes * (size_t) n, stream));
  if (owner && history_owner_begin(ctx, fn, n, stream)) return 1;
  double t0 = 0.0;
  if (mattes) {
    if (begin_mattes(ctx, fn, n, layers, stream)) return 1;
    HIP_TRY(ctx, hipStreamSynchronize(stream));  // (the clock of lumc_matte_stats; a render of guides alone synchronises nothing)
    t0 = now_seconds();
  }
  const WavefrontKernels& wf = *ctx->wf;
  // one sample id of every pixel per pass: the closest-hit pass of the debug shading modes (wavefront_depths), then k_guide adds into the planes
  for (uint32_t s = 0; s < num_samples; s++) {
    PassParams pp{nullptr, n, 1u, s};
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_ctrl.get(), 0, sizeof(uint32_t) * kCtlStride * (sc.max_ray_depth + 2), stream));
    {
      Launch l(ctx, stream, LUMC_KERNEL_GENERATE);
      wf.generate(grid_for(n), stream, sc, pp, ctx->work.queue[0], ctx->work.results, ctx->d_ctrl.get() + kCtlPaths, ctx->lens, ctx->camera);
    }
    first_hits(ctx, stream, sc, n);
    if (guides) {
      Launch l(ctx, stream, LUMC_KERNEL_OUTPUT);
      wf.guide(grid_for(n), stream, sc, ctx->work.queue[0], (const uint32_t*) ctx->d_ctrl.get(), ctx->d_guides.get(), n);
    }
    if (owner && s == 0 && history_owner_pass(ctx, ctx->work.queue[0].hit_id, ctx->d_ctrl.get() + kCtlPaths, sc.width, n, stream)) return 1;
    if (mattes) {
      Launch l(ctx, stream, LUMC_KERNEL_MATTE);
      const PathQueue& q = ctx->work.queue[0];
      HIP_TRY(ctx, matte_accumulate_launch(q.hit_id, q.hit_scene_tri, ctx->d_ctrl.get() + kCtlPaths, sc.tri_tex, sc.width, n, ctx->mattes.layer_planes(0), ctx->mattes.layer_planes(1), stream));
    }
  }
  if (guides) {
    Launch l(ctx, stream, LUMC_KERNEL_OUTPUT);
    wf.guide_normalise(grid_for(n), stream, ctx->d_guides.get(), n, num_samples);
  }
  HIP_TRY(ctx, hipGetLastError());
  if (mattes) {
    HIP_TRY(ctx, hipStreamSynchronize(stream));
    ctx->mattes.seconds = now_seconds() - t0;
    ctx->mattes.samples = num_samples;
    ctx->mattes.valid = true;
  }
  if (guides) ctx->guides_valid = true;
  if (owner) ctx->history.motion.owner_cur_valid = true;
  return 0;
}

int lumc_render_guides(LumContext* ctx, uint32_t num_samples, void* stream) {
  if (!ctx) return 1;
  return render_first_hits(ctx, "lumc_render_guides", num_samples, LUMC_FIRST_HIT_GUIDES, 0u, (hipStream_t) stream);
}

int lumc_render_first_hits(LumContext* ctx, uint32_t num_samples, uint32_t what, uint32_t layers, void* stream) {
  if (!ctx) return 1;
  return render_first_hits(ctx, "lumc_render_first_hits", num_samples, what, layers, (hipStream_t) stream);
}

// ---- ID mattes (matte.h - the definition -, matte.hip) ----
// The layer's planes of a valid set, or null with the error set. `layer` is one LUMC_MATTE_* bit.
static const uint32_t* matte_layer(LumContext* ctx, const char* fn, uint32_t layer) {
  const Mattes& m = ctx->mattes;
  const std::string name(fn);
  if (layer != LUMC_MATTE_INSTANCE && layer != LUMC_MATTE_MATERIAL) { ctx->error = name + ": layer is LUMC_MATTE_INSTANCE or LUMC_MATTE_MATERIAL"; return nullptr; }
  if (!m.valid) {
    ctx->error = m.stale ? name + ": the mattes are stale: " + m.stale + " (lumc_render_first_hits)" : name + ": no mattes (lumc_render_first_hits)";
    return nullptr;
  }
  const uint32_t* planes = m.layer_planes(layer == LUMC_MATTE_MATERIAL ? 1u : 0u);
  if (!planes) ctx->error = name + ": the last matte render did not ask for this layer";
  return planes;
}

int lumc_download_mattes(LumContext* ctx, uint32_t layer, uint32_t ranks, uint32_t* ids, float* coverage, uint32_t* dropped, uint32_t* rays) {
  if (!ctx) return 1;
  const uint32_t* planes = matte_layer(ctx, "lumc_download_mattes", layer);
  if (!planes) return 1;
  if (ranks == 0 || ranks > kMatteSlots) { ctx->error = "lumc_download_mattes: " + std::to_string(ranks) + " ranks (1 ... 8)"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t n = ctx->mattes.pixels;
  DeviceBuffer<uint32_t> d_ids, d_dropped, d_rays;
  DeviceBuffer<float> d_coverage;
  if (ids) HIP_TRY(ctx, d_ids.resize(ranks * n));
  if (coverage) HIP_TRY(ctx, d_coverage.resize(ranks * n));
  if (dropped) HIP_TRY(ctx, d_dropped.resize(n));
  if (rays) HIP_TRY(ctx, d_rays.resize(n));
  HIP_TRY(ctx, hipDeviceSynchronize());
  {
    Launch l(ctx, nullptr, LUMC_KERNEL_MATTE);
    HIP_TRY(ctx, matte_resolve_launch(planes, (uint32_t) n, ctx->mattes.samples, ranks, d_ids.get(), d_coverage.get(), d_dropped.get(), d_rays.get(), nullptr, nullptr));
  }
  HIP_TRY(ctx, hipDeviceSynchronize());
  if (ids) HIP_TRY(ctx, hipMemcpy(ids, d_ids.get(), sizeof(uint32_t) * ranks * n, hipMemcpyDeviceToHost));
  if (coverage) HIP_TRY(ctx, hipMemcpy(coverage, d_coverage.get(), sizeof(float) * ranks * n, hipMemcpyDeviceToHost));
  if (dropped) HIP_TRY(ctx, hipMemcpy(dropped, d_dropped.get(), sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
  if (rays) HIP_TRY(ctx, hipMemcpy(rays, d_rays.get(), sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
  return 0;
}

int lumc_download_matte_tables(LumContext* ctx, uint32_t layer, uint32_t* slots_id, uint32_t* slots_count, uint32_t* dropped) {
  if (!ctx) return 1;
  const uint32_t* planes = matte_layer(ctx, "lumc_download_matte_tables", layer);
  if (!planes) return 1;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipDeviceSynchronize());
  const size_t n = ctx->mattes.pixels;
  if (slots_id) HIP_TRY(ctx, hipMemcpy(slots_id, planes, sizeof(uint32_t) * kMatteSlots * n, hipMemcpyDeviceToHost));
  if (slots_count) HIP_TRY(ctx, hipMemcpy(slots_count, planes + kMatteSlots * n, sizeof(uint32_t) * kMatteSlots * n, hipMemcpyDeviceToHost));
  if (dropped) HIP_TRY(ctx, hipMemcpy(dropped, planes + 2u * kMatteSlots * n, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
  return 0;
}

int lumc_matte_mask(LumContext* ctx, uint32_t layer, const uint32_t* ids, uint32_t count, float* d_mask, void* stream_) {
  if (!ctx) return 1;
  const uint32_t* planes = matte_layer(ctx, "lumc_matte_mask", layer);
  if (!planes) return 1;
  if (!d_mask || (count && !ids)) { ctx->error = "lumc_matte_mask: null argument"; return 1; }
  if (count > kMatteMaxMaskIds) { ctx->error = "lumc_matte_mask: " + std::to_string(count) + " ids (at most 16)"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t stream = (hipStream_t) stream_;
  MatteIdList list{};
  list.count = count;
  for (uint32_t i = 0; i < count; i++) list.id[i] = ids[i];
  Launch l(ctx, stream, LUMC_KERNEL_MATTE);
  HIP_TRY(ctx, matte_mask_launch(planes, ctx->mattes.pixels, ctx->mattes.samples, list, d_mask, stream));
  return 0;
}

int lumc_matte_mask_host(LumContext* ctx, uint32_t layer, const uint32_t* ids, uint32_t count, float* mask) {
  if (!ctx || !mask) { if (ctx) ctx->error = "lumc_matte_mask_host: null argument"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  DeviceBuffer<float> d;
  HIP_TRY(ctx, d.resize(std::max<size_t>(ctx->mattes.pixels, 1)));
  if (lumc_matte_mask(ctx, layer, ids, count, d.get(), nullptr)) return 1;
  HIP_TRY(ctx, hipDeviceSynchronize());
  HIP_TRY(ctx, hipMemcpy(mask, d.get(), sizeof(float) * ctx->mattes.pixels, hipMemcpyDeviceToHost));
  return 0;
}

int lumc_has_mattes(const LumContext* ctx) { return (ctx && ctx->mattes.valid) ? 1 : 0; }

int lumc_matte_release(LumContext* ctx) {
  if (!ctx) return 1;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipDeviceSynchronize());
  ctx->mattes = Mattes{};
  return 0;
}

int lumc_matte_stats(LumContext* ctx, LumMatteStats* out) {
  if (!ctx || !out) return 1;
  const Mattes& m = ctx->mattes;
  std::memset(out, 0, sizeof(*out));
  out->bytes = sizeof(uint32_t) * (uint64_t) m.planes.count();
  out->layers = m.layers;
  out->valid = m.valid ? 1u : 0u;
  if (!m.valid) return 0;
  out->samples = m.samples;
  out->seconds = m.seconds;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipDeviceSynchronize());
  HIP_TRY(ctx, hipMemset(m.d_dropped.get(), 0, sizeof(uint32_t) * kMatteLayers));
  for (uint32_t layer = 0; layer < kMatteLayers; layer++)
    if (const uint32_t* planes = m.layer_planes(layer)) {
      Launch l(ctx, nullptr, LUMC_KERNEL_MATTE);
      HIP_TRY(ctx, matte_resolve_launch(planes, m.pixels, m.samples, 1u, nullptr, nullptr, nullptr, nullptr, m.d_dropped.get() + layer, nullptr));
    }
  HIP_TRY(ctx, hipDeviceSynchronize());
  HIP_TRY(ctx, hipMemcpy(out->dropped_pixels, m.d_dropped.get(), sizeof(uint32_t) * kMatteLayers, hipMemcpyDeviceToHost));
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
  const FrameMoments src = frame_moments(ctx, n);
  if (!src.usable) { ctx->error = "lumc_denoise: needs the full-frame accumulators"; return 1; }
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
  DenoiseArgs args{ctx->scene.width, ctx->scene.height, 1u, params->uniform_samples, params->sigma_luminance, params->sigma_normal, params->sigma_depth};
  const uint32_t iterations = std::min(params->iterations, 6u);
  float4* rec_a[2] = {ctx->d_denoise_rec[0].get(), ctx->d_denoise_rec[1].get()};
  uint4* rec_b = (uint4*) ctx->d_denoise_rec[2].get();
  const WavefrontKernels& wf = *ctx->wf;
  Launch l(ctx, stream, LUMC_KERNEL_OUTPUT);
  wf.denoise_prepare(grid_for(n), stream, src.view, args, src.first, src.second, d_image, ctx->d_guides.get(), rec_a[0], rec_b);
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

// ---- firefly rejection (firefly.h, firefly.hip) ----
int lumc_set_firefly_buckets(LumContext* ctx, uint32_t K) {
  if (!ctx) return 1;
  if (K != 0 && (K < kFireflyMinBuckets || K > kFireflyMaxBuckets)) {
    ctx->error = "lumc_set_firefly_buckets: " + std::to_string(K) + " buckets (0: off, or 4 ... 16)";
    return 1;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  DeviceBuffer<float> planes;
  DeviceBuffer<uint32_t> stats;
  const size_t floats = (size_t) K * 3 * ctx->num_pixels;
  if (K) {
    hipError_t e = planes.resize(ctx->d_first_moment ? floats : 0);
    if (e == hipSuccess) e = stats.resize(3);
    if (e != hipSuccess) {  // (the context's planes are still what they were)
      (void) hipGetLastError();
      ctx->error = "lumc_set_firefly_buckets: no room for " + std::to_string(floats * sizeof(float)) + " bytes of bucket planes: " + hipGetErrorString(e);
      return 1;
    }
  }
  ctx->firefly.planes = std::move(planes);
  ctx->firefly.d_stats = std::move(stats);
  ctx->firefly.K = K;
  ctx->firefly.pixels = ctx->firefly.planes ? ctx->num_pixels : 0u;
  ctx->firefly.counts = FireflyCounts{};
  return ctx->d_first_moment ? lumc_clear_accumulators(ctx) : 0;
}

int lumc_firefly_resolve(LumContext* ctx, float* d_image, void* stream_) {
  if (!ctx) return 1;
  FireflyBuckets& f = ctx->firefly;
  if (!f.K || !f.planes) { ctx->error = "lumc_firefly_resolve: no buckets (lumc_set_firefly_buckets)"; return 1; }
  if (ctx->adaptive.active) { ctx->error = "lumc_firefly_resolve: adaptive accumulation is active, its passes fill no buckets"; return 1; }
  const uint32_t n = ctx->has_scene ? ctx->scene.width * ctx->scene.height : 0u;
  if (!n || ctx->d_pixels || ctx->num_pixels != n || f.pixels != n) { ctx->error = "lumc_firefly_resolve: the image is not of the context's pixel set: the buckets need the full frame (lumc_set_pixels(ctx, NULL, 0))"; return 1; }
  if (!f.any()) { ctx->error = "lumc_firefly_resolve: no bucket has samples"; return 1; }
  if (!d_image) {
    if (ctx->d_frame_result.count() != 3 * (size_t) n) { ctx->error = "lumc_firefly_resolve: no result image (lumc_generate_result)"; return 1; }
    d_image = ctx->d_frame_result.get();
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t stream = (hipStream_t) stream_;
  HIP_TRY(ctx, hipMemsetAsync(f.d_stats.get(), 0, sizeof(uint32_t) * 3, stream));
  {
    Launch l(ctx, stream, LUMC_KERNEL_OUTPUT);
    HIP_TRY(ctx, firefly_resolve_launch(f.planes.get(), f.counts, f.K, n, d_image, f.d_stats.get(), stream));
  }
  f.resolves++;
  return 0;
}

int lumc_download_buckets(LumContext* ctx, float* sums, uint32_t* counts) {
  if (!ctx) return 1;
  const FireflyBuckets& f = ctx->firefly;
  if (!f.K || !f.planes) { ctx->error = "lumc_download_buckets: no buckets (lumc_set_firefly_buckets)"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipDeviceSynchronize());
  if (sums) HIP_TRY(ctx, hipMemcpy(sums, f.planes.get(), sizeof(float) * f.planes.count(), hipMemcpyDeviceToHost));
  if (counts) std::memcpy(counts, f.counts.n, sizeof(uint32_t) * f.K);
  return 0;
}

int lumc_upload_buckets(LumContext* ctx, const float* sums, const uint32_t* counts) {
  if (!ctx) return 1;
  FireflyBuckets& f = ctx->firefly;
  if (!f.K || !f.planes) { ctx->error = "lumc_upload_buckets: no buckets (lumc_set_firefly_buckets)"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipDeviceSynchronize());
  if (sums) HIP_TRY(ctx, hipMemcpy(f.planes.get(), sums, sizeof(float) * f.planes.count(), hipMemcpyHostToDevice));
  if (counts) std::memcpy(f.counts.n, counts, sizeof(uint32_t) * f.K);
  return 0;
}

int lumc_firefly_stats(LumContext* ctx, LumFireflyStats* out) {
  if (!ctx || !out) return 1;
  const FireflyBuckets& f = ctx->firefly;
  std::memset(out, 0, sizeof(*out));
  out->buckets = f.K;
  out->bytes = sizeof(float) * (uint64_t) f.planes.count();
  out->resolves = f.resolves;
  for (uint32_t b = 0; b < f.K; b++) out->samples += f.counts.n[b];
  if (f.d_stats && f.resolves) {
    uint32_t st[3];
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipDeviceSynchronize());
    HIP_TRY(ctx, hipMemcpy(st, f.d_stats.get(), sizeof(st), hipMemcpyDeviceToHost));
    out->last_rewritten = st[0]; out->last_trimmed = st[1]; out->last_nonfinite = st[2];
  }
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
                      ctx->lds_nodes, single_level_allowed(ctx), coherent_forced(ctx));
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
    ctx->wf->shadow_rays(grid_persistent(ctx, n), ray_kernel_lds(ctx), stream, ctx->scene, sq, d_order, ctrl, ctx->d_counters.get(), ctx->lds_nodes, single_level_allowed(ctx));
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

// The number of paths every depth of the LAST pass held (the control words' kCtlPaths, zeroed when a pass begins): out[d] for d < min(count, max_ray_depth + 2).
// Read-only; waits for the device.
int lumc_last_pass_path_counts(LumContext* ctx, uint32_t count, uint32_t* out) {
  if (!ctx || !ctx->has_scene || !out) { if (ctx) ctx->error = "lumc_last_pass_path_counts: no scene or null argument"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipDeviceSynchronize());
  const uint32_t rows = std::min(std::min(count, ctx->scene.max_ray_depth + 2u), kCtrlRows - 2u);
  for (uint32_t d = 0; d < count; d++) out[d] = 0u;
  for (uint32_t d = 0; d < rows; d++) HIP_TRY(ctx, hipMemcpy(out + d, ctx->d_ctrl.get() + kCtlStride * d + kCtlPaths, sizeof(uint32_t), hipMemcpyDeviceToHost));
  return 0;
}

// The particle pass on caller-made queue entries through the render's own kernel: a temporary PathQueue filled on the host (no kernel of the probe's own), the
// item count and the work cursor in the spare control row, the active flavour's k_trace_particles launched by trace_particles as a pass launches it. The hit words
// start as LUMC_PARTICLE_PROBE_UNTOUCHED, so an item that nobody answered - or that the kernel does not trace - shows.
int lumc_trace_particles_probe_host(LumContext* ctx, uint32_t n, const float* origins, const float* dirs, const float* tmax, const uint32_t* states, const uint32_t* pixel_samples,
                                    float* out_t, uint32_t* out_hit) {
  if (!ctx || !ctx->has_scene) { if (ctx) ctx->error = "lumc_trace_particles_probe_host: no scene"; return 1; }
  if (n == 0) return 0;
  if (!origins || !dirs || !tmax || !states || !pixel_samples || !out_t || !out_hit) { ctx->error = "lumc_trace_particles_probe_host: null argument"; return 1; }
  if (!ctx->scene.particles_active || !ctx->scene.particle_bvh_nodes) { ctx->error = "lumc_trace_particles_probe_host: the scene has no particles"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::vector<float4> h_origin_t(n), h_dir_slot(n);
  std::vector<uint4> h_aux(n), h_hit_id(n);
  for (uint32_t i = 0; i < n; i++) {
    h_origin_t[i] = make_float4(origins[3 * (size_t) i], origins[3 * (size_t) i + 1], origins[3 * (size_t) i + 2], tmax[i]);
    h_dir_slot[i] = make_float4(dirs[3 * (size_t) i], dirs[3 * (size_t) i + 1], dirs[3 * (size_t) i + 2], 0.0f);
    h_aux[i] = make_uint4(0u, 0u, 0u, states[i]);
    const uint32_t* ps = pixel_samples + 3 * (size_t) i;
    h_hit_id[i] = make_uint4(LUMC_PARTICLE_PROBE_UNTOUCHED, 0u, (ps[0] & 0xFFFFu) | (ps[1] << 16), ps[2]);
  }
  DeviceBuffer<float4> d_origin_t, d_dir_slot;
  DeviceBuffer<uint4> d_aux, d_hit_id;
  HIP_TRY(ctx, d_origin_t.assign(h_origin_t.data(), n));
  HIP_TRY(ctx, d_dir_slot.assign(h_dir_slot.data(), n));
  HIP_TRY(ctx, d_aux.assign(h_aux.data(), n));
  HIP_TRY(ctx, d_hit_id.assign(h_hit_id.data(), n));
  PathQueue q{};
  q.origin_t = d_origin_t.get(); q.dir_slot = d_dir_slot.get(); q.aux = d_aux.get(); q.hit_id = d_hit_id.get();
  uint32_t* ctrl = ctx->d_ctrl.get() + kCtlStride * (kCtrlRows - 2);
  HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t) (ctrl + kCtlPaths), (int) n, 1, nullptr));
  HIP_TRY(ctx, hipMemsetAsync(ctrl + kCtlParticleCursor, 0, sizeof(uint32_t), nullptr));
  trace_particles(ctx, nullptr, q, ctrl, n);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipDeviceSynchronize());
  HIP_TRY(ctx, hipMemcpy(h_origin_t.data(), d_origin_t.get(), sizeof(float4) * (size_t) n, hipMemcpyDeviceToHost));
  HIP_TRY(ctx, hipMemcpy(h_hit_id.data(), d_hit_id.get(), sizeof(uint4) * (size_t) n, hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < n; i++) { out_t[i] = h_origin_t[i].w; out_hit[i] = h_hit_id[i].x; }
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
  // What was rendered from the first hits - the denoiser's guides, the ID mattes - is dropped when the camera changes. A host sets the camera on every use
  // (api.cpp set_camera): the camera it already had is no change. (A refused camera drops them too.)
  const char* changed = "the camera's lens was set since (lumc_set_physical_camera)";
  if (!c) {
    if (ctx->camera != kCamThinLens) ctx->drop_first_hit_products(changed);
    ctx->camera = kCamThinLens;
    return 0;
  }
  struct DropUnlessSame {
    LumContext* ctx; const char* why; bool same = false;
    ~DropUnlessSame() { if (!same) ctx->drop_first_hit_products(why); }
  } drop{ctx, changed};
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
  const int kind = c->allow_reflections ? kCamPhysicalReflections : kCamPhysical;
  drop.same = ctx->camera == kind && std::memcmp(&ctx->lens, &l, sizeof(l)) == 0;
  if (!drop.same) ctx->lens = l;
  ctx->camera = kind;
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

int lumc_set_single_level(LumContext* ctx, int mode) {
  if (!ctx || mode < -1 || mode > 1) { if (ctx) ctx->error = "lumc_set_single_level: -1 (auto), 0 (never) or 1 (when the scene is eligible)"; return 1; }
  ctx->single_level = mode;
  return 0;
}
// what the launchers will decide for the uploaded scene's surfaces (the particle pass has no single-level form)
int lumc_get_single_level(const LumContext* ctx) { return (ctx && ctx->has_scene && single_level_allowed(ctx) && single_level_scene(ctx->scene)) ? 1 : 0; }

int lumc_set_plain_form(LumContext* ctx, int mode) {
  if (!ctx || mode < -1 || mode > 1) { if (ctx) ctx->error = "lumc_set_plain_form: -1 (auto), 0 (never) or 1 (when the scene is eligible)"; return 1; }
  ctx->plain_form = mode;
  return 0;
}

int lumc_get_plain_form(const LumContext* ctx) { return (ctx && ctx->has_scene && ctx->plain_form != 0 && plain_scene(ctx->scene)) ? 1 : 0; }

int lumc_set_overlap_light_query(LumContext* ctx, int mode) {
  if (!ctx || mode < -1 || mode > 1) { if (ctx) ctx->error = "lumc_set_overlap_light_query: -1 (auto), 0 (never) or 1 (when the pass allows it)"; return 1; }
  ctx->overlap_lq = mode;
  return 0;
}
// what the next pass will do for the uploaded scene (a fused resolve that finds no room for its buffers falls back to the reuse scheme and the serial order)
int lumc_get_overlap_light_query(const LumContext* ctx) { return (ctx && ctx->has_scene && overlap_allowed(ctx, wanted_scheme(ctx))) ? 1 : 0; }
int lumc_set_pixel_major(LumContext* ctx, int mode) {
  if (!ctx || mode < -1 || mode > 1) { if (ctx) ctx->error = "lumc_set_pixel_major: -1 (auto), 0 (sample-major slots) or 1 (pixel-major slots)"; return 1; }
  ctx->pixel_major = mode;
  return 0;
}
int lumc_get_pixel_major(const LumContext* ctx) { return (ctx && pixel_major_wanted(ctx)) ? 1 : 0; }
int lumc_set_coherent_first_hits(LumContext* ctx, int mode) {
  if (!ctx || mode < -1 || mode > 1) { if (ctx) ctx->error = "lumc_set_coherent_first_hits: -1 (auto), 0 (never) or 1 (when the scene is eligible)"; return 1; }
  ctx->coherent_first_hits = mode;
  return 0;
}
// what the depth-0 launch of the next lumc_render will be for the uploaded scene, at a batch that is a multiple of 64
int lumc_get_coherent_first_hits(const LumContext* ctx) { return (ctx && coherent_first_hits(ctx, pixel_major_wanted(ctx))) ? 1 : 0; }
int lumc_overlap_registers_fit(uint32_t ray_kernel_regs, uint32_t light_query_regs) { return overlap_registers_fit(ray_kernel_regs, light_query_regs) ? 1 : 0; }
int lumc_get_flavour(const LumContext* ctx) { return (ctx && ctx->wf == wavefront_kernels_exact()) ? LUMC_FLAVOUR_EXACT : LUMC_FLAVOUR_FAST; }

unsigned int lumc_lds_stack_bytes(void) { return LUM_LDS_STACK_BYTES; }

}  // extern "C"
