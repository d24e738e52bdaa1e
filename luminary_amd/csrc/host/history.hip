// Image history on the device (lumc_set_history, lumc_history_carry, lumc_history_blend): the state of the last shown frame gathered into the
// moved camera, and the blend of the carried plane with the new result image. The arithmetic is history.h's history_reproject_pixel and history_blend_pixel, the
// same source the host twins (history.cpp) are compiled from; this unit is compiled without contraction like that one, with IEEE divide and square root: both give
// the same bytes (tests/test_history_gpu.py). A unit of its own beside the output chain; no kernel of the renderer is touched.
//
//   k_history_reproject  one thread per pixel of the new frame, workgroups of 32 x 8 pixels: a wave holds two rows of 32, and a smooth motion field sends them to a
//                        few rows of the old frame, so the four taps of neighbouring lanes share their 64-byte lines in L2. A tap is two 16-byte loads, the guide
//                        record first: a tap it refuses never loads the shown record. The four taps unroll; nothing is indexed at run time. 28 bytes of guides in,
//                        16 out, and the gather's share of the 32-byte state. Three counters, each reduced across the wave, one atomic per wave and counter - into
//                        one of kHistoryStatStripes copies of the counters, a cache line each, which the host adds up: the 32 400 waves of a 1080p frame adding to ONE
//                        line took 0.464 ms, with the copies the kernel takes 0.039 ms (docs/HISTORY.md).
//   k_history_blend      one thread per pixel, the same tiles. 12 bytes of image, 16 of carried plane and 16 of guides in; 12 of image and 32 of state out. With
//                        the clamp it reads the 3 x 3 neighbourhood of a COPY of the image (the kernel writes the image it blends) from a 34 x 10 tile per channel
//                        staged in LDS (4080 bytes); the form that read the nine taps from global memory was slower and is gone (docs/HISTORY.md).
//
// Motion (lumc_set_history_motion; history.h "Motion"): three more kernels, launched only while that switch is on; the two above are what they were.
//   k_history_owner             one thread per path of the closest-hit pass of sample id 0, grid-stride, reading hit_id as k_matte_accumulate does: 16 bytes in, 4 out.
//   k_history_motion            one thread per instance: 32 + 32 bytes of transforms in, one 128-byte record out; the binary64 inverses are here, once per instance and
//                               carry, never per pixel. Three counters reduced per wave.
//   k_history_reproject_motion  k_history_reproject's shape - 32 x 8 tiles, taps unrolled, the guide record of a tap before its owner before its shown record, the
//                               counters (five now) into the 32 striped lines. A pixel loads its owner (4 bytes) and, for an instance id, the class word of its
//                               record; only lanes whose owner is MOVED load the record's line. A tap that passed its guide test costs 4 bytes of old owner, and the
//                               class word of that owner's record where it differs from the pixel's.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "context.h"

namespace lum {
namespace {

constexpr uint32_t kHistoryBlock = kHistoryTileX * kHistoryTileY;
constexpr uint32_t kHaloX = kHistoryTileX + 2u, kHaloY = kHistoryTileY + 2u;

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (uint32_t d = 32u; d > 0u; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

__global__ __launch_bounds__(kHistoryBlock) void k_history_reproject(HistoryKey now, HistoryKey old, HistorySettings st, const float* __restrict__ guides,
                                                                     const HistoryRec* __restrict__ shown, const HistoryRec* __restrict__ guide, HistoryRec* __restrict__ carried,
                                                                     uint32_t* stats) {
  const uint32_t x = blockIdx.x * kHistoryTileX + (threadIdx.x & (kHistoryTileX - 1u)), y = blockIdx.y * kHistoryTileY + threadIdx.x / kHistoryTileX;
  uint32_t cls = 3u;  // no pixel: counted nowhere; every lane stays for the wave's sums
  if (x < now.width && y < now.height) {
    const size_t n = (size_t) now.width * now.height, p = (size_t) y * now.width + x;
    const HistoryV3 n_cur = {guides[3 * n + p], guides[4 * n + p], guides[5 * n + p]};
    const float d_cur = guides[6 * n + p];
    HistoryRec out;
    cls = history_reproject_pixel(
        now, old, st, x, y, n_cur, d_cur, [&](uint32_t tx, uint32_t ty) { return shown[(size_t) ty * old.width + tx]; },
        [&](uint32_t tx, uint32_t ty) { return guide[(size_t) ty * old.width + tx]; }, out);
    carried[p] = out;
  }
  const uint32_t c0 = wave_sum(cls == kHistoryCarried ? 1u : 0u), c1 = wave_sum(cls == kHistoryRejected ? 1u : 0u), c2 = wave_sum(cls == kHistoryOff ? 1u : 0u);
  if ((threadIdx.x & 63u) == 0u) {
    uint32_t* mine = stats + ((blockIdx.x + blockIdx.y * 5u) & (kHistoryStatStripes - 1u)) * kHistoryStatStride;
    if (c0) atomicAdd(mine + 0, c0);
    if (c1) atomicAdd(mine + 1, c1);
    if (c2) atomicAdd(mine + 2, c2);
  }
}

// cur: the image the blend reads (== image without the clamp). carried may be null.
template <bool kClamp>
__global__ __launch_bounds__(kHistoryBlock) void k_history_blend(HistorySettings st, uint32_t width, uint32_t height, float N, const float* cur, const HistoryRec* __restrict__ carried,
                                                                 const float* __restrict__ guides, float* image, HistoryRec* __restrict__ shown_out, HistoryRec* __restrict__ guide_out) {
  const uint32_t x0 = blockIdx.x * kHistoryTileX, y0 = blockIdx.y * kHistoryTileY;
  const uint32_t x = x0 + (threadIdx.x & (kHistoryTileX - 1u)), y = y0 + threadIdx.x / kHistoryTileX;
  const size_t n = (size_t) width * height;
  __shared__ float tile[kClamp ? 3u * kHaloX * kHaloY : 1u];
  if constexpr (kClamp) {
    // the tile and its one-pixel halo, channel by channel; entries outside the frame are never read (the definition asks only for taps inside it)
    for (uint32_t e = threadIdx.x; e < 3u * kHaloX * kHaloY; e += kHistoryBlock) {
      const uint32_t ch = e / (kHaloX * kHaloY), r = e % (kHaloX * kHaloY);
      const int32_t gx = (int32_t) (x0 + r % kHaloX) - 1, gy = (int32_t) (y0 + r / kHaloX) - 1;
      if (gx >= 0 && gy >= 0 && gx < (int32_t) width && gy < (int32_t) height) tile[e] = cur[(size_t) ch * n + (size_t) gy * width + (uint32_t) gx];
    }
    __syncthreads();
  }
  if (x >= width || y >= height) return;
  const size_t p = (size_t) y * width + x;
  HistorySettings s = st;
  if constexpr (!kClamp) s.clamp_sigma = 0.0f;
  const HistoryRec c = carried ? carried[p] : HistoryRec{0.0f, 0.0f, 0.0f, 0.0f};
  HistoryRec shown;
  bool written;
  if constexpr (kClamp)
    written = history_blend_pixel(s, width, height, x, y, N, c, [&](uint32_t tx, uint32_t ty, uint32_t ch) { return tile[ch * (kHaloX * kHaloY) + (ty + 1u - y0) * kHaloX + (tx + 1u - x0)]; }, shown);
  else
    written = history_blend_pixel(s, width, height, x, y, N, c, [&](uint32_t tx, uint32_t ty, uint32_t ch) { return cur[(size_t) ch * n + (size_t) ty * width + tx]; }, shown);
  if (written) { image[p] = shown.x; image[n + p] = shown.y; image[2 * n + p] = shown.z; }
  shown_out[p] = shown;
  guide_out[p] = HistoryRec{guides[3 * n + p], guides[4 * n + p], guides[5 * n + p], guides[6 * n + p]};
}

// The first hits of sample id 0 as owner ids; the plane was preset to kMatteIdEmpty.
__global__ __launch_bounds__(kHistoryBlock) void k_history_owner(const uint4* __restrict__ hit_id, const uint32_t* __restrict__ paths_word, uint32_t width, uint32_t n,
                                                                 uint32_t* __restrict__ owner) {
  const uint32_t paths = *paths_word;
  for (uint32_t i = blockIdx.x * kHistoryBlock + threadIdx.x; i < paths; i += gridDim.x * kHistoryBlock) {
    const uint4 hid = hit_id[i];
    const uint32_t p = (hid.z & 0xFFFFu) + (hid.z >> 16) * width;  // as k_guide and k_matte_accumulate
    if (p >= n) continue;
    owner[p] = matte_sample_id(matte_classify(hid.x), hid.x);
  }
}

__global__ __launch_bounds__(kHistoryBlock) void k_history_motion(const float4* __restrict__ old_t, const float4* __restrict__ new_t, uint32_t count, HistoryMotion* __restrict__ records,
                                                                  uint32_t* counts) {
  const uint32_t i = blockIdx.x * kHistoryBlock + threadIdx.x;
  uint32_t cls = 3u;  // no instance: counted nowhere; every lane stays for the wave's sums
  if (i < count) {
    const float4 o0 = old_t[2 * (size_t) i], o1 = old_t[2 * (size_t) i + 1], n0 = new_t[2 * (size_t) i], n1 = new_t[2 * (size_t) i + 1];
    const float o[8] = {o0.x, o0.y, o0.z, o0.w, o1.x, o1.y, o1.z, o1.w}, w[8] = {n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, n1.z, n1.w};
    const HistoryMotion r = history_motion_record(o, w);
    records[i] = r;
    cls = r.cls;
  }
  const uint32_t c0 = wave_sum(cls == kHistoryMotionMoved ? 1u : 0u), c1 = wave_sum(cls == kHistoryMotionSame ? 1u : 0u), c2 = wave_sum(cls == kHistoryMotionVoid ? 1u : 0u);
  if ((threadIdx.x & 63u) == 0u) {
    if (c0) atomicAdd(counts + 0, c0);
    if (c1) atomicAdd(counts + 1, c1);
    if (c2) atomicAdd(counts + 2, c2);
  }
}

__global__ __launch_bounds__(kHistoryBlock) void k_history_reproject_motion(HistoryKey now, HistoryKey old, HistorySettings st, float motion_max_history, const float* __restrict__ guides,
                                                                            const HistoryRec* __restrict__ shown, const HistoryRec* __restrict__ guide,
                                                                            const uint32_t* __restrict__ owner, const uint32_t* __restrict__ old_owner,
                                                                            const HistoryMotion* __restrict__ records, uint32_t count, HistoryRec* __restrict__ carried, uint32_t* stats) {
  const uint32_t x = blockIdx.x * kHistoryTileX + (threadIdx.x & (kHistoryTileX - 1u)), y = blockIdx.y * kHistoryTileY + threadIdx.x / kHistoryTileX;
  uint32_t cls = 3u;
  bool moved = false;
  if (x < now.width && y < now.height) {
    const size_t n = (size_t) now.width * now.height, p = (size_t) y * now.width + x;
    const HistoryV3 n_cur = {guides[3 * n + p], guides[4 * n + p], guides[5 * n + p]};
    const float d_cur = guides[6 * n + p];
    HistoryRec out;
    cls = history_reproject_pixel_motion(
        now, old, st, motion_max_history, x, y, n_cur, d_cur, owner[p], count, [&](uint32_t tx, uint32_t ty) { return shown[(size_t) ty * old.width + tx]; },
        [&](uint32_t tx, uint32_t ty) { return guide[(size_t) ty * old.width + tx]; }, [&](uint32_t tx, uint32_t ty) { return old_owner[(size_t) ty * old.width + tx]; },
        [&](uint32_t id) { return records[id].cls; }, [&](uint32_t id) { return records[id]; }, out, moved);
    carried[p] = out;
  }
  const uint32_t c0 = wave_sum(cls == kHistoryCarried ? 1u : 0u), c1 = wave_sum(cls == kHistoryRejected ? 1u : 0u), c2 = wave_sum(cls == kHistoryOff ? 1u : 0u);
  const uint32_t c3 = wave_sum(moved ? 1u : 0u), c4 = wave_sum(moved && cls == kHistoryCarried ? 1u : 0u);
  if ((threadIdx.x & 63u) == 0u) {
    uint32_t* mine = stats + ((blockIdx.x + blockIdx.y * 5u) & (kHistoryStatStripes - 1u)) * kHistoryStatStride;
    if (c0) atomicAdd(mine + 0, c0);
    if (c1) atomicAdd(mine + 1, c1);
    if (c2) atomicAdd(mine + 2, c2);
    if (c3) atomicAdd(mine + kHistoryStatMoved, c3);
    if (c4) atomicAdd(mine + kHistoryStatMovedCarried, c4);
  }
}

inline dim3 history_grid(uint32_t width, uint32_t height) { return dim3((width + kHistoryTileX - 1u) / kHistoryTileX, (height + kHistoryTileY - 1u) / kHistoryTileY); }
inline bool frame_ok(uint32_t width, uint32_t height) { return width > 0 && height > 0 && width <= 0xFFFFu && height <= 0xFFFFu; }

}  // namespace

hipError_t history_reproject_launch(const HistoryKey& now, const HistoryKey& old, const HistorySettings& st, const float* d_guides, const HistoryRec* d_shown, const HistoryRec* d_guide,
                                    HistoryRec* d_carried, uint32_t* d_stats, hipStream_t stream) {
  if (!d_guides || !d_shown || !d_guide || !d_carried || !d_stats || !frame_ok(now.width, now.height) || !frame_ok(old.width, old.height)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_history_reproject, history_grid(now.width, now.height), dim3(kHistoryBlock), 0, stream, now, old, st, d_guides, d_shown, d_guide, d_carried, d_stats);
  return hipGetLastError();
}

hipError_t history_blend_launch(const HistorySettings& st, uint32_t width, uint32_t height, uint32_t uniform_samples, const float* d_cur, const HistoryRec* d_carried, const float* d_guides,
                                float* d_image, HistoryRec* d_shown, HistoryRec* d_guide, hipStream_t stream) {
  if (!d_cur || !d_guides || !d_image || !d_shown || !d_guide || !frame_ok(width, height)) return hipErrorInvalidValue;
  const bool clamp = st.clamp_sigma > 0.0f && d_carried != nullptr;
  if (clamp && d_cur == d_image) return hipErrorInvalidValue;  // the neighbourhoods would be read while they are written
  const dim3 grid = history_grid(width, height), block(kHistoryBlock);
  const float N = (float) uniform_samples;
  if (!clamp) hipLaunchKernelGGL(k_history_blend<false>, grid, block, 0, stream, st, width, height, N, d_cur, d_carried, d_guides, d_image, d_shown, d_guide);
  else hipLaunchKernelGGL(k_history_blend<true>, grid, block, 0, stream, st, width, height, N, d_cur, d_carried, d_guides, d_image, d_shown, d_guide);
  return hipGetLastError();
}

hipError_t history_owner_launch(const uint4* d_hit_id, const uint32_t* d_paths, uint32_t width, uint32_t n, uint32_t* d_owner, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  if (!d_hit_id || !d_paths || !d_owner || width == 0) return hipErrorInvalidValue;
  const uint32_t blocks = (n + kHistoryBlock - 1u) / kHistoryBlock;
  hipLaunchKernelGGL(k_history_owner, dim3(blocks > 2048u ? 2048u : blocks), dim3(kHistoryBlock), 0, stream, d_hit_id, d_paths, width, n, d_owner);
  return hipGetLastError();
}

hipError_t history_motion_launch(const float4* d_old, const float4* d_new, uint32_t count, HistoryMotion* d_records, uint32_t* d_counts, hipStream_t stream) {
  if (count == 0) return hipSuccess;
  if (!d_old || !d_new || !d_records || !d_counts) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_history_motion, dim3((count + kHistoryBlock - 1u) / kHistoryBlock), dim3(kHistoryBlock), 0, stream, d_old, d_new, count, d_records, d_counts);
  return hipGetLastError();
}

hipError_t history_reproject_motion_launch(const HistoryKey& now, const HistoryKey& old, const HistorySettings& st, float motion_max_history, const float* d_guides,
                                           const HistoryRec* d_shown, const HistoryRec* d_guide, const uint32_t* d_owner, const uint32_t* d_old_owner, const HistoryMotion* d_records,
                                           uint32_t count, HistoryRec* d_carried, uint32_t* d_stats, hipStream_t stream) {
  if (!d_guides || !d_shown || !d_guide || !d_owner || !d_old_owner || (count && !d_records) || !d_carried || !d_stats || !frame_ok(now.width, now.height) || !frame_ok(old.width, old.height))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_history_reproject_motion, history_grid(now.width, now.height), dim3(kHistoryBlock), 0, stream, now, old, st, motion_max_history, d_guides, d_shown, d_guide, d_owner,
                     d_old_owner, d_records, count, d_carried, d_stats);
  return hipGetLastError();
}

}  // namespace lum

// ---- the core's entry points (lum_core.h) ----
namespace {

static_assert(sizeof(LumHistoryKey) == sizeof(HistoryKey) && sizeof(LumHistoryParams) == sizeof(HistorySettings), "lum_core.h mirrors history.h field for field");
static_assert(sizeof(HistoryRec) == 16, "one 16-byte record");
static_assert(sizeof(LumHistoryMotionRecord) == sizeof(HistoryMotion) && sizeof(HistoryMotion) == 128 && sizeof(LumHistoryMotionParams) == 8, "lum_core.h mirrors history.h field for field");

HistoryKey current_key(const LumContext* ctx) {
  const DeviceScene& sc = ctx->scene;
  HistoryKey k{};
  for (int i = 0; i < 3; i++) k.pos[i] = sc.cam_pos[i];
  for (int i = 0; i < 4; i++) k.rot[i] = sc.cam_rotation[i];
  k.fov = sc.cam_fov; k.width = sc.width; k.height = sc.height;
  return k;
}
bool same_key(const HistoryKey& a, const HistoryKey& b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

const char* params_refusal(const LumHistoryParams& p) {
  if (!(p.max_history > 0.0f) || !std::isfinite(p.max_history)) return "max_history must be positive and finite";
  if (!(p.depth_tolerance >= 0.0f) || !std::isfinite(p.depth_tolerance)) return "depth_tolerance must be >= 0 and finite";
  if (!(p.normal_threshold >= -1.0f && p.normal_threshold <= 1.0f)) return "normal_threshold must lie in [-1, 1]";
  if (!(p.clamp_sigma >= 0.0f) || !std::isfinite(p.clamp_sigma)) return "clamp_sigma must be >= 0 and finite";
  return nullptr;
}

// A stamp pair of the history's own around a launch group, under the context's profiling switch (what: 0 carry, 1 blend).
struct HistoryLaunch {
  History& h;
  hipStream_t stream;
  size_t idx = (size_t) -1;
  HistoryLaunch(LumContext* ctx, hipStream_t s, int what) : h(ctx->history), stream(s) {
    if (!ctx->profiling) return;
    History::Stamp st;
    st.what = what;
    if (hipEventCreate(&st.a) != hipSuccess) return;
    if (hipEventCreate(&st.b) != hipSuccess) { (void) hipEventDestroy(st.a); return; }
    (void) hipEventRecord(st.a, stream);
    h.stamps.push_back(st);
    idx = h.stamps.size() - 1;
  }
  ~HistoryLaunch() { if (idx != (size_t) -1) (void) hipEventRecord(h.stamps[idx].b, stream); }
};
void resolve_history_stamps(History& h) {
  for (History::Stamp& st : h.stamps) {
    float ms = 0.0f;
    if (hipEventSynchronize(st.b) == hipSuccess && hipEventElapsedTime(&ms, st.a, st.b) == hipSuccess) { h.ms[st.what] += ms; h.launches[st.what]++; }
    (void) hipEventDestroy(st.a); (void) hipEventDestroy(st.b);
  }
  h.stamps.clear();
}

// planar [channels][n] <-> records
void to_records(const float* rgb, const float* w, size_t n, std::vector<HistoryRec>& out) {
  out.resize(n);
  for (size_t p = 0; p < n; p++) out[p] = HistoryRec{rgb[p], rgb[n + p], rgb[2 * n + p], w[p]};
}
void from_records(const std::vector<HistoryRec>& in, float* rgb, float* w) {
  const size_t n = in.size();
  for (size_t p = 0; p < n; p++) {
    if (rgb) { rgb[p] = in[p].x; rgb[n + p] = in[p].y; rgb[2 * n + p] = in[p].z; }
    if (w) w[p] = in[p].w;
  }
}

}  // namespace

extern "C" {

int lumc_set_history(LumContext* ctx, const LumHistoryParams* params) {
  if (!ctx || !params) { if (ctx) ctx->error = "lumc_set_history: null argument"; return 1; }
  if (params->enabled > 1u) { ctx->error = "lumc_set_history: enabled is 0 or 1"; return 1; }
  if (const char* why = params_refusal(*params)) { ctx->error = std::string("lumc_set_history: ") + why; return 1; }
  History& h = ctx->history;
  std::memcpy(&h.settings, params, sizeof(h.settings));
  if (!params->enabled && (h.has_state || h.has_carried)) return lumc_history_drop(ctx, "history was switched off");
  return 0;
}

int lumc_history_drop(LumContext* ctx, const char* why) {
  if (!ctx) return 1;
  History& h = ctx->history;
  if (h.has_state || h.has_carried) { h.drops++; h.dropped_why = why ? why : "dropped"; }
  h.has_state = false; h.has_carried = false; h.motion.has_snapshot = false; h.motion.state_current = false;
  return 0;
}

int lumc_has_history(const LumContext* ctx) { return (ctx && ctx->history.has_state) ? 1 : 0; }

int lumc_history_release(LumContext* ctx) {
  if (!ctx) return 1;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipDeviceSynchronize());
  History& h = ctx->history;
  resolve_history_stamps(h);
  h.shown.reset(); h.guide.reset(); h.carried.reset(); h.cur.reset(); h.d_stats.reset();
  History::Motion& m = h.motion;
  m.owner_state.reset(); m.owner_cur.reset(); m.snapshot.reset(); m.records.reset(); m.d_counts.reset();
  m.snapshot_instances = 0u; m.record_instances = 0u; m.has_snapshot = false; m.owner_cur_valid = false; m.state_current = false;
  h.has_state = false; h.has_carried = false;
  return 0;
}

int lumc_history_carry(LumContext* ctx, void* stream_) {
  if (!ctx) return 1;
  History& h = ctx->history;
  if (!h.settings.enabled) { ctx->error = "lumc_history_carry: history is off (lumc_set_history)"; return 1; }
  if (!ctx->has_scene) { ctx->error = "lumc_history_carry: no scene"; return 1; }
  if (!h.has_state) { ctx->error = h.dropped_why ? std::string("lumc_history_carry: no state: ") + h.dropped_why : std::string("lumc_history_carry: no state (lumc_history_blend)"); return 1; }
  if (ctx->camera != kCamThinLens) { ctx->error = "lumc_history_carry: the physical camera is not reprojected"; return 1; }
  const HistoryKey now = current_key(ctx);
  const size_t n = (size_t) now.width * now.height;
  if (now.width != h.key.width || now.height != h.key.height || h.pixels() != n) { ctx->error = "lumc_history_carry: the frame size differs from the state's"; return 1; }
  if (!ctx->guides_valid || ctx->d_guides.count() != kGuideSumPlanes * n) { ctx->error = "lumc_history_carry: no guides for this frame (lumc_render_guides)"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t stream = (hipStream_t) stream_;
  if (h.carried.count() != n) HIP_TRY(ctx, h.carried.resize(n));
  if (!h.d_stats) HIP_TRY(ctx, h.d_stats.resize(kHistoryStatWords));
  h.has_carried = false;
  History::Motion& m = h.motion;
  const bool motion = m.enabled && m.has_snapshot;  // (a state shown without an owner plane holds no snapshot: the camera form, as ever)
  if (motion) {
    const uint32_t count = ctx->scene.num_instances;
    if (count != m.snapshot_instances) { ctx->error = "lumc_history_carry: the instance count differs from the snapshot's"; return 1; }
    if (!m.owner_cur_valid || m.owner_cur.count() != n || m.owner_state.count() != n) { ctx->error = "lumc_history_carry: no owner plane for this frame (lumc_render_first_hits with LUMC_FIRST_HIT_OWNER)"; return 1; }
    if (count && !ctx->scene.instance_transforms) { ctx->error = "lumc_history_carry: the scene holds no instance transforms"; return 1; }
    if (m.records.count() != count) HIP_TRY(ctx, m.records.resize(count));
    if (!m.d_counts) HIP_TRY(ctx, m.d_counts.resize(kHistoryStatStride));
    HIP_TRY(ctx, hipMemsetAsync(m.d_counts.get(), 0, sizeof(uint32_t) * kHistoryStatStride, stream));
    HIP_TRY(ctx, hipMemsetAsync(h.d_stats.get(), 0, sizeof(uint32_t) * kHistoryStatWords, stream));
    {
      HistoryLaunch l(ctx, stream, 3);
      HIP_TRY(ctx, history_motion_launch(m.snapshot.get(), ctx->scene.instance_transforms, count, m.records.get(), m.d_counts.get(), stream));
    }
    {
      HistoryLaunch l(ctx, stream, 4);
      HIP_TRY(ctx, history_reproject_motion_launch(now, h.key, h.settings, m.max_history, ctx->d_guides.get(), h.shown.get(), h.guide.get(), m.owner_cur.get(), m.owner_state.get(),
                                                   m.records.get(), count, h.carried.get(), h.d_stats.get(), stream));
    }
    m.record_instances = count; m.carries++;
  }
  else {
    HIP_TRY(ctx, hipMemsetAsync(h.d_stats.get(), 0, sizeof(uint32_t) * kHistoryStatWords, stream));
    HistoryLaunch l(ctx, stream, 0);
    HIP_TRY(ctx, history_reproject_launch(now, h.key, h.settings, ctx->d_guides.get(), h.shown.get(), h.guide.get(), h.carried.get(), h.d_stats.get(), stream));
  }
  m.last_carry = motion;
  h.has_carried = true; h.carried_key = now; h.carries++;
  return 0;
}

int lumc_history_blend(LumContext* ctx, uint32_t uniform_samples, float* d_image, void* stream_) {
  if (!ctx) return 1;
  History& h = ctx->history;
  if (!h.settings.enabled) { ctx->error = "lumc_history_blend: history is off (lumc_set_history)"; return 1; }
  if (!ctx->has_scene) { ctx->error = "lumc_history_blend: no scene"; return 1; }
  if (uniform_samples == 0) { ctx->error = "lumc_history_blend: no samples"; return 1; }
  const HistoryKey now = current_key(ctx);
  const size_t n = (size_t) now.width * now.height;
  if (n == 0 || now.width > 0xFFFFu || now.height > 0xFFFFu) { ctx->error = "lumc_history_blend: frame size"; return 1; }
  if (!ctx->guides_valid || ctx->d_guides.count() != kGuideSumPlanes * n) { ctx->error = "lumc_history_blend: no guides for this frame (lumc_render_guides)"; return 1; }
  if (!d_image) {
    if (ctx->d_frame_result.count() != 3 * n) { ctx->error = "lumc_history_blend: no result image (lumc_generate_result)"; return 1; }
    d_image = ctx->d_frame_result.get();
  }
  if (h.has_carried && (!same_key(h.carried_key, now) || h.carried.count() != n)) { ctx->error = "lumc_history_blend: the camera changed since lumc_history_carry"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t stream = (hipStream_t) stream_;
  if (h.pixels() != n || h.guide.count() != n) {  // (a state of another frame size cannot be carried: it goes)
    if (h.has_state) (void) lumc_history_drop(ctx, "the frame size changed");
    h.shown.reset(); h.guide.reset(); h.motion.has_snapshot = false; h.motion.state_current = false;
    HIP_TRY(ctx, h.shown.resize(n));
    HIP_TRY(ctx, h.guide.resize(n));
  }
  const HistoryRec* carried = h.has_carried ? h.carried.get() : nullptr;
  const bool clamp = carried && h.settings.clamp_sigma > 0.0f;
  if (clamp && h.cur.count() != 3 * n) HIP_TRY(ctx, h.cur.resize(3 * n));
  {
    HistoryLaunch l(ctx, stream, 1);  // (the clamp's copy of the image is part of the blend's time)
    if (clamp) HIP_TRY(ctx, hipMemcpyAsync(h.cur.get(), d_image, sizeof(float) * 3 * n, hipMemcpyDeviceToDevice, stream));
    HIP_TRY(ctx, history_blend_launch(h.settings, now.width, now.height, uniform_samples, clamp ? h.cur.get() : d_image, carried, ctx->d_guides.get(), d_image, h.shown.get(), h.guide.get(), stream));
  }
  // motion: the state takes the owner plane and the instance transforms it was shown with. (A copy, not a swap of the two planes: every output of an accumulation
  // blends, and the second one finds the current plane where the first left it. The copy is made once per guide render: a scene update or a new guide render
  // clears owner_cur_valid or state_current, and until then neither the plane nor the transforms can have changed.)
  History::Motion& m = h.motion;
  const bool owned = m.enabled && m.owner_cur_valid && m.owner_cur.count() == n;
  const bool copied = owned && m.state_current && m.has_snapshot && m.owner_state.count() == n && m.snapshot_instances == ctx->scene.num_instances;
  if (owned && !copied) {
    const uint32_t count = ctx->scene.num_instances;
    if (m.owner_state.count() != n) HIP_TRY(ctx, m.owner_state.resize(n));
    if (m.snapshot.count() != 2 * (size_t) count) HIP_TRY(ctx, m.snapshot.resize(2 * (size_t) count));
    HIP_TRY(ctx, hipMemcpyAsync(m.owner_state.get(), m.owner_cur.get(), sizeof(uint32_t) * n, hipMemcpyDeviceToDevice, stream));
    if (count) HIP_TRY(ctx, hipMemcpyAsync(m.snapshot.get(), ctx->scene.instance_transforms, sizeof(float4) * 2 * (size_t) count, hipMemcpyDeviceToDevice, stream));
    m.snapshot_instances = count; m.has_snapshot = true; m.state_current = true;
  }
  else if (!owned) { m.has_snapshot = false; m.state_current = false; }
  h.key = now; h.has_state = true; h.blends++;
  return 0;
}

int lumc_history_stats(LumContext* ctx, LumHistoryStats* out) {
  if (!ctx || !out) return 1;
  History& h = ctx->history;
  std::memset(out, 0, sizeof(*out));
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipDeviceSynchronize());
  resolve_history_stamps(h);
  out->carries = h.carries; out->blends = h.blends; out->drops = h.drops;
  out->bytes = sizeof(HistoryRec) * (uint64_t) (h.shown.count() + h.guide.count() + h.carried.count()) + sizeof(float) * (uint64_t) h.cur.count();  // (the motion's: lumc_history_motion_stats)
  out->has_state = h.has_state ? 1u : 0u; out->has_carried = h.has_carried ? 1u : 0u;
  out->carry_ms = h.ms[0]; out->blend_ms = h.ms[1]; out->carry_launches = h.launches[0]; out->blend_launches = h.launches[1];
  out->dropped_why = h.dropped_why;
  if (h.d_stats && h.carries) {
    uint32_t st[kHistoryStatWords];
    HIP_TRY(ctx, hipMemcpy(st, h.d_stats.get(), sizeof(st), hipMemcpyDeviceToHost));
    for (uint32_t k = 0; k < kHistoryStatStripes; k++) { out->last_carried += st[k * kHistoryStatStride]; out->last_rejected += st[k * kHistoryStatStride + 1u]; out->last_off += st[k * kHistoryStatStride + 2u]; }
  }
  return 0;
}

int lumc_history_key(LumContext* ctx, LumHistoryKey* state_key, LumHistoryKey* current) {
  if (!ctx) return 1;
  if (state_key) { std::memset(state_key, 0, sizeof(*state_key)); if (ctx->history.has_state) std::memcpy(state_key, &ctx->history.key, sizeof(*state_key)); }
  if (current) {
    std::memset(current, 0, sizeof(*current));
    if (!ctx->has_scene) { ctx->error = "lumc_history_key: no scene"; return 1; }
    const HistoryKey k = current_key(ctx);
    std::memcpy(current, &k, sizeof(*current));
  }
  return 0;
}

int lumc_download_history(LumContext* ctx, float* shown, float* weight, float* carried, float* carried_weight) {
  if (!ctx) return 1;
  History& h = ctx->history;
  if (!h.has_state) { ctx->error = h.dropped_why ? std::string("lumc_download_history: no state: ") + h.dropped_why : std::string("lumc_download_history: no state (lumc_history_blend)"); return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipDeviceSynchronize());
  const size_t n = h.pixels();
  std::vector<HistoryRec> rec(n);
  if (shown || weight) {
    HIP_TRY(ctx, hipMemcpy(rec.data(), h.shown.get(), sizeof(HistoryRec) * n, hipMemcpyDeviceToHost));
    from_records(rec, shown, weight);
  }
  if (carried || carried_weight) {
    if (h.has_carried && h.carried.count() == n) HIP_TRY(ctx, hipMemcpy(rec.data(), h.carried.get(), sizeof(HistoryRec) * n, hipMemcpyDeviceToHost));
    else std::fill(rec.begin(), rec.end(), HistoryRec{0.0f, 0.0f, 0.0f, 0.0f});
    from_records(rec, carried, carried_weight);
  }
  return 0;
}

int lumc_history_kernels_host(LumContext* ctx, const LumHistoryKey* now_key, const LumHistoryKey* old_key, const LumHistoryParams* params, uint32_t uniform_samples,
                              const float* normal, const float* depth, const float* old_shown, const float* old_weight, const float* old_normal, const float* old_depth,
                              float* image_inout, float* carried, float* carried_weight, uint32_t stats[3], float* out_shown, float* out_weight, float* out_normal,
                              float* out_depth) {
  if (!ctx) return 1;
  if (!now_key || !old_key || !params || !normal || !depth || !old_shown || !old_weight || !old_normal || !old_depth || !image_inout) { ctx->error = "lumc_history_kernels_host: null argument"; return 1; }
  if (const char* why = params_refusal(*params)) { ctx->error = std::string("lumc_history_kernels_host: ") + why; return 1; }
  HistoryKey now, old;
  HistorySettings st;
  std::memcpy(&now, now_key, sizeof(now)); std::memcpy(&old, old_key, sizeof(old)); std::memcpy(&st, params, sizeof(st));
  if (!frame_ok(now.width, now.height) || !frame_ok(old.width, old.height)) { ctx->error = "lumc_history_kernels_host: frame size"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const size_t n = (size_t) now.width * now.height, q = (size_t) old.width * old.height;
  std::vector<float> planes(kGuideSumPlanes * n, 0.0f);  // the context's guide planes: [albedo 3 | normal 3 | depth | ...]
  std::memcpy(planes.data() + 3 * n, normal, sizeof(float) * 3 * n);
  std::memcpy(planes.data() + 6 * n, depth, sizeof(float) * n);
  std::vector<HistoryRec> rec;
  DeviceBuffer<float> d_guides, d_image, d_cur;
  DeviceBuffer<HistoryRec> d_old_shown, d_old_guide, d_carried, d_shown, d_guide;
  DeviceBuffer<uint32_t> d_stats;
  HIP_TRY(ctx, d_guides.assign(planes.data(), planes.size()));
  to_records(old_shown, old_weight, q, rec);
  HIP_TRY(ctx, d_old_shown.assign(rec.data(), q));
  to_records(old_normal, old_depth, q, rec);
  HIP_TRY(ctx, d_old_guide.assign(rec.data(), q));
  HIP_TRY(ctx, d_image.assign(image_inout, 3 * n));
  HIP_TRY(ctx, d_cur.assign(image_inout, 3 * n));
  HIP_TRY(ctx, d_carried.resize(n));
  HIP_TRY(ctx, d_shown.resize(n));
  HIP_TRY(ctx, d_guide.resize(n));
  HIP_TRY(ctx, d_stats.resize(kHistoryStatWords));
  HIP_TRY(ctx, hipMemset(d_stats.get(), 0, sizeof(uint32_t) * kHistoryStatWords));
  HIP_TRY(ctx, history_reproject_launch(now, old, st, d_guides.get(), d_old_shown.get(), d_old_guide.get(), d_carried.get(), d_stats.get(), nullptr));
  HIP_TRY(ctx, history_blend_launch(st, now.width, now.height, uniform_samples, d_cur.get(), d_carried.get(), d_guides.get(), d_image.get(), d_shown.get(), d_guide.get(), nullptr));
  HIP_TRY(ctx, hipDeviceSynchronize());
  HIP_TRY(ctx, hipMemcpy(image_inout, d_image.get(), sizeof(float) * 3 * n, hipMemcpyDeviceToHost));
  if (stats) {
    uint32_t st[kHistoryStatWords];
    HIP_TRY(ctx, hipMemcpy(st, d_stats.get(), sizeof(st), hipMemcpyDeviceToHost));
    stats[0] = stats[1] = stats[2] = 0u;
    for (uint32_t k = 0; k < kHistoryStatStripes; k++) for (uint32_t c = 0; c < 3u; c++) stats[c] += st[k * kHistoryStatStride + c];
  }
  rec.resize(n);
  HIP_TRY(ctx, hipMemcpy(rec.data(), d_carried.get(), sizeof(HistoryRec) * n, hipMemcpyDeviceToHost));
  from_records(rec, carried, carried_weight);
  HIP_TRY(ctx, hipMemcpy(rec.data(), d_shown.get(), sizeof(HistoryRec) * n, hipMemcpyDeviceToHost));
  from_records(rec, out_shown, out_weight);
  HIP_TRY(ctx, hipMemcpy(rec.data(), d_guide.get(), sizeof(HistoryRec) * n, hipMemcpyDeviceToHost));
  from_records(rec, out_normal, out_depth);
  return 0;
}

// ---- motion (lum_core.h "Image history, motion") ----
int lumc_set_history_motion(LumContext* ctx, const LumHistoryMotionParams* params) {
  if (!ctx || !params) { if (ctx) ctx->error = "lumc_set_history_motion: null argument"; return 1; }
  if (params->enabled > 1u) { ctx->error = "lumc_set_history_motion: enabled is 0 or 1"; return 1; }
  if (!(params->motion_max_history > 0.0f) || !std::isfinite(params->motion_max_history)) { ctx->error = "lumc_set_history_motion: motion_max_history must be positive and finite"; return 1; }
  ctx->history.motion.enabled = params->enabled;
  ctx->history.motion.max_history = params->motion_max_history;
  return 0;
}

int lumc_has_history_owner(const LumContext* ctx) { return (ctx && ctx->guides_valid && ctx->history.motion.owner_cur_valid) ? 1 : 0; }
int lumc_has_history_snapshot(const LumContext* ctx) { return (ctx && ctx->history.has_state && ctx->history.motion.has_snapshot) ? 1 : 0; }

int lumc_history_motion_stats(LumContext* ctx, LumHistoryMotionStats* out) {
  if (!ctx || !out) return 1;
  History& h = ctx->history;
  History::Motion& m = h.motion;
  std::memset(out, 0, sizeof(*out));
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipDeviceSynchronize());
  resolve_history_stamps(h);
  out->motion_carries = m.carries;
  out->bytes = sizeof(uint32_t) * (uint64_t) (m.owner_state.count() + m.owner_cur.count() + m.d_counts.count()) + sizeof(float4) * (uint64_t) m.snapshot.count() +
               sizeof(HistoryMotion) * (uint64_t) m.records.count();
  out->has_snapshot = (h.has_state && m.has_snapshot) ? 1u : 0u; out->has_owner = m.owner_cur_valid ? 1u : 0u; out->snapshot_instances = m.has_snapshot ? m.snapshot_instances : 0u;
  out->owner_ms = h.ms[2]; out->motion_ms = h.ms[3]; out->reproject_ms = h.ms[4];
  out->owner_launches = h.launches[2]; out->motion_launches = h.launches[3]; out->reproject_launches = h.launches[4];
  if (m.last_carry && h.d_stats && m.d_counts) {
    uint32_t st[kHistoryStatWords], counts[3];
    HIP_TRY(ctx, hipMemcpy(st, h.d_stats.get(), sizeof(st), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(counts, m.d_counts.get(), sizeof(counts), hipMemcpyDeviceToHost));
    out->instances_moved = counts[0]; out->instances_same = counts[1]; out->instances_void = counts[2];
    for (uint32_t k = 0; k < kHistoryStatStripes; k++) { out->last_moved_pixels += st[k * kHistoryStatStride + kHistoryStatMoved]; out->last_moved_carried += st[k * kHistoryStatStride + kHistoryStatMovedCarried]; }
  }
  return 0;
}

int lumc_download_history_owner(LumContext* ctx, uint32_t* state_owner, uint32_t* current_owner) {
  if (!ctx) return 1;
  History& h = ctx->history;
  History::Motion& m = h.motion;
  if (state_owner && !(h.has_state && m.has_snapshot)) { ctx->error = "lumc_download_history_owner: the state holds no owner plane"; return 1; }
  if (current_owner && !m.owner_cur_valid) { ctx->error = "lumc_download_history_owner: no owner plane for this frame (lumc_render_first_hits with LUMC_FIRST_HIT_OWNER)"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipDeviceSynchronize());
  if (state_owner) HIP_TRY(ctx, hipMemcpy(state_owner, m.owner_state.get(), sizeof(uint32_t) * m.owner_state.count(), hipMemcpyDeviceToHost));
  if (current_owner) HIP_TRY(ctx, hipMemcpy(current_owner, m.owner_cur.get(), sizeof(uint32_t) * m.owner_cur.count(), hipMemcpyDeviceToHost));
  return 0;
}

int lumc_download_history_transforms(LumContext* ctx, float* snapshot, float* current, uint32_t* count) {
  if (!ctx) return 1;
  History& h = ctx->history;
  History::Motion& m = h.motion;
  const bool held = h.has_state && m.has_snapshot;
  if (count) *count = held ? m.snapshot_instances : 0u;
  if (snapshot && !held) { ctx->error = "lumc_download_history_transforms: the state holds no snapshot"; return 1; }
  if (current && !ctx->has_scene) { ctx->error = "lumc_download_history_transforms: no scene"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipDeviceSynchronize());
  if (snapshot && m.snapshot_instances) HIP_TRY(ctx, hipMemcpy(snapshot, m.snapshot.get(), sizeof(float) * 8 * (size_t) m.snapshot_instances, hipMemcpyDeviceToHost));
  if (current && ctx->scene.num_instances) HIP_TRY(ctx, hipMemcpy(current, ctx->scene.instance_transforms, sizeof(float) * 8 * (size_t) ctx->scene.num_instances, hipMemcpyDeviceToHost));
  return 0;
}

int lumc_history_motion_kernels_host(LumContext* ctx, const LumHistoryKey* now_key, const LumHistoryKey* old_key, const LumHistoryParams* params, float motion_max_history,
                                     const float* normal, const float* depth, const float* old_shown, const float* old_weight, const float* old_normal, const float* old_depth,
                                     const uint32_t* hit_ids, uint32_t paths, const uint32_t* owner, const uint32_t* old_owner, const float* old8, const float* new8, uint32_t count,
                                     uint32_t* out_owner, LumHistoryMotionRecord* out_records, uint32_t motion_stats[3], float* carried, float* carried_weight, uint32_t stats[5]) {
  if (!ctx) return 1;
  if (!now_key || !old_key || !params || !normal || !depth || !old_shown || !old_weight || !old_normal || !old_depth || (!hit_ids && !owner) || !old_owner || (count && (!old8 || !new8))) {
    ctx->error = "lumc_history_motion_kernels_host: null argument"; return 1;
  }
  if (const char* why = params_refusal(*params)) { ctx->error = std::string("lumc_history_motion_kernels_host: ") + why; return 1; }
  if (!(motion_max_history > 0.0f) || !std::isfinite(motion_max_history)) { ctx->error = "lumc_history_motion_kernels_host: motion_max_history must be positive and finite"; return 1; }
  HistoryKey now, old;
  HistorySettings st;
  std::memcpy(&now, now_key, sizeof(now)); std::memcpy(&old, old_key, sizeof(old)); std::memcpy(&st, params, sizeof(st));
  if (!frame_ok(now.width, now.height) || !frame_ok(old.width, old.height)) { ctx->error = "lumc_history_motion_kernels_host: frame size"; return 1; }
  const size_t n = (size_t) now.width * now.height, q = (size_t) old.width * old.height;
  if (hit_ids && paths > n) { ctx->error = "lumc_history_motion_kernels_host: more paths than pixels"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  std::vector<float> planes(kGuideSumPlanes * n, 0.0f);
  std::memcpy(planes.data() + 3 * n, normal, sizeof(float) * 3 * n);
  std::memcpy(planes.data() + 6 * n, depth, sizeof(float) * n);
  std::vector<HistoryRec> rec;
  DeviceBuffer<float> d_guides;
  DeviceBuffer<HistoryRec> d_old_shown, d_old_guide, d_carried;
  DeviceBuffer<uint32_t> d_stats, d_counts, d_owner, d_old_owner, d_paths;
  DeviceBuffer<uint4> d_hits;
  DeviceBuffer<float4> d_old8, d_new8;
  DeviceBuffer<HistoryMotion> d_records;
  HIP_TRY(ctx, d_guides.assign(planes.data(), planes.size()));
  to_records(old_shown, old_weight, q, rec);
  HIP_TRY(ctx, d_old_shown.assign(rec.data(), q));
  to_records(old_normal, old_depth, q, rec);
  HIP_TRY(ctx, d_old_guide.assign(rec.data(), q));
  HIP_TRY(ctx, d_old_owner.assign(old_owner, q));
  HIP_TRY(ctx, d_carried.resize(n));
  HIP_TRY(ctx, d_stats.resize(kHistoryStatWords));
  HIP_TRY(ctx, d_counts.resize(kHistoryStatStride));
  HIP_TRY(ctx, hipMemset(d_stats.get(), 0, sizeof(uint32_t) * kHistoryStatWords));
  HIP_TRY(ctx, hipMemset(d_counts.get(), 0, sizeof(uint32_t) * kHistoryStatStride));
  if (hit_ids) {
    HIP_TRY(ctx, d_owner.resize(n));
    HIP_TRY(ctx, hipMemset(d_owner.get(), 0xFF, sizeof(uint32_t) * n));
    HIP_TRY(ctx, d_paths.assign(&paths, 1));
    if (paths) {
      HIP_TRY(ctx, d_hits.assign(reinterpret_cast<const uint4*>(hit_ids), paths));
      HIP_TRY(ctx, history_owner_launch(d_hits.get(), d_paths.get(), now.width, (uint32_t) n, d_owner.get(), nullptr));
    }
  }
  else HIP_TRY(ctx, d_owner.assign(owner, n));
  if (count) {
    HIP_TRY(ctx, d_old8.assign(reinterpret_cast<const float4*>(old8), 2 * (size_t) count));
    HIP_TRY(ctx, d_new8.assign(reinterpret_cast<const float4*>(new8), 2 * (size_t) count));
    HIP_TRY(ctx, d_records.resize(count));
    HIP_TRY(ctx, history_motion_launch(d_old8.get(), d_new8.get(), count, d_records.get(), d_counts.get(), nullptr));
  }
  HIP_TRY(ctx, history_reproject_motion_launch(now, old, st, motion_max_history, d_guides.get(), d_old_shown.get(), d_old_guide.get(), d_owner.get(), d_old_owner.get(), d_records.get(), count,
                                               d_carried.get(), d_stats.get(), nullptr));
  HIP_TRY(ctx, hipDeviceSynchronize());
  if (out_owner) HIP_TRY(ctx, hipMemcpy(out_owner, d_owner.get(), sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
  if (out_records && count) HIP_TRY(ctx, hipMemcpy(out_records, d_records.get(), sizeof(HistoryMotion) * (size_t) count, hipMemcpyDeviceToHost));
  if (motion_stats) HIP_TRY(ctx, hipMemcpy(motion_stats, d_counts.get(), sizeof(uint32_t) * 3, hipMemcpyDeviceToHost));
  if (stats) {
    uint32_t w[kHistoryStatWords];
    HIP_TRY(ctx, hipMemcpy(w, d_stats.get(), sizeof(w), hipMemcpyDeviceToHost));
    for (uint32_t c = 0; c < 5u; c++) stats[c] = 0u;
    for (uint32_t k = 0; k < kHistoryStatStripes; k++) for (uint32_t c = 0; c < 5u; c++) stats[c] += w[k * kHistoryStatStride + c];
  }
  rec.resize(n);
  HIP_TRY(ctx, hipMemcpy(rec.data(), d_carried.get(), sizeof(HistoryRec) * n, hipMemcpyDeviceToHost));
  from_records(rec, carried, carried_weight);
  return 0;
}

}  // extern "C"

// ---- what core.hip's render_first_hits calls for LUMC_FIRST_HIT_OWNER (context.h) ----
int history_owner_begin(LumContext* ctx, const char* fn, uint32_t n, hipStream_t stream) {
  History::Motion& m = ctx->history.motion;
  if (!m.enabled) { ctx->error = std::string(fn) + ": LUMC_FIRST_HIT_OWNER needs the history's motion switched on (lumc_set_history_motion)"; return 1; }
  m.owner_cur_valid = false; m.state_current = false;
  if (m.owner_cur.count() != n) HIP_TRY(ctx, m.owner_cur.resize(n));
  HIP_TRY(ctx, hipMemsetAsync(m.owner_cur.get(), 0xFF, sizeof(uint32_t) * (size_t) n, stream));  // kMatteIdEmpty: a pixel without a path
  return 0;
}
int history_owner_pass(LumContext* ctx, const uint4* d_hit_id, const uint32_t* d_paths, uint32_t width, uint32_t n, hipStream_t stream) {
  HistoryLaunch l(ctx, stream, 2);
  HIP_TRY(ctx, history_owner_launch(d_hit_id, d_paths, width, n, ctx->history.motion.owner_cur.get(), stream));
  return 0;
}
