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

}  // namespace lum

// ---- the core's entry points (lum_core.h) ----
namespace {

static_assert(sizeof(LumHistoryKey) == sizeof(HistoryKey) && sizeof(LumHistoryParams) == sizeof(HistorySettings), "lum_core.h mirrors history.h field for field");
static_assert(sizeof(HistoryRec) == 16, "one 16-byte record");

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
  h.has_state = false; h.has_carried = false;
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
  HIP_TRY(ctx, hipMemsetAsync(h.d_stats.get(), 0, sizeof(uint32_t) * kHistoryStatWords, stream));
  {
    HistoryLaunch l(ctx, stream, 0);
    HIP_TRY(ctx, history_reproject_launch(now, h.key, h.settings, ctx->d_guides.get(), h.shown.get(), h.guide.get(), h.carried.get(), h.d_stats.get(), stream));
  }
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
    h.shown.reset(); h.guide.reset();
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
  out->bytes = sizeof(HistoryRec) * (uint64_t) (h.shown.count() + h.guide.count() + h.carried.count()) + sizeof(float) * (uint64_t) h.cur.count();
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

}  // extern "C"
