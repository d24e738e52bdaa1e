// C ABI of the path-tracing core (include/lum_core.h), the part that spans GPUs: frame assembly, the tile gather, RCCL communicators and what the tiled
// render loop of the host API needs beyond them. No flavoured kernel is launched from here (context.h).
#include <algorithm>
#include <cstring>

#include <rccl/rccl.h>

#include "context.h"

extern "C" {

// ---- multi-GPU: the image is dealt to the GPUs in 32x32 tiles, every GPU accumulates its own pixels, and ONE reduce per output assembles
// the four moment planes on the display GPU. Replaces the reference's sample partition with host-staged sums
// (device/device_result_interface.c:107-299, at most four devices). Transport: RCCL over xGMI - one communicator rank per context, created
// either per process (lumc_comm_init_rank, launched as one process per GPU) or for all GPUs of one process (lumc_comm_init_all). ----
namespace {
__global__ __launch_bounds__(256) void k_frame_scatter(const float* __restrict__ fm, const float* __restrict__ sm, const uint32_t* __restrict__ pixels, uint32_t n,
                                                       uint32_t frame_pixels, float* __restrict__ frame) {
  for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < n; p += gridDim.x * 256u) {
    const uint32_t index = pixels ? pixels[p] : p;
    if (index >= frame_pixels) continue;
    frame[index] = fm[p]; frame[frame_pixels + index] = fm[n + p]; frame[2u * frame_pixels + index] = fm[2u * n + p];
    frame[3u * frame_pixels + index] = sm[p];
  }
}
__global__ __launch_bounds__(256) void k_frame_add(const float4* __restrict__ src, float4* __restrict__ dst, uint32_t count4) {  // buffer_add, cuda/kernels.cuh:646-675
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < count4; i += gridDim.x * 256u) {
    const float4 a = src[i]; float4 b = dst[i];
    b.x += a.x; b.y += a.y; b.z += a.z; b.w += a.w;
    dst[i] = b;
  }
}
#define NCCL_TRY(ctx, expr)                                                                          \
  do {                                                                                               \
    const ncclResult_t r__ = (expr);                                                                 \
    if (r__ != ncclSuccess) { (ctx)->error = std::string(#expr) + " failed: " + ncclGetErrorString(r__); return 1; } \
  } while (0)

// this context's pixels scattered into its zeroed [4][frame_pixels] frame buffer
int frame_scatter(LumContext* ctx, uint32_t frame_pixels, hipStream_t stream) {
  if (!ctx->d_first_moment || ctx->num_pixels == 0) { ctx->error = "lumc_frame_assemble: no accumulators (lumc_set_pixels)"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const uint32_t padded = frame_pixels;  // 4 planes of n floats = n float4s: the add kernel walks the whole buffer, planes keep stride n
  if (ctx->exchange.frame_pixels() != padded) HIP_TRY(ctx, ctx->exchange.d_frame.resize(4 * (size_t) padded));
  HIP_TRY(ctx, hipMemsetAsync(ctx->exchange.d_frame.get(), 0, sizeof(float) * 4 * (size_t) ctx->exchange.frame_pixels(), stream));
  hipLaunchKernelGGL(k_frame_scatter, dim3(grid_for(ctx->num_pixels)), dim3(256), 0, stream, (const float*) ctx->d_first_moment.get(), (const float*) ctx->d_second_moment.get(),
                     (const uint32_t*) ctx->d_pixels.get(), ctx->num_pixels, ctx->exchange.frame_pixels(), ctx->exchange.d_frame.get());
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}
}  // namespace

int lumc_device_count(void) {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

int lumc_comm_unique_id(uint8_t id[LUMC_COMM_ID_BYTES]) {
  static_assert(sizeof(ncclUniqueId) <= LUMC_COMM_ID_BYTES, "unique id does not fit");
  if (!id) return 1;
  ncclUniqueId u;
  if (ncclGetUniqueId(&u) != ncclSuccess) return 1;
  std::memset(id, 0, LUMC_COMM_ID_BYTES);
  std::memcpy(id, &u, sizeof(u));
  return 0;
}

int lumc_comm_init_rank(LumContext* ctx, int world, int rank, const uint8_t id[LUMC_COMM_ID_BYTES]) {
  if (!ctx || !id || world < 1 || rank < 0 || rank >= world) { if (ctx) ctx->error = "lumc_comm_init_rank: bad arguments"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (ctx->exchange.comm) { (void) ncclCommDestroy(ctx->exchange.comm); ctx->exchange.comm = nullptr; }
  ncclUniqueId u;
  std::memcpy(&u, id, sizeof(u));
  NCCL_TRY(ctx, ncclCommInitRank(&ctx->exchange.comm, world, u, rank));
  ctx->exchange.comm_rank = rank; ctx->exchange.comm_world = world;
  return 0;
}

int lumc_comm_init_all(LumContext** ctxs, int n) {
  if (!ctxs || n < 1) return 1;
  std::vector<int> devices(n);
  for (int i = 0; i < n; i++) {
    if (!ctxs[i]) return 1;
    devices[i] = ctxs[i]->device;
    for (int j = 0; j < i; j++)
      if (devices[j] == devices[i]) { ctxs[0]->error = "lumc_comm_init_all: two contexts on one device (RCCL needs one GPU per rank)"; return 1; }
  }
  std::vector<ncclComm_t> comms(n, nullptr);
  NCCL_TRY(ctxs[0], ncclCommInitAll(comms.data(), n, devices.data()));
  for (int i = 0; i < n; i++) {
    if (ctxs[i]->exchange.comm) (void) ncclCommDestroy(ctxs[i]->exchange.comm);
    ctxs[i]->exchange.comm = comms[i]; ctxs[i]->exchange.comm_rank = i; ctxs[i]->exchange.comm_world = n;
  }
  return 0;
}

void lumc_comm_destroy(LumContext* ctx) {
  if (ctx && ctx->exchange.comm) { (void) hipSetDevice(ctx->device); (void) ncclCommDestroy(ctx->exchange.comm); ctx->exchange.comm = nullptr; ctx->exchange.comm_world = 1; ctx->exchange.comm_rank = 0; }
}

// One process per GPU: this rank's pixels into its frame buffer, then ncclReduce(SUM) to `root` (every pixel has one owner, so the sum is
// a gather: 16 bytes per pixel and rank, once per output). Without a communicator (single GPU) the scatter alone is the frame.
int lumc_frame_assemble(LumContext* ctx, uint32_t frame_pixels, int root, void* stream_, float** d_frame_out) {
  if (!ctx) return 1;
  hipStream_t stream = (hipStream_t) stream_;
  if (frame_scatter(ctx, frame_pixels, stream)) return 1;
  if (ctx->exchange.comm) {
    if (root < 0 || root >= ctx->exchange.comm_world) { ctx->error = "lumc_frame_assemble: bad root"; return 1; }
    NCCL_TRY(ctx, ncclReduce(ctx->exchange.d_frame.get(), ctx->exchange.d_frame.get(), 4 * (size_t) ctx->exchange.frame_pixels(), ncclFloat, ncclSum, root, ctx->exchange.comm, stream));
  }
  if (d_frame_out) *d_frame_out = ctx->exchange.d_frame.get();
  return 0;
}

// One process, several GPUs: all contexts scatter, then one grouped ncclReduce to `root` (lumc_comm_init_all). Contexts without a common
// communicator (RCCL unavailable, or test set-ups with two contexts on one device) are summed through peer copies and the add kernel
// instead - the reference's own transport (device_result_interface.c:177-215), kept as the fallback.
int lumc_frame_assemble_all(LumContext** ctxs, int n, uint32_t frame_pixels, int root, float** d_frame_root) {
  if (!ctxs || n < 1 || root < 0 || root >= n) return 1;
  bool rccl = n > 1;
  for (int i = 0; i < n; i++) {
    if (!ctxs[i]) return 1;
    if (frame_scatter(ctxs[i], frame_pixels, (hipStream_t) 0)) { if (i) ctxs[0]->error = ctxs[i]->error; return 1; }
    rccl = rccl && ctxs[i]->exchange.comm && ctxs[i]->exchange.comm_world == n && ctxs[i]->exchange.comm_rank == i;
  }
  LumContext* r = ctxs[root];
  if (rccl) {
    NCCL_TRY(r, ncclGroupStart());
    for (int i = 0; i < n; i++) {
      (void) hipSetDevice(ctxs[i]->device);
      const ncclResult_t e = ncclReduce(ctxs[i]->exchange.d_frame.get(), ctxs[i]->exchange.d_frame.get(), 4 * (size_t) ctxs[i]->exchange.frame_pixels(), ncclFloat, ncclSum, root, ctxs[i]->exchange.comm, (hipStream_t) 0);
      if (e != ncclSuccess) { (void) ncclGroupEnd(); r->error = std::string("ncclReduce failed: ") + ncclGetErrorString(e); return 1; }
    }
    NCCL_TRY(r, ncclGroupEnd());
    for (int i = 0; i < n; i++) { HIP_TRY(r, hipSetDevice(ctxs[i]->device)); HIP_TRY(r, hipDeviceSynchronize()); }
  }
  else if (n > 1) {
    HIP_TRY(r, hipSetDevice(r->device));
    const size_t bytes = sizeof(float) * r->exchange.d_frame.count();
    DeviceBuffer<float> staging;
    HIP_TRY(r, staging.resize(r->exchange.d_frame.count()));
    for (int i = 0; i < n; i++) {
      if (i == root) continue;
      HIP_TRY(r, hipSetDevice(ctxs[i]->device));
      HIP_TRY(r, hipDeviceSynchronize());
      HIP_TRY(r, hipSetDevice(r->device));
      HIP_TRY(r, hipMemcpyPeer(staging.get(), r->device, ctxs[i]->exchange.d_frame.get(), ctxs[i]->device, bytes));
      hipLaunchKernelGGL(k_frame_add, dim3(grid_for(r->exchange.frame_pixels())), dim3(256), 0, 0, (const float4*) staging.get(), (float4*) r->exchange.d_frame.get(), r->exchange.frame_pixels());
      HIP_TRY(r, hipGetLastError());
    }
    HIP_TRY(r, hipDeviceSynchronize());
  }
  if (d_frame_root) *d_frame_root = r->exchange.d_frame.get();
  return 0;
}

// ---- tile gather: the frame assembled from the ranks' own pixels instead of a reduce over whole frames ----
// Every pixel has one owner, so summing the ranks' zero-padded full frames (lumc_frame_assemble: 16 bytes per FRAME pixel from every rank, 133 MB per
// rank at 4K) moves `world` times what is needed: a rank's contribution is the 16 bytes of each pixel it OWNS. Where the ranks' pixel sets are the tile
// deal of lumc_tile_pixels (32 x 32 tiles dealt by lumc_tile_owner's lattice - what bench.py and the host API's tiled render loop use), every rank can compute every other
// rank's pixel list, so nothing but the sums travels: each rank packs its [3][P] + [P] accumulators into a [4][M] buffer (M = the largest tile share,
// zero padded: the deal's shares differ by at most tiles_y % world tiles, see lumc_tile_lattice_step), ONE ncclGather brings the `world` buffers to the root, and a scatter kernel on the root puts every
// value at its pixel. Reference: device_result_interface.c:107-299 (sample partition, sums staged through pinned host memory).
namespace {
__global__ __launch_bounds__(256) void k_gather_pack(const float* __restrict__ fm, const float* __restrict__ sm, uint32_t n, uint32_t stride, float* __restrict__ send) {
  for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < stride; p += gridDim.x * 256u) {
    const bool in = p < n;
    send[p] = in ? fm[p] : 0.0f; send[stride + p] = in ? fm[n + p] : 0.0f; send[2u * stride + p] = in ? fm[2u * n + p] : 0.0f; send[3u * stride + p] = in ? sm[p] : 0.0f;
  }
}
__global__ __launch_bounds__(256) void k_gather_unpack(const float* __restrict__ recv, const uint32_t* __restrict__ pixels, uint32_t world, uint32_t stride, uint32_t frame_pixels,
                                                       float* __restrict__ frame) {
  const uint32_t total = world * stride;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < total; i += gridDim.x * 256u) {
    const uint32_t index = pixels[i];
    if (index >= frame_pixels) continue;  // padding
    const uint32_t r = i / stride, p = i - r * stride;
    const float* src = recv + (size_t) r * 4u * stride;
    frame[index] = src[p]; frame[frame_pixels + index] = src[stride + p]; frame[2u * frame_pixels + index] = src[2u * stride + p]; frame[3u * frame_pixels + index] = src[3u * stride + p];
  }
}

constexpr uint32_t kGatherTile = 32u;  // the deal bench.py, luminary_amd/distributed.py and the host API use

// Sizes this context's gather buffers for (width, height, world): the send buffer on every rank, the receive buffer and the pixel lists on the root.
// Fails when this context's pixel count is not its share of the deal (the gather is only for the standard deal; anything else reduces).
int gather_prepare(LumContext* ctx, uint32_t width, uint32_t height, int world, int rank, bool is_root) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  uint32_t share = 0, stride = 0;
  for (int r = 0; r < world; r++) {
    uint32_t c = 0;
    if (lumc_tile_pixels(width, height, (uint32_t) r, (uint32_t) world, kGatherTile, nullptr, &c)) { ctx->error = "lumc_frame_gather: bad deal"; return 1; }
    if (r == rank) share = c;
    stride = std::max(stride, c);
  }
  bool is_share = ctx->d_first_moment && ctx->num_pixels == share;
  if (is_share) {  // ... and the same pixels in the same order: the root scatters the rank's sums through the list IT derives from the deal
    std::vector<uint32_t> mine(share ? share : 1);
    uint32_t c = 0;
    (void) lumc_tile_pixels(width, height, (uint32_t) rank, (uint32_t) world, kGatherTile, mine.data(), &c);
    is_share = pixel_list_hash(mine.data(), share) == ctx->pixels_hash;
  }
  if (!is_share) {
    ctx->error = "lumc_frame_gather: this context's pixel set is not its share of the 32x32 tile deal, in the deal's order (use lumc_frame_assemble for other partitions)";
    return 1;
  }
  stride = (stride + 3u) & ~3u;
  const bool same = ctx->exchange.gather_key[0] == width && ctx->exchange.gather_key[1] == height && ctx->exchange.gather_key[2] == (uint32_t) world && ctx->exchange.gather_stride == stride && ctx->exchange.d_gather_send.get();
  if (!same) {
    ctx->exchange.d_gather_pixels.reset();
    HIP_TRY(ctx, ctx->exchange.d_gather_send.resize(4 * (size_t) stride));
    ctx->exchange.gather_stride = stride; ctx->exchange.gather_key[0] = width; ctx->exchange.gather_key[1] = height; ctx->exchange.gather_key[2] = (uint32_t) world;
  }
  if (is_root) {
    const size_t need = (size_t) world * 4 * stride;
    if (ctx->exchange.d_gather_recv.count() < need) HIP_TRY(ctx, ctx->exchange.d_gather_recv.resize(need));
    if (!ctx->exchange.d_gather_pixels) {
      std::vector<uint32_t> lists((size_t) world * stride, 0xFFFFFFFFu);
      for (int r = 0; r < world; r++) { uint32_t c = 0; (void) lumc_tile_pixels(width, height, (uint32_t) r, (uint32_t) world, kGatherTile, lists.data() + (size_t) r * stride, &c); }
      HIP_TRY(ctx, ctx->exchange.d_gather_pixels.assign(lists.data(), lists.size()));
    }
    const uint32_t frame_pixels = width * height;
    if (ctx->exchange.frame_pixels() != frame_pixels) HIP_TRY(ctx, ctx->exchange.d_frame.resize(4 * (size_t) frame_pixels));
  }
  return 0;
}
int gather_pack(LumContext* ctx, hipStream_t stream) {
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_gather_pack, dim3(grid_for(ctx->exchange.gather_stride)), dim3(256), 0, stream, (const float*) ctx->d_first_moment.get(), (const float*) ctx->d_second_moment.get(), ctx->num_pixels,
                     ctx->exchange.gather_stride, ctx->exchange.d_gather_send.get());
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}
int gather_unpack(LumContext* root, int world, hipStream_t stream) {
  HIP_TRY(root, hipSetDevice(root->device));
  hipLaunchKernelGGL(k_gather_unpack, dim3(grid_for((uint32_t) world * root->exchange.gather_stride)), dim3(256), 0, stream, (const float*) root->exchange.d_gather_recv.get(), (const uint32_t*) root->exchange.d_gather_pixels.get(),
                     (uint32_t) world, root->exchange.gather_stride, root->exchange.frame_pixels(), root->exchange.d_frame.get());
  HIP_TRY(root, hipGetLastError());
  return 0;
}
}  // namespace

// One process per GPU (lumc_comm_init_rank): pack, one ncclGather to `root`, scatter on the root. Without a communicator (one rank) the pack is copied.
int lumc_frame_gather(LumContext* ctx, uint32_t width, uint32_t height, int root, void* stream_, float** d_frame_out) {
  if (!ctx) return 1;
  hipStream_t stream = (hipStream_t) stream_;
  const int world = ctx->exchange.comm ? ctx->exchange.comm_world : 1, rank = ctx->exchange.comm ? ctx->exchange.comm_rank : 0;
  if (root < 0 || root >= world) { ctx->error = "lumc_frame_gather: bad root"; return 1; }
  if (gather_prepare(ctx, width, height, world, rank, rank == root)) return 1;
  if (gather_pack(ctx, stream)) return 1;
  const size_t count = 4 * (size_t) ctx->exchange.gather_stride;
  if (ctx->exchange.comm) NCCL_TRY(ctx, ncclGather(ctx->exchange.d_gather_send.get(), rank == root ? ctx->exchange.d_gather_recv.get() : nullptr, count, ncclFloat, root, ctx->exchange.comm, stream));
  else HIP_TRY(ctx, hipMemcpyAsync(ctx->exchange.d_gather_recv.get(), ctx->exchange.d_gather_send.get(), sizeof(float) * count, hipMemcpyDeviceToDevice, stream));
  if (rank == root && gather_unpack(ctx, world, stream)) return 1;
  if (d_frame_out) *d_frame_out = rank == root ? ctx->exchange.d_frame.get() : nullptr;
  return 0;
}

// One process, several GPUs (ctxs[i] holds share i of the deal over n): a grouped ncclGather when the contexts share a communicator
// (lumc_comm_init_all), peer copies of the packed buffers into the root's receive buffer otherwise.
int lumc_frame_gather_all(LumContext** ctxs, int n, uint32_t width, uint32_t height, int root, float** d_frame_root) {
  if (!ctxs || n < 1 || root < 0 || root >= n) return 1;
  bool rccl = n > 1;
  for (int i = 0; i < n; i++) {
    if (!ctxs[i]) return 1;
    if (gather_prepare(ctxs[i], width, height, n, i, i == root) || gather_pack(ctxs[i], (hipStream_t) 0)) { if (i) ctxs[0]->error = ctxs[i]->error; return 1; }
    rccl = rccl && ctxs[i]->exchange.comm && ctxs[i]->exchange.comm_world == n && ctxs[i]->exchange.comm_rank == i;
  }
  LumContext* r = ctxs[root];
  const size_t count = 4 * (size_t) r->exchange.gather_stride;
  if (rccl) {
    NCCL_TRY(r, ncclGroupStart());
    for (int i = 0; i < n; i++) {
      (void) hipSetDevice(ctxs[i]->device);
      const ncclResult_t e = ncclGather(ctxs[i]->exchange.d_gather_send.get(), i == root ? r->exchange.d_gather_recv.get() : nullptr, count, ncclFloat, root, ctxs[i]->exchange.comm, (hipStream_t) 0);
      if (e != ncclSuccess) { (void) ncclGroupEnd(); r->error = std::string("ncclGather failed: ") + ncclGetErrorString(e); return 1; }
    }
    NCCL_TRY(r, ncclGroupEnd());
    for (int i = 0; i < n; i++) { HIP_TRY(r, hipSetDevice(ctxs[i]->device)); HIP_TRY(r, hipDeviceSynchronize()); }
  }
  else {
    for (int i = 0; i < n; i++) {
      HIP_TRY(r, hipSetDevice(ctxs[i]->device));
      HIP_TRY(r, hipDeviceSynchronize());
      HIP_TRY(r, hipSetDevice(r->device));
      HIP_TRY(r, hipMemcpyPeer(r->exchange.d_gather_recv.get() + (size_t) i * count, r->device, ctxs[i]->exchange.d_gather_send.get(), ctxs[i]->device, sizeof(float) * count));
    }
  }
  if (gather_unpack(r, n, (hipStream_t) 0)) return 1;
  HIP_TRY(r, hipDeviceSynchronize());
  if (d_frame_root) *d_frame_root = r->exchange.d_frame.get();
  return 0;
}

// ---- one process, several GPUs: what the tiled render loop of the host API needs beyond the frame assembly ----
namespace {
// this context's accumulators <- the frame's values at its pixels; with an adaptive partition only inside the blocks it owns
__global__ __launch_bounds__(256) void k_accumulators_from_frame(const float* __restrict__ frame, uint32_t frame_pixels, const uint32_t* __restrict__ pixels, uint32_t n,
                                                                 const uint8_t* __restrict__ block_mask, uint32_t width, uint32_t blocks_x, float* __restrict__ fm, float* __restrict__ sm) {
  for (uint32_t p = blockIdx.x * 256u + threadIdx.x; p < n; p += gridDim.x * 256u) {
    const uint32_t index = pixels ? pixels[p] : p;
    bool mine = index < frame_pixels;
    if (mine && block_mask) { const uint32_t y = index / width, x = index - y * width; mine = block_mask[(y >> 2) * blocks_x + (x >> 2)] != 0; }
    fm[p] = mine ? frame[index] : 0.0f; fm[n + p] = mine ? frame[frame_pixels + index] : 0.0f; fm[2u * n + p] = mine ? frame[2u * frame_pixels + index] : 0.0f;
    sm[p] = mine ? frame[3u * frame_pixels + index] : 0.0f;
  }
}
}  // namespace

// The accumulators of `dst` (whatever its pixel set: a tile list, or the full frame with an adaptive partition) take the values the frame buffer of
// `src` holds at dst's pixels (lumc_frame_assemble on src first: its own full-frame accumulators, scattered). This is how the first sample of a
// frame, rendered coarse to fine on the main device alone (the undersampling preview, device.c:392-420), is handed to the devices that go on with
// the frame's tiles: every pixel's sums continue where the preview left them, so the tiled frame equals the single-device frame bit for bit.
int lumc_accumulators_from_frame(LumContext* dst, LumContext* src) {
  if (!dst || !src || !src->exchange.d_frame || !dst->d_first_moment || dst->num_pixels == 0) { if (dst) dst->error = "lumc_accumulators_from_frame: no frame on the source or no accumulators on the destination"; return 1; }
  const uint32_t frame_pixels = src->exchange.frame_pixels();
  const float* frame = src->exchange.d_frame.get();
  DeviceBuffer<float> staging;
  HIP_TRY(dst, hipSetDevice(src->device));
  HIP_TRY(dst, hipDeviceSynchronize());
  HIP_TRY(dst, hipSetDevice(dst->device));
  if (dst != src) {  // another context (another GPU, or the same one in test set-ups): a copy of the frame on dst's device
    const size_t bytes = sizeof(float) * 4 * (size_t) frame_pixels;
    HIP_TRY(dst, staging.resize(4 * (size_t) frame_pixels));
    HIP_TRY(dst, hipMemcpyPeer(staging.get(), dst->device, src->exchange.d_frame.get(), src->device, bytes));
    frame = staging.get();
  }
  const LumContext::Adaptive& a = dst->adaptive;
  hipLaunchKernelGGL(k_accumulators_from_frame, dim3(grid_for(dst->num_pixels)), dim3(256), 0, 0, frame, frame_pixels, (const uint32_t*) dst->d_pixels.get(), dst->num_pixels,
                     a.active ? (const uint8_t*) a.d_block_mask.get() : nullptr, dst->scene.width, a.active ? a.blocks_x : 0u, dst->d_first_moment.get(), dst->d_second_moment.get());
  HIP_TRY(dst, hipGetLastError());
  HIP_TRY(dst, hipDeviceSynchronize());
  return 0;
}

// A stage build of adaptive rendering tiled over the contexts of one process (lumc_adaptive_set_partition on each): every context computes the
// variances of its blocks, ONE all-reduce of 4 bytes per block makes the array complete everywhere (every block has one owner: the sum is a gather and
// exact), every context derives the same rates. Grouped ncclAllReduce when the contexts share a communicator (lumc_comm_init_all); otherwise - two
// contexts on one device in tests, or no RCCL - the arrays are summed on the host in context order.
int lumc_adaptive_exchange_all(LumContext** ctxs, int n) {
  if (!ctxs || n < 1) return 1;
  bool rccl = n > 1;
  for (int i = 0; i < n; i++) {
    if (!ctxs[i] || !ctxs[i]->adaptive.active) { if (ctxs[0]) ctxs[0]->error = "lumc_adaptive_exchange_all: adaptive mode is not active on every context"; return 1; }
    if (ctxs[i]->adaptive.num_blocks != ctxs[0]->adaptive.num_blocks) { ctxs[0]->error = "lumc_adaptive_exchange_all: contexts of different frames"; return 1; }
    HIP_TRY(ctxs[0], hipSetDevice(ctxs[i]->device));
    if (adaptive_compute_variance(ctxs[i], (hipStream_t) 0)) { ctxs[0]->error = ctxs[i]->error; return 1; }
    rccl = rccl && ctxs[i]->exchange.comm && ctxs[i]->exchange.comm_world == n && ctxs[i]->exchange.comm_rank == i;
  }
  const uint32_t nb = ctxs[0]->adaptive.num_blocks;
  if (rccl) {
    NCCL_TRY(ctxs[0], ncclGroupStart());
    for (int i = 0; i < n; i++) {
      (void) hipSetDevice(ctxs[i]->device);
      const ncclResult_t e = ncclAllReduce(ctxs[i]->adaptive.d_block_variance.get(), ctxs[i]->adaptive.d_block_variance.get(), nb, ncclFloat, ncclSum, ctxs[i]->exchange.comm, (hipStream_t) 0);
      if (e != ncclSuccess) { (void) ncclGroupEnd(); ctxs[0]->error = std::string("ncclAllReduce failed: ") + ncclGetErrorString(e); return 1; }
    }
    NCCL_TRY(ctxs[0], ncclGroupEnd());
  }
  else if (n > 1) {
    std::vector<float> sum(nb, 0.0f), part(nb);
    for (int i = 0; i < n; i++) {
      HIP_TRY(ctxs[0], hipSetDevice(ctxs[i]->device));
      HIP_TRY(ctxs[0], hipMemcpy(part.data(), ctxs[i]->adaptive.d_block_variance.get(), sizeof(float) * nb, hipMemcpyDeviceToHost));
      for (uint32_t b = 0; b < nb; b++) sum[b] += part[b];
    }
    for (int i = 0; i < n; i++) {
      HIP_TRY(ctxs[0], hipSetDevice(ctxs[i]->device));
      HIP_TRY(ctxs[0], hipMemcpy(ctxs[i]->adaptive.d_block_variance.get(), sum.data(), sizeof(float) * nb, hipMemcpyHostToDevice));
    }
  }
  for (int i = 0; i < n; i++) {
    HIP_TRY(ctxs[0], hipSetDevice(ctxs[i]->device));
    if (ctxs[i]->adaptive.stage_id >= kAdaptiveStages) { ctxs[0]->error = "lumc_adaptive_exchange_all: the last stage is already running"; return 1; }
    if (adaptive_finish_build(ctxs[i], (hipStream_t) 0)) { ctxs[0]->error = ctxs[i]->error; return 1; }
  }
  return 0;
}
// Ranks of the communicator this context belongs to (1 without one): what a launcher prints to show that RCCL saw every GPU.
int lumc_comm_count(const LumContext* ctx) {
  if (!ctx || !ctx->exchange.comm) return 1;
  int count = 1;
  return ncclCommCount(ctx->exchange.comm, &count) == ncclSuccess ? count : 1;
}

// The assembled frame of this context (valid on the root after lumc_frame_assemble*): planar first moment [3][frame_pixels] and second moment.
int lumc_frame_download(LumContext* ctx, uint32_t frame_pixels, float* first_moment, float* second_moment) {
  if (!ctx || !ctx->exchange.d_frame || frame_pixels > ctx->exchange.frame_pixels()) { if (ctx) ctx->error = "lumc_frame_download: no assembled frame"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipDeviceSynchronize());
  const size_t cap = ctx->exchange.frame_pixels();
  if (first_moment)
    for (int c = 0; c < 3; c++) HIP_TRY(ctx, hipMemcpy(first_moment + (size_t) c * frame_pixels, ctx->exchange.d_frame.get() + (size_t) c * cap, sizeof(float) * frame_pixels, hipMemcpyDeviceToHost));
  if (second_moment) HIP_TRY(ctx, hipMemcpy(second_moment, ctx->exchange.d_frame.get() + 3 * cap, sizeof(float) * frame_pixels, hipMemcpyDeviceToHost));
  return 0;
}
uint32_t lumc_frame_plane_stride(const LumContext* ctx) { return ctx ? ctx->exchange.frame_pixels() : 0; }
// The display entry points of this context (lumc_generate_result*, and through them the output chain) read the assembled full frame instead
// of the context's own accumulators: what the display GPU of a tiled render shows.
int lumc_use_assembled_frame(LumContext* ctx, int on) {
  if (!ctx) return 1;
  if (on && (!ctx->exchange.d_frame || !ctx->has_scene || ctx->exchange.frame_pixels() != ctx->scene.width * ctx->scene.height)) { ctx->error = "lumc_use_assembled_frame: no assembled frame of this scene's size"; return 1; }
  ctx->exchange.use_frame = on != 0;
  return 0;
}
}  // extern "C"

void free_exchange(LumContext* ctx) {
  LumContext::Exchange& x = ctx->exchange;
  if (x.comm) (void) ncclCommDestroy(x.comm);
  x = LumContext::Exchange();
}
