// GPU refit of a mesh's 4-wide tree after its vertices moved (luminary_ext_set_mesh_positions -> LUMC_DIRTY_MESH_POSITIONS): the topology stays, every
// child box becomes the builders' pad of the exact union of what lies below it. Host twin, and the checker of this unit: bvh_build.cpp refit_bvh4 - the
// union is min / max (exact, order-free up to the sign of a zero, and the order is the host's), the pad the one expression of set_child_box, compiled
// here without contraction like there: both give the same bytes.
//
//   k_refit_tri_boxes   one thread per triangle in leaf order: its box from the device scene's vertices; rewrites the triangle's traversal geometry
//   k_refit_level       one thread per node of ONE level, deepest level first, one launch per level: the kernel boundary is what makes a level's exact
//                       boxes (a per-node scratch array) visible to the level above - no in-launch hand-off, no counters. At most 26 launches.
// The per-level node lists come from one breadth-first walk on the host (bvh4_levels): the GPU builders number nodes through atomics, levels are no ranges.
//
// The same refit where the nodes live (resident_refit_run): the scene's node array in the resident layout of instance_update.h holds every
// mesh's nodes with absolute child words at slots that are no range, so no node is copied, downloaded or uploaded.
//   k_refit_level_resident  one thread per node slot of ONE depth below the mesh roots, over ALL moved meshes of the update (grid y = the mesh's row in a job
//                           table): one launch per depth, deepest first, at most 27 however many meshes moved. Writes the padded child boxes into the resident
//                           node, its own exact box into a per-slot scratch; child words, pad and empty slots are not touched
//   k_resident_mesh_boxes   one thread per moved mesh: its root's exact box into the moved instances' mesh boxes (instance_update.h) and the results
//   k_bvh4_cost             bvh4_cost of every moved mesh's nodes as they stand in the array: per node the occupied slots' half areas in double, in slot order,
//                           summed per workgroup in a fixed tree; k_bvh4_cost_sum adds a mesh's workgroup sums. No atomics: the same sum every time
// The reference has nothing like it: optixAccelBuild with OPTIX_BUILD_OPERATION_UPDATE would be its counterpart, and it does not use it (optix_bvh.c:150-684).
#include <hip/hip_runtime.h>

#include <cfloat>
#include <chrono>
#include <cstring>
#include <vector>

#include "bvh_refit.h"

namespace lum {
namespace {

constexpr uint32_t kRefitBlock = 256;

// std::min / std::max of bvh_build.cpp's grow, operand for operand (fminf may pick the other zero)
__device__ __forceinline__ float min_of(float a, float b) { return (b < a) ? b : a; }
__device__ __forceinline__ float max_of(float a, float b) { return (a < b) ? b : a; }
__device__ __forceinline__ void grow(Aabb& a, const Aabb& b) {
  for (int k = 0; k < 3; k++) { a.lo[k] = min_of(a.lo[k], b.lo[k]); a.hi[k] = max_of(a.hi[k], b.hi[k]); }
}
__device__ __forceinline__ Aabb empty_box() { return Aabb{{FLT_MAX, FLT_MAX, FLT_MAX}, {-FLT_MAX, -FLT_MAX, -FLT_MAX}}; }

// vertices: the mesh's first vertex (3 float4 per triangle, by triangle id); tris / prim_box: the mesh's first traversal triangle / box, in leaf order.
// id, scene_index and albedo_tex of a traversal triangle stay: the triangle order did not change.
__global__ __launch_bounds__(kRefitBlock) void k_refit_tri_boxes(const float4* __restrict__ vertices, const uint32_t* __restrict__ prims, uint32_t count,
                                                                 BvhTri* __restrict__ tris, Aabb* __restrict__ prim_box) {
  const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
  if (i >= count) return;
  const uint32_t t = prims[i];
  if (t >= count) return;  // (refit_plan_create checked the ids)
  const float4 a4 = vertices[3 * (size_t) t], b4 = vertices[3 * (size_t) t + 1], c4 = vertices[3 * (size_t) t + 2];
  const float a[3] = {a4.x, a4.y, a4.z}, b[3] = {b4.x, b4.y, b4.z}, c[3] = {c4.x, c4.y, c4.z};
  Aabb box;
  for (int k = 0; k < 3; k++) { box.lo[k] = min_of(a[k], min_of(b[k], c[k])); box.hi[k] = max_of(a[k], max_of(b[k], c[k])); }  // tri_box
  prim_box[i] = box;
  BvhTri& tri = tris[i];
  for (int k = 0; k < 3; k++) { tri.p0[k] = a[k]; tri.e1[k] = b[k] - a[k]; tri.e2[k] = c[k] - a[k]; }  // bvh_tri
}

// level: the node ids of one level. Reads node_box of the level below (written by the previous launch), writes node_box of its own nodes.
__global__ __launch_bounds__(kRefitBlock) void k_refit_level(Bvh4Node* __restrict__ nodes, const uint32_t* __restrict__ level, uint32_t n, uint32_t num_nodes,
                                                             uint32_t count, const Aabb* __restrict__ prim_box, Aabb* node_box) {
  const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t id = level[i];
  if (id >= num_nodes) return;
  Bvh4Node& node = nodes[id];
  Aabb all = empty_box();
  for (int k = 0; k < 4; k++) {
    const uint32_t c = node.child[k];
    if (c == kBvhEmpty) continue;
    Aabb box;
    if (c & kBvhLeafBit) {
      box = empty_box();
      const uint32_t first = c & 0x0FFFFFFFu, cnt = ((c >> 28) & 7u) + 1u;
      for (uint32_t j = 0; j < cnt && first + j < count; j++) grow(box, prim_box[first + j]);
    }
    else {
      if (c >= num_nodes) continue;
      box = node_box[c];
    }
    float lo[3], hi[3];
    for (int a = 0; a < 3; a++) {  // bvh_build.cpp set_child_box
      const float pad = 1e-5f * fmaxf(fmaxf(fabsf(box.lo[a]), fabsf(box.hi[a])), 1e-20f) + 1e-30f;
      lo[a] = box.lo[a] - pad; hi[a] = box.hi[a] + pad;
    }
    node.lo_x[k] = lo[0]; node.lo_y[k] = lo[1]; node.lo_z[k] = lo[2];
    node.hi_x[k] = hi[0]; node.hi_y[k] = hi[1]; node.hi_z[k] = hi[2];
    grow(all, box);
  }
  node_box[id] = all;
}

// ---- in the resident node array ----
// nodes: the scene's node array; a job's slots, the inner child words and (through first_tri) the leaf ranges are absolute. slot_box: by slot - capacity.
__global__ __launch_bounds__(kRefitBlock) void k_refit_level_resident(Bvh4Node* __restrict__ nodes, uint32_t capacity, uint32_t mesh_nodes, const ResidentJob* __restrict__ jobs,
                                                                      uint32_t num_jobs, uint32_t depth, Aabb* slot_box) {
  if (blockIdx.y >= num_jobs) return;
  const ResidentJob& job = jobs[blockIdx.y];
  if (depth >= job.depths || depth >= kResidentMaxDepths) return;
  const uint32_t first = job.depth_first[depth], end = job.depth_first[depth + 1];
  const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
  if (end > job.num_nodes || first > end || i >= end - first) return;
  const uint32_t slot = job.slots[first + i];
  if (slot < capacity || slot - capacity >= mesh_nodes) return;
  Bvh4Node& node = nodes[slot];
  Aabb all = empty_box();
  for (int k = 0; k < 4; k++) {
    const uint32_t c = node.child[k];
    if (c == kBvhEmpty) continue;
    Aabb box;
    if (c & kBvhLeafBit) {
      box = empty_box();
      const uint32_t tri = c & 0x0FFFFFFFu, cnt = ((c >> 28) & 7u) + 1u;
      if (tri < job.first_tri) continue;
      const uint32_t rel = tri - job.first_tri;  // (the range was rebased by the mesh's first triangle)
      for (uint32_t j = 0; j < cnt && rel + j < job.count; j++) grow(box, job.prim_box[rel + j]);
    }
    else {
      if (c < capacity || c - capacity >= mesh_nodes) continue;
      box = slot_box[c - capacity];
    }
    float lo[3], hi[3];
    for (int a = 0; a < 3; a++) {  // bvh_build.cpp set_child_box
      const float pad = 1e-5f * fmaxf(fmaxf(fabsf(box.lo[a]), fabsf(box.hi[a])), 1e-20f) + 1e-30f;
      lo[a] = box.lo[a] - pad; hi[a] = box.hi[a] + pad;
    }
    node.lo_x[k] = lo[0]; node.lo_y[k] = lo[1]; node.lo_z[k] = lo[2];
    node.hi_x[k] = hi[0]; node.hi_y[k] = hi[1]; node.hi_z[k] = hi[2];
    grow(all, box);
  }
  slot_box[slot - capacity] = all;
}

__global__ __launch_bounds__(kRefitBlock) void k_resident_mesh_boxes(const ResidentJob* __restrict__ jobs, uint32_t num_jobs, uint32_t capacity, uint32_t mesh_nodes,
                                                                     const Aabb* __restrict__ slot_box, Aabb* __restrict__ mesh_box, uint32_t num_meshes,
                                                                     ResidentResult* __restrict__ results) {
  const uint32_t j = blockIdx.x * kRefitBlock + threadIdx.x;
  if (j >= num_jobs) return;
  const uint32_t root = jobs[j].root_slot, m = jobs[j].mesh;
  if (root < capacity || root - capacity >= mesh_nodes || m >= num_meshes) return;
  const Aabb box = slot_box[root - capacity];
  mesh_box[m] = box;
  results[j].box = box;
}

// The sum of a workgroup's values in a fixed order (a tree over the thread index): thread 0 returns it.
__device__ __forceinline__ double block_sum(double v, double* shared) {
  shared[threadIdx.x] = v;
  __syncthreads();
  for (uint32_t w = kRefitBlock / 2; w > 0; w >>= 1) {
    if (threadIdx.x < w) shared[threadIdx.x] += shared[threadIdx.x + w];
    __syncthreads();
  }
  return shared[0];
}

// bvh_build.cpp bvh4_cost, a node per thread: every workgroup of a job's row writes its sum (0 behind the job's last node), stride per job.
__global__ __launch_bounds__(kRefitBlock) void k_bvh4_cost(const Bvh4Node* __restrict__ nodes, uint32_t capacity, uint32_t mesh_nodes, const ResidentJob* __restrict__ jobs,
                                                           uint32_t num_jobs, double* __restrict__ partials, uint32_t stride) {
  __shared__ double shared[kRefitBlock];
  if (blockIdx.y >= num_jobs || blockIdx.x >= stride) return;  // (uniform per workgroup)
  const ResidentJob& job = jobs[blockIdx.y];
  const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
  double term = 0.0;
  if (i < job.num_nodes) {
    const uint32_t slot = job.slots[i];
    if (slot >= capacity && slot - capacity < mesh_nodes) {
      const Bvh4Node& n = nodes[slot];
      for (int k = 0; k < 4; k++) {
        if (n.child[k] == kBvhEmpty) continue;
        const double dx = (double) n.hi_x[k] - (double) n.lo_x[k], dy = (double) n.hi_y[k] - (double) n.lo_y[k], dz = (double) n.hi_z[k] - (double) n.lo_z[k];
        term += dx * dy + dy * dz + dz * dx;
      }
    }
  }
  const double sum = block_sum(term, shared);
  if (threadIdx.x == 0) partials[(size_t) blockIdx.y * stride + blockIdx.x] = sum;
}

// One workgroup per job: the job's workgroup sums, thread t those of t, t + 256, ... in that order, then the tree.
__global__ __launch_bounds__(kRefitBlock) void k_bvh4_cost_sum(const double* __restrict__ partials, uint32_t stride, const ResidentJob* __restrict__ jobs, uint32_t num_jobs,
                                                               ResidentResult* __restrict__ results) {
  __shared__ double shared[kRefitBlock];
  if (blockIdx.x >= num_jobs) return;
  const uint32_t blocks = (jobs[blockIdx.x].num_nodes + kRefitBlock - 1) / kRefitBlock;
  double v = 0.0;
  for (uint32_t b = threadIdx.x; b < blocks && b < stride; b += kRefitBlock) v += partials[(size_t) blockIdx.x * stride + b];
  const double sum = block_sum(v, shared);
  if (threadIdx.x == 0) results[blockIdx.x].cost = sum;
}

}  // namespace

hipError_t refit_plan_create(RefitPlan& plan, const Bvh4& tree, uint32_t count) {
  plan.reset();
  std::vector<uint32_t> level_nodes;
  if (count == 0 || !bvh4_levels(tree, count, level_nodes, plan.level_first)) return hipErrorInvalidValue;
  for (uint32_t p : tree.prims) if (p >= count) return hipErrorInvalidValue;
  hipError_t e;
  if ((e = plan.nodes.assign(tree.nodes.data(), tree.nodes.size())) != hipSuccess) return e;
  if ((e = plan.prims.assign(tree.prims.data(), tree.prims.size())) != hipSuccess) return e;
  if ((e = plan.level_nodes.assign(level_nodes.data(), level_nodes.size())) != hipSuccess) return e;
  if ((e = plan.node_box.resize(tree.nodes.size())) != hipSuccess) return e;
  if ((e = plan.prim_box.resize(count)) != hipSuccess) return e;
  plan.num_nodes = (uint32_t) tree.nodes.size(); plan.count = count;
  return hipSuccess;
}

hipError_t refit_run(RefitPlan& plan, const float4* d_vertices, BvhTri* d_tris, const Aabb* host_boxes, Bvh4Node* out_nodes, Aabb* root_box, double* download_seconds) {
  if (!plan.nodes || !plan.count || plan.level_first.size() < 2 || (!d_vertices && !host_boxes) || (d_vertices && !d_tris)) return hipErrorInvalidValue;
  hipError_t e;
  if (d_vertices) {
    hipLaunchKernelGGL(k_refit_tri_boxes, dim3((plan.count + kRefitBlock - 1) / kRefitBlock), dim3(kRefitBlock), 0, 0, d_vertices, plan.prims.get(), plan.count, d_tris,
                       plan.prim_box.get());
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  else {
    std::vector<uint32_t> prims(plan.count);
    if ((e = hipMemcpy(prims.data(), plan.prims.get(), sizeof(uint32_t) * plan.count, hipMemcpyDeviceToHost)) != hipSuccess) return e;
    std::vector<Aabb> ordered(plan.count);
    for (uint32_t i = 0; i < plan.count; i++) ordered[i] = host_boxes[prims[i]];
    if ((e = hipMemcpy(plan.prim_box.get(), ordered.data(), sizeof(Aabb) * plan.count, hipMemcpyHostToDevice)) != hipSuccess) return e;
  }
  for (size_t l = plan.level_first.size() - 1; l-- > 0;) {  // deepest level first; launches on one stream run in order
    const uint32_t first = plan.level_first[l], n = plan.level_first[l + 1] - first;
    if (n == 0) continue;
    hipLaunchKernelGGL(k_refit_level, dim3((n + kRefitBlock - 1) / kRefitBlock), dim3(kRefitBlock), 0, 0, plan.nodes.get(), plan.level_nodes.get() + first, n, plan.num_nodes,
                       plan.count, plan.prim_box.get(), plan.node_box.get());
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  const auto t_download = std::chrono::steady_clock::now();
  if ((e = hipMemcpy(out_nodes, plan.nodes.get(), sizeof(Bvh4Node) * plan.num_nodes, hipMemcpyDefault)) != hipSuccess) return e;  // (waits for the launches; out_nodes may be device memory)
  e = hipMemcpy(root_box, plan.node_box.get(), sizeof(Aabb), hipMemcpyDeviceToHost);
  if (download_seconds) *download_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_download).count();
  return e;
}

hipError_t resident_mesh_create(ResidentMesh& rm, const Bvh4& tree, uint32_t count, const std::vector<uint32_t>& slots) {
  rm.reset();
  std::vector<uint32_t> depth_slots;
  if (count == 0 || !resident_depth_slots(tree, count, slots, depth_slots, rm.depth_first) || rm.depth_first.size() < 2 || rm.depth_first.size() > kResidentMaxDepths + 1) {
    rm.reset();
    return hipErrorInvalidValue;
  }
  for (uint32_t p : tree.prims) if (p >= count) { rm.reset(); return hipErrorInvalidValue; }
  hipError_t e;
  if ((e = rm.slots.assign(depth_slots.data(), depth_slots.size())) != hipSuccess || (e = rm.prims.assign(tree.prims.data(), tree.prims.size())) != hipSuccess ||
      (e = rm.prim_box.resize(count)) != hipSuccess) {
    rm.reset();
    return e;
  }
  rm.num_nodes = (uint32_t) tree.nodes.size(); rm.count = count;
  return hipSuccess;
}

hipError_t resident_refit_prepare(ResidentRefit& r, const std::vector<uint32_t>& moved, const uint32_t* mesh_tri_offset, uint32_t mesh_nodes) {
  if (moved.empty() || moved.size() > 65535u || !mesh_nodes) return hipErrorInvalidValue;  // (the job table is the grid's y)
  hipError_t e;
  if (r.slot_box.count() != mesh_nodes && (e = r.slot_box.resize(mesh_nodes)) != hipSuccess) return e;
  if (moved == r.batch && r.jobs && r.results && r.partials) return hipSuccess;
  r.batch.clear(); r.batch_first_tri.clear();
  std::vector<ResidentJob> jobs(moved.size());
  uint32_t stride = 1, widest = 1, depths = 0;
  for (size_t j = 0; j < moved.size(); j++) {
    const uint32_t m = moved[j];
    if (m >= r.mesh.size() || m >= r.mesh_slots.size() || !r.mesh[m].slots || r.mesh_slots[m].empty()) return hipErrorInvalidValue;
    const ResidentMesh& rm = r.mesh[m];
    ResidentJob& job = jobs[j];
    std::memset(&job, 0, sizeof(job));
    job.slots = rm.slots.get(); job.prim_box = rm.prim_box.get();
    job.depths = (uint32_t) rm.depth_first.size() - 1u;
    for (size_t d = 0; d < rm.depth_first.size(); d++) job.depth_first[d] = rm.depth_first[d];
    for (uint32_t d = 0; d < job.depths; d++) widest = std::max(widest, job.depth_first[d + 1] - job.depth_first[d]);
    job.num_nodes = rm.num_nodes; job.first_tri = mesh_tri_offset[m]; job.count = rm.count; job.mesh = m; job.root_slot = r.mesh_slots[m][0];
    stride = std::max(stride, (rm.num_nodes + kRefitBlock - 1) / kRefitBlock);
    depths = std::max(depths, job.depths);
  }
  if ((e = r.jobs.assign(jobs.data(), jobs.size())) != hipSuccess || (e = r.results.resize(jobs.size())) != hipSuccess ||
      (e = r.partials.resize((size_t) stride * jobs.size())) != hipSuccess)
    return e;
  r.partial_stride = stride; r.widest = widest; r.depths = depths;
  r.batch = moved;
  for (const ResidentJob& job : jobs) r.batch_first_tri.push_back(job.first_tri);
  return hipSuccess;
}

hipError_t resident_refit_run(ResidentRefit& r, const float4* d_vertices, BvhTri* d_tris, Bvh4Node* d_nodes, uint32_t capacity, uint32_t mesh_nodes, Aabb* d_mesh_box,
                              uint32_t num_meshes, ResidentResult* out, uint32_t* launches, double seconds[2]) {
  using clock = std::chrono::steady_clock;
  const uint32_t jobs = (uint32_t) r.batch.size();
  if (!jobs || r.batch_first_tri.size() != jobs || !r.jobs || !r.results || !r.partials || r.slot_box.count() != mesh_nodes || !d_vertices || !d_tris || !d_nodes || !d_mesh_box || !out) return hipErrorInvalidValue;
  hipError_t e;
  *launches = 0;
  auto t = clock::now();
  for (uint32_t j = 0; j < jobs; j++) {
    const ResidentMesh& rm = r.mesh[r.batch[j]];
    const uint32_t first_tri = r.batch_first_tri[j];
    hipLaunchKernelGGL(k_refit_tri_boxes, dim3((rm.count + kRefitBlock - 1) / kRefitBlock), dim3(kRefitBlock), 0, 0, d_vertices + 3 * (size_t) first_tri, rm.prims.get(), rm.count,
                       d_tris + first_tri, rm.prim_box.get());
    if ((e = hipGetLastError()) != hipSuccess) return e;
    (*launches)++;
  }
  for (uint32_t d = r.depths; d-- > 0;) {  // deepest first; launches on one stream run in order
    hipLaunchKernelGGL(k_refit_level_resident, dim3((r.widest + kRefitBlock - 1) / kRefitBlock, jobs), dim3(kRefitBlock), 0, 0, d_nodes, capacity, mesh_nodes,
                       (const ResidentJob*) r.jobs.get(), jobs, d, r.slot_box.get());
    if ((e = hipGetLastError()) != hipSuccess) return e;
    (*launches)++;
  }
  hipLaunchKernelGGL(k_resident_mesh_boxes, dim3((jobs + kRefitBlock - 1) / kRefitBlock), dim3(kRefitBlock), 0, 0, (const ResidentJob*) r.jobs.get(), jobs, capacity, mesh_nodes,
                     (const Aabb*) r.slot_box.get(), d_mesh_box, num_meshes, r.results.get());
  if ((e = hipGetLastError()) != hipSuccess) return e;
  (*launches)++;
  if ((e = hipDeviceSynchronize()) != hipSuccess) return e;
  seconds[0] = std::chrono::duration<double>(clock::now() - t).count();
  t = clock::now();
  hipLaunchKernelGGL(k_bvh4_cost, dim3(r.partial_stride, jobs), dim3(kRefitBlock), 0, 0, (const Bvh4Node*) d_nodes, capacity, mesh_nodes, (const ResidentJob*) r.jobs.get(), jobs,
                     r.partials.get(), r.partial_stride);
  hipLaunchKernelGGL(k_bvh4_cost_sum, dim3(jobs), dim3(kRefitBlock), 0, 0, (const double*) r.partials.get(), r.partial_stride, (const ResidentJob*) r.jobs.get(), jobs, r.results.get());
  if ((e = hipGetLastError()) != hipSuccess) return e;
  *launches += 2;
  e = hipMemcpy(out, r.results.get(), sizeof(ResidentResult) * jobs, hipMemcpyDeviceToHost);  // (waits for the launches)
  seconds[1] = std::chrono::duration<double>(clock::now() - t).count();
  return e;
}

}  // namespace lum

// lum_core.h lumc_bvh_refit_probe: a tree built over `built_boxes` by `builder`, refitted to `refit_boxes` on the host or on the device (tests/test_mesh_refit*.py)
extern "C" int lumc_bvh_refit_probe(const float* built_boxes, const float* refit_boxes, uint32_t count, uint32_t refit_count, int builder, int on_gpu, uint64_t sizes[3],
                                    void* built_nodes, void* refit_nodes, void* host_refit_nodes, uint32_t* prims, double cost[3], uint64_t* valid) {
  using namespace lum;
  if (!built_boxes || !refit_boxes || !sizes || count == 0) return 1;
  const Aabb* in = reinterpret_cast<const Aabb*>(built_boxes);
  const Aabb* to = reinterpret_cast<const Aabb*>(refit_boxes);
  Bvh4 tree;
  if (builder == 1) tree = build_bvh4_lbvh(in, count, kBvhLeafMaxTri, 26);
  else if (builder == 2) tree = build_bvh4_ploc(in, count, kBvhLeafMaxTri, 26);
  else if (builder == 3) tree = build_bvh4_sah_gpu(in, count, kBvhLeafMaxTri, 26);
  else if (builder == 0) tree = build_bvh4(in, count, kBvhLeafMaxTri, 26);
  if (tree.nodes.empty()) return 1;  // no silent fall back to another builder: the caller asked for this one
  const Bvh4 host_refit = refit_bvh4(tree, to, refit_count);
  Bvh4 refit;
  if (!on_gpu) refit = host_refit;
  else if (tree.prims.size() == refit_count) {
    RefitPlan plan;
    if (refit_plan_create(plan, tree, refit_count) != hipSuccess) return 1;
    refit.nodes.resize(tree.nodes.size()); refit.prims = tree.prims; refit.max_depth = tree.max_depth;
    Aabb root;
    if (refit_run(plan, nullptr, nullptr, to, refit.nodes.data(), &root) != hipSuccess) return 1;
  }
  sizes[0] = tree.nodes.size(); sizes[1] = tree.prims.size(); sizes[2] = refit.nodes.size();
  if (built_nodes) std::memcpy(built_nodes, tree.nodes.data(), sizeof(Bvh4Node) * tree.nodes.size());
  if (refit_nodes && !refit.nodes.empty()) std::memcpy(refit_nodes, refit.nodes.data(), sizeof(Bvh4Node) * refit.nodes.size());
  if (host_refit_nodes && !host_refit.nodes.empty()) std::memcpy(host_refit_nodes, host_refit.nodes.data(), sizeof(Bvh4Node) * host_refit.nodes.size());
  if (prims) std::memcpy(prims, tree.prims.data(), sizeof(uint32_t) * tree.prims.size());
  if (cost) { cost[0] = bvh4_cost(tree); cost[1] = refit.nodes.empty() ? 0.0 : bvh4_cost(refit); cost[2] = host_refit.nodes.empty() ? 0.0 : bvh4_cost(host_refit); }
  if (valid) *valid = (!refit.nodes.empty() && refit.prims == tree.prims && bvh4_valid(refit, to, refit_count)) ? 1u : 0u;
  return 0;
}
