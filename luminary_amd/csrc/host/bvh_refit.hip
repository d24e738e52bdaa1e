// GPU refit of a mesh's 4-wide tree after its vertices moved (luminary_ext_set_mesh_positions -> LUMC_DIRTY_MESH_POSITIONS): the topology stays, every
// child box becomes the builders' pad of the exact union of what lies below it. Host twin, and the checker of this unit: bvh_build.cpp refit_bvh4 - the
// union is min / max (exact, order-free up to the sign of a zero, and the order is the host's), the pad the one expression of set_child_box, compiled
// here without contraction like there: both give the same bytes.
//
//   k_refit_tri_boxes   one thread per triangle in leaf order: its box from the device scene's vertices; rewrites the triangle's traversal geometry
//   k_refit_level       one thread per node of ONE level, deepest level first, one launch per level: the kernel boundary is what makes a level's exact
//                       boxes (a per-node scratch array) visible to the level above - no in-launch hand-off, no counters. At most 26 launches.
// The per-level node lists come from one breadth-first walk on the host (bvh4_levels): the GPU builders number nodes through atomics, levels are no ranges.
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
  if ((e = hipMemcpy(out_nodes, plan.nodes.get(), sizeof(Bvh4Node) * plan.num_nodes, hipMemcpyDeviceToHost)) != hipSuccess) return e;  // (waits for the launches)
  e = hipMemcpy(root_box, plan.node_box.get(), sizeof(Aabb), hipMemcpyDeviceToHost);
  if (download_seconds) *download_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_download).count();
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
