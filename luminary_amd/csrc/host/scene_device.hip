// The scene on the device (lumc_scene_upload, lumc_scene_update and what they need): the process-wide cache of mesh trees, the particle tree, one update_*
// function per part of the scene, mesh refit, and the tables generated on the device - cloud noise, the sky's and the BSDFs' look-up tables, the sky panorama -
// with the entry points that read them back; the BVH settings and statistics. Shares nothing with the render schedule (core.hip) but LumContext; launches the
// kernels of device/kernels_scene.h, which this unit alone includes, compiled with the exact flavour's flags.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cfloat>
#include <cstring>
#include <map>
#include <string>
#include <mutex>
#include <tuple>

#include "../../../include/lum_core.h"
#include "../device/kernels_scene.h"
#include "context.h"
#include "update_plan.h"

namespace {

// Wall time since it was made, in seconds (`t = Stopwatch{}` starts it again).
struct Stopwatch {
  std::chrono::steady_clock::time_point start = std::chrono::steady_clock::now();
  double seconds() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count(); }
};

// What the stats of an update say about that update alone, before it runs; the counts since the context was created stay.
void reset_update(LumMeshRefitStats& st) {
  st.last_refits = st.last_rebuilds = 0; st.max_cost_growth = st.seconds = st.seconds_upload = st.seconds_refit = st.seconds_rebuild = st.seconds_assemble = 0.0;
  st.seconds_hash = st.seconds_download = st.seconds_lights = 0.0;
}
void reset_update(LumResidentRefitStats& rs) {
  rs.last_meshes = rs.last_launches = 0; rs.last_bytes_downloaded = 0;
  rs.seconds = rs.seconds_upload = rs.seconds_hash = rs.seconds_refit = rs.seconds_cost = rs.seconds_top_level = 0.0;
}
void reset_update(LumInstanceUpdateStats& st) { st.seconds = st.seconds_relayout = st.seconds_upload = st.seconds_boxes = st.seconds_build = st.seconds_leaves = 0.0; }

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

// A scene array on the device: a copy of the host's in its owner (ctx->arrays), with the scene's view of it. No host array or no elements: empty and null.
template <typename T>
int upload(LumContext* ctx, DeviceBuffer<T>& owner, const T* host, size_t count, const T** view) {
  *view = nullptr;
  HIP_TRY(ctx, owner.assign(host, count));
  *view = owner.get();
  return 0;
}

// A part's views from its owners: null for a part of ctx->arrays that was just released (`arrays.lights = {}`), its arrays for a filled one.
void point_views(DeviceScene& sc, const SceneArrays::Mesh& a) { sc.mesh_tri_offset = a.tri_offset.get(); sc.vertices = a.vertices.get(); sc.tri_tex = a.tri_tex.get(); sc.blas_tris = a.blas_tris.get(); }
void point_views(DeviceScene& sc, const SceneArrays::Inst& a) {
  sc.instance_mesh_ids = a.mesh_ids.get(); sc.instance_transforms = a.transforms.get(); sc.instance_rows = a.rows.get(); sc.tlas_leaves = a.tlas_leaves.get(); sc.bvh_nodes = a.nodes.get();
}
void point_views(DeviceScene& sc, const SceneArrays::Lights& a) {
  sc.light_tree_root = a.tree_root.get(); sc.light_tree_nodes = a.tree_nodes.get(); sc.light_root_children = a.root_children.get(); sc.light_tri_handles = a.tri_handles.get();
  sc.light_tri_table = a.tri_table.get(); sc.light_nodes = a.bvh_nodes.get(); sc.light_tris = a.bvh_tris.get();
}
void point_views(DeviceScene& sc, const SceneArrays::Textures& a) { sc.texture_table = a.table.get(); sc.texels = a.texels.get(); }
void point_views(DeviceScene& sc, const SceneArrays::Constants& a) {  // (the caller's copies; where there is none update_constants' functions point at the context's own tables)
  sc.sky_stars = a.stars.get(); sc.sky_stars_offsets = a.stars_offsets.get(); sc.sky_hdri = a.sky_hdri.get();
  sc.cloud_noise_shape = a.cloud_noise[0].get(); sc.cloud_noise_detail = a.cloud_noise[1].get(); sc.cloud_noise_weather = a.cloud_noise[2].get();
  sc.sky_lut_transmittance = a.sky_lut[0].get(); sc.sky_lut_multiscattering = a.sky_lut[1].get();
}
void point_views(DeviceScene& sc, const SceneArrays::Particles& a) {
  sc.particle_bvh_nodes = a.nodes.get(); sc.particle_tris = a.tris.get(); sc.particle_leaves = a.leaves.get(); sc.particle_normals = a.normals.get();
}

void mesh_boxes_changed(LumContext* ctx) { ctx->instance_update.prepared = false; }  // the moved instances' scratch holds a copy of ctx->mesh_box

void free_scene(LumContext* ctx) {
  ctx->arrays = SceneArrays{};
  for (auto& t : ctx->d_luts) t.reset();
  for (auto& t : ctx->d_sky_lut) t.reset();
  ctx->sky_lut_key.clear();
  ctx->d_bridge_lut.reset(); ctx->bridge_lut_host.clear();
  ctx->mesh_bvh.clear(); ctx->mesh_box.clear(); ctx->mesh_refit.clear(); ctx->mesh_tri_offset.clear();
  ctx->instance_update.reset(); ctx->instance_mesh_ids.clear();
  ctx->tri_material.clear(); ctx->material_words.clear(); ctx->light_handles.clear(); ctx->light_tree_flat = true;
  ctx->resident_refit.drop_layout(); ctx->stale_meshes = 0;
  ctx->mesh_deform.clear(); ctx->d_skin_flags.reset();
  ctx->mesh_shutter.clear(); ctx->d_shutter_flags.reset();
  ctx->light_refit.reset(); ctx->light_bvh = Bvh4{}; ctx->light_refit_needs_rebuild = false;
  ctx->has_scene = false;
}

// Mesh m's tree as a copy private to this context, made from the held one if it has none: what a refit writes (the shared, cached tree is never written, and the
// cache never sees this one). Becomes the held tree when the caller says so (ctx->mesh_bvh[m] = ctx->mesh_refit[m].own).
MeshTree& private_tree_of(LumContext* ctx, size_t m) {
  MeshRefit& mr = ctx->mesh_refit[m];
  if (!mr.own || mr.own.get() != ctx->mesh_bvh[m].get()) {
    const Bvh4& held = ctx->mesh_bvh[m]->bvh;
    mr.own = std::make_shared<MeshTree>();
    mr.own->bvh.prims = held.prims; mr.own->bvh.max_depth = held.max_depth; mr.own->built_on_gpu = ctx->mesh_bvh[m]->built_on_gpu;
    mr.own->bvh.nodes = held.nodes;
  }
  return *mr.own;
}

// Host copies after refits in the resident node array (refit_in_place below): ctx->mesh_bvh[m] of a mesh marked stale holds the boxes of earlier vertices, and a
// tree assembled or laid out from them would lose hits. Every reader of those nodes calls this first: the mesh part of the node array comes down, the box floats
// go through the layout's slot map into the mesh's private tree (private_tree_of), the mark goes. Needs the layout the refits ran in: whoever drops it calls this before.
int restore_stale_meshes(LumContext* ctx) {
  if (!ctx->stale_meshes) return 0;
  const ResidentRefit& rr = ctx->resident_refit;
  const DeviceBuffer<Bvh4Node>& d_nodes = ctx->arrays.inst.nodes;
  if (rr.mesh_slots.size() != ctx->mesh_bvh.size() || ctx->mesh_refit.size() != ctx->mesh_bvh.size() || !rr.mesh_nodes || d_nodes.count() != (size_t) rr.capacity + rr.mesh_nodes) {
    ctx->error = "meshes refitted in the resident node array, and the layout they were refitted in is gone";
    return 1;
  }
  std::vector<Bvh4Node> nodes(rr.mesh_nodes);
  HIP_TRY(ctx, hipMemcpy(nodes.data(), d_nodes.get() + rr.capacity, sizeof(Bvh4Node) * rr.mesh_nodes, hipMemcpyDeviceToHost));
  for (size_t m = 0; m < ctx->mesh_refit.size(); m++) {
    MeshRefit& mr = ctx->mesh_refit[m];
    if (!mr.stale) continue;
    const std::vector<uint32_t>& slots = rr.mesh_slots[m];
    if (slots.size() != ctx->mesh_bvh[m]->bvh.nodes.size()) { ctx->error = "the resident layout's slot map does not fit the mesh's tree"; return 1; }
    Bvh4& own = private_tree_of(ctx, m).bvh;
    for (size_t i = 0; i < slots.size(); i++) {
      if (slots[i] < rr.capacity || slots[i] - rr.capacity >= rr.mesh_nodes) { ctx->error = "the resident layout's slot map points outside the mesh part"; return 1; }
      std::memcpy(&own.nodes[i], &nodes[slots[i] - rr.capacity], offsetof(Bvh4Node, child));  // the 24 box floats; the child words stay relative to the mesh
    }
    ctx->mesh_bvh[m] = mr.own;
    mr.stale = false;
  }
  ctx->stale_meshes = 0;
  return 0;
}

}  // namespace

int scene_device_init() { return (int) exact::upload_sampler_seeds(); }  // this unit's own table: k_sky_hdri and k_generate_lut draw random numbers

extern "C" {

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
static int build_particle_tree(LumContext* ctx, const LumDeviceSceneView* v, DeviceScene& sc) {
  SceneArrays::Particles& a = ctx->arrays.particles;
  a = {}; point_views(sc, a);
  sc.particle_tlas_num_nodes = 0;
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
  if (upload(ctx, a.nodes, nodes.data(), nodes.size(), &sc.particle_bvh_nodes)) return 1;
  if (upload(ctx, a.tris, tris.data(), tris.size(), &sc.particle_tris)) return 1;
  if (upload(ctx, a.leaves, leaves.data(), leaves.size(), &sc.particle_leaves)) return 1;
  if (upload(ctx, a.normals, (const float4*) v->particle_normals, (size_t) sc.particles_count, &sc.particle_normals)) return 1;
  sc.particle_tlas_num_nodes = (uint32_t) tlas.nodes.size();
  sc.particle_num_leaves = (uint32_t) (leaves.size() / 4);
  ctx->particle_lds_nodes = (uint32_t) std::min<size_t>(ctx->lds_nodes, nodes.size());
  return 0;
}

// ---- the scene on the device, part by part (scene_update below runs the parts in this order). A part frees what it allocated before; a part that is not
// dirty keeps its device arrays and the fields of ctx->scene that point at them. ----
static uint32_t total_triangles(const LumDeviceSceneView* v) { return v->num_meshes ? v->mesh_tri_offset[v->num_meshes] : 0; }
static bool scene_too_large(LumContext* ctx, const LumDeviceSceneView* v, size_t num_nodes) {
  if (total_triangles(v) < (1u << 28) && num_nodes < (1u << 25)) return false;
  ctx->error = "scene too large for 28-bit leaf ranges / 32-bit node offsets";
  return true;
}

// The meshes' vertex arrays. The traversal triangles stay: new meshes bring new ones (scene_update has released them, update_scene_tree uploads them), moved
// vertices are written into the ones that are there (refit_mesh_copies, refit_in_place).
static int update_mesh_arrays(LumContext* ctx, const LumDeviceSceneView* v) {
  DeviceScene& sc = ctx->scene;
  SceneArrays::Mesh& a = ctx->arrays.mesh;
  const uint32_t total_tris = total_triangles(v);
  a.tri_offset.reset(); a.vertices.reset(); a.tri_tex.reset(); point_views(sc, a);
  if (upload(ctx, a.tri_offset, v->mesh_tri_offset, (size_t) v->num_meshes + 1, &sc.mesh_tri_offset)) return 1;
  if (upload(ctx, a.vertices, (const float4*) v->vertices, (size_t) total_tris * 3, &sc.vertices)) return 1;
  ctx->tri_material.resize(total_tris);
  for (uint32_t t = 0; t < total_tris; t++) ctx->tri_material[t] = (uint16_t) (v->tri_tex[4 * (size_t) t + 3] & 0xFFFFu);  // (scene_traits)
  return upload(ctx, a.tri_tex, (const uint4*) v->tri_tex, (size_t) total_tris, &sc.tri_tex);
}

// Releases the whole part; update_scene_tree, which runs whenever this does, uploads the rows, the node array and the leaf records.
static int update_instance_arrays(LumContext* ctx, const LumDeviceSceneView* v) {
  DeviceScene& sc = ctx->scene;
  SceneArrays::Inst& a = ctx->arrays.inst;
  if (restore_stale_meshes(ctx)) return 1;  // (the node array goes: what was refitted in it comes down first)
  a = {}; point_views(sc, a);
  ctx->instance_mesh_ids.assign(v->instance_mesh_ids, v->instance_mesh_ids + v->num_instances);
  if (upload(ctx, a.mesh_ids, v->instance_mesh_ids, v->num_instances, &sc.instance_mesh_ids)) return 1;
  return upload(ctx, a.transforms, (const float4*) v->instance_transforms, (size_t) v->num_instances * 2, &sc.instance_transforms);
}

static int update_materials(LumContext* ctx, const LumDeviceSceneView* v) {
  ctx->arrays.materials = {};
  ctx->material_words.assign(v->materials, v->materials + 16 * (size_t) v->num_materials);  // (scene_traits)
  return upload(ctx, ctx->arrays.materials.materials, (const uint4*) v->materials, (size_t) v->num_materials * 2, &ctx->scene.materials);
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
  return upload(ctx, ctx->arrays.lights.root_children, table.data(), table.size(), &ctx->scene.light_root_children);
}

// Releases the whole part; update_light_bvh and update_counts_and_tables, which run whenever this does, bring the light BVH and k_light_table's records.
static int update_light_tree(LumContext* ctx, const LumDeviceSceneView* v) {
  DeviceScene& sc = ctx->scene;
  SceneArrays::Lights& a = ctx->arrays.lights;
  a = {}; point_views(sc, a);
  sc.light_num_nodes = 0;
  ctx->light_handles.clear(); ctx->light_tree_flat = true;  // (scene_traits)
  if (!v->light_tree_root || !v->num_lights) return 0;
  ctx->light_handles.assign(v->light_tri_handles, v->light_tri_handles + 2 * (size_t) v->num_lights);
  ctx->light_tree_flat = v->num_light_tree_nodes == 0;  // the builder makes a node for every root child that is not a light (scene.cpp: the collapse's jobs)
  const uint32_t sections = v->light_tree_root[10];
  if (upload(ctx, a.tree_root, (const uint4*) v->light_tree_root, (size_t) 1 + 3 * sections, &sc.light_tree_root)) return 1;
  if (upload_light_root_children(ctx, v, sections)) return 1;
  if (upload(ctx, a.tree_nodes, (const uint4*) v->light_tree_nodes, (size_t) v->num_light_tree_nodes * 4, &sc.light_tree_nodes)) return 1;
  return upload(ctx, a.tri_handles, (const uint2*) v->light_tri_handles, v->num_lights, &sc.light_tri_handles);
}

static int update_textures(LumContext* ctx, const LumDeviceSceneView* v) {
  DeviceScene& sc = ctx->scene;
  SceneArrays::Textures& a = ctx->arrays.textures;
  a = {}; point_views(sc, a);
  sc.num_textures = 0;
  if (!v->num_textures || !v->texture_table || !v->texels) return 0;
  size_t texel_count = 0;
  for (uint32_t t = 0; t < v->num_textures; t++)
    texel_count = std::max(texel_count, (size_t) v->texture_table[4 * t] + (size_t) v->texture_table[4 * t + 1] * v->texture_table[4 * t + 2]);
  if (upload(ctx, a.table, (const uint4*) v->texture_table, v->num_textures, &sc.texture_table)) return 1;
  if (upload(ctx, a.texels, v->texels, texel_count, &sc.texels)) return 1;
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
  mesh_boxes_changed(ctx);
  ctx->mesh_refit.clear(); ctx->mesh_refit.resize(v->num_meshes); ctx->stale_meshes = 0;
  ctx->mesh_tri_offset.assign(v->mesh_tri_offset, v->mesh_tri_offset + v->num_meshes + 1);
  blas_tris.assign((size_t) total_triangles(v) + 1, BvhTri{});
  for (uint32_t m = 0; m < v->num_meshes; m++) {
    const uint32_t t0 = v->mesh_tri_offset[m], nt = v->mesh_tri_offset[m + 1] - t0;
    const float* vertices = v->vertices + (size_t) t0 * 12;
    std::vector<Aabb> tri_boxes(nt);
    ctx->mesh_box[m] = mesh_triangle_boxes(vertices, nt, tri_boxes.data());
    const Stopwatch t_build;
    const MeshTreeKey key = mesh_tree_key(vertices, nt, ctx->bvh_builder);
    std::shared_ptr<const MeshTree> tree = cached_or_built_mesh_tree(ctx, key, tri_boxes.data(), nt);
    if (!tree) return 1;
    ctx->bvh_meshes_by_builder[tree->built_on_gpu ? 1 : 0]++;
    ctx->bvh_build_seconds += t_build.seconds();
    fill_mesh_tris(vertices, t0, tree->bvh.prims.data(), nt, blas_tris.data() + t0);
    ctx->mesh_bvh[m] = std::move(tree);
    ctx->mesh_refit[m].fit_hash[0] = key.h0; ctx->mesh_refit[m].fit_hash[1] = key.h1;
  }
  return 0;
}

// ---- skinned and morphed meshes (lum_core.h lumc_mesh_skin_bind, lumc_mesh_morph_bind; mesh_deform.hip; DESIGN.md sections 11 and 12) ----
// A kernel wrote the scene's vertices of mesh m: the view's vertices of it are never trusted.
static bool written_on_device(const LumContext* ctx, uint32_t m) {
  const auto it = ctx->mesh_deform.find(m);
  if (it != ctx->mesh_deform.end() && it->second.written_on_device()) return true;
  const auto sh = ctx->mesh_shutter.find(m);
  return sh != ctx->mesh_shutter.end() && sh->second.both();  // (a mesh that holds both keys is k_shutter_vertices')
}

// The skinning step of an update that touches vertices (find_moved_meshes runs it, once), after the vertex arrays are in place and before anything reads them: every
// pending palette and every pending weight set goes up and k_deform_mesh writes its mesh's range of the scene's vertices (those meshes are moved: *posed,
// ascending) - with the mesh's morph if it has one, and with its skin once that has a palette; after an upload of the vertex arrays
// from the view (view_uploaded) every other bound mesh a kernel has written is written again from the palette and the weights it holds - the same bits as before
// the upload, so its tree still fits. One launch per mesh. Then the launches' flag words come back: a position that is not finite fails the update.
static int skin_meshes(LumContext* ctx, bool view_uploaded, std::vector<uint32_t>* posed) {
  std::vector<std::pair<uint32_t, MeshDeform*>> jobs;  // ascending
  bool any_skin = false, any_morph = false;
  for (auto& kv : ctx->mesh_deform) {
    MeshDeform& d = kv.second;
    if (!d.pending() && !(view_uploaded && d.written_on_device())) continue;
    any_skin = any_skin || !d.morph || d.new_pose();
    any_morph = any_morph || d.morph;
    jobs.emplace_back(kv.first, &d);
  }
  if (jobs.empty()) return 0;
  LumMeshSkinStats& st = ctx->skin_stats;
  LumMeshMorphStats& mst = ctx->morph_stats;
  if (any_skin) { st.last_meshes = st.last_launches = 0; st.last_bytes_uploaded = 0; st.seconds = st.seconds_upload = st.seconds_skin = 0.0; }
  if (any_morph) { mst.last_meshes = mst.last_launches = 0; mst.last_bytes_uploaded = 0; mst.seconds = mst.seconds_upload = mst.seconds_morph = 0.0; }
  DeviceBuffer<float4>& vertices = ctx->arrays.mesh.vertices;
  for (const auto& [m, d] : jobs) {  // every range a kernel will write, against the array that is there
    if ((size_t) m + 1 >= ctx->mesh_tri_offset.size() || 3 * (size_t) ctx->mesh_tri_offset[m + 1] > vertices.count() ||
        (d->skin_writes() && ctx->mesh_tri_offset[m + 1] - ctx->mesh_tri_offset[m] != d->skin->triangles) ||
        (d->morph && ctx->mesh_tri_offset[m + 1] - ctx->mesh_tri_offset[m] != d->morph->triangles)) {
      ctx->error = "lumc_scene_update: mesh " + std::to_string(m) + " is bound to a " + (d->morph ? "morph" : "skin") + " of another triangle count than the scene on the device";
      return 1;
    }
  }
  const Stopwatch t_all;
  if (ctx->d_skin_flags.count() < jobs.size()) HIP_TRY(ctx, ctx->d_skin_flags.resize(jobs.size()));
  HIP_TRY(ctx, hipMemset(ctx->d_skin_flags.get(), 0, sizeof(uint32_t) * jobs.size()));
  for (const auto& [m, d] : jobs) {
    if (d->new_pose()) {
      HIP_TRY(ctx, hipMemcpy(d->skin->palette.get(), d->skin->pending.data(), sizeof(float) * d->skin->pending.size(), hipMemcpyHostToDevice));
      st.last_bytes_uploaded += sizeof(float) * d->skin->pending.size();
    }
    if (d->new_weights()) {
      if (d->morph->pending.size() != d->morph->weights.count()) { ctx->error = "lumc_scene_update: mesh " + std::to_string(m) + " holds weights of another target count"; return 1; }
      HIP_TRY(ctx, hipMemcpy(d->morph->weights.get(), d->morph->pending.data(), sizeof(float) * d->morph->pending.size(), hipMemcpyHostToDevice));
      mst.last_bytes_uploaded += sizeof(float) * d->morph->pending.size();
    }
  }
  HIP_TRY(ctx, hipDeviceSynchronize());
  const double seconds_upload = t_all.seconds();
  const Stopwatch t_skin;
  for (size_t j = 0; j < jobs.size(); j++) {
    const MeshDeform& d = *jobs[j].second;
    HIP_TRY(ctx, mesh_deform_launch(d, vertices.get() + 3 * (size_t) ctx->mesh_tri_offset[jobs[j].first], ctx->d_skin_flags.get() + j));
    if (d.morph) mst.last_launches++;
    if (!d.morph || d.new_pose()) st.last_launches++;
  }
  std::vector<uint32_t> flags(jobs.size());
  HIP_TRY(ctx, hipMemcpy(flags.data(), ctx->d_skin_flags.get(), sizeof(uint32_t) * jobs.size(), hipMemcpyDeviceToHost));  // (waits for the launches)
  if (any_skin) { st.seconds_upload = seconds_upload; st.seconds_skin = t_skin.seconds(); st.seconds = t_all.seconds(); }
  if (any_morph) { mst.seconds_upload = seconds_upload; mst.seconds_morph = t_skin.seconds(); mst.seconds = t_all.seconds(); }
  for (size_t j = 0; j < jobs.size(); j++) {
    const std::string mesh = "lumc_scene_update: mesh " + std::to_string(jobs[j].first);
    if (flags[j] & kSkinFlagBadBone) { ctx->error = mesh + ": a bone id beyond the palette reached the skinning kernel"; return 1; }
    if (flags[j] & kMorphFlagBadLayout) { ctx->error = mesh + ": a target id or a row beyond the binding reached the morph kernel"; return 1; }
    if (flags[j] & kSkinFlagNotFinite) { ctx->error = mesh + (jobs[j].second->morph ? ": the weights give a position that is not finite" : ": the pose gives a position that is not finite"); return 1; }
  }
  for (const auto& [m, d] : jobs) {
    if (d->pending()) posed->push_back(m);
    if (d->new_pose()) { d->skin->pending.clear(); d->skin->posed = true; st.poses++; st.last_meshes++; }
    if (d->new_weights()) { d->morph->pending.clear(); d->morph->applied = true; mst.applied++; mst.last_meshes++; }
  }
  return 0;
}

// ---- shutter keys (lum_core.h lumc_mesh_shutter_key, lumc_shutter_time; mesh_shutter.hip) ----
// The shutter step of an update that touches vertices (find_moved_meshes runs it, once), after skin_meshes' launches and before anything reads the vertices: every
// mesh with a pending time is written by k_shutter_vertices at that time between its keys (those meshes are moved: appended to *posed); after an upload of the
// vertex arrays from the view (view_uploaded) every other mesh that holds both keys is written again at its last time - the same bits as before the upload, so its
// tree still fits. One launch per mesh, nothing goes up. Then the launches' flag words come back: a coordinate that is not finite fails the update.
static int shutter_meshes(LumContext* ctx, bool view_uploaded, bool counts_as_slice, std::vector<uint32_t>* posed) {
  std::vector<std::pair<uint32_t, MeshShutter*>> jobs;  // ascending
  for (auto& kv : ctx->mesh_shutter)
    if (kv.second.both() && (kv.second.pending || view_uploaded)) jobs.emplace_back(kv.first, &kv.second);
  if (jobs.empty()) return 0;
  LumShutterStats& st = ctx->shutter_stats;
  st.last_meshes = st.last_launches = 0; st.last_bytes_uploaded = 0; st.seconds = 0.0;
  DeviceBuffer<float4>& vertices = ctx->arrays.mesh.vertices;
  for (const auto& [m, s] : jobs) {  // every range a kernel will write, against the array that is there
    if ((size_t) m + 1 >= ctx->mesh_tri_offset.size() || 3 * (size_t) ctx->mesh_tri_offset[m + 1] > vertices.count() ||
        ctx->mesh_tri_offset[m + 1] - ctx->mesh_tri_offset[m] != s->triangles) {
      ctx->error = "lumc_scene_update: mesh " + std::to_string(m) + " holds shutter keys of another triangle count than the scene on the device";
      return 1;
    }
  }
  const Stopwatch t_all;
  if (ctx->d_shutter_flags.count() < jobs.size()) HIP_TRY(ctx, ctx->d_shutter_flags.resize(jobs.size()));
  HIP_TRY(ctx, hipMemset(ctx->d_shutter_flags.get(), 0, sizeof(uint32_t) * jobs.size()));
  for (size_t j = 0; j < jobs.size(); j++) {
    const size_t first = 3 * (size_t) ctx->mesh_tri_offset[jobs[j].first];
    HIP_TRY(ctx, mesh_shutter_launch(*jobs[j].second, vertices.get() + first, vertices.count() - first, ctx->d_shutter_flags.get() + j));
    st.last_launches++;
  }
  std::vector<uint32_t> flags(jobs.size());
  HIP_TRY(ctx, hipMemcpy(flags.data(), ctx->d_shutter_flags.get(), sizeof(uint32_t) * jobs.size(), hipMemcpyDeviceToHost));  // (waits for the launches)
  st.seconds = t_all.seconds();
  for (size_t j = 0; j < jobs.size(); j++)
    if (flags[j] & kShutterFlagNotFinite) { ctx->error = "lumc_scene_update: mesh " + std::to_string(jobs[j].first) + ": the shutter keys give a position that is not finite"; return 1; }
  bool any_pending = false;
  for (const auto& [m, s] : jobs)
    if (s->pending) { posed->push_back(m); s->pending = false; st.last_meshes++; any_pending = true; }
  if (any_pending && counts_as_slice) st.slices++;
  return 0;
}

// A posed mesh's vertices for a builder: its 3 * nt records as the device holds them, the layout of the view's `vertices`. Counted.
static int download_posed_vertices(LumContext* ctx, uint32_t m, uint32_t t0, uint32_t nt, std::vector<float>& out) {
  out.resize(12 * (size_t) nt);
  if (3 * ((size_t) t0 + nt) > ctx->arrays.mesh.vertices.count()) { ctx->error = "lumc_scene_update: a posed mesh lies outside the vertex array"; return 1; }
  HIP_TRY(ctx, hipMemcpy(out.data(), ctx->arrays.mesh.vertices.get() + 3 * (size_t) t0, sizeof(float) * out.size(), hipMemcpyDeviceToHost));
  const auto it = ctx->mesh_deform.find(m);
  if (it != ctx->mesh_deform.end() && it->second.morph) ctx->morph_stats.rebuild_downloads++;  // (LumMeshSkinStats keeps its meaning for meshes that are only skinned)
  else ctx->skin_stats.rebuild_downloads++;
  return 0;
}

// ---- moved vertices (LUMC_DIRTY_MESH_POSITIONS, LUMC_DIRTY_MESH_SKIN with a pending pose): the meshes that moved are found once, then one of two paths gives
// each a tree for its vertices - refit_in_place in the resident node array, refit_mesh_copies in copies on the host ----
struct MovedMeshes {
  std::vector<uint32_t> meshes;   // ascending
  std::vector<MeshTreeKey> keys;  // of the view's vertices; zeros for a posed mesh (no host vertices hash to what k_deform_mesh wrote)
  std::vector<bool> posed;        // moved by a pose: no hash, and the view's vertices of it are never read
  bool refittable = true;         // every one's tree has one reference per triangle (false - spatial splits -: refit_mesh_copies builds that mesh again)
  double seconds = 0.0;           // what finding them took, uploads and skinning included: the head of either path's `seconds`
};

// The front end of both paths: the vertex arrays of the same meshes again - the traversal triangles stay on the device (update_mesh_arrays) -, the skinning step,
// then the meshes whose vertices differ from those their held tree was fitted to: by a pose, or - among the others, where the view's vertices were taken over -
// by their hashes. upload_view: the view's vertex arrays are taken over (false: poses alone - only posed meshes move, the view's vertices are not read).
static int find_moved_meshes(LumContext* ctx, const LumDeviceSceneView* v, bool upload_view, bool shutter_slice, MovedMeshes* out) {
  LumMeshRefitStats& st = ctx->refit_stats;
  reset_update(st);
  if (ctx->mesh_bvh.size() != v->num_meshes || ctx->mesh_refit.size() != v->num_meshes || ctx->mesh_tri_offset.size() != (size_t) v->num_meshes + 1 ||
      std::memcmp(ctx->mesh_tri_offset.data(), v->mesh_tri_offset, sizeof(uint32_t) * ((size_t) v->num_meshes + 1)) != 0) {
    ctx->error = "lumc_scene_update: LUMC_DIRTY_MESH_POSITIONS with other meshes or triangle counts than the scene on the device";
    return 1;
  }
  const Stopwatch t_all;
  if (!ctx->arrays.mesh.blas_tris.get()) { ctx->error = "lumc_scene_update: the scene on the device has no traversal triangles"; return 1; }
  if (upload_view && update_mesh_arrays(ctx, v)) return 1;
  HIP_TRY(ctx, hipDeviceSynchronize());
  st.seconds_upload = t_all.seconds();
  std::vector<uint32_t> posed;
  if (skin_meshes(ctx, upload_view, &posed)) return 1;
  if (shutter_meshes(ctx, upload_view, shutter_slice, &posed)) return 1;
  std::sort(posed.begin(), posed.end());
  posed.erase(std::unique(posed.begin(), posed.end()), posed.end());
  for (uint32_t m = 0; m < v->num_meshes; m++) {
    const uint32_t t0 = v->mesh_tri_offset[m], nt = v->mesh_tri_offset[m + 1] - t0;
    if (nt == 0) continue;
    const bool by_pose = std::binary_search(posed.begin(), posed.end(), m);
    if (!by_pose && (!upload_view || written_on_device(ctx, m))) continue;
    MeshTreeKey key{};
    if (!by_pose) {
      const Stopwatch t_hash;
      key = mesh_tree_key(v->vertices + (size_t) t0 * 12, nt, ctx->bvh_builder);
      st.seconds_hash += t_hash.seconds();
      const MeshRefit& mr = ctx->mesh_refit[m];
      if (!mr.fit_to_pose && key.h0 == mr.fit_hash[0] && key.h1 == mr.fit_hash[1]) continue;  // the held tree fits these vertices
    }
    out->meshes.push_back(m); out->keys.push_back(key); out->posed.push_back(by_pose);
    if (ctx->mesh_bvh[m]->bvh.prims.size() != nt) out->refittable = false;
  }
  out->seconds = t_all.seconds();
  return 0;
}

// The moved meshes' trees in copies on the host: refitted on the device (bvh_refit.hip; the tree becomes private to this context, the shared one it came from is
// not touched and the cache never sees the refitted one) or, where the mode, the cost's growth or a tree that cannot be refitted says so, from the cache / the
// builder like an upload; scene_update assembles the node array from them. Also what an in-place update that fell back goes on with: the meshes refitted in the
// resident array come back to the host first. *rebuilt: a mesh's traversal triangles were written anew (k_tri_opacity).
static int refit_mesh_copies(LumContext* ctx, const LumDeviceSceneView* v, const MovedMeshes& moved, bool* rebuilt) {
  DeviceScene& sc = ctx->scene;
  LumMeshRefitStats& st = ctx->refit_stats;
  *rebuilt = false;
  if (restore_stale_meshes(ctx)) return 1;
  const Stopwatch t_all;
  BvhTri* d_tris = ctx->arrays.mesh.blas_tris.get();
  std::vector<float> posed_vertices;
  for (size_t j = 0; j < moved.meshes.size(); j++) {
    const uint32_t m = moved.meshes[j], t0 = v->mesh_tri_offset[m], nt = v->mesh_tri_offset[m + 1] - t0;
    const bool posed = moved.posed[j];
    MeshTreeKey key = moved.keys[j];
    const float* vertices = v->vertices + (size_t) t0 * 12;
    MeshRefit& mr = ctx->mesh_refit[m];
    bool build = ctx->refit_mode == 1;
    if (!build) {
      const Stopwatch t_refit;
      if (mr.built_cost == 0.0) mr.built_cost = bvh4_cost(ctx->mesh_bvh[m]->bvh);  // (no refit yet: the held tree is the built one)
      if (!mr.plan.nodes) {
        const hipError_t e = refit_plan_create(mr.plan, ctx->mesh_bvh[m]->bvh, nt);
        if (e == hipErrorInvalidValue) build = true;  // spatial splits: more references than triangles
        else HIP_TRY(ctx, e);
      }
      if (!build) {
        MeshTree& own = private_tree_of(ctx, m);
        Aabb box;
        double download = 0.0;
        HIP_TRY(ctx, refit_run(mr.plan, sc.vertices + 3 * (size_t) t0, d_tris + t0, nullptr, own.bvh.nodes.data(), &box, &download));
        st.seconds_download += download;
        const double growth = mr.built_cost > 0.0 ? bvh4_cost(own.bvh) / mr.built_cost : 1.0;
        st.max_cost_growth = std::max(st.max_cost_growth, growth);
        if (ctx->refit_max_cost_growth > 0.0f && growth > (double) ctx->refit_max_cost_growth) build = true;
        else { ctx->mesh_bvh[m] = mr.own; ctx->mesh_box[m] = box; mesh_boxes_changed(ctx); st.refits++; st.last_refits++; }
      }
      st.seconds_refit += t_refit.seconds();
    }
    if (build) {
      const Stopwatch t_build;
      if (posed) {  // the builder reads host vertices: the posed ones come down (the view's layout), and with them the key of the process's tree cache
        if (download_posed_vertices(ctx, m, t0, nt, posed_vertices)) return 1;
        vertices = posed_vertices.data();
        key = mesh_tree_key(vertices, nt, ctx->bvh_builder);
      }
      std::vector<Aabb> tri_boxes(nt);
      ctx->mesh_box[m] = mesh_triangle_boxes(vertices, nt, tri_boxes.data());
      mesh_boxes_changed(ctx);
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
      st.seconds_rebuild += t_build.seconds();
    }
    mr.fit_to_pose = posed;
    mr.fit_hash[0] = posed ? 0 : key.h0; mr.fit_hash[1] = posed ? 0 : key.h1;
  }
  st.seconds = moved.seconds + t_all.seconds();
  return 0;
}

// Top level + every mesh's tree in ONE node array (bvh_build.cpp assemble_scene_tree), of the instances' part; the traversal triangles are of the meshes'.
static int update_scene_tree(LumContext* ctx, const LumDeviceSceneView* v, bool dirty_meshes, size_t* num_nodes) {
  DeviceScene& sc = ctx->scene;
  std::vector<BvhTri> blas_tris;
  if (!dirty_meshes && restore_stale_meshes(ctx)) return 1;  // (new meshes: build_mesh_trees replaces every tree and mark)
  if (dirty_meshes && build_mesh_trees(ctx, v, blas_tris)) return 1;
  if (ctx->mesh_box.size() != v->num_meshes || ctx->mesh_bvh.size() != v->num_meshes) { ctx->error = "lumc_scene_update: the meshes changed but LUMC_DIRTY_MESHES is not set"; return 1; }
  std::vector<const Bvh4*> mesh_bvh(v->num_meshes);
  for (uint32_t m = 0; m < v->num_meshes; m++) mesh_bvh[m] = &ctx->mesh_bvh[m]->bvh;
  const SceneTree tree = assemble_scene_tree(*v, mesh_bvh.data(), ctx->mesh_box.data());
  if (tree.nodes.empty()) { ctx->error = "top-level BVH exceeds 16 levels"; return 1; }
  if (scene_too_large(ctx, v, tree.nodes.size())) return 1;
  // by instance id: the exact flavour's ambient reuse re-tests a ray against a hit's triangle (k_resolve_reuse)
  if (upload(ctx, ctx->arrays.inst.rows, tree.inv_rows.data(), tree.inv_rows.size(), &sc.instance_rows)) return 1;
  ctx->instance_update.resident = false;  // the one place: the node array in assemble_scene_tree's order, not relayout_resident's
  ctx->resident_refit.drop_layout();      // ... and with the layout the slot lists of the refits in it
  if (upload(ctx, ctx->arrays.inst.nodes, tree.nodes.data(), tree.nodes.size(), &sc.bvh_nodes)) return 1;
  if (dirty_meshes && upload(ctx, ctx->arrays.mesh.blas_tris, blas_tris.data(), blas_tris.size(), &sc.blas_tris)) return 1;
  if (upload(ctx, ctx->arrays.inst.tlas_leaves, tree.tlas_leaves.data(), tree.tlas_leaves.size(), &sc.tlas_leaves)) return 1;
  sc.tlas_num_nodes = tree.tlas_num_nodes;
  sc.tlas_num_leaves = (uint32_t) (tree.tlas_leaves.size() / 4);  // records that exist (one of padding included): what a workgroup may stage in LDS
  {  // does leaf record 0 map a ray onto itself (rows of 1 and +-0, no translation)? What the fast flavour's single-level form asks for (context.h single_level_allowed)
    bool identity = tree.tlas_leaves.size() >= 4;
    for (int k = 0; k < 3 && identity; k++) {
      const float4 r = tree.tlas_leaves[k];
      const float row[4] = {r.x, r.y, r.z, r.w};
      for (int c = 0; c < 4; c++) identity = identity && row[c] == (c == k ? 1.0f : 0.0f);
    }
    ctx->first_leaf_identity = identity;
  }
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

// ---- LUMC_DIRTY_INSTANCE_TRANSFORMS (lum_core.h lumc_set_instance_update; instance_update.hip) ----
// The resident layout: the node array laid out once on the host so that the top level has a range of its own, [0, C), and the mesh trees, [C, C + M), need not
// be written again; the leaf records get room for every instance. Replaces both arrays of the instances' part; costs what an instance edit costs.
static int relayout_resident(LumContext* ctx, const LumDeviceSceneView* v) {
  DeviceScene& sc = ctx->scene;
  InstanceUpdate& u = ctx->instance_update;
  SceneArrays::Inst& a = ctx->arrays.inst;
  const uint32_t n = v->num_instances, capacity = std::max<uint32_t>(1u, n > 0 ? n - 1u : 0u);
  if (restore_stale_meshes(ctx)) return 1;
  ResidentRefit& rr = ctx->resident_refit;
  rr.drop_layout();
  std::vector<const Bvh4*> mesh_bvh(v->num_meshes);
  for (uint32_t m = 0; m < v->num_meshes; m++) mesh_bvh[m] = &ctx->mesh_bvh[m]->bvh;
  std::vector<Bvh4Node> nodes;
  std::vector<uint32_t> mesh_root;
  layout_resident_nodes(*v, mesh_bvh.data(), capacity, nodes, mesh_root, ctx->refit_in_place ? &rr.mesh_slots : nullptr);
  if (scene_too_large(ctx, v, nodes.size())) return 1;
  a.nodes.reset(); a.tlas_leaves.reset(); point_views(sc, a);
  if (upload(ctx, a.nodes, nodes.data(), nodes.size(), &sc.bvh_nodes)) return 1;
  HIP_TRY(ctx, a.tlas_leaves.resize(4 * ((size_t) n + 1)));
  sc.tlas_leaves = a.tlas_leaves.get();
  HIP_TRY(ctx, hipMemset(a.tlas_leaves.get(), 0, sizeof(float4) * 4 * ((size_t) n + 1)));
  HIP_TRY(ctx, u.mesh_root.assign(mesh_root.data(), v->num_meshes));
  u.capacity = capacity; u.mesh_nodes = (uint32_t) (nodes.size() - capacity); u.tlas_nodes = 0;
  rr.capacity = u.capacity; rr.mesh_nodes = u.mesh_nodes;
  if (update_ray_kernel_lds(ctx, nodes.size())) return 1;
  u.resident = true;
  return 0;
}

// One update of the top level on the device, in three steps: the instances' boxes from the transforms in the array that is there, the resident layout if there is
// none, then top level and leaf records built in place. The caller sets *fell_back to false first; a step that sets it says that the device path could not take
// this update (fewer than two instances that can be hit, a top level deeper than 16, a failed allocation): nothing the scene points at is left half written that
// the host path, which the caller runs then, does not replace.
struct InstanceBoxes {
  uint32_t hittable = 0;  // instances that can be hit
  Aabb world;             // their bounds
  Stopwatch since_start;  // LumInstanceUpdateStats::seconds runs from here
};

// Step 1, which starts the update's timers: the moved instances' scratch, the transforms (upload_transforms = false: those on the device are the update's - they
// did not move, or an earlier step of this update uploaded them), then rows and boxes derived from them.
static int instance_boxes(LumContext* ctx, const LumDeviceSceneView* v, bool upload_transforms, InstanceBoxes* out, bool* fell_back) {
  DeviceScene& sc = ctx->scene;
  InstanceUpdate& u = ctx->instance_update;
  SceneArrays::Inst& a = ctx->arrays.inst;
  LumInstanceUpdateStats& st = ctx->instance_stats;
  reset_update(st);
  const uint32_t n = v->num_instances;
  if (n != sc.num_instances || ctx->instance_mesh_ids.size() != n || ctx->mesh_bvh.size() != v->num_meshes || ctx->mesh_box.size() != v->num_meshes ||
      (n && std::memcmp(ctx->instance_mesh_ids.data(), v->instance_mesh_ids, sizeof(uint32_t) * n) != 0)) {
    ctx->error = "lumc_scene_update: LUMC_DIRTY_INSTANCE_TRANSFORMS with another instance count or other mesh ids than the scene on the device";
    return 1;
  }
  out->since_start = Stopwatch{};
  if (!u.prepared || u.num_instances != n || u.num_meshes != v->num_meshes) {  // (whoever writes ctx->mesh_box drops `prepared`: mesh_boxes_changed)
    u.reset();
    if (instance_update_prepare(u, n, v->num_meshes, ctx->mesh_box.data()) != hipSuccess) { (void) hipGetLastError(); u.reset(); *fell_back = true; return 0; }
  }
  Stopwatch t;
  if (n && upload_transforms) HIP_TRY(ctx, hipMemcpy(a.transforms.get(), v->instance_transforms, sizeof(float4) * 2 * (size_t) n, hipMemcpyHostToDevice));
  HIP_TRY(ctx, hipDeviceSynchronize());
  st.seconds_upload = t.seconds();
  t = Stopwatch{};
  HIP_TRY(ctx, instance_update_boxes(u, sc.instance_transforms, sc.instance_mesh_ids, sc.mesh_tri_offset, a.rows.get(), &out->hittable, &out->world));
  st.seconds_boxes = t.seconds();
  if (out->hittable < 2) *fell_back = true;  // (before the layout: a scene of one instance never pays for one)
  return 0;
}

// Step 2: the resident layout exists.
static int ensure_resident_layout(LumContext* ctx, const LumDeviceSceneView* v, bool* fell_back) {
  if (ctx->instance_update.resident) return 0;
  const Stopwatch t;
  if (relayout_resident(ctx, v)) { (void) hipGetLastError(); ctx->error.clear(); *fell_back = true; return 0; }  // (the host path replaces whatever this left, or fails for the same reason)
  HIP_TRY(ctx, hipDeviceSynchronize());
  ctx->instance_stats.relayouts++;
  ctx->instance_stats.seconds_relayout = t.seconds();
  return 0;
}

// Step 3: the top level over the boxes into [0, C) of the node array, the leaf records, the scene's counts.
static int build_top_level(LumContext* ctx, const InstanceBoxes& boxes, bool* fell_back) {
  DeviceScene& sc = ctx->scene;
  InstanceUpdate& u = ctx->instance_update;
  SceneArrays::Inst& a = ctx->arrays.inst;
  LumInstanceUpdateStats& st = ctx->instance_stats;
  const uint32_t hittable = boxes.hittable;
  Stopwatch t;
  uint32_t num_nodes = 0, depth = 0;
  Bvh4Node* d_nodes = a.nodes.get();  // (after the layout, which replaces the array)
  if (!build_bvh4_sah_device(u.dense_boxes.get(), hittable, 1, 16, d_nodes, u.capacity, u.prims.get(), &num_nodes, &depth)) {
    (void) hipGetLastError();
    *fell_back = true;
    return 0;
  }
  st.seconds_build = t.seconds();
  t = Stopwatch{};
  HIP_TRY(ctx, instance_update_leaves(u, hittable, sc.instance_rows, sc.instance_mesh_ids, a.tlas_leaves.get(), d_nodes, num_nodes, std::max(num_nodes, u.tlas_nodes)));
  HIP_TRY(ctx, hipDeviceSynchronize());
  st.seconds_leaves = t.seconds();
  u.tlas_nodes = num_nodes;
  sc.tlas_num_nodes = num_nodes;
  sc.tlas_num_leaves = hittable + 1u;  // (one of padding)
  ctx->first_leaf_identity = false;    // (two instances or more: never asked)
  std::memcpy(ctx->sort.world_lo, boxes.world.lo, sizeof(ctx->sort.world_lo)); std::memcpy(ctx->sort.world_hi, boxes.world.hi, sizeof(ctx->sort.world_hi));
  ctx->bvh_stats[0] = u.mesh_nodes;
  ctx->bvh_stats[2] = num_nodes;
  st.device_updates++;
  st.tlas_nodes = num_nodes; st.tlas_depth = depth; st.tlas_capacity = u.capacity; st.hittable = hittable;
  st.seconds = boxes.since_start.seconds();
  return 0;
}

// ---- moved vertices where the nodes live (lum_core.h lumc_set_mesh_refit_in_place; bvh_refit.hip) ----
// The mesh part of such an update, for the meshes find_moved_meshes found: in the resident layout, laid out first if there is none (steps 1 and 2 above), their
// triangle boxes, their node boxes in [C, C + M), their root boxes into the moved instances' scratch and their costs. No node leaves or enters the device; the
// host's copies of the moved meshes' nodes become stale (restore_stale_meshes). The top level follows in scene_update (steps 1 and 3).
// *fell_back: this update takes refit_mesh_copies' path instead (a moved mesh that cannot be refitted, fewer than two instances that can be hit, a failed
// allocation or layout, a cost growth beyond the threshold); the context is consistent: nothing was written, or what was written in place is marked stale.
static int refit_in_place(LumContext* ctx, const LumDeviceSceneView* v, const MovedMeshes& moved, bool* fell_back) {
  DeviceScene& sc = ctx->scene;
  InstanceUpdate& u = ctx->instance_update;
  ResidentRefit& rr = ctx->resident_refit;
  LumMeshRefitStats& st = ctx->refit_stats;
  LumResidentRefitStats& rs = ctx->resident_stats;
  reset_update(rs);
  rs.seconds_upload = st.seconds_upload; rs.seconds_hash = st.seconds_hash;
  *fell_back = false;
  if (!moved.refittable) { *fell_back = true; return 0; }  // spatial splits: the other path builds that mesh
  const Stopwatch t;
  // the layout, and the moved instances' scratch with the meshes' boxes in it
  if (!u.resident || !u.prepared || u.num_instances != v->num_instances || u.num_meshes != v->num_meshes || rr.mesh_slots.size() != v->num_meshes) {
    if (u.resident && rr.mesh_slots.size() != v->num_meshes) {  // laid out while the switch was off: once more, for the slot map
      if (restore_stale_meshes(ctx)) return 1;
      u.resident = false;
    }
    InstanceBoxes boxes;
    if (instance_boxes(ctx, v, true, &boxes, fell_back)) return 1;
    if (!*fell_back && ensure_resident_layout(ctx, v, fell_back)) return 1;
    if (*fell_back) return 0;
    if (!u.resident || !u.prepared || rr.mesh_slots.size() != v->num_meshes) { *fell_back = true; return 0; }
  }
  if (moved.meshes.empty()) { rs.seconds = st.seconds = moved.seconds + t.seconds(); return 0; }  // (nothing to refit: the top level alone)
  // everything that can fail, before a node is written
  if (rr.mesh.size() != v->num_meshes) { rr.mesh.clear(); rr.mesh.resize(v->num_meshes); rr.batch.clear(); }
  for (uint32_t m : moved.meshes) {
    MeshRefit& mr = ctx->mesh_refit[m];
    if (mr.built_cost == 0.0) mr.built_cost = bvh4_cost(ctx->mesh_bvh[m]->bvh);  // (no refit yet: the held tree is the built one, and not stale)
    if (rr.mesh[m].slots) continue;
    const hipError_t e = resident_mesh_create(rr.mesh[m], ctx->mesh_bvh[m]->bvh, v->mesh_tri_offset[m + 1] - v->mesh_tri_offset[m], rr.mesh_slots[m]);
    if (e != hipSuccess) { (void) hipGetLastError(); *fell_back = true; return 0; }
  }
  if (resident_refit_prepare(rr, moved.meshes, v->mesh_tri_offset, u.mesh_nodes) != hipSuccess) { (void) hipGetLastError(); *fell_back = true; return 0; }
  // the refit
  std::vector<ResidentResult> results(moved.meshes.size());
  uint32_t launches = 0;
  double seconds[2] = {0.0, 0.0};
  HIP_TRY(ctx, resident_refit_run(rr, sc.vertices, ctx->arrays.mesh.blas_tris.get(), ctx->arrays.inst.nodes.get(), u.capacity, u.mesh_nodes, u.mesh_box.get(), u.num_meshes, results.data(), &launches, seconds));
  for (uint32_t m : moved.meshes) if (!ctx->mesh_refit[m].stale) { ctx->mesh_refit[m].stale = true; ctx->stale_meshes++; }  // from here on the device's nodes are ahead of the host's
  rs.seconds_cost = seconds[1];
  rs.seconds_refit = t.seconds() - seconds[1];
  double max_growth = 0.0;
  bool grown = false;
  for (size_t j = 0; j < moved.meshes.size(); j++) {
    const MeshRefit& mr = ctx->mesh_refit[moved.meshes[j]];
    const double growth = mr.built_cost > 0.0 ? results[j].cost / mr.built_cost : 1.0;
    max_growth = std::max(max_growth, growth);
    if (ctx->refit_max_cost_growth > 0.0f && growth > (double) ctx->refit_max_cost_growth) grown = true;
  }
  if (grown) {  // the other path refits from the restored nodes, measures the same growth and builds the mesh again; it writes ctx->mesh_box and drops `prepared`
    *fell_back = true;
    return 0;
  }
  for (size_t j = 0; j < moved.meshes.size(); j++) {
    MeshRefit& mr = ctx->mesh_refit[moved.meshes[j]];
    ctx->mesh_box[moved.meshes[j]] = results[j].box;  // (u.mesh_box on the device holds it already: `prepared` stays)
    mr.fit_to_pose = moved.posed[j];
    mr.fit_hash[0] = moved.keys[j].h0; mr.fit_hash[1] = moved.keys[j].h1;  // (zeros for a posed mesh)
    st.refits++; st.last_refits++;
  }
  st.max_cost_growth = max_growth;
  st.seconds_refit = rs.seconds_refit + rs.seconds_cost;
  rs.last_meshes = (uint32_t) moved.meshes.size(); rs.last_launches = launches;
  rs.last_bytes_downloaded = sizeof(ResidentResult) * moved.meshes.size();
  rs.seconds = st.seconds = moved.seconds + t.seconds();
  return 0;
}

// Light-only BVH (world-space triangles; reference: optix_bvh.c:382-478), of the lights' part.
static int update_light_bvh(LumContext* ctx, const LumDeviceSceneView* v) {
  DeviceScene& sc = ctx->scene;
  const uint32_t nl = (v->light_tree_root && v->light_bvh_tris) ? v->num_lights : 0;
  std::vector<Aabb> boxes(nl);
  for (uint32_t l = 0; l < nl; l++) { const float* p = v->light_bvh_tris + (size_t) l * 12; boxes[l] = tri_box(p, p + 4, p + 8); }
  Bvh4 lb = build_bvh4(boxes.data(), nl, kBvhLeafMaxTri, 40);
  if (lb.nodes.empty()) { ctx->error = "light BVH exceeds 40 levels"; return 1; }
  std::vector<BvhTri> tris(nl ? nl : 1, BvhTri{});
  for (uint32_t i = 0; i < nl; i++) tris[i] = bvh_tri(v->light_bvh_tris + (size_t) lb.prims[i] * 12, lb.prims[i], 0u, 0u);
  if (upload(ctx, ctx->arrays.lights.bvh_nodes, lb.nodes.data(), lb.nodes.size(), &sc.light_nodes)) return 1;
  if (upload(ctx, ctx->arrays.lights.bvh_tris, tris.data(), tris.size(), &sc.light_tris)) return 1;
  sc.light_num_nodes = (uint32_t) lb.nodes.size();
  ctx->bvh_stats[3] = lb.nodes.size();
  ctx->light_bvh = std::move(lb);  // what lumc_light_refit_bind makes the refit's topology from
  return 0;
}

// The bound light tree from the vertices as they now stand on the device (LUMC_DIRTY_LIGHT_POSITIONS; light_refit.hip): fragments and slot statistics into scratch,
// then - only once the flag word has come back clean and the cost is within the bound - the statistics' bytes of the root, its float table and the nodes in place,
// and the light BVH refitted from the lights' world-space triangles into the resident arrays. update_counts_and_tables, which follows, runs k_light_table. A
// fallback (no binding, a flag, the cost) touches nothing of the lights' part and is reported (lumc_light_refit_needs_rebuild); the view's light arrays are not read.
static int refit_lights(LumContext* ctx, const LumDeviceSceneView* v) {
  LightRefit& r = ctx->light_refit;
  LumLightRefitStats& st = ctx->light_refit_stats;
  DeviceScene& sc = ctx->scene;
  SceneArrays::Lights& a = ctx->arrays.lights;
  st.last_launches = st.last_flags = 0; st.last_bytes_uploaded = st.last_bytes_downloaded = 0;
  st.seconds = st.seconds_fragments = st.seconds_stats = st.seconds_nodes = st.seconds_light_bvh = st.seconds_table = st.cost_growth = 0.0;
  auto fall_back = [&]() { st.fallbacks++; ctx->light_refit_needs_rebuild = true; return 0; };
  if (!r.bound || r.num_fragments != sc.num_lights || !a.tree_root || !a.root_children || !a.bvh_nodes || !a.bvh_tris || a.bvh_tris.count() < r.num_fragments ||
      a.bvh_nodes.count() != r.bvh.num_nodes || a.tree_nodes.count() != 4 * (size_t) r.num_nodes || a.tree_root.count() != 1 + 3 * (size_t) r.sections ||
      a.root_children.count() != (size_t) r.sections * 64 + 16 || ctx->mesh_tri_offset.size() != (size_t) v->num_meshes + 1)
    return fall_back();
  // the per-part seconds cost a synchronisation each: only on request (LUM_LIGHT_REFIT_TIMING=1; tools/light_refit_bench.py). Otherwise the refit waits once, for the flag word.
  static const bool timed = [] { const char* e = getenv("LUM_LIGHT_REFIT_TIMING"); return e && atoi(e) != 0; }();
  const Stopwatch t_all;
  if (!r.pending.empty()) {
    HIP_TRY(ctx, hipMemcpy(r.transforms.get(), r.pending.data(), sizeof(LumLightTransform) * r.pending.size(), hipMemcpyHostToDevice));
    st.last_bytes_uploaded = sizeof(LumLightTransform) * r.pending.size();
    r.pending.clear();
  }
  const size_t corners = ctx->arrays.mesh.vertices.count();
  if (corners > 0xFFFFFFFFull) return fall_back();
  HIP_TRY(ctx, light_refit_fragments(r, ctx->arrays.mesh.vertices.get(), ctx->arrays.mesh.tri_offset.get(), v->num_meshes, (uint32_t) corners));
  if (timed) { HIP_TRY(ctx, hipDeviceSynchronize()); st.seconds_fragments = t_all.seconds(); }
  const Stopwatch t_stats;
  HIP_TRY(ctx, light_refit_stats(r));
  st.last_launches = 2;
  uint32_t flags = 0;
  float result[2 * kLightRootSlots];
  HIP_TRY(ctx, hipMemcpy(&flags, r.flags.get(), sizeof(flags), hipMemcpyDeviceToHost));  // (waits for the launches)
  HIP_TRY(ctx, hipMemcpy(result, r.result.get(), sizeof(result), hipMemcpyDeviceToHost));
  st.last_bytes_downloaded = sizeof(flags) + sizeof(result);
  if (timed) st.seconds_stats = t_stats.seconds();
  st.last_flags = flags;
  if (flags & kLightRefitFlagBadPlan) { ctx->error = "lumc_scene_update: an index of the light refit plan beyond the scene reached a kernel"; return 1; }
  double cost = 0.0;
  for (uint32_t c = 0; c < 8 * r.sections; c++) cost += (double) result[2 * c] * (double) result[2 * c + 1];
  st.cost_growth = r.root_cost > 0.0 ? cost / r.root_cost : 0.0;
  if (flags || (ctx->light_refit_max_cost_growth > 0.0f && st.cost_growth > (double) ctx->light_refit_max_cost_growth)) { st.seconds = t_all.seconds(); return fall_back(); }
  const Stopwatch t_nodes;
  HIP_TRY(ctx, light_refit_nodes(r, (uint8_t*) a.tree_root.get(), a.root_children.get(), (uint8_t*) a.tree_nodes.get()));
  st.last_launches++;
  if (timed) { HIP_TRY(ctx, hipDeviceSynchronize()); st.seconds_nodes = t_nodes.seconds(); }
  const Stopwatch t_bvh;
  Aabb root_box;
  HIP_TRY(ctx, refit_run(r.bvh, r.tris.get(), a.bvh_tris.get(), nullptr, a.bvh_nodes.get(), &root_box));
  st.last_launches += 1 + (uint32_t) r.bvh.level_first.size() - 1;
  st.last_bytes_downloaded += sizeof(Aabb);
  if (timed) st.seconds_light_bvh = t_bvh.seconds();
  st.seconds = t_all.seconds();
  st.refits++;
  ctx->lights_refitted = true;
  ctx->light_refit_needs_rebuild = false;
  return 0;
}

// DeviceScene::traits (dev_scene.h SceneTrait; plain_scene, wavefront_table.h) from the host's words of the materials, the light tree and the lights' triangles:
// nothing is read back. Called by every update after its parts have run, so an edited material, new lights or new meshes under the lights are seen; a light
// refit keeps the tree's topology and the lights' triangles, a flat tree stays flat across it.
static uint32_t scene_traits(const LumContext* ctx) {
  uint32_t traits = kTraitNoTranslucent | kTraitPlainEmitters;
  const size_t num_materials = ctx->material_words.size() / 16;
  for (size_t m = 0; m < num_materials; m++)
    if ((ctx->material_words[16 * m] & exact::kDMatSubstrateMask) != 0) traits &= ~(uint32_t) kTraitNoTranslucent;
  if (ctx->light_tree_flat) traits |= kTraitFlatLightTree;
  for (size_t l = 0; l < ctx->light_handles.size() / 2; l++) {  // the material k_light_table finds for the light: handle -> mesh -> scene triangle -> material id
    const uint32_t inst = ctx->light_handles[2 * l], tri = ctx->light_handles[2 * l + 1];
    bool plain = false;
    if (inst < ctx->instance_mesh_ids.size() && (size_t) ctx->instance_mesh_ids[inst] + 1 < ctx->mesh_tri_offset.size()) {
      const size_t scene_tri = (size_t) ctx->mesh_tri_offset[ctx->instance_mesh_ids[inst]] + tri;
      if (scene_tri < ctx->tri_material.size() && ctx->tri_material[scene_tri] < num_materials) {
        const uint16_t* w = &ctx->material_words[16 * (size_t) ctx->tri_material[scene_tri]];
        plain = w[12] == exact::kTextureNone && w[13] == exact::kTextureNone;  // albedo and emission texture (dev_bsdf.h load_material: b.z)
      }
    }
    if (!plain) traits &= ~(uint32_t) kTraitPlainEmitters;
  }
  return traits;
}

// The counts, then what two kernels derive from the arrays above: k_tri_opacity (needs the materials and blas_tris), k_light_table (needs the counts).
// triangles_rewritten: a moved-vertices update built a mesh again, its traversal triangles are new.
// keep_light_count: the caller said LUMC_DIRTY_LIGHT_POSITIONS without new lights - the view's light arrays and their count are not read, the device's stay.
static int update_counts_and_tables(LumContext* ctx, const LumDeviceSceneView* v, const UpdatePlan& plan, bool triangles_rewritten, bool keep_light_count) {
  DeviceScene& sc = ctx->scene;
  const uint32_t total_tris = total_triangles(v);
  const bool dirty_lights = plan.lights;
  const bool lights_refitted = ctx->lights_refitted;
  ctx->lights_refitted = false;
  ctx->bvh_stats[1] = total_tris;
  sc.num_meshes = v->num_meshes; sc.num_instances = v->num_instances; sc.num_materials = v->num_materials;  // (num_textures: update_textures)
  if (!keep_light_count) sc.num_lights = v->num_lights;
  if (total_tris && plan.tri_opacity(triangles_rewritten)) {  // the triangles' material words: texture id, or whether they stop a visibility ray on their own
    hipLaunchKernelGGL(k_tri_opacity, dim3((total_tris + kBlock - 1) / kBlock), dim3(kBlock), 0, 0, sc, ctx->arrays.mesh.blas_tris.get(), total_tris);
    HIP_TRY(ctx, hipGetLastError());
  }
  const bool lights_left_alone = keep_light_count && !lights_refitted;  // a refit that fell back: the table stays with the tree it belongs to until the caller's rebuild
  if (!lights_left_alone && (dirty_lights || ((plan.light_table_inputs() || lights_refitted) && sc.light_tri_table)) && sc.light_tree_root && sc.num_lights) {  // the emissive triangles in world space with what their material says, one record per light (load_tri_light_table)
    DeviceBuffer<float4>& table = ctx->arrays.lights.tri_table;  // a material edit alone refills the table in place (same lights)
    const Stopwatch t_table;
    if (dirty_lights) HIP_TRY(ctx, table.resize(4 * (size_t) sc.num_lights));
    hipLaunchKernelGGL(k_light_table, dim3((sc.num_lights + kBlock - 1) / kBlock), dim3(kBlock), 0, 0, sc, table.get());
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipDeviceSynchronize());
    sc.light_tri_table = table.get();
    if (lights_refitted) { ctx->light_refit_stats.last_launches++; ctx->light_refit_stats.seconds_table = t_table.seconds(); ctx->light_refit_stats.seconds += t_table.seconds(); }
  }
  return 0;
}

// The scalar fields of the constants' part.
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
  sc.sky_stars_count = 0; sc.sky_hdri_dim = 0;
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
  if (upload(ctx, ctx->arrays.constants.stars, (const float4*) v->sky_stars, (size_t) v->sky_stars_count, &sc.sky_stars)) return 1;
  if (upload(ctx, ctx->arrays.constants.stars_offsets, v->sky_stars_offsets, (size_t) 64 * 32 + 1, &sc.sky_stars_offsets)) return 1;
  sc.sky_stars_count = v->sky_stars_count;
  return 0;
}

// The clouds' noise textures: the caller's three, or the context's own (ensure_cloud_noise).
static int update_cloud_noise(LumContext* ctx, const LumDeviceSceneView* v) {
  DeviceScene& sc = ctx->scene;
  if (!sc.cloud_active) return 0;
  if (v->cloud_noise_shape && v->cloud_noise_detail && v->cloud_noise_weather) {
    DeviceBuffer<uint32_t>* a = ctx->arrays.constants.cloud_noise;
    if (upload(ctx, a[0], (const uint32_t*) v->cloud_noise_shape, kCloudNoiseTexels[0], &sc.cloud_noise_shape)) return 1;
    if (upload(ctx, a[1], (const uint32_t*) v->cloud_noise_detail, kCloudNoiseTexels[1], &sc.cloud_noise_detail)) return 1;
    return upload(ctx, a[2], (const uint32_t*) v->cloud_noise_weather, kCloudNoiseTexels[2], &sc.cloud_noise_weather);
  }
  if (ensure_cloud_noise(ctx, v->cloud_seed)) return 1;
  sc.cloud_noise_shape = ctx->d_cloud_noise[0].get(); sc.cloud_noise_detail = ctx->d_cloud_noise[1].get(); sc.cloud_noise_weather = ctx->d_cloud_noise[2].get();
  return 0;
}

// Sky look-up tables: the caller's or generated here (device/device_sky.c:64-200); not for a constant sky (HDRI mode bakes from them and samples the sun through them).
static int update_sky_tables(LumContext* ctx, const LumDeviceSceneView* v) {
  DeviceScene& sc = ctx->scene;
  if (sc.sky_mode == kSkyConstantColor) return 0;
  const size_t tm_texels = 2 * (size_t) kSkyTmWidth * kSkyTmHeight, ms_texels = 2 * (size_t) kSkyMsSize * kSkyMsSize;
  if (v->sky_lut_transmittance && v->sky_lut_multiscattering) {
    if (upload(ctx, ctx->arrays.constants.sky_lut[0], (const float4*) v->sky_lut_transmittance, tm_texels, &sc.sky_lut_transmittance)) return 1;
    if (upload(ctx, ctx->arrays.constants.sky_lut[1], (const float4*) v->sky_lut_multiscattering, ms_texels, &sc.sky_lut_multiscattering)) return 1;
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
    if (upload(ctx, ctx->arrays.constants.sky_hdri, (const float4*) v->sky_hdri, (size_t) v->sky_hdri_dim * v->sky_hdri_dim, &sc.sky_hdri)) return 1;
    sc.sky_hdri_dim = v->sky_hdri_dim;
    return 0;
  }
  ctx->has_scene = true;  // the bake renders this scene's sky
  if (lumc_sky_hdri_build(ctx, v->sky_hdri_origin, v->sky_hdri_dim, v->sky_hdri_samples ? v->sky_hdri_samples : 1u)) { ctx->has_scene = false; return 1; }
  return 0;
}

// Camera, settings, sky, fog, ocean, clouds, particles: the kernels' scalar arguments and the tables derived from them.
static int update_constants(LumContext* ctx, const LumDeviceSceneView* v, const UpdatePlan& plan) {
  ctx->arrays.constants = {}; point_views(ctx->scene, ctx->arrays.constants);
  if (copy_constants(ctx, v)) return 1;
  if (update_stars(ctx, v)) return 1;
  if (update_cloud_noise(ctx, v)) return 1;
  if (plan.particles && build_particle_tree(ctx, v, ctx->scene)) return 1;
  if (update_sky_tables(ctx, v)) return 1;
  if (update_bsdf_tables(ctx, v, plan.full_upload)) return 1;
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

// The scene on the device: the plan of this update (update_plan.h), then its parts in the order their kernels and uploads depend on. Until the update has gone
// through the context has no scene.
static int scene_update(LumContext* ctx, const LumDeviceSceneView* v, unsigned dirty) {
  ctx->drop_first_hit_products("the scene was uploaded or updated since");  // the denoiser's guides and the mattes were rendered from the scene as it was
  DeviceScene& sc = ctx->scene;
  if (!v->bluenoise_2d) { ctx->error = "scene has no blue-noise mask"; return 1; }
  if (v->max_ray_depth > 63) { ctx->error = "max_ray_depth exceeds 63 (6-bit field, device_structs.h:9)"; return 1; }
  bool pose_pending = false;
  for (const auto& kv : ctx->mesh_deform) pose_pending = pose_pending || kv.second.pending();  // pending weights are a pending pose
  bool shutter_pending = false;
  for (const auto& kv : ctx->mesh_shutter) shutter_pending = shutter_pending || (kv.second.both() && kv.second.pending);
  UpdatePlan plan = plan_update(dirty, ctx->refit_in_place != 0, ctx->refit_mode, ctx->instance_update_mode, pose_pending, ctx->light_refit.bound, shutter_pending);
  if (plan.moved_by_host) reset_update(ctx->instance_stats);
  auto host_path_since = [&](const Stopwatch& t) { if (plan.moved_by_host) ctx->instance_stats.seconds += t.seconds(); };
  auto lights_since = [&](const Stopwatch& t) { if (plan.time_lights) ctx->refit_stats.seconds_lights += t.seconds(); };
  ctx->has_scene = false;
  ctx->lights_refitted = false;
  if (plan.lights || plan.meshes) { ctx->light_refit.reset(); ctx->light_refit_needs_rebuild = false; }  // new lights: the plan's topology is not theirs, the caller binds again
  if (plan.meshes) { ctx->arrays.mesh = {}; ctx->mesh_deform.clear(); ctx->mesh_shutter.clear(); }  // the traversal triangles too; new meshes: the bindings go, the caller binds again
  if (plan.meshes && update_mesh_arrays(ctx, v)) return 1;
  bool triangles_rewritten = false;
  if (plan.positions) {
    MovedMeshes moved;
    if (find_moved_meshes(ctx, v, plan.upload_view, (dirty & LUMC_DIRTY_MESH_SHUTTER) != 0, &moved)) return 1;
    if (plan.in_place) {
      bool fell_back = false;
      if (refit_in_place(ctx, v, moved, &fell_back)) return 1;
      if (fell_back) { ctx->resident_stats.fallbacks++; plan.take_copies_path(); }
    }
    if (!plan.in_place && refit_mesh_copies(ctx, v, moved, &triangles_rewritten)) return 1;
  }
  const Stopwatch t_arrays;
  if (plan.instances && update_instance_arrays(ctx, v)) return 1;
  host_path_since(t_arrays);
  if (plan.materials && update_materials(ctx, v)) return 1;
  Stopwatch t_lights;
  if (plan.lights && update_light_tree(ctx, v)) return 1;
  lights_since(t_lights);
  if (!sc.bluenoise_2d && upload(ctx, ctx->arrays.bluenoise_2d, v->bluenoise_2d, 65536, &sc.bluenoise_2d)) return 1;
  if (plan.textures && update_textures(ctx, v)) return 1;
  size_t num_nodes = 0;
  const Stopwatch t_assemble;
  if (plan.instances && (update_scene_tree(ctx, v, plan.meshes, &num_nodes) || update_ray_kernel_lds(ctx, num_nodes))) return 1;
  if (plan.moved_by_host) { HIP_TRY(ctx, hipDeviceSynchronize()); host_path_since(t_assemble); }
  if (plan.transforms_on_device) {
    bool fell_back = false;
    InstanceBoxes boxes;
    if (instance_boxes(ctx, v, plan.instances_moved || !plan.in_place, &boxes, &fell_back)) return 1;  // (in place: the transforms are on the device unless they moved)
    if (!fell_back && ensure_resident_layout(ctx, v, &fell_back)) return 1;
    if (!fell_back && build_top_level(ctx, boxes, &fell_back)) return 1;
    if (fell_back) {  // this one update by the host's path, as LUMC_DIRTY_INSTANCES
      if (update_instance_arrays(ctx, v) || update_scene_tree(ctx, v, false, &num_nodes) || update_ray_kernel_lds(ctx, num_nodes)) return 1;  // (update_scene_tree brings meshes refitted in place back to the host first)
      ctx->instance_stats.fallbacks++;
      ctx->instance_stats.seconds = t_assemble.seconds();
    }
    if (plan.in_place) {
      LumResidentRefitStats& rs = ctx->resident_stats;
      if (fell_back) rs.fallbacks++; else rs.updates++;
      rs.seconds_top_level = t_assemble.seconds();
      rs.seconds += rs.seconds_top_level;
      rs.last_bytes_downloaded += 28;  // instance_update_boxes: the bounds and the count
    }
  }
  if (plan.positions) ctx->refit_stats.seconds_assemble = t_assemble.seconds();
  t_lights = Stopwatch{};
  if (plan.lights && update_light_bvh(ctx, v)) return 1;
  if (plan.light_positions && refit_lights(ctx, v)) return 1;
  if ((dirty & LUMC_DIRTY_LIGHT_POSITIONS) && !plan.lights && !plan.meshes && !ctx->light_refit.bound) { ctx->light_refit_stats.fallbacks++; ctx->light_refit_needs_rebuild = true; }  // no binding: reported, nothing touched
  if (update_counts_and_tables(ctx, v, plan, triangles_rewritten, (dirty & LUMC_DIRTY_LIGHT_POSITIONS) && !plan.lights && !plan.meshes)) return 1;
  lights_since(t_lights);
  if (plan.constants && update_constants(ctx, v, plan)) return 1;
  if (update_bridge_table(ctx, v)) return 1;
  sc.traits = scene_traits(ctx);
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
  if (scene_update(ctx, v, dirty & (LUMC_DIRTY_ALL | LUMC_DIRTY_MESH_POSITIONS | LUMC_DIRTY_INSTANCE_TRANSFORMS | LUMC_DIRTY_MESH_SKIN | LUMC_DIRTY_LIGHT_POSITIONS | LUMC_DIRTY_MESH_SHUTTER))) { free_scene(ctx); return 1; }  // a failed partial update leaves no half-updated scene behind
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

int lumc_set_instance_update(LumContext* ctx, uint32_t mode) {
  if (!ctx) return 1;
  if (mode > 1) { ctx->error = "lumc_set_instance_update: mode is 0 (device) or 1 (host assembly)"; return 1; }
  ctx->instance_update_mode = mode;
  return 0;
}

int lumc_instance_update_stats(const LumContext* ctx, LumInstanceUpdateStats* out) {
  if (!ctx || !out) return 1;
  *out = ctx->instance_stats;
  return 0;
}

int lumc_set_mesh_refit_in_place(LumContext* ctx, uint32_t on) {
  if (!ctx) return 1;
  if (on > 1) { ctx->error = "lumc_set_mesh_refit_in_place: on is 0 or 1"; return 1; }
  ctx->refit_in_place = on;
  return 0;
}

int lumc_resident_refit_stats(const LumContext* ctx, LumResidentRefitStats* out) {
  if (!ctx || !out) return 1;
  *out = ctx->resident_stats;
  return 0;
}

int lumc_mesh_skin_bind(LumContext* ctx, uint32_t mesh, const float* rest_positions, const float* rest_normals, const uint16_t* bone_ids, const float* weights,
                        uint32_t triangle_count, uint32_t bone_count) {
  if (!ctx) return 1;
  if (!ctx->has_scene || (size_t) mesh + 1 >= ctx->mesh_tri_offset.size() || ctx->mesh_tri_offset[mesh + 1] - ctx->mesh_tri_offset[mesh] != triangle_count) {
    ctx->error = "lumc_mesh_skin_bind: mesh " + std::to_string(mesh) + " is not in the scene on the device with that triangle count";
    return 1;
  }
  if (!rest_positions || !rest_normals || !bone_ids || !weights) { ctx->error = "lumc_mesh_skin_bind: a NULL array"; return 1; }
  if (bone_count == 0 || bone_count > kSkinMaxBones) { ctx->error = "lumc_mesh_skin_bind: bone_count is 1 ... 1024"; return 1; }
  for (size_t i = 0; i < 12 * (size_t) triangle_count; i++) {
    if (bone_ids[i] >= bone_count) { ctx->error = "lumc_mesh_skin_bind: a bone id is not below bone_count"; return 1; }
    if (!(weights[i] >= 0.0f) || !std::isfinite(weights[i])) { ctx->error = "lumc_mesh_skin_bind: a weight is negative or not finite"; return 1; }
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  MeshSkin skin;
  HIP_TRY(ctx, mesh_skin_upload(skin, rest_positions, rest_normals, bone_ids, weights, triangle_count, bone_count));
  ctx->mesh_deform[mesh].skin = std::move(skin);  // (the morph, if any, stays)
  return 0;
}

int lumc_mesh_skin_unbind(LumContext* ctx, uint32_t mesh) {
  if (!ctx) return 1;
  const auto it = ctx->mesh_deform.find(mesh);
  if (it == ctx->mesh_deform.end() || !it->second.skin) { ctx->error = "lumc_mesh_skin_unbind: mesh " + std::to_string(mesh) + " is not bound"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  it->second.skin.reset();
  if (it->second.empty()) ctx->mesh_deform.erase(it);
  return 0;
}

int lumc_mesh_skin_pose(LumContext* ctx, uint32_t mesh, const float* bones, uint32_t bone_count) {
  if (!ctx) return 1;
  const auto it = ctx->mesh_deform.find(mesh);
  if (it == ctx->mesh_deform.end() || !it->second.skin) { ctx->error = "lumc_mesh_skin_pose: mesh " + std::to_string(mesh) + " is not bound"; return 1; }
  if (!bones || bone_count != it->second.skin->bone_count) { ctx->error = "lumc_mesh_skin_pose: mesh " + std::to_string(mesh) + " is bound to another bone count"; return 1; }
  for (size_t i = 0; i < 12 * (size_t) bone_count; i++)
    if (!std::isfinite(bones[i])) { ctx->error = "lumc_mesh_skin_pose: a matrix entry is not finite"; return 1; }
  it->second.skin->pending.assign(bones, bones + 12 * (size_t) bone_count);
  return 0;
}

int lumc_mesh_skin_stats(const LumContext* ctx, LumMeshSkinStats* out) {
  if (!ctx || !out) return 1;
  *out = ctx->skin_stats;
  return 0;
}

int lumc_mesh_morph_bind(LumContext* ctx, uint32_t mesh, const float* base_positions, const float* base_normals, uint32_t triangle_count, uint32_t target_count,
                         const uint32_t* offsets, const uint32_t* corners, const float* delta_positions, const float* delta_normals) {
  if (!ctx) return 1;
  if (!ctx->has_scene || (size_t) mesh + 1 >= ctx->mesh_tri_offset.size() || ctx->mesh_tri_offset[mesh + 1] - ctx->mesh_tri_offset[mesh] != triangle_count) {
    ctx->error = "lumc_mesh_morph_bind: mesh " + std::to_string(mesh) + " is not in the scene on the device with that triangle count";
    return 1;
  }
  if (!base_positions || !base_normals) { ctx->error = "lumc_mesh_morph_bind: a NULL array"; return 1; }
  if (const char* why = morph_check(triangle_count, target_count, offsets, corners, delta_positions, delta_normals)) { ctx->error = std::string("lumc_mesh_morph_bind: ") + why; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  MeshMorph morph;
  HIP_TRY(ctx, mesh_morph_upload(morph, base_positions, base_normals, triangle_count, target_count, offsets, corners, delta_positions, delta_normals));
  ctx->mesh_deform[mesh].morph = std::move(morph);  // (the skin, if any, stays)
  return 0;
}

int lumc_mesh_morph_unbind(LumContext* ctx, uint32_t mesh) {
  if (!ctx) return 1;
  const auto it = ctx->mesh_deform.find(mesh);
  if (it == ctx->mesh_deform.end() || !it->second.morph) { ctx->error = "lumc_mesh_morph_unbind: mesh " + std::to_string(mesh) + " is not bound"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  it->second.morph.reset();
  if (it->second.empty()) ctx->mesh_deform.erase(it);
  return 0;
}

int lumc_mesh_morph_weights(LumContext* ctx, uint32_t mesh, const float* weights, uint32_t target_count) {
  if (!ctx) return 1;
  const auto it = ctx->mesh_deform.find(mesh);
  if (it == ctx->mesh_deform.end() || !it->second.morph) { ctx->error = "lumc_mesh_morph_weights: mesh " + std::to_string(mesh) + " is not bound"; return 1; }
  if (!weights || target_count != it->second.morph->target_count) { ctx->error = "lumc_mesh_morph_weights: mesh " + std::to_string(mesh) + " is bound to another target count"; return 1; }
  for (uint32_t t = 0; t < target_count; t++)
    if (!std::isfinite(weights[t])) { ctx->error = "lumc_mesh_morph_weights: a weight is not finite"; return 1; }
  it->second.morph->pending.assign(weights, weights + target_count);
  return 0;
}

int lumc_mesh_morph_stats(const LumContext* ctx, LumMeshMorphStats* out) {
  if (!ctx || !out) return 1;
  *out = ctx->morph_stats;
  return 0;
}

int lumc_mesh_shutter_key(LumContext* ctx, uint32_t mesh, uint32_t which) {
  if (!ctx) return 1;
  if (which > 1) { ctx->error = "lumc_mesh_shutter_key: which is 0 (open) or 1 (close)"; return 1; }
  if (!ctx->has_scene || (size_t) mesh + 1 >= ctx->mesh_tri_offset.size()) { ctx->error = "lumc_mesh_shutter_key: mesh " + std::to_string(mesh) + " is not in the scene on the device"; return 1; }
  const uint32_t t0 = ctx->mesh_tri_offset[mesh], nt = ctx->mesh_tri_offset[mesh + 1] - t0;
  const size_t corners = 3 * (size_t) nt;
  if (3 * ((size_t) t0 + nt) > ctx->arrays.mesh.vertices.count()) { ctx->error = "lumc_mesh_shutter_key: the mesh lies outside the vertex array"; return 1; }
  const auto held = ctx->mesh_shutter.find(mesh);
  if (which == 1 && (held == ctx->mesh_shutter.end() || !held->second.has_open || held->second.triangles != nt)) {
    ctx->error = "lumc_mesh_shutter_key: mesh " + std::to_string(mesh) + " has no open key";
    return 1;
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipDeviceSynchronize());
  MeshShutter fresh;
  MeshShutter& s = which == 1 ? held->second : fresh;
  DeviceBuffer<float4>& plane = which == 1 ? s.close : s.open;
  if (plane.count() != corners) HIP_TRY(ctx, plane.resize(corners));
  if (corners) HIP_TRY(ctx, hipMemcpy(plane.get(), ctx->arrays.mesh.vertices.get() + 3 * (size_t) t0, sizeof(float4) * corners, hipMemcpyDeviceToDevice));
  HIP_TRY(ctx, hipDeviceSynchronize());
  if (which == 0) {  // a new open key: the close key, if any, belonged to the old one
    fresh.triangles = nt; fresh.has_open = true;
    ctx->mesh_shutter[mesh] = std::move(fresh);
  }
  else { s.has_close = true; s.t = 1.0f; s.pending = false; }  // the scene's vertices ARE the close key: written at t = 1
  return 0;
}

int lumc_mesh_shutter_drop(LumContext* ctx, uint32_t mesh) {
  if (!ctx) return 1;
  const auto it = ctx->mesh_shutter.find(mesh);
  if (it == ctx->mesh_shutter.end()) { ctx->error = "lumc_mesh_shutter_drop: mesh " + std::to_string(mesh) + " holds no key"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  ctx->mesh_shutter.erase(it);
  return 0;
}

int lumc_shutter_time(LumContext* ctx, float t) {
  if (!ctx) return 1;
  if (!std::isfinite(t) || !(t >= 0.0f) || !(t <= 1.0f)) { ctx->error = "lumc_shutter_time: t is a finite number in [0, 1]"; return 1; }
  for (auto& kv : ctx->mesh_shutter)
    if (kv.second.both()) { kv.second.t = t; kv.second.pending = true; }
  return 0;
}

int lumc_shutter_stats(const LumContext* ctx, LumShutterStats* out) {
  if (!ctx || !out) return 1;
  *out = ctx->shutter_stats;
  return 0;
}

int lumc_mesh_vertices_probe(LumContext* ctx, uint32_t mesh, void* out) {
  if (!ctx || !out) return 1;
  if (!ctx->has_scene || (size_t) mesh + 1 >= ctx->mesh_tri_offset.size()) { ctx->error = "lumc_mesh_vertices_probe: no such mesh in the scene on the device"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const uint32_t t0 = ctx->mesh_tri_offset[mesh], nt = ctx->mesh_tri_offset[mesh + 1] - t0;
  if (3 * ((size_t) t0 + nt) > ctx->arrays.mesh.vertices.count()) { ctx->error = "lumc_mesh_vertices_probe: the mesh lies outside the vertex array"; return 1; }
  if (nt) HIP_TRY(ctx, hipMemcpy(out, ctx->arrays.mesh.vertices.get() + 3 * (size_t) t0, sizeof(float4) * 3 * (size_t) nt, hipMemcpyDeviceToHost));
  return 0;
}

int lumc_set_light_refit(LumContext* ctx, float max_cost_growth) {
  if (!ctx) return 1;
  if (!(max_cost_growth >= 0.0f) || !std::isfinite(max_cost_growth)) { ctx->error = "lumc_set_light_refit: max_cost_growth >= 0"; return 1; }
  ctx->light_refit_max_cost_growth = max_cost_growth;
  return 0;
}

int lumc_light_refit_bind(LumContext* ctx, const LumLightRefitPlan* plan) {
  if (!ctx || !plan) return 1;
  ctx->light_refit.reset();
  const DeviceScene& sc = ctx->scene;
  if (!ctx->has_scene) { ctx->error = "lumc_light_refit_bind: the context has no scene"; return 1; }
  if (plan->num_fragments != sc.num_lights) { ctx->error = "lumc_light_refit_bind: the plan's fragments are not the lights of the scene on the device"; return 1; }
  if (plan->num_fragments < 2) return 0;  // no light: nothing to refit; one light: its tree is constant and not refitted - a move takes the rebuild (no binding)
  const uint32_t n = plan->num_fragments;
  const size_t num_slots = kLightRootSlots + (size_t) kLightNodeSlots * plan->num_nodes;
  const SceneArrays::Lights& a = ctx->arrays.lights;
  if (!plan->fragments || !plan->transforms || !plan->slots || plan->num_transforms == 0 || !a.tree_root || a.tree_nodes.count() != 4 * (size_t) plan->num_nodes ||
      ctx->light_bvh.nodes.empty() || ctx->light_bvh.prims.size() != n || ctx->mesh_tri_offset.empty()) {
    ctx->error = "lumc_light_refit_bind: the plan does not belong to the light tree on the device (bind right after the LUMC_DIRTY_LIGHTS update that uploaded it)";
    return 1;
  }
  const uint32_t num_meshes = (uint32_t) ctx->mesh_tri_offset.size() - 1;
  std::vector<bool> seen(n, false);
  for (uint32_t i = 0; i < n; i++) {
    const LumLightFragment& f = plan->fragments[i];
    if (f.mesh >= num_meshes || f.triangle >= ctx->mesh_tri_offset[f.mesh + 1] - ctx->mesh_tri_offset[f.mesh] || f.transform >= plan->num_transforms || f.light_id >= n ||
        seen[f.light_id] || f.instance >= sc.num_instances) {
      ctx->error = "lumc_light_refit_bind: fragment " + std::to_string(i) + " names a mesh, triangle, instance, transform or light id the scene on the device does not have";
      return 1;
    }
    seen[f.light_id] = true;
  }
  for (size_t s = 0; s < num_slots; s++)
    if (plan->slots[s].first > n || plan->slots[s].count > n - plan->slots[s].first) { ctx->error = "lumc_light_refit_bind: a slot's range lies outside the fragments"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  uint8_t header[16];
  HIP_TRY(ctx, hipMemcpy(header, a.tree_root.get(), sizeof(header), hipMemcpyDeviceToHost));
  const uint32_t sections = header[10];
  if (sections == 0 || sections > kLightRootSlots / 8 || a.tree_root.count() != 1 + 3 * (size_t) sections) { ctx->error = "lumc_light_refit_bind: the root on the device has no sections"; return 1; }
  for (uint32_t c = 8 * sections; c < kLightRootSlots; c++)
    if (plan->slots[c].count) { ctx->error = "lumc_light_refit_bind: the plan has more root children than the root on the device"; return 1; }
  LightRefit& r = ctx->light_refit;
  hipError_t e = light_refit_upload(r, *plan, sections);
  if (e == hipSuccess) e = refit_plan_create(r.bvh, ctx->light_bvh, n);
  if (e != hipSuccess) { r.reset(); ctx->error = std::string("lumc_light_refit_bind: ") + hipGetErrorString(e); return 1; }
  r.bound = true;
  return 0;
}

int lumc_light_refit_transforms(LumContext* ctx, const LumLightTransform* transforms, uint32_t num_transforms) {
  if (!ctx || !transforms) return 1;
  LightRefit& r = ctx->light_refit;
  if (!r.bound) return 0;  // (the update that follows reports that the lights need a rebuild)
  if (num_transforms != r.num_transforms) { ctx->error = "lumc_light_refit_transforms: another number of transforms than the bound plan's"; return 1; }
  for (uint32_t i = 0; i < num_transforms; i++) {
    const LumLightTransform& t = transforms[i];
    bool finite = true;
    for (float x : t.q) finite = finite && std::isfinite(x);
    for (float x : t.scale) finite = finite && std::isfinite(x);
    for (float x : t.offset) finite = finite && std::isfinite(x);
    if (!finite) { ctx->error = "lumc_light_refit_transforms: a value that is not finite"; return 1; }
  }
  r.pending.assign(transforms, transforms + num_transforms);
  return 0;
}

int lumc_light_refit_needs_rebuild(const LumContext* ctx) { return ctx && ctx->light_refit_needs_rebuild ? 1 : 0; }

int lumc_light_refit_stats(const LumContext* ctx, LumLightRefitStats* out) {
  if (!ctx || !out) return 1;
  *out = ctx->light_refit_stats;
  return 0;
}

int lumc_light_arrays_probe(LumContext* ctx, uint64_t sizes[6], void* root, void* root_children, void* nodes, void* table, void* bvh_nodes, void* bvh_tris) {
  if (!ctx || !sizes) return 1;
  if (!ctx->has_scene) { ctx->error = "lumc_light_arrays_probe: the context has no scene"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  HIP_TRY(ctx, hipDeviceSynchronize());
  const SceneArrays::Lights& a = ctx->arrays.lights;
  sizes[0] = a.tree_root.count() * sizeof(uint4); sizes[1] = a.root_children.count(); sizes[2] = a.tree_nodes.count() * sizeof(uint4); sizes[3] = a.tri_table.count();
  sizes[4] = a.bvh_nodes.count(); sizes[5] = a.bvh_tris.count();
  auto down = [&](void* out, const void* src, size_t bytes) { return (out && bytes) ? hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost) : hipSuccess; };
  HIP_TRY(ctx, down(root, a.tree_root.get(), sizes[0]));
  HIP_TRY(ctx, down(root_children, a.root_children.get(), sizes[1] * sizeof(float)));
  HIP_TRY(ctx, down(nodes, a.tree_nodes.get(), sizes[2]));
  HIP_TRY(ctx, down(table, a.tri_table.get(), sizes[3] * sizeof(float4)));
  HIP_TRY(ctx, down(bvh_nodes, a.bvh_nodes.get(), sizes[4] * sizeof(Bvh4Node)));
  HIP_TRY(ctx, down(bvh_tris, a.bvh_tris.get(), sizes[5] * sizeof(BvhTri)));
  return 0;
}

int lumc_resident_mesh_nodes_probe(LumContext* ctx, void* nodes) {
  if (!ctx || !nodes) return 1;
  const InstanceUpdate& u = ctx->instance_update;
  if (!ctx->has_scene || !u.resident) { ctx->error = "lumc_resident_mesh_nodes_probe: the context has no resident layout"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (ctx->arrays.inst.nodes.count() != (size_t) u.capacity + u.mesh_nodes) { ctx->error = "lumc_resident_mesh_nodes_probe: the node array is not the layout's"; return 1; }
  if (u.mesh_nodes) HIP_TRY(ctx, hipMemcpy(nodes, ctx->scene.bvh_nodes + u.capacity, sizeof(Bvh4Node) * u.mesh_nodes, hipMemcpyDeviceToHost));
  return 0;
}

int lumc_resident_tree_probe(LumContext* ctx, uint64_t sizes[5], void* top_nodes, void* leaves, uint32_t* mesh_root, uint64_t* mesh_hash) {
  if (!ctx || !sizes) return 1;
  const InstanceUpdate& u = ctx->instance_update;
  if (!ctx->has_scene || !u.resident) { ctx->error = "lumc_resident_tree_probe: the context has no resident layout"; return 1; }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const DeviceScene& sc = ctx->scene;
  sizes[0] = u.capacity; sizes[1] = u.mesh_nodes; sizes[2] = sc.tlas_num_nodes; sizes[3] = sc.tlas_num_leaves; sizes[4] = ctx->instance_stats.tlas_depth;
  if (sc.tlas_num_leaves > u.num_instances + 1u) { ctx->error = "lumc_resident_tree_probe: more leaf records than instances"; return 1; }
  if (top_nodes) HIP_TRY(ctx, hipMemcpy(top_nodes, sc.bvh_nodes, sizeof(Bvh4Node) * u.capacity, hipMemcpyDeviceToHost));
  if (leaves) HIP_TRY(ctx, hipMemcpy(leaves, sc.tlas_leaves, sizeof(float4) * 4 * (size_t) sc.tlas_num_leaves, hipMemcpyDeviceToHost));
  if (mesh_root && u.num_meshes) HIP_TRY(ctx, hipMemcpy(mesh_root, u.mesh_root.get(), sizeof(uint32_t) * u.num_meshes, hipMemcpyDeviceToHost));
  if (mesh_hash) {
    std::vector<uint64_t> words((size_t) u.mesh_nodes * (sizeof(Bvh4Node) / 8));
    if (!words.empty()) HIP_TRY(ctx, hipMemcpy(words.data(), sc.bvh_nodes + u.capacity, sizeof(Bvh4Node) * u.mesh_nodes, hipMemcpyDeviceToHost));
    uint64_t h = 0xCBF29CE484222325ull;
    for (uint64_t w : words) { h = (h ^ w) * 0x100000001B3ull; h ^= h >> 29; }
    *mesh_hash = h;
  }
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
