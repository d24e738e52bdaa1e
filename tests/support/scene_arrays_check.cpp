// Stand-alone check of csrc/host/scene_arrays.h against the counting fake of the HIP runtime (fake_hip.h; tests/test_scene_arrays.py builds and runs it, not
// linked against HIP): what scene_device.hip does with the owners - release a part and fill it again, replace some arrays of a part and keep the others, the
// whole scene freed by one assignment, a part whose n-th allocation fails - frees every allocation exactly once and never one of another part.
#include <algorithm>
#include <map>
#include <string>

#include "../../luminary_amd/csrc/host/scene_arrays.h"
#include "fake_hip.h"

using lum::SceneArrays;

#define TRY(expr) do { if ((expr) != hipSuccess) return 1; } while (0)
template <typename T>
static hipError_t fill(DeviceBuffer<T>& owner, size_t count) {  // a few elements, as upload() does: assign from a host array
  std::vector<T> host(count);
  std::memset(static_cast<void*>(host.data()), 0, sizeof(T) * count);
  return owner.assign(host.data(), count);
}

// every part filled the way its update_* function fills it: released first, then array by array behind early returns
static int fill_mesh_arrays(SceneArrays::Mesh& a) {  // update_mesh_arrays: not the traversal triangles
  a.tri_offset.reset(); a.vertices.reset(); a.tri_tex.reset();
  TRY(fill(a.tri_offset, 3)); TRY(fill(a.vertices, 12)); TRY(fill(a.tri_tex, 4));
  return 0;
}
static int fill_inst(SceneArrays::Inst& a) {
  a = {};
  TRY(fill(a.mesh_ids, 3)); TRY(fill(a.transforms, 6)); TRY(fill(a.rows, 9)); TRY(fill(a.nodes, 5)); TRY(fill(a.tlas_leaves, 16));
  return 0;
}
static int fill_lights(SceneArrays::Lights& a) {
  a = {};
  TRY(fill(a.tree_root, 4)); TRY(fill(a.root_children, 80)); TRY(fill(a.tree_nodes, 8)); TRY(fill(a.tri_handles, 2)); TRY(fill(a.bvh_nodes, 1)); TRY(fill(a.bvh_tris, 2));
  TRY(a.tri_table.resize(8));
  return 0;
}
static int relayout(SceneArrays::Inst& a) {  // relayout_resident: the node array anew, the leaf records with room for every instance
  a.nodes.reset(); a.tlas_leaves.reset();
  TRY(fill(a.nodes, 7)); TRY(a.tlas_leaves.resize(16));
  return 0;
}
static int fill_all(SceneArrays& a) {
  a.mesh.blas_tris.reset();
  if (fill_mesh_arrays(a.mesh) || fill_inst(a.inst) || fill_lights(a.lights)) return 1;
  TRY(fill(a.mesh.blas_tris, 5));
  a.materials = {}; TRY(fill(a.materials.materials, 6));
  a.textures = {}; TRY(fill(a.textures.table, 2)); TRY(fill(a.textures.texels, 64));
  a.constants = {};
  TRY(fill(a.constants.stars, 3)); TRY(fill(a.constants.stars_offsets, 9));
  for (auto& b : a.constants.cloud_noise) TRY(fill(b, 8));
  for (auto& b : a.constants.sky_lut) TRY(fill(b, 4));
  TRY(fill(a.constants.sky_hdri, 4));
  a.particles = {}; TRY(fill(a.particles.nodes, 2)); TRY(fill(a.particles.tris, 3)); TRY(fill(a.particles.leaves, 8)); TRY(fill(a.particles.normals, 1));
  TRY(fill(a.bluenoise_2d, 16));
  return 0;
}

// every array's address by "part.member"
static std::map<std::string, void*> pointers(const SceneArrays& a) {
  return {{"mesh.tri_offset", a.mesh.tri_offset.get()}, {"mesh.vertices", a.mesh.vertices.get()}, {"mesh.tri_tex", a.mesh.tri_tex.get()}, {"mesh.blas_tris", a.mesh.blas_tris.get()},
          {"inst.mesh_ids", a.inst.mesh_ids.get()}, {"inst.transforms", a.inst.transforms.get()}, {"inst.rows", a.inst.rows.get()}, {"inst.tlas_leaves", a.inst.tlas_leaves.get()},
          {"inst.nodes", a.inst.nodes.get()}, {"materials.materials", a.materials.materials.get()},
          {"lights.tree_root", a.lights.tree_root.get()}, {"lights.tree_nodes", a.lights.tree_nodes.get()}, {"lights.root_children", a.lights.root_children.get()},
          {"lights.tri_handles", a.lights.tri_handles.get()}, {"lights.tri_table", a.lights.tri_table.get()}, {"lights.bvh_nodes", a.lights.bvh_nodes.get()},
          {"lights.bvh_tris", a.lights.bvh_tris.get()}, {"textures.table", a.textures.table.get()}, {"textures.texels", a.textures.texels.get()},
          {"constants.stars", a.constants.stars.get()}, {"constants.stars_offsets", a.constants.stars_offsets.get()}, {"constants.cloud_noise[0]", a.constants.cloud_noise[0].get()},
          {"constants.cloud_noise[1]", a.constants.cloud_noise[1].get()}, {"constants.cloud_noise[2]", a.constants.cloud_noise[2].get()},
          {"constants.sky_lut[0]", a.constants.sky_lut[0].get()}, {"constants.sky_lut[1]", a.constants.sky_lut[1].get()}, {"constants.sky_hdri", a.constants.sky_hdri.get()},
          {"particles.nodes", a.particles.nodes.get()}, {"particles.tris", a.particles.tris.get()}, {"particles.leaves", a.particles.leaves.get()},
          {"particles.normals", a.particles.normals.get()}, {"bluenoise_2d", a.bluenoise_2d.get()}};
}
constexpr size_t kArrays = 32;

// A step of an update: the arrays named in `replaced` (whole names, or a prefix such as "lights.") - and only those - were freed, each once; every other array
// is at its address and live; nothing is live without an owner.
struct Step {
  std::map<std::string, void*> before;
  explicit Step(const SceneArrays& a) : before(pointers(a)) { g_freed.clear(); }
  void check(const char* step, const SceneArrays& a, const std::vector<std::string>& replaced) const {
    const std::map<std::string, void*> after = pointers(a);
    std::vector<void*> expected, freed = g_freed;
    std::set<void*> owned;
    for (const auto& kv : after) if (kv.second) owned.insert(kv.second);
    for (const auto& kv : before) {
      bool is_replaced = false;
      for (const std::string& r : replaced) is_replaced |= kv.first.compare(0, r.size(), r) == 0;
      if (is_replaced) { if (kv.second) expected.push_back(kv.second); continue; }
      if (after.at(kv.first) != kv.second || (kv.second && !g_live.count(kv.second))) { std::printf("FAILED %s: %s moved or was freed\n", step, kv.first.c_str()); g_failures++; }
    }
    std::sort(expected.begin(), expected.end()); std::sort(freed.begin(), freed.end());
    if (freed != expected) { std::printf("FAILED %s: %zu pointers freed, %zu expected (or not the same ones)\n", step, freed.size(), expected.size()); g_failures++; }
    if (g_live != owned) { std::printf("FAILED %s: %zu allocations live, %zu owned\n", step, g_live.size(), owned.size()); g_failures++; }
  }
};

static void whole_scene() {
  {
    SceneArrays a;
    CHECK(fill_all(a) == 0);
    const auto p = pointers(a);
    CHECK(p.size() == kArrays && g_live.size() == kArrays);
    for (const auto& kv : p) CHECK(kv.second != nullptr && g_live.count(kv.second) == 1);
    a = SceneArrays{};  // free_scene
    CHECK(g_live.empty());
    for (const auto& kv : pointers(a)) CHECK(kv.second == nullptr);
    CHECK(fill_all(a) == 0 && g_live.size() == kArrays);  // ... and the next upload
  }  // the context's destructor
  end_case("whole_scene");
}

static void one_part_replaced() {
  {
    SceneArrays a;
    CHECK(fill_all(a) == 0);
    Step release(a);
    a.lights = {};
    CHECK(g_live.size() == kArrays - 7);
    for (const auto& kv : pointers(a)) CHECK((kv.second == nullptr) == (kv.first.compare(0, 7, "lights.") == 0));
    release.check("lights released", a, {"lights."});
    Step refill(a);
    CHECK(fill_lights(a.lights) == 0);
    refill.check("lights refilled", a, {"lights."});
    Step again(a);
    CHECK(fill_lights(a.lights) == 0);  // released and filled in one go, as update_light_tree does
    again.check("lights replaced", a, {"lights."});
    Step materials(a);
    a.materials = {}; CHECK(fill(a.materials.materials, 10) == hipSuccess);
    materials.check("materials", a, {"materials."});
    Step particles(a);
    a.particles = {};
    particles.check("particles off", a, {"particles."});
  }
  end_case("one_part_replaced");
}

static void moved_vertices() {
  {
    SceneArrays a;
    CHECK(fill_all(a) == 0);
    const Step step(a);
    lum::BvhTri* tris = a.mesh.blas_tris.get();
    CHECK(fill_mesh_arrays(a.mesh) == 0);
    CHECK(a.mesh.blas_tris.get() == tris && g_live.count(tris) == 1 && a.mesh.blas_tris.count() == 5);
    for (void* p : g_freed) CHECK(p != tris);
    step.check("moved vertices", a, {"mesh.tri_offset", "mesh.vertices", "mesh.tri_tex"});
  }
  end_case("moved_vertices");
}

static void resident_relayout() {
  {
    SceneArrays a;
    CHECK(fill_all(a) == 0);
    const Step step(a);
    CHECK(relayout(a.inst) == 0);
    CHECK(a.inst.mesh_ids.get() == step.before.at("inst.mesh_ids") && a.inst.transforms.get() == step.before.at("inst.transforms") && a.inst.rows.get() == step.before.at("inst.rows"));
    CHECK(a.inst.nodes.count() == 7 && a.inst.tlas_leaves.count() == 16);
    step.check("re-layout", a, {"inst.nodes", "inst.tlas_leaves"});
  }
  end_case("resident_relayout");
}

static void failed_allocations() {
  for (int k = 0; k <= 7; k++) {  // the light part's seven allocations fail in turn; k == 7: none does
    {
      SceneArrays a;
      CHECK(fill_all(a) == 0);
      const Step step(a);
      g_allocations = 0; g_fail_at = k;
      CHECK(fill_lights(a.lights) == (k < 7 ? 1 : 0));
      g_fail_at = -1;
      const void* first = a.lights.tree_root.get();
      CHECK(k == 0 ? first == nullptr : (first != nullptr && g_live.count(const_cast<void*>(first)) == 1));  // valid or empty, never a freed pointer
      step.check("failed light allocation", a, {"lights."});  // no other part touched, nothing live without an owner
      a = SceneArrays{};  // what lumc_scene_update does with a failed update
      CHECK(g_live.empty());
    }
    end_case("failed_allocations");
  }
  for (int k = 0; k < 2; k++) {  // the re-layout's two
    {
      SceneArrays a;
      CHECK(fill_all(a) == 0);
      const Step step(a);
      g_allocations = 0; g_fail_at = k;
      CHECK(relayout(a.inst) == 1);
      g_fail_at = -1;
      CHECK(!a.inst.tlas_leaves && bool(a.inst.nodes) == (k == 1));
      step.check("failed re-layout", a, {"inst.nodes", "inst.tlas_leaves"});
      const Step host_path(a);
      CHECK(fill_inst(a.inst) == 0);  // the host path replaces what it left
      host_path.check("host path after it", a, {"inst."});
    }
    end_case("failed_allocations");
  }
}

int main() {
  whole_scene();
  one_part_replaced();
  moved_vertices();
  resident_relayout();
  failed_allocations();
  std::printf("%s (%d failures)\n", g_failures ? "FAILED" : "ok", g_failures);
  return g_failures ? 1 : 0;
}
