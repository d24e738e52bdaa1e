// Stand-alone check of csrc/host/device_buffer.h against a counting fake of the HIP runtime (tests/test_device_buffer.py builds and runs it; it is not linked
// against HIP). The fake (fake_hip.h) keeps the set of live pointers: a free of a pointer it does not hold (a second free included) and any pointer still live at
// the end of a case fail the program, and it can be told to fail the k-th allocation.
#include <utility>
#include <vector>

#include "../../luminary_amd/csrc/host/device_buffer.h"
#include "fake_hip.h"

static void resize_combinations() {
  const size_t sizes[] = {8, 8, 32, 4, 0, 0, 16};  // same, larger, smaller, zero, zero again, from empty
  for (size_t first : sizes)
    for (size_t second : sizes) {
      DeviceBuffer<float> b;
      CHECK(!b && b.get() == nullptr && b.count() == 0);
      CHECK(b.resize(first) == hipSuccess);
      CHECK(b.count() == first && bool(b) == (first != 0) && g_live.size() == (first ? 1u : 0u));
      CHECK(b.resize(second) == hipSuccess);
      CHECK(b.count() == second && bool(b) == (second != 0) && g_live.size() == (second ? 1u : 0u));
      if (second) CHECK(g_live.count(b.get()) == 1);
      b.reset();
      CHECK(!b && b.count() == 0 && g_live.empty());
      b.reset();  // twice: nothing to free
    }
  end_case("resize_combinations");
}

static void failed_resize() {
  DeviceBuffer<int> b;
  CHECK(b.resize(5) == hipSuccess);
  g_fail_at = g_allocations;
  CHECK(b.resize(7) == hipErrorOutOfMemory);
  CHECK(b.count() == 0 && b.get() == nullptr && !b && g_live.empty());  // freed first, and empty after the failure
  CHECK(b.resize(7) == hipSuccess && b.count() == 7);
  g_fail_at = g_allocations;
  const int host[3] = {1, 2, 3};
  CHECK(b.assign(host, 3) == hipErrorOutOfMemory && b.count() == 0 && b.get() == nullptr);
  b.reset();
  end_case("failed_resize");
}

static void assign_cases() {
  const float host[4] = {1.0f, 2.0f, 3.0f, 4.0f};
  DeviceBuffer<float> b;
  CHECK(b.assign(host, 4) == hipSuccess && b.count() == 4 && std::memcmp(b.get(), host, sizeof(host)) == 0);
  const int copies = g_copies;
  CHECK(b.assign(nullptr, 4) == hipSuccess && !b && b.count() == 0 && g_live.empty());  // a null array: empty, and success
  CHECK(b.assign(host, 4) == hipSuccess && b.count() == 4);
  CHECK(b.assign(host, 0) == hipSuccess && !b && b.count() == 0 && g_live.empty());     // no elements: the same
  CHECK(b.assign(nullptr, 0) == hipSuccess && !b);
  CHECK(g_copies == copies + 1);
  end_case("assign_cases");
}

static void moves() {
  {
    DeviceBuffer<char> a;
    CHECK(a.resize(10) == hipSuccess);
    char* p = a.get();
    DeviceBuffer<char> b(std::move(a));  // move-construct
    CHECK(!a && a.count() == 0 && b.get() == p && b.count() == 10 && g_live.size() == 1);
    DeviceBuffer<char> c;
    CHECK(c.resize(20) == hipSuccess && g_live.size() == 2);
    c = std::move(b);  // move-assign onto a full buffer: what it held is freed
    CHECK(!b && c.get() == p && c.count() == 10 && g_live.size() == 1);
    DeviceBuffer<char>& self = c;
    c = std::move(self);  // self-move keeps the allocation
    CHECK(c.get() == p && c.count() == 10 && g_live.size() == 1);
    c = DeviceBuffer<char>();  // move-assign from an empty one
    CHECK(!c && g_live.empty());
  }
  static_assert(noexcept(DeviceBuffer<char>(std::declval<DeviceBuffer<char>>())), "vectors move their elements only if this is noexcept");
  static_assert(noexcept(std::declval<DeviceBuffer<char>&>() = std::declval<DeviceBuffer<char>>()), "");
  end_case("moves");
}

static void vector_of_buffers() {
  {
    std::vector<DeviceBuffer<char>> group;
    std::vector<char*> seen;
    for (size_t i = 0; i < 100; i++) {  // grown past its capacity several times: the elements move, nothing is freed or copied
      DeviceBuffer<char> d;
      CHECK(d.resize(i + 1) == hipSuccess);
      seen.push_back(d.get());
      group.push_back(std::move(d));
      CHECK(g_live.size() == i + 1);
    }
    for (size_t i = 0; i < 100; i++) CHECK(group[i].get() == seen[i] && group[i].count() == i + 1);
    group.clear();
    CHECK(g_live.empty());
    DeviceBuffer<char> last;
    CHECK(last.resize(3) == hipSuccess);
    group.push_back(std::move(last));
  }  // ... and the vector's destructor frees what it holds
  end_case("vector_of_buffers");
}

namespace {
struct Holder {  // shaped like LumContext::Adaptive: scalars, buffers, a vector
  bool active = false;
  unsigned blocks = 0;
  DeviceBuffer<unsigned> counts, tasks;
  DeviceBuffer<float> variance;
  DeviceBuffer<char> temp;
  std::vector<unsigned> host_copy;
};
}  // namespace

static void struct_reset() {
  {
    Holder a;
    for (int round = 0; round < 3; round++) {
      a = Holder();  // frees whatever the last round left
      CHECK(!a.active && !a.counts && !a.tasks && !a.variance && !a.temp && g_live.empty());
      a.active = true; a.blocks = 12;
      CHECK(a.counts.resize(12) == hipSuccess && a.tasks.resize(12) == hipSuccess && a.variance.resize(12) == hipSuccess);
      if (round == 1) CHECK(a.temp.resize(64) == hipSuccess);
      a.host_copy.assign(12, 7u);
      CHECK(g_live.size() == (round == 1 ? 4u : 3u));
    }
  }
  end_case("struct_reset");
}

// Shaped like the converted *_host wrappers: several uploads, then an output buffer, each behind an early return.
#define TRY(expr) do { if ((expr) != hipSuccess) return 1; } while (0)
static int wrapper(const float* origins, const float* dirs, const unsigned* ignore, unsigned n, int* reached) {
  DeviceBuffer<float> d_o, d_d;
  DeviceBuffer<unsigned> d_i, d_out;
  TRY(d_o.assign(origins, 3 * (size_t) n));
  TRY(d_d.assign(dirs, 3 * (size_t) n));
  TRY(d_i.assign(ignore, 2 * (size_t) n));
  TRY(d_out.resize(3 * (size_t) n));
  *reached = 1;
  return 0;
}

static void wrapper_failures() {
  const float rays[12] = {0};
  const unsigned ignore[8] = {0};
  for (int with_ignore = 0; with_ignore < 2; with_ignore++) {
    const int allocations = with_ignore ? 4 : 3;
    for (int k = 0; k <= allocations; k++) {  // k == allocations: nothing fails
      g_allocations = 0; g_fail_at = k;
      int reached = 0;
      const int rc = wrapper(rays, rays, with_ignore ? ignore : nullptr, 4, &reached);
      CHECK(rc == (k < allocations ? 1 : 0) && reached == (k < allocations ? 0 : 1));
      CHECK(g_live.empty());
      end_case("wrapper_failures");
    }
  }
}

int main() {
  resize_combinations();
  failed_resize();
  assign_cases();
  moves();
  vector_of_buffers();
  struct_reset();
  wrapper_failures();
  std::printf("%s (%d failures)\n", g_failures ? "FAILED" : "ok", g_failures);
  return g_failures ? 1 : 0;
}
