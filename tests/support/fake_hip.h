// A counting fake of the HIP runtime for the stand-alone checks of the host layer's owners of device memory (device_buffer_check.cpp, scene_arrays_check.cpp;
// each is one translation unit that is not linked against HIP). hipMalloc / hipFree / hipMemcpy over malloc with the set of live pointers: a free of a pointer
// it does not hold (a second free included) and any pointer still live at the end of a case fail the program, and it can be told to fail the k-th allocation.
#pragma once

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>
#include <vector>

#include <hip/hip_runtime_api.h>

static std::set<void*> g_live;
static std::vector<void*> g_freed;  // every pointer freed, in order (a check clears it where its step begins)
static int g_failures = 0, g_allocations = 0, g_fail_at = -1, g_copies = 0;

#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); g_failures++; } } while (0)

extern "C" hipError_t hipMalloc(void** p, size_t bytes) {
  if (g_allocations++ == g_fail_at) { *p = nullptr; return hipErrorOutOfMemory; }
  *p = std::malloc(bytes ? bytes : 1);
  g_live.insert(*p);
  return hipSuccess;
}
extern "C" hipError_t hipFree(void* p) {
  if (!p) return hipSuccess;
  if (!g_live.erase(p)) { std::printf("FAILED: free of %p, which is not live\n", p); g_failures++; return hipErrorInvalidValue; }
  g_freed.push_back(p);
  std::free(p);
  return hipSuccess;
}
extern "C" hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  if (kind != hipMemcpyHostToDevice || !g_live.count(dst)) { std::printf("FAILED: copy to %p\n", dst); g_failures++; return hipErrorInvalidValue; }
  std::memcpy(dst, src, bytes);
  g_copies++;
  return hipSuccess;
}

static void end_case(const char* name) {
  if (!g_live.empty()) { std::printf("FAILED %s: %zu allocations live at its end\n", name, g_live.size()); g_failures++; }
  for (void* p : g_live) std::free(p);
  g_live.clear(); g_freed.clear();
  g_allocations = 0; g_fail_at = -1;
}

