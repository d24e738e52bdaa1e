// The host twin of k_shutter_vertices (mesh_shutter.hip): mesh_shutter.h's shutter_record compiled by the host compiler, no HIP in it. It defines the bytes the
// kernel is held to (lum_core.h lumc_shutter_host; tests/test_mesh_shutter.py, tests/test_mesh_shutter_gpu.py).
#define LUM_DEFORM_HOST_ONLY 1
#include "mesh_shutter.h"

#include <string.h>

extern "C" int lumc_shutter_host(const void* open_records, const void* close_records, uint32_t count, float t, void* out_records, uint32_t* flags) {
  if (!open_records || !close_records || !out_records) return 1;
  if (!lum::skin_finite(t) || !(t >= 0.0f) || !(t <= 1.0f)) return 1;
  static_assert(sizeof(lum::ShutterRecord) == 16, "the scene's vertex record");
  const char *a = static_cast<const char*>(open_records), *b = static_cast<const char*>(close_records);
  char* out = static_cast<char*>(out_records);
  uint32_t flag = 0;
  for (size_t c = 0; c < count; c++) {  // (out may be one of the inputs: a record is read before it is written)
    lum::ShutterRecord ra, rb, r;
    memcpy(&ra, a + 16 * c, 16);
    memcpy(&rb, b + 16 * c, 16);
    flag |= lum::shutter_record(ra, rb, t, &r);
    memcpy(out + 16 * c, &r, 16);
  }
  if (flags) *flags = flag;
  return 0;
}
