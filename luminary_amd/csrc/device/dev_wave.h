// The wave64 idioms of the shading kernels (kernels.h), written once: the wave-aggregated append to a compacted list, the batch loop over a sparse
// subset of the queue, the visibility-ray record, and the russian roulette of the shading kernels. Everything here is force-inlined. The helpers that take
// and return values (rank, count, reserve, push_visibility) leave a kernel's instructions as they were with the text written out; the ones that hold a
// variable of the kernel by reference (the lambdas of append and for_each_batch, roulette's record) do not - same operations, another register
// allocation. A kernel is on those only where its time was measured to be what it was (k_ocean_shade, k_volume_inscatter); k_shade, k_particle_shade and
// k_clouds keep their own text of the loop and the roulette (profiles/wave_helpers_isa_identity.txt).
#pragma once

#include "dev_math.h"
#include "dev_scene.h"
#include "dev_sampler.h"

LUM_NS_BEGIN

constexpr int kBlock = 256;  // threads per workgroup of every kernel in kernels.h and kernels_shared.h (context.h's kLaunchBlock on the host side)

struct Wave {
  uint32_t lane;              // 0..63
  unsigned long long below;   // the lanes before this one
  LUM_DEV Wave() : lane(threadIdx.x & 63u), below((1ull << (threadIdx.x & 63u)) - 1ull) {}
  static LUM_DEV uint32_t count(unsigned long long ballot) { return (uint32_t) __popcll(ballot); }
  LUM_DEV uint32_t rank(unsigned long long ballot) const { return (uint32_t) __popcll(ballot & below); }  // of a lane that is in the ballot: its place among them

  // `count` (wave-uniform) consecutive entries of the list that `counter` counts: lane 0 adds, every lane gets the first entry's index. Nothing is issued
  // for a count of 0. One run may hold several kinds of entry (k_particle_shade: sampled light, ambient, sun), each behind the ones before it.
  LUM_DEV uint32_t reserve(uint32_t* counter, uint32_t count) const {
    uint32_t base = 0;
    if (count != 0u) {
      if (lane == 0) base = atomicAdd(counter, count);
      base = __builtin_amdgcn_readfirstlane(base);
    }
    return base;
  }
  // One kind of entry: every lane that wants one writes it at the index `write` is given, in lane order.
  template <class Write>
  LUM_DEV void append(bool want, uint32_t* counter, Write&& write) const {
    const unsigned long long b = __ballot(want);
    if (b != 0ull) {
      const uint32_t base = reserve(counter, count(b));
      if (want) write(base + rank(b));
    }
  }

  // The sparse-subset loop. The queue entries a kernel has work for are few (water-surface hits, paths inside a volume), so one lane per entry would
  // leave most of a wave idle during the expensive part. Instead the wave walks the queue grid-stride, collects the indices `pick` accepts in its LDS
  // slice `pending` (128 words: up to 63 carried over plus the 64 of a round) and hands them to `batch` 64 at a time - once 64 are pending, or the input
  // is used up and something is left. pick(idx) runs once for every entry of the queue (idx < n), by the lane that walks it, and may do the entry's
  // cheap work itself. batch(valid, i) is called by all 64 lanes (the bodies ballot); i is the lane's entry where valid.
  // k_shade, k_particle_shade and k_clouds keep a copy of this loop each: on the helper their instructions change (k_clouds measured slower on it,
  // k_particle_shade has no benchmark configuration to be timed with), see profiles/wave_helpers_isa_identity.txt.
  template <class Pick, class Batch>
  LUM_DEV void for_each_batch(uint32_t n, uint32_t* pending, Pick&& pick, Batch&& batch) const {
    uint32_t num_pending = 0;  // wave-uniform
    const uint32_t rounds = (n + gridDim.x * kBlock - 1) / (gridDim.x * kBlock);
    for (uint32_t round = 0;; round++) {
      const bool input_done = round >= rounds;
      if (!input_done) {
        const uint32_t idx = (round * gridDim.x + blockIdx.x) * kBlock + threadIdx.x;
        const bool picked = idx < n && pick(idx);
        const unsigned long long b = __ballot(picked);
        if (picked) pending[num_pending + rank(b)] = idx;
        num_pending += count(b);
      }
      if (num_pending < 64u && !(input_done && num_pending > 0u)) {
        if (input_done) break;
        continue;
      }
      __builtin_amdgcn_wave_barrier();
      const uint32_t take = min(num_pending, 64u);
      num_pending -= take;
      const bool valid = lane < take;
      const uint32_t i = valid ? pending[num_pending + lane] : 0u;
      __builtin_amdgcn_wave_barrier();
      batch(valid, i);
    }
  }
};

// One visibility ray (ShadowQueue, dev_scene.h) at entry j: from `origin` along `dir` up to `dist`; its transparency goes to sq.vis[tag], tag =
// kind * capacity + path index. ids: the triangle the ray is meant to reach and the one it starts on. kStream: streaming stores (k_shade's records are
// read once, by another kernel).
template <bool kStream = false>
LUM_DEV void push_visibility(ShadowQueue sq, uint32_t j, float4 origin_dist, float4 dir_tag, uint4 ids) {  // the record's words as they are stored
  if (kStream) { st_stream(&sq.origin_dist[j], origin_dist); st_stream(&sq.dir_out[j], dir_tag); st_stream(&sq.ids[j], ids); }
  else { sq.origin_dist[j] = origin_dist; sq.dir_out[j] = dir_tag; sq.ids[j] = ids; }
}
template <bool kStream = false>
LUM_DEV void push_visibility(ShadowQueue sq, uint32_t j, V3 origin, V3 dir, float dist, uint32_t tag, uint4 ids) {
  push_visibility<kStream>(sq, j, make_float4(origin.x, origin.y, origin.z, dist), make_float4(dir.x, dir.y, dir.z, bitsf(tag)), ids);
}
// ... with the origin in a float4's xyz and the direction and distance in one float4, as the shading kernels carry them across their ballots
template <bool kStream = false>
LUM_DEV void push_visibility(ShadowQueue sq, uint32_t j, float4 origin, float4 dir_dist, uint32_t tag, uint4 ids) {
  push_visibility<kStream>(sq, j, v3(origin.x, origin.y, origin.z), v3(dir_dist.x, dir_dist.y, dir_dist.z), dir_dist.w, tag, ids);
}
// The second segment of a sky ray that goes on beyond the water surface: open-ended, nothing to reach and nothing to leave out.
LUM_DEV void push_second_segment(ShadowQueue sq, uint32_t j, V3 origin, V3 dir, uint32_t tag) {
  push_visibility(sq, j, origin, dir, kFltMax, tag, make_uint4(0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u));
}

// Russian roulette (directives.cuh:11-32): a path that is not a delta path and whose throughput `record` has sunk below the camera's threshold goes on with
// probability p = importance / threshold (at least 1/8) and is weighted by 1 / p. Returns whether the path goes on.
template <class S>
LUM_DEV bool roulette(const DeviceScene& sc, uint32_t state, const S& smp, Col& record) {
  if ((state & kStDeltaPath) == 0) {
    const float value = importance(record);
    if (value < sc.cam_rr_threshold) {
      const float p = (value > 0.0f) ? fmaxf(value / sc.cam_rr_threshold, 1.0f / 8.0f) : 0.0f;
      if (smp.next1(kRndRussianRoulette) > p) return false;
      record = record * (1.0f / p);
    }
  }
  return true;
}

LUM_NS_END
