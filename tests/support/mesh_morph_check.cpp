// Stand-alone check of the morph twin (csrc/host/mesh_deform.cpp), built with the address and undefined-behaviour sanitizers by tests/test_mesh_morph.py: triangle
// counts on either side of a wave and of a workgroup of corners; 1, 3 and 1024 targets with the last target named; a corner with an entry in every target, one
// with a single entry, one with none; with and without normal deltas, with and without a skin of 1 and 1024 bones; outputs that alias the inputs, outputs left
// out, refused arguments. What it computes is held to numpy there; here every access is.
#define LUM_DEFORM_HOST_ONLY 1
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../luminary_amd/csrc/host/mesh_deform.h"

static int fail(const char* what, unsigned triangles, unsigned targets) {
  std::printf("mesh_morph_check: %s (triangles %u, targets %u)\n", what, triangles, targets);
  return 1;
}

static float rnd(unsigned& s) { s = s * 1664525u + 1013904223u; return (float) (s >> 8) * (1.0f / 8388608.0f) - 1.0f; }

int main() {
  const unsigned counts[] = {1, 21, 22, 85, 86}, target_counts[] = {1, 3, 1024};
  for (unsigned nt : counts)
    for (unsigned T : target_counts) {
      unsigned seed = nt * 7919u + T;
      const size_t corner_count = 3 * (size_t) nt;
      std::vector<float> p(3 * corner_count), n(3 * corner_count), w(T);
      for (float& x : p) x = 10.0f * rnd(seed);
      for (size_t c = 0; c < corner_count; c++) { n[3 * c] = 0.0f; n[3 * c + 1] = 0.6f; n[3 * c + 2] = -0.8f; }
      // target t holds corner 0, corner 1 if it is the last target, never corner 2, and every corner c > 2 with (c + t) % 5 == 0; its delta is 2^-t' per row,
      // t' = t % 8, so that with weights of 1 every sum is exact and the expected value is computed without rounding
      std::vector<uint32_t> offsets(T + 1, 0), corners;
      std::vector<float> dp, dn;
      for (unsigned t = 0; t < T; t++) {
        for (size_t c = 0; c < corner_count; c++) {
          const bool in = c == 0 || (c == 1 && t == T - 1) || (c > 2 && (c + t) % 5 == 0);
          if (!in) continue;
          corners.push_back((uint32_t) c);
          const float d = 1.0f / (float) (1u << (t % 8));
          dp.push_back(d); dp.push_back(-d); dp.push_back(0.0f);
          dn.push_back(0.0f); dn.push_back(0.0f); dn.push_back(-d);
        }
        offsets[t + 1] = (uint32_t) corners.size();
      }
      for (unsigned t = 0; t < T; t++) w[t] = (t % 3 == 1) ? -0.0f : 1.0f;
      w[T - 1] = 1.0f;
      const size_t entries = corners.size();
      std::vector<float> op(3 * corner_count), on(3 * corner_count);
      std::vector<uint32_t> packed(corner_count);
      uint64_t bad = 7;
      if (lum::morph_host(p.data(), n.data(), nt, T, offsets.data(), corners.data(), dp.data(), dn.data(), w.data(), nullptr, nullptr, nullptr, 0, op.data(), on.data(), packed.data(), &bad))
        return fail("refused valid arguments", nt, T);
      if (bad != 0) return fail("finite results counted as not finite", nt, T);
      for (size_t c = 0; c < corner_count; c++) {
        double sum = 0.0;  // exact: multiples of 2^-7 far below 2^24 of them
        unsigned used = 0;
        for (unsigned t = 0; t < T; t++) {
          const bool in = c == 0 || (c == 1 && t == T - 1) || (c > 2 && (c + t) % 5 == 0);
          if (in && w[t] != 0.0f) { sum += 1.0 / (double) (1u << (t % 8)); used++; }
        }
        if (c == 2 && used != 0) return fail("the corner without an entry has one", nt, T);
        if (c == 1 && used != 1) return fail("the corner of the last target is not named by it", nt, T);
        if (used == 0) {
          if (std::memcmp(&op[3 * c], &p[3 * c], 12) != 0 || std::memcmp(&on[3 * c], &n[3 * c], 12) != 0) return fail("an untouched corner is not the base record", nt, T);
          continue;
        }
        // (the additions go entry by entry; every partial sum p + k / 128 rounds as the whole does only if p is a multiple of 2^-7 too: compare loosely here, byte for byte in the tests)
        const float want_x = (float) ((double) p[3 * c] + sum), want_y = (float) ((double) p[3 * c + 1] - sum);
        if (std::fabs(op[3 * c] - want_x) > 1e-3f || std::fabs(op[3 * c + 1] - want_y) > 1e-3f || op[3 * c + 2] != p[3 * c + 2]) return fail("a morphed position is off", nt, T);
        if (packed[c] != lum::skin_pack_normal(on.data() + 3 * c)) return fail("a packed word is not that of the normal", nt, T);
      }
      // in place, with outputs left out, without normal deltas
      std::vector<float> p2 = p, n2 = n;
      if (lum::morph_host(p2.data(), n2.data(), nt, T, offsets.data(), corners.data(), dp.data(), dn.data(), w.data(), nullptr, nullptr, nullptr, 0, p2.data(), n2.data(), nullptr, nullptr))
        return fail("refused in place", nt, T);
      if (p2 != op || n2 != on) return fail("in place differs", nt, T);
      if (lum::morph_host(p.data(), n.data(), nt, T, offsets.data(), corners.data(), dp.data(), nullptr, w.data(), nullptr, nullptr, nullptr, 0, p2.data(), nullptr, nullptr, nullptr))
        return fail("refused without normal deltas", nt, T);
      if (p2 != op) return fail("without normal deltas the positions differ", nt, T);
      if (lum::morph_host(p.data(), n.data(), nt, T, offsets.data(), corners.data(), dp.data(), dn.data(), w.data(), nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr))
        return fail("refused without outputs", nt, T);
      // with a skin of 1 and of 1024 bones, the last bone named: translations, two half weights
      for (unsigned nb : {1u, 1024u}) {
        std::vector<float> bones(12 * (size_t) nb, 0.0f), sw(4 * corner_count);
        std::vector<uint16_t> ids(4 * corner_count);
        for (unsigned b = 0; b < nb; b++) {
          float* m = bones.data() + 12 * (size_t) b;
          m[0] = m[5] = m[10] = 1.0f;
          m[3] = (float) b * 0.25f; m[7] = -1.0f; m[11] = 2.0f;
        }
        for (size_t c = 0; c < corner_count; c++) {
          const uint16_t b = (uint16_t) ((c % 3 == 0) ? nb - 1 : (c * 2654435761u) % nb);
          ids[4 * c] = b; ids[4 * c + 1] = (uint16_t) (nb - 1); ids[4 * c + 2] = b; ids[4 * c + 3] = 0;
          sw[4 * c] = 0.5f; sw[4 * c + 1] = 0.0f; sw[4 * c + 2] = 0.5f; sw[4 * c + 3] = -0.0f;
        }
        std::vector<float> sp(3 * corner_count), sn(3 * corner_count);
        if (lum::morph_host(p.data(), n.data(), nt, T, offsets.data(), corners.data(), dp.data(), dn.data(), w.data(), ids.data(), sw.data(), bones.data(), nb, sp.data(), sn.data(),
                            packed.data(), &bad) || bad != 0)
          return fail("refused with a skin", nt, T);
        for (size_t c = 0; c < corner_count; c++) {
          const float* m = bones.data() + 12 * (size_t) ids[4 * c];
          for (int k = 0; k < 3; k++) {
            const float t = op[3 * c + k] + m[4 * k + 3], want = (0.0f + 0.5f * t) + 0.5f * t;  // (op: the morphed position, which no normalisation touches)
            if (std::memcmp(&want, &sp[3 * c + k], 4) != 0) return fail("a morphed and translated position differs", nt, T);
          }
        }
        ids[4 * (corner_count - 1) + 3] = (uint16_t) nb;
        std::vector<float> untouched = sp;
        if (!lum::morph_host(p.data(), n.data(), nt, T, offsets.data(), corners.data(), dp.data(), dn.data(), w.data(), ids.data(), sw.data(), bones.data(), nb, sp.data(), sn.data(),
                             packed.data(), nullptr))
          return fail("a bone id beyond the palette was taken", nt, T);
        if (untouched != sp) return fail("a refused call wrote", nt, T);
        ids[4 * (corner_count - 1) + 3] = 0;
        if (!lum::morph_host(p.data(), n.data(), nt, T, offsets.data(), corners.data(), dp.data(), dn.data(), w.data(), ids.data(), sw.data(), bones.data(), 1025, nullptr, nullptr, nullptr, nullptr))
          return fail("1025 bones taken", nt, T);
      }
      // refused: a corner one beyond the mesh, a target's corners out of order, offsets from 1 and decreasing, no targets, too many, a weight and a delta that are not finite
      std::vector<float> untouched = op;
      auto refused = [&](const std::vector<uint32_t>& o, const std::vector<uint32_t>& c, const std::vector<float>& d, const std::vector<float>& ww, unsigned targets) {
        return lum::morph_host(p.data(), n.data(), nt, targets, o.data(), c.data(), d.data(), dn.data(), ww.data(), nullptr, nullptr, nullptr, 0, op.data(), on.data(), packed.data(), nullptr) != 0 &&
               untouched == op;
      };
      std::vector<uint32_t> c2 = corners, o2 = offsets;
      c2[entries - 1] = (uint32_t) corner_count;
      if (!refused(offsets, c2, dp, w, T)) return fail("a corner beyond the mesh was taken", nt, T);
      if (offsets[1] >= 2) {
        c2 = corners; c2[1] = c2[0];
        if (!refused(offsets, c2, dp, w, T)) return fail("a corner twice in a target was taken", nt, T);
      }
      o2[0] = 1;
      if (!refused(o2, corners, dp, w, T)) return fail("offsets from 1 were taken", nt, T);
      if (T >= 3) {
        o2 = offsets; o2[1] = offsets[2] + 1;
        if (!refused(o2, corners, dp, w, T)) return fail("offsets that decrease were taken", nt, T);
      }
      if (!refused(offsets, corners, dp, w, 0)) return fail("no targets were taken", nt, T);
      std::vector<uint32_t> wide(1026, 0);
      std::vector<float> wide_w(1025, 1.0f);
      if (!refused(wide, corners, dp, wide_w, 1025)) return fail("1025 targets were taken", nt, T);
      std::vector<float> w2 = w, d2 = dp;
      w2[T - 1] = INFINITY;
      if (!refused(offsets, corners, dp, w2, T)) return fail("a weight that is not finite was taken", nt, T);
      d2[3 * (entries - 1) + 1] = NAN;
      if (!refused(offsets, corners, d2, w, T)) return fail("a delta that is not finite was taken", nt, T);
      // weights that overflow are counted, not a fault
      for (float& x : w) x = 3e38f;
      for (float& x : dp) x *= 1e3f;
      if (lum::morph_host(p.data(), n.data(), nt, T, offsets.data(), corners.data(), dp.data(), dn.data(), w.data(), nullptr, nullptr, nullptr, 0, op.data(), on.data(), packed.data(), &bad) || bad == 0)
        return fail("overflowing weights went unnoticed", nt, T);
    }
  std::printf("mesh_morph_check: ok\n");
  return 0;
}
