// The body of the kernels named k_shade (kernels.h), included into each of them: the general form's three-parameter template and the plain form's
// four-parameter one. Text, not a function: as a function that both kernels call the general kernels' register allocation changes (their arguments would
// reach it through references instead of being the kernel's own), and k_shade moves by 3-4 % with any such change (profiles/plain_form_isa.txt).
// In scope where it is included: the kernel's arguments and kSkyMode, kWater, kTable, kPlain.
  const uint32_t n = ctrl[kCtlPaths];
  uint32_t* count_out = ctrl + kCtlStride + kCtlPaths;
  // fused resolve, fused_flags & 4: the previous depth's vertices that no entry continues (its k_shade listed them) are input too - entries n .. n_input - 1 have
  // a parent and nothing else - instead of a kernel of their own after that depth's visibility pass (k_resolve_ended), which only waited for memory
  const uint32_t n_input = n + ((LUM_FAST && !kWater && (fused_flags & 5u) == 5u) ? (ctrl - kCtlStride)[kCtlSkyItems] : 0u);
  // (the fast flavour only: the exact flavour's sums land in the reference's order for every vertex, its kernels do not carry the code)
  // (its pointers come through memory, read where they are used: as kernel arguments they sat in scalar registers for the whole kernel, and the spills that
  // caused put 27 more lane reads into every iteration of the candidate loop)
  const bool resolve_parents = LUM_FAST && !kWater && (fused_flags & 1u) != 0u, announce_children = LUM_FAST && !kWater && (fused_flags & 2u) != 0u;
  // ambient_reuse (see AmbientReuse above): the ambient visibility of a surviving path comes from its next closest-hit ray; never with an ocean (the ambient
  // ray then ends at the water surface) or under the procedural sky (no ambient sample)
  const bool reuse_ambient = ambient_reuse != 0u && !kWater && kSkyMode != kSkyDefault;
  const uint32_t lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  const bool lights_present = sc.light_tree_root != nullptr && sc.num_lights > 0;
  const Col sky = (sc.sky_mode == kSkyConstantColor) ? col(sc.sky_constant_color[0], sc.sky_constant_color[1], sc.sky_constant_color[2]) : splat(0.0f);
  uint32_t vertices = 0;
  // Input by cursor: a wave takes the depth's queue entries in chunks through one atomic per chunk, fetched a chunk ahead, until the queue is used up. With a
  // fixed share per wave (a grid-stride loop) every wave of the grid ends on a partial batch of surface hits - one batch time per wave, 0.4 ms of a
  // 12.7 ms launch with 8 workgroups per resident place, measured as the intercept of time against pass size - and the more waves, the better the balance: with
  // the cursor the balance is the cursor's and the grid is the resident set (core.hip shade_grid). Chunks are guided: half of an equal share of what is left
  // (as far as the wave has seen the cursor), between 1 and kShadeChunkRounds rounds of 64 entries - long chunks while the queue is long (few atomics on one
  // word), single rounds at its end and in the short queues of deep depths, where a fixed 16 rounds left most of the chip without work (measured: +8 % on the
  // scan's and the Example-class scene's k_shade).
  // The cursor runs over a schedule of rounds of 64 entries: the queue's rounds with the rounds of the listed vertices (n .. n_input - 1: only a resolve, i.e.
  // only memory latency) spread evenly between them, one after every `every` of the queue's - at the queue's end they cost more than the kernel they replace
  // (all waves reach them together, with nothing to compute beside them: hall k_shade +9.5 ms per 3 steps for a kernel of 11.8).
  uint32_t* const cursor = ctrl + kCtlShadeCursor;
  const uint32_t n_listed = n_input - n, rounds_q = (n + 63u) / 64u, rounds_l = (n_listed + 63u) / 64u;
  const uint32_t every = rounds_l ? max(rounds_q / rounds_l, 1u) : 0u, groups = rounds_l ? min(rounds_l, rounds_q / every) : 0u;
  const uint32_t n_sched = (rounds_q + rounds_l) * 64u;
  auto entry_at = [&](uint32_t pos) -> uint32_t {  // the lane's entry at position `pos` of the schedule (wave-uniform, a multiple of 64): < n a queue entry, < n_input a listed vertex, else none
    const uint32_t t = pos / 64u, mixed = groups * (every + 1u);
    uint32_t base;
    bool listed;
    if (t < mixed) { const uint32_t g = t / (every + 1u), o = t - g * (every + 1u); listed = o == every; base = listed ? g : g * every + o; }
    else { const uint32_t r = t - mixed, left = rounds_q - groups * every; listed = r >= left; base = listed ? groups + (r - left) : groups * every + r; }
    const uint32_t e = base * 64u + lane;
    return listed ? (e < n_listed ? n + e : 0xFFFFFFFFu) : (e < n ? e : 0xFFFFFFFFu);
  };
  const uint32_t share_div = gridDim.x * (kBlock / 64u) * 2u * 64u;  // entries per round and wave, twice
  auto guided = [&](uint32_t seen) -> uint32_t { return 64u * min(max((seen < n_sched ? n_sched - seen : 0u) / share_div, 1u), kShadeChunkRounds); };
  uint32_t chunk_len = guided(0u), next_len = chunk_len;
  uint32_t grabbed = 0u;  // lane 0: the chunk after next (the atomic's result is only looked at when the current chunk ends)
  if (lane == 0u) grabbed = atomicAdd(cursor, chunk_len);
  uint32_t chunk = (uint32_t) __builtin_amdgcn_readfirstlane((int) grabbed), chunk_round = 0u;
  // a workgroup that only starts when the queue is used up (the grid is a little larger than the resident set, so that every place is taken from the start
  // wherever the dispatcher puts the workgroups) leaves before it stages anything
  if (!__syncthreads_or((int) (chunk < n_sched))) return;
  next_len = guided(chunk + chunk_len);
  if (lane == 0u) grabbed = atomicAdd(cursor, next_len);
  // Paths that left the scene only add the sky term; the surface vertices are two orders of magnitude more work. A wave therefore
  // collects the indices of its surface hits in LDS and shades them 64 at a time, so that misses do not leave lanes idle during the
  // expensive part (the reference sorts tasks by hit type for the same reason, cuda/kernels.cuh:391-484).
  __shared__ uint32_t pending_hits[kBlock / 64][128];
  uint32_t* pending = pending_hits[threadIdx.x >> 6];
  uint32_t num_pending = 0;  // wave-uniform
  // the candidate loop's table lines and handles of the first lights, in LDS (dev_light.h StagedLights)
  StagedLights staged_lights{nullptr, nullptr, 0u};
#if LUM_LDS_LIGHTS
  {
    __shared__ LdsF4 lds_light_table[4u * LUM_LDS_LIGHTS];
    __shared__ unsigned long long lds_light_handles[LUM_LDS_LIGHTS];
    const uint32_t staged = lights_present ? min(sc.num_lights, (uint32_t) LUM_LDS_LIGHTS) : 0u;
    for (uint32_t k = threadIdx.x; k < 4u * staged; k += kBlock) { const float4 v = sc.light_tri_table[k]; const LdsF4 t = {v.x, v.y, v.z, v.w}; lds_light_table[k] = t; }
    for (uint32_t k = threadIdx.x; k < staged; k += kBlock) { const uint2 h = sc.light_tri_handles[k]; lds_light_handles[k] = (unsigned long long) h.x | ((unsigned long long) h.y << 32); }
    __syncthreads();
    staged_lights.table = (const __attribute__((address_space(3))) LdsF4*) lds_light_table;
    staged_lights.handles = (const __attribute__((address_space(3))) unsigned long long*) lds_light_handles;
    staged_lights.count = staged;
  }
#endif
  ShadeClock clock;
  clock.start();
  // fused resolve: an entry's parent word and slot are fetched one round ahead (two registers across the batch in between: one dependent round trip less per round)
  uint32_t parent_ahead = 0u, slot_ahead = 0u;
  if (resolve_parents) {
    const uint32_t i0 = entry_at(chunk);
    if (i0 < n) { parent_ahead = in.parent[i0]; slot_ahead = fbits(reinterpret_cast<const float*>(&in.dir_slot[i0])[3]); }
    else if (i0 < n_input) parent_ahead = fused_dev->ended_prev[i0 - n];
  }
  // (the counter is unused since the grid-stride form of this loop left; the loop keeps its shape because without the counter's increment block the compiler lays the
  // kernel out differently - up to 24 bytes more scratch and a few hundred instructions' difference per instance, profiles/retired_variants_isa_identity.txt)
  for ([[maybe_unused]] uint32_t round = 0;; round++) {
    const bool input_done = chunk >= n_sched;
    if (!input_done) {
      const uint32_t i = entry_at(chunk + chunk_round * 64u);
      if (++chunk_round * 64u == chunk_len) {  // on to the chunk fetched ahead, and one more on its way
        chunk_round = 0u;
        chunk = (uint32_t) __builtin_amdgcn_readfirstlane((int) grabbed);
        chunk_len = next_len;
        next_len = guided(chunk + chunk_len);
        if (lane == 0u) grabbed = atomicAdd(cursor, next_len);
      }
      const uint32_t i_ahead = entry_at(chunk + chunk_round * 64u);  // (none once the schedule is used up)
      bool is_hit = false, is_sky = false;
      if (resolve_parents) {  // the vertex this entry continues: its sum, before the entry's own emission or sky term
        const FusedResolve& fused = *fused_dev;
        bool undecided = false;
        uint32_t ip = 0;
        uint4 amb = make_uint4(0u, 0u, 0u, 0u);
        const uint32_t p = parent_ahead;
        uint32_t slot = slot_ahead;
        {
          if (i_ahead < n) { parent_ahead = in.parent[i_ahead]; slot_ahead = fbits(reinterpret_cast<const float*>(&in.dir_slot[i_ahead])[3]); }
          else if (i_ahead < n_input) parent_ahead = fused.ended_prev[i_ahead - n];  // (its slot: with the vertex's records below)
        }
        if (i < n_input) {
          ip = p & kParentMask;
          // resolve_records<2> for a plain scene (no fog, no ocean: the reuse's condition), written out: the records, then - together - the hit word of a
          // deferred sample, the visibility words that matter and the result slot; the sums in the reference's order
          if (i >= n) slot = fbits(reinterpret_cast<const float*>(&fused.prev.dir_slot[ip])[3]);  // a listed vertex: the result slot from its own queue entry
          const uint4 paux = ld_stream(&fused.prev.aux[ip]);
          const float4 cl = ld_stream(&fused.nee_prev.geo_color_light[ip]), lc = ld_stream(&fused.nee_prev.bsdf_weight_sum[ip]);
          amb = ld_stream(&fused.nee_prev.ambient[ip]);
          uint4 sun = make_uint4(0u, 0u, 0u, 0u);
          if (kSkyMode == kSkyHdri) sun = fused.nee_prev.sun[ip];
          const bool deferred = (p & kParentDeferred) != 0u;
          const bool need_geo = fbits(cl.w) != kLightIdInvalid && lights_present && ((paux.w & kStVolumeScattered) == 0), need_bsdf = lc.w != 0.0f;
          const bool need_amb = !deferred && (amb.x != 0 || amb.y != 0), need_sun = kSkyMode == kSkyHdri && (sun.x != 0 || sun.y != 0);
          const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
          float4 vg = zero, vb = zero, va = zero, vs = zero;
          uint32_t word = 0u;
          const float4* __restrict__ vis = fused.fallback.vis;  // (the previous depth's visibility words: sq.vis)
          const uint32_t cap = fused.fallback.capacity;
          if (deferred) word = in.hit_scene_tri[i];
          if (need_geo) vg = ld_stream(&vis[ip]);
          if (need_bsdf) vb = ld_stream(&vis[cap + ip]);
          if (need_amb) va = ld_stream(&vis[2u * cap + ip]);
          if (need_sun) vs = vis[3u * cap + ip];
          const float4 before = results[slot];
          float ambient_vis = 0.0f;
          if (deferred) {  // nothing hit (and no cut-out skipped) = visible; an opaque nearest hit beyond eps = blocked; anything else is not decided here
            if (!(word & kHitTriHit)) { undecided = (word & kHitTriCutout) != 0u; ambient_vis = 1.0f; }
            else undecided = (word & (kHitTriBeyondEps | kHitTriOpaque)) != (kHitTriBeyondEps | kHitTriOpaque);
          }
          if (!undecided) {
            Col acc = splat(0.0f);
            acc = acc + col(cl.x, cl.y, cl.z) * col(vg.x, vg.y, vg.z);
            acc = acc + col(lc.x, lc.y, lc.z) * col(vb.x, vb.y, vb.z);
            if (kSkyMode == kSkyHdri) acc = acc + record_unpack(U2{sun.x, sun.y}) * col(vs.x, vs.y, vs.z);
            acc = acc + record_unpack(U2{amb.x, amb.y}) * (deferred ? splat(ambient_vis) : col(va.x, va.y, va.z));
            const Col v = acc * record_unpack(U2{paux.x, paux.y});
            if (any_positive(v)) results[slot] = make_float4(before.x + v.r, before.y + v.g, before.z + v.b, before.w);
          }
        }
        const unsigned long long bu = __ballot(undecided);
        if (bu) {  // rare: the vertex's own ambient ray, from its hit point along the record's packed direction (direct_lighting.cuh:388-405)
          uint32_t base = 0;
          if (lane == (uint32_t) __builtin_ctzll(bu)) {
            base = atomicAdd(ctrl + kCtlVolumeShadowItems, (uint32_t) __popcll(bu));
            atomicAdd((unsigned long long*) &counters[kCntAmbientFallback], (unsigned long long) __popcll(bu));
          }
          base = __shfl(base, __builtin_ctzll(bu));
          if (undecided) {
            const uint32_t k = base + (uint32_t) __popcll(bu & below);
            const float4 o4 = fused.prev.origin_t[ip], d4 = fused.prev.dir_slot[ip];  // the vertex's hit point as its own visibility rays had it (this path starts at the point projected onto the triangle)
            const V3 hit_origin = v3(o4.x, o4.y, o4.z) + v3(d4.x, d4.y, d4.z) * o4.w;
            const uint2 self = *reinterpret_cast<const uint2*>(&fused.prev.hit_id[ip]);
            const V3 ar = ray_unpack(U2{amb.z, amb.w});
            fused.fallback.origin_dist[k] = make_float4(hit_origin.x, hit_origin.y, hit_origin.z, kFltMax);
            fused.fallback.dir_out[k] = make_float4(ar.x, ar.y, ar.z, bitsf(2u * sq.capacity + ip));
            fused.fallback.ids[k] = make_uint4(0xFFFFFFFFu, 0u, self.x, self.y);
            fused.fallback.light_items[k] = ip;
          }
        }
      }
      if (i < n) {
        const uint32_t hit_type = in.hit_id[i].x;
        if (hit_type == kHitSky) {
          const uint4 aux = in.aux[i];
          if (aux.w & kStAllowAmbient) {
            if (kSkyMode == kSkyDefault) is_sky = true;  // the atmosphere is ray-marched by k_sky
            else if (kSkyMode == kSkyHdri) {
              const float4 o4 = in.origin_t[i], d4 = in.dir_slot[i];
              add_to_result(results, fbits(d4.w), sky_hdri_color(sc, v3(o4.x, o4.y, o4.z), v3(d4.x, d4.y, d4.z), aux.w) * record_unpack(U2{aux.x, aux.y}));
            }
            else add_to_result(results, fbits(in.dir_slot[i].w), sky * record_unpack(U2{aux.x, aux.y}));
          }
        }
        else is_hit = hit_type <= kHitTriangleLimit;  // fog: scattering events are bounced by k_volume_bounce, kHitInvalid ended in k_volume_events
      }
      const unsigned long long bs = __ballot(is_sky);
      if (bs) {  // the list grows downwards from the end of the light-query list: a path is in at most one of the two
        uint32_t base = 0;
        if (lane == (uint32_t) __builtin_ctzll(bs)) base = atomicAdd(ctrl + kCtlSkyItems, (uint32_t) __popcll(bs));
        base = __shfl(base, __builtin_ctzll(bs));
        if (is_sky) sq.light_items[sq.capacity - 1u - (base + (uint32_t) __popcll(bs & below))] = i;
      }
      const unsigned long long bh = __ballot(is_hit);
      if (is_hit) pending[num_pending + (uint32_t) __popcll(bh & below)] = i;
      num_pending += (uint32_t) __popcll(bh);
    }
    if (num_pending < 64u && !(input_done && num_pending > 0u)) {
      if (input_done) break;
      continue;
    }
    __builtin_amdgcn_wave_barrier();
    LUM_LAP(clock, 8);
    const uint32_t take = min(num_pending, 64u);
    num_pending -= take;
    const bool valid = lane < take;
    const uint32_t i = valid ? pending[num_pending + lane] : 0u;
    __builtin_amdgcn_wave_barrier();
    bool survive = false, want_geo = false, want_amb = false, want_sun = false, want_lq = false;
    float4 n_o, n_d; uint4 n_aux, n_hid;
    float4 s_origin, s_geo_dir, s_amb_dir, s_sun_dir; uint4 s_geo_ids;
    bool want_amb2 = false, want_sun2 = false;  // kWater: second segments beyond the water surface
    float4 s_amb2_o, s_amb2_d, s_sun2_o, s_sun2_d;
    if (valid) {
      const float4 o4 = ld_stream(&in.origin_t[i]), d4 = ld_stream(&in.dir_slot[i]);
      const uint4 aux = ld_stream(&in.aux[i]), hid = ld_stream(&in.hit_id[i]);
      const uint32_t slot = fbits(d4.w), state = aux.w;
      const Col record_in = record_unpack(U2{aux.x, aux.y});
      {
        vertices++;
        const V3 origin = v3(o4.x, o4.y, o4.z), ray = v3(d4.x, d4.y, d4.z);
        const V3 hit_origin = origin + ray * o4.w;
        SamplerT<kTable> smp{sc.bluenoise_2d, hid.z & 0xFFFFu, hid.z >> 16, path_sample_id(hid.w), depth_const};
        smp.use_table(sc.sobol_table + (size_t) depth_const * kRndTargetCount * sc.sobol_stride, sc.sobol_stride, sc.sobol_first);  // (kTable: the pass has one)
        const GeoContext g = build_context<kPlain>(sc, hit_origin, ray, state, hid.x, hid.y, in.hit_scene_tri[i] & kHitTriMask, aux.z);
        // the volume the vertex is in: without an ocean the stack holds the fog or nothing for the whole path
        const uint32_t top_volume = kWater ? volume_stack_peek(hid.w, false) : (sc.fog_active ? (uint32_t) kVolumeFog : (uint32_t) kVolumeNone);
        const uint32_t second_volume = kWater ? volume_stack_peek(hid.w, true) : (uint32_t) kVolumeNone;

        // NEE work (geometry.cuh:31-74; direct_lighting.cuh:352-443)
        const bool geo_allowed = lights_present && ((state & kStVolumeScattered) == 0);
        LUM_LAP(clock, 0);
        float4 geo_cl = make_float4(0.0f, 0.0f, 0.0f, bitsf(kLightIdInvalid));
        float4 bs_rp = make_float4(0.0f, 0.0f, 1.0f, 0.0f), bs_ws = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        s_origin = make_float4(hit_origin.x, hit_origin.y, hit_origin.z, 0.0f);
        s_geo_ids = make_uint4(0xFFFFFFFFu, 0u, hid.x, hid.y);
#ifndef LUM_ABLATE
#define LUM_ABLATE 0  // measurement only: 1 skips light sampling, 2 the BSDF light direction, 4 the bounce (results are wrong)
#endif
        float light_root_sum = 0.0f;
        if (geo_allowed) {
          LightSample ls;
          if (LUM_ABLATE & 1) { ls.light_id = kLightIdInvalid; ls.root_sum = 1.0f; ls.color = splat(0.0f); ls.ray = v3(0.0f, 0.0f, 1.0f); ls.dist = 1.0f; }
          else ls = sample_light<kPlain>(sc, g, smp, clock, staged_lights);
          if (top_volume != kVolumeNone) ls.color = ls.color * volume_transmittance(sc, top_volume, g.position, ls.ray, ls.dist);  // direct_lighting.cuh:329-337
          geo_cl = make_float4(ls.color.r, ls.color.g, ls.color.b, bitsf(ls.light_id));
          light_root_sum = ls.root_sum;
          if (ls.light_id != kLightIdInvalid) {
            want_geo = true;
            const uint2 target = light_handle<kPlain>(sc, staged_lights, ls.light_id);  // from the staged copy where there is one: no dependent round trip to memory
            s_geo_dir = make_float4(ls.ray.x, ls.ray.y, ls.ray.z, ls.dist);
            s_geo_ids.x = target.x; s_geo_ids.y = target.y;
          }
        }
        // the shading frame is formed after the light sampling: its thirteen registers need not live through the candidate loop
        const LocalFrame lf = local_frame(sc, g);
        if (geo_allowed) {
          LightDirSample lb;
          if (LUM_ABLATE & 2) { lb.ray = v3(0.0f, 0.0f, 1.0f); lb.weight = splat(0.0f); lb.probability = 0.0f; }
          else lb = sample_light_direction(lf, g, smp);
          bs_rp = make_float4(lb.ray.x, lb.ray.y, lb.ray.z, lb.probability);
          if (lb.probability != 0.0f) {
            want_lq = true;
            bs_ws = make_float4(lb.weight.r, lb.weight.g, lb.weight.b, light_root_sum);
          }
          LUM_LAP(clock, 3);
        }
        BounceSample bounce;
        if (LUM_ABLATE & 4) { bounce.ray = g.normal; bounce.weight = splat(0.5f); bounce.transparent_pass = false; bounce.microfacet_based = false; }
        else bounce = sample_bounce(lf, g, smp, 0);
        uint4 amb = make_uint4(0u, 0u, 0u, 0u);
        if (kSkyMode != kSkyDefault) {  // ambient: the bounce direction doubles as the sample (direct_lighting.cuh:388-405)
          const Col ambient = (kSkyMode == kSkyHdri) ? sky_hdri_color(sc, g.position, bounce.ray, 0u) : sky;
          const U2 c = record_pack(ambient * bounce.weight), r = ray_pack(bounce.ray);
          amb = make_uint4(c.x, c.y, r.x, r.y);
          if (c.x != 0 || c.y != 0) {
            const V3 ar = ray_unpack(r);
            if (kWater) {
              const SkyRayPlan plan = plan_ambient_ray(sc, hit_origin, hid.x, top_volume, second_volume, true, ar);
              if (!plan.valid) amb = make_uint4(0u, 0u, r.x, r.y);
              else {
                want_amb = true;
                s_amb_dir = make_float4(ar.x, ar.y, ar.z, plan.limit);
                nee.amb_t1[i] = make_float4(plan.t1.r, plan.t1.g, plan.t1.b, plan.fresnel_factor);
                nee.amb_t2[i] = make_float4(plan.t2.r, plan.t2.g, plan.t2.b, bitsf(sky_ray_flags(plan)));
                if (plan.second && !plan.total_reflection) {
                  want_amb2 = true;
                  s_amb2_o = make_float4(plan.second_origin.x, plan.second_origin.y, plan.second_origin.z, kFltMax);
                  s_amb2_d = make_float4(plan.second_dir.x, plan.second_dir.y, plan.second_dir.z, 0.0f);
                }
              }
            }
            else {
              want_amb = true;
              s_amb_dir = make_float4(ar.x, ar.y, ar.z, kFltMax);
            }
          }
        }
        LUM_LAP(clock, 4);
        if (kSkyMode != kSkyConstantColor) {  // the sun: its own record and the fourth kind of visibility ray
          uint4 sun = make_uint4(0u, 0u, 0u, 0u);
          Col sun_light; V3 sun_dir;
          bool have_sun;
          if (kWater && top_volume == kVolumeOcean) have_sun = sun_caustic_sample(sc, sky_view(sc), g, smp, 0u, top_volume, second_volume, sun_light, sun_dir);  // direct_lighting.cuh:368-380
          else {
            have_sun = sample_sun(sc, sky_view(sc), lf, g, smp, sun_light, sun_dir);
            if (have_sun && top_volume != kVolumeNone) sun_light = sun_light * volume_transmittance(sc, top_volume, g.position, sun_dir, kFltMax);  // direct_lighting.cuh:104-108
          }
          if (have_sun) {
            const U2 c = record_pack(sun_light), r = ray_pack(sun_dir);
            sun = make_uint4(c.x, c.y, r.x, r.y);
            if (c.x != 0 || c.y != 0) {
              want_sun = true;
              const V3 ar = ray_unpack(r);
              s_sun_dir = make_float4(ar.x, ar.y, ar.z, kFltMax);
              if (kWater) {
                const SkyRayPlan plan = plan_sun_ray(sc, hit_origin, hid.x, top_volume, true, ar);
                s_sun_dir.w = plan.limit;
                nee.sun_water[i] = make_float4(plan.fresnel_factor, 0.0f, 0.0f, bitsf(sky_ray_flags(plan)));
                if (plan.second && !plan.total_reflection) {
                  want_sun2 = true;
                  s_sun2_o = make_float4(plan.second_origin.x, plan.second_origin.y, plan.second_origin.z, kFltMax);
                  s_sun2_d = make_float4(plan.second_dir.x, plan.second_dir.y, plan.second_dir.z, 0.0f);
                }
              }
            }
          }
          st_stream(&nee.sun[i], sun);
          LUM_LAP(clock, 5);
        }
        st_stream(&nee.geo_color_light[i], geo_cl);
        st_stream(&nee.bsdf_ray_prob[i], bs_rp); st_stream(&nee.bsdf_weight_sum[i], bs_ws);
        st_stream(&nee.ambient[i], amb);

        // delta-path classification (geometry.cuh:80-101)
        const float roughness = g.params.roughness();
        bool is_delta;
        if (bounce.transparent_pass) {
          const float ior = g.params.ior();
          const float rs = (ior >= 1.0f) ? ior : 1.0f / ior;
          is_delta = roughness * fminf(rs - 1.0f, 1.0f) <= 0.05f;
        }
        else is_delta = bounce.microfacet_based && (roughness <= 0.05f);
        const bool pass_through = is_pass_through(g, bounce);

        // emission and throughput (geometry.cuh:103-119)
        Col record = record_in;
        const Col emission = g.params.emission();
        if (any_positive(emission)) add_to_result(results, slot, emission * record);
        record = record * bounce.weight;

        uint32_t new_state = state | kStUseIgnoreHandle;
        if (kSkyMode != kSkyDefault && !pass_through) new_state &= ~kStAllowAmbient; else new_state |= kStAllowAmbient;
        if (!is_delta) new_state &= ~kStDeltaPath;
        if (!pass_through) new_state &= ~(kStCameraDirection | kStAllowEmission);

        // russian roulette (directives.cuh:11-32)
        survive = true;
        if ((state & kStDeltaPath) == 0) {
          const float value = importance(record);
          if (value < sc.cam_rr_threshold) {
            const float p = (value > 0.0f) ? fmaxf(value / sc.cam_rr_threshold, 1.0f / 8.0f) : 0.0f;
            if (smp.next1(kRndRussianRoulette) > p) survive = false;
            else record = record * (1.0f / p);
          }
        }
        if (survive) {
          uint32_t medium = aux.z;
          if (bounce.transparent_pass) {
            const bool inside = (g.params.flags & kMatRefractionInside) != 0;
            float new_ior = 1.0f;
            if (!inside) new_ior = medium_ior_peek(medium, inside) / g.params.ior();
            medium = medium_ior_modify(medium, new_ior, !inside);
          }
          const U2 rp = record_pack(record);
          n_o = make_float4(g.position.x, g.position.y, g.position.z, kFltMax);
          n_d = make_float4(bounce.ray.x, bounce.ray.y, bounce.ray.z, d4.w);
          n_aux = make_uint4(rp.x, rp.y, medium, new_state);
          n_hid = make_uint4(g.instance_id, g.tri_id, hid.z, hid.w);
        }
      }
    }
    const bool amb_deferred = reuse_ambient && want_amb && survive;  // answered by the path's next closest-hit ray
    if (amb_deferred) { want_amb = false; vertices += 1u << 16; }   // counted in the upper half of the lane's vertex counter (a lane shades a few hundred vertices per launch)
    LUM_LAP(clock, 6);
    // Wave-aggregated appends. The three lists (survivors, visibility items, light queries) are reserved by ONE memory instruction: lanes 0-2
    // each bump one counter, so a batch waits for one atomic round trip instead of three in a row (the words sit on separate 128-byte lines).
    const unsigned long long ballot = __ballot(survive);
    const unsigned long long bg = __ballot(want_geo), ba = __ballot(want_amb), bn = __ballot(want_sun), bl = __ballot(want_lq);
    const unsigned long long b2a = kWater ? __ballot(want_amb2) : 0ull, b2s = kWater ? __ballot(want_sun2) : 0ull;
    const uint32_t ng = (uint32_t) __popcll(bg), na = (uint32_t) __popcll(ba), ns = (uint32_t) __popcll(bn), na2 = (uint32_t) __popcll(b2a);
    const unsigned long long be = announce_children ? __ballot(valid && !survive) : 0ull;  // fused resolve: vertices no entry will continue, listed for k_resolve_ended (a fourth counter, same instruction)
    const uint32_t want_count = (lane == 0) ? (uint32_t) __popcll(ballot) : (lane == 1) ? ng + na + ns + na2 + (uint32_t) __popcll(b2s) : (lane == 2) ? (uint32_t) __popcll(bl) :
                                (lane == 3) ? (uint32_t) __popcll(be) : 0u;
    uint32_t* const want_word = (lane == 0) ? count_out : (lane == 1) ? ctrl + kCtlShadowItems : (lane == 2) ? ctrl + kCtlLightItems : ctrl + kCtlSkyItems;
    uint32_t reserved = 0;
    if (want_count) reserved = atomicAdd(want_word, want_count);
    const uint32_t base_out = __builtin_amdgcn_readlane(reserved, 0), base_shadow = __builtin_amdgcn_readlane(reserved, 1), base_light = __builtin_amdgcn_readlane(reserved, 2);
    uint32_t amb_path = kNoAmbientPath;
    if (survive) {
      const uint32_t j = base_out + (uint32_t) __popcll(ballot & below);
      st_stream(&out.origin_t[j], n_o); st_stream(&out.dir_slot[j], n_d); st_stream(&out.aux[j], n_aux); st_stream(&out.hit_id[j], n_hid);
      amb_path = amb_deferred ? j : kNoAmbientPath;
      if (announce_children) out.parent[j] = i | (amb_deferred ? kParentDeferred : 0u);
    }
    if (reuse_ambient && valid && !announce_children) nee.amb_path[i] = amb_path;  // every vertex of the depth: k_resolve_reuse reads it for each of them (the fused resolve has the parent words and the list below instead)
    if (be != 0ull && valid && !survive) fused_dev->ended[__builtin_amdgcn_readlane(reserved, 3) + (uint32_t) __popcll(be & below)] = i;
    if (want_geo) {
      const uint32_t j = base_shadow + (uint32_t) __popcll(bg & below);
      st_stream(&sq.origin_dist[j], make_float4(s_origin.x, s_origin.y, s_origin.z, s_geo_dir.w));
      st_stream(&sq.dir_out[j], make_float4(s_geo_dir.x, s_geo_dir.y, s_geo_dir.z, bitsf(i)));
      st_stream(&sq.ids[j], s_geo_ids);
    }
    if (want_amb) {
      const uint32_t j = base_shadow + ng + (uint32_t) __popcll(ba & below);
      st_stream(&sq.origin_dist[j], make_float4(s_origin.x, s_origin.y, s_origin.z, s_amb_dir.w));
      st_stream(&sq.dir_out[j], make_float4(s_amb_dir.x, s_amb_dir.y, s_amb_dir.z, bitsf(2u * sq.capacity + i)));
      st_stream(&sq.ids[j], make_uint4(0xFFFFFFFFu, 0u, s_geo_ids.z, s_geo_ids.w));
    }
    if (want_sun) {
      const uint32_t j = base_shadow + ng + na + (uint32_t) __popcll(bn & below);
      st_stream(&sq.origin_dist[j], make_float4(s_origin.x, s_origin.y, s_origin.z, s_sun_dir.w));
      st_stream(&sq.dir_out[j], make_float4(s_sun_dir.x, s_sun_dir.y, s_sun_dir.z, bitsf(3u * sq.capacity + i)));
      st_stream(&sq.ids[j], make_uint4(0xFFFFFFFFu, 0u, s_geo_ids.z, s_geo_ids.w));
    }
    if (kWater) {  // second segments beyond the water surface
      if (want_amb2) {
        const uint32_t j = base_shadow + ng + na + ns + (uint32_t) __popcll(b2a & below);
        sq.origin_dist[j] = s_amb2_o;
        sq.dir_out[j] = make_float4(s_amb2_d.x, s_amb2_d.y, s_amb2_d.z, bitsf(kShadowKindAmbient2 * sq.capacity + i));
        sq.ids[j] = make_uint4(0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u);
      }
      if (want_sun2) {
        const uint32_t j = base_shadow + ng + na + ns + na2 + (uint32_t) __popcll(b2s & below);
        sq.origin_dist[j] = s_sun2_o;
        sq.dir_out[j] = make_float4(s_sun2_d.x, s_sun2_d.y, s_sun2_d.z, bitsf(kShadowKindSun2 * sq.capacity + i));
        sq.ids[j] = make_uint4(0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u);
      }
    }
    if (want_lq) sq.light_items[base_light + (uint32_t) __popcll(bl & below)] = i;
    LUM_LAP(clock, 7);
  }
  clock.flush();
  uint32_t deferred = vertices >> 16;
  vertices &= 0xFFFFu;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { vertices += __shfl_down(vertices, off); deferred += __shfl_down(deferred, off); }
  if ((threadIdx.x & 63) == 0 && vertices) atomicAdd((unsigned long long*) &counters[kCntVertices], (unsigned long long) vertices);
  if ((threadIdx.x & 63) == 0 && deferred) atomicAdd((unsigned long long*) &counters[kCntAmbientDeferred], (unsigned long long) deferred);
