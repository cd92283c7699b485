// rt_wf_fused_body.inc: the body of wf_trace_fused (rt_wf_device.hpp), included by the kernel and by
// its register-capped twin wf_trace_fused_cap, so that both compile the same statements.
// In scope: the template arguments PRIMARY, QUADS, LANE, TALLY, CAM, TRIS, CSG, ALIAS and the
// kernel arguments sc, cam, a.
  __shared__ int stack_lds[lane_static_lds_bytes(LANE) ? lane_static_lds_bytes(LANE) / 4 : 1];  // (1: never read)
  extern __shared__ __attribute__((aligned(16))) unsigned char lane_dyn[];
  __shared__ unsigned s_pre[kPreRays];
  const unsigned* pre = shard_prefix<true>(a.in_cnt, s_pre);
  if (a.dev_sized) bind_generation(a, pre);
  // a block without a chunk (static split below: its first chunk lies past the
  // last) leaves before staging the image; the exit is block-uniform
  const unsigned n_chunks = (a.n + 63u) / 64u;
  const unsigned waves_per_block = blockDim.x / 64u;
  const unsigned W = gridDim.x * waves_per_block;
  // fewer chunks than waves (a small frame, a deep generation): chunk c goes to
  // block c mod grid, so that the chunks spread over every CU instead of filling
  // the first blocks' CUs (a block's waves share one CU: 16 latency-bound walks
  // on one CU against 4-5 each): a 320x240 frame alone 24-29 % faster, frames
  // in flight slower (WfTuning::spread, off by default; profiles/r06_spread.txt)
  const bool spread = a.spread && n_chunks < W;
  if (spread ? blockIdx.x >= n_chunks : blockIdx.x * waves_per_block >= n_chunks) return;
  typedef LaneImage<LANE> Image;
  Image img;
  img.stage(sc, a.lds_flags, a.n_top, stack_lds, lane_dyn);
  FusedTally t;
  // Work distribution: chunk c = rays [64c, 64c + 64), one wave-iteration.
  // A launch with more chunks than waves hands them out dynamically from the
  // counter of the wave's block class (blocks are dealt round-robin to the 8
  // XCDs): class x holds the chunks x + X k. A wave that finishes early takes
  // the next chunk, so the launch ends with the last chunk, not with the
  // slowest wave of a static split (an LDS image holds its CU until every wave
  // of its block is done): C3 1.098 -> 1.013 ms/frame. The next chunk is asked
  // for when the current one starts. A launch with one to three chunks per
  // wave (the deep generations; most generations of a 2-way shard) gives each
  // wave its first chunk statically (chunk = wave index, no atomic to wait
  // for) and hands out the rest, W + x + X k, from the class counters: a
  // 2-way shard 0.554 -> 0.540 ms/frame; the same form for the large launches
  // cost 1.5 % on C3 (their chunks then leave the class-interleaved order).
  // A launch with at most one chunk per wave (an 8-way shard's deep
  // generations) strides over them statically, with no atomics.
  // Every lane of a wave works on the same chunk (the
  // appends are wave-wide); the chunk index is the wave-iteration index the
  // appends' regions and capacities are defined by.
  const bool dyn_all = n_chunks >= 3u * W;            // every chunk from the counters
  const bool dyn_tail = !dyn_all && n_chunks > W;     // the first chunk static, the rest from the counters
  const bool dyn = dyn_all || dyn_tail;
  const unsigned X = gridDim.x < (unsigned)kChunkClasses ? gridDim.x : (unsigned)kChunkClasses;
  const unsigned cls = blockIdx.x % X;
  unsigned* ctr = a.cnt->chunk + ((size_t)a.g * kChunkClasses + cls) * kChunkStride;
  const unsigned c_base = dyn_all ? cls : W + cls;  // the class's k-th counter chunk: c_base + X k
  unsigned c = spread ? (threadIdx.x / 64u) * gridDim.x + blockIdx.x : blockIdx.x * waves_per_block + threadIdx.x / 64u;
  if (dyn_all) {
    unsigned k0 = 0;
    if (lane_id() == 0) k0 = atomicAdd(ctr, 1u);
    c = cls + X * (unsigned)__shfl((int)k0, 0, 64);
  }
  // the chunk's rays, traversed: o, d and the hit of ray i (slot) of chunk c
  auto traverse = [&](unsigned i, bool valid, unsigned slot, V3& o, V3& d, Hit& h) {
    hit_init(h);
    if (valid) {
      wf_ray<CAM>(a, cam, slot, o, d);
      if constexpr (TALLY && QUADS) count_hier_gates<TRIS, CSG>(sc, o, d, t.gsk);
      if constexpr (!Image::kPerLane) {
        // the chunk's frame (chunks never mix frames): its shared-origin primary records
        const unsigned pf = a.n_frames > 1 ? (c * 64u) / a.frame_rays : 0u;
        img.template closest<PRIMARY>(sc, (cPrimRec)(a.prim + (size_t)pf * ((unsigned)sc.n_diag + 4)), o, d, h, t.disc,
                                      t.tests, t.boxes);
      }
      // (a per-lane walk: planes and the other records first, an early nearest hit tightens the culling)
      trace_rest<false, QUADS, true, TRIS, CSG, ALIAS, true, RUNS>(sc, o, d, h, t.disc, &t.gsk);
      if constexpr (QUADS) {
        other_trace<false>(sc, o, d, 0.0, h, t.disc, t.tests, t.boxes);
        line_trace<false>(sc, o, d, 0.0, h, t.tests, t.boxes);
      }
      if constexpr (TRIS) tri_trace<false>(sc, o, d, 0.0, h, t.tests, t.boxes);
      if constexpr (CSG) unit_trace<false>(sc, o, d, 0.0, h, t.disc, t.tests, t.boxes);
      if constexpr (Image::kPerLane) img.template walk<false>(sc, o, d, 0.0, h, t.disc, t.tests, t.boxes);
    }
    hit_finish(h);
    if constexpr (ALIAS) alias_finish(sc, h);
  };
  while (c < n_chunks) {
    unsigned k_next = 0;
    if (dyn && lane_id() == 0) k_next = atomicAdd(ctr, 1u);
    const unsigned i = c * 64u + lane_id();
    // a batch's generation 0: the padding slots after each frame's root rays hold no ray
    const bool valid = i < a.n && (a.g != 0 || a.n_frames <= 1 || i % a.frame_rays < a.frame_real);
    const unsigned slot = valid ? shard_slot<true>(pre, a.in_cap, i) : 0u;
    V3 o = v3(0, 0, 0), d = v3(0, 0, 0);
    Hit h;
    traverse(i, valid, slot, o, d, h);
    shade_fused<QUADS, CAM, TALLY, TRIS, CSG, ALIAS, RUNS>(sc, cam, a, img, c, slot, valid, o, d, h, t);
    c = dyn ? c_base + X * (unsigned)__shfl((int)k_next, 0, 64) : c + W;
  }
  if constexpr (!TALLY) return;
  if (sc.n_groups) add_gate_skips(a.cnt, t.gsk);
  const unsigned long long s = wave_sum(t.disc), st = wave_sum(t.tests), sb = wave_sum(t.boxes);
  const unsigned long long hs = wave_sum(t.sh_disc), hst = wave_sum(t.sh_tests), hsb = wave_sum(t.sh_boxes);
  const unsigned long long hr = wave_sum(t.sh_rays);
  if (lane_id() == 0) {
    WfWorkRow* w = work_row(a.cnt);
    if (s) atomicAdd(&w->disc[a.disc_slot], s);
    if (st) atomicAdd(&w->tests[a.disc_slot], st);
    if (sb) atomicAdd(&w->boxes[a.disc_slot], sb);
    if (hs) atomicAdd(&w->disc[WF_SHADOW], hs);
    if (hst) { atomicAdd(&w->tests[WF_SHADOW], hst); atomicAdd(&w->sh_tests[a.disc_slot], hst); }
    if (hsb) atomicAdd(&w->boxes[WF_SHADOW], hsb);
    if (hr) atomicAdd(&w->sh_rays[a.disc_slot], hr);
  }
  if (a.count) {  // counted launch: shade_hit runs and children per generation (read_stats)
    const unsigned long long n1 = wave_sum(t.hits), n2 = wave_sum(t.refl), n3 = wave_sum(t.refr);
    if (lane_id() == 0) {
      if (n1) atomicAdd(&a.cnt->n_hit[a.g], (unsigned)n1);
      if (n2) atomicAdd(&a.cnt->n_refl[a.g], (unsigned)n2);
      if (n3) atomicAdd(&a.cnt->n_refr[a.g], (unsigned)n3);
    }
  }
