// rt_wf_plan.hpp — which scene image a fused launch of the fast path runs over
// (wf_trace_fused's LANE), how its block's dynamic LDS is laid out, and the
// launch's shape (threads per block, the co-resident form). The host takes
// them from here (launch_fused_q asks for WfImagePlan::dyn bytes and threads),
// and so does the kernel: each image's stage (rt_trace.hpp LaneImage) takes its
// region offsets from lane_lds_layout; tests/cpp/plan_check.cpp holds the bytes
// a stage writes into a region to the region's size.
// Plain C++: a host compiler builds it with only the HIP headers on the include
// path, so no device builtins and no _Float16 here (a binary16 value is 2 bytes).
#pragma once
#include <stddef.h>

#include <algorithm>

#include "rt_layout.hpp"
#include "rt_wavefront.hpp"

namespace rtamd {

constexpr int kTraceBlock = 1024;  // trace kernels: 16 waves, one LDS image per block
// LDS a fused trace launch may take (of the CU's 160 KB)
constexpr size_t kFusedLdsLimit = 160 * 1024 - 1024;

// The co-resident launch shape (WfTuning::coresident). A fused block over an LDS
// image holds its CU's LDS, and its 16 waves of up to 128 registers every SIMD's register file,
// so no wave of another pass's combine fits beside it. Form 1 launches blocks of kTraceBlockCo
// threads: 15 waves, one SIMD of each CU at three, 128 registers per lane free there for
// kCoBlocksA one-wave combine blocks of at most 64. Form 2 keeps 16 waves of at most
// kCoCapVgprs registers, 32 free on every SIMD for kCoBlocksB combine blocks of at most 32.
// The LDS stacks keep their kTraceBlock stride either way (a block of fewer threads leaves
// the last columns unused), so lane_lds_layout does not depend on the form.
constexpr int kTraceBlockCo = kTraceBlock - 64;
constexpr int kCoBlocksA = 2, kCoBlocksB = 4, kCoCapVgprs = 120;
constexpr size_t kCuLdsBytes = 160 * 1024;
constexpr size_t kFusedPrefixLds = 528;    // wf_trace_fused's s_pre (and stack_lds's placeholder), as reported
constexpr size_t kCombineStaticLds = 260;  // wf_combine_parents' s_pre[kPreList]
// What a block's LDS takes of the CU's: whole allocation units. gfx950 hands its 160 KiB out
// in units of 320 words; the 128-word unit of the smaller LDS is held too.
constexpr size_t lds_alloc_bytes(size_t b) {
  const size_t u = (b + 1279) / 1280 * 1280, v = (b + 511) / 512 * 512;
  return u > v ? u : v;
}

// wf_trace_fused's LANE (the values are the template arguments):
constexpr int kLaneWave = 0;      // wave traversal for primary rays (shared-origin records)
constexpr int kLaneScratch = 1;   // binary nodes in global memory, scratch stack
constexpr int kLaneLdsStack = 3;  // binary nodes in global memory, LDS stack and treelet
constexpr int kLaneWide16 = 4;    // four-wide binary16 nodes in global memory, with an LDS treelet
constexpr int kLanePair = 14;     // pair layout in LDS
constexpr int kLaneWideLds = 15;  // four-wide hierarchy and 48-B sphere records in LDS

constexpr unsigned kLdsSpheres = 1u, kLdsDeltas = 2u;  // lds_flags (kLaneWave: sphere records; all: distances)

// The kernel's static LDS array (stack_lds): the per-lane stack of
// kLaneLdsStack, the per-wave stacks of kLaneWave; the other lanes keep none
// (their one-int placeholder is never referenced and takes no LDS). Every
// lane's queue prefix (s_pre, 528 B) comes out of kFusedLdsLimit's 1-KB margin.
constexpr size_t lane_static_lds_bytes(int lane) {
  return lane == kLaneLdsStack ? (size_t)kLaneLdsDepth * kTraceBlock * 4
         : lane == kLaneWave   ? (size_t)(kTraceBlock / 64) * (kBvhMaxDepth + 4) * 4
                               : 0;
}

__host__ __device__ inline size_t lane_stack_bytes(int depth) { return (size_t)(depth > 0 ? depth : 1) * kTraceBlock * 4; }
__host__ __device__ inline size_t sph_lds_bytes(const DevScene& sc) { return (size_t)sc.n_diag * sizeof(SphereDiag); }
// the LDS images' sphere records: 48 B each, then the metas (Sph48)
__host__ __device__ inline size_t sph48_lds_bytes(const DevScene& sc) {
  return (size_t)sc.n_diag * 48 + (((size_t)sc.n_diag * 4 + 15) & ~(size_t)15);
}
// The light buffer's distances in LDS as binary16 lower bounds of the binary32
// ones (2 B each): a stored value never exceeds the true distance, so a walk
// that stops at the first stored distance beyond the origin stops no earlier
// than the exact walk would (lb_walk).
__host__ __device__ inline size_t delta_lds_bytes(const DevScene& sc) {
  return sc.lb_cells ? (((size_t)sc.n_lights * sc.n_diag * 2 + 15) & ~(size_t)15) : 0;
}
// kLanePair: the 16-bit stack (bvh_depth + 1 with the sentinel) x kTraceBlock
__host__ __device__ inline size_t pair_stack_bytes(const DevScene& sc) {
  return (lane_stack_bytes(sc.bvh_depth + 1) / 2 + 15) & ~(size_t)15;
}
// kLaneWide16, kLaneWideLds: the 16-bit stack (sc.bvhw_stack entries) x kTraceBlock
__host__ __device__ inline size_t wide_stack_bytes(const DevScene& sc) {
  return ((size_t)(sc.bvhw_stack > 0 ? sc.bvhw_stack : 1) * kTraceBlock * 2 + 15) & ~(size_t)15;
}

// The dynamic LDS of a block, as byte offsets. Every lane keeps this order; a
// region the lane (or lds_flags, or n_top = 0) leaves out is empty:
//   stack    the per-lane 16-bit stack            kLanePair, kLaneWide16, kLaneWideLds
//   nodes    every node of the hierarchy          kLanePair (BvhPair), kLaneWideLds (BvhWide)
//   sph48    the 48-B sphere records and metas    kLanePair, kLaneWideLds
//   sph      the SphereDiag records               kLaneWave with kLdsSpheres
//   deltas   the light buffer's distances         any lane with kLdsDeltas
//   treelet  the first n_top nodes                kLaneLdsStack (BvhNode), kLaneWide16 (BvhWide16)
// `end` is the dynamic LDS the launch asks for.
struct LaneLdsLayout {
  size_t stack, nodes, sph48, sph, deltas, treelet, end;
};
__host__ __device__ inline LaneLdsLayout lane_lds_layout(int lane, const DevScene& sc, unsigned lds_flags,
                                                         unsigned n_top) {
  const bool lds_img = lane == kLanePair || lane == kLaneWideLds;
  LaneLdsLayout l{};
  size_t p = 0;
  l.stack = p;
  p += lane == kLanePair ? pair_stack_bytes(sc) : lane == kLaneWide16 || lane == kLaneWideLds ? wide_stack_bytes(sc) : 0;
  l.nodes = p;
  p += lane == kLanePair      ? (size_t)sc.n_bvh * sizeof(BvhPair)
       : lane == kLaneWideLds ? (size_t)sc.n_bvhw * sizeof(BvhWide)
                              : 0;
  l.sph48 = p;
  p += lds_img ? sph48_lds_bytes(sc) : 0;
  l.sph = p;
  p += lane == kLaneWave && (lds_flags & kLdsSpheres) ? sph_lds_bytes(sc) : 0;
  l.deltas = p;
  p += (lds_flags & kLdsDeltas) ? delta_lds_bytes(sc) : 0;
  l.treelet = p;
  p += (size_t)n_top * (lane == kLaneLdsStack ? sizeof(BvhNode) : lane == kLaneWide16 ? sizeof(BvhWide16) : 0);
  l.end = p;
  return l;
}
// The whole LDS images, before the distances (no pair image without the scene's
// 16-bit pair codes, rt_bvh.cpp pair_layout; no wide one without its nodes)
__host__ __device__ inline size_t pair_lds_bytes(const DevScene& sc) {
  return sc.bvh_pair ? lane_lds_layout(kLanePair, sc, 0, 0).end : (size_t)1 << 40;
}
__host__ __device__ inline size_t wide_lds_bytes(const DevScene& sc) {
  return sc.bvhw ? lane_lds_layout(kLaneWideLds, sc, 0, 0).end : (size_t)1 << 40;
}

// rt_scene.cpp's estimate of the pair image, from which it chooses the leaf
// size before the layouts exist: a scene whose estimate passes kFusedLdsLimit
// gets single-sphere leaves. NOT pair_lds_bytes (a 4-byte stack entry, 64-B
// sphere records, no sentinel): changing it changes which scenes get which
// leaves, a measured change of its own.
inline size_t pair_image_leaf_estimate(int bvh_depth, size_t n_nodes, size_t n_diag) {
  return (size_t)(bvh_depth + 1) * kTraceBlock * 4 + n_nodes * sizeof(BvhNode) + n_diag * sizeof(SphereDiag);
}

// The image of one fused launch: generation 0 of a camera render (`primary`)
// or any other, with shadow rays through the light buffer (`use_lb`) or not.
//   kLaneWideLds  image 0, lds_wide, and the whole four-wide image fits beside the distances (C3)
//   kLanePair     image 0 and the pair image fits; the distances take what room is left
//   kLaneWide16   image 0 or 3, wide, and the scene has the binary16 nodes (C5)
//   kLaneLdsStack image 0 or 3 and the tree is at most kLaneLdsDepth deep
//   kLaneScratch  everything else
// The global-memory images stage the distances and/or a treelet of their top
// nodes in the room their stack leaves (the treelet alone unless treelet_deltas).
// Primary rays take the wave traversal unless prim_lane sends them over the
// per-lane image too: 1 (default) = over any LDS or four-wide image (C3 primary
// class 0.128 -> 0.125 ms/frame with the LDS four-wide image; C5's global
// image: 2.06 -> 2.16 ms with binary32 nodes, 2.17 -> 2.01 ms with the
// binary16 ones), 2 = over the LDS images only.
//
// `coresident`: the form the launch may take (the caller's: WfTuning::coresident for a pass with
// others in flight, and for form 2 only where the launch's kernel has the capped twin; else 0).
// The plan grants it to the four-wide LDS image (kLaneWideLds, the image the shape was measured
// on) when the CU's LDS still holds the combine's blocks beside the fused block:
//   alloc(dyn + static) + blocks x alloc(the combine's static) <= 160 KiB
// and falls back to the usual shape (threads = kTraceBlock, coresident = 0) otherwise.
constexpr bool coresident_lds_fits(int lane, size_t dyn, int blocks) {
  return lds_alloc_bytes(dyn + lane_static_lds_bytes(lane) + kFusedPrefixLds) +
             (size_t)blocks * lds_alloc_bytes(kCombineStaticLds) <= kCuLdsBytes;
}
inline WfImagePlan wf_plan_image(const DevScene& sc, const WfTuning& tn, bool primary, bool use_lb,
                                 int coresident = 0) {
  const size_t dl = use_lb ? delta_lds_bytes(sc) : 0;
  const bool wide_ok = tn.image != 1 && tn.wide && sc.bvhw16 && wide_stack_bytes(sc) <= kFusedLdsLimit / 2;
  const bool wide_lds = tn.image == 0 && sc.bvhw && tn.lds_wide && wide_lds_bytes(sc) + dl <= kFusedLdsLimit;
  const bool pair_lds = tn.image == 0 && pair_lds_bytes(sc) <= kFusedLdsLimit;
  const bool lds_img = wide_lds || pair_lds;
  const bool lane_prim = tn.prim_lane == 1 ? (lds_img || wide_ok) : tn.prim_lane == 2 ? lds_img : false;
  WfImagePlan p;
  p.lane = primary && !lane_prim                              ? kLaneWave
           : wide_lds                                         ? kLaneWideLds
           : pair_lds                                         ? kLanePair
           : wide_ok                                          ? kLaneWide16
           : tn.image != 1 && sc.bvh_depth <= kLaneLdsDepth ? kLaneLdsStack
                                                              : kLaneScratch;
  const size_t room = kFusedLdsLimit - lane_static_lds_bytes(p.lane);
  auto used = [&] { return lane_lds_layout(p.lane, sc, p.lds_flags, p.n_top).end; };
  if (p.lane == kLaneWave && sph_lds_bytes(sc) <= room) p.lds_flags |= kLdsSpheres;
  const bool treelet = (p.lane == kLaneWide16 || p.lane == kLaneLdsStack) && tn.treelet;
  if (dl && used() + dl <= room && (!treelet || tn.treelet_deltas)) p.lds_flags |= kLdsDeltas;
  if (treelet) {
    const size_t n_nodes = p.lane == kLaneWide16 ? (size_t)sc.n_bvhw : (size_t)sc.n_bvh;
    p.n_top = (unsigned)std::min<size_t>(n_nodes, (room - used()) / 64);  // BvhNode and BvhWide16: 64 B
  }
  p.dyn = used();
  p.threads = kTraceBlock;
  if (p.lane == kLaneWideLds && coresident == 1 && coresident_lds_fits(p.lane, p.dyn, kCoBlocksA)) {
    p.threads = kTraceBlockCo;
    p.coresident = 1;
  } else if (p.lane == kLaneWideLds && coresident == 2 && coresident_lds_fits(p.lane, p.dyn, kCoBlocksB)) {
    p.coresident = 2;
  }
  return p;
}
static_assert(sizeof(BvhNode) == 64 && sizeof(BvhWide16) == 64, "wf_plan_image: a treelet node is 64 B");

}  // namespace rtamd
