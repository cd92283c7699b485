// Host check of rt_wf_plan.hpp (tests/test_image_plan.py): wf_plan_image and
// lane_lds_layout against `old_rules`, the decision launch_fused_q made inline
// before the plan existed (with the size functions it used), and against
// `staged_bytes`, the bytes each image's stage (rt_trace.hpp LaneImage, which
// takes its offsets from lane_lds_layout) writes into a region. A sweep of
// synthetic scenes (the pointers are dummies, never dereferenced) on both sides
// of every threshold; the outcomes are counted, so a sweep that stops reaching
// a lane or a flag fails.
#include <cstdio>

#include "rt_wf_plan.hpp"

using namespace rtamd;

// ---- the old rules: launch_fused_q's body, reduced to what it decided
namespace old {
constexpr size_t kWfLdsLimit = 160 * 1024 - 1024;
constexpr int kTraceBlock = 1024;
// (function objects: a call with a DevScene must not find rt_wf_plan.hpp's functions of the same names)
const auto lane_stack_bytes = [](int depth) -> size_t { return (size_t)(depth > 0 ? depth : 1) * kTraceBlock * 4; };
const auto sph_lds_bytes = [](const DevScene& sc) -> size_t { return (size_t)sc.n_diag * sizeof(SphereDiag); };
const auto sph48_lds_bytes = [](const DevScene& sc) -> size_t {
  return (size_t)sc.n_diag * 48 + (((size_t)sc.n_diag * 4 + 15) & ~(size_t)15);
};
const auto delta_lds_bytes = [](const DevScene& sc) -> size_t {
  return sc.lb_cells ? (((size_t)sc.n_lights * sc.n_diag * 2 /* sizeof(_Float16) */ + 15) & ~(size_t)15) : 0;
};
const auto pair_lds_bytes = [](const DevScene& sc) -> size_t {
  if (!sc.bvh_pair) return (size_t)1 << 40;
  return ((lane_stack_bytes(sc.bvh_depth + 1) / 2 + 15) & ~(size_t)15) + (size_t)sc.n_bvh * sizeof(BvhNode) +
         sph48_lds_bytes(sc);
};
const auto wide_stack_bytes = [](const DevScene& sc) -> size_t {
  return ((size_t)(sc.bvhw_stack > 0 ? sc.bvhw_stack : 1) * kTraceBlock * 2 + 15) & ~(size_t)15;
};
const auto wide_lds_bytes = [](const DevScene& sc) -> size_t {
  if (!sc.bvhw) return (size_t)1 << 40;
  return wide_stack_bytes(sc) + (size_t)sc.n_bvhw * sizeof(BvhWide) + sph48_lds_bytes(sc);
};
constexpr unsigned kLdsSpheres = 1u, kLdsDeltas = 2u;

struct A {
  unsigned use_lb, lds_flags, n_top;
};
static WfImagePlan done(int lane, const A& a, size_t dyn) {
  WfImagePlan p;
  p.lane = lane; p.lds_flags = a.lds_flags; p.n_top = a.n_top; p.dyn = dyn;
  return p;
}
static WfImagePlan rules(const DevScene& sc, const WfTuning& tn, bool primary, bool use_lb) {
  A a{use_lb ? 1u : 0u, 0u, 0u};
  const size_t dl = a.use_lb ? delta_lds_bytes(sc) : 0;
  size_t dyn = 0;
  a.lds_flags = 0;
  const bool wide_ok = tn.image != 1 && tn.wide && sc.bvhw16 && wide_stack_bytes(sc) <= kWfLdsLimit / 2;
  const bool wide_lds = sc.bvhw && tn.lds_wide && wide_lds_bytes(sc) + dl <= kWfLdsLimit;
  const bool lds_img = tn.image == 0 && (pair_lds_bytes(sc) <= kWfLdsLimit || wide_lds);
  const bool lane_prim = tn.prim_lane == 1 ? (lds_img || wide_ok) : tn.prim_lane == 2 ? lds_img : false;
  if (primary && !lane_prim) {
    const size_t room = kWfLdsLimit - (size_t)(kTraceBlock / 64) * (kBvhMaxDepth + 4) * 4;
    if (sph_lds_bytes(sc) <= room) { a.lds_flags |= kLdsSpheres; dyn += sph_lds_bytes(sc); }
    if (dl && dyn + dl <= room) { a.lds_flags |= kLdsDeltas; dyn += dl; }
    return done(0, a, dyn);
  }
  if (tn.image == 0 && wide_lds) {
    dyn = wide_lds_bytes(sc);
    if (dl) { a.lds_flags |= kLdsDeltas; dyn += dl; }
    return done(15, a, dyn);
  }
  if (tn.image == 0 && pair_lds_bytes(sc) <= kWfLdsLimit) {
    dyn = pair_lds_bytes(sc);
    if (dl && dyn + dl <= kWfLdsLimit) {
      a.lds_flags |= kLdsDeltas;
      dyn += dl;
    }
    return done(14, a, dyn);
  }
  if (wide_ok) {
    const size_t room = kWfLdsLimit - wide_stack_bytes(sc);
    dyn = wide_stack_bytes(sc);
    if (dl && dl <= room && (!tn.treelet || tn.treelet_deltas)) { a.lds_flags |= kLdsDeltas; dyn += dl; }
    if (tn.treelet) {
      a.n_top = (unsigned)std::min<size_t>((size_t)sc.n_bvhw, (kWfLdsLimit - dyn) / sizeof(BvhWide16));
      dyn += (size_t)a.n_top * sizeof(BvhWide16);
    }
    return done(4, a, dyn);
  }
  if (tn.image != 1 && sc.bvh_depth <= kLaneLdsDepth) {
    const size_t room = kWfLdsLimit - (size_t)kLaneLdsDepth * kTraceBlock * 4;
    const bool deltas = dl && dl <= room && (!tn.treelet || tn.treelet_deltas);
    if (deltas) { a.lds_flags |= kLdsDeltas; dyn = dl; }
    if (tn.treelet) {
      a.n_top = (unsigned)std::min<size_t>((size_t)sc.n_bvh, (room - dyn) / sizeof(BvhNode));
      dyn += (size_t)a.n_top * sizeof(BvhNode);
    }
    return done(3, a, dyn);
  }
  if (dl && dl <= kWfLdsLimit) { a.lds_flags |= kLdsDeltas; dyn = dl; }
  return done(1, a, dyn);
}
// the kernel's static LDS, as its declaration of stack_lds had it (the other lanes' one-int
// placeholder is never referenced and takes no LDS)
static size_t static_lds(int lane) {
  return lane == 3 ? (size_t)kLaneLdsDepth * kTraceBlock * 4 : lane == 0 ? (size_t)(kTraceBlock / 64) * (kBvhMaxDepth + 4) * 4 : 0;
}
}  // namespace old

// ---- the bytes each LaneImage<LANE>::stage (rt_trace.hpp) writes into a region, or the stack's
// walks touch: the regions start at the layout's offsets by construction (stage takes them from
// lane_lds_layout), so what is left to hold is that each ends at or before the next one's offset.
// (-1: not staged. The 16-bit stacks: entry k of lane t at halfword k * kTraceBlock + t.)
struct Staged {
  long stack = -1, nodes = -1, sph48 = -1, sph = -1, deltas = -1, treelet = -1;
};
static Staged staged_bytes(int lane, const DevScene& sc, unsigned lds_flags, unsigned n_top) {
  Staged w;
  const long sph48 = (long)sc.n_diag * 48 + (long)sc.n_diag * 4;  // stage_sph48: r[i], i < 3 n_diag (16 B each); mt[k]
  if (lane == kLaneWideLds) {
    w.stack = (long)sc.bvhw_stack * kTraceBlock * 2;
    w.nodes = (long)sc.n_bvhw * (long)sizeof(BvhWide);
    w.sph48 = sph48;
  }
  if (lane == kLaneWide16) {
    w.stack = (long)sc.bvhw_stack * kTraceBlock * 2;
    w.treelet = (long)n_top * (long)sizeof(BvhWide16);
  }
  if (lane == kLanePair) {
    w.stack = (long)(sc.bvh_depth + 1) * kTraceBlock * 2;
    w.nodes = (long)sc.n_bvh * (long)sizeof(BvhPair);
    w.sph48 = sph48;
  }
  if (lane == kLaneWave && (lds_flags & kLdsSpheres)) w.sph = (long)sc.n_diag * (long)sizeof(SphereDiag);
  if (lane == kLaneLdsStack) w.treelet = (long)n_top * (long)sizeof(BvhNode);
  if (lds_flags & kLdsDeltas) w.deltas = (long)sc.n_lights * sc.n_diag * 2;  // stage_shared
  return w;
}

static int n_bad = 0;
static void fail(const char* what, const DevScene& sc, const WfTuning& tn, bool primary, bool use_lb,
                 const WfImagePlan& p, const WfImagePlan& o) {
  if (n_bad++ < 10)
    std::printf("FAIL %s: n_diag %d lights %d lb %d depth %d wstack %d n_bvh %d n_bvhw %d pair %d bvhw %d bvhw16 %d | image %d "
                "wide %d lds_wide %d treelet %d treelet_deltas %d prim_lane %d | primary %d use_lb %d | plan %d %u %u %zu "
                "old %d %u %u %zu\n",
                what, sc.n_diag, sc.n_lights, sc.lb_cells != nullptr, sc.bvh_depth, sc.bvhw_stack, sc.n_bvh, sc.n_bvhw,
                sc.bvh_pair != nullptr, sc.bvhw != nullptr, sc.bvhw16 != nullptr, tn.image, tn.wide, tn.lds_wide, tn.treelet,
                tn.treelet_deltas, tn.prim_lane, (int)primary, (int)use_lb, p.lane, p.lds_flags, p.n_top, p.dyn, o.lane,
                o.lds_flags, o.n_top, o.dyn);
}

int main() {
  static_assert(kLaneWave == 0 && kLaneScratch == 1 && kLaneLdsStack == 3 && kLaneWide16 == 4 && kLanePair == 14 &&
                    kLaneWideLds == 15,
                "the lanes are wf_trace_fused's template arguments");
  static_assert(kFusedLdsLimit == old::kWfLdsLimit && kTraceBlock == old::kTraceBlock, "limits");
  // dummy non-null pointers
  static const LbCell cells[1] = {};
  static const BvhPair pair[1] = {};
  static const BvhWide wide[1] = {};
  static const BvhWide16 wide16[1] = {};
  static const BvhNode nodes[1] = {};
  static const SphereDiag sph[1] = {};

  // outcomes: [lane][primary], flags and treelets set / unset
  long n_lane[16][2] = {}, n_sph[2] = {}, n_del[2] = {}, n_top[2] = {}, n_cases = 0;
  const int diags[] = {0, 1, 250, 1000, 1400, 1600, 1800, 2500, 3000, 9996};
  // nodes per sphere record, binary and four-wide: what the builder gives (C3: 599 binary nodes of
  // 1000 records), and sparser hierarchies, which put both LDS images' limit between 1800 and 3000
  const int dens[2][4] = {{3, 5, 2, 5}, {1, 4, 1, 5}};
  for (const int* dn : dens)
  for (int n_diag : diags)
  for (int n_lights : {1, 2, 16})
  for (int lb = 0; lb < 2; ++lb)
  for (int depth : {5, 16, 17, 30})
  for (int wstack : {4, 12, 40})
  for (int ptrs = 0; ptrs < 8; ++ptrs) {
    DevScene sc{};
    sc.sph_diag = sph;
    sc.bvh = nodes;
    sc.n_diag = n_diag;
    sc.n_lights = n_lights;
    sc.lb_cells = lb ? cells : nullptr;
    sc.bvh_depth = depth;
    sc.bvhw_stack = wstack;
    sc.n_bvh = n_diag > 1 ? std::max(1, n_diag * dn[0] / dn[1]) : n_diag;
    sc.n_bvhw = n_diag > 1 ? std::max(1, n_diag * dn[2] / dn[3]) : n_diag;
    sc.bvh_pair = (ptrs & 1) ? pair : nullptr;
    sc.bvhw = (ptrs & 2) ? wide : nullptr;
    sc.bvhw16 = (ptrs & 4) ? wide16 : nullptr;
    for (int image : {0, 1, 3})
    for (int knobs = 0; knobs < 32; ++knobs)
    for (int prim_lane = 0; prim_lane < 3; ++prim_lane)
    for (int primary = 0; primary < 2; ++primary) {
      WfTuning tn;
      tn.image = image;
      tn.wide = knobs & 1; tn.lds_wide = (knobs >> 1) & 1; tn.treelet = (knobs >> 2) & 1;
      tn.treelet_deltas = (knobs >> 3) & 1; tn.shadow_lb = (knobs >> 4) & 1;
      tn.prim_lane = prim_lane;
      const bool use_lb = tn.shadow_lb && sc.lb_cells;  // as render_fast sets WfArgs::use_lb
      const WfImagePlan p = wf_plan_image(sc, tn, primary != 0, use_lb);
      const WfImagePlan o = old::rules(sc, tn, primary != 0, use_lb);
      ++n_cases;
      if (p.lane != o.lane || p.lds_flags != o.lds_flags || p.n_top != o.n_top || p.dyn != o.dyn) {
        fail("plan != old rules", sc, tn, primary, use_lb, p, o);
        continue;
      }
      const LaneLdsLayout L = lane_lds_layout(p.lane, sc, p.lds_flags, p.n_top);
      if (p.dyn != L.end) fail("dyn != layout end", sc, tn, primary, use_lb, p, o);
      if (lane_static_lds_bytes(p.lane) != old::static_lds(p.lane) || p.dyn + lane_static_lds_bytes(p.lane) > kFusedLdsLimit)
        fail("static + dynamic LDS past the limit", sc, tn, primary, use_lb, p, o);
      // the regions: in order, 16-B aligned, none overlapping the next
      const size_t off[7] = {L.stack, L.nodes, L.sph48, L.sph, L.deltas, L.treelet, L.end};
      bool ok = L.stack == 0;
      for (int r = 0; r < 7; ++r) ok = ok && off[r] % 16 == 0 && (r == 0 || off[r - 1] <= off[r]);
      // ... and what the kernel stages there ends inside each region
      const Staged w = staged_bytes(p.lane, sc, p.lds_flags, p.n_top);
      const long reg[6] = {w.stack, w.nodes, w.sph48, w.sph, w.deltas, w.treelet};
      for (int r = 0; r < 6; ++r) ok = ok && (reg[r] < 0 || (long)off[r] + reg[r] <= (long)off[r + 1]);
      if (!ok) fail("layout regions", sc, tn, primary, use_lb, p, o);
      ++n_lane[p.lane][primary];
      if (p.lane == kLaneWave) ++n_sph[(p.lds_flags & kLdsSpheres) ? 1 : 0];
      ++n_del[(p.lds_flags & kLdsDeltas) ? 1 : 0];
      if (p.lane == kLaneWide16 || p.lane == kLaneLdsStack) ++n_top[p.n_top > 0 ? 1 : 0];
    }
  }
  // the sweep reached everything: every per-lane image for secondary launches; for primary ones
  // the wave traversal (and no other launch takes it) or, through prim_lane, the LDS and four-wide
  // images (never the binary global-memory ones); every flag and the treelet on and off
  for (int lane : {kLaneWave, kLaneScratch, kLaneLdsStack, kLaneWide16, kLanePair, kLaneWideLds})
    for (int primary = 0; primary < 2; ++primary) {
      const bool serves = primary ? lane != kLaneScratch && lane != kLaneLdsStack : lane != kLaneWave;
      if ((n_lane[lane][primary] != 0) != serves) {
        std::printf("FAIL lane %d primary %d: %ld plans\n", lane, primary, n_lane[lane][primary]);
        ++n_bad;
      }
    }
  for (int v = 0; v < 2; ++v)
    if (n_sph[v] == 0 || n_del[v] == 0 || n_top[v] == 0) {
      std::printf("FAIL outcome %d never seen: spheres %ld, distances %ld, treelet %ld\n", v, n_sph[v], n_del[v], n_top[v]);
      ++n_bad;
    }
  if (n_bad) return 1;
  std::printf("OK %ld cases; plans per lane (secondary/primary): 0 %ld/%ld, 1 %ld/%ld, 3 %ld/%ld, 4 %ld/%ld, 14 %ld/%ld, "
              "15 %ld/%ld\n",
              n_cases, n_lane[0][0], n_lane[0][1], n_lane[1][0], n_lane[1][1], n_lane[3][0], n_lane[3][1], n_lane[4][0],
              n_lane[4][1], n_lane[14][0], n_lane[14][1], n_lane[15][0], n_lane[15][1]);
  return 0;
}
