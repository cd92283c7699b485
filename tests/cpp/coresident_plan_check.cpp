// Host check of the co-resident launch shape in rt_wf_plan.hpp (tests/test_coresident_plan.py):
// for C3-sized scenes (1000 diagonal spheres, one light with a light buffer) whose four-wide LDS
// image runs from well under kFusedLdsLimit up to it, and for the pair image and the
// global-memory images, wf_plan_image grants form 1 (blocks of kTraceBlock - 64 threads) or form 2
// exactly when the CU's LDS still holds the combine's blocks beside the fused block:
//   alloc(dyn + static) + blocks x alloc(260) <= 160 KiB, alloc = whole allocation units,
// stated here on its own; every other plan keeps kTraceBlock threads. The image (lane, flags,
// treelet, dyn) and lane_lds_layout are the same whatever form is asked for. The pointers are
// dummies, never dereferenced.
#include <cstdio>
#include <cstring>

#include "rt_wf_plan.hpp"

using namespace rtamd;

static size_t up(size_t b, size_t unit) { return (b + unit - 1) / unit * unit; }
// the condition, from the issue's statement: both allocation units must leave the room
static bool fits(size_t dyn, size_t fused_static, int blocks) {
  for (size_t unit : {(size_t)1280, (size_t)512})
    if (up(dyn + fused_static, unit) + (size_t)blocks * up(260, unit) > (size_t)160 * 1024) return false;
  return true;
}

static int n_bad = 0;
#define CHECK(c, ...)                                   \
  do {                                                  \
    if (!(c)) {                                         \
      if (n_bad++ < 10) { std::printf("FAIL " __VA_ARGS__); std::printf("\n"); } \
    }                                                   \
  } while (0)

int main() {
  static_assert(kTraceBlock == 1024 && kTraceBlockCo == 960, "16 and 15 waves");
  static const LbCell cells[1] = {};
  static const BvhPair pair[1] = {};
  static const BvhWide wide[1] = {};
  static const BvhWide16 wide16[1] = {};
  static const BvhNode nodes[1] = {};
  static const SphereDiag sph[1] = {};
  long granted[3] = {}, refused[3] = {}, other_lane = 0, n_cases = 0;
  for (int wstack : {8, 12, 16})
  for (int n_bvhw = 100; n_bvhw <= 1400; ++n_bvhw)
  for (int ptrs : {1, 2, 3, 6, 7})
  for (int primary = 0; primary < 2; ++primary) {
    DevScene sc{};
    sc.sph_diag = sph;
    sc.bvh = nodes;
    sc.n_diag = 1000;
    sc.n_lights = 1;
    sc.lb_cells = cells;
    sc.bvh_depth = 12;
    sc.bvhw_stack = wstack;
    sc.n_bvh = 599;  // C3's binary hierarchy
    sc.n_bvhw = n_bvhw;
    sc.bvh_pair = (ptrs & 1) ? pair : nullptr;
    sc.bvhw = (ptrs & 2) ? wide : nullptr;
    sc.bvhw16 = (ptrs & 4) ? wide16 : nullptr;
    WfTuning tn;
    const WfImagePlan p0 = wf_plan_image(sc, tn, primary != 0, true);
    const WfImagePlan pd = wf_plan_image(sc, tn, primary != 0, true, 0);
    CHECK(p0.threads == kTraceBlock && p0.coresident == 0 && pd.threads == kTraceBlock && pd.coresident == 0,
          "form 0: threads %d form %d", p0.threads, p0.coresident);
    const LaneLdsLayout L0 = lane_lds_layout(p0.lane, sc, p0.lds_flags, p0.n_top);
    const size_t fused_static = lane_static_lds_bytes(p0.lane) + 528;  // s_pre and the placeholder, as the build reports
    for (int form = 1; form <= 2; ++form) {
      const WfImagePlan p = wf_plan_image(sc, tn, primary != 0, true, form);
      ++n_cases;
      // the image does not depend on the form
      CHECK(p.lane == p0.lane && p.lds_flags == p0.lds_flags && p.n_top == p0.n_top && p.dyn == p0.dyn,
            "form %d changed the image: lane %d/%d dyn %zu/%zu", form, p.lane, p0.lane, p.dyn, p0.dyn);
      const LaneLdsLayout L = lane_lds_layout(p.lane, sc, p.lds_flags, p.n_top);
      CHECK(std::memcmp(&L, &L0, sizeof L) == 0, "form %d changed the layout", form);
      // the stack region keeps the kTraceBlock stride: 16-bit entries x bvhw_stack (or depth + 1) x 1024
      if (p.lane == kLaneWideLds) CHECK(L.nodes - L.stack == (size_t)wstack * 1024 * 2, "stack region %zu", L.nodes - L.stack);
      // only the four-wide LDS image takes the shape; the pair image and the global-memory images never do
      const bool want = p.lane == kLaneWideLds && fits(p.dyn, fused_static, form == 1 ? 2 : 4);
      if (p.lane != kLaneWideLds) ++other_lane;
      if (p.lane == kLaneWideLds) ++(want ? granted : refused)[form];  // (the LDS condition alone decides these)
      CHECK((p.coresident == form) == want && (p.coresident == 0 || p.coresident == form),
            "form %d lane %d dyn %zu: granted %d, the LDS condition says %d", form, p.lane, p.dyn, p.coresident, (int)want);
      CHECK(p.threads == (p.coresident == 1 ? kTraceBlockCo : kTraceBlock), "form %d ran %d: threads %d", form,
            p.coresident, p.threads);
      CHECK(p.dyn + lane_static_lds_bytes(p.lane) <= kFusedLdsLimit, "dyn %zu past the limit", p.dyn);
    }
  }
  // the sweep saw both outcomes of both forms, and plans over the other images
  for (int form = 1; form <= 2; ++form)
    CHECK(granted[form] > 0 && refused[form] > 0, "form %d: granted %ld refused %ld", form, granted[form], refused[form]);
  CHECK(other_lane > 0, "no plan over another image");
  // the edges of the condition themselves (four-wide image, no static stack): the last dyn that
  // fits and the first that does not
  CHECK(fits(163840 - 2 * 1280 - 528, 528, 2) && !fits(163840 - 2 * 1280 - 528 + 1, 528, 2), "edge of form 1");
  CHECK(coresident_lds_fits(kLaneWideLds, 163840 - 2 * 1280 - 528, 2) &&
            !coresident_lds_fits(kLaneWideLds, 163840 - 2 * 1280 - 528 + 1, 2),
        "edge of form 1 (the plan's)");
  CHECK(coresident_lds_fits(kLaneWideLds, 163840 - 4 * 1280 - 528, 4) &&
            !coresident_lds_fits(kLaneWideLds, 163840 - 4 * 1280 - 528 + 1, 4),
        "edge of form 2 (the plan's)");
  if (n_bad) return 1;
  std::printf("OK %ld cases; form 1 granted %ld refused %ld; form 2 granted %ld refused %ld; other images %ld\n", n_cases,
              granted[1], refused[1], granted[2], refused[2], other_lane);
  return 0;
}
