// rt_wavefront_glb.hip — the fast path's launches over the global-memory
// scene images (LANE 3: the treelet and the stack in LDS; LANE 1: the stack in
// scratch; LANE 4: the four-wide global image). Its own code object, compiled
// without the AMDGPU register-pressure trackers (Makefile), which help the LDS
// image (C3) and cost the global images (C5) ~2 %.
#include "rt_wf_launch.hpp"

#pragma clang fp contract(off)

namespace rtamd {

template <int LANE>
static hipError_t launch_glb_lane(bool quads, bool tris, bool csg, bool alias, bool runs, bool tally, bool cam_rays, const DevScene& sc, const DevCamera& cam,
                                  const WfArgs& a, size_t dyn, unsigned n, hipStream_t stream, int block, hipEvent_t e0,
                                  hipEvent_t e1) {
#define RT_GLB(Q, T, C) wf_launch(wf_trace_fused<false, Q, LANE, T, C>, block, dyn, n, stream, e0, e1, sc, cam, a)
#define RT_GLB_TRI(T, C) wf_launch(wf_trace_fused<false, true, LANE, T, C, true>, block, dyn, n, stream, e0, e1, sc, cam, a)
#define RT_GLB_RUNS(T, C, A) wf_launch(wf_trace_fused<false, true, LANE, T, C, true, true, A, true>, block, dyn, n, stream, e0, e1, sc, cam, a)
  if (runs && alias) {  // a scene with a run hierarchy, in a render that walks it
    if (cam_rays) return tally ? RT_GLB_RUNS(true, true, true) : RT_GLB_RUNS(false, true, true);
    return tally ? RT_GLB_RUNS(true, false, true) : RT_GLB_RUNS(false, false, true);
  }
  if (runs) {
    if (cam_rays) return tally ? RT_GLB_RUNS(true, true, false) : RT_GLB_RUNS(false, true, false);
    return tally ? RT_GLB_RUNS(true, false, false) : RT_GLB_RUNS(false, false, false);
  }
#undef RT_GLB_RUNS
#define RT_GLB_CSG(T, C) wf_launch(wf_trace_fused<false, true, LANE, T, C, true, true>, block, dyn, n, stream, e0, e1, sc, cam, a)
#define RT_GLB_ALIAS(T, C) wf_launch(wf_trace_fused<false, true, LANE, T, C, true, true, true>, block, dyn, n, stream, e0, e1, sc, cam, a)
  if (alias) {  // a scene with alias classes: the Csg kernels with the classes' loop
    if (cam_rays) return tally ? RT_GLB_ALIAS(true, true) : RT_GLB_ALIAS(false, true);
    return tally ? RT_GLB_ALIAS(true, false) : RT_GLB_ALIAS(false, false);
  }
#undef RT_GLB_ALIAS
  if (csg) {  // a scene with Csg units: the triangle kernels with the units' loop
    if (cam_rays) return tally ? RT_GLB_CSG(true, true) : RT_GLB_CSG(false, true);
    return tally ? RT_GLB_CSG(true, false) : RT_GLB_CSG(false, false);
  }
#undef RT_GLB_CSG
  if (tris) {  // a scene with triangles: the QUADS kernels with the triangle loop and walk
    if (cam_rays) return tally ? RT_GLB_TRI(true, true) : RT_GLB_TRI(false, true);
    return tally ? RT_GLB_TRI(true, false) : RT_GLB_TRI(false, false);
  }
  if (cam_rays) {
    if (quads) return tally ? RT_GLB(true, true, true) : RT_GLB(true, false, true);
    return tally ? RT_GLB(false, true, true) : RT_GLB(false, false, true);
  }
  if (quads) return tally ? RT_GLB(true, true, false) : RT_GLB(true, false, false);
  return tally ? RT_GLB(false, true, false) : RT_GLB(false, false, false);
#undef RT_GLB
#undef RT_GLB_TRI
}
hipError_t wf_launch_global(int lane, bool quads, bool tris, bool csg, bool alias, bool runs, bool tally, bool cam_rays, const DevScene& sc, const DevCamera& cam,
                            const WfArgs& a, size_t dyn, unsigned n, hipStream_t stream, int block, hipEvent_t e0,
                            hipEvent_t e1) {
#define RT_LANE(L) launch_glb_lane<L>(quads, tris, csg, alias, runs, tally, cam_rays, sc, cam, a, dyn, n, stream, block, e0, e1)
  if (lane == kLaneLdsStack) return RT_LANE(kLaneLdsStack);
  if (lane == kLaneScratch) return RT_LANE(kLaneScratch);
  if (lane == kLaneWide16) return RT_LANE(kLaneWide16);
#undef RT_LANE
  return hipErrorInvalidValue;
}

}  // namespace rtamd
