// rt_slab.hpp — the per-lane walks' binary32 slab test and the walk of a Csg
// unit's run hierarchy (rt_layout.hpp CsgRun) built from it.
//
// The kernels (rt_trace.hpp's walks, rt_device.hpp's streamed Csg evaluators) and a host compiler
// (tests/cpp/csg_run_check.cpp) build the same functions: `V` is any vector with double members
// x, y, z. Only the reciprocal differs: v_rcp_f32 on the device, a correctly rounded division on
// the host, both within the 1 ulp the bound below allows.
#pragma once
#include <math.h>
#include <stdint.h>

#include "rt_layout.hpp"

#if defined(__HIPCC__)
#define RT_SLAB_FN __device__ __forceinline__
#else
#define RT_SLAB_FN inline
#endif

namespace rtamd {

// The per-lane traversal's slab test runs in binary32 on an interval that is
// widened to contain the exact (real-arithmetic) one; DESIGN.md §5.2 has the
// error bound. Per ray and axis: inv = an approximate reciprocal of d in
// binary32 (slab_inv: relative error below 2^-22, exactly the value the FMAs
// use), and the plane constants c = o*inv -/+ delta with delta = 2^-20 |inv|
// (M + |o|), where M bounds every box coordinate on that axis (the root's
// children); the computed entry (exit) distance fma(corner, inv, -c) then
// never exceeds (falls short of) the exact one, (corner - o) / d: its error,
// the reciprocal's included, is below delta/3.
// An axis whose direction is (nearly) zero or whose origin is huge / NaN is
// not used for culling at all (interval (-inf, +inf)).
struct SlabRay {
  float inv[3], c_lo[3], c_hi[3];
};
// binary32 reciprocal of a binary64 direction component with 2^-60 <= |d|:
// (float)d rounds once (2^-24), v_rcp_f32 is within 1 ulp (2^-23); returned
// widened to binary64 (exact), the value every plane constant is built from.
#if defined(__HIPCC__)
RT_SLAB_FN double slab_inv(double d) { return (double)__builtin_amdgcn_rcpf((float)d); }
#else
RT_SLAB_FN double slab_inv(double d) { return (double)(1.0f / (float)d); }
#endif
// `grow` (other_trace's far origins): every box taken as that much larger on each axis, in world units.
template <typename V>
RT_SLAB_FN SlabRay slab_ray(V o, V d, const float* M, const double* grow = nullptr) {
  SlabRay r;
  const double oa[3] = {o.x, o.y, o.z}, da[3] = {d.x, d.y, d.z};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (fabs(da[a]) >= 0x1p-60 && fabs(oa[a]) <= 0x1p60 && M[a] <= 0x1p60f) {  // NaN fails
      const double inv = slab_inv(da[a]);
      const double oinv = oa[a] * inv;
      double delta = 0x1p-20 * fabs(inv) * ((double)M[a] + fabs(oa[a]));
      if (grow) delta = (delta + fabs(inv) * grow[a]) * (1.0 + 0x1p-20);
      const float on = (float)(oinv + delta), of = (float)(oinv - delta);
      r.inv[a] = (float)inv;
      r.c_lo[a] = inv >= 0.0 ? on : of;  // the lo plane is the entry plane when inv >= 0
      r.c_hi[a] = inv >= 0.0 ? of : on;
    } else {
      r.inv[a] = 0.0f;
      r.c_lo[a] = INFINITY;
      r.c_hi[a] = -INFINITY;
    }
  }
  return r;
}
// binary32 upper bound of a non-negative binary64 distance: RN(x) is within
// 2^-23 of x relative to it, and RN(f * (1 + 2^-22)) > f * (1 + 2^-23)
// (0 and inf map to themselves).
RT_SLAB_FN float f32_up(double x) { return (float)x * (1.0f + 0x1p-22f); }
// binary32 lower bound of a binary64 value of either sign (never NaN): RN(x), stepped down when it
// rounded up (-inf maps to itself).
RT_SLAB_FN float f32_below(double x) {
  const float f = (float)x;
  return (double)f > x ? nextafterf(f, -INFINITY) : f;
}
// max(entry, t_lo) <= min(exit, t_hi): the ray may meet the box within [t_lo, t_hi]
// (t_hi >= 0). `t_in` = the widened entry distance (child ordering only).
template <typename P>  // P: constant-address (scalar loads) or generic (per-lane loads) float pointer
RT_SLAB_FN bool slab_hit32(P lo, P hi, const SlabRay& r, float t_hi, float& t_in, float t_lo = 0.0f) {
  const float x0 = fmaf(lo[0], r.inv[0], -r.c_lo[0]), x1 = fmaf(hi[0], r.inv[0], -r.c_hi[0]);
  const float y0 = fmaf(lo[1], r.inv[1], -r.c_lo[1]), y1 = fmaf(hi[1], r.inv[1], -r.c_hi[1]);
  const float z0 = fmaf(lo[2], r.inv[2], -r.c_lo[2]), z1 = fmaf(hi[2], r.inv[2], -r.c_hi[2]);
  const float tmin = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fmaxf(fminf(z0, z1), t_lo));
  const float tmax = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fminf(fmaxf(z0, z1), t_hi));
  t_in = tmin;
  return tmin <= tmax;
}
// slab_ray's M of a hierarchy: the root's two child boxes contain every box below them.
template <typename P>  // P: constant-address or generic node pointer
RT_SLAB_FN void root_bound(P root, float M[3]) {
  for (int a = 0; a < 3; ++a)
    M[a] = fmaxf(fmaxf(fabsf(root->lo[0][a]), fabsf(root->hi[0][a])), fmaxf(fabsf(root->lo[1][a]), fabsf(root->hi[1][a])));
}

// ---- A Csg unit's run hierarchy (rt_layout.hpp CsgRun; DESIGN.md §5.2 "Csg units: run
// hierarchies"). The boxes hold, for every chained ray the run's bounds admit, the point of the
// chained ray at each root the reference's triangle arithmetic yields on it (rt_bvh.cpp tri_box
// with the run's bounds): a triangle whose box the line misses within [t_lo, t_hi] has no root
// there.
//
// The chained ray the padding was sized for: finite, |d|_inf <= dmax from |o|_inf <= omax. Any
// other one (a caller's own ray, a NaN) takes the run's ops one by one, as tri_trace's such rays
// test every record.
template <typename V>
RT_SLAB_FN bool csg_run_admits(const CsgRun& run, V co, V cd) {
  return fabs(cd.x) <= run.dmax && fabs(cd.y) <= run.dmax && fabs(cd.z) <= run.dmax && fabs(co.x) <= run.omax &&
         fabs(co.y) <= run.omax && fabs(co.z) <= run.omax;  // (a NaN fails; so does an infinity: the bounds are finite)
}
// One walk: visit(k) for record k of the run (csg_tris[run.first + k]): the remainder first (no
// box: every ray), then every boxed record under a leaf whose box the chained ray's line meets
// within [t_lo, t_hi], tri_trace's binary32 slabs. The interval is the caller's: t_hi = f32_up of
// the value its stop `t > h.t` compares against (it does not move during a walk), t_lo = -inf on a
// unit's first walk (radiance and shadow rays alike: the roots t < 0 move the filter bits that
// decide whether a root t >= 0 survives, so tri_trace's [0, distance) is wrong here), later the
// watermark's t rounded down: only roots above (wt, wk) can enter the batch.
// The visiting order is free: the keys are unique and csg_batch_insert keeps the kCsgListCap
// smallest entries above the watermark whatever order they come in, so the batch is the one the
// one-by-one ops make up to t_hi; `more` may differ only for roots beyond t_hi, where the
// evaluator stops anyway (tests/cpp/csg_run_check.cpp holds both).
template <typename V, typename Visit>
RT_SLAB_FN void csg_run_walk(const CsgRun& run, const BvhNode* nodes, V co, V cd, float t_lo, float t_hi, Visit visit) {
  for (int k = run.n_boxed; k < run.n; ++k) visit(k);
  float M[3];
  root_bound(nodes, M);
  const SlabRay sr = slab_ray(co, cd, M);
  int stk[kBvhMaxDepth + 4];
  int sp = 0, e = 0;
  while (e != kBvhEmpty) {
    const BvhNode& nd = nodes[e];
    int next[2], nn = 0;
    for (int c = 0; c < 2; ++c) {
      const int32_t code = nd.child[c];
      if (code == kBvhEmpty) continue;
      float t_in;
      if (!slab_hit32(nd.lo[c], nd.hi[c], sr, t_hi, t_in, t_lo)) continue;
      if (code >= 0) { next[nn++] = code; continue; }
      const int lc = -(code + 1), first = lc >> 7, cnt = lc & 127;
      for (int k = first; k < first + cnt; ++k) visit(k);
    }
    if (nn == 2) stk[sp++] = next[1];
    e = nn > 0 ? next[0] : (sp > 0 ? stk[--sp] : kBvhEmpty);
  }
}

}  // namespace rtamd
