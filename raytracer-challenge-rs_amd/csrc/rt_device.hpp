// rt_device.hpp — device-side building blocks of the render path, shared by
// the wavefront pipeline (rt_wavefront.hip) and the batch kernels
// (rt_kernels.hip). Every function restates a reference function (cited),
// in binary64 with the reference's operation order; include only from .hip
// files compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rt_csg.hpp"
#include "rt_layout.hpp"
#include "rt_pow.hpp"
#include "rt_slab.hpp"

#pragma clang fp contract(off)

namespace rtamd {

// --------------------------------------------------------------- vector math
// vector.rs / point.rs / color.rs, left-associative like the Rust expressions.
struct V3 {
  double x, y, z;
};
__device__ __forceinline__ V3 v3(double x, double y, double z) { return V3{x, y, z}; }
__device__ __forceinline__ V3 vadd(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 vsub(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 vneg(V3 a) { return v3(-a.x, -a.y, -a.z); }
__device__ __forceinline__ V3 vscale(V3 a, double s) { return v3(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ V3 vmul(V3 a, V3 b) { return v3(a.x * b.x, a.y * b.y, a.z * b.z); }
// vector.rs:99-101
__device__ __forceinline__ double vdot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
// vector.rs:21-28 (three divisions, not a reciprocal)
__device__ __forceinline__ V3 vnormalize(V3 a) {
  double m = sqrt(a.x * a.x + a.y * a.y + a.z * a.z);
  return v3(a.x / m, a.y / m, a.z / m);
}
// vector.rs:30-32: self - normal * 2.0 * dot(self, normal)
__device__ __forceinline__ V3 vreflect(V3 v, V3 n) { return vsub(v, vscale(vscale(n, 2.0), vdot(v, n))); }
// lib.rs:20-22
__device__ __forceinline__ bool req(double a, double b) { return fabs(a - b) < kEpsilon; }
// matrix.rs:232-245 (point, rows 0..2 with translation) and :247-260 (vector)
__device__ __forceinline__ V3 m34_point(const double* m, V3 p) {
  return v3(m[0] * p.x + m[1] * p.y + m[2] * p.z + m[3],
            m[4] * p.x + m[5] * p.y + m[6] * p.z + m[7],
            m[8] * p.x + m[9] * p.y + m[10] * p.z + m[11]);
}
__device__ __forceinline__ V3 m33_vector(const double* m, V3 v) {  // m: 3x3 row-major
  return v3(m[0] * v.x + m[1] * v.y + m[2] * v.z,
            m[3] * v.x + m[4] * v.y + m[5] * v.z,
            m[6] * v.x + m[7] * v.y + m[8] * v.z);
}

// Wave-uniform records through the constant address space -> s_load.
#define RT_CONST __attribute__((address_space(4)))
typedef const RT_CONST SphereDiag* cSphereDiag;
typedef const RT_CONST SphereGen* cSphereGen;
typedef const RT_CONST PlaneRec* cPlaneRec;
typedef const RT_CONST QuadRec* cQuadRec;
typedef const RT_CONST GroupRec* cGroupRec;
typedef const RT_CONST TriRec* cTriRec;
typedef const RT_CONST ConeCluster* cConeCluster;
typedef const RT_CONST LightRec* cLightRec;

typedef double d2 __attribute__((ext_vector_type(2)));  // ds_read_b128 operand
__host__ __device__ constexpr size_t lds_align16(size_t x) { return (x + 15) & ~(size_t)15; }

// ------------------------------------------------------------ trace (hot loop)
// World::intersect + intersections + hit (world.rs:31-38, intersection.rs:
// 108-125) without building or sorting the list: the nearest t >= 0 by
// (t, key) is the element the stable sort puts first, and the `containers`
// walk of prepare_computations (intersection.rs:63-90) only ever needs the two
// most recently entered containers (DESIGN.md "containers walk -> top-2").
struct Hit {
  double t;   // nearest t >= 0 (over eligible objects)
  int key;    // (object << kKeyShift) | list position, -1 = miss
  int hin;    // the hit object is in `containers` when the hit is reached
  // containers candidates (radiance rays): objects with an odd number of
  // intersections t < 0, keyed by their last such intersection; top 2.
  double c1t, c2t;
  int c1k, c2k;
};

__device__ __forceinline__ void hit_init(Hit& h) {
  h.t = INFINITY;
  h.key = 0x7fffffff;
  h.hin = 0;
  h.c1t = -INFINITY; h.c2t = -INFINITY; h.c1k = -1; h.c2k = -1;
}
__device__ __forceinline__ void hit_finish(Hit& h) {
  if (h.key == 0x7fffffff) h.key = -1;
}
__device__ __forceinline__ bool better(double t, int k, double bt, int bk) {
  return t < bt || (t == bt && k < bk);
}
__device__ __forceinline__ void push_container(Hit& h, double t, int k) {
  if (t > h.c1t || (t == h.c1t && k > h.c1k)) {
    h.c2t = h.c1t; h.c2k = h.c1k; h.c1t = t; h.c1k = k;
  } else if (t > h.c2t || (t == h.c2t && k > h.c2k)) {
    h.c2t = t; h.c2k = k;
  }
}

// Sphere::local_intersect (sphere.rs:47-62) from (a, dt = d.o, c) of the
// object-space ray. With b = 2*dt and disc = b*b - (4a)*c = 4*(dt*dt - a*c)
// exactly (power-of-two scaling commutes with rounding), t = (-b -/+
// sqrt(disc)) / (2a) equals (-dt -/+ sqrt(dt*dt - a*c)) / a bit for bit
// (DESIGN.md "Sphere roots"). The object index / shadow flag (`meta`) is read
// only when disc >= 0. Root 1 can only be the hit when root 0 < 0, i.e. when
// the sphere is a container at the hit.
template <bool SHADOW, typename MetaFn>
__device__ __forceinline__ void sphere_adc(double a, double dt, double c, MetaFn meta_fn, Hit& h,
                                           unsigned& n_disc) {
  const double disc = dt * dt - a * c;
  if (disc >= 0.0) {
    ++n_disc;
    const int meta = meta_fn();
    const double q = sqrt(disc);
    const double t1 = (-dt - q) / a;
    const int k1 = (meta >> 1) << kKeyShift;
    const bool eligible = !SHADOW || (meta & 1);
    if (t1 >= 0.0) {
      if (eligible && better(t1, k1, h.t, h.key)) { h.t = t1; h.key = k1; h.hin = 0; }
    } else {  // root 2 matters only now (t1 < 0 or NaN): its division is left out otherwise
      const double t2 = (-dt + q) / a;
      if (eligible && t2 >= 0.0 && better(t2, k1 + 1, h.t, h.key)) { h.t = t2; h.key = k1 + 1; h.hin = 1; }
      if (!SHADOW && t1 < 0.0 && t2 >= 0.0) push_container(h, t1, k1);
    }
  }
}
template <bool SHADOW, typename MetaFn>
__device__ __forceinline__ void sphere_test(double ox, double oy, double oz, double dx, double dy, double dz,
                                            MetaFn meta_fn, Hit& h, unsigned& n_disc) {
  const double a = dx * dx + dy * dy + dz * dz;
  const double dt = dx * ox + dy * oy + dz * oz;
  const double c = ox * ox + oy * oy + oz * oz - 1.0;
  sphere_adc<SHADOW>(a, dt, c, meta_fn, h, n_disc);
}

// Plane::local_intersect (plane.rs:53-60) from the object-space y of origin
// and direction.
template <bool SHADOW>
__device__ __forceinline__ void plane_test(double oy, double dy, int meta, Hit& h) {
  if (!(fabs(dy) < kEpsilon)) {
    // a shadow ray moving away from the plane (oy, dy of one sign, the quotient far
    // from underflow): t < 0, no blocker, and its division is left out (the
    // closest hit needs t < 0 for `containers`)
    if (SHADOW && (oy > 0.0) == (dy > 0.0) && fabs(oy) > 1e-280 && fabs(dy) < 1e20) return;
    const double t = -oy / dy;
    const int k = (meta >> 1) << kKeyShift;
    const bool eligible = !SHADOW || (meta & 1);
    if (eligible && t >= 0.0 && better(t, k, h.t, h.key)) { h.t = t; h.key = k; h.hin = 0; }
    if (!SHADOW && t < 0.0) push_container(h, t, k);
  }
}

// Cube::check_axis (cube.rs:30-47)
__device__ __forceinline__ void cube_check_axis(double origin, double direction, double& tmin, double& tmax) {
  const double tmin_numerator = -1.0 - origin;
  const double tmax_numerator = 1.0 - origin;
  if (fabs(direction) >= kEpsilon) {
    tmin = tmin_numerator / direction;
    tmax = tmax_numerator / direction;
  } else {
    tmin = tmin_numerator * INFINITY;
    tmax = tmax_numerator * INFINITY;
  }
  if (tmin > tmax) { const double x = tmin; tmin = tmax; tmax = x; }
}
// Cylinder::check_cap (cylinder.rs:42-46, radius 1) / Cone::check_cap
// (cone.rs:67-71, radius = the cap's y)
__device__ __forceinline__ bool check_cap(V3 o, V3 d, double t, double radius) {
  const double x = o.x + t * d.x;
  const double z = o.z + t * d.z;
  return (x * x + z * z) <= radius * radius;
}
// intersect_caps (cylinder.rs:48-65, cone.rs:48-65): appends to t[n..]
__device__ __forceinline__ int intersect_caps(int kind, double mn, double mx, bool closed, V3 o, V3 d, double* t,
                                              int n) {
  if (!closed) return n;
  const bool cone = kind == 4;
  double tc = (mn - o.y) / d.y;
  if (check_cap(o, d, tc, cone ? mn : 1.0)) t[n++] = tc;
  tc = (mx - o.y) / d.y;
  if (check_cap(o, d, tc, cone ? mx : 1.0)) t[n++] = tc;
  return n;
}
// Cube / Cylinder / Cone local_intersect (cube.rs:71-93, cylinder.rs:88-119,
// cone.rs:94-134): the reference's list, in push order, into t[0..n).
__device__ __forceinline__ int quad_local_intersect(int kind, double mn, double mx, bool closed, V3 o, V3 d,
                                                    double t[4]) {
  if (kind == 2) {
    double xtmin, xtmax, ytmin, ytmax, ztmin, ztmax;
    cube_check_axis(o.x, d.x, xtmin, xtmax);
    cube_check_axis(o.y, d.y, ytmin, ytmax);
    cube_check_axis(o.z, d.z, ztmin, ztmax);
    const double tmin = fmax(fmax(xtmin, ytmin), ztmin);  // f64::max: NaN-ignoring
    const double tmax = fmin(fmin(xtmax, ytmax), ztmax);
    if (tmin > tmax) return 0;
    t[0] = tmin; t[1] = tmax;
    return 2;
  }
  double a, b, c;
  if (kind == 3) {
    a = d.x * d.x + d.z * d.z;
    if (fabs(a) < kEpsilon) return intersect_caps(kind, mn, mx, closed, o, d, t, 0);
    b = 2.0 * o.x * d.x + 2.0 * o.z * d.z;
    c = o.x * o.x + o.z * o.z - 1.0;
  } else {
    a = d.x * d.x - d.y * d.y + d.z * d.z;
    b = 2.0 * o.x * d.x - 2.0 * o.y * d.y + 2.0 * o.z * d.z;
    c = o.x * o.x - o.y * o.y + o.z * o.z;
    if (fabs(a) < kEpsilon) {
      if (fabs(b) < kEpsilon) return intersect_caps(kind, mn, mx, closed, o, d, t, 0);
      t[0] = -c / 2.0 * b;  // sic (cone.rs:104)
      return intersect_caps(kind, mn, mx, closed, o, d, t, 1);
    }
  }
  const double disc = b * b - 4.0 * a * c;
  if (disc < 0.0) return 0;  // no caps either (cylinder.rs:103-105, cone.rs:113-115)
  const double q = sqrt(disc);
  const double t0 = (-b - q) / (2.0 * a);
  const double t1 = (-b + q) / (2.0 * a);
  int n = 0;
  const double y0 = o.y + t0 * d.y;
  if (mn < y0 && y0 < mx) t[n++] = t0;
  const double y1 = o.y + t1 * d.y;
  if (mn < y1 && y1 < mx) t[n++] = t1;
  return intersect_caps(kind, mn, mx, closed, o, d, t, n);
}
// Shape::intersect (geometry/mod.rs:46-49) of one QuadRec, folded into `h`:
// the nearest t >= 0 of the object's list competes by (t, key); an object
// with an odd number of t < 0 is a container, ordered by its last one.
template <bool SHADOW, typename QP>  // QP: constant-address (wave-uniform) or generic record pointer
__device__ __forceinline__ void quad_test(QP q, V3 o, V3 d, Hit& h) {
  const V3 lo = v3(q->m[0] * o.x + q->m[1] * o.y + q->m[2] * o.z + q->m[3],
                   q->m[4] * o.x + q->m[5] * o.y + q->m[6] * o.z + q->m[7],
                   q->m[8] * o.x + q->m[9] * o.y + q->m[10] * o.z + q->m[11]);
  const V3 ld = v3(q->m[0] * d.x + q->m[1] * d.y + q->m[2] * d.z, q->m[4] * d.x + q->m[5] * d.y + q->m[6] * d.z,
                   q->m[8] * d.x + q->m[9] * d.y + q->m[10] * d.z);
  double t[4];
  const int n = quad_local_intersect(q->kind, q->minimum, q->maximum, q->closed != 0, lo, ld, t);
  if (n == 0) return;
  const int meta = q->meta;
  const int k0 = (meta >> 1) << kKeyShift;
  int n_neg = 0, neg_i = -1, best_i = -1;
  double neg_t = -INFINITY, best_t = INFINITY;
  for (int i = 0; i < n; ++i) {
    if (t[i] < 0.0) {
      ++n_neg;
      if (t[i] >= neg_t) { neg_t = t[i]; neg_i = i; }
    } else if (t[i] >= 0.0 && t[i] < best_t) {
      best_t = t[i]; best_i = i;
    }
  }
  const bool eligible = !SHADOW || (meta & 1);
  if (eligible && best_i >= 0 && better(best_t, k0 + best_i, h.t, h.key)) {
    h.t = best_t; h.key = k0 + best_i; h.hin = n_neg & 1;
  }
  if (!SHADOW && (n_neg & 1)) push_container(h, neg_t, k0 + neg_i);
}

// vector.rs:103-109
__device__ __forceinline__ V3 vcross(V3 a, V3 b) {
  return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
// Triangle / SmoothTriangle::local_intersect (triangle.rs:63-90,
// smooth_triangle.rs:74-101), operation for operation: false = the empty
// list; otherwise the one intersection's t and its u, v. A NaN u fails
// RangeInclusive::contains, a NaN v passes both comparisons, as there.
__device__ __forceinline__ bool tri_local_intersect(V3 p1, V3 e1, V3 e2, V3 o, V3 d, double& t, double& u, double& v) {
  const V3 dir_cross_e2 = vcross(d, e2);
  const double det = vdot(e1, dir_cross_e2);
  if (fabs(det) < kEpsilon) return false;
  const double f = 1.0 / det;
  const V3 p1_to_origin = vsub(o, p1);
  u = f * vdot(p1_to_origin, dir_cross_e2);
  if (!(0.0 <= u && u <= 1.0)) return false;
  const V3 origin_cross_e1 = vcross(p1_to_origin, e1);
  v = f * vdot(d, origin_cross_e1);
  if (v < 0.0 || (u + v) > 1.0) return false;
  t = f * vdot(e2, origin_cross_e1);
  return true;
}
// Shape::intersect (geometry/mod.rs:46-49) of one TriRec, folded into `h` as
// quad_test folds a one-entry list: t >= 0 competes by (t, key) at list
// position 0; t < 0 is an odd number of negative roots, a container candidate.
// tri_hit: the record's list is not empty, and its t; tri_fold: that intersection into `h`.
template <typename TP>  // TP: constant-address (wave-uniform) or generic record pointer
__device__ __forceinline__ bool tri_hit(TP q, V3 o, V3 d, double& t) {
  const V3 lo = v3(q->m[0] * o.x + q->m[1] * o.y + q->m[2] * o.z + q->m[3],
                   q->m[4] * o.x + q->m[5] * o.y + q->m[6] * o.z + q->m[7],
                   q->m[8] * o.x + q->m[9] * o.y + q->m[10] * o.z + q->m[11]);
  const V3 ld = v3(q->m[0] * d.x + q->m[1] * d.y + q->m[2] * d.z, q->m[4] * d.x + q->m[5] * d.y + q->m[6] * d.z,
                   q->m[8] * d.x + q->m[9] * d.y + q->m[10] * d.z);
  double u, v;
  return tri_local_intersect(v3(q->p1[0], q->p1[1], q->p1[2]), v3(q->e1[0], q->e1[1], q->e1[2]),
                             v3(q->e2[0], q->e2[1], q->e2[2]), lo, ld, t, u, v);
}
template <bool SHADOW>
__device__ __forceinline__ void tri_fold(int meta, double t, Hit& h) {
  const int k0 = (meta >> 1) << kKeyShift;
  if (t >= 0.0) {
    if ((!SHADOW || (meta & 1)) && better(t, k0, h.t, h.key)) { h.t = t; h.key = k0; h.hin = 0; }
  } else if (!SHADOW && t < 0.0) {
    push_container(h, t, k0);
  }
}
template <bool SHADOW, typename TP>
__device__ __forceinline__ void tri_test(TP q, V3 o, V3 d, Hit& h) {
  double t;
  if (tri_hit(q, o, d, t)) tri_fold<SHADOW>(q->meta, t, h);
}

// BoundingBox::intersects (bounding_box.rs:95-136) of a Group's box, with the
// reference's operations: per axis (min - o) / d and (max - o) / d, or, when
// |d| < EPSILON, the numerators times infinity (0 * inf = NaN), swapped when
// reversed; then f64::max / f64::min, which ignore a NaN operand (fmax / fmin).
__device__ __forceinline__ void bbox_check_axis(double origin, double direction, double mn, double mx, double& t0,
                                                double& t1) {
  const double tmin_numerator = mn - origin, tmax_numerator = mx - origin;
  double tmin, tmax;
  if (fabs(direction) >= kEpsilon) {
    tmin = tmin_numerator / direction;
    tmax = tmax_numerator / direction;
  } else {
    tmin = tmin_numerator * INFINITY;
    tmax = tmax_numerator * INFINITY;
  }
  if (tmin > tmax) { t0 = tmax; t1 = tmin; } else { t0 = tmin; t1 = tmax; }
}
template <typename BP>  // BP: constant-address (wave-uniform) or generic pointer to a box's corners
__device__ __forceinline__ bool bbox_intersects(BP lo, BP hi, V3 o, V3 d) {
  double x0, x1, y0, y1, z0, z1;
  bbox_check_axis(o.x, d.x, lo[0], hi[0], x0, x1);
  bbox_check_axis(o.y, d.y, lo[1], hi[1], y0, y1);
  bbox_check_axis(o.z, d.z, lo[2], hi[2], z0, z1);
  const double tmin = fmax(fmax(x0, y0), z0), tmax = fmin(fmin(x1, y1), z1);
  return tmin <= tmax;
}
__device__ __forceinline__ bool bbox_intersects(cGroupRec g, V3 o, V3 d) { return bbox_intersects(g->lo, g->hi, o, d); }
// Group::intersect (group.rs:49-58): a shape inside groups is intersected only
// when the ray meets the box of every group around it, innermost first (the
// reference tests them outermost first and stops at the first miss; either
// order gives the same answer). `gate` = the record's gate (0: no group).
// A shape that fails it adds no intersection and no local_intersect call.
__device__ __forceinline__ bool group_gate(const DevScene& sc, int gate, V3 o, V3 d) {
  const cGroupRec groups = (cGroupRec)sc.groups;
  for (int g = gate; g > 0; g = groups[g - 1].parent)
    if (!bbox_intersects(groups + (g - 1), o, d)) return false;
  return true;
}
// Shapes a group's box kept out of a ray's World::intersect, by kind (the
// counted launches subtract them from the reference's rays x shapes).
struct GateSkips {
  unsigned sph = 0, plane = 0, other = 0;
};

// ------------------------------------------------------------------- Csg
__device__ __forceinline__ void csg_skip(GateSkips& sk, int counts) {
  sk.sph += counts & 31; sk.plane += (counts >> 5) & 31; sk.other += (unsigned)counts >> 10;
}
// Shape::intersect (geometry/mod.rs:46-49) of one leaf of kinds 0-4 under a Csg: its
// list in push order into t[0..n): the sphere's roots as sphere_adc forms them, the
// plane's as plane_test, the solids' as quad_test (quad_local_intersect).
__device__ __forceinline__ int csg_leaf_roots(const OtherRec* q, V3 o, V3 d, double t[4], unsigned& n_disc) {
  const double* m = q->m;
  const V3 lo = m34_point(m, o);
  const V3 ld = v3(m[0] * d.x + m[1] * d.y + m[2] * d.z, m[4] * d.x + m[5] * d.y + m[6] * d.z,
                   m[8] * d.x + m[9] * d.y + m[10] * d.z);
  if (q->kind == 0) {  // sphere.rs:47-62
    const double a = ld.x * ld.x + ld.y * ld.y + ld.z * ld.z;
    const double dt = ld.x * lo.x + ld.y * lo.y + ld.z * lo.z;
    const double c = lo.x * lo.x + lo.y * lo.y + lo.z * lo.z - 1.0;
    const double disc = dt * dt - a * c;
    if (!(disc >= 0.0)) return 0;
    ++n_disc;
    const double s = sqrt(disc);
    t[0] = (-dt - s) / a;
    t[1] = (-dt + s) / a;
    return 2;
  }
  if (q->kind == 1) {  // plane.rs:53-60
    if (fabs(ld.y) < kEpsilon) return 0;
    t[0] = -lo.y / ld.y;
    return 1;
  }
  return quad_local_intersect(q->kind, q->minimum, q->maximum, q->closed != 0, lo, ld, t);
}
// The same roots appended to the narrow evaluator's list in push order (a sphere's and a
// plane's straight from their registers).
__device__ __forceinline__ void csg_leaf(const OtherRec* q, V3 o, V3 d, CsgList& xs, unsigned& n_disc) {
  const double* m = q->m;
  const V3 lo = m34_point(m, o);
  const V3 ld = v3(m[0] * d.x + m[1] * d.y + m[2] * d.z, m[4] * d.x + m[5] * d.y + m[6] * d.z,
                   m[8] * d.x + m[9] * d.y + m[10] * d.z);
  const int k0 = (q->meta >> 1) << kKeyShift;
  if (q->kind == 0) {  // sphere.rs:47-62
    const double a = ld.x * ld.x + ld.y * ld.y + ld.z * ld.z;
    const double dt = ld.x * lo.x + ld.y * lo.y + ld.z * lo.z;
    const double c = lo.x * lo.x + lo.y * lo.y + lo.z * lo.z - 1.0;
    const double disc = dt * dt - a * c;
    if (disc >= 0.0) {
      ++n_disc;
      const double s = sqrt(disc);
      csg_push(xs, (-dt - s) / a, k0);
      csg_push(xs, (-dt + s) / a, k0 + 1);
    }
  } else if (q->kind == 1) {  // plane.rs:53-60
    if (!(fabs(ld.y) < kEpsilon)) csg_push(xs, -lo.y / ld.y, k0);
  } else {
    double t[4];
    const int n = quad_local_intersect(q->kind, q->minimum, q->maximum, q->closed != 0, lo, ld, t);
    for (int i = 0; i < n; ++i) csg_push(xs, t[i], k0 + i);
  }
}
// A unit's surviving intersections into `h`, as quad_test folds one object's
// list, but counted over each leaf's SURVIVORS: the nearest t >= 0 competes by
// (t, key) (the unit's list is in key order under ties, and its leaves' object
// indices are consecutive, so this is the world's stable sort, world.rs:31-38);
// the hit leaf is in `containers` when an odd number of its survivors lie
// before the origin; a leaf with an odd number of survivors t < 0 is a
// container candidate at its last one. Shadow rays: the leaf's own has_shadow.
template <bool SHADOW>
__device__ __forceinline__ void csg_fold(const DevScene& sc, const CsgList& xs, Hit& h) {
  int best = -1;
  double bt = h.t;
  int bk = h.key;
  for (int i = 0; i < xs.n; ++i) {
    const double t = xs.t[i];
    if (t >= 0.0) {
      if (better(t, xs.key[i], bt, bk) && (!SHADOW || sc.shade[xs.key[i] >> kKeyShift].shadow)) {
        bt = t; bk = xs.key[i]; best = i;
      }
    } else if (!SHADOW && t < 0.0) {
      const int obj = xs.key[i] >> kKeyShift;
      int n_neg = 0;
      bool last = true;
      for (int j = 0; j < xs.n; ++j)
        if ((xs.key[j] >> kKeyShift) == obj && xs.t[j] < 0.0) {
          ++n_neg;
          if (j > i) last = false;
        }
      if (last && (n_neg & 1)) push_container(h, t, xs.key[i]);
    }
  }
  if (best >= 0) {
    const int obj = bk >> kKeyShift;
    int n_neg = 0;
    for (int j = 0; j < xs.n; ++j)
      if ((xs.key[j] >> kKeyShift) == obj && xs.t[j] < 0.0) ++n_neg;
    h.t = bt; h.key = bk; h.hin = n_neg & 1;
  }
}
// World::intersect's share of one Csg unit (world.rs:31-38 over the Csgs of
// World::objects, and over those inside groups, whose gates the caller tests first).
// The ray goes down the chain one matrix after another (never a
// product), every gate is the reference's, in binary64; the leaves append to
// one list, each Csg node closes its tail (rt_csg.hpp), the root's survivors
// fold into `h`. COUNT_ONLY: the gates alone, for a counted launch's ray that
// was answered before (count_rest_gates) or whose walk never reached the unit
// (count_hier_gates). Inlined like every other trace
// function: the list, the ray stack and the list starts are private arrays
// indexed per lane (scratch, as the walks' stacks), and nothing is reached
// through a pointer to a local.
template <bool SHADOW, bool COUNT_ONLY>
__device__ __forceinline__ void csg_unit_eval(const DevScene& sc, const CsgUnit un, V3 o, V3 d, Hit& h, unsigned& disc,
                                              GateSkips& sk) {
  CsgList xs;
  xs.n = 0;
  double ray[kCsgMaxDepth + 1][6];
  int start[kCsgMaxDepth + 1];
  int lvl = 0;
  V3 co = o, cd = d;
  const int end = un.first + un.n;
  for (int pc = un.first; pc < end;) {
    const CsgOp op = sc.csg_ops[pc];
    if (op.code == kCsgEnter) {
      const CsgRec* c = sc.csg_nodes + op.arg;
      const V3 lo = m34_point(c->m, co);  // Ray::transform by the Csg's own inverse (ray.rs:26-28)
      const V3 ld = v3(c->m[0] * cd.x + c->m[1] * cd.y + c->m[2] * cd.z, c->m[4] * cd.x + c->m[5] * cd.y + c->m[6] * cd.z,
                       c->m[8] * cd.x + c->m[9] * cd.y + c->m[10] * cd.z);
      if (lvl >= kCsgMaxDepth || !bbox_intersects(c->lo, c->hi, lo, ld)) {  // csg.rs:116-118
        csg_skip(sk, op.counts);
        pc = op.skip_to;
        continue;
      }
      ray[lvl][0] = co.x; ray[lvl][1] = co.y; ray[lvl][2] = co.z;
      ray[lvl][3] = cd.x; ray[lvl][4] = cd.y; ray[lvl][5] = cd.z;
      start[lvl] = xs.n;
      ++lvl;
      co = lo; cd = ld;
    } else if (op.code == kCsgExit) {
      --lvl;
      if (!COUNT_ONLY) csg_close(xs, start[lvl], sc.csg_nodes[op.arg].op, sc.csg_nodes[op.arg].split);
      co = v3(ray[lvl][0], ray[lvl][1], ray[lvl][2]);
      cd = v3(ray[lvl][3], ray[lvl][4], ray[lvl][5]);
    } else if (op.code == kCsgGroup) {
      if (!bbox_intersects((cGroupRec)sc.groups + op.arg, co, cd)) {  // group.rs:50-52, the ray it is handed
        csg_skip(sk, op.counts);
        pc = op.skip_to;
        continue;
      }
    } else if (op.code == kCsgLeaf) {  // (kCsgTri: a wide unit's, here only for its gates, COUNT_ONLY)
      if (!COUNT_ONLY) csg_leaf(sc.csg_leaves + op.arg, co, cd, xs, disc);
    }
    ++pc;
  }
  if (!COUNT_ONLY) csg_fold<SHADOW>(sc, xs, h);
}
// The same for a WIDE unit (rt_layout.hpp kCsgWide: one with triangle leaves, whose list
// has no small bound), in the stream form of rt_csg.hpp. Each walk of the program (the
// same chain of rays and the same gates as above) collects the kCsgListCap smallest roots
// above a watermark (t, key), ascending; the batch goes through the nodes' filter bits
// (csg_stream_pass) and the survivors fold into `h` as csg_fold folds them: the first
// survivor t >= 0 (a shadow ray's: of a leaf that casts one) competes by (t, key), `hin` is
// the parity of its leaf's survivors t < 0, a leaf with an odd number of those is a
// container candidate at its last one (a triangle has one root: pushed at once; the
// others at the end, CsgNegTable). When the walk left roots out, the watermark moves to
// the batch's last entry and the program is walked again. It ends at the unit's hit, or at
// the first root beyond the current h.t: nothing later is a hit, a container or `hin`.
// The gate skips and sphere_disc_ge0 are the first walk's.
__device__ __forceinline__ bool csg_tri_roots(const TriRec* q, V3 o, V3 d, double& t) {
  const V3 lo = m34_point(q->m, o);
  const V3 ld = v3(q->m[0] * d.x + q->m[1] * d.y + q->m[2] * d.z, q->m[4] * d.x + q->m[5] * d.y + q->m[6] * d.z,
                   q->m[8] * d.x + q->m[9] * d.y + q->m[10] * d.z);
  double u, v;
  return tri_local_intersect(v3(q->p1[0], q->p1[1], q->p1[2]), v3(q->e1[0], q->e1[1], q->e1[2]),
                             v3(q->e2[0], q->e2[1], q->e2[2]), lo, ld, t, u, v);
}
// A run's hierarchy in place of its one-by-one ops (rt_slab.hpp csg_run_walk; DESIGN.md §5.2 "Csg
// units: run hierarchies"): at the first op of a run that has one, in a launch that walks them
// (DevScene::csg_runs), for a chained ray the run's bounds admit. Each reached triangle does what
// its kCsgTri op does: csg_tri_roots, then csg_batch_insert with the same key and tag. The visiting
// order is free (csg_run_walk). True: the run is done, the caller goes on past it (op.skip_to).
// The walk itself stays out of line: its slab constants, stack and node in flight are then a frame of its own,
// and the scenes that walk run faster for it (csg_mesh_scene 59 -> 50 ms a frame, csg_mesh_big 18 -> 14,
// profiles/csg_run_ab.txt). What the walk's presence costs the one-by-one ops is the same either way: the kernels
// of scenes without a run are compiled without it (RUNS = false).
template <typename Tag>
__device__ __noinline__ void csg_run_walk_into(const CsgRun* rp, const BvhNode* nodes, const TriRec* tris, V3 co, V3 cd, float t_lo,
                                               float t_hi, CsgBatchT<Tag>* b, Tag tag, double wt, int32_t wk, bool* more) {
  const CsgRun run = *rp;
  const TriRec* recs = tris + run.first;
  bool m = *more;
  csg_run_walk(run, nodes + run.node, co, cd, t_lo, t_hi, [&](int k) {
    const TriRec* q = recs + k;
    double t;
    if (csg_tri_roots(q, co, cd, t)) csg_batch_insert(*b, kCsgListCap, t, (q->meta >> 1) << kKeyShift, tag, wt, wk, m);
  });
  *more = m;
}
template <typename Tag>
__device__ __forceinline__ bool csg_run_eval(const DevScene& sc, const CsgOp op, V3 co, V3 cd, double t_stop, CsgBatchT<Tag>& b,
                                             Tag tag, double wt, int32_t wk, bool& more) {
  // (one op a run carries a run's index: against the ops of the runs without a hierarchy this is the cold side)
  if (__builtin_expect(!sc.csg_runs || op.counts <= 0, 1)) return false;
  const CsgRun* rp = sc.csg_runs + (op.counts - 1);
  if (!csg_run_admits(*rp, co, cd)) return false;
  csg_run_walk_into(rp, sc.csg_run_nodes, sc.csg_tris, co, cd, f32_below(wt), f32_up(t_stop), &b, tag, wt, wk, &more);
  return true;
}
// RUNS = false: a kernel that never walks a run's hierarchy: the batch kernels, and the render kernels that a scene
// without a run or an exhaustive render launches (the walk stays out of them: they keep their registers and scratch).
template <bool SHADOW, bool RUNS = false>
__device__ __forceinline__ void csg_wide_eval(const DevScene& sc, const CsgUnit un, V3 o, V3 d, Hit& h, unsigned& disc,
                                              GateSkips& sk) {
  CsgBatch b;
  CsgNegTable nt;
  nt.odd = 0;
  uint32_t inl = 0, inr = 0;
  double wt = -INFINITY;  // below every root: (t, key) > (-inf, -1)
  int32_t wk = -1;
  const int end = un.first + un.n;
  const CsgRec* nodes = sc.csg_nodes + sc.csg_ops[un.first].arg;  // the unit's own node first
  bool first = true;
  for (;;) {
    b.xs.n = 0;
    bool more = false;
    double ray[kCsgMaxDepth + 1][6];
    int lvl = 0, node = -1;
    V3 co = o, cd = d;
    for (int pc = un.first; pc < end;) {
      const CsgOp op = sc.csg_ops[pc];
      if (op.code == kCsgEnter) {
        const CsgRec* c = sc.csg_nodes + op.arg;
        const V3 lo = m34_point(c->m, co);
        const V3 ld = v3(c->m[0] * cd.x + c->m[1] * cd.y + c->m[2] * cd.z, c->m[4] * cd.x + c->m[5] * cd.y + c->m[6] * cd.z,
                         c->m[8] * cd.x + c->m[9] * cd.y + c->m[10] * cd.z);
        if (lvl >= kCsgMaxDepth || !bbox_intersects(c->lo, c->hi, lo, ld)) {  // csg.rs:116-118
          if (first) csg_skip(sk, op.counts);
          pc = op.skip_to;
          continue;
        }
        ray[lvl][0] = co.x; ray[lvl][1] = co.y; ray[lvl][2] = co.z;
        ray[lvl][3] = cd.x; ray[lvl][4] = cd.y; ray[lvl][5] = cd.z;
        ++lvl;
        node = c->self;
        co = lo; cd = ld;
      } else if (op.code == kCsgExit) {
        --lvl;
        node = nodes[node].parent;
        co = v3(ray[lvl][0], ray[lvl][1], ray[lvl][2]);
        cd = v3(ray[lvl][3], ray[lvl][4], ray[lvl][5]);
      } else if (op.code == kCsgGroup) {
        if (!bbox_intersects((cGroupRec)sc.groups + op.arg, co, cd)) {  // group.rs:50-52, the ray it is handed
          if (first) csg_skip(sk, op.counts);
          pc = op.skip_to;
          continue;
        }
      } else if (op.code == kCsgTri) {
        if constexpr (RUNS) {
          if (csg_run_eval(sc, op, co, cd, h.t, b, (uint16_t)(node | kCsgTagTri), wt, wk, more)) {
            pc = op.skip_to;
            continue;
          }
        }
        const TriRec* q = sc.csg_tris + op.arg;
        double t;
        if (csg_tri_roots(q, co, cd, t))
          csg_batch_insert(b, kCsgListCap, t, (q->meta >> 1) << kKeyShift, (uint16_t)(node | kCsgTagTri), wt, wk, more);
      } else {
        const OtherRec* q = sc.csg_leaves + op.arg;
        double t[4];
        unsigned nd = 0;
        const int n = csg_leaf_roots(q, co, cd, t, nd);
        if (first) disc += nd;
        const int k0 = (q->meta >> 1) << kKeyShift;
        const uint16_t tag = (uint16_t)(node | q->gate << kCsgTagSlotShift);
        for (int i = 0; i < n; ++i) csg_batch_insert(b, kCsgListCap, t[i], k0 + i, tag, wt, wk, more);
      }
      ++pc;
    }
    bool done = false;
    for (int i = 0; i < b.xs.n && !done; ++i) {
      const double t = b.xs.t[i];
      const int key = b.xs.key[i];
      const int tag = b.tag[i];
      if (t > h.t) {
        done = true;
      } else if (csg_stream_pass(nodes, tag & kCsgTagNode, key, inl, inr)) {
        const int slot = (tag >> kCsgTagSlotShift) & kCsgTagSlot;
        if (t < 0.0) {
          if (tag & kCsgTagTri) {
            if (!SHADOW) push_container(h, t, key);
          } else {
            csg_neg_note(nt, slot, t, key);
          }
        } else if (!SHADOW || sc.shade[key >> kKeyShift].shadow) {
          if (better(t, key, h.t, h.key)) {
            h.t = t; h.key = key; h.hin = (tag & kCsgTagTri) ? 0 : (int)((nt.odd >> slot) & 1u);
          }
          done = true;
        }
      }
    }
    if (done || !more) break;
    wt = b.xs.t[b.xs.n - 1];
    wk = b.xs.key[b.xs.n - 1];
    first = false;
  }
  if (!SHADOW)
    for (int s = 0; s < kCsgMaxLeaves; ++s)
      if ((nt.odd >> s) & 1u) push_container(h, nt.t[s], nt.key[s]);
}
// The same for a DEEP unit (rt_layout.hpp kCsgDeep: any depth, node and leaf count), the stream
// form again: csg_wide_eval's walk, gates, chained ray, batches and stop, with state that scales
// (rt_csg.hpp csg_deep_step / csg_deep_note). The filter bits, the leaves' parity bits and the
// ray each open level's Enter found live in the launch's state buffer, this lane's words
// (DevScene::csg_deep_state: no scratch grows with the unit); the batch is the wide evaluator's.
// The gates' sphere and plane counts come from DevScene::csg_counts. After the first pass over
// the stream (the hit, `hin`, the parities) a radiance ray with an odd leaf takes a second over
// its part t < 0 for the two container candidates. COUNT_ONLY: the first walk's gates alone.
__device__ __forceinline__ void csg_skip_deep(GateSkips& sk, const DevScene& sc, int pc, int counts) {
  sk.sph += sc.csg_counts[2 * pc]; sk.plane += sc.csg_counts[2 * pc + 1]; sk.other += (unsigned)counts >> 10;
}
__device__ __forceinline__ void csg_deep_save(const CsgDeepWords& st, int at, V3 o, V3 d) {
  const double v[6] = {o.x, o.y, o.z, d.x, d.y, d.z};
#pragma unroll
  for (int e = 0; e < 6; ++e) {
    st[at + 2 * e] = (uint32_t)__double2loint(v[e]);
    st[at + 2 * e + 1] = (uint32_t)__double2hiint(v[e]);
  }
}
__device__ __forceinline__ void csg_deep_load(const CsgDeepWords& st, int at, V3& o, V3& d) {
  double v[6];
#pragma unroll
  for (int e = 0; e < 6; ++e) v[e] = __hiloint2double((int)st[at + 2 * e + 1], (int)st[at + 2 * e]);
  o = v3(v[0], v[1], v[2]);
  d = v3(v[3], v[4], v[5]);
}
template <bool SHADOW, bool COUNT_ONLY, bool RUNS = false>
__device__ __forceinline__ void csg_deep_eval(const DevScene& sc, const CsgUnit un, V3 o, V3 d, Hit& h, unsigned& disc,
                                              GateSkips& sk) {
  const unsigned lane = blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= sc.csg_deep_lanes) return;  // (no launch is larger than its state buffer: rt_wavefront.hip, rt_render.cpp)
  const CsgDeepWords st{sc.csg_deep_state + lane, (size_t)sc.csg_deep_lanes};
  const int nw = sc.csg_deep_nw, lw = sc.csg_deep_lw, rays = 2 * nw + lw;
  const int end = un.first + un.n;
  const CsgRec* nodes = sc.csg_nodes + sc.csg_ops[un.first].arg;  // the unit's own node first
  CsgDeepBatch b;
  CsgDeepHit dh{h.t, h.key, h.hin};
  CsgDeepTop2 top;
  csg_deep_top2_init(top);
  bool first = true;
  // pass 0: the hit, `hin` and the parities; pass 1: the container candidates
  for (int pass = 0; pass < (SHADOW || COUNT_ONLY ? 1 : 2); ++pass) {
    if (pass == 1) {
      uint32_t any = 0;
      for (int i = 0; i < lw; ++i) any |= st[2 * nw + i];
      if (!any) break;
    }
    for (int i = 0; i < (pass == 0 ? rays : 2 * nw); ++i) st[i] = 0u;
    double wt = -INFINITY;  // below every root: (t, key) > (-inf, -1)
    int32_t wk = -1;
    for (;;) {
      b.xs.n = 0;
      bool more = false;
      int lvl = 0, node = -1;
      V3 co = o, cd = d;
      for (int pc = un.first; pc < end;) {
        const CsgOp op = sc.csg_ops[pc];
        if (op.code == kCsgEnter) {
          const CsgRec* c = sc.csg_nodes + op.arg;
          const V3 lo = m34_point(c->m, co);
          const V3 ld = v3(c->m[0] * cd.x + c->m[1] * cd.y + c->m[2] * cd.z, c->m[4] * cd.x + c->m[5] * cd.y + c->m[6] * cd.z,
                           c->m[8] * cd.x + c->m[9] * cd.y + c->m[10] * cd.z);
          if (lvl >= sc.csg_deep_levels || !bbox_intersects(c->lo, c->hi, lo, ld)) {  // csg.rs:116-118
            if (first) csg_skip_deep(sk, sc, pc, op.counts);
            pc = op.skip_to;
            continue;
          }
          csg_deep_save(st, rays + 12 * lvl, co, cd);
          ++lvl;
          node = c->self;
          co = lo; cd = ld;
        } else if (op.code == kCsgExit) {
          --lvl;
          node = nodes[node].parent;
          csg_deep_load(st, rays + 12 * lvl, co, cd);
        } else if (op.code == kCsgGroup) {
          if (!bbox_intersects((cGroupRec)sc.groups + op.arg, co, cd)) {  // group.rs:50-52, the ray it is handed
            if (first) csg_skip_deep(sk, sc, pc, op.counts);
            pc = op.skip_to;
            continue;
          }
        } else if (COUNT_ONLY) {
        } else if (op.code == kCsgTri) {
          if constexpr (RUNS) {  // (dh.t: what csg_deep_step's stop compares against; it moves only where a pass ends)
            if (csg_run_eval(sc, op, co, cd, dh.t, b, (uint32_t)node | kCsgDeepTagTri, wt, wk, more)) {
              pc = op.skip_to;
              continue;
            }
          }
          const TriRec* q = sc.csg_tris + op.arg;
          double t;
          if (csg_tri_roots(q, co, cd, t))
            csg_batch_insert(b, kCsgListCap, t, (q->meta >> 1) << kKeyShift, (uint32_t)node | kCsgDeepTagTri, wt, wk, more);
        } else {
          const OtherRec* q = sc.csg_leaves + op.arg;
          double t[4];
          unsigned nd = 0;
          const int n = csg_leaf_roots(q, co, cd, t, nd);
          if (first) disc += nd;
          const int k0 = (q->meta >> 1) << kKeyShift;
          const uint32_t tag = (uint32_t)node | (uint32_t)q->gate << kCsgDeepTagSlotShift;
          for (int i = 0; i < n; ++i) csg_batch_insert(b, kCsgListCap, t[i], k0 + i, tag, wt, wk, more);
        }
        ++pc;
      }
      first = false;
      if (COUNT_ONLY) return;
      bool done = false;
      for (int i = 0; i < b.xs.n && !done; ++i) {
        const double t = b.xs.t[i];
        const int key = b.xs.key[i];
        const uint32_t tag = b.tag[i];
        if (pass == 0) {
          const int r = csg_deep_step(nodes, st, nw, t, key, tag,
                                      [&](int32_t k) { return !SHADOW || sc.shade[k >> kKeyShift].shadow != 0; }, dh);
          if (r == kCsgDeepTriNeg) {
            if (!SHADOW) push_container(h, t, key);
          } else {
            done = r == kCsgDeepDone;
          }
        } else if (t < 0.0) {
          csg_deep_note(nodes, st, nw, t, key, tag, top);
        } else {
          done = true;
        }
      }
      if (done || !more) break;
      wt = b.xs.t[b.xs.n - 1];
      wk = b.xs.key[b.xs.n - 1];
    }
  }
  h.t = dh.t; h.key = dh.key; h.hin = dh.hin;
  if (!SHADOW) {
    if (top.k1 >= 0) push_container(h, top.t1, top.k1);
    if (top.k2 >= 0) push_container(h, top.t2, top.k2);
  }
}
// The units `units[0 .. n)`, each behind the gate of the groups around it (Group::intersect,
// group.rs:49-58): the exhaustive paths pass the scene's full list in the reference's order,
// the fast path the units outside the hierarchy (trace_rest; unit_trace walks the others).
// DEEP = false: a kernel that is launched only for scenes without a deep unit (the batch kernels have such
// twins: the deep evaluator stays out of them, and they keep their registers).
template <bool SHADOW, bool COUNT_ONLY, bool DEEP = true, bool RUNS = false>
__device__ __forceinline__ void csg_units(const DevScene& sc, const CsgUnit* units, int n, V3 o, V3 d, Hit& h,
                                          unsigned& n_disc, GateSkips* skips) {
  GateSkips sk;
  unsigned disc = 0;
  for (int u = 0; u < n; ++u) {
    CsgUnit un = units[u];
    const bool wide = (un.n & kCsgWide) != 0, deep = DEEP && (un.n & kCsgDeep) != 0;
    if (un.gate && !group_gate(sc, un.gate, o, d)) {
      if (deep) csg_skip_deep(sk, sc, un.first, un.counts);  // (its own Enter holds the unit's counts)
      else csg_skip(sk, un.counts);
      continue;
    }
    un.n &= ~kCsgKindMask;
    if (deep) csg_deep_eval<SHADOW, COUNT_ONLY, RUNS>(sc, un, o, d, h, disc, sk);
    else if (!COUNT_ONLY && wide) csg_wide_eval<SHADOW, RUNS>(sc, un, o, d, h, disc, sk);
    else csg_unit_eval<SHADOW, COUNT_ONLY>(sc, un, o, d, h, disc, sk);  // (a wide unit's gates alone: the same walk)
  }
  n_disc += disc;
  if (skips) { skips->sph += sk.sph; skips->plane += sk.plane; skips->other += sk.other; }
}

// ----------------------------------------------------------- alias classes
// World::intersect's share of the alias classes (rt_layout.hpp AliasClass; DESIGN.md "containers
// walk -> top-2", "Alias classes"). In the walk of prepare_computations `contains` and `position`
// compare by structural equality, so the members of a class are one `containers` entry: each
// intersection of any member before the hit toggles it. It is there at the hit iff the class has
// an odd number of roots t < 0 over ALL its members, at the place of the last of them by
// (t, key); its refractive index is any member's (equal shapes have bit-equal materials). So per
// class, in registers: the count of roots t < 0 and the greatest (t, key) among them, one
// push_container after the last member. The closest hit is each member's own business: every
// root t >= 0 competes by (t, key) with its own object index. A hit on a member finds its object
// in `containers` iff the class is there (`hin`).
// Each member's roots are its kind's, operation for operation: sphere_adc's, plane_test's,
// quad_local_intersect's; a NaN root (a sphere's, from a zero direction) is neither before the
// hit nor a hit, as everywhere else. Shadow rays (is_shadowed asks for any blocker): every member
// is an ordinary record. The members are in no hierarchy: every ray tests each behind its gate.
template <bool SHADOW>
__device__ __forceinline__ void alias_classes(const DevScene& sc, V3 o, V3 d, Hit& h, unsigned& n_disc,
                                              GateSkips* skips) {
  const cQuadRec rec = (cQuadRec)sc.alias_rec;
  const AliasClass RT_CONST* cls = (const AliasClass RT_CONST*)sc.alias_cls;
  for (int c = 0; c < sc.n_alias_cls; ++c) {
    const int first = cls[c].first, end = first + cls[c].n;
    int n_neg = 0, neg_k = -1;
    double neg_t = -INFINITY;
    bool took = false;
    for (int j = first; j < end; ++j) {
      const int kind = rec[j].kind;
      if (rec[j].gate && !group_gate(sc, rec[j].gate, o, d)) {  // Group::intersect (group.rs:49-58)
        if (skips) {
          if (kind == 0) ++skips->sph; else if (kind == 1) ++skips->plane; else ++skips->other;
        }
        continue;
      }
      if constexpr (SHADOW) {
        if (kind == 1) {
          plane_test<true>(rec[j].m[4] * o.x + rec[j].m[5] * o.y + rec[j].m[6] * o.z + rec[j].m[7],
                           rec[j].m[4] * d.x + rec[j].m[5] * d.y + rec[j].m[6] * d.z, rec[j].meta, h);
        } else if (kind == 0) {
          double m[12];
#pragma unroll
          for (int e = 0; e < 12; ++e) m[e] = rec[j].m[e];
          const V3 lo = m34_point(m, o);
          const V3 ld = v3(m[0] * d.x + m[1] * d.y + m[2] * d.z, m[4] * d.x + m[5] * d.y + m[6] * d.z,
                           m[8] * d.x + m[9] * d.y + m[10] * d.z);
          sphere_test<true>(lo.x, lo.y, lo.z, ld.x, ld.y, ld.z, [&] { return rec[j].meta; }, h, n_disc);
        } else {
          quad_test<true>(rec + j, o, d, h);
        }
      } else {
        double m[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) m[e] = rec[j].m[e];
        const V3 lo = m34_point(m, o);
        const V3 ld = v3(m[0] * d.x + m[1] * d.y + m[2] * d.z, m[4] * d.x + m[5] * d.y + m[6] * d.z,
                         m[8] * d.x + m[9] * d.y + m[10] * d.z);
        double t[4];
        int n = 0;
        if (kind == 0) {  // sphere.rs:47-62 (sphere_test, sphere_adc)
          const double a = ld.x * ld.x + ld.y * ld.y + ld.z * ld.z;
          const double dt = ld.x * lo.x + ld.y * lo.y + ld.z * lo.z;
          const double cc = lo.x * lo.x + lo.y * lo.y + lo.z * lo.z - 1.0;
          const double disc = dt * dt - a * cc;
          if (disc >= 0.0) {
            ++n_disc;
            const double q = sqrt(disc);
            t[0] = (-dt - q) / a;
            t[1] = (-dt + q) / a;
            n = 2;
          }
        } else if (kind == 1) {  // plane.rs:53-60 (plane_test)
          if (!(fabs(ld.y) < kEpsilon)) {
            t[0] = -lo.y / ld.y;
            n = 1;
          }
        } else {
          n = quad_local_intersect(kind, rec[j].minimum, rec[j].maximum, rec[j].closed != 0, lo, ld, t);
        }
        const int k0 = (rec[j].meta >> 1) << kKeyShift;
        for (int i = 0; i < n; ++i) {
          if (t[i] < 0.0) {
            ++n_neg;
            if (t[i] > neg_t || (t[i] == neg_t && k0 + i > neg_k)) { neg_t = t[i]; neg_k = k0 + i; }
          } else if (t[i] >= 0.0 && better(t[i], k0 + i, h.t, h.key)) {
            h.t = t[i]; h.key = k0 + i; took = true;
          }
        }
      }
    }
    if constexpr (!SHADOW) {
      if (n_neg & 1) push_container(h, neg_t, neg_k);
      if (took) h.hin = n_neg & 1;
    }
  }
}
// The gates alias_classes meets, without its tests (count_rest_gates).
__device__ __forceinline__ void count_alias_gates(const DevScene& sc, V3 o, V3 d, GateSkips& sk) {
  const cQuadRec rec = (cQuadRec)sc.alias_rec;
  for (int j = 0; j < sc.n_alias_rec; ++j)
    if (rec[j].gate && !group_gate(sc, rec[j].gate, o, d)) {
      if (rec[j].kind == 0) ++sk.sph; else if (rec[j].kind == 1) ++sk.plane; else ++sk.other;
    }
}
// After the whole trace of a radiance ray (hit_finish): prepare() asks whether the most recent
// container IS the hit object by comparing object indices; with alias classes the question is
// "the same class" (`position(|&el| el == i.object)`). When the hit object's class is that
// container, the container's key is replaced by the hit's own: the same object as far as
// prepare() can tell, and the same refractive index bit for bit. The stored hit (WfHit) and every
// prepare() then stay what they are for a world without classes.
__device__ __forceinline__ void alias_finish(const DevScene& sc, Hit& h) {
  if (h.key >= 0 && h.hin && h.c1k >= 0) {
    const int obj = h.key >> kKeyShift, c1 = h.c1k >> kKeyShift;
    if (c1 != obj && sc.alias_of[c1] == sc.alias_of[obj]) h.c1k = h.key;
  }
}

// The records outside the sphere BVH (general-transform spheres, planes,
// cubes / cylinders / cones), tested exhaustively from global memory.
// QUADS = false compiles the solids out (kernel variants for scenes without
// them keep the sphere loops' register allocation, hence their occupancy).
// FAST: the fast path's remainder (the records outside both hierarchies;
// the other bounded records are traversed by other_trace).
// TRIS: the triangles too (the kernels of scenes without solids never meet one).
// CSG: the Csg units too (csg_units): every unit, or on the fast path those outside the
// units' hierarchy (fx_units; unit_trace walks the others).
// ALIAS (with CSG): the alias classes too (alias_classes), every member on either path.
template <bool SHADOW, bool QUADS = true, bool FAST = false, bool TRIS = QUADS, bool CSG = false, bool ALIAS = false,
          bool DEEP = true, bool RUNS = false>
__device__ __forceinline__ void trace_rest(const DevScene& sc, V3 o, V3 d, Hit& h, unsigned& n_disc,
                                           GateSkips* skips = nullptr) {
  cSphereGen sg = (cSphereGen)(FAST ? sc.fx_gen : sc.sph_gen);
  const int n_gen = FAST ? sc.n_fx_gen : sc.n_gen;
  for (int j = 0; j < n_gen; ++j) {
    if (sg[j].gate && !group_gate(sc, sg[j].gate, o, d)) {
      if (skips) ++skips->sph;
      continue;
    }
    double m[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) m[e] = sg[j].m[e];
    const V3 lo = m34_point(m, o);
    const V3 ld = v3(m[0] * d.x + m[1] * d.y + m[2] * d.z, m[4] * d.x + m[5] * d.y + m[6] * d.z,
                     m[8] * d.x + m[9] * d.y + m[10] * d.z);
    sphere_test<SHADOW>(lo.x, lo.y, lo.z, ld.x, ld.y, ld.z, [&] { return (int)sg[j].meta; }, h, n_disc);
  }
  cPlaneRec pl = (cPlaneRec)sc.planes;
  for (int j = 0; j < sc.n_planes; ++j) {
    if (pl[j].gate && !group_gate(sc, pl[j].gate, o, d)) {
      if (skips) ++skips->plane;
      continue;
    }
    const double oy = pl[j].m[0] * o.x + pl[j].m[1] * o.y + pl[j].m[2] * o.z + pl[j].m[3];
    const double dy = pl[j].m[0] * d.x + pl[j].m[1] * d.y + pl[j].m[2] * d.z;
    plane_test<SHADOW>(oy, dy, (int)pl[j].meta, h);
  }
  if constexpr (QUADS) {
    cQuadRec qr = (cQuadRec)(FAST ? sc.fx_quads : sc.quads);
    const int n_quads = FAST ? sc.n_fx_quads : sc.n_quads;
    for (int j = 0; j < n_quads; ++j) {
      if (qr[j].gate && !group_gate(sc, qr[j].gate, o, d)) {
        if (skips) ++skips->other;
        continue;
      }
      quad_test<SHADOW>(qr + j, o, d, h);
    }
  }
  if constexpr (TRIS) {
    cTriRec tr = (cTriRec)(FAST ? sc.fx_tris : sc.tris);
    const int n_tris = FAST ? sc.n_fx_tris : sc.n_tris;
    for (int j = 0; j < n_tris; ++j) {
      if (tr[j].gate && !group_gate(sc, tr[j].gate, o, d)) {
        if (skips) ++skips->other;
        continue;
      }
      tri_test<SHADOW>(tr + j, o, d, h);
    }
  }
  if constexpr (CSG)
    csg_units<SHADOW, false, DEEP, RUNS>(sc, FAST ? sc.fx_units : sc.csg_units, FAST ? sc.n_fx_units : sc.n_csg_units, o, d, h,
                                   n_disc, skips);
  if constexpr (ALIAS) alias_classes<SHADOW>(sc, o, d, h, n_disc, skips);
}

// The group gates trace_rest<.., QUADS, true> meets, without its tests: a counted
// launch's ray that is answered before trace_rest runs (shadow_trace's `first`)
// still owes the reference's count of the shapes its groups kept out.
template <bool QUADS, bool TRIS = QUADS, bool CSG = false, bool ALIAS = false>
__device__ __forceinline__ void count_rest_gates(const DevScene& sc, V3 o, V3 d, GateSkips& sk) {
  if (!sc.n_groups) return;
  if constexpr (ALIAS) count_alias_gates(sc, o, d, sk);
  if constexpr (CSG) {
    Hit none;
    hit_init(none);
    unsigned nd = 0;
    csg_units<true, true>(sc, sc.fx_units, sc.n_fx_units, o, d, none, nd, &sk);
  }
  cSphereGen sg = (cSphereGen)sc.fx_gen;
  for (int j = 0; j < sc.n_fx_gen; ++j)
    if (sg[j].gate && !group_gate(sc, sg[j].gate, o, d)) ++sk.sph;
  cPlaneRec pl = (cPlaneRec)sc.planes;
  for (int j = 0; j < sc.n_planes; ++j)
    if (pl[j].gate && !group_gate(sc, pl[j].gate, o, d)) ++sk.plane;
  if constexpr (QUADS) {
    cQuadRec qr = (cQuadRec)sc.fx_quads;
    for (int j = 0; j < sc.n_fx_quads; ++j)
      if (qr[j].gate && !group_gate(sc, qr[j].gate, o, d)) ++sk.other;
  }
  if constexpr (TRIS) {
    cTriRec tr = (cTriRec)sc.fx_tris;
    for (int j = 0; j < sc.n_fx_tris; ++j)
      if (tr[j].gate && !group_gate(sc, tr[j].gate, o, d)) ++sk.other;
  }
}

// One culled other record (rt_layout.hpp OtherRec) with exactly the
// operations of the exhaustive loops above: a general sphere as trace_rest's
// general records, a solid as quad_test; a record inside groups only when the
// ray meets every group box around it (group_gate, as trace_rest).
template <bool SHADOW>
__device__ __forceinline__ void other_test(const DevScene& sc, const OtherRec* q, V3 o, V3 d, Hit& h,
                                           unsigned& n_disc) {
  if (q->gate && !group_gate(sc, q->gate, o, d)) return;  // Group::intersect (group.rs:49-58)
  if (q->kind == 0) {
    const double* m = q->m;
    const V3 lo = m34_point(m, o);
    const V3 ld = v3(m[0] * d.x + m[1] * d.y + m[2] * d.z, m[4] * d.x + m[5] * d.y + m[6] * d.z,
                     m[8] * d.x + m[9] * d.y + m[10] * d.z);
    sphere_test<SHADOW>(lo.x, lo.y, lo.z, ld.x, ld.y, ld.z, [&] { return (int)q->meta; }, h, n_disc);
  } else {
    quad_test<SHADOW>(q, o, d, h);
  }
}

// One diagonal-inverse sphere record (global memory, scalar loads).
template <bool SHADOW>
__device__ __forceinline__ void diag_test(cSphereDiag r, V3 o, V3 d, Hit& h, unsigned& n_disc) {
  // off-diagonal inverse entries are exact zeros: ((m00*x + 0) + 0) + m03 == m00*x + m03
  const double s0 = r->s[0], s1 = r->s[1], s2 = r->s[2];
  sphere_test<SHADOW>(s0 * o.x + r->t[0], s1 * o.y + r->t[1], s2 * o.z + r->t[2], s0 * d.x, s1 * d.y, s2 * d.z,
                      [&] { return (int)r->meta; }, h, n_disc);
}

// Generic exhaustive trace over the scene's records in global memory (scalar
// loads): the batch entry points (rt_hit_batch, rt_is_shadowed_batch) and
// the wavefront fallback when the trace image does not fit in LDS.
// TRIS = false: a scene without solids or triangles (trace_rest). CSG: one with Csg units.
// ALIAS (with CSG): one with alias classes.
// DEEP (with CSG): the deep units' evaluator too (csg_units). RUNS: the run hierarchies' walk too.
template <bool SHADOW, bool TRIS = true, bool CSG = false, bool ALIAS = false, bool DEEP = true, bool RUNS = false>
__device__ __forceinline__ void trace(const DevScene& sc, V3 o, V3 d, Hit& h, unsigned& n_disc,
                                      GateSkips* skips = nullptr) {
  hit_init(h);
  cSphereDiag sd = (cSphereDiag)sc.sph_diag;
  for (int j = 0; j < sc.n_diag; ++j) diag_test<SHADOW>(sd + j, o, d, h, n_disc);
  trace_rest<SHADOW, true, false, TRIS, CSG, ALIAS, DEEP, RUNS>(sc, o, d, h, n_disc, skips);
  hit_finish(h);
  if constexpr (ALIAS && !SHADOW) alias_finish(sc, h);
}

// --------------------------------------------------------------- shading
struct Comps {
  V3 point, over, under, eyev, normal;
  double n1, n2;
  int obj;
  bool inside;
};

// Shape::local_normal_at per kind (sphere.rs:64-67, plane.rs:62-64,
// cube.rs:95-106, cylinder.rs:121-130, cone.rs:136-149).
__device__ __forceinline__ V3 local_normal_at(const ShadeRec& s, V3 p) {
  switch (s.kind) {
    case 0: return vsub(p, v3(0.0, 0.0, 0.0));
    case 1: return v3(0.0, 1.0, 0.0);
    case 2: {
      const double maxc = fmax(fmax(fabs(p.x), fabs(p.y)), fabs(p.z));
      if (req(maxc, fabs(p.x))) return v3(p.x, 0.0, 0.0);
      if (req(maxc, fabs(p.y))) return v3(0.0, p.y, 0.0);
      return v3(0.0, 0.0, p.z);
    }
    default: {
      const double dist = p.x * p.x + p.z * p.z;
      if (dist < 1.0 && p.y >= s.maximum - kEpsilon) return v3(0.0, 1.0, 0.0);
      if (dist < 1.0 && p.y <= s.minimum + kEpsilon) return v3(0.0, -1.0, 0.0);
      if (s.kind == 3) return v3(p.x, 0.0, p.z);
      double y = sqrt(p.x * p.x + p.z * p.z);
      if (p.y > 0.0) y = -y;
      return v3(p.x, y, p.z);
    }
  }
}

// Triangle::local_normal_at (triangle.rs:92-94): the stored normal; SmoothTriangle's
// (smooth_triangle.rs:103-105): n2 * u + n3 * v + n1 * (1 - u - v) with the hit
// intersection's u and v. `Hit` does not carry them: they are computed again here from
// the same world ray and the same record values with tri_test's operations, so they
// are the intersection's own bits (a hit passed every rejection there, so only u and
// v are taken). Out of line: the kernels keep their registers for the walks.
__device__ __attribute__((noinline)) V3 tri_local_normal(const TriShade* tsp, const double* m, int kind, V3 o, V3 d) {
  const TriShade& ts = *tsp;
  if (kind == 5) return v3(ts.normal[0], ts.normal[1], ts.normal[2]);
  const V3 lo = m34_point(m, o);
  const V3 ld = v3(m[0] * d.x + m[1] * d.y + m[2] * d.z, m[4] * d.x + m[5] * d.y + m[6] * d.z,
                   m[8] * d.x + m[9] * d.y + m[10] * d.z);
  double t = 0.0, u = 0.0, v = 0.0;
  (void)tri_local_intersect(v3(ts.p1[0], ts.p1[1], ts.p1[2]), v3(ts.e1[0], ts.e1[1], ts.e1[2]),
                            v3(ts.e2[0], ts.e2[1], ts.e2[2]), lo, ld, t, u, v);
  const V3 n1 = v3(ts.n1[0], ts.n1[1], ts.n1[2]), n2 = v3(ts.n2[0], ts.n2[1], ts.n2[2]);
  const V3 n3 = v3(ts.n3[0], ts.n3[1], ts.n3[2]);
  return vadd(vadd(vscale(n2, u), vscale(n3, v)), vscale(n1, 1.0 - u - v));
}

// A SmoothTriangle under a Csg: the intersection's u and v are those of the ray the
// triangle was handed, the world ray through the inverse of each Csg above it, outermost
// first, each one rounded (csg_wide_eval's chain), then the triangle's own. `node`: the
// innermost CsgRec above it (TriShade::csg - 1); at most kCsgMaxDepth levels.
__device__ __attribute__((noinline)) V3 csg_tri_local_normal(const CsgRec* node, const TriShade* tsp, const double* m, V3 o,
                                                             V3 d) {
  const CsgRec* unit = node - node->self;
  int depth = 0;
  for (int g = node->self; g >= 0; g = unit[g].parent) ++depth;
  for (int lvl = depth - 1; lvl >= 0; --lvl) {
    int g = node->self;
    for (int k = 0; k < lvl; ++k) g = unit[g].parent;
    const double* c = unit[g].m;
    const V3 lo = m34_point(c, o);
    d = v3(c[0] * d.x + c[1] * d.y + c[2] * d.z, c[4] * d.x + c[5] * d.y + c[6] * d.z, c[8] * d.x + c[9] * d.y + c[10] * d.z);
    o = lo;
  }
  return tri_local_normal(tsp, m, 6, o, d);
}

// Intersection::prepare_computations (intersection.rs:53-105) with the exact
// top-2 replacement of the containers walk.
// TRIS = false: the kernels of scenes without triangles leave their normals out.
// CSG: the kernels of scenes with Csg units (a smooth triangle may lie under one).
template <bool TRIS = true, bool CSG = false>
__device__ __forceinline__ Comps prepare(const DevScene& sc, V3 o, V3 d, const Hit& h) {
  Comps c;
  const int obj = h.key >> kKeyShift;
  const ShadeRec& s = sc.shade[obj];
  c.obj = obj;
  c.point = vadd(o, vscale(d, h.t));  // ray.rs:22-24
  c.eyev = vneg(d);
  // Shape::normal_at (geometry/mod.rs:51-56)
  const V3 lp = m34_point(s.inv, c.point);
  V3 ln;
  if (TRIS && s.kind >= 5) {
    const TriShade* ts = sc.tri_shade + (s.pad0 - 1);
    if (CSG && s.kind == 6 && ts->csg) ln = csg_tri_local_normal(sc.csg_nodes + (ts->csg - 1), ts, s.inv, o, d);
    else ln = tri_local_normal(ts, s.inv, s.kind, o, d);
  } else {
    ln = local_normal_at(s, lp);
  }
  V3 n = vnormalize(m33_vector(s.invT, ln));
  c.inside = false;
  if (vdot(n, c.eyev) < 0.0) { c.inside = true; n = vneg(n); }
  c.normal = n;
  // n1 / n2 (intersection.rs:63-90, DESIGN.md "containers walk -> top-2"):
  // n1 = last container before the hit; n2 = last after toggling the hit object
  c.n1 = h.c1k >= 0 ? sc.shade[h.c1k >> kKeyShift].refractive_index : 1.0;
  if (!h.hin) {
    c.n2 = s.refractive_index;
  } else if ((h.c1k >> kKeyShift) == obj) {
    c.n2 = h.c2k >= 0 ? sc.shade[h.c2k >> kKeyShift].refractive_index : 1.0;
  } else {
    c.n2 = sc.shade[h.c1k >> kKeyShift].refractive_index;
  }
  c.over = vadd(c.point, vscale(n, kEpsilon));
  c.under = vsub(c.point, vscale(n, kEpsilon));
  return c;
}

// Computations::schlick (intersection.rs:147-162); powi(2) = q*q,
// powi(5) = x*((x*x)*(x*x)) (LLVM powi expansion / __powidf2).
__device__ __forceinline__ double schlick(V3 eyev, V3 normal, double n1, double n2) {
  double cosv = vdot(eyev, normal);
  if (n1 > n2) {
    const double nn = n1 / n2;
    const double sin2_t = nn * nn * (1.0 - cosv * cosv);
    if (sin2_t > 1.0) return 1.0;
    cosv = sqrt(1.0 - sin2_t);
  }
  const double q = (n1 - n2) / (n1 + n2);
  const double r0 = q * q;
  const double x = 1.0 - cosv;
  const double x5 = x * ((x * x) * (x * x));
  return r0 + (1.0 - r0) * x5;
}

// `v % 2.0 == 0.0` (Rust's f64 `%` is fmod) for an integer-valued or
// non-finite v, without the fmod loop: binary64 values of magnitude >= 2^53
// are even integers, below that the integer conversion is exact.
__device__ __forceinline__ bool fmod2_is_zero(double v) {
  if (!(fabs(v) < 0x1p53)) return !isnan(v) && !isinf(v);
  return (((long long)v) & 1) == 0;
}

// componentwise select (a select between whole structs becomes a scratch
// copy indexed by the condition)
__device__ __forceinline__ V3 vsel(bool c, V3 a, V3 b) { return v3(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z); }

// Pattern::color_at_shape (pattern/mod.rs:39-49) and the five kinds.
__device__ __forceinline__ V3 pattern_color(const ShadeRec& s, V3 world_point) {
  const V3 op = m34_point(s.inv, world_point);
  const V3 pp = m34_point(s.pat_inv, op);
  const V3 a = v3(s.pat_a[0], s.pat_a[1], s.pat_a[2]);
  const V3 b = v3(s.pat_b[0], s.pat_b[1], s.pat_b[2]);
  switch (s.pattern_kind) {
    case 0:  // test_pattern.rs:7-9
      return pp;
    case 1:  // stripe.rs:14-20
      return vsel(fmod2_is_zero(floor(pp.x)), a, b);
    case 2: {  // gradient.rs:14-18
      const V3 distance = vsub(b, a);
      const double fraction = pp.x - floor(pp.x);
      return vadd(a, vscale(distance, fraction));
    }
    case 3: {  // ring.rs:14-21
      const double distance = floor(sqrt(pp.x * pp.x + pp.z * pp.z));
      return vsel(fmod2_is_zero(distance), a, b);
    }
    default: {  // checkers.rs:14-21: `as isize` (saturating) then % 2
      const double distance = floor(pp.x) + floor(pp.y) + floor(pp.z);
      bool even;
      if (isnan(distance)) even = true;                          // NaN as isize = 0
      else if (distance >= 9223372036854775808.0) even = false;  // isize::MAX is odd
      else if (distance < -9223372036854775808.0) even = true;   // isize::MIN is even
      else even = fmod2_is_zero(distance);                      // exact integer parity
      return vsel(even, a, b);
    }
  }
}

// f64::powf of the specular term (material.rs:76): glibc 2.35's pow, operation
// for operation (rt_pow.hpp), so the colours are the reference host's bit for
// bit (OCML's pow differed by 1-2 ulps in about 1 of 4000 channels, round 5);
// the frame costs the same (profiles/r06_ab_pow.txt: +0.2 %, within noise).
// Out of line: inlined into the fused trace kernels, its constants were hoisted
// out of the ray loop into VGPRs and spilled across the BVH traversal.
__device__ __attribute__((noinline)) double spec_pow(double x, double y) { return pow_glibc(x, y); }

// Material::lighting (material.rs:38-82)
// `lightv` = (light.position - point).normalize(), which the caller may
// already hold: the shadow ray from `point` to the light has exactly that
// direction (same operands, same operations), so the shadow trace passes it.
__device__ __forceinline__ V3 lighting(const ShadeRec& m, cLightRec L, V3 point, V3 eyev, V3 normal,
                                       bool in_shadow, V3 lightv) {
  const V3 color = m.pattern_kind >= 0 ? pattern_color(m, point)
                                       : v3(m.color[0], m.color[1], m.color[2]);
  const V3 intensity = v3(L->intensity[0], L->intensity[1], L->intensity[2]);
  const V3 effective_color = vmul(color, intensity);
  const V3 ambient = vscale(effective_color, m.ambient);
  if (in_shadow) return ambient;
  const double light_dot_normal = vdot(lightv, normal);
  V3 diffuse = v3(0.0, 0.0, 0.0), specular = v3(0.0, 0.0, 0.0);
  if (!(light_dot_normal < 0.0)) {
    diffuse = vscale(vscale(effective_color, m.diffuse), light_dot_normal);
    const V3 reflectv = vreflect(vneg(lightv), normal);
    const double reflect_dot_eye = vdot(reflectv, eyev);
    if (!(reflect_dot_eye <= 0.0)) {
      // A material without specular (e.g. the C3/C5 floors): (I * 0) * f equals
      // I * 0 bit for bit whenever f = pow(x, y) is finite and not -0, which holds
      // for 0 < x <= 1 and 0 <= y < inf (f in [0, 1]); then pow need not run.
      const bool no_spec = m.specular == 0.0 && reflect_dot_eye <= 1.0 && m.shininess >= 0.0 &&
                           m.shininess < INFINITY && fabs(intensity.x) < INFINITY &&
                           fabs(intensity.y) < INFINITY && fabs(intensity.z) < INFINITY;
      if (no_spec) {
        specular = vscale(intensity, m.specular);
      } else {
        const double factor = spec_pow(reflect_dot_eye, m.shininess);
        specular = vscale(vscale(intensity, m.specular), factor);
      }
    }
  }
  return vadd(vadd(ambient, diffuse), specular);
}
__device__ __forceinline__ V3 lighting(const ShadeRec& m, cLightRec L, V3 point, V3 eyev, V3 normal,
                                       bool in_shadow) {
  return lighting(m, L, point, eyev, normal, in_shadow,
                  vnormalize(vsub(v3(L->pos[0], L->pos[1], L->pos[2]), point)));
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// camera.rs:57-69 (offsets 0.5, 0.5) and rays_for_pixel (camera.rs:71-90)
// with the AA sample offsets of get_offsets (camera.rs:92-126).
__device__ __forceinline__ void ray_for_pixel(const DevCamera& cam, uint32_t px, uint32_t py, V3& o, V3& d,
                                              double offx = 0.5, double offy = 0.5) {
  const double xoffset = ((double)px + offx) * cam.pixel_size;
  const double yoffset = ((double)py + offy) * cam.pixel_size;
  const double world_x = cam.half_width - xoffset;
  const double world_y = cam.half_height - yoffset;
  const V3 pixel = m34_point(cam.inv, v3(world_x, world_y, -1.0));
  o = m34_point(cam.inv, v3(0.0, 0.0, 0.0));
  d = vnormalize(vsub(pixel, o));
}

}  // namespace rtamd
