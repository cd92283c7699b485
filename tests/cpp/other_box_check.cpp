// other_box_check.cpp — other_box, line_box and build_other_bvh (rt_bvh.cpp) against a plain restatement.
//
// The contract under test, for every finite ray (o, d) with |d|_inf >= kOtherDirMin (the rays
// other_trace walks with; line_trace takes any ray, and is given those from |o|_inf <= kOtherOriginMax):
//  (a) every finite root t of a record that has a box has o + t d inside that box when |o|_inf <=
//      kOtherOriginMax, and for other_box from a farther origin inside that box grown on each axis by
//      other_far_pad (rt_layout.hpp; taken with the record's own box for the hierarchy's bound, the
//      smallest growth any hierarchy that holds the record gives it). For line_box a cone's a ~ 0
//      branch is left out: cone_prepass owns it;
//  (b) for a record other_box accepts: an odd number of roots at t < 0 means the origin is inside the
//      box, EXCEPT for the records other_needs_line names (the closed cylinders: with dx^2 + dz^2 <
//      EPSILON only their caps are tested, and one cap root can lie behind an origin outside the box).
//      Those are culled over the ray's whole line, for which (a) is all that is needed; build_other_bvh
//      must flag every child that holds one (BvhNode::line), which (d) checks;
//  (c) the refusals: cones and open or unbounded tubes in other_box, closed tubes and solids in
//      line_box, min > max, NaN bounds, a condition number above 1e6, non-finite matrices;
//  (d) build_other_bvh over 40 records: every record once, every box inside its parent's, the depth
//      bound, the line flags.
// sphere.rs:47-62, cube.rs:30-93, cylinder.rs:42-119 and cone.rs:48-134 are restated here in plain
// doubles with the device's operation order (the inverse's rows applied as quad_test does). Build with
// -ffp-contract=off. Linked against an rt_bvh.cpp without other_needs_line, (b) holds every record to
// the closed-solid rule.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rt_bvh.hpp"

namespace rtamd {
bool other_needs_line(const OtherRec& r) __attribute__((weak));
}
using namespace rtamd;

namespace {

struct Rng {
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  double u() { return (double)(next() >> 11) * 0x1p-53; }
  double range(double a, double b) { return a + (b - a) * u(); }
  int below(int n) { return (int)(next() % (uint64_t)n); }
  double sign() { return below(2) ? 1.0 : -1.0; }
};

struct V {
  double x, y, z;
};
V operator+(V a, V b) { return V{a.x + b.x, a.y + b.y, a.z + b.z}; }
V operator*(double s, V a) { return V{s * a.x, s * a.y, s * a.z}; }
double norm(V v) { return std::sqrt(v.x * v.x + v.y * v.y + v.z * v.z); }
double norm_inf(V v) { return std::fmax(std::fabs(v.x), std::fmax(std::fabs(v.y), std::fabs(v.z))); }
V unit(V v) { return (1.0 / norm(v)) * v; }
V cross(V a, V b) { return V{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

// 3x4 affine maps, rows 0..2
struct M34 {
  double m[12];
};
M34 mul(const M34& a, const M34& b) {
  M34 r{};
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j)
      for (int k = 0; k < 3; ++k) r.m[4 * i + j] += a.m[4 * i + k] * b.m[4 * k + j];
    r.m[4 * i + 3] = a.m[4 * i + 3];
    for (int k = 0; k < 3; ++k) r.m[4 * i + 3] += a.m[4 * i + k] * b.m[4 * k + 3];
  }
  return r;
}
M34 scaling(double x, double y, double z) { return M34{{x, 0, 0, 0, 0, y, 0, 0, 0, 0, z, 0}}; }
M34 translation(double x, double y, double z) { return M34{{1, 0, 0, x, 0, 1, 0, y, 0, 0, 1, z}}; }
M34 shearing(double xy, double xz, double yx, double yz, double zx, double zy) {
  return M34{{1, xy, xz, 0, yx, 1, yz, 0, zx, zy, 1, 0}};
}
M34 rotation(int axis, double r) {
  const double c = std::cos(r), s = std::sin(r);
  if (axis == 0) return M34{{1, 0, 0, 0, 0, c, -s, 0, 0, s, c, 0}};
  if (axis == 1) return M34{{c, 0, s, 0, 0, 1, 0, 0, -s, 0, c, 0}};
  return M34{{c, -s, 0, 0, s, c, 0, 0, 0, 0, 1, 0}};
}
// the inverse by cofactors; *cond = |A|_inf |A^-1|_inf of the 3x3 part
M34 inverse(const M34& f, double* cond) {
  const double* m = f.m;
  const double a[3][3] = {{m[0], m[1], m[2]}, {m[4], m[5], m[6]}, {m[8], m[9], m[10]}};
  double c[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
      c[i][j] = a[i1][j1] * a[i2][j2] - a[i1][j2] * a[i2][j1];
    }
  const double det = a[0][0] * c[0][0] + a[0][1] * c[0][1] + a[0][2] * c[0][2];
  M34 r{};
  double na = 0.0, ni = 0.0;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) r.m[4 * i + j] = c[j][i] / det;
    r.m[4 * i + 3] = -(r.m[4 * i] * m[3] + r.m[4 * i + 1] * m[7] + r.m[4 * i + 2] * m[11]);
    na = std::fmax(na, std::fabs(a[i][0]) + std::fabs(a[i][1]) + std::fabs(a[i][2]));
    ni = std::fmax(ni, std::fabs(r.m[4 * i]) + std::fabs(r.m[4 * i + 1]) + std::fabs(r.m[4 * i + 2]));
  }
  if (cond) *cond = na * ni;
  return r;
}
V point(const M34& f, V p) {
  const double* m = f.m;
  return V{m[0] * p.x + m[1] * p.y + m[2] * p.z + m[3], m[4] * p.x + m[5] * p.y + m[6] * p.z + m[7],
           m[8] * p.x + m[9] * p.y + m[10] * p.z + m[11]};
}
V vec(const M34& f, V p) {
  const double* m = f.m;
  return V{m[0] * p.x + m[1] * p.y + m[2] * p.z, m[4] * p.x + m[5] * p.y + m[6] * p.z,
           m[8] * p.x + m[9] * p.y + m[10] * p.z};
}

constexpr double EPS = 0.00001;  // lib.rs:18

void check_axis(double origin, double direction, double& tmin, double& tmax) {
  const double a = -1.0 - origin, b = 1.0 - origin;
  if (std::fabs(direction) >= EPS) { tmin = a / direction; tmax = b / direction; }
  else { tmin = a * INFINITY; tmax = b * INFINITY; }
  if (tmin > tmax) { const double x = tmin; tmin = tmax; tmax = x; }
}
bool check_cap(V o, V d, double t, double radius) {
  const double x = o.x + t * d.x, z = o.z + t * d.z;
  return (x * x + z * z) <= radius * radius;
}
int caps(const OtherRec& q, V o, V d, double* t, int n) {
  if (!q.closed) return n;
  const bool cone = q.kind == 4;
  double tc = (q.minimum - o.y) / d.y;
  if (check_cap(o, d, tc, cone ? q.minimum : 1.0)) t[n++] = tc;
  tc = (q.maximum - o.y) / d.y;
  if (check_cap(o, d, tc, cone ? q.maximum : 1.0)) t[n++] = tc;
  return n;
}
// the roots of one record on its local ray; *degenerate: a cone's a ~ 0 branch was taken
int local_roots(const OtherRec& q, V o, V d, double t[4], bool* degenerate) {
  *degenerate = false;
  if (q.kind == 0) {
    const double a = d.x * d.x + d.y * d.y + d.z * d.z;
    const double dt = d.x * o.x + d.y * o.y + d.z * o.z;
    const double c = o.x * o.x + o.y * o.y + o.z * o.z - 1.0;
    const double disc = dt * dt - a * c;
    if (!(disc >= 0.0)) return 0;
    const double s = std::sqrt(disc);
    t[0] = (-dt - s) / a;
    t[1] = (-dt + s) / a;
    return 2;
  }
  if (q.kind == 2) {
    double x0, x1, y0, y1, z0, z1;
    check_axis(o.x, d.x, x0, x1);
    check_axis(o.y, d.y, y0, y1);
    check_axis(o.z, d.z, z0, z1);
    const double tmin = std::fmax(std::fmax(x0, y0), z0), tmax = std::fmin(std::fmin(x1, y1), z1);
    if (tmin > tmax) return 0;
    t[0] = tmin;
    t[1] = tmax;
    return 2;
  }
  double a, b, c;
  if (q.kind == 3) {
    a = d.x * d.x + d.z * d.z;
    if (std::fabs(a) < EPS) return caps(q, o, d, t, 0);
    b = 2.0 * o.x * d.x + 2.0 * o.z * d.z;
    c = o.x * o.x + o.z * o.z - 1.0;
  } else {
    a = d.x * d.x - d.y * d.y + d.z * d.z;
    b = 2.0 * o.x * d.x - 2.0 * o.y * d.y + 2.0 * o.z * d.z;
    c = o.x * o.x - o.y * o.y + o.z * o.z;
    if (std::fabs(a) < EPS) {
      *degenerate = true;
      if (std::fabs(b) < EPS) return caps(q, o, d, t, 0);
      t[0] = -c / 2.0 * b;
      return caps(q, o, d, t, 1);
    }
  }
  const double disc = b * b - 4.0 * a * c;
  if (disc < 0.0) return 0;
  const double s = std::sqrt(disc);
  const double t0 = (-b - s) / (2.0 * a), t1 = (-b + s) / (2.0 * a);
  int n = 0;
  const double y0 = o.y + t0 * d.y;
  if (q.minimum < y0 && y0 < q.maximum) t[n++] = t0;
  const double y1 = o.y + t1 * d.y;
  if (q.minimum < y1 && y1 < q.maximum) t[n++] = t1;
  return caps(q, o, d, t, n);
}

int failures = 0;
#define CHECK(c, ...)                                  \
  do {                                                 \
    if (!(c)) {                                        \
      if (++failures <= 12) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                  \
  } while (0)

struct Rec {
  OtherRec r;
  M34 fwd;
  double cond;
};
enum Shape { kSphere, kCube, kClosedCyl, kOpenCyl, kCone };

// translation . rotations . shearing . scaling, scales log-uniform in [1e-3, 1e3]
Rec make_rec(Rng& g, Shape shape, int variant) {
  Rec out{};
  double s[3];
  const double base = std::pow(10.0, g.range(-3.0, 3.0));
  // variant 0: near-uniform; 1: anisotropic within [1e-3, 1e3]; 2: condition just below 1e6
  for (int a = 0; a < 3; ++a) {
    const double spread = variant == 0 ? 0.3 : variant == 1 ? 3.0 : 0.0;
    s[a] = std::fmin(1e3, std::fmax(1e-3, base * std::pow(10.0, g.range(-spread, spread))));
  }
  if (variant == 2) {
    const double lo = std::pow(10.0, g.range(-3.0, -2.7)), ratio = std::pow(10.0, g.range(5.0, 5.7));
    s[0] = lo; s[1] = lo * ratio; s[2] = lo * std::sqrt(ratio);
    std::swap(s[g.below(3)], s[0]);
  }
  const bool plain = variant != 2 && g.below(4) == 0;  // a quarter without shear (and variant 2: rotations only)
  M34 f = scaling(s[0], s[1], s[2]);
  if (!plain && variant != 2)
    f = mul(shearing(g.range(-0.5, 0.5), g.range(-0.5, 0.5), g.range(-0.5, 0.5), g.range(-0.5, 0.5), g.range(-0.5, 0.5),
                     g.range(-0.5, 0.5)), f);
  if (variant == 2) {  // a quarter turn about a random axis keeps the condition at the scales' ratio
    f = mul(rotation(g.below(3), 1.5707963267948966 * g.below(4)), f);
  } else if (g.below(5) != 0) {
    f = mul(rotation(2, g.range(-3.0, 3.0)), mul(rotation(1, g.range(-3.0, 3.0)), mul(rotation(0, g.range(-3.0, 3.0)), f)));
  }
  f = mul(translation(g.range(-8.0, 8.0), g.range(-8.0, 8.0), g.range(-8.0, 8.0)), f);
  out.fwd = f;
  const M34 inv = inverse(f, &out.cond);
  std::memcpy(out.r.m, inv.m, sizeof out.r.m);
  out.r.kind = shape == kSphere ? 0 : shape == kCube ? 2 : shape == kCone ? 4 : 3;
  out.r.closed = shape == kClosedCyl || (shape == kCone && g.below(2));
  out.r.minimum = -INFINITY;
  out.r.maximum = INFINITY;
  if (out.r.kind >= 3) {
    const int b = g.below(5);
    out.r.minimum = g.range(-2.0, 0.5);
    out.r.maximum = out.r.minimum + g.range(0.2, 3.0);
    if (b == 0) out.r.maximum = out.r.minimum;                         // min == max
    if (b == 1 && out.r.kind == 3) out.r.maximum = out.r.minimum + 1e3;  // a long thin tube: 1e3 radii
    if (b == 2 && out.r.kind == 4) { out.r.minimum = -1.0; out.r.maximum = 0.0; }
  }
  return out;
}

struct Tally {
  long rays = 0, roots = 0, odd_behind = 0, band = 0, skipped = 0, far = 0;
};

// (a) and (b) for one ray; `line`: the record is culled over the whole line
void check_ray(const Rec& rc, const double* lo, const double* hi, bool other, bool line, V o, V d, Tally& tl,
               const char* what) {
  const double om = norm_inf(o);
  if (!(norm_inf(d) >= kOtherDirMin && norm_inf(d) < INFINITY && om < INFINITY)) { ++tl.skipped; return; }
  double glo[3] = {lo[0], lo[1], lo[2]}, ghi[3] = {hi[0], hi[1], hi[2]};
  if (om > kOtherOriginMax) {  // other_trace's far origins: the box grown for this ray
    if (!other) { ++tl.skipped; return; }
    double m[3], mm = 0.0;
    for (int a = 0; a < 3; ++a) { m[a] = std::fmax(std::fabs(lo[a]), std::fabs(hi[a])); mm = std::fmax(mm, m[a]); }
    for (int a = 0; a < 3; ++a) {
      const double grow = other_far_pad((double)(float)m[a], (double)(float)mm, om);
      if (!(grow >= 0.0)) { ++tl.skipped; return; }
      glo[a] -= grow;
      ghi[a] += grow;
    }
    ++tl.far;
  }
  const OtherRec& q = rc.r;
  const M34& inv = *(const M34*)q.m;
  const V lo3 = point(inv, o), ld3 = vec(inv, d);
  double t[4];
  bool degenerate;
  const int n = local_roots(q, lo3, ld3, t, &degenerate);
  ++tl.rays;
  if (degenerate) return;
  if (q.kind == 2 && (std::fabs(ld3.x) < EPS || std::fabs(ld3.y) < EPS || std::fabs(ld3.z) < EPS) && n) ++tl.band;
  if (q.kind == 3 && std::fabs(ld3.x * ld3.x + ld3.z * ld3.z) < EPS && n) ++tl.band;
  int behind = 0;
  for (int i = 0; i < n; ++i) {
    if (t[i] < 0.0) ++behind;
    if (!std::isfinite(t[i])) continue;
    ++tl.roots;
    const double p[3] = {o.x + t[i] * d.x, o.y + t[i] * d.y, o.z + t[i] * d.z};
    for (int a = 0; a < 3; ++a)
      CHECK(p[a] >= glo[a] && p[a] <= ghi[a],
            "(a) %s: kind %d cond %.3g root %.17g: p[%d] = %.17g outside [%.17g, %.17g]; o (%.17g, %.17g, %.17g) d (%.17g, "
            "%.17g, %.17g)",
            what, q.kind, rc.cond, t[i], a, p[a], glo[a], ghi[a], o.x, o.y, o.z, d.x, d.y, d.z);
  }
  if (other && (behind & 1)) {
    ++tl.odd_behind;
    if (!line) {
      const double p[3] = {o.x, o.y, o.z};
      for (int a = 0; a < 3; ++a)
        CHECK(p[a] >= lo[a] && p[a] <= hi[a],
              "(b) %s: kind %d closed %d: %d of %d roots behind an origin outside the box: o[%d] = %.17g outside [%.17g, "
              "%.17g]; o (%.17g, %.17g, %.17g) d (%.17g, %.17g, %.17g)",
              what, q.kind, q.closed, behind, n, a, p[a], lo[a], hi[a], o.x, o.y, o.z, d.x, d.y, d.z);
    }
  }
}

// a point of the record's region in object space (f: how far out, 1 = up to the surface)
V region_point(Rng& g, const OtherRec& q, double f) {
  V p{f * g.range(-1, 1), f * g.range(-1, 1), f * g.range(-1, 1)};
  if (q.kind == 0) p = (f * std::cbrt(g.u())) * unit(V{g.range(-1, 1), g.range(-1, 1), g.range(-1, 1)});
  if (q.kind >= 3) {
    p.y = q.minimum + (q.maximum - q.minimum) * g.u();
    const double rad = (q.kind == 4 ? std::fabs(p.y) : 1.0) * f * std::sqrt(g.u()), ang = g.range(0.0, 6.283185307179586);
    p.x = rad * std::cos(ang);
    p.z = rad * std::sin(ang);
  }
  return p;
}
// a point on the record's surface and a tangent direction there
void surface_point(Rng& g, const OtherRec& q, V* p, V* tangent) {
  V nrm;
  if (q.kind == 0) {
    *p = unit(V{g.range(-1, 1), g.range(-1, 1), g.range(-1, 1)});
    nrm = *p;
  } else if (q.kind == 2) {
    double c[3] = {g.range(-1, 1), g.range(-1, 1), g.range(-1, 1)};
    const int ax = g.below(3);
    c[ax] = g.sign();
    if (g.below(3) == 0) c[(ax + 1) % 3] = g.sign();  // an edge
    *p = V{c[0], c[1], c[2]};
    nrm = V{ax == 0 ? 1.0 : 0.0, ax == 1 ? 1.0 : 0.0, ax == 2 ? 1.0 : 0.0};
  } else {
    const double y = g.below(4) == 0 ? (g.below(2) ? q.minimum : q.maximum) : q.minimum + (q.maximum - q.minimum) * g.u();
    const double rad = q.kind == 4 ? std::fabs(y) : 1.0, ang = g.range(0.0, 6.283185307179586);
    *p = V{rad * std::cos(ang), y, rad * std::sin(ang)};
    nrm = q.kind == 4 ? V{p->x, -y, p->z} : V{p->x, 0.0, p->z};
    if (norm(nrm) == 0.0) nrm = V{0, 1, 0};
  }
  V r{g.range(-1, 1), g.range(-1, 1), g.range(-1, 1)};
  *tangent = cross(nrm, r);
  if (norm(*tangent) == 0.0) *tangent = V{1, 0, 0};
}

// the world ray of an object-space origin and direction
void to_world(const Rec& rc, V lo3, V ld3, V* o, V* d) {
  *o = point(rc.fwd, lo3);
  *d = unit(vec(rc.fwd, ld3));
}

// the crafted rays of one record: object-space directions with components at the thresholds
void crafted(Rng& g, const Rec& rc, const double* lo, const double* hi, bool other, bool line, int n_rays, Tally& tl) {
  const OtherRec& q = rc.r;
  // component targets, in units of EPSILON, of the object-space direction the device computes
  const double targets[] = {1e-3, 0.3, 0.95, 1.0 - 1e-9, 1.0 + 1e-9, 1.5, 0.0};
  const double edges[] = {1.0, -1.0, 1.0 - 1e-9, -1.0 + 1e-9, 0.0};
  for (int r = 0; r < n_rays; ++r) {
    const int ax = g.below(3);
    double v[3] = {0, 0, 0}, p[3] = {g.range(-1.0, 1.0), g.range(-1.0, 1.0), g.range(-1.0, 1.0)};
    if (r % 4 == 0)
      for (int a = 0; a < 3; ++a) p[a] = g.below(2) ? edges[g.below(5)] : p[a];
    // how far back along the main axis, in world units: up to the domain's longest
    const V col{rc.fwd.m[ax], rc.fwd.m[4 + ax], rc.fwd.m[8 + ax]};
    const double step = norm(col);
    const double world_dist = r % 3 == 0 ? (r % 2 ? g.range(0.5, 0.95) : g.range(1.0, 6.0)) * kOtherOriginMax : std::pow(10.0, g.range(-1.0, 2.5)) * step;
    const double back = g.sign() * (g.below(8) == 0 ? g.range(0.0, 1.0) : 1.0 + world_dist / step);
    V lo3, ld3;
    if (q.kind == 3 || q.kind == 4) {
      // travel along y with dx^2 + dz^2 (the cylinder's a) near EPSILON; a cone's a = dx^2 - dy^2 + dz^2 is far from it
      const double ta = targets[g.below(7)] * EPS, ang = g.range(0.0, 6.283185307179586);
      double vx = 0.0, vz = 0.0;
      for (int it = 0; it < 4; ++it) {
        const double n = norm(vec(rc.fwd, V{vx, 1.0, vz}));
        vx = std::sqrt(ta) * n * std::cos(ang);
        vz = std::sqrt(ta) * n * std::sin(ang);
      }
      if (r % 16 == 0) { vx = 1.0; vz = g.range(-1.0, 1.0); ld3 = V{vx, 0.0, vz}; }  // dy = 0 exactly: the caps divide by zero
      else ld3 = V{vx, g.sign(), vz};
      // the origin: near the wall or the axis, beside the tube, beyond a cap, or far along the axis
      const double len = q.maximum - q.minimum, rad = g.below(2) ? g.range(0.9, 1.1) : g.range(0.0, 2.0);
      const double oa = g.range(0.0, 6.283185307179586);
      const double step_y = norm(V{rc.fwd.m[1], rc.fwd.m[5], rc.fwd.m[9]});
      const double oy = r % 3 == 0 ? g.sign() * (1.0 + (r % 2 ? g.range(0.0, 0.95) : g.range(1.0, 6.0)) * kOtherOriginMax / step_y)
                                   : g.range(q.minimum - 0.5 * len - 1.0, q.maximum + 0.5 * len + 1.0);
      lo3 = V{rad * std::cos(oa), oy, rad * std::sin(oa)};
    } else {
      // travel along `ax`; one or two other components at the targets
      v[ax] = 1.0;
      const int two = g.below(2);
      double tg[3] = {0, 0, 0};
      for (int k = 1; k <= 1 + two; ++k) tg[(ax + k) % 3] = g.sign() * targets[g.below(7)] * EPS;
      for (int it = 0; it < 4; ++it) {
        const double n = norm(vec(rc.fwd, V{v[0], v[1], v[2]}));
        for (int a = 0; a < 3; ++a)
          if (a != ax) v[a] = tg[a] * n;
      }
      p[ax] = back;
      lo3 = V{p[0], p[1], p[2]};
      ld3 = V{v[0], v[1], v[2]};
    }
    V o, d;
    to_world(rc, lo3, ld3, &o, &d);
    check_ray(rc, lo, hi, other, line, o, d, tl, "crafted");
  }
}

void check_records(Rng& g) {
  const int n_recs = 150, n_rays = 2400, n_crafted = 1200;
  int boxed[5] = {0, 0, 0, 0, 0}, near_limit = 0, thin = 0, flat = 0;
  Tally tl;
  for (int k = 0; k < n_recs; ++k) {
    const Shape shape = (Shape)(k % 5);
    const Rec rc = make_rec(g, shape, (k / 5) % 3);
    const OtherRec& q = rc.r;
    double lo[3], hi[3], l2[3], h2[3];
    const bool other = other_box(q, lo, hi);
    const bool lbox = line_box(q, l2, h2);
    CHECK(!(other && lbox), "kind %d closed %d has a box in both hierarchies", q.kind, q.closed);
    if (rc.cond <= 0.99e6) {
      CHECK(other == (shape <= kClosedCyl), "kind %d closed %d cond %.3g: other_box %d", q.kind, q.closed, rc.cond, other);
      CHECK(lbox == (shape >= kOpenCyl), "kind %d closed %d cond %.3g: line_box %d", q.kind, q.closed, rc.cond, lbox);
    }
    if (!other && !lbox) continue;
    if (!other) { std::memcpy(lo, l2, sizeof lo); std::memcpy(hi, h2, sizeof hi); }
    ++boxed[shape];
    if (rc.cond > 1e5) ++near_limit;
    if (q.kind == 3 && q.maximum - q.minimum >= 1e3) ++thin;
    if (q.kind >= 3 && q.maximum == q.minimum) ++flat;
    const bool line = !other || (other_needs_line && other_needs_line(q));
    const double c[3] = {0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2])};
    const double h[3] = {0.5 * (hi[0] - lo[0]), 0.5 * (hi[1] - lo[1]), 0.5 * (hi[2] - lo[2])};
    const double size = std::fmax(h[0], std::fmax(h[1], h[2]));
    for (int r = 0; r < n_rays; ++r) {
      V o, d;
      const int mode = r % 4;
      if (mode == 0) {  // random: from near or far towards a point of the box, or anywhere
        const V dir = unit(V{g.range(-1, 1), g.range(-1, 1), g.range(-1, 1)});
        const double far = r % 8 == 0 ? g.range(0.0, r % 16 ? 0.9 : 6.0) * kOtherOriginMax : size * g.range(1.2, 30.0);
        o = V{c[0] + far * dir.x, c[1] + far * dir.y, c[2] + far * dir.z};
        const V aim{c[0] + h[0] * g.range(-1.1, 1.1), c[1] + h[1] * g.range(-1.1, 1.1), c[2] + h[2] * g.range(-1.1, 1.1)};
        d = unit(aim + (-1.0) * o);
        if (r % 12 == 0) {  // exact zeros in the direction
          const int ax = g.below(3);
          d = V{ax == 0 ? g.sign() : 0.0, ax == 1 ? g.sign() : 0.0, ax == 2 ? g.sign() : 0.0};
          o = V{ax == 0 ? o.x : aim.x, ax == 1 ? o.y : aim.y, ax == 2 ? o.z : aim.z};
        }
      } else if (mode == 1) {  // grazing: a tangent through a surface point, from either side, near or far
        V p, tg;
        surface_point(g, q, &p, &tg);
        const V wp = point(rc.fwd, p), wd = unit(vec(rc.fwd, tg));
        const double back = r % 8 == 1 ? g.range(0.0, r % 16 == 1 ? 0.9 : 6.0) * kOtherOriginMax : size * g.range(0.0, 30.0);
        o = wp + (-back) * wd;
        d = g.below(2) ? wd : (-1.0) * wd;
      } else if (mode == 2) {  // from inside the shape, or just inside its surface
        const V p = region_point(g, q, r % 8 == 2 ? 1.0 - 1e-9 : 1.0);
        o = point(rc.fwd, p);
        d = unit(V{g.range(-1, 1), g.range(-1, 1), g.range(-1, 1)});
      } else {  // through a point of the shape, from outside
        const V p = point(rc.fwd, region_point(g, q, 1.0));
        d = unit(V{g.range(-1, 1), g.range(-1, 1), g.range(-1, 1)});
        o = p + (-size * g.range(0.0, 40.0)) * d;
      }
      check_ray(rc, lo, hi, other, line, o, d, tl, "ray");
    }
    crafted(g, rc, lo, hi, other, line, n_crafted, tl);
  }
  for (int s = 0; s < 5; ++s) CHECK(boxed[s] >= n_recs / 5 / 2, "only %d boxed records of shape %d", boxed[s], s);
  CHECK(near_limit >= 10, "only %d boxed records of condition above 1e5", near_limit);
  CHECK(thin >= 3, "only %d boxed tubes 1e3 radii long", thin);
  CHECK(flat >= 3, "only %d boxed records with min == max", flat);
  CHECK(tl.rays > 300000, "only %ld rays in the domain", tl.rays);
  CHECK(tl.roots > 200000, "only %ld roots checked", tl.roots);
  CHECK(tl.far > 20000, "only %ld rays from beyond kOtherOriginMax", tl.far);
  CHECK(tl.band > 5000, "only %ld rays with roots in a parallel band", tl.band);
  CHECK(tl.odd_behind > 20000, "only %ld rays with an odd number of roots behind the origin", tl.odd_behind);
  std::printf("boxed %d %d %d %d %d (cond > 1e5: %d), rays %ld (from far origins: %ld, not held: %ld), roots %ld, in a band %ld, odd behind %ld\n",
              boxed[0], boxed[1], boxed[2], boxed[3], boxed[4], near_limit, tl.rays, tl.far, tl.skipped, tl.roots, tl.band,
              tl.odd_behind);
}

// the two rays of the issue, on the records they were found on
void check_known(Tally& tl) {
  double lo[3], hi[3];
  for (double s : {50.0, 1.0}) {
    Rec cube{};
    cube.fwd = scaling(s, s, s);
    const M34 inv = inverse(cube.fwd, &cube.cond);
    std::memcpy(cube.r.m, inv.m, sizeof cube.r.m);
    cube.r.kind = 2;
    CHECK(other_box(cube.r, lo, hi), "a cube scaled by %g has a box", s);
    if (s == 50.0) check_ray(cube, lo, hi, true, false, V{-600, 49.95, 0}, unit(V{1, 4e-4, 0}), tl, "the scale-50 cube");
    else check_ray(cube, lo, hi, true, false, V{-600, 0.999, 0}, unit(V{1, 9e-6, 0}), tl, "the unit cube");
  }
  Rec cyl{};
  cyl.fwd = scaling(1, 1, 1);
  const M34 inv = inverse(cyl.fwd, &cyl.cond);
  std::memcpy(cyl.r.m, inv.m, sizeof cyl.r.m);
  cyl.r.kind = 3; cyl.r.closed = 1; cyl.r.minimum = 0.0; cyl.r.maximum = 1.0;
  CHECK(other_box(cyl.r, lo, hi), "the closed unit cylinder has a box");
  const long before = tl.odd_behind;
  check_ray(cyl, lo, hi, true, other_needs_line && other_needs_line(cyl.r), V{1.0055, 2, 0}, unit(V{3e-3, 1, 0}), tl,
            "the closed unit cylinder");
  CHECK(tl.odd_behind == before + 1, "the cylinder's ray has one root behind its origin");
}

void check_refusals(Rng& g) {
  double lo[3], hi[3];
  auto fresh = [&](Shape s) {
    Rec rc = make_rec(g, s, 0);
    if (rc.r.kind >= 3) { rc.r.minimum = -1.0; rc.r.maximum = 2.0; }
    return rc.r;
  };
  OtherRec q = fresh(kCone);
  q.closed = 1;
  CHECK(!other_box(q, lo, hi) && line_box(q, lo, hi), "a closed cone: the line hierarchy");
  q.closed = 0;
  CHECK(!other_box(q, lo, hi) && line_box(q, lo, hi), "an open cone: the line hierarchy");
  q = fresh(kOpenCyl);
  CHECK(!other_box(q, lo, hi) && line_box(q, lo, hi), "an open tube: the line hierarchy");
  q = fresh(kClosedCyl);
  CHECK(other_box(q, lo, hi) && !line_box(q, lo, hi), "a closed tube: the other hierarchy");
  q.kind = 1;
  CHECK(!other_box(q, lo, hi) && !line_box(q, lo, hi), "a plane: no box");
  q.kind = 5;
  CHECK(!other_box(q, lo, hi) && !line_box(q, lo, hi), "a triangle's kind: no box");
  for (Shape s : {kClosedCyl, kOpenCyl, kCone}) {
    for (int c = 0; c < 6; ++c) {
      q = fresh(s);
      if (c == 0) q.maximum = INFINITY;
      if (c == 1) q.minimum = -INFINITY;
      if (c == 2) { q.minimum = 1.0; q.maximum = 0.5; }
      if (c == 3) q.minimum = NAN;
      if (c == 4) q.maximum = NAN;
      if (c == 5) { q.minimum = -INFINITY; q.maximum = INFINITY; }
      CHECK(!other_box(q, lo, hi) && !line_box(q, lo, hi), "shape %d with bounds [%g, %g]: no box", (int)s, q.minimum, q.maximum);
    }
  }
  for (Shape s : {kSphere, kCube, kClosedCyl, kOpenCyl, kCone}) {
    for (int c = 0; c < 5; ++c) {
      q = fresh(s);
      const M34 stretch = c == 1 ? scaling(1e8, 1.0, 1.0) : scaling(1, 1, 1);
      const M34 m = c == 0 ? scaling(1.0, 1.01e6, 1.0) : mul(stretch, *(const M34*)q.m);
      std::memcpy(q.m, m.m, sizeof q.m);
      if (c == 2) q.m[g.below(12)] = NAN;
      if (c == 3) q.m[g.below(12)] = g.sign() * INFINITY;
      if (c == 4) for (int e = 0; e < 3; ++e) q.m[4 * 1 + e] = 0.0;  // singular
      CHECK(!other_box(q, lo, hi) && !line_box(q, lo, hi), "shape %d, matrix case %d: no box", (int)s, c);
    }
    // just below the limit: a box
    q = OtherRec{};
    const M34 ok = scaling(1.0, 0.99e6, 1.0);
    std::memcpy(q.m, ok.m, sizeof q.m);
    q.kind = s == kSphere ? 0 : s == kCube ? 2 : s == kCone ? 4 : 3;
    q.closed = s == kClosedCyl;
    q.minimum = -1.0; q.maximum = 1.0;
    CHECK(other_box(q, lo, hi) != line_box(q, lo, hi), "shape %d of condition 0.99e6: a box", (int)s);
  }
}

bool contains(const float* lo, const float* hi, const float* clo, const float* chi) {
  for (int a = 0; a < 3; ++a)
    if (!(lo[a] <= clo[a] && chi[a] <= hi[a])) return false;
  return true;
}
// returns whether a record of the line rule lies below `code`
bool walk_tree(const std::vector<BvhNode>& nodes, const std::vector<OtherRec>& recs, int32_t code, const float* lo,
               const float* hi, std::vector<int>& seen, int depth, int* max_depth) {
  if (code == kBvhEmpty) return false;
  if (code < 0) {
    const int lc = -(code + 1), first = lc >> 7, cnt = lc & 127;
    bool line = false;
    CHECK(cnt >= 1, "an empty leaf");
    for (int k = first; k < first + cnt; ++k) {
      CHECK(k >= 0 && k < (int)recs.size(), "leaf index %d out of range", k);
      if (k < 0 || k >= (int)recs.size()) continue;
      ++seen[(size_t)recs[(size_t)k].meta];
      double blo[3], bhi[3];
      CHECK(other_box(recs[(size_t)k], blo, bhi), "record %d in the hierarchy without a box", k);
      for (int a = 0; a < 3; ++a)
        CHECK((double)lo[a] <= blo[a] && bhi[a] <= (double)hi[a], "record %d outside its leaf's box on axis %d", k, a);
      line = line || (other_needs_line && other_needs_line(recs[(size_t)k]));
    }
    return line;
  }
  *max_depth = std::max(*max_depth, depth + 1);
  const BvhNode& nd = nodes[(size_t)code];
  bool any = false;
  for (int c = 0; c < 2; ++c) {
    if (nd.child[c] == kBvhEmpty) continue;
    if (lo) CHECK(contains(lo, hi, nd.lo[c], nd.hi[c]), "node %d child %d outside its parent's box", code, c);
    const bool line = walk_tree(nodes, recs, nd.child[c], nd.lo[c], nd.hi[c], seen, depth + 1, max_depth);
    if (other_needs_line)
      CHECK(((nd.line >> c) & 1u) == (line ? 1u : 0u), "node %d child %d: line flag %u, records say %d", code, c,
            (nd.line >> c) & 1u, line);
    any = any || line;
  }
  return any;
}

void check_bvh(Rng& g) {
  for (int mix = 0; mix < 3; ++mix)
    for (int leaf : {1, 2, 4}) {
      std::vector<OtherRec> recs;
      for (int k = 0; k < 40; ++k) {
        // mix 0: spheres and cubes only; 1: every kind; 2: 40 records on one spot
        const Shape s = mix == 0 ? (Shape)(k % 2) : (Shape)(k % 3);
        Rec rc = make_rec(g, s, 0);
        if (mix == 2) { const M34 one = translation(0.01 * k, 0, 0); std::memcpy(rc.r.m, inverse(one, nullptr).m, sizeof rc.r.m); }
        double lo[3], hi[3];
        if (!other_box(rc.r, lo, hi)) { --k; continue; }
        rc.r.meta = k;
        recs.push_back(rc.r);
      }
      int depth = -1;
      const std::vector<BvhNode> nodes = build_other_bvh(recs, leaf, &depth, 0.05);
      CHECK(!nodes.empty(), "no hierarchy over 40 boxed records");
      if (nodes.empty()) continue;
      CHECK(depth <= kBvhMaxDepth, "depth %d beyond kBvhMaxDepth", depth);
      CHECK(recs.size() == 40, "%zu records after the build", recs.size());
      std::vector<int> seen(40, 0);
      int max_depth = 0;
      walk_tree(nodes, recs, 0, nullptr, nullptr, seen, 0, &max_depth);
      for (int k = 0; k < 40; ++k) CHECK(seen[(size_t)k] == 1, "record %d appears %d times", k, seen[(size_t)k]);
      CHECK(max_depth == depth, "reported depth %d, walked %d", depth, max_depth);
    }
  std::vector<OtherRec> none;
  CHECK(build_other_bvh(none, 2).empty(), "no records: no hierarchy");
  std::vector<OtherRec> bad(3);
  bad[0].kind = 4;
  CHECK(build_other_bvh(bad, 2).empty(), "a record without a box: no hierarchy");
}

}  // namespace

int main() {
  Rng g{0x07E5B0C5ull};
  Tally known;
  check_known(known);
  check_records(g);
  check_refusals(g);
  check_bvh(g);
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
