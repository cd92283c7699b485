// unit_box_check.cpp — csg_unit_box and build_unit_bvh (rt_bvh.cpp) against a plain restatement.
//
// The contract under test: for every ray (o, d) the walk may cull with (finite, |d|_inf >=
// kUnitDirMin, |o|_inf <= kUnitOriginMax) and every leaf of a unit, each root t the leaf's test
// produces on the CHAINED ray (the world ray through every enclosing Csg's inverse, one matrix
// after another, then the leaf's) has o + t d inside csg_unit_box's box. The chained transform
// and the three leaf tests (sphere.rs:47-62, cube.rs:30-93, cylinder.rs:42-119) are restated
// here in plain doubles with the device's operation order. Build with -ffp-contract=off.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rt_bvh.hpp"

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
};

struct V {
  double x, y, z;
};

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
M34 rotation(int axis, double r) {
  const double c = std::cos(r), s = std::sin(r);
  if (axis == 0) return M34{{1, 0, 0, 0, 0, c, -s, 0, 0, s, c, 0}};
  if (axis == 1) return M34{{c, 0, s, 0, 0, 1, 0, 0, -s, 0, c, 0}};
  return M34{{c, -s, 0, 0, s, c, 0, 0, 0, 0, 1, 0}};
}
// the inverse of translation . rotations . scaling, factor by factor
struct Xf {
  double t[3], rx, ry, rz, s[3];
  M34 inverse() const {
    return mul(scaling(1.0 / s[0], 1.0 / s[1], 1.0 / s[2]),
               mul(rotation(0, -rx), mul(rotation(1, -ry), mul(rotation(2, -rz), translation(-t[0], -t[1], -t[2])))));
  }
  M34 forward() const {
    return mul(translation(t[0], t[1], t[2]),
               mul(rotation(2, rz), mul(rotation(1, ry), mul(rotation(0, rx), scaling(s[0], s[1], s[2])))));
  }
};

constexpr double EPS = 0.00001;  // lib.rs:18

// Ray::transform (ray.rs:26-28) as the device forms it
void xform(const double* m, V& o, V& d) {
  const V lo{m[0] * o.x + m[1] * o.y + m[2] * o.z + m[3], m[4] * o.x + m[5] * o.y + m[6] * o.z + m[7],
             m[8] * o.x + m[9] * o.y + m[10] * o.z + m[11]};
  const V ld{m[0] * d.x + m[1] * d.y + m[2] * d.z, m[4] * d.x + m[5] * d.y + m[6] * d.z,
             m[8] * d.x + m[9] * d.y + m[10] * d.z};
  o = lo;
  d = ld;
}
void check_axis(double origin, double direction, double& tmin, double& tmax) {
  const double a = -1.0 - origin, b = 1.0 - origin;
  if (std::fabs(direction) >= EPS) { tmin = a / direction; tmax = b / direction; }
  else { tmin = a * INFINITY; tmax = b * INFINITY; }
  if (tmin > tmax) { const double x = tmin; tmin = tmax; tmax = x; }
}
bool check_cap(V o, V d, double t) {
  const double x = o.x + t * d.x, z = o.z + t * d.z;
  return (x * x + z * z) <= 1.0;
}
int caps(const OtherRec& q, V o, V d, double* t, int n) {
  if (!q.closed) return n;
  double tc = (q.minimum - o.y) / d.y;
  if (check_cap(o, d, tc)) t[n++] = tc;
  tc = (q.maximum - o.y) / d.y;
  if (check_cap(o, d, tc)) t[n++] = tc;
  return n;
}
// the roots of one leaf on its local ray
int leaf_roots(const OtherRec& q, V o, V d, double t[4]) {
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
  const double a = d.x * d.x + d.z * d.z;
  if (std::fabs(a) < EPS) return caps(q, o, d, t, 0);
  const double b = 2.0 * o.x * d.x + 2.0 * o.z * d.z;
  const double c = o.x * o.x + o.z * o.z - 1.0;
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

struct Unit {
  std::vector<CsgOp> ops;
  std::vector<CsgRec> nodes;
  std::vector<OtherRec> leaves;
  std::vector<M34> leaf_to_world;  // test-side only: where to aim rays
  double max_scale = 1.0;
};

OtherRec make_leaf(Rng& g, int kind, double smax, double* used_scale, M34* fwd = nullptr) {
  OtherRec r{};
  Xf x;
  for (int a = 0; a < 3; ++a) x.t[a] = g.range(-4.0, 4.0);
  x.rx = g.range(-3.0, 3.0); x.ry = g.range(-3.0, 3.0); x.rz = g.range(-3.0, 3.0);
  // anisotropic: every axis its own scale, log-uniform up to smax
  for (int a = 0; a < 3; ++a) x.s[a] = std::pow(smax, g.u());
  *used_scale = std::fmax(x.s[0], std::fmax(x.s[1], x.s[2]));
  const M34 inv = x.inverse();
  if (fwd) *fwd = x.forward();
  std::memcpy(r.m, inv.m, sizeof r.m);
  r.kind = kind;
  r.minimum = -INFINITY;
  r.maximum = INFINITY;
  if (kind == 3) {
    r.minimum = g.range(-2.0, 0.5);
    r.maximum = r.minimum + g.range(0.2, 3.0);
    r.closed = g.below(2);
  }
  return r;
}

// a Csg of `depth` nested nodes: each node has the chain below it on one side and a leaf on the other
void emit(Rng& g, Unit& u, int depth, double smax, const M34& to_world) {
  const int rec = (int)u.nodes.size();
  CsgRec c{};
  Xf x;
  // every Csg its own transform (the transformed-Csg quirk: its gate's box and ray are in different
  // spaces; the gate is a filter inside the program and takes no part in the box)
  for (int a = 0; a < 3; ++a) { x.t[a] = g.range(-2.0, 2.0); x.s[a] = g.range(0.7, 1.4); }
  x.rx = g.range(-3.0, 3.0); x.ry = g.range(-3.0, 3.0); x.rz = g.range(-3.0, 3.0);
  const M34 inv = x.inverse();
  const M34 here = mul(to_world, x.forward());
  std::memcpy(c.m, inv.m, sizeof c.m);
  for (int a = 0; a < 3; ++a) { c.lo[a] = -1.0; c.hi[a] = 1.0; }
  c.op = g.below(3);
  u.nodes.push_back(c);
  const size_t at = u.ops.size();
  u.ops.push_back(CsgOp{kCsgEnter, rec, 0, 0});
  const bool nested_left = g.below(2) != 0;
  for (int side = 0; side < 2; ++side) {
    if (depth > 1 && (side == 0) == nested_left) {
      emit(g, u, depth - 1, smax, here);
    } else {
      const int kinds[3] = {0, 2, 3};
      double sc;
      M34 fwd;
      const OtherRec leaf = make_leaf(g, kinds[g.below(3)], smax, &sc, &fwd);
      u.leaf_to_world.push_back(mul(here, fwd));
      u.max_scale = std::fmax(u.max_scale, sc);
      u.ops.push_back(CsgOp{kCsgLeaf, (int32_t)u.leaves.size(), 0, 0});
      u.leaves.push_back(leaf);
    }
  }
  u.ops.push_back(CsgOp{kCsgExit, rec, 0, 0});
  u.ops[at].skip_to = (int32_t)u.ops.size();
}

int failures = 0;
#define CHECK(c, ...)                                  \
  do {                                                 \
    if (!(c)) {                                        \
      if (++failures <= 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                  \
  } while (0)

// every leaf's roots on the chained ray lie in the box; returns the roots checked
long check_ray(const Unit& u, const double* lo, const double* hi, V o, V d) {
  long roots = 0;
  V so[kCsgMaxDepth + 1], sd[kCsgMaxDepth + 1];
  int lvl = 0;
  V co = o, cd = d;
  for (const CsgOp& op : u.ops) {
    if (op.code == kCsgEnter) {
      so[lvl] = co; sd[lvl] = cd; ++lvl;
      xform(u.nodes[(size_t)op.arg].m, co, cd);
    } else if (op.code == kCsgExit) {
      --lvl;
      co = so[lvl]; cd = sd[lvl];
    } else if (op.code == kCsgLeaf) {
      const OtherRec& q = u.leaves[(size_t)op.arg];
      V lo3 = co, ld3 = cd;
      xform(q.m, lo3, ld3);
      double t[4];
      const int n = leaf_roots(q, lo3, ld3, t);
      for (int i = 0; i < n; ++i) {
        if (!std::isfinite(t[i])) continue;
        ++roots;
        const double p[3] = {o.x + t[i] * d.x, o.y + t[i] * d.y, o.z + t[i] * d.z};
        for (int a = 0; a < 3; ++a)
          CHECK(p[a] >= lo[a] && p[a] <= hi[a], "kind %d root %.17g: p[%d] = %.17g outside [%.17g, %.17g]", q.kind, t[i], a,
                p[a], lo[a], hi[a]);
      }
    }
  }
  return roots;
}

V unit(V v) {
  const double m = std::sqrt(v.x * v.x + v.y * v.y + v.z * v.z);
  return V{v.x / m, v.y / m, v.z / m};
}

void check_units(Rng& g) {
  int boxed = 0, boxed_big = 0, deep = 0, parallel = 0;
  long roots = 0;
  const int n_units = 60, n_rays = 3000;
  for (int k = 0; k < n_units; ++k) {
    Unit u;
    const int depth = 1 + k % 4;
    // a third of the units with leaf scalings up to 1e3, the rest up to 30
    emit(g, u, depth, k % 3 == 0 ? 1e3 : 30.0, scaling(1, 1, 1));
    double lo[3], hi[3];
    if (!csg_unit_box(u.ops.data(), 0, (int)u.ops.size(), u.nodes.data(), u.leaves.data(), lo, hi)) continue;
    ++boxed;
    if (u.max_scale >= 300.0) ++boxed_big;
    if (depth == 4) ++deep;
    const double c[3] = {0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1]), 0.5 * (lo[2] + hi[2])};
    const double h[3] = {0.5 * (hi[0] - lo[0]), 0.5 * (hi[1] - lo[1]), 0.5 * (hi[2] - lo[2])};
    const double size = std::fmax(h[0], std::fmax(h[1], h[2]));
    for (int r = 0; r < n_rays; ++r) {
      V o, d;
      const int mode = r % 5;
      auto in_box = [&](double f) {
        return V{c[0] + f * h[0] * g.range(-1, 1), c[1] + f * h[1] * g.range(-1, 1), c[2] + f * h[2] * g.range(-1, 1)};
      };
      if (mode == 0) {  // from inside the box, any direction
        o = in_box(1.0);
        d = unit(V{g.range(-1, 1), g.range(-1, 1), g.range(-1, 1)});
      } else {
        // from outside, near or far (up to the origin bound), towards a point of the box:
        // anywhere in it, on its surface (grazing faces, edges and corners), or just off it
        const double far = mode == 4 ? 0.9 * kUnitOriginMax : size * g.range(1.5, 20.0);
        const V dir = unit(V{g.range(-1, 1), g.range(-1, 1), g.range(-1, 1)});
        o = V{c[0] + far * dir.x, c[1] + far * dir.y, c[2] + far * dir.z};
        const double lim = kUnitOriginMax;
        o.x = std::fmax(-lim, std::fmin(lim, o.x)); o.y = std::fmax(-lim, std::fmin(lim, o.y));
        o.z = std::fmax(-lim, std::fmin(lim, o.z));
        V aim = in_box(1.0);
        if (mode == 1 || mode == 4) {  // at a leaf: a point of its region, or just off its silhouette
          const size_t li = (size_t)g.below((int)u.leaves.size());
          const OtherRec& q = u.leaves[li];
          const double w = r % 3 == 0 ? 1.0 : 0.7;
          V lp{g.range(-w, w), g.range(-w, w), g.range(-w, w)};
          if (q.kind == 3) lp.y = g.range(q.minimum, q.maximum);
          if (r % 3 == 0) lp = q.kind == 0 ? unit(lp) : V{lp.x, lp.y, g.below(2) ? 1.0 : -1.0};  // on the surface: tangent rays
          V zero{0, 0, 0};
          xform(u.leaf_to_world[li].m, lp, zero);
          aim = lp;
        }
        if (mode == 2 || mode == 3) {  // onto the surface: one to three coordinates on a face
          double* a3 = &aim.x;
          const int nfix = 1 + g.below(3);
          for (int f = 0; f < nfix; ++f) {
            const int ax = g.below(3);
            const double off = mode == 3 ? g.range(-1e-6, 1e-6) * size : 0.0;
            a3[ax] = (g.below(2) ? hi[ax] : lo[ax]) + off;
          }
        }
        d = unit(V{aim.x - o.x, aim.y - o.y, aim.z - o.z});
        if (r % 7 == 0) {  // axis-parallel rays: exact zeros in the direction
          const int ax = g.below(3);
          d = V{ax == 0 ? 1.0 : 0.0, ax == 1 ? 1.0 : 0.0, ax == 2 ? 1.0 : 0.0};
          o = V{ax == 0 ? o.x : aim.x, ax == 1 ? o.y : aim.y, ax == 2 ? o.z : aim.z};
        }
      }
      roots += check_ray(u, lo, hi, o, d);
    }
    // Cube::check_axis's parallel rule (cube.rs:30-47): a ray whose local direction has 0 < |d| <
    // EPSILON on an axis, starting inside that slab just under the face and a long way off along
    // another axis, reaches the cube's other faces up to |t| EPSILON outside the slab
    for (size_t li = 0; li < u.leaves.size(); ++li) {
      if (u.leaves[li].kind != 2) continue;
      const double* f = u.leaf_to_world[li].m;
      for (int r = 0; r < 60; ++r) {
        const int ax = g.below(3), par = (ax + 1 + g.below(2)) % 3;  // travel along ax, nearly parallel to slab `par`
        const double n = std::sqrt(f[ax] * f[ax] + f[4 + ax] * f[4 + ax] + f[8 + ax] * f[8 + ax]);  // world length of a local step
        const double world_dist = g.range(10.0, 0.4 * kUnitOriginMax);
        double ld[3] = {0, 0, 0}, lo3[3] = {g.range(-0.9, 0.9), g.range(-0.9, 0.9), g.range(-0.9, 0.9)};
        const double sgn = g.below(2) ? 1.0 : -1.0;
        ld[ax] = 1.0;
        ld[par] = sgn * g.range(0.3, 0.95) * EPS * n;
        lo3[ax] = -(1.0 + world_dist / n);
        lo3[par] = sgn * (1.0 - g.range(1e-9, 1e-3));
        V o{lo3[0], lo3[1], lo3[2]}, zero{0, 0, 0}, d{0, 0, 0};
        xform(f, o, zero);
        d = unit(V{f[0] * ld[0] + f[1] * ld[1] + f[2] * ld[2], f[4] * ld[0] + f[5] * ld[1] + f[6] * ld[2],
                   f[8] * ld[0] + f[9] * ld[1] + f[10] * ld[2]});
        if (std::fmax(std::fabs(o.x), std::fmax(std::fabs(o.y), std::fabs(o.z))) > kUnitOriginMax) continue;
        ++parallel;
        roots += check_ray(u, lo, hi, o, d);
      }
    }
  }
  CHECK(boxed >= n_units / 2, "only %d of %d units boxed", boxed, n_units);
  CHECK(boxed_big >= 3, "only %d boxed units with a leaf scaling >= 300", boxed_big);
  CHECK(deep >= 3, "only %d boxed units nested four deep", deep);
  CHECK(roots > 100000, "only %ld roots checked", roots);
  CHECK(parallel > 1000, "only %d nearly parallel cube rays", parallel);
  std::printf("units boxed %d (scaled >= 300: %d, four deep: %d), roots %ld\n", boxed, boxed_big, deep, roots);
}

// one-leaf-pair units that must have no box
void check_false_cases(Rng& g) {
  auto unit_with = [&](const OtherRec& bad, const double* csg_m) {
    Unit u;
    CsgRec c{};
    const M34 id = scaling(1, 1, 1);
    std::memcpy(c.m, csg_m ? csg_m : id.m, sizeof c.m);
    u.nodes.push_back(c);
    double sc;
    u.leaves.push_back(make_leaf(g, 0, 2.0, &sc));
    u.leaves.push_back(bad);
    u.ops = {CsgOp{kCsgEnter, 0, 4, 0}, CsgOp{kCsgLeaf, 0, 0, 0}, CsgOp{kCsgLeaf, 1, 0, 0}, CsgOp{kCsgExit, 0, 0, 0}};
    double lo[3], hi[3];
    return csg_unit_box(u.ops.data(), 0, 4, u.nodes.data(), u.leaves.data(), lo, hi);
  };
  double sc;
  OtherRec ok = make_leaf(g, 2, 2.0, &sc);
  CHECK(unit_with(ok, nullptr), "a sphere and a cube: a box");
  OtherRec plane = make_leaf(g, 1, 2.0, &sc);
  CHECK(!unit_with(plane, nullptr), "a plane leaf: no box");
  OtherRec cone = make_leaf(g, 4, 2.0, &sc);
  cone.minimum = -1.0; cone.maximum = 0.0; cone.closed = 1;
  CHECK(!unit_with(cone, nullptr), "a cone leaf: no box");
  OtherRec cyl = make_leaf(g, 3, 2.0, &sc);
  cyl.maximum = INFINITY;
  CHECK(!unit_with(cyl, nullptr), "a cylinder without an upper bound: no box");
  cyl.maximum = 1.0; cyl.minimum = -INFINITY;
  CHECK(!unit_with(cyl, nullptr), "a cylinder without a lower bound: no box");
  const M34 ill = scaling(1.0, 1e-8, 1.0);  // condition 1e8
  CHECK(!unit_with(ok, ill.m), "a chain matrix of condition 1e8: no box");
  OtherRec flat = ok;
  const M34 fm = mul(scaling(1e8, 1.0, 1.0), M34{{ok.m[0], ok.m[1], ok.m[2], ok.m[3], ok.m[4], ok.m[5], ok.m[6], ok.m[7],
                                                   ok.m[8], ok.m[9], ok.m[10], ok.m[11]}});
  std::memcpy(flat.m, fm.m, sizeof flat.m);
  CHECK(!unit_with(flat, nullptr), "a leaf matrix of condition 1e8: no box");
  // each matrix below 1e6, their product above it
  const M34 c1 = scaling(1.0, 1e-4, 1.0);
  OtherRec l1 = ok;
  const M34 lm = mul(scaling(1.0, 1.0, 1e4), M34{{ok.m[0], ok.m[1], ok.m[2], ok.m[3], ok.m[4], ok.m[5], ok.m[6], ok.m[7],
                                                   ok.m[8], ok.m[9], ok.m[10], ok.m[11]}});
  std::memcpy(l1.m, lm.m, sizeof l1.m);
  CHECK(!unit_with(l1, c1.m), "a chain whose condition bound is 1e8: no box");
  OtherRec nan = ok;
  nan.m[3] = NAN;
  CHECK(!unit_with(nan, nullptr), "a non-finite result: no box");
}

bool contains(const float* lo, const float* hi, const float* clo, const float* chi) {
  for (int a = 0; a < 3; ++a)
    if (!(lo[a] <= clo[a] && chi[a] <= hi[a])) return false;
  return true;
}
// every node's child box holds the boxes below it; every unit once in a leaf; returns the units seen
void walk_tree(const std::vector<BvhNode>& nodes, const std::vector<double>& boxes, const std::vector<int>& order,
               int32_t code, const float* lo, const float* hi, std::vector<int>& seen, int depth, int* max_depth) {
  if (code == kBvhEmpty) return;
  if (code < 0) {
    const int lc = -(code + 1), first = lc >> 7, cnt = lc & 127;
    for (int k = first; k < first + cnt; ++k) {
      CHECK(k >= 0 && k < (int)order.size(), "leaf index %d out of range", k);
      if (k < 0 || k >= (int)order.size()) continue;
      const int un = order[(size_t)k];
      ++seen[(size_t)un];
      if (lo)
        for (int a = 0; a < 3; ++a)
          CHECK((double)lo[a] <= boxes[6 * (size_t)un + a] && boxes[6 * (size_t)un + 3 + a] <= (double)hi[a],
                "unit %d outside its leaf's box on axis %d", un, a);
    }
    return;
  }
  *max_depth = std::max(*max_depth, depth + 1);
  const BvhNode& nd = nodes[(size_t)code];
  for (int c = 0; c < 2; ++c) {
    if (nd.child[c] == kBvhEmpty) continue;
    if (lo) CHECK(contains(lo, hi, nd.lo[c], nd.hi[c]), "node %d child %d outside its parent's box", code, c);
    walk_tree(nodes, boxes, order, nd.child[c], nd.lo[c], nd.hi[c], seen, depth + 1, max_depth);
  }
}

void check_bvh(Rng& g) {
  for (int collinear = 0; collinear < 2; ++collinear)
    for (int leaf : {1, 2, 4}) {
      std::vector<double> boxes;
      for (int k = 0; k < 40; ++k) {
        double c[3], h[3];
        for (int a = 0; a < 3; ++a) { c[a] = g.range(-20.0, 20.0); h[a] = g.range(0.2, 3.0); }
        if (collinear) { c[0] = 0.01 * k; c[1] = c[2] = 0.0; h[0] = h[1] = h[2] = 5.0; }  // 40 overlapping boxes on one line
        for (int a = 0; a < 3; ++a) boxes.push_back(c[a] - h[a]);
        for (int a = 0; a < 3; ++a) boxes.push_back(c[a] + h[a]);
      }
      int depth = -1;
      std::vector<int> order;
      const std::vector<BvhNode> nodes = build_unit_bvh(boxes, leaf, &depth, &order, 0.05);
      if (nodes.empty()) {  // allowed only as "too deep": never for 40 boxes the builder can split
        CHECK(collinear, "no hierarchy over 40 scattered boxes");
        continue;
      }
      CHECK(depth <= kBvhMaxDepth, "depth %d beyond kBvhMaxDepth", depth);
      CHECK(order.size() == 40, "order holds %zu units", order.size());
      std::vector<int> seen(40, 0);
      int max_depth = 0;
      walk_tree(nodes, boxes, order, 0, nullptr, nullptr, seen, 0, &max_depth);
      for (int k = 0; k < 40; ++k) CHECK(seen[(size_t)k] == 1, "unit %d appears %d times", k, seen[(size_t)k]);
      CHECK(max_depth == depth, "reported depth %d, walked %d", depth, max_depth);
      std::vector<int> in_order(40, 0);
      for (int i : order) CHECK(i >= 0 && i < 40 && ++in_order[(size_t)i] == 1, "order repeats unit %d", i);
    }
  std::vector<int> order;
  int depth = -1;
  CHECK(build_unit_bvh({}, 2, &depth, &order).empty() && order.empty(), "no boxes: no hierarchy");
}

}  // namespace

int main() {
  Rng g{0x5EEDB0C5ull};
  check_units(g);
  check_false_cases(g);
  check_bvh(g);
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
