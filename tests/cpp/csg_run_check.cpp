// csg_run_check.cpp — the run hierarchies inside wide and deep Csg units: tri_box with a run's
// bounds, csg_run_bounds and build_csg_run (rt_bvh.cpp), and the walk the evaluators make
// (rt_slab.hpp csg_run_admits / csg_run_walk, rt_csg.hpp csg_batch_insert: the functions the device
// compiles), against the one-by-one loop over the run's triangles.
//
// The contract, per run and per chained ray (co, cd) the run admits, for every interval
// [t_lo, t_hi] the evaluators can ask for (t_hi: +inf, any positive value, a root of the run;
// the watermark: none, or one of the run's own roots):
//   - every triangle whose root on the chained ray (triangle.rs:63-90, restated below in the
//     device's operation order) lies above the watermark and at or below t_hi is reached;
//   - the walk's batch equals the one-by-one loop's up to t_hi, and `more` agrees wherever a
//     root at or below t_hi was left out;
//   - a ray whose line clearly misses the root's box reaches no boxed triangle.
// And of the build: the boxed records are exactly those tri_box accepts with the run's bounds,
// each in exactly one leaf, inside its leaf's box; every child box inside its parent's; the depth
// bound; the remainder after them; the records a permutation of the input.
// Build with -ffp-contract=off.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rt_bvh.hpp"
#include "rt_slab.hpp"

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
  double logu(double a, double b) { return std::exp(range(std::log(a), std::log(b))); }
  int below(int n) { return (int)(next() % (uint64_t)n); }
};

struct V {
  double x, y, z;
};
V operator+(V a, V b) { return V{a.x + b.x, a.y + b.y, a.z + b.z}; }
V operator-(V a, V b) { return V{a.x - b.x, a.y - b.y, a.z - b.z}; }
V operator*(double s, V a) { return V{s * a.x, s * a.y, s * a.z}; }
double dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
V cross(V a, V b) { return V{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
double norm(V a) { return std::sqrt(dot(a, a)); }
double ninf(V a) { return std::fmax(std::fabs(a.x), std::fmax(std::fabs(a.y), std::fabs(a.z))); }
V unit(V a) { return (1.0 / norm(a)) * a; }

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
M34 shearing(double xy, double zx) { return M34{{1, xy, 0, 0, 0, 1, 0, 0, zx, 0, 1, 0}}; }
M34 rotation(int axis, double r) {
  const double c = std::cos(r), s = std::sin(r);
  if (axis == 0) return M34{{1, 0, 0, 0, 0, c, -s, 0, 0, s, c, 0}};
  if (axis == 1) return M34{{c, 0, s, 0, 0, 1, 0, 0, -s, 0, c, 0}};
  return M34{{c, -s, 0, 0, s, c, 0, 0, 0, 0, 1, 0}};
}
// a Csg's inverse: scaling^-1 . shear^-1 . rotations^-1 . translation^-1, factor by factor
M34 csg_inverse(Rng& g, double smin, double smax, double tmax) {
  const M34 s = scaling(1.0 / g.logu(smin, smax), 1.0 / g.logu(smin, smax), 1.0 / g.logu(smin, smax));
  const double xy = g.below(3) == 0 ? g.range(-0.5, 0.5) : 0.0, zx = g.below(3) == 0 ? g.range(-0.5, 0.5) : 0.0;
  const M34 r = mul(rotation(0, g.range(-3, 3)), mul(rotation(1, g.range(-3, 3)), rotation(2, g.range(-3, 3))));
  return mul(s, mul(shearing(-xy, -zx), mul(r, translation(g.range(-tmax, tmax), g.range(-tmax, tmax), g.range(-tmax, tmax)))));
}

// Ray::transform (ray.rs:26-28) as the device forms it
void xform(const double* m, V& o, V& d) {
  const V lo{m[0] * o.x + m[1] * o.y + m[2] * o.z + m[3], m[4] * o.x + m[5] * o.y + m[6] * o.z + m[7],
             m[8] * o.x + m[9] * o.y + m[10] * o.z + m[11]};
  const V ld{m[0] * d.x + m[1] * d.y + m[2] * d.z, m[4] * d.x + m[5] * d.y + m[6] * d.z,
             m[8] * d.x + m[9] * d.y + m[10] * d.z};
  o = lo;
  d = ld;
}
// Triangle::local_intersect (triangle.rs:63-90), the device's tri_local_intersect
long sliver_roots = 0;  // roots found at |det| below 5 EPSILON
bool tri_local(V p1, V e1, V e2, V o, V d, double& t) {
  const V dir_cross_e2 = cross(d, e2);
  const double det = dot(e1, dir_cross_e2);
  if (std::fabs(det) < kEpsilon) return false;
  const double f = 1.0 / det;
  const V p1_to_origin = o - p1;
  const double u = f * dot(p1_to_origin, dir_cross_e2);
  if (!(0.0 <= u && u <= 1.0)) return false;
  const V origin_cross_e1 = cross(p1_to_origin, e1);
  const double v = f * dot(d, origin_cross_e1);
  if (v < 0.0 || (u + v) > 1.0) return false;
  t = f * dot(e2, origin_cross_e1);
  if (std::fabs(det) < 5.0 * kEpsilon) ++sliver_roots;
  return true;
}
// csg_tri_roots: the record's inverse, then the triangle
bool tri_roots(const TriRec& q, V o, V d, double& t) {
  xform(q.m, o, d);
  return tri_local(V{q.p1[0], q.p1[1], q.p1[2]}, V{q.e1[0], q.e1[1], q.e1[2]}, V{q.e2[0], q.e2[1], q.e2[2]}, o, d, t);
}

int failures = 0;
#define CHECK(c, ...)                                  \
  do {                                                 \
    if (!(c)) {                                        \
      if (++failures <= 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                  \
  } while (0)

struct Run {
  std::vector<TriRec> recs;
  std::vector<BvhNode> nodes;
  CsgRun run{};
  M34 rec_fwd;  // the records' shared forward matrix (object -> the chained ray's space)
};

bool contains(const float* lo, const float* hi, const float* clo, const float* chi) {
  for (int a = 0; a < 3; ++a)
    if (!(lo[a] <= clo[a] && chi[a] <= hi[a])) return false;
  return true;
}
void walk_tree(const Run& r, int32_t code, const float* lo, const float* hi, std::vector<int>& seen, int depth, int* max_depth) {
  if (code == kBvhEmpty) return;
  if (code < 0) {
    const int lc = -(code + 1), first = lc >> 7, cnt = lc & 127;
    for (int k = first; k < first + cnt; ++k) {
      CHECK(k >= 0 && k < r.run.n_boxed, "leaf index %d outside the boxed records [0, %d)", k, r.run.n_boxed);
      if (k < 0 || k >= r.run.n_boxed) continue;
      ++seen[(size_t)k];
      double blo[3], bhi[3];
      const bool ok = tri_box(r.recs[(size_t)k], r.run.dmax, r.run.omax, blo, bhi);
      CHECK(ok, "boxed record %d has no box", k);
      for (int a = 0; ok && a < 3; ++a)
        CHECK((double)lo[a] <= blo[a] && bhi[a] <= (double)hi[a], "record %d outside its leaf's box on axis %d", k, a);
    }
    return;
  }
  CHECK(code < (int32_t)r.nodes.size(), "node index %d of %zu", code, r.nodes.size());
  if (code >= (int32_t)r.nodes.size()) return;
  *max_depth = std::max(*max_depth, depth + 1);
  const BvhNode& nd = r.nodes[(size_t)code];
  for (int c = 0; c < 2; ++c) {
    if (nd.child[c] == kBvhEmpty) continue;
    if (lo) CHECK(contains(lo, hi, nd.lo[c], nd.hi[c]), "node %d child %d outside its parent's box", code, c);
    walk_tree(r, nd.child[c], nd.lo[c], nd.hi[c], seen, depth + 1, max_depth);
  }
}

// One run of n triangles in the chained ray's space: edges around L in a region that holds a few
// per unit of length, some flat and axis-aligned, `bad` of them under an ill-conditioned inverse.
Run make_run(Rng& g, int n, double L, int bad, bool flat_grid, bool plain_rec) {
  Run r;
  const double region = L * std::cbrt((double)n) * 1.5;
  const double rs = plain_rec ? 1.0 : g.range(0.5, 2.0);
  const double rr[3] = {g.range(-3, 3), g.range(-3, 3), g.range(-3, 3)}, rt[3] = {g.range(-2, 2) * L, g.range(-2, 2) * L, g.range(-2, 2) * L};
  M34 fwd = scaling(1, 1, 1), inv = scaling(1, 1, 1);
  if (!plain_rec) {
    fwd = mul(translation(rt[0], rt[1], rt[2]), mul(rotation(2, rr[2]), mul(rotation(1, rr[1]), mul(rotation(0, rr[0]), scaling(rs, rs * 1.5, rs)))));
    inv = mul(scaling(1 / rs, 1 / (rs * 1.5), 1 / rs), mul(rotation(0, -rr[0]), mul(rotation(1, -rr[1]), mul(rotation(2, -rr[2]), translation(-rt[0], -rt[1], -rt[2])))));
  }
  r.rec_fwd = fwd;
  for (int i = 0; i < n; ++i) {
    TriRec q{};
    std::memcpy(q.m, inv.m, sizeof q.m);
    V p{g.range(-region, region), g.range(-region, region), g.range(-region, region)};
    const double l = L * g.logu(0.3, 3.0);
    V e1 = l * unit(V{g.range(-1, 1), g.range(-1, 1), g.range(-1, 1)}), e2 = l * unit(V{g.range(-1, 1), g.range(-1, 1), g.range(-1, 1)});
    if (flat_grid || i % 5 == 0) {  // axis-aligned, zero thickness: the whole triangle in one coordinate plane
      const int ax = flat_grid ? 1 : i % 3;
      double* c[3] = {&p.x, &p.y, &p.z};
      double* a1[3] = {&e1.x, &e1.y, &e1.z};
      double* a2[3] = {&e2.x, &e2.y, &e2.z};
      *a1[ax] = 0.0;
      *a2[ax] = 0.0;
      if (flat_grid) {
        *c[ax] = 0.25 * L;
        *a1[(ax + 1) % 3] = 0.0;  // a right triangle along the other two axes
        *a2[(ax + 2) % 3] = 0.0;
      }
    }
    if (i < bad) {  // an inverse of condition 1e7: tri_box refuses it
      const M34 ill = mul(scaling(1.0, 1e-7, 1.0), inv);
      std::memcpy(q.m, ill.m, sizeof q.m);
    }
    q.p1[0] = p.x; q.p1[1] = p.y; q.p1[2] = p.z;
    q.e1[0] = e1.x; q.e1[1] = e1.y; q.e1[2] = e1.z;
    q.e2[0] = e2.x; q.e2[1] = e2.y; q.e2[2] = e2.z;
    q.meta = (int32_t)((1000 + i) << 1 | 1);
    q.tri = i;
    r.recs.push_back(q);
  }
  return r;
}

struct Root {
  double t;
  int32_t key;
  int k;
};
bool root_less(const Root& a, const Root& b) { return a.t < b.t || (a.t == b.t && a.key < b.key); }

// the vertices of record k in the chained ray's space
void tri_points(const Run& r, int k, V out[3]) {
  const TriRec& q = r.recs[(size_t)k];
  const V p{q.p1[0], q.p1[1], q.p1[2]}, e1{q.e1[0], q.e1[1], q.e1[2]}, e2{q.e2[0], q.e2[1], q.e2[2]};
  V pts[3] = {p, p + e1, p + e2};
  for (int i = 0; i < 3; ++i) {
    V zero{0, 0, 0};
    xform(r.rec_fwd.m, pts[i], zero);
    out[i] = pts[i];
  }
}

struct Tally {
  long rays = 0, admitted = 0, roots = 0, visits = 0, second_walks = 0, full = 0, near_bound = 0, slivers = 0, misses = 0;
};

void check_ray(Rng& g, const Run& r, V co, V cd, Tally& tl) {
  ++tl.rays;
  if (!csg_run_admits(r.run, co, cd)) return;
  ++tl.admitted;
  const int n = r.run.n;
  std::vector<Root> roots;
  for (int k = 0; k < n; ++k) {
    double t;
    if (tri_roots(r.recs[(size_t)k], co, cd, t) && t == t) roots.push_back(Root{t, (r.recs[(size_t)k].meta >> 1) << kKeyShift, k});
  }
  tl.roots += (long)roots.size();
  std::sort(roots.begin(), roots.end(), root_less);
  // the intervals: t_hi = +inf, a random positive value, a root's own t; the watermark: none, or a root
  for (int trial = 0; trial < 3; ++trial) {
    double t_hi = INFINITY, wt = -INFINITY;
    int32_t wk = -1;
    if (trial == 1 && !roots.empty()) {
      const Root& h = roots[(size_t)g.below((int)roots.size())];
      t_hi = h.t >= 0.0 ? h.t : g.logu(1e-3, 1e3);
    } else if (trial == 2) {
      t_hi = g.below(2) ? INFINITY : g.logu(1e-3, 1e3);
      if (!roots.empty()) {
        const Root& w = roots[(size_t)g.below((int)roots.size())];
        wt = w.t;
        wk = w.key;
        ++tl.second_walks;
      }
    } else if (trial == 1) {
      t_hi = g.logu(1e-3, 1e3);
    }
    std::vector<char> seen((size_t)n, 0);
    CsgBatch one{}, hier{};
    bool more_one = false, more_hier = false;
    const uint16_t tag = (uint16_t)(3 | kCsgTagTri);
    for (int k = 0; k < n; ++k) {
      double t;
      if (tri_roots(r.recs[(size_t)k], co, cd, t))
        csg_batch_insert(one, kCsgListCap, t, (r.recs[(size_t)k].meta >> 1) << kKeyShift, tag, wt, wk, more_one);
    }
    long visits = 0;
    csg_run_walk(r.run, r.nodes.data(), co, cd, f32_below(wt), f32_up(t_hi), [&](int k) {
      ++visits;
      CHECK(k >= 0 && k < n && !seen[(size_t)k], "record %d visited twice or out of range", k);
      if (k < 0 || k >= n) return;
      seen[(size_t)k] = 1;
      double t;
      if (tri_roots(r.recs[(size_t)k], co, cd, t))
        csg_batch_insert(hier, kCsgListCap, t, (r.recs[(size_t)k].meta >> 1) << kKeyShift, tag, wt, wk, more_hier);
    });
    tl.visits += visits;
    std::vector<Root> in;  // the roots the evaluator still needs: above the watermark, at or below t_hi
    for (const Root& x : roots)
      if (csg_above(x.t, x.key, wt, wk) && x.t <= t_hi) {
        in.push_back(x);
        CHECK(seen[(size_t)x.k], "record %d with root %.17g in (%.17g, %.17g] not reached (dmax %.3g omax %.3g |cd| %.3g |co| %.3g)",
              x.k, x.t, wt, t_hi, r.run.dmax, r.run.omax, ninf(cd), ninf(co));
      }
    for (int k = r.run.n_boxed; k < n; ++k) CHECK(seen[(size_t)k], "remainder record %d not tested", k);
    const size_t want = std::min(in.size(), (size_t)kCsgListCap);
    int n_one = 0, n_hier = 0;
    while (n_one < one.xs.n && one.xs.t[n_one] <= t_hi) ++n_one;
    while (n_hier < hier.xs.n && hier.xs.t[n_hier] <= t_hi) ++n_hier;
    CHECK((size_t)n_one == want && (size_t)n_hier == want, "batch up to t_hi: one by one %d, walk %d, roots %zu", n_one, n_hier, want);
    for (size_t i = 0; i < want && i < (size_t)n_hier && i < (size_t)n_one; ++i)
      CHECK(hier.xs.t[i] == in[i].t && hier.xs.key[i] == in[i].key && hier.tag[i] == tag && one.xs.t[i] == in[i].t &&
                one.xs.key[i] == in[i].key,
            "batch entry %zu differs", i);
    if (in.size() > (size_t)kCsgListCap) {
      ++tl.full;
      CHECK(more_one && more_hier, "a root at or below t_hi left out: more %d / %d", (int)more_one, (int)more_hier);
    }
    if (!more_one) CHECK(!more_hier, "the walk left a root out that the loop did not");
  }
}

// the line of (co, cd) against the root's box in binary64, widened by `slack`: clearly a miss?
bool clear_miss(const Run& r, V co, V cd) {
  const BvhNode& rt = r.nodes[0];
  double lo[3], hi[3];
  for (int a = 0; a < 3; ++a) {
    lo[a] = rt.lo[0][a];
    hi[a] = rt.hi[0][a];
    if (rt.child[1] != kBvhEmpty) { lo[a] = std::fmin(lo[a], (double)rt.lo[1][a]); hi[a] = std::fmax(hi[a], (double)rt.hi[1][a]); }
  }
  const double o[3] = {co.x, co.y, co.z}, d[3] = {cd.x, cd.y, cd.z};
  double tmin = -INFINITY, tmax = INFINITY;
  for (int a = 0; a < 3; ++a) {
    const double w = 1e-3 * (hi[a] - lo[a]) + 1e-3 * (std::fabs(lo[a]) + std::fabs(hi[a]) + std::fabs(o[a]));
    if (std::fabs(d[a]) < 1e-30) {
      if (o[a] < lo[a] - w || o[a] > hi[a] + w) return true;
      continue;
    }
    double t0 = (lo[a] - w - o[a]) / d[a], t1 = (hi[a] + w - o[a]) / d[a];
    if (t0 > t1) std::swap(t0, t1);
    tmin = std::fmax(tmin, t0);
    tmax = std::fmin(tmax, t1);
  }
  return tmin > tmax;
}

void check_run(Rng& g, Run& r, const std::vector<M34>& chain, int n_rays, Tally& tl, bool expect, int bad) {
  const int n = (int)r.recs.size();
  std::vector<const double*> ms;
  for (const M34& m : chain) ms.push_back(m.m);
  csg_run_bounds(ms.data(), (int)ms.size(), &r.run.dmax, &r.run.omax);
  CHECK(r.run.dmax > 0.0 && r.run.omax > 0.0 && std::isfinite(r.run.dmax) && std::isfinite(r.run.omax), "bounds %g %g", r.run.dmax, r.run.omax);
  // the bounds hold for every world ray within kTriDirMax / kTriOriginMax, the corners included
  for (int k = 0; k < 200; ++k) {
    V o{g.range(-1, 1) * kTriOriginMax, g.range(-1, 1) * kTriOriginMax, g.range(-1, 1) * kTriOriginMax};
    V d{g.range(-1, 1) * kTriDirMax, g.range(-1, 1) * kTriDirMax, g.range(-1, 1) * kTriDirMax};
    if (k % 4 == 0) {
      o = V{g.below(2) ? kTriOriginMax : -kTriOriginMax, g.below(2) ? kTriOriginMax : -kTriOriginMax, g.below(2) ? kTriOriginMax : -kTriOriginMax};
      d = V{g.below(2) ? kTriDirMax : -kTriDirMax, g.below(2) ? kTriDirMax : -kTriDirMax, g.below(2) ? kTriDirMax : -kTriDirMax};
    }
    for (const M34& m : chain) xform(m.m, o, d);
    CHECK(csg_run_admits(r.run, o, d), "a chained world ray beyond the run's bounds: |cd| %.17g > %.17g or |co| %.17g > %.17g", ninf(d),
          r.run.dmax, ninf(o), r.run.omax);
  }
  const std::vector<TriRec> before = r.recs;
  int n_boxed = -1, depth = -1;
  r.nodes = build_csg_run(r.recs.data(), n, r.run.dmax, r.run.omax, 16, 2, 0.7, &n_boxed, &depth);
  int can = 0;
  double blo[3], bhi[3];
  for (const TriRec& q : before) can += tri_box(q, r.run.dmax, r.run.omax, blo, bhi) ? 1 : 0;
  // a hierarchy exactly where tri_box accepts 16 records (no tree here comes near kBvhMaxDepth)
  CHECK(r.nodes.empty() == (can < 16), "%s over %d boxed records of %d", r.nodes.empty() ? "no hierarchy" : "a hierarchy", can, n);
  if (expect) CHECK(!r.nodes.empty(), "no hierarchy where one is expected (%d boxed of %d)", can, n);
  if (r.nodes.empty()) {
    CHECK(std::memcmp(before.data(), r.recs.data(), before.size() * sizeof(TriRec)) == 0, "the records moved without a hierarchy");
    return;
  }
  r.run.first = 0; r.run.n = n; r.run.n_boxed = n_boxed; r.run.node = 0; r.run.n_nodes = (int32_t)r.nodes.size(); r.run.depth = depth;
  CHECK(n_boxed == can && n_boxed >= 16, "boxed %d, tri_box accepts %d", n_boxed, can);
  if (bad >= 0) CHECK(n - n_boxed >= bad, "remainder %d, ill-conditioned records %d", n - n_boxed, bad);
  CHECK(depth <= kBvhMaxDepth, "depth %d", depth);
  for (int k = 0; k < n; ++k) CHECK(tri_box(r.recs[(size_t)k], r.run.dmax, r.run.omax, blo, bhi) == (k < n_boxed), "record %d on the wrong side", k);
  std::vector<int> metas, metas0;
  for (const TriRec& q : r.recs) metas.push_back(q.meta);
  for (const TriRec& q : before) metas0.push_back(q.meta);
  std::sort(metas.begin(), metas.end());
  std::sort(metas0.begin(), metas0.end());
  CHECK(metas == metas0, "the records are no permutation of the input");
  for (const TriRec& q : r.recs) CHECK(std::memcmp(&q, &before[(size_t)q.tri], sizeof q) == 0, "record %d changed", q.tri);
  std::vector<int> seen((size_t)n_boxed, 0);
  int max_depth = 0;
  walk_tree(r, 0, nullptr, nullptr, seen, 0, &max_depth);
  for (int k = 0; k < n_boxed; ++k) CHECK(seen[(size_t)k] == 1, "boxed record %d in %d leaves", k, seen[(size_t)k]);
  CHECK(max_depth == depth, "reported depth %d, walked %d", depth, max_depth);

  // ---- the rays, in the space of the chained ray
  double ext = 0.0;
  for (int k = 0; k < n; ++k) {
    V p[3];
    tri_points(r, k, p);
    for (const V& q : p) ext = std::fmax(ext, ninf(q));
  }
  const double dmax = r.run.dmax, omax = r.run.omax;
  Tally mine;
  for (int i = 0; i < n_rays; ++i) {
    const int mode = i % 8, k = g.below(n);
    V p[3];
    tri_points(r, k, p);
    double a = g.u(), b = g.u();
    if (a + b > 1.0) { a = 1.0 - a; b = 1.0 - b; }
    V aim = p[0] + a * (p[1] - p[0]) + b * (p[2] - p[0]);
    const V nrm = cross(p[1] - p[0], p[2] - p[0]);
    V o, d;
    // |cd|: anywhere below the bound, a unit vector's image included
    double len = g.below(3) == 0 ? dmax * g.range(0.5, 1.0) / std::sqrt(3.0) : g.logu(std::fmin(1e-3, 0.5 * dmax), dmax / std::sqrt(3.0));
    if (mode == 0 || mode == 4) {  // at a point of a triangle, from outside or (4) from among the triangles
      o = mode == 4 ? V{g.range(-1, 1) * ext, g.range(-1, 1) * ext, g.range(-1, 1) * ext} : aim + g.logu(0.1, 30.0) * ext * unit(V{g.range(-1, 1), g.range(-1, 1), g.range(-1, 1)});
      d = unit(aim - o);
    } else if (mode == 1) {  // grazing: at an edge or a vertex, a hair off it
      const int e = g.below(3);
      const double s = g.below(2) ? g.u() : 0.0;
      aim = p[e] + s * (p[(e + 1) % 3] - p[e]) + g.range(-1e-9, 1e-9) * ext * unit(V{g.range(-1, 1), g.range(-1, 1), g.range(-1, 1)});
      o = aim + g.logu(0.1, 30.0) * ext * unit(V{g.range(-1, 1), g.range(-1, 1), g.range(-1, 1)});
      d = unit(aim - o);
    } else if (mode == 2) {  // in the triangle's plane, or a sliver off it: |det| of 1-4 EPSILON on this triangle
      const V w = unit(p[1 + g.below(2)] - p[0] + g.range(-1, 1) * (p[2] - p[1]));
      const TriRec& q = r.recs[(size_t)k];
      const V e1{q.e1[0], q.e1[1], q.e1[2]}, e2{q.e2[0], q.e2[1], q.e2[2]};
      const double area = norm(cross(e1, e2));
      d = w;
      if (i % 16 != 2 && area > 0.0 && norm(nrm) > 0.0) {
        // object-space det = -(ld . (e1 x e2)): a step s along the normal adds about s * len * area (the records'
        // matrix is near a rotation times a scaling: the factor is absorbed in the range below)
        const double det = g.range(1.0, 4.0) * kEpsilon;
        d = unit(w + (det / (len * area)) * g.range(0.5, 2.0) * unit(nrm));
        ++mine.slivers;
      }
      o = aim - g.logu(0.01, 10.0) * ext * d;
    } else if (mode == 3) {  // zero direction components
      const int ax = g.below(3);
      d = V{ax == 0 ? 1.0 : 0.0, ax == 1 ? 1.0 : 0.0, ax == 2 ? 1.0 : 0.0};
      if (g.below(2)) { d = V{ax == 0 ? 0.0 : g.range(-1, 1), ax == 1 ? 0.0 : g.range(-1, 1), ax == 2 ? 0.0 : g.range(-1, 1)}; d = unit(d); }
      o = aim - g.range(-3.0, 10.0) * ext * d;
    } else if (mode == 5) {  // from origins up to the bound
      const V dir = unit(V{g.range(-1, 1), g.range(-1, 1), g.range(-1, 1)});
      o = (omax * g.range(0.5, 1.0) / ninf(dir)) * dir;
      if (g.below(2)) o = (omax / ninf(o)) * o;
      const double m = ninf(o);
      if (m > omax) o = (omax / m * (1.0 - 1e-15)) * o;
      d = unit(aim - o);
    } else if (mode == 6) {  // just inside and just outside the bounds
      o = aim + g.logu(0.1, 30.0) * ext * unit(V{g.range(-1, 1), g.range(-1, 1), g.range(-1, 1)});
      d = unit(aim - o);
      const bool inside = g.below(2) != 0;
      len = dmax / ninf(d);
      d = len * d;
      const double m = ninf(d);  // the product's rounding can land either side: step to the side asked for
      double* c = std::fabs(d.x) == m ? &d.x : std::fabs(d.y) == m ? &d.y : &d.z;
      *c = std::copysign(inside ? dmax : std::nextafter(dmax, INFINITY), *c);
      CHECK(csg_run_admits(r.run, o, d) == (inside && ninf(o) <= omax), "|cd|_inf %.17g against dmax %.17g", ninf(d), dmax);
      V o2 = o;
      double* c2 = &o2.y;
      *c2 = inside ? omax : std::nextafter(omax, INFINITY);
      CHECK(csg_run_admits(r.run, o2, unit(d)) == inside, "|co|_inf %.17g against omax %.17g", ninf(o2), omax);
      ++mine.near_bound;
      check_ray(g, r, o, d, mine);
      check_ray(g, r, o2, unit(aim - o2), mine);
      continue;
    } else {  // away from everything: the line misses the root's box
      o = (g.range(3.0, 10.0) * ext) * unit(V{g.range(-1, 1), g.range(-1, 1), g.range(-1, 1)});
      d = unit(cross(o, V{g.range(-1, 1), g.range(-1, 1), g.range(-1, 1)}));
      if (ninf(o) <= omax && clear_miss(r, o, d)) {
        long visits = 0;
        csg_run_walk(r.run, r.nodes.data(), o, d, -INFINITY, INFINITY, [&](int kk) { visits += kk < r.run.n_boxed ? 1 : 0; });
        CHECK(visits == 0, "%ld boxed triangles tested by a ray whose line misses the root's box", visits);
        ++mine.misses;
      }
    }
    if (mode != 6) d = len * d;
    if (ninf(o) > omax) continue;
    check_ray(g, r, o, d, mine);
  }
  // what is never admitted
  const V o1{0.1, 0.2, 0.3}, d1{0.0, 0.0, 1.0};
  CHECK(csg_run_admits(r.run, o1, d1), "a plain ray");
  CHECK(!csg_run_admits(r.run, V{NAN, 0, 0}, d1) && !csg_run_admits(r.run, o1, V{0, NAN, 1}) && !csg_run_admits(r.run, V{0, 0, INFINITY}, d1) &&
            !csg_run_admits(r.run, o1, V{-INFINITY, 0, 0}),
        "a ray that is not finite is admitted");
  std::printf("run of %4d (chain %2zu, dmax %9.3g, omax %9.3g): boxed %4d, remainder %3d, nodes %4zu, depth %2d; "
              "rays %ld, admitted %ld, roots %ld, mean leaf tests per walk %.1f\n",
              n, chain.size(), dmax, omax, n_boxed, n - n_boxed, r.nodes.size(), depth, mine.rays, mine.admitted, mine.roots,
              mine.admitted ? (double)mine.visits / (3.0 * (double)mine.admitted) : 0.0);
  tl.rays += mine.rays; tl.admitted += mine.admitted; tl.roots += mine.roots; tl.visits += mine.visits;
  tl.second_walks += mine.second_walks; tl.full += mine.full; tl.near_bound += mine.near_bound; tl.slivers += mine.slivers;
  tl.misses += mine.misses;
}

// a deck of parallel triangles: one ray crosses all of them (more roots than a batch holds)
Run make_deck(int n) {
  Run r;
  r.rec_fwd = scaling(1, 1, 1);
  for (int i = 0; i < n; ++i) {
    TriRec q{};
    const M34 id = scaling(1, 1, 1);
    std::memcpy(q.m, id.m, sizeof q.m);
    const double y = 0.05 * i;
    q.p1[0] = -3.0 - 0.001 * i; q.p1[1] = y; q.p1[2] = -2.5;
    q.e1[0] = 6.0 + 0.001 * i; q.e1[1] = 0.0; q.e1[2] = 0.1 - 0.001 * i;
    q.e2[0] = 3.1 + 0.001 * i; q.e2[1] = 0.0; q.e2[2] = 5.5 + 0.001 * i;
    q.meta = (int32_t)((1000 + i) << 1 | 1);
    q.tri = i;
    r.recs.push_back(q);
  }
  return r;
}

}  // namespace

int main() {
  Rng g{0xC5A1B0C5ull};
  Tally tl;
  int built = 0, scaled = 0, deep = 0, with_remainder = 0;
  // (a) the world-level constants: tri_box's two signatures agree bit for bit
  {
    Run r = make_run(g, 64, 1.0, 0, false, false);
    for (const TriRec& q : r.recs) {
      double a[6], b[6];
      const bool ka = tri_box(q, a, a + 3), kb = tri_box(q, kTriDirMax, kTriOriginMax, b, b + 3);
      CHECK(ka && kb && std::memcmp(a, b, sizeof a) == 0, "tri_box with the constants as parameters differs");
    }
  }
  // (b) seeded runs under chains of 0-4 inverses (the wide form), up to 12 (the deep form)
  const int sizes[] = {16, 17, 24, 40, 64, 96, 150, 250, 400};
  for (int k = 0; k < 36; ++k) {
    const int n = sizes[k % 9];
    const bool is_deep = k >= 27;
    const int links = is_deep ? 5 + g.below(8) : k % 5;
    std::vector<M34> chain;
    // uneven scales: a third of the chains across 1e-2 .. 1e2 (one such link; the others mild), the rest 0.25 .. 4
    for (int j = 0; j < links; ++j) {
      const bool wild = !is_deep && k % 3 == 0 && j == 0;
      chain.push_back(is_deep ? csg_inverse(g, 0.8, 1.25, 1.0) : wild ? csg_inverse(g, 1e-2, 1e2, 5.0) : csg_inverse(g, 0.25, 4.0, 3.0));
    }
    // edges from 1e-3 to 1e2 (the long ones only under mild chains: kappa <= 1e12 is tri_box's rule)
    const double L = k % 4 == 0 ? g.logu(1e-3, 1e-1) : k % 4 == 1 ? g.logu(1.0, 1e2) : g.logu(0.05, 5.0);
    const int bad = k % 6 == 1 ? 2 : 0;
    Run r = make_run(g, n, L, bad, k % 9 == 4, k % 2 == 0);
    // expected of every run but those tri_box may refuse wholesale: a wild link, or edges up to 1e2 (kappa <= 1e12)
    const bool sure = !(k % 3 == 0 && links > 0 && !is_deep) && k % 4 != 1 && n - bad >= 16;
    check_run(g, r, chain, 2400, tl, sure, bad);
    if (!r.nodes.empty()) {
      ++built;
      if (r.run.dmax > 2.0 * kTriDirMax) ++scaled;
      if (is_deep) ++deep;
      if (r.run.n_boxed < r.run.n) ++with_remainder;
    }
  }
  // (c) a deck: more roots than a batch, walks from a watermark
  {
    Run r = make_deck(120);
    const std::vector<M34> chain = {csg_inverse(g, 0.5, 2.0, 1.0)};
    check_run(g, r, chain, 800, tl, true, 0);
    Tally deck;
    for (int i = 0; i < 400; ++i) {
      const V o{g.range(-0.5, 0.5), g.range(-3.0, 9.0), g.range(-0.5, 0.5)};
      const V d = unit(V{g.range(-0.05, 0.05), g.below(2) ? 1.0 : -1.0, g.range(-0.05, 0.05)});
      check_ray(g, r, o, d, deck);
    }
    CHECK(deck.full > 100, "only %ld intervals with more roots than a batch", deck.full);
    tl.full += deck.full; tl.rays += deck.rays; tl.admitted += deck.admitted; tl.roots += deck.roots; tl.second_walks += deck.second_walks;
    ++built;
  }
  // (d) below the threshold, and all refused: no hierarchy, the records untouched
  {
    Run r = make_run(g, 15, 1.0, 0, false, true);
    check_run(g, r, {}, 0, tl, false, -1);
    CHECK(r.nodes.empty(), "a hierarchy over 15 triangles");
    Run r2 = make_run(g, 40, 1.0, 30, false, true);
    check_run(g, r2, {}, 0, tl, false, -1);
    CHECK(r2.nodes.empty(), "a hierarchy over 10 boxed triangles");
    Run r3 = make_run(g, 40, 1.0, 0, false, true);
    const std::vector<M34> inf_chain = {scaling(INFINITY, 1, 1)};
    std::vector<const double*> ms = {inf_chain[0].m};
    double dm, om;
    csg_run_bounds(ms.data(), 1, &dm, &om);
    int nb = 0, dp = 0;
    CHECK(build_csg_run(r3.recs.data(), 40, dm, om, 16, 2, 0.7, &nb, &dp).empty(), "a hierarchy under a chain that is not finite");
  }
  CHECK(built >= 28, "only %d runs with a hierarchy", built);
  CHECK(scaled >= 8, "only %d runs with dmax beyond twice the world's", scaled);
  CHECK(deep >= 6, "only %d runs under a deep chain", deep);
  CHECK(with_remainder >= 4, "only %d runs with a remainder", with_remainder);
  CHECK(tl.admitted > 60000 && tl.roots > 100000, "only %ld admitted rays, %ld roots", tl.admitted, tl.roots);
  CHECK(tl.second_walks > 10000 && tl.near_bound > 5000 && tl.slivers > 5000 && tl.misses > 2000,
        "second walks %ld, rays at the bounds %ld, slivers %ld, clear misses %ld", tl.second_walks, tl.near_bound, tl.slivers, tl.misses);
  CHECK(sliver_roots > 20000, "only %ld roots at |det| below 5 EPSILON", sliver_roots);
  std::printf("roots at |det| < 5 EPSILON: %ld\n", sliver_roots);
  std::printf("runs %d (scaled %d, deep %d, with a remainder %d), rays %ld, admitted %ld, roots %ld, intervals over a batch %ld\n", built,
              scaled, deep, with_remainder, tl.rays, tl.admitted, tl.roots, tl.full);
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
