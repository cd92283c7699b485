// alias_check.cpp — stand-alone check of csrc/rt_alias.hpp (host code only; built plain and with
// -fsanitize=address,undefined by tests/test_alias_host.py):
//   equal_pairs        against a scan of every pair with shapes_equal, on seeded worlds of spheres,
//                      cubes and cylinders in clusters of exact and near duplicates, chains among them;
//   split_classes      against a restatement (components by flood fill, cliques by asking every pair):
//                      the classes, their members in ascending order, class_of, and for a component
//                      that is no clique a pair of its members that is really missing;
//   box_transform      the 0 * inf rule: a plane's box is empty after any set_transform.
// Prints "OK" and returns 0, or says what failed.
#include <cstdio>
#include <random>
#include <set>

#include "rt_alias.hpp"

using namespace rtalias;

static int failures = 0;
#define CHECK(c, ...)                       \
  do {                                      \
    if (!(c)) {                             \
      if (++failures <= 10) {               \
        std::printf("FAILED %s: ", #c);     \
        std::printf(__VA_ARGS__);           \
        std::printf("\n");                  \
      }                                     \
    }                                       \
  } while (0)

static rt_shape_desc make(int kind, double x, double y, double z, double s) {
  rt_shape_desc d;
  std::memset(&d, 0, sizeof d);
  d.kind = kind;
  d.casts_shadow = 1;
  const double t[16] = {s, 0, 0, x, 0, s, 0, y, 0, 0, s, z, 0, 0, 0, 1};
  const double inv[16] = {1 / s, 0, 0, -x / s, 0, 1 / s, 0, -y / s, 0, 0, 1 / s, -z / s, 0, 0, 0, 1};
  const double id[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  std::memcpy(d.transform, t, sizeof t);
  std::memcpy(d.inverse, inv, sizeof inv);
  std::memcpy(d.pattern_transform, id, sizeof id);
  std::memcpy(d.pattern_inverse, id, sizeof id);
  d.color[0] = d.color[1] = d.color[2] = 1.0;
  d.ambient = 0.1; d.diffuse = 0.9; d.specular = 0.9; d.shininess = 200.0; d.refractive_index = 1.0;
  d.pattern_kind = RT_PATTERN_NONE;
  d.minimum = kind >= RT_SHAPE_CYLINDER ? -1.0 : 0.0;
  d.maximum = kind >= RT_SHAPE_CYLINDER ? 2.0 : 0.0;
  d.closed = kind >= RT_SHAPE_CYLINDER ? 1 : 0;
  return d;
}

static void check_world(unsigned seed) {
  std::mt19937 rng(seed);
  std::uniform_real_distribution<double> pos(-20.0, 20.0), u(0.0, 1.0);
  std::vector<rt_shape_desc> s;
  const int n_clusters = 40 + (int)(seed % 17);
  for (int c = 0; c < n_clusters; ++c) {
    const int kind = (int)(rng() % 4);  // sphere, plane, cube, cylinder
    const double x = pos(rng), y = pos(rng), z = pos(rng), sc = 0.5 + u(rng);
    const int members = 1 + (int)(rng() % 4);
    const double step = u(rng) < 0.3 ? 0.0 : u(rng) < 0.5 ? 2e-6 : 6e-6;  // exact, a clique, a chain from three on
    for (int m = 0; m < members; ++m) {
      rt_shape_desc d = make(kind, x + m * step, y, z, sc);
      if (u(rng) < 0.1) d.casts_shadow = 0;
      if (u(rng) < 0.1) d.refractive_index = 1.5;
      s.push_back(d);
    }
  }
  std::shuffle(s.begin(), s.end(), rng);
  const size_t n = s.size();
  // ---- equal_pairs against every pair
  const std::vector<std::pair<int32_t, int32_t>> got = equal_pairs(s.data(), n);
  std::vector<std::pair<int32_t, int32_t>> want;
  for (size_t i = 0; i < n; ++i)
    for (size_t j = i + 1; j < n; ++j)
      if (shapes_equal(s[i], s[j])) want.emplace_back((int32_t)i, (int32_t)j);
  CHECK(got == want, "seed %u: %zu pairs, a scan finds %zu", seed, got.size(), want.size());
  CHECK(!want.empty(), "seed %u: no pair at all", seed);
  // ---- split_classes against a restatement
  std::vector<int32_t> flat;
  for (const auto& p : got) { flat.push_back(p.first); flat.push_back(p.second); }
  std::set<std::pair<int32_t, int32_t>> has(got.begin(), got.end());
  std::vector<int> comp(n, -1);
  std::vector<std::vector<int32_t>> comps;
  for (size_t i = 0; i < n; ++i) {
    if (comp[i] >= 0) continue;
    bool paired = false;
    for (const auto& p : got) paired = paired || p.first == (int32_t)i || p.second == (int32_t)i;
    if (!paired) continue;
    std::vector<int32_t> todo{(int32_t)i}, mem;
    comp[i] = (int)comps.size();
    while (!todo.empty()) {
      const int32_t a = todo.back();
      todo.pop_back();
      mem.push_back(a);
      for (const auto& p : got) {
        const int32_t b = p.first == a ? p.second : p.second == a ? p.first : -1;
        if (b >= 0 && comp[(size_t)b] < 0) { comp[(size_t)b] = comp[i]; todo.push_back(b); }
      }
    }
    std::sort(mem.begin(), mem.end());
    comps.push_back(mem);
  }
  bool all_cliques = true;
  for (const auto& m : comps)
    for (size_t a = 0; a < m.size(); ++a)
      for (size_t b = a + 1; b < m.size(); ++b) all_cliques = all_cliques && has.count({m[a], m[b]});
  std::vector<int32_t> class_of;
  std::vector<std::vector<int32_t>> classes;
  int32_t ba = -1, bb = -1;
  const bool ok = split_classes(n, flat.data(), got.size(), &class_of, &classes, &ba, &bb);
  CHECK(ok == all_cliques, "seed %u: split says %d, the restatement %d", seed, (int)ok, (int)all_cliques);
  CHECK(classes == comps, "seed %u: %zu classes, the restatement %zu", seed, classes.size(), comps.size());
  for (size_t i = 0; i < n; ++i) CHECK(class_of[i] == comp[i], "seed %u: class_of[%zu] = %d, not %d", seed, i, class_of[i], comp[i]);
  if (!ok) {
    CHECK(ba >= 0 && ba < bb && bb < (int32_t)n && comp[(size_t)ba] >= 0 && comp[(size_t)ba] == comp[(size_t)bb] && !has.count({ba, bb}),
          "seed %u: (%d, %d) is no missing pair of one component", seed, ba, bb);
  }
}

int main() {
  for (unsigned seed = 1; seed <= 60; ++seed) check_world(seed);
  {  // no pairs at all, and no shapes at all
    std::vector<int32_t> class_of;
    std::vector<std::vector<int32_t>> classes;
    int32_t a, b;
    CHECK(split_classes(5, nullptr, 0, &class_of, &classes, &a, &b) && classes.empty() && class_of == std::vector<int32_t>(5, -1), "empty");
    CHECK(split_classes(0, nullptr, 0, &class_of, &classes, &a, &b) && class_of.empty(), "no shapes");
    CHECK(equal_pairs(nullptr, 0).empty(), "no shapes");
  }
  {  // a chain of three and a clique of three
    const int32_t chain[] = {0, 1, 1, 2}, clique[] = {0, 1, 0, 2, 1, 2};
    std::vector<int32_t> class_of;
    std::vector<std::vector<int32_t>> classes;
    int32_t a = -1, b = -1;
    CHECK(!split_classes(3, chain, 2, &class_of, &classes, &a, &b) && a == 0 && b == 2, "chain: (%d, %d)", a, b);
    CHECK(split_classes(4, clique, 3, &class_of, &classes, &a, &b) && classes.size() == 1 && classes[0] == std::vector<int32_t>({0, 1, 2}) &&
              class_of == std::vector<int32_t>({0, 0, 0, -1}), "clique");
  }
  {  // BoundingBox::transform: a plane's infinite box is empty after any set_transform (0 * inf = NaN adds nothing)
    rt_shape_desc p = make(RT_SHAPE_PLANE, 0.0, 1.0, 0.0, 1.0);
    const Box b = shape_box(p);
    CHECK(b.lo[0] == INFINITY && b.hi[0] == -INFINITY && b.lo[1] == INFINITY && b.hi[2] == -INFINITY, "plane box %g %g", b.lo[1], b.hi[1]);
    rt_shape_desc q = make(RT_SHAPE_PLANE, 0.0, 0.0, 0.0, 1.0);  // the identity: set_transform never called
    const Box c = shape_box(q);
    CHECK(c.lo[0] == -INFINITY && c.hi[0] == INFINITY && c.lo[1] == 0.0 && c.hi[1] == 0.0, "default plane box");
    CHECK(eq_ignore_inf(INFINITY, -INFINITY) && !eq_ignore_inf(-INFINITY, INFINITY) && !eq_ignore_inf(INFINITY, 1.0), "lib.rs:24-31 as written");
  }
  {  // a mesh: 20 000 triangles under one transform and material beside two equal spheres. The helper's sweep
     // leaves the triangles out: it meets one candidate pair, where a sweep of every shape by its translation
     // (no vertices at hand) meets every pair of faces. Counted on a smaller mesh for the latter.
    std::vector<rt_shape_desc> s(20000, make(RT_SHAPE_TRIANGLE, 1.0, 2.0, 3.0, 1.0));
    s.push_back(make(RT_SHAPE_SPHERE, 1.0, 2.0, 3.0, 1.0));
    s.push_back(make(RT_SHAPE_SPHERE, 1.0, 2.0, 3.0, 1.0));
    size_t met = 0;
    sweep_candidates(s.data(), s.size(), {}, [&](size_t, size_t) { ++met; return false; }, kSweepPrimitives);
    CHECK(met == 1, "the helper's sweep met %zu candidate pairs", met);
    const auto pairs = equal_pairs(s.data(), s.size());
    CHECK(pairs.size() == 1 && pairs[0] == std::make_pair((int32_t)20000, (int32_t)20001), "%zu pairs beside the mesh", pairs.size());
    met = 0;
    sweep_candidates(s.data() + 19000, 1002, {}, [&](size_t, size_t) { ++met; return false; }, kSweepAll);
    CHECK(met == 1000u * 999u / 2u + 1u, "a sweep of every shape met %zu pairs", met);
    met = 0;  // the triangles alone, with their vertices: the grid key keeps distinct faces apart
    std::vector<rt_triangle_desc> t(1002);
    std::vector<const rt_triangle_desc*> tri_of(1002, nullptr);
    for (size_t i = 0; i < 1000; ++i) {
      std::memset(&t[i], 0, sizeof t[i]);
      t[i].p1[0] = (double)(i % 999);  // faces 0 and 999 are one triangle
      t[i].p2[1] = 1.0;
      t[i].p3[2] = 1.0;
      tri_of[i] = &t[i];
    }
    size_t fa = 0, fb = 0;
    sweep_candidates(s.data() + 19000, 1002, tri_of, [&](size_t a, size_t b) { ++met; fa = a; fb = b; return false; }, kSweepTriangles);
    CHECK(met == 1 && fa == 0 && fb == 999, "the triangles' sweep met %zu pairs (%zu, %zu)", met, fa, fb);
  }
  if (failures) {
    std::printf("%d checks failed\n", failures);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
