// rt_alias.hpp — structural shape equality on the host (no device code): the
// superset test and the sorted-key sweep behind RT_ERR_DUPLICATE_SHAPES, the
// exact relation of rt_shapes_equal_pairs, and the split of a caller's equal
// pairs into alias classes (rt_scene_create_aliased). Plain C++: rt_scene.cpp
// and tests/cpp/alias_check.cpp (under the sanitizers) include it.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/rt_render.h"

namespace rtalias {

constexpr double kEps = 0.00001;                                            // lib.rs:18
inline bool eq(double a, double b) { return std::fabs(a - b) < kEps; }      // lib.rs:20-22
inline bool m16_eq(const double* a, const double* b) {
  for (int i = 0; i < 16; ++i)
    if (!eq(a[i], b[i])) return false;
  return true;
}
inline bool c3_eq(const double* a, const double* b) { return eq(a[0], b[0]) && eq(a[1], b[1]) && eq(a[2], b[2]); }

// Necessary condition for the reference's structural `Shape` equality
// (derived PartialEq of BaseShape, geometry/mod.rs:12; Material, material.rs:10;
// Pattern, pattern/mod.rs:17). The bounding box is left out, so this is a
// SUPERSET of the reference relation: "no pair passes" certifies that the
// containers walk never sees two structurally-equal objects.
// `ta`, `tb`: the vertices of a Triangle / SmoothTriangle (null for the other kinds): the derived
// PartialEq compares p1..p3, and n1..n3 of the smooth kind, through Point's and Vector's `equal()`
// (triangle.rs:12, smooth_triangle.rs:12); e1, e2 and normal follow from the points.
inline bool may_be_equal(const rt_shape_desc& a, const rt_shape_desc& b, const rt_triangle_desc* ta = nullptr,
                         const rt_triangle_desc* tb = nullptr) {
  if (a.kind != b.kind || (a.casts_shadow != 0) != (b.casts_shadow != 0)) return false;
  if (ta && tb) {  // first: the triangles of a mesh share everything else
    if (!(c3_eq(ta->p1, tb->p1) && c3_eq(ta->p2, tb->p2) && c3_eq(ta->p3, tb->p3))) return false;
    if (a.kind == RT_SHAPE_SMOOTH_TRIANGLE && !(c3_eq(ta->n1, tb->n1) && c3_eq(ta->n2, tb->n2) && c3_eq(ta->n3, tb->n3)))
      return false;
  }
  if (!m16_eq(a.transform, b.transform) || !m16_eq(a.inverse, b.inverse)) return false;
  if (!c3_eq(a.color, b.color)) return false;
  if (!(a.ambient == b.ambient && a.diffuse == b.diffuse && a.specular == b.specular &&
        a.shininess == b.shininess && a.reflective == b.reflective &&
        a.transparency == b.transparency && a.refractive_index == b.refractive_index))
    return false;
  if ((a.kind == RT_SHAPE_CYLINDER || a.kind == RT_SHAPE_CONE) &&
      !(a.minimum == b.minimum && a.maximum == b.maximum && (a.closed != 0) == (b.closed != 0)))
    return false;
  if (a.pattern_kind != b.pattern_kind) return false;
  if (a.pattern_kind != RT_PATTERN_NONE) {
    if (!m16_eq(a.pattern_transform, b.pattern_transform) ||
        !m16_eq(a.pattern_inverse, b.pattern_inverse))
      return false;
    if (a.pattern_kind != RT_PATTERN_TEST && !(c3_eq(a.pattern_a, b.pattern_a) && c3_eq(a.pattern_b, b.pattern_b)))
      return false;
  }
  return true;
}

// Every pair (i < j) that passes may_be_equal, to `fn(i, j)`; fn returns true to stop the sweep
// (the return value then). `tri_of[i]`: shape i's vertices (null: not a triangle; `tri_of` empty:
// no triangles at all).
// Equal shapes have |translation-x difference| < EPSILON: sweep a sorted key. The triangles of
// a mesh share their transform, so their key adds p1: x + c1 y + c2 z with incommensurable
// weights keeps the vertices of a regular grid apart; equal triangles' keys differ by less
// than (2 + c1 + c2) EPSILON (and the rounding of the key itself, the relative term).
// `which`: the shapes that take part (the others get the key that pairs with nothing, so a mesh of a
// hundred thousand triangles under one transform costs its sort and no comparison where only the
// primitives are asked for).
enum { kSweepAll = 0, kSweepPrimitives = 1, kSweepTriangles = 2 };  // kinds 0-6, Sphere .. Cone, Triangle and SmoothTriangle
template <typename Fn>
inline bool sweep_candidates(const rt_shape_desc* s, size_t n, const std::vector<const rt_triangle_desc*>& tri_of, Fn fn,
                             int which = kSweepAll) {
  constexpr double c1 = 0.7548776662466927, c2 = 0.5698402909980532;
  const bool tris = !tri_of.empty();
  std::vector<std::pair<double, size_t>> key(n);  // (key, shape), sorted by value: no indirection in the sort
  for (size_t i = 0; i < n; ++i) {
    double k = s[i].transform[3];
    if (tris && tri_of[i]) k += tri_of[i]->p1[0] + c1 * tri_of[i]->p1[1] + c2 * tri_of[i]->p1[2];
    const bool tri = s[i].kind >= RT_SHAPE_TRIANGLE;
    const bool in = which == kSweepAll || (which == kSweepTriangles ? tri : !tri);
    key[i] = {in && std::isfinite(k) ? k : INFINITY, i};  // (a non-finite coordinate equals nothing)
  }
  const double window = tris ? (2.0 + c1 + c2) * kEps : kEps;
  std::sort(key.begin(), key.end());
  std::vector<size_t> idx(n);
  for (size_t i = 0; i < n; ++i) idx[i] = key[i].second;
  for (size_t p = 0; p < n; ++p)
    for (size_t q = p + 1;
         q < n && key[q].first - key[p].first < window + (tris ? 1e-13 * (std::fabs(key[q].first) + std::fabs(key[p].first)) : 0.0);
         ++q)
      if (may_be_equal(s[idx[p]], s[idx[q]], tris ? tri_of[idx[p]] : nullptr, tris ? tri_of[idx[q]] : nullptr))
        if (fn(std::min(idx[p], idx[q]), std::max(idx[p], idx[q]))) return true;
  return false;
}

// ---- the exact relation for shapes built by a constructor and at most one set_transform
struct Box {
  double lo[3], hi[3];
};
// BoundingBox::transform (bounding_box.rs:71-89): the eight corners through `m` (rows 0..2 of a
// row-major 4x4, matrix.rs:232-245, its operation order: a 0 * inf is a NaN there too), each
// added to an empty box (:31-52: max first, strict compares, so a NaN coordinate adds nothing).
inline Box box_transform(const Box& b, const double* m) {
  Box nb;
  for (int c = 0; c < 3; ++c) { nb.lo[c] = INFINITY; nb.hi[c] = -INFINITY; }
  for (int k = 0; k < 8; ++k) {
    const double x = (k & 4) ? b.hi[0] : b.lo[0], y = (k & 2) ? b.hi[1] : b.lo[1], z = (k & 1) ? b.hi[2] : b.lo[2];
    for (int c = 0; c < 3; ++c) {
      const double v = m[4 * c] * x + m[4 * c + 1] * y + m[4 * c + 2] * z + m[4 * c + 3];
      if (v > nb.hi[c]) nb.hi[c] = v;
      if (v < nb.lo[c]) nb.lo[c] = v;
    }
  }
  return nb;
}
// The box of a shape after its constructor (sphere.rs:16-25, plane.rs:19-31, cube.rs:17-26,
// cylinder.rs:27-42, cone.rs:26-47) and, unless `transform` is the identity bit for bit, one
// set_transform (geometry/mod.rs:74-85: through the old inverse, the identity, then `transform`).
inline Box shape_box(const rt_shape_desc& d) {
  Box b{{-1.0, -1.0, -1.0}, {1.0, 1.0, 1.0}};
  if (d.kind == RT_SHAPE_PLANE) {
    b = Box{{-INFINITY, 0.0, -INFINITY}, {INFINITY, 0.0, INFINITY}};
  } else if (d.kind == RT_SHAPE_CYLINDER) {
    b.lo[1] = d.minimum; b.hi[1] = d.maximum;
  } else if (d.kind == RT_SHAPE_CONE) {
    const double limit = std::fmax(std::fabs(d.minimum), std::fabs(d.maximum));
    b = Box{{-limit, d.minimum, -limit}, {limit, d.maximum, limit}};
  }
  static const double id[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  if (std::memcmp(d.transform, id, sizeof id) == 0) return b;
  return box_transform(box_transform(b, id), d.transform);
}
// equal_ignore_inf (lib.rs:24-31, its sign test as written), Point's PartialEq (point.rs:26-30)
inline bool eq_ignore_inf(double a, double b) {
  if (std::isinf(a) && std::isinf(b)) return !std::signbit(a) || std::signbit(b);
  return eq(a, b);
}
inline bool box_eq(const Box& a, const Box& b) {
  for (int c = 0; c < 3; ++c)
    if (!eq_ignore_inf(a.lo[c], b.lo[c])) return false;
  for (int c = 0; c < 3; ++c)
    if (!eq_ignore_inf(a.hi[c], b.hi[c])) return false;
  return true;
}
// `a == b` of two such shapes of kinds Sphere .. Cone (the inverse transpose compares as the
// inverse does, entry by entry)
inline bool shapes_equal(const rt_shape_desc& a, const rt_shape_desc& b) {
  if (a.kind < RT_SHAPE_SPHERE || a.kind > RT_SHAPE_CONE) return false;
  return may_be_equal(a, b) && box_eq(shape_box(a), shape_box(b));
}
// every pair (i < j) with shapes[i] == shapes[j], sorted
inline std::vector<std::pair<int32_t, int32_t>> equal_pairs(const rt_shape_desc* s, size_t n) {
  std::vector<std::pair<int32_t, int32_t>> out;
  sweep_candidates(s, n, {}, [&](size_t i, size_t j) {
    if (shapes_equal(s[i], s[j])) out.emplace_back((int32_t)i, (int32_t)j);
    return false;
  }, kSweepPrimitives);
  std::sort(out.begin(), out.end());
  return out;
}

// ---- alias classes
// The pairs' connected components; a component in which every two members are a pair (a clique)
// is one alias class. class_of[i]: shape i's class (-1: in no pair); classes[c]: its members,
// ascending. Returns false for a component that is not a clique, with two of its members that
// are no pair in *bad_a < *bad_b. The pairs are in range, i < j, sorted and distinct.
inline bool split_classes(size_t n_shapes, const int32_t* pairs, size_t n_pairs, std::vector<int32_t>* class_of,
                          std::vector<std::vector<int32_t>>* classes, int32_t* bad_a, int32_t* bad_b) {
  std::vector<int32_t> root(n_shapes);
  for (size_t i = 0; i < n_shapes; ++i) root[i] = (int32_t)i;
  auto find = [&](int32_t x) {
    while (root[(size_t)x] != x) x = root[(size_t)x] = root[(size_t)root[(size_t)x]];
    return x;
  };
  for (size_t p = 0; p < n_pairs; ++p) {
    const int32_t a = find(pairs[2 * p]), b = find(pairs[2 * p + 1]);
    if (a != b) root[(size_t)std::max(a, b)] = std::min(a, b);  // a component's root: its least member
  }
  class_of->assign(n_shapes, -1);
  classes->clear();
  std::vector<char> paired(n_shapes, 0);
  for (size_t p = 0; p < 2 * n_pairs; ++p) paired[(size_t)pairs[p]] = 1;
  for (size_t i = 0; i < n_shapes; ++i) {
    if (!paired[i]) continue;
    const int32_t r = find((int32_t)i);
    if ((*class_of)[(size_t)r] < 0) {
      (*class_of)[(size_t)r] = (int32_t)classes->size();
      classes->emplace_back();
    }
    (*class_of)[i] = (*class_of)[(size_t)r];
    (*classes)[(size_t)(*class_of)[i]].push_back((int32_t)i);
  }
  std::vector<size_t> n_in(classes->size(), 0);
  for (size_t p = 0; p < n_pairs; ++p) ++n_in[(size_t)(*class_of)[(size_t)pairs[2 * p]]];
  for (size_t c = 0; c < classes->size(); ++c) {
    const std::vector<int32_t>& m = (*classes)[c];
    if (n_in[c] == m.size() * (m.size() - 1) / 2) continue;
    // the missing pair: the members' pairs are sorted, so a binary search per candidate
    auto has = [&](int32_t a, int32_t b) {
      size_t lo = 0, hi = n_pairs;
      while (lo < hi) {
        const size_t mid = (lo + hi) / 2;
        if (pairs[2 * mid] < a || (pairs[2 * mid] == a && pairs[2 * mid + 1] < b)) lo = mid + 1;
        else hi = mid;
      }
      return lo < n_pairs && pairs[2 * lo] == a && pairs[2 * lo + 1] == b;
    };
    for (size_t x = 0; x < m.size(); ++x)
      for (size_t y = x + 1; y < m.size(); ++y)
        if (!has(m[x], m[y])) {
          *bad_a = m[x];
          *bad_b = m[y];
          return false;
        }
  }
  return true;
}

}  // namespace rtalias
