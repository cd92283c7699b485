// rt_scene.cpp — rt_scene_create / _groups / _mesh / _tree / rt_scene_destroy:
// the reference's World (world.rs:18-21, shape/group.rs) flattened into SoA
// records in the reference's object order, the exact-culling hierarchies
// (rt_bvh.cpp), the light buffer, and one upload to the scene's device.
#include <functional>

#include "rt_alias.hpp"
#include "rt_api_internal.hpp"
#include "rt_csg.hpp"
#include "rt_wf_plan.hpp"

using namespace rtapi;

static_assert(kCsgMaxLeaves == RT_CSG_MAX_LEAVES && kCsgMaxDepth == RT_CSG_MAX_DEPTH && kCsgMaxNodes == RT_CSG_MAX_NODES,
              "the Csg caps of include/rt_render.h are rt_csg.hpp's");
static_assert(kCsgDeepMaxNodes == RT_CSG_DEEP_MAX_NODES && kCsgDeepMaxLeaves == RT_CSG_DEEP_MAX_LEAVES,
              "the deep units' format limits of include/rt_render.h are rt_layout.hpp's");

namespace {

bool is_diag_inverse(const double* inv) {
  return inv[1] == 0.0 && inv[2] == 0.0 && inv[4] == 0.0 && inv[6] == 0.0 && inv[8] == 0.0 &&
         inv[9] == 0.0;
}

using rtalias::may_be_equal;

// `tri_of[i]`: shape i's vertices (null: not a triangle; `tri_of` empty: no triangles at all).
int find_duplicate(const rt_shape_desc* s, size_t n, const std::vector<const rt_triangle_desc*>& tri_of, size_t* ia,
                   size_t* ib) {
  return rtalias::sweep_candidates(s, n, tri_of, [&](size_t a, size_t b) {
    *ia = a;
    *ib = b;
    return true;
  }) ? 1 : 0;
}

// rt_scene_create_tree (aliased = false: two shapes that may be structurally equal are refused)
// and rt_scene_create_aliased (the caller's equal pairs: alias classes).
int create_tree(const rt_shape_desc* shapes, size_t n_shapes, const int32_t* shape_node, const int32_t* shape_side,
                const rt_node_desc* nodes, size_t n_nodes, const rt_triangle_desc* tri_descs, size_t n_tris,
                const rt_light_desc* lights, size_t n_lights, bool aliased, const int32_t* equal_pairs, size_t n_pairs,
                bool deep_csg, int device, rt_scene** out) {
  if (!out || (n_shapes && !shapes) || (n_lights && !lights) || (n_nodes && (!nodes || !shape_node)) ||
      (n_tris && !tri_descs))
    return fail(RT_ERR_INVALID_ARGUMENT, "null pointer");
  *out = nullptr;
  if (n_shapes > (size_t)(1u << 29)) return fail(RT_ERR_INVALID_ARGUMENT, "too many shapes");
  if (n_nodes > (size_t)(1u << 24)) return fail(RT_ERR_INVALID_ARGUMENT, "too many nodes");
  for (size_t g = 0; g < n_nodes; ++g)
    if (nodes[g].parent < -1 || nodes[g].parent >= (int32_t)g)
      return fail(RT_ERR_INVALID_ARGUMENT, "node " + std::to_string(g) + ": its parent must be -1 or an earlier node");
  // ---- Csg nodes: each node's unit (the outermost Csg at or above it, -1: none) and the
  // Csg nodes from that unit down to it
  // (deep_csg, rt_scene_create_ex: no cap; a unit beyond one is DEEP, rt_layout.hpp kCsgDeep)
  std::vector<int32_t> unit_of_node(n_nodes, -1), csg_level(n_nodes, 0), unit_levels(n_nodes, 0);
  std::vector<char> deep_unit(n_nodes, 0);
  bool any_csg = false;
  for (size_t g = 0; g < n_nodes; ++g) {
    const rt_node_desc& nd = nodes[g];
    if (nd.kind != RT_NODE_GROUP && nd.kind != RT_NODE_CSG)
      return fail(RT_ERR_INVALID_ARGUMENT, "node " + std::to_string(g) + ": bad kind");
    const bool csg = nd.kind == RT_NODE_CSG;
    if (csg && (nd.operation < RT_CSG_UNION || nd.operation > RT_CSG_DIFFERENCE))
      return fail(RT_ERR_INVALID_ARGUMENT, "node " + std::to_string(g) + ": bad Csg operation");
    if (nd.parent >= 0 && nodes[nd.parent].kind == RT_NODE_CSG && nd.side != 0 && nd.side != 1)
      return fail(RT_ERR_INVALID_ARGUMENT, "node " + std::to_string(g) + ": side must be 0 (left) or 1 (right)");
    const int32_t up = nd.parent >= 0 ? unit_of_node[(size_t)nd.parent] : -1;
    unit_of_node[g] = up >= 0 ? up : (csg ? (int32_t)g : -1);
    csg_level[g] = (up >= 0 ? csg_level[(size_t)nd.parent] : 0) + (csg ? 1 : 0);
    any_csg = any_csg || csg;
    if (unit_of_node[g] >= 0) {
      int32_t& lv = unit_levels[(size_t)unit_of_node[g]];
      lv = std::max(lv, csg_level[g]);
    }
    if (csg_level[g] > kCsgMaxDepth && deep_csg) {
      deep_unit[(size_t)unit_of_node[g]] = 1;
      if (csg_level[g] > RT_CSG_DEEP_MAX_LEVELS)
        return fail(RT_ERR_UNSUPPORTED_SHAPE, "node " + std::to_string(g) + ": more than RT_CSG_DEEP_MAX_LEVELS = " +
                                                  std::to_string(RT_CSG_DEEP_MAX_LEVELS) + " nested Csg nodes");
    } else if (csg_level[g] > kCsgMaxDepth)
      return fail(RT_ERR_UNSUPPORTED_SHAPE, "node " + std::to_string(g) + ": more than RT_CSG_MAX_DEPTH = " +
                                                std::to_string(kCsgMaxDepth) + " nested Csg nodes");
  }
  // a shape's gate: 1 + its innermost group (0: none)
  // (range-checked before the + 1: a caller's INT32_MAX must not overflow)
  for (size_t i = 0; shape_node && n_nodes && i < n_shapes; ++i)
    if (shape_node[i] < -1 || (int64_t)shape_node[i] >= (int64_t)n_nodes)
      return fail(RT_ERR_INVALID_ARGUMENT, "shape " + std::to_string(i) + ": bad node index");
  auto gate_of = [&](size_t i) -> int32_t { return shape_node && n_nodes ? shape_node[i] + 1 : 0; };
  for (size_t i = 0; i < n_shapes; ++i) {
    // (without vertex data, rt_scene_create / rt_scene_create_groups: no triangles)
    if (shapes[i].kind < RT_SHAPE_SPHERE || shapes[i].kind > (n_tris ? RT_SHAPE_SMOOTH_TRIANGLE : RT_SHAPE_CONE))
      return fail(RT_ERR_UNSUPPORTED_SHAPE, "shape " + std::to_string(i) +
                                                ": supported kinds are Sphere, Plane, Cube, Cylinder, Cone" +
                                                (n_tris ? ", Triangle, SmoothTriangle" : ""));
    if (shapes[i].pattern_kind < RT_PATTERN_NONE || shapes[i].pattern_kind > RT_PATTERN_CHECKERS)
      return fail(RT_ERR_INVALID_ARGUMENT, "shape " + std::to_string(i) + ": bad pattern kind");
  }
  // a shape under a Csg: a leaf of that Csg's unit. A unit with a triangle leaf is WIDE
  // (csg_wide_eval): no cap on its triangles, kCsgMaxLeaves primitives of kinds 0-4 (the
  // fold's table), kCsgMaxNodes Csg nodes (the filter's bits), as many `other` leaves as the
  // counter packing holds. Every other unit is narrow: kinds 0-4 only, kCsgMaxLeaves of them.
  std::vector<int32_t> unit_of(n_shapes, -1);
  std::vector<char> wide_unit(n_nodes, 0);
  if (any_csg) {
    std::vector<int32_t> n_leaves(n_nodes, 0), n_other(n_nodes, 0), n_csg_nodes(n_nodes, 0);
    for (size_t i = 0; i < n_shapes; ++i) {
      const int32_t nd = shape_node[i];
      if (nd < 0) continue;
      if (nodes[nd].kind == RT_NODE_CSG && (!shape_side || (shape_side[i] != 0 && shape_side[i] != 1)))
        return fail(RT_ERR_INVALID_ARGUMENT, "shape " + std::to_string(i) + ": side must be 0 (left) or 1 (right)");
      const int32_t u = unit_of_node[(size_t)nd];
      if (u < 0) continue;
      unit_of[i] = u;
      if (shapes[i].kind > RT_SHAPE_PLANE && ++n_other[(size_t)u] > kCsgCountOtherMax)
        return fail(RT_ERR_UNSUPPORTED_SHAPE, "node " + std::to_string(u) + ": more than " + std::to_string(kCsgCountOtherMax) +
                                                  " triangles and solids under one Csg (the gates' counter packing)");
      if (shapes[i].kind > RT_SHAPE_CONE) {
        // a mesh is a Group (ObjParser's, Group::divide's): the one refusal kept is a lone triangle as a
        // Csg's own left or right child, which the callers of this entry point were promised
        if (nodes[nd].kind == RT_NODE_CSG)
          return fail(RT_ERR_UNSUPPORTED_SHAPE, "shape " + std::to_string(i) +
                                                    ": a Triangle under a Csg as its own left or right child is not "
                                                    "supported: put it in a Group (triangles inside Groups under a Csg are)");
        wide_unit[(size_t)u] = 1;
        continue;
      }
      if (++n_leaves[(size_t)u] > kCsgMaxLeaves && deep_csg) {
        deep_unit[(size_t)u] = 1;
        if (n_leaves[(size_t)u] > kCsgDeepMaxLeaves)
          return fail(RT_ERR_UNSUPPORTED_SHAPE, "node " + std::to_string(u) + ": more than RT_CSG_DEEP_MAX_LEAVES = " +
                                                    std::to_string(kCsgDeepMaxLeaves) +
                                                    " primitives under one Csg (the deep units' batch tag)");
      } else if (n_leaves[(size_t)u] > kCsgMaxLeaves)
        return fail(RT_ERR_UNSUPPORTED_SHAPE, "node " + std::to_string(u) + ": more than RT_CSG_MAX_LEAVES = " +
                                                  std::to_string(kCsgMaxLeaves) +
                                                  " primitives under one Csg (Sphere, Plane, Cube, Cylinder, Cone; triangles are not counted)");
    }
    for (size_t g = 0; g < n_nodes; ++g) {
      const int32_t u = unit_of_node[g];
      if (u < 0 || nodes[g].kind != RT_NODE_CSG) continue;
      if (++n_csg_nodes[(size_t)u] > kCsgDeepMaxNodes)  // (only with deep_csg: 16 leaves or 4 levels hold fewer)
        return fail(RT_ERR_UNSUPPORTED_SHAPE, "node " + std::to_string(u) + ": more than RT_CSG_DEEP_MAX_NODES = " +
                                                  std::to_string(kCsgDeepMaxNodes) + " Csg nodes in one Csg (the deep units' batch tag)");
      if (n_csg_nodes[(size_t)u] > kCsgMaxNodes && wide_unit[(size_t)u] && deep_csg) deep_unit[(size_t)u] = 1;
      else if (n_csg_nodes[(size_t)u] > kCsgMaxNodes && wide_unit[(size_t)u])
        return fail(RT_ERR_UNSUPPORTED_SHAPE, "node " + std::to_string(u) + ": more than RT_CSG_MAX_NODES = " +
                                                  std::to_string(kCsgMaxNodes) + " Csg nodes in one Csg with triangles below it");
    }
  }
  // the j-th triangle shape takes tri_descs[j]
  std::vector<const rt_triangle_desc*> tri_of;
  if (n_tris) {
    tri_of.assign(n_shapes, nullptr);
    size_t j = 0;
    for (size_t i = 0; i < n_shapes; ++i)
      if (shapes[i].kind >= RT_SHAPE_TRIANGLE) {
        if (j < n_tris) tri_of[i] = tri_descs + j;
        ++j;
      }
    if (j != n_tris)
      return fail(RT_ERR_INVALID_ARGUMENT, "n_tris is " + std::to_string(n_tris) + ", the shapes hold " +
                                               std::to_string(j) + " triangles");
  }
  size_t da, db;
  if (!aliased && find_duplicate(shapes, n_shapes, tri_of, &da, &db))
    return fail(RT_ERR_DUPLICATE_SHAPES, "shapes " + std::to_string(da) + " and " + std::to_string(db) +
                                             " may be structurally equal (containers walk, intersection.rs:63-90)");
  // ---- the caller's equal pairs: alias classes (rt_layout.hpp AliasClass). No pair of
  // primitives is looked for on this path: an unlisted pair is distinct. (Triangles: below.)
  std::vector<int32_t> class_of;                 // per shape: its alias class, -1 none
  std::vector<std::vector<int32_t>> alias_cls;   // per class: its members, ascending
  if (aliased) {
    for (size_t p = 0; p < n_pairs; ++p) {
      const int64_t a = equal_pairs[2 * p], b = equal_pairs[2 * p + 1];
      const std::string which = "equal pair " + std::to_string(p) + " (" + std::to_string(a) + ", " + std::to_string(b) + ")";
      if (a < 0 || b >= (int64_t)n_shapes || a >= b)
        return fail(RT_ERR_INVALID_ARGUMENT, which + ": needs 0 <= i < j < n_shapes");
      if (p > 0 && !(equal_pairs[2 * p - 2] < a || (equal_pairs[2 * p - 2] == a && equal_pairs[2 * p - 1] < b)))
        return fail(RT_ERR_INVALID_ARGUMENT, which + ": the pairs must be sorted by (i, j), without repeats");
      if (!may_be_equal(shapes[a], shapes[b], n_tris ? tri_of[(size_t)a] : nullptr, n_tris ? tri_of[(size_t)b] : nullptr))
        return fail(RT_ERR_INVALID_ARGUMENT, which + ": the two descriptors differ in a field structural equality compares");
    }
    for (size_t p = 0; p < n_pairs; ++p) {
      const int32_t a = equal_pairs[2 * p], b = equal_pairs[2 * p + 1];
      const std::string which = "shapes " + std::to_string(a) + " and " + std::to_string(b) + " are structurally equal";
      if (shapes[a].kind >= RT_SHAPE_TRIANGLE)
        return fail(RT_ERR_DUPLICATE_SHAPES, which + ": aliased triangles are not supported");
      if (unit_of[(size_t)a] >= 0 || unit_of[(size_t)b] >= 0)
        return fail(RT_ERR_DUPLICATE_SHAPES, which + ": an aliased primitive under a Csg is not supported");
    }
    // The triangles keep the other entry points' refusal, listed or not: no yardstick restates
    // structural equality for them, so two that may be equal are never rendered as distinct.
    if (n_tris && rtalias::sweep_candidates(shapes, n_shapes, tri_of, [&](size_t a, size_t b) { da = a; db = b; return true; },
                                            rtalias::kSweepTriangles))
      return fail(RT_ERR_DUPLICATE_SHAPES, "shapes " + std::to_string(da) + " and " + std::to_string(db) +
                                               " may be structurally equal: aliased triangles are not supported");
    int32_t ba = -1, bb = -1;
    if (!rtalias::split_classes(n_shapes, equal_pairs, n_pairs, &class_of, &alias_cls, &ba, &bb))
      return fail(RT_ERR_DUPLICATE_SHAPES,
                  "shapes " + std::to_string(ba) + " and " + std::to_string(bb) +
                      " are not equal but are linked by a chain of equal pairs: structural equality is not transitive"
                      " there, and only complete components (alias classes) are supported");
  }
  if (class_of.empty()) class_of.assign(n_shapes, -1);

  int ndev = rt_device_count();
  if (ndev <= 0) return fail(RT_ERR_NO_DEVICE, "no HIP device available (no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(RT_ERR_INVALID_ARGUMENT, "bad device ordinal");

  // ---- flatten (reference object order preserved through `meta`)
  std::vector<SphereDiag> diag;
  std::vector<SphereGen> gen;
  std::vector<PlaneRec> planes;
  std::vector<QuadRec> quads;
  std::vector<TriRec> tris;
  std::vector<TriShade> tri_shade;
  std::vector<ShadeRec> shade(n_shapes);
  std::vector<OtherRec> csg_leaves;  // the leaves under Csg units live only here ...
  std::vector<TriRec> csg_tris;      // ... the triangles among them here: no hierarchy, light buffer or image knows them
  std::vector<int32_t> leaf_of(n_shapes, -1);
  // Triangle::new / SmoothTriangle::new (triangle.rs:24-44, smooth_triangle.rs:27-55)
  auto make_tri = [&](size_t i, int32_t gate) {
    const rt_shape_desc& d = shapes[i];
    const rt_triangle_desc& t = *tri_of[i];
    const rt::Point p1(t.p1[0], t.p1[1], t.p1[2]), p2(t.p2[0], t.p2[1], t.p2[2]), p3(t.p3[0], t.p3[1], t.p3[2]);
    const rt::Vector e1 = p2 - p1, e2 = p3 - p1, normal = rt::cross(e2, e1).normalize();
    TriRec r{};
    TriShade ts{};
    for (int e = 0; e < 12; ++e) r.m[e] = d.inverse[e];
    const double p[3] = {p1.x, p1.y, p1.z}, a[3] = {e1.x, e1.y, e1.z}, b[3] = {e2.x, e2.y, e2.z};
    const double nn[3] = {normal.x, normal.y, normal.z};
    for (int c = 0; c < 3; ++c) {
      r.p1[c] = ts.p1[c] = p[c]; r.e1[c] = ts.e1[c] = a[c]; r.e2[c] = ts.e2[c] = b[c];
      ts.normal[c] = nn[c]; ts.n1[c] = t.n1[c]; ts.n2[c] = t.n2[c]; ts.n3[c] = t.n3[c];
    }
    r.meta = (int32_t)(((int64_t)i << 1) | (d.casts_shadow ? 1 : 0));
    r.gate = gate;
    r.kind = d.kind;
    r.tri = (int32_t)tri_shade.size();
    tri_shade.push_back(ts);
    return r;
  };
  int32_t n_csg_kind[3] = {0, 0, 0};  // by counter class: spheres, planes, others
  // the alias classes' members, class by class (a class's members in object order); they enter
  // no other record list, so no sphere image, LDS plan, light buffer, own-sphere shadow rule or
  // hierarchy knows them: every ray tests every member behind its group gate (alias_classes)
  std::vector<OtherRec> alias_rec;
  std::vector<AliasClass> alias_tab;
  std::vector<int32_t> alias_of;  // (only a world with a class has the table)
  int32_t n_alias_kind[3] = {0, 0, 0};
  if (!alias_cls.empty()) {
    alias_of.assign(n_shapes + 1, 0);
    for (size_t i = 0; i < n_shapes; ++i) alias_of[i] = class_of[i] >= 0 ? alias_cls[(size_t)class_of[i]][0] : (int32_t)i;
  }
  for (const std::vector<int32_t>& members : alias_cls) {
    alias_tab.push_back(AliasClass{(int32_t)alias_rec.size(), (int32_t)members.size()});
    for (const int32_t i : members) {
      const rt_shape_desc& d = shapes[i];
      OtherRec r{};
      for (int e = 0; e < 12; ++e) r.m[e] = d.inverse[e];
      r.minimum = d.minimum;
      r.maximum = d.maximum;
      r.kind = d.kind;
      r.closed = d.closed ? 1 : 0;
      r.meta = (int32_t)(((int64_t)i << 1) | (d.casts_shadow ? 1 : 0));
      r.gate = gate_of((size_t)i);
      alias_rec.push_back(r);
    }
  }
  for (size_t i = 0; i < n_shapes; ++i) {
    const rt_shape_desc& d = shapes[i];
    const int64_t meta = ((int64_t)i << 1) | (d.casts_shadow ? 1 : 0);
    const int32_t gate = gate_of(i);  // shapes inside groups: general records with their group gate
    if (class_of[i] >= 0) {  // a member of an alias class: only in its class's records (below)
      ++n_alias_kind[d.kind == RT_SHAPE_SPHERE ? 0 : d.kind == RT_SHAPE_PLANE ? 1 : 2];
    } else if (unit_of[i] >= 0 && d.kind >= RT_SHAPE_TRIANGLE) {  // a wide unit's leaf (kCsgTri)
      leaf_of[i] = (int32_t)csg_tris.size();
      csg_tris.push_back(make_tri(i, 0));
      ++n_csg_kind[2];
    } else if (unit_of[i] >= 0) {  // its gates are the unit's program's (csg_units)
      OtherRec r{};
      for (int e = 0; e < 12; ++e) r.m[e] = d.inverse[e];
      r.minimum = d.minimum;
      r.maximum = d.maximum;
      r.kind = d.kind;
      r.closed = d.closed ? 1 : 0;
      r.meta = (int32_t)meta;
      leaf_of[i] = (int32_t)csg_leaves.size();
      csg_leaves.push_back(r);
      ++n_csg_kind[d.kind == RT_SHAPE_SPHERE ? 0 : d.kind == RT_SHAPE_PLANE ? 1 : 2];
    } else if (d.kind == RT_SHAPE_SPHERE) {
      if (is_diag_inverse(d.inverse) && gate == 0) {
        SphereDiag r{};
        r.s[0] = d.inverse[0]; r.s[1] = d.inverse[5]; r.s[2] = d.inverse[10];
        r.t[0] = d.inverse[3]; r.t[1] = d.inverse[7]; r.t[2] = d.inverse[11];
        r.meta = meta;
        diag.push_back(r);
      } else {
        SphereGen r{};
        for (int e = 0; e < 12; ++e) r.m[e] = d.inverse[e];
        r.meta = meta;
        r.gate = gate;
        gen.push_back(r);
      }
    } else if (d.kind == RT_SHAPE_PLANE) {
      PlaneRec r{};
      for (int e = 0; e < 4; ++e) r.m[e] = d.inverse[4 + e];
      r.meta = meta;
      r.gate = gate;
      planes.push_back(r);
    } else if (d.kind >= RT_SHAPE_TRIANGLE) {
      tris.push_back(make_tri(i, gate));
    } else {
      QuadRec r{};
      for (int e = 0; e < 12; ++e) r.m[e] = d.inverse[e];
      r.minimum = d.minimum;
      r.maximum = d.maximum;
      r.kind = d.kind;
      r.closed = d.closed ? 1 : 0;
      r.meta = (int32_t)meta;
      r.gate = gate;
      quads.push_back(r);
    }
    ShadeRec& s = shade[i];
    std::memset(&s, 0, sizeof s);
    for (int e = 0; e < 12; ++e) s.inv[e] = d.inverse[e];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) s.invT[r * 3 + c] = d.inverse[c * 4 + r];  // transpose (matrix.rs:79-89)
    for (int c = 0; c < 3; ++c) s.color[c] = d.color[c];
    s.ambient = d.ambient; s.diffuse = d.diffuse; s.specular = d.specular; s.shininess = d.shininess;
    s.reflective = d.reflective; s.transparency = d.transparency; s.refractive_index = d.refractive_index;
    s.pattern_kind = d.pattern_kind;
    for (int c = 0; c < 3; ++c) { s.pat_a[c] = d.pattern_a[c]; s.pat_b[c] = d.pattern_b[c]; }
    for (int e = 0; e < 12; ++e) s.pat_inv[e] = d.pattern_inverse[e];
    s.kind = d.kind;
    s.pad0 = d.kind >= RT_SHAPE_TRIANGLE ? (int32_t)tri_shade.size() : 0;  // 1 + its TriShade (pushed above)
    s.shadow = d.casts_shadow ? 1 : 0;
    s.minimum = d.minimum;
    s.maximum = d.maximum;
  }
  // exact-culling hierarchy over the diagonal spheres (reorders `diag`; keys
  // come from `meta`, so the order changes no result)
  int bvh_depth = 0;
  const int leaf = g_bvh_leaf > 0 ? g_bvh_leaf : 2;
  std::vector<BvhNode> bvh = build_sphere_bvh(diag, leaf, &bvh_depth, g_bvh_ct / 100.0);
  if (g_bvh_leaf == 0 && !bvh.empty()) {
    // a scene whose pair image (stack, nodes, sphere records) does not fit in
    // LDS is traversed from global memory, where single-sphere leaves win
    if (pair_image_leaf_estimate(bvh_depth, bvh.size(), diag.size()) > kFusedLdsLimit) bvh = build_sphere_bvh(diag, 1, &bvh_depth, g_bvh_ct / 100.0);
  }
  const std::vector<BvhPair> bvh_pair = pair_layout(bvh);
  int wide_stack = 0;
  const std::vector<BvhWide> bvh_wide = wide_layout(bvh, diag, &wide_stack);
  const std::vector<BvhWide16> bvh_wide16 = wide16_layout(bvh_wide);
  // ... and over the other bounded records (general spheres, cubes, cylinders
  // with finite caps); the rest stays exhaustive on the fast path too
  std::vector<OtherRec> orec;
  std::vector<SphereGen> fx_gen;
  std::vector<QuadRec> fx_quads;
  double blo[3], bhi[3];
  // (shapes inside groups too: their group gate goes with them, tested before the
  // shape at the leaf, as the reference tests a group's box before its children)
  for (const SphereGen& g : gen) {
    OtherRec r{};
    for (int e = 0; e < 12; ++e) r.m[e] = g.m[e];
    r.kind = 0;
    r.meta = (int32_t)g.meta;
    r.gate = g.gate;
    if (other_box(r, blo, bhi)) orec.push_back(r);
    else fx_gen.push_back(g);
  }
  std::vector<QuadRec> line_rec;  // open tubes and cones with finite bounds: the line hierarchy
  for (const QuadRec& q : quads) {
    if (other_box(q, blo, bhi)) orec.push_back(q);
    else if (q.gate == 0 && line_box(q, blo, bhi)) line_rec.push_back(q);  // (grouped tubes and cones: exhaustive)
    else fx_quads.push_back(q);
  }
  // ---- the Csg units' programs (rt_layout.hpp CsgOp), nodes and leaves depth first
  std::vector<CsgUnit> csg_units;
  std::vector<CsgOp> csg_ops;
  std::vector<CsgRec> csg_nodes;
  std::vector<uint32_t> csg_counts;  // per op: spheres, planes below (what a deep unit's gates read)
  long long deep_plan[4] = {0, 0, 0, 0};  // deep units; the largest one's levels, nodes, leaves of kinds 0-4
  if (any_csg) {
    // a node's children: sub-nodes and shapes, by the first shape below them (the shapes come depth first)
    struct Child { int32_t first, side, node, shape; };
    std::vector<std::vector<Child>> kids(n_nodes);
    std::vector<int32_t> first_shape(n_nodes, INT32_MAX);
    for (size_t i = n_shapes; i-- > 0;) {
      for (int32_t g = shape_node[i]; g >= 0; g = nodes[g].parent) first_shape[(size_t)g] = (int32_t)i;
    }
    for (size_t i = 0; i < n_shapes; ++i)
      if (unit_of[i] >= 0) kids[(size_t)shape_node[i]].push_back(Child{(int32_t)i, shape_side ? shape_side[i] : 0, -1, (int32_t)i});
    for (size_t g = 0; g < n_nodes; ++g)
      if (unit_of_node[g] >= 0 && unit_of_node[g] != (int32_t)g)
        kids[(size_t)nodes[g].parent].push_back(Child{first_shape[g], nodes[g].side, (int32_t)g, -1});
    for (auto& k : kids) std::stable_sort(k.begin(), k.end(), [](const Child& a, const Child& b) { return a.first < b.first; });
    int32_t next_shape = 0, unit_rec = 0, next_slot = 0;
    bool in_order = true, two_sided = true, deep_now = false;
    // emits the node's subtree; cnt: its leaves by counter class; above: the CsgRec of the
    // innermost Csg above the node (-1: none, the node is the unit's own)
    std::function<void(int32_t, int32_t*, int32_t)> emit = [&](int32_t g, int32_t* cnt, int32_t above) {
      const rt_node_desc& nd = nodes[g];
      const size_t at = csg_ops.size();
      const bool csg = nd.kind == RT_NODE_CSG;
      const int32_t rec = (int32_t)csg_nodes.size();
      if (csg) {
        CsgRec r{};
        for (int e = 0; e < 12; ++e) r.m[e] = nd.inverse[e];
        for (int c = 0; c < 3; ++c) { r.lo[c] = nd.min[c]; r.hi[c] = nd.max[c]; }
        r.op = nd.operation;
        r.self = rec - unit_rec;
        r.parent = above < 0 ? -1 : above - unit_rec;
        csg_nodes.push_back(r);
      }
      const int32_t inner = csg ? rec : above;  // the innermost Csg above this node's children
      csg_ops.push_back(CsgOp{csg ? kCsgEnter : kCsgGroup, csg ? rec : g, 0, 0});
      int32_t mine[3] = {0, 0, 0};
      int n_side[2] = {0, 0};
      for (int pass = 0; pass < (csg ? 2 : 1); ++pass) {
        if (csg && pass == 1) csg_nodes[(size_t)rec].split = next_shape;  // the right child's first object
        for (const Child& c : kids[(size_t)g]) {
          if (csg && c.side != pass) continue;
          ++n_side[pass];
          if (c.node >= 0) {
            emit(c.node, mine, inner);
          } else {
            in_order = in_order && c.shape == next_shape;
            next_shape = c.shape + 1;
            const int k = shapes[c.shape].kind;
            const int32_t leaf = leaf_of[(size_t)c.shape];
            ++mine[k == RT_SHAPE_SPHERE ? 0 : k == RT_SHAPE_PLANE ? 1 : 2];
            if (k >= RT_SHAPE_TRIANGLE) {
              tri_shade[(size_t)csg_tris[(size_t)leaf].tri].csg = 1 + inner;
              csg_ops.push_back(CsgOp{kCsgTri, leaf, 0, 0});
            } else {
              csg_leaves[(size_t)leaf].gate = next_slot++;  // its place in the wide fold's table (CsgNegTable)
              csg_ops.push_back(CsgOp{kCsgLeaf, leaf, 0, 0});
            }
          }
        }
      }
      if (csg) {
        two_sided = two_sided && n_side[0] == 1 && n_side[1] == 1;
        csg_ops.push_back(CsgOp{kCsgExit, rec, 0, 0});
      }
      csg_ops[at].skip_to = (int32_t)csg_ops.size();
      // (a deep unit's spheres and planes are in csg_counts alone: the packed fields hold 31 each)
      const int32_t others[3] = {0, 0, mine[2]};
      csg_ops[at].counts = csg_pack_counts(deep_now ? others : mine);
      csg_counts.resize(2 * csg_ops.size(), 0u);
      csg_counts[2 * at] = (uint32_t)mine[0];
      csg_counts[2 * at + 1] = (uint32_t)mine[1];
      for (int c = 0; c < 3; ++c) cnt[c] += mine[c];
    };
    for (size_t g = 0; g < n_nodes; ++g) {
      if (unit_of_node[g] != (int32_t)g) continue;
      CsgUnit u{};
      u.first = (int32_t)csg_ops.size();
      u.gate = nodes[g].parent + 1;
      int32_t cnt[3] = {0, 0, 0};
      next_shape = first_shape[g] == INT32_MAX ? 0 : first_shape[g];
      unit_rec = (int32_t)csg_nodes.size();
      next_slot = 0;
      deep_now = deep_unit[g] || g_csg_deep_all;
      emit((int32_t)g, cnt, -1);
      u.n = (int32_t)csg_ops.size() - u.first;
      if (deep_now) u.n |= kCsgDeep;
      else if (wide_unit[g] || g_csg_wide_all) u.n |= kCsgWide;
      const int32_t others[3] = {0, 0, cnt[2]};
      u.counts = csg_pack_counts(deep_now ? others : cnt);
      if (deep_now) {
        ++deep_plan[0];
        deep_plan[1] = std::max<long long>(deep_plan[1], unit_levels[g]);
        deep_plan[2] = std::max<long long>(deep_plan[2], (long long)csg_nodes.size() - unit_rec);
        deep_plan[3] = std::max<long long>(deep_plan[3], next_slot);
      }
      csg_units.push_back(u);
    }
    if (!two_sided) return fail(RT_ERR_INVALID_ARGUMENT, "a Csg node needs exactly one left and one right child");
    if (!in_order)
      return fail(RT_ERR_INVALID_ARGUMENT, "the shapes under a Csg are not in depth-first order (left before right)");
  }
  // ---- the run hierarchies (rt_layout.hpp CsgRun): per maximal sequence of kCsgTri ops, whose
  // records are consecutive in csg_tris (the shapes come depth first), bounds on the chained ray
  // from the Csg inverses above it, then a hierarchy over the boxed records when there are
  // g_csg_run_min of them. The records are put in leaf order inside their own range, the remainder
  // last: the ops keep their `arg`, so each names another record of the same run than before, and
  // nothing depends on the order inside a run (the batch is ordered by (t, key), keys come from
  // `meta`, the shading record from `tri`).
  std::vector<CsgRun> csg_runs;
  std::vector<BvhNode> csg_run_nodes;
  long long run_plan[4] = {0, 0, 0, 0};  // triangles boxed, remainder, nodes, greatest depth
  for (const CsgUnit& u : csg_units) {
    std::vector<const double*> chain;
    const int32_t end = u.first + (u.n & ~kCsgKindMask);
    for (int32_t pc = u.first; pc < end;) {
      const CsgOp& op = csg_ops[(size_t)pc];
      if (op.code == kCsgEnter) chain.push_back(csg_nodes[(size_t)op.arg].m);
      else if (op.code == kCsgExit && !chain.empty()) chain.pop_back();
      if (op.code != kCsgTri) {
        ++pc;
        continue;
      }
      int32_t past = pc + 1;
      while (past < end && csg_ops[(size_t)past].code == kCsgTri && csg_ops[(size_t)past].arg == op.arg + (past - pc)) ++past;
      const int32_t n = past - pc;
      if (n >= g_csg_run_min && csg_runs.size() < (size_t)INT32_MAX - 1) {
        CsgRun run{};
        csg_run_bounds(chain.data(), (int)chain.size(), &run.dmax, &run.omax);
        int n_boxed = 0, depth = 0;
        const std::vector<BvhNode> nodes = build_csg_run(&csg_tris[(size_t)op.arg], n, run.dmax, run.omax, g_csg_run_min,
                                                         leaf, g_bvh_ct / 100.0, &n_boxed, &depth);
        if (!nodes.empty()) {
          run.first = op.arg;
          run.n = n;
          run.n_boxed = n_boxed;
          run.node = (int32_t)csg_run_nodes.size();
          run.n_nodes = (int32_t)nodes.size();
          run.depth = depth;
          csg_run_nodes.insert(csg_run_nodes.end(), nodes.begin(), nodes.end());
          csg_runs.push_back(run);
          csg_ops[(size_t)pc].skip_to = past;
          csg_ops[(size_t)pc].counts = (int32_t)csg_runs.size();  // 1 + the run's index
          run_plan[0] += n_boxed;
          run_plan[1] += n - n_boxed;
          run_plan[2] += (long long)nodes.size();
          run_plan[3] = std::max<long long>(run_plan[3], depth);
        }
      }
      pc = past;
    }
  }
  std::vector<GroupRec> grec(n_nodes);
  for (size_t g = 0; g < n_nodes; ++g) {
    for (int c = 0; c < 3; ++c) { grec[g].lo[c] = nodes[g].min[c]; grec[g].hi[c] = nodes[g].max[c]; }
    grec[g].parent = nodes[g].parent + 1;
  }
  // A handful of records is cheaper in the exhaustive loops (wave-uniform, scalar loads) than
  // behind a per-lane walk from global memory: the hierarchies start at kMinHierRecords
  // (640x480 frames: the groups scene's 7 grouped records 0.92 ms in the hierarchies, 0.69
  // exhaustive; solids 0.72 -> 0.60, zoo 0.37 -> 0.29; a divided group of 800: 5.1 against
  // 32.3), except in a scene without any other hierarchy, where one of
  // them is what opens the fused generations (the hexagon demo: 1.0 -> 0.53 ms)
  constexpr size_t kMinHierRecords = 16;
  int obvh_depth = 0;
  std::vector<BvhNode> obvh;
  if (orec.size() >= kMinHierRecords || (bvh.empty() && !orec.empty()))
    obvh = build_other_bvh(orec, leaf, &obvh_depth, g_bvh_ct / 100.0);
  if (obvh_depth > kBvhMaxDepth) obvh.clear();  // deeper than other_trace's stack: exhaustive
  int lbvh_depth = 0;
  std::vector<ConeCluster> lclus;
  std::vector<int32_t> lcone;
  std::vector<BvhNode> lbvh;
  if (line_rec.size() >= kMinHierRecords || (bvh.empty() && obvh.empty() && !line_rec.empty()))
    lbvh = build_line_bvh(line_rec, &lclus, &lcone, &lbvh_depth);
  if (lbvh.empty() || lbvh_depth > kBvhMaxDepth) {  // exhaustive, as before the line hierarchy
    for (const QuadRec& q : line_rec) fx_quads.push_back(q);
    line_rec.clear();
    lbvh.clear();
    lclus.clear();
    lcone.clear();
  }
  // ... and over the triangles (tri_trace: grouped ones too, their gate at the leaf); those
  // without a box (an ill-conditioned inverse), or all of them below the threshold, stay exhaustive
  std::vector<TriRec> trec, fx_tris;
  for (const TriRec& r : tris) (tri_box(r, blo, bhi) ? trec : fx_tris).push_back(r);
  int tbvh_depth = 0;
  std::vector<BvhNode> tbvh;
  if (trec.size() >= kMinHierRecords || (bvh.empty() && obvh.empty() && lbvh.empty() && !trec.empty()))
    tbvh = build_tri_bvh(trec, leaf, &tbvh_depth, g_bvh_ct / 100.0);
  if (tbvh.empty() || tbvh_depth > kBvhMaxDepth) {  // none, or deeper than tri_trace's stack: exhaustive
    fx_tris = tris;
    trec.clear();
    tbvh.clear();
  }
  // ... and over the Csg units (unit_trace): only the 16-byte unit records are split and put in
  // leaf order; a unit without a box (a plane or cone leaf, an unbounded cylinder, an
  // ill-conditioned chain) stays in the loop. Built from g_csg_hier_min boxed units on, with no
  // "only hierarchy" exception: a handful of units is cheaper behind the reference's own gates.
  std::vector<CsgUnit> urec, fx_units;
  std::vector<double> unit_boxes;
  for (const CsgUnit& u : csg_units) {
    // (a wide or deep unit has no box: it stays in the loop, behind the reference's own Csg gate)
    if (!(u.n & kCsgKindMask) && csg_unit_box(csg_ops.data(), u.first, u.n, csg_nodes.data(), csg_leaves.data(), blo, bhi)) {
      urec.push_back(u);
      unit_boxes.insert(unit_boxes.end(), blo, blo + 3);
      unit_boxes.insert(unit_boxes.end(), bhi, bhi + 3);
    } else {
      fx_units.push_back(u);
    }
  }
  int ubvh_depth = 0;
  std::vector<BvhNode> ubvh;
  if (!urec.empty() && urec.size() >= (size_t)g_csg_hier_min) {
    // (a unit's evaluation costs tens of node visits: one unit a leaf unless the knob says otherwise)
    std::vector<int> order;
    ubvh = build_unit_bvh(unit_boxes, g_bvh_leaf > 0 ? g_bvh_leaf : 1, &ubvh_depth, &order, 0.05);
    if (!ubvh.empty()) {
      std::vector<CsgUnit> in_order;
      for (int i : order) in_order.push_back(urec[(size_t)i]);
      urec.swap(in_order);
    }
  }
  if (ubvh.empty() || ubvh_depth > kBvhMaxDepth) {  // none, or deeper than unit_trace's stack: the loop
    fx_units = csg_units;
    urec.clear();
    ubvh.clear();
    ubvh_depth = 0;
  }
  std::vector<int32_t> lrec_clus(line_rec.size(), -1);  // each cone's cluster (line_trace's pre-pass check)
  for (size_t c = 0; c < lclus.size(); ++c)
    for (int32_t j = lclus[c].first; j < lclus[c].first + lclus[c].count; ++j) lrec_clus[(size_t)lcone[(size_t)j]] = (int32_t)c;
  if (obvh.empty()) {  // (only when there are no records, or more than the leaf codes can index)
    for (const OtherRec& r : orec) {
      if (r.kind == 0) {
        SphereGen g{};
        for (int e = 0; e < 12; ++e) g.m[e] = r.m[e];
        g.meta = r.meta;
        g.gate = r.gate;
        fx_gen.push_back(g);
      } else {
        fx_quads.push_back(r);
      }
    }
    orec.clear();
  }
  std::vector<LightRec> lrec(n_lights);
  for (size_t i = 0; i < n_lights; ++i)
    for (int c = 0; c < 3; ++c) { lrec[i].pos[c] = lights[i].position[c]; lrec[i].intensity[c] = lights[i].intensity[c]; }
  // light buffers over the (reordered) diagonal spheres: the shadow rays' cell lists
  LightBuffer lb;
  const int lb_res = g_lb_res >= 0 ? g_lb_res : (diag.size() > 4096 ? 512 : 256);
  if (!diag.empty() && n_lights > 0 && n_lights <= (size_t)kLbMaxLights && lb_res > 0)
    lb = build_light_buffer(diag, lrec, lb_res);

  // ---- one blob, 64-B aligned sections
  auto align = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t o_diag = 0;
  // one zeroed padding record after each trace section (look-ahead loads)
  const size_t o_gen = align(o_diag + (diag.size() + 1) * sizeof(SphereDiag));
  const size_t o_pl = align(o_gen + (gen.size() + 1) * sizeof(SphereGen));
  const size_t o_qd = align(o_pl + (planes.size() + 1) * sizeof(PlaneRec));
  const size_t o_bv = align(o_qd + (quads.size() + 1) * sizeof(QuadRec));
  const size_t o_bp = align(o_bv + (bvh.size() + 1) * sizeof(BvhNode));
  const size_t o_bw = align(o_bp + (bvh_pair.size() + 1) * sizeof(BvhPair));
  const size_t o_bh = align(o_bw + (bvh_wide.size() + 1) * sizeof(BvhWide));
  const size_t o_ob = align(o_bh + (bvh_wide16.size() + 1) * sizeof(BvhWide16));
  const size_t o_or = align(o_ob + (obvh.size() + 1) * sizeof(BvhNode));
  const size_t o_lb = align(o_or + (orec.size() + 1) * sizeof(OtherRec));
  const size_t o_lr = align(o_lb + (lbvh.size() + 1) * sizeof(BvhNode));
  const size_t o_cc = align(o_lr + (line_rec.size() + 1) * sizeof(QuadRec));
  const size_t o_lm = align(o_cc + (lclus.size() + 1) * sizeof(ConeCluster));
  const size_t o_lk = align(o_lm + (lcone.size() + 1) * sizeof(int32_t));
  const size_t o_fg = align(o_lk + (lrec_clus.size() + 1) * sizeof(int32_t));
  const size_t o_fq = align(o_fg + (fx_gen.size() + 1) * sizeof(SphereGen));
  const size_t o_sh = align(o_fq + (fx_quads.size() + 1) * sizeof(QuadRec));
  const size_t o_rt = align(o_sh + shade.size() * sizeof(ShadeRec));
  const size_t o_od = align(o_rt + (shade.size() + 1) * 2 * sizeof(double));
  const size_t o_li = align(o_od + (shade.size() + 1) * sizeof(int32_t));
  const size_t o_lc = align(o_li + lrec.size() * sizeof(LightRec));
  const size_t o_lv = align(o_lc + lb.cells.size() * sizeof(LbCell));
  const size_t o_ld = align(o_lv + (lb.ov.size() + 1) * sizeof(uint16_t));
  const size_t o_ll = align(o_ld + lb.delta.size() * sizeof(float));
  const size_t o_gr = align(o_ll + lb.limit.size() * sizeof(float));
  const size_t o_tr = align(o_gr + grec.size() * sizeof(GroupRec));
  const size_t o_ts = align(o_tr + (tris.size() + 1) * sizeof(TriRec));
  const size_t o_tb = align(o_ts + (tri_shade.size() + 1) * sizeof(TriShade));
  const size_t o_tl = align(o_tb + (tbvh.size() + 1) * sizeof(BvhNode));
  const size_t o_tx = align(o_tl + (trec.size() + 1) * sizeof(TriRec));
  const size_t o_cu = align(o_tx + (fx_tris.size() + 1) * sizeof(TriRec));
  const size_t o_co = align(o_cu + (csg_units.size() + 1) * sizeof(CsgUnit));
  const size_t o_cn = align(o_co + (csg_ops.size() + 1) * sizeof(CsgOp));
  const size_t o_cl = align(o_cn + (csg_nodes.size() + 1) * sizeof(CsgRec));
  const size_t o_ub = align(o_cl + (csg_leaves.size() + 1) * sizeof(OtherRec));
  const size_t o_ur = align(o_ub + (ubvh.size() + 1) * sizeof(BvhNode));
  const size_t o_ux = align(o_ur + (urec.size() + 1) * sizeof(CsgUnit));
  const size_t o_ar = align(o_ux + (fx_units.size() + 1) * sizeof(CsgUnit));
  const size_t o_ac = align(o_ar + (alias_rec.size() + 1) * sizeof(OtherRec));
  const size_t o_ao = align(o_ac + (alias_tab.size() + 1) * sizeof(AliasClass));
  const size_t o_ct = align(o_ao + (alias_of.size() + 1) * sizeof(int32_t));
  if (!deep_plan[0]) csg_counts.clear();  // (only a deep unit's gates read them)
  const size_t o_dc = align(o_ct + (csg_tris.size() + 1) * sizeof(TriRec));
  // (the run hierarchies: a scene without one allocates nothing for them)
  const size_t o_rr = align(o_dc + (csg_counts.size() + 1) * sizeof(uint32_t));
  const size_t o_rn = csg_runs.empty() ? o_rr : align(o_rr + (csg_runs.size() + 1) * sizeof(CsgRun));
  const size_t total = (csg_runs.empty() ? o_rr : align(o_rn + (csg_run_nodes.size() + 1) * sizeof(BvhNode))) + 256;
  std::vector<unsigned char> host(total, 0);
  if (!diag.empty()) std::memcpy(&host[o_diag], diag.data(), diag.size() * sizeof(SphereDiag));
  if (!gen.empty()) std::memcpy(&host[o_gen], gen.data(), gen.size() * sizeof(SphereGen));
  if (!planes.empty()) std::memcpy(&host[o_pl], planes.data(), planes.size() * sizeof(PlaneRec));
  if (!quads.empty()) std::memcpy(&host[o_qd], quads.data(), quads.size() * sizeof(QuadRec));
  if (!bvh.empty()) std::memcpy(&host[o_bv], bvh.data(), bvh.size() * sizeof(BvhNode));
  if (!bvh_pair.empty()) std::memcpy(&host[o_bp], bvh_pair.data(), bvh_pair.size() * sizeof(BvhPair));
  if (!bvh_wide.empty()) std::memcpy(&host[o_bw], bvh_wide.data(), bvh_wide.size() * sizeof(BvhWide));
  if (!bvh_wide16.empty()) std::memcpy(&host[o_bh], bvh_wide16.data(), bvh_wide16.size() * sizeof(BvhWide16));
  if (!obvh.empty()) std::memcpy(&host[o_ob], obvh.data(), obvh.size() * sizeof(BvhNode));
  if (!orec.empty()) std::memcpy(&host[o_or], orec.data(), orec.size() * sizeof(OtherRec));
  if (!lbvh.empty()) std::memcpy(&host[o_lb], lbvh.data(), lbvh.size() * sizeof(BvhNode));
  if (!lclus.empty()) std::memcpy(&host[o_cc], lclus.data(), lclus.size() * sizeof(ConeCluster));
  if (!lcone.empty()) std::memcpy(&host[o_lm], lcone.data(), lcone.size() * sizeof(int32_t));
  if (!lrec_clus.empty()) std::memcpy(&host[o_lk], lrec_clus.data(), lrec_clus.size() * sizeof(int32_t));
  if (!line_rec.empty()) std::memcpy(&host[o_lr], line_rec.data(), line_rec.size() * sizeof(QuadRec));
  if (!fx_gen.empty()) std::memcpy(&host[o_fg], fx_gen.data(), fx_gen.size() * sizeof(SphereGen));
  if (!fx_quads.empty()) std::memcpy(&host[o_fq], fx_quads.data(), fx_quads.size() * sizeof(QuadRec));
  if (!shade.empty()) std::memcpy(&host[o_sh], shade.data(), shade.size() * sizeof(ShadeRec));
  for (size_t i = 0; i < shade.size(); ++i) {
    const double rt2[2] = {shade[i].reflective, shade[i].transparency};
    std::memcpy(&host[o_rt + i * 2 * sizeof(double)], rt2, sizeof rt2);
  }
  {  // each object's SphereDiag record after the hierarchy's reordering (meta = object << 1 | shadow),
     // flagged kOwnOutside when its own shadow test may be left out for a hit from outside
     // (rt_trace.hpp, shadow_trace): the over point then lies EPSILON off the surface in world
     // space, at least EPSILON / r_max in object space, far above every rounding in the sphere
     // test when the semi-axes are at most 1e3 and the extent at most 1e6 (the over point's
     // EPSILON step resolved to 1e-10)
    std::vector<int32_t> obj_diag(shade.size() + 1, -1);
    for (size_t k = 0; k < diag.size(); ++k) {
      const SphereDiag& r = diag[k];
      bool own = true;
      for (int a = 0; a < 3; ++a) {
        const double sa = std::fabs(r.s[a]), ra = 1.0 / sa, ca = std::fabs(r.t[a] / r.s[a]);
        own = own && std::isfinite(ra) && std::isfinite(ca) && ra <= 1e3 && ca + ra <= 1e6;
      }
      obj_diag[(size_t)(r.meta >> 1)] = (int32_t)k | (own ? kOwnOutside : 0);
    }
    std::memcpy(&host[o_od], obj_diag.data(), obj_diag.size() * sizeof(int32_t));
  }
  if (!lrec.empty()) std::memcpy(&host[o_li], lrec.data(), lrec.size() * sizeof(LightRec));
  if (!grec.empty()) std::memcpy(&host[o_gr], grec.data(), grec.size() * sizeof(GroupRec));
  if (!tris.empty()) std::memcpy(&host[o_tr], tris.data(), tris.size() * sizeof(TriRec));
  if (!tri_shade.empty()) std::memcpy(&host[o_ts], tri_shade.data(), tri_shade.size() * sizeof(TriShade));
  if (!tbvh.empty()) std::memcpy(&host[o_tb], tbvh.data(), tbvh.size() * sizeof(BvhNode));
  if (!trec.empty()) std::memcpy(&host[o_tl], trec.data(), trec.size() * sizeof(TriRec));
  if (!fx_tris.empty()) std::memcpy(&host[o_tx], fx_tris.data(), fx_tris.size() * sizeof(TriRec));
  if (!csg_units.empty()) std::memcpy(&host[o_cu], csg_units.data(), csg_units.size() * sizeof(CsgUnit));
  if (!csg_ops.empty()) std::memcpy(&host[o_co], csg_ops.data(), csg_ops.size() * sizeof(CsgOp));
  if (!csg_nodes.empty()) std::memcpy(&host[o_cn], csg_nodes.data(), csg_nodes.size() * sizeof(CsgRec));
  if (!csg_leaves.empty()) std::memcpy(&host[o_cl], csg_leaves.data(), csg_leaves.size() * sizeof(OtherRec));
  if (!csg_tris.empty()) std::memcpy(&host[o_ct], csg_tris.data(), csg_tris.size() * sizeof(TriRec));
  if (!csg_counts.empty()) std::memcpy(&host[o_dc], csg_counts.data(), csg_counts.size() * sizeof(uint32_t));
  if (!csg_runs.empty()) {
    std::memcpy(&host[o_rr], csg_runs.data(), csg_runs.size() * sizeof(CsgRun));
    std::memcpy(&host[o_rn], csg_run_nodes.data(), csg_run_nodes.size() * sizeof(BvhNode));
  }
  if (!ubvh.empty()) std::memcpy(&host[o_ub], ubvh.data(), ubvh.size() * sizeof(BvhNode));
  if (!urec.empty()) std::memcpy(&host[o_ur], urec.data(), urec.size() * sizeof(CsgUnit));
  if (!fx_units.empty()) std::memcpy(&host[o_ux], fx_units.data(), fx_units.size() * sizeof(CsgUnit));
  if (!alias_rec.empty()) std::memcpy(&host[o_ar], alias_rec.data(), alias_rec.size() * sizeof(OtherRec));
  if (!alias_tab.empty()) std::memcpy(&host[o_ac], alias_tab.data(), alias_tab.size() * sizeof(AliasClass));
  if (!alias_of.empty()) std::memcpy(&host[o_ao], alias_of.data(), alias_of.size() * sizeof(int32_t));
  if (!lb.cells.empty()) {
    std::memcpy(&host[o_lc], lb.cells.data(), lb.cells.size() * sizeof(LbCell));
    if (!lb.ov.empty()) std::memcpy(&host[o_lv], lb.ov.data(), lb.ov.size() * sizeof(uint16_t));
    std::memcpy(&host[o_ld], lb.delta.data(), lb.delta.size() * sizeof(float));
    std::memcpy(&host[o_ll], lb.limit.data(), lb.limit.size() * sizeof(float));
  }

  rt_scene* s = new rt_scene();
  s->device = device;
  // children per ray at most (WfSizing::branch): the exact bound of the arenas
  int branch = 0;
  for (size_t i = 0; i < n_shapes; ++i)
    branch = std::max(branch, (shapes[i].reflective != 0.0 ? 1 : 0) + (shapes[i].transparency != 0.0 ? 1 : 0));
  s->sizing.branch = branch;
  s->band_sizing.branch = branch;
  {
    std::lock_guard<std::mutex> tlk(g_tune_mu);
    s->tune = g_tune_defaults;
  }
  auto cleanup = [&](int rc) {
    rt_scene_destroy(s);
    return rc;
  };
  int rc;
  DeviceGuard restore;  // the caller's device, whatever happens below
  if ((rc = [&]() -> int {
         RT_HIP(hipSetDevice(device));
         RT_HIP(hipMalloc(&s->d_blob, total));
         RT_HIP(hipMemcpy(s->d_blob, host.data(), total, hipMemcpyHostToDevice));
         RT_HIP(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
         return RT_OK;
       }()) != RT_OK)
    return cleanup(rc);
  unsigned char* b = (unsigned char*)s->d_blob;
  s->dev.sph_diag = (const SphereDiag*)(b + o_diag);
  s->dev.sph_gen = (const SphereGen*)(b + o_gen);
  s->dev.planes = (const PlaneRec*)(b + o_pl);
  s->dev.quads = (const QuadRec*)(b + o_qd);
  s->dev.bvh = bvh.empty() ? nullptr : (const BvhNode*)(b + o_bv);
  s->dev.bvh_pair = bvh_pair.empty() ? nullptr : (const BvhPair*)(b + o_bp);
  s->dev.bvhw = bvh_wide.empty() ? nullptr : (const BvhWide*)(b + o_bw);
  s->dev.bvhw16 = bvh_wide16.empty() ? nullptr : (const BvhWide16*)(b + o_bh);
  s->dev.n_bvhw = (int32_t)bvh_wide.size();
  s->dev.bvhw_stack = wide_stack;
  s->dev.n_bvh = (int32_t)bvh.size();
  s->dev.bvh_depth = bvh_depth;
  s->dev.obvh = obvh.empty() ? nullptr : (const BvhNode*)(b + o_ob);
  s->dev.orec = (const OtherRec*)(b + o_or);
  s->dev.lbvh = lbvh.empty() ? nullptr : (const BvhNode*)(b + o_lb);
  s->dev.lclus = (const ConeCluster*)(b + o_cc);
  s->dev.lcone = (const int32_t*)(b + o_lm);
  s->dev.lrec_clus = (const int32_t*)(b + o_lk);
  s->dev.n_lclus = (int32_t)lclus.size();
  s->dev.lrec = (const QuadRec*)(b + o_lr);
  s->dev.n_lbvh = (int32_t)lbvh.size();
  s->dev.n_lrec = (int32_t)line_rec.size();
  s->dev.n_obvh = (int32_t)obvh.size();
  s->dev.obvh_depth = obvh_depth;
  s->dev.n_orec = (int32_t)orec.size();
  s->dev.fx_gen = (const SphereGen*)(b + o_fg);
  s->dev.fx_quads = (const QuadRec*)(b + o_fq);
  s->dev.n_fx_gen = (int32_t)fx_gen.size();
  s->dev.n_fx_quads = (int32_t)fx_quads.size();
  s->dev.lb_cells = lb.cells.empty() ? nullptr : (const LbCell*)(b + o_lc);
  s->dev.lb_ov = (const uint16_t*)(b + o_lv);
  s->dev.lb_delta = (const float*)(b + o_ld);
  s->dev.lb_limit = (const float*)(b + o_ll);
  s->dev.lb_res = lb.res;
  s->dev.lb_n_items = (int32_t)std::min<size_t>(lb.n_items, 0x7FFFFFFF);
  s->dev.shade = (const ShadeRec*)(b + o_sh);
  s->dev.refl_transp = (const double*)(b + o_rt);
  s->dev.obj_diag = (const int32_t*)(b + o_od);
  s->dev.lights = (const LightRec*)(b + o_li);
  s->dev.groups = (const GroupRec*)(b + o_gr);
  s->dev.n_groups = (int32_t)n_nodes;
  s->dev.tris = (const TriRec*)(b + o_tr);
  s->dev.tri_shade = (const TriShade*)(b + o_ts);
  s->dev.tbvh = tbvh.empty() ? nullptr : (const BvhNode*)(b + o_tb);
  s->dev.trec = (const TriRec*)(b + o_tl);
  s->dev.fx_tris = (const TriRec*)(b + o_tx);
  s->dev.n_tris = (int32_t)tris.size();
  s->dev.n_tbvh = (int32_t)tbvh.size();
  s->dev.n_trec = (int32_t)trec.size();
  s->dev.n_fx_tris = (int32_t)fx_tris.size();
  s->dev.tbvh_depth = tbvh_depth;
  s->dev.csg_units = (const CsgUnit*)(b + o_cu);
  s->dev.csg_ops = (const CsgOp*)(b + o_co);
  s->dev.csg_nodes = (const CsgRec*)(b + o_cn);
  s->dev.csg_leaves = (const OtherRec*)(b + o_cl);
  s->dev.csg_tris = (const TriRec*)(b + o_ct);
  s->dev.csg_counts = csg_counts.empty() ? nullptr : (const uint32_t*)(b + o_dc);
  if (deep_plan[0]) {  // (the state buffer itself is each launch's own: Wavefront, rt_scene::HostCtx)
    s->dev.csg_deep_levels = (int32_t)deep_plan[1];
    s->dev.csg_deep_nw = (int32_t)((deep_plan[2] + 31) / 32);
    s->dev.csg_deep_lw = (int32_t)((deep_plan[3] + 31) / 32);
  }
  for (int k = 0; k < 4; ++k) s->csg_deep_plan[k] = deep_plan[k];
  if (!csg_runs.empty()) {  // (csg_runs itself stays null here: a fast-path render sets it in its own copy)
    s->dev.csg_run_recs = (const CsgRun*)(b + o_rr);
    s->dev.csg_run_nodes = (const BvhNode*)(b + o_rn);
    s->dev.n_csg_runs = (int32_t)csg_runs.size();
  }
  for (int k = 0; k < 4; ++k) s->csg_run_plan[k] = run_plan[k];
  s->dev.n_csg_units = (int32_t)csg_units.size();
  s->dev.n_csg_sph = n_csg_kind[0];
  s->dev.n_csg_planes = n_csg_kind[1];
  s->dev.n_csg_other = n_csg_kind[2];
  s->dev.ubvh = ubvh.empty() ? nullptr : (const BvhNode*)(b + o_ub);
  s->dev.urec = (const CsgUnit*)(b + o_ur);
  s->dev.fx_units = (const CsgUnit*)(b + o_ux);
  s->dev.n_ubvh = (int32_t)ubvh.size();
  s->dev.n_urec = (int32_t)urec.size();
  s->dev.n_fx_units = (int32_t)fx_units.size();
  s->dev.ubvh_depth = ubvh_depth;
  s->dev.alias_rec = (const OtherRec*)(b + o_ar);
  s->dev.alias_cls = (const AliasClass*)(b + o_ac);
  s->dev.alias_of = alias_of.empty() ? nullptr : (const int32_t*)(b + o_ao);
  s->dev.n_alias_rec = (int32_t)alias_rec.size();
  s->dev.n_alias_cls = (int32_t)alias_tab.size();
  s->dev.n_alias_sph = n_alias_kind[0];
  s->dev.n_alias_planes = n_alias_kind[1];
  s->dev.n_alias_other = n_alias_kind[2];
  s->dev.n_diag = (int32_t)diag.size();
  s->dev.n_gen = (int32_t)gen.size();
  s->dev.n_planes = (int32_t)planes.size();
  s->dev.n_quads = (int32_t)quads.size();
  s->dev.n_objects = (int32_t)n_shapes;
  s->dev.n_lights = (int32_t)n_lights;
  s->n_objects = (int)n_shapes;
  s->n_lights = (int)n_lights;
  *out = s;
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_scene_create(const rt_shape_desc* shapes, size_t n_shapes, const rt_light_desc* lights,
                    size_t n_lights, int device, rt_scene** out) {
  return guarded([&]() -> int {
  return rt_scene_create_groups(shapes, n_shapes, nullptr, nullptr, 0, lights, n_lights, device, out);
  });
}

int rt_scene_create_groups(const rt_shape_desc* shapes, size_t n_shapes, const int32_t* shape_group,
                           const rt_group_desc* groups, size_t n_groups, const rt_light_desc* lights,
                           size_t n_lights, int device, rt_scene** out) {
  return rt_scene_create_mesh(shapes, n_shapes, shape_group, groups, n_groups, nullptr, 0, lights, n_lights, device, out);
}

// rt_scene_create_groups / _mesh: the tree whose nodes are all Groups.
int rt_scene_create_mesh(const rt_shape_desc* shapes, size_t n_shapes, const int32_t* shape_group,
                         const rt_group_desc* groups, size_t n_groups, const rt_triangle_desc* tri_descs, size_t n_tris,
                         const rt_light_desc* lights, size_t n_lights, int device, rt_scene** out) {
  return guarded([&]() -> int {
  if (!out || (n_shapes && !shapes) || (n_lights && !lights) || (n_groups && (!groups || !shape_group)) ||
      (n_tris && !tri_descs))
    return fail(RT_ERR_INVALID_ARGUMENT, "null pointer");
  *out = nullptr;
  if (n_groups > (size_t)(1u << 24)) return fail(RT_ERR_INVALID_ARGUMENT, "too many groups");
  for (size_t g = 0; g < n_groups; ++g)
    if (groups[g].parent < -1 || groups[g].parent >= (int32_t)g)
      return fail(RT_ERR_INVALID_ARGUMENT, "group " + std::to_string(g) + ": its parent must be -1 or an earlier group");
  for (size_t i = 0; n_groups && i < n_shapes; ++i)
    if (shape_group[i] < -1 || (int64_t)shape_group[i] >= (int64_t)n_groups)
      return fail(RT_ERR_INVALID_ARGUMENT, "shape " + std::to_string(i) + ": bad group index");
  std::vector<rt_node_desc> nodes(n_groups);
  for (size_t g = 0; g < n_groups; ++g) {
    nodes[g] = rt_node_desc{};
    nodes[g].kind = RT_NODE_GROUP;
    nodes[g].parent = groups[g].parent;
    for (int c = 0; c < 3; ++c) { nodes[g].min[c] = groups[g].min[c]; nodes[g].max[c] = groups[g].max[c]; }
  }
  return rt_scene_create_tree(shapes, n_shapes, shape_group, nullptr, nodes.data(), n_groups, tri_descs, n_tris, lights,
                              n_lights, device, out);
  });
}

int rt_scene_create_tree(const rt_shape_desc* shapes, size_t n_shapes, const int32_t* shape_node,
                         const int32_t* shape_side, const rt_node_desc* nodes, size_t n_nodes,
                         const rt_triangle_desc* tri_descs, size_t n_tris, const rt_light_desc* lights, size_t n_lights,
                         int device, rt_scene** out) {
  return guarded([&]() -> int {
    return create_tree(shapes, n_shapes, shape_node, shape_side, nodes, n_nodes, tri_descs, n_tris, lights, n_lights,
                       false, nullptr, 0, false, device, out);
  });
}

int rt_scene_create_aliased(const rt_shape_desc* shapes, size_t n_shapes, const int32_t* shape_node,
                            const int32_t* shape_side, const rt_node_desc* nodes, size_t n_nodes,
                            const rt_triangle_desc* tri_descs, size_t n_tris, const rt_light_desc* lights,
                            size_t n_lights, const int32_t* equal_pairs, size_t n_pairs, int device, rt_scene** out) {
  return guarded([&]() -> int {
    if (n_pairs && !equal_pairs) return fail(RT_ERR_INVALID_ARGUMENT, "null pointer");
    return create_tree(shapes, n_shapes, shape_node, shape_side, nodes, n_nodes, tri_descs, n_tris, lights, n_lights,
                       true, equal_pairs, n_pairs, false, device, out);
  });
}

int rt_scene_create_ex(const rt_shape_desc* shapes, size_t n_shapes, const int32_t* shape_node, const int32_t* shape_side,
                       const rt_node_desc* nodes, size_t n_nodes, const rt_triangle_desc* tri_descs, size_t n_tris,
                       const rt_light_desc* lights, size_t n_lights, const int32_t* equal_pairs, size_t n_pairs,
                       uint32_t flags, int device, rt_scene** out) {
  return guarded([&]() -> int {
    if (flags & ~(uint32_t)(RT_SCENE_ALIASED | RT_SCENE_DEEP_CSG))
      return fail(RT_ERR_INVALID_ARGUMENT, "unknown flag (RT_SCENE_ALIASED, RT_SCENE_DEEP_CSG)");
    const bool aliased = (flags & RT_SCENE_ALIASED) != 0;
    if (!aliased && (equal_pairs || n_pairs))
      return fail(RT_ERR_INVALID_ARGUMENT, "equal pairs without RT_SCENE_ALIASED");
    if (n_pairs && !equal_pairs) return fail(RT_ERR_INVALID_ARGUMENT, "null pointer");
    return create_tree(shapes, n_shapes, shape_node, shape_side, nodes, n_nodes, tri_descs, n_tris, lights, n_lights,
                       aliased, equal_pairs, n_pairs, (flags & RT_SCENE_DEEP_CSG) != 0, device, out);
  });
}

int rt_shapes_equal_pairs(const rt_shape_desc* shapes, size_t n_shapes, int32_t* out_pairs, size_t cap,
                          size_t* n_pairs) {
  return guarded([&]() -> int {
    if (!n_pairs || (n_shapes && !shapes) || (cap && !out_pairs)) return fail(RT_ERR_INVALID_ARGUMENT, "null pointer");
    if (n_shapes > (size_t)(1u << 29)) return fail(RT_ERR_INVALID_ARGUMENT, "too many shapes");
    const std::vector<std::pair<int32_t, int32_t>> pairs = rtalias::equal_pairs(shapes, n_shapes);
    *n_pairs = pairs.size();
    for (size_t p = 0; p < pairs.size() && p < cap; ++p) {
      out_pairs[2 * p] = pairs[p].first;
      out_pairs[2 * p + 1] = pairs[p].second;
    }
    if (pairs.size() > cap)
      return fail(RT_ERR_BUFFER_TOO_SMALL, "the shapes hold " + std::to_string(pairs.size()) + " equal pairs");
    return RT_OK;
  });
}

void rt_scene_destroy(rt_scene* s) {
  if (!s) return;
  DeviceGuard restore(s->device);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  s->multi.release();
  (void)hipSetDevice(s->device);
  if (s->d_blob) (void)hipFree(s->d_blob);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  delete s;  // the host contexts and workspaces release their memory (on the scene's device)
}

}  // extern "C"
