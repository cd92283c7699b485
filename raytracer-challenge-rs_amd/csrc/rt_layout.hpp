// rt_layout.hpp — device-resident layout of a flattened `World` (world.rs:18-21)
// shared by the host uploader (rt_api.cpp) and the HIP kernels.
//
// HBM layout (all 64-B aligned, all read-only during a render):
//   trace records  : the per-ray hot loop reads EVERY record of its class once
//                    per ray, wave-uniformly (s_load -> SGPR operands):
//       SphereDiag  8 doubles  (64 B)  inverse = diag(s) + translation t
//       SphereGen  16 doubles (128 B)  inverse rows 0-2 (general affine)
//       PlaneRec    8 doubles  (64 B)  inverse row 1 (only y matters)
//       QuadRec    16 doubles (128 B)  Cube / Cylinder / Cone: inverse rows 0-2,
//                                      minimum, maximum, kind, closed
//       TriRec     24 doubles (192 B)  Triangle / SmoothTriangle: inverse rows
//                                      0-2, p1, e1, e2
//     each carries `meta` = (object index << 1) | casts_shadow.
//   shade records  : ShadeRec per object index (AoS, 64 doubles = 512 B),
//                    gathered per lane only at a hit.
//   lights         : 6 doubles each (position, intensity), wave-uniform.
#pragma once
#include <stdint.h>
#include <cmath>

namespace rtamd {

constexpr double kEpsilon = 0.00001;  // raytracer/src/lib.rs:18

struct alignas(64) SphereDiag {  // translation . axis scaling (e.g. all C3/C5 spheres)
  double s[3];                   // inverse diagonal m00, m11, m22
  double t[3];                   // inverse translation m03, m13, m23
  int64_t meta;
  int64_t pad;
};
// `gate`: 0, or 1 + the innermost Group the shape belongs to (GroupRec): the
// shape is tested only by rays that meet the bounding box of that group and of
// every group enclosing it (Group::intersect, group.rs:49-58; group_gate).
// Shapes inside groups are always one of these three records.
struct alignas(64) SphereGen {  // any invertible affine transform
  double m[12];                 // inverse rows 0..2
  int64_t meta;
  int32_t gate, pad0;
  int64_t pad[2];
};
struct alignas(64) PlaneRec {
  double m[4];  // inverse row 1: m10 m11 m12 m13
  int64_t meta;
  int32_t gate, pad0;
  int64_t pad[2];
};
struct alignas(64) QuadRec {  // cube.rs / cylinder.rs / cone.rs
  double m[12];  // inverse rows 0..2
  double minimum, maximum;
  int32_t kind, closed;
  int32_t meta, gate;
};
// A Group's bounding box as the reference's Group::intersect tests it
// (BaseShape::bounding_box of the group, bounding_box.rs:95-136), and 1 + the
// group enclosing it (0: a top-level group of World::objects).
struct alignas(64) GroupRec {
  double lo[3], hi[3];
  int32_t parent, pad0;
  int64_t pad;
};
// Triangle / SmoothTriangle (triangle.rs, smooth_triangle.rs): inverse rows
// 0..2 (a triangle of a transformed group has its group's transform), p1 and
// the edges e1 = p2 - p1, e2 = p3 - p1 as the constructors derive them.
// `kind` = RT_SHAPE_TRIANGLE / RT_SHAPE_SMOOTH_TRIANGLE; `tri` = its TriShade.
struct alignas(64) TriRec {
  double m[12];
  double p1[3], e1[3], e2[3];
  int32_t meta, gate;
  int32_t kind, tri;
  int64_t pad;
};
static_assert(sizeof(TriRec) == 192, "TriRec must stay 192 B");
// The rays the triangle hierarchy's padding is sized for (rt_bvh.cpp tri_box,
// rt_trace.hpp tri_trace): |d|_inf and |o|_inf at most these.
constexpr double kTriDirMax = 2.0, kTriOriginMax = 16384.0;
// What a hit on a triangle reads besides its ShadeRec (ShadeRec::pad0 = 1 + its
// index here, 0 for every other kind): the flat normal, the vertex normals of
// the smooth kind, and p1 / e1 / e2 again, from which prepare() recomputes the
// hit's u and v (tri_local_intersect's operations on the same operands).
// `csg`: 1 + the innermost CsgRec above a triangle under a Csg (0: none): there the
// reference's u and v are those of the ray chained down the Csgs (csg_tri_local_normal).
struct alignas(64) TriShade {
  double normal[3];
  double n1[3], n2[3], n3[3];
  double p1[3], e1[3], e2[3];
  int32_t csg, pad0;
  double pad[2];
};
static_assert(sizeof(TriShade) == 192, "TriShade must stay 192 B");
static_assert(sizeof(GroupRec) == 64, "GroupRec must stay 64 B");

// ---- Csg (geometry/shape/csg.rs). A CSG with no CSG above it is one UNIT: per
// ray its whole tree is evaluated at once (rt_device.hpp csg_units) by a small
// program, the unit's nodes and leaves in the reference's depth-first order
// (a CSG's left before its right). The leaves under a unit live only here.
//   kCsgEnter  arg = the CsgRec: transform the ray by the CSG's own inverse
//              (Shape::intersect, geometry/mod.rs:46-49), gate on its box with
//              that local ray (csg.rs:115-118); a miss jumps to `skip_to`
//   kCsgExit   arg = the CsgRec: sort left ++ right, filter (csg.rs:120-125),
//              back to the enclosing ray
//   kCsgGroup  arg = the GroupRec: Group::intersect's gate (group.rs:49-58) with
//              the ray it is handed; a miss jumps to `skip_to`
//   kCsgLeaf   arg = the leaf (an OtherRec: kind 0 sphere, 1 plane, 2-4 solids;
//              its `gate` holds the leaf's number among these leaves of its unit)
//   kCsgTri    arg = the leaf (a TriRec of DevScene::csg_tris: a Triangle or
//              SmoothTriangle under a Csg): one root at list position 0
// `counts`: the leaves below the node by counter class, sphere | plane << 5 |
// other << 10 (a failed gate owes the reference's count of them, GateSkips):
// at most kCsgMaxLeaves spheres and planes, the triangles of a mesh among the others.
enum { kCsgEnter = 0, kCsgExit = 1, kCsgGroup = 2, kCsgLeaf = 3, kCsgTri = 4 };
constexpr int32_t kCsgCountOtherMax = (1 << 22) - 1;
inline int32_t csg_pack_counts(const int32_t* c) { return (int32_t)((uint32_t)c[0] | (uint32_t)c[1] << 5 | (uint32_t)c[2] << 10); }
struct alignas(16) CsgOp {
  int32_t code, arg, skip_to, counts;
};
// One Csg node: transform_inverse rows 0..2, get_bounds() as local_intersect
// tests it, the operation (csg.rs:14-19) and `split`, the first object index of
// its right child: an intersection's object is in `left` (Shape::includes,
// geometry/mod.rs:87-89, group.rs:104-106, csg.rs:132-134) iff its index is below.
// A unit's nodes are consecutive, the unit's own first; `self` is the node's number
// among them and `parent` the number of the Csg above it (-1: the unit's own node).
struct alignas(64) CsgRec {
  double m[12];
  double lo[3], hi[3];
  int32_t op, split;
  int32_t parent, self;
  int64_t pad[4];
};
static_assert(sizeof(CsgRec) == 192, "CsgRec must stay 192 B");
// One unit: its program ops[first .. first + n), the gate of the groups around it
// (as a record's `gate`), and its leaves by counter class (as CsgOp::counts).
// `n` | kCsgWide: a WIDE unit (one with a triangle leaf, or every unit under the
// development knob csg_wide_all): the streamed evaluator (csg_wide_eval), never the
// units' hierarchy.
constexpr int32_t kCsgWide = 1 << 30;
// `n` | kCsgDeep: a DEEP unit (rt_scene_create_ex with RT_SCENE_DEEP_CSG: one beyond a cap of the
// other two kinds, or every unit under the development knob csg_deep_all): csg_deep_eval, whose
// per-lane state scales with the unit and lives in the launch's own buffer (DevScene::
// csg_deep_state), never the units' hierarchy. Its gates read their sphere and plane counts from
// DevScene::csg_counts (two words per op of the program: the packed fields hold 31 of each, and
// are zero in a deep unit's ops and unit record); a leaf of kinds 0-4 has its number among the
// unit's such leaves in OtherRec::gate, as a wide unit's.
constexpr int32_t kCsgDeep = 1 << 29;
constexpr int32_t kCsgKindMask = kCsgWide | kCsgDeep;
// What a deep unit's batch tag holds (rt_csg.hpp kCsgDeepTag*): include/rt_render.h's
// RT_CSG_DEEP_MAX_NODES Csg nodes and RT_CSG_DEEP_MAX_LEAVES leaves of kinds 0-4 in one unit.
constexpr int32_t kCsgDeepMaxNodes = 1 << 15, kCsgDeepMaxLeaves = 1 << 16;
struct alignas(16) CsgUnit {
  int32_t first, n, gate, counts;
};
// A RUN: a maximal sequence of consecutive kCsgTri ops of a wide or deep unit's program. All its
// ops sit between the same Enter / Group gates, so the evaluators hand every one of them the same
// chained ray. A run of at least csg_run_min boxed triangles has a hierarchy over them (DESIGN.md
// §5.2 "Csg units: run hierarchies"; rt_slab.hpp csg_run_walk): its records are csg_tris[first ..
// first + n), the boxed ones first and in leaf order, then the remainder (those tri_box refuses),
// which every ray tests; its nodes csg_run_nodes[node .. node + n_nodes), child indices and leaf
// codes (first << 7 | cnt) relative to the run. The boxes are in the space of the chained ray and
// padded for chained rays with |d|_inf <= dmax from |o|_inf <= omax (derived from the CsgRec::m
// chain above the run); any other chained ray takes the run's ops one by one. The run's first op
// carries skip_to = the pc past the run and counts = 1 + the run's index (both zero in every
// other kCsgTri op; csg_unit_eval's gates-only walk reads neither).
struct alignas(64) CsgRun {
  double dmax, omax;
  int32_t first, n, n_boxed;
  int32_t node, n_nodes, depth;
  int64_t pad[3];
};
static_assert(sizeof(CsgRun) == 64, "CsgRun must stay 64 B");
// The deep state of one lane, in 32-bit words (word i of lane l at i * lanes + l, so a wave's
// accesses coalesce): the filter bits inl and inr, one bit each per Csg node of the unit (nw words
// each), the parity bits of the leaves of kinds 0-4 (lw words), and per open level of the ray
// chain the ray its Enter found (12 words: origin and direction).
constexpr int32_t csg_deep_words(int32_t nodes, int32_t leaves, int32_t levels) {
  return 2 * ((nodes + 31) / 32) + (leaves + 31) / 32 + 12 * levels;
}
static_assert(sizeof(QuadRec) == 128, "QuadRec must stay 128 B");
// ---- Alias classes (rt_scene_create_aliased): shapes the caller's structural `==` holds
// between, every two of a class (exact and near duplicates). In the `containers` walk of
// prepare_computations (intersection.rs:63-90) a class is ONE entry: `contains` and `position`
// find whichever member is there. Its members (kinds 0-4, top level or inside groups) live only
// in DevScene::alias_rec, general records with their group gate as the leaves under a Csg are
// (kind 0 sphere, 1 plane, 2-4 solids), grouped by class: records [first, first + n). They keep
// their object index (`meta`), so the closest hit, shading, shadows and the tie order are theirs.
struct alignas(8) AliasClass {
  int32_t first, n;
};
// The rays the unit hierarchy's padding is sized for (rt_bvh.cpp csg_unit_box, rt_trace.hpp
// unit_trace): finite, |d|_inf at least kUnitDirMin (a unit vector's is 0.577), from origins
// with |o|_inf at most kUnitOriginMax (a cube leaf's box grows with it: EPSILON times the
// longest t such a ray can reach the cube with).
constexpr double kUnitDirMin = 0.5, kUnitOriginMax = 4096.0;
// The same for the hierarchy over the other bounded records (rt_bvh.cpp other_box, rt_trace.hpp
// other_trace), whose cubes are widened by the same rule: e = EPSILON (kOtherOriginMax + |box|_inf)
// / kOtherDirMin of the unit cube, every cube of every scene. Here the origin bound is 1024 (2 %,
// against 8 % at the units' 4096), and a ray from farther off is not sent round every record (a
// floor's horizon rows start their shadow and reflection rays there: two pixel rows of such
// lanes, 800 tests each, nearly doubled the frame time of a divided group of 800,
// profiles/other_box_ab.txt): it walks the hierarchy with every box grown by other_far_pad, which
// is what a cube's root can add to its box from that origin. Rays that are not finite or have
// |d|_inf < kOtherDirMin (only a caller's own) test every record.
constexpr double kOtherDirMin = 0.5, kOtherOriginMax = 1024.0;
// World-space growth per axis for a ray from |o|_inf = o_inf > kOtherOriginMax: a cube's root
// leaves its slab by |t| EPSILON in object space, h |t| EPSILON on a world axis where the cube's
// half extent is h <= m_axis (the hierarchy's largest coordinate on that axis, root_bound), and
// |t| <= (o_inf + |p|_inf) / kOtherDirMin with |p|_inf <= m_max + the growth itself:
// D = m_max EPSILON (o_inf + m_max) / dmin / (1 - m_max EPSILON / dmin) bounds every axis' growth,
// so m_axis EPSILON (o_inf + m_max + D) / dmin bounds this one's. Negative: no bound (the caller
// tests every record).
constexpr double other_far_pad(double m_axis, double m_max, double o_inf) {
  const double q = m_max * kEpsilon / kOtherDirMin;
  if (!(q < 0.5) || !(o_inf < 1e300)) return -1.0;
  const double D = m_max * kEpsilon * (o_inf + m_max) / kOtherDirMin / (1.0 - q);
  return m_axis * kEpsilon * (o_inf + m_max + D) / kOtherDirMin * (1.0 + 1e-9);
}

// Bounding-volume hierarchies (built on the host, rt_bvh.cpp): one over the
// SphereDiag records, one over the other bounded records (OtherRec: general-
// transform spheres, cubes, bounded cylinders). Binary nodes carry both
// children's boxes, so one 64-B load (one s_load_dwordx16 for a wave, four
// 16-B loads for a lane) decides both children. Boxes are binary32 rounded
// OUTWARD from the padded binary64 boxes, so culling stays conservative
// (DESIGN.md "Exact culling"). A child is an internal node index (>= 0), a
// leaf code -(1 + (first << 7 | count)) over the (reordered) record array,
// or kBvhEmpty. `line` (the other records' hierarchy only, else 0): bit c set
// when a record below child c must be culled over the ray's whole line
// (rt_bvh.cpp other_box: the closed cylinders).
struct alignas(64) BvhNode {
  float lo[2][3], hi[2][3];
  int32_t child[2];
  int32_t axis;
  uint32_t line;
};
static_assert(sizeof(BvhNode) == 64, "BvhNode must stay 64 B");
// The same node in the pair layout the per-lane traversal reads
// (lane_trace_pair): per axis a, b[4a..4a+3] = lo[0][a], lo[1][a], hi[0][a],
// hi[1][a], so the two children's entry (or exit) planes on an axis are one
// 8-B pair, chosen by the sign of the ray's direction. Its child codes are
// 16-bit, so the traversal's LDS stack is too: a node index below 0x8000, a
// leaf 0x8000 | first << 3 | (count - 1) (first < 4095, count <= 8), 0xFFFF
// empty. A hierarchy that does not fit these codes has no pair image.
struct alignas(64) BvhPair {
  float b[12];
  int32_t child[2];
  int32_t axis;
  uint32_t pad;
};
static_assert(sizeof(BvhPair) == 64, "BvhPair must stay 64 B");
// The same hierarchy collapsed to four children per node (lane_trace_wide,
// LANE 15: the whole image in LDS): one 128-B node. Slot j's box is lo[a][j],
// hi[a][j] (one 16-B load per plane block and axis), child[j] a 16-bit code: a
// node index (< 0x8000), 0x8000 | the index of one sphere record (every leaf
// holds one record), or 0xFFFF (empty; its box is inverted, lo = +inf and hi =
// -inf, so no ray with a usable axis meets it). The boxes are the binary
// nodes' own (a collapsed node's children are its binary descendants) or,
// below a binary leaf of several records, each record's own padded box (and
// unions of them) rounded outward to binary32: every box holds what lies below
// it, so every culling decision stays exact (DESIGN.md "Exact culling").
struct alignas(128) BvhWide {
  float lo[3][4];
  float hi[3][4];
  uint16_t child[4];
  uint32_t pad[6];
};
static_assert(sizeof(BvhWide) == 128, "BvhWide must stay 128 B");
// The four-wide image read from global memory (LANE 4, with a treelet of its
// top nodes in LDS): the same nodes in 64 B, the planes rounded outward again,
// to binary16 (a coordinate past binary16's range becomes an infinite plane),
// so each box still holds what lies below it. A visit reads 56 B instead of
// 104, twice the nodes fit a cache line and the treelet, and v_fma_mix_f32
// converts each half exactly inside the slab test's FMA. The culling loses
// little: the area-weighted visit cost of C3's and C5's hierarchies grows by
// 0.3 % and 0.5 %, the record tests by 1.1 % and 2.6 % (tools/wide_sah.cpp).
// (The LDS image stays binary32: there the mixed FMAs cost more issue time
// than the halved LDS reads save, C3 closest class +3 %; from global memory
// C5 runs 4 % faster)
struct alignas(64) BvhWide16 {
  uint16_t lo[3][4];  // binary16 bit patterns
  uint16_t hi[3][4];
  uint16_t child[4];
  uint32_t pad[2];
};
static_assert(sizeof(BvhWide16) == 64, "BvhWide16 must stay 64 B");
// binary16 bits -> value (host checks and tools; the device converts in the FMA)
inline float wide_f16(uint16_t b) {
  const int e = (b >> 10) & 31, m = b & 1023;
  const float v = e == 31 ? (m ? NAN : INFINITY)
                          : e == 0 ? std::ldexp((float)m, -24) : std::ldexp((float)(1024 + m), e - 25);
  return (b & 0x8000u) ? -v : v;
}
constexpr unsigned kWideEmpty = 0xFFFFu, kWideLeaf = 0x8000u;  // BvhWide child codes: empty, leaf flag
// Line hierarchy (rt_bvh.cpp build_line_bvh, line_trace): open tubes
// (cylinder.rs with closed = false) and cones (cone.rs) with finite bounds.
// Their boxes are tested over the ray's whole line up to the current hit,
// (-inf, t_hi]: a culled record then has no root at t <= t_hi at all, so it
// neither hits nor enters `containers` (an open tube is no closed solid, so
// the [0, t_hi] argument of the other hierarchies does not cover its t < 0
// roots). A cone's a ~ 0 branch (cone.rs:102-110) pushes t = -c / 2.0 * b,
// a root anywhere on the line; every other root of a cone lies in its box. So
// the cones whose a, as the reference computes it, is below EPSILON for a ray
// are found before the traversal, cluster by cluster (cone_prepass), tested
// there, and skipped by the traversal. A cluster holds the cones whose
// direction quadratic is the same (cones equal up to position and a turn
// about their axis): with the world direction d, |d|_inf = dm and g = d^T Q d
// (Q: the six distinct entries of the symmetric 3x3 form, xx yy zz xy xz yz),
// every member i has |fl(a_i) - g| <= r dm^2 (r covers every rounding, host
// and device), so |g| - r dm^2 >= EPSILON (with a margin) rules out the whole
// cluster with one test. Members: lcone[first .. first + count) (indices
// into lrec).
struct alignas(64) ConeCluster {
  double q[6];
  double r;
  int32_t first, count;
};
static_assert(sizeof(ConeCluster) == 64, "ConeCluster must stay 64 B");

// A culled record other than a diagonal sphere: the QuadRec layout, with
// kind 0 = sphere under a general inverse (rows 0-2 in m).
typedef QuadRec OtherRec;
constexpr int32_t kBvhEmpty = (int32_t)0x80000000;
constexpr int kBvhLeafMax = 127;
constexpr int kBvhMaxDepth = 60;  // traversal stack entries per wave
constexpr int kLaneLdsDepth = 16;  // per-lane traversal: LDS stack when bvh_depth fits

// Light buffer (Haines & Greenberg 1986, made exact): per point light, a
// cube map of directions around the light (6 faces x R x R cells). Cell c of
// light l lists every shadow-casting SphereDiag record whose padded box may
// hold a point whose direction from the light falls in the cell (rt_bvh.cpp
// build_light_buffer: a conservative projection with margins far above the
// query's rounding), ordered by lb_delta[l * n_diag + idx], a binary32 lower
// bound on the distance from the light to the record's box. A shadow ray from
// o is blocked only by a sphere with a root point q on the segment
// [o, light), and every such q lies in that sphere's box in the cell of
// direction o - light (DESIGN.md "Light buffer"), so testing that cell's
// list up to delta > |light - o| answers is_shadowed exactly. Records whose
// box comes near the light are listed in every cell. The answer is valid
// while |light - o| <= lb_limit[l]; farther origins take the exhaustive loop.
//
// One 16-B record per cell holds the list's first kLbInline 16-bit indices,
// so a ray makes one dependent global load for its cell; longer lists
// continue in lb_ov[ov ..].
constexpr int kLbMaxLights = 16;
constexpr int kLbInline = 5;
struct alignas(16) LbCell {
  uint32_t w0;  // count (low 16) | idx0 (high 16)
  uint32_t w1;  // idx1 | idx2 << 16
  uint32_t w2;  // idx3 | idx4 << 16
  uint32_t ov;  // entries kLbInline.. at lb_ov[ov ..]
};
static_assert(sizeof(LbCell) == 16, "LbCell must stay 16 B");

// Intersection ordering key: (object index << 2) | position in the object's
// local_intersect list (at most 4 entries, cylinder/cone). Equal t resolve by
// this key exactly like the reference's stable sort (intersection.rs:108-116).
constexpr int kKeyShift = 2;

// What a hit on an unpatterned object reads (the inverses, the material, kind
// and pattern kind) fills the first two 128-B lines; patterns, the cylinder /
// cone bounds and the host-only shadow flag come after.
struct alignas(64) ShadeRec {
  double inv[12];   // transform_inverse rows 0..2
  double invT[9];   // transform_inverse_transpose upper 3x3 (= inv^T)
  double color[3];
  double ambient, diffuse, specular, shininess;
  double reflective, transparency, refractive_index;
  int32_t kind, pattern_kind;
  double pat_a[3], pat_b[3];
  double pat_inv[12];
  int32_t shadow, pad0;
  double minimum, maximum;  // Cylinder / Cone (local_normal_at)
  double pad1[11];
};
static_assert(__builtin_offsetof(ShadeRec, pattern_kind) < 256, "hot shading fields in the first two lines");
static_assert(sizeof(ShadeRec) == 512, "ShadeRec must stay 512 B");

struct LightRec {
  double pos[3];
  double intensity[3];
};

// Kernel-argument view of a scene (passed by value; pointers live in SGPRs).
struct DevScene {
  const SphereDiag* sph_diag;
  const SphereGen* sph_gen;
  const PlaneRec* planes;
  const ShadeRec* shade;
  const LightRec* lights;
  const QuadRec* quads;
  const BvhNode* bvh;  // nullptr when the scene has no BVH
  const BvhPair* bvh_pair;  // the same nodes in the pair layout
  int32_t n_diag, n_gen, n_planes, n_objects, n_lights;
  int32_t n_quads;
  int32_t n_bvh;
  int32_t bvh_depth;  // most far children pending on a traversal stack
  // fast path: the hierarchy over the other bounded records, and what stays
  // outside every hierarchy (tested exhaustively, with the planes)
  const BvhNode* obvh;      // nullptr when there are no culled other records
  const OtherRec* orec;     // in obvh leaf order
  int32_t n_obvh, obvh_depth, n_orec;
  // the line hierarchy (line_trace): open tubes and cones with finite bounds,
  // culled over the whole line up to the hit; the cones' a ~ 0 clusters
  const BvhNode* lbvh;          // nullptr when there are none
  const QuadRec* lrec;          // in lbvh leaf order
  const ConeCluster* lclus;     // the cones' clusters (cone_prepass)
  const int32_t* lcone;         // cluster members: indices into lrec
  const int32_t* lrec_clus;     // per line record: its cone's cluster (-1: an open tube)
  int32_t n_lbvh, n_lrec, n_lclus;
  const SphereGen* fx_gen;  // general spheres outside the hierarchies
  const QuadRec* fx_quads;  // cubes / cylinders / cones outside the hierarchies
  int32_t n_fx_gen, n_fx_quads;
  const LbCell* lb_cells;  // light buffer: n_lights * 6R^2 cells, nullptr when not built
  const uint16_t* lb_ov;
  const float* lb_delta;   // n_lights * n_diag
  const float* lb_limit;   // per light
  int32_t lb_res;          // R
  int32_t lb_n_items;
  // the sphere hierarchy collapsed to four children per node (nullptr when its
  // 16-bit codes cannot index it), and the most stack entries its traversal keeps
  const BvhWide* bvhw;
  const BvhWide16* bvhw16;  // the same nodes in binary16 (the global-memory image)
  int32_t n_bvhw, bvhw_stack;
  // per object: ShadeRec::reflective, transparency (what wf_combine_parents reads; 16 B a
  // record, so the table stays in the L2 where the 512-B shading records may not)
  const double* refl_transp;
  // per object: the index of its SphereDiag record (-1: not one), after the hierarchy's reordering,
  // | kOwnOutside when a shadow ray leaving its outside provably never meets it (rt_scene.cpp)
  const int32_t* obj_diag;
  // Groups (group.rs): the records' gates index this table (rt_scene_create_groups)
  const GroupRec* groups;
  int32_t n_groups, pad_groups;
  // Triangles (rt_scene_create_mesh): every record in object order (the
  // exhaustive loops), their shade table, and on the fast path the hierarchy
  // over them (tri_trace; `trec` in its leaf order) with the records it does
  // not hold (`fx_tris`, tested exhaustively by trace_rest)
  const TriRec* tris;
  const TriShade* tri_shade;
  const BvhNode* tbvh;  // nullptr when there is none
  const TriRec* trec;
  const TriRec* fx_tris;
  int32_t n_tris, n_tbvh, n_trec, n_fx_tris, tbvh_depth, pad_tris;
  // Csg (rt_scene_create_tree): the units, their programs, nodes and leaves (csg_units), and
  // the leaves by counter class (the reference's shape tests of a ray count them too)
  const CsgUnit* csg_units;
  const CsgOp* csg_ops;
  const CsgRec* csg_nodes;
  const OtherRec* csg_leaves;
  const TriRec* csg_tris;  // the triangle leaves of the wide units (they are in no other list)
  int32_t n_csg_units, n_csg_sph, n_csg_planes, n_csg_other;
  // on the fast path the hierarchy over the units' padded world boxes (unit_trace; `urec`: the
  // boxed units' records in its leaf order) and the units it does not hold (`fx_units`, every
  // one of them evaluated by trace_rest); programs, nodes and leaves stay where they are
  const BvhNode* ubvh;  // nullptr when there is none
  const CsgUnit* urec;
  const CsgUnit* fx_units;
  int32_t n_ubvh, n_urec, n_fx_units, ubvh_depth;
  // Alias classes (rt_scene_create_aliased; alias_classes): the members' records grouped by
  // class, the classes, and per object the least object index of its class (its own index when
  // it is in none: alias_finish). The members by counter class, as the Csg leaves.
  const OtherRec* alias_rec;
  const AliasClass* alias_cls;
  const int32_t* alias_of;
  int32_t n_alias_rec, n_alias_cls;
  int32_t n_alias_sph, n_alias_planes, n_alias_other, pad_alias;
  // Deep Csg units (rt_scene_create_ex, RT_SCENE_DEEP_CSG; csg_deep_eval). `csg_counts`: per op of
  // the programs its spheres and planes below (two words; nullptr without a deep unit).
  // csg_deep_nw / _lw / _levels: the scene's largest deep unit in filter words, parity words and
  // levels (all 0: no deep unit). csg_deep_state / _lanes: the launch's own state buffer and the
  // lanes it holds (the workspace's or the batch call's: set in its copy of this struct, never in
  // the scene's), csg_deep_words(...) * lanes words.
  const uint32_t* csg_counts;
  uint32_t* csg_deep_state;
  uint32_t csg_deep_lanes;
  int32_t csg_deep_nw, csg_deep_lw, csg_deep_levels;
  // Run hierarchies (CsgRun). `csg_run_recs` / `csg_run_nodes`: the scene's runs and their nodes
  // (nullptr without one). `csg_runs`: what a launch walks: csg_run_recs in the copy of this struct
  // a fast-path render launches with (Wavefront::render), nullptr in the scene's own, so the
  // exhaustive renders and the batch entry points test every triangle of a run.
  const CsgRun* csg_runs;
  const CsgRun* csg_run_recs;
  const BvhNode* csg_run_nodes;
  int32_t n_csg_runs, pad_runs;
};

constexpr int32_t kOwnOutside = 0x40000000, kOwnIndex = 0x3FFFFFFF;  // DevScene::obj_diag

struct DevCamera {
  double pixel_size, half_width, half_height;
  double inv[12];
  uint32_t hsize, vsize;
};

// Counters of one render (order = rt_stats prefix, then its ABI-3 fields).
struct DevStats {
  unsigned long long rays_primary, rays_reflect, rays_refract, rays_shadow;
  unsigned long long sphere_tests, plane_tests, sphere_disc_ge0, other_tests;
  unsigned long long rays_shadow_traced, sphere_tests_executed, box_tests_executed;
  unsigned exhaustive;  // sphere_disc_ge0 is exact (every sphere tested for every reference ray)
};

}  // namespace rtamd
