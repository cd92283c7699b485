// rt_bvh.hpp — host-side BVHs over the bounded records and the light buffer (see rt_layout.hpp).
#pragma once
#include <stddef.h>
#include <vector>

#include "rt_csg.hpp"
#include "rt_layout.hpp"

namespace rtamd {

// Builds the hierarchy over `spheres` (reordered in place into leaf order;
// `meta` keeps each record's object index, so keys and results do not depend
// on the order). Boxes are the exact world-space extent of each record's
// unit sphere under its stored inverse, padded outward (conservative
// culling: DESIGN.md "Exact culling"). Returns the node array (root = 0),
// empty when there are no spheres.
// `depth` receives the most far children a near-first traversal keeps
// pending (the number of internal nodes on the longest root-leaf path).
// `trav_cost`: SAH cost of a node visit relative to one sphere test.
std::vector<BvhNode> build_sphere_bvh(std::vector<SphereDiag>& spheres, int leaf_size, int* depth = nullptr,
                                      double trav_cost = 1.0);

// The nodes in the pair layout of the per-lane traversal (rt_layout.hpp BvhPair).
std::vector<BvhPair> pair_layout(const std::vector<BvhNode>& nodes);

// The hierarchy collapsed to four children per node (rt_layout.hpp BvhWide)
// over the records in leaf order (`spheres`, as build_sphere_bvh left them):
// each node takes its binary children and opens the one of largest box area
// (a binary node, or a leaf of several records that fits whole) until it
// holds four; every leaf of the result is one record (code 0x8000 | index).
// Node 0 is the root; the first nodes are in breadth-first order (a prefix is
// the top of the tree, for an LDS treelet). `stack` receives the most entries
// a near-first traversal keeps pending. Empty when the 16-bit codes cannot
// index the nodes or records.
std::vector<BvhWide> wide_layout(const std::vector<BvhNode>& nodes, const std::vector<SphereDiag>& spheres,
                                 int* stack);

// the global-memory copy of a four-wide image: its boxes rounded outward to binary16
std::vector<BvhWide16> wide16_layout(const std::vector<BvhWide>& w);
// binary16 bit patterns rounded outward (BvhWide16 boxes)
uint16_t f16_bits_down(double x);
uint16_t f16_bits_up(double x);

// The other bounded records (general-transform spheres, cubes, closed
// cylinders with finite caps; rt_layout.hpp OtherRec): other_box gives the
// padded world box of one (false for a cone, an open or unbounded cylinder,
// min > max or NaN bounds, a transform of condition above 1e6 or with a
// non-finite entry, a cube too large for its widening: the line hierarchy or
// the exhaustive loop takes those). The contract (tests/cpp/other_box_check.cpp):
// for every finite ray with |d|_inf >= kOtherDirMin from |o|_inf <=
// kOtherOriginMax, each finite root t the record's test produces has o + t d
// inside the box (a cube's box is widened for Cube::check_axis's parallel
// rule, which is what needs the ray domain; from a farther origin inside the
// box grown by other_far_pad, rt_layout.hpp). For a sphere or a cube an odd
// number of roots at t < 0 means the origin is inside the box, so those are
// culled over [0, t_hi]; a closed cylinder (other_needs_line) keeps no such
// rule (only its caps are tested when dx^2 + dz^2 < EPSILON) and is culled
// over (-inf, t_hi] by radiance rays. build_other_bvh builds the hierarchy
// over records that all have a box (reordered in place into leaf order) and
// sets BvhNode::line for the children that hold a record of the line rule;
// empty when there are none.
bool other_box(const OtherRec& r, double lo[3], double hi[3]);
bool other_needs_line(const OtherRec& r);
std::vector<BvhNode> build_other_bvh(std::vector<OtherRec>& recs, int leaf_size, int* depth = nullptr,
                                     double trav_cost = 1.0);

// The line hierarchy (rt_layout.hpp ConeCluster): line_box
// gives the padded world box of an open tube or a cone with finite bounds
// (false for any other record, or an ill-conditioned transform);
// build_line_bvh builds the hierarchy over records that all have one, leaves
// of one record where the builder can split (reordered in place into leaf
// order), and the cones' clusters (cones of one direction quadratic, their
// members' indices into `recs` in `members`); empty when there are none.
bool line_box(const QuadRec& r, double lo[3], double hi[3]);
std::vector<BvhNode> build_line_bvh(std::vector<QuadRec>& recs, std::vector<ConeCluster>* clusters,
                                    std::vector<int32_t>* members, int* depth = nullptr);

// The triangle hierarchy (rt_trace.hpp tri_trace, DESIGN.md §5.2 "Triangles"):
// tri_box gives the padded world box of a triangle's three vertices (false
// for an ill-conditioned transform: the exhaustive loop takes it);
// build_tri_bvh builds the hierarchy over records that all have one
// (reordered in place into leaf order); empty when there are none.
bool tri_box(const TriRec& r, double lo[3], double hi[3]);
// The same for rays with |d|_inf <= dir_max from |o|_inf <= origin_max (the one above: kTriDirMax,
// kTriOriginMax, bit for bit).
bool tri_box(const TriRec& r, double dir_max, double origin_max, double lo[3], double hi[3]);
std::vector<BvhNode> build_tri_bvh(std::vector<TriRec>& recs, int leaf_size, int* depth = nullptr,
                                   double trav_cost = 1.0);

// The run hierarchies inside wide and deep Csg units (rt_layout.hpp CsgRun, rt_slab.hpp
// csg_run_walk, DESIGN.md §5.2 "Csg units: run hierarchies"). csg_run_bounds: bounds on |d|_inf and
// |o|_inf of the ray chained down `n` Csg inverses (3x4, the outermost first) from a world ray
// within kTriDirMax / kTriOriginMax. build_csg_run: the hierarchy over the run's records
// recs[0 .. n): each one's box is tri_box with the run's bounds, in the space of the chained ray;
// the boxed records come first, in leaf order, the ones tri_box refuses after them (the remainder,
// tested by every ray); `n_boxed` receives the former's count. Empty, with the records untouched:
// fewer than `min_boxed` boxed records, or a tree deeper than kBvhMaxDepth.
void csg_run_bounds(const double* const* chain, int n, double* dir_max, double* origin_max);
std::vector<BvhNode> build_csg_run(TriRec* recs, int n, double dir_max, double origin_max, int min_boxed, int leaf_size,
                                   double trav_cost, int* n_boxed, int* depth);

// The Csg units' hierarchy (rt_trace.hpp unit_trace, DESIGN.md §5.2 "Csg units: the fifth
// hierarchy"). csg_unit_box: the padded world box of one unit's program ops[first .. first + n).
// For every ray (o, d) with |o|_inf <= kUnitOriginMax and every leaf of the unit, each root t
// the leaf's test produces on the chained ray (the world ray through every enclosing Csg's
// inverse one after another, then the leaf's) has o + t d inside the box: a superset of what
// survives the filters. The box comes from the leaves' own regions carried up the forward
// chain; the reference's get_bounds() gate stays in the program and takes no part. False (the
// unit stays in the exhaustive loop): a plane or cone leaf, a cylinder without finite bounds,
// an ill-conditioned matrix or chain, a non-finite result.
// build_unit_bvh: the hierarchy over such boxes (six doubles a unit: lo, hi); `order` receives
// the units' leaf order. Empty when there are none.
bool csg_unit_box(const CsgOp* ops, int first, int n, const CsgRec* nodes, const OtherRec* leaves, double lo[3],
                  double hi[3]);
std::vector<BvhNode> build_unit_bvh(const std::vector<double>& boxes, int leaf_size, int* depth,
                                    std::vector<int>* order, double trav_cost = 1.0);

// Light buffer over the shadow-casting records, one cube map of R x R cells
// per face per light (rt_layout.hpp LbCell; DESIGN.md "Light buffer").
// Empty (cells.size() == 0) when there are no records, or 65535 or more.
struct LightBuffer {
  int res = 0;
  size_t n_items = 0;
  std::vector<LbCell> cells;    // n_lights * 6R^2
  std::vector<uint16_t> ov;     // list entries past the inline ones
  std::vector<float> delta;     // n_lights * n_records
  std::vector<float> limit;     // per light
};
LightBuffer build_light_buffer(const std::vector<SphereDiag>& spheres, const std::vector<LightRec>& lights, int R);

}  // namespace rtamd
