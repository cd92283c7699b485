// rt_csg.hpp — the filter of a `Csg` (geometry/shape/csg.rs): the truth table of
// its three operations and, over one fixed-capacity intersection list per ray,
// each node's sort, filter and merge into the enclosing node's list.
//
// Plain C++ without device builtins: the kernels (rt_device.hpp csg_units)
// and a host compiler (tests/cpp/csg_check.cpp) build the same functions.
//
// The list holds (t, key), key = (object index << kKeyShift) | position in the
// object's own local_intersect list, appended in the reference's order: depth
// first, a CSG's left before its right, each leaf's list in push order. A CSG
// node owns the tail of the list from the length it found on entry: on exit
// that tail is left_xs ++ right_xs, both already filtered by the nodes below
// (nested CSGs filter bottom-up), and csg_close sorts and filters it in place.
#pragma once
#include <stdint.h>

#include "rt_layout.hpp"

#if defined(__HIPCC__)
#define RT_CSG_FN __host__ __device__ inline
#else
#define RT_CSG_FN inline
#endif

namespace rtamd {

enum { kCsgUnion = 0, kCsgIntersection = 1, kCsgDifference = 2 };  // Operation (csg.rs:14-19)

// Compile-time caps of one unit (a Csg with no Csg above it); a world beyond one
// is refused when the scene is created (rt_scene_create_tree).
constexpr int kCsgMaxLeaves = 16;  // primitives under one unit
constexpr int kCsgMaxDepth = 4;    // Csg nodes on a path from the unit down (groups between them are free)
// A leaf yields at most 4 intersections (list position 0..3, kKeyShift)
constexpr int kCsgListCap = kCsgMaxLeaves * (1 << kKeyShift);

struct CsgList {
  double t[kCsgListCap];
  int32_t key[kCsgListCap];
  int n;
};

// Operation::intersection_allowed (csg.rs:22-41)
RT_CSG_FN bool csg_allowed(int op, bool lhit, bool inl, bool inr) {
  if (op == kCsgUnion) return (lhit && !inr) || (!lhit && !inl);
  if (op == kCsgIntersection) return (lhit && inr) || (!lhit && inl);
  return (lhit && !inr) || (!lhit && inl);
}

// One intersection of a leaf; false when the list is full (the caps rule that out).
RT_CSG_FN bool csg_push(CsgList& xs, double t, int32_t key) {
  if (xs.n >= kCsgListCap) return false;
  xs.t[xs.n] = t;
  xs.key[xs.n] = key;
  ++xs.n;
  return true;
}

// intersections() (intersection.rs:108-116) over xs[start..n): by t, ties kept in
// list order (the project's stable rule: left's before right's, each in its own order).
RT_CSG_FN void csg_sort(CsgList& xs, int start) {
  for (int i = start + 1; i < xs.n; ++i) {
    const double t = xs.t[i];
    const int32_t k = xs.key[i];
    int j = i;
    while (j > start && xs.t[j - 1] > t) {
      xs.t[j] = xs.t[j - 1];
      xs.key[j] = xs.key[j - 1];
      --j;
    }
    xs.t[j] = t;
    xs.key[j] = k;
  }
}

// Csg::filter_intersections (csg.rs:71-91) over xs[start..n), in place.
// `split`: the first object index of the node's right child (CsgRec::split).
RT_CSG_FN void csg_filter(CsgList& xs, int start, int op, int32_t split) {
  bool inl = false, inr = false;
  int out = start;
  for (int i = start; i < xs.n; ++i) {
    const bool lhit = (xs.key[i] >> kKeyShift) < split;
    if (csg_allowed(op, lhit, inl, inr)) {
      xs.t[out] = xs.t[i];
      xs.key[out] = xs.key[i];
      ++out;
    }
    if (lhit) inl = !inl;
    else inr = !inr;
  }
  xs.n = out;
}

// The end of Csg::local_intersect (csg.rs:123-125) for the node that found the
// list at length `start`.
RT_CSG_FN void csg_close(CsgList& xs, int start, int op, int32_t split) {
  csg_sort(xs, start);
  csg_filter(xs, start, op, split);
}

}  // namespace rtamd
