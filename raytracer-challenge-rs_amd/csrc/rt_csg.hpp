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
constexpr int kCsgMaxLeaves = 16;  // primitives of kinds 0-4 under one unit (its triangles are not counted)
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

// ---- The stream form, for a WIDE unit (one with triangle leaves: its list has no
// small bound). The nested "sort left ++ right, filter, hand up" is one global order,
// ascending (t, key): a unit's leaves have consecutive object indices depth first, so
// every node's stable sort orders equal t by key, each node's list is a subsequence of
// that order, and a node sees exactly what every node below it let through. So the
// roots can be taken in ascending (t, key), a batch at a time, and each one sent up its
// chain of enclosing Csg nodes, innermost first, until a node drops it: the nodes above
// a drop never see it, and their state does not move. Per node the state is the two
// bits of filter_intersections, `inl` and `inr`: one bit per node of the unit in two
// words, hence the cap.
constexpr int kCsgMaxNodes = 32;  // Csg nodes in one wide unit

// A batch entry's tag: the innermost Csg node above its leaf (the unit's node number,
// < kCsgMaxNodes), and the leaf's place in the fold's table: its number among the unit's
// leaves of kinds 0-4 (< kCsgMaxLeaves), or kCsgTagTri for a triangle (one root, no place).
constexpr int kCsgTagNode = 31, kCsgTagSlotShift = 5, kCsgTagSlot = 15, kCsgTagTri = 1 << 9;
template <typename Tag>
struct CsgBatchT {
  CsgList xs;
  Tag tag[kCsgListCap];
};
typedef CsgBatchT<uint16_t> CsgBatch;

RT_CSG_FN bool csg_above(double t, int32_t key, double wt, int32_t wk) { return t > wt || (t == wt && key > wk); }

// One root into the batch of the `cap` smallest (t, key) above the watermark (wt, wk),
// kept ascending by insertion; `more`: a root above the watermark was left out (walk
// again from the batch's last entry). A NaN t is above no watermark (the reference's
// sort panics on one).
template <typename Tag>
RT_CSG_FN void csg_batch_insert(CsgBatchT<Tag>& b, int cap, double t, int32_t key, Tag tag, double wt, int32_t wk,
                                bool& more) {
  if (!csg_above(t, key, wt, wk)) return;
  CsgList& xs = b.xs;
  int j = xs.n;
  if (xs.n >= cap) {
    more = true;
    if (csg_above(t, key, xs.t[cap - 1], xs.key[cap - 1])) return;
    j = cap - 1;  // the last entry falls out
  } else {
    ++xs.n;
  }
  while (j > 0 && csg_above(xs.t[j - 1], xs.key[j - 1], t, key)) {
    xs.t[j] = xs.t[j - 1];
    xs.key[j] = xs.key[j - 1];
    b.tag[j] = b.tag[j - 1];
    --j;
  }
  xs.t[j] = t;
  xs.key[j] = key;
  b.tag[j] = tag;
}

// One root of the stream up its chain: `nodes` the unit's CsgRecs (the unit's own
// first), `node` the innermost one above the root's leaf. At each node lhit from its
// split, the truth table, then the toggle (csg.rs:71-91); false at the first drop.
RT_CSG_FN bool csg_stream_pass(const CsgRec* nodes, int node, int32_t key, uint32_t& inl, uint32_t& inr) {
  const int32_t obj = key >> kKeyShift;
  for (int g = node; g >= 0; g = nodes[g].parent) {
    const uint32_t bit = 1u << g;
    const bool lhit = obj < nodes[g].split;
    const bool ok = csg_allowed(nodes[g].op, lhit, (inl & bit) != 0, (inr & bit) != 0);
    if (lhit) inl ^= bit;
    else inr ^= bit;
    if (!ok) return false;
  }
  return true;
}

// The streamed fold's table: per leaf of kinds 0-4 (by its place) the count of its
// survivors t < 0 so far and the last of them. The stream is ascending, so when a
// survivor t >= 0 arrives every survivor t < 0 of its leaf has been counted (`hin`), and
// at the end a leaf with an odd count is a container candidate at its last one.
struct CsgNegTable {
  double t[kCsgMaxLeaves];
  int32_t key[kCsgMaxLeaves];
  uint32_t odd;  // bit s: leaf s has an odd number of survivors t < 0
};
RT_CSG_FN void csg_neg_note(CsgNegTable& nt, int slot, double t, int32_t key) {
  nt.t[slot] = t;
  nt.key[slot] = key;
  nt.odd ^= 1u << slot;
}

// ---- The same stream for a DEEP unit (rt_layout.hpp kCsgDeep): one of any depth, node and
// leaf count. Nothing in the argument above depends on them; only the state does. Here it
// scales: the filter bits are bitsets of `nw` words each, the leaves' parities one of `lw`
// words, all in the launch's state buffer (`W`: word i of this lane), and the containers need
// no per-leaf table (csg_deep_note).
//
// The tag: the innermost Csg node above the leaf (15 bits), the leaf's number among the unit's
// leaves of kinds 0-4 (16 bits), or kCsgDeepTagTri for a triangle.
constexpr uint32_t kCsgDeepTagNode = (uint32_t)kCsgDeepMaxNodes - 1, kCsgDeepTagSlot = (uint32_t)kCsgDeepMaxLeaves - 1;
constexpr uint32_t kCsgDeepTagTri = 1u << 31;
constexpr int kCsgDeepTagSlotShift = 15;
typedef CsgBatchT<uint32_t> CsgDeepBatch;

// One lane's words of the state buffer (rt_layout.hpp csg_deep_words).
struct CsgDeepWords {
  uint32_t* w;
  size_t stride;
  RT_CSG_FN uint32_t& operator[](int i) const { return w[(size_t)i * stride]; }
};

// csg_stream_pass over the bitsets: inl at words [0, nw), inr at [nw, 2 nw).
RT_CSG_FN bool csg_deep_pass(const CsgRec* nodes, int node, int32_t key, const CsgDeepWords& st, int nw) {
  const int32_t obj = key >> kKeyShift;
  for (int g = node; g >= 0; g = nodes[g].parent) {
    const uint32_t bit = 1u << (g & 31);
    const int wl = g >> 5, wr = nw + (g >> 5);
    const uint32_t l = st[wl], r = st[wr];
    const bool lhit = obj < nodes[g].split;
    const bool ok = csg_allowed(nodes[g].op, lhit, (l & bit) != 0, (r & bit) != 0);
    if (lhit) st[wl] = l ^ bit;
    else st[wr] = r ^ bit;
    if (!ok) return false;
  }
  return true;
}

// The unit's closest survivor so far, as the caller's Hit holds it.
struct CsgDeepHit {
  double t;
  int32_t key;
  int hin;
};
// The first pass: one entry of the ascending stream. The parity bits (words [2 nw, 2 nw + lw))
// toggle at each survivor t < 0 of a leaf of kinds 0-4; when a survivor t >= 0 arrives all of its
// leaf's survivors t < 0 have passed, so its bit is `hin`. `eligible(key)`: the leaf may be the
// hit (a shadow ray's: it casts one). Returns kCsgDeepDone at the unit's hit or at the first
// entry beyond h.t (nothing later is a hit, a container or `hin`), kCsgDeepTriNeg for a
// triangle's surviving root t < 0 (one root a leaf: the caller's container at once).
enum { kCsgDeepGoOn = 0, kCsgDeepDone = 1, kCsgDeepTriNeg = 2 };
template <typename Eligible>
RT_CSG_FN int csg_deep_step(const CsgRec* nodes, const CsgDeepWords& st, int nw, double t, int32_t key, uint32_t tag,
                            Eligible eligible, CsgDeepHit& h) {
  if (t > h.t) return kCsgDeepDone;
  if (!csg_deep_pass(nodes, (int)(tag & kCsgDeepTagNode), key, st, nw)) return kCsgDeepGoOn;
  const bool tri = (tag & kCsgDeepTagTri) != 0;
  const int slot = (int)((tag >> kCsgDeepTagSlotShift) & kCsgDeepTagSlot);
  if (t < 0.0) {
    if (tri) return kCsgDeepTriNeg;
    st[2 * nw + (slot >> 5)] ^= 1u << (slot & 31);
    return kCsgDeepGoOn;
  }
  if (!eligible(key)) return kCsgDeepGoOn;
  if (t < h.t || (t == h.t && key < h.key)) {
    h.t = t;
    h.key = key;
    h.hin = tri ? 0 : (int)((st[2 * nw + (slot >> 5)] >> (slot & 31)) & 1u);
  }
  return kCsgDeepDone;
}

// The second pass, over the part t < 0 of the same stream with fresh filter bits, when the first
// left a leaf odd: the caller's `containers` walk (push_container) needs of the unit only, among
// the leaves with an odd number of survivors t < 0, the two whose LAST such survivor is greatest
// by (t, key). The parities are final now, so a survivor of an odd leaf is a candidate as it
// arrives: c1 is the latest of them, c2 the latest one of a DIFFERENT leaf than c1's. A survivor
// of c1's leaf replaces c1; one of another leaf moves c1 to c2 and takes c1: the entry before a
// new c1 is the latest survivor of every other leaf. At the end c1 is the greatest last survivor
// and c2 the greatest among the other leaves'.
struct CsgDeepTop2 {
  double t1, t2;
  int32_t k1, k2;
  int32_t slot1;  // c1's leaf, -1: none yet
};
RT_CSG_FN void csg_deep_top2_init(CsgDeepTop2& c) {
  c.k1 = c.k2 = -1;
  c.slot1 = -1;
  c.t1 = c.t2 = 0.0;
}
RT_CSG_FN void csg_deep_note(const CsgRec* nodes, const CsgDeepWords& st, int nw, double t, int32_t key, uint32_t tag,
                             CsgDeepTop2& c) {
  if (!csg_deep_pass(nodes, (int)(tag & kCsgDeepTagNode), key, st, nw)) return;
  if (tag & kCsgDeepTagTri) return;  // (the first pass pushed it)
  const int slot = (int)((tag >> kCsgDeepTagSlotShift) & kCsgDeepTagSlot);
  if (!((st[2 * nw + (slot >> 5)] >> (slot & 31)) & 1u)) return;
  if (slot != c.slot1) {
    c.t2 = c.t1;
    c.k2 = c.k1;
    c.slot1 = slot;
  }
  c.t1 = t;
  c.k1 = key;
}

}  // namespace rtamd
