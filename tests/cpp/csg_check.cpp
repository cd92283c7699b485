// csg_check.cpp — host check of rt_csg.hpp (the Csg filter the kernels run), a
// stand-alone program: the reference's truth table (csg.rs:156-205) and filter
// cases (csg.rs:207-240), and seeded random trees up to the depth cap over random
// hit lists (ties included), each against a literal vector-based restatement of
// Csg::local_intersect's tail (csg.rs:120-125): concatenate, stable sort, filter
// with `includes` as membership in the left subtree.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <set>
#include <vector>

#include "rt_csg.hpp"

using namespace rtamd;

static int failures = 0;
#define CHECK(c)                                                 \
  do {                                                           \
    if (!(c)) {                                                  \
      ++failures;                                                \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);   \
    }                                                            \
  } while (0)

struct X {
  double t;
  int32_t key;
};
static bool allowed_ref(int op, bool lhit, bool inl, bool inr) {  // csg.rs:22-41, as written
  switch (op) {
    case kCsgUnion: return (lhit && !inr) || (!lhit && !inl);
    case kCsgIntersection: return (lhit && inr) || (!lhit && inl);
    default: return (lhit && !inr) || (!lhit && inl);
  }
}
static std::vector<X> filter_ref(int op, const std::set<int>& left, const std::vector<X>& xs) {  // csg.rs:71-91
  bool inl = false, inr = false;
  std::vector<X> result;
  for (const X& x : xs) {
    const bool lhit = left.count(x.key >> kKeyShift) != 0;
    if (allowed_ref(op, lhit, inl, inr)) result.push_back(x);
    if (lhit) inl = !inl;
    else inr = !inr;
  }
  return result;
}

// a random tree: node < 0 is a leaf (object index -node - 1)
struct Node {
  int op, left, right;
};
struct Tree {
  std::vector<Node> nodes;
  std::vector<std::vector<X>> hits;  // per leaf object, in push order
  int n_leaves = 0;
};
static int grow(Tree& t, std::mt19937& rng, int depth) {
  if (depth == 0 || (depth < kCsgMaxDepth && rng() % 3 == 0)) return -(++t.n_leaves);
  const int me = (int)t.nodes.size();
  t.nodes.push_back(Node{(int)(rng() % 3), 0, 0});
  const int l = grow(t, rng, depth - 1);  // left first: objects in depth-first order
  const int r = grow(t, rng, depth - 1);
  t.nodes[me].left = l;
  t.nodes[me].right = r;
  return me;
}
static void leaves_of(const Tree& t, int n, std::set<int>& out) {
  if (n < 0) { out.insert(-n - 1); return; }
  leaves_of(t, t.nodes[n].left, out);
  leaves_of(t, t.nodes[n].right, out);
}
static std::vector<X> eval_ref(const Tree& t, int n) {
  if (n < 0) return t.hits[-n - 1];
  std::vector<X> xs = eval_ref(t, t.nodes[n].left);
  const std::vector<X> r = eval_ref(t, t.nodes[n].right);
  xs.insert(xs.end(), r.begin(), r.end());
  std::stable_sort(xs.begin(), xs.end(), [](const X& a, const X& b) { return a.t < b.t; });
  std::set<int> left;
  leaves_of(t, t.nodes[n].left, left);
  return filter_ref(t.nodes[n].op, left, xs);
}
// the kernels' way: one list, each node closes its tail
static void eval_list(const Tree& t, int n, CsgList& xs) {
  if (n < 0) {
    for (const X& x : t.hits[-n - 1]) CHECK(csg_push(xs, x.t, x.key));
    return;
  }
  const int start = xs.n;
  eval_list(t, t.nodes[n].left, xs);
  std::set<int> right;
  leaves_of(t, t.nodes[n].right, right);
  const int32_t split = *right.begin();  // the right child's first object
  eval_list(t, t.nodes[n].right, xs);
  csg_close(xs, start, t.nodes[n].op, split);
}

int main() {
  // the truth table
  const int T = 1, F = 0;
  const int rows[24][5] = {
      {kCsgUnion, T, T, T, F}, {kCsgUnion, T, T, F, T}, {kCsgUnion, T, F, T, F}, {kCsgUnion, T, F, F, T},
      {kCsgUnion, F, T, T, F}, {kCsgUnion, F, T, F, F}, {kCsgUnion, F, F, T, T}, {kCsgUnion, F, F, F, T},
      {kCsgIntersection, T, T, T, T}, {kCsgIntersection, T, T, F, F}, {kCsgIntersection, T, F, T, T},
      {kCsgIntersection, T, F, F, F}, {kCsgIntersection, F, T, T, T}, {kCsgIntersection, F, T, F, T},
      {kCsgIntersection, F, F, T, F}, {kCsgIntersection, F, F, F, F},
      {kCsgDifference, T, T, T, F}, {kCsgDifference, T, T, F, T}, {kCsgDifference, T, F, T, F},
      {kCsgDifference, T, F, F, T}, {kCsgDifference, F, T, T, T}, {kCsgDifference, F, T, F, T},
      {kCsgDifference, F, F, T, F}, {kCsgDifference, F, F, F, F}};
  for (const auto& r : rows) CHECK(csg_allowed(r[0], r[1] != 0, r[2] != 0, r[3] != 0) == (r[4] != 0));
  // filtering a list of intersections: s1 (object 0) left, s2 (object 1) right; t = 1 2 3 4
  const int want[3][2] = {{0, 3}, {1, 2}, {0, 1}};
  for (int op = 0; op < 3; ++op) {
    CsgList xs;
    xs.n = 0;
    for (int i = 0; i < 4; ++i) csg_push(xs, 1.0 + i, (i & 1) << kKeyShift | (i >> 1));
    csg_close(xs, 0, op, 1);
    CHECK(xs.n == 2 && xs.t[0] == 1.0 + want[op][0] && xs.t[1] == 1.0 + want[op][1]);
  }
  // the list never overflows its capacity
  {
    CsgList xs;
    xs.n = 0;
    for (int i = 0; i < kCsgListCap; ++i) CHECK(csg_push(xs, (double)(i % 7), i));
    CHECK(!csg_push(xs, 0.0, 0) && xs.n == kCsgListCap);
    csg_close(xs, 0, kCsgUnion, 1 << 20);
    CHECK(xs.n <= kCsgListCap);
  }
  // random trees over random hit lists
  std::mt19937 rng(20240607u);
  long long survivors = 0, ties = 0, deep = 0;
  for (int it = 0; it < 4000; ++it) {
    Tree t;
    const int root = grow(t, rng, 1 + (int)(rng() % kCsgMaxDepth));
    CHECK(t.n_leaves <= kCsgMaxLeaves);
    if (root < 0) continue;
    t.hits.resize((size_t)t.n_leaves);
    for (int l = 0; l < t.n_leaves; ++l) {
      const int n = (int)(rng() % 5);  // 0..4 intersections a leaf, in push order (not sorted)
      for (int i = 0; i < n; ++i)
        t.hits[(size_t)l].push_back(X{(double)((int)(rng() % 17) - 8) * 0.5, (int32_t)(l << kKeyShift | i)});
    }
    const std::vector<X> ref = eval_ref(t, root);
    CsgList xs;
    xs.n = 0;
    eval_list(t, root, xs);
    CHECK(xs.n == (int)ref.size());
    for (int i = 0; i < xs.n && i < (int)ref.size(); ++i) CHECK(xs.t[i] == ref[(size_t)i].t && xs.key[i] == ref[(size_t)i].key);
    survivors += xs.n;
    for (size_t i = 1; i < ref.size(); ++i) ties += ref[i].t == ref[i - 1].t;
    deep += t.nodes.size() >= (size_t)kCsgMaxDepth;
  }
  CHECK(survivors > 4000 && ties > 500 && deep > 200);
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("OK survivors=%lld ties=%lld deep_trees=%lld\n", survivors, ties, deep);
  return 0;
}
