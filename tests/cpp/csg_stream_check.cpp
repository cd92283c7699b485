// csg_stream_check.cpp — host check of the stream form in rt_csg.hpp (what the wide
// units' evaluator runs per ray: csg_batch_insert, csg_stream_pass, CsgNegTable), a
// stand-alone program. Seeded random units (up to kCsgMaxNodes Csg nodes, kCsgMaxDepth
// deep, groups of several children between the nodes, all three operations) over random
// root lists (ties in t, roots before and behind the origin, leaves of 1, 2 and 4 roots),
// each evaluated twice:
//   - literally nested: every node concatenates its children's lists, sorts them stably
//     by t, and filters them with csg_filter, bottom up; then a literal fold of the
//     unit's survivors (first t >= 0, the parity of its leaf's survivors t < 0, every
//     leaf with an odd number of those at its last one, the two greatest);
//   - by the stream functions, batch after batch above a watermark, with batch
//     capacities 1, 2, 3 and kCsgListCap, folding as csg_wide_eval folds.
// The survivors in order, the hit, `hin` and both container candidates must be identical.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
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
struct Leaf {
  int node;            // the innermost Csg node above it
  int slot;            // its place among the leaves of kinds 0-4, -1: a triangle (one root)
  std::vector<X> xs;   // its roots in push order (not sorted)
};
struct Node {
  int op, parent, split;
  std::vector<int> kids[2];  // >= 0: a node; < 0: leaf -(k + 1). A side with several: a group
};
struct Unit {
  std::vector<Node> nodes;
  std::vector<Leaf> leaves;
  int n_slots = 0;
};

// the fold's result
struct Fold {
  double t = INFINITY;
  int32_t key = -1;
  int hin = 0;
  double c1t = -INFINITY, c2t = -INFINITY;
  int32_t c1k = -1, c2k = -1;
  bool operator==(const Fold& o) const {
    return t == o.t && key == o.key && hin == o.hin && c1t == o.c1t && c2t == o.c2t && c1k == o.c1k && c2k == o.c2k;
  }
};
static void push_container(Fold& f, double t, int32_t k) {  // rt_device.hpp push_container
  if (t > f.c1t || (t == f.c1t && k > f.c1k)) {
    f.c2t = f.c1t; f.c2k = f.c1k; f.c1t = t; f.c1k = k;
  } else if (t > f.c2t || (t == f.c2t && k > f.c2k)) {
    f.c2t = t; f.c2k = k;
  }
}

static int new_leaf(Unit& u, std::mt19937& rng, int node, int& budget, bool dense) {
  Leaf l;
  l.node = node;
  int n_roots = 1;
  if (u.n_slots < kCsgMaxLeaves && rng() % (dense ? 12 : 2) == 0) {
    l.slot = u.n_slots++;
    n_roots = 1 << (rng() % 3);  // 1, 2 or 4
  } else {
    l.slot = -1;
    if (rng() % (dense ? 8 : 3) == 0) n_roots = 0;  // the ray misses this triangle
  }
  const int obj = (int)u.leaves.size();
  for (int i = 0; i < n_roots && budget > 0; ++i, --budget)
    l.xs.push_back(X{(double)((int)(rng() % 41) - 20) * 0.25, (int32_t)(obj << kKeyShift | i)});
  u.leaves.push_back(l);
  return -(obj + 1);
}
static int grow(Unit& u, std::mt19937& rng, int depth, int parent, int& budget, bool dense) {
  const int me = (int)u.nodes.size();
  u.nodes.push_back(Node{(int)(rng() % 3), parent, 0, {}});
  for (int side = 0; side < 2; ++side) {
    if (side == 1) u.nodes[(size_t)me].split = (int)u.leaves.size();  // the right child's first object
    int n_kids = 1;
    if (dense) n_kids = 20 + (int)(rng() % 40);  // a group: a mesh
    else if (rng() % 3 == 0) n_kids = 2 + (int)(rng() % 3);
    for (int k = 0; k < n_kids; ++k) {
      int kid;
      if (depth > 1 && (int)u.nodes.size() < kCsgMaxNodes && rng() % 5 < 3) kid = grow(u, rng, depth - 1, me, budget, dense);
      else kid = new_leaf(u, rng, me, budget, dense);
      u.nodes[(size_t)me].kids[side].push_back(kid);
    }
  }
  return me;
}

// ---- literally nested
static std::vector<X> eval_nested(const Unit& u, int n) {
  if (n < 0) return u.leaves[(size_t)(-n - 1)].xs;
  std::vector<X> xs;
  for (int side = 0; side < 2; ++side)
    for (int kid : u.nodes[(size_t)n].kids[side]) {
      const std::vector<X> k = eval_nested(u, kid);
      xs.insert(xs.end(), k.begin(), k.end());
    }
  std::stable_sort(xs.begin(), xs.end(), [](const X& a, const X& b) { return a.t < b.t; });
  // csg_filter works on a CsgList: a piece of kCsgListCap at a time cannot be cut (the filter has state), so
  // the literal filter here is csg_filter's own loop over a vector, with csg_allowed
  bool inl = false, inr = false;
  std::vector<X> out;
  for (const X& x : xs) {
    const bool lhit = (x.key >> kKeyShift) < u.nodes[(size_t)n].split;
    if (csg_allowed(u.nodes[(size_t)n].op, lhit, inl, inr)) out.push_back(x);
    if (lhit) inl = !inl;
    else inr = !inr;
  }
  if (xs.size() <= (size_t)kCsgListCap) {  // ... and csg_filter itself wherever the list fits it
    CsgList l;
    l.n = 0;
    for (const X& x : xs) csg_push(l, x.t, x.key);
    csg_filter(l, 0, u.nodes[(size_t)n].op, u.nodes[(size_t)n].split);
    CHECK(l.n == (int)out.size());
    for (int i = 0; i < l.n && i < (int)out.size(); ++i) CHECK(l.t[i] == out[(size_t)i].t && l.key[i] == out[(size_t)i].key);
  }
  return out;
}
static Fold fold_literal(const std::vector<X>& xs) {  // rt_device.hpp csg_fold, radiance rays
  Fold f;
  for (size_t i = 0; i < xs.size(); ++i) {
    const int obj = xs[i].key >> kKeyShift;
    int n_neg = 0;
    bool last = true;
    for (size_t j = 0; j < xs.size(); ++j)
      if ((xs[j].key >> kKeyShift) == obj && xs[j].t < 0.0) {
        ++n_neg;
        if (j > i) last = false;
      }
    if (xs[i].t >= 0.0) {
      if (f.key < 0) { f.t = xs[i].t; f.key = xs[i].key; f.hin = n_neg & 1; }
    } else if (last && (n_neg & 1)) {
      push_container(f, xs[i].t, xs[i].key);
    }
  }
  return f;
}

// ---- the stream: csg_wide_eval's loop (rt_device.hpp) with a batch of `cap`
static Fold eval_stream(const Unit& u, const std::vector<CsgRec>& recs, int cap, bool stop, std::vector<X>* survivors,
                        int* walks) {
  Fold f;
  CsgBatch b;
  CsgNegTable nt;
  nt.odd = 0;
  uint32_t inl = 0, inr = 0;
  double wt = -INFINITY;
  int32_t wk = -1;
  *walks = 0;
  for (;;) {
    ++*walks;
    b.xs.n = 0;
    bool more = false;
    for (const Leaf& l : u.leaves) {
      const uint16_t tag = (uint16_t)(l.node | (l.slot < 0 ? kCsgTagTri : l.slot << kCsgTagSlotShift));
      for (const X& x : l.xs) csg_batch_insert(b, cap, x.t, x.key, tag, wt, wk, more);
    }
    CHECK(b.xs.n <= cap);
    bool done = false;
    for (int i = 0; i < b.xs.n && !done; ++i) {
      const double t = b.xs.t[i];
      const int32_t key = b.xs.key[i];
      const int tag = b.tag[i];
      CHECK(csg_above(t, key, wt, wk) && (i == 0 || csg_above(t, key, b.xs.t[i - 1], b.xs.key[i - 1])));
      if (!csg_stream_pass(recs.data(), tag & kCsgTagNode, key, inl, inr)) continue;
      if (survivors) survivors->push_back(X{t, key});
      const int slot = (tag >> kCsgTagSlotShift) & kCsgTagSlot;
      if (t < 0.0) {
        if (tag & kCsgTagTri) push_container(f, t, key);
        else csg_neg_note(nt, slot, t, key);
      } else if (f.key < 0) {
        f.t = t; f.key = key; f.hin = (tag & kCsgTagTri) ? 0 : (int)((nt.odd >> slot) & 1u);
        done = stop;
      }
    }
    if (done || !more) break;
    wt = b.xs.t[b.xs.n - 1];
    wk = b.xs.key[b.xs.n - 1];
  }
  for (int s = 0; s < kCsgMaxLeaves; ++s)
    if ((nt.odd >> s) & 1u) push_container(f, nt.t[s], nt.key[s]);
  return f;
}

int main() {
  std::mt19937 rng(20250911u);
  const int caps[4] = {1, 2, 3, kCsgListCap};
  long long cases = 0, multi = 0, ties = 0, survivors_all = 0, full_units = 0, deep = 0, with_hit = 0, with_cont = 0, with_hin = 0;
  for (int it = 0; it < 1500; ++it) {
    Unit u;
    const bool dense = it % 3 == 0;  // a mesh: groups of many triangles, 65 to 200 roots
    int budget = dense ? 65 + (int)(rng() % 136) : 1 + (int)(rng() % 40);
    const int depth = 1 + (int)(rng() % kCsgMaxDepth);
    grow(u, rng, depth, -1, budget, dense);
    CHECK((int)u.nodes.size() <= kCsgMaxNodes && u.n_slots <= kCsgMaxLeaves);
    std::vector<CsgRec> recs(u.nodes.size());
    for (size_t g = 0; g < u.nodes.size(); ++g) {
      recs[g] = CsgRec{};
      recs[g].op = u.nodes[g].op;
      recs[g].split = u.nodes[g].split;
      recs[g].parent = u.nodes[g].parent;
      recs[g].self = (int32_t)g;
    }
    size_t n_roots = 0;
    for (const Leaf& l : u.leaves) n_roots += l.xs.size();
    CHECK(n_roots <= 200);
    const std::vector<X> ref = eval_nested(u, 0);
    const Fold want = fold_literal(ref);
    for (int cap : caps) {
      std::vector<X> got;
      int walks = 0, walks_stop = 0;
      const Fold all = eval_stream(u, recs, cap, false, &got, &walks);
      const Fold stopped = eval_stream(u, recs, cap, true, nullptr, &walks_stop);
      CHECK(got.size() == ref.size());
      for (size_t i = 0; i < got.size() && i < ref.size(); ++i) CHECK(got[i].t == ref[i].t && got[i].key == ref[i].key);
      CHECK(all == want);
      CHECK(stopped == want);
      CHECK(walks_stop <= walks && walks == (int)std::max<size_t>(1, (n_roots + (size_t)cap - 1) / (size_t)cap));
      if (cap == kCsgListCap) multi += walks > 1;
    }
    ++cases;
    survivors_all += (long long)ref.size();
    for (size_t i = 1; i < ref.size(); ++i) ties += ref[i].t == ref[i - 1].t;
    full_units += u.nodes.size() >= 24;
    deep += depth == kCsgMaxDepth;
    with_hit += want.key >= 0;
    with_cont += want.c2k >= 0;
    with_hin += want.hin;
  }
  // at least a fifth of the cases need more than one batch at the kernels' capacity
  CHECK(multi * 5 >= cases);
  CHECK(survivors_all > 5000 && ties > 500 && full_units > 10 && deep > 150 && with_hit > 500 && with_cont > 150 && with_hin > 50);
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("OK cases=%lld multi_batch=%lld survivors=%lld ties=%lld big_units=%lld hits=%lld two_containers=%lld hin=%lld\n",
              cases, multi, survivors_all, ties, full_units, with_hit, with_cont, with_hin);
  return 0;
}
