// csg_deep_check.cpp — host check of the deep units' stream functions in rt_csg.hpp (what
// csg_deep_eval runs per ray: csg_batch_insert with 32-bit tags, csg_deep_pass over the bitsets,
// csg_deep_step, csg_deep_note), a stand-alone program. Seeded random units (up to 200 leaves, 60
// levels, 4 roots a leaf; chains and bushy trees, groups of several leaves on a side, all three
// operations) over random root lists (ties in t, most roots behind the origin in half the
// cases), each evaluated twice:
//   - literally nested: every node concatenates its children's lists, sorts them stably by t and
//     filters them, bottom up; then the hit is the first survivor t >= 0 (of a leaf that may be
//     hit), and the containers are a literal list walk over the survivors before it (an object in
//     the list is removed, one that is not is appended): `hin` is the hit's membership, the two
//     candidates are the list's last two entries;
//   - by the stream functions as csg_deep_eval calls them: batches of `cap` above a watermark, the
//     first pass to the hit, the second over the part t < 0 when a leaf ended odd; the state in a
//     strided word buffer with canaries between the lanes' words.
// The hit, `hin` and both candidates must be identical, for a radiance ray, for a ray whose caller
// already holds a closer or farther hit, and (the hit alone) for a shadow ray past shadowless leaves.
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
  bool shadow;         // casts a shadow
  std::vector<X> xs;   // its roots in push order (not sorted)
};
struct Node {
  int op, parent, split, level;
  std::vector<int> kids[2];  // >= 0: a node; < 0: leaf -(k + 1). A side with several: a group
};
struct Unit {
  std::vector<Node> nodes;
  std::vector<Leaf> leaves;
  int n_slots = 0, levels = 0;
  int owed = 0;  // while growing: sides opened and not yet begun (each takes a leaf at least)
};
struct Fold {
  double t = INFINITY;
  int32_t key = 0x7fffffff;
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

struct Shape {
  int max_leaves, max_levels;
  bool chain, behind;
};
static int new_leaf(Unit& u, std::mt19937& rng, int node, const Shape& sh) {
  Leaf l;
  l.node = node;
  l.shadow = rng() % 5 != 0;
  int n_roots;
  if (rng() % 5 != 0) {
    l.slot = u.n_slots++;
    const int pick = (int)(rng() % 8);
    n_roots = pick == 0 ? 0 : pick < 3 ? 1 : pick < 7 ? 2 : 4;
  } else {
    l.slot = -1;
    n_roots = rng() % 4 == 0 ? 0 : 1;
  }
  const int obj = (int)u.leaves.size();
  for (int i = 0; i < n_roots; ++i) {
    // quarter steps: ties among the leaves; `behind`: four in five roots lie behind the origin
    int q = (int)(rng() % 41) - 20;
    if (sh.behind && q >= 0 && rng() % 5 != 0) q = -q - 1;
    l.xs.push_back(X{(double)q * 0.25, (int32_t)(obj << kKeyShift | i)});
  }
  u.leaves.push_back(l);
  return -(obj + 1);
}
static int grow(Unit& u, std::mt19937& rng, int level, int parent, const Shape& sh) {
  const int me = (int)u.nodes.size();
  const unsigned r = rng() % 25;  // mostly unions: a deep tree of random operations lets next to nothing through
  u.nodes.push_back(Node{r < 22 ? kCsgUnion : r < 24 ? kCsgDifference : kCsgIntersection, parent, 0, level, {}});
  u.levels = std::max(u.levels, level);
  const int chain_side = (int)(rng() % 8 == 0);  // mostly left chains
  u.owed += 2;
  for (int side = 0; side < 2; ++side) {
    if (side == 1) u.nodes[(size_t)me].split = (int)u.leaves.size();  // the right child's first object
    --u.owed;
    // what max_leaves leaves for this side beyond the one leaf it must have
    const int spare = sh.max_leaves - (int)u.leaves.size() - u.owed - 1;
    const int n_kids = rng() % 6 == 0 ? 1 + std::min(std::max(spare, 0), 1 + (int)(rng() % 3)) : 1;
    u.owed += n_kids;
    for (int k = 0; k < n_kids; ++k) {
      --u.owed;
      // (a subtree takes two leaves at least)
      const bool room = level < sh.max_levels && (int)u.leaves.size() + u.owed + 2 <= sh.max_leaves;
      const bool down = sh.chain ? (side == chain_side && k == 0 ? rng() % 16 != 0 : rng() % 12 == 0) : rng() % 5 < 3;
      const int kid = room && down ? grow(u, rng, level + 1, me, sh) : new_leaf(u, rng, me, sh);
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
  bool inl = false, inr = false;
  std::vector<X> out;
  for (const X& x : xs) {
    const bool lhit = (x.key >> kKeyShift) < u.nodes[(size_t)n].split;
    if (csg_allowed(u.nodes[(size_t)n].op, lhit, inl, inr)) out.push_back(x);
    if (lhit) inl = !inl;
    else inr = !inr;
  }
  return out;
}
// `prior`: the hit the caller holds already. `shadow`: only leaves that cast one may be hit.
static Fold fold_literal(const Unit& u, const std::vector<X>& xs, const Fold& prior, bool shadow, int* odd_behind) {
  Fold f = prior;
  std::vector<X> containers;  // (object, at its latest entry)
  size_t hit = xs.size();
  for (size_t i = 0; i < xs.size(); ++i) {
    if (xs[i].t >= 0.0 && (!shadow || u.leaves[(size_t)(xs[i].key >> kKeyShift)].shadow)) {
      hit = i;
      break;
    }
  }
  for (size_t i = 0; i < xs.size() && xs[i].t < 0.0; ++i) {  // (every survivor t < 0 lies before the hit)
    const int obj = xs[i].key >> kKeyShift;
    auto at = std::find_if(containers.begin(), containers.end(), [&](const X& c) { return (c.key >> kKeyShift) == obj; });
    if (at != containers.end()) containers.erase(at);
    else containers.push_back(xs[i]);
  }
  if (odd_behind) *odd_behind = (int)containers.size();
  if (hit < xs.size()) {
    const X& x = xs[hit];
    if (x.t < f.t || (x.t == f.t && x.key < f.key)) {
      f.t = x.t;
      f.key = x.key;
      const int obj = x.key >> kKeyShift;
      f.hin = std::any_of(containers.begin(), containers.end(), [&](const X& c) { return (c.key >> kKeyShift) == obj; });
    }
  }
  if (!shadow)  // the caller's top two by (t, key): of this unit's, the list's last two entries
    for (size_t i = containers.size() > 2 ? containers.size() - 2 : 0; i < containers.size(); ++i)
      push_container(f, containers[i].t, containers[i].key);
  return f;
}

// ---- the stream: csg_deep_eval's loop (rt_device.hpp) with a batch of `cap`
constexpr int kStride = 3;
constexpr uint32_t kCanary = 0xC0FFEE11u;
static Fold eval_stream(const Unit& u, const std::vector<CsgRec>& recs, int cap, const Fold& prior, bool shadow, int* walks) {
  const int nw = ((int)u.nodes.size() + 31) / 32, lw = (u.n_slots + 31) / 32, words = 2 * nw + lw;
  std::vector<uint32_t> buf((size_t)std::max(words, 1) * kStride, kCanary);
  const CsgDeepWords st{buf.data() + 1, (size_t)kStride};  // lane 1 of 3
  Fold f = prior;
  CsgDeepHit dh{f.t, f.key, f.hin};
  CsgDeepTop2 top;
  csg_deep_top2_init(top);
  CsgDeepBatch b;
  *walks = 0;
  for (int pass = 0; pass < (shadow ? 1 : 2); ++pass) {
    if (pass == 1) {
      uint32_t any = 0;
      for (int i = 0; i < lw; ++i) any |= st[2 * nw + i];
      if (!any) break;
    }
    for (int i = 0; i < (pass == 0 ? words : 2 * nw); ++i) st[i] = 0u;
    double wt = -INFINITY;
    int32_t wk = -1;
    for (;;) {
      if (pass == 0) ++*walks;  // (the first pass's: a second pass is no second batch)
      b.xs.n = 0;
      bool more = false;
      for (const Leaf& l : u.leaves) {
        const uint32_t tag = (uint32_t)l.node | (l.slot < 0 ? kCsgDeepTagTri : (uint32_t)l.slot << kCsgDeepTagSlotShift);
        for (const X& x : l.xs) csg_batch_insert(b, cap, x.t, x.key, tag, wt, wk, more);
      }
      CHECK(b.xs.n <= cap);
      bool done = false;
      for (int i = 0; i < b.xs.n && !done; ++i) {
        const double t = b.xs.t[i];
        const int32_t key = b.xs.key[i];
        const uint32_t tag = b.tag[i];
        if (pass == 0) {
          const int r = csg_deep_step(recs.data(), st, nw, t, key, tag,
                                      [&](int32_t k) { return !shadow || u.leaves[(size_t)(k >> kKeyShift)].shadow; }, dh);
          if (r == kCsgDeepTriNeg) {
            if (!shadow) push_container(f, t, key);
          } else {
            done = r == kCsgDeepDone;
          }
        } else if (t < 0.0) {
          csg_deep_note(recs.data(), st, nw, t, key, tag, top);
        } else {
          done = true;
        }
      }
      if (done || !more) break;
      wt = b.xs.t[b.xs.n - 1];
      wk = b.xs.key[b.xs.n - 1];
    }
  }
  f.t = dh.t; f.key = dh.key; f.hin = dh.hin;
  if (!shadow) {
    if (top.k1 >= 0) push_container(f, top.t1, top.k1);
    if (top.k2 >= 0) push_container(f, top.t2, top.k2);
  }
  for (size_t i = 0; i < buf.size(); ++i)
    if (i % kStride != 1) CHECK(buf[i] == kCanary);  // the other lanes' words
  return f;
}

int main() {
  std::mt19937 rng(20261021u);
  const int caps[3] = {1, 7, kCsgListCap};
  long long cases = 0, multi = 0, three_odd = 0, ties = 0, survivors_all = 0, with_hit = 0, with_hin = 0, two_cont = 0;
  long long deep60 = 0, many_nodes = 0, leaves200 = 0, max_roots = 0;
  for (int it = 0; it < 1200; ++it) {
    Unit u;
    Shape sh;
    sh.chain = it % 2 == 0;
    sh.behind = it % 4 < 2;
    sh.max_levels = it % 6 == 0 ? 60 : 5 + (int)(rng() % 56);
    sh.max_leaves = it % 6 == 0 ? 200 : 20 + (int)(rng() % 181);
    grow(u, rng, 1, -1, sh);
    CHECK(u.levels <= 60 && (int)u.leaves.size() <= 200 && (int)u.nodes.size() <= kCsgDeepMaxNodes);
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
    const std::vector<X> ref = eval_nested(u, 0);
    Fold priors[3];
    priors[1].t = 0.5; priors[1].key = 0x7ffffff0;                 // a hit of a later object at a tie
    priors[2].t = 1.25; priors[2].key = 0; priors[2].c1t = -0.3; priors[2].c1k = 5 << 20;  // an earlier object's, with a container
    int odd = 0;
    const Fold want = fold_literal(u, ref, priors[0], false, &odd);
    for (int cap : caps) {
      int walks = 0;
      for (const Fold& p : priors) {
        int wk2 = 0;
        CHECK(eval_stream(u, recs, cap, p, false, &wk2) == fold_literal(u, ref, p, false, nullptr));
        const Fold sw = fold_literal(u, ref, p, true, nullptr), sg = eval_stream(u, recs, cap, p, true, &wk2);
        CHECK(sg.t == sw.t && sg.key == sw.key);
      }
      (void)eval_stream(u, recs, cap, priors[0], false, &walks);
      if (cap == kCsgListCap) multi += walks > 1;  // (the stream itself walked again: more than one batch)
    }
    ++cases;
    survivors_all += (long long)ref.size();
    for (size_t i = 1; i < ref.size(); ++i) ties += ref[i].t == ref[i - 1].t;
    three_odd += odd >= 3;
    with_hit += want.key != 0x7fffffff;
    with_hin += want.hin;
    two_cont += want.c2k >= 0;
    deep60 += u.levels >= 40;
    many_nodes += u.nodes.size() > 64;
    leaves200 += u.leaves.size() >= 150;
    max_roots = std::max<long long>(max_roots, (long long)n_roots);
  }
  CHECK(cases >= 1000 && multi * 5 >= cases && three_odd * 5 >= cases);
  CHECK(survivors_all > 4000 && ties > 500 && with_hit > 300 && with_hin > 50 && two_cont > 200);
  CHECK(deep60 > 20 && many_nodes > 50 && leaves200 > 50);
  std::printf("%s cases=%lld multi_batch=%lld three_odd=%lld survivors=%lld ties=%lld hits=%lld hin=%lld two_containers=%lld "
              "levels40=%lld nodes65=%lld leaves150=%lld max_roots=%lld\n",
              failures ? "FAILED" : "OK", cases, multi, three_odd, survivors_all, ties, with_hit, with_hin, two_cont, deep60,
              many_nodes, leaves200, max_roots);
  return failures ? 1 : 0;
}
