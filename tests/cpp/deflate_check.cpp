// deflate_check — the compressed PNG writers' shared arithmetic (csrc/rt_png_deflate.hpp)
// against serial restatements, on the CPU: built with -fsanitize=address,undefined by
// tests/test_png_deflate.py.
//  - lengths_from_sorted: Fibonacci-like counts (which want 20-bit codes) come out at <= 15
//    bits with a Kraft sum of exactly 1; one used symbol, two, all 286 equal, random counts;
//    every used symbol gets a length; the 7-bit limit of the code-length code.
//  - canonical_codes: prefix-free, and what a decoder that rebuilds the code from the
//    lengths alone reads back.
//  - BitWriter and token_bits: a token stream is read back by a bit-at-a-time inflate of this
//    program's own (dynamic header included).
//  - run_tokens on runs of 1-600 bytes against deflate_rle restated serially, whole and in
//    every split into two parts, and in chunks as the device kernel walks them.
// `deflate_check lens` instead prints dynamic_len and stored_len for filtered bytes it reads.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <utility>
#include <vector>

#include "rt_png_deflate.hpp"

using namespace rtpngz;

static int fails = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      std::printf("FAIL %s: ", #cond);   \
      std::printf(__VA_ARGS__);          \
      std::printf("\n");                 \
      if (++fails > 20) std::exit(1);    \
    }                                    \
  } while (0)

// ---- code lengths
static void check_lengths(const char* what, const std::vector<uint32_t>& count, int max_len) {
  const int n = (int)count.size();
  HuffScratch s;
  std::vector<uint8_t> len(n);
  const int used = sort_used(count.data(), n, s);
  for (int i = 1; i < used; ++i)
    CHECK(s.key[i - 1] < s.key[i] || (s.key[i - 1] == s.key[i] && s.sym[i - 1] < s.sym[i]), "%s: order at %d", what, i);
  std::vector<std::pair<uint32_t, int>> by_count;
  for (int i = 0; i < n; ++i)
    if (count[i]) by_count.push_back({count[i], i});
  lengths_from_sorted(s, used, n, max_len, len.data());
  uint64_t kraft = 0;
  int given = 0;
  for (int i = 0; i < n; ++i) {
    CHECK(len[i] <= max_len, "%s: symbol %d has %d bits", what, i, len[i]);
    if (count[i]) CHECK(len[i] > 0, "%s: used symbol %d has no code", what, i);
    if (len[i]) {
      kraft += 1ull << (max_len - len[i]);
      ++given;
    }
  }
  CHECK(kraft == 1ull << max_len, "%s: Kraft sum %llu / %llu", what, (unsigned long long)kraft, 1ull << max_len);
  CHECK(given == std::max(used, 2), "%s: %d symbols have codes, %d are used", what, given, used);
  // a more frequent symbol never has a longer code
  std::sort(by_count.begin(), by_count.end());
  for (size_t i = 1; i < by_count.size(); ++i)
    CHECK(len[by_count[i - 1].second] >= len[by_count[i].second], "%s: lengths not monotone at %zu", what, i);
  // prefix-free canonical codes (written bit-reversed: compare from bit 0 up)
  std::vector<uint16_t> code(n);
  canonical_codes(len.data(), n, max_len, code.data(), s);
  {  // each symbol's code on its own, as the device builds it
    uint32_t cnt[17] = {}, first[17];
    for (int k = 0; k < n; ++k) ++cnt[len[k]];
    for (int l = 1; l <= max_len; ++l) CHECK(used < 2 || cnt[l] == s.num[l], "%s: %d-bit codes", what, l);
    first_codes(cnt, max_len, first);
    for (int i = 0; i < n; ++i)
      CHECK(canonical_code_at(len.data(), i, first) == code[i], "%s: symbol %d's code on its own", what, i);
  }
  for (int a = 0; a < n; ++a)
    for (int b = 0; b < n; ++b) {
      if (a == b || !len[a] || !len[b] || len[a] > len[b]) continue;
      CHECK((code[b] & ((1u << len[a]) - 1u)) != code[a], "%s: code %d is a prefix of %d", what, a, b);
    }
}

// ---- a bit-at-a-time inflate for one dynamic block followed by the closing stored block
struct BitReader {
  const std::vector<uint8_t>& v;
  uint64_t pos = 0;
  uint32_t bit() {
    if ((pos >> 3) >= v.size()) {
      CHECK(false, "read past the stream");
      std::exit(1);
    }
    const uint32_t b = (v[pos >> 3] >> (pos & 7)) & 1u;
    ++pos;
    return b;
  }
  uint32_t bits(int n) {
    uint32_t r = 0;
    for (int i = 0; i < n; ++i) r |= bit() << i;
    return r;
  }
};
struct Decoder {  // canonical code from lengths alone (RFC 1951 3.2.2), one bit at a time
  std::vector<int> count, symbol;
  explicit Decoder(const std::vector<int>& len) : count(16, 0) {
    for (int l : len) ++count[l];
    count[0] = 0;
    std::vector<int> offs(16, 0);
    for (int i = 1; i < 16; ++i) offs[i] = offs[i - 1] + count[i - 1];
    symbol.resize(len.size());
    for (size_t s = 0; s < len.size(); ++s)
      if (len[s]) symbol[offs[len[s]]++] = (int)s;
  }
  int decode(BitReader& r) const {
    int code = 0, first = 0, index = 0;
    for (int l = 1; l < 16; ++l) {
      code |= (int)r.bit();
      const int c = count[l];
      if (code - c < first) return symbol[index + (code - first)];
      index += c;
      first += c;
      first <<= 1;
      code <<= 1;
    }
    CHECK(false, "no code matches");
    std::exit(1);
  }
};
static std::vector<uint8_t> inflate_segment(const std::vector<uint8_t>& z, bool* final_seen) {
  static const int base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59,
                               67, 83, 99, 115, 131, 163, 195, 227, 258};
  static const int extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
  static const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  BitReader r{z};
  std::vector<uint8_t> out;
  CHECK(r.bits(1) == 0 && r.bits(2) == 2, "a dynamic block that is not final");
  const int hlit = (int)r.bits(5) + 257, hdist = (int)r.bits(5) + 1, hclen = (int)r.bits(4) + 4;
  CHECK(hdist == 1, "one distance code, not %d", hdist);
  std::vector<int> cl(19, 0);
  for (int i = 0; i < hclen; ++i) {
    cl[order[i]] = (int)r.bits(3);
    CHECK(order[i] == (int)cl_order(i), "cl_order(%d)", i);
  }
  const Decoder cld(cl);
  std::vector<int> ll(hlit), dist(1);
  for (int i = 0; i < hlit + hdist; ++i) {
    const int l = cld.decode(r);
    CHECK(l < 16, "no run codes in the header");
    (i < hlit ? ll[i] : dist[0]) = l;
  }
  const Decoder lld(ll);
  for (;;) {
    const int s = lld.decode(r);
    if (s == 256) break;
    if (s < 256) {
      out.push_back((uint8_t)s);
      continue;
    }
    const int len = base[s - 257] + (int)r.bits(extra[s - 257]);
    CHECK(dist[0] == 1 && r.bit() == 0, "the distance code is one zero bit");
    CHECK(!out.empty(), "a match at the start");
    for (int i = 0; i < len; ++i) out.push_back(out.back());
  }
  *final_seen = r.bits(1) == 1;
  CHECK(r.bits(2) == 0, "a stored block closes the segment");
  r.pos = (r.pos + 7) / 8 * 8;
  CHECK(r.bits(16) == 0 && r.bits(16) == 0xffff, "the stored block is empty");
  CHECK(r.pos / 8 == z.size(), "the segment ends after it (%llu of %zu)", (unsigned long long)(r.pos / 8), z.size());
  return out;
}

template <class Fn>
static void for_runs(const std::vector<uint8_t>& F, Fn&& f) {
  for (size_t i = 0; i < F.size();) {
    size_t j = i + 1;
    while (j < F.size() && F[j] == F[i]) ++j;
    f(F[i], (uint32_t)(j - i));
    i = j;
  }
}
// the host encoder's dynamic path on F, restated with the header's pieces
static std::vector<uint8_t> deflate_segment(const std::vector<uint8_t>& F, bool last) {
  uint32_t hist[kHist] = {};
  for_runs(F, [&](uint8_t b, uint32_t L) {
    run_tokens(L, 0, L, [&](uint32_t, uint32_t len) {
      if (!len) ++hist[b];
      else ++hist[len_symbol(len).sym], ++hist[kDistSlot];
    });
  });
  hist[256] = 1;
  HuffScratch s;
  BlockCode c;
  lengths_from_sorted(s, sort_used(hist, kLitLen, s), kLitLen, kMaxBits, c.len);
  finish_code(c, s, hist[kDistSlot] != 0);
  std::vector<uint8_t> z(F.size() * 3 + 600, 0);
  BitWriter w{z.data(), 0};
  put_fixed_head(w, c);
  CHECK(w.pos == fixed_head_bits(c), "fixed_head_bits");
  for (uint32_t k = 0; k <= c.hlit; ++k) w.put(c.cl_code[sent_length(c, k)], c.cl_len[sent_length(c, k)]);
  CHECK(w.pos == c.head_bits, "head_bits %u, written %llu", c.head_bits, (unsigned long long)w.pos);
  for_runs(F, [&](uint8_t b, uint32_t L) {
    run_tokens(L, 0, L, [&](uint32_t, uint32_t len) {
      const TokenBits t = token_bits(c, b, len);
      w.put(t.v, t.n);
    });
  });
  w.put(c.code[256], c.len[256]);
  const uint64_t n = close_dynamic(z.data(), w.pos, last);
  CHECK(n == dynamic_len(w.pos), "dynamic_len");
  z.resize((size_t)n);
  return z;
}

// ---- deflate_rle, serially: (position, length) of every token of a run of L bytes
static std::vector<std::pair<uint32_t, uint32_t>> rle_serial(uint32_t L) {
  std::vector<std::pair<uint32_t, uint32_t>> t;
  uint32_t p = 0;
  while (p < L) {
    const uint32_t left = L - p;
    if (p > 0 && left >= 3) {
      const uint32_t m = std::min(left, 258u);
      t.push_back({p, m});
      p += m;
    } else {
      t.push_back({p, 0});
      ++p;
    }
  }
  return t;
}

// `deflate_check lens`: every line of the standard input is a segment's filtered bytes in hex;
// prints "<dynamic_len> <stored_len>" for each, the two sides of the encoders' decision. It
// labels inputs for tests/test_png_deflate.py's tie canvases; it checks nothing itself.
static int print_lens() {
  char line[4096];
  while (std::fgets(line, sizeof line, stdin)) {
    std::vector<uint8_t> F;
    unsigned v;
    for (const char* p = line; std::sscanf(p, "%2x", &v) == 1; p += 2) F.push_back((uint8_t)v);
    if (F.empty()) continue;
    std::printf("%zu %llu\n", deflate_segment(F, true).size(), (unsigned long long)stored_len(F.size()));
  }
  return fails ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "lens") == 0) return print_lens();
  std::mt19937_64 rng(20240611);
  {  // Fibonacci-like counts: an unlimited code would be 20+ bits deep
    std::vector<uint32_t> fib(286, 0);
    uint32_t a = 1, b = 1;
    for (int i = 0; i < 24; ++i) {
      fib[i * 7 % 286] = a;
      const uint32_t c = a + b;
      a = b;
      b = c;
    }
    check_lengths("fibonacci", fib, kMaxBits);
    std::vector<uint32_t> fib19(19, 0);
    a = b = 1;
    for (int i = 0; i < 16; ++i) {
      fib19[i] = a;
      const uint32_t c = a + b;
      a = b;
      b = c;
    }
    check_lengths("fibonacci, 7 bits", fib19, kMaxClBits);
  }
  {
    std::vector<uint32_t> one(286, 0), two(286, 0), first(286, 0), all(286, 7), ramp(286);
    one[256] = 1;
    two[0] = 5;
    two[256] = 1;
    first[0] = 9;
    for (int i = 0; i < 286; ++i) ramp[i] = (uint32_t)i + 1;
    check_lengths("one symbol", one, kMaxBits);
    check_lengths("symbol 0 alone", first, kMaxBits);
    check_lengths("two symbols", two, kMaxBits);
    check_lengths("all equal", all, kMaxBits);
    check_lengths("ramp", ramp, kMaxBits);
  }
  for (int round = 0; round < 200; ++round) {
    std::vector<uint32_t> c(286, 0);
    const int used = 2 + (int)(rng() % 285), shape = round % 4;
    for (int i = 0; i < used; ++i) {
      const uint32_t v = shape == 0 ? 1 + (uint32_t)(rng() % 4) : shape == 1 ? 1 + (uint32_t)(rng() % 100000)
                         : shape == 2 ? 1u << (rng() % 24) : 1 + (uint32_t)((rng() % 1000) * (rng() % 1000));
      c[rng() % 286] = v;
    }
    c[256] = 1;
    check_lengths("random", c, kMaxBits);
    std::vector<uint32_t> c19(c.begin(), c.begin() + 16);
    c19.resize(19, 0);
    c19[0] += 1;
    check_lengths("random, 7 bits", c19, kMaxClBits);
  }

  // the tokeniser
  for (uint32_t L = 1; L <= 600; ++L) {
    const auto want = rle_serial(L);
    std::vector<std::pair<uint32_t, uint32_t>> got;
    run_tokens(L, 0, L, [&](uint32_t p, uint32_t len) { got.push_back({p, len}); });
    CHECK(got == want, "run of %u bytes", L);
    for (uint32_t cut = 0; cut <= L; cut += (L < 40 ? 1 : 7)) {
      got.clear();
      run_tokens(L, 0, cut, [&](uint32_t p, uint32_t len) { got.push_back({p, len}); });
      run_tokens(L, cut, L + 5, [&](uint32_t p, uint32_t len) { got.push_back({p, len}); });
      CHECK(got == want, "run of %u bytes cut at %u", L, cut);
    }
    for (uint32_t chunk : {1u, 4u, 36u, 100u}) {
      got.clear();
      for (uint32_t lo = 0; lo < L; lo += chunk)
        run_tokens(L, lo, std::min(L, lo + chunk), [&](uint32_t p, uint32_t len) { got.push_back({p, len}); });
      CHECK(got == want, "run of %u bytes in chunks of %u", L, chunk);
    }
  }
  for (uint32_t len = 3; len <= 258; ++len) {
    static const int base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59,
                                 67, 83, 99, 115, 131, 163, 195, 227, 258};
    int s = 28;
    while (base[s] > (int)len) --s;
    const LenSym ls = len_symbol(len);
    CHECK(ls.sym == 257u + s && ls.extra == len - base[s] && ls.extra < (1u << ls.extra_bits) + (ls.extra_bits ? 0 : 1),
          "len_symbol(%u) = %u + %u in %u bits", len, ls.sym, ls.extra, ls.extra_bits);
  }

  // token streams through the bit writer and back
  for (int round = 0; round < 60; ++round) {
    std::vector<uint8_t> F;
    const int kind = round % 6;
    const size_t n = kind == 5 ? 1 : 1 + rng() % 5000;
    while (F.size() < n) {
      const uint8_t b = kind == 0 ? (uint8_t)rng() : (uint8_t)(rng() % (kind == 1 ? 2 : 7));
      size_t run = kind == 0 || kind == 4 ? 1 : 1 + rng() % (kind == 2 ? 700 : 9);
      if (kind == 4 && !F.empty() && F.back() == b) continue;  // (no byte repeats: no match, no distance code)
      while (run-- && F.size() < n) F.push_back(b);
    }
    bool fin = false;
    const std::vector<uint8_t> z = deflate_segment(F, round & 1);
    const std::vector<uint8_t> back = inflate_segment(z, &fin);
    CHECK(back == F, "round %d: %zu bytes in, %zu out", round, F.size(), back.size());
    CHECK(fin == (bool)(round & 1), "round %d: the final bit", round);
  }
  for (uint32_t L : {258u, 259u, 260u, 261u, 262u, 516u, 517u, 518u, 519u, 520u}) {
    std::vector<uint8_t> F(L, 42);
    bool fin = false;
    CHECK(inflate_segment(deflate_segment(F, true), &fin) == F && fin, "a run of %u", L);
  }

  // geometry
  CHECK(rows_per_segment(1) == kSegment / 4 && rows_per_segment(5461) == 1 && rows_per_segment(5462) == 1 &&
            rows_per_segment(5460) == 1 && rows_per_segment(2730) == 2,
        "rows_per_segment");
  CHECK(stored_len(65535) == 65540 && stored_len(65536) == 65546 && stored_len(1) == 6, "stored_len");
  CHECK(bound(1, 1) == 63 + 4 + 5 && bound(30000, 2) == 63 + 2 * (90001 + 10), "bound");

  if (fails) return 1;
  std::printf("OK\n");
  return 0;
}
