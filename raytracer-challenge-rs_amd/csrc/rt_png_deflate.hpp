// rt_png_deflate.hpp — the arithmetic of the compressed PNG writer, shared by the host
// encoder (rt_png_deflate.cpp), the device encoder (rt_png_deflate_dev.hip) and
// tests/cpp/deflate_check.cpp. Plain C++: no HIP header is needed to compile it.
//
// The file (DESIGN.md "Output: compressed PNG"): rt_png.hpp's head with the IDAT's actual
// length, 78 01, the segments, the Adler-32 of the filtered image, the IDAT CRC, IEND.
//   filter    every row carries the PNG filter type (None, Sub, Up, Average, Paeth; bpp 3,
//             zeros above row 0) with the least sum of min(b, 256 - b) over its 3W filtered
//             bytes; ties go to the lowest type
//   segment   rows_per_segment(W) whole rows of the filtered image; encoded alone, ends on
//             a byte boundary
//   tokens    zlib's deflate_rle: a maximal run of one byte value is a literal, matches of
//             distance 1 and up to 258 bytes while at least 3 bytes are left, then 1-2 literals
//   code      one dynamic Huffman code per segment (lengths <= 15: minimum redundancy over
//             the symbols sorted by (count, symbol), then the Kraft sum repaired from the
//             deepest level up), one distance code of one bit (none when nothing matches),
//             the code lengths sent plainly (no run codes 16-18) under a <= 7-bit code
//   dynamic   [0, 10 | HLIT HDIST=0 HCLEN | lengths | tokens | EOB] [BFINAL, 00, pad, 00 00 FF FF]
//   stored    the segment in stored blocks of <= 65535 bytes, when the dynamic form would
//             not be smaller; BFINAL sits on the last block of the last segment
#pragma once
#include <cstddef>
#include <cstdint>

#include "rt_png.hpp"

namespace rtpngz {

using rtpng::kStoredMax;

constexpr uint32_t kSegment = 16384;  // RT_PNG_DEFLATE_SEGMENT: raw bytes per segment (a row, if longer)
constexpr int kLitLen = 286;          // literal/length symbols 0..285
constexpr int kDistSlot = 286;        // the histogram's slot for the matches (the one distance symbol)
constexpr int kHist = 287;
constexpr int kMaxBits = 15, kMaxClBits = 7;
constexpr uint32_t kMaxMatch = 258, kMinMatch = 3;

// ---- geometry
RT_PNG_HD inline uint64_t row_len(uint32_t w) { return 3ull * w + 1; }
RT_PNG_HD inline uint32_t rows_per_segment(uint32_t w) {
  const uint64_t r = kSegment / row_len(w);
  return r ? (uint32_t)r : 1u;
}
RT_PNG_HD inline uint64_t n_segments(uint32_t w, uint32_t h) {
  const uint32_t rps = rows_per_segment(w);
  return ((uint64_t)h + rps - 1) / rps;
}
// a segment of n raw bytes as stored blocks
RT_PNG_HD inline uint64_t stored_len(uint64_t n) { return n + 5 * ((n + kStoredMax - 1) / kStoredMax); }
// every segment stored: the most a file can take
RT_PNG_HD inline uint64_t bound(uint32_t w, uint32_t h) {
  const uint64_t rps = rows_per_segment(w), full = h / rps, rest = h % rps;
  return 63 + full * stored_len(rps * row_len(w)) + (rest ? stored_len(rest * row_len(w)) : 0);
}
// a dynamic segment of `bits` bits (block header to end-of-block) and its closing empty block
RT_PNG_HD inline uint64_t dynamic_len(uint64_t bits) { return (bits + 3 + 7) / 8 + 4; }

// ---- filters (PNG specification 9.2): x the byte, a left (3 back), b above, c above left
RT_PNG_HD inline uint32_t paeth(uint32_t a, uint32_t b, uint32_t c) {
  const int p = (int)a + (int)b - (int)c;
  const int pa = p > (int)a ? p - (int)a : (int)a - p;
  const int pb = p > (int)b ? p - (int)b : (int)b - p;
  const int pc = p > (int)c ? p - (int)c : (int)c - p;
  return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
RT_PNG_HD inline uint32_t filtered(uint32_t type, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
  const uint32_t pred = type == 0 ? 0u : type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : paeth(a, b, c);
  return (x - pred) & 0xffu;
}
RT_PNG_HD inline uint32_t filter_cost(uint32_t f) { return f < 256u - f ? f : 256u - f; }
// the type with the least cost; ties go to the lowest
RT_PNG_HD inline uint32_t best_filter(const uint64_t cost[5]) {
  uint32_t best = 0;
  for (uint32_t k = 1; k < 5; ++k)
    if (cost[k] < cost[best]) best = k;
  return best;
}

// ---- tokens
// the length symbol of a match of len bytes (3..258), its extra bits and their value
struct LenSym {
  uint32_t sym, extra_bits, extra;
};
RT_PNG_HD inline LenSym len_symbol(uint32_t len) {
  const uint32_t l = len - kMinMatch;
  if (l < 8) return {257 + l, 0, 0};
  if (len == kMaxMatch) return {285, 0, 0};
  const uint32_t e = (31u - (uint32_t)__builtin_clz(l)) - 2u;
  return {261 + 4 * e + ((l >> e) & 3u), e, l & ((1u << e) - 1u)};
}
// The tokens of a run of L equal bytes that start at the run's positions [pa, pb):
// emit(p, 0) is a literal at p, emit(p, len) a match of len bytes at p. Every part of a
// run can be tokenised without the others.
template <class Emit>
RT_PNG_HD inline void run_tokens(uint32_t L, uint32_t pa, uint32_t pb, Emit&& emit) {
  if (pb > L) pb = L;
  if (L <= kMinMatch) {  // (nothing to match; most runs of a busy image)
    for (uint32_t p = pa; p < pb; ++p) emit(p, 0u);
    return;
  }
  if (pa == 0 && pb > 0) emit(0u, 0u);
  const uint32_t r = L - 1, left = r < kMaxMatch ? r : r % kMaxMatch;
  const uint32_t m_end = L - (left < kMinMatch ? left : 0u);  // the matches cover [1, m_end)
  uint32_t q = pa <= 1 ? 1u : 1u + (pa - 1 + kMaxMatch - 1) / kMaxMatch * kMaxMatch;
  for (; q < pb && q < m_end; q += kMaxMatch) emit(q, m_end - q < kMaxMatch ? m_end - q : kMaxMatch);
  uint32_t p = pa > m_end ? pa : m_end;
  if (p == 0) p = 1;
  for (; p < pb; ++p) emit(p, 0u);
}

// ---- the code
struct HuffScratch {
  uint32_t key[288];      // the used symbols in ascending (count, symbol) order
  uint16_t sym[288];
  uint32_t num[33];       // codes per length
  uint32_t first[17];     // the first code of every length
  uint32_t cl_count[19];  // how often the header sends each code length
};
struct BlockCode {
  uint8_t len[288];    // literal/length code lengths
  uint16_t code[288];  // ... and codes, bit-reversed: the first bit to write is bit 0
  uint8_t cl_len[19];  // the code of the code lengths (symbols 0..15 used)
  uint16_t cl_code[19];
  uint32_t hlit;       // literal/length lengths sent (257..286)
  uint32_t hclen;      // code-length-code lengths sent (4..19)
  uint32_t dist_len;   // 1: matches; 0: none, no distance code
  uint32_t head_bits;  // block header, HLIT/HDIST/HCLEN, both tables
};
RT_PNG_HD inline uint32_t cl_order(uint32_t i) {  // RFC 1951 3.2.7
  return i < 3 ? 16 + i : i == 3 ? 0 : (i & 1u) ? 8 - ((i - 3) >> 1) : 7 + ((i - 2) >> 1);
}

// the symbols with a count, sorted by (count, symbol); the device sorts in parallel instead
RT_PNG_HD inline int sort_used(const uint32_t* count, int n, HuffScratch& s) {
  int used = 0;
  for (int i = 0; i < n; ++i) {
    if (!count[i]) continue;
    int j = used++;
    for (; j > 0 && s.key[j - 1] > count[i]; --j) {  // (equal counts stay in symbol order)
      s.key[j] = s.key[j - 1];
      s.sym[j] = s.sym[j - 1];
    }
    s.key[j] = count[i];
    s.sym[j] = (uint16_t)i;
  }
  return used;
}

// Code lengths <= max_len for the `used` symbols sorted in s, into len[0..n) (0: unused).
// Minimum redundancy in place (Moffat and Katajainen); lengths beyond max_len are cut and
// the Kraft sum repaired by lengthening the deepest shorter codes; the lengths then go to
// the symbols from the most frequent (shortest) down. A single used symbol gets one bit
// and a second symbol another, so that the code is complete.
RT_PNG_HD inline void lengths_from_sorted(HuffScratch& s, int used, int n, int max_len, uint8_t* len) {
  uint32_t* num = s.num;  // codes per length, left for first_codes
  for (int i = 0; i < 33; ++i) num[i] = 0;
  for (int i = 0; i < n; ++i) len[i] = 0;
  if (used == 0) return;
  if (used == 1) {
    len[s.sym[0]] = 1;
    len[s.sym[0] == 0 ? 1 : 0] = 1;
    num[1] = 2;
    return;
  }
  uint32_t* A = s.key;
  A[0] += A[1];
  int root = 0, leaf = 2;
  for (int next = 1; next < used - 1; ++next) {
    if (leaf >= used || A[root] < A[leaf]) {
      A[next] = A[root];
      A[root++] = (uint32_t)next;
    } else {
      A[next] = A[leaf++];
    }
    if (leaf >= used || (root < next && A[root] < A[leaf])) {
      A[next] += A[root];
      A[root++] = (uint32_t)next;
    } else {
      A[next] += A[leaf++];
    }
  }
  A[used - 2] = 0;
  for (int next = used - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
  {  // depths of the internal nodes -> the number of leaves at every depth
    int avail = 1, taken = 0, depth = 0;
    root = used - 2;
    while (avail > 0) {
      while (root >= 0 && (int)A[root] == depth) {
        ++taken;
        --root;
      }
      while (avail > taken) {
        ++num[depth < max_len ? depth : max_len];
        --avail;
      }
      avail = 2 * taken;
      ++depth;
      taken = 0;
    }
  }
  uint32_t total = 0;
  for (int i = max_len; i > 0; --i) total += num[i] << (max_len - i);
  while (total != (1u << max_len)) {
    --num[max_len];
    for (int i = max_len - 1; i > 0; --i)
      if (num[i]) {
        --num[i];
        num[i + 1] += 2;
        break;
      }
    --total;
  }
  int j = used;
  for (int i = 1; i <= max_len; ++i)
    for (uint32_t l = num[i]; l > 0; --l) len[s.sym[--j]] = (uint8_t)i;
}

// canonical codes (RFC 1951 3.2.2): the first code of every length from the number of codes
// of every length (cnt[0] is ignored)
RT_PNG_HD inline void first_codes(const uint32_t* cnt, int max_len, uint32_t* first) {
  uint32_t c = 0, before = 0;
  first[0] = 0;
  for (int b = 1; b <= max_len; ++b) {
    c = (c + before) << 1;
    before = cnt[b];
    first[b] = c;
  }
}
RT_PNG_HD inline uint16_t reversed_code(uint32_t v, uint32_t len) {
  uint32_t r = 0;
  for (uint32_t b = 0; b < len; ++b) r |= ((v >> b) & 1u) << (len - 1 - b);
  return (uint16_t)r;
}
// symbol i's code, bit-reversed, on its own: the first code of its length plus the symbols
// of that length before it
RT_PNG_HD inline uint16_t canonical_code_at(const uint8_t* len, int i, const uint32_t* first) {
  const uint32_t l = len[i];
  if (!l) return 0;
  uint32_t rank = 0;
  for (int j = 0; j < i; ++j) rank += len[j] == l ? 1u : 0u;
  return reversed_code(first[l] + rank, l);
}
// ... and all of them in one pass
RT_PNG_HD inline void canonical_codes(const uint8_t* len, int n, int max_len, uint16_t* code, HuffScratch& s) {
  uint32_t* next = s.first;
  for (int i = 0; i < 17; ++i) s.num[i] = 0;
  for (int i = 0; i < n; ++i) ++s.num[len[i]];
  first_codes(s.num, max_len, next);
  for (int i = 0; i < n; ++i) code[i] = len[i] ? reversed_code(next[len[i]]++, len[i]) : (uint16_t)0;
}

// What the header sends once c.len, c.hlit, c.dist_len and s.cl_count are known: the code of
// the code lengths and the header's size.
RT_PNG_HD inline void finish_header(BlockCode& c, HuffScratch& s) {
  const int used = sort_used(s.cl_count, 19, s);
  lengths_from_sorted(s, used, 19, kMaxClBits, c.cl_len);
  canonical_codes(c.cl_len, 19, kMaxClBits, c.cl_code, s);
  c.hclen = 4;
  for (uint32_t i = 19; i > 4; --i)
    if (c.cl_len[cl_order(i - 1)]) {
      c.hclen = i;
      break;
    }
  uint32_t bits = 3 + 5 + 5 + 4 + 3 * c.hclen;
  for (int i = 0; i < 16; ++i) bits += s.cl_count[i] * c.cl_len[i];
  c.head_bits = bits;
}
// The rest of the block's code once c.len holds the literal/length lengths, serially: the
// codes, what the header sends and its size. (The device does the per-symbol parts in
// parallel with the pieces above.)
RT_PNG_HD inline void finish_code(BlockCode& c, HuffScratch& s, bool has_match) {
  canonical_codes(c.len, kLitLen, kMaxBits, c.code, s);
  c.dist_len = has_match ? 1u : 0u;
  c.hlit = 257;
  for (uint32_t i = kLitLen; i > 257; --i)
    if (c.len[i - 1]) {
      c.hlit = i;
      break;
    }
  for (int i = 0; i < 19; ++i) s.cl_count[i] = 0;
  for (uint32_t i = 0; i < c.hlit; ++i) ++s.cl_count[c.len[i]];
  ++s.cl_count[c.dist_len];
  finish_header(c, s);
}
// bits of the first part of the header: the block's three bits, HLIT, HDIST, HCLEN and the
// code-length code; the lengths follow from bit fixed_head_bits(c) on
RT_PNG_HD inline uint32_t fixed_head_bits(const BlockCode& c) { return 17 + 3 * c.hclen; }

// ---- the bit writer: least significant bit first into a zeroed buffer
struct BitWriter {
  uint8_t* p;
  uint64_t pos;  // in bits
  RT_PNG_HD void put(uint32_t v, uint32_t nbits) {
    uint64_t x = (uint64_t)v << (pos & 7u);
    for (uint64_t i = pos >> 3; x; ++i, x >>= 8) p[i] |= (uint8_t)x;
    pos += nbits;
  }
};
// the header's fixed part (BFINAL 0, BTYPE 10, ...)
RT_PNG_HD inline void put_fixed_head(BitWriter& w, const BlockCode& c) {
  w.put(0u | 2u << 1, 3);
  w.put(c.hlit - 257, 5);
  w.put(0, 5);
  w.put(c.hclen - 4, 4);
  for (uint32_t i = 0; i < c.hclen; ++i) w.put(c.cl_len[cl_order(i)], 3);
}
// the k-th code length the header sends (k == hlit: the distance code's)
RT_PNG_HD inline uint32_t sent_length(const BlockCode& c, uint32_t k) { return k < c.hlit ? c.len[k] : c.dist_len; }
// a token's bits and their number: a literal (len 0) or a match with its one-bit distance
struct TokenBits {
  uint32_t v, n;
};
RT_PNG_HD inline TokenBits token_bits(const BlockCode& c, uint32_t byte, uint32_t len) {
  if (len == 0) return {c.code[byte], c.len[byte]};
  const LenSym ls = len_symbol(len);
  const uint32_t n = c.len[ls.sym];
  return {(uint32_t)c.code[ls.sym] | ls.extra << n, n + ls.extra_bits + 1u};  // (the distance code is 0)
}
// after end-of-block at bit `pos`: the empty stored block; returns the segment's bytes
RT_PNG_HD inline uint64_t close_dynamic(uint8_t* p, uint64_t pos, bool last) {
  if (last) p[pos >> 3] |= (uint8_t)(1u << (pos & 7u));
  uint64_t at = (pos + 3 + 7) / 8;
  p[at] = 0; p[at + 1] = 0; p[at + 2] = 0xff; p[at + 3] = 0xff;
  return at + 4;
}
// the 5-byte header of the stored block that starts at byte kb of a stored segment of n bytes
RT_PNG_HD inline void stored_header(uint64_t kb, uint64_t n, bool last, uint8_t h[5]) {
  const uint64_t left = n - kb;
  const uint32_t len = left > kStoredMax ? kStoredMax : (uint32_t)left;
  h[0] = (last && left <= kStoredMax) ? 1 : 0;
  h[1] = (uint8_t)len;
  h[2] = (uint8_t)(len >> 8);
  h[3] = (uint8_t)~len;
  h[4] = (uint8_t)(~len >> 8);
}

}  // namespace rtpngz
