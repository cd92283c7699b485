// rt_png_deflate.cpp — the compressed PNG writer on the host: row filters, run-length
// matches and one dynamic Huffman code per segment (rt_png_deflate.hpp). The segments are
// encoded independently, each into a slot of its own, by the calling thread and helpers
// (as rt_png.cpp's blocks); the caller packs them and combines their checksums.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <new>
#include <thread>
#include <vector>

#include "../../include/rt_render.h"
#include "rt_png_deflate.hpp"
#include "rt_quant.hpp"

namespace {

using namespace rtpng;
using namespace rtpngz;

static_assert(kSegment == RT_PNG_DEFLATE_SEGMENT, "the header's constant is the format's");

struct CrcTable {
  uint32_t t[256];
  CrcTable() {
    for (uint32_t v = 0; v < 256; ++v) t[v] = crc32_byte(0, v);
  }
};
const CrcTable kCrc;

inline uint32_t crc_update(uint32_t reg, const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; ++i) reg = kCrc.t[(reg ^ p[i]) & 0xffu] ^ (reg >> 8);
  return reg;
}

constexpr unsigned kMaxThreads = 16;

struct Segment {
  uint64_t len = 0;  // file bytes
  uint32_t adler = 1, reg = 0;
};

struct DeflateJob {
  const double* rgb = nullptr;
  uint32_t width = 0, height = 0, rps = 1;
  uint64_t n_seg = 0, slot = 0;
  uint8_t* stage = nullptr;
  Segment* seg = nullptr;
  std::atomic<uint64_t> next{0};
  std::atomic<uint64_t> done{0};

  // the rows [r0, r1) filtered into F (quantised rows in q: the row above, then the row)
  void filter_rows(uint32_t r0, uint32_t r1, std::vector<uint8_t>& q, uint8_t* F) const {
    const size_t n3 = (size_t)3 * width;
    uint8_t* up = q.data();
    uint8_t* cur = q.data() + n3;
    auto quantise = [&](uint32_t row, uint8_t* dst) {
      const double* src = rgb + (size_t)row * n3;
      for (size_t x = 0; x < n3; ++x) dst[x] = (uint8_t)rtamd::scale_color_component(src[x]);
    };
    if (r0 == 0) std::memset(up, 0, n3);
    else quantise(r0 - 1, up);
    for (uint32_t y = r0; y < r1; ++y) {
      quantise(y, cur);
      uint64_t cost[5] = {0, 0, 0, 0, 0};
      for (size_t x = 0; x < n3; ++x) {
        const uint32_t a = x >= 3 ? cur[x - 3] : 0u, b = up[x], c = x >= 3 ? up[x - 3] : 0u;
        for (uint32_t k = 0; k < 5; ++k) cost[k] += filter_cost(filtered(k, cur[x], a, b, c));
      }
      const uint32_t type = best_filter(cost);
      uint8_t* dst = F + (size_t)(y - r0) * (n3 + 1);
      dst[0] = (uint8_t)type;
      for (size_t x = 0; x < n3; ++x)
        dst[x + 1] = (uint8_t)filtered(type, cur[x], x >= 3 ? cur[x - 3] : 0u, up[x], x >= 3 ? up[x - 3] : 0u);
      std::swap(up, cur);
    }
  }

  // every maximal run of F[0, n): f(byte, length)
  template <class Fn>
  static void for_runs(const uint8_t* F, size_t n, Fn&& f) {
    for (size_t i = 0; i < n;) {
      size_t j = i + 1;
      while (j < n && F[j] == F[i]) ++j;
      f(F[i], j - i);
      i = j;
    }
  }

  void encode(uint64_t b, std::vector<uint8_t>& q, std::vector<uint8_t>& Fbuf) {
    const uint32_t r0 = (uint32_t)(b * rps), r1 = (uint32_t)std::min<uint64_t>(height, (b + 1) * (uint64_t)rps);
    const size_t n = (size_t)(r1 - r0) * (size_t)row_len(width);
    const bool last = b + 1 == n_seg;
    uint8_t* F = Fbuf.data();
    uint8_t* out = stage + b * slot;
    filter_rows(r0, r1, q, F);

    uint32_t hist[kHist] = {};
    uint64_t extra = 0;
    for_runs(F, n, [&](uint8_t byte, size_t L) {
      // (a run longer than 2^32 - 1 bytes cannot occur: rows are at most 3 * 2^32 bytes but a
      // row starts with its filter byte and `encodable` holds the image below 2^31 bytes)
      run_tokens((uint32_t)L, 0, (uint32_t)L, [&](uint32_t, uint32_t len) {
        if (len == 0) {
          ++hist[byte];
        } else {
          const LenSym ls = len_symbol(len);
          ++hist[ls.sym];
          ++hist[kDistSlot];
          extra += ls.extra_bits;
        }
      });
    });
    hist[256] = 1;
    HuffScratch s;
    BlockCode c;
    const int used = sort_used(hist, kLitLen, s);
    lengths_from_sorted(s, used, kLitLen, kMaxBits, c.len);
    finish_code(c, s, hist[kDistSlot] != 0);
    uint64_t bits = c.head_bits + extra + hist[kDistSlot];
    for (int i = 0; i < kLitLen; ++i) bits += (uint64_t)hist[i] * c.len[i];

    Segment& sg = seg[b];
    if (dynamic_len(bits) < stored_len(n)) {
      std::memset(out, 0, (size_t)dynamic_len(bits));
      BitWriter w{out, 0};
      put_fixed_head(w, c);
      for (uint32_t k = 0; k <= c.hlit; ++k) {
        const uint32_t l = sent_length(c, k);
        w.put(c.cl_code[l], c.cl_len[l]);
      }
      for_runs(F, n, [&](uint8_t byte, size_t L) {
        run_tokens((uint32_t)L, 0, (uint32_t)L, [&](uint32_t, uint32_t len) {
          const TokenBits t = token_bits(c, byte, len);
          w.put(t.v, t.n);
        });
      });
      w.put(c.code[256], c.len[256]);
      sg.len = close_dynamic(out, w.pos, last);
    } else {
      uint8_t* p = out;
      for (size_t k = 0; k < n; k += kStoredMax) {
        stored_header(k, n, last, p);
        const size_t m = std::min<size_t>(kStoredMax, n - k);
        std::memcpy(p + 5, F + k, m);
        p += 5 + m;
      }
      sg.len = (uint64_t)(p - out);
    }
    sg.adler = adler32(F, n);
    sg.reg = crc_update(0, out, (size_t)sg.len);
  }

  void run() {
    std::vector<uint8_t> q, F;
    try {
      q.assign((size_t)6 * width, 0);
      F.assign((size_t)rps * (size_t)row_len(width), 0);
    } catch (...) {
      return;  // (the segments go to the other participants; the caller checks `done`)
    }
    for (uint64_t b; (b = next.fetch_add(1)) < n_seg;) {
      encode(b, q, F);
      done.fetch_add(1, std::memory_order_release);
    }
  }
  void run_on(unsigned t) {
    std::vector<std::thread> pool;
    try {  // nothing may throw across the C ABI: segments whose thread cannot start run here
      for (unsigned k = 1; k < t; ++k) pool.emplace_back([this] { run(); });
    } catch (...) {
    }
    run();
    for (std::thread& th : pool) th.join();
  }
};

}  // namespace

extern "C" {

int rtamd_fail(int code, const char* msg) noexcept;               // rt_api.cpp
int rtamd_png_check(uint32_t width, uint32_t height) noexcept;    // rt_png.cpp

// every segment stored (rt_png_deflate.hpp); 0 for a canvas the format cannot hold
size_t rt_png_deflate_bound(uint32_t width, uint32_t height) {
  return encodable(width, height) ? (size_t)bound(width, height) : 0;
}

int rt_canvas_to_png_deflate(const double* rgb, uint32_t width, uint32_t height, uint8_t* out, size_t cap,
                             size_t* out_len) {
  if (!out_len) return rtamd_fail(RT_ERR_INVALID_ARGUMENT, "null pointer");
  if (const int rc = rtamd_png_check(width, height)) return rc;
  *out_len = (size_t)bound(width, height);
  if (!out) return RT_OK;
  if (!rgb) return rtamd_fail(RT_ERR_INVALID_ARGUMENT, "null pointer");
  DeflateJob j;
  j.rgb = rgb; j.width = width; j.height = height;
  j.rps = rows_per_segment(width);
  j.n_seg = n_segments(width, height);
  j.slot = stored_len((uint64_t)j.rps * row_len(width));
  std::vector<uint8_t> stage;
  std::vector<Segment> seg;
  try {
    stage.resize((size_t)(j.n_seg * j.slot));
    seg.resize((size_t)j.n_seg);
  } catch (...) {
    return rtamd_fail(RT_ERR_HOST, "out of memory (compressed PNG staging buffer)");
  }
  j.stage = stage.data();
  j.seg = seg.data();
  unsigned t = std::thread::hardware_concurrency();
  t = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(std::min(t, kMaxThreads), j.n_seg));
  if (raw_len(width, height) < ((uint64_t)1 << 18)) t = 1;
  j.run_on(t);
  if (j.done.load(std::memory_order_acquire) < j.n_seg)
    return rtamd_fail(RT_ERR_HOST, "out of memory (compressed PNG row buffers)");

  uint64_t body = 0;
  for (const Segment& s : seg) body += s.len;
  if (6 + body > kIdatMax) return rtamd_fail(RT_ERR_INVALID_ARGUMENT, "PNG: the IDAT payload would exceed 2^31 - 1 bytes");
  const size_t len = (size_t)(63 + body);
  *out_len = len;
  if (cap < len) return rtamd_fail(RT_ERR_BUFFER_TOO_SMALL, "PNG buffer too small");
  PngHead hd = make_head(width, height);
  put_be32(hd.b + 33, (uint32_t)(6 + body));
  std::memcpy(out, hd.b, kFirstBlock);
  uint32_t adler = 1, reg = crc_update(~0u, out + kIdatType, kFirstBlock - kIdatType);
  uint8_t* p = out + kFirstBlock;
  const uint64_t seg_raw = (uint64_t)j.rps * row_len(width), raw = raw_len(width, height);
  for (uint64_t b = 0; b < j.n_seg; ++b) {
    std::memcpy(p, j.stage + b * j.slot, (size_t)seg[b].len);
    p += seg[b].len;
    adler = adler32_combine(adler, seg[b].adler, std::min(seg_raw, raw - b * seg_raw));
    reg = crc32_combine(reg, seg[b].reg, seg[b].len);
  }
  put_tail(p, adler, reg);
  return RT_OK;
}

}  // extern "C"
