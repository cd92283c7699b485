// rt_png.cpp — output side of the path (image/png.rs:13-31): the PNG writer on the host.
// The file's layout and its checksums' arithmetic are in rt_png.hpp; the pixels are
// `(v * 255.0).round() as u8` (png.rs:29-31), the PPM writer's rule (rt_quant.hpp).
#include <algorithm>
#include <atomic>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/rt_render.h"
#include "rt_png.hpp"
#include "rt_quant.hpp"

namespace {

using namespace rtpng;

struct CrcTable {  // crc32_byte of every byte, for a byte-at-a-time register update
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

// The rows in kBlocks contiguous blocks, encoded by the calling thread and up to
// kBlocks - 1 helpers started once (as rt_canvas_to_ppm): every participant takes blocks
// from a counter and writes each block's rows at their final offsets, with the stored-block
// headers that start inside it, and leaves the block's Adler-32 and the CRC register (from
// 0) of its file bytes. Positions depend on the size alone, so one pass does it.
constexpr unsigned kBlocks = 16;

struct PngJob {
  const double* rgb = nullptr;
  uint32_t width = 0, height = 0;
  uint8_t* out = nullptr;
  uint64_t raw = 0;
  uint32_t adler[kBlocks] = {};
  uint32_t reg[kBlocks] = {};
  std::atomic<unsigned> next{0};
  uint32_t r0(unsigned b) const { return (uint32_t)(((uint64_t)height * b) / kBlocks); }
  uint64_t k0(unsigned b) const { return (uint64_t)r0(b) * (3ull * width + 1); }
  void run() {
    const size_t row_len = (size_t)3 * width + 1;
    std::vector<uint8_t> row;
    try {
      row.assign(row_len, 0);
    } catch (...) {
      return;  // (the blocks go to the other participants; run_on's caller checks `done`)
    }
    for (unsigned b; (b = next.fetch_add(1)) < kBlocks;) {
      uint32_t ad = 1;
      uint64_t k = k0(b);
      for (uint32_t j = r0(b); j < r0(b + 1); ++j) {
        const double* src = rgb + (size_t)j * 3 * width;
        for (size_t x = 0; x + 1 < row_len; ++x) row[x + 1] = (uint8_t)rtamd::scale_color_component(src[x]);
        ad = adler32_update(ad, row.data(), row_len);
        for (size_t x = 0; x < row_len;) {  // the row in pieces that end at stored-block ends
          if (k % kStoredMax == 0) block_header(k, raw, out + raw_offset(k) - 5);
          const size_t m = (size_t)std::min<uint64_t>(row_len - x, kStoredMax - k % kStoredMax);
          std::memcpy(out + raw_offset(k), row.data() + x, m);
          x += m;
          k += m;
        }
      }
      adler[b] = ad;
      reg[b] = crc_update(0, out + image_end(k0(b)), (size_t)(image_end(k) - image_end(k0(b))));
      done.fetch_add(1, std::memory_order_release);
    }
  }
  std::atomic<unsigned> done{0};
  // run() on the calling thread and up to `t` - 1 helpers
  void run_on(unsigned t) {
    std::vector<std::thread> pool;
    try {  // nothing may throw across the C ABI: blocks whose thread cannot start run here
      for (unsigned k = 1; k < t; ++k) pool.emplace_back([this] { run(); });
    } catch (...) {
    }
    run();
    for (std::thread& th : pool) th.join();
  }
};

}  // namespace

extern "C" {

int rtamd_fail(int code, const char* msg) noexcept;  // rt_api.cpp

// 63 + 5n + R (rt_png.hpp); 0 for a canvas the format cannot hold
size_t rt_png_size(uint32_t width, uint32_t height) {
  return encodable(width, height) ? (size_t)file_len(raw_len(width, height)) : 0;
}

// the refusal shared by every PNG entry point (RT_OK: encodable)
int rtamd_png_check(uint32_t width, uint32_t height) noexcept {
  if (width == 0) return rtamd_fail(RT_ERR_INVALID_ARGUMENT, "PNG: the canvas has no columns (width 0)");
  if (height == 0) return rtamd_fail(RT_ERR_INVALID_ARGUMENT, "PNG: the canvas has no rows (height 0)");
  if (!encodable(width, height))
    return rtamd_fail(RT_ERR_INVALID_ARGUMENT, "PNG: the IDAT payload would exceed 2^31 - 1 bytes");
  return RT_OK;
}

int rt_canvas_to_png(const double* rgb, uint32_t width, uint32_t height, uint8_t* out, size_t cap,
                     size_t* out_len) {
  if (!out_len) return rtamd_fail(RT_ERR_INVALID_ARGUMENT, "null pointer");
  if (const int rc = rtamd_png_check(width, height)) return rc;
  const uint64_t raw = raw_len(width, height);
  const size_t len = (size_t)file_len(raw);
  *out_len = len;
  if (!out) return RT_OK;
  if (!rgb) return rtamd_fail(RT_ERR_INVALID_ARGUMENT, "null pointer");
  if (cap < len) return rtamd_fail(RT_ERR_BUFFER_TOO_SMALL, "PNG buffer too small");
  const PngHead hd = make_head(width, height);
  std::memcpy(out, hd.b, kFirstBlock);
  unsigned t = std::thread::hardware_concurrency();
  t = std::max(1u, std::min(t, kBlocks));
  if (raw < ((uint64_t)1 << 18) || height < 2 * kBlocks) t = 1;
  PngJob j;
  j.rgb = rgb; j.width = width; j.height = height; j.out = out; j.raw = raw;
  j.run_on(t);
  if (j.done.load(std::memory_order_acquire) < kBlocks)
    return rtamd_fail(RT_ERR_HOST, "out of memory (PNG row buffer)");
  uint32_t adler = 1, reg = crc_update(~0u, out + kIdatType, kFirstBlock - kIdatType);
  for (unsigned b = 0; b < kBlocks; ++b) {
    adler = adler32_combine(adler, j.adler[b], j.k0(b + 1) - j.k0(b));
    reg = crc32_combine(reg, j.reg[b], image_end(j.k0(b + 1)) - image_end(j.k0(b)));
  }
  put_tail(out + image_end(raw), adler, reg);
  return RT_OK;
}

}  // extern "C"
