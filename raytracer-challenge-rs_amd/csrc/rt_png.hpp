// rt_png.hpp — the arithmetic of the PNG writer (image/png.rs:13-31), shared by the host
// encoder (rt_png.cpp), the device encoder (rt_png_dev.hip) and tests/cpp/png_check.cpp.
// Plain C++: no HIP header is needed to compile it.
//
// The file is an 8-bit RGB PNG whose zlib stream holds *stored* deflate blocks, so every
// byte's position follows from the canvas size alone (DESIGN.md "Output: PNG"):
//   signature (8) | IHDR chunk (25) | IDAT length, "IDAT" (8) | 78 01 |
//   n blocks of [final, LEN, ~LEN (5 bytes), <= 65535 raw bytes] | Adler-32 | IDAT CRC | IEND (12)
// with the raw image being H rows of one filter byte 00 and 3W quantised components.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define RT_PNG_HD __host__ __device__
#else
#define RT_PNG_HD
#endif

namespace rtpng {

constexpr uint32_t kStoredMax = 65535;   // bytes of a stored deflate block
constexpr uint32_t kFirstBlock = 43;     // file offset of the first block header (after 78 01)
constexpr uint32_t kIdatType = 37;       // file offset of "IDAT": where the chunk CRC starts
constexpr uint64_t kIdatMax = 0x7fffffffull;  // a chunk's length field is at most 2^31 - 1

// ---- sizes and positions
RT_PNG_HD inline uint64_t raw_len(uint32_t w, uint32_t h) { return (uint64_t)h * (3ull * w + 1); }
RT_PNG_HD inline uint64_t n_blocks(uint64_t r) { return (r + kStoredMax - 1) / kStoredMax; }
RT_PNG_HD inline uint64_t idat_len(uint64_t r) { return 6 + 5 * n_blocks(r) + r; }
RT_PNG_HD inline uint64_t file_len(uint64_t r) { return 63 + 5 * n_blocks(r) + r; }
// a canvas the format can hold: neither side empty, the IDAT payload within a chunk's length
RT_PNG_HD inline bool encodable(uint32_t w, uint32_t h) {
  if (w == 0 || h == 0 || h > kIdatMax / (3ull * w + 1)) return false;
  return idat_len(raw_len(w, h)) <= kIdatMax;
}
// file offset of raw byte k
RT_PNG_HD inline uint64_t raw_offset(uint64_t k) { return kFirstBlock + 5 * (k / kStoredMax + 1) + k; }
// file offset one past the bytes that belong to raw bytes [0, k): the block header in front
// of raw byte k (when k starts a block) is not among them
RT_PNG_HD inline uint64_t image_end(uint64_t k) { return k == 0 ? kFirstBlock : raw_offset(k - 1) + 1; }
// the five header bytes of the block that starts at raw byte kb (a multiple of 65535) of r
RT_PNG_HD inline void block_header(uint64_t kb, uint64_t r, uint8_t h[5]) {
  const uint64_t left = r - kb;
  const uint32_t len = left > kStoredMax ? kStoredMax : (uint32_t)left;
  h[0] = left <= kStoredMax ? 1 : 0;
  h[1] = (uint8_t)len;
  h[2] = (uint8_t)(len >> 8);
  h[3] = (uint8_t)~len;
  h[4] = (uint8_t)(~len >> 8);
}
RT_PNG_HD inline void put_be32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v;
}

// ---- Adler-32: a = 1 + sum d_i, b = sum of the a's after each byte, both mod 65521
constexpr uint32_t kAdlerMod = 65521;
// 32-bit sums of all-255 bytes stay below 2^32 for this many bytes (zlib's NMAX)
constexpr uint32_t kAdlerNmax = 5552;

RT_PNG_HD inline uint32_t adler32_update(uint32_t adler, const uint8_t* p, size_t n) {
  uint32_t a = adler & 0xffffu, b = adler >> 16;
  while (n) {
    const size_t m = n < kAdlerNmax ? n : kAdlerNmax;
    for (size_t i = 0; i < m; ++i) {
      a += p[i];
      b += a;
    }
    a %= kAdlerMod;
    b %= kAdlerMod;
    p += m;
    n -= m;
  }
  return b << 16 | a;
}
RT_PNG_HD inline uint32_t adler32(const uint8_t* p, size_t n) { return adler32_update(1u, p, n); }
// adler32(A || B) from adler32(A), adler32(B) and len(B): B's bytes each see A's sum a1 - 1
// on top of their own start of 1
RT_PNG_HD inline uint32_t adler32_combine(uint32_t ad1, uint32_t ad2, uint64_t len2) {
  const uint32_t a1 = ad1 & 0xffffu, b1 = ad1 >> 16, a2 = ad2 & 0xffffu, b2 = ad2 >> 16;
  const uint32_t rem = (uint32_t)(len2 % kAdlerMod);
  const uint32_t a = (a1 + a2 + kAdlerMod - 1) % kAdlerMod;
  const uint32_t b = (uint32_t)(((uint64_t)rem * ((a1 + kAdlerMod - 1) % kAdlerMod) + b1 + b2) % kAdlerMod);
  return b << 16 | a;
}

// ---- CRC-32 (reflected, polynomial 0xEDB88320). crc32_update works on the register:
// crc32(M) = ~crc32_update(~0, M). The register after M from the start value s is
// s * x^(8 len(M)) + (the register after M from 0), so registers and finished CRCs
// both combine as crc32_shift(first, len(second)) ^ second.
constexpr uint32_t kCrcPoly = 0xEDB88320u;

RT_PNG_HD constexpr uint32_t crc32_byte(uint32_t reg, uint32_t byte) {
  reg ^= byte;
  for (int k = 0; k < 8; ++k) reg = (reg >> 1) ^ (kCrcPoly & (0u - (reg & 1u)));
  return reg;
}
RT_PNG_HD inline uint32_t crc32_update(uint32_t reg, const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; ++i) reg = crc32_byte(reg, p[i]);
  return reg;
}
RT_PNG_HD inline uint32_t crc32(const uint8_t* p, size_t n) { return ~crc32_update(~0u, p, n); }

// a * b modulo the polynomial; bit 31 is x^0 (the reflected order), so 0x80000000 is 1
RT_PNG_HD constexpr uint32_t crc32_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 31; i >= 0; --i) {
    p ^= b & (0u - ((a >> i) & 1u));
    b = (b >> 1) ^ (kCrcPoly & (0u - (b & 1u)));
  }
  return p;
}
struct Crc32Pow {  // x2n[k] = x^(2^k); x has an order that divides 2^32 - 1, so x^(2^32) = x
  uint32_t x2n[32];
};
constexpr Crc32Pow crc32_pow_table() {
  Crc32Pow t{};
  t.x2n[0] = 0x40000000u;  // x^1
  for (int k = 1; k < 32; ++k) t.x2n[k] = crc32_mul(t.x2n[k - 1], t.x2n[k - 1]);
  return t;
}
// x^(8 n) modulo the polynomial
RT_PNG_HD constexpr uint32_t crc32_x8n(uint64_t n) {
  constexpr Crc32Pow t = crc32_pow_table();
  uint32_t p = 0x80000000u;
  for (int k = 0; k < 61; ++k)
    if ((n >> k) & 1u) p = crc32_mul(t.x2n[(k + 3) & 31], p);
  return p;
}
// the register (or CRC) moved past n further bytes: multiplication by x^(8 n)
RT_PNG_HD inline uint32_t crc32_shift(uint32_t crc, uint64_t n) { return crc32_mul(crc32_x8n(n), crc); }
// crc32(A || B) from crc32(A), crc32(B) and len(B)
RT_PNG_HD inline uint32_t crc32_combine(uint32_t crc1, uint32_t crc2, uint64_t len2) {
  return crc32_shift(crc1, len2) ^ crc2;
}

// ---- the fixed head and tail
struct PngHead {  // file bytes 0..42: signature, IHDR, IDAT's length and type, 78 01
  uint8_t b[44];
};
inline PngHead make_head(uint32_t w, uint32_t h) {
  PngHead hd{};
  const uint8_t sig[8] = {0x89, 0x50, 0x4E, 0x47, 0x0D, 0x0A, 0x1A, 0x0A};
  for (int i = 0; i < 8; ++i) hd.b[i] = sig[i];
  put_be32(hd.b + 8, 13);
  hd.b[12] = 'I'; hd.b[13] = 'H'; hd.b[14] = 'D'; hd.b[15] = 'R';
  put_be32(hd.b + 16, w);
  put_be32(hd.b + 20, h);
  hd.b[24] = 8;  // bit depth
  hd.b[25] = 2;  // colour type: RGB
  hd.b[26] = hd.b[27] = hd.b[28] = 0;  // compression, filter, interlace
  put_be32(hd.b + 29, crc32(hd.b + 12, 17));
  put_be32(hd.b + 33, (uint32_t)idat_len(raw_len(w, h)));
  hd.b[37] = 'I'; hd.b[38] = 'D'; hd.b[39] = 'A'; hd.b[40] = 'T';
  hd.b[41] = 0x78; hd.b[42] = 0x01;
  return hd;
}
// the tail after the last block: Adler-32 of the raw image, the IDAT CRC (which covers
// "IDAT", the payload before the trailer — register `reg` — and the trailer), IEND
RT_PNG_HD inline void put_tail(uint8_t* p, uint32_t adler, uint32_t reg) {
  put_be32(p, adler);
  put_be32(p + 4, ~crc32_update(reg, p, 4));
  const uint8_t iend[12] = {0, 0, 0, 0, 0x49, 0x45, 0x4E, 0x44, 0xAE, 0x42, 0x60, 0x82};
  for (int i = 0; i < 12; ++i) p[8 + i] = iend[i];
}

}  // namespace rtpng
