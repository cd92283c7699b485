// png_check — the PNG writers' shared arithmetic (csrc/rt_png.hpp) against the serial
// definitions, on the CPU: built with -fsanitize=address,undefined by tests/test_png.py.
//  - Adler-32 and CRC-32 of segments, combined over random splits of random buffers
//    (empty segments included), equal the checksums of the whole buffer; an all-255
//    buffer longer than 5552 bytes (where 32-bit Adler sums must have been reduced).
//  - raw_offset / image_end / block_header / file_len against a writer that emits the
//    file byte by byte.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "rt_png.hpp"

using namespace rtpng;

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

// the definitions, one byte at a time
static uint32_t adler_serial(const std::vector<uint8_t>& v) {
  uint64_t a = 1, b = 0;
  for (uint8_t d : v) {
    a = (a + d) % 65521;
    b = (b + a) % 65521;
  }
  return (uint32_t)(b << 16 | a);
}
static uint32_t crc_serial(const std::vector<uint8_t>& v) {
  uint32_t c = 0xFFFFFFFFu;
  for (uint8_t d : v) {
    c ^= d;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
  }
  return ~c;
}

static void check_splits(const std::vector<uint8_t>& buf, std::mt19937_64& rng, int n_cuts) {
  std::vector<size_t> cut{0, buf.size()};
  for (int i = 0; i < n_cuts; ++i) cut.push_back(buf.empty() ? 0 : rng() % (buf.size() + 1));
  if (n_cuts > 1) cut.push_back(cut[2]);  // an empty segment in the middle
  std::sort(cut.begin(), cut.end());
  uint32_t ad = adler32(nullptr, 0), crc = crc32(nullptr, 0), reg = ~0u;
  CHECK(ad == 1 && crc == 0, "empty buffer");
  for (size_t i = 0; i + 1 < cut.size(); ++i) {
    const uint8_t* p = buf.data() + cut[i];
    const size_t n = cut[i + 1] - cut[i];
    ad = adler32_combine(ad, adler32(p, n), n);
    crc = crc32_combine(crc, crc32(p, n), n);
    reg = crc32_shift(reg, n) ^ crc32_update(0, p, n);  // registers combine the same way
  }
  CHECK(ad == adler_serial(buf), "adler of %zu bytes in %zu segments", buf.size(), cut.size() - 1);
  CHECK(crc == crc_serial(buf), "crc of %zu bytes in %zu segments", buf.size(), cut.size() - 1);
  CHECK(~reg == crc_serial(buf), "crc register of %zu bytes", buf.size());
  CHECK(adler32(buf.data(), buf.size()) == adler_serial(buf), "adler32 of %zu bytes", buf.size());
  CHECK(crc32(buf.data(), buf.size()) == crc_serial(buf), "crc32 of %zu bytes", buf.size());
}

// the file of an H x W image of bytes `px`, emitted serially
static std::vector<uint8_t> serial_file(uint32_t w, uint32_t h, const std::vector<uint8_t>& raw) {
  std::vector<uint8_t> f;
  auto be32 = [&](uint32_t v) { for (int s = 24; s >= 0; s -= 8) f.push_back((uint8_t)(v >> s)); };
  auto chunk = [&](const char* kind, const std::vector<uint8_t>& payload) {
    be32((uint32_t)payload.size());
    std::vector<uint8_t> body(kind, kind + 4);
    body.insert(body.end(), payload.begin(), payload.end());
    f.insert(f.end(), body.begin(), body.end());
    be32(crc_serial(body));
  };
  const uint8_t sig[8] = {0x89, 0x50, 0x4E, 0x47, 0x0D, 0x0A, 0x1A, 0x0A};
  f.assign(sig, sig + 8);
  std::vector<uint8_t> ihdr;
  for (int s = 24; s >= 0; s -= 8) ihdr.push_back((uint8_t)(w >> s));
  for (int s = 24; s >= 0; s -= 8) ihdr.push_back((uint8_t)(h >> s));
  const uint8_t rest[5] = {8, 2, 0, 0, 0};
  ihdr.insert(ihdr.end(), rest, rest + 5);
  chunk("IHDR", ihdr);
  std::vector<uint8_t> z{0x78, 0x01};
  for (size_t k = 0; k < raw.size(); k += 65535) {
    const size_t len = std::min<size_t>(65535, raw.size() - k);
    z.push_back(k + len == raw.size() ? 1 : 0);
    z.push_back((uint8_t)len); z.push_back((uint8_t)(len >> 8));
    z.push_back((uint8_t)~len); z.push_back((uint8_t)(~len >> 8));
    z.insert(z.end(), raw.begin() + (std::ptrdiff_t)k, raw.begin() + (std::ptrdiff_t)(k + len));
  }
  const uint32_t ad = adler_serial(raw);
  for (int s = 24; s >= 0; s -= 8) z.push_back((uint8_t)(ad >> s));
  chunk("IDAT", z);
  chunk("IEND", {});
  return f;
}

// the same file through the header's formulas, raw bytes placed in a scrambled order
static void check_layout(uint32_t w, uint32_t h, std::mt19937_64& rng) {
  const uint64_t r = raw_len(w, h);
  CHECK(encodable(w, h), "%u x %u", w, h);
  std::vector<uint8_t> raw((size_t)r);
  for (size_t k = 0; k < raw.size(); ++k) raw[k] = k % (3 * (size_t)w + 1) == 0 ? 0 : (uint8_t)rng();
  const std::vector<uint8_t> want = serial_file(w, h, raw);
  CHECK(file_len(r) == want.size() && idat_len(r) + 57 == want.size(), "%u x %u: length %llu, serial %zu", w, h,
        (unsigned long long)file_len(r), want.size());
  std::vector<uint8_t> got((size_t)file_len(r), 0xEE);
  const PngHead hd = make_head(w, h);
  for (unsigned i = 0; i < kFirstBlock; ++i) got[i] = hd.b[i];
  const size_t stride = 7919;  // every residue in turn: neighbours in the file are written far apart
  for (size_t s = 0; s < stride; ++s)
    for (size_t k = s; k < raw.size(); k += stride) {
      got[(size_t)raw_offset(k)] = raw[k];
      if (k % kStoredMax == 0) block_header(k, r, &got[(size_t)raw_offset(k) - 5]);
    }
  CHECK(image_end(r) + 20 == got.size() && image_end(0) == kFirstBlock, "%u x %u: image_end", w, h);
  for (uint64_t k : {(uint64_t)1, r / 2, r})
    CHECK(image_end(k) == raw_offset(k - 1) + 1, "%u x %u: image_end(%llu)", w, h, (unsigned long long)k);
  const uint32_t reg = crc32_update(~0u, got.data() + kIdatType, (size_t)(image_end(r) - kIdatType));
  put_tail(got.data() + image_end(r), adler32(raw.data(), raw.size()), reg);
  size_t bad = 0, first = 0;
  for (size_t i = 0; i < got.size(); ++i)
    if (got[i] != want[i] && !bad++) first = i;
  CHECK(bad == 0, "%u x %u: %zu bytes differ, the first at %zu", w, h, bad, first);
}

int main() {
  std::mt19937_64 rng(20240607);
  for (size_t n : {(size_t)0, (size_t)1, (size_t)2, (size_t)255, (size_t)5552, (size_t)5553, (size_t)9211, (size_t)65535,
                   (size_t)65536, (size_t)200001}) {
    std::vector<uint8_t> buf(n);
    for (uint8_t& b : buf) b = (uint8_t)rng();
    for (int cuts : {0, 1, 2, 7, 40}) check_splits(buf, rng, cuts);
  }
  {  // all 255: the largest sums; longer than 5552 bytes, in one segment and in many
    std::vector<uint8_t> buf(300 * 901, 255);
    for (int cuts : {0, 1, 3, 64}) check_splits(buf, rng, cuts);
  }
  CHECK(crc32_x8n(0) == 0x80000000u && crc32_mul(0x80000000u, 0x12345678u) == 0x12345678u, "x^0 is the unit");
  CHECK(crc32_shift(crc32_shift(0xDEADBEEFu, 9211), 5) == crc32_shift(0xDEADBEEFu, 9216), "shifts add");
  CHECK(crc32_x8n((uint64_t)1 << 40) == crc32_x8n((uint64_t)1 << 8), "x^(2^43) = x^(2^11): the order of x divides 2^32 - 1");

  const uint32_t sizes[][2] = {{1, 1}, {3, 5}, {771, 28}, {772, 28}, {1542, 28}, {1543, 28}, {2, 21845},
                               {1, 21844}, {1, 21845}, {7, 21846}, {300, 300}, {360, 640}};
  for (const auto& hw : sizes) check_layout(hw[1], hw[0], rng);
  CHECK(!encodable(0, 4) && !encodable(4, 0) && !encodable(26754, 26754) && encodable(26753, 26753) &&
            !encodable(0xFFFFFFFFu, 0xFFFFFFFFu) && !encodable(1, 0xFFFFFFFFu),
        "encodable");
  if (fails) return 1;
  std::printf("OK\n");
  return 0;
}
