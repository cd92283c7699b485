// rt_png_deflate_dev.hip — the compressed PNG writer (rt_png_deflate.hpp) on the device.
//
//  pngz_encode  one block of 256 threads per segment, everything in LDS. It quantises the
//               segment's rows (q255) into the buffer that later holds the file bytes; a wave
//               per row adds up the five filters' costs and writes the winning filtered row
//               into F (the row above the segment is quantised from the canvas again). Each
//               thread then owns `chunk` consecutive bytes of F: it finds the run starts in
//               them, and two scans over the block (the last start before, the first start
//               after) give every thread the whole extent of the runs that cross its chunk,
//               so rtpngz::run_tokens yields exactly the tokens that start in the chunk.
//               Three walks over the chunk: symbol counts (LDS atomics), token bit lengths
//               (scanned over the block into bit offsets), and the tokens' bits ORed into
//               the LDS image of the block. Between the first two, the used symbols are
//               ranked by (count, symbol) in parallel and one lane runs the shared header's
//               code-length routine (its scratch in LDS); the canonical codes and the counts
//               of the header's code lengths are per-symbol work again, and one lane builds
//               the small code of the code lengths. The header's code lengths are written
//               as the tokens are, two per thread. A segment that would not shrink is one stored block. The
//               segment goes to its slot of the staging buffer in words; its length and the
//               two Adler sums of F are left per segment.
//  pngz_scan    one block: segment lengths -> offsets in the IDAT, and the total.
//  pngz_pack    one block per segment: the slot to its final, unaligned offset through an
//               LDS image of rt_png_dev.hip's shape (256 chunks of 36 bytes, right-aligned
//               behind zeros), one 9216-byte tile after another; the CRC register of the
//               segment (Horner over the tiles) moved to the end of the IDAT's blocks.
//  pngz_finish  one block: the head with the IDAT's length, the Adler-32, the IDAT CRC, IEND,
//               and the file's length where the host reads it.
// Nothing is written to the output when the file does not fit its capacity.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rt_png_crc_dev.hpp"
#include "rt_png_deflate_dev.hpp"
#include "rt_quant_dev.hpp"

namespace rtamd {
namespace {

using namespace rtpngz;

constexpr unsigned kTile = kPngBlock * kChunk;  // 9216: the pack kernel's LDS image
constexpr uint32_t kTileShift = crc32_x8n(kTile);

struct Work {  // d_work's layout for n_seg segments
  size_t off, len, part, stage, bytes, slot;
};
inline Work work_layout(uint32_t W, uint32_t H) {
  const size_t n_seg = (size_t)n_segments(W, H);
  Work k{};
  k.slot = ((size_t)stored_len((uint64_t)rows_per_segment(W) * row_len(W)) + 3) & ~(size_t)3;
  k.off = 8;
  k.len = k.off + 8 * n_seg;
  k.part = k.len + 4 * n_seg;
  k.stage = (k.part + 12 * n_seg + 15) & ~(size_t)15;
  k.bytes = k.stage + n_seg * k.slot;
  return k;
}

// inclusive scan of one value per thread; buf (256 words) holds every thread's result after
template <class Op>
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* buf, Op op) {
  const unsigned t = threadIdx.x;
  __syncthreads();  // (buf may still be read from the previous scan)
  buf[t] = v;
  __syncthreads();
  for (unsigned off = 1; off < (unsigned)kPngBlock; off <<= 1) {
    if (t >= off) v = op(buf[t - off], v);
    __syncthreads();
    buf[t] = v;
    __syncthreads();
  }
  return v;
}

// the tokens that start in F[lo, hi): emit(byte, len), len 0 a literal. s_in: the start of
// the run that F[lo] continues; e_out: the first run start at or after hi.
template <class Emit>
__device__ __forceinline__ void walk_chunk(const uint8_t* F, unsigned lo, unsigned hi, unsigned s_in, unsigned e_out,
                                           Emit&& emit) {
  unsigned i = lo, s = s_in;
  while (i < hi) {
    if (i == 0 || F[i] != F[i - 1]) s = i;
    unsigned j = i + 1;
    while (j < hi && F[j] == F[j - 1]) ++j;
    const unsigned e = j < hi ? j : e_out;
    const unsigned byte = F[i];
    run_tokens(e - s, i - s, j - s, [&](uint32_t, uint32_t len) { emit(byte, len); });
    i = j;
  }
}

__device__ __forceinline__ void or_bits(uint32_t* image, uint32_t pos, uint32_t v, uint32_t n) {
  if (n == 0) return;
  const unsigned long long x = (unsigned long long)v << (pos & 31u);
  if ((uint32_t)x) atomicOr(&image[pos >> 5], (uint32_t)x);
  if ((uint32_t)(x >> 32)) atomicOr(&image[(pos >> 5) + 1], (uint32_t)(x >> 32));
}

// `chunk`: bytes of F per thread (a multiple of 4, an odd number of words); the dynamic LDS
// holds F (256 * chunk bytes) and the file image (256 * chunk + 16).
__global__ __launch_bounds__(kPngBlock) void pngz_encode(const double* __restrict__ rgb, unsigned W, unsigned H,
                                                        unsigned rps, unsigned chunk, uint8_t* __restrict__ stage,
                                                        unsigned long long slot, uint32_t* __restrict__ seg_len,
                                                        uint32_t* __restrict__ part) {
  extern __shared__ uint32_t lds[];
  __shared__ uint32_t hist[288];
  __shared__ BlockCode code;
  __shared__ HuffScratch hs;
  __shared__ uint32_t scan[kPngBlock];
  __shared__ uint32_t wave_part[kPngBlock / 64];
  __shared__ uint32_t n_used;
  const unsigned t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  const unsigned cap = kPngBlock * chunk;
  uint8_t* F = (uint8_t*)lds;
  uint32_t* image_w = lds + cap / 4;
  uint8_t* image = (uint8_t*)image_w;
  const unsigned r0 = blockIdx.x * rps, r1 = min(H, r0 + rps), rows = r1 - r0;
  const unsigned n3 = 3u * W, row_bytes = n3 + 1u, n = rows * row_bytes;
  const bool last = r1 == H;

  // the segment's rows, quantised, into the image buffer
  uint8_t* Q = image;
  const double* src = rgb + (size_t)r0 * n3;
  constexpr unsigned kLoads = 4;
  for (unsigned i0 = t; i0 < rows * n3; i0 += kLoads * kPngBlock) {
    double v[kLoads];
#pragma unroll
    for (unsigned j = 0; j < kLoads; ++j) {
      const unsigned i = i0 + j * kPngBlock;
      v[j] = i < rows * n3 ? src[i] : 0.0;
    }
#pragma unroll
    for (unsigned j = 0; j < kLoads; ++j) {
      const unsigned i = i0 + j * kPngBlock;
      if (i < rows * n3) Q[i] = (uint8_t)q255(v[j]);
    }
  }
  for (unsigned i = t; i < 288; i += kPngBlock) hist[i] = 0;
  if (t == 0) n_used = 0;
  __syncthreads();

  // a wave per row: the five costs, then the winning filter's bytes
  for (unsigned y = r0 + wave; y < r1; y += kPngBlock / 64) {
    const uint8_t* cur = Q + (size_t)(y - r0) * n3;
    const uint8_t* upq = y > r0 ? cur - n3 : nullptr;
    const double* upg = y > 0 ? rgb + (size_t)(y - 1) * n3 : nullptr;
    auto up = [&](unsigned x) -> uint32_t { return upq ? upq[x] : upg ? q255(upg[x]) : 0u; };
    uint32_t cost[5] = {0, 0, 0, 0, 0};
    for (unsigned x = lane; x < n3; x += 64) {
      const uint32_t a = x >= 3 ? cur[x - 3] : 0u, b = up(x), c = x >= 3 ? up(x - 3) : 0u;
#pragma unroll
      for (uint32_t k = 0; k < 5; ++k) cost[k] += filter_cost(filtered(k, cur[x], a, b, c));
    }
    uint64_t total[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      uint32_t v = cost[k];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
      total[k] = v;
    }
    const uint32_t type = best_filter(total);
    uint8_t* dst = F + (size_t)(y - r0) * row_bytes;
    if (lane == 0) dst[0] = (uint8_t)type;
    for (unsigned x = lane; x < n3; x += 64) {
      const uint32_t a = x >= 3 ? cur[x - 3] : 0u, b = up(x), c = x >= 3 ? up(x - 3) : 0u;
      dst[1 + x] = (uint8_t)filtered(type, cur[x], a, b, c);
    }
  }
  __syncthreads();
  for (unsigned i = t; i < cap / 4 + 4; i += kPngBlock) image_w[i] = 0;

  // this thread's chunk: run starts, Adler sums
  const unsigned lo = min(t * chunk, n), hi = min(lo + chunk, n);
  uint32_t first = n, lastst = 0, s1 = 0, s2 = 0;
  for (unsigned i = lo; i < hi; ++i) {
    const uint32_t d = F[i];
    if (i == 0 || d != F[i - 1]) {
      if (first == n) first = i;
      lastst = i;
    }
    s1 += d;
    s2 += d * (n - i);  // (< 100 * 255 * 25600: 32 bits hold it)
  }
  block_scan(lastst, scan, [](uint32_t a, uint32_t b) { return a > b ? a : b; });
  const unsigned s_in = t ? scan[t - 1] : 0u;
  // the first start after the chunk: a prefix minimum over the threads in reverse
  {
    __syncthreads();
    scan[kPngBlock - 1 - t] = first;
    __syncthreads();
    const uint32_t mine = scan[t];
    block_scan(mine, scan, [](uint32_t a, uint32_t b) { return a < b ? a : b; });
  }
  const unsigned e_out = t + 1 < (unsigned)kPngBlock ? scan[kPngBlock - 2 - t] : n;
  if (t == 0) hist[256] = 1;
  __syncthreads();

  walk_chunk(F, lo, hi, s_in, e_out, [&](uint32_t byte, uint32_t len) {
    if (len == 0) {
      atomicAdd(&hist[byte], 1u);
    } else {
      atomicAdd(&hist[len_symbol(len).sym], 1u);
      atomicAdd(&hist[kDistSlot], 1u);
    }
  });
  __syncthreads();

  // the used symbols in (count, symbol) order: every symbol finds its own rank
  for (unsigned s = t; s < (unsigned)kLitLen; s += kPngBlock) {
    const uint32_t cnt = hist[s];
    if (!cnt) continue;
    unsigned rank = 0;
    for (unsigned j = 0; j < (unsigned)kLitLen; ++j) {
      const uint32_t o = hist[j];
      rank += (o && (o < cnt || (o == cnt && j < s))) ? 1u : 0u;
    }
    hs.key[rank] = cnt;
    hs.sym[rank] = (uint16_t)s;
    atomicAdd(&n_used, 1u);
  }
  __syncthreads();
  if (t == 0) {  // (the serial part: the minimum-redundancy lengths; hs.num: codes per length)
    lengths_from_sorted(hs, (int)n_used, kLitLen, kMaxBits, code.len);
    first_codes(hs.num, kMaxBits, hs.first);
    code.dist_len = hist[kDistSlot] != 0 ? 1u : 0u;
    code.hlit = 257;
  }
  if (t < 19) hs.cl_count[t] = 0;
  __syncthreads();
  // per symbol: its canonical code, the last length symbol with a code
  for (unsigned s = t; s < (unsigned)kLitLen; s += kPngBlock) {
    code.code[s] = canonical_code_at(code.len, (int)s, hs.first);
    if (s >= 257 && code.len[s]) atomicMax(&code.hlit, s + 1);
  }
  __syncthreads();
  for (unsigned s = t; s <= code.hlit; s += kPngBlock) atomicAdd(&hs.cl_count[sent_length(code, s)], 1u);
  __syncthreads();
  if (t == 0) finish_header(code, hs);
  __syncthreads();

  // bit lengths: the header's code lengths (two per thread), then the tokens
  uint32_t head_mine = 0;
  for (unsigned k = 2 * t; k < 2 * t + 2 && k <= code.hlit; ++k) head_mine += code.cl_len[sent_length(code, k)];
  const uint32_t head_incl = block_scan(head_mine, scan, [](uint32_t a, uint32_t b) { return a + b; });
  uint32_t bits_mine = 0;
  walk_chunk(F, lo, hi, s_in, e_out,
             [&](uint32_t byte, uint32_t len) { bits_mine += token_bits(code, byte, len).n; });
  const uint32_t bits_incl = block_scan(bits_mine, scan, [](uint32_t a, uint32_t b) { return a + b; });
  const uint32_t token_total = scan[kPngBlock - 1];
  const uint32_t eob_at = code.head_bits + token_total, all_bits = eob_at + code.len[256];
  const bool dynamic = dynamic_len(all_bits) < stored_len(n);
  uint32_t out_len;
  if (dynamic) {
    if (t == 0) {
      BitWriter w{image, 0};
      put_fixed_head(w, code);
    }
    __syncthreads();
    uint32_t pos = fixed_head_bits(code) + head_incl - head_mine;
    for (unsigned k = 2 * t; k < 2 * t + 2 && k <= code.hlit; ++k) {
      const uint32_t l = sent_length(code, k);
      or_bits(image_w, pos, code.cl_code[l], code.cl_len[l]);
      pos += code.cl_len[l];
    }
    pos = code.head_bits + bits_incl - bits_mine;
    walk_chunk(F, lo, hi, s_in, e_out, [&](uint32_t byte, uint32_t len) {
      const TokenBits tb = token_bits(code, byte, len);
      or_bits(image_w, pos, tb.v, tb.n);
      pos += tb.n;
    });
    if (t == 0) or_bits(image_w, eob_at, code.code[256], code.len[256]);
    __syncthreads();
    if (t == 0) close_dynamic(image, all_bits, last);
    out_len = (uint32_t)dynamic_len(all_bits);
  } else {  // (one stored block: kPngzSegMax <= 65535)
    if (t == 0) stored_header(0, n, last, image);
    for (unsigned i = t; i < n; i += kPngBlock) image[5 + i] = F[i];
    out_len = n + 5;
  }
  __syncthreads();
  uint32_t* dst = (uint32_t*)(stage + (size_t)blockIdx.x * slot);
  for (unsigned i = t; i < (out_len + 3) / 4; i += kPngBlock) dst[i] = image_w[i];

  s1 = block_reduce<false>(s1 % kAdlerMod, wave_part);
  s2 = block_reduce<false>(s2 % kAdlerMod, wave_part);
  if (t == 0) {
    seg_len[blockIdx.x] = out_len;
    part[3 * blockIdx.x + 1] = s1 % kAdlerMod;
    part[3 * blockIdx.x + 2] = s2 % kAdlerMod;
  }
}

// off[i]: the bytes of the segments before i; *total_len: the file's length
__global__ __launch_bounds__(kPngBlock) void pngz_scan(const uint32_t* __restrict__ seg_len, unsigned n_seg,
                                                      unsigned long long* __restrict__ off,
                                                      unsigned long long* __restrict__ file_len) {
  __shared__ uint32_t scan[kPngBlock];
  const unsigned t = threadIdx.x;
  unsigned long long carry = 0;
  for (unsigned base = 0; base < n_seg; base += kPngBlock) {
    const unsigned i = base + t;
    const uint32_t mine = i < n_seg ? seg_len[i] : 0u;  // (256 segments: below 2^23 bytes)
    const uint32_t incl = block_scan(mine, scan, [](uint32_t a, uint32_t b) { return a + b; });
    if (i < n_seg) off[i] = carry + incl - mine;
    carry += scan[kPngBlock - 1];
  }
  if (t == 0) *file_len = 63 + carry;
}

__global__ __launch_bounds__(kPngBlock) void pngz_pack(const uint8_t* __restrict__ stage, unsigned long long slot,
                                                      const uint32_t* __restrict__ seg_len,
                                                      const unsigned long long* __restrict__ off,
                                                      const unsigned long long* __restrict__ file_len,
                                                      unsigned long long cap, uint8_t* __restrict__ out,
                                                      uint32_t* __restrict__ part) {
  __shared__ uint32_t image_w[kTile / 4];
  __shared__ uint32_t slice[4 * 256];
  __shared__ uint32_t wave_part[kPngBlock / 64];
  if (*file_len > cap) return;
  uint8_t* image = (uint8_t*)image_w;
  const unsigned t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 4; ++k) slice[k * 256 + t] = kCrcSlices.v[k][t];
  const unsigned len = seg_len[blockIdx.x];
  const uint8_t* src = stage + (size_t)blockIdx.x * slot;
  const unsigned long long body = *file_len - 63, at = off[blockIdx.x];
  uint8_t* dst = out + kFirstBlock + at;
  const unsigned tiles = (len + kTile - 1) / kTile, pad = tiles * kTile - len;
  uint32_t acc = 0;
  for (unsigned j = 0; j < tiles; ++j) {
    __syncthreads();  // (the image may still be read from the previous tile)
    for (unsigned p = t; p < kTile; p += kPngBlock) {
      const unsigned q = j * kTile + p;
      image[p] = q >= pad ? src[q - pad] : (uint8_t)0;
    }
    __syncthreads();
    // the tile's segment bytes [b0, b1) to dst: bytes up to an aligned word, words, the rest
    const unsigned z = j == 0 ? pad : 0u, b0 = j * kTile + z - pad, cnt = kTile - z;
    uint8_t* d = dst + b0;
    const uint8_t* im = image + z;
    const unsigned lead = min(cnt, (unsigned)((4u - (unsigned)((uintptr_t)d & 3u)) & 3u));
    const unsigned words = (cnt - lead) / 4u;
    if (t < lead) d[t] = im[t];
    uint32_t* d_w = (uint32_t*)(d + lead);
    for (unsigned i = t; i < words; i += kPngBlock) {
      const uint8_t* p = im + lead + 4u * i;
      d_w[i] = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
    }
    const unsigned done = lead + 4u * words;
    if (t < cnt - done) d[done + t] = im[done + t];
    uint32_t reg = 0;
#pragma unroll
    for (unsigned i = 0; i < kChunk / 4; ++i) {
      const uint32_t v = reg ^ image_w[t * (kChunk / 4) + i];
      reg = slice[3 * 256 + (v & 0xffu)] ^ slice[2 * 256 + ((v >> 8) & 0xffu)] ^ slice[256 + ((v >> 16) & 0xffu)] ^
            slice[v >> 24];
    }
    acc = crc32_mul(acc, kTileShift) ^ reg;
  }
  acc = crc32_mul(acc, kChunkShift.v[kPngBlock - 1 - t]);
  acc = block_reduce<true>(acc, wave_part);
  if (t < 64) acc = crc32_mul(acc, wave_x8n((uint32_t)(body - (at + len))));  // (thread 0's is used)
  if (t == 0) part[3 * blockIdx.x] = acc;
}

// `lead_reg`: the register after "IDAT" 78 01; seg_raw: the raw bytes of a full segment
__global__ __launch_bounds__(kPngBlock) void pngz_finish(const uint32_t* __restrict__ part, unsigned n_seg,
                                                        unsigned long long R, unsigned long long seg_raw,
                                                        uint32_t lead_reg, PngHead head,
                                                        const unsigned long long* __restrict__ file_len,
                                                        unsigned long long cap, uint8_t* __restrict__ out) {
  __shared__ uint32_t wave_part[kPngBlock / 64];
  __shared__ unsigned long long wave_part64[kPngBlock / 64];
  if (*file_len > cap) return;
  const unsigned long long body = *file_len - 63;
  uint32_t reg = 0;
  unsigned long long a = 0, b = 0;
  for (unsigned i = threadIdx.x; i < n_seg; i += kPngBlock) {
    const unsigned long long k1 = min(R, (unsigned long long)(i + 1) * seg_raw);
    reg ^= part[3 * i];
    const unsigned long long s1 = part[3 * i + 1], s2 = part[3 * i + 2];
    a += s1;
    b = (b + s2 + s1 * ((R - k1) % kAdlerMod)) % kAdlerMod;  // every later raw byte adds this segment's sum to b
  }
  reg = block_reduce<true>(reg, wave_part);
  a = block_reduce<false>(a % kAdlerMod, wave_part64);
  b = block_reduce<false>(b, wave_part64);
  uint32_t start = 0;
  if (threadIdx.x < 64) start = crc32_mul(lead_reg, wave_x8n((uint32_t)body));  // (thread 0's is used)
  if (threadIdx.x < kFirstBlock) {
    uint8_t v = head.b[threadIdx.x];
    if (threadIdx.x >= 33 && threadIdx.x < 37) v = (uint8_t)((uint32_t)(6 + body) >> (8 * (36 - threadIdx.x)));
    out[threadIdx.x] = v;
  }
  if (threadIdx.x == 0) {
    const uint32_t adler = (uint32_t)((b + R) % kAdlerMod) << 16 | (uint32_t)((a + 1) % kAdlerMod);
    put_tail(out + kFirstBlock + body, adler, start ^ reg);
  }
}

}  // namespace

size_t pngz_work_bytes(uint32_t W, uint32_t H) { return work_layout(W, H).bytes; }

hipError_t pngz_encode_device(const double* d_rgb, uint32_t W, uint32_t H, uint8_t* d_out, size_t cap, void* d_work,
                              hipStream_t stream, hipEvent_t* marks) {
  if (!pngz_device_encodable(W, H)) return hipErrorInvalidValue;
  auto mark = [&](int k) {
    if (marks) (void)hipEventRecord(marks[k], stream);
  };
  const Work k = work_layout(W, H);
  const unsigned n_seg = (unsigned)n_segments(W, H), rps = rows_per_segment(W);
  const uint64_t seg_raw = (uint64_t)rps * row_len(W);
  // bytes per thread: whole words, an odd number of them (no LDS bank conflict between the
  // threads' walks)
  unsigned chunk = (unsigned)((seg_raw + kPngBlock - 1) / kPngBlock + 3) & ~3u;
  if (chunk % 8 == 0) chunk += 4;
  uint8_t* w = (uint8_t*)d_work;
  unsigned long long* file_len = (unsigned long long*)w;
  unsigned long long* off = (unsigned long long*)(w + k.off);
  uint32_t* seg_len = (uint32_t*)(w + k.len);
  uint32_t* part = (uint32_t*)(w + k.part);
  uint8_t* stage = w + k.stage;
  mark(0);
  hipLaunchKernelGGL(pngz_encode, dim3(n_seg), dim3(kPngBlock), 2 * kPngBlock * chunk + 16, stream, d_rgb, W, H, rps,
                     chunk, stage, (unsigned long long)k.slot, seg_len, part);
  mark(1);
  hipLaunchKernelGGL(pngz_scan, dim3(1), dim3(kPngBlock), 0, stream, (const uint32_t*)seg_len, n_seg, off, file_len);
  mark(2);
  hipLaunchKernelGGL(pngz_pack, dim3(n_seg), dim3(kPngBlock), 0, stream, (const uint8_t*)stage,
                     (unsigned long long)k.slot, (const uint32_t*)seg_len, (const unsigned long long*)off,
                     (const unsigned long long*)file_len, (unsigned long long)cap, d_out, part);
  mark(3);
  const uint8_t lead[6] = {'I', 'D', 'A', 'T', 0x78, 0x01};
  hipLaunchKernelGGL(pngz_finish, dim3(1), dim3(kPngBlock), 0, stream, (const uint32_t*)part, n_seg,
                     (unsigned long long)raw_len(W, H), (unsigned long long)seg_raw, crc32_update(~0u, lead, 6),
                     make_head(W, H), (const unsigned long long*)file_len, (unsigned long long)cap, d_out);
  mark(4);
  return hipGetLastError();
}

}  // namespace rtamd
