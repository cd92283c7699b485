// rt_png_dev.hip — the PNG writer (image/png.rs:13-31) on the device.
//
// The file holds stored deflate blocks (rt_png.hpp), so every byte's offset follows from
// the canvas size and no scan is needed. Two kernels:
//
//  png_encode   one block of 256 threads per *segment* of kPngSegment = 9211 raw bytes
//               (filter bytes and quantised components). The block reads its part of the
//               f64 canvas once, coalesced, quantises it (q255) and builds the segment's
//               file bytes in LDS — the raw bytes plus the 5-byte header of the stored
//               block that starts inside the segment, if one does (a segment is shorter
//               than a stored block, so at most one) — then copies them to their final
//               offset in aligned words. Block 0 also writes the fixed head. Per segment
//               it leaves three words: the CRC register (from 0) of the segment's file
//               bytes, moved past every file byte that follows up to the Adler trailer
//               (times x^(8 * that many bytes)), and the two Adler sums of its raw bytes.
//  png_finish   one block: xors the registers, adds the Adler sums (a segment's sum counts
//               once more for every raw byte after it), writes the Adler-32 trailer, folds
//               its four bytes into the register, writes the IDAT CRC and IEND.
//
// Why 9211: the LDS image is 256 chunks of 36 bytes = 9216, one chunk per thread; a
// segment and a block header just fit, right-aligned, behind zero bytes. Leading
// zero bytes do not change a CRC register started at 0, so every thread's chunk is a full
// 36 bytes (nine words at an odd word stride: no LDS bank conflict) and sits a fixed
// (255 - t) * 36 bytes before the segment's end, whatever the segment's length: its
// register times a constant x^(8 * 36 * (255 - t)) is its share, and the shares xor.
// A chunk's register comes from four 256-entry tables in LDS, a word per step (slicing by
// four). x^(8 n) for the bytes after the segment is a product of up to 32 table entries
// x^(2^k), one per set bit of n: each lane of one wave takes a bit, and five
// shuffle-and-multiply steps give the product (a lane alone would multiply 32 times; the
// first version of png_finish did, per thread, and took as long as png_encode).
// Adler: a thread adds d and d * (raw bytes from d to the segment's end) for its <= 36
// bytes; 36 * 255 * 9211 < 2^27 cannot overflow 32 bits (all-255 is the worst case), and
// the sums are reduced modulo 65521 before the block adds 256 of them (< 2^24).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rt_png_crc_dev.hpp"
#include "rt_png_dev.hpp"
#include "rt_quant_dev.hpp"

namespace rtamd {
namespace {

using namespace rtpng;

constexpr unsigned kImage = kPngBlock * kChunk;    // 9216
static_assert(kPngSegment + 5 <= kImage && kChunk % 4 == 0, "a segment and a block header fit the LDS image");
static_assert((uint64_t)kChunk * 255 * kPngSegment < (1ull << 32), "a thread's Adler sums fit 32 bits");

__global__ __launch_bounds__(kPngBlock) void png_encode(const double* __restrict__ rgb, unsigned W,
                                                       unsigned long long R, PngHead head,
                                                       uint8_t* __restrict__ out, uint32_t* __restrict__ part) {
  __shared__ uint32_t image_w[kImage / 4];
  __shared__ uint32_t slice[4 * 256];
  __shared__ uint32_t wave_part[kPngBlock / 64];
  uint8_t* image = (uint8_t*)image_w;
  const unsigned t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < 4; ++k) slice[k * 256 + t] = kCrcSlices.v[k][t];
  const unsigned long long k0 = (unsigned long long)blockIdx.x * kPngSegment;
  const unsigned n = (unsigned)min((unsigned long long)kPngSegment, R - k0);  // raw bytes here
  // the stored block that starts in [k0, k0 + n), if any: its header sits before raw byte kb
  const unsigned long long kb = (k0 + kStoredMax - 1) / kStoredMax * kStoredMax;
  const bool has_hdr = kb < k0 + n;
  const unsigned hr = has_hdr ? (unsigned)(kb - k0) : 0xffffffffu;
  const unsigned len = n + (has_hdr ? 5u : 0u);  // file bytes here
  const unsigned pad = kImage - len;
  for (unsigned i = t; i < kImage / 4; i += kPngBlock) image_w[i] = 0;
  __syncthreads();

  const unsigned row_len = 3u * W + 1u;
  uint32_t s1 = 0, s2 = 0;
  // kLoads loads in flight per thread: the blocks are few (2-3 per CU for a 1920x1080 frame),
  // so a thread that waited for each load in turn would leave the memory system idle
  constexpr unsigned kLoads = 6;
  static_assert(kChunk % kLoads == 0, "whole batches");
  for (unsigned r0 = t; r0 < n; r0 += kLoads * kPngBlock) {
    double v[kLoads];
#pragma unroll
    for (unsigned j = 0; j < kLoads; ++j) {
      const unsigned r = r0 + j * kPngBlock;
      const unsigned k = (unsigned)k0 + r;  // (R < 2^31: rtpng::encodable)
      const unsigned row = k / row_len, col = k - row * row_len;
      v[j] = 0.0;  // the row's filter byte (col 0) is 00, which is what 0.0 quantises to
      if (r < n && col) v[j] = rgb[(size_t)row * (row_len - 1) + (col - 1)];
    }
#pragma unroll
    for (unsigned j = 0; j < kLoads; ++j) {
      const unsigned r = r0 + j * kPngBlock;
      if (r < n) {
        const unsigned d = q255(v[j]);
        image[pad + r + (r >= hr ? 5u : 0u)] = (uint8_t)d;
        s1 += d;
        s2 += d * (n - r);
      }
    }
  }
  if (has_hdr && t == 0) block_header(kb, R, image + pad + hr);
  __syncthreads();

  // the segment's file bytes to out[f0, f0 + len): bytes up to the first aligned word, whole
  // words, then the bytes left
  const unsigned long long f0 = image_end(k0);
  uint8_t* dst = out + f0;
  const unsigned lead = min(len, (unsigned)((4u - (unsigned)((uintptr_t)dst & 3u)) & 3u));
  const unsigned words = (len - lead) / 4u;
  if (t < lead) dst[t] = image[pad + t];
  uint32_t* dst_w = (uint32_t*)(dst + lead);
  const uint8_t* src = image + pad + lead;
  for (unsigned i = t; i < words; i += kPngBlock) {
    const uint8_t* p = src + 4u * i;
    dst_w[i] = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
  }
  const unsigned done = lead + 4u * words;
  if (t < len - done) dst[done + t] = image[pad + done + t];
  if (blockIdx.x == 0 && t < kFirstBlock) out[t] = head.b[t];

  // the register (from 0) of this thread's nine words, moved to the segment's end
  uint32_t reg = 0;
#pragma unroll
  for (unsigned i = 0; i < kChunk / 4; ++i) {
    const uint32_t v = reg ^ image_w[t * (kChunk / 4) + i];
    reg = slice[3 * 256 + (v & 0xffu)] ^ slice[2 * 256 + ((v >> 8) & 0xffu)] ^ slice[256 + ((v >> 16) & 0xffu)] ^
          slice[v >> 24];
  }
  reg = crc32_mul(reg, kChunkShift.v[kPngBlock - 1 - t]);
  reg = block_reduce<true>(reg, wave_part);
  // ... and past the file bytes between this segment's end and the Adler trailer
  if (t < 64) reg = crc32_mul(reg, wave_x8n((uint32_t)(image_end(R) - (f0 + len))));  // (thread 0's is used)
  s1 = block_reduce<false>(s1 % kAdlerMod, wave_part);
  s2 = block_reduce<false>(s2 % kAdlerMod, wave_part);
  if (t == 0) {
    part[3 * blockIdx.x + 0] = reg;
    part[3 * blockIdx.x + 1] = s1 % kAdlerMod;
    part[3 * blockIdx.x + 2] = s2 % kAdlerMod;
  }
}

// One block. `start`: the register after "IDAT" 78 01 moved past every block (the host's,
// from the size alone).
__global__ __launch_bounds__(kPngBlock) void png_finish(const uint32_t* __restrict__ part, unsigned n_seg,
                                                       unsigned long long R, uint32_t start,
                                                       uint8_t* __restrict__ out) {
  __shared__ uint32_t wave_part[kPngBlock / 64];
  __shared__ unsigned long long wave_part64[kPngBlock / 64];
  uint32_t reg = 0;
  unsigned long long a = 0, b = 0;
  for (unsigned i = threadIdx.x; i < n_seg; i += kPngBlock) {
    const unsigned long long k1 = min(R, (unsigned long long)(i + 1) * kPngSegment);
    reg ^= part[3 * i];
    const unsigned long long s1 = part[3 * i + 1], s2 = part[3 * i + 2];
    a += s1;
    b = (b + s2 + s1 * ((R - k1) % kAdlerMod)) % kAdlerMod;  // every later raw byte adds this segment's sum to b
  }
  reg = block_reduce<true>(reg, wave_part);
  a = block_reduce<false>(a % kAdlerMod, wave_part64);
  b = block_reduce<false>(b, wave_part64);
  if (threadIdx.x == 0) {
    const uint32_t adler = (uint32_t)((b + R) % kAdlerMod) << 16 | (uint32_t)((a + 1) % kAdlerMod);
    put_tail(out + image_end(R), adler, start ^ reg);
  }
}

}  // namespace

hipError_t png_encode_device(const double* d_rgb, uint32_t W, uint32_t H, uint8_t* d_out, uint32_t* d_part,
                             hipStream_t stream) {
  if (!encodable(W, H)) return hipErrorInvalidValue;
  const uint64_t R = raw_len(W, H);
  const unsigned n_seg = (unsigned)png_segments(R);
  hipLaunchKernelGGL(png_encode, dim3(n_seg), dim3(kPngBlock), 0, stream, d_rgb, W, (unsigned long long)R,
                     make_head(W, H), d_out, d_part);
  const uint8_t lead[6] = {'I', 'D', 'A', 'T', 0x78, 0x01};
  const uint32_t start = crc32_shift(crc32_update(~0u, lead, 6), image_end(R) - kFirstBlock);
  hipLaunchKernelGGL(png_finish, dim3(1), dim3(kPngBlock), 0, stream, (const uint32_t*)d_part, n_seg,
                     (unsigned long long)R, start, d_out);
  return hipGetLastError();
}

}  // namespace rtamd
