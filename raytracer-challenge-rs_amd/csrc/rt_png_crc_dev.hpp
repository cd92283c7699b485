// rt_png_crc_dev.hpp — what both device PNG encoders (rt_png_dev.hip, rt_png_deflate_dev.hip)
// share: blocks of 256 threads whose threads each take the CRC register of a 36-byte chunk of
// an LDS image (slicing by four), the constant x^(8 * 36 * j) that moves a chunk's register to
// the image's end, x^(8 n) across a wave, and the block reductions. Every translation unit
// gets its own copy of the tables.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rt_png.hpp"

namespace rtamd {
namespace {

using namespace rtpng;

constexpr int kPngBlock = 256;
constexpr unsigned kChunk = 36;                    // LDS image bytes per thread

struct ChunkShift {  // x^(8 * kChunk * j): the register of a chunk that ends j chunks before the end
  uint32_t v[kPngBlock];
};
constexpr ChunkShift chunk_shift_table() {
  ChunkShift t{};
  const uint32_t step = crc32_x8n(kChunk);
  t.v[0] = 0x80000000u;
  for (int j = 1; j < kPngBlock; ++j) t.v[j] = crc32_mul(t.v[j - 1], step);
  return t;
}
__constant__ ChunkShift kChunkShift = chunk_shift_table();

struct CrcSlices {  // v[k][b]: the register of byte b followed by k zero bytes, from 0
  uint32_t v[4][256];
};
constexpr CrcSlices crc_slice_table() {
  CrcSlices t{};
  for (uint32_t b = 0; b < 256; ++b) {
    t.v[0][b] = crc32_byte(0, b);
    for (int k = 1; k < 4; ++k) t.v[k][b] = crc32_byte(t.v[k - 1][b], 0);
  }
  return t;
}
__constant__ CrcSlices kCrcSlices = crc_slice_table();
__constant__ Crc32Pow kCrcPow = crc32_pow_table();

// x^(8 n), n < 2^32, in lanes 0..31 of the calling wave (all 64 lanes call it): lane k holds
// x^(8 * 2^k) if bit k of n is set, else 1, and five steps multiply the 32 together
__device__ __forceinline__ uint32_t wave_x8n(uint32_t n) {
  const unsigned lane = threadIdx.x & 63u;
  uint32_t f = (lane < 32u && ((n >> lane) & 1u)) ? kCrcPow.x2n[(lane + 3u) & 31u] : 0x80000000u;
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) f = crc32_mul(f, __shfl_xor(f, off, 64));
  return f;
}

// sum (or xor) of one value per thread over the block; every thread gets the result
template <bool kXor, typename T>
__device__ __forceinline__ T block_reduce(T v, T* wave_part) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const T o = __shfl_xor(v, off, 64);
    v = kXor ? (v ^ o) : (v + o);
  }
  __syncthreads();  // (wave_part may still be read from the previous reduction)
  if ((threadIdx.x & 63u) == 0) wave_part[threadIdx.x >> 6] = v;
  __syncthreads();
  T r = wave_part[0];
#pragma unroll
  for (int w = 1; w < kPngBlock / 64; ++w) r = kXor ? (r ^ wave_part[w]) : (r + wave_part[w]);
  return r;
}

}  // namespace
}  // namespace rtamd
