// rt_png_dev.hpp — the PNG writer on the device (rt_png_dev.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rt_png.hpp"

namespace rtamd {

// Raw bytes (filter bytes and components) encoded by one block of the kernel.
constexpr uint32_t kPngSegment = 9211;

inline uint64_t png_segments(uint64_t raw) { return (raw + kPngSegment - 1) / kPngSegment; }
// words of d_part for a raw image of `raw` bytes: three per segment
inline size_t png_part_words(uint64_t raw) { return (size_t)(3 * png_segments(raw)); }

// Encodes the H x W x 3 f64 canvas at d_rgb into d_out, which holds
// rtpng::file_len(raw_len(W, H)) bytes; d_part: png_part_words() words of scratch.
// hipErrorInvalidValue for a canvas the format cannot hold (rtpng::encodable).
// Stream-ordered; nothing is synchronised.
hipError_t png_encode_device(const double* d_rgb, uint32_t W, uint32_t H, uint8_t* d_out, uint32_t* d_part,
                             hipStream_t stream);

}  // namespace rtamd
