// rt_png_deflate_dev.hpp — the compressed PNG writer on the device (rt_png_deflate_dev.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rt_png_deflate.hpp"

namespace rtamd {

// A segment's filtered bytes and its file bytes both live in a workgroup's LDS: 256 threads
// with at most 100 bytes each of either, so a row may hold 25600 bytes.
constexpr uint32_t kPngzThreadMax = 100;
constexpr uint32_t kPngzSegMax = 256 * kPngzThreadMax;
constexpr uint32_t kPngzMaxWidth = (kPngzSegMax - 1) / 3;  // 8533
static_assert(rtpngz::kSegment <= kPngzSegMax && kPngzSegMax <= rtpng::kStoredMax,
              "a segment fits the LDS image, and one stored block");

// a canvas the device encoder takes: encodable, a row within the LDS image, and the bound's
// IDAT payload within a chunk's length (the kernels' offsets are then below 2^31)
inline bool pngz_device_encodable(uint32_t W, uint32_t H) {
  return rtpng::encodable(W, H) && W <= kPngzMaxWidth && rtpngz::bound(W, H) - 57 <= rtpng::kIdatMax;
}

// bytes of d_work for a W x H canvas: the file's length (its first 8 bytes, written last),
// per-segment offsets, lengths and checksum words, and the staging slots
size_t pngz_work_bytes(uint32_t W, uint32_t H);

// Encodes the H x W x 3 f64 canvas at d_rgb into d_out (cap bytes) if the file fits, and
// leaves its length in the first 8 bytes of d_work either way. hipErrorInvalidValue for a
// canvas pngz_device_encodable refuses. Stream-ordered; nothing is synchronised. `marks`
// (five events, or NULL): recorded before the first kernel and after each of the four.
hipError_t pngz_encode_device(const double* d_rgb, uint32_t W, uint32_t H, uint8_t* d_out, size_t cap, void* d_work,
                              hipStream_t stream, hipEvent_t* marks = nullptr);

}  // namespace rtamd
