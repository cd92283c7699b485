// rt_quant_dev.hpp — the canvas quantiser of both device encoders (rt_ppm_dev.hip, rt_png_dev.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace rtamd {

// scale_color_component (ppm.rs:73-75, png.rs:29-31): round() is half away from zero like
// f64::round; `as u8` saturates and maps NaN to 0.
__device__ __forceinline__ unsigned q255(double v) {
  const double s = round(v * 255.0);
  if (!(s > 0.0)) return 0u;
  if (s >= 255.0) return 255u;
  return (unsigned)s;
}

}  // namespace rtamd
