// rt_quant.hpp — the canvas quantiser of both writers (image/ppm.rs:73-75, image/png.rs:29-31),
// host side (rt_ppm.cpp, rt_png.cpp).
#pragma once

namespace rtamd {

// `(value * 255.0).round() as u8` — C round() is half away
// from zero like f64::round; the `as u8` cast saturates and maps NaN to 0.
// round(s) for 0 < s < 254.5 without a libm call: the truncating conversion
// is exact there, and so is s - trunc(s), so `frac >= 0.5` is round's
// half-away-from-zero rule exactly.
inline unsigned scale_color_component(double v) {
  const double s = v * 255.0;
  if (!(s >= 0.5)) return 0;  // also NaN (as u8: 0) and everything that rounds to <= 0
  if (s >= 254.5) return 255;
  const unsigned i = (unsigned)s;
  return i + (s - (double)i >= 0.5 ? 1u : 0u);
}

}  // namespace rtamd
