// OpenCV 4.x resize(): the source coordinate of output index d of an axis n_in -> n_out and its cvFloor split, as
// resizeGeneric_'s table loop computes them (imgproc/src/resize.cpp).  Shared by attwarp_lanczos4_coeffs and
// attwarp_cubic_coeffs (HOST).
#pragma once
#include <cmath>

namespace attwarp {

// -> fractional part (float32); *s: the integer source index (taps are placed relative to it)
inline float resize_source_coord(int n_in, int n_out, int d, int* s) {
  const double inv = (double)n_out / n_in, scale = 1. / inv;
  float f = (float)((d + 0.5) * scale - 0.5);
  *s = (int)std::floor(f);          // cvFloor
  f -= *s;
  return f;
}

}  // namespace attwarp
