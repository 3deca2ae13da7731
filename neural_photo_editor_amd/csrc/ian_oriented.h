// ian_oriented.h -- the integer geometry of an oriented placement (npe_ops.oriented_derive / oriented_inside /
// oriented_bbox are the specification).  Plain C++, no HIP: the runtime checks and derives with it on the host, and
// tests/oriented_main.cpp runs it alone under AddressSanitizer and UBSan.
//
// A placement is (cx2, cy2, ax, ay): the square's centre in half pixels of the canvas (pixel X covers [X, X+1), its centre is 2X+1)
// and A = (ax, ay), the canvas displacement per field pixel along the field's x axis in Q16; the field's y axis is B = (-ay, ax).
// L2 = ax*ax + ay*ay in [2^32, 2^40] is a step of 1..16 canvas pixels.  Nothing here shifts a negative value left or overflows
// int64 for ANY int32 input: the range of L2 is decided before anything is multiplied further.
#pragma once
#include <cstdint>

// what the window kernels share with the host (oriented_bbox) is compiled for both sides there; elsewhere this expands to nothing
#if defined(__HIPCC__)
#define IAN_ORIENTED_HD __host__ __device__
#else
#define IAN_ORIENTED_HD
#endif

namespace ian {

constexpr int64_t ORIENTED_L2_MIN = (int64_t)1 << 32, ORIENTED_L2_MAX = (int64_t)1 << 40;

struct OrientedDerived {
  int32_t m;        // 0..4: the gather takes n = 2^m samples per field pixel per axis, the smallest m with 2^(32+2m) >= L2
  int32_t bx, by;   // round(A * 2^36 / L2): field pixels per canvas pixel in Q20, |b| <= 2^20
};

// floor(a / b) for b > 0
IAN_ORIENTED_HD inline int64_t oriented_floor_div(int64_t a, int64_t b) {
  const int64_t q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

// false: L2 outside its range, d untouched
inline bool oriented_derive(int32_t ax, int32_t ay, OrientedDerived* d) {
  const int64_t lim = (int64_t)1 << 20;   // |a| > 2^20 alone puts L2 past 2^40, and its square may not be added to another
  if (ax > lim || ax < -lim || ay > lim || ay < -lim) return false;
  const int64_t L2 = (int64_t)ax * ax + (int64_t)ay * ay;
  if (L2 < ORIENTED_L2_MIN || L2 > ORIENTED_L2_MAX) return false;
  int m = 0;
  while (((int64_t)1 << (32 + 2 * m)) < L2) ++m;
  d->m = m;
  d->bx = (int32_t)oriented_floor_div((int64_t)ax * ((int64_t)1 << 37) + L2, 2 * L2);
  d->by = (int32_t)oriented_floor_div((int64_t)ay * ((int64_t)1 << 37) + L2, 2 * L2);
  return true;
}

// the canvas pixel of one gather sample along one axis: ((c2 << (16+m)) + d) >> (17+m), the shift arithmetic
inline int64_t oriented_sample(int32_t c2, int m, int64_t d) {
  return oriented_floor_div((int64_t)c2 * ((int64_t)1 << (16 + m)) + d, (int64_t)1 << (17 + m));
}

// Whether every gather sample lies on a w x h canvas.  X and Y are monotone in (U, V), U and V odd in -(64n-1) .. 64n-1, so the four
// corner samples decide.  (ax, ay) must have passed oriented_derive, which gave m.
inline bool oriented_inside(int32_t w, int32_t h, int32_t cx2, int32_t cy2, int32_t ax, int32_t ay, int m) {
  const int64_t e = ((int64_t)64 << m) - 1;
  for (int i = 0; i < 4; ++i) {
    const int64_t U = (i & 1) ? e : -e, V = (i & 2) ? e : -e;
    const int64_t X = oriented_sample(cx2, m, U * ax - V * ay), Y = oriented_sample(cy2, m, U * ay + V * ax);
    if (X < 0 || X >= w || Y < 0 || Y >= h) return false;
  }
  return true;
}

// Inclusive pixel bounds that contain every pixel the compose can change: the half extent of the square along either axis is
// 32 * (|ax| + |ay|) / 65536 pixels, rounded up to half pixels; one pixel more covers the rounding of (bx, by), which moves the
// square's rim by less than 0.2 pixels on a canvas of up to 8192 (|dx| * 0.5 + |dy| * 0.5 <= 2^14 in Q21, times a step <= 16).
struct OrientedBox {
  int32_t x0, y0, x1, y1;
};
IAN_ORIENTED_HD inline OrientedBox oriented_bbox(int32_t cx2, int32_t cy2, int32_t ax, int32_t ay) {
  const int64_t aax = ax < 0 ? -(int64_t)ax : ax, aay = ay < 0 ? -(int64_t)ay : ay;
  const int64_t h2 = (aax + aay + 1023) / 1024;
  return OrientedBox{(int32_t)(oriented_floor_div((int64_t)cx2 - h2, 2) - 1), (int32_t)(oriented_floor_div((int64_t)cy2 - h2, 2) - 1),
                     (int32_t)(oriented_floor_div((int64_t)cx2 + h2, 2) + 1), (int32_t)(oriented_floor_div((int64_t)cy2 + h2, 2) + 1)};
}

}  // namespace ian
