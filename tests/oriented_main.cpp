// Stand-alone driver of csrc/ian_oriented.h for tests/test_canvas_oriented_host.py, built under AddressSanitizer and UBSan: a signed
// overflow or a shift the language does not define, for any int32 input, ends the program.  The arguments are cases of six integers
// each, w h cx2 cy2 ax ay; one line per case:
//   bad                                 L2 = ax*ax + ay*ay outside 2^32 .. 2^40
//   ok m bx by inside x0 y0 x1 y1       oriented_derive, oriented_inside on a w x h canvas (0 / 1), oriented_bbox
#include <cstdio>
#include <cstdlib>

#include "ian_oriented.h"

int main(int argc, char** argv) {
  using namespace ian;
  if (argc < 7 || (argc - 1) % 6 != 0) return 2;
  for (int at = 1; at < argc; at += 6) {
    int32_t v[6];
    for (int i = 0; i < 6; ++i) v[i] = (int32_t)strtol(argv[at + i], nullptr, 10);
    OrientedDerived d;
    if (!oriented_derive(v[4], v[5], &d)) {
      printf("bad\n");
      continue;
    }
    const OrientedBox b = oriented_bbox(v[2], v[3], v[4], v[5]);
    printf("ok %d %d %d %d %d %d %d %d\n", d.m, d.bx, d.by, oriented_inside(v[0], v[1], v[2], v[3], v[4], v[5], d.m) ? 1 : 0, b.x0, b.y0,
           b.x1, b.y1);
  }
  return 0;
}
